"""CPU: the proof container (include/eon_prove.h "proof bytes") without a GPU.

* tests/golden/proof_fib8_fs.bin / .npz: the FibonacciAir n = 8 proof (publics 0, 1, 21; SRS alpha =
  12345, max_degree 1024; Fiat-Shamir with the challenger Perm::new_from_rng(4, 22, SmallRng(1)); the
  per-column opening) as Proof.to_bytes wrote it and as the arrays prove_native returned.  The
  Python mirror (tests/mirror_proofio.py) parses the bytes into exactly those arrays and writes them
  back; eon_proof_serialize -- host only, libeonprove.so loads without a GPU -- does the same.
* eon_proof_peek's rejections, each with its reason, and the mirror's agreement.
* tests/proofio_check.cpp under AddressSanitizer and UBSan: mutated headers never make peek read
  outside the buffer or accept a length that is not the shape's.

Every comparison is exact."""

import ctypes
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mirror_proofio as M

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def golden():
    data = (GOLDEN / "proof_fib8_fs.bin").read_bytes()
    with np.load(GOLDEN / "proof_fib8_fs.npz") as z:
        arrays = {k: z[k] for k in z.files}
    shape = {k: int(arrays.pop(k)) for k in ("flags", "degree_bits", "width", "chunks", "pre_width", "perm_width")}
    return data, shape, arrays


@pytest.fixture(scope="module")
def plib():
    from plonky3_eon_amd import _lib, native

    if not _lib.LIB_PATH.exists() or not native.PROVE_LIB_PATH.exists():
        pytest.skip("libraries not built (run __graft_entry__.build())")
    return native.load()


def c_shape(s):
    from plonky3_eon_amd.native import eon_proof_shape

    return eon_proof_shape(s["flags"], s["degree_bits"], s["width"], s["chunks"], s["pre_width"], s["perm_width"])


def test_golden_is_the_fibonacci_proof(golden):
    data, shape, arrays = golden
    assert shape == dict(flags=0, degree_bits=3, width=2, chunks=1, pre_width=0, perm_width=0)
    assert len(data) == 48 + 32 * (3 + 5 + 5) == M.size(shape)
    assert arrays["trace_witnesses"].shape == (2, 2, 8) and arrays["trace_opened"].shape == (2, 2, 4)


def test_mirror_parses_the_golden_bytes_into_the_golden_arrays(golden):
    data, shape, arrays = golden
    s, a = M.parse(data)
    assert s == shape and sorted(a) == sorted(arrays)
    for k in arrays:
        assert a[k].dtype == arrays[k].dtype == np.uint64 and a[k].shape == arrays[k].shape, k
        np.testing.assert_array_equal(a[k], arrays[k], err_msg=k)


def test_mirror_writer_reproduces_the_golden_bytes(golden):
    data, shape, arrays = golden
    assert M.write(shape, arrays) == data


def serialize(plib, shape, arrays, cap=None):
    from plonky3_eon_amd.native import _proof_lk

    a = {short: np.ascontiguousarray(arrays[name], dtype=np.uint64) for short, name in (
        ("tc", "trace_commit"), ("qc", "quotient_commit"), ("to", "trace_opened"), ("tw", "trace_witnesses"),
        ("qo", "quotient_opened"), ("qw", "quotient_witnesses"), ("po", "preprocessed_opened"),
        ("pw", "preprocessed_witnesses"), ("mc", "permutation_commit"), ("mo", "permutation_opened"),
        ("mw", "permutation_witnesses")) if name in arrays}
    lk = _proof_lk(a, shape["degree_bits"])
    cs = c_shape(shape)
    size = plib.eon_proof_bytes_size(ctypes.byref(cs))
    cap = size if cap is None else cap
    out = np.zeros(max(cap, 1), np.uint8)
    written = ctypes.c_uint64(0)
    rc = plib.eon_proof_serialize(ctypes.byref(lk), ctypes.byref(cs), out.ctypes.data_as(ctypes.c_void_p), cap,
                                  ctypes.byref(written))
    return rc, out[:written.value].tobytes() if rc == 0 else b"", written.value


def test_eon_proof_serialize_reproduces_the_golden_bytes(plib, golden):
    from plonky3_eon_amd import _lib

    data, shape, arrays = golden
    cs = c_shape(shape)
    assert plib.eon_proof_bytes_size(ctypes.byref(cs)) == len(data)
    rc, out, written = serialize(plib, shape, arrays)
    assert rc == 0 and written == len(data) and out == data
    # a buffer one byte too small is refused and told the size; an opened value >= r is not written
    rc, _, written = serialize(plib, shape, arrays, cap=len(data) - 1)
    assert rc == _lib.EON_E_SHAPE and written == len(data)
    bad = dict(arrays, quotient_opened=np.array([M.limbs(M.R)], dtype=np.uint64))
    assert serialize(plib, shape, bad)[0] == _lib.EON_E_ARG


def test_bytes_size_is_the_mirrors_and_zero_on_an_invalid_shape(plib):
    m = 0xFFFFFFFF
    for s in (dict(flags=0, degree_bits=3, width=2, chunks=1, pre_width=0, perm_width=0),
              dict(flags=1, degree_bits=3, width=60, chunks=2, pre_width=0, perm_width=0),
              dict(flags=7, degree_bits=4, width=5, chunks=4, pre_width=2, perm_width=1),
              dict(flags=6, degree_bits=20, width=1312, chunks=2, pre_width=3, perm_width=9),
              dict(flags=7, degree_bits=0, width=m, chunks=m, pre_width=m, perm_width=m),
              dict(flags=8, degree_bits=3, width=2, chunks=1, pre_width=0, perm_width=0),
              dict(flags=0, degree_bits=3, width=2, chunks=1, pre_width=1, perm_width=0),
              dict(flags=4, degree_bits=3, width=2, chunks=1, pre_width=0, perm_width=0)):
        cs = c_shape(s)
        assert plib.eon_proof_bytes_size(ctypes.byref(cs)) == M.size(s), s
    assert M.size(dict(flags=8, degree_bits=3, width=2, chunks=1, pre_width=0, perm_width=0)) == 0


def peek(plib, data):
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.native import eon_proof_io_report, eon_proof_shape
    from plonky3_eon_amd.proof import ProofFormatError

    buf = np.frombuffer(data, dtype=np.uint8)
    shape, rep = eon_proof_shape(), eon_proof_io_report()
    rc = plib.eon_proof_peek(buf.ctypes.data_as(ctypes.c_void_p) if buf.size else None, buf.size, ctypes.byref(shape),
                             ctypes.byref(rep))
    if rc == 0:
        assert rep.reason == 0
        return {k: getattr(shape, k) for k, _ in eon_proof_shape._fields_}
    assert rc == _lib.EON_E_FORMAT and rep.section == 0 and rep.index == 0
    return ProofFormatError.REASONS[rep.reason]


def patched(data, offset, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


def test_peek_accepts_the_golden_and_rejects_each_header_fault(plib, golden):
    data, shape, _ = golden
    assert peek(plib, data) == shape == M.peek(data)
    cases = {
        "wrong magic": (patched(data, 6, "<B", ord("2")), "MAGIC"),
        "version 2": (patched(data, 8, "<I", 2), "VERSION"),
        "flag bit 3": (patched(data, 12, "<I", 8), "FLAGS"),
        "Wp != 0 with its flag clear": (patched(data, 28, "<I", 1), "FLAGS"),
        "Wq == 0 with its flag set": (patched(data, 12, "<I", 4), "FLAGS"),
        "reserved word": (patched(data, 36, "<I", 1), "FLAGS"),
        "one byte short": (data[:-1], "LENGTH"),
        "one byte long": (data + b"\0", "LENGTH"),
        "stated length one more": (patched(data, 40, "<Q", len(data) - 48 + 1), "LENGTH"),
        # W = 2^31 with the true body: the shape's length is 5 * 2^36 bytes more than the buffer has --
        # rejected from the header alone, with nothing allocated
        "W = 2^31": (patched(data, 20, "<I", 1 << 31), "LENGTH"),
        "shorter than a header": (data[:47], "LENGTH"),
        "empty": (b"", "LENGTH"),
    }
    for what, (bad, reason) in cases.items():
        assert peek(plib, bad) == reason, what
        with pytest.raises(M.Rejected) as e:
            M.peek(bad)
        assert e.value.reason == reason, what


def test_python_peek_and_format_error(plib, golden):
    from plonky3_eon_amd.native import proof_peek
    from plonky3_eon_amd.proof import ProofFormatError, VerificationError

    data, shape, _ = golden
    s = proof_peek(data)
    assert (s.flags, s.degree_bits, s.width, s.chunks, s.pre_width, s.perm_width) == (0, 3, 2, 1, 0, 0)
    with pytest.raises(ProofFormatError) as e:
        proof_peek(data + b"\0")
    assert (e.value.reason, e.value.section, e.value.index) == ("LENGTH", "HEADER", 0)
    assert not issubclass(ProofFormatError, VerificationError)
    assert ProofFormatError.SECTIONS == M.SECTIONS


def test_mirror_element_rules(golden):
    """the mirror's own rejections, on mutated copies of the golden bytes (the device's are in
    tests/test_gpu_proof_io.py)"""
    data, shape, _ = golden

    def put(section, index, b32):
        at = M.offset_of(shape, section, index)
        return data[:at] + b32 + data[at + 32:]

    x = next(x for x in range(1, 100) if pow(x**3 + 3, (M.Q - 1) // 2, M.Q) == M.Q - 1)  # x^3 + 3 is no square
    for bad, want in ((put("TRACE_NEXT", 1, M.R.to_bytes(32, "little")), ("FR_NOT_CANONICAL", "TRACE_NEXT", 1)),
                      (put("QUOTIENT_WITNESS", 0, M.Q.to_bytes(32, "little")),
                       ("G1_NOT_CANONICAL", "QUOTIENT_WITNESS", 0)),
                      (put("TRACE_COMMIT", 1, bytes(31) + b"\x41"), ("G1_ENCODING", "TRACE_COMMIT", 1)),
                      (put("TRACE_WITNESS_NEXT", 0, x.to_bytes(32, "little")),
                       ("G1_NOT_ON_CURVE", "TRACE_WITNESS_NEXT", 0))):
        with pytest.raises(M.Rejected) as e:
            M.parse(bad)
        assert (e.value.reason, e.value.section, e.value.index) == want
    # the identity is an element like any other
    s, a = M.parse(put("TRACE_WITNESS_ZETA", 0, bytes(31) + b"\x40"))
    assert not a["trace_witnesses"][0, 0].any()
    assert M.write(s, a) == put("TRACE_WITNESS_ZETA", 0, bytes(31) + b"\x40")


def test_header_parser_under_the_sanitizers(tmp_path):
    """tests/proofio_check.cpp: 2000 single-byte header mutations per shape, every buffer an exactly
    sized heap block, AddressSanitizer and UBSan on"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "proofio_check"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(ROOT / "plonky3_eon_amd" / "host"), str(ROOT / "tests" / "proofio_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    p = subprocess.run([str(exe), "2000"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    word, cases, accepted, rejected = p.stdout.split()
    assert word == "ok" and int(cases) == int(accepted) + int(rejected) and int(cases) >= 3 * 2000
    assert int(accepted) >= 3  # the unchanged buffers; a mutation of degree_bits is accepted too
