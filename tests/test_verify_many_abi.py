"""CPU-side checks of the many-proof verify surface: both libraries export the new entry points
with the prototypes the Python bindings declare, the headers declare them, and the two ABI versions
are the ones that introduced them (no device calls)."""

import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIP_NEW = ("eon_multi_pairing_many", "eon_kzg_verify_batch_many", "eon_air_eval_at_points_dev")
PROVE_NEW = ("eon_verify_air_many", "eon_verify_air_many_fs", "eon_verify_many_detail",
             "eon_verify_many_opening_challenges")


def prototype(header, name):
    """(return type, number of parameters) of `name` as the header declares it"""
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?[ *]+)" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{header} does not declare {name}"
    return " ".join(m.group(1).split()), len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])


@pytest.fixture(scope="module")
def libs():
    from plonky3_eon_amd import _lib, native

    if not _lib.LIB_PATH.exists() or not native.PROVE_LIB_PATH.exists():
        pytest.skip("libraries not built (run __graft_entry__.build())")
    return _lib, native, _lib.load(), native.load()


def test_abi_versions(libs):
    _lib, native, hip, prove = libs
    assert hip.eon_abi_version() == 16 == _lib.ABI_VERSION
    assert prove.eon_prove_abi_version() == 11


@pytest.mark.parametrize("name", HIP_NEW)
def test_hip_library_exports_the_declared_prototype(libs, name):
    _lib, _, hip, _ = libs
    ret, n_args = prototype("eon.h", name)
    res, args = _lib.SIGNATURES[name]
    assert ret == "int" and res is ctypes.c_int
    assert len(args) == n_args
    fn = getattr(hip, name)
    assert fn.restype is res and list(fn.argtypes) == list(args)


@pytest.mark.parametrize("name", PROVE_NEW)
def test_prove_library_exports_the_declared_prototype(libs, name):
    _, native, _, prove = libs
    ret, n_args = prototype("eon_prove.h", name)
    res, args = native.SIGNATURES[name]
    assert (ret, res) in (("int", ctypes.c_int), ("const char*", ctypes.c_char_p), ("const char *", ctypes.c_char_p))
    assert len(args) == n_args
    fn = getattr(prove, name)
    assert fn.restype is res and list(fn.argtypes) == list(args)


def test_segment_offsets_are_64_bit():
    """The offsets of both segmented calls are uint64_t, as the counts of the single calls."""
    text = (ROOT / "include" / "eon.h").read_text()
    for name in HIP_NEW[:2]:
        decl = text[text.index(f"int {name}("):]
        assert "const uint64_t* seg, uint32_t nseg" in " ".join(decl[:decl.index(";")].split())


def test_null_handles_are_refused_without_a_device(libs):
    _lib, _, hip, prove = libs
    assert hip.eon_multi_pairing_many(None, None, None, None, 0, None) == _lib.EON_E_ARG
    assert hip.eon_kzg_verify_batch_many(None, None, None, None, None, None, 0, None, None) == _lib.EON_E_ARG
    assert hip.eon_air_eval_at_points_dev(None, None, 0, None, None, None, None, 0, None, None, 0, None) == _lib.EON_E_ARG
    assert prove.eon_verify_air_many(None, None, None, 0, None, 0, 0, 0, None, None, 0, None, None, None, None,
                                     None) == _lib.EON_E_ARG
    assert prove.eon_verify_many_detail(None, 0) is None
