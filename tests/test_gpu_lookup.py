"""LogUp lookups on the GPU, bit-exact against the CPU restatement (tests/mirror_lookup.py):
generate_permutation (eon_lookup_permutation_dev: term program, contributions, running sum), the
quotient with three matrices and challenges (eon_air_program_create_lk, eon_quotient_values_lk_dev)
against the oracle's quotient_values_fn, and the Some(permutation) branch of the native prove
(eon_prove_air_lk[_fs]) with the reference's own configuration
(eon-uni-stark/tests/lookup_air.rs: KzgPcs::new(1024, 12345), Poseidon2Bn254<3>::new_from_rng(4, 22,
SmallRng(1)))."""

import copy
import ctypes
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mirror_lookup as M
from airs import FibonacciAir
from airs_lookup import (LookupMockAir, LookupMultisetEqAir, RangeCheckAir, fold, multiset_constraints,
                         multiset_permuted_trace, multiset_terms, multiset_trace, range_check_constraints,
                         range_check_preprocessed, range_check_terms, range_check_trace)
from airs_preprocessed import MulFibPAir, mul_fib_p_preprocessed, mul_fib_p_trace
from oracle import coracle as C
from oracle import pyoracle as O
from oracle.smallrng import SmallRng, poseidon2_new_from_rng

pytestmark = pytest.mark.gpu
P = O.P
ROOT = Path(__file__).resolve().parent.parent
SRS_ALPHA = 12345
ints, lim = M.ints, M.lim
PM1 = np.array(O.int_to_limbs(P - 1), dtype=np.uint64)
PM1_INT = O.from_mont(P - 1)  # the canonical int whose stored residue is p - 1


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def host_ints(t):
    """(rows, cols, 4) device tensor -> rows of canonical ints"""
    a = t.cpu().numpy().view(np.uint64)
    return [ints(r) for r in a]


def rand_ints(seed, n):
    return [int(x) for x in ints(C.random_fr(seed, n))]


# ---- shared inputs, computed once ------------------------------------------------------------------
_CASES = {}


def perm_case(air, n):
    """-> (rows, pre_rows or None, publics, terms, perm_width), cached"""
    if (air, n) not in _CASES:
        if air == "multiset":
            _CASES[(air, n)] = (multiset_permuted_trace(n), None, [], multiset_terms, 1)
        else:
            rows, pub = range_check_trace(n)
            _CASES[(air, n)] = (rows, range_check_preprocessed(n), pub, range_check_terms, 2)
    return _CASES[(air, n)]


def program(gpu_ctx, air):
    from plonky3_eon_amd.air import AirProgram

    return AirProgram(LookupMultisetEqAir() if air == "multiset" else RangeCheckAir(), gpu_ctx)


# ---- 1. permutation trace --------------------------------------------------------------------------
@pytest.mark.parametrize("air", ["multiset", "range"])
@pytest.mark.parametrize("n", [1, 2, 8, 256, 512, 2048])  # the scan's block is 256 rows
def test_permutation_trace_vs_mirror(gpu_ctx, air, n):
    rows, pre, pub, terms, wq = perm_case(air, n)
    prog = program(gpu_ctx, air)
    assert (prog.permutation_width, prog.num_challenges) == (wq, 2 * wq)
    ch = rand_ints(900 + n + wq, 2 * wq)  # full-range challenges
    got = prog.lookup_permutation(dev(M.to_limbs(rows)), ch, pub,
                                  preprocessed_trace=dev(M.to_limbs(pre)) if pre else None)
    assert tuple(got.shape) == (n, wq, 4)
    want = M.generate_permutation(terms, rows, pre, pub, ch, wq)
    assert host_ints(got) == want
    assert n < 8 or any(any(r) for r in want)


@pytest.mark.parametrize("air", ["multiset", "range"])
def test_permutation_trace_extreme_operands(gpu_ctx, air):
    """Every cell stored as p - 1; the challenges stored as p - 1 too, except alpha stored as 0,
    since alpha equal to a cell would zero a single-element denominator."""
    n = 8
    prog = program(gpu_ctx, air)
    w, wp, wq = prog.width, prog.preprocessed_width, prog.permutation_width
    trace = np.tile(PM1, (n, w, 1))
    pre = np.tile(PM1, (n, wp, 1)) if wp else None
    ch = [0 if i % 2 == 0 else PM1_INT for i in range(2 * wq)]
    pub = [PM1_INT] * prog.n_public
    got = prog.lookup_permutation(dev(trace), ch, pub, preprocessed_trace=dev(pre) if wp else None)
    terms = multiset_terms if air == "multiset" else range_check_terms
    want = M.generate_permutation(terms, [[PM1_INT] * w] * n, [[PM1_INT] * wp] * n if wp else None, pub, ch, wq)
    assert host_ints(got) == want
    # equal cells cancel in the multiset AIR (+1 / d - 1 / d); the range check's m = p - 1 does not
    assert air == "multiset" or any(any(r) for r in want)


# ---- 2. zero denominator ---------------------------------------------------------------------------
@pytest.mark.parametrize("row", [0, 511])
def test_zero_denominator_is_an_error_and_the_context_survives(gpu_ctx, row):
    from plonky3_eon_amd import _lib

    n = 512
    rows, _, _, terms, _ = perm_case("multiset", n)
    prog = program(gpu_ctx, "multiset")
    trace = dev(M.to_limbs(rows))
    with pytest.raises(_lib.EonError) as e:
        prog.lookup_permutation(trace, [rows[row][0], 5])  # alpha = val of that row
    assert e.value.code == _lib.EON_E_ARG and "lookup 0" in str(e.value) and "zero" in str(e.value)
    with pytest.raises(M.ZeroDenominator):
        M.generate_permutation(terms, rows, None, [], [rows[row][0], 5], 1)
    ch = rand_ints(77, 2)
    assert host_ints(prog.lookup_permutation(trace, ch)) == M.generate_permutation(terms, rows, None, [], ch, 1)


# ---- 3. quotient with three matrices ---------------------------------------------------------------
def quotient_both(prog, fn, lde, pre, perm, log_n, log_qd, alpha, pub, ch):
    """(device result, oracle result) as canonical ints"""
    got = prog.quotient_values(dev(lde), log_n, log_qd, alpha, pub, preprocessed_lde=dev(pre) if pre is not None else None,
                               permutation_lde=dev(perm), challenges=ch)
    got = ints(got.cpu().numpy().view(np.uint64))
    rows = [ints(lde[i]) + (ints(pre[i]) if pre is not None else []) + ints(perm[i]) for i in range(lde.shape[0])]
    want = O.quotient_values_fn(rows, log_n, log_qd, M.split_fn(fn, prog.width, prog.preprocessed_width, ch), alpha, pub)
    return got, want


def three_ldes(prog, q, seed, kind=None):
    mats = []
    for k, w in enumerate((prog.width, prog.preprocessed_width, prog.permutation_width)):
        if w == 0:
            mats.append(None)
        elif kind is None:
            mats.append(C.random_fr(seed + 1000 * k, q * w).reshape(q, w, 4))
        else:
            mats.append(extreme_lde(kind, q, w, seed + 1000 * k))
    return mats


@pytest.mark.parametrize("air,fn,log_n,log_qd", [
    ("multiset", multiset_constraints, 0, 1), ("multiset", multiset_constraints, 3, 1),
    ("multiset", multiset_constraints, 8, 1),  # 512 quotient rows: the next row wraps across blocks
    ("range", range_check_constraints, 0, 1), ("range", range_check_constraints, 3, 1),
    ("range", range_check_constraints, 8, 1)])
def test_quotient_values_vs_oracle(gpu_ctx, air, fn, log_n, log_qd):
    prog = program(gpu_ctx, air)
    assert prog.log_quotient_degree() == log_qd  # both AIRs have degree 3: no (3, 2) case
    q = 1 << (log_n + log_qd)
    lde, pre, perm = three_ldes(prog, q, 31 * log_n + 7)  # random, not valid, three different seeds
    pub = rand_ints(99 + log_n, prog.n_public)
    ch = rand_ints(199 + log_n, prog.num_challenges)
    got, want = quotient_both(prog, fn, lde, pre, perm, log_n, log_qd, 0x1234567890ABCDEF1234567, pub, ch)
    assert got == want


@pytest.mark.parametrize("width,pre_width,perm_width,specs", [
    (3, 2, 3, [("perm", 0, 0)]),
    (3, 2, 3, [("perm", 0, 0), ("perm", 0, 1), ("perm", 0, 2), ("perm", 1, 0), ("perm", 1, 1), ("perm", 1, 2)]),
    (3, 2, 3, [("main", 0, 2), ("pre", 0, 1), ("perm", 0, 0), ("pre", 1, 0), ("perm", 1, 2), ("main", 1, 0)]),
    (3, 2, 3, [("challenge", 0, 0), ("challenge", 0, 5), ("perm", 1, 2)]),
    (2, 0, 1, [("perm", 1, 0), ("main", 1, 1), ("challenge", 0, 1), ("perm", 0, 0)]),  # no preprocessed matrix
    (1, 3, 2, [("pre", 0, 2), ("perm", 0, 1), ("main", 1, 0), ("perm", 1, 0), ("pre", 1, 0)])])  # swapped strides
def test_addressing_edges(gpu_ctx, width, pre_width, perm_width, specs):
    """Every permutation column at both offsets, first and last column, the first and the last
    challenge, next to the other matrices' boundary columns, as bare-leaf constraints; the three
    matrices are filled from different seeds, so a read from the wrong matrix or stride cannot match."""
    from plonky3_eon_amd.air import AirProgram

    air = LookupMockAir(specs, width, pre_width, perm_width)
    prog = AirProgram(air, gpu_ctx)
    assert (prog.num_constraints, prog.permutation_width, prog.num_challenges) == (len(specs), perm_width, 2 * perm_width)
    log_n, log_qd = 3, 1
    q = 1 << (log_n + log_qd)
    lde, pre, perm = three_ldes(prog, q, 40 + len(specs))
    ch = rand_ints(55 + len(specs), 2 * perm_width)
    got, want = quotient_both(prog, air.constraints, lde, pre, perm, log_n, log_qd, 0x2F1E0D0C0B0A09080706050403020100,
                              [], ch)
    assert got == want


def extreme_lde(kind, rows, width, seed):
    out = np.zeros((rows, width, 4), dtype=np.uint64)
    if kind == "pm1":
        out[:] = PM1
    elif kind == "alt":
        out[(np.add.outer(np.arange(rows), np.arange(width)) % 2) == 0] = PM1
    elif kind == "alt_rows":
        out[::2] = PM1
    else:
        out[:] = C.random_fr(seed, rows * width).reshape(rows, width, 4)
        out[np.random.default_rng(seed).random((rows, width)) < 0.25] = PM1
    return out


@pytest.mark.parametrize("kind", ["pm1", "alt", "alt_rows", "rand_pm1"])
def test_quotient_extreme_operands(gpu_ctx, kind):
    """The bound tracking treats a permutation cell as a trace cell (raw leaves of bound 32) and a
    challenge as a public value: the three matrices, the public value, the challenges and alpha
    stored as p - 1 (or p - 1 next to 0)."""
    prog = program(gpu_ctx, "range")
    for log_n, log_qd in ((3, 1), (2, 1)):
        q = 1 << (log_n + log_qd)
        lde, pre, perm = three_ldes(prog, q, 5 + log_n, kind)
        got, want = quotient_both(prog, range_check_constraints, lde, pre, perm, log_n, log_qd, PM1_INT, [PM1_INT],
                                  [PM1_INT] * 4)
        assert got == want, (kind, log_n)


def test_register_file_modes(gpu_ctx):
    """LDS and global register files (EON_AIR_REGS, read once per process: child processes) give
    the same values for a program with permutation and challenge leaves."""
    code = ("import numpy as np, torch, sys; sys.path[:0] = [sys.argv[2] + '/tests', sys.argv[2]];"
            "from airs_lookup import RangeCheckAir; from plonky3_eon_amd import Context;"
            "from plonky3_eon_amd.air import AirProgram; from oracle import coracle as C;"
            "ctx = Context(0); prog = AirProgram(RangeCheckAir(), ctx);"
            "t = lambda s, w: torch.from_numpy(C.random_fr(s, 16 * w).reshape(16, w, 4).view(np.int64)).to('cuda:0');"
            "out = prog.quotient_values(t(5, 3), 3, 1, 77, [6], preprocessed_lde=t(9, 1), permutation_lde=t(13, 2),"
            " challenges=[3, 4, 5, 6]);"
            "np.save(sys.argv[1], out.cpu().numpy())")
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for mode in ("lds", "global"):
            f = os.path.join(d, mode + ".npy")
            subprocess.run([sys.executable, "-c", code, f, str(ROOT)], check=True, timeout=300,
                           env=dict(os.environ, EON_AIR_REGS=mode))
            outs.append(np.load(f))
    np.testing.assert_array_equal(outs[0], outs[1])
    assert outs[0].any()


class ThreeLiveProductsAir(LookupMockAir):
    """LookupMockAir without constraints of its own over seven main columns a, b, c, d, e, f, x and
    one lookup of four tuples [v1 + v2 + v3], [v1 x], [v2 x], [v3 x] with v1 = a b, v2 = c d,
    v3 = e f: the three products are computed for the first denominator and stay live until the
    second, third and fourth read them."""

    def __init__(self):
        super().__init__([], 7, 0, 0)

    def add_lookup_columns(self):
        return [0]

    def get_lookups(self):
        from plonky3_eon_amd.symbolic import Direction, Entry, Kind, SymbolicVariable, register_lookup

        a, b, c, d, e, f, x = (SymbolicVariable(Entry("main", 0), i) for i in range(7))
        v1, v2, v3 = a * b, c * d, e * f
        return [register_lookup(self, Kind.Local, [([v1 + v2 + v3], 1, Direction.RECEIVE), ([v1 * x], 1, Direction.SEND),
                                                   ([v2 * x], 1, Direction.SEND), ([v3 * x], 1, Direction.SEND)])]


def three_live_products_terms(loc, nxt, ploc, pnxt, pub, ch):
    a, b, c, d, e, f, x = loc
    v1, v2, v3 = a * b % P, c * d % P, e * f % P
    return [(0, [((ch[0] - fold([(v1 + v2 + v3) % P], ch[1])) % P, 1)] +
             [((ch[0] - fold([v * x % P], ch[1])) % P, P - 1) for v in (v1, v2, v3)])]


def test_permutation_trace_register_file_modes(gpu_ctx):
    """eon_lookup_permutation_dev with the term program's register file in LDS and in global memory
    (EON_AIR_REGS, read once per process: one child process per mode) gives bit-equal permutation
    traces, and the LDS one is the mirror's.  Registers 0 and 1 live in VGPRs, so only a term
    program with more than two registers touches the file: ThreeLiveProductsAir's has 5, three of
    them in memory (25 instructions; LookupMultisetEqAir's has 1 and RangeCheckAir's 2: counted
    once by running the library's compile() on each AIR's term roots on the host).  8 rows are a
    partial wave; 512 rows are two blocks, so the global planes' stride (the height) differs from
    the block size."""
    heights = (8, 512)
    code = ("import numpy as np, torch, sys; sys.path[:0] = [sys.argv[2] + '/tests', sys.argv[2]];"
            "from test_gpu_lookup import ThreeLiveProductsAir, rand_ints; from plonky3_eon_amd import Context;"
            "from plonky3_eon_amd.air import AirProgram; from oracle import coracle as C;"
            "ctx = Context(0); prog = AirProgram(ThreeLiveProductsAir(), ctx);"
            "t = lambda n: torch.from_numpy(C.random_fr(21 + n, n * 7).reshape(n, 7, 4).view(np.int64)).to('cuda:0');"
            "np.savez(sys.argv[1], **{str(n): prog.lookup_permutation(t(n), rand_ints(23, 2)).cpu().numpy()"
            " for n in map(int, sys.argv[3:])})")
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for mode in ("lds", "global"):
            f = os.path.join(d, mode + ".npz")
            subprocess.run([sys.executable, "-c", code, f, str(ROOT), *map(str, heights)], check=True, timeout=300,
                           env=dict(os.environ, EON_AIR_REGS=mode))
            outs.append(dict(np.load(f)))
    for n in heights:
        lds, glob = outs[0][str(n)], outs[1][str(n)]
        np.testing.assert_array_equal(lds, glob)
        rows = [ints(r) for r in C.random_fr(21 + n, n * 7).reshape(n, 7, 4)]
        want = M.generate_permutation(three_live_products_terms, rows, None, [], rand_ints(23, 2), 1)
        assert [ints(r) for r in lds.view(np.uint64)] == want
        assert any(any(r) for r in want)


# ---- 4. native prove -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ch_consts():
    # the reference's challenger permutation: Perm::new_from_rng(4, 22, SmallRng(1)) (lookup_air.rs:128-134)
    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    return py, ([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]])


@pytest.fixture(scope="module")
def srs():
    return C.g1_srs(1025, C.fr_from_u64(SRS_ALPHA))


@pytest.fixture(scope="module")
def pcs(gpu_ctx):
    from plonky3_eon_amd.native import NativeKzgPcs

    p = NativeKzgPcs(1024, SRS_ALPHA, gpu_ctx)
    yield p
    p.close()


def challenger(ch_consts):
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants

    return Challenger(Poseidon2Constants(*ch_consts[1]))


def assert_proofs_equal(got, want):
    """byte-equal: challenges, every commitment, every opened value and witness, the order of `opened`"""
    assert list(got.permutation_challenges) == list(want.permutation_challenges)
    assert (got.alpha, got.zeta) == (want.alpha, want.zeta)
    np.testing.assert_array_equal(got.trace_commit[0], want.trace_commit[0])
    np.testing.assert_array_equal(got.permutation_commit[0], want.permutation_commit[0])
    assert (got.preprocessed_commit is None) == (want.preprocessed_commit is None)
    if want.preprocessed_commit is not None:
        np.testing.assert_array_equal(got.preprocessed_commit[0], want.preprocessed_commit[0])
    assert len(got.quotient_commit) == len(want.quotient_commit)
    for c in range(len(want.quotient_commit)):
        np.testing.assert_array_equal(got.quotient_commit[c], want.quotient_commit[c])
    assert len(got.opened) == len(want.opened)  # trace, permutation, quotient chunks(, preprocessed)
    for r in range(len(want.opened)):
        assert len(got.opened[r].values) == len(want.opened[r].values)
        for m in range(len(want.opened[r].values)):
            assert len(got.opened[r].values[m]) == len(want.opened[r].values[m])
            for p in range(len(want.opened[r].values[m])):
                np.testing.assert_array_equal(got.opened[r].values[m][p], want.opened[r].values[m][p])
                np.testing.assert_array_equal(got.opened[r].witnesses[m][p], want.opened[r].witnesses[m][p])


def gpu_verify_batch(gpu_ctx, claims):
    """the mirror's KZG claims through KzgPcs::verify's multi-pairing on the GPU"""
    from plonky3_eon_amd import verify as GV

    g2a = GV.g2_mul(SRS_ALPHA, ctx=gpu_ctx)
    return GV.verify_batch(np.stack([np.asarray(c, dtype=np.uint64).reshape(8) for c, _, _, _ in claims]),
                           np.stack([np.asarray(w, dtype=np.uint64).reshape(8) for _, _, _, w in claims]),
                           np.stack([lim(v) for _, _, v, _ in claims]), np.stack([lim(z) for _, z, _, _ in claims]),
                           g2a, ctx=gpu_ctx)


ALL_TRUE = {"transcript": True, "ood": True, "opened_vs_trace": True, "kzg": True}


@pytest.mark.parametrize("rows", [multiset_trace(8), multiset_permuted_trace(64)], ids=["test_lookup_ok", "permuted64"])
def test_multiset_prove_vs_mirror_and_verify(gpu_ctx, pcs, srs, ch_consts, rows):
    from plonky3_eon_amd.native import prove_native

    n = len(rows)
    log_n = n.bit_length() - 1
    trace = M.to_limbs(rows)
    prog = program(gpu_ctx, "multiset")
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts))
    assert proof.degree_bits == log_n and proof.preprocessed_commit is None and len(proof.opened) == 3
    want = M.prove(trace, None, None, srs, multiset_constraints, multiset_terms, 1, 1,
                   challenger=O.DuplexChallenger(ch_consts[0]))
    assert_proofs_equal(proof, want)
    res, claims = M.verify(proof, None, multiset_constraints, 1, log_n, 1, SRS_ALPHA,
                           challenger=O.DuplexChallenger(ch_consts[0]), trace=trace, perm=want.permutation)
    assert res == ALL_TRUE, res
    assert gpu_verify_batch(gpu_ctx, claims) is True


def range_inputs(n):
    rows, pub = range_check_trace(n)
    return M.to_limbs(rows), M.to_limbs(range_check_preprocessed(n)), pub


def test_range_check_prove_with_preprocessed_vs_mirror_and_verify(gpu_ctx, pcs, srs, ch_consts):
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    n = 16
    trace, pre, pub = range_inputs(n)
    prog = program(gpu_ctx, "range")
    pp = setup_preprocessed(pcs, dev(pre))
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), public_values=pub,
                         preprocessed=pp, preprocessed_trace=dev(pre))
    assert len(proof.opened) == 4 and len(proof.permutation_challenges) == 4
    mpp = M.setup(pre, srs)
    want = M.prove(trace, mpp, pre, srs, range_check_constraints, range_check_terms, 2, 1, pub,
                   challenger=O.DuplexChallenger(ch_consts[0]))
    assert_proofs_equal(proof, want)
    res, claims = M.verify(proof, mpp.commitment, range_check_constraints, 2, 4, 1, SRS_ALPHA,
                           challenger=O.DuplexChallenger(ch_consts[0]), trace=trace, pre=pre, perm=want.permutation,
                           publics=pub)
    assert res == ALL_TRUE, res
    assert gpu_verify_batch(gpu_ctx, claims) is True
    # the entry with given challenges, alpha and zeta
    ch, a, z = rand_ints(5, 4), 0x1111222233334444, 0x5555666677778888
    proof = prove_native(prog, pcs, dev(trace), a, z, public_values=pub, preprocessed=pp, preprocessed_trace=dev(pre),
                         permutation_challenges=ch)
    want = M.prove(trace, mpp, pre, srs, range_check_constraints, range_check_terms, 2, 1, pub, challenges=ch, alpha=a,
                   zeta=z)
    assert_proofs_equal(proof, want)
    res, _ = M.verify(proof, mpp.commitment, range_check_constraints, 2, 4, 1, SRS_ALPHA, challenges=ch, alpha=a, zeta=z,
                      trace=trace, pre=pre, perm=want.permutation, publics=pub)
    assert res == {"ood": True, "opened_vs_trace": True, "kzg": True}, res
    pp.close()


# ---- 5. soundness behaviour ------------------------------------------------------------------------
def test_bad_trace_and_tampered_opening_do_not_verify(gpu_ctx, pcs, ch_consts):
    """lookup_air.rs:112 (val = 1 on row 0, the table all zero): the prove goes through -- the
    reference panics only in its debug check -- and the verifier's out-of-domain identity fails;
    lookup_air.rs:169-187: permutation_local[0] += 1 on an honest proof is rejected."""
    from plonky3_eon_amd.native import prove_native

    prog = program(gpu_ctx, "multiset")
    trace = M.to_limbs(multiset_trace(8, bad=True))
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts))
    res, _ = M.verify(proof, None, multiset_constraints, 1, 3, 1, SRS_ALPHA, challenger=O.DuplexChallenger(ch_consts[0]),
                      trace=trace, perm=M.to_limbs(M.generate_permutation(
                          multiset_terms, multiset_trace(8, bad=True), None, [], proof.permutation_challenges, 1)))
    assert res == {"transcript": True, "ood": False, "opened_vs_trace": True, "kzg": True}, res
    proof = prove_native(prog, pcs, dev(M.to_limbs(multiset_trace(8))), None, None, challenger=challenger(ch_consts))
    bad = copy.deepcopy(proof)
    v = ints(bad.opened[1].values[0][0])
    bad.opened[1].values[0][0] = np.stack([lim(v[0] + 1)] + [lim(x) for x in v[1:]])
    res, claims = M.verify(bad, None, multiset_constraints, 1, 3, 1, SRS_ALPHA, challenger=O.DuplexChallenger(ch_consts[0]))
    assert res["transcript"] and not res["ood"] and not res["kzg"], res
    assert gpu_verify_batch(gpu_ctx, claims) is False


def test_wrong_preprocessed_trace_does_not_verify(gpu_ctx, pcs, srs, ch_consts):
    """pre_trace is not checked against the committed data: a permutation trace generated from
    another matrix gives a proof the verifier rejects."""
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    n = 16
    trace, pre, pub = range_inputs(n)
    wrong = M.to_limbs([[(i + 1) % n] for i in range(n)])
    prog = program(gpu_ctx, "range")
    pp = setup_preprocessed(pcs, dev(pre))
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), public_values=pub,
                         preprocessed=pp, preprocessed_trace=dev(wrong))
    res, _ = M.verify(proof, pp.commitment, range_check_constraints, 2, 4, 1, SRS_ALPHA,
                      challenger=O.DuplexChallenger(ch_consts[0]), publics=pub)
    assert res == {"transcript": True, "ood": False, "kzg": True}, res
    pp.close()


# ---- 6. refusals -----------------------------------------------------------------------------------
def raw_create_lk(ctx, nodes, roots=(0,), width=2, pre_width=0, perm_width=1, n_challenges=2, lookups=(), terms=(),
                  consts=(0,)):
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.field import ints_to_limbs

    arr = (_lib.eon_sym_node * max(1, len(nodes)))(*[_lib.eon_sym_node(*n) for n in nodes])
    ca = np.ascontiguousarray(ints_to_limbs(list(consts)))
    ra = np.ascontiguousarray(np.array(roots, dtype=np.uint32))
    la = (_lib.eon_lookup_desc * max(1, len(lookups)))(*[_lib.eon_lookup_desc(*x) for x in lookups])
    ta = (_lib.eon_lookup_term * max(1, len(terms)))(*[_lib.eon_lookup_term(*x) for x in terms])
    h = ctypes.c_void_p()
    rc = ctx.lib.eon_air_program_create_lk(ctx.handle, arr, len(nodes), ca.ctypes.data_as(ctypes.c_void_p), len(consts),
                                           ra.ctypes.data_as(ctypes.c_void_p), len(roots), width, pre_width, 0,
                                           perm_width, n_challenges, la, len(lookups), ta, ctypes.byref(h))
    return rc, h


def last_error(ctx):
    return ctx.lib.eon_last_error(ctx.handle).decode()


def test_create_refusals(gpu_ctx):
    from plonky3_eon_amd import _lib

    ARG = _lib.EON_E_ARG
    MAIN, SEL, PERM, CH = (1, 0, 0), (3, 0, 0), (11, 0, 0), (12, 0, 0)

    def rejected(word, nodes, **kw):
        rc, _ = raw_create_lk(gpu_ctx, nodes, **kw)
        return rc == ARG and word in last_error(gpu_ctx)

    assert rejected("permutation", [(11, 1, 0)])  # permutation column >= permutation_width
    assert rejected("permutation", [(11, 0, 2)])  # offset 2
    assert rejected("challenge", [(12, 2, 0)])  # challenge index >= n_challenges
    assert rejected("n_challenges", [MAIN], n_challenges=3)  # != 2 * permutation_width
    assert rejected("n_challenges", [MAIN], perm_width=0, n_challenges=2)
    two = dict(perm_width=2, n_challenges=4)
    assert rejected("duplicate", [MAIN, CH], lookups=[(0, 1), (0, 1)], terms=[(1, 0), (1, 0)], **two)
    assert rejected("auxiliary column", [MAIN, CH], lookups=[(0, 1), (2, 1)], terms=[(1, 0), (1, 0)], **two)
    assert rejected("every permutation column", [MAIN, CH], lookups=[(0, 1)], terms=[(1, 0)], **two)
    assert rejected("permutation", [MAIN, PERM], lookups=[(0, 1)], terms=[(1, 0)])  # denominator reaches a perm leaf
    assert rejected("permutation", [MAIN, PERM, (6, 0, 1)], lookups=[(0, 1)], terms=[(0, 2)])  # multiplicity does
    assert rejected("selector", [MAIN, SEL, (9, 0, 1)], lookups=[(0, 1)], terms=[(2, 0)])  # ... a selector
    assert rejected("out of range", [MAIN], lookups=[(0, 1)], terms=[(0, 7)])  # a term names no node
    # accepted: the last permutation column, next row, and the last challenge, with one lookup
    rc, h = raw_create_lk(gpu_ctx, [(11, 0, 1), (12, 1, 0), MAIN], roots=(0, 1), lookups=[(0, 1)], terms=[(1, 2)])
    assert rc == 0, last_error(gpu_ctx)
    lib = gpu_ctx.lib
    assert (lib.eon_air_program_permutation_width(h), lib.eon_air_program_num_challenges(h),
            lib.eon_air_program_num_lookups(h)) == (1, 2, 1)
    lib.eon_air_program_destroy(h)
    # the context is usable afterwards
    test_permutation_trace_vs_mirror(gpu_ctx, "multiset", 8)


def test_lookup_program_through_the_old_calls_and_missing_matrices(gpu_ctx, pcs, ch_consts):
    import torch

    from plonky3_eon_amd import _lib, native
    from plonky3_eon_amd.field import fr_to_abi
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    ARG = _lib.EON_E_ARG
    n = 16
    trace, pre, pub = range_inputs(n)
    prog = program(gpu_ctx, "range")
    multi = program(gpu_ctx, "multiset")
    q = 2 * n
    z = lambda w: torch.zeros((q, w, 4), dtype=torch.int64, device="cuda:0")  # noqa: E731
    for call in (lambda: multi.quotient_values(z(2), 4, 1, 5),  # eon_quotient_values_dev
                 lambda: prog.quotient_values(z(3), 4, 1, 5, [1], preprocessed_lde=z(1)),  # ..._pp_dev
                 lambda: prog.quotient_values(z(3), 4, 1, 5, [1], preprocessed_lde=z(1), challenges=[1, 2, 3, 4])):
        with pytest.raises(_lib.EonError) as e:  # the last one: a missing perm_lde
            call()
        assert e.value.code == ARG and "perm" in str(e.value)
    with pytest.raises(_lib.EonError) as e:  # a term reads a preprocessed leaf: pre_trace is required
        prog.lookup_permutation(dev(trace), [1, 2, 3, 4], pub)
    assert e.value.code == ARG and "pre_trace" in str(e.value)
    # eon_prove_air_fs, eon_prove_air_pp and the lookup prove without pre_trace
    pp = setup_preprocessed(pcs, dev(pre))
    p = native._p
    w, tdev = 2, dev(M.to_limbs(multiset_trace(8)))
    arrs = [np.zeros(s, np.uint64) for s in ((w, 8), (2, 8), (2, w, 4), (2, w, 8), (2, 4), (2, 8))]
    out = native.eon_proof(*[p(a) for a in arrs], 0)
    rc = pcs.lib.eon_prove_air_fs(pcs._h, multi.handle, ctypes.c_void_p(tdev.data_ptr()), 8, None, 0,
                                  challenger(ch_consts).handle, ctypes.byref(out), None, None)
    assert rc == ARG and "eon_prove_air_lk" in pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode()
    out_pp = native.eon_proof_pp(out, None, None, None)
    a, zt = fr_to_abi(3), fr_to_abi(4)
    rc = pcs.lib.eon_prove_air_pp(pcs._h, multi.handle, ctypes.c_void_p(tdev.data_ptr()), 8, None, 0, None,
                                  ctypes.byref(a), ctypes.byref(zt), ctypes.byref(out_pp))
    assert rc == ARG and "eon_prove_air_lk" in pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode()
    with pytest.raises(_lib.EonError) as e:
        prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), public_values=pub,
                     preprocessed=pp)
    assert e.value.code == ARG and "pre_trace" in str(e.value)
    # the pcs and the context still prove
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), public_values=pub,
                         preprocessed=pp, preprocessed_trace=dev(pre))
    res, _ = M.verify(proof, pp.commitment, range_check_constraints, 2, 4, 1, SRS_ALPHA,
                      challenger=O.DuplexChallenger(ch_consts[0]), publics=pub)
    assert res == {"transcript": True, "ood": True, "kzg": True}, res
    pp.close()


def test_lk_call_without_lookups_is_eon_prove_air_pp(gpu_ctx, pcs):
    """A program without lookups through eon_prove_air_lk gives eon_prove_air_pp's proof, byte for byte."""
    from plonky3_eon_amd import native
    from plonky3_eon_amd.air import AirProgram, _publics_limbs
    from plonky3_eon_amd.field import fr_to_abi
    from plonky3_eon_amd.native import setup_preprocessed

    p = native._p
    a, z = fr_to_abi(0x1111), fr_to_abi(0x2222)

    def arrays(w, wp):
        shapes = [(w, 8), (1 << 1, 8), (2, w, 4), (2, w, 8), (1 << 1, 4), (1 << 1, 8), (wp, 8), (2, wp, 4), (2, wp, 8)]
        return [np.zeros(s, np.uint64) for s in shapes]

    # MulFibPAir with preprocessed data, and FibonacciAir without
    n = 8
    pre = dev(M.to_limbs(mul_fib_p_preprocessed(n)))
    pp = setup_preprocessed(pcs, pre)
    cases = [(AirProgram(MulFibPAir(), gpu_ctx), dev(M.to_limbs(mul_fib_p_trace(0, 1, n))), [], pp, 2),
             (AirProgram(FibonacciAir(), gpu_ctx), dev(M.to_limbs(O.fib_trace(0, 1, n))), [0, 1, 21], None, 0)]
    for prog, trace, pis, handle, wp in cases:
        pub = _publics_limbs(pis)
        tp = ctypes.c_void_p(trace.data_ptr())
        outs = []
        for lk in (False, True):
            arr = arrays(prog.width, max(wp, 1))
            base = native.eon_proof(*[p(x) for x in arr[:6]], 0)
            opp = native.eon_proof_pp(base, *([p(x) for x in arr[6:]] if wp else [None] * 3))
            h = handle.handle if handle is not None else None
            if lk:
                olk = native.eon_proof_lk(opp, None, None, None)
                pcs.check(pcs.lib.eon_prove_air_lk(pcs._h, prog.handle, tp, n, p(pub), len(pis), h, None, None, 0,
                                                   ctypes.byref(a), ctypes.byref(z), ctypes.byref(olk)))
            else:
                pcs.check(pcs.lib.eon_prove_air_pp(pcs._h, prog.handle, tp, n, p(pub), len(pis), h, ctypes.byref(a),
                                                   ctypes.byref(z), ctypes.byref(opp)))
            outs.append(arr)
        chunks = 1 << prog.log_quotient_degree()
        for x, y in zip(*outs):
            np.testing.assert_array_equal(x, y)
        assert outs[0][0].any() and outs[0][1][:chunks].any() and (not wp or outs[0][6].any())
    pp.close()
