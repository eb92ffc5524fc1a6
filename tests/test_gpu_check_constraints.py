"""check_constraints on the GPU (eon_check_constraints_dev, k_air_check) and in the native prove
(eon_kzg_pcs_set_check_constraints), exact against the CPU mirror (tests/mirror_check.py): the
reference's first failure (row, constraint, value), the total and the per-constraint counts.

The mirror evaluates the constraint functions the other suites already use: pyoracle's
fib_constraints and p2_constraints, MulAir's and MixedAir's of test_gpu_air_program, the
preprocessed AIRs' (airs_preprocessed) and the lookup AIRs' (airs_lookup)."""

import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mirror_check as MC
import mirror_lookup as ML
from airs import FibonacciAir, MixedAir, MockAir, MulAir
from airs_lookup import (LookupMultisetEqAir, RangeCheckAir, multiset_constraints, multiset_permuted_trace,
                         multiset_terms, multiset_trace, range_check_constraints, range_check_preprocessed,
                         range_check_trace)
from airs_preprocessed import (MixedPreAir, MulFibPAir, mixed_pre_constraints, mixed_pre_preprocessed,
                               mixed_pre_trace, mul_fib_p_constraints, mul_fib_p_preprocessed, mul_fib_p_trace)
from oracle import coracle as C
from oracle import pyoracle as O
from test_gpu_air_program import mixed_constraints, mul_constraints, mul_trace

pytestmark = pytest.mark.gpu
P = O.P
ROOT = Path(__file__).resolve().parent.parent
ints, lim, to_limbs = ML.ints, ML.lim, ML.to_limbs
PM1_INT = O.from_mont(P - 1)  # the canonical ints whose stored residues are p - 1 and 1
ONE_INT = O.from_mont(1)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def host_ints(t):
    return [ints(r) for r in t.cpu().numpy().view(np.uint64)]


def rand_ints(seed, n):
    return [int(x) for x in ints(C.random_fr(seed, n))]


def rand_rows(seed, n, w):
    v = rand_ints(seed, n * w)
    return [v[i * w:(i + 1) * w] for i in range(n)]


def program(gpu_ctx, air):
    from plonky3_eon_amd.air import AirProgram

    return AirProgram(air, gpu_ctx)


def gpu_check(prog, rows, pub=(), pre=None, perm=None, ch=()):
    return prog.check_constraints(dev(to_limbs(rows)), pub, preprocessed_trace=dev(to_limbs(pre)) if pre else None,
                                  permutation_trace=dev(to_limbs(perm)) if perm else None, challenges=ch,
                                  per_constraint=True)


def as_dict(rep):
    return {"failures": rep.failures, "row": rep.row, "constraint": rep.constraint, "value": rep.value,
            "failing_constraints": rep.failing_constraints, "counts": rep.counts}


def both(prog, fn, rows, pub=(), pre=None, perm=None, ch=(), only_rows=None):
    """(device report, mirror summary) as dicts"""
    got = as_dict(gpu_check(prog, rows, pub, pre, perm, ch))
    want = MC.summary(MC.check_constraints(fn, rows, pre, perm, pub, ch, only_rows), prog.num_constraints)
    return got, want


CLEAN = {"failures": 0, "row": 0, "constraint": 0, "value": 0, "failing_constraints": 0}


def assert_clean(got, want):
    assert want["failures"] == 0, want  # the trace is valid by the mirror as well
    assert got == dict(CLEAN, counts=[0] * len(want["counts"]))


# ---- the reference's own cases ---------------------------------------------------------------------
@pytest.mark.parametrize("name,rows,publics,first", MC.ROW_LOGIC_CASES, ids=[c[0] for c in MC.ROW_LOGIC_CASES])
def test_row_logic_cases(gpu_ctx, name, rows, publics, first):
    """check_constraints.rs:308-422, the 1-row trace included (next wraps onto the row itself and
    the wave has one live lane)."""
    prog = program(gpu_ctx, MC.RowLogicAir())
    got, want = both(prog, MC.main_fn(MC.row_logic_constraints), rows, publics)
    assert got == want
    if first is None:
        assert_clean(got, want)
    else:
        assert (got["row"], got["constraint"], got["failures"]) == (*first, 1)


# ---- valid traces ----------------------------------------------------------------------------------
def test_fibonacci_valid(gpu_ctx):
    prog = program(gpu_ctx, FibonacciAir())
    assert_clean(*both(prog, MC.main_fn(O.fib_constraints), O.fib_trace(0, 1, 8), [0, 1, 21]))


@pytest.mark.parametrize("n", [8, 512])  # 512: two blocks, the last row's next is row 0 of another block
def test_mul_air_valid(gpu_ctx, n):
    prog = program(gpu_ctx, MulAir())
    assert_clean(*both(prog, MC.main_fn(mul_constraints), mul_trace(n)))


def test_preprocessed_airs_valid(gpu_ctx):
    n = 16
    prog = program(gpu_ctx, MulFibPAir())
    assert_clean(*both(prog, MC.pre_fn(mul_fib_p_constraints), mul_fib_p_trace(1, 1, n), pre=mul_fib_p_preprocessed(n)))
    prog = program(gpu_ctx, MixedPreAir())
    rows, pub = mixed_pre_trace(3, 4, 5, n)
    assert_clean(*both(prog, MC.pre_fn(mixed_pre_constraints), rows, pub, pre=mixed_pre_preprocessed(n)))


@pytest.mark.parametrize("air", ["multiset", "range"])
def test_lookup_airs_valid(gpu_ctx, air):
    """The permutation trace of lookup_permutation under random challenges satisfies the LogUp
    constraints, the last row's wrap onto perm[0] = 0 included."""
    n = 16
    if air == "multiset":
        prog, fn, rows, pre, pub = program(gpu_ctx, LookupMultisetEqAir()), multiset_constraints, multiset_permuted_trace(n), None, []
    else:
        rows, pub = range_check_trace(n)
        prog, fn, pre = program(gpu_ctx, RangeCheckAir()), range_check_constraints, range_check_preprocessed(n)
    ch = rand_ints(900 + n, prog.num_challenges)
    perm = host_ints(prog.lookup_permutation(dev(to_limbs(rows)), ch, pub,
                                             preprocessed_trace=dev(to_limbs(pre)) if pre else None))
    assert any(any(r) for r in perm)
    assert_clean(*both(prog, fn, rows, pub, pre, perm, ch))


@pytest.fixture(scope="module")
def p2():
    py = O.p2_constants(2024, 4, 56)
    k = C.P2Constants([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]])
    return py, k


def p2_trace(gpu_ctx, k, vl, n, seed):
    from plonky3_eon_amd.air import Poseidon2Air

    air = Poseidon2Air(k.begin, k.partial, k.end, vl, gpu_ctx)
    inputs = C.random_fr(seed, n * vl * 3).reshape(n * vl, 3, 4)
    return air, air.generate_trace(dev(inputs))


@pytest.mark.parametrize("vl", [1, 8])
def test_poseidon2_generated_trace_valid(gpu_ctx, p2, vl):
    py, k = p2
    air, trace = p2_trace(gpu_ctx, k, vl, 8, 31 + vl)
    prog = program(gpu_ctx, air)
    rep = prog.check_constraints(trace, per_constraint=True)
    want = MC.summary(MC.check_constraints(MC.p2_fn(O.p2_constraints, py, vl), host_ints(trace)), prog.num_constraints)
    assert_clean(as_dict(rep), want)


# ---- one tampered cell -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mul512():
    return mul_trace(512)


@pytest.mark.parametrize("r", [0, 63, 64, 255, 256, 511])  # wave and block edges, first and last row
def test_mul_air_one_tampered_cell(gpu_ctx, mul512, r):
    """a of triple 3 on row r is one more: a^2 b - c fails there, the first-row constraint on row 0,
    the transition out of r (not on the last row) and into r (not into row 0)."""
    rows = [list(x) for x in mul512]
    rows[r][9] = (rows[r][9] + 1) % P
    prog = program(gpu_ctx, MulAir())
    got, want = both(prog, MC.main_fn(mul_constraints), rows)
    assert got == want
    assert want["row"] == (r - 1 if r else 0) and want["failures"] == (2 if r == 511 else 3)


def test_poseidon2_one_tampered_cell(gpu_ctx, p2):
    """512 rows, VECTOR_LEN 1, one cell of row 300 changed; the AIR has no next-row constraint, so
    the mirror evaluates that row only."""
    py, k = p2
    air, trace = p2_trace(gpu_ctx, k, 1, 512, 77)
    row = host_ints(trace[300:301])[0]
    row[10] = (row[10] + 1) % P
    trace[300, 10] = dev(lim(row[10]))
    prog = program(gpu_ctx, air)
    got = as_dict(prog.check_constraints(trace, per_constraint=True))
    rows = [None] * 300 + [row] + [None] * 211
    rows[301] = row  # the (unread) next row
    want = MC.summary(MC.check_constraints(MC.p2_fn(O.p2_constraints, py, 1), rows, only_rows=[300]), prog.num_constraints)
    assert got == want
    assert want["row"] == 300 and want["failures"] >= 1


# ---- fully random traces: the 0 / 1 selectors ------------------------------------------------------
def test_random_trace_mixed_air(gpu_ctx):
    """Every ungated constraint fails on every row; the first-row-gated one on row 0 only, the
    last-row-gated one on row 63 only, the transition-gated one on every row but the last."""
    n = 64
    prog = program(gpu_ctx, MixedAir())
    rows, pub = rand_rows(5, n, prog.width), rand_ints(6, 2)
    got, want = both(prog, MC.main_fn(mixed_constraints), rows, pub)
    assert got == want
    assert (want["counts"][1], want["counts"][2], want["counts"][3]) == (1, 1, n - 1) and want["counts"][0] == n


def test_random_trace_range_check_air(gpu_ctx):
    n = 64
    prog = program(gpu_ctx, RangeCheckAir())
    rows, pre, perm = rand_rows(7, n, 3), rand_rows(8, n, 1), rand_rows(9, n, 2)
    pub, ch = rand_ints(10, 1), rand_ints(11, 4)
    got, want = both(prog, range_check_constraints, rows, pub, pre, perm, ch)
    assert got == want
    # the AIR's own and each lookup's first-row constraint on row 0 only, the running sums everywhere
    assert want["counts"] == [1, 1, n, 1, n]


# ---- zero modulo p ---------------------------------------------------------------------------------
class ZeroModAir:
    """Differences and a product of cells that cancel: the interpreter's lazy values are a - b + K p
    (a nonzero multiple of p when a = b), never the integer 0."""

    def width(self):
        return 3

    def num_public_values(self):
        return 0

    def eval(self, builder):
        m = builder.main()
        loc, nxt = m[0], m[1]
        builder.assert_zero(loc[0] - nxt[0])
        builder.assert_zero(loc[0] * loc[1] - loc[2])
        builder.assert_zero(loc[1] + loc[2] - nxt[1] - nxt[2])
        builder.assert_zero(-loc[0] + nxt[0])


def zero_mod_constraints(loc, nxt, sels, pub):
    return [(loc[0] - nxt[0]) % P, (loc[0] * loc[1] - loc[2]) % P, (loc[1] + loc[2] - nxt[1] - nxt[2]) % P,
            (-loc[0] + nxt[0]) % P]


# rows of cells whose stored residue is p - 1, 0 or 1 that satisfy the AIR when repeated: x y = z
# needs a zero factor, x and y + z are constant over the rows
ZERO_MOD_ROWS = [[PM1_INT, 0, 0], [0, PM1_INT, 0], [ONE_INT, 0, 0], [0, ONE_INT, 0], [0, 0, 0]]


@pytest.mark.parametrize("row", ZERO_MOD_ROWS, ids=["pm1_0_0", "0_pm1_0", "1_0_0", "0_1_0", "0_0_0"])
def test_zero_modulo_p(gpu_ctx, row):
    n = 8
    prog = program(gpu_ctx, ZeroModAir())
    fn = MC.main_fn(zero_mod_constraints)
    rows = [list(row) for _ in range(n)]
    assert_clean(*both(prog, fn, rows))
    for col in range(3):  # one cell one more: exactly the mirror's failures
        bad = [list(x) for x in rows]
        bad[3][col] = (bad[3][col] + 1) % P
        got, want = both(prog, fn, bad)
        assert got == want and want["failures"] >= 2, (col, want)


# ---- register-file modes ---------------------------------------------------------------------------
def test_register_file_modes(gpu_ctx):
    """LDS and global register files (EON_AIR_REGS, read once per process: child processes) report
    the same failures on a failing RangeCheckAir trace, and the default run equals the mirror."""
    code = ("import numpy as np, torch, sys; sys.path[:0] = [sys.argv[2] + '/tests', sys.argv[2]];"
            "from airs_lookup import RangeCheckAir; from plonky3_eon_amd import Context;"
            "from plonky3_eon_amd.air import AirProgram; from oracle import coracle as C;"
            "ctx = Context(0); prog = AirProgram(RangeCheckAir(), ctx);"
            "t = lambda s, w: torch.from_numpy(C.random_fr(s, 64 * w).reshape(64, w, 4).view(np.int64)).to('cuda:0');"
            "r = prog.check_constraints(t(5, 3), [6], preprocessed_trace=t(9, 1), permutation_trace=t(13, 2),"
            " challenges=[3, 4, 5, 6], per_constraint=True);"
            "np.save(sys.argv[1], np.array([r.failures, r.row, r.constraint, r.failing_constraints]"
            " + [(r.value >> (64 * i)) & (2 ** 64 - 1) for i in range(4)] + r.counts, dtype=np.uint64))")
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for mode in ("lds", "global"):
            f = os.path.join(d, mode + ".npy")
            subprocess.run([sys.executable, "-c", code, f, str(ROOT)], check=True, timeout=300,
                           env=dict(os.environ, EON_AIR_REGS=mode))
            outs.append(np.load(f))
    np.testing.assert_array_equal(outs[0], outs[1])
    rows, pre, perm = ([ints(r) for r in C.random_fr(s, 64 * w).reshape(64, w, 4)] for s, w in ((5, 3), (9, 1), (13, 2)))
    want = MC.summary(MC.check_constraints(range_check_constraints, rows, pre, perm, [6], [3, 4, 5, 6]), 5)
    value = sum(int(v) << (64 * i) for i, v in enumerate(outs[0][4:8]))
    assert [int(v) for v in outs[0][:4]] == [want["failures"], want["row"], want["constraint"], want["failing_constraints"]]
    assert value == want["value"] and [int(v) for v in outs[0][8:]] == want["counts"] and want["failures"] > 64


# ---- argument rules --------------------------------------------------------------------------------
def test_argument_errors(gpu_ctx):
    import ctypes

    from plonky3_eon_amd import Context, _lib

    def raises(code, word, f):
        with pytest.raises(_lib.EonError) as e:
            f()
        assert e.value.code == code and word in str(e.value), str(e.value)

    n = 8
    rng = program(gpu_ctx, RangeCheckAir())
    t, pre, perm = dev(to_limbs(rand_rows(1, n, 3))), dev(to_limbs(rand_rows(2, n, 1))), dev(to_limbs(rand_rows(3, n, 2)))
    ok = dict(preprocessed_trace=pre, permutation_trace=perm, challenges=[1, 2, 3, 4])
    assert rng.check_constraints(t, [5], **ok).failures > 0
    raises(_lib.EON_E_ARG, "pre_trace must not be null", lambda: rng.check_constraints(t, [5], **dict(ok, preprocessed_trace=None)))
    raises(_lib.EON_E_ARG, "perm_trace must not be null", lambda: rng.check_constraints(t, [5], **dict(ok, permutation_trace=None)))
    raises(_lib.EON_E_SHAPE, "public value count", lambda: rng.check_constraints(t, [5, 6], **ok))
    raises(_lib.EON_E_SHAPE, "challenge count", lambda: rng.check_constraints(t, [5], **dict(ok, challenges=[1, 2, 3])))
    noncanon = np.array([O.int_to_limbs(P)], dtype=np.uint64)
    raises(_lib.EON_E_ARG, "public value is not a canonical", lambda: rng.check_constraints(t, noncanon, **ok))
    raises(_lib.EON_E_ARG, "challenge is not a canonical",
           lambda: rng.check_constraints(t, [5], **dict(ok, challenges=np.tile(noncanon, (4, 1)))))
    fib = program(gpu_ctx, FibonacciAir())
    t2 = dev(to_limbs(O.fib_trace(0, 1, n)))
    raises(_lib.EON_E_SHAPE, "power of two", lambda: fib.check_constraints(t2[:6], [0, 1, 21]))
    # through the C ABI: a matrix the program does not read, and a program of another context
    rep, pub = _lib.eon_constraint_report(), to_limbs([[0, 1, 21]])[0]
    tp = ctypes.c_void_p(t2.data_ptr())

    def raw(ctx, pre_ptr, perm_ptr):
        rc = ctx.lib.eon_check_constraints_dev(ctx.handle, fib.handle, tp, pre_ptr, perm_ptr, n,
                                               pub.ctypes.data_as(ctypes.c_void_p), 3, None, 0, None, ctypes.byref(rep))
        return rc, ctx.lib.eon_last_error(ctx.handle)

    assert raw(gpu_ctx, None, None)[0] == _lib.EON_OK and rep.failures == 0
    rc, msg = raw(gpu_ctx, tp, None)
    assert rc == _lib.EON_E_ARG and b"pre_trace must be null" in msg
    rc, msg = raw(gpu_ctx, None, tp)
    assert rc == _lib.EON_E_ARG and b"perm_trace must be null" in msg
    rc, msg = raw(Context(0), None, None)
    assert rc == _lib.EON_E_ARG and b"another context" in msg
    # a program without constraints reports no failure
    empty = program(gpu_ctx, MockAir([], 2))
    assert empty.num_constraints == 0
    assert as_dict(empty.check_constraints(dev(to_limbs(rand_rows(5, n, 2))), per_constraint=True)) == dict(CLEAN, counts=[])


# ---- the native prove ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pcs(gpu_ctx):
    from plonky3_eon_amd.native import NativeKzgPcs

    p = NativeKzgPcs(1024, 12345, gpu_ctx)
    yield p
    p.close()


def assert_same_proof(a, b):
    np.testing.assert_array_equal(a.trace_commit[0], b.trace_commit[0])
    assert len(a.quotient_commit) == len(b.quotient_commit) and len(a.opened) == len(b.opened)
    for x, y in zip(a.quotient_commit, b.quotient_commit):
        np.testing.assert_array_equal(x, y)
    for name in ("preprocessed_commit", "permutation_commit"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None)
        if x is not None:
            np.testing.assert_array_equal(x[0], y[0])
    for r, s in zip(a.opened, b.opened):
        for m in range(len(s.values)):
            for p in range(len(s.values[m])):
                np.testing.assert_array_equal(r.values[m][p], s.values[m][p])
                np.testing.assert_array_equal(r.witnesses[m][p], s.witnesses[m][p])
    assert (a.alpha, a.zeta, a.degree_bits) == (b.alpha, b.zeta, b.degree_bits)


@pytest.mark.parametrize("air", ["fibonacci", "mul_fib_p", "range"])
def test_prove_with_the_check_on_equals_the_prove_without(gpu_ctx, pcs, air):
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    n, kw, pp = 8, {}, None
    if air == "fibonacci":
        prog, rows, kw = program(gpu_ctx, FibonacciAir()), O.fib_trace(0, 1, n), dict(public_values=[0, 1, 21])
    elif air == "mul_fib_p":
        prog, rows = program(gpu_ctx, MulFibPAir()), mul_fib_p_trace(1, 1, n)
        pp = setup_preprocessed(pcs, dev(to_limbs(mul_fib_p_preprocessed(n))))
        kw = dict(preprocessed=pp)
    else:
        rows, pub = range_check_trace(n)
        pre = dev(to_limbs(range_check_preprocessed(n)))
        prog, pp = program(gpu_ctx, RangeCheckAir()), setup_preprocessed(pcs, pre)
        kw = dict(public_values=pub, preprocessed=pp, preprocessed_trace=pre, permutation_challenges=rand_ints(5, 4))
    trace, a, z = dev(to_limbs(rows)), 0x1111222233334444, 0x5555666677778888
    assert pcs.check_constraints is False
    off = prove_native(prog, pcs, trace, a, z, **kw)
    pcs.check_constraints = True
    try:
        assert pcs.check_constraints is True
        on = prove_native(prog, pcs, trace, a, z, **kw)
        assert pcs.last_constraint_report().failures == 0
    finally:
        pcs.check_constraints = False
    assert_same_proof(on, off)
    if pp is not None:
        pp.close()


def failing(pcs, f):
    """the prove with the switch on -> the ConstraintError it raises"""
    from plonky3_eon_amd.native import ConstraintError

    pcs.check_constraints = True
    try:
        with pytest.raises(ConstraintError) as e:
            f()
    finally:
        pcs.check_constraints = False
    return e.value


def report_dict(rep):
    d = as_dict(rep)
    d.pop("counts")
    return d


def test_prove_invalid_mul_air_trace(gpu_ctx, pcs):
    """mul_air.rs's invalid trace (c doubled): with the switch off a proof comes back, as before;
    with it on the prove stops with the mirror's first failure, fixed challenges and Fiat-Shamir alike."""
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants, prove_native

    rows = mul_trace(8, valid=False)
    prog, trace = program(gpu_ctx, MulAir()), dev(to_limbs(rows))
    off = prove_native(prog, pcs, trace, 5, 7)  # the switch is off: a proof, as before
    assert off.degree_bits == 3
    want = MC.summary(MC.check_constraints(MC.main_fn(mul_constraints), rows), prog.num_constraints)
    want.pop("counts")
    assert want["failures"] > 0
    py = O.p2_constants(99, 2, 22)
    consts = Poseidon2Constants([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]],
                                [[lim(v) for v in r] for r in py[2]])
    chal = Challenger(consts)
    for a, z, kw in ((5, 7, {}), (None, None, dict(challenger=chal))):
        err = failing(pcs, lambda: prove_native(prog, pcs, trace, a, z, **kw))
        assert err.code == _lib.EON_E_CONSTRAINT and report_dict(err.report) == want
        assert str(err) == (f"Constraint failed at row {want['row']}: constraint {want['constraint']} of "
                            f"{prog.num_constraints}, expected zero, got 0x{want['value']:064x}")
        assert report_dict(pcs.last_constraint_report()) == want
    # the challenger is left where the check stopped the prove: log_ext_degree, log_degree, the
    # preprocessed width and the trace commitment observed (prover.rs:196-208), alpha not sampled
    exp = Challenger(consts)
    exp.observe(np.stack([lim(3), lim(3), lim(0)]))
    exp.observe_g1(off.trace_commit[0])
    np.testing.assert_array_equal(chal.sample(), exp.sample())


def test_prove_invalid_lookup_trace(gpu_ctx, pcs):
    """lookup_air.rs:112 (val = 1 on row 0 against an all-zero table): the permutation trace is
    generated and its LogUp constraints fail; the mirror's generate_permutation supplies the rows."""
    from plonky3_eon_amd.native import prove_native

    rows, ch = multiset_trace(8, bad=True), rand_ints(21, 2)
    prog, trace = program(gpu_ctx, LookupMultisetEqAir()), dev(to_limbs(rows))
    assert prove_native(prog, pcs, trace, 5, 7, permutation_challenges=ch).degree_bits == 3
    perm = ML.generate_permutation(multiset_terms, rows, None, [], ch, 1)
    want = MC.summary(MC.check_constraints(multiset_constraints, rows, None, perm, [], ch), prog.num_constraints)
    want.pop("counts")
    assert want["failures"] > 0
    err = failing(pcs, lambda: prove_native(prog, pcs, trace, 5, 7, permutation_challenges=ch))
    assert report_dict(err.report) == want
