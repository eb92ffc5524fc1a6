"""Every radix-2^29 curve formula of the MSM bucket sums (csrc/ec29.h) on its own, one formula per
thread through eon_diag_ec29_op, against big-integer group arithmetic (mirror_ec29.py on the Python
oracle's affine law).  Everything is exact: the decoded group element, the coordinate bounds
ec29.h documents for each result, the return code; nothing is skipped, and every test counts what
it checked.

A whole MSM reaches these formulas with whatever representatives random data gives -- near the
bottom of their ranges.  Here the accumulators come at k q above the canonical value for k = 0,
the largest k inside the invariant (X < 8q, Y < 4q, ZZ, ZZZ < 2q) and random k, and with ZZZ
lazily negated (limbs < 2^30, below 3q) for the formulas whose callers can pass that (the list is
in mirror_ec29.py); exceptional additions use a different z on each side."""

import ctypes

import numpy as np
import pytest

import mirror_ec29 as M
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

SIZES = [1, 65, 1000]  # one lane, a wave and a lane, 15 waves and a partial one


def u32(rows):
    return None if rows[0] is None else np.array(rows, dtype=np.uint32)


def run(ctx, cs, op=None):
    out, code = ctx.diag_ec29_op(op or cs.op, u32(cs.acc), u32(cs.arg))
    assert out.shape == (len(cs), 36) and code.shape == (len(cs),)
    return [[int(x) for x in row] for row in out], [int(c) for c in code]


def shifts(n, classes):
    """A run of one case is repeated for every input class; longer runs hold them all."""
    return range(classes) if n == 1 else (0,)


def check_exact(cs, out, code, bounds, inf_by_code=False):
    """Return codes, word-for-word copies, decoded points and result bounds -> cases checked.  An
    identity result is 36 zero words, or with inf_by_code the return code alone."""
    checked = 0
    for i in range(len(cs)):
        assert code[i] == cs.code[i], (cs.op, i, code[i], cs.code[i])
        if cs.same[i]:
            assert out[i] == getattr(cs, cs.same[i])[i], (cs.op, i)
        elif cs.expect[i] is O.INF:
            assert inf_by_code or out[i] == [0] * 36, (cs.op, i)
        else:
            assert M.decode(out[i]) == cs.expect[i], (cs.op, i)
            M.check_bounds(out[i], *bounds)
        checked += 1
    return checked


GENERIC = ("madd", "madd_unchecked", "madd_negsum", "dbl_affine", "dbl", "add", "add_ilp", "dbl_ilp")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", GENERIC)
def test_generic(gpu_ctx, op, n):
    """acc + A, -(acc + A) for madd29_negsum (with +y and the lazy -y), 2A, 2P, P + Q."""
    checked = generated = 0
    for s in shifts(n, 12):
        cs = M.generic_cases(op, n, 100 + n, s)
        out, code = run(gpu_ctx, cs)
        generated += len(cs)
        checked += check_exact(cs, out, code, M.OUT_BOUNDS[op])
    assert checked == generated == n * len(shifts(n, 12))


def test_add_variants_give_the_same_point(gpu_ctx):
    a, b = M.generic_cases("add", 65, 7), M.generic_cases("add_ilp", 65, 7)
    assert a.acc == b.acc and a.arg == b.arg
    (oa, ca), (ob, cb) = run(gpu_ctx, a), run(gpu_ctx, b)
    assert ca == cb == [0] * 65
    assert [M.decode(w) for w in oa] == [M.decode(w) for w in ob] == a.expect
    a, b = M.generic_cases("dbl", 65, 8), M.generic_cases("dbl_ilp", 65, 8)
    assert a.acc == b.acc
    assert [M.decode(w) for w in run(gpu_ctx, a)[0]] == [M.decode(w) for w in run(gpu_ctx, b)[0]] == a.expect


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", ("acc", "acc_ilp"))
def test_acc_identity_flags(gpu_ctx, op, n):
    """All four flag combinations; an identity input passes the other side through word for word
    (ld_raw29 / st_raw29), P + P doubles, P + (-P) stores 36 zero words with the flag set."""
    checked = generated = 0
    for s in shifts(n, 48):
        cs = M.acc_cases(op, n, 200 + n, s)
        out, code = run(gpu_ctx, cs)
        generated += len(cs)
        checked += check_exact(cs, out, code, (8, 2) if op == "acc" else (8, 4))
    assert checked == generated == n * len(shifts(n, 48))


def launches(cs, n):
    """cs as the entry point gets it: one case per launch for n == 1, else all at once."""
    step = 1 if n == 1 else len(cs)
    for lo in range(0, len(cs), step):
        part = M.Cases(cs.op)
        for i in range(lo, lo + step):
            part.add(cs.acc[i], cs.arg[i], cs.expect[i], cs.code[i], cs.same[i])
        yield part


@pytest.mark.parametrize("n", SIZES)
def test_madd_exceptional(gpu_ctx, n):
    """madd29 on acc == A and acc == -A returns false and leaves acc as it was; madd29_exceptional
    then gives 2A, respectively reports the identity."""
    n_cases = max(n, 12)
    cs = M.exceptional_cases("madd", n_cases, 300 + n)
    ex = M.exceptional_cases("madd_exceptional", n_cases, 300 + n)
    assert cs.acc == ex.acc and cs.arg == ex.arg and set(ex.code) == {0, 1}
    checked = 0
    for part in launches(cs, n):
        out, code = run(gpu_ctx, part)
        checked += check_exact(part, out, code, M.OUT_BOUNDS["madd"])
    for part in launches(ex, n):
        out, code = run(gpu_ctx, part)  # A == -acc: the return value 1 is the whole result
        checked += check_exact(part, out, code, M.OUT_BOUNDS["madd_exceptional"], inf_by_code=True)
    assert checked == 2 * n_cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", ("madd_unchecked", "madd_negsum"))
def test_unchecked_exception_parks_zz_at_zero(gpu_ctx, op, n):
    """The invariant k_piece_sum29's flush relies on: after an exceptional unchecked addition ZZ is
    0 modulo q (is_zero_mod29: the value 0 or q), and it stays so under a further addition of an
    unrelated base, fed back in as the loop's next step."""
    n_cases = max(n, 12)
    cs = M.exceptional_cases(op, n_cases, 400 + n)
    checked = 0
    for part in launches(cs, n):
        out, code = run(gpu_ctx, part)
        nxt = M.Cases(op)
        for i, w in enumerate(out):
            assert M.zz_is_zero_mod(w) and code[i] == 0, (op, checked + i)
            M.check_bounds(w, 8, 2)  # the bounds are arithmetic, not the group's: they hold all the same
            unrelated = M.multiple(M.K_MAX + 1 + (checked + i) % 50)
            nxt.add(w, M.affine_limbs(unrelated, lazy_neg=(op == "madd_negsum" and i % 2 == 1)), None, 0)
        out2, code2 = run(gpu_ctx, nxt)
        for i, w in enumerate(out2):
            assert M.zz_is_zero_mod(w) and code2[i] == 0, (op, checked + i)
            M.check_bounds(w, 8, 2)
        checked += len(part)
    assert checked == n_cases


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ilp", (False, True))
def test_add_exceptional(gpu_ctx, ilp, n):
    """Q == P: code 1, Q == -P: code 2, p unchanged either way; acc29 on the same inputs then
    gives 2P and the identity."""
    n_cases = max(n, 12)
    add, acc = ("add_ilp", "acc_ilp") if ilp else ("add", "acc")
    a, b = M.exceptional_cases(add, n_cases, 500 + n), M.exceptional_cases(acc, n_cases, 500 + n)
    assert a.acc == b.acc and a.arg == b.arg and set(a.code) == {1, 2}
    checked = 0
    for cs, bounds in ((a, M.OUT_BOUNDS[add]), (b, (6, 4) if ilp else (6, 2))):
        for part in launches(cs, n):
            out, code = run(gpu_ctx, part)
            checked += check_exact(part, out, code, bounds)
    assert checked == 2 * n_cases


@pytest.mark.parametrize("op", ("madd_negsum", "madd_unchecked"))
def test_chain_as_the_piece_loop_drives_it(gpu_ctx, op):
    """16 additions per chain, 65 chains in step, driven as k_piece_sum29 drives its run: the run
    opens with the unnegated base, madd29_negsum's accumulator holds (-1)^flip times the sum, the
    next base goes in with sign neg_digit != flip as a lazy negation of y, flip toggles every step,
    and the flush negates ZZZ lazily when flip is set.  The bounds are checked after every step."""
    n = 65
    plan = M.chain_plan(n, 77)
    sums = M.chain_sums(plan)
    negsum = op == "madd_negsum"
    acc = [M.affine_acc(ch[0][0] if negsum or not ch[0][1] else O.g1_neg(ch[0][0])) for ch in plan]
    flip = [negsum and ch[0][1] for ch in plan]
    checked = 0
    for j in range(1, M.CHAIN_STEPS + 1):
        cs = M.Cases(op)
        for c in range(n):
            pt, neg_digit = plan[c][j]
            if negsum:
                ng = neg_digit != flip[c]
                arg = M.affine_limbs(O.g1_neg(pt), lazy_neg=True) if ng else M.affine_limbs(pt)
                flip[c] = not flip[c]
            else:
                arg = M.affine_limbs(O.g1_neg(pt) if neg_digit else pt)
            cs.add(acc[c], arg, O.g1_neg(sums[c][j]) if flip[c] else sums[c][j], 0)
        acc, code = run(gpu_ctx, cs)
        checked += check_exact(cs, acc, code, M.OUT_BOUNDS[op])
    assert checked == n * M.CHAIN_STEPS
    # the flush: neg29_lazy<3> of ZZZ where flip is set, by the device's own negation, which must
    # be the mirror's
    neg = M.Cases("neg_lazy")
    for c in range(n):
        neg.add(M.limbs(0) + acc[c][9:], None, None, 0)
    negated, _ = run(gpu_ctx, neg)
    flushed = 0
    for c in range(n):
        w = list(acc[c])
        assert not M.zz_is_zero_mod(w)
        if flip[c]:
            w[27:] = negated[c][27:]
            assert w[27:] == M.neg_lazy(acc[c][27:], 3)
        M.check_bounds(w, 8, 2, lazy_zzz_ok=True)
        assert M.decode(w) == sums[c][-1]
        acc[c] = w
        flushed += 1
    assert flushed == n and (not negsum or {True, False} == set(flip))
    # the flushed pieces go on as the reductions read them: piece c + piece c + 1 by acc29
    cs = M.Cases("acc")
    for c in range(n - 1):
        e = O.g1_add(sums[c][-1], sums[c + 1][-1])
        cs.add(acc[c], acc[c + 1], e, 1 if e is O.INF else 0)
    out, code = run(gpu_ctx, cs)
    assert check_exact(cs, out, code, (8, 2)) == n - 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", ("to_xyzz", "x29_to_xyzz"))
def test_raw29_to_xyzz(gpu_ctx, op, n):
    """Top-of-bound and lazily negated accumulators -> the canonical radix-2^32 Montgomery
    coordinates of the same representatives; raw ZZ == 0 -> xyzz_inf() whatever the other words."""
    checked = generated = 0
    for s in shifts(n, 42):
        cs = M.to_xyzz_cases(n, 600 + n, s)
        out, code = run(gpu_ctx, cs, op)
        generated += len(cs)
        for i in range(len(cs)):
            assert out[i] == cs.expect[i] and code[i] == cs.code[i], i
            checked += 1
    assert checked == generated == n * len(shifts(n, 42))


@pytest.mark.parametrize("n", SIZES)
def test_neg29_lazy(gpu_ctx, n):
    """2q - y and 3q - ZZZ limb by limb against the borrowed-limb constants, 0 and the largest
    admitted values included: limbs below 2^30, no carry, the other coordinates untouched."""
    cs = M.neg_lazy_cases(max(n, 4), 650 + n)
    out, code = run(gpu_ctx, cs)
    checked = 0
    for i in range(len(cs)):
        assert out[i] == cs.expect[i] and code[i] == 0, i
        checked += 1
    assert checked == max(n, 4)


@pytest.mark.parametrize("n", SIZES)
def test_fq256_fq261_round_trip(gpu_ctx, n):
    cs = M.roundtrip_cases(max(n, 3), 700 + n)
    out, code = run(gpu_ctx, cs)
    checked = 0
    for i in range(len(cs)):
        assert out[i] == cs.expect[i] and code[i] == 0, i
        checked += 1
    assert checked == max(n, 3)


def test_refusals_leave_the_context_usable(gpu_ctx):
    from plonky3_eon_amd import _lib

    lib, h = gpu_ctx.lib, gpu_ctx.handle
    a = np.array([M.encode(M.multiple(3), 5)] * 4, dtype=np.uint32)
    b = np.array([M.encode(M.multiple(4), 6)] * 4, dtype=np.uint32)
    out, code = np.zeros((4, 36), dtype=np.uint32), np.zeros(4, dtype=np.int32)
    a_in = a.copy()
    p = [x.ctypes.data_as(ctypes.c_void_p) for x in (a, b, out, code)]
    n_ops = len(M.OPS)
    assert gpu_ctx.EC29_OPS == M.OPS
    assert lib.eon_diag_ec29_op(h, n_ops, p[0], p[1], 4, p[2], p[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_ec29_op(h, 0xFFFFFFFF, p[0], p[1], 4, p[2], p[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_ec29_op(h, 6, p[0], p[1], (1 << 20) + 1, p[2], p[3]) == _lib.EON_E_ARG
    for hole in range(4):
        q = list(p)
        q[hole] = None
        assert lib.eon_diag_ec29_op(h, 6, q[0], q[1], 4, q[2], q[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_ec29_op(h, 0, p[0], None, 4, p[2], p[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_ec29_op(h, 5, None, None, 4, p[2], p[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_ec29_op(None, 6, p[0], p[1], 4, p[2], p[3]) == _lib.EON_E_ARG
    assert not out.any() and not code.any()
    assert lib.eon_diag_ec29_op(h, 6, None, None, 0, None, None) == 0  # nothing to do
    assert lib.eon_diag_ec29_op(h, 5, p[0], None, 4, p[2], p[3]) == 0  # dbl29 reads no argument
    np.testing.assert_array_equal(a, a_in)
    assert [M.decode([int(x) for x in w]) for w in out] == [M.multiple(6)] * 4
    cs = M.generic_cases("add", 65, 3)
    o, c = run(gpu_ctx, cs)
    assert check_exact(cs, o, c, M.OUT_BOUNDS["add"]) == 65
