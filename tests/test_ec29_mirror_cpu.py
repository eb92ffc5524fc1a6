"""The big-integer mirror behind tests/test_gpu_ec29.py, checked without a device: it is that file's
reference, so its encodings, its bounds and the expectations its generators emit are held here to
the textbook XYZZ formulas and to oracle/pyoracle.py's affine group law."""

import pytest

import mirror_ec29 as M
from oracle import pyoracle as O

Q = M.Q


def test_limbs_and_borrowed_multiples():
    for v in (0, 1, Q - 1, Q, 8 * Q - 1, (1 << 261) - 1):
        assert M.val(M.limbs(v)) == v and all(x <= M.M29 for x in M.limbs(v))
    for k in (2, 3, 9):
        b = M.kpb(k)
        assert M.val(b) == k * Q and all(x >= M.M29 for x in b[:8]) and all(x < 1 << 30 for x in b)
    assert M.from_words32(M.words32(Q - 1)) == Q - 1


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("mode", M.REP_MODES)
def test_encode_decode_round_trip(mode, lazy):
    rng = M.Rng(11)
    for k in range(1, 40):
        pt = M.multiple(k)
        w = M.encode(pt, rng.z(), M.rep(rng, mode), lazy)
        assert len(w) == 36 and M.decode(w) == pt
        M.check_bounds(w, lazy_zzz_ok=lazy)
    assert M.decode(M.identity_words()) is O.INF
    w = M.encode(M.multiple(3), 5)
    w[18:27] = [0] * 9  # raw ZZ == 0 alone marks the identity
    assert M.decode(w) is O.INF


def test_decode_rejects_a_broken_tuple():
    w = M.encode(M.multiple(7), 12345)
    M.decode(w)
    for word in (0, 9, 18, 27):
        bad = list(w)
        bad[word] ^= 1
        with pytest.raises(AssertionError):
            M.decode(bad)
    neg = list(w)  # (X, Y, ZZ, -ZZZ) is a consistent tuple: of the negated point
    neg[27:] = M.limbs(-M.val(w[27:]) % Q)
    assert M.decode(neg) == O.g1_neg(M.multiple(7))


def test_top_representatives_sit_just_below_their_bounds():
    rng = M.Rng(5)
    for k in range(1, 30):
        w = M.encode(M.multiple(k), rng.z(), M.TOP)
        for l, b in zip(M.split(w), M.BOUND):
            assert M.val(l) < b * Q <= M.val(l) + Q
        with pytest.raises(AssertionError):
            M.encode(M.multiple(k), 3, tuple(t + 1 for t in M.TOP))


def test_lazy_negations():
    rng = M.Rng(6)
    for k in range(1, 30):
        for kz in (0, 1):
            z = rng.z()
            plain = M.encode(M.multiple(k), z, (0, 0, 0, 0))
            w = M.encode(M.multiple(k), z, (7, 3, 1, kz), lazy_zzz=True)
            zzz = M.split(w)[3]
            assert all(x < 1 << 30 for x in zzz) and M.val(zzz) < 3 * Q
            assert M.val(zzz) % Q == M.val(M.split(plain)[3])  # the same ZZZ modulo q
            n = M.limbs(3 * Q - M.val(zzz))  # the normalised value the flip started from
            assert M.val(n) < 2 * Q and M.neg_lazy(n, 3) == zzz
            assert [a + b for a, b in zip(n, zzz)] == M.kpb(3)  # limb by limb, no carry
        a = M.affine_limbs(M.multiple(k), lazy_neg=True)
        assert all(x < 1 << 30 for x in a[9:]) and M.val(a[9:]) < 2 * Q
        assert M.affine_point(a) == M.multiple(k) == M.affine_point(M.affine_limbs(M.multiple(k)))
    assert any(x > M.M29 for x in M.encode(M.multiple(1), 1, M.TOP, True)[27:])


def run_textbook(cs, i):
    """Case i of cs through the textbook formulas -> (affine result, return code)."""
    op = cs.op
    p = None if cs.acc[i] is None else M.tb_tuple(cs.acc[i])
    if op in ("madd", "madd_unchecked", "madd_negsum", "madd_exceptional"):
        a = M.affine_point(cs.arg[i])
        exceptional = (a[0] * p[2] - p[0]) % Q == 0
        r = M.tb_madd(p, a)
        if op == "madd":
            return (M.tb_affine(p), 0) if exceptional else (M.tb_affine(r), 1)
        if op == "madd_exceptional":
            assert exceptional
            return M.tb_affine(r), 1 if r is None else 0
        if exceptional:
            return None, 0
        return (O.g1_neg(M.tb_affine(r)) if op == "madd_negsum" else M.tb_affine(r)), 0
    if op == "dbl_affine":
        a = M.affine_point(cs.arg[i])
        return M.tb_affine(M.tb_dbl((a[0], a[1], 1, 1))), 0
    if op in ("dbl", "dbl_ilp"):
        return M.tb_affine(M.tb_dbl(p)), 0
    q = M.tb_tuple(cs.arg[i])
    r = M.tb_add(p, q)
    if op in ("add", "add_ilp"):
        if (q[0] * p[2] - p[0] * q[2]) % Q == 0:
            return M.tb_affine(p), 2 if r is None else 1
        return M.tb_affine(r), 0
    return M.tb_affine(r), 1 if r is None else 0


GENERIC = ("madd", "madd_unchecked", "madd_negsum", "dbl_affine", "dbl", "add", "add_ilp", "dbl_ilp")
EXCEPTIONAL = ("madd", "madd_exceptional", "madd_unchecked", "madd_negsum", "add", "add_ilp", "acc", "acc_ilp")


def check_against_textbook_and_oracle(cs):
    for i in range(len(cs)):
        pt, code = run_textbook(cs, i)
        assert pt == cs.expect[i] and code == cs.code[i], (cs.op, i)
        for words, lazy_ok in ((cs.acc[i], cs.op in M.LAZY_ZZZ_OPS), (cs.arg[i], True)):
            if words is not None and len(words) == 36 and not M.is_identity(words):
                M.check_bounds(words, lazy_zzz_ok=lazy_ok)  # inputs inside the documented invariant
        if cs.same[i]:
            assert M.decode(getattr(cs, cs.same[i])[i]) == cs.expect[i]


@pytest.mark.parametrize("op", GENERIC)
def test_generic_cases_agree_with_the_textbook_formulas(op):
    cs = M.generic_cases(op, 130, 21)
    assert len(cs) == 130
    check_against_textbook_and_oracle(cs)
    assert all(e is not O.INF for e in cs.expect)


@pytest.mark.parametrize("op", ("acc", "acc_ilp"))
def test_acc_cases_agree_and_cover_the_flag_combinations(op):
    cs = M.acc_cases(op, 200, 22)
    assert len(cs) == 200
    check_against_textbook_and_oracle(cs)
    flags = {(M.is_identity(a), M.is_identity(b)) for a, b in zip(cs.acc, cs.arg)}
    assert len(flags) == 4
    assert {0, 1} == set(cs.code) and {None, "acc", "arg"} == set(cs.same)


@pytest.mark.parametrize("op", EXCEPTIONAL)
def test_exceptional_cases_agree_with_the_textbook_formulas(op):
    cs = M.exceptional_cases(op, 48, 23)
    assert len(cs) == 48
    check_against_textbook_and_oracle(cs)
    for i in range(len(cs)):  # equal points never come as equal limbs
        arg = cs.arg[i]
        assert cs.acc[i][:9] != arg[:9] and (len(arg) == 18 or cs.acc[i][18:27] != arg[18:27])


def test_every_class_appears_in_a_short_run():
    """65 cases hold every representative mode with and without the lazy ZZZ, on both sides."""
    cs = M.generic_cases("add", 65, 1)
    seen = set()
    for a, b in zip(cs.acc, cs.arg):
        seen.add((max(a[27:]) > M.M29, max(b[27:]) > M.M29, M.val(a[:9]) // Q, M.val(b[:9]) // Q))
    for la in (False, True):
        for lb in (False, True):
            assert (la, lb, 0, 0) in seen and (la, lb, 7, 7) in seen
    cs = M.generic_cases("madd_negsum", 65, 1)
    assert not any(max(a[27:]) > M.M29 for a in cs.acc)  # no caller passes it a lazy ZZZ
    lazy_y = [max(b[9:]) > M.M29 for b in cs.arg]
    tops = [M.val(a[:9]) // Q == 7 and M.val(a[9:18]) // Q == 3 for a in cs.acc]
    assert {(True, True), (True, False), (False, True), (False, False)} <= set(zip(lazy_y, tops))


def test_chain_plan_matches_the_oracle_and_is_never_exceptional():
    plan = M.chain_plan(9, 31)
    sums = M.chain_sums(plan)
    assert len(plan) == 9 and all(len(ch) == M.CHAIN_STEPS + 1 for ch in plan)
    for ch, ss in zip(plan, sums):
        t = None
        for j, ((pt, ng), s) in enumerate(zip(ch, ss)):
            a = O.g1_neg(pt) if ng else pt
            if t is not None:
                assert (a[0] * t[2] - t[0]) % Q != 0  # x(acc) != x(base)
            t = (a[0], a[1], 1, 1) if t is None else M.tb_madd(t, a)
            assert M.tb_affine(t) == s
    assert {ng for ch in plan for _, ng in ch} == {False, True}


def test_conversion_cases():
    cs = M.to_xyzz_cases(65, 41)
    assert len(cs) == 65 and sum(cs.code) == 9
    for w, e, c in zip(cs.acc, cs.expect, cs.code):
        assert len(e) == 36 and e[32:] == [0] * 4
        if c:
            assert M.is_identity(w) and any(w[:18]) and M.from_words32(e[:8]) == O.R_MOD_Q and not any(e[16:])
        else:
            # radix-2^32 Montgomery (x 2^256) coordinates of the same point
            X, Y, ZZ, ZZZ = (O.fq_from_mont(M.from_words32(e[8 * j:8 * j + 8])) for j in range(4))
            assert (X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q) == M.decode(w)
    cs = M.neg_lazy_cases(65, 43)
    assert len(cs) == 65
    for w, e in zip(cs.acc, cs.expect):
        assert M.val(w[:9]) < Q and M.val(w[27:]) < 2 * Q and e[9:27] == w[9:27]
        assert M.val(e[:9]) == 2 * Q - M.val(w[:9]) and M.val(e[27:]) == 3 * Q - M.val(w[27:])
        assert all(x < 1 << 30 for x in e)
    assert {M.val(w[27:]) for w in cs.acc} >= {0, 2 * Q - 1}
    cs = M.roundtrip_cases(65, 42)
    assert len(cs) == 65
    vals = {M.val(w[9 * j:9 * j + 9]) for w in cs.acc for j in range(4)}
    assert {0, 1, Q - 1} <= vals and all(v < Q for v in vals)
    for w, e in zip(cs.acc, cs.expect):
        assert [M.from_words32(e[8 * j:8 * j + 8]) for j in range(4)] == [M.val(l) for l in M.split(w)]
