"""The pairing verifier (csrc/pairing.hip) past one block of pairs and at the group-law edges,
through verify.multi_pairing, verify.verify_batch and verify.g2_mul.

* multi_pairing, bit for bit on the eon_fq12 limbs: pair counts around the 8-team blocks of
  k_miller_team (the clamped idle teams of the last block, a second and a ninth block, a product
  loop in k_final_exp_team longer than 5), infinities and cancellation at the block edges, and
  non-canonical inputs.  The expected values are final exponentiations of cached oracle Miller
  values (tests/mirror_pairing.py), or one oracle pairing by bilinearity.
* verify_batch: the verdict of the reference's unrandomised product (kzg/src/util.rs:245-292) in
  its merged form, mirror_pairing.verify_batch_merged, pinned to the unmerged restatement in
  tests/test_pairing_mirror_cpu.py: 8 to 17 merged pairs, groups and commitment sums past the
  128-thread stride of k_vb_sums, the doubling and inverse branches of the sums, infinities in
  every merged pair, and every bit of the fixed-generator tables k_vb_pairs reads.
* g2_mul at the word boundaries of g2_mul_words."""

import ctypes

import numpy as np
import pytest

import mirror_pairing as M
from mirror_pairing import g1_limbs, g2_limbs, gt_limbs
from oracle import pairing as E
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

G1, G2 = O.G1_GEN, E.G2_GEN
ONE = gt_limbs(E.f12_one())


def _raw(v):
    """The plain (not Montgomery) limbs of v: what a non-canonical field element looks like."""
    return np.array(O.int_to_limbs(v), dtype=np.uint64)


def _ab(i):
    """The scalars of pair i: distinct, a few bits wide."""
    return 3 + 2 * i, 5 + 3 * i


def _pair(i):
    a, b = _ab(i)
    return O.g1_mul(G1, a), E.g2_mul(G2, b)


def _multi_pairing(ctx, pairs):
    from plonky3_eon_amd import verify as V

    return V.multi_pairing(np.stack([g1_limbs(p) for p, _ in pairs]), np.stack([g2_limbs(q) for _, q in pairs]), ctx=ctx)


@pytest.fixture(scope="module")
def pairs17():
    """17 pairs (a_i G1, b_i G2) and their oracle Miller values, computed once."""
    pairs = [_pair(i) for i in range(17)]
    return pairs, [M.miller(p, q) for p, q in pairs]


def _expected(values):
    return gt_limbs(E.final_exponentiation(M.miller_product(values)))


# ---- multi_pairing: pair counts and block edges --------------------------------------------------
@pytest.mark.parametrize("m", [1, 7, 8, 9, 16, 17])
def test_pair_counts_around_the_blocks(gpu_ctx, pairs17, m):
    """7, 8, 9 straddle the first block of 8 teams and 16, 17 the second; with 17 pairs the third
    block holds one real team and seven that recompute pair 16 and must write nothing."""
    pairs, values = pairs17
    np.testing.assert_array_equal(_multi_pairing(gpu_ctx, pairs[:m]), _expected(values[:m]))


def test_infinities_at_block_edges(gpu_ctx, pairs17):
    """P = inf in the last team of block 0, Q = inf in the first team of block 1, both in the only
    real team of block 2 (the one the clamped teams copy): those factors are 1."""
    pairs, values = pairs17
    ps = list(pairs)
    ps[7] = (None, ps[7][1])
    ps[8] = (ps[8][0], None)
    ps[16] = (None, None)
    want = _expected([v for i, v in enumerate(values) if i not in (7, 8, 16)])
    np.testing.assert_array_equal(_multi_pairing(gpu_ctx, ps), want)
    # nine pairs, every one with a point at infinity
    inf9 = [(None, pairs[i][1]) if i % 3 == 0 else (pairs[i][0], None) if i % 3 == 1 else (None, None) for i in range(9)]
    np.testing.assert_array_equal(_multi_pairing(gpu_ctx, inf9), ONE)


def test_cancellation_across_blocks(gpu_ctx, pairs17):
    """e(P, Q) in block 0 and e(-P, Q) in block 1, infinities between: the product is 1."""
    p, q = pairs17[0][0]
    ps = [(p, q)] + [(None, None)] * 7 + [(O.g1_neg(p), q)]
    np.testing.assert_array_equal(_multi_pairing(gpu_ctx, ps), ONE)


def test_repeated_pair(gpu_ctx, pairs17):
    """e(aG1, bG2)^9 = e([9a]G1, [b]G2): the same pair in every team of block 0 and in block 1."""
    p, q = pairs17[0][0]
    a, _ = _ab(0)
    np.testing.assert_array_equal(_multi_pairing(gpu_ctx, [(p, q)] * 9), gt_limbs(E.pairing(O.g1_mul(G1, 9 * a), q)))


def test_many_blocks(gpu_ctx):
    """67 pairs: nine blocks, the last with three real teams.  prod e(a_i G1, b_i G2) =
    e([sum a_i b_i]G1, G2), the reduced Gt value being unique."""
    m = 67
    k = sum(a * b for a, b in map(_ab, range(m))) % M.R
    np.testing.assert_array_equal(_multi_pairing(gpu_ctx, [_pair(i) for i in range(m)]),
                                  gt_limbs(E.pairing(O.g1_mul(G1, k), G2)))


@pytest.mark.parametrize("which", ["g1", "g2"])
def test_rejects_a_non_canonical_coordinate_in_the_second_block(gpu_ctx, pairs17, which):
    """A coordinate equal to q at index 8 of 9 pairs is EON_E_ARG, and the context computes the
    9-pair product afterwards."""
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd import verify as V

    pairs, values = pairs17
    p = np.stack([g1_limbs(x) for x, _ in pairs[:9]])
    q = np.stack([g2_limbs(x) for _, x in pairs[:9]])
    (p if which == "g1" else q)[8, 0:4] = _raw(O.Q)
    with pytest.raises(_lib.EonError) as e:
        V.multi_pairing(p, q, ctx=gpu_ctx)
    assert e.value.code == _lib.EON_E_ARG
    np.testing.assert_array_equal(_multi_pairing(gpu_ctx, pairs[:9]), _expected(values[:9]))


# ---- verify_batch: verdict parity with the reference ---------------------------------------------
@pytest.fixture(scope="module")
def g2a(gpu_ctx):
    from plonky3_eon_amd import verify as V

    out = V.g2_mul(M.ALPHA, ctx=gpu_ctx)
    np.testing.assert_array_equal(out, g2_limbs(E.g2_alpha(M.ALPHA)))
    return out


def _gpu_verdict(ctx, g2a, openings):
    from plonky3_eon_amd import verify as V

    return V.verify_batch(*M.opening_arrays(openings), g2a, ctx=ctx)


def _check(ctx, g2a, openings, want, why=""):
    """The GPU's verdict is the mirror's, and both are the one the case's reason gives."""
    assert M.verify_batch_merged(openings, M.ALPHA) is want, why
    assert _gpu_verdict(ctx, g2a, openings) is want, why


def _plus_g1(opening):
    return M.with_witness(opening, O.g1_add(opening[1], G1))


@pytest.mark.parametrize("name", list(M.SMALL_VERDICTS))
def test_small_cases(gpu_ctx, g2a, name):
    """mirror_pairing.small_cases: identical openings and cancellation at n = 2, the point edges
    z in {0, 1, r - 1, 2^253, alpha}, the value edges, constant and zero polynomials, and the parity
    cases below.  Each entry of the table states why its verdict follows.

    Parity with the unrandomised reference (kzg/src/util.rs:245-292): its product has no random
    weights, so it accepts v_0 + 1, v_1 - 1 at two points ("compensating") and two witnesses of
    one point swapped ("swapped-within"), and rejects witnesses swapped across points.  These are
    the reference's verdicts, and the merged GPU form must give exactly them."""
    openings, why = M.small_cases()[name]
    _check(gpu_ctx, g2a, openings, M.SMALL_VERDICTS[name], why)


@pytest.fixture(scope="module")
def distinct16():
    """16 points, two valid openings of degree-3 polynomials at each."""
    s = M.srs()
    return [[M.open_poly(s, [1 + j, 2, 3 + 2 * j, 1], 100 + 7 * j), M.open_poly(s, [4, j + 1, 1, 2 + j], 100 + 7 * j)]
            for j in range(16)]


@pytest.mark.parametrize("tamper", ["valid", "first", "last"])
@pytest.mark.parametrize("g", [7, 8, 9, 16])
def test_distinct_points(gpu_ctx, g2a, distinct16, g, tamper):
    """g points give g + 1 merged pairs: 8, 9, 10 and 17, around the Miller blocks.  A witness
    replaced by W + G1 multiplies the product by e(-G1, [alpha - z]G2) != 1, in the first group
    (pair 1) or the last (pair g: the last team of block 0, or a team of block 1 or 2)."""
    groups = [list(x) for x in distinct16[:g]]
    if tamper == "first":
        groups[0][0] = _plus_g1(groups[0][0])
    elif tamper == "last":
        groups[g - 1][1] = _plus_g1(groups[g - 1][1])
    _check(gpu_ctx, g2a, [o for grp in groups for o in grp], tamper == "valid")


@pytest.fixture(scope="module")
def progression257():
    return M.open_progression(M.srs(), M.PA, M.PB, M.Z2, 257)


@pytest.mark.parametrize("tamper", [False, True])
@pytest.mark.parametrize("n", [127, 128, 129, 257])
def test_group_sizes_at_one_point(gpu_ctx, g2a, progression257, n, tamper):
    """One group around the 128 threads of k_vb_sums: below, at, one past, and two strides plus
    one.  The tampered witness (W + G1) is the opening at index 128, the first of a thread's second
    stride, where there is one, and the last opening otherwise."""
    openings = list(progression257[:n])
    if tamper:
        i = min(128, n - 1)
        openings[i] = _plus_g1(openings[i])
    _check(gpu_ctx, g2a, openings, not tamper)


@pytest.mark.parametrize("tamper", [False, True])
def test_257_openings_over_three_points(gpu_ctx, g2a, tamper):
    """The commitment-sum block strides (257 > 128) while the groups (86, 86, 85) do not.  The
    value at index 128 is off by one: only the strided sum of the values sees it."""
    s = M.srs()
    fams = [M.open_progression(s, M.PA, M.PD, z, 86) for z in (M.Z1, M.Z2, 1 << 200)]
    openings = [fams[i % 3][i // 3] for i in range(257)]
    if tamper:
        openings[128] = M.with_value(openings[128], openings[128][2] + 1)
    _check(gpu_ctx, g2a, openings, not tamper)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [2, 129, 256])
def test_identical_openings(gpu_ctx, g2a, n, off):
    """The same valid opening n times: sum C = [n]C through the doubling branch of
    xyzz_add_affine (a thread's stride meets the point again, n > 128) and of xyzz_add (the LDS
    tree adds equal partial sums).  With v + 1 in every copy sum v is off by n."""
    o = M.open_poly(M.srs(), M.PA, M.Z1)
    _check(gpu_ctx, g2a, [M.with_value(o, o[2] + off)] * n, off == 0)


def test_submission_order(gpu_ctx, g2a):
    """12 openings over 3 points in three orders (grouped; interleaved starting at the last
    point; reversed): the grouping by point and the first-seen order of points change, the verdict
    does not."""
    s = M.srs()
    pts = (M.Z1, 1 << 253, M.R - 2)
    base = [M.open_poly(s, [1 + i, 3, i + 2, 5], pts[i // 4]) for i in range(12)]
    orders = [list(range(12)), [4 * ((k + 2) % 3) + k // 3 for k in range(12)], list(range(11, -1, -1))]
    assert all(sorted(o) == list(range(12)) for o in orders)
    for tampered, want in ((None, True), (6, False)):
        batch = [(_plus_g1(o) if i == tampered else o) for i, o in enumerate(base)]
        for order in orders:
            _check(gpu_ctx, g2a, [batch[i] for i in order], want, f"order {order}")


@pytest.mark.parametrize("lo", [0, 64, 128, 192])
def test_bit_sweep_of_the_fixed_generator_sums(gpu_ctx, g2a, lo):
    """p(x) = c_0 + x opened at z = 2^i with value v = 2^((37 i + 11) mod 254): W = G1,
    c_0 = v - z, C = [c_0 + alpha]G1, valid by construction.  [z]G2 reads exactly entry i of
    G2_POW2 and [v]G1 exactly one entry of G1_POW2 (37 is coprime to 254, so the 254 values use
    every entry once): a wrong entry, word index or shift on either side answers False.  Two
    wrong values per chunk keep a sweep that always answers True from passing."""
    hi = min(lo + 64, 254)
    for i in range(lo, hi):
        z, v = 1 << i, 1 << ((37 * i + 11) % 254)
        c = O.g1_mul(G1, (v - z + M.ALPHA) % M.R)
        assert _gpu_verdict(gpu_ctx, g2a, [(c, G1, v, z)]) is True, i
        if i in (lo, hi - 1):
            assert _gpu_verdict(gpu_ctx, g2a, [(c, G1, (v + z) % M.R, z)]) is False, i


def _raw_verify(ctx, arrays, g2a):
    """eon_kzg_verify_batch itself: (return code, *ok)."""
    c, w, v, z = [np.ascontiguousarray(a, dtype=np.uint64) for a in arrays]
    ok = ctypes.c_int(0)
    rc = ctx.lib.eon_kzg_verify_batch(ctx.handle, *[a.ctypes.data_as(ctypes.c_void_p) for a in (c, w, v, z)],
                                      c.shape[0], g2a.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ok))
    return rc, ok.value


@pytest.mark.parametrize("what", ["value", "point", "commitment-coordinate", "witness-coordinate", "off-curve"])
def test_verify_batch_rejects_bad_arguments(gpu_ctx, g2a, what):
    """A non-canonical value, point or coordinate at index 1 of two openings, or a commitment off
    the curve at the last index, is EON_E_ARG with *ok left 0; the same batch untouched is Ok."""
    from plonky3_eon_amd import _lib

    s = M.srs()
    arrays = M.opening_arrays([M.open_poly(s, M.PA, M.Z1), M.open_poly(s, M.PD, M.Z2)])
    assert _raw_verify(gpu_ctx, arrays, g2a) == (0, 1)
    if what == "value":
        arrays[2][1] = _raw(M.R)
    elif what == "point":
        arrays[3][1] = _raw(M.R)
    elif what == "commitment-coordinate":
        arrays[0][1, 0:4] = _raw(O.Q)
    elif what == "witness-coordinate":
        arrays[1][1, 4:8] = _raw(O.Q)
    else:
        arrays[0][1, 4] ^= 1
    assert _raw_verify(gpu_ctx, arrays, g2a) == (_lib.EON_E_ARG, 0)
    from plonky3_eon_amd import verify as V

    with pytest.raises(_lib.EonError) as e:
        V.verify_batch(*arrays, g2a, ctx=gpu_ctx)
    assert e.value.code == _lib.EON_E_ARG


# ---- g2_mul --------------------------------------------------------------------------------------
def test_g2_mul_at_word_boundaries(gpu_ctx):
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd import verify as V

    for i in (0, 31, 32, 63, 64, 127, 128, 191, 192, 253):
        np.testing.assert_array_equal(V.g2_mul(1 << i, ctx=gpu_ctx), g2_limbs(E.g2_mul(G2, 1 << i)), err_msg=f"2^{i}")
    seven = E.g2_mul(G2, 7)
    np.testing.assert_array_equal(V.g2_mul(M.R - 1, base=g2_limbs(seven), ctx=gpu_ctx), g2_limbs(E.g2_neg(seven)))
    assert not V.g2_mul(12345, base=np.zeros(16, dtype=np.uint64), ctx=gpu_ctx).any()  # a base at infinity
    with pytest.raises(_lib.EonError) as e:
        V.g2_mul(O.int_to_limbs(M.R), ctx=gpu_ctx)  # the limbs of r itself: not a canonical Fr
    assert e.value.code == _lib.EON_E_ARG
