"""The batched KZG opening restated with Python integers (tests/mirror_batched.py), checked on the
CPU against the trapdoor identity: for a matrix with column commitments C_j, opened values v_j at z
and ONE witness W,   sum_j gamma^j C_j - [sum_j gamma^j v_j] G1 = (s - z) W   (s the test SRS's
trapdoor), which is verify_single's pairing equation with the pairing replaced by s.  An 8 x 3 and
an 8 x 1 matrix, two points each."""

import random

import numpy as np

import mirror_batched as MB
from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V

P = O.P
SRS_ALPHA = 12345
GAMMA = 0x0123456789ABCDEF0123456789ABCDEF
DELTA = 0x0FEDCBA9876543210FEDCBA987654321


def matrices(seed=5):
    rng = random.Random(seed)
    return [[[rng.randrange(P) for _ in range(w)] for _ in range(8)] for w in (3, 1)]


def folded_commitment(mat, gamma):
    """sum_j gamma^j C_j from the columns' own commitments (points, one CPU MSM)"""
    width = len(mat[0])
    cols = [MB.point(MB.commit_dlog([row[j] for row in mat], SRS_ALPHA)) for j in range(width)]
    return cols, C.g1_msm(np.stack(cols), np.stack([V.fr_limbs(pow(gamma, j, P)) for j in range(width)]))


def test_fold_is_the_gamma_combination_of_the_columns():
    mat = matrices()[0]
    assert MB.fold(mat, 0) == [row[0] for row in mat]
    assert MB.fold(mat, 1) == [sum(row) % P for row in mat]
    assert MB.fold(mat, GAMMA, 7) == [7 * (row[0] + GAMMA * row[1] + GAMMA * GAMMA * row[2]) % P for row in mat]
    assert MB.fold([], GAMMA) == [] and MB.fold([[], []], GAMMA) == [0, 0]


def test_quotient_and_eval_is_the_division_by_x_minus_z():
    f = matrices()[1]
    col = [row[0] for row in f]
    z = 0xABCDEF
    q, v = MB.quotient_and_eval(col, z)
    assert len(q) == 7 and v == MB.commit_dlog(col, z)
    # f(X) - v = (X - z) q(X), coefficient by coefficient
    prod = [0] * 8
    for i, c in enumerate(q):
        prod[i + 1] = (prod[i + 1] + c) % P
        prod[i] = (prod[i] - z * c) % P
    assert prod == [(col[0] - v) % P] + col[1:]


def test_batched_witnesses_satisfy_the_trapdoor_identity():
    mats = matrices()
    zs = [0x1111222233334444, 0x5555666677778888 % P]
    values, wits = MB.open_batched_coeffs(mats, [zs, zs], GAMMA, SRS_ALPHA)
    claims = []
    for mat, vals, ws in zip(mats, values, wits):
        cols, folded = folded_commitment(mat, GAMMA)
        for z, v, w in zip(zs, vals, ws):
            assert v == [MB.commit_dlog([row[j] for row in mat], z) for j in range(len(mat[0]))]
            # sum gamma^j C_j - [sum gamma^j v_j] G1 == (s - z) W, as one claim of the oracle's check
            assert V.kzg_claims_identity([(folded, z, MB.fold([v], GAMMA)[0], MB.point(w))], SRS_ALPHA)
            claims.append((np.stack(cols), v, MB.point(w), z))
    assert MB.verify(claims, GAMMA, DELTA, SRS_ALPHA) and MB.verify(claims, GAMMA, 1, SRS_ALPHA)
    # a wrong value, a wrong witness, another gamma: rejected
    c0 = claims[0]
    assert not MB.verify([(c0[0], [(c0[1][0] + 1) % P] + c0[1][1:], c0[2], c0[3])] + claims[1:], GAMMA, DELTA, SRS_ALPHA)
    assert not MB.verify([(c0[0], c0[1], claims[1][2], c0[3])] + claims[1:], GAMMA, DELTA, SRS_ALPHA)
    assert not MB.verify(claims, GAMMA + 1, DELTA, SRS_ALPHA)


def test_width_one_witness_is_the_per_column_witness():
    mat = matrices()[1]
    col = [row[0] for row in mat]
    z = 0x77
    _, wits = MB.open_batched_coeffs([mat], [[z]], GAMMA, SRS_ALPHA)
    assert wits[0][0] == MB.commit_dlog(MB.quotient_and_eval(col, z)[0], SRS_ALPHA)
    # and as a point: commit_column(quotient_and_eval(...)) over the SRS powers
    srs = C.g1_srs(8, V.fr_limbs(SRS_ALPHA))
    q = np.stack([V.fr_limbs(c) for c in MB.quotient_and_eval(col, z)[0]])
    np.testing.assert_array_equal(MB.point(wits[0][0]), C.g1_msm(srs[:7], q))


def test_evaluation_route_agrees_with_the_coefficient_route():
    """the GPU tests feed the mirror evaluations on the trace domain (shift 1)"""
    mats = matrices(9)
    zs = [0x1234567, 0x89ABCDEF]
    want_v, want_w = MB.open_batched_coeffs(mats, [zs, zs], GAMMA, SRS_ALPHA)
    w = MB.two_adic_generator(3)
    for mat, wv, ww in zip(mats, want_v, want_w):
        width = len(mat[0])
        evals = [[MB.commit_dlog([row[j] for row in mat], pow(w, i, P)) for j in range(width)] for i in range(8)]
        v, wit = MB.open_batched_evals(evals, 3, zs, GAMMA, SRS_ALPHA)
        assert v == wv and wit == ww


def test_a_cancelling_pair_passes_unweighted_and_fails_weighted():
    """W_0 + (s - z_1) E and W_1 - (s - z_0) E cancel in the unweighted product of two claims on one
    matrix; the delta weights tell them apart"""
    mat = matrices()[0]
    zs = [0x1111, 0x2222]
    values, wits = MB.open_batched_coeffs([mat], [zs], GAMMA, SRS_ALPHA)
    cols, _ = folded_commitment(mat, GAMMA)
    e = 0xE
    w0 = (wits[0][0] + (SRS_ALPHA - zs[1]) * e) % P
    w1 = (wits[0][1] - (SRS_ALPHA - zs[0]) * e) % P
    claims = [(np.stack(cols), values[0][0], MB.point(w0), zs[0]), (np.stack(cols), values[0][1], MB.point(w1), zs[1])]
    assert MB.verify(claims, GAMMA, 1, SRS_ALPHA)
    assert not MB.verify(claims, GAMMA, DELTA, SRS_ALPHA)
