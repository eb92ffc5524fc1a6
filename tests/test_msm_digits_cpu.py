"""The Python signed-window recoding the GPU digit tests compare against (mirror_msm_digits),
pinned on its own: for the edge scalars and random ones at every window width the MSM can choose,
the digits sum back to the scalar, stay in [-(B - 1), B] and leave no carry above the top window."""

import random

import numpy as np
import pytest

from mirror_msm_digits import (SENTINEL, bucket_of, chunk_counts, edge_scalars, exclusive_sum_u32, recode,
                               reference_pairs)

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617  # BN254 Fr modulus


def scalars_for(c):
    rng = random.Random(1000 + c)
    return edge_scalars(c, R) + [rng.randrange(R) for _ in range(200)] + [rng.randrange(1 << 48) for _ in range(20)]


@pytest.mark.parametrize("c", range(4, 21))
def test_recoding_sums_to_the_scalar(c):
    W = (255 + c - 1) // c
    B = 1 << (c - 1)
    saw_exact_b = saw_top_carry = saw_zero_after_carry = False
    for s in scalars_for(c):
        assert 0 <= s < R
        digits, raws, carry = recode(s, c, W)
        assert len(digits) == W
        assert sum(d << (c * w) for w, d in enumerate(digits)) == s, hex(s)
        assert all(-(B - 1) <= d <= B for d in digits), hex(s)
        assert carry == 0, hex(s)
        for w, (d, raw) in enumerate(zip(digits, raws)):
            assert d == (raw if raw <= B else raw - (1 << c))
            if raw == B:
                assert d == B  # exactly 2^(c-1) stays positive
                saw_exact_b = True
        saw_top_carry |= raws[W - 1] == ((s >> (c * (W - 1))) & ((1 << c) - 1)) + 1
        saw_zero_after_carry |= any(raw == (1 << c) and d == 0 for d, raw in zip(digits, raws))
    assert saw_exact_b and saw_top_carry and saw_zero_after_carry


def test_edge_scalars_hold_their_patterns():
    """The patterns over the W - 1 low windows are below r, so they reach the recoding intact."""
    for c in range(4, 21):
        W = (255 + c - 1) // c
        B = 1 << (c - 1)
        e = edge_scalars(c, R)
        assert e[:5] == [0, 1, B, B + 1, (1 << c) - 1] and e[-1] == R - 1
        all_b, chain, ripple = e[8], e[9], e[10]
        assert recode(all_b, c, W)[0] == [B] * (W - 1) + [0]
        assert recode(chain, c, W)[0] == [-(B - 1)] + [-(B - 2)] * (W - 2) + [1]
        assert recode(ripple, c, W)[0] == [-(B - 1)] + [0] * (W - 2) + [1]
        assert recode(R - 1, c, W)[1][W - 1] != 0


def test_reference_pairs_layout():
    """Keys, values, groups and the group-major emission on a case small enough to write out."""
    c, W = 4, 3  # B = 8
    cols = [[0x1F8, 0], [7, 0x008]]  # 0x1F8: raws 8, 15, 1 + 1 -> digits 8, -1, 2
    for fixed in (True, False):
        keys, vals = reference_pairs(cols, c, W, ref_windows=5, fixed=fixed)
        n = 2
        want = {}
        for (j, i, w, d) in [(0, 0, 0, 8), (0, 0, 1, -1), (0, 0, 2, 2), (1, 0, 0, 7), (1, 1, 0, 8)]:
            g = j if fixed else j * W + w
            ref = i * 5 + w if fixed else i
            want[(j * W + w) * n + i] = ((g << c) | (abs(d) - 1), ref | ((1 << 31) if d < 0 else 0))
        for e in range(len(keys)):
            assert (int(keys[e]), int(vals[e])) == want.get(e, (SENTINEL, 0)), (fixed, e)
        groups = 2 if fixed else 2 * W
        nb = groups * 8
        b = bucket_of(keys, c, groups, nb)
        assert b[0] == 7 * groups + 0 and (b[keys == SENTINEL] == nb).all()


def test_chunk_counts_and_exclusive_sum():
    start = np.array([0, 0, 16, 17, 17, 49, 64], dtype=np.uint32)  # empty, ends on a boundary, spans chunks
    np.testing.assert_array_equal(chunk_counts(start, 4), [0, 1, 1, 0, 3, 1, 0])
    np.testing.assert_array_equal(exclusive_sum_u32(np.array([3, 0xFFFFFFFF, 5, 1], dtype=np.uint32)),
                                  [0, 3, 2, 7])
    assert len(exclusive_sum_u32(np.zeros(0, dtype=np.uint32))) == 0
