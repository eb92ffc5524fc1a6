"""Segmented pairing products (eon_multi_pairing_many, csrc/pairing.hip): one Miller launch over
every pair, one final-exponentiation block per segment.  Bit for bit on the eon_fq12 limbs against
verify.multi_pairing / verify.pairing of the same slices (themselves pinned to the oracle in
test_gpu_pairing.py and test_gpu_pairing_edges.py):

* segments of 0, 1, 2, 9 and 17 pairs: 9 crosses the 8 teams of one Miller block, 17 those of two,
  and the segment boundaries fall inside Miller blocks; the empty segment is the identity of Gt;
* 33 one-pair segments against 33 pairing calls;
* nseg = 0 writes nothing; the argument rejections of eon_multi_pairing, and those of the offsets;
* (P, Q), (-P, Q) in one segment is the identity."""

import ctypes

import numpy as np
import pytest

from mirror_pairing import g1_limbs, g2_limbs, gt_limbs
from oracle import pairing as E
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

ONE = gt_limbs(E.f12_one())
SIZES = (0, 1, 2, 9, 17)


@pytest.fixture(scope="module")
def pairs33():
    """33 pairs (a_i G1, b_i G2), a_i and b_i random 16-bit scalars, as limb arrays."""
    rng = np.random.default_rng(2024)
    ab = rng.integers(1, 1 << 16, (33, 2))
    p = np.stack([g1_limbs(O.g1_mul(O.G1_GEN, int(a))) for a, _ in ab])
    q = np.stack([g2_limbs(E.g2_mul(E.G2_GEN, int(b))) for _, b in ab])
    return p, q


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _raw_many(ctx, p, q, seg, nseg, out):
    seg = np.ascontiguousarray(seg, dtype=np.uint64)
    return ctx.lib.eon_multi_pairing_many(ctx.handle, _ptr(p), _ptr(q), _ptr(seg), nseg, _ptr(out))


@pytest.mark.parametrize("order", [SIZES, SIZES[::-1], (17, 0, 9, 0, 2, 1)])
def test_segments_equal_multi_pairing_of_each_slice(gpu_ctx, pairs33, order):
    from plonky3_eon_amd import verify as V

    p, q = pairs33
    m = sum(order)
    got = V.multi_pairing_many(p[:m], q[:m], order, ctx=gpu_ctx)
    assert got.shape == (len(order), 12, 4)
    at = 0
    for s, size in enumerate(order):
        want = V.multi_pairing(p[at:at + size], q[at:at + size], ctx=gpu_ctx)
        np.testing.assert_array_equal(got[s], want, err_msg=f"segment {s} of {order}")
        if size == 0:
            np.testing.assert_array_equal(got[s], ONE)
        at += size


def test_one_pair_segments_equal_pairing_calls(gpu_ctx, pairs33):
    from plonky3_eon_amd import verify as V

    p, q = pairs33
    got = V.multi_pairing_many(p, q, [1] * 33, ctx=gpu_ctx)
    for i in range(33):
        np.testing.assert_array_equal(got[i], V.pairing(p[i], q[i], ctx=gpu_ctx), err_msg=f"pair {i}")
    # distinct pairs give distinct values: an index slip between segments would show
    assert len({got[i].tobytes() for i in range(33)}) == 33


def test_one_segment_is_multi_pairing(gpu_ctx, pairs33):
    from plonky3_eon_amd import verify as V

    p, q = pairs33
    np.testing.assert_array_equal(V.multi_pairing_many(p[:9], q[:9], [9], ctx=gpu_ctx)[0],
                                  V.multi_pairing(p[:9], q[:9], ctx=gpu_ctx))


def test_only_empty_segments(gpu_ctx):
    from plonky3_eon_amd import verify as V

    got = V.multi_pairing_many(np.zeros((0, 8), np.uint64), np.zeros((0, 16), np.uint64), [0, 0, 0], ctx=gpu_ctx)
    for s in range(3):
        np.testing.assert_array_equal(got[s], ONE)


def test_no_segments_writes_nothing(gpu_ctx, pairs33):
    p, q = pairs33
    out = np.full((2, 12, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    keep = out.copy()
    assert _raw_many(gpu_ctx, p, q, [0], 0, out) == 0
    assert gpu_ctx.lib.eon_multi_pairing_many(gpu_ctx.handle, None, None, None, 0, None) == 0
    np.testing.assert_array_equal(out, keep)


def test_cancelling_pairs_in_one_segment(gpu_ctx, pairs33):
    """(P, Q) and (-P, Q) in one segment: the identity; the neighbours keep their values."""
    from plonky3_eon_amd import verify as V

    p, q = pairs33
    neg = p[3].copy()
    y = sum(int(v) << (64 * i) for i, v in enumerate(p[3][4:]))
    assert y  # not the identity
    neg[4:] = np.array(O.int_to_limbs(O.Q - y), dtype=np.uint64)  # the Montgomery residue of -y
    ps = np.stack([p[0], p[3], neg, p[1]])
    qs = np.stack([q[0], q[3], q[3], q[1]])
    got = V.multi_pairing_many(ps, qs, [1, 2, 1], ctx=gpu_ctx)
    np.testing.assert_array_equal(got[1], ONE)
    np.testing.assert_array_equal(got[0], V.pairing(p[0], q[0], ctx=gpu_ctx))
    np.testing.assert_array_equal(got[2], V.pairing(p[1], q[1], ctx=gpu_ctx))


@pytest.mark.parametrize("which", ["g1-off-curve", "g2-off-curve", "g1-coordinate", "g2-coordinate"])
def test_rejects_what_multi_pairing_rejects(gpu_ctx, pairs33, which):
    """A bad point in the second Miller block of the last segment is EON_E_ARG for the call, as in
    eon_multi_pairing; the context computes the same segments afterwards."""
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd import verify as V

    p, q = pairs33[0][:12].copy(), pairs33[1][:12].copy()
    raw_q = np.array(O.int_to_limbs(O.Q), dtype=np.uint64)  # the modulus itself: not canonical
    if which == "g1-off-curve":
        p[10, 4] ^= 1
    elif which == "g2-off-curve":
        q[10, 0] ^= 1
    elif which == "g1-coordinate":
        p[10, 0:4] = raw_q
    else:
        q[10, 0:4] = raw_q
    with pytest.raises(_lib.EonError) as e:
        V.multi_pairing_many(p, q, [1, 2, 9], ctx=gpu_ctx)
    assert e.value.code == _lib.EON_E_ARG
    with pytest.raises(_lib.EonError) as e:
        V.multi_pairing(p, q, ctx=gpu_ctx)
    assert e.value.code == _lib.EON_E_ARG
    good = V.multi_pairing_many(pairs33[0][:12], pairs33[1][:12], [1, 2, 9], ctx=gpu_ctx)
    np.testing.assert_array_equal(good[1], V.multi_pairing(pairs33[0][1:3], pairs33[1][1:3], ctx=gpu_ctx))


def test_rejects_null_arguments_and_bad_offsets(gpu_ctx, pairs33):
    from plonky3_eon_amd import _lib

    p, q = pairs33
    out = np.zeros((2, 12, 4), np.uint64)
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    seg = np.array([0, 1, 3], dtype=np.uint64)
    assert lib.eon_multi_pairing_many(h, _ptr(p), _ptr(q), _ptr(seg), 2, None) == _lib.EON_E_ARG
    assert lib.eon_multi_pairing_many(h, _ptr(p), _ptr(q), None, 2, _ptr(out)) == _lib.EON_E_ARG
    assert lib.eon_multi_pairing_many(h, None, _ptr(q), _ptr(seg), 2, _ptr(out)) == _lib.EON_E_ARG
    assert lib.eon_multi_pairing_many(h, _ptr(p), None, _ptr(seg), 2, _ptr(out)) == _lib.EON_E_ARG
    assert _raw_many(gpu_ctx, p, q, [1, 2, 3], 2, out) == _lib.EON_E_ARG  # seg[0] != 0
    assert _raw_many(gpu_ctx, p, q, [0, 3, 2], 2, out) == _lib.EON_E_ARG  # descending
    assert _raw_many(gpu_ctx, p, q, [0, 1, (1 << 24) + 1], 2, out) == _lib.EON_E_SHAPE  # as eon_multi_pairing's limit
    assert not out.any()
    assert _raw_many(gpu_ctx, p, q, [0, 1, 3], 2, out) == 0 and out.any()
