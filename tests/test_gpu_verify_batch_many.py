"""Many independent verify_batch checks in one pass (eon_kzg_verify_batch_many, csrc/pairing.hip):
k_vb_sums / k_vb_pairs over the blocks of every segment at once, one Miller launch, one
final-exponentiation block per segment, one status per segment.

Real openings over an 8-power SRS (mirror_pairing's commit / open builders) in groups of 0, 1, 3
and 130 openings with -, 1, 2 and 3 distinct points; 130 exceeds the 128 threads of k_vb_sums, so
its commitment block strides.  Every status is compared with verify.verify_batch of that group
alone: exact verdicts, no tolerances."""

import ctypes

import numpy as np
import pytest

import mirror_pairing as M
from mirror_pairing import g2_limbs
from oracle import pairing as E
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 3, 130)
POINTS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def g2a(gpu_ctx):
    from plonky3_eon_amd import verify as V

    out = V.g2_mul(M.ALPHA, ctx=gpu_ctx)
    np.testing.assert_array_equal(out, g2_limbs(E.g2_alpha(M.ALPHA)))
    return out


@pytest.fixture(scope="module")
def groups():
    """The four groups of valid openings [(C, W, v, z)]; in a group with several points the
    openings of the points alternate, so each point's openings are scattered over the group."""
    s = M.srs()
    g1 = [M.open_poly(s, M.PB, 1 << 200)]
    g3 = [M.open_poly(s, M.PA, M.Z1), M.open_poly(s, M.PD, M.Z2), M.open_poly(s, [7, 7, 1, 3], M.Z1)]
    fams = [M.open_progression(s, p0, d, z, 44) for p0, d, z in ((M.PA, M.PD, M.Z2), (M.PB, M.PA, M.R - 2),
                                                                 (M.PD, M.PB, 1 << 253))]
    g130 = [fams[i % 3][i // 3] for i in range(130)]
    out = [[], g1, g3, g130]
    assert tuple(len(g) for g in out) == SIZES
    assert tuple(len({o[3] for o in g}) for g in out) == POINTS
    return out


def _many(ctx, g2a, batch):
    from plonky3_eon_amd import verify as V

    arrays = M.opening_arrays([o for g in batch for o in g])
    return V.verify_batch_many(*arrays, [len(g) for g in batch], g2a, ctx=ctx)


def _single(ctx, g2a, group):
    from plonky3_eon_amd import verify as V

    return V.verify_batch(*M.opening_arrays(group), g2a, ctx=ctx)


def test_honest_groups(gpu_ctx, g2a, groups):
    got = _many(gpu_ctx, g2a, groups)
    assert got == [True] * 4
    assert got == [_single(gpu_ctx, g2a, g) for g in groups]


def _swap_witnesses_of_two_points(group):
    """Swap the witnesses of the first opening and the first one at another point."""
    j = next(i for i, o in enumerate(group) if o[3] != group[0][3])
    out = list(group)
    out[0], out[j] = M.with_witness(group[0], group[j][1]), M.with_witness(group[j], group[0][1])
    return out


@pytest.mark.parametrize("k,tamper", [(1, "value"), (2, "value"), (2, "swap"), (3, "value"), (3, "value-strided"),
                                      (3, "swap")])
def test_a_tampered_group_fails_alone(gpu_ctx, g2a, groups, k, tamper):
    """A value off by one (in group 3 also the one at index 129, which only the strided part of the
    sums reads), or the witnesses of two different points swapped, fails group k and no other."""
    batch = [list(g) for g in groups]
    if tamper == "swap":
        batch[k] = _swap_witnesses_of_two_points(batch[k])
    else:
        i = 129 if tamper == "value-strided" else 0
        batch[k][i] = M.with_value(batch[k][i], batch[k][i][2] + 1)
    got = _many(gpu_ctx, g2a, batch)
    assert got == [s != k for s in range(4)]
    assert _single(gpu_ctx, g2a, batch[k]) is False


def _raw_status(ctx, g2a, batch, arrays=None):
    """eon_kzg_verify_batch_many itself: (return code, statuses)."""
    c, w, v, z = arrays if arrays is not None else M.opening_arrays([o for g in batch for o in g])
    seg = np.concatenate([[0], np.cumsum([len(g) for g in batch])]).astype(np.uint64)
    status = np.full(len(batch), 77, dtype=np.int32)
    rc = ctx.lib.eon_kzg_verify_batch_many(ctx.handle, *[a.ctypes.data_as(ctypes.c_void_p) for a in (c, w, v, z, seg)],
                                           len(batch), g2a.ctypes.data_as(ctypes.c_void_p),
                                           status.ctypes.data_as(ctypes.c_void_p))
    return rc, [int(s) for s in status]


@pytest.mark.parametrize("what", ["off-curve-commitment", "off-curve-witness", "value", "point"])
@pytest.mark.parametrize("k", [1, 3])
def test_a_malformed_group_is_arg_per_segment(gpu_ctx, g2a, groups, k, what):
    """An off-curve point or a non-canonical value in the last opening of group k: that status is
    EON_E_ARG, the call is EON_OK, and the other groups -- group 2 tampered, so that not all of them
    are 1 -- keep their verdicts."""
    from plonky3_eon_amd import _lib

    batch = [list(g) for g in groups]
    batch[2][1] = M.with_value(batch[2][1], batch[2][1][2] + 1)
    arrays = M.opening_arrays([o for g in batch for o in g])
    at = sum(SIZES[:k + 1]) - 1
    raw_r = np.array(O.int_to_limbs(M.R), dtype=np.uint64)  # the modulus itself: not canonical
    if what == "off-curve-commitment":
        arrays[0][at, 4] ^= 1
    elif what == "off-curve-witness":
        arrays[1][at, 4] ^= 1
    elif what == "value":
        arrays[2][at] = raw_r
    else:
        arrays[3][at] = raw_r
    want = [1, 1, 0, 1]
    assert _raw_status(gpu_ctx, g2a, batch) == (0, want)
    want[k] = _lib.EON_E_ARG
    assert _raw_status(gpu_ctx, g2a, batch, arrays) == (0, want)
    # the single call on that group: the same refusal, as a return code
    from plonky3_eon_amd import verify as V

    lo = sum(SIZES[:k])
    with pytest.raises(_lib.EonError) as e:
        V.verify_batch(*[a[lo:at + 1] for a in arrays], g2a, ctx=gpu_ctx)
    assert e.value.code == _lib.EON_E_ARG


@pytest.mark.parametrize("order", [(3, 2, 1, 0), (2, 0, 3, 1), (1, 3, 3, 0, 2, 2)])
def test_groups_in_another_order(gpu_ctx, g2a, groups, order):
    """The statuses follow the groups; groups 1 and 3 are tampered, so a permutation shows."""
    batch = [list(g) for g in groups]
    batch[1][0] = M.with_value(batch[1][0], batch[1][0][2] + 1)
    batch[3] = _swap_witnesses_of_two_points(batch[3])
    verdict = [True, False, True, False]
    assert _many(gpu_ctx, g2a, batch) == verdict
    assert _many(gpu_ctx, g2a, [batch[i] for i in order]) == [verdict[i] for i in order]


def test_empty_calls(gpu_ctx, g2a):
    from plonky3_eon_amd import _lib

    assert _many(gpu_ctx, g2a, []) == []
    assert _many(gpu_ctx, g2a, [[], []]) == [True, True]
    status = np.full(2, 77, dtype=np.int32)
    assert gpu_ctx.lib.eon_kzg_verify_batch_many(gpu_ctx.handle, None, None, None, None, None, 0, None,
                                                 status.ctypes.data_as(ctypes.c_void_p)) == 0
    assert list(status) == [77, 77]
    seg = np.array([0, 0], dtype=np.uint64)
    assert gpu_ctx.lib.eon_kzg_verify_batch_many(gpu_ctx.handle, None, None, None, None,
                                                 seg.ctypes.data_as(ctypes.c_void_p), 1, None,
                                                 status.ctypes.data_as(ctypes.c_void_p)) == _lib.EON_E_ARG  # no g2_alpha
