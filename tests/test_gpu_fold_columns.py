"""eon_fr_fold_columns_dev (csrc/fold.hip): out[i] = scale * sum_j gamma^j mat[i][j], bit-exact
against Python integers.

The kernel as built: a wave takes a row and walks it in TILE = 64-column tiles (one Horner step of
gamma^64 per tile, lane l on column 64 t + l); the loads of UNROLL = 4 tiles (256 columns) are issued
ahead of their steps and the remaining tiles go one by one; a block is WAVES = 4 waves = 4 rows; the
grid is capped at MAX_BLOCKS = 2048 blocks, so from 8192 rows on a wave takes more than one row.
Widths and row counts sit at, one below and one above each of these boundaries.

The reference works on the Montgomery residues themselves: the fold is linear and gamma^j, scale
enter as plain integers, so out_residue = scale * sum_j gamma^j residue_j mod r."""

import ctypes

import numpy as np
import pytest

from oracle import coracle as C

pytestmark = pytest.mark.gpu

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
TILE, UNROLL, WAVES, MAX_BLOCKS = 64, 4, 4, 2048
GAMMA = 0x2B1C9E0F77A1D3C5B6E4F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D % P
SCALE = 0x1F2E3D4C5B6A79888796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F0 % P


def residues(limbs):
    """(..., 4) u64 limbs -> flat list of the residues as Python ints (no Montgomery conversion)"""
    a = np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def limbs_of(values):
    return np.array([[(v >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


def reference(mat_limbs, rows, width, gamma, scale):
    x = residues(mat_limbs)
    pw = [pow(gamma, j, P) for j in range(width)]
    s = 1 if scale is None else scale
    return [s * sum(pw[j] * x[i * width + j] for j in range(width)) % P for i in range(rows)]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def run(gpu_ctx, mat, gamma, scale):
    from plonky3_eon_amd.msm import fold_columns

    out = fold_columns(dev(mat), gamma, scale, gpu_ctx)
    import torch

    torch.cuda.synchronize()
    return residues(out.cpu().numpy().view(np.uint64))


def check(gpu_ctx, rows, width, gamma=GAMMA, scale=None, seed=1):
    mat = C.random_fr(seed + 1000 * rows + width, rows * width).reshape(rows, width, 4)
    got = run(gpu_ctx, mat, gamma, scale)
    assert got == reference(mat, rows, width, gamma, scale)
    assert all(v < P for v in got)


@pytest.mark.parametrize("rows", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3])
def test_smallest_shapes(gpu_ctx, rows, width):
    check(gpu_ctx, rows, width)
    check(gpu_ctx, rows, width, scale=SCALE)


def test_width_one_is_a_scaled_copy(gpu_ctx):
    mat = C.random_fr(3, 9).reshape(9, 1, 4)
    assert run(gpu_ctx, mat, GAMMA, None) == residues(mat)
    assert run(gpu_ctx, mat, 0, None) == residues(mat)  # gamma^0 = 1, also for gamma = 0
    assert run(gpu_ctx, mat, GAMMA, SCALE) == [SCALE * x % P for x in residues(mat)]


# one tile, the unrolled group of four tiles, two groups; rows 5 = one more than a block
@pytest.mark.parametrize("width", [TILE - 1, TILE, TILE + 1, UNROLL * TILE - 1, UNROLL * TILE, UNROLL * TILE + 1,
                                   2 * UNROLL * TILE - 1, 2 * UNROLL * TILE, 2 * UNROLL * TILE + 1,
                                   (UNROLL + 1) * TILE, (UNROLL + 1) * TILE + 1])
def test_width_at_tile_and_unroll_boundaries(gpu_ctx, width):
    check(gpu_ctx, WAVES + 1, width, scale=SCALE)


# a block's four rows; the grid cap, past which a wave's loop makes a second trip (8193 x 65 is
# 2^19.02 elements; 2 x 8192 + 3 rows x 3 puts every wave through two trips and some through three)
@pytest.mark.parametrize("rows,width", [(WAVES - 1, 3), (WAVES, 3), (WAVES + 1, 3), (WAVES + 1, TILE + 1),
                                        (MAX_BLOCKS * WAVES - 1, 3), (MAX_BLOCKS * WAVES, 3),
                                        (MAX_BLOCKS * WAVES + 1, 3), (MAX_BLOCKS * WAVES + 1, TILE + 1),
                                        (2 * MAX_BLOCKS * WAVES + 3, 3)])
def test_rows_at_block_and_grid_boundaries(gpu_ctx, rows, width):
    assert rows * width <= 1 << 20
    check(gpu_ctx, rows, width)


@pytest.mark.parametrize("rows,width", [(64, 1312), (8, 9168)], ids=["poseidon2_vl8", "blake3"])
def test_committed_widths(gpu_ctx, rows, width):
    check(gpu_ctx, rows, width)
    check(gpu_ctx, rows, width, scale=SCALE, seed=2)


@pytest.mark.parametrize("scale", [None, SCALE], ids=["noscale", "scale"])
@pytest.mark.parametrize("gamma", [0, 1, P - 1, GAMMA], ids=["zero", "one", "minus_one", "random"])
def test_gamma_and_scale_values(gpu_ctx, gamma, scale):
    check(gpu_ctx, 9, 2 * TILE + 2, gamma, scale)
    if scale is not None:
        for s in (0, 1, P - 1):
            check(gpu_ctx, 5, TILE + 1, gamma, s)


@pytest.mark.parametrize("scale", [None, P - 1], ids=["noscale", "scale"])
def test_bound_case_all_operands_at_the_maximum(gpu_ctx, scale):
    """every entry the largest residue r - 1, gamma = r - 1, at the widest committed shape: the lazy
    accumulators at their largest"""
    rows, width = 8, 9168
    mat = np.tile(limbs_of([P - 1]), (rows * width, 1)).reshape(rows, width, 4)
    assert run(gpu_ctx, mat, P - 1, scale) == reference(mat, rows, width, P - 1, scale)
    # and the largest terms that do not cancel: gamma = 1
    assert run(gpu_ctx, mat, 1, scale) == reference(mat, rows, width, 1, scale)


def raw(gpu_ctx, mat_ptr, rows, width, gamma, scale, out_ptr):
    from plonky3_eon_amd.field import fr_to_abi

    g = fr_to_abi(gamma) if gamma is not None else None
    s = fr_to_abi(scale) if scale is not None else None
    return gpu_ctx.lib.eon_fr_fold_columns_dev(gpu_ctx.handle, mat_ptr, rows, width,
                                               ctypes.byref(g) if g is not None else None,
                                               ctypes.byref(s) if s is not None else None, out_ptr)


def test_argument_errors(gpu_ctx):
    import torch

    from plonky3_eon_amd import _lib

    gpu_ctx.set_stream(None)
    rows, width = 4, 5
    mat = dev(C.random_fr(4, rows * width).reshape(rows, width, 4))
    out = torch.full((rows, 4), -1, dtype=torch.int64, device="cuda:0")
    mp, op = ctypes.c_void_p(mat.data_ptr()), ctypes.c_void_p(out.data_ptr())
    p_limbs = tuple(int(x) for x in limbs_of([P])[0])  # r itself: not canonical
    assert raw(gpu_ctx, mp, rows, width, p_limbs, None, op) == _lib.EON_E_ARG
    assert raw(gpu_ctx, mp, rows, width, GAMMA, p_limbs, op) == _lib.EON_E_ARG
    assert raw(gpu_ctx, None, rows, width, GAMMA, None, op) == _lib.EON_E_ARG
    assert raw(gpu_ctx, mp, rows, width, GAMMA, None, None) == _lib.EON_E_ARG
    assert raw(gpu_ctx, mp, rows, width, None, None, op) == _lib.EON_E_ARG
    # out inside mat
    assert raw(gpu_ctx, mp, rows, width, GAMMA, None, ctypes.c_void_p(mat.data_ptr() + 64)) == _lib.EON_E_ARG
    torch.cuda.synchronize()
    assert bool((out == -1).all())  # none of the refused calls wrote
    # rows == 0 writes nothing (and reads no pointer); width == 0 writes zeros
    assert raw(gpu_ctx, None, 0, width, None, None, None) == _lib.EON_OK
    assert raw(gpu_ctx, mp, 0, width, GAMMA, None, op) == _lib.EON_OK
    torch.cuda.synchronize()
    assert bool((out == -1).all())
    assert raw(gpu_ctx, None, rows, 0, None, None, None) == _lib.EON_E_ARG
    assert raw(gpu_ctx, None, rows, 0, GAMMA, None, op) == _lib.EON_OK
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    # the context still works
    check(gpu_ctx, 3, 7)
