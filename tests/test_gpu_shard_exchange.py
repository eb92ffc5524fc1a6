"""The two copies around the column-sharded prove's one all_to_all, on the GPU in one process:
eon_shard_pack_rows_dev on every rank's column slice of a random Q x W matrix, the exchange emulated
by permuting blocks in torch (recv_r[g] = send_g[r]), eon_shard_unpack_cols_dev -- every rank's
window must be full[(r R + j) mod Q, :], exactly."""

import numpy as np
import pytest

from oracle import coracle as C

pytestmark = pytest.mark.gpu

SHAPES = [
    # Q, S, W, world
    (16, 2, 5, 3),   # widths 2, 2, 1; the last rank short (R = 6: rows 12..15); the halo wraps past Q
    (64, 8, 60, 4),  # even split
    (64, 8, 60, 7),  # 7 * 10 > 64: the last rank holds 4 rows; widths 9 x 4, 8 x 3
    (8, 2, 6, 5),    # R = 2: rank 4 has no rows, its window still exists
]


@pytest.mark.parametrize("q,s,width,world", SHAPES)
def test_pack_exchange_unpack(gpu_ctx, q, s, width, world):
    import torch

    from plonky3_eon_amd import distributed as D

    full_np = C.random_fr(1000 + q + width + world, q * width).reshape(q, width, 4)
    full = torch.from_numpy(full_np.view(np.int64)).to("cuda:0")
    r_block, wmax = -(-q // world), -(-width // world)
    sends = []
    for g in range(world):
        c0, wl = D.column_range(width, world, g)
        send = D.shard_pack_rows(gpu_ctx, full[:, c0:c0 + wl].contiguous(), width, world, g, s)
        assert tuple(send.shape) == (world, r_block + s, wmax, 4)
        # block h, row j is this rank's slice of row (h R + j) mod Q; the padding column is zero
        rows = torch.tensor([D.window_rows(q, world, h, s) for h in range(world)], device="cuda:0")
        assert torch.equal(send[:, :, :wl], full[rows][:, :, c0:c0 + wl])
        assert not send[:, :, wl:].any()
        sends.append(send)
    for r in range(world):
        recv = torch.stack([sends[g][r] for g in range(world)])  # the all_to_all
        window = D.shard_unpack_cols(gpu_ctx, recv, q, width, s)
        want = full[torch.tensor(D.window_rows(q, world, r, s), device="cuda:0")]
        assert tuple(window.shape) == (r_block + s, width, 4)
        assert torch.equal(window, want), f"rank {r}"


def test_shapes_are_checked(gpu_ctx):
    import torch

    from plonky3_eon_amd import _lib
    from plonky3_eon_amd import distributed as D

    lde = torch.zeros((16, 1, 4), dtype=torch.int64, device="cuda:0")
    with pytest.raises(_lib.EonError) as e:  # 2 columns over 3 ranks
        D.shard_pack_rows(gpu_ctx, lde, 2, 3, 0, 2)
    assert e.value.code == _lib.EON_E_ARG and "more ranks than columns" in str(e.value)
    with pytest.raises(_lib.EonError) as e:  # the slice of rank 0 of 2 over 5 columns is 3 wide
        D.shard_pack_rows(gpu_ctx, lde, 5, 2, 0, 2)
    assert e.value.code == _lib.EON_E_SHAPE
    lde12 = torch.zeros((12, 3, 4), dtype=torch.int64, device="cuda:0")
    with pytest.raises(_lib.EonError) as e:  # Q not a power of two
        D.shard_pack_rows(gpu_ctx, lde12, 5, 2, 0, 2)
    assert e.value.code == _lib.EON_E_SHAPE
