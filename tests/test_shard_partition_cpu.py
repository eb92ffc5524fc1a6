"""The partition of the column-sharded prove (no GPU): eon_shard_column_range / eon_shard_row_range
of libeonhip.so and their Python twins in plonky3_eon_amd.distributed agree and have the properties
the driver, the pack / unpack kernels and the tests rely on."""

import ctypes

import pytest

from plonky3_eon_amd import _lib
from plonky3_eon_amd import distributed as D


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def c_columns(lib, width, world, rank):
    c0, wl = ctypes.c_uint32(7), ctypes.c_uint32(7)
    rc = lib.eon_shard_column_range(width, world, rank, ctypes.byref(c0), ctypes.byref(wl))
    return rc, c0.value, wl.value


def c_rows(lib, q, world, rank):
    r0, n = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = lib.eon_shard_row_range(q, world, rank, ctypes.byref(r0), ctypes.byref(n))
    return rc, r0.value, n.value


def test_column_ranges_tile_the_width(lib):
    """every (W, world) with 1 <= world <= W <= 40: contiguous, in rank order, sizes differing by
    at most one with the wider ranges first, widest = ceil(W / world); C and Python agree"""
    for width in range(1, 41):
        for world in range(1, width + 1):
            at, sizes = 0, []
            for rank in range(world):
                rc, c0, wl = c_columns(lib, width, world, rank)
                assert rc == 0 and (c0, wl) == D.column_range(width, world, rank), (width, world, rank)
                assert c0 == at and wl >= 1
                at += wl
                sizes.append(wl)
            assert at == width
            assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
            assert max(sizes) == -(-width // world)


def test_more_ranks_than_columns_is_refused(lib):
    for width, world in [(2, 3), (1, 2), (40, 41), (5, 8)]:
        for rank in range(world):  # every rank decides alike, from (width, world) alone
            assert c_columns(lib, width, world, rank)[0] == _lib.EON_E_ARG
            with pytest.raises(_lib.EonError) as e:
                D.column_range(width, world, rank)
            assert e.value.code == _lib.EON_E_ARG and "more ranks than columns" in str(e.value)
    assert c_columns(lib, 4, 0, 0)[0] == _lib.EON_E_ARG
    assert c_columns(lib, 4, 2, 2)[0] == _lib.EON_E_ARG
    assert lib.eon_shard_column_range(4, 2, 0, None, None) == _lib.EON_E_ARG
    with pytest.raises(_lib.EonError):
        D.column_range(4, 2, 2)


def test_row_ranges_and_windows(lib):
    """Q a power of two, any world: blocks of R = ceil(Q / world) rows in rank order tile [0, Q),
    trailing ranks short or empty; window row t of rank r is row r R + t, its next row t + S is row
    (r R + t + S) mod Q -- the row pair the unsharded quotient reads"""
    for log_q in range(0, 8):
        q = 1 << log_q
        for world in range(1, 41):
            r_block = -(-q // world)
            at = 0
            for rank in range(world):
                rc, row0, n = c_rows(lib, q, world, rank)
                assert rc == 0 and (row0, n) == D.shard_row_range(q, world, rank), (q, world, rank)
                assert row0 == min(q, rank * r_block) and 0 <= n <= r_block
                assert row0 == at or (n == 0 and row0 == q)
                at += n
                for log_s in range(0, log_q + 1):
                    s = 1 << log_s
                    win = D.window_rows(q, world, rank, s)
                    assert len(win) == r_block + s
                    assert win == [(rank * r_block + j) % q for j in range(r_block + s)]
                    for t in range(n):
                        assert win[t] == row0 + t and win[t + s] == (row0 + t + s) % q
            assert at == q
    assert c_rows(lib, 8, 0, 0)[0] == _lib.EON_E_ARG
    assert c_rows(lib, 8, 2, 2)[0] == _lib.EON_E_ARG
    assert c_rows(lib, 0, 1, 0)[0] == _lib.EON_E_ARG
