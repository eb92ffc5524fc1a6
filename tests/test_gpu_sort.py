"""The MSM digit pipeline's device-wide primitives on their own (sort.hip, sort_pass.h), through the
diagnostic entry points: the stable LSD radix sort of (u32 key, u32 value) pairs against numpy's
stable argsort, and the two exclusive scans against numpy sums.  Everything is exact.

A bucket sum is order-free, so no MSM result shows a sort that loses stability between passes or a
rank that wraps; these cases do: the tile edges (1024 x 16 = 16384 pairs), one / two / three / four
passes with even and uneven digit widths, one digit holding whole tiles, and the look-back through
tiles with zero counts."""

import ctypes

import numpy as np
import pytest

from mirror_msm_digits import chunk_counts, exclusive_sum_u32

pytestmark = pytest.mark.gpu

TILE = 16384  # sort_pass.h: SORT_THREADS x SORT_ITEMS


def pass_widths(bits):
    """sort.hip split_bits: ceil(bits / 8) passes, the low ones one bit wider when uneven."""
    p = (bits + 7) // 8
    return [bits // p + (1 if q < bits % p else 0) for q in range(p)]


def make_keys(pattern, n, bits, seed):
    rng = np.random.default_rng(seed)
    mask = (1 << bits) - 1
    if pattern == "uniform":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if pattern == "msm":
        # as the digit kernels emit: (group << c) | (|digit| - 1) group-major, one sentinel in 2^15
        c = min(max(bits, 16), 24)
        per_group = 1 << 13
        mag = rng.integers(0, 1 << (c - 1), n, dtype=np.uint64)
        k = ((np.arange(n, dtype=np.uint64) // per_group) << c | mag) & 0xFFFFFFFF
        k[rng.integers(0, 1 << 15, n) == 0] = 0xFFFFFFFF
        return k.astype(np.uint32)
    if pattern == "distinct8":
        vals = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
        return vals[rng.integers(0, 8, n)]
    if pattern == "equal":
        return np.full(n, 0xA5C3F00F, dtype=np.uint32)
    if pattern in ("sorted", "reverse"):
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        k = k[np.argsort(k & np.uint32(mask), kind="stable")]
        return k if pattern == "sorted" else k[::-1].copy()
    if pattern == "lookback":
        # tile 0 all one key; the later tiles never use that key's digit in any pass, so every
        # look-back for it walks through zero counts down to tile 0
        k0 = 0x5A5A5A5A
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        shift = 0
        for w in pass_widths(bits):
            m = np.uint32(((1 << w) - 1) << shift)
            same = (k & m) == (np.uint32(k0) & m)
            k[same] ^= np.uint32(1 << shift)
            shift += w
        k[:min(n, TILE)] = k0
        return k
    raise ValueError(pattern)


def check_sort(ctx, keys, bits, seed, vals=None):
    n = len(keys)
    if vals is None:  # arbitrary u32 values, bit 31 included: an index written instead fails
        vals = np.random.default_rng(seed + 99).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k_in, v_in = keys.copy(), vals.copy()
    k_out, v_out = ctx.diag_radix_sort_pairs(keys, vals, bits)
    np.testing.assert_array_equal(keys, k_in)  # the inputs are left unchanged
    np.testing.assert_array_equal(vals, v_in)
    mask = np.uint32(0xFFFFFFFF if bits == 32 else (1 << bits) - 1)
    idx = np.argsort(keys & mask, kind="stable")
    np.testing.assert_array_equal(k_out, keys[idx])
    np.testing.assert_array_equal(v_out, vals[idx])


SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 5, (1 << 20) + 7]
BITS = [1, 4, 7, 8, 9, 12, 16, 17, 19, 20, 23, 32]
PATTERNS = ["uniform", "msm", "distinct8", "equal", "sorted", "reverse", "lookback"]


@pytest.mark.parametrize("n", SIZES)
def test_sort_sizes(gpu_ctx, n):
    """Every size edge at the MSM's own 16 bits (two 8-bit passes) and at 19 (three passes of
    7 / 6 / 6 bits): below, at and above one tile, several tiles, more than 2^20 pairs."""
    for bits in (16, 19):
        check_sort(gpu_ctx, make_keys("uniform", n, bits, n + bits), bits, n)


@pytest.mark.parametrize("bits", BITS)
def test_sort_bits(gpu_ctx, bits):
    """One pass (runtime and compile-time digit widths), two, three with an uneven split, four:
    the key bits above `bits` do not order and come back unchanged (uniform 32-bit keys)."""
    n = 3 * TILE + 5
    keys = make_keys("uniform", n, bits, bits)
    assert bits == 32 or (keys >> np.uint32(bits)).any()
    check_sort(gpu_ctx, keys, bits, bits)
    check_sort(gpu_ctx, make_keys("msm", n, bits, bits + 1), bits, bits + 1)


@pytest.mark.parametrize("bits", [8, 16, 20, 32])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sort_patterns(gpu_ctx, pattern, bits):
    """n = 5 tiles and a partial one: with all keys equal one digit holds 16384 pairs of every tile
    and 82697 overall (a rank that wraps at 65536 fails); `lookback` walks zero counts."""
    n = 5 * TILE + 777
    check_sort(gpu_ctx, make_keys(pattern, n, bits, 7 * bits + len(pattern)), bits, bits)


def test_sort_values_are_carried_not_indices(gpu_ctx):
    """Values equal to the input index (stability readable off the output) and values that are a
    fixed permutation of it with bit 31 set: both come back as stored."""
    n, bits = 2 * TILE + 1, 12
    keys = make_keys("distinct8", n, bits, 5)
    check_sort(gpu_ctx, keys, bits, 0, vals=np.arange(n, dtype=np.uint32))
    check_sort(gpu_ctx, keys, bits, 0, vals=(np.arange(n, dtype=np.uint32)[::-1] | np.uint32(1 << 31)))


def test_sort_refusals_leave_the_context_usable(gpu_ctx):
    from plonky3_eon_amd import _lib

    lib, h = gpu_ctx.lib, gpu_ctx.handle
    a = np.arange(8, dtype=np.uint32)
    b, c, d = a.copy(), a.copy(), a.copy()
    p = [x.ctypes.data_as(ctypes.c_void_p) for x in (a, b, c, d)]
    assert lib.eon_diag_radix_sort_pairs(h, p[0], p[1], (1 << 24) + 1, 16, p[2], p[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_radix_sort_pairs(h, p[0], p[1], 8, 33, p[2], p[3]) == _lib.EON_E_ARG
    for hole in range(4):
        q = list(p)
        q[hole] = None
        assert lib.eon_diag_radix_sort_pairs(h, q[0], q[1], 8, 16, q[2], q[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_radix_sort_pairs(None, p[0], p[1], 8, 16, p[2], p[3]) == _lib.EON_E_ARG
    assert lib.eon_diag_exclusive_scan_u32(h, p[0], (1 << 24) + 1, p[2]) == _lib.EON_E_ARG
    assert lib.eon_diag_exclusive_scan_u32(h, None, 8, p[2]) == _lib.EON_E_ARG
    mx = ctypes.c_uint32()
    assert lib.eon_diag_scan_chunk_counts(h, p[0], (1 << 24) + 1, 4, p[2], ctypes.byref(mx)) == _lib.EON_E_ARG
    assert lib.eon_diag_scan_chunk_counts(h, p[0], 7, 4, p[2], None) == _lib.EON_E_ARG
    np.testing.assert_array_equal(a, np.arange(8))
    check_sort(gpu_ctx, make_keys("uniform", 1000, 16, 3), 16, 3)


SCAN_SIZES = [0, 1, 255, 256, 4095, 4096, 4097, 256 * 4096, 256 * 4096 + 1, (1 << 20) + 4097]


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan(gpu_ctx, n):
    """Below, at and above one 4096-element block, 256 blocks and the 257th (the second chunk of
    the block-sum scan)."""
    v = np.random.default_rng(n).integers(0, 8, n, dtype=np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(gpu_ctx.diag_exclusive_scan_u32(v), exclusive_sum_u32(v))


def test_exclusive_scan_wraps_modulo_2_32(gpu_ctx):
    n = 3 * 4096 + 17
    v = np.random.default_rng(1).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    assert int(v.astype(np.uint64).sum()) > 1 << 32
    np.testing.assert_array_equal(gpu_ctx.diag_exclusive_scan_u32(v), exclusive_sum_u32(v))


def bucket_starts(nb, chunk, seed):
    """Random bucket sizes, most buckets empty or small, with (where nb allows) a bucket that ends
    exactly on a chunk boundary and one that spans many chunks -> nb + 1 starts."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 4, nb, dtype=np.int64) * (rng.integers(0, 3, nb) > 0)
    if nb >= 8:
        sizes[nb // 2] = 37 * chunk + 3
        sizes[5] = chunk - int(sizes[:5].sum()) % chunk  # bucket 5 is not empty and ends on a boundary
        sizes[6] = 0
    start = np.zeros(nb + 1, dtype=np.int64)
    start[1:] = np.cumsum(sizes)
    return start.astype(np.uint32)


def check_chunk_counts(ctx, start, log_chunk):
    out, mx = ctx.diag_scan_chunk_counts(start, log_chunk)
    cnt = chunk_counts(start, log_chunk)
    np.testing.assert_array_equal(out, exclusive_sum_u32(cnt.astype(np.uint32)))
    assert mx == (int(cnt.max()) if cnt.max() > 1 else 0)


@pytest.mark.parametrize("log_chunk", [4, 7])
@pytest.mark.parametrize("nb", [1, 4096, (1 << 20) + 3])
def test_scan_chunk_counts(gpu_ctx, nb, log_chunk):
    chunk = 1 << log_chunk
    if nb == 1:  # one bucket: empty, one pair, ending on a boundary over many chunks, just past it
        for size in (0, 1, 8 * chunk, 8 * chunk + 1):
            check_chunk_counts(gpu_ctx, np.array([0, size], dtype=np.uint32), log_chunk)
        check_chunk_counts(gpu_ctx, np.array([chunk - 1, chunk + 1], dtype=np.uint32), log_chunk)
    else:
        check_chunk_counts(gpu_ctx, bucket_starts(nb, chunk, nb + log_chunk), log_chunk)


def test_scan_chunk_counts_maximum_threshold(gpu_ctx):
    """The maximum is reported only above 1: 2 where buckets straddle a chunk edge, 0 where every
    bucket is one piece (the combine levels read 0 as `none needed`)."""
    start = np.arange(0, 3001, 3, dtype=np.uint32)  # 3-pair buckets inside 16-pair chunks, some straddle
    out, mx = gpu_ctx.diag_scan_chunk_counts(start, 4)
    cnt = chunk_counts(start, 4)
    assert cnt.max() == 2 and mx == 2
    start = np.arange(0, 16 * 500 + 1, 16, dtype=np.uint32)  # every bucket exactly one chunk
    out, mx = gpu_ctx.diag_scan_chunk_counts(start, 4)
    assert mx == 0
    np.testing.assert_array_equal(out, np.arange(501, dtype=np.uint32))
