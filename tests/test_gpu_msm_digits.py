"""The MSM digit pipeline stage by stage (msm_digits.hip: k_msm_digits, k_msm_digits4, the fused
k_digit_sort_pass over DigitSource, the radix sort, k_bucket_start, the piece offsets) against the
Python recoding of mirror_msm_digits: what a prepared handle keeps of every batch is read back and
compared exactly, on every digit route and at window widths forced through EON_MSM_FORCE_C to reach
the one-pass, three-pass and fused sorts at test sizes.  The commitments of the same call are
compared with the C Pippenger."""

import random

import numpy as np
import pytest

from mirror_msm_digits import (SENTINEL, bucket_of, chunk_counts, edge_scalars, exclusive_sum_u32, recode,
                               reference_pairs)
from oracle import coracle as C
from oracle import pyoracle as O
from plonky3_eon_amd.msm import MsmBases, srs_powers

pytestmark = pytest.mark.gpu

R = O.P


def choose_c(n, fixed):
    """msm_bases.hip choose_c: the width minimising n W mixed additions + 6 additions per bucket."""
    best, best_cost = 4, float("inf")
    for c in range(4, 21):
        W = (255 + c - 1) // c
        cost = float(n) * W + 6.0 * float(1 << (c - 1)) * (1.0 if fixed else W)
        if cost < best_cost:
            best, best_cost = c, cost
    return best


def to_matrix(cols):
    """cols[j][i] canonical ints -> (rows, width, 4) Montgomery limbs."""
    return np.array([[O.int_to_limbs(O.to_mont(cols[j][i])) for j in range(len(cols))]
                     for i in range(len(cols[0]))], dtype=np.uint64)


def column(kind, rows, c, seed, thin=False):
    """One column of a kind.  `thin`: the r - 1 column holds r - 1 in every third row and the edge
    column an edge value in every eighth, random scalars elsewhere (see test_fused_sort_many_groups)."""
    rng = random.Random(seed)
    if kind == "zero":
        return [0] * rows
    if kind == "random":
        return [rng.randrange(R) for _ in range(rows)]
    if kind == "r-1":
        if thin:
            return [R - 1 if i % 3 == 0 else rng.randrange(R) for i in range(rows)]
        return [R - 1] * rows
    edge = edge_scalars(c, R)
    if thin:
        return [edge[(i // 8) % len(edge)] if i % 8 == 0 else rng.randrange(R) for i in range(rows)]
    return [edge[i % len(edge)] for i in range(rows)]


KINDS = ["zero", "random", "r-1", "edge"]


def check_batches(prep, cols, fixed, c, unfused):
    """Every batch of `prep` against the reference pairs of its columns; -> the most pieces one
    bucket holds."""
    rows = len(cols[0])
    max_pieces = 0
    nbatches = prep.num_batches()
    assert nbatches >= 1
    covered = 0
    for k in range(nbatches):
        r = prep.read_batch(k)
        W, ref_windows, groups, nb = r["windows"], r["ref_windows"], r["groups"], r["nb"]
        assert r["c"] == c and r["col0"] == covered
        assert ref_windows == (255 + c - 1) // c and W <= ref_windows
        assert groups == (r["cols"] if fixed else r["cols"] * W) and nb == groups << (c - 1)
        assert r["pairs"] == rows * W * r["cols"]
        covered += r["cols"]
        # recode asserts that the windows above W hold no nonzero digit (no carry out of window W - 1)
        rk, rv = reference_pairs(cols[r["col0"]:r["col0"] + r["cols"]], c, W, ref_windows, fixed)
        live = rk != SENTINEL
        n_pairs = int(live.sum())
        keys, vals = r["keys"], r["vals"]
        assert r["n_pairs"] == n_pairs
        assert (keys[n_pairs:] == SENTINEL).all() and not vals[n_pairs:].any()
        assert (keys[:n_pairs] != SENTINEL).all()
        b = bucket_of(keys, c, groups, nb)
        assert (np.diff(b) >= 0).all(), "buckets are not contiguous runs in bucket order"
        assert n_pairs == 0 or b[n_pairs - 1] < nb
        # every bucket's multiset at once: both sides ordered by (bucket, value)
        rb = bucket_of(rk[live], c, groups, nb)
        o_dev = np.lexsort((vals[:n_pairs], b[:n_pairs]))
        o_ref = np.lexsort((rv[live], rb))
        np.testing.assert_array_equal(keys[:n_pairs][o_dev], rk[live][o_ref])
        np.testing.assert_array_equal(vals[:n_pairs][o_dev], rv[live][o_ref])
        if unfused:  # the stable sort of the group-major emission on the low c key bits, exactly
            idx = np.argsort(rk & np.uint32((1 << c) - 1), kind="stable")
            np.testing.assert_array_equal(keys, rk[idx])
            np.testing.assert_array_equal(vals, rv[idx])
        np.testing.assert_array_equal(r["start"], np.searchsorted(b, np.arange(nb + 1), side="left"))
        assert 4 <= r["log_chunk"] <= 7
        counts = chunk_counts(r["start"], r["log_chunk"])
        max_pieces = max(max_pieces, int(counts.max()))
        want_off = exclusive_sum_u32(counts.astype(np.uint32))
        np.testing.assert_array_equal(r["piece_off"], want_off)
        assert r["n_pieces"] == int(r["piece_off"][nb])
    assert covered == len(cols)
    return max_pieces


def run_case(ctx, rows, width, fixed, c, kernel, seed, thin=False):
    """Prepare `width` columns of the four kinds (in as many calls as it takes to show each kind),
    read every batch back and check it; -> (the last call's profiled kernels, the most pieces one
    bucket held in any call)."""
    import torch

    pts = srs_powers(rows, 777, ctx)
    bases = MsmBases(pts, ctx, precompute=fixed)
    fused = kernel == "k_digit_sort_pass"
    seen, max_pieces = [], 0
    for call in range((len(KINDS) + width - 1) // width):
        kinds = [KINDS[(call * width + j) % len(KINDS)] for j in range(width)]
        cols = [column(kd, rows, c, seed + 100 * call + j, thin) for j, kd in enumerate(kinds)]
        mat = to_matrix(cols)
        ctx.profile(True)
        try:
            got, prep = bases.prepare_columns(torch.from_numpy(mat.view(np.int64)).to("cuda:0"))
            kernels = ctx.profile_report()
        finally:
            ctx.profile(False)
        digit_kernels = {"k_msm_digits", "k_msm_digits4", "k_digit_sort_pass"} & set(kernels)
        assert digit_kernels == {kernel}, sorted(kernels)
        assert ("k_msm_digit_hist" in kernels) == fused
        max_pieces = max(max_pieces, check_batches(prep, cols, fixed, c, unfused=not fused))
        for j in range(width):
            np.testing.assert_array_equal(got[j], C.g1_msm(pts, mat[:, j]), err_msg=f"column {j} ({kinds[j]})")
        prep.close()
        seen += [s for col in cols for s in col]
        last_kernels = kernels
    bases.close()
    # the edge coverage is real: some scalar has a raw window of exactly 2^(c-1), and some carries
    # into the top window
    W = (255 + c - 1) // c
    exact_b = top_carry = False
    for s in set(seen):
        _, raws, _ = recode(s, c, W)
        exact_b |= (1 << (c - 1)) in raws
        top_carry |= raws[W - 1] == ((s >> (c * (W - 1))) & ((1 << c) - 1)) + 1
    assert exact_b and top_carry
    return last_kernels, max_pieces


@pytest.mark.parametrize("fixed", [True, False])
def test_digits_one_row_per_thread(gpu_ctx, monkeypatch, fixed):
    """k_msm_digits (203 rows: not a multiple of 4), the fixed-base keys (group = column, reference
    = row x windows + window) and the plain ones (group = column x window, reference = row), at the
    width choose_c picks."""
    monkeypatch.delenv("EON_MSM_FORCE_C", raising=False)
    rows = 203
    run_case(gpu_ctx, rows, 3, fixed, choose_c(rows, fixed), "k_msm_digits", 11)


def test_digits_four_rows_per_thread(gpu_ctx, monkeypatch):
    """k_msm_digits4<true> at its own width: 256 rows x 5 columns (a 4-column tile and a 1-column one)."""
    monkeypatch.delenv("EON_MSM_FORCE_C", raising=False)
    run_case(gpu_ctx, 256, 5, True, choose_c(256, True), "k_msm_digits4", 12)


def test_digits_four_rows_c16_unfused(gpu_ctx, monkeypatch):
    """c = 16 with 1028 rows (no whole 1024-row tiles): k_msm_digits4<true> and two stored passes."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "16")
    run_case(gpu_ctx, 1028, 5, True, 16, "k_msm_digits4", 13)


@pytest.mark.parametrize("rows", [1024, 2048])
def test_fused_digit_sort_buckets(gpu_ctx, monkeypatch, rows):
    """The fused first pass ranks a column's pairs in another order than the stored route; what the
    piece sums rely on is checked here: every (magnitude, column) bucket is one contiguous run, in
    bucket order, holding exactly the reference's pairs, and start / piece_off describe those runs.
    2048 rows: two tiles per column, ten tiles of look-back."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "16")
    run_case(gpu_ctx, rows, 5, True, 16, "k_digit_sort_pass", 14 + rows)


@pytest.mark.parametrize("c", [4, 8])
def test_one_sort_pass(gpu_ctx, monkeypatch, c):
    """c <= 8: a single sort pass (runtime digit width at 4, the compile-time 8)."""
    monkeypatch.setenv("EON_MSM_FORCE_C", str(c))
    run_case(gpu_ctx, 512, 2, True, c, "k_msm_digits4", 20 + c)


@pytest.mark.parametrize("c", [17, 20])
def test_three_sort_passes(gpu_ctx, monkeypatch, c):
    """17..20 key bits: three passes of uneven widths; at c = 20 the 2^20 + 1 bucket starts take
    the piece-offset scan into its 257th block."""
    monkeypatch.setenv("EON_MSM_FORCE_C", str(c))
    run_case(gpu_ctx, 512, 2, True, c, "k_msm_digits4", 30 + c)


@pytest.mark.parametrize("thin", [False, True])
def test_fused_sort_many_groups(gpu_ctx, monkeypatch, thin):
    """66 columns (>= 64 groups) at c = 16 under the fused sort.  A fixed-base column shares one
    bucket set among its 16 windows, so a whole column of one scalar (r - 1 in all 1024 rows) and
    the edge column's repeated patterns (every window at 2^15) put more than 32 pieces into one
    bucket: two combine levels, which takes the batch off the fused bucket reduction.  `thin`
    therefore keeps r - 1 in every third row and an edge value in every eighth, which leaves at
    most 32 pieces in any bucket, and asserts that the call-wide fused reduction ran.  Both piece
    counts are read off the batch."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "16")
    kernels, max_pieces = run_case(gpu_ctx, 1024, 66, True, 16, "k_digit_sort_pass", 40, thin=thin)
    if thin:
        assert max_pieces <= 32
        assert "bucket_reduce" in kernels and "k_group_finish" in kernels, sorted(kernels)
    else:
        assert max_pieces > 32 and "k_group_finish" not in kernels, sorted(kernels)


def single_column(bits, rows, c, seed):
    """Scalars below 2^bits whose largest is 2^bits - 1 (every window below the top bit at its
    maximum: the recoding carries into the window above), plus the values around it."""
    rng = random.Random(seed)
    col = [rng.randrange(1 << bits) for _ in range(rows)]
    col[:5] = [(1 << bits) - 1, (1 << bits) - (1 << (c - 1)), 1 << (bits - 1), 0, 1]
    return col


@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("bits", [45, 48])
def test_single_msm_window_truncation(gpu_ctx, monkeypatch, bits, fixed):
    """The single MSM digitises only the windows its largest scalar reaches, one more for the carry
    (k_scalar_or, active_windows); fixed-base references stay row x the layout's windows + window.
    Its batch, kept by the diagnostic entry that runs that same route, is compared with the
    reference recoded at the kept window count: the count comes from the info, is the expected
    ceil((bits + 1) / c) -- well below the layout's -- and every window it drops holds only zero
    digits of the reference.  45 bits end on a window edge of both widths (c = 9 fixed-base, c = 5
    plain), so there the top kept digit is the carry's alone."""
    import torch

    monkeypatch.delenv("EON_MSM_FORCE_C", raising=False)
    rows = 300
    c = choose_c(rows, fixed)
    W = (255 + c - 1) // c
    col = single_column(bits, rows, c, bits)
    pts = srs_powers(rows, 777, gpu_ctx)
    bases = MsmBases(pts, gpu_ctx, precompute=fixed)
    mat = to_matrix([col])
    gpu_ctx.profile(True)
    try:
        got, prep = bases.diag_msm_keep_batch(torch.from_numpy(mat[:, 0].view(np.int64)).to("cuda:0"))
        kernels = gpu_ctx.profile_report()
    finally:
        gpu_ctx.profile(False)
    assert "k_msm_digits4" in kernels and "k_digit_sort_pass" not in kernels, sorted(kernels)
    info = prep.read_batch(0, arrays=False)
    kept = info["windows"]
    assert prep.num_batches() == 1 and info["ref_windows"] == W
    assert kept == (bits + 1 + c - 1) // c and kept < W
    reaches_last = False
    for s in col:
        digits = recode(s, c, W)[0]
        assert len(digits[kept:]) == W - kept and not any(digits[kept:]), hex(s)
        reaches_last |= digits[kept - 1] != 0
    assert reaches_last, "no scalar reaches the last kept window: one window fewer would pass too"
    check_batches(prep, [col], fixed, c, unfused=True)
    want = C.g1_msm(pts, mat[:, 0])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(bases.msm(mat[:, 0]), want)
    prep.close()
    bases.close()


def test_prepared_single_column_keeps_every_window(gpu_ctx, monkeypatch):
    """A handle made by prepare_columns never truncates (its digits serve other bases later): one
    column of scalars below 2^48 keeps all of the layout's windows, the high ones all sentinel."""
    import torch

    monkeypatch.delenv("EON_MSM_FORCE_C", raising=False)
    rows = 300
    c = choose_c(rows, True)
    col = single_column(48, rows, c, 5)
    pts = srs_powers(rows, 777, gpu_ctx)
    bases = MsmBases(pts, gpu_ctx, precompute=True)
    mat = to_matrix([col])
    got, prep = bases.prepare_columns(torch.from_numpy(mat.view(np.int64)).to("cuda:0"))
    info = prep.read_batch(0, arrays=False)
    assert prep.num_batches() == 1 and info["windows"] == info["ref_windows"] == (255 + c - 1) // c
    check_batches(prep, [col], True, c, unfused=True)
    np.testing.assert_array_equal(got[0], C.g1_msm(pts, mat[:, 0]))
    prep.close()
    bases.close()
