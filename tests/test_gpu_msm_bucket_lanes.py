"""The one-bucket-per-lane piece sums of column batches (k_bucket_order in msm_digits.hip,
k_piece_sum_bucket29 in msm_pieces.hip): the bucket order a prepared batch keeps, read back through
eon_diag_msm_scalars_order and checked exactly, the route every batch reports, and every column against the C Pippenger
restatement (or the Python double-and-add oracle where the bases repeat)."""

import numpy as np
import pytest

from oracle import coracle as C
from oracle import pyoracle as O
from plonky3_eon_amd.msm import MsmBases, srs_powers
from mirror_msm_digits import chunk_counts
from test_gpu_msm_digits import column, to_matrix

pytestmark = pytest.mark.gpu

ORDER_CAP = 1023  # k_bucket_order sorts run lengths up to here; longer ones compare equal (eon.h)
PIECE = 32  # the chunked route's one-level bound: pieces of one bucket (msm_batch.h)


def fr(x):
    return np.array(O.int_to_limbs(O.to_mont(x)), dtype=np.uint64)


def pt(p):
    return np.frombuffer(O.g1_to_bytes(p), dtype=np.uint64).copy()


def as_py(a):
    return O.g1_from_bytes(np.ascontiguousarray(a, dtype=np.uint64).tobytes())


def dev(mat):
    import torch

    return torch.from_numpy(np.ascontiguousarray(mat).view(np.int64)).to("cuda:0")


def check_order(prep):
    """Every batch's order against its own bucket starts: per window a permutation of the window's
    bucket indices, run lengths non-decreasing along it, equal lengths in index order.
    The reported route is the rule's (msm_digits.hip bucket_lanes_route): >= 64 groups, no bucket
    above PIECE pieces of the chunked route, no run above ORDER_CAP.
    -> per batch (bucket_lanes, the run lengths)."""
    out = []
    for k in range(prep.num_batches()):
        r = prep.read_batch(k)
        o = prep.read_order(k)
        nb, win, order = r["nb"], o["window"], o["order"]
        assert win > 0 and order is not None and order.shape == (nb,)
        lens = np.diff(r["start"].astype(np.int64))
        key = np.minimum(lens, ORDER_CAP)
        for w0 in range(0, nb, win):
            w1 = min(w0 + win, nb)
            seg = order[w0:w1].astype(np.int64)
            np.testing.assert_array_equal(np.sort(seg), np.arange(w0, w1), err_msg=f"batch {k} window {w0}")
            assert (np.diff(key[seg]) >= 0).all(), (k, w0)
            ties = np.diff(key[seg]) == 0
            assert (np.diff(seg)[ties] > 0).all(), (k, w0)
            # the three together: the stable sort by length
            np.testing.assert_array_equal(seg, w0 + np.argsort(key[w0:w1], kind="stable"))
        one_level = int(chunk_counts(r["start"], r["log_chunk"]).max()) <= PIECE
        assert o["bucket_lanes"] == (r["groups"] >= 64 and one_level and int(lens.max()) <= ORDER_CAP), k
        out.append((o["bucket_lanes"], lens))
    return out


def prepare_and_check(ctx, pts, mat, precompute=True):
    """prepare_columns over `pts`, every column against the C Pippenger restatement, the order
    checked -> check_order's list."""
    bases = MsmBases(pts, ctx, precompute=precompute)
    got, prep = bases.prepare_columns(dev(mat))
    try:
        for j in range(mat.shape[1]):
            np.testing.assert_array_equal(got[j], C.g1_msm(pts, mat[:, j]), err_msg=f"column {j}")
        return check_order(prep)
    finally:
        prep.close()
        bases.close()


def test_order_runs_of_250(gpu_ctx, monkeypatch):
    """66 fixed-base columns x 1024 rows at c = 8: 8448 buckets (one short window) of ~256 pairs."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "8")
    pts = srs_powers(1024, 4242, gpu_ctx)
    mat = C.random_fr(61, 1024 * 66).reshape(1024, 66, 4)
    (lanes, lens), = prepare_and_check(gpu_ctx, pts, mat)
    assert lanes and lens.shape == (66 * 128,)
    # ~256 pairs per bucket, half of that in the buckets of the largest magnitude (|digit| = 128
    # is the signed recoding of the raw window 128 alone)
    assert 64 < lens.min() and 220 < np.median(lens) < 290 and lens.max() < 400


def test_order_mostly_empty_buckets(gpu_ctx, monkeypatch):
    """The same at c = 16: 66 x 2^15 = 2.1 M buckets in 66 windows for 1.08 M pairs, so runs of
    length 0 (the identity piece), 1 (the copy-only iteration) and 2."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "16")
    pts = srs_powers(1024, 4242, gpu_ctx)
    mat = C.random_fr(62, 1024 * 66).reshape(1024, 66, 4)
    (lanes, lens), = prepare_and_check(gpu_ctx, pts, mat)
    assert lanes and lens.shape == (66 << 15,)
    counts = np.bincount(lens, minlength=3)
    assert counts[0] > len(lens) // 2 and counts[1] > 0 and counts[2] > 0


def test_order_partly_filled_last_wave(gpu_ctx, monkeypatch):
    """65 columns x 127 rows at c = 6: 65 * 32 = 2080 buckets = 32.5 waves, and an odd pair count
    (65 * 127 * 43), so the references are read one at a time instead of in aligned quads."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "6")
    pts = srs_powers(127, 4242, gpu_ctx)
    mat = C.random_fr(63, 127 * 65).reshape(127, 65, 4)
    (lanes, lens), = prepare_and_check(gpu_ctx, pts, mat)
    assert lanes and len(lens) % 64 == 32


def test_wave_with_unequal_runs(gpu_ctx, monkeypatch):
    """Thin columns (test_gpu_msm_digits.column): every third row of the r - 1 columns is r - 1, so
    among buckets of 0, 1 or 2 pairs a window holds a few of ~341 and its last wave runs of clearly
    different lengths."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "16")
    kinds = ["zero", "random", "r-1", "edge"]
    cols = [column(kinds[j % 4], 1024, 16, 700 + j, thin=True) for j in range(66)]
    pts = srs_powers(1024, 4242, gpu_ctx)
    (lanes, lens), = prepare_and_check(gpu_ctx, pts, to_matrix(cols))
    assert lanes and 300 < lens.max() <= ORDER_CAP
    # the window of the longest run: its last 64 entries (one wave) span short and long runs
    w0 = int(np.argmax(lens)) >> 15 << 15
    last_wave = np.sort(lens[w0:w0 + (1 << 15)])[-64:]
    assert last_wave[-1] > 300 and 4 * last_wave[0] < last_wave[-1]


def edge_columns(rows, width, seed):
    rng = O.SplitMix64(seed)
    cols = []
    for j in range(width):
        if j == 0:
            s = [0] * rows
        elif j % 3 == 1:  # equal scalars: one run of `rows` pairs per window
            s = [O.from_mont(rng.fr_mont())] * rows
        elif j % 3 == 2:  # small scalars
            s = [rng.next() % 1000 for _ in range(rows)]
        else:
            s = [O.from_mont(rng.fr_mont()) for _ in range(rows)]
        cols.append(s)
    return cols


@pytest.mark.parametrize("rows", [300, 100])
def test_exceptional_additions_inside_a_bucket(gpu_ctx, monkeypatch, rows):
    """66 columns x `rows` rows over bases P x rows/2 then -P x rows/2, and over all-P bases: every
    addition inside a bucket after its first is a doubling or a cancellation, so every bucket's
    unchecked run ends with ZZ = 0 and is summed again by the checked additions at the lane's one
    flush.  A zero column, equal-scalar columns and scalars < 1000; against double-and-add.
    300 rows (c = 9): an equal-scalar column whose scalar repeats a digit in two of its 29 windows
    puts 600 pairs -- 38 pieces of 16 -- in one bucket, above the one-level bound, so that batch
    runs in chunks.  100 rows (c = 8): the longest run is 300 pairs and the batch runs one bucket
    per lane."""
    monkeypatch.delenv("EON_MSM_FORCE_C", raising=False)
    P = O.g1_mul(O.G1_GEN, 1234567)
    width, h = 66, rows // 2
    cols = edge_columns(rows, width, 5)
    mat = np.stack([np.stack([fr(cols[j][i]) for j in range(width)]) for i in range(rows)])
    for bases_pts, signs in (([P] * h + [O.g1_neg(P)] * h, [1] * h + [-1] * h), ([P] * rows, [1] * rows)):
        bases = MsmBases(np.stack([pt(p) for p in bases_pts]), gpu_ctx, precompute=True)
        got, prep = bases.prepare_columns(dev(mat))
        try:
            for j in range(width):
                k = sum(s * sg for s, sg in zip(cols[j], signs)) % O.P
                assert as_py(got[j]) == (O.g1_mul(P, k) if k else O.INF), j
            (lanes, lens), = check_order(prep)
            assert lanes == (rows == 100), int(lens.max())
        finally:
            prep.close()
            bases.close()


def test_skewed_batch_takes_chunks(gpu_ctx, monkeypatch):
    """Column 0 all-equal scalars: 2048 pairs in one bucket per digit value, above the cap, so the
    batch reports the chunked route, and every column still matches."""
    monkeypatch.delenv("EON_MSM_FORCE_C", raising=False)
    pts = srs_powers(2048, 4242, gpu_ctx)
    mat = C.random_fr(64, 2048 * 66).reshape(2048, 66, 4)
    mat[:, 0] = C.random_fr(65, 1)[0]
    (lanes, lens), = prepare_and_check(gpu_ctx, pts, mat)
    assert lens.max() > ORDER_CAP and not lanes


def test_prepared_reuses_order(gpu_ctx, monkeypatch):
    """prepare_columns once, then the prepared MSMs against two other bases of the same layout: each
    equals a fresh msm_columns against that base, on the bucket route, and the order read back after
    both passes is the commitment's.  Then the same for a batch whose stored plan is the chunked
    piece sums and the CombineGroups route."""
    monkeypatch.setenv("EON_MSM_FORCE_C", "8")
    rows, width = 512, 66
    mat = C.random_fr(66, rows * width).reshape(rows, width, 4)
    pts = [srs_powers(rows, 1000 + t, gpu_ctx) for t in range(3)]
    bases = [MsmBases(p, gpu_ctx, precompute=True) for p in pts]
    got, prep = bases[0].prepare_columns(dev(mat))
    try:
        for j in range(width):
            np.testing.assert_array_equal(got[j], C.g1_msm(pts[0], mat[:, j]), err_msg=f"column {j}")
        (lanes, _), = check_order(prep)
        assert lanes
        before = prep.read_order(0)["order"].copy()
        for t in (1, 2):
            res = prep.msm([bases[t]])[0]
            np.testing.assert_array_equal(res, bases[t].msm_columns(mat))
            for j in range(0, width, 13):
                np.testing.assert_array_equal(res[j], C.g1_msm(pts[t], mat[:, j]), err_msg=f"bases {t} column {j}")
            after = prep.read_order(0)
            assert after["bucket_lanes"]
            np.testing.assert_array_equal(after["order"], before)
    finally:
        prep.close()
        for b in bases:
            b.close()
    # A stored plan other than the default one: test_gpu_msm._route_combine_groups' input, 66 columns
    # x 256 rows (c = 8) with column 0 the scalar 0x0101...01 in every row -- 512 pieces in one bucket,
    # so chunked piece sums and the CombineGroups route -- multiplied against two bases objects in
    # one call.
    monkeypatch.delenv("EON_MSM_FORCE_C")
    rows = 256
    mat = C.random_fr(56, rows * width).reshape(rows, width, 4)
    mat[:, 0] = fr(int.from_bytes(b"\x01" * 32, "little"))
    pts = [srs_powers(rows, 2000 + t, gpu_ctx) for t in range(3)]
    bases = [MsmBases(p, gpu_ctx, precompute=True) for p in pts]
    got, prep = bases[0].prepare_columns(dev(mat))
    try:
        (lanes, _), = check_order(prep)
        assert not lanes
        gpu_ctx.profile(True)
        try:
            res = prep.msm([bases[1], bases[2]])
            kernels = set(gpu_ctx.profile_report())
        finally:
            gpu_ctx.profile(False)
        assert {"k_partial_combine", "bucket_reduce"} <= kernels and "k_group_finish" not in kernels, sorted(kernels)
        for t in (1, 2):
            np.testing.assert_array_equal(res[t - 1], bases[t].msm_columns(mat))
            for j in range(width):
                np.testing.assert_array_equal(res[t - 1][j], C.g1_msm(pts[t], mat[:, j]),
                                              err_msg=f"bases {t} column {j}")
        assert not prep.read_order(0)["bucket_lanes"]
    finally:
        prep.close()
        for b in bases:
            b.close()
