"""GPU parity of KzgMmcs (kzg/src/mmcs.rs): commit, batched row openings and verify_batch through
eon_quotient_and_eval_columns_multi_dev / eon_kzg_mmcs_open_dev / eon_kzg_mmcs_verify_batch, against
the oracle's restatement of the reference's route -- quotient_and_eval per column and point
(kzg/src/util.rs:100-111), commit_column of the quotient over the SRS (util.rs:37-40) -- bit for bit."""

import ctypes

import numpy as np
import pytest

from oracle import coracle as C
from plonky3_eon_amd import DegreeTooLarge, EonError, KzgMmcs, ProofShapeMismatch, _lib
from plonky3_eon_amd.field import FR_MODULUS, fr_to_abi, ints_to_limbs

pytestmark = pytest.mark.gpu

SHAPES = [(513, 2), (300, 3), (8, 3), (5, 2), (1, 2)]
MAX_HEIGHT = 513
INDICES = [0, 7, 512, 1023, 1026]
ALPHA = 0x1234567
IDENTITY = np.zeros(8, np.uint64)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def _local(height, index, max_height=MAX_HEIGHT):
    """kzg/src/mmcs.rs:213-218"""
    log2 = lambda x: (max(x, 1) - 1).bit_length()  # noqa: E731
    return (index >> (log2(max_height) - log2(height))) % height


# ---- 1. the reference KAT ------------------------------------------------------------------------
def test_reference_kat_mmcs_roundtrip(gpu_ctx):
    """kzg/src/tests.rs:51-70: alpha 5, max_degree 4, [[1, 2], [3, 4]], index 0."""
    mmcs = KzgMmcs(4, 5, gpu_ctx)
    mat = ints_to_limbs([1, 2, 3, 4]).reshape(2, 2, 4)
    commitment, data = mmcs.commit([mat])
    srs = C.g1_srs(5, C.fr_from_u64(5))
    np.testing.assert_array_equal(commitment[0], C.g1_msm_columns(srs, mat))
    assert len(mmcs.get_matrices(data)) == 1
    np.testing.assert_array_equal(mmcs.get_matrices(data)[0].cpu().numpy().view(np.uint64), mat)
    values, wits = mmcs.open_batch(0, data)
    want_v, want_w = C.open_columns(srs, mat, C.fr_from_u64(0))
    np.testing.assert_array_equal(values[0], want_v)
    np.testing.assert_array_equal(wits[0], want_w)
    np.testing.assert_array_equal(values[0], mat[0])  # f(0) = c_0: the opened row
    assert mmcs.verify_batch(commitment, [(2, 2)], 0, values, wits) is None


# ---- 2. the multi-point division kernel alone ----------------------------------------------------
def _points(npoints, seed):
    special = [C.fr_from_u64(0), C.fr_from_u64(1), ints_to_limbs([FR_MODULUS - 1])[0], C.fr_from_u64(2),
               C.fr_from_u64(7)]
    rnd = list(C.random_fr(seed, 4))
    return {1: [special[2]], 4: special[:3] + rnd[:1], 5: special[:4] + rnd[:1], 9: special + rnd}[npoints]


def _multi(gpu_ctx, coeffs_dev, rows, width, points, quotients, values):
    import torch

    zs = (_lib.eon_fr * max(len(points), 1))(*[fr_to_abi(z) for z in points])
    gpu_ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return gpu_ctx.lib.eon_quotient_and_eval_columns_multi_dev(
        gpu_ctx.handle, None if coeffs_dev is None else ctypes.c_void_p(coeffs_dev.data_ptr()), rows, width, zs,
        len(points), None if quotients is None else ctypes.c_void_p(quotients.data_ptr()),
        None if values is None else ctypes.c_void_p(values.data_ptr()))


@pytest.mark.parametrize("npoints", [1, 4, 5, 9])
@pytest.mark.parametrize("width", [1, 3, 130])
@pytest.mark.parametrize("rows", [1, 2, 255, 256, 257, 700])
def test_multi_point_division_matches_quotient_and_eval(gpu_ctx, rows, width, npoints):
    """One block, exactly full blocks, a partial top block; more columns than a thread block; a full
    group of points, a group plus one, three groups.  Column t * width + j of the quotient matrix is
    point t's quotient of column j; quotients = NULL leaves the same values."""
    import torch

    coeffs = C.random_fr(1000 * rows + width, rows * width).reshape(rows, width, 4)
    points = _points(npoints, rows + width)
    cd = _dev(coeffs)
    q = torch.full((max(rows - 1, 1), npoints * width, 4), -1, dtype=torch.int64, device="cuda:0")
    v = torch.full((npoints, width, 4), -1, dtype=torch.int64, device="cuda:0")
    gpu_ctx.check(_multi(gpu_ctx, cd, rows, width, points, q, v))
    got_q, got_v = q.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint64)
    for t, z in enumerate(points):
        for j in range(width):
            want_q, want_v = C.quotient_and_eval(coeffs[:, j], z)
            np.testing.assert_array_equal(got_v[t, j], want_v, err_msg=f"value, point {t} column {j}")
            if rows > 1:
                np.testing.assert_array_equal(got_q[:, t * width + j], want_q,
                                              err_msg=f"quotient, point {t} column {j}")
    if rows == 1:  # the quotients are empty: nothing is written
        assert bool((q == -1).all())
    v2 = torch.full((npoints, width, 4), -1, dtype=torch.int64, device="cuda:0")
    gpu_ctx.check(_multi(gpu_ctx, cd, rows, width, points, None, v2))
    np.testing.assert_array_equal(v2.cpu().numpy().view(np.uint64), got_v)


@pytest.mark.parametrize("rows,width,npoints", [(256 * 32 + 5, 2, 5), (256 * 32 * 3, 1, 4)])
def test_multi_point_division_across_carry_chunks(gpu_ctx, rows, width, npoints):
    """More than one chunk of 32 scan blocks: the chunk carries feed the block carries (a partial
    top chunk with a partial top block, and three exactly full chunks)."""
    import torch

    coeffs = C.random_fr(rows, rows * width).reshape(rows, width, 4)
    points = _points(npoints, rows)
    q = torch.full((rows - 1, npoints * width, 4), -1, dtype=torch.int64, device="cuda:0")
    v = torch.full((npoints, width, 4), -1, dtype=torch.int64, device="cuda:0")
    gpu_ctx.check(_multi(gpu_ctx, _dev(coeffs), rows, width, points, q, v))
    got_q, got_v = q.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint64)
    for t, z in enumerate(points):
        for j in range(width):
            want_q, want_v = C.quotient_and_eval(coeffs[:, j], z)
            np.testing.assert_array_equal(got_v[t, j], want_v, err_msg=f"value, point {t} column {j}")
            np.testing.assert_array_equal(got_q[:, t * width + j], want_q, err_msg=f"quotient, point {t} column {j}")


def test_multi_point_division_equals_the_single_point_entry(gpu_ctx):
    """Bit-identical to eon_quotient_and_eval_columns_dev called once per point."""
    import torch

    rows, width = 700, 3
    coeffs = _dev(C.random_fr(4242, rows * width).reshape(rows, width, 4))
    points = _points(5, 99)
    q = torch.zeros((rows - 1, 5 * width, 4), dtype=torch.int64, device="cuda:0")
    v = torch.zeros((5, width, 4), dtype=torch.int64, device="cuda:0")
    gpu_ctx.check(_multi(gpu_ctx, coeffs, rows, width, points, q, v))
    for t, z in enumerate(points):
        q1 = torch.zeros((rows - 1, width, 4), dtype=torch.int64, device="cuda:0")
        v1 = torch.zeros((width, 4), dtype=torch.int64, device="cuda:0")
        zz = fr_to_abi(z)
        gpu_ctx.check(gpu_ctx.lib.eon_quotient_and_eval_columns_dev(
            gpu_ctx.handle, ctypes.c_void_p(coeffs.data_ptr()), rows, width, ctypes.byref(zz),
            ctypes.c_void_p(q1.data_ptr()), ctypes.c_void_p(v1.data_ptr())))
        assert torch.equal(q[:, t * width:(t + 1) * width], q1) and torch.equal(v[t], v1)


def test_multi_point_division_edge_cases(gpu_ctx):
    import torch

    pts = [C.fr_from_u64(3), C.fr_from_u64(4)]
    c = _dev(C.random_fr(3, 4 * 3).reshape(4, 3, 4))
    q = torch.full((3, 6, 4), 7, dtype=torch.int64, device="cuda:0")
    v = torch.full((2, 3, 4), 7, dtype=torch.int64, device="cuda:0")
    # width == 0 and npoints == 0: OK, nothing written (even with NULL outputs)
    gpu_ctx.check(_multi(gpu_ctx, c, 4, 0, pts, q, v))
    gpu_ctx.check(_multi(gpu_ctx, c, 4, 3, [], q, v))
    gpu_ctx.check(_multi(gpu_ctx, None, 4, 0, pts, None, None))
    torch.cuda.synchronize()
    assert bool((q == 7).all()) and bool((v == 7).all())
    # rows == 0: zero values (kzg/src/util.rs:101-103), no quotients, coeffs not read
    gpu_ctx.check(_multi(gpu_ctx, None, 0, 3, pts, q, v))
    torch.cuda.synchronize()
    assert int(v.abs().sum().item()) == 0 and bool((q == 7).all())
    # NULL pointers that would be read or written, and a point that is not canonical
    for args in [(None, 4, 3, pts, q, v), (c, 4, 3, pts, q, None), (c, 0, 3, pts, q, None)]:
        assert _multi(gpu_ctx, *args) == _lib.EON_E_ARG
    bad = np.array([0x43E1F593F0000001, 0x2833E84879B97091, 0xB85045B68181585D, 0x30644E72E131A029], np.uint64)  # r
    assert _multi(gpu_ctx, c, 4, 3, [pts[0], bad], q, v) == _lib.EON_E_ARG
    with pytest.raises(EonError):
        gpu_ctx.check(_multi(gpu_ctx, c, 4, 3, [bad], None, v))


# ---- 3.-5. a mixed batch -------------------------------------------------------------------------
class _Batch:
    pass


@pytest.fixture(scope="module")
def batch(gpu_ctx):
    """The mixed batch, committed once, with the oracle's expected opening of every distinct
    (matrix, local index) the tests use."""
    b = _Batch()
    b.mmcs = KzgMmcs(520, ALPHA, gpu_ctx)
    b.mats = [C.random_fr(500 + k, h * w).reshape(h, w, 4) for k, (h, w) in enumerate(SHAPES)]
    b.commitment, b.data = b.mmcs.commit([_dev(m) if k % 2 else m for k, m in enumerate(b.mats)])
    b.srs = C.g1_srs(521, C.fr_from_u64(ALPHA))
    b.dims = list(SHAPES)
    cache = {}

    def expected(k, index):
        loc = _local(SHAPES[k][0], index)
        if (k, loc) not in cache:
            cache[(k, loc)] = C.open_columns(b.srs, b.mats[k], C.fr_from_u64(loc))
        return cache[(k, loc)]

    b.expected = expected
    b.openings = {i: b.mmcs.open_batch(i, b.data) for i in INDICES}
    return b


def test_mixed_batch_commitment(batch):
    for k, m in enumerate(batch.mats):
        np.testing.assert_array_equal(batch.commitment[k], C.g1_msm_columns(batch.srs, m), err_msg=f"matrix {k}")


@pytest.mark.parametrize("index", INDICES)
def test_mixed_batch_open_matches_oracle_and_verifies(batch, index):
    values, wits = batch.openings[index]
    assert len(values) == len(wits) == len(SHAPES)
    for k, (h, w) in enumerate(SHAPES):
        assert batch.mmcs.ctx.lib.eon_kzg_mmcs_local_index(MAX_HEIGHT, h, index) == _local(h, index)
        want_v, want_w = batch.expected(k, index)
        np.testing.assert_array_equal(values[k], want_v, err_msg=f"values, matrix {k}")
        np.testing.assert_array_equal(wits[k], want_w, err_msg=f"witnesses, matrix {k}")
    # the height-1 matrix: the identity witness and c_0
    np.testing.assert_array_equal(values[4], batch.mats[4][0])
    np.testing.assert_array_equal(wits[4], np.zeros((2, 8), np.uint64))
    assert batch.mmcs.verify_batch(batch.commitment, batch.dims, index, values, wits) is None


def test_open_batch_many_equals_open_batch(batch):
    """Repeats, and indices that collapse onto one row of the short matrices (1022 and 1023 open the
    same row of every matrix but the tallest): the deduplication and the copy-out."""
    indices = [1023, 0, 7, 1022, 0, 512, 1026, 1023, 6, 2, 3]
    many = batch.mmcs.open_batch_many(indices, batch.data)
    assert len(many) == len(indices)
    singles = dict(batch.openings)
    for i in set(indices) - set(singles):
        singles[i] = batch.mmcs.open_batch(i, batch.data)
    for i, (values, wits) in zip(indices, many):
        for k in range(len(SHAPES)):
            np.testing.assert_array_equal(values[k], singles[i][0][k], err_msg=f"index {i} matrix {k}")
            np.testing.assert_array_equal(wits[k], singles[i][1][k], err_msg=f"index {i} matrix {k}")
            np.testing.assert_array_equal(values[k], batch.expected(k, i)[0])
            np.testing.assert_array_equal(wits[k], batch.expected(k, i)[1])
    assert batch.mmcs.open_batch_many([], batch.data) == []


def test_open_batch_many_in_several_groups(batch, monkeypatch):
    """The distinct points of a matrix split into groups by quotient scratch: with a cap of two
    points of the tallest matrix (512 x 2 x 32 bytes each) its five distinct points run as 2 + 2 + 1
    and the (300, 3) matrix's two at a time; the openings do not change."""
    indices = [1023, 0, 7, 512, 1026, 6, 1023]
    monkeypatch.setenv("EON_MMCS_GROUP_BYTES", str(2 * 512 * 2 * 32))
    grouped = batch.mmcs.open_batch_many(indices, batch.data)
    monkeypatch.delenv("EON_MMCS_GROUP_BYTES")
    for i, (values, wits) in zip(indices, grouped):
        for k in range(len(SHAPES)):
            np.testing.assert_array_equal(values[k], batch.expected(k, i)[0], err_msg=f"index {i} matrix {k}")
            np.testing.assert_array_equal(wits[k], batch.expected(k, i)[1], err_msg=f"index {i} matrix {k}")


def test_verify_batch_rejections(batch):
    mmcs, cm, dims = batch.mmcs, batch.commitment, batch.dims
    values, wits = batch.openings[7]
    copy = lambda xs: [x.copy() for x in xs]  # noqa: E731
    # one value changed
    v = copy(values)
    v[1][2] = C.fr_from_u64(9)
    with pytest.raises(ProofShapeMismatch):
        mmcs.verify_batch(cm, dims, 7, v, wits)
    # one witness replaced by another column's
    w = copy(wits)
    w[0][0] = wits[0][1]
    with pytest.raises(ProofShapeMismatch):
        mmcs.verify_batch(cm, dims, 7, values, w)
    # the right opening under a different index
    with pytest.raises(ProofShapeMismatch):
        mmcs.verify_batch(cm, dims, 512, values, wits)
    # a dropped matrix
    with pytest.raises(ProofShapeMismatch):
        mmcs.verify_batch(cm, dims, 7, values[:-1], wits[:-1])
    # a per-matrix width disagreement
    v = copy(values)
    v[2] = v[2][:-1]
    with pytest.raises(ProofShapeMismatch):
        mmcs.verify_batch(cm, dims, 7, v, wits)
    w = copy(wits)
    w[3] = np.concatenate([w[3], w[3][:1]])
    with pytest.raises(ProofShapeMismatch):
        mmcs.verify_batch(cm, dims, 7, values, w)
    # and the untouched opening still passes
    assert mmcs.verify_batch(cm, dims, 7, values, wits) is None


def test_verify_batch_zips_like_the_reference(batch):
    """The walk stops at the shortest of values / commitments / dimensions / witnesses
    (mmcs.rs:260-264), with max_height over all dimensions (:254)."""
    mmcs, cm, dims = batch.mmcs, batch.commitment, batch.dims
    values, wits = batch.openings[7]
    # fewer witness lists than matrices: only the zipped prefix is checked
    assert mmcs.verify_batch(cm, dims, 7, values, wits[:2]) is None
    # fewer dimensions: max_height is then 8 over [(8, 3)], so index 7 opens row 7 of the third matrix
    v8, w8 = batch.expected(2, 1023)  # local index 7 of the height-8 matrix
    assert mmcs.verify_batch([cm[2]] + cm[:1], [(8, 3)], 7, [v8, values[0]], [w8, wits[0]]) is None


def test_degree_too_large_and_height_zero(batch, gpu_ctx):
    import torch

    mmcs = batch.mmcs
    values, wits = batch.openings[0]
    dims = [(522, 2)] + batch.dims[1:]
    with pytest.raises(DegreeTooLarge):
        mmcs.verify_batch(batch.commitment, dims, 0, values, wits)
    assert mmcs.verify_batch(batch.commitment, [(521, 2)] + batch.dims[1:], 0, values, wits) is None
    with pytest.raises(DegreeTooLarge):
        mmcs.commit([np.zeros((522, 1, 4), np.uint64)])
    # open on a matrix of height 0: the shape error (the reference panics)
    from plonky3_eon_amd.mmcs import KzgMmcsProverData

    empty = KzgMmcsProverData([torch.zeros((0, 2, 4), dtype=torch.int64, device="cuda:0")])
    with pytest.raises(EonError) as e:
        mmcs.open_batch(0, empty)
    assert e.value.code == _lib.EON_E_SHAPE
    # open on a matrix taller than the SRS: the C entry's own check
    tall = KzgMmcsProverData([torch.zeros((522, 1, 4), dtype=torch.int64, device="cuda:0")])
    with pytest.raises(DegreeTooLarge):
        mmcs.open_batch(0, tall)
