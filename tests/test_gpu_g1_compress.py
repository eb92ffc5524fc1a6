"""eon_g1_compress (k_g1_compress, csrc/srs.hip): G1Affine::to_bytes of n points in one device
call, the exact inverse of eon_g1_decompress.

Sizes around the workgroup (256 lanes) and the wave (64): 0, 1, 63, 64, 65, 255, 256, 257 and 1025
(five workgroups, the last with one lane).  The points are SRS powers of alpha = 12345, every other
one negated so both parities of y occur, with (0,0) at index 0, in the middle and last.  Every
comparison is of bytes or integers."""

import numpy as np
import pytest

from oracle import pyoracle as O

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
Q = O.Q


def limbs(v):
    return [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]


def unlimbs(row):
    return sum(int(x) << (64 * i) for i, x in enumerate(row))


@pytest.fixture(scope="module")
def powers(gpu_ctx):
    """1025 SRS powers, odd indices negated (y -> q - y on the Montgomery residue)"""
    from plonky3_eon_amd.msm import srs_powers

    p = np.array(srs_powers(max(SIZES), 12345, gpu_ctx), dtype=np.uint64)
    for i in range(1, p.shape[0], 2):
        p[i, 4:] = limbs(Q - unlimbs(p[i, 4:]))
    return p


def point_set(powers, n):
    p = powers[:n].copy()
    for i in {0, n // 2, n - 1} if n else ():
        p[i] = 0
    return p


@pytest.fixture(scope="module")
def reference(powers):
    """eon_g1_to_bytes of every point, once"""
    from plonky3_eon_amd.native import g1_to_bytes

    inf = bytes(31) + b"\x40"
    per_point = [g1_to_bytes(p) for p in powers]
    assert {b[31] >> 7 for b in per_point} == {0, 1}  # both parities occur

    def of(n):
        return b"".join(inf if i in (0, n // 2, n - 1) else per_point[i] for i in range(n))

    return of


@pytest.mark.parametrize("n", SIZES)
def test_compress_equals_g1_to_bytes_and_inverts_decompress(gpu_ctx, powers, reference, n):
    from plonky3_eon_amd.srs import g1_compress, g1_decompress

    pts = point_set(powers, n)
    got = g1_compress(pts, gpu_ctx)
    assert len(got) == 32 * n
    assert got == reference(n)
    if n:
        assert got[:32] == got[-32:] == bytes(31) + b"\x40"
    np.testing.assert_array_equal(g1_decompress(got, gpu_ctx), pts)


def test_lowest_non_canonical_index_is_reported(gpu_ctx, powers):
    from plonky3_eon_amd.srs import SrsError, g1_compress

    pts = point_set(powers, 257)
    pts[70, :4] = limbs(Q)        # x = q
    pts[3, 4:] = limbs(Q + 1)     # y = q + 1
    with pytest.raises(SrsError) as e:
        g1_compress(pts, gpu_ctx)
    assert (e.value.reason, e.value.index) == ("NOT_CANONICAL", 3)
    only = point_set(powers, 257)
    only[256, :4] = limbs(2**256 - 1)  # the single lane of the second workgroup
    with pytest.raises(SrsError) as e:
        g1_compress(only, gpu_ctx)
    assert (e.value.reason, e.value.index) == ("NOT_CANONICAL", 256)


def test_rejected_points_are_written_as_zero_bytes(gpu_ctx, powers, reference):
    """through the C entry point: EON_E_SRS, the report, and the bytes of every other point intact"""
    import ctypes

    from plonky3_eon_amd import _lib

    n = 65
    pts = point_set(powers, n)
    pts[64, 4:] = limbs(Q)
    out = np.full(n * 4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rep = _lib.eon_srs_report()
    rc = gpu_ctx.lib.eon_g1_compress(gpu_ctx.handle, pts.ctypes.data_as(ctypes.c_void_p), n,
                                     out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rep))
    assert rc == _lib.EON_E_SRS and (rep.reason, rep.index) == (_lib.EON_SRS_NOT_CANONICAL, 64)
    got = out.tobytes()
    assert got[:32 * 64] == reference(n)[:32 * 64] and got[32 * 64:] == bytes(32)


def test_device_entry_point_on_device_buffers(gpu_ctx, powers, reference):
    import ctypes

    import torch

    from plonky3_eon_amd import _lib

    n = 257
    pts = torch.from_numpy(point_set(powers, n).view(np.int64)).to("cuda:0")
    out = torch.zeros(n * 4, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    gpu_ctx.set_stream(None)
    rep = _lib.eon_srs_report()
    rc = gpu_ctx.lib.eon_g1_compress_dev(gpu_ctx.handle, ctypes.c_void_p(pts.data_ptr()), n,
                                         ctypes.c_void_p(out.data_ptr()), ctypes.byref(rep))
    assert rc == 0 and rep.reason == _lib.EON_SRS_OK
    assert out.cpu().numpy().tobytes() == reference(n)
    # a byte pointer that is not 16-byte aligned is refused, not rounded
    rc = gpu_ctx.lib.eon_g1_compress_dev(gpu_ctx.handle, ctypes.c_void_p(pts.data_ptr()), 4,
                                         ctypes.c_void_p(out.data_ptr() + 8), ctypes.byref(rep))
    assert rc == _lib.EON_E_ARG


def test_srs_compress_bytes_are_the_per_point_join(gpu_ctx):
    from plonky3_eon_amd.native import g1_to_bytes
    from plonky3_eon_amd.srs import Srs

    srs = Srs.unsafe(300, 12345, gpu_ctx)
    c = srs.compress()
    assert c.compressed and c.n == 301
    assert c.g1_bytes == b"".join(g1_to_bytes(p) for p in srs.g1_powers)
