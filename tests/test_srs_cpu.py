"""CPU side of the SRS loader: the big-int decompressor (tests/mirror_srs.py) against the oracle's
compressed encoding, and srs.Srs's container -- round trips in both encodings, prefix loads and
every header rejection.  No device call: the container is read and checked on the host."""

import struct

import numpy as np
import pytest

import mirror_srs as M
from mirror_pairing import g1_limbs, g2_limbs
from oracle import pairing as E
from oracle import pyoracle as O

KS = list(range(1, 64)) + [O.P - 1]  # 64 multiples of G


@pytest.fixture(scope="module")
def points():
    return [O.g1_mul(O.G1_GEN, k) for k in KS]


def test_mirror_decompress_inverts_the_oracle_encoding(points):
    assert len(points) == 64
    parities = {p[1] & 1 for p in points}
    assert parities == {0, 1}  # both roots are exercised
    data = b"".join(O.g1_compressed(p) for p in points)
    assert M.decompress(data) == points
    assert M.decompress(O.g1_compressed(O.INF)) == [None]
    for p in points[:8]:  # the other parity flag selects the other root
        assert M.decompress_one(M.compress(p, odd=1 - (p[1] & 1))) == (p[0], O.Q - p[1])


def test_mirror_rejections_and_lowest_index(points):
    good = [O.g1_compressed(p) for p in points[:5]]
    xnr = M.non_residue_x()
    assert not M.is_square(xnr ** 3 + 3)
    bad = {M.NOT_CANONICAL: M.raw_x(O.Q), M.NOT_ON_CURVE: M.raw_x(xnr), M.ENCODING: M.raw_x(5, inf=1)}
    for reason, enc in bad.items():
        for at in (0, 2, 4):
            data = list(good)
            data[at] = enc
            with pytest.raises(M.Rejected) as e:
                M.decompress(b"".join(data))
            assert (e.value.reason, e.value.index) == (reason, at)
    data = list(good)
    data[3], data[1] = bad[M.NOT_CANONICAL], bad[M.ENCODING]
    with pytest.raises(M.Rejected) as e:
        M.decompress(b"".join(data))
    assert (e.value.reason, e.value.index) == (M.ENCODING, 1)
    # the identity flag with the parity flag set is an encoding error too; x = q - 1 is canonical
    with pytest.raises(M.Rejected) as e:
        M.decompress_one(M.raw_x(0, odd=1, inf=1))
    assert e.value.reason == M.ENCODING
    x = O.Q - 1  # the largest canonical x is judged by its square root, not by its size
    if M.is_square(x ** 3 + 3):
        assert M.decompress_one(M.raw_x(x))[0] == x
    else:
        with pytest.raises(M.Rejected) as e:
            M.decompress_one(M.raw_x(x))
        assert e.value.reason == M.NOT_ON_CURVE


def test_mirror_validate():
    g = (O.fq_to_mont(1), O.fq_to_mont(2))
    M.validate_raw([g])
    for pt, reason in (((g[0], (g[1] + 1) % O.Q), M.NOT_ON_CURVE), ((g[0] + O.Q, g[1]), M.NOT_CANONICAL),
                       ((0, 0), M.IDENTITY)):
        with pytest.raises(M.Rejected) as e:
            M.validate_raw([g, pt])
        assert (e.value.reason, e.value.index) == (reason, 1)
    assert g[0] + O.Q < 1 << 256


def test_twist_point_outside_the_subgroup():
    p = M.twist_point_outside_subgroup()
    assert E.g2_on_curve(p) and M.g2_mul_int(p, O.P) is not None
    assert M.g2_mul_int(E.G2_GEN, O.P) is None  # the generator is inside
    assert M.f2_sqrt(E.f2_mul((3, 4), (3, 4))) in ((3, 4), E.f2_neg((3, 4)))


# ---- container ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def srs(points):
    from plonky3_eon_amd.srs import Srs

    alpha = 7
    pts = [O.g1_mul(O.G1_GEN, pow(alpha, i, O.P)) for i in range(9)]
    return Srs(np.stack([g1_limbs(p) for p in pts]), g2_limbs(E.g2_alpha(alpha))), pts


@pytest.mark.parametrize("compressed", [True, False])
def test_container_round_trip_and_prefix(tmp_path, srs, compressed):
    from plonky3_eon_amd.srs import HEADER_BYTES, MAGIC, Srs

    s, pts = srs
    path = tmp_path / "srs.bin"
    s.save(path, compressed=compressed)
    raw = path.read_bytes()
    assert raw[:8] == MAGIC == b"EONSRS1\0"
    assert struct.unpack("<QII", raw[8:24]) == (9, 1 if compressed else 0, 0)
    assert raw[24:152] == g2_limbs(E.g2_alpha(7)).tobytes() and HEADER_BYTES == 152
    assert len(raw) == 152 + 9 * (32 if compressed else 64)
    if compressed:  # the entries are the oracle's encoding of the points
        assert raw[152:] == b"".join(O.g1_compressed(p) for p in pts)
    else:
        assert raw[152:] == s.g1_powers.tobytes()
    back = Srs.load(path)
    assert back.max_degree == 8 and back.compressed == compressed
    assert np.array_equal(back.g2_alpha, s.g2_alpha)
    for k in (0, 3, 8):
        pre = Srs.load(path, max_degree=k)
        assert pre.max_degree == k and pre.n == k + 1
        if compressed:
            assert pre.g1_bytes == raw[152:152 + 32 * (k + 1)]
            assert M.decompress(pre.g1_bytes) == pts[:k + 1]
        else:
            assert np.array_equal(pre.g1_powers, s.g1_powers[:k + 1])
    assert back.compress().g1_bytes == s.compress().g1_bytes


def test_container_header_rejections(tmp_path, srs):
    from plonky3_eon_amd.srs import Srs, SrsError

    s, _ = srs
    path = tmp_path / "srs.bin"
    s.save(path)
    good = path.read_bytes()

    def rejected(data, **kw):
        bad = tmp_path / "bad.bin"
        bad.write_bytes(data)
        with pytest.raises(SrsError) as e:
            Srs.load(bad, **kw)
        assert e.value.reason == "CONTAINER" and e.value.index == 0
        return str(e.value)

    assert "magic" in rejected(b"EONSRS2\0" + good[8:])
    assert "truncated" in rejected(good[:100])  # inside the header
    assert "truncated" in rejected(good[:-1])  # one byte short of the last entry
    assert "truncated" in rejected(good[:-1], max_degree=2)  # even when the prefix itself is there
    assert "needs 10 powers" in rejected(good, max_degree=9)  # k + 1 > count
    assert "reserved" in rejected(good[:16] + struct.pack("<I", 3) + good[20:])  # an unknown flag bit
    assert "reserved" in rejected(good[:20] + struct.pack("<I", 1) + good[24:])  # the zero word
    assert "no G1 powers" in rejected(good[:8] + struct.pack("<Q", 0) + good[16:])
    assert "needs 0 powers" in rejected(good, max_degree=-1)
    Srs.load(path, max_degree=8)  # exactly the count is fine
