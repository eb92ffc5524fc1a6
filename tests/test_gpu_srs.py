"""KzgPcs::from_srs on the device (csrc/srs.hip, host/pcs.cpp): decompression and validation of
supplied G1 powers, the trapdoor-free structure check, and prove / verify over a supplied SRS.

Every comparison is bit for bit: decompressed points against the points they were compressed from
and against the big-int mirror (tests/mirror_srs.py); rejection reasons and the lowest rejected
index against the mirror's; proofs over a supplied SRS against the proofs of the handle made from
alpha, field by field.  Shapes are the smallest at which the kernels can go wrong: 1, 2, one short
of a workgroup, a workgroup, one past it, and 1025 points (five workgroups, the last one partial)."""

import copy
import ctypes

import numpy as np
import pytest

import mirror_lookup as ML
import mirror_srs as M
from airs import FibonacciAir, MixedAir
from airs_preprocessed import MixedPreAir, mixed_pre_preprocessed, mixed_pre_trace
from mirror_pairing import g1_limbs, g2_limbs
from oracle import coracle as C
from oracle import pairing as E
from oracle import pyoracle as O
from oracle.smallrng import SmallRng, poseidon2_new_from_rng

pytestmark = pytest.mark.gpu
ALPHA = 12345
RHO = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF  # the fixed challenge of these tests
NMAX = 1025
ints, lim, to_limbs = ML.ints, ML.lim, ML.to_limbs


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def point_ints(limbs):
    """(n, 8) Montgomery limbs -> the oracle's points"""
    out = []
    for row in np.asarray(limbs, dtype=np.uint64).reshape(-1, 8):
        x, y = O.limbs_to_int(row[:4]), O.limbs_to_int(row[4:])
        out.append(None if x == 0 and y == 0 else (O.fq_from_mont(x), O.fq_from_mont(y)))
    return out


@pytest.fixture(scope="module")
def powers(gpu_ctx):
    """alpha^i G for i < 1025 as limbs, their compressed bytes, and the same points as ints"""
    from plonky3_eon_amd.msm import srs_powers
    from plonky3_eon_amd.native import g1_to_bytes

    pts = srs_powers(NMAX, ALPHA, gpu_ctx)
    pts.setflags(write=False)
    data = b"".join(g1_to_bytes(p) for p in pts)
    as_ints = point_ints(pts)
    assert as_ints[:3] == [O.G1_GEN, O.g1_mul(O.G1_GEN, ALPHA), O.g1_mul(O.G1_GEN, ALPHA * ALPHA)]
    assert data == b"".join(O.g1_compressed(p) for p in as_ints)  # the driver's encoding is the oracle's
    return pts, data, as_ints


@pytest.fixture(scope="module")
def g2a(gpu_ctx):
    from plonky3_eon_amd.verify import g2_mul

    g = g2_mul(ALPHA, ctx=gpu_ctx)
    assert np.array_equal(g, g2_limbs(E.g2_alpha(ALPHA)))
    g.setflags(write=False)
    return g


def rejected(fn, *a, **kw):
    from plonky3_eon_amd.srs import SrsError

    with pytest.raises(SrsError) as e:
        fn(*a, **kw)
    return e.value.reason, e.value.index


# ---- decompress ------------------------------------------------------------------------------------
def test_workgroup_size_is_the_kernels():
    from pathlib import Path

    import plonky3_eon_amd.srs as S

    text = (Path(S.__file__).parent / "csrc" / "srs.hip").read_text()
    assert f"constexpr uint32_t SRS_THREADS = {S.DECOMPRESS_WORKGROUP};" in text


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, NMAX])
def test_decompress_inverts_compression(gpu_ctx, powers, n):
    from plonky3_eon_amd.srs import DECOMPRESS_WORKGROUP as W
    from plonky3_eon_amd.srs import g1_decompress

    assert (255, 256, 257) == (W - 1, W, W + 1)
    pts, data, as_ints = powers
    got = g1_decompress(data[:32 * n], gpu_ctx)
    assert np.array_equal(got, pts[:n])
    assert M.decompress(data[:32 * n]) == as_ints[:n] == point_ints(got)


def test_decompress_both_parities_identity_and_empty(gpu_ctx, powers):
    from plonky3_eon_amd.srs import g1_decompress

    pts, data, as_ints = powers
    assert {p[1] & 1 for p in as_ints[:64]} == {0, 1}
    # the other parity flag gives the negated point; the identity decodes to (0, 0) between points
    k = 5
    flipped = M.compress(as_ints[k], odd=1 - (as_ints[k][1] & 1))
    enc = data[:32] + O.g1_compressed(O.INF) + flipped
    got = g1_decompress(enc, gpu_ctx)
    want = [as_ints[0], None, O.g1_neg(as_ints[k])]
    assert M.decompress(enc) == want
    assert np.array_equal(got, np.stack([g1_limbs(p) for p in want]))
    assert g1_decompress(b"", gpu_ctx).shape == (0, 8)


def bad_encodings():
    xnr = M.non_residue_x(1000)
    assert not M.is_square(xnr ** 3 + 3)  # Euler's criterion
    return {"NOT_CANONICAL": M.raw_x(O.Q), "NOT_ON_CURVE": M.raw_x(xnr, odd=1), "ENCODING": M.raw_x(7, inf=1)}


@pytest.mark.parametrize("kind", ["NOT_CANONICAL", "NOT_ON_CURVE", "ENCODING"])
def test_decompress_rejects_with_reason_and_index(gpu_ctx, powers, kind):
    from plonky3_eon_amd.srs import g1_decompress

    n = 257
    _, data, _ = powers
    enc = bad_encodings()[kind]
    for at in (0, 128, n - 1):
        blob = data[:32 * at] + enc + data[32 * (at + 1):32 * n]
        assert rejected(g1_decompress, blob, gpu_ctx) == (kind, at)
        with pytest.raises(M.Rejected) as e:
            M.decompress(blob)
        assert (e.value.reason, e.value.index) == (kind, at)


def test_decompress_lowest_bad_index_wins(gpu_ctx, powers):
    from plonky3_eon_amd.srs import g1_decompress

    n = NMAX
    _, data, _ = powers
    bad = bad_encodings()
    # a later workgroup's rejection never hides an earlier one, whatever their reasons
    for (lo, klo), (hi, khi) in [((3, "NOT_ON_CURVE"), (1000, "ENCODING")), ((300, "ENCODING"), (301, "NOT_CANONICAL")),
                                 ((0, "NOT_CANONICAL"), (n - 1, "NOT_ON_CURVE"))]:
        blob = bytearray(data[:32 * n])
        blob[32 * lo:32 * lo + 32] = bad[klo]
        blob[32 * hi:32 * hi + 32] = bad[khi]
        assert rejected(g1_decompress, bytes(blob), gpu_ctx) == (klo, lo)
        with pytest.raises(M.Rejected) as e:
            M.decompress(bytes(blob))
        assert (e.value.reason, e.value.index) == (klo, lo)


# ---- validate --------------------------------------------------------------------------------------
def raw_limbs(v):
    return np.array(O.int_to_limbs(v), dtype=np.uint64)


def test_validate(gpu_ctx, powers):
    from plonky3_eon_amd.srs import g1_validate

    pts, _, _ = powers
    n = 257
    g1_validate(pts[:n], gpu_ctx)
    g1_validate(pts[:0], gpu_ctx)
    x = O.limbs_to_int(pts[9][:4])
    y = O.limbs_to_int(pts[9][4:])
    assert x + O.Q < 1 << 256  # still fits the limbs
    cases = {"NOT_ON_CURVE": np.concatenate([raw_limbs(x), raw_limbs((y + 1) % O.Q)]),
             "NOT_CANONICAL": np.concatenate([raw_limbs(x + O.Q), raw_limbs(y)]),
             "IDENTITY": np.zeros(8, np.uint64)}
    for reason, pt in cases.items():
        for at in (0, 130, n - 1):
            bad = pts[:n].copy()
            bad[at] = pt
            assert rejected(g1_validate, bad, gpu_ctx) == (reason, at)
            rows = [(O.limbs_to_int(r[:4]), O.limbs_to_int(r[4:])) for r in bad]
            with pytest.raises(M.Rejected) as e:
                M.validate_raw(rows)
            assert (e.value.reason, e.value.index) == (reason, at)
    bad = pts[:n].copy()
    bad[200], bad[20] = cases["IDENTITY"], cases["NOT_ON_CURVE"]
    assert rejected(g1_validate, bad, gpu_ctx) == ("NOT_ON_CURVE", 20)


# ---- structure -------------------------------------------------------------------------------------
def bases_of(gpu_ctx, pts):
    from plonky3_eon_amd.msm import MsmBases

    return MsmBases(pts, gpu_ctx, precompute=True)


@pytest.mark.parametrize("n", [1, 2, 3, 257, NMAX])
def test_structure_accepts_an_honest_srs(gpu_ctx, powers, g2a, n):
    from plonky3_eon_amd.srs import srs_check

    b = bases_of(gpu_ctx, powers[0][:n])
    srs_check(b, n, g2a, RHO)
    if n == NMAX:  # a prefix of the table is checked against the same tables
        srs_check(b, 600, g2a, RHO)
    b.close()


def doubled(pts, as_ints, k):
    out = pts.copy()
    out[k] = g1_limbs(O.g1_add(as_ints[k], as_ints[k]))
    return out


@pytest.mark.parametrize("k", [1, 128, 256])
def test_structure_rejects_a_doubled_power(gpu_ctx, powers, g2a, k):
    from plonky3_eon_amd.srs import srs_check

    pts, _, as_ints = powers
    b = bases_of(gpu_ctx, doubled(pts[:257], as_ints, k))
    assert rejected(srs_check, b, 257, g2a, RHO) == ("STRUCTURE", 0)
    if k == 256:  # the prefix without the bad point is an SRS
        srs_check(b, 256, g2a, RHO)
    b.close()


def test_structure_rejects_swapped_points_and_a_foreign_g2(gpu_ctx, powers, g2a):
    from plonky3_eon_amd.srs import srs_check
    from plonky3_eon_amd.verify import g2_mul

    pts, _, as_ints = powers
    swapped = pts[:257].copy()
    swapped[[100, 101]] = swapped[[101, 100]]
    b = bases_of(gpu_ctx, swapped)
    assert rejected(srs_check, b, 257, g2a, RHO) == ("STRUCTURE", 0)
    b.close()
    b = bases_of(gpu_ctx, pts[:257])
    assert rejected(srs_check, b, 257, g2_mul(ALPHA + 1, ctx=gpu_ctx), RHO) == ("STRUCTURE", 0)
    b.close()
    two_g = pts[:257].copy()
    two_g[0] = g1_limbs(O.g1_add(O.G1_GEN, O.G1_GEN))
    b = bases_of(gpu_ctx, two_g)
    assert rejected(srs_check, b, 257, g2a, RHO) == ("G0_NOT_GENERATOR", 0)
    assert rejected(srs_check, b, 1, g2a, RHO) == ("G0_NOT_GENERATOR", 0)
    b.close()


def test_structure_rejects_an_invalid_g2(gpu_ctx, powers, g2a):
    from plonky3_eon_amd.srs import srs_check

    b = bases_of(gpu_ctx, powers[0][:3])
    off = np.array(g2a).copy()
    off[8:12] = raw_limbs((O.limbs_to_int(off[8:12]) + 1) % O.Q)  # y.c0 + 1: off the twist
    outside = M.twist_point_outside_subgroup()
    assert E.g2_on_curve(outside) and M.g2_mul_int(outside, O.P) is not None
    not_canonical = np.array(g2a).copy()
    not_canonical[0:4] = raw_limbs(O.limbs_to_int(not_canonical[0:4]) + O.Q)
    for g in (off, g2_limbs(outside), np.zeros(16, np.uint64), not_canonical):
        for n in (1, 3):  # checked with and without the pairing step
            assert rejected(srs_check, b, n, g, RHO) == ("G2_INVALID", 0)
    srs_check(b, 3, g2a, RHO)
    b.close()


def test_structure_argument_errors(gpu_ctx, powers, g2a):
    from plonky3_eon_amd import EonError, _lib
    from plonky3_eon_amd.srs import srs_check

    b = bases_of(gpu_ctx, powers[0][:3])
    with pytest.raises(EonError) as e:
        srs_check(b, 3, g2a, 0)
    assert e.value.code == _lib.EON_E_ARG
    rep = _lib.eon_srs_report()
    big = raw_limbs(O.P)  # the limbs of r itself: not a canonical Fr
    g = np.ascontiguousarray(g2a)
    rc = gpu_ctx.lib.eon_kzg_srs_check(gpu_ctx.handle, b._h, 3, g.ctypes.data_as(ctypes.c_void_p),
                                       big.ctypes.data_as(ctypes.c_void_p), ctypes.byref(rep))
    assert rc == _lib.EON_E_ARG and rep.reason == 0
    with pytest.raises(EonError) as e:
        srs_check(b, 4, g2a, RHO)  # more points than the table has
    assert e.value.code == _lib.EON_E_SHAPE
    b.close()


def test_from_srs_validates_by_default_and_trusts_on_request(gpu_ctx, powers, g2a):
    from plonky3_eon_amd.native import NativeKzgPcs
    from plonky3_eon_amd.srs import Srs

    pts, data, as_ints = powers
    honest = Srs(pts[:257], g2a)
    NativeKzgPcs.from_srs(honest, ctx=gpu_ctx).close()  # rho drawn by the binding
    tampered = Srs(doubled(pts[:257], as_ints, 128), g2a)
    assert rejected(NativeKzgPcs.from_srs, tampered, ctx=gpu_ctx) == ("STRUCTURE", 0)
    assert rejected(NativeKzgPcs.from_srs, tampered, rho=RHO, ctx=gpu_ctx) == ("STRUCTURE", 0)
    # EON_SRS_TRUSTED skips the structure check and nothing else: this is what the flag means
    p = NativeKzgPcs.from_srs(tampered, validate=False, ctx=gpu_ctx)
    assert p.max_degree == 256
    p.close()
    off_curve = pts[:257].copy()
    off_curve[77, 4] ^= np.uint64(1)
    assert rejected(NativeKzgPcs.from_srs, Srs(off_curve, g2a), validate=False, ctx=gpu_ctx) == ("NOT_ON_CURVE", 77)
    blob = data[:32 * 40] + O.g1_compressed(O.INF) + data[32 * 41:32 * 257]
    assert rejected(NativeKzgPcs.from_srs, Srs(blob, g2a), validate=False, ctx=gpu_ctx) == ("IDENTITY", 40)
    blob = data[:32 * 256] + bad_encodings()["NOT_ON_CURVE"]
    assert rejected(NativeKzgPcs.from_srs, Srs(blob, g2a), rho=RHO, ctx=gpu_ctx) == ("NOT_ON_CURVE", 256)


# ---- prove and verify over a supplied SRS ----------------------------------------------------------
@pytest.fixture(scope="module")
def ch_consts():
    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    return [[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]]


@pytest.fixture(scope="module")
def handles(gpu_ctx, tmp_path_factory):
    """name -> pcs: the handle made from alpha, and the same SRS supplied as affine points, as
    compressed bytes, and through save / load with a shorter max_degree; plus a verifier handle"""
    from plonky3_eon_amd.native import NativeKzgPcs
    from plonky3_eon_amd.srs import Srs

    srs = Srs.unsafe(2 ** 6, ALPHA, gpu_ctx)
    assert srs.max_degree == 64 and not srs.compressed
    path = tmp_path_factory.mktemp("srs") / "srs.bin"
    srs.save(path)
    loaded = Srs.load(path, max_degree=31)
    assert loaded.compressed and loaded.max_degree == 31
    out = {"alpha": NativeKzgPcs(2 ** 6, ALPHA, gpu_ctx),
           "affine": NativeKzgPcs.from_srs(srs, rho=RHO, ctx=gpu_ctx),
           "bytes": NativeKzgPcs.from_srs(srs.compress(), rho=RHO, ctx=gpu_ctx),
           "loaded": NativeKzgPcs.from_srs(loaded, rho=RHO, ctx=gpu_ctx),
           "verifier": NativeKzgPcs.verifier(2 ** 6, srs.g2_alpha, gpu_ctx)}
    yield out, srs
    for p in out.values():
        p.close()


class Job:
    def __init__(self, prover, prog, trace, publics=(), fs=False, satisfiable=True, pre=None):
        self.prover, self.prog, self.trace, self.publics = prover, prog, trace, list(publics)
        self.fs, self.satisfiable, self.pre = fs, satisfiable, pre


@pytest.fixture(scope="module")
def jobs(gpu_ctx):
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air

    out = {}
    fib = AirProgram(FibonacciAir(), gpu_ctx)
    out["fibonacci"] = Job(fib, fib, dev(to_limbs(O.fib_trace(0, 1, 8))), [0, 1, 21])
    # MixedAir has no satisfying trace (s = 0 forces loc[1] = 0 on every row while (loc[2] - 7)
    # (next[1] - 11) = 0 forces next[1] = 11 or s^2 = 7): its proofs are compared byte for byte and
    # their verdicts handle against handle; acceptance is asserted on the other AIRs
    mixed = AirProgram(MixedAir(), gpu_ctx)
    out["mixed_fs"] = Job(mixed, mixed, dev(C.random_fr(41, 16 * 5).reshape(16, 5, 4)),
                          [int(x) for x in ints(C.random_fr(42, 2))], fs=True, satisfiable=False)
    rows, pub = mixed_pre_trace(3, 4, 5, 16)
    mp = AirProgram(MixedPreAir(), gpu_ctx)
    out["mixed_pre_fs"] = Job(mp, mp, dev(to_limbs(rows)), pub, fs=True, pre=dev(to_limbs(mixed_pre_preprocessed(16))))
    p2py = O.p2_constants(2024, 4, 56)
    k = C.P2Constants([[lim(v) for v in r] for r in p2py[0]], [lim(v) for v in p2py[1]],
                      [[lim(v) for v in r] for r in p2py[2]])
    air = Poseidon2Air(k.begin, k.partial, k.end, 1, gpu_ctx)
    trace = air.generate_trace(dev(C.random_fr(61, 8 * 3).reshape(8, 3, 4)))
    out["p2air"] = Job(air, AirProgram(air, gpu_ctx), trace)
    return out


def run_prove(job, pcs, ch_consts):
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants, prove_native, setup_preprocessed

    kw = dict(public_values=job.publics) if job.publics else {}
    pp = None
    if job.pre is not None:
        pp = setup_preprocessed(pcs, job.pre)
        kw["preprocessed"] = pp
    if job.fs:
        ch = Challenger(Poseidon2Constants(*ch_consts))
        proof = prove_native(job.prover, pcs, job.trace, None, None, challenger=ch, **kw)
    else:
        proof = prove_native(job.prover, pcs, job.trace, 0x1111222233334444, 0x5555666677778888, **kw)
    vk = (pp.width, pp.degree_bits, pp.commitment.copy()) if pp is not None else None
    if pp is not None:
        pp.close()
    return proof, vk


def flat(x):
    """every array of a nested proof field, in order"""
    if x is None:
        return []
    if isinstance(x, (list, tuple)):
        return [a for y in x for a in flat(y)]
    return [np.asarray(x, dtype=np.uint64)]


def assert_same_proof(a, b):
    assert (a.degree_bits, a.alpha, a.zeta, a.permutation_challenges) == \
        (b.degree_bits, b.alpha, b.zeta, b.permutation_challenges)
    for field in ("trace_commit", "quotient_commit", "preprocessed_commit", "permutation_commit"):
        fa, fb = flat(getattr(a, field)), flat(getattr(b, field))
        assert len(fa) == len(fb) and all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb)), field
    assert len(a.opened) == len(b.opened)
    for oa, ob in zip(a.opened, b.opened):
        for part in ("values", "witnesses"):
            fa, fb = flat(getattr(oa, part)), flat(getattr(ob, part))
            assert len(fa) == len(fb) and all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb)), part


def verdict(job, pcs, proof, vk, ch_consts):
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants, VerificationError, verify_native

    ch = Challenger(Poseidon2Constants(*ch_consts)) if job.fs else None
    try:
        verify_native(job.prog, pcs, proof, job.publics, challenger=ch, preprocessed_vk=vk)
    except VerificationError as e:
        return e.kind
    return None


@pytest.mark.parametrize("name", ["fibonacci", "mixed_fs", "mixed_pre_fs", "p2air"])
def test_proofs_over_a_supplied_srs_are_the_alpha_handles(handles, jobs, ch_consts, name):
    pcs, _ = handles
    job = jobs[name]
    ref, vk = run_prove(job, pcs["alpha"], ch_consts)
    want = verdict(job, pcs["alpha"], ref, vk, ch_consts)
    assert want == (None if job.satisfiable else "OodEvaluationMismatch")
    bad = copy.deepcopy(ref)
    v = ints(bad.opened[0].values[0][0])
    v[0] = (v[0] + 1) % O.P  # one opened value flipped
    bad.opened[0].values[0][0] = np.stack([lim(x) for x in v])
    want_bad = verdict(job, pcs["alpha"], bad, vk, ch_consts)
    assert want_bad == "InvalidOpeningArgument"
    for how in ("affine", "bytes", "loaded"):
        got, vk2 = run_prove(job, pcs[how], ch_consts)
        assert_same_proof(got, ref)
        if vk is not None:
            assert vk2[:2] == vk[:2] and vk2[2].tobytes() == vk[2].tobytes()
        # each proof on the other handle, and on the verifier's
        assert verdict(job, pcs["alpha"], got, vk, ch_consts) == want
        assert verdict(job, pcs[how], ref, vk, ch_consts) == want
        assert verdict(job, pcs["verifier"], got, vk, ch_consts) == want
        assert verdict(job, pcs[how], bad, vk, ch_consts) == want_bad
    assert verdict(job, pcs["verifier"], bad, vk, ch_consts) == want_bad


def test_srs_length_bounds_the_degree(gpu_ctx, handles, jobs):
    """8 rows, quotient chunks of 8 rows: degree 7, so 8 powers prove and 7 do not"""
    from plonky3_eon_amd import EonError, _lib
    from plonky3_eon_amd.native import NativeKzgPcs, prove_native

    _, srs = handles
    job = jobs["fibonacci"]
    short = NativeKzgPcs.from_srs(srs.prefix(6), rho=RHO, ctx=gpu_ctx)
    with pytest.raises(EonError) as e:
        prove_native(job.prover, short, job.trace, 3, 5, public_values=job.publics)
    assert e.value.code == _lib.EON_E_DEGREE_TOO_LARGE
    short.close()
    exact = NativeKzgPcs.from_srs(srs.prefix(7), rho=RHO, ctx=gpu_ctx)
    got = prove_native(job.prover, exact, job.trace, 3, 5, public_values=job.publics)
    assert_same_proof(got, prove_native(job.prover, handles[0]["alpha"], job.trace, 3, 5, public_values=job.publics))
    exact.close()


def test_verifier_handle_does_not_prove(handles, jobs):
    from plonky3_eon_amd import EonError, _lib
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    v = handles[0]["verifier"]
    for name in ("fibonacci", "p2air"):
        job = jobs[name]
        with pytest.raises(EonError) as e:
            prove_native(job.prover, v, job.trace, 3, 5, **(dict(public_values=job.publics) if job.publics else {}))
        assert e.value.code == _lib.EON_E_ARG and "verifier-only" in str(e.value)
    with pytest.raises(EonError) as e:
        setup_preprocessed(v, jobs["mixed_pre_fs"].pre)
    assert e.value.code == _lib.EON_E_ARG and "verifier-only" in str(e.value)
