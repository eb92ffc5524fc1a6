"""native.verify_native (eon_verify_air / eon_verify_air_fs): the product's own verifier, with the
reference's verdict and VerificationError variant (eon-uni-stark/src/verifier.rs:244-502).

Honest proofs of prove_native verify, with Fiat-Shamir (the challenger ends where the prover's did)
and with given challenges; the verdict and the derived alpha / zeta agree with the CPU mirrors
(verify_oracle.verify_kzg_proof, mirror_preprocessed.verify, mirror_lookup.verify) on the same
proofs; every way of spoiling a proof yields exactly the named variant.  Heights 2^3 and 2^4.

The proofs are made once per module and never modified: every spoiled proof is a deep copy."""

import copy

import numpy as np
import pytest

import mirror_lookup as ML
import mirror_preprocessed as MP
from airs import FibonacciAir, MulAir
from airs_lookup import (LookupMultisetEqAir, RangeCheckAir, multiset_constraints, multiset_trace,
                         range_check_constraints, range_check_preprocessed, range_check_trace)
from airs_preprocessed import MixedPreAir, mixed_pre_constraints, mixed_pre_preprocessed, mixed_pre_trace
from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V
from oracle.smallrng import SmallRng, poseidon2_new_from_rng
from test_gpu_air_program import mul_constraints, mul_trace

pytestmark = pytest.mark.gpu
P = O.P
SRS_ALPHA = 12345
ints, lim, to_limbs = ML.ints, ML.lim, ML.to_limbs
GIVEN = dict(alpha=0x1111222233334444, zeta=0x5555666677778888)
OK, SHAPE, OPENING, OOD = None, "InvalidProofShape", "InvalidOpeningArgument", "OodEvaluationMismatch"


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def rand_ints(seed, n):
    return [int(x) for x in ints(C.random_fr(seed, n))]


@pytest.fixture(scope="module")
def ch_consts():
    # the reference's challenger permutation: Perm::new_from_rng(4, 22, SmallRng(1)) (fib_air.rs:113-115)
    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    return py, ([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]])


def challenger(ch_consts):
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants

    return Challenger(Poseidon2Constants(*ch_consts[1]))


@pytest.fixture(scope="module")
def pcs(gpu_ctx):
    from plonky3_eon_amd.native import NativeKzgPcs

    p = NativeKzgPcs(1024, SRS_ALPHA, gpu_ctx)
    yield p
    p.close()


class Case:
    """One AIR with a trace: the program that verifies, what prove_native takes, the verifier key
    and the CPU mirror's verify of a proof -> {"transcript", "ood", "kzg"}."""

    def __init__(self, prog, trace, log_n, mirror, prover=None, publics=(), prove_kw=None, vk=None, lookups=False):
        self.prog, self.trace, self.log_n, self.mirror = prog, trace, log_n, mirror
        self.prover = prover if prover is not None else prog  # the fused Poseidon2Air proves, its program verifies
        self.publics, self.prove_kw, self.vk, self.lookups = list(publics), prove_kw or {}, vk, lookups
        self.proofs, self.prover_state = {}, {}


def generic_mirror(fn, log_n, log_qd, publics=()):
    def run(proof, py, fs):
        kw = dict(challenger=O.DuplexChallenger(py)) if fs else dict(alpha=proof.alpha, zeta=proof.zeta)
        return V.verify_kzg_proof(proof, fn, log_n, log_qd, SRS_ALPHA, publics=list(publics), **kw)

    return run


@pytest.fixture(scope="module")
def cases(gpu_ctx, pcs, ch_consts):
    """name -> Case with proofs["fs"] and proofs["given"], proved once"""
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    py = ch_consts[0]
    out = {}
    pis = [0, 1, 21]
    out["fibonacci"] = Case(AirProgram(FibonacciAir(), gpu_ctx), to_limbs(O.fib_trace(0, 1, 8)), 3,
                            generic_mirror(V.fib_constraint_fn(pis), 3, 0, pis), publics=pis)
    mul_fn = lambda loc, nxt, sels: mul_constraints(loc, nxt, sels[:3], ())  # noqa: E731
    mul = AirProgram(MulAir(), gpu_ctx)
    assert mul.log_quotient_degree() == 1  # two quotient chunks
    out["mul"] = Case(mul, to_limbs(mul_trace(8)), 3, generic_mirror(mul_fn, 3, 1))
    out["mul_invalid"] = Case(mul, to_limbs(mul_trace(8, valid=False)), 3, generic_mirror(mul_fn, 3, 1))

    n = 16
    rows, pub = mixed_pre_trace(3, 4, 5, n)
    pre = to_limbs(mixed_pre_preprocessed(n))
    pp = setup_preprocessed(pcs, dev(pre))
    mixed = AirProgram(MixedPreAir(), gpu_ctx)
    assert mixed.log_quotient_degree() == 2  # four chunks

    def mixed_mirror(proof, py, fs, commit=pp.commitment):
        kw = dict(challenger=O.DuplexChallenger(py)) if fs else dict(alpha=proof.alpha, zeta=proof.zeta)
        return MP.verify(proof, commit, 3, mixed_pre_constraints, 4, 2, SRS_ALPHA, publics=pub, **kw)

    out["mixed_pre"] = Case(mixed, to_limbs(rows), 4, mixed_mirror, publics=pub, prove_kw=dict(preprocessed=pp), vk=pp)

    rows, pub_r = range_check_trace(n)
    pre_r = to_limbs(range_check_preprocessed(n))
    pp_r = setup_preprocessed(pcs, dev(pre_r))

    def range_mirror(proof, py, fs):
        kw = dict(challenger=O.DuplexChallenger(py)) if fs else dict(
            challenges=proof.permutation_challenges, alpha=proof.alpha, zeta=proof.zeta)
        return ML.verify(proof, pp_r.commitment, range_check_constraints, 2, 4, 1, SRS_ALPHA, publics=pub_r, **kw)[0]

    out["range_check"] = Case(AirProgram(RangeCheckAir(), gpu_ctx), to_limbs(rows), 4, range_mirror, publics=pub_r,
                              prove_kw=dict(preprocessed=pp_r, preprocessed_trace=dev(pre_r)), vk=pp_r, lookups=True)

    def multiset_mirror(proof, py, fs):
        kw = dict(challenger=O.DuplexChallenger(py)) if fs else dict(
            challenges=proof.permutation_challenges, alpha=proof.alpha, zeta=proof.zeta)
        return ML.verify(proof, None, multiset_constraints, 1, 3, 1, SRS_ALPHA, **kw)[0]

    ms = AirProgram(LookupMultisetEqAir(), gpu_ctx)
    out["multiset"] = Case(ms, to_limbs(multiset_trace(8)), 3, multiset_mirror, lookups=True)
    out["multiset_bad"] = Case(ms, to_limbs(multiset_trace(8, bad=True)), 3, multiset_mirror, lookups=True)

    p2py = O.p2_constants(2024, 4, 56)
    k = C.P2Constants([[lim(v) for v in r] for r in p2py[0]], [lim(v) for v in p2py[1]],
                      [[lim(v) for v in r] for r in p2py[2]])
    for vl in (1, 8):
        air = Poseidon2Air(k.begin, k.partial, k.end, vl, gpu_ctx)
        trace = air.generate_trace(dev(C.random_fr(60 + vl, 8 * vl * 3).reshape(8 * vl, 3, 4)))
        out[f"poseidon2_vl{vl}"] = Case(AirProgram(air, gpu_ctx), trace, 3,
                                        generic_mirror(V.p2air_constraint_fn(p2py, vl), 3, 1), prover=air)

    for name, c in out.items():
        trace = c.trace if not isinstance(c.trace, np.ndarray) else dev(c.trace)
        kw = dict(c.prove_kw)
        if c.publics:
            kw["public_values"] = c.publics
        ch = challenger(ch_consts)
        c.proofs["fs"] = prove_native(c.prover, pcs, trace, None, None, challenger=ch, **kw)
        c.prover_state["fs"] = (ch.state().copy(), ch.sample().copy())  # the sponge, and what it gives next
        if c.lookups:
            kw["permutation_challenges"] = rand_ints(77, c.prog.num_challenges)
        c.proofs["given"] = prove_native(c.prover, pcs, trace, GIVEN["alpha"], GIVEN["zeta"], **kw)
    yield out
    pp.close()
    pp_r.close()


def verdict_of(mirror_res):
    """the reference's verdict from a mirror's named checks: the openings are checked before the
    out-of-domain identity, and a transcript the proof was not made with moves the points they are
    checked at"""
    if not mirror_res.get("transcript", True) or not mirror_res["kzg"]:
        return OPENING
    return OK if mirror_res["ood"] else OOD


def native_verdict(case, pcs, proof, ch=None, vk="case", publics=None, transcript=None):
    from plonky3_eon_amd.native import VerificationError, verify_native

    try:
        r = verify_native(case.prog, pcs, proof, case.publics if publics is None else publics, challenger=ch,
                          preprocessed_vk=case.vk if vk == "case" else vk, transcript=transcript)
    except VerificationError as e:
        assert e.kind in (SHAPE, OPENING, OOD) and str(e).startswith(e.kind)
        return e.kind
    assert r is None
    return OK


HONEST = ("fibonacci", "mul", "mixed_pre", "range_check", "multiset", "poseidon2_vl1", "poseidon2_vl8")


@pytest.mark.parametrize("mode", ["fs", "given"])
@pytest.mark.parametrize("name", HONEST)
def test_honest_proofs_verify(cases, pcs, ch_consts, name, mode):
    c = cases[name]
    proof = c.proofs[mode]
    ch = challenger(ch_consts) if mode == "fs" else None
    used = {}
    assert native_verdict(c, pcs, proof, ch, transcript=used) is OK
    assert (used["alpha"], used["zeta"]) == (proof.alpha, proof.zeta)
    assert used["permutation_challenges"] == list(proof.permutation_challenges or [])
    res = c.mirror(proof, ch_consts[0], mode == "fs")
    assert verdict_of(res) is OK and res.get("transcript", True), res
    if mode == "fs":  # the challenger was advanced exactly as the prover's
        state, nxt = c.prover_state["fs"]
        np.testing.assert_array_equal(ch.state(), state)
        np.testing.assert_array_equal(ch.sample(), nxt)


@pytest.mark.parametrize("mode", ["fs", "given"])
@pytest.mark.parametrize("name", ["mul_invalid", "multiset_bad"])
def test_invalid_trace_is_an_ood_mismatch(cases, pcs, ch_consts, name, mode):
    """proved with the constraint check off from a trace that breaks the AIR: the transcript and
    every opening are fine, the out-of-domain identity is not"""
    c = cases[name]
    proof = c.proofs[mode]
    used = {}
    assert native_verdict(c, pcs, proof, challenger(ch_consts) if mode == "fs" else None, transcript=used) == OOD
    assert (used["alpha"], used["zeta"]) == (proof.alpha, proof.zeta)
    res = c.mirror(proof, ch_consts[0], mode == "fs")
    assert res["kzg"] and not res["ood"] and verdict_of(res) == OOD, res


def bump(values, col=0):
    """the (w, 4) opened values with column `col` one more"""
    v = ints(values)
    v[col] = (v[col] + 1) % P
    return np.stack([lim(x) for x in v])


def spoil_trace_value(p):
    p.opened[0].values[0][1] = bump(p.opened[0].values[0][1], 1)


def spoil_quotient_value(p):
    quot = p.opened[2 if p.permutation_commit is not None else 1]  # trace, (permutation), quotient chunks
    quot.values[0][0] = bump(quot.values[0][0])


def spoil_witness_other(p):
    """column 0's witness at zeta replaced by its witness at zeta h: still a curve point.  (Two
    witnesses SWAPPED at one point would pass, here as in the reference: verify_batch,
    kzg/src/util.rs:245-292, multiplies the pairings without random weights, so only their sum per
    point enters.)"""
    w = np.array(p.opened[0].witnesses[0][0], dtype=np.uint64).reshape(-1, 8).copy()
    w[0] = np.asarray(p.opened[0].witnesses[0][1], dtype=np.uint64).reshape(-1, 8)[0]
    p.opened[0].witnesses[0][0] = w


def spoil_witness_bit(p):
    w = np.array(p.opened[0].witnesses[0][0], dtype=np.uint64).reshape(-1, 8).copy()
    w[0, 0] ^= np.uint64(1)  # no longer on the curve
    p.opened[0].witnesses[0][0] = w


@pytest.mark.parametrize("mode", ["fs", "given"])
@pytest.mark.parametrize("spoil", [spoil_trace_value, spoil_quotient_value, spoil_witness_other, spoil_witness_bit],
                         ids=["trace_value", "quotient_chunk", "witness_other", "witness_bit"])
@pytest.mark.parametrize("name", ["fibonacci", "mixed_pre", "range_check"])
def test_spoiled_opening_is_an_invalid_opening_argument(cases, pcs, ch_consts, name, spoil, mode):
    c = cases[name]
    bad = copy.deepcopy(c.proofs[mode])
    spoil(bad)
    assert native_verdict(c, pcs, bad, challenger(ch_consts) if mode == "fs" else None) == OPENING
    if spoil is not spoil_witness_bit:  # the mirror's curve arithmetic takes curve points only
        res = c.mirror(bad, ch_consts[0], mode == "fs")
        assert not res["kzg"] and verdict_of(res) == OPENING, res


def test_changed_commitment_or_public_value_moves_the_challenges(cases, pcs, ch_consts):
    """under Fiat-Shamir the verifier derives other challenges than the proof was made with"""
    c = cases["fibonacci"]
    proof = c.proofs["fs"]
    bad = copy.deepcopy(proof)
    tc = np.array(bad.trace_commit[0], dtype=np.uint64).reshape(-1, 8).copy()
    tc[0] = tc[1]  # another curve point
    bad.trace_commit = [tc]
    used = {}
    assert native_verdict(c, pcs, bad, challenger(ch_consts), transcript=used) == OPENING
    qc = np.stack([np.asarray(q, dtype=np.uint64).reshape(8) for q in bad.quotient_commit])
    want = V.replay_transcript(O.DuplexChallenger(ch_consts[0]), 3, tc, qc, c.publics)
    assert (used["alpha"], used["zeta"]) == want and want != (proof.alpha, proof.zeta)
    assert verdict_of(c.mirror(bad, ch_consts[0], True)) == OPENING
    # a public value that is not the prover's
    pis = [0, 1, 22]
    used = {}
    assert native_verdict(c, pcs, proof, challenger(ch_consts), publics=pis, transcript=used) == OPENING
    tc = np.asarray(proof.trace_commit[0], dtype=np.uint64).reshape(-1, 8)
    want = V.replay_transcript(O.DuplexChallenger(ch_consts[0]), 3, tc, qc, pis)
    assert (used["alpha"], used["zeta"]) == want and want != (proof.alpha, proof.zeta)
    # with the challenges given, the same public value leaves the openings valid and breaks the identity
    assert native_verdict(c, pcs, c.proofs["given"], publics=pis) == OOD


@pytest.mark.parametrize("mode", ["fs", "given"])
def test_foreign_verifier_key_commitment(cases, pcs, ch_consts, mode):
    """the key's commitment is the one observed and checked, never the proof's copy"""
    c = cases["mixed_pre"]
    proof = c.proofs[mode]
    # column 0's commitment replaced by column 1's: curve points, another sum (a mere permutation of
    # the columns' commitments would leave the unweighted batch of the reference unchanged)
    foreign = np.asarray(c.vk.commitment, dtype=np.uint64).reshape(-1, 8).copy()
    foreign[0] = foreign[1]
    assert not np.array_equal(foreign, c.vk.commitment)
    ch = challenger(ch_consts) if mode == "fs" else None
    assert native_verdict(c, pcs, proof, ch, vk=(3, 4, foreign)) == OPENING
    res = c.mirror(proof, ch_consts[0], mode == "fs", commit=foreign)
    assert verdict_of(res) == OPENING, res
    # the same key as plain values verifies
    ch = challenger(ch_consts) if mode == "fs" else None
    assert native_verdict(c, pcs, proof, ch, vk=(3, 4, c.vk.commitment)) is OK


@pytest.mark.parametrize("mode", ["fs", "given"])
def test_invalid_proof_shapes(cases, pcs, ch_consts, mode):
    fs = mode == "fs"
    ch = challenger(ch_consts) if fs else None
    zero = ch.state().copy() if fs else None
    mixed, fib, rng = cases["mixed_pre"], cases["fibonacci"], cases["range_check"]
    commit = mixed.vk.commitment
    # the key's degree_bits against the proof's
    assert native_verdict(mixed, pcs, mixed.proofs[mode], ch, vk=(3, 5, commit)) == SHAPE
    # a key given to a program without preprocessed columns
    assert native_verdict(fib, pcs, fib.proofs[mode], ch, vk=(3, 3, commit)) == SHAPE
    # no key for a program with them
    assert native_verdict(mixed, pcs, mixed.proofs[mode], ch, vk=None) == SHAPE
    # a lookup program's proof without its permutation part
    bad = copy.deepcopy(rng.proofs[mode])
    bad.permutation_commit, bad.permutation_challenges = None, None
    del bad.opened[1]
    assert native_verdict(rng, pcs, bad, ch) == SHAPE
    if fs:  # a shape is rejected before the transcript: the challenger has observed nothing
        np.testing.assert_array_equal(ch.state(), zero)
        np.testing.assert_array_equal(ch.sample(), challenger(ch_consts).sample())


def test_array_shapes_are_rejected_before_any_c_call(cases):
    """opened widths against the program's width, the chunk count against log_quotient_degree, the
    permutation width: InvalidProofShape with no pcs to call"""
    from plonky3_eon_amd.native import VerificationError, verify_native

    def shape_error(case, proof, **kw):
        with pytest.raises(VerificationError) as e:
            verify_native(case.prog, None, proof, case.publics, preprocessed_vk=case.vk, **kw)
        assert e.value.kind == SHAPE

    fib, mul, rng = cases["fibonacci"], cases["mul"], cases["range_check"]
    bad = copy.deepcopy(fib.proofs["given"])
    bad.opened[0].values[0][0] = np.asarray(bad.opened[0].values[0][0])[:1]
    shape_error(fib, bad)
    bad = copy.deepcopy(fib.proofs["given"])
    bad.trace_commit = [np.asarray(bad.trace_commit[0])[:1]]
    shape_error(fib, bad)
    bad = copy.deepcopy(mul.proofs["given"])  # one chunk of two
    bad.quotient_commit = bad.quotient_commit[:1]
    bad.opened[1].values, bad.opened[1].witnesses = bad.opened[1].values[:1], bad.opened[1].witnesses[:1]
    shape_error(mul, bad)
    bad = copy.deepcopy(rng.proofs["given"])  # one permutation column of two
    bad.permutation_commit = [np.asarray(bad.permutation_commit[0])[:1]]
    shape_error(rng, bad)
    bad = copy.deepcopy(rng.proofs["given"])
    bad.opened[1].witnesses[0][1] = np.asarray(bad.opened[1].witnesses[0][1])[:1]
    shape_error(rng, bad)
    bad = copy.deepcopy(rng.proofs["given"])  # the preprocessed openings against the key's width
    bad.opened[3].values[0][0] = np.concatenate([np.asarray(bad.opened[3].values[0][0])] * 2)
    shape_error(rng, bad)


@pytest.mark.parametrize("mode", ["fs", "given"])
def test_srs_smaller_than_the_trace_degree(gpu_ctx, cases, ch_consts, mode):
    """ensure_supported (kzg/src/params.rs:164-173) fails inside KzgPcs::verify: an opening error"""
    from plonky3_eon_amd.native import NativeKzgPcs

    small = NativeKzgPcs(4, SRS_ALPHA, gpu_ctx)  # degree 7 needed
    try:
        c = cases["fibonacci"]
        ch = challenger(ch_consts) if mode == "fs" else None
        assert native_verdict(c, small, c.proofs[mode], ch) == OPENING
        if ch is not None:  # the transcript ran first, as in the reference
            np.testing.assert_array_equal(ch.state(), c.prover_state["fs"][0])
    finally:
        small.close()
