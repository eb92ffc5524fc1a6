"""The batched KZG opening mode through prove_native / verify_native (EON_OPENING_BATCHED):
one witness per (matrix, point), gamma-folded columns, a delta-weighted verify.

Four AIRs -- Fibonacci with public values, the multiset lookup AIR, the preprocessed AIR and the
fused Poseidon2-AIR at VECTOR_LEN 1 -- each with fixed challenges and with Fiat-Shamir, heights 2^3
and 2^4, an SRS of 2^8 powers.  Against the per-column proof of the same inputs and against
tests/mirror_batched.py (Python integers, the test SRS's trapdoor).

The proofs are made once per module and never modified: every spoiled proof is a deep copy."""

import copy
import dataclasses

import numpy as np
import pytest

import mirror_batched as MB
import mirror_lookup as ML
import mirror_preprocessed as MP
from airs import FibonacciAir
from airs_lookup import LookupMultisetEqAir, multiset_permuted_trace, multiset_terms
from airs_preprocessed import MixedPreAir, mixed_pre_preprocessed, mixed_pre_trace
from oracle import coracle as C
from oracle import pyoracle as O
from oracle.smallrng import SmallRng, poseidon2_new_from_rng

pytestmark = pytest.mark.gpu
P = O.P
SRS_ALPHA = 12345
ints, lim, to_limbs = ML.ints, ML.lim, ML.to_limbs
GIVEN = dict(alpha=0x1111222233334444, zeta=0x5555666677778888)
GAMMA = 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF
DELTA = 0x0FEDCBA9876543210FEDCBA9876543210FEDCBA987654321
NAMES = ("fibonacci", "multiset", "mixed_pre", "poseidon2_vl1")
MODES = ("fs", "given")
SHAPE, OPENING = "InvalidProofShape", "InvalidOpeningArgument"


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


@pytest.fixture(scope="module")
def ch_consts():
    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    return py, ([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]])


def challenger(ch_consts):
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants

    return Challenger(Poseidon2Constants(*ch_consts[1]))


@pytest.fixture(scope="module")
def pcs(gpu_ctx):
    from plonky3_eon_amd.native import NativeKzgPcs

    p = NativeKzgPcs(255, SRS_ALPHA, gpu_ctx)  # 2^8 powers
    yield p
    p.close()


class Case:
    def __init__(self, prog, trace, rows, log_n, prover=None, publics=(), prove_kw=None, vk=None, pre_rows=None,
                 perm_of=None):
        self.prog, self.trace, self.rows, self.log_n = prog, trace, rows, log_n
        self.prover = prover if prover is not None else prog
        self.publics, self.prove_kw, self.vk = list(publics), prove_kw or {}, vk
        self.pre_rows, self.perm_of = pre_rows, perm_of  # int rows; challenges -> the permutation trace's int rows
        self.per_column, self.batched, self.prover_state = {}, {}, {}


@pytest.fixture(scope="module")
def cases(gpu_ctx, pcs, ch_consts):
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    out = {}
    pis = [0, 1, 21]
    fib = O.fib_trace(0, 1, 8)
    out["fibonacci"] = Case(AirProgram(FibonacciAir(), gpu_ctx), to_limbs(fib), [list(r) for r in fib], 3, publics=pis)

    ms_rows = multiset_permuted_trace(8)
    out["multiset"] = Case(AirProgram(LookupMultisetEqAir(), gpu_ctx), to_limbs(ms_rows), ms_rows, 3,
                           perm_of=lambda ch: ML.generate_permutation(multiset_terms, ms_rows, None, (), ch, 1))

    n = 16
    rows, pub = mixed_pre_trace(3, 4, 5, n)
    pre_rows = mixed_pre_preprocessed(n)
    pp = setup_preprocessed(pcs, dev(to_limbs(pre_rows)))
    out["mixed_pre"] = Case(AirProgram(MixedPreAir(), gpu_ctx), to_limbs(rows), rows, 4, publics=pub,
                            prove_kw=dict(preprocessed=pp), vk=pp, pre_rows=pre_rows)

    p2py = O.p2_constants(2024, 4, 56)
    k = C.P2Constants([[lim(v) for v in r] for r in p2py[0]], [lim(v) for v in p2py[1]],
                      [[lim(v) for v in r] for r in p2py[2]])
    air = Poseidon2Air(k.begin, k.partial, k.end, 1, gpu_ctx)
    trace = air.generate_trace(dev(C.random_fr(61, 8 * 3).reshape(8, 3, 4)))
    host = trace.cpu().numpy().view(np.uint64)
    out["poseidon2_vl1"] = Case(AirProgram(air, gpu_ctx), trace, [ints(r) for r in host], 3, prover=air)

    for name, c in out.items():
        trace = c.trace if not isinstance(c.trace, np.ndarray) else dev(c.trace)
        kw = dict(c.prove_kw)
        if c.publics:
            kw["public_values"] = c.publics
        given = dict(kw)
        if c.perm_of is not None:
            given["permutation_challenges"] = [int(x) for x in ints(C.random_fr(77, c.prog.num_challenges))]
        # the per-column proofs first: made before set_opening is ever called on this pcs for this case
        c.per_column["fs"] = prove_native(c.prover, pcs, trace, None, None, challenger=challenger(ch_consts), **kw)
        c.per_column["given"] = prove_native(c.prover, pcs, trace, GIVEN["alpha"], GIVEN["zeta"], **given)
        ch = challenger(ch_consts)
        c.batched["fs"] = prove_native(c.prover, pcs, trace, None, None, challenger=ch, opening="batched", **kw)
        c.prover_state["fs"] = (ch.state().copy(), ch.sample().copy())
        c.batched["given"] = prove_native(c.prover, pcs, trace, GIVEN["alpha"], GIVEN["zeta"], opening="batched",
                                          gamma=GAMMA, delta=DELTA, **given)
        c.device_trace, c.given_kw, c.fs_kw = trace, given, kw
    yield out
    pp.close()


def verdict(case, pcs, proof, ch=None, transcript=None):
    from plonky3_eon_amd.native import VerificationError, verify_native

    try:
        r = verify_native(case.prog, pcs, proof, case.publics, challenger=ch, preprocessed_vk=case.vk,
                          transcript=transcript)
    except VerificationError as e:
        return e.kind
    assert r is None
    return None


def ch_for(mode, ch_consts):
    return challenger(ch_consts) if mode == "fs" else None


def quot_index(proof):
    return 2 if proof.permutation_commit is not None else 1


# ---- (a) everything but the witnesses is the per-column proof's ------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_commitments_values_and_challenges_equal_the_per_column_proof(cases, name, mode):
    b, p = cases[name].batched[mode], cases[name].per_column[mode]
    assert (b.opening, p.opening) == ("batched", "per_column") and (p.gamma, p.delta) == (None, None)
    assert (b.alpha, b.zeta) == (p.alpha, p.zeta) and b.degree_bits == p.degree_bits
    assert b.permutation_challenges == p.permutation_challenges
    np.testing.assert_array_equal(b.trace_commit[0], p.trace_commit[0])
    np.testing.assert_array_equal(np.stack(b.quotient_commit), np.stack(p.quotient_commit))
    for name_ in ("permutation_commit", "preprocessed_commit"):
        assert (getattr(b, name_) is None) == (getattr(p, name_) is None)
        if getattr(b, name_) is not None:
            np.testing.assert_array_equal(getattr(b, name_)[0], getattr(p, name_)[0])
    assert len(b.opened) == len(p.opened)
    for ob, op in zip(b.opened, p.opened):
        assert len(ob.values) == len(op.values)
        for vb, vp in zip(ob.values, op.values):
            assert len(vb) == len(vp)
            for x, y in zip(vb, vp):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


# ---- (b) the witnesses ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_witnesses_equal_the_mirror_and_chunk_witnesses_the_per_column_ones(cases, name, mode):
    c = cases[name]
    b, p = c.batched[mode], c.per_column[mode]
    if mode == "given":
        assert (b.gamma, b.delta) == (GAMMA, DELTA)
    zeta = b.zeta
    points = [zeta, zeta * MB.two_adic_generator(c.log_n) % P]
    mats = [(0, c.rows)]
    if c.perm_of is not None:
        mats.append((1, c.perm_of(b.permutation_challenges)))
    if c.pre_rows is not None:
        mats.append((len(b.opened) - 1, c.pre_rows))
    for r, evals in mats:
        values, wits = MB.open_batched_evals(evals, c.log_n, points, b.gamma, SRS_ALPHA)
        for t in range(2):
            assert np.asarray(b.opened[r].witnesses[0][t]).shape == (1, 8)
            assert ints(b.opened[r].values[0][t]) == values[t]
            np.testing.assert_array_equal(np.asarray(b.opened[r].witnesses[0][t])[0], MB.point(wits[t]))
    q = quot_index(b)
    assert len(b.opened[q].witnesses) == len(p.opened[q].witnesses) == len(b.quotient_commit)
    for wb, wp in zip(b.opened[q].witnesses, p.opened[q].witnesses):
        assert np.asarray(wb[0]).shape == (1, 8)
        np.testing.assert_array_equal(np.asarray(wb[0]), np.asarray(wp[0]))


@pytest.mark.parametrize("name", NAMES)
def test_fiat_shamir_gamma_and_delta_are_the_mirror_transcript(cases, ch_consts, name):
    """unchanged up to zeta; then the opened values in claim order, gamma, the K witnesses, delta"""
    c = cases[name]
    b = c.batched["fs"]
    ch = O.DuplexChallenger(ch_consts[0])
    vk_commit = c.vk.commitment if c.vk is not None else None
    MP.observe_instance(ch, c.log_n, b.trace_commit[0], c.vk.width if c.vk is not None else 0, vk_commit, c.publics)
    if b.permutation_commit is not None:
        assert [ch.sample() for _ in range(c.prog.num_challenges)] == b.permutation_challenges
        ch.observe_g1(MP._points(b.permutation_commit[0]))
    assert ch.sample() == b.alpha
    ch.observe_g1(MP._points(np.stack(b.quotient_commit)))
    assert ch.sample() == b.zeta
    claims = MB.claims_of(b, c.log_n, vk_commit)
    assert len(claims) == 2 + len(b.quotient_commit) + (2 if b.permutation_commit is not None else 0) + \
        (2 if c.vk is not None else 0)
    assert MB.transcript_tail(ch, claims) == (b.gamma, b.delta)
    assert MB.verify(claims, b.gamma, b.delta, SRS_ALPHA)


# ---- (c) verify -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_batched_proofs_verify_and_the_challengers_end_equal(cases, pcs, ch_consts, name, mode):
    c = cases[name]
    proof = c.batched[mode]
    ch = ch_for(mode, ch_consts)
    used = {}
    assert verdict(c, pcs, proof, ch, transcript=used) is None
    assert (used["alpha"], used["zeta"], used["gamma"], used["delta"]) == (proof.alpha, proof.zeta, proof.gamma,
                                                                          proof.delta)
    vk_commit = c.vk.commitment if c.vk is not None else None
    assert MB.verify(MB.claims_of(proof, c.log_n, vk_commit), proof.gamma, proof.delta, SRS_ALPHA)
    if mode == "fs":
        state, nxt = c.prover_state["fs"]
        np.testing.assert_array_equal(ch.state(), state)
        np.testing.assert_array_equal(ch.sample(), nxt)
    # the per-column proof of the same inputs still verifies on the same pcs
    assert verdict(c, pcs, c.per_column[mode], ch_for(mode, ch_consts)) is None


# ---- (d) rejected -----------------------------------------------------------------------------------
def bump(values, col=0):
    v = ints(values)
    v[col] = (v[col] + 1) % P
    return np.stack([lim(x) for x in v])


def spoil_value(p):
    p.opened[0].values[0][1] = bump(p.opened[0].values[0][1], 1)


def spoil_chunk_value(p):
    q = p.opened[quot_index(p)]
    q.values[0][0] = bump(q.values[0][0])


def spoil_witness(p):
    """the trace witness at zeta replaced by the one at zeta h: still a curve point"""
    p.opened[0].witnesses[0][0] = np.array(p.opened[0].witnesses[0][1], dtype=np.uint64).copy()


def spoil_swap_commitments(p):
    t = np.array(p.trace_commit[0], dtype=np.uint64).copy()
    t[[0, 1]] = t[[1, 0]]
    p.trace_commit = [t]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("spoil", [spoil_value, spoil_chunk_value, spoil_witness, spoil_swap_commitments],
                         ids=["value", "chunk_value", "witness", "swapped_commitments"])
@pytest.mark.parametrize("name", NAMES)
def test_spoiled_batched_proofs_are_invalid_opening_arguments(cases, pcs, ch_consts, name, spoil, mode):
    c = cases[name]
    bad = copy.deepcopy(c.batched[mode])
    spoil(bad)
    assert not np.array_equal(np.asarray(bad.trace_commit[0])[0], np.asarray(bad.trace_commit[0])[1])
    assert verdict(c, pcs, bad, ch_for(mode, ch_consts)) == OPENING


@pytest.mark.parametrize("name", NAMES)
def test_changed_gamma_or_delta_is_an_invalid_opening_argument(cases, pcs, name):
    """gamma: an honest proof does not verify under another gamma.

    delta: every claim of an honest proof holds on its own, so the weights multiply identities and
    NO delta can reject it -- that a changed delta is rejected can only show on a proof whose claims
    do not all hold.  The pair W_0 + delta (s - zeta h) E, W_1 - (s - zeta) E is tuned to cancel under
    the weights 1, delta: verify accepts it with exactly that delta (fixed challenges a prover knows
    in advance bind nothing; Fiat-Shamir samples delta after the witnesses) and rejects it with any
    other; the mirror says the same."""
    c = cases[name]
    proof = c.batched["given"]
    assert verdict(c, pcs, proof) is None
    assert verdict(c, pcs, dataclasses.replace(proof, gamma=GAMMA + 1)) == OPENING
    assert verdict(c, pcs, dataclasses.replace(proof, delta=DELTA + 1)) is None  # all claims hold
    zeta = proof.zeta
    zeta_next = zeta * MB.two_adic_generator(c.log_n) % P
    e = MB.point(0xE4E5E6)
    tuned = copy.deepcopy(proof)
    tuned.opened[0].witnesses[0][0] = C.g1_add(
        np.asarray(proof.opened[0].witnesses[0][0], dtype=np.uint64)[0],
        C.g1_mul(e, MB.V.fr_limbs(DELTA * (SRS_ALPHA - zeta_next) % P))).reshape(1, 8)
    tuned.opened[0].witnesses[0][1] = C.g1_add(
        np.asarray(proof.opened[0].witnesses[0][1], dtype=np.uint64)[0],
        C.g1_mul(e, MB.V.fr_limbs((zeta - SRS_ALPHA) % P))).reshape(1, 8)
    claims = MB.claims_of(tuned, c.log_n, c.vk.commitment if c.vk is not None else None)
    assert MB.verify(claims, GAMMA, DELTA, SRS_ALPHA) and not MB.verify(claims, GAMMA, DELTA + 1, SRS_ALPHA)
    assert not MB.verify(claims, GAMMA, 1, SRS_ALPHA)
    assert verdict(c, pcs, tuned) is None
    assert verdict(c, pcs, dataclasses.replace(tuned, delta=DELTA + 1)) == OPENING
    assert verdict(c, pcs, dataclasses.replace(tuned, delta=1)) == OPENING


def test_a_witness_off_the_curve_is_an_invalid_opening_argument(cases, pcs, ch_consts):
    c = cases["fibonacci"]
    for mode in MODES:
        bad = copy.deepcopy(c.batched[mode])
        w = np.array(bad.opened[0].witnesses[0][0], dtype=np.uint64).copy()
        w[0, 0] ^= np.uint64(1)
        bad.opened[0].witnesses[0][0] = w
        assert verdict(c, pcs, bad, ch_for(mode, ch_consts)) == OPENING


# ---- (e) the cancelling pair: what the delta weights are for --------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_cancelling_witness_pair_passes_unweighted_and_is_rejected(cases, pcs, ch_consts, name, mode):
    """W_0 + (s - zeta h) E and W_1 - (s - zeta) E: the unweighted product of the reference's
    verify_batch cannot see the pair, the weighted one does"""
    c = cases[name]
    proof = c.batched[mode]
    zeta = proof.zeta
    zeta_next = zeta * MB.two_adic_generator(c.log_n) % P
    e = MB.point(0xE1E2E3)
    w0 = C.g1_add(np.asarray(proof.opened[0].witnesses[0][0], dtype=np.uint64)[0],
                  C.g1_mul(e, MB.V.fr_limbs((SRS_ALPHA - zeta_next) % P)))
    w1 = C.g1_add(np.asarray(proof.opened[0].witnesses[0][1], dtype=np.uint64)[0],
                  C.g1_mul(e, MB.V.fr_limbs((zeta - SRS_ALPHA) % P)))
    bad = copy.deepcopy(proof)
    bad.opened[0].witnesses[0][0] = w0.reshape(1, 8)
    bad.opened[0].witnesses[0][1] = w1.reshape(1, 8)
    vk_commit = c.vk.commitment if c.vk is not None else None
    claims = MB.claims_of(bad, c.log_n, vk_commit)
    assert MB.verify(claims, proof.gamma, 1, SRS_ALPHA)  # the unweighted product accepts the pair
    if mode == "given":
        assert not MB.verify(claims, proof.gamma, proof.delta, SRS_ALPHA)
    assert verdict(c, pcs, bad, ch_for(mode, ch_consts)) == OPENING


# ---- (f) shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["fibonacci", "mixed_pre", "poseidon2_vl1"])
def test_a_proof_read_in_the_other_mode_is_an_invalid_proof_shape(cases, pcs, ch_consts, name, mode):
    c = cases[name]
    as_per_column = dataclasses.replace(c.batched[mode], opening="per_column")
    assert verdict(c, pcs, as_per_column, ch_for(mode, ch_consts)) == SHAPE
    as_batched = dataclasses.replace(c.per_column[mode], opening="batched", gamma=GAMMA, delta=DELTA)
    assert verdict(c, pcs, as_batched, ch_for(mode, ch_consts)) == SHAPE


def test_shape_errors_come_before_any_c_call(cases):
    """no pcs at all: the shapes are checked in Python first"""
    from plonky3_eon_amd.native import VerificationError, verify_native

    c = cases["fibonacci"]
    for proof in (dataclasses.replace(c.batched["given"], opening="per_column"),
                  dataclasses.replace(c.per_column["given"], opening="batched", gamma=GAMMA, delta=DELTA),
                  dataclasses.replace(c.batched["given"], opening="folded")):
        with pytest.raises(VerificationError) as e:
            verify_native(c.prog, None, proof, c.publics)
        assert e.value.kind == SHAPE


def test_batched_mode_refuses_a_collective_and_missing_challenges(cases, pcs, ch_consts):
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.native import EON_OPENING_PER_COLUMN, EmulatedCollective, prove_native

    c = cases["poseidon2_vl1"]
    for kw in (dict(gamma=GAMMA), dict(challenger=challenger(ch_consts))):
        with pytest.raises(ValueError):
            prove_native(c.prover, pcs, c.device_trace, GIVEN["alpha"], GIVEN["zeta"],
                         collective=EmulatedCollective(0, 2), opening="batched", **kw)
    with pytest.raises(ValueError):
        prove_native(c.prover, pcs, c.device_trace, GIVEN["alpha"], GIVEN["zeta"], opening="folded")
    # fixed challenges: the prover needs gamma, the verifier gamma and delta (EON_E_ARG)
    with pytest.raises(_lib.EonError) as e:
        prove_native(c.prover, pcs, c.device_trace, GIVEN["alpha"], GIVEN["zeta"], opening="batched")
    assert e.value.code == _lib.EON_E_ARG
    with pytest.raises(_lib.EonError) as e:
        verdict(c, pcs, dataclasses.replace(c.batched["given"], delta=None))
    assert e.value.code == _lib.EON_E_ARG
    # the mode was restored after every call, the refused ones included; an unknown mode is refused
    assert pcs.lib.eon_kzg_pcs_opening(pcs._h) == EON_OPENING_PER_COLUMN
    assert pcs.lib.eon_kzg_pcs_set_opening(pcs._h, 7) == _lib.EON_E_ARG
    assert pcs.lib.eon_kzg_pcs_opening(pcs._h) == EON_OPENING_PER_COLUMN
    assert verdict(c, pcs, c.batched["given"]) is None


# ---- (g) the default mode is untouched ---------------------------------------------------------------
def proof_bytes(p):
    parts = [np.asarray(p.trace_commit[0]), np.stack(p.quotient_commit)]
    for o in p.opened:
        for m in o.values:
            parts += [np.asarray(x) for x in m]
        for m in o.witnesses:
            parts += [np.asarray(x) for x in m]
    for extra in (p.permutation_commit, p.preprocessed_commit):
        if extra is not None:
            parts.append(np.asarray(extra[0]))
    return b"".join(np.ascontiguousarray(x, dtype=np.uint64).tobytes() for x in parts)


@pytest.mark.parametrize("name", NAMES)
def test_default_mode_is_byte_identical_before_and_after_the_batched_mode(gpu_ctx, cases, pcs, ch_consts, name):
    """a fresh pcs on which set_opening was never called, against the module's pcs after its batched
    proves (the fixture's, at the least) and against that pcs's own first per-column proofs"""
    from plonky3_eon_amd.native import NativeKzgPcs, prove_native, setup_preprocessed

    c = cases[name]
    fresh = NativeKzgPcs(255, SRS_ALPHA, gpu_ctx)
    pp = None
    try:
        kw_fs, kw_given = dict(c.fs_kw), dict(c.given_kw)
        if c.vk is not None:
            pp = setup_preprocessed(fresh, dev(to_limbs(c.pre_rows)))
            kw_fs["preprocessed"] = kw_given["preprocessed"] = pp
        before_fs = prove_native(c.prover, fresh, c.device_trace, None, None, challenger=challenger(ch_consts), **kw_fs)
        before_given = prove_native(c.prover, fresh, c.device_trace, GIVEN["alpha"], GIVEN["zeta"], **kw_given)
    finally:
        if pp is not None:
            pp.close()
        fresh.close()
    after_fs = prove_native(c.prover, pcs, c.device_trace, None, None, challenger=challenger(ch_consts), **c.fs_kw)
    after_given = prove_native(c.prover, pcs, c.device_trace, GIVEN["alpha"], GIVEN["zeta"], **c.given_kw)
    for before, after, first in ((before_fs, after_fs, c.per_column["fs"]),
                                 (before_given, after_given, c.per_column["given"])):
        assert (before.alpha, before.zeta, before.opening) == (after.alpha, after.zeta, "per_column")
        assert proof_bytes(before) == proof_bytes(after) == proof_bytes(first)
