"""native.verify_native_many / verify_native_bytes_many (eon_verify_air_many[_fs]): a batch of
proofs verified in one pass -- one segmented pairing check, one launch of the constraints at every
zeta -- gives, per proof, exactly what native.verify_native gives for that proof alone: the same
VerificationError kind and detail (or None), the same reported challenges, and under Fiat-Shamir
the same end state of that proof's challenger.

Proofs of FibonacciAir (2^3 rows), MixedPreAir (with its verifier key), RangeCheckAir and
LookupMultisetEqAir (permutation part) and MulAir from prove_native, made once per module and never
modified: every spoiled proof is a deep copy."""

import copy
from pathlib import Path

import numpy as np
import pytest

from airs import FibonacciAir, MulAir
from airs_lookup import LookupMultisetEqAir, RangeCheckAir, multiset_trace, range_check_preprocessed, range_check_trace
from airs_preprocessed import MixedPreAir, mixed_pre_preprocessed, mixed_pre_trace
from oracle import pyoracle as O
from test_gpu_air_program import mul_trace
from test_gpu_verify_native import (GIVEN, OOD, OPENING, SHAPE, SRS_ALPHA, challenger, ch_consts, dev,  # noqa: F401
                                    rand_ints, spoil_quotient_value, spoil_trace_value, spoil_witness_bit, to_limbs)

pytestmark = pytest.mark.gpu
MODES = ("given", "fs")


@pytest.fixture(scope="module")
def pcs(gpu_ctx):
    from plonky3_eon_amd.native import NativeKzgPcs

    p = NativeKzgPcs(255, SRS_ALPHA, gpu_ctx)
    yield p
    p.close()


class Batch:
    """Proofs of one program: entry = (proof per mode, public values, verifier key)."""

    def __init__(self, prog):
        self.prog, self.entries = prog, []

    def add(self, proofs, publics=(), vk=None):
        self.entries.append((proofs, list(publics), vk))
        return self

    def proofs(self, mode):
        return [e[0][mode] for e in self.entries]

    def publics(self):
        return [e[1] for e in self.entries]

    def vks(self):
        return [e[2] for e in self.entries]


def spoiled(proofs, spoil):
    out = {}
    for mode, p in proofs.items():
        out[mode] = copy.deepcopy(p)
        spoil(out[mode])
    return out


@pytest.fixture(scope="module")
def made(gpu_ctx, pcs, ch_consts):  # noqa: F811
    """name -> Batch, every proof proved once in both modes"""
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    def prove(prog, rows, publics=(), lookups=False, **kw):
        trace = dev(to_limbs(rows))
        if publics:
            kw["public_values"] = list(publics)
        fs = prove_native(prog, pcs, trace, None, None, challenger=challenger(ch_consts), **kw)
        if lookups:
            kw["permutation_challenges"] = rand_ints(77, prog.num_challenges)
        if kw.get("opening") == "batched":
            kw.update(gamma=0x123456789, delta=0x987654321)
        return {"fs": fs, "given": prove_native(prog, pcs, trace, GIVEN["alpha"], GIVEN["zeta"], **kw)}

    out = {}
    fib = AirProgram(FibonacciAir(), gpu_ctx)
    honest = prove(fib, O.fib_trace(0, 1, 8), [0, 1, 21])
    other = prove(fib, O.fib_trace(2, 3, 8), [2, 3, 89])
    invalid = prove(fib, O.fib_trace(0, 1, 8), [0, 1, 22])  # the trace does not end in the public value
    wide = spoiled(honest, lambda p: setattr(p, "trace_commit", [np.zeros((3, 8), np.uint64)]))  # 3 columns: shape
    out["fibonacci"] = (Batch(fib).add(honest, [0, 1, 21]).add(spoiled(honest, spoil_trace_value), [0, 1, 21])
                        .add(other, [2, 3, 89]).add(invalid, [0, 1, 22]).add(wide, [0, 1, 21]))
    out["both_wrong"] = Batch(fib).add(spoiled(invalid, spoil_trace_value), [0, 1, 22]).add(honest, [0, 1, 21])
    fib_b = prove(fib, O.fib_trace(0, 1, 8), [0, 1, 21], opening="batched")
    other_b = prove(fib, O.fib_trace(2, 3, 8), [2, 3, 89], opening="batched")
    out["batched"] = (Batch(fib).add(fib_b, [0, 1, 21]).add(spoiled(fib_b, spoil_trace_value), [0, 1, 21])
                      .add(other_b, [2, 3, 89]).add(spoiled(other_b, spoil_witness_bit), [2, 3, 89]))
    out["mixed_modes"] = (Batch(fib).add(honest, [0, 1, 21]).add(fib_b, [0, 1, 21])
                          .add(spoiled(other_b, spoil_quotient_value), [2, 3, 89]).add(invalid, [0, 1, 22])
                          .add(other, [2, 3, 89]))

    n = 16
    rows, pub = mixed_pre_trace(3, 4, 5, n)
    pp = setup_preprocessed(pcs, dev(to_limbs(mixed_pre_preprocessed(n))))
    mixed = AirProgram(MixedPreAir(), gpu_ctx)
    mp = prove(mixed, rows, pub, preprocessed=pp)
    foreign = np.asarray(pp.commitment, dtype=np.uint64).reshape(-1, 8).copy()
    foreign[0] = foreign[1]  # curve points, another sum: the key observed and checked is the verifier's
    out["mixed_pre"] = (Batch(mixed).add(mp, pub, pp).add(mp, pub, (3, 4, foreign))
                        .add(spoiled(mp, spoil_quotient_value), pub, pp).add(mp, pub, pp))

    rows, pub_r = range_check_trace(n)
    pre_r = dev(to_limbs(range_check_preprocessed(n)))
    pp_r = setup_preprocessed(pcs, pre_r)
    rng = AirProgram(RangeCheckAir(), gpu_ctx)
    rp = prove(rng, rows, pub_r, lookups=True, preprocessed=pp_r, preprocessed_trace=pre_r)

    def no_permutation_part(p):
        p.permutation_commit, p.permutation_challenges = None, None
        del p.opened[1]

    out["range_check"] = (Batch(rng).add(rp, pub_r, pp_r).add(spoiled(rp, spoil_trace_value), pub_r, pp_r)
                          .add(spoiled(rp, no_permutation_part), pub_r, pp_r).add(rp, pub_r, pp_r))
    ms = AirProgram(LookupMultisetEqAir(), gpu_ctx)
    good, bad = prove(ms, multiset_trace(8), lookups=True), prove(ms, multiset_trace(8, bad=True), lookups=True)
    out["multiset"] = Batch(ms).add(good).add(bad).add(good)
    mul = AirProgram(MulAir(), gpu_ctx)
    out["mul"] = (Batch(mul).add(prove(mul, mul_trace(8))).add(prove(mul, mul_trace(8, valid=False)))
                  .add(prove(mul, mul_trace(8))))
    yield out
    pp.close()
    pp_r.close()


def outcome(e):
    return None if e is None else (type(e).__name__, e.kind, str(e))


def one_by_one(batch, pcs, mode, consts):
    """verify_native on every proof: (outcome, transcript, challenger state and next sample)"""
    from plonky3_eon_amd.native import VerificationError, verify_native

    out = []
    for proof, pub, vk in zip(batch.proofs(mode), batch.publics(), batch.vks()):
        ch = challenger(consts) if mode == "fs" else None
        used = {}
        try:
            res = verify_native(batch.prog, pcs, proof, pub, challenger=ch, preprocessed_vk=vk, transcript=used)
        except VerificationError as e:
            res = e
        out.append((outcome(res), used, (ch.state().copy(), ch.sample().copy()) if ch else None))
    return out


def all_at_once(batch, pcs, mode, consts, order=None):
    from plonky3_eon_amd.native import verify_native_many

    order = list(range(len(batch.entries))) if order is None else order
    chs = [challenger(consts) for _ in order] if mode == "fs" else None
    used = [{} for _ in order]
    proofs, pubs, vks = batch.proofs(mode), batch.publics(), batch.vks()
    res = verify_native_many(batch.prog, pcs, [proofs[i] for i in order], [pubs[i] for i in order], chs,
                             [vks[i] for i in order], used)
    return [(outcome(r), used[j], (chs[j].state().copy(), chs[j].sample().copy()) if chs else None)
            for j, r in enumerate(res)]


def assert_same(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    assert [g[1] for g in got] == [w[1] for w in want]  # the challenges each verifier used
    for g, w in zip(got, want):
        if w[2] is not None:  # the challenger ends where verify_native leaves it
            np.testing.assert_array_equal(g[2][0], w[2][0])
            np.testing.assert_array_equal(g[2][1], w[2][1])


KINDS = {"fibonacci": {"given": [None, OPENING, None, OOD, SHAPE], "fs": [None, OPENING, None, OOD, SHAPE]},
         "both_wrong": {m: [OPENING, None] for m in MODES},
         "batched": {m: [None, OPENING, None, OPENING] for m in MODES},
         "mixed_modes": {m: [None, None, OPENING, OOD, None] for m in MODES},
         "mixed_pre": {m: [None, OPENING, OPENING, None] for m in MODES},
         "range_check": {m: [None, OPENING, SHAPE, None] for m in MODES},
         "multiset": {m: [None, OOD, None] for m in MODES},
         "mul": {m: [None, OOD, None] for m in MODES}}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(KINDS))
def test_batch_equals_verify_native_on_each_proof(made, pcs, ch_consts, name, mode):  # noqa: F811
    """The kinds are the named ones (a proof whose opening and constraints are both wrong is an
    InvalidOpeningArgument: the reference's order of checks), and everything else -- the detail, the
    reported challenges, the challengers -- is verify_native's."""
    batch = made[name]
    want = one_by_one(batch, pcs, mode, ch_consts)
    assert [w[0] and w[0][1] for w in want] == KINDS[name][mode]
    got = all_at_once(batch, pcs, mode, ch_consts)
    assert_same(got, want)


@pytest.mark.parametrize("mode", MODES)
def test_reversed_batch_reverses_the_verdicts(made, pcs, ch_consts, mode):  # noqa: F811
    batch = made["fibonacci"]
    fwd = all_at_once(batch, pcs, mode, ch_consts)
    rev = all_at_once(batch, pcs, mode, ch_consts, order=[4, 3, 2, 1, 0])
    assert_same(rev, fwd[::-1])


@pytest.mark.parametrize("mode", MODES)
def test_batch_of_one_and_of_none(made, pcs, ch_consts, mode):  # noqa: F811
    from plonky3_eon_amd.native import verify_native_many

    batch = made["fibonacci"]
    want = one_by_one(batch, pcs, mode, ch_consts)
    for i in (0, 1, 3):
        assert_same(all_at_once(batch, pcs, mode, ch_consts, order=[i]), [want[i]])
    assert verify_native_many(batch.prog, pcs, []) == []
    assert verify_native_many(batch.prog, pcs, [], [], [] if mode == "fs" else None) == []


def test_more_proofs_than_prepare_threads(made, pcs, ch_consts):  # noqa: F811
    """19 proofs: past the 8 prepare threads, and 19 three-pair segments cross the 8 teams of a
    Miller block at every alignment."""
    batch = made["fibonacci"]
    order = [i % 4 for i in range(19)]
    want = one_by_one(batch, pcs, "fs", ch_consts)
    assert_same(all_at_once(batch, pcs, "fs", ch_consts, order=order), [want[i] for i in order])


def test_errors_name_the_proof(made, pcs):
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.native import verify_native, verify_native_many

    batch = made["fibonacci"]
    proofs = [copy.deepcopy(p) for p in batch.proofs("given")[:3]]
    proofs[2].zeta = 1
    # its openings were made at another zeta: rejected there, never evaluated
    res = verify_native_many(batch.prog, pcs, proofs, batch.publics()[:3])
    assert [r and r.kind for r in res] == [None, OPENING, OPENING]
    # (a proof that passes its openings at a zeta on the domain cannot be made.)  What verify_native
    # raises as an error code is raised for the batch, naming the proof: a wrong public value count
    proofs = batch.proofs("given")[:3]
    with pytest.raises(_lib.EonError) as e1:
        verify_native(batch.prog, pcs, proofs[0], [0, 1])
    with pytest.raises(_lib.EonError) as e2:
        verify_native_many(batch.prog, pcs, proofs, [[0, 1]] * 3)
    assert e1.value.code == e2.value.code == _lib.EON_E_SHAPE
    assert "public value count" in str(e1.value) and "proof 0: " in str(e2.value) and "public value count" in str(e2.value)


def test_bytes(made, pcs, ch_consts):  # noqa: F811
    from plonky3_eon_amd.native import verify_native_bytes_many
    from plonky3_eon_amd.proof import ProofFormatError

    batch = made["fibonacci"]
    want = one_by_one(batch, pcs, "fs", ch_consts)[:4]  # the fifth has no byte form: its shape is wrong
    blobs = [p.to_bytes() for p in batch.proofs("fs")[:4]]
    blobs.insert(2, blobs[0][:-5])
    chs = [challenger(ch_consts) for _ in blobs]
    zero = chs[2].state().copy()
    res = verify_native_bytes_many(batch.prog, pcs, blobs, [[0, 1, 21], [0, 1, 21], [0, 1, 21], [2, 3, 89], [0, 1, 22]],
                                   chs)
    assert isinstance(res[2], ProofFormatError)
    np.testing.assert_array_equal(chs[2].state(), zero)
    del res[2], chs[2]
    assert [outcome(r) for r in res] == [w[0] for w in want]
    for ch, w in zip(chs, want):
        np.testing.assert_array_equal(ch.state(), w[2][0])
    with pytest.raises(ValueError):
        verify_native_bytes_many(batch.prog, pcs, blobs)


def test_golden_proof(made, pcs, ch_consts):  # noqa: F811
    """tests/golden/proof_fib8_fs.bin verifies as a batch of one and as three copies."""
    from plonky3_eon_amd.native import verify_native_bytes_many

    blob = (Path(__file__).resolve().parent / "golden" / "proof_fib8_fs.bin").read_bytes()
    prog = made["fibonacci"].prog
    for k in (1, 3):
        chs = [challenger(ch_consts) for _ in range(k)]
        assert verify_native_bytes_many(prog, pcs, [blob] * k, [[0, 1, 21]] * k, chs) == [None] * k
        for ch in chs[1:]:
            np.testing.assert_array_equal(ch.state(), chs[0].state())
