"""Proof bytes on the GPU: Proof.to_bytes / from_bytes / save / load and native.verify_native_bytes
(eon_proof_serialize / eon_proof_deserialize, include/eon_prove.h).

Seven AIRs, each proved with Fiat-Shamir under the per-column and the batched opening, heights 2^3
and 2^4, an SRS of 2^8 powers of alpha = 12345: Fibonacci (publics), MulAir (two chunks), the
preprocessed AIR, the multiset lookup AIR, the range-check AIR (preprocessed AND lookup), the fused
Poseidon2-AIR at VECTOR_LEN 2, and a three-column AIR whose constraints read column 0 only, with
column 1 constant 7 and column 2 all zero -- an identity witness and an identity commitment.

Every proof is made once per module and never modified; every comparison is of bytes or integers.
tests/mirror_proofio.py is the independent writer and parser."""

import numpy as np
import pytest

import mirror_lookup as ML
import mirror_proofio as M
from airs import FibonacciAir, MulAir
from airs_lookup import (LookupMultisetEqAir, RangeCheckAir, multiset_trace, range_check_preprocessed,
                         range_check_trace)
from airs_preprocessed import MixedPreAir, mixed_pre_preprocessed, mixed_pre_trace
from oracle import coracle as C
from oracle import pyoracle as O
from oracle.smallrng import SmallRng, poseidon2_new_from_rng
from test_gpu_air_program import mul_trace

pytestmark = pytest.mark.gpu
SRS_ALPHA = 12345
ints, lim, to_limbs = ML.ints, ML.lim, ML.to_limbs
NAMES = ("fibonacci", "mul", "mixed_pre", "multiset", "range_check", "poseidon2_vl2", "identity")
OPENINGS = ("per_column", "batched")
SHAPE, OPENING, OOD = "InvalidProofShape", "InvalidOpeningArgument", "OodEvaluationMismatch"


class CountAir:
    """Three columns; the constraints read column 0 only: 0 on the first row, +1 per row."""

    def width(self):
        return 3

    def num_public_values(self):
        return 0

    def eval(self, builder):
        m = builder.main()
        loc, nxt = m[0], m[1]
        builder.when_first_row().assert_zero(loc[0])
        builder.when_transition().assert_eq(loc[0] + 1, nxt[0])


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


@pytest.fixture(scope="module")
def ch_consts():
    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    return [[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]]


def challenger(ch_consts):
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants

    return Challenger(Poseidon2Constants(*ch_consts))


@pytest.fixture(scope="module")
def pcs(gpu_ctx):
    from plonky3_eon_amd.native import NativeKzgPcs

    p = NativeKzgPcs(255, SRS_ALPHA, gpu_ctx)
    yield p
    p.close()


class Case:
    def __init__(self, prog, trace, prover=None, publics=(), prove_kw=None, vk=None):
        self.prog, self.trace = prog, trace
        self.prover = prover if prover is not None else prog
        self.publics, self.prove_kw, self.vk = list(publics), prove_kw or {}, vk
        self.proof, self.data, self.prover_state = {}, {}, {}


@pytest.fixture(scope="module")
def cases(gpu_ctx, pcs, ch_consts):
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    out = {}
    out["fibonacci"] = Case(AirProgram(FibonacciAir(), gpu_ctx), to_limbs(O.fib_trace(0, 1, 8)), publics=[0, 1, 21])
    out["mul"] = Case(AirProgram(MulAir(), gpu_ctx), to_limbs(mul_trace(8)))
    rows, pub = mixed_pre_trace(3, 4, 5, 16)
    pp = setup_preprocessed(pcs, dev(to_limbs(mixed_pre_preprocessed(16))))
    out["mixed_pre"] = Case(AirProgram(MixedPreAir(), gpu_ctx), to_limbs(rows), publics=pub,
                            prove_kw=dict(preprocessed=pp), vk=pp)
    out["multiset"] = Case(AirProgram(LookupMultisetEqAir(), gpu_ctx), to_limbs(multiset_trace(8)))
    rows, pub_r = range_check_trace(16)
    pre_r = to_limbs(range_check_preprocessed(16))
    pp_r = setup_preprocessed(pcs, dev(pre_r))
    out["range_check"] = Case(AirProgram(RangeCheckAir(), gpu_ctx), to_limbs(rows), publics=pub_r,
                              prove_kw=dict(preprocessed=pp_r, preprocessed_trace=dev(pre_r)), vk=pp_r)
    p2py = O.p2_constants(2024, 4, 56)
    k = C.P2Constants([[lim(v) for v in r] for r in p2py[0]], [lim(v) for v in p2py[1]],
                      [[lim(v) for v in r] for r in p2py[2]])
    air = Poseidon2Air(k.begin, k.partial, k.end, 2, gpu_ctx)
    inputs = C.random_fr(62, 16 * 3).reshape(16, 3, 4)  # 2^3 rows of two permutations
    out["poseidon2_vl2"] = Case(AirProgram(air, gpu_ctx), air.generate_trace(dev(inputs)), prover=air)
    out["identity"] = Case(AirProgram(CountAir(), gpu_ctx), to_limbs([[i, 7, 0] for i in range(8)]))
    for c in out.values():
        trace = c.trace if not isinstance(c.trace, np.ndarray) else dev(c.trace)
        kw = dict(c.prove_kw)
        if c.publics:
            kw["public_values"] = c.publics
        for opening in OPENINGS:
            ch = challenger(ch_consts)
            c.proof[opening] = prove_native(c.prover, pcs, trace, None, None, challenger=ch, opening=opening, **kw)
            c.prover_state[opening] = (ch.state().copy(), ch.sample().copy())
            c.data[opening] = c.proof[opening].to_bytes()
    yield out
    pp.close()
    pp_r.close()


def verdict(case, pcs, proof, ch, prog=None):
    from plonky3_eon_amd.native import VerificationError, verify_native

    try:
        assert verify_native(prog or case.prog, pcs, proof, case.publics, challenger=ch,
                             preprocessed_vk=case.vk) is None
    except VerificationError as e:
        return e.kind
    return None


def verdict_bytes(case, pcs, data, ch, prog=None):
    from plonky3_eon_amd.native import VerificationError, verify_native_bytes

    try:
        assert verify_native_bytes(prog or case.prog, pcs, data, case.publics, challenger=ch,
                                   preprocessed_vk=case.vk) is None
    except VerificationError as e:
        return e.kind
    return None


def widths(case):
    p = case.prog
    return p.width, 1 << p.log_quotient_degree(), case.vk.width if case.vk is not None else 0, p.permutation_width


def expected_size(case, opening):
    w, c, wp, wq = widths(case)
    commits, values = w + wq + c, 2 * w + 2 * wq + 2 * wp + c
    witnesses = 2 * w + 2 * wq + 2 * wp + c if opening == "per_column" else 2 + 2 * (wq > 0) + 2 * (wp > 0) + c
    return 48 + 32 * (commits + values + witnesses), witnesses


# ---- the round trip ---------------------------------------------------------------------------------
@pytest.mark.parametrize("opening", OPENINGS)
@pytest.mark.parametrize("name", NAMES)
def test_round_trip(gpu_ctx, cases, name, opening):
    from plonky3_eon_amd.proof import Proof

    c = cases[name]
    proof, data = c.proof[opening], c.data[opening]
    assert len(data) == expected_size(c, opening)[0]
    assert data == M.write(*M.proof_arrays(proof))  # the independent writer
    back = Proof.from_bytes(data, gpu_ctx)
    assert back.preprocessed_commit is None and back.timings_ms == {}
    assert (back.alpha, back.zeta, back.gamma, back.delta, back.permutation_challenges) == (None,) * 5
    assert (back.opening, back.degree_bits) == (opening, proof.degree_bits)
    assert (back.permutation_commit is None) == (proof.permutation_commit is None)
    assert len(back.opened) == len(proof.opened)
    (s0, a0), (s1, a1), (s2, a2) = M.proof_arrays(proof), M.proof_arrays(back), M.parse(data)
    assert s0 == s1 == s2 and sorted(a0) == sorted(a1) == sorted(a2)
    for k in a0:
        assert a1[k].shape == a0[k].shape == a2[k].shape, k
        np.testing.assert_array_equal(a1[k], a0[k], err_msg=k)
        np.testing.assert_array_equal(a2[k], a0[k], err_msg=k)
    assert back.to_bytes() == data


@pytest.mark.parametrize("opening", OPENINGS)
@pytest.mark.parametrize("name", NAMES)
def test_loaded_proofs_verify_and_the_challengers_end_where_the_provers_did(gpu_ctx, cases, pcs, ch_consts, name,
                                                                            opening):
    from plonky3_eon_amd.proof import Proof

    c = cases[name]
    state, nxt = c.prover_state[opening]
    ch = challenger(ch_consts)
    assert verdict(c, pcs, Proof.from_bytes(c.data[opening], gpu_ctx), ch) is None
    np.testing.assert_array_equal(ch.state(), state)
    np.testing.assert_array_equal(ch.sample(), nxt)
    ch = challenger(ch_consts)
    assert verdict_bytes(c, pcs, c.data[opening], ch) is None
    np.testing.assert_array_equal(ch.state(), state)
    np.testing.assert_array_equal(ch.sample(), nxt)


@pytest.mark.parametrize("name", NAMES)
def test_batched_bytes_are_shorter_by_the_witnesses_saved(cases, name):
    c = cases[name]
    per_column, batched = expected_size(c, "per_column")[1], expected_size(c, "batched")[1]
    assert M.witness_count(M.peek(c.data["per_column"])) == per_column
    assert M.witness_count(M.peek(c.data["batched"])) == batched
    assert len(c.data["per_column"]) - len(c.data["batched"]) == 32 * (per_column - batched)


def test_the_identity_case_holds_identity_points(cases):
    c = cases["identity"]
    s, a = M.parse(c.data["per_column"])
    inf = bytes(31) + b"\x40"
    data = c.data["per_column"]
    at = M.offset_of(s, "TRACE_COMMIT", 2)
    assert data[at:at + 32] == inf and not a["trace_commit"][2].any() and a["trace_commit"][1].any()
    for section in ("TRACE_WITNESS_ZETA", "TRACE_WITNESS_NEXT"):
        for col in (1, 2):  # a constant column's quotient is zero
            at = M.offset_of(s, section, col)
            assert data[at:at + 32] == inf
        at = M.offset_of(s, section, 0)
        assert data[at:at + 32] != inf
    at = M.offset_of(M.peek(c.data["batched"]), "TRACE_COMMIT", 2)
    assert c.data["batched"][at:at + 32] == inf


def test_fibonacci_bytes_are_the_golden_file(cases):
    from pathlib import Path

    golden = Path(__file__).resolve().parent / "golden" / "proof_fib8_fs.bin"
    assert cases["fibonacci"].data["per_column"] == golden.read_bytes()


def test_save_load_and_a_verifier_only_pcs(gpu_ctx, cases, ch_consts, tmp_path):
    """a proof written by one side and verified by a side that holds no G1 table"""
    from plonky3_eon_amd.native import NativeKzgPcs, verify_native
    from plonky3_eon_amd.proof import Proof
    from plonky3_eon_amd.verify import g2_mul

    c = cases["mul"]
    verifier = NativeKzgPcs.verifier(255, g2_mul(SRS_ALPHA, ctx=gpu_ctx), gpu_ctx)
    try:
        for opening in OPENINGS:
            path = tmp_path / f"{opening}.proof"
            c.proof[opening].save(path)
            assert path.read_bytes() == c.data[opening]
            ch = challenger(ch_consts)
            assert verify_native(c.prog, verifier, Proof.load(path, gpu_ctx), challenger=ch) is None
            np.testing.assert_array_equal(ch.state(), c.prover_state[opening][0])
    finally:
        verifier.close()


def test_bytes_without_a_challenger_are_refused(cases, pcs):
    from plonky3_eon_amd.native import verify_native_bytes

    with pytest.raises(ValueError):
        verify_native_bytes(cases["fibonacci"].prog, pcs, cases["fibonacci"].data["per_column"], [0, 1, 21])


# ---- bytes that do not deserialise ----------------------------------------------------------------------
def put(data, shape, section, index, b32):
    at = M.offset_of(shape, section, index)
    return data[:at] + b32 + data[at + 32:]


def rejection(gpu_ctx, data):
    from plonky3_eon_amd.proof import Proof, ProofFormatError, VerificationError

    with pytest.raises(ProofFormatError) as e:
        Proof.from_bytes(data, gpu_ctx)
    assert not isinstance(e.value, VerificationError)
    with pytest.raises(M.Rejected) as m:  # the mirror says the same
        M.parse(data)
    assert (m.value.reason, m.value.section, m.value.index) == (e.value.reason, e.value.section, e.value.index)
    return e.value.reason, e.value.section, e.value.index


@pytest.mark.parametrize("opening", OPENINGS)
def test_format_rejections(gpu_ctx, cases, pcs, ch_consts, opening):
    from plonky3_eon_amd.native import verify_native_bytes
    from plonky3_eon_amd.proof import ProofFormatError

    c = cases["mul"]
    data = c.data[opening]
    s = M.peek(data)
    r_bytes, q_bytes = M.R.to_bytes(32, "little"), M.Q.to_bytes(32, "little")
    x = 1
    while pow(x**3 + 3, (M.Q - 1) // 2, M.Q) != M.Q - 1:  # the smallest x >= 1 whose x^3 + 3 is no square
        x += 1
    off_curve = x.to_bytes(32, "little")
    last_w = M.counts(s)["TRACE_WITNESS_NEXT"] - 1
    flag = bytearray(data[M.offset_of(s, "QUOTIENT_COMMIT", 1):][:32])
    flag[31] = 0x41

    bad_value = put(data, s, "TRACE_NEXT", 59, r_bytes)
    assert rejection(gpu_ctx, bad_value) == ("FR_NOT_CANONICAL", "TRACE_NEXT", 59)
    assert rejection(gpu_ctx, put(data, s, "QUOTIENT_OPENED", 1, bytes([255] * 32))) == \
        ("FR_NOT_CANONICAL", "QUOTIENT_OPENED", 1)
    bad_witness = put(data, s, "TRACE_WITNESS_NEXT", last_w, q_bytes)
    assert rejection(gpu_ctx, bad_witness) == ("G1_NOT_CANONICAL", "TRACE_WITNESS_NEXT", last_w)
    bad_commit = put(data, s, "TRACE_COMMIT", 17, off_curve)
    assert rejection(gpu_ctx, bad_commit) == ("G1_NOT_ON_CURVE", "TRACE_COMMIT", 17)
    assert rejection(gpu_ctx, put(data, s, "QUOTIENT_COMMIT", 1, bytes(flag))) == ("G1_ENCODING", "QUOTIENT_COMMIT", 1)
    # several bad elements: the lowest byte offset is the one reported, whatever its kind
    two_points = put(put(data, s, "QUOTIENT_WITNESS", 1, off_curve), s, "QUOTIENT_WITNESS", 0, q_bytes)
    assert rejection(gpu_ctx, two_points) == ("G1_NOT_CANONICAL", "QUOTIENT_WITNESS", 0)
    assert rejection(gpu_ctx, put(bad_witness, s, "TRACE_COMMIT", 59, bytes(flag))) == \
        ("G1_ENCODING", "TRACE_COMMIT", 59)
    assert rejection(gpu_ctx, put(bad_witness, s, "TRACE_NEXT", 59, r_bytes)) == ("FR_NOT_CANONICAL", "TRACE_NEXT", 59)
    assert rejection(gpu_ctx, put(bad_value, s, "QUOTIENT_COMMIT", 0, off_curve)) == \
        ("G1_NOT_ON_CURVE", "QUOTIENT_COMMIT", 0)
    assert rejection(gpu_ctx, put(bad_value, s, "TRACE_LOCAL", 0, r_bytes)) == ("FR_NOT_CANONICAL", "TRACE_LOCAL", 0)
    # the frame
    for bad in (data[:-1], data[:48], data[:47], data + b"\0"):
        assert rejection(gpu_ctx, bad) == ("LENGTH", "HEADER", 0)
    assert rejection(gpu_ctx, data[:8] + (2).to_bytes(4, "little") + data[12:]) == ("VERSION", "HEADER", 0)
    assert rejection(gpu_ctx, b"EONSRS1\0" + data[8:]) == ("MAGIC", "HEADER", 0)
    # verify_native_bytes fails the same way, before any verification: the challenger is untouched
    ch = challenger(ch_consts)
    before = ch.state().copy()
    with pytest.raises(ProofFormatError) as e:
        verify_native_bytes(c.prog, pcs, bad_commit, challenger=ch)
    assert (e.value.reason, e.value.section, e.value.index) == ("G1_NOT_ON_CURVE", "TRACE_COMMIT", 17)
    np.testing.assert_array_equal(ch.state(), before)


# ---- well-formed but wrong ------------------------------------------------------------------------------
def neg_point(row):
    row = np.array(row, dtype=np.uint64).copy()
    row[4:] = M.limbs(M.Q - M.unlimbs(row[4:]))
    return row


@pytest.mark.parametrize("opening", OPENINGS)
def test_a_negated_witness_loads_and_fails_as_in_the_arrays(gpu_ctx, cases, pcs, ch_consts, opening):
    import copy

    from plonky3_eon_amd.proof import Proof

    c = cases["mul"]
    data, s = c.data[opening], M.peek(c.data[opening])
    at = M.offset_of(s, "TRACE_WITNESS_ZETA", 0) + 31
    assert data[at] & 0x40 == 0
    flipped = data[:at] + bytes([data[at] ^ 0x80]) + data[at + 1:]
    direct = copy.deepcopy(c.proof[opening])
    w = np.array(direct.opened[0].witnesses[0][0], dtype=np.uint64).copy()
    w[0] = neg_point(w[0])
    direct.opened[0].witnesses[0][0] = w
    loaded = Proof.from_bytes(flipped, gpu_ctx)
    np.testing.assert_array_equal(np.asarray(loaded.opened[0].witnesses[0][0]), w)
    want = verdict(c, pcs, direct, challenger(ch_consts))
    assert want == OPENING
    assert verdict(c, pcs, loaded, challenger(ch_consts)) == want
    assert verdict_bytes(c, pcs, flipped, challenger(ch_consts)) == want


@pytest.mark.parametrize("opening", OPENINGS)
def test_a_changed_opened_value_loads_and_fails_as_in_the_arrays(gpu_ctx, cases, pcs, ch_consts, opening):
    import copy

    c = cases["mul"]
    data, s = c.data[opening], M.peek(c.data[opening])
    other = np.array(lim(0x123456789), dtype=np.uint64)
    changed = put(data, s, "TRACE_LOCAL", 5, other.astype("<u8").tobytes())
    direct = copy.deepcopy(c.proof[opening])
    v = np.array(direct.opened[0].values[0][0], dtype=np.uint64).copy()
    assert not np.array_equal(v[5], other)
    v[5] = other
    direct.opened[0].values[0][0] = v
    want = verdict(c, pcs, direct, challenger(ch_consts))
    assert want in (OPENING, OOD)
    assert verdict_bytes(c, pcs, changed, challenger(ch_consts)) == want


@pytest.mark.parametrize("opening", OPENINGS)
def test_bytes_of_another_air_are_an_invalid_proof_shape(cases, pcs, ch_consts, opening):
    from plonky3_eon_amd.native import VerificationError, verify_native_bytes

    fib, mul = cases["fibonacci"], cases["mul"]
    with pytest.raises(VerificationError) as e:
        verify_native_bytes(mul.prog, pcs, fib.data[opening], challenger=challenger(ch_consts))
    assert e.value.kind == SHAPE
