"""The Keccak-AIR on the device: trace generation (eon_keccak_generate_trace_dev) byte for byte
against the CPU restatement (tests/airs_keccak.py), and its 3182 constraints through the generic
program (AirProgram): check_constraints, quotient_values, eval_at_point, prove_native and
verify_native, against mirror_check, pyoracle.quotient_values_fn and verify_oracle with
keccak_constraints.

A byte-for-byte proof comparison with prove_oracle.prove is not made: the driver is the one already
compared for the other AIRs, and 2633 CPU column commitments and openings do not fit a quick test."""

import ctypes

import numpy as np
import pytest

import mirror_check as MC
from airs_keccak import (AP, NUM_CONSTRAINTS, WIDTH, flip_a_prime_bit, flipped_bit_failures, keccak_constraints,
                         keccak_trace, mont16_table, smallrng_inputs, trace_limbs)
from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V
from oracle.smallrng import SmallRng, poseidon2_new_from_rng

pytestmark = pytest.mark.gpu
P = O.P
SRS_ALPHA = 12345
FLIP_COL = AP + 64 * (5 * 2 + 3) + 17  # a_prime[y=2][x=3][z=17]


def lim(x):
    return np.array(O.int_to_limbs(O.to_mont(x % P)), dtype=np.uint64)


def ints(a):
    return [O.from_mont(O.limbs_to_int([int(v) for v in e])) for e in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def dev_inputs(inputs):
    return dev(np.array(inputs, dtype=np.uint64).reshape(-1, 25))


@pytest.fixture(scope="module")
def air(gpu_ctx):
    from plonky3_eon_amd import KeccakAir

    return KeccakAir(gpu_ctx)


@pytest.fixture(scope="module")
def prog(gpu_ctx, air):
    from plonky3_eon_amd.air import AirProgram

    p = AirProgram(air, gpu_ctx)
    assert (p.width, p.num_constraints, p.max_constraint_degree, p.log_quotient_degree()) == (WIDTH, NUM_CONSTRAINTS, 3, 1)
    return p


@pytest.fixture(scope="module")
def rows1():
    """the 1-hash trace (32 rows): never modified"""
    return keccak_trace(smallrng_inputs(1))


@pytest.mark.parametrize("n_hashes", [1, 2, 5, 11, 43])
def test_trace_bytes(air, n_hashes):
    """32, 64, 128, 512 and 2048 rows; every shape ends in a cut padding permutation"""
    inputs = smallrng_inputs(n_hashes)
    got = air.generate_trace(dev_inputs(inputs))
    want = trace_limbs(keccak_trace(inputs))
    assert tuple(got.shape) == want.shape == (1 << (24 * n_hashes - 1).bit_length(), WIDTH, 4)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), want)


def test_trace_past_4_gib(air):
    """n_hashes = 2730: 65,536 rows, 5.5 GB, rows past 50,975 above the 4-GiB mark, the last
    permutation 16 rows.  Compared on the device; nothing comes back to the host."""
    import torch

    n = 2730
    inputs = dev(np.random.default_rng(3).integers(0, 1 << 64, (n, 25), dtype=np.uint64))
    big = air.generate_trace(inputs)
    assert tuple(big.shape) == (1 << 16, WIDTH, 4) and big.numel() * 8 > 5 << 30
    for k in (0, 2047, 2729):
        one = air.generate_trace(inputs[k:k + 1])
        assert torch.equal(big[24 * k:24 * k + 24], one[:24]), k
    zero = air.generate_trace(torch.zeros((1, 25), dtype=torch.int64, device=inputs.device))
    assert 24 * n == (1 << 16) - 16 and torch.equal(big[24 * n:], zero[:16])
    del big
    torch.cuda.empty_cache()


def test_argument_errors(gpu_ctx, air):
    import torch

    from plonky3_eon_amd import _lib

    ok = dev_inputs(smallrng_inputs(1))
    with pytest.raises(_lib.EonError) as e:
        air.generate_trace(ok[:0])
    assert e.value.code == _lib.EON_E_SHAPE
    lib = gpu_ctx.lib
    assert lib.eon_keccak_air_width() == WIDTH
    assert [lib.eon_keccak_air_rows(n) for n in (0, 1, 2, 43, 2730)] == [0, 32, 64, 2048, 65536]
    out = torch.empty((64, WIDTH, 4), dtype=torch.int64, device="cuda:0")
    for n_rows in (64, 16, 0):  # 1 hash is 32 rows
        rc = lib.eon_keccak_generate_trace_dev(gpu_ctx.handle, ctypes.c_void_p(ok.data_ptr()), 1,
                                               ctypes.c_void_p(out.data_ptr()), n_rows)
        assert rc == _lib.EON_E_SHAPE and len(lib.eon_last_error(gpu_ctx.handle)) > 0
    assert lib.eon_keccak_generate_trace_dev(gpu_ctx.handle, ctypes.c_void_p(ok.data_ptr()), 0,
                                             ctypes.c_void_p(out.data_ptr()), 0) == _lib.EON_E_SHAPE
    for bad in (ok.to(torch.int32), ok.reshape(5, 5), ok.reshape(25), ok[:, :24], ok.cpu(),
                ok.cpu().numpy()):
        with pytest.raises(ValueError):
            air.generate_trace(bad)


def report(rep):
    return dict(failures=rep.failures, row=rep.row, constraint=rep.constraint, value=rep.value,
                failing_constraints=rep.failing_constraints)


def test_check_constraints_honest(air, prog):
    """the 11-hash device trace (512 rows, 22 permutations, the last cut to 8 rows)"""
    trace = air.generate_trace(dev_inputs(smallrng_inputs(11)))
    rep = prog.check_constraints(trace, per_constraint=True)
    assert report(rep) == dict(failures=0, row=0, constraint=0, value=0, failing_constraints=0)
    assert rep.counts == [0] * NUM_CONSTRAINTS


@pytest.mark.parametrize("seed,want", [(1, [1839, 2799, 2960]), (2, [1839, 2799, 2952, 2956, 2960])])
def test_check_constraints_flipped_bit(air, prog, seed, want):
    """a_prime[2][3][17] of row 5 flipped on the device trace: row 5, constraint 1839 (limb 1 of
    a[2][3]) first, with the value and the counts mirror_check computes.  Of the five constraints the
    flip can break, two depend on the row's data (airs_keccak.flipped_bit_failures): the SmallRng(1)
    trace breaks three, the SmallRng(2) trace all five."""
    import torch

    inputs = smallrng_inputs(1, seed)
    rows = keccak_trace(inputs)
    trace = air.generate_trace(dev_inputs(inputs))
    bit = rows[5][FLIP_COL]
    trace[5, FLIP_COL] = torch.from_numpy(mont16_table()[1 - bit].view(np.int64)).to(trace.device)
    bad = flip_a_prime_bit(rows)
    fails = MC.check_constraints(MC.main_fn(keccak_constraints), bad)
    assert [(r, k) for r, k, _ in fails] == [(5, k) for k in want] == [(5, k) for k in flipped_bit_failures(rows)]
    exp = MC.summary(fails, NUM_CONSTRAINTS)
    rep = prog.check_constraints(trace, per_constraint=True)
    assert (rep.row, rep.constraint, rep.failing_constraints) == (5, 1839, len(want))
    assert report(rep) == {k: v for k, v in exp.items() if k != "counts"} and rep.counts == exp["counts"]


def test_quotient_values(gpu_ctx, prog):
    """log_n = 5, log_qd = 1 on a random LDE: all 64 outputs against pyoracle.quotient_values_fn"""
    lde = C.random_fr(31, 64 * WIDTH).reshape(64, WIDTH, 4)
    alpha = 0x1234567890ABCDEF1122334455667788
    vals = ints(lde)
    lde_rows = [vals[i * WIDTH:(i + 1) * WIDTH] for i in range(64)]
    want = O.quotient_values_fn(lde_rows, 5, 1, keccak_constraints, alpha)
    got = prog.quotient_values(dev(lde), 5, 1, alpha)
    assert ints(got.cpu().numpy().view(np.uint64)) == want


def test_eval_at_point(prog):
    """the verifier's evaluation at an out-of-domain point on random opened rows"""
    rows = C.random_fr(32, 2 * WIDTH).reshape(2, WIDTH, 4)
    loc, nxt = ints(rows[0]), ints(rows[1])
    zeta, alpha, log_n = 0x5555666677778888, 0x1111222233334444, 5
    sels = V.selectors_at_point(log_n, zeta)
    folded = V.fold_constraints(keccak_constraints(loc, nxt, sels[:3], ()), alpha)
    assert prog.eval_at_point(log_n, zeta, alpha, dev(rows[0]), dev(rows[1])) == (folded, folded * sels[3] % P)


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

    p = NativeKzgPcs(64, SRS_ALPHA, gpu_ctx)
    yield p
    p.close()


@pytest.fixture(scope="module")
def honest_proof(air, prog, pcs, ch_consts):
    """1 hash, 32 rows, Fiat-Shamir: proved once, never modified"""
    from plonky3_eon_amd.native import prove_native

    trace = air.generate_trace(dev_inputs(smallrng_inputs(1)))
    return prove_native(prog, pcs, trace, None, None, challenger=challenger(ch_consts))


def test_prove_and_verify(prog, pcs, ch_consts, honest_proof):
    from plonky3_eon_amd.native import verify_native

    assert honest_proof.degree_bits == 5 and len(honest_proof.quotient_commit) == 2
    used = {}
    assert verify_native(prog, pcs, honest_proof, (), challenger=challenger(ch_consts), transcript=used) is None
    assert (used["alpha"], used["zeta"]) == (honest_proof.alpha, honest_proof.zeta)


def test_prove_flipped_bit(prog, pcs, ch_consts, rows1):
    """the bit-flipped trace: with check_constraints off a proof comes back and the verifier reports
    OodEvaluationMismatch; with it on the prove stops at row 5, constraint 1839"""
    from plonky3_eon_amd.native import ConstraintError, VerificationError, prove_native, verify_native

    trace = dev(trace_limbs(flip_a_prime_bit(rows1)))
    assert pcs.check_constraints is False
    proof = prove_native(prog, pcs, trace, None, None, challenger=challenger(ch_consts))
    with pytest.raises(VerificationError) as e:
        verify_native(prog, pcs, proof, (), challenger=challenger(ch_consts))
    assert e.value.kind == "OodEvaluationMismatch"
    pcs.check_constraints = True
    try:
        with pytest.raises(ConstraintError) as ce:
            prove_native(prog, pcs, trace, None, None, challenger=challenger(ch_consts))
    finally:
        pcs.check_constraints = False
    assert (ce.value.report.row, ce.value.report.constraint) == (5, 1839)
    assert str(ce.value).startswith(f"Constraint failed at row 5: constraint 1839 of {NUM_CONSTRAINTS}, ")


def test_oracle_verifies_the_proof(ch_consts, honest_proof):
    """verify_oracle.verify_kzg_proof (the CPU restatement of the reference's verifier) accepts the
    device's proof: transcript, the out-of-domain identity with keccak_constraints, and the 5268 KZG
    openings in one CPU MSM.  0.27 s on the GPU machine's host (pytest's call duration), so not
    marked slow."""
    fn = lambda loc, nxt, sels: keccak_constraints(loc, nxt, sels[:3], ())  # noqa: E731
    res = V.verify_kzg_proof(honest_proof, fn, 5, 1, SRS_ALPHA, challenger=O.DuplexChallenger(ch_consts[0]))
    assert res == {"transcript": True, "ood": True, "kzg": True}, res
