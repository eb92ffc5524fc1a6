"""The Blake3-AIR on the device: trace generation (eon_blake3_generate_trace_dev) byte for byte
against the CPU restatement (tests/airs_blake3.py), and its 9760 constraints through the generic
program (AirProgram): check_constraints, quotient_values, eval_at_point, prove_native and
verify_native, against mirror_check, pyoracle.quotient_values_fn and verify_oracle with
blake3_constraints.

A byte-for-byte proof comparison with prove_oracle.prove is not made: the driver is the one already
compared for the other AIRs, and 9168 CPU column commitments and openings do not fit a quick test."""

import ctypes

import numpy as np
import pytest

import mirror_check as MC
from airs_blake3 import (BUMP_COL, BUMP_FAILS, BUMP_ROW, FLIP_COL, FLIP_FAILS, FLIP_ROW, NUM_CONSTRAINTS, WIDTH,
                         blake3_constraints, blake3_trace, mont16_table, smallrng_inputs, tamper, trace_limbs)
from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V
from oracle.smallrng import SmallRng, poseidon2_new_from_rng

pytestmark = pytest.mark.gpu
P = O.P
SRS_ALPHA = 12345


def lim(x):
    return np.array(O.int_to_limbs(O.to_mont(x % P)), dtype=np.uint64)


def ints(a):
    return [O.from_mont(O.limbs_to_int([int(v) for v in e])) for e in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def dev_inputs(inputs):
    import torch

    return torch.from_numpy(np.array(inputs, dtype=np.uint32).reshape(-1, 24).view(np.int32)).to("cuda:0")


@pytest.fixture(scope="module")
def air(gpu_ctx):
    from plonky3_eon_amd import Blake3Air

    return Blake3Air(gpu_ctx)


@pytest.fixture(scope="module")
def prog(gpu_ctx, air):
    from plonky3_eon_amd.air import AirProgram

    p = AirProgram(air, gpu_ctx)
    assert (p.width, p.num_constraints, p.max_constraint_degree, p.log_quotient_degree()) == (WIDTH, NUM_CONSTRAINTS, 3, 1)
    return p


@pytest.fixture(scope="module")
def cpu_traces():
    """n -> rows of the SmallRng(1) trace, computed once: never modified"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = blake3_trace(smallrng_inputs(n))
        return cache[n]

    return get


@pytest.mark.parametrize("n", [1, 2, 8, 64, 256])
def test_trace_bytes(air, cpu_traces, n):
    """a lone row (block_len 1); counter > 0 with block_len != 1; rows cut into 16, 16, 16, 16 and 8
    slices; 256 rows are more workgroups than one wave of them"""
    got = air.generate_trace(dev_inputs(smallrng_inputs(n)))
    want = trace_limbs(cpu_traces(n))
    assert tuple(got.shape) == want.shape == (n, WIDTH, 4)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("parts", [1, 2, 4, 8, 16])
def test_trace_does_not_depend_on_the_slicing(gpu_ctx, air, parts):
    """eon_diag_blake3_trace_parts: every number of workgroups per row writes the same 8 rows"""
    import torch

    inputs = dev_inputs(smallrng_inputs(8))
    want = air.generate_trace(inputs)
    got = torch.full_like(want, -1)
    gpu_ctx.check(gpu_ctx.lib.eon_diag_blake3_trace_parts(gpu_ctx.handle, ctypes.c_void_p(inputs.data_ptr()), 8,
                                                          ctypes.c_void_p(got.data_ptr()), 8, parts))
    assert torch.equal(got, want)


def test_trace_past_4_gib(air, prog):
    """2^14 rows, 4.8 GB, rows from 14,640 up above the 4-GiB mark (one workgroup per row).  Checked
    on the device, nothing comes back to the host: columns 0..895 (inputs, chaining values, counter,
    block_len, flags) against the bits computed with torch integer ops, and every constraint on every
    row -- the constraints determine the other columns from those."""
    import torch

    n = 1 << 14
    raw = np.random.default_rng(3).integers(0, 1 << 32, (n, 24), dtype=np.uint32)
    inputs = torch.from_numpy(raw.view(np.int32)).to("cuda:0")
    big = air.generate_trace(inputs)
    assert tuple(big.shape) == (n, WIDTH, 4) and big.numel() * 8 > 4 << 30 and 14640 * WIDTH * 32 > 1 << 32
    k = torch.arange(n, dtype=torch.int64, device=inputs.device)
    zero = torch.zeros_like(k)
    words = torch.cat([inputs.to(torch.int64) & 0xFFFFFFFF, torch.stack([k, zero, zero + n, zero], dim=1)], dim=1)
    bits = (words[:, :, None] >> torch.arange(32, device=inputs.device)) & 1  # (n, 28, 32)
    one = torch.from_numpy(mont16_table()[1].view(np.int64)).to(inputs.device)
    assert torch.equal(big[:, :896], bits.reshape(n, 896, 1) * one)
    del bits, words
    rep = prog.check_constraints(big)
    assert (rep.failures, rep.failing_constraints) == (0, 0)
    del big
    torch.cuda.empty_cache()


def test_argument_errors(gpu_ctx, air):
    import torch

    from plonky3_eon_amd import _lib

    ok = dev_inputs(smallrng_inputs(4))
    for bad_n in (0, 3):
        with pytest.raises(_lib.EonError) as e:
            air.generate_trace(ok[:bad_n])
        assert e.value.code == _lib.EON_E_SHAPE
    lib = gpu_ctx.lib
    assert lib.eon_blake3_air_width() == WIDTH
    out = torch.empty((8, WIDTH, 4), dtype=torch.int64, device="cuda:0")

    def call(n_hashes, n_rows, inp=ok.data_ptr(), trace=out.data_ptr(), h=gpu_ctx.handle):
        return lib.eon_blake3_generate_trace_dev(h, ctypes.c_void_p(inp), n_hashes, ctypes.c_void_p(trace), n_rows)

    # n_hashes 0, no power of two, n_rows != n_hashes, more than 2^28 rows
    for n_hashes, n_rows in ((0, 0), (3, 3), (4, 8), (4, 2), (1 << 29, 1 << 29)):
        assert call(n_hashes, n_rows) == _lib.EON_E_SHAPE and len(lib.eon_last_error(gpu_ctx.handle)) > 0
    assert call(4, 4, inp=None) == _lib.EON_E_ARG and call(4, 4, trace=None) == _lib.EON_E_ARG
    assert call(4, 4, h=None) == _lib.EON_E_ARG
    for parts in (3, 32):
        assert lib.eon_diag_blake3_trace_parts(gpu_ctx.handle, ctypes.c_void_p(ok.data_ptr()), 4,
                                               ctypes.c_void_p(out.data_ptr()), 4, parts) == _lib.EON_E_SHAPE
    for bad in (ok.to(torch.int64), ok.reshape(4, 4, 6), ok.reshape(96), ok[:, :23], ok.cpu(), ok.cpu().numpy()):
        with pytest.raises(ValueError):
            air.generate_trace(bad)


def report(rep):
    return dict(failures=rep.failures, row=rep.row, constraint=rep.constraint, value=rep.value,
                failing_constraints=rep.failing_constraints)


def test_check_constraints_honest(air, prog):
    trace = air.generate_trace(dev_inputs(smallrng_inputs(64)))
    rep = prog.check_constraints(trace, per_constraint=True)
    assert report(rep) == dict(failures=0, row=0, constraint=0, value=0, failing_constraints=0)
    assert rep.counts == [0] * NUM_CONSTRAINTS


@pytest.mark.parametrize("row,col,delta,want", [(FLIP_ROW, FLIP_COL, None, FLIP_FAILS), (BUMP_ROW, BUMP_COL, 1, BUMP_FAILS)])
def test_check_constraints_tampered(air, prog, cpu_traces, row, col, delta, want):
    """the two tampered cells of the n = 4 trace (a flipped bit of full_rounds[3].state_middle.row1[2],
    a low limb of full_rounds[0].state_prime.row0[1] plus 1): the row, the first constraint, the value
    and the counts mirror_check computes"""
    import torch

    rows = cpu_traces(4)
    if delta is None:
        delta = 1 - 2 * rows[row][col]
    trace = air.generate_trace(dev_inputs(smallrng_inputs(4)))
    trace[row, col] = torch.from_numpy(mont16_table()[rows[row][col] + delta].view(np.int64)).to(trace.device)
    fails = MC.check_constraints(MC.main_fn(blake3_constraints), tamper(rows, row, col, delta))
    assert [(r, k) for r, k, _ in fails] == [(row, k) for k in want]
    exp = MC.summary(fails, NUM_CONSTRAINTS)
    rep = prog.check_constraints(trace, per_constraint=True)
    assert (rep.row, rep.constraint, rep.failing_constraints) == (row, want[0], len(want))
    assert report(rep) == {k: v for k, v in exp.items() if k != "counts"} and rep.counts == exp["counts"]


def test_quotient_values(gpu_ctx, prog):
    """log_n = 3, log_qd = 1 on a random LDE: all 16 outputs against pyoracle.quotient_values_fn"""
    lde = C.random_fr(31, 16 * WIDTH).reshape(16, WIDTH, 4)
    alpha = 0x1234567890ABCDEF1122334455667788
    vals = ints(lde)
    lde_rows = [vals[i * WIDTH:(i + 1) * WIDTH] for i in range(16)]
    want = O.quotient_values_fn(lde_rows, 3, 1, blake3_constraints, alpha)
    got = prog.quotient_values(dev(lde), 3, 1, alpha)
    assert ints(got.cpu().numpy().view(np.uint64)) == want


def test_eval_at_point(prog):
    """the verifier's evaluation at an out-of-domain point on random opened rows"""
    rows = C.random_fr(32, 2 * WIDTH).reshape(2, WIDTH, 4)
    loc, nxt = ints(rows[0]), ints(rows[1])
    zeta, alpha, log_n = 0x5555666677778888, 0x1111222233334444, 3
    sels = V.selectors_at_point(log_n, zeta)
    folded = V.fold_constraints(blake3_constraints(loc, nxt, sels[:3], ()), alpha)
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

    p = NativeKzgPcs(16, SRS_ALPHA, gpu_ctx)
    yield p
    p.close()


@pytest.fixture(scope="module")
def honest_proof(air, prog, pcs, ch_consts):
    """8 rows, Fiat-Shamir: proved once, never modified"""
    from plonky3_eon_amd.native import prove_native

    trace = air.generate_trace(dev_inputs(smallrng_inputs(8)))
    return prove_native(prog, pcs, trace, None, None, challenger=challenger(ch_consts))


def test_prove_and_verify(prog, pcs, ch_consts, honest_proof):
    from plonky3_eon_amd.native import verify_native

    assert honest_proof.degree_bits == 3 and len(honest_proof.quotient_commit) == 2
    used = {}
    assert verify_native(prog, pcs, honest_proof, (), challenger=challenger(ch_consts), transcript=used) is None
    assert (used["alpha"], used["zeta"]) == (honest_proof.alpha, honest_proof.zeta)


def test_prove_flipped_bit(prog, pcs, ch_consts, cpu_traces):
    """the n = 8 trace with the bit of column 4525 flipped on row 2: with check_constraints off a proof
    comes back and the verifier reports OodEvaluationMismatch; with it on the prove stops at row 2,
    constraint 4798"""
    from plonky3_eon_amd.native import ConstraintError, VerificationError, prove_native, verify_native

    rows = cpu_traces(8)
    trace = dev(trace_limbs(tamper(rows, FLIP_ROW, FLIP_COL, 1 - 2 * rows[FLIP_ROW][FLIP_COL])))
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
    assert (ce.value.report.row, ce.value.report.constraint) == (2, 4798)
    assert str(ce.value).startswith(f"Constraint failed at row 2: constraint 4798 of {NUM_CONSTRAINTS}, ")


def test_oracle_verifies_the_proof(ch_consts, honest_proof):
    """verify_oracle.verify_kzg_proof (the CPU restatement of the reference's verifier) accepts the
    device's proof: transcript, the out-of-domain identity with blake3_constraints, and the KZG
    openings in one CPU MSM"""
    fn = lambda loc, nxt, sels: blake3_constraints(loc, nxt, sels[:3], ())  # noqa: E731
    res = V.verify_kzg_proof(honest_proof, fn, 3, 1, SRS_ALPHA, challenger=O.DuplexChallenger(ch_consts[0]))
    assert res == {"transcript": True, "ood": True, "kzg": True}, res
