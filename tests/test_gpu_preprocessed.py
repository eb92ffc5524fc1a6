"""Preprocessed columns on the GPU: EON_SYM_PREPROCESSED leaves in k_air_quotient
(eon_air_program_create_pp / eon_quotient_values_pp_dev) against the oracle's quotient_values_fn, and
setup_preprocessed / prove with preprocessed data through the native driver (eon_setup_preprocessed,
eon_prove_air_pp[_fs]) against the CPU restatement of the reference's Some(preprocessed) branch
(tests/mirror_preprocessed.py; uni-stark/tests/mul_fib_pair.rs is the specification of MulFibPAir
and its tamper test)."""

import ctypes
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mirror_preprocessed as M
from airs import FibonacciAir
from airs_preprocessed import (MixedPreAir, MulFibPAir, PreMockAir, mixed_pre_constraints, mixed_pre_preprocessed,
                               mixed_pre_trace, mul_fib_p_constraints, mul_fib_p_preprocessed, mul_fib_p_trace)
from oracle import coracle as C
from oracle import pyoracle as O
from oracle.smallrng import SmallRng, poseidon2_new_from_rng

pytestmark = pytest.mark.gpu
P = O.P
ROOT = Path(__file__).resolve().parent.parent
SRS_ALPHA = 12345
ints, lim = M.ints, M.lim


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def quotient_both(prog, fn, lde, pre, log_n, log_qd, alpha, pub):
    """(device result, oracle result) as canonical ints"""
    got = prog.quotient_values(dev(lde), log_n, log_qd, alpha, pub, preprocessed_lde=dev(pre))
    got = ints(got.cpu().numpy().view(np.uint64))
    rows = [ints(r) + ints(p) for r, p in zip(lde, pre)]
    want = O.quotient_values_fn(rows, log_n, log_qd, M.split_fn(fn, prog.width), alpha, pub)
    return got, want


# ---- 1. quotient against quotient_values_fn, bit-exact ------------------------------------------
@pytest.mark.parametrize("air_cls,fn,log_n,log_qd", [
    (MulFibPAir, mul_fib_p_constraints, 0, 1), (MulFibPAir, mul_fib_p_constraints, 3, 1),
    (MulFibPAir, mul_fib_p_constraints, 8, 1),  # 512 quotient rows: the next row wraps across blocks
    (MixedPreAir, mixed_pre_constraints, 3, 2), (MixedPreAir, mixed_pre_constraints, 5, 2)])
def test_quotient_values_vs_oracle(gpu_ctx, air_cls, fn, log_n, log_qd):
    from plonky3_eon_amd.air import AirProgram

    prog = AirProgram(air_cls(), gpu_ctx)
    assert prog.preprocessed_width == air_cls().preprocessed_width()
    assert prog.log_quotient_degree() == log_qd
    q = 1 << (log_n + log_qd)
    lde = C.random_fr(log_n * 7 + log_qd, q * prog.width).reshape(q, prog.width, 4)
    pre = C.random_fr(1000 + log_n, q * prog.preprocessed_width).reshape(q, prog.preprocessed_width, 4)
    pub = [int(x) for x in ints(C.random_fr(99 + log_n, prog.n_public))]
    got, want = quotient_both(prog, fn, lde, pre, log_n, log_qd, 0x1234567890ABCDEF1234567, pub)
    assert got == want


# ---- 2. addressing edges --------------------------------------------------------------------------
@pytest.mark.parametrize("width,pre_width,specs", [
    (3, 2, [("pre", 0, 0)]),
    (3, 2, [("main", 0, 2), ("pre", 0, 0)]),
    (3, 2, [("pre", 1, 1), ("main", 1, 0), ("pre", 0, 1)]),
    (3, 2, [("pre", 0, 0), ("pre", 0, 1), ("pre", 1, 0), ("pre", 1, 1)]),
    (1, 3, [("pre", 0, 2), ("main", 1, 0), ("pre", 1, 0), ("pre", 0, 1), ("pre", 1, 2)])])  # a swapped stride
def test_addressing_edges(gpu_ctx, width, pre_width, specs):
    """Every matrix, offset and boundary column as a bare-leaf constraint, one to five of them;
    the two matrices are filled from different seeds, so a read from the wrong matrix or with the
    wrong stride cannot match."""
    from plonky3_eon_amd.air import AirProgram

    air = PreMockAir(specs, width, pre_width)
    prog = AirProgram(air, gpu_ctx)
    assert prog.num_constraints == len(specs) and prog.preprocessed_width == pre_width
    log_n, log_qd = 3, 1
    q = 1 << (log_n + log_qd)
    lde = C.random_fr(40 + len(specs), q * width).reshape(q, width, 4)
    pre = C.random_fr(7040 + len(specs), q * pre_width).reshape(q, pre_width, 4)
    got, want = quotient_both(prog, air.constraints, lde, pre, log_n, log_qd, 0x2F1E0D0C0B0A09080706050403020100, [])
    assert got == want


# ---- 3. extreme operands --------------------------------------------------------------------------
PM1 = np.array(O.int_to_limbs(P - 1), dtype=np.uint64)


def extreme_lde(kind, rows, width, seed):
    out = np.zeros((rows, width, 4), dtype=np.uint64)
    if kind == "pm1":
        out[:] = PM1
    elif kind == "alt":
        out[(np.add.outer(np.arange(rows), np.arange(width)) % 2) == 0] = PM1
    elif kind == "alt_rows":
        out[::2] = PM1
    else:
        out[:] = C.random_fr(seed, rows * width).reshape(rows, width, 4)
        out[np.random.default_rng(seed).random((rows, width)) < 0.25] = PM1
    return out


@pytest.mark.parametrize("kind", ["pm1", "alt", "alt_rows", "rand_pm1"])
def test_quotient_extreme_mixed_pre(gpu_ctx, kind):
    """The bound tracking treats a preprocessed cell as a trace cell (raw leaves of bound 32): both
    matrices, the public value and alpha stored as p - 1 (or p - 1 next to 0)."""
    from plonky3_eon_amd.air import AirProgram

    prog = AirProgram(MixedPreAir(), gpu_ctx)
    for log_n, log_qd in ((3, 2), (2, 2)):
        q = 1 << (log_n + log_qd)
        lde = extreme_lde(kind, q, 3, 5 + log_n)
        pre = extreme_lde(kind, q, 3, 50 + log_n)
        pm1 = O.from_mont(P - 1)  # the canonical int whose stored residue is p - 1
        got, want = quotient_both(prog, mixed_pre_constraints, lde, pre, log_n, log_qd, pm1, [pm1])
        assert got == want, (kind, log_n)


# ---- 4. register-file modes -----------------------------------------------------------------------
def test_register_file_modes(gpu_ctx):
    """LDS and global register files (EON_AIR_REGS, read once per process: child processes) give
    the same values for a program with preprocessed leaves."""
    code = ("import numpy as np, torch, sys; sys.path[:0] = [sys.argv[2] + '/tests', sys.argv[2]];"
            "from airs_preprocessed import MixedPreAir; from plonky3_eon_amd import Context;"
            "from plonky3_eon_amd.air import AirProgram; from oracle import coracle as C;"
            "ctx = Context(0); prog = AirProgram(MixedPreAir(), ctx);"
            "t = lambda s: torch.from_numpy(C.random_fr(s, 32 * 3).reshape(32, 3, 4).view(np.int64)).to('cuda:0');"
            "out = prog.quotient_values(t(5), 3, 2, 77, [6], preprocessed_lde=t(9));"
            "np.save(sys.argv[1], out.cpu().numpy())")
    with tempfile.TemporaryDirectory() as d:
        outs = []
        for mode in ("lds", "global"):
            f = os.path.join(d, mode + ".npy")
            subprocess.run([sys.executable, "-c", code, f, str(ROOT)], check=True, timeout=300,
                           env=dict(os.environ, EON_AIR_REGS=mode))
            outs.append(np.load(f))
    np.testing.assert_array_equal(outs[0], outs[1])
    assert outs[0].any()


# ---- 5. Wp = 0 equivalence, 6. rejections ---------------------------------------------------------
def raw_create(ctx, nodes, width=2, pre_width=None, npub=0, consts=(0,), roots=(0,)):
    """eon_air_program_create (pre_width None) or eon_air_program_create_pp -> (code, handle)"""
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.field import ints_to_limbs

    arr = (_lib.eon_sym_node * max(1, len(nodes)))(*[_lib.eon_sym_node(*n) for n in nodes])
    ca = np.ascontiguousarray(ints_to_limbs(list(consts)))
    ra = np.ascontiguousarray(np.array(roots, dtype=np.uint32))
    h = ctypes.c_void_p()
    cp, rp = ca.ctypes.data_as(ctypes.c_void_p), ra.ctypes.data_as(ctypes.c_void_p)
    if pre_width is None:
        rc = ctx.lib.eon_air_program_create(ctx.handle, arr, len(nodes), cp, len(consts), rp, len(roots), width, npub,
                                            ctypes.byref(h))
    else:
        rc = ctx.lib.eon_air_program_create_pp(ctx.handle, arr, len(nodes), cp, len(consts), rp, len(roots), width,
                                               pre_width, npub, ctypes.byref(h))
    return rc, h


def last_error(ctx):
    return ctx.lib.eon_last_error(ctx.handle).decode()


def test_no_preprocessed_width_is_the_old_program(gpu_ctx):
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd import symbolic as S

    lib = gpu_ctx.lib
    nodes, consts, roots = S.serialize(S.get_symbolic_constraints(FibonacciAir(), 0, 3))
    progs, stats = [], []
    for pre_width in (None, 0):
        rc, h = raw_create(gpu_ctx, nodes, 2, pre_width, 3, consts or (0,), roots)
        assert rc == 0, last_error(gpu_ctx)
        st = _lib.eon_air_program_stats()
        assert lib.eon_air_program_info(h, ctypes.byref(st)) == 0
        assert lib.eon_air_program_preprocessed_width(h) == 0
        progs.append(h)
        stats.append([int(getattr(st, k)) for k, _ in st._fields_])
    assert stats[0] == stats[1]
    log_n, log_qd = 4, 1
    q = 1 << (log_n + log_qd)
    lde = dev(C.random_fr(11, q * 2).reshape(q, 2, 4))
    import torch

    from plonky3_eon_amd.field import fr_to_abi

    pub = np.ascontiguousarray(C.random_fr(12, 3).reshape(3, 4))
    a = fr_to_abi(0x1234567890ABCDEF1234567)
    outs = [torch.zeros((q, 4), dtype=torch.int64, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    gpu_ctx.set_stream(None)
    pp, lp = pub.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(lde.data_ptr())
    op = [ctypes.c_void_p(o.data_ptr()) for o in outs]
    gpu_ctx.check(lib.eon_quotient_values_dev(gpu_ctx.handle, progs[0], lp, log_n, log_qd, ctypes.byref(a), pp, 3,
                                              op[0]))
    gpu_ctx.check(lib.eon_quotient_values_pp_dev(gpu_ctx.handle, progs[0], lp, None, log_n, log_qd, ctypes.byref(a),
                                                 pp, 3, op[1]))
    gpu_ctx.check(lib.eon_quotient_values_pp_dev(gpu_ctx.handle, progs[1], lp, None, log_n, log_qd, ctypes.byref(a),
                                                 pp, 3, op[2]))
    gpu_ctx.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and bool(outs[0].any())
    # a preprocessed matrix for a program without preprocessed columns is refused
    rc = lib.eon_quotient_values_pp_dev(gpu_ctx.handle, progs[1], lp, lp, log_n, log_qd, ctypes.byref(a), pp, 3, op[2])
    assert rc == _lib.EON_E_ARG and "preprocessed" in last_error(gpu_ctx)
    for h in progs:
        lib.eon_air_program_destroy(h)


def test_program_and_quotient_rejections(gpu_ctx):
    import torch

    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.air import AirProgram

    ARG = _lib.EON_E_ARG

    def rejected(nodes, **kw):
        rc, _ = raw_create(gpu_ctx, nodes, **kw)
        return rc == ARG and len(last_error(gpu_ctx)) > 0

    assert rejected([(10, 2, 0)], pre_width=2)  # column >= Wp
    assert "preprocessed" in last_error(gpu_ctx)
    assert rejected([(10, 0, 2)], pre_width=2)  # offset 2
    assert rejected([(11, 0, 0)], pre_width=2)  # permutation (LogUp)
    assert rejected([(12, 0, 0)], pre_width=2)  # challenge
    assert rejected([(10, 0, 0)])  # a preprocessed node through the old create: column out of range
    rc, h = raw_create(gpu_ctx, [(10, 1, 1)], pre_width=2)  # the last column, next row: accepted
    assert rc == 0, last_error(gpu_ctx)
    gpu_ctx.lib.eon_air_program_destroy(h)
    # operand indices are 28 bits over main + preprocessed columns
    rc, _ = raw_create(gpu_ctx, [(1, 0, 0)], width=1 << 27, pre_width=1 << 27)
    assert rc == _lib.EON_E_SHAPE and len(last_error(gpu_ctx)) > 0

    prog = AirProgram(MulFibPAir(), gpu_ctx)
    lde = torch.zeros((16, 2, 4), dtype=torch.int64, device="cuda:0")
    with pytest.raises(_lib.EonError) as e:  # the old quotient call on a Wp > 0 program
        prog.quotient_values(lde, 3, 1, 5)
    assert e.value.code == ARG and "eon_quotient_values_pp_dev" in str(e.value)
    out = torch.zeros((16, 4), dtype=torch.int64, device="cuda:0")
    from plonky3_eon_amd.field import fr_to_abi

    a = fr_to_abi(5)
    rc = gpu_ctx.lib.eon_quotient_values_pp_dev(gpu_ctx.handle, prog.handle, ctypes.c_void_p(lde.data_ptr()), None, 3,
                                                1, ctypes.byref(a), None, 0, ctypes.c_void_p(out.data_ptr()))
    assert rc == ARG and "pre_lde" in last_error(gpu_ctx)  # NULL pre_lde


# ---- 7-10. setup and prove through the native driver ----------------------------------------------
@pytest.fixture(scope="module")
def ch_consts():
    # the challenger permutation of the Fibonacci tests: Perm::new_from_rng(4, 22, SmallRng(1))
    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    return py, ([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]])


@pytest.fixture(scope="module")
def srs():
    return C.g1_srs(1025, C.fr_from_u64(SRS_ALPHA))


@pytest.fixture(scope="module")
def pcs(gpu_ctx):
    from plonky3_eon_amd.native import NativeKzgPcs

    p = NativeKzgPcs(1024, SRS_ALPHA, gpu_ctx)
    yield p
    p.close()


def challenger(ch_consts):
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants

    return Challenger(Poseidon2Constants(*ch_consts[1]))


def assert_proofs_equal(got, want):
    """byte-equal: challenges, every commitment, every opened value and every witness"""
    assert (got.alpha, got.zeta) == (want.alpha, want.zeta)
    np.testing.assert_array_equal(got.trace_commit[0], want.trace_commit[0])
    np.testing.assert_array_equal(got.preprocessed_commit[0], want.preprocessed_commit[0])
    assert len(got.quotient_commit) == len(want.quotient_commit)
    for c in range(len(want.quotient_commit)):
        np.testing.assert_array_equal(got.quotient_commit[c], want.quotient_commit[c])
    assert len(got.opened) == 3
    for r in range(3):
        assert len(got.opened[r].values) == len(want.opened[r].values)
        for m in range(len(want.opened[r].values)):
            assert len(got.opened[r].values[m]) == len(want.opened[r].values[m])
            for p in range(len(want.opened[r].values[m])):
                np.testing.assert_array_equal(got.opened[r].values[m][p], want.opened[r].values[m][p])
                np.testing.assert_array_equal(got.opened[r].witnesses[m][p], want.opened[r].witnesses[m][p])


ALL_TRUE = {"transcript": True, "ood": True, "opened_vs_trace": True, "kzg": True}


@pytest.mark.parametrize("n", [8, 64])
def test_setup_commitment(gpu_ctx, pcs, srs, n):
    from plonky3_eon_amd.native import setup_preprocessed

    pre = C.random_fr(300 + n, n * 3).reshape(n, 3, 4)
    pp = setup_preprocessed(pcs, dev(pre))
    assert (pp.width, pp.degree_bits) == (3, n.bit_length() - 1) and pp.commitment.shape == (3, 8)
    np.testing.assert_array_equal(pp.commitment, C.g1_msm_columns(srs[:n], C.idft_batch(pre)))
    pp.close()


@pytest.mark.parametrize("log_n", [3, 6])
def test_mul_fib_pair_prove_vs_mirror_and_verify(gpu_ctx, pcs, srs, ch_consts, log_n):
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    n = 1 << log_n
    trace = M.to_limbs(mul_fib_p_trace(0, 1, n))
    pre = M.to_limbs(mul_fib_p_preprocessed(n))
    prog = AirProgram(MulFibPAir(), gpu_ctx)
    pp = setup_preprocessed(pcs, dev(pre))
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), preprocessed=pp)
    assert proof.degree_bits == log_n
    mpp = M.setup(pre, srs)
    np.testing.assert_array_equal(pp.commitment, mpp.commitment)
    want = M.prove(trace, mpp, srs, mul_fib_p_constraints, 1, challenger=O.DuplexChallenger(ch_consts[0]))
    assert_proofs_equal(proof, want)
    res = M.verify(proof, mpp.commitment, 2, mul_fib_p_constraints, log_n, 1, SRS_ALPHA,
                   challenger=O.DuplexChallenger(ch_consts[0]), trace=trace, pre=pre)
    assert res == ALL_TRUE, res
    pp.close()


def test_mixed_pre_prove_four_chunks_and_given_challenges(gpu_ctx, pcs, srs, ch_consts):
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    prog = AirProgram(MixedPreAir(), gpu_ctx)
    # Fiat-Shamir, 2^4 rows, four quotient chunks
    n = 16
    rows, pub = mixed_pre_trace(3, 4, 5, n)
    trace, pre = M.to_limbs(rows), M.to_limbs(mixed_pre_preprocessed(n))
    pp = setup_preprocessed(pcs, dev(pre))
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), public_values=pub,
                         preprocessed=pp)
    assert len(proof.quotient_commit) == 4
    mpp = M.setup(pre, srs)
    want = M.prove(trace, mpp, srs, mixed_pre_constraints, 2, pub, challenger=O.DuplexChallenger(ch_consts[0]))
    assert_proofs_equal(proof, want)
    res = M.verify(proof, mpp.commitment, 3, mixed_pre_constraints, 4, 2, SRS_ALPHA,
                   challenger=O.DuplexChallenger(ch_consts[0]), trace=trace, pre=pre, publics=pub)
    assert res == ALL_TRUE, res
    pp.close()
    # given alpha and zeta (no challenger), 2^3 rows
    n = 8
    rows, pub = mixed_pre_trace(7, 8, 9, n)
    trace, pre = M.to_limbs(rows), M.to_limbs(mixed_pre_preprocessed(n))
    pp = setup_preprocessed(pcs, dev(pre))
    a, z = 0x1111222233334444, 0x5555666677778888
    proof = prove_native(prog, pcs, dev(trace), a, z, public_values=pub, preprocessed=pp)
    mpp = M.setup(pre, srs)
    assert_proofs_equal(proof, M.prove(trace, mpp, srs, mixed_pre_constraints, 2, pub, alpha=a, zeta=z))
    res = M.verify(proof, mpp.commitment, 3, mixed_pre_constraints, 3, 2, SRS_ALPHA, alpha=a, zeta=z, trace=trace,
                   pre=pre, publics=pub)
    assert res == {"ood": True, "opened_vs_trace": True, "kzg": True}, res
    pp.close()


def test_one_setup_many_proves(gpu_ctx, pcs, srs, ch_consts):
    """PreprocessedProverData is reused across proofs (preprocessed.rs:8-11)."""
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    n = 8
    pre = M.to_limbs(mul_fib_p_preprocessed(n))
    prog = AirProgram(MulFibPAir(), gpu_ctx)
    pp = setup_preprocessed(pcs, dev(pre))
    commit = C.g1_msm_columns(srs[:n], C.idft_batch(pre))
    proofs = []
    for a, b in ((0, 1), (2, 3)):
        trace = M.to_limbs(mul_fib_p_trace(a, b, n))
        proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), preprocessed=pp)
        np.testing.assert_array_equal(proof.preprocessed_commit[0], commit)
        # the preprocessed openings verify against the one setup commitment
        res = M.verify(proof, commit, 2, mul_fib_p_constraints, 3, 1, SRS_ALPHA,
                       challenger=O.DuplexChallenger(ch_consts[0]), trace=trace, pre=pre)
        assert res == ALL_TRUE, res
        proofs.append(proof)
    assert proofs[0].zeta != proofs[1].zeta
    np.testing.assert_array_equal(proofs[0].preprocessed_commit[0], proofs[1].preprocessed_commit[0])
    np.testing.assert_array_equal(pp.commitment, commit)
    pp.close()


def test_tampered_preprocessed_and_foreign_setup_do_not_verify(gpu_ctx, pcs, srs, ch_consts):
    """mul_fib_pair.rs's tamper test on the GPU: the setup commits a preprocessed trace that
    differs at row 3 from the one the (honest) trace was generated with; and an honest proof
    against another setup's commitment."""
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import prove_native, setup_preprocessed

    n = 8
    trace = M.to_limbs(mul_fib_p_trace(0, 1, n))
    prog = AirProgram(MulFibPAir(), gpu_ctx)
    bad = M.to_limbs(mul_fib_p_preprocessed(n, tamper_index=3))
    pp = setup_preprocessed(pcs, dev(bad))
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), preprocessed=pp)
    res = M.verify(proof, pp.commitment, 2, mul_fib_p_constraints, 3, 1, SRS_ALPHA,
                   challenger=O.DuplexChallenger(ch_consts[0]), trace=trace, pre=bad)
    assert res == {"transcript": True, "ood": False, "opened_vs_trace": True, "kzg": True}, res
    pp.close()
    good = M.to_limbs(mul_fib_p_preprocessed(n))
    pp = setup_preprocessed(pcs, dev(good))
    proof = prove_native(prog, pcs, dev(trace), None, None, challenger=challenger(ch_consts), preprocessed=pp)
    other = M.setup(bad, srs).commitment
    res = M.verify(proof, other, 2, mul_fib_p_constraints, 3, 1, SRS_ALPHA, challenger=O.DuplexChallenger(ch_consts[0]))
    assert res["transcript"] is False
    pp.close()


def test_prove_rejections(gpu_ctx, pcs):
    import torch

    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import NativeKzgPcs, prove_native, setup_preprocessed

    n = 8
    trace = dev(M.to_limbs(mul_fib_p_trace(0, 1, n)))
    prog = AirProgram(MulFibPAir(), gpu_ctx)

    def fails(code, **kw):
        with pytest.raises(_lib.EonError) as e:
            prove_native(prog, pcs, trace, 3, 4, **kw)
        msg = pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode()
        return e.value.code == code and len(msg) > 0

    assert fails(_lib.EON_E_ARG)  # eon_prove_air on a program with preprocessed columns
    tall = setup_preprocessed(pcs, dev(M.to_limbs(mul_fib_p_preprocessed(16))))
    assert fails(_lib.EON_E_SHAPE, preprocessed=tall)  # degree_bits 4 for a 2^3-row trace
    wide = setup_preprocessed(pcs, dev(M.to_limbs(mixed_pre_preprocessed(n))))
    assert fails(_lib.EON_E_SHAPE, preprocessed=wide)  # width 3 for an AIR with 2
    other_pcs = NativeKzgPcs(16, SRS_ALPHA, gpu_ctx)
    foreign = setup_preprocessed(other_pcs, dev(M.to_limbs(mul_fib_p_preprocessed(n))))
    assert fails(_lib.EON_E_ARG, preprocessed=foreign)  # committed with another pcs
    foreign.close()
    other_pcs.close()
    # a program without preprocessed columns refuses preprocessed data (width 0 != 2) ...
    fib = AirProgram(FibonacciAir(), gpu_ctx)
    good = setup_preprocessed(pcs, dev(M.to_limbs(mul_fib_p_preprocessed(n))))
    with pytest.raises(_lib.EonError) as e:
        prove_native(fib, pcs, trace, 3, 4, public_values=[0, 1, 21], preprocessed=good)
    assert e.value.code == _lib.EON_E_SHAPE
    for h in (tall, wide, good):
        h.close()
    # ... and setup refuses a matrix without columns (the reference returns None)
    with pytest.raises(_lib.EonError) as e:
        setup_preprocessed(pcs, torch.zeros((n, 0, 4), dtype=torch.int64, device="cuda:0"))
    assert e.value.code == _lib.EON_E_SHAPE and len(pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode()) > 0
    h = ctypes.c_void_p()
    rc = pcs.lib.eon_setup_preprocessed(pcs._h, ctypes.c_void_p(trace.data_ptr()), n, 0, ctypes.byref(h))
    assert rc == _lib.EON_E_SHAPE


def test_pp_call_without_preprocessed_is_the_plain_prove(gpu_ctx, pcs):
    """eon_prove_air_pp with pp = NULL on a program without preprocessed columns is eon_prove_air."""
    from plonky3_eon_amd import native
    from plonky3_eon_amd.air import AirProgram, _publics_limbs
    from plonky3_eon_amd.field import fr_to_abi

    pis = [0, 1, 21]
    trace = dev(M.to_limbs(O.fib_trace(0, 1, 8)))
    prog = AirProgram(FibonacciAir(), gpu_ctx)
    plain = native.prove_native(prog, pcs, trace, 0x1111, 0x2222, public_values=pis)
    tc, qc = np.zeros((2, 8), np.uint64), np.zeros((1, 8), np.uint64)
    to, tw = np.zeros((2, 2, 4), np.uint64), np.zeros((2, 2, 8), np.uint64)
    qo, qw = np.zeros((1, 4), np.uint64), np.zeros((1, 8), np.uint64)
    p = native._p
    out = native.eon_proof_pp(native.eon_proof(p(tc), p(qc), p(to), p(tw), p(qo), p(qw), 0), None, None, None)
    pub = _publics_limbs(pis)
    a, z = fr_to_abi(0x1111), fr_to_abi(0x2222)
    pcs.check(pcs.lib.eon_prove_air_pp(pcs._h, prog.handle, ctypes.c_void_p(trace.data_ptr()), 8, p(pub), 3, None,
                                       ctypes.byref(a), ctypes.byref(z), ctypes.byref(out)))
    np.testing.assert_array_equal(tc, plain.trace_commit[0])
    np.testing.assert_array_equal(qc[0:1], plain.quotient_commit[0])
    np.testing.assert_array_equal(tw[1], plain.opened[0].witnesses[0][1])
    np.testing.assert_array_equal(qw[0:1], plain.opened[1].witnesses[0][0])
    assert plain.preprocessed_commit is None and len(plain.opened) == 2
