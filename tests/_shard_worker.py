"""One rank of the column-sharded prove tests (launched by test_gpu_prove_sharded.py as a subprocess,
RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment, backend gloo, every rank on
cuda:0).

Every rank proves its column slice over a TorchCollective AND the full trace unsharded on its own,
with given alpha / zeta and with a challenger, and compares Proof.to_bytes() and the challenges: no
rank may end with other bytes than the one-device prove.

  mixed    MixedAir (W = 5, log_qd 3: 8 chunks, public values, selectors), log_n 4, random trace
  mul      MulAir (W = 60, 2 chunks), log_n 5, random trace
  fib      FibonacciAir (W = 2), log_n 3, the valid trace; verify_native accepts the sharded proof
  fib_too_many   FibonacciAir over more ranks than columns: every rank must raise, none may wait
  keccak   KeccakAir (W = 2633), one hash: 32 rows
  refuse   what stays unsharded raises with its reason before any exchange

Writes {"ok": true} or {"ok": false, "why": ...} as JSON to argv[2].
"""

import json
import os
import sys
import traceback
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

from oracle import coracle as C  # noqa: E402
from oracle import pyoracle as O  # noqa: E402
from oracle.smallrng import SmallRng, poseidon2_new_from_rng  # noqa: E402

ALPHA, ZETA = 0x1234567890ABCDEF1234, 0xFEDCBA0987654321
SRS_ALPHA = 12345


def lim(x):
    return np.array(O.int_to_limbs(O.to_mont(x % O.P)), dtype=np.uint64)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def challenger():
    from plonky3_eon_amd.native import Challenger, Poseidon2Constants

    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    return Challenger(Poseidon2Constants([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]],
                                         [[lim(v) for v in r] for r in py[2]]))


def same(got, want, what):
    """None when the two proofs are the same bytes and challenges, else why not"""
    if (got.alpha, got.zeta) != (want.alpha, want.zeta):
        return f"{what}: challenges differ from the unsharded prove's"
    if got.to_bytes() != want.to_bytes():
        for name in ("trace_commit", "quotient_commit"):
            if not np.array_equal(np.asarray(getattr(got, name)), np.asarray(getattr(want, name))):
                return f"{what}: {name} differs from the unsharded prove's"
        return f"{what}: proof bytes differ from the unsharded prove's (openings)"
    return None


def compare(rank, world, prog, pcs, full, publics, full_width_too=True):
    """sharded (slice, and the full-width trace) against unsharded, given challenges and transcript"""
    from plonky3_eon_amd import distributed as D
    from plonky3_eon_amd.collective import TorchCollective
    from plonky3_eon_amd.native import prove_native

    coll = TorchCollective(rank, world, None)
    c0, wl = D.column_range(prog.width, world, rank)
    mine = full[:, c0:c0 + wl].contiguous()
    want = prove_native(prog, pcs, full, ALPHA, ZETA, public_values=publics)
    got = prove_native(prog, pcs, mine, ALPHA, ZETA, collective=coll, public_values=publics)
    why = same(got, want, f"rank {rank}, given challenges")
    if why:
        return why, None
    if full_width_too:
        again = prove_native(prog, pcs, full, ALPHA, ZETA, collective=coll, public_values=publics)
        if again.to_bytes() != got.to_bytes():
            return f"rank {rank}: the full-width trace gives other bytes than the slice", None
    want_fs = prove_native(prog, pcs, full, None, None, challenger=challenger(), public_values=publics)
    got_fs = prove_native(prog, pcs, mine, None, None, collective=coll, challenger=challenger(),
                          public_values=publics)
    return same(got_fs, want_fs, f"rank {rank}, Fiat-Shamir"), got_fs


def random_trace(seed, n, width):
    return dev(C.random_fr(seed, n * width).reshape(n, width, 4))


def run_mixed(rank, world):
    from airs import MixedAir
    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import NativeKzgPcs

    ctx = Context(0)
    prog = AirProgram(MixedAir(), ctx)
    if (prog.width, prog.log_quotient_degree()) != (5, 3):
        return "MixedAir is not the 5-column, 8-chunk AIR this case is about"
    return compare(rank, world, prog, NativeKzgPcs(64, SRS_ALPHA, ctx), random_trace(11, 16, 5), [5, 6])[0]


def run_mul(rank, world):
    from airs import MulAir
    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import NativeKzgPcs

    ctx = Context(0)
    prog = AirProgram(MulAir(), ctx)
    if (prog.width, prog.log_quotient_degree()) != (60, 1):
        return "MulAir is not the 60-column, 2-chunk AIR this case is about"
    return compare(rank, world, prog, NativeKzgPcs(64, SRS_ALPHA, ctx), random_trace(12, 32, 60), [])[0]


def fib_case():
    from airs import FibonacciAir
    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import NativeKzgPcs

    ctx = Context(0)
    rows = O.fib_trace(0, 1, 8)
    trace = dev(np.stack([np.stack([lim(v) for v in r]) for r in rows]))
    return AirProgram(FibonacciAir(), ctx), NativeKzgPcs(64, SRS_ALPHA, ctx), trace, [0, 1, rows[-1][1]]


def run_fib(rank, world):
    from plonky3_eon_amd.native import verify_native

    prog, pcs, trace, publics = fib_case()
    why, proof = compare(rank, world, prog, pcs, trace, publics)
    if why:
        return why
    verify_native(prog, pcs, proof, publics, challenger=challenger())  # raises when rejected
    return None


def run_fib_too_many(rank, world):
    """world > W = 2: decided alike on every rank before the first collective call.  The slice a
    rank would own does not exist, so each passes the full trace; given challenges and transcript."""
    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.collective import TorchCollective
    from plonky3_eon_amd.native import prove_native

    prog, pcs, trace, publics = fib_case()
    coll = TorchCollective(rank, world, None)
    for ch in (None, challenger()):
        try:
            prove_native(prog, pcs, trace, ALPHA, ZETA, collective=coll, challenger=ch, public_values=publics)
        except _lib.EonError as e:
            if e.code != _lib.EON_E_ARG or "more ranks than columns" not in str(e):
                return f"rank {rank}: {e!r}"
        else:
            return f"rank {rank}: {world} ranks over 2 columns gave a proof"
    # the C entry point itself, behind the Python check: same code, same reason
    import ctypes

    from plonky3_eon_amd.field import fr_to_abi
    from plonky3_eon_amd.native import eon_proof

    a, z = fr_to_abi(ALPHA), fr_to_abi(ZETA)
    bufs = [np.zeros((2 * 8,), np.uint64) for _ in range(6)]
    out = eon_proof(*[b.ctypes.data_as(ctypes.c_void_p) for b in bufs], 0)
    pub = np.stack([lim(v) for v in publics])
    rc = pcs.lib.eon_prove_air_sharded(pcs._h, prog.handle, ctypes.c_void_p(trace.data_ptr()), 8,
                                       pub.ctypes.data_as(ctypes.c_void_p), 3, ctypes.byref(a), ctypes.byref(z),
                                       ctypes.byref(coll.c), ctypes.byref(out))
    msg = pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode()
    if rc != _lib.EON_E_ARG or "more ranks than columns" not in msg:
        return f"rank {rank}: eon_prove_air_sharded returned {rc} ({msg})"
    return None


def run_keccak(rank, world):
    from airs_keccak import smallrng_inputs
    from plonky3_eon_amd import Context, KeccakAir
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import NativeKzgPcs

    ctx = Context(0)
    air = KeccakAir(ctx)
    prog = AirProgram(air, ctx)
    if prog.width != 2633:
        return "KeccakAir is not 2633 columns wide"
    trace = air.generate_trace(dev(np.array(smallrng_inputs(1), dtype=np.uint64).reshape(-1, 25)))
    if tuple(trace.shape) != (32, 2633, 4):
        return f"Keccak trace {tuple(trace.shape)}"
    return compare(rank, world, prog, NativeKzgPcs(64, SRS_ALPHA, ctx), trace, [], full_width_too=False)[0]


def run_refuse(rank, world):
    from airs import MixedAir
    from airs_lookup import LookupMultisetEqAir, multiset_trace
    from airs_preprocessed import MulFibPAir, mul_fib_p_preprocessed, mul_fib_p_trace
    from plonky3_eon_amd import Context, _lib
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.collective import TorchCollective
    from plonky3_eon_amd.native import NativeKzgPcs, prove_native, setup_preprocessed

    ctx = Context(0)
    pcs = NativeKzgPcs(64, SRS_ALPHA, ctx)
    coll = TorchCollective(rank, world, None)

    def limbs(rows):
        return dev(np.stack([np.stack([lim(v) for v in r]) for r in rows]))

    def refused(reason, fn):
        try:
            fn()
        except (ValueError, _lib.EonError) as e:
            return None if reason in str(e) else f"rank {rank}: expected a refusal naming {reason!r}, got {e!r}"
        return f"rank {rank}: not refused ({reason})"

    mixed, mixed_trace = AirProgram(MixedAir(), ctx), random_trace(11, 16, 5)
    pre_prog = AirProgram(MulFibPAir(), ctx)
    pre_trace = limbs(mul_fib_p_trace(0, 1, 8))
    pp = setup_preprocessed(pcs, limbs(mul_fib_p_preprocessed(8)))
    lk_prog = AirProgram(LookupMultisetEqAir(), ctx)
    lk_trace = limbs(multiset_trace(8))
    checks = [
        ("preprocessed", lambda: prove_native(pre_prog, pcs, pre_trace, ALPHA, ZETA, collective=coll, preprocessed=pp)),
        # no handle given: the driver itself refuses the program
        ("preprocessed", lambda: prove_native(pre_prog, pcs, pre_trace, ALPHA, ZETA, collective=coll)),
        ("lookups", lambda: prove_native(lk_prog, pcs, lk_trace, None, None, collective=coll,
                                         challenger=challenger())),
        ("batched", lambda: prove_native(mixed, pcs, mixed_trace, ALPHA, ZETA, collective=coll, public_values=[5, 6],
                                         opening="batched", gamma=7)),
        ("columns", lambda: prove_native(mixed, pcs, mixed_trace[:, :4].contiguous(), ALPHA, ZETA, collective=coll,
                                         public_values=[5, 6])),
    ]
    for reason, fn in checks:
        why = refused(reason, fn)
        if why:
            return why
    pcs.check_constraints = True
    try:
        why = refused("check_constraints", lambda: prove_native(mixed, pcs, mixed_trace, ALPHA, ZETA, collective=coll,
                                                                public_values=[5, 6]))
        if why:
            return why
        # the driver's own refusal, behind the Python check
        import ctypes

        from plonky3_eon_amd.field import fr_to_abi
        from plonky3_eon_amd.native import eon_proof

        a, z = fr_to_abi(ALPHA), fr_to_abi(ZETA)
        bufs = [np.zeros((2 * 8 * 8,), np.uint64) for _ in range(6)]
        out = eon_proof(*[b.ctypes.data_as(ctypes.c_void_p) for b in bufs], 0)
        pub = np.stack([lim(5), lim(6)])
        rc = pcs.lib.eon_prove_air_sharded(pcs._h, mixed.handle, ctypes.c_void_p(mixed_trace.data_ptr()), 16,
                                           pub.ctypes.data_as(ctypes.c_void_p), 2, ctypes.byref(a), ctypes.byref(z),
                                           ctypes.byref(coll.c), ctypes.byref(out))
        msg = pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode()
        if rc != _lib.EON_E_ARG or "check_constraints" not in msg:
            return f"rank {rank}: eon_prove_air_sharded with the check on returned {rc} ({msg})"
    finally:
        pcs.check_constraints = False
    # and after all the refusals the group still proves
    return compare(rank, world, mixed, pcs, mixed_trace, [5, 6], full_width_too=False)[0]


MODES = {"mixed": run_mixed, "mul": run_mul, "fib": run_fib, "fib_too_many": run_fib_too_many,
         "keccak": run_keccak, "refuse": run_refuse}


def main():
    import torch.distributed as dist

    mode, out = sys.argv[1], sys.argv[2]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        why = MODES[mode](rank, world)
    except Exception:
        why = traceback.format_exc()
    finally:
        try:
            dist.barrier()
        except Exception:
            pass
        dist.destroy_process_group()
    Path(out).write_text(json.dumps({"ok": why is None, "why": why}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
