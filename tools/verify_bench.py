#!/usr/bin/env python3
"""Times the verifier's two device parts on one GPU and prints one JSON line:

* eon_air_eval_at_point_dev (k_air_point) of AirProgram(Poseidon2Air, VECTOR_LEN 8) -- 1312 columns,
  1280 constraints, one lane running the whole program -- on random opened values: the kernel by the
  context's HIP-event profile and the whole synchronous call by the host clock;
* native.verify_native of one small proof of the same AIR (2^3 rows, fused prove, given
  challenges): the host clock around the call, and the profile's split into k_air_point and the
  kernels of eon_kzg_verify_batch.  The proof has the headline's 2 * 1312 + 2 = 2626 openings (their
  number does not depend on the height), so the pairing part is the headline's.

The in-kernel clock of eon_diag_clock_probe right after, as bench.py reports it.

    python tools/verify_bench.py [--vector-len 8] [--steps 9] [--warmup 3]
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vector-len", type=int, default=8)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air
    from plonky3_eon_amd.native import NativeKzgPcs, prove_native, verify_native

    vl = args.vector_len
    ctx = Context(0)
    rng = np.random.default_rng(1)  # a fixed round-constant set: the values do not matter for the time
    k = rng.integers(0, 1 << 60, (8 * 3 + 56, 4), dtype=np.uint64)
    air = Poseidon2Air(k[:12].reshape(4, 3, 4), k[24:], k[12:24].reshape(4, 3, 4), vl, ctx)
    prog = AirProgram(air, ctx)

    def random_fr(*shape):
        """canonical residues: the top limb below 2^60 < p's"""
        t = torch.randint(-(1 << 63), (1 << 63) - 1, (*shape, 4), dtype=torch.int64, device="cuda:0")
        t[..., 3] &= (1 << 60) - 1
        return t

    def timed(fn):
        """-> (median host ms of the synchronous call, median per-kernel ms {name: ms})"""
        wall, kern = [], {}
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            ctx.profile(True)
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            rep = ctx.profile_report()
            ctx.profile(False)
            if i >= args.warmup:
                wall.append((t1 - t0) * 1e3)
                for name, r in rep.items():
                    kern.setdefault(name, []).append(r["total_ms"])
        return statistics.median(wall), {n: statistics.median(v) for n, v in kern.items()}

    local, nxt = random_fr(air.width), random_fr(air.width)
    eval_wall, eval_kern = timed(lambda: prog.eval_at_point(17, 0x123456789abcdef, 0xfedcba987654321, local, nxt))

    n = 8
    trace = air.generate_trace(random_fr(n * vl, 3))
    pcs = NativeKzgPcs(n, 12345, ctx)
    proof = prove_native(air, pcs, trace, 0x1111222233334444, 0x5555666677778888)
    verify_native(prog, pcs, proof)  # g2_alpha is made at the first verify
    ver_wall, ver_kern = timed(lambda: verify_native(prog, pcs, proof))
    pcs.close()
    clock = ctx.clock_probe(160, 1024)
    point = ver_kern.get("k_air_point", 0.0)
    print(json.dumps({
        "workload": "verify", "air": f"AirProgram(Poseidon2Air, VECTOR_LEN {vl})", "width": air.width,
        "num_constraints": prog.num_constraints, "num_instructions": prog.stats["num_instructions"],
        "num_registers": prog.stats["num_registers"],
        "eval_at_point_call_ms": round(eval_wall, 4), "eval_at_point_kernel_ms": round(eval_kern["k_air_point"], 4),
        "verify_log_trace": 3, "verify_openings": 2 * air.width + 2, "verify_call_ms": round(ver_wall, 4),
        "verify_k_air_point_ms": round(point, 4),
        "verify_other_kernels_ms": round(sum(v for name, v in ver_kern.items() if name != "k_air_point"), 4),
        "verify_kernels_ms": {name: round(v, 4) for name, v in sorted(ver_kern.items())},
        "gpu_clock_inkernel_mhz": round(clock["clock_mhz_median"], 1)}))


if __name__ == "__main__":
    main()
