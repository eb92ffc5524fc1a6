#!/usr/bin/env python3
"""Times check_constraints on one GPU at the headline shape and prints one JSON line:
AirProgram(Poseidon2Air, VECTOR_LEN 8), 2^17 rows x 1312 columns, on a valid trace (generate_trace)
and on a fully random one (every row failing: the worst case of the per-wave atomics), next to the
generic quotient_values of the same program at 2^18 rows in the same process -- the yardstick: the
check runs the same program over half as many rows without the alpha folds and the inv_vanishing
product, so check / quotient above 1 means something is wrong.  Each figure is the k_air_check /
k_air_quotient launch by the context's HIP-event profile, and the whole call between two HIP events
on the stream (the check's includes its synchronous read-back); the in-kernel clock of
eon_diag_clock_probe right after, as bench.py reports it.

    python tools/check_bench.py [--log-trace 17] [--vector-len 8] [--steps 5] [--warmup 2]
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-trace", type=int, default=17)
    ap.add_argument("--vector-len", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air

    n, vl = 1 << args.log_trace, args.vector_len
    ctx = Context(0)
    # a fixed round-constant set: the values do not matter for the time
    rng = np.random.default_rng(1)
    k = rng.integers(0, 1 << 60, (8 * 3 + 56, 4), dtype=np.uint64)
    air = Poseidon2Air(k[:12].reshape(4, 3, 4), k[24:], k[12:24].reshape(4, 3, 4), vl, ctx)
    prog = AirProgram(air, ctx)

    def random_fr(rows, cols):
        """canonical residues: the top limb below 2^60 < p's"""
        t = torch.randint(-(1 << 63), (1 << 63) - 1, (rows, cols, 4), dtype=torch.int64, device="cuda:0")
        t[:, :, 3] &= (1 << 60) - 1
        return t

    valid = air.generate_trace(random_fr(n * vl, 3))
    rand = random_fr(n, air.width)
    lde = random_fr(2 * n, air.width)

    def timed(name, fn):
        """-> (kernel ms by the context's profile, call ms between two HIP events), medians"""
        kern, call = [], []
        for i in range(args.warmup + args.steps):
            ctx.profile(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            rep = ctx.profile_report()
            ctx.profile(False)
            if i >= args.warmup:
                call.append(e0.elapsed_time(e1))
                kern.append(rep[name]["total_ms"] / rep[name]["launches"])
        return statistics.median(kern), statistics.median(call), out

    check_k, check_c, rep_valid = timed("k_air_check", lambda: prog.check_constraints(valid))
    rand_k, rand_c, rep_rand = timed("k_air_check", lambda: prog.check_constraints(rand))
    quot_k, quot_c, _ = timed("k_air_quotient", lambda: prog.quotient_values(lde, args.log_trace, 1, 0x1234567))
    clock = ctx.clock_probe(160, 1024)
    assert rep_valid.failures == 0, rep_valid
    print(json.dumps({
        "workload": "check_constraints", "air": f"AirProgram(Poseidon2Air, VECTOR_LEN {vl})",
        "log_trace": args.log_trace, "width": air.width, "num_constraints": prog.num_constraints,
        "check_valid_kernel_ms": round(check_k, 4), "check_valid_call_ms": round(check_c, 4),
        "check_random_kernel_ms": round(rand_k, 4), "check_random_call_ms": round(rand_c, 4),
        "check_random_failures": rep_rand.failures,
        "quotient_kernel_ms": round(quot_k, 4), "quotient_call_ms": round(quot_c, 4),
        "check_over_quotient_kernel": round(check_k / quot_k, 4) if quot_k else None,
        "check_random_over_valid_kernel": round(rand_k / check_k, 4) if check_k else None,
        "gpu_clock_inkernel_mhz": round(clock["clock_mhz_median"], 1)}))


if __name__ == "__main__":
    main()
