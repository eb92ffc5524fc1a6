#!/usr/bin/env python3
"""Times the two opening modes at the headline shape on one GPU, in one session, and prints one JSON
line: the open stage and the whole prove per-column (the reference's KzgPcs::open: one witness per
column and point) and batched (EON_OPENING_BATCHED: one witness per matrix and point), the verify in
both modes, the gamma-fold kernel on the trace-shaped matrix with its read bandwidth against a plain
device copy of the same matrix measured right there, and the in-kernel clock of
eon_diag_clock_probe, as bench.py reports it.  Medians of --steps runs after --warmup.

The per-column mode is the baseline: with the mode at its default the prove is launch for launch
what it was before the batched mode existed, so both columns come from one build on one box.

    python tools/batched_open_bench.py [--log-trace 17] [--vector-len 8] [--steps 5] [--warmup 2]
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
    ap.add_argument("--log-trace", type=int, default=17)
    ap.add_argument("--vector-len", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-verify", action="store_true")
    args = ap.parse_args()

    import torch

    from bench import p2_constants_limbs, synthetic_fr
    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air
    from plonky3_eon_amd.msm import fold_columns
    from plonky3_eon_amd.native import Challenger, NativeKzgPcs, Poseidon2Constants, prove_native, verify_native

    ctx = Context(0)
    n, vl = 1 << args.log_trace, args.vector_len
    air = Poseidon2Air(*p2_constants_limbs(99), vl, ctx)
    pcs = NativeKzgPcs(n, 12345, ctx)
    inputs = synthetic_fr(n * vl, 3, 5).reshape(-1, 3, 4)
    trace = air.generate_trace(torch.from_numpy(np.ascontiguousarray(inputs).view(np.int64)).to("cuda:0"))
    del inputs
    ch_consts = p2_constants_limbs(77)

    def challenger():
        return Challenger(Poseidon2Constants(*ch_consts))

    def median(xs):
        return round(statistics.median(xs), 3)

    out = {"workload": "batched_open", "log_trace": args.log_trace, "vector_len": vl, "trace_width": int(trace.shape[1]),
           "steps": args.steps, "warmup": args.warmup}
    proofs = {}
    for mode in ("per_column", "batched"):
        opens, totals = [], []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = prove_native(air, pcs, trace, None, None, challenger=challenger(), opening=mode)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                opens.append(p.timings_ms["open"])
                totals.append(dt)
        proofs[mode] = p
        out[mode] = {"open_ms": [round(x, 3) for x in opens], "open_ms_median": median(opens),
                     "prove_ms": [round(x, 3) for x in totals], "prove_ms_median": median(totals),
                     "witnesses": int(sum(np.asarray(w).reshape(-1, 8).shape[0] for o in p.opened for m in o.witnesses
                                          for w in m))}
    a, b = proofs["per_column"], proofs["batched"]
    assert (a.alpha, a.zeta) == (b.alpha, b.zeta) and np.array_equal(a.trace_commit[0], b.trace_commit[0])
    assert all(np.array_equal(x, y) for x, y in zip(a.opened[0].values[0], b.opened[0].values[0]))
    out["same_commitments_values_challenges"] = True

    if not args.no_verify:
        prog = AirProgram(air, ctx)
        for mode in ("per_column", "batched"):
            ms = []
            for i in range(args.warmup + args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                verify_native(prog, pcs, proofs[mode], challenger=challenger())
                if i >= args.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            out[mode]["verify_ms"] = [round(x, 3) for x in ms]
            out[mode]["verify_ms_median"] = median(ms)

    # the fold kernel alone on the trace-shaped matrix (the coefficients have the trace's shape), and
    # a plain device copy of the same matrix: HIP events on torch's stream
    def event_ms(fn):
        ms = []
        for i in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        return ms

    gamma = b.gamma
    fold_ms = event_ms(lambda: fold_columns(trace, gamma, None, ctx))
    dst = torch.empty_like(trace)
    copy_ms = event_ms(lambda: dst.copy_(trace))
    del dst
    mat_bytes = trace.numel() * 8
    fold_gbps = mat_bytes / (statistics.median(fold_ms) * 1e-3) / 1e9
    copy_gbps = 2 * mat_bytes / (statistics.median(copy_ms) * 1e-3) / 1e9  # read + write
    out["fold"] = {"rows": n, "width": int(trace.shape[1]), "matrix_bytes": mat_bytes,
                   "fold_ms": [round(x, 3) for x in fold_ms], "fold_ms_median": median(fold_ms),
                   "fold_read_GBps": round(fold_gbps, 1),
                   "copy_ms": [round(x, 3) for x in copy_ms], "copy_ms_median": median(copy_ms),
                   "copy_read_plus_write_GBps": round(copy_gbps, 1),
                   "fold_bandwidth_over_copy": round(fold_gbps / copy_gbps, 3),
                   "products_per_s": round(n * int(trace.shape[1]) / (statistics.median(fold_ms) * 1e-3), 0)}
    clock = ctx.clock_probe(160, 1024)
    out["gpu_clock_inkernel_mhz"] = round(clock["clock_mhz_median"], 1)
    out["probe_products_per_s"] = round(clock["products_per_s"], 0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
