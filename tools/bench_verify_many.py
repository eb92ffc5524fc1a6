#!/usr/bin/env python3
"""Times native.verify_native_many against the same proofs verified one call at a time, in one
process and one session, and writes one JSON file (also printed as one line).

Two shapes: the headline's -- AirProgram(Poseidon2Air, VECTOR_LEN 8), 1312 columns, whose proof has
the headline's 2 * 1312 + 2 = 2626 openings whatever the height -- and a small one (VECTOR_LEN 1).
N distinct inputs are proved at 2^3 rows for N = 1, 4, 16, 64 (capped by --max-n), in both opening
modes, and verified with the given challenges and under Fiat-Shamir.  Per cell: the median wall time
of the batch and of the N sequential calls, their ratio, the batch's per-kernel times
(eon_ctx_profile) and what is left of its wall time for the host (prepare, marshalling).  The
in-kernel clock (eon_diag_clock_probe) is read at the end, as bench.py reports it.

    python tools/bench_verify_many.py [--max-n 64] [--steps 5] [--warmup 2] [--out profiles/r07/verify_many.json]
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
    ap.add_argument("--max-n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--vector-lens", type=int, nargs="+", default=[8, 1])
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "r07" / "verify_many.json")
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air
    from plonky3_eon_amd.native import (Challenger, NativeKzgPcs, Poseidon2Constants, prove_native, verify_native,
                                        verify_native_many)

    ctx = Context(0)
    rng = np.random.default_rng(1)  # fixed constants: the values do not matter for the time
    k = rng.integers(0, 1 << 60, (8 * 3 + 56, 4), dtype=np.uint64)
    kc = rng.integers(0, 1 << 60, (8 * 3 + 22, 4), dtype=np.uint64)
    ch_consts = Poseidon2Constants(kc[:12].reshape(4, 3, 4), kc[24:], kc[12:24].reshape(4, 3, 4))
    ns = [n for n in (1, 4, 16, 64) if n <= args.max_n]
    rows = 8

    def random_fr(*shape):
        """canonical residues: the top limb below 2^60 < p's"""
        t = torch.randint(-(1 << 63), (1 << 63) - 1, (*shape, 4), dtype=torch.int64, device="cuda:0")
        t[..., 3] &= (1 << 60) - 1
        return t

    def median_ms(fn):
        out = []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    def kernels_ms(fn):
        torch.cuda.synchronize()
        ctx.profile(True)
        fn()
        rep = ctx.profile_report()
        ctx.profile(False)
        return {name: round(r["total_ms"], 4) for name, r in sorted(rep.items())}

    cells = []
    for vl in args.vector_lens:
        air = Poseidon2Air(k[:12].reshape(4, 3, 4), k[24:], k[12:24].reshape(4, 3, 4), vl, ctx)
        prog = AirProgram(air, ctx)
        pcs = NativeKzgPcs(rows, 12345, ctx)
        traces = [air.generate_trace(random_fr(rows * vl, 3)) for _ in range(max(ns))]
        for opening in ("per_column", "batched"):
            proofs = {"given": [prove_native(air, pcs, t, 0x1111222233334444 + i, 0x5555666677778888 + i,
                                             opening=opening, gamma=0x1234 + i if opening == "batched" else None,
                                             delta=0x4321 + i if opening == "batched" else None)
                                for i, t in enumerate(traces)],
                      "fs": [prove_native(air, pcs, t, None, None, challenger=Challenger(ch_consts), opening=opening)
                             for t in traces]}
            verify_native(prog, pcs, proofs["given"][0])  # a proof that does not verify is no measurement
            for mode in ("given", "fs"):
                for n in ns:
                    batch = proofs[mode][:n]

                    def chs():
                        return [Challenger(ch_consts) for _ in range(n)] if mode == "fs" else None

                    def many():
                        res = verify_native_many(prog, pcs, batch, None, chs())
                        assert res == [None] * n, res

                    def sequential():
                        cs = chs()
                        for i, p in enumerate(batch):
                            verify_native(prog, pcs, p, challenger=cs[i] if cs else None)

                    sequential()  # g2_alpha is made at the first verify
                    seq, bat = median_ms(sequential), median_ms(many)
                    kern = kernels_ms(many)
                    device = sum(kern.values())
                    cells.append({"vector_len": vl, "width": air.width, "openings_per_proof": 2 * air.width + 2,
                                  "opening": opening, "mode": mode, "n": n, "sequential_ms": round(seq, 3),
                                  "batch_ms": round(bat, 3), "sequential_over_batch": round(seq / bat, 3),
                                  "batch_kernels_ms": kern, "batch_device_ms": round(device, 3),
                                  "batch_host_ms": round(bat - device, 3)})
                    print(json.dumps(cells[-1]), file=sys.stderr)
        pcs.close()
    clock = ctx.clock_probe(160, 1024)
    out = {"workload": "verify_many", "rows": rows, "steps": args.steps, "warmup": args.warmup,
           "gpu_clock_inkernel_mhz": round(clock["clock_mhz_median"], 1), "cells": cells}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
