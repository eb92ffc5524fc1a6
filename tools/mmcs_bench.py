#!/usr/bin/env python3
"""Times a KzgMmcs query batch on one GPU and prints one JSON line: open_batch_many
(eon_kzg_mmcs_open_dev: every distinct (matrix, local index) divided in one multi-point pass, one wide
column MSM per group) against the same openings done point by point through the single-point entries
-- eon_quotient_and_eval_columns_dev, then eon_msm_g1_columns_dev of that point's `width` quotient
columns -- on the same library and the same SRS tables, with the in-kernel clock of
eon_diag_clock_probe right after, as bench.py reports it.  Both routes are checked to agree.

    python tools/mmcs_bench.py [--log-heights 16 14] [--width 16] [--indices 32] [--steps 5] [--warmup 2]
"""

import argparse
import ctypes
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
    ap.add_argument("--log-heights", type=int, nargs="+", default=[16, 14])
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--indices", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Context, KzgMmcs
    from plonky3_eon_amd.field import fr_to_abi
    from plonky3_eon_amd.mmcs import local_index

    ctx = Context(0)
    heights = [1 << k for k in args.log_heights]
    w = args.width
    mmcs = KzgMmcs(max(heights) - 1, 12345, ctx)
    g = torch.Generator(device="cuda:0").manual_seed(1)

    def random_fr(h):
        lo = torch.randint(-(1 << 63), (1 << 63) - 1, (h, w, 3), dtype=torch.int64, device="cuda:0", generator=g)
        hi = torch.randint(0, 0x30644E72E131A029, (h, w, 1), dtype=torch.int64, device="cuda:0", generator=g)
        return torch.cat([lo, hi], dim=2).contiguous()  # top limb below the modulus': canonical

    mats = [random_fr(h) for h in heights]
    _, data = mmcs.commit(mats)
    rng = np.random.default_rng(2)
    indices = [int(i) for i in rng.integers(0, max(heights), args.indices)]
    distinct = [sorted({local_index(max(heights), h, i) for i in indices}) for h in heights]

    def timed(fn):
        out = []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            if i >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    batched = {}

    def run_batched():
        batched["out"] = mmcs.open_batch_many(indices, data)

    lib, h_ctx = ctx.lib, ctx.handle
    quot = [torch.empty((h - 1, w, 4), dtype=torch.int64, device="cuda:0") for h in heights]
    vals = torch.empty((w, 4), dtype=torch.int64, device="cuda:0")
    single = {}

    def run_single():
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for k, (m, h) in enumerate(zip(mats, heights)):
            for loc in distinct[k]:
                z = fr_to_abi(loc)
                wit = np.zeros((w, 8), dtype=np.uint64)
                ctx.check(lib.eon_quotient_and_eval_columns_dev(h_ctx, ctypes.c_void_p(m.data_ptr()), h, w,
                                                                ctypes.byref(z), ctypes.c_void_p(quot[k].data_ptr()),
                                                                ctypes.c_void_p(vals.data_ptr())))
                ctx.check(lib.eon_msm_g1_columns_dev(h_ctx, mmcs.bases._h, ctypes.c_void_p(quot[k].data_ptr()), h - 1,
                                                     w, wit.ctypes.data_as(ctypes.c_void_p)))
                single[(k, loc)] = (vals.cpu().numpy().view(np.uint64).copy(), wit)

    batched_ms = timed(run_batched)
    single_ms = timed(run_single)
    for q, i in enumerate(indices):
        for k, h in enumerate(heights):
            v, wt = single[(k, local_index(max(heights), h, i))]
            assert np.array_equal(batched["out"][q][0][k], v) and np.array_equal(batched["out"][q][1][k], wt), (q, k)
    ctx.profile(True)
    run_batched()
    ctx.synchronize()
    kernels = ctx.profile_report()
    ctx.profile(False)
    clock = ctx.clock_probe(160, 1024)
    print(json.dumps({
        "workload": "mmcs_open", "heights": heights, "width": w, "indices": args.indices,
        "distinct_points": [len(d) for d in distinct],
        "open_batch_many_ms": [round(x, 3) for x in batched_ms],
        "open_batch_many_ms_median": round(statistics.median(batched_ms), 3),
        "per_point_route_ms": [round(x, 3) for x in single_ms],
        "per_point_route_ms_median": round(statistics.median(single_ms), 3),
        "routes_agree": True,
        "open_batch_many_kernels": {k: v for k, v in kernels.items() if k.startswith("k_horner")},
        "gpu_clock_inkernel_mhz": round(clock["clock_mhz_median"], 1)}))


if __name__ == "__main__":
    main()
