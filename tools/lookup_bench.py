#!/usr/bin/env python3
"""Times the LogUp path on one GPU and prints one JSON line: eon_lookup_permutation_dev (wall per
call, and per kernel from the context's HIP-event profile: k_lookup_terms + k_lookup_contrib are the
contributions, k_sum_block + k_sum_apply the running sum) and the lookup prove (eon_prove_air_lk_fs)
for the range-check AIR of tests/airs_lookup.py (preprocessed table, two lookups, four terms), with
the in-kernel clock of eon_diag_clock_probe right after, as bench.py reports it.

    python tools/lookup_bench.py [--log-trace 17] [--steps 5] [--warmup 2]
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-trace", type=int, default=17)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    from airs_lookup import RangeCheckAir

    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.field import ints_to_limbs
    from plonky3_eon_amd.native import Challenger, NativeKzgPcs, Poseidon2Constants, prove_native, setup_preprocessed

    n = 1 << args.log_trace
    rng = np.random.default_rng(1)
    v = rng.integers(0, n, n)
    m = np.bincount(v, minlength=n)
    rows = np.stack([v, m, (v + 1) % n], axis=1)

    def dev(ints, w):
        a = np.ascontiguousarray(ints_to_limbs([int(x) for x in ints])).reshape(n, w, 4)
        return torch.from_numpy(a.view(np.int64)).to("cuda:0")

    trace, pre = dev(rows.reshape(-1), 3), dev(np.arange(n), 1)
    pub = [int(rows[0][2])]
    ctx = Context(0)
    prog = AirProgram(RangeCheckAir(), ctx)
    ch = [int(x) for x in rng.integers(1 << 62, 1 << 63, 4)]

    def timed(fn, steps, warmup):
        out = []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            torch.cuda.synchronize()
            if i >= warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    perm_ms = timed(lambda: prog.lookup_permutation(trace, ch, pub, preprocessed_trace=pre), args.steps, args.warmup)
    ctx.profile(True)
    prog.lookup_permutation(trace, ch, pub, preprocessed_trace=pre)
    ctx.synchronize()
    kernels = ctx.profile_report()
    ctx.profile(False)

    # a fixed round-constant set for the transcript: its values do not matter for the time
    k = np.arange(1, 1 + 4 * 3 * 4, dtype=np.uint64).reshape(4, 3, 4) % 7
    consts = Poseidon2Constants(k[:2], np.arange(22 * 4, dtype=np.uint64).reshape(22, 4) % 5, k[2:])
    pcs = NativeKzgPcs(n, 12345, ctx)
    pp = setup_preprocessed(pcs, pre)
    stages = {}

    def prove():
        p = prove_native(prog, pcs, trace, None, None, challenger=Challenger(consts), public_values=pub,
                         preprocessed=pp, preprocessed_trace=pre)
        stages.update(p.timings_ms)

    prove_ms = timed(prove, max(1, args.steps // 2 + 1), 1)
    clock = ctx.clock_probe(160, 1024)
    print(json.dumps({
        "workload": "lookup", "air": "RangeCheckAir (tests/airs_lookup.py)", "log_trace": args.log_trace,
        "lookup_permutation_ms": [round(x, 4) for x in perm_ms],
        "lookup_permutation_ms_median": round(statistics.median(perm_ms), 4),
        "lookup_permutation_kernels": kernels,
        "prove_lk_ms": [round(x, 3) for x in prove_ms], "prove_lk_ms_median": round(statistics.median(prove_ms), 3),
        "prove_lk_stage_ms": {k_: round(v_, 3) for k_, v_ in stages.items()},
        "gpu_clock_inkernel_mhz": round(clock["clock_mhz_median"], 1)}))
    pp.close()
    pcs.close()


if __name__ == "__main__":
    main()
