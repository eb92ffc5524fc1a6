#!/usr/bin/env python3
"""Rank 0's critical path of the column-sharded Keccak-AIR prove, on ONE GPU.

A one-GPU machine cannot run the exchanges, so this is the per-rank proxy bench.py --emulate-world is
for the lane-sharded prove: rank 0's column slice, its rows of the quotient, its opening-bases rows,
its quotient chunk and the full replicated transcript, with the emulated collective's device copies
standing in for the all_to_all and the all-gathers (eon_emulated_collective_init).  The proof it
returns is therefore NOT valid, and the xGMI time of the exchanges is not in these numbers.

For world 1, 2, 4, 8 it proves the Keccak-AIR at 682 hashes (16,384 rows, the height of the README's
trace-generation figure) with a Fiat-Shamir challenger and records the driver's stage_ms (mean over
the timed steps) and the wall time per prove.  It then times the pack and unpack kernels alone on
an LDE of that shape against a plain device copy of the bytes each one moves (HIP events, median),
alternating the two.  One JSON document, printed and written to --out.

    python tools/bench_prove_sharded.py [--hashes 682] [--steps 3] [--warmup 1] [--out profiles/r08/prove_sharded.json]
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

WORLDS = (1, 2, 4, 8)
FR_P3 = 0x30644E72E131A029


def synthetic_constants(seed, hf=4, pr=56):
    """the challenger's Poseidon2 round constants: canonical Montgomery limbs from a fixed seed"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.integers(0, 2**64, size=(6 * hf + pr, 4), dtype=np.uint64)
    x[..., 3] %= np.uint64(FR_P3)
    return x[:3 * hf].reshape(hf, 3, 4), x[3 * hf:3 * hf + pr], x[3 * hf + pr:].reshape(hf, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes", type=int, default=682)  # 16,384 rows
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08" / "prove_sharded.json"))
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Context, KeccakAir
    from plonky3_eon_amd import distributed as D
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import (STAGES, Challenger, EmulatedCollective, NativeKzgPcs, Poseidon2Constants,
                                        prove_native)

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this is a measurement, it does not fall back")
    ctx = Context(0)
    air = KeccakAir(ctx)
    prog = AirProgram(air, ctx)
    width, log_qd = prog.width, prog.log_quotient_degree()
    g = torch.Generator(device="cuda:0").manual_seed(1)
    inputs = torch.randint(-(1 << 63), (1 << 63) - 1, (args.hashes, 25), dtype=torch.int64, device="cuda:0", generator=g)
    trace = air.generate_trace(inputs)
    n = int(trace.shape[0])
    q, step = n << log_qd, 1 << log_qd
    pcs = NativeKzgPcs(n, 12345, ctx)
    consts = synthetic_constants(77)

    res = {"workload": "keccak_prove_column_sharded_emulated", "n_hashes": args.hashes, "rows": n, "width": width,
           "quotient_rows": q, "steps": args.steps, "warmup": args.warmup,
           "note": "rank 0 on one GPU, exchanges are local device copies: not a valid proof, no xGMI time",
           "worlds": {}}
    for world in WORLDS:
        coll = EmulatedCollective(0, world) if world > 1 else None
        c0, wl = D.column_range(width, world, 0)
        mine = trace[:, c0:c0 + wl].contiguous() if world > 1 else trace
        stage, wall = {}, []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = prove_native(prog, pcs, mine, None, None, collective=coll,
                             challenger=Challenger(Poseidon2Constants(*consts)))
            torch.cuda.synchronize()
            if i >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                for name in STAGES:
                    stage[name] = stage.get(name, 0.0) + p.timings_ms.get(name, 0.0) / args.steps
        del mine
        r_block = -(-q // world)
        res["worlds"][str(world)] = {
            "columns": wl, "quotient_rows": min(q, r_block), "window_rows": r_block + step if world > 1 else q,
            # what a real all_to_all sends off this rank: every block but its own
            "all_to_all_bytes_sent": (world - 1) * (r_block + step) * (-(-width // world)) * 32 if world > 1 else 0,
            "wall_ms": [round(x, 2) for x in wall], "wall_ms_mean": round(statistics.mean(wall), 2),
            "stage_ms": {k: round(v, 2) for k, v in stage.items()}}
    base = res["worlds"]["1"]["stage_ms"]
    for world in WORLDS[1:]:
        st = res["worlds"][str(world)]["stage_ms"]
        res["worlds"][str(world)]["gap_over_ideal_ms"] = {k: round(st[k] - base.get(k, 0.0) / world, 2) for k in st}
    del trace

    # the two copies alone, against a plain device copy of the same bytes
    def timed(fn, reps=10, warm=3):
        ms = []
        for i in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warm:
                ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    res["copies"] = {}
    for world in WORLDS[1:]:
        _, wl = D.column_range(width, world, 0)
        wmax, win = -(-width // world), -(-q // world) + step
        lde = torch.empty((q, wl, 4), dtype=torch.int64, device="cuda:0")
        lde.random_(generator=g)
        send = D.shard_pack_rows(ctx, lde, width, world, 0, step)
        window = D.shard_unpack_cols(ctx, send, q, width, step)  # the emulated exchange keeps the blocks
        # bytes = read + written; the plain copy compared with moves the same total (half each way)
        pack_bytes = world * win * (wl + wmax) * 32       # read wl, written wmax per block row
        unpack_bytes = 2 * win * width * 32               # every window element read and written once
        a_src = torch.zeros(pack_bytes // 16, dtype=torch.int64, device="cuda:0")
        a_dst = torch.empty_like(a_src)
        b_src, b_dst = window.reshape(-1), torch.empty_like(window.reshape(-1))
        rec = {}
        for name, fn, copy, nbytes in (
                ("pack", lambda: D.shard_pack_rows(ctx, lde, width, world, 0, step), lambda: a_dst.copy_(a_src),
                 pack_bytes),
                ("unpack", lambda: D.shard_unpack_cols(ctx, send, q, width, step), lambda: b_dst.copy_(b_src),
                 unpack_bytes)):
            c1, k, c2 = timed(copy), timed(fn), timed(copy)
            cm = (c1 + c2) / 2
            rec[name] = {"bytes": nbytes, "ms": round(k, 4), "gb_s": round(nbytes / k / 1e6, 1),
                         "copy_ms": round(cm, 4), "copy_gb_s": round(nbytes / cm / 1e6, 1),
                         "kernel_over_copy_time": round(k / cm, 3)}
        res["copies"][str(world)] = rec
        del lde, send, window, a_src, a_dst, b_src, b_dst
    res["gpu_clock_inkernel_mhz"] = round(ctx.clock_probe(160, 1024)["clock_mhz_median"], 1)

    text = json.dumps(res, indent=1)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
