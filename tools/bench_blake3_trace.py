#!/usr/bin/env python3
"""Times the Blake3-AIR witness generation (eon_blake3_generate_trace_dev, a pure-store kernel) on
one GPU against a plain device fill of the same byte count in the same process, and prints one JSON
line: milliseconds (HIP events, median after a warm-up), GB/s, the ratio to the fill and the
in-kernel clock of eon_diag_clock_probe right after, as bench.py reports it.

With --parts it also times small traces (--parts-rows) with 1, 2, 4, 8 and 16 workgroups per row
(eon_diag_blake3_trace_parts) next to the library's own choice: the measurement behind
auto_log_parts in csrc/blake3_air.hip.  With --program it compiles the Blake3-AIR's generic program
and reports its statistics (instructions, registers, the register file plan_regs picks) and the time
of quotient_values on a random LDE of --program-log-n trace rows.

    python tools/bench_blake3_trace.py [--rows 16384] [--steps 10] [--warmup 3] [--parts] [--program]
"""

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)  # 4.8 GB
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", action="store_true", help="also: small traces by workgroups per row")
    ap.add_argument("--parts-rows", type=int, nargs="*", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--program", action="store_true", help="also: AirProgram statistics and quotient_values")
    ap.add_argument("--program-log-n", type=int, default=12)
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Blake3Air, Context
    from plonky3_eon_amd.blake3 import NUM_BLAKE3_COLS

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this is a measurement, it does not fall back")
    ctx = Context(0)
    air = Blake3Air(ctx)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    rows = args.rows
    inputs = torch.randint(-(1 << 31), (1 << 31) - 1, (rows, 24), dtype=torch.int32, device="cuda:0", generator=g)
    nbytes = rows * NUM_BLAKE3_COLS * 32
    out = torch.empty((rows, NUM_BLAKE3_COLS, 4), dtype=torch.int64, device="cuda:0")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def generate(n=rows, parts=0):
        ctx.check(ctx.lib.eon_diag_blake3_trace_parts(ctx.handle, ctypes.c_void_p(inputs.data_ptr()), n,
                                                      ctypes.c_void_p(out.data_ptr()), n, parts))

    def fill():
        out.fill_(0x0123456789ABCDEF)

    def timed(fn, steps=args.steps, run_ahead=False):
        ms = []
        for i in range(args.warmup + steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if run_ahead:  # a short call: keep the device busy while the host enqueues both events and the call
                out[-min(rows, 1024):].fill_(0)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        return ms

    # alternate the two, so that a drift of the clock or a neighbour's load reaches both
    fill_a = timed(fill)
    gen_ms = timed(generate)
    fill_b = timed(fill)
    generate()
    assert torch.equal(air.generate_trace(inputs), out)  # parts = 0 is Blake3Air.generate_trace's call
    fill_ms = fill_a + fill_b
    clock = ctx.clock_probe(160, 1024)
    med_g, med_f = statistics.median(gen_ms), statistics.median(fill_ms)
    res = {"workload": "blake3_trace", "rows": rows, "bytes": nbytes,
           "generate_ms": [round(x, 3) for x in gen_ms], "generate_ms_median": round(med_g, 3),
           "generate_gb_s": round(nbytes / med_g / 1e6, 1),
           "fill_ms": [round(x, 3) for x in fill_ms], "fill_ms_median": round(med_f, 3),
           "fill_gb_s": round(nbytes / med_f / 1e6, 1),
           "generate_over_fill_time": round(med_g / med_f, 3),
           "fill_over_generate_bandwidth": round(med_f / med_g, 3),
           "gpu_clock_inkernel_mhz": round(clock["clock_mhz_median"], 1)}

    if args.parts:
        # microseconds per call, median of 3 x steps; every variant twice, in turn
        table = {}
        for n in args.parts_rows:
            if n > rows or n & (n - 1):
                continue
            per = {p: [] for p in (0, 1, 2, 4, 8, 16)}
            for _ in range(2):
                for p in per:
                    per[p] += timed(lambda: generate(n, p), 3 * args.steps, run_ahead=True)
            table[n] = {("auto" if p == 0 else str(p)): round(statistics.median(v) * 1e3, 2) for p, v in per.items()}
        res["small_traces_us_by_parts"] = table

    if args.program:
        from plonky3_eon_amd.air import AirProgram

        del out
        torch.cuda.empty_cache()
        t0 = time.perf_counter()
        prog = AirProgram(air, ctx)
        res["program_create_s"] = round(time.perf_counter() - t0, 2)
        res["program"] = dict(prog.stats, dag_nodes=prog.num_nodes)
        log_n = args.program_log_n
        log_qd = prog.log_quotient_degree()
        q = 1 << (log_n + log_qd)
        regs = max(0, prog.stats["num_registers"] - 2) * 36  # bytes per thread outside the two VGPR registers
        res["program"]["register_bytes_per_thread"] = regs
        block = 256  # plan_regs (csrc/air_program.hip): halve the block while it needs more than 64 KB of LDS
        while block > 64 and block * regs > 64 * 1024:
            block //= 2
        res["program"]["register_file"] = f"lds, {block}-thread blocks" if block * regs <= 160 * 1024 else "global"
        hi = torch.randint(0, 0x30644E72E131A029, (q, NUM_BLAKE3_COLS, 1), dtype=torch.int64, device="cuda:0", generator=g)
        lo = torch.randint(-(1 << 63), (1 << 63) - 1, (q, NUM_BLAKE3_COLS, 3), dtype=torch.int64, device="cuda:0",
                           generator=g)
        lde = torch.cat([lo, hi], dim=2).contiguous()  # top limb below the modulus': canonical
        del lo, hi
        qms = []
        for i in range(1 + 3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            prog.quotient_values(lde, log_n, log_qd, 0x1234567890ABCDEF)
            ctx.synchronize()
            torch.cuda.synchronize()
            if i >= 1:
                qms.append((time.perf_counter() - t0) * 1e3)
        res["quotient_values"] = {"log_n": log_n, "log_qd": log_qd, "ms": [round(x, 2) for x in qms],
                                  "ms_median": round(statistics.median(qms), 2)}
        res["gpu_clock_inkernel_mhz_after_quotient"] = round(ctx.clock_probe(160, 1024)["clock_mhz_median"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
