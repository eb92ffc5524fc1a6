#!/usr/bin/env python3
"""Times the Keccak-AIR witness generation (eon_keccak_generate_trace_dev, a pure-store kernel) on
one GPU against a plain device fill of the same byte count in the same process, and prints one JSON
line: milliseconds (HIP events, median after a warm-up), GB/s, the ratio to the fill and the
in-kernel clock of eon_diag_clock_probe right after, as bench.py reports it.  With --program it also
compiles the Keccak-AIR's generic program and reports its statistics (instructions, registers, the
register file plan_regs picks) and the time of quotient_values on a random LDE of the trace height.

    python tools/bench_keccak_trace.py [--hashes 682] [--steps 10] [--warmup 3] [--program]
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hashes", type=int, default=682)  # 16,384 rows, 1.38 GB
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--program", action="store_true", help="also: AirProgram statistics and quotient_values")
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Context, KeccakAir
    from plonky3_eon_amd.keccak import NUM_KECCAK_COLS, keccak_air_rows

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this is a measurement, it does not fall back")
    ctx = Context(0)
    air = KeccakAir(ctx)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    inputs = torch.randint(-(1 << 63), (1 << 63) - 1, (args.hashes, 25), dtype=torch.int64, device="cuda:0", generator=g)
    rows = keccak_air_rows(args.hashes)
    nbytes = rows * NUM_KECCAK_COLS * 32
    out = torch.empty((rows, NUM_KECCAK_COLS, 4), dtype=torch.int64, device="cuda:0")

    import ctypes

    def generate():
        ctx.check(ctx.lib.eon_keccak_generate_trace_dev(ctx.handle, ctypes.c_void_p(inputs.data_ptr()), args.hashes,
                                                        ctypes.c_void_p(out.data_ptr()), rows))

    def fill():
        out.fill_(0x0123456789ABCDEF)

    ctx.set_stream(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ms = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
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
    assert torch.equal(air.generate_trace(inputs), out)  # the timed call is KeccakAir.generate_trace's
    fill_ms = fill_a + fill_b
    clock = ctx.clock_probe(160, 1024)
    med_g, med_f = statistics.median(gen_ms), statistics.median(fill_ms)
    res = {"workload": "keccak_trace", "n_hashes": args.hashes, "rows": rows, "bytes": nbytes,
           "generate_ms": [round(x, 3) for x in gen_ms], "generate_ms_median": round(med_g, 3),
           "generate_gb_s": round(nbytes / med_g / 1e6, 1),
           "fill_ms": [round(x, 3) for x in fill_ms], "fill_ms_median": round(med_f, 3),
           "fill_gb_s": round(nbytes / med_f / 1e6, 1),
           "generate_over_fill_time": round(med_g / med_f, 3),
           "gpu_clock_inkernel_mhz": round(clock["clock_mhz_median"], 1)}

    if args.program:
        from plonky3_eon_amd.air import AirProgram

        t0 = time.perf_counter()
        prog = AirProgram(air, ctx)
        res["program_create_s"] = round(time.perf_counter() - t0, 2)
        res["program"] = dict(prog.stats, dag_nodes=prog.num_nodes)
        log_n = rows.bit_length() - 1
        log_qd = prog.log_quotient_degree()
        q = rows << log_qd
        regs = max(0, prog.stats["num_registers"] - 2) * 36  # bytes per thread outside the two VGPR registers
        res["program"]["register_bytes_per_thread"] = regs
        block = 256  # plan_regs (csrc/air_program.hip): halve the block while it needs more than 64 KB of LDS
        while block > 64 and block * regs > 64 * 1024:
            block //= 2
        res["program"]["register_file"] = f"lds, {block}-thread blocks" if block * regs <= 160 * 1024 else "global"
        hi = torch.randint(0, 0x30644E72E131A029, (q, NUM_KECCAK_COLS, 1), dtype=torch.int64, device="cuda:0", generator=g)
        lo = torch.randint(-(1 << 63), (1 << 63) - 1, (q, NUM_KECCAK_COLS, 3), dtype=torch.int64, device="cuda:0",
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
