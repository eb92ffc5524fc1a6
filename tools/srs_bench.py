#!/usr/bin/env python3
"""Times loading a supplied SRS on one GPU and prints one JSON line: NativeKzgPcs.from_srs over
n compressed G1 powers (eon_kzg_pcs_create_from_srs_bytes, structure check included), its four device
steps on their own -- eon_g1_decompress_dev, eon_g1_validate_dev, eon_msm_bases_create_dev with
EON_MSM_PRECOMPUTE, eon_kzg_srs_check -- and eon_kzg_pcs_create from alpha beside it, in the same
process, with the in-kernel clock of eon_diag_clock_probe right after, as bench.py reports it.
Medians over --steps runs after --warmup.

    python tools/srs_bench.py [--n 131073] [--steps 5] [--warmup 2]
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
    ap.add_argument("--n", type=int, default=(1 << 17) + 1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    from plonky3_eon_amd import Context, _lib
    from plonky3_eon_amd.field import fr_to_abi
    from plonky3_eon_amd.msm import MsmBases
    from plonky3_eon_amd.native import NativeKzgPcs
    from plonky3_eon_amd.srs import Srs, check_report

    ctx = Context(0)
    n, alpha, rho = args.n, 12345, 0x1234567890ABCDEF1234567890ABCDEF
    srs = Srs.unsafe(n - 1, alpha, ctx).compress()
    dbytes = torch.frombuffer(bytearray(srs.g1_bytes), dtype=torch.uint8).to("cuda:0")
    dpts = torch.zeros((n, 8), dtype=torch.int64, device="cuda:0")
    g2 = np.ascontiguousarray(srs.g2_alpha)
    r = fr_to_abi(rho)
    torch.cuda.synchronize()
    ctx.set_stream(None)

    def timed(fn):
        out = []
        for i in range(args.warmup + args.steps):
            ctx.synchronize()
            t0 = time.perf_counter()
            keep = fn()
            ctx.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
            if hasattr(keep, "close"):
                keep.close()
        return round(statistics.median(out[args.warmup:]), 3)

    def decompress():
        rep = _lib.eon_srs_report()
        check_report(ctx, ctx.lib.eon_g1_decompress_dev(ctx.handle, ctypes.c_void_p(dbytes.data_ptr()), n,
                                                        ctypes.c_void_p(dpts.data_ptr()), ctypes.byref(rep)), rep)

    def validate():
        rep = _lib.eon_srs_report()
        check_report(ctx, ctx.lib.eon_g1_validate_dev(ctx.handle, ctypes.c_void_p(dpts.data_ptr()), n,
                                                      ctypes.byref(rep)), rep)

    def table():
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.eon_msm_bases_create_dev(ctx.handle, ctypes.c_void_p(dpts.data_ptr()), n,
                                                   _lib.EON_MSM_PRECOMPUTE, ctypes.byref(h)))
        return MsmBases._from_handle(h, n, ctx)

    res = {"n": n, "steps": args.steps, "warmup": args.warmup}
    res["decompress_ms"] = timed(decompress)
    res["validate_ms"] = timed(validate)
    res["table_build_ms"] = timed(table)
    bases = table()

    def structure():
        rep = _lib.eon_srs_report()
        check_report(ctx, ctx.lib.eon_kzg_srs_check(ctx.handle, bases._h, n, g2.ctypes.data_as(ctypes.c_void_p),
                                                    ctypes.byref(r), ctypes.byref(rep)), rep)

    res["structure_check_ms"] = timed(structure)
    bases.close()
    res["from_srs_bytes_ms"] = timed(lambda: NativeKzgPcs.from_srs(srs, rho=rho, ctx=ctx))
    res["from_srs_bytes_trusted_ms"] = timed(lambda: NativeKzgPcs.from_srs(srs, validate=False, ctx=ctx))
    res["create_from_alpha_ms"] = timed(lambda: NativeKzgPcs(n - 1, alpha, ctx))
    res["gpu_clock_inkernel_mhz"] = round(ctx.clock_probe(160, 1024)["clock_mhz_median"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
