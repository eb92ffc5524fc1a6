#!/usr/bin/env python3
"""Times the proof container at the headline shape on one GPU and prints one JSON line: the
configs[3] proof of bench.py (Poseidon2-AIR, VECTOR_LEN 8, 2^17 rows, Fiat-Shamir) under
--opening per_column|batched, then Proof.to_bytes (host only), Proof.from_bytes (one device
decompression of every point) and native.verify_native of the loaded proof with a fresh challenger.
With --srs-n it also times Srs.compress() of that many powers -- ONE eon_g1_compress call -- beside
the loop it replaced, eon_g1_to_bytes per point through ctypes, in the same process.  Medians over
--steps runs after --warmup, with the in-kernel clock of eon_diag_clock_probe right after, as bench.py
reports it.  A record, not a threshold.

    python tools/proofio_bench.py [--opening per_column] [--log-trace 17] [--vector-len 8]
                                  [--srs-n 131073] [--steps 5] [--warmup 2]
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
    ap.add_argument("--opening", choices=["per_column", "batched"], default="per_column")
    ap.add_argument("--log-trace", type=int, default=17)
    ap.add_argument("--vector-len", type=int, default=8)
    ap.add_argument("--srs-n", type=int, default=0, help="also time Srs.compress() of this many powers (0: skip)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    from bench import p2_constants_limbs, synthetic_fr
    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air
    from plonky3_eon_amd.native import (Challenger, NativeKzgPcs, Poseidon2Constants, g1_to_bytes, prove_native,
                                        verify_native)
    from plonky3_eon_amd.proof import Proof
    from plonky3_eon_amd.srs import Srs

    ctx = Context(0)

    def timed(fn):
        out = []
        for _ in range(args.warmup + args.steps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(out[args.warmup:]), 3)

    n, vl = 1 << args.log_trace, args.vector_len
    air = Poseidon2Air(*p2_constants_limbs(99), vl, ctx)
    prog = AirProgram(air, ctx)
    pcs = NativeKzgPcs(n, 12345, ctx)
    inputs = synthetic_fr(n * vl, 3, 5).reshape(-1, 3, 4)
    trace = air.generate_trace(torch.from_numpy(np.ascontiguousarray(inputs).view(np.int64)).to("cuda:0"))
    ch_consts = p2_constants_limbs(77)
    proof = prove_native(air, pcs, trace, None, None, challenger=Challenger(Poseidon2Constants(*ch_consts)),
                         opening=args.opening)
    data = proof.to_bytes()
    loaded = Proof.from_bytes(data, ctx)
    assert loaded.to_bytes() == data
    res = {"opening": args.opening, "log_trace": args.log_trace, "width": air.width, "proof_bytes": len(data),
           "steps": args.steps, "warmup": args.warmup}
    res["to_bytes_ms"] = timed(proof.to_bytes)
    res["from_bytes_ms"] = timed(lambda: Proof.from_bytes(data, ctx))
    res["verify_native_ms"] = timed(lambda: verify_native(prog, pcs, loaded,
                                                          challenger=Challenger(Poseidon2Constants(*ch_consts))))
    if args.srs_n:
        srs = Srs.unsafe(args.srs_n - 1, 12345, ctx)
        one_call = srs.compress(ctx).g1_bytes
        assert one_call == b"".join(g1_to_bytes(p) for p in srs.g1_powers)
        res["srs_n"] = args.srs_n
        res["srs_compress_ms"] = timed(lambda: srs.compress(ctx))
        res["srs_compress_per_point_loop_ms"] = timed(lambda: b"".join(g1_to_bytes(p) for p in srs.g1_powers))
    res["gpu_clock_inkernel_mhz"] = round(ctx.clock_probe(160, 1024)["clock_mhz_median"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
