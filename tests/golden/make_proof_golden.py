"""Writes tests/golden/proof_fib8_fs.bin and .npz (needs a GPU): the FibonacciAir n = 8 proof with
publics (0, 1, 21), SRS alpha = 12345 (max_degree 1024), Fiat-Shamir with the challenger
Perm::new_from_rng(4, 22, SmallRng(1)) and the per-column opening -- the constants of
tests/test_gpu_air_program.py -- as Proof.to_bytes writes it, next to the arrays prove_native returned
(tests/mirror_proofio.py's layout, plus the six shape fields).

    python tests/golden/make_proof_golden.py [out_dir]
"""

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]


def main(out_dir: Path):
    import torch

    import mirror_lookup as ML
    import mirror_proofio as M
    from airs import FibonacciAir
    from oracle import pyoracle as O
    from oracle.smallrng import SmallRng, poseidon2_new_from_rng
    from plonky3_eon_amd import Context
    from plonky3_eon_amd.air import AirProgram
    from plonky3_eon_amd.native import Challenger, NativeKzgPcs, Poseidon2Constants, prove_native

    ctx = Context(0)
    py = poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)
    lim = ML.lim
    ch = Challenger(Poseidon2Constants([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]],
                                       [[lim(v) for v in r] for r in py[2]]))
    trace = torch.from_numpy(np.ascontiguousarray(ML.to_limbs(O.fib_trace(0, 1, 8))).view(np.int64)).to("cuda:0")
    pcs = NativeKzgPcs(1024, 12345, ctx)
    proof = prove_native(AirProgram(FibonacciAir(), ctx), pcs, trace, None, None, challenger=ch,
                         public_values=[0, 1, 21])
    data = proof.to_bytes()
    shape, arrays = M.proof_arrays(proof)
    assert M.write(shape, arrays) == data
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "proof_fib8_fs.bin").write_bytes(data)
    np.savez(out_dir / "proof_fib8_fs.npz", **arrays, **{k: np.uint32(v) for k, v in shape.items()})
    print(f"wrote {len(data)} bytes and {len(arrays)} arrays to {out_dir}")


if __name__ == "__main__":
    main(Path(sys.argv[1]) if len(sys.argv) > 1 else HERE)
