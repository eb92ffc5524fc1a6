"""plonky3_eon_amd -- MI355X-native prover hot path for the plonky3-eon BN254/KZG stack.

Kernels live in libeonhip.so (csrc/, C ABI include/eon.h); this package is the thin host-side
mirror of the reference's interfaces over that ABI:

* ``dft``   -- TwoAdicSubgroupDft<Fr> (Radix2Dit / Radix2DitParallel), dft/src/traits.rs
* ``field`` -- Fr value formatting for the ABI
* ``mmcs``  -- KzgMmcs, Mmcs<Fr> over the KZG SRS, kzg/src/mmcs.rs
* ``srs``   -- Srs, a supplied StructuredReferenceString (kzg/src/params.rs): container, device
               decompression and validation; native.NativeKzgPcs.from_srs is KzgPcs::from_srs
* ``keccak`` -- KeccakAir, keccak-air/src/air.rs (device trace generation, symbolic constraints)
* ``blake3`` -- Blake3Air, blake3-air/src/air.rs (device trace generation, symbolic constraints)

There is no CPU fallback: importing an entry point loads libeonhip.so and raises if it is absent.
"""

from . import _lib  # noqa: F401
from .dft import Context, Radix2Dit, Radix2DitParallel, BitReversedMatrix, default_context  # noqa: F401
from ._lib import EonError  # noqa: F401
from .proof import VerificationError  # noqa: F401  (native.verify_native's rejection)
from .mmcs import DegreeTooLarge, KzgMmcs, ProofShapeMismatch  # noqa: F401  (kzg/src/mmcs.rs)
from .srs import Srs, SrsError  # noqa: F401  (kzg/src/params.rs StructuredReferenceString)
from .keccak import KeccakAir  # noqa: F401  (keccak-air/src/air.rs)
from .blake3 import Blake3Air  # noqa: F401  (blake3-air/src/air.rs)

__all__ = ["Context", "Radix2Dit", "Radix2DitParallel", "BitReversedMatrix", "default_context", "EonError",
           "VerificationError", "KzgMmcs", "DegreeTooLarge", "ProofShapeMismatch", "Srs", "SrsError", "KeccakAir",
           "Blake3Air"]
