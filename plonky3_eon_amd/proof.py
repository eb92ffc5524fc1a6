"""The proof the native driver returns (libeonprove.so, native.prove_native), in the reference's
shape: eon-uni-stark/src/proof.rs:19-44 (commitments, opened values, opening proof, degree bits)
with KzgPcs's per-column witnesses (kzg/src/pcs.rs:289-335).

``Proof.to_bytes`` / ``from_bytes`` / ``save`` / ``load`` are the proof container of
include/eon_prove.h ("proof bytes": eon_proof_serialize / eon_proof_deserialize).  The bytes hold the
commitments, opened values and witnesses; the preprocessed commitment (the verifier key's), every
challenge and the timings are not in them, so a loaded proof is verified with a challenger
(native.verify_native_bytes)."""

from __future__ import annotations

from dataclasses import dataclass, field


@dataclass
class Opened:
    values: list = field(default_factory=list)     # [matrix][point] -> (width, 4) u64 Fr
    witnesses: list = field(default_factory=list)  # [matrix][point] -> (width, 8) u64 G1


@dataclass
class Proof:
    """eon-uni-stark/src/proof.rs:19-44 (commitments, opened values, opening proof, degree bits)."""

    trace_commit: object
    quotient_commit: object
    opened: object
    degree_bits: int
    timings_ms: dict = field(default_factory=dict)
    alpha: int | None = None  # the challenges used (canonical ints)
    zeta: int | None = None
    # with preprocessed columns: the setup's commitment [(Wp, 8)]; their openings are opened[2]
    preprocessed_commit: object = None
    # with lookups: the permutation trace's commitment [(Wq, 8)] and the 2 Wq challenges used
    # (canonical ints); `opened` follows the reference's rounds (prover.rs:426-439): trace,
    # permutation, quotient chunks, preprocessed
    permutation_commit: object = None
    permutation_challenges: list | None = None
    # the opening mode: "per_column" (the reference's KzgProof: one witness per column and point) or
    # "batched" (one witness per matrix and point: opened[r].witnesses[m][t] is then (1, 8)), with the
    # opening challenges used (canonical ints; delta is None after a prove with fixed challenges
    # that was given none)
    opening: str = "per_column"
    gamma: int | None = None
    delta: int | None = None

    def to_bytes(self) -> bytes:
        """The proof container (eon_proof_serialize): host only, no GPU needed."""
        from .native import proof_to_bytes

        return proof_to_bytes(self)

    @classmethod
    def from_bytes(cls, data, ctx=None) -> "Proof":
        """eon_proof_deserialize: every opened value checked < r, every point decompressed and
        checked on the device in one call.  Raises ProofFormatError(reason, section, index).  The
        loaded proof has preprocessed_commit None and every challenge None."""
        from .native import proof_from_bytes

        return proof_from_bytes(data, ctx)

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def load(cls, path, ctx=None) -> "Proof":
        with open(path, "rb") as f:
            return cls.from_bytes(f.read(), ctx)


class ProofFormatError(Exception):
    """Proof bytes that do not deserialise (EON_E_FORMAT).  Not a VerificationError: the reference
    fails in serde before its verifier runs.  `reason` is one of REASONS, `section` one of SECTIONS
    ("HEADER" for the header's reasons) and `index` the element's index within that section."""

    REASONS = ["OK", "MAGIC", "VERSION", "FLAGS", "LENGTH", "FR_NOT_CANONICAL", "G1_ENCODING", "G1_NOT_CANONICAL",
               "G1_NOT_ON_CURVE"]
    SECTIONS = ["HEADER", "TRACE_COMMIT", "PERMUTATION_COMMIT", "QUOTIENT_COMMIT", "TRACE_LOCAL", "TRACE_NEXT",
                "PERMUTATION_LOCAL", "PERMUTATION_NEXT", "PREPROCESSED_LOCAL", "PREPROCESSED_NEXT",
                "QUOTIENT_OPENED", "TRACE_WITNESS_ZETA", "TRACE_WITNESS_NEXT", "PERMUTATION_WITNESS_ZETA",
                "PERMUTATION_WITNESS_NEXT", "QUOTIENT_WITNESS", "PREPROCESSED_WITNESS_ZETA",
                "PREPROCESSED_WITNESS_NEXT"]

    def __init__(self, reason, section=0, index: int = 0):
        self.reason = self.REASONS[reason] if isinstance(reason, int) else reason
        self.section = self.SECTIONS[section] if isinstance(section, int) else section
        self.index = int(index)
        where = "" if self.section == "HEADER" else f" at {self.section}[{self.index}]"
        super().__init__(f"proof bytes rejected: {self.reason}{where}")


class VerificationError(Exception):
    """native.verify_native rejected a proof.  `kind` names the reference's VerificationError
    variant (eon-uni-stark/src/verifier.rs:504-526): "InvalidProofShape", "InvalidOpeningArgument" or
    "OodEvaluationMismatch"."""

    KINDS = {1: "InvalidProofShape", 2: "InvalidOpeningArgument", 3: "OodEvaluationMismatch"}

    def __init__(self, kind: str, detail: str = ""):
        super().__init__(f"{kind}: {detail}" if detail else kind)
        self.kind = kind
        self.detail = detail


def log_quotient_degree(max_constraint_degree: int) -> int:
    """get_log_quotient_degree (eon-uni-stark/src/symbolic_builder.rs:15-43), ZK off."""
    d = max(max_constraint_degree, 2) - 1
    return (d - 1).bit_length()
