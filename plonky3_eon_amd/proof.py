"""The proof the native driver returns (libeonprove.so, native.prove_native), in the reference's
shape: eon-uni-stark/src/proof.rs:19-44 (commitments, opened values, opening proof, degree bits)
with KzgPcs's per-column witnesses (kzg/src/pcs.rs:289-335)."""

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
