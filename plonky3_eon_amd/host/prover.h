// prove_with_preprocessed (eon-uni-stark/src/prover.rs:28-512) over KzgPcs, as a C++ driver above
// eon.h, for the Poseidon2-AIR (fused quotient kernel) or any AIR given as a constraint program
// with public values and, optionally, preprocessed columns (the Some(preprocessed) branch:
// setup_preprocessed, eon-uni-stark/src/preprocessed.rs:47-94) and local LogUp lookups (the
// Some(permutation) branch, prover.rs:210-278, 317-319, 427-437): ZK off (KzgPcs::ZK = false,
// kzg/src/pcs.rs:216), Challenge = Fr; the challenges are inputs or sampled from a DuplexChallenger
// (SURVEY.md 8(f) N2).
#pragma once
#include "eon_prove.h"
#include "pcs.h"
#include "transcript.h"

namespace eon_host {

// get_log_quotient_degree (eon-uni-stark/src/symbolic_builder.rs:15-43), ZK off
uint32_t log_quotient_degree(uint32_t max_constraint_degree);

struct Proof {
    std::vector<eon_g1_affine> trace_commit;        // [W]
    std::vector<eon_g1_affine> quotient_commit;     // [C]
    std::vector<eon_fr> trace_opened[2];            // at zeta, zeta * h: [W] each
    std::vector<eon_g1_affine> trace_witnesses[2];  // [W] each
    std::vector<eon_fr> quotient_opened;            // [C]
    std::vector<eon_g1_affine> quotient_witnesses;  // [C]
    uint32_t degree_bits = 0;
    double stage_ms[EON_STAGES] = {};
    Fr alpha, zeta;  // the challenges used
    // with preprocessed columns (proof.rs opened_values.preprocessed_local / _next; the commitment
    // is the setup's, carried for the caller's convenience)
    std::vector<eon_g1_affine> pre_commit;        // [Wp]
    std::vector<eon_fr> pre_opened[2];            // at zeta, zeta * h: [Wp] each
    std::vector<eon_g1_affine> pre_witnesses[2];  // [Wp] each
    // with lookups (proof.rs commitments.permutation, opened_values.permutation_local / _next)
    std::vector<Fr> perm_challenges;               // [2 Wq], the challenges used
    std::vector<eon_g1_affine> perm_commit;        // [Wq]
    std::vector<eon_fr> perm_opened[2];            // at zeta, zeta * h: [Wq] each
    std::vector<eon_g1_affine> perm_witnesses[2];  // [Wq] each
};

// What a program with lookups needs beyond the plain prove: the preprocessed trace on the trace
// domain (device, height x Wp; what air.preprocessed_trace() returns next to the committed data,
// prover.rs:220-224), required when a lookup tuple reads a preprocessed column, and the permutation
// challenges when they are given rather than sampled (host, 2 Wq).
struct LookupInputs {
    const eon_fr* pre_trace = nullptr;
    const eon_fr* challenges = nullptr;
};

// PreprocessedProverData (preprocessed.rs:12-24): the preprocessed trace committed once per
// AIR / degree (KzgPcs::commit on the natural domain) and reused by every prove.
struct Preprocessed {
    const KzgPcs* pcs = nullptr;  // the pcs it was committed with
    uint32_t width = 0, degree_bits = 0;
    std::vector<eon_g1_affine> commitment;  // [width]
    std::vector<MatrixProverData> data;     // one matrix: evaluations, coefficients, prepared digits
};

// setup_preprocessed (preprocessed.rs:47-94): `pre_trace` is height x width on device and is
// copied (it need not outlive the call).  width == 0 is EON_E_SHAPE (the reference returns None).
std::unique_ptr<Preprocessed> setup_preprocessed(KzgPcs& pcs, const eon_fr* pre_trace, uint64_t height,
                                                 uint32_t width);

// The constraint check of the reference's debug builds (prover.rs:252-262, check_constraints.rs):
// when a prove is given one, eon_check_constraints_dev runs on the trace, the preprocessed trace,
// the permutation trace and the challenges after the permutation trace is generated and before
// alpha is sampled; `report` is filled either way, and a failure throws EON_E_CONSTRAINT.
struct ConstraintCheck {
    eon_constraint_report report{};
};

// The batched opening mode (EON_OPENING_BATCHED): when a prove is given one, the open stage is
// KzgPcs::open_batched -- one witness per (matrix, point), every witness vector of the Proof then
// has ONE entry per point -- and no lane sharding (EON_E_ARG).  Claims are numbered in the round
// order: trace zeta, trace zeta h; [permutation zeta, zeta h]; chunk 0..C-1 at zeta; [preprocessed
// zeta, zeta h].  With a challenger the transcript goes on after zeta: every opened value in claim
// order, column by column; gamma sampled; the K witnesses in claim order (observe_g1); delta
// sampled -- the verifier does the same, so both challengers end in the same state.  Without one,
// `gamma` is an input (have_gamma; missing is EON_E_ARG) and delta is the verifier's alone.
struct BatchedOpening {
    bool have_gamma = false;
    Fr gamma = Fr::zero();
    Fr gamma_used = Fr::zero(), delta_used = Fr::zero();  // out; delta only with a challenger
};

// The AIR being proved: the fused Poseidon2-AIR kernel (lane-shardable), or a generic constraint
// program compiled from get_symbolic_constraints (eon_air_program) with its public values.
struct AirRef {
    const eon_p2air* p2 = nullptr;
    const eon_air_program* prog = nullptr;
    const eon_fr* publics = nullptr;
    uint32_t n_public = 0;
    uint32_t width() const;
};

// `trace`: this rank's height x width(air) device trace.  With `shard` (world > 1) every rank
// returns the full proof: of the Poseidon2-AIR the AIR is the rank's lane range; of a program
// `trace` is the rank's height x wl column range (eon_shard_column_range) of the program's full
// width (prover.cpp: column sharding; main trace and public values only -- preprocessed columns,
// lookups, the constraint check and the batched opening are EON_E_ARG with a collective).  With `challenger`, alpha
// and zeta are sampled from it (prover.rs:196-208, 300, 373, 416) and the inputs are ignored.
// max_constraint_degree is the Poseidon2-AIR's (3); a program carries its own.  `preprocessed`
// (programs only, no sharding) is required exactly when the program has preprocessed columns: it is
// observed after the trace commitment (prover.rs:196-208), extended to the quotient domain for the
// constraints (:321-322) and opened at {zeta, zeta h} in a third round (:426-439).  `lookups`
// (programs only, no sharding) is required exactly when the program has permutation columns: the
// 2 Wq challenges are sampled after the public values (:214-216), generate_permutation runs on the
// device (:238-245), its trace is committed on the trace domain and observed (:270-273) before
// alpha (:300), extended next to the trace (:317-319) and opened at {zeta, zeta h} in the round
// after the trace's (:427-437).  `check` (programs only; null = off, the prove is then launch for
// launch what it is without it): see ConstraintCheck; its time is counted in EON_STAGE_TRACE_LDE.
// `batched` (null = the per-column opening, byte for byte and launch for launch what it is without
// it): see BatchedOpening.
Proof prove(KzgPcs& pcs, const AirRef& air, const eon_fr* trace, uint64_t height, const Fr& alpha,
            const Fr& zeta, uint32_t max_constraint_degree, const eon_collective* shard,
            DuplexChallenger* challenger = nullptr, const Preprocessed* preprocessed = nullptr,
            const LookupInputs* lookups = nullptr, ConstraintCheck* check = nullptr,
            BatchedOpening* batched = nullptr);

}  // namespace eon_host
