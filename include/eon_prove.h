/*
 * eon_prove.h -- C ABI of the native prove driver (libeonprove.so), the host side ABOVE eon.h.
 *
 * The reference's prover is compiled Rust; its toolchain is absent here, so the orchestration is
 * C++ (plonky3_eon_amd/host/) calling only the eon.h entry points, with the reference's shapes:
 *   eon_kzg_pcs      KzgPcs (kzg/src/pcs.rs:143-402) with the test SRS init_srs_unsafe
 *                    (kzg/src/params.rs:123-139): commit / get_evaluations_on_domain /
 *                    commit_quotient / open of the Pcs trait (commit/src/pcs.rs:21-187)
 *   eon_prove_p2air  prove_with_preprocessed (eon-uni-stark/src/prover.rs:28-512) for the
 *                    Poseidon2-AIR: no preprocessed columns, no lookups,
 *                    ZK off, Challenge = Fr.  alpha and zeta are either inputs
 *                    (eon_prove_p2air) or sampled from the Fiat-Shamir transcript
 *                    (eon_prove_p2air_fs with an eon_challenger).
 *   eon_prove_air    the same for any AIR compiled into an eon_air_program (eon.h), with public
 *                    values (e.g. eon-uni-stark/tests/fib_air.rs's FibonacciAir)
 *   eon_preprocessed PreprocessedProverData (eon-uni-stark/src/preprocessed.rs:12-24) from
 *                    setup_preprocessed (:47-94), and eon_prove_air_pp, the Some(preprocessed)
 *                    branch of prove_with_preprocessed (prover.rs:58-88, 190-208, 321-322, 431)
 *   eon_prove_air_lk the Some(permutation) branch (prover.rs:210-278, 317-319, 427-437): local LogUp
 *                    lookups, the permutation trace generated on the device
 *   eon_verify_air   verify_with_preprocessed (eon-uni-stark/src/verifier.rs:244-502) for a proof of
 *                    any of the above: the verdict is the reference's Ok or VerificationError variant
 *   eon_challenger   DuplexChallenger<Fr, Poseidon2Bn254<3>, 3, 2>
 *                    (challenger/src/duplex_challenger.rs, bn254/src/poseidon2.rs) on the host.
 * Conventions are eon.h's: 0 / negative EON_E_* codes (the reference panics), host outputs,
 * device inputs, work on the context's stream.
 */
#ifndef EON_PROVE_H
#define EON_PROVE_H

#include <stdint.h>

#include "eon.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eon_kzg_pcs eon_kzg_pcs;

/* KzgPcs::new(max_degree, alpha): SRS g1_powers[0..=max_degree] generated and kept on device as
 * fixed-base MSM bases (alpha is a host pointer). */
int eon_kzg_pcs_create(eon_ctx* ctx, uint64_t max_degree, const eon_fr* srs_alpha, eon_kzg_pcs** out);
/* KzgPcs::from_srs(StructuredReferenceString) (kzg/src/pcs.rs:170-175): a prover and verifier over a
 * SUPPLIED SRS, without its trapdoor.  g1_powers = n host affine points (eon_kzg_pcs_create_from_srs)
 * or n x 32 compressed bytes, G1Affine::to_bytes each (eon_kzg_pcs_create_from_srs_bytes);
 * max_degree = n - 1 (n == 0 is EON_E_ARG); g2_alpha is kept as given and no alpha is known.  In
 * order: upload; per point, eon_g1_decompress_dev (bytes only) and eon_g1_validate_dev -- always, they
 * cost far less than the tables; eon_msm_bases_create_dev(EON_MSM_PRECOMPUTE); eon_kzg_srs_check with
 * `rho` (host, a nonzero canonical Fr the caller draws uniformly AFTER the SRS is fixed), unless flags
 * has EON_SRS_TRUSTED -- the caller vouches for the SRS (its own file, checked before), rho may then
 * be NULL and a table that is no SRS is accepted.  On a rejected SRS the call returns EON_E_SRS,
 * *report (eon.h) says why, nothing is kept and *out is untouched.  The device state of a handle made
 * from the powers of alpha is byte for byte that of eon_kzg_pcs_create(max_degree, alpha), so its
 * proofs are too. */
enum {
    EON_SRS_TRUSTED = 1
};
int eon_kzg_pcs_create_from_srs(eon_ctx* ctx, const eon_g1_affine* g1_powers, uint64_t n,
                                const eon_g2_affine* g2_alpha, uint32_t flags, const eon_fr* rho,
                                eon_kzg_pcs** out, eon_srs_report* report);
int eon_kzg_pcs_create_from_srs_bytes(eon_ctx* ctx, const uint8_t* g1_bytes, uint64_t n,
                                      const eon_g2_affine* g2_alpha, uint32_t flags, const eon_fr* rho,
                                      eon_kzg_pcs** out, eon_srs_report* report);
/* The verifier's half: max_degree and g2_alpha, no G1 table (the verifier reads neither).
 * eon_verify_air[_fs] work on the handle; every prove and setup entry point returns EON_E_ARG and
 * eon_kzg_pcs_last_error says the handle is verifier-only.  g2_alpha is taken as given: it comes from
 * an SRS that eon_kzg_pcs_create_from_srs (or the party that made it) has checked. */
int eon_kzg_pcs_create_verifier(eon_ctx* ctx, uint64_t max_degree, const eon_g2_affine* g2_alpha,
                                eon_kzg_pcs** out);
void eon_kzg_pcs_destroy(eon_kzg_pcs* pcs);
/* message of the last failing call on this pcs (driver-side errors and eon.h errors) */
const char* eon_kzg_pcs_last_error(const eon_kzg_pcs* pcs);

/* ---- check_constraints in the prove (eon-uni-stark/src/prover.rs:252-262) -----------------------
 * The reference runs check_constraints (check_constraints.rs:22-101) in every debug build, right
 * after the permutation trace is generated and before alpha is sampled.  This switch is that
 * cfg(debug_assertions): off by default, and with it off every prove is byte for byte and launch
 * for launch what it is without this surface.  With it on, eon_prove_air, _pp and _lk (fixed
 * challenges and _fs alike) run eon_check_constraints_dev at that point -- after
 * generate_permutation, before the permutation commitment and alpha -- on the trace, the
 * preprocessed trace (pre_trace of the _lk forms when given; otherwise the device copy of the
 * matrix that eon_setup_preprocessed already keeps next to its coefficients, so nothing is
 * recomputed), the device permutation trace and the permutation challenges.  Its time is counted
 * in EON_STAGE_TRACE_LDE.  On a failing constraint the prove returns EON_E_CONSTRAINT (eon.h),
 * eon_kzg_pcs_last_error reads
 *   "Constraint failed at row R: constraint K of N, expected zero, got 0x<canonical value, 64 hex>"
 * (the reference's panic, check_constraints.rs:165-173, plus the constraint), no field of the proof
 * is written, and in the _fs forms the challenger is left as advanced so far: log_ext_degree,
 * log_degree, the preprocessed width, the trace and preprocessed commitments and the public values
 * observed, the permutation challenges sampled; the permutation commitment is not observed and alpha
 * is not sampled.  eon_kzg_pcs_last_constraint_report copies the report of the last eon_prove_air*
 * call that ran with the switch on (failures == 0 when it passed, or when the prove failed before
 * the check).  eon_prove_p2air[_fs] (the fused kernel) has no program and ignores the switch: check
 * a Poseidon2 trace by compiling the same AIR into an eon_air_program (AirProgram(Poseidon2Air))
 * and calling eon_check_constraints_dev or eon_prove_air. */
int eon_kzg_pcs_set_check_constraints(eon_kzg_pcs* pcs, int enable);
int eon_kzg_pcs_check_constraints(const eon_kzg_pcs* pcs); /* 1 / 0 */
int eon_kzg_pcs_last_constraint_report(const eon_kzg_pcs* pcs, eon_constraint_report* out);

/* ---- the opening mode ---------------------------------------------------------------------------
 * EON_OPENING_PER_COLUMN (the default) is the reference's KzgPcs::open: one witness per opened
 * column and point, and a verify that multiplies all pairing checks WITHOUT random weights, as the
 * reference's verify_batch does (kzg/src/util.rs:245-292) -- restated faithfully, and as a batch
 * check not sound.  With the mode at its default every prove and verify is byte for byte and launch
 * for launch what it is without this surface.
 *
 * EON_OPENING_BATCHED is the standard batched KZG opening, NOT the reference's KzgProof: a matrix's
 * columns are folded with powers of a challenge gamma, F = sum_j gamma^j f_j
 * (eon_fr_fold_columns_dev), F is opened once per point, W = commit_column(quotient_and_eval(F, z).0),
 * and the claims are combined with a second challenge delta.  Commitments and opened values are laid
 * out as in the per-column mode; the witness arrays are compact: trace_witnesses,
 * permutation_witnesses and preprocessed_witnesses hold [2] points (zeta, zeta h) and
 * quotient_witnesses stays [C] (a width-1 matrix is its own fold: those witnesses equal the
 * per-column ones bit for bit).  Every unsharded eon_prove_* entry writes them so; a collective with
 * world > 1 in this mode is EON_E_ARG.
 *   Claims i = 0..K-1, in the reference's round order: trace zeta, trace zeta h; [permutation zeta,
 *   zeta h]; chunk 0..C-1 at zeta; [preprocessed zeta, zeta h].
 *   Transcript (_fs forms): unchanged up to zeta -- alpha, zeta, all commitments and all opened values
 *   equal the per-column proof's; then every opened value is observed in claim order, column by
 *   column; gamma is sampled; the K witnesses are observed in claim order (observe_g1); delta is
 *   sampled.  Prover and verifier both do this: their challengers end in the same state.
 *   Fixed-challenge forms take gamma and delta from eon_kzg_pcs_set_opening_challenges (host,
 *   canonical Fr, copied; NULL clears one): the prover needs gamma, the verifier both; a missing one
 *   is EON_E_ARG.
 *   eon_verify_air[_fs]: shape checks as in the per-column mode; per claim C_i = sum_j gamma^j C_(m,j)
 *   and v_i = sum_j gamma^j v_(i,j); ONE eon_kzg_verify_batch on (delta^i C_i, delta^i W_i,
 *   delta^i v_i, z_i), i.e. prod_i e(delta^i (C_i - v_i G1), G2) e(-delta^i W_i, g2_alpha - z_i G2)
 *   = 1, every scaled point from ONE variable-base column MSM (eon_msm_g1_columns) over the proof's
 *   commitments and witnesses.  A failure, or a commitment or
 *   witness that is no curve point, is EON_VERIFY_INVALID_OPENING_ARGUMENT.
 * eon_kzg_pcs_last_opening_challenges: the gamma and delta of the last batched prove or verify on
 * this pcs (either pointer may be NULL; a fixed-challenge prove reports the delta that was set, or
 * zero); EON_E_ARG when none has run. */
enum { EON_OPENING_PER_COLUMN = 0, EON_OPENING_BATCHED = 1 };
int eon_kzg_pcs_set_opening(eon_kzg_pcs* pcs, uint32_t mode);
int eon_kzg_pcs_opening(const eon_kzg_pcs* pcs); /* the mode */
int eon_kzg_pcs_set_opening_challenges(eon_kzg_pcs* pcs, const eon_fr* gamma, const eon_fr* delta);
int eon_kzg_pcs_last_opening_challenges(const eon_kzg_pcs* pcs, eon_fr* gamma, eon_fr* delta);

/* Lane-sharded prove: this rank's share of VECTOR_LEN and an all-gather over
 * DEVICE buffers (eon_collective, declared in eon.h). */

/* An RCCL (NCCL API over xGMI) all-gather for eon_collective: rank 0 creates the unique id
 * (128 bytes), every rank receives it out of band (e.g. torch.distributed) and initialises its
 * communicator on the current HIP device (the context's). */
int eon_rccl_unique_id(uint8_t id[128]);
int eon_rccl_collective_init(uint32_t rank, uint32_t world, const uint8_t id[128], eon_collective* out);
/* What the communicator itself reports (evidence that RCCL saw `world` ranks on distinct GPUs):
 * ncclCommCount, ncclCommUserRank, ncclCommCuDevice and that device's PCI bus id (NUL-terminated,
 * at most pci_len bytes); any output pointer may be NULL.  EON_E_ARG if `coll` is not an RCCL
 * collective of eon_rccl_collective_init. */
int eon_rccl_collective_info(const eon_collective* coll, int32_t* count, int32_t* user_rank, int32_t* device,
                             char* pci_bus_id, uint32_t pci_len);
void eon_rccl_collective_finalize(eon_collective* coll);
/* The one-GPU proxy of rank `rank` in a `world`-rank lane-sharded prove (bench.py
 * --emulate-world): its all-gather writes this rank's block into every slot, its all-to-all
 * keeps every block, both as device copies on the given stream.  Results are NOT a valid
 * proof; the point is the rank's own work, including the full replicated transcript. */
int eon_emulated_collective_init(uint32_t rank, uint32_t world, eon_collective* out);

enum {
    EON_STAGE_COMMIT_TRACE = 0,    /* "commit to trace data" (prover.rs:186-187) */
    EON_STAGE_TRACE_LDE = 1,       /* get_evaluations_on_domain (prover.rs:315) */
    EON_STAGE_QUOTIENT = 2,        /* quotient_values (prover.rs:328-342) */
    EON_STAGE_EXCHANGE = 3,        /* sharded: all-gather + combine of partial quotients (lanes); the
                                      window all_to_all + the quotient blocks' all-gather (columns) */
    EON_STAGE_COMMIT_QUOTIENT = 4, /* "commit to quotient poly chunks" (prover.rs:371-372) */
    EON_STAGE_OPEN = 5,            /* "open" (prover.rs:424-442) */
    EON_STAGE_ASSEMBLE = 6,        /* sharded: all-gather of per-column results */
    EON_STAGES = 8
};

/* Proof fields (eon-uni-stark/src/proof.rs:19-44), caller-allocated host arrays; W is the FULL
 * trace width (164 * VECTOR_LEN over all ranks), C = 2^log_qd quotient chunks (2 for degree 3).
 * In the batched opening mode (EON_OPENING_BATCHED, above) trace_witnesses -- and the
 * preprocessed_witnesses / permutation_witnesses of the structs below -- hold [2] points, one per
 * opened point; every other array is as given here. */
typedef struct {
    eon_g1_affine* trace_commit;       /* [W] */
    eon_g1_affine* quotient_commit;    /* [C] */
    eon_fr* trace_opened;              /* [2][W]: values at zeta, zeta * h */
    eon_g1_affine* trace_witnesses;    /* [2][W] */
    eon_fr* quotient_opened;           /* [C]: chunk c at zeta */
    eon_g1_affine* quotient_witnesses; /* [C] */
    uint32_t degree_bits;              /* out: log2 of the trace height */
    double stage_ms[EON_STAGES];       /* out: host clock around each stage (device synchronized) */
} eon_proof;

/* prove: `trace` is this rank's (height x width(air)) trace on device; `alpha`, `zeta` host.
 * `shard` NULL = the whole AIR on this device.  max_constraint_degree = 3 for the Poseidon2-AIR
 * (log_qd = 1, get_log_quotient_degree, symbolic_builder.rs:15-43). */
int eon_prove_p2air(eon_kzg_pcs* pcs, const eon_p2air* air, const eon_fr* trace, uint64_t height,
                    const eon_fr* alpha, const eon_fr* zeta, uint32_t max_constraint_degree,
                    const eon_collective* shard, eon_proof* out);

/* ---- Fiat-Shamir transcript, host only ---------------------------------
 * Poseidon2Bn254<3>::permute_mut (poseidon2/src/lib.rs:107-111) of state[3] in place, with the
 * round constants of `perm` (the AIR's constant layout; the reference draws them with
 * Poseidon2::new_from_rng(2 * half_full_rounds, partial_rounds), lib.rs:66-74). */
int eon_poseidon2_bn254_permute(const eon_poseidon2_constants* perm, eon_fr state[3]);
/* G1Affine::to_bytes, the 32-byte compressed form KzgCommitment observation reads
 * (kzg/src/pcs.rs:417-436): canonical x little-endian, bit 7 of byte 31 = y odd, bit 6 =
 * identity.  halo2curves' encoding, absent here: parity unpinned. */
int eon_g1_to_bytes(const eon_g1_affine* point, uint8_t out[32]);

typedef struct eon_challenger eon_challenger;
/* DuplexChallenger::new(Poseidon2Bn254<3>) (duplex_challenger.rs:68-78): zero sponge state */
int eon_challenger_create(const eon_poseidon2_constants* perm, eon_challenger** out);
void eon_challenger_destroy(eon_challenger* ch);
/* observe(Fr) for each of values[0..n) (duplex_challenger.rs:111-121) */
int eon_challenger_observe(eon_challenger* ch, const eon_fr* values, uint64_t n);
/* observe(KzgCommitment) for one matrix's n column commitments (kzg/src/pcs.rs:417-436) */
int eon_challenger_observe_g1(eon_challenger* ch, const eon_g1_affine* points, uint64_t n);
/* sample() -> Fr = sample_algebra_element for Challenge = Fr (duplex_challenger.rs:185-200) */
int eon_challenger_sample(eon_challenger* ch, eon_fr* out);
/* the sponge state (3 Fr), for tests */
int eon_challenger_state(const eon_challenger* ch, eon_fr out[3]);

/* prove with the transcript of prove_with_preprocessed: observe log_ext_degree, log_degree, the
 * preprocessed width (0 here) and the trace commitment (prover.rs:196-202), sample alpha (:300),
 * observe the quotient commitment (:373), sample zeta (:416).  `challenger` is the config's
 * initialised challenger and is advanced as the reference's; alpha_out / zeta_out (host,
 * nullable) receive the sampled challenges.  Sharded: the trace commitments are all-gathered
 * before alpha so every rank observes the full transcript. */
int eon_prove_p2air_fs(eon_kzg_pcs* pcs, const eon_p2air* air, const eon_fr* trace, uint64_t height,
                       eon_challenger* challenger, uint32_t max_constraint_degree,
                       const eon_collective* shard, eon_proof* out, eon_fr* alpha_out, eon_fr* zeta_out);

/* prove_with_preprocessed (prover.rs:28-512) for ANY AIR given as an eon_air_program (eon.h: the
 * compiled get_symbolic_constraints DAG) with its public values (host, n_public Fr): the quotient
 * degree is the program's get_log_quotient_degree (prover.rs:150-157), C = 2^that chunks, the
 * public values are observed after the trace commitment (prover.rs:208) and read by the
 * constraints (Entry::Public).  No sharding.  The trace is height x width(prog) on device. */
int eon_prove_air(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                  const eon_fr* publics, uint32_t n_public, const eon_fr* alpha, const eon_fr* zeta,
                  eon_proof* out);
int eon_prove_air_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                     const eon_fr* publics, uint32_t n_public, eon_challenger* challenger, eon_proof* out,
                     eon_fr* alpha_out, eon_fr* zeta_out);

/* Column-sharded prove of a program over a process group: eon_prove_air[_fs] with
 * `shard` (world > 1; NULL or world <= 1 is eon_prove_air[_fs] itself).  Rank g owns the columns
 * [c0, c0 + wl) of eon_shard_column_range(width(prog), world, g) (eon.h): `trace` is ITS height x wl
 * slice on device, and it commits, extends and opens only those.  The trace commitments are
 * all-gathered so every rank observes the full transcript; the ranks exchange their extended columns
 * once as row blocks (eon_shard_pack_rows_dev, all_to_all, eon_shard_unpack_cols_dev), each
 * evaluates the quotient on its own rows (eon_quotient_values_rows_dev) and the blocks are
 * all-gathered; chunk c is then committed and opened by rank c % world, the opening bases are
 * sharded over the group, and the per-column records are all-gathered.  Every rank's `out` (arrays
 * of the FULL width W) is byte for byte the unsharded eon_prove_air[_fs] proof of the full trace.
 * The collective needs all_gather and all_to_all.  EON_E_ARG, decided alike on every rank before
 * the first collective call: world > W; a program with preprocessed columns or lookups; the
 * check_constraints switch; the batched opening mode.  stage_ms[EON_STAGE_EXCHANGE] holds both data
 * exchanges (the window and the quotient blocks). */
int eon_prove_air_sharded(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                          const eon_fr* publics, uint32_t n_public, const eon_fr* alpha, const eon_fr* zeta,
                          const eon_collective* shard, eon_proof* out);
int eon_prove_air_sharded_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                             const eon_fr* publics, uint32_t n_public, eon_challenger* challenger,
                             const eon_collective* shard, eon_proof* out, eon_fr* alpha_out, eon_fr* zeta_out);

/* ---- preprocessed columns (eon-uni-stark/src/preprocessed.rs) -------------------------------
 * eon_preprocessed is PreprocessedProverData (preprocessed.rs:12-24): the width, degree_bits, the
 * column commitments and the Pcs prover data (coefficients and their prepared MSM digits) of a
 * preprocessed trace committed once per AIR / degree and reused by every prove.  The verifier's
 * PreprocessedVerifierKey (:30-40) is (width, degree_bits, commitment): eon_preprocessed_info and
 * eon_preprocessed_commitment.
 *
 * eon_setup_preprocessed is setup_preprocessed (:47-94): KzgPcs::commit of `pre_trace` (device,
 * height x width, row-major) on natural_domain_for_degree(height) (:78-80).  The matrix is copied
 * and need not outlive the call.  width == 0 is EON_E_SHAPE (the reference returns None, :68-70,
 * and the caller proves without preprocessed data); height must be a power of two.  Destroy the
 * handle before its pcs. */
typedef struct eon_preprocessed eon_preprocessed;
int eon_setup_preprocessed(eon_kzg_pcs* pcs, const eon_fr* pre_trace, uint64_t height, uint32_t width,
                           eon_preprocessed** out);
void eon_preprocessed_destroy(eon_preprocessed* pp);
/* width and degree_bits (either pointer may be NULL) */
int eon_preprocessed_info(const eon_preprocessed* pp, uint32_t* width, uint32_t* degree_bits);
/* the column commitments, out[width] (host) */
int eon_preprocessed_commitment(const eon_preprocessed* pp, eon_g1_affine* out);

/* eon_proof plus the preprocessed openings (proof.rs opened_values.preprocessed_local / _next,
 * prover.rs:463-493); Wp = the preprocessed width.  The commitment is the setup's own (the
 * verifier takes it from its key, verifier.rs:165-235), copied here for convenience.  The three
 * arrays are untouched (and may be NULL) when the prove ran without preprocessed data. */
typedef struct {
    eon_proof base;
    eon_g1_affine* preprocessed_commit;    /* [Wp] */
    eon_fr* preprocessed_opened;           /* [2][Wp]: values at zeta, zeta * h */
    eon_g1_affine* preprocessed_witnesses; /* [2][Wp] */
} eon_proof_pp;

/* eon_prove_air / eon_prove_air_fs for a program with preprocessed columns
 * (eon_air_program_create_pp), in the reference's order: commit the trace; observe log_ext_degree,
 * log_degree, the preprocessed width Wp, the trace commitment, then the preprocessed commitment,
 * then the public values (prover.rs:196-208); alpha; get_evaluations_on_domain of the trace and of
 * the preprocessed data on the quotient domain (:315-322; the latter recomputed each prove, counted
 * in EON_STAGE_TRACE_LDE); quotient_values, commit_quotient, zeta; open the trace at
 * {zeta, zeta h}, the quotient chunks at {zeta}, the preprocessed data at {zeta, zeta h}
 * (:426-439).  The reference's asserts (prover.rs:58-88): pp's degree_bits != log2(height) or pp's
 * width != the program's preprocessed width is EON_E_SHAPE; a program with preprocessed columns
 * and pp == NULL is EON_E_ARG ("no PreprocessedProverData was provided"; eon_prove_air[_fs] answer
 * the same), as is a pp committed with another pcs.  A program without preprocessed columns and
 * pp == NULL proves exactly as eon_prove_air.  No sharding. */
int eon_prove_air_pp(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                     const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp, const eon_fr* alpha,
                     const eon_fr* zeta, eon_proof_pp* out);
int eon_prove_air_pp_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                        const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp,
                        eon_challenger* challenger, eon_proof_pp* out, eon_fr* alpha_out, eon_fr* zeta_out);

/* ---- LogUp lookups (lookup/src/logup.rs; eon-uni-stark/tests/lookup_air.rs) ---------------------
 * eon_proof_pp plus the permutation trace's commitment and openings (proof.rs
 * commitments.permutation, opened_values.permutation_local / _next); Wq = the program's permutation
 * width (one running-sum column per lookup).  The three arrays are untouched (and may be NULL) when
 * the program has no lookups. */
typedef struct {
    eon_proof_pp pp;
    eon_g1_affine* permutation_commit;    /* [Wq] */
    eon_fr* permutation_opened;           /* [2][Wq]: values at zeta, zeta * h */
    eon_g1_affine* permutation_witnesses; /* [2][Wq] */
} eon_proof_lk;

/* eon_prove_air_pp / eon_prove_air_pp_fs for a program with local lookups
 * (eon_air_program_create_lk with a lookup description), the Some(permutation) branch of
 * prove_with_preprocessed, in the reference's order: commit the trace; observe log_ext_degree,
 * log_degree, Wp, the trace commitment, the preprocessed commitment, the public values
 * (prover.rs:196-208); sample the 2 Wq permutation challenges (:214-216); generate_permutation on the
 * device (:238-245, eon_lookup_permutation_dev); commit the permutation trace on the trace domain
 * (:270) and observe its commitment (:273); alpha (:300); the trace, the permutation trace and the
 * preprocessed data on the quotient domain (:315-322); quotient_values, commit_quotient, zeta; open
 * the trace at {zeta, zeta h}, the permutation trace at {zeta, zeta h}, the quotient chunks at
 * {zeta}, the preprocessed data at {zeta, zeta h} (:426-439).  Generating, committing and extending
 * the permutation trace is counted in EON_STAGE_TRACE_LDE.
 *   pp         NULL exactly when the program has no preprocessed columns (as eon_prove_air_pp)
 *   pre_trace  the preprocessed trace on the trace domain (device, height x Wp), what the reference
 *              takes from air.preprocessed_trace() next to the committed data (:220-224): required
 *              when a lookup tuple reads a preprocessed column (EON_E_ARG otherwise), NULL when the
 *              program has no preprocessed columns.  It is NOT checked against pp's commitment: a
 *              proof made with another matrix does not verify.
 *   challenges (eon_prove_air_lk) the 2 Wq permutation challenges, host; n_challenges must be the
 *              program's count (EON_E_SHAPE)
 *   challenges_out (eon_prove_air_lk_fs; host, nullable) receives the sampled ones, 2 Wq Fr
 * A zero LogUp denominator on any row is EON_E_ARG (the reference panics).  A program without
 * lookups proves exactly as eon_prove_air_pp; eon_prove_air[_pp][_fs] answer EON_E_ARG to a program
 * with lookups.  Local lookups only: a global lookup spans several AIRs, and the reference's own
 * single-AIR verifier passes no lookup_data (verifier.rs:498).  No sharding. */
int eon_prove_air_lk(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                     const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp, const eon_fr* pre_trace,
                     const eon_fr* challenges, uint32_t n_challenges, const eon_fr* alpha, const eon_fr* zeta,
                     eon_proof_lk* out);
int eon_prove_air_lk_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                        const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp,
                        const eon_fr* pre_trace, eon_challenger* challenger, eon_proof_lk* out,
                        eon_fr* challenges_out, eon_fr* alpha_out, eon_fr* zeta_out);

/* ---- verify (eon-uni-stark/src/verifier.rs:244-502) ----------------------------------------------
 * verify_with_preprocessed for a proof of ANY eon_prove_* entry, in the reference's order:
 *   1. shapes: the preprocessed width against the verifier key (process_preprocessed_trace,
 *      verifier.rs:165-225), the key's degree_bits against the proof's (:272-277), the permutation
 *      part against the program (:330-352);
 *   2. the transcript (:355-397): observe degree_bits twice, the preprocessed width, the trace
 *      commitment, the KEY's preprocessed commitment, the public values; with a permutation
 *      commitment sample the 2 Wq permutation challenges and observe it; sample alpha, observe the
 *      quotient commitment, sample zeta;
 *   3. KzgPcs::verify (kzg/src/pcs.rs:337-401): ensure_supported, then every opening -- trace at
 *      {zeta, zeta h}, permutation at {zeta, zeta h}, quotient chunks at {zeta}, preprocessed at
 *      {zeta, zeta h} -- in ONE eon_kzg_verify_batch against g2_alpha = [srs_alpha] G2 (made once per
 *      pcs with eon_g2_mul);
 *   4. recompose_quotient_from_chunks (:30-70) on the host;
 *   5. verify_constraints (:77-160): eon_air_eval_at_point_dev (eon.h) on the opened values, and
 *      folded * inv_vanishing == quotient(zeta).
 * A failure of step 3 is reported before step 5 is looked at.
 *   proof      eon_proof_lk as the superset of the three proof structs: the preprocessed arrays are
 *              NULL when the proof has no preprocessed part (preprocessed_commit is never read: the
 *              key's commitment is the one observed and checked), the permutation arrays when it has
 *              no permutation part.  Array lengths are the program's: W, C = 2^log_quotient_degree,
 *              Wq, and the key's width (C arrays carry none; a binding checks them, as native.py does).
 *              A proof of eon_prove_p2air[_fs] is verified with the generic program of the same AIR
 *              (its constraint order is the fused kernel's).
 *   vk_*       PreprocessedVerifierKey (preprocessed.rs:30-40) as plain values; vk_commitment NULL =
 *              no key (vk_width and vk_degree_bits are then ignored)
 *   challenges, alpha, zeta (eon_verify_air; host) the ones the proof was made with, mirroring
 *              eon_prove_air_lk; n_challenges must be the program's (EON_E_SHAPE)
 *   challenger (eon_verify_air_fs) is advanced exactly as the reference's verifier advances its own;
 *              challenges_out (2 Wq Fr) / alpha_out / zeta_out (host, nullable) receive what it gave
 *   *result    EON_VERIFY_*: the reference's Ok(()) or its VerificationError variant.  A commitment or
 *              witness that is no curve point, or an opened value that is no canonical Fr, is
 *              EON_VERIFY_INVALID_OPENING_ARGUMENT.
 * The return code is EON_OK whenever the verification ran to a verdict (eon_kzg_pcs_last_error then
 * says why a proof was rejected); negative codes stay for bad arguments and device errors: a NULL
 * trace or quotient array, a public value count that is not the program's (EON_E_SHAPE), a zeta on
 * the trace domain (EON_E_ARG: the reference panics).  ZK (RandomizationError) and global lookups
 * are outside, as in the prover. */
enum {
    EON_VERIFY_OK = 0,
    EON_VERIFY_INVALID_PROOF_SHAPE = 1,      /* VerificationError::InvalidProofShape */
    EON_VERIFY_INVALID_OPENING_ARGUMENT = 2, /* VerificationError::InvalidOpeningArgument(KzgError) */
    EON_VERIFY_OOD_EVALUATION_MISMATCH = 3   /* VerificationError::OodEvaluationMismatch */
};
int eon_verify_air(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proof, const eon_fr* publics,
                   uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits, const eon_g1_affine* vk_commitment,
                   const eon_fr* challenges, uint32_t n_challenges, const eon_fr* alpha, const eon_fr* zeta,
                   int* result);
int eon_verify_air_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proof,
                      const eon_fr* publics, uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits,
                      const eon_g1_affine* vk_commitment, eon_challenger* challenger, int* result,
                      eon_fr* challenges_out, eon_fr* alpha_out, eon_fr* zeta_out);

/* ---- proof bytes --------------------------------------------------------------------------------
 * A proof written down: the reference's Proof / Commitments / OpenedValues and KZG proof types derive
 * Serialize / Deserialize (eon-uni-stark/src/proof.rs:17-44, kzg/src/pcs.rs:21-98).  The ELEMENT
 * encodings are the reference's: an Fr is the 32 raw bytes of its Montgomery representation,
 * little-endian -- the bytes of eon_fr -- and a value >= r does not deserialise
 * (bn254/src/field.rs:188-207); a G1 is G1Affine::to_bytes, 32 compressed bytes, and an invalid point
 * does not deserialise (bn254/src/curve.rs:84-98) -- eon_g1_to_bytes / eon_g1_decompress_dev.  The
 * FRAMING is this project's own (serde's container format is the caller's choice in the reference and
 * pinned nowhere), as EONSRS1 is for an SRS.  All integers little-endian:
 *     0  magic "EONPRF1\0"
 *     8  u32 version = 1
 *    12  u32 flags: EON_PROOF_BATCHED | EON_PROOF_PREPROCESSED | EON_PROOF_PERMUTATION, every other bit zero
 *    16  u32 degree_bits
 *    20  u32 W, u32 C, u32 Wp, u32 Wq    (Wp / Wq zero exactly when their flag is clear)
 *    36  u32 zero
 *    40  u64 body length
 *    48  body, the sections EON_PROOF_SECTION_* in their numeric order (proof.rs:19-44, the rounds of
 *        prover.rs:426-439): commitments trace [W], permutation [Wq], quotient chunks [C]; opened values
 *        trace_local [W], trace_next [W], permutation_local / _next [Wq], preprocessed_local / _next
 *        [Wp], quotient chunks [C]; witnesses trace at zeta, at zeta h, permutation at zeta, at zeta h,
 *        chunks [C], preprocessed at zeta, at zeta h -- each witness section but the chunks' has the
 *        matrix's width in the per-column mode and ONE point in the batched mode (none when the part is
 *        absent).
 * Not in the bytes, as in the reference's Proof: the preprocessed commitment (the verifier key's; no
 * verify reads the proof's copy), every challenge (a loaded proof is verified with a challenger,
 * eon_verify_air_fs) and the timings.
 *
 * eon_proof_bytes_size: 48 + the body length of a shape, overflow-checked; 0 on an invalid shape.
 * eon_proof_serialize: host only, no context -- eon_g1_to_bytes per point -- so a tool without a GPU
 *   writes a proof.  Reads the arrays of `proof` at the lengths `shape` gives (preprocessed_commit and
 *   proof->pp.base.degree_bits are not read: shape->degree_bits is written); *written receives the
 *   size; cap below it or an invalid shape is EON_E_SHAPE; a NULL array that the shape needs, or an
 *   opened value >= r, is EON_E_ARG.
 * eon_proof_peek: host only; the header and the length.  The body length is recomputed from the
 *   header's shape and compared with the stated one AND with len before anything else happens: one
 *   byte short or one trailing byte is a rejection, and nothing is allocated.
 * eon_proof_deserialize: peek, then fills the caller's arrays, sized from peek's shape
 *   (preprocessed_commit is untouched and may be NULL; degree_bits is set).  Every opened value must
 *   be < r (FR_NOT_CANONICAL); ALL points of the proof are decompressed and checked on the device in
 *   one upload and one eon_g1_decompress call, whose report is mapped onto (reason, section, index in
 *   the section).  When several elements are bad the one at the lowest byte offset is reported.  An
 *   encoded identity is accepted and loads as (0,0): a constant column's witness and an all-zero
 *   column's commitment are the identity.  After a rejection the arrays hold unspecified values.
 * A rejection returns EON_E_FORMAT (eon.h) with *report filled (section EON_PROOF_SECTION_HEADER and
 * index 0 for the header's reasons); EON_OK leaves reason = EON_PROOF_IO_OK. */
enum { EON_PROOF_BATCHED = 1, EON_PROOF_PREPROCESSED = 2, EON_PROOF_PERMUTATION = 4 };
enum {
    EON_PROOF_IO_OK = 0,
    EON_PROOF_IO_MAGIC = 1,
    EON_PROOF_IO_VERSION = 2,
    EON_PROOF_IO_FLAGS = 3,  /* an unknown flag bit, a width that contradicts its flag, the reserved word */
    EON_PROOF_IO_LENGTH = 4, /* fewer than 48 bytes, or stated / actual length != the shape's */
    EON_PROOF_IO_FR_NOT_CANONICAL = 5,
    EON_PROOF_IO_G1_ENCODING = 6,      /* identity flag with other bits set */
    EON_PROOF_IO_G1_NOT_CANONICAL = 7, /* x >= q */
    EON_PROOF_IO_G1_NOT_ON_CURVE = 8   /* x^3 + 3 is no square */
};
enum {
    EON_PROOF_SECTION_HEADER = 0,
    EON_PROOF_SECTION_TRACE_COMMIT = 1,
    EON_PROOF_SECTION_PERMUTATION_COMMIT = 2,
    EON_PROOF_SECTION_QUOTIENT_COMMIT = 3,
    EON_PROOF_SECTION_TRACE_LOCAL = 4,
    EON_PROOF_SECTION_TRACE_NEXT = 5,
    EON_PROOF_SECTION_PERMUTATION_LOCAL = 6,
    EON_PROOF_SECTION_PERMUTATION_NEXT = 7,
    EON_PROOF_SECTION_PREPROCESSED_LOCAL = 8,
    EON_PROOF_SECTION_PREPROCESSED_NEXT = 9,
    EON_PROOF_SECTION_QUOTIENT_OPENED = 10,
    EON_PROOF_SECTION_TRACE_WITNESS_ZETA = 11,
    EON_PROOF_SECTION_TRACE_WITNESS_NEXT = 12,
    EON_PROOF_SECTION_PERMUTATION_WITNESS_ZETA = 13,
    EON_PROOF_SECTION_PERMUTATION_WITNESS_NEXT = 14,
    EON_PROOF_SECTION_QUOTIENT_WITNESS = 15,
    EON_PROOF_SECTION_PREPROCESSED_WITNESS_ZETA = 16,
    EON_PROOF_SECTION_PREPROCESSED_WITNESS_NEXT = 17
};
typedef struct {
    uint32_t flags, degree_bits, width, chunks, pre_width, perm_width;
} eon_proof_shape;
typedef struct {
    uint32_t reason, section;
    uint64_t index;
} eon_proof_io_report;
uint64_t eon_proof_bytes_size(const eon_proof_shape* shape);
int eon_proof_serialize(const eon_proof_lk* proof, const eon_proof_shape* shape, uint8_t* out, uint64_t cap,
                        uint64_t* written);
int eon_proof_peek(const uint8_t* bytes, uint64_t len, eon_proof_shape* shape, eon_proof_io_report* report);
int eon_proof_deserialize(eon_ctx* ctx, const uint8_t* bytes, uint64_t len, eon_proof_lk* out,
                          eon_proof_io_report* report);

/* ---- verifying many proofs in one pass ----------------------------------------------------------
 * n proofs of ONE program against one pcs, one verdict per proof: results[i] -- and the detail, the
 * challenges reported and the end state of challenger i -- is exactly what eon_verify_air[_fs] gives
 * for proof i alone.  The three phases of the verifier run over the whole batch: the host part of
 * every proof (shapes, transcript, the opening list, quotient(zeta)) on min(n, 8) threads; the
 * openings of every proof still standing in ONE eon_kzg_verify_batch_many, a segment per proof (each
 * proof keeps its own Gt product: no random weights across proofs, and a bad proof is located
 * without bisection); ONE eon_air_eval_at_points_dev over the proofs whose openings passed.
 *   proofs: n eon_proof_lk.  publics: n x n_public.  The verifier key is shared (one AIR).
 *   eon_verify_air_many: challenges n x n_challenges, alphas[n], zetas[n]; in the batched opening
 *     mode gammas[n] / deltas[n], or NULL for the pcs's eon_kzg_pcs_set_opening_challenges pair.
 *     (The arrays are there because result i must be eon_verify_air's for proof i: a proof made
 *     with given challenges carries its OWN gamma and delta, and the pcs holds one pair.  For the
 *     same reason eon_verify_many_opening_challenges reports, per proof, what
 *     eon_kzg_pcs_last_opening_challenges reports for a single verify.)
 *   eon_verify_air_many_fs: n distinct challengers, advanced as eon_verify_air_fs advances one;
 *     challenges_out (n x the program's challenge count), alphas_out[n], zetas_out[n] may be NULL
 *     and entry i is left unwritten for a shape-rejected proof.
 * Every proof of a call uses the pcs's current opening mode.  What is an error code (not a verdict)
 * in eon_verify_air is one here, its message starting "proof i: ", and no verdicts are written.
 * After EON_OK, eon_kzg_pcs_last_error holds the first rejected proof's reason as "proof i: ..."
 * (empty when all are valid), eon_verify_many_detail(pcs, i) the reason of proof i (empty when
 * valid; NULL for an index past the last call's n; valid until the next call on the pcs), and
 * eon_verify_many_opening_challenges the gamma / delta used for proof i in the batched mode.
 * n = 0 writes nothing. */
int eon_verify_air_many(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proofs, uint32_t n,
                        const eon_fr* publics, uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits,
                        const eon_g1_affine* vk_commitment, const eon_fr* challenges, uint32_t n_challenges,
                        const eon_fr* alphas, const eon_fr* zetas, const eon_fr* gammas, const eon_fr* deltas,
                        int* results);
int eon_verify_air_many_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proofs, uint32_t n,
                           const eon_fr* publics, uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits,
                           const eon_g1_affine* vk_commitment, eon_challenger* const* challengers, int* results,
                           eon_fr* challenges_out, eon_fr* alphas_out, eon_fr* zetas_out);
const char* eon_verify_many_detail(const eon_kzg_pcs* pcs, uint32_t i);
int eon_verify_many_opening_challenges(const eon_kzg_pcs* pcs, uint32_t i, eon_fr* gamma, eon_fr* delta);

/* 11 also carries eon_prove_air_sharded[_fs], added later without a bump (new symbols only).
 * 11: eon_verify_air_many[_fs], eon_verify_many_detail / _opening_challenges, additive.
 * bumped on any signature or struct-layout change (4: the preprocessed surface above; 5: the lookup
 * surface above; 6: the check_constraints switch and report; 7: eon_verify_air[_fs]; 8:
 * eon_kzg_pcs_create_from_srs[_bytes] and eon_kzg_pcs_create_verifier; 9: the opening mode,
 * eon_kzg_pcs_set_opening and its challenges; 10: the proof bytes, eon_proof_bytes_size / _serialize /
 * _peek / _deserialize; all additive) */
uint32_t eon_prove_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* EON_PROVE_H */
