/*
 * eon.h -- C ABI of the MI355X (gfx950) prover hot path for the plonky3-eon BN254/KZG stack.
 *
 * This is the drop-in boundary: every entry point replaces one reference interface on the
 * prover path, cited below as reference file:line (reference = Lolazyx/plonky3-eon).  Plain
 * pointers and sizes only; no torch or HIP types in signatures (streams are passed as void*).
 * A Rust shim binds these with `extern "C"`.
 *
 * Data layout (shared with the reference, zero-copy):
 *   eon_fr        = p3_bn254::Fr: [u64;4] little-endian Montgomery residue a*2^256 mod r,
 *                   canonical (< r)                                   (bn254/src/field.rs:98-105)
 *   matrices      = p3_matrix RowMajorMatrix<Fr>: element (row, col) at values[row*width + col]
 *                                                                     (matrix/src/dense.rs:24-37)
 *   eon_g1_affine = BN254 G1 affine point, x and y as Fq Montgomery residues (R = 2^256 mod q),
 *                   [u64;4] LE each; the point at infinity is encoded as x = y = 0.
 *
 * Conventions:
 *   - return 0 on success, a negative EON_E_* code otherwise; eon_last_error() has the message.
 *     The reference panics in these cases (assert!/log2_strict_usize/unwrap); a Rust shim
 *     should panic on a nonzero return to keep that behaviour.
 *   - `*_dev` entry points take DEVICE pointers and enqueue asynchronously on the context's
 *     stream (eon_ctx_set_stream); the others take HOST pointers and are synchronous.
 *   - a context is internally locked: entry points are thread-safe (the reference's DFTs are
 *     Clone + Sync and share twiddle caches, dft/src/radix_2_dit_parallel.rs:30-40).
 */
#ifndef EON_H
#define EON_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t l[4];
} eon_fr;

typedef struct {
    uint64_t x[4];
    uint64_t y[4];
} eon_g1_affine;

/* BN254 G2 affine point on the sextic twist over Fq2 = Fq[u]/(u^2 + 1): x = x[0] + x[1] u (Fq
 * Montgomery [u64;4] LE each), identity = all zero.  Gt / Fq12 element in the tower
 * Fq12 = Fq6[w]/(w^2 - v), Fq6 = Fq2[v]/(v^3 - (9 + u)): c[2k], c[2k+1] = the Fq2 coefficient k
 * in the order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (halo2curves' Fq12 layout). */
typedef struct {
    uint64_t x[2][4];
    uint64_t y[2][4];
} eon_g2_affine;

typedef struct {
    uint64_t c[12][4];
} eon_fq12;

typedef struct eon_ctx eon_ctx;

/* Collectives over DEVICE buffers among `world` processes (one per GPU), called with a context's
 * stream; each must leave recv complete and ordered before that stream's later work (an RCCL call
 * enqueued on `hip_stream` does; a host-staged one synchronizes).
 *   all_gather: recv receives `world` blocks of `bytes`, in rank order.  Used by the lane-sharded
 *               prove (eon_prove.h), a context's sharded work (eon_ctx_set_collective) and
 *               eon_msm_sharded_dev.
 *   all_to_all: send holds `world` blocks of `bytes` (block h goes to rank h); recv receives
 *               `world` blocks, block g from rank g (ncclAllToAll).  Used by
 *               eon_fourstep_dft_dev; may be NULL when no four-step transform runs. */
typedef struct {
    uint32_t rank;
    uint32_t world;
    int (*all_gather)(void* user, const void* send, void* recv, uint64_t bytes, void* hip_stream);
    void* user;
    int (*all_to_all)(void* user, const void* send, void* recv, uint64_t bytes, void* hip_stream);
} eon_collective;
typedef struct eon_msm_bases eon_msm_bases;
typedef struct eon_msm_scalars eon_msm_scalars;

enum {
    EON_OK = 0,
    EON_E_SHAPE = -1,            /* height not a power of two, size mismatch (reference: panic) */
    EON_E_DEGREE_TOO_LARGE = -2, /* KzgError::DegreeTooLarge (kzg/src/params.rs:164-173) */
    EON_E_DEVICE = -3,           /* HIP runtime error */
    EON_E_OOM = -4,              /* device allocation failed */
    EON_E_ARG = -5,              /* null pointer / invalid argument */
    EON_E_CONSTRAINT = -6,       /* the prove driver's constraint check failed (eon_prove.h; the reference's
                                    debug-build panic, check_constraints.rs:165-173) */
    EON_E_SRS = -7,              /* a supplied SRS was rejected; the eon_srs_report says why */
    EON_E_FORMAT = -8            /* proof bytes were rejected (eon_prove.h); the eon_proof_io_report says why */
};

enum {
    EON_ORDER_NATURAL = 0, /* RowMajorMatrix output, as Radix2Dit (dft/src/radix_2_dit.rs:61-77) */
    EON_ORDER_BITREV = 1   /* storage of Radix2DitParallel's BitReversedMatrixView: storage row
                              reverse_bits_len(k, log2 h) holds logical row k
                              (dft/src/radix_2_dit_parallel.rs:146,165,227) */
};

/* output layouts of eon_fourstep_dft_dev */
enum {
    EON_FOURSTEP_NATURAL = 0,    /* rank g holds X[g N/G, (g+1) N/G): its contiguous natural slice
                                    (a second all_to_all) */
    EON_FOURSTEP_TRANSPOSED = 1  /* rank g holds the N2 x N1/G row-major block of the N2 x N1 view:
                                    row k2, column k1' = X[N1 k2 + g N1/G + k1'] (one all_to_all) */
};

/* ---- context ---------------------------------------------------------------------------- */
int eon_ctx_create(int device_ordinal, eon_ctx** out);
void eon_ctx_destroy(eon_ctx* ctx);
const char* eon_last_error(const eon_ctx* ctx);
/* Stream (a hipStream_t) for all subsequent work of this context, used verbatim: NULL selects
 * the HIP null (default) stream.  Until the first call the context uses a stream of its own. */
int eon_ctx_set_stream(eon_ctx* ctx, void* hip_stream);
/* The stream the context currently enqueues on (as set, or its own). */
void* eon_ctx_stream(eon_ctx* ctx);
/* The device ordinal the context was created on. */
int eon_ctx_device(const eon_ctx* ctx);
/* Bind the context to a process group (copied; NULL or world <= 1 unbinds).  Work that is the
 * same on every rank then splits across the ranks: eon_kzg_opening_bases_create(_many) computes
 * 1/world of the rows and all-gathers the tables.  Every rank must then make the same calls in
 * the same order. */
int eon_ctx_set_collective(eon_ctx* ctx, const eon_collective* coll);
int eon_ctx_synchronize(eon_ctx* ctx);
/* Give back to the device every cached idle buffer of the context: the transient-buffer pool
 * (KZG opening-bases tables and scratch; capped at EON_POOL_CAP_GB, default 8, read at creation)
 * and the kept sorted-digit buffers of destroyed eon_msm_scalars (capped at 48 GB).  Synchronizes
 * the context's streams first.  Call it between proofs when another allocator in the process
 * (e.g. torch's caching allocator) needs the memory; the next proof allocates afresh. */
int eon_ctx_trim(eon_ctx* ctx);
/* Per-launch kernel timing with HIP events on the launch stream (the analogue of the
 * reference's tracing spans, e.g. dft/src/radix_2_dit_parallel.rs:168).  eon_ctx_profile(ctx, 1)
 * clears the record and starts recording; eon_ctx_profile_report writes a JSON object
 * {kernel: {launches, total_ms, alg_bytes}} into buf (synchronizes on the recorded events). */
int eon_ctx_profile(eon_ctx* ctx, int enable);
int eon_ctx_profile_report(eon_ctx* ctx, char* buf, uint64_t len);
/* Serial mode (also EON_SERIAL=1 at creation): every kernel of this context on its one stream,
 * none on the MSM / opening side streams, so that each launch runs alone on the device and its
 * event-timed or profiler duration is isolated.  For measurement only: results are identical,
 * the prove is slower (no overlap of digit sorts with piece sums). */
int eon_ctx_set_serial(eon_ctx* ctx, int serial);
int eon_ctx_serial(const eon_ctx* ctx);
/* ---- diagnostics (measurement only; not on any product path) ------------------------------ */
typedef struct {
    double clock_mhz_median; /* in-kernel shader clock: delta s_memtime / delta s_memrealtime x 100 MHz */
    double clock_mhz_min;    /* over the blocks of the last launch */
    double clock_mhz_max;
    double products_per_s;   /* radix-2^29 Montgomery products per second over the timed launches */
    double ms_per_launch;
} eon_clock_probe;
/* Run `launches` back-to-back launches of a radix-2^29 product chain (`iters` products per chain,
 * two chains per thread, 4096 x 256 threads) on the context stream, after one untimed launch, and
 * report the shader clock the chip held (median over blocks of the last launch) and the product
 * rate (MI355X_MICROARCH.md, DVFS item 6).  Synchronous. */
int eon_diag_clock_probe(eon_ctx* ctx, uint32_t launches, uint32_t iters, eon_clock_probe* out);
/* Self-check of the whole-product asm statements the MSM piece sums use (prod_asm.h) against the
 * column-block products, bit for bit, on n pseudo-random operands of each kind at their limb
 * bounds (half of them at the maximum limb); mismatches[0..2] = mismatching mul / sqr / sum2
 * cases. */
int eon_diag_prod_asm_check(eon_ctx* ctx, uint32_t n, uint32_t seed, uint32_t mismatches[3]);
/* The same for the in-place forms the piece sums' hot loop uses (mul29_asm_ip: a = a b;
 * mul29_sum2_asm_ip: c = a b + c d; tied read-write operands, another register arrangement than
 * the out-of-place statements): operands drawn as above, the overwritten operand copied first,
 * results compared bit for bit with the column-block mul29 / mul29_sum2.  mismatches[0..1] =
 * mismatching mul / sum2 cases. */
int eon_diag_prod_asm_ip_check(eon_ctx* ctx, uint32_t n, uint32_t seed, uint32_t mismatches[2]);
/* The stages of the MSM digit pipeline on their own (tests; host pointers, synchronous, scratch
 * from the context's pool).
 * eon_diag_radix_sort_pairs: the stable LSD radix sort of the n pairs (keys[i], vals[i]) on key
 *   bits [0, bits), bits <= 32, with the sort's own histogram kernel; key bits above `bits` do not
 *   order and are kept.  n <= 2^24.
 * eon_diag_exclusive_scan_u32: out[i] = in[0] + ... + in[i-1] modulo 2^32, n <= 2^24.
 * eon_diag_scan_chunk_counts: the piece offsets of nb buckets given by their nb + 1 `start`s: the
 *   exclusive sum (nb + 1 outputs) of count[b] = the 2^log_chunk-aligned runs the pairs
 *   [start[b], start[b+1]) touch (0 if empty, count[nb] = 0); *max_out = the largest count if it
 *   exceeds 1, else 0.  nb <= 2^24, log_chunk < 32. */
int eon_diag_radix_sort_pairs(eon_ctx* ctx, const uint32_t* keys, const uint32_t* vals, uint64_t n, uint32_t bits,
                              uint32_t* keys_out, uint32_t* vals_out);
int eon_diag_exclusive_scan_u32(eon_ctx* ctx, const uint32_t* in, uint64_t n, uint32_t* out);
int eon_diag_scan_chunk_counts(eon_ctx* ctx, const uint32_t* start, uint32_t nb, uint32_t log_chunk, uint32_t* out,
                               uint32_t* max_out);
/* One radix-2^29 curve formula of the MSM bucket sums (csrc/ec29.h) per thread, on n independent
 * cases (tests; host pointers, synchronous, scratch from the context's pool; n <= 2^20).
 * `acc` and `acc_out` are n raw accumulators of 36 words: X, Y, ZZ, ZZZ as 9 limbs of 29 bits each
 * (value sum l[i] 2^(29 i), x 2^261 mod q), raw ZZ == 0 meaning the identity; they are read and
 * written with the bucket sums' own load and store.  `arg` is per case an affine base as 18 words
 * (x then y, 9 limbs each, passed to the formula as they are) or a second raw accumulator of 36
 * words, by `op`:
 *    0 madd29            acc += arg(18); code = its return (0: exceptional, acc unchanged)
 *    1 madd29_unchecked  acc += arg(18); code 0
 *    2 madd29_negsum     acc = the tuple of -(acc + arg(18)); code 0
 *    3 madd29_exceptional(acc, arg(18)); code = its return (1: the sum is the identity)
 *    4 dbl29_affine      acc_out = 2 arg(18); `acc` is not read and may be NULL
 *    5 dbl29             acc = 2 acc; no arg
 *    6 add29             acc += arg(36); code = its return 0 / 1 / 2
 *    7 add29_ilp         the same
 *    8 dbl29_ilp         acc = 2 acc; no arg
 *    9 acc29             acc += arg(36) with the identity flags of both raw inputs; code = the
 *                        resulting flag, an identity is stored as 36 zero words
 *   10 acc29_ilp         the same
 *   11 raw29_to_xyzz     words 0..31 of acc_out = the canonical radix-2^32 Montgomery X, Y, ZZ, ZZZ
 *                        (8 words each), words 32..35 zero; code = 1 for the identity; no arg
 *   12 to_fq261(to_fq256(c)) of each of acc's four coordinates c, as 256-bit integers in words
 *                        0..31 of acc_out, words 32..35 zero; code 0; no arg
 *   13 neg29_lazy        X = 2q - X and ZZZ = 3q - ZZZ limb by limb (X < q, ZZZ < 2q, normalised),
 *                        the piece loop's negations of a base's y and of a flushed ZZZ; Y and ZZ
 *                        pass through; code 0; no arg
 *   14 x29_to_xyzz       as 11, from the loaded accumulator and its identity flag
 * An `arg` that `op` does not read may be NULL.  EON_E_ARG for an unknown op, n > 2^20, or a NULL
 * pointer that is read or written with n > 0.  The formulas' preconditions (non-identity inputs,
 * coordinate bounds) are the caller's. */
int eon_diag_ec29_op(eon_ctx* ctx, uint32_t op, const uint32_t* acc, const uint32_t* arg, uint64_t n,
                     uint32_t* acc_out, int32_t* code_out);
/* What a prepared handle (eon_msm_g1_columns_prepare_dev) keeps of its column batches.  A batch
 * covers columns [col0, col0 + cols) with window width c and `windows` digit windows per scalar;
 * `ref_windows` is the window count of the bases' layout (a fixed-base reference is row *
 * ref_windows + window).  Keys are (group << c) | (|digit| - 1) with `groups` groups (the batch's
 * columns, or column x window without fixed-base tables), nb = groups * 2^(c-1) buckets, bucket
 * (|digit| - 1) * groups + group.  The batch keeps `pairs` = rows * windows * cols sorted (key, value)
 * pairs, of which the first n_pairs are nonzero digits in bucket order and the rest the zero-digit
 * sentinel 0xFFFFFFFF; start[b] = the first pair of bucket >= b (nb + 1 entries) and piece_off = the
 * piece offsets of `start` at log_chunk (nb + 1 entries, n_pieces = piece_off[nb]). */
typedef struct {
    uint64_t pairs;
    uint32_t c;
    uint32_t windows;
    uint32_t ref_windows;
    uint32_t groups;
    uint32_t nb;
    uint32_t log_chunk;
    uint32_t cols;
    uint32_t col0;
    uint32_t n_pairs;
    uint32_t n_pieces;
} eon_msm_batch_info;
/* The number of batches of `prepared` (0 for an empty matrix). */
int eon_diag_msm_scalars_batches(eon_ctx* ctx, const eon_msm_scalars* prepared, uint32_t* count);
/* Batch k's layout into *info and copies of its kept arrays into the host buffers that are not
 * NULL: keys / vals (info->pairs entries each), start / piece_off (info->nb + 1 entries each).
 * Reads only; the handle is unchanged. */
int eon_diag_msm_scalars_batch(eon_ctx* ctx, const eon_msm_scalars* prepared, uint32_t k, eon_msm_batch_info* info,
                               uint32_t* keys, uint32_t* vals, uint32_t* start, uint32_t* piece_off);
/* Batch k's bucket order, kept by column batches (>= 64 groups) for the one-bucket-per-lane piece
 * sums: per window of *window consecutive bucket indices (the last may be short), those indices
 * stably sorted by run length start[b + 1] - start[b], shortest first (lengths of 1023 and above
 * compare equal).  *window = 0 for a batch without an order, whose `order` is then left unwritten;
 * otherwise `order`, when not NULL, receives info->nb entries.  *bucket_lanes = 1 when the batch's
 * piece sums take the one-bucket-per-lane route (every MSM against the handle does alike), 0 for
 * the chunked route.  Reads only. */
int eon_diag_msm_scalars_order(eon_ctx* ctx, const eon_msm_scalars* prepared, uint32_t k, uint32_t* window,
                               uint32_t* bucket_lanes, uint32_t* order);

/* One single-column MSM over device scalars as eon_msm_g1_dev runs it -- digitising only the
 * windows its largest scalar reaches (one more for the recoding's carry), which a handle made by
 * eon_msm_g1_columns_prepare_dev never does -- that also keeps its one batch in *prepared, for
 * eon_diag_msm_scalars_batch to read back: info->windows may then be below info->ref_windows while
 * the fixed-base references stay row * ref_windows + window.  *out receives the MSM's point. */
int eon_diag_msm_g1_prepare_active_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* scalars, uint64_t n,
                                       eon_g1_affine* out, eon_msm_scalars** prepared);

/* ABI version; bumped on any signature or struct-layout change.
 *   16 also carries, added later without a bump (new symbols only, no signature or layout of
 *       version 16 changed; a binding that needs them looks the symbols up): the column-sharded
 *       prove's device side -- eon_shard_column_range / _row_range, eon_shard_pack_rows_dev /
 *       _unpack_cols_dev and eon_quotient_values_rows_dev;
 *   16: many checks in one pass -- eon_multi_pairing_many, eon_kzg_verify_batch_many and
 *       eon_air_eval_at_points_dev, additive;
 *   15: eon_diag_msm_scalars_order, a column batch's bucket order and piece-sum route, additive;
 *   14: eon_g1_compress[_dev], the inverse of eon_g1_decompress[_dev], and EON_E_FORMAT, additive;
 *   13: eon_fr_fold_columns_dev, the gamma-fold of the batched KZG opening, additive;
 *   12: loading a supplied SRS -- eon_g1_decompress[_dev], eon_g1_validate_dev, eon_kzg_srs_check,
 *       eon_srs_report and EON_E_SRS, additive;
 *   11: KzgMmcs -- eon_quotient_and_eval_columns_multi_dev, eon_kzg_mmcs_local_index / _open_dev /
 *       _verify_batch and eon_mmcs_matrix, additive;
 *   10: eon_air_eval_at_point_dev, the compiled constraints at one out-of-domain point, additive;
 *   9: eon_check_constraints_dev and eon_constraint_report, EON_E_CONSTRAINT, additive;
 *   8: eon_diag_ec29_op, the curve formulas of the MSM bucket sums one per thread, additive;
 *   7: the eon_diag_* stage diagnostics of the MSM digit pipeline and eon_msm_batch_info, additive;
 *   6: the LogUp lookup entry points eon_air_program_create_lk / eon_quotient_values_lk_dev /
 *      eon_lookup_permutation_dev, additive;
 *   5: preprocessed columns in the generic quotient, eon_air_program_create_pp /
 *      eon_quotient_values_pp_dev, additive;
 *   4: the verifier pairings and their eon_g2_affine / eon_fq12 types;
 *   3: eon_collective's all_to_all field.
 * Bindings must check it at load time: a binding built against an older layout would pass a
 * shorter eon_collective. */
uint32_t eon_abi_version(void);

/* ---- TwoAdicSubgroupDft<Fr> (dft/src/traits.rs:27-249) -----------------------------------
 * `in` is height x width, row-major.  height must be a power of two with log2(height) (+ added
 * bits) <= 28 (Fr::TWO_ADICITY, bn254/src/field.rs:564).  `in` and `out` may alias. */

/* dft_batch (dft/src/traits.rs:61): coefficients -> evaluations on H. */
int eon_dft_batch(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height, uint32_t width,
                  int out_order);
/* idft_batch (dft/src/traits.rs:111-122): evaluations on H -> coefficients (natural order). */
int eon_idft_batch(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height, uint32_t width);
/* coset_dft_batch (dft/src/traits.rs:83-91): coefficients -> evaluations on shift*H. */
int eon_coset_dft_batch(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                        uint32_t width, const eon_fr* shift, int out_order);
/* coset_idft_batch (dft/src/traits.rs:144-153): evaluations on shift*H -> coefficients. */
int eon_coset_idft_batch(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                         uint32_t width, const eon_fr* shift);
/* coset_lde_batch (dft/src/traits.rs:226-249; Radix2DitParallel override at
 * dft/src/radix_2_dit_parallel.rs:169-228): evaluations on H -> evaluations on shift*K,
 * |K| = height << added_bits.  `out` holds (height << added_bits) x width.  shift NULL = ONE
 * (lde_batch, dft/src/traits.rs:187-192).  `shift` is always a host pointer. */
int eon_coset_lde_batch(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                        uint32_t width, uint32_t added_bits, const eon_fr* shift, int out_order);
/* coset_dft_batch of the COEFFICIENT matrix zero-padded to height << added_bits -- the second
 * half of coset_lde_batch (dft/src/traits.rs:226-249), and KzgPcs::get_evaluations_on_domain from
 * the committed coefficients (kzg/src/pcs.rs:267-287, commit/src/testing.rs:93-105):
 * out[k] = sum_j coeffs[j] (shift * w^k)^j, |K| = height << added_bits.  `in` != `out`. */
int eon_coset_dft_padded_batch(eon_ctx* ctx, const eon_fr* coeffs, eon_fr* out, uint64_t height,
                               uint32_t width, uint32_t added_bits, const eon_fr* shift,
                               int out_order);

/* device-pointer variants (same semantics, asynchronous on the context stream) */
int eon_dft_batch_dev(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                      uint32_t width, int out_order);
int eon_idft_batch_dev(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                       uint32_t width);
int eon_coset_dft_batch_dev(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                            uint32_t width, const eon_fr* shift, int out_order);
int eon_coset_idft_batch_dev(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                             uint32_t width, const eon_fr* shift);
int eon_coset_lde_batch_dev(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint64_t height,
                            uint32_t width, uint32_t added_bits, const eon_fr* shift,
                            int out_order);
int eon_coset_dft_padded_batch_dev(eon_ctx* ctx, const eon_fr* coeffs, eon_fr* out, uint64_t height,
                                   uint32_t width, uint32_t added_bits, const eon_fr* shift,
                                   int out_order);

/* ---- BN254 G1 multi-scalar multiplication -------------------------------------------------
 * Value of G1::multi_exp (bn254/src/curve.rs:158-179, halo2curves msm_best): sum_i s_i * P_i,
 * returned in affine form ((0,0) = identity; empty input -> identity).  Bases are uploaded
 * once into an eon_msm_bases handle and reused, as the KZG SRS g1_powers is
 * (kzg/src/params.rs:57-139, commit_column kzg/src/util.rs:37-40). */
enum {
    EON_MSM_PRECOMPUTE = 1 /* fixed-base mode: store 2^(c*w) * P_i for every window (SRS bases) */
};
/* `bases`: host array of n affine points with canonical coordinates. */
int eon_msm_bases_create(eon_ctx* ctx, const eon_g1_affine* bases, uint64_t n, uint32_t flags,
                         eon_msm_bases** out);
void eon_msm_bases_destroy(eon_msm_bases* bases);
uint64_t eon_msm_bases_len(const eon_msm_bases* bases);
/* MSM over the first n bases; `scalars` host (eon_msm_g1) or device (eon_msm_g1_dev) Fr array;
 * `out` is a host pointer; both calls return when the result is in *out.  n > len(bases) is
 * EON_E_SHAPE (the reference asserts equal lengths, curve.rs:159-162). */
int eon_msm_g1(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* scalars, uint64_t n,
               eon_g1_affine* out);
int eon_msm_g1_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* scalars, uint64_t n,
                   eon_g1_affine* out);
/* One MSM per column of a row-major rows x width Fr matrix over bases[0..rows): out[j] =
 * sum_i mat[i][j] * P_i (width affine points, host) -- the per-column commit_column loop of
 * KzgPcs::commit (kzg/src/pcs.rs:244-251) and of open's witnesses (pcs.rs:310-316).  `mat` is
 * host (eon_msm_g1_columns) or device (eon_msm_g1_columns_dev). */
int eon_msm_g1_columns(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* mat, uint64_t rows,
                       uint32_t width, eon_g1_affine* out);
int eon_msm_g1_columns_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* mat,
                           uint64_t rows, uint32_t width, eon_g1_affine* out);
/* quotient_and_eval (kzg/src/util.rs:100-111) for every column of a row-major rows x width
 * coefficient matrix (device) at `point` (host): quotient (device) receives the (rows-1) x width
 * synthetic-division quotients, values (device) the width evaluations f_j(point), as
 * KzgPcs::open computes per (matrix, point, column) (kzg/src/pcs.rs:297-330).  quotient NULL:
 * values only. */
int eon_quotient_and_eval_columns_dev(eon_ctx* ctx, const eon_fr* coeffs, uint64_t rows,
                                      uint32_t width, const eon_fr* point, eon_fr* quotient,
                                      eon_fr* values);
/* The remainder of quotient_and_eval (kzg/src/util.rs:100-111) only -- f_j(z) for every column
 * of the rows x width coefficient matrix (device) at npoints points (host array): values
 * (device) receives npoints x width Fr, values[t * width + j] = f_j(points[t]).  One read of the
 * coefficients serves up to four points (KzgPcs::open's opened values, kzg/src/pcs.rs:305-316). */
int eon_eval_columns_dev(eon_ctx* ctx, const eon_fr* coeffs, uint64_t rows, uint32_t width,
                         const eon_fr* points, uint32_t npoints, eon_fr* values);
/* quotient_and_eval (kzg/src/util.rs:100-111) for every column of the rows x width coefficient
 * matrix (device) at npoints points (host array of canonical Fr) in one pass over the coefficients,
 * as KzgMmcs::open_batch needs it per (matrix, local index, column) (kzg/src/mmcs.rs:223-230):
 * values (device) receives npoints x width Fr, values[t * width + j] = f_j(points[t]); quotients
 * (device) ONE row-major (rows-1) x (npoints*width) matrix whose column t * width + j is the
 * synthetic-division quotient of column j by (X - points[t]) -- the quotients side by side, so that
 * one eon_msm_g1_columns_dev over bases[0..rows-1) gives every witness.  Every output is canonical
 * and bit-identical to eon_quotient_and_eval_columns_dev called once per point.  One load of a
 * coefficient serves up to four points; more points run in groups of four.  width == 0 or
 * npoints == 0: nothing is written; rows == 0: zero values; rows == 1: values only (the quotients
 * are empty); quotients NULL: values only.  EON_E_ARG for a point that is not canonical and for a
 * NULL pointer that would be read or written. */
int eon_quotient_and_eval_columns_multi_dev(eon_ctx* ctx, const eon_fr* coeffs, uint64_t rows, uint32_t width,
                                            const eon_fr* points, uint32_t npoints,
                                            eon_fr* quotients, eon_fr* values);
/* As eon_msm_bases_create with `bases` a DEVICE pointer (coordinates are not re-validated). */
int eon_msm_bases_create_dev(eon_ctx* ctx, const eon_g1_affine* bases, uint64_t n, uint32_t flags,
                             eon_msm_bases** out);
/* One-shot G1::multi_exp(points, scalars) on host arrays (bases uploaded for this call only). */
int eon_g1_multi_exp(eon_ctx* ctx, const eon_g1_affine* points, const eon_fr* scalars, uint64_t n,
                     eon_g1_affine* out);

/* Prepared scalar columns.  eon_msm_g1_columns_prepare_dev is eon_msm_g1_columns_dev (out may be
 * NULL) that also keeps every column's sorted bucket digits on device in *prepared
 * (~8 bytes x rows x ceil(255/c) per column), so that MSMs of the SAME columns against other
 * bases of the same window layout skip the digit extraction and sort:
 * eon_msm_g1_columns_prepared writes out[t * width + j] = sum_i mat[i][j] * bases[t][i].  KzgPcs
 * commits a matrix with the first (kzg/src/pcs.rs:244-251) and opens it with the second against
 * eon_kzg_opening_bases_create bases (pcs.rs:305-316).  `mat` need not outlive the prepare call;
 * every bases[t] must hold >= rows points with the window layout of the prepare call's bases
 * (EON_E_SHAPE otherwise). */
int eon_msm_g1_columns_prepare_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* mat,
                                   uint64_t rows, uint32_t width, eon_g1_affine* out,
                                   eon_msm_scalars** prepared);
int eon_msm_g1_columns_prepared(eon_ctx* ctx, const eon_msm_bases* const* bases, uint32_t nbases,
                                const eon_msm_scalars* prepared, eon_g1_affine* out);
void eon_msm_scalars_destroy(eon_msm_scalars* prepared);
/* KZG opening bases for `point` z (host) over the first n-1 points G_i of `srs`:
 * H_j = sum_{i<j} z^(j-1-i) G_i, j < n (H_0 = identity), in the window layout of `srs`.  For any
 * coefficient column c of length n, sum_j c_j H_j = commit_column(quotient_and_eval(c, z).0)
 * (kzg/src/util.rs:37-40,100-111): the opening witness of KzgPcs::open (kzg/src/pcs.rs:305-316)
 * as an MSM of the committed coefficients themselves. */
int eon_kzg_opening_bases_create(eon_ctx* ctx, const eon_msm_bases* srs, uint64_t n,
                                 const eon_fr* point, eon_msm_bases** out);
/* The same for npoints points (host array) at once (the points' constructions overlap on the
 * device): outs[t] = the opening bases of points[t]. */
int eon_kzg_opening_bases_create_many(eon_ctx* ctx, const eon_msm_bases* srs, uint64_t n,
                                      const eon_fr* points, uint32_t npoints, eon_msm_bases** outs);

/* ---- eon-uni-stark quotient on the Poseidon2-AIR --------------------------------------------
 * selectors_on_coset (commit/src/domain.rs:252-292): for the trace domain H (shift 1, 2^log_n) on
 * the coset shift * K (2^log_q), writes 4 x 2^log_q Fr to device `out`: is_first_row,
 * is_last_row, is_transition, inv_vanishing.  shift (host) must not be ONE (domain.rs:254). */
int eon_selectors_on_coset_dev(eon_ctx* ctx, uint32_t log_n, uint32_t log_q, const eon_fr* shift,
                               eon_fr* out);

/* Poseidon2-AIR over BN254 Fr (poseidon2-air/src/air.rs): WIDTH 3, SBOX_DEGREE 5,
 * SBOX_REGISTERS 1, external layer mds_light, internal layer [2,1,1;1,2,1;1,1,3]
 * (bn254/src/poseidon2.rs:55-63); VECTOR_LEN permutations per row (vectorized.rs).  Constants
 * are host arrays: beginning/ending half_full_rounds x 3, partial partial_rounds
 * (RoundConstants, poseidon2-air/src/constants.rs:17-31). */
typedef struct {
    uint32_t half_full_rounds;
    uint32_t partial_rounds;
    const eon_fr* beginning;
    const eon_fr* partial;
    const eon_fr* ending;
} eon_poseidon2_constants;
typedef struct eon_p2air eon_p2air;
/* Poseidon2Air::new / VectorizedPoseidon2Air::new (vector_len: power of two <= 32) */
int eon_p2air_create(eon_ctx* ctx, const eon_poseidon2_constants* constants, uint32_t vector_len,
                     eon_p2air** out);
void eon_p2air_destroy(eon_p2air* air);
/* trace width: (4 + 12 * half_full_rounds + 2 * partial_rounds) * vector_len (164 * vector_len) */
uint32_t eon_p2air_width(const eon_p2air* air);
/* VECTOR_LEN, and the constraints of one permutation: 12 * half_full_rounds + 2 * partial_rounds
 * (160; the folder's per-lane block, eon-uni-stark/src/folder.rs:81-85) */
uint32_t eon_p2air_vector_len(const eon_p2air* air);
uint32_t eon_p2air_constraints_per_perm(const eon_p2air* air);
/* generate_vectorized_trace_rows (poseidon2-air/src/generation.rs:14-72): inputs n_perms x 3 Fr
 * (device), trace (n_perms / vector_len) x width (device); n_perms = vector_len * 2^k. */
int eon_p2air_generate_trace_dev(eon_ctx* ctx, const eon_p2air* air, const eon_fr* inputs,
                                 uint64_t n_perms, eon_fr* trace);
/* quotient_values (eon-uni-stark/src/prover.rs:539-709) with the ProverConstraintFolder
 * accumulator (folder.rs:81-85): `lde` is the trace on the quotient domain GENERATOR * K,
 * |K| = 2^(log_n + log_qd), natural order (KzgPcs::get_evaluations_on_domain), device;
 * out[i] = sum_k alpha^(K-1-k) C_k(row i) * inv_vanishing[i], device, 2^(log_n+log_qd) Fr.
 * `alpha` is a host pointer. */
int eon_p2air_quotient_values_dev(eon_ctx* ctx, const eon_p2air* air, const eon_fr* lde,
                                  uint32_t log_n, uint32_t log_qd, const eon_fr* alpha,
                                  eon_fr* out);

/* ---- Keccak-AIR witness generation (keccak-air/src/{columns,generation}.rs) -------------------
 * One row per round of Keccak-f[1600], 24 rows per permutation, KeccakCols order: step_flags[24],
 * export, preimage[5][5][4], a[5][5][4], c[5][64], c_prime[5][64], a_prime[5][5][64],
 * a_prime_prime[5][5][4], a_prime_prime_0_0_bits[64], a_prime_prime_prime_0_0_limbs[4]; the 5x5
 * arrays y-major, a u64 as four 16-bit limbs or 64 bits, little-endian.  The constraints go through
 * the generic AIR program below like any other EonAir. */
/* NUM_KECCAK_COLS (columns.rs:120): 2633 */
uint32_t eon_keccak_air_width(void);
/* the trace height of n_hashes permutations, (24 n_hashes).next_power_of_two() (generation.rs:21);
 * 0 for n_hashes == 0 */
uint64_t eon_keccak_air_rows(uint64_t n_hashes);
/* generate_trace_rows (generation.rs:17-46): `inputs` n_hashes x 25 u64 (device), input[5x + y] the
 * lane of preimage[y][x] (the reference transmutes [u64; 25] to a state indexed [x][y]); `trace`
 * n_rows x 2633 Fr (device), on ctx's stream.  Permutations past n_hashes take the all-zero input,
 * the last one is cut to the rows that remain, export is 0.  n_rows != eon_keccak_air_rows(n_hashes)
 * is EON_E_SHAPE, and so is n_hashes == 0: the reference builds a 1-row all-zero trace there that
 * its own eval cannot read (no next row, no first step flag). */
int eon_keccak_generate_trace_dev(eon_ctx* ctx, const uint64_t* inputs, uint64_t n_hashes, eon_fr* trace,
                                  uint64_t n_rows);

/* ---- Blake3-AIR witness generation (blake3-air/src/{columns,generation}.rs) -------------------
 * One row per BLAKE3 compression (7 rounds), Blake3Cols order: inputs[16][32], chaining_values[2][4][32],
 * counter_low[32], counter_hi[32], block_len[32], flags[32], initial_row0[4][2], initial_row2[4][2],
 * full_rounds[7] (each state_prime, state_middle, state_middle_prime, state_output; a state is
 * row0[4][2], row1[4][32], row2[4][2], row3[4][32]), final_round_helpers[4][32], outputs[4][4][32]; a u32
 * as 32 bits or two 16-bit limbs, little-endian.  The constraints go through the generic AIR program
 * below like any other EonAir. */
/* NUM_BLAKE3_COLS (columns.rs): 9168 */
uint32_t eon_blake3_air_width(void);
/* generate_trace_rows (generation.rs:16-46) with generate_trace_rows_for_perm, generate_trace_row_for_round,
 * verifiable_half_round and save_state_to_trace (generation.rs:49-250): `inputs` n_hashes x 24 u32
 * (device), words 0..15 the block and 16..23 the chaining value; `trace` n_rows x 9168 Fr (device), on
 * ctx's stream.  Row k has counter = k, block_len = n_hashes, flags = 0 (generation.rs:38-43, 63-68).
 * EON_E_SHAPE: n_hashes == 0 or not a power of two (the reference asserts it, generation.rs:21-24),
 * n_rows != n_hashes, n_rows > 2^28. */
int eon_blake3_generate_trace_dev(eon_ctx* ctx, const uint32_t* inputs, uint64_t n_hashes, eon_fr* trace,
                                  uint64_t n_rows);
/* The same with the number of workgroups that share a row given: parts = 1, 2, 4, 8 or 16 (each
 * redoes the compression and stores one slice of the row), 0 = the library's choice, which is what
 * eon_blake3_generate_trace_dev takes.  The trace does not depend on it; it is there to be timed. */
int eon_diag_blake3_trace_parts(eon_ctx* ctx, const uint32_t* inputs, uint64_t n_hashes, eon_fr* trace, uint64_t n_rows,
                                uint32_t parts);

/* ---- generic AIR: quotient_values for any EonAir ---------------------------------------------
 * The constraints get_symbolic_constraints returns (eon-uni-stark/src/symbolic_builder.rs:72-126)
 * as a DAG of SymbolicExpression nodes (symbolic_expression.rs:78-145; SymbolicVariable /
 * Entry, symbolic_variable.rs:8-40), in topological order: every operand index is smaller than
 * its user's (a shared Arc is emitted once and referenced by index).  `constraints` lists the
 * root node of each constraint in assert order (the folder's constraint_index order,
 * folder.rs:81-85).  Leaves: EON_SYM_CONSTANT a = index into consts (canonical Fr);
 * EON_SYM_MAIN a = column, b = row offset (0 local, 1 next); EON_SYM_PUBLIC a = public index;
 * the three selectors (symbolic_builder.rs:205-221); EON_SYM_PREPROCESSED a = column of the
 * preprocessed trace (< the program's preprocessed width), b = row offset, a degree-1 leaf like
 * EON_SYM_MAIN (symbolic_variable.rs:8-40; the folder's preprocessed window, folder.rs:25-40,
 * prover.rs:677).  EON_SYM_PERMUTATION a = column of the permutation (LogUp running-sum) trace,
 * b = row offset, a degree-1 leaf read from a third matrix; EON_SYM_CHALLENGE a = index of a
 * permutation challenge, a degree-0 leaf (prover.rs:210-278, 630-676).  Both need a program made
 * by eon_air_program_create_lk; eon_air_program_create and eon_air_program_create_pp answer
 * EON_E_ARG to them. */
enum {
    EON_SYM_CONSTANT = 0,
    EON_SYM_MAIN = 1,
    EON_SYM_PUBLIC = 2,
    EON_SYM_IS_FIRST_ROW = 3,
    EON_SYM_IS_LAST_ROW = 4,
    EON_SYM_IS_TRANSITION = 5,
    EON_SYM_ADD = 6, /* a + b */
    EON_SYM_SUB = 7, /* a - b */
    EON_SYM_NEG = 8, /* -a */
    EON_SYM_MUL = 9, /* a * b */
    EON_SYM_PREPROCESSED = 10,
    EON_SYM_PERMUTATION = 11,
    EON_SYM_CHALLENGE = 12
};
typedef struct {
    uint32_t kind;
    uint32_t a;
    uint32_t b;
} eon_sym_node;
typedef struct eon_air_program eon_air_program;
typedef struct {
    uint32_t width;                 /* main trace width */
    uint32_t num_public_values;
    uint32_t num_constraints;
    uint32_t max_constraint_degree; /* get_max_constraint_degree (symbolic_builder.rs:46-69) */
    uint32_t num_instructions;      /* compiled program (after common-subexpression elimination) */
    uint32_t num_registers;
    uint32_t num_constants;
} eon_air_program_stats;
/* Compile the constraint DAG for a trace of `width` columns and n_public public values. */
int eon_air_program_create(eon_ctx* ctx, const eon_sym_node* nodes, uint32_t n_nodes, const eon_fr* consts,
                           uint32_t n_consts, const uint32_t* constraints, uint32_t n_constraints,
                           uint32_t width, uint32_t n_public, eon_air_program** out);
/* The same for an AIR with `preprocessed_width` preprocessed columns (the preprocessed_width
 * argument of get_symbolic_constraints, symbolic_builder.rs:72-80): EON_SYM_PREPROCESSED nodes may
 * name columns below it.  eon_air_program_create is this call with preprocessed_width = 0, so it
 * answers EON_E_ARG to every EON_SYM_PREPROCESSED node (column out of range). */
int eon_air_program_create_pp(eon_ctx* ctx, const eon_sym_node* nodes, uint32_t n_nodes, const eon_fr* consts,
                              uint32_t n_consts, const uint32_t* constraints, uint32_t n_constraints,
                              uint32_t width, uint32_t preprocessed_width, uint32_t n_public,
                              eon_air_program** out);
/* ---- LogUp lookups (lookup/src/logup.rs, lookup_traits.rs; local lookups, Challenge = Fr) -------
 * The same for an AIR with lookups: `permutation_width` running-sum columns (one per lookup,
 * LogUpGadget::num_aux_cols) and n_challenges = 2 * permutation_width challenges (num_challenges;
 * lookup with auxiliary column c uses alpha = challenges[2c], beta = challenges[2c + 1]).  The
 * nodes hold the AIR's constraints followed by the lookups' (AirLookupHandler::eval,
 * lookup_traits.rs:257-269) and, as shared nodes of the same DAG, what generate_permutation
 * evaluates per row (logup.rs:379-562): lookups[l] has n_terms consecutive entries of `terms`, each
 * the node of one tuple's denominator alpha - fold(elements, beta) and the node of its (signed)
 * multiplicity.  n_lookups is 0 (a program for eon_quotient_values_lk_dev only) or
 * permutation_width.  EON_E_ARG: a permutation column >= permutation_width, a challenge index >=
 * n_challenges, an auxiliary column >= permutation_width or used by two lookups (the reference's
 * debug assert, logup.rs:398-410), n_challenges != 2 * permutation_width, a denominator or
 * multiplicity that reaches a permutation leaf (symbolic_to_expr is unimplemented there,
 * lookup_traits.rs:408) or a row selector (the reference evaluates selectors there as unnormalised
 * 0 / 1 and warns; refused here).  With permutation_width = 0 this is eon_air_program_create_pp. */
typedef struct {
    uint32_t aux_column; /* Lookup::columns[0] */
    uint32_t n_terms;    /* element tuples = multiplicities */
} eon_lookup_desc;
typedef struct {
    uint32_t denominator;  /* node index */
    uint32_t multiplicity; /* node index */
} eon_lookup_term;
int eon_air_program_create_lk(eon_ctx* ctx, const eon_sym_node* nodes, uint32_t n_nodes, const eon_fr* consts,
                              uint32_t n_consts, const uint32_t* constraints, uint32_t n_constraints,
                              uint32_t width, uint32_t preprocessed_width, uint32_t n_public,
                              uint32_t permutation_width, uint32_t n_challenges, const eon_lookup_desc* lookups,
                              uint32_t n_lookups, const eon_lookup_term* terms, eon_air_program** out);
/* the permutation width, challenge count and lookup count the program was compiled for (0 unless
 * made by eon_air_program_create_lk) */
uint32_t eon_air_program_permutation_width(const eon_air_program* prog);
uint32_t eon_air_program_num_challenges(const eon_air_program* prog);
uint32_t eon_air_program_num_lookups(const eon_air_program* prog);
void eon_air_program_destroy(eon_air_program* prog);
/* the preprocessed width the program was compiled for (0 for eon_air_program_create) */
uint32_t eon_air_program_preprocessed_width(const eon_air_program* prog);
int eon_air_program_info(const eon_air_program* prog, eon_air_program_stats* out);
/* get_log_quotient_degree (symbolic_builder.rs:15-43): log2_ceil(max(max_degree + is_zk, 2) - 1) */
uint32_t eon_air_program_log_quotient_degree(const eon_air_program* prog, uint32_t is_zk);
/* quotient_values (eon-uni-stark/src/prover.rs:539-709) of the program: `lde` = the trace on the
 * quotient domain GENERATOR * K, |K| = 2^(log_n + log_qd), natural order, device, width columns;
 * publics = host array of n_public Fr (public_values); alpha host.  out (device, 2^(log_n+log_qd)
 * Fr) = sum_k alpha^(K-1-k) C_k(local = row i, next = row (i + 2^log_qd) mod Q, selectors of
 * selectors_on_coset, publics) * inv_vanishing[i]. */
int eon_quotient_values_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* lde, uint32_t log_n,
                            uint32_t log_qd, const eon_fr* alpha, const eon_fr* publics, uint32_t n_public,
                            eon_fr* out);
/* The same with the preprocessed trace on the same quotient domain (prover.rs:321-322:
 * get_evaluations_on_domain of the preprocessed data): `pre_lde` = 2^(log_n + log_qd) rows x
 * preprocessed_width columns, row-major, natural order, device, read through the same row pair as
 * `lde` (local = row i, next = row (i + 2^log_qd) mod Q; vertically_packed_row_pair,
 * prover.rs:677, matrix/src/lib.rs:392-411).  pre_lde must be non-NULL exactly when the program's
 * preprocessed width is > 0 (EON_E_ARG otherwise); eon_quotient_values_dev is this call with
 * pre_lde = NULL and answers EON_E_ARG for a program with preprocessed columns. */
int eon_quotient_values_pp_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* lde,
                               const eon_fr* pre_lde, uint32_t log_n, uint32_t log_qd, const eon_fr* alpha,
                               const eon_fr* publics, uint32_t n_public, eon_fr* out);

/* The same with the permutation trace on the same quotient domain (prover.rs:317-319, 630-670):
 * `perm_lde` = 2^(log_n + log_qd) rows x permutation_width columns, read through the same row pair,
 * and `challenges` = host array of n_challenges Fr (the program's count, EON_E_SHAPE otherwise).
 * perm_lde must be non-NULL exactly when the program has permutation columns (EON_E_ARG otherwise);
 * eon_quotient_values_pp_dev and eon_quotient_values_dev answer EON_E_ARG for such a program. */
int eon_quotient_values_lk_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* lde,
                               const eon_fr* pre_lde, const eon_fr* perm_lde, uint32_t log_n, uint32_t log_qd,
                               const eon_fr* alpha, const eon_fr* publics, uint32_t n_public,
                               const eon_fr* challenges, uint32_t n_challenges, eon_fr* out);
/* eon_quotient_values_dev on a block of rows, from a WINDOW of the LDE (the column-sharded prove,
 * below): `window` = the n_rows + 2^log_qd LDE rows (row0 + j) mod Q, j < n_rows + 2^log_qd,
 * Q = 2^(log_n + log_qd), row-major, width columns, device.  out[t] (device, n_rows Fr), t < n_rows,
 * is eon_quotient_values_dev's out[row0 + t] bit for bit: local = window row t, next = window row
 * t + 2^log_qd, the selectors and inv_vanishing of row row0 + t.  row0 + n_rows <= Q (EON_E_SHAPE
 * otherwise); n_rows = 0 does nothing.  A program with preprocessed or permutation columns is
 * EON_E_ARG. */
int eon_quotient_values_rows_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* window, uint32_t log_n,
                                 uint32_t log_qd, uint64_t row0, uint64_t n_rows, const eon_fr* alpha,
                                 const eon_fr* publics, uint32_t n_public, eon_fr* out);
/* LogUpGadget::generate_permutation (logup.rs:379-562) for a program with a lookup description:
 * `trace` = the main trace (device, height x width, height a power of two), `pre_trace` = the
 * preprocessed trace on the same (trace) domain, publics / challenges host arrays, perm_out =
 * height x permutation_width (device, row-major).  Row i evaluates every tuple's denominator and
 * multiplicity with local = row i, next = row (i + 1) mod height; contribution[i][l] = sum over
 * lookup l's tuples of multiplicity / denominator (one field inversion per row, Montgomery's
 * trick); perm[0][c] = 0 and perm[i + 1][c] = perm[i][c] + contribution[i][l] in l's auxiliary
 * column c.  The last row's contribution is computed and not stored.  A zero denominator on any
 * row (the reference panics, field/src/batch_inverse.rs:17-18) is EON_E_ARG with a message naming
 * the lookup; perm_out is then unspecified.  pre_trace must be non-NULL when a tuple reads a
 * preprocessed column and NULL when the program has no preprocessed columns (EON_E_ARG).  The term
 * program's register file follows eon_quotient_values_lk_dev's rule (LDS, or global for very large
 * programs and with EON_AIR_REGS=global). */
int eon_lookup_permutation_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* trace,
                               const eon_fr* pre_trace, uint64_t height, const eon_fr* publics, uint32_t n_public,
                               const eon_fr* challenges, uint32_t n_challenges, eon_fr* perm_out);

/* check_constraints (eon-uni-stark/src/check_constraints.rs:22-101), what prove_with_preprocessed
 * runs in every debug build right after the permutation trace (prover.rs:252-262), on the device:
 * every trace row i runs the program with local = row i, next = row (i + 1) mod height (:41-47) of
 * the main, the preprocessed (:55-69) and the permutation (:71-79) trace, all on the TRACE domain,
 * with is_first_row / is_last_row / is_transition the field elements 1 / 0 for i == 0,
 * i == height - 1, i != height - 1 (:88-90; not the coset selectors), and every constraint -- the
 * AIR's, then the lookups', in assert order -- is tested for zero (assert_zero, :165-173).  The
 * reference panics at the first failure, "Constraint failed at row R: expected zero, got V"; here
 * every (row, constraint) is evaluated and the report carries that first failure -- the lowest row,
 * then the lowest constraint on it -- with its value, plus the counts. */
typedef struct {
    uint64_t failures;             /* (row, constraint) pairs whose value is nonzero */
    uint64_t row;                  /* first failing row; valid when failures > 0 */
    uint32_t constraint;           /* first failing constraint on that row, assert order */
    uint32_t failing_constraints;  /* constraints that fail on at least one row */
    eon_fr   value;                /* that constraint's value on that row, canonical */
} eon_constraint_report;
/* `trace` = height x width (device, row-major), `pre_trace` = height x preprocessed_width and
 * `perm_trace` = height x permutation_width likewise; publics / challenges host arrays;
 * `per_constraint` (host, num_constraints entries, nullable) receives the number of rows on which
 * each constraint fails; *out (host) the report.  EON_OK whether or not a constraint fails: the
 * report says which (failures == 0: the trace satisfies the AIR; row, constraint and value are then
 * zero).  The result is synchronous: the call returns after the device has finished, like the
 * zero-denominator flag of eon_lookup_permutation_dev.  As eon_quotient_values_lk_dev: pre_trace
 * must be non-NULL exactly when the program has preprocessed columns (the reference takes
 * air.preprocessed_trace(), :39) and perm_trace exactly when it has permutation columns (:25; both
 * EON_E_ARG otherwise); n_public (:27) and n_challenges (:26) must be the program's (EON_E_SHAPE);
 * a public value or challenge that is not canonical is EON_E_ARG; height (:38) must be a power of
 * two in [1, 2^28] (EON_E_SHAPE; height 1 wraps next onto the row itself, :42); a program created
 * on another context is EON_E_ARG.  A program with zero constraints reports failures = 0.  The
 * register file follows eon_quotient_values_lk_dev's rule (LDS, or global for very large programs
 * and with EON_AIR_REGS=global). */
int eon_check_constraints_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* trace,
                              const eon_fr* pre_trace, const eon_fr* perm_trace, uint64_t height,
                              const eon_fr* publics, uint32_t n_public, const eon_fr* challenges,
                              uint32_t n_challenges, uint32_t* per_constraint, eon_constraint_report* out);

/* The constraints at ONE out-of-domain point: the evaluation of verify_constraints
 * (eon-uni-stark/src/verifier.rs:101-152), the only part of the verifier that needs the AIR.  The
 * program runs once on opened values: `local` / `next` = width Fr each (the trace at zeta and
 * zeta h), `pre_local` / `pre_next` = preprocessed_width Fr each, `perm_local` / `perm_next` =
 * permutation_width Fr each -- six separate DEVICE arrays of canonical Fr, not rows of one matrix.
 * The selectors are selectors_at_point(zeta) of the trace domain of size 2^log_n
 * (commit/src/domain.rs:237-246): with Z_H = zeta^N - 1 and h the domain's generator,
 * is_first_row = Z_H / (zeta - 1), is_last_row = Z_H / (zeta - h^-1), is_transition = zeta - h^-1,
 * inv_vanishing = 1 / Z_H, computed exactly on the host.  Every constraint -- the AIR's, then the
 * lookups', in assert order -- is folded as acc = acc alpha + C (folder.rs:188-190).
 *   out[0] (host) = the folded accumulator, out[1] = folded * inv_vanishing -- the side the verifier
 *   compares with quotient(zeta); both canonical, ABI form.  A program with zero constraints gives 0.
 * `zeta`, `alpha`, `publics`, `challenges` are host pointers.  Synchronous, like
 * eon_check_constraints_dev.  pre_* must be non-NULL exactly when the program has preprocessed
 * columns and perm_* exactly when it has permutation columns (EON_E_ARG); n_public and n_challenges
 * must be the program's (EON_E_SHAPE); a zeta, alpha, public value or challenge that is not canonical
 * is EON_E_ARG; log_n > 28 is EON_E_SHAPE; a program created on another context is EON_E_ARG.  Where
 * the reference panics on the inverse of zero -- zeta = 1, zeta = h^-1 or Z_H(zeta) = 0 -- the call
 * returns EON_E_ARG.  One lane runs the program (a latency-bound dependent chain); the register file
 * follows eon_quotient_values_lk_dev's rule (LDS, or global for very large programs and with
 * EON_AIR_REGS=global). */
int eon_air_eval_at_point_dev(eon_ctx* ctx, const eon_air_program* prog, uint32_t log_n, const eon_fr* zeta,
                              const eon_fr* alpha, const eon_fr* local, const eon_fr* next, const eon_fr* pre_local,
                              const eon_fr* pre_next, const eon_fr* perm_local, const eon_fr* perm_next,
                              const eon_fr* publics, uint32_t n_public, const eon_fr* challenges,
                              uint32_t n_challenges, eon_fr* out);

/* The same evaluation for n proofs of one program in ONE launch (kernel k_air_points: block i is
 * proof i, one lane live as above, so the n dependent chains run side by side).  `rows` is a DEVICE
 * array of n x row_stride canonical Fr; row i holds proof i's opened values as
 * local | next | pre_local | pre_next | perm_local | perm_next (width, width, preprocessed_width x 2,
 * permutation_width x 2; row_stride at least their sum, EON_E_SHAPE otherwise).  Host arrays:
 * log_n[n], zeta[n], alpha[n], publics (n x the program's public value count), challenges
 * (n x n_challenges), out (2 n: out[2 i] the folded value of proof i, out[2 i + 1] the quotient
 * side).  Every pair is bit-identical to eon_air_eval_at_point_dev on the same inputs.  The errors
 * are that call's; one caused by proof i's inputs (a zeta_i on its trace domain, a value that is not
 * canonical, log_n[i] > 28) has a message that starts "point i: ".  n = 0 writes nothing.  The
 * register file follows the same rule: each block its own LDS, or row i of n rows of the global
 * buffer. */
int eon_air_eval_at_points_dev(eon_ctx* ctx, const eon_air_program* prog, uint32_t n, const uint32_t* log_n,
                               const eon_fr* zeta, const eon_fr* alpha, const eon_fr* rows, uint64_t row_stride,
                               const eon_fr* publics, const eon_fr* challenges, uint32_t n_challenges, eon_fr* out);

/* out[i] = sum_{j<k} coeffs[j] * in[j * rows + i] (device in/out, host coeffs, 1 <= k <= 64):
 * the combine step of the lane-sharded quotient -- every rank all-gathers the
 * shards' partial quotients and weights shard g by alpha^(K_lane * (VECTOR_LEN - lane_end_g)). */
int eon_fr_lincomb_dev(eon_ctx* ctx, const eon_fr* in, uint32_t k, uint64_t rows,
                       const eon_fr* coeffs, eon_fr* out);

/* out[i] = scale * sum_{j<width} gamma^j * mat[i*width + j] (device mat/out, host gamma/scale): the
 * gamma-fold of a row-major rows x width matrix into one column, F = sum_j gamma^j f_j of the
 * batched KZG opening (eon_prove.h, EON_OPENING_BATCHED).  scale NULL = one.  out is canonical and
 * must not overlap mat (EON_E_ARG).  gamma and scale follow `point` of eon_eval_columns_dev: host
 * pointers to canonical Fr, EON_E_ARG otherwise.  width == 1 is a (scaled) copy; rows == 0 writes
 * nothing; width == 0 writes rows zeros.  A NULL pointer that would be read or written is EON_E_ARG.
 * Any width runs (a wave walks its row in 64-column tiles; 9168, the Blake3-AIR's, is 144 of them):
 * there is no upper limit short of rows * width * 32 overflowing 64 bits (EON_E_SHAPE).  The powers
 * gamma^0..gamma^63 are made on the device per call as Shoup constants; asynchronous on the
 * context's stream. */
int eon_fr_fold_columns_dev(eon_ctx* ctx, const eon_fr* mat, uint64_t rows, uint32_t width,
                            const eon_fr* gamma, const eon_fr* scale, eon_fr* out);

/* ---- four-step NTT across ranks (BASELINE configs[4]) ------------------------
 * Step 2 + the local half of step 3 of a size-2^log_n forward DFT split as N1 x N2
 * (N1 = 2^log_n1): y is the rank's N1 x cols block (columns col0 .. col0+cols of the N1 x N2 view
 * x[N2 i1 + i2], after a size-N1 eon_dft_batch_dev over its columns); writes
 * send[h][i2][k1'] = y[h N1/parts + k1'][i2] * w_N^((col0 + i2)(h N1/parts + k1')), i.e. `parts`
 * contiguous cols x (N1/parts) blocks, one per destination rank (device pointers). */
int eon_fourstep_twiddle_pack_dev(eon_ctx* ctx, const eon_fr* y, uint32_t log_n, uint32_t log_n1,
                                  uint64_t col0, uint32_t cols, uint32_t parts, eon_fr* send);

/* The whole sharded forward DFT: dft_batch (dft/src/traits.rs:61, natural order; the reference
 * has no multi-GPU path -- this is SURVEY.md 8(e)'s four-step scheme) of ONE column of N = 2^log_n
 * elements spread over the collective's `world` ranks (every rank calls with the same log_n,
 * layout and collective; world must divide N2 and N1, N1 = 2^ceil(log_n / 2), N2 = N / N1).
 *   in:  the rank's N1 x (N2/world) row-major block of the N1 x N2 view x[N2 i1 + i2]: columns
 *        [rank N2/world, (rank+1) N2/world) -- i.e. in[i1 C + c] = x[N2 i1 + rank C + c];
 *   out: N/world elements in `layout` (EON_FOURSTEP_NATURAL or EON_FOURSTEP_TRANSPOSED).
 * Steps: size-N1 column DFTs, twiddles w_N^(i2 k1) fused with the pack per destination,
 * all_to_all, size-N2 DFTs, and for the natural layout a second all_to_all plus a block
 * interleave.  coll NULL = the context's bound collective (eon_ctx_set_collective), or one rank.
 * Device pointers; `in` is not modified.  Synchronous with respect to the collective calls. */
int eon_fourstep_dft_dev(eon_ctx* ctx, const eon_fr* in, eon_fr* out, uint32_t log_n, int layout,
                         const eon_collective* coll);

/* G1::multi_exp (bn254/src/curve.rs:158-179) of ONE MSM whose terms are split over the ranks by
 * contiguous range (SURVEY.md 8(e), configs[4] (ii)): every rank passes its bases (over its own
 * range) and its n_local scalars (device pointer); each runs a full Pippenger, the `world` affine
 * partial points are all-gathered (64 B per rank) and summed (EC additions -- not an RCCL
 * reduction).  Every rank receives the same result in *out (host).  coll NULL = the context's
 * bound collective, or one rank. */
int eon_msm_sharded_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* scalars, uint64_t n_local,
                        const eon_collective* coll, eon_g1_affine* out);

/* ---- column-sharded prove of a generic AIR (eon_prove_air_sharded, eon_prove.h) ----------------
 * The partition.  Columns: rank g of `world` owns the contiguous range [c0, c0 + wl) of the `width`
 * columns, in rank order, the first width % world ranks one column wider (wmax = ceil(width /
 * world)).  Rows: with q_rows = Q quotient-domain rows and R = ceil(Q / world), rank r evaluates rows
 * [row0, row0 + n_rows) = [min(Q, r R), min(Q, (r+1) R)), possibly none.  Its window is the R + S
 * rows (r R + j) mod Q, j < R + S, where S = next_step = 2^log_qd.  Both are host-only and need no
 * device; world = 0, rank >= world, and for the columns world > width, are EON_E_ARG. */
int eon_shard_column_range(uint32_t width, uint32_t world, uint32_t rank, uint32_t* c0, uint32_t* wl);
int eon_shard_row_range(uint64_t q_rows, uint32_t world, uint32_t rank, uint64_t* row0, uint64_t* n_rows);
/* The two copies around the exchange (device pointers, on the context's stream).
 *   pack:   lde = rank's q_rows x wl row-major LDE of its own columns; send receives `world` blocks
 *           of (R + S) x wmax elements: block h, row j = LDE row (h R + j) mod Q, columns past wl zero.
 *   (the caller's all_to_all, blocks of (R + S) wmax 32 bytes: recv block g = rank g's send block for
 *   this rank)
 *   unpack: recv = those `world` blocks; window receives the (R + S) x width row-major matrix of
 *           window rows, columns [c0(g), c0(g) + wl(g)) from block g.
 * q_rows and next_step powers of two, next_step <= q_rows <= 2^28 (EON_E_SHAPE); world > width is
 * EON_E_ARG. */
int eon_shard_pack_rows_dev(eon_ctx* ctx, const eon_fr* lde, uint64_t q_rows, uint32_t width, uint32_t world,
                            uint32_t rank, uint64_t next_step, eon_fr* send);
int eon_shard_unpack_cols_dev(eon_ctx* ctx, const eon_fr* recv, uint64_t q_rows, uint32_t width, uint32_t world,
                              uint64_t next_step, eon_fr* window);

/* ---- test SRS (setup, not prove time) --------------------------------------------------------
 * init_srs_unsafe's g1_powers (kzg/src/params.rs:123-139): out[i] = alpha^i * G1::generator(),
 * affine, i < n.  `alpha` is a host pointer; `out` host (eon_g1_srs_powers) or device (_dev). */
int eon_g1_srs_powers(eon_ctx* ctx, const eon_fr* alpha, uint64_t n, eon_g1_affine* out);
int eon_g1_srs_powers_dev(eon_ctx* ctx, const eon_fr* alpha, uint64_t n, eon_g1_affine* out);

/* ---- a supplied SRS (KzgPcs::from_srs, kzg/src/pcs.rs:170-175) -------------------------------
 * The reference serialises an SRS's G1 powers as G1Affine::to_bytes (bn254/src/curve.rs:84-98):
 * 32 bytes per point, the canonical (not Montgomery) x little-endian, bit 7 of byte 31 = the
 * canonical y is odd, bit 6 of byte 31 = the identity.  Loading one is a square root in Fq per
 * point, and accepting one without its trapdoor is a pairing check; both run on the device.
 *
 * Every check reports through an eon_srs_report: `reason` is EON_SRS_OK or why the SRS was
 * rejected, `index` the LOWEST offending point index for the per-point reasons (ENCODING,
 * NOT_CANONICAL, NOT_ON_CURVE, IDENTITY; when several points are bad, the reason is that point's)
 * and 0 otherwise.  The index is a 64-bit vector atomic minimum over (index, reason) on the
 * device, so it does not depend on scheduling.  A rejected SRS returns EON_E_SRS with the report
 * filled; EON_OK leaves reason = EON_SRS_OK.  Other negative codes leave the report zeroed. */
typedef struct {
    uint32_t reason;
    uint32_t pad;
    uint64_t index;
} eon_srs_report;
enum {
    EON_SRS_OK = 0,
    EON_SRS_ENCODING = 1,         /* identity flag with other bits set */
    EON_SRS_NOT_CANONICAL = 2,    /* a coordinate >= q */
    EON_SRS_NOT_ON_CURVE = 3,     /* x^3 + 3 is no square (compressed), y^2 != x^3 + 3 (affine) */
    EON_SRS_IDENTITY = 4,         /* an SRS power that is the point at infinity */
    EON_SRS_G0_NOT_GENERATOR = 5, /* g1_powers[0] != G1::generator() */
    EON_SRS_G2_INVALID = 6,       /* g2_alpha not canonical, off the twist, the identity or outside
                                     the order-r subgroup */
    EON_SRS_STRUCTURE = 7         /* the points are not consecutive powers of g2_alpha's scalar */
};
/* The exact inverse of eon_g1_to_bytes (eon_prove.h), one point per lane: `bytes` = n x 32 bytes
 * (device, 4-byte aligned), `out` = n affine points, canonical Montgomery (device).  Per point:
 * identity flag set -> every other bit must be zero (else ENCODING) and the output is (0,0);
 * otherwise the flags are cleared, x >= q is NOT_CANONICAL, t = x^3 + 3, y = t^((q+1)/4) (q = 3 mod
 * 4; one fixed 2-bit-window chain, the same for every lane), y^2 != t is NOT_ON_CURVE, and the
 * root with the flagged parity is taken.  A rejected point is written as (0,0).  The report is
 * read back before the call returns (it synchronizes the context's stream); n == 0 is valid.
 * eon_g1_decompress is the same on host arrays. */
int eon_g1_decompress_dev(eon_ctx* ctx, const uint8_t* bytes, uint64_t n, eon_g1_affine* out,
                          eon_srs_report* report);
int eon_g1_decompress(eon_ctx* ctx, const uint8_t* bytes, uint64_t n, eon_g1_affine* out, eon_srs_report* report);
/* G1Affine::to_bytes on the device, the exact inverse of eon_g1_decompress_dev and byte for byte
 * eon_g1_to_bytes (eon_prove.h) of every accepted point, one point per lane: `pts` = n affine points,
 * Montgomery (device, 16-byte aligned), `bytes` = n x 32 bytes (device, 16-byte aligned).  Per point:
 * (0,0) -> 31 zero bytes and 0x40; otherwise both coordinates leave Montgomery form, x is stored
 * little-endian and bit 7 of byte 31 is set when the canonical y is odd.  A coordinate >= q is
 * NOT_CANONICAL (lowest index reported, EON_E_SRS) and that point is written as 32 zero bytes.  No
 * curve test: to_bytes has none.  Synchronous like eon_g1_decompress_dev; n == 0 is valid.
 * eon_g1_compress is the same on host arrays. */
int eon_g1_compress_dev(eon_ctx* ctx, const eon_g1_affine* pts, uint64_t n, uint8_t* bytes, eon_srs_report* report);
int eon_g1_compress(eon_ctx* ctx, const eon_g1_affine* pts, uint64_t n, uint8_t* bytes, eon_srs_report* report);
/* Uncompressed SRS powers (device): both coordinates < q (else NOT_CANONICAL), not (0,0)
 * (IDENTITY), y^2 = x^3 + 3 (else NOT_ON_CURVE).  G1 has cofactor 1, so on the curve is in the
 * group.  Synchronous like eon_g1_decompress_dev. */
int eon_g1_validate_dev(eon_ctx* ctx, const eon_g1_affine* pts, uint64_t n, eon_srs_report* report);
/* Accept bases[0..n) with g2_alpha as an SRS without knowing alpha (n >= 1, n <= the bases' length):
 *   1. bases[0] == G1::generator(), else G0_NOT_GENERATOR;
 *   2. g2_alpha canonical, on the twist, not the identity and [r - 1] Q == -Q (eon_g2_mul's plain
 *      double-and-add with complete case handling: it assumes nothing about Q's order), else
 *      G2_INVALID;
 *   3. for n > 1, with A = sum_{i<n-1} rho^i G_i and B = sum_{i<n-1} rho^i G_(i+1) -- both from ONE
 *      column MSM (eon_msm_g1_columns_dev's) over the bases' own tables, of the n x 2 matrix with
 *      columns (rho^0 .. rho^(n-2), 0) and (0, rho^0 .. rho^(n-2)) built on the device --
 *      e(A, g2_alpha) e(-B, G2) == 1 through eon_multi_pairing, else STRUCTURE.
 * If G_(i+1) != alpha G_i for some i the check passes only when rho is a root of a nonzero
 * polynomial of degree < n: a chance below n / r for a uniformly random rho, which the caller
 * must draw AFTER the SRS is fixed.  rho (host, Montgomery ABI form) zero or not canonical is
 * EON_E_ARG.  The per-point checks above are the caller's (the MSM needs curve points).  Host
 * outputs, synchronous. */
int eon_kzg_srs_check(eon_ctx* ctx, const eon_msm_bases* bases, uint64_t n, const eon_g2_affine* g2_alpha,
                      const eon_fr* rho, eon_srs_report* report);

/* ---- verifier pairings (setup / verify, not prove time) --------------------
 * All host pointers, synchronous.  G1 / G2 inputs must be canonical and on their curves
 * (EON_E_ARG otherwise).
 *
 * eon_g2_mul: out = k * base (base NULL = G2::generator()); init_srs_unsafe's
 *   g2_alpha = [alpha] G2 (kzg/src/params.rs:123-139), G2::mul_scalar (bn254/src/curve.rs).
 * eon_multi_pairing: out = prod_i e(p[i], q[i]) (multi_pairing, bn254/src/curve.rs:439-452;
 *   pairing, :429-436, is n = 1): the optimal-ate Miller loops and one final exponentiation; the
 *   identity of Gt (Fq12 one) for n = 0.
 * eon_kzg_verify_batch: *ok = 1 iff prod_i e(C_i - v_i G1, G2) e(-W_i, g2_alpha - z_i G2) is the
 *   identity -- verify_batch (kzg/src/util.rs:245-292; for n = 1 verify_single, :150-168, whose
 *   e(C - vG1, G2) == e(W, g2_alpha - zG2) is the same condition).  *ok = 0 is the reference's
 *   Err(KzgError::ProofShapeMismatch); n = 0 is Ok.  Pairs sharing a G2 argument are merged by
 *   bilinearity before the Miller loops (one pairing per distinct opening point, plus one). */
int eon_g2_mul(eon_ctx* ctx, const eon_g2_affine* base, const eon_fr* k, eon_g2_affine* out);
int eon_multi_pairing(eon_ctx* ctx, const eon_g1_affine* p, const eon_g2_affine* q, uint64_t n, eon_fq12* out);
int eon_kzg_verify_batch(eon_ctx* ctx, const eon_g1_affine* commitments, const eon_g1_affine* witnesses,
                         const eon_fr* values, const eon_fr* points, uint64_t n, const eon_g2_affine* g2_alpha,
                         int* ok);

/* Many independent checks in one pass.  `seg` (host) holds nseg + 1 ascending offsets with
 * seg[0] = 0: segment s is items [seg[s], seg[s + 1]) of the arrays, seg[nseg] their length.  One
 * Miller launch covers every pair; the final exponentiation runs one block per segment, so every
 * segment keeps its own Gt product (no random weights across segments).  nseg = 0 writes nothing;
 * seg not ascending from 0 is EON_E_ARG; more than 2^24 segments is EON_E_SHAPE.
 *
 * eon_multi_pairing_many: out[s] = prod_{i in segment s} e(p[i], q[i]), each limb for limb what
 *   eon_multi_pairing gives for that slice (the identity of Gt for an empty segment).  Arguments
 *   are validated as in eon_multi_pairing (any bad point fails the call).
 * eon_kzg_verify_batch_many: segment s holds the openings of one verify_batch.  status[s] = 1 when
 *   its product is the identity (an empty segment is 1), 0 when it is not, and EON_E_ARG when the
 *   segment holds a commitment or witness that is not a G1 point or a value or point that is not a
 *   canonical Fr -- per segment: such a segment is left out of the device work, the others are
 *   still checked and the call returns EON_OK (eon_kzg_verify_batch on that segment alone gives
 *   the message).  The openings are grouped by distinct point per segment; k_vb_sums / k_vb_pairs
 *   run sum_s (G_s + 1) blocks in one launch each.  A null or invalid g2_alpha fails the call. */
int eon_multi_pairing_many(eon_ctx* ctx, const eon_g1_affine* p, const eon_g2_affine* q, const uint64_t* seg,
                           uint32_t nseg, eon_fq12* out);
int eon_kzg_verify_batch_many(eon_ctx* ctx, const eon_g1_affine* commitments, const eon_g1_affine* witnesses,
                              const eon_fr* values, const eon_fr* points, const uint64_t* seg, uint32_t nseg,
                              const eon_g2_affine* g2_alpha, int* status);

/* ---- KzgMmcs: Mmcs<Fr> over the same SRS (kzg/src/mmcs.rs) -----------------------------------
 * A batch of matrices of mixed heights (any height >= 1, powers of two or not), every column a
 * polynomial in COEFFICIENT form.  commit is eon_msm_g1_columns_dev per matrix (commit_matrix,
 * mmcs.rs:155-165).  A query index opens, in matrix m, the point z = Fr::new(local_index):
 *
 * eon_kzg_mmcs_local_index: the index mapping of open_batch and verify_batch (mmcs.rs:213-218,
 *   :272-277): with log2_x = next_power_of_two(x).trailing_zeros(),
 *   local = (log2_max >= log2_h ? index >> (log2_max - log2_h) : index) % height.  Pure host
 *   function, no context.  height == 0 returns UINT64_MAX (the reference divides by zero).
 *
 * eon_kzg_mmcs_open_dev: open_batch (mmcs.rs:196-236) for nidx indices at once.  `mats` (host array
 *   of nmats descriptors; coeffs DEVICE pointers, row-major height x width), max_height = the largest
 *   height among them.  With W = the sum of the widths, `values` (host, nidx x W Fr) and `witnesses`
 *   (host, nidx x W points) are filled matrices in order, columns in order:
 *   values[q * W + off_m + j] = f_j(z), witnesses[...] = commit_column(quotient_and_eval(column j,
 *   z).0) over srs[0..height-1).  Per matrix the distinct local indices over all queries are
 *   computed once (short matrices map many queries to one row) and copied to every query that uses
 *   them: eon_quotient_and_eval_columns_multi_dev over the distinct points, then one column MSM over
 *   the side-by-side quotients.  The distinct points run in groups whose quotient scratch is at most
 *   1 GiB (a single point above that still runs; EON_MMCS_GROUP_BYTES, read at each call, sets
 *   another cap -- the tests' way to several groups at small shapes).  height == 1: the witness is the identity and the
 *   value c_0.  height == 0 is EON_E_SHAPE (the reference panics), height > eon_msm_bases_len(srs)
 *   -- ensure_supported(height - 1) -- EON_E_DEGREE_TOO_LARGE.  Synchronous: returns with the host
 *   arrays filled.
 *
 * eon_kzg_mmcs_verify_batch: verify_batch (mmcs.rs:242-294) for one index.  `commitments`, `values`
 *   and `witnesses` (host) hold W entries each, laid out by `heights` / `widths` (nmats entries) as
 *   above.  Per matrix ensure_supported(height - 1) against max_degree (EON_E_DEGREE_TOO_LARGE;
 *   height == 0 is EON_E_SHAPE), then the (commitment, witness, value, Fr::new(local_index)) list
 *   goes to one eon_kzg_verify_batch.  *ok = 0 is the reference's Err(ProofShapeMismatch). */
typedef struct {
    const eon_fr* coeffs; /* device */
    uint64_t height;
    uint32_t width;
} eon_mmcs_matrix;
uint64_t eon_kzg_mmcs_local_index(uint64_t max_height, uint64_t height, uint64_t index);
int eon_kzg_mmcs_open_dev(eon_ctx* ctx, const eon_msm_bases* srs, const eon_mmcs_matrix* mats, uint32_t nmats,
                          const uint64_t* indices, uint32_t nidx, eon_fr* values, eon_g1_affine* witnesses);
int eon_kzg_mmcs_verify_batch(eon_ctx* ctx, const eon_g1_affine* commitments, const uint64_t* heights,
                              const uint32_t* widths, uint32_t nmats, uint64_t index, const eon_fr* values,
                              const eon_g1_affine* witnesses, uint64_t max_degree,
                              const eon_g2_affine* g2_alpha, int* ok);

#ifdef __cplusplus
}
#endif
#endif /* EON_H */
