// Pippenger multi-scalar multiplication on BN254 G1 for gfx950.
//
// Replaces G1::multi_exp (bn254/src/curve.rs:158-179 -> halo2curves::msm::msm_best) and the KZG
// column commitment commit_column (kzg/src/util.rs:37-40).  The value sum_i s_i * P_i is unique,
// so the result (returned in affine form) is bit-identical to the reference's.
//
// Pipeline (all on device; each step's kernels and host code are in the file named, the batch and
// the constants they share in msm_batch.h, the bases object in msm_bases.hip, and this file holds
// the host pipeline over the batches of a call, the prepared-scalars handle and the C API):
//  msm_digits.hip
//   1. k_msm_digits     scalars (Montgomery) -> canonical -> signed c-bit digits; one
//                       (bucket key, point reference | sign) pair per nonzero digit.
//   2. radix sort       radix_sort_pairs (sort.hip: stable LSD, 8-bit digits, LDS-ranked tiles
//                       with a decoupled look-back) on the low c key bits of the
//                       group-major pairs: buckets b' = magnitude * groups + group, zero digits
//                       last (see k_msm_digits).
//   3. k_bucket_start   bucket boundaries in the sorted pairs.
//   4. pieces           a piece is the part of a bucket inside one chunk (2^log_chunk aligned
//                       sorted pairs); exclusive scan of the per-bucket piece counts.  The counts
//                       read back, the batch's plan is decided once (batch_counts): its reduction
//                       route of step 6-7 and the form of its piece sums.
//  msm_pieces.hip
//   5. k_piece_sum29    one thread per chunk of sorted pairs (every lane does the same number of
//                       XYZZ mixed additions of affine bases, radix 2^29), flushing a partial per
//                       piece.  Column batches (>= 64 groups, no skew) instead give every lane one
//                       whole bucket, 64 buckets of nearly equal length per wave
//                       (k_bucket_order at sort time, k_piece_sum_bucket29): one piece per bucket.
//  msm_reduce.hip
//   6. k_partial_combine levels of <= PIECE-way sums until each bucket holds one partial
//                       (log-depth under any skew, e.g. all-equal scalars), k_bucket_final.
//   7. k_bucket_reduce29 sum_d d * B_d per group: T_j / U_j the plain / locally weighted sums of
//      (k_seg_level) /  segment j (SEG buckets, by running sums), then
//      k_group_finish   sum_j U_j + SEG sum_j j T_j + sum_j T_j per group (deferred to one launch
//                       per call).  Batches with < 64 groups (a single MSM) use the shorter-chain
//                       k_segment_sum (running sums + lo * run) + k_tree_sum instead: there
//                       latency, not additions, sets the time.
//   8. k_window_horner  (per-window buckets only) sum_w 2^(c*w) G_w per MSM; batched affine.
//
// Batched mode (eon_msm_g1_columns*): one pipeline run handles many MSMs at once -- the columns
// of a row-major coefficient matrix, as KzgPcs::commit commits every column against the same
// SRS prefix (kzg/src/pcs.rs:244-251) -- with the column index in the high bits of the key.
//
// Fixed-base mode (eon_msm_bases_create with EON_MSM_PRECOMPUTE; the KZG SRS): the bases object
// stores 2^(c*w) * P_i in affine for every window w, so every window's digits land in ONE bucket
// set (groups = 1): no per-window bucket reduction and no serial doubling chain at the end.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "msm_batch.h"

using namespace eon;

// Prepared scalars: every batch's digit pairs sorted once and kept on device, so that MSMs of the
// same scalar columns against other bases objects of the same window layout skip the digit
// extraction and the sort (KzgPcs: the SRS for the commitment, then the opening bases H(z) of
// every opening point, kzg/src/pcs.rs:244-251,297-330).  The scalars themselves are not retained.
struct eon_msm_scalars {
    eon_ctx* ctx = nullptr;
    uint64_t n = 0;
    uint32_t width = 0;
    eon::MsmLayout layout;
    std::vector<eon::Batch> batches;
    std::vector<eon::SortedBufs> sorted;
    // diagnostics only (eon_diag_msm_g1_prepare_active_dev): digitise a single column's active
    // windows as the unprepared single MSM does, so that its batch can be read back; false for every
    // handle the product path makes
    bool active_windows = false;
    // buffers go back to the context's cache (caller holds ctx->mu)
    ~eon_msm_scalars() {
        constexpr size_t CAP = 48ull << 30;  // MSM_SORTED_CACHE_CAP
        size_t cached = 0;
        if (ctx)
            for (const auto& sb : ctx->sorted_cache) cached += sb.bytes();
        for (auto& sb : sorted) {
            if (ctx && cached + sb.bytes() <= CAP) {
                cached += sb.bytes();
                ctx->sorted_cache.push_back(std::move(sb));
                sb = eon::SortedBufs{};
            } else {
                sb.release();
            }
        }
    }
};

namespace eon {

static eon_g1_affine g1_to_abi(const G1Affine& a) {
    eon_g1_affine r;
    for (int i = 0; i < 4; i++) {
        r.x[i] = (uint64_t)a.x.v[2 * i] | (uint64_t)a.x.v[2 * i + 1] << 32;
        r.y[i] = (uint64_t)a.y.v[2 * i] | (uint64_t)a.y.v[2 * i + 1] << 32;
    }
    return r;
}

// digit pairs per column batch: 2^29 (the prove's 1312 columns in 6 batches of <= 256, a rank's
// 164 of the 8-way sharded prove in one): fewer, larger piece-sum launches than 2^28 -- prove
// -0.5 %, emulated 8-rank prove -1 % (profiles/r05/s23, s24; 2^30 measured the same)
constexpr uint32_t MSM_BATCH_LOG_PAIRS = 29;
static MsmLayout msm_layout(const eon_msm_bases* b, uint64_t n, uint32_t width) {
    MsmLayout L;
    L.precomputed = bases_precomputed(b);
    L.c = L.precomputed ? bases_window(b) : choose_c(n, false);
    L.W = (255 + L.c - 1) / L.c;
    // columns per batch: keep the digit pairs of one batch at <= 2^MSM_BATCH_LOG_PAIRS (8 GiB of
    // sort buffers at 2^29)
    uint64_t cpb = (1ull << MSM_BATCH_LOG_PAIRS) / (n * L.W);
    if (cpb < 1) cpb = 1;
    const uint64_t max_groups = L.precomputed ? cpb : cpb * L.W;
    if (max_groups > 65535) cpb = L.precomputed ? 65535 : 65535 / L.W;
    // equal batches (164 columns -> 82 + 82, not 128 + 36): the two streams overlap evenly
    const uint64_t n_batches = (width + cpb - 1) / cpb;
    L.cpb = (width + n_batches - 1) / n_batches;
    return L;
}

static std::vector<Batch> make_batches(const Fr* scalars, uint32_t width, uint64_t cpb) {
    std::vector<Batch> batches;
    for (uint32_t j0 = 0; j0 < width; j0 += (uint32_t)cpb) {
        Batch bt;
        bt.scalars = scalars + j0;
        bt.col0 = j0;
        bt.cols = (uint32_t)std::min<uint64_t>(cpb, width - j0);
        batches.push_back(bt);
    }
    return batches;
}

static SortedRef sorted_ref(const SortedBufs& s) {
    return SortedRef{s.keys2.as<uint32_t>(), s.vals2.as<uint32_t>(), s.start.as<uint32_t>(),
                     s.piece_off.as<uint32_t>(), s.order.as<uint32_t>()};
}

static SortedBufs& wks_sorted(eon_ctx* ctx, size_t w) {
    MsmWork* wks[3] = {&ctx->msm, &ctx->msm_b, &ctx->msm_c};
    return wks[w]->sorted;
}

// device XYZZ results -> affine on the host (synchronises `st`)
static Status results_to_host_affine(const G1Xyzz* dev, uint64_t m, G1Affine* out_host, hipStream_t st) {
    std::vector<G1Xyzz> h(m);
    EON_HIP(hipMemcpyAsync(h.data(), dev, m * sizeof(G1Xyzz), hipMemcpyDeviceToHost, st));
    EON_HIP(hipStreamSynchronize(st));
    host_xyzz_to_affine(h.data(), m, out_host);
    return Status::ok();
}

static Status identity_columns(uint32_t width, G1Affine* out_host) {
    // G1::multi_exp returns the identity for empty input (curve.rs:163-165)
    for (uint32_t j = 0; j < width; j++) {
        out_host[j].x = Fq::zero();
        out_host[j].y = Fq::zero();
    }
    return Status::ok();
}

Status msm_run_columns(eon_ctx* ctx, const eon_msm_bases* b, const Fr* scalars, uint64_t n,
                       uint32_t width, G1Affine* out_host, eon_msm_scalars* keep) {
    if (n > bases_len(b)) return Status::err(EON_E_SHAPE, "more scalars than bases");
    if (keep) {
        keep->ctx = ctx;
        keep->n = n;
        keep->width = width;
        keep->layout = msm_layout(b, n ? n : 1, width ? width : 1);
    }
    if (width == 0) return Status::ok();
    if (n == 0) return out_host ? identity_columns(width, out_host) : Status::ok();
    const MsmLayout L = msm_layout(b, n, width);
    // every batch leaves XYZZ results; one batched XYZZ -> affine conversion at the end (the
    // conversion is an inversion-latency-bound launch, so it is paid once per call)
    EON_HIP(ctx->msm.results.ensure(width * (sizeof(G1Affine) + sizeof(G1Xyzz))));
    G1Affine* res = ctx->msm.results.as<G1Affine>();
    G1Xyzz* res_xyzz = reinterpret_cast<G1Xyzz*>(res + width);
    std::vector<Batch> batches = make_batches(scalars, width, L.cpb);
    for (Batch& bt : batches) bt.out = res_xyzz + bt.col0;
    static const bool all_windows = getenv("EON_MSM_ALL_WINDOWS") != nullptr;
    if (width == 1 && (!keep || keep->active_windows) && !all_windows)
        EON_TRY(active_windows(ctx, L, scalars, n, batches[0].w_act));
    // sorted pairs land in the workspace of batch k % 3, or, when kept, in buffers of their own
    if (keep) {
        keep->sorted.resize(batches.size());
        for (auto& sb : keep->sorted) {
            if (ctx->sorted_cache.empty()) break;
            sb = std::move(ctx->sorted_cache.back());
            ctx->sorted_cache.back() = SortedBufs{};
            ctx->sorted_cache.pop_back();
        }
    }
    auto sorted_of = [&](size_t k) -> SortedBufs& { return keep ? keep->sorted[k] : wks_sorted(ctx, k % 3); };
    // Three streams: every digit sort on the high-priority sort stream, piece sums + reductions
    // alternating between the context stream and the side stream.  Three workspaces (batch k uses
    // k % 3): sort(k+1) only waits for reduce(k-2).  Events order sort(k) after reduce(k - 3)
    // and pieces(k) after sort(k).
    hipStream_t comp[2] = {ctx->stream, ctx->side(ctx->msm_side)};
    hipStream_t sort_st = ctx->side(ctx->msm_sort);
    MsmWork* wks[3] = {&ctx->msm, &ctx->msm_b, &ctx->msm_c};
    EON_HIP(hipEventRecord(ctx->msm_ev[0], ctx->stream));  // scalars and earlier work are ready
    EON_HIP(hipStreamWaitEvent(sort_st, ctx->msm_ev[0], 0));
    for (hipStream_t st : comp)
        if (st != ctx->stream) EON_HIP(hipStreamWaitEvent(st, ctx->msm_ev[0], 0));
    // wait: read the batch's counts back before returning (otherwise batch_pieces does, after
    // launching its piece sums over all pairs: the read-back then overlaps them).  An ordered batch
    // always waits: the form of its piece sums is part of the plan the counts decide (Batch::ordered).
    auto sort_batch = [&](size_t k, bool wait) -> Status {
        const int w = (int)(k % 3);
        if (k >= 3) EON_HIP(hipStreamWaitEvent(sort_st, ctx->msm_reduced[w], 0));
        EON_TRY(batch_sort(ctx, L, n, width, batches[k], *wks[w], sorted_of(k), sort_st, ctx->msm_sorted[w]));
        if (wait || batches[k].ordered) EON_TRY(batch_counts(ctx, L, batches[k], *wks[w], n));
        return Status::ok();
    };
    auto pieces = [&](size_t k) -> Status {
        const int i = (int)(k & 1), w = (int)(k % 3);
        EON_HIP(hipStreamWaitEvent(comp[i], ctx->msm_sorted[w], 0));
        return batch_pieces(ctx, L, bases_pieces29(b), batches[k], sorted_ref(sorted_of(k)), *wks[w], comp[i]);
    };
    DeferredFinish df;
    EON_TRY(prepare_deferred(ctx, L, width, res_xyzz, df));
    // the first batch of a call: a single MSM launches its piece sums ahead of the read-back
    EON_TRY(sort_batch(0, false));
    for (size_t k = 0; k < batches.size(); k++) {
        const int i = (int)(k & 1), w = (int)(k % 3);
        // pieces(k + 1) is enqueued only after reduce(k)'s read-backs: launched earlier it starves
        // the latency-bound reduction (measured +20 ms per prove)
        EON_TRY(pieces(k));
        if (k + 1 < batches.size()) EON_TRY(sort_batch(k + 1, true));
        EON_TRY(batch_reduce(ctx, L, batches[k], sorted_ref(sorted_of(k)), *wks[w], comp[i], df));
        EON_HIP(hipEventRecord(ctx->msm_reduced[w], comp[i]));
    }
    // the context stream resumes after both compute streams' last reductions
    for (int i = 0; i < 2; i++) {
        if (comp[i] == ctx->stream) continue;
        EON_HIP(hipEventRecord(ctx->msm_ev[1 + i], comp[i]));
        EON_HIP(hipStreamWaitEvent(ctx->stream, ctx->msm_ev[1 + i], 0));
    }
    EON_TRY(run_deferred_finish(ctx, df, ctx->stream));
    if (keep) {
        keep->batches = batches;
        for (Batch& bt : keep->batches) bt.scalars = nullptr;
    }
    if (out_host) return results_to_host_affine(res_xyzz, width, out_host, ctx->stream);
    EON_HIP(hipStreamSynchronize(ctx->stream));
    return Status::ok();
}

// out_host[t * width + j] = MSM of column j against bases[t]
Status msm_run_prepared(eon_ctx* ctx, const eon_msm_bases* const* bases, uint32_t nbases,
                        const eon_msm_scalars* s, G1Affine* out_host) {
    const uint32_t width = s->width;
    if (width == 0 || nbases == 0) return Status::ok();
    for (uint32_t t = 0; t < nbases; t++) {
        const eon_msm_bases* b = bases[t];
        if (!b) return Status::err(EON_E_ARG, "null bases");
        if (s->n > bases_len(b)) return Status::err(EON_E_SHAPE, "more scalars than bases");
        // every stored batch's plan (Batch::route, Batch::bucket_lanes) holds for the bases accepted here
        const MsmLayout L = msm_layout(b, s->n ? s->n : 1, width);
        if (L.c != s->layout.c || L.precomputed != s->layout.precomputed)
            return Status::err(EON_E_SHAPE, "bases window layout differs from the prepared scalars'");
    }
    if (s->n == 0) {
        for (uint32_t t = 0; t < nbases; t++) identity_columns(width, out_host + (uint64_t)t * width);
        return Status::ok();
    }
    const uint64_t total = (uint64_t)width * nbases;
    EON_HIP(ctx->msm.results.ensure(total * (sizeof(G1Affine) + sizeof(G1Xyzz))));
    G1Affine* res = ctx->msm.results.as<G1Affine>();
    G1Xyzz* res_xyzz = reinterpret_cast<G1Xyzz*>(res + total);
    // Jobs (batch k, bases t) round-robin over NS = 3 streams and workspaces, enqueued without a
    // host wait (the reductions have no read-backs); a workspace is reused only by its own
    // stream, NS jobs later.
    constexpr uint32_t NS = 3;
    hipStream_t comp[NS] = {ctx->stream, ctx->side(ctx->msm_side), ctx->side(ctx->msm_side2)};
    MsmWork* wks[NS] = {&ctx->msm, &ctx->msm_b, &ctx->msm_c};
    DeferredFinish df;
    EON_TRY(prepare_deferred(ctx, s->layout, total, res_xyzz, df));
    EON_HIP(hipEventRecord(ctx->msm_ev[0], ctx->stream));
    for (uint32_t i = 1; i < NS; i++) EON_HIP(hipStreamWaitEvent(comp[i], ctx->msm_ev[0], 0));
    for (size_t k = 0; k < s->batches.size(); k++)
        for (uint32_t t = 0; t < nbases; t++) {
            const size_t j = k * nbases + t;
            hipStream_t st = comp[j % NS];
            Batch bt = s->batches[k];
            bt.out = res_xyzz + (uint64_t)t * width + bt.col0;
            const SortedRef sr = sorted_ref(s->sorted[k]);
            EON_TRY(batch_pieces(ctx, s->layout, bases_pieces29(bases[t]), bt, sr, *wks[j % NS], st));
            EON_TRY(batch_reduce(ctx, s->layout, bt, sr, *wks[j % NS], st, df));
        }
    for (uint32_t i = 1; i < NS; i++) {
        EON_HIP(hipEventRecord(ctx->msm_ev[1], comp[i]));
        EON_HIP(hipStreamWaitEvent(ctx->stream, ctx->msm_ev[1], 0));
    }
    EON_TRY(run_deferred_finish(ctx, df, ctx->stream));
    return results_to_host_affine(res_xyzz, total, out_host, ctx->stream);
}

Status msm_run(eon_ctx* ctx, const eon_msm_bases* b, const Fr* scalars, uint64_t n,
               G1Affine* result) {
    return msm_run_columns(ctx, b, scalars, n, 1, result, nullptr);
}

}  // namespace eon

namespace {

int finish(eon_ctx* ctx, const Status& s) {
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

}  // namespace

extern "C" {

int eon_msm_bases_create(eon_ctx* ctx, const eon_g1_affine* bases, uint64_t n, uint32_t flags,
                         eon_msm_bases** out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    return finish(ctx, bases_create(ctx, bases, n, flags, false, out));
}

int eon_msm_bases_create_dev(eon_ctx* ctx, const eon_g1_affine* bases, uint64_t n, uint32_t flags,
                             eon_msm_bases** out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    return finish(ctx, bases_create(ctx, bases, n, flags, true, out));
}

int eon_msm_g1(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* scalars, uint64_t n,
               eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (!bases || !out || (n && !scalars)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s;
    if (n > bases_len(bases)) {
        s = Status::err(EON_E_SHAPE, "more scalars than bases");
    } else {
        s = [&]() -> Status {
            EON_HIP(ctx->stage_in.ensure((n ? n : 1) * sizeof(Fr)));
            if (n)
                EON_HIP(hipMemcpyAsync(ctx->stage_in.p, scalars, n * sizeof(Fr),
                                       hipMemcpyHostToDevice, ctx->stream));
            G1Affine r;
            EON_TRY(msm_run(ctx, bases, ctx->stage_in.as<Fr>(), n, &r));
            *out = g1_to_abi(r);
            return Status::ok();
        }();
    }
    return finish(ctx, s);
}

int eon_msm_g1_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* scalars, uint64_t n,
                   eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (!bases || !out || (n && !scalars)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    G1Affine r;
    Status s = msm_run(ctx, bases, reinterpret_cast<const Fr*>(scalars), n, &r);
    if (!s.bad()) *out = g1_to_abi(r);
    return finish(ctx, s);
}

int eon_msm_g1_columns_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* mat,
                           uint64_t rows, uint32_t width, eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (!bases || (width && !out) || (rows && width && !mat)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    std::vector<G1Affine> r(width);
    Status s = msm_run_columns(ctx, bases, reinterpret_cast<const Fr*>(mat), rows, width, r.data(), nullptr);
    if (!s.bad())
        for (uint32_t j = 0; j < width; j++) out[j] = g1_to_abi(r[j]);
    return finish(ctx, s);
}

int eon_msm_g1_columns(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* mat, uint64_t rows,
                       uint32_t width, eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (!bases || (width && !out) || (rows && width && !mat)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    std::vector<G1Affine> r(width);
    Status s = [&]() -> Status {
        if (rows > bases_len(bases)) return Status::err(EON_E_SHAPE, "more rows than bases");
        const size_t bytes = (size_t)rows * width * sizeof(Fr);
        EON_HIP(ctx->stage_in.ensure(bytes ? bytes : 32));
        if (bytes) EON_HIP(hipMemcpyAsync(ctx->stage_in.p, mat, bytes, hipMemcpyHostToDevice, ctx->stream));
        return msm_run_columns(ctx, bases, ctx->stage_in.as<Fr>(), rows, width, r.data(), nullptr);
    }();
    if (!s.bad())
        for (uint32_t j = 0; j < width; j++) out[j] = g1_to_abi(r[j]);
    return finish(ctx, s);
}

int eon_msm_g1_columns_prepare_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* mat,
                                   uint64_t rows, uint32_t width, eon_g1_affine* out,
                                   eon_msm_scalars** prepared) {
    if (!ctx) return EON_E_ARG;
    if (!bases || !prepared || (rows && width && !mat)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    auto* keep = new eon_msm_scalars();
    std::vector<G1Affine> r(width);
    Status s = msm_run_columns(ctx, bases, reinterpret_cast<const Fr*>(mat), rows, width,
                               out ? r.data() : nullptr, keep);
    if (s.bad()) {
        delete keep;
        return finish(ctx, s);
    }
    if (out)
        for (uint32_t j = 0; j < width; j++) out[j] = g1_to_abi(r[j]);
    *prepared = keep;
    return EON_OK;
}

void eon_msm_scalars_destroy(eon_msm_scalars* s) {
    if (!s) return;
    if (s->ctx) {
        std::lock_guard<std::mutex> lk(s->ctx->mu);
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);
        delete s;
        return;
    }
    delete s;
}

int eon_msm_g1_columns_prepared(eon_ctx* ctx, const eon_msm_bases* const* bases, uint32_t nbases,
                                const eon_msm_scalars* prepared, eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (!prepared || (nbases && !bases) || (nbases && prepared->width && !out)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    if (prepared->ctx && prepared->ctx != ctx) return finish(ctx, Status::err(EON_E_ARG, "prepared scalars of another context"));
    const uint64_t total = (uint64_t)nbases * prepared->width;
    std::vector<G1Affine> r(total);
    Status s = msm_run_prepared(ctx, bases, nbases, prepared, r.data());
    if (!s.bad())
        for (uint64_t j = 0; j < total; j++) out[j] = g1_to_abi(r[j]);
    return finish(ctx, s);
}

// Diagnostics (tests): what a prepared handle keeps of its batches, read back.  Reads only.
int eon_diag_msm_scalars_batches(eon_ctx* ctx, const eon_msm_scalars* prepared, uint32_t* count) {
    if (!ctx) return EON_E_ARG;
    if (!prepared || !count) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (prepared->ctx && prepared->ctx != ctx) return finish(ctx, Status::err(EON_E_ARG, "prepared scalars of another context"));
    *count = (uint32_t)prepared->batches.size();
    return EON_OK;
}

int eon_diag_msm_scalars_batch(eon_ctx* ctx, const eon_msm_scalars* prepared, uint32_t k, eon_msm_batch_info* info,
                               uint32_t* keys, uint32_t* vals, uint32_t* start, uint32_t* piece_off) {
    if (!ctx) return EON_E_ARG;
    if (!prepared || !info) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (prepared->ctx && prepared->ctx != ctx) return Status::err(EON_E_ARG, "prepared scalars of another context");
        if (k >= prepared->batches.size() || k >= prepared->sorted.size())
            return Status::err(EON_E_ARG, "batch index out of range");
        const Batch& bt = prepared->batches[k];
        if (!bt.counted) return Status::err(EON_E_ARG, "the batch's counts were never read back");
        info->pairs = bt.E;
        info->c = bt.c;
        info->windows = bt.W;
        info->ref_windows = prepared->layout.W;
        info->groups = bt.groups;
        info->nb = bt.nb;
        info->log_chunk = bt.log_chunk;
        info->cols = bt.cols;
        info->col0 = bt.col0;
        info->n_pairs = bt.n_pairs;
        info->n_pieces = bt.n_pieces;
        const SortedBufs& sb = prepared->sorted[k];
        const size_t pair_bytes = bt.E * 4, bucket_bytes = ((size_t)bt.nb + 1) * 4;
        if (sb.keys2.bytes < pair_bytes || sb.vals2.bytes < pair_bytes || sb.start.bytes < bucket_bytes ||
            sb.piece_off.bytes < bucket_bytes)
            return Status::err(EON_E_ARG, "the batch's sorted buffers are not held");
        // the prepare call returned after its streams had drained into the context stream
        if (keys) EON_HIP(hipMemcpyAsync(keys, sb.keys2.p, pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (vals) EON_HIP(hipMemcpyAsync(vals, sb.vals2.p, pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (start) EON_HIP(hipMemcpyAsync(start, sb.start.p, bucket_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (piece_off)
            EON_HIP(hipMemcpyAsync(piece_off, sb.piece_off.p, bucket_bytes, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}

int eon_diag_msm_scalars_order(eon_ctx* ctx, const eon_msm_scalars* prepared, uint32_t k, uint32_t* window,
                               uint32_t* bucket_lanes, uint32_t* order) {
    if (!ctx) return EON_E_ARG;
    if (!prepared || !window || !bucket_lanes) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (prepared->ctx && prepared->ctx != ctx) return Status::err(EON_E_ARG, "prepared scalars of another context");
        if (k >= prepared->batches.size() || k >= prepared->sorted.size())
            return Status::err(EON_E_ARG, "batch index out of range");
        const Batch& bt = prepared->batches[k];
        if (!bt.counted) return Status::err(EON_E_ARG, "the batch's counts were never read back");
        *window = bt.ordered ? ORDER_WINDOW : 0;
        *bucket_lanes = bt.bucket_lanes ? 1 : 0;
        if (!order || !bt.ordered) return Status::ok();
        const SortedBufs& sb = prepared->sorted[k];
        const size_t bytes = (size_t)bt.nb * 4;
        if (sb.order.bytes < bytes) return Status::err(EON_E_ARG, "the batch's bucket order is not held");
        EON_HIP(hipMemcpyAsync(order, sb.order.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}

// The unprepared single MSM (msm_run with its active-window truncation) that also keeps its batch.
int eon_diag_msm_g1_prepare_active_dev(eon_ctx* ctx, const eon_msm_bases* bases, const eon_fr* scalars, uint64_t n,
                                       eon_g1_affine* out, eon_msm_scalars** prepared) {
    if (!ctx) return EON_E_ARG;
    if (!bases || !out || !prepared || (n && !scalars)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    auto* keep = new eon_msm_scalars();
    keep->active_windows = true;
    G1Affine r;
    Status s = msm_run_columns(ctx, bases, reinterpret_cast<const Fr*>(scalars), n, 1, &r, keep);
    if (s.bad()) {
        delete keep;
        return finish(ctx, s);
    }
    *out = g1_to_abi(r);
    *prepared = keep;
    return EON_OK;
}

int eon_g1_multi_exp(eon_ctx* ctx, const eon_g1_affine* points, const eon_fr* scalars, uint64_t n,
                     eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (!out || (n && (!points || !scalars))) return EON_E_ARG;
    eon_msm_bases* b = nullptr;
    int rc = eon_msm_bases_create(ctx, points, n, 0, &b);
    if (rc) return rc;
    rc = eon_msm_g1(ctx, b, scalars, n, out);
    eon_msm_bases_destroy(b);
    return rc;
}

}  // extern "C"
