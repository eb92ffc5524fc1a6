// MSM stage 2: the piece sums of one sorted batch (batch_pieces), chunked or one bucket per lane by
// the batch's plan, and the merge of two-piece buckets (piece_merge).  The pipeline is described
// in msm.hip.
#include <algorithm>

#include "msm_batch.h"

namespace eon {

constexpr uint32_t PIECE_MINWAVES = 4;  // k_piece_sum29's waves per SIMD (its VGPR budget: 128)

// Thread t sums the sorted pairs [t 2^log_chunk, (t+1) 2^log_chunk) (nonzero digits only): one
// partial per bucket run, stored at piece_off[b] + t - (start[b] >> log_chunk).  The XYZZ
// accumulator is in 29-bit limbs (ec29.h: lazy bounds, no carry captures in the products) and the
// bases are read in 29-Montgomery form (k_table_to29).  Each bucket run stores its raw accumulator (144 bytes,
// ZZ = 0 for the identity); k_raw29_to_xyzz converts the pieces for the combine levels.
//
// The additions are unchecked (madd29_negsum): x(acc) == x(A) -- a duplicate base, or a base
// meeting its negation -- leaves ZZ = 0 mod p for the rest of the run, so the run's ZZ is tested
// once at its flush and such a run is summed again with the checked additions (piece_run29).
// An identity base ((0, 0) in the table) is recognised by y = 0 alone: G1 has prime order, so no
// curve point has y = 0.

// sum of the bases of sorted pairs [e_begin, e_end) with every exceptional case resolved;
// returns whether the sum is the identity
__device__ __forceinline__ bool piece_run29(const uint32_t* vals, const G1Affine* pts29, uint32_t e_begin,
                                            uint32_t e_end, G1X29& acc) {
    bool inf = true;
    for (uint32_t e = e_begin; e < e_end; e++) {
        const uint32_t v = vals[e];
        G1Affine a = ld_affine(pts29 + (v & 0x7fffffffu));
        if (a.y.is_zero()) continue;
        if (v >> 31) a.y = neg(a.y);
        const F29 ax = unpack29(a.x), ay = unpack29(a.y);
        if (inf) {
            acc.X = ax;
            acc.Y = ay;
            acc.ZZ = const29<FqP>(R29<FqP>::ONE);
            acc.ZZZ = acc.ZZ;
            inf = false;
        } else if (!madd29(acc, ax, ay)) {
            inf = madd29_exceptional(acc, ax, ay);
        }
    }
    return inf;
}

__global__ void __launch_bounds__(64, PIECE_MINWAVES) k_piece_sum29(
    const uint32_t* keys, const uint32_t* vals, const uint32_t* start, const uint32_t* piece_off,
    uint32_t log_chunk, uint32_t c, uint32_t groups, uint32_t nb, const G1Affine* pts29, G1Raw29* piece_raw) {
    // the nonzero-digit pairs (start[nb]): read here, so that the launch need not wait for the
    // count read-back (the grid covers every pair of the batch)
    const uint32_t n_pairs = start[nb];
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; ((uint64_t)t << log_chunk) < n_pairs;
         t += gridDim.x * blockDim.x) {
        const uint32_t e0 = t << log_chunk;
        const uint32_t e1 = min(e0 + (1u << log_chunk), n_pairs);
        uint32_t b = keys[e0];
        uint32_t run = e0;  // first pair of the current bucket run
        G1X29 acc;
        bool inf = true;
        // the accumulator holds (-1)^flip times the run's sum (madd29_negsum returns the negated
        // sum; a run opening with a negative digit starts from the unnegated base with flip set)
        bool flip = false;
        auto flush = [&](uint32_t e_end) __attribute__((always_inline)) {
            if (!inf && is_zero_mod29<FqP>(acc.ZZ)) {
                inf = piece_run29(vals, pts29, run, e_end, acc);
                flip = false;
            }
            if (flip) acc.ZZZ = neg29_lazy<3>(acc.ZZZ);  // ZZZ < 2p normalised -> 3p - ZZZ
            const uint32_t bb = bucket_of(b, c, groups, nb);
            G1Raw29* dst = piece_raw + piece_off[bb] + t - (start[bb] >> log_chunk);
            // an identity piece is any raw accumulator with ZZ = 0 (every reader tests ZZ alone):
            // one store of acc either way, instead of selecting all 36 words between acc and zeros
            if (inf) acc.ZZ = F29{};
            st_raw29(dst, acc);
        };
        // 16-byte loads of four keys and four references every fourth pair (chunks are aligned to
        // 2^LOG_CHUNK_MIN pairs; a chunk cut short by n_pairs reads one pair at a time): a quarter
        // of the pair-stream requests (prove -2.5 % A/B against one-pair loads)
        const bool vec = ((e0 | e1) & 3) == 0;
        uint4 kq = make_uint4(0, 0, 0, 0), vq = kq;
        for (uint32_t e = e0;; e++) {
            // one flush site (the run's end or the chunk's), so the checked re-sum is emitted once
            const bool last = e == e1;
            // the pair is always picked from the register quads (a chunk cut short reloads
            // component 0 every pair): a pick written as "vec ? quad component : *p" was compiled
            // as one load through a selected pointer, which kept the quads in scratch (eight
            // scratch stores per quad, a flat load and a wait per pair)
            const uint32_t sub = vec ? (e & 3) : 0;
            if (!last && sub == 0) {
                if (vec) {
                    kq = *reinterpret_cast<const uint4*>(keys + e);
                    vq = *reinterpret_cast<const uint4*>(vals + e);
                } else {
                    kq.x = keys[e];
                    vq.x = vals[e];
                }
            }
            auto pick = [&](const uint4& q) __attribute__((always_inline)) {
                return sub == 0 ? q.x : sub == 1 ? q.y : sub == 2 ? q.z : q.w;
            };
            const uint32_t k = last ? b : pick(kq);
            if (last || k != b) {
                flush(e);
                if (last) break;
                inf = true;
                b = k;
                run = e;
            }
            const uint32_t v = pick(vq);
            G1Affine a = ld_affine(pts29 + (v & 0x7fffffffu));
            if (a.y.is_zero()) continue;
            // the digit's sign and the accumulator's are applied together, as one lazy negation of
            // the base's y in radix 2^29 (9 subtractions and 9 selects instead of a borrow chain)
            const bool neg_digit = v >> 31;
            const F29 ax = unpack29(a.x), ay = unpack29(a.y);
            if (inf) {
                acc.X = ax;
                acc.Y = ay;
                acc.ZZ = const29<FqP>(R29<FqP>::ONE);
                acc.ZZZ = acc.ZZ;
                flip = neg_digit;
                inf = false;
            } else {
                const F29 ayn = neg29_lazy<2>(ay);
                const bool ng = neg_digit != flip;
                F29 ys;
#pragma unroll
                for (int i = 0; i < 9; i++) ys.l[i] = ng ? ayn.l[i] : ay.l[i];
                madd29_negsum(acc, ax, ys);
                flip = !flip;
            }
        }
        // acc holds the chunk's last piece as stored.  When its bucket goes on into the next chunk
        // and ends there (two pieces), lane t + 1 of this wave stored the bucket's second piece
        // at its first flush -- earlier in this wave's instruction stream, every lane's pair loop
        // having ended -- so lane t sums it in here (k_piece_merge29 covers lane 63's boundary).
        // This exchange goes through global memory between lanes of one wave and assumes what the
        // HIP memory model does not promise: that the wave's lanes have reconverged after the
        // divergent pair loop, so that lane t + 1's store was issued before lane t's load in the one
        // instruction stream they share (gfx950 runs a wave's lanes in lockstep and the compiler
        // keeps the loop's exit as the join point), and that the block-scope fence below then makes
        // that store visible to the load.  A compiler that sank the first flush's store below this
        // point, or hardware with independent lane progress, would break it.
        if (e1 < n_pairs && ((t + 1) & 63u) != 0 && keys[e1] == b) {
            const uint32_t bb = bucket_of(b, c, groups, nb);
            const uint32_t p0 = piece_off[bb];
            if (piece_off[bb + 1] - p0 == 2) {
                __threadfence_block();
                G1X29 x;
                const bool x_inf = ld_raw29(piece_raw + p0 + 1, x);
                acc29(acc, inf, x, x_inf);
                if (inf) acc.ZZ = F29{};
                st_raw29(piece_raw + p0, acc);
                // the second piece becomes the identity, for the reductions that read every piece
                st_raw29_inf(piece_raw + p0 + 1);
            }
        }
    }
}

// The piece sums of a column batch, one whole bucket per lane: the wave takes 64 consecutive entries
// of `order` (k_bucket_order: runs of nearly equal length), lane l sums the pairs
// [start[b], start[b + 1]) of its bucket b and stores the bucket's one piece at index b.  Every lane
// opens its run in the first iteration and flushes after the last, so the wave executes the run
// start and the flush once instead of wherever one of 64 chunks crosses a bucket boundary, no
// bucket is cut in two (nothing to merge) and the keys are not read.  The arithmetic is
// k_piece_sum29's.  Correct for any run lengths; the host sends skewed batches down the chunked
// route because a wave here runs as long as its longest bucket.
__global__ void __launch_bounds__(64, PIECE_MINWAVES) k_piece_sum_bucket29(
    const uint32_t* vals, const uint32_t* start, const uint32_t* order, uint32_t nb, bool vec,
    const G1Affine* pts29, G1Raw29* piece_raw) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < nb;
    const uint32_t b = live ? order[i] : 0u;
    const uint32_t e0 = live ? start[b] : 0u;
    const uint32_t len = live ? start[b + 1] - e0 : 0u;
    // the wave's longest run bounds the loop (a uniform trip count); shorter runs sit out the rest
    uint32_t longest = len;
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, (int)d));
    longest = __builtin_amdgcn_readfirstlane(longest);
    G1X29 acc;
    bool inf = true;
    // the accumulator holds (-1)^flip times the run's sum, as in k_piece_sum29
    bool flip = false;
    // the references in aligned 16-byte quads with a per-lane pick: a lane's run starts at any pair,
    // so its first quad is aligned down (the pairs before the run are loaded and not picked) and
    // the lanes reload at different iterations; prove -0.7 % A/B against one 4-byte load per pair
    // fetched an iteration ahead.  vec: the batch holds a multiple of 4 pairs, so the last quad
    // stays inside `vals`; otherwise one pair at a time into component 0.
    uint4 vq = make_uint4(0, 0, 0, 0);
    for (uint32_t k = 0; k < longest; k++) {
        if (k >= len) continue;
        const uint32_t e = e0 + k, sub = vec ? (e & 3u) : 0u;
        if (vec) {
            if (k == 0 || sub == 0) vq = *reinterpret_cast<const uint4*>(vals + (e & ~3u));
        } else {
            vq.x = vals[e];
        }
        const uint32_t v = sub == 0 ? vq.x : sub == 1 ? vq.y : sub == 2 ? vq.z : vq.w;
        G1Affine a = ld_affine(pts29 + (v & 0x7fffffffu));
        if (a.y.is_zero()) continue;
        const bool neg_digit = v >> 31;
        const F29 ax = unpack29(a.x), ay = unpack29(a.y);
        if (inf) {
            acc.X = ax;
            acc.Y = ay;
            acc.ZZ = const29<FqP>(R29<FqP>::ONE);
            acc.ZZZ = acc.ZZ;
            flip = neg_digit;
            inf = false;
        } else {
            const F29 ayn = neg29_lazy<2>(ay);
            const bool ng = neg_digit != flip;
            F29 ys;
#pragma unroll
            for (int j = 0; j < 9; j++) ys.l[j] = ng ? ayn.l[j] : ay.l[j];
            madd29_negsum(acc, ax, ys);
            flip = !flip;
        }
    }
    if (!live) return;
    // the one flush: a run that met an exceptional addition (ZZ = 0 mod p) is summed again, checked
    if (!inf && is_zero_mod29<FqP>(acc.ZZ)) {
        inf = piece_run29(vals, pts29, e0, e0 + len, acc);
        flip = false;
    }
    if (inf) {  // an empty bucket, identity bases only, or a sum that cancelled
        st_raw29_inf(piece_raw + b);
        return;
    }
    if (flip) acc.ZZZ = neg29_lazy<3>(acc.ZZZ);  // ZZZ < 2p normalised -> 3p - ZZZ
    st_raw29(piece_raw + b, acc);
}

__global__ void k_raw29_to_xyzz(const G1Raw29* in, uint32_t n, G1Xyzz* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st_xyzz(out + i, raw29_to_xyzz(in + i));
}

// The two-piece contract between the chunked piece sums and k_bucket_reduce29<.., ONE_PIECE = false>
// (msm_reduce.hip).  A bucket whose pairs straddle exactly one chunk boundary holds two pieces, at
// piece_off[b] and piece_off[b] + 1 (k_piece_sum29's thread t - 1 ends the bucket's first run,
// thread t starts its second).  Before the reduction both are summed into the FIRST:
//   - k_piece_sum29 itself, for the boundary between lanes t and t + 1 of one wave; it also
//     rewrites the second piece as the identity;
//   - k_piece_merge29 (piece_merge, launched by the Deferred and FusedGroups routes ahead of the
//     reduction), for the boundaries between waves, lane 63 | lane 0; it leaves the second piece
//     as it was.
// k_bucket_reduce29<.., false> therefore reads the first piece alone of every bucket that has
// exactly two and never the second, which after k_piece_merge29 is stale, not the identity.  Every
// other reader of chunked pieces (k_segment_reduce29, k_bucket_sums29, the combine levels) runs on
// a route without piece_merge and sums every piece; there an in-wave merge's second piece is the
// identity and the sum is the same.  Buckets with three or more pieces are never merged.
//
// Here: one thread per chunk boundary.  In the reduction a wave walks the buckets of a segment in step, one lane
// per group, and pays the most pieces any lane has per bucket -- two almost always (a bucket of
// ~64 sorted pairs straddles a 128-pair chunk boundary half of the time), so its three additions
// per bucket become two there, and this kernel's half addition per bucket runs with every lane
// busy.  Buckets spanning three or more chunks (rare) keep all their pieces.
// Thread i takes the boundary before chunk (i + 1) 2^log_step (log_step 6: the boundaries between
// k_piece_sum29's waves, the rest merged there).
__global__ void __launch_bounds__(64) k_piece_merge29(const uint32_t* keys, const uint32_t* start,
                                                      const uint32_t* piece_off, uint32_t log_chunk,
                                                      uint32_t log_step, uint32_t c, uint32_t groups, uint32_t nb,
                                                      G1Raw29* pieces) {
    const uint32_t n_pairs = start[nb];
    const uint64_t e0 = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x + 1) << (log_chunk + log_step);
    if (e0 >= n_pairs) return;
    const uint32_t k = keys[e0];
    if (keys[e0 - 1] != k) return;
    const uint32_t bb = bucket_of(k, c, groups, nb);
    const uint32_t p0 = piece_off[bb];
    if (piece_off[bb + 1] - p0 != 2) return;
    G1X29 a, x;
    bool a_inf = ld_raw29(pieces + p0, a);
    const bool x_inf = ld_raw29(pieces + p0 + 1, x);
    acc29(a, a_inf, x, x_inf);
    if (a_inf)
        st_raw29_inf(pieces + p0);
    else
        st_raw29(pieces + p0, a);
}

Status batch_pieces(eon_ctx* ctx, const MsmLayout& L, const G1Affine* pts, Batch& bt, const SortedRef& sr,
                    MsmWork& wk, hipStream_t st) {
    // the piece-sum form needs the counts (Batch::ordered); only a batch without a bucket order
    // may launch its (chunked) piece sums ahead of the read-back
    if (bt.ordered && !bt.counted) return Status::err(EON_E_ARG, "an ordered MSM batch is counted before its piece sums");
    EON_HIP(ctx_ensure(ctx, wk.piece_sums, std::max<uint64_t>(bt.max_pieces * sizeof(G1Xyzz), (uint64_t)bt.nb * sizeof(G1Raw29))));
    EON_HIP(ctx_ensure(ctx, wk.piece_sums2, bt.max_pieces * sizeof(G1Xyzz)));
    EON_HIP(ctx_ensure(ctx, wk.owner, bt.max_pieces * 4));
    EON_HIP(ctx_ensure(ctx, wk.bucket_sums, (uint64_t)bt.nb * sizeof(G1Xyzz)));
    EON_HIP(ctx_ensure(ctx, wk.off2, (bt.nb + 1) * 4ull));
    EON_HIP(ctx_ensure(ctx, wk.off3, (bt.nb + 1) * 4ull));
    EON_HIP(ctx_ensure(ctx, wk.count, (bt.nb + 1) * 4ull));
    EON_HIP(ctx_ensure(ctx, wk.temp, bt.scan_bytes));
    EON_HIP(ctx_ensure(ctx, wk.piece_raw, bt.max_pieces * sizeof(G1Raw29)));
    if (!wk.host_counts) EON_HIP(hipHostMalloc(reinterpret_cast<void**>(&wk.host_counts), 64));
    // algorithmic bytes: n (64 + 32) B per MSM of n terms -- each
    // base and scalar read once; design bytes: what this kernel's access pattern moves instead,
    // a 4-byte key, a 4-byte reference and a 64-byte table entry per nonzero digit plus one
    // 144-byte partial per piece
    // mulmods: one XYZZ mixed addition (madd-2008-s, 8M + 2S) per nonzero digit
    const uint64_t msm_n = bt.E / ((uint64_t)bt.W * bt.cols);
    // launched before the count read-back (batch_counts), the grid covers all E pairs and the
    // profiler record gets its counts later
    const uint64_t pairs_max = bt.counted ? bt.n_pairs : bt.E;
    if (!bt.counted && ctx->prof.enabled) bt.prof_rec = ctx->prof.recs.size();
    if (bt.bucket_lanes) {  // false until the batch is counted
        // design bytes: a 4-byte reference and a 64-byte table entry per pair; per bucket its order
        // entry, its two starts and one 144-byte piece
        ctx->prof.begin("k_piece_sum", (uint64_t)bt.cols * msm_n * 96, st, (uint64_t)bt.n_pairs * 10,
                        (uint64_t)bt.n_pairs * 68 + (uint64_t)bt.nb * 156);
        hipLaunchKernelGGL(k_piece_sum_bucket29, dim3(blocks_for(bt.nb, 64)), dim3(64), 0, st, sr.vals, sr.start,
                           sr.order, bt.nb, (bt.E & 3) == 0, pts, wk.piece_raw.as<G1Raw29>());
        ctx->prof.end(st);
        EON_HIP(hipGetLastError());
        return Status::ok();
    }
    ctx->prof.begin("k_piece_sum", (uint64_t)bt.cols * msm_n * 96, st, (uint64_t)bt.n_pairs * 10,
                    (uint64_t)bt.n_pairs * 72 + (uint64_t)bt.n_pieces * 144);
    const uint32_t blocks = blocks_for((pairs_max + (1u << bt.log_chunk) - 1) >> bt.log_chunk, 64);
    if (pairs_max)
        hipLaunchKernelGGL(k_piece_sum29, dim3(blocks), dim3(64), 0, st, sr.keys, sr.vals, sr.start, sr.piece_off,
                           bt.log_chunk, bt.c, bt.groups, bt.nb, pts, wk.piece_raw.as<G1Raw29>());
    ctx->prof.end(st);
    if (!bt.counted) EON_TRY(batch_counts(ctx, L, bt, wk, msm_n));
    // the Combine routes sum radix-2^32 pieces
    if (bt.n_pieces && (bt.route == Reduce::CombineGroups || bt.route == Reduce::CombineSegments))
        hipLaunchKernelGGL(k_raw29_to_xyzz, dim3(blocks_for(bt.n_pieces, 128)), dim3(128), 0, st,
                           wk.piece_raw.as<G1Raw29>(), bt.n_pieces, wk.piece_sums.as<G1Xyzz>());
    EON_HIP(hipGetLastError());
    return Status::ok();
}

// k_piece_merge29 over the boundaries between k_piece_sum29's waves (the two-piece contract above)
Status piece_merge(eon_ctx* ctx, const Batch& bt, const SortedRef& sr, MsmWork& wk, hipStream_t st) {
    const uint64_t chunks = ((uint64_t)bt.n_pairs + (1u << bt.log_chunk) - 1) >> bt.log_chunk;
    const uint32_t log_step = 6;  // the boundaries between k_piece_sum29's waves (k_piece_merge29)
    const uint64_t boundaries = (chunks - 1) >> log_step;
    if (chunks < 2 || boundaries == 0) return Status::ok();
    // ~one addition per boundary: 2 x 144 B read, 144 B written
    ctx->prof.begin("k_piece_merge29", boundaries * 432, st, boundaries * 14);
    hipLaunchKernelGGL(k_piece_merge29, dim3(blocks_for(boundaries, 64)), dim3(64), 0, st, sr.keys, sr.start,
                       sr.piece_off, bt.log_chunk, log_step, bt.c, bt.groups, bt.nb, wk.piece_raw.as<G1Raw29>());
    ctx->prof.end(st);
    EON_HIP(hipGetLastError());
    return Status::ok();
}

}  // namespace eon
