// MSM stage 3: a batch's pieces -> one point per group by the batch's route (batch_reduce), and the
// call-wide deferred group finish.  The pipeline is described in msm.hip.
#include <algorithm>

#include "msm_batch.h"
#include "sort.h"

namespace eon {

// a raw radix-2^29 accumulator to memory in the destination's form: G1Xyzz (radix 2^32, canonical)
// or G1Raw29 (the raw lazy accumulator, ZZ = 0 for the identity)
__device__ __forceinline__ void st_point(G1Xyzz* p, const G1X29& a, bool inf) { st_xyzz(p, x29_to_xyzz(a, inf)); }
__device__ __forceinline__ void st_point(G1Raw29* p, const G1X29& a, bool inf) {
    if (inf)
        st_raw29_inf(p);
    else
        st_raw29(p, a);
}

__global__ void k_piece_owner(const uint32_t* piece_off, uint32_t nb, uint32_t* owner) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    for (uint32_t p = piece_off[b]; p < piece_off[b + 1]; p++) owner[p] = b;
}

// One combine level: new partial p of bucket b sums old partials
// [off_old[b] + PIECE*j, min(+PIECE, off_old[b+1])), j = p - off_new[b].
// The launch covers an upper bound of the new partial count; the count itself is off_new[nb].
__global__ void k_partial_combine(const uint32_t* off_old, const uint32_t* off_new,
                                  const uint32_t* owner, uint32_t nb, const G1Xyzz* in,
                                  G1Xyzz* out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= off_new[nb]) return;
    const uint32_t b = owner[p];
    const uint32_t j = p - off_new[b];
    const uint32_t e0 = off_old[b] + j * PIECE;
    const uint32_t e1 = min(e0 + PIECE, off_old[b + 1]);
    G1Xyzz acc = ld_xyzz(in + e0);
    for (uint32_t e = e0 + 1; e < e1; e++) acc = xyzz_add(acc, ld_xyzz(in + e));
    st_xyzz(out + p, acc);
}

// count[b] = ceil((off[b+1] - off[b]) / PIECE) (0 for the terminator)
__global__ void k_level_count(const uint32_t* off, uint32_t nb, uint32_t* count) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > nb) return;
    count[b] = b == nb ? 0 : (off[b + 1] - off[b] + PIECE - 1) / PIECE;
}

// every bucket holds at most one partial: bucket_sums[b] = it, or the identity
__global__ void k_bucket_final(const uint32_t* off, uint32_t B, uint32_t groups,
                               const G1Xyzz* partials, G1Xyzz* bucket_sums) {
    // bucket_sums is column-major (group * B + m) for the reduction; partials follow b' order
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B * groups) return;
    const uint32_t bp = (b % B) * groups + b / B;
    st_xyzz(bucket_sums + b, off[bp + 1] > off[bp] ? ld_xyzz(partials + off[bp]) : xyzz_inf());
}

// Segment s of group g covers buckets [lo, lo + SEG) (bucket b holds digit b + 1):
// out = sum_b (b + 1) * S_b = (running-sum form) + lo * (sum_b S_b).  The latency-optimal form
// for few groups (one short chain per segment, one tree): used when a batch has < 64 groups.
__global__ void __launch_bounds__(64) k_segment_sum(const G1Xyzz* bucket_sums, uint32_t B,
                                                    uint32_t groups, G1Xyzz* seg_out) {
    const uint32_t nseg = B / SEG;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseg * groups) return;
    const uint32_t g = t / nseg, s = t % nseg;
    const uint32_t lo = s * SEG;
    const G1Xyzz* sb = bucket_sums + (uint64_t)g * B + lo;
    G1Xyzz run = xyzz_inf(), acc = xyzz_inf();
    for (int k = SEG - 1; k >= 0; k--) {
        run = xyzz_add(run, ld_xyzz(sb + k));
        acc = xyzz_add(acc, run);
    }
    if (lo) acc = xyzz_add(acc, xyzz_mul_small(run, lo));
    st_xyzz(seg_out + t, acc);
}

// One level of the weighted bucket sum: segment j of group g covers x = X[g L + j seg ..+ seg);
// T = sum_k x_k and U = sum_k k x_k, by running sums from the top (2 (seg - 1) + 1 additions).
__global__ void __launch_bounds__(64) k_seg_level(const G1Xyzz* X, uint32_t L, uint32_t seg, uint32_t groups, G1Xyzz* T,
                            G1Xyzz* U) {
    const uint32_t nseg = L / seg;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseg * groups) return;
    const G1Xyzz* x = X + (uint64_t)(t / nseg) * L + (uint64_t)(t % nseg) * seg;
    G1Xyzz run = xyzz_inf(), acc = xyzz_inf();
    for (uint32_t k = seg - 1; k >= 1; k--) {
        run = xyzz_add(run, ld_xyzz(x + k));
        acc = xyzz_add(acc, run);
    }
    run = xyzz_add(run, ld_xyzz(x));
    st_xyzz(T + t, run);
    st_xyzz(U + t, acc);
}

// The first level of the weighted bucket sum fused with the bucket sums, straight from
// k_piece_sum29's raw partials (radix 2^29, lazy): segment s of group g covers magnitudes
// [s seg, s seg + seg); bucket m is the sum of its pieces [piece_off[b'], piece_off[b' + 1]),
// b' = m groups + g (<= PIECE of them: used when no combine level is needed).  Same T / U as
// k_seg_level over the bucket sums, at T[g nseg + s] / U[g nseg + s]; a wave covers consecutive
// groups of one segment, so its piece reads are adjacent.
// OutT = G1Xyzz (the per-batch k_group_finish) or G1Raw29 (the call-wide k_group_finish29).
// ONE_PIECE: the pieces of k_piece_sum_bucket29, bucket bp's one piece at index bp (piece_off unread).
// Otherwise the chunked pieces after piece_merge: a bucket with exactly two pieces has their sum in
// the first and the second is not read (the two-piece contract, msm_pieces.hip: k_piece_merge29).
template <class OutT, bool ONE_PIECE>
__global__ void __launch_bounds__(64) k_bucket_reduce29(const G1Raw29* pieces, const uint32_t* piece_off,
                                                        uint32_t B, uint32_t seg, uint32_t groups, OutT* T,
                                                        OutT* U) {
    const uint32_t nseg = B / seg;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseg * groups) return;
    const uint32_t g = t % groups, s = t / groups;
    G1X29 run, acc, x;
    bool run_inf = true, acc_inf = true;
    for (int k = (int)seg - 1; k >= 0; k--) {
        const uint32_t bp = (s * seg + (uint32_t)k) * groups + g;
        const uint32_t e0 = ONE_PIECE ? bp : piece_off[bp];
        uint32_t e1 = ONE_PIECE ? bp + 1 : piece_off[bp + 1];
        if (e1 - e0 == 2) e1 = e0 + 1;  // k_piece_sum29 / k_piece_merge29 summed the two into the first
        for (uint32_t e = e0; e < e1; e++) {
            const bool inf = ld_raw29(pieces + e, x);
            acc29(run, run_inf, x, inf);
        }
        if (k >= 1) acc29(acc, acc_inf, run, run_inf);
    }
    st_point(T + (uint64_t)g * nseg + s, run, run_inf);
    st_point(U + (uint64_t)g * nseg + s, acc, acc_inf);
}

// k_group_finish in radix 2^29 over raw segment sums (k_bucket_reduce29<G1Raw29>): the same
// out[g] = sum_j U_j + 2^log_seg sum_j j T_j + sum_j T_j, with the 1.4x faster carry-free product
// and no radix conversion of the inputs; the LDS tree holds raw accumulators (144 B per thread).
template <uint32_t GF_THREADS>
__global__ void __launch_bounds__(GF_THREADS) k_group_finish29(const G1Raw29* T, const G1Raw29* U, uint32_t S,
                                                              uint32_t log_seg, G1Xyzz* out) {
    __shared__ G1Raw29 sh[GF_THREADS];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const uint32_t nt = S < GF_THREADS ? S : GF_THREADS;
    const uint32_t Q = S / nt;
    G1X29 c, x;
    bool c_inf = true;
    if (t < nt) {
        const G1Raw29* Tg = T + (uint64_t)g * S + (uint64_t)t * Q;
        const G1Raw29* Ug = U + (uint64_t)g * S + (uint64_t)t * Q;
        G1X29 run, acc, us;
        bool run_inf = true, acc_inf = true, us_inf = true;
        for (uint32_t k = Q - 1; k >= 1; k--) {
            const bool inf = ld_raw29(Tg + k, x);
            acc29(run, run_inf, x, inf);
            acc29(acc, acc_inf, run, run_inf);
        }
        {
            const bool inf = ld_raw29(Tg, x);
            acc29(run, run_inf, x, inf);
        }
        for (uint32_t k = 0; k < Q; k++) {
            const bool inf = ld_raw29(Ug + k, x);
            acc29(us, us_inf, x, inf);
        }
        const uint32_t lo = t * Q;
        if (lo && !run_inf) {  // acc += lo * run (double-and-add, MSB first)
            G1X29 m;
            bool m_inf = true;
            for (int bit = 31 - __builtin_clz(lo); bit >= 0; bit--) {
                if (!m_inf) dbl29(m);
                if ((lo >> bit) & 1) acc29(m, m_inf, run, false);
            }
            acc29(acc, acc_inf, m, m_inf);
        }
        if (!acc_inf)
            for (uint32_t d = 0; d < log_seg; d++) dbl29(acc);
        acc29(us, us_inf, acc, acc_inf);
        acc29(us, us_inf, run, run_inf);
        c = us;
        c_inf = us_inf;
    }
    st_point(sh + t, c, c_inf);
    __syncthreads();
    for (uint32_t w = GF_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            const bool inf = ld_raw29(sh + t + w, x);
            acc29(c, c_inf, x, inf);
            st_point(sh + t, c, c_inf);
        }
        __syncthreads();
    }
    if (t == 0) st_xyzz(out + g, x29_to_xyzz(c, c_inf));
}

// After the first level (T_j, U_j of the S segments of each group): one block per group does
// the rest, out[g] = sum_j U_j + 2^log_seg sum_j j T_j + sum_j T_j (= sum_b (b + 1) B_b).
// Thread t takes segments [t Q, (t + 1) Q): running sums give its total and locally weighted sum,
// (t Q) times its total by double-and-add, then an LDS tree over the block.  One launch instead
// of the seg-level / tree / final chain (~12 latency-bound launches per batch).
template <uint32_t GF_THREADS>
__global__ void __launch_bounds__(GF_THREADS) k_group_finish(const G1Xyzz* T, const G1Xyzz* U, uint32_t S,
                                                            uint32_t log_seg, G1Xyzz* out) {
    __shared__ G1Xyzz sh[GF_THREADS];
    const uint32_t g = blockIdx.x, t = threadIdx.x;
    const uint32_t nt = S < GF_THREADS ? S : GF_THREADS;
    const uint32_t Q = S / nt;
    G1Xyzz c = xyzz_inf();
    if (t < nt) {
        const G1Xyzz* Tg = T + (uint64_t)g * S + (uint64_t)t * Q;
        const G1Xyzz* Ug = U + (uint64_t)g * S + (uint64_t)t * Q;
        G1Xyzz run = xyzz_inf(), acc = xyzz_inf(), us = xyzz_inf();
        for (uint32_t k = Q - 1; k >= 1; k--) {
            run = xyzz_add(run, ld_xyzz(Tg + k));
            acc = xyzz_add(acc, run);
        }
        run = xyzz_add(run, ld_xyzz(Tg));
        for (uint32_t k = 0; k < Q; k++) us = xyzz_add(us, ld_xyzz(Ug + k));
        if (t) acc = xyzz_add(acc, xyzz_mul_small(run, t * Q));
        for (uint32_t d = 0; d < log_seg; d++) acc = xyzz_dbl(acc);
        c = xyzz_add(xyzz_add(us, acc), run);
    }
    sh[t] = c;
    __syncthreads();
    for (uint32_t w = GF_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            G1Xyzz o = sh[t + w];
            pin(o);
            c = xyzz_add(c, o);
            sh[t] = c;
        }
        __syncthreads();
    }
    if (t == 0) st_xyzz(out + g, c);
}

// Few-groups form of k_bucket_reduce29 (a single MSM, the quotient chunks): segment s of group g
// (buckets [lo, lo + SEG), lo = s SEG; bucket b holds digit b + 1) sums its buckets' raw
// radix-2^29 pieces and returns sum_b (b + 1) B_b = running-sum form + lo * (sum_b B_b) -- the
// value of k_segment_sum over the bucket sums, without the combine / bucket-final passes.
__global__ void __launch_bounds__(64) k_segment_reduce29(const G1Raw29* pieces, const uint32_t* piece_off,
                                                         uint32_t B, uint32_t groups, G1Xyzz* seg_out) {
    const uint32_t nseg = B / SEG;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseg * groups) return;
    const uint32_t g = t / nseg, s = t % nseg;
    const uint32_t lo = s * SEG;
    G1X29 run, acc, x;
    bool run_inf = true, acc_inf = true;
    for (int k = (int)SEG - 1; k >= 0; k--) {
        const uint32_t bp = (lo + (uint32_t)k) * groups + g;
        const uint32_t e1 = piece_off[bp + 1];
        for (uint32_t e = piece_off[bp]; e < e1; e++) {
            const bool inf = ld_raw29(pieces + e, x);
            acc29(run, run_inf, x, inf);
        }
        acc29(acc, acc_inf, run, run_inf);
    }
    if (lo && !run_inf) {  // acc += lo * run (double-and-add, MSB first)
        G1X29 m;
        bool m_inf = true;
        for (int bit = 31 - __builtin_clz(lo); bit >= 0; bit--) {
            if (!m_inf) dbl29(m);
            if ((lo >> bit) & 1) acc29(m, m_inf, run, false);
        }
        acc29(acc, acc_inf, m, m_inf);
    }
    st_xyzz(seg_out + t, x29_to_xyzz(acc, acc_inf));
}

// Few groups with several pieces per bucket (a single 2^20 MSM: ~4.5), round 5.  Two short,
// wide kernels instead of combine level + bucket final + k_segment_sum in radix 2^32:
//   k_bucket_sums29   one thread per bucket (the whole MSM's buckets: 4 waves per SIMD at 2^18)
//                     sums its raw pieces -> raw bucket sum, group-major (g B + m)
//   k_segment_sum29   one thread per segment of SEG buckets: running sums of the bucket sums
//                     plus lo times their total by double-and-add, in radix 2^29 -> XYZZ
// then the k_tree_sum levels as before.  The sums are the same group elements as the combine path
// (exact EC arithmetic; only the order of additions differs).
__global__ void __launch_bounds__(256) k_bucket_sums29(const G1Raw29* pieces, const uint32_t* piece_off, uint32_t B,
                                                      uint32_t groups, G1Raw29* sums) {
    const uint32_t bp = blockIdx.x * blockDim.x + threadIdx.x;  // b' = m groups + g
    if (bp >= B * groups) return;
    G1X29 run, x;
    bool run_inf = true;
    const uint32_t e1 = piece_off[bp + 1];
    for (uint32_t e = piece_off[bp]; e < e1; e++) {
        const bool inf = ld_raw29(pieces + e, x);
        acc29(run, run_inf, x, inf);
    }
    const uint32_t g = bp % groups, m = bp / groups;
    st_point(sums + (uint64_t)g * B + m, run, run_inf);
}

// One thread per segment of `seg` bucket sums (seg29_for), 256 segments of one group per block
// (segments past the group's last are the identity): running sums and lo times their total, then
// the block's LDS tree -> one raw partial per block (part[g bpg + blk]).  Latency-bound (a 2^20
// MSM has 65536 segments: one wave per SIMD), so every addition / doubling issues its independent
// products together (add29_ilp / dbl29_ilp).
constexpr uint32_t SEG_BLOCK = 256;
// Buckets per k_segment_sum29 thread (seg29): the fewest (>= 4) that keep the threads within one
// wave per SIMD -- below that the waves are issue-bound alone and a shorter chain per wave is the
// gain (2^18 buckets: 4 per thread, 0.31 ms, against 8: 0.36 ms, half the SIMDs idle); above it
// the SIMDs share waves and the total work counts (2^19 buckets at 4: 0.60 ms, at 8: 0.43 ms).
// profiles/r05/s17.
static uint32_t seg29_for(uint64_t buckets) {
    uint32_t seg = 4;
    while (seg < 64 && buckets / seg > (1u << 16)) seg <<= 1;
    return seg;
}
__global__ void __launch_bounds__(SEG_BLOCK) k_segment_sum29(const G1Raw29* sums, uint32_t B, uint32_t seg,
                                                             uint32_t bpg, G1Raw29* part) {
    __shared__ G1Raw29 sh[SEG_BLOCK];
    const uint32_t nseg = B / seg;
    const uint32_t g = blockIdx.x / bpg, blk = blockIdx.x % bpg;
    const uint32_t s = blk * SEG_BLOCK + threadIdx.x;
    G1X29 acc, x;
    bool acc_inf = true;
    if (s < nseg) {
        const uint32_t lo = s * seg;
        const G1Raw29* sb = sums + (uint64_t)g * B + lo;
        G1X29 run;
        bool run_inf = true;
        for (int k = (int)seg - 1; k >= 0; k--) {  // bucket lo + k holds digit lo + k + 1
            const bool inf = ld_raw29(sb + k, x);
            acc29_ilp(run, run_inf, x, inf);
            acc29_ilp(acc, acc_inf, run, run_inf);
        }
        if (lo && !run_inf) {  // acc += lo * run (double-and-add, MSB first)
            G1X29 m;
            bool m_inf = true;
            for (int bit = 31 - __builtin_clz(lo); bit >= 0; bit--) {
                if (!m_inf) dbl29_ilp(m);
                if ((lo >> bit) & 1) acc29_ilp(m, m_inf, run, false);
            }
            acc29_ilp(acc, acc_inf, m, m_inf);
        }
    }
    st_point(sh + threadIdx.x, acc, acc_inf);
    __syncthreads();
    for (uint32_t w = SEG_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const bool inf = ld_raw29(sh + threadIdx.x + w, x);
            acc29_ilp(acc, acc_inf, x, inf);
            st_point(sh + threadIdx.x, acc, acc_inf);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) st_point(part + blockIdx.x, acc, acc_inf);
}

// out[g] = sum of part[g bpg .. (g + 1) bpg), one block per group (LDS tree, radix 2^29)
__global__ void __launch_bounds__(SEG_BLOCK) k_tree_sum29(const G1Raw29* part, uint32_t bpg, G1Xyzz* out) {
    __shared__ G1Raw29 sh[SEG_BLOCK];
    G1X29 acc, x;
    bool acc_inf = true;
    for (uint32_t i = threadIdx.x; i < bpg; i += SEG_BLOCK) {
        const bool inf = ld_raw29(part + (uint64_t)blockIdx.x * bpg + i, x);
        acc29_ilp(acc, acc_inf, x, inf);
    }
    st_point(sh + threadIdx.x, acc, acc_inf);
    __syncthreads();
    for (uint32_t w = SEG_BLOCK / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const bool inf = ld_raw29(sh + threadIdx.x + w, x);
            acc29_ilp(acc, acc_inf, x, inf);
            st_point(sh + threadIdx.x, acc, acc_inf);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) st_xyzz(out + blockIdx.x, x29_to_xyzz(acc, acc_inf));
}

// out[g * gridDim.x + blk] = sum of in[g * n + blk * TREE .. + TREE)
__global__ void __launch_bounds__(TREE) k_tree_sum(const G1Xyzz* in, uint32_t n, G1Xyzz* out) {
    __shared__ G1Xyzz sh[TREE];
    const uint32_t g = blockIdx.y;
    const uint32_t i = blockIdx.x * TREE + threadIdx.x;
    G1Xyzz acc = i < n ? ld_xyzz(in + (uint64_t)g * n + i) : xyzz_inf();
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t w = TREE / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            G1Xyzz o = sh[threadIdx.x + w];
            pin(o);
            acc = xyzz_add(acc, o);
            sh[threadIdx.x] = acc;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) st_xyzz(out + (uint64_t)g * gridDim.x + blockIdx.x, acc);
}

// per-window sums -> per-column result: sum_w 2^(c*w) * G[col*W + w] (one thread per column)
__global__ void k_window_horner(const G1Xyzz* gs, uint32_t cols, uint32_t W, uint32_t c,
                                G1Xyzz* out) {
    const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= cols) return;
    const G1Xyzz* g = gs + (uint64_t)col * W;
    G1Xyzz acc = ld_xyzz(g + W - 1);
    for (int w = (int)W - 2; w >= 0; w--) {
        for (uint32_t k = 0; k < c; k++) acc = xyzz_dbl(acc);
        acc = xyzz_add(acc, ld_xyzz(g + w));
    }
    st_xyzz(out + col, acc);
}

// The route of a counted batch.  Called once per batch, by batch_counts, which stores the answer
// (Batch::route); it depends on the batch's counts and the layout alone.
Reduce reduce_route(const Batch& bt, const MsmLayout& L) {
    const bool one_level = bt.levels <= 1;  // no bucket holds more than PIECE pieces
    // batches below COLUMN_BATCH_GROUPS (a single MSM) use the shorter-chain k_segment_sum (running
    // sums + lo * run) + k_tree_sum: there latency, not additions, sets the time
    const bool few_groups = bt.groups < COLUMN_BATCH_GROUPS;
    // the reduction reads k_piece_sum29's raw partials directly (k_bucket_reduce29 /
    // k_segment_reduce29): radix-2^29 pieces, no combine level needed, and either many groups or few
    // pieces per bucket -- with few groups and several pieces per bucket (a single 2^20 MSM: ~4.5)
    // the one-thread-per-segment chain is longer than combine + bucket-final + k_segment_sum
    // (3.23 vs 3.00 ms for the 2^20 MSM)
    if (one_level && (!few_groups || (uint64_t)bt.n_pieces <= 2ull * bt.nb)) {
        if (few_groups) return Reduce::FusedSegments;
        // fixed-base layouts: first level only; the finish runs once per call (prepare_deferred,
        // run_deferred_finish)
        return L.precomputed ? Reduce::Deferred : Reduce::FusedGroups;
    }
    // few groups, several pieces per bucket, none above PIECE: k_bucket_sums29 + k_segment_sum29
    // (round 5; the combine-level path stays for skewed inputs, whose buckets hold more pieces)
    if (one_level && few_groups) return Reduce::Sums29;
    // combine levels until every bucket holds one partial (skewed scalars put many pieces in a
    // bucket: all-equal scalars put n pieces in one bucket per window)
    return few_groups ? Reduce::CombineSegments : Reduce::CombineGroups;
}

// per-column output step shared by both bucket reductions
static Status write_columns(const MsmLayout& L, const Batch& bt, const G1Xyzz* per_group,
                            hipStream_t st) {
    // one point per group; per column: the group itself (fixed base) or the Horner combination of
    // its windows
    if (!L.precomputed) {
        hipLaunchKernelGGL(k_window_horner, dim3(blocks_for(bt.cols, 64)), dim3(64), 0, st, per_group,
                           bt.cols, bt.W, bt.c, bt.out);
        EON_HIP(hipGetLastError());
    } else {
        EON_HIP(hipMemcpyAsync(bt.out, per_group, bt.cols * sizeof(G1Xyzz), hipMemcpyDeviceToDevice, st));
    }
    return Status::ok();
}

// sum_d d * B_d per group, few-groups form: k_segment_sum + LDS trees (short dependency chains).
// The segment routes open alike: the two segment buffers and the k_segment_sum record
static Status begin_segments(eon_ctx* ctx, const Batch& bt, MsmWork& wk, hipStream_t st) {
    const uint32_t nseg = bt.B / SEG;
    EON_HIP(ctx_ensure(ctx, wk.red_a, (uint64_t)bt.groups * nseg * sizeof(G1Xyzz)));
    EON_HIP(ctx_ensure(ctx, wk.red_b, (uint64_t)bt.groups * nseg * sizeof(G1Xyzz)));
    ctx->prof.begin("k_segment_sum", (uint64_t)bt.nb * 128 + (uint64_t)bt.groups * nseg * 128, st);
    return Status::ok();
}

// closes the k_segment_sum record; B / SEG segment sums per group in wk.red_a -> k_tree_sum levels
// -> the columns
static Status tree_sum_segments(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, MsmWork& wk, hipStream_t st) {
    ctx->prof.end(st);
    G1Xyzz* cur = wk.red_a.as<G1Xyzz>();
    G1Xyzz* nxt = wk.red_b.as<G1Xyzz>();
    uint32_t len = bt.B / SEG;
    while (len > 1) {
        const uint32_t blk = (len + TREE - 1) / TREE;
        hipLaunchKernelGGL(k_tree_sum, dim3(blk, bt.groups), dim3(TREE), 0, st, cur, len, nxt);
        std::swap(cur, nxt);
        len = blk;
    }
    EON_HIP(hipGetLastError());
    return write_columns(L, bt, cur, st);
}

// k_group_finish over the deferred rows (merged into maximal runs) on `st`
Status run_deferred_finish(eon_ctx* ctx, DeferredFinish& df, hipStream_t st) {
    if (df.rows.empty()) return Status::ok();
    std::sort(df.rows.begin(), df.rows.end());
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    for (auto& r : df.rows) {
        if (!runs.empty() && runs.back().first + runs.back().second == r.first)
            runs.back().second += r.second;
        else
            runs.push_back(r);
    }
    for (auto& r : runs) {
        ctx->prof.begin("k_group_finish", r.second * df.nseg * 256ull, st, r.second * df.nseg * 3ull * 14);
        hipLaunchKernelGGL(k_group_finish29<FINISH_THREADS>, dim3((uint32_t)r.second), dim3(FINISH_THREADS), 0, st,
                           df.T + r.first * df.nseg, df.U + r.first * df.nseg, df.nseg, LOG_SEG,
                           df.out_base + r.first);
        EON_HIP(hipGetLastError());
        ctx->prof.end(st);
    }
    df.rows.clear();
    return Status::ok();
}

// the call-wide arrays of a fixed-base layout: exactly the layouts whose column batches take the
// Deferred route (reduce_route)
Status prepare_deferred(eon_ctx* ctx, const MsmLayout& L, uint64_t rows, G1Xyzz* out_base, DeferredFinish& df) {
    df = DeferredFinish{};
    if (!L.precomputed) return Status::ok();
    df.nseg = (1u << (L.c - 1)) / SEG;
    EON_HIP(ctx_ensure(ctx, ctx->fin_T, rows * df.nseg * sizeof(G1Raw29)));
    EON_HIP(ctx_ensure(ctx, ctx->fin_U, rows * df.nseg * sizeof(G1Raw29)));
    df.T = ctx->fin_T.as<G1Raw29>();
    df.U = ctx->fin_U.as<G1Raw29>();
    df.out_base = out_base;
    return Status::ok();
}

// combine levels until every bucket holds one partial, then the bucket sums (wk.bucket_sums,
// group-major) of the Combine routes
static Status combine_levels(eon_ctx* ctx, const Batch& bt, const SortedRef& sr, MsmWork& wk, hipStream_t st) {
    const uint32_t nb = bt.nb;
    const uint32_t* off_cur = sr.piece_off;
    uint32_t* off_bufs[2] = {wk.off2.as<uint32_t>(), wk.off3.as<uint32_t>()};
    int next_off = 0;
    G1Xyzz* part_cur = wk.piece_sums.as<G1Xyzz>();
    G1Xyzz* part_nxt = wk.piece_sums2.as<G1Xyzz>();
    uint64_t bound = bt.n_pieces;  // >= the partials of the current level
    for (uint32_t level = 0; level < bt.levels; level++) {
        uint32_t* off_nxt = off_bufs[next_off];
        hipLaunchKernelGGL(k_level_count, dim3(blocks_for(nb + 1, 256)), dim3(256), 0, st, off_cur,
                           nb, wk.count.as<uint32_t>());
        EON_HIP(exclusive_scan_u32(wk.temp.p, wk.count.as<uint32_t>(), off_nxt, nb + 1, st));
        hipLaunchKernelGGL(k_piece_owner, dim3(blocks_for(nb, 256)), dim3(256), 0, st, off_nxt, nb,
                           wk.owner.as<uint32_t>());
        // sum_b ceil(p_b / PIECE) <= min(bound, nb + bound / PIECE)
        const uint64_t nxt = std::min<uint64_t>(bound, nb + bound / PIECE);
        ctx->prof.begin("k_partial_combine", (bound + nxt) * 128, st, (bound - std::min(bound, nxt)) * 14);
        hipLaunchKernelGGL(k_partial_combine, dim3(blocks_for(nxt, 64)), dim3(64), 0, st, off_cur, off_nxt,
                           wk.owner.as<uint32_t>(), nb, part_cur, part_nxt);
        ctx->prof.end(st);
        off_cur = off_nxt;
        next_off ^= 1;
        std::swap(part_cur, part_nxt);
        bound = nxt;
    }
    hipLaunchKernelGGL(k_bucket_final, dim3(blocks_for(nb, 256)), dim3(256), 0, st, off_cur, bt.B, bt.groups,
                       part_cur, wk.bucket_sums.as<G1Xyzz>());
    return Status::ok();
}

static Status reduce_fused_segments(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const SortedRef& sr,
                                    MsmWork& wk, hipStream_t st) {
    EON_TRY(begin_segments(ctx, bt, wk, st));
    hipLaunchKernelGGL(k_segment_reduce29, dim3(blocks_for((uint64_t)bt.B / SEG * bt.groups, 64)), dim3(64), 0, st,
                       wk.piece_raw.as<G1Raw29>(), sr.piece_off, bt.B, bt.groups, wk.red_a.as<G1Xyzz>());
    return tree_sum_segments(ctx, L, bt, wk, st);
}

static Status reduce_combine_segments(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const SortedRef& sr,
                                      MsmWork& wk, hipStream_t st) {
    EON_TRY(combine_levels(ctx, bt, sr, wk, st));
    EON_TRY(begin_segments(ctx, bt, wk, st));
    hipLaunchKernelGGL(k_segment_sum, dim3(blocks_for((uint64_t)bt.B / SEG * bt.groups, 64)), dim3(64), 0, st,
                       wk.bucket_sums.as<G1Xyzz>(), bt.B, bt.groups, wk.red_a.as<G1Xyzz>());
    return tree_sum_segments(ctx, L, bt, wk, st);
}

static Status reduce_sums29(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const SortedRef& sr, MsmWork& wk,
                            hipStream_t st) {
    const uint32_t groups = bt.groups;
    ctx->prof.begin("k_bucket_sums29", (uint64_t)bt.n_pieces * 144 + (uint64_t)bt.nb * 144, st);
    hipLaunchKernelGGL(k_bucket_sums29, dim3(blocks_for(bt.nb, 256)), dim3(256), 0, st, wk.piece_raw.as<G1Raw29>(),
                       sr.piece_off, bt.B, groups, wk.piece_sums.as<G1Raw29>());
    ctx->prof.end(st);
    EON_HIP(hipGetLastError());
    EON_TRY(begin_segments(ctx, bt, wk, st));
    // raw bucket sums (k_bucket_sums29, in wk.piece_sums as G1Raw29) -> one raw partial per
    // 256 segments -> one point per group, all in radix 2^29
    const uint32_t seg = std::min(bt.B, seg29_for((uint64_t)bt.B * groups));
    const uint32_t bpg = (bt.B / seg + SEG_BLOCK - 1) / SEG_BLOCK;
    EON_HIP(ctx_ensure(ctx, wk.red_b, (uint64_t)groups * bpg * sizeof(G1Raw29)));
    hipLaunchKernelGGL(k_segment_sum29, dim3(groups * bpg), dim3(SEG_BLOCK), 0, st, wk.piece_sums.as<G1Raw29>(),
                       bt.B, seg, bpg, wk.red_b.as<G1Raw29>());
    hipLaunchKernelGGL(k_tree_sum29, dim3(groups), dim3(SEG_BLOCK), 0, st, wk.red_b.as<G1Raw29>(), bpg,
                       wk.red_a.as<G1Xyzz>());
    ctx->prof.end(st);
    EON_HIP(hipGetLastError());
    return write_columns(L, bt, wk.red_a.as<G1Xyzz>(), st);
}

// the batch's first-level segment sums into its rows of the call-wide arrays (DeferredFinish)
static Status reduce_deferred(eon_ctx* ctx, const Batch& bt, const SortedRef& sr, MsmWork& wk, hipStream_t st,
                              DeferredFinish& df) {
    const uint64_t row0 = (uint64_t)(bt.out - df.out_base);
    if (!bt.bucket_lanes) EON_TRY(piece_merge(ctx, bt, sr, wk, st));
    ctx->prof.begin("bucket_reduce", (uint64_t)bt.nb * 128 + (uint64_t)bt.nb / SEG * 256, st);
    hipLaunchKernelGGL((bt.bucket_lanes ? k_bucket_reduce29<G1Raw29, true> : k_bucket_reduce29<G1Raw29, false>),
                       dim3(blocks_for((uint64_t)df.nseg * bt.groups, 64)), dim3(64), 0, st,
                       wk.piece_raw.as<G1Raw29>(), sr.piece_off, bt.B, SEG, bt.groups, df.T + row0 * df.nseg,
                       df.U + row0 * df.nseg);
    ctx->prof.end(st);
    EON_HIP(hipGetLastError());
    df.rows.emplace_back(row0, bt.groups);
    return Status::ok();
}

// sum_d d * B_d per group (bucket b holds digit b + 1): segment sums T, U of SEG buckets
// (k_bucket_reduce29 from the raw pieces, or k_seg_level from bucket sums), then k_group_finish
struct GroupLevel {
    G1Xyzz *T, *U;
    uint32_t nseg;
};

// the group routes open alike: the per-group buffer and the bucket_reduce record
static Status begin_groups(eon_ctx* ctx, const Batch& bt, MsmWork& wk, hipStream_t st, GroupLevel& g) {
    g.T = wk.piece_sums.as<G1Xyzz>();
    g.U = wk.piece_sums2.as<G1Xyzz>();
    EON_HIP(wk.red_a.ensure((uint64_t)bt.groups * sizeof(G1Xyzz)));
    ctx->prof.begin("bucket_reduce", (uint64_t)bt.nb * 128 + (uint64_t)bt.nb / SEG * 256, st);
    g.nseg = bt.B / SEG;
    return Status::ok();
}

// k_group_finish over the segment sums (closing the bucket_reduce record), then the columns
static Status finish_groups(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const GroupLevel& g, MsmWork& wk,
                            hipStream_t st) {
    G1Xyzz* per_group = wk.red_a.as<G1Xyzz>();
    hipLaunchKernelGGL(k_group_finish<FINISH_THREADS>, dim3(bt.groups), dim3(FINISH_THREADS), 0, st, g.T, g.U, g.nseg,
                       LOG_SEG, per_group);
    ctx->prof.end(st);
    EON_HIP(hipGetLastError());
    return write_columns(L, bt, per_group, st);
}

static Status reduce_fused_groups(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const SortedRef& sr,
                                  MsmWork& wk, hipStream_t st) {
    GroupLevel g;
    EON_TRY(begin_groups(ctx, bt, wk, st, g));
    if (!bt.bucket_lanes) EON_TRY(piece_merge(ctx, bt, sr, wk, st));
    hipLaunchKernelGGL((bt.bucket_lanes ? k_bucket_reduce29<G1Xyzz, true> : k_bucket_reduce29<G1Xyzz, false>),
                       dim3(blocks_for((uint64_t)g.nseg * bt.groups, 64)), dim3(64), 0, st,
                       wk.piece_raw.as<G1Raw29>(), sr.piece_off, bt.B, SEG, bt.groups, g.T, g.U);
    return finish_groups(ctx, L, bt, g, wk, st);
}

static Status reduce_combine_groups(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const SortedRef& sr,
                                    MsmWork& wk, hipStream_t st) {
    EON_TRY(combine_levels(ctx, bt, sr, wk, st));
    GroupLevel g;
    EON_TRY(begin_groups(ctx, bt, wk, st, g));
    hipLaunchKernelGGL(k_seg_level, dim3(blocks_for((uint64_t)g.nseg * bt.groups, 64)), dim3(64), 0, st,
                       wk.bucket_sums.as<G1Xyzz>(), bt.B, SEG, bt.groups, g.T, g.U);
    return finish_groups(ctx, L, bt, g, wk, st);
}

// combine levels, bucket sums and the weighted bucket reduction of one batch's pieces by the
// batch's stored route (Batch::route; no read-backs: the counts came with batch_counts); leaves one XYZZ
// point per column at bt.out, or, deferred, the group's segment sums in df's rows.  The
// sorted piece offsets are only read (a prepared batch is reduced once per bases object).
Status batch_reduce(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const SortedRef& sr, MsmWork& wk,
                    hipStream_t st, DeferredFinish& df) {
    if (!bt.counted) return Status::err(EON_E_ARG, "an MSM batch is counted before its reduction");
    switch (bt.route) {
        case Reduce::Deferred:
            if (!df.T) return Status::err(EON_E_ARG, "a Deferred MSM batch without the call's deferred-finish arrays");
            return reduce_deferred(ctx, bt, sr, wk, st, df);
        case Reduce::FusedGroups: return reduce_fused_groups(ctx, L, bt, sr, wk, st);
        case Reduce::FusedSegments: return reduce_fused_segments(ctx, L, bt, sr, wk, st);
        case Reduce::Sums29: return reduce_sums29(ctx, L, bt, sr, wk, st);
        case Reduce::CombineGroups: return reduce_combine_groups(ctx, L, bt, sr, wk, st);
        case Reduce::CombineSegments: return reduce_combine_segments(ctx, L, bt, sr, wk, st);
    }
    return Status::err(EON_E_ARG, "unknown bucket reduction route");
}

}  // namespace eon
