// MSM stage 1: scalars -> sorted digit pairs, bucket starts, piece offsets and bucket order of one
// batch (batch_sort), the count read-back that fixes the batch's plan (batch_counts), and a single
// MSM's active windows.  The pipeline is described in msm.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "msm_batch.h"
#include "sort.h"
#include "sort_pass.h"

namespace eon {

__device__ __forceinline__ uint32_t window_bits(const uint32_t* s, uint32_t pos, uint32_t c) {
    // bits [pos, pos + c) of the 256-bit canonical scalar s (little-endian u32 limbs), c <= 24
    const uint32_t li = pos >> 5, off = pos & 31;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        lo = (j == li) ? s[j] : lo;
        hi = (j == li + 1) ? s[j] : hi;
    }
    const uint64_t v = ((uint64_t)hi << 32 | lo) >> off;
    return (uint32_t)v & ((1u << c) - 1);
}

// Digit pairs.  Key of a nonzero digit: (group << c) | (|digit| - 1), group = the column
// (fixed-base mode: every window shares the column's bucket set) or (column, window); zero digits
// get the sentinel 0xFFFFFFFF.  Pairs are emitted group-major (e = group * n + i: (col * W + w) * n
// + i in both modes) and radix-sorted on the low c key bits only -- 2 passes of the stable
// onesweep instead of 3 on the full key -- so equal magnitudes stay in group order: the sorted
// pairs run over buckets b' = (|digit| - 1) * groups + group, each contiguous.
constexpr uint32_t DIGIT_COLS = 4;  // widest scalar tile of one 256-thread block: 64 rows x 4 cols

// The digit sort's per-pass histograms of the keys (radix_sort_histograms) are counted here, in
// LDS per block and added to the global bins once per block, so the sort never re-reads the keys
// for them.  Blocks walk row tiles grid-stride (the grid is capped near DIGIT_BLOCKS): every block
// adds its bins to the same few hundred global counters, so one block per tile would put
// ~E / 8 atomics on those addresses.
constexpr uint32_t DIGIT_BLOCKS = 4096;

// canonical x from its Montgomery form x 2^256 (any 256-bit input): the radix-2^29 product by the
// plain integer 32 is x 2^256 32 2^-261 = x, under half the instructions of the radix-2^32
// to_canonical
__device__ __forceinline__ Fr canonical_from_mont(const Fr& a) {
    F29 thirty_two;
#pragma unroll
    for (int j = 0; j < 9; j++) thirty_two.l[j] = j == 0 ? 32u : 0u;
    return pack29<FrP>(canon29<FrP>(mul29<FrP>(unpack29(a), thirty_two)));
}

__global__ void __launch_bounds__(256) k_msm_digits(const Fr* scalars, uint64_t n, uint64_t ld,
                                                    uint32_t cols, uint32_t c, uint32_t windows,
                                                    uint32_t ref_windows, uint32_t precomputed,
                                                    uint32_t tile_cols, uint32_t* keys, uint32_t* vals,
                                                    RadixPasses pb, uint32_t* hist, Fr* /* k_msm_digits4's */) {
    __shared__ uint32_t h[RADIX_SORT_MAX_PASSES][256];
    for (uint32_t j = threadIdx.x; j < RADIX_SORT_MAX_PASSES * 256; j += 256) (&h[0][0])[j] = 0;
    __syncthreads();
    // a tile is 256 / tile_cols row segments of tile_cols adjacent columns (up to 128 contiguous
    // bytes), so the group-major writes stay in runs of consecutive rows
    const uint32_t col = blockIdx.y * tile_cols + threadIdx.x % tile_cols;
    const uint32_t rows = 256 / tile_cols;
    const uint32_t B = 1u << (c - 1);
    for (uint64_t i = (uint64_t)blockIdx.x * rows + threadIdx.x / tile_cols; col < cols && i < n;
         i += (uint64_t)gridDim.x * rows) {
        Fr s = canonical_from_mont(ld_pinned(scalars + i * ld + col));
        pin(s);
        uint32_t carry = 0;
        for (uint32_t w = 0; w < windows; w++) {
            const uint32_t raw = window_bits(s.v, w * c, c) + carry;
            uint32_t mag;
            uint32_t neg;
            if (raw > B) {  // signed digit raw - 2^c in [-(B-1), -1], carry into the next window
                mag = (1u << c) - raw;
                neg = 1;
                carry = 1;
            } else {
                mag = raw;
                neg = 0;
                carry = 0;
            }
            const uint64_t e = ((uint64_t)col * windows + w) * n + i;
            uint32_t key;
            if (mag == 0) {
                key = 0xFFFFFFFFu;
                vals[e] = 0;
            } else {
                const uint32_t g = precomputed ? col : col * windows + w;
                key = (g << c) | (mag - 1);
                const uint32_t ref = precomputed ? (uint32_t)(i * ref_windows + w) : (uint32_t)i;
                vals[e] = ref | (neg << 31);
            }
            keys[e] = key;
#pragma unroll
            for (uint32_t p = 0; p < RADIX_SORT_MAX_PASSES; p++)
                if (p < pb.passes) atomicAdd(&h[p][(key >> pb.shift[p]) & ((1u << pb.bits[p]) - 1)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < pb.passes * 256; j += 256) {
        const uint32_t v = (&h[0][0])[j];
        if (v) atomicAdd(hist + j, v);
    }
}

// The same pairs with four consecutive rows per thread (n a multiple of 4): a lane writes a
// window's four keys and four references as one 16-byte store each, so a store instruction covers
// tile_cols runs of 16 * 4 rows (256 contiguous bytes per column) instead of tile_cols runs of 64
// bytes.  A tile is 256 / tile_cols row quads of tile_cols adjacent columns.  WRITE = false: the
// histograms and the canonical scalars column-major (canon[col n + i]) instead of the pairs, for
// the fused first sort pass (k_digit_sort_pass computes the pairs again from them).
template <bool WRITE>
__global__ void __launch_bounds__(256) k_msm_digits4(const Fr* scalars, uint64_t n, uint64_t ld,
                                                     uint32_t cols, uint32_t c, uint32_t windows,
                                                     uint32_t ref_windows, uint32_t precomputed,
                                                     uint32_t tile_cols, uint32_t* keys, uint32_t* vals,
                                                     RadixPasses pb, uint32_t* hist, Fr* canon) {
    __shared__ uint32_t h[RADIX_SORT_MAX_PASSES][256];
    for (uint32_t j = threadIdx.x; j < RADIX_SORT_MAX_PASSES * 256; j += 256) (&h[0][0])[j] = 0;
    __syncthreads();
    const uint32_t col = blockIdx.y * tile_cols + threadIdx.x % tile_cols;
    const uint32_t quads = 256 / tile_cols;
    const uint32_t B = 1u << (c - 1);
    for (uint64_t i = ((uint64_t)blockIdx.x * quads + threadIdx.x / tile_cols) * 4; col < cols && i < n;
         i += (uint64_t)gridDim.x * quads * 4) {
        Fr s[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            s[r] = canonical_from_mont(ld_pinned(scalars + (i + r) * ld + col));
            pin(s[r]);
        }
        if (!WRITE) {  // the canonical scalars, column-major, for the fused first sort pass
#pragma unroll
            for (int r = 0; r < 4; r++) st_vec(canon + (uint64_t)col * n + i + r, s[r]);
        }
        uint32_t carry[4] = {0, 0, 0, 0};
        for (uint32_t w = 0; w < windows; w++) {
            uint32_t key[4], val[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint32_t raw = window_bits(s[r].v, w * c, c) + carry[r];
                uint32_t mag, neg;
                if (raw > B) {  // signed digit raw - 2^c in [-(B-1), -1], carry into the next window
                    mag = (1u << c) - raw;
                    neg = 1;
                    carry[r] = 1;
                } else {
                    mag = raw;
                    neg = 0;
                    carry[r] = 0;
                }
                if (mag == 0) {
                    key[r] = 0xFFFFFFFFu;
                    val[r] = 0;
                } else {
                    const uint32_t g = precomputed ? col : col * windows + w;
                    key[r] = (g << c) | (mag - 1);
                    const uint32_t ref = precomputed ? (uint32_t)((i + r) * ref_windows + w) : (uint32_t)(i + r);
                    val[r] = ref | (neg << 31);
                }
#pragma unroll
                for (uint32_t p = 0; p < RADIX_SORT_MAX_PASSES; p++)
                    if (p < pb.passes) atomicAdd(&h[p][(key[r] >> pb.shift[p]) & ((1u << pb.bits[p]) - 1)], 1u);
            }
            if (WRITE) {
                const uint64_t e = ((uint64_t)col * windows + w) * n + i;
                *reinterpret_cast<uint4*>(keys + e) = make_uint4(key[0], key[1], key[2], key[3]);
                *reinterpret_cast<uint4*>(vals + e) = make_uint4(val[0], val[1], val[2], val[3]);
            }
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < pb.passes * 256; j += 256) {
        const uint32_t v = (&h[0][0])[j];
        if (v) atomicAdd(hist + j, v);
    }
}

// The first (low-byte) pass of the digit sort fused with the digit extraction, for fixed-base
// tables with c = 16 and 16 windows: the pairs are ranked as they are computed from the scalars,
// never written unsorted nor read back (k_msm_digits4 + the first k_sort_pass moved 8 + 16 bytes
// per pair; this pass reads 2 of canonical scalar, coalesced, and writes 8; the histogram kernel
// before it writes the canonical scalars column-major).  Tile t covers rows [r0, r0 + SORT_THREADS)
// of column col = t / tiles_per_col (r0 = (t % tiles_per_col) SORT_THREADS, n a multiple of
// SORT_THREADS): thread (w, lane) takes row r0 + 64 w + lane and its 16 window digits are its 16
// items.  Within a column the pairs are ranked in another order than k_msm_digits' (window-major),
// but the tiles run column by column, so after both passes every bucket (digit, column) is still
// one contiguous run -- the only order the piece sums rely on (a bucket's sum is order-free).
struct DigitSource {
    const Fr* canon;  // canonical scalars, column-major (k_msm_digits4<false>)
    uint64_t n;
    uint32_t tiles_per_col, ref_windows;
    template <bool FULL>
    __device__ __forceinline__ void load(uint32_t tile, uint32_t w, uint32_t lane, uint32_t,
                                         uint32_t (&key)[sortpass::SORT_ITEMS],
                                         uint32_t (&val)[sortpass::SORT_ITEMS]) const {
        static_assert(sortpass::SORT_ITEMS == 16, "one item per 16-bit window of a 256-bit scalar");
        const uint32_t col = tile / tiles_per_col;
        const uint64_t i = (uint64_t)(tile - col * tiles_per_col) * sortpass::SORT_THREADS + w * 64 + lane;
        const Fr s = ld_pinned(canon + (uint64_t)col * n + i);
        uint32_t carry = 0;
#pragma unroll
        for (uint32_t j = 0; j < 16; j++) {
            const uint32_t raw = ((s.v[j >> 1] >> (16 * (j & 1))) & 0xffffu) + carry;
            uint32_t mag, neg;
            if (raw > (1u << 15)) {  // signed digit raw - 2^16, carry into the next window
                mag = (1u << 16) - raw;
                neg = 1;
                carry = 1;
            } else {
                mag = raw;
                neg = 0;
                carry = 0;
            }
            key[j] = mag ? (col << 16 | (mag - 1)) : 0xFFFFFFFFu;
            val[j] = mag ? ((uint32_t)(i * ref_windows + j) | neg << 31) : 0u;
        }
    }
};

__global__ void __launch_bounds__(sortpass::SORT_THREADS) k_digit_sort_pass(DigitSource src, uint32_t* kd, uint32_t* vd,
                                                                            uint32_t n, uint32_t shift,
                                                                            const uint32_t* base, uint64_t* status,
                                                                            uint32_t* tile_ctr) {
    sortpass::sort_pass_tile<8>(src, kd, vd, n, shift, 8, base, status, tile_ctr);
}

// OR of every canonical scalar into or_out[8] (zeroed before): its top set bit bounds the
// digits a single MSM needs (active windows, msm_run_columns)
constexpr uint32_t SCALAR_OR_COPIES = 64;
__global__ void __launch_bounds__(256) k_scalar_or(const Fr* scalars, uint64_t n, uint32_t* or_out) {
    __shared__ uint32_t acc[8];
    if (threadIdx.x < 8) acc[threadIdx.x] = 0;
    __syncthreads();
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Fr s = canonical_from_mont(ld_pinned(scalars + i));
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] |= s.v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t x = v[j];
        for (int o = 32; o > 0; o >>= 1) x |= (uint32_t)__shfl_xor(x, o);
        if ((threadIdx.x & 63) == 0 && x) atomicOr(&acc[j], x);
    }
    __syncthreads();
    // SCALAR_OR_COPIES copies of the 8 words (block b ORs into copy b % SCALAR_OR_COPIES): few
    // atomics per address -- one copy's 32k atomics from 4096 blocks took 56 us (profiles/r05/s14)
    if (threadIdx.x < 8 && acc[threadIdx.x])
        atomicOr(or_out + (blockIdx.x % SCALAR_OR_COPIES) * 8 + threadIdx.x, acc[threadIdx.x]);
}

// start[b'] = index of the first sorted pair in bucket >= b', for b' in [0, nb]; each thread
// handles BS_KEYS consecutive pairs, its BS_KEYS / 4 16-byte loads issued together (more bytes in
// flight per wave: one 16-byte load per thread ran the kernel at ~3.8 TB/s), plus the key before
// its range; E a multiple of 4 (the MSM's pair counts), a partial last group per element
constexpr uint32_t BS_KEYS = 16;
__global__ void __launch_bounds__(256) k_bucket_start(const uint32_t* keys, uint64_t E, uint32_t c, uint32_t groups,
                                                      uint32_t nb, uint32_t* start) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * BS_KEYS;
    if (i0 > E) return;
    uint32_t k[BS_KEYS];
    if (i0 + BS_KEYS <= E && (E & 3) == 0) {
#pragma unroll
        for (uint32_t q = 0; q < BS_KEYS / 4; q++) {
            const uint4 v = *reinterpret_cast<const uint4*>(keys + i0 + 4 * q);
            k[4 * q] = v.x; k[4 * q + 1] = v.y; k[4 * q + 2] = v.z; k[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < BS_KEYS; j++) k[j] = i0 + j < E ? keys[i0 + j] : 0u;
    }
    int64_t prev = i0 == 0 ? -1 : (int64_t)bucket_of(keys[i0 - 1], c, groups, nb);
#pragma unroll
    for (uint32_t j = 0; j < BS_KEYS; j++) {
        const uint64_t i = i0 + j;
        if (i > E) break;
        const int64_t cur = i == E ? (int64_t)nb : (int64_t)bucket_of(k[j], c, groups, nb);
        for (int64_t b = prev + 1; b <= cur; b++) start[b] = (uint32_t)i;
        prev = cur;
    }
}

// Bucket order of the one-bucket-per-lane piece sums (k_piece_sum_bucket29): per window of
// ORDER_WINDOW consecutive bucket indices, the indices stably sorted by run length
// start[b + 1] - start[b], shortest first, so that 64 consecutive entries -- one wave -- hold runs of
// nearly equal length (uniform scalars: 0.999 of the lane slots busy against 0.766 in index order).
// One block per window, a counting sort: an LDS histogram of the lengths (those above ORDER_CAP
// share the last bin, in index order), its scan, then tiles of ORDER_THREADS buckets in index order,
// each lane ranked among the equal lengths of its wave by ballots and each wave behind the earlier
// waves of its tile.  The batch's longest run goes to *max_run (zeroed by the caller).
// The window keeps a wave's 64 runs inside the pairs of 2^15 neighbouring buckets (~8 MB of `vals`
// at the prove's 64 pairs per bucket): sorting the whole batch instead would spread them over all
// of it for no utilisation left to gain.
constexpr uint32_t ORDER_THREADS = 512, ORDER_WAVES = ORDER_THREADS / 64;
__global__ void __launch_bounds__(ORDER_THREADS) k_bucket_order(const uint32_t* start, uint32_t nb, uint32_t* order,
                                                                uint32_t* max_run) {
    __shared__ uint32_t base[ORDER_BINS];                  // next free slot of every length
    __shared__ uint32_t wave_cnt[ORDER_WAVES][ORDER_BINS];  // the tile's buckets per wave and length
    __shared__ uint32_t longest;
    const uint32_t b0 = blockIdx.x * ORDER_WINDOW;
    const uint32_t b1 = min(b0 + ORDER_WINDOW, nb);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < ORDER_BINS; i += ORDER_THREADS) base[i] = 0;
    if (tid == 0) longest = 0;
    __syncthreads();
    uint32_t mx = 0;
    for (uint32_t b = b0 + tid; b < b1; b += ORDER_THREADS) {
        const uint32_t len = start[b + 1] - start[b];
        mx = max(mx, len);
        atomicAdd(&base[min(len, ORDER_CAP)], 1u);
    }
    atomicMax(&longest, mx);
    __syncthreads();
    if (tid == 0) {
        if (longest) atomicMax(max_run, longest);
        uint32_t sum = 0;
        for (uint32_t i = 0; i < ORDER_BINS; i++) {
            const uint32_t n = base[i];
            base[i] = sum;
            sum += n;
        }
    }
    for (uint32_t t0 = b0; t0 < b1; t0 += ORDER_THREADS) {
        for (uint32_t i = tid; i < ORDER_WAVES * ORDER_BINS; i += ORDER_THREADS) (&wave_cnt[0][0])[i] = 0;
        __syncthreads();  // also orders the scan of `base` before the first tile
        const uint32_t b = t0 + tid;
        const bool live = b < b1;
        const uint32_t bin = live ? min(start[b + 1] - start[b], ORDER_CAP) : 0u;
        // the lanes of this wave with the same length: one ballot per bin bit
        uint64_t same = __ballot(live);
#pragma unroll
        for (uint32_t k = 0; k < ORDER_BIN_BITS; k++) {
            const uint64_t m = __ballot((bin >> k) & 1u);
            same &= ((bin >> k) & 1u) ? m : ~m;
        }
        const uint32_t rank = __popcll(same & ((1ull << lane) - 1));
        if (live && rank == 0) wave_cnt[wave][bin] = __popcll(same);
        __syncthreads();
        for (uint32_t i = tid; i < ORDER_BINS; i += ORDER_THREADS) {
            // counts -> slots: the earlier waves' buckets of this length first
            uint32_t at = base[i];
#pragma unroll
            for (uint32_t w = 0; w < ORDER_WAVES; w++) {
                const uint32_t n = wave_cnt[w][i];
                wave_cnt[w][i] = at;
                at += n;
            }
            base[i] = at;
        }
        __syncthreads();
        if (live) order[b0 + wave_cnt[wave][bin] + rank] = b;
        __syncthreads();
    }
}

static bool msm_debug() {
    static const bool d = getenv("EON_MSM_DEBUG") != nullptr;
    return d;
}

// digits + radix sort + bucket starts + piece offsets of one batch into `out`; `wk` supplies the
// unsorted pairs, the sort / scan scratch and the count read-back slots
Status batch_sort(eon_ctx* ctx, const MsmLayout& L, uint64_t n, uint64_t ld, Batch& bt, MsmWork& wk,
                  SortedBufs& out, hipStream_t st, hipEvent_t sorted_ev) {
    bt.c = L.c;
    bt.W = bt.w_act ? std::min(bt.w_act, L.W) : L.W;
    bt.B = 1u << (bt.c - 1);
    bt.groups = L.precomputed ? bt.cols : bt.cols * bt.W;
    bt.nb = bt.groups * bt.B;
    bt.E = n * bt.W * bt.cols;
    if (bt.E > RADIX_SORT_MAX_PAIRS) return Status::err(EON_E_SHAPE, "MSM batch too large for 32-bit pair indices");
    // keys are (group << c) | (|digit| - 1); only the low c bits are sorted
    if (((uint64_t)bt.groups << bt.c) > 0xFFFFFFFFull)
        return Status::err(EON_E_SHAPE, "too many MSM groups for 32-bit digit keys");
    bt.key_bits = bt.c;
    const uint64_t E = bt.E;
    const uint32_t nb = bt.nb;

    EON_HIP(ctx_ensure(ctx, wk.keys, E * 4));
    EON_HIP(ctx_ensure(ctx, wk.vals, E * 4));
    EON_HIP(ctx_ensure(ctx, out.keys2, E * 4));
    EON_HIP(ctx_ensure(ctx, out.vals2, E * 4));
    EON_HIP(ctx_ensure(ctx, out.start, (nb + 1) * 4ull));
    EON_HIP(ctx_ensure(ctx, out.piece_off, (nb + 1) * 4ull));
    bt.sort_bytes = radix_sort_temp_bytes(E, bt.key_bits);
    bt.scan_bytes = exclusive_scan_temp_bytes(nb + 1);
    EON_HIP(ctx_ensure(ctx, wk.temp, std::max(bt.sort_bytes, bt.scan_bytes)));
    bt.log_chunk = LOG_CHUNK_MIN;
    while (bt.log_chunk < LOG_CHUNK_MAX && (E >> (bt.log_chunk + 1)) >= (1ull << PIECE_THREADS_LOG)) bt.log_chunk++;
    // few buckets for many pairs (a bucket would collect more than ~8 pieces): longer chunks while
    // the piece sums keep 2^18 threads (4 waves per SIMD)
    while (bt.log_chunk < LOG_CHUNK_MAX && (E >> bt.log_chunk) > 8ull * nb && (E >> (bt.log_chunk + 1)) >= (1ull << 18))
        bt.log_chunk++;
    bt.max_pieces = (E >> bt.log_chunk) + nb + 1;  // >= the real piece count
    if (!wk.host_counts) EON_HIP(hipHostMalloc(reinterpret_cast<void**>(&wk.host_counts), 64));

    Profiler* prof = &ctx->prof;
    uint32_t* hist = radix_sort_histograms(wk.temp.p, E);
    EON_HIP(hipMemsetAsync(hist, 0, RADIX_SORT_MAX_PASSES * 256 * 4, st));
    const uint32_t tile_cols = bt.cols >= DIGIT_COLS ? DIGIT_COLS : (bt.cols >= 2 ? 2 : 1);
    // four rows per thread (16-byte stores) when n allows it, k_msm_digits otherwise: 6.2 vs 10.4 ms
    // of digits per prove (round 4, profiles/r04/s19)
    const bool quad = (n & 3) == 0;
    const uint32_t tile_rows = (quad ? 1024 : 256) / tile_cols;
    const uint32_t grid_y = (bt.cols + tile_cols - 1) / tile_cols;
    const uint64_t tiles = (n + tile_rows - 1) / tile_rows;
    const uint32_t grid_x = (uint32_t)std::min<uint64_t>(tiles, std::max<uint32_t>(1, DIGIT_BLOCKS / grid_y));
    // the first sort pass fused with the digits (DigitSource): fixed-base tables, c = 16, all 16
    // windows, whole 1024-row tiles, two passes
    const bool fused = L.precomputed && bt.c == 16 && bt.W == 16 && L.W == 16 && n % sortpass::SORT_THREADS == 0 &&
                       radix_sort_passes(bt.key_bits).passes == 2;
    if (fused) {
        EON_HIP(ctx_ensure(ctx, wk.canon, n * bt.cols * sizeof(Fr)));
        prof->begin("k_msm_digit_hist", n * bt.cols * 64, st);
        hipLaunchKernelGGL(k_msm_digits4<false>, dim3(grid_x, grid_y), dim3(256), 0, st, bt.scalars, n, ld, bt.cols,
                           bt.c, bt.W, L.W, 1u, tile_cols, nullptr, nullptr, radix_sort_passes(bt.key_bits), hist,
                           wk.canon.as<Fr>());
        prof->end(st);
        EON_HIP(hipGetLastError());
        EON_HIP(radix_sort_prepare(wk.temp.p, E, bt.key_bits, st));
        const RadixPassArgs a0 = radix_sort_pass_args(wk.temp.p, E, bt.key_bits, 0);
        // the pass's own traffic: 32 bytes of scalar per 16 pairs read, 8 bytes per pair written
        prof->begin("k_digit_sort_pass", n * bt.cols * 32 + E * 8, st);
        // per call: the attribute is per device (another context may run on another GPU)
        EON_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_digit_sort_pass),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sortpass::SORT_LDS));
        const DigitSource src{wk.canon.as<Fr>(), n, (uint32_t)(n / sortpass::SORT_THREADS), L.W};
        hipLaunchKernelGGL(k_digit_sort_pass, dim3(a0.tiles), dim3(sortpass::SORT_THREADS), sortpass::SORT_LDS, st, src,
                           wk.keys.as<uint32_t>(), wk.vals.as<uint32_t>(), (uint32_t)E, a0.shift, a0.base, a0.status,
                           a0.tile_ctr);
        prof->end(st);
        EON_HIP(hipGetLastError());
        prof->begin("radix_sort_pairs", E * 16, st);  // the second pass
        EON_HIP(radix_sort_tail(wk.temp.p, wk.keys.as<uint32_t>(), wk.vals.as<uint32_t>(), out.keys2.as<uint32_t>(),
                                out.vals2.as<uint32_t>(), E, bt.key_bits, st));
        prof->end(st);
    } else {
        // the profile record names the kernel that runs (the stage tests assert their route by it)
        prof->begin(quad ? "k_msm_digits4" : "k_msm_digits", n * bt.cols * 32 + E * 8, st);
        hipLaunchKernelGGL(quad ? k_msm_digits4<true> : k_msm_digits, dim3(grid_x, grid_y),
                           dim3(256), 0, st, bt.scalars, n, ld, bt.cols, bt.c, bt.W, L.W, (uint32_t)L.precomputed,
                           tile_cols, wk.keys.as<uint32_t>(), wk.vals.as<uint32_t>(), radix_sort_passes(bt.key_bits),
                           hist, nullptr);
        prof->end(st);
        EON_HIP(hipGetLastError());
        // every pass reads and writes each (key, value) pair once: 16 bytes per pair and pass
        prof->begin("radix_sort_pairs", E * 16 * radix_sort_passes(bt.key_bits).passes, st);
        EON_HIP(radix_sort_pairs(wk.temp.p, wk.keys.as<uint32_t>(), out.keys2.as<uint32_t>(), wk.vals.as<uint32_t>(),
                                 out.vals2.as<uint32_t>(), E, bt.key_bits, st, true));
        prof->end(st);
    }
    prof->begin("k_bucket_start", E * 4, st);
    hipLaunchKernelGGL(k_bucket_start, dim3(blocks_for(E / BS_KEYS + 1, 256)), dim3(256), 0, st,
                       out.keys2.as<uint32_t>(), E, bt.c, bt.groups, nb, out.start.as<uint32_t>());
    prof->end(st);
    // the most pieces one bucket holds fixes the combine levels (no read-backs in the reduction)
    EON_HIP(ctx_ensure(ctx, wk.stat, 16));
    EON_HIP(hipMemsetAsync(wk.stat.p, 0, 16, st));
    EON_HIP(exclusive_scan_chunk_counts(wk.temp.p, out.start.as<uint32_t>(), nb, bt.log_chunk,
                                        out.piece_off.as<uint32_t>(), wk.stat.as<uint32_t>(), st));
    // column batches: the bucket order of the one-bucket-per-lane piece sums, and the longest run
    // (wk.stat[1]) for the route choice (bucket_lanes_route)
    bt.ordered = bt.groups >= COLUMN_BATCH_GROUPS;
    if (bt.ordered) {
        EON_HIP(ctx_ensure(ctx, out.order, (uint64_t)nb * 4));
        prof->begin("k_bucket_order", (uint64_t)nb * 12, st);
        hipLaunchKernelGGL(k_bucket_order, dim3(blocks_for(nb, ORDER_WINDOW)), dim3(ORDER_THREADS), 0, st,
                           out.start.as<uint32_t>(), nb, out.order.as<uint32_t>(), wk.stat.as<uint32_t>() + 1);
        prof->end(st);
        EON_HIP(hipGetLastError());
    }
    // the sorted pairs are ready for the piece sums (sorted_ev), ahead of the count read-back
    EON_HIP(hipEventRecord(sorted_ev, st));
    // the reduction's launches are sized by the real counts (12-byte read-back: pieces, nonzero
    // digits, max pieces); batch_counts waits for them
    EON_HIP(hipMemcpyAsync(wk.host_counts, out.piece_off.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, st));
    EON_HIP(hipMemcpyAsync(wk.host_counts + 1, out.start.as<uint32_t>() + nb, 4, hipMemcpyDeviceToHost, st));
    EON_HIP(hipMemcpyAsync(wk.host_counts + 3, wk.stat.p, 8, hipMemcpyDeviceToHost, st));  // + the longest run
    if (!wk.counts_ev) EON_HIP(hipEventCreateWithFlags(&wk.counts_ev, hipEventDisableTiming));
    EON_HIP(hipEventRecord(wk.counts_ev, st));
    bt.counted = false;
    return Status::ok();
}

// Whether a counted batch's piece sums run one bucket per lane (k_piece_sum_bucket29) instead of one
// chunk per lane: a column batch (it has its bucket order) whose reduction is the one-level
// k_bucket_reduce29 and whose largest bucket is within ORDER_CAP pairs.  The cap is for speed
// alone: a wave runs as long as its longest bucket, k_bucket_order sorts lengths only up to the
// cap, and the chunked route bounds every lane's work whatever the skew.
static bool bucket_lanes_route(const Batch& bt) {
    return bt.ordered && bt.max_run <= ORDER_CAP &&
           (bt.route == Reduce::Deferred || bt.route == Reduce::FusedGroups);
}

// The first moment every input of the batch's plan exists: the route and the piece-sum form are
// decided here and nowhere else (Batch::route, Batch::bucket_lanes).
Status batch_counts(eon_ctx* ctx, const MsmLayout& L, Batch& bt, MsmWork& wk, uint64_t n) {
    EON_HIP(hipEventSynchronize(wk.counts_ev));
    bt.n_pieces = wk.host_counts[0];
    bt.n_pairs = wk.host_counts[1];
    bt.levels = 0;
    for (uint64_t m = wk.host_counts[3]; m > 1; m = (m + PIECE - 1) / PIECE) bt.levels++;
    bt.max_run = wk.host_counts[4];
    if (msm_debug())
        fprintf(stderr, "msm_batch n=%llu cols=%u c=%u W=%u nb=%u E=%llu pairs=%u pieces=%u\n",
                (unsigned long long)n, bt.cols, bt.c, bt.W, bt.nb, (unsigned long long)bt.E, bt.n_pairs,
                bt.n_pieces);
    bt.counted = true;
    bt.route = reduce_route(bt, L);
    bt.bucket_lanes = bucket_lanes_route(bt);
    if (bt.prof_rec < ctx->prof.recs.size()) {  // k_piece_sum was launched before the counts
        ctx->prof.recs[bt.prof_rec].alg_mulmods = (uint64_t)bt.n_pairs * 10;
        ctx->prof.recs[bt.prof_rec].design_bytes = (uint64_t)bt.n_pairs * 72 + (uint64_t)bt.n_pieces * 144;
        bt.prof_rec = SIZE_MAX;
    }
    return Status::ok();
}

// A single MSM digitises only the windows its largest scalar reaches (the signed recoding carries
// at most one bit past it): scalars < 2^64, as in kzg/benches, need 5 of 16 windows of 16 bits.
// One OR-reduction over the scalars and a 32-byte read-back.
Status active_windows(eon_ctx* ctx, const MsmLayout& L, const Fr* scalars, uint64_t n, uint32_t& w_act) {
    constexpr size_t or_bytes = SCALAR_OR_COPIES * 8 * 4;
    EON_HIP(ctx->msm.stat.ensure(std::max<size_t>(64, or_bytes)));
    EON_HIP(hipMemsetAsync(ctx->msm.stat.p, 0, or_bytes, ctx->stream));
    const unsigned blocks = (unsigned)std::min<uint64_t>(blocks_for(n, 256), 4096);
    hipLaunchKernelGGL(k_scalar_or, dim3(blocks), dim3(256), 0, ctx->stream, scalars, n,
                       ctx->msm.stat.as<uint32_t>());
    EON_HIP(hipGetLastError());
    if (!ctx->msm.or_host) EON_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->msm.or_host), or_bytes));
    EON_HIP(hipMemcpyAsync(ctx->msm.or_host, ctx->msm.stat.p, or_bytes, hipMemcpyDeviceToHost, ctx->stream));
    EON_HIP(hipStreamSynchronize(ctx->stream));
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < SCALAR_OR_COPIES; k++)
        for (int j = 0; j < 8; j++) h[j] |= ctx->msm.or_host[k * 8 + j];
    uint32_t bits = 0;
    for (int j = 7; j >= 0 && !bits; j--)
        if (h[j]) bits = 32 * j + 32 - __builtin_clz(h[j]);
    w_act = std::max<uint32_t>(1, std::min<uint32_t>(L.W, (bits + 1 + L.c - 1) / L.c));
    return Status::ok();
}

}  // namespace eon
