// What the MSM pipeline's stages share (msm.hip describes the pipeline and names each stage's
// file): the constants, a batch and its plan, and the stage functions.  Internal to the msm*.hip
// files; the rest of the library sees msm.h.
#pragma once
#include <utility>
#include <vector>

#include "context.h"
#include "ec.h"
#include "ec29.h"
#include "msm.h"

namespace eon {

// sorted pairs per k_piece_sum thread: 2^log_chunk, sized so a batch launches ~2^20 threads
// (>= 4 waves on every SIMD) within [2^4, 2^7]
constexpr uint32_t LOG_CHUNK_MIN = 4, LOG_CHUNK_MAX = 7;
// a batch's chunks grow while its piece sums keep >= 2^PIECE_THREADS_LOG threads
constexpr uint32_t PIECE_THREADS_LOG = 20;
constexpr uint32_t PIECE = 32;   // partials per combine step
// buckets per reduction segment: a lane of the first reduction level walks SEG buckets, the group
// finish combines B / SEG segments per group.  B = 2^(c - 1) >= SEG for every bases object: its
// window size is checked to be 4 <= c <= 20 where it is set (bases_create, bases_alloc_table)
constexpr uint32_t LOG_SEG = 3, SEG = 1u << LOG_SEG;
constexpr uint32_t MSM_C_MIN = 4, MSM_C_MAX = 20;
// A batch with at least this many groups is a column batch: it gets its bucket order at sort time
// (Batch::ordered) and its reduction ends in a group finish; below it (a single MSM, the quotient
// chunks) latency, not additions, sets the time and the reduction ends in LDS trees.
constexpr uint32_t COLUMN_BATCH_GROUPS = 64;
constexpr uint32_t TREE = 256;  // points per tree-reduction block
constexpr uint32_t FINISH_THREADS = 256;  // threads per group of k_group_finish / k_group_finish29

// k_bucket_order: bucket indices per sorting window; run lengths above ORDER_CAP share the last bin
constexpr uint32_t ORDER_WINDOW = 1u << 15;
constexpr uint32_t ORDER_BIN_BITS = 10;
constexpr uint32_t ORDER_BINS = 1u << ORDER_BIN_BITS, ORDER_CAP = ORDER_BINS - 1;

// bucket index b' of a sorted key (nb for the zero-digit sentinel)
__device__ __forceinline__ uint32_t bucket_of(uint32_t key, uint32_t c, uint32_t groups, uint32_t nb) {
    return key == 0xFFFFFFFFu ? nb : (key & ((1u << (c - 1)) - 1)) * groups + (key >> c);
}

static inline unsigned blocks_for(uint64_t n, unsigned bs) { return (unsigned)((n + bs - 1) / bs); }

// The way a counted batch's pieces become one point per group (batch_reduce): the Fused routes and
// Sums29 read k_piece_sum29's raw radix-2^29 pieces, the Combine routes their radix-2^32 conversion
// (k_raw29_to_xyzz, batch_pieces); the Groups routes and Deferred end in a group finish, the
// Segments routes and Sums29 in LDS trees.
enum class Reduce { Deferred, FusedGroups, FusedSegments, Sums29, CombineGroups, CombineSegments };

// One batch of `cols` MSMs of length n over bases[0..n): MSM j uses scalars[i * ld + j].  A batch
// runs in three steps on one stream with its own workspace, so that consecutive batches on two
// streams overlap the memory-bound digit sort of one with the VALU-bound piece sums of the other:
//   batch_sort    digits, radix sort, bucket starts, piece offsets, bucket order; enqueues the
//                 read-back of the pair / piece counts
//   batch_counts  waits for the counts and decides the batch's plan from them
//   batch_pieces  k_piece_sum (asynchronous)
//   batch_reduce  combine levels, bucket sums, weighted bucket reduction (no read-backs);
//                 leaves one XYZZ point per column at `out`
struct Batch {
    const Fr* scalars = nullptr;
    uint32_t cols = 0, col0 = 0;
    G1Xyzz* out = nullptr;
    uint32_t c = 0, W = 0, B = 0, groups = 0, nb = 0, key_bits = 0, log_chunk = 0;
    uint64_t E = 0, max_pieces = 0;
    size_t sort_bytes = 0, scan_bytes = 0;
    uint32_t n_pieces = 0, n_pairs = 0;
    uint32_t levels = 0;  // PIECE-way combine levels until every bucket holds <= 1 partial
    bool counted = false;  // n_pieces / n_pairs / levels read back and the plan decided (batch_counts)
    size_t prof_rec = SIZE_MAX;  // the k_piece_sum profiler record to complete with the counts
    uint32_t w_act = 0;   // windows that can hold a nonzero digit (0: all of the layout's)
    // the sorted buffers hold the batch's bucket order (k_bucket_order): a column batch.  An ordered
    // batch is counted before its piece sums (batch_pieces refuses it otherwise), since whether they
    // run one bucket per lane depends on the counts.
    bool ordered = false;
    uint32_t max_run = 0;   // ordered and counted: the pairs of the batch's largest bucket
    // The plan, decided once by batch_counts and read by batch_pieces, batch_reduce and the
    // diagnostics.  It depends on the batch's counts and on the layout's c and `precomputed` alone,
    // so a prepared handle's stored plan holds for every bases object msm_run_prepared accepts: that
    // function rejects bases of another c or `precomputed`.
    Reduce route = Reduce::CombineSegments;
    bool bucket_lanes = false;  // the piece sums run one bucket per lane (k_piece_sum_bucket29)
};

struct SortedRef {
    const uint32_t *keys, *vals, *start, *piece_off;
    const uint32_t* order;  // meaningful for an ordered batch (Batch::ordered)
};

// Layout of a batched column MSM of n-row columns against bases with this window layout: the
// window size, window count and columns per batch (<= 2^28 digit pairs per batch).
struct MsmLayout {
    uint32_t c = 0, W = 0;
    bool precomputed = false;
    uint64_t cpb = 1;
};

// Deferred group finish: the batches of one call leave their first-level segment sums (T, U of
// k_bucket_reduce29) in call-wide arrays, row = the group's output index, and ONE k_group_finish
// launch over every row runs after the last batch.  Per batch, that finish was 120 groups x 256
// threads -- under one wave per SIMD, a chain of ~75 dependent additions (1.1 ms per batch,
// latency-bound); over the whole call (1312 or 2624 groups) it is throughput-bound.
// Fixed-base layouts have the arrays (prepare_deferred), the others leave T null.
struct DeferredFinish {
    G1Raw29* T = nullptr;
    G1Raw29* U = nullptr;
    G1Xyzz* out_base = nullptr;  // row r's result goes to out_base[r]
    uint32_t nseg = 0;           // B / SEG segments per group
    std::vector<std::pair<uint64_t, uint64_t>> rows;  // deferred [row0, row0 + n)
};

// msm_digits.hip
// digits + radix sort + bucket starts + piece offsets (+ bucket order) of one batch into `out`; `wk`
// supplies the unsorted pairs, the sort / scan scratch and the count read-back slots
Status batch_sort(eon_ctx* ctx, const MsmLayout& L, uint64_t n, uint64_t ld, Batch& bt, MsmWork& wk,
                  SortedBufs& out, hipStream_t st, hipEvent_t sorted_ev);
// waits for batch_sort's read-back and stores the batch's counts and plan
Status batch_counts(eon_ctx* ctx, const MsmLayout& L, Batch& bt, MsmWork& wk, uint64_t n);
// the windows a single MSM's largest scalar reaches (synchronises the context stream)
Status active_windows(eon_ctx* ctx, const MsmLayout& L, const Fr* scalars, uint64_t n, uint32_t& w_act);

// msm_pieces.hip
// piece sums of one sorted batch over the 29-form bases `pts29` (asynchronous); wk supplies the
// piece buffers
Status batch_pieces(eon_ctx* ctx, const MsmLayout& L, const G1Affine* pts29, Batch& bt, const SortedRef& sr,
                    MsmWork& wk, hipStream_t st);
Status piece_merge(eon_ctx* ctx, const Batch& bt, const SortedRef& sr, MsmWork& wk, hipStream_t st);

// msm_reduce.hip
Reduce reduce_route(const Batch& bt, const MsmLayout& L);
Status prepare_deferred(eon_ctx* ctx, const MsmLayout& L, uint64_t rows, G1Xyzz* out_base, DeferredFinish& df);
Status batch_reduce(eon_ctx* ctx, const MsmLayout& L, const Batch& bt, const SortedRef& sr, MsmWork& wk,
                    hipStream_t st, DeferredFinish& df);
Status run_deferred_finish(eon_ctx* ctx, DeferredFinish& df, hipStream_t st);

// msm_bases.hip
uint32_t choose_c(uint64_t n, bool precomputed);
uint64_t bases_len(const eon_msm_bases* b);
// the affine points the piece sums read, 29-Montgomery form: the window table or the plain bases
const G1Affine* bases_pieces29(const eon_msm_bases* b);

}  // namespace eon
