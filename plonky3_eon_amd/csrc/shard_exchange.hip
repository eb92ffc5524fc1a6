// Column-sharded prove of a generic AIR: the partition of columns and quotient-domain
// rows over the ranks, and the two copies around the one all_to_all that turns "every row of my
// columns" into "every column of my rows".
//
// Partition (the one definition: the driver, the kernels below and the Python twin in
// distributed.py all come here).  Columns: rank g owns [c0(g), c0(g) + wl(g)), contiguous, in rank
// order, the first W mod world ranks one column wider; wmax = ceil(W / world).  Rows: with
// Q = 2^(log_n + log_qd) and R = ceil(Q / world), rank r evaluates quotient rows [r R, min(Q, (r+1) R))
// (possibly none).  Its WINDOW is the R + S rows (r R + j) mod Q, j < R + S, S = 2^log_qd the
// distance to a row's "next" row: the local row of window row t is t, its next row t + S.
//
//   eon_shard_pack_rows_dev    the rank's LDE (Q x wl, row-major) -> `world` send blocks of
//                              (R + S) x wmax: block h, row j = LDE row (h R + j) mod Q, the
//                              columns past wl zero;
//   all_to_all                 (the caller's) block h to rank h, (R + S) wmax 32 bytes each;
//   eon_shard_unpack_cols_dev  the `world` received blocks (block g = rank g's columns of this
//                              rank's window) -> the (R + S) x W row-major window, columns
//                              [c0(g), c0(g) + wl(g)) from block g.
//
// Both kernels are copies: one wave per row segment (a block's row), consecutive lanes on
// consecutive 16-byte halves of its elements, one division per segment (which block, which row).
#include <algorithm>

#include "context.h"

using namespace eon;

namespace {

constexpr uint32_t SEG_LANES = 64, SEG_PER_BLOCK = 4;  // a 256-thread block copies four row segments

struct ColRange {
    uint32_t c0, wl;
};
// balanced contiguous split of `width` columns: base = width / world, the first extra = width %
// world ranks one more
__host__ __device__ inline ColRange col_range(uint32_t base, uint32_t extra, uint32_t g) {
    return {g * base + (g < extra ? g : extra), base + (g < extra ? 1u : 0u)};
}

// send[(h win + j) wmax + c] = lde[((h r + j) mod q) wl + c], c < wl; zero for wl <= c < wmax
__global__ void __launch_bounds__(SEG_LANES * SEG_PER_BLOCK)
    k_shard_pack_rows(const uint4* __restrict__ lde, uint64_t q, uint32_t wl, uint32_t wmax, uint64_t r, uint64_t win,
                      uint64_t n_seg, uint4* __restrict__ send) {
    const uint64_t seg = (uint64_t)blockIdx.x * SEG_PER_BLOCK + threadIdx.y;
    if (seg >= n_seg) return;
    const uint64_t h = seg / win, j = seg - h * win;
    const uint4* const src = lde + ((h * r + j) % q) * (2ull * wl);
    uint4* const dst = send + seg * (2ull * wmax);
    const uint32_t halves = 2 * wl, padded = 2 * wmax;
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < halves; i += SEG_LANES) dst[i] = src[i];
    for (uint32_t i = halves + threadIdx.x; i < padded; i += SEG_LANES) dst[i] = make_uint4(0, 0, 0, 0);
}

// window[j width + c0(g) + k] = recv[(g win + j) wmax + k], k < wl(g)
__global__ void __launch_bounds__(SEG_LANES * SEG_PER_BLOCK)
    k_shard_unpack_cols(const uint4* __restrict__ recv, uint64_t win, uint32_t width, uint32_t wmax, uint32_t base,
                        uint32_t extra, uint64_t n_seg, uint4* __restrict__ window) {
    const uint64_t seg = (uint64_t)blockIdx.x * SEG_PER_BLOCK + threadIdx.y;
    if (seg >= n_seg) return;
    const uint64_t g = seg / win, j = seg - g * win;
    const ColRange cr = col_range(base, extra, (uint32_t)g);
    const uint4* const src = recv + seg * (2ull * wmax);
    uint4* const dst = window + (j * width + cr.c0) * 2ull;
    const uint32_t halves = 2 * cr.wl;
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < halves; i += SEG_LANES) dst[i] = src[i];
}

struct Shape {
    uint64_t r, win, n_seg;
    uint32_t wmax, base, extra;
};
// what both entry points check alike; the segment count must fit a launch (one block per four)
Status shard_shape(uint64_t q_rows, uint32_t width, uint32_t world, uint64_t next_step, Shape* out) {
    if (world == 0 || width == 0 || world > width)
        return Status::err(EON_E_ARG, "column sharding: more ranks than columns (or none of either)");
    if (q_rows == 0 || (q_rows & (q_rows - 1)) || q_rows > (1ull << 28))
        return Status::err(EON_E_SHAPE, "the quotient domain must be a power of two <= 2^28 rows");
    if (next_step == 0 || (next_step & (next_step - 1)) || next_step > q_rows)
        return Status::err(EON_E_SHAPE, "next_step must be a power of two <= the quotient domain");
    Shape s;
    s.r = (q_rows + world - 1) / world;
    s.win = s.r + next_step;
    s.n_seg = s.win * world;
    s.wmax = (width + world - 1) / world;
    s.base = width / world;
    s.extra = width % world;
    if ((s.n_seg + SEG_PER_BLOCK - 1) / SEG_PER_BLOCK > 0x7fffffffull)
        return Status::err(EON_E_SHAPE, "too many row segments for one launch");
    *out = s;
    return Status::ok();
}

template <class Body>
int with_ctx(eon_ctx* ctx, Body body) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    const Status s = body();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

}  // namespace

extern "C" {

int eon_shard_column_range(uint32_t width, uint32_t world, uint32_t rank, uint32_t* c0, uint32_t* wl) {
    if (!c0 || !wl || world == 0 || rank >= world || world > width) return EON_E_ARG;
    const ColRange cr = col_range(width / world, width % world, rank);
    *c0 = cr.c0;
    *wl = cr.wl;
    return EON_OK;
}

int eon_shard_row_range(uint64_t q_rows, uint32_t world, uint32_t rank, uint64_t* row0, uint64_t* n_rows) {
    if (!row0 || !n_rows || world == 0 || rank >= world || q_rows == 0) return EON_E_ARG;
    const uint64_t r = (q_rows + world - 1) / world;
    const uint64_t lo = std::min<uint64_t>(q_rows, (uint64_t)rank * r);
    const uint64_t hi = std::min<uint64_t>(q_rows, (uint64_t)(rank + 1) * r);
    *row0 = lo;
    *n_rows = hi - lo;
    return EON_OK;
}

int eon_shard_pack_rows_dev(eon_ctx* ctx, const eon_fr* lde, uint64_t q_rows, uint32_t width, uint32_t world,
                            uint32_t rank, uint64_t next_step, eon_fr* send) {
    if (!ctx) return EON_E_ARG;
    return with_ctx(ctx, [&]() -> Status {
        if (!lde || !send) return Status::err(EON_E_ARG, "null pointer");
        Shape s;
        EON_TRY(shard_shape(q_rows, width, world, next_step, &s));
        if (rank >= world) return Status::err(EON_E_ARG, "rank >= world");
        const ColRange cr = col_range(s.base, s.extra, rank);
        // read: every segment's wl elements; written: its wmax
        ctx->prof.begin("k_shard_pack_rows", s.n_seg * ((uint64_t)cr.wl + s.wmax) * sizeof(Fr), ctx->stream);
        hipLaunchKernelGGL(k_shard_pack_rows, dim3((unsigned)((s.n_seg + SEG_PER_BLOCK - 1) / SEG_PER_BLOCK)),
                           dim3(SEG_LANES, SEG_PER_BLOCK), 0, ctx->stream, reinterpret_cast<const uint4*>(lde), q_rows,
                           cr.wl, s.wmax, s.r, s.win, s.n_seg, reinterpret_cast<uint4*>(send));
        ctx->prof.end(ctx->stream);
        EON_HIP(hipGetLastError());
        return Status::ok();
    });
}

int eon_shard_unpack_cols_dev(eon_ctx* ctx, const eon_fr* recv, uint64_t q_rows, uint32_t width, uint32_t world,
                              uint64_t next_step, eon_fr* window) {
    if (!ctx) return EON_E_ARG;
    return with_ctx(ctx, [&]() -> Status {
        if (!recv || !window) return Status::err(EON_E_ARG, "null pointer");
        Shape s;
        EON_TRY(shard_shape(q_rows, width, world, next_step, &s));
        ctx->prof.begin("k_shard_unpack_cols", 2 * s.win * width * sizeof(Fr), ctx->stream);
        hipLaunchKernelGGL(k_shard_unpack_cols, dim3((unsigned)((s.n_seg + SEG_PER_BLOCK - 1) / SEG_PER_BLOCK)),
                           dim3(SEG_LANES, SEG_PER_BLOCK), 0, ctx->stream, reinterpret_cast<const uint4*>(recv), s.win,
                           width, s.wmax, s.base, s.extra, s.n_seg, reinterpret_cast<uint4*>(window));
        ctx->prof.end(ctx->stream);
        EON_HIP(hipGetLastError());
        return Status::ok();
    });
}

}  // extern "C"
