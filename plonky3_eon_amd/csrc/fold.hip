// gamma-fold of a row-major matrix: out[i] = scale * sum_j gamma^j mat[i][j], the folded polynomial
// F = sum_j gamma^j f_j of the batched KZG opening (one witness per matrix and point instead of one
// per column).
//
// With j = 64 t + l:   sum_j gamma^j x_j = sum_{l < 64} gamma^l  sum_t (gamma^64)^t x_(64 t + l).
// A wave takes a row.  Lane l walks the row's 64-column tiles top-down with the Horner step
// r <- x + G r, G = gamma^64 wave-uniform (its Shoup pair in SGPRs, mul29_shoup_u: 143 multiply-adds
// per element, no Montgomery multipliers), so adjacent lanes read adjacent 32-byte elements and a
// tile is one contiguous 2 KiB read.  The lane's total is then multiplied once by its own gamma^l
// (a Shoup pair in VGPRs, from a 64-entry table k_fold_powers makes on the device per call) and
// the 64 terms are summed across the wave.  The elements are in the ABI's Montgomery form x 2^256;
// a Shoup product multiplies by the PLAIN integer gamma^j, which keeps that form, so nothing is
// converted on the way in or out.
//
// Bounds (p < 2^254; normalised = limbs < 2^29):
//   x canonical (< p); mul29_shoup* returns [0, 3p) for any normalised y < 2^261;
//   Horner: r = x + G r < p + 3p = 4p (add29_norm);      term = gamma^l r in [0, 3p);
//   wave sum: three butterfly steps of limb-wise adds (8 terms: limbs < 2^32, value < 24p < 2^261),
//   carry propagation, reduce_top29 (< 2p); three more steps (8 x 2p = 16p), the same (< 2p);
//   scale: a Shoup product (< 3p) and reduce_top29 (< 2p); ONE canon29 per output element.
#include "context.h"
#include "field29.h"

#include <algorithm>

using namespace eon;

namespace {

constexpr uint32_t FOLD_TILE = 64;  // columns per Horner step of a wave = the wave size
constexpr uint32_t FOLD_WPB = 4;    // waves (rows in flight) per block
constexpr uint32_t FOLD_UNR = 4;    // tiles whose loads are issued before their Horner steps
constexpr uint32_t FOLD_MAX_BLOCKS = 256 * 8;

struct FoldArgs {
    F29 g, gq;  // gamma^64 and its Shoup quotient
    F29 s, sq;  // scale, likewise
    uint32_t has_scale;
};

__device__ __forceinline__ Fr ld(const Fr* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    Fr x;
    x.v[0] = a.x; x.v[1] = a.y; x.v[2] = a.z; x.v[3] = a.w;
    x.v[4] = b.x; x.v[5] = b.y; x.v[6] = b.z; x.v[7] = b.w;
    return x;
}

__device__ __forceinline__ void st(Fr* p, const Fr& x) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    q[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
}

// carry propagation of limbs < 2^32 whose value is < 2^261
__device__ __forceinline__ F29 norm29_wide(const F29& a) {
    F29 r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint64_t t = (uint64_t)a.l[i] + c;
        r.l[i] = i < 8 ? (uint32_t)t & M29 : (uint32_t)t;
        c = t >> 29;
    }
    return r;
}

// a + (the same value of lane ^ mask), limb by limb without carries
__device__ __forceinline__ F29 xor_add29(const F29& a, int mask) {
    F29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = a.l[i] + (uint32_t)__shfl_xor((int)a.l[i], mask, 64);
    return r;
}

// tab[i * 64 + l] = limb i of gamma^l (i < 9) and of its Shoup quotient (9 <= i < 18), l < 64
__global__ void k_fold_powers(Fr gamma, uint32_t* tab) {
    const uint32_t l = threadIdx.x;
    if (l >= FOLD_TILE) return;
    // gamma^l 2^261 mod p (the Montgomery form of 32 gamma^l) -> plain gamma^l and its quotient
    const Fr t = mul(pow_u64(gamma, l), from_u64<FrP>(32));
    F29 w, wq;
    shoup_pair29<FrP>(unpack29(t), w, wq);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        tab[i * FOLD_TILE + l] = w.l[i];
        tab[(9 + i) * FOLD_TILE + l] = wq.l[i];
    }
}

__global__ void __launch_bounds__(FOLD_TILE* FOLD_WPB)
k_fold_columns(const Fr* __restrict__ mat, uint64_t rows, uint32_t width, FoldArgs a,
               const uint32_t* __restrict__ tab, Fr* __restrict__ out) {
    const uint32_t lane = threadIdx.x % FOLD_TILE, wave = threadIdx.x / FOLD_TILE;
    F29 w, wq;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        w.l[i] = tab[i * FOLD_TILE + lane];
        wq.l[i] = tab[(9 + i) * FOLD_TILE + lane];
    }
    const uint32_t tiles = (width + FOLD_TILE - 1) / FOLD_TILE;
    // the row of a wave does not depend on the lane: every lane of a wave makes every trip, so the
    // cross-lane sums below see all 64 lanes
    for (uint64_t row = (uint64_t)blockIdx.x * FOLD_WPB + wave; row < rows; row += (uint64_t)gridDim.x * FOLD_WPB) {
        const Fr* rp = mat + row * width;
        F29 r = unpack29(Fr::zero());
        uint32_t t = tiles;
        while (t >= FOLD_UNR) {
            Fr x[FOLD_UNR];
#pragma unroll
            for (uint32_t k = 0; k < FOLD_UNR; k++) {
                const uint32_t col = (t - 1 - k) * FOLD_TILE + lane;  // only the top tile can be partial
                x[k] = col < width ? ld(rp + col) : Fr::zero();
            }
#pragma unroll
            for (uint32_t k = 0; k < FOLD_UNR; k++)
                r = add29_norm(unpack29(x[k]), mul29_shoup_u<FrP>(r, a.g, a.gq));  // < p + 3p
            t -= FOLD_UNR;
        }
        while (t > 0) {
            const uint32_t col = (t - 1) * FOLD_TILE + lane;
            const Fr x = col < width ? ld(rp + col) : Fr::zero();
            r = add29_norm(unpack29(x), mul29_shoup_u<FrP>(r, a.g, a.gq));
            t--;
        }
        F29 s = mul29_shoup<FrP>(r, w, wq);  // gamma^lane r, < 3p
        s = xor_add29(s, 1);
        s = xor_add29(s, 2);
        s = xor_add29(s, 4);  // 8 terms: limbs < 2^32, value < 24p
        s = reduce_top29<FrP>(norm29_wide(s));  // < 2p
        s = xor_add29(s, 8);
        s = xor_add29(s, 16);
        s = xor_add29(s, 32);  // 8 x 2p = 16p
        s = reduce_top29<FrP>(norm29_wide(s));
        if (a.has_scale) s = reduce_top29<FrP>(mul29_shoup_u<FrP>(s, a.s, a.sq));
        if (lane == 0) st(out + row, pack29<FrP>(canon29<FrP>(s)));
    }
}

Status fold_columns(eon_ctx* ctx, const Fr* mat, uint64_t rows, uint32_t width, const eon_fr* gamma,
                    const eon_fr* scale, Fr* out) {
    if (rows == 0) return Status::ok();
    if (!out) return Status::err(EON_E_ARG, "null argument");
    if (width == 0) {
        EON_HIP(hipMemsetAsync(out, 0, rows * sizeof(Fr), ctx->stream));
        return Status::ok();
    }
    if (!mat || !gamma) return Status::err(EON_E_ARG, "null argument");
    if (rows > UINT64_MAX / sizeof(Fr) / width) return Status::err(EON_E_SHAPE, "matrix size overflows");
    {
        const uintptr_t m0 = reinterpret_cast<uintptr_t>(mat), m1 = m0 + rows * width * sizeof(Fr);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + rows * sizeof(Fr);
        if (o0 < m1 && m0 < o1) return Status::err(EON_E_ARG, "out must not alias mat");
    }
    const Fr g = fr_from_abi(gamma);
    if (!fr_is_canonical(g)) return Status::err(EON_E_ARG, "gamma is not a canonical Fr");
    FoldArgs a{};
    shoup_pair29<FrP>(unpack29(ntt_scale_form(pow_u64(g, FOLD_TILE))), a.g, a.gq);
    if (scale) {
        const Fr s = fr_from_abi(scale);
        if (!fr_is_canonical(s)) return Status::err(EON_E_ARG, "scale is not a canonical Fr");
        shoup_pair29<FrP>(unpack29(ntt_scale_form(s)), a.s, a.sq);
        a.has_scale = 1;
    }
    DevBuf& tab = ctx->tables["fold_powers"];
    EON_HIP(tab.ensure(18 * FOLD_TILE * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_fold_powers, dim3(1), dim3(FOLD_TILE), 0, ctx->stream, g, tab.as<uint32_t>());
    const uint64_t want = (rows + FOLD_WPB - 1) / FOLD_WPB;
    const unsigned grid = (unsigned)std::min<uint64_t>(want, FOLD_MAX_BLOCKS);
    ctx->prof.begin("k_fold_columns", rows * width * 32ull + rows * 32ull, ctx->stream, rows * width);
    hipLaunchKernelGGL(k_fold_columns, dim3(grid), dim3(FOLD_TILE * FOLD_WPB), 0, ctx->stream, mat, rows, width, a,
                       tab.as<uint32_t>(), out);
    ctx->prof.end(ctx->stream);
    EON_HIP(hipGetLastError());
    return Status::ok();
}

}  // namespace

extern "C" int eon_fr_fold_columns_dev(eon_ctx* ctx, const eon_fr* mat, uint64_t rows, uint32_t width,
                                       const eon_fr* gamma, const eon_fr* scale, eon_fr* out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    const Status s = fold_columns(ctx, reinterpret_cast<const Fr*>(mat), rows, width, gamma, scale,
                                  reinterpret_cast<Fr*>(out));
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}
