// KZG opening on device: quotient_and_eval (kzg/src/util.rs:100-111) for every column of a
// row-major coefficient matrix at one point, as KzgPcs::open does per (matrix, point, column)
// (kzg/src/pcs.rs:297-330).
//
// With r_i = sum_{j >= i} c_j z^(j-i) (so r_i = c_i + z * r_(i+1), r_n = 0): f(z) = r_0 and the
// synthetic-division quotient is q_i = r_(i+1), i < n-1.  The recurrence runs as a blocked scan:
//   k_horner_block   per (block of BL rows, column): local suffix Horner total T_b (carry-in 0)
//   k_horner_carry   per column, over blocks top-down: carry_b = T_(b+1) + z^BL * carry_(b+1)
//   k_horner_apply   per (block, column): the local recurrence again from carry_b, writing q
// Two mulmods per coefficient; threads = (n / BL) x width, adjacent threads = adjacent columns.
#include "context.h"
#include "field29.h"
#include "ntt.h"

#include <algorithm>

using namespace eon;

namespace {

constexpr uint32_t BL = 256;  // rows per scan block

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

__global__ void k_horner_block(const Fr* c, uint64_t n, uint32_t width, Fr z, Fr* totals) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblk = (n + BL - 1) / BL;
    if (t >= nblk * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t b = t / width;
    const uint64_t lo = b * BL, hi = lo + BL < n ? lo + BL : n;
    Fr r = Fr::zero();
    for (uint64_t i = hi; i-- > lo;) r = add(ld(c + i * width + col), mul(z, r));
    st(totals + b * width + col, r);
}

// carries[b] = r at the first row above block b (0 for the top block)
__global__ void k_horner_carry(const Fr* totals, uint64_t nblk, uint32_t width, Fr z_bl, Fr* carries,
                               Fr* values) {
    const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= width) return;
    Fr carry = Fr::zero();
    for (uint64_t b = nblk; b-- > 0;) {
        st(carries + b * width + col, carry);
        // r_(lo_b) = T_b + z^(rows in block b) * carry; every block but the top one is full
        carry = add(ld(totals + b * width + col), mul(z_bl, carry));
    }
    st(values + col, carry);  // r_0 = f(z)
}

__global__ void k_horner_apply(const Fr* c, uint64_t n, uint32_t width, Fr z, const Fr* carries,
                               Fr* q) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblk = (n + BL - 1) / BL;
    if (t >= nblk * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t b = t / width;
    const uint64_t lo = b * BL, hi = lo + BL < n ? lo + BL : n;
    Fr r = ld(carries + b * width + col);
    for (uint64_t i = hi; i-- > lo;) {
        if (i < n - 1) st(q + i * width + col, r);  // q_i = r_(i+1)
        r = add(ld(c + i * width + col), mul(z, r));
    }
}

// ---- values only, several points in one pass ------------------------------------------------------
// f(z) = sum_b T_b Z^b with T_b the block totals above and Z = z^BL; the blocks' Horner chain is
// split once more into chunks of CH blocks (P_q = sum over the chunk, then sum_q P_q (Z^CH)^q), so
// no thread walks more than max(BL, CH, n / (BL CH)) steps; one read of the coefficients serves
// every point.
constexpr uint32_t CH = 32;
constexpr uint32_t MAX_PTS = 4;
struct Pts {
    Fr z[MAX_PTS];
};

// the points as Shoup multipliers (plain root z and floor(z 2^261 / p), field29.h mul29_shoup):
// r <- c + z r per coefficient is then 143 multiply-adds with no Montgomery multipliers, the
// running value kept lazy (< 4p) in 29-bit limbs
struct PtsShoup {
    F29 w[MAX_PTS], q[MAX_PTS];
};

__global__ void k_eval_block(const Fr* c, uint64_t n, uint32_t width, PtsShoup zs, uint32_t np, Fr* totals) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblk = (n + BL - 1) / BL;
    if (t >= nblk * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t b = t / width;
    const uint64_t lo = b * BL, hi = lo + BL < n ? lo + BL : n;
    // r[] indexed only by unrolled loops, so it stays in registers (a rolled loop over it kept it in
    // scratch, read and written every coefficient)
    F29 r[MAX_PTS];
#pragma unroll
    for (uint32_t p = 0; p < MAX_PTS; p++) r[p] = unpack29(Fr::zero());
    for (uint64_t i = hi; i-- > lo;) {
        const F29 x = unpack29(ld(c + i * width + col));  // canonical
#pragma unroll
        for (uint32_t p = 0; p < MAX_PTS; p++)
            if (p < np) r[p] = add29_norm(x, mul29_shoup_u<FrP>(r[p], zs.w[p], zs.q[p]));  // < p + 3p; z in SGPRs
    }
#pragma unroll
    for (uint32_t p = 0; p < MAX_PTS; p++)
        if (p < np)
            st(totals + ((uint64_t)p * nblk + b) * width + col, pack29<FrP>(canon29<FrP>(reduce_top29<FrP>(r[p]))));
}

// per (point, chunk of CH blocks, column): P_q = sum_{b in chunk} T_b Z^(b - q CH)
__global__ void k_eval_chunks(const Fr* totals, uint64_t nblk, uint32_t width, Pts zbl, uint32_t np, Fr* part) {
    const uint64_t nq = (nblk + CH - 1) / CH;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)np * nq * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t q = (t / width) % nq;
    const uint32_t p = (uint32_t)(t / (width * nq));
    const uint64_t b0 = q * CH, b1 = b0 + CH < nblk ? b0 + CH : nblk;
    Fr acc = Fr::zero();
    for (uint64_t b = b1; b-- > b0;) acc = add(ld(totals + ((uint64_t)p * nblk + b) * width + col), mul(zbl.z[p], acc));
    st(part + ((uint64_t)p * nq + q) * width + col, acc);
}

// per (point, column): f(z) = sum_q P_q (Z^CH)^q
__global__ void k_eval_final(const Fr* part, uint64_t nq, uint32_t width, Pts zch, uint32_t np, Fr* values) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)np * width) return;
    const uint32_t col = (uint32_t)(t % width), p = (uint32_t)(t / width);
    Fr acc = Fr::zero();
    for (uint64_t q = nq; q-- > 0;) acc = add(ld(part + ((uint64_t)p * nq + q) * width + col), mul(zch.z[p], acc));
    st(values + (uint64_t)p * width + col, acc);
}

// ---- quotients and values, several points in one pass (KzgMmcs::open_batch, kzg/src/mmcs.rs:223-230)
// The blocked scan above for up to MAX_PTS points per read of a coefficient, plain Montgomery
// arithmetic (every stored quotient is canonical as it stands: the MSM digitises it).  One launch
// covers up to LAUNCH_PTS points: a scan block has only n / BL x width threads, so the groups of
// MAX_PTS points are the grid's y dimension and run side by side.
//   k_hornerm_block   per (group, block, column): the group's local totals T_b,
//                     totals[(p nblk + b) width + col]
//   k_hornerm_part    per (point, chunk of CH blocks, column): P_q = sum_{b in chunk} T_b Z^(b - q CH)
//   k_hornerm_chunks  per (point, column), over chunks top-down: the carry into each chunk, f(z)
//   k_hornerm_carry   per (point, chunk, column), over its blocks top-down: the carry into each block
//   k_hornerm_apply   per (group, block, column): the group's recurrences again from their carries,
//                     writing q[i][(p0 + p) width + col] -- the points' quotients side by side in one
//                     (n-1) x (npoints width) matrix, adjacent threads adjacent 32-byte elements
// so the serial walks are BL, CH and n / (BL CH) steps long.
constexpr uint32_t LAUNCH_PTS = 32;
struct PtsL {
    Fr z[LAUNCH_PTS];
};

// np = the launch's points; group g = blockIdx.y holds points [MAX_PTS g, MAX_PTS g + MAX_PTS) of them
__global__ void k_hornerm_block(const Fr* c, uint64_t n, uint32_t width, PtsL zs, uint32_t np, Fr* totals) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblk = (n + BL - 1) / BL;
    if (t >= nblk * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t b = t / width;
    const uint64_t lo = b * BL, hi = lo + BL < n ? lo + BL : n;
    const uint32_t g0 = blockIdx.y * MAX_PTS, ng = np - g0 < MAX_PTS ? np - g0 : MAX_PTS;
    // z[] and r[] indexed only by unrolled loops, so they stay in registers (see k_eval_block)
    Fr z[MAX_PTS], r[MAX_PTS];
#pragma unroll
    for (uint32_t p = 0; p < MAX_PTS; p++) {
        z[p] = zs.z[g0 + (p < ng ? p : 0)];
        r[p] = Fr::zero();
    }
    for (uint64_t i = hi; i-- > lo;) {
        const Fr x = ld(c + i * width + col);
#pragma unroll
        for (uint32_t p = 0; p < MAX_PTS; p++)
            if (p < ng) r[p] = add(x, mul(z[p], r[p]));
    }
#pragma unroll
    for (uint32_t p = 0; p < MAX_PTS; p++)
        if (p < ng) st(totals + ((uint64_t)(g0 + p) * nblk + b) * width + col, r[p]);
}

// point p = blockIdx.y in the three carry kernels
__global__ void k_hornerm_part(const Fr* totals, uint64_t nblk, uint32_t width, PtsL zbl, Fr* part) {
    const uint64_t nq = (nblk + CH - 1) / CH;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq * width) return;
    const uint32_t col = (uint32_t)(t % width), p = blockIdx.y;
    const uint64_t q = t / width;
    const uint64_t b0 = q * CH, b1 = b0 + CH < nblk ? b0 + CH : nblk;
    const Fr z = zbl.z[p];
    Fr acc = Fr::zero();
    for (uint64_t b = b1; b-- > b0;) acc = add(ld(totals + ((uint64_t)p * nblk + b) * width + col), mul(z, acc));
    st(part + ((uint64_t)p * nq + q) * width + col, acc);
}

// ccarry[q] = r at the first row above chunk q (0 for the top chunk); every chunk but the top one
// holds CH full blocks, so r below chunk q = P_q + (Z^CH) ccarry[q]
__global__ void k_hornerm_chunks(const Fr* part, uint64_t nq, uint32_t width, PtsL zch, Fr* ccarry, Fr* values) {
    const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
    if (col >= width) return;
    const Fr z = zch.z[p];
    Fr carry = Fr::zero();
    for (uint64_t q = nq; q-- > 0;) {
        st(ccarry + ((uint64_t)p * nq + q) * width + col, carry);
        carry = add(ld(part + ((uint64_t)p * nq + q) * width + col), mul(z, carry));
    }
    st(values + (uint64_t)p * width + col, carry);  // r_0 = f(z)
}

// carries[b] = r at the first row above block b, walking chunk q's blocks down from ccarry[q]
__global__ void k_hornerm_carry(const Fr* totals, uint64_t nblk, uint32_t width, PtsL zbl, const Fr* ccarry,
                                Fr* carries) {
    const uint64_t nq = (nblk + CH - 1) / CH;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq * width) return;
    const uint32_t col = (uint32_t)(t % width), p = blockIdx.y;
    const uint64_t q = t / width;
    const uint64_t b0 = q * CH, b1 = b0 + CH < nblk ? b0 + CH : nblk;
    const Fr z = zbl.z[p];
    Fr carry = ld(ccarry + ((uint64_t)p * nq + q) * width + col);
    for (uint64_t b = b1; b-- > b0;) {
        st(carries + ((uint64_t)p * nblk + b) * width + col, carry);
        carry = add(ld(totals + ((uint64_t)p * nblk + b) * width + col), mul(z, carry));
    }
}

// qw = npoints * width, the row length of q; qcol0 = p0 * width, the first column of the launch's points
__global__ void k_hornerm_apply(const Fr* c, uint64_t n, uint32_t width, PtsL zs, uint32_t np, const Fr* carries,
                                Fr* q, uint64_t qw, uint64_t qcol0) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblk = (n + BL - 1) / BL;
    if (t >= nblk * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t b = t / width;
    const uint64_t lo = b * BL, hi = lo + BL < n ? lo + BL : n;
    const uint32_t g0 = blockIdx.y * MAX_PTS, ng = np - g0 < MAX_PTS ? np - g0 : MAX_PTS;
    Fr z[MAX_PTS], r[MAX_PTS];
#pragma unroll
    for (uint32_t p = 0; p < MAX_PTS; p++) {
        z[p] = zs.z[g0 + (p < ng ? p : 0)];
        r[p] = p < ng ? ld(carries + ((uint64_t)(g0 + p) * nblk + b) * width + col) : Fr::zero();
    }
    for (uint64_t i = hi; i-- > lo;) {
        const Fr x = ld(c + i * width + col);
        Fr* row = q + i * qw + qcol0 + (uint64_t)g0 * width + col;
#pragma unroll
        for (uint32_t p = 0; p < MAX_PTS; p++)
            if (p < ng) {
                if (i < n - 1) st(row + (uint64_t)p * width, r[p]);  // q_i = r_(i+1)
                r[p] = add(x, mul(z[p], r[p]));
            }
    }
}

}  // namespace

namespace eon {

Status quotient_and_eval_multi(eon_ctx* ctx, const Fr* c, uint64_t rows, uint32_t width, const Fr* points,
                               uint32_t npoints, Fr* quotients, Fr* values) {
    if ((npoints && !points) || (width && npoints && !values)) return Status::err(EON_E_ARG, "null argument");
    if (width == 0 || npoints == 0) return Status::ok();
    for (uint32_t p = 0; p < npoints; p++)
        if (!fr_is_canonical(points[p])) return Status::err(EON_E_ARG, "point is not a canonical Fr");
    if (rows == 0) {  // empty column: (empty quotient, 0) (kzg/src/util.rs:101-103)
        EON_HIP(hipMemsetAsync(values, 0, (size_t)npoints * width * sizeof(Fr), ctx->stream));
        return Status::ok();
    }
    if (!c) return Status::err(EON_E_ARG, "null argument");
    const uint64_t nblk = (rows + BL - 1) / BL, nq = (nblk + CH - 1) / CH;
    if (nblk * width > (uint64_t)0x7fffffff * 128) return Status::err(EON_E_SHAPE, "matrix too large for one launch");
    // points per launch: LAUNCH_PTS, fewer (whole groups of MAX_PTS) where their scan scratch --
    // totals, carries and the chunks' two arrays per point -- would pass 256 MiB
    const uint64_t point_bytes = 2 * (nblk + nq) * width * sizeof(Fr);
    const uint32_t lp = (uint32_t)std::min<uint64_t>(
        LAUNCH_PTS, std::max<uint64_t>(1, (256ull << 20) / (MAX_PTS * point_bytes)) * MAX_PTS);
    EON_HIP(ctx->kzg_tmp.ensure((uint64_t)std::min(lp, (npoints + MAX_PTS - 1) / MAX_PTS * MAX_PTS) * point_bytes));
    const unsigned grid = (unsigned)((nblk * width + 127) / 128), cgrid = (unsigned)((nq * width + 127) / 128);
    const bool want_q = quotients && rows > 1;
    for (uint32_t p0 = 0; p0 < npoints; p0 += lp) {
        const uint32_t np = std::min<uint32_t>(lp, npoints - p0), groups = (np + MAX_PTS - 1) / MAX_PTS;
        Fr* totals = ctx->kzg_tmp.as<Fr>();
        Fr* carries = totals + (uint64_t)np * nblk * width;
        Fr* part = carries + (uint64_t)np * nblk * width;
        Fr* ccarry = part + (uint64_t)np * nq * width;
        PtsL zs{}, zbl{}, zch{};
        for (uint32_t p = 0; p < np; p++) {
            zs.z[p] = points[p0 + p];
            zbl.z[p] = pow_u64(zs.z[p], BL);
            zch.z[p] = pow_u64(zbl.z[p], CH);
        }
        ctx->prof.begin("k_hornerm_block", rows * width * 32ull * groups, ctx->stream);
        hipLaunchKernelGGL(k_hornerm_block, dim3(grid, groups), dim3(128), 0, ctx->stream, c, rows, width, zs, np,
                           totals);
        ctx->prof.end(ctx->stream);
        hipLaunchKernelGGL(k_hornerm_part, dim3(cgrid, np), dim3(128), 0, ctx->stream, totals, nblk, width, zbl, part);
        hipLaunchKernelGGL(k_hornerm_chunks, dim3((width + 63) / 64, np), dim3(64), 0, ctx->stream, part, nq, width,
                           zch, ccarry, values + (uint64_t)p0 * width);
        if (want_q) {
            hipLaunchKernelGGL(k_hornerm_carry, dim3(cgrid, np), dim3(128), 0, ctx->stream, totals, nblk, width, zbl,
                               ccarry, carries);
            // algorithmic bytes: the coefficients read once per group, np quotients written
            ctx->prof.begin("k_hornerm_apply", rows * width * 32ull * (groups + np), ctx->stream);
            hipLaunchKernelGGL(k_hornerm_apply, dim3(grid, groups), dim3(128), 0, ctx->stream, c, rows, width, zs, np,
                               carries, quotients, (uint64_t)npoints * width, (uint64_t)p0 * width);
            ctx->prof.end(ctx->stream);
        }
        EON_HIP(hipGetLastError());
    }
    return Status::ok();
}

}  // namespace eon

extern "C" {

int eon_quotient_and_eval_columns_multi_dev(eon_ctx* ctx, const eon_fr* coeffs, uint64_t rows, uint32_t width,
                                            const eon_fr* points, uint32_t npoints, eon_fr* quotients,
                                            eon_fr* values) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (npoints && !points) return Status::err(EON_E_ARG, "null argument");
        std::vector<Fr> zs(npoints);
        for (uint32_t p = 0; p < npoints; p++) zs[p] = fr_from_abi(points + p);
        return quotient_and_eval_multi(ctx, reinterpret_cast<const Fr*>(coeffs), rows, width, zs.data(), npoints,
                                       reinterpret_cast<Fr*>(quotients), reinterpret_cast<Fr*>(values));
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_eval_columns_dev(eon_ctx* ctx, const eon_fr* coeffs, uint64_t rows, uint32_t width, const eon_fr* points,
                         uint32_t npoints, eon_fr* values) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if ((npoints && !points) || (width && npoints && !values)) return Status::err(EON_E_ARG, "null argument");
        if (width == 0 || npoints == 0) return Status::ok();
        if (rows == 0) {  // empty column: (empty quotient, 0) (kzg/src/util.rs:101-103)
            EON_HIP(hipMemsetAsync(values, 0, (size_t)npoints * width * sizeof(Fr), ctx->stream));
            return Status::ok();
        }
        if (!coeffs) return Status::err(EON_E_ARG, "null argument");
        const uint64_t nblk = (rows + BL - 1) / BL, nq = (nblk + CH - 1) / CH;
        EON_HIP(ctx->kzg_tmp.ensure((uint64_t)MAX_PTS * (nblk + nq) * width * sizeof(Fr)));
        Fr* totals = ctx->kzg_tmp.as<Fr>();
        Fr* part = totals + (uint64_t)MAX_PTS * nblk * width;
        const Fr* c = reinterpret_cast<const Fr*>(coeffs);
        for (uint32_t p0 = 0; p0 < npoints; p0 += MAX_PTS) {
            const uint32_t np = std::min<uint32_t>(MAX_PTS, npoints - p0);
            Pts zs{}, zbl{}, zch{};
            PtsShoup zsh{};
            for (uint32_t p = 0; p < np; p++) {
                zs.z[p] = fr_from_abi(points + p0 + p);
                if (!fr_is_canonical(zs.z[p])) return Status::err(EON_E_ARG, "point is not a canonical Fr");
                zbl.z[p] = pow_u64(zs.z[p], BL);
                zch.z[p] = pow_u64(zbl.z[p], CH);
                // z 2^261 mod p (the Montgomery form of 32 z) -> plain z and its Shoup quotient
                shoup_pair29<FrP>(unpack29(ntt_scale_form(zs.z[p])), zsh.w[p], zsh.q[p]);
            }
            ctx->prof.begin("k_eval_block", rows * width * 32ull, ctx->stream);
            hipLaunchKernelGGL(k_eval_block, dim3((unsigned)((nblk * width + 127) / 128)), dim3(128), 0, ctx->stream,
                               c, rows, width, zsh, np, totals);
            ctx->prof.end(ctx->stream);
            hipLaunchKernelGGL(k_eval_chunks, dim3((unsigned)((np * nq * width + 127) / 128)), dim3(128), 0,
                               ctx->stream, totals, nblk, width, zbl, np, part);
            hipLaunchKernelGGL(k_eval_final, dim3((unsigned)((np * width + 63) / 64)), dim3(64), 0, ctx->stream, part,
                               nq, width, zch, np, reinterpret_cast<Fr*>(values) + (uint64_t)p0 * width);
            EON_HIP(hipGetLastError());
        }
        return Status::ok();
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_quotient_and_eval_columns_dev(eon_ctx* ctx, const eon_fr* coeffs, uint64_t rows,
                                      uint32_t width, const eon_fr* point, eon_fr* quotient,
                                      eon_fr* values) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (!point || (width && !values)) return Status::err(EON_E_ARG, "null argument");
        if (width == 0) return Status::ok();
        if (rows == 0) {  // empty column: (empty quotient, 0) (kzg/src/util.rs:101-103)
            EON_HIP(hipMemsetAsync(values, 0, (size_t)width * sizeof(Fr), ctx->stream));
            return Status::ok();
        }
        if (!coeffs) return Status::err(EON_E_ARG, "null argument");
        const Fr z = fr_from_abi(point);
        if (!fr_is_canonical(z)) return Status::err(EON_E_ARG, "point is not a canonical Fr");
        const uint64_t nblk = (rows + BL - 1) / BL;
        EON_HIP(ctx->kzg_tmp.ensure(2 * nblk * width * sizeof(Fr)));
        Fr* totals = ctx->kzg_tmp.as<Fr>();
        Fr* carries = totals + nblk * width;
        const Fr* c = reinterpret_cast<const Fr*>(coeffs);
        const uint64_t threads = nblk * width;
        const unsigned grid = (unsigned)((threads + 127) / 128);
        ctx->prof.begin("k_horner_block", rows * width * 32ull, ctx->stream);
        hipLaunchKernelGGL(k_horner_block, dim3(grid), dim3(128), 0, ctx->stream, c, rows, width, z, totals);
        ctx->prof.end(ctx->stream);
        hipLaunchKernelGGL(k_horner_carry, dim3((width + 63) / 64), dim3(64), 0, ctx->stream, totals, nblk,
                           width, pow_u64(z, BL), carries, reinterpret_cast<Fr*>(values));
        if (!quotient || rows < 2) return Status::ok();  // values only
        ctx->prof.begin("k_horner_apply", rows * width * 64ull, ctx->stream);
        hipLaunchKernelGGL(k_horner_apply, dim3(grid), dim3(128), 0, ctx->stream, c, rows, width, z, carries,
                           reinterpret_cast<Fr*>(quotient));
        ctx->prof.end(ctx->stream);
        EON_HIP(hipGetLastError());
        return Status::ok();
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

}  // extern "C"
