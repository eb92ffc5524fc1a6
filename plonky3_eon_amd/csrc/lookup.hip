// LogUp permutation trace (generate_permutation, lookup/src/logup.rs:379-562) after the term program
// (k_lookup_terms, air_program.hip) has written every row's denominators and multiplicities.
//
// Contributions (k_lookup_contrib), one thread per trace row: Montgomery's trick over the row's T
// denominators -- prefix products, ONE field inversion, the walk back -- gives
// contribution[row][l] = sum over lookup l's terms of multiplicity / denominator, stored to column
// aux[l] of `perm`.  desc = term_off[L + 1] then aux[L].  A zero denominator (the reference panics,
// field/src/batch_inverse.rs:17-18) records the lowest such lookup in *zero_flag and goes on with 1
// in its place.  Field results are canonical, so the schedule is bit-exact against the reference's
// batch_multiplicative_inverse.
//
// Running sum (logup.rs:535-538): `perm` holds contribution[i][c] and leaves holding the exclusive
// prefix sums
//   perm[0][c] = 0,  perm[i + 1][c] = perm[i][c] + contribution[i][c],
// so the last row's contribution is computed (a zero denominator there is still found) but not
// stored.  A blocked scan in place, after kzg.hip's Horner scan:
//   k_sum_block   per (block of BL rows, column): the block's total
//   k_sum_carry   per column, over the blocks bottom-up: carry_b = sum of the totals below b
//   k_sum_apply   per (block, column): the running sum again from carry_b, written over the rows
// threads = (height / BL) x width, adjacent threads = adjacent columns.
#include "context.h"
#include "field29.h"
#include "quotient.h"

using namespace eon;

namespace {

constexpr uint32_t BL = 256;  // rows per scan block

// value k of a row as the term program left it (x 2^261 below 32p in 29-bit limbs: limbs 0-3 and
// 4-7 in 16-byte planes 2k and 2k + 1, limb 8 in a 4-byte plane after them) -> the canonical ABI
// form: times the stored one (2^256), x 2^261 2^256 2^-261 = x 2^256
__device__ __forceinline__ Fr ld_term(const uint4* base, const uint32_t* top, uint32_t k, uint64_t height) {
    const uint4 a = base[(uint64_t)(2 * k) * height], b = base[(uint64_t)(2 * k + 1) * height];
    F29 x;
    x.l[0] = a.x; x.l[1] = a.y; x.l[2] = a.z; x.l[3] = a.w;
    x.l[4] = b.x; x.l[5] = b.y; x.l[6] = b.z; x.l[7] = b.w;
    x.l[8] = top[(uint64_t)k * height];
    return pack29<FrP>(canon29<FrP>(mul29<FrP>(x, unpack29(Fr::one()))));
}

__global__ void k_lookup_contrib(const uint4* __restrict__ emitted, Fr* __restrict__ prefix, uint64_t height,
                                 const uint32_t* __restrict__ desc, uint32_t n_lookups, uint32_t n_terms,
                                 Fr* __restrict__ perm, uint32_t perm_width, uint32_t* zero_flag) {
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= height) return;
    const uint4* base = emitted + row;
    const uint32_t* top = reinterpret_cast<const uint32_t*>(emitted + 4ull * n_terms * height) + row;
    Fr* mine = prefix + row;
    Fr run = Fr::one();
    for (uint32_t l = 0; l < n_lookups; l++)
        for (uint32_t t = desc[l]; t < desc[l + 1]; t++) {
            Fr d = ld_term(base, top, 2 * t, height);
            if (d.is_zero()) {
                atomicMin(zero_flag, l);
                d = Fr::one();
            }
            run = mul(run, d);
            st_vec(mine + (uint64_t)t * height, run);
        }
    Fr inv = inverse(run);  // 1 / (d_0 ... d_(T-1))
    for (uint32_t l = n_lookups; l-- > 0;) {
        Fr sum = Fr::zero();
        for (uint32_t t = desc[l + 1]; t-- > desc[l];) {
            Fr d = ld_term(base, top, 2 * t, height);
            if (d.is_zero()) d = Fr::one();
            const Fr below = t > 0 ? ld_pinned(mine + (uint64_t)(t - 1) * height) : Fr::one();
            const Fr d_inv = mul(inv, below);  // 1 / d_t
            inv = mul(inv, d);
            sum = add(sum, mul(ld_term(base, top, 2 * t + 1, height), d_inv));
        }
        st_vec(perm + row * perm_width + desc[n_lookups + 1 + l], sum);
    }
}


__global__ void k_sum_block(const Fr* perm, uint64_t n, uint32_t width, Fr* totals) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblk = (n + BL - 1) / BL;
    if (t >= nblk * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t b = t / width;
    const uint64_t lo = b * BL, hi = lo + BL < n ? lo + BL : n;
    Fr r = Fr::zero();
    for (uint64_t i = lo; i < hi; i++) r = add(r, ld_pinned(perm + i * width + col));
    st_vec(totals + b * width + col, r);
}

__global__ void k_sum_carry(const Fr* totals, uint64_t nblk, uint32_t width, Fr* carries) {
    const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= width) return;
    Fr carry = Fr::zero();
    for (uint64_t b = 0; b < nblk; b++) {
        st_vec(carries + b * width + col, carry);
        carry = add(carry, ld_pinned(totals + b * width + col));
    }
}

__global__ void k_sum_apply(Fr* perm, uint64_t n, uint32_t width, const Fr* carries) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nblk = (n + BL - 1) / BL;
    if (t >= nblk * width) return;
    const uint32_t col = (uint32_t)(t % width);
    const uint64_t b = t / width;
    const uint64_t lo = b * BL, hi = lo + BL < n ? lo + BL : n;
    Fr r = ld_pinned(carries + b * width + col);
    for (uint64_t i = lo; i < hi; i++) {
        const Fr x = ld_pinned(perm + i * width + col);
        st_vec(perm + i * width + col, r);
        r = add(r, x);
    }
}

}  // namespace

namespace eon {

Status lookup_contributions(eon_ctx* ctx, const uint4* emitted, Fr* prefix, uint64_t height, const uint32_t* desc, uint32_t n_lookups,
                            uint32_t n_terms, Fr* perm, uint32_t perm_width, uint32_t* zero_flag) {
    if (height == 0 || n_lookups == 0) return Status::ok();
    ctx->prof.begin("k_lookup_contrib", height * (3ull * n_terms + perm_width) * 32, ctx->stream);
    hipLaunchKernelGGL(k_lookup_contrib, dim3((unsigned)((height + 127) / 128)), dim3(128), 0, ctx->stream, emitted,
                       prefix, height, desc, n_lookups, n_terms, perm, perm_width, zero_flag);
    ctx->prof.end(ctx->stream);
    EON_HIP(hipGetLastError());
    return Status::ok();
}

Status lookup_running_sum(eon_ctx* ctx, Fr* perm, uint64_t height, uint32_t width) {
    if (width == 0 || height == 0) return Status::ok();
    const uint64_t nblk = (height + BL - 1) / BL;
    EON_HIP(ctx->kzg_tmp.ensure(2 * nblk * width * sizeof(Fr)));
    Fr* totals = ctx->kzg_tmp.as<Fr>();
    Fr* carries = totals + nblk * width;
    const uint64_t threads = nblk * width;
    const unsigned grid = (unsigned)((threads + 127) / 128);
    ctx->prof.begin("k_sum_block", height * width * 32ull, ctx->stream);
    hipLaunchKernelGGL(k_sum_block, dim3(grid), dim3(128), 0, ctx->stream, perm, height, width, totals);
    ctx->prof.end(ctx->stream);
    hipLaunchKernelGGL(k_sum_carry, dim3((width + 63) / 64), dim3(64), 0, ctx->stream, totals, nblk, width, carries);
    ctx->prof.begin("k_sum_apply", height * width * 64ull, ctx->stream);
    hipLaunchKernelGGL(k_sum_apply, dim3(grid), dim3(128), 0, ctx->stream, perm, height, width, carries);
    ctx->prof.end(ctx->stream);
    EON_HIP(hipGetLastError());
    return Status::ok();
}

}  // namespace eon
