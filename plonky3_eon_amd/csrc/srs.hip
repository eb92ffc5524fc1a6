// Test-SRS generation on device: init_srs_unsafe's g1_powers[i] = alpha^i * G
// (kzg/src/params.rs:123-139).  Setup cost, not prove time; it lets
// the MSM benchmark and tests build 2^20+ bases without a host scalar-multiplication loop.
#include <cstdint>
#include <string>

#include "context.h"
#include "ec.h"
#include "msm.h"
#include "pairing_consts.h"

using namespace eon;

namespace {

constexpr uint32_t CHUNK = 4;  // consecutive exponents per thread

__global__ void k_srs_points(uint64_t n, Fr alpha, G1Xyzz* out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i0 = t * CHUNK;
    if (i0 >= n) return;
    // alpha^i0 by square-and-multiply, then consecutive powers
    Fr s = Fr::one(), b = alpha;
    for (uint64_t e = i0; e; e >>= 1) {
        if (e & 1) s = mul(s, b);
        b = sqr(b);
    }
    G1Affine g;
    g.x = from_u64<FqP>(1);
    g.y = from_u64<FqP>(2);
    const uint64_t i1 = i0 + CHUNK < n ? i0 + CHUNK : n;
    for (uint64_t i = i0; i < i1; i++) {
        const Fr k = to_canonical(s);
        G1Xyzz acc = xyzz_inf();
        for (int w = 7; w >= 0; w--)
            for (int bit = 31; bit >= 0; bit--) {
                acc = xyzz_dbl(acc);
                if ((k.v[w] >> bit) & 1) acc = xyzz_add_affine(acc, g);
            }
        out[i] = acc;
        s = mul(s, alpha);
    }
}

Status srs_dev(eon_ctx* ctx, const eon_fr* alpha, uint64_t n, G1Affine* out) {
    if (!alpha) return Status::err(EON_E_ARG, "null alpha");
    if (n == 0) return Status::ok();
    const Fr a = fr_from_abi(alpha);
    if (!fr_is_canonical(a)) return Status::err(EON_E_ARG, "alpha is not a canonical Fr");
    DevBuf tmp;
    EON_HIP(tmp.ensure(n * sizeof(G1Xyzz)));
    const uint64_t threads = (n + CHUNK - 1) / CHUNK;
    hipLaunchKernelGGL(k_srs_points, dim3((unsigned)((threads + 127) / 128)), dim3(128), 0,
                       ctx->stream, n, a, tmp.as<G1Xyzz>());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_batch_to_affine(tmp.as<G1Xyzz>(), n, out, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    tmp.release();
    EON_HIP(e);
    return Status::ok();
}

// ---- a supplied SRS: decompress, validate, structure check (eon.h) ------------------------------
//
//   k_g1_decompress  one compressed point per lane: x -> Montgomery, t = x^3 + 3, y = t^((q+1)/4)
//                    by one fixed chain of 2-bit windows (the exponent is a constant, so every
//                    branch of the chain is uniform over the wave: no divergence, and a rejected
//                    lane runs the chain on whatever it holds and stores (0,0)), y^2 == t, parity
//   k_g1_compress    the inverse, one affine point per lane: both coordinates out of Montgomery
//                    form (one product by 1 each), x as two 16-byte stores with y's parity in bit
//                    255; (0,0) -> the identity flag; a coordinate >= q is rejected, 32 zero bytes
//   k_g1_validate    one affine point per lane: coordinates < q, not (0,0), on the curve
//   k_rho_columns    the n x 2 matrix (rho^0 .. rho^(n-2), 0 | 0, rho^0 .. rho^(n-2)) of the
//                    structure check, one row pair per lane
// A rejecting lane folds (index << 3 | reason) into one 64-bit word with a vector atomic minimum,
// so the report names the lowest bad index whatever the order the waves ran in.

constexpr uint32_t SRS_THREADS = 256;  // the workgroup of the per-point kernels
constexpr unsigned long long SRS_NONE = ~0ull;

struct SqrtExp {
    uint32_t w[8];
};

// (q + 1) / 4 as 8 LE words; q = 3 mod 4, so t^((q+1)/4) is a square root of every square t
constexpr SqrtExp sqrt_exponent() {
    SqrtExp e{};
    uint32_t p1[8] = {};
    uint64_t c = 1;
    for (int i = 0; i < 8; i++) {
        c += FqP::P[i];
        p1[i] = (uint32_t)c;
        c >>= 32;
    }
    for (int i = 0; i < 8; i++) e.w[i] = (p1[i] >> 2) | (i < 7 ? p1[i + 1] << 30 : 0u);
    return e;
}
constexpr SqrtExp SQRT_EXP = sqrt_exponent();
static_assert(SQRT_EXP.w[7] >> 28 == 0, "(q + 1) / 4 fits 252 bits: 126 two-bit windows");
__constant__ SqrtExp d_sqrt_exp = SQRT_EXP;

__device__ __forceinline__ bool fq_lt_q(const Fq& x) {
    int64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        br += (int64_t)x.v[i] - FqP::P[i];
        br >>= 32;
    }
    return br < 0;
}

__device__ __forceinline__ Fq fq_three() {
    const Fq one = Fq::one();
    return add(add(one, one), one);
}

// t^((q+1)/4): bits 251..0 of the exponent two at a time, most significant first
__device__ __forceinline__ Fq fq_sqrt_candidate(const Fq& t) {
    const Fq t2 = sqr(t), t3 = mul(t2, t);
    Fq r = Fq::one();
    for (int d = 125; d >= 0; d--) {
        r = sqr(sqr(r));
        const uint32_t dig = (d_sqrt_exp.w[d >> 4] >> (2 * (d & 15))) & 3u;  // uniform over the wave
        if (dig) {
            Fq m;
#pragma unroll
            for (int i = 0; i < 8; i++) m.v[i] = dig == 1 ? t.v[i] : dig == 2 ? t2.v[i] : t3.v[i];
            r = mul(r, m);
        }
    }
    return r;
}

__device__ __forceinline__ void srs_reject(unsigned long long* worst, uint64_t i, uint32_t reason) {
    atomicMin(worst, (unsigned long long)(i << 3 | reason));
}

__global__ void __launch_bounds__(SRS_THREADS) k_g1_decompress(const uint32_t* __restrict__ bytes, uint64_t n,
                                                               G1Affine* __restrict__ out,
                                                               unsigned long long* __restrict__ worst) {
    const uint64_t i = (uint64_t)blockIdx.x * SRS_THREADS + threadIdx.x;
    if (i >= n) return;
    Fq x;
#pragma unroll
    for (int j = 0; j < 8; j++) x.v[j] = bytes[i * 8 + j];
    const bool odd = (x.v[7] >> 31) != 0, inf = ((x.v[7] >> 30) & 1u) != 0;
    uint32_t rest = x.v[7] & 0xbfffffffu;  // everything but the identity flag
#pragma unroll
    for (int j = 0; j < 7; j++) rest |= x.v[j];
    x.v[7] &= 0x3fffffffu;
    uint32_t reason = EON_SRS_OK;
    if (inf) {
        if (rest) reason = EON_SRS_ENCODING;
    } else if (!fq_lt_q(x)) {
        reason = EON_SRS_NOT_CANONICAL;
    }
    Fq r2;
#pragma unroll
    for (int j = 0; j < 8; j++) r2.v[j] = FqP::R2[j];
    const Fq xm = mul(x, r2);
    const Fq t = add(mul(sqr(xm), xm), fq_three());
    Fq y = fq_sqrt_candidate(t);
    if (reason == EON_SRS_OK && !inf && sqr(y) != t) reason = EON_SRS_NOT_ON_CURVE;
    if (((to_canonical(y).v[0] & 1u) != 0) != odd) y = neg(y);
    G1Affine p;
    const bool keep = reason == EON_SRS_OK && !inf;
    p.x = keep ? xm : Fq::zero();
    p.y = keep ? y : Fq::zero();
    st_affine(out + i, p);
    if (reason != EON_SRS_OK) srs_reject(worst, i, reason);
}

__global__ void __launch_bounds__(SRS_THREADS) k_g1_compress(const G1Affine* __restrict__ pts, uint64_t n,
                                                             uint4* __restrict__ out,
                                                             unsigned long long* __restrict__ worst) {
    const uint64_t i = (uint64_t)blockIdx.x * SRS_THREADS + threadIdx.x;
    if (i >= n) return;
    const G1Affine p = ld_affine(pts + i);
    const bool bad = !fq_lt_q(p.x) || !fq_lt_q(p.y), inf = is_inf(p);
    const Fq x = to_canonical(p.x), y = to_canonical(p.y);
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = bad || inf ? 0u : x.v[j];  // x < q < 2^254: bits 254, 255 are free
    if (!bad) w[7] |= inf ? 0x40000000u : (y.v[0] & 1u) << 31;
    out[2 * i] = make_uint4(w[0], w[1], w[2], w[3]);
    out[2 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    if (bad) srs_reject(worst, i, EON_SRS_NOT_CANONICAL);
}

__global__ void __launch_bounds__(SRS_THREADS) k_g1_validate(const G1Affine* __restrict__ pts, uint64_t n,
                                                             unsigned long long* __restrict__ worst) {
    const uint64_t i = (uint64_t)blockIdx.x * SRS_THREADS + threadIdx.x;
    if (i >= n) return;
    const G1Affine p = ld_affine(pts + i);
    uint32_t reason = EON_SRS_OK;
    if (!fq_lt_q(p.x) || !fq_lt_q(p.y))
        reason = EON_SRS_NOT_CANONICAL;
    else if (is_inf(p))
        reason = EON_SRS_IDENTITY;
    else if (sqr(p.y) != add(mul(sqr(p.x), p.x), fq_three()))
        reason = EON_SRS_NOT_ON_CURVE;
    if (reason != EON_SRS_OK) srs_reject(worst, i, reason);
}

// rows i < n - 1: mat[i][0] = mat[i + 1][1] = rho^i; mat[n - 1][0] = mat[0][1] = 0 (n >= 2)
__global__ void __launch_bounds__(SRS_THREADS) k_rho_columns(Fr rho, uint64_t n, Fr* __restrict__ mat) {
    const uint64_t i = (uint64_t)blockIdx.x * SRS_THREADS + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) {
        st_vec(mat + 2 * i, Fr::zero());
        st_vec(mat + 1, Fr::zero());
        return;
    }
    Fr s = Fr::one(), b = rho;
    for (uint64_t e = i; e; e >>= 1) {
        if (e & 1) s = mul(s, b);
        b = sqr(b);
    }
    st_vec(mat + 2 * i, s);
    st_vec(mat + 2 * (i + 1) + 1, s);
}

void report_from_word(unsigned long long w, eon_srs_report* report) {
    report->reason = w == SRS_NONE ? (uint32_t)EON_SRS_OK : (uint32_t)(w & 7u);
    report->pad = 0;
    report->index = w == SRS_NONE ? 0 : (uint64_t)(w >> 3);
}

const char* srs_reason_name(uint32_t reason) {
    static const char* const names[] = {"ok", "bad identity encoding", "coordinate is not canonical",
                                        "point is not on the curve", "point is the identity",
                                        "g1_powers[0] is not the generator", "g2_alpha is not a valid G2 element",
                                        "the points are not consecutive powers of g2_alpha's scalar"};
    return reason < 8 ? names[reason] : "?";
}

Status srs_rejected(const eon_srs_report& r) {
    std::string m = std::string("SRS rejected: ") + srs_reason_name(r.reason);
    if (r.reason >= EON_SRS_ENCODING && r.reason <= EON_SRS_IDENTITY) m += " (index " + std::to_string(r.index) + ")";
    return Status::err(EON_E_SRS, m);
}

// runs `launch(worst)` with a fresh device word and reads the report back (caller holds ctx->mu)
template <class L>
Status per_point_check(eon_ctx* ctx, eon_srs_report* report, L&& launch) {
    DevBuf word;
    PoolScope ps(ctx->pool, ctx->stream);
    EON_HIP(ps.take(word, 256));
    EON_HIP(hipMemsetAsync(word.p, 0xff, 8, ctx->stream));
    launch(word.as<unsigned long long>());
    EON_HIP(hipGetLastError());
    unsigned long long w = SRS_NONE;
    EON_HIP(hipMemcpyAsync(&w, word.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    EON_HIP(hipStreamSynchronize(ctx->stream));
    report_from_word(w, report);
    return report->reason == EON_SRS_OK ? Status::ok() : srs_rejected(*report);
}

Status decompress_dev(eon_ctx* ctx, const uint8_t* bytes, uint64_t n, G1Affine* out, eon_srs_report* report) {
    if (n > (1ull << 27)) return Status::err(EON_E_SHAPE, "at most 2^27 points");
    if (n == 0) return Status::ok();
    if (reinterpret_cast<uintptr_t>(bytes) & 3)
        return Status::err(EON_E_ARG, "compressed points must be 4-byte aligned");
    return per_point_check(ctx, report, [&](unsigned long long* worst) {
        ctx->prof.begin("k_g1_decompress", n * (32 + 64), ctx->stream);
        hipLaunchKernelGGL(k_g1_decompress, dim3((unsigned)((n + SRS_THREADS - 1) / SRS_THREADS)), dim3(SRS_THREADS), 0,
                           ctx->stream, reinterpret_cast<const uint32_t*>(bytes), n, out, worst);
        ctx->prof.end(ctx->stream);
    });
}

Status compress_dev(eon_ctx* ctx, const G1Affine* pts, uint64_t n, uint8_t* bytes, eon_srs_report* report) {
    if (n > (1ull << 27)) return Status::err(EON_E_SHAPE, "at most 2^27 points");
    if (n == 0) return Status::ok();
    if ((reinterpret_cast<uintptr_t>(bytes) | reinterpret_cast<uintptr_t>(pts)) & 15)
        return Status::err(EON_E_ARG, "points and compressed bytes must be 16-byte aligned");
    return per_point_check(ctx, report, [&](unsigned long long* worst) {
        ctx->prof.begin("k_g1_compress", n * (64 + 32), ctx->stream);
        hipLaunchKernelGGL(k_g1_compress, dim3((unsigned)((n + SRS_THREADS - 1) / SRS_THREADS)), dim3(SRS_THREADS), 0,
                           ctx->stream, pts, n, reinterpret_cast<uint4*>(bytes), worst);
        ctx->prof.end(ctx->stream);
    });
}

bool g2_abi_is_zero(const eon_g2_affine& q) {
    uint64_t acc = 0;
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < 4; i++) acc |= q.x[k][i] | q.y[k][i];
    return acc == 0;
}

Fq fq_from_abi(const uint64_t (&l)[4]) {
    Fq r;
    for (int i = 0; i < 4; i++) {
        r.v[2 * i] = (uint32_t)l[i];
        r.v[2 * i + 1] = (uint32_t)(l[i] >> 32);
    }
    return r;
}

void fq_to_abi(const Fq& a, uint64_t (&l)[4]) {
    for (int i = 0; i < 4; i++) l[i] = (uint64_t)a.v[2 * i] | (uint64_t)a.v[2 * i + 1] << 32;
}

}  // namespace

extern "C" {

int eon_g1_decompress_dev(eon_ctx* ctx, const uint8_t* bytes, uint64_t n, eon_g1_affine* out,
                          eon_srs_report* report) {
    if (!ctx || !report) return EON_E_ARG;
    *report = eon_srs_report{};
    if (n && (!bytes || !out)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = decompress_dev(ctx, bytes, n, reinterpret_cast<G1Affine*>(out), report);
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_g1_decompress(eon_ctx* ctx, const uint8_t* bytes, uint64_t n, eon_g1_affine* out, eon_srs_report* report) {
    if (!ctx || !report) return EON_E_ARG;
    *report = eon_srs_report{};
    if (n && (!bytes || !out)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (n > (1ull << 27)) return Status::err(EON_E_SHAPE, "at most 2^27 points");
        if (n == 0) return Status::ok();
        DevBuf in, pts;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(in, n * 32));
        EON_HIP(ps.take(pts, n * sizeof(G1Affine)));
        EON_HIP(hipMemcpyAsync(in.p, bytes, n * 32, hipMemcpyHostToDevice, ctx->stream));
        const Status d = decompress_dev(ctx, in.as<uint8_t>(), n, pts.as<G1Affine>(), report);
        if (d.bad() && d.code != EON_E_SRS) return d;
        EON_HIP(hipMemcpyAsync(out, pts.p, n * sizeof(G1Affine), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return d;
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_g1_compress_dev(eon_ctx* ctx, const eon_g1_affine* pts, uint64_t n, uint8_t* bytes, eon_srs_report* report) {
    if (!ctx || !report) return EON_E_ARG;
    *report = eon_srs_report{};
    if (n && (!pts || !bytes)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = compress_dev(ctx, reinterpret_cast<const G1Affine*>(pts), n, bytes, report);
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_g1_compress(eon_ctx* ctx, const eon_g1_affine* pts, uint64_t n, uint8_t* bytes, eon_srs_report* report) {
    if (!ctx || !report) return EON_E_ARG;
    *report = eon_srs_report{};
    if (n && (!pts || !bytes)) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (n > (1ull << 27)) return Status::err(EON_E_SHAPE, "at most 2^27 points");
        if (n == 0) return Status::ok();
        DevBuf in, out;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(in, n * sizeof(G1Affine)));
        EON_HIP(ps.take(out, n * 32));
        EON_HIP(hipMemcpyAsync(in.p, pts, n * sizeof(G1Affine), hipMemcpyHostToDevice, ctx->stream));
        const Status d = compress_dev(ctx, in.as<G1Affine>(), n, out.as<uint8_t>(), report);
        if (d.bad() && d.code != EON_E_SRS) return d;
        EON_HIP(hipMemcpyAsync(bytes, out.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return d;
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_g1_validate_dev(eon_ctx* ctx, const eon_g1_affine* pts, uint64_t n, eon_srs_report* report) {
    if (!ctx || !report) return EON_E_ARG;
    *report = eon_srs_report{};
    if (n && !pts) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (n > (1ull << 27)) return Status::err(EON_E_SHAPE, "at most 2^27 points");
        if (n == 0) return Status::ok();
        return per_point_check(ctx, report, [&](unsigned long long* worst) {
            ctx->prof.begin("k_g1_validate", n * 64, ctx->stream);
            hipLaunchKernelGGL(k_g1_validate, dim3((unsigned)((n + SRS_THREADS - 1) / SRS_THREADS)), dim3(SRS_THREADS),
                               0, ctx->stream, reinterpret_cast<const G1Affine*>(pts), n, worst);
            ctx->prof.end(ctx->stream);
        });
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_kzg_srs_check(eon_ctx* ctx, const eon_msm_bases* bases, uint64_t n, const eon_g2_affine* g2_alpha,
                      const eon_fr* rho, eon_srs_report* report) {
    if (!ctx || !report) return EON_E_ARG;
    *report = eon_srs_report{};
    if (!bases || !g2_alpha || !rho) return EON_E_ARG;
    auto fail = [&](const Status& s) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->last_error = s.msg;
        return s.code;
    };
    auto reject = [&](uint32_t reason) {
        report->reason = reason;
        return fail(srs_rejected(*report));
    };
    if (n == 0 || n > eon_msm_bases_len(bases)) return fail(Status::err(EON_E_SHAPE, "n must be in [1, len(bases)]"));
    const Fr rh = fr_from_abi(rho);
    if (rh.is_zero() || !fr_is_canonical(rh)) return fail(Status::err(EON_E_ARG, "rho must be a nonzero canonical Fr"));
    // 1. G_0 is the generator (1, 2)
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
        G1Affine g0;
        hipError_t e = hipMemcpyAsync(&g0, bases_points(bases), sizeof(g0), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            ctx->last_error = hipGetErrorString(e);
            return EON_E_DEVICE;
        }
        const Fq one = Fq::one();
        if (g0.x != one || g0.y != add(one, one)) {
            report->reason = EON_SRS_G0_NOT_GENERATOR;
            ctx->last_error = srs_rejected(*report).msg;
            return EON_E_SRS;
        }
    }
    // 2. g2_alpha is a nonzero element of the order-r subgroup: [r - 1] Q == -Q.  eon_g2_mul rejects
    // a coordinate >= q and a point off the twist with EON_E_ARG.
    if (g2_abi_is_zero(*g2_alpha)) return reject(EON_SRS_G2_INVALID);
    {
        const Fr rm1 = neg(Fr::one());  // r - 1, Montgomery form
        eon_fr k;
        for (int i = 0; i < 4; i++) k.l[i] = (uint64_t)rm1.v[2 * i] | (uint64_t)rm1.v[2 * i + 1] << 32;
        eon_g2_affine m;
        const int rc = eon_g2_mul(ctx, g2_alpha, &k, &m);
        if (rc == EON_E_ARG) return reject(EON_SRS_G2_INVALID);
        if (rc != EON_OK) return rc;
        bool same = true;
        for (int c = 0; c < 2; c++) {
            uint64_t ny[4];
            fq_to_abi(neg(fq_from_abi(g2_alpha->y[c])), ny);
            for (int i = 0; i < 4; i++) same = same && m.x[c][i] == g2_alpha->x[c][i] && m.y[c][i] == ny[i];
        }
        if (!same) return reject(EON_SRS_G2_INVALID);
    }
    if (n == 1) return EON_OK;
    // 3. e(A, g2_alpha) e(-B, G2) == 1
    G1Affine ab[2];
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
        Status s = [&]() -> Status {
            DevBuf mat;
            PoolScope ps(ctx->pool, ctx->stream);
            EON_HIP(ps.take(mat, n * 2 * sizeof(Fr)));
            ctx->prof.begin("k_rho_columns", n * 64, ctx->stream);
            hipLaunchKernelGGL(k_rho_columns, dim3((unsigned)((n + SRS_THREADS - 1) / SRS_THREADS)), dim3(SRS_THREADS),
                               0, ctx->stream, rh, n, mat.as<Fr>());
            ctx->prof.end(ctx->stream);
            EON_HIP(hipGetLastError());
            return msm_run_columns(ctx, bases, mat.as<Fr>(), n, 2, ab, nullptr);
        }();
        if (s.bad()) {
            ctx->last_error = s.msg;
            return s.code;
        }
    }
    eon_g1_affine p[2];
    eon_g2_affine q[2];
    ab[1] = affine_neg(ab[1]);
    for (int k = 0; k < 2; k++) {
        fq_to_abi(ab[k].x, p[k].x);
        fq_to_abi(ab[k].y, p[k].y);
    }
    q[0] = *g2_alpha;
    for (int c = 0; c < 2; c++) {
        for (int i = 0; i < 4; i++) {
            q[1].x[c][i] = (uint64_t)pc::G2_GEN_X[c][2 * i] | (uint64_t)pc::G2_GEN_X[c][2 * i + 1] << 32;
            q[1].y[c][i] = (uint64_t)pc::G2_GEN_Y[c][2 * i] | (uint64_t)pc::G2_GEN_Y[c][2 * i + 1] << 32;
        }
    }
    eon_fq12 gt;
    const int rc = eon_multi_pairing(ctx, p, q, 2, &gt);
    if (rc != EON_OK) return rc;
    uint64_t one[4];
    fq_to_abi(Fq::one(), one);
    bool is_one = true;
    for (int k = 0; k < 12; k++)
        for (int i = 0; i < 4; i++) is_one = is_one && gt.c[k][i] == (k == 0 ? one[i] : 0);
    if (!is_one) return reject(EON_SRS_STRUCTURE);
    return EON_OK;
}

int eon_g1_srs_powers_dev(eon_ctx* ctx, const eon_fr* alpha, uint64_t n, eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (n && !out) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = srs_dev(ctx, alpha, n, reinterpret_cast<G1Affine*>(out));
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_g1_srs_powers(eon_ctx* ctx, const eon_fr* alpha, uint64_t n, eon_g1_affine* out) {
    if (!ctx) return EON_E_ARG;
    if (n && !out) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        EON_HIP(ctx->stage_out.ensure((n ? n : 1) * sizeof(G1Affine)));
        EON_TRY(srs_dev(ctx, alpha, n, ctx->stage_out.as<G1Affine>()));
        if (n)
            EON_HIP(hipMemcpy(out, ctx->stage_out.p, n * sizeof(G1Affine), hipMemcpyDeviceToHost));
        return Status::ok();
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

}  // extern "C"
