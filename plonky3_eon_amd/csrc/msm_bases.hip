// The MSM's bases object: the affine points, the fixed-base window table (2^(c w) P_i) and their
// 29-Montgomery forms the piece sums read; the batched XYZZ -> affine conversions on the device and
// on the host.  The pipeline that consumes them is described in msm.hip.
#include <cstdlib>
#include <vector>

#include "msm_batch.h"
#include "fq_host.h"

using namespace eon;

struct eon_msm_bases {
    eon_ctx* ctx = nullptr;
    uint64_t n = 0;
    DevBuf points;  // n affine bases
    bool precomputed = false;
    uint32_t c = 0, windows = 0;
    DevBuf table;  // precomputed: n * windows affine points, entry i * windows + w = 2^(c*w) P_i
    // the piece sums read 29-Montgomery coordinates from `table` (precomputed) or `points29`;
    // `points` stays in the ABI form (the KZG opening bases are derived from it)
    DevBuf points29;
    // 3 * table (29-form affine, same layout), built on first use by the KZG opening bases'
    // radix-4 fixed-base multiplications (bases_table3_29)
    DevBuf table3;
    // points / table come from (and return to) the context's DevPool (the opening bases)
    bool pooled = false;
};

namespace eon {

// affine points (canonical radix-2^32 Montgomery) -> 29-Montgomery in place; (0, 0) stays
__global__ void k_table_to29(G1Affine* pts, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine a = ld_affine(pts + i);
    a.x = to_fq261(a.x);
    a.y = to_fq261(a.y);
    st_affine(pts + i, a);
}

// --- fixed-base precomputation ------------------------------------------------------------
// tmp[i * W + w] = 2^(c*w) * P_i (XYZZ)
__global__ void k_precompute_windows(const G1Affine* pts, uint64_t n, uint32_t c, uint32_t W,
                                     G1Xyzz* tmp) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Xyzz p = xyzz_from_affine(ld_affine(pts + i));
    for (uint32_t w = 0; w < W; w++) {
        st_xyzz(tmp + i * W + w, p);
        if (w + 1 < W)
            for (uint32_t k = 0; k < c; k++) p = xyzz_dbl(p);
    }
}

// XYZZ -> affine with Montgomery's batch inversion over chunks of BATCH consecutive points; the
// prefix products are parked in the outputs' x coordinates (no per-lane array, no scratch)
template <uint32_t CHUNK>
__global__ void k_batch_to_affine(const G1Xyzz* in, uint64_t m, G1Affine* out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i0 = t * CHUNK;
    if (i0 >= m) return;
    const uint64_t i1 = min(i0 + CHUNK, m);
    Fq acc = Fq::one();
    for (uint64_t i = i0; i < i1; i++) {
        st_vec(&out[i].x, acc);
        if (!ld_pinned(&in[i].ZZ).is_zero()) acc = mul(acc, ld_pinned(&in[i].ZZZ));
    }
    Fq inv = inverse(acc);
    for (uint64_t i = i1; i-- > i0;) {
        const G1Xyzz p = ld_xyzz(in + i);
        if (is_inf(p)) {
            st_affine(out + i, xyzz_to_affine_with_inv(p, Fq::zero()));
            continue;
        }
        const Fq inv_zzz = mul(inv, ld_pinned(&out[i].x));
        inv = mul(inv, p.ZZZ);
        st_affine(out + i, xyzz_to_affine_with_inv(p, inv_zzz));
    }
}

uint32_t choose_c(uint64_t n, bool precomputed) {
    // minimise mixed additions n * ceil(255 / c) plus the bucket reduction, ~6 full additions
    // per bucket (per window when the windows keep their own buckets)
    uint32_t best = MSM_C_MIN;
    double best_cost = 1e300;
    for (uint32_t c = MSM_C_MIN; c <= MSM_C_MAX; c++) {
        const double W = (255 + c - 1) / c;
        const double buckets = (double)(1u << (c - 1)) * (precomputed ? 1.0 : W);
        const double cost = (double)n * W + 6.0 * buckets;
        if (cost < best_cost) {
            best_cost = cost;
            best = c;
        }
    }
    return best;
}

// every bases object's window size passes this where it is set, so B = 2^(c - 1) >= SEG downstream
static bool window_size_ok(uint32_t c) { return c >= MSM_C_MIN && c <= MSM_C_MAX; }

static G1Affine g1_from_abi(const eon_g1_affine& a) {
    G1Affine r;
    for (int i = 0; i < 4; i++) {
        r.x.v[2 * i] = (uint32_t)a.x[i];
        r.x.v[2 * i + 1] = (uint32_t)(a.x[i] >> 32);
        r.y.v[2 * i] = (uint32_t)a.y[i];
        r.y.v[2 * i + 1] = (uint32_t)(a.y[i] >> 32);
    }
    return r;
}

static bool fq_canonical(const Fq& x) {
    for (int i = 7; i >= 0; i--) {
        if (x.v[i] < FqP::P[i]) return true;
        if (x.v[i] > FqP::P[i]) return false;
    }
    return false;
}

hipError_t launch_batch_to_affine(const G1Xyzz* in, uint64_t m, G1Affine* out, hipStream_t st) {
    if (m == 0) return hipSuccess;
    // one inversion (~380 dependent products) per BATCH points: a smaller chunk spends more
    // products, a larger one leaves the SIMDs idle behind the latency of too few waves
    const unsigned threads = 128;
    hipLaunchKernelGGL(k_batch_to_affine<BATCH>, dim3(blocks_for((m + BATCH - 1) / BATCH, threads)), dim3(threads), 0,
                       st, in, m, out);
    return hipGetLastError();
}

Status bases_create(eon_ctx* ctx, const eon_g1_affine* bases, uint64_t n, uint32_t flags,
                    bool device_ptr, eon_msm_bases** out, uint32_t force_c, hipStream_t stream,
                    DevBuf* async_tmp) {
    if (!out) return Status::err(EON_E_ARG, "null output handle");
    if (n && !bases) return Status::err(EON_E_ARG, "null bases");
    if (n > (1ull << 27)) return Status::err(EON_E_SHAPE, "at most 2^27 bases");
    if (force_c && !window_size_ok(force_c)) return Status::err(EON_E_ARG, "MSM window size outside 4..20");
    if (!device_ptr) {
        for (uint64_t i = 0; i < n; i++) {
            const G1Affine a = g1_from_abi(bases[i]);
            if (!fq_canonical(a.x) || !fq_canonical(a.y))
                return Status::err(EON_E_ARG, "base coordinate is not a canonical Fq");
        }
    }
    eon_msm_bases* b = new eon_msm_bases();
    b->ctx = ctx;
    b->n = n;
    // async_tmp: enqueue on `stream` and return without a sync, the precompute scratch parked in
    // *async_tmp until the caller has synchronised the stream
    hipStream_t st = async_tmp ? stream : ctx->stream;
    auto fail = [&](Status s) {
        b->points.release();
        b->table.release();
        b->points29.release();
        delete b;
        return s;
    };
    hipError_t e = b->points.ensure((n ? n : 1) * sizeof(G1Affine));
    if (e != hipSuccess) return fail(Status::err(EON_E_OOM, "bases allocation failed"));
    if (n) {
        e = hipMemcpyAsync(b->points.p, bases, n * sizeof(G1Affine),
                           device_ptr ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(Status::err(EON_E_DEVICE, hipGetErrorString(e)));
    }
    b->precomputed = (flags & EON_MSM_PRECOMPUTE) != 0 && n > 0;
    // EON_MSM_FORCE_C (tests): the window width of a fixed-base table, e.g. c = 16 at sizes whose
    // own choice is narrower, so the fused digit sort (batch_sort) runs at test sizes
    if (!force_c && b->precomputed) {
        const char* fc = getenv("EON_MSM_FORCE_C");
        const int v = fc ? atoi(fc) : 0;
        if (v > 0 && window_size_ok((uint32_t)v)) force_c = (uint32_t)v;
    }
    b->c = force_c ? force_c : choose_c(n ? n : 1, b->precomputed);
    b->windows = (255 + b->c - 1) / b->c;
    if (b->precomputed) {
        const uint64_t m = n * b->windows;
        DevBuf tmp_local;
        DevBuf& tmp = async_tmp ? *async_tmp : tmp_local;
        if (tmp.ensure(m * sizeof(G1Xyzz)) != hipSuccess ||
            b->table.ensure(m * sizeof(G1Affine)) != hipSuccess) {
            tmp.release();
            return fail(Status::err(EON_E_OOM, "precomputed table allocation failed"));
        }
        hipLaunchKernelGGL(k_precompute_windows, dim3(blocks_for(n, 128)), dim3(128), 0, st,
                           b->points.as<G1Affine>(), n, b->c, b->windows, tmp.as<G1Xyzz>());
        e = launch_batch_to_affine(tmp.as<G1Xyzz>(), m, b->table.as<G1Affine>(), st);
        if (!async_tmp) {
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            tmp.release();
        }
        if (e != hipSuccess) return fail(Status::err(EON_E_DEVICE, hipGetErrorString(e)));
    }
    if (n) {
        const uint64_t m = b->precomputed ? n * b->windows : n;
        if (!b->precomputed) {
            e = b->points29.ensure(n * sizeof(G1Affine));
            if (e == hipSuccess)
                e = hipMemcpyAsync(b->points29.p, b->points.p, n * sizeof(G1Affine), hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return fail(Status::err(EON_E_OOM, "bases allocation failed"));
        }
        G1Affine* src = b->precomputed ? b->table.as<G1Affine>() : b->points29.as<G1Affine>();
        hipLaunchKernelGGL(k_table_to29, dim3(blocks_for(m, 256)), dim3(256), 0, st, src, m);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(Status::err(EON_E_DEVICE, hipGetErrorString(e)));
    }
    if (!async_tmp) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(Status::err(EON_E_DEVICE, hipGetErrorString(e)));
    *out = b;
    return Status::ok();
}

const G1Affine* bases_points(const eon_msm_bases* b) { return b->points.as<G1Affine>(); }

// out[e] = 3 tab[e] (tab: 29-form canonical affine; out radix-2^32 XYZZ for the batched affine
// conversion)
__global__ void k_triple29(const G1Affine* tab, uint64_t m, G1Xyzz* out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m) return;
    const G1Affine a = ld_affine(tab + e);
    if (is_inf(a)) {
        st_xyzz(out + e, xyzz_inf());
        return;
    }
    const F29 x = unpack29(a.x), y = unpack29(a.y);
    G1X29 acc = dbl29_affine(x, y);  // 2T (T has odd order r: 2T != -T, != O)
    bool inf = false;
    if (!madd29(acc, x, y)) inf = madd29_exceptional(acc, x, y);
    st_xyzz(out + e, x29_to_xyzz(acc, inf));
}

const G1Affine* bases_table3_29(const eon_msm_bases* cb, hipStream_t st) {
    eon_msm_bases* b = const_cast<eon_msm_bases*>(cb);  // a cache filled once
    if (!b->precomputed || b->n == 0) return nullptr;
    if (b->table3.p) return b->table3.as<G1Affine>();
    const uint64_t m = b->n * b->windows;
    DevBuf tmp;
    if (tmp.ensure(m * sizeof(G1Xyzz)) != hipSuccess || b->table3.ensure(m * sizeof(G1Affine)) != hipSuccess) {
        tmp.release();
        b->table3.release();
        return nullptr;
    }
    hipLaunchKernelGGL(k_triple29, dim3(blocks_for(m, 128)), dim3(128), 0, st, b->table.as<G1Affine>(), m,
                       tmp.as<G1Xyzz>());
    hipError_t e = launch_batch_to_affine(tmp.as<G1Xyzz>(), m, b->table3.as<G1Affine>(), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_table_to29, dim3(blocks_for(m, 256)), dim3(256), 0, st, b->table3.as<G1Affine>(), m);
        e = hipStreamSynchronize(st);  // tmp is released below
    }
    tmp.release();
    if (e != hipSuccess) {
        b->table3.release();
        return nullptr;
    }
    return b->table3.as<G1Affine>();
}

const G1Affine* bases_table29(const eon_msm_bases* b) {
    return b->precomputed ? b->table.as<G1Affine>() : nullptr;
}

uint32_t bases_windows(const eon_msm_bases* b) { return b->windows; }

Status bases_alloc_table(eon_ctx* ctx, uint64_t n, uint32_t c, eon_msm_bases** out) {
    if (n == 0 || n > (1ull << 27)) return Status::err(EON_E_SHAPE, "table bases need 1 <= n <= 2^27");
    if (!window_size_ok(c)) return Status::err(EON_E_ARG, "MSM window size outside 4..20");
    auto* b = new eon_msm_bases();
    b->ctx = ctx;
    b->n = n;
    b->precomputed = true;
    b->c = c;
    b->windows = (255 + c - 1) / c;
    b->pooled = true;
    if (ctx->pool.take(b->points, n * sizeof(G1Affine)) != hipSuccess ||
        ctx->pool.take(b->table, n * b->windows * sizeof(G1Affine)) != hipSuccess) {
        bases_free(b);
        return Status::err(EON_E_OOM, "bases allocation failed");
    }
    *out = b;
    return Status::ok();
}

G1Affine* bases_table_mut(eon_msm_bases* b) { return b->table.as<G1Affine>(); }

Status bases_seal_table(eon_msm_bases* b, hipStream_t st) {
    // points = the w = 0 entries (radix-2^32 ABI form), then the table to 29-Montgomery
    EON_HIP(hipMemcpy2DAsync(b->points.p, sizeof(G1Affine), b->table.p, sizeof(G1Affine) * b->windows,
                             sizeof(G1Affine), b->n, hipMemcpyDeviceToDevice, st));
    const uint64_t m = b->n * b->windows;
    hipLaunchKernelGGL(k_table_to29, dim3(blocks_for(m, 256)), dim3(256), 0, st, b->table.as<G1Affine>(), m);
    EON_HIP(hipGetLastError());
    return Status::ok();
}

void bases_free(eon_msm_bases* b) {
    if (b->pooled) {  // the caller has synchronised the context's streams
        b->ctx->pool.give(b->points);
        b->ctx->pool.give(b->table);
    }
    b->points.release();
    b->table.release();
    b->table3.release();
    b->points29.release();
    delete b;
}

uint32_t bases_window(const eon_msm_bases* b) { return b->c; }

uint64_t bases_len(const eon_msm_bases* b) { return b->n; }

const G1Affine* bases_pieces29(const eon_msm_bases* b) {
    return b->precomputed ? b->table.as<G1Affine>() : b->points29.as<G1Affine>();
}

bool bases_precomputed(const eon_msm_bases* b) { return b->precomputed; }

// ---- host-side XYZZ -> affine for a call's few results ------------------------------------------
// A device conversion of a handful of points is one thread's Fermat inversion: ~380 dependent
// products, ~0.5 ms of latency per call (0.7 ms of a 2^20 MSM's 3.5).  The results travel to the
// host anyway, so they are converted there: Montgomery batch inversion with 64-bit limbs (the same
// R = 2^256 residues, so the bytes equal the device conversion's).
namespace hostq {

static F from_dev(const Fq& a) {
    F r;
    for (int i = 0; i < 4; i++) r.l[i] = (uint64_t)a.v[2 * i] | ((uint64_t)a.v[2 * i + 1] << 32);
    return r;
}

static Fq to_dev(const F& a) {
    Fq r;
    for (int i = 0; i < 4; i++) {
        r.v[2 * i] = (uint32_t)a.l[i];
        r.v[2 * i + 1] = (uint32_t)(a.l[i] >> 32);
    }
    return r;
}

// out[i] = affine(in[i]) (x = X / ZZ, y = Y / ZZZ; the identity -> (0, 0))
static void batch_to_affine(const G1Xyzz* in, uint64_t m, G1Affine* out) {
    std::vector<F> pre(m);
    F acc{{0, 0, 0, 0}};
    bool any = false;
    for (uint64_t i = 0; i < m; i++) {
        pre[i] = acc;
        const F zzz = from_dev(in[i].ZZZ);
        if (is_zero(from_dev(in[i].ZZ))) continue;
        acc = any ? mul(acc, zzz) : zzz;
        any = true;
    }
    if (!any) {
        for (uint64_t i = 0; i < m; i++) out[i] = G1Affine{Fq::zero(), Fq::zero()};
        return;
    }
    F inv = inverse(acc);  // 1 / prod ZZZ over the non-identity points
    for (uint64_t i = m; i-- > 0;) {
        if (is_zero(from_dev(in[i].ZZ))) {
            out[i] = G1Affine{Fq::zero(), Fq::zero()};
            continue;
        }
        const F zzz = from_dev(in[i].ZZZ);
        // pre[i] = product of the earlier non-identity ZZZ (zero when there is none)
        const bool first_live = is_zero(pre[i]);
        const F inv_zzz = first_live ? inv : mul(inv, pre[i]);
        if (!first_live) inv = mul(inv, zzz);
        const F inv_z = mul(from_dev(in[i].ZZ), inv_zzz);  // ZZ / ZZZ = 1 / Z
        out[i].x = to_dev(mul(from_dev(in[i].X), mul(inv_z, inv_z)));
        out[i].y = to_dev(mul(from_dev(in[i].Y), inv_zzz));
    }
}

}  // namespace hostq

void host_xyzz_to_affine(const G1Xyzz* in, uint64_t m, G1Affine* out) { hostq::batch_to_affine(in, m, out); }

}  // namespace eon

// the object's own entry points; the rest of the C API is in msm.hip
extern "C" {

void eon_msm_bases_destroy(eon_msm_bases* b) {
    if (!b) return;
    std::lock_guard<std::mutex> lk(b->ctx->mu);
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->ctx->stream);
    eon::bases_free(b);
}

uint64_t eon_msm_bases_len(const eon_msm_bases* b) { return b ? b->n : 0; }

}  // extern "C"
