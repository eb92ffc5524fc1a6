// Diagnostic: the shader clock the chip holds under this VALU load, and the radix-2^29 product
// rate at that clock, measured live on the box that runs the bench (MI355X_MICROARCH.md, "DVFS
// give-back" item 6: the in-kernel clock is delta s_memtime / delta s_memrealtime x 100 MHz,
// stamped around the loop on random data; sysfs pp_dpm_sclk is not that clock).  Not on any
// product path: bench.py calls it after its timed region, so the bench line can say at what clock
// its numbers were taken and compare the piece sums against the product peak of the same box.
//
// The loop is the roofline denominator's own benchmark (tools/ubench_r29.hip: mul29<Fq>, two
// independent chains per thread, 256-thread blocks, 4096 blocks) with both timestamps taken by
// wave 0 of every block around its chain; the result is the median over blocks.
#include <algorithm>
#include <vector>

#include "context.h"
#include "ec29.h"
#include "field29.h"
#include "sort.h"

namespace {

using namespace eon;

constexpr uint32_t PROBE_THREADS = 256, PROBE_BLOCKS = 4096;

__global__ void __launch_bounds__(PROBE_THREADS) k_clock_probe(uint32_t iters, uint32_t seed, uint64_t* stamps,
                                                               uint32_t* sink) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t s = (tid ^ seed) * 2654435761u + 0x9e3779b9u;
    auto rnd = [&]() {
        s = s * 1664525u + 1013904223u;
        return s;
    };
    F29 x0, x1, y;  // random values below 2^248 < p, normalised limbs
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const uint32_t m = i == 8 ? 0xffffu : M29;
        x0.l[i] = rnd() & m;
        x1.l[i] = rnd() & m;
        y.l[i] = rnd() & m;
    }
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
    for (uint32_t it = 0; it < iters; it++) {
        x0 = mul29<FqP>(x0, y);
        x1 = mul29<FqP>(x1, y);
    }
    const uint64_t t1 = __builtin_amdgcn_s_memtime();
    const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        stamps[2 * blockIdx.x] = t1 - t0;
        stamps[2 * blockIdx.x + 1] = r1 - r0;
    }
    uint32_t h = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) h ^= x0.l[i] ^ x1.l[i];
    if (h == 0x5bd1e995u) sink[0] = tid;  // keeps both chains live
}

// The whole-product asm statements (prod_asm.h) against the column-block products of field29.h,
// bit for bit, on n pseudo-random operands per kind at their contracts' limb bounds (mul29 /
// sqr29: limbs < 2^30; mul29_sum2: a, c, d < 2^29, b < 2^31) -- every other thread's limbs all at
// the bound's maximum, the worst column sums.  mism[k] counts the mismatching threads of kind k
// (0 mul, 1 sqr, 2 sum2).
__global__ void __launch_bounds__(256) k_prod_asm_check(uint32_t n, uint32_t seed, uint32_t* mism) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t s = (t ^ seed) * 2654435761u + 0x9e3779b9u;
    auto rnd = [&](uint32_t bits) {
        s ^= s << 13;
        s ^= s >> 17;
        s ^= s << 5;
        const uint32_t m = (1u << bits) - 1;
        return (t & 1) ? m : (s * 2654435761u) & m;
    };
    F29 a, b, c, d;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        a.l[i] = rnd(30);
        b.l[i] = rnd(30);
    }
    const F29 m1 = mul29<FqP>(a, b), m2 = mul29_asm<FqP>(a, b);
    const F29 q1 = sqr29<FqP>(a), q2 = sqr29_asm<FqP>(a);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        a.l[i] = rnd(29);
        b.l[i] = rnd(31);
        c.l[i] = rnd(29);
        d.l[i] = rnd(29);
    }
    const F29 s1 = mul29_sum2<FqP>(a, b, c, d), s2 = mul29_sum2_asm<FqP>(a, b, c, d);
    uint32_t e0 = 0, e1 = 0, e2 = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        e0 |= m1.l[i] ^ m2.l[i];
        e1 |= q1.l[i] ^ q2.l[i];
        e2 |= s1.l[i] ^ s2.l[i];
    }
    if (e0) atomicAdd(mism + 0, 1u);
    if (e1) atomicAdd(mism + 1, 1u);
    if (e2) atomicAdd(mism + 2, 1u);
}

// The in-place forms (mul29_asm_ip: a = a b; mul29_sum2_asm_ip: c = a b + c d; tied read-write
// operands, the hot loop's register arrangement) against the same column-block products, on the
// operands k_prod_asm_check draws (same generator and order) at the out-of-place contracts' limb
// bounds -- prod_asm.h states no narrower contract for the in-place forms.  The operand a
// statement overwrites is copied first.  mism[k]: 0 mul, 1 sum2.
__global__ void __launch_bounds__(256) k_prod_asm_ip_check(uint32_t n, uint32_t seed, uint32_t* mism) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    uint32_t s = (t ^ seed) * 2654435761u + 0x9e3779b9u;
    auto rnd = [&](uint32_t bits) {
        s ^= s << 13;
        s ^= s >> 17;
        s ^= s << 5;
        const uint32_t m = (1u << bits) - 1;
        return (t & 1) ? m : (s * 2654435761u) & m;
    };
    F29 a, b, c, d;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        a.l[i] = rnd(30);
        b.l[i] = rnd(30);
    }
    const F29 m1 = mul29<FqP>(a, b);
    F29 m2 = a;
    mul29_asm_ip<FqP>(m2, b);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        a.l[i] = rnd(29);
        b.l[i] = rnd(31);
        c.l[i] = rnd(29);
        d.l[i] = rnd(29);
    }
    const F29 s1 = mul29_sum2<FqP>(a, b, c, d);
    F29 s2 = c;
    mul29_sum2_asm_ip<FqP>(a, b, s2, d);
    uint32_t e0 = 0, e1 = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        e0 |= m1.l[i] ^ m2.l[i];
        e1 |= s1.l[i] ^ s2.l[i];
    }
    if (e0) atomicAdd(mism + 0, 1u);
    if (e1) atomicAdd(mism + 1, 1u);
}

// One ec29.h formula per thread (eon_diag_ec29_op): thread t reads accumulator acc[t] (ld_raw29)
// and its argument -- an affine base as 18 limbs (x, y; read as they are, so y may be a lazy
// negation) or a second raw accumulator -- runs the formula once and stores the accumulator
// (st_raw29) and the formula's return value.  One kernel per formula, 64-thread blocks: each gets
// the register allocation it would get on its own, tied-operand asm products included.
enum : uint32_t {
    EC29_MADD = 0,
    EC29_MADD_UNCHECKED,
    EC29_MADD_NEGSUM,
    EC29_MADD_EXCEPTIONAL,
    EC29_DBL_AFFINE,
    EC29_DBL,
    EC29_ADD,
    EC29_ADD_ILP,
    EC29_DBL_ILP,
    EC29_ACC,
    EC29_ACC_ILP,
    EC29_TO_XYZZ,
    EC29_ROUNDTRIP,
    EC29_NEG_LAZY,
    EC29_X29_TO_XYZZ,
    EC29_OPS
};
// words of one argument: 18 (affine x, y), 36 (raw accumulator) or 0 (none)
constexpr uint32_t ec29_arg_words(uint32_t op) {
    return op <= EC29_DBL_AFFINE ? 18u
           : op == EC29_ADD || op == EC29_ADD_ILP || op == EC29_ACC || op == EC29_ACC_ILP ? 36u
                                                                                          : 0u;
}

__device__ __forceinline__ F29 ld_limbs29(const uint32_t* p) {
    F29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = p[i];
    pin29(r);
    return r;
}

__device__ __forceinline__ void st_words8(uint32_t* p, const Fq& a) {
#pragma unroll
    for (int i = 0; i < 8; i++) p[i] = a.v[i];
}

template <uint32_t OP>
__global__ void __launch_bounds__(64) k_ec29_op(const G1Raw29* acc, const uint32_t* arg, uint32_t n, G1Raw29* out,
                                                int32_t* code) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if constexpr (OP == EC29_TO_XYZZ || OP == EC29_X29_TO_XYZZ) {
        // the four canonical radix-2^32 coordinates in words 0..31, code = identity: of the raw
        // accumulator (raw29_to_xyzz), or of the loaded one and its flag (x29_to_xyzz)
        G1Xyzz r;
        if constexpr (OP == EC29_TO_XYZZ) {
            r = raw29_to_xyzz(acc + t);
        } else {
            G1X29 a;
            const bool a_inf = ld_raw29(acc + t, a);
            r = x29_to_xyzz(a, a_inf);
        }
        uint32_t* w = out[t].w;
        st_words8(w, r.X);
        st_words8(w + 8, r.Y);
        st_words8(w + 16, r.ZZ);
        st_words8(w + 24, r.ZZZ);
#pragma unroll
        for (int i = 32; i < 36; i++) w[i] = 0;
        code[t] = is_inf(r) ? 1 : 0;
    } else if constexpr (OP == EC29_ROUNDTRIP) {
        // to_fq261(to_fq256(c)) of each coordinate c as a 256-bit integer, words 0..31
        G1X29 a;
        ld_raw29(acc + t, a);
        uint32_t* w = out[t].w;
        st_words8(w, to_fq261(to_fq256(a.X)));
        st_words8(w + 8, to_fq261(to_fq256(a.Y)));
        st_words8(w + 16, to_fq261(to_fq256(a.ZZ)));
        st_words8(w + 24, to_fq261(to_fq256(a.ZZZ)));
#pragma unroll
        for (int i = 32; i < 36; i++) w[i] = 0;
        code[t] = 0;
    } else {
        G1X29 a;
        bool a_inf = false;
        int rc = 0;
        if constexpr (OP != EC29_DBL_AFFINE) a_inf = ld_raw29(acc + t, a);
        if constexpr (ec29_arg_words(OP) == 18) {
            const F29 x = ld_limbs29(arg + (uint64_t)t * 18), y = ld_limbs29(arg + (uint64_t)t * 18 + 9);
            if constexpr (OP == EC29_MADD) rc = madd29(a, x, y);
            if constexpr (OP == EC29_MADD_UNCHECKED) madd29_unchecked(a, x, y);
            if constexpr (OP == EC29_MADD_NEGSUM) madd29_negsum(a, x, y);
            if constexpr (OP == EC29_MADD_EXCEPTIONAL) rc = madd29_exceptional(a, x, y);
            if constexpr (OP == EC29_DBL_AFFINE) a = dbl29_affine(x, y);
        } else if constexpr (ec29_arg_words(OP) == 36) {
            G1X29 q;
            const bool q_inf = ld_raw29(reinterpret_cast<const G1Raw29*>(arg) + t, q);
            if constexpr (OP == EC29_ADD) rc = add29(a, q);
            if constexpr (OP == EC29_ADD_ILP) rc = add29_ilp(a, q);
            if constexpr (OP == EC29_ACC) acc29(a, a_inf, q, q_inf);
            if constexpr (OP == EC29_ACC_ILP) acc29_ilp(a, a_inf, q, q_inf);
            if constexpr (OP == EC29_ACC || OP == EC29_ACC_ILP) rc = a_inf;
        } else {
            if constexpr (OP == EC29_DBL) dbl29(a);
            if constexpr (OP == EC29_DBL_ILP) dbl29_ilp(a);
            if constexpr (OP == EC29_NEG_LAZY) {  // the piece loop's two lazy negations
                a.X = neg29_lazy<2>(a.X);
                a.ZZZ = neg29_lazy<3>(a.ZZZ);
            }
        }
        if ((OP == EC29_ACC || OP == EC29_ACC_ILP) && a_inf)
            st_raw29_inf(out + t);
        else
            st_raw29(out + t, a);
        code[t] = rc;
    }
}

template <uint32_t OP = 0>
void launch_ec29_op(uint32_t op, const G1Raw29* acc, const uint32_t* arg, uint32_t n, G1Raw29* out, int32_t* code,
                    hipStream_t st) {
    if constexpr (OP < EC29_OPS) {
        if (op == OP)
            hipLaunchKernelGGL(k_ec29_op<OP>, dim3((n + 63) / 64), dim3(64), 0, st, acc, arg, n, out, code);
        else
            launch_ec29_op<OP + 1>(op, acc, arg, n, out, code, st);
    }
}

// largest input of the stage diagnostics (2^24 pairs: 64 MiB per array)
constexpr uint64_t DIAG_MAX_N = 1ull << 24;
// and of the formula diagnostic (2^20 accumulators: 144 MiB per array)
constexpr uint64_t DIAG_EC29_MAX_N = 1ull << 20;

int finish(eon_ctx* ctx, const Status& s) {
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

}  // namespace

extern "C" int eon_diag_clock_probe(eon_ctx* ctx, uint32_t launches, uint32_t iters, eon_clock_probe* out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (!out) return Status::err(EON_E_ARG, "null argument");
        if (launches == 0 || launches > 100000 || iters == 0 || iters > (1u << 24))
            return Status::err(EON_E_ARG, "1 <= launches <= 1e5, 1 <= iters <= 2^24");
        DevBuf stamps, sink;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(stamps, (size_t)PROBE_BLOCKS * 2 * sizeof(uint64_t)));
        EON_HIP(ps.take(sink, 64));
        // the guard exists before either event is created, and destroys only those that were
        struct Ev {
            hipEvent_t a = nullptr, b = nullptr;
            ~Ev() {
                if (a) (void)hipEventDestroy(a);
                if (b) (void)hipEventDestroy(b);
            }
        } ev;
        EON_HIP(hipEventCreate(&ev.a));
        EON_HIP(hipEventCreate(&ev.b));
        hipEvent_t a = ev.a, b = ev.b;
        // one untimed launch, then `launches` back to back (the clock settles under the load)
        hipLaunchKernelGGL(k_clock_probe, dim3(PROBE_BLOCKS), dim3(PROBE_THREADS), 0, ctx->stream, iters, 0u,
                           stamps.as<uint64_t>(), sink.as<uint32_t>());
        EON_HIP(hipGetLastError());
        EON_HIP(hipEventRecord(a, ctx->stream));
        for (uint32_t k = 0; k < launches; k++)
            hipLaunchKernelGGL(k_clock_probe, dim3(PROBE_BLOCKS), dim3(PROBE_THREADS), 0, ctx->stream, iters, k + 1,
                               stamps.as<uint64_t>(), sink.as<uint32_t>());
        EON_HIP(hipGetLastError());
        EON_HIP(hipEventRecord(b, ctx->stream));
        std::vector<uint64_t> h((size_t)PROBE_BLOCKS * 2);
        EON_HIP(hipMemcpyAsync(h.data(), stamps.p, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        EON_HIP(hipEventElapsedTime(&ms, a, b));
        std::vector<double> mhz;
        mhz.reserve(PROBE_BLOCKS);
        for (uint32_t i = 0; i < PROBE_BLOCKS; i++)
            if (h[2 * i + 1]) mhz.push_back((double)h[2 * i] / (double)h[2 * i + 1] * 100.0);
        if (mhz.empty()) return Status::err(EON_E_DEVICE, "no clock stamps");
        std::sort(mhz.begin(), mhz.end());
        out->clock_mhz_median = mhz[mhz.size() / 2];
        out->clock_mhz_min = mhz.front();
        out->clock_mhz_max = mhz.back();
        out->ms_per_launch = ms / launches;
        out->products_per_s = (double)PROBE_BLOCKS * PROBE_THREADS * 2.0 * iters * launches / (ms * 1e-3);
        return Status::ok();
    }();
    return finish(ctx, s);
}

extern "C" int eon_diag_prod_asm_check(eon_ctx* ctx, uint32_t n, uint32_t seed, uint32_t mismatches[3]) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (!mismatches) return Status::err(EON_E_ARG, "null argument");
        DevBuf cnt;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(cnt, 64));
        EON_HIP(hipMemsetAsync(cnt.p, 0, 16, ctx->stream));
        if (n) hipLaunchKernelGGL(k_prod_asm_check, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, seed,
                                  cnt.as<uint32_t>());
        EON_HIP(hipGetLastError());
        EON_HIP(hipMemcpyAsync(mismatches, cnt.p, 12, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}

extern "C" int eon_diag_prod_asm_ip_check(eon_ctx* ctx, uint32_t n, uint32_t seed, uint32_t mismatches[2]) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (!mismatches) return Status::err(EON_E_ARG, "null argument");
        DevBuf cnt;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(cnt, 64));
        EON_HIP(hipMemsetAsync(cnt.p, 0, 16, ctx->stream));
        if (n) hipLaunchKernelGGL(k_prod_asm_ip_check, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, seed,
                                  cnt.as<uint32_t>());
        EON_HIP(hipGetLastError());
        EON_HIP(hipMemcpyAsync(mismatches, cnt.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}

extern "C" int eon_diag_radix_sort_pairs(eon_ctx* ctx, const uint32_t* keys, const uint32_t* vals, uint64_t n,
                                         uint32_t bits, uint32_t* keys_out, uint32_t* vals_out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (n > DIAG_MAX_N) return Status::err(EON_E_ARG, "at most 2^24 pairs");
        if (bits > 32) return Status::err(EON_E_ARG, "at most 32 key bits");
        if (n && (!keys || !vals || !keys_out || !vals_out)) return Status::err(EON_E_ARG, "null argument");
        if (n == 0) return Status::ok();
        DevBuf k, v, k2, v2, temp;
        PoolScope ps(ctx->pool, ctx->stream);
        for (DevBuf* b : {&k, &v, &k2, &v2}) EON_HIP(ps.take(*b, n * 4));
        EON_HIP(ps.take(temp, radix_sort_temp_bytes(n, bits)));
        EON_HIP(hipMemcpyAsync(k.p, keys, n * 4, hipMemcpyHostToDevice, ctx->stream));
        EON_HIP(hipMemcpyAsync(v.p, vals, n * 4, hipMemcpyHostToDevice, ctx->stream));
        EON_HIP(radix_sort_pairs(temp.p, k.as<uint32_t>(), k2.as<uint32_t>(), v.as<uint32_t>(), v2.as<uint32_t>(), n,
                                 bits, ctx->stream));
        EON_HIP(hipMemcpyAsync(keys_out, k2.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipMemcpyAsync(vals_out, v2.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}

extern "C" int eon_diag_exclusive_scan_u32(eon_ctx* ctx, const uint32_t* in, uint64_t n, uint32_t* out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (n > DIAG_MAX_N) return Status::err(EON_E_ARG, "at most 2^24 elements");
        if (n && (!in || !out)) return Status::err(EON_E_ARG, "null argument");
        if (n == 0) return Status::ok();
        DevBuf a, b, temp;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(a, n * 4));
        EON_HIP(ps.take(b, n * 4));
        EON_HIP(ps.take(temp, exclusive_scan_temp_bytes(n)));
        EON_HIP(hipMemcpyAsync(a.p, in, n * 4, hipMemcpyHostToDevice, ctx->stream));
        EON_HIP(exclusive_scan_u32(temp.p, a.as<uint32_t>(), b.as<uint32_t>(), n, ctx->stream));
        EON_HIP(hipMemcpyAsync(out, b.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}

extern "C" int eon_diag_scan_chunk_counts(eon_ctx* ctx, const uint32_t* start, uint32_t nb, uint32_t log_chunk,
                                          uint32_t* out, uint32_t* max_out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (nb > DIAG_MAX_N) return Status::err(EON_E_ARG, "at most 2^24 buckets");
        if (log_chunk > 31) return Status::err(EON_E_ARG, "log_chunk < 32");
        if (!start || !out || !max_out) return Status::err(EON_E_ARG, "null argument");
        const uint64_t m = (uint64_t)nb + 1;
        DevBuf a, b, temp, mx;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(a, m * 4));
        EON_HIP(ps.take(b, m * 4));
        EON_HIP(ps.take(temp, exclusive_scan_temp_bytes(m)));
        EON_HIP(ps.take(mx, 64));
        EON_HIP(hipMemcpyAsync(a.p, start, m * 4, hipMemcpyHostToDevice, ctx->stream));
        EON_HIP(hipMemsetAsync(mx.p, 0, 16, ctx->stream));  // as batch_sort zeroes its slot (msm_digits.hip)
        EON_HIP(exclusive_scan_chunk_counts(temp.p, a.as<uint32_t>(), nb, log_chunk, b.as<uint32_t>(),
                                            mx.as<uint32_t>(), ctx->stream));
        EON_HIP(hipMemcpyAsync(out, b.p, m * 4, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipMemcpyAsync(max_out, mx.p, 4, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}

extern "C" int eon_diag_ec29_op(eon_ctx* ctx, uint32_t op, const uint32_t* acc, const uint32_t* arg, uint64_t n,
                                uint32_t* acc_out, int32_t* code_out) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (op >= EC29_OPS) return Status::err(EON_E_ARG, "unknown ec29 op");
        if (n > DIAG_EC29_MAX_N) return Status::err(EON_E_ARG, "at most 2^20 accumulators");
        const uint32_t aw = ec29_arg_words(op);
        const bool uses_acc = op != EC29_DBL_AFFINE;
        if (n && ((uses_acc && !acc) || (aw && !arg) || !acc_out || !code_out))
            return Status::err(EON_E_ARG, "null argument");
        if (n == 0) return Status::ok();
        DevBuf a, b, o, c;
        PoolScope ps(ctx->pool, ctx->stream);
        EON_HIP(ps.take(a, n * sizeof(G1Raw29)));
        EON_HIP(ps.take(b, n * sizeof(G1Raw29)));
        EON_HIP(ps.take(o, n * sizeof(G1Raw29)));
        EON_HIP(ps.take(c, n * sizeof(int32_t)));
        if (uses_acc) EON_HIP(hipMemcpyAsync(a.p, acc, n * sizeof(G1Raw29), hipMemcpyHostToDevice, ctx->stream));
        if (aw) EON_HIP(hipMemcpyAsync(b.p, arg, n * aw * 4, hipMemcpyHostToDevice, ctx->stream));
        launch_ec29_op(op, a.as<G1Raw29>(), b.as<uint32_t>(), (uint32_t)n, o.as<G1Raw29>(), c.as<int32_t>(),
                       ctx->stream);
        EON_HIP(hipGetLastError());
        EON_HIP(hipMemcpyAsync(acc_out, o.p, n * sizeof(G1Raw29), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipMemcpyAsync(code_out, c.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    }();
    return finish(ctx, s);
}
