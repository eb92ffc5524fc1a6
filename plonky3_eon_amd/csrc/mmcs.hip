// KzgMmcs (kzg/src/mmcs.rs): Mmcs<Fr> over the KZG SRS.  Matrices of mixed heights, every column a
// polynomial in coefficient form; a query index opens row-point z = Fr::new(local_index) of every
// matrix.  The reference's open_batch runs one quotient_and_eval and one commit_column per
// (index, matrix, column) (mmcs.rs:196-236); here the distinct (matrix, local_index) pairs of a whole
// query batch are divided in one pass (kzg.hip: quotient_and_eval_multi) into quotients laid side by
// side, and ONE column MSM over srs[0..height-1) produces all their witnesses.
#include "context.h"
#include "msm.h"

#include <algorithm>
#include <cstdlib>
#include <limits>

using namespace eon;

namespace {

constexpr uint64_t GROUP_BYTES = 1ull << 30;  // quotient scratch of one group of distinct points
constexpr uint64_t GROUP_COLS = 1ull << 20;   // MSM columns of one group (its results: 160 B each)

// next_power_of_two(x).trailing_zeros() (0 and 1 -> 0); 64 past 2^63, where the reference overflows
uint32_t log2_ceil_u64(uint64_t x) {
    if (x <= 1) return 0;
    return 64 - (uint32_t)__builtin_clzll(x - 1);
}

eon_fr fr_to_abi(const Fr& x) {
    eon_fr r;
    for (int i = 0; i < 4; i++) r.l[i] = (uint64_t)x.v[2 * i] | (uint64_t)x.v[2 * i + 1] << 32;
    return r;
}

eon_g1_affine g1_to_abi(const G1Affine& a) {
    eon_g1_affine r;
    for (int i = 0; i < 4; i++) {
        r.x[i] = (uint64_t)a.x.v[2 * i] | (uint64_t)a.x.v[2 * i + 1] << 32;
        r.y[i] = (uint64_t)a.y.v[2 * i] | (uint64_t)a.y.v[2 * i + 1] << 32;
    }
    return r;
}

Status open_matrix(eon_ctx* ctx, const eon_msm_bases* srs, const eon_mmcs_matrix& m, uint64_t max_height,
                   const uint64_t* indices, uint32_t nidx, uint64_t W, uint64_t off, eon_fr* values,
                   eon_g1_affine* witnesses) {
    const uint64_t h = m.height;
    const uint32_t w = m.width;
    // the distinct local indices of the query batch, and each query's slot among them
    std::vector<uint64_t> local(nidx), distinct;
    for (uint32_t q = 0; q < nidx; q++) local[q] = eon_kzg_mmcs_local_index(max_height, h, indices[q]);
    distinct = local;
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    std::vector<uint32_t> slot(nidx);
    for (uint32_t q = 0; q < nidx; q++)
        slot[q] = (uint32_t)(std::lower_bound(distinct.begin(), distinct.end(), local[q]) - distinct.begin());
    const uint64_t nd = distinct.size();
    // groups of distinct points: quotient scratch <= GROUP_BYTES (a single point above it still runs)
    const uint64_t point_bytes = (h - 1) * w * sizeof(Fr);
    const char* cap_env = getenv("EON_MMCS_GROUP_BYTES");  // tests: several groups at small shapes
    const uint64_t cap = cap_env && *cap_env ? strtoull(cap_env, nullptr, 10) : GROUP_BYTES;
    uint64_t per = point_bytes ? std::max<uint64_t>(1, cap / point_bytes) : nd;
    per = std::min<uint64_t>({per, nd, std::max<uint64_t>(1, GROUP_COLS / w)});
    if ((h - 1) > std::numeric_limits<uint64_t>::max() / sizeof(Fr) / w / per)
        return Status::err(EON_E_SHAPE, "matrix too large");
    DevBuf dq, dv;
    PoolScope ps(ctx->pool, ctx->stream);
    if (point_bytes) EON_HIP(ps.take(dq, per * point_bytes));
    EON_HIP(ps.take(dv, per * w * sizeof(Fr)));
    std::vector<Fr> zs(per), hv(per * w);
    std::vector<G1Affine> hw(per * w);
    const Fr* c = reinterpret_cast<const Fr*>(m.coeffs);
    for (uint64_t d0 = 0; d0 < nd; d0 += per) {
        const uint32_t np = (uint32_t)std::min<uint64_t>(per, nd - d0);
        for (uint32_t p = 0; p < np; p++) zs[p] = from_u64<FrP>(distinct[d0 + p]);  // Fr::new(local_index)
        EON_TRY(quotient_and_eval_multi(ctx, c, h, w, zs.data(), np, dq.as<Fr>(), dv.as<Fr>()));
        // commit_column of every quotient over srs[0..h-1); h == 1: empty quotients, identity witnesses
        EON_TRY(msm_run_columns(ctx, srs, dq.as<Fr>(), h - 1, np * w, hw.data(), nullptr));
        EON_HIP(hipMemcpyAsync(hv.data(), dv.p, (size_t)np * w * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        for (uint32_t q = 0; q < nidx; q++) {
            if (slot[q] < d0 || slot[q] >= d0 + np) continue;
            const uint64_t p = slot[q] - d0;
            for (uint32_t j = 0; j < w; j++) {
                values[q * W + off + j] = fr_to_abi(hv[p * w + j]);
                witnesses[q * W + off + j] = g1_to_abi(hw[p * w + j]);
            }
        }
    }
    return Status::ok();
}

}  // namespace

extern "C" {

uint64_t eon_kzg_mmcs_local_index(uint64_t max_height, uint64_t height, uint64_t index) {
    if (height == 0) return UINT64_MAX;
    const uint32_t log2_max = log2_ceil_u64(max_height), log2_h = log2_ceil_u64(height);
    if (log2_max >= log2_h) {
        const uint32_t sh = log2_max - log2_h;
        index = sh >= 64 ? 0 : index >> sh;
    }
    return index % height;
}

int eon_kzg_mmcs_open_dev(eon_ctx* ctx, const eon_msm_bases* srs, const eon_mmcs_matrix* mats, uint32_t nmats,
                          const uint64_t* indices, uint32_t nidx, eon_fr* values, eon_g1_affine* witnesses) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (!srs || (nmats && !mats) || (nidx && !indices)) return Status::err(EON_E_ARG, "null argument");
        uint64_t W = 0, max_height = 0;
        for (uint32_t m = 0; m < nmats; m++) {
            if (mats[m].height == 0) return Status::err(EON_E_SHAPE, "matrix of height 0 (the reference panics)");
            // ensure_supported(height - 1) against the SRS's max_degree = len - 1 (kzg/src/params.rs:164-173)
            if (mats[m].height > eon_msm_bases_len(srs))
                return Status::err(EON_E_DEGREE_TOO_LARGE, "matrix " + std::to_string(m) + ": degree " +
                                                               std::to_string(mats[m].height - 1) +
                                                               " exceeds the SRS");
            if (mats[m].width && !mats[m].coeffs) return Status::err(EON_E_ARG, "null matrix");
            W += mats[m].width;
            max_height = std::max(max_height, mats[m].height);
        }
        if (nidx && W && (!values || !witnesses)) return Status::err(EON_E_ARG, "null argument");
        if (nidx == 0 || W == 0) return Status::ok();
        uint64_t off = 0;
        for (uint32_t m = 0; m < nmats; m++) {
            if (mats[m].width)
                EON_TRY(open_matrix(ctx, srs, mats[m], max_height, indices, nidx, W, off, values, witnesses));
            off += mats[m].width;
        }
        return Status::ok();
    }();
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

int eon_kzg_mmcs_verify_batch(eon_ctx* ctx, const eon_g1_affine* commitments, const uint64_t* heights,
                              const uint32_t* widths, uint32_t nmats, uint64_t index, const eon_fr* values,
                              const eon_g1_affine* witnesses, uint64_t max_degree, const eon_g2_affine* g2_alpha,
                              int* ok) {
    if (!ctx) return EON_E_ARG;
    std::vector<eon_fr> points;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        Status s = [&]() -> Status {
            if (!ok || !g2_alpha || (nmats && (!heights || !widths))) return Status::err(EON_E_ARG, "null argument");
            *ok = 0;
            uint64_t max_height = 0;
            for (uint32_t m = 0; m < nmats; m++) max_height = std::max(max_height, heights[m]);
            for (uint32_t m = 0; m < nmats; m++) {
                // ensure_supported(height.saturating_sub(1)) (mmcs.rs:269-270), then the index mapping
                if (heights[m] && heights[m] - 1 > max_degree)
                    return Status::err(EON_E_DEGREE_TOO_LARGE, "matrix " + std::to_string(m) + ": degree " +
                                                                   std::to_string(heights[m] - 1) + " exceeds " +
                                                                   std::to_string(max_degree));
                if (heights[m] == 0) return Status::err(EON_E_SHAPE, "matrix of height 0 (the reference panics)");
                const eon_fr z =
                    fr_to_abi(from_u64<FrP>(eon_kzg_mmcs_local_index(max_height, heights[m], index)));
                points.insert(points.end(), widths[m], z);
            }
            if (!points.empty() && (!commitments || !values || !witnesses))
                return Status::err(EON_E_ARG, "null argument");
            return Status::ok();
        }();
        if (s.bad()) {
            ctx->last_error = s.msg;
            return s.code;
        }
    }
    // verify_batch(&all_openings, &self.params) (mmcs.rs:293; kzg/src/util.rs:245-292)
    return eon_kzg_verify_batch(ctx, commitments, witnesses, values, points.data(), points.size(), g2_alpha, ok);
}

}  // extern "C"
