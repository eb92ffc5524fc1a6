// See verifier.h.  Line numbers are eon-uni-stark/src/verifier.rs unless another file is named.
#include "verifier.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <thread>

#include "verify_host.h"

namespace eon_host {

namespace {

void reject(Prepared& p, int v, const std::string& why) {
    p.out.verdict = v;
    p.out.detail = why;
    p.done = true;
}

ProgShape prog_shape(eon_ctx* ctx, const eon_air_program* prog) {
    if (!prog) throw Error(EON_E_ARG, "null program or proof");
    eon_air_program_stats st{};
    check(ctx, eon_air_program_info(prog, &st), "eon_air_program_info");
    return {st.width,
            st.num_public_values,
            eon_air_program_preprocessed_width(prog),
            eon_air_program_permutation_width(prog),
            eon_air_program_num_challenges(prog),
            eon_air_program_log_quotient_degree(prog, 0)};  // :296-304
}

// batched mode: delta^i C_i and delta^i W_i of the K claims, one variable-base column MSM
void scale_claims(eon_ctx* ctx, Prepared& p) {
    const size_t K = p.vs.size(), cols = 2 * K, n_pts = p.pts.size();
    std::vector<eon_g1_affine> scaled(cols);
    eon_msm_bases* bases = nullptr;
    check(ctx, eon_msm_bases_create(ctx, p.pts.data(), n_pts, 0, &bases), "eon_msm_bases_create");
    const int mrc = eon_msm_g1_columns(ctx, bases, p.scal.data(), n_pts, (uint32_t)cols, scaled.data());
    eon_msm_bases_destroy(bases);
    check(ctx, mrc, "eon_msm_g1_columns");
    p.cs.assign(scaled.begin(), scaled.begin() + K);
    p.ws.assign(scaled.begin() + K, scaled.end());
}

// one proof's verify_batch alone: 1 / 0, or EON_E_ARG with the library's message in *why
int openings_alone(KzgPcs& pcs, const Prepared& p, std::string* why) {
    eon_ctx* ctx = pcs.ctx();
    int ok = 0;
    const int rc = eon_kzg_verify_batch(ctx, p.cs.data(), p.ws.data(), p.vs.data(), p.zs.data(), p.cs.size(),
                                        &pcs.g2_alpha(), &ok);
    // a commitment or witness that is no curve point, or an opened value that is no canonical
    // Fr, cannot come out of the reference's deserialisation: not an opening
    if (rc == EON_E_ARG) {
        const char* msg = eon_last_error(ctx);
        *why = msg ? msg : "invalid argument";
        return EON_E_ARG;
    }
    check(ctx, rc, "eon_kzg_verify_batch");
    return ok;
}

// ---- phase 2: the openings of every live proof, one segment each --------------------------------
void check_openings(KzgPcs& pcs, const std::vector<Prepared*>& live) {
    eon_ctx* ctx = pcs.ctx();
    if (live.empty()) return;
    for (Prepared* p : live)
        if (p->batched) scale_claims(ctx, *p);
    std::vector<int> status(live.size(), 0);
    std::vector<std::string> why(live.size());
    if (live.size() == 1) {
        status[0] = openings_alone(pcs, *live[0], &why[0]);
    } else {
        std::vector<eon_g1_affine> cs, ws;
        std::vector<eon_fr> vs, zs;
        std::vector<uint64_t> seg(1, 0);
        for (const Prepared* p : live) {
            cs.insert(cs.end(), p->cs.begin(), p->cs.end());
            ws.insert(ws.end(), p->ws.begin(), p->ws.end());
            vs.insert(vs.end(), p->vs.begin(), p->vs.end());
            zs.insert(zs.end(), p->zs.begin(), p->zs.end());
            seg.push_back(cs.size());
        }
        check(ctx,
              eon_kzg_verify_batch_many(ctx, cs.data(), ws.data(), vs.data(), zs.data(), seg.data(),
                                        (uint32_t)live.size(), &pcs.g2_alpha(), status.data()),
              "eon_kzg_verify_batch_many");
        // the message of a malformed segment is the single call's on that segment
        for (size_t i = 0; i < live.size(); i++)
            if (status[i] == EON_E_ARG && openings_alone(pcs, *live[i], &why[i]) != EON_E_ARG)
                throw Error(EON_E_DEVICE, "eon_kzg_verify_batch_many and eon_kzg_verify_batch disagree on a segment");
    }
    for (size_t i = 0; i < live.size(); i++) {
        Prepared& p = *live[i];
        if (status[i] == EON_E_ARG)
            reject(p, EON_VERIFY_INVALID_OPENING_ARGUMENT, "malformed opening: " + why[i]);
        else if (!status[i])
            reject(p, EON_VERIFY_INVALID_OPENING_ARGUMENT,
                   std::string("KzgError::ProofShapeMismatch: the ") + (p.batched ? "weighted" : "batched") +
                       " pairing check of " + std::to_string(p.cs.size()) + (p.batched ? " batched" : "") +
                       " openings failed");
    }
}

// ---- phase 3: constraints(zeta) / Z_H(zeta) against quotient(zeta) for the proofs that passed ---
// `ins[p.index]` are the inputs proof p was prepared from; `many`: the messages name the index.
void check_ood(KzgPcs& pcs, const ProgShape& ps, const VerifyInputs* ins, const std::vector<Prepared*>& live,
               bool many) {
    eon_ctx* ctx = pcs.ctx();
    if (live.empty()) return;
    for (const Prepared* p : live)
        if (p->zeta_on_domain)
            throw Error(EON_E_ARG, (many ? "proof " + std::to_string(p->index) + ": " : std::string()) +
                                       "zeta lies on the trace domain: the selectors at zeta are undefined");
    const uint32_t width = ps.width, perm_width = ps.perm_width, pre_width = live[0]->pre_width;
    const size_t n = live.size(), stride = live[0]->rows.size();
    const uint32_t n_ch = (uint32_t)live[0]->out.challenges.size();
    std::vector<eon_fr> host(n * stride), ch(std::max<size_t>(n * n_ch, 1)), pub(std::max<size_t>(n * ps.n_public, 1));
    std::vector<eon_fr> alpha(n), zeta(n), res(2 * n);
    std::vector<uint32_t> log_n(n);
    for (size_t i = 0; i < n; i++) {
        const Prepared& p = *live[i];
        std::memcpy(host.data() + i * stride, p.rows.data(), stride * sizeof(eon_fr));
        for (uint32_t j = 0; j < n_ch; j++) ch[i * n_ch + j] = p.out.challenges[j].abi();
        for (uint32_t j = 0; j < ps.n_public; j++) pub[i * ps.n_public + j] = ins[p.index].publics[j];
        alpha[i] = p.out.alpha.abi();
        zeta[i] = p.out.zeta.abi();
        log_n[i] = p.log_n;
    }
    // the opened rows on the device: local | next | pre_local | pre_next | perm_local | perm_next
    DeviceBuffer rows(host.size() * sizeof(eon_fr));
    hipStream_t stream = static_cast<hipStream_t>(eon_ctx_stream(ctx));
    if (hipMemcpyAsync(rows.get(), host.data(), host.size() * sizeof(eon_fr), hipMemcpyHostToDevice, stream) !=
            hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        throw Error(EON_E_DEVICE, "copying the opened values to the device failed");
    const eon_fr* d = rows.as<eon_fr>();
    if (n == 1) {
        const eon_fr* d_pre = d + 2 * width;
        const eon_fr* d_perm = d_pre + 2 * pre_width;
        try {
            check(ctx,
                  eon_air_eval_at_point_dev(ctx, ins[live[0]->index].prog, log_n[0], &zeta[0], &alpha[0], d, d + width,
                                            pre_width ? d_pre : nullptr, pre_width ? d_pre + pre_width : nullptr,
                                            perm_width ? d_perm : nullptr, perm_width ? d_perm + perm_width : nullptr,
                                            ins[live[0]->index].publics, ps.n_public, ch.data(), n_ch, res.data()),
                  "eon_air_eval_at_point_dev");
        } catch (const Error& e) {
            if (!many) throw;
            throw Error(e.code, "proof " + std::to_string(live[0]->index) + ": " + e.what());
        }
    } else {
        const int rc = eon_air_eval_at_points_dev(ctx, ins[live[0]->index].prog, (uint32_t)n, log_n.data(),
                                                  zeta.data(), alpha.data(), d, stride, pub.data(), ch.data(), n_ch,
                                                  res.data());
        if (rc != EON_OK) {
            // the library names the point among those it was given: name the caller's proof instead
            const char* raw = eon_last_error(ctx);
            std::string msg = raw ? raw : "error";
            size_t j = 0;
            int used = 0;
            if (sscanf(msg.c_str(), "point %zu:%n", &j, &used) == 1 && used > 0 && j < n)
                msg = "proof " + std::to_string(live[j]->index) + ":" + msg.substr((size_t)used);
            throw Error(rc, "eon_air_eval_at_points_dev: " + msg);
        }
    }
    for (size_t i = 0; i < n; i++)
        if (!(Fr::from_abi(res[2 * i + 1]) == live[i]->quotient))  // :155
            reject(*live[i], EON_VERIFY_OOD_EVALUATION_MISMATCH,
                   "constraints(zeta) / Z_H(zeta) differs from quotient(zeta)");
}

}  // namespace

VerifyOutcome verify(KzgPcs& pcs, const VerifyInputs& in, DuplexChallenger* challenger) {
    const ProgShape ps = prog_shape(pcs.ctx(), in.prog);
    Prepared p = prepare(pcs.max_degree(), ps, in, challenger);
    std::vector<Prepared*> live;
    if (!p.done) live.push_back(&p);
    check_openings(pcs, live);
    if (p.done) live.clear();
    check_ood(pcs, ps, &in, live, false);
    return p.out;
}

std::vector<VerifyOutcome> verify_many(KzgPcs& pcs, const std::vector<VerifyInputs>& ins,
                                       const std::vector<DuplexChallenger*>& challengers) {
    const size_t n = ins.size();
    if (n == 0) return {};
    if (!challengers.empty() && challengers.size() != n) throw Error(EON_E_ARG, "one challenger per proof, or none");
    for (size_t i = 0; i < n; i++)
        if (ins[i].prog != ins[0].prog) throw Error(EON_E_ARG, "proof " + std::to_string(i) + ": another AIR program");
    const ProgShape ps = prog_shape(pcs.ctx(), ins[0].prog);
    // phase 1 on min(n, 8) threads (a constant, not the machine's CPU count): thread t prepares
    // proofs t, t + T, ...; the proofs share nothing but read-only inputs
    std::vector<Prepared> prepared(n);
    std::vector<std::exception_ptr> failed(n);
    const size_t T = std::min<size_t>(n, VERIFY_PREPARE_THREADS);
    auto work = [&](size_t t) {
        for (size_t i = t; i < n; i += T) {
            try {
                prepared[i] = prepare(pcs.max_degree(), ps, ins[i], challengers.empty() ? nullptr : challengers[i]);
                prepared[i].index = i;
            } catch (...) {
                failed[i] = std::current_exception();
            }
        }
    };
    if (T == 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (size_t t = 0; t < T; t++) pool.emplace_back(work, t);
        for (std::thread& th : pool) th.join();
    }
    for (size_t i = 0; i < n; i++) {
        if (!failed[i]) continue;
        try {
            std::rethrow_exception(failed[i]);
        } catch (const Error& e) {
            throw Error(e.code, "proof " + std::to_string(i) + ": " + e.what());
        }
    }
    std::vector<Prepared*> live;
    for (Prepared& p : prepared)
        if (!p.done) live.push_back(&p);
    check_openings(pcs, live);
    live.erase(std::remove_if(live.begin(), live.end(), [](const Prepared* p) { return p->done; }), live.end());
    check_ood(pcs, ps, ins.data(), live, true);
    std::vector<VerifyOutcome> out;
    for (Prepared& p : prepared) out.push_back(std::move(p.out));
    return out;
}

}  // namespace eon_host

