// See verifier.h.  Line numbers are eon-uni-stark/src/verifier.rs unless another file is named.
#include "verifier.h"

#include <hip/hip_runtime_api.h>

#include <cstring>

#include "verify_host.h"

namespace eon_host {

namespace {

VerifyOutcome verdict(VerifyOutcome o, int v, const std::string& why) {
    o.verdict = v;
    o.detail = why;
    return o;
}

}  // namespace

VerifyOutcome verify(KzgPcs& pcs, const VerifyInputs& in, DuplexChallenger* challenger) {
    eon_ctx* ctx = pcs.ctx();
    if (!in.prog || !in.proof) throw Error(EON_E_ARG, "null program or proof");
    if (in.n_public && !in.publics) throw Error(EON_E_ARG, "null public values");
    const eon_proof_lk& lk = *in.proof;
    const eon_proof_pp& pp = lk.pp;
    const eon_proof& b = pp.base;
    if (!b.trace_commit || !b.quotient_commit || !b.trace_opened || !b.trace_witnesses || !b.quotient_opened ||
        !b.quotient_witnesses)
        throw Error(EON_E_ARG, "null trace or quotient arrays in the proof");
    eon_air_program_stats st{};
    check(ctx, eon_air_program_info(in.prog, &st), "eon_air_program_info");
    if (in.n_public != st.num_public_values)
        throw Error(EON_E_SHAPE, "public value count differs from the program's");
    const uint32_t width = st.width;
    const uint32_t prog_pre_width = eon_air_program_preprocessed_width(in.prog);
    const uint32_t perm_width = eon_air_program_permutation_width(in.prog);
    const uint32_t n_challenges = eon_air_program_num_challenges(in.prog);
    const uint32_t log_qd = eon_air_program_log_quotient_degree(in.prog, 0);  // :296-304
    const uint32_t num_chunks = 1u << log_qd;
    const uint32_t log_n = b.degree_bits;
    if (log_n + log_qd > Fr::TWO_ADICITY)  // the reference's two_adic_generator panics
        throw Error(EON_E_SHAPE, "degree_bits " + std::to_string(log_n) + " + log_quotient_degree exceeds the field's "
                                 "two-adicity");
    VerifyOutcome out;

    // ---- 1. shapes ------------------------------------------------------------------------------
    // process_preprocessed_trace (:165-225): the expected width is the key's, else the AIR's; the
    // proof carries preprocessed openings exactly when it is nonzero; a width needs a key and a key's
    // width is the width.  (The array widths themselves are the caller's: C arrays carry no length.)
    const bool has_vk = in.vk_commitment != nullptr;
    const uint32_t pre_width = has_vk ? in.vk_width : prog_pre_width;
    const bool proof_has_pre = pp.preprocessed_opened != nullptr;
    if ((pre_width > 0) != proof_has_pre)
        return verdict(out, EON_VERIFY_INVALID_PROOF_SHAPE,
                       "the verifier expects " + std::to_string(pre_width) + " preprocessed columns and the proof " +
                           (proof_has_pre ? "opens some" : "opens none"));
    if (pre_width > 0 && !has_vk)
        return verdict(out, EON_VERIFY_INVALID_PROOF_SHAPE,
                       "the AIR has preprocessed columns but no verifier key was given");
    if (pre_width > 0 && !pp.preprocessed_witnesses)
        return verdict(out, EON_VERIFY_INVALID_PROOF_SHAPE, "preprocessed openings without witnesses");
    // the program reads exactly its own preprocessed columns (the reference's AIR would index past
    // the opened row, or ignore it)
    if (pre_width != prog_pre_width)
        return verdict(out, EON_VERIFY_INVALID_PROOF_SHAPE,
                       "the verifier key's width " + std::to_string(pre_width) + " differs from the AIR's " +
                           std::to_string(prog_pre_width));
    if (has_vk && pre_width > 0 && in.vk_degree_bits != log_n)  // :272-277
        return verdict(out, EON_VERIFY_INVALID_PROOF_SHAPE,
                       "the verifier key's degree_bits " + std::to_string(in.vk_degree_bits) +
                           " differs from the proof's " + std::to_string(log_n));
    // :330-352: the permutation commitment and both opened rows, all or none; and all exactly when
    // the program has lookups
    const bool has_perm_commit = lk.permutation_commit != nullptr;
    const bool has_perm_opened = lk.permutation_opened != nullptr;
    if (has_perm_commit != has_perm_opened || (has_perm_commit && !lk.permutation_witnesses))
        return verdict(out, EON_VERIFY_INVALID_PROOF_SHAPE, "permutation commitment and openings must come together");
    if (has_perm_commit != (perm_width > 0))
        return verdict(out, EON_VERIFY_INVALID_PROOF_SHAPE,
                       perm_width > 0 ? "the AIR has lookups but the proof has no permutation part"
                                      : "the proof has a permutation part but the AIR has no lookups");
    // the given challenges are the program's (after the shapes: a proof without its permutation part
    // is a verdict, whatever came with it)
    if (!challenger && in.n_challenges != n_challenges)
        throw Error(EON_E_SHAPE, "challenge count differs from the program's");
    if (!challenger && n_challenges && !in.challenges) throw Error(EON_E_ARG, "null permutation challenges");

    // ---- 2. the transcript (:355-397) -----------------------------------------------------------
    out.alpha = in.alpha;
    out.zeta = in.zeta;
    out.challenges.resize(has_perm_commit ? n_challenges : 0);
    if (challenger) {
        challenger->observe(fr_from_u64(log_n));      // degree_bits
        challenger->observe(fr_from_u64(log_n));      // degree_bits - is_zk
        challenger->observe(fr_from_u64(pre_width));  // preprocessed width
        challenger->observe_g1(b.trace_commit, width);
        if (pre_width > 0) challenger->observe_g1(in.vk_commitment, pre_width);  // the key's, never the proof's
        for (uint32_t i = 0; i < in.n_public; i++) {
            const Fr v = Fr::from_abi(in.publics[i]);
            if (!fr_is_canonical(v)) throw Error(EON_E_ARG, "public value is not a canonical Fr");
            challenger->observe(v);
        }
        if (has_perm_commit) {
            for (auto& c : out.challenges) c = challenger->sample();
            challenger->observe_g1(lk.permutation_commit, perm_width);
        }
        out.alpha = challenger->sample();
        challenger->observe_g1(b.quotient_commit, num_chunks);
        out.zeta = challenger->sample();
    } else {
        for (uint32_t i = 0; i < (uint32_t)out.challenges.size(); i++) out.challenges[i] = Fr::from_abi(in.challenges[i]);
        if (!fr_is_canonical(out.alpha) || !fr_is_canonical(out.zeta))
            throw Error(EON_E_ARG, "alpha or zeta is not a canonical Fr");
    }
    const Fr zeta = out.zeta;
    const Fr zeta_next = pcs.natural_domain_for_degree(1ull << log_n).next_point(zeta);

    // ---- 3. KzgPcs::verify (kzg/src/pcs.rs:337-401) ---------------------------------------------
    // ensure_supported per domain: the trace domain and the chunk domains all have 2^log_n points
    try {
        pcs.ensure_supported((1ull << log_n) - 1);
    } catch (const Error& e) {
        if (e.code != EON_E_DEGREE_TOO_LARGE) throw;
        return verdict(out, EON_VERIFY_INVALID_OPENING_ARGUMENT, std::string("KzgError::DegreeTooLarge: ") + e.what());
    }
    {
        // the reference's round order: trace at {zeta, zeta h}, permutation at {zeta, zeta h}, quotient
        // chunks at {zeta}, preprocessed at {zeta, zeta h} (:415-471)
        std::vector<eon_g1_affine> cs, ws;
        std::vector<eon_fr> vs, zs;
        auto matrix = [&](const eon_g1_affine* commit, const eon_fr* opened, const eon_g1_affine* wit, uint32_t w) {
            const Fr pts[2] = {zeta, zeta_next};
            for (int p = 0; p < 2; p++)
                for (uint32_t c = 0; c < w; c++) {
                    cs.push_back(commit[c]);
                    ws.push_back(wit[(size_t)p * w + c]);
                    vs.push_back(opened[(size_t)p * w + c]);
                    zs.push_back(pts[p].abi());
                }
        };
        matrix(b.trace_commit, b.trace_opened, b.trace_witnesses, width);
        if (has_perm_commit) matrix(lk.permutation_commit, lk.permutation_opened, lk.permutation_witnesses, perm_width);
        for (uint32_t c = 0; c < num_chunks; c++) {
            cs.push_back(b.quotient_commit[c]);
            ws.push_back(b.quotient_witnesses[c]);
            vs.push_back(b.quotient_opened[c]);
            zs.push_back(zeta.abi());
        }
        if (pre_width > 0) matrix(in.vk_commitment, pp.preprocessed_opened, pp.preprocessed_witnesses, pre_width);
        int ok = 0;
        const int rc = eon_kzg_verify_batch(ctx, cs.data(), ws.data(), vs.data(), zs.data(), cs.size(),
                                            &pcs.g2_alpha(), &ok);
        // a commitment or witness that is no curve point, or an opened value that is no canonical
        // Fr, cannot come out of the reference's deserialisation: not an opening
        if (rc == EON_E_ARG) {
            const char* msg = eon_last_error(ctx);
            return verdict(out, EON_VERIFY_INVALID_OPENING_ARGUMENT,
                           std::string("malformed opening: ") + (msg ? msg : "invalid argument"));
        }
        check(ctx, rc, "eon_kzg_verify_batch");
        if (!ok)
            return verdict(out, EON_VERIFY_INVALID_OPENING_ARGUMENT,
                           "KzgError::ProofShapeMismatch: the batched pairing check of " + std::to_string(cs.size()) +
                               " openings failed");
    }

    // ---- 4. quotient(zeta) (:476-480) -----------------------------------------------------------
    std::vector<Fr> chunks(num_chunks);
    for (uint32_t c = 0; c < num_chunks; c++) chunks[c] = Fr::from_abi(b.quotient_opened[c]);
    const Fr quotient = recompose_quotient(log_n, log_qd, chunks.data(), zeta);

    // ---- 5. verify_constraints (:77-160) --------------------------------------------------------
    SelectorsAtPoint sels;
    if (!selectors_at_point(log_n, zeta, &sels))  // the reference panics: inverse of zero
        throw Error(EON_E_ARG, "zeta lies on the trace domain: the selectors at zeta are undefined");
    // the opened rows on the device: local | next | pre_local | pre_next | perm_local | perm_next
    const size_t total = 2 * ((size_t)width + pre_width + perm_width);
    DeviceBuffer rows(std::max<size_t>(total, 1) * sizeof(eon_fr));
    hipStream_t stream = static_cast<hipStream_t>(eon_ctx_stream(ctx));
    std::vector<eon_fr> host(std::max<size_t>(total, 1));
    std::memcpy(host.data(), b.trace_opened, 2 * (size_t)width * sizeof(eon_fr));
    if (pre_width) std::memcpy(host.data() + 2 * width, pp.preprocessed_opened, 2 * (size_t)pre_width * sizeof(eon_fr));
    if (perm_width)
        std::memcpy(host.data() + 2 * (width + pre_width), lk.permutation_opened,
                    2 * (size_t)perm_width * sizeof(eon_fr));
    if (hipMemcpyAsync(rows.get(), host.data(), host.size() * sizeof(eon_fr), hipMemcpyHostToDevice, stream) !=
            hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        throw Error(EON_E_DEVICE, "copying the opened values to the device failed");
    const eon_fr* d = rows.as<eon_fr>();
    const eon_fr* d_pre = d + 2 * width;
    const eon_fr* d_perm = d_pre + 2 * pre_width;
    std::vector<eon_fr> ch(std::max<size_t>(out.challenges.size(), 1));
    for (size_t i = 0; i < out.challenges.size(); i++) ch[i] = out.challenges[i].abi();
    const eon_fr a = out.alpha.abi(), z = zeta.abi();
    eon_fr res[2];
    check(ctx,
          eon_air_eval_at_point_dev(ctx, in.prog, log_n, &z, &a, d, d + width, pre_width ? d_pre : nullptr,
                                    pre_width ? d_pre + pre_width : nullptr, perm_width ? d_perm : nullptr,
                                    perm_width ? d_perm + perm_width : nullptr, in.publics, in.n_public, ch.data(),
                                    (uint32_t)out.challenges.size(), res),
          "eon_air_eval_at_point_dev");
    if (!(Fr::from_abi(res[1]) == quotient))  // :155
        return verdict(out, EON_VERIFY_OOD_EVALUATION_MISMATCH,
                       "constraints(zeta) / Z_H(zeta) differs from quotient(zeta)");
    return out;
}

}  // namespace eon_host
