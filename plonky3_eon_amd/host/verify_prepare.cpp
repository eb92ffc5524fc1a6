// See verify_prepare.h.  Line numbers are eon-uni-stark/src/verifier.rs unless another file is named.
#include "verify_prepare.h"

#include <algorithm>
#include <cstring>

#include "verify_host.h"

namespace eon_host {

namespace {

// A G1 point as the reference's deserialisation admits it: the identity (0, 0), or canonical
// coordinates with y^2 = x^3 + 3 (Montgomery residues; G1 has cofactor 1, so on the curve is in the
// group).  The batched verify folds commitments through an MSM before the pairing check sees them,
// so the raw points are tested here.
struct Fq4 {
    uint64_t l[4];
};
constexpr uint64_t FQ_P[4] = {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull,
                              0x30644e72e131a029ull};
// 3 * 2^256 mod q: the curve's b in Montgomery form
constexpr uint64_t FQ_THREE[4] = {0x7a17caa950ad28d7ull, 0x1f6ac17ae15521b9ull, 0x334bea4e696bd284ull,
                                  0x2a1f6744ce179d8eull};

bool fq_geq_p(const Fq4& a) {
    for (int i = 3; i >= 0; i--)
        if (a.l[i] != FQ_P[i]) return a.l[i] > FQ_P[i];
    return true;
}

// a b 2^-256 mod q, canonical (CIOS; a, b < q)
Fq4 fq_mul(const Fq4& a, const Fq4& b) {
    typedef unsigned __int128 u128;
    uint64_t inv = 1;  // -q^-1 mod 2^64 by Newton iteration
    for (int i = 0; i < 6; i++) inv *= 2 - FQ_P[0] * inv;
    inv = ~inv + 1;
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a.l[j] * b.l[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * inv;
        c = (u128)m * FQ_P[0] + t[0];
        c >>= 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * FQ_P[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    Fq4 r{{t[0], t[1], t[2], t[3]}};
    if (t[4] || fq_geq_p(r)) {
        uint64_t borrow = 0;
        for (int i = 0; i < 4; i++) {
            const u128 x = (u128)r.l[i] - FQ_P[i] - borrow;
            r.l[i] = (uint64_t)x;
            borrow = (uint64_t)(x >> 64) & 1;
        }
    }
    return r;
}

bool g1_valid(const eon_g1_affine& p) {
    typedef unsigned __int128 u128;
    Fq4 x, y;
    for (int i = 0; i < 4; i++) x.l[i] = p.x[i], y.l[i] = p.y[i];
    if (!(x.l[0] | x.l[1] | x.l[2] | x.l[3] | y.l[0] | y.l[1] | y.l[2] | y.l[3])) return true;
    if (fq_geq_p(x) || fq_geq_p(y)) return false;
    Fq4 rhs = fq_mul(fq_mul(x, x), x);
    u128 c = 0;
    for (int i = 0; i < 4; i++) {  // + 3: below 2q < 2^255
        c += (u128)rhs.l[i] + FQ_THREE[i];
        rhs.l[i] = (uint64_t)c;
        c >>= 64;
    }
    if (fq_geq_p(rhs)) {
        uint64_t borrow = 0;
        for (int i = 0; i < 4; i++) {
            const u128 d = (u128)rhs.l[i] - FQ_P[i] - borrow;
            rhs.l[i] = (uint64_t)d;
            borrow = (uint64_t)(d >> 64) & 1;
        }
    }
    const Fq4 lhs = fq_mul(y, y);
    return lhs.l[0] == rhs.l[0] && lhs.l[1] == rhs.l[1] && lhs.l[2] == rhs.l[2] && lhs.l[3] == rhs.l[3];
}

VerifyOutcome verdict(VerifyOutcome o, int v, const std::string& why) {
    o.verdict = v;
    o.detail = why;
    return o;
}

void reject(Prepared& p, int v, const std::string& why) {
    p.out = verdict(p.out, v, why);
    p.done = true;
}

}  // namespace

// ---- phase 1: everything before the first device call -------------------------------------------
// The shape checks, the transcript (on the proof's own challenger, or the given challenges),
// ensure_supported, the openings in the reference's round order (the batched mode: the claims,
// their canonical / G1 checks, gamma and delta, the scalar matrix of the scaling MSM), the opened
// rows and quotient(zeta).  Reads nothing but its arguments and writes only its result and its own
// challenger, so the proofs of a batch run it side by side.
Prepared prepare(uint64_t max_degree, const ProgShape& ps, const VerifyInputs& in, DuplexChallenger* challenger) {
    Prepared P;
    if (!in.prog || !in.proof) throw Error(EON_E_ARG, "null program or proof");
    if (in.n_public && !in.publics) throw Error(EON_E_ARG, "null public values");
    const eon_proof_lk& lk = *in.proof;
    const eon_proof_pp& pp = lk.pp;
    const eon_proof& b = pp.base;
    if (!b.trace_commit || !b.quotient_commit || !b.trace_opened || !b.trace_witnesses || !b.quotient_opened ||
        !b.quotient_witnesses)
        throw Error(EON_E_ARG, "null trace or quotient arrays in the proof");
    if (in.n_public != ps.n_public) throw Error(EON_E_SHAPE, "public value count differs from the program's");
    const uint32_t width = ps.width;
    const uint32_t prog_pre_width = ps.pre_width;
    const uint32_t perm_width = ps.perm_width;
    const uint32_t n_challenges = ps.n_challenges;
    const uint32_t log_qd = ps.log_qd;
    const uint32_t num_chunks = 1u << log_qd;
    const uint32_t log_n = b.degree_bits;
    if (log_n + log_qd > Fr::TWO_ADICITY)  // the reference's two_adic_generator panics
        throw Error(EON_E_SHAPE, "degree_bits " + std::to_string(log_n) + " + log_quotient_degree exceeds the field's "
                                 "two-adicity");
    VerifyOutcome& out = P.out;
    P.log_n = log_n;
    P.batched = in.batched;

    // ---- 1. shapes ------------------------------------------------------------------------------
    // process_preprocessed_trace (:165-225): the expected width is the key's, else the AIR's; the
    // proof carries preprocessed openings exactly when it is nonzero; a width needs a key and a key's
    // width is the width.  (The array widths themselves are the caller's: C arrays carry no length.)
    const bool has_vk = in.vk_commitment != nullptr;
    const uint32_t pre_width = has_vk ? in.vk_width : prog_pre_width;
    P.pre_width = pre_width;
    const bool proof_has_pre = pp.preprocessed_opened != nullptr;
    if ((pre_width > 0) != proof_has_pre) {
        reject(P, EON_VERIFY_INVALID_PROOF_SHAPE,
               "the verifier expects " + std::to_string(pre_width) + " preprocessed columns and the proof " +
                   (proof_has_pre ? "opens some" : "opens none"));
        return P;
    }
    if (pre_width > 0 && !has_vk) {
        reject(P, EON_VERIFY_INVALID_PROOF_SHAPE, "the AIR has preprocessed columns but no verifier key was given");
        return P;
    }
    if (pre_width > 0 && !pp.preprocessed_witnesses) {
        reject(P, EON_VERIFY_INVALID_PROOF_SHAPE, "preprocessed openings without witnesses");
        return P;
    }
    // the program reads exactly its own preprocessed columns (the reference's AIR would index past
    // the opened row, or ignore it)
    if (pre_width != prog_pre_width) {
        reject(P, EON_VERIFY_INVALID_PROOF_SHAPE,
               "the verifier key's width " + std::to_string(pre_width) + " differs from the AIR's " +
                   std::to_string(prog_pre_width));
        return P;
    }
    if (has_vk && pre_width > 0 && in.vk_degree_bits != log_n) {  // :272-277
        reject(P, EON_VERIFY_INVALID_PROOF_SHAPE,
               "the verifier key's degree_bits " + std::to_string(in.vk_degree_bits) + " differs from the proof's " +
                   std::to_string(log_n));
        return P;
    }
    // :330-352: the permutation commitment and both opened rows, all or none; and all exactly when
    // the program has lookups
    const bool has_perm_commit = lk.permutation_commit != nullptr;
    const bool has_perm_opened = lk.permutation_opened != nullptr;
    if (has_perm_commit != has_perm_opened || (has_perm_commit && !lk.permutation_witnesses)) {
        reject(P, EON_VERIFY_INVALID_PROOF_SHAPE, "permutation commitment and openings must come together");
        return P;
    }
    if (has_perm_commit != (perm_width > 0)) {
        reject(P, EON_VERIFY_INVALID_PROOF_SHAPE,
               perm_width > 0 ? "the AIR has lookups but the proof has no permutation part"
                              : "the proof has a permutation part but the AIR has no lookups");
        return P;
    }
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
    const Fr zeta_next = fr_mul(zeta, fr_two_adic_generator(log_n));  // the trace domain's next_point (domain.rs:115-117)

    // ---- 3. KzgPcs::verify (kzg/src/pcs.rs:337-401): the openings -------------------------------
    // ensure_supported per domain: the trace domain and the chunk domains all have 2^log_n points
    if ((1ull << log_n) - 1 > max_degree) {  // KzgPcs::ensure_supported's refusal, as a verdict
        reject(P, EON_VERIFY_INVALID_OPENING_ARGUMENT,
               "KzgError::DegreeTooLarge: degree " + std::to_string((1ull << log_n) - 1) + " > max " +
                   std::to_string(max_degree));
        return P;
    }
    if (in.batched) {
        // The batched opening (EON_OPENING_BATCHED; not the reference's proof format): claim i =
        // (matrix, point) in the round order carries ONE witness W_i.  With C_i = sum_j gamma^j C_(m,j)
        // and v_i = sum_j gamma^j v_(i,j), the K claims go to ONE verify_batch as
        // (delta^i C_i, delta^i W_i, delta^i v_i, z_i): prod_i e(delta^i (C_i - v_i G1), G2)
        // e(-delta^i W_i, g2_alpha - z_i G2) = 1.  The weights are what makes the product a sound
        // batch check (the per-column mode keeps the reference's unweighted one).
        struct Claim {
            const eon_g1_affine* commit;
            const eon_fr* values;
            const eon_g1_affine* witness;
            uint32_t w;
            Fr z;
        };
        std::vector<Claim> claims;
        auto matrix = [&](const eon_g1_affine* commit, const eon_fr* opened, const eon_g1_affine* wit, uint32_t w) {
            claims.push_back({commit, opened, wit, w, zeta});
            claims.push_back({commit, opened + w, wit + 1, w, zeta_next});
        };
        matrix(b.trace_commit, b.trace_opened, b.trace_witnesses, width);
        if (has_perm_commit) matrix(lk.permutation_commit, lk.permutation_opened, lk.permutation_witnesses, perm_width);
        for (uint32_t c = 0; c < num_chunks; c++)
            claims.push_back({b.quotient_commit + c, b.quotient_opened + c, b.quotient_witnesses + c, 1, zeta});
        if (pre_width > 0) matrix(in.vk_commitment, pp.preprocessed_opened, pp.preprocessed_witnesses, pre_width);
        // what the reference's deserialisation would refuse is no opening (as in the per-column mode)
        for (const Claim& c : claims) {
            const char* why = nullptr;
            for (uint32_t j = 0; j < c.w && !why; j++)
                if (!fr_is_canonical(Fr::from_abi(c.values[j]))) why = "an opened value is not a canonical Fr";
            for (uint32_t j = 0; j < c.w && !why; j++)
                if (!g1_valid(c.commit[j])) why = "a commitment is not a point of G1";
            if (!why && !g1_valid(*c.witness)) why = "a witness is not a point of G1";
            if (why) {
                reject(P, EON_VERIFY_INVALID_OPENING_ARGUMENT, std::string("malformed opening: ") + why);
                return P;
            }
        }
        out.gamma = in.gamma;
        out.delta = in.delta;
        if (challenger) {
            for (const Claim& c : claims)
                for (uint32_t j = 0; j < c.w; j++) challenger->observe(Fr::from_abi(c.values[j]));
            out.gamma = challenger->sample();
            for (const Claim& c : claims) challenger->observe_g1(c.witness, 1);
            out.delta = challenger->sample();
        } else if (!fr_is_canonical(out.gamma) || !fr_is_canonical(out.delta)) {
            throw Error(EON_E_ARG, "gamma or delta is not a canonical Fr");
        }
        // Every scaled point from ONE variable-base column MSM (scale_claims): the bases are the
        // proof's commitments (a matrix's once, shared by its two claims) followed by the K
        // witnesses; column i of the scalar matrix holds delta^i gamma^j on the rows of claim i's
        // commitments and gives delta^i C_i, column K + i holds delta^i on the row of W_i and gives
        // delta^i W_i.
        const size_t K = claims.size();
        std::vector<size_t> first(K);
        for (size_t i = 0; i < K; i++) {
            if (i > 0 && claims[i].commit == claims[i - 1].commit) {
                first[i] = first[i - 1];
                continue;
            }
            first[i] = P.pts.size();
            P.pts.insert(P.pts.end(), claims[i].commit, claims[i].commit + claims[i].w);
        }
        const size_t wit0 = P.pts.size();
        for (const Claim& c : claims) P.pts.push_back(*c.witness);
        const size_t n_pts = P.pts.size(), cols = 2 * K;
        P.scal.assign(n_pts * cols, eon_fr{{0, 0, 0, 0}});
        P.vs.resize(K);
        P.zs.resize(K);
        Fr dpow = Fr::one();
        for (size_t i = 0; i < K; i++) {
            const Claim& c = claims[i];
            Fr s = dpow, v = Fr::zero();
            for (uint32_t j = 0; j < c.w; j++) {
                P.scal[(first[i] + j) * cols + i] = s.abi();
                v = fr_sum(v, fr_mul(s, Fr::from_abi(c.values[j])));
                s = fr_mul(s, out.gamma);
            }
            P.scal[(wit0 + i) * cols + K + i] = dpow.abi();
            P.vs[i] = v.abi();
            P.zs[i] = c.z.abi();
            dpow = fr_mul(dpow, out.delta);
        }
    } else {
        // the reference's round order: trace at {zeta, zeta h}, permutation at {zeta, zeta h}, quotient
        // chunks at {zeta}, preprocessed at {zeta, zeta h} (:415-471)
        auto matrix = [&](const eon_g1_affine* commit, const eon_fr* opened, const eon_g1_affine* wit, uint32_t w) {
            const Fr pts[2] = {zeta, zeta_next};
            for (int p = 0; p < 2; p++)
                for (uint32_t c = 0; c < w; c++) {
                    P.cs.push_back(commit[c]);
                    P.ws.push_back(wit[(size_t)p * w + c]);
                    P.vs.push_back(opened[(size_t)p * w + c]);
                    P.zs.push_back(pts[p].abi());
                }
        };
        matrix(b.trace_commit, b.trace_opened, b.trace_witnesses, width);
        if (has_perm_commit) matrix(lk.permutation_commit, lk.permutation_opened, lk.permutation_witnesses, perm_width);
        for (uint32_t c = 0; c < num_chunks; c++) {
            P.cs.push_back(b.quotient_commit[c]);
            P.ws.push_back(b.quotient_witnesses[c]);
            P.vs.push_back(b.quotient_opened[c]);
            P.zs.push_back(zeta.abi());
        }
        if (pre_width > 0) matrix(in.vk_commitment, pp.preprocessed_opened, pp.preprocessed_witnesses, pre_width);
    }

    // ---- 4. quotient(zeta) (:476-480) -----------------------------------------------------------
    std::vector<Fr> chunks(num_chunks);
    for (uint32_t c = 0; c < num_chunks; c++) chunks[c] = Fr::from_abi(b.quotient_opened[c]);
    P.quotient = recompose_quotient(log_n, log_qd, chunks.data(), zeta);

    // ---- 5. what verify_constraints (:77-160) evaluates -----------------------------------------
    SelectorsAtPoint sels;
    P.zeta_on_domain = !selectors_at_point(log_n, zeta, &sels);  // the reference panics: inverse of zero
    const size_t total = 2 * ((size_t)width + pre_width + perm_width);
    P.rows.resize(std::max<size_t>(total, 1));
    std::memcpy(P.rows.data(), b.trace_opened, 2 * (size_t)width * sizeof(eon_fr));
    if (pre_width) std::memcpy(P.rows.data() + 2 * width, pp.preprocessed_opened, 2 * (size_t)pre_width * sizeof(eon_fr));
    if (perm_width)
        std::memcpy(P.rows.data() + 2 * (width + pre_width), lk.permutation_opened,
                    2 * (size_t)perm_width * sizeof(eon_fr));
    return P;
}

}  // namespace eon_host
