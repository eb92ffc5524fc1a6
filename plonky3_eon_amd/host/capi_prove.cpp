// extern "C" surface of the prove driver (include/eon_prove.h).
#include <cstring>
#include <memory>
#include <string>

#include "eon_prove.h"
#include "prover.h"
#include "transcript.h"
#include "verifier.h"

struct eon_kzg_pcs {
    eon_host::KzgPcs* pcs = nullptr;
    std::string last_error;
    bool check_constraints = false;        // eon_kzg_pcs_set_check_constraints
    eon_constraint_report last_report{};   // of the last eon_prove_air* that ran with the switch on
    uint32_t opening = EON_OPENING_PER_COLUMN;  // eon_kzg_pcs_set_opening
    bool have_gamma = false, have_delta = false;  // eon_kzg_pcs_set_opening_challenges
    eon_host::Fr gamma = eon_host::Fr::zero(), delta = eon_host::Fr::zero();
    bool have_last = false;  // of the last batched prove / verify
    eon_host::Fr last_gamma = eon_host::Fr::zero(), last_delta = eon_host::Fr::zero();
    std::vector<eon_host::VerifyOutcome> many;  // of the last eon_verify_air_many[_fs]
};

struct eon_preprocessed {
    std::unique_ptr<eon_host::Preprocessed> pp;
};

struct eon_challenger {
    eon_host::DuplexChallenger ch;
};

namespace {

template <class F>
int guarded(eon_kzg_pcs* h, F&& f) {
    try {
        f();
        if (h) h->last_error.clear();
        return EON_OK;
    } catch (const eon_host::Error& e) {
        if (h) h->last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        if (h) h->last_error = "host allocation failed";
        return EON_E_OOM;
    } catch (const std::exception& e) {
        if (h) h->last_error = e.what();
        return EON_E_DEVICE;
    }
}

// a prove of a program: f(check) with the constraint check when the pcs has it switched on; the
// report is kept on the pcs whether the prove succeeded or not
template <class F>
int guarded_prove(eon_kzg_pcs* h, F&& f) {
    eon_host::ConstraintCheck cc;
    const bool on = h->check_constraints;
    const int rc = guarded(h, [&] { f(on ? &cc : nullptr); });
    if (on) h->last_report = cc.report;
    return rc;
}

// The pcs's opening mode for one prove: get() is null in the per-column mode, so that prove is then
// what it is without this surface; done() records the challenges a batched prove used (delta: the
// transcript's with a challenger, else the one set on the pcs, else zero).
struct OpeningScope {
    eon_kzg_pcs* h;
    eon_host::BatchedOpening bo;
    explicit OpeningScope(eon_kzg_pcs* h_) : h(h_) {
        bo.have_gamma = h->have_gamma;
        bo.gamma = h->gamma;
    }
    eon_host::BatchedOpening* get() { return h->opening == EON_OPENING_BATCHED ? &bo : nullptr; }
    void done(bool fs) {
        if (h->opening != EON_OPENING_BATCHED) return;
        h->have_last = true;
        h->last_gamma = bo.gamma_used;
        h->last_delta = fs ? bo.delta_used : h->have_delta ? h->delta : eon_host::Fr::zero();
    }
};

bool canonical(const eon_fr& v) {
    for (int k = 3; k >= 0; k--) {
        if (v.l[k] < eon_host::Fr::P[k]) return true;
        if (v.l[k] > eon_host::Fr::P[k]) return false;
    }
    return false;
}

void copy_out(const eon_host::Proof& p, eon_proof* out);
void copy_out_pp(const eon_host::Proof& p, eon_proof_pp* out);
void copy_out_lk(const eon_host::Proof& p, eon_proof_lk* out);

void check_lk_arrays(const eon_air_program* prog, bool has_pp, const eon_proof_lk* out) {
    if (has_pp && (!out->pp.preprocessed_commit || !out->pp.preprocessed_opened || !out->pp.preprocessed_witnesses))
        throw eon_host::Error(EON_E_ARG, "null preprocessed output arrays");
    if (eon_air_program_permutation_width(prog) > 0 &&
        (!out->permutation_commit || !out->permutation_opened || !out->permutation_witnesses))
        throw eon_host::Error(EON_E_ARG, "null permutation output arrays");
}

bool proof_arrays_ok(const eon_proof* out) {
    return out->trace_commit && out->quotient_commit && out->trace_opened && out->trace_witnesses &&
           out->quotient_opened && out->quotient_witnesses;
}

}  // namespace

extern "C" {

uint32_t eon_prove_abi_version(void) { return 11; }

int eon_kzg_pcs_create(eon_ctx* ctx, uint64_t max_degree, const eon_fr* srs_alpha, eon_kzg_pcs** out) {
    if (!ctx || !srs_alpha || !out) return EON_E_ARG;
    eon_kzg_pcs* h = new eon_kzg_pcs();
    const int rc = guarded(h, [&] {
        h->pcs = new eon_host::KzgPcs(ctx, max_degree, eon_host::Fr::from_abi(*srs_alpha));
    });
    if (rc != EON_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return EON_OK;
}

static int create_from_srs(eon_ctx* ctx, const void* g1_powers, bool compressed, uint64_t n,
                           const eon_g2_affine* g2_alpha, uint32_t flags, const eon_fr* rho, eon_kzg_pcs** out,
                           eon_srs_report* report) {
    if (!ctx || !g1_powers || !n || !g2_alpha || !out || !report) return EON_E_ARG;
    if (!rho && !(flags & EON_SRS_TRUSTED)) return EON_E_ARG;
    *report = eon_srs_report{};
    eon_kzg_pcs* h = new eon_kzg_pcs();
    const int rc = guarded(h, [&] {
        h->pcs = new eon_host::KzgPcs(ctx, g1_powers, compressed, n, *g2_alpha, flags, rho, report);
    });
    if (rc != EON_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return EON_OK;
}

int eon_kzg_pcs_create_from_srs(eon_ctx* ctx, const eon_g1_affine* g1_powers, uint64_t n,
                                const eon_g2_affine* g2_alpha, uint32_t flags, const eon_fr* rho,
                                eon_kzg_pcs** out, eon_srs_report* report) {
    return create_from_srs(ctx, g1_powers, false, n, g2_alpha, flags, rho, out, report);
}

int eon_kzg_pcs_create_from_srs_bytes(eon_ctx* ctx, const uint8_t* g1_bytes, uint64_t n,
                                      const eon_g2_affine* g2_alpha, uint32_t flags, const eon_fr* rho,
                                      eon_kzg_pcs** out, eon_srs_report* report) {
    return create_from_srs(ctx, g1_bytes, true, n, g2_alpha, flags, rho, out, report);
}

int eon_kzg_pcs_create_verifier(eon_ctx* ctx, uint64_t max_degree, const eon_g2_affine* g2_alpha,
                                eon_kzg_pcs** out) {
    if (!ctx || !g2_alpha || !out) return EON_E_ARG;
    eon_kzg_pcs* h = new eon_kzg_pcs();
    const int rc = guarded(h, [&] { h->pcs = new eon_host::KzgPcs(ctx, max_degree, *g2_alpha); });
    if (rc != EON_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return EON_OK;
}

void eon_kzg_pcs_destroy(eon_kzg_pcs* pcs) {
    if (!pcs) return;
    delete pcs->pcs;
    delete pcs;
}

const char* eon_kzg_pcs_last_error(const eon_kzg_pcs* pcs) { return pcs ? pcs->last_error.c_str() : "null pcs"; }

int eon_kzg_pcs_set_check_constraints(eon_kzg_pcs* pcs, int enable) {
    if (!pcs) return EON_E_ARG;
    pcs->check_constraints = enable != 0;
    return EON_OK;
}

int eon_kzg_pcs_check_constraints(const eon_kzg_pcs* pcs) { return pcs && pcs->check_constraints ? 1 : 0; }

int eon_kzg_pcs_last_constraint_report(const eon_kzg_pcs* pcs, eon_constraint_report* out) {
    if (!pcs || !out) return EON_E_ARG;
    *out = pcs->last_report;
    return EON_OK;
}

int eon_kzg_pcs_set_opening(eon_kzg_pcs* pcs, uint32_t mode) {
    if (!pcs || (mode != EON_OPENING_PER_COLUMN && mode != EON_OPENING_BATCHED)) return EON_E_ARG;
    pcs->opening = mode;
    return EON_OK;
}

int eon_kzg_pcs_opening(const eon_kzg_pcs* pcs) { return pcs ? (int)pcs->opening : EON_E_ARG; }

int eon_kzg_pcs_set_opening_challenges(eon_kzg_pcs* pcs, const eon_fr* gamma, const eon_fr* delta) {
    if (!pcs || (gamma && !canonical(*gamma)) || (delta && !canonical(*delta))) return EON_E_ARG;
    pcs->have_gamma = gamma != nullptr;
    pcs->have_delta = delta != nullptr;
    if (gamma) pcs->gamma = eon_host::Fr::from_abi(*gamma);
    if (delta) pcs->delta = eon_host::Fr::from_abi(*delta);
    return EON_OK;
}

int eon_kzg_pcs_last_opening_challenges(const eon_kzg_pcs* pcs, eon_fr* gamma, eon_fr* delta) {
    if (!pcs || !pcs->have_last) return EON_E_ARG;
    if (gamma) *gamma = pcs->last_gamma.abi();
    if (delta) *delta = pcs->last_delta.abi();
    return EON_OK;
}

int eon_poseidon2_bn254_permute(const eon_poseidon2_constants* perm, eon_fr state[3]) {
    if (!perm || !state) return EON_E_ARG;
    return guarded(nullptr, [&] {
        using namespace eon_host;
        const Poseidon2Bn254 p(*perm);
        Fr s[3] = {Fr::from_abi(state[0]), Fr::from_abi(state[1]), Fr::from_abi(state[2])};
        p.permute(s);
        for (int i = 0; i < 3; i++) state[i] = s[i].abi();
    });
}

int eon_g1_to_bytes(const eon_g1_affine* point, uint8_t out[32]) {
    if (!point || !out) return EON_E_ARG;
    eon_host::g1_to_bytes(*point, out);
    return EON_OK;
}

int eon_challenger_create(const eon_poseidon2_constants* perm, eon_challenger** out) {
    if (!perm || !out) return EON_E_ARG;
    return guarded(nullptr, [&] { *out = new eon_challenger{eon_host::DuplexChallenger(eon_host::Poseidon2Bn254(*perm))}; });
}

void eon_challenger_destroy(eon_challenger* ch) { delete ch; }

int eon_challenger_observe(eon_challenger* ch, const eon_fr* values, uint64_t n) {
    if (!ch || (n && !values)) return EON_E_ARG;
    for (uint64_t i = 0; i < n; i++) {
        const eon_host::Fr v = eon_host::Fr::from_abi(values[i]);
        for (int k = 3; k >= 0; k--) {  // canonical (Fr deserialisation rejects >= r)
            if (v.l[k] != eon_host::Fr::P[k]) {
                if (v.l[k] > eon_host::Fr::P[k]) return EON_E_ARG;
                break;
            }
            if (k == 0) return EON_E_ARG;
        }
    }
    for (uint64_t i = 0; i < n; i++) ch->ch.observe(eon_host::Fr::from_abi(values[i]));
    return EON_OK;
}

int eon_challenger_observe_g1(eon_challenger* ch, const eon_g1_affine* points, uint64_t n) {
    if (!ch || (n && !points)) return EON_E_ARG;
    ch->ch.observe_g1(points, n);
    return EON_OK;
}

int eon_challenger_sample(eon_challenger* ch, eon_fr* out) {
    if (!ch || !out) return EON_E_ARG;
    *out = ch->ch.sample().abi();
    return EON_OK;
}

int eon_challenger_state(const eon_challenger* ch, eon_fr out[3]) {
    if (!ch || !out) return EON_E_ARG;
    for (int i = 0; i < 3; i++) out[i] = ch->ch.state()[i].abi();
    return EON_OK;
}

int eon_prove_p2air(eon_kzg_pcs* pcs, const eon_p2air* air, const eon_fr* trace, uint64_t height,
                    const eon_fr* alpha, const eon_fr* zeta, uint32_t max_constraint_degree,
                    const eon_collective* shard, eon_proof* out) {
    if (!pcs || !pcs->pcs || !air || !trace || !alpha || !zeta || !out) return EON_E_ARG;
    if (!out->trace_commit || !out->quotient_commit || !out->trace_opened || !out->trace_witnesses ||
        !out->quotient_opened || !out->quotient_witnesses)
        return EON_E_ARG;
    return guarded(pcs, [&] {
        using namespace eon_host;
        AirRef a;
        a.p2 = air;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::from_abi(*alpha), Fr::from_abi(*zeta),
                        max_constraint_degree, shard, nullptr, nullptr, nullptr, nullptr, os.get());
        os.done(false);
        copy_out(p, out);
    });
}

int eon_prove_air(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                  const eon_fr* publics, uint32_t n_public, const eon_fr* alpha, const eon_fr* zeta,
                  eon_proof* out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !alpha || !zeta || !out || (n_public && !publics))
        return EON_E_ARG;
    if (!out->trace_commit || !out->quotient_commit || !out->trace_opened || !out->trace_witnesses ||
        !out->quotient_opened || !out->quotient_witnesses)
        return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::from_abi(*alpha), Fr::from_abi(*zeta), 0, nullptr, nullptr,
                        nullptr, nullptr, cc, os.get());
        os.done(false);
        copy_out(p, out);
    });
}

int eon_prove_air_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                     const eon_fr* publics, uint32_t n_public, eon_challenger* challenger, eon_proof* out,
                     eon_fr* alpha_out, eon_fr* zeta_out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !challenger || !out || (n_public && !publics)) return EON_E_ARG;
    if (!out->trace_commit || !out->quotient_commit || !out->trace_opened || !out->trace_witnesses ||
        !out->quotient_opened || !out->quotient_witnesses)
        return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::zero(), Fr::zero(), 0, nullptr, &challenger->ch, nullptr,
                        nullptr, cc, os.get());
        os.done(true);
        copy_out(p, out);
        if (alpha_out) *alpha_out = p.alpha.abi();
        if (zeta_out) *zeta_out = p.zeta.abi();
    });
}

int eon_prove_air_sharded(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                          const eon_fr* publics, uint32_t n_public, const eon_fr* alpha, const eon_fr* zeta,
                          const eon_collective* shard, eon_proof* out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !alpha || !zeta || !out || (n_public && !publics))
        return EON_E_ARG;
    if (!proof_arrays_ok(out)) return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::from_abi(*alpha), Fr::from_abi(*zeta), 0, shard, nullptr,
                        nullptr, nullptr, cc, os.get());
        os.done(false);
        copy_out(p, out);
    });
}

int eon_prove_air_sharded_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                             const eon_fr* publics, uint32_t n_public, eon_challenger* challenger,
                             const eon_collective* shard, eon_proof* out, eon_fr* alpha_out, eon_fr* zeta_out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !challenger || !out || (n_public && !publics)) return EON_E_ARG;
    if (!proof_arrays_ok(out)) return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::zero(), Fr::zero(), 0, shard, &challenger->ch, nullptr,
                        nullptr, cc, os.get());
        os.done(true);
        copy_out(p, out);
        if (alpha_out) *alpha_out = p.alpha.abi();
        if (zeta_out) *zeta_out = p.zeta.abi();
    });
}

int eon_setup_preprocessed(eon_kzg_pcs* pcs, const eon_fr* pre_trace, uint64_t height, uint32_t width,
                           eon_preprocessed** out) {
    if (!pcs || !pcs->pcs) return EON_E_ARG;
    return guarded(pcs, [&] {
        using namespace eon_host;
        if (!out) throw Error(EON_E_ARG, "null argument");
        auto* h = new eon_preprocessed();
        try {
            h->pp = setup_preprocessed(*pcs->pcs, pre_trace, height, width);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
    });
}

void eon_preprocessed_destroy(eon_preprocessed* pp) { delete pp; }

int eon_preprocessed_info(const eon_preprocessed* pp, uint32_t* width, uint32_t* degree_bits) {
    if (!pp || !pp->pp) return EON_E_ARG;
    if (width) *width = pp->pp->width;
    if (degree_bits) *degree_bits = pp->pp->degree_bits;
    return EON_OK;
}

int eon_preprocessed_commitment(const eon_preprocessed* pp, eon_g1_affine* out) {
    if (!pp || !pp->pp || !out) return EON_E_ARG;
    std::memcpy(out, pp->pp->commitment.data(), pp->pp->commitment.size() * sizeof(eon_g1_affine));
    return EON_OK;
}

int eon_prove_air_pp(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                     const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp, const eon_fr* alpha,
                     const eon_fr* zeta, eon_proof_pp* out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !alpha || !zeta || !out || (n_public && !publics))
        return EON_E_ARG;
    if (!proof_arrays_ok(&out->base)) return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        if (pp && (!out->preprocessed_commit || !out->preprocessed_opened || !out->preprocessed_witnesses))
            throw Error(EON_E_ARG, "null preprocessed output arrays");
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::from_abi(*alpha), Fr::from_abi(*zeta), 0, nullptr, nullptr,
                        pp ? pp->pp.get() : nullptr, nullptr, cc, os.get());
        os.done(false);
        copy_out_pp(p, out);
    });
}

int eon_prove_air_pp_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                        const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp,
                        eon_challenger* challenger, eon_proof_pp* out, eon_fr* alpha_out, eon_fr* zeta_out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !challenger || !out || (n_public && !publics)) return EON_E_ARG;
    if (!proof_arrays_ok(&out->base)) return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        if (pp && (!out->preprocessed_commit || !out->preprocessed_opened || !out->preprocessed_witnesses))
            throw Error(EON_E_ARG, "null preprocessed output arrays");
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::zero(), Fr::zero(), 0, nullptr, &challenger->ch,
                        pp ? pp->pp.get() : nullptr, nullptr, cc, os.get());
        os.done(true);
        copy_out_pp(p, out);
        if (alpha_out) *alpha_out = p.alpha.abi();
        if (zeta_out) *zeta_out = p.zeta.abi();
    });
}

int eon_prove_air_lk(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                     const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp, const eon_fr* pre_trace,
                     const eon_fr* challenges, uint32_t n_challenges, const eon_fr* alpha, const eon_fr* zeta,
                     eon_proof_lk* out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !alpha || !zeta || !out || (n_public && !publics) ||
        (n_challenges && !challenges))
        return EON_E_ARG;
    if (!proof_arrays_ok(&out->pp.base)) return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        check_lk_arrays(prog, pp != nullptr, out);
        if (n_challenges != eon_air_program_num_challenges(prog))
            throw Error(EON_E_SHAPE, "challenge count differs from the program's");
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        LookupInputs lk;
        lk.pre_trace = pre_trace;
        lk.challenges = challenges;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::from_abi(*alpha), Fr::from_abi(*zeta), 0, nullptr, nullptr,
                        pp ? pp->pp.get() : nullptr, &lk, cc, os.get());
        os.done(false);
        copy_out_lk(p, out);
    });
}

int eon_prove_air_lk_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_fr* trace, uint64_t height,
                        const eon_fr* publics, uint32_t n_public, const eon_preprocessed* pp,
                        const eon_fr* pre_trace, eon_challenger* challenger, eon_proof_lk* out,
                        eon_fr* challenges_out, eon_fr* alpha_out, eon_fr* zeta_out) {
    if (!pcs || !pcs->pcs || !prog || !trace || !challenger || !out || (n_public && !publics)) return EON_E_ARG;
    if (!proof_arrays_ok(&out->pp.base)) return EON_E_ARG;
    return guarded_prove(pcs, [&](eon_host::ConstraintCheck* cc) {
        using namespace eon_host;
        check_lk_arrays(prog, pp != nullptr, out);
        AirRef a;
        a.prog = prog;
        a.publics = publics;
        a.n_public = n_public;
        LookupInputs lk;
        lk.pre_trace = pre_trace;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::zero(), Fr::zero(), 0, nullptr, &challenger->ch,
                        pp ? pp->pp.get() : nullptr, &lk, cc, os.get());
        os.done(true);
        copy_out_lk(p, out);
        if (challenges_out)
            for (size_t i = 0; i < p.perm_challenges.size(); i++) challenges_out[i] = p.perm_challenges[i].abi();
        if (alpha_out) *alpha_out = p.alpha.abi();
        if (zeta_out) *zeta_out = p.zeta.abi();
    });
}

int eon_prove_p2air_fs(eon_kzg_pcs* pcs, const eon_p2air* air, const eon_fr* trace, uint64_t height,
                       eon_challenger* challenger, uint32_t max_constraint_degree,
                       const eon_collective* shard, eon_proof* out, eon_fr* alpha_out, eon_fr* zeta_out) {
    if (!pcs || !pcs->pcs || !air || !trace || !challenger || !out) return EON_E_ARG;
    if (!out->trace_commit || !out->quotient_commit || !out->trace_opened || !out->trace_witnesses ||
        !out->quotient_opened || !out->quotient_witnesses)
        return EON_E_ARG;
    return guarded(pcs, [&] {
        using namespace eon_host;
        AirRef a;
        a.p2 = air;
        OpeningScope os(pcs);
        Proof p = prove(*pcs->pcs, a, trace, height, Fr::zero(), Fr::zero(), max_constraint_degree, shard,
                        &challenger->ch, nullptr, nullptr, nullptr, os.get());
        os.done(true);
        copy_out(p, out);
        if (alpha_out) *alpha_out = p.alpha.abi();
        if (zeta_out) *zeta_out = p.zeta.abi();
    });
}

int eon_verify_air(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proof, const eon_fr* publics,
                   uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits, const eon_g1_affine* vk_commitment,
                   const eon_fr* challenges, uint32_t n_challenges, const eon_fr* alpha, const eon_fr* zeta,
                   int* result) {
    if (!pcs || !pcs->pcs || !prog || !proof || !alpha || !zeta || !result || (n_public && !publics) ||
        (n_challenges && !challenges))
        return EON_E_ARG;
    std::string detail;
    const int rc = guarded(pcs, [&] {
        using namespace eon_host;
        VerifyInputs in;
        in.prog = prog;
        in.proof = proof;
        in.publics = publics;
        in.n_public = n_public;
        in.vk_width = vk_width;
        in.vk_degree_bits = vk_degree_bits;
        in.vk_commitment = vk_commitment;
        in.challenges = challenges;
        in.n_challenges = n_challenges;
        in.alpha = Fr::from_abi(*alpha);
        in.zeta = Fr::from_abi(*zeta);
        in.batched = pcs->opening == EON_OPENING_BATCHED;
        if (in.batched && (!pcs->have_gamma || !pcs->have_delta))
            throw Error(EON_E_ARG, "the batched opening without a challenger needs gamma and delta "
                                   "(eon_kzg_pcs_set_opening_challenges)");
        in.gamma = pcs->gamma;
        in.delta = pcs->delta;
        const VerifyOutcome o = verify(*pcs->pcs, in, nullptr);
        if (in.batched) {
            pcs->have_last = true;
            pcs->last_gamma = o.gamma;
            pcs->last_delta = o.delta;
        }
        *result = o.verdict;
        detail = o.detail;
    });
    if (rc == EON_OK) pcs->last_error = detail;  // why a proof was rejected
    return rc;
}

int eon_verify_air_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proof,
                      const eon_fr* publics, uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits,
                      const eon_g1_affine* vk_commitment, eon_challenger* challenger, int* result,
                      eon_fr* challenges_out, eon_fr* alpha_out, eon_fr* zeta_out) {
    if (!pcs || !pcs->pcs || !prog || !proof || !challenger || !result || (n_public && !publics)) return EON_E_ARG;
    std::string detail;
    const int rc = guarded(pcs, [&] {
        using namespace eon_host;
        VerifyInputs in;
        in.prog = prog;
        in.proof = proof;
        in.publics = publics;
        in.n_public = n_public;
        in.vk_width = vk_width;
        in.vk_degree_bits = vk_degree_bits;
        in.vk_commitment = vk_commitment;
        in.batched = pcs->opening == EON_OPENING_BATCHED;
        const VerifyOutcome o = verify(*pcs->pcs, in, &challenger->ch);
        if (in.batched) {
            pcs->have_last = true;
            pcs->last_gamma = o.gamma;
            pcs->last_delta = o.delta;
        }
        *result = o.verdict;
        detail = o.detail;
        if (o.verdict == EON_VERIFY_INVALID_PROOF_SHAPE) return;  // rejected before the transcript
        if (challenges_out)
            for (size_t i = 0; i < o.challenges.size(); i++) challenges_out[i] = o.challenges[i].abi();
        if (alpha_out) *alpha_out = o.alpha.abi();
        if (zeta_out) *zeta_out = o.zeta.abi();
    });
    if (rc == EON_OK) pcs->last_error = detail;
    return rc;
}

}  // extern "C"

namespace {

// eon_verify_air_many[_fs]: the n inputs from the C arrays, eon_host::verify_many, the verdicts out
// and the outcomes kept for eon_verify_many_detail / _opening_challenges.  `fill(i, in)` sets what
// differs between the two entry points.
template <class Fill>
int verify_many_c(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proofs, uint32_t n,
                  const eon_fr* publics, uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits,
                  const eon_g1_affine* vk_commitment, const std::vector<eon_host::DuplexChallenger*>& challengers,
                  int* results, Fill fill) {
    pcs->many.clear();
    std::string first;
    const int rc = guarded(pcs, [&] {
        using namespace eon_host;
        std::vector<VerifyInputs> ins(n);
        for (uint32_t i = 0; i < n; i++) {
            VerifyInputs& in = ins[i];
            in.prog = prog;
            in.proof = &proofs[i];
            in.publics = n_public ? publics + (size_t)i * n_public : nullptr;
            in.n_public = n_public;
            in.vk_width = vk_width;
            in.vk_degree_bits = vk_degree_bits;
            in.vk_commitment = vk_commitment;
            in.batched = pcs->opening == EON_OPENING_BATCHED;
            fill(i, in);
        }
        std::vector<VerifyOutcome> outs = verify_many(*pcs->pcs, ins, challengers);
        for (uint32_t i = 0; i < n; i++) {
            results[i] = outs[i].verdict;
            if (outs[i].verdict != EON_VERIFY_OK && first.empty())
                first = "proof " + std::to_string(i) + ": " + outs[i].detail;
        }
        pcs->many = std::move(outs);
    });
    if (rc == EON_OK) pcs->last_error = first;  // why the first rejected proof was rejected
    return rc;
}

}  // namespace

extern "C" {

int eon_verify_air_many(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proofs, uint32_t n,
                        const eon_fr* publics, uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits,
                        const eon_g1_affine* vk_commitment, const eon_fr* challenges, uint32_t n_challenges,
                        const eon_fr* alphas, const eon_fr* zetas, const eon_fr* gammas, const eon_fr* deltas,
                        int* results) {
    if (!pcs || !pcs->pcs) return EON_E_ARG;
    if (n == 0) {
        pcs->many.clear();
        return EON_OK;
    }
    if (!prog || !proofs || !alphas || !zetas || !results || (n_public && !publics) || (n_challenges && !challenges))
        return EON_E_ARG;
    const bool batched = pcs->opening == EON_OPENING_BATCHED;
    if (batched && ((!gammas && !pcs->have_gamma) || (!deltas && !pcs->have_delta))) {
        pcs->last_error = "the batched opening without a challenger needs gamma and delta (the arrays, or "
                          "eon_kzg_pcs_set_opening_challenges)";
        return EON_E_ARG;
    }
    return verify_many_c(pcs, prog, proofs, n, publics, n_public, vk_width, vk_degree_bits, vk_commitment, {}, results,
                         [&](uint32_t i, eon_host::VerifyInputs& in) {
                             using eon_host::Fr;
                             in.challenges = n_challenges ? challenges + (size_t)i * n_challenges : nullptr;
                             in.n_challenges = n_challenges;
                             in.alpha = Fr::from_abi(alphas[i]);
                             in.zeta = Fr::from_abi(zetas[i]);
                             in.gamma = gammas ? Fr::from_abi(gammas[i]) : pcs->gamma;
                             in.delta = deltas ? Fr::from_abi(deltas[i]) : pcs->delta;
                         });
}

int eon_verify_air_many_fs(eon_kzg_pcs* pcs, const eon_air_program* prog, const eon_proof_lk* proofs, uint32_t n,
                           const eon_fr* publics, uint32_t n_public, uint32_t vk_width, uint32_t vk_degree_bits,
                           const eon_g1_affine* vk_commitment, eon_challenger* const* challengers, int* results,
                           eon_fr* challenges_out, eon_fr* alphas_out, eon_fr* zetas_out) {
    if (!pcs || !pcs->pcs) return EON_E_ARG;
    if (n == 0) {
        pcs->many.clear();
        return EON_OK;
    }
    if (!prog || !proofs || !challengers || !results || (n_public && !publics)) return EON_E_ARG;
    std::vector<eon_host::DuplexChallenger*> chs(n);
    for (uint32_t i = 0; i < n; i++) {
        if (!challengers[i]) return EON_E_ARG;
        for (uint32_t j = 0; j < i; j++)
            if (challengers[j] == challengers[i]) return EON_E_ARG;  // one transcript per proof
        chs[i] = &challengers[i]->ch;
    }
    const int rc = verify_many_c(pcs, prog, proofs, n, publics, n_public, vk_width, vk_degree_bits, vk_commitment, chs,
                                 results, [](uint32_t, eon_host::VerifyInputs&) {});
    if (rc != EON_OK) return rc;
    const uint32_t n_ch = eon_air_program_num_challenges(prog);
    for (uint32_t i = 0; i < n; i++) {
        const eon_host::VerifyOutcome& o = pcs->many[i];
        if (o.verdict == EON_VERIFY_INVALID_PROOF_SHAPE) continue;  // rejected before the transcript
        if (challenges_out)
            for (size_t j = 0; j < o.challenges.size(); j++) challenges_out[(size_t)i * n_ch + j] = o.challenges[j].abi();
        if (alphas_out) alphas_out[i] = o.alpha.abi();
        if (zetas_out) zetas_out[i] = o.zeta.abi();
    }
    return rc;
}

const char* eon_verify_many_detail(const eon_kzg_pcs* pcs, uint32_t i) {
    if (!pcs || i >= pcs->many.size()) return nullptr;
    return pcs->many[i].detail.c_str();
}

int eon_verify_many_opening_challenges(const eon_kzg_pcs* pcs, uint32_t i, eon_fr* gamma, eon_fr* delta) {
    if (!pcs || !gamma || !delta || i >= pcs->many.size()) return EON_E_ARG;
    *gamma = pcs->many[i].gamma.abi();
    *delta = pcs->many[i].delta.abi();
    return EON_OK;
}

}  // extern "C"

namespace {

void copy_out(const eon_host::Proof& p, eon_proof* out) {
    // nw: the witnesses per point, w per column or one in the batched mode ([2] compact entries)
    const size_t w = p.trace_commit.size(), c = p.quotient_commit.size(), nw = p.trace_witnesses[0].size();
    std::memcpy(out->trace_commit, p.trace_commit.data(), w * sizeof(eon_g1_affine));
    for (int k = 0; k < 2; k++) {
        std::memcpy(out->trace_opened + k * w, p.trace_opened[k].data(), w * sizeof(eon_fr));
        std::memcpy(out->trace_witnesses + k * nw, p.trace_witnesses[k].data(), nw * sizeof(eon_g1_affine));
    }
    std::memcpy(out->quotient_commit, p.quotient_commit.data(), c * sizeof(eon_g1_affine));
    std::memcpy(out->quotient_opened, p.quotient_opened.data(), c * sizeof(eon_fr));
    std::memcpy(out->quotient_witnesses, p.quotient_witnesses.data(), c * sizeof(eon_g1_affine));
    out->degree_bits = p.degree_bits;
    for (int s = 0; s < EON_STAGES; s++) out->stage_ms[s] = p.stage_ms[s];
}

void copy_out_pp(const eon_host::Proof& p, eon_proof_pp* out) {
    copy_out(p, &out->base);
    const size_t w = p.pre_commit.size(), nw = p.pre_witnesses[0].size();
    if (!w) return;
    std::memcpy(out->preprocessed_commit, p.pre_commit.data(), w * sizeof(eon_g1_affine));
    for (int k = 0; k < 2; k++) {
        std::memcpy(out->preprocessed_opened + k * w, p.pre_opened[k].data(), w * sizeof(eon_fr));
        std::memcpy(out->preprocessed_witnesses + k * nw, p.pre_witnesses[k].data(), nw * sizeof(eon_g1_affine));
    }
}

void copy_out_lk(const eon_host::Proof& p, eon_proof_lk* out) {
    copy_out_pp(p, &out->pp);
    const size_t w = p.perm_commit.size(), nw = p.perm_witnesses[0].size();
    if (!w) return;
    std::memcpy(out->permutation_commit, p.perm_commit.data(), w * sizeof(eon_g1_affine));
    for (int k = 0; k < 2; k++) {
        std::memcpy(out->permutation_opened + k * w, p.perm_opened[k].data(), w * sizeof(eon_fr));
        std::memcpy(out->permutation_witnesses + k * nw, p.perm_witnesses[k].data(), nw * sizeof(eon_g1_affine));
    }
}

}  // namespace
