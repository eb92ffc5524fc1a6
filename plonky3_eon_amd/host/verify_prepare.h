// The verifier's prepare phase: everything verify (verifier.h) does for one proof before its first
// device call, in a translation unit that includes no device header and calls nothing of
// libeonhip.so -- so that it runs on several threads at once (verify_many) and builds into a
// stand-alone host program under the sanitizers (tests/verify_prepare_check.cpp).
#pragma once
#include <string>
#include <vector>

#include "eon_prove.h"
#include "pcs.h"  // Error; declarations only
#include "transcript.h"

namespace eon_host {

struct VerifyInputs {
    const eon_air_program* prog = nullptr;
    const eon_proof_lk* proof = nullptr;  // the superset of the proof structs; NULL arrays = absent
    const eon_fr* publics = nullptr;
    uint32_t n_public = 0;
    // PreprocessedVerifierKey (preprocessed.rs:30-40) as plain values; vk_commitment NULL = no key
    uint32_t vk_width = 0, vk_degree_bits = 0;
    const eon_g1_affine* vk_commitment = nullptr;
    // without a challenger: the challenges the proof was made with
    const eon_fr* challenges = nullptr;
    uint32_t n_challenges = 0;
    Fr alpha = Fr::zero(), zeta = Fr::zero();
    // EON_OPENING_BATCHED: the witness arrays of the proof hold ONE point per opened point ([2],
    // [2], [C], [2]); without a challenger gamma and delta are the ones given here
    bool batched = false;
    Fr gamma = Fr::zero(), delta = Fr::zero();
};

struct VerifyOutcome {
    int verdict = EON_VERIFY_OK;  // EON_VERIFY_*
    std::string detail;           // why, when not OK
    Fr alpha = Fr::zero(), zeta = Fr::zero();  // the challenges used (sampled with a challenger)
    std::vector<Fr> challenges;
    Fr gamma = Fr::zero(), delta = Fr::zero();  // batched mode: the opening challenges used
};

// What the verifier reads off the program, once per call.
struct ProgShape {
    uint32_t width, n_public, pre_width, perm_width, n_challenges, log_qd;
};

// One proof between the phases.  prepare() fills it without touching a device; a proof whose
// verdict is reached (done) has left the batch.
struct Prepared {
    VerifyOutcome out;
    bool done = false;
    size_t index = 0;  // in the caller's batch, for the messages of what throws
    uint32_t log_n = 0, pre_width = 0;
    bool batched = false;
    Fr quotient = Fr::zero();    // quotient(zeta) recomposed from the opened chunks
    bool zeta_on_domain = false;  // the selectors at zeta are undefined: thrown once the openings passed
    // the openings of ONE verify_batch: the per-column mode's as they are, the batched mode's K
    // weighted claims (cs and ws filled by scale_claims)
    std::vector<eon_g1_affine> cs, ws;
    std::vector<eon_fr> vs, zs;
    // batched mode: the variable-base column MSM that scales the claims
    std::vector<eon_g1_affine> pts;
    std::vector<eon_fr> scal;
    std::vector<eon_fr> rows;  // the opened values: local | next | pre_local | pre_next | perm_local | perm_next
};

// Phase 1.  `max_degree`: the pcs's (KzgPcs::ensure_supported); `ps`: the program's shape; with a
// challenger the transcript is replayed on it, without, the given challenges of `in` are used.
// Throws Error where verify throws; a proof rejected here comes back with done set.
Prepared prepare(uint64_t max_degree, const ProgShape& ps, const VerifyInputs& in, DuplexChallenger* challenger);

}  // namespace eon_host
