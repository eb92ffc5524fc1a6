// verify_with_preprocessed (eon-uni-stark/src/verifier.rs:244-502) over KzgPcs, as a C++ driver
// above eon.h, for any AIR given as a constraint program: ZK off, Challenge = Fr, local lookups.
// The order is the reference's: shape checks (:257-352), the transcript (:355-397), KzgPcs::verify
// (kzg/src/pcs.rs:337-401: every opening in ONE eon_kzg_verify_batch against g2_alpha),
// recompose_quotient_from_chunks (:30-70, verify_host.h) and verify_constraints (:77-160), whose
// constraint evaluation at zeta is eon_air_eval_at_point_dev -- the AIR exists only as the compiled
// device program.
#pragma once
#include <string>
#include <vector>

#include "eon_prove.h"
#include "pcs.h"
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

// Throws Error for bad arguments and device errors (negative codes); every other outcome is a
// verdict.  `challenger` (nullable) is advanced exactly as the reference's verifier advances its own.
VerifyOutcome verify(KzgPcs& pcs, const VerifyInputs& in, DuplexChallenger* challenger);

}  // namespace eon_host
