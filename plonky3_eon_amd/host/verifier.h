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
#include "verify_prepare.h"

namespace eon_host {

// Throws Error for bad arguments and device errors (negative codes); every other outcome is a
// verdict.  `challenger` (nullable) is advanced exactly as the reference's verifier advances its own.
VerifyOutcome verify(KzgPcs& pcs, const VerifyInputs& in, DuplexChallenger* challenger);

// A batch of proofs of ONE program against one pcs, one outcome per proof: outcome i -- verdict,
// detail, the challenges used -- and the end state of challengers[i] are exactly those of verify on
// proof i alone.  verify's three phases, each over the whole batch:
//   1. prepare, per proof and without a device: shapes, the transcript, the openings in the
//      reference's round order, quotient(zeta); on min(n, VERIFY_PREPARE_THREADS) threads.  A proof
//      rejected here has its verdict and leaves the batch;
//   2. the openings of every remaining proof in ONE eon_kzg_verify_batch_many, a segment per proof
//      (every proof keeps its own Gt product: no weights across proofs).  A batched-mode proof's
//      gamma / delta scaling stays one column MSM per proof, run in sequence before it;
//   3. ONE eon_air_eval_at_points_dev over the proofs whose openings passed -- a proof that fails
//      its openings is never reported as an out-of-domain mismatch.
// `challengers`: empty (the given challenges of every input), or one per proof.  What throws in
// verify throws here with "proof i: " before the message, and no outcome is returned.
constexpr size_t VERIFY_PREPARE_THREADS = 8;
std::vector<VerifyOutcome> verify_many(KzgPcs& pcs, const std::vector<VerifyInputs>& ins,
                                       const std::vector<DuplexChallenger*>& challengers);

}  // namespace eon_host
