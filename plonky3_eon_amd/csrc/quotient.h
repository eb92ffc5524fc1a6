// Shared by quotient.hip (Poseidon2-AIR fused kernel) and air_program.hip (generic AIRs).
#pragma once
#include "context.h"

namespace eon {

// log_q - log_n <= 16, log_q <= 28
Status check_domains(uint32_t log_n, uint32_t log_q);
// Z_H(x_i) = shift^n w_rate^j - 1 and its inverse for the 2^(log_q - log_n) distinct values
// (ctx->sel_tab); enqueued on ctx->stream
Status vanishing_table(eon_ctx* ctx, uint32_t log_n, uint32_t log_q, const Fr& shift, Fr** zh, Fr** zh_inv);
// selectors_on_coset (commit/src/domain.rs:252-292) into out[0..4q): is_first_row, is_last_row,
// is_transition, inv_vanishing; shift != 1; enqueued on ctx->stream
Status selectors_launch(eon_ctx* ctx, uint32_t log_n, uint32_t log_q, const Fr& shift, Fr* out);
// LogUp contributions (lookup.hip): emitted = the 2 n_terms values k_lookup_terms wrote per row
// (denominator 2t, multiplicity 2t + 1; radix-2^29 registers in three planes, air_program.hip
// MemRegs), prefix = n_terms planes of `height` Fr of scratch, desc = term_off[L + 1] then aux[L]
// (device); perm[row][aux[l]] = sum of lookup l's multiplicity / denominator on the row;
// *zero_flag (device, preset to ~0) = the lowest lookup with a zero denominator; on ctx->stream
Status lookup_contributions(eon_ctx* ctx, const uint4* emitted, Fr* prefix, uint64_t height, const uint32_t* desc, uint32_t n_lookups,
                            uint32_t n_terms, Fr* perm, uint32_t perm_width, uint32_t* zero_flag);
// LogUp running sum (lookup.hip): perm (height x width, row-major, device) holds the per-row
// contributions and is replaced, in place, by their exclusive prefix sums over the rows of each
// column; enqueued on ctx->stream
Status lookup_running_sum(eon_ctx* ctx, Fr* perm, uint64_t height, uint32_t width);

}  // namespace eon
