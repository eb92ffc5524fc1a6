// The verifier's pure host maths (eon-uni-stark/src/verifier.rs:30-70, commit/src/domain.rs:174-246)
// over fr_host.h alone, so that it compiles and is tested stand-alone: canonical add / sub, the
// inverse, selectors_at_point, the quotient chunk domains' shifts and
// recompose_quotient_from_chunks.  Everything here is a few hundred products per verify.
#pragma once
#include <stdint.h>

#include <vector>

#include "fr_host.h"

namespace eon_host {

inline bool fr_is_canonical(const Fr& a) {
    for (int k = 3; k >= 0; k--) {
        if (a.l[k] < Fr::P[k]) return true;
        if (a.l[k] > Fr::P[k]) return false;
    }
    return false;
}

inline bool fr_is_zero(const Fr& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }

// a + b mod r for canonical a, b (a + b < 2r < 2^255: no 256-bit overflow).  Not named fr_add:
// transcript.h declares that one, defined in transcript.cpp, and this header stands alone.
inline Fr fr_sum(const Fr& a, const Fr& b) {
    Fr s;
    detail::u128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (detail::u128)a.l[i] + b.l[i];
        s.l[i] = (uint64_t)c;
        c >>= 64;
    }
    detail::cond_sub(s.l, Fr::P);
    return s;
}

// a - b mod r for canonical a, b
inline Fr fr_sub(const Fr& a, const Fr& b) {
    Fr d;
    uint64_t borrow = 0;
    for (int i = 0; i < 4; i++) {
        const detail::u128 t = (detail::u128)a.l[i] - b.l[i] - borrow;
        d.l[i] = (uint64_t)t;
        borrow = (uint64_t)(t >> 127);
    }
    if (borrow) {
        detail::u128 c = 0;
        for (int i = 0; i < 4; i++) {
            c += (detail::u128)d.l[i] + Fr::P[i];
            d.l[i] = (uint64_t)c;
            c >>= 64;
        }
    }
    return d;
}

// a^(r - 2): the inverse of a nonzero a (Fermat); 0 for a = 0 (the reference's inverse() panics there:
// callers test for zero first)
inline Fr fr_inverse(const Fr& a) {
    uint64_t e[4] = {Fr::P[0] - 2, Fr::P[1], Fr::P[2], Fr::P[3]};  // P[0] >= 2: no borrow
    Fr r = Fr::one();
    for (int w = 3; w >= 0; w--)
        for (int bit = 63; bit >= 0; bit--) {
            r = fr_mul(r, r);
            if ((e[w] >> bit) & 1) r = fr_mul(r, a);
        }
    return r;
}

// x^(2^log_n)
inline Fr fr_exp_power_of_2(Fr x, uint32_t log_n) {
    for (uint32_t i = 0; i < log_n; i++) x = fr_mul(x, x);
    return x;
}

// LagrangeSelectors at a point (commit/src/domain.rs:237-246) of the trace domain of size 2^log_n
// (shift 1), generator h: with Z_H = x^N - 1,
//   is_first_row = Z_H / (x - 1), is_last_row = Z_H / (x - h^-1), is_transition = x - h^-1,
//   inv_vanishing = 1 / Z_H
struct SelectorsAtPoint {
    Fr is_first_row, is_last_row, is_transition, inv_vanishing;
};
// false where the reference panics on the inverse of zero: x = 1, x = h^-1 or Z_H(x) = 0
inline bool selectors_at_point(uint32_t log_n, const Fr& x, SelectorsAtPoint* out) {
    const Fr z_h = fr_sub(fr_exp_power_of_2(x, log_n), Fr::one());
    const Fr h_inv = fr_inverse(fr_two_adic_generator(log_n));
    const Fr d_first = fr_sub(x, Fr::one()), d_last = fr_sub(x, h_inv);
    if (fr_is_zero(z_h) || fr_is_zero(d_first) || fr_is_zero(d_last)) return false;
    out->is_first_row = fr_mul(z_h, fr_inverse(d_first));
    out->is_last_row = fr_mul(z_h, fr_inverse(d_last));
    out->is_transition = d_last;
    out->inv_vanishing = fr_inverse(z_h);
    return true;
}

// The shifts of the 2^log_qd quotient chunk domains: the quotient domain is
// trace_domain.create_disjoint_domain(2^(log_n + log_qd)) (shift GENERATOR = 5, domain.rs:155-168),
// split_domains (domain.rs:174-186) gives chunk c the shift GENERATOR * g_Q^c (g_Q the quotient
// domain's generator) and the size 2^log_n.  A chunk domain's first_point is its shift.
inline std::vector<Fr> quotient_chunk_shifts(uint32_t log_n, uint32_t log_qd) {
    const Fr g_q = fr_two_adic_generator(log_n + log_qd);
    std::vector<Fr> out;
    Fr s = fr_from_u64(5);
    for (uint32_t c = 0; c < (1u << log_qd); c++) {
        out.push_back(s);
        s = fr_mul(s, g_q);
    }
    return out;
}

// vanishing_poly_at_point of the coset shift * H_(2^log_n) (domain.rs:226-228): (x / shift)^N - 1
inline Fr vanishing_at(const Fr& shift_inv, uint32_t log_n, const Fr& x) {
    return fr_sub(fr_exp_power_of_2(fr_mul(x, shift_inv), log_n), Fr::one());
}

// recompose_quotient_from_chunks (verifier.rs:30-70) for Challenge = Fr (one basis element per
// chunk): sum_i zps_i chunk_i with zps_i = prod_{j != i} Z_j(zeta) / Z_j(first_point_i).  The
// divisors never vanish: chunk i's first point lies on no other chunk's coset.
inline Fr recompose_quotient(uint32_t log_n, uint32_t log_qd, const Fr* chunk_values, const Fr& zeta) {
    const std::vector<Fr> shifts = quotient_chunk_shifts(log_n, log_qd);
    std::vector<Fr> shift_inv;
    for (const Fr& s : shifts) shift_inv.push_back(fr_inverse(s));
    Fr total = Fr::zero();
    for (size_t i = 0; i < shifts.size(); i++) {
        Fr zp = Fr::one();
        for (size_t j = 0; j < shifts.size(); j++) {
            if (j == i) continue;
            zp = fr_mul(zp, fr_mul(vanishing_at(shift_inv[j], log_n, zeta),
                                   fr_inverse(vanishing_at(shift_inv[j], log_n, shifts[i]))));
        }
        total = fr_sum(total, fr_mul(zp, chunk_values[i]));
    }
    return total;
}

}  // namespace eon_host
