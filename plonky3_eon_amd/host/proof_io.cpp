// eon_proof_bytes_size / _serialize / _peek / _deserialize (include/eon_prove.h): the proof container
// over the framing of proof_io.h.  Writing is host only (g1_to_bytes per point); loading sends every
// point of the proof through ONE eon_g1_decompress call, i.e. one upload and one k_g1_decompress.
#include "proof_io.h"

#include <new>
#include <vector>

#include "eon_prove.h"
#include "fr_host.h"
#include "transcript.h"

namespace pio = eon_host::proofio;

static_assert(sizeof(eon_proof_shape) == sizeof(pio::Shape) && sizeof(eon_proof_shape) == 24, "eon_proof_shape");
static_assert(EON_PROOF_IO_G1_NOT_ON_CURVE == (int)pio::G1_NOT_ON_CURVE && EON_PROOF_IO_MAGIC == (int)pio::BAD_MAGIC &&
                  EON_PROOF_IO_FR_NOT_CANONICAL == (int)pio::FR_NOT_CANONICAL,
              "EON_PROOF_IO_* are proof_io.h's reasons");
static_assert(EON_PROOF_SECTION_TRACE_COMMIT == (int)pio::TRACE_COMMIT &&
                  EON_PROOF_SECTION_QUOTIENT_OPENED == (int)pio::QUOTIENT_OPENED &&
                  EON_PROOF_SECTION_PREPROCESSED_WITNESS_NEXT == (int)pio::PREPROCESSED_WITNESS_NEXT,
              "EON_PROOF_SECTION_* are proof_io.h's sections");

namespace {

pio::Shape shape_of(const eon_proof_shape& s) {
    return pio::Shape{s.flags, s.degree_bits, s.width, s.chunks, s.pre_width, s.perm_width};
}

// where a section lives in the caller's arrays (NULL when its array is)
void* section_array(const eon_proof_lk* p, const uint64_t count[pio::SECTIONS], uint32_t section) {
    const eon_proof& b = p->pp.base;
    auto fr = [](eon_fr* a, uint64_t off) -> void* { return a ? a + off : nullptr; };
    auto g1 = [](eon_g1_affine* a, uint64_t off) -> void* { return a ? a + off : nullptr; };
    switch (section) {
        case pio::TRACE_COMMIT: return b.trace_commit;
        case pio::PERMUTATION_COMMIT: return p->permutation_commit;
        case pio::QUOTIENT_COMMIT: return b.quotient_commit;
        case pio::TRACE_LOCAL: return b.trace_opened;
        case pio::TRACE_NEXT: return fr(b.trace_opened, count[pio::TRACE_LOCAL]);
        case pio::PERMUTATION_LOCAL: return p->permutation_opened;
        case pio::PERMUTATION_NEXT: return fr(p->permutation_opened, count[pio::PERMUTATION_LOCAL]);
        case pio::PREPROCESSED_LOCAL: return p->pp.preprocessed_opened;
        case pio::PREPROCESSED_NEXT: return fr(p->pp.preprocessed_opened, count[pio::PREPROCESSED_LOCAL]);
        case pio::QUOTIENT_OPENED: return b.quotient_opened;
        case pio::TRACE_WITNESS_ZETA: return b.trace_witnesses;
        case pio::TRACE_WITNESS_NEXT: return g1(b.trace_witnesses, count[pio::TRACE_WITNESS_ZETA]);
        case pio::PERMUTATION_WITNESS_ZETA: return p->permutation_witnesses;
        case pio::PERMUTATION_WITNESS_NEXT: return g1(p->permutation_witnesses, count[pio::PERMUTATION_WITNESS_ZETA]);
        case pio::QUOTIENT_WITNESS: return b.quotient_witnesses;
        case pio::PREPROCESSED_WITNESS_ZETA: return p->pp.preprocessed_witnesses;
        case pio::PREPROCESSED_WITNESS_NEXT:
            return g1(p->pp.preprocessed_witnesses, count[pio::PREPROCESSED_WITNESS_ZETA]);
        default: return nullptr;
    }
}

bool arrays_present(const eon_proof_lk* p, const uint64_t count[pio::SECTIONS]) {
    for (uint32_t s = 1; s < pio::SECTIONS; s++)
        if (count[s] && !section_array(p, count, s)) return false;
    return true;
}

bool fr_canonical(const eon_fr& v) {
    for (int k = 3; k >= 0; k--) {
        if (v.l[k] < eon_host::Fr::P[k]) return true;
        if (v.l[k] > eon_host::Fr::P[k]) return false;
    }
    return false;
}

int rejected(eon_proof_io_report* r, uint32_t reason, uint32_t section, uint64_t index) {
    r->reason = reason;
    r->section = section;
    r->index = index;
    return EON_E_FORMAT;
}

}  // namespace

extern "C" {

uint64_t eon_proof_bytes_size(const eon_proof_shape* shape) {
    uint64_t total;
    return shape && pio::total_bytes(shape_of(*shape), &total) ? total : 0;
}

int eon_proof_serialize(const eon_proof_lk* proof, const eon_proof_shape* shape, uint8_t* out, uint64_t cap,
                        uint64_t* written) {
    if (!proof || !shape || !written) return EON_E_ARG;
    const pio::Shape s = shape_of(*shape);
    uint64_t body, total;
    if (!pio::body_bytes(s, &body) || !pio::total_bytes(s, &total)) return EON_E_SHAPE;
    *written = total;
    if (cap < total) return EON_E_SHAPE;
    uint64_t count[pio::SECTIONS];
    pio::section_counts(s, count);
    if (!out || !arrays_present(proof, count)) return EON_E_ARG;
    pio::write_header(s, body, out);
    uint8_t* w = out + pio::HEADER_BYTES;
    for (uint32_t sec = 1; sec < pio::SECTIONS; sec++) {
        for (uint64_t i = 0; i < count[sec]; i++, w += pio::ELEM_BYTES) {
            if (pio::section_is_g1(sec)) {
                eon_host::g1_to_bytes(static_cast<const eon_g1_affine*>(section_array(proof, count, sec))[i], w);
            } else {
                const eon_fr& v = static_cast<const eon_fr*>(section_array(proof, count, sec))[i];
                if (!fr_canonical(v)) return EON_E_ARG;  // bytes that no loader accepts are not written
                for (int k = 0; k < 4; k++) pio::store_u64(w + 8 * k, v.l[k]);
            }
        }
    }
    return EON_OK;
}

int eon_proof_peek(const uint8_t* bytes, uint64_t len, eon_proof_shape* shape, eon_proof_io_report* report) {
    if (!shape || !report || (len && !bytes)) return EON_E_ARG;
    *report = eon_proof_io_report{};
    pio::Shape s;
    const pio::Reason r = pio::peek(bytes, len, &s);
    if (r != pio::OK) return rejected(report, r, pio::HEADER, 0);
    *shape = eon_proof_shape{s.flags, s.degree_bits, s.width, s.chunks, s.pre_width, s.perm_width};
    return EON_OK;
}

int eon_proof_deserialize(eon_ctx* ctx, const uint8_t* bytes, uint64_t len, eon_proof_lk* out,
                          eon_proof_io_report* report) {
    if (!ctx || !out || !report || (len && !bytes)) return EON_E_ARG;
    *report = eon_proof_io_report{};
    pio::Shape s;
    const pio::Reason pr = pio::peek(bytes, len, &s);  // the length is settled before anything is allocated
    if (pr != pio::OK) return rejected(report, pr, pio::HEADER, 0);
    uint64_t count[pio::SECTIONS];
    pio::section_counts(s, count);
    if (!arrays_present(out, count)) return EON_E_ARG;
    uint64_t n_points = 0;
    for (uint32_t sec = 1; sec < pio::SECTIONS; sec++)
        if (pio::section_is_g1(sec)) n_points += count[sec];
    try {
        // opened values: copied out, the first that is >= r remembered; points: gathered for one call
        std::vector<uint64_t> packed(n_points * 4 + 1);  // 8-byte aligned staging of the compressed points
        uint32_t bad_fr_section = 0;
        uint64_t bad_fr_index = 0;
        const uint8_t* r = bytes + pio::HEADER_BYTES;
        uint64_t at = 0;
        for (uint32_t sec = 1; sec < pio::SECTIONS; sec++) {
            for (uint64_t i = 0; i < count[sec]; i++, r += pio::ELEM_BYTES) {
                if (pio::section_is_g1(sec)) {
                    for (int k = 0; k < 4; k++) packed[4 * at + k] = pio::load_u64(r + 8 * k);
                    at++;
                } else {
                    eon_fr& v = static_cast<eon_fr*>(section_array(out, count, sec))[i];
                    for (int k = 0; k < 4; k++) v.l[k] = pio::load_u64(r + 8 * k);
                    if (!bad_fr_section && !fr_canonical(v)) bad_fr_section = sec, bad_fr_index = i;
                }
            }
        }
        std::vector<eon_g1_affine> points(n_points + 1);
        eon_srs_report rep{};
        const int rc = eon_g1_decompress(ctx, reinterpret_cast<const uint8_t*>(packed.data()), n_points,
                                         points.data(), &rep);
        if (rc != EON_OK && rc != EON_E_SRS) return rc;
        // the lowest byte offset wins: commitments precede the opened values, witnesses follow them
        uint32_t bad_g1_section = 0;
        uint64_t bad_g1_index = 0;
        if (rc == EON_E_SRS) {
            uint64_t left = rep.index;
            for (uint32_t sec = 1; sec < pio::SECTIONS; sec++) {
                if (!pio::section_is_g1(sec)) continue;
                if (left < count[sec]) {
                    bad_g1_section = sec, bad_g1_index = left;
                    break;
                }
                left -= count[sec];
            }
        }
        if (bad_fr_section && (!bad_g1_section || bad_g1_section > bad_fr_section))
            return rejected(report, pio::FR_NOT_CANONICAL, bad_fr_section, bad_fr_index);
        if (bad_g1_section) {
            const uint32_t reason = rep.reason == EON_SRS_ENCODING        ? pio::G1_ENCODING
                                    : rep.reason == EON_SRS_NOT_CANONICAL ? pio::G1_NOT_CANONICAL
                                                                          : pio::G1_NOT_ON_CURVE;
            return rejected(report, reason, bad_g1_section, bad_g1_index);
        }
        at = 0;
        for (uint32_t sec = 1; sec < pio::SECTIONS; sec++) {
            if (!pio::section_is_g1(sec)) continue;
            eon_g1_affine* dst = static_cast<eon_g1_affine*>(section_array(out, count, sec));
            for (uint64_t i = 0; i < count[sec]; i++) dst[i] = points[at++];
        }
    } catch (const std::bad_alloc&) {
        return EON_E_OOM;
    }
    out->pp.base.degree_bits = s.degree_bits;
    return EON_OK;
}

}  // extern "C"
