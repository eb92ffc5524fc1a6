// The proof container's framing (include/eon_prove.h, "proof bytes"): header, section table and the
// overflow-checked size.  Header-only and free of every other include of the driver, so a tool or a
// sanitizer build reads a header with nothing else linked (tests/proofio_check.cpp).
//
//   offset  0  magic  "EONPRF1\0"
//           8  u32    version = 1
//          12  u32    flags: bit 0 batched opening, bit 1 preprocessed part, bit 2 permutation part
//          16  u32    degree_bits
//          20  u32    W, C, Wp, Wq   (Wp / Wq zero exactly when their flag is clear)
//          36  u32    zero
//          40  u64    body length
//          48  body: the sections below in order, every G1 32 compressed bytes, every Fr its 32 raw
//              eon_fr bytes; all integers little-endian
#pragma once
#include <stdint.h>
#include <string.h>

namespace eon_host {
namespace proofio {

constexpr uint64_t HEADER_BYTES = 48;
constexpr uint64_t ELEM_BYTES = 32;
constexpr uint32_t VERSION = 1;
constexpr uint32_t FLAG_BATCHED = 1, FLAG_PREPROCESSED = 2, FLAG_PERMUTATION = 4, FLAG_ALL = 7;
constexpr unsigned char MAGIC[8] = {'E', 'O', 'N', 'P', 'R', 'F', '1', 0};

struct Shape {
    uint32_t flags, degree_bits, width, chunks, pre_width, perm_width;
};

// reasons and sections: the values of EON_PROOF_IO_* / EON_PROOF_SECTION_* (eon_prove.h)
enum Reason : uint32_t {
    OK = 0, BAD_MAGIC = 1, BAD_VERSION = 2, BAD_FLAGS = 3, BAD_LENGTH = 4, FR_NOT_CANONICAL = 5, G1_ENCODING = 6,
    G1_NOT_CANONICAL = 7, G1_NOT_ON_CURVE = 8
};
enum Section : uint32_t {
    HEADER = 0,
    TRACE_COMMIT, PERMUTATION_COMMIT, QUOTIENT_COMMIT,                                    // G1
    TRACE_LOCAL, TRACE_NEXT, PERMUTATION_LOCAL, PERMUTATION_NEXT, PREPROCESSED_LOCAL,     // Fr
    PREPROCESSED_NEXT, QUOTIENT_OPENED,
    TRACE_WITNESS_ZETA, TRACE_WITNESS_NEXT, PERMUTATION_WITNESS_ZETA, PERMUTATION_WITNESS_NEXT,  // G1
    QUOTIENT_WITNESS, PREPROCESSED_WITNESS_ZETA, PREPROCESSED_WITNESS_NEXT,
    SECTIONS
};
inline bool section_is_g1(uint32_t s) { return s != HEADER && (s < TRACE_LOCAL || s > QUOTIENT_OPENED); }

inline bool shape_ok(const Shape& s) {
    if (s.flags & ~FLAG_ALL) return false;
    if ((s.pre_width != 0) != ((s.flags & FLAG_PREPROCESSED) != 0)) return false;
    if ((s.perm_width != 0) != ((s.flags & FLAG_PERMUTATION) != 0)) return false;
    return true;
}

// elements of every section (count[HEADER] = 0); the witness arrays of a matrix hold its width in
// the per-column mode and one point in the batched mode, none when the part is absent
inline void section_counts(const Shape& s, uint64_t count[SECTIONS]) {
    const bool batched = (s.flags & FLAG_BATCHED) != 0;
    const uint64_t W = s.width, C = s.chunks, Wp = s.pre_width, Wq = s.perm_width;
    const uint64_t tw = batched ? 1 : W, qw = batched ? (Wq ? 1 : 0) : Wq, pw = batched ? (Wp ? 1 : 0) : Wp;
    const uint64_t c[SECTIONS] = {0, W, Wq, C, W, W, Wq, Wq, Wp, Wp, C, tw, tw, qw, qw, C, pw, pw};
    memcpy(count, c, sizeof(c));
}

// the body's length from the shape, every step overflow-checked; false on an invalid shape
inline bool body_bytes(const Shape& s, uint64_t* out) {
    if (!shape_ok(s)) return false;
    uint64_t count[SECTIONS], n = 0;
    section_counts(s, count);
    for (uint32_t k = 0; k < SECTIONS; k++)
        if (__builtin_add_overflow(n, count[k], &n)) return false;
    return !__builtin_mul_overflow(n, ELEM_BYTES, out);
}

inline bool total_bytes(const Shape& s, uint64_t* out) {
    uint64_t body;
    return body_bytes(s, &body) && !__builtin_add_overflow(body, HEADER_BYTES, out);
}

inline uint32_t load_u32(const uint8_t* p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
inline uint64_t load_u64(const uint8_t* p) { return (uint64_t)load_u32(p) | (uint64_t)load_u32(p + 4) << 32; }
inline void store_u32(uint8_t* p, uint32_t v) {
    for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
}
inline void store_u64(uint8_t* p, uint64_t v) {
    for (int k = 0; k < 8; k++) p[k] = (uint8_t)(v >> (8 * k));
}

// the 48 header bytes of a valid shape (body = body_bytes(s))
inline void write_header(const Shape& s, uint64_t body, uint8_t out[HEADER_BYTES]) {
    memcpy(out, MAGIC, 8);
    store_u32(out + 8, VERSION);
    store_u32(out + 12, s.flags);
    store_u32(out + 16, s.degree_bits);
    store_u32(out + 20, s.width);
    store_u32(out + 24, s.chunks);
    store_u32(out + 28, s.pre_width);
    store_u32(out + 32, s.perm_width);
    store_u32(out + 36, 0);
    store_u64(out + 40, body);
}

// Header and length of `len` bytes at `data`: reads data[0, min(len, 48)) and nothing else, allocates
// nothing.  OK fills *shape, and then 48 + body_bytes(*shape) == len exactly.
inline Reason peek(const uint8_t* data, uint64_t len, Shape* shape) {
    if (len < HEADER_BYTES) return BAD_LENGTH;
    if (memcmp(data, MAGIC, 8) != 0) return BAD_MAGIC;
    if (load_u32(data + 8) != VERSION) return BAD_VERSION;
    Shape s;
    s.flags = load_u32(data + 12);
    s.degree_bits = load_u32(data + 16);
    s.width = load_u32(data + 20);
    s.chunks = load_u32(data + 24);
    s.pre_width = load_u32(data + 28);
    s.perm_width = load_u32(data + 32);
    if (!shape_ok(s) || load_u32(data + 36) != 0) return BAD_FLAGS;
    uint64_t body, total;
    if (!body_bytes(s, &body) || __builtin_add_overflow(body, HEADER_BYTES, &total)) return BAD_LENGTH;
    if (load_u64(data + 40) != body || total != len) return BAD_LENGTH;
    *shape = s;
    return OK;
}

}  // namespace proofio
}  // namespace eon_host
