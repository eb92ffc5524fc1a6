// Stand-alone check of the proof container's header parser (plonky3_eon_amd/host/proof_io.h), meant
// to be built with -fsanitize=address,undefined: every buffer is a heap block of exactly the length
// peek is told, so a read outside it is an error of the sanitizer, and for every mutated header peek
// must either reject or return a shape whose size is the buffer's length.
//
//   proofio_check [mutations]     prints "ok <cases> <accepted> <rejected>" and exits 0, or says
//                                 what went wrong and exits 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "proof_io.h"

namespace pio = eon_host::proofio;

static uint64_t cases = 0, accepted = 0, rejected = 0;

// peek on a private, exactly sized copy; false when an acceptance contradicts the length
static bool run(const uint8_t* data, uint64_t len, const char* what, long k) {
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(buf, data, len);
    pio::Shape s;
    const pio::Reason r = pio::peek(buf, len, &s);
    free(buf);
    cases++;
    if (r != pio::OK) {
        rejected++;
        return true;
    }
    accepted++;
    uint64_t total = 0;
    if (!pio::total_bytes(s, &total) || total != len) {
        printf("FAIL %s %ld: accepted, but the shape's size is %llu and the buffer has %llu bytes\n", what, k,
               (unsigned long long)total, (unsigned long long)len);
        return false;
    }
    return true;
}

int main(int argc, char** argv) {
    const long mutations = argc > 1 ? atol(argv[1]) : 2000;
    bool ok = true;
    const pio::Shape shapes[] = {{0, 3, 3, 2, 0, 0},
                                 {pio::FLAG_BATCHED | pio::FLAG_PREPROCESSED | pio::FLAG_PERMUTATION, 4, 5, 4, 2, 1},
                                 {pio::FLAG_PERMUTATION, 3, 3, 2, 0, 1}};
    for (const pio::Shape& shape : shapes) {
        uint64_t body = 0, total = 0;
        if (!pio::body_bytes(shape, &body) || !pio::total_bytes(shape, &total)) {
            printf("FAIL: a valid shape has no size\n");
            return 1;
        }
        uint8_t* good = (uint8_t*)calloc(total, 1);
        pio::write_header(shape, body, good);
        const uint64_t before = accepted;
        ok = run(good, total, "unchanged", 0) && ok;
        if (accepted != before + 1) {
            printf("FAIL: the valid buffer was rejected\n");
            ok = false;
        }
        // one byte short, and every length below the header's
        ok = run(good, total - 1, "short", 0) && ok;
        for (uint64_t len = 0; len < pio::HEADER_BYTES; len++) ok = run(good, len, "truncated header", (long)len) && ok;
        // single-byte mutations of the 48 header bytes: every position in turn, values from an LCG,
        // with the extremes that make a width or the stated length huge
        uint64_t lcg = 0x9e3779b97f4a7c15ull;
        uint8_t* bad = (uint8_t*)malloc(total);
        for (long k = 0; k < mutations; k++) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            const uint64_t pos = (uint64_t)k % pio::HEADER_BYTES;
            uint8_t v = (uint8_t)(lcg >> 56);
            if (k % 5 == 0) v = 0xff;
            if (k % 7 == 0) v = 0x80;
            if (v == good[pos]) v ^= 1;
            memcpy(bad, good, total);
            bad[pos] = v;
            ok = run(bad, total, "mutation", k) && ok;
        }
        // widths whose sum times 32 is as large as the fields allow, and a stated length of 2^64 - 1:
        // the size arithmetic must reject, not wrap
        for (int m = 0; m < 16; m++) {
            memcpy(bad, good, total);
            for (int f = 0; f < 4; f++)
                if (m >> f & 1) pio::store_u32(bad + 20 + 4 * f, 0xffffffffu);
            pio::store_u32(bad + 12, pio::FLAG_ALL);
            if (m & 1) pio::store_u64(bad + 40, ~0ull);
            ok = run(bad, total, "huge widths", m) && ok;
        }
        free(bad);
        free(good);
    }
    // the size arithmetic itself: an invalid shape has none
    uint64_t n = 0;
    if (pio::body_bytes(pio::Shape{8, 0, 1, 1, 0, 0}, &n) || pio::body_bytes(pio::Shape{0, 0, 1, 1, 1, 0}, &n) ||
        pio::body_bytes(pio::Shape{pio::FLAG_PERMUTATION, 0, 1, 1, 0, 0}, &n)) {
        printf("FAIL: an invalid shape has a size\n");
        ok = false;
    }
    if (!pio::body_bytes(pio::Shape{pio::FLAG_ALL, 0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, &n) ||
        n != 32ull * (11ull * 0xffffffffull + 6ull)) {  // batched: 3 W + 3 Wq + 2 Wp + 3 C and six witnesses
        printf("FAIL: the largest shape's size is wrong (%llu)\n", (unsigned long long)n);
        ok = false;
    }
    if (!ok) return 1;
    printf("ok %llu %llu %llu\n", (unsigned long long)cases, (unsigned long long)accepted,
           (unsigned long long)rejected);
    return 0;
}
