// Blake3-AIR witness generation (generate_trace_rows, blake3-air/src/generation.rs:16-250) as one
// pure-store kernel: a row is 9168 Fr = 293,376 B, the arithmetic behind it one 7-round BLAKE3
// compression (56 quarter rounds on u32), so the kernel is laid out from the stores backwards.
//
// A workgroup owns one row, or one of `parts` equal slices of it when rows are few (each slice
// redoes the cheap compression).  The first wave runs the compression, lane i & 3 owning column i of
// the 4x4 state: a half round is three adds, two xors and two rotates per lane, the step from
// columns to diagonals and back three 4-lane shuffles, and the message schedule one nibble lookup a
// round (MSG_PERMUTATION is applied to the lane's four word indices, not to the words).  Lanes 0..3
// leave the row as 504 u32 words in LDS, in Blake3Cols order (columns.rs):
//
//   word   0..15   inputs[16]                         bits    columns    0..511
//         16..23   chaining_values[2][4]              bits             512..767
//         24..27   counter_low, counter_hi, block_len, flags   bits    768..895
//         28..31   initial_row0[4]                    limbs            896..903
//         32..35   initial_row2[4]                    limbs            904..911
//         36 + 16 s, s = 4 round + {prime, middle, middle_prime, output}:     912 + 272 s
//            +0..3   row0[4]                          limbs             +0..7
//            +4..7   row1[4]                          bits              +8..135
//            +8..11  row2[4]                          limbs           +136..143
//            +12..15 row3[4]                          bits            +144..271
//        484..487  final_round_helpers[4]             bits            8528..8655
//        488..503  outputs[4][4]                      bits            8656..9167
//
// A state is two halves of 136 columns (4 limb words, then 4 bit words), so a round column is
// (word, bit) or (word, limb) by one division by the constant 136 (a multiply and a shift) and two
// compares.  Then all 256 threads sweep the slice in column order: thread t of pass k writes
// 16-byte half 256 k + t, so a wave instruction is one global_store_dwordx4 over 1 KiB of contiguous
// bytes; no thread walks a column.  A bit cell is 0 or the Montgomery one, a limb cell from_u64 of a
// 16-bit value (canonical).  Byte offsets are 64-bit: a 2^14-row trace is 4.8 GB.
#include "context.h"

using namespace eon;

namespace {

constexpr uint32_t BLAKE3_ROUNDS = 7;
constexpr uint32_t BLAKE3_COLS = 9168;
constexpr uint32_t ROW_HALVES = 2 * BLAKE3_COLS;  // 16-byte halves of one row
constexpr uint32_t SWEEP_THREADS = 256;
constexpr uint32_t MAX_LOG_PARTS = 4;

// first column of each Blake3Cols field past the leading bit words, and a state's half
constexpr uint32_t COL_INIT = 896, COL_ROUNDS = 912, COL_HELPERS = 8528, HALF_STATE_COLS = 136;
// first LDS word of each field
constexpr uint32_t W_INPUTS = 0, W_ROW3 = 24, W_INIT0 = 28, W_INIT2 = 32, W_ROUNDS = 36, W_HELPERS = 484,
                   W_OUTPUTS = 488, W_COUNT = 504;
static_assert(COL_ROUNDS + BLAKE3_ROUNDS * 8 * HALF_STATE_COLS == COL_HELPERS && COL_HELPERS + 20 * 32 == BLAKE3_COLS,
              "Blake3Cols");
static_assert(W_ROUNDS + BLAKE3_ROUNDS * 4 * 16 == W_HELPERS && W_OUTPUTS + 16 == W_COUNT, "row words");

// BLAKE3's IV (the SHA-256 initial hash values), of which the compression reads the first four
constexpr uint32_t IV0 = 0x6A09E667, IV1 = 0xBB67AE85, IV2 = 0x3C6EF372, IV3 = 0xA54FF53A;

// MSG_PERMUTATION (constants.rs:27) as sixteen nibbles: word i of the next round is word P[i] of this one
constexpr uint64_t pack_permutation() {
    constexpr uint8_t p[16] = {2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8};
    uint64_t v = 0, seen = 0;
    for (uint32_t i = 0; i < 16; i++) {
        v |= (uint64_t)p[i] << (4 * i);
        seen |= 1ull << p[i];
    }
    return seen == 0xffff ? v : 0;
}
constexpr uint64_t MSG_PERMUTATION = pack_permutation();
static_assert(MSG_PERMUTATION != 0 && (MSG_PERMUTATION & 15) == 2 && (MSG_PERMUTATION >> 60) == 8, "a permutation");

__device__ __forceinline__ uint32_t permuted(uint32_t i) { return (uint32_t)(MSG_PERMUTATION >> (4 * i)) & 15; }
__device__ __forceinline__ uint32_t rotr32(uint32_t v, uint32_t n) { return (v >> n) | (v << (32 - n)); }

// verifiable_half_round (generation.rs:206-230)
template <uint32_t R1, uint32_t R2>
__device__ __forceinline__ void half_round(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t m) {
    a = a + b + m;
    d = rotr32(d ^ a, R1);
    c = c + d;
    b = rotr32(b ^ c, R2);
}

__global__ void __launch_bounds__(SWEEP_THREADS)
    k_blake3_trace(const uint32_t* __restrict__ inputs, uint32_t n_hashes, uint32_t log_parts, uint4* __restrict__ trace) {
    __shared__ uint32_t words[W_COUNT];
    const uint32_t t = threadIdx.x;
    const uint64_t row = blockIdx.x >> log_parts;
    const uint32_t part = blockIdx.x & ((1u << log_parts) - 1);

    if (t < 24) words[W_INPUTS + t] = inputs[row * 24 + t];  // inputs, then chaining_values
    __syncthreads();

    if (t < 64) {  // one whole wave, so that the shuffles see no inactive lane; lanes 0..3 store
        const uint32_t i = t & 3, i1 = (i + 1) & 3, i2 = (i + 2) & 3, i3 = (i + 3) & 3;
        const bool owner = t < 4;
        const uint32_t cv_lo = words[16 + i], cv_hi = words[20 + i];
        uint32_t a = cv_lo, b = cv_hi;
        uint32_t c = i == 0 ? IV0 : i == 1 ? IV1 : i == 2 ? IV2 : IV3;
        uint32_t d = i == 0 ? (uint32_t)row : i == 1 ? (uint32_t)(row >> 32) : i == 2 ? n_hashes : 0;  // flags = 0
        if (owner) {
            words[W_ROW3 + i] = d;
            words[W_INIT0 + i] = a;
            words[W_INIT2 + i] = c;
        }
        uint32_t k0 = 2 * i, k1 = 2 * i + 1, k2 = 2 * i + 8, k3 = 2 * i + 9;  // the lane's four message words
#pragma unroll
        for (uint32_t r = 0; r < BLAKE3_ROUNDS; r++) {
            uint32_t* st = words + W_ROUNDS + 64 * r;
            half_round<16, 12>(a, b, c, d, words[k0]);
            if (owner) st[i] = a, st[4 + i] = b, st[8 + i] = c, st[12 + i] = d;  // state_prime
            half_round<8, 7>(a, b, c, d, words[k1]);
            if (owner) st[16 + i] = a, st[20 + i] = b, st[24 + i] = c, st[28 + i] = d;  // state_middle
            // diagonal i: state[0][i], state[1][i + 1], state[2][i + 2], state[3][i + 3]
            b = __shfl(b, i1, 4);
            c = __shfl(c, i2, 4);
            d = __shfl(d, i3, 4);
            half_round<16, 12>(a, b, c, d, words[k2]);
            if (owner) st[32 + i] = a, st[36 + i1] = b, st[40 + i2] = c, st[44 + i3] = d;  // state_middle_prime
            half_round<8, 7>(a, b, c, d, words[k3]);
            if (owner) st[48 + i] = a, st[52 + i1] = b, st[56 + i2] = c, st[60 + i3] = d;  // state_output
            b = __shfl(b, i3, 4);  // back to columns: lane i - 1 holds state[1][i]
            c = __shfl(c, i2, 4);
            d = __shfl(d, i1, 4);
            k0 = permuted(k0), k1 = permuted(k1), k2 = permuted(k2), k3 = permuted(k3);
        }
        if (owner) {
            words[W_HELPERS + i] = c;
            words[W_OUTPUTS + i] = a ^ c;
            words[W_OUTPUTS + 4 + i] = b ^ d;
            words[W_OUTPUTS + 8 + i] = c ^ cv_lo;
            words[W_OUTPUTS + 12 + i] = d ^ cv_hi;
        }
    }
    __syncthreads();

    // the slice of this part: whole 1-KiB wave stores, the last part takes what remains
    const uint32_t per_part = (((ROW_HALVES + (1u << log_parts) - 1) >> log_parts) + 63) & ~63u;
    const uint32_t begin = part * per_part;
    const uint32_t end = begin + per_part < ROW_HALVES ? begin + per_part : ROW_HALVES;
    const Fr one = Fr::one();
    uint4* out = trace + row * (uint64_t)ROW_HALVES;
    for (uint32_t h = begin + t; h < end; h += SWEEP_THREADS) {
        const uint32_t col = h >> 1, hi = h & 1;
        uint32_t w, idx;
        bool limb;
        if (col < COL_INIT) {
            w = col >> 5, idx = col & 31, limb = false;
        } else if (col < COL_ROUNDS) {
            w = W_INIT0 + ((col - COL_INIT) >> 1), idx = col & 1, limb = true;
        } else if (col < COL_HELPERS) {
            const uint32_t c = col - COL_ROUNDS, half = c / HALF_STATE_COLS, r = c - half * HALF_STATE_COLS;
            limb = r < 8;
            w = W_ROUNDS + 8 * half + (limb ? r >> 1 : 4 + ((r - 8) >> 5));
            idx = limb ? r & 1 : (r - 8) & 31;
        } else {
            w = W_HELPERS + ((col - COL_HELPERS) >> 5), idx = (col - COL_HELPERS) & 31, limb = false;
        }
        const uint32_t v = words[w];
        Fr cell;
        if (limb) {
            cell = from_u64<FrP>((v >> (16 * idx)) & 0xffff);
        } else {
            cell = (v >> idx) & 1 ? one : Fr::zero();
        }
        out[h] = hi ? make_uint4(cell.v[4], cell.v[5], cell.v[6], cell.v[7])
                    : make_uint4(cell.v[0], cell.v[1], cell.v[2], cell.v[3]);
    }
}

int finish(eon_ctx* ctx, const Status& s) {
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

// Rows are few: below 2048 workgroups (8 to a CU) a row is cut into up to 16 slices
uint32_t auto_log_parts(uint64_t n_rows) {
    uint32_t lp = 0;
    while (lp < MAX_LOG_PARTS && (n_rows << lp) < 2048) lp++;
    return lp;
}

Status generate(eon_ctx* ctx, const uint32_t* inputs, uint64_t n_hashes, eon_fr* trace, uint64_t n_rows, uint32_t parts) {
    if (n_hashes == 0 || (n_hashes & (n_hashes - 1)))
        return Status::err(EON_E_SHAPE, "n_hashes must be a power of two, at least 1 (generation.rs:21-24)");
    if (n_rows != n_hashes) return Status::err(EON_E_SHAPE, "n_rows must equal n_hashes: one compression per row");
    if (n_rows > (1ull << 28)) return Status::err(EON_E_SHAPE, "trace height exceeds 2^28 (Fr::TWO_ADICITY)");
    if (parts & (parts - 1) || parts > (1u << MAX_LOG_PARTS))
        return Status::err(EON_E_SHAPE, "parts must be 0 (chosen by the library) or a power of two up to 16");
    if (!inputs || !trace) return Status::err(EON_E_ARG, "null argument");
    uint32_t log_parts = auto_log_parts(n_rows);
    if (parts) {
        log_parts = 0;
        while ((1u << log_parts) < parts) log_parts++;
    }
    if ((n_rows << log_parts) > (1ull << 30)) return Status::err(EON_E_SHAPE, "n_rows x parts exceeds 2^30 workgroups");
    ctx->prof.begin("k_blake3_trace", n_rows * (uint64_t)BLAKE3_COLS * 32, ctx->stream);
    hipLaunchKernelGGL(k_blake3_trace, dim3((unsigned)(n_rows << log_parts)), dim3(SWEEP_THREADS), 0, ctx->stream, inputs,
                       (uint32_t)n_hashes, log_parts, reinterpret_cast<uint4*>(trace));
    ctx->prof.end(ctx->stream);
    EON_HIP(hipGetLastError());
    return Status::ok();
}

}  // namespace

extern "C" {

uint32_t eon_blake3_air_width(void) { return BLAKE3_COLS; }

int eon_blake3_generate_trace_dev(eon_ctx* ctx, const uint32_t* inputs, uint64_t n_hashes, eon_fr* trace,
                                  uint64_t n_rows) {
    return eon_diag_blake3_trace_parts(ctx, inputs, n_hashes, trace, n_rows, 0);
}

int eon_diag_blake3_trace_parts(eon_ctx* ctx, const uint32_t* inputs, uint64_t n_hashes, eon_fr* trace, uint64_t n_rows,
                                uint32_t parts) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    return finish(ctx, generate(ctx, inputs, n_hashes, trace, n_rows, parts));
}

}  // extern "C"
