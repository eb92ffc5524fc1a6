// Keccak-AIR witness generation (generate_trace_rows, keccak-air/src/generation.rs:17-137) as one
// pure-store kernel: a row is 2633 Fr = 84,256 B, the arithmetic behind it 25 lanes of xor, rotate
// and and-not, so the kernel is laid out from the stores backwards.
//
// One workgroup per trace row (row = 24 perm + round).  Threads 0..24 own one lane (x, y) of the
// state each and run rounds 0..round of the row's permutation through LDS (two barriers a round:
// A' out, A''' out); re-running the <= 23 earlier rounds is ~25 lanes x a few dozen instructions
// against the row's 5266 16-byte stores.  The last round leaves the row's values as u64 words in
// LDS, in KeccakCols order (columns.rs:18-61):
//
//   word   0..24   preimage[y][x]      limbs   columns   25..124
//         25..49   a[y][x]             limbs            125..224
//         50..54   c[x]                bits             225..544
//         55..59   c_prime[x]          bits             545..864
//         60..84   a_prime[y][x]       bits             865..2464
//         85..109  a_prime_prime[y][x] limbs           2465..2564
//        110       a''[0][0]           bits            2565..2628
//        111       a'''[0][0]          limbs           2629..2632
//        112       1 << round          bits               0..24   (step_flags, export = 0)
//
// so a column is (word, bit) or (word, 16-bit limb) by five compares.  Then all 256 threads sweep
// the row in column order: thread t of pass k writes 16-byte half 256 k + t of the row, so a wave
// instruction is one global_store_dwordx4 over 1 KiB of contiguous bytes; no thread walks a column.
// A bit cell is 0 or the Montgomery one, a limb cell from_u64 of a 16-bit value (canonical).  Byte
// offsets are 64-bit: a 2^16-row trace is 5.5 GB.
//
// The reference transmutes the [u64; 25] input to a state it indexes [x][y] (generation.rs:50-53):
// lane (x, y) starts from input[5x + y], and preimage[y][x] holds that lane.
#include "context.h"

using namespace eon;

namespace {

constexpr uint32_t KECCAK_ROUNDS = 24;
constexpr uint32_t KECCAK_COLS = 2633;
constexpr uint32_t ROW_HALVES = 2 * KECCAK_COLS;  // 16-byte halves of one row
constexpr uint32_t SWEEP_THREADS = 256;

// first column of each KeccakCols field
constexpr uint32_t COL_PREIMAGE = 25, COL_C = 225, COL_APP = 2465, COL_APP00_BITS = 2565, COL_APPP = 2629;
// first LDS word of each field
constexpr uint32_t W_PREIMAGE = 0, W_A = 25, W_C = 50, W_CP = 55, W_AP = 60, W_APP = 85, W_APP00 = 110,
                   W_APPP = 111, W_FLAGS = 112, W_COUNT = 113;

// FIPS 202 3.2.2: the rho offsets r[x][y] = (t + 1)(t + 2) / 2 mod 64 along (x, y) -> (y, 2x + 3y)
// from (1, 0)
struct RhoOffsets {
    uint8_t r[25];  // [5x + y]
};

constexpr RhoOffsets make_rho_offsets() {
    RhoOffsets k{};
    uint32_t x = 1, y = 0;
    for (uint32_t t = 0; t < 24; t++) {
        k.r[5 * x + y] = (uint8_t)(((t + 1) * (t + 2) / 2) % 64);
        const uint32_t ny = (2 * x + 3 * y) % 5;
        x = y;
        y = ny;
    }
    return k;
}

// FIPS 202 3.2.5, algorithm 5: the next round's iota constant, RC[ir] bit 2^j - 1 = rc(j + 7 ir), from
// the LFSR x^8 + x^6 + x^5 + x^4 + 1; `lfsr` starts at 1 and is carried from round to round
__host__ __device__ constexpr uint64_t next_iota(uint32_t& lfsr) {
    uint64_t rc = 0;
    for (uint32_t j = 0; j < 7; j++) {
        if (lfsr & 1) rc |= 1ull << ((1u << j) - 1);
        lfsr <<= 1;
        if (lfsr & 0x100) lfsr ^= 0x171;
    }
    return rc;
}

constexpr uint64_t iota_of_round(uint32_t ir) {
    uint32_t lfsr = 1;
    uint64_t rc = 0;
    for (uint32_t i = 0; i <= ir; i++) rc = next_iota(lfsr);
    return rc;
}

constexpr RhoOffsets RHO_HOST = make_rho_offsets();
static_assert(iota_of_round(0) == 1 && iota_of_round(1) == 0x8082 && iota_of_round(23) == 0x8000000080008008ull,
              "iota constants");
static_assert(RHO_HOST.r[5] == 1 && RHO_HOST.r[1] == 36 && RHO_HOST.r[10] == 62 && RHO_HOST.r[24] == 14 &&
                  RHO_HOST.r[0] == 0,
              "rho offsets");

__constant__ RhoOffsets RHO = make_rho_offsets();

__device__ __forceinline__ uint64_t rotl64(uint64_t v, uint32_t n) { return (v << n) | (v >> ((64 - n) & 63)); }

__global__ void __launch_bounds__(SWEEP_THREADS)
    k_keccak_trace(const uint64_t* __restrict__ inputs, uint64_t n_hashes, uint4* __restrict__ trace) {
    __shared__ uint64_t words[W_COUNT];
    __shared__ uint64_t state[25], theta[25];  // [5x + y]: the round's input A, then A'
    const uint32_t t = threadIdx.x;
    const uint64_t row = blockIdx.x;
    const uint64_t perm = row / KECCAK_ROUNDS;
    const uint32_t round = (uint32_t)(row % KECCAK_ROUNDS);
    const uint32_t x = t / 5, y = t % 5;  // the lane of threads 0..24
    const bool lane = t < 25;
    const uint32_t yx = 5 * y + x;  // the lane's word inside a y-major field

    // B[i][y] = rotl(A'[a][i], r[a][i]), a = (i + 3y) mod 5, for i = x, x + 1, x + 2: where this
    // lane's three B values come from, and by how much they turn
    uint32_t b_src[3] = {0, 0, 0}, b_rot[3] = {0, 0, 0};
    if (lane) {
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const uint32_t i = (x + k) % 5;
            b_src[k] = 5 * ((i + 3 * y) % 5) + i;
            b_rot[k] = RHO.r[b_src[k]];
        }
    }
    uint32_t lfsr = 1;  // next_iota's state

    uint64_t s = 0;
    if (lane) {
        if (perm < n_hashes) s = inputs[perm * 25 + t];  // padding permutations: the zero input
        words[W_PREIMAGE + yx] = s;
        state[t] = s;
    }
    if (t == 0) words[W_FLAGS] = 1ull << round;
    __syncthreads();

    for (uint32_t r = 0; r <= round; r++) {
        const bool last = r == round;
        const uint64_t rc = next_iota(lfsr);
        if (lane) {
            // C[x] and its neighbours from the round's input, then C'[x] and A'[x][y]
            uint64_t c[3];
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                const uint32_t xx = (x + (k == 0 ? 0 : k == 1 ? 4 : 1)) % 5;
                uint64_t acc = 0;
#pragma unroll
                for (uint32_t yy = 0; yy < 5; yy++) acc ^= state[5 * xx + yy];
                c[k] = acc;
            }
            const uint64_t cp = c[0] ^ c[1] ^ rotl64(c[2], 1);
            const uint64_t ap = s ^ c[0] ^ cp;
            theta[t] = ap;
            if (last) {
                words[W_A + yx] = s;
                words[W_AP + yx] = ap;
                if (y == 0) {
                    words[W_C + x] = c[0];
                    words[W_CP + x] = cp;
                }
            }
        }
        __syncthreads();
        if (lane) {
            uint64_t b[3];
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) b[k] = rotl64(theta[b_src[k]], b_rot[k]);
            s = b[0] ^ (~b[1] & b[2]);  // A''[x][y]
            if (last) words[W_APP + yx] = s;
            if (t == 0) {
                if (last) words[W_APP00] = s;
                s ^= rc;  // A'''[0][0]
                if (last) words[W_APPP] = s;
            }
            state[t] = s;
        }
        __syncthreads();
    }

    const Fr one = Fr::one();
    uint4* out = trace + row * (uint64_t)ROW_HALVES;
    for (uint32_t h = t; h < ROW_HALVES; h += SWEEP_THREADS) {
        const uint32_t col = h >> 1, hi = h & 1;
        uint32_t w, idx;
        bool limb;
        if (col < COL_PREIMAGE) {
            w = W_FLAGS, idx = col, limb = false;
        } else if (col < COL_C) {
            w = W_PREIMAGE + ((col - COL_PREIMAGE) >> 2), idx = (col - COL_PREIMAGE) & 3, limb = true;
        } else if (col < COL_APP) {
            w = W_C + ((col - COL_C) >> 6), idx = (col - COL_C) & 63, limb = false;
        } else if (col < COL_APP00_BITS) {
            w = W_APP + ((col - COL_APP) >> 2), idx = (col - COL_APP) & 3, limb = true;
        } else if (col < COL_APPP) {
            w = W_APP00, idx = col - COL_APP00_BITS, limb = false;
        } else {
            w = W_APPP, idx = col - COL_APPP, limb = true;
        }
        const uint64_t v = words[w];
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

}  // namespace

extern "C" {

uint32_t eon_keccak_air_width(void) { return KECCAK_COLS; }

uint64_t eon_keccak_air_rows(uint64_t n_hashes) {
    if (n_hashes == 0 || n_hashes > (1ull << 58)) return 0;
    uint64_t rows = 1;
    while (rows < KECCAK_ROUNDS * n_hashes) rows <<= 1;
    return rows;
}

int eon_keccak_generate_trace_dev(eon_ctx* ctx, const uint64_t* inputs, uint64_t n_hashes, eon_fr* trace,
                                  uint64_t n_rows) {
    if (!ctx) return EON_E_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    Status s = [&]() -> Status {
        if (n_hashes == 0) return Status::err(EON_E_SHAPE, "n_hashes must be at least 1 (a 1-row trace has no next row)");
        if (n_rows != eon_keccak_air_rows(n_hashes))
            return Status::err(EON_E_SHAPE, "n_rows must be (24 n_hashes).next_power_of_two()");
        if (n_rows > (1ull << 28)) return Status::err(EON_E_SHAPE, "trace height exceeds 2^28 (Fr::TWO_ADICITY)");
        if (!inputs || !trace) return Status::err(EON_E_ARG, "null argument");
        ctx->prof.begin("k_keccak_trace", n_rows * (uint64_t)KECCAK_COLS * 32, ctx->stream);
        hipLaunchKernelGGL(k_keccak_trace, dim3((unsigned)n_rows), dim3(SWEEP_THREADS), 0, ctx->stream, inputs,
                           n_hashes, reinterpret_cast<uint4*>(trace));
        ctx->prof.end(ctx->stream);
        EON_HIP(hipGetLastError());
        return Status::ok();
    }();
    return finish(ctx, s);
}

}  // extern "C"
