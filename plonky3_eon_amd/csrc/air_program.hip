// Generic AIR quotient: quotient_values (eon-uni-stark/src/prover.rs:539-709) for ANY AIR whose
// constraints arrive as the symbolic DAG get_symbolic_constraints returns
// (eon-uni-stark/src/symbolic_builder.rs:72-126; SymbolicExpression, symbolic_expression.rs:78-145).
//
// Host side (eon_air_program_create): the DAG is value-numbered (hash-consing: identical leaves,
// constants by value, commutative + and * with sorted operands), scheduled constraint by
// constraint in the folder's order (each constraint's not-yet-computed sub-DAG in post-order, then
// its ASSERT), and register-allocated by liveness (a register is reused right after its last read).
// Leaves are operand modes, not instructions: trace column of the local / next row, a constant
// (program constants, then the public values), a selector.  A preprocessed column
// (Entry::Preprocessed, symbolic_variable.rs:8-15; the folder's second window, folder.rs:25-40) is
// the same local / next mode with its index past the main width: index W + c reads column c of the
// second matrix `pre_lde` (Wp columns, same quotient coset, same row pair, prover.rs:677).
// degree_multiple follows symbolic_expression.rs:171-190, get_log_quotient_degree
// symbolic_builder.rs:15-43.
//
// Device side (k_air_quotient): one thread per quotient-domain row i runs the program with its
// row window (local = row i, next = row (i + 2^qd) mod Q, vertically_packed_row_pair,
// matrix/src/lib.rs:392-411), the selectors of selectors_on_coset at i, and the folder's
// accumulator as a Horner chain acc = acc * alpha + C_k (folder.rs:81-85 with the reversed alpha
// powers of prover.rs:578-579), stepped two constraints at a time (acc alpha^2 + C_k alpha +
// C_k+1: two limb products, one Montgomery reduction).  out[i] = acc * inv_vanishing[i] (prover.rs:699).  Every lane of
// a wave executes the same instruction (uniform program counter: scalar instruction fetch, the next
// instruction's fetch issued before the current one executes, no divergence).  A value read only
// by the next instruction is forwarded in registers (operand mode M_PREV, no register-file round
// trip).  Arithmetic is radix 2^29 with compiler-tracked value bounds (below).  Registers 0 and 1
// live in VGPRs, the rest in LDS (three planes: two 16-byte, one 4-byte; conflict-free accesses)
// sized by the program's register count, or in a global buffer for very large programs.
//
// Structure: ONE interpreter (fetch, exec1, run_program over a Window and a MemRegs file) and FIVE
// drivers, kernels that differ only in the rows they hand it and in what an ASSERT does (the
// Window's Sink):
//   k_air_quotient  quotient domain, next = row (i + 2^qd) mod Q, coset selectors, ASSERTs folded;
//   k_air_quotient_rows  the same on n_rows quotient rows from row0, read from a WINDOW matrix
//                   that holds rows row0 .. row0 + n_rows + 2^qd (mod Q) of the LDE (the
//                   column-sharded prove, shard_exchange.hip): next = window row t + 2^qd, no wrap;
//   k_lookup_terms  trace domain, next = row (i + 1) mod height, no selectors, no permutation
//                   matrix; ASSERT k emits the lookups' k-th denominator or multiplicity;
//   k_air_check     trace domain, all three matrices, 0 / 1 selectors synthesised from the row; every
//                   ASSERT tested for zero mod p, reduced to the first failure and the counts
//                   (check_constraints, eon-uni-stark/src/check_constraints.rs:22-101);
//   k_air_point     the verifier's: one evaluation on six opened rows at an out-of-domain point,
//                   selectors_at_point, ASSERTs folded.
// What they share is written once: make_window builds every Window, reg_file every register file;
// on the host check_args validates what the entry points take alike, plan_regs alone decides block
// size, register-file mode and dynamic LDS, and launch_air picks the (mode, PRE, PERM) instance
// and launches it.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "field29.h"
#include "quotient.h"

using namespace eon;

namespace {

enum : uint32_t { OP_ADD = 0, OP_SUB = 1, OP_MUL = 2, OP_NEG = 3, OP_ASSERT = 4, OP_NOP = 5, OP_SQR = 6 };
// OP_SQR: a product of a value by itself (x * x after hash-consing), sqr29's 45 limb products
// instead of 81
// op word: opcode (bits 0-3) | OP_RED (the result is brought below 2p by reduce_top29) | K << K_SHIFT
// (OP_SUB / OP_NEG: the multiple of p added, at least the subtrahend's bound)
constexpr uint32_t OP_MASK = 0xf, OP_RED = 0x10, K_SHIFT = 8;
// OP_ASSERT's kind (in the K field): the constraints are folded in pairs, acc alpha^2 + C_k alpha +
// C_k+1 with one reduction (mul29_sum2): the first of a pair is held (AS_PEND), the second folds
// both (AS_PAIR).  With an odd count the first constraint opens the chain alone (AS_INIT: acc = C,
// acc alpha + C from acc = 0).
enum : uint32_t { AS_INIT = 0, AS_PEND = 1, AS_PAIR = 2 };
// Value bounds.  Every value is held in radix 2^29 as x 2^261 ("29-Montgomery", field29.h) with
// normalised limbs and a value below B p, B tracked per value by the compiler: products B = 2, a
// sum B_a + B_b, a difference B_a + K.  A result whose bound would exceed B_MAX is reduced in the
// same instruction (OP_RED: reduce_top29, B = 2), so every computed operand is below B_MAX p; with
// the raw leaves below (OPND_RAW) every product stays below 160 p^2, inside mul29's 167 p^2, and a
// reduced input below 64 p < 2^261.  The folder's accumulator stays below (2 + B_RAW) p.
constexpr uint32_t B_MAX = 12;
// A leaf (trace cell, constant, selector) is loaded either reduced (shl5_to261, B = 2) or raw
// (shl5_raw, B = 32: the reduction skipped) -- chosen per use by the compiler (OPND_RAW): raw
// wherever the reader allows it (a sum or difference, whose result is reduced anyway when it
// exceeds B_MAX, a constraint value, one side of a product whose other side is < 5p), so a
// two-leaf sum costs one reduction instead of two.  The subtrahend multiple K then reaches 32.
constexpr uint32_t B_RAW = 32, K_MAX = 32;
// Registers 0 and 1 -- the busiest: the allocator hands out the lowest free register -- are held in
// VGPRs, the others in LDS (36 bytes each, MemRegs).  At the Poseidon2-AIR's 5 registers and 256
// threads per block that is 27 KB of LDS per block instead of 45, so occupancy is set by the VGPRs
// (4 waves per SIMD) instead of the LDS (3).  Measured (round 4, profiles/r04/s13): all registers
// in LDS 15.6 ms, one in VGPRs 13.6, two 12.9; three spill; 64- or 128-thread blocks and a
// 5-wave launch bound (spills) are slower or equal.
constexpr uint32_t AIR_VREGS = 2, AIR_BLOCK = 256;
// operand = mode << 29 | index
enum : uint32_t { M_REG = 0, M_LOCAL = 1, M_NEXT = 2, M_CONST = 3, M_FIRST = 4, M_LAST = 5, M_TRANS = 6, M_PREV = 7 };
constexpr uint32_t OPND_RAW = 1u << 28, IDX_MASK = (1u << 28) - 1;
constexpr uint32_t NO_DST = ~0u;  // result only forwarded to the next instruction (M_PREV)

struct Instr {
    uint32_t op, dst, a, b;
};

// K p in normalised 29-bit limbs for K <= K_MAX (OP_SUB / OP_NEG); K is uniform, so its row is
// read with scalar loads
struct KpTable {
    uint32_t l[K_MAX + 1][9];
    constexpr KpTable() : l{} {
        for (uint32_t k = 0; k <= K_MAX; k++) {
            uint64_t c = 0;
            for (int i = 0; i < 9; i++) {
                c += (uint64_t)R29<FrP>::P[i] * k;
                l[k][i] = (uint32_t)(c & M29);
                c >>= 29;
            }
        }
    }
};
__device__ constexpr KpTable KP_TABLE{};

// a - b + K p, normalised (b < K p; a, b normalised: the signed column sums stay inside int32)
__device__ __forceinline__ F29 sub29_k(const F29& a, const F29& b, uint32_t k) {
    const uint32_t* kp = KP_TABLE.l[k];
    F29 r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const int32_t t = (int32_t)(a.l[i] + kp[i]) - (int32_t)b.l[i] + c;
        r.l[i] = (uint32_t)t & M29;
        c = t >> 29;  // arithmetic: -1, 0 or 1
    }
    return r;
}

__device__ __forceinline__ F29 zero29() {
    F29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = 0;
    return r;
}

// a trace cell, constant or selector (canonical, x 2^256) as x 2^261: below 2p, or below 32p
// unreduced when the operand is marked raw (the flag is uniform: a scalar branch)
__device__ __forceinline__ F29 ld29(const Fr* p, bool raw) {
    const F29 x = shl5_raw<FrP>(ld_pinned(p));
    return raw ? x : reduce_top29<FrP>(x);
}

// register file in LDS or in a global buffer: 36 bytes per register in three planes (limbs 0-3
// and 4-7 as 16-byte planes, limb 8 as a 4-byte one), conflict-free b128 / b32 accesses
struct MemRegs {
    uint4* base;     // plane j of register r at (2 r + j) stride
    uint32_t* top;   // limb 8 of register r at r stride
    uint64_t stride;
    __device__ __forceinline__ F29 get(uint32_t r) const {
        const uint4 a = base[(uint64_t)(2 * r) * stride], b = base[(uint64_t)(2 * r + 1) * stride];
        F29 x;
        x.l[0] = a.x; x.l[1] = a.y; x.l[2] = a.z; x.l[3] = a.w;
        x.l[4] = b.x; x.l[5] = b.y; x.l[6] = b.z; x.l[7] = b.w;
        x.l[8] = top[(uint64_t)r * stride];
        return x;
    }
    __device__ __forceinline__ void set(uint32_t r, const F29& x) {
        base[(uint64_t)(2 * r) * stride] = make_uint4(x.l[0], x.l[1], x.l[2], x.l[3]);
        base[(uint64_t)(2 * r + 1) * stride] = make_uint4(x.l[4], x.l[5], x.l[6], x.l[7]);
        top[(uint64_t)r * stride] = x.l[8];
    }
};
// The file of the n_regs - AIR_VREGS registers kept in memory, as lane `slot` of `stride` sees it.
// MODE 0: in LDS (slot = the thread, stride = the block); 1: in the global buffer `gregs` (slot =
// the row, stride = the rows of the launch, so a wave's accesses are contiguous).
template <int MODE>
__device__ __forceinline__ MemRegs reg_file(uint32_t n_regs, uint4* lds, uint4* gregs, uint64_t slot,
                                            uint64_t stride) {
    const uint32_t n_mem = n_regs > AIR_VREGS ? n_regs - AIR_VREGS : 0;
    uint4* const mem = MODE == 0 ? lds : gregs;
    return MemRegs{mem + slot, reinterpret_cast<uint32_t*>(mem + 2ull * n_mem * stride) + slot, stride};
}

// PRE: the program reads preprocessed columns.  Without them the kernel is the one-matrix kernel,
// instruction for instruction (the second matrix's compare and select are compiled out: measured at
// +1 % on the Poseidon2-AIR when left in)
// PERM: the program reads permutation (LogUp running-sum) columns, a third matrix through the same
// row pair: a local / next index >= W + Wp is permutation column index - (W + Wp).  Compiled out
// likewise when absent.
// Sink: what an ASSERT does, chosen at compile time (exec1).  FoldSink: the folder's Horner chain
// (the quotient, the out-of-domain point); EmitSink: the value is stored (the lookup terms);
// CheckSink: it is tested for zero, and the selectors are synthesised from the row.
struct FoldSink {
    static constexpr bool terms = false, check = false;
};
template <bool PRE, bool PERM, class Sink = FoldSink>
struct Window : Sink {
    static constexpr bool has_pre = PRE, has_perm = PERM;
    const Fr* local;
    const Fr* next;
    const Fr* pre_local;  // the preprocessed matrix's row pair (PRE only)
    const Fr* pre_next;
    const Fr* perm_local;  // the permutation matrix's row pair (PERM only)
    const Fr* perm_next;
    uint32_t width;       // main width W: a local / next index >= W is preprocessed column index - W
    uint32_t perm_base;   // W + Wp (PERM only)
    const F29* table;  // program constants, then public values: x 2^261 (< 2p), converted on the host
    // is_first_row | is_last_row | is_transition, q each (null if unused).  The term and check
    // kernels never read it (a term that reaches a selector is refused at compile time; the check
    // synthesises its selectors in fetch) and pass a valid address, the trace
    const Fr* sels;
    uint64_t row, q;  // q: the rows of the domain (the quotient domain; the trace height; 1)
};

// The one way to build a window: row `row` of the three "local" matrices and row `next_row` of the
// three "next" ones (row-major, widths width / pre_width / perm_width).  The matrix kernels take
// both rows from the same matrix and pass it twice; k_air_point passes its six opened rows with
// row = next_row = 0.  Field by field in this order: the PERM instances keep the window in
// scratch, and their code follows the order of these stores.
template <bool PRE, bool PERM, class Sink = FoldSink>
__device__ __forceinline__ Window<PRE, PERM, Sink> make_window(const Fr* local, const Fr* next, const Fr* pre_local,
                                                               const Fr* pre_next, const Fr* perm_local,
                                                               const Fr* perm_next, uint32_t width, uint32_t pre_width,
                                                               uint32_t perm_width, uint64_t row, uint64_t next_row,
                                                               uint64_t q, const F29* table, const Fr* sels,
                                                               const Sink& sink = Sink{}) {
    Window<PRE, PERM, Sink> w;
    static_cast<Sink&>(w) = sink;
    w.local = local + row * width;
    w.next = next + next_row * width;
    w.pre_local = PRE ? pre_local + row * pre_width : nullptr;
    w.pre_next = PRE ? pre_next + next_row * pre_width : nullptr;
    w.perm_local = PERM ? perm_local + row * perm_width : nullptr;
    w.perm_next = PERM ? perm_next + next_row * perm_width : nullptr;
    w.width = width;
    w.perm_base = PERM ? width + pre_width : 0;
    w.table = table;
    w.sels = sels;
    w.row = row;
    w.q = q;
    return w;
}

// the registers held in VGPRs: register j < AIR_VREGS is hj (named values, not an array: an array
// indexed by the register number went to scratch); the register number is uniform, so the choice
// is a scalar branch
static_assert(AIR_VREGS <= 4, "at most four registers in VGPRs");
struct Hot {
    F29 h0, h1, h2, h3;
};
__device__ __forceinline__ bool hot_get(const Hot& h, uint32_t i, F29& x) {
    if (i >= AIR_VREGS) return false;
    // limb-wise value selects (a branch per register was merged into a load through a selected
    // pointer, which put the registers in scratch)
#pragma unroll
    for (int k = 0; k < 9; k++) {
        uint32_t v = h.h0.l[k];
        if (AIR_VREGS > 1) v = i == 1 ? h.h1.l[k] : v;
        if (AIR_VREGS > 2) v = i == 2 ? h.h2.l[k] : v;
        if (AIR_VREGS > 3) v = i == 3 ? h.h3.l[k] : v;
        x.l[k] = v;
    }
    return true;
}
__device__ __forceinline__ bool hot_set(Hot& h, uint32_t i, const F29& x) {
    if (i >= AIR_VREGS) return false;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        h.h0.l[k] = i == 0 ? x.l[k] : h.h0.l[k];
        if (AIR_VREGS > 1) h.h1.l[k] = i == 1 ? x.l[k] : h.h1.l[k];
        if (AIR_VREGS > 2) h.h2.l[k] = i == 2 ? x.l[k] : h.h2.l[k];
        if (AIR_VREGS > 3) h.h3.l[k] = i == 3 ? x.l[k] : h.h3.l[k];
    }
    return true;
}

// One load site for every trace-cell / selector mode and one second-operand fetch per slot: the
// kernel body (four slots written out) is 61 KB instead of 103 (round 6; the instruction cache hit
// 99.7 % before, and the time did not change: 11.69 vs 11.64 ms, profiles/r06/s7)

template <class RF, class Win>
__device__ __forceinline__ F29 fetch(uint32_t opnd, const RF& rf, const F29& prev, const Hot& hot, const Win& w) {
    const uint32_t i = opnd & IDX_MASK;
    const bool raw = (opnd & OPND_RAW) != 0;
    const uint32_t m = opnd >> 29;
    if (m == M_PREV) return prev;
    if (m == M_CONST) return w.table[i];  // uniform index: scalar loads, no conversion
    if (m == M_REG) {
        F29 x;
        if (hot_get(hot, i, x)) return x;
        return rf.get(i - AIR_VREGS);
    }
    if constexpr (Win::check) {
        // the trace-domain selectors are the field elements 1 / 0 (check_constraints.rs:88-90),
        // synthesised from the row: no table, no load
        if (m >= M_FIRST) {
            const bool one = m == M_FIRST ? w.row == 0 : m == M_LAST ? w.row + 1 == w.q : w.row + 1 != w.q;
            F29 s;
#pragma unroll
            for (int k = 0; k < 9; k++) s.l[k] = one ? R29<FrP>::ONE[k] : 0u;
            return s;
        }
    }
    // local / next row cell (of the main or the preprocessed matrix: the index is uniform, so
    // which one is a scalar compare) or a selector: the address picked by the (uniform) mode, one
    // load
    const Fr* p;
    if constexpr (Win::has_perm) {
        const bool perm = i >= w.perm_base;
        const bool pre = Win::has_pre && !perm && i >= w.width;
        const uint32_t col = perm ? i - w.perm_base : pre ? i - w.width : i;
        p = m == M_LOCAL ? (perm ? w.perm_local : pre ? w.pre_local : w.local) + col
            : m == M_NEXT ? (perm ? w.perm_next : pre ? w.pre_next : w.next) + col
                          : w.sels + (uint64_t)(m - M_FIRST) * w.q + w.row;
    } else {
        const bool pre = Win::has_pre && i >= w.width;
        const uint32_t col = pre ? i - w.width : i;
        p = m == M_LOCAL ? (pre ? w.pre_local : w.local) + col
            : m == M_NEXT ? (pre ? w.pre_next : w.next) + col
                          : w.sels + (uint64_t)(m - M_FIRST) * w.q + w.row;
    }
    return ld29(p, raw);
}

// The program is fetched in blocks of CODE_BLOCK instructions (one 64-byte scalar load each; the
// device copy is padded with OP_NOP to a whole block), the next block's load issued before the
// current block runs: the program (~130 KB for the Poseidon2-AIR) does not fit the scalar cache, so
// every fetch is an L2 round trip that an instruction-at-a-time loop waits on.
constexpr uint32_t CODE_BLOCK = 4;
struct CodeBlock {
    Instr i[CODE_BLOCK];
};

// The four slots of a block are unrolled, each with its own product per op kind.  One shared body
// (the slot's words picked by scalar selects, one product for MUL and ASSERT) measured slower,
// 15.8 vs 14.8 ms for the Poseidon2-AIR at 2^18 rows (round 4, profiles/r04/s7): not kept.
template <class RF, class Win>
__device__ __forceinline__ void exec1(const Instr& in, RF& rf, const Win& w, const F29& alpha,
                                      const F29& alpha2, F29& acc, F29& pend, F29& prev, Hot& hot) {
    const uint32_t opc = in.op & OP_MASK;
    if (opc == OP_NOP) return;
    const F29 x = fetch(in.a, rf, prev, hot, w);
    if constexpr (Win::terms) {  // the term program (lookup terms): an ASSERT emits root K
        if (opc == OP_ASSERT) {
            w.emit(in.op >> K_SHIFT, x);
            return;
        }
    }
    if constexpr (Win::check) {  // check_constraints: an ASSERT is tested for zero mod p, not folded
        if (opc == OP_ASSERT) {
            w.test(x);
            return;
        }
    } else if (opc == OP_ASSERT) {  // folder.rs:81-85, alpha powers reversed
        const uint32_t kind = in.op >> K_SHIFT;
        if (kind == AS_PAIR)  // acc < 34p, pend < 32p: acc alpha^2 + pend alpha < 132 p^2
            acc = add29_lazy(mul29_sum2_u<FrP>(alpha2, acc, alpha, pend), x);
        else if (kind == AS_PEND)
            pend = x;
        else
            acc = x;
        return;
    }
    F29 r;
    if (opc == OP_SQR) {
        r = sqr29<FrP>(x);
    } else {
        F29 a = x, b;
        if (opc == OP_NEG) {  // 0 - x + K p
            b = x;
            a = zero29();
        } else {
            b = fetch(in.b, rf, prev, hot, w);
        }
        if (opc == OP_MUL) {
            r = mul29<FrP>(a, b);
        } else {
            r = opc == OP_ADD ? add29_norm(a, b) : sub29_k(a, b, in.op >> K_SHIFT);
            if (in.op & OP_RED) r = reduce_top29<FrP>(r);
        }
    }
    prev = r;
    if (in.dst == NO_DST || hot_set(hot, in.dst, r)) return;
    rf.set(in.dst - AIR_VREGS, r);
}

template <class RF, class Win>
__device__ __forceinline__ void run_program(const CodeBlock* __restrict__ code, uint32_t n_blocks, RF& rf,
                                            const Win& w, const F29& alpha, F29& acc) {
    if (n_blocks == 0) return;
    const F29 alpha2 = uniform29(sqr29<FrP>(alpha));
    F29 prev, pend;
    Hot hot;
#pragma unroll
    for (int i = 0; i < 9; i++) prev.l[i] = pend.l[i] = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) hot.h0.l[i] = hot.h1.l[i] = hot.h2.l[i] = hot.h3.l[i] = 0;
    CodeBlock nx = code[0];
    for (uint32_t bk = 0; bk < n_blocks; bk++) {
        const CodeBlock cur = nx;
        if (bk + 1 < n_blocks) nx = code[bk + 1];  // in flight while this block runs
        // the four slots written out: a loop over them is left rolled by the compiler at this body
        // size, and the block then goes through scratch to be indexed
        auto slot = [&](const Instr& raw) __attribute__((always_inline)) {
            const Instr in{(uint32_t)__builtin_amdgcn_readfirstlane(raw.op),
                           (uint32_t)__builtin_amdgcn_readfirstlane(raw.dst),
                           (uint32_t)__builtin_amdgcn_readfirstlane(raw.a),
                           (uint32_t)__builtin_amdgcn_readfirstlane(raw.b)};
            exec1(in, rf, w, alpha, alpha2, acc, pend, prev, hot);
        };
        static_assert(CODE_BLOCK == 4, "four slots below");
        slot(cur.i[0]);
        slot(cur.i[1]);
        slot(cur.i[2]);
        slot(cur.i[3]);
    }
}

// MODE 0: registers in LDS; 1: in the global buffer `gregs` (n_regs 36-byte registers per row).
// PRE: with the preprocessed matrix `pre_lde` (pre_width columns); otherwise both are unused.
// PERM: with the permutation matrix `perm_lde` (perm_width columns), likewise (a program with
// permutation columns runs the PRE instance whatever its preprocessed width).
template <int MODE, bool PRE, bool PERM>
__global__ void __launch_bounds__(AIR_BLOCK) k_air_quotient(const CodeBlock* __restrict__ code, uint32_t n_blocks,
                                                      uint32_t n_regs, const Fr* __restrict__ lde, uint32_t width,
                                                      const Fr* __restrict__ pre_lde, uint32_t pre_width,
                                                      const Fr* __restrict__ perm_lde, uint32_t perm_width,
                                                      uint64_t q, uint64_t next_step, const F29* __restrict__ table,
                                                      const Fr* __restrict__ sels, const Fr* __restrict__ inv_van,
                                                      uint32_t nr_mask, Fr alpha, Fr* __restrict__ out,
                                                      uint4* __restrict__ gregs) {
    extern __shared__ uint4 lds_regs[];
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= q) return;
    const uint64_t next_row = (row + next_step) & (q - 1);
    const auto w = make_window<PRE, PERM>(lde, lde, pre_lde, pre_lde, perm_lde, perm_lde, width, pre_width, perm_width,
                                          row, next_row, q, table, sels);
    // written out here and in run_program, not zero29(): with the helper the six instances of this
    // kernel come out scheduled and allocated differently (6 to 12 instructions of 6500 to 6800)
    F29 acc;
#pragma unroll
    for (int i = 0; i < 9; i++) acc.l[i] = 0;
    MemRegs rf = reg_file<MODE>(n_regs, lds_regs, gregs, MODE == 0 ? threadIdx.x : row, MODE == 0 ? blockDim.x : q);
    run_program(code, n_blocks, rf, w, uniform29(shl5_to261<FrP>(alpha)), acc);
    // acc (x 2^261, < (2 + B_RAW) p, limbs < 2^30) times inv_vanishing in the ABI form: x 2^261 y 2^256 2^-261
    // = x y 2^256 (prover.rs:699)
    const F29 r = mul29<FrP>(acc, unpack29(ld_pinned(inv_van + (row & nr_mask))));
    st_vec(out + row, pack29<FrP>(canon29<FrP>(r)));
}

// The quotient on a block of rows (the column-sharded prove: every rank evaluates its own rows of
// the quotient domain after the ranks exchanged their columns as row blocks).  `window` holds the
// n_rows + next_step LDE rows (row0 + j) mod q, j < n_rows + next_step, row-major: thread t runs
// the program with local = window row t and next = window row t + next_step (the wrap is in how the
// window was gathered), and everything indexed by the position in the domain -- the coset
// selectors, inv_vanishing -- is taken at the global row row0 + t.  out[t] is k_air_quotient's
// out[row0 + t], bit for bit.  Main trace only (no PRE / PERM instance).  The global register file
// is indexed by t over the n_rows of the launch.
template <int MODE>
__global__ void __launch_bounds__(AIR_BLOCK) k_air_quotient_rows(const CodeBlock* __restrict__ code, uint32_t n_blocks,
                                                           uint32_t n_regs, const Fr* __restrict__ window,
                                                           uint32_t width, uint64_t q, uint64_t next_step,
                                                           uint64_t row0, uint64_t n_rows,
                                                           const F29* __restrict__ table,
                                                           const Fr* __restrict__ sels,
                                                           const Fr* __restrict__ inv_van, uint32_t nr_mask, Fr alpha,
                                                           Fr* __restrict__ out, uint4* __restrict__ gregs) {
    extern __shared__ uint4 lds_regs[];
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows) return;
    const uint64_t row = row0 + t;  // < q: the host checks row0 + n_rows <= q
    auto w = make_window<false, false>(window, window, nullptr, nullptr, nullptr, nullptr, width, 0, 0, t,
                                       t + next_step, q, table, sels);
    w.row = row;  // the selectors' index
    F29 acc;
#pragma unroll
    for (int i = 0; i < 9; i++) acc.l[i] = 0;
    MemRegs rf =
        reg_file<MODE>(n_regs, lds_regs, gregs, MODE == 0 ? threadIdx.x : t, MODE == 0 ? blockDim.x : n_rows);
    run_program(code, n_blocks, rf, w, uniform29(shl5_to261<FrP>(alpha)), acc);
    const F29 r = mul29<FrP>(acc, unpack29(ld_pinned(inv_van + (row & nr_mask))));
    st_vec(out + t, pack29<FrP>(canon29<FrP>(r)));
}

// ---- LogUp permutation trace: per-row contributions (generate_permutation, lookup/src/logup.rs:379-562)
// The term program runs on the TRACE domain: local = row i, next = row (i + 1) mod height, no
// selectors, no permutation columns.  Its k-th root is emitted (not folded) as register k of a
// MemRegs file in global memory, in the interpreter's own form (x 2^261, < 32p): planes of `height`
// rows, so a wave's stores are contiguous.  lookup.hip brings them to canonical form.
struct EmitSink {
    static constexpr bool terms = true, check = false;
    MemRegs out;  // this row's view of the emitted values
    __device__ __forceinline__ void emit(uint32_t k, const F29& x) const {
        MemRegs o = out;
        o.set(k, x);
    }
};

// One thread per trace row: the term program writes the row's denominators (plane 2t) and
// multiplicities (plane 2t + 1); lookup.hip inverts and sums them.
template <int MODE, bool PRE>
__global__ void __launch_bounds__(AIR_BLOCK) k_lookup_terms(const CodeBlock* __restrict__ code, uint32_t n_blocks,
                                                        uint32_t n_regs, const Fr* __restrict__ trace, uint32_t width,
                                                        const Fr* __restrict__ pre, uint32_t pre_width,
                                                        uint64_t height, const F29* __restrict__ table,
                                                        uint32_t n_out, uint4* __restrict__ planes,
                                                        uint4* __restrict__ gregs) {
    extern __shared__ uint4 lds_regs[];
    const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= height) return;
    const uint64_t next_row = row + 1 == height ? 0 : row + 1;
    const EmitSink sink{
        MemRegs{planes + row, reinterpret_cast<uint32_t*>(planes + 2ull * n_out * height) + row, height}};
    const auto w = make_window<PRE, false>(trace, trace, pre, pre, nullptr, nullptr, width, pre_width, 0, row, next_row,
                                           height, table, trace, sink);
    MemRegs rf =
        reg_file<MODE>(n_regs, lds_regs, gregs, MODE == 0 ? threadIdx.x : row, MODE == 0 ? blockDim.x : height);
    F29 acc = zero29();
    run_program(code, n_blocks, rf, w, zero29(), acc);
}

// ---- check_constraints (eon-uni-stark/src/check_constraints.rs:22-101) ------------------------------
// The third way to run the program: on the TRACE domain (local = row i, next = row (i + 1) mod
// height, all three matrices), with the 0 / 1 row selectors (:88-90), every ASSERT tested for zero
// mod p in assert order (the reference's assert_zero, :182-190) instead of folded.
//
// The program counter is uniform, so the k-th ASSERT is reached by every lane at once and k is a
// uniform counter (the schedule emits the ASSERTs in constraint order).  Per ASSERT the fail flags
// are one ballot: its popcount goes to per_constraint[k] (one global vector atomic of lane 0, only
// when nonzero) and to the wave's total (uniform arithmetic: the sum of the lanes' own counts);
// each lane keeps its first failing k by a select.  After the program the lowest lane with a
// failure -- the wave's lowest row, so its lowest key row * num_constraints + k -- does one 64-bit
// atomic min, and lane 0 one 64-bit atomic add of the total.  No per-lane atomics, no branch on a
// lane's fail flag; lanes past the last row have returned and take part in no ballot.
//
// With `target` set (the second launch: one thread on the first failing row) nothing is counted and
// ASSERT `target`'s operand is stored as a canonical Fr in ABI form.
constexpr uint32_t NO_FAIL = ~0u;
struct CheckState {
    uint32_t k = 0;            // ordinal of the next ASSERT (uniform)
    uint32_t first = NO_FAIL;  // this lane's first failing constraint
    uint64_t total = 0;        // the wave's failures so far (uniform)
};
struct CheckSink {
    static constexpr bool terms = false, check = true;
    uint32_t target;  // NO_FAIL: count failures; else store that ASSERT's value
    uint32_t* per_constraint;
    Fr* value_out;
    mutable CheckState st;
    // x: the interpreter's lazy form (x 2^261, normalised limbs, < B_RAW p < 2^261).  reduce_top29
    // brings it below 2p, where zero mod p is {0, p}: a nonzero multiple of p is zero.
    __device__ __forceinline__ void test(const F29& x) const {
        const F29 r = reduce_top29<FrP>(x);
        const uint32_t k = st.k;
        st.k = k + 1;
        if (target != NO_FAIL) {  // uniform
            if (k == target)  // x 2^261 * 2^256 2^-261 = x 2^256, the ABI form
                st_vec(value_out, pack29<FrP>(canon29<FrP>(mul29<FrP>(r, const29<FrP>(R29<FrP>::TO256)))));
            return;
        }
        const bool fail = !is_zero_mod29<FrP>(r);
        const uint64_t mask = __ballot(fail);
        if (mask != 0) {  // uniform
            const uint32_t n = (uint32_t)__popcll(mask);
            st.total += n;
            if ((threadIdx.x & 63) == 0) atomicAdd(per_constraint + k, n);
        }
        st.first = (fail && st.first == NO_FAIL) ? k : st.first;
    }
};

// One thread per trace row row0 + t, t < n_rows (the check: row0 = 0, n_rows = height; the value
// launch: row0 = the failing row, n_rows = 1).  summary[0]: min key, summary[1]: failures.
// A partial wave exists only when n_rows < 64 (heights are powers of two): its live lanes are the
// low ones, so lane 0 is live in every wave that runs.
template <int MODE, bool PRE, bool PERM>
__global__ void __launch_bounds__(AIR_BLOCK) k_air_check(const CodeBlock* __restrict__ code, uint32_t n_blocks,
                                                     uint32_t n_regs, const Fr* __restrict__ trace, uint32_t width,
                                                     const Fr* __restrict__ pre, uint32_t pre_width,
                                                     const Fr* __restrict__ perm, uint32_t perm_width,
                                                     uint64_t height, const F29* __restrict__ table, uint64_t row0,
                                                     uint64_t n_rows, uint32_t target, uint32_t n_constraints,
                                                     uint32_t* __restrict__ per_constraint,
                                                     unsigned long long* __restrict__ summary,
                                                     Fr* __restrict__ value_out, uint4* __restrict__ gregs) {
    extern __shared__ uint4 lds_regs[];
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_rows) return;
    const uint64_t row = row0 + t;
    const uint64_t next_row = row + 1 == height ? 0 : row + 1;
    const auto w = make_window<PRE, PERM>(trace, trace, pre, pre, perm, perm, width, pre_width, perm_width, row,
                                          next_row, height, table, trace,
                                          CheckSink{target, per_constraint, value_out, {}});
    MemRegs rf =
        reg_file<MODE>(n_regs, lds_regs, gregs, MODE == 0 ? threadIdx.x : row, MODE == 0 ? blockDim.x : height);
    F29 acc = zero29();
    run_program(code, n_blocks, rf, w, zero29(), acc);
    if (target != NO_FAIL) return;
    const uint64_t any = __ballot(w.st.first != NO_FAIL);
    if (any != 0) {  // uniform
        const uint32_t lane = threadIdx.x & 63;
        if (lane == (uint32_t)__ffsll((long long)any) - 1)
            atomicMin(summary, (unsigned long long)(row * n_constraints + w.st.first));
        if (lane == 0) atomicAdd(summary + 1, (unsigned long long)w.st.total);
    }
}

// ---- the constraints at one out-of-domain point (verify_constraints, eon-uni-stark/src/verifier.rs:101-152)
// The fourth way to run the program: ONE evaluation, on opened values instead of matrix rows.  It is
// the quotient's Window over a one-row "domain" (q = 1, row = 0): local / next (and the preprocessed
// and permutation pairs) are six separate arrays, the selectors are the three Fr of
// selectors_at_point(zeta) (commit/src/domain.rs:237-246) computed exactly on the host and read
// through the same `sels` addressing (mode * q + row), and the folder is the same Horner chain
// acc = acc alpha + C (folder.rs:188-190).  One lane of one wave is live -- lane 0, as in
// k_air_check's value launch -- so every readfirstlane in the interpreter reads the live lane; the
// run is one dependent chain, latency-bound by construction.  out[0] = the folded accumulator,
// out[1] = folded * inv_vanishing (sels[3]), both canonical in the ABI form.
template <int MODE, bool PRE, bool PERM>
__global__ void __launch_bounds__(AIR_BLOCK) k_air_point(const CodeBlock* __restrict__ code, uint32_t n_blocks,
                                                     uint32_t n_regs, const Fr* __restrict__ local,
                                                     const Fr* __restrict__ next, const Fr* __restrict__ pre_local,
                                                     const Fr* __restrict__ pre_next,
                                                     const Fr* __restrict__ perm_local,
                                                     const Fr* __restrict__ perm_next, uint32_t width,
                                                     uint32_t pre_width, const F29* __restrict__ table,
                                                     const Fr* __restrict__ sels, Fr alpha, Fr* __restrict__ out,
                                                     uint4* __restrict__ gregs) {
    extern __shared__ uint4 lds_regs[];
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const auto w = make_window<PRE, PERM>(local, next, pre_local, pre_next, perm_local, perm_next, width, pre_width, 0,
                                          0, 0, 1, table, sels);
    // thread 0 of the block; in the global buffer one row, so the planes are contiguous
    MemRegs rf = reg_file<MODE>(n_regs, lds_regs, gregs, 0, MODE == 0 ? blockDim.x : 1);
    F29 acc = zero29();
    run_program(code, n_blocks, rf, w, uniform29(shl5_to261<FrP>(alpha)), acc);
    // acc: x 2^261, < (2 + B_RAW) p, limbs < 2^30.  Times 2^256 (a plain integer < p) it is
    // x 2^256, the ABI form; times inv_vanishing in the ABI form x y 2^256 (as k_air_quotient)
    const F29 folded = mul29<FrP>(acc, const29<FrP>(R29<FrP>::TO256));
    const F29 quot = mul29<FrP>(acc, unpack29(ld_pinned(sels + 3)));
    st_vec(out, pack29<FrP>(canon29<FrP>(folded)));
    st_vec(out + 1, pack29<FrP>(canon29<FrP>(quot)));
}

// k_air_point at many points: block i is the evaluation of proof i, one wave's lane 0 live exactly
// as above, so a batch costs one launch and the proofs run side by side.  Proof i's opened values
// are row i of `rows` (row_stride Fr): local | next | pre_local | pre_next | perm_local | perm_next;
// its four selectors are sels[4 i ..], its alpha alphas[i], its constant table (the program's
// constants, then its own publics and challenges) tables[i * table_stride ..], its results
// out[2 i], out[2 i + 1].  Registers: the block's own LDS, or row i of the n rows of `gregs`.
template <int MODE, bool PRE, bool PERM>
__global__ void __launch_bounds__(AIR_BLOCK) k_air_points(const CodeBlock* __restrict__ code, uint32_t n_blocks,
                                                      uint32_t n_regs, const Fr* __restrict__ rows,
                                                      uint64_t row_stride, uint32_t width, uint32_t pre_width,
                                                      uint32_t perm_width, const F29* __restrict__ tables,
                                                      uint32_t table_stride, const Fr* __restrict__ sels,
                                                      const Fr* __restrict__ alphas, Fr* __restrict__ out,
                                                      uint4* __restrict__ gregs) {
    extern __shared__ uint4 lds_regs[];
    if (threadIdx.x != 0) return;
    const uint32_t i = blockIdx.x;
    const Fr* const local = rows + (uint64_t)i * row_stride;
    const Fr* const pre = local + 2 * width;
    const Fr* const perm = pre + 2 * pre_width;
    const auto w = make_window<PRE, PERM>(local, local + width, pre, pre + pre_width, perm, perm + perm_width, width,
                                          pre_width, 0, 0, 0, 1, tables + (uint64_t)i * table_stride, sels + 4 * i);
    MemRegs rf = reg_file<MODE>(n_regs, lds_regs, gregs, MODE == 0 ? 0 : i, MODE == 0 ? blockDim.x : gridDim.x);
    F29 acc = zero29();
    run_program(code, n_blocks, rf, w, uniform29(shl5_to261<FrP>(ld_pinned(alphas + i))), acc);
    const F29 folded = mul29<FrP>(acc, const29<FrP>(R29<FrP>::TO256));
    const F29 quot = mul29<FrP>(acc, unpack29(ld_pinned(w.sels + 3)));
    st_vec(out + 2 * i, pack29<FrP>(canon29<FrP>(folded)));
    st_vec(out + 2 * i + 1, pack29<FrP>(canon29<FrP>(quot)));
}

}  // namespace

struct eon_air_program {
    eon_ctx* ctx = nullptr;
    uint32_t width = 0, pre_width = 0, n_public = 0, n_constraints = 0, max_degree = 0, n_regs = 0, n_consts = 0;
    uint32_t perm_width = 0, n_challenges = 0;
    bool uses_sels = false;
    // lookups (eon_air_program_create_lk): lookup l's terms are [term_off[l], term_off[l + 1]) and
    // its running sum is permutation column aux[l]; `terms` is the term program, whose k-th root
    // (an OP_ASSERT with K = k) is the denominator (k even) or the multiplicity (k odd) of term k / 2
    std::vector<uint32_t> term_off, aux;
    std::unique_ptr<eon_air_program> terms;
    bool terms_read_pre = false;
    DevBuf d_desc, d_terms, d_flag;
    std::vector<Instr> code;
    std::vector<Fr> consts;
    DevBuf d_code, d_table, d_sels, d_regs;
    DevBuf d_check;  // eon_check_constraints_dev: min key | failures | value | per-constraint counts
    DevBuf d_point;  // eon_air_eval_at_point_dev: the four selectors at zeta | the two results
    // eon_air_eval_at_points_dev, for n proofs: 4n selectors | 2n results | n alphas | n constant tables
    DevBuf d_points;
    std::vector<Fr> staged;  // host copy of the table for the current launch
    std::vector<F29> staged29;  // the same in the device's form (x 2^261, < 2p)
};

namespace {

int finish(eon_ctx* ctx, const Status& s) {
    if (s.bad()) ctx->last_error = s.msg;
    return s.code;
}

// the frame of an entry point: the context's lock and device around `body`, its Status kept for
// eon_ctx_last_error
template <class Body>
int with_ctx(eon_ctx* ctx, Body body) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (hipSetDevice(ctx->device) != hipSuccess) return EON_E_DEVICE;
    return finish(ctx, body());
}

// A matrix argument of an entry point, given exactly when the program has such columns.  `name`:
// as the entry's header spells it, for the message (null: the entry has no such argument); any /
// all: of its pointers, given; `hint` ends the message of a missing one.
struct MatArg {
    const char* name;
    bool any, all;
    const char* hint;
    static MatArg none() { return {nullptr, false, false, ""}; }
    static MatArg one(const char* name, const void* p, const char* hint = "") { return {name, !!p, !!p, hint}; }
    static MatArg pair(const char* name, const void* a, const void* b) { return {name, a || b, a && b, ""}; }
    Status check(bool has, const char* kind) const {
        if (!name || (has ? all : !any)) return Status::ok();
        return Status::err(EON_E_ARG, std::string("the program ") + (has ? "reads " : "has no ") + kind +
                                          " columns: " + name + (has ? " must not be null" : " must be null") +
                                          (has ? hint : ""));
    }
};

// What the entry points that run a program check alike, in this order: `missing` (a required
// pointer of the entry's own is null), the context, the permutation matrix, the challenge count,
// the preprocessed matrix, the public value count, the trace height (when the entry takes one).
Status check_args(const eon_ctx* ctx, const eon_air_program* prog, bool missing, const MatArg& perm,
                  const MatArg& pre, const eon_fr* publics, uint32_t n_public, const eon_fr* challenges,
                  uint32_t n_challenges, const uint64_t* height = nullptr) {
    if (missing || (n_public && !publics) || (n_challenges && !challenges))
        return Status::err(EON_E_ARG, "null argument");
    if (prog->ctx != ctx) return Status::err(EON_E_ARG, "program belongs to another context");
    EON_TRY(perm.check(prog->perm_width > 0, "permutation"));
    if (n_challenges != prog->n_challenges)
        return Status::err(EON_E_SHAPE, "challenge count differs from the program's");
    EON_TRY(pre.check(prog->pre_width > 0, "preprocessed"));
    if (n_public != prog->n_public) return Status::err(EON_E_SHAPE, "public value count differs from the program's");
    if (height && (*height == 0 || (*height & (*height - 1)) || *height > (1ull << 28)))
        return Status::err(EON_E_SHAPE, "trace height must be a power of two <= 2^28");
    return Status::ok();
}

// The register file of a launch over `rows` rows, for all four kernels: LDS (the block shrinks
// with the register count), or the program's global buffer for very large programs and with
// EON_AIR_REGS=global (for tests; read once per process).  MemRegs: 36 bytes per register in
// memory.  The only place that decides the block size, the mode and the dynamic LDS.
struct RegFile {
    uint32_t block = AIR_BLOCK;
    int mode = 0;  // 0: LDS, 1: global
    size_t shmem = 0;
};
Status plan_regs(eon_air_program* prog, uint64_t rows, RegFile* out) {
    const uint64_t per_thread = (uint64_t)(prog->n_regs > AIR_VREGS ? prog->n_regs - AIR_VREGS : 0) * 36;
    static const bool force_global = [] {
        const char* e = getenv("EON_AIR_REGS");
        return e && std::string(e) == "global";
    }();
    RegFile r;
    while (r.block > 64 && r.block * per_thread > 64 * 1024) r.block /= 2;
    r.mode = !force_global && r.block * per_thread <= 160 * 1024 ? 0 : 1;
    if (r.mode != 0) r.block = AIR_BLOCK;
    if (r.mode == 1) EON_HIP(prog->d_regs.ensure(std::max<uint64_t>(1, rows * per_thread)));
    r.shmem = r.mode == 0 ? (size_t)r.block * per_thread : 0;
    *out = r;
    return Status::ok();
}

uint32_t code_blocks(size_t n_instr) { return (uint32_t)((n_instr + CODE_BLOCK - 1) / CODE_BLOCK); }

// algorithmic 256-bit products of one run of the program: its multiplications and, where ASSERTs
// are folded, one acc * alpha each (additions, subtractions and negations are not products)
uint64_t products(const std::vector<Instr>& code, bool count_asserts) {
    uint64_t n = 0;
    for (const Instr& in : code) {
        const uint32_t opc = in.op & OP_MASK;
        n += (opc == OP_MUL || opc == OP_SQR || (count_asserts && opc == OP_ASSERT)) ? 1 : 0;
    }
    return n;
}

// the profiler's record of a launch (label null: not recorded)
struct Profile {
    const char* label;
    uint64_t bytes, mulmods;
};

// Launches one of the four kernels over `rows` rows: the first `n_blocks` code blocks of `run`
// with the register file `regs` planned for it.  `pick(mode, pre, perm)` names the kernel
// template's instance for three std::integral_constant; every instance of a template has the same
// function type, and every kernel takes (code, n_blocks, n_regs, args..., gregs).
template <class Pick, class... Args>
Status launch_air(eon_ctx* ctx, const eon_air_program* run, const RegFile& regs, uint64_t rows, uint32_t n_blocks,
                  const Profile& prof, bool has_pre, bool has_perm, Pick pick, Args... args) {
    constexpr std::integral_constant<int, 0> LDS{};
    constexpr std::integral_constant<int, 1> GLOBAL{};
    constexpr std::true_type T{};
    constexpr std::false_type F{};
    // a program with permutation columns runs the PRE instance whatever its preprocessed width
    const auto kern = regs.mode == 0 ? (has_perm ? pick(LDS, T, T) : has_pre ? pick(LDS, T, F) : pick(LDS, F, F))
                                     : (has_perm  ? pick(GLOBAL, T, T)
                                        : has_pre ? pick(GLOBAL, T, F)
                                                  : pick(GLOBAL, F, F));
    if (regs.mode == 0)  // per launch: the attribute is per device, and this context's device may
                         // differ from the one another context set it on
        EON_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (prof.label) ctx->prof.begin(prof.label, prof.bytes, ctx->stream, prof.mulmods);
    hipLaunchKernelGGL(kern, dim3((unsigned)((rows + regs.block - 1) / regs.block)), dim3(regs.block), regs.shmem,
                       ctx->stream, run->d_code.as<CodeBlock>(), n_blocks, run->n_regs, args...,
                       regs.mode == 1 ? run->d_regs.as<uint4>() : nullptr);
    if (prof.label) ctx->prof.end(ctx->stream);
    EON_HIP(hipGetLastError());
    return Status::ok();
}

// the constant table of a launch: program constants ++ public values ++ challenges, in the device's
// form
Status stage_table(eon_ctx* ctx, eon_air_program* prog, const eon_fr* publics, uint32_t n_public,
                   const eon_fr* challenges, uint32_t n_challenges) {
    prog->staged.assign(prog->consts.begin(), prog->consts.end());
    for (uint32_t i = 0; i < n_public; i++) {
        const Fr v = fr_from_abi(&publics[i]);
        if (!fr_is_canonical(v)) return Status::err(EON_E_ARG, "public value is not a canonical Fr");
        prog->staged.push_back(v);
    }
    for (uint32_t i = 0; i < n_challenges; i++) {
        const Fr v = fr_from_abi(&challenges[i]);
        if (!fr_is_canonical(v)) return Status::err(EON_E_ARG, "challenge is not a canonical Fr");
        prog->staged.push_back(v);
    }
    if (!prog->staged.empty()) {
        prog->staged29.resize(prog->staged.size());
        for (size_t i = 0; i < prog->staged.size(); i++) prog->staged29[i] = shl5_to261<FrP>(prog->staged[i]);
        EON_HIP(hipMemcpyAsync(prog->d_table.p, prog->staged29.data(), prog->staged29.size() * sizeof(F29),
                               hipMemcpyHostToDevice, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));  // `staged` is reused by the next launch
    }
    return Status::ok();
}

// selectors_at_point of the trace domain of 2^log_n rows (shift 1), commit/src/domain.rs:237-246,
// exact on the host: Z_H = zeta^N - 1, out = is_first_row = Z_H / (zeta - 1) | is_last_row =
// Z_H / (zeta - h^-1) | is_transition = zeta - h^-1 | inv_vanishing = 1 / Z_H.  The reference panics
// (inverse of zero) where one of the three divisors vanishes.
Status selectors_at_point(uint32_t log_n, const Fr& z, Fr out[4]) {
    Fr zn = z;
    for (uint32_t i = 0; i < log_n; i++) zn = sqr(zn);
    const Fr z_h = sub(zn, Fr::one());
    const Fr h_inv = inverse(fr_two_adic_generator(log_n));
    const Fr d_first = sub(z, Fr::one()), d_last = sub(z, h_inv);
    if (z_h.is_zero() || d_first.is_zero() || d_last.is_zero())
        return Status::err(EON_E_ARG, "zeta lies on the trace domain: the selectors at zeta are undefined "
                                      "(the reference's inverse of zero)");
    out[0] = mul(z_h, inverse(d_first));
    out[1] = mul(z_h, inverse(d_last));
    out[2] = d_last;
    out[3] = inverse(z_h);
    return Status::ok();
}

void release_program(eon_air_program* p) {
    for (DevBuf* b : {&p->d_code, &p->d_table, &p->d_sels, &p->d_regs, &p->d_desc, &p->d_terms, &p->d_flag,
                      &p->d_check, &p->d_point, &p->d_points})
        b->release();
    if (p->terms) release_program(p->terms.get());
}

// compile nodes -> program; see the file comment
// term_mode: the roots are lookup terms, not constraints: root k's OP_ASSERT carries K = k (the
// kernel emits the value instead of folding it), and the roots may reach neither a permutation leaf
// nor a selector (*reads_pre: whether they reach a preprocessed leaf)
Status compile(eon_air_program* p, const eon_sym_node* nodes, uint32_t n_nodes, const eon_fr* consts,
               uint32_t n_consts, const uint32_t* roots, uint32_t n_roots, bool term_mode = false,
               bool* reads_pre = nullptr) {
    // operand indices are 28 bits (bit 28 is OPND_RAW): a wider main-column index, constant slot
    // or public slot would set the raw flag and read the wrong leaf
    // (the preprocessed columns share the local / next index space, after the main ones)
    if ((uint64_t)p->width + p->pre_width + p->perm_width > IDX_MASK ||
        (uint64_t)n_consts + p->n_public + p->n_challenges > IDX_MASK)
        return Status::err(EON_E_SHAPE, "trace width (main + preprocessed) and constant + public slots must each "
                                        "be < 2^28");
    // value numbering
    std::vector<uint32_t> vn(n_nodes);
    std::vector<uint32_t> degree(n_nodes);
    struct Val {
        uint32_t op;            // OP_* for computed values, ~0u for leaves
        uint32_t a, b;          // operand value numbers (computed) / operand code (leaf)
    };
    std::vector<Val> vals;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> memo;
    std::map<std::vector<uint32_t>, uint32_t> const_slot;  // canonical limbs -> table index
    auto intern = [&](uint32_t op, uint32_t a, uint32_t b) -> uint32_t {
        auto key = std::make_tuple(op, a, b);
        auto it = memo.find(key);
        if (it != memo.end()) return it->second;
        const uint32_t id = (uint32_t)vals.size();
        vals.push_back({op, a, b});
        memo.emplace(key, id);
        return id;
    };
    constexpr uint32_t LEAF = ~0u;
    for (uint32_t i = 0; i < n_nodes; i++) {
        const eon_sym_node& nd = nodes[i];
        auto operand = [&](uint32_t j) -> Status {
            if (j >= i) return Status::err(EON_E_ARG, "node " + std::to_string(i) + ": operand must precede it");
            return Status::ok();
        };
        switch (nd.kind) {
            case EON_SYM_CONSTANT: {
                if (nd.a >= n_consts) return Status::err(EON_E_ARG, "constant index out of range");
                const Fr c = fr_from_abi(&consts[nd.a]);
                if (!fr_is_canonical(c)) return Status::err(EON_E_ARG, "constant is not a canonical Fr");
                std::vector<uint32_t> key(c.v, c.v + 8);
                auto it = const_slot.find(key);
                uint32_t slot;
                if (it == const_slot.end()) {
                    slot = (uint32_t)p->consts.size();
                    p->consts.push_back(c);
                    const_slot.emplace(key, slot);
                } else {
                    slot = it->second;
                }
                vn[i] = intern(LEAF, M_CONST << 29 | slot, 0);
                degree[i] = 0;
                break;
            }
            case EON_SYM_MAIN:
                if (nd.a >= p->width || nd.b > 1) return Status::err(EON_E_ARG, "main variable out of range");
                vn[i] = intern(LEAF, (nd.b ? M_NEXT : M_LOCAL) << 29 | nd.a, 0);
                degree[i] = 1;
                break;
            case EON_SYM_PUBLIC:
                if (nd.a >= p->n_public) return Status::err(EON_E_ARG, "public value index out of range");
                vn[i] = intern(LEAF, 0xffffffffu, nd.a);  // resolved to a table slot below
                degree[i] = 0;
                break;
            case EON_SYM_IS_FIRST_ROW:
            case EON_SYM_IS_LAST_ROW:
            case EON_SYM_IS_TRANSITION: {
                const uint32_t m = nd.kind == EON_SYM_IS_FIRST_ROW ? M_FIRST
                                   : nd.kind == EON_SYM_IS_LAST_ROW ? M_LAST : M_TRANS;
                vn[i] = intern(LEAF, m << 29, 0);
                degree[i] = nd.kind == EON_SYM_IS_TRANSITION ? 0 : 1;
                break;
            }
            case EON_SYM_ADD:
            case EON_SYM_MUL: {
                EON_TRY(operand(nd.a));
                EON_TRY(operand(nd.b));
                uint32_t x = vn[nd.a], y = vn[nd.b];
                if (x > y) std::swap(x, y);  // commutative
                vn[i] = intern(nd.kind == EON_SYM_ADD ? OP_ADD : OP_MUL, x, y);
                degree[i] = nd.kind == EON_SYM_ADD ? std::max(degree[nd.a], degree[nd.b])
                                                   : degree[nd.a] + degree[nd.b];
                break;
            }
            case EON_SYM_SUB:
                EON_TRY(operand(nd.a));
                EON_TRY(operand(nd.b));
                vn[i] = intern(OP_SUB, vn[nd.a], vn[nd.b]);
                degree[i] = std::max(degree[nd.a], degree[nd.b]);
                break;
            case EON_SYM_NEG:
                EON_TRY(operand(nd.a));
                vn[i] = intern(OP_NEG, vn[nd.a], 0);
                degree[i] = degree[nd.a];
                break;
            case EON_SYM_PREPROCESSED:  // a trace leaf of the second matrix: index W + column
                if (nd.a >= p->pre_width || nd.b > 1)
                    return Status::err(EON_E_ARG, "preprocessed variable out of range (column " + std::to_string(nd.a) +
                                                      ", offset " + std::to_string(nd.b) + ", preprocessed width " +
                                                      std::to_string(p->pre_width) + ")");
                vn[i] = intern(LEAF, (nd.b ? M_NEXT : M_LOCAL) << 29 | (p->width + nd.a), 0);
                degree[i] = 1;
                break;
            case EON_SYM_PERMUTATION:  // a trace leaf of the third matrix: index W + Wp + column
                if (p->perm_width == 0)
                    return Status::err(EON_E_ARG, "permutation (LogUp) variables need a program with permutation "
                                                  "columns (eon_air_program_create_lk)");
                if (nd.a >= p->perm_width || nd.b > 1)
                    return Status::err(EON_E_ARG, "permutation variable out of range (column " + std::to_string(nd.a) +
                                                      ", offset " + std::to_string(nd.b) + ", permutation width " +
                                                      std::to_string(p->perm_width) + ")");
                vn[i] = intern(LEAF, (nd.b ? M_NEXT : M_LOCAL) << 29 | (p->width + p->pre_width + nd.a), 0);
                degree[i] = 1;
                break;
            case EON_SYM_CHALLENGE:  // a run-time constant after the public values
                if (nd.a >= p->n_challenges)
                    return Status::err(EON_E_ARG, p->n_challenges == 0
                                                      ? "challenge variables need a program with permutation "
                                                        "challenges (eon_air_program_create_lk)"
                                                      : "challenge index " + std::to_string(nd.a) +
                                                            " out of range (" + std::to_string(p->n_challenges) +
                                                            " challenges)");
                vn[i] = intern(LEAF, 0xffffffffu, p->n_public + nd.a);  // resolved to a table slot below
                degree[i] = 0;
                break;
            default:
                return Status::err(EON_E_ARG, "unknown node kind " + std::to_string(nd.kind));
        }
    }
    p->n_consts = (uint32_t)p->consts.size();
    // public values occupy the table slots after the constants
    for (auto& v : vals)
        if (v.op == LEAF && v.a == 0xffffffffu) v.a = M_CONST << 29 | (p->n_consts + v.b);
    for (auto& v : vals)
        if (v.op == LEAF) {
            const uint32_t m = v.a >> 29;
            if (m == M_FIRST || m == M_LAST || m == M_TRANS) p->uses_sels = true;
        }
    p->max_degree = 0;
    for (uint32_t k = 0; k < n_roots; k++) {
        if (roots[k] >= n_nodes)
            return Status::err(EON_E_ARG, term_mode ? "lookup term index out of range" : "constraint index out of range");
        p->max_degree = std::max(p->max_degree, degree[roots[k]]);
    }
    if (term_mode) {  // what the terms reach
        if (n_roots >= (1u << (32 - K_SHIFT))) return Status::err(EON_E_SHAPE, "more than 2^23 - 1 lookup terms");
        std::vector<char> seen_v(vals.size(), 0);
        std::vector<uint32_t> st;
        for (uint32_t k = 0; k < n_roots; k++) st.push_back(vn[roots[k]]);
        p->uses_sels = false;
        while (!st.empty()) {
            const uint32_t v = st.back();
            st.pop_back();
            if (seen_v[v]) continue;
            seen_v[v] = 1;
            if (vals[v].op != LEAF) {
                st.push_back(vals[v].a);
                if (vals[v].op != OP_NEG) st.push_back(vals[v].b);
                continue;
            }
            const uint32_t m = vals[v].a >> 29, idx = vals[v].a & IDX_MASK;
            if (m == M_FIRST || m == M_LAST || m == M_TRANS)
                return Status::err(EON_E_ARG, "a lookup denominator or multiplicity reads a row selector: refused "
                                              "(the reference evaluates selectors there as unnormalised 0 / 1)");
            if ((m == M_LOCAL || m == M_NEXT) && idx >= p->width + p->pre_width)
                return Status::err(EON_E_ARG, "a lookup denominator or multiplicity reads a permutation column");
            if ((m == M_LOCAL || m == M_NEXT) && idx >= p->width && reads_pre) *reads_pre = true;
        }
    }
    // schedule: per constraint, post-order of its not-yet-emitted values, then ASSERT
    const uint32_t nv = (uint32_t)vals.size();
    std::vector<uint32_t> order;  // emitted computed values
    std::vector<char> done(nv, 0);
    std::vector<std::pair<uint32_t, uint32_t>> asserts;  // (position in order, value)
    for (uint32_t k = 0; k < n_roots; k++) {
        std::vector<std::pair<uint32_t, bool>> st{{vn[roots[k]], false}};
        while (!st.empty()) {
            auto [v, ready] = st.back();
            st.pop_back();
            if (done[v] || vals[v].op == LEAF) continue;
            if (!ready) {
                st.push_back({v, true});
                const uint32_t kids[2] = {vals[v].a, vals[v].op == OP_NEG ? LEAF : vals[v].b};
                for (int t = 1; t >= 0; t--)
                    if (kids[t] != LEAF && !done[kids[t]] && vals[kids[t]].op != LEAF) st.push_back({kids[t], false});
                continue;
            }
            done[v] = 1;
            order.push_back(v);
        }
        asserts.push_back({(uint32_t)order.size(), vn[roots[k]]});
    }
    // instruction stream: computed values interleaved with asserts
    struct Item {
        bool assert_;
        uint32_t v;
    };
    std::vector<Item> items;
    {
        size_t ai = 0;
        for (uint32_t pos = 0; pos <= order.size(); pos++) {
            while (ai < asserts.size() && asserts[ai].first == pos) items.push_back({true, asserts[ai++].second});
            if (pos < order.size()) items.push_back({false, order[pos]});
        }
    }
    // liveness: last read of each computed value
    std::vector<int64_t> last(nv, -1);
    for (size_t t = 0; t < items.size(); t++) {
        const Item& it = items[t];
        if (it.assert_) {
            last[it.v] = (int64_t)t;
        } else {
            const Val& x = vals[it.v];
            last[x.a] = (int64_t)t;
            if (x.op != OP_NEG) last[x.b] = (int64_t)t;
        }
    }
    // forwarding: a value whose only reader is the very next item never touches the register
    // file (the kernel keeps the previous result in registers, operand mode M_PREV)
    std::vector<int64_t> first_read(nv, -1);
    std::vector<uint32_t> n_readers(nv, 0);
    {
        std::vector<int64_t> last_reader(nv, -1);
        for (size_t t = 0; t < items.size(); t++) {
            const Item& it = items[t];
            uint32_t rd[2] = {it.v, LEAF};
            if (!it.assert_) {
                rd[0] = vals[it.v].a;
                rd[1] = vals[it.v].op == OP_NEG ? LEAF : vals[it.v].b;
            }
            for (uint32_t v : rd) {
                if (v == LEAF || vals[v].op == LEAF || last_reader[v] == (int64_t)t) continue;
                last_reader[v] = (int64_t)t;
                n_readers[v]++;
                if (first_read[v] < 0) first_read[v] = (int64_t)t;
            }
        }
    }
    std::vector<size_t> pos_of(nv, 0);
    for (size_t t = 0; t < items.size(); t++)
        if (!items[t].assert_) pos_of[items[t].v] = t;
    auto forwarded = [&](uint32_t v) {
        return vals[v].op != LEAF && n_readers[v] == 1 && first_read[v] == (int64_t)pos_of[v] + 1;
    };
    // register allocation (lowest free register; operands freed before the result is assigned)
    std::vector<uint32_t> reg(nv, ~0u);
    std::vector<uint32_t> free_regs;
    uint32_t n_regs = 0;
    auto opnd = [&](uint32_t v) {
        if (vals[v].op == LEAF) return vals[v].a;
        return forwarded(v) ? (M_PREV << 29) : (M_REG << 29 | reg[v]);
    };
    auto release = [&](uint32_t v, size_t t) {
        if (vals[v].op != LEAF && last[v] == (int64_t)t && reg[v] != ~0u) {
            free_regs.push_back(reg[v]);
            std::sort(free_regs.begin(), free_regs.end(), std::greater<uint32_t>());
        }
    };
    // value bounds in multiples of p (see B_MAX): products 2, leaves 2 or B_RAW as loaded, sums
    // and differences add up, a result above B_MAX is reduced by its own instruction
    std::vector<uint32_t> bound(nv, 2);
    auto is_leaf = [&](uint32_t v) { return vals[v].op == LEAF; };
    auto is_tleaf = [&](uint32_t v) { return is_leaf(v) && (vals[v].a >> 29) != M_CONST; };
    // assert kinds: pairs from the end of the chain, so an odd count leaves the first one alone
    uint32_t n_asserts = 0, seen = 0;
    for (const Item& it : items) n_asserts += it.assert_ ? 1 : 0;
    for (size_t t = 0; t < items.size(); t++) {
        const Item& it = items[t];
        if (it.assert_) {  // constraint values: < B_RAW p (raw leaf) or < B_MAX p
            const uint32_t odd = n_asserts & 1;
            const uint32_t kind =
                term_mode ? seen : (odd && seen == 0) ? AS_INIT : ((seen - odd) % 2 == 0 ? AS_PEND : AS_PAIR);
            seen++;
            p->code.push_back({OP_ASSERT | kind << K_SHIFT, 0, opnd(it.v) | (is_tleaf(it.v) ? OPND_RAW : 0u), 0});
            release(it.v, t);
            continue;
        }
        const Val& x = vals[it.v];
        const bool unary = x.op == OP_NEG;
        // per use: the leaf operands raw unless a product's other side is too wide for it; constants
        // arrive reduced (the table is converted on the host), never raw
        bool raw_a = is_tleaf(x.a), raw_b = !unary && is_tleaf(x.b);
        const bool square = x.op == OP_MUL && x.a == x.b;  // sqr29: x < 12.9p, so never a raw leaf
        if (square) {
            raw_a = raw_b = false;
        } else if (x.op == OP_MUL) {
            if (raw_a && raw_b)
                raw_b = false;  // 32 x 2
            else if (raw_a && bound[x.b] * B_RAW > 160)
                raw_a = false;
            else if (raw_b && bound[x.a] * B_RAW > 160)
                raw_b = false;
        }
        const uint32_t ba = raw_a ? B_RAW : bound[x.a], bb = unary ? 0 : raw_b ? B_RAW : bound[x.b];
        uint32_t op = square ? OP_SQR : x.op, b = 2;
        if (x.op == OP_ADD) {
            b = ba + bb;
        } else if (x.op == OP_SUB) {
            op |= bb << K_SHIFT;  // + K p with K = the subtrahend's bound
            b = ba + bb;
        } else if (x.op == OP_NEG) {
            op |= ba << K_SHIFT;
            b = ba;
        }
        if (b > B_MAX) {
            op |= OP_RED;
            b = 2;
        }
        bound[it.v] = b;
        Instr in{op, 0, opnd(x.a) | (raw_a ? OPND_RAW : 0u),
                 (unary || square) ? 0u : opnd(x.b) | (raw_b ? OPND_RAW : 0u)};
        release(x.a, t);
        if (x.op != OP_NEG && x.b != x.a) release(x.b, t);
        if (last[it.v] < 0) continue;  // never read (cannot happen for reachable values)
        if (forwarded(it.v)) {
            in.dst = NO_DST;
            p->code.push_back(in);
            continue;
        }
        uint32_t r;
        if (!free_regs.empty()) {
            r = free_regs.back();
            free_regs.pop_back();
        } else {
            r = n_regs++;
        }
        reg[it.v] = r;
        in.dst = r;
        p->code.push_back(in);
    }
    p->n_regs = n_regs;
    if (n_regs > IDX_MASK) return Status::err(EON_E_SHAPE, "more than 2^28 - 1 registers");
    return Status::ok();
}

}  // namespace

extern "C" {

int eon_air_program_create_lk(eon_ctx* ctx, const eon_sym_node* nodes, uint32_t n_nodes, const eon_fr* consts,
                              uint32_t n_consts, const uint32_t* constraints, uint32_t n_constraints, uint32_t width,
                              uint32_t preprocessed_width, uint32_t n_public, uint32_t permutation_width,
                              uint32_t n_challenges, const eon_lookup_desc* lookups, uint32_t n_lookups,
                              const eon_lookup_term* terms, eon_air_program** out) {
    if (!ctx) return EON_E_ARG;
    return with_ctx(ctx, [&]() -> Status {
        if (!out || (n_nodes && !nodes) || (n_consts && !consts) || (n_constraints && !constraints) ||
            (n_lookups && !lookups))
            return Status::err(EON_E_ARG, "null argument");
        // LogUp: one auxiliary column and two challenges per lookup (logup.rs:266-273, prover.rs:93-94)
        if (n_challenges != 2 * (uint64_t)permutation_width)
            return Status::err(EON_E_ARG, "n_challenges must be 2 * permutation_width (" +
                                              std::to_string(n_challenges) + " challenges, permutation width " +
                                              std::to_string(permutation_width) + ")");
        if (n_lookups != 0 && n_lookups != permutation_width)
            return Status::err(EON_E_ARG, "the lookup description must cover every permutation column (" +
                                              std::to_string(n_lookups) + " lookups, permutation width " +
                                              std::to_string(permutation_width) + ")");
        auto p = std::make_unique<eon_air_program>();
        p->ctx = ctx;
        p->width = width;
        p->pre_width = preprocessed_width;
        p->n_public = n_public;
        p->n_constraints = n_constraints;
        p->perm_width = permutation_width;
        p->n_challenges = n_challenges;
        std::vector<uint32_t> term_roots;
        {
            std::vector<char> used(permutation_width, 0);
            uint64_t t = 0;
            for (uint32_t l = 0; l < n_lookups; l++) {
                const uint32_t c = lookups[l].aux_column;
                if (c >= permutation_width)
                    return Status::err(EON_E_ARG, "lookup " + std::to_string(l) + ": auxiliary column " +
                                                      std::to_string(c) + " >= permutation width " +
                                                      std::to_string(permutation_width));
                if (used[c])  // logup.rs:398-410
                    return Status::err(EON_E_ARG, "duplicate aux column index " + std::to_string(c) + " across lookups");
                used[c] = 1;
                if (lookups[l].n_terms && !terms) return Status::err(EON_E_ARG, "null argument");
                p->term_off.push_back((uint32_t)t);
                p->aux.push_back(c);
                for (uint32_t k = 0; k < lookups[l].n_terms; k++, t++) {
                    term_roots.push_back(terms[t].denominator);
                    term_roots.push_back(terms[t].multiplicity);
                }
                if (t >= (1u << 22)) return Status::err(EON_E_SHAPE, "more than 2^22 - 1 lookup terms");
            }
            if (n_lookups) p->term_off.push_back((uint32_t)t);
        }
        EON_TRY(compile(p.get(), nodes, n_nodes, consts, n_consts, constraints, n_constraints));
        if (n_lookups) {
            p->terms = std::make_unique<eon_air_program>();
            eon_air_program* t = p->terms.get();
            t->ctx = ctx;
            t->width = width;
            t->pre_width = preprocessed_width;
            t->n_public = n_public;
            t->perm_width = permutation_width;
            t->n_challenges = n_challenges;
            EON_TRY(compile(t, nodes, n_nodes, consts, n_consts, term_roots.data(), (uint32_t)term_roots.size(), true,
                            &p->terms_read_pre));
        }
        // device copies padded with OP_NOP to whole CODE_BLOCKs
        auto upload = [&](eon_air_program* q) -> hipError_t {
            std::vector<Instr> padded(q->code);
            while (padded.size() % CODE_BLOCK) padded.push_back({OP_NOP, NO_DST, M_PREV << 29, 0});
            hipError_t e = q->d_code.ensure(std::max<size_t>(1, padded.size()) * sizeof(Instr));
            if (e == hipSuccess && !padded.empty())
                e = hipMemcpy(q->d_code.p, padded.data(), padded.size() * sizeof(Instr), hipMemcpyHostToDevice);
            if (e == hipSuccess)
                e = q->d_table.ensure(std::max<size_t>(1, q->n_consts + n_public + n_challenges) * sizeof(F29));
            return e;
        };
        hipError_t e = upload(p.get());
        if (e == hipSuccess && p->terms) e = upload(p->terms.get());
        if (e == hipSuccess && p->terms) {
            std::vector<uint32_t> desc(p->term_off);
            desc.insert(desc.end(), p->aux.begin(), p->aux.end());
            e = p->d_desc.ensure(desc.size() * sizeof(uint32_t));
            if (e == hipSuccess)
                e = hipMemcpy(p->d_desc.p, desc.data(), desc.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = p->d_flag.ensure(sizeof(uint32_t));
        }
        if (e != hipSuccess) {
            release_program(p.get());
            EON_HIP(e);
        }
        *out = p.release();
        return Status::ok();
    });
}

int eon_air_program_create_pp(eon_ctx* ctx, const eon_sym_node* nodes, uint32_t n_nodes, const eon_fr* consts,
                              uint32_t n_consts, const uint32_t* constraints, uint32_t n_constraints, uint32_t width,
                              uint32_t preprocessed_width, uint32_t n_public, eon_air_program** out) {
    return eon_air_program_create_lk(ctx, nodes, n_nodes, consts, n_consts, constraints, n_constraints, width,
                                     preprocessed_width, n_public, 0, 0, nullptr, 0, nullptr, out);
}

int eon_air_program_create(eon_ctx* ctx, const eon_sym_node* nodes, uint32_t n_nodes, const eon_fr* consts,
                           uint32_t n_consts, const uint32_t* constraints, uint32_t n_constraints, uint32_t width,
                           uint32_t n_public, eon_air_program** out) {
    return eon_air_program_create_pp(ctx, nodes, n_nodes, consts, n_consts, constraints, n_constraints, width, 0,
                                     n_public, out);
}

void eon_air_program_destroy(eon_air_program* p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(p->ctx->mu);
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    release_program(p);
    delete p;
}

int eon_air_program_info(const eon_air_program* p, eon_air_program_stats* out) {
    if (!p || !out) return EON_E_ARG;
    out->width = p->width;
    out->num_public_values = p->n_public;
    out->num_constraints = p->n_constraints;
    out->max_constraint_degree = p->max_degree;
    out->num_instructions = (uint32_t)p->code.size();
    out->num_registers = p->n_regs;
    out->num_constants = p->n_consts;
    return EON_OK;
}

uint32_t eon_air_program_preprocessed_width(const eon_air_program* p) { return p ? p->pre_width : 0; }
uint32_t eon_air_program_permutation_width(const eon_air_program* p) { return p ? p->perm_width : 0; }
uint32_t eon_air_program_num_challenges(const eon_air_program* p) { return p ? p->n_challenges : 0; }
uint32_t eon_air_program_num_lookups(const eon_air_program* p) { return p ? (uint32_t)p->aux.size() : 0; }

uint32_t eon_air_program_log_quotient_degree(const eon_air_program* p, uint32_t is_zk) {
    // symbolic_builder.rs:28-42: log2_ceil(max(max_degree + is_zk, 2) - 1)
    if (!p) return 0;
    const uint32_t d = std::max<uint32_t>(p->max_degree + (is_zk ? 1 : 0), 2) - 1;
    uint32_t b = 0;
    while ((1u << b) < d) b++;
    return b;
}

int eon_quotient_values_lk_dev(eon_ctx* ctx, const eon_air_program* prog_c, const eon_fr* lde, const eon_fr* pre_lde,
                               const eon_fr* perm_lde, uint32_t log_n, uint32_t log_qd, const eon_fr* alpha,
                               const eon_fr* publics, uint32_t n_public, const eon_fr* challenges,
                               uint32_t n_challenges, eon_fr* out) {
    if (!ctx || !prog_c) return EON_E_ARG;
    auto* prog = const_cast<eon_air_program*>(prog_c);  // device scratch only
    return with_ctx(ctx, [&]() -> Status {
        EON_TRY(check_args(ctx, prog, !lde || !alpha || !out,
                           MatArg::one("perm_lde", perm_lde, " (eon_quotient_values_lk_dev)"),
                           MatArg::one("pre_lde", pre_lde), publics, n_public, challenges, n_challenges));
        const uint32_t log_q = log_n + log_qd;
        EON_TRY(check_domains(log_n, log_q));
        const Fr al = fr_from_abi(alpha);
        if (!fr_is_canonical(al)) return Status::err(EON_E_ARG, "alpha is not a canonical Fr");
        const uint64_t q = 1ull << log_q;
        EON_TRY(stage_table(ctx, prog, publics, n_public, challenges, n_challenges));
        // quotient domain = trace domain (shift 1).create_disjoint_domain: shift GENERATOR
        // (commit/src/domain.rs:155-168); selectors_on_coset over it (prover.rs:563-564)
        const Fr g5 = from_u64<FrP>(5);
        const Fr* inv_van;
        if (prog->uses_sels) {
            EON_HIP(prog->d_sels.ensure(4 * q * sizeof(Fr)));
            EON_TRY(selectors_launch(ctx, log_n, log_q, g5, prog->d_sels.as<Fr>()));
            inv_van = prog->d_sels.as<Fr>() + 3 * q;
        } else {
            Fr *zh, *zh_inv;
            EON_TRY(vanishing_table(ctx, log_n, log_q, g5, &zh, &zh_inv));
            inv_van = zh_inv;
        }
        const uint32_t nr_mask = prog->uses_sels ? (uint32_t)(q - 1) : (1u << log_qd) - 1;
        RegFile regs;
        EON_TRY(plan_regs(prog, q, &regs));
        // products per row: the program's, one per fold, the final inv_vanishing product
        const Profile prof{"k_air_quotient",
                           q * ((uint64_t)prog->width + prog->pre_width + prog->perm_width) * 32 + q * 32,
                           q * (products(prog->code, true) + 1)};
        return launch_air(
            ctx, prog, regs, q, code_blocks(prog->code.size()), prof, prog->pre_width > 0, prog->perm_width > 0,
            [](auto m, auto pre, auto perm) { return k_air_quotient<m(), pre(), perm()>; },
            reinterpret_cast<const Fr*>(lde), prog->width, reinterpret_cast<const Fr*>(pre_lde), prog->pre_width,
            reinterpret_cast<const Fr*>(perm_lde), prog->perm_width, q, 1ull << log_qd, prog->d_table.as<F29>(),
            prog->uses_sels ? prog->d_sels.as<Fr>() : nullptr, inv_van, nr_mask, al, reinterpret_cast<Fr*>(out));
    });
}

int eon_quotient_values_pp_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* lde, const eon_fr* pre_lde,
                               uint32_t log_n, uint32_t log_qd, const eon_fr* alpha, const eon_fr* publics,
                               uint32_t n_public, eon_fr* out) {
    if (!ctx || !prog) return EON_E_ARG;
    if (prog->perm_width > 0 || prog->n_challenges > 0) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        return finish(ctx, Status::err(EON_E_ARG, "the program reads permutation columns and challenges: call "
                                                  "eon_quotient_values_lk_dev with perm_lde and the challenges"));
    }
    return eon_quotient_values_lk_dev(ctx, prog, lde, pre_lde, nullptr, log_n, log_qd, alpha, publics, n_public,
                                      nullptr, 0, out);
}

int eon_quotient_values_dev(eon_ctx* ctx, const eon_air_program* prog, const eon_fr* lde, uint32_t log_n,
                            uint32_t log_qd, const eon_fr* alpha, const eon_fr* publics, uint32_t n_public,
                            eon_fr* out) {
    if (!ctx || !prog) return EON_E_ARG;
    if (prog->pre_width > 0) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        return finish(ctx, Status::err(EON_E_ARG, "the program reads preprocessed columns: call "
                                                  "eon_quotient_values_pp_dev with their LDE"));
    }
    return eon_quotient_values_pp_dev(ctx, prog, lde, nullptr, log_n, log_qd, alpha, publics, n_public, out);
}

int eon_quotient_values_rows_dev(eon_ctx* ctx, const eon_air_program* prog_c, const eon_fr* window, uint32_t log_n,
                                 uint32_t log_qd, uint64_t row0, uint64_t n_rows, const eon_fr* alpha,
                                 const eon_fr* publics, uint32_t n_public, eon_fr* out) {
    if (!ctx || !prog_c) return EON_E_ARG;
    auto* prog = const_cast<eon_air_program*>(prog_c);  // device scratch only
    return with_ctx(ctx, [&]() -> Status {
        if (prog->pre_width > 0 || prog->perm_width > 0 || prog->n_challenges > 0)
            return Status::err(EON_E_ARG, "the windowed quotient takes a main trace only: the program reads "
                                          "preprocessed or permutation columns");
        EON_TRY(check_args(ctx, prog, !alpha || (n_rows && (!window || !out)), MatArg::none(), MatArg::none(), publics,
                           n_public, nullptr, 0));
        const uint32_t log_q = log_n + log_qd;
        EON_TRY(check_domains(log_n, log_q));
        const uint64_t q = 1ull << log_q;
        if (row0 > q || n_rows > q - row0) return Status::err(EON_E_SHAPE, "row0 + n_rows exceeds the quotient domain");
        const Fr al = fr_from_abi(alpha);
        if (!fr_is_canonical(al)) return Status::err(EON_E_ARG, "alpha is not a canonical Fr");
        if (n_rows == 0) return Status::ok();
        EON_TRY(stage_table(ctx, prog, publics, n_public, nullptr, 0));
        // the selector and vanishing tables of the whole domain, as eon_quotient_values_lk_dev makes
        // them: the rows of this launch index into them at row0 + t
        const Fr g5 = from_u64<FrP>(5);
        const Fr* inv_van;
        if (prog->uses_sels) {
            EON_HIP(prog->d_sels.ensure(4 * q * sizeof(Fr)));
            EON_TRY(selectors_launch(ctx, log_n, log_q, g5, prog->d_sels.as<Fr>()));
            inv_van = prog->d_sels.as<Fr>() + 3 * q;
        } else {
            Fr *zh, *zh_inv;
            EON_TRY(vanishing_table(ctx, log_n, log_q, g5, &zh, &zh_inv));
            inv_van = zh_inv;
        }
        const uint32_t nr_mask = prog->uses_sels ? (uint32_t)(q - 1) : (1u << log_qd) - 1;
        RegFile regs;
        EON_TRY(plan_regs(prog, n_rows, &regs));
        const Profile prof{"k_air_quotient_rows", (n_rows + (1ull << log_qd)) * prog->width * 32 + n_rows * 32,
                           n_rows * (products(prog->code, true) + 1)};
        return launch_air(
            ctx, prog, regs, n_rows, code_blocks(prog->code.size()), prof, false, false,
            [](auto m, auto, auto) { return k_air_quotient_rows<m()>; }, reinterpret_cast<const Fr*>(window),
            prog->width, q, 1ull << log_qd, row0, n_rows, prog->d_table.as<F29>(),
            prog->uses_sels ? prog->d_sels.as<Fr>() : nullptr, inv_van, nr_mask, al, reinterpret_cast<Fr*>(out));
    });
}

int eon_lookup_permutation_dev(eon_ctx* ctx, const eon_air_program* prog_c, const eon_fr* trace,
                               const eon_fr* pre_trace, uint64_t height, const eon_fr* publics, uint32_t n_public,
                               const eon_fr* challenges, uint32_t n_challenges, eon_fr* perm_out) {
    if (!ctx || !prog_c) return EON_E_ARG;
    auto* prog = const_cast<eon_air_program*>(prog_c);  // device scratch only
    return with_ctx(ctx, [&]() -> Status {
        // no permutation matrix here, and pre_trace follows the terms, not the program (below)
        EON_TRY(check_args(ctx, prog, !trace || !perm_out, MatArg::none(), MatArg::none(), publics, n_public,
                           challenges, n_challenges, &height));
        if (!prog->terms)
            return Status::err(EON_E_ARG, "the program carries no lookup description (eon_air_program_create_lk)");
        if (prog->terms_read_pre != (pre_trace != nullptr) && (prog->terms_read_pre || prog->pre_width == 0))
            return Status::err(EON_E_ARG, prog->terms_read_pre
                                              ? "a lookup term reads a preprocessed column: pre_trace must not be null"
                                              : "the program has no preprocessed columns: pre_trace must be null");
        eon_air_program* tp = prog->terms.get();
        EON_TRY(stage_table(ctx, tp, publics, n_public, challenges, n_challenges));
        const uint32_t n_lookups = (uint32_t)prog->aux.size(), n_terms = prog->term_off.back();
        // per row: 2 T emitted values of 36 bytes (padded to 48 so the prefix planes stay aligned),
        // then T prefix products
        const uint64_t emitted = 2ull * n_terms * height * 48;
        EON_HIP(ctx_ensure(ctx, prog->d_terms, std::max<uint64_t>(1, emitted + (uint64_t)n_terms * height * sizeof(Fr))));
        EON_HIP(hipMemsetAsync(prog->d_flag.p, 0xff, sizeof(uint32_t), ctx->stream));
        RegFile regs;  // of the term program, over the trace's rows
        EON_TRY(plan_regs(tp, height, &regs));
        const Profile prof{"k_lookup_terms",
                           height * ((uint64_t)prog->width + prog->pre_width + prog->perm_width) * 32, 0};
        EON_TRY(launch_air(
            ctx, tp, regs, height, code_blocks(tp->code.size()), prof, pre_trace != nullptr && prog->pre_width > 0,
            false, [](auto m, auto pre, auto) { return k_lookup_terms<m(), pre()>; },
            reinterpret_cast<const Fr*>(trace), prog->width, reinterpret_cast<const Fr*>(pre_trace), prog->pre_width,
            height, tp->d_table.as<F29>(), 2 * n_terms, prog->d_terms.as<uint4>()));
        EON_TRY(lookup_contributions(ctx, prog->d_terms.as<uint4>(),
                                     reinterpret_cast<Fr*>(prog->d_terms.as<char>() + emitted), height, prog->d_desc.as<uint32_t>(), n_lookups,
                                     n_terms, reinterpret_cast<Fr*>(perm_out), prog->perm_width,
                                     prog->d_flag.as<uint32_t>()));
        EON_TRY(lookup_running_sum(ctx, reinterpret_cast<Fr*>(perm_out), height, prog->perm_width));
        uint32_t flag = 0;
        EON_HIP(hipMemcpyAsync(&flag, prog->d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        if (flag != 0xffffffffu)
            return Status::err(EON_E_ARG, "lookup " + std::to_string(flag) + " (auxiliary column " +
                                              std::to_string(prog->aux[flag]) +
                                              "): a denominator alpha - fold(elements, beta) is zero on some row; "
                                              "the permutation trace is not valid");
        return Status::ok();
    });
}

int eon_check_constraints_dev(eon_ctx* ctx, const eon_air_program* prog_c, const eon_fr* trace,
                              const eon_fr* pre_trace, const eon_fr* perm_trace, uint64_t height,
                              const eon_fr* publics, uint32_t n_public, const eon_fr* challenges,
                              uint32_t n_challenges, uint32_t* per_constraint, eon_constraint_report* out) {
    if (!ctx || !prog_c) return EON_E_ARG;
    auto* prog = const_cast<eon_air_program*>(prog_c);  // device scratch only
    return with_ctx(ctx, [&]() -> Status {
        EON_TRY(check_args(ctx, prog, !trace || !out, MatArg::one("perm_trace", perm_trace),
                           MatArg::one("pre_trace", pre_trace), publics, n_public, challenges, n_challenges, &height));
        EON_TRY(stage_table(ctx, prog, publics, n_public, challenges, n_challenges));
        *out = eon_constraint_report{};
        const uint32_t nc = prog->n_constraints;
        if (per_constraint) std::fill(per_constraint, per_constraint + nc, 0u);
        if (nc == 0) return Status::ok();
        // device results: min key (8) | failures (8) | value (32) | per-constraint counts (4 nc)
        constexpr size_t HEAD = 16 + sizeof(Fr);
        EON_HIP(prog->d_check.ensure(HEAD + (size_t)nc * sizeof(uint32_t)));
        char* res = prog->d_check.as<char>();
        EON_HIP(hipMemsetAsync(res, 0, HEAD + (size_t)nc * sizeof(uint32_t), ctx->stream));
        EON_HIP(hipMemsetAsync(res, 0xff, 8, ctx->stream));
        RegFile regs;
        EON_TRY(plan_regs(prog, height, &regs));
        auto* summary = reinterpret_cast<unsigned long long*>(res);
        Fr* value = reinterpret_cast<Fr*>(res + 16);
        uint32_t* counts = reinterpret_cast<uint32_t*>(res + HEAD);
        auto launch = [&](uint64_t row0, uint64_t n_rows, uint32_t target, uint32_t run_blocks, const Profile& prof) {
            return launch_air(
                ctx, prog, regs, n_rows, run_blocks, prof, prog->pre_width > 0, prog->perm_width > 0,
                [](auto m, auto pre, auto perm) { return k_air_check<m(), pre(), perm()>; },
                reinterpret_cast<const Fr*>(trace), prog->width, reinterpret_cast<const Fr*>(pre_trace),
                prog->pre_width, reinterpret_cast<const Fr*>(perm_trace), prog->perm_width, height,
                prog->d_table.as<F29>(), row0, n_rows, target, nc, counts, summary, value);
        };
        // products per row: no folds, no inv_vanishing
        EON_TRY(launch(0, height, NO_FAIL, code_blocks(prog->code.size()),
                       Profile{"k_air_check", height * ((uint64_t)prog->width + prog->pre_width + prog->perm_width) * 32,
                               height * products(prog->code, false)}));
        std::vector<unsigned long long> head(2);
        std::vector<uint32_t> host_counts(nc);
        EON_HIP(hipMemcpyAsync(head.data(), summary, 16, hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipMemcpyAsync(host_counts.data(), counts, (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        if (per_constraint) std::copy(host_counts.begin(), host_counts.end(), per_constraint);
        out->failures = head[1];
        for (const uint32_t c : host_counts) out->failing_constraints += c != 0 ? 1 : 0;
        if (head[1] == 0) return Status::ok();
        out->row = head[0] / nc;
        out->constraint = (uint32_t)(head[0] % nc);
        // the value: one thread on that row runs the program up to that ASSERT's code block and
        // stores its operand
        uint32_t at = 0;
        for (uint32_t seen = 0; at < prog->code.size(); at++)
            if ((prog->code[at].op & OP_MASK) == OP_ASSERT && seen++ == out->constraint) break;
        EON_TRY(launch(out->row, 1, out->constraint, at / CODE_BLOCK + 1, Profile{nullptr, 0, 0}));
        static_assert(sizeof(Fr) == sizeof(eon_fr), "Fr is the ABI's 32 little-endian bytes");
        EON_HIP(hipMemcpyAsync(&out->value, value, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    });
}

int eon_air_eval_at_point_dev(eon_ctx* ctx, const eon_air_program* prog_c, uint32_t log_n, const eon_fr* zeta,
                              const eon_fr* alpha, const eon_fr* local, const eon_fr* next, const eon_fr* pre_local,
                              const eon_fr* pre_next, const eon_fr* perm_local, const eon_fr* perm_next,
                              const eon_fr* publics, uint32_t n_public, const eon_fr* challenges,
                              uint32_t n_challenges, eon_fr* out) {
    if (!ctx || !prog_c) return EON_E_ARG;
    auto* prog = const_cast<eon_air_program*>(prog_c);  // device scratch only
    return with_ctx(ctx, [&]() -> Status {
        EON_TRY(check_args(ctx, prog, !zeta || !alpha || !out || (prog->width && (!local || !next)),
                           MatArg::pair("perm_local and perm_next", perm_local, perm_next),
                           MatArg::pair("pre_local and pre_next", pre_local, pre_next), publics, n_public, challenges,
                           n_challenges));
        if (log_n > 28) return Status::err(EON_E_SHAPE, "log_n must be <= 28 (Fr::TWO_ADICITY)");
        const Fr al = fr_from_abi(alpha), z = fr_from_abi(zeta);
        if (!fr_is_canonical(al)) return Status::err(EON_E_ARG, "alpha is not a canonical Fr");
        if (!fr_is_canonical(z)) return Status::err(EON_E_ARG, "zeta is not a canonical Fr");
        Fr sel_host[4];
        EON_TRY(selectors_at_point(log_n, z, sel_host));
        EON_TRY(stage_table(ctx, prog, publics, n_public, challenges, n_challenges));
        EON_HIP(prog->d_point.ensure(6 * sizeof(Fr)));
        Fr* sels = prog->d_point.as<Fr>();
        Fr* res = sels + 4;
        EON_HIP(hipMemcpyAsync(sels, sel_host, sizeof(sel_host), hipMemcpyHostToDevice, ctx->stream));
        RegFile regs;  // over one row
        EON_TRY(plan_regs(prog, 1, &regs));
        // products: the program's, one per fold, the two results
        const Profile prof{"k_air_point",
                           2 * ((uint64_t)prog->width + prog->pre_width + prog->perm_width) * 32 + 6 * 32,
                           products(prog->code, true) + 2};
        EON_TRY(launch_air(
            ctx, prog, regs, 1, code_blocks(prog->code.size()), prof, prog->pre_width > 0, prog->perm_width > 0,
            [](auto m, auto pre, auto perm) { return k_air_point<m(), pre(), perm()>; },
            reinterpret_cast<const Fr*>(local), reinterpret_cast<const Fr*>(next),
            reinterpret_cast<const Fr*>(pre_local), reinterpret_cast<const Fr*>(pre_next),
            reinterpret_cast<const Fr*>(perm_local), reinterpret_cast<const Fr*>(perm_next), prog->width,
            prog->pre_width, prog->d_table.as<F29>(), sels, al, res));
        static_assert(sizeof(Fr) == sizeof(eon_fr), "Fr is the ABI's 32 little-endian bytes");
        EON_HIP(hipMemcpyAsync(out, res, 2 * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    });
}

int eon_air_eval_at_points_dev(eon_ctx* ctx, const eon_air_program* prog_c, uint32_t n, const uint32_t* log_n,
                               const eon_fr* zeta, const eon_fr* alpha, const eon_fr* rows, uint64_t row_stride,
                               const eon_fr* publics, const eon_fr* challenges, uint32_t n_challenges, eon_fr* out) {
    if (!ctx || !prog_c) return EON_E_ARG;
    auto* prog = const_cast<eon_air_program*>(prog_c);  // device scratch only
    return with_ctx(ctx, [&]() -> Status {
        if (n == 0) return Status::ok();
        const uint64_t opened = 2 * ((uint64_t)prog->width + prog->pre_width + prog->perm_width);
        EON_TRY(check_args(ctx, prog, !log_n || !zeta || !alpha || !out || (opened && !rows), MatArg::none(),
                           MatArg::none(), publics, prog->n_public, challenges, n_challenges));
        if (row_stride < opened) return Status::err(EON_E_SHAPE, "row_stride is below the program's opened values");
        if (n > (1u << 20)) return Status::err(EON_E_SHAPE, "at most 2^20 points");
        const auto at = [](uint32_t i, const std::string& what) { return "point " + std::to_string(i) + ": " + what; };
        // per proof: the selectors at its zeta, its alpha, and its copy of the constant table
        // (stage_table's layout: program constants ++ public values ++ challenges)
        const uint32_t n_public = prog->n_public;
        const uint32_t table_stride = (uint32_t)prog->consts.size() + n_public + n_challenges;
        std::vector<Fr> head(7 * (size_t)n);  // 4n selectors | 2n results (unset) | n alphas
        std::vector<F29> tables((size_t)n * table_stride);
        for (uint32_t i = 0; i < n; i++) {
            if (log_n[i] > 28) return Status::err(EON_E_SHAPE, at(i, "log_n must be <= 28 (Fr::TWO_ADICITY)"));
            const Fr al = fr_from_abi(&alpha[i]), z = fr_from_abi(&zeta[i]);
            if (!fr_is_canonical(al)) return Status::err(EON_E_ARG, at(i, "alpha is not a canonical Fr"));
            if (!fr_is_canonical(z)) return Status::err(EON_E_ARG, at(i, "zeta is not a canonical Fr"));
            const Status sel = selectors_at_point(log_n[i], z, &head[4 * (size_t)i]);
            if (sel.bad()) return Status::err(sel.code, at(i, sel.msg));
            head[6 * (size_t)n + i] = al;
            F29* t = tables.data() + (size_t)i * table_stride;
            for (const Fr& c : prog->consts) *t++ = shl5_to261<FrP>(c);
            for (uint32_t j = 0; j < n_public + n_challenges; j++) {
                const bool pub = j < n_public;
                const Fr v = fr_from_abi(pub ? &publics[(size_t)i * n_public + j]
                                             : &challenges[(size_t)i * n_challenges + (j - n_public)]);
                if (!fr_is_canonical(v))
                    return Status::err(EON_E_ARG, at(i, pub ? "public value is not a canonical Fr"
                                                            : "challenge is not a canonical Fr"));
                *t++ = shl5_to261<FrP>(v);
            }
        }
        const size_t head_bytes = head.size() * sizeof(Fr), table_bytes = tables.size() * sizeof(F29);
        EON_HIP(prog->d_points.ensure(head_bytes + std::max<size_t>(table_bytes, sizeof(F29))));
        Fr* sels = prog->d_points.as<Fr>();
        Fr* res = sels + 4 * (size_t)n;
        const Fr* alphas = sels + 6 * (size_t)n;
        F29* d_tables = reinterpret_cast<F29*>(prog->d_points.as<char>() + head_bytes);
        RegFile regs;  // one register row per proof
        EON_TRY(plan_regs(prog, n, &regs));
        // from here on the stream reads `head` and `tables`: every path out synchronises first
        const auto drained = [&](Status s) {
            (void)hipStreamSynchronize(ctx->stream);
            return s;
        };
        EON_HIP(hipMemcpyAsync(sels, head.data(), head_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (table_bytes) {
            const hipError_t e = hipMemcpyAsync(d_tables, tables.data(), table_bytes, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) return drained(Status::err(EON_E_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e)));
        }
        const Profile prof{"k_air_points", (uint64_t)n * (opened * 32 + 7 * 32),
                           (uint64_t)n * (products(prog->code, true) + 2)};
        // one block of regs.block threads per proof: launch_air sizes the grid from the rows
        const Status launched = launch_air(
            ctx, prog, regs, (uint64_t)n * regs.block, code_blocks(prog->code.size()), prof, prog->pre_width > 0,
            prog->perm_width > 0, [](auto m, auto pre, auto perm) { return k_air_points<m(), pre(), perm()>; },
            reinterpret_cast<const Fr*>(rows), row_stride, prog->width, prog->pre_width, prog->perm_width,
            const_cast<const F29*>(d_tables), table_stride, const_cast<const Fr*>(sels), alphas, res);
        if (launched.bad()) return drained(launched);
        const hipError_t e = hipMemcpyAsync(out, res, 2 * (size_t)n * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) return drained(Status::err(EON_E_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e)));
        EON_HIP(hipStreamSynchronize(ctx->stream));
        return Status::ok();
    });
}

}  // extern "C"
