"""The Blake3-AIR (blake3-air/src/{air,columns,generation,constants}.rs): one row per compression,
9168 columns, 9760 constraints of degree <= 3, none of which reads the next row.

* ``Blake3Air.eval``           -- Blake3Air::eval on the symbolic builder, in the reference's assert
                                  order; it goes through ``AirProgram`` like every other generic AIR
                                  (quotient_values, check_constraints, eval_at_point, prove_native /
                                  verify_native).
* ``Blake3Air.generate_trace`` -- generate_trace_rows (generation.rs:16-121) on the device
                                  (eon_blake3_generate_trace_dev, csrc/blake3_air.hip).

Column order is Blake3Cols' (columns.rs): a u32 is either 32 bits or two 16-bit limbs, both
little-endian.  The quarter round keeps a and c as limbs (they are summed) and b and d as bits (they
are xored and rotated).
"""

from __future__ import annotations

import ctypes

BITS_PER_LIMB = 16
NUM_ROUNDS = 7

# BLAKE3's IV (the SHA-256 initial hash values) and message permutation
IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
MSG_PERMUTATION = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)

# Blake3Cols<T> as column offsets
COL_INPUTS = 0
COL_CHAINING_VALUES = COL_INPUTS + 16 * 32
COL_COUNTER_LOW = COL_CHAINING_VALUES + 2 * 4 * 32
COL_COUNTER_HI = COL_COUNTER_LOW + 32
COL_BLOCK_LEN = COL_COUNTER_HI + 32
COL_FLAGS = COL_BLOCK_LEN + 32
COL_INITIAL_ROW0 = COL_FLAGS + 32
COL_INITIAL_ROW2 = COL_INITIAL_ROW0 + 4 * 2
COL_FULL_ROUNDS = COL_INITIAL_ROW2 + 4 * 2
# Blake3State<T>: row0[4][2] limbs, row1[4][32] bits, row2[4][2] limbs, row3[4][32] bits
STATE_ROW0, STATE_ROW1, STATE_ROW2, STATE_ROW3 = 0, 8, 136, 144
STATE_COLS = 272
# FullRound<T>: state_prime, state_middle, state_middle_prime, state_output
STATE_PRIME, STATE_MIDDLE, STATE_MIDDLE_PRIME, STATE_OUTPUT = range(4)
ROUND_COLS = 4 * STATE_COLS
COL_FINAL_ROUND_HELPERS = COL_FULL_ROUNDS + NUM_ROUNDS * ROUND_COLS
COL_OUTPUTS = COL_FINAL_ROUND_HELPERS + 4 * 32
NUM_BLAKE3_COLS = COL_OUTPUTS + 4 * 4 * 32  # 9168


class _State:
    """Blake3State<T>: row0 and row2 as [4] pairs of limbs, row1 and row3 as [4] lists of 32 bits."""

    def __init__(self, row0, row1, row2, row3):
        self.row0, self.row1, self.row2, self.row3 = row0, row1, row2, row3

    @staticmethod
    def at(row, base):
        def limbs(off):
            return [row[base + off + 2 * i:base + off + 2 * i + 2] for i in range(4)]

        def bits(off):
            return [row[base + off + 32 * i:base + off + 32 * i + 32] for i in range(4)]

        return _State(limbs(STATE_ROW0), bits(STATE_ROW1), limbs(STATE_ROW2), bits(STATE_ROW3))


def _words(row, base, n):
    return [row[base + 32 * i:base + 32 * i + 32] for i in range(n)]


def _limb_pairs(row, base, n):
    return [row[base + 2 * i:base + 2 * i + 2] for i in range(n)]


class Blake3Air:
    """Blake3Air (blake3-air/src/air.rs).  ``ctx`` is needed by ``generate_trace`` only (the default
    context of the inputs' device when None); ``eval`` needs no device."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def width(self) -> int:
        return NUM_BLAKE3_COLS

    def num_public_values(self) -> int:
        return 0

    # --- constraints ---------------------------------------------------------------------------
    @staticmethod
    def _quarter_round(builder, a, b, c, d, m_two_i, m_two_i_plus_one, prime, output):
        """quarter_round_function (air.rs:38-106): `prime` and `output` are the (a, b, c, d) after
        the first and the second half."""
        from .symbolic import add2, add3, pack_bits_le, xor_32_shift

        def halves(bits):
            return [pack_bits_le(bits[:BITS_PER_LIMB]), pack_bits_le(bits[BITS_PER_LIMB:])]

        a_prime, b_prime, c_prime, d_prime = prime
        a_output, b_output, c_output, d_output = output
        add3(builder, a_prime, a, halves(b), m_two_i)  # a' = a + b + m_2i
        xor_32_shift(builder, a_prime, d, d_prime, 16)  # a' = d ^ (d' <<< 16)
        add2(builder, c_prime, c, halves(d_prime))  # c' = c + d'
        xor_32_shift(builder, c_prime, b, b_prime, 12)  # c' = b ^ (b' <<< 12)
        add3(builder, a_output, a_prime, halves(b_prime), m_two_i_plus_one)  # a'' = a' + b' + m_2i+1
        xor_32_shift(builder, a_output, d_prime, d_output, 8)  # a'' = d' ^ (d'' <<< 8)
        add2(builder, c_output, c_prime, halves(d_output))  # c'' = c' + d''
        xor_32_shift(builder, c_output, b_prime, b_output, 7)  # c'' = b' ^ (b'' <<< 7)

    def _verify_round(self, builder, inp, states, m):
        """verify_round (air.rs:170-224): the four columns, then the four diagonals."""
        prime, middle, middle_prime, output = states
        for i in range(4):
            self._quarter_round(builder, inp.row0[i], inp.row1[i], inp.row2[i], inp.row3[i], m[2 * i], m[2 * i + 1],
                                (prime.row0[i], prime.row1[i], prime.row2[i], prime.row3[i]),
                                (middle.row0[i], middle.row1[i], middle.row2[i], middle.row3[i]))
        for i in range(4):
            j, k, l = (i + 1) % 4, (i + 2) % 4, (i + 3) % 4
            self._quarter_round(builder, middle.row0[i], middle.row1[j], middle.row2[k], middle.row3[l],
                                m[2 * i + 8], m[2 * i + 9],
                                (middle_prime.row0[i], middle_prime.row1[j], middle_prime.row2[k], middle_prime.row3[l]),
                                (output.row0[i], output.row1[j], output.row2[k], output.row3[l]))

    def eval(self, builder):
        from .symbolic import SymbolicExpression, pack_bits_le, xor_32_shift

        E = SymbolicExpression.lift
        local = builder.main()[0]
        inputs = _words(local, COL_INPUTS, 16)
        cv = [_words(local, COL_CHAINING_VALUES + 128 * i, 4) for i in range(2)]
        initial_row3 = _words(local, COL_COUNTER_LOW, 4)  # counter_low, counter_hi, block_len, flags
        initial_row0 = _limb_pairs(local, COL_INITIAL_ROW0, 4)
        initial_row2 = _limb_pairs(local, COL_INITIAL_ROW2, 4)
        rounds = [[_State.at(local, COL_FULL_ROUNDS + ROUND_COLS * r + STATE_COLS * s) for s in range(4)]
                  for r in range(NUM_ROUNDS)]
        helpers = _words(local, COL_FINAL_ROUND_HELPERS, 4)
        outputs = [_words(local, COL_OUTPUTS + 128 * i, 4) for i in range(4)]

        def halves(bits):
            return [pack_bits_le(bits[:BITS_PER_LIMB]), pack_bits_le(bits[BITS_PER_LIMB:])]

        # every initialization input is a bit (air.rs:247-257)
        for word in inputs + cv[0] + cv[1] + initial_row3:
            for bit in word:
                builder.assert_bool(bit)

        # row0 of the initial state packs the first four chaining values (air.rs:261-270)
        for bits, word in zip(cv[0], initial_row0):
            lo, hi = halves(bits)
            builder.assert_eq(lo, word[0])
            builder.assert_eq(hi, word[1])

        # row2 holds the first four constants of IV (air.rs:272-280)
        for word, constant in zip(initial_row2, IV):
            builder.assert_eq(word[0], SymbolicExpression.constant(constant & 0xFFFF))
            builder.assert_eq(word[1], SymbolicExpression.constant(constant >> 16))

        m_values = [halves(bits) for bits in inputs]
        state = _State(initial_row0, cv[1], initial_row2, initial_row3)

        # the seven rounds, the message words permuted in between (air.rs:296-365)
        for r in range(NUM_ROUNDS):
            if r > 0:
                m_values = [m_values[MSG_PERMUTATION[i]] for i in range(16)]
            self._verify_round(builder, state, rounds[r], m_values)
            state = rounds[r][STATE_OUTPUT]

        # the final xors.  state[8..12] are limbs: their bits are the helpers (air.rs:373-389)
        for bits, word in zip(helpers, state.row2):
            lo, hi = halves(bits)
            builder.assert_eq(lo, word[0])
            builder.assert_eq(hi, word[1])
        for word in helpers + outputs[0]:
            for bit in word:
                builder.assert_bool(bit)

        # outputs[0] = state[0..4] ^ state[8..12], as state[0..4] = outputs[0] ^ helpers (air.rs:394-403)
        for out_bits, left_words, right_bits in zip(outputs[0], state.row0, helpers):
            xor_32_shift(builder, left_words, out_bits, right_bits, 0)

        # outputs[1] = state[4..8] ^ state[12..16], outputs[2] = state[8..12] ^ cv[0..4],
        # outputs[3] = state[12..16] ^ cv[4..8], bit by bit (air.rs:408-445)
        for outs, lefts, rights in ((outputs[1], state.row1, state.row3), (outputs[2], cv[0], helpers),
                                    (outputs[3], cv[1], state.row3)):
            for out_bits, left_bits, right_bits in zip(outs, lefts, rights):
                for out_bit, left_bit, right_bit in zip(out_bits, left_bits, right_bits):
                    builder.assert_eq(out_bit, E(left_bit).xor(E(right_bit)))

    # --- witness -------------------------------------------------------------------------------
    def generate_trace(self, inputs):
        """generate_trace_rows (generation.rs:16-121) on the device.  `inputs`: (n, 24) int32 device
        tensor of u32 bit patterns, words 0..15 the block and 16..23 the chaining value -> the
        (n, 9168, 4) int64 trace of Fr Montgomery limbs.  Row k has counter = k, block_len = n and
        flags = 0, as in the reference.  n must be a power of two (generation.rs:21-24); n = 0 or any
        other n is EON_E_SHAPE."""
        import torch

        from .dft import default_context

        if not isinstance(inputs, torch.Tensor):
            raise ValueError("inputs must be a torch tensor")
        if inputs.dtype != torch.int32:
            raise ValueError(f"inputs must be int32 (u32 bit patterns), not {inputs.dtype}")
        if inputs.ndim != 2 or inputs.shape[1] != 24:
            raise ValueError(f"inputs must be (n, 24), not {tuple(inputs.shape)}")
        if inputs.device.type != "cuda":
            raise ValueError(f"inputs must be on the device, not {inputs.device}")
        ctx = self.ctx or default_context(inputs.device.index or 0)
        if (inputs.device.index or 0) != ctx.device:
            raise ValueError(f"inputs are on {inputs.device}, the context on device {ctx.device}")
        n = int(inputs.shape[0])  # the library answers 0 and non-powers of two with EON_E_SHAPE
        out = torch.empty((n, NUM_BLAKE3_COLS, 4), dtype=torch.int64, device=inputs.device)
        ctx.set_stream(torch.cuda.current_stream(inputs.device).cuda_stream)
        ctx.check(ctx.lib.eon_blake3_generate_trace_dev(ctx.handle, ctypes.c_void_p(inputs.contiguous().data_ptr()), n,
                                                        ctypes.c_void_p(out.data_ptr()), n))
        return out
