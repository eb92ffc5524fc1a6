"""The Keccak-AIR (keccak-air/src/{air,columns,generation,round_flags,constants}.rs): one row per
round of Keccak-f[1600], 24 rows per permutation, 2633 columns, 3182 constraints of degree <= 3.

* ``KeccakAir.eval``           -- eval_round_flags then KeccakAir::eval on the symbolic builder, in
                                  the reference's assert order; it goes through ``AirProgram`` like
                                  every other generic AIR (quotient_values, check_constraints,
                                  eval_at_point, prove_native / verify_native).
* ``KeccakAir.generate_trace`` -- generate_trace_rows (generation.rs:17-46) on the device
                                  (eon_keccak_generate_trace_dev, csrc/keccak_air.hip).

Column order is KeccakCols' (columns.rs:18-61): the 5x5 arrays are y-major, a u64 is four 16-bit
limbs or 64 bits, both little-endian.  B is not stored: it is a rotation of A' (columns.rs:64-79).
Both constant tables are derived from FIPS 202 (section 3.2.2 rho, algorithm 5 rc) at import.
"""

from __future__ import annotations

import ctypes

NUM_ROUNDS = 24
BITS_PER_LIMB = 16
U64_LIMBS = 4

# KeccakCols<T> as column offsets
COL_STEP_FLAGS = 0
COL_EXPORT = COL_STEP_FLAGS + NUM_ROUNDS
COL_PREIMAGE = COL_EXPORT + 1
COL_A = COL_PREIMAGE + 25 * U64_LIMBS
COL_C = COL_A + 25 * U64_LIMBS
COL_C_PRIME = COL_C + 5 * 64
COL_A_PRIME = COL_C_PRIME + 5 * 64
COL_A_PRIME_PRIME = COL_A_PRIME + 25 * 64
COL_A_PRIME_PRIME_0_0_BITS = COL_A_PRIME_PRIME + 25 * U64_LIMBS
COL_A_PRIME_PRIME_PRIME_0_0_LIMBS = COL_A_PRIME_PRIME_0_0_BITS + 64
NUM_KECCAK_COLS = COL_A_PRIME_PRIME_PRIME_0_0_LIMBS + U64_LIMBS  # 2633


def _rotation_offsets():
    """FIPS 202 3.2.2: r[x][y] = (t + 1)(t + 2) / 2 mod 64 along (x, y) -> (y, 2x + 3y) from (1, 0)."""
    r = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


def _round_constants():
    """FIPS 202 algorithm 5 / 3.2.5: RC[ir] bit 2^j - 1 = rc(j + 7 ir), rc the LFSR x^8 + x^6 + x^5 + x^4 + 1."""
    def rc(t):
        reg = 1
        for _ in range(t % 255):
            reg <<= 1
            if reg & 0x100:
                reg ^= 0x171
        return reg & 1

    return [sum(rc(j + 7 * ir) << ((1 << j) - 1) for j in range(7)) for ir in range(NUM_ROUNDS)]


R = _rotation_offsets()  # R[x][y]
RC = _round_constants()


def rc_value_bit(round: int, bit_index: int) -> int:
    return (RC[round] >> bit_index) & 1


def keccak_air_rows(n_hashes: int) -> int:
    """(24 n).next_power_of_two(), generation.rs:21; 0 for n = 0 (no trace, see generate_trace)."""
    return 0 if n_hashes <= 0 else 1 << (NUM_ROUNDS * n_hashes - 1).bit_length()


class _Cols:
    """KeccakCols<T> over one row (a list of `NUM_KECCAK_COLS` variables)."""

    def __init__(self, row):
        assert len(row) == NUM_KECCAK_COLS
        self.row = row

    def step_flags(self, i):
        return self.row[COL_STEP_FLAGS + i]

    @property
    def export(self):
        return self.row[COL_EXPORT]

    def preimage(self, y, x, limb):
        return self.row[COL_PREIMAGE + (5 * y + x) * U64_LIMBS + limb]

    def a(self, y, x, limb):
        return self.row[COL_A + (5 * y + x) * U64_LIMBS + limb]

    def c(self, x, z):
        return self.row[COL_C + 64 * x + z]

    def c_prime(self, x, z):
        return self.row[COL_C_PRIME + 64 * x + z]

    def a_prime(self, y, x, z):
        return self.row[COL_A_PRIME + (5 * y + x) * 64 + z]

    def a_prime_prime(self, y, x, limb):
        return self.row[COL_A_PRIME_PRIME + (5 * y + x) * U64_LIMBS + limb]

    def a_prime_prime_0_0_bits(self, z):
        return self.row[COL_A_PRIME_PRIME_0_0_BITS + z]

    def a_prime_prime_prime_0_0_limbs(self, limb):
        return self.row[COL_A_PRIME_PRIME_PRIME_0_0_LIMBS + limb]

    def b(self, x, y, z):
        """columns.rs:64-79: B[x, y] = ROT(A'[a, x], r[a, x]) with a = (x + 3y) mod 5."""
        a = (x + 3 * y) % 5
        return self.a_prime(x, a, (z + 64 - R[a][x]) % 64)

    def a_prime_prime_prime(self, y, x, limb):
        """columns.rs:81-91"""
        if y == 0 and x == 0:
            return self.a_prime_prime_prime_0_0_limbs(limb)
        return self.a_prime_prime(y, x, limb)


class KeccakAir:
    """KeccakAir (keccak-air/src/air.rs).  ``ctx`` is needed by ``generate_trace`` only (the default
    context of the inputs' device when None); ``eval`` needs no device."""

    def __init__(self, ctx=None):
        self.ctx = ctx

    def width(self) -> int:
        return NUM_KECCAK_COLS

    def num_public_values(self) -> int:
        return 0

    # --- constraints ---------------------------------------------------------------------------
    def eval(self, builder):
        from .symbolic import SymbolicExpression

        E = SymbolicExpression.lift
        ZERO, ONE, TWO = (SymbolicExpression.constant(v) for v in (0, 1, 2))
        main = builder.main()
        local, nxt = _Cols(main[0]), _Cols(main[1])
        limbs = range(U64_LIMBS)

        def limb_of(get_bit, limb):
            acc = ZERO
            for z in reversed(range(limb * BITS_PER_LIMB, (limb + 1) * BITS_PER_LIMB)):
                acc = acc.double() + get_bit(z)
            return acc

        # eval_round_flags (round_flags.rs:22-57)
        builder.when_first_row().assert_one(local.step_flags(0))
        builder.when_first_row().assert_zeros([local.step_flags(i) for i in range(1, NUM_ROUNDS)])
        builder.when_transition().assert_zeros([local.step_flags(i) - nxt.step_flags((i + 1) % NUM_ROUNDS)
                                                for i in range(NUM_ROUNDS)])

        first_step = local.step_flags(0)
        final_step = local.step_flags(NUM_ROUNDS - 1)
        not_final_step = ONE - final_step

        # the input A is the preimage on the first step (air.rs:55-64)
        for y in range(5):
            for x in range(5):
                builder.when(first_step).assert_zeros([local.preimage(y, x, l) - local.a(y, x, l) for l in limbs])

        # the preimage is carried while the step is not final (air.rs:66-76)
        for y in range(5):
            for x in range(5):
                builder.when(not_final_step).when_transition().assert_zeros(
                    [local.preimage(y, x, l) - nxt.preimage(y, x, l) for l in limbs])

        # export is a bit, and off unless the step is final (air.rs:78-84)
        builder.assert_bool(local.export)
        builder.when(not_final_step).assert_zero(local.export)

        # C'[x, z] = xor(C[x, z], C[x - 1, z], C[x + 1, z - 1]) (air.rs:86-99)
        for x in range(5):
            builder.assert_bools([local.c(x, z) for z in range(64)])
            builder.assert_zeros([
                local.c_prime(x, z) - E(local.c(x, z)).xor3(E(local.c((x + 4) % 5, z)),
                                                            E(local.c((x + 1) % 5, (z + 63) % 64)))
                for z in range(64)])

        # A = xor(A', C, C') limb by limb, A' boolean (air.rs:101-131)
        for y in range(5):
            for x in range(5):
                def get_bit(z, y=y, x=x):
                    return E(local.a_prime(y, x, z)).xor3(E(local.c(x, z)), E(local.c_prime(x, z)))

                builder.assert_bools([local.a_prime(y, x, z) for z in range(64)])
                builder.assert_zeros([limb_of(get_bit, l) - local.a(y, x, l) for l in limbs])

        # xor_y A'[x, y, z] = C'[x, z]: diff (diff - 2) (diff - 4) = 0 (air.rs:133-143)
        for x in range(5):
            four = TWO.double()
            cs = []
            for z in range(64):
                s = E(local.a_prime(0, x, z))
                for y in range(1, 5):
                    s = s + E(local.a_prime(y, x, z))
                diff = s - local.c_prime(x, z)
                cs.append(diff * (diff - TWO) * (diff - four))
            builder.assert_zeros(cs)

        # A''[x, y] = xor(B[x, y], andn(B[x + 1, y], B[x + 2, y])) (air.rs:145-164)
        for y in range(5):
            for x in range(5):
                def get_bit(z, y=y, x=x):
                    andn = E(local.b((x + 1) % 5, y, z)).andn(E(local.b((x + 2) % 5, y, z)))
                    return andn.xor(E(local.b(x, y, z)))

                builder.assert_zeros([limb_of(get_bit, l) - local.a_prime_prime(y, x, l) for l in limbs])

        # the bits of A''[0, 0] (air.rs:166-177)
        builder.assert_bools([local.a_prime_prime_0_0_bits(z) for z in range(64)])
        builder.assert_zeros([limb_of(lambda z: local.a_prime_prime_0_0_bits(z), l) - local.a_prime_prime(0, 0, l)
                              for l in limbs])

        # A'''[0, 0] = A''[0, 0] xor RC (air.rs:179-197)
        def get_xored_bit(i):
            rc_bit_i = ZERO
            for r in range(NUM_ROUNDS):
                rc_bit_i = rc_bit_i + local.step_flags(r) * SymbolicExpression.from_bool(rc_value_bit(r, i) != 0)
            return rc_bit_i.xor(E(local.a_prime_prime_0_0_bits(i)))

        builder.assert_zeros([limb_of(get_xored_bit, l) - local.a_prime_prime_prime_0_0_limbs(l) for l in limbs])

        # this round's output is the next round's input (air.rs:199-209)
        for x in range(5):
            for y in range(5):
                builder.when_transition().when(not_final_step).assert_zeros(
                    [local.a_prime_prime_prime(y, x, l) - nxt.a(y, x, l) for l in limbs])

    # --- witness -------------------------------------------------------------------------------
    def generate_trace(self, inputs):
        """generate_trace_rows (generation.rs:17-46) on the device.  `inputs`: (n_hashes, 25) int64
        device tensor of u64 bit patterns, input[5x + y] feeding preimage[y][x] (the reference
        transmutes [u64; 25] to a state it indexes [x][y]) -> the (next_pow2(24 n_hashes), 2633, 4)
        int64 trace of Fr Montgomery limbs.  Permutations past n_hashes take the all-zero input, the
        last one is cut to the rows that remain, export is 0.

        n_hashes = 0 is EON_E_SHAPE: the reference builds a 1-row all-zero trace there, which its own
        eval cannot read (it wants a next row and a first step flag)."""
        import torch

        from .dft import default_context

        if not isinstance(inputs, torch.Tensor):
            raise ValueError("inputs must be a torch tensor")
        if inputs.dtype != torch.int64:
            raise ValueError(f"inputs must be int64 (u64 bit patterns), not {inputs.dtype}")
        if inputs.ndim != 2 or inputs.shape[1] != 25:
            raise ValueError(f"inputs must be (n_hashes, 25), not {tuple(inputs.shape)}")
        if inputs.device.type != "cuda":
            raise ValueError(f"inputs must be on the device, not {inputs.device}")
        ctx = self.ctx or default_context(inputs.device.index or 0)
        if (inputs.device.index or 0) != ctx.device:
            raise ValueError(f"inputs are on {inputs.device}, the context on device {ctx.device}")
        n = int(inputs.shape[0])
        rows = keccak_air_rows(n)  # 0 for n = 0, which the library answers with EON_E_SHAPE
        out = torch.empty((rows, NUM_KECCAK_COLS, 4), dtype=torch.int64, device=inputs.device)
        ctx.set_stream(torch.cuda.current_stream(inputs.device).cuda_stream)
        ctx.check(ctx.lib.eon_keccak_generate_trace_dev(ctx.handle, ctypes.c_void_p(inputs.contiguous().data_ptr()), n,
                                                        ctypes.c_void_p(out.data_ptr()), rows))
        return out
