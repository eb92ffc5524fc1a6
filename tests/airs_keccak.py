"""The Keccak-AIR (keccak-air/src/{air,columns,generation,round_flags}.rs) restated over Python
ints.  TEST INFRASTRUCTURE ONLY: the yardstick of plonky3_eon_amd.keccak and of the device trace
generation, sharing no code with either.

* ``keccak_f1600``        the standard permutation (FIPS 202 3.3), lanes S[x + 5y]
* ``keccak_trace``        generate_trace_rows (generation.rs:17-137) -> rows of ints < 2^16
* ``keccak_constraints``  every assert_zero value of eval_round_flags + KeccakAir::eval, in assert
                          order, in the shape pyoracle.quotient_values_fn / mirror_check.main_fn take
* ``trace_limbs``         rows -> (n, 2633, 4) u64 Montgomery limbs through a 65,536-entry table

The constants are derived from FIPS 202 here as well: rc(t) of algorithm 5 and the rho walk of 3.2.2.
"""

import numpy as np

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
M64 = (1 << 64) - 1
ROUNDS = 24

# KeccakCols (columns.rs:18-61) as column offsets
STEP, EXPORT, PRE, A, C, CP, AP, APP, BITS, APPP, WIDTH = 0, 24, 25, 125, 225, 545, 865, 2465, 2565, 2629, 2633
# constraint blocks in assert order
BLOCKS = (("round_flags", 48), ("preimage_first", 100), ("preimage_carried", 100), ("export", 2), ("c_c_prime", 640),
          ("a_prime_a", 1700), ("parity_cubic", 320), ("a_prime_prime", 100), ("a_prime_prime_0_0_bits", 68),
          ("a_prime_prime_prime_0_0", 4), ("next_a", 100))
NUM_CONSTRAINTS = sum(n for _, n in BLOCKS)  # 3182


def _rc(t):
    reg = 1
    for _ in range(t % 255):
        reg <<= 1
        if reg & 0x100:
            reg ^= 0x171
    return reg & 1


RC = [sum(_rc(j + 7 * ir) << ((1 << j) - 1) for j in range(7)) for ir in range(ROUNDS)]


def _rho():
    r = [[0] * 5 for _ in range(5)]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = (t + 1) * (t + 2) // 2 % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


R = _rho()  # R[x][y]


def rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f1600(lanes):
    """FIPS 202 3.3 on 25 lanes, lanes[x + 5y] = lane (x, y)."""
    a = [[lanes[x + 5 * y] for y in range(5)] for x in range(5)]
    for ir in range(ROUNDS):
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = rotl(a[x][y], R[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & M64 & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= RC[ir]
    return [a[i % 5][i // 5] for i in range(25)]


def _limbs(v):
    return [(v >> (16 * i)) & 0xFFFF for i in range(4)]


def _bits(v):
    return [(v >> i) & 1 for i in range(64)]


def _perm_rows(inp, n_rows):
    """generate_trace_rows_for_perm (generation.rs:49-137): `n_rows` <= 24 rows of one permutation."""
    st = [[inp[5 * i + j] for j in range(5)] for i in range(5)]  # the transmuted input, indexed [x][y]
    pre = [l for y in range(5) for x in range(5) for l in _limbs(st[x][y])]
    rows = []
    for rnd in range(n_rows):
        row = [0] * WIDTH
        row[STEP + rnd] = 1
        row[PRE:PRE + 100] = pre
        row[A:A + 100] = [l for y in range(5) for x in range(5) for l in _limbs(st[x][y])]
        c = [st[x][0] ^ st[x][1] ^ st[x][2] ^ st[x][3] ^ st[x][4] for x in range(5)]
        cp = [c[x] ^ c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
        row[C:C + 320] = [b for x in range(5) for b in _bits(c[x])]
        row[CP:CP + 320] = [b for x in range(5) for b in _bits(cp[x])]
        st = [[st[x][y] ^ c[x] ^ cp[x] for y in range(5)] for x in range(5)]
        row[AP:AP + 1600] = [b for y in range(5) for x in range(5) for b in _bits(st[x][y])]
        bb = [[rotl(st[(i + 3 * j) % 5][i], R[(i + 3 * j) % 5][i]) for j in range(5)] for i in range(5)]
        st = [[bb[i][j] ^ (~bb[(i + 1) % 5][j] & M64 & bb[(i + 2) % 5][j]) for j in range(5)] for i in range(5)]
        row[APP:APP + 100] = [l for y in range(5) for x in range(5) for l in _limbs(st[x][y])]
        row[BITS:BITS + 64] = _bits(st[0][0])
        st[0][0] ^= RC[rnd]
        row[APPP:APPP + 4] = _limbs(st[0][0])
        rows.append(row)
    return rows


def keccak_trace(inputs):
    """generate_trace_rows (generation.rs:17-46): next_pow2(24 n) rows; permutations past the inputs
    take the zero input and the last one is cut to the rows that remain; export stays 0."""
    n = len(inputs)
    assert n > 0
    n_rows = 1 << (ROUNDS * n - 1).bit_length()
    rows = []
    k = 0
    while len(rows) < n_rows:
        inp = [int(v) & M64 for v in inputs[k]] if k < n else [0] * 25
        rows += _perm_rows(inp, min(ROUNDS, n_rows - len(rows)))
        k += 1
    return rows


def smallrng_inputs(n_hashes, seed=1):
    """KeccakAir::generate_trace_rows's inputs (air.rs:21-29): n draws of [u64; 25] from SmallRng(seed)."""
    from oracle.smallrng import SmallRng

    rng = SmallRng.seed_from_u64(seed)
    return [[rng.next_u64() for _ in range(25)] for _ in range(n_hashes)]


def _xor(a, b):
    return a + b - 2 * a * b


def _xor3(a, b, c):
    return _xor(_xor(a, b), c)


def keccak_constraints(loc, nxt, sels, publics=()):
    """The 3182 assert_zero values in assert order (BLOCKS), mod P."""
    first, last, trans = sels[:3]
    out = []
    flags, nflags = loc[STEP:STEP + 24], nxt[STEP:STEP + 24]
    # 1 round flags (round_flags.rs:22-57)
    out.append(first * (flags[0] - 1))
    out += [first * flags[i] for i in range(1, 24)]
    out += [trans * (flags[i] - nflags[(i + 1) % 24]) for i in range(24)]
    first_step, not_final = flags[0], 1 - flags[23]
    # 2, 3 preimage (air.rs:55-76)
    out += [first_step * (loc[PRE + k] - loc[A + k]) for k in range(100)]
    out += [not_final * (trans * (loc[PRE + k] - nxt[PRE + k])) for k in range(100)]
    # 4 export (air.rs:78-84)
    e = loc[EXPORT]
    out += [(1 - e) * e, not_final * e]
    # 5 C and C' (air.rs:86-99)
    c = [loc[C + 64 * x:C + 64 * x + 64] for x in range(5)]
    cp = [loc[CP + 64 * x:CP + 64 * x + 64] for x in range(5)]
    for x in range(5):
        out += [(1 - v) * v for v in c[x]]
        out += [cp[x][z] - _xor3(c[x][z], c[(x + 4) % 5][z], c[(x + 1) % 5][(z + 63) % 64]) for z in range(64)]
    # 6 A' boolean, A = xor(A', C, C') limb by limb (air.rs:101-131)
    ap = [[loc[AP + 64 * (5 * y + x):AP + 64 * (5 * y + x) + 64] for x in range(5)] for y in range(5)]  # [y][x][z]
    for y in range(5):
        for x in range(5):
            out += [(1 - v) * v for v in ap[y][x]]
            bits = [_xor3(ap[y][x][z], c[x][z], cp[x][z]) % P for z in range(64)]
            out += [sum(bits[16 * l + k] << k for k in range(16)) - loc[A + 4 * (5 * y + x) + l] for l in range(4)]
    # 7 the 5-way parity (air.rs:133-143)
    for x in range(5):
        for z in range(64):
            diff = sum(ap[y][x][z] for y in range(5)) - cp[x][z]
            out.append(diff * (diff - 2) % P * (diff - 4))

    def b(x, y, z):  # columns.rs:64-79
        a = (x + 3 * y) % 5
        return ap[x][a][(z + 64 - R[a][x]) % 64]

    # 8 A'' (air.rs:145-164)
    for y in range(5):
        for x in range(5):
            bits = [_xor((1 - b((x + 1) % 5, y, z)) * b((x + 2) % 5, y, z) % P, b(x, y, z)) % P for z in range(64)]
            out += [sum(bits[16 * l + k] << k for k in range(16)) - loc[APP + 4 * (5 * y + x) + l] for l in range(4)]
    # 9 the bits of A''[0][0] (air.rs:166-177)
    bits00 = loc[BITS:BITS + 64]
    out += [(1 - v) * v for v in bits00]
    out += [sum(bits00[16 * l + k] << k for k in range(16)) - loc[APP + l] for l in range(4)]
    # 10 A'''[0][0] = A''[0][0] xor RC (air.rs:179-197)
    xored = [_xor(sum(flags[r] for r in range(24) if (RC[r] >> i) & 1), bits00[i]) % P for i in range(64)]
    out += [sum(xored[16 * l + k] << k for k in range(16)) - loc[APPP + l] for l in range(4)]
    # 11 next row's A (air.rs:199-209): x outer, y inner
    for x in range(5):
        for y in range(5):
            for l in range(4):
                cur = loc[APPP + l] if (x, y) == (0, 0) else loc[APP + 4 * (5 * y + x) + l]
                out.append(trans * (not_final * (cur - nxt[A + 4 * (5 * y + x) + l])))
    return [v % P for v in out]


_MONT16 = None


def mont16_table():
    """(65536, 4) u64: the Montgomery limbs of every 16-bit value."""
    global _MONT16
    if _MONT16 is None:
        r = (1 << 256) % P
        t = np.empty((1 << 16, 4), dtype=np.uint64)
        v = 0
        for i in range(1 << 16):
            t[i] = [(v >> (64 * k)) & M64 for k in range(4)]
            v += r
            if v >= P:
                v -= P
        _MONT16 = t
    return _MONT16


def trace_limbs(rows):
    """rows of ints < 2^16 -> (n, width, 4) u64 Montgomery limbs"""
    idx = np.asarray(rows, dtype=np.int64)
    assert idx.min() >= 0 and idx.max() < 1 << 16
    return mont16_table()[idx]


def b_col(x, y, z):
    """the column that holds B[x][y][z] (columns.rs:64-79): a bit of a_prime[x][(x + 3y) mod 5]"""
    a = (x + 3 * y) % 5
    return AP + 64 * (5 * x + a) + (z + 64 - R[a][x]) % 64


def flip_a_prime_bit(rows, row=5, y=2, x=3, z=17):
    """a copy of `rows` with a_prime[y][x][z] of one row flipped"""
    out = [list(r) for r in rows]
    out[row][AP + 64 * (5 * y + x) + z] ^= 1
    return out


def flipped_bit_failures(rows, row=5):
    """The constraints that flip_a_prime_bit(rows, row, y=2, x=3, z=17) breaks on `row`, from the
    constraints' own structure.  Always: limb 1 of a[2][3] (1839 = 890 + 68 * 13 + 64 + 1) and the
    parity of (x = 3, z = 17) (2799 = 2590 + 64 * 3 + 17).  The bit is B[2][2][42] (r[3][2] = 25), so
    limb 2 of A''[x][2] = B[x] ^ (~B[x + 1] & B[x + 2]) changes for x = 2 always (2960), for x = 1
    where B[3][2][42] = 1 (2956) and for x = 0 where B[1][2][42] = 0 (2952): the last two depend on
    the row's data."""
    assert b_col(2, 2, 42) == AP + 64 * (5 * 2 + 3) + 17
    r = rows[row]
    out = [1839, 2799]
    if r[b_col(1, 2, 42)] == 0:
        out.append(2910 + 4 * 10 + 2)
    if r[b_col(3, 2, 42)] == 1:
        out.append(2910 + 4 * 11 + 2)
    return out + [2910 + 4 * 12 + 2]
