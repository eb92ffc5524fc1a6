"""The Blake3-AIR (blake3-air/src/{air,columns,generation,constants}.rs, air/src/utils.rs) restated
over Python ints.  TEST INFRASTRUCTURE ONLY: the yardstick of plonky3_eon_amd.blake3 and of the
device trace generation, sharing no code with either.

* ``compress``            the BLAKE3 compression function, all sixteen output words
* ``blake3_trace``        generate_trace_rows (generation.rs:16-121) -> rows of ints < 2^16
* ``blake3_constraints``  every assert_zero value of Blake3Air::eval, in assert order, in the shape
                          pyoracle.quotient_values_fn / mirror_check.main_fn take
* ``trace_limbs``         rows -> (n, 9168, 4) u64 Montgomery limbs (airs_keccak's 65,536-entry table)
"""

from airs_keccak import mont16_table, trace_limbs  # noqa: F401

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
M32 = (1 << 32) - 1
ROUNDS = 7
IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
MSG_PERMUTATION = (2, 6, 3, 10, 7, 0, 4, 13, 1, 11, 12, 5, 9, 14, 15, 8)

# Blake3Cols as column offsets
INPUTS, CV, COUNTER_LOW, COUNTER_HI, BLOCK_LEN, FLAGS = 0, 512, 768, 800, 832, 864
INIT_ROW0, INIT_ROW2, ROUNDS_AT, HELPERS, OUTPUTS, WIDTH = 896, 904, 912, 8528, 8656, 9168
ROUND_COLS, STATE_COLS = 1088, 272
ROW0, ROW1, ROW2, ROW3 = 0, 8, 136, 144  # inside a Blake3State
PRIME, MIDDLE, MIDDLE_PRIME, OUTPUT = range(4)  # the states of a FullRound

# constraint blocks in assert order
QR_CONSTRAINTS, ROUND_CONSTRAINTS = 144, 1152
BLOCKS = (("bools", 896), ("initial_row0", 8), ("initial_row2", 8), ("rounds", ROUNDS * ROUND_CONSTRAINTS),
          ("helpers_pack", 8), ("helpers_out0_bools", 256), ("outputs0", 136), ("outputs1", 128), ("outputs2", 128),
          ("outputs3", 128))
NUM_CONSTRAINTS = sum(n for _, n in BLOCKS)  # 9760
# inside a quarter round: (offset, count)
QR_PARTS = (("add3_a", 0, 2), ("xor16", 2, 34), ("add2_c", 36, 2), ("xor12", 38, 34), ("add3_b", 72, 2),
            ("xor8", 74, 34), ("add2_d", 108, 2), ("xor7", 110, 34))


def state_col(rnd, state, row, i, k=0):
    """the column of full_rounds[rnd].<state>.row<row>[i][k]: k a limb for rows 0 and 2, a bit for 1 and 3"""
    base = ROUNDS_AT + ROUND_COLS * rnd + STATE_COLS * state
    return base + (ROW0, ROW1, ROW2, ROW3)[row] + (2 if row in (0, 2) else 32) * i + k


def qr_constraint(rnd, q, offset=0):
    """the first constraint of quarter round q of round rnd (q = 0..3 columns, 4..7 diagonals) + offset"""
    return 912 + ROUND_CONSTRAINTS * rnd + QR_CONSTRAINTS * q + offset


def rotr(v, n):
    return ((v >> n) | (v << (32 - n))) & M32


def _g(s, a, b, c, d, mx, my):
    s[a] = (s[a] + s[b] + mx) & M32
    s[d] = rotr(s[d] ^ s[a], 16)
    s[c] = (s[c] + s[d]) & M32
    s[b] = rotr(s[b] ^ s[c], 12)
    s[a] = (s[a] + s[b] + my) & M32
    s[d] = rotr(s[d] ^ s[a], 8)
    s[c] = (s[c] + s[d]) & M32
    s[b] = rotr(s[b] ^ s[c], 7)


def compress(cv, block, counter, block_len, flags):
    """BLAKE3's compression function (the BLAKE3 paper, section 2.2): sixteen output words, the
    first eight the new chaining value."""
    s = list(cv) + list(IV[:4]) + [counter & M32, (counter >> 32) & M32, block_len & M32, flags & M32]
    m = list(block)
    for r in range(ROUNDS):
        _g(s, 0, 4, 8, 12, m[0], m[1])
        _g(s, 1, 5, 9, 13, m[2], m[3])
        _g(s, 2, 6, 10, 14, m[4], m[5])
        _g(s, 3, 7, 11, 15, m[6], m[7])
        _g(s, 0, 5, 10, 15, m[8], m[9])
        _g(s, 1, 6, 11, 12, m[10], m[11])
        _g(s, 2, 7, 8, 13, m[12], m[13])
        _g(s, 3, 4, 9, 14, m[14], m[15])
        if r + 1 < ROUNDS:
            m = [m[MSG_PERMUTATION[i]] for i in range(16)]
    return [s[i] ^ s[i + 8] for i in range(8)] + [s[i + 8] ^ cv[i] for i in range(8)]


def _bits(v):
    return [(v >> i) & 1 for i in range(32)]


def _limbs(v):
    return [v & 0xFFFF, v >> 16]


def _half(a, b, c, d, m, second):
    """verifiable_half_round (generation.rs:206-230)"""
    r1, r2 = (8, 7) if second else (16, 12)
    a = (a + b + m) & M32
    d = rotr(d ^ a, r1)
    c = (c + d) & M32
    b = rotr(b ^ c, r2)
    return a, b, c, d


def _save(row, base, st):
    """save_state_to_trace (generation.rs:232-250)"""
    for i in range(4):
        row[base + ROW0 + 2 * i:base + ROW0 + 2 * i + 2] = _limbs(st[0][i])
        row[base + ROW1 + 32 * i:base + ROW1 + 32 * i + 32] = _bits(st[1][i])
        row[base + ROW2 + 2 * i:base + ROW2 + 2 * i + 2] = _limbs(st[2][i])
        row[base + ROW3 + 32 * i:base + ROW3 + 32 * i + 32] = _bits(st[3][i])


def _row(inp, counter, block_len):
    """generate_trace_rows_for_perm (generation.rs:49-121)"""
    row = [0] * WIDTH
    for i in range(24):
        row[32 * i:32 * i + 32] = _bits(inp[i])  # inputs, then chaining_values
    row[COUNTER_LOW:COUNTER_LOW + 32] = _bits(counter & M32)
    row[COUNTER_HI:COUNTER_HI + 32] = _bits((counter >> 32) & M32)
    row[BLOCK_LEN:BLOCK_LEN + 32] = _bits(block_len & M32)
    for i in range(4):
        row[INIT_ROW0 + 2 * i:INIT_ROW0 + 2 * i + 2] = _limbs(inp[16 + i])
        row[INIT_ROW2 + 2 * i:INIT_ROW2 + 2 * i + 2] = _limbs(IV[i])
    m = list(inp[:16])
    st = [list(inp[16:20]), list(inp[20:24]), list(IV[:4]), [counter & M32, (counter >> 32) & M32, block_len & M32, 0]]
    for r in range(ROUNDS):
        base = ROUNDS_AT + ROUND_COLS * r
        for second in (False, True):
            for i in range(4):
                st[0][i], st[1][i], st[2][i], st[3][i] = _half(st[0][i], st[1][i], st[2][i], st[3][i],
                                                               m[2 * i + second], second)
            _save(row, base + STATE_COLS * (MIDDLE if second else PRIME), st)
        for second in (False, True):
            for i in range(4):
                j, k, l = (i + 1) % 4, (i + 2) % 4, (i + 3) % 4
                st[0][i], st[1][j], st[2][k], st[3][l] = _half(st[0][i], st[1][j], st[2][k], st[3][l],
                                                               m[8 + 2 * i + second], second)
            _save(row, base + STATE_COLS * (OUTPUT if second else MIDDLE_PRIME), st)
        m = [m[MSG_PERMUTATION[i]] for i in range(16)]
    for i in range(4):
        row[HELPERS + 32 * i:HELPERS + 32 * i + 32] = _bits(st[2][i])
        for k, v in enumerate((st[0][i] ^ st[2][i], st[1][i] ^ st[3][i], st[2][i] ^ inp[16 + i], st[3][i] ^ inp[20 + i])):
            row[OUTPUTS + 128 * k + 32 * i:OUTPUTS + 128 * k + 32 * i + 32] = _bits(v)
    return row


def blake3_trace(inputs):
    """generate_trace_rows (generation.rs:16-46): row k is the compression of inputs[k] with
    counter = k, block_len = len(inputs), flags = 0; the length is a power of two."""
    n = len(inputs)
    assert n > 0 and n & (n - 1) == 0
    return [_row([int(v) & M32 for v in inp], k, n) for k, inp in enumerate(inputs)]


def row_outputs(row):
    """outputs[0..1] of a row packed into eight u32 words"""
    return [sum(row[OUTPUTS + 32 * i + b] << b for b in range(32)) for i in range(8)]


def smallrng_inputs(n, seed=1):
    """Blake3Air::generate_trace_rows's inputs (air.rs:22-30): n draws of [u32; 24] from SmallRng(seed)."""
    from oracle.smallrng import SmallRng

    rng = SmallRng.seed_from_u64(seed)
    return [[rng.next_u32() for _ in range(24)] for _ in range(n)]


def _xor(a, b):
    return a + b - 2 * a * b


def _pack(bits):
    return sum(int(b) << k for k, b in enumerate(bits))


def _halves(bits):
    return [_pack(bits[:16]), _pack(bits[16:])]


def _carries(out, acc_16, acc_32, n):
    """add2 (n = 1) and add3 (n = 2) (air/src/utils.rs:82-194) on the two limb differences"""
    acc = (acc_16 + (acc_32 << 16)) % P
    acc_16 %= P
    for v, step in ((acc, 1 << 32), (acc_16, 1 << 16)):
        prod = v * (v + step) % P
        if n == 2:
            prod = prod * (v + 2 * step)
        out.append(prod)


def _xor_shift(out, a, b, c, shift):
    """xor_32_shift (air/src/utils.rs:202-230)"""
    out += [(1 - v) * v for v in c]
    x = [_xor(b[i], c[(32 + i - shift) % 32]) % P for i in range(32)]
    out += [a[0] - _pack(x[:16]), a[1] - _pack(x[16:])]


def _quarter(out, a, b, c, d, mx, my, prime, output):
    """quarter_round_function (air.rs:38-106)"""
    ap, bp, cp, dp = prime
    ao, bo, co, do = output
    hb, hdp, hbp, hdo = _halves(b), _halves(dp), _halves(bp), _halves(do)
    _carries(out, ap[0] - a[0] - hb[0] - mx[0], ap[1] - a[1] - hb[1] - mx[1], 2)
    _xor_shift(out, ap, d, dp, 16)
    _carries(out, cp[0] - c[0] - hdp[0], cp[1] - c[1] - hdp[1], 1)
    _xor_shift(out, cp, b, bp, 12)
    _carries(out, ao[0] - ap[0] - hbp[0] - my[0], ao[1] - ap[1] - hbp[1] - my[1], 2)
    _xor_shift(out, ao, dp, do, 8)
    _carries(out, co[0] - cp[0] - hdo[0], co[1] - cp[1] - hdo[1], 1)
    _xor_shift(out, co, bp, bo, 7)


def _state(loc, base):
    return ([loc[base + ROW0 + 2 * i:base + ROW0 + 2 * i + 2] for i in range(4)],
            [loc[base + ROW1 + 32 * i:base + ROW1 + 32 * i + 32] for i in range(4)],
            [loc[base + ROW2 + 2 * i:base + ROW2 + 2 * i + 2] for i in range(4)],
            [loc[base + ROW3 + 32 * i:base + ROW3 + 32 * i + 32] for i in range(4)])


def blake3_constraints(loc, nxt=None, sels=None, publics=()):
    """The 9760 assert_zero values in assert order (BLOCKS), mod P.  Only the local row is read."""
    out = []
    word = lambda base, i: loc[base + 32 * i:base + 32 * i + 32]  # noqa: E731
    inputs = [word(INPUTS, i) for i in range(16)]
    cv = [word(CV, i) for i in range(8)]
    row3 = [word(COUNTER_LOW, i) for i in range(4)]
    init0 = [loc[INIT_ROW0 + 2 * i:INIT_ROW0 + 2 * i + 2] for i in range(4)]
    init2 = [loc[INIT_ROW2 + 2 * i:INIT_ROW2 + 2 * i + 2] for i in range(4)]
    helpers = [word(HELPERS, i) for i in range(4)]
    outs = [[word(OUTPUTS + 128 * k, i) for i in range(4)] for k in range(4)]
    # bool checks of the first 896 columns (air.rs:247-257)
    out += [(1 - v) * v for v in loc[:INIT_ROW0]]
    # initial_row0 packs cv[0..4], initial_row2 is IV[0..4] (air.rs:261-280)
    for i in range(4):
        h = _halves(cv[i])
        out += [h[0] - init0[i][0], h[1] - init0[i][1]]
    for i in range(4):
        out += [init2[i][0] - (IV[i] & 0xFFFF), init2[i][1] - (IV[i] >> 16)]
    # the rounds (air.rs:296-365)
    m = [_halves(w) for w in inputs]
    st = (init0, cv[4:8], init2, row3)
    for r in range(ROUNDS):
        base = ROUNDS_AT + ROUND_COLS * r
        prime, middle, mprime, output = (_state(loc, base + STATE_COLS * s) for s in range(4))
        for i in range(4):
            _quarter(out, st[0][i], st[1][i], st[2][i], st[3][i], m[2 * i], m[2 * i + 1],
                     (prime[0][i], prime[1][i], prime[2][i], prime[3][i]),
                     (middle[0][i], middle[1][i], middle[2][i], middle[3][i]))
        for i in range(4):
            j, k, l = (i + 1) % 4, (i + 2) % 4, (i + 3) % 4
            _quarter(out, middle[0][i], middle[1][j], middle[2][k], middle[3][l], m[2 * i + 8], m[2 * i + 9],
                     (mprime[0][i], mprime[1][j], mprime[2][k], mprime[3][l]),
                     (output[0][i], output[1][j], output[2][k], output[3][l]))
        st = output
        m = [m[MSG_PERMUTATION[i]] for i in range(16)]
    # the helpers are the bits of state[8..12] (air.rs:373-389)
    for i in range(4):
        h = _halves(helpers[i])
        out += [h[0] - st[2][i][0], h[1] - st[2][i][1]]
    out += [(1 - v) * v for w in helpers + outs[0] for v in w]
    # outputs[0] (air.rs:394-403), then outputs[1..3] bit by bit (air.rs:408-445)
    for i in range(4):
        _xor_shift(out, st[0][i], outs[0][i], helpers[i], 0)
    for k, lefts, rights in ((1, st[1], st[3]), (2, cv[:4], helpers), (3, cv[4:], st[3])):
        for i in range(4):
            out += [outs[k][i][b] - _xor(lefts[i][b], rights[i][b]) for b in range(32)]
    return [v % P for v in out]


def tamper(rows, row, col, delta):
    """a copy of `rows` with `delta` added to one cell (a bit flip is +1 or -1)"""
    out = [list(r) for r in rows]
    out[row][col] += delta
    return out


# the two tampered cells of the n = 4, seed 1 trace and the constraints each breaks, which do not
# depend on the data: every constraint is linear or cubic in the cell, and the change is no multiple of 2^16
#   full_rounds[3].state_middle.row1[2] bit 5 (column 4525) flipped on row 2 (still a bit, so no bool
#   check fails): it is b_output of round 3's column quarter round 2, whose xor by 7 puts it into the low
#   limb (4798 = qr_constraint(3, 2, 142)), and b of diagonal 1: both checks of its first add3 (5088,
#   5089) and the low limb of its xor by 12 (5158 = qr_constraint(3, 5, 70))
FLIP_ROW, FLIP_COL, FLIP_FAILS = 2, 4525, [4798, 5088, 5089, 5158]
#   full_rounds[0].state_prime.row0[1] low limb (column 914) plus 1 on row 1: a_prime of round 0's column
#   quarter round 1: both checks of the first add3 (1056, 1057), the low limb of the xor by 16 (1090) and
#   both checks of the second add3 (1128, 1129)
BUMP_ROW, BUMP_COL, BUMP_FAILS = 1, 914, [1056, 1057, 1090, 1128, 1129]
