"""The Blake3-AIR above the device boundary, without a GPU: the helpers pack_bits_le / add2 / add3 /
xor_32_shift of the symbolic layer, Blake3Air::eval on the symbolic builder against the constraints
written out directly (tests/airs_blake3.py), and the CPU restatement of the trace generation against
the BLAKE3 compression function and against the constraints -- the yardsticks of
tests/test_gpu_blake3.py."""

import collections
import random

import pytest

import mirror_check as MC
from airs_blake3 import (BLOCKS, BUMP_COL, BUMP_FAILS, BUMP_ROW, CV, FLIP_COL, FLIP_FAILS, FLIP_ROW, HELPERS, INIT_ROW0,
                         INIT_ROW2, INPUTS, IV, MIDDLE, NUM_CONSTRAINTS, OUTPUT, OUTPUTS, PRIME, QR_PARTS, ROUNDS,
                         ROUNDS_AT, WIDTH, P, blake3_constraints, blake3_trace, compress, qr_constraint, row_outputs,
                         smallrng_inputs, state_col, tamper)
from plonky3_eon_amd import symbolic as S
from test_keccak_cpu import evaluate


@pytest.fixture(scope="module")
def constraints():
    from plonky3_eon_amd import Blake3Air

    return S.get_symbolic_constraints(Blake3Air())


@pytest.fixture(scope="module")
def traces():
    """n -> (inputs, rows) of the SmallRng(1) trace: never modified"""
    out = {}
    for n in (1, 2, 4):
        inputs = smallrng_inputs(n)
        out[n] = (inputs, blake3_trace(inputs))
    return out


def test_compress_is_blake3():
    """BLAKE3("") is one compression of the zero block: cv = IV, counter 0, block_len 0, flags
    CHUNK_START | CHUNK_END | ROOT = 11"""
    out = compress(IV, [0] * 16, 0, 0, 11)
    digest = b"".join(v.to_bytes(4, "little") for v in out[:8]).hex()
    assert digest == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"


def test_smallrng_inputs():
    inputs = smallrng_inputs(2)
    assert inputs[0][:3] == [0xCFC5D07F, 0xBF424132, 0x19A37D57]
    assert len(inputs) == 2 and all(len(r) == 24 and all(0 <= v < 1 << 32 for v in r) for r in inputs)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_trace_outputs_are_the_compression(traces, n):
    inputs, rows = traces[n]
    assert len(rows) == n and all(len(r) == WIDTH and all(0 <= v < 1 << 16 for v in r) for r in rows)
    for k, row in enumerate(rows):
        assert row_outputs(row) == compress(inputs[k][16:], inputs[k][:16], k, n, 0)[:8], k
        assert sum(b << i for i, b in enumerate(row[768:800])) == k and sum(b << i for i, b in enumerate(row[832:864])) == n


def test_shape_of_the_air(constraints):
    from plonky3_eon_amd import Blake3Air
    from plonky3_eon_amd import blake3 as B

    air = Blake3Air()
    assert air.width() == WIDTH == 9168 == B.NUM_BLAKE3_COLS and air.num_public_values() == 0
    assert len(constraints) == NUM_CONSTRAINTS == 9760
    assert collections.Counter(c.degree_multiple for c in constraints) == {1: 24, 2: 9512, 3: 224}
    assert S.get_max_constraint_degree(air) == 3 and S.get_log_quotient_degree(air) == 1
    assert (B.COL_CHAINING_VALUES, B.COL_COUNTER_LOW, B.COL_COUNTER_HI, B.COL_BLOCK_LEN, B.COL_FLAGS) == (512, 768, 800,
                                                                                                      832, 864)
    assert (B.COL_INITIAL_ROW0, B.COL_INITIAL_ROW2, B.COL_FULL_ROUNDS, B.ROUND_COLS, B.STATE_COLS) == (896, 904, 912,
                                                                                                     1088, 272)
    assert (B.COL_FINAL_ROUND_HELPERS, B.COL_OUTPUTS) == (8528, 8656)
    assert (B.STATE_ROW0, B.STATE_ROW1, B.STATE_ROW2, B.STATE_ROW3) == (0, 8, 136, 144)
    assert tuple(B.IV) == tuple(IV) and sorted(B.MSG_PERMUTATION) == list(range(16))
    nodes, consts, roots = S.serialize(constraints)
    assert len(roots) == 9760 and 100_000 < len(nodes) < 150_000
    # 1, 2^16, 2 2^16, 2^32, 2 2^32 and the eight limbs of IV[0..4]
    assert sorted(consts) == sorted({1, 1 << 16, 1 << 17, 1 << 32, 1 << 33} | {v for c in IV[:4] for v in (c & 0xFFFF, c >> 16)})


# --- block boundaries -----------------------------------------------------------------------------

def field_of(col):
    """a column's field: the top-level fields, and (round, state, row) inside the rounds"""
    if col < ROUNDS_AT:
        names = (("inputs", INPUTS), ("cv0", CV), ("cv1", CV + 128), ("row3", 768), ("init0", INIT_ROW0),
                 ("init2", INIT_ROW2))
        return [n for n, s in names if s <= col][-1]
    if col < HELPERS:
        c = col - ROUNDS_AT
        r = c % 272
        return (c // 1088, c % 1088 // 272, 0 if r < 8 else 1 if r < 136 else 2 if r < 144 else 3)
    return "helpers" if col < OUTPUTS else f"out{(col - OUTPUTS) // 128}"


def leaves(expr):
    """the fields one constraint reads; every leaf must be a main column of the local row"""
    seen, out, stack = set(), set(), [expr]
    while stack:
        e = stack.pop()
        if id(e) in seen:
            continue
        seen.add(id(e))
        if e.op == "var":
            assert e.var.entry.kind == "main" and e.var.entry.offset == 0, e.var
            out.add(field_of(e.var.index))
        else:
            assert e.op not in ("first", "last", "trans")
        stack += [k for k in (e.x, e.y) if k is not None]
    return out


def quarter_round_reads(rnd, q):
    """per part of airs_blake3.QR_PARTS, the fields quarter round q of round rnd reads: (round, state,
    row) triples, the previous round's output (or the initial state) as its input"""
    if rnd == 0:
        before = ["init0", "cv1", "init2", "row3"]
    else:
        before = [(rnd - 1, OUTPUT, k) for k in range(4)]
    col = q < 4
    a, b, c, d = before if col else [(rnd, MIDDLE, k) for k in range(4)]
    ap, bp, cp, dp = [(rnd, PRIME if col else 2, k) for k in range(4)]
    ao, bo, co, do = [(rnd, MIDDLE if col else OUTPUT, k) for k in range(4)]
    m = "inputs"
    return {"add3_a": {ap, a, b, m}, "xor16": {ap, d, dp}, "add2_c": {cp, c, dp}, "xor12": {cp, b, bp},
            "add3_b": {ao, ap, bp, m}, "xor8": {ao, dp, do}, "add2_d": {co, cp, do}, "xor7": {co, bp, bo}}


def test_blocks_in_assert_order(constraints):
    """the ten blocks of airs_blake3.BLOCKS in order with their counts, and the 56 quarter rounds
    part by part: every constraint reads what its block is about, nothing else, at row offset 0"""
    starts = {}
    k = 0
    for name, count in BLOCKS:
        starts[name] = k
        k += count
    assert k == len(constraints) == 9760
    assert (starts["initial_row0"], starts["initial_row2"], starts["rounds"], starts["helpers_pack"]) == (896, 904, 912, 8976)
    assert (starts["helpers_out0_bools"], starts["outputs0"], starts["outputs1"], starts["outputs2"],
            starts["outputs3"]) == (8984, 9240, 9376, 9504, 9632)
    last = (ROUNDS - 1, OUTPUT)
    reads = {"bools": [{"inputs"}, {"cv0"}, {"cv1"}, {"row3"}], "initial_row0": [{"cv0", "init0"}],
             "initial_row2": [{"init2"}], "helpers_pack": [{"helpers", last + (2,)}],
             "helpers_out0_bools": [{"helpers"}, {"out0"}],
             "outputs0": [{"helpers"}, {"out0", "helpers", last + (0,)}],
             "outputs1": [{"out1", last + (1,), last + (3,)}], "outputs2": [{"out2", "cv0", "helpers"}],
             "outputs3": [{"out3", "cv1", last + (3,)}]}
    for name, count in BLOCKS:
        if name == "rounds":
            continue
        for c in constraints[starts[name]:starts[name] + count]:
            assert leaves(c) in reads[name], (name, leaves(c))
    # the bool block in field order: inputs 512, cv[0] 128, cv[1] 128, then counter / block_len / flags
    assert [leaves(constraints[i]) for i in (0, 511, 512, 639, 640, 767, 768, 895)] == [
        {"inputs"}, {"inputs"}, {"cv0"}, {"cv0"}, {"cv1"}, {"cv1"}, {"row3"}, {"row3"}]
    assert leaves(constraints[9240 + 31]) == {"helpers"} and "out0" in leaves(constraints[9240 + 32])
    for rnd in range(ROUNDS):
        for q in range(8):
            want = quarter_round_reads(rnd, q)
            for part, off, count in QR_PARTS:
                for j in range(count):
                    got = leaves(constraints[qr_constraint(rnd, q, off + j)])
                    if part.startswith("xor") and j < 32:  # the bool checks of the rotated word
                        assert len(got) == 1 and got <= want[part], (rnd, q, part, j, got)
                    else:
                        assert got == want[part], (rnd, q, part, j, got)
    # degrees: add3 cubic, everything else quadratic but the 24 linear packings
    for rnd in range(ROUNDS):
        for q in range(8):
            degs = [constraints[qr_constraint(rnd, q, j)].degree_multiple for j in range(144)]
            assert [j for j, d in enumerate(degs) if d == 3] == [0, 1, 72, 73] and set(degs) == {2, 3}
    assert {c.degree_multiple for c in constraints[896:912]} == {1}
    assert {c.degree_multiple for c in constraints[8976:8984]} == {1}


# --- the helpers ------------------------------------------------------------------------------------

def test_pack_bits_le():
    b = S.SymbolicAirBuilder(0, 16, 0)
    bits = b.main()[0]
    e = S.pack_bits_le(bits)
    assert e.degree_multiple == 1
    rng = random.Random(3)
    for v in [0, 1, 0x8000, 0xFFFF] + [rng.getrandbits(16) for _ in range(8)]:
        env = {"main": [[(v >> i) & 1 for i in range(16)], [0] * 16]}
        assert evaluate([e], env) == [v]
    # the reference's form: a Horner chain from the top bit, acc.double() + bit
    top = "((main0[2] + main0[2]) + main0[1])"
    assert repr(S.pack_bits_le(bits[:3])) == f"(({top} + {top}) + main0[0])"
    assert S.pack_bits_le([]).is_const() and S.pack_bits_le([]).value == 0


def _limbs(v):
    return [v & 0xFFFF, v >> 16]


@pytest.mark.parametrize("terms", [2, 3])
def test_add2_add3(terms):
    """a = b + c (+ d) mod 2^32 on limbs: both checks vanish exactly when the sum is right"""
    b = S.SymbolicAirBuilder(0, 2 * (terms + 1), 0)
    v = b.main()[0]
    pairs = [v[2 * i:2 * i + 2] for i in range(terms + 1)]
    if terms == 2:
        S.add2(b, pairs[0], pairs[1], [S.SymbolicExpression.lift(x) for x in pairs[2]])
    else:
        S.add3(b, pairs[0], pairs[1], *[[S.SymbolicExpression.lift(x) for x in p] for p in pairs[2:]])
    assert [c.degree_multiple for c in b.constraints] == [terms, terms]
    rng = random.Random(5)
    edge = [0, 1, 0xFFFF, 0x10000, 0xFFFFFFFF, 0x80000000]
    cases = [[rng.choice(edge) for _ in range(terms)] for _ in range(40)]
    cases += [[rng.getrandbits(32) for _ in range(terms)] for _ in range(40)]
    for xs in cases:
        good = sum(xs) & 0xFFFFFFFF
        for a in (good, good ^ 1, good ^ 0x10000, (good + 0x8000) & 0xFFFFFFFF):
            row = _limbs(a) + [l for x in xs for l in _limbs(x)]
            vals = evaluate(b.constraints, {"main": [row, [0] * len(row)]})
            assert (vals == [0, 0]) == (a == good), (xs, a, vals)


@pytest.mark.parametrize("shift", [0, 7, 8, 12, 16])
def test_xor_32_shift(shift):
    """a = b ^ rotl(c, shift): 32 bool checks of c, then the two limb equalities"""
    b = S.SymbolicAirBuilder(0, 66, 0)
    v = b.main()[0]
    S.xor_32_shift(b, v[:2], v[2:34], v[34:66], shift)
    assert [c.degree_multiple for c in b.constraints] == [2] * 34
    rng = random.Random(shift)
    for _ in range(20):
        x, y = rng.getrandbits(32), rng.getrandbits(32)
        good = x ^ (((y << shift) | (y >> (32 - shift))) & 0xFFFFFFFF)
        for a in (good, good ^ (1 << rng.randrange(32))):
            row = _limbs(a) + [(x >> i) & 1 for i in range(32)] + [(y >> i) & 1 for i in range(32)]
            vals = evaluate(b.constraints, {"main": [row, [0] * 66]})
            assert vals[:32] == [0] * 32 and (vals[32:] == [0, 0]) == (a == good)
    row = [0, 0] + [0] * 32 + [2] + [0] * 31  # c[0] = 2 is no bit
    assert evaluate(b.constraints, {"main": [row, [0] * 66]})[0] == (1 - 2) * 2 % P


def test_mul_2exp_u64_is_a_constant_product():
    b = S.SymbolicAirBuilder(0, 1, 0)
    x = S.SymbolicExpression.lift(b.main()[0][0])
    e = x.mul_2exp_u64(16)
    assert e.op == "mul" and e.y.is_const() and e.y.value == 1 << 16 and e.degree_multiple == 1


# --- symbolic against written-out, traces against both -------------------------------------------

def test_symbolic_equals_the_written_constraints(constraints):
    rng = random.Random(11)
    for _ in range(2):
        loc, nxt = ([rng.randrange(P) for _ in range(WIDTH)] for _ in range(2))
        sels = tuple(rng.randrange(P) for _ in range(3))
        env = {"main": [loc, nxt], "first": sels[0], "last": sels[1], "trans": sels[2]}
        assert evaluate(constraints, env) == blake3_constraints(loc, nxt, sels, ())


@pytest.mark.parametrize("n", [1, 2, 4])
def test_traces_satisfy_every_constraint(traces, constraints, n):
    rows = traces[n][1]
    assert MC.check_constraints(MC.main_fn(blake3_constraints), rows) == []
    env = {"main": [rows[n - 1], rows[0]], "first": 0, "last": 1, "trans": 0}
    assert evaluate(constraints, env) == [0] * NUM_CONSTRAINTS


def test_tampered_cells_fail_where_expected(traces):
    """the two tampered cells of the n = 4 trace: exactly the listed constraints, on that row only"""
    rows = traces[4][1]
    assert FLIP_COL == state_col(3, MIDDLE, 1, 2, 5) == 4525 and BUMP_COL == state_col(0, PRIME, 0, 1, 0) == 914
    assert FLIP_FAILS == [qr_constraint(3, 2, 142), qr_constraint(3, 5, 0), qr_constraint(3, 5, 1), qr_constraint(3, 5, 70)]
    assert BUMP_FAILS == [qr_constraint(0, 1, j) for j in (0, 1, 34, 72, 73)]
    flipped = tamper(rows, FLIP_ROW, FLIP_COL, 1 - 2 * rows[FLIP_ROW][FLIP_COL])
    fails = MC.check_constraints(MC.main_fn(blake3_constraints), flipped)
    assert [(r, k) for r, k, _ in fails] == [(2, k) for k in [4798, 5088, 5089, 5158]] == [(FLIP_ROW, k) for k in FLIP_FAILS]
    bumped = tamper(rows, BUMP_ROW, BUMP_COL, 1)
    fails = MC.check_constraints(MC.main_fn(blake3_constraints), bumped)
    assert [(r, k) for r, k, _ in fails] == [(1, k) for k in [1056, 1057, 1090, 1128, 1129]] == [(BUMP_ROW, k) for k in BUMP_FAILS]
    assert rows[FLIP_ROW][FLIP_COL] in (0, 1) and rows == traces[4][1]  # the fixture is untouched
