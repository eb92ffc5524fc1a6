"""Big-integer mirror of the radix-2^29 G1 accumulators (csrc/ec29.h) and the case generators of
tests/test_gpu_ec29.py, on oracle/pyoracle.py's affine group law.  Plain Python integers only.

A raw accumulator is 36 words: X, Y, ZZ, ZZZ as 9 limbs each, value sum l[i] << 29 i, holding
x z^2, y z^3, z^2, z^3 times 2^261 modulo q ("29-Montgomery") plus a multiple of q; raw ZZ == 0
is the identity.  The documented invariant is X < 8q, Y < 4q, ZZ < 2q, ZZZ < 3q, ZZZ alone
possibly with lazy limbs < 2^30 (the piece loop's flush negates it limb by limb).

Which formula sees which inputs (the call sites in msm_pieces.hip, msm_reduce.hip and msm_bases.hip):
  * madd29 / madd29_unchecked / madd29_negsum / madd29_exceptional only ever see an accumulator
    built in registers from a base (canonical X, Y, ZZ = ZZZ = one), their own output or
    dbl29_affine's: ZZZ normalised below 2q.  The base is canonical; madd29_negsum alone also
    gets y as a lazy negation (2q - y limb by limb).
  * acc29 and through it add29 / dbl29 read raw pieces (in-wave merge, k_piece_merge29,
    k_bucket_reduce29, k_segment_reduce29, k_bucket_sums29, k_group_finish29): ZZZ lazily
    negated on either side.
  * acc29_ilp and through it add29_ilp / dbl29_ilp / mul29_n read k_bucket_sums29's output,
    which is a copy of the raw piece for a bucket of one piece: lazily negated ZZZ as well.
  * raw29_to_xyzz reads raw pieces (k_raw29_to_xyzz) and x29_to_xyzz whatever acc29 / acc29_ilp
    left, a passed-through piece included: lazily negated ZZZ."""

from oracle import pyoracle as O

Q = O.Q
INF = O.INF
R261 = (1 << 261) % Q
R261_INV = pow(R261, -1, Q)
M29 = (1 << 29) - 1
BOUND = (8, 4, 2, 2)  # X, Y, ZZ, ZZZ (normalised) in multiples of q
TOP = tuple(b - 1 for b in BOUND)  # the largest multiplier of q that keeps a canonical value below the bound

OPS = ("madd", "madd_unchecked", "madd_negsum", "madd_exceptional", "dbl_affine", "dbl", "add", "add_ilp", "dbl_ilp",
       "acc", "acc_ilp", "to_xyzz", "roundtrip", "neg_lazy", "x29_to_xyzz")


# ---- limbs ---------------------------------------------------------------------------------------
def limbs(v):
    assert 0 <= v < 1 << 261
    return [(v >> (29 * i)) & M29 for i in range(9)]


def val(l):
    assert len(l) == 9
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def kpb(k):
    """k q in borrowed limbs (field29.h KPB29): same value, every limb below the top one >= 2^29 - 1."""
    l = limbs(k * Q)
    return [l[0] + (1 << 29)] + [x + (1 << 29) - 1 for x in l[1:8]] + [l[8] - 1]


def neg_lazy(l, k):
    """neg29_lazy<k>: k q - a limb by limb with no carry (a normalised, a < (k - 1) q)."""
    assert all(x <= M29 for x in l) and val(l) < (k - 1) * Q
    r = [b - int(a) for a, b in zip(l, kpb(k))]
    assert all(0 <= x < 1 << 30 for x in r)
    return r


def words32(v):
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def from_words32(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


# ---- encode / decode ------------------------------------------------------------------------------
def encode(pt, z, k=(0, 0, 0, 0), lazy_zzz=False):
    """The 36 words of the accumulator (x z^2, y z^3, z^2, z^3) of the affine point pt, each
    coordinate in 29-Montgomery form plus k[i] q.  lazy_zzz: ZZZ as the piece loop's flush leaves it
    after a flip: 3q - n limb by limb for the normalised representative n (< 2q) of -ZZZ."""
    x, y = pt
    z %= Q
    assert z
    z2, z3 = z * z % Q, z * z * z % Q
    c = [x * z2 % Q, y * z3 % Q, z2, z3]
    if lazy_zzz:
        c[3] = -c[3] % Q
    c = [v * R261 % Q + ki * Q for v, ki in zip(c, k)]
    assert all(v < b * Q for v, b in zip(c, BOUND))
    w = [limbs(v) for v in c]
    if lazy_zzz:
        w[3] = neg_lazy(w[3], 3)
    return w[0] + w[1] + w[2] + w[3]


def identity_words():
    return [0] * 36


def split(words):
    assert len(words) == 36
    return [[int(x) for x in words[9 * j:9 * j + 9]] for j in range(4)]


def coords(words):
    """The four field values (Montgomery factor removed) of a raw accumulator."""
    return [val(l) * R261_INV % Q for l in split(words)]


def is_identity(words):
    return not any(int(x) for x in words[18:27])


def decode(words):
    """The affine point of a raw accumulator (INF for raw ZZ == 0), checked to be a consistent XYZZ
    tuple of a curve point."""
    if is_identity(words):
        return INF
    X, Y, ZZ, ZZZ = coords(words)
    assert ZZ and ZZZ, "ZZ or ZZZ is 0 modulo q in a non-identity accumulator"
    assert pow(ZZ, 3, Q) == ZZZ * ZZZ % Q, "ZZ^3 != ZZZ^2"
    pt = (X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q)
    assert O.g1_is_on_curve(pt), "not on the curve"
    return pt


def zz_is_zero_mod(words):
    """is_zero_mod29 of ZZ: the value 0 or q, normalised."""
    l = split(words)[2]
    return all(x <= M29 for x in l) and val(l) in (0, Q)


def affine_limbs(pt, lazy_neg=False):
    """The 18 limbs of a canonical 29-Montgomery base; lazy_neg: the same point with y written as the
    piece loop writes the negation of the table's entry -pt (neg29_lazy<2>: limbs < 2^30, < 2q)."""
    x, y = pt
    if lazy_neg:
        return limbs(x * R261 % Q) + neg_lazy(limbs(-y * R261 % Q), 2)
    return limbs(x * R261 % Q) + limbs(y * R261 % Q)


def affine_acc(pt):
    """The accumulator a run opens with: (ax, ay, one, one)."""
    return limbs(pt[0] * R261 % Q) + limbs(pt[1] * R261 % Q) + limbs(R261) + limbs(R261)


def check_bounds(words, xb=8, yb=4, lazy_zzz_ok=False):
    """Normalised limbs and X < xb q, Y < yb q, ZZ, ZZZ < 2q (ZZZ: limbs < 2^30, < 3q if lazy_zzz_ok)."""
    l = split(words)
    for j, b in enumerate((xb, yb, 2, 3 if lazy_zzz_ok else 2)):
        top = (1 << 30) if (j == 3 and lazy_zzz_ok) else (1 << 29)
        assert all(x < top for x in l[j]), ("limb", j, l[j])
        assert val(l[j]) < b * Q, ("bound", j, val(l[j]) // Q, b)


# ---- the textbook XYZZ formulas (EFD madd-2008-s, add-2008-s, dbl-2008-s-1 with a = 0), on field values
def tb_dbl(p):
    X1, Y1, ZZ1, ZZZ1 = p
    U = 2 * Y1 % Q
    V = U * U % Q
    W = U * V % Q
    S = X1 * V % Q
    M = 3 * X1 * X1 % Q
    X3 = (M * M - 2 * S) % Q
    return (X3, (M * (S - X3) - W * Y1) % Q, V * ZZ1 % Q, W * ZZZ1 % Q)


def tb_add(p, q):
    """p + q for two XYZZ tuples, None for the identity on either side or as the result."""
    if p is None:
        return q
    if q is None:
        return p
    X1, Y1, ZZ1, ZZZ1 = p
    X2, Y2, ZZ2, ZZZ2 = q
    U1, U2 = X1 * ZZ2 % Q, X2 * ZZ1 % Q
    S1, S2 = Y1 * ZZZ2 % Q, Y2 * ZZZ1 % Q
    P, R = (U2 - U1) % Q, (S2 - S1) % Q
    if P == 0:
        return tb_dbl(p) if R == 0 else None
    PP = P * P % Q
    PPP = P * PP % Q
    Qv = U1 * PP % Q
    X3 = (R * R - PPP - 2 * Qv) % Q
    return (X3, (R * (Qv - X3) - S1 * PPP) % Q, ZZ1 * ZZ2 * PP % Q, ZZZ1 * ZZZ2 * PPP % Q)


def tb_madd(p, a):
    """p + (x2, y2) for an XYZZ tuple and an affine point (mixed addition)."""
    X1, Y1, ZZ1, ZZZ1 = p
    X2, Y2 = a
    U2, S2 = X2 * ZZ1 % Q, Y2 * ZZZ1 % Q
    P, R = (U2 - X1) % Q, (S2 - Y1) % Q
    if P == 0:
        return tb_dbl((X2, Y2, 1, 1)) if R == 0 else None
    PP = P * P % Q
    PPP = P * PP % Q
    Qv = X1 * PP % Q
    X3 = (R * R - PPP - 2 * Qv) % Q
    return (X3, (R * (Qv - X3) - Y1 * PPP) % Q, ZZ1 * PP % Q, ZZZ1 * PPP % Q)


def tb_affine(t):
    if t is None:
        return INF
    X, Y, ZZ, ZZZ = t
    assert pow(ZZ, 3, Q) == ZZZ * ZZZ % Q
    return (X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q)


def tb_tuple(words):
    return None if is_identity(words) else tuple(coords(words))


def affine_point(arg18):
    """The affine point of 18 base limbs (canonical or lazily negated y)."""
    return (val(arg18[:9]) * R261_INV % Q, val(arg18[9:]) * R261_INV % Q)


# ---- points -----------------------------------------------------------------------------------------
_MULT = [INF]


def multiple(k):
    """k G, from a growing table (k small)."""
    while len(_MULT) <= k:
        _MULT.append(O.g1_add(_MULT[-1], O.G1_GEN))
    return _MULT[k]


K_MAX = 200  # generic cases draw k from [1, K_MAX]: k1 != k2 gives points with different x


class Rng:
    def __init__(self, seed):
        self.r = O.SplitMix64(seed)

    def below(self, n):
        return self.r.next() % n

    def z(self):
        """A nonzero field element from four SplitMix64 words."""
        while True:
            v = O.limbs_to_int([self.r.next() for _ in range(4)]) % Q
            if v:
                return v


REP_MODES = ("zero", "top", "rand")


def rep(rng, mode):
    if mode == "zero":
        return (0, 0, 0, 0)
    if mode == "top":
        return TOP
    return tuple(rng.below(b) for b in BOUND)


def acc_class(i, lazy_allowed):
    """Case i's representative mode and whether its ZZZ is lazily negated: all combinations in any
    six (lazy_allowed) or three consecutive cases."""
    return REP_MODES[i % 3], lazy_allowed and (i // 3) % 2 == 1


class Cases:
    """n cases of one op: inputs as word lists, the expected affine result and return code, and
    `same`: 'acc' / 'arg' when the output must equal that input word for word, else None."""

    def __init__(self, op):
        self.op = op
        self.acc, self.arg, self.expect, self.code, self.same = [], [], [], [], []

    def add(self, acc, arg, expect, code, same=None):
        self.acc.append(acc)
        self.arg.append(arg)
        self.expect.append(expect)
        self.code.append(code)
        self.same.append(same)

    def __len__(self):
        return len(self.expect)


# formulas whose accumulator callers can hand a lazily negated ZZZ (module docstring)
LAZY_ZZZ_OPS = ("dbl", "add", "add_ilp", "dbl_ilp", "acc", "acc_ilp", "to_xyzz")
# result bounds (X, Y in multiples of q) as ec29.h states them
OUT_BOUNDS = {"madd": (8, 2), "madd_unchecked": (8, 2), "madd_negsum": (8, 2), "madd_exceptional": (6, 4),
              "dbl_affine": (6, 4), "dbl": (6, 2), "add": (8, 2), "add_ilp": (8, 4), "dbl_ilp": (6, 4)}


def generic_cases(op, n, seed, shift=0):
    """n non-exceptional cases of a curve op; case i is of class acc_class(i + shift)."""
    rng = Rng(seed)
    lazy = op in LAZY_ZZZ_OPS
    cs = Cases(op)
    for i in range(n):
        c = i + shift
        mode, lz = acc_class(c, lazy)
        k1 = 1 + rng.below(K_MAX)
        k2 = 1 + (k1 - 1 + 1 + rng.below(K_MAX - 1)) % K_MAX  # != k1
        P1, P2 = multiple(k1), multiple(k2)
        acc = encode(P1, rng.z(), rep(rng, mode), lz)
        if op in ("madd", "madd_unchecked"):
            cs.add(acc, affine_limbs(P2), O.g1_add(P1, P2), 1 if op == "madd" else 0)
        elif op == "madd_negsum":
            # +y and the lazy -y alternate independently of the representative classes
            cs.add(acc, affine_limbs(P2, lazy_neg=(c // 6) % 2 == 1), O.g1_neg(O.g1_add(P1, P2)), 0)
        elif op == "dbl_affine":
            cs.add(None, affine_limbs(P2), O.g1_add(P2, P2), 0)
        elif op in ("dbl", "dbl_ilp"):
            cs.add(acc, None, O.g1_add(P1, P1), 0)
        elif op in ("add", "add_ilp"):
            mode2, lz2 = acc_class(c // 6 + c, lazy)  # both sides walk through every class
            cs.add(acc, encode(P2, rng.z(), rep(rng, mode2), lz2), O.g1_add(P1, P2), 0)
        else:
            raise ValueError(op)
    return cs


def acc_cases(op, n, seed, shift=0):
    """acc29 / acc29_ilp: the four identity-flag combinations in turn, the representative classes
    under them; with both sides finite every fourth such case is P + P and every fourth P + (-P)."""
    rng = Rng(seed)
    cs = Cases(op)
    for i in range(n):
        c = i + shift
        p_inf, q_inf = bool(c & 1), bool(c & 2)
        mode, lz = acc_class(c // 4, True)
        mode2, lz2 = acc_class(c // 4 + c // 24 + 1, True)
        k1 = 1 + rng.below(K_MAX)
        k2 = 1 + (k1 + rng.below(K_MAX - 1)) % K_MAX
        P1 = multiple(k1)
        kind = (c // 4) % 4 if not (p_inf or q_inf) else 0
        P2 = P1 if kind == 1 else O.g1_neg(P1) if kind == 3 else multiple(k2)
        a = identity_words() if p_inf else encode(P1, rng.z(), rep(rng, mode), lz)
        b = identity_words() if q_inf else encode(P2, rng.z(), rep(rng, mode2), lz2)
        e = O.g1_add(INF if p_inf else P1, INF if q_inf else P2)
        cs.add(a, b, e, 1 if e is INF else 0, "acc" if q_inf else "arg" if p_inf else None)
    return cs


EXC_KINDS = ("equal", "opposite")


def exceptional_cases(op, n, seed):
    """x(acc) == x(arg) with a different z on each side: the two points equal (even cases) or
    opposite (odd).  Expected results per op:
      madd: code 0, output == acc;  madd_exceptional: 2A code 0, or code 1;
      add / add_ilp: code 1 or 2, output == acc;  acc / acc_ilp: 2P code 0, or the identity code 1;
      madd_unchecked / madd_negsum: ZZ becomes 0 modulo q (expect is None, code 0)."""
    rng = Rng(seed)
    cs = Cases(op)
    lazy = op in LAZY_ZZZ_OPS
    for i in range(n):
        opposite = i % 2 == 1
        mode, lz = acc_class(i // 2, lazy)
        P1 = multiple(1 + rng.below(K_MAX))
        A = O.g1_neg(P1) if opposite else P1
        acc = encode(P1, rng.z(), rep(rng, mode), lz)
        total = INF if opposite else O.g1_add(P1, P1)
        if op == "madd":
            cs.add(acc, affine_limbs(A), P1, 0, "acc")
        elif op == "madd_exceptional":
            cs.add(acc, affine_limbs(A), total, 1 if opposite else 0)
        elif op in ("madd_unchecked", "madd_negsum"):
            cs.add(acc, affine_limbs(A, lazy_neg=(op == "madd_negsum" and (i // 2) % 2 == 1)), None, 0)
        elif op in ("add", "add_ilp"):
            mode2, lz2 = acc_class(i // 2 + i // 12 + 1, lazy)
            cs.add(acc, encode(A, rng.z(), rep(rng, mode2), lz2), P1, 2 if opposite else 1, "acc")
        elif op in ("acc", "acc_ilp"):
            mode2, lz2 = acc_class(i // 2 + i // 12 + 1, lazy)
            cs.add(acc, encode(A, rng.z(), rep(rng, mode2), lz2), total, 1 if opposite else 0)
        else:
            raise ValueError(op)
    return cs


# ---- chains as the piece loop drives them -----------------------------------------------------------
CHAIN_STEPS = 16
# base j of a chain is c 4^j G with c in 1..3: 4^j exceeds the sum of all earlier multipliers, so no
# signed partial sum meets the next base or its negation and no step is exceptional
_CHAIN_BASES = {}


def chain_base(j, c):
    if (j, c) not in _CHAIN_BASES:
        _CHAIN_BASES[(j, c)] = O.g1_mul(O.G1_GEN, c * 4 ** j)
    return _CHAIN_BASES[(j, c)]


def chain_plan(n, seed):
    """n chains of CHAIN_STEPS + 1 signed bases: per chain a list of (point, neg_digit)."""
    rng = Rng(seed)
    return [[(chain_base(j, 1 + rng.below(3)), bool(rng.below(2))) for j in range(CHAIN_STEPS + 1)] for _ in range(n)]


def chain_sums(plan):
    """Per chain the oracle's signed partial sums after base 0, 1, ..."""
    out = []
    for ch in plan:
        s, sums = INF, []
        for pt, ng in ch:
            s = O.g1_add(s, O.g1_neg(pt) if ng else pt)
            sums.append(s)
        out.append(sums)
    return out


# ---- conversions -------------------------------------------------------------------------------------
def to_xyzz_cases(n, seed, shift=0):
    """raw29_to_xyzz: expected 36 output words (four canonical radix-2^32 Montgomery coordinates,
    x 2^256 = the 29-Montgomery value / 32, then four zero words) and the identity code; every
    seventh case is the identity with nonzero X, Y, ZZZ words."""
    rng = Rng(seed)
    inv32 = pow(32, -1, Q)
    one256 = (1 << 256) % Q
    cs = Cases("to_xyzz")
    for i in range(n):
        c = i + shift
        mode, lz = acc_class(c, True)
        w = encode(multiple(1 + rng.below(K_MAX)), rng.z(), rep(rng, mode), lz)
        if c % 7 == 6:
            w[18:27] = [0] * 9
            e = words32(one256) * 2 + [0] * 16
        else:
            e = sum((words32(val(l) * inv32 % Q) for l in split(w)), [])
        cs.add(w, None, e + [0] * 4, 1 if c % 7 == 6 else 0)
    return cs


def neg_lazy_cases(n, seed):
    """The piece loop's two lazy negations on their own words: X = a canonical y (neg29_lazy<2>),
    ZZZ normalised below 2q (neg29_lazy<3>), Y and ZZ passed through; the extreme values first."""
    rng = Rng(seed)
    edge = [(0, 0), (Q - 1, 2 * Q - 1), (1, Q), (Q - 1, 0)]
    cs = Cases("neg_lazy")
    for i in range(n):
        x, zzz = edge[i] if i < len(edge) else (rng.z(), rng.z() + rng.below(2) * Q)
        w = limbs(x) + limbs(rng.z()) + limbs(rng.z()) + limbs(zzz)
        cs.add(w, None, neg_lazy(w[:9], 2) + w[9:27] + neg_lazy(w[27:], 3), 0)
    return cs


def roundtrip_cases(n, seed):
    """to_fq261(to_fq256(a)) == a for canonical a: 0, 1, q - 1 and 2^261 mod q first, then random."""
    rng = Rng(seed)
    fixed = [0, 1, Q - 1, R261, Q - 2, 1 << 253]
    cs = Cases("roundtrip")
    for i in range(n):
        v = [fixed[(4 * i + j) % len(fixed)] if 4 * i + j < 2 * len(fixed) else rng.z() for j in range(4)]
        cs.add(sum((limbs(x) for x in v), []), None, sum((words32(x) for x in v), []) + [0] * 4, 0)
    return cs
