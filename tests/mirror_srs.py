"""Big-int mirror of the SRS loader (csrc/srs.hip): the decompressor with the kernel's rejection
rules, the per-point validation, and the helpers the tests build their bad inputs with.  Points
are the oracle's: (x, y) canonical ints, None = identity."""

from oracle import pairing as E
from oracle import pyoracle as O

Q = O.Q
R = O.P
OK, ENCODING, NOT_CANONICAL, NOT_ON_CURVE, IDENTITY = "OK", "ENCODING", "NOT_CANONICAL", "NOT_ON_CURVE", "IDENTITY"
G0_NOT_GENERATOR, G2_INVALID, STRUCTURE = "G0_NOT_GENERATOR", "G2_INVALID", "STRUCTURE"
SQRT_EXP = (Q + 1) // 4  # q = 3 mod 4


class Rejected(Exception):
    def __init__(self, reason, index):
        super().__init__(f"{reason} at {index}")
        self.reason, self.index = reason, index


def decompress_one(b: bytes):
    """32 bytes -> point; raises Rejected(reason, 0).  The kernel's order: the identity flag first
    (every other bit must be zero), then x < q, then the square root."""
    assert len(b) == 32
    v = int.from_bytes(b, "little")
    odd, inf = (v >> 255) & 1, (v >> 254) & 1
    if inf:
        if v != 1 << 254:
            raise Rejected(ENCODING, 0)
        return None
    x = v & ((1 << 254) - 1)
    if x >= Q:
        raise Rejected(NOT_CANONICAL, 0)
    t = (x * x * x + 3) % Q
    y = pow(t, SQRT_EXP, Q)
    if y * y % Q != t:
        raise Rejected(NOT_ON_CURVE, 0)
    if (y & 1) != odd:
        y = (Q - y) % Q
    return (x, y)


def decompress(data: bytes):
    """n x 32 bytes -> list of points; the lowest rejected index wins."""
    assert len(data) % 32 == 0
    out = []
    for i in range(len(data) // 32):
        try:
            out.append(decompress_one(data[32 * i: 32 * i + 32]))
        except Rejected as e:
            raise Rejected(e.reason, i) from None
    return out


def validate_raw(points):
    """points as (x, y) of raw 256-bit integers (what the ABI limbs hold after leaving Montgomery
    form is not defined for x >= q, so the rule is on the stored residues): both < q, not (0, 0),
    on the curve."""
    for i, (x, y) in enumerate(points):
        if x >= Q or y >= Q:
            raise Rejected(NOT_CANONICAL, i)
        if x == 0 and y == 0:
            raise Rejected(IDENTITY, i)
        xc, yc = O.fq_from_mont(x), O.fq_from_mont(y)
        if (yc * yc - xc * xc * xc - 3) % Q:
            raise Rejected(NOT_ON_CURVE, i)


def is_square(t: int) -> bool:
    """Euler's criterion in Fq."""
    return t % Q == 0 or pow(t, (Q - 1) // 2, Q) == 1


def non_residue_x(start: int = 1) -> int:
    """The first x >= start whose x^3 + 3 is no square: no curve point has it."""
    x = start
    while is_square(x * x * x + 3):
        x += 1
    return x


def compress(p, odd=None) -> bytes:
    """pyoracle.g1_compressed, with the parity flag forced when `odd` is given."""
    b = bytearray(O.g1_compressed(p))
    if odd is not None and p is not None:
        b[31] = (b[31] & 0x7F) | (0x80 if odd else 0)
    return bytes(b)


def raw_x(x: int, odd: int = 0, inf: int = 0) -> bytes:
    """An encoding with the given 254-bit x field and flags, valid or not."""
    assert 0 <= x < 1 << 254
    return (x | odd << 255 | inf << 254).to_bytes(32, "little")


# ---- Fq2 square roots and a twist point outside the order-r subgroup -------------------------------
def fq_sqrt(t: int):
    y = pow(t % Q, SQRT_EXP, Q)
    return y if y * y % Q == t % Q else None


def f2_sqrt(a):
    """A square root of a = a0 + a1 u in Fq2 = Fq[u] / (u^2 + 1), or None."""
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        s = fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fq_sqrt(-a0)  # (s u)^2 = -s^2
        return (0, s)
    n = fq_sqrt(a0 * a0 + a1 * a1)
    if n is None:
        return None
    inv2 = pow(2, -1, Q)
    for s in (n, Q - n):
        x0 = fq_sqrt((a0 + s) * inv2)
        if x0:
            x1 = a1 * pow(2 * x0, -1, Q) % Q
            r = (x0, x1)
            if E.f2_mul(r, r) == (a0, a1):
                return r
    return None


def g2_mul_int(p, k: int):
    """[k] p for any integer k >= 0, without the oracle's reduction of k modulo r."""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = E.g2_double(acc)
        if bit == "1":
            acc = E.g2_add(acc, p)
    return acc


def twist_point_outside_subgroup():
    """The first point (x = k, k = 1, 2, ...) of the twist whose order does not divide r: the twist
    has r (2q - r) points, so almost every one."""
    k = 1
    while True:
        x = (k, 0)
        y = f2_sqrt(E.f2_add(E.f2_mul(E.f2_mul(x, x), x), E.B2))
        if y is not None:
            p = (x, y)
            assert E.g2_on_curve(p)
            if g2_mul_int(p, R) is not None:
                return p
        k += 1

