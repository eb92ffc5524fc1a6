"""TEST-ONLY mirror of the merged form of the KZG batch check (csrc/pairing.hip) over plain Python
integers, on oracle/pairing.py (E) and oracle/pyoracle.py (O), with the ABI layouts and the case
builders of tests/test_gpu_pairing*.py.

The reference's verify_batch (kzg/src/util.rs:245-292) tests
    prod_i e(C_i - v_i G1, G2) e(-W_i, [alpha]G2 - z_i G2) == 1
with 2n Miller loops.  Pairs that share their G2 argument merge by bilinearity, so the same
element of Gt is
    e(sum_i C_i - (sum_i v_i) G1, G2) * prod_z e(-sum_{i: z_i = z} W_i, [alpha - z]G2)
over the distinct points z: 1 + #points Miller loops.  `merged_pairs` states those pairs and
`verify_batch_merged` their verdict; tests/test_pairing_mirror_cpu.py pins the verdict to
E.verify_batch, the unmerged restatement.

Points are the oracles': G1 (x, y) canonical ints, G2 ((x0, x1), (y0, y1)), None = infinity.
An opening is (commitment, witness, value, point)."""

from functools import lru_cache

import numpy as np

from oracle import pairing as E
from oracle import pyoracle as O

R = O.P  # the group order


# ---- ABI layouts (include/eon.h; plonky3_eon_amd/verify.py) --------------------------------------
def g1_limbs(p):
    if p is None:
        return np.zeros(8, dtype=np.uint64)
    return np.array(O.int_to_limbs(O.fq_to_mont(p[0])) + O.int_to_limbs(O.fq_to_mont(p[1])), dtype=np.uint64)


def g2_limbs(q):
    if q is None:
        return np.zeros(16, dtype=np.uint64)
    (x0, x1), (y0, y1) = q
    out = []
    for v in (x0, x1, y0, y1):
        out += O.int_to_limbs(O.fq_to_mont(v))
    return np.array(out, dtype=np.uint64)


def fr_limbs(x):
    return np.array(O.int_to_limbs(O.to_mont(x % O.P)), dtype=np.uint64)


def gt_limbs(f):
    """oracle Fq12 (w-basis, w^12 = 18 w^6 - 82) -> the tower layout of eon_fq12: the coefficient
    of w^k (k = 2j + i) is a + b u with u = w^6 - 9, i.e. flat[k] = a - 9 b, flat[k + 6] = b."""
    out = np.zeros((12, 4), dtype=np.uint64)
    for i in range(2):
        for j in range(3):
            k = 2 * j + i
            b = f[k + 6] % O.Q
            a = (f[k] + 9 * b) % O.Q
            m = 3 * i + j
            out[2 * m] = O.int_to_limbs(O.fq_to_mont(a))
            out[2 * m + 1] = O.int_to_limbs(O.fq_to_mont(b))
    return out


def opening_arrays(openings):
    """[(C, W, v, z)] -> the four arrays verify.verify_batch takes."""
    if not openings:
        return [np.zeros((0, 8), np.uint64), np.zeros((0, 8), np.uint64), np.zeros((0, 4), np.uint64),
                np.zeros((0, 4), np.uint64)]
    return [np.stack([g1_limbs(c) for c, _, _, _ in openings]), np.stack([g1_limbs(w) for _, w, _, _ in openings]),
            np.stack([fr_limbs(v) for _, _, v, _ in openings]), np.stack([fr_limbs(z) for _, _, _, z in openings])]


# ---- cached Miller values ------------------------------------------------------------------------
@lru_cache(maxsize=None)
def miller(p, q):
    """The Miller value of one pair as E.multi_pairing forms it, computed once per (P, Q)."""
    return E.miller_loop(E.twist(q), E.cast_g1(p))


def miller_product(values):
    f = E.f12_one()
    for v in values:
        f = E.f12_mul(f, v)
    return f


def multi_pairing(pairs):
    """E.multi_pairing(pairs) -- the same product and final exponentiation -- over cached Miller
    values (pinned to E.multi_pairing in tests/test_pairing_mirror_cpu.py)."""
    return E.final_exponentiation(miller_product(miller(p, q) for p, q in pairs))


# ---- the merged form -----------------------------------------------------------------------------
@lru_cache(maxsize=None)
def g2_of(k):
    return E.g2_mul(E.G2_GEN, k % R)


def merged_pairs(openings, alpha):
    """[(sum C - [sum v]G1, G2)] + [(-sum_{z_i = z} W_i, [alpha - z]G2) for each distinct z], the
    distinct z in first-seen order (pairing.hip's grouping), None for infinity."""
    sum_c, sum_v = None, 0
    order, sum_w = [], {}
    for c, w, v, z in openings:
        sum_c = O.g1_add(sum_c, c)
        sum_v = (sum_v + v) % R
        z %= R
        if z not in sum_w:
            order.append(z)
            sum_w[z] = None
        sum_w[z] = O.g1_add(sum_w[z], w)
    pairs = [(O.g1_add(sum_c, O.g1_neg(O.g1_mul(O.G1_GEN, sum_v))), E.G2_GEN)]
    return pairs + [(O.g1_neg(sum_w[z]), g2_of(alpha - z)) for z in order]


def verify_batch_merged(openings, alpha):
    """The reference's verdict on a batch: by bilinearity its product of 2n pairings is the product
    of the merged pairs."""
    return multi_pairing(merged_pairs(openings, alpha)) == E.f12_one()


# ---- builders of valid openings ------------------------------------------------------------------
def quotient(coeffs, z):
    """quotient_and_eval (kzg/src/util.rs:100-111) over ints: (p(x) - p(z)) / (x - z) and p(z)."""
    n = len(coeffs)
    q = [0] * (n - 1)
    carry = coeffs[-1] % R
    for i in range(n - 2, -1, -1):
        q[i] = carry
        carry = (coeffs[i] + carry * z) % R
    return q, carry


def open_poly(srs, coeffs, z):
    """The valid opening of the polynomial with these coefficients (low degree first) at z."""
    q, v = quotient(coeffs, z)
    return (O.commit_column(srs, [c % R for c in coeffs]), O.commit_column(srs, q), v, z % R)


def open_progression(srs, p0, d, z, n):
    """The valid openings at z of p_i = p0 + i d, i < n: commitments, witnesses and values each
    advance by one point or field addition (commit and quotient are linear)."""
    c, w, v, _ = open_poly(srs, p0, z)
    dc, dw, dv, _ = open_poly(srs, d, z)
    out = []
    for _ in range(n):
        out.append((c, w, v, z % R))
        c, w, v = O.g1_add(c, dc), O.g1_add(w, dw), (v + dv) % R
    return out


def open_constant(c, z):
    """The constant polynomial c: C = [c]G1, the quotient is zero, W = infinity."""
    return (O.g1_mul(O.G1_GEN, c), None, c % R, z % R)


def negate(opening):
    """The opening of -p: (-C, -W, -v, z)."""
    c, w, v, z = opening
    return (O.g1_neg(c), O.g1_neg(w), (-v) % R, z)


def with_value(opening, v):
    return (opening[0], opening[1], v % R, opening[3])


def with_witness(opening, w):
    return (opening[0], w, opening[2], opening[3])


# ---- the small verify_batch cases (n <= 4) of tests/test_gpu_pairing_edges.py --------------------
ALPHA = 0x5EED0A1FA
Z1, Z2 = 5, 11
PA, PB, PD = [3, 1, 4, 1], [2, 7, 1, 8], [5, 0, 9, 2]
POINT_EDGES = {"0": 0, "1": 1, "r-1": R - 1, "2^253": 1 << 253, "alpha": ALPHA}


@lru_cache(maxsize=None)
def srs():
    """init_srs_unsafe's g1_powers for ALPHA, 8 powers."""
    return tuple(O.init_srs_g1(7, ALPHA))


def _eval(coeffs, z):
    return quotient(coeffs, z)[1]


@lru_cache(maxsize=None)
def small_cases():
    """name -> (openings, why the reference's verdict follows).  The verdict itself is
    verify_batch_merged's; tests/test_pairing_mirror_cpu.py pins CPU_PINNED of them to E.verify_batch."""
    s = srs()
    a, b, d = open_poly(s, PA, Z1), open_poly(s, PB, Z1), open_poly(s, PD, Z2)
    cases = {}
    # identical openings: sum C = [2]C, sum W = [2]W, sum v = 2v
    cases["identical-2"] = ([a, a], "a valid opening twice: every factor of the product appears squared")
    cases["identical-2-v+1"] = ([with_value(a, a[2] + 1)] * 2, "sum v is off by 2: P_0 = -[2]G1, the product is e(G1, G2)^-2")
    # p and -p at one point: every merged pair is infinity and sum v = 0
    cases["cancel"] = ([a, negate(a)], "valid openings of p and -p: sum C = sum W = infinity, sum v = 0")
    cases["cancel-v+1"] = ([a, with_value(negate(a), 1 - a[2])], "sum v = 1: P_0 = -G1 against an infinite witness sum")
    # point edges
    for name, z in POINT_EDGES.items():
        o = open_poly(s, PA, z)
        why = "p(alpha) = v makes C - vG1 infinity while [alpha - z]G2 is infinity" if name == "alpha" else "a valid opening"
        cases[f"z={name}"] = ([o], why)
        why = ("C - (v+1)G1 = -G1 pairs with G2 and nothing cancels it (Q_z is infinity)" if name == "alpha"
               else "the value is off by one")
        cases[f"z={name}-v+1"] = ([with_value(o, o[2] + 1)], why)
    # value edges
    root = [(-2 * Z1) % R, (2 - Z1) % R, 1]  # (x - Z1)(x + 2)
    cases["v=0"] = ([open_poly(s, root, Z1)], "a root of the polynomial: sum v = 0, P_0 = C")
    cases["v=0-tampered"] = ([with_value(open_poly(s, root, Z1), 1)], "value 1 at a root")
    top = [(PA[0] - _eval(PA, Z1) - 1) % R] + PA[1:]  # PA shifted so that its value at Z1 is -1
    cases["v=r-1"] = ([open_poly(s, top, Z1)], "a valid opening whose value is r - 1")
    cases["v=r-1-tampered"] = ([with_value(open_poly(s, top, Z1), 0)], "value r - 1 + 1 = 0 instead of r - 1")
    opp = [(PD[0] - _eval(PD, Z2) - a[2]) % R] + PD[1:]  # PD shifted so that its value at Z2 is -PA(Z1)
    cases["v0+v1=0"] = ([a, open_poly(s, opp, Z2)], "two valid openings whose non-zero values sum to 0: [sum v]G1 is infinity")
    cases["v0+v1=0-tampered"] = ([a, with_value(open_poly(s, opp, Z2), 1 - a[2])], "sum v = 1 instead of 0")
    # constant and zero polynomials: W = infinity
    cases["const-1"] = ([open_constant(9, Z1)], "C = [9]G1, v = 9: both pairs are infinity")
    cases["const-1-tampered"] = ([with_value(open_constant(9, Z1), 10)], "C - 10 G1 = -G1")
    cases["const-2"] = ([open_constant(9, Z1), open_constant(12, Z2)], "sum C = [21]G1 = [sum v]G1, no witnesses")
    cases["const-2-tampered"] = ([open_constant(9, Z1), with_value(open_constant(12, Z2), 13)], "sum v = 22 against [21]G1")
    cases["zero"] = ([(None, None, 0, Z1)], "the zero polynomial: every point and value is zero")
    cases["zero-v=1"] = ([(None, None, 1, Z1)], "P_0 = -G1 against an infinite witness")
    # the unrandomised product accepts errors that cancel in it (kzg/src/util.rs:245-292)
    cases["compensating"] = ([with_value(a, a[2] + 1), with_value(d, d[2] - 1)],
                             "v_0 + 1 and v_1 - 1 at two points: only sum v enters the product, and it is unchanged")
    cases["swapped-within"] = ([with_witness(a, b[1]), with_witness(b, a[1])],
                               "two witnesses of one point swapped: both pair with the same [alpha - z]G2, "
                               "so the product is that of the valid batch")
    cases["swapped-across"] = ([with_witness(a, d[1]), with_witness(d, a[1])],
                               "witnesses of different points swapped: W_a now pairs with [alpha - z_d]G2")
    return cases


# The verdict each case's reason gives (the tests parametrise over these names, and assert that the
# mirror and the GPU both return it).  True: the reference's Ok(()); False: its ProofShapeMismatch.
SMALL_VERDICTS = {
    "identical-2": True, "identical-2-v+1": False, "cancel": True, "cancel-v+1": False,
    **{f"z={name}": True for name in POINT_EDGES}, **{f"z={name}-v+1": False for name in POINT_EDGES},
    "v=0": True, "v=0-tampered": False, "v=r-1": True, "v=r-1-tampered": False,
    "v0+v1=0": True, "v0+v1=0-tampered": False,
    "const-1": True, "const-1-tampered": False, "const-2": True, "const-2-tampered": False,
    "zero": True, "zero-v=1": False,
    "compensating": True, "swapped-within": True, "swapped-across": False,
}

# the cases the CPU test runs through the unmerged E.verify_batch as well (about 0.14 s per
# non-infinite pair and 0.15 s per final exponentiation there)
CPU_PINNED = ("compensating", "swapped-within", "swapped-across", "identical-2", "cancel", "z=alpha", "z=alpha-v+1",
              "const-2", "zero", "zero-v=1")
