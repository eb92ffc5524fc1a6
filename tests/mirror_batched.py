"""TEST-ONLY restatement of the batched KZG opening (EON_OPENING_BATCHED) with Python integers.

The product folds a matrix's columns with powers of gamma (eon_fr_fold_columns_dev), opens the
folded polynomial once per point (KzgPcs::open_batched) and verifies the claims weighted by powers
of delta (eon_verify_air[_fs]).  Here the same three steps are plain arithmetic modulo r:

* ``fold``                   -- out[i] = scale * sum_j gamma^j mat[i][j]
* ``quotient_and_eval``      -- kzg/src/util.rs:100-111 by synthetic division
* ``open_batched_coeffs``    -- values and witnesses of coefficient matrices; a witness is kept as
                                its discrete logarithm q(s) with respect to G1 (the test SRS's
                                trapdoor s is known: commit_column(q) = [q(s)] G1), ``point`` makes
                                the affine point
* ``open_batched_evals``     -- the same from a matrix's EVALUATIONS on the trace domain: with
                                F = sum_j gamma^j f_j the witness at z is [(F(s) - F(z)) / (s - z)] G1,
                                both values barycentric -- no coefficients needed
* ``claims_of`` / ``verify`` -- the K claims of a proof in claim order and the check
                                sum_i delta^i (sum_j gamma^j C_(m,j) - v_i G1 - (s - z_i) W_i) == 0,
                                the pairing product with the pairing replaced by the trapdoor;
                                delta = 1 is the UNWEIGHTED product of the per-column mode
* ``transcript_tail``        -- what prover and verifier append to the transcript after zeta
"""

from __future__ import annotations

import numpy as np

from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V

P = O.P
_TWO_ADIC_GENERATOR = pow(5, (P - 1) >> 28, P)  # bn254/src/field.rs:556-561: 5^((r-1)/2^28)


def two_adic_generator(bits: int) -> int:
    """bn254/src/field.rs:563-574: the generator of the subgroup of order 2^bits"""
    return pow(_TWO_ADIC_GENERATOR, 1 << (28 - bits), P)


def fold(rows, gamma: int, scale: int = 1):
    """rows: a list of rows of canonical ints -> one int per row"""
    out = []
    for row in rows:
        acc, g = 0, 1
        for x in row:
            acc = (acc + g * x) % P
            g = g * gamma % P
        out.append(acc * scale % P)
    return out


def quotient_and_eval(coeffs, z: int):
    """(the n - 1 quotient coefficients of f by (X - z), f(z)): r_i = c_i + z r_(i+1), q_i = r_(i+1)"""
    if not coeffs:
        return [], 0
    q = [0] * (len(coeffs) - 1)
    r = 0
    for i in range(len(coeffs) - 1, -1, -1):
        if i < len(coeffs) - 1:
            q[i] = r
        r = (coeffs[i] + z * r) % P
    return q, r


def commit_dlog(coeffs, srs_alpha: int) -> int:
    """the discrete logarithm of commit_column(coeffs) over the SRS [s^i] G1: f(s)"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * srs_alpha + c) % P
    return acc


def point(dlog: int) -> np.ndarray:
    """[dlog] G1 as an ABI row (8 u64; the identity is all zero)"""
    return C.g1_mul(C.g1_generator(), V.fr_limbs(dlog))


def open_batched_coeffs(mats, points, gamma: int, srs_alpha: int):
    """mats[m]: rows x width coefficient ints; points[m]: the matrix's points ->
    (values[m][p][j], witness_dlog[m][p])"""
    values, wits = [], []
    for mat, pts in zip(mats, points):
        width = len(mat[0]) if mat else 0
        cols = [[row[j] for row in mat] for j in range(width)]
        folded = fold(mat, gamma)
        values.append([[quotient_and_eval(c, z)[1] for c in cols] for z in pts])
        wits.append([commit_dlog(quotient_and_eval(folded, z)[0], srs_alpha) for z in pts])
    return values, wits


def bary_eval_columns(evals, log_n: int, x: int):
    """f_j(x) of every column from its evaluations on the subgroup of size 2^log_n (shift 1, natural
    order), x off the subgroup: (x^n - 1) / n * sum_i e_i w^i / (x - w^i)"""
    n = 1 << log_n
    assert len(evals) == n
    w = two_adic_generator(log_n)
    weights, wi = [], 1
    for _ in range(n):
        weights.append(wi * pow((x - wi) % P, -1, P) % P)
        wi = wi * w % P
    scale = (pow(x, n, P) - 1) * pow(n, -1, P) % P
    width = len(evals[0])
    return [scale * sum(weights[i] * evals[i][j] for i in range(n)) % P for j in range(width)]


def open_batched_evals(evals, log_n: int, points, gamma: int, srs_alpha: int):
    """one matrix given by its evaluations on the trace domain -> (values[p][j], witness_dlog[p])"""
    at_s = bary_eval_columns(evals, log_n, srs_alpha)
    f_s = fold([at_s], gamma)[0]
    values, wits = [], []
    for z in points:
        v = bary_eval_columns(evals, log_n, z)
        values.append(v)
        wits.append((f_s - fold([v], gamma)[0]) * pow((srs_alpha - z) % P, -1, P) % P)
    return values, wits


def rows8(a):
    return np.asarray(a, dtype=np.uint64).reshape(-1, 8)


def ints4(a):
    return [V.fr_int(r) for r in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def claims_of(proof, log_n: int, vk_commit=None):
    """The claims (commit_rows (w, 8), values [w ints], witness_row (8,), z) of a batched proof in
    claim order: trace zeta, trace zeta h; [permutation zeta, zeta h]; chunk 0..C-1 at zeta;
    [preprocessed zeta, zeta h] -- the preprocessed commitment is the verifier key's."""
    zeta = proof.zeta
    zeta_next = zeta * two_adic_generator(log_n) % P
    has_perm = proof.permutation_commit is not None
    opened = list(proof.opened)
    out = []

    def matrix(commit, op):
        for p, z in enumerate((zeta, zeta_next)):
            out.append((rows8(commit), ints4(op.values[0][p]), rows8(op.witnesses[0][p])[0], z))

    matrix(proof.trace_commit[0], opened[0])
    if has_perm:
        matrix(proof.permutation_commit[0], opened[1])
    quot = opened[2 if has_perm else 1]
    for c, commit in enumerate(proof.quotient_commit):
        out.append((rows8(commit), ints4(quot.values[c][0]), rows8(quot.witnesses[c][0])[0], zeta))
    if len(opened) > (3 if has_perm else 2):
        matrix(vk_commit if vk_commit is not None else proof.preprocessed_commit[0], opened[-1])
    return out


def verify(claims, gamma: int, delta: int, srs_alpha: int) -> bool:
    """sum_i delta^i (sum_j gamma^j C_(m,j) - [sum_j gamma^j v_(i,j)] G1 - (s - z_i) W_i) is the
    identity: one CPU MSM over the proof's own points.  delta = 1: the unweighted product."""
    idx, pts, sc = {}, [], []

    def add(row, k):
        row = np.ascontiguousarray(row, dtype=np.uint64).reshape(8)
        key = row.tobytes()
        if key not in idx:
            idx[key] = len(pts)
            pts.append(row)
            sc.append(0)
        sc[idx[key]] = (sc[idx[key]] + k) % P

    g_coef, d = 0, 1
    for commit, values, wit, z in claims:
        g = d
        for crow, v in zip(commit, values):
            add(crow, g)
            g_coef -= g * v
            g = g * gamma % P
        add(wit, -d * (srs_alpha - z))
        d = d * delta % P
    add(C.g1_generator(), g_coef)
    out = C.g1_msm(np.stack(pts), np.stack([V.fr_limbs(s) for s in sc]))
    return not np.any(out)


def transcript_tail(challenger, claims):
    """after zeta: every opened value in claim order, column by column; gamma; the K witnesses in
    claim order; delta.  `challenger` is a pyoracle.DuplexChallenger -> (gamma, delta)."""
    for _, values, _, _ in claims:
        for v in values:
            challenger.observe(v)
    gamma = challenger.sample()
    for _, _, wit, _ in claims:
        challenger.observe_g1([O.g1_from_bytes(np.ascontiguousarray(wit, dtype=np.uint64).tobytes())])
    delta = challenger.sample()
    return gamma, delta
