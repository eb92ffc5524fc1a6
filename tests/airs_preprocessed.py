"""Test AIRs with preprocessed columns, written against the EonAirBuilder surface
(plonky3_eon_amd.symbolic: ``builder.preprocessed()`` is the PairBuilder window), each with its
constraints written out directly as ``fn(local, next, pre_local, pre_next, sels, publics)`` (the
assert_zero values in eval order, sels = (is_first_row, is_last_row, is_transition)) and its trace
generators (canonical ints)."""

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


class MulFibPAir:
    """uni-stark/tests/mul_fib_pair.rs:55-81: main (a, b), preprocessed (prod_coeff, sum_coeff);
    when_transition: b == next.a and prod_coeff a b + sum_coeff (a + b) == next.b."""

    def width(self):
        return 2

    def preprocessed_width(self):
        return 2

    def num_public_values(self):
        return 0

    def eval(self, builder):
        main = builder.main()
        prep = builder.preprocessed()[0]
        local, nxt = main[0], main[1]
        when_transition = builder.when_transition()
        when_transition.assert_eq(local[1], nxt[0])  # a' <- b
        prod_term = prep[0] * local[0] * local[1]
        sum_term = prep[1] * (local[0] + local[1])
        when_transition.assert_eq(prod_term + sum_term, nxt[1])  # b' <- prod a b + sum (a + b)


def mul_fib_p_constraints(loc, nxt, ploc, pnxt, sels, pub):
    trans = sels[2]
    return [trans * (loc[1] - nxt[0]) % P,
            trans * (ploc[0] * loc[0] * loc[1] + ploc[1] * (loc[0] + loc[1]) - nxt[1]) % P]


def mul_fib_p_preprocessed(n, tamper_index=None):
    """generate_preprocessed_trace (mul_fib_pair.rs:104-128): prod_coeff = i % 2, sum_coeff =
    (i + 1) % 6; the tampered row's prod_coeff is one more."""
    rows = [[i % 2, (i + 1) % 6] for i in range(n)]
    if tamper_index is not None and tamper_index < n:
        rows[tamper_index][0] += 1
    return rows


def mul_fib_p_trace(a, b, n):
    """generate_trace_rows (mul_fib_pair.rs:83-102), from the untampered preprocessed trace."""
    prep = mul_fib_p_preprocessed(n)
    rows = [[a % P, b % P]]
    for i in range(1, n):
        pa, pb = rows[-1]
        rows.append([pb, (prep[i - 1][0] * pa * pb + prep[i - 1][1] * (pa + pb)) % P])
    return rows


class MixedPreAir:
    """Main (m0, m1, m2), preprocessed (p0, p1, p2), one public x; degree 4 (two quotient bits).
    Reads the preprocessed local and next rows, the first and last preprocessed column next to the
    last main column (in a shared sub-expression), a preprocessed cell times a selector minus a
    public value, and a preprocessed cell as a bare constraint (p1 is the zero column)."""

    def width(self):
        return 3

    def preprocessed_width(self):
        return 3

    def num_public_values(self):
        return 1

    def eval(self, builder):
        m = builder.main()
        pre = builder.preprocessed()
        loc, nxt, p, pn = m[0], m[1], pre[0], pre[1]
        (x,) = builder.public_values()
        s = p[0] * loc[2] + p[2]  # shared below
        builder.when_transition().assert_eq(nxt[0], s * s)
        builder.assert_zero(builder.is_first_row() * p[2] - builder.is_first_row() * x)
        builder.when_transition().assert_eq(nxt[1], loc[1] + pn[0])
        builder.when_transition().assert_eq(nxt[2], loc[2] + pn[2] * loc[1])
        builder.assert_zero(p[1])  # constraints that are leaves
        builder.assert_zero(pn[1])
        builder.when_last_row().assert_eq(loc[0] * p[0], s * p[0] - (s - loc[0]) * p[0])


def mixed_pre_constraints(loc, nxt, ploc, pnxt, sels, pub):
    first, last, trans = sels
    s = (ploc[0] * loc[2] + ploc[2]) % P
    return [trans * (nxt[0] - s * s) % P, (first * ploc[2] - first * pub[0]) % P,
            trans * (nxt[1] - (loc[1] + pnxt[0])) % P, trans * (nxt[2] - (loc[2] + pnxt[2] * loc[1])) % P,
            ploc[1], pnxt[1], last * (loc[0] * ploc[0] - (s * ploc[0] - (s - loc[0]) * ploc[0])) % P]


def mixed_pre_preprocessed(n, tamper_index=None):
    rows = [[(i * i + 3) % 7 + 1, 0, (5 * i + 2) % 11] for i in range(n)]
    if tamper_index is not None and tamper_index < n:
        rows[tamper_index][0] += 1
    return rows


def mixed_pre_trace(a, b, c, n):
    """A satisfying trace for the untampered preprocessed columns; the public value is p2[0]."""
    prep = mixed_pre_preprocessed(n)
    rows = [[a % P, b % P, c % P]]
    for i in range(1, n):
        m0, m1, m2 = rows[-1]
        s = (prep[i - 1][0] * m2 + prep[i - 1][2]) % P
        rows.append([s * s % P, (m1 + prep[i][0]) % P, (m2 + prep[i][2] * m1) % P])
    return rows, [prep[0][2]]


class PreMockAir:
    """MockAir (symbolic_builder.rs:308-354) over both matrices: one assert_zero per
    (matrix, offset, index), matrix "main" or "pre"."""

    def __init__(self, specs, width, preprocessed_width):
        self.specs = specs
        self._w = width
        self._wp = preprocessed_width

    def width(self):
        return self._w

    def preprocessed_width(self):
        return self._wp

    def num_public_values(self):
        return 0

    def eval(self, builder):
        mats = {"main": builder.main(), "pre": builder.preprocessed()}
        for matrix, offset, index in self.specs:
            builder.assert_zero(mats[matrix][offset][index])

    def constraints(self, loc, nxt, ploc, pnxt, sels, pub):
        rows = {("main", 0): loc, ("main", 1): nxt, ("pre", 0): ploc, ("pre", 1): pnxt}
        return [rows[(matrix, offset)][index] for matrix, offset, index in self.specs]
