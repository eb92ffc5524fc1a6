"""Test AIRs with LogUp lookups, written against the EonAirBuilder surface and the lookup types of
plonky3_eon_amd.symbolic (``get_lookups`` / ``add_lookup_columns`` / ``register_lookup``), each with

* its constraints written out directly as
  ``fn(local, next, pre_local, pre_next, perm_local, perm_next, sels, publics, challenges)``
  (the assert_zero values in eval order: the AIR's own, then per lookup in list order the first-row
  and the running-sum constraint of logup.rs:154-263), and
* its lookup terms written out directly as ``terms(local, next, pre_local, pre_next, publics,
  challenges)`` -> per lookup in list order (auxiliary column, [(denominator, multiplicity)]),
  what generate_permutation evaluates per row (logup.rs:379-562),

over canonical ints, plus trace generators."""

import random

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def logup_constraints(col, terms, ploc, pnxt, first):
    """logup.rs:97-142, 224, 261 for one lookup: [first * s_local,
    (s_next - s_local) * prod(d) - sum_i m_i prod_{j != i} d_j]."""
    den = 1
    for d, _ in terms:
        den = den * d % P
    num = 0
    for i, (_, m) in enumerate(terms):
        others = 1
        for j, (d, _) in enumerate(terms):
            if j != i:
                others = others * d % P
        num = (num + m * others) % P
    return [first * ploc[col] % P, ((pnxt[col] - ploc[col]) * den - num) % P]


def fold(elements, beta):
    """logup.rs:84-86: acc -> elt + acc * beta from 0."""
    acc = 0
    for e in elements:
        acc = (e + acc * beta) % P
    return acc


class LookupMultisetEqAir:
    """eon-uni-stark/tests/lookup_air.rs:18-72: main (val, table), no constraints of its own, one
    local lookup +table -val, so multiset(table) == multiset(val)."""

    def __init__(self, kind=None):
        self.next_lookup_col = 0
        self.kind = kind

    def width(self):
        return 2

    def num_public_values(self):
        return 0

    def eval(self, builder):
        pass

    def add_lookup_columns(self):
        col = self.next_lookup_col
        self.next_lookup_col += 1
        return [col]

    def get_lookups(self):
        from plonky3_eon_amd.symbolic import Direction, Entry, Kind, SymbolicVariable, register_lookup

        self.next_lookup_col = 0
        val = SymbolicVariable(Entry("main", 0), 0)
        table = SymbolicVariable(Entry("main", 0), 1)
        inputs = [([table], 1, Direction.RECEIVE), ([val], 1, Direction.SEND)]
        return [register_lookup(self, self.kind or Kind.Local, inputs)]


def multiset_terms(loc, nxt, ploc, pnxt, pub, ch):
    alpha, beta = ch[0], ch[1]
    return [(0, [((alpha - fold([loc[1]], beta)) % P, 1), ((alpha - fold([loc[0]], beta)) % P, P - 1)])]


def multiset_constraints(loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch):
    (col, terms), = multiset_terms(loc, nxt, ploc, pnxt, pub, ch)
    return logup_constraints(col, terms, mloc, mnxt, sels[0])


def multiset_trace(n, bad=False):
    """generate_trace_rows (lookup_air.rs:98-117): all zero; `bad`: val = 1 on row 0."""
    return [[1 if bad and i == 0 else 0, 0] for i in range(n)]


def multiset_permuted_trace(n, seed=7):
    """table: n distinct values; val: a random permutation of them."""
    rng = random.Random(seed)
    table = rng.sample(range(1, 1 << 60), n)
    val = list(table)
    rng.shuffle(val)
    return [[val[i], table[i]] for i in range(n)]


class RangeCheckAir:
    """Preprocessed table column t = 0 .. n-1; main (v, m, x) with x = (v + 1) mod n and one public
    value: when_first_row x == public[0].  Two local lookups:

    * A: [t] with multiplicity m (Receive) against [v] with 1 (Send): every v is in the table;
    * B: [t, t_next, t + t_next] with m (Receive) against [v, x, v + x] with 1 (Send): (v, x) is a
      row of the table and its cyclic successor -- three-element tuples (beta's Horner fold), a
      next-row cell, the wrap at the last row.

    B is registered first and A second, and get_lookups returns [A, B]: list order and auxiliary
    column order differ (A has column 1, B column 0)."""

    def __init__(self):
        self.next_lookup_col = 0

    def width(self):
        return 3

    def preprocessed_width(self):
        return 1

    def num_public_values(self):
        return 1

    def eval(self, builder):
        loc = builder.main()[0]
        (x0,) = builder.public_values()
        builder.when_first_row().assert_eq(loc[2], x0)

    def add_lookup_columns(self):
        col = self.next_lookup_col
        self.next_lookup_col += 1
        return [col]

    def get_lookups(self):
        from plonky3_eon_amd.symbolic import Direction, Entry, Kind, SymbolicVariable, register_lookup

        self.next_lookup_col = 0
        v, m, x = (SymbolicVariable(Entry("main", 0), i) for i in range(3))
        t = SymbolicVariable(Entry("preprocessed", 0), 0)
        tn = SymbolicVariable(Entry("preprocessed", 1), 0)
        b = register_lookup(self, Kind.Local, [([t, tn, t + tn], m, Direction.RECEIVE),
                                               ([v, x, v + x], 1, Direction.SEND)])
        a = register_lookup(self, Kind.Local, [([t], m, Direction.RECEIVE), ([v], 1, Direction.SEND)])
        return [a, b]


def range_check_terms(loc, nxt, ploc, pnxt, pub, ch):
    v, m, x = loc
    t, tn = ploc[0], pnxt[0]
    a_alpha, a_beta = ch[2], ch[3]  # A: auxiliary column 1
    b_alpha, b_beta = ch[0], ch[1]  # B: auxiliary column 0
    a = [((a_alpha - fold([t], a_beta)) % P, m), ((a_alpha - fold([v], a_beta)) % P, P - 1)]
    b = [((b_alpha - fold([t, tn, (t + tn) % P], b_beta)) % P, m),
         ((b_alpha - fold([v, x, (v + x) % P], b_beta)) % P, P - 1)]
    return [(1, a), (0, b)]


def range_check_constraints(loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch):
    out = [sels[0] * (loc[2] - pub[0]) % P]
    for col, terms in range_check_terms(loc, nxt, ploc, pnxt, pub, ch):
        out += logup_constraints(col, terms, mloc, mnxt, sels[0])
    return out


def range_check_preprocessed(n):
    return [[i] for i in range(n)]


def range_check_trace(n, seed=11):
    """-> (rows, publics): v random in [0, n), m[i] = #{j: v[j] == i}, x = (v + 1) mod n."""
    rng = random.Random(seed)
    v = [rng.randrange(n) for _ in range(n)]
    rows = [[v[i], sum(1 for u in v if u == i), (v[i] + 1) % n] for i in range(n)]
    return rows, [rows[0][2]]


class LookupMockAir:
    """MockAir (symbolic_builder.rs:308-354) over the three matrices and the challenges: one
    assert_zero per (kind, offset, index), kind "main", "pre", "perm" or "challenge"."""

    def __init__(self, specs, width, preprocessed_width, permutation_width):
        self.specs = specs
        self._w, self._wp, self._wq = width, preprocessed_width, permutation_width

    def width(self):
        return self._w

    def preprocessed_width(self):
        return self._wp

    def permutation_width(self):
        return self._wq

    def num_public_values(self):
        return 0

    def eval(self, builder):
        mats = {"main": builder.main(), "pre": builder.preprocessed(),
                "perm": builder.permutation() if self._wq else None}
        for kind, offset, index in self.specs:
            if kind == "challenge":
                builder.assert_zero(builder.permutation_randomness()[index])
            else:
                builder.assert_zero(mats[kind][offset][index])

    def constraints(self, loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch):
        rows = {("main", 0): loc, ("main", 1): nxt, ("pre", 0): ploc, ("pre", 1): pnxt, ("perm", 0): mloc,
                ("perm", 1): mnxt}
        return [ch[index] if kind == "challenge" else rows[(kind, offset)][index]
                for kind, offset, index in self.specs]
