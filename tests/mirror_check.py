"""CPU restatement of check_constraints (eon-uni-stark/src/check_constraints.rs:22-101): every
trace row with local = row i, next = row (i + 1) mod height of the main, preprocessed and
permutation trace, the row selectors as the field elements 1 / 0 (:88-90), every assert_zero value
in eval order.  TEST INFRASTRUCTURE ONLY.

An AIR is its constraints written out directly over canonical ints,
``fn(local, next, pre_local, pre_next, perm_local, perm_next, sels, publics, challenges)`` (the
shape of tests/airs_lookup.py); ``main_fn`` / ``pre_fn`` / ``p2_fn`` adapt the one-matrix functions
(pyoracle.fib_constraints, ...), the two-matrix ones (tests/airs_preprocessed.py) and the
Poseidon2-AIR's.  The reference panics at the first failure; ``check_constraints`` returns all of
them, from which ``summary`` takes that first failure, its value, the total and the per-constraint
counts -- what eon_check_constraints_dev reports."""

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def main_fn(fn):
    """fn(local, next, sels, publics) -> the nine-argument shape"""
    return lambda loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch: fn(loc, nxt, sels, pub)


def pre_fn(fn):
    """fn(local, next, pre_local, pre_next, sels, publics) -> the nine-argument shape"""
    return lambda loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch: fn(loc, nxt, ploc, pnxt, sels, pub)


def p2_fn(p2_constraints, consts, vector_len):
    """the (vectorized) Poseidon2-AIR: pyoracle.p2_constraints lane after lane (vectorized.rs:259-274)"""

    def fn(loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch):
        nc = len(loc) // vector_len
        out = []
        for v in range(vector_len):
            out += p2_constraints(list(loc[v * nc:(v + 1) * nc]), consts)
        return out

    return fn


def check_constraints(fn, rows, pre_rows=None, perm_rows=None, publics=(), challenges=(), only_rows=None):
    """-> the full failure set [(row, constraint, value)], ordered by row, then constraint: the
    first entry is the reference's panic.  `only_rows`: evaluate just these rows (a large trace
    known to be valid elsewhere)."""
    n = len(rows)
    out = []
    for i in (range(n) if only_rows is None else sorted(only_rows)):
        j = (i + 1) % n  # :42
        sels = (1 if i == 0 else 0, 1 if i == n - 1 else 0, 1 if i != n - 1 else 0)  # :88-90
        cs = fn(list(rows[i]), list(rows[j]),
                list(pre_rows[i]) if pre_rows is not None else [], list(pre_rows[j]) if pre_rows is not None else [],
                list(perm_rows[i]) if perm_rows is not None else [], list(perm_rows[j]) if perm_rows is not None else [],
                sels, list(publics), list(challenges))
        out += [(i, k, c % P) for k, c in enumerate(cs) if c % P]
    return out


def summary(failures, num_constraints):
    """-> what the device reports: failures, row, constraint, value (zero without a failure),
    failing_constraints and the per-constraint counts"""
    counts = [0] * num_constraints
    for _, k, _ in failures:
        counts[k] += 1
    row, k, value = failures[0] if failures else (0, 0, 0)
    return {"failures": len(failures), "row": row, "constraint": k, "value": value,
            "failing_constraints": sum(1 for c in counts if c), "counts": counts}


class RowLogicAir:
    """RowLogicAir of the reference's own check_constraints tests (check_constraints.rs:235-281,
    without the aux columns): two main columns, two public values; when_transition: next[0] =
    local[0] + 1; when_last_row: local[0] = pv0 and local[1] = pv1."""

    def width(self):
        return 2

    def num_public_values(self):
        return 2

    def eval(self, builder):
        m = builder.main()
        loc, nxt = m[0], m[1]
        pv0, pv1 = builder.public_values()
        builder.when_transition().assert_eq(nxt[0], loc[0] + 1)
        when_last = builder.when_last_row()
        when_last.assert_eq(loc[0], pv0)
        when_last.assert_eq(loc[1], pv1)


def row_logic_constraints(loc, nxt, sels, pub):
    _, last, trans = sels
    return [trans * (nxt[0] - (loc[0] + 1)) % P, last * (loc[0] - pub[0]) % P, last * (loc[1] - pub[1]) % P]


# the data of check_constraints.rs:308-422: (name, rows, publics, first failure (row, constraint) or None)
ROW_LOGIC_CASES = [
    ("incremental_rows_with_last_row_check", [[1, 4], [2, 3], [3, 2], [4, 1]], [4, 1], None),
    ("incorrect_increment_logic", [[1, 1], [2, 2], [5, 5], [6, 6]], [6, 6], (1, 0)),
    ("wrong_last_row_public_value", [[1, 1], [2, 2], [3, 3], [4, 4]], [4, 5], (3, 2)),
    ("single_row_wraparound_logic", [[99, 77]], [99, 77], None),
]
