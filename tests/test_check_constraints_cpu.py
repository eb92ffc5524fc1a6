"""The CPU mirror of check_constraints (tests/mirror_check.py) on the reference's own test data
(eon-uni-stark/src/check_constraints.rs:308-422): RowLogicAir, two columns, next[0] = local[0] + 1
on transitions and the last row equal to the two public values.  No GPU."""

import pytest

import mirror_check as MC
from test_symbolic import eval_serialized

P = MC.P


@pytest.mark.parametrize("name,rows,publics,first", MC.ROW_LOGIC_CASES, ids=[c[0] for c in MC.ROW_LOGIC_CASES])
def test_row_logic_cases(name, rows, publics, first):
    """test_incremental_rows_with_last_row_check and test_single_row_wraparound_logic pass;
    test_incorrect_increment_logic fails on the transition out of row 1 (constraint 0);
    test_wrong_last_row_public_value on the last row's second public value (constraint 2)."""
    fails = MC.check_constraints(MC.main_fn(MC.row_logic_constraints), rows, publics=publics)
    s = MC.summary(fails, 3)
    if first is None:
        assert fails == [] and s == {"failures": 0, "row": 0, "constraint": 0, "value": 0, "failing_constraints": 0,
                                     "counts": [0, 0, 0]}
        return
    assert (s["row"], s["constraint"]) == first and s["failures"] == 1 and s["failing_constraints"] == 1
    assert s["counts"] == [1 if k == first[1] else 0 for k in range(3)]
    # the values: row 2 holds 5 where 3 was due; the public value is 5 where the cell holds 4
    assert s["value"] == {(1, 0): 5 - 3, (3, 2): (4 - 5) % P}[first]


def test_selectors_and_wraparound():
    """Row selectors are 1 / 0 on the trace domain and the last row's next is row 0: a constraint
    gated by nothing sees the wrap, a transition-gated one does not."""
    seen = []

    def fn(loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch):
        seen.append((loc[0], nxt[0], sels))
        return [nxt[0] - loc[0] - 1, sels[2] * (nxt[0] - loc[0] - 1)]

    fails = MC.check_constraints(fn, [[5], [6], [7], [8]])
    assert seen == [(5, 6, (1, 0, 1)), (6, 7, (0, 0, 1)), (7, 8, (0, 0, 1)), (8, 5, (0, 1, 0))]
    assert fails == [(3, 0, (5 - 8 - 1) % P)]
    assert MC.check_constraints(fn, [[5], [6], [7], [8]], only_rows=[1, 2]) == []


def test_three_matrices_and_challenges_reach_the_function():
    def fn(loc, nxt, ploc, pnxt, mloc, mnxt, sels, pub, ch):
        return [loc[0] - ploc[0], nxt[0] - pnxt[0], mloc[0] - ch[0], mnxt[0] - pub[0]]

    rows, pre, perm = [[1], [2]], [[1], [2]], [[9], [4]]
    fails = MC.check_constraints(fn, rows, pre, perm, publics=[4], challenges=[9])
    assert fails == [(1, 2, (4 - 9) % P), (1, 3, 9 - 4)]
    s = MC.summary(fails, 4)
    assert (s["failures"], s["row"], s["constraint"], s["failing_constraints"]) == (2, 1, 2, 2)
    assert s["counts"] == [0, 0, 1, 1]


def test_row_logic_air_is_the_written_out_function():
    """RowLogicAir on the symbolic builder (what the device program is compiled from) evaluates to
    row_logic_constraints, constraint for constraint."""
    from plonky3_eon_amd import symbolic as S

    nodes, consts, roots = S.serialize(S.get_symbolic_constraints(MC.RowLogicAir()))
    for loc, nxt, sels, pub in [([1, 4], [2, 3], (1, 0, 1), [4, 1]), ([4, 4], [1, 1], (0, 1, 0), [4, 5]),
                                ([2, 2], [5, 5], (0, 0, 1), [6, 6]), ([99, 77], [99, 77], (1, 1, 0), [99, 77])]:
        assert eval_serialized(nodes, consts, roots, loc, nxt, sels, pub) == MC.row_logic_constraints(loc, nxt, sels, pub)
