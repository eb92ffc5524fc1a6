"""tests/mirror_pairing.py against the unmerged restatement of the reference's batch check
(oracle/pairing.py verify_batch, kzg/src/util.rs:245-292; no GPU): the merged form gives the same
verdict, the compensating-error and swapped-within-a-point batches are accepted and the
swapped-across-points batch rejected, and the cached Miller values multiply to E.multi_pairing.

The unmerged check costs two Miller loops per opening and a final exponentiation in pure Python,
so it runs on M.CPU_PINNED -- the three parity cases, the doubling in the commitment sum, and the
cases whose merged pairs are at infinity, where the two forms differ most -- and the other small
cases get the table's stated verdict from the merged form alone in tests/test_gpu_pairing_edges.py."""

import pytest

import mirror_pairing as M
from oracle import pairing as E
from oracle import pyoracle as O


def test_case_table_is_complete():
    cases = M.small_cases()
    assert set(cases) == set(M.SMALL_VERDICTS)
    assert set(M.CPU_PINNED) <= set(cases)
    for name, (openings, why) in cases.items():
        assert 1 <= len(openings) <= 4 and why, name
        for c, w, v, z in openings:
            assert O.g1_is_on_curve(c) and O.g1_is_on_curve(w) and 0 <= v < M.R and 0 <= z < M.R, name


@pytest.mark.parametrize("name", M.CPU_PINNED)
def test_merged_verdict_is_the_reference_verdict(name):
    openings, why = M.small_cases()[name]
    want = M.SMALL_VERDICTS[name]
    assert E.verify_batch(openings, E.g2_alpha(M.ALPHA)) is want, why
    assert M.verify_batch_merged(openings, M.ALPHA) is want, why


def test_merged_pairs_shape_and_order():
    """1 + #points pairs, the points in first-seen order, None for infinity."""
    s = M.srs()
    a, d = M.open_poly(s, M.PA, M.Z1), M.open_poly(s, M.PD, M.Z2)
    pairs = M.merged_pairs([d, a, d], M.ALPHA)
    assert len(pairs) == 3 and pairs[0][1] == E.G2_GEN
    assert pairs[1] == (O.g1_neg(O.g1_add(d[1], d[1])), E.g2_mul(E.G2_GEN, M.ALPHA - M.Z2))
    assert pairs[2] == (O.g1_neg(a[1]), E.g2_mul(E.G2_GEN, M.ALPHA - M.Z1))
    # P_0 = sum C - [sum v]G1 = [sum (p_i(alpha) - v_i)]G1
    k = sum(M.quotient(p, M.ALPHA)[1] - M.quotient(p, z)[1] for p, z in ((M.PD, M.Z2), (M.PA, M.Z1), (M.PD, M.Z2)))
    assert pairs[0][0] == O.g1_mul(O.G1_GEN, k % M.R)
    # every pair of a cancelling batch, and Q_z at z = alpha, is infinity
    assert M.merged_pairs([a, M.negate(a)], M.ALPHA)[0][0] is None
    assert M.merged_pairs([a, M.negate(a)], M.ALPHA)[1][0] is None
    at_alpha = M.merged_pairs([M.open_poly(s, M.PA, M.ALPHA)], M.ALPHA)
    assert at_alpha[0] == (None, E.G2_GEN) and at_alpha[1][0] is not None and at_alpha[1][1] is None


def test_progression_openings_are_the_polynomials_openings():
    s = M.srs()
    fam = M.open_progression(s, M.PA, M.PB, M.Z2, 4)
    for i, o in enumerate(fam):
        assert o == M.open_poly(s, [x + i * y for x, y in zip(M.PA, M.PB)], M.Z2), i


def test_cached_miller_prefix_product_is_multi_pairing():
    pairs = [(O.g1_mul(O.G1_GEN, 3 + 2 * i), E.g2_mul(E.G2_GEN, 5 + 3 * i)) for i in range(3)]
    values = [M.miller(p, q) for p, q in pairs]
    hits = M.miller.cache_info().hits
    assert E.final_exponentiation(M.miller_product(values)) == E.multi_pairing(pairs)
    assert M.miller(*pairs[1]) is values[1] and M.miller.cache_info().hits == hits + 1  # computed once
    assert M.miller(None, pairs[0][1]) == E.f12_one() == M.miller(pairs[0][0], None)
