"""Preprocessed columns above the device boundary, without a GPU: the symbolic layer emits the
EON_SYM_PREPROCESSED leaves the device program reads, and the CPU restatement of the
Some(preprocessed) prove / verify (tests/mirror_preprocessed.py) -- the yardstick of the GPU tests --
accepts its own honest proof and rejects mul_fib_pair.rs's tampered preprocessed trace."""

import pytest

import mirror_preprocessed as M
from airs_preprocessed import (MixedPreAir, MulFibPAir, mixed_pre_constraints, mixed_pre_preprocessed,
                               mixed_pre_trace, mul_fib_p_constraints, mul_fib_p_preprocessed, mul_fib_p_trace)
from oracle import coracle as C
from oracle import pyoracle as O
from oracle.smallrng import SmallRng, poseidon2_new_from_rng
from plonky3_eon_amd import symbolic as S

SRS_ALPHA = 12345


def test_mul_fib_pair_serialises_preprocessed_leaves():
    cs = S.get_symbolic_constraints(MulFibPAir(), preprocessed_width=2)
    assert len(cs) == 2
    nodes, consts, roots = S.serialize(cs)
    pre = sorted({(a, b) for kind, a, b in nodes if kind == S.SYM_PREPROCESSED})
    assert pre == [(0, 0), (1, 0)]  # prod_coeff and sum_coeff of the local row
    main = sorted({(a, b) for kind, a, b in nodes if kind == S.SYM_MAIN})
    assert main == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert max(c.degree_multiple for c in cs) == 3
    assert S.get_max_constraint_degree(MulFibPAir(), 2) == 3
    assert S.get_log_quotient_degree(MulFibPAir(), 2) == 1


def test_mixed_pre_air_serialises_both_rows_and_two_quotient_bits():
    cs = S.get_symbolic_constraints(MixedPreAir(), preprocessed_width=3)
    nodes, _, roots = S.serialize(cs)
    pre = sorted({(a, b) for kind, a, b in nodes if kind == S.SYM_PREPROCESSED})
    assert pre == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
    assert len(roots) == 7
    # two constraints are bare preprocessed leaves
    assert [nodes[r] for r in roots[4:6]] == [(S.SYM_PREPROCESSED, 1, 0), (S.SYM_PREPROCESSED, 1, 1)]
    assert S.get_max_constraint_degree(MixedPreAir(), 3) == 4
    assert S.get_log_quotient_degree(MixedPreAir(), 3) == 2


@pytest.fixture(scope="module")
def py_perm():
    return poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)


@pytest.fixture(scope="module")
def srs():
    return C.g1_srs(9, C.fr_from_u64(SRS_ALPHA))


def test_mirror_accepts_its_own_mul_fib_pair_proof(py_perm, srs):
    n = 8
    trace = M.to_limbs(mul_fib_p_trace(0, 1, n))
    pre = M.to_limbs(mul_fib_p_preprocessed(n))
    pp = M.setup(pre, srs)
    proof = M.prove(trace, pp, srs, mul_fib_p_constraints, 1, challenger=O.DuplexChallenger(py_perm))
    res = M.verify(proof, pp.commitment, 2, mul_fib_p_constraints, 3, 1, SRS_ALPHA,
                   challenger=O.DuplexChallenger(py_perm), trace=trace, pre=pre)
    assert res == {"transcript": True, "ood": True, "opened_vs_trace": True, "kzg": True}, res


def test_mirror_rejects_tampered_preprocessed(py_perm, srs):
    """mul_fib_pair.rs's tamper test: the preprocessed trace committed at setup differs at row 3
    from the one the trace was generated with."""
    n = 8
    trace = M.to_limbs(mul_fib_p_trace(0, 1, n))
    pre = M.to_limbs(mul_fib_p_preprocessed(n, tamper_index=3))
    pp = M.setup(pre, srs)
    proof = M.prove(trace, pp, srs, mul_fib_p_constraints, 1, challenger=O.DuplexChallenger(py_perm))
    res = M.verify(proof, pp.commitment, 2, mul_fib_p_constraints, 3, 1, SRS_ALPHA,
                   challenger=O.DuplexChallenger(py_perm), trace=trace, pre=pre)
    assert res == {"transcript": True, "ood": False, "opened_vs_trace": True, "kzg": True}, res


def test_mirror_binds_the_setup_commitment(py_perm, srs):
    """An honest proof replayed against another setup's commitment: the transcript differs."""
    n = 8
    trace = M.to_limbs(mul_fib_p_trace(0, 1, n))
    pp = M.setup(M.to_limbs(mul_fib_p_preprocessed(n)), srs)
    other = M.setup(M.to_limbs(mul_fib_p_preprocessed(n, tamper_index=5)), srs)
    proof = M.prove(trace, pp, srs, mul_fib_p_constraints, 1, challenger=O.DuplexChallenger(py_perm))
    res = M.verify(proof, other.commitment, 2, mul_fib_p_constraints, 3, 1, SRS_ALPHA,
                   challenger=O.DuplexChallenger(py_perm))
    assert res["transcript"] is False


def test_mixed_pre_trace_satisfies_its_constraints():
    """The MixedPreAir generator's trace is satisfying on every row (selectors of the trace domain:
    first / last row indicators, transition off on the last row)."""
    n = 16
    rows, pub = mixed_pre_trace(3, 4, 5, n)
    pre = mixed_pre_preprocessed(n)
    for i in range(n):
        sels = (int(i == 0), int(i == n - 1), int(i != n - 1))
        j = (i + 1) % n
        assert not any(mixed_pre_constraints(rows[i], rows[j], pre[i], pre[j], sels, pub)), i
    bad = mixed_pre_preprocessed(n, tamper_index=3)
    assert any(mixed_pre_constraints(rows[3], rows[4], bad[3], bad[4], (0, 0, 1), pub))
