"""LogUp lookups above the device boundary, without a GPU: the symbolic gadget
(plonky3_eon_amd.symbolic.LogUpGadget, lookup/src/logup.rs) against the constraints written out
directly, the degree functions, and the CPU restatement of the lookup branch of prove / verify
(tests/mirror_lookup.py) -- the yardstick of the GPU tests -- which accepts honest proofs and rejects
eon-uni-stark/tests/lookup_air.rs's bad trace and tampered permutation opening."""

import copy
import random

import numpy as np
import pytest

import mirror_lookup as M
from airs import FibonacciAir
from airs_lookup import (LookupMultisetEqAir, RangeCheckAir, multiset_constraints, multiset_permuted_trace,
                         multiset_terms, multiset_trace, range_check_constraints, range_check_preprocessed,
                         range_check_terms, range_check_trace)
from oracle import coracle as C
from oracle import pyoracle as O
from oracle.smallrng import SmallRng, poseidon2_new_from_rng
from plonky3_eon_amd import symbolic as S

P = O.P
SRS_ALPHA = 12345


def evaluate(exprs, env):
    """Numeric value of each SymbolicExpression (iterative, memoised by node)."""
    memo = {}

    def leaf(e):
        if e.op == "const":
            return e.value
        if e.op in ("first", "last", "trans"):
            return env[e.op]
        v = e.var
        if v.entry.kind in ("public", "challenge"):
            return env[v.entry.kind][v.index]
        return env[v.entry.kind][v.entry.offset][v.index]

    for root in exprs:
        stack = [root]
        while stack:
            e = stack[-1]
            if id(e) in memo:
                stack.pop()
                continue
            kids = [k for k in (e.x, e.y) if k is not None]
            todo = [k for k in kids if id(k) not in memo]
            if todo:
                stack.extend(todo)
                continue
            if not kids:
                val = leaf(e)
            elif e.op == "neg":
                val = -memo[id(e.x)]
            else:
                a, b = memo[id(e.x)], memo[id(e.y)]
                val = a + b if e.op == "add" else a - b if e.op == "sub" else a * b
            memo[id(e)] = val % P
            stack.pop()
    return [memo[id(e)] for e in exprs]


def random_env(rng, w, wp, wq, npub):
    r = lambda k: [rng.randrange(P) for _ in range(k)]  # noqa: E731
    return {"main": [r(w), r(w)], "preprocessed": [r(wp), r(wp)], "permutation": [r(wq), r(wq)], "public": r(npub),
            "challenge": r(2 * wq), "first": rng.randrange(P), "last": rng.randrange(P), "trans": rng.randrange(P)}


CASES = [(LookupMultisetEqAir, multiset_constraints, multiset_terms, 2, 0, 1, 0, 0),
         (RangeCheckAir, range_check_constraints, range_check_terms, 3, 1, 2, 1, 1)]


@pytest.mark.parametrize("air_cls,fn,terms,w,wp,wq,npub,own", CASES)
def test_symbolic_logup_equals_the_written_constraints(air_cls, fn, terms, w, wp, wq, npub, own):
    cs, lookups, sym_terms = S.get_symbolic_constraints_and_lookups(air_cls(), wp, npub)
    assert len(lookups) == wq
    assert len(cs) == own + 2 * len(lookups)  # the AIR's own, then two per lookup
    assert S.serialize(cs) == S.serialize(S.get_symbolic_constraints(air_cls(), wp, npub))
    rng = random.Random(5)
    for _ in range(4):
        env = random_env(rng, w, wp, wq, npub)
        sels = (env["first"], env["last"], env["trans"])
        want = fn(env["main"][0], env["main"][1], env["preprocessed"][0], env["preprocessed"][1],
                  env["permutation"][0], env["permutation"][1], sels, env["public"], env["challenge"])
        assert evaluate(cs, env) == want  # value and order
        # the terms handed to the permutation-trace generator, in list order
        direct = terms(env["main"][0], env["main"][1], env["preprocessed"][0], env["preprocessed"][1], env["public"],
                       env["challenge"])
        assert [lk.columns[0] for lk in lookups] == [c for c, _ in direct]
        for tl, (_, dl) in zip(sym_terms, direct):
            assert [tuple(evaluate(list(pair), env)) for pair in tl] == [(d % P, m % P) for d, m in dl]


def test_denominators_are_shared_nodes_of_one_dag():
    cs, lookups, terms = S.get_symbolic_constraints_and_lookups(RangeCheckAir(), 1, 1)
    flat = [e for tl in terms for pair in tl for e in pair]
    nodes_c, _, _ = S.serialize(cs)
    nodes_all, _, roots = S.serialize(list(cs) + flat)
    dens = [d for tl in terms for d, _ in tl]
    extra = len(nodes_all) - len(nodes_c)
    # serialising the terms after the constraints adds no node for any denominator: they are the
    # constraints' own sub-expressions (only multiplicity nodes that the numerators rebuilt may add)
    assert extra <= len(flat) - len(dens)
    assert all(r < len(nodes_c) for r in roots[len(cs)::2])  # every denominator root


def test_degrees():
    assert S.get_log_quotient_degree(LookupMultisetEqAir()) == 1
    assert S.get_max_constraint_degree(LookupMultisetEqAir()) == 3
    assert S.get_max_constraint_degree(RangeCheckAir(), 1, 1) == 3
    assert S.get_log_quotient_degree(RangeCheckAir(), 1, 1) == 1
    gadget = S.LogUpGadget()
    assert (gadget.num_aux_cols, gadget.num_challenges) == (1, 2)
    for air, wp, npub, own in ((LookupMultisetEqAir(), 0, 0, 0), (RangeCheckAir(), 1, 1, 1)):
        cs, lookups, _ = S.get_symbolic_constraints_and_lookups(air, wp, npub)
        for i, lk in enumerate(lookups):
            assert gadget.constraint_degree(lk) == cs[own + 2 * i + 1].degree_multiple


def test_global_lookups_are_refused():
    with pytest.raises(NotImplementedError, match="local"):
        S.get_symbolic_constraints(LookupMultisetEqAir(kind=S.Kind.Global("bus")))


def test_air_without_lookups_is_unchanged():
    cs = S.get_symbolic_constraints(FibonacciAir(), 0, 3)
    b = S.SymbolicAirBuilder(0, 2, 3)
    FibonacciAir().eval(b)
    assert S.serialize(cs) == S.serialize(b.constraints)
    assert S.get_symbolic_constraints_and_lookups(FibonacciAir(), 0, 3)[1:] == ([], [])


def test_direction_and_register_lookup():
    air = LookupMultisetEqAir()
    (lk,) = air.get_lookups()
    assert lk.columns == [0] and lk.kind == S.Kind.Local
    env = random_env(random.Random(1), 2, 0, 1, 0)
    assert evaluate(lk.multiplicities_exprs, env) == [1, P - 1]  # Receive keeps, Send negates
    a, b = RangeCheckAir().get_lookups()
    assert (a.columns, b.columns) == ([1], [0])  # list order and column order differ


def test_traces_satisfy_their_constraints():
    """The generators' traces with the mirror's permutation trace satisfy every constraint on every
    row, and the running sum closes (the wrapped transition on the last row)."""
    rng = random.Random(3)
    for fn, terms, rows, pre, pub, wq in (
            (multiset_constraints, multiset_terms, multiset_permuted_trace(16), None, [], 1),
            (range_check_constraints, range_check_terms, *range_check_trace(16)[:1], range_check_preprocessed(16),
             range_check_trace(16)[1], 2)):
        n = len(rows)
        ch = [rng.randrange(P) for _ in range(2 * wq)]
        perm = M.generate_permutation(terms, rows, pre, pub, ch, wq)
        assert perm[0] == [0] * wq and any(any(r) for r in perm)
        for i in range(n):
            j = (i + 1) % n
            sels = (int(i == 0), int(i == n - 1), int(i != n - 1))
            pl, pn = (pre[i], pre[j]) if pre else ([], [])
            assert not any(fn(rows[i], rows[j], pl, pn, perm[i], perm[j], sels, pub, ch)), i


@pytest.fixture(scope="module")
def py_perm():
    return poseidon2_new_from_rng(SmallRng.seed_from_u64(1), 4, 22)


@pytest.fixture(scope="module")
def srs():
    return C.g1_srs(17, C.fr_from_u64(SRS_ALPHA))


ALL_TRUE = {"transcript": True, "ood": True, "opened_vs_trace": True, "kzg": True}


@pytest.mark.parametrize("rows", [multiset_trace(8), multiset_permuted_trace(16)], ids=["zero8", "permuted16"])
def test_mirror_accepts_its_own_proof(py_perm, srs, rows):
    trace = M.to_limbs(rows)
    log_n = len(rows).bit_length() - 1
    proof = M.prove(trace, None, None, srs, multiset_constraints, multiset_terms, 1, 1,
                    challenger=O.DuplexChallenger(py_perm))
    assert len(proof.opened) == 3 and len(proof.permutation_challenges) == 2
    res, _ = M.verify(proof, None, multiset_constraints, 1, log_n, 1, SRS_ALPHA,
                      challenger=O.DuplexChallenger(py_perm), trace=trace, perm=proof.permutation)
    assert res == ALL_TRUE, res


def test_mirror_rejects_the_bad_trace(py_perm, srs):
    """lookup_air.rs:112: val = 1 on row 0 against an all-zero table.  The proof is well formed
    (transcript and openings hold); the out-of-domain identity fails."""
    trace = M.to_limbs(multiset_trace(8, bad=True))
    proof = M.prove(trace, None, None, srs, multiset_constraints, multiset_terms, 1, 1,
                    challenger=O.DuplexChallenger(py_perm))
    res, _ = M.verify(proof, None, multiset_constraints, 1, 3, 1, SRS_ALPHA, challenger=O.DuplexChallenger(py_perm),
                      trace=trace, perm=proof.permutation)
    assert res == {"transcript": True, "ood": False, "opened_vs_trace": True, "kzg": True}, res


def test_mirror_rejects_a_tampered_permutation_opening(py_perm, srs):
    """lookup_air.rs:169-187: permutation_local[0] += 1."""
    trace = M.to_limbs(multiset_trace(8))
    proof = M.prove(trace, None, None, srs, multiset_constraints, multiset_terms, 1, 1,
                    challenger=O.DuplexChallenger(py_perm))
    bad = copy.deepcopy(proof)
    v = M.ints(bad.opened[1].values[0][0])
    bad.opened[1].values[0][0] = np.stack([M.lim(v[0] + 1)] + [M.lim(x) for x in v[1:]])
    res, _ = M.verify(bad, None, multiset_constraints, 1, 3, 1, SRS_ALPHA, challenger=O.DuplexChallenger(py_perm))
    assert res["transcript"] and not res["ood"] and not res["kzg"], res


def test_mirror_zero_denominator_raises():
    rows = multiset_permuted_trace(8)
    with pytest.raises(M.ZeroDenominator):
        M.generate_permutation(multiset_terms, rows, None, [], [rows[7][0], 5], 1)  # alpha = val of the last row
