"""The compiled constraint program at one out-of-domain point (eon_air_eval_at_point_dev,
k_air_point; AirProgram.eval_at_point): both outputs EXACTLY equal to
verify_oracle.fold_constraints(constraint_fn(local, next, selectors_at_point(zeta)), alpha) and to
that value times inv_vanishing, for inputs that need not come from a proof.

The per-AIR constraint functions are the ones the mirrors and verify_oracle already use.  Input
kinds: random canonical Fr; every cell, public value, challenge and alpha the VALUE p - 1; and the
same with the stored Montgomery RESIDUE p - 1 (all limbs at their maximum: the interpreter's lazy
bounds).  zeta stays random there: p - 1 lies on every trace domain used."""

import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import mirror_check as MC
import mirror_lookup as ML
from airs import FibonacciAir, MockAir, MulAir
from airs_lookup import LookupMultisetEqAir, RangeCheckAir, multiset_constraints, range_check_constraints
from airs_preprocessed import MixedPreAir, mixed_pre_constraints
from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V
from test_gpu_air_program import mul_constraints

pytestmark = pytest.mark.gpu
P = O.P
ROOT = Path(__file__).resolve().parent.parent
ints, lim, to_limbs = ML.ints, ML.lim, ML.to_limbs
PM1_RESIDUE = O.from_mont(P - 1)  # the canonical int whose stored residue is p - 1
LOG_NS = (1, 5)
KINDS = ("random", "pm1_value", "pm1_residue")


def dev(row):
    """canonical ints -> (len, 4) device tensor of Montgomery limbs"""
    import torch

    return torch.from_numpy(np.ascontiguousarray(to_limbs([row])[0]).view(np.int64)).to("cuda:0")


def rand_ints(seed, n):
    return [int(x) for x in ints(C.random_fr(seed, n))] if n else []


@pytest.fixture(scope="module")
def p2_consts():
    py = O.p2_constants(2024, 4, 56)
    k = C.P2Constants([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]])
    return py, k


@pytest.fixture(scope="module")
def programs(gpu_ctx, p2_consts):
    """name -> (AirProgram, nine-argument constraint function), compiled once"""
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air

    py, k = p2_consts
    out = {"fibonacci": (AirProgram(FibonacciAir(), gpu_ctx), MC.main_fn(O.fib_constraints)),
           "mul": (AirProgram(MulAir(), gpu_ctx), MC.main_fn(mul_constraints)),
           "mixed_pre": (AirProgram(MixedPreAir(), gpu_ctx), MC.pre_fn(mixed_pre_constraints)),
           "range_check": (AirProgram(RangeCheckAir(), gpu_ctx), range_check_constraints),
           "multiset": (AirProgram(LookupMultisetEqAir(), gpu_ctx), multiset_constraints)}
    for vl in (1, 8):
        out[f"poseidon2_vl{vl}"] = (AirProgram(Poseidon2Air(k.begin, k.partial, k.end, vl, gpu_ctx), gpu_ctx),
                                    MC.p2_fn(O.p2_constraints, py, vl))
    return out


def inputs(prog, kind, seed):
    """-> dict of canonical-int inputs: the six rows, publics, challenges, alpha"""
    sizes = [prog.width, prog.width, prog.preprocessed_width, prog.preprocessed_width, prog.permutation_width,
             prog.permutation_width, prog.n_public, prog.num_challenges, 1]
    if kind == "random":
        flat = rand_ints(seed, sum(sizes))
    else:
        flat = [P - 1 if kind == "pm1_value" else PM1_RESIDUE] * sum(sizes)
    parts, at = [], 0
    for s in sizes:
        parts.append(flat[at:at + s])
        at += s
    names = ("local", "next", "pre_local", "pre_next", "perm_local", "perm_next", "publics", "challenges")
    d = dict(zip(names, parts[:8]))
    d["alpha"] = parts[8][0]
    return d


def expected(fn, d, zeta, log_n):
    sels = V.selectors_at_point(log_n, zeta)
    cs = fn(d["local"], d["next"], d["pre_local"], d["pre_next"], d["perm_local"], d["perm_next"], sels[:3],
            d["publics"], d["challenges"])
    folded = V.fold_constraints(cs, d["alpha"])
    return folded, folded * sels[3] % P


def run(prog, d, zeta, log_n):
    opt = lambda row: dev(row) if row else None  # noqa: E731
    return prog.eval_at_point(log_n, zeta, d["alpha"], dev(d["local"]), dev(d["next"]), d["publics"],
                              preprocessed_local=opt(d["pre_local"]), preprocessed_next=opt(d["pre_next"]),
                              permutation_local=opt(d["perm_local"]), permutation_next=opt(d["perm_next"]),
                              challenges=d["challenges"])


AIRS = ("fibonacci", "mul", "mixed_pre", "range_check", "multiset", "poseidon2_vl1", "poseidon2_vl8")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", AIRS)
def test_eval_at_point_vs_oracle(programs, name, kind):
    prog, fn = programs[name]
    if name == "mul":
        assert prog.width == 60 and prog.max_constraint_degree == 3
    if name == "poseidon2_vl8":  # the large-register-file case
        assert prog.num_constraints == 1280
    d = inputs(prog, kind, 100 + AIRS.index(name))
    for log_n in LOG_NS:
        zeta = rand_ints(500 + 7 * AIRS.index(name) + log_n, 1)[0]
        want = expected(fn, d, zeta, log_n)
        got = run(prog, d, zeta, log_n)
        print(f"{name} {kind} log_n={log_n}: folded {got[0]:#x} quotient side {got[1]:#x}")
        assert got == want, (name, kind, log_n)
    if kind == "random":
        assert want[0] != 0  # the inputs satisfy nothing: the fold is a real value


def test_zeta_edges(programs):
    """zeta = 0 (Z_H = -1) and a zeta next to the forbidden points are ordinary points."""
    prog, fn = programs["fibonacci"]
    d = inputs(prog, "random", 31)
    for log_n in LOG_NS:
        h_inv = pow(O.two_adic_generator(log_n), -1, P)
        for zeta in (0, 2, (h_inv + 1) % P, P - 2):
            assert run(prog, d, zeta, log_n) == expected(fn, d, zeta, log_n), (log_n, hex(zeta))


def test_register_file_global(programs):
    """EON_AIR_REGS=global (read once per process: a child process) gives the LDS run's values, which
    are the oracle's."""
    code = ("import numpy as np, torch, sys; sys.path[:0] = [sys.argv[2] + '/tests', sys.argv[2]];"
            "from airs_lookup import RangeCheckAir; from plonky3_eon_amd import Context;"
            "from plonky3_eon_amd.air import AirProgram; from oracle import coracle as C;"
            "ctx = Context(0); prog = AirProgram(RangeCheckAir(), ctx);"
            "t = lambda s, w: torch.from_numpy(C.random_fr(s, w).reshape(w, 4).view(np.int64)).to('cuda:0');"
            "r = prog.eval_at_point(5, 0x1234567, 0x89abcdef, t(1, 3), t(2, 3), [6], preprocessed_local=t(3, 1),"
            " preprocessed_next=t(4, 1), permutation_local=t(5, 2), permutation_next=t(6, 2), challenges=[3, 4, 5, 6]);"
            "np.save(sys.argv[1], np.array([(v >> (64 * i)) & (2 ** 64 - 1) for v in r for i in range(4)],"
            " dtype=np.uint64))")
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "global.npy")
        subprocess.run([sys.executable, "-c", code, f, str(ROOT)], check=True, timeout=300,
                       env=dict(os.environ, EON_AIR_REGS="global"))
        out = np.load(f)
    got = tuple(sum(int(v) << (64 * i) for i, v in enumerate(out[4 * k:4 * k + 4])) for k in range(2))
    rows = [ints(C.random_fr(s, w).reshape(w, 4)) for s, w in ((1, 3), (2, 3), (3, 1), (4, 1), (5, 2), (6, 2))]
    d = dict(zip(("local", "next", "pre_local", "pre_next", "perm_local", "perm_next"), rows),
             publics=[6], challenges=[3, 4, 5, 6], alpha=0x89abcdef)
    prog, fn = programs["range_check"]
    assert got == expected(fn, d, 0x1234567, 5)
    assert got == run(prog, d, 0x1234567, 5)


def test_rejections(gpu_ctx, programs):
    import ctypes

    from plonky3_eon_amd import Context, _lib

    def raises(code, word, f):
        with pytest.raises(_lib.EonError) as e:
            f()
        assert e.value.code == code and word in str(e.value), str(e.value)

    fib, _ = programs["fibonacci"]
    d = inputs(fib, "random", 41)
    for log_n in LOG_NS:
        h = O.two_adic_generator(log_n)
        raises(_lib.EON_E_ARG, "zeta lies on the trace domain", lambda: run(fib, d, 1, log_n))
        raises(_lib.EON_E_ARG, "zeta lies on the trace domain", lambda: run(fib, d, pow(h, -1, P), log_n))
    raises(_lib.EON_E_ARG, "zeta lies on the trace domain", lambda: run(fib, d, pow(O.two_adic_generator(5), 3, P), 5))
    raises(_lib.EON_E_SHAPE, "public value count", lambda: run(fib, dict(d, publics=d["publics"][:2]), 7, 3))
    noncanon = np.array([O.int_to_limbs(P)] * 3, dtype=np.uint64)
    raises(_lib.EON_E_ARG, "public value is not a canonical", lambda: run(fib, dict(d, publics=noncanon), 7, 3))
    rng, _ = programs["range_check"]
    e = inputs(rng, "random", 42)
    raises(_lib.EON_E_ARG, "pre_local and pre_next must not be null", lambda: run(rng, dict(e, pre_next=[]), 7, 3))
    raises(_lib.EON_E_ARG, "perm_local and perm_next must not be null", lambda: run(rng, dict(e, perm_local=[]), 7, 3))
    raises(_lib.EON_E_SHAPE, "challenge count", lambda: run(rng, dict(e, challenges=e["challenges"][:3]), 7, 3))
    # through the C ABI: rows the program does not read, a program of another context, a non-canonical zeta
    loc, nxt, out = dev(d["local"]), dev(d["next"]), np.zeros((2, 4), np.uint64)
    pub = to_limbs([d["publics"]])[0]

    def raw(ctx, zeta_limbs, pre=None, perm=None):
        z = np.array(zeta_limbs, dtype=np.uint64)
        a = lim(5)
        rc = ctx.lib.eon_air_eval_at_point_dev(ctx.handle, fib.handle, 3, z.ctypes.data_as(ctypes.c_void_p),
                                               a.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(loc.data_ptr()),
                                               ctypes.c_void_p(nxt.data_ptr()), pre, pre, perm, perm,
                                               pub.ctypes.data_as(ctypes.c_void_p), 3, None, 0,
                                               out.ctypes.data_as(ctypes.c_void_p))
        return rc, ctx.lib.eon_last_error(ctx.handle)

    assert raw(gpu_ctx, lim(7))[0] == _lib.EON_OK
    rc, msg = raw(gpu_ctx, lim(7), pre=ctypes.c_void_p(loc.data_ptr()))
    assert rc == _lib.EON_E_ARG and b"pre_local and pre_next must be null" in msg
    rc, msg = raw(gpu_ctx, lim(7), perm=ctypes.c_void_p(loc.data_ptr()))
    assert rc == _lib.EON_E_ARG and b"perm_local and perm_next must be null" in msg
    rc, msg = raw(Context(0), lim(7))
    assert rc == _lib.EON_E_ARG and b"another context" in msg
    rc, msg = raw(gpu_ctx, O.int_to_limbs(P))
    assert rc == _lib.EON_E_ARG and b"zeta is not a canonical" in msg


def test_zero_constraints(gpu_ctx):
    from plonky3_eon_amd.air import AirProgram

    empty = AirProgram(MockAir([], 2), gpu_ctx)
    assert empty.num_constraints == 0
    assert empty.eval_at_point(3, 12345, 678, dev(rand_ints(1, 2)), dev(rand_ints(2, 2))) == (0, 0)
