"""The compiled constraint program at the out-of-domain points of n proofs in one launch
(eon_air_eval_at_points_dev, k_air_points; AirProgram.eval_at_points): every pair EXACTLY equal to
AirProgram.eval_at_point on the same inputs, and for n = 3 also to the oracle's fold
(verify_oracle.fold_constraints over the AIR's constraint function), as test_gpu_air_eval_point.py
computes it.  Each proof has its own rows, publics, challenges, alpha, zeta and log_n (alternating 1
and 5); one proof of every batch of three has every cell at the value p - 1."""

import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mirror_check as MC
from airs import FibonacciAir
from airs_lookup import LookupMultisetEqAir, RangeCheckAir, multiset_constraints, range_check_constraints
from airs_preprocessed import MixedPreAir, mixed_pre_constraints
from oracle import coracle as C
from oracle import pyoracle as O
from test_gpu_air_eval_point import ROOT, expected, inputs, lim, rand_ints, run, to_limbs

pytestmark = pytest.mark.gpu
P = O.P
AIRS = ("fibonacci", "mixed_pre", "range_check", "multiset", "poseidon2_vl8")
ROW_NAMES = ("local", "next", "pre_local", "pre_next", "perm_local", "perm_next")


@pytest.fixture(scope="module")
def programs(gpu_ctx):
    """name -> (AirProgram, nine-argument constraint function), compiled once"""
    from plonky3_eon_amd.air import AirProgram, Poseidon2Air

    py = O.p2_constants(2024, 4, 56)
    k = C.P2Constants([[lim(v) for v in r] for r in py[0]], [lim(v) for v in py[1]], [[lim(v) for v in r] for r in py[2]])
    return {"fibonacci": (AirProgram(FibonacciAir(), gpu_ctx), MC.main_fn(O.fib_constraints)),
            "mixed_pre": (AirProgram(MixedPreAir(), gpu_ctx), MC.pre_fn(mixed_pre_constraints)),
            "range_check": (AirProgram(RangeCheckAir(), gpu_ctx), range_check_constraints),
            "multiset": (AirProgram(LookupMultisetEqAir(), gpu_ctx), multiset_constraints),
            "poseidon2_vl8": (AirProgram(Poseidon2Air(k.begin, k.partial, k.end, 8, gpu_ctx), gpu_ctx),
                              MC.p2_fn(O.p2_constraints, py, 8))}


def batch_inputs(prog, n, seed):
    """n input sets (proof 1 of the batch: every cell, public, challenge and alpha the value p - 1),
    their log_n (1, 5, 1, ...) and random zetas"""
    ds = [inputs(prog, "pm1_value" if i == 1 else "random", seed + 13 * i) for i in range(n)]
    log_ns = [(1, 5)[i % 2] for i in range(n)]
    return ds, log_ns, rand_ints(seed + 7, n)


def rows_tensor(ds, pad=0):
    """(n, opened + pad, 4) device tensor: row i = proof i's six rows back to back (then padding)"""
    import torch

    flat = [[v for name in ROW_NAMES for v in d[name]] + [0] * pad for d in ds]
    if not flat[0]:
        return torch.zeros((len(ds), 1, 4), dtype=torch.int64, device="cuda:0")
    return torch.from_numpy(np.ascontiguousarray(to_limbs(flat)).view(np.int64)).to("cuda:0")


def run_many(prog, ds, log_ns, zetas, pad=0):
    return prog.eval_at_points(log_ns, zetas, [d["alpha"] for d in ds], rows_tensor(ds, pad),
                               publics=[d["publics"] for d in ds], challenges=[d["challenges"] for d in ds])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", AIRS)
def test_points_equal_single_calls(programs, name, n):
    prog, fn = programs[name]
    ds, log_ns, zetas = batch_inputs(prog, n, 900 + 31 * AIRS.index(name))
    got = run_many(prog, ds, log_ns, zetas, pad=3 if n == 3 else 0)  # n = 3: a row stride past the opened values
    assert len(got) == n
    for i in range(n):
        assert got[i] == run(prog, ds[i], zetas[i], log_ns[i]), (name, i)
        if n == 3:
            assert got[i] == expected(fn, ds[i], zetas[i], log_ns[i]), (name, i)
    assert got[0][0] != 0  # random inputs satisfy nothing: the fold is a real value
    if n == 3:
        assert len(set(got)) == 3  # each proof its own inputs


@pytest.mark.parametrize("name", ["fibonacci", "range_check"])
def test_65_points(programs, name):
    """More blocks than one proof per anything: every block reads its own rows, table and alpha."""
    prog, _ = programs[name]
    ds, log_ns, zetas = batch_inputs(prog, 65, 4000 + AIRS.index(name))
    got = run_many(prog, ds, log_ns, zetas)
    assert got == [run(prog, ds[i], zetas[i], log_ns[i]) for i in range(65)]
    assert len(set(got)) == 65


def test_no_points(programs):
    import torch

    prog, _ = programs["fibonacci"]
    assert prog.eval_at_points([], [], [], torch.zeros((0, 4, 4), dtype=torch.int64, device="cuda:0")) == []
    out = np.full((2, 4), 77, dtype=np.uint64)
    ctx = prog.ctx
    assert ctx.lib.eon_air_eval_at_points_dev(ctx.handle, prog.handle, 0, None, None, None, None, 0, None, None, 0,
                                              out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert (out == 77).all()


def test_rejections_name_the_point(programs):
    from plonky3_eon_amd import _lib

    def raises(code, words, f):
        with pytest.raises(_lib.EonError) as e:
            f()
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)

    prog, _ = programs["fibonacci"]
    ds, log_ns, zetas = batch_inputs(prog, 3, 77)
    h_inv = pow(O.two_adic_generator(log_ns[1]), -1, P)
    for on_domain in (1, h_inv, pow(O.two_adic_generator(5), 3, P)):
        raises(_lib.EON_E_ARG, ("point 1:", "zeta lies on the trace domain"),
               lambda: run_many(prog, ds, log_ns, [zetas[0], on_domain, zetas[2]]))
    # the same zeta in the single call: the same refusal
    raises(_lib.EON_E_ARG, ("zeta lies on the trace domain",), lambda: run(prog, ds[1], h_inv, log_ns[1]))
    noncanon = np.array([O.int_to_limbs(P)] * len(ds[2]["publics"]), dtype=np.uint64)
    pubs = np.concatenate([to_limbs([d["publics"]])[0] for d in ds[:2]] + [noncanon])
    rows = rows_tensor(ds)
    raises(_lib.EON_E_ARG, ("point 2:", "public value is not a canonical"),
           lambda: prog.eval_at_points(log_ns, zetas, [d["alpha"] for d in ds], rows,
                                       publics=[pubs[3 * i:3 * i + 3] for i in range(3)]))
    raises(_lib.EON_E_SHAPE, ("point 0:", "log_n"), lambda: run_many(prog, ds, [29, 5, 1], zetas))
    # a row stride below the opened values
    raises(_lib.EON_E_SHAPE, ("row_stride",),
           lambda: prog.eval_at_points(log_ns, zetas, [d["alpha"] for d in ds], rows[:, :3].contiguous(),
                                       publics=[d["publics"] for d in ds]))
    rng, _ = programs["range_check"]
    es, lg, zs = batch_inputs(rng, 2, 78)
    raises(_lib.EON_E_SHAPE, ("challenge count",),
           lambda: rng.eval_at_points(lg, zs, [d["alpha"] for d in es], rows_tensor(es),
                                      publics=[d["publics"] for d in es], challenges=[d["challenges"][:3] for d in es]))
    # the context still computes
    assert run_many(prog, ds, log_ns, zetas) == [run(prog, ds[i], zetas[i], log_ns[i]) for i in range(3)]


def test_register_file_global(programs):
    """EON_AIR_REGS=global (read once per process: a child process): block i uses row i of the n
    register rows in global memory, and gives the LDS run's values."""
    code = ("import numpy as np, torch, sys; sys.path[:0] = [sys.argv[2] + '/tests', sys.argv[2]];"
            "from airs_lookup import RangeCheckAir; from plonky3_eon_amd import Context;"
            "from plonky3_eon_amd.air import AirProgram; from oracle import coracle as C;"
            "ctx = Context(0); prog = AirProgram(RangeCheckAir(), ctx);"
            "rows = torch.from_numpy(C.random_fr(11, 36).reshape(3, 12, 4).view(np.int64)).to('cuda:0');"
            "r = prog.eval_at_points([1, 5, 1], [0x1234567, 0x89abcde, 0x777], [0x89abcdef, 5, 6], rows,"
            " publics=[[6], [7], [8]], challenges=[[3, 4, 5, 6], [7, 8, 9, 10], [11, 12, 13, 14]]);"
            "np.save(sys.argv[1], np.array([(v >> (64 * i)) & (2 ** 64 - 1) for p in r for v in p for i in range(4)],"
            " dtype=np.uint64))")
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "global.npy")
        subprocess.run([sys.executable, "-c", code, f, str(ROOT)], check=True, timeout=300,
                       env=dict(os.environ, EON_AIR_REGS="global"))
        out = np.load(f)
    vals = [sum(int(v) << (64 * i) for i, v in enumerate(out[4 * k:4 * k + 4])) for k in range(6)]
    got = [(vals[2 * i], vals[2 * i + 1]) for i in range(3)]
    import torch

    prog, fn = programs["range_check"]
    assert 2 * (prog.width + prog.preprocessed_width + prog.permutation_width) == 12
    rows = torch.from_numpy(C.random_fr(11, 36).reshape(3, 12, 4).view(np.int64)).to("cuda:0")
    lds = prog.eval_at_points([1, 5, 1], [0x1234567, 0x89abcde, 0x777], [0x89abcdef, 5, 6], rows,
                              publics=[[6], [7], [8]], challenges=[[3, 4, 5, 6], [7, 8, 9, 10], [11, 12, 13, 14]])
    assert got == lds
    assert len(set(got)) == 3
