"""The column-sharded prove of a generic AIR over a process group (eon_prove_air_sharded[_fs],
prove_native(AirProgram, ..., collective=)): gloo ranks sharing cuda:0, each running
tests/_shard_worker.py, where every rank compares its sharded proof with the unsharded prove of the
full trace -- Proof.to_bytes() and the challenges, once with given alpha / zeta and once with a
challenger.  Without the feature every multi-rank case ends in the old "not lane-sharded" refusal."""

import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import pytest

from _launch import _heartbeat, free_port

pytestmark = pytest.mark.gpu
WORKER = Path(__file__).resolve().parent / "_shard_worker.py"
MAX_RANKS = 8


def run_shard_world(mode: str, world: int, timeout: int):
    """_launch.run_world for _shard_worker.py: one process per rank, killed at the timeout"""
    assert 1 <= world <= MAX_RANKS
    port = free_port()
    with tempfile.TemporaryDirectory() as d:
        procs, outs, logs = [], [], []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="2")
            out = Path(d) / f"rank{r}.json"
            outs.append(out)
            log = open(Path(d) / f"rank{r}.log", "wb")
            logs.append(log)
            procs.append(subprocess.Popen([sys.executable, str(WORKER), mode, str(out)], env=env, stdout=log,
                                          stderr=subprocess.STDOUT))
        t0 = last = time.monotonic()
        try:
            while any(p.poll() is None for p in procs):
                now = time.monotonic()
                if now - t0 > timeout:
                    break
                if now - last >= 20:
                    _heartbeat(f"run_shard_world {mode} x{world}: {now - t0:.0f} s, "
                               f"{sum(p.poll() is None for p in procs)} ranks running")
                    last = now
                time.sleep(0.2)
        finally:
            hung = [r for r, p in enumerate(procs) if p.poll() is None]
            for p in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()
            for f in logs:
                f.close()
        res = []
        for r, out in enumerate(outs):
            if not out.exists():
                text = (Path(d) / f"rank{r}.log").read_bytes().decode(errors="replace")
                what = "was still running at the timeout" if r in hung else f"wrote no verdict (rc {procs[r].returncode})"
                res.append({"ok": False, "why": f"rank {r} {what}:\n{text[-3000:]}"})
            else:
                res.append(json.loads(out.read_text()))
        return res


def check(mode, world):
    res = run_shard_world(mode, world, timeout=600)
    assert all(r["ok"] for r in res), [r["why"] for r in res if not r["ok"]]


@pytest.mark.parametrize("world", [2, 3])
def test_mixed_air(world):
    """W = 5: widths 3, 2 and 2, 2, 1; 8 quotient chunks over the ranks; Q = 128, S = 8: with three
    ranks R = 43, the last block short"""
    check("mixed", world)


@pytest.mark.parametrize("world", [3, 7])
def test_mul_air(world):
    """W = 60, 2 chunks: with three ranks rank 2 commits no chunk, with seven ranks 2 .. 6 do not
    and the widths are 9, 9, 9, 9, 8, 8, 8"""
    check("mul", world)


def test_fibonacci_verifies():
    """W = 2 over two ranks, one column each, no quotient split (log_qd 0: S = 1); the sharded
    Fiat-Shamir proof of the valid trace is accepted by verify_native"""
    check("fib", 2)


def test_more_ranks_than_columns():
    """FibonacciAir over three ranks: every rank raises the same error and none waits for another"""
    check("fib_too_many", 3)


def test_keccak_air():
    """the workload the feature is for: W = 2633 (odd: 1317 + 1316) at the 32 rows
    tests/test_gpu_keccak.py proves at"""
    check("keccak", 2)


def test_what_stays_unsharded_is_refused():
    """preprocessed columns, lookups, check_constraints, the batched opening and a trace of another
    width each raise with their reason, on every rank, and the group proves afterwards"""
    check("refuse", 2)
