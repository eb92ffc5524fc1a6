"""CPU: bench.py's launch logic (no GPU call happens on these paths)."""

import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _run(args, **env):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env)
    return subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                          timeout=120, env=e)


def test_world_size_mismatch_is_an_error():
    out = _run(["--gpus", "4"], WORLD_SIZE="1")
    assert out.returncode == 2 and "WORLD_SIZE=1" in out.stderr
    assert out.stdout.strip() == ""


def test_zero_gpus_rejected():
    out = _run(["--gpus", "0"])
    assert out.returncode == 2


def test_self_launch_builds_the_launcher_command(monkeypatch):
    sys.path.insert(0, str(ROOT))
    import bench

    seen = {}

    def fake_call(cmd):
        seen["cmd"] = cmd
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.main() == 7  # the launcher's status is the exit status
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "8", "--steps", "2"]


def test_collective_choice():
    """The N > 1 prove uses the driver's RCCL communicator by default, torch.distributed when the
    ranks share a device or the backend is gloo, and whatever --collective names."""
    import bench

    assert bench.choose_collective("auto", {}) == "rccl"
    assert bench.choose_collective("auto", {"EON_BENCH_BACKEND": "nccl"}) == "rccl"
    assert bench.choose_collective("auto", {"EON_BENCH_ONE_DEVICE": "1"}) == "torch"
    assert bench.choose_collective("auto", {"EON_BENCH_BACKEND": "gloo"}) == "torch"
    assert bench.choose_collective("torch", {}) == "torch"
    assert bench.choose_collective("rccl", {"EON_BENCH_ONE_DEVICE": "1"}) == "rccl"
    args = bench.make_parser().parse_args([])
    assert args.collective == "auto" and not args.no_clock_probe


def test_dump_outputs_exact_and_bounded(tmp_path):
    """--dump-outputs: 64-bit words survive as exact float64 halves, an array above its share of the
    limit is cut to the same seeded row sample every time, and the files stay within 64 MB."""
    import numpy as np

    import bench

    rng = np.random.Generator(np.random.PCG64(1))
    small = rng.integers(0, 2**64, size=(5, 4), dtype=np.uint64)
    rows = bench.DUMP_LIMIT_BYTES // 2 // (16 * 4) + 1000  # just above a two-array share
    big = rng.integers(0, 2**64, size=(rows, 4), dtype=np.uint64)
    shapes = bench.dump_outputs({"small": small, "big": big}, tmp_path / "a")
    bench.dump_outputs({"small": small, "big": big}, tmp_path / "b")
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and s.shape == (5, 8) == tuple(shapes["small"])
    np.testing.assert_array_equal(s.astype(np.uint32).view(np.uint64), small)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (rows - 1000, 8)
    np.testing.assert_array_equal(a, b)
    back = a.astype(np.uint32).view(np.uint64)
    idx = np.flatnonzero((big[:, None, 0] == back[:10, 0]).any(axis=1))  # the sample is rows of `big`, in order
    assert len(idx) == 10 and (np.diff(idx) > 0).all()
    np.testing.assert_array_equal(big[idx], back[:10])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 * 1000 * 1000
