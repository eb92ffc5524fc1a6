"""CPU: the verifier's pure host maths (plonky3_eon_amd/host/verify_host.h) -- the Fr inverse, the
canonical add / sub, selectors_at_point (commit/src/domain.rs:237-246) and
recompose_quotient_from_chunks (eon-uni-stark/src/verifier.rs:30-70) -- compiled stand-alone with
the host compiler (tests/verify_host_check.cpp) and compared EXACTLY with
oracle/verify_oracle.py's selectors_at_point and recompose_quotient and with big integers:
log_n in {1, 3, 17}, log_qd in {0, 1, 2}, random zeta plus the edges zeta = 0 and zeta = p - 1,
chunk values random, all 0 and all p - 1."""

import random
import shutil
import subprocess
from pathlib import Path

import pytest

from oracle import pyoracle as O
from oracle import verify_oracle as V

ROOT = Path(__file__).resolve().parents[1]
P = O.P
LOG_NS = (1, 3, 17)
LOG_QDS = (0, 1, 2)


def hx(v: int) -> str:
    return f"{v % P:064x}"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("verifyhost") / "verify_host_check"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", str(ROOT / "include"), "-I",
                    str(ROOT / "plonky3_eon_amd" / "host"), str(ROOT / "tests" / "verify_host_check.cpp"), "-o",
                    str(out)], check=True, capture_output=True)
    return out


def run(exe, tmp_path, lines):
    case_file = tmp_path / "cases.txt"
    case_file.write_text("\n".join(lines) + "\n")
    p = subprocess.run([str(exe), str(case_file)], check=True, capture_output=True, text=True)
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    return [ln.split() for ln in out]


def zetas(rng):
    return [0, P - 1] + [rng.randrange(P) for _ in range(4)]


def test_inverse_add_sub(exe, tmp_path):
    rng = random.Random(11)
    vals = [1, 2, P - 1, P - 2, (P + 1) // 2, 1 << 253] + [rng.randrange(1, P) for _ in range(40)]
    lines = [f"inv {hx(a)}" for a in vals]
    pairs = [(a, b) for a in (0, 1, P - 1) for b in (0, 1, P - 1)] + \
            [(rng.randrange(P), rng.randrange(P)) for _ in range(40)]
    lines += [f"add {hx(a)} {hx(b)}" for a, b in pairs] + [f"sub {hx(a)} {hx(b)}" for a, b in pairs]
    out = run(exe, tmp_path, lines)
    want = [pow(a, -1, P) for a in vals] + [(a + b) % P for a, b in pairs] + [(a - b) % P for a, b in pairs]
    for ln, got, w in zip(lines, out, want):
        assert int(got[1], 16) == w, ln


def test_selectors_at_point(exe, tmp_path):
    rng = random.Random(12)
    cases = [(log_n, z) for log_n in LOG_NS for z in zetas(rng)]
    # the points where the reference panics (inverse of zero): 1, h^-1, another point of the domain
    for log_n in LOG_NS:
        h = O.two_adic_generator(log_n)
        cases += [(log_n, 1), (log_n, pow(h, -1, P)), (log_n, pow(h, (1 << log_n) // 2, P))]
    out = run(exe, tmp_path, [f"sel {log_n} {hx(z)}" for log_n, z in cases])
    defined = 0
    for (log_n, z), got in zip(cases, out):
        try:
            want = V.selectors_at_point(log_n, z)
        except ValueError:  # pow(0, -1, P): the reference's panic
            assert got[1] == "0", (log_n, hex(z))
            continue
        defined += 1
        assert got[1] == "1" and tuple(int(x, 16) for x in got[2:]) == want, (log_n, hex(z))
    assert defined >= len(LOG_NS) * 5  # zeta = 0 and the random ones; p - 1 lies on every domain here


def test_recompose_quotient(exe, tmp_path):
    rng = random.Random(13)
    cases = []
    for log_n in LOG_NS:
        for log_qd in LOG_QDS:
            n = 1 << log_qd
            for z in zetas(rng):
                for chunks in ([rng.randrange(P) for _ in range(n)], [0] * n, [P - 1] * n):
                    cases.append((log_n, log_qd, z, chunks))
    out = run(exe, tmp_path, [f"rec {a} {b} {hx(z)} " + " ".join(hx(c) for c in ch) for a, b, z, ch in cases])
    for (log_n, log_qd, z, chunks), got in zip(cases, out):
        assert int(got[1], 16) == V.recompose_quotient(log_n, log_qd, chunks, z), (log_n, log_qd, hex(z))
