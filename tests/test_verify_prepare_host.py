"""CPU: the verifier's prepare phase (plonky3_eon_amd/host/verify_prepare.*) is device-free code --
it builds with the host compiler from two translation units and no library of the project -- and is
safe to run on several threads, as verify_many does: tests/verify_prepare_check.cpp runs prepare
over 8 synthetic proofs with 1 and with 8 threads, under Fiat-Shamir and with given challenges, and
compares the verdicts, the challenges, everything else prepare produces and every challenger's end
state.  The program is built with -fsanitize=address,undefined and with -fsanitize=thread and run
directly; any report of a sanitizer fails the run."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HOST = ROOT / "plonky3_eon_amd" / "host"
# per mode: five proofs prepared (0), a malformed batched opening (2), a missing permutation part (1),
# a trace degree above the pcs's (2)
WANT = "ok 00000212 00000212"


def build(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / ("verify_prepare_check_" + sanitize.split(",")[0])
    return exe, subprocess.run(
        [cxx, "-O1", "-g", "-std=c++17", "-pthread", f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined",
         "-I", str(ROOT / "include"), "-I", str(HOST), str(ROOT / "tests" / "verify_prepare_check.cpp"),
         str(HOST / "verify_prepare.cpp"), str(HOST / "transcript.cpp"), "-o", str(exe)],
        capture_output=True, text=True)


def test_prepare_includes_no_device_header():
    for name in ("verify_prepare.h", "verify_prepare.cpp"):
        text = (HOST / name).read_text()
        assert "hip/" not in text and "eon_ctx" not in text, name


def test_one_and_eight_threads_agree_under_asan_and_ubsan(tmp_path):
    exe, built = build(tmp_path, "address,undefined")
    assert built.returncode == 0, built.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == WANT and not out.stderr.strip(), out.stdout + out.stderr[-3000:]


def test_one_and_eight_threads_agree_under_tsan(tmp_path):
    exe, built = build(tmp_path, "thread")
    if built.returncode != 0 and ("tsan" in built.stderr or "cannot find" in built.stderr):
        pytest.skip("the thread sanitizer's runtime does not link with this toolchain")
    assert built.returncode == 0, built.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and "unexpected memory mapping" in out.stderr:
        pytest.skip("the thread sanitizer's runtime does not start on this kernel's address layout")
    assert out.returncode == 0 and out.stdout.strip() == WANT and not out.stderr.strip(), out.stdout + out.stderr[-3000:]
