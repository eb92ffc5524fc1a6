"""The windowed quotient driver (eon_quotient_values_rows_dev, AirProgram.quotient_values_rows) on
the GPU: on a window of LDE rows built by a wrapped row gather it reproduces, exactly, the rows of
the full quotient_values output -- the reference here, itself checked against the oracle in
test_gpu_air_program.py."""

import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from airs import MixedAir, MulAir
from oracle import coracle as C

pytestmark = pytest.mark.gpu
ALPHA = 0x1234567890ABCDEF1234567
PUBLICS = [5, 6]


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def window_of(lde, row0, n_rows, step):
    """rows (row0 + j) mod Q, j < n_rows + step"""
    import torch

    q = lde.shape[0]
    idx = (torch.arange(n_rows + step, device=lde.device) + row0) % q
    return lde[idx].contiguous()


@pytest.fixture(scope="module")
def mixed(gpu_ctx):
    """MixedAir (log_qd 3, public values, all three selectors) at log_n 3: the program, a random
    LDE of Q = 64 rows and its full quotient; never modified"""
    from plonky3_eon_amd.air import AirProgram

    prog = AirProgram(MixedAir(), gpu_ctx)
    assert prog.log_quotient_degree() == 3
    lde = dev(C.random_fr(5, 64 * 5).reshape(64, 5, 4))
    return prog, lde, prog.quotient_values(lde, 3, 3, ALPHA, PUBLICS)


@pytest.mark.parametrize("row0,n_rows", [(0, 64), (40, 24), (22, 21), (63, 1), (64, 0), (17, 0)])
def test_mixed_air_row_blocks(mixed, row0, n_rows):
    """the whole domain (the window is the LDE plus its first 8 rows again); a block whose halo
    wraps past Q; an odd block inside; the last row alone; no rows"""
    prog, lde, full = mixed
    window = window_of(lde, row0, n_rows, 8)
    got = prog.quotient_values_rows(window, 3, row0, n_rows, ALPHA, PUBLICS)
    assert tuple(got.shape) == (n_rows, 4)
    np.testing.assert_array_equal(got.cpu().numpy(), full[row0:row0 + n_rows].cpu().numpy())


def test_more_than_one_block(gpu_ctx):
    """MulAir at log_n 8: Q = 512, rows [200, 512) -- 312 threads, two 256-thread blocks, the second
    partial -- with the halo wrapping to rows 0, 1"""
    from plonky3_eon_amd.air import AirProgram

    prog = AirProgram(MulAir(), gpu_ctx)
    assert prog.log_quotient_degree() == 1
    lde = dev(C.random_fr(6, 512 * 60).reshape(512, 60, 4))
    full = prog.quotient_values(lde, 8, 1, ALPHA)
    got = prog.quotient_values_rows(window_of(lde, 200, 312, 2), 8, 200, 312, ALPHA)
    np.testing.assert_array_equal(got.cpu().numpy(), full[200:].cpu().numpy())


def test_global_register_file(mixed):
    """the register file in global memory (EON_AIR_REGS=global, read once per process: a child) is
    indexed by the row of the launch, not of the domain: rows [22, 43) again"""
    prog, lde, full = mixed
    code = ("import numpy as np, torch, sys; sys.path[:0] = ['tests', '.'];"
            "from airs import MixedAir; from plonky3_eon_amd import Context; from plonky3_eon_amd.air import AirProgram;"
            "ctx = Context(0); prog = AirProgram(MixedAir(), ctx);"
            "w = torch.from_numpy(np.load(sys.argv[1])).to('cuda:0');"
            f"out = prog.quotient_values_rows(w, 3, 22, 21, {ALPHA}, {PUBLICS});"
            "np.save(sys.argv[2], out.cpu().numpy())")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        win, out = os.path.join(d, "window.npy"), os.path.join(d, "out.npy")
        np.save(win, window_of(lde, 22, 21, 8).cpu().numpy())
        subprocess.run([sys.executable, "-c", code, win, out], check=True, cwd=root,
                       env=dict(os.environ, EON_AIR_REGS="global"), timeout=300)
        got = np.load(out)
    np.testing.assert_array_equal(got, full[22:43].cpu().numpy())


def test_rejections(gpu_ctx, mixed):
    from airs_preprocessed import MulFibPAir

    from plonky3_eon_amd import _lib
    from plonky3_eon_amd.air import AirProgram

    prog, lde, _ = mixed
    pre = AirProgram(MulFibPAir(), gpu_ctx)
    step = 1 << pre.log_quotient_degree()
    import torch

    w = torch.zeros((4 + step, pre.width, 4), dtype=torch.int64, device="cuda:0")
    with pytest.raises(_lib.EonError) as e:  # a program with preprocessed columns
        pre.quotient_values_rows(w, 3, 0, 4, ALPHA)
    assert e.value.code == _lib.EON_E_ARG and "preprocessed" in str(e.value)
    with pytest.raises(_lib.EonError) as e:  # rows past the domain
        prog.quotient_values_rows(window_of(lde, 60, 8, 8), 3, 60, 8, ALPHA, PUBLICS)
    assert e.value.code == _lib.EON_E_SHAPE
    with pytest.raises(ValueError):  # a window without its halo
        prog.quotient_values_rows(lde[:8].contiguous(), 3, 0, 8, ALPHA, PUBLICS)
