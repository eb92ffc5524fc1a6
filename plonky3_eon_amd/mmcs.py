"""Host-side mirror of the reference's KzgMmcs (kzg/src/mmcs.rs) over the C ABI (include/eon.h).

``KzgMmcs`` implements p3_commit::Mmcs<Fr> over the KZG SRS: a caller commits to a batch of matrices
of mixed heights (any height >= 1), every column a polynomial in COEFFICIENT form, and later opens
single rows: query ``index`` opens, in every matrix, the point ``Fr::new(local_index)`` with
``local_index = (index >> (log2_max_height - log2_height)) % height`` (mmcs.rs:213-218).

* ``commit``          -- one column MSM per matrix against the SRS tables (commit_matrix, mmcs.rs:155-165)
* ``open_batch``      -- open_batch (mmcs.rs:196-236) for one index
* ``open_batch_many`` -- the same for a list of indices in one call: every distinct (matrix, local
                         index) is divided once, all quotients go through one wide column MSM
                         (eon_kzg_mmcs_open_dev)
* ``verify_batch``    -- verify_batch (mmcs.rs:242-294): one batched pairing check

Matrices are (h, w, 4) uint64 Montgomery limbs, torch device tensors (int64 views) or numpy arrays
(uploaded).  Commitments and witnesses are (w, 8) uint64 affine points per matrix, opened values
(w, 4).  Everything runs in libeonhip.so; there is no CPU fallback.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .dft import Context, default_context, _is_torch
from .msm import MsmBases, srs_powers


class KzgError(Exception):
    """kzg/src/params.rs KzgError."""


class DegreeTooLarge(KzgError):
    """KzgError::DegreeTooLarge (kzg/src/params.rs:164-173)."""

    def __init__(self, degree: int, max_degree: int):
        super().__init__(f"polynomial degree {degree} exceeds SRS max degree {max_degree}")
        self.degree, self.max_degree = degree, max_degree


class ProofShapeMismatch(KzgError):
    """KzgError::ProofShapeMismatch: a malformed or rejected opening."""


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class KzgMmcsProverData:
    """KzgMmcsProverData: the committed matrices, kept on the device."""

    def __init__(self, matrices):
        self.matrices = matrices


def local_index(max_height: int, height: int, index: int) -> int:
    """The row of a matrix of `height` that query `index` opens (eon_kzg_mmcs_local_index)."""
    return int(_lib.load().eon_kzg_mmcs_local_index(int(max_height), int(height), int(index)))


class KzgMmcs:
    def __init__(self, max_degree: int, alpha, ctx: Context | None = None):
        """KzgMmcs::new: init_srs_unsafe(max_degree, alpha) (kzg/src/params.rs:123-139)."""
        from .verify import g2_mul

        self.ctx = ctx or default_context(0)
        self.max_degree = int(max_degree)
        self.bases = MsmBases(srs_powers(self.max_degree + 1, alpha, self.ctx), self.ctx, precompute=True)
        self.g2_alpha = g2_mul(alpha, ctx=self.ctx)

    @classmethod
    def from_srs(cls, bases: MsmBases, g2_alpha, max_degree: int) -> "KzgMmcs":
        """KzgMmcs::from_srs over an existing SRS table (shared with a KzgPcs, say)."""
        if bases.n < int(max_degree) + 1:
            raise DegreeTooLarge(int(max_degree), bases.n - 1)
        m = cls.__new__(cls)
        m.ctx, m.max_degree, m.bases = bases.ctx, int(max_degree), bases
        m.g2_alpha = np.ascontiguousarray(g2_alpha, dtype=np.uint64).reshape(16)
        return m

    # -- commit ---------------------------------------------------------------------------------
    def _to_device(self, mat):
        import torch

        if _is_torch(mat):
            return mat.contiguous()
        a = np.ascontiguousarray(mat, dtype=np.uint64)
        return torch.from_numpy(a.view(np.int64)).to(f"cuda:{self.ctx.device}")

    def commit(self, matrices):
        """-> (commitment: list of (w, 8) arrays, KzgMmcsProverData).  The columns are committed as
        they stand (coefficient form).  Raises DegreeTooLarge where the reference unwraps
        ensure_supported(height - 1) (mmcs.rs:178-182)."""
        dev, commitment = [], []
        for mat in matrices:
            h = int(mat.shape[0])
            if max(h - 1, 0) > self.max_degree:
                raise DegreeTooLarge(h - 1, self.max_degree)
        for mat in matrices:
            m = self._to_device(mat)
            commitment.append(self.bases.msm_columns(m))
            dev.append(m)
        return commitment, KzgMmcsProverData(dev)

    def get_matrices(self, prover_data: KzgMmcsProverData):
        return list(prover_data.matrices)

    # -- open -----------------------------------------------------------------------------------
    def open_batch_many(self, indices, prover_data: KzgMmcsProverData):
        """[(opened_values, witnesses) per index]; opened_values / witnesses are lists with one
        (w, 4) / (w, 8) array per matrix."""
        import torch

        mats = prover_data.matrices
        idx = np.asarray([int(i) for i in indices], dtype=np.uint64)
        widths = [int(m.shape[1]) for m in mats]
        W = sum(widths)
        descs = (_lib.eon_mmcs_matrix * max(len(mats), 1))()
        for k, m in enumerate(mats):
            descs[k].coeffs, descs[k].height, descs[k].width = m.data_ptr(), int(m.shape[0]), widths[k]
        values = np.zeros((len(idx), W, 4), dtype=np.uint64)
        wits = np.zeros((len(idx), W, 8), dtype=np.uint64)
        ctx = self.ctx
        if mats:
            ctx.set_stream(torch.cuda.current_stream(mats[0].device).cuda_stream)
        rc = ctx.lib.eon_kzg_mmcs_open_dev(ctx.handle, self.bases._h, descs, len(mats), _p(idx), len(idx),
                                           _p(values), _p(wits))
        if rc == _lib.EON_E_DEGREE_TOO_LARGE:
            raise DegreeTooLarge(max(int(m.shape[0]) for m in mats) - 1, self.bases.n - 1)
        ctx.check(rc)
        offs = np.concatenate([[0], np.cumsum(widths)]).astype(int)
        out = []
        for q in range(len(idx)):
            out.append(([values[q, offs[k]:offs[k + 1]].copy() for k in range(len(mats))],
                        [wits[q, offs[k]:offs[k + 1]].copy() for k in range(len(mats))]))
        return out

    def open_batch(self, index: int, prover_data: KzgMmcsProverData):
        return self.open_batch_many([index], prover_data)[0]

    # -- verify ---------------------------------------------------------------------------------
    def verify_batch(self, commitment, dimensions, index: int, opened_values, witnesses) -> None:
        """None for Ok(()), raises ProofShapeMismatch / DegreeTooLarge: the reference's verdicts.
        `dimensions` are (height, width) pairs or objects with .height / .width.

        As the reference: len(opened_values) != len(commitment) is a mismatch; then values,
        commitments, dimensions and witnesses are ZIPPED, so the walk stops at the shortest of the
        four lists and surplus entries of the others are not looked at -- except that max_height is
        taken over ALL dimensions (mmcs.rs:254).  Per matrix, a length disagreement between its
        values, its committed columns and its witnesses is a mismatch (the dimension's width is not
        consulted), and ensure_supported(height - 1) may answer DegreeTooLarge, in the reference's
        order.  A failed pairing check is a mismatch."""
        if len(opened_values) != len(commitment):
            raise ProofShapeMismatch("opened values for another number of matrices than committed")
        dims = [(int(d[0]), int(d[1])) if isinstance(d, (tuple, list)) else (int(d.height), int(d.width))
                for d in dimensions]
        k = min(len(opened_values), len(commitment), len(dims), len(witnesses))
        heights, widths, cs, vs, ws = [], [], [], [], []
        for m in range(k):
            v = np.asarray(opened_values[m], dtype=np.uint64).reshape(-1, 4)
            c = np.asarray(commitment[m], dtype=np.uint64).reshape(-1, 8)
            w = np.asarray(witnesses[m], dtype=np.uint64).reshape(-1, 8)
            if len(v) != len(c) or len(v) != len(w):
                raise ProofShapeMismatch(f"matrix {m}: {len(v)} values, {len(c)} columns, {len(w)} witnesses")
            if max(dims[m][0] - 1, 0) > self.max_degree:
                raise DegreeTooLarge(dims[m][0] - 1, self.max_degree)
            heights.append(dims[m][0])
            widths.append(len(v))
            cs.append(c), vs.append(v), ws.append(w)
        # max_height over all dimensions: a taller surplus dimension shifts the index further
        log2 = lambda x: (max(int(x), 1) - 1).bit_length()  # noqa: E731  next_power_of_two().trailing_zeros()
        extra = log2(max((h for h, _ in dims), default=0)) - log2(max(heights, default=0))
        index = int(index) >> extra
        cat = lambda xs, n: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros((0, n)), dtype=np.uint64)  # noqa: E731
        c, v, w = cat(cs, 8), cat(vs, 4), cat(ws, 8)
        hs, wd = np.asarray(heights, dtype=np.uint64), np.asarray(widths, dtype=np.uint32)
        ok = ctypes.c_int(0)
        ctx = self.ctx
        rc = ctx.lib.eon_kzg_mmcs_verify_batch(ctx.handle, _p(c), _p(hs), _p(wd), k, index, _p(v), _p(w),
                                               self.max_degree, _p(self.g2_alpha), ctypes.byref(ok))
        ctx.check(rc)
        if not ok.value:
            raise ProofShapeMismatch("the batched pairing check failed")
