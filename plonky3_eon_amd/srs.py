"""A supplied structured reference string: StructuredReferenceString of kzg/src/params.rs and the
input of KzgPcs::from_srs (kzg/src/pcs.rs:170-175).

* ``Srs(g1_powers, g2_alpha)``     -- the G1 powers as (n, 8) affine points (Fq Montgomery limbs) or
                                      as n x 32 compressed bytes (G1Affine::to_bytes), and g2_alpha
                                      as (16,) limbs in the eon_g2_affine layout; ``max_degree = n - 1``.
* ``Srs.unsafe(max_degree, alpha)``-- init_srs_unsafe (params.rs:123-139) from a known trapdoor: tests.
* ``g1_decompress(bytes)``         -- eon_g1_decompress: the device's inverse of g1_to_bytes.
* ``g1_compress(points)``          -- eon_g1_compress: g1_to_bytes of every point in one device call.
* ``g1_validate(points)``          -- eon_g1_validate_dev on uploaded points.
* ``srs_check(bases, n, g2, rho)`` -- eon_kzg_srs_check over an MsmBases table.
* ``Srs.save`` / ``Srs.load``      -- this project's own container (no ceremony format is read):

      offset  0  magic  b"EONSRS1\\0"
              8  u64    count n of G1 powers
             16  u32    flags: bit 0 = the G1 entries are compressed; every other bit zero
             20  u32    zero
             24  128 B  g2_alpha, eon_g2_affine (x.c0, x.c1, y.c0, y.c1 as Fq Montgomery LE)
            152  n entries: 32 B compressed, or 64 B eon_g1_affine (x, y Fq Montgomery LE)

  ``load(path, max_degree=k)`` reads only the first k + 1 entries: a prefix of a valid SRS is a
  valid SRS.  A bad header raises SrsError before any device work.

``SrsError(reason, index)`` is also what a rejected SRS raises (EON_E_SRS): the reason names of
include/eon.h's EON_SRS_* and, for the per-point reasons, the lowest offending index.
"""

from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _lib
from .dft import Context, default_context
from .field import FR_MODULUS, fr_to_abi

MAGIC = b"EONSRS1\0"
HEADER_BYTES = 8 + 8 + 4 + 4 + 128
FLAG_COMPRESSED = 1
DECOMPRESS_WORKGROUP = 256  # lanes per workgroup of the per-point kernels (csrc/srs.hip SRS_THREADS)

REASONS = {
    _lib.EON_SRS_OK: "OK",
    _lib.EON_SRS_ENCODING: "ENCODING",
    _lib.EON_SRS_NOT_CANONICAL: "NOT_CANONICAL",
    _lib.EON_SRS_NOT_ON_CURVE: "NOT_ON_CURVE",
    _lib.EON_SRS_IDENTITY: "IDENTITY",
    _lib.EON_SRS_G0_NOT_GENERATOR: "G0_NOT_GENERATOR",
    _lib.EON_SRS_G2_INVALID: "G2_INVALID",
    _lib.EON_SRS_STRUCTURE: "STRUCTURE",
}


class SrsError(Exception):
    """A rejected SRS.  `reason` is one of REASONS' names, or "CONTAINER" for a malformed file;
    `index` the lowest offending point for ENCODING / NOT_CANONICAL / NOT_ON_CURVE / IDENTITY, else 0."""

    def __init__(self, reason, index: int = 0, detail: str = ""):
        self.reason = REASONS.get(reason, reason)
        self.index = int(index)
        self.code = _lib.EON_E_SRS
        where = f" at index {self.index}" if self.reason in ("ENCODING", "NOT_CANONICAL", "NOT_ON_CURVE",
                                                             "IDENTITY") else ""
        super().__init__(f"SRS rejected: {self.reason}{where}" + (f" ({detail})" if detail else ""))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def check_report(ctx: Context, rc: int, report: "_lib.eon_srs_report"):
    """rc of an entry point that fills an eon_srs_report: SrsError on EON_E_SRS, EonError otherwise."""
    if rc == _lib.EON_E_SRS:
        raise SrsError(int(report.reason), int(report.index))
    ctx.check(rc)


def g1_decompress(data, ctx: Context | None = None) -> np.ndarray:
    """n x 32 compressed bytes -> (n, 8) affine points (eon_g1_decompress); SrsError names the
    lowest rejected index."""
    ctx = ctx or default_context(0)
    b = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else \
        np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if b.size % 32:
        raise ValueError("compressed G1 points are 32 bytes each")
    n = b.size // 32
    # a copy in 8-byte-aligned storage: the device reads words
    buf = np.zeros(max(n, 1) * 4, dtype=np.uint64)
    buf.view(np.uint8)[:b.size] = b
    out = np.zeros((n, 8), dtype=np.uint64)
    rep = _lib.eon_srs_report()
    check_report(ctx, ctx.lib.eon_g1_decompress(ctx.handle, _p(buf), n, _p(out), ctypes.byref(rep)), rep)
    return out


def g1_compress(points, ctx: Context | None = None) -> bytes:
    """(n, 8) affine points -> n x 32 compressed bytes (eon_g1_compress): eon_g1_to_bytes of every
    point, one lane each; (0,0) is the identity.  SrsError("NOT_CANONICAL", index) names the lowest
    point with a coordinate >= q."""
    ctx = ctx or default_context(0)
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    n = p.shape[0]
    out = np.zeros(max(n, 1) * 4, dtype=np.uint64)
    rep = _lib.eon_srs_report()
    check_report(ctx, ctx.lib.eon_g1_compress(ctx.handle, _p(p), n, _p(out), ctypes.byref(rep)), rep)
    return out.view(np.uint8)[:32 * n].tobytes()


def g1_validate(points, ctx: Context | None = None) -> None:
    """eon_g1_validate_dev on (n, 8) affine points (uploaded): canonical, on the curve, no identity."""
    import torch

    ctx = ctx or default_context(0)
    p = np.array(points, dtype=np.uint64).reshape(-1, 8)  # a writable copy for torch
    d = torch.from_numpy(p.view(np.int64)).to(f"cuda:{ctx.device}")
    torch.cuda.synchronize(d.device)
    rep = _lib.eon_srs_report()
    check_report(ctx, ctx.lib.eon_g1_validate_dev(ctx.handle, ctypes.c_void_p(d.data_ptr()), p.shape[0],
                                                  ctypes.byref(rep)), rep)


def srs_check(bases, n: int, g2_alpha, rho: int, ctx: Context | None = None) -> None:
    """eon_kzg_srs_check of the first n points of an MsmBases table against g2_alpha with the
    challenge rho (a canonical int in [1, r)); SrsError on rejection."""
    ctx = ctx or bases.ctx
    g = np.ascontiguousarray(g2_alpha, dtype=np.uint64).reshape(16)
    if not 0 <= int(rho) < FR_MODULUS:
        raise _lib.EonError(_lib.EON_E_ARG, "rho must be a canonical Fr")
    r = fr_to_abi(int(rho))
    rep = _lib.eon_srs_report()
    check_report(ctx, ctx.lib.eon_kzg_srs_check(ctx.handle, bases._h, int(n), _p(g), ctypes.byref(r),
                                                ctypes.byref(rep)), rep)


class Srs:
    """g1_powers: (n, 8) uint64 affine points, or bytes / a uint8 array of n x 32 compressed points
    (kept compressed: the device decompresses them when a prover is made); g2_alpha: (16,) uint64."""

    def __init__(self, g1_powers, g2_alpha):
        if isinstance(g1_powers, (bytes, bytearray, memoryview)) or \
                (isinstance(g1_powers, np.ndarray) and g1_powers.dtype == np.uint8):
            raw = bytes(g1_powers) if not isinstance(g1_powers, np.ndarray) else g1_powers.tobytes()
            if len(raw) % 32 or not raw:
                raise ValueError("compressed G1 powers are 32 bytes each, at least one")
            self.compressed = True
            self.g1_bytes = raw
            self.g1_powers = None
            self.n = len(raw) // 32
        else:
            self.compressed = False
            self.g1_powers = np.ascontiguousarray(g1_powers, dtype=np.uint64).reshape(-1, 8)
            self.g1_bytes = None
            self.n = self.g1_powers.shape[0]
            if self.n == 0:
                raise ValueError("an SRS has at least one G1 power")
        self.g2_alpha = np.ascontiguousarray(g2_alpha, dtype=np.uint64).reshape(16).copy()

    @property
    def max_degree(self) -> int:
        return self.n - 1

    @classmethod
    def unsafe(cls, max_degree: int, alpha: int, ctx: Context | None = None) -> "Srs":
        """init_srs_unsafe(max_degree, alpha): the trapdoor is known to the caller.  Tests only."""
        from .msm import srs_powers
        from .verify import g2_mul

        ctx = ctx or default_context(0)
        return cls(srs_powers(int(max_degree) + 1, alpha, ctx), g2_mul(alpha, ctx=ctx))

    def prefix(self, max_degree: int) -> "Srs":
        """The SRS of the first max_degree + 1 powers."""
        k = int(max_degree) + 1
        if k < 1 or k > self.n:
            raise SrsError("CONTAINER", 0, f"max_degree {max_degree} needs {k} powers, the SRS has {self.n}")
        return Srs(self.g1_bytes[:32 * k] if self.compressed else self.g1_powers[:k], self.g2_alpha)

    def compress(self, ctx: Context | None = None) -> "Srs":
        """The same SRS with its G1 powers as compressed bytes: eon_g1_to_bytes of every point, in
        ONE g1_compress call on the device.  Only a host with no GPU at all (a tool that writes a
        container, like eon_proof_serialize) takes the host's eon_g1_to_bytes per point instead; with
        a device present a failing kernel is an error, never that loop."""
        if self.compressed:
            return self
        if ctx is None:
            import torch

            if not torch.cuda.is_available():
                from .native import g1_to_bytes

                return Srs(b"".join(g1_to_bytes(p) for p in self.g1_powers), self.g2_alpha)
        return Srs(g1_compress(self.g1_powers, ctx), self.g2_alpha)

    def save(self, path, compressed: bool = True) -> None:
        if compressed:
            body = self.compress().g1_bytes
        elif self.compressed:
            raise ValueError("decompress the powers first (g1_decompress): this Srs holds compressed bytes")
        else:
            body = self.g1_powers.astype("<u8").tobytes()
        head = MAGIC + struct.pack("<QII", self.n, FLAG_COMPRESSED if compressed else 0, 0) + \
            self.g2_alpha.astype("<u8").tobytes()
        with open(path, "wb") as f:
            f.write(head)
            f.write(body)

    @classmethod
    def load(cls, path, max_degree: int | None = None) -> "Srs":
        """Read the container; with max_degree = k only the first k + 1 entries are read.  Bad magic,
        a truncated file, k + 1 > count, count == 0 and nonzero reserved bits raise
        SrsError("CONTAINER") -- the header is checked before any entry is touched."""
        with open(path, "rb") as f:
            head = f.read(HEADER_BYTES)
            if len(head) < HEADER_BYTES:
                raise SrsError("CONTAINER", 0, "truncated header")
            if head[:8] != MAGIC:
                raise SrsError("CONTAINER", 0, "bad magic")
            count, flags, zero = struct.unpack("<QII", head[8:24])
            if flags & ~FLAG_COMPRESSED or zero:
                raise SrsError("CONTAINER", 0, "reserved bits set")
            if count == 0:
                raise SrsError("CONTAINER", 0, "no G1 powers")
            k = count if max_degree is None else int(max_degree) + 1
            if k < 1 or k > count:
                raise SrsError("CONTAINER", 0, f"max_degree {max_degree} needs {k} powers, the file has {count}")
            entry = 32 if flags & FLAG_COMPRESSED else 64
            f.seek(0, 2)
            if f.tell() < HEADER_BYTES + count * entry:
                raise SrsError("CONTAINER", 0, "truncated: fewer entries than the header's count")
            f.seek(HEADER_BYTES)
            body = f.read(k * entry)
        g2 = np.frombuffer(head[24:], dtype="<u8").astype(np.uint64)
        if flags & FLAG_COMPRESSED:
            return cls(body, g2)
        return cls(np.frombuffer(body, dtype="<u8").astype(np.uint64).reshape(k, 8), g2)
