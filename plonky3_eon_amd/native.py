"""ctypes binding of the native prove driver libeonprove.so (include/eon_prove.h).

The driver is the C++ host side above eon.h (plonky3_eon_amd/host/): KzgPcs + prove for the
Poseidon2-AIR, the product host (tests/mirror_prover.py is a test-only Python mirror of the same
orchestration).  Its Proof has prover.Proof's shape, so the two are compared field by field in the tests.

Sharded prove: an eon_collective is either
* ``TorchCollective(group)`` -- a ctypes callback over torch.distributed (gloo stages through host
  memory; used by the CPU-hosted multi-rank tests), or
* ``RcclCollective(rank, world, group)`` -- the driver's own RCCL communicator (ncclAllGather on
  device buffers over xGMI); the 128-byte unique id is broadcast with torch.distributed.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

from . import _lib
from .collective import ALL_GATHER_FN, TorchCollective, eon_collective  # noqa: F401 (re-exported)
from .dft import Context, default_context
from .field import fr_to_abi, fr_unmont
from .proof import Opened, Proof, ProofFormatError, VerificationError, log_quotient_degree  # noqa: F401 (re-exported)

PROVE_LIB_PATH = Path(__file__).resolve().parent / "libeonprove.so"

_P = ctypes.c_void_p
_U32 = ctypes.c_uint32
_U64 = ctypes.c_uint64
_INT = ctypes.c_int

STAGES = ["commit to trace data", "trace LDE (get_evaluations_on_domain)", "quotient_values",
          "exchange partial quotients", "commit to quotient poly chunks", "open", "assemble columns"]
EON_STAGES = 8
EON_SRS_TRUSTED = 1  # eon_kzg_pcs_create_from_srs flags: skip eon_kzg_srs_check
EON_OPENING_PER_COLUMN = 0
EON_OPENING_BATCHED = 1
OPENING_MODES = {"per_column": EON_OPENING_PER_COLUMN, "batched": EON_OPENING_BATCHED}

class eon_proof(ctypes.Structure):
    _fields_ = [("trace_commit", _P), ("quotient_commit", _P), ("trace_opened", _P), ("trace_witnesses", _P),
                ("quotient_opened", _P), ("quotient_witnesses", _P), ("degree_bits", _U32),
                ("stage_ms", ctypes.c_double * EON_STAGES)]


class eon_proof_pp(ctypes.Structure):
    _fields_ = [("base", eon_proof), ("preprocessed_commit", _P), ("preprocessed_opened", _P),
                ("preprocessed_witnesses", _P)]


class eon_proof_lk(ctypes.Structure):
    _fields_ = [("pp", eon_proof_pp), ("permutation_commit", _P), ("permutation_opened", _P),
                ("permutation_witnesses", _P)]


class eon_proof_shape(ctypes.Structure):
    _fields_ = [(k, _U32) for k in ("flags", "degree_bits", "width", "chunks", "pre_width", "perm_width")]


class eon_proof_io_report(ctypes.Structure):
    _fields_ = [("reason", _U32), ("section", _U32), ("index", _U64)]


EON_PROOF_BATCHED = 1
EON_PROOF_PREPROCESSED = 2
EON_PROOF_PERMUTATION = 4

# name -> (restype, argtypes): every entry point of include/eon_prove.h
SIGNATURES = {
    "eon_prove_abi_version": (_U32, []),
    "eon_kzg_pcs_create": (_INT, [_P, _U64, _P, ctypes.POINTER(_P)]),
    "eon_kzg_pcs_create_from_srs": (_INT, [_P, _P, _U64, _P, _U32, _P, ctypes.POINTER(_P),
                                           ctypes.POINTER(_lib.eon_srs_report)]),
    "eon_kzg_pcs_create_from_srs_bytes": (_INT, [_P, _P, _U64, _P, _U32, _P, ctypes.POINTER(_P),
                                                 ctypes.POINTER(_lib.eon_srs_report)]),
    "eon_kzg_pcs_create_verifier": (_INT, [_P, _U64, _P, ctypes.POINTER(_P)]),
    "eon_kzg_pcs_destroy": (None, [_P]),
    "eon_kzg_pcs_last_error": (ctypes.c_char_p, [_P]),
    "eon_kzg_pcs_set_check_constraints": (_INT, [_P, _INT]),
    "eon_kzg_pcs_check_constraints": (_INT, [_P]),
    "eon_kzg_pcs_last_constraint_report": (_INT, [_P, ctypes.POINTER(_lib.eon_constraint_report)]),
    "eon_kzg_pcs_set_opening": (_INT, [_P, _U32]),
    "eon_kzg_pcs_opening": (_INT, [_P]),
    "eon_kzg_pcs_set_opening_challenges": (_INT, [_P, _P, _P]),
    "eon_kzg_pcs_last_opening_challenges": (_INT, [_P, _P, _P]),
    "eon_rccl_unique_id": (_INT, [_P]),
    "eon_rccl_collective_init": (_INT, [_U32, _U32, _P, ctypes.POINTER(eon_collective)]),
    "eon_rccl_collective_info": (_INT, [ctypes.POINTER(eon_collective), ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                        ctypes.c_char_p, _U32]),
    "eon_rccl_collective_finalize": (None, [ctypes.POINTER(eon_collective)]),
    "eon_emulated_collective_init": (_INT, [_U32, _U32, ctypes.POINTER(eon_collective)]),
    "eon_prove_p2air": (_INT, [_P, _P, _P, _U64, _P, _P, _U32, ctypes.POINTER(eon_collective),
                               ctypes.POINTER(eon_proof)]),
    "eon_poseidon2_bn254_permute": (_INT, [_P, _P]),
    "eon_g1_to_bytes": (_INT, [_P, _P]),
    "eon_challenger_create": (_INT, [_P, ctypes.POINTER(_P)]),
    "eon_challenger_destroy": (None, [_P]),
    "eon_challenger_observe": (_INT, [_P, _P, _U64]),
    "eon_challenger_observe_g1": (_INT, [_P, _P, _U64]),
    "eon_challenger_sample": (_INT, [_P, _P]),
    "eon_challenger_state": (_INT, [_P, _P]),
    "eon_prove_p2air_fs": (_INT, [_P, _P, _P, _U64, _P, _U32, ctypes.POINTER(eon_collective),
                                  ctypes.POINTER(eon_proof), _P, _P]),
    "eon_prove_air": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, _P, ctypes.POINTER(eon_proof)]),
    "eon_prove_air_fs": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, ctypes.POINTER(eon_proof), _P, _P]),
    "eon_prove_air_sharded": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, _P, ctypes.POINTER(eon_collective),
                                     ctypes.POINTER(eon_proof)]),
    "eon_prove_air_sharded_fs": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, ctypes.POINTER(eon_collective),
                                        ctypes.POINTER(eon_proof), _P, _P]),
    "eon_setup_preprocessed": (_INT, [_P, _P, _U64, _U32, ctypes.POINTER(_P)]),
    "eon_preprocessed_destroy": (None, [_P]),
    "eon_preprocessed_info": (_INT, [_P, ctypes.POINTER(_U32), ctypes.POINTER(_U32)]),
    "eon_preprocessed_commitment": (_INT, [_P, _P]),
    "eon_prove_air_pp": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, _P, _P, ctypes.POINTER(eon_proof_pp)]),
    "eon_prove_air_pp_fs": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, _P, ctypes.POINTER(eon_proof_pp), _P, _P]),
    "eon_prove_air_lk": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, _P, _P, _U32, _P, _P, ctypes.POINTER(eon_proof_lk)]),
    "eon_prove_air_lk_fs": (_INT, [_P, _P, _P, _U64, _P, _U32, _P, _P, _P, ctypes.POINTER(eon_proof_lk), _P, _P, _P]),
    "eon_proof_bytes_size": (_U64, [ctypes.POINTER(eon_proof_shape)]),
    "eon_proof_serialize": (_INT, [ctypes.POINTER(eon_proof_lk), ctypes.POINTER(eon_proof_shape), _P, _U64,
                                   ctypes.POINTER(_U64)]),
    "eon_proof_peek": (_INT, [_P, _U64, ctypes.POINTER(eon_proof_shape), ctypes.POINTER(eon_proof_io_report)]),
    "eon_proof_deserialize": (_INT, [_P, _P, _U64, ctypes.POINTER(eon_proof_lk),
                                     ctypes.POINTER(eon_proof_io_report)]),
    "eon_verify_air": (_INT, [_P, _P, ctypes.POINTER(eon_proof_lk), _P, _U32, _U32, _U32, _P, _P, _U32, _P, _P,
                              ctypes.POINTER(_INT)]),
    "eon_verify_air_fs": (_INT, [_P, _P, ctypes.POINTER(eon_proof_lk), _P, _U32, _U32, _U32, _P, _P,
                                 ctypes.POINTER(_INT), _P, _P, _P]),
    "eon_verify_air_many": (_INT, [_P, _P, ctypes.POINTER(eon_proof_lk), _U32, _P, _U32, _U32, _U32, _P, _P, _U32,
                                   _P, _P, _P, _P, _P]),
    "eon_verify_air_many_fs": (_INT, [_P, _P, ctypes.POINTER(eon_proof_lk), _U32, _P, _U32, _U32, _U32, _P, _P, _P,
                                      _P, _P, _P]),
    "eon_verify_many_detail": (ctypes.c_char_p, [_P, _U32]),
    "eon_verify_many_opening_challenges": (_INT, [_P, _U32, _P, _P]),
}

_plib = None


def load() -> ctypes.CDLL:
    """Load libeonprove.so (after libeonhip.so, which it links).  Raises if it is absent."""
    global _plib
    if _plib is not None:
        return _plib
    _lib.load()
    path = Path(os.environ["EON_PROVE_LIB"]) if os.environ.get("EON_PROVE_LIB") else PROVE_LIB_PATH
    if not path.exists():
        raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(os.fspath(path))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _plib = lib
    return lib


class ConstraintError(RuntimeError):
    """EON_E_CONSTRAINT from a prove with NativeKzgPcs.check_constraints on: the trace does not
    satisfy the AIR.  `report` (air.ConstraintReport) is the first failure and the counts."""

    def __init__(self, msg: str, report):
        super().__init__(msg)
        self.code = _lib.EON_E_CONSTRAINT
        self.report = report


class NativeKzgPcs:
    """KzgPcs::new(max_degree, alpha) inside the native driver (SRS and bases on device)."""

    def __init__(self, max_degree: int, alpha: int, ctx: Context | None = None):
        self.ctx = ctx or default_context(0)
        self.lib = load()
        self.max_degree = max_degree
        h = ctypes.c_void_p()
        a = fr_to_abi(alpha)
        self.ctx.check(self.lib.eon_kzg_pcs_create(self.ctx.handle, max_degree, ctypes.byref(a), ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_srs(cls, srs, validate: bool = True, rho: int | None = None,
                 ctx: Context | None = None) -> "NativeKzgPcs":
        """KzgPcs::from_srs (kzg/src/pcs.rs:170-175) over a supplied srs.Srs, affine or compressed:
        eon_kzg_pcs_create_from_srs[_bytes].  Every point is decompressed / validated on the device;
        with `validate` the SRS is also checked against its g2_alpha (eon_kzg_srs_check) with the
        challenge `rho`, by default drawn here, after the SRS is fixed, from the OS's randomness.
        validate=False is EON_SRS_TRUSTED: the caller vouches for the table.  Raises srs.SrsError
        (reason, index) when the SRS is rejected."""
        import secrets

        from .field import FR_MODULUS
        from .srs import SrsError

        self = cls.__new__(cls)
        self.ctx = ctx or default_context(0)
        self.lib = load()
        self.max_degree = srs.max_degree
        self._h = None
        flags = 0 if validate else EON_SRS_TRUSTED
        r = None
        if validate:
            r = fr_to_abi(int(rho) if rho is not None else secrets.randbelow(FR_MODULUS - 1) + 1)
        g2 = np.ascontiguousarray(srs.g2_alpha, dtype=np.uint64).reshape(16)
        rep = _lib.eon_srs_report()
        h = ctypes.c_void_p()
        self.ctx.set_stream(None)
        if srs.compressed:
            buf = np.zeros(srs.n * 4, dtype=np.uint64)  # word-aligned staging of the bytes
            buf.view(np.uint8)[:] = np.frombuffer(srs.g1_bytes, dtype=np.uint8)
            rc = self.lib.eon_kzg_pcs_create_from_srs_bytes(self.ctx.handle, _p(buf), srs.n, _p(g2), flags,
                                                            ctypes.byref(r) if r is not None else None,
                                                            ctypes.byref(h), ctypes.byref(rep))
        else:
            pts = np.ascontiguousarray(srs.g1_powers, dtype=np.uint64)
            rc = self.lib.eon_kzg_pcs_create_from_srs(self.ctx.handle, _p(pts), srs.n, _p(g2), flags,
                                                      ctypes.byref(r) if r is not None else None,
                                                      ctypes.byref(h), ctypes.byref(rep))
        if rc == _lib.EON_E_SRS:
            raise SrsError(int(rep.reason), int(rep.index))
        self.ctx.check(rc)
        self._h = h
        return self

    @classmethod
    def verifier(cls, max_degree: int, g2_alpha, ctx: Context | None = None) -> "NativeKzgPcs":
        """eon_kzg_pcs_create_verifier: the verifier's half of an SRS (max_degree and g2_alpha), no
        G1 table.  verify_native works on it; every prove and setup raises EonError(EON_E_ARG)."""
        self = cls.__new__(cls)
        self.ctx = ctx or default_context(0)
        self.lib = load()
        self.max_degree = int(max_degree)
        g2 = np.ascontiguousarray(g2_alpha, dtype=np.uint64).reshape(16)
        h = ctypes.c_void_p()
        self.ctx.check(self.lib.eon_kzg_pcs_create_verifier(self.ctx.handle, self.max_degree, _p(g2), ctypes.byref(h)))
        self._h = h
        return self

    def check(self, rc: int):
        if rc == _lib.EON_E_CONSTRAINT:
            raise ConstraintError(self.lib.eon_kzg_pcs_last_error(self._h).decode(), self.last_constraint_report())
        if rc != 0:
            raise _lib.EonError(rc, self.lib.eon_kzg_pcs_last_error(self._h).decode())

    @property
    def check_constraints(self) -> bool:
        """Run check_constraints (prover.rs:252-262, the reference's debug builds) in every generic
        prove; a failing trace then raises ConstraintError instead of yielding a proof."""
        return bool(self.lib.eon_kzg_pcs_check_constraints(self._h))

    @check_constraints.setter
    def check_constraints(self, enable: bool):
        _check(self.lib.eon_kzg_pcs_set_check_constraints(self._h, 1 if enable else 0),
               "eon_kzg_pcs_set_check_constraints")

    def last_constraint_report(self):
        from .air import ConstraintReport

        rep = _lib.eon_constraint_report()
        _check(self.lib.eon_kzg_pcs_last_constraint_report(self._h, ctypes.byref(rep)),
               "eon_kzg_pcs_last_constraint_report")
        return ConstraintReport.from_abi(rep)

    def opening_scope(self, opening: str, gamma=None, delta=None):
        """Context manager: the pcs's opening mode ("per_column" / "batched") and fixed opening
        challenges (canonical ints or None) for one call, the mode restored afterwards.  The
        per-column mode makes no C call at all, so a default prove is what it is without this."""
        import contextlib

        if opening not in OPENING_MODES:
            raise ValueError(f"opening must be one of {sorted(OPENING_MODES)}, not {opening!r}")

        @contextlib.contextmanager
        def scope():
            if opening == "per_column":
                if self.lib.eon_kzg_pcs_opening(self._h) == EON_OPENING_PER_COLUMN:
                    yield
                    return
            before = self.lib.eon_kzg_pcs_opening(self._h)
            g = fr_to_abi(gamma) if gamma is not None else None
            d = fr_to_abi(delta) if delta is not None else None
            _check(self.lib.eon_kzg_pcs_set_opening_challenges(self._h, ctypes.byref(g) if g is not None else None,
                                                               ctypes.byref(d) if d is not None else None),
                   "eon_kzg_pcs_set_opening_challenges")
            _check(self.lib.eon_kzg_pcs_set_opening(self._h, OPENING_MODES[opening]), "eon_kzg_pcs_set_opening")
            try:
                yield
            finally:
                self.lib.eon_kzg_pcs_set_opening(self._h, before)

        return scope()

    def last_opening_challenges(self):
        """(gamma, delta) of the last batched prove or verify on this pcs, canonical ints."""
        g, d = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        _check(self.lib.eon_kzg_pcs_last_opening_challenges(self._h, _p(g), _p(d)),
               "eon_kzg_pcs_last_opening_challenges")
        unm = lambda v: fr_unmont(sum(int(x) << (64 * i) for i, x in enumerate(v)))  # noqa: E731
        return unm(g), unm(d)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.eon_kzg_pcs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RcclInitError(RuntimeError):
    """The RCCL communicator could not be made on every rank; raised on EVERY rank alike, so all of
    them can fall back together (a rank-local failure would leave the others in a collective)."""


class RcclCollective:
    """eon_collective backed by the driver's RCCL communicator.

    Construction is itself collective over the torch process group `group` and ends the same way
    on every rank: rank 0 broadcasts the unique id -- or a failure sentinel when
    eon_rccl_unique_id fails, so the other ranks never wait in a broadcast rank 0 skipped -- every
    rank initialises its communicator, and the ranks then agree on the outcome (an all-gather of
    the init codes).  If any rank failed, every rank finalises the communicator it may have made
    and raises RcclInitError."""

    def __init__(self, rank: int, world: int, group=None):
        import torch.distributed as dist

        self.lib = load()
        self.c = None
        idbuf = (ctypes.c_uint8 * 128)()
        id_rc = 0
        if rank == 0:
            id_rc = self.lib.eon_rccl_unique_id(idbuf)
        if world > 1:
            obj = [bytes(idbuf) if id_rc == 0 else None]
            dist.broadcast_object_list(obj, src=0, group=group)
            if obj[0] is None:
                raise RcclInitError("eon_rccl_unique_id failed on rank 0")
            idbuf = (ctypes.c_uint8 * 128).from_buffer_copy(obj[0])
        elif id_rc != 0:
            raise RcclInitError(f"eon_rccl_unique_id failed ({id_rc})")
        c = eon_collective()
        try:
            rc = self.lib.eon_rccl_collective_init(rank, world, idbuf, ctypes.byref(c))
        except Exception:  # ctypes-level failure: report it to the other ranks like an error code
            rc = -1
        codes = [rc]
        if world > 1:
            codes = [None] * world
            dist.all_gather_object(codes, rc, group=group)
        if any(x != 0 for x in codes):
            if rc == 0:
                self.lib.eon_rccl_collective_finalize(ctypes.byref(c))
            bad = [g for g, x in enumerate(codes) if x != 0]
            raise RcclInitError(f"eon_rccl_collective_init failed on ranks {bad} (codes {[codes[g] for g in bad]})")
        self.c = c

    def info(self) -> dict:
        """ncclCommCount / ncclCommUserRank / ncclCommCuDevice and the device's PCI bus id, as the
        communicator reports them (bench.py's N > 1 line carries these per rank)."""
        n, r, d = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        pci = ctypes.create_string_buffer(64)
        rc = self.lib.eon_rccl_collective_info(ctypes.byref(self.c), ctypes.byref(n), ctypes.byref(r),
                                               ctypes.byref(d), pci, 64)
        if rc != 0:
            raise _lib.EonError(rc, "eon_rccl_collective_info")
        return {"nccl_comm_count": n.value, "nccl_user_rank": r.value, "nccl_cu_device": d.value,
                "nccl_pci_bus_id": pci.value.decode()}

    def close(self):
        if getattr(self, "c", None) is not None and self.c.user:
            self.lib.eon_rccl_collective_finalize(ctypes.byref(self.c))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EmulatedCollective:
    """eon_emulated_collective_init: the exchanges of rank `rank` in a `world`-rank prove emulated
    on one GPU (bench.py --emulate-world): same bytes and stream order, own data in every slot."""

    def __init__(self, rank: int, world: int):
        self.lib = load()
        self.c = eon_collective()
        rc = self.lib.eon_emulated_collective_init(rank, world, ctypes.byref(self.c))
        if rc != 0:
            raise _lib.EonError(rc, "eon_emulated_collective_init")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check(rc: int, what: str):
    if rc != 0:
        raise _lib.EonError(rc, what)


class Poseidon2Constants:
    """eon_poseidon2_constants over host arrays, the layout Poseidon2Air takes: begin/end
    (half_full_rounds, 3, 4) and partial (partial_rounds, 4) Montgomery u64 limbs."""

    def __init__(self, begin, partial, end):
        self.begin = np.ascontiguousarray(begin, dtype=np.uint64).reshape(-1, 3, 4)
        self.partial = np.ascontiguousarray(partial, dtype=np.uint64).reshape(-1, 4)
        self.end = np.ascontiguousarray(end, dtype=np.uint64).reshape(-1, 3, 4)
        self.c = _lib.eon_poseidon2_constants(self.begin.shape[0], self.partial.shape[0], _p(self.begin),
                                              _p(self.partial), _p(self.end))


def poseidon2_permute(consts: Poseidon2Constants, state) -> np.ndarray:
    """eon_poseidon2_bn254_permute: state = 3 Montgomery Fr (3, 4) u64."""
    s = np.ascontiguousarray(np.asarray(state, dtype=np.uint64).reshape(3, 4)).copy()
    _check(load().eon_poseidon2_bn254_permute(ctypes.byref(consts.c), _p(s)), "eon_poseidon2_bn254_permute")
    return s


def g1_to_bytes(point) -> bytes:
    """eon_g1_to_bytes of one eon_g1_affine (8 u64: x, y Fq Montgomery)."""
    p = np.ascontiguousarray(np.asarray(point, dtype=np.uint64).reshape(8))
    out = (ctypes.c_uint8 * 32)()
    _check(load().eon_g1_to_bytes(_p(p), out), "eon_g1_to_bytes")
    return bytes(out)


class Challenger:
    """DuplexChallenger<Fr, Poseidon2Bn254<3>, 3, 2> of libeonprove (eon_challenger_*)."""

    def __init__(self, consts: Poseidon2Constants):
        self.lib = load()
        self.consts = consts  # the C side copies them; kept for symmetry with the AIR
        h = _P()
        _check(self.lib.eon_challenger_create(ctypes.byref(consts.c), ctypes.byref(h)), "eon_challenger_create")
        self._h = h

    @property
    def handle(self):
        return self._h

    def observe(self, values):
        """Montgomery Fr limbs (..., 4)"""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1, 4))
        _check(self.lib.eon_challenger_observe(self._h, _p(v), v.shape[0]), "eon_challenger_observe")

    def observe_g1(self, points):
        """eon_g1_affine rows (..., 8)"""
        v = np.ascontiguousarray(np.asarray(points, dtype=np.uint64).reshape(-1, 8))
        _check(self.lib.eon_challenger_observe_g1(self._h, _p(v), v.shape[0]), "eon_challenger_observe_g1")

    def sample(self) -> np.ndarray:
        out = np.zeros(4, np.uint64)
        _check(self.lib.eon_challenger_sample(self._h, _p(out)), "eon_challenger_sample")
        return out

    def state(self) -> np.ndarray:
        out = np.zeros((3, 4), np.uint64)
        _check(self.lib.eon_challenger_state(self._h, _p(out)), "eon_challenger_state")
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.lib.eon_challenger_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Preprocessed:
    """eon_preprocessed: PreprocessedProverData (eon-uni-stark/src/preprocessed.rs:12-24), the
    preprocessed trace committed once and reused by every prove; (width, degree_bits, commitment)
    is the verifier's PreprocessedVerifierKey."""

    def __init__(self, pcs: NativeKzgPcs, handle):
        self.pcs = pcs  # the handle's data lives on the pcs's context
        self._h = handle
        w, d = _U32(), _U32()
        _check(pcs.lib.eon_preprocessed_info(handle, ctypes.byref(w), ctypes.byref(d)), "eon_preprocessed_info")
        self.width, self.degree_bits = int(w.value), int(d.value)
        self.commitment = np.zeros((self.width, 8), np.uint64)
        _check(pcs.lib.eon_preprocessed_commitment(handle, _p(self.commitment)), "eon_preprocessed_commitment")

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self.pcs.lib.eon_preprocessed_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def setup_preprocessed(pcs: NativeKzgPcs, pre_trace) -> Preprocessed:
    """setup_preprocessed (preprocessed.rs:47-94): commit the (N, Wp, 4) device tensor `pre_trace`
    on the natural domain of N.  The tensor is copied; it need not outlive the call."""
    import torch

    t = pre_trace.contiguous()
    torch.cuda.synchronize(t.device)  # produced on torch's stream
    pcs.ctx.set_stream(None)
    h = _P()
    pcs.check(pcs.lib.eon_setup_preprocessed(pcs._h, ctypes.c_void_p(t.data_ptr()), int(t.shape[0]), int(t.shape[1]),
                                             ctypes.byref(h)))
    return Preprocessed(pcs, h)


class _Marshalled:
    """A proof as the C ABI takes it: the eon_proof_lk, the arrays that back its pointers (kept alive
    here), and what verify_native reads off the proof and the verifier key on the way."""

    __slots__ = ("lk", "keep", "opening", "batched", "has_perm", "vk_w", "vk_bits", "vk_c")


def _bad_shape(why):
    return VerificationError("InvalidProofShape", why)


def _marshal_proof(prog, proof, preprocessed_vk) -> _Marshalled:
    """verify_native's marshalling, shared with verify_native_many: array shapes that do not fit the
    program raise InvalidProofShape here, before any C call."""
    bad_shape = _bad_shape

    def mat(a, cols):
        return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, cols))

    def pair(op, cols, what, width):
        """[values, witnesses] of one matrix at {zeta, zeta h} as (2, width, .) arrays"""
        if len(op.values) != 1 or len(op.values[0]) != 2 or len(op.witnesses) != 1 or len(op.witnesses[0]) != 2:
            raise bad_shape(f"{what}: one matrix opened at two points expected")
        v = [mat(x, 4) for x in op.values[0]]
        w = [mat(x, 8) for x in op.witnesses[0]]
        if any(x.shape[0] != width for x in v):
            raise bad_shape(f"{what}: opened widths {[x.shape[0] for x in v]}, expected {width}")
        nw = 1 if batched else width  # one witness per point in the batched mode
        if any(x.shape[0] != nw for x in w):
            raise bad_shape(f"{what}: {[x.shape[0] for x in w]} witnesses per point, the {opening} opening has {nw}")
        return np.ascontiguousarray(np.stack(v)), np.ascontiguousarray(np.stack(w))

    opening = getattr(proof, "opening", "per_column")
    if opening not in OPENING_MODES:
        raise bad_shape(f"unknown opening mode {opening!r}")
    batched = opening == "batched"
    has_perm = proof.permutation_commit is not None
    opened = list(proof.opened)
    if len(opened) < 2 + (1 if has_perm else 0) or len(opened) > 3 + (1 if has_perm else 0):
        raise bad_shape(f"{len(opened)} opening rounds")
    tc = mat(proof.trace_commit[0], 8)
    if tc.shape[0] != prog.width:
        raise bad_shape(f"trace commitment of {tc.shape[0]} columns, the AIR has {prog.width}")
    to, tw = pair(opened[0], 4, "trace", prog.width)
    mc = mo = mw = None
    if has_perm:
        mc = mat(proof.permutation_commit[0], 8)
        if mc.shape[0] != prog.permutation_width:
            raise bad_shape(f"permutation commitment of {mc.shape[0]} columns, the AIR has {prog.permutation_width}")
        mo, mw = pair(opened[1], 4, "permutation", prog.permutation_width)
    quot = opened[2 if has_perm else 1]
    chunks = 1 << prog.log_quotient_degree()
    qc = np.ascontiguousarray(np.stack([mat(c, 8) for c in proof.quotient_commit]).reshape(-1, 8)) \
        if len(proof.quotient_commit) else np.zeros((0, 8), np.uint64)
    if qc.shape[0] != chunks or len(quot.values) != chunks or len(quot.witnesses) != chunks:
        raise bad_shape(f"{qc.shape[0]} quotient chunk commitments, {len(quot.values)} opened, expected {chunks}")
    if any(len(v) != 1 or mat(v[0], 4).shape[0] != 1 for v in quot.values) or \
            any(len(w) != 1 or mat(w[0], 8).shape[0] != 1 for w in quot.witnesses):
        raise bad_shape("each quotient chunk is one column opened at one point")
    qo = np.ascontiguousarray(np.stack([mat(v[0], 4)[0] for v in quot.values]))
    qw = np.ascontiguousarray(np.stack([mat(w[0], 8)[0] for w in quot.witnesses]))
    vk_w = vk_bits = 0
    vk_c = None
    if preprocessed_vk is not None:
        if isinstance(preprocessed_vk, Preprocessed):
            vk_w, vk_bits, vk_c = preprocessed_vk.width, preprocessed_vk.degree_bits, preprocessed_vk.commitment
        else:
            vk_w, vk_bits, vk_c = preprocessed_vk
        vk_w, vk_bits = int(vk_w), int(vk_bits)
        vk_c = mat(vk_c, 8) if vk_w else np.zeros((1, 8), np.uint64)
        if vk_w and vk_c.shape[0] != vk_w:
            raise ValueError(f"the verifier key's commitment has {vk_c.shape[0]} columns, its width is {vk_w}")
    po = pw = None
    if len(opened) > (3 if has_perm else 2):  # the proof opens preprocessed columns
        # process_preprocessed_trace (verifier.rs:184-201): the expected width is the key's, else the AIR's
        expect = vk_w if preprocessed_vk is not None else prog.preprocessed_width
        po, pw = pair(opened[-1], 4, "preprocessed", expect)
    out = eon_proof(_p(tc), _p(qc), _p(to), _p(tw), _p(qo), _p(qw), int(proof.degree_bits))
    out_pp = eon_proof_pp(out, None, _p(po) if po is not None else None, _p(pw) if pw is not None else None)
    out_lk = eon_proof_lk(out_pp, _p(mc) if mc is not None else None, _p(mo) if mo is not None else None,
                          _p(mw) if mw is not None else None)
    m = _Marshalled()
    m.lk, m.keep = out_lk, (tc, qc, to, tw, qo, qw, po, pw, mc, mo, mw, vk_c)
    m.opening, m.batched, m.has_perm = opening, batched, has_perm
    m.vk_w, m.vk_bits, m.vk_c = vk_w, vk_bits, vk_c
    return m


def verify_native(prog, pcs: NativeKzgPcs, proof, public_values=(), challenger: Challenger | None = None,
                  preprocessed_vk=None, transcript: dict | None = None) -> None:
    """verify_with_preprocessed (eon-uni-stark/src/verifier.rs:244-502) through the C++ driver
    (eon_verify_air[_fs]).  `prog` is the air.AirProgram of the AIR (for a Poseidon2 proof of the
    fused kernel: AirProgram(Poseidon2Air), the same constraints in the same order); `proof` has
    prove_native's shape; `preprocessed_vk` is the verifier key, a Preprocessed or a
    (width, degree_bits, commitment) tuple -- its commitment is the one observed and checked, never
    the proof's copy.  With `challenger` the challenges are re-derived from the transcript and the
    challenger ends where the prover's did; without, proof.alpha, proof.zeta and
    proof.permutation_challenges are used.  `transcript` (a dict, optional) receives the alpha, zeta
    and permutation_challenges the verifier used.  Returns None when the proof is valid; raises
    VerificationError whose `.kind` names the reference's variant.  Array shapes that do not fit the
    program (opened widths, the chunk count, the permutation width, the key's width) raise
    InvalidProofShape before any C call."""
    if public_values is None:
        public_values = ()
    from .air import _publics_limbs

    m = _marshal_proof(prog, proof, preprocessed_vk)
    out_lk, opening, batched, has_perm = m.lk, m.opening, m.batched, m.has_perm
    vk_w, vk_bits, vk_c = m.vk_w, m.vk_bits, m.vk_c
    pub = _publics_limbs(public_values)
    npub = len(public_values)
    pcs.ctx.set_stream(None)
    res = _INT(-1)
    vkp = _p(vk_c) if vk_c is not None else None
    unm = lambda v: fr_unmont(sum(int(x) << (64 * i) for i, x in enumerate(v)))  # noqa: E731
    if challenger is None:
        chal = [int(c) for c in (proof.permutation_challenges or ())] if has_perm else []
        if len(chal) != (prog.num_challenges if has_perm else 0):
            raise _bad_shape(f"{len(chal)} permutation challenges, the AIR has {prog.num_challenges}")
        ch = _publics_limbs(chal)
        a, z = fr_to_abi(proof.alpha), fr_to_abi(proof.zeta)
        with pcs.opening_scope(opening, proof.gamma if batched else None, proof.delta if batched else None):
            pcs.check(pcs.lib.eon_verify_air(pcs._h, prog.handle, ctypes.byref(out_lk), _p(pub), npub, vk_w, vk_bits,
                                             vkp, _p(ch), len(chal), ctypes.byref(a), ctypes.byref(z),
                                             ctypes.byref(res)))
        used = {"alpha": proof.alpha, "zeta": proof.zeta, "permutation_challenges": chal}
    else:
        a_out, z_out = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
        c_out = np.zeros((max(1, prog.num_challenges), 4), np.uint64)
        with pcs.opening_scope(opening):
            pcs.check(pcs.lib.eon_verify_air_fs(pcs._h, prog.handle, ctypes.byref(out_lk), _p(pub), npub, vk_w,
                                                vk_bits, vkp, challenger.handle, ctypes.byref(res), _p(c_out),
                                                _p(a_out), _p(z_out)))
        used = {"alpha": unm(a_out), "zeta": unm(z_out),
                "permutation_challenges": [unm(c) for c in c_out[:prog.num_challenges]] if has_perm else []}
    if batched and res.value != 1:
        used["gamma"], used["delta"] = pcs.last_opening_challenges()
    if transcript is not None and res.value != 1:  # a shape rejection comes before the transcript
        transcript.update(used)
    if res.value != 0:
        raise VerificationError(VerificationError.KINDS[res.value], pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode())
    return None


def proof_shape(proof) -> eon_proof_shape:
    """The eon_proof_shape of a Proof, read off its arrays."""
    if proof.opening not in OPENING_MODES:
        raise ValueError(f"unknown opening mode {proof.opening!r}")
    has_perm = proof.permutation_commit is not None
    has_pre = len(proof.opened) > (3 if has_perm else 2)
    flags = (EON_PROOF_BATCHED if proof.opening == "batched" else 0) | (EON_PROOF_PREPROCESSED if has_pre else 0) | \
        (EON_PROOF_PERMUTATION if has_perm else 0)
    rows = lambda a: np.asarray(a).reshape(-1, 4).shape[0]  # noqa: E731
    return eon_proof_shape(flags, int(proof.degree_bits), np.asarray(proof.trace_commit[0]).reshape(-1, 8).shape[0],
                           len(proof.quotient_commit), rows(proof.opened[-1].values[0][0]) if has_pre else 0,
                           rows(proof.opened[1].values[0][0]) if has_perm else 0)


def _proof_arrays(shape: eon_proof_shape):
    """Zeroed arrays of a shape and the eon_proof_lk over them (the arrays keep it alive)."""
    batched = bool(shape.flags & EON_PROOF_BATCHED)
    w, c, wp, wq = shape.width, shape.chunks, shape.pre_width, shape.perm_width
    a = {"tc": np.zeros((w, 8), np.uint64), "qc": np.zeros((c, 8), np.uint64), "to": np.zeros((2, w, 4), np.uint64),
         "tw": np.zeros((2, 1 if batched else w, 8), np.uint64), "qo": np.zeros((c, 4), np.uint64),
         "qw": np.zeros((c, 8), np.uint64)}
    if wp:
        a["po"] = np.zeros((2, wp, 4), np.uint64)
        a["pw"] = np.zeros((2, 1 if batched else wp, 8), np.uint64)
    if wq:
        a["mc"] = np.zeros((wq, 8), np.uint64)
        a["mo"] = np.zeros((2, wq, 4), np.uint64)
        a["mw"] = np.zeros((2, 1 if batched else wq, 8), np.uint64)
    return a


def _proof_lk(a, degree_bits: int) -> eon_proof_lk:
    ptr = lambda k: _p(a[k]) if k in a else None  # noqa: E731
    base = eon_proof(_p(a["tc"]), _p(a["qc"]), _p(a["to"]), _p(a["tw"]), _p(a["qo"]), _p(a["qw"]), int(degree_bits))
    return eon_proof_lk(eon_proof_pp(base, None, ptr("po"), ptr("pw")), ptr("mc"), ptr("mo"), ptr("mw"))


def _proof_io_check(rc: int, rep: eon_proof_io_report, what: str):
    if rc == _lib.EON_E_FORMAT:
        raise ProofFormatError(int(rep.reason), int(rep.section), int(rep.index))
    _check(rc, what)


def proof_to_bytes(proof) -> bytes:
    """Proof.to_bytes: eon_proof_serialize over the proof's arrays (host only)."""
    lib = load()
    shape = proof_shape(proof)
    a = _proof_arrays(shape)
    has_perm, has_pre = "mc" in a, "po" in a

    def fill(dst, src, what):
        src = np.asarray(src, dtype=np.uint64)
        if src.size != dst.size:
            raise ValueError(f"{what}: {src.size // dst.shape[-1]} entries, the proof's shape has "
                             f"{dst.size // dst.shape[-1]}")
        dst[...] = src.reshape(dst.shape)

    def fill_pair(vals, wits, op, what):
        if len(op.values) != 1 or len(op.values[0]) != 2 or len(op.witnesses) != 1 or len(op.witnesses[0]) != 2:
            raise ValueError(f"{what}: one matrix opened at two points expected")
        for t in range(2):
            fill(vals[t], op.values[0][t], f"{what} values")
            fill(wits[t], op.witnesses[0][t], f"{what} witnesses")

    opened = list(proof.opened)
    fill(a["tc"], proof.trace_commit[0], "trace commitment")
    fill(a["qc"], np.stack([np.asarray(c, dtype=np.uint64).reshape(8) for c in proof.quotient_commit]),
         "quotient commitment")
    fill_pair(a["to"], a["tw"], opened[0], "trace")
    quot = opened[2 if has_perm else 1]
    if len(quot.values) != shape.chunks or len(quot.witnesses) != shape.chunks:
        raise ValueError(f"{len(quot.values)} quotient chunks opened, {shape.chunks} committed")
    fill(a["qo"], np.stack([np.asarray(v[0], dtype=np.uint64).reshape(4) for v in quot.values]), "quotient values")
    fill(a["qw"], np.stack([np.asarray(w[0], dtype=np.uint64).reshape(8) for w in quot.witnesses]),
         "quotient witnesses")
    if has_perm:
        fill(a["mc"], proof.permutation_commit[0], "permutation commitment")
        fill_pair(a["mo"], a["mw"], opened[1], "permutation")
    if has_pre:
        fill_pair(a["po"], a["pw"], opened[-1], "preprocessed")
    lk = _proof_lk(a, shape.degree_bits)
    size = lib.eon_proof_bytes_size(ctypes.byref(shape))
    if size == 0:
        raise ValueError("the proof's shape is not serialisable")
    out = np.zeros(size, np.uint8)
    written = _U64(0)
    _check(lib.eon_proof_serialize(ctypes.byref(lk), ctypes.byref(shape), _p(out), size, ctypes.byref(written)),
           "eon_proof_serialize")
    return out[:written.value].tobytes()


def proof_peek(data) -> eon_proof_shape:
    """eon_proof_peek: the shape in the header of proof bytes, after the header and length checks
    (host only).  Raises ProofFormatError."""
    lib = load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    shape, rep = eon_proof_shape(), eon_proof_io_report()
    _proof_io_check(lib.eon_proof_peek(_p(buf) if buf.size else None, buf.size, ctypes.byref(shape),
                                       ctypes.byref(rep)), rep, "eon_proof_peek")
    return shape


def proof_from_bytes(data, ctx: Context | None = None) -> Proof:
    """Proof.from_bytes: eon_proof_peek for the shape, then eon_proof_deserialize into fresh arrays."""
    lib = load()
    raw = bytes(data)
    shape = proof_peek(raw)
    ctx = ctx or default_context(0)
    buf = np.frombuffer(raw, dtype=np.uint8)
    a = _proof_arrays(shape)
    lk = _proof_lk(a, 0)
    rep = eon_proof_io_report()
    ctx.set_stream(None)
    rc = lib.eon_proof_deserialize(ctx.handle, _p(buf), buf.size, ctypes.byref(lk), ctypes.byref(rep))
    if rc not in (0, _lib.EON_E_FORMAT):
        ctx.check(rc)
    _proof_io_check(rc, rep, "eon_proof_deserialize")
    chunks = shape.chunks
    opened = [Opened(values=[[a["to"][0], a["to"][1]]], witnesses=[[a["tw"][0], a["tw"][1]]]),
              Opened(values=[[a["qo"][c:c + 1]] for c in range(chunks)],
                     witnesses=[[a["qw"][c:c + 1]] for c in range(chunks)])]
    if "mc" in a:
        opened.insert(1, Opened(values=[[a["mo"][0], a["mo"][1]]], witnesses=[[a["mw"][0], a["mw"][1]]]))
    if "po" in a:
        opened.append(Opened(values=[[a["po"][0], a["po"][1]]], witnesses=[[a["pw"][0], a["pw"][1]]]))
    return Proof([a["tc"]], [a["qc"][c:c + 1] for c in range(chunks)], opened, int(lk.pp.base.degree_bits),
                 permutation_commit=[a["mc"]] if "mc" in a else None,
                 opening="batched" if shape.flags & EON_PROOF_BATCHED else "per_column")


def verify_native_bytes(prog, pcs: NativeKzgPcs, data, public_values=(), challenger: Challenger | None = None,
                        preprocessed_vk=None, transcript: dict | None = None) -> None:
    """Proof.from_bytes(data) followed by verify_native: a proof that arrived as bytes.  The bytes
    carry no challenge, so a `challenger` is required.  ProofFormatError when the bytes do not
    deserialise (before any verification), VerificationError as verify_native."""
    if challenger is None:
        raise ValueError("proof bytes carry no challenges: verify them with a challenger")
    proof = proof_from_bytes(data, pcs.ctx)
    return verify_native(prog, pcs, proof, public_values, challenger, preprocessed_vk, transcript)


def verify_native_many(prog, pcs: NativeKzgPcs, proofs, public_values=None, challengers=None, preprocessed_vk=None,
                       transcripts=None) -> list:
    """verify_native over a batch of proofs of one AIR in one pass (eon_verify_air_many[_fs]): the
    host part of every proof on a few threads, every proof's openings as one segment of ONE
    segmented pairing check, ONE launch for the constraints at every zeta.  Entry i of the result is
    None for a valid proof, else the VerificationError verify_native would have raised for proof i
    alone -- the InvalidProofShape it raises before any C call included.  `public_values`: one
    sequence per proof (None: no public values); `challengers`: one Challenger per proof, each left
    where verify_native leaves it, or None for the challenges the proofs carry; `transcripts`: a list
    of dicts, entry i updated as verify_native's `transcript`.  `preprocessed_vk`: the verifier key
    of every proof, or a list with one key per proof.  Proofs are grouped by opening mode (and by
    key, when several are given), one C call per group.  What verify_native raises as an EonError (a
    zeta on the trace domain, a wrong public value count) is raised here for the whole batch, its
    message naming the proof's index in `proofs`.  An entry of `proofs` that is already an
    exception is passed through (verify_native_bytes_many)."""
    from .air import _publics_limbs

    n = len(proofs)
    if n == 0:
        return []
    publics = [()] * n if public_values is None else [() if p is None else p for p in public_values]
    if len(publics) != n or (challengers is not None and len(challengers) != n) or \
            (transcripts is not None and len(transcripts) != n):
        raise ValueError("one sequence of public values, one challenger and one transcript per proof")
    vks = list(preprocessed_vk) if isinstance(preprocessed_vk, list) else [preprocessed_vk] * n
    if len(vks) != n:
        raise ValueError("one verifier key per proof, or one for all")
    results: list = [None] * n
    live = {}
    chals = {}
    for i, proof in enumerate(proofs):
        if isinstance(proof, Exception):
            results[i] = proof
            continue
        try:
            m = _marshal_proof(prog, proof, vks[i])
            if challengers is None:
                chal = [int(c) for c in (proof.permutation_challenges or ())] if m.has_perm else []
                if len(chal) != (prog.num_challenges if m.has_perm else 0):
                    raise _bad_shape(f"{len(chal)} permutation challenges, the AIR has {prog.num_challenges}")
                chals[i] = chal
            live[i] = m
        except VerificationError as e:
            results[i] = e
    unm = lambda v: fr_unmont(sum(int(x) << (64 * i) for i, x in enumerate(v)))  # noqa: E731
    n_ch = prog.num_challenges
    pcs.ctx.set_stream(None)
    def checked(rc, idx):
        """pcs.check, with the "proof j:" of a C call's error turned into the caller's index"""
        try:
            pcs.check(rc)
        except _lib.EonError as e:
            import re

            msg = pcs.lib.eon_kzg_pcs_last_error(pcs._h).decode()
            raise _lib.EonError(e.code, re.sub(r"proof (\d+):", lambda g: f"proof {idx[int(g.group(1))]}:", msg,
                                               count=1)) from None

    groups = {}  # (opening mode, verifier key) -> the proofs of one C call, in order
    for i in live:
        groups.setdefault((live[i].opening, id(vks[i])), []).append(i)
    for (opening, _), idx in groups.items():
        k = len(idx)
        batched = opening == "batched"
        npub = len(publics[idx[0]])
        if any(len(publics[i]) != npub for i in idx):
            raise ValueError("every proof of a batch has the AIR's number of public values")
        lks = (eon_proof_lk * k)(*[live[i].lk for i in idx])
        pub = _publics_limbs([v for i in idx for v in publics[i]])
        first = live[idx[0]]
        vkp = _p(first.vk_c) if first.vk_c is not None else None
        res = np.full(k, -1, dtype=np.int32)
        if challengers is None:
            ch = _publics_limbs([v for i in idx for v in (chals[i] + [0] * (n_ch - len(chals[i])))])
            a = _publics_limbs([proofs[i].alpha for i in idx])
            z = _publics_limbs([proofs[i].zeta for i in idx])
            g = _publics_limbs([proofs[i].gamma for i in idx]) if batched else None
            d = _publics_limbs([proofs[i].delta for i in idx]) if batched else None
            with pcs.opening_scope(opening):
                checked(pcs.lib.eon_verify_air_many(pcs._h, prog.handle, lks, k, _p(pub), npub, first.vk_w,
                                                      first.vk_bits, vkp, _p(ch), n_ch, _p(a), _p(z),
                                                      _p(g) if batched else None, _p(d) if batched else None,
                                                      _p(res)), idx)
            used = [{"alpha": proofs[i].alpha, "zeta": proofs[i].zeta, "permutation_challenges": chals[i]}
                    for i in idx]
        else:
            handles = (ctypes.c_void_p * k)(*[challengers[i].handle for i in idx])
            a_out, z_out = np.zeros((k, 4), np.uint64), np.zeros((k, 4), np.uint64)
            c_out = np.zeros((k, max(1, n_ch), 4), np.uint64)
            with pcs.opening_scope(opening):
                checked(pcs.lib.eon_verify_air_many_fs(pcs._h, prog.handle, lks, k, _p(pub), npub, first.vk_w,
                                                         first.vk_bits, vkp, handles, _p(res),
                                                         _p(c_out.reshape(-1, 4)) if n_ch else None, _p(a_out),
                                                         _p(z_out)), idx)
            used = [{"alpha": unm(a_out[j]), "zeta": unm(z_out[j]),
                     "permutation_challenges": [unm(c) for c in c_out[j][:n_ch]] if live[i].has_perm else []}
                    for j, i in enumerate(idx)]
        for j, i in enumerate(idx):
            r = int(res[j])
            if batched and r != 1:
                g1, d1 = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
                _check(pcs.lib.eon_verify_many_opening_challenges(pcs._h, j, _p(g1), _p(d1)),
                       "eon_verify_many_opening_challenges")
                used[j]["gamma"], used[j]["delta"] = unm(g1), unm(d1)
            if transcripts is not None and r != 1:  # a shape rejection comes before the transcript
                transcripts[i].update(used[j])
            if r != 0:
                results[i] = VerificationError(VerificationError.KINDS[r],
                                               pcs.lib.eon_verify_many_detail(pcs._h, j).decode())
    return results


def verify_native_bytes_many(prog, pcs: NativeKzgPcs, blobs, public_values=None, challengers=None,
                             preprocessed_vk=None, transcripts=None) -> list:
    """verify_native_many on proofs that arrived as bytes: entry i is a ProofFormatError when blob i
    does not deserialise (that proof's challenger is left untouched), else as verify_native_many.
    The bytes carry no challenge, so the challengers are required."""
    if challengers is None:
        raise ValueError("proof bytes carry no challenges: verify them with challengers")
    proofs = []
    for data in blobs:
        try:
            proofs.append(proof_from_bytes(data, pcs.ctx))
        except ProofFormatError as e:
            proofs.append(e)
    return verify_native_many(prog, pcs, proofs, public_values, challengers, preprocessed_vk, transcripts)


def prove_native(air, pcs: NativeKzgPcs, trace, alpha: int | None, zeta: int | None,
                 max_constraint_degree: int = 3, collective=None, challenger: Challenger | None = None,
                 public_values=(), preprocessed: Preprocessed | None = None, permutation_challenges=None,
                 preprocessed_trace=None, opening: str = "per_column", gamma: int | None = None,
                 delta: int | None = None) -> Proof:
    """prover.prove through the C++ driver.  `air` is a Poseidon2Air (fused quotient kernel) or an
    air.AirProgram (any AIR, with `public_values`: canonical ints).  `trace`: (N, width, 4) device
    tensor.  With a collective (world > 1; TorchCollective or RcclCollective) every rank returns the
    full proof, equal to the one-device proof byte for byte.  Of a Poseidon2Air, `air`/`trace` are
    this rank's lanes.  An AirProgram is sharded by columns (eon_prove_air_sharded[_fs]): rank g
    owns the columns distributed.column_range(air.width, world, g), and `trace` is either that slice,
    (N, wl, 4), or the full (N, width, 4) trace, from which the rank's columns are copied out; any
    other width is a ValueError, more ranks than columns an EonError(EON_E_ARG) on every rank.  The
    ranks exchange their extended columns once as row blocks, each evaluates the quotient on its own
    rows, and the rest is sharded as for the lanes.  Preprocessed columns, lookups, the
    check_constraints switch and the batched opening are refused with a collective.  With `challenger` (eon_prove_*_fs) alpha and zeta are sampled from
    the transcript and returned in proof.alpha / proof.zeta (canonical ints); the arguments are
    ignored.  With `preprocessed` (setup_preprocessed; generic AIRs only) the proof carries its
    commitment and a third Opened entry, the preprocessed columns at zeta and zeta * h.  An
    AirProgram with lookups goes through eon_prove_air_lk[_fs]: `permutation_challenges` (canonical
    ints) are given next to alpha and zeta, or sampled with `challenger`; `preprocessed_trace` is
    the (N, Wp, 4) preprocessed trace itself when a lookup reads it.  The proof then carries
    permutation_commit and permutation_challenges, and its `opened` list has the permutation
    columns second (the reference's rounds: trace, permutation, quotient chunks, preprocessed).

    `opening` = "batched" (eon_kzg_pcs_set_opening, set for this call and restored) makes the
    standard batched KZG opening instead of the reference's per-column one: commitments and opened
    values are the same, every opened[r].witnesses[m][t] is ONE point, shape (1, 8).  Without a
    challenger `gamma` is required (EonError EON_E_ARG otherwise; `delta` is the verifier's and is
    carried in the Proof when given); with one both are sampled after zeta and returned in
    proof.gamma / proof.delta.  No collective (ValueError)."""
    from .air import AirProgram, _publics_limbs

    if opening not in OPENING_MODES:
        raise ValueError(f"opening must be one of {sorted(OPENING_MODES)}, not {opening!r}")
    batched = opening == "batched"
    if batched and collective is not None and collective.c.world > 1:
        raise ValueError("the batched opening is not sharded: prove without a collective")

    generic = isinstance(air, AirProgram)
    world = collective.c.world if collective is not None else 1
    # a program is sharded by columns (its width is the full one), the Poseidon2-AIR by lanes
    col_shard = generic and world > 1
    w = air.width if generic else air.width * world
    log_qd = air.log_quotient_degree() if generic else log_quotient_degree(max_constraint_degree)
    chunks = 1 << log_qd
    tc = np.zeros((w, 8), np.uint64)
    qc = np.zeros((chunks, 8), np.uint64)
    to = np.zeros((2, w, 4), np.uint64)
    tw = np.zeros((2, 1 if batched else w, 8), np.uint64)
    qo = np.zeros((chunks, 4), np.uint64)
    qw = np.zeros((chunks, 8), np.uint64)
    out = eon_proof(_p(tc), _p(qc), _p(to), _p(tw), _p(qo), _p(qw), 0)
    if preprocessed is not None:
        if not generic or collective is not None:
            raise ValueError("preprocessed columns need an AirProgram and no collective (they are not sharded)")
        wp = preprocessed.width
        pc = np.zeros((wp, 8), np.uint64)
        po = np.zeros((2, wp, 4), np.uint64)
        pw = np.zeros((2, 1 if batched else wp, 8), np.uint64)
        out_pp = eon_proof_pp(out, _p(pc), _p(po), _p(pw))
        out = out_pp.base  # a view: the driver's degree_bits and stage_ms land here
    lookups = generic and air.permutation_width > 0
    if lookups:
        if collective is not None:
            raise ValueError("lookups are not sharded: prove without a collective")
        wq = air.permutation_width
        mc = np.zeros((wq, 8), np.uint64)
        mo = np.zeros((2, wq, 4), np.uint64)
        mw = np.zeros((2, 1 if batched else wq, 8), np.uint64)
        if preprocessed is None:
            out_pp = eon_proof_pp(out, None, None, None)
        out_lk = eon_proof_lk(out_pp, _p(mc), _p(mo), _p(mw))
        out = out_lk.pp.base
    elif permutation_challenges is not None or preprocessed_trace is not None:
        raise ValueError("permutation_challenges / preprocessed_trace need an AirProgram with lookups")
    t = trace
    if col_shard:
        from .distributed import column_range

        if generic and pcs.check_constraints:
            raise ValueError("check_constraints is not column-sharded: switch it off or prove without a collective")
        c0, wl = column_range(air.width, world, collective.c.rank)
        if t.shape[1] == air.width:  # the full trace (also when wl == width cannot be: world > 1)
            t = t[:, c0:c0 + wl]
        elif t.shape[1] != wl:
            raise ValueError(f"the trace has {t.shape[1]} columns: rank {collective.c.rank} of {world} takes its "
                             f"slice of {wl} columns or the full width {air.width}")
    t = t.contiguous()
    import torch

    torch.cuda.synchronize(t.device)  # the trace was produced on torch's stream
    pcs.ctx.set_stream(None)
    coll = ctypes.byref(collective.c) if collective is not None else None
    pub = _publics_limbs(public_values)
    npub = len(public_values)
    if not generic and npub:
        raise ValueError("the Poseidon2-AIR has no public values")
    tp = ctypes.c_void_p(t.data_ptr())
    with pcs.opening_scope(opening, gamma, delta):
        if lookups:
            pt = preprocessed_trace.contiguous() if preprocessed_trace is not None else None
            ptp = ctypes.c_void_p(pt.data_ptr()) if pt is not None else None
            pph = preprocessed.handle if preprocessed is not None else None
            if challenger is None:
                a, z = fr_to_abi(alpha), fr_to_abi(zeta)
                chal = [int(c) for c in (permutation_challenges or ())]
                ch = _publics_limbs(chal)
                pcs.check(pcs.lib.eon_prove_air_lk(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub, pph, ptp,
                                                   _p(ch), len(chal), ctypes.byref(a), ctypes.byref(z),
                                                   ctypes.byref(out_lk)))
            else:
                a_out, z_out = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
                c_out = np.zeros((air.num_challenges, 4), np.uint64)
                pcs.check(pcs.lib.eon_prove_air_lk_fs(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub, pph, ptp,
                                                      challenger.handle, ctypes.byref(out_lk), _p(c_out), _p(a_out),
                                                      _p(z_out)))
                unm = lambda v: fr_unmont(sum(int(x) << (64 * i) for i, x in enumerate(v)))  # noqa: E731
                alpha, zeta, chal = unm(a_out), unm(z_out), [unm(c) for c in c_out]
        elif challenger is None:
            a, z = fr_to_abi(alpha), fr_to_abi(zeta)
            if preprocessed is not None:
                pcs.check(pcs.lib.eon_prove_air_pp(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub,
                                                   preprocessed.handle, ctypes.byref(a), ctypes.byref(z),
                                                   ctypes.byref(out_pp)))
            elif col_shard:
                pcs.check(pcs.lib.eon_prove_air_sharded(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub,
                                                        ctypes.byref(a), ctypes.byref(z), coll, ctypes.byref(out)))
            elif generic:
                pcs.check(pcs.lib.eon_prove_air(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub, ctypes.byref(a),
                                                ctypes.byref(z), ctypes.byref(out)))
            else:
                pcs.check(pcs.lib.eon_prove_p2air(pcs._h, air.handle, tp, int(t.shape[0]), ctypes.byref(a),
                                                  ctypes.byref(z), max_constraint_degree, coll, ctypes.byref(out)))
        else:
            a_out, z_out = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
            if preprocessed is not None:
                pcs.check(pcs.lib.eon_prove_air_pp_fs(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub,
                                                      preprocessed.handle, challenger.handle, ctypes.byref(out_pp),
                                                      _p(a_out), _p(z_out)))
            elif col_shard:
                pcs.check(pcs.lib.eon_prove_air_sharded_fs(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub,
                                                           challenger.handle, coll, ctypes.byref(out), _p(a_out),
                                                           _p(z_out)))
            elif generic:
                pcs.check(pcs.lib.eon_prove_air_fs(pcs._h, air.handle, tp, int(t.shape[0]), _p(pub), npub,
                                                   challenger.handle, ctypes.byref(out), _p(a_out), _p(z_out)))
            else:
                pcs.check(pcs.lib.eon_prove_p2air_fs(pcs._h, air.handle, tp, int(t.shape[0]), challenger.handle,
                                                     max_constraint_degree, coll, ctypes.byref(out), _p(a_out),
                                                     _p(z_out)))
            alpha = fr_unmont(sum(int(v) << (64 * i) for i, v in enumerate(a_out)))
            zeta = fr_unmont(sum(int(v) << (64 * i) for i, v in enumerate(z_out)))
    opened_trace = Opened(values=[[to[0], to[1]]], witnesses=[[tw[0], tw[1]]])
    opened_quot = Opened(values=[[qo[c:c + 1]] for c in range(chunks)], witnesses=[[qw[c:c + 1]] for c in range(chunks)])
    timings = {name: out.stage_ms[i] for i, name in enumerate(STAGES)}
    if collective is None:
        timings.pop("exchange partial quotients")
        timings.pop("assemble columns")
    opened = [opened_trace, opened_quot]
    if lookups:  # the permutation round comes before the quotient's (prover.rs:426-439)
        opened.insert(1, Opened(values=[[mo[0], mo[1]]], witnesses=[[mw[0], mw[1]]]))
    if preprocessed is not None:
        opened.append(Opened(values=[[po[0], po[1]]], witnesses=[[pw[0], pw[1]]]))
    if batched and challenger is not None:
        gamma, delta = pcs.last_opening_challenges()
    return Proof([tc], [qc[c:c + 1] for c in range(chunks)], opened, out.degree_bits, timings, alpha, zeta,
                 [pc] if preprocessed is not None else None, [mc] if lookups else None, chal if lookups else None,
                 opening, gamma if batched else None, delta if batched else None)
