"""Host-side mirror of the Poseidon2-AIR and eon-uni-stark's quotient over the C ABI.

* ``Poseidon2Air``      -- Poseidon2Air / VectorizedPoseidon2Air (poseidon2-air/src/air.rs,
                           vectorized.rs) for BN254 (width 3, x^5, one register):
                           ``generate_trace`` (generation.rs) and ``quotient_values``
                           (eon-uni-stark/src/prover.rs:539-709) on device-resident matrices.
* ``selectors_on_coset`` -- commit/src/domain.rs:252-292.

Device matrices are torch CUDA int64 tensors of shape (rows, cols, 4) (Fr Montgomery limbs).
"""

from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from . import _lib
from .dft import Context, default_context
from .field import fr_to_abi


def _dp(t):
    return ctypes.c_void_p(t.data_ptr())


class Poseidon2Air:
    def __init__(self, begin, partial, end, vector_len: int = 1, ctx: Context | None = None):
        """begin/end: (half_full_rounds, 3, 4) u64 limbs; partial: (partial_rounds, 4)."""
        self.ctx = ctx or default_context(0)
        self._b = np.ascontiguousarray(begin, dtype=np.uint64).reshape(-1, 3, 4)
        self._p = np.ascontiguousarray(partial, dtype=np.uint64).reshape(-1, 4)
        self._e = np.ascontiguousarray(end, dtype=np.uint64).reshape(-1, 3, 4)
        k = _lib.eon_poseidon2_constants(self._b.shape[0], self._p.shape[0],
                                         self._b.ctypes.data_as(ctypes.c_void_p),
                                         self._p.ctypes.data_as(ctypes.c_void_p),
                                         self._e.ctypes.data_as(ctypes.c_void_p))
        h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.eon_p2air_create(self.ctx.handle, ctypes.byref(k), vector_len, ctypes.byref(h)))
        self._h = h
        self.vector_len = vector_len
        self.width = int(self.ctx.lib.eon_p2air_width(h))
        self.constraints_per_perm = 12 * self._b.shape[0] + 2 * self._p.shape[0]

    @property
    def handle(self):
        return self._h

    def _stream(self, t):
        import torch

        self.ctx.set_stream(torch.cuda.current_stream(t.device).cuda_stream)

    def generate_trace(self, inputs):
        """inputs: (n_perms, 3, 4) device tensor -> (n_perms / VECTOR_LEN, width, 4) trace."""
        import torch

        n = inputs.shape[0]
        out = torch.empty((n // self.vector_len, self.width, 4), dtype=torch.int64, device=inputs.device)
        self._stream(inputs)
        self.ctx.check(self.ctx.lib.eon_p2air_generate_trace_dev(self.ctx.handle, self._h, _dp(inputs.contiguous()),
                                                                 n, _dp(out)))
        return out

    def quotient_values(self, lde, log_n: int, log_qd: int, alpha):
        """quotient_values on the trace's LDE over GENERATOR * K (natural order)."""
        import torch

        q = 1 << (log_n + log_qd)
        out = torch.empty((q, 4), dtype=torch.int64, device=lde.device)
        a = fr_to_abi(alpha)
        self._stream(lde)
        self.ctx.check(self.ctx.lib.eon_p2air_quotient_values_dev(self.ctx.handle, self._h, _dp(lde.contiguous()),
                                                                  log_n, log_qd, ctypes.byref(a), _dp(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.ctx.lib.eon_p2air_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- the same AIR through the generic path: EonAir::eval on a symbolic builder -------------
    def num_public_values(self) -> int:
        return 0

    def eval(self, builder):
        """Poseidon2Air::eval (poseidon2-air/src/air.rs:108-166) on the symbolic builder, lanes in
        order (vectorized.rs:259-274): the initial external layer, full rounds (eval_full_round
        :200-221: add round constant, eval_sbox :253-288 with one committed x^3 register, external
        layer, assert_eq(state, post) then state = post), partial rounds (eval_partial_round
        :224-243: only state[0] through the S-box, internal layer).  The export column is
        unconstrained."""
        from .field import limbs_to_ints
        from .symbolic import SymbolicExpression

        E = SymbolicExpression.lift
        hf, pr = self._b.shape[0], self._p.shape[0]
        begin = [limbs_to_ints(self._b[r]) for r in range(hf)]
        partial = limbs_to_ints(self._p)
        end = [limbs_to_ints(self._e[r]) for r in range(hf)]
        nc = 4 + 12 * hf + 2 * pr
        local = builder.main()[0]

        def ext(s):  # mds_light width 3 (poseidon2/src/external.rs:128-133)
            t = s[0] + s[1] + s[2]
            return [s[0] + t, s[1] + t, s[2] + t]

        def internal(s):  # [2,1,1;1,2,1;1,1,3] (bn254/src/poseidon2.rs:55-63)
            t = s[0] + s[1] + s[2]
            return [s[0] + t, s[1] + t, s[2].double() + t]

        def sbox(x, x3):  # eval_sbox, degree 5 with one register: x3 = x^3, out = x3 * x^2
            x2 = x.square()
            builder.assert_eq(x3, x2 * x)
            return x3 * x2

        for v in range(self.vector_len):
            row = local[v * nc:(v + 1) * nc]
            s = ext([E(row[1]), E(row[2]), E(row[3])])
            k = 4

            def full(s, rc, k):
                s = [sbox(s[i] + rc[i], row[k + i]) for i in range(3)]
                s = ext(s)
                for i in range(3):
                    builder.assert_eq(s[i], row[k + 3 + i])
                return [E(row[k + 3 + i]) for i in range(3)], k + 6

            for rc in begin:
                s, k = full(s, rc, k)
            for rc in partial:
                x = sbox(s[0] + rc, row[k])
                builder.assert_eq(x, row[k + 1])
                s = internal([E(row[k + 1]), s[1], s[2]])
                k += 2
            for rc in end:
                s, k = full(s, rc, k)


@dataclasses.dataclass
class ConstraintReport:
    """eon_constraint_report (include/eon.h): what check_constraints found.  `row`, `constraint`
    and `value` (canonical int) describe the reference's first failure and are zero when
    `failures` is; `counts[k]` = rows on which constraint k fails (when asked for)."""

    failures: int
    row: int
    constraint: int
    value: int
    failing_constraints: int
    counts: list | None = None

    @classmethod
    def from_abi(cls, rep, counts=None) -> "ConstraintReport":
        from .field import fr_unmont

        v = sum(int(x) << (64 * i) for i, x in enumerate(rep.value.l))
        return cls(int(rep.failures), int(rep.row), int(rep.constraint), fr_unmont(v),
                   int(rep.failing_constraints), counts)


class AirProgram:
    """An AIR compiled for the generic quotient path (eon_air_program, include/eon.h): the
    constraint DAG get_symbolic_constraints returns (symbolic.py) -> device program.

    ``air`` is any object with ``width()``, ``num_public_values()`` and ``eval(builder)`` on the
    EonAirBuilder surface (symbolic.SymbolicAirBuilder).  An AIR with preprocessed columns
    (``builder.preprocessed()``) also has ``preprocessed_width()``, or the width is given here;
    their LDE is then a second matrix of ``quotient_values``.  An AIR with lookups has
    ``get_lookups()`` (symbolic.Lookup, symbolic.register_lookup): the LogUp constraints follow its
    own, the program reads ``permutation_width`` running-sum columns (a third matrix) and
    ``num_challenges`` challenges, and ``lookup_permutation`` generates the permutation trace."""

    def __init__(self, air, ctx: Context | None = None, preprocessed_width: int | None = None,
                 permutation_width: int | None = None):
        from . import symbolic

        self.ctx = ctx or default_context(0)
        self.air = air
        self.n_public = int(air.num_public_values())
        self.width = symbolic.air_width(air)
        if preprocessed_width is None:
            preprocessed_width = air.preprocessed_width() if hasattr(air, "preprocessed_width") else 0
        self.preprocessed_width = int(preprocessed_width)
        gadget = symbolic.LogUpGadget
        # an AIR without lookups may still read permutation columns and challenges it declares
        # itself (permutation_width here or as a method): a program for quotient_values only
        if permutation_width is None:
            permutation_width = air.permutation_width() if hasattr(air, "permutation_width") else 0
        cs, lookups, terms = symbolic.get_symbolic_constraints_and_lookups(
            air, self.preprocessed_width, self.n_public, int(permutation_width),
            int(permutation_width) * gadget.num_challenges)
        if lookups:
            permutation_width = len(lookups) * gadget.num_aux_cols
        self.permutation_width = int(permutation_width)
        self.num_challenges = self.permutation_width * gadget.num_challenges
        # the constraints and the lookup terms as one DAG: the denominators are shared nodes
        flat = [e for tl in terms for pair in tl for e in pair]
        nodes, consts, roots = symbolic.serialize(list(cs) + flat)
        roots, term_roots = roots[:len(cs)], roots[len(cs):]
        self.num_nodes = len(nodes)
        na = (_lib.eon_sym_node * max(1, len(nodes)))(*[_lib.eon_sym_node(*n) for n in nodes])
        from .field import ints_to_limbs

        ca = np.ascontiguousarray(ints_to_limbs(consts) if consts else np.zeros((1, 4), np.uint64))
        ra = np.ascontiguousarray(np.array(roots if roots else [0], dtype=np.uint32))
        h = ctypes.c_void_p()
        if self.permutation_width == 0:
            self.ctx.check(self.ctx.lib.eon_air_program_create_pp(
                self.ctx.handle, na, len(nodes), ca.ctypes.data_as(ctypes.c_void_p), len(consts),
                ra.ctypes.data_as(ctypes.c_void_p), len(roots), self.width, self.preprocessed_width, self.n_public,
                ctypes.byref(h)))
        else:
            la = (_lib.eon_lookup_desc * max(1, len(lookups)))(*[_lib.eon_lookup_desc(lk.columns[0], len(tl))
                                                         for lk, tl in zip(lookups, terms)])
            nt = len(term_roots) // 2
            ta = (_lib.eon_lookup_term * max(1, nt))(*[_lib.eon_lookup_term(term_roots[2 * t], term_roots[2 * t + 1])
                                                       for t in range(nt)])
            self.ctx.check(self.ctx.lib.eon_air_program_create_lk(
                self.ctx.handle, na, len(nodes), ca.ctypes.data_as(ctypes.c_void_p), len(consts),
                ra.ctypes.data_as(ctypes.c_void_p), len(roots), self.width, self.preprocessed_width, self.n_public,
                self.permutation_width, self.num_challenges, la, len(lookups), ta, ctypes.byref(h)))
        self._h = h
        st = _lib.eon_air_program_stats()
        self.ctx.check(self.ctx.lib.eon_air_program_info(h, ctypes.byref(st)))
        self.stats = {k: int(getattr(st, k)) for k, _ in st._fields_}
        self.max_constraint_degree = self.stats["max_constraint_degree"]
        self.num_constraints = self.stats["num_constraints"]

    @property
    def handle(self):
        return self._h

    def log_quotient_degree(self, is_zk: int = 0) -> int:
        return int(self.ctx.lib.eon_air_program_log_quotient_degree(self._h, is_zk))

    def lookup_permutation(self, trace, challenges, publics=(), preprocessed_trace=None):
        """LogUpGadget::generate_permutation (logup.rs:379-562) on the device: `trace` (N, width, 4),
        `challenges` num_challenges canonical ints, `preprocessed_trace` (N, preprocessed_width, 4)
        on the trace domain when a lookup reads it -> the (N, permutation_width, 4) running sums."""
        import torch

        n = int(trace.shape[0])
        out = torch.empty((n, self.permutation_width, 4), dtype=torch.int64, device=trace.device)
        pub = _publics_limbs(publics)
        ch = _publics_limbs(challenges)
        pre = None
        if preprocessed_trace is not None:
            pre = preprocessed_trace.contiguous()
            if pre.device != trace.device or tuple(pre.shape) != (n, self.preprocessed_width, 4):
                raise ValueError(f"preprocessed_trace must be ({n}, {self.preprocessed_width}, 4) on {trace.device}")
        self.ctx.set_stream(torch.cuda.current_stream(trace.device).cuda_stream)
        self.ctx.check(self.ctx.lib.eon_lookup_permutation_dev(
            self.ctx.handle, self._h, _dp(trace.contiguous()), _dp(pre) if pre is not None else None, n,
            pub.ctypes.data_as(ctypes.c_void_p), len(publics), ch.ctypes.data_as(ctypes.c_void_p), len(challenges),
            _dp(out)))
        return out

    def check_constraints(self, trace, publics=(), preprocessed_trace=None, permutation_trace=None, challenges=(),
                          per_constraint: bool = False) -> "ConstraintReport":
        """check_constraints (eon-uni-stark/src/check_constraints.rs:22-101) on the device: every row
        of `trace` (N, width, 4) with its successor (wrapping), `preprocessed_trace` (N,
        preprocessed_width, 4) and `permutation_trace` (N, permutation_width, 4) on the same trace
        domain, the 0 / 1 row selectors, `publics` and `challenges` as canonical ints.  Returns the
        reference's first failure (lowest row, then lowest constraint in assert order) with its
        value, and the counts; `per_constraint`: also the rows on which each constraint fails."""
        import torch

        n = int(trace.shape[0])
        mats = []
        for name, m, w in (("preprocessed_trace", preprocessed_trace, self.preprocessed_width),
                           ("permutation_trace", permutation_trace, self.permutation_width)):
            if m is not None:
                m = m.contiguous()
                if m.device != trace.device or tuple(m.shape) != (n, w, 4):
                    raise ValueError(f"{name} must be ({n}, {w}, 4) on {trace.device}")
            mats.append(m)
        pub = _publics_limbs(publics)
        ch = _publics_limbs(challenges)
        counts = np.zeros(max(1, self.num_constraints), np.uint32) if per_constraint else None
        rep = _lib.eon_constraint_report()
        self.ctx.set_stream(torch.cuda.current_stream(trace.device).cuda_stream)
        self.ctx.check(self.ctx.lib.eon_check_constraints_dev(
            self.ctx.handle, self._h, _dp(trace.contiguous()), _dp(mats[0]) if mats[0] is not None else None,
            _dp(mats[1]) if mats[1] is not None else None, n, pub.ctypes.data_as(ctypes.c_void_p), len(publics),
            ch.ctypes.data_as(ctypes.c_void_p), len(challenges),
            counts.ctypes.data_as(ctypes.c_void_p) if counts is not None else None, ctypes.byref(rep)))
        return ConstraintReport.from_abi(rep, [int(c) for c in counts[:self.num_constraints]]
                                         if counts is not None else None)

    def eval_at_point(self, log_n: int, zeta, alpha, local, next, publics=(), preprocessed_local=None,
                      preprocessed_next=None, permutation_local=None, permutation_next=None, challenges=()):
        """The constraints at one out-of-domain point (verify_constraints, verifier.rs:101-152) on
        the device: `local` / `next` (width, 4) device tensors of opened values (the trace at zeta and
        zeta h), the preprocessed and permutation pairs likewise, the selectors
        selectors_at_point(zeta) of the trace domain of size 2^log_n, every constraint folded as
        acc = acc alpha + C.  `zeta`, `alpha`, `publics`, `challenges`: canonical ints.  Returns
        (folded, folded * inv_vanishing) as canonical ints; the second is what the verifier compares
        with quotient(zeta).  zeta = 1, zeta = h^-1 or Z_H(zeta) = 0 is EON_E_ARG."""
        import torch

        from .field import fr_unmont

        rows = []
        for name, m, w in (("local", local, self.width), ("next", next, self.width),
                           ("preprocessed_local", preprocessed_local, self.preprocessed_width),
                           ("preprocessed_next", preprocessed_next, self.preprocessed_width),
                           ("permutation_local", permutation_local, self.permutation_width),
                           ("permutation_next", permutation_next, self.permutation_width)):
            if m is not None:
                m = m.contiguous()
                if m.device != local.device or tuple(m.shape) != (w, 4):
                    raise ValueError(f"{name} must be ({w}, 4) on {local.device}")
            rows.append(m)
        z, a = fr_to_abi(zeta), fr_to_abi(alpha)
        pub = _publics_limbs(publics)
        ch = _publics_limbs(challenges)
        out = np.zeros((2, 4), np.uint64)
        self.ctx.set_stream(torch.cuda.current_stream(local.device).cuda_stream)
        self.ctx.check(self.ctx.lib.eon_air_eval_at_point_dev(
            self.ctx.handle, self._h, log_n, ctypes.byref(z), ctypes.byref(a),
            *[_dp(m) if m is not None else None for m in rows], pub.ctypes.data_as(ctypes.c_void_p), len(publics),
            ch.ctypes.data_as(ctypes.c_void_p), len(challenges), out.ctypes.data_as(ctypes.c_void_p)))
        return tuple(fr_unmont(sum(int(x) << (64 * i) for i, x in enumerate(v))) for v in out)

    def eval_at_points(self, log_ns, zetas, alphas, rows, publics=None, challenges=None):
        """eval_at_point for n proofs in one launch (eon_air_eval_at_points_dev).  `rows`: an
        (n, row_stride, 4) device tensor, row i = proof i's opened values local | next |
        preprocessed_local | preprocessed_next | permutation_local | permutation_next; `log_ns`,
        `zetas`, `alphas`: n canonical ints each; `publics` / `challenges`: per proof a sequence of the
        program's public values / challenges (None when the program has none).  Returns a list of n
        pairs, each what eval_at_point returns for that proof."""
        import torch

        from .field import fr_unmont

        n = len(zetas)
        if len(log_ns) != n or len(alphas) != n:
            raise ValueError("one log_n and one alpha per zeta")
        publics = [()] * n if publics is None else list(publics)
        challenges = [()] * n if challenges is None else list(challenges)
        if len(publics) != n or len(challenges) != n:
            raise ValueError("one sequence of public values and of challenges per proof")
        n_ch = len(challenges[0]) if n else 0
        if any(len(p) != self.n_public for p in publics) or any(len(c) != n_ch for c in challenges):
            raise ValueError("every proof needs the program's public values and the same number of challenges")
        if n == 0:
            return []
        rows = rows.contiguous()
        if rows.dim() != 3 or rows.shape[0] != n or rows.shape[2] != 4:
            raise ValueError(f"rows must be ({n}, row_stride, 4)")
        lg = np.asarray(log_ns, dtype=np.uint32)
        z = _publics_limbs(zetas)
        a = _publics_limbs(alphas)
        def flat(seqs):  # per proof canonical ints, or (k, 4) Montgomery limbs
            if seqs and isinstance(seqs[0], np.ndarray) and seqs[0].ndim == 2:
                return np.concatenate(seqs)
            return [v for s in seqs for v in s]

        pub = _publics_limbs(flat(publics))
        ch = _publics_limbs(flat(challenges))
        out = np.zeros((2 * n, 4), np.uint64)
        self.ctx.set_stream(torch.cuda.current_stream(rows.device).cuda_stream)
        self.ctx.check(self.ctx.lib.eon_air_eval_at_points_dev(
            self.ctx.handle, self._h, n, *[x.ctypes.data_as(ctypes.c_void_p) for x in (lg, z, a)], _dp(rows),
            int(rows.shape[1]), pub.ctypes.data_as(ctypes.c_void_p), ch.ctypes.data_as(ctypes.c_void_p), n_ch,
            out.ctypes.data_as(ctypes.c_void_p)))
        vals = [fr_unmont(sum(int(x) << (64 * i) for i, x in enumerate(v))) for v in out]
        return [(vals[2 * i], vals[2 * i + 1]) for i in range(n)]

    def quotient_values(self, lde, log_n: int, log_qd: int, alpha, publics=(), preprocessed_lde=None,
                        permutation_lde=None, challenges=()):
        """quotient_values (prover.rs:539-709) on the trace's LDE over GENERATOR * K (natural);
        `preprocessed_lde`: the preprocessed trace on the same domain, (Q, preprocessed_width, 4);
        `permutation_lde`: the permutation trace likewise, (Q, permutation_width, 4), with the
        permutation `challenges` (canonical ints)."""
        import torch

        from .field import fr_to_abi

        q = 1 << (log_n + log_qd)
        out = torch.empty((q, 4), dtype=torch.int64, device=lde.device)
        a = fr_to_abi(alpha)
        pub = _publics_limbs(publics)
        self.ctx.set_stream(torch.cuda.current_stream(lde.device).cuda_stream)
        if permutation_lde is not None or len(challenges):
            mats = []
            for name, m, w in (("preprocessed_lde", preprocessed_lde, self.preprocessed_width),
                               ("permutation_lde", permutation_lde, self.permutation_width)):
                if m is not None:
                    m = m.contiguous()
                    if m.device != lde.device or tuple(m.shape) != (q, w, 4):
                        raise ValueError(f"{name} must be ({q}, {w}, 4) on {lde.device}")
                mats.append(m)
            ch = _publics_limbs(challenges)
            self.ctx.check(self.ctx.lib.eon_quotient_values_lk_dev(
                self.ctx.handle, self._h, _dp(lde.contiguous()), _dp(mats[0]) if mats[0] is not None else None,
                _dp(mats[1]) if mats[1] is not None else None, log_n, log_qd, ctypes.byref(a),
                pub.ctypes.data_as(ctypes.c_void_p), len(publics), ch.ctypes.data_as(ctypes.c_void_p),
                len(challenges), _dp(out)))
            return out
        if preprocessed_lde is None:
            self.ctx.check(self.ctx.lib.eon_quotient_values_dev(
                self.ctx.handle, self._h, _dp(lde.contiguous()), log_n, log_qd, ctypes.byref(a),
                pub.ctypes.data_as(ctypes.c_void_p), len(publics), _dp(out)))
            return out
        pre = preprocessed_lde.contiguous()
        if pre.device != lde.device or tuple(pre.shape) != (q, self.preprocessed_width, 4):
            raise ValueError(f"preprocessed_lde must be ({q}, {self.preprocessed_width}, 4) on {lde.device}")
        self.ctx.check(self.ctx.lib.eon_quotient_values_pp_dev(
            self.ctx.handle, self._h, _dp(lde.contiguous()), _dp(pre), log_n, log_qd, ctypes.byref(a),
            pub.ctypes.data_as(ctypes.c_void_p), len(publics), _dp(out)))
        return out

    def quotient_values_rows(self, window, log_n: int, row0: int, n_rows: int, alpha, public_values=()):
        """quotient_values on quotient-domain rows [row0, row0 + n_rows) alone, from a window of
        the LDE (eon_quotient_values_rows_dev): `window` holds the n_rows + 2^log_qd LDE rows
        (row0 + j) mod Q, j < n_rows + 2^log_qd, as (n_rows + 2^log_qd, width, 4).  Returns
        (n_rows, 4): rows row0.. of quotient_values' output, bit for bit.  What a rank of the
        column-sharded prove runs on its own rows (distributed.shard_row_range)."""
        import torch

        from .field import fr_to_abi

        log_qd = self.log_quotient_degree()
        rows = n_rows + (1 << log_qd)
        w = window.contiguous()
        if tuple(w.shape) != (rows, self.width, 4):
            raise ValueError(f"window must be ({rows}, {self.width}, 4): n_rows + 2^log_qd rows of the AIR's width")
        out = torch.empty((n_rows, 4), dtype=torch.int64, device=w.device)
        a = fr_to_abi(alpha)
        pub = _publics_limbs(public_values)
        self.ctx.set_stream(torch.cuda.current_stream(w.device).cuda_stream)
        self.ctx.check(self.ctx.lib.eon_quotient_values_rows_dev(
            self.ctx.handle, self._h, _dp(w), log_n, log_qd, row0, n_rows, ctypes.byref(a),
            pub.ctypes.data_as(ctypes.c_void_p), len(public_values), _dp(out)))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.ctx.lib.eon_air_program_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _publics_limbs(publics) -> np.ndarray:
    """canonical ints (or (n, 4) Montgomery limbs) -> contiguous (max(n,1), 4) u64 limbs"""
    from .field import ints_to_limbs

    if len(publics) == 0:
        return np.zeros((1, 4), np.uint64)
    if isinstance(publics, np.ndarray) and publics.ndim == 2:
        return np.ascontiguousarray(publics, dtype=np.uint64)
    return np.ascontiguousarray(ints_to_limbs([int(x) for x in publics]))


def selectors_on_coset(log_n: int, log_q: int, shift, device=0, ctx: Context | None = None):
    """-> (4, 2^log_q, 4) device tensor: is_first_row, is_last_row, is_transition, inv_vanishing."""
    import torch

    ctx = ctx or default_context(device)
    out = torch.empty((4, 1 << log_q, 4), dtype=torch.int64, device=f"cuda:{device}")
    s = fr_to_abi(shift)
    ctx.set_stream(torch.cuda.current_stream(out.device).cuda_stream)
    ctx.check(ctx.lib.eon_selectors_on_coset_dev(ctx.handle, log_n, log_q, ctypes.byref(s), _dp(out)))
    return out
