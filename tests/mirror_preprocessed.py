"""CPU restatement of the Some(preprocessed) branch of eon-uni-stark's prove and verify over KzgPcs
(setup_preprocessed preprocessed.rs:47-94; prover.rs:190-208, 321-322, 426-439; verifier.rs:165-235,
357-366, 459-490), assembled only from the oracle modules.  TEST INFRASTRUCTURE ONLY.

An AIR is its constraints written out directly: fn(local, next, pre_local, pre_next, sels, publics)
-> the assert_zero values in eval order (tests/airs_preprocessed.py).  The quotient is the oracle's
quotient_values_fn over rows that are the main LDE row followed by the preprocessed LDE row, split
again at the main width."""

from types import SimpleNamespace

import numpy as np

from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V

P = O.P


def lim(x):
    return np.array(O.int_to_limbs(O.to_mont(x % P)), dtype=np.uint64)


def ints(a):
    return [O.from_mont(O.limbs_to_int([int(v) for v in e])) for e in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def to_limbs(rows):
    """canonical int rows -> (n, w, 4) Montgomery limbs"""
    return np.stack([np.stack([lim(v) for v in r]) for r in rows])


def _points(abi_rows):
    return [O.g1_from_bytes(np.ascontiguousarray(r, dtype=np.uint64).tobytes())
            for r in np.asarray(abi_rows, dtype=np.uint64).reshape(-1, 8)]


def split_fn(fn, width):
    """fn over the two matrices -> the oracle's constraint_fn over concatenated rows"""
    return lambda loc, nxt, sels, pub: fn(loc[:width], nxt[:width], loc[width:], nxt[width:], sels, pub)


def setup(pre, srs):
    """setup_preprocessed: KzgPcs::commit on the natural domain (coset_idft_batch with shift 1, one
    commit_column per column).  `pre`: (n, wp, 4) limbs."""
    n = pre.shape[0]
    coeffs = C.idft_batch(pre)
    return SimpleNamespace(width=pre.shape[1], degree_bits=n.bit_length() - 1, coeffs=coeffs,
                           commitment=C.g1_msm_columns(srs[:n], coeffs))


def observe_instance(challenger, log_n, trace_commit, pp_width, pp_commit, publics):
    """prover.rs:196-208 / verifier.rs:357-366: log_ext_degree, log_degree, the preprocessed width,
    the trace commitment, then the preprocessed commitment, then the public values."""
    for v in (log_n, log_n, pp_width):
        challenger.observe(v)
    challenger.observe_g1(_points(trace_commit))
    if pp_width > 0:
        challenger.observe_g1(_points(pp_commit))
    for v in publics:
        challenger.observe(v)


def prove(trace, pp, srs, fn, log_qd, publics=(), challenger=None, alpha=None, zeta=None):
    """prove_with_preprocessed with Some(pp).  trace: (n, w, 4) limbs.  Returns a proof in
    native.prove_native's shape (trace_commit, quotient_commit, opened[3], alpha, zeta,
    preprocessed_commit)."""
    n, w = trace.shape[0], trace.shape[1]
    log_n = n.bit_length() - 1
    assert pp.degree_bits == log_n
    coeffs = C.idft_batch(trace)
    trace_commit = C.g1_msm_columns(srs[:n], coeffs)
    if challenger is not None:
        observe_instance(challenger, log_n, trace_commit, pp.width, pp.commitment, publics)
        alpha = challenger.sample()
    g = lim(O.GENERATOR)
    lde = C.kzg_evaluations_on_domain(coeffs, log_n + log_qd, g)
    pre_lde = C.kzg_evaluations_on_domain(pp.coeffs, log_n + log_qd, g)
    rows = [ints(r) + ints(pr) for r, pr in zip(lde, pre_lde)]
    qv = np.stack([lim(v) for v in O.quotient_values_fn(rows, log_n, log_qd, split_fn(fn, w), alpha, list(publics))])
    chunks = 1 << log_qd
    g_q = O.two_adic_generator(log_n + log_qd)
    q_coeffs, quotient_commit = [], []
    for c in range(chunks):
        ev = np.ascontiguousarray(qv.reshape(n, chunks, 4)[:, c:c + 1, :])
        cc = C.coset_idft_batch(ev, lim(O.GENERATOR * pow(g_q, c, P) % P))
        q_coeffs.append(cc)
        quotient_commit.append(C.g1_msm(srs[:n], cc[:, 0]))
    if challenger is not None:
        challenger.observe_g1(_points(quotient_commit))
        zeta = challenger.sample()
    zeta_next = zeta * O.two_adic_generator(log_n) % P

    def open_matrix(cf, points):
        vals, wits = [], []
        for z in points:
            v, wt = C.open_columns(srs[:max(n - 1, 1)], cf, lim(z))
            vals.append(v)
            wits.append(wt)
        return SimpleNamespace(values=[vals], witnesses=[wits])

    # the rounds in the reference's order: trace, quotient chunks, preprocessed (prover.rs:426-439)
    tr = open_matrix(coeffs, [zeta, zeta_next])
    qs = [open_matrix(cc, [zeta]) for cc in q_coeffs]
    qo = SimpleNamespace(values=[q.values[0] for q in qs], witnesses=[q.witnesses[0] for q in qs])
    po = open_matrix(pp.coeffs, [zeta, zeta_next])
    return SimpleNamespace(trace_commit=[trace_commit], quotient_commit=[c.reshape(1, 8) for c in quotient_commit],
                           opened=[tr, qo, po], degree_bits=log_n, alpha=alpha, zeta=zeta,
                           preprocessed_commit=[pp.commitment], quotient_values=qv)


def verify(proof, vk_commit, vk_width, fn, log_n, log_qd, srs_alpha, challenger=None, alpha=None, zeta=None,
           trace=None, pre=None, publics=(), seed=2024):
    """verify_with_preprocessed against the SETUP's commitment `vk_commit` (the verifier key's,
    verifier.rs:165-235), never the proof's copy.  The three checks of verify_kzg_proof with the
    preprocessed openings among the claims; with `trace` / `pre` (limbs) also the opened values
    against the matrices themselves."""
    tc = np.asarray(proof.trace_commit[0], dtype=np.uint64).reshape(-1, 8)
    qc = np.stack([np.asarray(c, dtype=np.uint64).reshape(8) for c in proof.quotient_commit])
    pc = np.asarray(vk_commit, dtype=np.uint64).reshape(-1, 8)
    assert pc.shape[0] == vk_width
    w = tc.shape[0]
    res = {}
    if challenger is not None:
        observe_instance(challenger, log_n, tc, vk_width, pc, publics)
        alpha = challenger.sample()
        challenger.observe_g1(_points(qc))
        zeta = challenger.sample()
        res["transcript"] = (proof.alpha, proof.zeta) == (alpha, zeta)
    zeta_next = zeta * O.two_adic_generator(log_n) % P
    tr, qo, po = proof.opened
    local, nxt = ints(tr.values[0][0]), ints(tr.values[0][1])
    plocal, pnxt = ints(po.values[0][0]), ints(po.values[0][1])
    qvals = [ints(qo.values[c][0])[0] for c in range(len(qo.values))]
    res["ood"] = V.ood_check(lambda loc, nx, sels: fn(loc[:w], nx[:w], loc[w:], nx[w:], sels[:3], list(publics)),
                             local + plocal, nxt + pnxt, qvals, alpha, zeta, log_n, log_qd)
    claims = []
    for opened, commit, vals_at in ((tr, tc, (local, nxt)), (po, pc, (plocal, pnxt))):
        for p, z in enumerate((zeta, zeta_next)):
            wits = np.asarray(opened.witnesses[0][p]).reshape(-1, 8)
            for c in range(commit.shape[0]):
                claims.append((commit[c], z, vals_at[p][c], wits[c]))
    for c in range(len(qvals)):
        claims.append((qc[c], zeta, qvals[c], np.asarray(qo.witnesses[c][0]).reshape(-1, 8)[0]))
    extra = []
    if trace is not None:
        ok = True
        pts = np.stack([lim(zeta), lim(zeta_next), lim(srs_alpha)])
        for mat, opened, commit in ((trace, tr, tc), (pre, po, pc)):
            ev = C.bary_eval_cols(np.ascontiguousarray(mat, dtype=np.uint64), pts)
            ok = ok and all(np.array_equal(ev[p], np.asarray(opened.values[0][p]).reshape(-1, 4)) for p in range(2))
            extra += [(commit[c], V.fr_int(ev[2][c])) for c in range(commit.shape[0])]
        res["opened_vs_trace"] = bool(ok)
    res["kzg"] = V.kzg_claims_identity(claims, srs_alpha, seed, extra)
    return res
