"""CPU restatement of the lookup branch of eon-uni-stark's prove and verify over KzgPcs
(prover.rs:90-95, 210-278, 317-319, 427-437; verifier.rs:354-473; generate_permutation,
lookup/src/logup.rs:379-562), assembled only from the oracle modules in the manner of
tests/mirror_preprocessed.py.  TEST INFRASTRUCTURE ONLY.

An AIR is its constraints written out directly,
fn(local, next, pre_local, pre_next, perm_local, perm_next, sels, publics, challenges), and its
lookup terms, terms(local, next, pre_local, pre_next, publics, challenges) (tests/airs_lookup.py).
The quotient is the oracle's quotient_values_fn over rows that are the main LDE row followed by the
preprocessed and the permutation LDE rows, split again at the widths, with the challenges closed
over."""

from types import SimpleNamespace

import numpy as np

import mirror_preprocessed as MP
from oracle import coracle as C
from oracle import pyoracle as O
from oracle import verify_oracle as V

P = O.P
lim, ints, to_limbs, _points, setup = MP.lim, MP.ints, MP.to_limbs, MP._points, MP.setup


def split_fn(fn, w, wp, challenges):
    """fn over the three matrices -> the oracle's constraint_fn over concatenated rows"""
    ch = list(challenges)
    return lambda loc, nxt, sels, pub: fn(loc[:w], nxt[:w], loc[w:w + wp], nxt[w:w + wp], loc[w + wp:],
                                          nxt[w + wp:], sels, pub, ch)


class ZeroDenominator(Exception):
    """batch_multiplicative_inverse panics on a zero (field/src/batch_inverse.rs:17-18)."""


def generate_permutation(terms, rows, pre_rows, publics, challenges, perm_width):
    """LogUpGadget::generate_permutation over canonical int rows -> height x perm_width ints:
    perm[0] = 0, perm[i + 1][c] = perm[i][c] + sum_t m_t / d_t with local = row i, next = row
    (i + 1) mod height.  The last row's contribution is computed (and may raise) but not stored."""
    n = len(rows)
    perm = [[0] * perm_width for _ in range(n)]
    for i in range(n):
        j = (i + 1) % n
        ploc = pre_rows[i] if pre_rows is not None else []
        pnxt = pre_rows[j] if pre_rows is not None else []
        for l, (col, tl) in enumerate(terms(rows[i], rows[j], ploc, pnxt, list(publics), list(challenges))):
            s = 0
            for d, m in tl:
                if d % P == 0:
                    raise ZeroDenominator(f"lookup {l}, row {i}")
                s = (s + m * pow(d, -1, P)) % P
            if i < n - 1:
                perm[i + 1][col] = (perm[i][col] + s) % P
    return perm


def prove(trace, pp, pre, srs, fn, terms, perm_width, log_qd, publics=(), challenger=None, challenges=None,
          alpha=None, zeta=None):
    """prove_with_preprocessed with lookups.  trace: (n, w, 4) limbs; pp: mirror_preprocessed.setup
    of `pre` (n, wp, 4) limbs, or both None.  Returns a proof in native.prove_native's shape: opened
    = [trace, permutation, quotient chunks(, preprocessed)]."""
    n, w = trace.shape[0], trace.shape[1]
    log_n = n.bit_length() - 1
    wp = pp.width if pp is not None else 0
    coeffs = C.idft_batch(trace)
    trace_commit = C.g1_msm_columns(srs[:n], coeffs)
    if challenger is not None:
        MP.observe_instance(challenger, log_n, trace_commit, wp, pp.commitment if pp is not None else None, publics)
        challenges = [challenger.sample() for _ in range(2 * perm_width)]  # prover.rs:214-216
    rows = [ints(r) for r in trace]
    pre_rows = [ints(r) for r in pre] if pre is not None else None
    perm = to_limbs(generate_permutation(terms, rows, pre_rows, publics, challenges, perm_width))
    perm_coeffs = C.idft_batch(perm)  # committed on the trace domain (:270)
    perm_commit = C.g1_msm_columns(srs[:n], perm_coeffs)
    if challenger is not None:
        challenger.observe_g1(_points(perm_commit))  # :273
        alpha = challenger.sample()  # :300
    g = lim(O.GENERATOR)
    ldes = [C.kzg_evaluations_on_domain(coeffs, log_n + log_qd, g)]
    if pp is not None:
        ldes.append(C.kzg_evaluations_on_domain(pp.coeffs, log_n + log_qd, g))
    ldes.append(C.kzg_evaluations_on_domain(perm_coeffs, log_n + log_qd, g))
    lde_rows = [sum((ints(m[i]) for m in ldes), []) for i in range(1 << (log_n + log_qd))]
    qv = np.stack([lim(v) for v in O.quotient_values_fn(lde_rows, log_n, log_qd, split_fn(fn, w, wp, challenges),
                                                       alpha, list(publics))])
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

    # the rounds in the reference's order (prover.rs:426-439)
    tr = open_matrix(coeffs, [zeta, zeta_next])
    pm = open_matrix(perm_coeffs, [zeta, zeta_next])
    qs = [open_matrix(cc, [zeta]) for cc in q_coeffs]
    qo = SimpleNamespace(values=[q.values[0] for q in qs], witnesses=[q.witnesses[0] for q in qs])
    opened = [tr, pm, qo]
    if pp is not None:
        opened.append(open_matrix(pp.coeffs, [zeta, zeta_next]))
    return SimpleNamespace(trace_commit=[trace_commit], quotient_commit=[c.reshape(1, 8) for c in quotient_commit],
                           opened=opened, degree_bits=log_n, alpha=alpha, zeta=zeta,
                           preprocessed_commit=[pp.commitment] if pp is not None else None,
                           permutation_commit=[perm_commit], permutation_challenges=list(challenges),
                           quotient_values=qv, permutation=perm)


def verify(proof, vk_commit, fn, perm_width, log_n, log_qd, srs_alpha, challenger=None, challenges=None, alpha=None,
           zeta=None, trace=None, pre=None, perm=None, publics=(), seed=2024):
    """verify_with_preprocessed with lookups (verifier.rs:354-499): the transcript, the OOD identity
    over the opened main | preprocessed | permutation rows, and every opening as a KZG claim (the
    preprocessed ones against the SETUP's commitment `vk_commit`, None without preprocessed columns).
    With `trace` / `pre` / `perm` (limbs) also the opened values against the matrices themselves.
    Returns the named checks and the claims (commitment, z, value, witness) for a pairing check."""
    tc = np.asarray(proof.trace_commit[0], dtype=np.uint64).reshape(-1, 8)
    qc = np.stack([np.asarray(c, dtype=np.uint64).reshape(8) for c in proof.quotient_commit])
    mc = np.asarray(proof.permutation_commit[0], dtype=np.uint64).reshape(-1, 8)
    pc = np.asarray(vk_commit, dtype=np.uint64).reshape(-1, 8) if vk_commit is not None else None
    wp = pc.shape[0] if pc is not None else 0
    assert mc.shape[0] == perm_width
    w = tc.shape[0]
    res = {}
    if challenger is not None:
        MP.observe_instance(challenger, log_n, tc, wp, pc, publics)
        challenges = [challenger.sample() for _ in range(2 * perm_width)]  # verifier.rs:369-375
        challenger.observe_g1(_points(mc))  # :378-380
        alpha = challenger.sample()
        challenger.observe_g1(_points(qc))
        zeta = challenger.sample()
        res["transcript"] = (list(proof.permutation_challenges), proof.alpha, proof.zeta) == (challenges, alpha, zeta)
    zeta_next = zeta * O.two_adic_generator(log_n) % P
    tr, pm, qo = proof.opened[:3]
    po = proof.opened[3] if wp else None
    local, nxt = ints(tr.values[0][0]), ints(tr.values[0][1])
    mlocal, mnxt = ints(pm.values[0][0]), ints(pm.values[0][1])
    plocal, pnxt = (ints(po.values[0][0]), ints(po.values[0][1])) if wp else ([], [])
    qvals = [ints(qo.values[c][0])[0] for c in range(len(qo.values))]
    ch = list(challenges)
    res["ood"] = V.ood_check(lambda loc, nx, sels: fn(loc[:w], nx[:w], loc[w:w + wp], nx[w:w + wp], loc[w + wp:],
                                                      nx[w + wp:], sels[:3], list(publics), ch),
                             local + plocal + mlocal, nxt + pnxt + mnxt, qvals, alpha, zeta, log_n, log_qd)
    rounds = [(tr, tc, (local, nxt)), (pm, mc, (mlocal, mnxt))]
    if wp:
        rounds.append((po, pc, (plocal, pnxt)))
    claims = []
    for opened, commit, vals_at in rounds:
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
        mats = [(trace, tr, tc), (perm, pm, mc)] + ([(pre, po, pc)] if wp else [])
        for mat, opened, commit in mats:
            ev = C.bary_eval_cols(np.ascontiguousarray(mat, dtype=np.uint64), pts)
            ok = ok and all(np.array_equal(ev[p], np.asarray(opened.values[0][p]).reshape(-1, 4)) for p in range(2))
            extra += [(commit[c], V.fr_int(ev[2][c])) for c in range(commit.shape[0])]
        res["opened_vs_trace"] = bool(ok)
    res["kzg"] = V.kzg_claims_identity(claims, srs_alpha, seed, extra)
    return res, claims
