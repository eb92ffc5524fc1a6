"""Plain-Python restatement of the MSM's digit pipeline (msm_digits.hip: k_msm_digits, k_msm_digits4,
DigitSource; k_bucket_start; the piece offsets of sort.h), for the stage-level tests.

Signed-window recoding of a canonical scalar s into W windows of c bits, B = 2^(c-1): window w's raw
value is bits [cw, cw + c) of s plus the carry of the window below; a raw value above B becomes the
negative digit raw - 2^c in [-(B - 1), -1] and carries 1 into the next window, a raw value of exactly
B stays the positive digit B.  So every digit lies in [-(B - 1), B] and sum_w d_w 2^(cw) = s.

A nonzero digit d of row i, column col, window w is the pair
    key   = (group << c) | (|d| - 1)      group = col (fixed-base tables) or col W + w
    value = ref | neg << 31               ref = i ref_windows + w (fixed-base tables) or i
and a zero digit the sentinel (0xFFFFFFFF, 0).  The kernels emit the pairs group-major, pair
e = (col W + w) n + i, and sort them on the low c key bits; bucket (|d| - 1) groups + group of the
sorted sequence is then one contiguous run.
"""

from __future__ import annotations

import numpy as np

SENTINEL = 0xFFFFFFFF


def recode(s: int, c: int, W: int):
    """-> (digits d_0..d_{W-1}, raw windows incl. the carry in, carry out of the top window)."""
    B = 1 << (c - 1)
    mask = (1 << c) - 1
    digits, raws, carry = [], [], 0
    for w in range(W):
        raw = ((s >> (c * w)) & mask) + carry
        raws.append(raw)
        if raw > B:
            digits.append(raw - (1 << c))
            carry = 1
        else:
            digits.append(raw)
            carry = 0
    return digits, raws, carry


def edge_scalars(c: int, r: int):
    """The recoding's edge values for window width c, each below r (reduced where the pattern is
    not): 0, 1, around B = 2^(c-1), every window at B (no carry, magnitude B everywhere), every
    window at B + 1 (a carry chain through all windows), B + 1 then windows of 2^c - 1 (the carry
    ripples and leaves zero digits) -- each over all W windows and over the W - 1 low ones, which
    stay below r so the pattern survives -- and r - 1, the largest value below r (its top window is
    nonzero)."""
    W = (255 + c - 1) // c
    B = 1 << (c - 1)
    full = (1 << c) - 1
    out = [0, 1, B, B + 1, full]
    for k in (W, W - 1):
        out.append(sum(B << (c * w) for w in range(k)))
        out.append(sum((B + 1) << (c * w) for w in range(k)))
        out.append((B + 1) + sum(full << (c * w) for w in range(1, k)))
    out.append(r - 1)
    return [v % r for v in out]


def reference_pairs(cols, c: int, W: int, ref_windows: int, fixed: bool):
    """The group-major emission of the columns' digit pairs: cols[j][i] = canonical scalar of row i,
    column j (columns local to the batch).  -> (keys, vals) of n W len(cols) entries, u32."""
    n = len(cols[0]) if cols else 0
    keys = np.full(len(cols) * W * n, SENTINEL, dtype=np.uint32)
    vals = np.zeros(len(cols) * W * n, dtype=np.uint32)
    at, ks, vs = [], [], []
    for j, col in enumerate(cols):
        for i, s in enumerate(col):
            if s == 0:
                continue
            digits, _, carry = recode(s, c, W)
            assert carry == 0, "a nonzero digit above the top window"
            for w, d in enumerate(digits):
                if d == 0:
                    continue
                at.append((j * W + w) * n + i)
                g = j if fixed else j * W + w
                ks.append((g << c) | (abs(d) - 1))
                vs.append(((i * ref_windows + w) if fixed else i) | ((1 << 31) if d < 0 else 0))
    keys[at] = ks
    vals[at] = vs
    return keys, vals


def bucket_of(keys: np.ndarray, c: int, groups: int, nb: int) -> np.ndarray:
    """msm_batch.h bucket_of: (|d| - 1) groups + group, nb for the sentinel."""
    k = keys.astype(np.uint64)
    b = (k & np.uint64((1 << (c - 1)) - 1)) * np.uint64(groups) + (k >> np.uint64(c))
    return np.where(keys == np.uint32(SENTINEL), np.uint64(nb), b).astype(np.int64)


def chunk_counts(start: np.ndarray, log_chunk: int) -> np.ndarray:
    """sort.h's piece counts: the 2^log_chunk-aligned runs bucket b's pairs [start[b], start[b+1])
    touch, 0 if empty; one entry per bucket plus a trailing 0 (nb + 1 entries for nb + 1 starts)."""
    s = start[:-1].astype(np.int64)
    e = start[1:].astype(np.int64)
    cnt = np.where(s == e, 0, ((e - 1) >> log_chunk) - (s >> log_chunk) + 1)
    return np.concatenate([cnt, [0]]).astype(np.int64)


def exclusive_sum_u32(v: np.ndarray) -> np.ndarray:
    """out[i] = v[0] + ... + v[i-1] modulo 2^32."""
    out = np.zeros(len(v), dtype=np.uint64)
    if len(v) > 1:
        out[1:] = np.cumsum(v[:-1].astype(np.uint64))
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)
