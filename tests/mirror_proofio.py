"""Pure-Python writer and parser of the proof container (include/eon_prove.h "proof bytes",
plonky3_eon_amd/host/proof_io.h), on Python integers: the header rules, the section order, the Fr
and G1 element rules (decompression is pow(t, (q + 1) // 4, q), as in tests/mirror_srs.py) and the
lowest-offset rule, which a sequential parse gives by construction.

A proof is a dict of uint64 arrays in the layout of eon_proof_lk (Montgomery limbs, as the prover
returns them) next to a shape dict:

    trace_commit (W, 8)        quotient_commit (C, 8)        permutation_commit (Wq, 8)
    trace_opened (2, W, 4)     quotient_opened (C, 4)        permutation_opened (2, Wq, 4)
    trace_witnesses (2, w, 8)  quotient_witnesses (C, 8)     permutation_witnesses (2, wq, 8)
    preprocessed_opened (2, Wp, 4)   preprocessed_witnesses (2, wp, 8)

with w = W (per column) or 1 (batched), and the permutation / preprocessed arrays present exactly
when the proof has that part."""

import struct

import numpy as np

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = 1 << 256
MAGIC = b"EONPRF1\0"
HEADER_BYTES = 48
VERSION = 1
BATCHED, PREPROCESSED, PERMUTATION = 1, 2, 4
SECTIONS = ["HEADER", "TRACE_COMMIT", "PERMUTATION_COMMIT", "QUOTIENT_COMMIT", "TRACE_LOCAL", "TRACE_NEXT",
            "PERMUTATION_LOCAL", "PERMUTATION_NEXT", "PREPROCESSED_LOCAL", "PREPROCESSED_NEXT", "QUOTIENT_OPENED",
            "TRACE_WITNESS_ZETA", "TRACE_WITNESS_NEXT", "PERMUTATION_WITNESS_ZETA", "PERMUTATION_WITNESS_NEXT",
            "QUOTIENT_WITNESS", "PREPROCESSED_WITNESS_ZETA", "PREPROCESSED_WITNESS_NEXT"]
FR_SECTIONS = SECTIONS[4:11]
# section -> (array, row of the leading [2] axis or None)
WHERE = {"TRACE_COMMIT": ("trace_commit", None), "PERMUTATION_COMMIT": ("permutation_commit", None),
         "QUOTIENT_COMMIT": ("quotient_commit", None), "TRACE_LOCAL": ("trace_opened", 0),
         "TRACE_NEXT": ("trace_opened", 1), "PERMUTATION_LOCAL": ("permutation_opened", 0),
         "PERMUTATION_NEXT": ("permutation_opened", 1), "PREPROCESSED_LOCAL": ("preprocessed_opened", 0),
         "PREPROCESSED_NEXT": ("preprocessed_opened", 1), "QUOTIENT_OPENED": ("quotient_opened", None),
         "TRACE_WITNESS_ZETA": ("trace_witnesses", 0), "TRACE_WITNESS_NEXT": ("trace_witnesses", 1),
         "PERMUTATION_WITNESS_ZETA": ("permutation_witnesses", 0),
         "PERMUTATION_WITNESS_NEXT": ("permutation_witnesses", 1), "QUOTIENT_WITNESS": ("quotient_witnesses", None),
         "PREPROCESSED_WITNESS_ZETA": ("preprocessed_witnesses", 0),
         "PREPROCESSED_WITNESS_NEXT": ("preprocessed_witnesses", 1)}


class Rejected(Exception):
    def __init__(self, reason, section="HEADER", index=0):
        super().__init__(f"{reason} at {section}[{index}]")
        self.reason, self.section, self.index = reason, section, index


def shape_ok(s) -> bool:
    return not (s["flags"] & ~7) and (s["pre_width"] != 0) == bool(s["flags"] & PREPROCESSED) and \
        (s["perm_width"] != 0) == bool(s["flags"] & PERMUTATION)


def counts(s) -> dict:
    """elements per section, in body order"""
    batched = bool(s["flags"] & BATCHED)
    w, c, wp, wq = s["width"], s["chunks"], s["pre_width"], s["perm_width"]
    tw, qw, pw = (1, min(wq, 1), min(wp, 1)) if batched else (w, wq, wp)
    return dict(zip(SECTIONS[1:], [w, wq, c, w, w, wq, wq, wp, wp, c, tw, tw, qw, qw, c, pw, pw]))


def size(s) -> int:
    """48 + the body length; 0 on an invalid shape (also one whose length leaves 64 bits)"""
    if not shape_ok(s):
        return 0
    n = HEADER_BYTES + 32 * sum(counts(s).values())
    return n if n < 1 << 64 else 0


def header(s, body=None) -> bytes:
    body = size(s) - HEADER_BYTES if body is None else body
    return MAGIC + struct.pack("<IIIIIIIIQ", VERSION, s["flags"], s["degree_bits"], s["width"], s["chunks"],
                               s["pre_width"], s["perm_width"], 0, body)


def peek(data: bytes) -> dict:
    if len(data) < HEADER_BYTES:
        raise Rejected("LENGTH")
    if data[:8] != MAGIC:
        raise Rejected("MAGIC")
    version, flags, bits, w, c, wp, wq, zero, body = struct.unpack("<IIIIIIIIQ", data[8:48])
    if version != VERSION:
        raise Rejected("VERSION")
    s = dict(flags=flags, degree_bits=bits, width=w, chunks=c, pre_width=wp, perm_width=wq)
    if not shape_ok(s) or zero:
        raise Rejected("FLAGS")
    if size(s) == 0 or body != size(s) - HEADER_BYTES or size(s) != len(data):
        raise Rejected("LENGTH")
    return s


# ---- elements -----------------------------------------------------------------------------------------
def limbs(v: int, n: int = 4):
    return [(v >> (64 * i)) & (2**64 - 1) for i in range(n)]


def unlimbs(row) -> int:
    return sum(int(x) << (64 * i) for i, x in enumerate(row))


def g1_encode(row) -> bytes:
    """8 Montgomery limbs (x, y) -> G1Affine::to_bytes"""
    xm, ym = unlimbs(row[:4]), unlimbs(row[4:])
    if xm == 0 and ym == 0:
        return bytes(31) + b"\x40"
    x, y = xm * pow(MONT, -1, Q) % Q, ym * pow(MONT, -1, Q) % Q
    return (x | (y & 1) << 255).to_bytes(32, "little")


def g1_decode(b: bytes):
    """32 bytes -> 8 Montgomery limbs; raises Rejected(reason): the identity flag first (every
    other bit zero), then x < q, then the square root and its parity"""
    v = int.from_bytes(b, "little")
    if (v >> 254) & 1:
        if v != 1 << 254:
            raise Rejected("G1_ENCODING")
        return [0] * 8
    x = v & ((1 << 254) - 1)
    if x >= Q:
        raise Rejected("G1_NOT_CANONICAL")
    t = (x * x * x + 3) % Q
    y = pow(t, (Q + 1) // 4, Q)
    if y * y % Q != t:
        raise Rejected("G1_NOT_ON_CURVE")
    if (y & 1) != v >> 255:
        y = (Q - y) % Q
    return limbs(x * MONT % Q) + limbs(y * MONT % Q)


def fr_decode(b: bytes):
    v = int.from_bytes(b, "little")
    if v >= R:
        raise Rejected("FR_NOT_CANONICAL")
    return limbs(v)


# ---- the container ------------------------------------------------------------------------------------
def parse(data: bytes):
    """bytes -> (shape, arrays); raises Rejected(reason, section, index) at the first bad element"""
    s = peek(data)
    batched = bool(s["flags"] & BATCHED)
    w, c, wp, wq = s["width"], s["chunks"], s["pre_width"], s["perm_width"]
    a = {"trace_commit": np.zeros((w, 8), np.uint64), "quotient_commit": np.zeros((c, 8), np.uint64),
         "trace_opened": np.zeros((2, w, 4), np.uint64),
         "trace_witnesses": np.zeros((2, 1 if batched else w, 8), np.uint64),
         "quotient_opened": np.zeros((c, 4), np.uint64), "quotient_witnesses": np.zeros((c, 8), np.uint64)}
    if wq:
        a.update(permutation_commit=np.zeros((wq, 8), np.uint64), permutation_opened=np.zeros((2, wq, 4), np.uint64),
                 permutation_witnesses=np.zeros((2, 1 if batched else wq, 8), np.uint64))
    if wp:
        a.update(preprocessed_opened=np.zeros((2, wp, 4), np.uint64),
                 preprocessed_witnesses=np.zeros((2, 1 if batched else wp, 8), np.uint64))
    at = HEADER_BYTES
    for section, n in counts(s).items():
        name, row = WHERE[section]
        for i in range(n):
            try:
                v = (fr_decode if section in FR_SECTIONS else g1_decode)(data[at:at + 32])
            except Rejected as e:
                raise Rejected(e.reason, section, i) from None
            dst = a[name] if row is None else a[name][row]
            dst[i] = np.array(v, dtype=np.uint64)
            at += 32
    assert at == len(data)
    return s, a


def write(s, a) -> bytes:
    """(shape, arrays) -> bytes"""
    assert size(s)
    out = [header(s)]
    for section, n in counts(s).items():
        name, row = WHERE[section]
        if n == 0:
            continue
        src = np.asarray(a[name] if row is None else a[name][row], dtype=np.uint64)
        assert src.shape[0] == n, (section, src.shape, n)
        for i in range(n):
            out.append(src[i].astype("<u8").tobytes() if section in FR_SECTIONS else g1_encode(src[i]))
    data = b"".join(out)
    assert len(data) == size(s)
    return data


def offset_of(s, section: str, index: int = 0) -> int:
    """byte offset of an element"""
    at = HEADER_BYTES
    for name, n in counts(s).items():
        if name == section:
            assert index < n
            return at + 32 * index
        at += 32 * n
    raise KeyError(section)


# ---- a Proof (plonky3_eon_amd.proof) as (shape, arrays) -----------------------------------------------
def proof_arrays(proof):
    u = lambda x, k: np.asarray(x, dtype=np.uint64).reshape(-1, k)  # noqa: E731
    has_perm = proof.permutation_commit is not None
    opened = list(proof.opened)
    has_pre = len(opened) > (3 if has_perm else 2)
    quot = opened[2 if has_perm else 1]

    def pair(op, k, which):
        return np.stack([u(x, k) for x in getattr(op, which)[0]])

    a = {"trace_commit": u(proof.trace_commit[0], 8),
         "quotient_commit": np.concatenate([u(c, 8) for c in proof.quotient_commit]),
         "trace_opened": pair(opened[0], 4, "values"), "trace_witnesses": pair(opened[0], 8, "witnesses"),
         "quotient_opened": np.concatenate([u(v[0], 4) for v in quot.values]),
         "quotient_witnesses": np.concatenate([u(w[0], 8) for w in quot.witnesses])}
    if has_perm:
        a.update(permutation_commit=u(proof.permutation_commit[0], 8), permutation_opened=pair(opened[1], 4, "values"),
                 permutation_witnesses=pair(opened[1], 8, "witnesses"))
    if has_pre:
        a.update(preprocessed_opened=pair(opened[-1], 4, "values"),
                 preprocessed_witnesses=pair(opened[-1], 8, "witnesses"))
    s = dict(flags=(BATCHED if proof.opening == "batched" else 0) | (PREPROCESSED if has_pre else 0) |
             (PERMUTATION if has_perm else 0), degree_bits=int(proof.degree_bits), width=a["trace_commit"].shape[0],
             chunks=a["quotient_commit"].shape[0],
             pre_width=a["preprocessed_opened"].shape[1] if has_pre else 0,
             perm_width=a["permutation_opened"].shape[1] if has_perm else 0)
    return s, a


def witness_count(s) -> int:
    c = counts(s)
    return sum(n for name, n in c.items() if "WITNESS" in name)
