"""Signature rows on which exactly ONE of libsodium's reject conditions acts.

libsodium 1.0.18 crypto_sign_verify_detached accepts iff
    (1) S < L, (2) R is not small-order, (3) A is canonical, (4) A is not
    small-order, (5) A decodes, and (8) encode([S]B - [h]A) == R,
    h = SHA-512(R || A || M) mod L.
The fixtures make their small-order / non-canonical rows by putting a
blacklisted encoding into a signature made for another key, so on those rows
(8) fails as well and a verifier that lost one of the other terms would still
reject them.  The rows here are built so that the point equation
[S]B - [h]A_pt == R_pt HOLDS (decoding as the kernels do: y reduced mod p,
x = 0 keeps x = 0 whatever the sign bit) while exactly one of (1)-(5) fails:

iso_small_A   A = E, one of the 14 blacklist encodings (7 entries x bit 255),
              T its point (a torsion point, T = [j]T8).  R = enc(rB + [k]T8),
              h = H(R || E || M); the row is kept when -[h]T == [k]T8, and
              then S = r gives [S]B - [h]T == R_pt.  R is canonical and not
              small-order, 0 < S < L: only (4) fails (and (3) for y >= p).
              Such a row is the forgery a verifier without (4) accepts.
iso_small_R   R = E.  A' = enc(aB + [kA]T8) with kA odd (mixed order: canonical,
              not blacklisted, decodable), h = H(E || A' || M), S = h a mod L:
              [S]B - [h]A'_pt = -[h kA]T8, kept when that is T.  Only (2)
              fails.  For 6 of the 14 encodings E is not the canonical
              encoding of T (y = p, p + 1, and x = 0 with the sign bit), where
              libsodium's byte compare (8) rejects too; the rows are kept
              because the warm path compares projectively (column canonical_R).
iso_S_ge_L_lo a valid signature with S + L in place of S; S + L < 2^253, so
              clearing bits 253..255 (the comb kernel's mask) leaves it alone.
iso_S_ge_L_hi ... with S + kL, k = 2..15, all >= 2^253.  (S + L itself reaches
              2^253 only for S within 2^125 of L, which no grinding finds: a
              valid S is uniform mod L.  These are the encodings >= 2^253
              that are congruent to a valid S.)  Only (1) fails.
control_valid, control_torsion
              the accepts among them: ordinary signatures, and mixed-order
              keys (torsion_rows.torsion_row(..., accept=True)).

Everything is pure Python over hashlib and the point helpers of
torsion_rows.py, deterministic (scalars and messages are derived by SHA-512
from fixed tags), and checked by holds() as it is emitted.  A row that is not
found within MAX_TRIES messages is an error, never a skip.
"""
import functools
import hashlib

import numpy as np

from torsion_rows import D, L, P, TORSION, T8_ENC, _add, _dec, _enc, _hram, rfc8032_secrets, torsion_row

MAX_TRIES = 64
CLASS_NAMES = ("iso_small_A", "iso_small_R", "iso_S_ge_L_lo", "iso_S_ge_L_hi", "control_valid", "control_torsion")

B_ENC = bytes.fromhex("58" + "66" * 31)
B = _dec(B_ENC)
IDENT = (0, 1, 1, 0)

# The blacklist (libsodium ge25519_has_small_order) by what it holds, not copied
# from the engine: the y of every torsion point -- 1 (identity), p - 1 (order
# 2), 0 (order 4), +-y8 (order 8) -- and the aliases p, p + 1 of 0 and 1.
_Y8 = int.from_bytes(T8_ENC, "little") & ((1 << 255) - 1)
BLACKLIST_Y = (0, 1, _Y8, P - _Y8, P - 1, P, P + 1)
assert sorted({p[1] * pow(p[2], P - 2, P) % P for p in TORSION}) == sorted({0, 1, _Y8, P - _Y8, P - 1})
# the 14 encodings: index e = 2 * entry + sign bit
ENCODINGS = tuple((y | (s << 255)).to_bytes(32, "little") for y in BLACKLIST_Y for s in (0, 1))


def _neg(p):
    return (-p[0] % P, p[1], p[2], -p[3] % P)


def _eq(p, q):
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def _mul(k, p):
    """[k]p by double-and-add (the addition law is complete, so any p)."""
    acc = IDENT
    while k:
        if k & 1:
            acc = _add(acc, p)
        p = _add(p, p)
        k >>= 1
    return acc


@functools.lru_cache(maxsize=None)
def _b_table():
    """d * 16^i * B, d = 1..15, i = 0..63."""
    tab, base = [], B
    for _ in range(64):
        row, acc = [IDENT], IDENT
        for _d in range(15):
            acc = _add(acc, base)
            row.append(acc)
        tab.append(row)
        base = _add(row[15], base)
    return tab


def _mul_B(k):
    k %= L
    acc, tab = IDENT, _b_table()
    for i in range(64):
        d = (k >> (4 * i)) & 15
        if d:
            acc = _add(acc, tab[i][d])
    return acc


def dec_lenient(s):
    """The point an encoding stands for when decoded as the kernels do: y
    reduced mod p, the sign bit choosing x, x = 0 staying 0 (None: off-curve)."""
    y = (int.from_bytes(s, "little") & ((1 << 255) - 1)) % P
    sign = s[31] >> 7
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    if (v * x * x - u) % P != 0:
        if (v * x * x + u) % P != 0:
            return None
        x = x * pow(2, (P - 1) // 4, P) % P
    if x and (x & 1) != sign:
        x = P - x
    return (x, y, 1, x * y % P)


def is_blacklisted(s):
    return (int.from_bytes(s, "little") & ((1 << 255) - 1)) in BLACKLIST_Y


def blacklist_index(s):
    """Index into ENCODINGS of a blacklisted encoding (else -1)."""
    y = int.from_bytes(s, "little") & ((1 << 255) - 1)
    return 2 * BLACKLIST_Y.index(y) + (s[31] >> 7) if y in BLACKLIST_Y else -1


def _torsion_index(p):
    for j, t in enumerate(TORSION):
        if _eq(p, t):
            return j
    return -1


def conditions(pk, sig):
    """The set of the conditions (1)-(5) that fail on a row."""
    pk, sig = bytes(pk), bytes(sig)
    failing = set()
    if int.from_bytes(sig[32:], "little") >= L:
        failing.add(1)
    if is_blacklisted(sig[:32]):
        failing.add(2)
    if (int.from_bytes(pk, "little") & ((1 << 255) - 1)) >= P:
        failing.add(3)
    if is_blacklisted(pk):
        failing.add(4)
    if dec_lenient(pk) is None:
        failing.add(5)
    return failing


def holds(pk, sig, msg):
    """(equation, failing): whether [S]B - [h]A_pt == R_pt in Python integers
    (lenient decoding; False when A or R has no point), and the set of the
    conditions (1)-(5) that fail on the row."""
    pk, sig, msg = bytes(pk), bytes(sig), bytes(msg)
    Renc, S = sig[:32], int.from_bytes(sig[32:], "little")
    failing = conditions(pk, sig)
    A, R = dec_lenient(pk), dec_lenient(Renc)
    if A is None or R is None:
        return False, failing
    h = _hram(Renc, pk, msg)
    j = _torsion_index(A)
    hA = TORSION[h * j % 8] if j >= 0 else _mul(h, A)
    return _eq(_add(_mul_B(S), _neg(hA)), R), failing


def census(d):
    """The reject rows of a fixture-shaped dict whose point equation holds, by
    the conditions that fail on them: {"S": rows where only (1) fails,
    "A": {encoding index: rows} where only A is small-order ((4), with (3) for
    y >= p), "R": the same for (2), "AR": rows where A and R both are}.  The
    equation is evaluated only where it can matter (one of those sets).  These
    count the rows whose R is the canonical encoding of its point, where
    libsodium's byte compare (8) holds as well; rows whose R is not (the compare
    fails, the projective test does not) are counted under "noncanonical_R"."""
    out = {"S": 0, "A": {}, "R": {}, "AR": 0, "noncanonical_R": 0}
    for i in np.nonzero(np.asarray(d["verdict"]) == 0)[0]:
        pk, sig = d["pk"][i].tobytes(), d["sig"][i].tobytes()
        f = conditions(pk, sig)
        a, r = bool(f & {4}), 2 in f
        if not f or (f - {2, 3, 4}) not in (set(), {1}) or (1 in f and (a or r)) or (3 in f and not a):
            continue
        o, ln = int(d["msg_off"][i]), int(d["msg_len"][i])
        if not holds(pk, sig, d["msg"][o:o + ln].tobytes())[0]:
            continue
        if _enc(dec_lenient(sig[:32])) != sig[:32]:
            out["noncanonical_R"] += 1
        elif a and r:
            out["AR"] += 1
        elif a:
            out["A"][blacklist_index(pk)] = out["A"].get(blacklist_index(pk), 0) + 1
        elif r:
            out["R"][blacklist_index(sig[:32])] = out["R"].get(blacklist_index(sig[:32]), 0) + 1
        else:
            out["S"] += 1
    return out


def _bytes(tag, *parts):
    h = hashlib.sha512(tag.encode())
    for x in parts:
        h.update(int(x).to_bytes(8, "little"))
    return h.digest()


def _scalar(tag, *parts):
    """A scalar in [1, L) derived from the tag."""
    return int.from_bytes(_bytes(tag, *parts), "little") % (L - 1) + 1


def _message(mlen, *parts):
    out = b""
    c = 0
    while len(out) < mlen:
        out += _bytes("isolating-rows message", mlen, c, *parts)
        c += 1
    return out[:mlen]


def _sign(a, A_enc, r, msg):
    R_enc = _enc(_mul_B(r))
    S = (r + _hram(R_enc, A_enc, msg) * a) % L
    return R_enc + S.to_bytes(32, "little")


def small_A_row(e, idx, mlen):
    """(pk, sig, msg, tries) of iso_small_A for encoding e, row idx."""
    E = ENCODINGS[e]
    j = _torsion_index(dec_lenient(E))
    assert j >= 0
    for t in range(MAX_TRIES):
        msg = _message(mlen, 1, e, idx, t)
        r = _scalar("isolating-rows small_A r", mlen, e, idx, t)
        rB = _mul_B(r)
        for k in range(8):
            R_enc = _enc(_add(rB, TORSION[k]))
            h = _hram(R_enc, E, msg)
            if (-h * j - k) % 8 == 0:  # -[h]T == [k]T8
                return E, R_enc + r.to_bytes(32, "little"), msg, t + 1
    raise RuntimeError("iso_small_A: no row for encoding %d within %d tries" % (e, MAX_TRIES))


def small_R_row(e, idx, mlen):
    """(pk, sig, msg, tries) of iso_small_R for encoding e, row idx."""
    E = ENCODINGS[e]
    j = _torsion_index(dec_lenient(E))
    assert j >= 0
    a = _scalar("isolating-rows small_R a", mlen, e, idx)
    aB = _mul_B(a)
    keys = [(kA, _enc(_add(aB, TORSION[kA]))) for kA in (1, 3, 5, 7)]
    for t in range(MAX_TRIES):
        msg = _message(mlen, 2, e, idx, t)
        for kA, A_enc in keys:
            h = _hram(E, A_enc, msg)
            S = h * a % L
            if (-h * kA - j) % 8 == 0 and S != 0:  # -[h kA]T8 == T
                return A_enc, E + S.to_bytes(32, "little"), msg, t + 1
    raise RuntimeError("iso_small_R: no row for encoding %d within %d tries" % (e, MAX_TRIES))


def _valid_row(tag, idx, mlen):
    a = _scalar("isolating-rows %s a" % tag, mlen, idx)
    A_enc = _enc(_mul_B(a))
    msg = _message(mlen, 3, idx, sum(tag.encode()))
    return A_enc, _sign(a, A_enc, _scalar("isolating-rows %s r" % tag, mlen, idx), msg), msg


def S_ge_L_row(idx, mlen, k):
    """A valid signature with S + kL in place of S."""
    pk, sig, msg = _valid_row("S_ge_L%d" % (k > 1), idx, mlen)
    S = int.from_bytes(sig[32:], "little") + k * L
    assert (S < 1 << 253) == (k == 1) and S < 1 << 256
    return pk, sig[:32] + S.to_bytes(32, "little"), msg


def _rfc8032_sign(seed, msg):
    a, r = rfc8032_secrets(seed, msg)
    pk = _enc(_mul_B(a))
    return pk, _sign(a, pk, r, msg)


def torsion_control_row(idx, mlen):
    seed = _bytes("isolating-rows torsion seed", mlen, idx)[:32]
    msg = _message(mlen, 4, idx)
    pk, sig = _rfc8032_sign(seed, msg)
    pk2, sig2, _, _ = torsion_row(seed, msg, pk, sig, accept=True, start=idx)
    return pk2, sig2, msg


@functools.lru_cache(maxsize=None)
def generate(mlen, per_pair=3, n_S=6, n_valid=24, n_torsion=8):
    """The rows for messages of mlen bytes, as a fixture-shaped dict of
    read-only arrays: pk, sig, msg, msg_off, msg_len, verdict (expected: 0 on
    every iso_* row, 1 on the controls), cls / class_names, enc (index into
    ENCODINGS, -1 where none), canonical_R (0: R is not the canonical encoding
    of its point) and tries.  Every row is checked with holds()."""
    rows = []  # (cls, enc, tries, pk, sig, msg)
    for e in range(len(ENCODINGS)):
        for idx in range(per_pair):
            pk, sig, msg, t = small_A_row(e, idx, mlen)
            rows.append((0, e, t, pk, sig, msg))
            pk, sig, msg, t = small_R_row(e, idx, mlen)
            rows.append((1, e, t, pk, sig, msg))
    for idx in range(n_S):
        rows.append((2, -1, 0) + S_ge_L_row(idx, mlen, 1))
        rows.append((3, -1, 0) + S_ge_L_row(idx, mlen, 2 + (13 * idx // max(1, n_S - 1) if n_S > 1 else 0)))
    for idx in range(n_valid):
        rows.append((4, -1, 0) + _valid_row("control", idx, mlen))
    for idx in range(n_torsion):
        rows.append((5, -1, 0) + torsion_control_row(idx, mlen))
    want_failing = {0: None, 1: {2}, 2: {1}, 3: {1}, 4: set(), 5: set()}
    for cls, e, _, pk, sig, msg in rows:
        eq, failing = holds(pk, sig, msg)
        assert eq, (CLASS_NAMES[cls], e)
        S = int.from_bytes(sig[32:], "little")
        if cls == 0:
            assert failing == ({4, 3} if BLACKLIST_Y[e // 2] >= P else {4}), (e, failing)
            assert 0 < S < L and not is_blacklisted(sig[:32]) and _enc(dec_lenient(sig[:32])) == sig[:32]
        else:
            assert failing == want_failing[cls], (CLASS_NAMES[cls], e, failing)
        if cls == 1:
            assert 0 < S < L and _dec(pk) is not None and _torsion_index(_dec(pk)) < 0
        if cls == 5:
            assert _torsion_index(_mul(L, dec_lenient(pk))) > 0  # mixed order
    n = len(rows)
    d = {
        "pk": np.frombuffer(b"".join(r[3] for r in rows), np.uint8).reshape(n, 32).copy(),
        "sig": np.frombuffer(b"".join(r[4] for r in rows), np.uint8).reshape(n, 64).copy(),
        "msg": np.frombuffer(b"".join(r[5] for r in rows), np.uint8).copy() if mlen else np.zeros(1, np.uint8),
        "msg_off": np.arange(n, dtype=np.uint64) * np.uint64(mlen),
        "msg_len": np.full(n, mlen, np.uint32),
        "cls": np.array([r[0] for r in rows], np.uint16),
        "class_names": np.array(CLASS_NAMES),
        "enc": np.array([r[1] for r in rows], np.int16),
        "tries": np.array([r[2] for r in rows], np.uint16),
    }
    d["verdict"] = (d["cls"] >= 4).astype(np.uint8)
    d["canonical_R"] = np.array([1 if _enc(dec_lenient(r[4][:32])) == r[4][:32] else 0 for r in rows], np.uint8)
    for v in d.values():
        v.setflags(write=False)
    return d


def interleaved(d, n, hot=(0, 63, 64)):
    """Row indices (into d) of a batch of n: every row of d at least once when
    n >= len(d), iso_* rows on the lanes `hot` and on the last index, controls
    and iso_* rows alternating elsewhere."""
    iso = [i for i in range(len(d["cls"])) if d["cls"][i] < 4]
    ctl = [i for i in range(len(d["cls"])) if d["cls"][i] >= 4]
    assert n >= len(hot) + 1
    out, ni, nc = [], 0, 0
    special = set(hot) | {n - 1}
    for pos in range(n):
        # (iso rows outnumber the controls: two iso rows per control, so both lists cycle about once)
        if pos in special or pos % 3 != 2:
            out.append(iso[ni % len(iso)])
            ni += 1
        else:
            out.append(ctl[nc % len(ctl)])
            nc += 1
    return np.array(out)


def gather(d, rows):
    """The sub-batch of `rows` as a fixture-shaped dict with its own message buffer."""
    rows = np.asarray(rows)
    ln = d["msg_len"][rows]
    off = np.zeros(len(rows), np.uint64)
    if len(rows) > 1:
        off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    msg = np.concatenate([d["msg"][int(d["msg_off"][i]):int(d["msg_off"][i]) + int(d["msg_len"][i])] for i in rows]
                         + [np.zeros(0, np.uint8)])
    return {"pk": d["pk"][rows].copy(), "sig": d["sig"][rows].copy(), "msg": msg if msg.size else np.zeros(1, np.uint8),
            "msg_off": off, "msg_len": ln.copy(), "verdict": d["verdict"][rows].copy(), "cls": d["cls"][rows].copy(),
            "enc": d["enc"][rows].copy(), "class_names": d["class_names"]}
