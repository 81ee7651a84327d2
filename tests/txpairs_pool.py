"""Input pool and plain-Python contract of the hinted tx-body entry points
(test_txpairs_cpu.py, test_gpu_txpairs.py).

expected(s, oracle) enumerates the contract of sv_ed25519_verify_txbodies_hinted
directly: a double loop over each body's signatures and keys, a pair where the
hint equals bytes 28..31 of the key, hashlib for the digests, the oracle for the
verdicts.  Nothing here comes from the code under test.

make_pool(nb, ...) builds nb bodies (kinds and lengths from txbodies_pool) with
their decorated signatures and candidate keys.  The first bodies are the
mandatory cases, in CASES order (one body each unless noted):
  no_match      a signature whose hint matches no key
  multi         a hint matching three keys of its body: the signer and two
                "wrong keys" (28 random bytes + the shared tail)
  neighbour     three bodies; the middle one's only key is in neither
                neighbour, its two signatures carry the hints of the
                neighbours' keys: no pair in the middle body
  dup_key       the same key listed twice: two pairs
  sigs_only     signatures and no keys
  keys_only     keys and no signatures
  empty         neither
  grid          20 signatures x 20 keys, all sharing one hint: 400 pairs
  one_byte      four signatures, hint differing from the key's tail in byte b only
  head          a hint equal to bytes 0..3 of the key, not its tail
the rest have 0 / 1 / 20 signatures (txbodies_pool.sigs_per_body), each signed
by one of the body's keys, with the pool's rejects (corrupted signature bytes,
a body mutated after signing).
"""
import numpy as np

import txbodies_pool as tp

CASES = ("no_match", "multi", "neighbour", "neighbour_mid", "neighbour_hi", "dup_key", "sigs_only", "keys_only",
         "empty", "grid", "one_byte", "head")


def enumerate_pairs(s):
    """The contract: (pair_begin, pair_sig, pair_key) by double loop."""
    sb, kb, hint, key = s["sig_begin"], s["key_begin"], s["hint"], s["key"]
    begin, ps, pk = [0], [], []
    for t in range(s["nb"]):
        for i in range(int(sb[t]), int(sb[t + 1])):
            h = hint[i].tobytes()
            for k in range(int(kb[t]), int(kb[t + 1])):
                if key[k, 28:].tobytes() == h:
                    ps.append(i)
                    pk.append(k)
        begin.append(len(ps))
    return np.array(begin, np.uint64), np.array(ps, np.uint32), np.array(pk, np.uint32)


def expected(s, oracle=None):
    """-> dict(pair_begin, pair_sig, pair_key, verdict, digests); verdicts by the
    oracle, or (large sets) by construction from s["valid"] (signature index ->
    the key index it verifies under)."""
    begin, ps, pk = enumerate_pairs(s)
    digests = np.array([np.frombuffer(tp.contents_hash(int(s["kind"][t]), body(s, t)), np.uint8)
                        for t in range(s["nb"])], np.uint8).reshape(s["nb"], 32)
    owner = np.searchsorted(begin, np.arange(len(ps)), side="right") - 1
    if oracle is not None:
        v = np.array([1 if oracle.oracle_ed25519_verify(s["sig"][ps[i]].tobytes(), digests[owner[i]].tobytes(), 32,
                                                        s["key"][pk[i]].tobytes()) == 0 else 0
                      for i in range(len(ps))], np.uint8)
    else:
        v = np.array([1 if s["valid"].get(int(ps[i])) == int(pk[i]) else 0 for i in range(len(ps))], np.uint8)
    return dict(pair_begin=begin, pair_sig=ps, pair_key=pk, verdict=v, digests=digests)


def body(s, t):
    o, ln = int(s["off"][t]), int(s["len"][t])
    return s["bodies"][o:o + ln]


def args(s):
    """Positional arguments of sv.verify_txbodies_hinted / _cpu."""
    return (tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"],
            s["key_begin"], s["key"])


def check(got, want, n_bodies=None):
    """got: the binding's (pair_begin, pair_sig, pair_key, pair_verdict, digests)."""
    pb, ps, pk, pv, dig = got
    assert (np.asarray(pb) == want["pair_begin"]).all()
    assert len(ps) == len(want["pair_sig"]) and (ps == want["pair_sig"]).all()
    assert (pk == want["pair_key"]).all()
    assert (pv == want["verdict"]).all()
    assert (dig == want["digests"]).all()


class _Builder:
    """Bodies with explicit signature / key lists.  A signature is (key row to
    sign with or None for random bytes, hint bytes or None for that key's own
    tail); keys are rows of self.keys (32-byte values)."""

    def __init__(self, rng, signer, n_keys=6):
        self.rng = rng
        self.signer = signer
        self.seeds = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
        pk, _ = signer(self.seeds, np.zeros((n_keys, 32), np.uint8))
        self.pks = [pk[i].tobytes() for i in range(n_keys)]
        self.kind, self.length, self.sigs, self.keys = [], [], [], []

    def wrong_key(self, tail):
        return bytes(self.rng.integers(0, 256, 28, dtype=np.uint8)) + bytes(tail)

    def add(self, kind, length, sigs, keys):
        self.kind.append(kind)
        self.length.append(length)
        self.sigs.append(list(sigs))
        self.keys.append(list(keys))

    def finish(self):
        rng = self.rng
        nb = len(self.kind)
        kind = np.array(self.kind, np.uint8)
        length = np.array(self.length, np.uint32)
        off = np.zeros(nb, np.uint64)
        off[1:] = np.cumsum(length[:-1], dtype=np.uint64)
        blob = rng.integers(0, 256, int(length.sum(dtype=np.uint64)) + 1, dtype=np.uint8)
        sig_begin = np.zeros(nb + 1, np.uint64)
        sig_begin[1:] = np.cumsum([len(x) for x in self.sigs])
        key_begin = np.zeros(nb + 1, np.uint64)
        key_begin[1:] = np.cumsum([len(x) for x in self.keys])
        ns, nk = int(sig_begin[-1]), int(key_begin[-1])
        key = np.zeros((nk, 32), np.uint8)
        for t in range(nb):
            for j, kv in enumerate(self.keys[t]):
                key[int(key_begin[t]) + j] = np.frombuffer(kv, np.uint8)
        hashes = [tp.contents_hash(int(kind[t]), blob[int(off[t]):int(off[t]) + int(length[t])]) for t in range(nb)]
        hint = np.zeros((ns, 4), np.uint8)
        sig = rng.integers(0, 256, (ns, 64), dtype=np.uint8)
        rows, seeds, msgs = [], [], []
        for t in range(nb):
            for j, (signer_row, h) in enumerate(self.sigs[t]):
                i = int(sig_begin[t]) + j
                if signer_row is not None:
                    rows.append(i)
                    seeds.append(self.seeds[signer_row])
                    msgs.append(np.frombuffer(hashes[t], np.uint8))
                hint[i] = np.frombuffer(h if h is not None else self.pks[signer_row][28:], np.uint8)
        valid = {}
        if rows:
            _, made = self.signer(np.array(seeds, np.uint8), np.array(msgs, np.uint8))
            sig[rows] = made
        # valid[i] = the key index signature i verifies under (first listing of its signer in the body)
        for t in range(nb):
            for j, (signer_row, _) in enumerate(self.sigs[t]):
                if signer_row is None:
                    continue
                for q, kv in enumerate(self.keys[t]):
                    if kv == self.pks[signer_row]:
                        valid[int(sig_begin[t]) + j] = int(key_begin[t]) + q
                        break
        return dict(bodies=blob, off=off, len=length, kind=kind, sig_begin=sig_begin, key_begin=key_begin, hint=hint,
                    sig=sig, key=key, nb=nb, ns=ns, nk=nk, valid=valid)


def make_pool(nb, seed, signer, big=False):
    """The mandatory cases (as many as fit in nb), then pool bodies."""
    rng = np.random.default_rng(seed)
    b = _Builder(rng, signer)
    P = b.pks
    shapes = tp.pool_shapes(max(nb, 1), rng, big)
    tail = lambda k: P[k][28:]  # noqa: E731
    case = {
        "no_match": ([(0, b"\x01\x02\x03\x04")], [P[0], P[1]]),
        "multi": ([(0, None), (1, None)], [b.wrong_key(tail(0)), P[0], b.wrong_key(tail(0)), P[1]]),
        # the middle body's signatures carry the hints of keys that only its neighbours list
        "neighbour": ([(2, None)], [P[2]]),
        "neighbour_mid": ([(2, None), (3, None)], [P[4]]),
        "neighbour_hi": ([(3, None)], [P[3]]),
        "dup_key": ([(1, None)], [P[1], P[0], P[1]]),
        "sigs_only": ([(0, None), (None, tail(1))], []),
        "keys_only": ([], [P[0], P[1], P[2]]),
        "empty": ([], []),
        "grid": ([(5, None)] * 2 + [(None, tail(5))] * 18, [P[5]] + [b.wrong_key(tail(5)) for _ in range(19)]),
        "one_byte": ([(None, bytes(x ^ (0x80 if i == j else 0) for i, x in enumerate(tail(0)))) for j in range(4)],
                     [P[0]]),
        "head": ([(None, P[1][:4])], [P[1]]),
    }
    assert P[1][:4] != P[1][28:]
    for t in range(nb):
        kind, length = shapes[t]
        if t < len(CASES):
            sigs, keys = case[CASES[t]]
        else:
            nk = 1 + t % 3
            keys = [P[(t + j) % len(P)] for j in range(nk)]
            sigs = [((t + j % nk) % len(P), None) for j in range(tp.sigs_per_body(t))]
        b.add(kind, length, sigs, keys)
    s = b.finish()
    # the pool's rejects: corrupted signature bytes; a body mutated after signing
    for i in range(4, s["ns"], 9):
        s["sig"][i, 40] ^= 1
        s["valid"].pop(i, None)
    for t in range(len(CASES), nb):
        if t % 13 == 1 and s["len"][t] > 0:
            s["bodies"][int(s["off"][t]) + int(s["len"][t]) // 2] ^= 0x10
            for i in range(int(s["sig_begin"][t]), int(s["sig_begin"][t + 1])):
                s["valid"].pop(i, None)
    return s


def make_sparse(nb, seed, signer, block, max_len=40, one_in=32, keys_per_body=1):
    """nb bodies of 0..max_len bytes, about one in `one_in` with a pair; the
    first body, the last body and the first body of every `block`-body tile have
    one.  Every body lists keys_per_body keys: its signer at position t %
    keys_per_body, random keys elsewhere, and (keys_per_body > 1, every fifth
    body) a "wrong key" with the signer's tail right after the signer.  A body
    with a pair has one signature by its signer (every seventh of them
    corrupted), one body in 16 of the others a signature with a foreign hint.
    Verdicts by construction (s["valid"])."""
    rng = np.random.default_rng(seed)
    n_keys, q = 4, keys_per_body
    seeds = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    kpk, _ = signer(seeds, np.zeros((n_keys, 32), np.uint8))
    kind = rng.integers(0, 3, nb).astype(np.uint8)
    length = rng.integers(0, max_len + 1, nb).astype(np.uint32)
    off = np.zeros(nb, np.uint64)
    off[1:] = np.cumsum(length[:-1], dtype=np.uint64)
    blob = rng.integers(0, 256, int(length.sum(dtype=np.uint64)) + 1, dtype=np.uint8)
    has = rng.integers(0, one_in, nb) == 0
    has[0] = has[nb - 1] = True
    has[::block] = True
    stray = (~has) & (rng.integers(0, 16, nb) == 0)
    counts = (has | stray).astype(np.uint64)
    sig_begin = np.zeros(nb + 1, np.uint64)
    sig_begin[1:] = np.cumsum(counts)
    key_begin = np.arange(nb + 1, dtype=np.uint64) * np.uint64(q)
    krow = np.arange(nb) % n_keys
    pos = np.arange(nb) % q
    key = rng.integers(0, 256, (nb, q, 32), dtype=np.uint8)
    key[np.arange(nb), pos] = kpk[krow]
    if q > 1:
        twin = np.arange(0, nb, 5)
        key[twin, (pos[twin] + 1) % q, 28:] = kpk[krow[twin]][:, 28:]
    key = key.reshape(nb * q, 32)
    ns = int(sig_begin[-1])
    owner = np.repeat(np.arange(nb), counts.astype(np.int64))
    signed = owner[has[owner]]
    msgs = np.array([np.frombuffer(tp.contents_hash(int(kind[t]), blob[int(off[t]):int(off[t]) + int(length[t])]),
                                   np.uint8) for t in signed], np.uint8).reshape(len(signed), 32)
    _, made = signer(seeds[krow[signed]], msgs)
    sig = rng.integers(0, 256, (ns, 64), dtype=np.uint8)
    hint = np.zeros((ns, 4), np.uint8)
    rows = np.nonzero(has[owner])[0]
    sig[rows] = made
    hint[rows] = kpk[krow[signed]][:, 28:]
    other = np.nonzero(~has[owner])[0]
    hint[other] = kpk[krow[owner[other]]][:, 28:] ^ 0x55  # (the tail of no key the pool signs with)
    valid = {int(i): int(owner[i]) * q + int(pos[owner[i]]) for i in rows}
    for i in rows[::7]:
        sig[i, 33] ^= 4
        valid.pop(int(i))
    return dict(bodies=blob, off=off, len=length, kind=kind, sig_begin=sig_begin, key_begin=key_begin,
                hint=np.ascontiguousarray(hint), sig=sig, key=np.ascontiguousarray(key), nb=nb, ns=ns, nk=nb * q,
                valid=valid)


def expected_fast(s):
    """expected() for make_sparse sets, vectorised (the same contract: each
    signature against the keys of its body, pairs in signature-then-key order),
    digests by hashlib, verdicts by construction."""
    nb = s["nb"]
    counts = np.diff(s["sig_begin"].astype(np.int64))
    owner = np.repeat(np.arange(nb), counts)
    q = s["nk"] // nb
    assert (np.diff(s["key_begin"].astype(np.int64)) == q).all()
    tails = s["key"].reshape(nb, q, 32)[:, :, 28:]
    match = (tails[owner] == s["hint"][:, None, :]).all(axis=2)  # (ns, q)
    si, kj = np.nonzero(match)  # row-major: signature, then key
    ps = si.astype(np.uint32)
    pk = (owner[si] * q + kj).astype(np.uint32)
    per_body = np.bincount(owner[si], minlength=nb)
    begin = np.zeros(nb + 1, np.uint64)
    begin[1:] = np.cumsum(per_body)
    v = np.array([1 if s["valid"].get(int(i)) == int(k) else 0 for i, k in zip(ps, pk)], np.uint8)
    digests = np.array([np.frombuffer(tp.contents_hash(int(s["kind"][t]), body(s, t)), np.uint8) for t in range(nb)],
                       np.uint8).reshape(nb, 32)
    return dict(pair_begin=begin, pair_sig=ps, pair_key=pk, verdict=v, digests=digests)
