"""Input builder and plain-Python contract of the check entry points
(sv_ed25519_check_txbodies*; test_txchecks_cpu.py, test_gpu_txchecks.py).

Builder collects bodies one at a time: candidate key rows, decorated
signatures and checks (needed weight + signer list), and lays them out in the
CSR tables of the C-ABI.  Signatures are made over the bodies' contents hashes
in one signer batch (txbodies_pool.pysign_signer / device_signer).

The reference is txset_gen.Checker, which restates SignatureChecker.cpp: run
per check with a fresh `used` list over the signers of the first three stages
(type-3 signers are the caller's).  The Checker keeps its weight to itself, so
replay() below restates the accumulation once more to give check_weight; its
ok and marks are asserted equal to the Checker's on every check it is used on.
Nothing here comes from the code under test.
"""
import hashlib

import numpy as np

import txbodies_pool as tp
import txset_gen as tg

ED, PRE, HX, SP = tg.ED25519, tg.PRE_AUTH_TX, tg.HASH_X, tg.SIGNED_PAYLOAD


def seed_of(i):
    return hashlib.sha256(b"txchecks seed %d" % i).digest()


class Body:
    def __init__(self, kind, data):
        self.kind, self.data = kind, bytes(data)
        self.hash = tp.contents_hash(kind, self.data)
        self.keys, self.sigs, self.checks = [], [], []

    # --- keys: return the body-local index
    def key_ed(self, seed):
        self.keys.append(("ed", seed))
        return len(self.keys) - 1

    def key_wrong(self, seed):
        """28 random bytes + the tail (hint) of `seed`'s public key."""
        self.keys.append(("wrong", seed))
        return len(self.keys) - 1

    def key_raw(self, row):
        assert len(row) == 32
        self.keys.append(("raw", bytes(row)))
        return len(self.keys) - 1

    def key_hashx(self, preimage):
        return self.key_raw(hashlib.sha256(bytes(preimage)).digest())

    def key_preauth(self):
        return self.key_raw(self.hash)

    # --- signatures: return the body-local index
    def sig_ed(self, seed, corrupt=False, length=64, msg=None, hint=None):
        self.sigs.append(dict(kind="ed", seed=seed, corrupt=corrupt, length=length, msg=msg, hint=hint))
        return len(self.sigs) - 1

    def sig_raw(self, hint, data):
        assert len(hint) == 4 and len(data) <= 64
        self.sigs.append(dict(kind="raw", hint=bytes(hint), data=bytes(data)))
        return len(self.sigs) - 1

    def sig_hashx(self, preimage, hint=None):
        h = hashlib.sha256(bytes(preimage)).digest()[28:] if hint is None else hint
        return self.sig_raw(h, preimage)

    def check(self, needed, signers):
        """signers: [(type, weight, body-local key index)] in list order."""
        self.checks.append((int(needed), [tuple(g) for g in signers]))
        return len(self.checks) - 1


class Builder:
    def __init__(self, seed=1):
        self.rng = np.random.default_rng(seed)
        self.bodies = []

    def body(self, kind=None, length=None):
        kind = int(self.rng.integers(0, 3)) if kind is None else kind
        length = int(self.rng.integers(0, 200)) if length is None else length
        b = Body(kind, self.rng.integers(0, 256, length, dtype=np.uint8).tobytes())
        self.bodies.append(b)
        return b

    def finish(self, signer):
        B = self.bodies
        nb = len(B)
        # one signer batch: every seed once (its public key), then every signature
        seeds_used = sorted({k[1] for b in B for k in b.keys if k[0] in ("ed", "wrong")}
                            | {s["seed"] for b in B for s in b.sigs if s["kind"] == "ed"})
        req = [(sd, bytes(32)) for sd in seeds_used]
        for b in B:
            for s in b.sigs:
                if s["kind"] == "ed":
                    s["req"] = len(req)
                    req.append((s["seed"], b.hash if s["msg"] is None else s["msg"]))
        pks = {}
        made = None
        if req:
            sd = np.array([np.frombuffer(seed_of(r[0]), np.uint8) for r in req], np.uint8)
            ms = np.array([np.frombuffer(r[1], np.uint8) for r in req], np.uint8)
            pk, made = signer(sd, ms)
            pks = {s: pk[i].tobytes() for i, s in enumerate(seeds_used)}
        kind = np.array([b.kind for b in B], np.uint8)
        length = np.array([len(b.data) for b in B], np.uint32)
        off = np.zeros(nb, np.uint64)
        if nb:
            off[1:] = np.cumsum(length[:-1], dtype=np.uint64)
        blob = np.frombuffer(b"".join(b.data for b in B) + b"\0", np.uint8).copy()
        csr = lambda counts: np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)  # noqa: E731
        sig_begin = csr([len(b.sigs) for b in B])
        key_begin = csr([len(b.keys) for b in B])
        check_begin = csr([len(b.checks) for b in B])
        ns, nk, nc = int(sig_begin[-1]), int(key_begin[-1]), int(check_begin[-1])
        key = np.zeros((nk, 32), np.uint8)
        hint = np.zeros((ns, 4), np.uint8)
        sig = np.zeros((ns, 64), np.uint8)
        sig_len = np.full(ns, 64, np.uint8)
        needed, signer_counts, gt, gw, gk = [], [], [], [], []
        for t, b in enumerate(B):
            rows = []
            for k in b.keys:
                if k[0] == "ed":
                    rows.append(pks[k[1]])
                elif k[0] == "wrong":
                    rows.append(self.rng.integers(0, 256, 28, dtype=np.uint8).tobytes() + pks[k[1]][28:])
                else:
                    rows.append(k[1])
            b.key_rows = rows
            for j, r in enumerate(rows):
                key[int(key_begin[t]) + j] = np.frombuffer(r, np.uint8)
            b.sig_rows = []
            for j, s in enumerate(b.sigs):
                i = int(sig_begin[t]) + j
                if s["kind"] == "ed":
                    raw = bytearray(made[s["req"]].tobytes())
                    if s["corrupt"]:
                        raw[40] ^= 1
                    data = bytes(raw[:s["length"]])
                    h = pks[s["seed"]][28:] if s["hint"] is None else s["hint"]
                else:
                    data, h = s["data"], s["hint"]
                hint[i] = np.frombuffer(h, np.uint8)
                sig[i, :len(data)] = np.frombuffer(data, np.uint8)
                sig_len[i] = len(data)
                b.sig_rows.append({"hint": bytes(h), "sig": data})
            for need, signers in b.checks:
                needed.append(need)
                signer_counts.append(len(signers))
                for ty, w, k in signers:
                    gt.append(ty)
                    gw.append(w)
                    gk.append(int(key_begin[t]) + k)
        return dict(bodies=blob, off=off, len=length, kind=kind, nb=nb, sig_begin=sig_begin, key_begin=key_begin,
                    hint=hint, sig=sig, key=key, ns=ns, nk=nk, sig_len=sig_len, check_begin=check_begin,
                    check_needed=np.array(needed, np.int32).reshape(-1), signer_begin=csr(signer_counts),
                    signer_type=np.array(gt, np.uint8).reshape(-1), signer_weight=np.array(gw, np.uint32).reshape(-1),
                    signer_key=np.array(gk, np.uint32).reshape(-1), nc=nc, ng=len(gt), B=B,
                    digests=np.array([np.frombuffer(b.hash, np.uint8) for b in B], np.uint8).reshape(nb, 32))


def args(s):
    """Positional arguments of sv.check_txbodies / check_txbodies_cpu."""
    return (tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"],
            s["key_begin"], s["key"], s["check_begin"], s["check_needed"], s["signer_begin"], s["signer_type"],
            s["signer_weight"], s["signer_key"])


def oracle_verify(oracle):
    cache = {}

    def verify(key, sig, msg):
        k = (key, sig, msg)
        if k not in cache:
            cache[k] = oracle.oracle_ed25519_verify(sig, msg, len(msg), key) == 0
        return cache[k]
    return verify


def replay_check(protocol, contents_hash, sigs, signers, needed, verify):
    """(ok, weight, used mask) of one check over the first three stages: the
    accumulation restated for the weight; ok and the marks must equal
    txset_gen.Checker's."""
    signers = [g for g in signers if g["type"] != SP]
    ck = tg.Checker(protocol, contents_hash, sigs, verify)
    ok = ck.check([dict(g) for g in signers], needed)
    mask = sum(1 << i for i, u in enumerate(ck.used) if u)
    clamp = (lambda w: min(w, 255)) if protocol >= 10 else (lambda w: w)
    total, done, used = 0, False, 0
    for g in signers:
        if g["type"] == PRE and g["key"] == contents_hash and not done:
            total += clamp(g["weight"])
            done = total >= needed
    for ty in (HX, ED):
        rest = [g for g in signers if g["type"] == ty]
        for i, s in enumerate(sigs):
            if done:
                break
            for g in rest:
                if s["hint"] != g["key"][28:]:
                    continue
                if ty == HX:
                    hit = hashlib.sha256(s["sig"]).digest() == g["key"]
                else:
                    hit = len(s["sig"]) == 64 and verify(g["key"], s["sig"], contents_hash)
                if hit:
                    used |= 1 << i
                    total += clamp(g["weight"])
                    done = total >= needed
                    rest.remove(g)
                    break
    assert (done, used) == (bool(ok), mask), "the restated accumulation disagrees with txset_gen.Checker"
    return int(done), min(total, 0xffffffff), used


def expected(s, verify, protocol=21):
    """-> (check_ok, check_weight, check_used) by the Python replay."""
    ok, weight, used = [], [], []
    for b in s["B"]:
        for need, signers in b.checks:
            gs = [{"type": ty, "key": b.key_rows[k], "weight": w, "payload": b""} for ty, w, k in signers]
            o, w, u = replay_check(protocol, b.hash, b.sig_rows, gs, need, verify)
            ok.append(o)
            weight.append(w)
            used.append(u)
    return (np.array(ok, np.uint8).reshape(-1), np.array(weight, np.uint32).reshape(-1),
            np.array(used, np.uint64).reshape(-1))


def assert_equal(got, want, s=None):
    ok, weight, used = got[:3]
    assert (ok == want[0]).all(), (ok.tolist(), want[0].tolist())
    assert (weight == want[1]).all(), (weight.tolist(), want[1].tolist())
    assert (used == want[2]).all(), (used.tolist(), want[2].tolist())
    if s is not None and len(got) > 3:
        assert (got[3] == s["digests"]).all()


# ----------------------------------------------------------------- the edge cases
def edge_cases(bld):
    """Adds the issue's edge cases to `bld`, one tiny body each (the zero-count
    trio is three bodies); returns {name: (first check index, by-hand
    expectation [(ok, weight, mask), ...] at protocol 21 or None)}."""
    out = {}
    nc = lambda: sum(len(b.checks) for b in bld.bodies)  # noqa: E731

    def case(name, hand=None):
        out[name] = (nc(), hand)
        return bld.body(length=int(bld.rng.integers(1, 120)))

    # early exit: three valid signatures, needed reached by the second / unreachable
    b = case("early_exit", [(1, 2, 0b011), (0, 3, 0b111)])
    k = [b.key_ed(s) for s in (1, 2, 3)]
    for s in (1, 2, 3):
        b.sig_ed(s)
    b.check(2, [(ED, 1, x) for x in k])
    b.check(1000, [(ED, 1, x) for x in k])
    # erasure: the same decorated signature twice, one signer
    b = case("erase_same_sig", [(0, 1, 0b01)])
    k0 = b.key_ed(1)
    b.sig_ed(1)
    b.sig_ed(1)
    b.check(2, [(ED, 1, k0)])
    # one key index listed twice (weights 1 then 255, needed 2), the signature twice
    b = case("erase_dup_signer", [(1, 256, 0b11)])
    k0 = b.key_ed(1)
    b.sig_ed(1)
    b.sig_ed(1)
    b.check(2, [(ED, 1, k0), (ED, 255, k0)])
    # a hint collision with a wrong key (verdict 0) listed before the right key
    b = case("collision", [(1, 7, 0b1)])
    kw, kr = b.key_wrong(4), b.key_ed(4)
    b.sig_ed(4)
    b.check(7, [(ED, 9, kw), (ED, 7, kr)])
    # signer order opposite to key order
    b = case("reverse_order", [(1, 30, 0b011)])
    k = [b.key_ed(s) for s in (1, 2, 3)]
    for s in (1, 2, 3):
        b.sig_ed(s)
    b.check(30, [(ED, 40, k[2]), (ED, 20, k[1]), (ED, 10, k[0])])
    # clamp: weight 300, needed 256
    b = case("clamp", [(0, 255, 0b1)])
    k0 = b.key_ed(1)
    b.sig_ed(1)
    b.check(256, [(ED, 300, k0)])
    # needed 0: no match is false, one match is true
    b = case("needed_zero", [(0, 0, 0), (1, 5, 0b1), (0, 0, 0)])
    k0, k1 = b.key_ed(1), b.key_ed(2)
    b.sig_ed(1)
    b.check(0, [(ED, 5, k1)])
    b.check(0, [(ED, 5, k0)])
    b.check(-3, [(ED, 5, k1)])
    # zero counts: no signers; no signatures; a body without checks between two that have some
    b = case("no_signers", [(0, 0, 0)])
    b.key_ed(1)
    b.sig_ed(1)
    b.check(0, [])
    b = case("no_signatures", [(0, 0, 0)])
    b.check(1, [(ED, 1, b.key_ed(1))])
    b = case("no_checks", [])
    b.key_ed(1)
    b.sig_ed(1)
    b = case("after_no_checks", [(1, 1, 0b1)])
    k0 = b.key_ed(2)
    b.sig_ed(2)
    b.check(1, [(ED, 1, k0)])
    # PRE_AUTH_TX: alone reaching needed; not reaching it, carried into an ED25519 match
    b = case("preauth", [(1, 3, 0), (1, 5, 0b1), (0, 2, 0b1)])
    kp, ke, kx = b.key_preauth(), b.key_ed(1), b.key_raw(bytes(range(32)))
    b.sig_ed(1)
    b.check(3, [(ED, 2, ke), (PRE, 3, kp)])
    b.check(5, [(ED, 2, ke), (PRE, 3, kp)])
    b.check(5, [(ED, 2, ke), (PRE, 3, kx)])  # (a pre-auth signer for another transaction)
    # HASH_X: preimages of 0, 1, 55, 56 and 64 bytes
    for n in (0, 1, 55, 56, 64):
        pre = bytes((7 * i + n) & 255 for i in range(n))
        b = case("hashx_%d" % n, [(1, 4, 0b1)])
        kh = b.key_hashx(pre)
        b.sig_hashx(pre)
        b.check(4, [(HX, 4, kh)])
    # the right preimage with a wrong hint
    b = case("hashx_wrong_hint", [(0, 0, 0)])
    pre = b"the preimage"
    kh = b.key_hashx(pre)
    b.sig_hashx(pre, hint=b"\1\2\3\4")
    b.check(1, [(HX, 1, kh)])
    # weight carried over from the HASH_X pass into the ED25519 pass (the ed25519
    # signature comes first in the body: the passes, not the signatures, order the marks)
    b = case("hashx_carry", [(1, 5, 0b11), (1, 3, 0b10)])
    pre = b"x" * 33
    ke, kh = b.key_ed(1), b.key_hashx(pre)
    b.sig_ed(1)
    b.sig_hashx(pre)
    b.check(5, [(ED, 2, ke), (HX, 3, kh)])
    b.check(3, [(ED, 2, ke), (HX, 3, kh)])
    # a 63-byte signature whose hint matches an ED25519 signer
    b = case("short_sig", [(0, 0, 0)])
    k0 = b.key_ed(1)
    b.sig_ed(1, length=63)
    b.check(1, [(ED, 1, k0)])
    # a type-3 signer present: skipped, the state is that of the first three stages
    b = case("payload_signer", [(0, 1, 0b01)])
    k0, k1 = b.key_ed(1), b.key_ed(2)
    b.sig_ed(1)
    b.sig_ed(2)
    b.check(3, [(SP, 2, k1), (ED, 1, k0)])
    return out


def random_pool(bld, nb, max_sigs=20, check_counts=None):
    """nb bodies with 0..max_sigs signatures and 1..6 checks each (or, with
    check_counts, one body per entry with that many checks)."""
    rng = bld.rng
    if check_counts is not None:
        nb = len(check_counts)
    for t in range(nb):
        b = bld.body(length=int(rng.integers(0, 300)))
        seeds = [int(x) for x in rng.choice(np.arange(1, 9), size=int(rng.integers(1, 5)), replace=False)]
        ked = [b.key_ed(s) for s in seeds]
        kinds = [(ED, k) for k in ked]
        if rng.random() < 0.4:
            kinds.append((ED, b.key_wrong(seeds[0])))
        pres = []
        if rng.random() < 0.4:
            pre = rng.integers(0, 256, int(rng.integers(0, 65)), dtype=np.uint8).tobytes()
            pres.append(pre)
            kinds.append((HX, b.key_hashx(pre)))
        if rng.random() < 0.3:
            kinds.append((PRE, b.key_preauth() if rng.random() < 0.6 else b.key_raw(bytes(32))))
        if rng.random() < 0.2:
            kinds.append((ED, ked[0]))  # the same key index listed twice
        if rng.random() < 0.2:
            kinds.append((SP, ked[-1]))
        n_sigs = 0 if t % 9 == 4 else (max_sigs if t % 11 == 0 else int(rng.integers(0, 6)))
        for _ in range(n_sigs):
            r = rng.random()
            if r < 0.55:
                b.sig_ed(seeds[int(rng.integers(0, len(seeds)))])
            elif r < 0.65:
                b.sig_ed(seeds[0], corrupt=True)
            elif r < 0.75:
                b.sig_ed(int(rng.integers(9, 12)))  # a signer the body does not list
            elif r < 0.85 and pres:
                b.sig_hashx(pres[0])
            elif r < 0.92:
                b.sig_ed(seeds[0], length=63)
            else:
                b.sig_raw(rng.integers(0, 256, 4, dtype=np.uint8).tobytes(),
                          rng.integers(0, 256, 64, dtype=np.uint8).tobytes())
        for _ in range(int(rng.integers(1, 7)) if check_counts is None else check_counts[t]):
            order = rng.permutation(len(kinds))[:int(rng.integers(0, len(kinds) + 1))]
            b.check(int(rng.choice([0, 1, 2, 3, 255, 256, 400])),
                    [(kinds[i][0], int(rng.choice([1, 1, 2, 100, 255, 300])), kinds[i][1]) for i in order])


def seam_counts(n_checks):
    """Checks per body summing to n_checks: runs of bodies without checks, and
    bodies of up to 11 checks, one of them across every 256-check boundary."""
    pattern = (3, 0, 0, 1, 5, 0, 2, 9, 1, 0, 0, 0, 4, 7)
    out, total, i = [], 0, 0
    while total < n_checks:
        c = pattern[i % len(pattern)]
        edge = (total // 256 + 1) * 256
        if total < edge <= total + 9 and edge < n_checks:
            c = edge - total + 2  # this body's checks straddle the boundary
        c = min(c, n_checks - total)
        out.append(c)
        total += c
        i += 1
    return out + [0, 0]


def sparse_tables(s, checks_per_body=1, signers_per_check=None):
    """Check tables over a txpairs_pool.make_sparse set, vectorised: every body
    gets checks_per_body checks of needed 1 whose signers are the body's keys
    in order (or signers_per_check times its first key), ED25519, weight 1.
    Returns (tables dict, (ok, weight, used) by construction): a body's checks
    succeed, with its one signature marked, iff that signature verifies under
    one of the listed keys (s["valid"])."""
    nb = s["nb"]
    q = s["nk"] // nb
    nc = nb * checks_per_body
    per = q if signers_per_check is None else signers_per_check
    body_of = np.repeat(np.arange(nb, dtype=np.uint64), checks_per_body)
    if signers_per_check is None:
        gk = (body_of[:, None] * np.uint64(q) + np.arange(q, dtype=np.uint64)[None, :]).reshape(-1)
    else:
        # (the key the body's signature is made with, listed several times)
        gk = np.repeat(body_of * np.uint64(q) + (body_of % np.uint64(q)), per)
    tables = dict(check_begin=np.arange(nb + 1, dtype=np.uint64) * np.uint64(checks_per_body),
                  check_needed=np.ones(nc, np.int32), signer_begin=np.arange(nc + 1, dtype=np.uint64) * np.uint64(per),
                  signer_type=np.zeros(nc * per, np.uint8), signer_weight=np.ones(nc * per, np.uint32),
                  signer_key=gk.astype(np.uint32))
    good = np.zeros(nb, bool)
    first = s["sig_begin"][:-1].astype(np.int64)
    has = np.diff(s["sig_begin"].astype(np.int64)) > 0
    for t in np.nonzero(has)[0]:
        k = s["valid"].get(int(first[t]))
        good[t] = k is not None and (signers_per_check is None or k == int(t) * q + int(t) % q)
    ok = np.repeat(good, checks_per_body).astype(np.uint8)
    return tables, (ok, ok.astype(np.uint32), ok.astype(np.uint64))


def sparse_args(s, tables):
    return (tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"],
            s["key_begin"], s["key"], tables["check_begin"], tables["check_needed"], tables["signer_begin"],
            tables["signer_type"], tables["signer_weight"], tables["signer_key"])
