"""Model and input builder of the account store and the ledger forms
(sv_set_account_store, sv_ed25519_check_txbodies_ledger*; test_txledger_cpu.py,
test_gpu_txledger.py).

The model of the store is a plain dict: account ID (32 bytes) -> (thresholds,
[(type, weight, key bytes, payload or None), ...]).  batch() lays accounts out
as sv_account_store_upsert's arrays, check_read() compares what
account_store_read returned with the dict.

LBuilder extends txaccounts_pool.ABuilder: every account is a STORE account
(named by ID in the ledger call; its master key is its ID, so store accounts
have distinct master keys), a LOCAL account (a pseudo-account of the call) or
ABSENT (an ID the store does not hold: in the twin's table the empty account --
master weight 0, no signers, thresholds 0 -- that include/stellar_sigverify.h
puts in its place).  finish() is ABuilder's: the by-account twin's input on the
COMBINED table, which is the oracle's input.  ledger() derives the ledger call's
input from the builder's own objects: the local table, bacct with
BACCT_BY_ID, bacct_id, and the bacct_found the definition gives.  Nothing here
comes from the code under test.
"""
import hashlib
import struct

import numpy as np

import txaccounts_pool as ap
import txbodies_pool as tp
import txpayload_pool as pl

ED, PRE, HX, SP = ap.ED, ap.PRE, ap.HX, ap.SP
BY_ID = 0xFFFFFFFF
STORE, LOCAL, ABSENT = "store", "local", "absent"


# ------------------------------------------------------------------ the store's model
def rand_id(rng):
    return rng.integers(0, 256, 32, dtype=np.uint8).tobytes()


def rand_account(rng, n_signers, payloads=False):
    """(thresholds, signers) with n_signers signers; payloads: all of type 3."""
    signers = []
    for _ in range(n_signers):
        ty = SP if payloads else int(rng.integers(0, 3))
        p = rng.integers(0, 256, int(rng.integers(1, 65)), dtype=np.uint8).tobytes() if ty == SP else None
        signers.append((ty, int(rng.integers(0, 2 ** 32)), rand_id(rng), p))
    return tuple(int(x) for x in rng.integers(0, 256, 4)), signers


def batch(rows):
    """[(id, (thresholds, signers)), ...] -> the keyword arguments of sv.account_store_upsert."""
    key = np.zeros((len(rows), 32), np.uint8)
    thr = np.zeros((len(rows), 4), np.uint8)
    begin, gt, gw, gk, gp, pay, plen = [0], [], [], [], [], [], []
    for i, (aid, (t, signers)) in enumerate(rows):
        key[i] = np.frombuffer(aid, np.uint8)
        thr[i] = t
        for ty, w, k, p in signers:
            gt.append(ty)
            gw.append(w)
            gk.append(np.frombuffer(k, np.uint8))
            gp.append(len(pay) if p is not None else 0xFFFFFFFF)
            if p is not None:
                row = np.zeros(64, np.uint8)
                row[:len(p)] = np.frombuffer(p, np.uint8)
                pay.append(row)
                plen.append(len(p))
        begin.append(len(gt))
    return dict(acct_key=key, acct_thresholds=thr, asigner_begin=np.array(begin, np.uint64),
                asigner_type=np.array(gt, np.uint8), asigner_weight=np.array(gw, np.uint32),
                asigner_key=np.array(gk, np.uint8).reshape(-1, 32), asigner_payload=np.array(gp, np.uint32),
                apayload=np.array(pay, np.uint8).reshape(-1, 64), apayload_len=np.array(plen, np.uint8))


def upsert(sv, model, rows):
    """Upserts `rows` and, once the call returned, the model."""
    sv.account_store_upsert(**batch(rows))
    for aid, acct in rows:
        model[aid] = acct


def erase(sv, model, ids):
    sv.account_store_erase(np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32))
    for aid in ids:
        model.pop(aid, None)


def check_read(got, model, ids):
    """account_store_read's rows of `ids` against the model: found, thresholds, the signers in order, zeros
    behind them (no stale signer) and for an ID that is not held."""
    assert len(got.found) == len(ids)
    for i, aid in enumerate(ids):
        acct = model.get(aid)
        assert int(got.found[i]) == (acct is not None), i
        thr, signers = acct if acct is not None else ((0, 0, 0, 0), [])
        assert tuple(int(x) for x in got.thresholds[i]) == tuple(thr), i
        assert int(got.n_signers[i]) == len(signers), i
        for j in range(20):
            if j >= len(signers):
                assert not got.signer_type[i, j] and not got.signer_weight[i, j] and not got.signer_key[i, j].any()
                assert not got.signer_payload[i, j].any() and not got.signer_payload_len[i, j], (i, j)
                continue
            ty, w, k, p = signers[j]
            assert (int(got.signer_type[i, j]), int(got.signer_weight[i, j])) == (ty, w), (i, j)
            assert got.signer_key[i, j].tobytes() == k, (i, j)
            p = p or b""
            assert int(got.signer_payload_len[i, j]) == len(p), (i, j)
            assert got.signer_payload[i, j].tobytes() == p + bytes(64 - len(p)), (i, j)


def read_all(sv, model, ids, device=-1):
    check_read(sv.account_store_read(np.frombuffer(b"".join(ids), np.uint8).reshape(-1, 32), device=device), model,
               ids)


def semantic_sequence(sv, device=-1, seed=3):
    """The fixed sequence of upserts, overwrites and erases of the store tests, the store read back (from
    `device`) against the model after every step.  -> (model, ids, the stats the model implies)."""
    rng = np.random.default_rng(seed)
    sv.set_account_store(16, 2, 4)
    model, ids = {}, [rand_id(rng) for _ in range(8)]
    check = lambda: read_all(sv, model, ids, device)  # noqa: E731
    check()
    upsert(sv, model, [(ids[i], rand_account(rng, 20 if i == 0 else i)) for i in range(6)])
    check()
    upsert(sv, model, [(ids[0], rand_account(rng, 1))])  # 20 -> 1 signers: no stale signer
    check()
    for _ in range(50):  # two payload rows survive 50 overwrites of one type-3 signer
        upsert(sv, model, [(ids[1], rand_account(rng, 1, payloads=True))])
    check()
    # a duplicate ID inside one batch: the last row wins
    upsert(sv, model, [(ids[6], rand_account(rng, 3)), (ids[2], rand_account(rng, 2)), (ids[6], rand_account(rng, 5))])
    assert len(model[ids[6]][1]) == 5
    check()
    erase(sv, model, [ids[3], ids[7], ids[3]])  # ids[7] never was there, ids[3] twice
    check()
    want = dict(capacity=16, accounts=6, payload_capacity=2, payloads=1, local_accounts=4, index_slots=32,
                upsert_calls=53, inserted=7, replaced=52, erase_calls=1, erased=1, erase_absent=2)
    return model, ids, want


def acct_hash(aid, seed):
    """csrc/accthash.h restated: the seeded mix of all eight ID words."""
    m = (1 << 64) - 1
    h = seed & m
    for w in struct.unpack("<8I", aid):
        h = ((h ^ w) * 0x9E3779B97F4A7C15) & m
        h ^= h >> 29
    h = (h * 0xD6E8FEB86659FD93) & m
    return h ^ (h >> 32)


WRAP_SEED = 12345  # SV_ACCT_STORE_SEED of the smallest-index tests


def wrapping_ids(seed=WRAP_SEED, slots=8):
    """4 IDs for a store of 4 accounts (8 index slots) under `seed`, chosen by trial on the restated hash: three
    whose home is the LAST slot -- inserted in this order they occupy slots 7, 0 and 1, a probe run that wraps --
    and one at home in slot 3.  ids[1] is the middle of the run."""
    rng = np.random.default_rng(17)
    run, other = [], None
    while len(run) < 3 or other is None:
        aid = rand_id(rng)
        home = acct_hash(aid, seed) & (slots - 1)
        if home == slots - 1 and len(run) < 3:
            run.append(aid)
        elif home == 3 and other is None:
            other = aid
    return run + [other]


def last_byte_ids(rng, n=64):
    base = bytearray(rand_id(rng))
    out = []
    for i in range(n):
        base[31] = i
        out.append(bytes(base))
    return out


# ------------------------------------------------------------------ ledger calls
class LBuilder(ap.ABuilder):
    def __init__(self, seed=1):
        super().__init__(seed)
        self.where = []

    def account(self, master, thresholds, signers=(), where=STORE):
        if where == ABSENT:
            assert tuple(thresholds) == (0, 0, 0, 0) and not signers
        self.where.append(where)
        return super().account(master, thresholds, signers)

    def absent(self, tag):
        return self.account(ap.raw(hashlib.sha256(b"absent %d" % tag).digest()), (0, 0, 0, 0), where=ABSENT)

    def model(self):
        """The store's content: the STORE accounts by ID."""
        m = {}
        for a, w in zip(self.accounts, self.where):
            if w != STORE:
                continue
            aid = ap.key_bytes(a.master)
            assert aid not in m, "two store accounts with one ID"
            m[aid] = (a.thresholds, [(ty, wt, ap.key_bytes(k), p) for ty, wt, k, p in a.signers])
        assert not any(ap.key_bytes(a.master) in m for a, w in zip(self.accounts, self.where) if w == ABSENT)
        return m

    def ledger(self, s):
        """The ledger call's arrays for the finished set `s`: the local table, bacct / bacct_id, found."""
        local = [i for i, w in enumerate(self.where) if w == LOCAL]
        at = {a: j for j, a in enumerate(local)}
        t = batch([(ap.key_bytes(self.accounts[a].master),
                    (self.accounts[a].thresholds,
                     [(ty, wt, ap.key_bytes(k), p) for ty, wt, k, p in self.accounts[a].signers])) for a in local])
        ne = len(s["bacct"])
        bacct = np.zeros(ne, np.uint32)
        ids = np.zeros((ne, 32), np.uint8)
        found = np.zeros(ne, np.uint8)
        for e, a in enumerate(s["bacct"]):
            a = int(a)
            if self.where[a] == LOCAL:
                bacct[e], found[e] = at[a], 1
                ids[e] = 0xEE  # (not read)
            else:
                bacct[e], found[e] = BY_ID, self.where[a] == STORE
                ids[e] = np.frombuffer(ap.key_bytes(self.accounts[a].master), np.uint8)
        t.update(bacct=bacct, bacct_id=ids, found=found, nl=len(local), nls=len(t["asigner_type"]),
                 nlp=len(t["apayload_len"]))
        return t


LEDGER_KEYS = ("acct_key", "acct_thresholds", "asigner_begin", "asigner_type", "asigner_weight", "asigner_key",
               "asigner_payload", "apayload", "apayload_len")


def args(s, lg):
    """Positional arguments of sv.check_txbodies_ledger_cpu for set `s` and its ledger arrays `lg`."""
    return ((tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"])
            + tuple(lg[k] for k in LEDGER_KEYS)
            + (s["bacct_begin"], lg["bacct"], lg["bacct_id"], s["check_begin"], s["check_acct"], s["check_level"],
               s["acheck_needed"]))


def edge_cases(bld):
    """The edge set of txaccounts_pool.edge_cases restated for the ledger forms: store accounts by ID (distinct
    master keys, at most 20 signers), the two pseudo-account kinds as local accounts, an ID the store does not
    hold.  -> {name: (first check index, by-hand [(ok, weight, mask), ...] at protocol 21)}."""
    out = {}
    nc = lambda: sum(len(b.achecks) for b in bld.bodies)  # noqa: E731
    ed, raw = ap.ed, ap.raw

    def case(name, hand):
        out[name] = (nc(), hand)
        return bld.body(length=int(bld.rng.integers(1, 120)))

    # master weight 0: the master is no signer and no candidate
    a = bld.account(ed(11), (0, 1, 1, 1), [(ED, 1, ed(2))])
    b = case("master_weight_zero", [(0, 0, 0), (1, 1, 0b10)])
    b.sig_ed(11)
    b.acheck(b.use(a), 1)
    b = bld.body(length=20)
    b.sig_ed(11)
    b.sig_ed(2)
    b.acheck(b.use(a), 1)
    # levels 1, 2, 3 pick their own threshold
    a = bld.account(ed(12), (2, 1, 2, 3))
    b = case("levels", [(1, 2, 1), (1, 2, 1), (0, 2, 1)])
    p = b.use(a)
    b.sig_ed(12)
    for level in (1, 2, 3):
        b.acheck(p, level)
    # the extra-signer pseudo-account, local: master weight 0, weight 1 each, needed = their count
    short, full = pl.payload_of(3), pl.payload_of(64)
    x = bld.account(raw(bytes(32)), (0, 0, 0, 0), [(ED, 1, ed(3)), (SP, 1, ed(4), short), (SP, 1, ed(4), full)],
                    where=LOCAL)
    b = case("extra_signers", [(1, 3, 0b111), (1, 2, 0b1000)])
    b.sig_payload(4, full)
    b.sig_ed(3)
    b.sig_payload(4, short)
    b.sig_ed(12)
    b.acheck(b.use(x), 0, 3)
    b.acheck(b.use(a), 1)  # (a store account beside the local one)
    b = case("extra_signers_one_missing", [(0, 2, 0b11)])
    b.sig_payload(4, full)
    b.sig_ed(3)
    b.acheck(b.use(x), 0, 3)
    # the no-account pseudo-account, local: master weight 1, no signers, needed 0
    n = bld.account(ed(5), (1, 0, 0, 0), where=LOCAL)
    b = case("no_account", [(1, 1, 1), (0, 0, 0)])
    b.sig_ed(5)
    b.acheck(b.use(n), 0, 0)
    b = bld.body(length=9)
    b.sig_ed(6)
    b.acheck(b.use(n), 0, 0)
    # a store account with type-3 signers (its payload rows live in the store)
    sp = bld.account(ed(13), (1, 2, 2, 2), [(SP, 1, ed(4), pl.payload_of(32)), (SP, 5, ed(7), pl.payload_of(5, 1))])
    b = case("store_payload_signers", [(1, 2, 0b11), (0, 1, 0b1)])
    b.sig_ed(13)
    b.sig_payload(4, pl.payload_of(32))
    b.acheck(b.use(sp), 2)
    b = bld.body(length=31)
    b.sig_payload(4, pl.payload_of(32))
    b.sig_payload(7, pl.payload_of(5, 0))  # (another payload: no match)
    b.acheck(b.use(sp), 2)
    # one store account used by several checks of a body, and by several bodies
    m = bld.account(ed(14), (1, 1, 2, 3), [(ED, 1, ed(2)), (ED, 1, ed(3))])
    b = case("shared_account", [(1, 1, 0b001), (1, 2, 0b011), (1, 3, 0b111), (0, 1, 0b1), (0, 1, 0b1)])
    p = b.use(m)
    for sd in (14, 2, 3):
        b.sig_ed(sd)
    for level in (1, 2, 3):
        b.acheck(p, level)
    for _ in range(2):
        b = bld.body(length=30)
        b.sig_ed(3)
        b.acheck(b.use(m), 2)
    # a body using one store account twice: the duplicated entry only repeats candidate rows
    b = case("duplicate_entry", [(1, 2, 0b011), (1, 2, 0b011), (1, 3, 0b111)])
    p0, p1 = b.use(m), b.use(m)
    for sd in (14, 2, 3):
        b.sig_ed(sd)
    b.acheck(p0, 2)
    b.acheck(p1, 2)
    b.acheck(p1, 3)
    # an ID the store does not hold: found 0, its checks 0 (also with needed 0), the body's other checks unaffected
    z = bld.absent(1)
    b = case("not_held", [(0, 0, 0), (0, 0, 0), (1, 1, 0b1)])
    b.sig_ed(14)
    pz, pm = b.use(z), b.use(m)
    b.acheck(pz, 1)
    b.acheck(pz, 0, 0)
    b.acheck(pm, 1)
    # PRE_AUTH_TX and HASH_X signers of a store account
    pre = b"a preimage of the account's"
    b = case("preauth_hashx", [(1, 7, 0b1), (1, 4, 0), (0, 7, 0b1)])
    h = bld.account(ed(15), (0, 4, 7, 8), [(PRE, 4, raw(b.hash)), (HX, 3, ap.hashx(pre))])
    b.sig_hashx(pre)
    p = b.use(h)
    b.acheck(p, 2)
    b.acheck(p, 1)
    b.acheck(p, 3)
    # a body without checks (it lists an account), a body without accounts, then one that has both again
    b = case("no_checks", [])
    b.use(m)
    b.sig_ed(14)
    b = case("no_accounts", [])
    b.sig_ed(2)
    b = case("after_none", [(1, 1, 1)])
    b.sig_ed(14)
    b.acheck(b.use(m), 1)
    # the weight clamp: 300 against needed 256 (255 from protocol 10 on), a local account
    c = bld.account(ed(1), (0, 0, 0, 0), [(ED, 300, ed(2))], where=LOCAL)
    b = case("clamp", [(0, 255, 1)])
    b.sig_ed(2)
    b.acheck(b.use(c), 0, 256)
    # 20 signers + the master: the longest list the store holds (the signing key is the last signer)
    rows = [raw(hashlib.sha256(b"filler %d" % i).digest()) for i in range(19)]
    big = bld.account(ed(16), (1, 3, 3, 3), [(ED, 1, r) for r in rows] + [(ED, 2, ed(7))])
    b = case("twenty_signers", [(1, 3, 0b11)])
    b.sig_ed(7)
    b.sig_ed(16)
    b.acheck(b.use(big), 2)
    return out


def random_pool(bld, nb, n_store=40, n_local=6, n_absent=3, entries=None):
    """n_store store accounts (distinct masters, 0..20 signers of all four types), n_local pseudo-accounts and
    n_absent IDs that are not held, shared by nb bodies of 1..3 entries, 0..5 signatures and 0..4 checks;
    entries: the exact number of bacct entries (the last bodies get one each until it is reached)."""
    rng = bld.rng
    first = len(bld.accounts)
    pres = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (0, 5, 33)]
    for i in range(n_store):
        signers = []
        for _ in range(int(rng.choice([0, 1, 2, 3, 20]))):
            r, w = rng.random(), int(rng.choice([1, 1, 2, 3, 255, 300]))
            if r < 0.6:
                signers.append((ED, w, ap.ed(int(rng.integers(1, 9)))))
            elif r < 0.75:
                signers.append((HX, w, ap.hashx(pres[int(rng.integers(0, len(pres)))])))
            else:
                signers.append((SP, w, ap.ed(int(rng.integers(1, 9))), pl.payload_of(int(rng.choice([0, 3, 32, 64])))))
        thr = (int(rng.choice([0, 1, 1, 2])),) + tuple(int(x) for x in rng.integers(0, 4, 3))
        bld.account(ap.ed(100 + i), thr, signers)
    for i in range(n_local):
        if i % 2:
            bld.account(ap.ed(int(rng.integers(1, 9))), (1, 0, 0, 0), where=LOCAL)
        else:
            bld.account(ap.raw(bytes(32)), (0, 0, 0, 0),
                        [(ED, 1, ap.ed(3)), (SP, 1, ap.ed(4), pl.payload_of(int(rng.choice([3, 64]))))], where=LOCAL)
    for i in range(n_absent):
        bld.absent(1000 + i)
    n_accounts = n_store + n_local + n_absent
    total = 0
    for t in range(nb):
        b = bld.body(length=int(rng.integers(0, 120)))
        k = int(rng.integers(1, 4))
        if entries is not None:
            k = min(k, entries - total - (nb - 1 - t)) if entries - total >= nb - t else 0
            if t == nb - 1:
                k = entries - total
        total += k
        accts = [first + int(x) for x in rng.integers(0, n_accounts, k)]
        pos = [b.use(a) for a in accts]
        for _ in range(int(rng.integers(0, 6))):
            A = bld.accounts[accts[int(rng.integers(0, len(accts)))]] if accts else None
            r = rng.random()
            sp = [g for g in A.signers if g[0] == SP] if A else []
            if r < 0.4 and A and A.master[0] == "ed":
                b.sig_ed(A.master[1])
            elif r < 0.6 and A and any(g[0] == ED for g in A.signers):
                g = [g for g in A.signers if g[0] == ED]
                b.sig_ed(g[int(rng.integers(0, len(g)))][2][1], corrupt=rng.random() < 0.1)
            elif r < 0.8 and sp:
                g = sp[int(rng.integers(0, len(sp)))]
                b.sig_payload(g[2][1], g[3], corrupt=rng.random() < 0.1)
            elif r < 0.9:
                b.sig_hashx(pres[int(rng.integers(0, len(pres)))])
            else:
                b.sig_ed(int(rng.integers(1, 9)))
        if pos:
            for _ in range(int(rng.integers(0, 5))):
                b.acheck(pos[int(rng.integers(0, len(pos)))], int(rng.integers(0, 4)),
                         int(rng.choice([0, 0, 1, 2, 3])))
    assert entries is None or total == entries
