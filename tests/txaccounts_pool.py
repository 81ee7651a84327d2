"""Input builder and plain-Python contract of the by-account check entry points
(sv_ed25519_check_txbodies_accounts*; test_txaccounts_cpu.py,
test_gpu_txaccounts.py).

ABuilder extends txpayload_pool.PBuilder: the builder owns an account table
(key, thresholds, signer list), a body lists the accounts it uses (use()) and
its checks name one of them by position plus a threshold level (acheck()).

expand() IS the reference expansion of include/stellar_sigverify.h, written in
plain Python over the builder's own objects: for each body, in use() order, the
account's key iff its master weight is > 0, then its signers of types 0-2, go to
the body's key list, its type-3 signers to the body's payload candidates; a
check's signer list is (ED25519, master weight, master row) iff the master
weight is > 0, then the account's signers in list order; needed is
thresholds[level], or the check's own value at level 0.  finish() lays that
expansion out as the explicit tables (PBuilder.finish; the replay of
txpayload_pool.expected / txset_gen.Checker and the explicit _cpu entry point
run on them) next to the by-account arrays.  Nothing here comes from the code
under test.  (PBuilder.finish gives a body whose checks have a type-3 signer
and no key row one unrelated key row; it matches no hint and changes no result.)
"""
import hashlib

import numpy as np

import txbodies_pool as tp
import txchecks_pool as cp
import txpayload_pool as pl

ED, PRE, HX, SP = cp.ED, cp.PRE, cp.HX, cp.SP


def ed(seed):
    return ("ed", seed)


def raw(row):
    assert len(row) == 32
    return ("raw", bytes(row))


def hashx(preimage):
    return raw(hashlib.sha256(bytes(preimage)).digest())


def key_bytes(spec):
    return pl.pk_of(spec[1]) if spec[0] == "ed" else spec[1]


class Account:
    def __init__(self, master, thresholds, signers):
        self.master, self.thresholds = master, tuple(int(x) for x in thresholds)
        assert len(self.thresholds) == 4 and all(0 <= x < 256 for x in self.thresholds)
        # (type, weight, key spec, payload or None)
        self.signers = [(g[0], int(g[1]), g[2], bytes(g[3]) if len(g) > 3 and g[3] is not None else None)
                        for g in signers]
        assert all((ty == SP) == (p is not None) and (ty != SP or k[0] == "ed") for ty, _, k, p in self.signers)


class ABody(pl.PBody):
    def __init__(self, kind, data):
        super().__init__(kind, data)
        self.uses, self.achecks = [], []

    def use(self, acct):
        """Lists account `acct` (table index); returns its position in the body's list."""
        self.uses.append(int(acct))
        return len(self.uses) - 1

    def acheck(self, pos, level, needed=0):
        self.achecks.append((int(pos), int(level), int(needed)))
        return len(self.achecks) - 1


class ABuilder(pl.PBuilder):
    def __init__(self, seed=1):
        super().__init__(seed)
        self.accounts = []

    def account(self, master, thresholds, signers=()):
        self.accounts.append(Account(master, thresholds, signers))
        return len(self.accounts) - 1

    def body(self, kind=None, length=None):
        kind = int(self.rng.integers(0, 3)) if kind is None else kind
        length = int(self.rng.integers(0, 200)) if length is None else length
        b = ABody(kind, self.rng.integers(0, 256, length, dtype=np.uint8).tobytes())
        self.bodies.append(b)
        return b

    def expand(self):
        """The expansion of the header comment, into each body's keys / pkeys / checks."""
        def add_key(b, spec):
            return b.key_ed(spec[1]) if spec[0] == "ed" else b.key_raw(spec[1])
        for b in self.bodies:
            b.keys, b.pkeys, b.checks = [], [], []
            rows = []
            for a in b.uses:
                A = self.accounts[a]
                m = add_key(b, A.master) if A.thresholds[0] > 0 else None
                gs = []
                for ty, w, k, payload in A.signers:
                    gs.append((ty, w, b.pkey(k[1], payload) if ty == SP else add_key(b, k)))
                rows.append((m, gs))
            for pos, level, needed in b.achecks:
                A = self.accounts[b.uses[pos]]
                m, gs = rows[pos]
                b.check(A.thresholds[level] if level else needed, ([(ED, A.thresholds[0], m)] if m is not None else []) + gs)

    def finish(self, signer, oracle, layout_only=False):
        self.expand()
        s = super().finish(signer, oracle, layout_only)
        A, B = self.accounts, self.bodies
        na = len(A)
        csr = lambda counts: np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)  # noqa: E731
        acct_key = np.zeros((na, 32), np.uint8)
        thr = np.zeros((na, 4), np.uint8)
        gt, gw, gk, gp, pay_rows, pay_of = [], [], [], [], [], {}
        for i, a in enumerate(A):
            acct_key[i] = np.frombuffer(key_bytes(a.master), np.uint8)
            thr[i] = a.thresholds
            for ty, w, k, payload in a.signers:
                gt.append(ty)
                gw.append(w)
                gk.append(np.frombuffer(key_bytes(k), np.uint8))
                if ty == SP:  # (equal payloads share a row)
                    if payload not in pay_of:
                        pay_of[payload] = len(pay_rows)
                        pay_rows.append(payload)
                    gp.append(pay_of[payload])
                else:
                    gp.append(0xFFFFFFFF)  # (read only for type 3)
        npay = len(pay_rows)
        apayload, alen = np.zeros((npay, 64), np.uint8), np.zeros(npay, np.uint8)
        for i, p in enumerate(pay_rows):
            apayload[i, :len(p)] = np.frombuffer(p, np.uint8)
            alen[i] = len(p)
        s.update(acct_key=acct_key, acct_thresholds=thr, asigner_begin=csr([len(a.signers) for a in A]),
                 asigner_type=np.array(gt, np.uint8).reshape(-1), asigner_weight=np.array(gw, np.uint32).reshape(-1),
                 asigner_key=np.array(gk, np.uint8).reshape(-1, 32), asigner_payload=np.array(gp, np.uint32).reshape(-1),
                 apayload=apayload, apayload_len=alen, na=na, nas=len(gt), npay=npay,
                 bacct_begin=csr([len(b.uses) for b in B]),
                 bacct=np.array([a for b in B for a in b.uses], np.uint32).reshape(-1),
                 check_acct=np.array([c[0] for b in B for c in b.achecks], np.uint32).reshape(-1),
                 check_level=np.array([c[1] for b in B for c in b.achecks], np.uint8).reshape(-1),
                 acheck_needed=np.array([c[2] for b in B for c in b.achecks], np.int32).reshape(-1))
        s["ne"] = len(s["bacct"])
        assert len(s["check_acct"]) == s["nc"]
        return s


ACCOUNT_KEYS = ("acct_key", "acct_thresholds", "asigner_begin", "asigner_type", "asigner_weight", "asigner_key",
                "asigner_payload", "apayload", "apayload_len", "bacct_begin", "bacct", "check_begin", "check_acct",
                "check_level", "acheck_needed")


def args(s, **over):
    """Positional arguments of sv.check_txbodies_accounts / _cpu (`over` replaces arrays by name)."""
    t = dict(s)
    t.update(over)
    return (tp.NETWORK_ID, t["bodies"], t["off"], t["len"], t["kind"], t["sig_begin"], t["hint"], t["sig"]) + tuple(
        t[k] for k in ACCOUNT_KEYS)


def explicit_args(s):
    """... and of sv.check_txbodies / _cpu over the Python expansion: (positional, keywords)."""
    return pl.args(s), dict(sig_len=s["sig_len"], **pl.tables(s))


def expected(s, verify, protocol=21):
    return pl.expected(s, verify, protocol)


# ----------------------------------------------------------------- the edge cases
def edge_cases(bld):
    """Adds the edge cases to `bld`; returns {name: (first check index, by-hand
    [(ok, weight, mask), ...] at protocol 21)}."""
    out = {}
    nc = lambda: sum(len(b.achecks) for b in bld.bodies)  # noqa: E731

    def case(name, hand):
        out[name] = (nc(), hand)
        return bld.body(length=int(bld.rng.integers(1, 120)))

    # master weight 0: the master is no signer and no candidate; its valid signature earns nothing, stays unused
    a = bld.account(ed(1), (0, 1, 1, 1), [(ED, 1, ed(2))])
    b = case("master_weight_zero", [(0, 0, 0), (1, 1, 0b10)])
    b.sig_ed(1)
    b.acheck(b.use(a), 1)
    b = bld.body(length=20)
    b.sig_ed(1)
    b.sig_ed(2)
    b.acheck(b.use(a), 1)
    # levels 1, 2, 3 pick their own threshold
    a = bld.account(ed(1), (2, 1, 2, 3))
    b = case("levels", [(1, 2, 1), (1, 2, 1), (0, 2, 1)])
    p = b.use(a)
    b.sig_ed(1)
    for level in (1, 2, 3):
        b.acheck(p, level)
    # level 0 with needed 0: a match is true, no match is false
    a1, a2 = bld.account(ed(1), (5, 9, 9, 9)), bld.account(ed(2), (5, 9, 9, 9))
    b = case("level0_needed0", [(1, 5, 1), (0, 0, 0)])
    b.sig_ed(1)
    b.acheck(b.use(a1), 0, 0)
    b.acheck(b.use(a2), 0, 0)
    # the extra-signer pseudo-account: master weight 0, weight 1 each, needed = their count; a short and a 64-byte payload
    short, full = pl.payload_of(3), pl.payload_of(64)
    x = bld.account(raw(bytes(32)), (0, 0, 0, 0), [(ED, 1, ed(3)), (SP, 1, ed(4), short), (SP, 1, ed(4), full)])
    b = case("extra_signers", [(1, 3, 0b111)])
    b.sig_payload(4, full)
    b.sig_ed(3)
    b.sig_payload(4, short)
    b.acheck(b.use(x), 0, 3)
    b = case("extra_signers_one_missing", [(0, 2, 0b11)])
    b.sig_payload(4, full)
    b.sig_ed(3)
    b.acheck(b.use(x), 0, 3)
    # the no-account pseudo-account: master weight 1, no signers, needed 0
    n = bld.account(ed(5), (1, 0, 0, 0))
    b = case("no_account", [(1, 1, 1), (0, 0, 0)])
    b.sig_ed(5)
    b.acheck(b.use(n), 0, 0)
    b = bld.body(length=9)
    b.sig_ed(6)
    b.acheck(b.use(n), 0, 0)
    # one account used by several checks of a body, and by several bodies
    m = bld.account(ed(1), (1, 1, 2, 3), [(ED, 1, ed(2)), (ED, 1, ed(3))])
    b = case("shared_account", [(1, 1, 0b001), (1, 2, 0b011), (1, 3, 0b111), (0, 1, 0b1), (0, 1, 0b1)])
    p = b.use(m)
    for sd in (1, 2, 3):
        b.sig_ed(sd)
    for level in (1, 2, 3):
        b.acheck(p, level)
    for _ in range(2):
        b = bld.body(length=30)
        b.sig_ed(3)
        b.acheck(b.use(m), 2)
    # two accounts of one body sharing a signer key
    p_, q_ = bld.account(ed(1), (1, 2, 2, 2), [(ED, 1, ed(3))]), bld.account(ed(2), (1, 2, 2, 2), [(ED, 2, ed(3))])
    b = case("shared_signer_key", [(0, 1, 1), (1, 2, 1)])
    b.sig_ed(3)
    b.acheck(b.use(p_), 2)
    b.acheck(b.use(q_), 2)
    # a duplicated bacct entry only repeats candidate rows
    b = case("duplicate_entry", [(1, 2, 0b011), (1, 2, 0b011), (1, 3, 0b111)])
    p0, p1 = b.use(m), b.use(m)
    for sd in (1, 2, 3):
        b.sig_ed(sd)
    b.acheck(p0, 2)
    b.acheck(p1, 2)
    b.acheck(p1, 3)
    # PRE_AUTH_TX and HASH_X account signers
    pre = b"a preimage of the account's"
    b = case("preauth_hashx", [(1, 7, 0b1), (1, 4, 0), (0, 7, 0b1)])
    h = bld.account(ed(1), (0, 4, 7, 8), [(PRE, 4, raw(b.hash)), (HX, 3, hashx(pre))])
    b.sig_hashx(pre)
    p = b.use(h)
    b.acheck(p, 2)
    b.acheck(p, 1)
    b.acheck(p, 3)
    # an account with no signer at all: false, also with needed 0
    z = bld.account(ed(1), (0, 0, 0, 0))
    b = case("no_signer", [(0, 0, 0), (0, 0, 0)])
    b.sig_ed(1)
    p = b.use(z)
    b.acheck(p, 1)
    b.acheck(p, 0, 0)
    # a body without checks (it lists an account), a body without accounts, then one that has both again
    b = case("no_checks", [])
    b.use(m)
    b.sig_ed(1)
    b = case("no_accounts", [])
    b.sig_ed(2)
    b = case("after_none", [(1, 1, 1)])
    b.sig_ed(1)
    b.acheck(b.use(m), 1)
    # the weight clamp: 300 against needed 256 (255 from protocol 10 on)
    c = bld.account(ed(1), (0, 0, 0, 0), [(ED, 300, ed(2))])
    b = case("clamp", [(0, 255, 1)])
    b.sig_ed(2)
    b.acheck(b.use(c), 0, 256)
    # 63 signers + the master: the longest expanded list (the signing key is the last signer)
    rows = [raw(hashlib.sha256(b"filler %d" % i).digest()) for i in range(62)]
    big = bld.account(ed(1), (1, 3, 3, 3), [(ED, 1, r) for r in rows] + [(ED, 2, ed(7))])
    b = case("sixty_four_signers", [(1, 3, 0b11)])
    b.sig_ed(7)
    b.sig_ed(1)
    b.acheck(b.use(big), 2)
    return out


def random_pool(bld, nb, n_accounts=24):
    """n_accounts accounts of mixed shape (master weight 0..3, 0..4 signers of all
    four types, pseudo-accounts among them) shared by nb bodies of 1..3 accounts
    (some listed twice), 0..7 signatures and 0..5 checks at levels 0..3."""
    rng = bld.rng
    first = len(bld.accounts)
    pres = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (0, 5, 33, 64)]
    for i in range(n_accounts):
        signers = []
        for _ in range(int(rng.integers(0, 5))):
            r, w = rng.random(), int(rng.choice([1, 1, 2, 3, 100, 255, 300]))
            if r < 0.55:
                signers.append((ED, w, ed(int(rng.integers(1, 9)))))
            elif r < 0.7:
                signers.append((HX, w, hashx(pres[int(rng.integers(0, len(pres)))])))
            elif r < 0.75:
                signers.append((PRE, w, raw(hashlib.sha256(b"not a transaction").digest())))
            else:
                n = int(rng.choice([0, 3, 4, 32, 32, 64]))
                signers.append((SP, w, ed(int(rng.integers(1, 9))), pl.payload_of(n, int(rng.integers(0, 2)))))
        thr = (int(rng.choice([0, 1, 1, 2, 3])),) + tuple(int(x) for x in rng.integers(0, 5, 3))
        bld.account(ed(int(rng.integers(1, 9))), thr, signers)
    for t in range(nb):
        b = bld.body(length=int(rng.integers(0, 200)))
        accts = [first + int(x) for x in rng.integers(0, n_accounts, int(rng.integers(1, 4)))]
        if rng.random() < 0.15:
            accts.append(accts[0])
        if t % 17 == 5:
            accts = []
        pos = [b.use(a) for a in accts]
        cands = [bld.accounts[a] for a in accts]
        for _ in range(0 if t % 9 == 4 else int(rng.integers(0, 8))):
            r = rng.random()
            A = cands[int(rng.integers(0, len(cands)))] if cands else None
            sp = [g for g in A.signers if g[0] == SP] if A else []
            if r < 0.3 and A:
                b.sig_ed(A.master[1])
            elif r < 0.55 and A and any(g[0] == ED for g in A.signers):
                g = [g for g in A.signers if g[0] == ED]
                b.sig_ed(g[int(rng.integers(0, len(g)))][2][1], corrupt=rng.random() < 0.1)
            elif r < 0.75 and sp:
                g = sp[int(rng.integers(0, len(sp)))]
                b.sig_payload(g[2][1], g[3], corrupt=rng.random() < 0.1)
            elif r < 0.85:
                b.sig_hashx(pres[int(rng.integers(0, len(pres)))])
            elif r < 0.92:
                b.sig_ed(int(rng.integers(1, 9)), length=63 if rng.random() < 0.3 else 64)
            else:
                b.sig_raw(rng.integers(0, 256, 4, dtype=np.uint8).tobytes(),
                          rng.integers(0, 256, 64, dtype=np.uint8).tobytes())
        if pos:
            for _ in range(int(rng.integers(0, 6))):
                b.acheck(pos[int(rng.integers(0, len(pos)))], int(rng.integers(0, 4)),
                         int(rng.choice([0, 0, 1, 2, 3, 256, -1])))
