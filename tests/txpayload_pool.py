"""Input builder and plain-Python contract of the check entry points with the
payload tables (sv_ed25519_check_txbodies* with sv_txchecks_payload;
test_txpayload_cpu.py, test_gpu_txpayload.py).

PBuilder extends txchecks_pool.Builder: a body also has signed-payload
candidates (key seed, payload) and signatures made over a payload, whose
default hint is txset_gen.payload_hint.  A signer (SP, weight, j) names the
body's candidate j.  finish() lays the candidates out in the C-ABI's tables and
gives every SP signer two key indices: into pkey (tables present) and, for the
same batch run without the tables, its body's first key row, which the skip
ignores.

The reference is replay4(): the four stages of SignatureChecker.cpp:30-136
restated with no protocol gate on the last, txset_gen.payload_hint for the hint
rule and the oracle for every verification; it is asserted equal to
txset_gen.Checker on every check at protocol >= 19 (the Checker gates the
signed-payload signer type at 19, where the network introduced it; the
reference's checkSignature itself has no gate).  Nothing here comes from the
code under test.
"""
import hashlib

import numpy as np

import ed25519_pysign as ps
import txbodies_pool as tp
import txchecks_pool as cp
import txset_gen as tg

ED, PRE, HX, SP = cp.ED, cp.PRE, cp.HX, cp.SP
PAYLOAD_LENGTHS = (0, 1, 3, 4, 5, 31, 32, 47, 48, 63, 64)

_keys = {}


def keypair(seed):
    if seed not in _keys:
        _keys[seed] = ps.keypair(cp.seed_of(seed))
    return _keys[seed]


def pk_of(seed):
    return keypair(seed)[2]


def payload_of(n, salt=0):
    return bytes((11 * i + 3 * n + salt) & 255 for i in range(n))


class PBody(cp.Body):
    def __init__(self, kind, data):
        super().__init__(kind, data)
        self.pkeys = []

    def pkey(self, seed, payload):
        """A signed-payload candidate; returns its body-local index."""
        assert len(payload) <= 64
        self.pkeys.append((seed, bytes(payload)))
        return len(self.pkeys) - 1

    def sig_payload(self, seed, payload, corrupt=False, length=64, hint=None):
        """A signature by `seed` over `payload`, hinted for the signed-payload signer (seed, payload)."""
        self.sigs.append(dict(kind="payload", seed=seed, payload=bytes(payload), corrupt=corrupt, length=length,
                              hint=tg.payload_hint(pk_of(seed), bytes(payload)) if hint is None else bytes(hint)))
        return len(self.sigs) - 1


class PBuilder(cp.Builder):
    def body(self, kind=None, length=None):
        kind = int(self.rng.integers(0, 3)) if kind is None else kind
        length = int(self.rng.integers(0, 200)) if length is None else length
        b = PBody(kind, self.rng.integers(0, 256, length, dtype=np.uint8).tobytes())
        self.bodies.append(b)
        return b

    def finish(self, signer, oracle, layout_only=False):
        """signer: the 32-byte batch signer of txbodies_pool (payloads of 32
        bytes go through it too); payloads of other lengths are signed by the
        plain-Python signer, every signature checked by the oracle.
        layout_only: no signing, the payload signatures are zero rows."""
        B = self.bodies
        batch = [(b, s) for b in B for s in b.sigs if s["kind"] == "payload" and len(s["payload"]) == 32]
        if layout_only:
            for b in B:
                for s in b.sigs:
                    if s["kind"] == "payload":
                        s["made"] = bytes(64)
        elif batch:
            sd = np.array([np.frombuffer(cp.seed_of(s["seed"]), np.uint8) for _, s in batch], np.uint8)
            ms = np.array([np.frombuffer(s["payload"], np.uint8) for _, s in batch], np.uint8)
            pk, made = signer(sd, ms)
            for i, (_, s) in enumerate(batch):
                assert pk[i].tobytes() == pk_of(s["seed"])
                s["made"] = made[i].tobytes()
        for b in B:
            for s in b.sigs:
                if s["kind"] != "payload":
                    continue
                raw = bytearray(s["made"] if "made" in s else ps.sign_checked(oracle, keypair(s["seed"]), s["payload"]))
                if s["corrupt"]:
                    raw[40] ^= 1
                h, n = s["hint"], s["length"]
                s.clear()
                s.update(kind="raw", hint=h, data=bytes(raw[:n]))
            # (the skip needs a key row to point at)
            if any(ty == SP for _, gs in b.checks for ty, _, _ in gs) and not b.keys:
                b.key_raw(hashlib.sha256(b"no key").digest())
        s = super().finish(signer)
        nb = len(B)
        pkey_begin = np.concatenate([[0], np.cumsum([len(b.pkeys) for b in B], dtype=np.uint64)]).astype(np.uint64)
        nq = int(pkey_begin[-1])
        pkey, pay, plen = np.zeros((nq, 32), np.uint8), np.zeros((nq, 64), np.uint8), np.zeros(nq, np.uint8)
        for t, b in enumerate(B):
            b.pkey_rows = []
            for j, (seed, payload) in enumerate(b.pkeys):
                i = int(pkey_begin[t]) + j
                pkey[i] = np.frombuffer(pk_of(seed), np.uint8)
                pay[i, :len(payload)] = np.frombuffer(payload, np.uint8)
                plen[i] = len(payload)
                b.pkey_rows.append((pk_of(seed), payload))
        with_tables, without = s["signer_key"].copy(), s["signer_key"].copy()
        g = 0
        for t, b in enumerate(B):
            for _, signers in b.checks:
                for ty, _, k in signers:
                    if ty == SP:
                        with_tables[g] = int(pkey_begin[t]) + k
                        without[g] = int(s["key_begin"][t])
                    g += 1
        assert g == s["ng"] and nb == s["nb"]
        s.update(signer_key=with_tables, signer_key_skip=without, pkey_begin=pkey_begin, pkey=pkey, pkey_payload=pay,
                 pkey_len=plen, nq=nq)
        return s


def args(s, tables=True):
    """Positional arguments of sv.check_txbodies / check_txbodies_cpu."""
    return cp.args(s)[:-1] + (s["signer_key"] if tables else s["signer_key_skip"],)


def tables(s):
    """The payload keyword arguments."""
    return dict(pkey_begin=s["pkey_begin"], pkey=s["pkey"], pkey_payload=s["pkey_payload"], pkey_len=s["pkey_len"])


def replay4(protocol, contents_hash, sigs, signers, needed, verify):
    """(ok, weight, used mask) of one check over all four stages."""
    clamp = (lambda w: min(w, 255)) if protocol >= 10 else (lambda w: w)
    total, done, used = 0, False, 0
    for g in signers:
        if g["type"] == PRE and g["key"] == contents_hash and not done:
            total += clamp(g["weight"])
            done = total >= needed

    def match(ty, s, g):
        if ty == HX:
            return s["hint"] == g["key"][28:] and hashlib.sha256(s["sig"]).digest() == g["key"]
        if ty == ED:
            return s["hint"] == g["key"][28:] and len(s["sig"]) == 64 and verify(g["key"], s["sig"], contents_hash)
        return (s["hint"] == tg.payload_hint(g["key"], g["payload"]) and len(s["sig"]) == 64
                and verify(g["key"], s["sig"], g["payload"]))

    for ty in (HX, ED, SP):
        rest = [g for g in signers if g["type"] == ty]
        for i, s in enumerate(sigs):
            if done:
                break
            for g in rest:
                if match(ty, s, g):
                    used |= 1 << i
                    total += clamp(g["weight"])
                    done = total >= needed
                    rest.remove(g)
                    break
    if protocol >= 19:
        ck = tg.Checker(protocol, contents_hash, sigs, verify)
        ok = ck.check([dict(g) for g in signers], needed)
        mask = sum(1 << i for i, u in enumerate(ck.used) if u)
        assert (done, used) == (bool(ok), mask), "the restated four stages disagree with txset_gen.Checker"
    return int(done), min(total, 0xffffffff), used


def expected(s, verify, protocol=21, tables=True):
    """-> (check_ok, check_weight, check_used) by the Python replay: all four
    stages with the tables, txchecks_pool's three (type 3 skipped) without."""
    ok, weight, used = [], [], []
    for b in s["B"]:
        for need, signers in b.checks:
            gs = []
            for ty, w, k in signers:
                if ty == SP:
                    gs.append({"type": ty, "key": b.pkey_rows[k][0], "weight": w, "payload": b.pkey_rows[k][1]})
                else:
                    gs.append({"type": ty, "key": b.key_rows[k], "weight": w, "payload": b""})
            fn = replay4 if tables else cp.replay_check
            o, w, u = fn(protocol, b.hash, b.sig_rows, gs, need, verify)
            ok.append(o)
            weight.append(w)
            used.append(u)
    return (np.array(ok, np.uint8).reshape(-1), np.array(weight, np.uint32).reshape(-1),
            np.array(used, np.uint64).reshape(-1))


# ----------------------------------------------------------------- the edge cases
def edge_cases(bld):
    """Adds the issue's edge cases to `bld`, one tiny body each; returns {name:
    (first check index, by-hand [(ok, weight, mask), ...] at protocol 21 with the tables)}."""
    out = {}
    nc = lambda: sum(len(b.checks) for b in bld.bodies)  # noqa: E731

    def case(name, hand):
        out[name] = (nc(), hand)
        return bld.body(length=int(bld.rng.integers(1, 120)))

    # every payload length: the hint rule changes at 4, R || A || M needs a second SHA-512 block from 48
    for n in PAYLOAD_LENGTHS:
        b = case("len_%d" % n, [(1, 7, 0b1)])
        p = payload_of(n)
        b.sig_payload(1, p)
        b.check(7, [(SP, 7, b.pkey(1, p))])
    # the right signature with a wrong hint
    b = case("wrong_hint", [(0, 0, 0)])
    p = payload_of(20)
    b.sig_payload(1, p, hint=b"\1\2\3\4")
    b.check(1, [(SP, 1, b.pkey(1, p))])
    # the right hint with a corrupted signature
    b = case("corrupt", [(0, 0, 0)])
    b.sig_payload(1, p, corrupt=True)
    b.check(1, [(SP, 1, b.pkey(1, p))])
    # a 63-byte signature
    b = case("short_sig", [(0, 0, 0)])
    b.sig_payload(1, p, length=63)
    b.check(1, [(SP, 1, b.pkey(1, p))])
    # weight carried from PRE_AUTH_TX, HASH_X and ED25519 into the payload pass (the payload signature comes
    # first in the body: the passes, not the signatures, order the marks)
    b = case("carry", [(1, 15, 0b111), (0, 7, 0b110), (1, 9, 0b001)])
    pre = b"a preimage of some length"
    kp, kh, ke, q = b.key_preauth(), b.key_hashx(pre), b.key_ed(2), b.pkey(1, p)
    b.sig_payload(1, p)
    b.sig_hashx(pre)
    b.sig_ed(2)
    b.check(15, [(SP, 8, q), (ED, 4, ke), (HX, 2, kh), (PRE, 1, kp)])
    b.check(15, [(ED, 4, ke), (HX, 2, kh), (PRE, 1, kp)])
    b.check(9, [(SP, 8, q), (PRE, 1, kp)])
    # success inside the ED25519 pass leaves the payload signers untouched
    b = case("ed_first", [(1, 4, 0b10)])
    ke, q = b.key_ed(2), b.pkey(1, p)
    b.sig_payload(1, p)
    b.sig_ed(2)
    b.check(4, [(SP, 8, q), (ED, 4, ke)])
    # erasure: one payload signer, the same decorated signature twice
    b = case("erase_same_sig", [(0, 1, 0b01)])
    q = b.pkey(1, p)
    b.sig_payload(1, p)
    b.sig_payload(1, p)
    b.check(2, [(SP, 1, q)])
    # one candidate index listed twice (weights 1 then 255, needed 2), the signature twice
    b = case("dup_signer", [(1, 256, 0b11)])
    q = b.pkey(1, p)
    b.sig_payload(1, p)
    b.sig_payload(1, p)
    b.check(2, [(SP, 1, q), (SP, 255, q)])
    # two payload signers with the same key and different payloads (with equal last four bytes: one hint)
    pa, pb_ = b"first one" + b"tail", b"the second" + b"tail"
    b = case("same_key_two_payloads", [(1, 2, 0b1), (1, 6, 0b11)])
    qa, qb = b.pkey(1, pa), b.pkey(1, pb_)
    b.sig_payload(1, pb_)
    b.sig_payload(1, pa)
    b.check(2, [(SP, 4, qa), (SP, 2, qb)])
    b.check(6, [(SP, 4, qa), (SP, 2, qb)])
    # a payload equal to the body's contents hash: the one signature serves an ED25519 and a payload signer
    b = case("payload_is_tx", [(1, 3, 0b11), (1, 2, 0b10)])
    ke, q = b.key_ed(1), b.pkey(1, b.hash)
    b.sig_ed(1)
    b.sig_payload(1, b.hash)
    b.check(3, [(SP, 2, q), (ED, 1, ke)])
    b.check(2, [(SP, 2, q)])
    # hint collisions, both directions: an ED25519 signer's key row ending in the candidate's XORed hint (a pair
    # of verdict 0 in the ED25519 pass) ...
    b = case("collide_ed_key", [(1, 5, 0b1)])
    kx = b.key_raw(hashlib.sha256(b"collide").digest()[:28] + tg.payload_hint(pk_of(1), p))
    q = b.pkey(1, p)
    b.sig_payload(1, p)
    b.check(5, [(ED, 9, kx), (SP, 5, q)])
    # ... and a candidate whose XORed hint is an ed25519 key's hint (a payload pair of verdict 0)
    b = case("collide_candidate", [(0, 1, 0b1)])
    pc = b"collide" + bytes(x ^ y for x, y in zip(pk_of(1)[28:], pk_of(2)[28:]))
    assert tg.payload_hint(pk_of(1), pc) == pk_of(2)[28:]
    ke, q = b.key_ed(2), b.pkey(1, pc)
    b.sig_ed(2)
    b.check(3, [(ED, 1, ke), (SP, 2, q)])
    # needed <= 0: no match is false, a match is true
    b = case("needed_zero", [(0, 0, 0), (1, 5, 0b1), (1, 5, 0b1)])
    q0, q1 = b.pkey(1, p), b.pkey(2, p)
    b.sig_payload(1, p)
    b.check(0, [(SP, 5, q1)])
    b.check(0, [(SP, 5, q0)])
    b.check(-3, [(SP, 5, q0)])
    # clamp: weight 300, needed 256 (protocol 21; unclamped at protocol 9)
    b = case("clamp", [(0, 255, 0b1)])
    b.sig_payload(1, p)
    b.check(256, [(SP, 300, b.pkey(1, p))])
    # candidates and no signatures; a body with no candidates between two that have some
    b = case("no_signatures", [(0, 0, 0)])
    b.check(1, [(SP, 1, b.pkey(1, p))])
    b = case("before_none", [(1, 1, 0b1)])
    b.sig_payload(2, p)
    b.check(1, [(SP, 1, b.pkey(2, p))])
    b = case("none", [(1, 1, 0b1)])
    ke = b.key_ed(3)
    b.sig_ed(3)
    b.check(1, [(ED, 1, ke)])
    b = case("after_none", [(1, 1, 0b1)])
    b.sig_payload(3, p)
    b.check(1, [(SP, 1, b.pkey(3, p))])
    return out


def random_pool(bld, nb, share=0.5):
    """txchecks_pool.random_pool's bodies (mixed signer types; its own type-3
    entries removed) with, in about `share` of them, one to three payload
    candidates, signatures over some of their payloads and the candidates mixed
    into the checks' signer lists."""
    rng = bld.rng
    first = len(bld.bodies)
    cp.random_pool(bld, nb, max_sigs=8)
    for b in bld.bodies[first:]:
        b.checks = [(need, [g for g in gs if g[0] != SP]) for need, gs in b.checks]
        if rng.random() >= share:
            continue
        cands = []
        for _ in range(int(rng.integers(1, 4))):
            seed = int(rng.integers(1, 5))
            n = int(rng.choice([0, 2, 4, 32, 32, 32, 40, 64]))
            payload = b.hash if rng.random() < 0.15 else payload_of(n, int(rng.integers(0, 3)))
            cands.append((seed, payload, b.pkey(seed, payload)))
        for seed, payload, _ in cands:
            r = rng.random()
            if len(b.sigs) >= 12 or r < 0.25:
                continue
            pos = int(rng.integers(0, len(b.sigs) + 1))
            b.sig_payload(seed, payload, corrupt=0.8 < r < 0.9, length=63 if r > 0.95 else 64)
            b.sigs.insert(pos, b.sigs.pop())
        checks = []
        for need, gs in b.checks:
            gs = list(gs)
            for _, _, q in cands:
                if rng.random() < 0.6:
                    gs.insert(int(rng.integers(0, len(gs) + 1)), (SP, int(rng.choice([1, 2, 100, 255, 300])), q))
            checks.append((need, gs))
        b.checks = checks


# ----------------------------------------------------------------- envelope sets
def envelope_cases(s):
    """The envelopes of an envelope_bodies.build_set dict as the case dicts
    txset_gen.replay_envelope takes, read back from the flat arrays of the C
    call (hashes from `envs`, the ones hashlib computed)."""
    sigs, ops, signers, accounts = s["rest"]

    def signer(r):
        n = int(r["payload_len"])
        return {"type": int(r["type"]), "key": r["key"].tobytes(), "weight": int(r["weight"]),
                "payload": r["payload"][:n].tobytes()}

    def dsigs(off, n):
        return [{"hint": d["hint"].tobytes(), "sig": d["sig"][:int(d["sig_len"])].tobytes()} for d in sigs[off:off + n]]

    accs = [{"id": a["account_id"].tobytes(), "thresholds": [int(x) for x in a["thresholds"]],
             "signers": [signer(g) for g in signers[int(a["signer_off"]):int(a["signer_off"]) + int(a["nsigners"])]]}
            for a in accounts[:s["naccounts"]]]
    out = []
    for e in s["envs"][:s["n"]]:
        case = {"accounts": accs, "hash": e["contents_hash"].tobytes(), "source": e["source"].tobytes(),
                "sigs": dsigs(int(e["sig_off"]), int(e["nsigs"])),
                "ops": [{"level": int(o["level"]), "source": o["source"].tobytes() if o["has_source"] else None}
                        for o in ops[int(e["op_off"]):int(e["op_off"]) + int(e["nops"])]],
                "extra": [signer(g) for g in signers[int(e["extra_off"]):int(e["extra_off"]) + int(e["nextra"])]]}
        if e["fee_bump"]:
            case["fee_bump"] = {"hash": e["fee_bump_hash"].tobytes(), "fee_source": e["fee_source"].tobytes(),
                                "sigs": dsigs(int(e["outer_off"]), int(e["nouter"]))}
        out.append(case)
    return out
