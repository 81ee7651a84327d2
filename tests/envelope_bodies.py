"""Helper for svh_check_envelopes_bodies (include/stellar_host.h), beside
envelopes.py: the C call, and a hand-built envelope set whose transactions are
given as bodies -- V1 and V0 bodies, a fee-bump envelope, a 3-of-5 multisig,
a signed-payload signer and a body mutated after signing."""
import ctypes

import numpy as np

import envelopes as ev
import txbodies_pool as tp

ENVELOPE_BODY = np.dtype([("off", "<u8"), ("len", "<u4"), ("kind", "<u4"), ("outer_off", "<u8"), ("outer_len", "<u4"),
                          ("reserved", "<u4")])
assert ENVELOPE_BODY.itemsize == 32

txSUCCESS, txFEE_BUMP_INNER_SUCCESS, txBAD_AUTH = 0, 1, -6


def check_envelopes_bodies(host, envs, sigs, ops, signers, accounts, n, naccounts, protocol, bodies, ebody,
                           prefetch=0, for_apply=0, network_id=tp.NETWORK_ID, expect_rc=0):
    """-> (results, pairs, contents hashes n x 32, fee-bump hashes n x 32), or the
    return code when expect_rc != 0."""
    res = np.zeros(max(1, n), ev.RESULT)
    ch, fb = np.full((max(1, n), 32), 0xEE, np.uint8), np.full((max(1, n), 32), 0xEE, np.uint8)
    pairs = ctypes.c_uint64()
    vp = ctypes.c_void_p
    nid = np.frombuffer(network_id, np.uint8).copy()
    rc = host.svh_check_envelopes_bodies(
        vp(envs.ctypes.data), ctypes.c_size_t(n), vp(sigs.ctypes.data), vp(ops.ctypes.data), vp(signers.ctypes.data),
        vp(accounts.ctypes.data), ctypes.c_size_t(naccounts), ctypes.c_uint32(protocol), prefetch, for_apply,
        vp(res.ctypes.data), ctypes.byref(pairs), vp(nid.ctypes.data), vp(bodies.ctypes.data), vp(ebody.ctypes.data),
        vp(ch.ctypes.data), vp(fb.ctypes.data))
    if expect_rc:
        assert rc == expect_rc
        return rc
    assert rc == 0, host.svh_last_error_string()
    return res[:n], pairs.value, ch[:n], fb[:n]


N_KEYS = 9  # A, F, M1..M5, P, K
K_A, K_F, K_M, K_P, K_K = 0, 1, 2, 7, 8
UNIT = ("v1", "v0", "fee_bump", "multisig", "payload", "mutated")


def build_set(units, seed, signer, with_payload=True):
    """`units` repetitions of the hand-built unit (without the signed-payload
    envelope if with_payload is false).  Returns a dict: the arrays of the C
    call with hashlib hashes in the envelopes (`envs`) and with junk there
    (`envs_blank`), the body blob and svh_envelope_body array, the expected
    hashes and the expected codes by construction."""
    rng = np.random.default_rng(seed)
    key_seeds = rng.integers(0, 256, (N_KEYS, 32), dtype=np.uint8)
    kinds = [k for k in UNIT if with_payload or k != "payload"] * units
    payload = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    # bodies, back to back, lengths multiples of 4 (XDR)
    blob, ebody, hashes = bytearray(), np.zeros(len(kinds), ENVELOPE_BODY), []

    def new_body():
        b = bytes(rng.integers(0, 256, 4 * int(rng.integers(25, 101)), dtype=np.uint8))
        off = len(blob)
        blob.extend(b)
        return off, b

    jobs = [(k, bytes(32)) for k in range(N_KEYS)]  # (key, 32-byte message); the first N_KEYS only yield the keys
    plan = []
    for t, kind in enumerate(kinds):
        off, body = new_body()
        bk = tp.V0 if kind == "v0" else tp.V1
        ebody[t]["off"], ebody[t]["len"], ebody[t]["kind"] = off, len(body), bk
        inner = tp.contents_hash(bk, body)
        outer = bytes(32)
        signers_of = {"multisig": [K_M, K_M + 2, K_M + 4], "payload": [K_P]}.get(kind, [K_A])
        rows = [len(jobs) + i for i in range(len(signers_of))]
        jobs += [(k, inner) for k in signers_of]
        extra = {}
        if kind == "payload":
            extra["payload_row"] = len(jobs)
            jobs.append((K_K, payload))
        if kind == "fee_bump":
            ooff, obody = new_body()
            ebody[t]["outer_off"], ebody[t]["outer_len"] = ooff, len(obody)
            outer = tp.contents_hash(tp.FEE_BUMP, obody)
            extra["outer_row"] = len(jobs)
            jobs.append((K_F, outer))
        if kind == "mutated":  # one bit of the body after signing: the hash is that of the new bytes
            blob[off + len(body) // 2] ^= 0x04
            inner = tp.contents_hash(bk, bytes(blob[off:off + len(body)]))
        hashes.append((inner, outer))
        plan.append((kind, signers_of, rows, extra))
    pk, sig = signer(key_seeds[[k for k, _ in jobs]], np.array([np.frombuffer(m, np.uint8) for _, m in jobs], np.uint8))
    keys = [pk[k].tobytes() for k in range(N_KEYS)]

    def dsig(row, hint=None):
        return {"hint": (hint or pk[row].tobytes()[28:]).hex(), "sig": sig[row].tobytes().hex()}

    hx = lambda k: keys[k].hex()  # noqa: E731
    accounts = [
        {"id": hx(K_A), "thresholds": [1, 0, 0, 0], "signers": []},
        {"id": hx(K_F), "thresholds": [1, 0, 0, 0], "signers": []},
        # 3-of-5: no master key, five signers of weight 1, every threshold 3
        {"id": hx(K_M), "thresholds": [0, 3, 3, 3], "signers": [{"key": hx(K_M + i), "weight": 1} for i in range(5)]},
        # master key + a signed-payload signer, both needed
        {"id": hx(K_P), "thresholds": [1, 2, 2, 2],
         "signers": [{"type": 3, "key": hx(K_K), "weight": 1, "payload": payload.hex()}]},
    ]
    pay_hint = bytes(a ^ b for a, b in zip(keys[K_K][28:], payload[28:]))
    sets = {}
    for name in ("envs", "envs_blank"):
        es = ev.EnvelopeSet()
        for a in accounts:
            es.account(a)
        for t, (kind, signers_of, rows, extra) in enumerate(plan):
            inner, outer = hashes[t] if name == "envs" else (b"\xaa" * 32, b"\xbb" * 32)
            sigs = [dsig(r) for r in rows]
            if kind == "payload":
                sigs.append(dsig(extra["payload_row"], pay_hint))
            source = {"multisig": K_M, "payload": K_P}.get(kind, K_A)
            fee = None
            if kind == "fee_bump":
                fee = {"hash": outer.hex(), "fee_source": hx(K_F), "sigs": [dsig(extra["outer_row"])]}
            es.envelope(hx(source), inner.hex(), sigs, [{"level": 2}], fee_bump=fee)
        sets[name] = es.arrays()
    expect = np.array([{"fee_bump": txFEE_BUMP_INNER_SUCCESS, "mutated": txBAD_AUTH}.get(k, txSUCCESS) for k in kinds],
                      np.int32)
    return dict(n=len(kinds), naccounts=len(accounts), kinds=kinds, expect=expect,
                envs=sets["envs"][0], envs_blank=sets["envs_blank"][0], rest=sets["envs"][1:],
                bodies=np.frombuffer(bytes(blob), np.uint8).copy(), ebody=ebody,
                contents_hash=np.array([np.frombuffer(h[0], np.uint8) for h in hashes], np.uint8),
                fee_bump_hash=np.array([np.frombuffer(h[1], np.uint8) for h in hashes], np.uint8))
