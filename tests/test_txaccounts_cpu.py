"""Signature checks against an account table, on a host without a GPU: the CPU
form sv_ed25519_check_txbodies_accounts_cpu against the plain-Python expansion
of txaccounts_pool.py -- fed to the Python replay (txpayload_pool.expected /
txset_gen.Checker) and to the explicit sv_ed25519_check_txbodies_cpu -- and
by-hand expectations; every reject of the host forms alone; the by-account
planner and packer against a numpy restatement; the host code under sanitizers
as a stand-alone program.  Every expectation is exact equality."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import envelope_bodies as eb
import envelopes as ev
import txaccounts_pool as ap
import txbodies_pool as tp
import txchecks_pool as cp
import txpayload_pool as pl

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ED, SP = ap.ED, ap.SP


@pytest.fixture(scope="module")
def edge(sv, oracle):
    bld = ap.ABuilder(5)
    cases = ap.edge_cases(bld)
    s = bld.finish(tp.pysign_signer(oracle), oracle)
    return s, cases, cp.oracle_verify(oracle)


def _cpu(sv, s, protocol=21, threads=0, **over):
    return sv.check_txbodies_accounts_cpu(*ap.args(s, **over), sig_len=s["sig_len"], protocol_version=protocol,
                                          threads=threads)


def _explicit_cpu(sv, s, protocol=21):
    a, kw = ap.explicit_args(s)
    return sv.check_txbodies_cpu(*a, protocol_version=protocol, **kw)


def test_edge_cases_by_hand(sv, edge):
    s, cases, _ = edge
    assert {"master_weight_zero", "levels", "level0_needed0", "extra_signers", "no_account", "shared_account",
            "shared_signer_key", "duplicate_entry", "preauth_hashx", "no_signer", "no_checks", "no_accounts", "clamp",
            "sixty_four_signers"} <= set(cases)
    ok, weight, used, dig = _cpu(sv, s)
    assert (dig == s["digests"]).all()
    for name, (c0, hand) in cases.items():
        got = [(int(ok[c0 + i]), int(weight[c0 + i]), int(used[c0 + i])) for i in range(len(hand))]
        assert got == hand, name
    # the longest legal list really is 64 signers; the master of a weight-0 account is no candidate
    c = cases["sixty_four_signers"][0]
    assert int(s["signer_begin"][c + 1] - s["signer_begin"][c]) == 64
    assert int(s["key_begin"][1] - s["key_begin"][0]) == 1 and s["B"][0].key_rows == [pl.pk_of(2)]


def test_edge_cases_match_the_replay_and_the_explicit_form(sv, edge):
    s, cases, verify = edge
    for protocol in (21, 10, 9):
        want = ap.expected(s, verify, protocol)
        assert want[0].any() and not want[0].all()
        for threads in (1, 4):
            cp.assert_equal(_cpu(sv, s, protocol, threads=threads), want, s)
        cp.assert_equal(_explicit_cpu(sv, s, protocol), want, s)
    # the weight clamp: protocol 9 against protocol 10
    c = cases["clamp"][0]
    for protocol, hand in ((9, (1, 300, 1)), (10, (0, 255, 1))):
        got = _cpu(sv, s, protocol)
        assert (int(got[0][c]), int(got[1][c]), int(got[2][c])) == hand


def test_duplicate_entry_changes_no_result(sv, oracle):
    """The same body with its account listed once, twice and three times."""
    res = []
    for copies in (1, 2, 3):
        bld = ap.ABuilder(77)  # (the same seed: the same body bytes)
        m = bld.account(ap.ed(1), (1, 1, 2, 3), [(ED, 1, ap.ed(2)), (SP, 1, ap.ed(3), pl.payload_of(32))])
        b = bld.body(length=40)
        pos = [b.use(m) for _ in range(copies)]
        b.sig_ed(2)
        b.sig_payload(3, pl.payload_of(32))
        b.sig_ed(1)
        for level in (1, 2, 3):
            b.acheck(pos[-1], level)
        s = bld.finish(tp.pysign_signer(oracle), oracle)
        assert s["nk"] == 2 * copies and s["nq"] == copies
        got = _cpu(sv, s)
        cp.assert_equal(got, ap.expected(s, cp.oracle_verify(oracle)), s)
        res.append([x.tolist() for x in got[:3]])
    assert res[0] == res[1] == res[2] == [[1, 1, 1], [1, 2, 3], [0b001, 0b101, 0b111]]


def test_random_pool_matches_both_references(sv, oracle):
    verify = cp.oracle_verify(oracle)
    bld = ap.ABuilder(61)
    ap.random_pool(bld, 200)
    s = bld.finish(tp.pysign_signer(oracle), oracle)
    uses = np.bincount(s["bacct"], minlength=s["na"])
    assert s["nb"] == 200 and s["nc"] > 300 and s["nq"] > 40 and uses.max() >= 10 and (s["check_level"] == 0).any()
    assert (np.diff(s["bacct_begin"].astype(np.int64)) == 0).any()
    for protocol in (21, 9):
        want = ap.expected(s, verify, protocol)
        assert want[0].any() and not want[0].all() and want[2].any()
        cp.assert_equal(_cpu(sv, s, protocol), want, s)
        cp.assert_equal(_explicit_cpu(sv, s, protocol), want, s)


# ------------------------------------------------ every reject alone
def _raw(sv, fn_name, s, over=None, struct_size=None, protocol=21, null_out=False, nid=True):
    """One of the two host-array entry points through ctypes over a struct of the
    test's own; `over` replaces table pointers (None: NULL) and counts.  -> rc."""
    lib = sv.load_library()
    P = lambda a: a.ctypes.data  # noqa: E731
    ac = sv.sv_txaccounts()
    ac.struct_size = ctypes.sizeof(sv.sv_txaccounts) if struct_size is None else struct_size
    ac.protocol_version = protocol
    vals = dict(sig_len=s["sig_len"], acct_key=s["acct_key"], acct_thresholds=s["acct_thresholds"],
                asigner_begin=s["asigner_begin"], asigner_type=s["asigner_type"], asigner_weight=s["asigner_weight"],
                asigner_key=s["asigner_key"], asigner_payload=s["asigner_payload"], apayload=s["apayload"],
                apayload_len=s["apayload_len"], bacct_begin=s["bacct_begin"], bacct=s["bacct"],
                check_begin=s["check_begin"], check_acct=s["check_acct"], check_level=s["check_level"],
                check_needed=s["acheck_needed"], n_accounts=s["na"], n_asigners=s["nas"], n_apayloads=s["npay"],
                n_bacct=s["ne"], n_checks=s["nc"])
    top = dict(sig_begin=s["sig_begin"], hint=s["hint"], sig=s["sig"], kind=s["kind"], n_sigs=s["ns"])
    for k, v in (over or {}).items():
        (top if k in top else vals)[k] = v
    hold = []
    for k, v in vals.items():
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v)
            hold.append(v)
            v = P(v)
        setattr(ac, k, v)
    t = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in top.items()}
    nc = s["nc"]
    ok, weight, used = np.full(nc, 0xA5, np.uint8), np.full(nc, 0xA5A5A5A5, np.uint32), np.full(nc, 0xA5, np.uint64)
    nidb = np.frombuffer(tp.NETWORK_ID, np.uint8).copy()
    ptr = lambda v: P(v) if isinstance(v, np.ndarray) else v  # noqa: E731
    rc = getattr(lib, fn_name)(P(nidb) if nid else None, P(s["bodies"]), P(s["off"]), P(s["len"]), ptr(t["kind"]),
                               s["nb"], ptr(t["sig_begin"]), ptr(t["hint"]), ptr(t["sig"]), t["n_sigs"],
                               ctypes.byref(ac), None if null_out else P(ok), P(weight), P(used), None,
                               0 if fn_name.endswith("_cpu") else None)
    if rc != 0:
        assert (ok == 0xA5).all() and (weight == 0xA5A5A5A5).all() and (used == 0xA5).all(), "written before a reject"
    return rc


def _rejects(s):
    """{name: keyword arguments of _raw} -- each breaks exactly one rule of a valid set."""
    def edit(key, i, v, src=None):
        a = s[src or key].copy()
        a[i] = v
        return {key: a}
    b_checks = int(np.nonzero(np.diff(s["check_begin"].astype(np.int64)) > 0)[0][0])  # a body with checks
    c0 = int(s["check_begin"][b_checks])
    e0, e1 = int(s["bacct_begin"][b_checks]), int(s["bacct_begin"][b_checks + 1])
    g3 = int(np.nonzero(s["asigner_type"] == 3)[0][0])
    out = {
        "null network_id": dict(nid=False),
        "null accounts struct arrays: acct_key": dict(over={"acct_key": None}),
        "null acct_thresholds": dict(over={"acct_thresholds": None}),
        "null asigner_begin": dict(over={"asigner_begin": None}),
        "null asigner_type": dict(over={"asigner_type": None}),
        "null asigner_weight": dict(over={"asigner_weight": None}),
        "null asigner_key": dict(over={"asigner_key": None}),
        "null asigner_payload with a type-3 signer": dict(over={"asigner_payload": None}),
        "null apayload": dict(over={"apayload": None}),
        "null apayload_len": dict(over={"apayload_len": None}),
        "null bacct_begin": dict(over={"bacct_begin": None}),
        "null bacct": dict(over={"bacct": None}),
        "null check_begin": dict(over={"check_begin": None}),
        "null check_acct": dict(over={"check_acct": None}),
        "null check_level": dict(over={"check_level": None}),
        "null check_needed with a level-0 check": dict(over={"check_needed": None}),
        "null check_ok": dict(null_out=True),
        "null hint": dict(over={"hint": None}),
        "null sig": dict(over={"sig": None}),
        "null sig_begin": dict(over={"sig_begin": None}),
        "sig_begin does not start at 0": dict(over=edit("sig_begin", 0, 1)),
        "sig_begin decreases": dict(over=edit("sig_begin", 1, int(s["sig_begin"][2]) + 1)),
        "sig_begin ends past n_sigs": dict(over={"n_sigs": s["ns"] - 1}),
        "asigner_begin does not start at 0": dict(over=edit("asigner_begin", 0, 1)),
        "asigner_begin decreases": dict(over=edit("asigner_begin", 1, int(s["asigner_begin"][2]) + 1)),
        "asigner_begin ends past n_asigners": dict(over={"n_asigners": s["nas"] - 1}),
        "bacct_begin does not start at 0": dict(over=edit("bacct_begin", 0, 1)),
        "bacct_begin decreases": dict(over=edit("bacct_begin", 2, int(s["bacct_begin"][1]) - 1)),
        "bacct_begin ends past n_bacct": dict(over={"n_bacct": s["ne"] - 1}),
        "check_begin does not start at 0": dict(over=edit("check_begin", 0, 1)),
        "check_begin decreases": dict(over=edit("check_begin", 2, int(s["check_begin"][1]) - 1)),
        "check_begin ends past n_checks": dict(over={"n_checks": s["nc"] - 1}),
        "bacct entry == n_accounts": dict(over=edit("bacct", e0, s["na"])),
        "bacct entry 2^32 - 1": dict(over=edit("bacct", e0, 0xFFFFFFFF)),
        "check_acct == the body's entries": dict(over=edit("check_acct", c0, e1 - e0)),
        "level 4": dict(over=edit("check_level", c0, 4)),
        "signer type 4": dict(over=edit("asigner_type", 0, 4)),
        "type-3 payload index == n_apayloads": dict(over=edit("asigner_payload", g3, s["npay"])),
        "apayload_len 65": dict(over=edit("apayload_len", 0, 65)),
        "sig_len 65": dict(over=edit("sig_len", 0, 65)),
        "body kind 3": dict(over=edit("kind", 0, 3)),
        "protocol 7": dict(protocol=7),
        "struct_size one byte short": dict(struct_size=ctypes.sizeof(ctypes.c_void_p) * 16 + 8 + 5 * 8 - 1),
    }
    return out


@pytest.fixture(scope="module")
def valid(sv, oracle):
    """A small valid set the rejects are cut from (its first account has a signer, a type-3 signer exists, its
    second body has entries; nothing is signed: no verification is reached)."""
    bld = ap.ABuilder(9)
    a = bld.account(ap.ed(1), (1, 1, 2, 3), [(ED, 1, ap.ed(2)), (SP, 1, ap.ed(3), pl.payload_of(5))])
    z = bld.account(ap.ed(2), (1, 0, 0, 0))
    for t in range(4):
        b = bld.body(length=10 + t)
        b.sig_ed(1)
        b.sig_ed(2)
        p = [b.use(a), b.use(z)]
        b.acheck(p[t % 2], t % 4, 1)
        b.acheck(p[0], 0, 0)
    return bld.finish(tp.pysign_signer(oracle), oracle)


def test_every_reject_alone(sv, valid):
    """Every reject of the host forms, alone, on sv_ed25519_check_txbodies_accounts (before any device work: it
    answers on a host without a GPU too) and on _cpu; the unbroken set passes on _cpu."""
    s = valid
    assert ctypes.sizeof(sv.sv_txaccounts) == ctypes.sizeof(ctypes.c_void_p) * 16 + 8 + 5 * 8
    assert _raw(sv, "sv_ed25519_check_txbodies_accounts_cpu", s) == 0
    for name, kw in _rejects(s).items():
        for fn in ("sv_ed25519_check_txbodies_accounts", "sv_ed25519_check_txbodies_accounts_cpu"):
            assert _raw(sv, fn, s, **kw) == -1, (name, fn)


def test_binding_raises_on_the_same_inputs(sv, valid):
    s = valid
    ok = _cpu(sv, s)
    assert len(ok[0]) == s["nc"]
    for name, kw in _rejects(s).items():
        over = dict(kw.get("over") or {})
        if any(v is None for v in over.values()) or not over or "n_" in "".join(over):
            continue  # (NULL pointers and counts are not expressible through the binding)
        over = {("acheck_needed" if k == "check_needed" else k): v for k, v in over.items()}
        sl = over.pop("sig_len", s["sig_len"])
        for fn in (sv.check_txbodies_accounts, sv.check_txbodies_accounts_cpu):
            with pytest.raises((sv.SigVerifyError, ValueError)):
                fn(*ap.args(s, **over), sig_len=sl)
    for fn in (sv.check_txbodies_accounts, sv.check_txbodies_accounts_cpu):
        with pytest.raises(sv.SigVerifyError, match="SV_ERR_INVALID_ARG"):
            fn(*ap.args(s), sig_len=s["sig_len"], protocol_version=7)


def test_expanded_list_limit(sv, oracle):
    """63 signers + the master is the longest list (accepted: the edge set); 64 + the master is refused, 64 with
    master weight 0 accepted; a body with checks and 65 signatures is refused, without checks accepted."""
    rows = [ap.raw(hashlib.sha256(b"limit %d" % i).digest()) for i in range(64)]

    def build(master_weight, n_sigs=1, checks=True):
        bld = ap.ABuilder(3)
        a = bld.account(ap.ed(1), (master_weight, 1, 1, 1), [(ED, 1, r) for r in rows])
        b = bld.body(length=12)
        for _ in range(n_sigs):
            b.sig_raw(b"\1\2\3\4", bytes(64))
        p = b.use(a)
        if checks:
            b.acheck(p, 1)
        return bld
    s = build(0).finish(tp.pysign_signer(oracle), oracle)
    assert int(s["signer_begin"][1]) == 64 and _cpu(sv, s)[0].tolist() == [0]
    # (65 signers: the explicit tables cannot even be laid out by the explicit form -- only the by-account arrays)
    for fn in ("sv_ed25519_check_txbodies_accounts", "sv_ed25519_check_txbodies_accounts_cpu"):
        thr = s["acct_thresholds"].copy()
        thr[0, 0] = 1
        assert _raw(sv, fn, s, over={"acct_thresholds": thr}) == -1
    s = build(0, n_sigs=65, checks=False).finish(tp.pysign_signer(oracle), oracle)
    assert _raw(sv, "sv_ed25519_check_txbodies_accounts_cpu", s) == 0
    s2 = dict(s, check_begin=np.array([0, 1], np.uint64), check_acct=np.zeros(1, np.uint32),
              check_level=np.ones(1, np.uint8), acheck_needed=np.zeros(1, np.int32), nc=1)
    for fn in ("sv_ed25519_check_txbodies_accounts", "sv_ed25519_check_txbodies_accounts_cpu"):
        assert _raw(sv, fn, s2) == -1


# ------------------------------------------------ planner and packer
@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """tests/native/txacct_core.cpp built as the planner / packer shim."""
    so = str(tmp_path_factory.mktemp("txacct") / "libtxacctstage.so")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-DTXACCT_STAGE_SHIM",
           "-Wno-unknown-pragmas", "-o", so, os.path.join(HERE, "native", "txacct_core.cpp"), "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.hs_acct_plan.argtypes = [vp] * 8 + [ctypes.c_int] + [u64] * 7 + [vp, ctypes.c_int]
    lib.hs_acct_pack.argtypes = [vp] * 4 + [u64] + [vp] * 14
    return lib


WORDS = ("b0", "b1", "s0", "s1", "k0", "k1", "body_bytes", "o_sig", "o_hint", "o_off", "o_sb", "o_kb", "o_len",
         "o_kind", "o_body", "p_bytes", "e0", "e1", "c0", "c1", "nk", "nq", "ng", "o_eb", "o_cb", "o_ea", "o_ca",
         "o_need", "o_lvl", "o_sl", "bytes")


def _account_rows(s):
    """Per account [key rows, payload candidates], from the table alone."""
    acnt = np.zeros((s["na"], 2), np.uint32)
    for a in range(s["na"]):
        g = s["asigner_type"][int(s["asigner_begin"][a]):int(s["asigner_begin"][a + 1])]
        acnt[a] = (int(s["acct_thresholds"][a, 0] > 0) + int((g != 3).sum()), int((g == 3).sum()))
    return acnt


def _plan(stage, s, acnt, bounds, with_len=True, B0=0, B1=None):
    B1 = s["nb"] if B1 is None else B1
    zeros = np.zeros(s["nb"] + 1, np.uint64)
    out = np.zeros(31 * (s["nb"] + 1), np.uint64)
    P = lambda a: a.ctypes.data  # noqa: E731
    n = stage.hs_acct_plan(P(s["len"]), P(s["sig_begin"]), P(zeros), P(s["bacct_begin"]), P(s["bacct"]),
                           P(s["check_begin"]), P(s["check_acct"]), P(acnt), int(with_len), B0, B1, *bounds, P(out),
                           s["nb"] + 1)
    return [dict(zip(WORDS, (int(x) for x in out[31 * i:31 * i + 31]))) for i in range(n)], out


def _numpy_plan(s, acnt, bounds, B0, B1):
    """The planner restated: greedy runs of whole bodies under the five bounds, the expanded rows standing in for
    the explicit key / candidate / signer counts.  -> [(b0, b1, nk, nq, ng)]"""
    al16 = lambda x: (int(x) + 15) & ~15  # noqa: E731
    sb, eb, cb = (s[k].astype(np.int64) for k in ("sig_begin", "bacct_begin", "check_begin"))
    rows = []
    for t in range(s["nb"]):
        ent = s["bacct"][eb[t]:eb[t + 1]]
        k, q = int(acnt[ent, 0].sum()), int(acnt[ent, 1].sum())
        g = sum(int(acnt[ent[int(p)]].sum()) for p in s["check_acct"][cb[t]:cb[t + 1]])
        rows.append((k, q, g))
    max_s, max_k, max_b, max_c, max_g = bounds
    out, t = [], B0
    while t < B1:
        b0, nk, nq, ng, nbytes = t, 0, 0, 0, 0
        while True:
            nbytes += al16(s["len"][t])
            nk, nq, ng = nk + rows[t][0], nq + rows[t][1], ng + rows[t][2]
            t += 1
            if not (t < B1 and sb[t + 1] - sb[b0] <= max_s and nk + nq + rows[t][0] + rows[t][1] <= max_k
                    and cb[t + 1] - cb[b0] <= max_c and ng + rows[t][2] <= max_g
                    and nbytes + al16(s["len"][t]) <= max_b):
                break
        out.append((b0, t, nk, nq, ng))
    return out


def test_planner_and_packer_against_numpy(sv, oracle, stage):
    bld = ap.ABuilder(19)
    ap.random_pool(bld, 150, n_accounts=12)
    s = bld.finish(tp.pysign_signer(oracle), oracle, layout_only=True)
    acnt = _account_rows(s)
    # (the per-account rows agree with the Python expansion's totals)
    assert int(acnt[s["bacct"], 0].sum()) == s["nk"] - sum(
        1 for b in s["B"] if b.keys and b.keys[-1] == ("raw", hashlib.sha256(b"no key").digest())) \
        and int(acnt[s["bacct"], 1].sum()) == s["nq"]
    big = 1 << 18
    al16 = lambda x: (int(x) + 15) & ~15  # noqa: E731
    sb, eb, cb = (s[k].astype(np.int64) for k in ("sig_begin", "bacct_begin", "check_begin"))
    crossing = 0
    for bounds in ((big, big, 64 << 20, big, big), (25, big, 64 << 20, big, big), (big, 9, 64 << 20, big, big),
                   (big, big, 700, big, big), (big, big, 64 << 20, 3, big), (big, big, 64 << 20, big, 5),
                   (1, 1, 16, 1, 1)):
        for with_len in (True, False):
            for B0, B1 in ((0, s["nb"]), (37, 111)):
                plan, _ = _plan(stage, s, acnt, bounds, with_len, B0, B1)
                want = _numpy_plan(s, acnt, bounds, B0, B1)
                assert [(c["b0"], c["b1"], c["nk"], c["nq"], c["ng"]) for c in plan] == want, bounds
                if bounds[0] < big or bounds[1] < big or bounds[3] < big:
                    assert len(plan) > 3  # forced multi-chunk plans
                for c in plan:
                    k, m = c["b1"] - c["b0"], c["s1"] - c["s0"]
                    ne, nc = c["e1"] - c["e0"], c["c1"] - c["c0"]
                    assert (c["s0"], c["s1"], c["k0"], c["k1"]) == (sb[c["b0"]], sb[c["b1"]], 0, 0)
                    assert (c["e0"], c["e1"], c["c0"], c["c1"]) == (eb[c["b0"]], eb[c["b1"]], cb[c["b0"]], cb[c["b1"]])
                    assert c["o_sig"] == 0 and c["o_eb"] == al16(c["p_bytes"]) and c["o_cb"] == c["o_eb"] + 8 * (k + 1)
                    assert c["o_ea"] == c["o_cb"] + 8 * (k + 1) and c["o_ca"] == c["o_ea"] + 4 * ne
                    assert c["o_need"] == c["o_ca"] + 4 * nc and c["o_lvl"] == c["o_need"] + 4 * nc
                    assert c["o_sl"] == c["o_lvl"] + nc and c["bytes"] == al16(c["o_sl"] + (m if with_len else 0) + 1)
                # an account referenced from both sides of a chunk boundary
                for c, d in zip(plan, plan[1:]):
                    left = set(s["bacct"][c["e0"]:c["e1"]].tolist())
                    crossing += bool(left & set(s["bacct"][d["e0"]:d["e1"]].tolist()))
    assert crossing > 20
    # the packed image of every chunk of a small-bound plan, guard bytes behind it
    P = lambda a: a.ctypes.data  # noqa: E731
    zeros = np.zeros(s["nb"] + 1, np.uint64)
    for with_len in (True, False):
        plan, words = _plan(stage, s, acnt, (9, 12, 900, 7, 30), with_len)
        assert len(plan) > 10
        for i, c in enumerate(plan):
            img = np.full(c["bytes"] + 64, 0xC3, np.uint8)
            chunk = words[31 * i:31 * i + 31].copy()
            stage.hs_acct_pack(P(s["bodies"]), P(s["off"]), P(s["len"]), P(s["kind"]), s["nb"], P(s["sig_begin"]),
                               P(s["hint"]), P(s["sig"]), P(zeros), P(s["sig_len"]) if with_len else None,
                               P(s["bacct_begin"]), P(s["bacct"]), P(s["check_begin"]), P(s["check_acct"]),
                               P(s["check_level"]), P(s["acheck_needed"]) if with_len else None, P(acnt), P(chunk),
                               P(img))
            assert (img[c["bytes"]:] == 0xC3).all(), "a write past the planned image"
            k, m, ne, nc = c["b1"] - c["b0"], c["s1"] - c["s0"], c["e1"] - c["e0"], c["c1"] - c["c0"]
            view = lambda o, n, dt: img[o:o + n * np.dtype(dt).itemsize].view(dt)  # noqa: E731
            assert (img[c["o_sig"]:c["o_sig"] + 64 * m].reshape(-1, 64) == s["sig"][c["s0"]:c["s1"]]).all()
            assert (img[c["o_hint"]:c["o_hint"] + 4 * m].reshape(-1, 4) == s["hint"][c["s0"]:c["s1"]]).all()
            assert (view(c["o_sb"], k + 1, np.uint64) == s["sig_begin"][c["b0"]:c["b1"] + 1] - np.uint64(c["s0"])).all()
            assert (view(c["o_kb"], k + 1, np.uint64) == 0).all()
            assert (view(c["o_eb"], k + 1, np.uint64) == s["bacct_begin"][c["b0"]:c["b1"] + 1] - np.uint64(c["e0"])).all()
            assert (view(c["o_cb"], k + 1, np.uint64) == s["check_begin"][c["b0"]:c["b1"] + 1] - np.uint64(c["c0"])).all()
            assert (view(c["o_ea"], ne, np.uint32) == s["bacct"][c["e0"]:c["e1"]]).all()  # (global account indices)
            assert (view(c["o_ca"], nc, np.uint32) == s["check_acct"][c["c0"]:c["c1"]]).all()
            assert (view(c["o_lvl"], nc, np.uint8) == s["check_level"][c["c0"]:c["c1"]]).all()
            need = s["acheck_needed"][c["c0"]:c["c1"]] if with_len else np.zeros(nc, np.int32)
            assert (view(c["o_need"], nc, np.int32) == need).all()
            if with_len:
                assert (view(c["o_sl"], m, np.uint8) == s["sig_len"][c["s0"]:c["s1"]]).all()
            for t in range(c["b0"], c["b1"]):
                o = c["o_body"] + int(view(c["o_off"], k, np.uint64)[t - c["b0"]])
                n = int(s["len"][t])
                assert (img[o:o + n] == s["bodies"][int(s["off"][t]):int(s["off"][t]) + n]).all()


# ------------------------------------------------ host mirror (prefetch 7)
class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    st = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(st))
    return st


def _gpu(sv):
    try:
        return sv.device_count() > 0
    except sv.SigVerifyError:
        return False


def _host_lib(sv):
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_signer_lists_built.restype = ctypes.c_uint64
    return host


@pytest.mark.parametrize("with_payload", [True, False])
def test_mirror_prefetch7_matches_prefetch0(sv, oracle, with_payload):
    """The envelope pool of test_mirror_prefetch5_matches_prefetch0 (same units, same seed): prefetch 7 gives
    prefetch 0's codes and hashes through ONE engine call (the CPU form on a host without a GPU, one fallback
    counted), lists every account once, and builds no signer list -- neither when it lists the checks nor when it
    consumes the decisions -- where prefetch 5 builds them per check."""
    host = _host_lib(sv)
    s = eb.build_set(2, 23, tp.pysign_signer(oracle), with_payload=with_payload)

    def call(prefetch, for_apply=0, protocol=21):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], protocol,
                                         s["bodies"], s["ebody"], prefetch=prefetch, for_apply=for_apply)

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all(), ref["code"]
    assert eb.txBAD_AUTH in ref["code"] and eb.txSUCCESS in ref["code"]
    _stats(host)
    built = host.svh_signer_lists_built()
    res, checks, ch, fb = call(7)
    assert host.svh_signer_lists_built() == built, "prefetch 7 built a std::vector<Signer>"
    st = _stats(host)
    assert (res == ref).all()
    assert (ch == ch0).all() and (fb == fb0).all()
    assert (ch == s["contents_hash"]).all() and (fb == s["fee_bump_hash"]).all()
    assert checks == 2 * s["n"] + s["kinds"].count("fee_bump")
    assert (st.fallbacks == 0 and st.gpu_batches == 1) if _gpu(sv) else (st.fallbacks == 1 and st.gpu_batches == 0)
    # prefetch 5 / 6 on the same set: the same codes, one list per check when listing them and more when the
    # decisions are consumed (a transaction stops at its first failing check, so fewer than one per check there)
    built = host.svh_signer_lists_built()
    res5, checks5, _, _ = call(6 if with_payload else 5)
    assert (res5 == ref).all() and checks5 == checks and host.svh_signer_lists_built() - built > checks
    assert (call(7, for_apply=1)[0] == call(0, for_apply=1)[0]).all()
    # protocol 7: every check is true without the engine; protocols on both sides of the clamp and of the
    # extra signers (19) and fee bumps (13)
    for protocol in (7, 9, 12, 18):
        r7, r0 = call(7, protocol=protocol), call(0, protocol=protocol)
        assert (r7[0] == r0[0]).all() and (r7[2] == r0[2]).all() and (r7[3] == r0[3]).all(), protocol


def _special_envelopes(oracle):
    """The special envelopes of test_mirror_prefetch5_special_envelopes, restated: a fee bump with an unused outer
    signature, operations whose source account is missing (with and without that key's signature), a HASH_X signer
    with a short preimage, extra signers (present and missing), a missing transaction source, a surplus inner
    signature, a good fee bump, and two envelopes beyond the engine's limits (65 signatures; a fee bump whose inner
    transaction has 65).  -> (names, envelope arrays with junk hashes, the other arrays, accounts, bodies, ebody)"""
    rng = np.random.default_rng(77)
    A, F, X, E, G = range(5)
    seeds = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    preimage = b"hash-x preimage of 29 bytes..."[:29]
    hxkey = hashlib.sha256(preimage).digest()
    names = ("bump_extra_sig", "op_no_account_signed", "op_no_account_unsigned", "hashx", "extra_signer",
             "extra_signer_missing", "no_source", "surplus_sig", "bump_ok", "over_limit", "bump_over_limit")
    blob, ebody = bytearray(), np.zeros(len(names), eb.ENVELOPE_BODY)
    jobs, plans = [(k, bytes(32)) for k in range(5)], []

    def new_body():
        b = bytes(rng.integers(0, 256, 4 * int(rng.integers(25, 60)), dtype=np.uint8))
        off = len(blob)
        blob.extend(b)
        return off, b

    def job(k, msg):
        jobs.append((k, msg))
        return len(jobs) - 1

    for t, name in enumerate(names):
        off, body = new_body()
        ebody[t]["off"], ebody[t]["len"], ebody[t]["kind"] = off, len(body), tp.V1
        inner = tp.contents_hash(tp.V1, body)
        plan = {"inner": inner, "outer": bytes(32), "rows": [job(A, inner)], "outer_rows": []}
        if name.startswith("bump"):
            ooff, obody = new_body()
            ebody[t]["outer_off"], ebody[t]["outer_len"] = ooff, len(obody)
            plan["outer"] = tp.contents_hash(tp.FEE_BUMP, obody)
            plan["outer_rows"] = [job(F, plan["outer"])] + ([job(A, plan["outer"])] if name == "bump_extra_sig" else [])
        if name == "op_no_account_signed":
            plan["rows"].append(job(X, inner))
        if name == "extra_signer":
            plan["rows"].append(job(E, inner))
        if name == "surplus_sig":
            plan["rows"].append(job(G, inner))
        if name == "no_source":
            plan["rows"] = [job(X, inner)]
        plans.append(plan)
    pk, sig = tp.pysign_signer(oracle)(seeds[[k for k, _ in jobs]],
                                       np.array([np.frombuffer(m, np.uint8) for _, m in jobs], np.uint8))
    keys = [pk[k].tobytes() for k in range(5)]
    hx = lambda k: keys[k].hex()  # noqa: E731
    dsig = lambda row: {"hint": pk[row].tobytes()[28:].hex(), "sig": sig[row].tobytes().hex()}  # noqa: E731
    accounts = [{"id": hx(A), "thresholds": [1, 0, 0, 0], "signers": []},
                {"id": hx(F), "thresholds": [1, 0, 0, 0], "signers": []},
                # no master key: a HASH_X signer alone
                {"id": hx(G), "thresholds": [0, 1, 1, 1], "signers": [{"type": 2, "key": hxkey.hex(), "weight": 1}]}]
    sets = {}
    for which in ("envs", "envs_blank"):
        es = ev.EnvelopeSet()
        for a in accounts:
            es.account(a)
        for t, name in enumerate(names):
            pl_ = plans[t]
            inner, outer = (pl_["inner"], pl_["outer"]) if which == "envs" else (b"\xaa" * 32, b"\xbb" * 32)
            sigs = [dsig(r) for r in pl_["rows"]]
            source, ops, extra, fee = hx(A), [{"level": 2}], (), None
            if name.startswith("op_no_account"):
                ops = [{"level": 1}, {"level": 2, "source": hx(X)}]
            if name == "hashx":
                source = hx(G)
                sigs = [{"hint": hxkey[28:].hex(), "sig": preimage.hex()}]
            if name.startswith("extra_signer"):
                extra = [{"type": 0, "key": hx(E), "weight": 1}]
            if name == "no_source":
                source = hx(X)
            if name.endswith("over_limit"):  # the signer's signature last, behind 64 that match nothing
                sigs = [{"hint": "00000000", "sig": bytes([i]).hex() * 64} for i in range(64)] + sigs
            if name.startswith("bump"):
                fee = {"hash": outer.hex(), "fee_source": hx(F), "sigs": [dsig(r) for r in pl_["outer_rows"]]}
            es.envelope(source, inner.hex(), sigs, ops, extra=extra, fee_bump=fee)
        sets[which] = es.arrays()
    return names, sets, len(accounts), np.frombuffer(bytes(blob), np.uint8).copy(), ebody


def test_mirror_prefetch7_special_envelopes(sv, oracle):
    """Prefetch 7 on the special envelopes: prefetch 0's codes in both modes; every envelope but the two over the
    limits is decided by the engine (they go to SignatureChecker, they alone), one engine call per prefetch-7 call."""
    host = _host_lib(sv)
    names, sets, naccounts, bodies, ebody = _special_envelopes(oracle)
    n = len(names)

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, sets["envs_blank"][0], *sets["envs"][1:], n, naccounts, 21, bodies,
                                         ebody, prefetch=prefetch, for_apply=for_apply)

    ref = call(0)
    assert dict(zip(names, ref[0]["code"].tolist())) == {
        "bump_extra_sig": -10, "op_no_account_signed": 0, "op_no_account_unsigned": -1, "hashx": 0, "extra_signer": 0,
        "extra_signer_missing": -6, "no_source": -8, "surplus_sig": -10, "bump_ok": 1, "over_limit": -10,
        "bump_over_limit": -13}
    _stats(host)
    for for_apply in (0, 1):
        want, got = call(0, for_apply), call(7, for_apply)
        assert (got[0] == want[0]).all(), (got[0], want[0])
        assert (got[2] == want[2]).all() and (got[3] == want[3]).all()
        assert got[1] == 3 + 3 + 3 + 2 + 3 + 3 + 0 + 2 + 3 + 0 + 1  # (as prefetch 5: the checks the engine decided)
    st = _stats(host)
    assert (st.gpu_batches, st.fallbacks) == ((2, 0) if _gpu(sv) else (0, 2))


# ------------------------------------------------ host code under sanitizers
def test_host_code_under_sanitizers(tmp_path):
    """tests/native/txacct_core.cpp (its own main) + the CPU path, built with
    ASan and UBSan and run directly: nothing is loaded into Python."""
    exe = str(tmp_path / "txacct_core")
    # (the sanitizer runtimes linked statically: the program needs nothing preloaded)
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(HERE, "native", "txacct_core.cpp"),
           os.path.join(REPO, "stellar-core_amd", "csrc", "sv_cpu.cpp"), "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "txacct_core ok" in r.stdout, r.stdout[-4000:]
