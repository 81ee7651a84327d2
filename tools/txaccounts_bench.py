#!/usr/bin/env python3
"""Measurement tool for signature checks against a device-side account table
(sv_ed25519_check_txbodies_accounts*); prints one JSON line (the one committed
as profiles/r11/txaccounts/bench.json).

Three workloads, each in its explicit form (sv_ed25519_check_txbodies*) and
restated by account -- the same bodies, signatures and decisions:
  single      tools/txchecks_bench.py's set: n single-signature bodies, two
              checks each; one account per body (its one key, master weight 1)
  multisig    its second set: m bodies of 1..20 signatures and as many signers,
              a source check plus 1..5 operation checks; one account per body
              (master + the other keys as signers), the checks at level 0
  checkpoint  n bodies over n / 16 accounts: every account signs about 16
              bodies, each with one signature and two checks (levels 1 and 2)
Per workload, after one checked warm-up call per leg, medians of `reps` rounds
with the legs alternated inside each round:
  (a) by-account, device-resident     sv_ed25519_check_txbodies_accounts_device
  (b) explicit, device-resident       sv_ed25519_check_txbodies_device
  (c) the expansion kernels alone (sv_launch_acct_table / _count / _fill)
      between two events on the caller's stream
  (d) by-account from host buffers    sv_ed25519_check_txbodies_accounts
  (e) explicit from host buffers      sv_ed25519_check_txbodies
and the bytes each host form hands to the engine (the sum of the caller's array
sizes, not a count taken inside the engine: its staged images add alignment
padding and rebased CSR words, and the account table goes up once per slot),
and once, on one generated envelope set (tests/envelope_bodies.py):
  the mirror: svh_check_envelopes_bodies with prefetch 5, 6 and 7, and the
  std::vector<Signer> copies each call builds (svh_signer_lists_built).
With --explicit-only only
(b) and (e) run (a build without the by-account entry points; --root names the
tree whose package is imported).

  python tools/txaccounts_bench.py [--n N] [--m M] [--reps R] [--units U] [--out FILE] [--explicit-only]
                                   [--root DIR]"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_account_one_per_body(s):
    """An explicit txchecks_bench set restated: body t's keys are account t (the
    first its master key with weight 1, the others its signers with weight 1),
    every check names it at level 0 with the check's own needed weight."""
    nb = s["nb"]
    kb = s["key_begin"].astype(np.int64)
    k = np.diff(kb)
    first = np.zeros(s["n"], bool)
    first[kb[:-1]] = True
    thr = np.zeros((nb, 4), np.uint8)
    thr[:, 0] = 1
    ns = int((~first).sum())
    s.update(acct_key=s["key"][first], acct_thresholds=thr,
             asigner_begin=np.concatenate([[0], np.cumsum(k - 1)]).astype(np.uint64),
             asigner_type=np.zeros(ns, np.uint8), asigner_weight=np.ones(ns, np.uint32), asigner_key=s["key"][~first],
             asigner_payload=np.zeros(ns, np.uint32), apayload=np.zeros((0, 64), np.uint8),
             apayload_len=np.zeros(0, np.uint8), bacct_begin=np.arange(nb + 1, dtype=np.uint64),
             bacct=np.arange(nb, dtype=np.uint32), check_acct=np.zeros(s["nc"], np.uint32),
             check_level=np.zeros(s["nc"], np.uint8), na=nb, nas=ns, ne=nb)
    return s


def build_checkpoint(sv, tb, dev, stream, nb, per_account, seed):
    """nb bodies over nb / per_account accounts; body t is signed by account
    t % accounts (one reject in sixteen) and has two checks over it."""
    import torch
    s = tb.build(sv, dev, stream, nb, np.ones(nb, np.int64), seed)  # (bodies and digests; its signatures are redone)
    na = max(1, nb // per_account)
    rng = np.random.default_rng(seed + 1)
    seeds = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    owner = (np.arange(nb) % na)
    t_seed = torch.from_numpy(seeds[owner]).to(dev)
    t_msg = torch.from_numpy(s["digests"]).to(dev)
    t_pk = torch.empty((nb, 32), dtype=torch.uint8, device=dev)
    t_sig = torch.empty((nb, 64), dtype=torch.uint8, device=dev)
    sv.sign_device(0, t_seed.data_ptr(), t_msg.data_ptr(), nb, t_pk.data_ptr(), t_sig.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    pk, sig = t_pk.cpu().numpy(), t_sig.cpu().numpy()
    sig[::16, 40] ^= 0x08
    nc = 2 * nb
    thr = np.ones((na, 4), np.uint8)
    want = np.repeat(s["want"], 2)
    s.update(key=pk, sig=sig, hint=np.ascontiguousarray(pk[:, 28:]),
             check_begin=(2 * np.arange(nb + 1)).astype(np.uint64), check_needed=np.ones(nc, np.int32),
             signer_begin=np.arange(nc + 1, dtype=np.uint64), signer_type=np.zeros(nc, np.uint8),
             signer_weight=np.ones(nc, np.uint32), signer_key=np.repeat(np.arange(nb), 2).astype(np.uint32), nc=nc,
             ng=nc, want_ok=want.astype(np.uint8), want_weight=want.astype(np.uint32),
             acct_key=pk[:na].copy(), acct_thresholds=thr, asigner_begin=np.zeros(na + 1, np.uint64),
             asigner_type=np.zeros(0, np.uint8), asigner_weight=np.zeros(0, np.uint32),
             asigner_key=np.zeros((0, 32), np.uint8), asigner_payload=np.zeros(0, np.uint32),
             apayload=np.zeros((0, 64), np.uint8), apayload_len=np.zeros(0, np.uint8),
             bacct_begin=np.arange(nb + 1, dtype=np.uint64), bacct=owner.astype(np.uint32),
             check_acct=np.zeros(nc, np.uint32), check_level=np.tile(np.array([1, 2], np.uint8), nb), na=na, nas=0,
             ne=nb)
    return s


EXPLICIT = ("bodies", "off", "len", "kind", "sig_begin", "key_begin", "hint", "sig", "key", "check_begin",
            "check_needed", "signer_begin", "signer_type", "signer_weight", "signer_key")
BY_ACCOUNT = ("bodies", "off", "len", "kind", "sig_begin", "hint", "sig", "acct_key", "acct_thresholds",
              "asigner_begin", "asigner_type", "asigner_weight", "asigner_key", "asigner_payload", "apayload",
              "apayload_len", "bacct_begin", "bacct", "check_begin", "check_acct", "check_level", "check_needed")


class AcctTab(ctypes.Structure):  # csrc/txacct.h sv_acct_tab
    _fields_ = [(f, ctypes.c_void_p) for f in ("key", "thr", "sbeg", "stype", "sweight", "skey", "spay", "pay",
                                               "plen")] + [(f, ctypes.c_uint64) for f in ("na", "ns", "np")]


class AcctUse(ctypes.Structure):  # sv_acct_use
    _fields_ = [(f, ctypes.c_void_p) for f in ("ebeg", "eacct", "cbeg", "cacct", "clevel", "cneed")] + [
        (f, ctypes.c_uint64) for f in ("nb", "ne", "nc")]


class AcctOut(ctypes.Structure):  # sv_acct_out
    _fields_ = [(f, ctypes.c_void_p) for f in ("key_begin", "pkey_begin", "signer_begin", "check_needed", "key",
                                               "pkey", "ppay", "plen", "gtype", "gweight", "gkey")] + [
        (f, ctypes.c_uint64) for f in ("nk", "nq", "ng")]


def run(sv, tb, dev, stream, s, reps, explicit_only):
    import torch
    lib = sv.load_library()
    nb, n, nc, ng = s["nb"], s["n"], s["nc"], s["ng"]
    nk = int(s["key_begin"][-1])
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    names = EXPLICIT if explicit_only else tuple(dict.fromkeys(EXPLICIT + BY_ACCOUNT))
    t = {k: up(s[k] if s[k].size else np.zeros(16, np.uint8)) for k in names}
    p = lambda name: t[name].data_ptr()  # noqa: E731
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    t_ok = torch.zeros(nc, dtype=torch.uint8, device=dev)
    t_w = torch.zeros(nc, dtype=torch.int32, device=dev)
    t_u = torch.zeros(nc, dtype=torch.int64, device=dev)
    NID = tb.NETWORK_ID

    def explicit_device():
        sv.check_txbodies_device(0, NID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"),
                                 p("sig"), n, p("key_begin"), p("key"), nk, p("check_begin"), p("check_needed"), nc,
                                 p("signer_begin"), p("signer_type"), p("signer_weight"), p("signer_key"), ng,
                                 t_ok.data_ptr(), t_w.data_ptr(), t_u.data_ptr(), d_digests=t_dig.data_ptr(),
                                 stream=stream)

    def account_device():
        sv.check_txbodies_accounts_device(
            0, NID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"), n,
            p("acct_key"), p("acct_thresholds"), p("asigner_begin"), p("asigner_type"), p("asigner_weight"),
            p("asigner_key"), p("asigner_payload"), p("apayload"), p("apayload_len"), s["na"], s["nas"], 0,
            p("bacct_begin"), p("bacct"), s["ne"], p("check_begin"), p("check_acct"), p("check_level"),
            p("check_needed"), nc, t_ok.data_ptr(), t_w.data_ptr(), t_u.data_ptr(), d_digests=t_dig.data_ptr(),
            stream=stream)

    out = {}
    host_head = (NID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"])

    def explicit_host():
        out["e"] = sv.check_txbodies(*host_head, s["key_begin"], s["key"], s["check_begin"], s["check_needed"],
                                     s["signer_begin"], s["signer_type"], s["signer_weight"], s["signer_key"], device=0)

    def account_host():
        out["d"] = sv.check_txbodies_accounts(*host_head, *(s[k] for k in BY_ACCOUNT[7:]), device=0)

    # (c): the expansion alone, into buffers of the tool's own
    if not explicit_only:
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        lib.sv_acct_tab_ws_bytes.restype = lib.sv_acct_ws_bytes.restype = ctypes.c_size_t
        lib.sv_acct_tab_ws_bytes.argtypes = [u64, u64]
        lib.sv_acct_ws_bytes.argtypes = [u64, u64, u64]
        for f in (lib.sv_launch_acct_count, lib.sv_launch_acct_fill):
            f.argtypes = [vp, vp, vp, vp, vp, vp]
        lib.sv_launch_acct_table.argtypes = [vp, vp, vp]
        T = AcctTab(p("acct_key"), p("acct_thresholds"), p("asigner_begin"), p("asigner_type"), p("asigner_weight"),
                    p("asigner_key"), p("asigner_payload"), p("apayload"), p("apayload_len"), s["na"], s["nas"], 0)
        U = AcctUse(p("bacct_begin"), p("bacct"), p("check_begin"), p("check_acct"), p("check_level"),
                    p("check_needed"), nb, s["ne"], nc)
        buf = lambda b: torch.zeros(int(b) + 64, dtype=torch.uint8, device=dev)  # noqa: E731
        w_tab, w_use = buf(lib.sv_acct_tab_ws_bytes(s["na"], s["nas"])), buf(lib.sv_acct_ws_bytes(nb, s["ne"], nc))
        o = {k: buf(b) for k, b in (("kb", 8 * (nb + 1)), ("qb", 8 * (nb + 1)), ("gb", 8 * (nc + 1)), ("need", 4 * nc),
                                     ("key", 32 * nk), ("q", 64), ("gt", ng), ("gw", 4 * ng), ("gk", 4 * ng))}
        O = AcctOut(o["kb"].data_ptr(), o["qb"].data_ptr(), o["gb"].data_ptr(), o["need"].data_ptr(),
                    o["key"].data_ptr(), o["q"].data_ptr(), o["q"].data_ptr(), o["q"].data_ptr(), o["gt"].data_ptr(),
                    o["gw"].data_ptr(), o["gk"].data_ptr(), nk, 0, ng)

        def expansion_alone():
            st = stream or None
            assert lib.sv_launch_acct_table(ctypes.byref(T), w_tab.data_ptr(), st) == 0
            for f in (lib.sv_launch_acct_count, lib.sv_launch_acct_fill):
                assert f(ctypes.byref(T), w_tab.data_ptr(), ctypes.byref(U), ctypes.byref(O), w_use.data_ptr(), st) == 0

    def dev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def results_ok():
        torch.cuda.synchronize(dev)
        assert (t_ok.cpu().numpy() == s["want_ok"]).all()
        assert (t_w.cpu().numpy().view(np.uint32) == s["want_weight"]).all()
        assert (t_dig.cpu().numpy() == s["digests"]).all()
        t_ok.zero_()

    # the untimed warm-up call of every leg, with its results checked
    explicit_device()
    results_ok()
    explicit_host()
    assert (out["e"][0] == s["want_ok"]).all() and (out["e"][1] == s["want_weight"]).all()
    dev_legs = [("b_explicit_device_ms", explicit_device)]
    host_legs = [("e_explicit_host_ms", explicit_host)]
    if not explicit_only:
        account_device()
        results_ok()
        expansion_alone()
        torch.cuda.synchronize(dev)
        # (the expansion's tables are the explicit ones, byte for byte)
        for k, name in (("kb", "key_begin"), ("gb", "signer_begin"), ("need", "check_needed"), ("key", "key"),
                        ("gt", "signer_type"), ("gw", "signer_weight"), ("gk", "signer_key")):
            want = np.ascontiguousarray(s[name]).view(np.uint8).reshape(-1)
            assert (o[k].cpu().numpy()[:want.size] == want).all(), name
        account_host()
        for i in range(3):
            assert (out["d"][i] == out["e"][i]).all()
        assert (out["d"][3] == s["digests"]).all()
        dev_legs.insert(0, ("a_account_device_ms", account_device))
        host_legs.insert(0, ("d_account_host_ms", account_host))
    legs = {k: [] for k, _ in dev_legs + host_legs}
    if not explicit_only:
        legs["c_expansion_ms"] = []
    for rnd in range(reps):
        # (one untimed call after the host-bound legs, during which the GPU's clocks drop; the legs of a pair take
        # turns at going first)
        explicit_device()
        torch.cuda.synchronize(dev)
        for name, fn in dev_legs[::1 - 2 * (rnd & 1)]:
            legs[name].append(dev_ms(fn))
        if not explicit_only:
            legs["c_expansion_ms"].append(dev_ms(expansion_alone))
        for name, fn in host_legs[::1 - 2 * (rnd & 1)]:
            legs[name].append(host_ms(fn))
    r = {k: round(statistics.median(v), 4) for k, v in legs.items()}
    r.update({k.replace("_ms", "_min_max_ms"): [round(min(v), 4), round(max(v), 4)] for k, v in legs.items()})
    size = lambda keys: int(sum(np.ascontiguousarray(s[k]).nbytes for k in keys))  # noqa: E731
    r.update(bodies=nb, signatures=n, checks=nc, expanded_keys=nk, expanded_signers=ng,
             bytes_up_explicit=size(EXPLICIT))
    if not explicit_only:
        r.update(accounts=s["na"], account_signers=s["nas"], bytes_up_by_account=size(BY_ACCOUNT),
                 a_over_b_pct=round(100.0 * (r["a_account_device_ms"] / r["b_explicit_device_ms"] - 1), 2),
                 d_over_e_pct=round(100.0 * (r["d_account_host_ms"] / r["e_explicit_host_ms"] - 1), 2))
    return r


def mirror(sv, units, reps):
    """svh_check_envelopes_bodies on units x 6 generated envelopes (the signed-payload unit included), prefetch 5,
    6 and 7 alternated."""
    import envelope_bodies as eb
    import txbodies_pool as tp
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_signer_lists_built.restype = ctypes.c_uint64
    s = eb.build_set(units, 31, tp.device_signer(sv), with_payload=True)

    def call(prefetch):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch)

    ref = call(0)
    lists = {}
    for p in (5, 6, 7):  # the untimed warm-up, with its results checked
        built = host.svh_signer_lists_built()
        got = call(p)
        lists[p] = int(host.svh_signer_lists_built() - built)
        assert (got[0] == ref[0]).all() and (got[2] == ref[2]).all() and (got[3] == ref[3]).all()
    legs = {5: [], 6: [], 7: []}
    for rnd in range(reps):
        for p in ((5, 6, 7), (7, 6, 5), (6, 7, 5))[rnd % 3]:
            t0 = time.perf_counter()
            call(p)
            legs[p].append((time.perf_counter() - t0) * 1e3)
    r = {"prefetch%d_ms" % p: round(statistics.median(v), 4) for p, v in legs.items()}
    r.update({"prefetch%d_min_max_ms" % p: [round(min(v), 4), round(max(v), 4)] for p, v in legs.items()})
    r.update({"prefetch%d_signer_lists_built" % p: n for p, n in lists.items()})
    r.update(envelopes=s["n"], p7_over_p6_pct=round(100.0 * (r["prefetch7_ms"] / r["prefetch6_ms"] - 1), 2),
             p7_over_p5_pct=round(100.0 * (r["prefetch7_ms"] / r["prefetch5_ms"] - 1), 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--units", type=int, default=4000, help="envelope units (6 envelopes each) of the mirror legs")
    ap.add_argument("--explicit-only", action="store_true")
    ap.add_argument("--root", default=REPO, help="the tree whose stellar-core_amd package is imported")
    ap.add_argument("--out", default="", help="where the JSON line is also written")
    a = ap.parse_args()
    for d in (os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
        sys.path.insert(0, d)
    import torch
    import txchecks_bench as cb
    import txpairs_bench as tb
    # --root goes in LAST: the helper modules above put this tree's root at the front of sys.path as they load
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sv = importlib.import_module("stellar-core_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(sv.__file__))) == root, (sv.__file__, root)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(5, a.reps)
    res = {"tool": "tools/txaccounts_bench.py", "reps": reps, "explicit_only": bool(a.explicit_only),
           "kernel_source_digest": sv.kernel_source_digest(),
           "package": os.path.relpath(os.path.abspath(sv.__file__), REPO),
           "library": os.path.relpath(sv.LIB_PATH, REPO)}
    single = cb.add_checks(tb.build(sv, dev, stream, a.n, np.ones(a.n, np.int64), 20), np.ones(a.n, np.int64),
                           np.random.default_rng(23))
    res["single"] = run(sv, tb, dev, stream, by_account_one_per_body(single), reps, a.explicit_only)
    del single
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 21, a.m)
    multi = cb.add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)
    res["multisig"] = run(sv, tb, dev, stream, by_account_one_per_body(multi), reps, a.explicit_only)
    del multi
    res["checkpoint"] = run(sv, tb, dev, stream, build_checkpoint(sv, tb, dev, stream, a.n, 16, 24), reps,
                            a.explicit_only)
    if not a.explicit_only:
        res["mirror"] = mirror(sv, a.units, reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
