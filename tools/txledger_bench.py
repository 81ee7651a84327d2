#!/usr/bin/env python3
"""Measurement tool for the account store and the checks that name its accounts
by ID (sv_set_account_store, sv_ed25519_check_txbodies_ledger and _device); prints
one JSON line (the one committed as profiles/r16/txledger/bench.json).

The three workloads of tools/txaccounts_bench.py (single, multisig,
checkpoint), built by its functions.  Every account goes into the store once,
untimed; then, after one checked warm-up call per leg, medians with min - max of
`reps` rounds, the legs alternated inside each round:
  (a) ledger, device-resident         sv_ed25519_check_txbodies_ledger_device:
                                      no account table in the call, every bacct
                                      entry by ID (32 bytes per entry)
  (b) by-account, device-resident     sv_ed25519_check_txbodies_accounts_device
  (c) ledger from host buffers        sv_ed25519_check_txbodies_ledger: the IDs
                                      resolved on the host index, no account table
                                      uploaded, 4 bytes per entry in a chunk
  (d) by-account from host buffers    sv_ed25519_check_txbodies_accounts
and per workload: the bytes the caller hands over in both forms (the sum of its
array sizes), the lookup kernel's own time per call (sv_timing_enable;
sv_account_store_get_stats lookup_ms over the timed calls), the store's bytes on
the host and on the device, and the time of ONE sv_account_store_upsert of 1 %,
10 % and 100 % of the accounts (overwrites: host update, staging, upload,
scatter kernel and the wait, as the caller sees it).

  python tools/txledger_bench.py [--n N] [--m M] [--reps R] [--out FILE] [--root DIR]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = ("acct_key", "acct_thresholds", "asigner_begin", "asigner_type", "asigner_weight", "asigner_key",
         "asigner_payload", "apayload", "apayload_len")
USE = ("bodies", "off", "len", "kind", "sig_begin", "hint", "sig", "bacct_begin", "bacct", "check_begin", "check_acct",
       "check_level", "check_needed")


def run(sv, tb, dev, stream, s, reps):
    import torch
    nb, n, nc, na, ne = s["nb"], s["n"], s["nc"], s["na"], s["ne"]
    assert len(np.unique(s["acct_key"], axis=0)) == na, "the store holds one account per ID"
    assert int(np.diff(s["asigner_begin"].astype(np.int64)).max(initial=0)) <= 20
    # every account into the store, once, untimed
    sv.set_account_store(na, 0, 0)
    table = {k: s[k] for k in TABLE}
    sv.account_store_upsert(**table)
    s = dict(s, bacct_id=np.ascontiguousarray(s["acct_key"][s["bacct"]]),
             bacct_by_id=np.full(ne, 0xFFFFFFFF, np.uint32))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    t = {k: up(s[k] if s[k].size else np.zeros(16, np.uint8)) for k in TABLE + USE + ("bacct_id", "bacct_by_id")}
    p = lambda name: t[name].data_ptr()  # noqa: E731
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    t_ok = torch.zeros(nc, dtype=torch.uint8, device=dev)
    t_w = torch.zeros(nc, dtype=torch.int32, device=dev)
    t_u = torch.zeros(nc, dtype=torch.int64, device=dev)
    t_found = torch.zeros(ne, dtype=torch.uint8, device=dev)
    head = (0, tb.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"), n)
    tail = (p("check_begin"), p("check_acct"), p("check_level"), p("check_needed"), nc, t_ok.data_ptr(),
            t_w.data_ptr(), t_u.data_ptr())

    def account_device():
        sv.check_txbodies_accounts_device(*head, *(p(k) for k in TABLE), na, s["nas"], 0, p("bacct_begin"), p("bacct"),
                                          ne, *tail, d_digests=t_dig.data_ptr(), stream=stream)

    def ledger_device():
        sv.check_txbodies_ledger_device(*head, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, p("bacct_begin"), p("bacct_by_id"),
                                        ne, p("bacct_id"), t_found.data_ptr(), *tail, d_digests=t_dig.data_ptr(),
                                        stream=stream)

    out = {}
    host_head = (tb.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"])
    empty = (np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8),
             np.zeros(0, np.uint32), np.zeros((0, 32), np.uint8), None, None, None)

    def account_host():
        out["d"] = sv.check_txbodies_accounts(*host_head, *(s[k] for k in TABLE), s["bacct_begin"], s["bacct"],
                                              s["check_begin"], s["check_acct"], s["check_level"], s["check_needed"],
                                              device=0)

    def ledger_host():
        out["c"], out["found"] = sv.check_txbodies_ledger(*host_head, *empty, s["bacct_begin"], s["bacct_by_id"],
                                                          s["bacct_id"], s["check_begin"], s["check_acct"],
                                                          s["check_level"], s["check_needed"], device=0)

    def host_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def dev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def results_ok():
        torch.cuda.synchronize(dev)
        assert (t_ok.cpu().numpy() == s["want_ok"]).all()
        assert (t_w.cpu().numpy().view(np.uint32) == s["want_weight"]).all()
        assert (t_dig.cpu().numpy() == s["digests"]).all()
        t_ok.zero_()

    account_device()
    results_ok()
    ledger_device()
    results_ok()
    assert t_found.cpu().numpy().all()
    account_host()
    ledger_host()
    for i in range(3):
        assert (out["c"][i] == out["d"][i]).all()
    assert (out["c"][0] == s["want_ok"]).all() and (out["c"][3] == s["digests"]).all() and out["found"].all()
    legs = [("a_ledger_device_ms", ledger_device), ("b_account_device_ms", account_device)]
    host_legs = [("c_ledger_host_ms", ledger_host), ("d_account_host_ms", account_host)]
    ms = {k: [] for k, _ in legs + host_legs}
    sv.timing_enable(True)
    look0 = sv.account_store_stats(0)
    for rnd in range(reps):
        account_device()  # (one untimed call: the legs of the pair take turns at going first)
        torch.cuda.synchronize(dev)
        for name, fn in legs[::1 - 2 * (rnd & 1)]:
            ms[name].append(dev_ms(fn))
        for name, fn in host_legs[::1 - 2 * (rnd & 1)]:
            ms[name].append(host_ms(fn))
    look1 = sv.account_store_stats(0)
    sv.timing_enable(False)
    r = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    r.update({k.replace("_ms", "_min_max_ms"): [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()})
    size = lambda keys: int(sum(np.ascontiguousarray(s[k]).nbytes for k in keys))  # noqa: E731
    r.update(bodies=nb, signatures=n, checks=nc, accounts=na, account_signers=s["nas"], entries=ne,
             bytes_by_account=size(TABLE + USE), bytes_ledger=size(USE + ("bacct_id",)),
             a_over_b_pct=round(100.0 * (r["a_ledger_device_ms"] / r["b_account_device_ms"] - 1), 2),
             ranges_overlap=bool(min(ms["a_ledger_device_ms"]) <= max(ms["b_account_device_ms"])
                                 and min(ms["b_account_device_ms"]) <= max(ms["a_ledger_device_ms"])),
             c_over_d_pct=round(100.0 * (r["c_ledger_host_ms"] / r["d_account_host_ms"] - 1), 2),
             host_ranges_overlap=bool(min(ms["c_ledger_host_ms"]) <= max(ms["d_account_host_ms"])
                                      and min(ms["d_account_host_ms"]) <= max(ms["c_ledger_host_ms"])),
             lookup_kernel_ms_per_call=round((look1["lookup_ms"] - look0["lookup_ms"]) / reps, 4),
             store_host_bytes=look1["host_bytes"], store_device_bytes=look1["device_bytes"],
             max_probe=look1["max_probe"])
    # one upsert of 1 %, 10 % and 100 % of the accounts (overwrites with the same rows)
    gb = s["asigner_begin"].astype(np.int64)
    for pct in (1, 10, 100):
        k = max(1, na * pct // 100)
        part = dict(table, acct_key=s["acct_key"][:k], acct_thresholds=s["acct_thresholds"][:k],
                    asigner_begin=s["asigner_begin"][:k + 1], asigner_type=s["asigner_type"][:gb[k]],
                    asigner_weight=s["asigner_weight"][:gb[k]], asigner_key=s["asigner_key"][:gb[k]],
                    asigner_payload=s["asigner_payload"][:gb[k]])
        tms = []
        for _ in range(3):
            t0 = time.perf_counter()
            sv.account_store_upsert(**part)
            tms.append((time.perf_counter() - t0) * 1e3)
        r["upsert_%dpct_ms" % pct] = round(statistics.median(tms), 3)
        r["upsert_%dpct_min_max_ms" % pct] = [round(min(tms), 3), round(max(tms), 3)]
        r["upsert_%dpct_accounts" % pct] = k
    assert sv.account_store_stats(0)["replica_current"] == 1
    ledger_device()  # (the overwrites left every account as it was)
    results_ok()
    sv.set_account_store(0)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--root", default=REPO, help="the tree whose stellar-core_amd package is imported")
    ap.add_argument("--out", default="", help="where the JSON line is also written")
    a = ap.parse_args()
    for d in (os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
        sys.path.insert(0, d)
    import torch
    import txaccounts_bench as ab
    import txchecks_bench as cb
    import txpairs_bench as tb
    # --root goes in LAST: the helper modules above put this tree's root at the front of sys.path as they load
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sv = importlib.import_module("stellar-core_amd")
    assert os.path.dirname(os.path.dirname(os.path.abspath(sv.__file__))) == root, (sv.__file__, root)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(7, a.reps)
    res = {"tool": "tools/txledger_bench.py", "reps": reps, "n": a.n, "m": a.m,
           "kernel_source_digest": sv.kernel_source_digest(),
           "package": os.path.relpath(os.path.abspath(sv.__file__), REPO),
           "library": os.path.relpath(sv.LIB_PATH, REPO)}
    single = cb.add_checks(tb.build(sv, dev, stream, a.n, np.ones(a.n, np.int64), 20), np.ones(a.n, np.int64),
                           np.random.default_rng(23))
    res["single"] = run(sv, tb, dev, stream, ab.by_account_one_per_body(single), reps)
    del single
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 21, a.m)
    multi = cb.add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)
    res["multisig"] = run(sv, tb, dev, stream, ab.by_account_one_per_body(multi), reps)
    del multi
    res["checkpoint"] = run(sv, tb, dev, stream, ab.build_checkpoint(sv, tb, dev, stream, a.n, 16, 24), reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
