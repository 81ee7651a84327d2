#!/usr/bin/env python3
"""Measurement tool for the verdict cache (sv_set_verdict_cache); prints one
JSON line (the one committed as profiles/r14/vcache/bench.json).

Workload: sv_ed25519_decide_txbodies_device (explicit tables, no per-check
output, the bad list and its count) over the three sets of
tools/txresults_bench.py: 2^20 single-signature bodies, 2^16 multisig bodies and
the checkpoint set.  Per set, `reps` rounds, the legs interleaved inside each
round; a leg is one call from its enqueue to the end of its work on the caller's
stream, by the host's clock:
  off    capacity 0
  cold   cache on and cleared: every pair misses (the price of keys + probe +
         gather + insert)
  warm   the same set again: every retained pair hits
  half   every second body replaced by a fresh one (a byte that no earlier call
         used), the others cached
Afterwards two rounds with sv_timing_enable on give each leg's split: the verify
launches (sv_kernel_time), the cache's own kernels and the miss-count wait
(sv_verdict_cache_get_stats).  With --off-only only `off` runs and no cache
function is called (a build without the cache; --root names the tree whose
package is imported): the parent's figures for the first condition.

  python tools/vcache_bench.py [--n N] [--m M] [--reps R] [--entries E] [--off-only] [--root DIR]
                               [--parent FILE] [--out FILE]"""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(sv, ab, tb, dev, stream, s, reps, entries, off_only):
    import torch
    nb, n, nc, ng = s["nb"], s["n"], s["nc"], s["ng"]
    nk = int(s["key_begin"][-1])
    cb = s["check_begin"].astype(np.int64)
    s["check_role"] = (np.arange(nc) != np.repeat(cb[:-1], np.diff(cb))).astype(np.uint8)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    t = {k: up(s[k] if s[k].size else np.zeros(16, np.uint8)) for k in ab.EXPLICIT + ("check_role",)}
    p = lambda name: t[name].data_ptr()  # noqa: E731
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    t_code = torch.zeros(nb, dtype=torch.uint8, device=dev)
    t_fail = torch.zeros(nb, dtype=torch.int32, device=dev)
    t_bad = torch.zeros(nb, dtype=torch.int32, device=dev)
    t_nbad = torch.zeros(1, dtype=torch.int64, device=dev)
    res = sv.results_desc(check_role=p("check_role"), body_code=t_code.data_ptr(), body_fail=t_fail.data_ptr(),
                          bad_body=t_bad.data_ptr(), bad_cap=nb, n_bad=t_nbad.data_ptr())
    # the half leg's bodies: a copy in which the first byte of every second body changes before each call
    t_half = t["bodies"].clone()
    odd = torch.from_numpy(s["off"][1::2].astype(np.int64)).to(dev)
    assert (s["len"] > 0).all()
    fresh = [0]

    def decide(bodies):
        sv.decide_txbodies_device(0, tb.NETWORK_ID, bodies.data_ptr(), p("off"), p("len"), p("kind"), nb,
                                  p("sig_begin"), p("hint"), p("sig"), n, p("key_begin"), p("key"), nk,
                                  p("check_begin"), p("check_needed"), nc, p("signer_begin"), p("signer_type"),
                                  p("signer_weight"), p("signer_key"), ng, res, d_digests=t_dig.data_ptr(),
                                  stream=stream)

    def timed(bodies):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        decide(bodies)
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def next_half():
        fresh[0] += 1
        assert fresh[0] < 256, "the half leg has used every fresh byte"
        t_half[odd] = t["bodies"][odd] ^ fresh[0]

    def snapshot():
        st = sv.verdict_cache_stats(0)
        return dict(st, verify_ms=sv.kernel_time(0)[0])

    # the untimed warm-up, with its codes kept as the reference of every later call
    decide(t["bodies"])
    torch.cuda.synchronize(dev)
    ref = t_code.cpu().numpy().copy()
    n_bad = int(t_nbad.cpu().numpy()[0])
    assert n_bad == int((ref != 0).sum())
    legs = {"off": []} if off_only else {"off": [], "cold": [], "warm": [], "half": []}
    split = {}

    def one_round(record, timing):
        def leg(name, bodies, same=True):
            before = snapshot() if timing else None
            ms = timed(bodies)
            if same:
                assert (t_code.cpu().numpy() == ref).all() and int(t_nbad.cpu().numpy()[0]) == n_bad, name
            if timing:
                after = snapshot()
                d = {k: after[k] - before[k] for k in ("lookups", "hits", "inserted", "dropped", "kernel_ms",
                                                       "wait_ms", "verify_ms")}
                d["total_ms"] = ms
                split.setdefault(name, []).append(d)
            elif record:
                legs[name].append(ms)

        if off_only:
            leg("off", t["bodies"])
            return
        sv.set_verdict_cache(0)
        decide(t["bodies"])
        if timing:  # (with the cache off there is nothing to ask the stats for)
            torch.cuda.synchronize(dev)
            v0 = sv.kernel_time(0)[0]
            ms = timed(t["bodies"])
            split.setdefault("off", []).append({"total_ms": ms, "verify_ms": sv.kernel_time(0)[0] - v0})
        else:
            leg("off", t["bodies"])
        sv.set_verdict_cache(entries)
        decide(t["bodies"])  # (allocates the table and the workspace)
        sv.verdict_cache_clear()
        leg("cold", t["bodies"])
        decide(t["bodies"])  # (a pair that lost its claim in the cold pass is stored now)
        leg("warm", t["bodies"])
        next_half()
        leg("half", t_half, same=False)
        code = t_code.cpu().numpy()
        assert (code[0::2] == ref[0::2]).all() and (code[1::2] != 0).all()

    one_round(False, False)
    for _ in range(reps):
        one_round(True, False)
    r = {"bodies": nb, "signatures": n, "checks": nc, "failing_bodies": n_bad}
    for k, v in legs.items():
        r[k + "_ms"] = round(statistics.median(v), 4)
        r[k + "_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
    if not off_only:
        sv.timing_enable(True)
        try:
            for _ in range(2):
                one_round(False, True)
        finally:
            sv.timing_enable(False)
            sv.set_verdict_cache(0)
        r["split"] = {name: {k: round(statistics.median(d[k] for d in v), 4) for k in v[0]} for name, v in split.items()}
        spread = r["off_min_max_ms"][1] - r["off_min_max_ms"][0]
        r.update(cold_over_off=round(r["cold_ms"] / r["off_ms"], 4), warm_over_off=round(r["warm_ms"] / r["off_ms"], 4),
                 half_over_off=round(r["half_ms"] / r["off_ms"], 4), off_spread_ms=round(spread, 4),
                 warm_faster_than_off_by_more_than_spread=bool(r["off_ms"] - r["warm_ms"] > spread))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--entries", type=int, default=1 << 23, help="verdict-cache entries of the cached legs")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--root", default=REPO, help="the tree whose stellar-core_amd package is imported")
    ap.add_argument("--parent", default="", help="an --off-only record of the parent commit, same session")
    ap.add_argument("--out", default="", help="where the JSON line is also written")
    a = ap.parse_args()
    for d in (os.path.join(REPO, "tests"), os.path.join(REPO, "tools"), os.path.abspath(a.root)):
        sys.path.insert(0, d)
    import torch
    import txaccounts_bench as ab
    import txchecks_bench as cb
    import txpairs_bench as tb
    sv = importlib.import_module("stellar-core_amd")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(5, a.reps)
    res = {"tool": "tools/vcache_bench.py", "reps": reps, "off_only": bool(a.off_only), "entries": a.entries,
           "kernel_source_digest": sv.kernel_source_digest()}
    sets = {}
    sets["single"] = lambda: cb.add_checks(tb.build(sv, dev, stream, a.n, np.ones(a.n, np.int64), 20),
                                           np.ones(a.n, np.int64), np.random.default_rng(23))

    def multisig():
        rng = np.random.default_rng(21)
        counts = rng.integers(1, 21, a.m)
        return cb.add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)

    sets["multisig"] = multisig
    sets["checkpoint"] = lambda: ab.build_checkpoint(sv, tb, dev, stream, a.n, 16, 24)
    for name, build in sets.items():
        res[name] = run(sv, ab, tb, dev, stream, build(), reps, a.entries, a.off_only)
        print("%s: %s" % (name, json.dumps(res[name])), file=sys.stderr, flush=True)
    if not a.off_only:
        with open(os.path.join(REPO, "profiles", "r14", "vcache", "kernel_resources.csv")) as fh:
            res["kernel_resources"] = list(csv.DictReader(fh))
    if a.parent:
        with open(a.parent) as fh:
            parent = json.loads(fh.read())
        res["parent_off"] = {}
        for name in sets:
            q, r = parent[name], res[name]
            spread = q["off_min_max_ms"][1] - q["off_min_max_ms"][0]
            res["parent_off"][name] = {"off_ms": q["off_ms"], "off_min_max_ms": q["off_min_max_ms"],
                                       "spread_ms": round(spread, 4),
                                       "off_not_slower_than_parent_by_more_than_spread":
                                           bool(r["off_ms"] - q["off_ms"] <= spread)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
