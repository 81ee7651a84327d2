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

--fed measures the cache's feed (sv_set_verdict_cache_feed) instead, the record
committed as profiles/r15/vcfeed/bench.json: on the multisig set and on a
config-3-sized set of 5000 bodies, decide_txbodies_device cold, warm and fed
(the pairs sent through keyed latency-lane batches of 8192 first), with each
call's hits; the keyed 1k lane batch's p50 with the feed off and on; a 2^18 keyed
bulk batch with the bit clear, cold and warm.  Medians and min-max over at least
7 interleaved rounds.  Ahead of all that every build runs the `feed_off` section,
in one order and state: cold / warm decide on both sets before the process's
first lane batch, then the keyed 1k p50, then the 2^18 keyed bulk batch.  --root
DIR measures another build's package (checked to be the one imported; the record
names it and says whether it has the feed): a build of the parent commit stops
after `feed_off`.  --parent FILE folds such a record in -- refused unless it says
feed_api false -- and says whether each of this build's feed_off medians lies
within the parent's own min-max.

  python tools/vcache_bench.py [--n N] [--m M] [--reps R] [--entries E] [--off-only] [--root DIR]
                               [--parent FILE] [--out FILE] [--fed]"""
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


def _med(v):
    return {"ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def prepare_fed(sv, ab, tb, dev, stream, s, reps, entries):
    """--fed, one set -> (off_phase, fed_phase, the set's pairs).  Both phases time decide_txbodies_device after a
    clear (cold) and after an identical call (warm), legs interleaved per round, with each call's hits.
    off_phase: the feed off -- what a build without the feed runs too (the parent's, --root), and it runs before
    any latency-lane batch of the process, so both builds measure it in the same state.
    fed_phase: SV_VC_FEED_LANE on, and a third leg: a clear, the set's pairs sent through keyed latency-lane
    batches of 8192, then the call (fed: the timed call includes the drain).  Its three legs all run within the
    lane's share window (bulk launches leave a workgroup slot per CU free for SV_LAT_SHARE_MS after a lane
    batch), so its cold is slower than off_phase's: compare fed with the cold and warm beside it."""
    import torch
    has_feed = hasattr(sv, "set_verdict_cache_feed")
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

    def decide():
        sv.decide_txbodies_device(0, tb.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"),
                                  p("hint"), p("sig"), n, p("key_begin"), p("key"), nk, p("check_begin"),
                                  p("check_needed"), nc, p("signer_begin"), p("signer_type"), p("signer_weight"),
                                  p("signer_key"), ng, res, d_digests=t_dig.data_ptr(), stream=stream)

    def timed():
        torch.cuda.synchronize(dev)
        h0 = sv.verdict_cache_stats(0)["hits"]
        t0 = time.perf_counter()
        decide()
        torch.cuda.synchronize(dev)
        ms = (time.perf_counter() - t0) * 1e3
        return ms, sv.verdict_cache_stats(0)["hits"] - h0

    # the pairs, as the engine enumerates them
    pb, ps, pk, pv, dig = sv.verify_txbodies_hinted(tb.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"],
                                                    s["sig_begin"], s["hint"], s["sig"], s["key_begin"], s["key"],
                                                    device=0)
    body = np.repeat(np.arange(nb), np.diff(pb.astype(np.int64)))
    f_pk = np.ascontiguousarray(s["key"].reshape(-1, 32)[pk])
    f_sig = np.ascontiguousarray(s["sig"].reshape(-1, 64)[ps])
    f_msg = np.ascontiguousarray(dig[body])
    pairs = len(pk)
    step = 8192
    offs, lens = (32 * np.arange(step)).astype(np.uint64), np.full(step, 32, np.uint32)
    journal = 1 << max(16, int(np.ceil(np.log2(max(pairs, 1)))))

    def feed():
        t0 = time.perf_counter()
        for a in range(0, pairs, step):
            b = min(pairs, a + step)
            v, _ = sv.verify_batch_keyed(f_pk[a:b], f_sig[a:b], f_msg[a:b].reshape(-1), offs[:b - a], lens[:b - a],
                                         device=0)
            assert (v == pv[a:b]).all()
        return (time.perf_counter() - t0) * 1e3

    def rounds(with_fed):
        sv.set_verdict_cache(entries)
        if has_feed:
            sv.set_verdict_cache_feed(1 if with_fed else 0, journal if with_fed else 0)
        decide()
        torch.cuda.synchronize(dev)
        ref = t_code.cpu().numpy().copy()
        legs = {k: [] for k in (("cold", "warm", "fed") if with_fed else ("cold", "warm"))}
        hits = {k: [] for k in legs}
        lane_ms = []
        for r in range(reps + 1):
            def leg(name):
                ms, h = timed()
                assert (t_code.cpu().numpy() == ref).all(), name
                if r:  # (round 0 warms everything up)
                    legs[name].append(ms)
                    hits[name].append(h)
            sv.verdict_cache_clear()
            leg("cold")
            decide()  # (a pair that lost its claim in the cold pass is stored now)
            leg("warm")
            if with_fed:
                sv.verdict_cache_clear()
                ms = feed()
                if r:
                    lane_ms.append(ms)
                leg("fed")
        out = {"bodies": nb, "signatures": n, "pairs": pairs, "journal_rows": journal if with_fed else 0}
        for k, v in legs.items():
            out[k] = dict(_med(v), hits=int(statistics.median(hits[k])))
        if with_fed:
            st = sv.verdict_cache_stats(0)
            out["fed_counters"] = {k: st[k] for k in ("fed_rows", "fed_overflow", "fed_present", "fed_inserted",
                                                       "fed_dropped")}
            out["lane_batches_ms"] = _med(lane_ms)
            out["fed_minus_warm_ms"] = round(out["fed"]["ms"] - out["warm"]["ms"], 4)
            sv.set_verdict_cache_feed(0)
        sv.set_verdict_cache(0)
        return out

    return (lambda: rounds(False)), (lambda: rounds(True)), (f_pk, f_sig, f_msg, pv)


def feed_off_host_legs(sv, pairs, reps, entries):
    """--fed, what both builds run with the cache on and the feed off, after the sets' off phases: the keyed 1k
    latency-lane batch's p50, then a 2^18 keyed bulk batch."""
    f_pk, f_sig, f_msg, pv = pairs
    k1 = (f_pk[:1000], f_sig[:1000], f_msg[:1000], pv[:1000])
    sv.set_verdict_cache(entries)
    if hasattr(sv, "set_verdict_cache_feed"):
        sv.set_verdict_cache_feed(0)
    lane = [lane_p50(sv, k1, 300) for _ in range(reps + 1)][1:]
    nbulk = min(len(f_pk), 1 << 18)
    offs, lens = (32 * np.arange(nbulk)).astype(np.uint64), np.full(nbulk, 32, np.uint32)
    flat = f_msg[:nbulk].reshape(-1)
    bulk = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        v, _ = sv.verify_batch_keyed(f_pk[:nbulk], f_sig[:nbulk], flat, offs, lens, device=0)
        bulk.append((time.perf_counter() - t0) * 1e3)
        assert (v == pv[:nbulk]).all()
    sv.set_verdict_cache(0)
    return {"lane_1k_p50": _med(lane), "bulk_2p18": _med(bulk[1:])}


def lane_p50(sv, rows, iters):
    """p50 of one keyed 1k latency-lane batch over `iters` calls, ms."""
    pk, sig, msg, want = rows
    offs, lens = (32 * np.arange(len(pk))).astype(np.uint64), np.full(len(pk), 32, np.uint32)
    flat = msg.reshape(-1)
    ts = []
    for i in range(iters + 30):
        t0 = time.perf_counter()
        v, _ = sv.verify_batch_keyed(pk, sig, flat, offs, lens, device=0)
        ts.append((time.perf_counter() - t0) * 1e3)
    assert (v == want).all()
    return statistics.median(ts[30:])


def run_lane_and_bulk(sv, pairs, reps, entries):
    """--fed, the host-buffer legs over the multisig set's pairs.  lane_1k: the keyed 1k batch's p50 with the cache
    on and the feed off, and with SV_VC_FEED_LANE on (interleaved).  bulk: a 2^18 keyed host batch with the cache on,
    the bit clear, and with SV_VC_FEED_BULK after a clear (cold) and again (warm)."""
    has_feed = hasattr(sv, "set_verdict_cache_feed")
    f_pk, f_sig, f_msg, pv = pairs
    k1 = (f_pk[:1000], f_sig[:1000], f_msg[:1000], pv[:1000])
    out = {}
    sv.set_verdict_cache(entries)
    off, on = [], []
    for r in range(reps + 1):
        if has_feed:
            sv.set_verdict_cache_feed(0)
        a = lane_p50(sv, k1, 300)
        if has_feed:
            sv.set_verdict_cache_feed(1, 1 << 22)  # (room for every row of the leg: each batch pays its copy)
            b = lane_p50(sv, k1, 300)
            sv.set_verdict_cache_feed(0)
        if r:
            off.append(a)
            if has_feed:
                on.append(b)
    out["lane_1k"] = {"feed_off_p50": _med(off)}
    if has_feed:
        out["lane_1k"]["feed_lane_p50"] = _med(on)
        lo, hi = out["lane_1k"]["feed_off_p50"]["min_max_ms"]
        out["lane_1k"]["on_median_within_off_min_max"] = bool(lo <= out["lane_1k"]["feed_lane_p50"]["ms"] <= hi)
    nbulk = min(len(f_pk), 1 << 18)
    offs, lens = (32 * np.arange(nbulk)).astype(np.uint64), np.full(nbulk, 32, np.uint32)
    flat = f_msg[:nbulk].reshape(-1)

    def bulk():
        t0 = time.perf_counter()
        v, _ = sv.verify_batch_keyed(f_pk[:nbulk], f_sig[:nbulk], flat, offs, lens, device=0)
        ms = (time.perf_counter() - t0) * 1e3
        assert (v == pv[:nbulk]).all()
        return ms

    legs = {"bit_clear": [], "cold": [], "warm": []} if has_feed else {"bit_clear": []}
    hits = []
    for r in range(reps + 1):
        if has_feed:
            sv.set_verdict_cache_feed(0)
        a = bulk()
        if r:
            legs["bit_clear"].append(a)
        if has_feed:
            sv.set_verdict_cache_feed(2)
            sv.verdict_cache_clear()
            c = bulk()
            h0 = sv.verdict_cache_stats(0)["hits"]
            w = bulk()
            if r:
                legs["cold"].append(c)
                legs["warm"].append(w)
                hits.append(sv.verdict_cache_stats(0)["hits"] - h0)
            sv.set_verdict_cache_feed(0)
    out["bulk"] = {"signatures": nbulk}
    for k, v in legs.items():
        out["bulk"][k] = _med(v)
    if has_feed:
        out["bulk"]["warm"]["hits"] = int(statistics.median(hits))
    sv.set_verdict_cache(0)
    return out


def main_fed(a, sv, ab, cb, tb, dev, stream, reps):
    import txset_gen as tg
    res = {"tool": "tools/vcache_bench.py --fed", "reps": reps, "entries": a.entries,
           "feed_api": hasattr(sv, "set_verdict_cache_feed"), "kernel_source_digest": sv.kernel_source_digest(),
           "package": os.path.relpath(os.path.realpath(os.path.dirname(sv.__file__)), REPO)}
    if a.parent:  # (before anything is measured: a record of a build that has the feed is no parent record)
        with open(a.parent) as fh:
            q = json.loads(fh.read())
        if q.get("feed_api") is not False or "feed_off" not in q or "multisig" in q:
            sys.exit("vcache_bench: %s is not a record of a build without the feed (feed_api %r)"
                     % (a.parent, q.get("feed_api")))
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 21, a.m)
    # the feed off, in the order and state every build runs it in: each set's tx-body calls right after the set is
    # built, before any lane batch of the process
    multisig = cb.add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)
    m_off, m_fed, pairs = prepare_fed(sv, ab, tb, dev, stream, multisig, reps, a.entries)
    res["feed_off"] = {"multisig": m_off()}
    # a config-3-sized set: 5000 bodies with the signature counts of 5000 tests/txset_gen.py transactions (that
    # generator makes contents hashes, not bodies, so its counts shape a set the tx-body call can hash itself)
    txs = tg.generate(5000, lambda reqs: [(bytes(32), bytes(64))] * len(reqs), seed=9000, extra_types=False)
    counts = np.array([max(1, len(tx["sigs"])) for tx in txs], np.int64)
    rng = np.random.default_rng(25)
    txset = cb.add_checks(tb.build(sv, dev, stream, 5000, counts, 26), rng.integers(1, 6, 5000), rng)
    t_off, t_fed, _ = prepare_fed(sv, ab, tb, dev, stream, txset, reps, a.entries)
    res["feed_off"]["txset_5000"] = t_off()
    res["feed_off"].update(feed_off_host_legs(sv, pairs, reps, a.entries))
    print("feed_off: %s" % json.dumps(res["feed_off"]), file=sys.stderr, flush=True)
    if res["feed_api"]:
        # (each set is uploaded again right before its rounds, as in its off phase)
        _, m_fed, pairs = prepare_fed(sv, ab, tb, dev, stream, multisig, reps, a.entries)
        res["multisig"] = m_fed()
        print("multisig: %s" % json.dumps(res["multisig"]), file=sys.stderr, flush=True)
        _, t_fed, _ = prepare_fed(sv, ab, tb, dev, stream, txset, reps, a.entries)
        res["txset_5000"] = t_fed()
        print("txset_5000: %s" % json.dumps(res["txset_5000"]), file=sys.stderr, flush=True)
        res.update(run_lane_and_bulk(sv, pairs, reps, a.entries))
        with open(os.path.join(REPO, "profiles", "r15", "vcfeed", "kernel_resources.csv")) as fh:
            res["kernel_resources"] = list(csv.DictReader(fh))
    if a.parent:
        within = lambda mine, theirs: bool(theirs["min_max_ms"][0] <= mine["ms"] <= theirs["min_max_ms"][1])  # noqa: E731
        res["parent"] = {"feed_api": q["feed_api"], "package": q.get("package"), "feed_off": q["feed_off"],
                         "this_median_within_parent_min_max": {}}
        w = res["parent"]["this_median_within_parent_min_max"]
        for name in ("multisig", "txset_5000"):
            for leg in ("cold", "warm"):
                w["%s_%s" % (name, leg)] = within(res["feed_off"][name][leg], q["feed_off"][name][leg])
        for leg in ("lane_1k_p50", "bulk_2p18"):
            w[leg] = within(res["feed_off"][leg], q["feed_off"][leg])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fed", action="store_true", help="the feed's record (profiles/r15/vcfeed/bench.json)")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--entries", type=int, default=1 << 23, help="verdict-cache entries of the cached legs")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--root", default=REPO, help="the tree whose stellar-core_amd package is imported")
    ap.add_argument("--parent", default="", help="an --off-only record of the parent commit, same session")
    ap.add_argument("--out", default="", help="where the JSON line is also written")
    a = ap.parse_args()
    for d in (os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
        sys.path.insert(0, d)
    import torch
    import txaccounts_bench as ab
    import txchecks_bench as cb
    import txpairs_bench as tb
    # --root goes in front last: the helper modules above put this tree in front of the path as they are imported.
    # The package that came in is checked to be the one asked for, and the record says which it was.
    root = os.path.realpath(a.root)
    sys.path.insert(0, root)
    sv = importlib.import_module("stellar-core_amd")
    if os.path.realpath(os.path.dirname(os.path.dirname(sv.__file__))) != root:
        sys.exit("vcache_bench: imported %s, not the package under --root %s" % (sv.__file__, root))
    if os.path.dirname(os.path.realpath(sv.LIB_PATH)) != os.path.join(root, "stellar-core_amd"):
        sys.exit("vcache_bench: the package loads %s, outside --root %s" % (sv.LIB_PATH, root))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(5, a.reps)
    if a.fed:
        res = main_fed(a, sv, ab, cb, tb, dev, stream, max(7, a.reps))
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
        return
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
