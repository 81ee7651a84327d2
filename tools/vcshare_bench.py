#!/usr/bin/env python3
"""Measurement tool for sv_set_verdict_cache_share; prints one JSON line (the
record committed as profiles/r19/vcshare/bench.json).  Run with
SV_DEVICE_MAP=0,0: two slots on ONE card, which shows the mechanism and its
cost, not the gain of a real multi-GPU node.

The set is tools/vcache_bench.py's multisig set: `m` (2^16) bodies with 1..20
signatures, 2..6 checks a body.  Medians of `reps` rounds with min - max.

  leg1   share off against the parent commit.  --parent-root DIR names a tree
         holding a build of the parent commit; its package is loaded INTO THIS
         PROCESS beside this tree's (two libraries, two engines, one card) and
         the two builds alternate round by round, which build goes first
         alternating too: sv_ed25519_decide_txbodies_device on slot 0 after a
         clear (cold) and again (warm), and the p50 of a keyed 1k latency-lane
         batch.  The record says whether each median of this tree lies inside
         the parent build's own min - max.
  leg2   host-buffer sv_ed25519_decide_txbodies over both slots (device -1): the
         set, then the set ROTATED BY HALF, so the slices trade slots; the
         second call timed with share off and with SV_VC_SHARE_STORES, with its
         hits summed over the slots; the same for an unrotated second call (the
         ceiling).  Journal rows sized to the set.  The rotated call's codes are
         checked to be the first call's, rotated.
  leg3   what it costs: the first (cold) call of leg2 with the bit set against
         clear; two more rounds under sv_timing_enable give, per slot, the time of
         the cache's own kernels in the first call (the export kernel on top of
         probe and insert) and in the second (the larger drain); and the keyed 1k
         lane p50 with SV_VC_FEED_LANE alone and with SV_VC_SHARE_FEED, at this
         process's slot count (--lane-only: nothing else, for a G = 8 run).

  python tools/vcshare_bench.py [--m M] [--reps R] [--entries E] [--parent-root DIR] [--out FILE]
                                [--legs 1,2,3] [--lane-only]"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _med(v):
    return {"ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}


def load_package(root, name):
    """The stellar-core_amd package under `root` as module `name` (its library is the one beside it)."""
    path = os.path.join(os.path.realpath(root), "stellar-core_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    assert os.path.dirname(os.path.realpath(m.LIB_PATH)) == os.path.dirname(path)
    return m


def _csr(begin, perm):
    """begin: a CSR row-begin array over parents; perm: new parent -> old parent.  -> (the new begin array, for every
    new child row the old child row)."""
    b = begin.astype(np.int64)
    cnt = np.diff(b)[perm]
    nb = np.zeros(len(perm) + 1, np.int64)
    nb[1:] = np.cumsum(cnt)
    idx = np.repeat(b[:-1][perm] - nb[:-1], cnt) + np.arange(nb[-1])
    return nb.astype(begin.dtype), idx


def rotate(s, h):
    """The set with its bodies rotated by h: new body t is old body (t + h) mod nb, with everything that hangs on it."""
    nb = s["nb"]
    perm = np.concatenate([np.arange(h, nb), np.arange(0, h)])
    inv = np.empty(nb, np.int64)
    inv[perm] = np.arange(nb)
    rows = lambda x, n: np.ascontiguousarray(x).reshape(n, -1)  # noqa: E731
    r = dict(s)
    total, cut = len(s["bodies"]), int(s["off"][h])
    r["bodies"] = np.concatenate([s["bodies"][cut:], s["bodies"][:cut]])
    r["off"] = ((s["off"].astype(np.int64) - cut) % total).astype(s["off"].dtype)[perm]
    r["len"], r["kind"] = s["len"][perm], s["kind"][perm]
    r["sig_begin"], si = _csr(s["sig_begin"], perm)
    r["hint"], r["sig"] = rows(s["hint"], s["n"])[si], rows(s["sig"], s["n"])[si]
    nk = int(s["key_begin"][-1])
    r["key_begin"], ki = _csr(s["key_begin"], perm)
    r["key"] = rows(s["key"], nk)[ki]
    r["check_begin"], ci = _csr(s["check_begin"], perm)
    r["check_needed"], r["check_role"] = s["check_needed"][ci], s["check_role"][ci]
    r["signer_begin"], gi = _csr(s["signer_begin"], ci)
    r["signer_type"], r["signer_weight"] = s["signer_type"][gi], s["signer_weight"][gi]
    # a signer names its key by index: the index moves with its body's keys
    body_of_check = np.repeat(np.arange(nb), np.diff(s["check_begin"].astype(np.int64)))
    owner = np.repeat(body_of_check[ci], np.diff(r["signer_begin"].astype(np.int64)))
    kb_old, kb_new = s["key_begin"].astype(np.int64), r["key_begin"].astype(np.int64)
    r["signer_key"] = (s["signer_key"][gi].astype(np.int64) - kb_old[owner] + kb_new[inv[owner]]).astype(
        s["signer_key"].dtype)
    return r, perm


def lane_p50(sv, rows, iters=300):
    pk, sig, msg, want = rows
    offs, lens = (32 * np.arange(len(pk))).astype(np.uint64), np.full(len(pk), 32, np.uint32)
    flat = msg.reshape(-1)
    ts = []
    for _ in range(iters + 30):
        t0 = time.perf_counter()
        v, _k = sv.verify_batch_keyed(pk, sig, flat, offs, lens, device=0)
        ts.append((time.perf_counter() - t0) * 1e3)
    assert (v == want).all()
    return statistics.median(ts[30:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--entries", type=int, default=1 << 22)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--legs", default="1,2,3")
    ap.add_argument("--lane-only", action="store_true")
    a = ap.parse_args()
    legs = set() if a.lane_only else set(a.legs.split(","))
    for d in (os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
        sys.path.insert(0, d)
    import torch
    import txaccounts_bench as ab
    import txchecks_bench as cb
    import txpairs_bench as tb
    sv = load_package(REPO, "sv_this")
    parent = load_package(a.parent_root, "sv_parent") if a.parent_root and "1" in legs else None
    if parent is not None:
        assert not hasattr(parent, "set_verdict_cache_share"), "--parent-root holds a build with the setter"
    slots = sv.device_count()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = a.reps
    r = {"tool": "tools/vcshare_bench.py", "slots": slots, "reps": reps, "entries": a.entries,
         "note": "slots share ONE card: the mechanism and its cost, not the gain of a multi-GPU node"}

    rng = np.random.default_rng(21)
    m = 2048 if a.lane_only else a.m
    counts = rng.integers(1, 21, m)
    s = cb.add_checks(tb.build(sv, dev, stream, m, counts, 22), rng.integers(1, 6, m), rng)
    nb, n, nc, ng = s["nb"], s["n"], s["nc"], s["ng"]
    cbeg = s["check_begin"].astype(np.int64)
    s["check_role"] = (np.arange(nc) != np.repeat(cbeg[:-1], np.diff(cbeg))).astype(np.uint8)
    pb, ps, pk, pv, dig = sv.verify_txbodies_hinted(tb.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"],
                                                    s["sig_begin"], s["hint"], s["sig"], s["key_begin"], s["key"],
                                                    device=0)
    body = np.repeat(np.arange(nb), np.diff(pb.astype(np.int64)))
    k1 = tuple(np.ascontiguousarray(x[:1000]) for x in (s["key"].reshape(-1, 32)[pk], s["sig"].reshape(-1, 64)[ps],
                                                        dig[body], pv))
    pairs = len(pk)
    r.update(bodies=nb, signatures=n, pairs=pairs)

    # ------------------------------------------------------------ leg 1
    if "1" in legs:
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
        t = {k: up(s[k] if s[k].size else np.zeros(16, np.uint8)) for k in ab.EXPLICIT + ("check_role",)}
        p = lambda name: t[name].data_ptr()  # noqa: E731
        nk = int(s["key_begin"][-1])
        t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
        t_code = torch.zeros(nb, dtype=torch.uint8, device=dev)
        t_fail = torch.zeros(nb, dtype=torch.int32, device=dev)
        t_bad = torch.zeros(nb, dtype=torch.int32, device=dev)
        t_nbad = torch.zeros(1, dtype=torch.int64, device=dev)
        builds = {"this": sv}
        if parent is not None:
            builds["parent"] = parent
        res = {name: B.results_desc(check_role=p("check_role"), body_code=t_code.data_ptr(),
                                    body_fail=t_fail.data_ptr(), bad_body=t_bad.data_ptr(), bad_cap=nb,
                                    n_bad=t_nbad.data_ptr()) for name, B in builds.items()}

        def decide(name):
            builds[name].decide_txbodies_device(
                0, tb.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"),
                n, p("key_begin"), p("key"), nk, p("check_begin"), p("check_needed"), nc, p("signer_begin"),
                p("signer_type"), p("signer_weight"), p("signer_key"), ng, res[name], d_digests=t_dig.data_ptr(),
                stream=stream)

        def timed(name):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            decide(name)
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e3

        ref = None
        for name, B in builds.items():
            B.set_verdict_cache(a.entries)
            decide(name)
            torch.cuda.synchronize(dev)
            code = t_code.cpu().numpy().copy()
            assert ref is None or (code == ref).all(), "the two builds disagree"
            ref = code
        got = {name: {"cold": [], "warm": [], "lane_1k_p50": []} for name in builds}
        order = list(builds)
        for rnd in range(reps + 1):
            for name in (order if rnd % 2 == 0 else order[::-1]):
                B = builds[name]
                B.verdict_cache_clear()
                c = timed(name)
                assert (t_code.cpu().numpy() == ref).all(), name
                decide(name)  # (a pair that lost its claim in the cold pass is stored now)
                w = timed(name)
                assert (t_code.cpu().numpy() == ref).all(), name
                if rnd:
                    got[name]["cold"].append(c)
                    got[name]["warm"].append(w)
            for name in (order if rnd % 2 == 0 else order[::-1]):
                lp = lane_p50(builds[name], k1)
                if rnd:
                    got[name]["lane_1k_p50"].append(lp)
        for B in builds.values():
            B.set_verdict_cache(0)
        r["leg1"] = {name: {k: _med(v) for k, v in g.items()} for name, g in got.items()}
        r["leg1"]["interleaved_in_one_process"] = parent is not None
        if parent is not None:
            r["leg1"]["this_median_within_parent_min_max"] = {
                k: bool(r["leg1"]["parent"][k]["min_max_ms"][0] <= r["leg1"]["this"][k]["ms"]
                        <= r["leg1"]["parent"][k]["min_max_ms"][1]) for k in ("cold", "warm", "lane_1k_p50")}
        del t
        print("leg1: %s" % json.dumps(r["leg1"]), file=sys.stderr, flush=True)

    # ------------------------------------------------------------ legs 2 and 3
    if legs & {"2", "3"} and slots >= 2:
        s2, perm = rotate(s, nb // 2)
        journal = 1 << max(16, int(np.ceil(np.log2(pairs))))

        def host(x):
            return sv.decide_txbodies(tb.NETWORK_ID, x["bodies"], x["off"], x["len"], x["kind"], x["sig_begin"],
                                      x["hint"], x["sig"], x["key_begin"], x["key"], x["check_begin"],
                                      x["check_needed"], x["signer_begin"], x["signer_type"], x["signer_weight"],
                                      x["signer_key"], check_role=x["check_role"], bad_cap=nb)

        def timed_host(x, want):
            t0 = time.perf_counter()
            out = host(x)
            ms = (time.perf_counter() - t0) * 1e3
            assert (out.body_code == want).all()
            return ms

        stat = lambda f: [sv.verdict_cache_stats(b)[f] for b in range(2)]  # noqa: E731
        sv.set_verdict_cache(a.entries)
        sv.set_verdict_cache_feed(0, journal)
        ref1 = host(s).body_code.copy()
        ref2 = host(s2).body_code.copy()
        assert (ref2 == ref1[perm]).all(), "the rotated set's codes are not the set's, rotated"
        for b in range(2):
            assert sv.verdict_cache_stats(b)["lookups"] > 0, "slot %d got no slice" % b
        settings = (("off", 0), ("stores", sv.VC_SHARE_STORES))
        got = {name: {k: [] for k in ("first", "rotated", "rotated_hits", "unrotated", "unrotated_hits")}
               for name, _ in settings}
        split = {name: [] for name, _ in settings}

        def one(name, share, record, timing):
            sv.set_verdict_cache_share(share)
            sv.verdict_cache_clear()
            k0 = stat("kernel_ms")
            first = timed_host(s, ref1)
            k1_ = stat("kernel_ms")
            h0 = sum(stat("hits"))
            rot = timed_host(s2, ref2)
            h1 = sum(stat("hits"))
            k2 = stat("kernel_ms")
            sv.verdict_cache_clear()
            timed_host(s, ref1)
            h2 = sum(stat("hits"))
            unrot = timed_host(s, ref1)
            h3 = sum(stat("hits"))
            if timing:
                split[name].append({"first_ms": first, "rotated_ms": rot,
                                    "first_cache_kernels_ms": [round(k1_[b] - k0[b], 4) for b in range(2)],
                                    "rotated_cache_kernels_ms": [round(k2[b] - k1_[b], 4) for b in range(2)]})
            elif record:
                for k, v in (("first", first), ("rotated", rot), ("rotated_hits", h1 - h0), ("unrotated", unrot),
                             ("unrotated_hits", h3 - h2)):
                    got[name][k].append(v)

        for rnd in range(reps + 1):
            for name, share in (settings if rnd % 2 == 0 else settings[::-1]):
                one(name, share, rnd > 0, False)
        sv.timing_enable(True)
        try:
            for _ in range(2):
                for name, share in settings:
                    one(name, share, False, True)
        finally:
            sv.timing_enable(False)
        st = [sv.verdict_cache_stats(b) for b in range(2)]
        leg2 = {"journal_rows": journal}
        for name, g in got.items():
            leg2[name] = {"rotated": dict(_med(g["rotated"]), hits=int(statistics.median(g["rotated_hits"]))),
                          "unrotated": dict(_med(g["unrotated"]), hits=int(statistics.median(g["unrotated_hits"])))}
        leg2["rotated_shared_over_unshared"] = round(leg2["stores"]["rotated"]["ms"] / leg2["off"]["rotated"]["ms"], 4)
        leg2["shared_median_below_unshared_min"] = bool(leg2["stores"]["rotated"]["ms"]
                                                        < leg2["off"]["rotated"]["min_max_ms"][0])
        leg2["counters_at_the_end"] = [{k: st[b][k] for k in ("shared_out", "shared_in", "shared_skipped",
                                                              "shared_pinned_bytes", "fed_overflow", "fed_dropped",
                                                              "dropped")} for b in range(2)]
        r["leg2"] = leg2
        r["leg3"] = {"first_call": {name: _med(g["first"]) for name, g in got.items()},
                     "first_call_stores_minus_off_ms": round(statistics.median(got["stores"]["first"])
                                                             - statistics.median(got["off"]["first"]), 4),
                     "timing_rounds": {name: v for name, v in split.items()}}
        sv.set_verdict_cache_share(0)
        sv.set_verdict_cache_feed(0)
        print("leg2: %s\nleg3: %s" % (json.dumps(r["leg2"]), json.dumps(r["leg3"])), file=sys.stderr, flush=True)

    # ------------------------------------------------------------ the lane with SHARE_FEED
    if "3" in legs or a.lane_only:
        sv.set_verdict_cache(a.entries)
        lanes = {"off": [], "feed": [], "feed_share": []}
        for rnd in range(reps + 1):
            for name, src, share in (("off", 0, 0), ("feed", sv.VC_FEED_LANE, 0),
                                     ("feed_share", sv.VC_FEED_LANE, sv.VC_SHARE_FEED)):
                sv.set_verdict_cache_feed(src, 1 << 22 if src else 0)  # (room for every row: each batch pays its copies)
                sv.set_verdict_cache_share(share)
                lp = lane_p50(sv, k1)
                if rnd:
                    lanes[name].append(lp)
        r.setdefault("leg3", {})["lane_1k_p50"] = dict({name: _med(v) for name, v in lanes.items()}, slots=slots)
        sv.set_verdict_cache_share(0)
        sv.set_verdict_cache_feed(0)
    sv.set_verdict_cache(0)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
