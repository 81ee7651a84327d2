#!/usr/bin/env python3
"""Measurement tool for the verdict audit (sv_set_audit); prints one JSON line
(the one committed as profiles/r18/audit/bench.json).

Workloads, both device-resident and timed with device events around the call
on the caller's stream:
  verify   sv_ed25519_verify_device over --n GPU-signed rows (32-byte messages,
           one in 64 corrupted), the bulk route
  decide   sv_ed25519_decide_txbodies_device over the multisig set of
           tools/vcache_bench.py (--m bodies, explicit tables)
Legs, alternated inside each of `reps` (at least 7) rounds:
  off            the audit off
  rejects        SV_AUDIT_REJECTS (select / scan / fill over every row, the
                 textbook kernel over the rejects alone)
  sample_1024 / sample_64 / sample_1   SV_AUDIT_SAMPLE at that one_in, the
                 budget at its maximum so that one_in = 1 audits every row
Each leg: median and min-max in ms, and its ratio to the same build's `off`.
With --off-only only `off` runs and no audit function is called (a build of
the parent commit; --root names the tree whose package is imported).
--parent FILE folds such a record in and says, per workload, whether this
build's `off` median lies within the parent's own min-max.

  python tools/audit_bench.py [--n N] [--m M] [--reps R] [--off-only] [--root DIR] [--parent FILE] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = (("off", 0, 0), ("rejects", 1, 0), ("sample_1024", 2, 1024), ("sample_64", 2, 64), ("sample_1", 2, 1))


def measure(sv, torch, dev, call, check, reps, off_only):
    legs = [LEGS[0]] if off_only else list(LEGS)
    ms = {name: [] for name, _, _ in legs}
    audited = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 1):  # (round 0 warms every leg up: buffers grow there)
        for name, what, one_in in (legs if r % 2 == 0 else legs[::-1]):
            if not off_only:
                sv.set_audit(what, one_in=one_in, seed=r, budget=sv.AUDIT_BUDGET_MAX if what else 0)
                before = sv.audit_stats(0)["audited"] if what else 0
            torch.cuda.synchronize(dev)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize(dev)
            check()
            if what:
                st = sv.audit_stats(0)
                assert st["mismatches"] == 0, st
                audited[name] = st["audited"] - before
            if r:
                ms[name].append(e0.elapsed_time(e1))
    if not off_only:
        sv.set_audit(0)
    out = {}
    for name, v in ms.items():
        out[name] = {"ms": round(statistics.median(v), 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)]}
        if name != "off":
            out[name]["ratio_to_off"] = round(statistics.median(v) / statistics.median(ms["off"]), 4)
            out[name]["audited_rows"] = audited[name]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=7)
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
    root = os.path.realpath(a.root)
    sys.path.insert(0, root)
    sv = importlib.import_module("stellar-core_amd")
    if os.path.realpath(os.path.dirname(os.path.dirname(sv.__file__))) != root:
        sys.exit("audit_bench: imported %s, not the package under --root %s" % (sv.__file__, root))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(7, a.reps)
    res = {"tool": "tools/audit_bench.py", "reps": reps, "off_only": bool(a.off_only), "root": root,
           "audit_api": hasattr(sv, "set_audit"), "kernel_source_digest": sv.kernel_source_digest()}

    # verify: n GPU-signed rows
    n = a.n
    rng = np.random.default_rng(18)
    ts = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    tm = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    tpk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    tsig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    tv = torch.zeros(n, dtype=torch.uint8, device=dev)
    sv.sign_device(0, ts.data_ptr(), tm.data_ptr(), n, tpk.data_ptr(), tsig.data_ptr(), stream)
    tsig[1::64, 40] ^= 1
    torch.cuda.synchronize(dev)
    want = np.ones(n, np.uint8)
    want[1::64] = 0

    def verify():
        sv.verify_device(0, tpk.data_ptr(), tsig.data_ptr(), tm.data_ptr(), n, tv.data_ptr(), stream=stream)

    def verify_check():
        assert (tv.cpu().numpy() == want).all()

    prev = sv.set_kernel_path(sv.PATH_THROUGHPUT)
    res["verify"] = dict(measure(sv, torch, dev, verify, verify_check, reps, a.off_only), rows=n)
    print("verify: %s" % json.dumps(res["verify"]), file=sys.stderr, flush=True)

    # decide: the multisig set
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 21, a.m)
    s = cb.add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)
    nb, ns, nc, ng = s["nb"], s["n"], s["nc"], s["ng"]
    nk = int(s["key_begin"][-1])
    cbeg = s["check_begin"].astype(np.int64)
    s["check_role"] = (np.arange(nc) != np.repeat(cbeg[:-1], np.diff(cbeg))).astype(np.uint8)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    t = {k: up(s[k] if s[k].size else np.zeros(16, np.uint8)) for k in ab.EXPLICIT + ("check_role",)}
    p = lambda name: t[name].data_ptr()  # noqa: E731
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    t_code = torch.zeros(nb, dtype=torch.uint8, device=dev)
    t_fail = torch.zeros(nb, dtype=torch.int32, device=dev)
    t_bad = torch.zeros(nb, dtype=torch.int32, device=dev)
    t_nbad = torch.zeros(1, dtype=torch.int64, device=dev)
    r = sv.results_desc(check_role=p("check_role"), body_code=t_code.data_ptr(), body_fail=t_fail.data_ptr(),
                        bad_body=t_bad.data_ptr(), bad_cap=nb, n_bad=t_nbad.data_ptr())

    def decide():
        sv.decide_txbodies_device(0, tb.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"),
                                  p("hint"), p("sig"), ns, p("key_begin"), p("key"), nk, p("check_begin"),
                                  p("check_needed"), nc, p("signer_begin"), p("signer_type"), p("signer_weight"),
                                  p("signer_key"), ng, r, d_digests=t_dig.data_ptr(), stream=stream)

    decide()
    torch.cuda.synchronize(dev)
    ref = t_code.cpu().numpy().copy()

    def decide_check():
        assert (t_code.cpu().numpy() == ref).all()

    res["decide"] = dict(measure(sv, torch, dev, decide, decide_check, reps, a.off_only), bodies=nb, signatures=ns)
    print("decide: %s" % json.dumps(res["decide"]), file=sys.stderr, flush=True)
    sv.set_kernel_path(prev)
    if a.parent:
        with open(a.parent) as fh:
            q = json.loads(fh.read())
        res["parent_off"] = {}
        for w in ("verify", "decide"):
            lo, hi = q[w]["off"]["min_max_ms"]
            res["parent_off"][w] = {"off": q[w]["off"], "this_off_median_within_parent_min_max":
                                    bool(lo <= res[w]["off"]["ms"] <= hi)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
