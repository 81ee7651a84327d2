#!/usr/bin/env python3
"""Measurement tool for one signature result per transaction body
(sv_ed25519_decide_txbodies_accounts*); prints one JSON line (the one committed
as profiles/r12/txresults/bench.json).

The three workloads of tools/txaccounts_bench.py (single, multisig,
checkpoint), by account.  A body's first check has role TX, the others OP; no
body has SKIP_UNUSED.  Per workload, after one checked warm-up call per leg,
medians of `reps` rounds with the legs alternated inside each round:
  (a) decide, device-resident      sv_ed25519_decide_txbodies_accounts_device,
                                   no per-check output, the bad list and its count
  (b) check, device-resident       sv_ed25519_check_txbodies_accounts_device
  (c) the result kernels alone (sv_launch_txresult with the bad list) over (b)'s
      outputs, between two events on the caller's stream
  (d) decide from host buffers     sv_ed25519_decide_txbodies_accounts, body_code,
                                   body_fail and the bad list, nothing per check
  (e) check from host buffers      sv_ed25519_check_txbodies_accounts (the 13
                                   bytes per check; the caller's fold is NOT in it)
and once, on one generated envelope set (tests/envelope_bodies.py):
  the mirror: svh_check_envelopes_bodies with prefetch 6, 7 and 8.
With --existing-only only (b) and (e) run (a build without the decide entry
points; --root names the tree whose package is imported).

  python tools/txresults_bench.py [--n N] [--m M] [--reps R] [--units U] [--out FILE] [--existing-only]
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
NONE = 0xFFFFFFFF


def fold(cb, sb, ok, used, role):
    """The definition over arrays, vectorised (every body has a check; flags are 0) -> (code, fail)."""
    cb = cb.astype(np.int64)
    first = cb[:-1]
    assert (np.diff(cb) > 0).all()
    local = np.arange(len(ok), dtype=np.int64) - np.repeat(first, np.diff(cb))
    fail = np.minimum.reduceat(np.where(ok != 1, local, NONE), first)
    marks = np.bitwise_or.reduceat(used.astype(np.uint64), first)
    ns = np.minimum(np.diff(sb.astype(np.int64)), 64)
    want = np.where(ns >= 64, np.uint64(2**64 - 1), (np.uint64(1) << ns.astype(np.uint64)) - np.uint64(1))
    failed = fail != NONE
    frole = role[np.minimum(first + np.where(failed, fail, 0), len(ok) - 1)]
    code = np.where(failed, np.where(frole == 0, 1, 2), np.where((marks & want) != want, 3, 0)).astype(np.uint8)
    return code, fail.astype(np.uint32)


class TxResultIn(ctypes.Structure):  # csrc/txresult.h sv_txresult_in
    _fields_ = ([(f, ctypes.c_void_p) for f in ("check_begin", "sig_begin", "check_ok", "check_used", "check_role",
                                                "body_flags")]
                + [(f, ctypes.c_uint64) for f in ("nb", "nc", "ns")])


def run(sv, ab, tb, dev, stream, s, reps, existing_only):
    import torch
    nb, n, nc = s["nb"], s["n"], s["nc"]
    cb = s["check_begin"].astype(np.int64)
    s["check_role"] = (np.arange(nc) != np.repeat(cb[:-1], np.diff(cb))).astype(np.uint8)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    names = ab.BY_ACCOUNT + ("check_role",)
    t = {k: up(s[k] if s[k].size else np.zeros(16, np.uint8)) for k in names}
    p = lambda name: t[name].data_ptr()  # noqa: E731
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    t_ok = torch.zeros(nc, dtype=torch.uint8, device=dev)
    t_w = torch.zeros(nc, dtype=torch.int32, device=dev)
    t_u = torch.zeros(nc, dtype=torch.int64, device=dev)
    t_code = torch.zeros(nb, dtype=torch.uint8, device=dev)
    t_fail = torch.zeros(nb, dtype=torch.int32, device=dev)
    t_bad = torch.zeros(nb, dtype=torch.int32, device=dev)
    t_nbad = torch.zeros(1, dtype=torch.int64, device=dev)
    NID = tb.NETWORK_ID
    head = (0, NID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"), n,
            p("acct_key"), p("acct_thresholds"), p("asigner_begin"), p("asigner_type"), p("asigner_weight"),
            p("asigner_key"), p("asigner_payload"), p("apayload"), p("apayload_len"), s["na"], s["nas"], 0,
            p("bacct_begin"), p("bacct"), s["ne"], p("check_begin"), p("check_acct"), p("check_level"),
            p("check_needed"), nc)

    def check_device():
        sv.check_txbodies_accounts_device(*head, t_ok.data_ptr(), t_w.data_ptr(), t_u.data_ptr(),
                                          d_digests=t_dig.data_ptr(), stream=stream)

    out = {}
    host_head = (NID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"])

    def check_host():
        out["e"] = sv.check_txbodies_accounts(*host_head, *(s[k] for k in ab.BY_ACCOUNT[7:]), device=0)

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

    # the untimed warm-up call of every leg, with its results checked
    check_device()
    torch.cuda.synchronize(dev)
    ok, used = t_ok.cpu().numpy(), t_u.cpu().numpy().view(np.uint64)
    assert (ok == s["want_ok"]).all() and (t_dig.cpu().numpy() == s["digests"]).all()
    check_host()
    assert (out["e"][0] == ok).all() and (out["e"][2] == used).all()
    dev_legs = [("b_check_device_ms", check_device)]
    host_legs = [("e_check_host_ms", check_host)]
    legs = {}
    if not existing_only:
        lib = sv.load_library()
        code, fail = fold(s["check_begin"], s["sig_begin"], ok, used, s["check_role"])
        bad = np.flatnonzero(code != 0)
        res = sv.results_desc(check_role=p("check_role"), body_code=t_code.data_ptr(), body_fail=t_fail.data_ptr(),
                              bad_body=t_bad.data_ptr(), bad_cap=nb, n_bad=t_nbad.data_ptr())

        def decide_device():
            sv.decide_txbodies_accounts_device(*head, res, d_digests=t_dig.data_ptr(), stream=stream)

        def decide_host():
            out["d"] = sv.decide_txbodies_accounts(*host_head, *(s[k] for k in ab.BY_ACCOUNT[7:]),
                                                   check_role=s["check_role"], bad_cap=nb, device=0)

        lib.sv_launch_txresult.restype = ctypes.c_int
        lib.sv_launch_txresult.argtypes = [ctypes.POINTER(TxResultIn)] + [ctypes.c_void_p] * 4 + [
            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        t_ws = torch.zeros(lib.sv_txresult_ws_bytes(nb) + 64, dtype=torch.uint8, device=dev)
        I = TxResultIn(p("check_begin"), p("sig_begin"), t_ok.data_ptr(), t_u.data_ptr(), p("check_role"), None, nb,
                       nc, n)

        def kernels_alone():
            assert lib.sv_launch_txresult(ctypes.byref(I), t_code.data_ptr(), t_fail.data_ptr(), t_ws.data_ptr(),
                                          t_bad.data_ptr(), nb, t_nbad.data_ptr(), stream or None) == 0

        def device_results_ok():
            torch.cuda.synchronize(dev)
            assert (t_code.cpu().numpy() == code).all() and (t_fail.cpu().numpy().view(np.uint32) == fail).all()
            assert int(t_nbad.cpu().numpy()[0]) == len(bad)
            assert (t_bad.cpu().numpy()[:len(bad)] == bad).all()
            t_code.zero_()
            t_bad.zero_()

        decide_device()
        device_results_ok()
        kernels_alone()
        device_results_ok()
        decide_host()
        d = out["d"]
        assert (d.body_code == code).all() and (d.body_fail == fail).all() and d.n_bad == len(bad)
        assert (d.bad_body == bad).all() and (d.digests == s["digests"]).all()
        dev_legs.insert(0, ("a_decide_device_ms", decide_device))
        host_legs.insert(0, ("d_decide_host_ms", decide_host))
        legs["c_result_kernels_ms"] = []
    legs.update({k: [] for k, _ in dev_legs + host_legs})
    for rnd in range(reps):
        # (one untimed call after the host-bound legs, during which the GPU's clocks drop; the legs of a pair take
        # turns at going first)
        check_device()
        torch.cuda.synchronize(dev)
        for name, fn in dev_legs[::1 - 2 * (rnd & 1)]:
            legs[name].append(dev_ms(fn))
        if not existing_only:
            legs["c_result_kernels_ms"].append(dev_ms(kernels_alone))
        for name, fn in host_legs[::1 - 2 * (rnd & 1)]:
            legs[name].append(host_ms(fn))
    r = {k: round(statistics.median(v), 4) for k, v in legs.items()}
    r.update({k.replace("_ms", "_min_max_ms"): [round(min(v), 4), round(max(v), 4)] for k, v in legs.items()})
    r.update(bodies=nb, signatures=n, checks=nc, bytes_down_check=13 * nc + 32 * nb)
    if not existing_only:
        r.update(failing_bodies=int(len(bad)), bytes_down_decide=5 * nb + 32 * nb,
                 a_over_b_pct=round(100.0 * (r["a_decide_device_ms"] / r["b_check_device_ms"] - 1), 2),
                 d_over_e_pct=round(100.0 * (r["d_decide_host_ms"] / r["e_check_host_ms"] - 1), 2))
    return r


def mirror(sv, units, reps):
    """svh_check_envelopes_bodies on units x 6 generated envelopes (the signed-payload unit included), prefetch 6,
    7 and 8 alternated."""
    import envelope_bodies as eb
    import txbodies_pool as tp
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_decided_walks.restype = ctypes.c_uint64
    s = eb.build_set(units, 31, tp.device_signer(sv), with_payload=True)

    def call(prefetch):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch)

    ref = call(0)
    walks = host.svh_decided_walks()
    for p in (6, 7, 8):  # the untimed warm-up, with its results checked
        got = call(p)
        assert (got[0] == ref[0]).all() and (got[2] == ref[2]).all() and (got[3] == ref[3]).all()
    walks = int(host.svh_decided_walks() - walks)
    legs = {6: [], 7: [], 8: []}
    for rnd in range(reps):
        for p in ((6, 7, 8), (8, 7, 6), (7, 8, 6))[rnd % 3]:
            t0 = time.perf_counter()
            call(p)
            legs[p].append((time.perf_counter() - t0) * 1e3)
    r = {"prefetch%d_ms" % p: round(statistics.median(v), 4) for p, v in legs.items()}
    r.update({"prefetch%d_min_max_ms" % p: [round(min(v), 4), round(max(v), 4)] for p, v in legs.items()})
    r.update(envelopes=s["n"], failing_envelopes=int(((ref[0]["code"] != 0) & (ref[0]["code"] != 1)).sum()),
             prefetch8_walks=walks, p8_over_p7_pct=round(100.0 * (r["prefetch8_ms"] / r["prefetch7_ms"] - 1), 2),
             p8_over_p6_pct=round(100.0 * (r["prefetch8_ms"] / r["prefetch6_ms"] - 1), 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--units", type=int, default=4000, help="envelope units (6 envelopes each) of the mirror legs")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--root", default=REPO, help="the tree whose stellar-core_amd package is imported")
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
    res = {"tool": "tools/txresults_bench.py", "reps": reps, "existing_only": bool(a.existing_only),
           "kernel_source_digest": sv.kernel_source_digest()}
    single = cb.add_checks(tb.build(sv, dev, stream, a.n, np.ones(a.n, np.int64), 20), np.ones(a.n, np.int64),
                           np.random.default_rng(23))
    res["single"] = run(sv, ab, tb, dev, stream, ab.by_account_one_per_body(single), reps, a.existing_only)
    del single
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 21, a.m)
    multi = cb.add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)
    res["multisig"] = run(sv, ab, tb, dev, stream, ab.by_account_one_per_body(multi), reps, a.existing_only)
    del multi
    res["checkpoint"] = run(sv, ab, tb, dev, stream, ab.build_checkpoint(sv, tb, dev, stream, a.n, 16, 24), reps,
                            a.existing_only)
    if not a.existing_only:
        res["mirror"] = mirror(sv, a.units, reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
