#!/usr/bin/env python3
"""Measurement tool for signature checks decided on the device
(sv_ed25519_check_txbodies*); prints one JSON line (the one committed as
profiles/r09/txchecks/bench.json).

The two workloads of tools/txpairs_bench.py (same seeds, signatures made by
sv_ed25519_sign_device, one reject in sixteen) with check tables added:
  single    n single-signature V1 bodies (default 2^20): one LOW check plus one
            operation check per body, each over the body's one key
  multisig  m bodies (default 2^16) with 1..20 signatures and as many signers:
            a source check (needed 1) plus 1..5 operation checks whose
            thresholds need 1..k of the k signatures (weights 1)
Per workload, after one untimed warm-up call that also checks the results,
medians of `reps` rounds with the legs alternated inside each round:
  (a) the device-resident check call        sv_ed25519_check_txbodies_device
  (b) sv_ed25519_verify_txbodies_hinted_device on the same set
  (c) the check kernel alone: sv_launch_txcheck over (b)'s pairs, verdicts and
      digests, between two events on the caller's stream
  (d) the host-buffer check call against the host-buffer hinted call
and once, on one generated envelope set (tests/envelope_bodies.py):
  (e) the mirror: svh_check_envelopes_bodies with prefetch 5 against 3 and 1

  python tools/txchecks_bench.py [--n N] [--m M] [--reps R] [--units U] [--out FILE]"""
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
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402
import txpairs_bench as tb  # noqa: E402

NETWORK_ID = tb.NETWORK_ID


def add_checks(s, ops_per_body, rng):
    """Check tables over a txpairs_bench.build set (signature i <-> key i): per
    body a source check (needed 1) and ops_per_body[t] operation checks, all over
    the body's keys in order with weight 1; the operation checks need
    1..(signatures of the body).  Expected ok / weight by construction."""
    nb = s["nb"]
    k = np.diff(s["sig_begin"].astype(np.int64))
    per = 1 + np.asarray(ops_per_body, np.int64)
    cb = np.zeros(nb + 1, np.uint64)
    cb[1:] = np.cumsum(per)
    nc = int(cb[-1])
    body_of = np.repeat(np.arange(nb), per)
    first = np.zeros(nc, bool)
    first[cb[:-1].astype(np.int64)] = True
    need = np.where(first, 1, 1 + rng.integers(0, 1 << 30, nc) % k[body_of]).astype(np.int32)
    gcount = k[body_of]
    gb = np.zeros(nc + 1, np.uint64)
    gb[1:] = np.cumsum(gcount)
    ng = int(gb[-1])
    within = np.arange(ng) - np.repeat(gb[:-1].astype(np.int64), gcount)
    gk = (np.repeat(s["key_begin"][:-1].astype(np.int64)[body_of], gcount) + within).astype(np.uint32)
    valid = np.add.reduceat(s["want"].astype(np.int64), s["sig_begin"][:-1].astype(np.int64))
    have = valid[body_of]
    s.update(check_begin=cb, check_needed=need, signer_begin=gb, signer_type=np.zeros(ng, np.uint8),
             signer_weight=np.ones(ng, np.uint32), signer_key=gk, nc=nc, ng=ng,
             want_ok=(have >= need).astype(np.uint8), want_weight=np.minimum(have, need).astype(np.uint32))
    return s


def run(sv, dev, stream, s, reps):
    lib = sv.load_library()
    nb, n, nc, ng = s["nb"], s["n"], s["nc"], s["ng"]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    names = ("bodies", "off", "len", "kind", "sig_begin", "key_begin", "hint", "sig", "key", "check_begin",
             "check_needed", "signer_begin", "signer_type", "signer_weight", "signer_key")
    t = {k: up(s[k]) for k in names}
    p = lambda name: t[name].data_ptr()  # noqa: E731
    t_pb = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    t_ps = torch.zeros(n, dtype=torch.int32, device=dev)
    t_pk = torch.zeros(n, dtype=torch.int32, device=dev)
    t_v = torch.zeros(n, dtype=torch.uint8, device=dev)
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    t_ok = torch.zeros(nc, dtype=torch.uint8, device=dev)
    t_w = torch.zeros(nc, dtype=torch.int32, device=dev)
    t_u = torch.zeros(nc, dtype=torch.int64, device=dev)

    def check_device():
        sv.check_txbodies_device(0, NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"),
                                 p("hint"), p("sig"), n, p("key_begin"), p("key"), n, p("check_begin"),
                                 p("check_needed"), nc, p("signer_begin"), p("signer_type"), p("signer_weight"),
                                 p("signer_key"), ng, t_ok.data_ptr(), t_w.data_ptr(), t_u.data_ptr(),
                                 d_digests=t_dig.data_ptr(), stream=stream)

    def hinted_device():
        return sv.verify_txbodies_hinted_device(0, NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb,
                                                p("sig_begin"), p("hint"), p("sig"), n, p("key_begin"), p("key"), n, n,
                                                t_pb.data_ptr(), t_ps.data_ptr(), t_pk.data_ptr(), t_v.data_ptr(), 0,
                                                t_dig.data_ptr(), stream)

    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.sv_launch_txcheck.argtypes = ([vp, vp, vp, vp, u64, vp, vp, u64, u64, vp, vp, vp, vp, u64, vp, vp, vp, u64, vp,
                                       vp, vp, vp, u64, ctypes.c_int, vp, vp, vp, vp])

    def kernel_alone():  # (over the pair arrays the last hinted_device call left)
        rc = lib.sv_launch_txcheck(p("sig_begin"), p("hint"), p("sig"), None, n, p("key_begin"), p("key"), n, nb,
                                   t_pb.data_ptr(), t_ps.data_ptr(), t_pk.data_ptr(), t_v.data_ptr(), n,
                                   t_dig.data_ptr(), p("check_begin"), p("check_needed"), nc, p("signer_begin"),
                                   p("signer_type"), p("signer_weight"), p("signer_key"), ng, 1, t_ok.data_ptr(),
                                   t_w.data_ptr(), t_u.data_ptr(), stream or None)
        assert rc == 0, rc

    out = {}
    host_args = (NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"], s["sig"],
                 s["key_begin"], s["key"])

    def check_host():
        out["d"] = sv.check_txbodies(*host_args, s["check_begin"], s["check_needed"], s["signer_begin"],
                                     s["signer_type"], s["signer_weight"], s["signer_key"], device=0)

    def hinted_host():
        out["h"] = sv.verify_txbodies_hinted(*host_args, pair_cap=n, device=0)

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

    # the untimed warm-up call of every leg, with its results checked
    check_device()
    results_ok()
    assert (t_dig.cpu().numpy() == s["digests"]).all()
    assert hinted_device() == n
    t_ok.zero_()
    kernel_alone()
    results_ok()
    check_host()
    assert (out["d"][0] == s["want_ok"]).all() and (out["d"][1] == s["want_weight"]).all()
    assert (out["d"][3] == s["digests"]).all()
    hinted_host()
    legs = {k: [] for k in ("a_check_device_ms", "b_hinted_device_ms", "c_check_kernel_ms", "d_check_host_ms",
                            "d_hinted_host_ms")}
    for rnd in range(reps):
        # (one untimed call after the host-bound legs, during which the GPU's clocks drop; (a) and (b) take turns
        # at going first)
        hinted_device()
        torch.cuda.synchronize(dev)
        for name, fn in (("a_check_device_ms", check_device), ("b_hinted_device_ms", hinted_device))[::1 - 2 * (rnd & 1)]:
            legs[name].append(dev_ms(fn))
        hinted_device()
        legs["c_check_kernel_ms"].append(dev_ms(kernel_alone))
        for name, fn in (("d_check_host_ms", check_host), ("d_hinted_host_ms", hinted_host))[::1 - 2 * (rnd & 1)]:
            legs[name].append(host_ms(fn))
    r = {k: round(statistics.median(v), 4) for k, v in legs.items()}
    r.update(bodies=nb, signatures=n, keys=n, pairs=n, checks=nc, signers=ng,
             a_over_b_pct=round(100.0 * (r["a_check_device_ms"] / r["b_hinted_device_ms"] - 1), 2),
             d_check_over_hinted_pct=round(100.0 * (r["d_check_host_ms"] / r["d_hinted_host_ms"] - 1), 2),
             bytes_back_checks=13 * nc, bytes_back_pairs=9 * n + 8 * (nb + 1))
    return r


def mirror(sv, units, reps):
    """(e): svh_check_envelopes_bodies on units x 5 generated envelopes."""
    import envelope_bodies as eb
    import txbodies_pool as tp
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(units, 31, tp.device_signer(sv), with_payload=False)

    def call(prefetch):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch)

    ref = call(0)
    for p in (1, 3, 5):  # the untimed warm-up, with its results checked
        got = call(p)
        assert (got[0] == ref[0]).all() and (got[2] == ref[2]).all() and (got[3] == ref[3]).all()
    legs = {1: [], 3: [], 5: []}
    for rnd in range(reps):
        for p in ((1, 3, 5), (5, 3, 1), (3, 5, 1))[rnd % 3]:
            t0 = time.perf_counter()
            call(p)
            legs[p].append((time.perf_counter() - t0) * 1e3)
    r = {"e_prefetch%d_ms" % p: round(statistics.median(v), 4) for p, v in legs.items()}
    r.update(envelopes=s["n"], e_5_over_1_pct=round(100.0 * (r["e_prefetch5_ms"] / r["e_prefetch1_ms"] - 1), 2),
             e_5_over_3_pct=round(100.0 * (r["e_prefetch5_ms"] / r["e_prefetch3_ms"] - 1), 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--units", type=int, default=4000, help="envelope units (5 envelopes each) of the mirror leg")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r09", "txchecks", "bench.json"),
                    help="where the JSON line is also written ('' for nowhere)")
    a = ap.parse_args()
    sv = importlib.import_module("stellar-core_amd")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(5, a.reps)
    res = {"tool": "tools/txchecks_bench.py", "reps": reps, "kernel_source_digest": sv.kernel_source_digest()}
    single = add_checks(tb.build(sv, dev, stream, a.n, np.ones(a.n, np.int64), 20), np.ones(a.n, np.int64),
                        np.random.default_rng(23))
    res["single"] = run(sv, dev, stream, single, reps)
    del single
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 21, a.m)
    multi = add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)
    res["multisig"] = run(sv, dev, stream, multi, reps)
    del multi
    res["mirror"] = mirror(sv, a.units, reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
