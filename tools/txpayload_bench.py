#!/usr/bin/env python3
"""Measurement tool for the ED25519_SIGNED_PAYLOAD stage decided on the device
(sv_ed25519_check_txbodies_device with the payload tables); prints one JSON
line (the one committed as profiles/r10/txpayload/bench.json).

The multisig workload of tools/txchecks_bench.py (same seeds: m bodies, default
2^16, with 1..20 signatures and as many signers, a source check plus 1..5
operation checks), twice:
  plain     as it is: no payload candidate anywhere
  payload   one body in `--one-in` (default 64) has its first signer turned into
            a signed-payload signer: the candidate is (that key, the body's
            contents hash as a 32-byte payload), the signature keeps its bytes
            and gets the XORed hint, and every check of the body names the
            candidate first.  The decisions are the plain set's by construction.
After one untimed warm-up call of every leg that also checks the results,
medians of `reps` rounds with the legs alternated inside each round:
  plain     (p0) the device-resident call, tables absent
            (p1) the same with empty tables (pkey_begin of zeros, n_pkeys 0)
  payload   (a) the device-resident call with the tables
            (b) the same set with the tables absent, the check results copied to
                the host, plus the continuation the mirror runs today
                (DecidedChecker::check): for every check that came back 0 and has
                a payload signer, one sv_ed25519_verify_cpu call per (signature,
                signer) whose hint matches, serially, until the check succeeds.
                The loop is driven from Python over lists made outside the timer
                (about 1 us of call overhead against a verification)
            (c) the payload pairing kernels alone (count, scan, fill), between
                two events on the caller's stream

  python tools/txpayload_bench.py [--m M] [--one-in K] [--reps R] [--out FILE]"""
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
import txchecks_bench as cb  # noqa: E402
import txpairs_bench as tb  # noqa: E402

NETWORK_ID = tb.NETWORK_ID


def add_payload(s, one_in):
    """-> a copy of the add_checks set `s` with payload candidates in the bodies t % one_in == 0."""
    p = dict(s)
    nb = s["nb"]
    sb, kb = s["sig_begin"].astype(np.int64), s["key_begin"].astype(np.int64)
    T = np.arange(0, nb, one_in)
    si, ki = sb[T], kb[T]  # (signature i <-> key i: the body's first of each)
    dig = s["digests"][T]
    hint = s["hint"].copy()
    hint[si] = s["key"][ki][:, 28:] ^ dig[:, 28:]
    pay = np.zeros((len(T), 64), np.uint8)
    pay[:, :32] = dig
    qb = np.zeros(nb + 1, np.uint64)
    is_t = np.zeros(nb, bool)
    is_t[T] = True
    qb[1:] = np.cumsum(is_t)
    # every check's first signer names its body's first key: in the bodies of T it becomes the candidate
    g_first = s["signer_begin"][:-1].astype(np.int64)
    per = np.diff(s["check_begin"].astype(np.int64))
    body_of = np.repeat(np.arange(nb), per)
    g = g_first[is_t[body_of]]
    gt, gk = s["signer_type"].copy(), s["signer_key"].copy()
    gt[g] = 3
    gk[g] = (qb[:-1].astype(np.int64)[body_of])[is_t[body_of]]
    p.update(hint=hint, signer_type=gt, signer_key=gk, signer_key_skip=s["signer_key"], pkey_begin=qb,
             pkey=np.ascontiguousarray(s["key"][ki]), pkey_payload=pay, pkey_len=np.full(len(T), 32, np.uint8),
             nq=len(T), payload_bodies=T)
    return p


def run(sv, dev, stream, plain, pay, reps):
    lib = sv.load_library()
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    names = ("bodies", "off", "len", "kind", "sig_begin", "key_begin", "hint", "sig", "key", "check_begin",
             "check_needed", "signer_begin", "signer_type", "signer_weight", "signer_key")
    nb, n, nc, ng, nq = plain["nb"], plain["n"], plain["nc"], plain["ng"], pay["nq"]
    tp_ = {k: up(plain[k]) for k in names}
    ty = {k: up(pay[k]) for k in names + ("signer_key_skip", "pkey_begin", "pkey", "pkey_payload", "pkey_len")}
    t_zero = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    t_ok = torch.zeros(nc, dtype=torch.uint8, device=dev)
    t_w = torch.zeros(nc, dtype=torch.int32, device=dev)
    t_u = torch.zeros(nc, dtype=torch.int64, device=dev)

    def call(t, gk="signer_key", **kw):
        p = lambda name: t[name].data_ptr()  # noqa: E731
        sv.check_txbodies_device(0, NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"),
                                 p("hint"), p("sig"), n, p("key_begin"), p("key"), n, p("check_begin"),
                                 p("check_needed"), nc, p("signer_begin"), p("signer_type"), p("signer_weight"),
                                 p(gk), ng, t_ok.data_ptr(), t_w.data_ptr(), t_u.data_ptr(), stream=stream, **kw)

    p0 = lambda: call(tp_)  # noqa: E731
    p1 = lambda: call(tp_, d_pkey_begin=t_zero.data_ptr(), n_pkeys=0)  # noqa: E731
    a = lambda: call(ty, d_pkey_begin=ty["pkey_begin"].data_ptr(), d_pkey=ty["pkey"].data_ptr(),  # noqa: E731
                     d_pkey_payload=ty["pkey_payload"].data_ptr(), d_pkey_len=ty["pkey_len"].data_ptr(), n_pkeys=nq)
    b_device = lambda: call(ty, gk="signer_key_skip")  # noqa: E731

    # (b)'s continuation: per failed check with a payload signer, the (candidate, signature) pairs whose hint matches
    verify_cpu = lib.sv_ed25519_verify_cpu
    verify_cpu.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
    sb, cbeg = pay["sig_begin"].astype(np.int64), pay["check_begin"].astype(np.int64)
    gbeg = pay["signer_begin"].astype(np.int64)
    todo = {}
    for j, t in enumerate(pay["payload_bodies"]):
        key, msg = pay["pkey"][j].tobytes(), pay["pkey_payload"][j, :32].tobytes()
        want = (pay["pkey"][j, 28:] ^ pay["pkey_payload"][j, 28:32]).tobytes()
        sigs = [pay["sig"][i].tobytes() for i in range(sb[t], sb[t + 1]) if pay["hint"][i].tobytes() == want]
        for c in range(cbeg[t], cbeg[t + 1]):
            todo[c] = (key, msg, sigs, int(pay["check_needed"][c]), int(pay["signer_weight"][gbeg[c]]))
    cand = np.array(sorted(todo), np.int64)
    state = {}

    def b():
        b_device()
        ok = t_ok.cpu().numpy()  # (synchronises: the decisions are needed on the host)
        w = t_w.cpu().numpy()
        done = 0
        for c in cand[ok[cand] == 0]:
            key, msg, sigs, need, weight = todo[int(c)]
            for sg in sigs:
                if verify_cpu(key, sg, msg, 32) == 1:
                    ok[c] = int(w[c]) + weight >= need
                    break
            done += 1
        state["ok"], state["continued"] = ok, done

    # (c): the payload pairing kernels alone
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    for f in (lib.sv_pair_ws_bytes, lib.sv_ppair_ws_bytes):
        f.argtypes, f.restype = [u64], ctypes.c_size_t
    lib.sv_launch_ppair_count.argtypes = [vp, vp, u64, vp, vp, vp, vp, u64, u64, vp, vp, vp, vp]
    lib.sv_launch_ppair_fill.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, u64, u64, vp, vp, vp, u64] + [vp] * 8
    lib.sv_pair_total.argtypes, lib.sv_pair_total.restype = [vp, u64], vp
    ws = torch.zeros(lib.sv_pair_ws_bytes(nb) + 16, dtype=torch.uint8, device=dev)
    pws = torch.zeros(lib.sv_ppair_ws_bytes(nb) + 16, dtype=torch.uint8, device=dev)
    ppb = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    cap = 4 * nq + 16  # (a candidate pairs with its one signature, and with chance hint matches)
    g = {k: torch.zeros(cap * w, dtype=torch.uint8, device=dev) for k, w in
         (("ps", 4), ("pk", 4), ("key", 32), ("sig", 64), ("msg", 64), ("off", 8), ("len", 4))}
    y = lambda name: ty[name].data_ptr()  # noqa: E731

    def c_kernels():
        rc = lib.sv_launch_ppair_count(y("sig_begin"), y("hint"), n, y("pkey_begin"), y("pkey"), y("pkey_payload"),
                                       y("pkey_len"), nq, nb, ws.data_ptr(), pws.data_ptr(), ppb.data_ptr(),
                                       stream or None)
        assert rc == 0, rc
        rc = lib.sv_launch_ppair_fill(y("sig_begin"), y("hint"), y("sig"), n, y("pkey_begin"), y("pkey"),
                                      y("pkey_payload"), y("pkey_len"), nq, nb, ws.data_ptr(), pws.data_ptr(),
                                      ppb.data_ptr(), cap, g["ps"].data_ptr(), g["pk"].data_ptr(), g["key"].data_ptr(),
                                      g["sig"].data_ptr(), g["msg"].data_ptr(), g["off"].data_ptr(),
                                      g["len"].data_ptr(), stream or None)
        assert rc == 0, rc

    def dev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_ms(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def results_ok():
        torch.cuda.synchronize(dev)
        assert (t_ok.cpu().numpy() == plain["want_ok"]).all()
        assert (t_w.cpu().numpy().view(np.uint32) == plain["want_weight"]).all()

    # the untimed warm-up call of every leg, with its results checked
    outs = {}
    for name, fn in (("p0", p0), ("p1", p1), ("a", a)):
        t_ok.zero_()
        fn()
        results_ok()
        outs[name] = (t_ok.cpu().numpy().copy(), t_w.cpu().numpy().copy(), t_u.cpu().numpy().copy())
    assert all((x == z).all() for x, z in zip(outs["p0"], outs["p1"]))
    b()
    assert (state["ok"] == plain["want_ok"]).all()
    need_payload = int((t_ok.cpu().numpy() != plain["want_ok"]).sum())  # checks only the payload signer satisfies
    c_kernels()
    torch.cuda.synchronize(dev)
    npp = int(ppb.cpu().numpy()[-1])
    assert nq <= npp <= cap
    if npp == nq:  # (no chance hint match: pair j is candidate j with its body's first signature)
        assert (g["ps"].cpu().numpy().view(np.uint32)[:nq] == sb[pay["payload_bodies"]]).all()
        assert (g["pk"].cpu().numpy().view(np.uint32)[:nq] == np.arange(nq)).all()
    legs = {k: [] for k in ("p0_absent_ms", "p1_empty_ms", "a_tables_ms", "b_absent_plus_host_ms",
                            "b_device_part_ms", "c_pairing_kernels_ms")}
    for rnd in range(reps):
        p0()
        torch.cuda.synchronize(dev)
        for name, fn in (("p0_absent_ms", p0), ("p1_empty_ms", p1))[::1 - 2 * (rnd & 1)]:
            legs[name].append(dev_ms(fn))
        for name, fn in (("a_tables_ms", a), ("b_absent_plus_host_ms", b))[::1 - 2 * (rnd & 1)]:
            legs[name].append(host_ms(fn))
        legs["b_device_part_ms"].append(host_ms(b_device))
        legs["c_pairing_kernels_ms"].append(dev_ms(c_kernels))
    r = {k: round(statistics.median(v), 4) for k, v in legs.items()}
    r.update({k.replace("_ms", "_min_max"): [round(min(v), 4), round(max(v), 4)] for k, v in legs.items()})
    r.update(bodies=nb, signatures=n, checks=nc, signers=ng, payload_candidates=nq, payload_pairs=npp,
             checks_with_payload_signer=len(cand), checks_needing_payload_signer=need_payload,
             share_of_checks_needing_payload_signer=round(need_payload / nc, 5), continued_on_host=state["continued"],
             p1_over_p0_pct=round(100.0 * (r["p1_empty_ms"] / r["p0_absent_ms"] - 1), 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--one-in", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10", "txpayload", "bench.json"),
                    help="where the JSON line is also written ('' for nowhere)")
    a = ap.parse_args()
    sv = importlib.import_module("stellar-core_amd")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(5, a.reps)
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 21, a.m)
    plain = cb.add_checks(tb.build(sv, dev, stream, a.m, counts, 22), rng.integers(1, 6, a.m), rng)
    res = {"tool": "tools/txpayload_bench.py", "reps": reps, "one_in": a.one_in,
           "kernel_source_digest": sv.kernel_source_digest(),
           "multisig": run(sv, dev, stream, plain, add_payload(plain, a.one_in), reps)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
