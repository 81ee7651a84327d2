#!/usr/bin/env python3
"""Measurement tool for pairing by hint on the device
(sv_ed25519_verify_txbodies_hinted*); prints one JSON line (the one committed
as profiles/r08/txpairs/bench.json).

Two workloads from fixed seeds, signatures made by sv_ed25519_sign_device over
the hashlib digests, one reject in sixteen:
  single    n single-signature V1 bodies (default 2^20) of 100..400 bytes
            (multiples of 4), one candidate key each
  multisig  m bodies (default 2^16) with 1..20 signatures and as many signers
            each; every signature matches exactly its signer
Per workload, medians of `reps` rounds with the legs alternated inside each
round (device events for the device-resident calls, a host clock around the
blocking ones):
  (a) the hinted device-resident call      sv_ed25519_verify_txbodies_hinted_device
  (b) sv_ed25519_verify_txbodies_device on the same set, pairs enumerated beforehand
  (c) the hinted host-buffer call          sv_ed25519_verify_txbodies_hinted
  (d) the C++ mirror's host enumeration (SignatureBatchPrefetch::add per body)
      followed by sv_ed25519_verify_txbodies (runBodies); d2: the mirror's
      hinted form (addHinted + runBodiesHinted) on the same objects
  (e) the pairing stages alone: the hinted device call without a verdict array
      (hash + count + scan + count read-back + fill), the tx-hash kernel alone,
      and the hinted call with pair_cap 0 (hash + count + scan + read-back)

  python tools/txpairs_bench.py [--n N] [--m M] [--reps R] [--warmup W] [--out FILE]"""
import argparse
import ctypes
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

NETWORK_ID = hashlib.sha256(b"Public Global Stellar Network ; September 2015").digest()


def build(sv, dev, stream, nb, counts, seed):
    """nb V1 bodies with counts[t] signatures and as many keys: signature i is
    made by its own key i, so key_begin == sig_begin and the pairs are (i, i)."""
    rng = np.random.default_rng(seed)
    length = (4 * rng.integers(25, 101, nb)).astype(np.uint32)
    step = (length.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15)  # bodies 16-byte aligned
    off = np.zeros(nb, np.uint64)
    off[1:] = np.cumsum(step[:-1], dtype=np.uint64)
    blob = rng.integers(0, 256, int(off[-1] + step[-1]), dtype=np.uint8)
    prefix = NETWORK_ID + b"\0\0\0\2"
    digests = np.frombuffer(b"".join(hashlib.sha256(prefix + blob[int(o):int(o) + int(ln)].tobytes()).digest()
                                     for o, ln in zip(off, length)), np.uint8).reshape(nb, 32).copy()
    sig_begin = np.zeros(nb + 1, np.uint64)
    sig_begin[1:] = np.cumsum(counts, dtype=np.uint64)
    n = int(sig_begin[-1])
    owner = np.repeat(np.arange(nb), counts)
    t_seed = torch.from_numpy(rng.integers(0, 256, (n, 32), dtype=np.uint8)).to(dev)
    t_msg = torch.from_numpy(digests[owner]).to(dev)
    t_pk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    t_sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    sv.sign_device(0, t_seed.data_ptr(), t_msg.data_ptr(), n, t_pk.data_ptr(), t_sig.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    pk, sig = t_pk.cpu().numpy(), t_sig.cpu().numpy()
    sig[::16, 40] ^= 0x08  # one reject in sixteen
    want = np.ones(n, np.uint8)
    want[::16] = 0
    hint = np.ascontiguousarray(pk[:, 28:])  # (distinct within a body: the warm-up checks the pairs are (i, i))
    return dict(nb=nb, n=n, bodies=blob, off=off, len=length, kind=np.zeros(nb, np.uint8), sig_begin=sig_begin,
                key_begin=sig_begin.copy(), hint=hint, sig=sig, key=pk, digests=digests, want=want,
                step_bytes=int(step.sum(dtype=np.uint64)))


def run(sv, host, dev, stream, s, reps, warmup):
    lib = sv.load_library()
    nb, n = s["nb"], s["n"]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    t = {k: up(s[k]) for k in ("bodies", "off", "len", "kind", "sig_begin", "key_begin", "hint", "sig", "key")}
    t_pb = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    t_ps = torch.zeros(n, dtype=torch.int32, device=dev)
    t_pk = torch.zeros(n, dtype=torch.int32, device=dev)
    t_v = torch.zeros(n, dtype=torch.uint8, device=dev)
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    p = lambda name: t[name].data_ptr()  # noqa: E731

    def hinted_device(cap=n, verdict=True):
        return sv.verify_txbodies_hinted_device(0, NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb,
                                                p("sig_begin"), p("hint"), p("sig"), n, p("key_begin"), p("key"), n,
                                                cap, t_pb.data_ptr(), t_ps.data_ptr(), t_pk.data_ptr(),
                                                t_v.data_ptr() if verdict else 0, 0, t_dig.data_ptr(), stream)

    def count_only():
        try:
            hinted_device(cap=0)
        except sv.SigVerifyError as e:
            assert e.needed == n

    def plain_device(nsig=n):
        # the pairs enumerated beforehand: here row i of (key, sig) is pair i
        sv.verify_txbodies_device(0, NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"),
                                  p("key"), p("sig"), nsig, t_v.data_ptr(), 0, t_dig.data_ptr(), stream)

    out = {}

    def hinted_host():
        out["c"] = sv.verify_txbodies_hinted(NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"],
                                             s["hint"], s["sig"], s["key_begin"], s["key"], pair_cap=n, device=0)

    vp = ctypes.c_void_p
    a = lambda x: vp(x.ctypes.data)  # noqa: E731
    nid = np.frombuffer(NETWORK_ID, np.uint8).copy()

    def mirror(hinted):
        ms = (ctypes.c_double * 2)()
        pairs, acc = ctypes.c_uint64(), ctypes.c_uint64()
        rc = host.svh_bench_prefetch_bodies(a(nid), a(s["bodies"]), a(s["off"]), a(s["len"]), a(s["kind"]),
                                            ctypes.c_size_t(nb), a(s["sig_begin"]), a(s["hint"]), a(s["sig"]),
                                            a(s["key_begin"]), a(s["key"]), hinted, ms, ctypes.byref(pairs),
                                            ctypes.byref(acc))
        assert rc == 0 and pairs.value == n and acc.value == int(s["want"].sum()), (rc, pairs.value, acc.value)
        return ms[0], ms[1]

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

    # warm-up and checks
    for _ in range(warmup):
        assert hinted_device() == n
        torch.cuda.synchronize(dev)
        assert (t_v.cpu().numpy() == s["want"]).all() and (t_dig.cpu().numpy() == s["digests"]).all()
        assert (t_ps.cpu().numpy() == np.arange(n)).all() and (t_pk.cpu().numpy() == np.arange(n)).all()
        assert (t_pb.cpu().numpy() == s["sig_begin"].astype(np.int64)).all()
        t_v.zero_()
        plain_device()
        torch.cuda.synchronize(dev)
        assert (t_v.cpu().numpy() == s["want"]).all()
        hinted_host()
        pb, ps, pk, pv, dig = out["c"]
        assert (pv == s["want"]).all() and (ps == np.arange(n)).all() and (pk == np.arange(n)).all()
        assert (pb == s["sig_begin"]).all() and (dig == s["digests"]).all()
        mirror(0)
        mirror(1)
        hinted_device(verdict=False)
        count_only()
        plain_device(0)
    torch.cuda.synchronize(dev)
    legs = {k: [] for k in ("a_hinted_device_ms", "b_txbodies_device_ms", "c_hinted_host_ms", "d_mirror_enum_ms",
                            "d_mirror_run_ms", "d_mirror_total_ms", "d2_mirror_hinted_add_ms",
                            "d2_mirror_hinted_run_ms", "d2_mirror_hinted_total_ms", "e_pairing_stages_ms",
                            "e_txhash_only_ms", "e_hash_count_scan_ms")}
    for rnd in range(reps):  # the legs alternated inside every round
        # (a) and (b) follow the host-bound legs of the round before, during which the GPU idles and its clocks
        # drop: the first verify after them ran 0.5-0.8 ms slower in a kernel trace, whichever leg it was.  So
        # one untimed call first, and the two legs take turns at going first.
        plain_device()
        torch.cuda.synchronize(dev)
        for name, fn in (("a_hinted_device_ms", hinted_device), ("b_txbodies_device_ms", plain_device))[::1 - 2 * (rnd & 1)]:
            legs[name].append(dev_ms(fn))
        legs["c_hinted_host_ms"].append(host_ms(hinted_host))
        add, runms = mirror(0)
        legs["d_mirror_enum_ms"].append(add)
        legs["d_mirror_run_ms"].append(runms)
        legs["d_mirror_total_ms"].append(add + runms)
        add, runms = mirror(1)
        legs["d2_mirror_hinted_add_ms"].append(add)
        legs["d2_mirror_hinted_run_ms"].append(runms)
        legs["d2_mirror_hinted_total_ms"].append(add + runms)
        legs["e_pairing_stages_ms"].append(dev_ms(lambda: hinted_device(verdict=False)))
        legs["e_txhash_only_ms"].append(dev_ms(lambda: plain_device(0)))
        legs["e_hash_count_scan_ms"].append(dev_ms(count_only))
    r = {k: round(statistics.median(v), 4) for k, v in legs.items()}
    # where (a) - (b) goes: the verify launch alone inside each call, from the engine's own event brackets
    # (sv_timing_enable), alternated; outside the timed legs above, which run without the brackets
    sv.timing_enable(True)
    inner = {"a_verify_launch_ms": [], "b_verify_launch_ms": []}
    for _ in range(reps):
        for name, fn in (("a_verify_launch_ms", hinted_device), ("b_verify_launch_ms", plain_device)):
            sv.kernel_time_reset()
            fn()
            torch.cuda.synchronize(dev)
            inner[name].append(sv.kernel_time(0)[0])
    sv.timing_enable(False)
    r.update({k: round(statistics.median(v), 4) for k, v in inner.items()})
    r.update(bodies=nb, signatures=n, keys=n, pairs=n, body_bytes=int(s["len"].sum(dtype=np.uint64)),
             a_over_b_pct=round(100.0 * (r["a_hinted_device_ms"] / r["b_txbodies_device_ms"] - 1), 2),
             c_over_d_pct=round(100.0 * (r["c_hinted_host_ms"] / r["d_mirror_total_ms"] - 1), 2),
             e_count_scan_ms=round(r["e_hash_count_scan_ms"] - r["e_txhash_only_ms"], 4),
             e_fill_ms=round(r["e_pairing_stages_ms"] - r["e_hash_count_scan_ms"], 4),
             # bytes the pairing stages move: CSR words + hint + key tail in; indices, gathered rows, pair_begin out
             pairing_in_bytes=int(16 * (nb + 1) + 4 * n + 4 * n + 96 * n + 32 * nb),
             pairing_out_bytes=int(136 * n + 8 * (nb + 1) + 8 * nb))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=1 << 16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r08", "txpairs", "bench.json"),
                    help="where the JSON line is also written ('' for nowhere)")
    a = ap.parse_args()
    sv = importlib.import_module("stellar-core_amd")
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    reps = max(10, a.reps)
    res = {"tool": "tools/txpairs_bench.py", "reps": reps, "warmup": a.warmup,
           "kernel_source_digest": sv.kernel_source_digest()}
    single = build(sv, dev, stream, a.n, np.ones(a.n, np.int64), 20)
    res["single"] = run(sv, host, dev, stream, single, reps, max(1, a.warmup))
    del single
    rng = np.random.default_rng(21)
    multi = build(sv, dev, stream, a.m, rng.integers(1, 21, a.m), 22)
    res["multisig"] = run(sv, host, dev, stream, multi, reps, max(1, a.warmup))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
