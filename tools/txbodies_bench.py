#!/usr/bin/env python3
"""Measurement tool for the tx-body path (sv_ed25519_verify_txbodies*); prints
one JSON line (the one committed as profiles/r07/txbodies/bench.json).

Workload: n single-signature V1 bodies (default 2^20), lengths multiples of 4
drawn uniformly from 100..400 bytes from a fixed seed, signatures made by
sv_ed25519_sign_device over the hashlib digests.  After a warm-up, medians of
`reps` runs (device events for the device-resident calls, a host clock around
the blocking host-buffer calls) of
  (a) the fused device-resident call          sv_ed25519_verify_txbodies_device
  (b) sv_ed25519_verify_device alone on the precomputed digests
  (c) the fused host-buffer call              sv_ed25519_verify_txbodies
  (d) sv_ed25519_verify_batch_fixed on the precomputed digests
  (e) the hash stage alone (the fused call with no signatures) against
      sv_sha256_device on the pre-concatenated payloads, alternated in one run
  (f) hashlib SHA-256 of the payloads on one thread (interpreter loop
      included), and one sixteenth of it: the bound no 16-thread host hash beats

  python tools/txbodies_bench.py [--n N] [--reps R] [--warmup W]"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    n, reps = a.n, max(10, a.reps)
    sv = importlib.import_module("stellar-core_amd")
    lib = sv.load_library()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(20)
    length = (4 * rng.integers(25, 101, n)).astype(np.uint32)
    # bodies 16-byte aligned (the layout the engine's own staging uses)
    step = (length.astype(np.uint64) + np.uint64(15)) & ~np.uint64(15)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(step[:-1], dtype=np.uint64)
    blob = rng.integers(0, 256, int(off[-1] + step[-1]), dtype=np.uint8)
    prefix = NETWORK_ID + b"\0\0\0\2"
    payloads = [prefix + blob[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(off, length)]
    t0 = time.perf_counter()
    digs = [hashlib.sha256(p).digest() for p in payloads]
    hashlib_s = time.perf_counter() - t0
    digests = np.frombuffer(b"".join(digs), np.uint8).reshape(n, 32).copy()
    pay_len = (length + np.uint32(len(prefix))).astype(np.uint32)
    pay_off = np.zeros(n, np.uint64)
    pay_off[1:] = np.cumsum(pay_len[:-1], dtype=np.uint64)
    pay = np.frombuffer(b"".join(payloads), np.uint8).copy()
    del payloads, digs
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    t_seed, t_dig = up(rng.integers(0, 256, (n, 32), dtype=np.uint8)), up(digests)
    t_pk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    t_sig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    sv.sign_device(0, t_seed.data_ptr(), t_dig.data_ptr(), n, t_pk.data_ptr(), t_sig.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    pk, sig = t_pk.cpu().numpy(), t_sig.cpu().numpy()
    sig[::16, 40] ^= 0x08  # one reject in sixteen
    t_sig.copy_(torch.from_numpy(sig))
    want = np.ones(n, np.uint8)
    want[::16] = 0
    kind = np.zeros(n, np.uint8)
    sig_begin = np.arange(n + 1, dtype=np.uint64)
    t_blob, t_off, t_len, t_kind, t_sb = up(blob), up(off), up(length), up(kind), up(sig_begin)
    t_pay, t_poff, t_plen = up(pay), up(pay_off), up(pay_len)
    t_v = torch.zeros(n, dtype=torch.uint8, device=dev)
    t_out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    t_out2 = torch.zeros((n, 32), dtype=torch.uint8, device=dev)

    def fused_device(nsig):
        sv.verify_txbodies_device(0, NETWORK_ID, t_blob.data_ptr(), t_off.data_ptr(), t_len.data_ptr(),
                                  t_kind.data_ptr(), n, t_sb.data_ptr(), t_pk.data_ptr(), t_sig.data_ptr(), nsig,
                                  t_v.data_ptr(), 0, t_out.data_ptr(), stream)

    def verify_device():
        sv.verify_device(0, t_pk.data_ptr(), t_sig.data_ptr(), t_dig.data_ptr(), n, t_v.data_ptr(), stream=stream)

    def sha_device():
        sv._check(lib.sv_sha256_device(0, t_pay.data_ptr(), t_poff.data_ptr(), t_plen.data_ptr(), 0, n,
                                       t_out2.data_ptr(), stream))

    def dev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_ms(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    res = {}

    def measure(name, fn, timer, check=None):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize(dev)
        if check:
            check()
        res[name] = statistics.median(timer(fn) for _ in range(reps))

    def check_device():
        assert (t_v.cpu().numpy() == want).all(), "device verdicts"

    def check_fused():
        check_device()
        assert (t_out.cpu().numpy() == digests).all(), "fused digests"

    measure("a_fused_device_ms", lambda: fused_device(n), dev_ms, check_fused)
    t_v.zero_()
    measure("b_verify_device_ms", verify_device, dev_ms, check_device)
    host_out = {}

    def fused_host():
        host_out["v"], host_out["d"] = sv.verify_txbodies(NETWORK_ID, blob, off, length, kind, sig_begin, pk, sig,
                                                          device=0)

    def fixed_host():
        host_out["f"] = sv.verify_fixed(pk, sig, digests, 32, device=0)

    measure("c_fused_host_ms", fused_host, host_ms)
    assert (host_out["v"] == want).all() and (host_out["d"] == digests).all(), "host verdicts / digests"
    measure("d_verify_fixed_host_ms", fixed_host, host_ms)
    assert (host_out["f"] == want).all(), "fixed verdicts"
    # (e) the two device hashes, alternated
    for _ in range(a.warmup):
        fused_device(0)
        sha_device()
    torch.cuda.synchronize(dev)
    assert (t_out.cpu().numpy() == digests).all() and (t_out2.cpu().numpy() == digests).all(), "hash stage digests"
    tx, sh = [], []
    for _ in range(reps):
        tx.append(dev_ms(lambda: fused_device(0)))
        sh.append(dev_ms(sha_device))
    res["e_txhash_kernel_ms"] = statistics.median(tx)
    res["e_sha256_device_ms"] = statistics.median(sh)
    body_bytes = int(length.sum(dtype=np.uint64))
    out = {
        "tool": "tools/txbodies_bench.py", "n": n, "reps": reps, "warmup": a.warmup,
        "body_bytes": body_bytes, "payload_bytes": int(pay.size),
        "kernel_source_digest": sv.kernel_source_digest(),
        **{k: round(v, 4) for k, v in res.items()},
        "fused_over_verify_device_pct": round(100.0 * (res["a_fused_device_ms"] / res["b_verify_device_ms"] - 1), 2),
        "fused_over_fixed_host_pct": round(100.0 * (res["c_fused_host_ms"] / res["d_verify_fixed_host_ms"] - 1), 2),
        "txhash_over_sha256_device": round(res["e_txhash_kernel_ms"] / res["e_sha256_device_ms"], 4),
        # per host-buffer step: the fused call's image (pk, sig, the four index arrays, aligned bodies) against
        # the fixed call's (pk, sig, digests); both bring n verdict bytes back, the fused call the digests too
        "c_h2d_bytes": int(96 * n + 8 * n + 8 * (n + 1) + 4 * n + n + int(step.sum(dtype=np.uint64))),
        "c_d2h_bytes": int(n + 32 * n),
        "d_h2d_bytes": int(128 * n), "d_d2h_bytes": int(n),
        "f_hashlib_1thread_ms": round(hashlib_s * 1e3, 2),
        "f_hashlib_over_16_ms": round(hashlib_s * 1e3 / 16, 2),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
