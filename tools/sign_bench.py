#!/usr/bin/env python3
"""Measurement tool for the batch signer (sv_ed25519_sign_batch*); writes one
JSON record (the one committed as profiles/r17/sign/bench.json) and prints it.

7 rounds per leg, the legs alternated inside every round, after a warm-up
round; device-resident legs are timed with device events around the call and a
synchronise, the host-form leg with a host clock around the blocking call.

  (a) 2^20 distinct seeds, 32-byte messages, device-resident: the new
      sv_ed25519_sign_batch_device against the EXISTING sv_ed25519_sign_device
      in the same process, after asserting that their outputs are byte-equal.
      The claim to confirm: the new signer's max over the rounds lies below the
      existing signer's min (recorded as a_new_max_below_old_min).
  (b) 100 keys x 2^20 messages of 128..384 bytes, device-resident.
  (c) the reference's benchmark shape, 10 000 keys x 256-byte messages, through
      the host form, against libsodium's crypto_sign_detached where the box
      has a libsodium, else against sv_ed25519_sign_batch_cpu (c_baseline says
      which).

  python tools/sign_bench.py [--n N] [--rounds R] [--out PATH]"""
import argparse
import ctypes
import ctypes.util
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


def find_sodium():
    for cand in (ctypes.util.find_library("sodium"), "libsodium.so.23", "libsodium.so"):
        if not cand:
            continue
        try:
            lib = ctypes.CDLL(cand)
            if lib.sodium_init() >= 0:
                return lib
        except OSError:
            pass
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17", "sign", "bench.json"))
    a = ap.parse_args()
    n, rounds = a.n, a.rounds
    sv = importlib.import_module("stellar-core_amd")
    assert sv.device_count() >= 1, "no GPU: nothing is measured without one"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(17)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)  # noqa: E731

    # (a)
    t_seed = up(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    t_m32 = up(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    t_pk_new, t_pk_old = (torch.zeros((n, 32), dtype=torch.uint8, device=dev) for _ in range(2))
    t_sig_new, t_sig_old = (torch.zeros((n, 64), dtype=torch.uint8, device=dev) for _ in range(2))

    def a_new():
        sv.sign_batch_device(0, t_seed.data_ptr(), n, t_m32.data_ptr(), n, t_sig_new.data_ptr(),
                             d_pk=t_pk_new.data_ptr(), fixed_msg_len=32, stream=stream)

    def a_old():
        sv.sign_device(0, t_seed.data_ptr(), t_m32.data_ptr(), n, t_pk_old.data_ptr(), t_sig_old.data_ptr(), stream)

    # (b)
    kb = 100
    lens = rng.integers(128, 385, n).astype(np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    t_bmsg = up(rng.integers(0, 256, int(lens.sum(dtype=np.uint64)), dtype=np.uint8))
    t_boff, t_blen = up(off), up(lens)
    t_bkey = up(rng.integers(0, kb, n).astype(np.uint32))
    t_bseed = up(rng.integers(0, 256, (kb, 32), dtype=np.uint8))
    t_bsig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)

    def b_shared():
        sv.sign_batch_device(0, t_bseed.data_ptr(), kb, t_bmsg.data_ptr(), n, t_bsig.data_ptr(),
                             d_key_of=t_bkey.data_ptr(), fixed_msg_len=0, d_msg_off=t_boff.data_ptr(),
                             d_msg_len=t_blen.data_ptr(), stream=stream)

    # (c)
    kc = 10_000
    c_seed = rng.integers(0, 256, (kc, 32), dtype=np.uint8)
    c_msg = rng.integers(0, 256, (kc, 256), dtype=np.uint8)
    c_out = {}

    def c_host():
        c_out["sig"], c_out["pk"] = sv.sign_batch(c_seed, c_msg, fixed_msg_len=256, device=0)

    sodium = find_sodium()
    if sodium is not None:
        sks = []
        for i in range(kc):
            pk, sk = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
            sodium.crypto_sign_seed_keypair(pk, sk, c_seed[i].tobytes())
            sks.append(sk)
        msgs = [c_msg[i].tobytes() for i in range(kc)]
        sig_buf = ctypes.create_string_buffer(64)

        def c_base():
            for i in range(kc):
                sodium.crypto_sign_detached(sig_buf, None, msgs[i], ctypes.c_ulonglong(256), sks[i])
        c_label = "libsodium crypto_sign_detached, one thread, ctypes loop (keys expanded beforehand)"
    else:
        def c_base():
            c_out["base"] = sv.sign_batch_cpu(c_seed, c_msg, fixed_msg_len=256)[0]
        c_label = "sv_ed25519_sign_batch_cpu, default threads (no libsodium on this box)"

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

    legs = (("a_new_ms", a_new, dev_ms), ("a_old_ms", a_old, dev_ms), ("b_shared_ms", b_shared, dev_ms),
            ("c_host_ms", c_host, host_ms), ("c_baseline_ms", c_base, host_ms))
    for _, fn, _t in legs:  # warm-up: code objects, tables, buffers
        fn()
    torch.cuda.synchronize(dev)
    assert (t_pk_new.cpu().numpy() == t_pk_old.cpu().numpy()).all(), "leg (a): public keys differ"
    assert (t_sig_new.cpu().numpy() == t_sig_old.cpu().numpy()).all(), "leg (a): signatures differ"
    if "base" in c_out:
        assert (c_out["sig"] == c_out["base"]).all(), "leg (c): host and CPU forms differ"
    times = {name: [] for name, _, _ in legs}
    for _ in range(rounds):
        for name, fn, timer in legs:
            times[name].append(timer(fn))
    out = {"tool": "tools/sign_bench.py", "n": n, "rounds": rounds, "kernel_source_digest": sv.kernel_source_digest(),
           "device": torch.cuda.get_device_name(0), "b_keys": kb, "b_message_bytes": int(lens.sum(dtype=np.uint64)),
           "c_keys": kc, "c_msg_len": 256, "c_baseline": c_label, "a_outputs_byte_equal": True}
    for name, v in times.items():
        out[name] = {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4),
                     "all": [round(x, 4) for x in v]}
    out["a_new_max_below_old_min"] = bool(max(times["a_new_ms"]) < min(times["a_old_ms"]))
    out["a_old_over_new_median"] = round(statistics.median(times["a_old_ms"]) / statistics.median(times["a_new_ms"]), 3)
    out["a_new_sigs_per_s"] = round(n / (statistics.median(times["a_new_ms"]) * 1e-3))
    out["b_sigs_per_s"] = round(n / (statistics.median(times["b_shared_ms"]) * 1e-3))
    out["c_host_sigs_per_s"] = round(kc / (statistics.median(times["c_host_ms"]) * 1e-3))
    out["c_baseline_sigs_per_s"] = round(kc / (statistics.median(times["c_baseline_ms"]) * 1e-3))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
