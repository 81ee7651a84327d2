"""Multi-chunk host signing calls, run as a program by
test_gpu_sign.py::test_multi_chunk_host_call with SV_STAGE_CHUNK=1024 in the
environment (the engine reads the staging chunk once per process): 2500
variable-length messages in three pieces, with key_of == NULL (k == n, so each
piece's records start at its first row) and with three shared keys, then 2500
transaction bodies' digests in three pieces through sv_ed25519_sign_txbodies.
The host forms must equal the CPU forms.  Prints "sign multichunk ok"."""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime per process)

import txbodies_pool as tp  # noqa: E402


def main():
    assert os.environ.get("SV_STAGE_CHUNK") == "1024"
    sv = importlib.import_module("stellar-core_amd")
    n = 2500
    rng = np.random.default_rng(2500)
    lens = rng.integers(0, 150, n).astype(np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    msg = rng.integers(0, 256, int(lens.sum()) + 1, dtype=np.uint8)
    for k in (n, 3):
        seeds = rng.integers(0, 256, (k, 32), dtype=np.uint8)
        key_of = None if k == n else rng.integers(0, k, n).astype(np.uint32)
        sig, pk = sv.sign_batch(seeds, msg, off, lens, key_of=key_of, device=0)
        want, want_pk = sv.sign_batch_cpu(seeds, msg, off, lens, key_of=key_of)
        assert (pk == want_pk).all() and (sig == want).all(), k
    fixed = rng.integers(0, 256, (n, 48), dtype=np.uint8)
    sig, _ = sv.sign_batch(seeds, fixed, key_of=key_of, fixed_msg_len=48, device=0)
    want, _ = sv.sign_batch_cpu(seeds, fixed, key_of=key_of, fixed_msg_len=48)
    assert (sig == want).all()
    # bodies: one signature each, every third body none, lengths around the 16-byte packing
    blen = rng.integers(0, 120, n).astype(np.uint32)
    boff = np.zeros(n, np.uint64)
    boff[1:] = np.cumsum(blen[:-1], dtype=np.uint64)
    bodies = rng.integers(0, 256, int(blen.sum()) + 1, dtype=np.uint8)
    kind = (np.arange(n) % 3).astype(np.uint8)
    counts = (np.arange(n) % 3 != 1).astype(np.uint64)
    sig_begin = np.zeros(n + 1, np.uint64)
    sig_begin[1:] = np.cumsum(counts)
    ns = int(sig_begin[-1])
    tx_key = rng.integers(0, 3, ns).astype(np.uint32)
    got = sv.sign_txbodies(tp.NETWORK_ID, bodies, boff, blen, kind, sig_begin, seeds, tx_key, device=0)
    want = sv.sign_txbodies_cpu(tp.NETWORK_ID, bodies, boff, blen, kind, sig_begin, seeds, tx_key)
    for a, b in zip(got, want):
        assert (a == b).all()
    print("sign multichunk ok")


if __name__ == "__main__":
    main()
