"""Input pool of the tx-body tests (test_txbodies_cpu.py, test_gpu_txbodies.py).

make_set(nb, ...) builds nb transaction bodies and their signatures in the
layout of sv_ed25519_verify_txbodies, drawing from one pool:
  * prefix + body lengths that hit 55, 56, 63, 0 and 1 mod 64, for each kind;
  * body lengths 0, 1, 3, 4, 28 for each kind, one 65 KiB body, the rest
    100..4096 bytes;
  * bodies packed back to back, so every byte alignment occurs;
  * 0, 1 and 20 signatures per body;
  * rejects: a body mutated by one bit after signing, corrupted signature
    bytes, a signature made over the neighbouring body.
Expected digests are hashlib.sha256(prefix + body), expected verdicts the
oracle's over (pk, sig, digest); every set holds an accept and a reject.
"""
import hashlib

import numpy as np

NETWORK_ID = hashlib.sha256(b"Test SDF Network ; September 2015").digest()
V1, V0, FEE_BUMP = 0, 1, 2


def prefix(kind, network_id=NETWORK_ID):
    return network_id + {V1: b"\0\0\0\2", V0: b"\0\0\0\2\0\0\0\0", FEE_BUMP: b"\0\0\0\5"}[kind]


def contents_hash(kind, body, network_id=NETWORK_ID):
    return hashlib.sha256(prefix(kind, network_id) + bytes(body)).digest()


def pool_shapes(nb, rng, big=True):
    """nb (kind, length) pairs: the mandatory shapes first, then random ones."""
    shapes = []
    for kind in (V1, V0, FEE_BUMP):
        for k, r in enumerate((55, 56, 63, 0, 1)):
            shapes.append((kind, (r - len(prefix(kind))) % 64 + 64 * (k % 3)))
    for kind in (V1, V0, FEE_BUMP):
        shapes += [(kind, ln) for ln in (0, 1, 3, 4, 28)]
    if big:
        shapes.append((V1, 65 * 1024))
    while len(shapes) < nb:
        shapes.append((int(rng.integers(0, 3)), int(rng.integers(100, 4097))))
    return shapes[:nb]


def sigs_per_body(t):
    return 20 if t % 25 == 0 else (0 if t % 7 == 3 else 1)


def pysign_signer(oracle):
    """signer(seeds n x 32, msgs n x 32) -> (pk, sig) with the plain-Python
    signer, every signature checked by the oracle."""
    import ed25519_pysign as ps
    keys = {}

    def signer(seeds, msgs):
        pk = np.zeros((len(seeds), 32), np.uint8)
        sig = np.zeros((len(seeds), 64), np.uint8)
        for i in range(len(seeds)):
            s = seeds[i].tobytes()
            if s not in keys:
                keys[s] = ps.keypair(s)
            pk[i] = np.frombuffer(keys[s][2], np.uint8)
            sig[i] = np.frombuffer(ps.sign_checked(oracle, keys[s], msgs[i].tobytes()), np.uint8)
        return pk, sig
    return signer


def device_signer(sv, device=0):
    """The same through sv.sign_device."""
    import torch

    def signer(seeds, msgs):
        n = len(seeds)
        dev = torch.device("cuda", device)
        ts, tm = torch.from_numpy(np.ascontiguousarray(seeds)).to(dev), torch.from_numpy(np.ascontiguousarray(msgs)).to(dev)
        tpk = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        tsig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        sv.sign_device(device, ts.data_ptr(), tm.data_ptr(), n, tpk.data_ptr(), tsig.data_ptr(),
                       torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        return tpk.cpu().numpy(), tsig.cpu().numpy()
    return signer


def oracle_over_digests(oracle, pk, sig, digests, sig_begin):
    out = np.zeros(len(pk), np.uint8)
    for t in range(len(sig_begin) - 1):
        d = digests[t].tobytes()
        for i in range(int(sig_begin[t]), int(sig_begin[t + 1])):
            out[i] = 1 if oracle.oracle_ed25519_verify(sig[i].tobytes(), d, 32, pk[i].tobytes()) == 0 else 0
    return out


def make_set(nb, seed, signer, oracle, big=True, n_keys=8):
    """nb bodies from the pool, 0 / 1 / 20 signatures each (sigs_per_body)."""
    rng = np.random.default_rng(seed)
    shapes = pool_shapes(nb, rng, big)
    return make_custom([k for k, _ in shapes], [ln for _, ln in shapes], [sigs_per_body(t) for t in range(nb)], rng,
                       signer, oracle, n_keys)


def make_custom(kind, length, counts, rng, signer, oracle=None, n_keys=8):
    """Bodies of the given kinds / lengths / signature counts, with the pool's
    rejects.  verdict: the oracle's, or without an oracle (large sets) the
    verdicts by construction -- a signature is valid unless it was corrupted,
    its body was mutated after signing or it was made over the neighbour."""
    nb = len(kind)
    kind = np.array(kind, np.uint8)
    length = np.array(length, np.uint32)
    off = np.zeros(nb, np.uint64)
    off[1:] = np.cumsum(length[:-1], dtype=np.uint64)
    blob = rng.integers(0, 256, int(length.sum(dtype=np.uint64)) + 1, dtype=np.uint8)  # (never empty)
    body = lambda t: blob[int(off[t]):int(off[t]) + int(length[t])]  # noqa: E731
    counts = np.array(counts, np.uint64)
    sig_begin = np.zeros(nb + 1, np.uint64)
    sig_begin[1:] = np.cumsum(counts)
    n = int(sig_begin[-1])
    owner = np.repeat(np.arange(nb), counts.astype(np.int64))
    # each signature signs its body's hash, except the ones attached to the neighbour's
    signed = [contents_hash(int(kind[t]), body(t)) for t in range(nb)]
    target = owner.copy()
    for t in range(nb - 1):
        if t % 17 == 2 and counts[t] == 1:
            target[int(sig_begin[t])] = t + 1
    key_seeds = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    seeds = key_seeds[np.arange(n) % n_keys]
    msgs = np.array([np.frombuffer(signed[t], np.uint8) for t in target], np.uint8).reshape(n, 32)
    pk, sig = signer(seeds, msgs)
    pk, sig = np.ascontiguousarray(pk), np.array(sig, np.uint8)
    built = (target == owner).astype(np.uint8)
    for t in range(nb):  # one bit of the body, after signing
        if t % 13 == 1 and counts[t] > 0 and length[t] > 0:
            blob[int(off[t]) + int(length[t]) // 2] ^= 0x10
            built[int(sig_begin[t]):int(sig_begin[t + 1])] = 0
    sig[4::9, 40] ^= 1  # corrupted signature bytes
    built[4::9] = 0
    digests = np.array([np.frombuffer(contents_hash(int(kind[t]), body(t)), np.uint8) for t in range(nb)],
                       np.uint8).reshape(nb, 32)
    verdict = oracle_over_digests(oracle, pk, sig, digests, sig_begin) if oracle is not None else built
    assert verdict.any() and not verdict.all(), "the set needs an accept and a reject"
    return dict(bodies=blob, off=off, len=length, kind=kind, sig_begin=sig_begin, pk=pk, sig=sig, n=n, nb=nb,
                digests=digests, verdict=verdict, built=built)


def args(s):
    """Positional arguments of sv.verify_txbodies / verify_txbodies_cpu."""
    return (NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["pk"], s["sig"])
