"""Batch signing on the device (sv_sign.hip through sv_ed25519_sign_batch_device, sv_ed25519_sign_batch and the
tx-body forms): byte-equal to libsodium's signatures (the committed fixtures, digests.json), to the old dataset
signer, and between the device, host and CPU forms."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sign_sets as ss
import txbodies_pool as tp
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GUARD = 64  # sentinel bytes on either side of a device output (keeps the 16-byte alignment)


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _guarded(dev, nbytes, fill):
    return torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)


def _inner(t, nbytes, fill, what):
    a = t.cpu().numpy()
    assert (a[:GUARD] == fill).all() and (a[GUARD + nbytes:] == fill).all(), "%s: a sentinel was overwritten" % what
    return a[GUARD:GUARD + nbytes]


def dev_sign(sv, dev, seeds, msg, off=None, ln=None, key_of=None, fixed=0, want_pk=True, n=None, k=None):
    """sv_ed25519_sign_batch_device -> (sig n x 64, pk k x 32), with the sentinels around both outputs checked."""
    seeds = np.ascontiguousarray(seeds, np.uint8).reshape(-1, 32)
    k = seeds.shape[0] if k is None else k
    n = (k if key_of is None else len(key_of)) if n is None else n
    t_seed = _up(dev, seeds if seeds.size else np.zeros((1, 32), np.uint8))
    t_msg = _up(dev, msg if np.asarray(msg).size else np.zeros(1, np.uint8))
    t_off = _up(dev, np.asarray(off, np.uint64)) if off is not None and len(off) else None
    t_len = _up(dev, np.asarray(ln, np.uint32)) if ln is not None and len(ln) else None
    t_key = _up(dev, np.asarray(key_of, np.uint32)) if key_of is not None and len(key_of) else None
    t_sig, t_pk = _guarded(dev, 64 * n, 0xA5), _guarded(dev, 32 * k, 0x5A)
    sv.sign_batch_device(0, t_seed.data_ptr(), k, t_msg.data_ptr(), n, t_sig.data_ptr() + GUARD,
                         d_pk=t_pk.data_ptr() + GUARD if want_pk else 0, d_key_of=t_key.data_ptr() if t_key is not None else 0,
                         fixed_msg_len=fixed, d_msg_off=t_off.data_ptr() if t_off is not None else 0,
                         d_msg_len=t_len.data_ptr() if t_len is not None else 0,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    sig = _inner(t_sig, 64 * n, 0xA5, "d_sig").reshape(n, 64).copy()
    pk = _inner(t_pk, 32 * k, 0x5A, "d_pk").reshape(k, 32).copy()
    return sig, pk


def test_fixture_reproduction(sv, dev, golden):
    """The ~1600 libsodium signatures of the fixtures, one mixed-length call, through the device and the host form."""
    s = ss.fixture_set(golden)
    for what, (sig, pk) in (("device", dev_sign(sv, dev, s["seed"], s["msg"], s["off"], s["len"])),
                            ("host", sv.sign_batch(s["seed"], s["msg"], s["off"], s["len"], device=0))):
        assert (pk == s["pk"]).all(), what
        bad = np.nonzero((sig != s["sig"]).any(axis=1))[0]
        assert bad.size == 0, "%s: signatures differ at rows %s (lengths %s)" % (what, bad[:10], s["len"][bad[:10]])
    # the slot's own tables of B (32 x 129 entries of 192 bytes) and its signing buffers are accounted for
    assert sv.workspace_bytes(0) >= 32 * 129 * 192 + 96 * s["n"]


def test_digest_65536(sv, dev):
    with open(os.path.join(GOLDEN, "digests.json")) as f:
        want = json.load(f)["65536"]
    seeds, msgs = ss.svseed_set(65536)
    sig, pk = dev_sign(sv, dev, seeds, msgs, fixed=32)
    assert ss.stream_digest(pk, sig, msgs) == want


def test_equals_old_signer(sv, dev):
    """4099 random seeds and 32-byte messages: sv_ed25519_sign_device's bytes, in fixed-length mode and in
    variable-length mode with every length 32."""
    n = 4099
    rng = np.random.default_rng(4099)
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    old_pk, old_sig = tp.device_signer(sv)(seeds, msgs)
    sig, pk = dev_sign(sv, dev, seeds, msgs, fixed=32)
    assert (pk == old_pk).all() and (sig == old_sig).all()
    sig, pk = dev_sign(sv, dev, seeds, msgs, off=32 * np.arange(n, dtype=np.uint64), ln=np.full(n, 32, np.uint32))
    assert (pk == old_pk).all() and (sig == old_sig).all()


def _seam_set(n, k, shared):
    rng = np.random.default_rng(1000 * k + n)
    seeds = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    key_of = rng.integers(0, k, n).astype(np.uint32) if shared else None
    lens = rng.integers(0, 200, n).astype(np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    msg = rng.integers(0, 256, int(lens.sum()) + 1, dtype=np.uint8)
    return seeds, key_of, msg, off, lens


SEAMS = [(n, n, False) for n in (1, 63, 64, 65, 255, 256, 257)] + [(1000, 1, True), (1000, 3, True)]


@pytest.fixture(scope="module")
def seam_results(sv, dev):
    """Per (n, k): the set and the device form's (sig, pk); shared and left unchanged."""
    out = {}
    for n, k, shared in SEAMS:
        seeds, key_of, msg, off, lens = _seam_set(n, k, shared)
        out[(n, k)] = (seeds, key_of, msg, off, lens) + dev_sign(sv, dev, seeds, msg, off, lens, key_of=key_of)
    return out


@pytest.mark.parametrize("n,k,shared", SEAMS)
def test_block_seams(sv, dev, seam_results, n, k, shared):
    """Sizes around the 64-lane wave and the 256-lane block, and shared keys: device, host and CPU forms byte-equal."""
    seeds, key_of, msg, off, lens, sig_d, pk_d = seam_results[(n, k)]
    sig_c, pk_c = sv.sign_batch_cpu(seeds, msg, off, lens, key_of=key_of)
    sig_h, pk_h = sv.sign_batch(seeds, msg, off, lens, key_of=key_of, device=0)
    assert (pk_d == pk_c).all() and (pk_h == pk_c).all()
    assert (sig_d == sig_c).all() and (sig_h == sig_c).all()


def test_round_trip(sv, dev, seam_results):
    """One sv_ed25519_verify_device call over the largest seam set accepts every signature."""
    seeds, key_of, msg, off, lens, sig, pk = seam_results[(1000, 3)]
    n = len(key_of)
    t_pk, t_sig, t_msg = _up(dev, pk[key_of]), _up(dev, sig), _up(dev, msg)
    t_off, t_len = _up(dev, off), _up(dev, lens)
    t_v = torch.zeros(n, dtype=torch.uint8, device=dev)
    sv.verify_device(0, t_pk.data_ptr(), t_sig.data_ptr(), t_msg.data_ptr(), n, t_v.data_ptr(),
                     stream=torch.cuda.current_stream(dev).cuda_stream, fixed_msg_len=0, d_msg_off=t_off.data_ptr(),
                     d_msg_len=t_len.data_ptr())
    torch.cuda.synchronize(dev)
    assert (t_v.cpu().numpy() == 1).all()


def test_device_clamps(sv, dev):
    """Nothing is validated on the device: an out-of-range key_of row is 64 zero bytes with its neighbours intact,
    nothing lands outside d_sig and d_pk (dev_sign checks the sentinels), n == 0 and k == 0 work."""
    seeds, _, msg, off, lens = _seam_set(300, 3, True)
    key_of = (np.arange(300) % 3).astype(np.uint32)
    want, want_pk = sv.sign_batch_cpu(seeds, msg, off, lens, key_of=key_of)
    bad = key_of.copy()
    rows = np.array([0, 63, 64, 200, 255, 256, 299])
    bad[rows] = [3, 4, 0xFFFFFFFF, 3, 1 << 31, 3, 7]
    sig, pk = dev_sign(sv, dev, seeds, msg, off, lens, key_of=bad)
    assert (pk == want_pk).all()
    assert (sig[rows] == 0).all()
    keep = np.setdiff1d(np.arange(300), rows)
    assert (sig[keep] == want[keep]).all()
    # key_of NULL with k < n: rows at or past k have no key
    sig, pk = dev_sign(sv, dev, seeds, msg, off[:5], lens[:5], n=5)
    alone, _ = sv.sign_batch_cpu(seeds, msg, off[:3], lens[:3])
    assert (sig[:3] == alone).all() and (sig[3:] == 0).all()
    # n == 0 with k > 0: public keys only; without d_pk: nothing at all is written
    sig, pk = dev_sign(sv, dev, seeds, msg, n=0, fixed=32)
    assert sig.shape == (0, 64) and (pk == want_pk).all()
    sig, pk = dev_sign(sv, dev, seeds, msg, off, lens, key_of=key_of, want_pk=False)
    assert (sig == want).all() and (pk == 0x5A).all()
    # k == 0
    sig, pk = dev_sign(sv, dev, np.zeros((0, 32), np.uint8), msg, n=0, k=0, fixed=32)
    assert sig.shape == (0, 64) and pk.shape == (0, 32)
    assert sv.sign_batch(np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), fixed_msg_len=32, device=0)[0].shape == (0, 64)
    sig, pk = sv.sign_batch(seeds, np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32),
                            key_of=np.zeros(0, np.uint32), device=0)
    assert sig.shape == (0, 64) and (pk == want_pk).all()


def test_sign_txbodies_gpu(sv, dev):
    """The tx-body forms on the GPU: device form == host form == CPU form, and the device outputs go straight into
    sv_ed25519_verify_txbodies_hinted_device, which pairs every signature with its signer and accepts it."""
    s = ss.tx_signing_set(np.random.default_rng(5))
    n, nb, k = s["n"], s["nb"], len(s["seed"])
    want = sv.sign_txbodies_cpu(tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["seed"],
                                s["key_of"])
    assert (want[3] == s["digests"]).all()
    host = sv.sign_txbodies(tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["seed"],
                            s["key_of"], device=0)
    for a, b in zip(host, want):
        assert (a == b).all()
    t_bodies, t_off, t_len, t_kind = _up(dev, s["bodies"]), _up(dev, s["off"]), _up(dev, s["len"]), _up(dev, s["kind"])
    t_sb, t_seed, t_key_of = _up(dev, s["sig_begin"]), _up(dev, s["seed"]), _up(dev, s["key_of"])
    t_hint, t_sig = _guarded(dev, 4 * n, 0xA5), _guarded(dev, 64 * n, 0xA5)
    t_pk, t_dig = _guarded(dev, 32 * k, 0x5A), _guarded(dev, 32 * nb, 0x5A)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sv.sign_txbodies_device(0, tp.NETWORK_ID, t_bodies.data_ptr(), t_off.data_ptr(), t_len.data_ptr(),
                            t_kind.data_ptr(), nb, t_sb.data_ptr(), t_seed.data_ptr(), k, t_key_of.data_ptr(), n,
                            t_hint.data_ptr() + GUARD, t_sig.data_ptr() + GUARD, t_pk.data_ptr() + GUARD,
                            t_dig.data_ptr() + GUARD, stream)
    # ... and, queued behind it on the same stream, the hinted verifier over the signer's outputs
    t_keys = t_pk[GUARD:GUARD + 32 * k].reshape(k, 32)[t_key_of.view(torch.int32).long()].contiguous()
    cap = n
    t_pb = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
    t_ps = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    t_pkey = torch.full((cap,), -1, dtype=torch.int32, device=dev)
    t_v = torch.full((cap,), 7, dtype=torch.uint8, device=dev)
    n_pairs = sv.verify_txbodies_hinted_device(0, tp.NETWORK_ID, t_bodies.data_ptr(), t_off.data_ptr(),
                                               t_len.data_ptr(), t_kind.data_ptr(), nb, t_sb.data_ptr(),
                                               t_hint.data_ptr() + GUARD, t_sig.data_ptr() + GUARD, n,
                                               t_sb.data_ptr(), t_keys.data_ptr(), n, cap, t_pb.data_ptr(),
                                               t_ps.data_ptr(), t_pkey.data_ptr(), t_v.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)
    got = (_inner(t_hint, 4 * n, 0xA5, "d_hint").reshape(n, 4), _inner(t_sig, 64 * n, 0xA5, "d_sig").reshape(n, 64),
           _inner(t_pk, 32 * k, 0x5A, "d_pk").reshape(k, 32), _inner(t_dig, 32 * nb, 0x5A, "d_digests").reshape(nb, 32))
    for a, b in zip(got, want):
        assert (a == b).all()
    assert n_pairs == n
    assert sorted(t_ps.cpu().numpy().tolist()) == list(range(n))
    assert (t_pkey.cpu().numpy() == t_ps.cpu().numpy()).all()
    assert (t_v.cpu().numpy() == 1).all()


def test_multi_chunk_host_call(sv, dev):
    """The staging chunk is read once per process, so the calls run in a fresh child with a small SV_STAGE_CHUNK
    (tests/sign_multichunk.py holds the sets and the comparisons)."""
    env = dict(os.environ, SV_STAGE_CHUNK="1024")
    r = subprocess.run([sys.executable, os.path.join(HERE, "sign_multichunk.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "sign multichunk ok" in r.stdout, r.stdout[-4000:]


def test_fixed_base_probe(dev):
    """The sign_core.h fixed-base multiplication compiled for gfx950 with the product's flags, one lane per chosen
    scalar, against integer arithmetic."""
    d = os.path.join(HERE, "native")
    subprocess.run(["make", "-s", "-f", "sign.mk", "libsignprobe.so"], cwd=d, check=True)
    lib = ctypes.CDLL(os.path.join(d, "libsignprobe.so"))
    lib.sgp_fixed_base.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _, s = ss.chosen_scalars()
    out = np.zeros_like(s)
    p = lambda a: ctypes.c_void_p(a.__array_interface__["data"][0])  # noqa: E731
    assert lib.sgp_fixed_base(p(s), len(s), p(out)) == 0
    ref = ss.fixed_base_ref()
    bad = np.nonzero((out != ref).any(axis=1))[0]
    assert bad.size == 0, "rows %s" % bad[:10]
