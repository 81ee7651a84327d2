"""Batch signing on the engine's CPU path and the host-side refusals
(sv_ed25519_sign_batch_cpu, sv_ed25519_sign_txbodies_cpu, the C++ mirror).

Ed25519 signing is deterministic, so the expected bytes are libsodium's own:
the committed fixtures were signed from derivable seeds (sign_sets.py)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import sign_sets as ss
import txbodies_pool as tp
from conftest import GOLDEN, REPO

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1  # SV_ERR_INVALID_ARG


def _p(a):
    return ctypes.c_void_p(a.__array_interface__["data"][0])


def test_exports(sv):
    lib = ctypes.CDLL(sv.LIB_PATH)
    assert sv.SV_ERRORS[INVALID] == "SV_ERR_INVALID_ARG"
    for name in ("sv_ed25519_sign_batch", "sv_ed25519_sign_batch_device", "sv_ed25519_sign_batch_cpu",
                 "sv_ed25519_sign_txbodies", "sv_ed25519_sign_txbodies_device", "sv_ed25519_sign_txbodies_cpu"):
        assert name in sv.EXPORTED_SYMBOLS and getattr(lib, name)


def test_fixture_reproduction(sv, golden):
    """All 513 msglen_valid, 1024 valid32, 64 valid256 and 18 long_valid rows in one mixed-length call: pk and sig
    byte-equal to libsodium's."""
    s = ss.fixture_set(golden)
    assert s["n"] == 513 + 1024 + 64 + 18
    sig, pk = sv.sign_batch_cpu(s["seed"], s["msg"], s["off"], s["len"])
    assert (pk == s["pk"]).all(), "public keys differ at rows %s" % np.nonzero((pk != s["pk"]).any(axis=1))[0][:10]
    bad = np.nonzero((sig != s["sig"]).any(axis=1))[0]
    assert bad.size == 0, "signatures differ at rows %s (lengths %s)" % (bad[:10], s["len"][bad[:10]])


def test_digest_1024(sv):
    with open(os.path.join(GOLDEN, "digests.json")) as f:
        want = json.load(f)["1024"]
    seeds, msgs = ss.svseed_set(1024)
    sig, pk = sv.sign_batch_cpu(seeds, msgs, fixed_msg_len=32)
    assert ss.stream_digest(pk, sig, msgs) == want


@pytest.mark.parametrize("k", [1, 3])
def test_shared_keys(sv, oracle, k):
    n = 1000
    rng = np.random.default_rng(100 + k)
    seeds = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    key_of = rng.integers(0, k, n).astype(np.uint32)
    lens = rng.integers(0, 200, n).astype(np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    msg = rng.integers(0, 256, int(lens.sum()) + 1, dtype=np.uint8)
    sig, pk = sv.sign_batch_cpu(seeds, msg, off, lens, key_of=key_of)
    alone, pk_alone = sv.sign_batch_cpu(seeds[key_of], msg, off, lens)
    assert (sig == alone).all() and (pk[key_of] == pk_alone).all()
    for i in range(n):
        m = msg[int(off[i]):int(off[i]) + int(lens[i])].tobytes()
        assert oracle.oracle_ed25519_verify(sig[i].tobytes(), m, len(m), pk[key_of[i]].tobytes()) == 0, i


def _raw_call(lib, form, seed, k, key_of, msg, off, ln, fixed, n, sig, pk):
    if form == "cpu":
        return lib.sv_ed25519_sign_batch_cpu(seed, k, key_of, msg, off, ln, fixed, n, sig, pk, 1)
    return lib.sv_ed25519_sign_batch(seed, k, key_of, msg, off, ln, fixed, n, sig, pk, None)


@pytest.mark.parametrize("form", ["cpu", "host"])
def test_refusals(sv, form):
    """Each refusal alone, SV_ERR_INVALID_ARG before any work: the outputs stay untouched between their sentinels.
    (The host form refuses before it looks for a device, so this runs without one.)"""
    lib = sv.load_library()
    n = k = 4
    seed = np.arange(32 * k, dtype=np.uint8)
    msg = np.arange(64, dtype=np.uint8)
    off = np.array([0, 3, 10, 20], np.uint64)
    ln = np.array([3, 7, 10, 5], np.uint32)
    good_key = np.array([0, 3, 1, 1], np.uint32)
    cases = {
        "null seed": dict(seed=None),
        "null sig": dict(sig=None),
        "null msg_off": dict(off=None),
        "null msg_len": dict(ln=None),
        "null msg, fixed": dict(msg=None, fixed=8),
        "null msg, nonzero length": dict(msg=None),
        "key_of NULL with k != n": dict(k=3),
        "key_of entry == k": dict(key_of=np.array([0, 4, 1, 1], np.uint32)),
        "key_of entry huge": dict(key_of=np.array([0, 1, 0xFFFFFFFF, 1], np.uint32)),
        "k >= 2^32": dict(k=1 << 32, key_of=good_key),
        "n >= 2^32": dict(n=1 << 32, key_of=good_key),
    }
    for what, c in cases.items():
        sig = np.full(64 * n + 32, 0xA5, np.uint8)
        pk = np.full(32 * k + 32, 0x5A, np.uint8)
        a = dict(seed=seed, k=k, key_of=None, msg=msg, off=off, ln=ln, fixed=0, n=n, sig=sig[16:], pk=pk[16:])
        a.update(c)
        ptr = {key: (None if a[key] is None else _p(a[key])) for key in ("seed", "key_of", "msg", "off", "ln", "sig", "pk")}
        rc = _raw_call(lib, form, ptr["seed"], a["k"], ptr["key_of"], ptr["msg"], ptr["off"], ptr["ln"], a["fixed"],
                       a["n"], ptr["sig"], ptr["pk"])
        assert rc == INVALID, (what, rc)
        assert (sig == 0xA5).all() and (pk == 0x5A).all(), what
    # legal: k == 0 with n == 0 (nothing happens), and on the CPU form n == 0 with k > 0 (public keys only)
    assert _raw_call(lib, form, None, 0, None, None, None, None, 0, 0, None, None) == 0
    pk = np.zeros((k, 32), np.uint8)
    assert _raw_call(lib, "cpu", _p(seed), k, None, None, None, None, 0, 0, None, _p(pk)) == 0
    _, want = sv.sign_batch_cpu(seed.reshape(k, 32), msg, off, ln)
    assert (pk == want).all()


def test_sign_txbodies_cpu(sv, oracle):
    s = ss.tx_signing_set(np.random.default_rng(5))
    hint, sig, pk, dig = sv.sign_txbodies_cpu(tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"],
                                              s["seed"], s["key_of"])
    assert (dig == s["digests"]).all()
    want, want_pk = sv.sign_batch_cpu(s["seed"], s["sig_msgs"], key_of=s["key_of"], fixed_msg_len=32)
    assert (sig == want).all() and (pk == want_pk).all()
    assert (hint == pk[s["key_of"]][:, 28:]).all()
    # the outputs are the inputs of the hinted verifier: one candidate key per signature, its signer's
    key_begin = s["sig_begin"]
    pb, ps, pkey, pv, dig2 = sv.verify_txbodies_hinted_cpu(tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"],
                                                          s["sig_begin"], hint, sig, key_begin,
                                                          _signer_keys(s, pk))
    _check_pairs(s, ps, pkey, pv)
    assert (dig2 == s["digests"]).all()


def _signer_keys(s, pk):
    """Per body the distinct public keys of its signers, in first-use order (m x 32), with key_begin == sig_begin
    only when no body repeats a signer; the tx set repeats none inside a body."""
    for t in range(s["nb"]):
        ks = s["key_of"][int(s["sig_begin"][t]):int(s["sig_begin"][t + 1])]
        assert len(set(ks.tolist())) == len(ks)
    return pk[s["key_of"]]


def _check_pairs(s, pair_sig, pair_key, pair_verdict):
    """One pair per signature -- hints are 4 bytes of distinct random keys, so only the signer's key matches --
    and every pair verified."""
    assert len(pair_sig) == s["n"], (len(pair_sig), s["n"])
    assert sorted(pair_sig.tolist()) == list(range(s["n"]))
    assert (pair_key == pair_sig).all()
    assert (pair_verdict == 1).all()


def test_sign_txbodies_cpu_refusals(sv):
    lib = sv.load_library()
    s = ss.tx_signing_set(np.random.default_rng(5))
    nid = np.frombuffer(tp.NETWORK_ID, np.uint8).copy()
    n, nb, k = s["n"], s["nb"], 5
    bad_key = s["key_of"].copy()
    bad_key[3] = k
    bad_begin = s["sig_begin"].copy()
    bad_begin[-1] += 1
    for what, c in {"null key_of": dict(key_of=None), "key_of entry == k": dict(key_of=bad_key),
                    "null hint": dict(hint=None), "null network id": dict(nid=None),
                    "sig_begin does not end at n": dict(sb=bad_begin)}.items():
        hint = np.full(4 * n + 32, 0xA5, np.uint8)
        sig = np.full(64 * n + 32, 0xA5, np.uint8)
        a = dict(nid=nid, key_of=s["key_of"], hint=hint[16:], sb=s["sig_begin"])
        a.update(c)
        q = lambda v: None if v is None else _p(v)  # noqa: E731
        rc = lib.sv_ed25519_sign_txbodies_cpu(q(a["nid"]), _p(s["bodies"]), _p(s["off"]), _p(s["len"]), _p(s["kind"]),
                                              nb, _p(a["sb"]), _p(s["seed"]), k, q(a["key_of"]), n, q(a["hint"]),
                                              _p(sig[16:]), None, None, 1)
        assert rc == INVALID, (what, rc)
        assert (hint == 0xA5).all() and (sig == 0xA5).all(), what


@pytest.fixture(scope="module")
def host(sv):
    lib = ctypes.CDLL(os.path.join(REPO, "stellar-core_amd", "libstellar_host.so"))
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.svh_sign_batch.argtypes = [vp, sz, vp, vp, vp, vp, sz, vp, vp]
    lib.svh_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.c_char_p, ctypes.c_char_p]
    lib.svh_verify_sig.argtypes = [ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.c_char_p, sz]
    lib.svh_bench_sign.argtypes = [sz, sz, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    lib.svh_sign_fallbacks.restype = ctypes.c_uint64
    return lib


def test_mirror(sv, host, golden):
    """svh_sign_batch equals the C-ABI (here, with no device, through the mirror's re-run on the CPU path: an engine
    error is never a wrong signature), and a mirror sign -> verifySig round trip."""
    s = ss.fixture_set(golden)
    rows = np.r_[0:40, 513:530, 1537:1545]
    seeds = np.ascontiguousarray(s["seed"][rows])
    off, ln = np.ascontiguousarray(s["off"][rows]), np.ascontiguousarray(s["len"][rows])
    want, want_pk = sv.sign_batch_cpu(seeds, s["msg"], off, ln)
    sig = np.zeros((len(rows), 64), np.uint8)
    pk = np.zeros((len(rows), 32), np.uint8)
    assert host.svh_sign_batch(_p(seeds), len(rows), None, _p(s["msg"]), _p(off), _p(ln), len(rows), _p(sig), _p(pk)) == 0
    assert (sig == want).all() and (pk == want_pk).all()
    assert (sig == s["sig"][rows]).all()
    # a malformed batch is an error, not a fallback
    bad = np.full(len(rows), len(rows), np.uint32)
    host.svh_sign_fallbacks()
    assert host.svh_sign_batch(_p(seeds), len(rows), _p(bad), _p(s["msg"]), _p(off), _p(ln), len(rows), _p(sig), None) != 0
    assert host.svh_sign_fallbacks() == 0
    # sign -> verifySig
    m = b"mirror round trip"
    sg, p = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
    assert host.svh_sign(seeds[0].tobytes(), m, len(m), sg, p) == 0
    assert p.raw == want_pk[0].tobytes()
    assert host.svh_verify_sig(p.raw, sg.raw, 64, m, len(m)) == 1
    assert host.svh_verify_sig(p.raw, sg.raw, 64, m + b"!", len(m) + 1) == 0
    rate = ctypes.c_double(0)
    assert host.svh_bench_sign(16, 256, 1, 0, ctypes.byref(rate)) == 0 and rate.value > 0


def test_fixed_base_host(sv):
    """The sign_core.h fixed-base multiplication (host build, the device's field form) on the chosen scalars,
    against integer arithmetic."""
    lib = ctypes.CDLL(_build_signcore())
    ints, s = ss.chosen_scalars()
    out = np.zeros_like(s)
    lib.sgc_fixed_base.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.sgc_fixed_base(_p(s), len(s), _p(out))
    ref = ss.fixed_base_ref()
    bad = np.nonzero((out != ref).any(axis=1))[0]
    assert bad.size == 0, "rows %s" % bad[:10]


def _build_signcore():
    d = os.path.join(HERE, "native")
    subprocess.run(["make", "-s", "-f", "sign.mk", "libsigncore.so"], cwd=d, check=True)
    return os.path.join(d, "libsigncore.so")


def test_sign_core_sanitizers(tmp_path):
    """tests/native/sign_san.cpp (its own main) over csrc/sign_core.h, built with ASan and UBSan and run directly:
    nothing is loaded into Python."""
    exe = str(tmp_path / "sign_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas",
           "-I", os.path.join(REPO, "stellar-core_amd", "csrc"), "-o", exe,
           os.path.join(HERE, "native", "sign_san.cpp"), "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "sign_san ok: 1204 signatures" in r.stdout, r.stdout[-4000:]
