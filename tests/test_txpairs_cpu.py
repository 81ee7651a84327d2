"""Pairing by hint, on a host without a GPU: the CPU form
sv_ed25519_verify_txbodies_hinted_cpu and the binding against the plain-Python
contract of txpairs_pool.py (double loop, hashlib, the oracle), the capacity
error, the argument errors, sv_txbodies_pair_bound, the host mirror's prefetch
3 through its CPU fallback, and the host code under sanitizers as a stand-alone
program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envelope_bodies as eb
import txbodies_pool as tp
import txpairs_pool as pp

HERE = os.path.dirname(os.path.abspath(__file__))
NB = 70


@pytest.fixture(scope="module")
def pool(sv, oracle):
    sv.load_library().sv_ed25519_verify_txbodies_hinted_cpu  # (the entry points under test exist)
    s = pp.make_pool(NB, 41, tp.pysign_signer(oracle))
    return s, pp.expected(s, oracle)


def test_pool_holds_the_mandatory_cases(pool):
    s, want = pool
    pb, ps, pk, v = want["pair_begin"], want["pair_sig"], want["pair_key"], want["verdict"]
    count = lambda name: int(pb[pp.CASES.index(name) + 1] - pb[pp.CASES.index(name)])  # noqa: E731
    rows = lambda name: slice(int(pb[pp.CASES.index(name)]), int(pb[pp.CASES.index(name) + 1]))  # noqa: E731
    assert count("no_match") == 0
    assert count("multi") == 4 and v[rows("multi")].tolist() == [0, 1, 0, 1]  # wrong keys reject, the signers accept
    assert count("neighbour") == 1 and count("neighbour_mid") == 0 and count("neighbour_hi") == 1
    assert count("dup_key") == 2 and v[rows("dup_key")].tolist() == [1, 1]
    assert count("sigs_only") == 0 and count("keys_only") == 0 and count("empty") == 0
    g = pp.CASES.index("grid")
    assert count("grid") == 400
    s0, k0 = int(s["sig_begin"][g]), int(s["key_begin"][g])
    assert (ps[rows("grid")] == s0 + np.repeat(np.arange(20), 20)).all()  # signature-major
    assert (pk[rows("grid")] == k0 + np.tile(np.arange(20), 20)).all()
    assert 0 < int(v[rows("grid")].sum()) < 400
    assert count("one_byte") == 0 and count("head") == 0
    assert set(s["kind"].tolist()) == {0, 1, 2}
    assert v.any() and not v.all()


def test_cpu_form_matches_the_contract(sv, pool):
    s, want = pool
    for threads in (1, 4):
        pp.check(sv.verify_txbodies_hinted_cpu(*pp.args(s), threads=threads), want)


def test_pair_cap(sv, pool):
    s, want = pool
    n = len(want["pair_sig"])
    pp.check(sv.verify_txbodies_hinted_cpu(*pp.args(s), pair_cap=n), want)
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_PAIR_CAP") as e:
        sv.verify_txbodies_hinted_cpu(*pp.args(s), pair_cap=n - 1)
    assert e.value.needed == n and e.value.code == sv.SV_ERR_PAIR_CAP
    # zero pairs with pair_cap == 0 (null pair arrays): digests are still produced
    nb = 9
    none = np.zeros(nb + 1, np.uint64)
    got = sv.verify_txbodies_hinted_cpu(tp.NETWORK_ID, s["bodies"], s["off"][:nb], s["len"][:nb], s["kind"][:nb], none,
                                        np.zeros((0, 4), np.uint8), np.zeros((0, 64), np.uint8), none,
                                        np.zeros((0, 32), np.uint8), pair_cap=0)
    assert (got[0] == 0).all() and got[1].size == 0 and got[3].size == 0
    assert (got[4] == want["digests"][:nb]).all()
    # signatures and keys, but no match: still legal with pair_cap == 0
    t = pp.CASES.index("no_match")
    sl = lambda a, b, w: a[int(b[t]):int(b[t + 1])]  # noqa: E731
    got = sv.verify_txbodies_hinted_cpu(tp.NETWORK_ID, s["bodies"], s["off"][t:t + 1], s["len"][t:t + 1],
                                        s["kind"][t:t + 1], [0, 1], sl(s["hint"], s["sig_begin"], 4),
                                        sl(s["sig"], s["sig_begin"], 64), [0, 2], sl(s["key"], s["key_begin"], 32),
                                        pair_cap=0)
    assert got[0].tolist() == [0, 0] and (got[4] == want["digests"][t:t + 1]).all()


def test_pair_bound(sv, pool):
    s, want = pool
    ns, nk = np.diff(s["sig_begin"].astype(np.int64)), np.diff(s["key_begin"].astype(np.int64))
    bound = sv.txbodies_pair_bound(s["sig_begin"], s["key_begin"])
    assert bound == int((ns * nk).sum()) and bound >= len(want["pair_sig"])
    assert sv.txbodies_pair_bound([0], [0]) == 0


def test_malformed_csr_is_rejected(sv, pool):
    s, _ = pool
    a = list(pp.args(s))
    SB, KB = 5, 8
    for which in (SB, KB):
        good = a[which]
        for bad in (good + np.uint64(1),                       # does not start at 0
                    np.concatenate([good[:-1], good[-1:] + np.uint64(1)]),  # does not end at the count
                    np.concatenate([good[:3], good[2:3] - np.uint64(1), good[4:]]) if good[2] > 0 else None,
                    good[:-1]):                                # wrong length
            if bad is None:
                continue
            b = list(a)
            b[which] = bad
            with pytest.raises(ValueError):
                sv.verify_txbodies_hinted_cpu(*b)
            with pytest.raises(ValueError):
                sv.verify_txbodies_hinted(*b)
    with pytest.raises(ValueError):
        sv.verify_txbodies_hinted_cpu(*a[:6], a[6][:-1], *a[7:])  # hint / sig row mismatch


def test_c_entry_points_reject_bad_arguments(sv, pool):
    """The C layer's own checks (the binding's ValueErrors never reach it)."""
    s, want = pool
    lib = sv.load_library()
    p = sv._ptr
    nid = np.frombuffer(tp.NETWORK_ID, np.uint8).copy()
    nb, ns, nk = s["nb"], s["ns"], s["nk"]
    cap = len(want["pair_sig"])
    pb, ps, pk, pv = np.zeros(nb + 1, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    n = ctypes.c_size_t(0)

    def run(entry, **kw):
        a = dict(nid=p(nid), bodies=p(s["bodies"]), off=p(s["off"]), ln=p(s["len"]), kind=p(s["kind"]), nb=nb,
                 sb=p(s["sig_begin"]), hint=p(s["hint"]), sig=p(s["sig"]), ns=ns, kb=p(s["key_begin"]), key=p(s["key"]),
                 nk=nk, cap=cap, pb=p(pb), ps=p(ps), pk=p(pk), pv=p(pv), n=ctypes.byref(n))
        a.update(kw)
        args = [a[k] for k in ("nid", "bodies", "off", "ln", "kind", "nb", "sb", "hint", "sig", "ns", "kb", "key", "nk",
                               "cap", "pb", "ps", "pk", "pv", "n")]
        if entry == "cpu":
            return lib.sv_ed25519_verify_txbodies_hinted_cpu(*args, None, 1)
        return lib.sv_ed25519_verify_txbodies_hinted(*args, None, None)

    for entry in ("cpu", "host"):
        for name in ("nid", "off", "ln", "kind", "sb", "hint", "sig", "kb", "key", "pb", "ps", "pk", "pv", "n"):
            assert run(entry, **{name: None}) == -1, (entry, name)
        for which, arr in (("sb", s["sig_begin"]), ("kb", s["key_begin"])):
            bad = arr.copy()
            bad[-1] += 1
            assert run(entry, **{which: p(bad)}) == -1
            bad = arr.copy()
            bad[0] = 1
            assert run(entry, **{which: p(bad)}) == -1
            bad = arr.copy()
            bad[3], bad[4] = max(bad[3], bad[4]) + 1, min(bad[3], bad[4])  # decreases
            assert run(entry, **{which: p(bad)}) == -1
        kind = s["kind"].copy()
        kind[2] = 3
        assert run(entry, kind=p(kind)) == -1
        assert run(entry, ns=1 << 32) == -1 and run(entry, nk=1 << 32) == -1
    assert run("cpu", cap=cap - 1) == sv.SV_ERR_PAIR_CAP and n.value == cap
    # the device form: null and misaligned arguments fail before anything is read
    dev = lambda **kw: lib.sv_ed25519_verify_txbodies_hinted_device(  # noqa: E731
        0, p(nid), 16, 16, 16, 16, 1, 16, kw.get("hint", 16), kw.get("sig", 16), 1, 16, kw.get("key", 16), 1, 1,
        kw.get("pb", 16), 16, 16, 16, None, ctypes.byref(n), None, None)
    assert dev(pb=None) == -1 and dev(sig=None) == -1 and dev(key=None) == -1
    assert dev(sig=24) == -6 and dev(key=8) == -6 and dev(hint=18) == -6  # SV_ERR_ALIGN


def test_gpu_entries_without_gpu(sv, pool):
    s, want = pool
    try:
        n = sv.device_count()
    except sv.SigVerifyError:
        n = 0
    if n > 0:  # a GPU is present: the host entry works instead (test_gpu_txpairs.py checks it in full)
        pp.check(sv.verify_txbodies_hinted(*pp.args(s)), want)
        return
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_NO_DEVICE"):
        sv.verify_txbodies_hinted(*pp.args(s))
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_NO_DEVICE"):
        # (placeholder addresses: the call fails before any is read)
        sv.verify_txbodies_hinted_device(0, tp.NETWORK_ID, 16, 16, 16, 16, 1, 16, 16, 16, 1, 16, 16, 1, 1, 16, 16, 16, 16)


# ------------------------------------------------ host mirror (prefetch 3)
class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    st = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(st))
    return st


@pytest.mark.parametrize("with_payload", [True, False])
def test_mirror_prefetch3_matches_prefetch0(sv, oracle, with_payload):
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(2, 23, tp.pysign_signer(oracle), with_payload=with_payload)
    try:
        gpu = sv.device_count() > 0
    except sv.SigVerifyError:
        gpu = False

    def call(prefetch):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch)

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all(), ref["code"]
    assert eb.txBAD_AUTH in ref["code"] and eb.txSUCCESS in ref["code"]
    _stats(host)
    res, pairs, ch, fb = call(3)
    st = _stats(host)
    assert (res == ref).all()
    assert (ch == ch0).all() and (fb == fb0).all()
    assert (ch == s["contents_hash"]).all() and (fb == s["fee_bump_hash"]).all()
    assert pairs > 0
    # without a GPU the one engine call fails and is re-run on the CPU form
    assert (st.fallbacks == 0 and st.gpu_batches >= 1) if gpu else st.fallbacks >= 1
    _, pairs1, _, _ = call(1)
    assert pairs == pairs1  # the engine found the pairs the host enumeration finds


# ------------------------------------------------ host code under sanitizers
def test_host_code_under_sanitizers(tmp_path):
    """tests/native/txpair_core.cpp (its own main) + the CPU path, built with
    ASan and UBSan and run directly: nothing is loaded into Python."""
    exe = str(tmp_path / "txpair_core")
    repo = os.path.dirname(HERE)
    # (the sanitizer runtimes linked statically: the program needs nothing preloaded)
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(HERE, "native", "txpair_core.cpp"),
           os.path.join(repo, "stellar-core_amd", "csrc", "sv_cpu.cpp"), "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "txpair_core ok" in r.stdout, r.stdout[-4000:]
