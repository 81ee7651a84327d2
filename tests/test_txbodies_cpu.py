"""Signatures straight from transaction bodies, on a host without a GPU: the
CPU entry point against hashlib and the oracle, the argument errors of all
three entry points, and the host mirror's svh_check_envelopes_bodies through
its host-hash form and its CPU fallback."""
import ctypes

import numpy as np
import pytest

import txbodies_pool as tp


@pytest.fixture(scope="module")
def pool(oracle):
    # ~200 bodies / ~300 signatures, signed by the plain-Python signer (each
    # signature asserted valid by the oracle before it is used)
    return tp.make_set(200, 11, tp.pysign_signer(oracle), oracle)


def test_cpu_entry_matches_hashlib_and_oracle(sv, pool):
    assert pool["nb"] == 200 and 250 <= pool["n"] <= 400
    for threads in (1, 4):
        verdict, digests = sv.verify_txbodies_cpu(*tp.args(pool), threads=threads)
        assert (digests == pool["digests"]).all()
        assert (verdict == pool["verdict"]).all()
    assert pool["verdict"].any() and not pool["verdict"].all()


def test_cpu_entry_digests_only_and_empty(sv, pool):
    """n == 0 with n_bodies > 0 is legal (only digests); so is an empty batch."""
    nb = 40
    none = np.zeros(nb + 1, np.uint64)
    verdict, digests = sv.verify_txbodies_cpu(tp.NETWORK_ID, pool["bodies"], pool["off"][:nb], pool["len"][:nb],
                                              pool["kind"][:nb], none, np.zeros((0, 32), np.uint8),
                                              np.zeros((0, 64), np.uint8))
    assert verdict.size == 0 and (digests == pool["digests"][:nb]).all()
    verdict, digests = sv.verify_txbodies_cpu(tp.NETWORK_ID, np.zeros(0, np.uint8), [], [], [], [0],
                                              np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8))
    assert verdict.size == 0 and digests.shape == (0, 32)


def _raw_calls(sv):
    """The three entry points with one argument list: f(nid, bodies, off, len,
    kind, nb, sig_begin, pk, sig, n, verdict, digests) -> return code."""
    lib = sv.load_library()
    return {
        "cpu": lambda *a: lib.sv_ed25519_verify_txbodies_cpu(*a, 1),
        "host": lambda *a: lib.sv_ed25519_verify_txbodies(*a, None),
        # (host arrays where device arrays go: an argument error returns before any is read)
        "device": lambda nid, b, o, ln, k, nb, sb, pk, sig, n, v, d: lib.sv_ed25519_verify_txbodies_device(
            0, nid, b, o, ln, k, nb, sb, pk, sig, n, v, None, d, None),
    }


@pytest.mark.parametrize("entry", ["cpu", "host", "device"])
def test_argument_errors(sv, pool, entry):
    call = _raw_calls(sv)[entry]
    nb = 8
    p = sv._ptr
    nid = np.frombuffer(tp.NETWORK_ID, np.uint8).copy()
    off, ln, kind = pool["off"][:nb].copy(), pool["len"][:nb].copy(), pool["kind"][:nb].copy()
    sb = np.arange(nb + 1, dtype=np.uint64)
    n = nb
    pk, sig = np.zeros((n, 32), np.uint8), np.zeros((n, 64), np.uint8)
    verdict, dig = np.zeros(n, np.uint8), np.zeros((nb, 32), np.uint8)

    def run(**kw):
        a = dict(nid=p(nid), bodies=p(pool["bodies"]), off=p(off), ln=p(ln), kind=p(kind), nb=nb, sb=p(sb), pk=p(pk),
                 sig=p(sig), n=n, verdict=p(verdict), dig=p(dig))
        a.update(kw)
        return call(a["nid"], a["bodies"], a["off"], a["ln"], a["kind"], a["nb"], a["sb"], a["pk"], a["sig"], a["n"],
                    a["verdict"], a["dig"])

    for name in ("nid", "bodies", "off", "ln", "kind", "sb", "pk", "sig", "verdict"):
        assert run(**{name: None}) == -1, name  # SV_ERR_INVALID_ARG
    if entry == "device":
        return  # (its kinds and CSR array are device memory: not validated by the host)
    bad_kind = kind.copy()
    bad_kind[3] = 3
    assert run(kind=p(bad_kind)) == -1
    for bad in (np.array([1, 1, 2, 3, 4, 5, 6, 7, 8], np.uint64),   # does not start at 0
                np.array([0, 1, 2, 3, 4, 5, 6, 7, 7], np.uint64),   # does not end at n
                np.array([0, 1, 3, 2, 4, 5, 6, 7, 8], np.uint64)):  # decreases
        assert run(sb=p(bad)) == -1


def test_gpu_entries_raise_without_gpu(sv, pool):
    try:
        n = sv.device_count()
    except sv.SigVerifyError:
        n = 0
    if n > 0:  # a GPU is present: the host entry works instead (test_gpu_txbodies.py checks it in full)
        verdict, digests = sv.verify_txbodies(*tp.args(pool))
        assert (digests == pool["digests"]).all() and (verdict == pool["verdict"]).all()
        return
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_NO_DEVICE"):
        sv.verify_txbodies(*tp.args(pool))
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_NO_DEVICE"):
        # (placeholder addresses: the call fails before any is read)
        sv.verify_txbodies_device(0, tp.NETWORK_ID, 16, 16, 16, 16, 1, 16, 16, 16, 1, 16)


# ------------------------------------------------ host mirror (svh_check_envelopes_bodies)
import envelope_bodies as eb  # noqa: E402
import envelopes as ev  # noqa: E402


class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    s = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(s))
    return s


@pytest.fixture(scope="module")
def host(sv):
    lib = ctypes.CDLL(sv.HOSTLIB_PATH)
    lib.svh_last_error_string.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope="module")
def handbuilt(oracle):
    return eb.build_set(2, 23, tp.pysign_signer(oracle))


def _bodies_call(host, s, prefetch, **kw):
    return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                     s["ebody"], prefetch=prefetch, **kw)


def test_mirror_bodies_match_hashed_envelopes(sv, host, handbuilt):
    s = handbuilt
    try:
        gpu = sv.device_count() > 0
    except sv.SigVerifyError:
        gpu = False
    ref, _ = ev.check_envelopes(host, s["envs"], *s["rest"], s["n"], s["naccounts"], 21)
    assert (ref["code"] == s["expect"]).all(), ref["code"]
    assert eb.txBAD_AUTH in ref["code"] and eb.txSUCCESS in ref["code"]
    for prefetch in (0, 1):
        _stats(host)
        res, pairs, ch, fb = _bodies_call(host, s, prefetch)
        assert (res == ref).all(), prefetch
        assert (ch == s["contents_hash"]).all() and (fb == s["fee_bump_hash"]).all(), prefetch
        st = _stats(host)
        if prefetch == 1:
            assert pairs > 0
            # without a GPU the one engine call fails and is re-run on the CPU path
            assert (st.fallbacks == 0 and st.gpu_batches >= 1) if gpu else st.fallbacks >= 1


def test_mirror_bodies_refuses_keyed_form_and_bad_kind(host, handbuilt):
    s = handbuilt
    assert _bodies_call(host, s, 2, expect_rc=-1) == -1  # SVH_ERR_INVALID_ARG
    bad = s["ebody"].copy()
    bad[0]["kind"] = 2
    assert eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"], bad,
                                     prefetch=0, expect_rc=-1) == -1
