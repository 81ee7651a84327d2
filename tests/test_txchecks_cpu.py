"""Signature checks decided by the engine, on a host without a GPU: the CPU
form sv_ed25519_check_txbodies_cpu and the binding against the Python replay of
txchecks_pool.py (txset_gen.Checker per check) and by-hand expectations, the
argument errors and limits, the check planner and packer against a numpy
restatement of the layout, the host mirror's prefetch 5 through its CPU
fallback, and the host code under sanitizers as a stand-alone program.  Every
expectation is exact equality."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import envelope_bodies as eb
import envelopes as ev
import txbodies_pool as tp
import txchecks_pool as cp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def edge(sv, oracle):
    sv.load_library().sv_ed25519_check_txbodies_cpu  # (the entry points under test exist)
    bld = cp.Builder(3)
    cases = cp.edge_cases(bld)
    s = bld.finish(tp.pysign_signer(oracle))
    verify = cp.oracle_verify(oracle)
    return s, cases, verify


def _cpu(sv, s, protocol=21, sig_len=True, threads=0):
    return sv.check_txbodies_cpu(*cp.args(s), sig_len=s["sig_len"] if sig_len else None, protocol_version=protocol,
                                 threads=threads)


def test_edge_cases_by_hand(sv, edge):
    s, cases, _ = edge
    ok, weight, used, dig = _cpu(sv, s)
    assert (dig == s["digests"]).all()
    for name, (c0, hand) in cases.items():
        got = [(int(ok[c0 + i]), int(weight[c0 + i]), int(used[c0 + i])) for i in range(len(hand))]
        assert got == hand, name


def test_edge_cases_match_the_replay(sv, edge):
    s, _, verify = edge
    for protocol in (21, 10, 9):
        want = cp.expected(s, verify, protocol)
        for threads in (1, 4):
            cp.assert_equal(_cpu(sv, s, protocol, threads=threads), want, s)


def test_clamp_depends_on_the_protocol(sv, edge):
    s, cases, _ = edge
    c = cases["clamp"][0]
    for protocol, want in ((9, (1, 300, 1)), (10, (0, 255, 1))):
        ok, weight, used, _ = _cpu(sv, s, protocol)
        assert (int(ok[c]), int(weight[c]), int(used[c])) == want


def test_sig_len_null_means_64(sv, oracle):
    bld = cp.Builder(5)
    b = bld.body(length=40)
    k = b.key_ed(1)
    b.sig_ed(1)
    b.sig_ed(2)
    b.check(1, [(cp.ED, 1, k)])
    s = bld.finish(tp.pysign_signer(oracle))
    for with_len in (True, False):
        ok, weight, used, _ = _cpu(sv, s, sig_len=with_len)
        assert (ok.tolist(), weight.tolist(), used.tolist()) == ([1], [1], [1])


def _limit_set(oracle, n_sigs, n_signers):
    bld = cp.Builder(6)
    b = bld.body(length=30)
    k = b.key_ed(1)
    kw = b.key_wrong(2)
    for _ in range(n_sigs - 1):
        b.sig_raw(b"\0\0\0\0", bytes(64))
    b.sig_ed(1)  # the last signature is the one that matches
    b.check(1, [(cp.ED, 1, kw)] * (n_signers - 1) + [(cp.ED, 1, k)])  # ... the last signer
    return bld.finish(tp.pysign_signer(oracle))


def test_limits(sv, oracle):
    s = _limit_set(oracle, 64, 64)
    ok, weight, used, _ = _cpu(sv, s)
    assert (ok.tolist(), weight.tolist(), used.tolist()) == ([1], [1], [1 << 63])
    for ns, ng in ((65, 64), (64, 65)):
        with pytest.raises(sv.SigVerifyError, match="SV_ERR_INVALID_ARG"):
            _cpu(sv, _limit_set(oracle, ns, ng))
    # 65 signatures are legal on a body without checks
    bld = cp.Builder(7)
    b = bld.body(length=10)
    for _ in range(65):
        b.sig_raw(b"\0\0\0\0", bytes(64))
    b2 = bld.body(length=10)
    b2.check(0, [])
    s = bld.finish(tp.pysign_signer(oracle))
    assert _cpu(sv, s)[0].tolist() == [0]


def test_random_pool_matches_the_replay(sv, oracle):
    bld = cp.Builder(11)
    cp.random_pool(bld, 300)
    s = bld.finish(tp.pysign_signer(oracle))
    assert s["nc"] >= 300 and int(np.diff(s["sig_begin"].astype(np.int64)).max()) == 20
    want = cp.expected(s, cp.oracle_verify(oracle))
    assert want[0].any() and not want[0].all()
    cp.assert_equal(_cpu(sv, s), want, s)
    cp.assert_equal(_cpu(sv, s, protocol=9, threads=3), cp.expected(s, cp.oracle_verify(oracle), 9), s)


def test_c_entry_points_reject_bad_arguments(sv, edge):
    """The C layer's own checks, on the CPU form and the host form alike."""
    s, _, _ = edge
    lib = sv.load_library()
    p = sv._ptr
    nid = np.frombuffer(tp.NETWORK_ID, np.uint8).copy()
    nb, ns, nk, nc, ng = s["nb"], s["ns"], s["nk"], s["nc"], s["ng"]
    ok, weight, used = np.zeros(nc, np.uint8), np.zeros(nc, np.uint32), np.zeros(nc, np.uint64)
    a = lambda x: x.__array_interface__["data"][0]  # noqa: E731

    def run(entry, tables=None, **kw):
        t = dict(sig_len=a(s["sig_len"]), check_begin=a(s["check_begin"]), check_needed=a(s["check_needed"]),
                 signer_begin=a(s["signer_begin"]), signer_type=a(s["signer_type"]),
                 signer_weight=a(s["signer_weight"]), signer_key=a(s["signer_key"]), n_checks=nc, n_signers=ng,
                 protocol_version=21)
        keep = []
        for k, v in (tables or {}).items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = a(v)
            t[k] = v
        ck = sv._checks_desc(**t)
        if "struct_size" in kw:
            ck.struct_size = kw.pop("struct_size")
        args = dict(nid=p(nid), bodies=p(s["bodies"]), off=p(s["off"]), ln=p(s["len"]), kind=p(s["kind"]), nb=nb,
                    sb=p(s["sig_begin"]), hint=p(s["hint"]), sig=p(s["sig"]), ns=ns, kb=p(s["key_begin"]),
                    key=p(s["key"]), nk=nk, ck=ctypes.byref(ck), ok=p(ok), weight=p(weight), used=p(used))
        args.update(kw)
        order = [args[k] for k in ("nid", "bodies", "off", "ln", "kind", "nb", "sb", "hint", "sig", "ns", "kb", "key",
                                   "nk", "ck", "ok", "weight", "used")]
        if entry == "cpu":
            return lib.sv_ed25519_check_txbodies_cpu(*order, None, 1)
        return lib.sv_ed25519_check_txbodies(*order, None, None)

    def changed(name, fn):
        x = s[name].copy()
        fn(x)
        return {name: x}

    def set_(i, v):
        def f(x):
            x[i] = v
        return f

    for entry in ("cpu", "host"):
        assert run("cpu") == 0
        for name in ("nid", "off", "ln", "kind", "sb", "hint", "sig", "kb", "key", "ck", "ok", "weight", "used"):
            assert run(entry, **{name: None}) == -1, (entry, name)
        for name in ("check_begin", "check_needed", "signer_begin", "signer_type", "signer_weight", "signer_key"):
            assert run(entry, {name: 0}) == -1, (entry, name)
        assert run(entry, struct_size=16) == -1
        assert run(entry, {"protocol_version": 7}) == -1
        for which in ("sig_begin", "key_begin"):
            for i, v in ((0, 1), (-1, int(s[which][-1]) + 1), (3, int(s[which][4]) + 1)):
                bad = s[which].copy()
                bad[i] = v
                assert run(entry, **{"sb" if which == "sig_begin" else "kb": p(bad)}) == -1, (entry, which, i)
        for which in ("check_begin", "signer_begin"):
            for i, v in ((0, 1), (-1, int(s[which][-1]) + 1), (3, int(s[which][4]) + 1)):
                assert run(entry, changed(which, set_(i, v))) == -1, (entry, which, i)
        assert run(entry, changed("signer_type", set_(0, 4))) == -1
        assert run(entry, changed("sig_len", set_(0, 65))) == -1
        # a key index outside its body: the previous body's last key, the next body's first, past the array
        g = int(s["signer_begin"][int(s["check_begin"][1])])  # first signer of body 1
        for v in (int(s["key_begin"][1]) - 1, int(s["key_begin"][2]), nk):
            assert run(entry, changed("signer_key", set_(g, v))) == -1, (entry, v)
        kind = s["kind"].copy()
        kind[2] = 3
        assert run(entry, kind=p(kind)) == -1
        assert run(entry, ns=1 << 32) == -1 and run(entry, nk=1 << 32) == -1
    # the device form: null and misaligned arguments fail before anything is read
    ck = sv._checks_desc(21, 0, 16, 16, 16, 16, 16, 16, 1, 1)

    def dev(**kw):
        return lib.sv_ed25519_check_txbodies_device(
            0, p(nid), 16, 16, 16, 16, 1, 16, kw.get("hint", 16), kw.get("sig", 16), 1, 16, kw.get("key", 16), 1,
            ctypes.byref(kw.get("ck", ck)), kw.get("ok", 16), kw.get("weight", 16), 16, None, None)
    assert dev(ok=None) == -1 and dev(sig=None) == -1 and dev(key=None) == -1
    assert dev(ck=sv._checks_desc(7, 0, 16, 16, 16, 16, 16, 16, 1, 1)) == -1
    assert dev(ck=sv._checks_desc(21, 0, 0, 16, 16, 16, 16, 16, 1, 1)) == -1
    assert dev(sig=24) == -6 and dev(key=8) == -6 and dev(hint=18) == -6 and dev(weight=18) == -6  # SV_ERR_ALIGN


def test_binding_rejects_malformed_tables(sv, edge):
    s, _, _ = edge
    a = list(cp.args(s))
    CB, NEED, GB, GT = 10, 11, 12, 13
    for which in (CB, GB):
        b = list(a)
        b[which] = a[which][:-1]
        with pytest.raises(ValueError):
            sv.check_txbodies_cpu(*b)
    b = list(a)
    b[GT] = a[GT][:-1]
    with pytest.raises(ValueError):
        sv.check_txbodies_cpu(*b)
    with pytest.raises(ValueError):
        sv.check_txbodies_cpu(*a, sig_len=s["sig_len"][:-1])


def test_gpu_entries_without_gpu(sv, edge):
    s, _, verify = edge
    try:
        n = sv.device_count()
    except sv.SigVerifyError:
        n = 0
    if n > 0:  # a GPU is present: the host entry works instead (test_gpu_txchecks.py checks it in full)
        cp.assert_equal(sv.check_txbodies(*cp.args(s), sig_len=s["sig_len"]), cp.expected(s, verify), s)
        return
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_NO_DEVICE"):
        sv.check_txbodies(*cp.args(s), sig_len=s["sig_len"])
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_NO_DEVICE"):
        # (placeholder addresses: the call fails before any is read)
        sv.check_txbodies_device(0, tp.NETWORK_ID, 16, 16, 16, 16, 1, 16, 16, 16, 1, 16, 16, 1, 16, 16, 1, 16, 16, 16,
                                 16, 1, 16, 16, 16)


# ------------------------------------------------ planner and packer against numpy
@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """tests/native/txcheck_core.cpp built as the planner / packer shim."""
    so = str(tmp_path_factory.mktemp("txcheck") / "libtxcheckstage.so")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-DTXCHECK_STAGE_SHIM",
           "-Wno-unknown-pragmas", "-o", so, os.path.join(HERE, "native", "txcheck_core.cpp"), "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.hs_check_plan.argtypes = [vp] * 5 + [ctypes.c_int] + [u64] * 7 + [vp, ctypes.c_int]
    lib.hs_check_pack.argtypes = [vp] * 4 + [u64] + [vp] * 14
    return lib


PLAN_WORDS = ("b0", "b1", "s0", "s1", "k0", "k1", "body_bytes", "o_sig", "o_hint", "o_off", "o_sb", "o_kb", "o_len",
              "o_kind", "o_body", "p_bytes", "c0", "c1", "g0", "g1", "o_cb", "o_gb", "o_need", "o_gw", "o_gk", "o_gt",
              "o_sl", "bytes")


@pytest.mark.parametrize("with_len", [True, False])
def test_check_plan_and_pack(sv, oracle, stage, with_len):
    bld = cp.Builder(13)
    cp.random_pool(bld, 60)
    # (the layout needs no real signatures: a key per seed, constant signature bytes)
    s = bld.finish(lambda seeds, msgs: (np.ascontiguousarray(seeds[:, ::-1]), np.ones((len(seeds), 64), np.uint8)))
    P = sv._ptr
    nb = s["nb"]
    sb, kb, cb, gb = s["sig_begin"], s["key_begin"], s["check_begin"], s["signer_begin"]
    al16 = lambda v: (int(v) + 15) & ~15  # noqa: E731
    sl = s["sig_len"] if with_len else None
    for max_s, max_k, max_b, max_c, max_g in ((1 << 18, 1 << 18, 64 << 20, 1 << 18, 1 << 18), (25, 1 << 18, 64 << 20, 1 << 18, 1 << 18),
                                               (1 << 18, 1 << 18, 64 << 20, 5, 1 << 18), (1 << 18, 1 << 18, 64 << 20, 1 << 18, 9),
                                               (1 << 18, 6, 600, 1 << 18, 1 << 18), (1, 1, 16, 1, 1)):
        out = np.zeros(28 * 128, np.uint64)
        n = stage.hs_check_plan(P(s["len"]), P(sb), P(kb), P(cb), P(gb), int(with_len), 0, nb, max_s, max_k, max_b,
                                max_c, max_g, P(out), 128)
        assert 1 <= n <= 128
        plan = [dict(zip(PLAN_WORDS, map(int, out[28 * i:28 * i + 28]))) for i in range(n)]
        assert plan[0]["b0"] == 0 and plan[-1]["b1"] == nb
        if max_c == 5 or max_g == 9:
            assert n > 1  # the bound on checks / signers alone splits the set
        for i, c in enumerate(plan):
            k, m, q = c["b1"] - c["b0"], c["s1"] - c["s0"], c["k1"] - c["k0"]
            nc, ng = c["c1"] - c["c0"], c["g1"] - c["g0"]
            if i:
                assert c["b0"] == plan[i - 1]["b1"]
            assert (c["s0"], c["s1"], c["k0"], c["k1"]) == tuple(int(x) for x in (sb[c["b0"]], sb[c["b1"]], kb[c["b0"]], kb[c["b1"]]))
            assert (c["c0"], c["c1"]) == (int(cb[c["b0"]]), int(cb[c["b1"]]))
            assert (c["g0"], c["g1"]) == (int(gb[c["c0"]]), int(gb[c["c1"]]))
            bytes_ = sum(al16(x) for x in s["len"][c["b0"]:c["b1"]])
            assert c["body_bytes"] == bytes_
            assert k == 1 or (m <= max_s and q <= max_k and bytes_ <= max_b and nc <= max_c and ng <= max_g)
            if c["b1"] < nb:  # greedy: the next body would break a bound
                t = c["b1"]
                assert (int(sb[t + 1]) - c["s0"] > max_s or int(kb[t + 1]) - c["k0"] > max_k
                        or int(cb[t + 1]) - c["c0"] > max_c or int(gb[int(cb[t + 1])]) - c["g0"] > max_g
                        or bytes_ + al16(s["len"][t]) > max_b)
            # the hinted image, then the check tables
            want = {"o_sig": 32 * q, "o_hint": 32 * q + 64 * m}
            want["o_off"] = al16(want["o_hint"] + 4 * m)
            want["o_sb"] = want["o_off"] + 8 * k
            want["o_kb"] = want["o_sb"] + 8 * (k + 1)
            want["o_len"] = want["o_kb"] + 8 * (k + 1)
            want["o_kind"] = want["o_len"] + 4 * k
            want["o_body"] = al16(want["o_kind"] + k)
            want["p_bytes"] = want["o_body"] + max(bytes_, 16)
            want["o_cb"] = al16(want["p_bytes"])
            want["o_gb"] = want["o_cb"] + 8 * (k + 1)
            want["o_need"] = want["o_gb"] + 8 * (nc + 1)
            want["o_gw"] = want["o_need"] + 4 * nc
            want["o_gk"] = want["o_gw"] + 4 * ng
            want["o_gt"] = want["o_gk"] + 4 * ng
            want["o_sl"] = want["o_gt"] + ng
            want["bytes"] = al16(want["o_sl"] + (m if with_len else 0) + 1)
            assert {x: c[x] for x in want} == want
            h = np.full(c["bytes"] + 64, 0xCD, np.uint8)
            chunk = np.asarray([c[x] for x in PLAN_WORDS], np.uint64)
            stage.hs_check_pack(P(s["bodies"]), P(s["off"]), P(s["len"]), P(s["kind"]), nb, P(sb), P(s["hint"]),
                                P(s["sig"]), P(kb), P(s["key"]), P(sl) if with_len else None, P(cb),
                                P(s["check_needed"]), P(gb), P(s["signer_type"]), P(s["signer_weight"]),
                                P(s["signer_key"]), P(chunk), P(h))
            assert (h[c["bytes"]:] == 0xCD).all()  # nothing past the plan
            assert np.array_equal(h[:32 * q], s["key"][c["k0"]:c["k1"]].ravel())
            assert np.array_equal(h[c["o_sig"]:c["o_hint"]], s["sig"][c["s0"]:c["s1"]].ravel())
            assert np.array_equal(h[c["o_hint"]:c["o_hint"] + 4 * m], s["hint"][c["s0"]:c["s1"]].ravel())
            u64 = lambda a, b: h[a:b].view(np.uint64)  # noqa: E731
            assert np.array_equal(u64(c["o_sb"], c["o_kb"]), sb[c["b0"]:c["b1"] + 1] - np.uint64(c["s0"]))
            assert np.array_equal(u64(c["o_kb"], c["o_len"]), kb[c["b0"]:c["b1"] + 1] - np.uint64(c["k0"]))
            assert np.array_equal(u64(c["o_cb"], c["o_gb"]), cb[c["b0"]:c["b1"] + 1] - np.uint64(c["c0"]))
            assert np.array_equal(u64(c["o_gb"], c["o_need"]), gb[c["c0"]:c["c1"] + 1] - np.uint64(c["g0"]))
            assert np.array_equal(h[c["o_need"]:c["o_gw"]].view(np.int32), s["check_needed"][c["c0"]:c["c1"]])
            assert np.array_equal(h[c["o_gw"]:c["o_gk"]].view(np.uint32), s["signer_weight"][c["g0"]:c["g1"]])
            assert np.array_equal(h[c["o_gk"]:c["o_gt"]].view(np.uint32),
                                  s["signer_key"][c["g0"]:c["g1"]] - np.uint32(c["k0"]))
            assert np.array_equal(h[c["o_gt"]:c["o_sl"]], s["signer_type"][c["g0"]:c["g1"]])
            if with_len:
                assert np.array_equal(h[c["o_sl"]:c["o_sl"] + m], s["sig_len"][c["s0"]:c["s1"]])
            boff = u64(c["o_off"], c["o_sb"])
            for j in range(k):
                t = c["b0"] + j
                o, ln = c["o_body"] + int(boff[j]), int(s["len"][t])
                assert int(boff[j]) % 16 == 0
                assert np.array_equal(h[o:o + ln], s["bodies"][int(s["off"][t]):int(s["off"][t]) + ln])


# ------------------------------------------------ host mirror (prefetch 5)
class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    st = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(st))
    return st


def _gpu(sv):
    try:
        return sv.device_count() > 0
    except sv.SigVerifyError:
        return False


@pytest.mark.parametrize("with_payload", [True, False])
def test_mirror_prefetch5_matches_prefetch0(sv, oracle, with_payload):
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(2, 23, tp.pysign_signer(oracle), with_payload=with_payload)

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch, for_apply=for_apply)

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all(), ref["code"]
    assert eb.txBAD_AUTH in ref["code"] and eb.txSUCCESS in ref["code"]
    _stats(host)
    res, checks, ch, fb = call(5)
    st = _stats(host)
    assert (res == ref).all()
    assert (ch == ch0).all() and (fb == fb0).all()
    assert (ch == s["contents_hash"]).all() and (fb == s["fee_bump_hash"]).all()
    # source at LOW + one operation per envelope, and the fee bumps' outer checks
    assert checks == 2 * s["n"] + s["kinds"].count("fee_bump")
    # without a GPU the one engine call fails and is re-run on the CPU form
    assert (st.fallbacks == 0 and st.gpu_batches == 1) if _gpu(sv) else st.fallbacks == 1
    assert (call(5, for_apply=1)[0] == call(0, for_apply=1)[0]).all()
    # protocol 7: every check is true without the engine
    r7 = eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 7, s["bodies"],
                                   s["ebody"], prefetch=5)
    r70 = eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 7, s["bodies"],
                                    s["ebody"], prefetch=0)
    assert (r7[0] == r70[0]).all() and (r7[2] == ch0).all()


def test_mirror_prefetch5_special_envelopes(sv, oracle):
    """A fee bump with an unused outer signature (txBAD_AUTH_EXTRA), operations
    whose source account is missing (with and without that key's signature), a
    HASH_X signer with a short preimage, extra signers, a missing transaction
    source, a surplus inner signature, and two envelopes beyond the engine's
    limits (65 signatures; a fee bump whose inner transaction has 65), which
    are checked on the host, they alone."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    rng = np.random.default_rng(77)
    A, F, X, E, G = range(5)
    seeds = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    preimage = b"hash-x preimage of 29 bytes..."[:29]
    hxkey = hashlib.sha256(preimage).digest()
    # (kind, what)
    names = ("bump_extra_sig", "op_no_account_signed", "op_no_account_unsigned", "hashx", "extra_signer",
             "extra_signer_missing", "no_source", "surplus_sig", "bump_ok", "over_limit", "bump_over_limit")
    blob, ebody, jobs, plans = bytearray(), np.zeros(len(names), eb.ENVELOPE_BODY), [(k, bytes(32)) for k in range(5)], []

    def new_body():
        b = bytes(rng.integers(0, 256, 4 * int(rng.integers(25, 60)), dtype=np.uint8))
        off = len(blob)
        blob.extend(b)
        return off, b

    def job(k, msg):
        jobs.append((k, msg))
        return len(jobs) - 1

    for t, name in enumerate(names):
        off, body = new_body()
        ebody[t]["off"], ebody[t]["len"], ebody[t]["kind"] = off, len(body), tp.V1
        inner = tp.contents_hash(tp.V1, body)
        plan = {"inner": inner, "outer": bytes(32), "rows": [job(A, inner)], "outer_rows": []}
        if name.startswith("bump"):
            ooff, obody = new_body()
            ebody[t]["outer_off"], ebody[t]["outer_len"] = ooff, len(obody)
            plan["outer"] = tp.contents_hash(tp.FEE_BUMP, obody)
            plan["outer_rows"] = [job(F, plan["outer"])] + ([job(A, plan["outer"])] if name == "bump_extra_sig" else [])
        if name == "op_no_account_signed":
            plan["rows"].append(job(X, inner))
        if name == "extra_signer":
            plan["rows"].append(job(E, inner))
        if name == "surplus_sig":
            plan["rows"].append(job(G, inner))
        if name == "no_source":
            plan["rows"] = [job(X, inner)]
        plans.append(plan)
    pk, sig = tp.pysign_signer(oracle)(seeds[[k for k, _ in jobs]],
                                       np.array([np.frombuffer(m, np.uint8) for _, m in jobs], np.uint8))
    keys = [pk[k].tobytes() for k in range(5)]
    hx = lambda k: keys[k].hex()  # noqa: E731
    dsig = lambda row: {"hint": pk[row].tobytes()[28:].hex(), "sig": sig[row].tobytes().hex()}  # noqa: E731
    accounts = [{"id": hx(A), "thresholds": [1, 0, 0, 0], "signers": []},
                {"id": hx(F), "thresholds": [1, 0, 0, 0], "signers": []},
                # no master key: a HASH_X signer alone
                {"id": hx(G), "thresholds": [0, 1, 1, 1], "signers": [{"type": 2, "key": hxkey.hex(), "weight": 1}]}]
    sets = {}
    for which in ("envs", "envs_blank"):
        es = ev.EnvelopeSet()
        for a in accounts:
            es.account(a)
        for t, name in enumerate(names):
            pl = plans[t]
            inner, outer = (pl["inner"], pl["outer"]) if which == "envs" else (b"\xaa" * 32, b"\xbb" * 32)
            sigs = [dsig(r) for r in pl["rows"]]
            source, ops, extra, fee = hx(A), [{"level": 2}], (), None
            if name.startswith("op_no_account"):
                ops = [{"level": 1}, {"level": 2, "source": hx(X)}]
            if name == "hashx":
                source = hx(G)
                sigs = [{"hint": hxkey[28:].hex(), "sig": preimage.hex()}]
            if name.startswith("extra_signer"):
                extra = [{"type": 0, "key": hx(E), "weight": 1}]
            if name == "no_source":
                source = hx(X)
            if name.endswith("over_limit"):  # the signer's signature last, behind 64 that match nothing
                sigs = [{"hint": "00000000", "sig": bytes([i]).hex() * 64} for i in range(64)] + sigs
            if name.startswith("bump"):
                fee = {"hash": outer.hex(), "fee_source": hx(F), "sigs": [dsig(r) for r in pl["outer_rows"]]}
            es.envelope(source, inner.hex(), sigs, ops, extra=extra, fee_bump=fee)
        sets[which] = es.arrays()
    n, bodies = len(names), np.frombuffer(bytes(blob), np.uint8).copy()

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, sets["envs_blank"][0], *sets["envs"][1:], n, len(accounts), 21, bodies,
                                         ebody, prefetch=prefetch, for_apply=for_apply)

    ref = call(0)
    code = dict(zip(names, ref[0]["code"].tolist()))
    assert code == {"bump_extra_sig": -10, "op_no_account_signed": 0, "op_no_account_unsigned": -1, "hashx": 0,
                    "extra_signer": 0, "extra_signer_missing": -6, "no_source": -8, "surplus_sig": -10, "bump_ok": 1,
                    "over_limit": -10, "bump_over_limit": -13}
    t = names.index("op_no_account_unsigned")
    assert (int(ref[0]["failed_op"][t]), int(ref[0]["op_code"][t])) == (1, -1)
    _stats(host)
    for for_apply in (0, 1):
        want, got = call(0, for_apply), call(5, for_apply)
        assert (got[0] == want[0]).all(), (got[0], want[0])
        assert (got[2] == want[2]).all() and (got[3] == want[3]).all()
        # every envelope but the two over the limits was decided by the engine, in `names` order: source + one per
        # operation (+ the extra signers' check), 1 + 2 for a fee bump, none without a source; of bump_over_limit
        # only the outer check went in before its inner transaction was refused
        assert got[1] == 3 + 3 + 3 + 2 + 3 + 3 + 0 + 2 + 3 + 0 + 1
    st = _stats(host)
    assert (st.gpu_batches, st.fallbacks) == ((2, 0) if _gpu(sv) else (0, 2))  # one engine call per prefetch-5 call


# ------------------------------------------------ host code under sanitizers
def test_host_code_under_sanitizers(tmp_path):
    """tests/native/txcheck_core.cpp (its own main) + the CPU path, built with
    ASan and UBSan and run directly: nothing is loaded into Python."""
    exe = str(tmp_path / "txcheck_core")
    # (the sanitizer runtimes linked statically: the program needs nothing preloaded)
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas", "-o", exe,
           os.path.join(HERE, "native", "txcheck_core.cpp"),
           os.path.join(REPO, "stellar-core_amd", "csrc", "sv_cpu.cpp"), "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "txcheck_core ok" in r.stdout, r.stdout[-4000:]
