"""One signature result per transaction body, on the GPU: the result kernels of
sv_txresult.hip through their launcher on synthetic device arrays (the quad's
stride seams, the signature-count clamp, the workgroup seams and the second
round of the scan), both decide trios against their _cpu forms on every
verify-kernel path, unvalidated device tables, two slots and a multi-chunk host
call, and the mirror's prefetch 8.  Expectations come from the numpy fold of
txresults_pool.py; every comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import envelope_bodies as eb
import test_gpu_txaccounts as ta
import txaccounts_pool as ap
import txbodies_pool as tp
import txresults_pool as rp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

B = 64      # bodies per workgroup of the result kernel (sv_txresult_block())
GUARD = 64  # guard bytes on each side of every output
SLACK = ta.SLACK


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    assert sv.load_library().sv_txresult_block() == B
    return torch.device("cuda", 0)


kpath = ta.kpath


class TxResultIn(ctypes.Structure):  # csrc/txresult.h sv_txresult_in
    _fields_ = ([(f, ctypes.c_void_p) for f in ("check_begin", "sig_begin", "check_ok", "check_used", "check_role",
                                                "body_flags")]
                + [(f, ctypes.c_uint64) for f in ("nb", "nc", "ns")])


class Guarded:
    """A device output of n bytes between GUARD bytes of 0xA5 on each side."""

    def __init__(self, dev, n):
        self.n = n
        self.t = torch.full((2 * GUARD + max(n, 1),), 0xA5, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def get(self, dtype=np.uint8):
        h = self.t.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + self.n:] == 0xA5).all(), "a write outside the output array"
        return h[GUARD:GUARD + self.n].copy().view(dtype)


def _up(dev, a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.zeros(16, np.uint8)]).copy()).to(dev)


# ----------------------------------------------------------------- 1. the launcher
def _synthetic(nb, seed):
    """nb bodies: check counts from the quad's stride seams (0, 1, 3, 4, 5, 9, 130), signature counts 0, 1, 63, 64
    and 70 (clamped to 64), check_ok of 0, 1 and 2, random marks, roles and flags; one body in three passes every
    check with every mark set, one in six passes with random marks."""
    rng = np.random.default_rng(seed)
    counts = rng.choice([0, 1, 3, 4, 5, 9, 130], nb, p=[.1, .25, .25, .15, .1, .1, .05])
    counts[:min(nb, 7)] = [0, 1, 3, 4, 5, 9, 130][:min(nb, 7)]
    sigs = rng.choice([0, 1, 63, 64, 70], nb)
    cb = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    sb = np.concatenate([[0], np.cumsum(sigs)]).astype(np.uint64)
    nc = int(cb[-1])
    mode = np.repeat(rng.integers(0, 6, nb), counts)
    ok = np.where(mode < 3, 1, rng.choice([0, 1, 1, 1, 1, 2], nc)).astype(np.uint8)
    used = rng.integers(0, 2**63, nc, dtype=np.uint64) | (rng.integers(0, 2, nc, dtype=np.uint64) << np.uint64(63))
    used[mode < 2] = np.uint64(2**64 - 1)
    return dict(nb=nb, nc=nc, ns=int(sb[-1]), cb=cb, sb=sb, ok=ok, used=used,
                role=rng.integers(0, 2, nc).astype(np.uint8), flags=(rng.random(nb) < 0.25).astype(np.uint8))


def _launch(sv, dev, s, want_fail=True, bad_cap=None, want_n=True):
    """sv_launch_txresult over the set -> (code, fail or None, the whole bad buffer or None, n_bad or None)."""
    lib = sv.load_library()
    lib.sv_launch_txresult.restype = ctypes.c_int
    lib.sv_launch_txresult.argtypes = [ctypes.POINTER(TxResultIn)] + [ctypes.c_void_p] * 4 + [ctypes.c_uint64,
                                                                                               ctypes.c_void_p,
                                                                                               ctypes.c_void_p]
    nb, nc = s["nb"], s["nc"]
    d = {k: _up(dev, s[k]) for k in ("cb", "sb", "ok", "used", "role", "flags")}
    code, fail = Guarded(dev, nb), Guarded(dev, 4 * nb)
    ws = Guarded(dev, lib.sv_txresult_ws_bytes(nb))
    bad = Guarded(dev, 4 * bad_cap) if bad_cap is not None else None
    n_bad = Guarded(dev, 8)
    I = TxResultIn(d["cb"].data_ptr(), d["sb"].data_ptr(), d["ok"].data_ptr(), d["used"].data_ptr(),
                   d["role"].data_ptr(), d["flags"].data_ptr(), nb, nc, s["ns"])
    rc = lib.sv_launch_txresult(ctypes.byref(I), code.ptr, fail.ptr if want_fail else None, ws.ptr,
                                bad.ptr if bad is not None else None, bad_cap or 0, n_bad.ptr if want_n else None,
                                torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize(dev)
    ws.get()
    f = fail.get(np.uint32)
    if not want_fail:
        assert (f == 0xA5A5A5A5).all()
    n = n_bad.get(np.uint64)
    if not want_n:
        assert int(n[0]) == 0xA5A5A5A5A5A5A5A5
    return code.get(), f if want_fail else None, bad.get(np.uint32) if bad is not None else None, \
        int(n[0]) if want_n else None


@pytest.mark.parametrize("nb", [1, B - 1, B, B + 1, 256 * B, 256 * B + 1])
def test_launcher_against_the_numpy_fold(sv, dev, nb):
    s = _synthetic(nb, 1000 + nb)
    want_code, want_fail = rp.fold(s["cb"], s["sb"], s["ok"], s["used"], s["role"], s["flags"])
    want_bad, n = rp.bad_list(want_code, nb)
    if nb >= B - 1:
        assert set(want_code.tolist()) == {0, 1, 2, 3} and 2 < n < nb
    # the codes alone: no list, no count (the scan and the fill are not launched)
    code, fail, _, _ = _launch(sv, dev, s, want_fail=False, want_n=False)
    assert (code == want_code).all() and fail is None
    # a count without a list
    code, fail, _, got_n = _launch(sv, dev, s)
    assert (code == want_code).all() and (fail == want_fail).all() and got_n == n
    # the whole list; a capacity below the count: entries at or past it are never written; a list without a count
    for cap, want_n in ((nb, True), (n // 2, True), (n, False)):
        code, fail, bad, got_n = _launch(sv, dev, s, bad_cap=cap, want_n=want_n)
        k = min(cap, n)
        assert (code == want_code).all() and (fail == want_fail).all() and got_n == (n if want_n else None)
        assert (bad[:k] == want_bad[:k]).all() and (bad[k:] == 0xA5A5A5A5).all()


def test_launcher_null_roles_flags_and_no_body(sv, dev):
    s = _synthetic(200, 5)
    want_code, want_fail = rp.fold(s["cb"], s["sb"], s["ok"], s["used"])
    lib = sv.load_library()
    d = {k: _up(dev, s[k]) for k in ("cb", "sb", "ok", "used")}
    code, fail, ws, n_bad = Guarded(dev, 200), Guarded(dev, 800), Guarded(dev, lib.sv_txresult_ws_bytes(200)), \
        Guarded(dev, 8)
    I = TxResultIn(d["cb"].data_ptr(), d["sb"].data_ptr(), d["ok"].data_ptr(), d["used"].data_ptr(), None, None, 200,
                   s["nc"], s["ns"])
    _launch(sv, dev, _synthetic(1, 1))  # (sets the prototype)
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert lib.sv_launch_txresult(ctypes.byref(I), code.ptr, fail.ptr, ws.ptr, None, 0, n_bad.ptr, stream) == 0
    torch.cuda.synchronize(dev)
    assert (code.get() == want_code).all() and (fail.get(np.uint32) == want_fail).all()
    assert int(n_bad.get(np.uint64)[0]) == int((want_code != 0).sum())
    # no body: only the count is written
    I.nb = 0
    n_bad = Guarded(dev, 8)
    assert lib.sv_launch_txresult(ctypes.byref(I), code.ptr, fail.ptr, ws.ptr, None, 0, n_bad.ptr, stream) == 0
    torch.cuda.synchronize(dev)
    assert int(n_bad.get(np.uint64)[0]) == 0 and (code.get() == want_code).all()


# ----------------------------------------------------------------- 2. the pipeline
@pytest.fixture(scope="module")
def pool(sv, dev, oracle):
    """The by-account edge cases, a random pool of 300 bodies and the constructed bodies, GPU-signed, with the
    results of both _cpu forms; shared and left unchanged."""
    bld = rp.RBuilder(5)
    ap.edge_cases(bld)
    ap.random_pool(bld, 300)
    rp.assign(bld, 99)
    cases = rp.code_cases(bld)
    s = bld.finish(tp.device_signer(sv), oracle)
    want = {}
    for protocol in (21, 9):
        want[protocol] = sv.decide_txbodies_accounts_cpu(*rp.args(s), protocol_version=protocol,
                                                         **rp.kwargs(s, want_checks=True, bad_cap=s["nb"]))
        a, kw = rp.explicit(s)
        e = sv.decide_txbodies_cpu(*a, protocol_version=protocol, want_checks=True, bad_cap=s["nb"], **kw)
        for x, y in zip(want[protocol], e):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        assert set(want[protocol].body_code.tolist()) == {0, 1, 2, 3}
    return s, cases, want


ACCT_INPUTS = dict(ta.DEVICE_INPUTS, check_role=("check_role", 1), body_flags=("body_flags", 1))
EXPLICIT_INPUTS = {"bodies": ("bodies", 1), "off": ("off", 8), "len": ("len", 4), "kind": ("kind", 1),
                   "sig_begin": ("sig_begin", 8), "hint": ("hint", 4), "sig": ("sig", 64), "sig_len": ("sig_len", 1),
                   "key_begin": ("key_begin", 8), "key": ("key", 32), "check_begin": ("check_begin", 8),
                   "check_needed": ("check_needed", 4), "signer_begin": ("signer_begin", 8),
                   "signer_type": ("signer_type", 1), "signer_weight": ("signer_weight", 4),
                   "signer_key": ("signer_key", 4), "pkey_begin": ("pkey_begin", 8), "pkey": ("pkey", 32),
                   "pkey_payload": ("pkey_payload", 64), "pkey_len": ("pkey_len", 1),
                   "check_role": ("check_role", 1), "body_flags": ("body_flags", 1)}


def _decide_device(sv, dev, s, form="accounts", protocol=21, over=None, want_checks=True, bad_cap=None):
    """The device-resident decide call over the set -> sv.TxResults.  Every input sits between SLACK rows of 0xEE
    sentinels and must come back as it went up; every output sits between guard bytes that must stay untouched.
    `over` replaces arrays with unvalidated ones (the counts stay the set's)."""
    t = dict(s)
    t.update(over or {})
    inputs = ACCT_INPUTS if form == "accounts" else EXPLICIT_INPUTS
    bufs, sent = {}, {}
    for name, (key, row) in inputs.items():
        data = np.ascontiguousarray(t[key]).view(np.uint8).reshape(-1)
        h = np.concatenate([np.full(SLACK * row, 0xEE, np.uint8), data, np.full(SLACK * row, 0xEE, np.uint8)])
        sent[name] = h
        bufs[name] = torch.from_numpy(h.copy()).to(dev)
    p = lambda name: bufs[name].data_ptr() + SLACK * inputs[name][1]  # noqa: E731
    nb, ns, nc = s["nb"], s["ns"], s["nc"]
    code, fail, n_bad = Guarded(dev, nb), Guarded(dev, 4 * nb), Guarded(dev, 8)
    ok, weight, used = Guarded(dev, nc), Guarded(dev, 4 * nc), Guarded(dev, 8 * nc)
    bad = Guarded(dev, 4 * bad_cap) if bad_cap is not None else None
    dig = Guarded(dev, 32 * nb)
    res = sv.results_desc(p("check_role"), p("body_flags"), code.ptr, fail.ptr, ok.ptr if want_checks else 0,
                          weight.ptr if want_checks else 0, used.ptr if want_checks else 0,
                          bad.ptr if bad_cap else 0, bad_cap or 0, n_bad.ptr)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if form == "accounts":
        sv.decide_txbodies_accounts_device(
            0, tp.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"), ns,
            p("acct_key"), p("acct_thresholds"), p("asigner_begin"), p("asigner_type"), p("asigner_weight"),
            p("asigner_key"), p("asigner_payload"), p("apayload"), p("apayload_len"), s["na"], s["nas"], s["npay"],
            p("bacct_begin"), p("bacct"), s["ne"], p("check_begin"), p("check_acct"), p("check_level"),
            p("check_needed"), nc, res, d_sig_len=p("sig_len"), protocol_version=protocol, d_digests=dig.ptr,
            stream=stream)
    else:
        sv.decide_txbodies_device(
            0, tp.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"), ns,
            p("key_begin"), p("key"), s["nk"], p("check_begin"), p("check_needed"), nc, p("signer_begin"),
            p("signer_type"), p("signer_weight"), p("signer_key"), s["ng"], res, d_sig_len=p("sig_len"),
            protocol_version=protocol, d_digests=dig.ptr, stream=stream, d_pkey_begin=p("pkey_begin"),
            d_pkey=p("pkey"), d_pkey_payload=p("pkey_payload"), d_pkey_len=p("pkey_len"), n_pkeys=s["nq"])
    torch.cuda.synchronize(dev)
    for name, h in sent.items():
        assert (bufs[name].cpu().numpy() == h).all(), "an input or its sentinels changed: " + name
    n = int(n_bad.get(np.uint64)[0])
    o, w, u = ok.get(), weight.get(np.uint32), used.get(np.uint64)
    if not want_checks:
        assert (o == 0xA5).all() and (u == 0xA5A5A5A5A5A5A5A5).all()
    b = bad.get(np.uint32) if bad is not None else None
    if b is not None:
        assert (b[min(n, bad_cap):] == 0xA5A5A5A5).all()
        b = b[:min(n, bad_cap)]
    return sv.TxResults(code.get(), fail.get(np.uint32), b, n, o if want_checks else None, w if want_checks else None,
                        u if want_checks else None, dig.get().reshape(nb, 32))


def _same(got, want, checks=True):
    assert (got.body_code == want.body_code).all() and (got.body_fail == want.body_fail).all()
    assert got.n_bad == want.n_bad and got.digests.tobytes() == want.digests.tobytes()
    if got.bad_body is not None:
        assert (got.bad_body == want.bad_body[:len(got.bad_body)]).all()
    if checks:
        assert got.check_ok.tobytes() == want.check_ok.tobytes()
        assert got.check_weight.tobytes() == want.check_weight.tobytes()
        assert got.check_used.tobytes() == want.check_used.tobytes()


def _decide_host(sv, s, form="accounts", protocol=21, **kw):
    if form == "accounts":
        return sv.decide_txbodies_accounts(*rp.args(s), protocol_version=protocol, **rp.kwargs(s, **kw))
    a, k = rp.explicit(s)
    k.update(kw)
    return sv.decide_txbodies(*a, protocol_version=protocol, **k)


@pytest.mark.parametrize("form", ["accounts", "explicit"])
def test_host_and_device_forms_equal_the_cpu_form(sv, dev, pool, kpath, form):
    s, cases, want = pool
    for protocol in (21, 9):
        w = want[protocol]
        _same(_decide_host(sv, s, form, protocol, device=0, want_checks=True, bad_cap=s["nb"]), w)
        _same(_decide_device(sv, dev, s, form, protocol, bad_cap=s["nb"]), w)
    # no per-check output: the same codes, the check arrays untouched
    got = _decide_host(sv, s, form, device=0)
    _same(got, want[21], checks=False)
    assert got.check_ok is None
    got = _decide_device(sv, dev, s, form, want_checks=False, bad_cap=3)
    _same(got, want[21], checks=False)
    assert len(got.bad_body) == 3
    for name, (t, code, fail) in cases.items():
        assert (int(got.body_code[t]), int(got.body_fail[t])) == (code, fail), name


def test_requested_check_outputs_equal_the_twin_device_call(sv, dev, pool):
    s = pool[0]
    for protocol in (21, 9):
        twin = ta._device_call(sv, dev, s, protocol)
        got = _decide_device(sv, dev, s, "accounts", protocol)
        for x, y in zip((got.check_ok, got.check_weight, got.check_used, got.digests), twin):
            assert x.tobytes() == y.tobytes()
        code, fail = rp.fold(s["check_begin"], s["sig_begin"], twin[0], twin[2], s["check_role"], s["body_flags"])
        assert (got.body_code == code).all() and (got.body_fail == fail).all()


# ----------------------------------------------------------------- 3. unvalidated device tables
@pytest.mark.parametrize("form", ["accounts", "explicit"])
def test_device_form_clamps_unvalidated_tables(sv, dev, pool, form):
    """What the host forms refuse is legal for the device-resident forms: CSR arrays that end past their tables
    are clamped, a role of 7 reads as OP and flag bits other than bit 0 are ignored.  The valid equivalent's
    results are the expectation; _decide_device asserts that nothing but the outputs is written."""
    s, _, want = pool
    role = s["check_role"].copy()
    role[role == 1] = 7
    flags = (s["body_flags"] | 0xFE).astype(np.uint8)
    cb, sb = s["check_begin"].copy(), s["sig_begin"].copy()
    cb[-1] += np.uint64(9)
    sb[-1] += np.uint64(5)
    assert (role == 7).any() and (flags == 0xFF).any() and (flags == 0xFE).any()
    for over in ({"check_role": role}, {"body_flags": flags}, {"check_begin": cb, "sig_begin": sb},
                 {"check_role": role, "body_flags": flags, "check_begin": cb, "sig_begin": sb}):
        _same(_decide_device(sv, dev, s, form, over=over, bad_cap=s["nb"]), want[21])


# ----------------------------------------------------------------- 4. slots and chunks
def _big(sv, nb, na, extra, sig_every):
    """test_gpu_txaccounts' vectorised set with roles (one check in three an operation's) and flags (one body in
    five SKIP_UNUSED); -> (set, (code, fail) by the fold of the check results it has by construction)."""
    s, (ok, _, used) = ta._big_set(sv, nb, na, extra, sig_every)
    s["check_role"] = (np.arange(s["nc"]) % 3 == 1).astype(np.uint8)
    s["body_flags"] = (np.arange(nb) % 5 == 0).astype(np.uint8)
    return s, rp.fold(s["check_begin"], s["sig_begin"], ok, used, s["check_role"], s["body_flags"])


def test_two_slots_codes_and_bad_list_are_global(sv, dev):
    s, (code, fail) = _big(sv, 2400, 50, 2, 1)
    bad, n = rp.bad_list(code, 2400)
    assert set(code.tolist()) == {0, 1, 2, 3} and (bad < 1200).any() and (bad >= 1200).any()
    one = _decide_host(sv, s, device=0, bad_cap=2400)
    sv.set_device_map([0, 0])
    try:
        sv.set_min_shard(1000)
        assert sv.device_count() == 2
        two = _decide_host(sv, s, bad_cap=2400, want_checks=True)
        assert sv.pinned_bytes(0) > 0 and sv.pinned_bytes(1) > 0  # both slots staged a slice
    finally:
        sv.set_min_shard(0)
        sv.set_device_map([])
    for got in (one, two):
        assert (got.body_code == code).all() and (got.body_fail == fail).all()
        assert got.n_bad == n and (got.bad_body == bad).all()
    twin = ta._host(sv, s, device=0)
    assert two.check_ok.tobytes() == twin[0].tobytes() and two.check_used.tobytes() == twin[2].tobytes()
    assert two.digests.tobytes() == twin[3].tobytes() == one.digests.tobytes()


def test_multi_chunk_codes_and_bad_list_are_global(sv, dev):
    """The shape of test_multi_chunk_account_in_first_and_last_chunk: 61 expanded key rows per body cross a chunk's
    key bound three times; codes, body-local fail indices and the ascending bad list span the chunks."""
    nb = 12000
    s, (code, fail) = _big(sv, nb, 7, 60, 2)
    bad, n = rp.bad_list(code, nb)
    assert 61 * nb > 2 * (1 << 18) and set(code.tolist()) == {0, 1, 2, 3}
    got = _decide_host(sv, s, device=0, bad_cap=n - 1)
    assert (got.body_code == code).all() and (got.body_fail == fail).all()
    assert got.n_bad == n and (got.bad_body == bad[:n - 1]).all() and bad[-1] > nb - 100 and bad[0] < 100
    dev_got = _decide_device(sv, dev, s, "accounts", want_checks=False, bad_cap=n)
    assert (dev_got.body_code == code).all() and (dev_got.bad_body == bad).all() and dev_got.n_bad == n
    assert dev_got.digests.tobytes() == got.digests.tobytes()


# ----------------------------------------------------------------- 5. the mirror
def test_mirror_prefetch8(sv, dev):
    """The generated envelope set: prefetch 8 is ONE engine batch with no fallback, gives prefetch 0's results in
    both modes, walks only the failing envelopes and builds no signer list; with the engine failing the results
    are the same through the CPU form, with one fallback counted."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_signer_lists_built.restype = ctypes.c_uint64
    host.svh_decided_walks.restype = ctypes.c_uint64
    s = eb.build_set(50, 37, tp.device_signer(sv), with_payload=True)

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch, for_apply=for_apply)

    def counted(for_apply=0):
        st = ta.EngineStats()
        host.svh_engine_counts_ex(ctypes.byref(st))
        walks, built = host.svh_decided_walks(), host.svh_signer_lists_built()
        out = call(8, for_apply)
        host.svh_engine_counts_ex(ctypes.byref(st))
        return out, st, host.svh_decided_walks() - walks, host.svh_signer_lists_built() - built

    for for_apply in (0, 1):
        ref = call(0, for_apply)
        assert (ref[0]["code"] == s["expect"]).all()
        (res, checks, ch, fb), st, walks, built = counted(for_apply)
        assert (res == ref[0]).all() and (ch == ref[2]).all() and (fb == ref[3]).all()
        assert checks == 2 * s["n"] + s["kinds"].count("fee_bump")
        assert (st.gpu_batches, st.fallbacks, st.cpu_signatures, walks, built) == (1, 0, 0, 50, 0)
    prev = sv.set_debug_flags(sv.DBG_FAIL)
    try:
        (res, _, ch, fb), st, walks, built = counted()
    finally:
        sv.set_debug_flags(prev)
    ref = call(0)
    assert (st.fallbacks, st.gpu_batches, walks, built) == (1, 0, 50, 0)
    assert (res == ref[0]).all() and (ch == ref[2]).all() and (fb == ref[3]).all()
