"""The ED25519_SIGNED_PAYLOAD stage decided on the GPU: the payload pairing
kernels of sv_txpair.hip, the second (variable-length) verify launch and the
fourth pass of the check kernels behind sv_ed25519_check_txbodies / _device with
the payload tables -- the edge cases, the pairing's and the check kernel's block
seams, unvalidated device tables, the path without candidates, two slots, a
multi-chunk host-buffer call and the host mirror's prefetch 6.  Expectations come from the Python replay of
txpayload_pool.py (by construction for the large GPU-signed set) and must also
equal the _cpu form; every comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import envelope_bodies as eb
import txbodies_pool as tp
import txchecks_pool as cp
import txpairs_pool as pp
import txpayload_pool as pl
import txset_gen as tg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PAIR_BLOCK = 256   # lanes (bodies) per workgroup of the pairing kernels
CHECK_BLOCK = 256  # lanes (checks) per workgroup of the check kernels
GUARD = 16         # guard bytes on each side of every output of the device-resident call
SP, ED = pl.SP, pl.ED


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    lib = sv.load_library()
    assert lib.sv_check_block() == CHECK_BLOCK and lib.sv_pair_block() == PAIR_BLOCK
    return torch.device("cuda", 0)


@pytest.fixture(params=["throughput", "quad", "default"])
def kpath(sv, request):
    """The throughput path forced in both geometries, and the default path."""
    if request.param == "default":
        yield
        return
    prev = sv.set_kernel_path(sv.PATH_THROUGHPUT)
    prev_dbg = sv.set_debug_flags({"throughput": sv.DBG_NO_QUAD, "quad": sv.DBG_QUAD}[request.param])
    yield
    sv.set_kernel_path(prev)
    sv.set_debug_flags(prev_dbg)


def _host(sv, s, protocol=21, tables=True, **kw):
    return sv.check_txbodies(*pl.args(s, tables), sig_len=s["sig_len"], protocol_version=protocol,
                             **(pl.tables(s) if tables else {}), **kw)


def _cpu(sv, s, protocol=21, tables=True):
    return sv.check_txbodies_cpu(*pl.args(s, tables), sig_len=s["sig_len"], protocol_version=protocol,
                                 **(pl.tables(s) if tables else {}))


def _device_call(sv, dev, s, protocol=21, tables="present", over=None):
    """sv_ed25519_check_txbodies_device over the set as it is packed -> (ok,
    weight, used, digests).  Every input array is allocated at its exact size;
    the outputs sit between guard bytes that must stay untouched.  tables:
    "present", "absent" (the plain struct, the skip's key indices), "empty"
    (pkey_begin of zeros, n_pkeys 0) or "null" (pkey_begin NULL).  `over`
    overrides arrays (and n_pkeys) with unvalidated ones."""
    t = dict(s)
    if tables != "present":
        t["signer_key"] = s["signer_key_skip"]
    t.update(over or {})
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    pad = lambda a, w: a if len(a) else np.zeros((1, w), np.uint8)  # noqa: E731
    one = lambda a, dt: a if len(a) else np.zeros(1, dt)  # noqa: E731
    nb, ns, nk, nc, ng = s["nb"], s["ns"], s["nk"], s["nc"], s["ng"]
    d = {k: up(t[k]) for k in ("bodies", "off", "len", "kind", "sig_begin", "key_begin", "check_begin", "signer_begin")}
    d["hint"], d["sig"], d["key"] = up(pad(t["hint"], 4)), up(pad(t["sig"], 64)), up(pad(t["key"], 32))
    d["need"] = up(one(t["check_needed"], np.int32))
    d["gt"], d["gw"] = up(one(t["signer_type"], np.uint8)), up(one(t["signer_weight"], np.uint32))
    d["gk"], d["sl"] = up(one(t["signer_key"], np.uint32)), up(one(t["sig_len"], np.uint8))
    kw = {}
    if tables == "present":
        d["qb"], d["qk"], d["qp"] = up(t["pkey_begin"]), up(pad(t["pkey"], 32)), up(pad(t["pkey_payload"], 64))
        d["ql"] = up(one(t["pkey_len"], np.uint8))
        kw = dict(d_pkey_begin=d["qb"].data_ptr(), d_pkey=d["qk"].data_ptr(), d_pkey_payload=d["qp"].data_ptr(),
                  d_pkey_len=d["ql"].data_ptr(), n_pkeys=t.get("n_pkeys", s["nq"]))
    elif tables == "empty":
        d["qb"] = up(np.zeros(nb + 1, np.uint64))
        kw = dict(d_pkey_begin=d["qb"].data_ptr(), n_pkeys=0)
    elif tables == "null":
        kw = dict(n_pkeys=0)
    outs = [torch.full((2 * GUARD + w * max(nc, 1),), 0xA5, dtype=torch.uint8, device=dev) for w in (1, 4, 8)]
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sv.check_txbodies_device(0, tp.NETWORK_ID, d["bodies"].data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(),
                             d["kind"].data_ptr(), nb, d["sig_begin"].data_ptr(), d["hint"].data_ptr(),
                             d["sig"].data_ptr(), ns, d["key_begin"].data_ptr(), d["key"].data_ptr(), nk,
                             d["check_begin"].data_ptr(), d["need"].data_ptr(), nc, d["signer_begin"].data_ptr(),
                             d["gt"].data_ptr(), d["gw"].data_ptr(), d["gk"].data_ptr(), ng,
                             outs[0].data_ptr() + GUARD, outs[1].data_ptr() + GUARD, outs[2].data_ptr() + GUARD,
                             d_sig_len=d["sl"].data_ptr(), protocol_version=protocol, d_digests=t_dig.data_ptr(),
                             stream=stream, **kw)
    torch.cuda.synchronize(dev)
    res = []
    for o, w, dt in zip(outs, (1, 4, 8), (np.uint8, np.uint32, np.uint64)):
        h = o.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + w * nc:] == 0xA5).all(), "a write outside the output array"
        res.append(h[GUARD:GUARD + w * nc].copy().view(dt))
    return res[0], res[1], res[2], t_dig.cpu().numpy()


@pytest.fixture(scope="module")
def edge(sv, dev, oracle):
    """The edge cases and a random pool in one batch, GPU-signed; shared and left unchanged."""
    bld = pl.PBuilder(3)
    cases = pl.edge_cases(bld)
    pl.random_pool(bld, 150)
    s = bld.finish(tp.device_signer(sv), oracle)
    verify = cp.oracle_verify(oracle)
    return s, cases, {p: pl.expected(s, verify, p) for p in (21, 9)}, pl.expected(s, verify, tables=False)


def test_edge_cases_and_pool_host_and_device(sv, dev, edge, kpath):
    s, cases, want, skip = edge
    assert (want[21][0] != skip[0]).any()
    for protocol in (21, 9):
        w = want[protocol]
        cp.assert_equal(_cpu(sv, s, protocol), w, s)
        cp.assert_equal(_host(sv, s, protocol, device=0), w, s)
        cp.assert_equal(_device_call(sv, dev, s, protocol), w, s)
    ok, weight, used, _ = _device_call(sv, dev, s)
    for name, (c0, hand) in cases.items():
        got = [(int(ok[c0 + i]), int(weight[c0 + i]), int(used[c0 + i])) for i in range(len(hand))]
        assert got == hand, name
    # the tables absent: the skip, on the host form and the device form
    cp.assert_equal(_host(sv, s, tables=False, device=0), skip, s)
    cp.assert_equal(_device_call(sv, dev, s, tables="absent"), skip, s)


def _seam_set(sv, oracle, nb, checks_per_body=None, force=()):
    """nb bodies of a few bytes: a payload candidate in about one body of seven,
    always in the first and last body of a 256-body tile, runs of bodies with
    none; a body has 0..2 signatures (ed25519, or over its candidate's 32-byte
    payload, some corrupted) and checks_per_body(t) checks (default 1); the
    bodies of `force` have a candidate and a signature over its payload."""
    bld = pl.PBuilder(900 + nb)
    rng = bld.rng
    for t in range(nb):
        b = bld.body(length=int(rng.integers(0, 12)))
        seed = 1 + t % 4
        edge_of_tile = t % PAIR_BLOCK in (0, PAIR_BLOCK - 1) or t == nb - 1
        has = edge_of_tile or t in force or (t % 16 >= 11 and rng.random() < 0.45)  # (runs of ten bodies without)
        signers = []
        if t % 3 == 0:
            signers.append((ED, 1, b.key_ed(seed)))
            if t % 2 == 0:
                b.sig_ed(seed)
        if has:
            payload = pl.payload_of(32, t % 3)
            signers.append((SP, 2, b.pkey(seed, payload)))
            if t % 5 != 4 or t in force:
                b.sig_payload(seed, payload, corrupt=t % 11 == 3)
        for c in range(1 if checks_per_body is None else checks_per_body(t)):
            b.check(1 + (t + c) % 3, signers[::-1] if c % 2 else signers)
    return bld.finish(tp.device_signer(sv), oracle)


@pytest.mark.parametrize("nb", [1, 255, 256, 257, 513])
def test_payload_pairing_seams(sv, dev, oracle, nb):
    """(the payload pairing reuses sv_pair_scan_kernel, whose second level the
    65 537-body case of test_gpu_txpairs.py covers)"""
    s = _seam_set(sv, oracle, nb)
    has = np.diff(s["pkey_begin"].astype(np.int64)) > 0
    assert has[0] and has[-1] and s["ns"] < 1000
    if nb > 16:
        assert 0.08 < has.mean() < 0.25 and not has[1:11].any()
    want = pl.expected(s, cp.oracle_verify(oracle))
    if nb > 1:
        assert want[0].any() and not want[0].all()
    cp.assert_equal(_cpu(sv, s), want, s)
    cp.assert_equal(_host(sv, s, device=0), want, s)
    cp.assert_equal(_device_call(sv, dev, s), want, s)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_check_block_seams(sv, dev, oracle, n):
    """n checks; the checks of a body with a payload signer straddle the 256-check boundary."""
    counts = cp.seam_counts(n)
    cb = np.concatenate([[0], np.cumsum(counts)])
    across = int(np.searchsorted(cb, CHECK_BLOCK, side="right")) - 1  # the body of check 256, if there is one
    s = _seam_set(sv, oracle, len(counts), checks_per_body=lambda t: counts[t], force=(across,))
    assert s["nc"] == n and (s["check_begin"].astype(np.int64) == cb).all()
    if n > CHECK_BLOCK:
        assert cb[across] < CHECK_BLOCK < cb[across + 1]
        c = int(cb[across])
        g0, g1 = int(s["signer_begin"][c]), int(s["signer_begin"][c + 1])
        assert (s["signer_type"][g0:g1] == 3).any()  # a payload check on each side of the boundary
    want = pl.expected(s, cp.oracle_verify(oracle))
    cp.assert_equal(_cpu(sv, s), want, s)
    cp.assert_equal(_host(sv, s, device=0), want, s)
    cp.assert_equal(_device_call(sv, dev, s), want, s)


def test_device_form_clamps_unvalidated_payload_tables(sv, dev, oracle):
    """Tables the host forms would refuse, legal for the device-resident entry
    point and clamped by design: nothing faults, nothing is written outside the
    outputs (the guard bytes of _device_call), the affected checks are 0."""
    bld = pl.PBuilder(23)
    p = pl.payload_of(64)
    for t in range(5):
        b = bld.body(length=50 + t)
        q = b.pkey(1, p)  # the same candidate in every body
        b.pkey(2 + t % 3, pl.payload_of(32, t))
        b.sig_payload(1, p)
        b.check(1, [(SP, 1, q)])
        b.check(2, [(SP, 1, q)])
    s = bld.finish(tp.device_signer(sv), oracle)
    want = pl.expected(s, cp.oracle_verify(oracle))
    assert want[0].tolist() == [1, 0] * 5
    cp.assert_equal(_device_call(sv, dev, s), want, s)
    # a pkey_len of 200 reads as 64: the same candidate, the same results
    ln = s["pkey_len"].copy()
    ln[0::2] = 200
    cp.assert_equal(_device_call(sv, dev, s, over={"pkey_len": ln}), want, s)
    # body 2's first check names body 1's / body 3's copy of the candidate, body 4's an index far past the table
    gk = s["signer_key"].copy()
    g = lambda t: int(s["signer_begin"][int(s["check_begin"][t])])  # noqa: E731
    gk[g(2)] = int(s["pkey_begin"][1])
    gk[g(3)] = int(s["pkey_begin"][4])
    gk[g(4)] = 0xFFFFFFFF
    ok, weight, used = (x.copy() for x in want)
    for t in (2, 3, 4):
        c = int(s["check_begin"][t])
        ok[c], weight[c], used[c] = 0, 0, 0
    cp.assert_equal(_device_call(sv, dev, s, over={"signer_key": gk}), (ok, weight, used), s)
    # a pkey_begin that ends past n_pkeys: the last body's range is clamped to the table
    qb = s["pkey_begin"].copy()
    qb[-1] += np.uint64(9)
    cp.assert_equal(_device_call(sv, dev, s, over={"pkey_begin": qb}), want, s)
    # ... and an n_pkeys that cuts the last body's candidates off: its checks are 0
    ok, weight, used = (x.copy() for x in want)
    ok[-2:], weight[-2:], used[-2:] = 0, 0, 0
    cp.assert_equal(_device_call(sv, dev, s, over={"n_pkeys": int(s["pkey_begin"][4])}), (ok, weight, used), s)


def test_no_candidate_is_the_call_without_tables(sv, dev, oracle):
    """A batch without payload candidates: identical outputs with the tables
    absent, with empty tables and with a NULL pkey_begin."""
    bld = pl.PBuilder(31)
    cp.random_pool(bld, 80, max_sigs=8)
    for b in bld.bodies:  # (with tables, also empty ones, the host forms refuse a type-3 signer without a candidate)
        b.checks = [(need, [g for g in gs if g[0] != SP]) for need, gs in b.checks]
    s = bld.finish(tp.device_signer(sv), oracle)
    assert s["nq"] == 0 and not (s["signer_type"] == 3).any()
    want = cp.expected(s, cp.oracle_verify(oracle))
    ref = _device_call(sv, dev, s, tables="absent")
    cp.assert_equal(ref, want, s)
    for mode in ("empty", "null"):
        got = _device_call(sv, dev, s, tables=mode)
        for a, b in zip(ref, got):
            assert (a == b).all(), mode
    host = sv.check_txbodies(*pl.args(s, False), sig_len=s["sig_len"], device=0)
    empty = sv.check_txbodies(*pl.args(s, False), sig_len=s["sig_len"], device=0,
                              pkey_begin=np.zeros(s["nb"] + 1, np.uint64))
    for a, b, c in zip(ref, host, empty):
        assert (a == b).all() and (a == c).all()


def test_two_slots_payload_bodies_on_both_sides(sv, dev, oracle):
    bld = pl.PBuilder(8)
    for t in range(2400):
        b = bld.body(length=int(bld.rng.integers(0, 60)))
        seed = 1 + t % 4
        if t % 3 == 1:
            payload = pl.payload_of(32, t % 5)
            q = b.pkey(seed, payload)
            b.sig_payload(seed, payload, corrupt=t % 11 == 5)
            b.check(1 + t % 2, [(SP, 1 + t % 2, q)])
        else:
            k = b.key_ed(seed)
            b.sig_ed(seed, corrupt=t % 13 == 5)
            b.check(1, [(ED, 1, k)])
    s = bld.finish(tp.device_signer(sv), oracle)
    has = np.diff(s["pkey_begin"].astype(np.int64)) > 0
    assert s["ns"] == 2400 and has[:1200].any() and has[1200:].any()
    want = pl.expected(s, cp.oracle_verify(oracle))
    assert want[0].any() and not want[0].all()
    one = _host(sv, s, device=0)
    sv.set_device_map([0, 0])
    try:
        sv.set_min_shard(1000)
        assert sv.device_count() == 2
        two = _host(sv, s)
        assert sv.pinned_bytes(0) > 0 and sv.pinned_bytes(1) > 0  # both slots staged a slice
    finally:
        sv.set_min_shard(0)
        sv.set_device_map([])
    cp.assert_equal(one, want, s)
    cp.assert_equal(two, want, s)
    assert sv.device_count() >= 1


def test_multi_chunk_payload_tables_cross_the_chunk_boundary(sv, dev):
    """2^18 + 5000 single-signature bodies with one key each; every fifth
    body's signature is hinted for a payload candidate (the body's key, its
    contents hash as the payload) instead of the key, so only the payload signer
    can satisfy its check.  Keys and candidates together cross the key bound of
    a chunk (2^18) before the signatures do; the results are global."""
    nb = (1 << 18) + 5000
    s = pp.make_sparse(nb, 7, tp.device_signer(sv), PAIR_BLOCK, max_len=60, one_in=1)
    tables, want = cp.sparse_tables(s)
    assert s["ns"] == nb == s["nk"]
    T = np.arange(0, nb, 5)
    dig = np.array([np.frombuffer(tp.contents_hash(int(s["kind"][t]), pp.body(s, t)), np.uint8) for t in T], np.uint8)
    hint = s["hint"].copy()
    hint[T] = s["key"][T][:, 28:] ^ dig[:, 28:]
    pay = np.zeros((len(T), 64), np.uint8)
    pay[:, :32] = dig
    qb = np.zeros(nb + 1, np.uint64)
    qb[1:] = np.cumsum(np.isin(np.arange(nb), T))
    # every body: one check of needed 1 over [its key, ED25519]; the payload bodies' checks name the candidate too
    is_t = np.isin(np.arange(nb), T)
    per = 1 + is_t.astype(np.int64)
    gb = np.zeros(nb + 1, np.uint64)
    gb[1:] = np.cumsum(per)
    ng = int(gb[-1])
    gt, gk = np.zeros(ng, np.uint8), np.zeros(ng, np.uint32)
    gk[gb[:-1].astype(np.int64)] = np.arange(nb)
    extra = gb[:-1].astype(np.int64)[T] + 1
    gt[extra], gk[extra] = 3, np.arange(len(T))
    assert int(qb[-1]) == len(T) and nb + len(T) > (1 << 18) + (1 << 15)
    got = sv.check_txbodies(tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], hint, s["sig"],
                            s["key_begin"], s["key"], tables["check_begin"], tables["check_needed"], gb, gt,
                            np.ones(ng, np.uint32), gk, device=0, pkey_begin=qb, pkey=s["key"][T], pkey_payload=pay,
                            pkey_len=np.full(len(T), 32, np.uint8))
    assert 0 < int(want[0][T].sum()) < len(T)
    cp.assert_equal(got, want)
    # without the tables those bodies' checks cannot succeed
    gk_skip = gk.copy()
    gk_skip[extra] = T
    skip = sv.check_txbodies(tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], hint, s["sig"],
                             s["key_begin"], s["key"], tables["check_begin"], tables["check_needed"], gb, gt,
                             np.ones(ng, np.uint32), gk_skip, device=0)
    assert not skip[0][T].any() and (np.delete(skip[0], T) == np.delete(want[0], T)).all()


class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def test_mirror_prefetch6(sv, dev, oracle):
    """The generated envelope set with its signed-payload unit: prefetch 6 is ONE
    engine batch with no fallback, gives the result codes of prefetch 1 and of
    replay_envelope, and makes no single verification for the payload signers
    (no verifySig lookup, no signature beyond the engine batch's), where
    prefetch 5 looks them up one by one; with the engine failing the results
    are the same through the CPU form, with one fallback counted."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(50, 37, tp.device_signer(sv), with_payload=True)
    npay = s["kinds"].count("payload")
    assert s["n"] == 300 and npay == 50

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch, for_apply=for_apply)

    def counted(prefetch):
        host.svh_cache_clear()
        hits, misses, st = ctypes.c_uint64(), ctypes.c_uint64(), EngineStats()
        host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
        host.svh_engine_counts_ex(ctypes.byref(st))
        out = call(prefetch)
        host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
        host.svh_engine_counts_ex(ctypes.byref(st))
        return out, st, hits.value + misses.value

    ref, _, ch1, fb1 = call(1)
    assert (ref["code"] == s["expect"]).all()
    verify = cp.oracle_verify(oracle)
    want = [tg.replay_envelope(c, 21, 0, verify) for c in pl.envelope_cases(s)]
    sigs_sent = int(s["envs_blank"]["nsigs"].sum() + s["envs_blank"]["nouter"].sum())
    (res, checks, ch, fb), st, lookups = counted(6)
    for k in ("code", "inner_code", "failed_op", "op_code"):
        assert res[k].tolist() == [w[k] for w in want], k
    assert (res == ref).all() and (ch == ch1).all() and (fb == fb1).all()
    assert checks == 2 * s["n"] + s["kinds"].count("fee_bump")
    assert (st.gpu_batches, st.fallbacks, st.gpu_signatures, st.cpu_signatures, lookups) == (1, 0, sigs_sent, 0, 0)
    (res5, _, _, _), st5, lookups5 = counted(5)
    assert (res5 == ref).all() and lookups5 >= npay and st5.gpu_signatures + st5.cpu_signatures > sigs_sent
    assert (call(6, for_apply=1)[0] == call(1, for_apply=1)[0]).all()
    prev = sv.set_debug_flags(sv.DBG_FAIL)
    try:
        (res, _, ch, fb), st, lookups = counted(6)
    finally:
        sv.set_debug_flags(prev)
    assert (st.fallbacks, st.gpu_batches, lookups) == (1, 0, 0)
    assert (res == ref).all() and (ch == ch1).all() and (fb == fb1).all()
