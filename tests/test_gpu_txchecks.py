"""Signature checks decided on the GPU: the check kernel of sv_txcheck.hip behind
sv_ed25519_check_txbodies / _device -- the edge cases of the decision function,
the block and binary-search seams, the chunking (by signatures, by signers),
the slicing over two slots, unvalidated device tables and the host mirror's
prefetch 5.  Expectations come from the Python replay of txchecks_pool.py
(txset_gen.Checker per check; by construction for the large GPU-signed sets)
and must also equal the _cpu form; every comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import envelope_bodies as eb
import txbodies_pool as tp
import txchecks_pool as cp
import txpairs_pool as pp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHECK_BLOCK = 256  # lanes (checks) per workgroup of the check kernel
SEAMS = (1, 255, 256, 257, 511, 513)
GUARD = 16  # guard bytes on each side of every output of the device-resident call


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    assert sv.load_library().sv_check_block() == CHECK_BLOCK
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


def _device_call(sv, dev, s, protocol=21, sig_len=True, tables=None, digests=True):
    """sv_ed25519_check_txbodies_device over the set as it is packed -> (ok,
    weight, used, digests).  Every input array is allocated at its exact size;
    the outputs sit between guard bytes that must stay untouched.  `tables`
    overrides arrays (and the counts n_checks / n_signers) with unvalidated ones."""
    t = dict(s)
    t.update(tables or {})
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    pad = lambda a, w: a if len(a) else np.zeros((1, w), np.uint8)  # noqa: E731
    one = lambda a, dt: a if len(a) else np.zeros(1, dt)  # noqa: E731
    nb, ns, nk = s["nb"], s["ns"], s["nk"]
    nc, ng = t.get("n_checks", len(s["check_needed"])), t.get("n_signers", len(s["signer_type"]))
    d = {k: up(t[k]) for k in ("bodies", "off", "len", "kind", "sig_begin", "key_begin", "check_begin", "signer_begin")}
    d["hint"], d["sig"], d["key"] = up(pad(t["hint"], 4)), up(pad(t["sig"], 64)), up(pad(t["key"], 32))
    d["need"] = up(one(t["check_needed"], np.int32))
    d["gt"], d["gw"] = up(one(t["signer_type"], np.uint8)), up(one(t["signer_weight"], np.uint32))
    d["gk"] = up(one(t["signer_key"], np.uint32))
    d["sl"] = up(one(t["sig_len"], np.uint8)) if sig_len else None
    outs = [torch.full((2 * GUARD + w * max(nc, 1),), 0xA5, dtype=torch.uint8, device=dev) for w in (1, 4, 8)]
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sv.check_txbodies_device(0, tp.NETWORK_ID, d["bodies"].data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(),
                             d["kind"].data_ptr(), nb, d["sig_begin"].data_ptr(), d["hint"].data_ptr(),
                             d["sig"].data_ptr(), ns, d["key_begin"].data_ptr(), d["key"].data_ptr(), nk,
                             d["check_begin"].data_ptr(), d["need"].data_ptr(), nc, d["signer_begin"].data_ptr(),
                             d["gt"].data_ptr(), d["gw"].data_ptr(), d["gk"].data_ptr(), ng,
                             outs[0].data_ptr() + GUARD, outs[1].data_ptr() + GUARD, outs[2].data_ptr() + GUARD,
                             d_sig_len=d["sl"].data_ptr() if sig_len else 0, protocol_version=protocol,
                             d_digests=t_dig.data_ptr() if digests else 0, stream=stream)
    torch.cuda.synchronize(dev)
    res = []
    for o, w, dt in zip(outs, (1, 4, 8), (np.uint8, np.uint32, np.uint64)):
        h = o.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + w * nc:] == 0xA5).all(), "a write outside the output array"
        res.append(h[GUARD:GUARD + w * nc].copy().view(dt))
    return res[0], res[1], res[2], t_dig.cpu().numpy()


@pytest.fixture(scope="module")
def edge(sv, dev, oracle):
    """All the edge cases in one batch, GPU-signed; shared and left unchanged."""
    bld = cp.Builder(3)
    cases = cp.edge_cases(bld)
    s = bld.finish(tp.device_signer(sv))
    verify = cp.oracle_verify(oracle)
    return s, cases, {p: cp.expected(s, verify, p) for p in (21, 9)}


def test_edge_cases_host_and_device(sv, dev, edge, kpath):
    s, cases, want = edge
    for protocol in (21, 9):
        w = want[protocol]
        cpu = sv.check_txbodies_cpu(*cp.args(s), sig_len=s["sig_len"], protocol_version=protocol)
        cp.assert_equal(cpu, w, s)
        cp.assert_equal(sv.check_txbodies(*cp.args(s), sig_len=s["sig_len"], protocol_version=protocol, device=0), w, s)
        cp.assert_equal(_device_call(sv, dev, s, protocol), w, s)
    ok, weight, used, _ = _device_call(sv, dev, s, digests=False)  # (the engine's own digest array)
    for name, (c0, hand) in cases.items():
        got = [(int(ok[c0 + i]), int(weight[c0 + i]), int(used[c0 + i])) for i in range(len(hand))]
        assert got == hand, name


def test_sig_len_null_on_the_device(sv, dev):
    """Row 0 holds a whole valid signature whose sig_len says 63: with sig_len
    it never matches an ED25519 signer, without sig_len every row counts as 64
    bytes and it does."""
    bld = cp.Builder(5)
    b = bld.body(length=40)
    k1, k2 = b.key_ed(1), b.key_ed(2)
    b.sig_ed(1, length=63)
    b.sig_ed(2)
    b.sig_ed(1)
    b.check(2, [(cp.ED, 1, k1), (cp.ED, 1, k2)])
    s = bld.finish(tp.device_signer(sv))
    s["sig"][0] = s["sig"][2]  # (signing is deterministic: the same signature, untruncated)
    for got in (_device_call(sv, dev, s, sig_len=False), sv.check_txbodies(*cp.args(s), device=0)):
        assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == ([1], [2], [0b011])
    for got in (_device_call(sv, dev, s, sig_len=True), sv.check_txbodies(*cp.args(s), sig_len=s["sig_len"], device=0)):
        assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == ([1], [2], [0b110])


@pytest.fixture(scope="module")
def seam_sets(sv, dev, oracle):
    signer = tp.device_signer(sv)
    verify = cp.oracle_verify(oracle)
    out = {}
    for n in SEAMS:
        bld = cp.Builder(700 + n)
        cp.random_pool(bld, 0, max_sigs=6, check_counts=cp.seam_counts(n))
        s = bld.finish(signer)
        out[n] = (s, cp.expected(s, verify))
    return out


@pytest.mark.parametrize("n", SEAMS)
def test_block_and_search_seams(sv, dev, seam_sets, n):
    s, want = seam_sets[n]
    cb = s["check_begin"].astype(np.int64)
    assert s["nc"] == n and (np.diff(cb) == 0).sum() >= 2  # bodies without checks, also at the end
    if n > 3:
        assert ((np.diff(cb)[:-1] == 0) & (np.diff(cb)[1:] == 0)).any()  # a run of them
    body_of = np.searchsorted(cb, np.arange(n), side="right") - 1
    for edge in range(CHECK_BLOCK, n, CHECK_BLOCK):
        lo = edge - CHECK_BLOCK
        assert body_of[lo] != body_of[edge - 1]      # a block's first and last check: different bodies
        assert body_of[edge - 1] == body_of[edge]    # one body's checks straddle the block boundary
    if n > 1:
        assert want[0].any() and not want[0].all()
    cp.assert_equal(sv.check_txbodies_cpu(*cp.args(s), sig_len=s["sig_len"]), want, s)
    cp.assert_equal(sv.check_txbodies(*cp.args(s), sig_len=s["sig_len"], device=0), want, s)
    cp.assert_equal(_device_call(sv, dev, s), want, s)


def test_multi_chunk_by_signatures(sv, dev):
    """2^18 + 5000 single-signature bodies of 0-60 bytes with one check each:
    more than one staging chunk of signatures; the results are global."""
    nb = (1 << 18) + 5000
    s = pp.make_sparse(nb, 7, tp.device_signer(sv), CHECK_BLOCK, max_len=60, one_in=1)
    tables, want = cp.sparse_tables(s)
    assert s["ns"] == nb == len(want[0]) and 0 < int(want[0].sum()) < nb
    got = sv.check_txbodies(*cp.sparse_args(s, tables), device=0)
    cp.assert_equal(got, want)
    assert (got[3] == pp.expected_fast(s)["digests"]).all()


def test_multi_chunk_by_signers(sv, dev):
    """70000 bodies, two checks each, every check naming the body's key 16
    times: 2.24 million signers cross the signer bound of a chunk (8 x 2^18)
    while signatures, keys and checks stay below theirs (2^18 each)."""
    nb = 70000
    s = pp.make_sparse(nb, 9, tp.device_signer(sv), CHECK_BLOCK, one_in=3)
    tables, want = cp.sparse_tables(s, checks_per_body=2, signers_per_check=16)
    assert len(tables["signer_type"]) > (8 << 18) and (1 << 18) > max(s["ns"], s["nk"], len(tables["check_needed"]))
    assert 0 < int(want[0].sum()) < len(want[0])
    cp.assert_equal(sv.check_txbodies(*cp.sparse_args(s, tables), device=0), want)
    cp.assert_equal(sv.check_txbodies_cpu(*cp.sparse_args(s, tables)), want)


def _boundary_set(sv):
    """2400 signatures in 2402 bodies; an equal share ends at the edge between
    body 1199 (a signature, no check) and bodies 1200, 1201 (nothing at all)."""
    bld = cp.Builder(8)
    for t in range(2402):
        b = bld.body(length=int(bld.rng.integers(0, 200)))
        if t in (1200, 1201):
            continue
        seed = 1 + t % 5
        k = b.key_ed(seed)
        kw = b.key_wrong(seed)
        b.sig_ed(seed, corrupt=t % 11 == 5)
        if t != 1199:
            b.check(1 + t % 2, [(cp.ED, 1, kw), (cp.ED, 2, k)])
    s = bld.finish(tp.device_signer(sv))
    assert s["ns"] == 2400 and int(s["sig_begin"][1200]) == 1200
    assert int(s["check_begin"][1199]) == int(s["check_begin"][1202])
    return s


def test_two_slots_on_one_gpu_boundary_at_body_edge(sv, dev, oracle):
    s = _boundary_set(sv)
    want = cp.expected(s, cp.oracle_verify(oracle))
    assert want[0].any() and not want[0].all()
    one = sv.check_txbodies(*cp.args(s), sig_len=s["sig_len"], device=0)
    sv.set_device_map([0, 0])
    try:
        sv.set_min_shard(1000)
        assert sv.device_count() == 2
        two = sv.check_txbodies(*cp.args(s), sig_len=s["sig_len"])
        assert sv.pinned_bytes(0) > 0 and sv.pinned_bytes(1) > 0  # both slots staged a slice
    finally:
        sv.set_min_shard(0)
        sv.set_device_map([])
    cp.assert_equal(one, want, s)
    cp.assert_equal(two, want, s)  # (every digest delivered: the binding's array starts as zeros)
    for a, b in zip(one, two):
        assert (a == b).all()
    assert sv.device_count() >= 1


def test_device_form_clamps_unvalidated_tables(sv, dev, oracle):
    """Junk the host forms would refuse: a key index outside its body (the same
    key row in the neighbouring body, and an index past the array) matches
    nothing; CSR ends past their arrays are clamped; nothing is written outside
    the outputs (the guard bytes of _device_call)."""
    bld = cp.Builder(21)
    for t in range(5):
        b = bld.body(length=50 + t)
        k = b.key_ed(1)  # the same key in every body
        b.key_ed(2 + t)
        b.sig_ed(1)
        b.check(1, [(cp.ED, 1, k)])
        b.check(2, [(cp.ED, 1, k)])
    s = bld.finish(tp.device_signer(sv))
    want = cp.expected(s, cp.oracle_verify(oracle))
    assert want[0].tolist() == [1, 0] * 5
    cp.assert_equal(_device_call(sv, dev, s), want, s)
    # body 2's first check names body 1's / body 3's copy of the key, body 4's an index far past the array
    gk = s["signer_key"].copy()
    g = lambda t: int(s["signer_begin"][int(s["check_begin"][t])])  # noqa: E731
    gk[g(2)] = int(s["key_begin"][1])
    gk[g(3)] = int(s["key_begin"][4])
    gk[g(4)] = 0xFFFFFFFF
    ok, weight, used = (x.copy() for x in want)
    for t in (2, 3, 4):
        c = int(s["check_begin"][t])
        ok[c], weight[c], used[c] = 0, 0, 0
    cp.assert_equal(_device_call(sv, dev, s, tables={"signer_key": gk}), (ok, weight, used), s)
    # every CSR array ends past its array: the last body's ranges are clamped
    junk = {}
    for name, extra in (("sig_begin", 7), ("key_begin", 9), ("check_begin", 50), ("signer_begin", 1000)):
        a = s[name].copy()
        a[-1] += np.uint64(extra)
        junk[name] = a
    cp.assert_equal(_device_call(sv, dev, s, tables=junk), want, s)
    # a check table that claims fewer bodies' checks than n_checks: the checks no body owns are false
    short = s["check_begin"].copy()
    short[-1] -= np.uint64(1)
    got = _device_call(sv, dev, s, tables={"check_begin": short})
    assert (got[0][:-1] == want[0][:-1]).all() and (got[0][-1], got[1][-1], got[2][-1]) == (0, 0, 0)


class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    st = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(st))
    return st


def test_mirror_prefetch5(sv, dev):
    """~2000 envelopes: prefetch 5 is ONE engine batch with no fallback and gives
    the results and hashes of prefetch 0, 1 and 3; with the engine failing the
    results are the same through the CPU form, with one fallback counted."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(400, 31, tp.device_signer(sv), with_payload=False)
    assert s["n"] == 2000

    def call(prefetch):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch)

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all()
    assert (ch0 == s["contents_hash"]).all() and (fb0 == s["fee_bump_hash"]).all()
    for p in (1, 3):
        res, _, ch, fb = call(p)
        assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()
    _stats(host)
    res, checks, ch, fb = call(5)
    st = _stats(host)
    assert st.gpu_batches == 1 and st.fallbacks == 0
    assert checks == 2 * s["n"] + s["kinds"].count("fee_bump")
    assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()
    prev = sv.set_debug_flags(sv.DBG_FAIL)
    try:
        res, _, ch, fb = call(5)
    finally:
        sv.set_debug_flags(prev)
    st = _stats(host)
    assert st.fallbacks == 1 and st.gpu_batches == 0
    assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()


def test_mirror_prefetch5_with_payload_signers(sv, dev):
    """The set with its signed-payload unit: the check of that account comes
    back false from the device (weight 1 of 2) and is finished on the host from
    the device's weight and marks."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(50, 37, tp.device_signer(sv), with_payload=True)
    assert s["n"] == 300 and s["kinds"].count("payload") == 50

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch, for_apply=for_apply)

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all()
    _stats(host)
    res, checks, ch, fb = call(5)
    st = _stats(host)
    assert st.fallbacks == 0 and st.gpu_batches >= 1
    assert checks == 2 * s["n"] + s["kinds"].count("fee_bump")
    assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()
    assert (call(5, for_apply=1)[0] == call(0, for_apply=1)[0]).all()
