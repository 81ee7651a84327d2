"""The account store's replica on the device and the ledger forms' device path
(sv_txstore.hip; the stride instantiations of sv_txacct.hip), on the GPU.  The
replica is read back through account_store_read(device=0) -- its lookup kernel
and a gather -- and compared with the plain-Python model of txledger_pool.py.
The reference of every check result is the existing
sv_ed25519_check_txbodies_accounts_device / _decide_ twin on the combined table
the definition describes, built by the helper from the model; every comparison
is byte equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import txaccounts_pool as ap
import txbodies_pool as tp
import txledger_pool as lp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STORE_BLOCK = 256  # lanes per workgroup of the lookup kernel
GUARD = 16         # guard bytes on each side of every output of the device-resident call
SLACK = 16         # sentinel rows on each side of every input of the device-resident call


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    assert sv.load_library().sv_store_block() == STORE_BLOCK
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def store_off(sv):
    sv.set_account_store(0)
    yield
    sv.set_account_store(0)


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


# the device-resident inputs: name -> (bytes per row, where it comes from)
COMMON = {"bodies": 1, "off": 8, "len": 4, "kind": 1, "sig_begin": 8, "hint": 4, "sig": 64, "sig_len": 1,
          "bacct_begin": 8, "check_begin": 8, "check_acct": 4, "check_level": 1, "acheck_needed": 4}
TABLE = {"acct_key": 32, "acct_thresholds": 4, "asigner_begin": 8, "asigner_type": 1, "asigner_weight": 4,
         "asigner_key": 32, "asigner_payload": 4, "apayload": 64, "apayload_len": 1}


def _up(dev, arrays):
    """Every array between SLACK rows of 0xEE sentinels -> (buffers, what was sent, pointer of name)."""
    bufs, sent = {}, {}
    for name, (a, row) in arrays.items():
        data = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        h = np.concatenate([np.full(SLACK * row, 0xEE, np.uint8), data, np.full(SLACK * row, 0xEE, np.uint8)])
        sent[name] = (h, row)
        bufs[name] = torch.from_numpy(h.copy()).to(dev)
    return bufs, sent, lambda name: bufs[name].data_ptr() + SLACK * sent[name][1]


def _guarded(dev, n, widths):
    return [torch.full((2 * GUARD + w * max(n, 1),), 0xA5, dtype=torch.uint8, device=dev) for w in widths]


def _unguard(o, w, n, dt):
    h = o.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + w * n:] == 0xA5).all(), "a write outside an output array"
    return h[GUARD:GUARD + w * n].copy().view(dt)


def _device(sv, dev, s, lg=None, protocol=21, decide=None):
    """The ledger device form (lg: the ledger arrays) or its by-account twin (lg None: the set's combined table)
    -> (ok, weight, used, digests[, found]) and, with decide=(role, flags), also (code, fail, bad, n_bad).  Inputs
    between sentinels that must come back unchanged, outputs between guards."""
    arrays = {k: (s[k], w) for k, w in COMMON.items()}
    src = lg if lg is not None else s
    arrays.update({k: (src[k], w) for k, w in TABLE.items()})
    arrays["bacct"] = (src["bacct"], 4)
    if lg is not None:
        arrays["bacct_id"] = (lg["bacct_id"], 32)
    if decide:
        arrays["role"], arrays["flags"] = (decide[0], 1), (decide[1], 1)
    bufs, sent, p = _up(dev, arrays)
    nb, ns, nc, ne = s["nb"], s["ns"], s["nc"], s["ne"]
    na, nas, npay = (lg["nl"], lg["nls"], lg["nlp"]) if lg is not None else (s["na"], s["nas"], s["npay"])
    ok, weight, used = _guarded(dev, nc, (1, 4, 8))
    found, = _guarded(dev, ne, (1,))
    code, fail, bad = _guarded(dev, nb, (1, 4, 4))
    n_bad = torch.zeros(1, dtype=torch.int64, device=dev)
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    g = lambda t: t.data_ptr() + GUARD  # noqa: E731
    head = (0, tp.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"), ns,
            p("acct_key"), p("acct_thresholds"), p("asigner_begin"), p("asigner_type"), p("asigner_weight"),
            p("asigner_key"), p("asigner_payload"), p("apayload"), p("apayload_len"), na, nas, npay, p("bacct_begin"),
            p("bacct"), ne)
    if lg is not None:
        head += (p("bacct_id"), g(found))
    head += (p("check_begin"), p("check_acct"), p("check_level"), p("acheck_needed"), nc)
    kw = dict(d_sig_len=p("sig_len"), protocol_version=protocol, d_digests=t_dig.data_ptr(),
              stream=torch.cuda.current_stream(dev).cuda_stream)
    if decide:
        res = sv.results_desc(p("role"), p("flags"), g(code), g(fail), g(ok), g(weight), g(used), g(bad), nb,
                              n_bad.data_ptr())
        fn = sv.decide_txbodies_ledger_device if lg is not None else sv.decide_txbodies_accounts_device
        fn(*head, res, **kw)
    else:
        fn = sv.check_txbodies_ledger_device if lg is not None else sv.check_txbodies_accounts_device
        fn(*head, g(ok), g(weight), g(used), **kw)
    torch.cuda.synchronize(dev)
    for name, (h, _) in sent.items():
        assert (bufs[name].cpu().numpy() == h).all(), "an input or its sentinels changed: " + name
    out = [_unguard(ok, 1, nc, np.uint8), _unguard(weight, 4, nc, np.uint32), _unguard(used, 8, nc, np.uint64),
           t_dig.cpu().numpy()]
    if lg is not None:
        out.append(_unguard(found, 1, ne, np.uint8))
    else:
        assert (found.cpu().numpy() == 0xA5).all()
    if decide:
        k = int(n_bad.cpu()[0])
        out += [_unguard(code, 1, nb, np.uint8), _unguard(fail, 4, nb, np.uint32),
                _unguard(bad, 4, nb, np.uint32)[:k], k]
    else:
        assert all((x.cpu().numpy() == 0xA5).all() for x in (code, fail, bad))
    return out


def _host(sv, s, lg, protocol=21, **kw):
    """The host-buffer ledger form -> (ok, weight, used, digests, found)."""
    r, found = sv.check_txbodies_ledger(*lp.args(s, lg), sig_len=s["sig_len"], protocol_version=protocol, **kw)
    return list(r) + [found]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.asarray(g).tobytes() == np.asarray(w).tobytes(), i


def _fill(sv, bld, accounts=64, payloads=16, local=8):
    sv.set_account_store(accounts, payloads, local)
    model = bld.model()
    if model:
        sv.account_store_upsert(**lp.batch(list(model.items())))
    return model


# ------------------------------------------------ 1. the replica equals the model
def test_replica_equals_model(sv, dev):
    model, ids, want = lp.semantic_sequence(sv, device=0)
    st = sv.account_store_stats(0)
    assert {k: st[k] for k in want} == want
    rows, prows = 16 + 4, 2 + 20 * 4
    assert st["replica_current"] == 1 and st["device_bytes"] >= 948 * rows + 65 * prows + 4 * 32
    assert st["lookups"] > 0 and sv.workspace_bytes(0) >= st["device_bytes"]
    lp.read_all(sv, model, ids, device=-1)
    sv.account_store_clear()
    lp.read_all(sv, {}, ids, device=0)
    sv.set_account_store(0)
    lp.read_all(sv, {}, ids, device=0)
    assert sv.account_store_stats(0)["device_bytes"] == 0


def test_replica_smallest_index(sv, dev, monkeypatch):
    monkeypatch.setenv("SV_ACCT_STORE_SEED", str(lp.WRAP_SEED))
    ids = lp.wrapping_ids()
    rng = np.random.default_rng(5)
    rows = [(i, lp.rand_account(rng, 2)) for i in ids]
    for gone in range(4):
        sv.set_account_store(4, 0, 0)
        model = {}
        lp.read_all(sv, model, ids, device=0)  # (the replica exists before the writes: they go through the scatter)
        lp.upsert(sv, model, rows)
        assert sv.account_store_stats()["max_probe"] == 3
        lp.read_all(sv, model, ids, device=0)
        lp.erase(sv, model, [ids[gone]])
        lp.read_all(sv, model, ids, device=0)
        lp.upsert(sv, model, [rows[gone]])
        lp.read_all(sv, model, ids, device=0)
        assert sv.account_store_stats(0)["replica_current"] == 1


def test_replica_many_ids_in_one_read(sv, dev, monkeypatch):
    """300 IDs in one read -- more than one 256-lane block of the lookup -- 7 of them absent; 64 that differ in
    their last byte only among them."""
    monkeypatch.setenv("SV_ACCT_STORE_SEED", "7")
    rng = np.random.default_rng(9)
    ids = lp.last_byte_ids(rng) + [lp.rand_id(rng) for _ in range(300 - 64)]
    absent = set(range(3, 300, 45))
    assert len(absent) == 7
    sv.set_account_store(300, 64, 0)
    model = {}
    lp.read_all(sv, model, ids[:2], device=0)
    lp.upsert(sv, model, [(aid, lp.rand_account(rng, i % 4, payloads=(i % 50 == 1))) for i, aid in enumerate(ids)
                          if i not in absent])
    lp.read_all(sv, model, ids, device=0)
    # a slot that first uses the store later starts from the host copy: drop the replica, read again
    lp.erase(sv, model, ids[10:20])
    sv.set_device_map([0])
    assert sv.account_store_stats()["capacity"] == 0  # (the store goes with the slots)
    sv.set_account_store(300, 64, 0)
    model = {}
    lp.upsert(sv, model, [(aid, lp.rand_account(rng, 1)) for aid in ids[:40]])  # no replica yet: host only
    assert sv.account_store_stats(0)["device_bytes"] == 0
    lp.read_all(sv, model, ids, device=0)
    sv.set_device_map([])


# ------------------------------------------------ 2. all forms agree
@pytest.fixture(scope="module")
def edge(sv, dev, oracle):
    """The ledger edge cases and a random pool in one batch, GPU-signed; shared and left unchanged."""
    bld = lp.LBuilder(5)
    cases = lp.edge_cases(bld)
    lp.random_pool(bld, 120, n_store=30, n_local=4)
    s = bld.finish(tp.device_signer(sv), oracle)
    return bld, s, cases, bld.ledger(s)


def test_all_forms_agree(sv, dev, edge, kpath):
    bld, s, cases, lg = edge
    assert lg["nl"] >= 7 and not lg["found"].all() and (lg["bacct"] == lp.BY_ID).sum() > 100
    _fill(sv, bld, accounts=64, payloads=30 * 20 + 8, local=lg["nl"])
    for protocol in (21, 9):
        want = _device(sv, dev, s, protocol=protocol)
        assert want[0].any() and not want[0].all()
        got = _device(sv, dev, s, lg, protocol)
        _same(got[:4], want)
        assert (got[4] == lg["found"]).all()
        host = _host(sv, s, lg, protocol, device=0)
        _same(host[:4], want)
        assert (host[4] == lg["found"]).all()
        cpu, found = sv.check_txbodies_ledger_cpu(*lp.args(s, lg), sig_len=s["sig_len"], protocol_version=protocol)
        _same(cpu, want)
        assert (found == lg["found"]).all()
    got = _device(sv, dev, s, lg)
    for name, (c0, hand) in cases.items():
        assert [(int(got[0][c0 + i]), int(got[1][c0 + i]), int(got[2][c0 + i])) for i in range(len(hand))] == hand, name


def test_decide_forms_agree(sv, dev, edge):
    bld, s, cases, lg = edge
    _fill(sv, bld, accounts=64, payloads=30 * 20 + 8, local=lg["nl"])
    rng = np.random.default_rng(2)
    decide = (rng.integers(0, 2, s["nc"]).astype(np.uint8), rng.integers(0, 2, s["nb"]).astype(np.uint8))
    want = _device(sv, dev, s, decide=decide)
    got = _device(sv, dev, s, lg, decide=decide)
    assert 0 < want[-1] < s["nb"]
    _same(got[:4] + got[5:], want)
    assert (got[4] == lg["found"]).all()
    kw = dict(check_role=decide[0], body_flags=decide[1], sig_len=s["sig_len"], want_checks=True, bad_cap=s["nb"])
    for cpu, found in (sv.decide_txbodies_ledger_cpu(*lp.args(s, lg), **kw),
                       sv.decide_txbodies_ledger(*lp.args(s, lg), device=0, **kw)):
        _same([cpu.check_ok, cpu.check_weight, cpu.check_used, cpu.digests, cpu.body_code, cpu.body_fail,
               cpu.bad_body], want[:-1])
        assert cpu.n_bad == want[-1] and (found == lg["found"]).all()


# ------------------------------------------------ 3. seams
def _seam(sv, dev, oracle, nb, entries, n_local):
    bld = lp.LBuilder(900 + nb + (entries or 0))
    lp.random_pool(bld, nb, n_store=12, n_local=n_local, n_absent=2, entries=entries)
    s = bld.finish(tp.device_signer(sv), oracle)
    lg = bld.ledger(s)
    assert s["nb"] == nb and lg["nl"] == n_local and (entries is None or s["ne"] == entries)
    _fill(sv, bld, accounts=12, payloads=12 * 20, local=n_local)  # a local table of exactly local_accounts rows
    want = _device(sv, dev, s)
    got = _device(sv, dev, s, lg)
    _same(got[:4], want)
    assert (got[4] == lg["found"]).all()
    host = _host(sv, s, lg, device=0)
    _same(host[:4], want)
    assert (host[4] == lg["found"]).all()
    if s["nc"] > 8:
        assert want[0].any() and not want[0].all()


@pytest.mark.parametrize("nb", [1, 255, 256, 257])
def test_body_seams(sv, dev, oracle, nb):
    _seam(sv, dev, oracle, nb, None, 4)


@pytest.mark.parametrize("entries", [255, 256, 257])
def test_entry_seams(sv, dev, oracle, entries):
    _seam(sv, dev, oracle, 130, entries, 3)


# ------------------------------------------------ 4. the device form clamps
def test_device_form_clamps(sv, dev, edge, oracle):
    bld, s, cases, lg = edge
    model = _fill(sv, bld, accounts=64, payloads=30 * 20 + 8, local=lg["nl"])
    want = _device(sv, dev, s)
    rng = np.random.default_rng(4)
    # a bacct_id array of garbage behind the entries that are not by ID
    junk = lg["bacct_id"].copy()
    junk[lg["bacct"] != lp.BY_ID] = rng.integers(0, 256, (int((lg["bacct"] != lp.BY_ID).sum()), 32), dtype=np.uint8)
    _same(_device(sv, dev, s, dict(lg, bacct_id=junk))[:4], want)
    # ... and a call with NO entry by ID over a bacct_id array that is garbage throughout
    lb = lp.LBuilder(31)
    n1 = lb.account(ap.ed(5), (1, 0, 0, 0), where=lp.LOCAL)
    x1 = lb.account(ap.raw(bytes(32)), (0, 0, 0, 0), [(lp.ED, 1, ap.ed(3)), (lp.ED, 1, ap.ed(4))], where=lp.LOCAL)
    for t in range(5):
        b = lb.body(length=20 + t)
        b.sig_ed(5 if t % 2 else 3)
        b.sig_ed(4)
        b.acheck(b.use(n1), 0, 0)
        b.acheck(b.use(x1), 0, 2)
    ls = lb.finish(tp.device_signer(sv), oracle)
    ll = lb.ledger(ls)
    assert (ll["bacct"] != lp.BY_ID).all() and ll["nl"] == 2
    ll["bacct_id"] = rng.integers(0, 256, ll["bacct_id"].shape, dtype=np.uint8)
    lwant = _device(sv, dev, ls)
    lgot = _device(sv, dev, ls, ll)
    _same(lgot[:4], lwant)
    assert lgot[4].all() and lwant[0].any() and not lwant[0].all()
    _same(_host(sv, ls, ll, device=0)[:4], lwant)
    # a local index past the local table names no account: the twin with that entry past ITS table
    e = int(np.flatnonzero(lg["bacct"] != lp.BY_ID)[0])
    b2, t2 = lg["bacct"].copy(), s["bacct"].copy()
    b2[e], t2[e] = lg["nl"] + 3, s["na"] + 3
    got = _device(sv, dev, s, dict(lg, bacct=b2))
    _same(got[:4], _device(sv, dev, dict(s, bacct=t2)))
    f2 = lg["found"].copy()
    f2[e] = 0
    assert (got[4] == f2).all() and not (np.asarray(got[0]) == np.asarray(want[0])).all()
    # more local accounts than the store lends rows for: those past the last row are not read
    sv.set_account_store(64, 30 * 20 + 8, lg["nl"] - 1)
    sv.account_store_upsert(**lp.batch(list(model.items())))
    last = lg["nl"] - 1
    t3 = s["bacct"].copy()
    local_rows = [i for i, w in enumerate(bld.where) if w == lp.LOCAL]
    t3[s["bacct"] == local_rows[last]] = s["na"]
    got = _device(sv, dev, s, lg)
    _same(got[:4], _device(sv, dev, dict(s, bacct=t3)))
    assert (got[4] == np.where(lg["bacct"] == last, 0, lg["found"])).all()
    # every entry by ID with the store empty (max_probe at its smallest): nothing is found, only the local
    # accounts' checks can succeed
    sv.set_account_store(64, 8, lg["nl"])
    assert sv.account_store_stats()["max_probe"] == 1
    t4 = s["bacct"].copy()
    t4[lg["bacct"] == lp.BY_ID] = s["na"]
    got = _device(sv, dev, s, lg)
    _same(got[:4], _device(sv, dev, dict(s, bacct=t4)))
    assert (got[4] == (lg["bacct"] != lp.BY_ID)).all() and got[0].any()
    # bacct_id NULL: no entry by ID is found
    stream = torch.cuda.current_stream(dev).cuda_stream
    z = torch.zeros(64, dtype=torch.uint8, device=dev)
    b = torch.from_numpy(np.array([lp.BY_ID], np.uint32)).to(dev)
    beg = torch.from_numpy(np.array([0, 1], np.uint64)).to(dev)
    zero = torch.zeros(2, dtype=torch.int64, device=dev)
    f = torch.full((1,), 7, dtype=torch.uint8, device=dev)
    sv.check_txbodies_ledger_device(0, tp.NETWORK_ID, z.data_ptr(), zero.data_ptr(), zero.data_ptr(), z.data_ptr(), 1,
                                    zero.data_ptr(), 0, 0, 0, 0, 0, zero.data_ptr(), 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                    beg.data_ptr(), b.data_ptr(), 1, 0, f.data_ptr(), zero.data_ptr(), 0, 0, 0, 0,
                                    0, 0, 0, stream=stream)
    torch.cuda.synchronize(dev)
    assert f.cpu().tolist() == [0]
    # the store off: refused
    sv.set_account_store(0)
    with pytest.raises(sv.SigVerifyError) as err:
        _device(sv, dev, s, lg)
    assert err.value.code == -1


# ------------------------------------------------ 5. two slots on one GPU
def test_two_slots_hold_the_same_replica(sv, dev):
    rng = np.random.default_rng(12)
    ids = [lp.rand_id(rng) for _ in range(40)]
    sv.set_device_map([0, 0])
    try:
        assert sv.device_count() == 2
        sv.set_account_store(40, 8, 2)
        model = {}
        lp.upsert(sv, model, [(aid, lp.rand_account(rng, i % 5)) for i, aid in enumerate(ids[:30])])
        for d in (0, 1):  # (each slot's replica starts from the host copy)
            lp.read_all(sv, model, ids, device=d)
        lp.upsert(sv, model, [(ids[i], lp.rand_account(rng, 1, payloads=(i % 3 == 0))) for i in range(25, 40)])
        lp.erase(sv, model, ids[:5])
        for d in (0, 1):  # (... and follows every write through the scatter)
            assert sv.account_store_stats(d)["replica_current"] == 1
            lp.read_all(sv, model, ids, device=d)
    finally:
        sv.set_device_map([])
    assert sv.account_store_stats()["capacity"] == 0


def test_sliced_host_call_equals_the_one_slot_call(sv, dev, edge):
    bld, s, cases, lg = edge
    assert s["ns"] > 200
    sv.set_device_map([0, 0])
    try:
        sv.set_min_shard(64)
        _fill(sv, bld, accounts=64, payloads=30 * 20 + 8, local=lg["nl"])
        one = _host(sv, s, lg, device=0)
        lookups = [sv.account_store_stats(d)["device_bytes"] for d in (0, 1)]
        assert lookups[0] > 0 and lookups[1] == 0  # (slot 1 has not used the store yet)
        two = _host(sv, s, lg)  # sliced over both slots: each uploads the local accounts and reads its own replica
        assert all(sv.account_store_stats(d)["device_bytes"] > 0 for d in (0, 1))
        _same(two, one)
        _same(one[:4], _device(sv, dev, s))
        assert (one[4] == lg["found"]).all()
    finally:
        sv.set_min_shard(0)
        sv.set_device_map([])


# ------------------------------------------------ 6. a multi-chunk host call
def test_multi_chunk_host_call(sv, dev):
    """The staging chunk is read once per process, so the call runs in a fresh child with a small
    SV_STAGE_CHUNK (tests/txledger_multichunk.py holds the set and the comparison)."""
    env = dict(os.environ, SV_STAGE_CHUNK="1024")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                     "txledger_multichunk.py")],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "multichunk ok" in r.stdout, r.stdout[-4000:]


# ------------------------------------------------ 7. an upsert between two device calls
def test_upsert_between_two_device_calls(sv, dev, oracle):
    def build(signers):
        bld = lp.LBuilder(8)  # (the same seed: the same body bytes)
        a = bld.account(ap.ed(21), (0, 1, 2, 2), signers)
        b = bld.body(length=50)
        b.sig_ed(2)
        b.sig_ed(3)
        p = b.use(a)
        b.acheck(p, 1)
        b.acheck(p, 2)
        s = bld.finish(tp.device_signer(sv), oracle)
        return bld, s, bld.ledger(s)

    one, two = [(lp.ED, 1, ap.ed(2))], [(lp.ED, 1, ap.ed(2)), (lp.ED, 1, ap.ed(3))]
    bld1, s1, lg1 = build(one)
    bld2, s2, lg2 = build(two)
    model = _fill(sv, bld1)
    got = _device(sv, dev, s1, lg1)
    _same(got[:4], _device(sv, dev, s1))
    assert got[0].tolist() == [1, 0]
    lp.upsert(sv, model, list(bld2.model().items()))  # (returns when the replica holds it: nothing else to wait for)
    got = _device(sv, dev, s2, lg2)
    _same(got[:4], _device(sv, dev, s2))
    assert got[0].tolist() == [1, 1] and got[2].tolist() == [0b01, 0b11]
    _same(_host(sv, s2, lg2, device=0), got)
    lp.erase(sv, model, list(model))
    got = _device(sv, dev, s2, lg2)
    assert got[0].tolist() == [0, 0] and got[4].tolist() == [0]


# ------------------------------------------------ 8. with a verdict cache on
def test_with_a_verdict_cache(sv, dev, edge):
    bld, s, cases, lg = edge
    _fill(sv, bld, accounts=64, payloads=30 * 20 + 8, local=lg["nl"])
    want = _device(sv, dev, s, lg)
    sv.set_verdict_cache(1 << 14)
    try:
        first = _device(sv, dev, s, lg)
        h0 = sv.verdict_cache_stats(0)["hits"]
        second = _device(sv, dev, s, lg)
        assert sv.verdict_cache_stats(0)["hits"] > h0
        _same(first, want)
        _same(second, want)
        _same(_host(sv, s, lg, device=0), want)
    finally:
        sv.set_verdict_cache(0)
