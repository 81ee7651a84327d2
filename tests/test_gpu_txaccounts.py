"""Signature checks against a device-side account table, on the GPU: the
expansion kernels of sv_txacct.hip behind sv_ed25519_check_txbodies_accounts /
_accounts_device -- the edge cases and a random pool on every verify-kernel
path, the block seams of the per-body, per-check and per-account kernels and
the second level of their scan, unvalidated device tables, equality with the
explicit device form over the Python expansion, two slots and a multi-chunk
host call.  Expectations come from the Python replay over the plain-Python
expansion of txaccounts_pool.py (by construction for the large vectorised
sets); every comparison is exact equality."""
import ctypes

import numpy as np
import pytest

import envelope_bodies as eb
import txaccounts_pool as ap
import txbodies_pool as tp
import txchecks_pool as cp
import txpayload_pool as pl
import txset_gen as tg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ACCT_BLOCK = 256  # lanes per workgroup of the expansion's count / scan kernels
GUARD = 16        # guard bytes on each side of every output of the device-resident call
SLACK = 16        # sentinel rows on each side of every input of the device-resident call
ED, SP = ap.ED, ap.SP


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    assert sv.load_library().sv_acct_block() == ACCT_BLOCK
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


def _host(sv, s, protocol=21, **kw):
    return sv.check_txbodies_accounts(*ap.args(s), sig_len=s["sig_len"], protocol_version=protocol, **kw)


def _cpu(sv, s, protocol=21):
    return sv.check_txbodies_accounts_cpu(*ap.args(s), sig_len=s["sig_len"], protocol_version=protocol)


# name -> (key in the set, bytes per row)
DEVICE_INPUTS = {"bodies": ("bodies", 1), "off": ("off", 8), "len": ("len", 4), "kind": ("kind", 1),
                 "sig_begin": ("sig_begin", 8), "hint": ("hint", 4), "sig": ("sig", 64), "sig_len": ("sig_len", 1),
                 "acct_key": ("acct_key", 32), "acct_thresholds": ("acct_thresholds", 4),
                 "asigner_begin": ("asigner_begin", 8), "asigner_type": ("asigner_type", 1),
                 "asigner_weight": ("asigner_weight", 4), "asigner_key": ("asigner_key", 32),
                 "asigner_payload": ("asigner_payload", 4), "apayload": ("apayload", 64),
                 "apayload_len": ("apayload_len", 1), "bacct_begin": ("bacct_begin", 8), "bacct": ("bacct", 4),
                 "check_begin": ("check_begin", 8), "check_acct": ("check_acct", 4), "check_level": ("check_level", 1),
                 "check_needed": ("acheck_needed", 4)}


def _device_call(sv, dev, s, protocol=21, over=None):
    """sv_ed25519_check_txbodies_accounts_device over the set -> (ok, weight,
    used, digests).  Every input sits between SLACK rows of 0xEE sentinels --
    an index a few rows past its table still lands inside the test's own
    allocation -- and must come back byte for byte as it went up; the outputs
    sit between guard bytes that must stay untouched.  `over` replaces arrays
    with unvalidated ones (the counts stay the set's)."""
    t = dict(s)
    t.update(over or {})
    bufs, sent = {}, {}
    for name, (key, row) in DEVICE_INPUTS.items():
        data = np.ascontiguousarray(t[key]).view(np.uint8).reshape(-1)
        h = np.concatenate([np.full(SLACK * row, 0xEE, np.uint8), data, np.full(SLACK * row, 0xEE, np.uint8)])
        sent[name] = h
        bufs[name] = torch.from_numpy(h.copy()).to(dev)
    p = lambda name: bufs[name].data_ptr() + SLACK * DEVICE_INPUTS[name][1]  # noqa: E731
    nb, ns, nc = s["nb"], s["ns"], s["nc"]
    outs = [torch.full((2 * GUARD + w * max(nc, 1),), 0xA5, dtype=torch.uint8, device=dev) for w in (1, 4, 8)]
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sv.check_txbodies_accounts_device(
        0, tp.NETWORK_ID, p("bodies"), p("off"), p("len"), p("kind"), nb, p("sig_begin"), p("hint"), p("sig"), ns,
        p("acct_key"), p("acct_thresholds"), p("asigner_begin"), p("asigner_type"), p("asigner_weight"),
        p("asigner_key"), p("asigner_payload"), p("apayload"), p("apayload_len"), s["na"], s["nas"], s["npay"],
        p("bacct_begin"), p("bacct"), s["ne"], p("check_begin"), p("check_acct"), p("check_level"), p("check_needed"),
        nc, outs[0].data_ptr() + GUARD, outs[1].data_ptr() + GUARD, outs[2].data_ptr() + GUARD,
        d_sig_len=p("sig_len"), protocol_version=protocol, d_digests=t_dig.data_ptr(), stream=stream)
    torch.cuda.synchronize(dev)
    for name, h in sent.items():
        assert (bufs[name].cpu().numpy() == h).all(), "an input or its sentinels changed: " + name
    res = []
    for o, w, dt in zip(outs, (1, 4, 8), (np.uint8, np.uint32, np.uint64)):
        h = o.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + w * nc:] == 0xA5).all(), "a write outside the output array"
        res.append(h[GUARD:GUARD + w * nc].copy().view(dt))
    return res[0], res[1], res[2], t_dig.cpu().numpy()


def _explicit_device_call(sv, dev, s, protocol=21):
    """sv_ed25519_check_txbodies_device over the Python expansion of the set."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    pad = lambda a, w: a if len(a) else np.zeros((1, w), np.uint8)  # noqa: E731
    one = lambda a, dt: a if len(a) else np.zeros(1, dt)  # noqa: E731
    nb, ns, nk, nc, ng, nq = s["nb"], s["ns"], s["nk"], s["nc"], s["ng"], s["nq"]
    d = {k: up(s[k]) for k in ("bodies", "off", "len", "kind", "sig_begin", "key_begin", "check_begin", "signer_begin",
                               "pkey_begin")}
    d["hint"], d["sig"], d["key"] = up(pad(s["hint"], 4)), up(pad(s["sig"], 64)), up(pad(s["key"], 32))
    d["need"] = up(one(s["check_needed"], np.int32))
    d["gt"], d["gw"] = up(one(s["signer_type"], np.uint8)), up(one(s["signer_weight"], np.uint32))
    d["gk"], d["sl"] = up(one(s["signer_key"], np.uint32)), up(one(s["sig_len"], np.uint8))
    d["qk"], d["qp"], d["ql"] = up(pad(s["pkey"], 32)), up(pad(s["pkey_payload"], 64)), up(one(s["pkey_len"], np.uint8))
    outs = [torch.zeros(w * max(nc, 1), dtype=torch.uint8, device=dev) for w in (1, 4, 8)]
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    sv.check_txbodies_device(0, tp.NETWORK_ID, d["bodies"].data_ptr(), d["off"].data_ptr(), d["len"].data_ptr(),
                             d["kind"].data_ptr(), nb, d["sig_begin"].data_ptr(), d["hint"].data_ptr(),
                             d["sig"].data_ptr(), ns, d["key_begin"].data_ptr(), d["key"].data_ptr(), nk,
                             d["check_begin"].data_ptr(), d["need"].data_ptr(), nc, d["signer_begin"].data_ptr(),
                             d["gt"].data_ptr(), d["gw"].data_ptr(), d["gk"].data_ptr(), ng, outs[0].data_ptr(),
                             outs[1].data_ptr(), outs[2].data_ptr(), d_sig_len=d["sl"].data_ptr(),
                             protocol_version=protocol, d_digests=t_dig.data_ptr(),
                             stream=torch.cuda.current_stream(dev).cuda_stream, d_pkey_begin=d["pkey_begin"].data_ptr(),
                             d_pkey=d["qk"].data_ptr(), d_pkey_payload=d["qp"].data_ptr(), d_pkey_len=d["ql"].data_ptr(),
                             n_pkeys=nq)
    torch.cuda.synchronize(dev)
    return tuple(o.cpu().numpy()[:w * nc].view(dt) for o, w, dt in zip(outs, (1, 4, 8), (np.uint8, np.uint32,
                                                                                         np.uint64))) + (
        t_dig.cpu().numpy(),)


@pytest.fixture(scope="module")
def edge(sv, dev, oracle):
    """The edge cases and a random pool in one batch, GPU-signed; shared and left unchanged."""
    bld = ap.ABuilder(5)
    cases = ap.edge_cases(bld)
    ap.random_pool(bld, 200)
    s = bld.finish(tp.device_signer(sv), oracle)
    verify = cp.oracle_verify(oracle)
    return s, cases, {p: ap.expected(s, verify, p) for p in (21, 9)}


def test_edge_cases_and_pool_host_and_device(sv, dev, edge, kpath):
    s, cases, want = edge
    for protocol in (21, 9):
        w = want[protocol]
        assert w[0].any() and not w[0].all()
        cp.assert_equal(_host(sv, s, protocol, device=0), w, s)
        cp.assert_equal(_device_call(sv, dev, s, protocol), w, s)
    ok, weight, used, _ = _device_call(sv, dev, s)
    for name, (c0, hand) in cases.items():
        got = [(int(ok[c0 + i]), int(weight[c0 + i]), int(used[c0 + i])) for i in range(len(hand))]
        assert got == hand, name


def test_cpu_form_agrees(sv, dev, edge):
    s, _, want = edge
    cp.assert_equal(_cpu(sv, s), want[21], s)


def test_device_form_equals_explicit_device_form(sv, dev, edge):
    """Byte for byte, digests included, at both protocol sides of the clamp."""
    s = edge[0]
    for protocol in (21, 9):
        a, b = _device_call(sv, dev, s, protocol), _explicit_device_call(sv, dev, s, protocol)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def _seam_set(sv, oracle, nb, na, checks_per_body=None):
    """na accounts of several shapes (master weight 0..2, none to two signers, a
    signed-payload signer in one of five) and nb bodies of a few bytes; body t
    lists one or two accounts (the first and last account of every 256-account
    tile are used), has 0..2 signatures and checks_per_body(t) checks (default
    1, none in one body of seven)."""
    bld = ap.ABuilder(700 + nb + na)
    for i in range(na):
        signers = []
        if i % 4 == 1:
            signers.append((ED, 1 + i % 2, ap.ed(1 + (i + 1) % 6)))
        if i % 5 == 2:
            signers.append((SP, 2, ap.ed(1 + i % 6), pl.payload_of(32, i % 3)))
        bld.account(ap.ed(1 + i % 6), ((i + 1) % 3, 1, 2, 3), signers)
    for t in range(nb):
        b = bld.body(length=int(bld.rng.integers(0, 12)))
        first = (t * 7) % na if t >= 4 else (0, na - 1, min(na - 1, ACCT_BLOCK - 1), min(na - 1, ACCT_BLOCK))[t]
        pos = [b.use(first)]
        if t % 3 == 1:
            pos.append(b.use((t + 1) % na))
        A = bld.accounts[first]
        if t % 2 == 0:
            b.sig_ed(A.master[1], corrupt=t % 11 == 4)
        if t % 4 == 1 and A.signers:
            g = A.signers[-1]
            if g[0] == SP:
                b.sig_payload(g[2][1], g[3])
            else:
                b.sig_ed(g[2][1])
        n = (0 if t % 7 == 3 else 1) if checks_per_body is None else checks_per_body(t)
        for c in range(n):
            b.acheck(pos[(t + c) % len(pos)], (t + c) % 4, c % 3)
    return bld.finish(tp.device_signer(sv), oracle)


def _check_all_forms(sv, dev, oracle, s):
    want = ap.expected(s, cp.oracle_verify(oracle))
    if s["nc"] > 4:
        assert want[0].any() and not want[0].all()
    cp.assert_equal(_host(sv, s, device=0), want, s)
    cp.assert_equal(_device_call(sv, dev, s), want, s)


@pytest.mark.parametrize("nb", [1, 255, 256, 257, 513])
def test_body_seams(sv, dev, oracle, nb):
    s = _seam_set(sv, oracle, nb, 40)
    assert s["nb"] == nb
    _check_all_forms(sv, dev, oracle, s)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_check_seams(sv, dev, oracle, n):
    """n checks; the checks of one body straddle the 256-check boundary."""
    counts = cp.seam_counts(n)
    s = _seam_set(sv, oracle, len(counts), 40, checks_per_body=lambda t: counts[t])
    assert s["nc"] == n
    _check_all_forms(sv, dev, oracle, s)


@pytest.mark.parametrize("na", [1, 256, 257])
def test_account_seams(sv, dev, oracle, na):
    s = _seam_set(sv, oracle, na + 40, na)
    assert s["na"] == na and len(set(s["bacct"].tolist())) > min(na, 200) * 0.9
    _check_all_forms(sv, dev, oracle, s)


def _big_set(sv, nb, na, extra, sig_every):
    """A vectorised set (no builder objects): account a has the master key of
    seed a with weight 1 + a % 2, thresholds 1 / 2 / 3 and `extra` signers of
    weight 1 over random rows -- ED25519, but the first one of every account
    with a % 4 == 1 a signed-payload signer (nobody signs its payload); body t
    lists account t % na and, when t % 5 == 2, account (t + 1) % na behind it;
    it has one check at level 1 + t % 3 (none when t % 7 == 3), on its second
    account when t % 10 == 7, and, every sig_every-th body, one signature by
    its first account's master (one in nine of them corrupted).
    -> (set, (ok, weight, used) by construction: a check succeeds iff it names
    the first account, its body has a valid signature and the master weight
    reaches the level's threshold; a check on the second account meets no
    signature of that account)."""
    rng = np.random.default_rng(nb + na)
    T = np.arange(nb)
    length = (4 + T % 5).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(length[:-1])]).astype(np.uint64)
    blob = rng.integers(0, 256, int(length.sum()) + 1, dtype=np.uint8)
    kind = (T % 3).astype(np.uint8)
    signing = T[T % sig_every == 0]
    acct_of = T % na
    seeds = np.array([np.frombuffer(cp.seed_of(1000 + a), np.uint8) for a in range(na)], np.uint8)
    msgs = np.array([np.frombuffer(tp.contents_hash(int(kind[t]), blob[int(off[t]):int(off[t]) + int(length[t])]
                                                    .tobytes()), np.uint8) for t in signing], np.uint8)
    pk, made = tp.device_signer(sv)(np.concatenate([seeds, seeds[acct_of[signing]]]),
                                    np.concatenate([np.zeros((na, 32), np.uint8), msgs]))
    acct_key, sig = pk[:na].copy(), made[na:].copy()
    bad = np.arange(len(signing)) % 9 == 5
    sig[bad, 40] ^= 1
    sig_begin = np.concatenate([[0], np.cumsum(T % sig_every == 0)]).astype(np.uint64)
    has_check = T % 7 != 3
    level = (1 + T % 3).astype(np.uint8)
    thr = np.stack([1 + np.arange(na) % 2, np.full(na, 1), np.full(na, 2), np.full(na, 3)], 1).astype(np.uint8)
    # the signers: account a's are rows a * extra ..; a payload row per signed-payload signer
    gtype = np.zeros(na * extra, np.uint8)
    sp = np.arange(na)[np.arange(na) % 4 == 1] * extra if extra else np.zeros(0, np.int64)
    gtype[sp] = 3
    gpay = np.zeros(na * extra, np.uint32)
    gpay[sp] = np.arange(len(sp))
    two = T % 5 == 2
    per = 1 + two.astype(np.int64)
    eb_ = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    bacct = np.zeros(int(eb_[-1]), np.uint32)
    bacct[eb_[:-1].astype(np.int64)] = acct_of
    bacct[eb_[:-1].astype(np.int64)[two] + 1] = (T[two] + 1) % na
    second = (T % 10 == 7) & (na > 1)
    s = dict(bodies=blob, off=off, len=length, kind=kind, nb=nb, sig_begin=sig_begin,
             hint=acct_key[acct_of[signing]][:, 28:].copy(), sig=sig, ns=len(signing),
             sig_len=np.full(len(signing), 64, np.uint8), acct_key=acct_key, acct_thresholds=thr,
             asigner_begin=(np.arange(na + 1) * extra).astype(np.uint64), asigner_type=gtype,
             asigner_weight=np.ones(na * extra, np.uint32),
             asigner_key=rng.integers(0, 256, (na * extra, 32), dtype=np.uint8), asigner_payload=gpay,
             apayload=rng.integers(0, 256, (len(sp), 64), dtype=np.uint8),
             apayload_len=np.full(len(sp), 64, np.uint8), na=na, nas=na * extra, npay=len(sp), bacct_begin=eb_,
             bacct=bacct, ne=len(bacct), check_begin=np.concatenate([[0], np.cumsum(has_check)]).astype(np.uint64),
             check_acct=second[has_check].astype(np.uint32), check_level=level[has_check],
             acheck_needed=np.zeros(int(has_check.sum()), np.int32), nc=int(has_check.sum()))
    valid = np.zeros(nb, bool)
    valid[signing[~bad]] = True
    valid &= ~second
    mw = thr[acct_of, 0].astype(np.uint32)
    weight = np.where(valid, mw, 0).astype(np.uint32)
    ok = (valid & (mw >= level)).astype(np.uint8)
    return s, (ok[has_check], weight[has_check], valid[has_check].astype(np.uint64))


def _explicit_cpu_over_numpy_expansion(sv, s):
    """The second reference for the vectorised sets: the expansion of
    include/stellar_sigverify.h restated over the set's arrays with plain loops
    (nothing of the code under test), fed to sv_ed25519_check_txbodies_cpu."""
    gb, gt, gw = s["asigner_begin"].astype(np.int64), s["asigner_type"], s["asigner_weight"]
    eb_, cb = s["bacct_begin"].astype(np.int64), s["check_begin"].astype(np.int64)
    key, qkey, qpay, qlen, kb, qb = [], [], [], [], [0], [0]
    need, sb, st, sw, sk = [], [0], [], [], []
    for t in range(s["nb"]):
        rows = []  # per entry: (master row or None, [(type, weight, row)])
        for a in s["bacct"][eb_[t]:eb_[t + 1]]:
            a = int(a)
            m = None
            if s["acct_thresholds"][a, 0]:
                m = len(key)
                key.append(s["acct_key"][a])
            gs = []
            for g in range(gb[a], gb[a + 1]):
                if gt[g] == 3:
                    gs.append((3, int(gw[g]), len(qkey)))
                    qkey.append(s["asigner_key"][g])
                    qpay.append(s["apayload"][s["asigner_payload"][g]])
                    qlen.append(s["apayload_len"][s["asigner_payload"][g]])
                else:
                    gs.append((int(gt[g]), int(gw[g]), len(key)))
                    key.append(s["asigner_key"][g])
            rows.append((a, m, gs))
        for c in range(cb[t], cb[t + 1]):
            a, m, gs = rows[int(s["check_acct"][c])]
            lv = int(s["check_level"][c])
            need.append(int(s["acct_thresholds"][a, lv]) if lv else int(s["acheck_needed"][c]))
            for ty, w, k in ([(0, int(s["acct_thresholds"][a, 0]), m)] if m is not None else []) + gs:
                st.append(ty)
                sw.append(w)
                sk.append(k)
            sb.append(len(st))
        kb.append(len(key))
        qb.append(len(qkey))
    arr = lambda x, dt, w=None: (np.array(x, dt).reshape(-1, w) if w else np.array(x, dt).reshape(-1))  # noqa: E731
    return sv.check_txbodies_cpu(tp.NETWORK_ID, s["bodies"], s["off"], s["len"], s["kind"], s["sig_begin"], s["hint"],
                                 s["sig"], arr(kb, np.uint64), arr(key, np.uint8, 32), s["check_begin"],
                                 arr(need, np.int32), arr(sb, np.uint64), arr(st, np.uint8), arr(sw, np.uint32),
                                 arr(sk, np.uint32), sig_len=s["sig_len"], pkey_begin=arr(qb, np.uint64),
                                 pkey=arr(qkey, np.uint8, 32), pkey_payload=arr(qpay, np.uint8, 64),
                                 pkey_len=arr(qlen, np.uint8))


def test_scan_second_level(sv, dev):
    """65 537 bodies: the scan of the per-body counts takes a second round of 256 blocks."""
    nb = 65537
    s, want = _big_set(sv, nb, 300, 1, 64)
    assert s["nb"] == nb > ACCT_BLOCK * ACCT_BLOCK and want[0].any() and not want[0].all()
    ref = _explicit_cpu_over_numpy_expansion(sv, s)
    cp.assert_equal(ref[:3], want)
    for got in (_device_call(sv, dev, s), _host(sv, s, device=0)):
        cp.assert_equal(got[:3], want)
        assert (got[3] == ref[3]).all()


def test_device_form_clamps_unvalidated_tables(sv, dev, oracle):
    """Indices the host forms refuse, legal for the device-resident form and
    clamped by design.  Each has a valid equivalent, whose replay is the
    expectation: a bacct entry >= n_accounts contributes nothing and a check
    that names it (or a position past its body's entries) has no signer -- the
    entry of an account without master weight and signers; a payload index past
    the table reads as the empty payload.  _device_call asserts that the inputs,
    their sentinels and the guards around the outputs are untouched."""
    bld = ap.ABuilder(29)
    p32 = pl.payload_of(32)
    a = bld.account(ap.ed(1), (1, 1, 2, 3), [(ED, 1, ap.ed(2)), (SP, 1, ap.ed(3), p32)])
    void = bld.account(ap.ed(4), (0, 0, 0, 0))
    e = bld.account(ap.ed(1), (1, 1, 2, 3), [(SP, 1, ap.ed(3), b"")])  # (its payload index goes out of range below)
    for t in range(6):
        b = bld.body(length=30 + t)
        pa, pv, pe = b.use(a), b.use(void), b.use(e)
        b.sig_ed(1)
        b.sig_payload(3, p32)
        b.sig_payload(3, b"")
        b.sig_ed(2)
        b.acheck(pa, 3)
        b.acheck(pv, 0, 0)
        b.acheck(pe, 2)
        b.acheck(pv, 1)
    s = bld.finish(tp.device_signer(sv), oracle)
    want = ap.expected(s, cp.oracle_verify(oracle))
    assert want[0].tolist() == [1, 0, 1, 0] * 6 and want[1].tolist() == [3, 0, 2, 0] * 6
    cp.assert_equal(_device_call(sv, dev, s), want, s)
    bacct, cacct, spay = s["bacct"].copy(), s["check_acct"].copy(), s["asigner_payload"].copy()
    for t in range(6):
        e0, c0 = int(s["bacct_begin"][t]), int(s["check_begin"][t])
        bacct[e0 + 1] = s["na"] + t                                  # the void entry: an account past the table
        cacct[c0 + 3] = 3 + t % 3                                    # a position at or past the body's three entries
    g = int(s["asigner_begin"][e])
    assert s["asigner_type"][g] == 3 and s["apayload_len"][spay[g]] == 0
    spay[g] = s["npay"] + 2                                          # a payload past the table
    for over in ({"bacct": bacct}, {"check_acct": cacct}, {"asigner_payload": spay},
                 {"bacct": bacct, "check_acct": cacct, "asigner_payload": spay}):
        cp.assert_equal(_device_call(sv, dev, s, over=over), want, s)
    # CSR arrays that end past their tables: the last ranges are clamped
    eb = s["bacct_begin"].copy()
    eb[-1] += np.uint64(5)
    gb = s["asigner_begin"].copy()
    gb[-1] += np.uint64(4)  # (account e, the last one, would gain four signers of sentinel bytes)
    cp.assert_equal(_device_call(sv, dev, s, over={"bacct_begin": eb, "asigner_begin": gb}), want, s)
    # a level above 3 reads as 3
    lv = s["check_level"].copy()
    lv[0] = 9
    cp.assert_equal(_device_call(sv, dev, s, over={"check_level": lv}), want, s)


def test_two_slots_accounts_on_both_sides(sv, dev):
    s, want = _big_set(sv, 2400, 50, 2, 1)
    half = int(s["bacct_begin"][1200])
    assert s["ns"] == 2400 and set(s["bacct"][:half].tolist()) == set(s["bacct"][half:].tolist())
    assert (s["asigner_type"] == 3).any() and (s["check_acct"] == 1).any()
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
    ref = _explicit_cpu_over_numpy_expansion(sv, s)
    cp.assert_equal(ref[:3], want)
    cp.assert_equal(one[:3], want)
    cp.assert_equal(two[:3], want)
    assert (one[3] == ref[3]).all() and (two[3] == ref[3]).all() and sv.device_count() >= 1


def test_multi_chunk_account_in_first_and_last_chunk(sv, dev):
    """12 000 bodies over accounts of 60 signers and a master: 61 expanded key
    rows per body cross the key bound of a chunk (2^18) three times while the
    signatures stay far below theirs; every account is used in every chunk, the
    results are global."""
    nb = 12000
    s, want = _big_set(sv, nb, 7, 60, 2)
    assert 61 * nb > 2 * (1 << 18) and s["ns"] < (1 << 14) and want[0].any() and not want[0].all()
    got = _host(sv, s, device=0)
    cp.assert_equal(got[:3], want)
    ref = _explicit_cpu_over_numpy_expansion(sv, s)
    cp.assert_equal(ref[:3], want)
    assert (got[3] == ref[3]).all()
    dig = np.array([np.frombuffer(tp.contents_hash(int(s["kind"][t]), s["bodies"][int(s["off"][t]):int(s["off"][t])
                                                   + int(s["len"][t])].tobytes()), np.uint8) for t in range(0, nb, 97)])
    assert (got[3][::97] == dig).all()
    cp.assert_equal(_device_call(sv, dev, s)[:3], want)


class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def test_mirror_prefetch7(sv, dev, oracle):
    """The generated envelope set with its signed-payload unit: prefetch 7 is ONE
    engine batch with no fallback, gives the result codes of prefetch 1 and of
    replay_envelope, makes no single verification (no verifySig lookup, no
    signature beyond the engine batch's) and builds no signer list; with the
    engine failing the results are the same through the CPU form, with one
    fallback counted."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_signer_lists_built.restype = ctypes.c_uint64
    s = eb.build_set(50, 37, tp.device_signer(sv), with_payload=True)
    assert s["n"] == 300 and s["kinds"].count("payload") == 50

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch, for_apply=for_apply)

    def counted(prefetch):
        host.svh_cache_clear()
        hits, misses, st = ctypes.c_uint64(), ctypes.c_uint64(), EngineStats()
        host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
        host.svh_engine_counts_ex(ctypes.byref(st))
        built = host.svh_signer_lists_built()
        out = call(prefetch)
        built = host.svh_signer_lists_built() - built
        host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
        host.svh_engine_counts_ex(ctypes.byref(st))
        return out, st, hits.value + misses.value, built

    ref, _, ch1, fb1 = call(1)
    assert (ref["code"] == s["expect"]).all()
    verify = cp.oracle_verify(oracle)
    want = [tg.replay_envelope(c, 21, 0, verify) for c in pl.envelope_cases(s)]
    sigs_sent = int(s["envs_blank"]["nsigs"].sum() + s["envs_blank"]["nouter"].sum())
    (res, checks, ch, fb), st, lookups, built = counted(7)
    for k in ("code", "inner_code", "failed_op", "op_code"):
        assert res[k].tolist() == [w[k] for w in want], k
    assert (res == ref).all() and (ch == ch1).all() and (fb == fb1).all()
    assert checks == 2 * s["n"] + s["kinds"].count("fee_bump")
    assert (st.gpu_batches, st.fallbacks, st.gpu_signatures, st.cpu_signatures, lookups, built) == (1, 0, sigs_sent, 0,
                                                                                                    0, 0)
    (res6, checks6, _, _), _, _, built6 = counted(6)
    assert (res6 == ref).all() and checks6 == checks and built6 > checks
    assert (call(7, for_apply=1)[0] == call(1, for_apply=1)[0]).all()
    prev = sv.set_debug_flags(sv.DBG_FAIL)
    try:
        (res, _, ch, fb), st, lookups, built = counted(7)
    finally:
        sv.set_debug_flags(prev)
    assert (st.fallbacks, st.gpu_batches, lookups, built) == (1, 0, 0, 0)
    assert (res == ref).all() and (ch == ch1).all() and (fb == fb1).all()
