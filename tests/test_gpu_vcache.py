"""The verdict cache on the GPU: sv_ed25519_verify_device_cached over the
golden fixtures twice, near misses of cached rows, a table of one set, the
compaction's edges with the bitmap, clear / off / error behaviour, the tx-body
pipeline (device-resident decide, host-buffer check, a multi-chunk host call)
and two slots.
Verdicts are compared with the golden verdicts, the oracle or the CPU path;
hit flags, counters and table behaviour with the host model of csrc/vcache.h
(vcache_model.py) fed with cache keys from hashlib.  Exact equality throughout."""
import numpy as np
import pytest

import test_gpu_txresults as tr
import txaccounts_pool as ap
import txbodies_pool as tp
import txresults_pool as rp
import vcache_model as vm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 64


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def core():
    return vm.load_core()


class Rows:
    """pk, sig, a list of message byte strings and the wanted verdicts."""

    def __init__(self, pk, sig, msgs, want):
        self.pk, self.sig = np.ascontiguousarray(pk, np.uint8), np.ascontiguousarray(sig, np.uint8)
        self.msgs, self.want = list(msgs), np.asarray(want, np.uint8)
        self._keys = None

    def __len__(self):
        return len(self.msgs)

    @property
    def keys(self):
        if self._keys is None:
            self._keys = vm.cache_keys(self.pk, self.sig, self.msgs)
        return self._keys

    def take(self, idx):
        idx = np.asarray(idx, np.int64)
        r = Rows(self.pk[idx], self.sig[idx], [self.msgs[i] for i in idx], self.want[idx])
        if self._keys is not None:
            r._keys = self._keys[idx]
        return r


def _golden_rows(d):
    msgs = [d["msg"][int(o):int(o) + int(n)].tobytes() for o, n in zip(d["msg_off"], d["msg_len"])]
    return Rows(d["pk"], d["sig"], msgs, d["verdict"])


def _oracle(oracle, pk, sig, msgs):
    return np.array([oracle.oracle_ed25519_verify(sig[i].tobytes(), msgs[i], len(msgs[i]), pk[i].tobytes()) == 0
                     for i in range(len(msgs))], np.uint8)


@pytest.fixture(scope="module")
def signed(sv, dev, oracle):
    """600 GPU-signed rows with 32-byte messages, one in four corrupted; verdicts from the oracle.  Shared."""
    n = 600
    rng = np.random.default_rng(77)
    seeds = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pk, sig = tp.device_signer(sv)(seeds, msgs)
    sig = sig.copy()
    sig[1::4, 40] ^= 1
    m = [msgs[i].tobytes() for i in range(n)]
    want = _oracle(oracle, pk, sig, m)
    assert want.sum() == n - len(range(1, n, 4))
    r = Rows(pk, sig, m, want)
    r.keys
    return r


def _guarded(dev, nbytes):
    return torch.full((2 * GUARD + max(nbytes, 1),), 0xA5, dtype=torch.uint8, device=dev)


def _inner(t, nbytes):
    h = t.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + nbytes:] == 0xA5).all(), "a write outside an output array"
    return h[GUARD:GUARD + nbytes].copy()


def _call(sv, dev, rows, fixed=False, bitmap=False, msg_shift=0):
    """-> (verdict, hit, keys, bitmap words or None); every output between guard bytes.  fixed: the 32-byte form
    (msg_shift: the message array starts that many bytes off a 16-byte boundary), else offsets and lengths."""
    n = len(rows)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tpk, tsig = up(rows.pk), up(rows.sig)
    flat = np.frombuffer(b"".join(rows.msgs) + bytes(16), np.uint8)
    tmsg = up(np.concatenate([np.zeros(msg_shift, np.uint8), flat]))
    lens = np.array([len(m) for m in rows.msgs], np.uint32)
    offs = (np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]) if n else np.zeros(0)).astype(np.uint64)
    toff, tlen = up(offs), up(lens)
    words = (n + 63) // 64
    tv, th, tk, tb = _guarded(dev, n), _guarded(dev, n), _guarded(dev, 32 * n), _guarded(dev, 8 * words)
    kw = dict(fixed_msg_len=32) if fixed else dict(fixed_msg_len=0, d_msg_off=toff.data_ptr(), d_msg_len=tlen.data_ptr())
    if fixed:
        assert (lens == 32).all()
    sv.verify_device_cached(0, tpk.data_ptr(), tsig.data_ptr(), tmsg.data_ptr() + msg_shift, n, tv.data_ptr() + GUARD,
                            d_bitmap=tb.data_ptr() + GUARD if bitmap else 0, d_hit=th.data_ptr() + GUARD,
                            d_keys=tk.data_ptr() + GUARD, stream=torch.cuda.current_stream(dev).cuda_stream, **kw)
    torch.cuda.synchronize(dev)
    bm = _inner(tb, 8 * words)
    if not bitmap:
        assert (bm == 0xA5).all()
    return _inner(tv, n), _inner(th, n), _inner(tk, 32 * n).view("<u4").reshape(n, 8), bm if bitmap else None


def _stats(sv, device=0):
    st = sv.verdict_cache_stats(device)
    return [st["hits"], st["inserted"], st["dropped"]], st


class Cached:
    """The device cache at `entries` beside its model; step() runs a batch through both and compares everything."""

    def __init__(self, sv, dev, core, entries):
        self.sv, self.dev = sv, dev
        sv.set_verdict_cache(entries)
        self.model = vm.NativeCache(core, entries)
        self.lookups = 0

    def step(self, rows, **kw):
        v, hit, keys, bm = _call(self.sv, self.dev, rows, **kw)
        assert (keys == rows.keys).all(), "the engine's cache keys differ from hashlib's"
        mh, mv = self.model.run(rows.keys, rows.want)
        assert (v == rows.want).all(), "verdicts"
        assert (mv == rows.want).all(), "the model returned a verdict that no verification gives"
        assert (hit == mh).all(), "hit flags differ from the model's"
        self.lookups += len(rows)
        counters, st = _stats(self.sv)
        assert counters == self.model.counters.tolist() and st["lookups"] == self.lookups
        assert st["entries"] == self.model.entries and st["bytes"] >= 52 * self.model.entries
        if bm is not None:
            want = np.zeros(8 * ((len(rows) + 63) // 64) * 8, np.uint8)
            want[:len(rows)] = rows.want
            assert (bm == np.packbits(want, bitorder="little")).all(), "bitmap"
        return hit


# ----------------------------------------------------------------- 1. the fixtures twice
@pytest.mark.parametrize("name", ["intree", "adversarial", "msglen", "lattice_edge"])
def test_fixtures_twice(sv, dev, core, golden, name):
    rows = _golden_rows(golden[name])
    forms = [False] + ([True] if all(len(m) == 32 for m in rows.msgs) else [])
    try:
        for fixed in forms:
            c = Cached(sv, dev, core, 4096)
            hit = c.step(rows, fixed=fixed, bitmap=True)
            assert not hit.any()  # (also for rows that repeat inside the batch: the probe precedes every insert)
            hit = c.step(rows, fixed=fixed, bitmap=True)
            assert hit.any()
            if (rows.want == 0).any():
                assert hit[rows.want == 0].any()  # rejecting rows hit, and stay 0 (step compares the verdicts)
    finally:
        sv.set_verdict_cache(0)


# ----------------------------------------------------------------- 2. near misses
def test_near_misses_are_verified(sv, dev, core, golden, oracle):
    src = _golden_rows(golden["msglen"])
    pick = [i for i in range(len(src)) if src.want[i] == 1 and len(src.msgs[i]) >= 1][:64]
    if len(pick) < 64:
        more = _golden_rows(golden["valid"])
        idx = [i for i in range(len(more)) if more.want[i] == 1 and len(more.msgs[i]) >= 1][:64 - len(pick)]
        a, b = src.take(pick), more.take(idx)
        base = Rows(np.concatenate([a.pk, b.pk]), np.concatenate([a.sig, b.sig]), a.msgs + b.msgs,
                    np.concatenate([a.want, b.want]))
    else:
        base = src.take(pick)
    assert len(base) == 64
    rng = np.random.default_rng(8)
    pk, sig, msgs = [], [], []
    for i in range(64):
        m = base.msgs[i]
        for what in ("pk", "R", "S", "msg", "shorter", "longer"):
            p, s, mm = base.pk[i].copy(), base.sig[i].copy(), bytearray(m)
            bit = int(rng.integers(0, 256))
            if what == "pk":
                p[bit // 8] ^= 1 << (bit % 8)
            elif what == "R":
                s[bit // 8] ^= 1 << (bit % 8)
            elif what == "S":
                s[32 + bit // 8] ^= 1 << (bit % 8)
            elif what == "msg":
                b = int(rng.integers(0, 8 * len(m)))
                mm[b // 8] ^= 1 << (b % 8)
            elif what == "shorter":
                mm = mm[:-1]
            else:
                mm = mm + bytes([int(rng.integers(0, 256))])
            pk.append(p)
            sig.append(s)
            msgs.append(bytes(mm))
    near = Rows(np.array(pk), np.array(sig), msgs, _oracle(oracle, np.array(pk), np.array(sig), msgs))
    try:
        c = Cached(sv, dev, core, 4096)
        for _ in range(3):  # (a row that lost its claim in one pass is stored in the next)
            c.step(base)
        assert c.step(base).all()
        hit = c.step(near)
        assert not hit.any()
        assert c.step(base).all()  # the cached rows are still there, and still accept
    finally:
        sv.set_verdict_cache(0)


# ----------------------------------------------------------------- 3. one set
def test_one_set(sv, dev, core, signed):
    try:
        c = Cached(sv, dev, core, 4)
        hits = 0
        for p in range(5):
            for n in (1, 3, 4, 5, 300):
                hits += int(c.step(signed.take(range(n)), fixed=bool(p & 1)).sum())
        assert hits > 0 and c.model.counters[1] > 4  # hits happened, and more stores than the set has ways
        assert (vm.holds(c.model.tab[:, 8])).all()
    finally:
        sv.set_verdict_cache(0)


# ----------------------------------------------------------------- 4. the compaction's edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 255, 256, 257, 2 * 256 + 3])
def test_compaction_edges_and_bitmap(sv, dev, core, signed, n):
    rows = signed.take(range(n))
    patterns = {"all hit": np.ones(n, bool), "all miss": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0,
                "miss at 0": np.arange(n) != 0, "miss at n - 1": np.arange(n) != n - 1}
    try:
        c = Cached(sv, dev, core, 1 << 14)
        for name, cached in patterns.items():
            sv.verdict_cache_clear()
            c.model.clear()
            prime = rows.take(np.flatnonzero(cached))
            for _ in range(4):  # until every primed row is stored (a lost claim is stored in the next pass)
                if len(prime) and not c.step(prime, fixed=True).all():
                    continue
                break
            hit = c.step(rows, fixed=(n % 2 == 1), bitmap=True, msg_shift=4 if n == 65 else 0)
            assert (hit.astype(bool) == cached).all(), name
    finally:
        sv.set_verdict_cache(0)


# ----------------------------------------------------------------- 5. clear, off, errors
def test_clear_off_and_errors(sv, dev, core, signed):
    rows = signed.take(range(200))
    try:
        c = Cached(sv, dev, core, 4096)
        c.step(rows, fixed=True)
        assert c.step(rows, fixed=True).any()
        sv.verdict_cache_clear()
        c.model.clear()
        assert not c.step(rows, fixed=True).any()  # zero hits after the clear
        # the injected error touches nothing: afterwards the first pass over the same rows has zero hits
        sv.set_verdict_cache(4096)
        c = Cached(sv, dev, core, 4096)
        sv.set_debug_flags(sv.DBG_FAIL)
        try:
            with pytest.raises(sv.SigVerifyError):
                _call(sv, dev, rows, fixed=True)
        finally:
            sv.set_debug_flags(0)
        assert not c.step(rows, fixed=True).any()
        # without verdicts (PREP_ONLY, a knob of the one-lane throughput kernels) the cache is bypassed: nothing is
        # looked up or inserted
        before = _stats(sv)[1]
        prev = sv.set_kernel_path(sv.PATH_THROUGHPUT)
        sv.set_debug_flags(sv.DBG_PREP_ONLY | sv.DBG_NO_QUAD)
        try:
            _, hit, keys, _ = _call(sv, dev, signed.take(range(300, 400)), fixed=True)
        finally:
            sv.set_debug_flags(0)
            sv.set_kernel_path(prev)
        assert not hit.any() and (keys == signed.keys[300:400]).all() and _stats(sv)[1] == before
        assert not c.step(signed.take(range(300, 400)), fixed=True).any()
    finally:
        sv.set_verdict_cache(0)
    # capacity 0: the cached call is verify_device, with no hit, and the slot holds no cache memory
    st = sv.verdict_cache_stats(0)
    assert st["bytes"] == 0 and st["entries"] == 0 and st["lookups"] == 0
    for fixed in (True, False):
        v, hit, keys, bm = _call(sv, dev, rows, fixed=fixed, bitmap=True)
        tv = torch.zeros(len(rows), dtype=torch.uint8, device=dev)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        tpk, tsig, tmsg = up(rows.pk), up(rows.sig), up(np.frombuffer(b"".join(rows.msgs), np.uint8))
        sv.verify_device(0, tpk.data_ptr(), tsig.data_ptr(), tmsg.data_ptr(), len(rows), tv.data_ptr(),
                         stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert (v == tv.cpu().numpy()).all() and (v == rows.want).all() and not hit.any()
        assert (keys == rows.keys).all()
    assert sv.verdict_cache_stats(0)["bytes"] == 0


# ----------------------------------------------------------------- 6. the pipeline
def _pairs(s, digests, oracle):
    """The pipeline's two verify launches over the set, in the engine's order (body, signature, candidate):
    (keys, verdicts, body of each pair) of the ed25519 pairs and of the payload pairs."""
    hint = np.ascontiguousarray(s["hint"]).view(np.uint8).reshape(-1, 4)
    sig = np.ascontiguousarray(s["sig"]).reshape(-1, 64)
    key, pkey = np.ascontiguousarray(s["key"]).reshape(-1, 32), np.ascontiguousarray(s["pkey"]).reshape(-1, 32)
    pay, plen = np.ascontiguousarray(s["pkey_payload"]).reshape(-1, 64), s["pkey_len"]
    ed, pl = [], []
    for t in range(s["nb"]):
        sigs = range(int(s["sig_begin"][t]), int(s["sig_begin"][t + 1]))
        for i in sigs:
            for k in range(int(s["key_begin"][t]), int(s["key_begin"][t + 1])):
                if key[k, 28:].tobytes() == hint[i].tobytes():
                    ed.append((key[k].tobytes(), sig[i].tobytes(), bytes(digests[t]), t))
        for i in sigs:
            for q in range(int(s["pkey_begin"][t]), int(s["pkey_begin"][t + 1])):
                n = int(plen[q])
                tail = pay[q, n - min(n, 4):n].tobytes() + bytes(4 - min(n, 4))
                if bytes(a ^ b for a, b in zip(tail, pkey[q, 28:].tobytes())) == hint[i].tobytes():
                    pl.append((pkey[q].tobytes(), sig[i].tobytes(), pay[q, :n].tobytes(), t))
    out = []
    for triples in (ed, pl):
        keys = np.array([vm.cache_key(*x[:3]) for x in triples], np.uint32).reshape(-1, 8)
        want = np.array([oracle.oracle_ed25519_verify(x[1], x[2], len(x[2]), x[0]) == 0 for x in triples], np.uint8)
        out.append((keys, want, np.array([x[3] for x in triples], np.int64)))
    return out


def test_pipeline_decide_device_and_check_host(sv, dev, core, oracle):
    bld = rp.RBuilder(5)
    ap.edge_cases(bld)
    ap.random_pool(bld, 300)
    rp.assign(bld, 99)
    s = bld.finish(tp.device_signer(sv), oracle)
    a, kw = rp.explicit(s)
    cpu = sv.decide_txbodies_cpu(*a, protocol_version=21, want_checks=True, bad_cap=s["nb"], **kw)
    ca, ckw = ap.explicit_args(s)
    off_dec = tr._decide_device(sv, dev, s, "explicit", bad_cap=s["nb"])
    off_chk = sv.check_txbodies(*ca, protocol_version=21, device=0, **ckw)
    tr._same(off_dec, cpu)
    (ek, ev, eb_), (pk_, pv, _) = _pairs(s, cpu.digests, oracle)
    assert len(ek) > 300 and len(pk_) > 0  # both verify launches run
    # one byte of one body with ed25519 pairs changes: its contents hash, so the messages of exactly its pairs
    # (a body that is OK now and whose pairs all verify: afterwards none of them does)
    t = next(int(b) for b in np.unique(eb_)
             if cpu.body_code[b] == 0 and ev[eb_ == b].all() and s["len"][b] > 0 and (eb_ == b).sum() >= 1)
    s3 = dict(s)
    s3["bodies"] = s["bodies"].copy()
    s3["bodies"][int(s["off"][t])] ^= 0x40
    a3, kw3 = rp.explicit(s3)
    cpu3 = sv.decide_txbodies_cpu(*a3, protocol_version=21, want_checks=True, bad_cap=s["nb"], **kw3)
    assert cpu3.digests[t].tobytes() != cpu.digests[t].tobytes()
    (ek3, ev3, eb3), (pk3, pv3, _) = _pairs(s3, cpu3.digests, oracle)
    model = vm.NativeCache(core, 1 << 14)

    def model_pass(e, p):
        h = [model.run(*e[:2])[0], model.run(*p[:2])[0]]
        return h

    try:
        sv.set_verdict_cache(1 << 14)
        # pass 1, device-resident decide: every output as with the cache off, no hit
        tr._same(tr._decide_device(sv, dev, s, "explicit", bad_cap=s["nb"]), off_dec)
        h = model_pass((ek, ev), (pk_, pv))
        assert not h[0].any() and not h[1].any()
        counters, st = _stats(sv)
        assert counters == model.counters.tolist() and counters[0] == 0 and st["lookups"] == len(ek) + len(pk_)
        # pass 2, host-buffer check: identical outputs, and the model's hits: every pair but the dropped inserts
        # whose key no other pair stored
        got = sv.check_txbodies(*ca, protocol_version=21, device=0, **ckw)
        for x, y in zip(got, off_chk):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        h = model_pass((ek, ev), (pk_, pv))
        counters, st = _stats(sv)
        assert counters == model.counters.tolist() and st["lookups"] == 2 * (len(ek) + len(pk_))
        assert counters[0] == int(h[0].sum() + h[1].sum()) >= 0.9 * (len(ek) + len(pk_))
        for _ in range(2):  # (the dropped ones are stored now)
            tr._same(tr._decide_device(sv, dev, s, "explicit", bad_cap=s["nb"]), off_dec)
            h = model_pass((ek, ev), (pk_, pv))
        assert h[0].all() and h[1].all() and _stats(sv)[0] == model.counters.tolist()
        # pass 3: the changed body
        before = int(model.counters[0])
        got3 = tr._decide_device(sv, dev, s3, "explicit", bad_cap=s["nb"])
        tr._same(got3, cpu3)
        assert got3.body_code[t] != 0 and (np.delete(got3.body_code, t) == np.delete(off_dec.body_code, t)).all()
        h = model_pass((ek3, ev3), (pk3, pv3))
        assert (h[0].astype(bool) == (eb3 != t)).all() and h[1].all()  # exactly that body's pairs miss
        assert _stats(sv)[0] == model.counters.tolist()
        assert int(model.counters[0]) - before == len(ek3) + len(pk3) - int((eb3 == t).sum())
    finally:
        sv.set_verdict_cache(0)


def test_multi_chunk_host_call_twice(sv, dev):
    """The shape of test_gpu_txresults' multi-chunk test (61 expanded key rows per body cross a chunk's key bound
    three times): with the cache on every chunk waits once more, for its miss count, and the outputs stay those of
    the cache-off call; the second call finds what the first one stored."""
    nb = 12000
    s, (code, fail) = tr._big(sv, nb, 7, 60, 2)
    assert 61 * nb > 2 * (1 << 18)
    off = tr._decide_host(sv, s, device=0, bad_cap=nb, want_checks=True)
    try:
        sv.set_verdict_cache(1 << 16)
        first = tr._decide_host(sv, s, device=0, bad_cap=nb, want_checks=True)
        st1 = sv.verdict_cache_stats(0)
        second = tr._decide_host(sv, s, device=0, bad_cap=nb, want_checks=True)
        st2 = sv.verdict_cache_stats(0)
    finally:
        sv.set_verdict_cache(0)
    for got in (first, second):
        tr._same(got, off)
        assert (got.body_code == code).all() and (got.body_fail == fail).all()
    assert st1["lookups"] > 0 and st1["inserted"] > 0 and st2["lookups"] == 2 * st1["lookups"]
    assert st1["hits"] + st1["inserted"] + st1["dropped"] == st1["lookups"]
    assert st2["hits"] - st1["hits"] >= 0.9 * st1["lookups"]


# ----------------------------------------------------------------- 7. two slots
def test_two_slots_each_cache_its_own_slice(sv, dev):
    s, (code, fail) = tr._big(sv, 2400, 50, 2, 1)
    try:
        sv.set_verdict_cache(1 << 15)
        one = tr._decide_host(sv, s, device=0, bad_cap=2400, want_checks=True)
        pairs = sv.verdict_cache_stats(0)["lookups"]
        assert pairs > 0
        sv.set_device_map([0, 0])
        try:
            sv.set_min_shard(1000)
            assert sv.device_count() == 2
            first = tr._decide_host(sv, s, bad_cap=2400, want_checks=True)
            st1 = [sv.verdict_cache_stats(g) for g in (0, 1)]
            second = tr._decide_host(sv, s, bad_cap=2400, want_checks=True)
            st2 = [sv.verdict_cache_stats(g) for g in (0, 1)]
        finally:
            sv.set_min_shard(0)
            sv.set_device_map([])
    finally:
        sv.set_verdict_cache(0)
    for got in (first, second):  # global results, equal to one slot's
        tr._same(got, one)
        assert (got.body_code == code).all() and (got.body_fail == fail).all()
    assert st1[0]["lookups"] + st1[1]["lookups"] == pairs
    for g in (0, 1):
        # a slot sees its own slice only: no hit in the first call, and in the second at least what it stored of
        # the first (a stored verdict is evicted only from a full set: 2^15 entries for a few thousand pairs)
        assert st1[g]["lookups"] > 0 and st1[g]["hits"] == 0 and st1[g]["inserted"] > 0
        assert st2[g]["lookups"] == 2 * st1[g]["lookups"]
        assert st1[g]["inserted"] <= st2[g]["hits"] <= st1[g]["lookups"]
        assert st2[g]["hits"] >= 0.9 * st1[g]["lookups"]
