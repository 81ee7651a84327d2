"""The verdict cache's feed on the GPU: keyed latency-lane batches journaled and
drained into the slot's table, the lookups, the overflow, what drops the
journal, keyed bulk batches behind the cache, a tx-body call that finds what
the lane verified, and two slots.  Table contents (through
sv_verdict_cache_lookup), hit flags and every counter are compared with the
host model of csrc/vjournal.h and csrc/vcache.h (vcache_feed_model.py) fed with
cache keys from hashlib; verdicts with the oracle or the CPU path.  Exact
equality throughout; every device output sits between guard bytes."""
import numpy as np
import pytest

import test_gpu_txresults as tr
import test_gpu_vcache as gv
import txaccounts_pool as ap
import txbodies_pool as tp
import txresults_pool as rp
import vcache_feed_model as fm
import vcache_model as vm
from test_gpu_vcache import dev, signed  # noqa: F401  (fixtures: the 600 GPU-signed rows idiom)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LANE, BULK = 1, 2


@pytest.fixture(scope="module")
def cores():
    return vm.load_core(), fm.load_feed_core()


@pytest.fixture(autouse=True)
def _feed_off_afterwards(sv):
    yield
    sv.set_verdict_cache_feed(0)
    sv.set_verdict_cache(0)


def _flat(rows):
    lens = np.array([len(m) for m in rows.msgs], np.uint32)
    offs = np.zeros(len(lens), np.uint64)
    if len(lens):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(rows.msgs) + bytes(1), np.uint8), offs, lens


def _keyed(sv, rows, device=0):
    """One keyed host batch (the latency lane for n <= 12,288 under SV_PATH_AUTO): verdicts and keys as always."""
    msg, offs, lens = _flat(rows)
    v, k = sv.verify_batch_keyed(rows.pk.reshape(-1, 32), rows.sig.reshape(-1, 64), msg, offs, lens, device=device)
    assert (v == rows.want).all(), "verdicts"
    assert (k.reshape(-1).view("<u4").reshape(-1, 8) == rows.keys.reshape(-1, 8)).all(), "keys differ from hashlib's"


def _lookup_both(sv, dev, keys, device=0):
    """The host form and the device form (its output between guards); they agree."""
    keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 8)
    n = len(keys)
    host = sv.verdict_cache_lookup(keys, device=device)
    tk = torch.from_numpy(keys.view(np.uint8).reshape(-1).copy() if n else np.zeros(32, np.uint8)).to(dev)
    out = gv._guarded(dev, n)
    sv.verdict_cache_lookup_device(device, tk.data_ptr(), n, out.data_ptr() + gv.GUARD,
                                   stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    got = gv._inner(out, n)
    assert (got == host).all(), "the device form of the lookup differs from the host form"
    return host


class Fed:
    """The device cache with its feed beside the model; every step runs through both."""

    def __init__(self, sv, dev, cores, entries, sources, journal_rows=0, device=0):
        self.sv, self.dev, self.device = sv, dev, device
        sv.set_verdict_cache(entries)
        sv.set_verdict_cache_feed(sources, journal_rows)
        self.model = fm.NativeFeed(cores[0], cores[1], entries, journal_rows or fm.DEFAULT_ROWS)
        self.lookups = 0

    def lane(self, rows, fed=True):
        _keyed(self.sv, rows, self.device)
        if fed:
            self.model.append(rows.keys, rows.want)

    def sync(self):
        self.sv.verdict_cache_sync(self.device)
        self.model.drain()

    def same(self, keys):
        """Table contents by lookup, and every counter."""
        look = _lookup_both(self.sv, self.dev, keys, self.device)
        self.model.drain()  # (a lookup drains first)
        assert (look == self.model.lookup(keys)).all(), "the table differs from the model's"
        self.counters()
        return look

    def counters(self):
        st = self.sv.verdict_cache_stats(self.device)
        assert {f: st[f] for f in fm.FED} == self.model.fed_counters()
        assert [st["hits"], st["inserted"], st["dropped"]] == self.model.counters.tolist()
        assert st["lookups"] == self.lookups  # (neither a drain nor a lookup moves it)
        return st

    def cached_pass(self, rows, **kw):
        v, hit, keys, _ = gv._call(self.sv, self.dev, rows, **kw)
        self.model.drain()  # (ahead of the probe)
        mh, _ = self.model.run(rows.keys, rows.want)
        assert (v == rows.want).all() and (keys == rows.keys).all()
        assert (hit == mh).all(), "hit flags differ from the model's"
        self.lookups += len(rows)
        self.counters()
        return hit


# ----------------------------------------------------------------- 1. the lane feeds the table
def test_lane_feeds_the_table(sv, dev, cores, signed):
    rows, never = signed.take(range(40)), signed.take(range(500, 508))
    c = Fed(sv, dev, cores, 64, LANE)
    c.lane(rows)
    c.sync()
    look = c.same(np.concatenate([rows.keys, never.keys]))
    assert (look[40:] == sv.VC_MISS).all() and (look[:40] != sv.VC_MISS).sum() >= 15
    held = look[:40] != sv.VC_MISS
    assert (look[:40][held] == rows.want[held]).all() and (rows.want[held] == 0).any()  # rejects are fed too
    st = c.counters()
    assert st["fed_rows"] == 40 and st["fed_inserted"] + st["fed_dropped"] == 40 and st["fed_present"] == 0
    hit = c.cached_pass(rows, fixed=True)
    assert (hit.astype(bool) == held).all() and hit.sum() == st["fed_inserted"]


# ----------------------------------------------------------------- 2. one set
def test_one_set(sv, dev, cores, signed):
    c = Fed(sv, dev, cores, 4, LANE)
    first, second = signed.take(range(5)), signed.take([5, 6, 2, 7])  # (row 2 again)
    everything = signed.take(range(8)).keys
    c.lane(first)
    c.sync()
    look = c.same(everything)
    assert 1 <= (look != sv.VC_MISS).sum() <= 4
    c.lane(second)
    c.sync()
    look = c.same(everything)
    assert 2 <= (look != sv.VC_MISS).sum() <= 4
    st = c.counters()
    assert st["fed_rows"] == 9 and st["fed_present"] + st["fed_inserted"] + st["fed_dropped"] == 9


# ----------------------------------------------------------------- 3. edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_drain_and_lookup_edges(sv, dev, cores, signed, n):
    rows = signed.take(range(n))
    c = Fed(sv, dev, cores, 16, LANE)
    c.lane(rows)
    c.sync()
    look = c.same(rows.keys)  # a lookup of n keys, both forms, the device form between guards
    assert len(look) == n and (look != sv.VC_MISS).sum() == min(c.counters()["fed_inserted"], 16)
    st = c.counters()
    assert st["fed_rows"] == n and st["fed_inserted"] + st["fed_dropped"] == n
    # a second drain of the same size against the table the first one left, and a lookup of other sizes
    c.lane(signed.take(range(300, 300 + n)))
    c.same(signed.take(range(300, 301 + n)).keys)
    c.same(rows.keys)


# ----------------------------------------------------------------- 4. present rows evict nothing
def test_present_rows_evict_nothing(sv, dev, cores, signed):
    """Feed a batch, sync, note the lookup; feed it again, sync: fed_present is what the table held, and what was
    held answers as before.  The rows the first drain DROPPED (they lost a claim) are not present: they compete
    again, so the second lookup may differ from the first exactly there -- a miss that became a verdict where the
    set had room, and in a crowded table an eviction, both as the model says (same()).  Once every row is held,
    feeding the batch again leaves the lookup identical and stores nothing."""
    rows = signed.take(range(100, 140))
    c = Fed(sv, dev, cores, 1024, LANE)
    c.lane(rows)
    c.sync()
    look = c.same(rows.keys)
    was = look != sv.VC_MISS
    c.lane(rows)
    c.sync()
    again = c.same(rows.keys)
    st = c.counters()
    assert st["fed_present"] == int(was.sum())
    assert (again[was] == look[was]).all() and (look[again != look] == sv.VC_MISS).all()
    assert (again != sv.VC_MISS).all()  # (256 sets for 40 keys: the rows dropped at first found room)
    c.lane(rows)
    c.sync()
    third = c.same(rows.keys)
    after = c.counters()
    assert (third == again).all() and (third == rows.want).all()
    assert after["fed_present"] - st["fed_present"] == 40
    assert after["fed_inserted"] == st["fed_inserted"] and after["fed_dropped"] == st["fed_dropped"]
    # 16 sets for 40 keys: present is still what the table held; a key held before is still held unless a row
    # that was not present took its slot, which same() compares with the model entry by entry
    c = Fed(sv, dev, cores, 64, LANE)
    c.lane(rows)
    c.sync()
    look = c.same(rows.keys)
    was = look != sv.VC_MISS
    before = c.counters()
    c.lane(rows)
    c.sync()
    again = c.same(rows.keys)
    st = c.counters()
    assert st["fed_present"] - before["fed_present"] == int(was.sum())
    lost = was & (again == sv.VC_MISS)
    assert int(lost.sum()) <= st["fed_inserted"] - before["fed_inserted"]  # only a store evicts
    assert (again[was & ~lost] == look[was & ~lost]).all()


# ----------------------------------------------------------------- 5. overflow
def test_overflow_keeps_the_first_32_rows(sv, dev, cores, signed):
    c = Fed(sv, dev, cores, 4096, LANE, journal_rows=32)
    for b in range(3):
        c.lane(signed.take(range(200 + 20 * b, 220 + 20 * b)))
    st = c.counters()
    assert st["fed_rows"] == 32 and st["fed_overflow"] == 28
    c.sync()
    look = c.same(signed.take(range(200, 260)).keys)
    assert (look[32:] == sv.VC_MISS).all()
    st = c.counters()
    assert (look[:32] != sv.VC_MISS).sum() == st["fed_inserted"] >= 30 and st["fed_inserted"] + st["fed_dropped"] == 32


# ----------------------------------------------------------------- 6. feed off, and unkeyed batches
def test_feed_off_and_unkeyed_batches_append_nothing(sv, dev, cores, signed):
    rows = signed.take(range(50))
    c = Fed(sv, dev, cores, 256, 0)
    c.lane(rows, fed=False)
    c.sync()
    assert (c.same(rows.keys) == sv.VC_MISS).all()
    assert all(c.counters()[f] == 0 for f in fm.FED)
    c = Fed(sv, dev, cores, 256, LANE)
    msg, offs, lens = _flat(rows)
    assert (sv.verify_batch(rows.pk, rows.sig, msg, offs, lens, device=0) == rows.want).all()
    c.sync()
    assert (c.same(rows.keys) == sv.VC_MISS).all()
    assert all(c.counters()[f] == 0 for f in fm.FED)
    # an erring keyed batch appends nothing either
    sv.set_debug_flags(sv.DBG_FAIL)
    try:
        with pytest.raises(sv.SigVerifyError):
            sv.verify_batch_keyed(rows.pk, rows.sig, msg, offs, lens, device=0)
    finally:
        sv.set_debug_flags(0)
    assert (c.same(rows.keys) == sv.VC_MISS).all() and c.counters()["fed_rows"] == 0


# ----------------------------------------------------------------- 7. clear, resize, feed setter, off
def test_clear_resize_setter_and_off_drop_the_journal(sv, dev, cores, signed):
    rows = signed.take(range(30))
    c = Fed(sv, dev, cores, 256, LANE)
    c.lane(rows)
    sv.verdict_cache_clear()
    c.model.clear()
    assert (c.same(rows.keys) == sv.VC_MISS).all()
    st = c.counters()
    assert st["fed_rows"] == 30 and st["fed_inserted"] == 0  # (the counters stay, the rows are gone)
    c.lane(rows)
    c = Fed(sv, dev, cores, 256, LANE)  # sv_set_verdict_cache: a new table, journal and counters
    assert (c.same(rows.keys) == sv.VC_MISS).all() and c.counters()["fed_rows"] == 0
    c.lane(rows)
    sv.set_verdict_cache_feed(LANE)
    c.model.drop()
    assert (c.same(rows.keys) == sv.VC_MISS).all() and c.counters()["fed_rows"] == 30
    c.lane(rows)  # ... and the feed still works afterwards
    assert (c.same(rows.keys) != sv.VC_MISS).sum() >= 25
    # the cache off: sync and lookup succeed and do nothing
    sv.set_verdict_cache(0)
    _keyed(sv, rows)
    sv.verdict_cache_sync(0)
    assert (_lookup_both(sv, dev, rows.keys) == sv.VC_MISS).all()
    st = sv.verdict_cache_stats(0)
    assert st["bytes"] == 0 and all(st[f] == 0 for f in fm.FED)


# ----------------------------------------------------------------- 8. bulk keyed batches
def test_bulk_keyed_batches_behind_the_cache(sv, dev, cores, signed):
    rows = signed.take(range(300))
    prev = sv.set_kernel_path(sv.PATH_THROUGHPUT)
    try:
        c = Fed(sv, dev, cores, 4096, BULK)
        for call in range(2):
            _keyed(sv, rows)  # verdicts against the oracle's, keys against hashlib's
            hit, _ = c.model.run(rows.keys, rows.want)
            c.lookups += 300
            st = c.counters()  # hits, inserted, dropped and lookups equal the model's
            assert (st["hits"] == 0) if call == 0 else (st["hits"] == int(hit.sum()) >= 250)
        assert all(st[f] == 0 for f in fm.FED)
        # the bit clear: the same two calls move no counter
        c = Fed(sv, dev, cores, 4096, LANE)
        for call in range(2):
            _keyed(sv, rows)
        st = c.counters()
        assert st["lookups"] == 0 and all(st[f] == 0 for f in fm.FED)
    finally:
        sv.set_kernel_path(prev)


# ----------------------------------------------------------------- 9. the scenario
def multisig_set(signer, oracle, nb=24):
    """nb bodies over six 2-of-3 style accounts: every signer an ed25519 key, every signature 64 bytes, one
    signature in five corrupted -- so every pair of a decide call is an ed25519 pair."""
    bld = rp.RBuilder(9)
    for a in range(6):
        bld.account(ap.ed(1 + a), (1, 1, 2, 3), [(ap.ED, 1, ap.ed(11 + a)), (ap.ED, 2, ap.ed(21 + a))])
    for t in range(nb):
        b = bld.body(length=40 + t)
        a = t % 6
        pos = b.use(a)
        b.sig_ed(1 + a)
        b.sig_ed(11 + a, corrupt=(t % 5 == 0))
        if t % 3 == 0:
            b.sig_ed(21 + a)
        b.acheck(pos, 1 + t % 3)
        if t % 4 == 0:
            pos2 = b.use((a + 1) % 6)
            b.sig_ed(1 + (a + 1) % 6)
            b.acheck(pos2, 1, role=rp.OP)
    return bld.finish(signer, oracle)


def scenario_pairs(sv, s):
    """(pk, sig, contents hash) of every pair, in the engine's order, by the hinted CPU form; with its verdicts."""
    a, _ = rp.explicit(s)
    pb, ps, pk, pv, dig = sv.verify_txbodies_hinted_cpu(*a[:10])
    body = np.repeat(np.arange(s["nb"]), np.diff(pb.astype(np.int64)))
    key = np.ascontiguousarray(s["key"]).reshape(-1, 32)[pk]
    sig = np.ascontiguousarray(s["sig"]).reshape(-1, 64)[ps]
    msgs = [dig[t].tobytes() for t in body]
    return gv.Rows(key, sig, msgs, pv)


def test_scenario_tx_bodies_find_what_the_lane_verified(sv, dev, cores, oracle):
    s = multisig_set(tp.device_signer(sv), oracle)
    assert s["nq"] == 0 and (np.asarray(s["sig_len"]) == 64).all()
    pairs = scenario_pairs(sv, s)
    n = len(pairs)
    assert n >= 48 and 0 < pairs.want.sum() < n
    a, kw = rp.explicit(s)
    cpu = sv.decide_txbodies_cpu(*a, protocol_version=21, want_checks=True, bad_cap=s["nb"], **kw)
    assert len(set(cpu.body_code.tolist())) >= 2
    for sources in (LANE, 0):
        c = Fed(sv, dev, cores, 1 << 18, sources)  # (no two of the pairs name one slot: the model drops none)
        c.lane(pairs, fed=bool(sources))
        got = tr._decide_device(sv, dev, s, "explicit", bad_cap=s["nb"])
        tr._same(got, cpu)
        c.model.drain()
        hit, _ = c.model.run(pairs.keys, pairs.want)
        c.lookups += n
        st = c.counters()
        assert st["hits"] == int(hit.sum()) == (n if sources else 0)
        assert st["fed_rows"] == (n if sources else 0) and st["fed_dropped"] == 0


# ----------------------------------------------------------------- 10. two slots
def test_two_slots_a_lane_batch_feeds_its_own_slot(sv, dev, cores, signed):
    rows = signed.take(range(400, 440))
    sv.set_device_map([0, 0])
    try:
        assert sv.device_count() == 2
        c = Fed(sv, dev, cores, 256, LANE, device=1)
        c.lane(rows)
        c.sync()
        look = c.same(rows.keys)
        assert (look != sv.VC_MISS).sum() >= 35
        assert (_lookup_both(sv, dev, rows.keys, device=0) == sv.VC_MISS).all()
        st0 = sv.verdict_cache_stats(0)
        assert all(st0[f] == 0 for f in fm.FED) and c.counters()["fed_rows"] == 40
    finally:
        sv.set_verdict_cache_feed(0)
        sv.set_verdict_cache(0)
        sv.set_device_map([])


# ----------------------------------------------------------------- 11. the mirror
def envelope_pairs(s):
    """Every (key, signature, message) the set's envelopes pair by hint -- ed25519 keys: the account ids and the
    plain signers -- in envelope order, the fee bump's outer signatures after its inner ones; and the payload
    pairs (signer key, signature, payload), which the admission batch below does not carry."""
    envs, dsig, signers, accounts = s["envs"], s["rest"][0], s["rest"][2], s["rest"][3]
    keys = {bytes(a["account_id"]) for a in accounts[:s["naccounts"]]}
    keys |= {bytes(g["key"]) for g in signers if g["type"] == 0 and g["weight"]}
    by_hint = {k[28:]: k for k in keys}
    assert len(by_hint) == len(keys)
    pay = {bytes(a ^ b for a, b in zip(bytes(g["key"])[28:], bytes(g["payload"])[g["payload_len"] - 4:g["payload_len"]])):
           (bytes(g["key"]), bytes(g["payload"])[:g["payload_len"]]) for g in signers if g["type"] == 3}
    ed, pl = [], []
    for t in range(s["n"]):
        e = envs[t]
        spans = [(int(e["sig_off"]), int(e["nsigs"]), s["contents_hash"][t].tobytes())]
        if e["fee_bump"]:
            spans.append((int(e["outer_off"]), int(e["nouter"]), s["fee_bump_hash"][t].tobytes()))
        for off, cnt, msg in spans:
            for d in dsig[off:off + cnt]:
                h = bytes(d["hint"])
                if h in by_hint:
                    ed.append((by_hint[h], bytes(d["sig"]), msg))
                if h in pay:
                    pl.append((pay[h][0], bytes(d["sig"]), pay[h][1]))
    return ed, pl


def _pair_rows(triples, oracle):
    pk = np.array([np.frombuffer(x[0], np.uint8) for x in triples], np.uint8).reshape(-1, 32)
    sig = np.array([np.frombuffer(x[1], np.uint8) for x in triples], np.uint8).reshape(-1, 64)
    msgs = [x[2] for x in triples]
    return gv.Rows(pk, sig, msgs, gv._oracle(oracle, pk, sig, msgs))


def test_mirror_admission_batch_warms_the_envelope_check(sv, dev, cores, oracle):
    import ctypes

    import envelope_bodies as eb
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_set_keyed_threshold.argtypes = [ctypes.c_size_t]
    s = eb.build_set(50, 37, tp.device_signer(sv), with_payload=True)
    ed, pl = envelope_pairs(s)
    rows, prows = _pair_rows(ed, oracle), _pair_rows(pl, oracle)
    assert len(rows) >= 256 and 0 < rows.want.sum() < len(rows) and len(prows) == 50 and prows.want.all()

    def call(prefetch):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch)

    ref = call(0)
    assert (ref[0]["code"] == s["expect"]).all()
    msg, offs, lens = _flat(rows)
    vp = ctypes.c_void_p
    for sources in (LANE, 0):
        c = Fed(sv, dev, cores, 1 << 16, sources)
        host.svh_cache_clear()  # (the mirror's own cache: every row is a miss there, so the batch reaches the engine)
        host.svh_set_keyed_threshold(256)
        out = np.full(len(rows), 7, np.uint8)
        rc = host.svh_verify_sig_batch(vp(rows.pk.ctypes.data), vp(rows.sig.ctypes.data), None, vp(msg.ctypes.data),
                                       vp(offs.ctypes.data), vp(lens.ctypes.data), ctypes.c_size_t(len(rows)),
                                       vp(out.ctypes.data))
        assert rc == 0 and (out == rows.want).all()
        if sources:
            c.model.append(rows.keys, rows.want)
        res, _, ch, fb = call(8)
        assert (res == ref[0]).all() and (ch == ref[2]).all() and (fb == ref[3]).all()
        c.model.drain()
        hit, _ = c.model.run(rows.keys, rows.want)
        phit, _ = c.model.run(prows.keys, prows.want)
        c.lookups += len(rows) + len(prows)
        st = c.counters()
        assert st["hits"] == int(hit.sum()) + int(phit.sum())
        assert (st["hits"] > 0.9 * len(rows)) if sources else (st["hits"] == 0)
    host.svh_cache_clear()
