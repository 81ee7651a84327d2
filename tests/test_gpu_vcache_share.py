"""One view across slots on the GPU (sv_set_verdict_cache_share): two slots on
one card; what a cached launch on one slot verified reaches the other slot's
table through its journal, a keyed lane batch reaches every journal, the bounds,
what drops pending rows, the default, which shares nothing, and a sharded
host-buffer decide call whose bodies come back rotated by half.  Table contents
(through sv_verdict_cache_lookup, both forms), hit flags and every fed_* and
shared_* counter are compared with the host model of csrc/vshare.h,
csrc/vjournal.h and csrc/vcache.h (vshare_model.py) fed with cache keys from
hashlib; verdicts with the oracle.  Exact equality throughout; every device
output sits between guard bytes.

The device forms used here return with their work queued; every step below waits
for the stream before the next one, so an export is complete when the next cache
entry point comes by and the model passes everything on ahead of every step."""
import ctypes
import threading

import numpy as np
import pytest

import test_gpu_txresults as tr
import test_gpu_vcache as gv
import test_gpu_vcache_feed as gf
import txaccounts_pool as ap
import txbodies_pool as tp
import txresults_pool as rp
import vcache_feed_model as fm
import vcache_model as vm
import vshare_model as sm
from test_gpu_vcache import dev, signed  # noqa: F401  (fixtures: the 600 GPU-signed rows idiom)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FEED, STORES = 1, 2
LANE = 1


@pytest.fixture(scope="module")
def cores():
    return vm.load_core(), fm.load_feed_core(), sm.load_share_core()


@pytest.fixture(autouse=True)
def _two_slots_and_everything_back(sv, dev):
    sv.set_device_map([0, 0])
    assert sv.device_count() == 2
    yield
    sv.set_verdict_cache_share(0)
    sv.set_verdict_cache_feed(0)
    sv.set_verdict_cache(0)
    sv.set_device_map([])


class _OnSlot:
    """gv._call names slot 0; this hands its launch to another slot."""

    def __init__(self, sv, device):
        self._sv, self._device = sv, device

    def __getattr__(self, name):
        return getattr(self._sv, name)

    def verify_device_cached(self, _device, *a, **kw):
        return self._sv.verify_device_cached(self._device, *a, **kw)


def pinned_bound(journal_rows):
    """include/stellar_sigverify.h: 4 * (33 * journal_rows rounded up to 4096) bytes per slot."""
    return 4 * ((33 * journal_rows + 4095) // 4096) * 4096


class Shared:
    """The two device slots beside the model; every step runs through both."""

    def __init__(self, sv, dev, cores, entries, share, sources=0, journal_rows=0):
        self.sv, self.dev = sv, dev
        sv.set_verdict_cache(entries)
        sv.set_verdict_cache_feed(sources, journal_rows)
        sv.set_verdict_cache_share(share)
        self.rows = journal_rows or fm.DEFAULT_ROWS
        self.model = sm.NativeShare(cores, 2, entries, self.rows, stores=bool(share & STORES),
                                    feed=bool(share & FEED) and bool(sources & LANE))
        self.lookups = [0, 0]

    def launch(self, a, rows, fixed=True):
        v, hit, keys, _ = gv._call(_OnSlot(self.sv, a), self.dev, rows, fixed=fixed)
        self.model.pass_on(wait=True)
        mh = self.model.cached_pass(a, rows.keys, rows.want)
        assert (v == rows.want).all(), "verdicts differ from the oracle's"
        assert (keys == rows.keys).all()
        assert (hit == mh).all(), "hit flags differ from the model's"
        self.lookups[a] += len(rows)
        return hit

    def lane(self, a, rows):
        gf._keyed(self.sv, rows, a)
        self.model.lane(a, rows.keys, rows.want)

    def sync(self, b):
        self.sv.verdict_cache_sync(b)
        self.model.sync(b)

    def counters(self, b):
        st = self.sv.verdict_cache_stats(b)
        self.model.pass_on(wait=True)
        slot = self.model.slots[b]
        assert {f: st[f] for f in fm.FED} == slot.fed_counters()
        assert [st["hits"], st["inserted"], st["dropped"]] == slot.counters.tolist()
        assert {f: st[f] for f in sm.SHARED} == self.model.shared_counters(b)
        assert st["lookups"] == self.lookups[b]
        assert st["shared_pinned_bytes"] <= pinned_bound(self.rows)
        # the counters' invariant
        assert st["fed_rows"] == st["fed_present"] + st["fed_inserted"] + st["fed_dropped"] + self.model.held(b)
        return st

    def same(self, b, keys):
        look = gf._lookup_both(self.sv, self.dev, keys, device=b)
        self.model.pass_on(wait=True)
        self.model.slots[b].drain()  # (a lookup drains first)
        assert (look == self.model.slots[b].lookup(keys)).all(), "slot %d's table differs from the model's" % b
        self.counters(b)
        return look


# ----------------------------------------------------------------- 1. a launch on slot 0 teaches slot 1
@pytest.mark.parametrize("n", [1, 7, 127, 128, 129, 300])
def test_a_launch_on_slot_0_teaches_slot_1(sv, dev, cores, signed, n):
    rows = signed.take(range(n))
    assert n < 4 or 0 < rows.want.sum() < n  # accepts and rejects mixed
    c = Shared(sv, dev, cores, 4096, STORES)
    assert not c.launch(0, rows).any()
    torch.cuda.synchronize(dev)
    c.sync(1)
    look = c.same(1, rows.keys)
    st1, st0 = c.counters(1), c.counters(0)
    assert st0["shared_out"] == n and st0["shared_skipped"] == 0 and st0["shared_in"] == 0
    assert st1["shared_in"] == n == st1["fed_rows"] and st1["fed_inserted"] + st1["fed_dropped"] == n
    assert st1["shared_out"] == 0 and st1["lookups"] == 0
    held = look != sv.VC_MISS
    assert held.sum() == st1["fed_inserted"] >= 1 and (look[held] == rows.want[held]).all()
    assert 0 < st0["shared_pinned_bytes"] and st1["shared_pinned_bytes"] == 0


# ----------------------------------------------------------------- 2. only misses travel, nothing echoes
def test_only_misses_travel_and_nothing_echoes(sv, dev, cores, signed):
    rows = signed.take(range(300))
    c = Shared(sv, dev, cores, 4096, STORES)
    c.launch(0, rows)
    first = c.counters(0)
    assert first["shared_out"] == 300 and first["dropped"] > 0  # (4096 entries: some of 300 rows lose a claim)
    hit = c.launch(0, rows)
    second = c.counters(0)
    misses = 300 - int(hit.sum())
    assert misses == first["dropped"] and second["shared_out"] - first["shared_out"] == misses
    hit1 = c.launch(1, rows)  # slot 1 has drained both exports ahead of its probe
    st1 = c.counters(1)
    assert st1["shared_in"] == 300 + misses and int(hit1.sum()) == st1["fed_inserted"]
    mine = 300 - int(hit1.sum())
    assert st1["shared_out"] == mine
    c.sync(0)
    c.same(0, rows.keys)
    st0 = c.counters(0)
    assert st0["shared_in"] == mine == st0["fed_rows"]
    assert st0["fed_present"] + st0["fed_inserted"] + st0["fed_dropped"] == mine
    # a warm pass changes no shared_* counter, on either slot
    for _ in range(4):
        if c.launch(0, rows).all():
            break
    before = [c.counters(b) for b in (0, 1)]
    assert c.launch(0, rows).all()
    torch.cuda.synchronize(dev)
    c.sync(1)
    after = [c.counters(b) for b in (0, 1)]
    for b in (0, 1):
        assert all(after[b][f] == before[b][f] for f in sm.SHARED + ("shared_pinned_bytes", "fed_rows"))


# ----------------------------------------------------------------- 3. variable-length messages
def test_variable_length_messages_export_the_same_way(sv, dev, cores, oracle):
    rng = np.random.default_rng(91)
    pk, sig, msgs = [], [], []
    for i, ln in enumerate([0, 1, 111, 112, 300]):
        seed, m = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, ln, dtype=np.uint8))
        p, k, s = (ctypes.create_string_buffer(x) for x in (32, 64, 64))
        oracle.oracle_ed25519_seed_keypair(p, k, seed)
        oracle.oracle_ed25519_sign(s, m, ln, k)
        s = bytearray(s.raw)
        if i == 2:
            s[40] ^= 1  # one reject
        pk.append(np.frombuffer(p.raw, np.uint8))
        sig.append(np.frombuffer(bytes(s), np.uint8))
        msgs.append(m)
    pk, sig = np.array(pk), np.array(sig)
    rows = gv.Rows(pk, sig, msgs, gv._oracle(oracle, pk, sig, msgs))
    assert rows.want.tolist() == [1, 1, 0, 1, 1]
    c = Shared(sv, dev, cores, 4096, STORES)
    assert not c.launch(0, rows, fixed=False).any()
    c.sync(1)
    look = c.same(1, rows.keys)
    st = c.counters(1)
    assert c.counters(0)["shared_out"] == 5 and st["shared_in"] == 5
    held = look != sv.VC_MISS
    assert held.sum() == st["fed_inserted"] >= 4 and (look[held] == rows.want[held]).all()


# ----------------------------------------------------------------- 4. SHARE_FEED
@pytest.mark.parametrize("share", [FEED, 0])
def test_share_feed_sends_a_lane_batch_to_every_journal(sv, dev, cores, signed, share):
    rows = signed.take(range(400, 440))
    c = Shared(sv, dev, cores, 256, share, sources=LANE)
    c.lane(1, rows)
    c.sync(0)
    c.sync(1)
    look0, look1 = c.same(0, rows.keys), c.same(1, rows.keys)
    st0, st1 = c.counters(0), c.counters(1)
    assert st1["fed_rows"] == 40 and (look1 != sv.VC_MISS).sum() >= 35
    if share:
        assert st0["fed_rows"] == 40 and st0["shared_in"] == 40 and st1["shared_out"] == 40
        assert (look0 == look1).all()
    else:  # today's behaviour: the batch feeds its own slot
        assert (look0 == sv.VC_MISS).all() and all(st0[f] == 0 for f in fm.FED + sm.SHARED)
        assert st1["shared_out"] == 0
    assert st0["shared_pinned_bytes"] == 0 == st1["shared_pinned_bytes"]  # (no export: the rows went straight over)


# ----------------------------------------------------------------- 5. bounds
def test_bounds(sv, dev, cores, signed):
    a, b = signed.take(range(40)), signed.take(range(100, 140))
    c = Shared(sv, dev, cores, 4096, STORES, journal_rows=32)
    c.launch(0, a)
    st0 = c.counters(0)
    assert st0["shared_out"] == 32 and st0["shared_skipped"] == 8
    c.launch(0, b)  # slot 1 has not drained: its journal is full
    st0, st1 = c.counters(0), c.counters(1)
    assert st0["shared_out"] == 64 and st0["shared_skipped"] == 16
    assert st1["shared_in"] == 32 and st1["fed_overflow"] == 32
    assert 0 < st0["shared_pinned_bytes"] <= pinned_bound(32) == 4 * 4096
    c.sync(1)
    look = c.same(1, np.concatenate([a.keys, b.keys]))
    assert (look[32:] == sv.VC_MISS).all() and (look[:32] != sv.VC_MISS).sum() == c.counters(1)["fed_inserted"] >= 30


# ----------------------------------------------------------------- 6. what drops pending rows
@pytest.mark.parametrize("how", ["clear", "resize", "share", "feed"])
def test_what_drops_pending_rows(sv, dev, cores, signed, how):
    rows = signed.take(range(200, 260))
    c = Shared(sv, dev, cores, 1024, STORES)
    c.launch(0, rows)
    torch.cuda.synchronize(dev)
    if how == "clear":
        sv.verdict_cache_clear()
    elif how == "resize":
        sv.set_verdict_cache(1024)
    elif how == "share":
        sv.set_verdict_cache_share(0)
    else:
        sv.set_verdict_cache_feed(0)
    sv.verdict_cache_sync(1)
    assert (gf._lookup_both(sv, dev, rows.keys, device=1) == sv.VC_MISS).all()
    st1 = sv.verdict_cache_stats(1)
    assert st1["fed_rows"] == 0 and st1["shared_in"] == 0 and st1["fed_inserted"] == 0
    if how == "clear":  # ... and slot 0 forgot them too; nothing verified before the clear is anywhere
        assert (gf._lookup_both(sv, dev, rows.keys, device=0) == sv.VC_MISS).all()
    if how in ("clear", "feed"):  # sharing goes on afterwards
        c2 = signed.take(range(300, 320))
        gv._call(_OnSlot(sv, 0), dev, c2, fixed=True)
        sv.verdict_cache_sync(1)
        assert (gf._lookup_both(sv, dev, c2.keys, device=1) != sv.VC_MISS).sum() >= 18


# ----------------------------------------------------------------- 7. off is off
def test_off_is_off(sv, dev, cores, signed):
    rows, lane = signed.take(range(129)), signed.take(range(400, 440))
    seen = []
    for call_setter in (False, True):
        sv.set_verdict_cache(4096)
        sv.set_verdict_cache_feed(LANE)
        if call_setter:
            sv.set_verdict_cache_share(0)
        gv._call(_OnSlot(sv, 0), dev, rows, fixed=True)
        gf._keyed(sv, lane, 1)
        sv.verdict_cache_sync(0)
        sv.verdict_cache_sync(1)
        assert (gf._lookup_both(sv, dev, rows.keys, device=1) == sv.VC_MISS).all()
        assert (gf._lookup_both(sv, dev, lane.keys, device=0) == sv.VC_MISS).all()
        st = [sv.verdict_cache_stats(b) for b in (0, 1)]
        for s in st:
            assert all(s[f] == 0 for f in sm.SHARED + ("shared_pinned_bytes",))
        assert st[0]["fed_rows"] == 0 and st[1]["fed_rows"] == 40
        seen.append([s["bytes"] for s in st])
    assert seen[0] == seen[1]


# ----------------------------------------------------------------- 8. a sharded host call, re-sliced
def _multisig_builder(nb):
    """The bodies of test_gpu_vcache_feed.multisig_set, not finished yet: six 2-of-3 style accounts, every signer an
    ed25519 key, one signature in five corrupted."""
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
    return bld


def test_a_sharded_host_call_re_sliced(sv, dev, cores, oracle):
    nb, entries = 64, 4096
    bld = _multisig_builder(nb)
    signer = tp.device_signer(sv)
    first = bld.finish(signer, oracle)
    bld.bodies = bld.bodies[nb // 2:] + bld.bodies[:nb // 2]  # rotated by half: the slices trade slots
    second = bld.finish(signer, oracle)
    sets = [first, second]
    pairs = [gf.scenario_pairs(sv, s) for s in sets]
    n = len(pairs[0])
    assert n == len(pairs[1]) >= 128
    # the same pairs, each once, in another order
    k0 = sorted(k.tobytes() for k in pairs[0].keys)
    assert k0 == sorted(k.tobytes() for k in pairs[1].keys) and len(set(k0)) == n
    # no eviction at 4096 entries: no set of the table is named by more than its four ways
    assert np.bincount(pairs[0].keys[:, 0] % (entries // 4)).max() <= 4
    cpu = []
    for s in sets:
        a, kw = rp.explicit(s)
        cpu.append(sv.decide_txbodies_cpu(*a, protocol_version=21, want_checks=True, bad_cap=nb, **kw))
    assert len(set(cpu[0].body_code.tolist())) >= 2
    total = lambda f: sum(sv.verdict_cache_stats(b)[f] for b in (0, 1))  # noqa: E731
    hits = {}
    sv.set_min_shard(32)
    try:
        for share in (STORES, 0):
            sv.set_verdict_cache(entries)
            sv.set_verdict_cache_share(share)
            got = tr._decide_host(sv, first, form="explicit", bad_cap=nb, want_checks=True)
            tr._same(got, cpu[0])
            for b in (0, 1):
                assert sv.verdict_cache_stats(b)["lookups"] > 0, "slot %d got no slice" % b
                sv.verdict_cache_sync(b)
            assert total("lookups") == n and total("hits") == 0
            lost = sum(total(f) for f in ("dropped", "fed_dropped", "fed_overflow", "shared_skipped"))
            if share:
                assert total("shared_out") == n == total("shared_in")
            else:
                assert all(total(f) == 0 for f in sm.SHARED + ("shared_pinned_bytes", "fed_rows"))
            got = tr._decide_host(sv, second, form="explicit", bad_cap=nb, want_checks=True)
            tr._same(got, cpu[1])
            assert total("lookups") == 2 * n
            hits[share] = total("hits")
            print("share %d: %d pairs, second call %d hits, lost before it %d" % (share, n, hits[share], lost))
            if share:
                assert hits[share] >= n - lost
    finally:
        sv.set_min_shard(0)
    assert hits[STORES] > hits[0]


# ----------------------------------------------------------------- two threads, a slot each
def test_two_threads_launch_on_their_own_slots(sv, dev, signed):
    """20 cached device-form launches of 64 rows per thread, each thread on its own slot and stream, sharing on:
    verdicts are the oracle's, both syncs return and the counters' invariant holds on both slots."""
    sv.set_verdict_cache(1 << 16)
    sv.set_verdict_cache_share(STORES)
    errors, n, launches = [], 64, 20

    def work(slot):
        try:
            st = torch.cuda.Stream(dev)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
            for k in range(launches):
                # the two threads walk the same 9 windows of rows, shifted: each meets rows the other verified
                lo = 64 * ((k + 4 * slot) % 9)
                rows = signed.take(range(lo, lo + n))
                with torch.cuda.stream(st):
                    tpk, tsig = up(rows.pk), up(rows.sig)
                    tmsg = up(np.frombuffer(b"".join(rows.msgs) + bytes(16), np.uint8).copy())
                    tv = gv._guarded(dev, n)
                    st.synchronize()
                    sv.verify_device_cached(slot, tpk.data_ptr(), tsig.data_ptr(), tmsg.data_ptr(), n,
                                            tv.data_ptr() + gv.GUARD, fixed_msg_len=32, stream=st.cuda_stream)
                    st.synchronize()
                    got = gv._inner(tv, n)
                if not (got == rows.want).all():
                    errors.append("slot %d launch %d: verdicts" % (slot, k))
        except Exception as e:  # noqa: BLE001
            errors.append("slot %d: %r" % (slot, e))

    threads = [threading.Thread(target=work, args=(s,), daemon=True) for s in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(100)
        assert not t.is_alive(), "a launch did not return"
    assert not errors, errors
    # the syncs and the stats on a thread of their own too, so that one that does not return fails the test
    # instead of holding it: the whole test is bounded by the joins
    stats = []

    def tail():
        try:
            torch.cuda.synchronize(dev)
            for b in (0, 1):
                sv.verdict_cache_sync(b)
            stats.extend(sv.verdict_cache_stats(b) for b in (0, 1))
        except Exception as e:  # noqa: BLE001
            errors.append("syncs: %r" % (e,))

    t = threading.Thread(target=tail, daemon=True)
    t.start()
    t.join(60)
    assert not t.is_alive(), "a sync or a stats call did not return"
    assert not errors and len(stats) == 2, errors
    total_in = 0
    for b in (0, 1):
        st = stats[b]
        assert st["lookups"] == n * launches and st["hits"] + st["inserted"] + st["dropped"] == n * launches
        assert st["fed_rows"] == st["fed_present"] + st["fed_inserted"] + st["fed_dropped"]  # (drained: none held)
        assert st["shared_in"] == st["fed_rows"] and st["fed_overflow"] == 0
        assert st["shared_pinned_bytes"] <= pinned_bound(fm.DEFAULT_ROWS)
        total_in += st["shared_in"]
    out = [stats[b]["shared_out"] for b in (0, 1)]
    skipped = [stats[b]["shared_skipped"] for b in (0, 1)]
    # every miss was offered or counted as skipped, and what was offered reached the one other slot
    for b in (0, 1):
        assert out[b] + skipped[b] == stats[b]["inserted"] + stats[b]["dropped"]
    assert total_in == out[0] + out[1]
