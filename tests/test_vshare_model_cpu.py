"""The sharing of verified verdicts between slots on a host without a GPU:
csrc/vshare.h instantiated for the host (tests/native/vshare_core.cpp) over the
journals and tables of vcache_feed_model, against a restatement written out in
Python (vshare_model.PyShare) -- every table, every fed_* and shared_* counter,
exact equality -- and csrc/vshare.h under contention in a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import vcache_feed_model as fm
import vcache_model as vm
import vshare_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cores():
    return vm.load_core(), fm.load_feed_core(), sm.load_share_core()


def _keys(rng, n):
    return rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)


class Both:
    """The native model and the restatement side by side; every step runs through both, same() compares them."""

    def __init__(self, cores, g, entries, **kw):
        self.g = g
        self.native, self.py = sm.NativeShare(cores, g, entries, **kw), sm.PyShare(g, entries, **kw)

    def __getattr__(self, name):
        def both(*a, **kw):
            x, y = getattr(self.native, name)(*a, **kw), getattr(self.py, name)(*a, **kw)
            if x is not None:
                assert (np.asarray(x) == np.asarray(y)).all(), name
            self.same()
            return x
        return both

    def same(self):
        out = []
        for a in range(self.g):
            n, p = self.native.slots[a], self.py.slots[a]
            assert n.tab.tobytes() == p.tab.tobytes()
            assert n.counters.tolist() == p.counters
            fed = n.fed_counters()
            assert fed == p.fed_counters()
            sh = self.native.shared_counters(a)
            assert sh == self.py.shared_counters(a)
            held = self.native.held(a)
            assert held == self.py.held(a)
            # the counters' invariant, per slot, at every step
            assert fed["fed_rows"] == fed["fed_present"] + fed["fed_inserted"] + fed["fed_dropped"] + held
            assert sh["shared_in"] <= fed["fed_rows"]
            out.append({**fed, **sh})
        return out


def test_a_pass_on_one_slot_teaches_the_others_and_nothing_echoes(cores):
    rng = np.random.default_rng(31)
    keys = _keys(rng, 129)
    want = (keys[:, 2] & 1).astype(np.uint8)
    m = Both(cores, 3, 4096)
    hit = m.cached_pass(0, keys, want)
    assert not hit.any()
    c = m.same()
    assert c[0]["shared_out"] == 129 and c[0]["shared_in"] == 0 and c[1]["shared_in"] == 0  # (not passed on yet)
    assert m.sync(1) == 129
    c = m.same()
    assert c[1]["shared_in"] == 129 == c[2]["shared_in"] and c[1]["fed_rows"] == 129
    assert c[1]["fed_inserted"] + c[1]["fed_dropped"] == 129 and c[0]["fed_rows"] == 0
    # slot 1 over the same rows: what the drain stored hits, only its misses travel -- to 0 and 2, never back to 1
    hit1 = m.cached_pass(1, keys, want)
    assert int(hit1.sum()) == c[1]["fed_inserted"]
    misses1 = 129 - int(hit1.sum())
    m.sync(0)
    c = m.same()
    assert c[1]["shared_out"] == misses1 and c[0]["shared_in"] == misses1 and c[1]["shared_in"] == 129
    assert c[0]["fed_rows"] == misses1 and c[2]["fed_rows"] == 129 + misses1
    # a warm pass exports nothing: no counter moves anywhere
    for _ in range(3):
        m.cached_pass(0, keys, want)
    before = m.same()
    assert m.cached_pass(0, keys, want).all()
    m.pass_on(wait=True)
    assert m.same() == before
    # nothing echoes: slot 2 only ever drained -- it exported nothing
    m.sync(2)
    assert m.same()[2]["shared_out"] == 0


def test_truncation_at_the_journal_bound_and_a_full_queue(cores):
    rng = np.random.default_rng(32)
    keys = _keys(rng, 40)
    want = np.ones(40, np.uint8)
    m = Both(cores, 2, 4096, journal_rows=32)
    m.cached_pass(0, keys, want)
    c = m.same()
    assert c[0]["shared_out"] == 32 and c[0]["shared_skipped"] == 8
    assert m.sync(1) == 32
    look = m.native.slots[1].lookup(keys)
    assert (look[32:] == fm.MISS).all() and (look[:32] != fm.MISS).sum() == m.same()[1]["fed_inserted"]
    # five exports that nobody passes on: the fifth finds every buffer pending and is skipped whole
    m = Both(cores, 2, 4096, journal_rows=32)
    for b in range(5):
        m.cached_pass(0, _keys(rng, 10), np.ones(10, np.uint8), complete=False)
    c = m.same()
    assert c[0]["shared_out"] == 40 and c[0]["shared_skipped"] == 10
    m.pass_on()  # (none is complete: nothing moves)
    assert m.same()[1]["shared_in"] == 0
    m.sync(1)  # 40 rows for a journal of 32
    c = m.same()
    assert c[1]["shared_in"] == 32 and c[1]["fed_overflow"] == 8
    assert sm.load_share_core().vsm_pinned_bound(32) == 4 * 4096


def test_overflow_at_the_peer_and_share_feed(cores):
    rng = np.random.default_rng(33)
    a, b = _keys(rng, 40), _keys(rng, 40)
    ones = np.ones(40, np.uint8)
    m = Both(cores, 2, 4096, journal_rows=32)
    m.cached_pass(0, a, ones)
    m.cached_pass(0, b, ones)  # slot 1 has not drained: its journal is full after the first export
    m.pass_on()
    c = m.same()
    assert c[0]["shared_out"] == 64 and c[0]["shared_skipped"] == 16
    assert c[1]["shared_in"] == 32 and c[1]["fed_overflow"] == 32 and c[1]["fed_rows"] == 32
    # SHARE_FEED: a lane batch goes to every journal; without it to its own
    for feed in (True, False):
        m = Both(cores, 3, 256, stores=False, feed=feed)
        v = (a[:, 3] & 1).astype(np.uint8)
        m.lane(1, a, v)
        for s in range(3):
            m.sync(s)
        c = m.same()
        assert c[1]["fed_rows"] == 40 and c[1]["shared_out"] == (40 if feed else 0) and c[1]["shared_in"] == 0
        for s in (0, 2):
            assert c[s]["fed_rows"] == c[s]["shared_in"] == (40 if feed else 0)
            look = m.native.slots[s].lookup(a)
            assert ((look != fm.MISS).sum() == c[s]["fed_inserted"]) and ((look != fm.MISS).any() == feed)
        # a rejected byte other than 0 or 1 travels as it is and is skipped by the journal alone
        m.cached_pass(0, b[:4], np.array([1, 2, 0, 7], np.uint8))
    m = Both(cores, 2, 256)
    m.cached_pass(0, b[:4], np.array([1, 2, 0, 7], np.uint8))
    m.sync(1)
    c = m.same()
    assert c[0]["shared_out"] == 4 and c[1]["shared_in"] == 2 and c[1]["fed_rows"] == 2


def test_drop_and_clear_forget_the_pending_exports(cores):
    rng = np.random.default_rng(34)
    keys = _keys(rng, 20)
    ones = np.ones(20, np.uint8)
    for how in ("drop", "clear"):
        m = Both(cores, 2, 256)
        m.cached_pass(0, keys, ones, complete=False)
        getattr(m, how)()
        assert m.sync(1) == 0
        assert (m.native.slots[1].lookup(keys) == fm.MISS).all()
        c = m.same()
        assert c[0]["shared_out"] == 20 and c[1]["shared_in"] == 0  # (the counters stay)
        # the buffers came back: four more exports fit
        for b in range(4):
            m.cached_pass(0, _keys(rng, 5), np.ones(5, np.uint8), complete=False)
        assert m.same()[0]["shared_skipped"] == 0


def test_one_slot_shares_nothing(cores):
    rng = np.random.default_rng(35)
    keys = _keys(rng, 30)
    m = Both(cores, 1, 256, feed=True)
    m.cached_pass(0, keys, np.ones(30, np.uint8))
    m.lane(0, keys, np.ones(30, np.uint8))
    m.sync(0)
    c = m.same()
    assert all(c[0][f] == 0 for f in sm.SHARED) and c[0]["fed_rows"] == 30


def test_share_queue_under_contention(tmp_path):
    """tests/native/vshare_stress.cpp, a stand-alone host program: four exporters pass rows on to three journals
    while three drainers take(); per exporter every journal receives rows in export order and the counts add up."""
    exe = tmp_path / "vshare_stress"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-o", str(exe), os.path.join(HERE, "native", "vshare_stress.cpp"),
                    "-lpthread"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and ": ok" in r.stdout, r.stdout[-3000:]
