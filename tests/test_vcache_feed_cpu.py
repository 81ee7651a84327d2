"""The verdict cache's feed on a host without a GPU: csrc/vjournal.h and the
insert pass of csrc/vcache.h instantiated for the host
(tests/native/vcache_feed_core.cpp) against a restatement written out from the
description alone (vcache_feed_model.PyFeed) -- table contents and the five
fed_* counters, exact equality; the journal under contention in a stand-alone
ThreadSanitizer build; and the new C-ABI calls' validation."""
import os
import subprocess

import numpy as np
import pytest

import vcache_feed_model as fm
import vcache_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def cores():
    return vm.load_core(), fm.load_feed_core()


def _keys(rng, n):
    return rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)


class Pair:
    """The native model and the restatement side by side; same() compares everything they hold."""

    def __init__(self, cores, entries, journal_rows=fm.DEFAULT_ROWS):
        self.native = fm.NativeFeed(cores[0], cores[1], entries, journal_rows)
        self.py = fm.PyFeed(entries, journal_rows)

    def append(self, keys, verdicts):
        self.native.append(keys, verdicts)
        self.py.append(keys, verdicts)

    def drain(self):
        a, b = self.native.drain(), self.py.drain()
        assert a == b
        self.same()
        return a

    def same(self):
        assert self.native.tab.tobytes() == self.py.tab.tobytes()
        assert self.native.fed_counters() == self.py.fed_counters()
        assert (self.native.claim == 0xFFFFFFFF).all()
        # the passes' own counters never move in a drain
        assert self.native.counters.tolist() == [0, 0, 0] and self.py.counters == [0, 0, 0]
        return self.native.fed_counters()


def test_one_set_nine_rows_with_duplicates_and_rejects(cores):
    rng = np.random.default_rng(21)
    keys = _keys(rng, 9)
    keys[4] = keys[1]  # two duplicate keys: each row loses to (or, drained later, finds) its first copy
    keys[7] = keys[2]
    verdicts = np.ones(9, np.uint8)
    verdicts[[0, 3, 6]] = 0  # three rejects: cached like accepts
    p = Pair(cores, 4)
    p.append(keys, verdicts)
    assert p.drain() == 9
    c = p.same()
    assert c["fed_rows"] == 9 and c["fed_overflow"] == 0 and c["fed_present"] == 0
    assert c["fed_inserted"] + c["fed_dropped"] == 9
    assert 1 <= c["fed_inserted"] <= 4 and c["fed_dropped"] >= 2 + (7 - 4)  # the duplicates, and 7 keys for 4 slots
    look = p.native.lookup(keys)
    assert (look == p.py.lookup(keys)).all()
    held = look != fm.MISS
    assert held.sum() >= c["fed_inserted"] and (look[held] == verdicts[held]).all()
    assert (look[4] == look[1]) and (look[7] == look[2])  # a key is one entry, whichever row carried it
    # a stored reject is a held 0, never a miss
    if held[[0, 3, 6]].any():
        assert (look[[0, 3, 6]][held[[0, 3, 6]]] == 0).all()


def test_four_sets_65_rows(cores):
    rng = np.random.default_rng(22)
    keys = _keys(rng, 65)
    verdicts = (keys[:, 2] & 1).astype(np.uint8)
    p = Pair(cores, 16)
    p.append(keys[:30], verdicts[:30])  # two batches, one drain: journal order is append order
    p.append(keys[30:], verdicts[30:])
    assert p.drain() == 65
    c = p.same()
    assert c["fed_rows"] == 65 and c["fed_inserted"] + c["fed_dropped"] == 65 and c["fed_inserted"] <= 16
    assert (p.native.lookup(keys) == p.py.lookup(keys)).all()
    # a second drain of other rows against the now full table: every row names its start way (an eviction)
    more = _keys(rng, 20)
    p.append(more, np.ones(20, np.uint8))
    p.drain()
    assert (p.native.lookup(np.concatenate([keys, more])) == p.py.lookup(np.concatenate([keys, more]))).all()


@pytest.mark.parametrize("entries", [4, 16, 256])
def test_the_same_rows_twice_are_present_and_change_nothing(cores, entries):
    rng = np.random.default_rng(23 + entries)
    keys = _keys(rng, 65)
    verdicts = (keys[:, 3] & 1).astype(np.uint8)
    p = Pair(cores, entries)
    p.append(keys, verdicts)
    p.drain()
    first = p.same()
    look = p.native.lookup(keys)
    stored = int((look != fm.MISS).sum())
    assert stored == first["fed_inserted"]  # (distinct random keys: every stored row is found again)
    p.append(keys, verdicts)
    p.drain()
    second = p.same()
    assert second["fed_present"] == stored
    # (the rows the table did not hold compete again, so where rows were dropped the table may change: the two
    # models agree on how -- same() above.  Where every row is stored nothing changes at all:)
    q = Pair(cores, 1024)
    few = keys[:8]
    for _ in range(3):  # (until no row loses its claim)
        q.append(few, verdicts[:8])
        q.drain()
    tab = q.native.tab.copy()
    before = q.same()
    q.append(few, verdicts[:8])
    q.drain()
    after = q.same()
    assert q.native.tab.tobytes() == tab.tobytes()
    assert after["fed_present"] - before["fed_present"] == 8 and after["fed_inserted"] == before["fed_inserted"]


def test_overflow_keeps_the_first_rows_in_append_order(cores):
    rng = np.random.default_rng(24)
    keys = _keys(rng, 60)
    verdicts = np.ones(60, np.uint8)
    p = Pair(cores, 4096, journal_rows=32)
    for b in range(3):
        p.append(keys[20 * b:20 * b + 20], verdicts[20 * b:20 * b + 20])
    c = p.same()
    assert c["fed_rows"] == 32 and c["fed_overflow"] == 28  # the third batch contributes no row
    assert p.drain() == 32
    c = p.same()
    assert c["fed_inserted"] + c["fed_dropped"] == 32
    look = p.native.lookup(keys)
    assert (look[32:] == fm.MISS).all() and (look[:32] != fm.MISS).sum() == c["fed_inserted"]
    # the journal is empty again: the next batch fits
    p.append(keys[40:], verdicts[40:])
    assert p.same()["fed_rows"] == 52 and p.drain() == 20


def test_rows_with_verdict_byte_2_are_skipped(cores):
    rng = np.random.default_rng(25)
    keys = _keys(rng, 12)
    verdicts = np.array([1, 2, 0, 2, 255, 1, 1, 2, 0, 1, 2, 1], np.uint8)
    p = Pair(cores, 4096, journal_rows=6)
    p.append(keys, verdicts)
    c = p.same()
    # 7 verdict bytes: the first 6 fit, the seventh overflows; the others count nowhere
    assert c["fed_rows"] == 6 and c["fed_overflow"] == 1
    assert p.drain() == 6
    look = p.native.lookup(keys)
    assert (look[verdicts > 1] == fm.MISS).all() and look[11] == fm.MISS
    kept = np.flatnonzero(verdicts <= 1)[:6]
    assert (look[kept][look[kept] != fm.MISS] == verdicts[kept][look[kept] != fm.MISS]).all()
    # the insert pass itself never stores such a byte either
    n = fm.NativeFeed(cores[0], cores[1], 64)
    cnt = np.zeros(3, np.uint64)
    v = np.array([2, 1], np.uint8)
    cores[1].vfm_insert_pass(n.tab.ctypes.data, n.claim.ctypes.data, 16, keys[:2].ctypes.data, v.ctypes.data, 2,
                             cnt.ctypes.data)
    assert cnt.tolist() == [0, 1, 0] and n.lookup(keys[:2]).tolist() == [fm.MISS, 1]


def test_drop_and_clear_forget_the_journaled_rows(cores):
    rng = np.random.default_rng(26)
    keys = _keys(rng, 10)
    n = fm.NativeFeed(cores[0], cores[1], 64)
    n.append(keys, np.ones(10, np.uint8))
    n.drop()
    assert n.drain() == 0 and (n.lookup(keys) == fm.MISS).all()
    assert n.fed_counters()["fed_rows"] == 10  # (the counters stay)
    n.append(keys, np.ones(10, np.uint8))
    n.clear()
    assert n.drain() == 0 and (n.lookup(keys) == fm.MISS).all()


def test_journal_under_contention_with_thread_sanitizer(tmp_path):
    """tests/native/vjournal_stress.cpp, a stand-alone host program: four appenders against one thread looping on
    take(); every offered row is taken exactly once or counted as overflow."""
    exe = tmp_path / "vjournal_stress"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-o", str(exe),
                    os.path.join(HERE, "native", "vjournal_stress.cpp"), "-lpthread"], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and ": ok" in r.stdout and "ThreadSanitizer" not in r.stdout, r.stdout[-3000:]


def _gpus(sv):
    try:
        return sv.device_count()
    except sv.SigVerifyError:
        return 0


def test_feed_setter_validates_and_needs_no_gpu(sv):
    lib = sv.load_library()
    assert sv.VC_FEED_LANE == 1 and sv.VC_FEED_BULK == 2 and sv.VC_MISS == 0xFF
    try:
        assert lib.sv_set_verdict_cache_feed(4, 0) == -1  # SV_ERR_INVALID_ARG: an unknown bit
        assert lib.sv_set_verdict_cache_feed(0x80000001, 0) == -1
        assert lib.sv_set_verdict_cache_feed(1, (1 << 24) + 1) == -1
        with pytest.raises(sv.SigVerifyError):
            sv.set_verdict_cache_feed(8)
        with pytest.raises(ValueError):
            sv.set_verdict_cache_feed(-1)
        with pytest.raises(ValueError):
            sv.set_verdict_cache_feed(1, -5)
        # every valid setting is remembered with the cache off and on, without a device
        for sources in (0, 1, 2, 3):
            sv.set_verdict_cache_feed(sources)
            sv.set_verdict_cache_feed(sources, 32)
        sv.set_verdict_cache(64)
        sv.set_verdict_cache_feed(sv.VC_FEED_LANE | sv.VC_FEED_BULK, 1 << 24)
        sv.verdict_cache_clear()
    finally:
        sv.set_verdict_cache_feed(0)
        sv.set_verdict_cache(0)
    with pytest.raises(ValueError):
        sv.verdict_cache_lookup(np.zeros(33, np.uint8))
    with pytest.raises(ValueError):
        sv.verdict_cache_lookup_device(0, 0x1008, 4, 0x2000)  # keys not 16-byte aligned
    with pytest.raises(ValueError):
        sv.verdict_cache_lookup_device(0, 0, 4, 0x2000)
    with pytest.raises(ValueError):
        sv.verdict_cache_lookup_device(0, 0x1000, -1, 0x2000)
    # n == 0 needs no device, as the other host forms' empty batches do not
    assert sv.verdict_cache_lookup(np.zeros((0, 32), np.uint8)).shape == (0,)
    # the C-ABI refuses null buffers itself
    assert lib.sv_verdict_cache_lookup(0, None, 3, None) == -1


def test_lookup_and_sync_with_the_cache_off(sv):
    """With the cache off a lookup answers SV_VC_MISS for every key and a sync does nothing -- on a slot, so on a
    host without a GPU both return SV_ERR_NO_DEVICE, as every host form does there."""
    keys = _keys(np.random.default_rng(27), 5)
    sv.set_verdict_cache(0)
    if _gpus(sv) > 0:
        assert (sv.verdict_cache_lookup(keys) == sv.VC_MISS).all()
        sv.verdict_cache_sync(0)
        return
    for call in (lambda: sv.verdict_cache_lookup(keys), lambda: sv.verdict_cache_sync(0),
                 lambda: sv.verdict_cache_lookup_device(0, 0x1000, 4, 0x2000)):
        with pytest.raises(sv.SigVerifyError) as e:
            call()
        assert "SV_ERR_NO_DEVICE" in str(e.value)
    assert [f for f, _ in sv.VerdictCacheStats._fields_[-5:]] == list(fm.FED)
