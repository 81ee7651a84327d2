"""The verdict cache's feed for the tests: the native instantiation of
csrc/vjournal.h and of the insert pass of csrc/vcache.h
(tests/native/libvcachefeedcore.so) on top of vcache_model.NativeCache, and a
Python restatement that shares no code with it.

The feed, restated.  A journal is a list of at most `journal_rows` rows (key,
verdict byte).  Appending a batch goes through its rows in order: a row whose
verdict byte is neither 0 nor 1 is skipped and counts nowhere; any other row is
added while the journal has room (fed_rows) and counted as fed_overflow once it
is full.  A drain takes the whole list and leaves the journal empty.  Against
the table as the drain found it, a row whose key a holding slot of its set has
is present and does nothing more.  Every other row names a slot -- the first
slot of its set that holds nothing, going round from its start way, or the
start way if all four hold something.  Among the rows naming one slot the one
earliest in the journal is written there (fed_inserted); the others are
fed_dropped.  Nothing in this moves hits, inserted or dropped of the passes."""
import ctypes
import os
import subprocess

import numpy as np

import vcache_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
MISS = 0xFF
DEFAULT_ROWS = 65536
FED = ("fed_rows", "fed_overflow", "fed_present", "fed_inserted", "fed_dropped")


def load_feed_core():
    d = os.path.join(HERE, "native")
    # make every time, as vcache_model.load_core does
    subprocess.run(["make", "-s", "-f", "vcache_feed.mk", "libvcachefeedcore.so"], cwd=d, check=True)
    lib = ctypes.CDLL(os.path.join(d, "libvcachefeedcore.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.vfm_insert_pass.argtypes = [vp, vp, u64, vp, vp, u64, vp]
    lib.vfm_insert_pass.restype = None
    lib.vfm_journal_new.restype = vp
    lib.vfm_journal_free.argtypes = [vp]
    lib.vfm_journal_free.restype = None
    lib.vfm_journal_append.argtypes = [vp, vp, vp, u64, u64]
    lib.vfm_journal_append.restype = u64
    lib.vfm_journal_held.argtypes = [vp]
    lib.vfm_journal_held.restype = u64
    for f in (lib.vfm_journal_drop, lib.vfm_journal_reset):
        f.argtypes = [vp]
        f.restype = None
    lib.vfm_journal_counters.argtypes = [vp, vp]
    lib.vfm_journal_counters.restype = None
    lib.vfm_journal_drain.argtypes = [vp, vp, vp, u64, vp]
    lib.vfm_journal_drain.restype = u64
    return lib


def _rows(keys, verdicts):
    keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 8)
    verdicts = np.ascontiguousarray(verdicts, np.uint8).reshape(-1)
    assert len(keys) == len(verdicts)
    return keys, verdicts


class NativeFeed(vm.NativeCache):
    """csrc/vjournal.h and the insert pass of csrc/vcache.h on the host, over NativeCache's table.
    fed: present, inserted, dropped of the drains."""

    def __init__(self, core, fcore, entries, journal_rows=DEFAULT_ROWS):
        super().__init__(core, entries)
        self.fcore, self.journal_rows = fcore, journal_rows
        self.journal = fcore.vfm_journal_new()
        self.fed = np.zeros(3, np.uint64)

    def __del__(self):
        if getattr(self, "journal", None):
            self.fcore.vfm_journal_free(self.journal)
            self.journal = None

    def append(self, keys, verdicts):
        keys, verdicts = _rows(keys, verdicts)
        return int(self.fcore.vfm_journal_append(self.journal, keys.ctypes.data, verdicts.ctypes.data, len(keys),
                                                 self.journal_rows))

    def drain(self):
        return int(self.fcore.vfm_journal_drain(self.journal, self.tab.ctypes.data, self.claim.ctypes.data,
                                                self.entries // 4, self.fed.ctypes.data))

    def drop(self):
        self.fcore.vfm_journal_drop(self.journal)

    def clear(self):  # (sv_verdict_cache_clear: the table and the journaled rows; every counter stays)
        super().clear()
        if getattr(self, "journal", None):
            self.drop()

    def lookup(self, keys):
        keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 8)
        out = [self.core.vcm_lookup(self.tab.ctypes.data, self.entries // 4, keys[i].ctypes.data)
               for i in range(len(keys))]
        return np.array([MISS if v < 0 else v for v in out], np.uint8)

    def fed_counters(self):
        two = np.zeros(2, np.uint64)
        self.fcore.vfm_journal_counters(self.journal, two.ctypes.data)
        return dict(zip(FED, [int(x) for x in two.tolist() + self.fed.tolist()]))


class PyFeed(vm.PyCache):
    """The restatement (module docstring)."""

    def __init__(self, entries, journal_rows=DEFAULT_ROWS):
        super().__init__(entries)
        self.journal_rows, self.journal = journal_rows, []
        self.count = dict.fromkeys(FED, 0)

    def append(self, keys, verdicts):
        keys, verdicts = _rows(keys, verdicts)
        for k, v in zip(keys, verdicts):
            if int(v) > 1:
                continue
            if len(self.journal) < self.journal_rows:
                self.journal.append((tuple(int(w) for w in k), int(v)))
                self.count["fed_rows"] += 1
            else:
                self.count["fed_overflow"] += 1

    def _find(self, k):
        first = 4 * (k[0] % self.sets)
        for slot in range(first, first + 4):
            if self._holding(slot) and tuple(int(w) for w in self.tab[slot, :8]) == k:
                return slot
        return None

    def drain(self):
        rows, self.journal = self.journal, []
        named, winner = {}, {}
        for j, (k, v) in enumerate(rows):  # (the table is still as the drain found it)
            if self._find(k) is not None:
                self.count["fed_present"] += 1
                continue
            first, start = 4 * (k[0] % self.sets), k[1] % 4
            free = [w % 4 for w in range(start, start + 4) if not self._holding(first + w % 4)]
            named[j] = first + (free[0] if free else start)
            winner.setdefault(named[j], j)
        for j, slot in named.items():
            if winner[slot] == j:
                k, v = rows[j]
                self.tab[slot] = list(k) + [vm.HOLDS0 + v, 0, 0, 0]
                self.count["fed_inserted"] += 1
            else:
                self.count["fed_dropped"] += 1
        return len(rows)

    def lookup(self, keys):
        out = []
        for k in np.asarray(keys).reshape(-1, 8):
            slot = self._find(tuple(int(w) for w in k))
            out.append(MISS if slot is None else int(self.tab[slot, 8]) - vm.HOLDS0)
        return np.array(out, np.uint8)

    def fed_counters(self):
        return dict(self.count)
