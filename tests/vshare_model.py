"""The sharing of verified verdicts between slots for the tests: the native
instantiation of csrc/vshare.h (tests/native/libvsharecore.so) over G of
vcache_feed_model.NativeFeed, and a Python restatement that shares no code with
it, over G of vcache_feed_model.PyFeed.

The sharing, restated.  Every slot has a table, a journal of `journal_rows`
rows and a queue of at most four pending exports.  A cached pass on slot A
drains A's journal, looks every item up, verifies the misses and inserts them
(vcache_model); then, if it had misses, it exports: with four exports already
pending every miss counts as shared_skipped and nothing else happens; else the
leading min(misses, journal_rows) miss rows (key, verdict byte), in item order,
become a pending export, they count as shared_out and the misses beyond them as
shared_skipped.  Hits are not exported and neither is anything a drain put into
the table.  Passing on takes A's pending exports in order, stopping at the first
that is not complete (a sync completes them all): its rows are appended to every
journal but A's by the journal's own rule (vcache_feed_model: rows with a byte
other than 0 or 1 skipped, the rest stored while there is room, else
fed_overflow), and what a journal stored counts as its slot's shared_in.  A lane
batch on slot A goes to A's journal and, with SHARE_FEED, to every other one
too: shared_in there by what was stored, shared_out on A by the batch's rows.
Dropping forgets the pending exports; the counters stay."""
import ctypes
import os
import subprocess

import numpy as np

import vcache_feed_model as fm

HERE = os.path.dirname(os.path.abspath(__file__))
PENDING = 4
SHARED = ("shared_out", "shared_in", "shared_skipped")


def load_share_core():
    d = os.path.join(HERE, "native")
    subprocess.run(["make", "-s", "-f", "vshare.mk", "libvsharecore.so"], cwd=d, check=True)
    lib = ctypes.CDLL(os.path.join(d, "libvsharecore.so"))
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    for f in (lib.vsm_pending_max, lib.vsm_offer, lib.vsm_pinned_bound, lib.vsm_pass, lib.vsm_pending):
        f.restype = u64
    lib.vsm_offer.argtypes = [u64, u64]
    lib.vsm_pinned_bound.argtypes = [u64]
    lib.vsm_new.restype = vp
    lib.vsm_free.argtypes = [vp]
    lib.vsm_free.restype = None
    lib.vsm_export.argtypes = [vp, vp, vp, u64, u64]
    lib.vsm_export.restype = ci
    lib.vsm_complete.argtypes = [vp, ci]
    lib.vsm_complete.restype = None
    lib.vsm_count_out.argtypes = [vp, u64]
    lib.vsm_count_out.restype = None
    lib.vsm_pass.argtypes = [vp, ci, vp, ci, ci, u64, vp]
    for f in (lib.vsm_drop, lib.vsm_reset):
        f.argtypes = [vp]
        f.restype = None
    lib.vsm_pending.argtypes = [vp]
    lib.vsm_counters.argtypes = [vp, vp]
    lib.vsm_counters.restype = None
    assert lib.vsm_pending_max() == PENDING
    return lib


def _misses(keys, want, hit):
    keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 8)
    m = np.flatnonzero(np.asarray(hit) == 0)
    return np.ascontiguousarray(keys[m]), np.ascontiguousarray(np.asarray(want, np.uint8)[m])


class NativeShare:
    """csrc/vshare.h on the host over g NativeFeed slots."""

    def __init__(self, cores, g, entries, journal_rows=fm.DEFAULT_ROWS, stores=True, feed=False):
        self.score, self.g, self.journal_rows = cores[2], g, journal_rows
        self.stores, self.feed = stores, feed
        self.slots = [fm.NativeFeed(cores[0], cores[1], entries, journal_rows) for _ in range(g)]
        self.exp = [self.score.vsm_new() for _ in range(g)]
        self.shared_in = np.zeros(g, np.uint64)
        self.journals = (ctypes.c_void_p * g)(*[s.journal for s in self.slots])

    def __del__(self):
        for e in getattr(self, "exp", []):
            self.score.vsm_free(e)
        self.exp = []

    def cached_pass(self, a, keys, want, complete=True):
        s = self.slots[a]
        s.drain()
        hit, _ = s.run(keys, want)
        mk, mv = _misses(keys, want, hit)
        if self.stores and self.g > 1 and len(mk):
            b = self.score.vsm_export(self.exp[a], mk.ctypes.data, mv.ctypes.data, len(mk), self.journal_rows)
            if b >= 0 and complete:
                self.score.vsm_complete(self.exp[a], b)
        return hit

    def lane(self, a, keys, verdicts):
        keys, verdicts = fm._rows(keys, verdicts)
        self.slots[a].append(keys, verdicts)
        if self.feed and self.g > 1:
            for j in range(self.g):
                if j != a:
                    self.shared_in[j] += self.slots[j].append(keys, verdicts)
            self.score.vsm_count_out(self.exp[a], len(keys))

    def pass_on(self, wait=False):
        for a in range(self.g):
            self.score.vsm_pass(self.exp[a], int(wait), self.journals, self.g, a, self.journal_rows,
                                self.shared_in.ctypes.data)

    def sync(self, b):
        self.pass_on(wait=True)
        return self.slots[b].drain()

    def drop(self):  # (what drops the journals drops the pending exports first)
        for e in self.exp:
            self.score.vsm_drop(e)
        for s in self.slots:
            s.drop()

    def clear(self):
        for e in self.exp:
            self.score.vsm_drop(e)
        for s in self.slots:
            s.clear()

    def shared_counters(self, a):
        two = np.zeros(2, np.uint64)
        self.score.vsm_counters(self.exp[a], two.ctypes.data)
        return {"shared_out": int(two[0]), "shared_in": int(self.shared_in[a]), "shared_skipped": int(two[1])}

    def held(self, a):
        return int(self.slots[a].fcore.vfm_journal_held(self.slots[a].journal))


class PyShare:
    """The restatement (module docstring) over g PyFeed slots."""

    def __init__(self, g, entries, journal_rows=fm.DEFAULT_ROWS, stores=True, feed=False):
        self.g, self.journal_rows, self.stores, self.feed = g, journal_rows, stores, feed
        self.slots = [fm.PyFeed(entries, journal_rows) for _ in range(g)]
        self.pending = [[] for _ in range(g)]  # [rows (keys, verdicts), complete]
        self.count = [dict.fromkeys(SHARED, 0) for _ in range(g)]

    def cached_pass(self, a, keys, want, complete=True):
        s = self.slots[a]
        s.drain()
        hit, _ = s.run(keys, want)
        mk, mv = _misses(keys, want, hit)
        if self.stores and self.g > 1 and len(mk):
            if len(self.pending[a]) == PENDING:
                self.count[a]["shared_skipped"] += len(mk)
            else:
                r = min(len(mk), self.journal_rows)
                self.pending[a].append([(mk[:r], mv[:r]), complete])
                self.count[a]["shared_out"] += r
                self.count[a]["shared_skipped"] += len(mk) - r
        return hit

    def _append_counted(self, j, keys, verdicts):
        before = self.slots[j].count["fed_rows"]
        self.slots[j].append(keys, verdicts)
        self.count[j]["shared_in"] += self.slots[j].count["fed_rows"] - before

    def lane(self, a, keys, verdicts):
        keys, verdicts = fm._rows(keys, verdicts)
        self.slots[a].append(keys, verdicts)
        if self.feed and self.g > 1:
            for j in range(self.g):
                if j != a:
                    self._append_counted(j, keys, verdicts)
            self.count[a]["shared_out"] += len(keys)

    def pass_on(self, wait=False):
        for a in range(self.g):
            while self.pending[a] and (wait or self.pending[a][0][1]):
                (keys, verdicts), _ = self.pending[a].pop(0)
                if keys is None:
                    continue  # (dropped)
                for j in range(self.g):
                    if j != a:
                        self._append_counted(j, keys, verdicts)

    def sync(self, b):
        self.pass_on(wait=True)
        return self.slots[b].drain()

    def _forget(self):
        for q in self.pending:
            for e in q:
                e[0] = (None, None)

    def drop(self):
        self._forget()
        for s in self.slots:
            s.journal = []

    def clear(self):
        self._forget()
        for s in self.slots:
            s.tab[:] = 0
            s.journal = []

    def shared_counters(self, a):
        return dict(self.count[a])

    def held(self, a):
        return len(self.slots[a].journal)
