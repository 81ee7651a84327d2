"""The verdict cache's model for the tests: the native instantiation of
csrc/vcache.h (tests/native/libvcachecore.so), a Python restatement of the
policy that shares no code with it, and the cache keys from hashlib.

The policy, restated.  A table of `entries` slots (a power of two >= 4), four
consecutive slots to a set.  A slot is twelve words: the key's eight, a state,
three zeros.  A slot holds a verdict iff its state is HOLDS0 or HOLDS1.  A key
(eight little-endian words of BLAKE2b-256(pk || sig || msg)) belongs to set
word0 mod sets and starts its search at way word1 mod 4.  A pass over a batch:
first every item is looked up in the table as the pass found it -- a hit is a
holding slot of its set with all eight words equal.  Then every missed item
whose verdict is 0 or 1 names a slot: the first slot of its set that holds
nothing, going round from its start way, or the start way if all four hold
something.  Among the items naming one slot the lowest index wins and is
written there; the others are dropped."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HOLDS0, HOLDS1 = 0x56430A50, 0x56430A51
ENTRY_BYTES = 48


def round_entries(entries):
    p = 4
    while p < entries:
        p *= 2
    return p


def holds(state):
    return (state == HOLDS0) | (state == HOLDS1)


def cache_key(pk, sig, msg):
    """Eight words of the reference's cache key, from hashlib."""
    d = hashlib.blake2b(bytes(pk) + bytes(sig) + bytes(msg), digest_size=32).digest()
    return np.frombuffer(d, "<u4")


def cache_keys(pk, sig, msgs):
    return np.array([cache_key(pk[i], sig[i], msgs[i]) for i in range(len(pk))], np.uint32).reshape(-1, 8)


def load_core():
    d = os.path.join(HERE, "native")
    # make every time, as conftest.py does: an edited header rebuilds the library instead of testing a stale one
    subprocess.run(["make", "-s", "-f", "vcache.mk", "libvcachecore.so"], cwd=d, check=True)
    lib = ctypes.CDLL(os.path.join(d, "libvcachecore.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.vcm_entry_bytes.restype = u64
    lib.vcm_lookup.argtypes = [vp, u64, vp]
    lib.vcm_candidate.argtypes = [vp, u64, vp]
    lib.vcm_candidate.restype = u64
    lib.vcm_pass.argtypes = [vp, vp, u64, vp, u64, vp, vp, vp, vp]
    lib.vcm_pass.restype = None
    assert lib.vcm_entry_bytes() == ENTRY_BYTES
    return lib


class NativeCache:
    """csrc/vcache.h on the host.  counters: hits, inserted, dropped."""

    def __init__(self, core, entries):
        self.core = core
        self.entries = round_entries(entries)
        self.clear()
        self.counters = np.zeros(3, np.uint64)

    def clear(self):
        self.tab = np.zeros((self.entries, 12), np.uint32)
        self.claim = np.full(self.entries, 0xFFFFFFFF, np.uint32)

    def run(self, keys, verify):
        keys = np.ascontiguousarray(keys, np.uint32).reshape(-1, 8)
        verify = np.ascontiguousarray(verify, np.uint8)
        n = len(keys)
        assert len(verify) == n
        hit, verdict = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.core.vcm_pass(self.tab.ctypes.data, self.claim.ctypes.data, self.entries // 4, keys.ctypes.data, n,
                           verify.ctypes.data, hit.ctypes.data, verdict.ctypes.data, self.counters.ctypes.data)
        return hit, verdict


class PyCache:
    """The restatement (module docstring)."""

    def __init__(self, entries):
        self.entries = round_entries(entries)
        self.sets = self.entries // 4
        self.tab = np.zeros((self.entries, 12), np.uint32)
        self.counters = [0, 0, 0]

    def _holding(self, slot):
        return int(self.tab[slot, 8]) in (HOLDS0, HOLDS1)

    def run(self, keys, verify):
        keys = [tuple(int(w) for w in k) for k in np.asarray(keys).reshape(-1, 8)]
        n = len(keys)
        hit, verdict = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        missed = []
        for i, k in enumerate(keys):
            first = 4 * (k[0] % self.sets)
            for slot in range(first, first + 4):
                if self._holding(slot) and tuple(int(w) for w in self.tab[slot, :8]) == k:
                    hit[i] = 1
                    verdict[i] = int(self.tab[slot, 8]) - HOLDS0
            if hit[i]:
                self.counters[0] += 1
            else:
                missed.append(i)
                verdict[i] = verify[i]
        winner = {}
        named = {}
        for i in missed:  # (the table is still as the pass found it)
            if verify[i] > 1:
                continue
            k = keys[i]
            first, start = 4 * (k[0] % self.sets), k[1] % 4
            free = [w % 4 for w in range(start, start + 4) if not self._holding(first + w % 4)]
            named[i] = first + (free[0] if free else start)
            winner[named[i]] = min(i, winner.get(named[i], i))
        for i in missed:
            if i in named and winner[named[i]] == i:
                self.tab[named[i]] = list(keys[i]) + [HOLDS0 + int(verify[i]), 0, 0, 0]
                self.counters[1] += 1
            else:
                self.counters[2] += 1
        return hit, verdict
