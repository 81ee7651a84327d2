"""The verdict cache's policy (csrc/vcache.h) on a host without a GPU: the
header instantiated for the host (tests/native/vcache_core.cpp) against a
restatement of the policy written out here from its description alone, step by
step over random batches; the fail-closed rules of a lookup; the retention
condition; and the four C-ABI functions' declarations and binding.  Every
expectation but the retention bound is exact equality."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import vcache_model as vm

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def core():
    return vm.load_core()


def _keys(rng, n):
    return rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("entries", [4, 8, 64, 4096])
def test_native_model_equals_the_restatement_step_by_step(core, entries):
    rng = np.random.default_rng(1000 + entries)
    native, py = vm.NativeCache(core, entries), vm.PyCache(entries)
    pool = _keys(rng, 3 * entries + 50)  # keys come back in later batches, some after their eviction
    sizes = [1, 3, entries // 2 + 1, entries, entries + 7, 3 * entries, 2, entries]
    seen_hit = seen_drop = seen_evict = False
    for step, n in enumerate(sizes):
        idx = rng.integers(0, len(pool), n)
        if n >= 3:
            idx[n // 2] = idx[0]  # a key repeated inside the batch
        keys = pool[idx]
        verify = (keys[:, 2] & 1).astype(np.uint8)  # a key's verdict is a function of the key
        held_before, inserted_before = int(vm.holds(py.tab[:, 8]).sum()), py.counters[1]
        h1, v1 = native.run(keys, verify)
        h2, v2 = py.run(keys, verify)
        assert (h1 == h2).all() and (v1 == v2).all() and (v1 == verify).all(), step
        assert native.tab.tobytes() == py.tab.tobytes(), step
        assert native.counters.tolist() == py.counters, step
        assert (native.claim == 0xFFFFFFFF).all()
        seen_hit |= bool(h1.any())
        seen_drop |= py.counters[2] > 0
        # (an insert that did not add a holding slot overwrote one)
        seen_evict |= held_before + py.counters[1] - inserted_before > int(vm.holds(py.tab[:, 8]).sum())
    assert seen_hit and seen_drop and seen_evict
    # a repeated key never sits in two slots
    held = py.tab[vm.holds(py.tab[:, 8])]
    assert len({r[:8].tobytes() for r in held}) == len(held)


def test_probe_precedes_every_insert(core):
    # the same key twice in one batch: both miss, one is stored, the other dropped; then both hit
    c = vm.NativeCache(core, 64)
    k = _keys(np.random.default_rng(3), 1)
    keys = np.concatenate([k, k])
    hit, _ = c.run(keys, np.array([1, 1], np.uint8))
    assert hit.tolist() == [0, 0] and c.counters.tolist() == [0, 1, 1]
    hit, v = c.run(keys, np.array([0, 0], np.uint8))  # (the cached verdict, not this pass's)
    assert hit.tolist() == [1, 1] and v.tolist() == [1, 1] and c.counters.tolist() == [2, 1, 1]


def test_only_verdict_bytes_0_and_1_are_stored(core):
    c = vm.NativeCache(core, 4)
    keys = _keys(np.random.default_rng(4), 3)
    c.run(keys, np.array([2, 255, 0], np.uint8))
    assert c.counters.tolist() == [0, 1, 2]
    assert [core.vcm_lookup(c.tab.ctypes.data, 1, keys[i].ctypes.data) for i in range(3)] == [-1, -1, 0]


def test_lookup_fails_closed(core):
    rng = np.random.default_rng(5)
    for entries in (4, 64):
        c = vm.NativeCache(core, entries)
        keys = _keys(rng, 2)
        c.run(keys[:1], np.array([1], np.uint8))
        c.run(keys[1:], np.array([0], np.uint8))  # (a pass of its own: in one pass the two might name one slot)
        k = keys[0].copy()
        look = lambda key: core.vcm_lookup(c.tab.ctypes.data, entries // 4, np.ascontiguousarray(key).ctypes.data)
        assert look(k) == 1 and look(keys[1]) == 0
        # a key differing in any single one of its 256 bits is a miss
        for bit in range(256):
            q = k.copy()
            q[bit // 32] ^= np.uint32(1 << (bit % 32))
            assert look(q) == -1, bit
        # any state other than the two valid ones is a miss: neighbours, single-bit damage, zero, all ones
        slot = int(np.flatnonzero((c.tab[:, :8] == k).all(axis=1))[0])
        good = int(c.tab[slot, 8])
        assert good == vm.HOLDS1
        others = {0, 1, 2, 0xFFFFFFFF, vm.HOLDS0 - 1, vm.HOLDS1 + 1, vm.HOLDS0 >> 1}
        others |= {good ^ (1 << b) for b in range(1, 32)}  # (bit 0 turns it into the other valid state)
        others |= {int(x) for x in rng.integers(0, 1 << 32, 200)}
        for st in others - {vm.HOLDS0, vm.HOLDS1}:
            c.tab[slot, 8] = st
            assert look(k) == -1, hex(st)
        c.tab[slot, 8] = vm.HOLDS0
        assert look(k) == 0
    # an entry that holds nothing may be taken by an insert: all-zero memory is an empty table
    assert vm.NativeCache(core, 4).tab.tobytes() == bytes(4 * 48)


@pytest.mark.parametrize("n", [1000, 4096])
def test_retention_condition(core, n):
    """A batch of n distinct random keys inserted once into an empty cache of 8 x its size: at least 0.90 of the
    batch is found again (the suggested policy gave 0.936-0.947 over six seeds and sizes)."""
    for seed in (11, 12):
        c = vm.NativeCache(core, 8 * n)  # (rounded up to a power of two, as the engine rounds it)
        keys = _keys(np.random.default_rng(seed), n)
        assert len({k.tobytes() for k in keys}) == n
        hit, _ = c.run(keys, np.ones(n, np.uint8))
        assert not hit.any()
        hit, _ = c.run(keys, np.ones(n, np.uint8))
        kept = float(hit.mean())
        print("retention n=%d seed=%d entries=%d: %.4f" % (n, seed, c.entries, kept))
        assert kept >= 0.90


def test_native_model_builds_clean_under_sanitizers(tmp_path):
    """vcache.h in a stand-alone host program under ASan + UBSan: passes over exact-size heap arrays at one set."""
    src = tmp_path / "main.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "%s"
extern "C" void vcm_pass(void*, uint32_t*, uint64_t, const uint32_t*, uint64_t, const uint8_t*, uint8_t*, uint8_t*, uint64_t*);
int main() {
  for (uint64_t sets : {1ull, 2ull, 16ull}) {
    const uint64_t e = 4 * sets, n = 5 * e + 3;
    void* tab = std::calloc(e, sizeof(sv_vc_entry));
    uint32_t* claim = (uint32_t*)std::malloc(4 * e);
    std::memset(claim, 0xFF, 4 * e);
    uint32_t* keys = (uint32_t*)std::malloc(32 * n);
    uint8_t *ver = (uint8_t*)std::malloc(n), *hit = (uint8_t*)std::malloc(n), *out = (uint8_t*)std::malloc(n);
    uint64_t x = 88172645463325252ull, cnt[3] = {0, 0, 0};
    for (int pass = 0; pass < 4; ++pass) {
      for (uint64_t i = 0; i < 8 * n; ++i) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; keys[i] = (uint32_t)(x >> 20) %% 97; }
      for (uint64_t i = 0; i < n; ++i) ver[i] = (uint8_t)(keys[8 * i + 2] & 1);
      vcm_pass(tab, claim, sets, keys, n, ver, hit, out, cnt);
      if (std::memcmp(ver, out, n)) { std::printf("verdict mismatch\n"); return 1; }
    }
    if (cnt[0] + cnt[1] + cnt[2] != 4 * n) { std::printf("counters\n"); return 1; }
    std::free(tab); std::free(claim); std::free(keys); std::free(ver); std::free(hit); std::free(out);
  }
  std::printf("vcache_core ok\n");
  return 0;
}
''' % os.path.join(REPO, "stellar-core_amd", "csrc", "vcache.h"))
    exe = tmp_path / "vcache_core"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(src),
                    os.path.join(HERE, "native", "vcache_core.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "vcache_core ok" in r.stdout, r.stdout[-2000:]


def test_header_declares_the_four_functions(sv):
    with open(os.path.join(REPO, "include", "stellar_sigverify.h")) as f:
        text = f.read()
    lib = ctypes.CDLL(sv.LIB_PATH)
    for name in ("sv_set_verdict_cache", "sv_verdict_cache_clear", "sv_verdict_cache_get_stats",
                 "sv_ed25519_verify_device_cached"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in sv.EXPORTED_SYMBOLS
        getattr(lib, name)
    m = re.search(r"typedef struct sv_verdict_cache_stats \{(.*?)\} sv_verdict_cache_stats;", text, re.S)
    fields = re.findall(r"^\s*(?:uint64_t|double) (\w+);", m.group(1), re.M)
    assert fields[:7] == ["struct_size", "entries", "lookups", "hits", "inserted", "dropped", "bytes"]
    assert fields == [f for f, _ in sv.VerdictCacheStats._fields_]


def test_binding_validates_and_needs_a_gpu_only_to_verify(sv):
    with pytest.raises(ValueError):
        sv.set_verdict_cache(-1)
    with pytest.raises(ValueError):
        sv.set_verdict_cache((1 << 24) + 1)
    with pytest.raises(ValueError):
        sv.verify_device_cached(0, 0x1000, 0x2000, 0x3000, -1, 0x4000)
    with pytest.raises(ValueError):
        sv.verify_device_cached(0, 0, 0x2000, 0x3000, 4, 0x4000)  # null pk
    with pytest.raises(ValueError):
        sv.verify_device_cached(0, 0x1000, 0x2000, 0x3000, 4, 0x4000, fixed_msg_len=0)  # no offsets / lengths
    with pytest.raises(ValueError):
        sv.verify_device_cached(0, 0x1008, 0x2000, 0x3000, 4, 0x4000)  # pk not 16-byte aligned
    with pytest.raises(ValueError):
        sv.verify_device_cached(0, 0x1000, 0x2000, 0x3000, 4, 0x4000, d_keys=0x5004)
    # the C-ABI refuses a capacity above its maximum itself
    lib = sv.load_library()
    assert lib.sv_set_verdict_cache((1 << 24) + 1) == -1
    # the setter and the clear need no device
    try:
        sv.set_verdict_cache(4096)
        sv.verdict_cache_clear()
    finally:
        sv.set_verdict_cache(0)


def test_cached_verify_raises_without_gpu(sv):
    """On a host without a GPU the cached call raises (never rejects), as every verify entry point does."""
    try:
        n = sv.device_count()
    except sv.SigVerifyError:
        n = 0
    if n > 0:
        pytest.skip("a GPU is present")
    try:
        sv.set_verdict_cache(4096)
        with pytest.raises(sv.SigVerifyError):
            sv.verify_device_cached(0, 0x1000, 0x2000, 0x3000, 4, 0x4000)
        with pytest.raises(sv.SigVerifyError):
            sv.verdict_cache_stats(0)
    finally:
        sv.set_verdict_cache(0)
