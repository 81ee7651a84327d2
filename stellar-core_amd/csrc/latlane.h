// Latency lane of a device slot: its creation and release, the key cache of
// the warm-key kernel (planning, table builds), the launch and completion of
// one latency-bound host batch, and the cold launch shared with the device
// API.  Included by sv_api.cpp.
#pragma once

#include <array>
#include <chrono>
#include <cstdio>

#include "engine_state.h"
#include "host_image.h"

namespace sv {
namespace {

// ------------------------------------------------------------ latency lane
inline std::atomic<size_t> g_key_cap{~(size_t)0};  // sv_set_key_cache (~0: SV_KEY_CACHE or the default)
inline size_t key_cache_cap() {
  const size_t v = g_key_cap.load();
  return v != ~(size_t)0 ? v : env_size("SV_KEY_CACHE", 1024);
}
// keys admitted for a table build per batch (a flood of fresh keys costs at
// most this many ~0.3 ms builds on the low-priority stream per batch)
constexpr size_t kMaxBuildsPerBatch = 256;

inline void lat_drop_builds(LatLane& L) {
  for (auto& b : L.inflight) {
    (void)hipEventDestroy(b.uploaded);
    (void)hipEventDestroy(b.done);
  }
  L.inflight.clear();
}

// Caller holds L.mu and has set the device.
// A context's quad workspace of at least `bytes`; growing it frees the old
// one, so the work queued on the context (a device-API batch) drains first.
inline int lat_ws(LatCtx& c, size_t bytes) {
  if (bytes > c.ws.cap) SV_HIP(hipStreamSynchronize(c.stream));  // (never free under a running kernel)
  return c.ws.ensure(bytes);
}

// Every batch queued on the lane's verify streams has completed.
inline void lat_sync(LatLane& L) {
  for (int k = 0; k < L.nctx; ++k) {
    if (L.ctx[k].stream) (void)hipStreamSynchronize(L.ctx[k].stream);
    if (L.ctx[k].hstream) (void)hipStreamSynchronize(L.ctx[k].hstream);
  }
}

// (no batch holds a context: the API's teardown guard has drained the calls)
inline void release_lat(LatLane& L) {
  if (!L.ready) return;
  lat_sync(L);
  (void)hipStreamSynchronize(L.build);
  lat_drop_builds(L);
  L.timer.release();
  for (LatCtx& c : L.ctx) {
    c.h_in.release(); c.h_out.release(); c.z_out.release(); c.z_keys.release(); c.z_stat.release();
    c.d_in.release(); c.d_out.release(); c.d_keys.release(); c.ws.release();
    if (c.done) (void)hipEventDestroy(c.done);
    if (c.keys_down) (void)hipEventDestroy(c.keys_down);
    if (c.ev) (void)hipEventDestroy(c.ev);
    if (c.dev_done) (void)hipEventDestroy(c.dev_done);
    if (c.stream) (void)hipStreamDestroy(c.stream);
    if (c.hstream) (void)hipStreamDestroy(c.hstream);
    c.done = c.keys_down = c.ev = c.dev_done = nullptr;
    c.stream = c.hstream = nullptr;
    c.busy = false;
  }
  L.h_build.release();
  L.d_build.release();
  L.ktab.release(); L.kstat.release();
  if (L.ctab) (void)hipFree(L.ctab);
  L.ctab = nullptr;
  if (L.ev_lat) (void)hipEventDestroy(L.ev_lat);
  L.ev_lat = nullptr;
  if (L.build) (void)hipStreamDestroy(L.build);
  L.build = nullptr;
  L.index.reset(0);
  L.cap = 0;
  L.ready = false;
}

// Creates the lane (caller holds D.lat.mu, device set).  Lock order: lat.mu
// before D.mu (the slot's base-point tables, which the octet kernel reads,
// are created under D.mu and immutable afterwards).
inline int lat_ready(Device& D) {
  LatLane& L = D.lat;
  if (L.ready) return SV_OK;
  int rc;
  {
    std::lock_guard<std::mutex> g(D.mu);
    if ((rc = ready_locked(D))) return rc;
  }
  int least = 0, greatest = 0;
  SV_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
  L.nctx = (int)std::min<size_t>(kLatCtxMax, std::max<size_t>(1, env_size("SV_LAT_CONTEXTS", 2)));
  L.ready = true;  // (release_lat cleans up whatever exists from here on)
  hipError_t e = hipSuccess;
  for (int k = 0; k < L.nctx && e == hipSuccess; ++k) {
    LatCtx& c = L.ctx[k];
    c.z_out.mapped = c.z_keys.mapped = c.z_stat.mapped = true;
    c.h_in.mapped = true;  // (the kernels read it in place: lat_in_place)
    e = hipStreamCreateWithPriority(&c.stream, hipStreamNonBlocking, greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&c.hstream, hipStreamNonBlocking, greatest);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c.done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c.keys_down, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c.ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c.dev_done, hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&L.build, hipStreamNonBlocking, least);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev_lat, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&L.ctab, sv_comb_btab_bytes());
  if (e == hipSuccess) e = sv_launch_comb_btab((uint32_t*)L.ctab, L.ctx[0].stream);
  if (e == hipSuccess) e = hipStreamSynchronize(L.ctx[0].stream);
  if (e != hipSuccess) {
    release_lat(L);
    return hip_fail(e, "latency lane init");
  }
  const size_t build_bytes = kMaxBuildsPerBatch * 36;
  if ((rc = L.h_build.ensure(build_bytes)) || (rc = L.d_build.ensure(build_bytes))) {
    release_lat(L);
    return rc;
  }
  return SV_OK;
}

// Sizes the key cache to key_cache_cap() (caller holds L.mu, device set).  An
// allocation failure leaves the cache off: the octet kernel needs no tables.
inline void lat_cache_ready(LatLane& L) {
  const size_t cap = key_cache_cap();
  if (cap == L.cap) return;
  lat_sync(L);  // (no queued kernel reads the tables; a batch past its launch only copies out)
  (void)hipStreamSynchronize(L.build);
  lat_drop_builds(L);
  L.ktab.release();
  L.kstat.release();
  L.index.reset(0);
  L.cap = 0;
  if (cap == 0) return;
  if (L.ktab.ensure(cap * sv_key_slot_bytes()) != SV_OK || L.kstat.ensure(cap * 4) != SV_OK) {
    L.ktab.release();
    L.kstat.release();
    return;
  }
  L.index.reset(cap);
  L.cap = cap;
}

// Promotes the slots of finished builds to READY.
inline void lat_poll(LatLane& L) {
  while (!L.inflight.empty()) {
    LatLane::Build& b = L.inflight.front();
    const hipError_t q = hipEventQuery(b.done);
    if (q == hipErrorNotReady) break;
    for (int32_t s : b.slots) {
      if (q == hipSuccess) L.index.set_ready(s, b.gen);
      else L.index.drop(s, b.gen);
    }
    (void)hipEventDestroy(b.uploaded);
    (void)hipEventDestroy(b.done);
    L.inflight.pop_front();
  }
}

// Looks up every key of the batch: true iff all are READY (L.kslots holds
// their slots).  Keys admitted on this sighting are inserted as BUILDING and
// listed in fresh_pk / fresh_slot for lat_build.
inline bool lat_plan(LatLane& L, const HostIn& in, size_t n) {
  L.fresh_pk.clear();
  L.fresh_slot.clear();
  if (!L.cap) return false;
  const uint64_t now = ++L.tick;
  L.kslots.resize(n);
  bool warm = true;
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* pk = in.pkp(i);
    int32_t s = L.index.find(pk);
    if (s >= 0) {
      L.index.touch(s, now);
      if (L.index.state(s) == sv::KeyIndex::READY) {
        L.kslots[i] = (uint32_t)s;
        continue;
      }
      warm = false;  // (its build is still running)
      continue;
    }
    warm = false;
    if (L.fresh_pk.size() < kMaxBuildsPerBatch && L.index.admit(pk)) {
      bool ev = false;
      s = L.index.insert(pk, L.next_gen, now, &ev);
      if (s >= 0) {
        L.fresh_pk.push_back(pk);
        L.fresh_slot.push_back(s);
        if (ev) ++L.evicted;
      }
    }
  }
  return warm;
}

// Queues the table build of the keys lat_plan admitted, after everything
// already on the lane's verify streams (a build may overwrite an evicted slot
// that an earlier comb kernel reads, on either context).  A failed build only
// leaves its keys uncached.
inline void lat_build(LatLane& L) {
  const size_t k = L.fresh_pk.size();
  if (!k) return;
  const uint64_t gen = L.next_gen++;
  LatLane::Build b;
  b.gen = gen;
  b.uploaded = b.done = nullptr;
  b.slots = L.fresh_slot;
  hipError_t e = hipSuccess;
  // the previous build's upload has left the pinned buffer before it is rewritten
  if (!L.inflight.empty()) e = hipEventSynchronize(L.inflight.back().uploaded);
  uint8_t* h = (uint8_t*)L.h_build.p;
  if (e == hipSuccess) {
    for (size_t i = 0; i < k; ++i) {
      std::memcpy(h + 32 * i, L.fresh_pk[i], 32);
      const uint32_t s = (uint32_t)L.fresh_slot[i];
      std::memcpy(h + 32 * k + 4 * i, &s, 4);
    }
    e = hipEventCreateWithFlags(&b.uploaded, hipEventDisableTiming);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&b.done, hipEventDisableTiming);
  for (int c = 0; c < L.nctx && e == hipSuccess; ++c) {
    e = hipEventRecord(L.ctx[c].ev, L.ctx[c].stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(L.build, L.ctx[c].ev, 0);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(L.d_build.p, h, 36 * k, hipMemcpyHostToDevice, L.build);
  if (e == hipSuccess) e = hipEventRecord(b.uploaded, L.build);
  if (e == hipSuccess)
    e = sv_launch_keytab(L.d_build.p, (const uint32_t*)((uint8_t*)L.d_build.p + 32 * k), (uint32_t)k,
                         (uint32_t*)L.ktab.p, (uint32_t*)L.kstat.p, L.build);
  if (e == hipSuccess) e = hipEventRecord(b.done, L.build);
  if (e != hipSuccess) {
    // (an upload already queued completes on its own; the slots stay uncached)
    if (b.uploaded) (void)hipEventSynchronize(b.uploaded);
    for (int32_t s : b.slots) L.index.drop(s, gen);
    if (b.uploaded) (void)hipEventDestroy(b.uploaded);
    if (b.done) (void)hipEventDestroy(b.done);
    return;
  }
  L.built += k;
  L.inflight.push_back(std::move(b));
}

// Zero-copy verdicts (SV_LAT_ZERO_COPY, default on): the kernel of a
// verdict-only latency batch writes its verdicts straight into mapped pinned
// memory, which saves the blit dispatch of a D2H copy (~6 us of a ~0.12 ms
// batch, tools/gpu/api_probe.hip).

inline std::atomic<int> g_lat_zc{-1};
inline bool lat_zero_copy() {
  int v = g_lat_zc.load();
  if (v < 0) {
    const char* e = getenv("SV_LAT_ZERO_COPY");
    v = (e && e[0] == '0') ? 0 : 1;
    g_lat_zc.store(v);
  }
  return v != 0;
}

// Input read in place (SV_LAT_ZC_IN, default on; 0: one staged H2D copy):
// the kernels read the packed image straight from mapped pinned memory.  The
// kernel runs longer (+10 us at 1k signatures, reads over the fabric) but the
// H2D dispatch is gone: p50 1000 / 4096 / 12288 warm 0.116 / 0.261 / 0.551 ->
// 0.112 / 0.253 / 0.508 ms, and a staged copy queues behind a bulk call's
// chunk upload (up to ~0.8 ms per 32 MB chunk): p99 under the 2^22 host
// batch 0.61-0.86 -> 0.22 ms (profiles/r04/isolation/).
// Cold latency batches of at most this many signatures take the three-wave
// octet kernel (SV_OCT_HI_MAX; 0: never).  Measured (profiles/r05/octet_hi/):
// p50 1k 0.241-0.245 -> 0.221-0.226 ms, 2k 0.256 -> 0.240, 4k 0.378 -> 0.375;
// at 6k the third wave's repeated doublings cost more than they save (0.50
// against 0.42-0.44 ms).
inline size_t oct_hi_max() {
  static const size_t v = env_size("SV_OCT_HI_MAX", 4096);
  return v;
}
// Above this many signatures (more octet workgroups than CUs) the third wave
// takes W / 4 of the windows instead of W / 6 (SV_KP_OCT_HI_WIDE): 4k p50
// 0.372 -> 0.352 ms, where 1k and 2k are 2-5 us faster with W / 6
// (profiles/r05/octet_hi/cold_r5an_flags_divisors.jsonl, cold_r5ao_flags.jsonl).
inline size_t oct_hi_wide_min() {
  static const size_t v = env_size("SV_OCT_HI_WIDE_MIN", 2048);
  return v;
}

inline bool lat_in_place() {
  static const bool b = env_size("SV_LAT_ZC_IN", 1) != 0;
  return b;
}

inline std::atomic<int> g_lat_trace{-1};
inline bool lat_trace() {
  int v = g_lat_trace.load();
  if (v < 0) {
    v = getenv("SV_LAT_TRACE") ? 1 : 0;
    g_lat_trace.store(v);
  }
  return v != 0;
}

// Host-side stages of this thread's last latency-lane batch (sv_lat_last_trace).
inline thread_local std::array<double, 8> t_lat_last{};

// A cold launch on context c's stream (caller holds L.mu, device set): above
// kOctetMax the quad kernel on the context's workspace, else the octet kernel
// (hi: its three-wave flags, stat: that variant's failure word).
inline bool lat_quad(uint64_t n) { return n > kOctetMax && !(g_dbg.load() & SV_DBG_NO_QUAD); }
inline int lat_launch_cold(Device& D, LatCtx& c, int mode, const void* pk, const void* sig, const void* msg,
                           const uint64_t* off, const uint32_t* len, uint32_t fixed, uint64_t n, void* verdict,
                           void* bitmap, uint32_t hi, uint32_t* stat) {
  const uint32_t dbg = g_dbg.load() & kKernelDbgMask;
  if (!lat_quad(n)) {
    SV_HIP(sv_launch_verify(mode, SV_PATH_LATENCY, 1, pk, sig, msg, off, len, fixed, n, verdict, bitmap, nullptr,
                            D.btab, dbg | hi, 0, nullptr, stat, c.stream));
    return SV_OK;
  }
  int rc;
  if ((rc = lat_ws(c, sv_verify_ws_bytes(kGeomQuad, 0, n)))) return rc;
  SV_HIP(sv_launch_verify(mode, kGeomQuad, 1, pk, sig, msg, off, len, fixed, n, verdict, bitmap, c.ws.p, D.btab,
                          dbg | SV_KP_LAT, 0, nullptr, nullptr, c.stream));
  return SV_OK;
}

// What a launched latency batch leaves for its completion (lat_finish).
struct LatPending {
  size_t n = 0;
  bool warm = false, early = false, zc = false, zk = false, in_place = false;
  const uint8_t* vho = nullptr;  // its verdicts on the host, once `done`
  const volatile uint32_t* stat = nullptr;  // its kernel's failure word, once `done` (nullptr: none)
  uint8_t* kho = nullptr;        // its cache keys on the host, once `keys_down`
  std::chrono::steady_clock::time_point t0, t1, t_up, t_k, t_down, t_b;
};

// One latency-bound host batch on context c of the slot's latency lane,
// launched (caller holds L.mu): pinned image (+ the key slots when warm) read
// in place (or one H2D), [hash kernel, keys D2H], the comb kernel (every key
// cached) or the octet / quad kernel, one D2H; then the key-table builds it
// admitted.  lat_finish waits and copies out, without the lock.
inline int lat_launch_locked(Device& D, LatCtx& c, const HostIn& in, size_t n, uint8_t* verdict, uint8_t* keys,
                             const KeysCb& kcb, LatPending& pd) {
  LatLane& L = D.lat;
  int rc;
  pd.t0 = std::chrono::steady_clock::now();
  pd.n = n;
  D.lat_last_ns.store(now_ns(), std::memory_order_relaxed);
  audit_lane_count(D);
  lat_cache_ready(L);
  lat_poll(L);
  const uint32_t dbg = g_dbg.load() & kKernelDbgMask;
  // (the lattice test knobs select the octet kernel's code paths)
  const bool warm = lat_plan(L, in, n) && verdict && dbg == 0;
  pd.warm = warm;
  size_t msg_total;
  const Image im = image_of(in, 0, n, &msg_total);
  const size_t o_ks = (im.bytes + 3) & ~(size_t)3;
  const size_t in_bytes = warm ? o_ks + 4 * n : im.bytes;
  // zero-copy outputs: verdicts (and a keyed batch's cache keys) written by
  // the kernels straight into mapped pinned memory, no D2H blit
  const bool zc = verdict && lat_zero_copy();
  const bool zk = keys && lat_zero_copy();
  pd.zc = zc;
  pd.zk = zk;
  const size_t out_per = (verdict && !zc ? 1 : 0) + (keys && !zk ? 32 : 0);
  const bool in_place = lat_in_place();
  pd.in_place = in_place;
  if ((rc = c.h_in.ensure(in_bytes)) || (!in_place && (rc = c.d_in.ensure(in_bytes)))) return rc;
  if (zc && (rc = c.z_out.ensure(n))) return rc;
  if (zk && (rc = c.z_keys.ensure(32 * n))) return rc;
  if (out_per && (rc = c.h_out.ensure(out_per * n))) return rc;
  if (verdict && !zc && (rc = c.d_out.ensure(n))) return rc;
  if (keys && !zk && (rc = c.d_keys.ensure(32 * n))) return rc;
  uint8_t* h = (uint8_t*)c.h_in.p;
  pack(in, 0, n, im, h);
  if (warm) std::memcpy(h + o_ks, L.kslots.data(), 4 * n);
  pd.t1 = std::chrono::steady_clock::now();
  if (!in_place) SV_HIP(hipMemcpyAsync(c.d_in.p, h, in_bytes, hipMemcpyHostToDevice, c.stream));
  pd.t_up = std::chrono::steady_clock::now();
  uint8_t* d = (uint8_t*)(in_place ? c.h_in.dp : c.d_in.p);
  void* d_verdict = zc ? c.z_out.dp : c.d_out.p;
  void* d_keys = zk ? c.z_keys.dp : c.d_keys.p;
  const uint64_t* d_off = im.var ? (const uint64_t*)(d + im.o_off) : nullptr;
  const uint32_t* d_len = im.var ? (const uint32_t*)(d + im.o_len) : nullptr;
  uint8_t* ho = (uint8_t*)c.h_out.p;
  pd.vho = zc ? (const uint8_t*)c.z_out.p : ho;                  // verdicts on the host
  pd.kho = zk ? (uint8_t*)c.z_keys.p : ho + (verdict && !zc ? n : 0);  // keys on the host
  pd.early = kcb && keys && verdict;
  pd.t_k = pd.t_up;
  // A keyed batch's cache keys: with the image read in place, on the
  // context's second stream, beside the verify kernel (the caller's cache
  // walk then overlaps the verification); the windows are staged in LDS (kind 2).
  const bool kside = keys && in_place;
  hipStream_t ks = kside ? c.hstream : c.stream;
  if (keys) {
    SV_HIP(sv_launch_hash(in_place ? 2 : 0, D.grid * 2, d, d + im.o_sig, d + im.o_msg, d_off, d_len, in.fixed, n,
                          d_keys, ks));
    if (!zk) SV_HIP(hipMemcpyAsync(pd.kho, c.d_keys.p, 32 * n, hipMemcpyDeviceToHost, ks));
    SV_HIP(hipEventRecord(c.keys_down, ks));
  }
  if (verdict) {
    const int mode = verify_mode(im.var, in.fixed);
    if ((rc = L.timer.begin(c.stream))) return rc;
    // (while bulk work runs, only the 1-signature-per-wave geometry fits the
    // slot a shared-mode bulk launch leaves free on each CU)
    const bool bulk_busy = hipStreamQuery(D.stream) == hipErrorNotReady;
    if (warm)
      SV_HIP(sv_launch_comb(mode, bulk_busy ? 1 : sv_comb_spw(n, D.cus), d, d + im.o_sig, d + im.o_msg, d_off, d_len, in.fixed, n,
                            d_verdict, (const uint32_t*)(d + o_ks), (const uint32_t*)L.ktab.p,
                            (const uint32_t*)L.kstat.p, (const uint32_t*)L.ctab, c.stream));
    else {
      // (a third wave per workgroup takes the chains' top windows while no
      // bulk work runs: its larger workgroup would not fit the slot a
      // shared-mode bulk launch leaves free)
      const uint32_t hi = (!lat_quad(n) && !bulk_busy && n <= oct_hi_max())
                              ? SV_KP_OCT_HI | (n > oct_hi_wide_min() ? SV_KP_OCT_HI_WIDE : 0u)
                              : 0u;
      // (the three-wave kernel's hand-overs are bounded waits: it reports one
      // that ran out in this word, and lat_finish turns that into an error)
      uint32_t* stat = nullptr;
      if (hi) {
        if ((rc = c.z_stat.ensure(sizeof(uint32_t)))) return rc;
        *(volatile uint32_t*)c.z_stat.p = 0;
        stat = (uint32_t*)c.z_stat.dp;
        pd.stat = (const volatile uint32_t*)c.z_stat.p;
      }
      if ((rc = lat_launch_cold(D, c, mode, d, d + im.o_sig, d + im.o_msg, d_off, d_len, in.fixed, n, d_verdict,
                                nullptr, hi, stat)))
        return rc;
    }
    if ((rc = L.timer.end(c.stream, n))) return rc;
    pd.t_k = std::chrono::steady_clock::now();
    if (!zc) SV_HIP(hipMemcpyAsync(ho, c.d_out.p, n, hipMemcpyDeviceToHost, c.stream));
  }
  SV_HIP(hipEventRecord(c.done, c.stream));
  pd.t_down = std::chrono::steady_clock::now();
  lat_build(L);  // (after the verify work: a build waits for it on the device)
  pd.t_b = std::chrono::steady_clock::now();
  if (warm) ++L.warm;
  else ++L.cold;
  return SV_OK;
}

// The rest of a launched batch, without the lane's lock: the keys-ready
// callback, the wait, the copy-out.
inline int lat_finish(LatCtx& c, const LatPending& pd, uint8_t* verdict, uint8_t* keys, const KeysCb& kcb,
                      bool* cb_done) {
  const size_t n = pd.n;
  if (pd.early) {
    SV_HIP(hipEventSynchronize(c.keys_down));
    std::memcpy(keys, pd.kho, 32 * n);
    kcb(n);
    *cb_done = true;
  }
  SV_HIP(hipEventSynchronize(c.done));
  if (keys && !pd.early) SV_HIP(hipEventSynchronize(c.keys_down));
  // An in-kernel failure: the kernel wrote fail-closed rejects, which are not
  // verdicts.  The batch errs (include/stellar_sigverify.h: an error is never
  // a reject), so a caller re-verifies it instead of caching false
  // (src/crypto/SecretKey.cpp:464-466 of stellar-core caches what it gets).
  if (pd.stat && *pd.stat != 0)
    return fail(SV_ERR_KERNEL, "in-kernel failure " + std::to_string(*pd.stat) +
                                   " (three-wave octet kernel: a hand-over wait ran out); verdicts discarded");
  if (verdict) std::memcpy(verdict, pd.vho, n);
  if (keys && !pd.early) std::memcpy(keys, pd.kho, 32 * n);
  const auto t2 = std::chrono::steady_clock::now();
  auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
  };
  t_lat_last = {us(pd.t0, pd.t1), us(pd.t1, pd.t_up), us(pd.t_up, pd.t_k), us(pd.t_k, pd.t_down),
                us(pd.t_down, pd.t_b), us(pd.t_b, t2), us(pd.t0, t2), pd.warm ? 1.0 : 0.0};
  if (lat_trace()) {
    fprintf(stderr,
            "SV_LAT_TRACE n=%zu %s plan+pack %.1f us | h2d call %.1f launch %.1f d2h+rec %.1f build %.1f sync %.1f"
            " | device %.1f us @%.1f%s\n",
            n, pd.warm ? "warm" : "cold", us(pd.t0, pd.t1), us(pd.t1, pd.t_up), us(pd.t_up, pd.t_k),
            us(pd.t_k, pd.t_down), us(pd.t_down, pd.t_b), us(pd.t_b, t2), us(pd.t1, t2),
            trace_abs_us() - us(pd.t0, t2), pd.in_place ? " in place" : "");
  }
  return SV_OK;
}

inline int lat_slice(Device& D, const HostIn& in, size_t n, uint8_t* verdict, uint8_t* keys, const KeysCb& kcb,
                     bool* cb_done) {
  LatLane& L = D.lat;
  std::unique_lock<std::mutex> lk(L.mu);
  SV_HIP(hipSetDevice(D.phys));
  int rc;
  if ((rc = lat_ready(D))) return rc;
  // a free context (every one busy: wait for the first batch to finish)
  LatCtx* c = nullptr;
  L.freed.wait(lk, [&] {
    for (int k = 0; k < L.nctx; ++k)
      if (!L.ctx[k].busy) {
        c = &L.ctx[k];
        return true;
      }
    return false;
  });
  c->busy = true;
  // Releases the context however this call leaves (an error return, or an
  // exception from the keys-ready callback inside lat_finish): unless the
  // batch completed, its streams are drained first, so the next batch on the
  // context never overwrites staging a kernel still reads.  (notify_all: a
  // device-API caller waiting here takes no context, so a single wake-up
  // could land on it and leave a host batch asleep beside a free one.)
  struct Release {
    LatLane& L;
    LatCtx* c;
    std::unique_lock<std::mutex>& lk;
    bool completed = false;
    ~Release() {
      if (!completed) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->hstream);
      }
      if (!lk.owns_lock()) lk.lock();
      c->busy = false;
      L.freed.notify_all();
    }
  } release{L, c, lk};
  LatPending pd;
  if ((rc = lat_launch_locked(D, *c, in, n, verdict, keys, kcb, pd))) return rc;
  lk.unlock();
  rc = lat_finish(*c, pd, verdict, keys, kcb, cb_done);
  release.completed = rc == SV_OK;
  // A keyed batch's keys and verdicts into the slot's journal (sv_set_verdict_cache_feed; one relaxed load while
  // the bit is clear): the next drain on the bulk stream inserts them.  The rows come from the context's own
  // pinned copies, which the kernels wrote and only this batch holds -- not from the caller's arrays, which the
  // keys-ready callback has already handed to the caller -- so the context stays busy for the copy.  The lane
  // itself still never touches the table.  An error appended nothing.
  if (rc == SV_OK && (vc_feed() & SV_VC_FEED_LANE) && keys && verdict && vc_entries() &&
      !(g_dbg.load() & SV_DBG_PREP_ONLY)) {
    const size_t cap = vc_journal_rows();
    D.vj.append(pd.kho, pd.vho, n, cap);
    // SV_VC_SHARE_FEED (sv_set_verdict_cache_share; one more relaxed load): the same rows from the same pinned
    // copies into every other slot's journal, each with its own bound and its own fed_overflow -- G copies on
    // this return path where there was one
    if ((vc_share() & SV_VC_SHARE_FEED) && g_devs.size() > 1) {
      for (Device* P : g_devs)
        if (P != &D) P->shared_in.fetch_add(P->vj.append(pd.kho, pd.vho, n, cap), std::memory_order_relaxed);
      D.shq.count_out(n);
    }
  }
  return rc;
}

}  // namespace
}  // namespace sv
