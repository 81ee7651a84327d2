// State of the engine: error reporting, device and pinned buffers, the
// staging slots, the latency lane's contexts, the per-key tables, the verdict cache, the verdict audit, the Device
// slot with the creation and release of its resources, the slot table and the
// process-wide settings.  Included by sv_api.cpp (and by bulk.h and latlane.h,
// which work on this state).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/stellar_sigverify.h"
#include "audit.h"
#include "host_env.h"
#include "keycache.h"
#include "keytab.h"
#include "launch.h"
#include "pool.h"
#include "txstore.h"
#include "vcache.h"
#include "vjournal.h"
#include "vshare.h"

namespace sv {
namespace {

inline thread_local std::string t_err;
inline int fail(int code, const std::string& msg) {
  t_err = msg;
  return code;
}
inline int hip_fail(hipError_t e, const char* what) {
  return fail(SV_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define SV_HIP(call)                                   \
  do {                                                 \
    hipError_t _e = (call);                            \
    if (_e != hipSuccess) return hip_fail(_e, #call);  \
  } while (0)

// Kernel-time accounting (sv_timing_enable): begin / end bracket a launch on
// a stream with a pair of events, harvest adds the finished pairs to the
// totals.  Used under its owner's mutex (Device::mu, LatLane::mu).  A bracket
// that a failing HIP call cuts short leaves at most its first event, which
// the next begin (or release) destroys.
inline std::atomic<int> g_timing{0};
struct KernelTimer {
  double total_ms = 0;
  uint64_t launches = 0, sigs = 0;

  int begin(hipStream_t st) {
    drop_open();
    if (!g_timing.load()) return SV_OK;
    SV_HIP(hipEventCreate(&open_));
    SV_HIP(hipEventRecord(open_, st));
    return SV_OK;
  }
  int end(hipStream_t st, uint64_t n) {
    if (!open_) return SV_OK;
    Span sp{open_, nullptr, n};
    open_ = nullptr;
    hipError_t e = hipEventCreate(&sp.e1);
    if (e == hipSuccess) e = hipEventRecord(sp.e1, st);
    if (e != hipSuccess) {
      destroy(sp);
      return hip_fail(e, "kernel timing");
    }
    pending_.push_back(sp);
    return SV_OK;
  }
  int harvest() {
    while (!pending_.empty()) {
      const Span& sp = pending_.front();
      SV_HIP(hipEventSynchronize(sp.e1));
      float ms = 0;
      SV_HIP(hipEventElapsedTime(&ms, sp.e0, sp.e1));
      total_ms += ms;
      launches += 1;
      sigs += sp.n;
      destroy(sp);
      pending_.pop_front();
    }
    return SV_OK;
  }
  void reset() {
    total_ms = 0;
    launches = sigs = 0;
  }
  // (the owner's streams are drained)
  void release() {
    drop_open();
    for (const Span& sp : pending_) destroy(sp);
    pending_.clear();
  }

 private:
  struct Span {
    hipEvent_t e0, e1;
    uint64_t n;
  };
  static void destroy(const Span& sp) {
    if (sp.e0) (void)hipEventDestroy(sp.e0);
    if (sp.e1) (void)hipEventDestroy(sp.e1);
  }
  void drop_open() {
    if (open_) (void)hipEventDestroy(open_);
    open_ = nullptr;
  }
  hipEvent_t open_ = nullptr;  // begin's event of the bracket in progress
  std::deque<Span> pending_;
};

// Keys-ready notification of the keyed gather entry points: fn(ctx, ready)
// with keys [0, ready) in the caller's array, called with increasing `ready`,
// the last time with ready == n.
struct KeysCb {
  void (*fn)(void*, size_t) = nullptr;
  void* ctx = nullptr;
  explicit operator bool() const { return fn != nullptr; }
  void operator()(size_t ready) const { fn(ctx, ready); }
};
// Depth of engine entry points on this thread (sv_api.cpp LifeGuard); > 0 also on a
// KeyNotifier thread, whose callbacks run inside the caller's entry point, so
// sv_shutdown / sv_set_device_map from a callback is refused there too.
inline thread_local int t_life_depth = 0;

// NUMA node of a GPU (-1: unknown) from its PCI address.
inline int gpu_numa_node(int phys) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), phys) != hipSuccess) return -1;
  return pci_numa_node(bus);
}

// ------------------------------------------------------------ buffers
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return SV_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = std::max<size_t>(bytes, 1 << 16);
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(SV_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    cap = want;
    return SV_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// Pinned host staging (hipHostMalloc).  `mapped` buffers are fine-grained
// (coherent) and read / written by kernels in place: `dp` is their device
// address.
struct HostBuf {
  void* p = nullptr;
  void* dp = nullptr;
  size_t cap = 0;
  bool mapped = false;
  int ensure(size_t bytes) {
    if (bytes <= cap) return SV_OK;
    release();
    const size_t want = std::max<size_t>(bytes + bytes / 8, 1 << 16);
    hipError_t e =
        hipHostMalloc(&p, want, mapped ? (hipHostMallocMapped | hipHostMallocCoherent) : hipHostMallocDefault);
    if (e == hipSuccess && mapped) e = hipHostGetDevicePointer(&dp, p, 0);
    if (e != hipSuccess) {
      release();
      return fail(SV_ERR_ALLOC, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    cap = want;
    return SV_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = dp = nullptr;
    cap = 0;
  }
};

// One pinned + device staging slot of the host-buffer pipeline.
struct Stage {
  HostBuf h_in, h_out;
  DevBuf d_in, d_verdict, d_keys;
  DevBuf d_pair;  // hinted tx-body chunks: the pairing workspace, then pair_begin / pair_sig / pair_key
  HostBuf h_cnt;  // ... and the chunk's pair count, read back before its verify launch
  DevBuf d_acct;  // by-account check chunks: the expansion's workspace and the tables it fills (sv_txacct.hip)
  hipEvent_t up = nullptr, done = nullptr, down = nullptr, keys_down = nullptr;
  std::vector<hipEvent_t> pev;  // keys of piece k are down (one-chunk keyed batches)
  bool busy = false;  // a chunk's D2H is pending on `down`
  size_t lo = 0, m = 0;
  const uint8_t* zv = nullptr;  // the chunk's verdicts in mapped memory (written in place), else in h_out
};

// Latency lane of a slot.  Batches that take the latency kernels (one staging
// chunk, SV_PATH_LATENCY) run here on their own high-priority stream, pinned
// staging and mutex, so an SCP batch never waits on the host side for the
// slot's bulk work (a tx set or a catchup batch holding Device::mu).  The lane
// also owns the key cache of the warm-key kernel (keycache.h, comb.h): a batch
// whose keys are all cached runs sv_comb_kernel, any other batch the octet
// kernel, after which its new keys are queued for a table build on the
// low-priority build stream.
// One latency batch in flight on the lane: its staging and streams.  The
// lane's mutex covers a batch's planning and launch; its wait and copy-out
// run outside it, so with two contexts the next batch (an SCP burst's second
// micro-batch) is planned and launched while the first one runs, instead of
// queueing behind it on the host (SV_LAT_CONTEXTS, default 2; 1 serialises).
struct LatCtx {
  hipStream_t stream = nullptr;   // verify work (highest priority)
  hipStream_t hstream = nullptr;  // a keyed batch's cache keys, beside the verify kernel (highest priority)
  hipEvent_t done = nullptr, keys_down = nullptr;
  hipEvent_t ev = nullptr;        // (a key-table build waits for the work queued here)
  hipEvent_t dev_done = nullptr;  // a device-API batch queued here is done (the caller's stream waits on it;
                                  // `done` stays the host batch's own, which must not wait for device-API work)
  HostBuf h_in, h_out;
  HostBuf z_out;   // mapped: the kernels write verdicts in place
  HostBuf z_keys;  // mapped: the hash kernel writes cache keys in place (keyed batches)
  HostBuf z_stat;  // mapped: the launch's failure word (sv_kparams::status), zeroed per batch
  DevBuf d_in, d_out, d_keys;
  DevBuf ws;  // the quad kernel's tables (cold batches above kOctetMax)
  bool busy = false;  // (under LatLane::mu) a batch holds it
};
constexpr int kLatCtxMax = 2;
struct LatLane {
  std::mutex mu;
  std::condition_variable freed;  // a context was released
  bool ready = false;
  int nctx = 1;
  LatCtx ctx[kLatCtxMax];
  hipStream_t build = nullptr;   // key-table builds (lowest priority)
  hipEvent_t ev_lat = nullptr;   // (device-API batches: the caller's stream)
  HostBuf h_build;
  DevBuf d_build;
  void* ctab = nullptr;  // tables of B (built at lane init)
  DevBuf ktab, kstat;    // tables of -A per cached key, status per slot
  size_t cap = 0;        // key-cache capacity the index / tables are sized for
  sv::KeyIndex index;
  uint64_t tick = 0, next_gen = 1;
  struct Build {
    uint64_t gen;
    hipEvent_t uploaded, done;
    std::vector<int32_t> slots;
  };
  std::deque<Build> inflight;
  KernelTimer timer;  // the lane's verify launches
  std::vector<uint32_t> kslots;          // per signature of the batch being planned
  std::vector<const uint8_t*> fresh_pk;  // keys admitted by it
  std::vector<int32_t> fresh_slot;
  uint64_t warm = 0, cold = 0, built = 0, evicted = 0;
};

// Per-key tables of the throughput path (sv_kernels.hip sv_keyslot_kernel),
// one set per slot: claim words, entries, per-chunk slot and builder lists,
// the two counters and a pinned copy of them (read lazily: the claims decide
// when the claim words are cleared, never a verdict).
struct KeyTabs {
  DevBuf index, store, kslot, builders, count;
  HostBuf h_count;
  hipEvent_t copied = nullptr;  // h_count holds the counters after the last launch
  size_t slots = 0;
  uint64_t salt = 0;
  uint64_t launches = 0, clears = 0, claims = 0;
};

// The verdict cache of a slot (vcache.h, sv_vcache.hip; bulk.h launch_cached_locked): the table, its claim words,
// the device counters (hits | inserted | dropped | the pass's miss count), the pinned word the miss count comes
// back in and the compaction workspace of the largest cached launch so far.  Allocated on the first cached launch
// after a non-zero capacity was set (sv_set_verdict_cache); touched only by kernels on D.stream, under D.mu.
// The feed (sv_set_verdict_cache_feed): `counters` continues with present | inserted | dropped of the journal's
// drains (words 4-6); a drain moves the taken rows through the pinned `h_feed` into `ws` (`fed_up`: the upload
// has left h_feed, which the next drain rewrites).
struct VerdictCache {
  DevBuf tab, claim, counters, ws;
  HostBuf h_cnt;
  HostBuf h_feed;
  hipEvent_t fed_up = nullptr;
  JournalRows taken;  // the rows of the drain in progress (its buffers go back to the journal at the next take)
  size_t entries = 0;    // entries of `tab` (0: not allocated)
  uint64_t lookups = 0;  // items probed
  double wait_ms = 0;    // host time spent waiting for miss counts
  KernelTimer timer;     // the cache's own kernels (keys, probe, scan, fill, gather; claim, store, bitmap)
  size_t bytes() const { return tab.cap + claim.cap + counters.cap + ws.cap; }
  // (D.stream is drained)
  void release() {
    tab.release(); claim.release(); counters.release(); ws.release(); h_cnt.release();
    h_feed.release();
    if (fed_up) (void)hipEventDestroy(fed_up);
    fed_up = nullptr;
    taken = JournalRows();
    timer.release();
    timer.reset();
    entries = 0;
    lookups = 0;
    wait_ms = 0;
  }
};

// A slot's replica of the account store (acctstore.h, txstore.h, sv_txstore.hip): one allocation for the arrays,
// allocated at the slot's first use of the store; `version` is the host store's version the replica holds (0: none,
// or stale after a failed write -- the next use copies the host's arrays up again).  At `version` the replica's
// first `accounts` rows, payload rows and index words are the host copy's, byte for byte (an erased row's zeroed
// counts are scattered too, and a clear zeroes every row's counts on both sides).  Written only by the scatter
// and local kernels on D.stream, under D.mu.  `ws`: a lookup's IDs, rows and gathered accounts (sv_account_store_
// read); `d_stage` / `h_stage`: a write's records on their way up.
struct AcctReplica {
  DevBuf buf, ws, d_stage;
  HostBuf h_stage;
  sv_store_tab tab{};
  uint64_t version = 0;
  uint32_t max_probe = 1;  // the host's bound as of `version`
  uint64_t lookups = 0;
  KernelTimer timer;  // the lookup kernel
  size_t bytes() const { return buf.cap + ws.cap + d_stage.cap; }
  // (D.stream is drained)
  void release() {
    buf.release(); ws.release(); d_stage.release(); h_stage.release();
    tab = sv_store_tab{};
    version = 0;
    max_probe = 1;
    lookups = 0;
    timer.release();
    timer.reset();
  }
};

// The verdict audit of a slot (audit.h, sv_audit.hip; bulk.h audit_locked): the device counters with the ring
// behind them (`state`: SV_AC_WORDS words, then SV_AUDIT_RING records), the pick list, audit bytes and block sums
// of the largest audited launch so far (`buf`), and the pinned words the counters (64 bytes) and the ring come
// back in.  Allocated at the slot's first audited launch; touched only by kernels on D.stream, under D.mu.
// seq: audited launches of the bulk route so far.  seen: `mismatches` as of the last read-back (the strict check
// compares against it).  lane_launches: latency-lane launches while the audit was on, which are not audited.
struct Audit {
  DevBuf state, buf;
  HostBuf h_rd;
  uint64_t seq = 0, seen = 0;
  int blocks_per_cu = 0;
  std::atomic<uint64_t> lane_launches{0};
  KernelTimer timer;  // the audit's kernels
  static constexpr size_t kRingOff = 8 * SV_AC_WORDS;
  static constexpr size_t kStateBytes = kRingOff + (size_t)SV_AUDIT_RING * sizeof(sv_audit_record);
  size_t bytes() const { return state.cap + buf.cap; }
  // (D.stream is drained)
  void release() {
    state.release(); buf.release(); h_rd.release();
    timer.release();
    timer.reset();
    seq = seen = 0;
    lane_launches.store(0);
  }
};

struct Device {
  int slot = -1;
  int phys = -1;
  bool ready = false;  // resources created lazily on first use (under mu)
  int cus = 0;
  unsigned grid = 0;  // persistent grid (workgroups)
  unsigned grid_share = 0;  // the same in shared mode (latency batches live: share_now)
  hipStream_t stream = nullptr, h2d = nullptr, d2h = nullptr;
  void* btab = nullptr;
  DevBuf ws;  // kernel workspace, grown on demand (after draining `stream`)
  hipEvent_t dep_in = nullptr, dep_out = nullptr;
  std::mutex mu;
  Stage st[2];
  HostBuf z_in;   // mapped: a one-chunk batch's image, read in place (bulk_in_place)
  HostBuf z_out;  // mapped: its verdicts, written in place (bulk_zc_out)
  DevBuf msg, off, len, keys;  // sha256 batches
  HostBuf h_sha;
  DevBuf txmsg;  // tx-body batches: the n x 32 message array the hash kernel fills (grown after draining `stream`)
  // hinted tx-body batches: the pairs' keys (n_pairs x 32) and signatures (n_pairs x 64) gathered next to
  // txmsg for the verify launch, the pairing workspace and the pair count of the device-resident form
  DevBuf txpk, txsg, txpair;
  HostBuf h_txcnt;
  DevBuf txchk;  // device-resident check calls: the pairs' indices and verdicts, which stay inside the engine
  DevBuf txpp;   // check calls with payload candidates: the payload pairs' verdicts, indices and gathered arrays
  // by-account check calls: the account table (host form: its image; both forms: the per-account counts and
  // ranks), and the device-resident form's expansion -- workspace and CSR arrays, then the rows sized from its totals
  DevBuf txatab, txaws, txarows;
  DevBuf txres;  // device-resident decide calls: the check arrays the caller did not ask for, the result kernels' workspace
  // signing calls (sv_sign.hip): the slot's own comb tables of B, built at its first signing call (the latency
  // lane keeps its copy, so the lane's start-up and first batch are what they were); the expanded-key records,
  // cleared behind every call's last kernel; the host form's seeds, chunk inputs and outputs
  void* sign_ctab = nullptr;
  DevBuf sign_rec, sign_seed, sign_in, sign_out;
  KernelTimer timer;  // the bulk launches (launch_locked)
  LatLane lat;
  KeyTabs kt;  // (under mu)
  VerdictCache vc;  // (under mu)
  AcctReplica as;   // (under mu)
  Audit audit;      // (under mu; lane_launches: atomic)
  Journal vj;       // keyed latency-lane batches on their way into vc (its own mutex: vjournal.h)
  // What this slot's cached launches export to the other slots' journals (vshare.h; sv_set_verdict_cache_share):
  // the queue of pending exports and, per buffer of it, the pinned image with the event behind its copy.  A
  // buffer is allocated or grown under mu while the exporter has it reserved, and read by whoever passes the
  // export on; released with D.stream drained (share_release).  shared_in: rows the others appended to vj.
  ShareQueue shq;
  struct ShareBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
  } shb[kSharePending];
  std::atomic<size_t> share_pinned{0};
  std::atomic<uint64_t> shared_in{0};
  std::atomic<int64_t> lat_last_ns{INT64_MIN / 2};  // steady clock of the last latency-lane batch
  std::atomic<uint64_t> shared_launches{0};          // bulk launches in shared mode
  // The slot's own staging workers for multi-slot calls (shard): its slice is
  // driven and packed here, not on the shared pool, so G slots pack on G sets
  // of threads at once.  Pinned to the GPU's NUMA node where the host tells
  // it (slot_pool).  Created on first multi-slot use, under spool_mu.
  std::mutex spool_mu;
  std::unique_ptr<sv::Pool> spool;
  int numa = -2;        // GPU's NUMA node (-1 unknown; -2 not looked up yet)
  size_t numa_cpus = 0;  // CPUs the workers are pinned to (0: not pinned)
};

inline std::mutex g_mu;
inline std::vector<Device*> g_devs;
inline std::vector<int> g_map;  // slot -> physical device (empty: identity)
inline bool g_inited = false;
inline std::atomic<int> g_path{SV_PATH_AUTO};   // sv_set_kernel_path
inline std::atomic<uint32_t> g_dbg{0};          // sv_set_debug_flags
inline std::atomic<size_t> g_min_shard{0};      // sv_set_min_shard (0: default)
inline std::atomic<uint64_t> g_rr{0};           // round-robin slot for single-slot calls

// sv_set_verdict_cache: entries per slot, 0 (the default) off; ~0: SV_VERDICT_CACHE, read once.  Rounded up to
// a power of two >= 4 (one set), at most SV_VC_MAX_ENTRIES.
inline std::atomic<size_t> g_vc_entries{~(size_t)0};
inline size_t vc_round(size_t v) {
  if (!v) return 0;
  size_t p = SV_VC_WAYS;
  while (p < v && p < SV_VC_MAX_ENTRIES) p <<= 1;
  return p;
}
inline size_t vc_entries() {
  const size_t v = g_vc_entries.load();
  if (v != ~(size_t)0) return v;
  static const size_t e = vc_round(env_size("SV_VERDICT_CACHE", 0));
  return e;
}
// sv_set_verdict_cache_feed: the SV_VC_FEED_* sources (~0: SV_VERDICT_CACHE_FEED, resolved at the first read) and
// the rows of a slot's journal (0: SV_VERDICT_CACHE_JOURNAL or kJournalDefaultRows).
inline std::atomic<uint32_t> g_vc_feed{~0u};
inline std::atomic<size_t> g_vc_journal{0};
inline uint32_t vc_feed() {
  uint32_t v = g_vc_feed.load(std::memory_order_relaxed);
  if (v != ~0u) return v;
  const uint32_t e = (uint32_t)env_size("SV_VERDICT_CACHE_FEED", 0) & (SV_VC_FEED_LANE | SV_VC_FEED_BULK);
  g_vc_feed.compare_exchange_strong(v, e);
  return g_vc_feed.load(std::memory_order_relaxed);
}
inline size_t vc_journal_rows() {
  const size_t v = g_vc_journal.load(std::memory_order_relaxed);
  if (v) return std::min(v, kJournalMaxRows);
  // (read once: this sits on the return path of every fed lane batch)
  static const size_t e =
      std::max<size_t>(1, std::min(env_size("SV_VERDICT_CACHE_JOURNAL", kJournalDefaultRows), kJournalMaxRows));
  return e;
}

// sv_set_verdict_cache_share: the SV_VC_SHARE_* bits (~0: SV_VERDICT_CACHE_SHARE, resolved at the first read).
inline std::atomic<uint32_t> g_vc_share{~0u};
inline uint32_t vc_share() {
  uint32_t v = g_vc_share.load(std::memory_order_relaxed);
  if (v != ~0u) return v;
  const uint32_t e = (uint32_t)env_size("SV_VERDICT_CACHE_SHARE", 0) & (SV_VC_SHARE_FEED | SV_VC_SHARE_STORES);
  g_vc_share.compare_exchange_strong(v, e);
  return g_vc_share.load(std::memory_order_relaxed);
}
// Whether cached launches export what they verified: the bit, the cache on and more than one slot.
inline bool share_stores() { return (vc_share() & SV_VC_SHARE_STORES) && g_devs.size() > 1 && vc_entries(); }

// The pinned image and the event of export buffer b of D at `rows` rows (caller holds D.mu, device set, and has
// the buffer reserved: nothing of an earlier export is in flight in it).  A buffer that has to grow at least
// doubles, up to the size of an export of `cap` rows -- the most a launch offers -- so a run of growing launches
// frees and allocates pinned memory (which synchronises the device) a few times, not once per launch.
inline int share_buf_ensure(Device& D, int b, size_t rows, size_t cap) {
  Device::ShareBuf& B = D.shb[b];
  if (!B.ev) SV_HIP(hipEventCreateWithFlags(&B.ev, hipEventDisableTiming));
  size_t want = share_buf_bytes(rows);
  if (want <= B.cap) return SV_OK;
  want = std::max(want, std::min(2 * B.cap, share_buf_bytes(std::max(rows, cap))));
  if (B.p) (void)hipHostFree(B.p);
  D.share_pinned.fetch_sub(B.cap);
  B.p = nullptr;
  B.cap = 0;
  hipError_t e = hipHostMalloc(&B.p, want, hipHostMallocDefault);
  if (e != hipSuccess) {
    B.p = nullptr;
    return fail(SV_ERR_ALLOC, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  }
  B.cap = want;
  D.share_pinned.fetch_add(want);
  return SV_OK;
}
// Forgets D's pending exports and frees their memory, counters included (caller holds D.mu; D.stream is drained,
// or the slot never was ready).
inline void share_release(Device& D) {
  D.shq.reset();
  for (Device::ShareBuf& B : D.shb) {
    if (B.p) (void)hipHostFree(B.p);
    if (B.ev) (void)hipEventDestroy(B.ev);
    B = Device::ShareBuf();
  }
  D.share_pinned.store(0);
  D.shared_in.store(0);
}
// Passes D's complete exports on to every other slot's journal, in export order (vshare.h pass()).  Holds no
// Device::mu of another slot and waits for none; wait: for the events of the exports pending now (D's own
// stream), else nothing is waited for at all.  An event that fails loses its export.
inline void share_pass(Device& D, bool wait) {
  if (!D.shq.pending()) return;
  (void)D.shq.pass(
      wait,
      [&](int b, bool w) -> int {
        const hipError_t e = w ? hipEventSynchronize(D.shb[b].ev) : hipEventQuery(D.shb[b].ev);
        return e == hipSuccess ? 1 : e == hipErrorNotReady ? 0 : -1;
      },
      [&](const uint8_t* image, size_t rows) {
        const size_t cap = vc_journal_rows();
        for (Device* P : g_devs)
          if (P != &D)
            P->shared_in.fetch_add(P->vj.append(image, image + share_image_verdicts(rows), rows, cap),
                                   std::memory_order_relaxed);
      });
}
// ... of every slot: what a cache entry point does on its way (with one slot, or nothing pending, nothing).
inline void share_pass_all(bool wait) {
  if (g_devs.size() < 2) return;
  for (Device* D : g_devs) share_pass(*D, wait);
}
// Marks every slot's pending exports as forgotten (whatever drops the journals drops them first).
inline void share_drop_all() {
  for (Device* D : g_devs) D->shq.drop();
}

// sv_set_audit: the process-wide setting.  what: the SV_AUDIT_* bits, 0 (the default) off; ~0: SV_AUDIT,
// SV_AUDIT_ONE_IN (default 1024) and SV_AUDIT_SEED, read once at first use.  The other three words are written
// under g_audit_mu before `what` is published.
struct AuditCfg {
  uint32_t what = 0, one_in = 0;
  uint64_t seed = 0, budget = 0;
};
inline std::mutex g_audit_mu;
inline std::atomic<uint32_t> g_audit_what{~0u};
inline AuditCfg g_audit_cfg;
inline uint32_t audit_what() {
  uint32_t v = g_audit_what.load(std::memory_order_acquire);
  if (v != ~0u) return v;
  std::lock_guard<std::mutex> g(g_audit_mu);
  v = g_audit_what.load(std::memory_order_acquire);
  if (v != ~0u) return v;
  AuditCfg c;
  c.what = (uint32_t)env_size("SV_AUDIT", 0) & SV_AUDIT_WHAT_MASK;
  c.one_in = (uint32_t)std::min<size_t>(env_size("SV_AUDIT_ONE_IN", 1024), 0xFFFFFFFFu);
  c.seed = (uint64_t)env_size("SV_AUDIT_SEED", 0);
  if (!c.one_in) c.what &= ~SV_AUDIT_SAMPLE;  // (what sv_set_audit refuses)
  if (!(c.what & (SV_AUDIT_REJECTS | SV_AUDIT_SAMPLE))) c.what = 0;
  g_audit_cfg = c;
  g_audit_what.store(c.what, std::memory_order_release);
  return c.what;
}
inline AuditCfg audit_cfg() {
  AuditCfg c;
  if (!audit_what()) return c;
  std::lock_guard<std::mutex> g(g_audit_mu);
  c = g_audit_cfg;
  return c;
}

constexpr uint32_t kKernelDbgMask =
    SV_DBG_TRIVIAL_PAIR | SV_DBG_MAX_WINDOWS | SV_DBG_PREP_ONLY | SV_DBG_KEY_COLLIDE | SV_DBG_DROP_HANDOVER;

// Batches up to this size take the latency kernel under SV_PATH_AUTO
// (measured crossover on MI355X).
constexpr uint64_t kQuickMax = 12288;

inline int resolve_path(int requested, uint64_t n) {
  int p = requested != SV_PATH_AUTO ? requested : g_path.load();
  if (p == SV_PATH_AUTO) p = n <= kQuickMax ? SV_PATH_LATENCY : SV_PATH_THROUGHPUT;
  return p;
}

// Throughput-path launches of at most this many signatures run one signature
// per quad of lanes (sv_kernels.hip sv_quad_kernel): below about one wave per
// SIMD the one-lane kernels run at a lone wave's serial latency
// (tools/size_sweep.py).  SV_QUAD_MAX overrides (0: never).
constexpr uint64_t kQuadMax = 32768;
// Cold latency-lane batches above this size run the quad kernel (on the
// lane, at wave priority 3) instead of the octet kernel: one signature per 4
// lanes instead of 16 overtakes the octet's shorter chains from ~6k
// signatures (tools/size_sweep.py, profiles/r05/size_sweep/).
constexpr uint64_t kOctetMax = 6144;
inline uint64_t quad_max() {
  static const uint64_t v = env_size("SV_QUAD_MAX", kQuadMax);
  return v;
}
constexpr int kGeomQuad = 3;  // sv_launch_verify's path code of the quad geometry
// The kernel geometry of a launch of n on resolved path rp.  (A quad launch
// decodes every key itself: the per-key tables only serve the one-lane
// kernels of larger launches.)
inline int launch_geometry(int rp, uint64_t n) {
  if (rp != SV_PATH_THROUGHPUT) return rp;
  const uint32_t d = g_dbg.load();
  if (d & SV_DBG_NO_QUAD) return rp;
  if (d & SV_DBG_QUAD) return kGeomQuad;
  return n <= quad_max() ? kGeomQuad : rp;
}
inline int path_from_flags(uint32_t flags) {
  if (flags & SV_FLAG_PATH_LATENCY) return SV_PATH_LATENCY;
  if (flags & SV_FLAG_PATH_THROUGHPUT) return SV_PATH_THROUGHPUT;
  return SV_PATH_AUTO;
}

inline int init_device(Device& D) {
  SV_HIP(hipSetDevice(D.phys));
  hipDeviceProp_t prop;
  SV_HIP(hipGetDeviceProperties(&prop, D.phys));
  D.cus = prop.multiProcessorCount;
  SV_HIP(hipStreamCreateWithFlags(&D.stream, hipStreamNonBlocking));
  SV_HIP(hipStreamCreateWithFlags(&D.h2d, hipStreamNonBlocking));
  SV_HIP(hipStreamCreateWithFlags(&D.d2h, hipStreamNonBlocking));
  SV_HIP(hipEventCreateWithFlags(&D.dep_in, hipEventDisableTiming));
  SV_HIP(hipEventCreateWithFlags(&D.dep_out, hipEventDisableTiming));
  D.z_in.mapped = D.z_out.mapped = true;
  for (Stage& s : D.st) {
    SV_HIP(hipEventCreateWithFlags(&s.up, hipEventDisableTiming));
    SV_HIP(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    SV_HIP(hipEventCreateWithFlags(&s.down, hipEventDisableTiming));
    SV_HIP(hipEventCreateWithFlags(&s.keys_down, hipEventDisableTiming));
  }
  SV_HIP(hipMalloc(&D.btab, sv_btab_bytes()));
  SV_HIP(sv_launch_btab_init((uint32_t*)D.btab, D.stream));
  D.grid = (unsigned)(D.cus * sv_occupancy_blocks_per_cu());
  D.grid_share = (unsigned)(D.cus * std::max(1, sv_share_blocks_per_cu()));
  SV_HIP(hipStreamSynchronize(D.stream));
  return SV_OK;
}

inline void release_device(Device& D) {
  if (!D.ready) return;
  (void)hipSetDevice(D.phys);
  (void)hipStreamSynchronize(D.stream);
  (void)hipStreamSynchronize(D.h2d);
  (void)hipStreamSynchronize(D.d2h);
  D.timer.release();
  D.z_in.release();
  D.z_out.release();
  for (Stage& s : D.st) {
    s.h_in.release(); s.h_out.release();
    s.d_in.release(); s.d_verdict.release(); s.d_keys.release();
    s.d_pair.release(); s.h_cnt.release(); s.d_acct.release();
    if (s.up) (void)hipEventDestroy(s.up);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.down) (void)hipEventDestroy(s.down);
    if (s.keys_down) (void)hipEventDestroy(s.keys_down);
    for (hipEvent_t e : s.pev) (void)hipEventDestroy(e);
    s.pev.clear();
    s.up = s.done = s.down = s.keys_down = nullptr;
  }
  D.msg.release(); D.off.release(); D.len.release(); D.keys.release(); D.h_sha.release();
  D.txmsg.release();
  D.txpk.release(); D.txsg.release(); D.txpair.release(); D.h_txcnt.release(); D.txchk.release(); D.txpp.release();
  D.txatab.release(); D.txaws.release(); D.txarows.release(); D.txres.release();
  D.sign_rec.release(); D.sign_seed.release(); D.sign_in.release(); D.sign_out.release();
  if (D.sign_ctab) (void)hipFree(D.sign_ctab);
  D.sign_ctab = nullptr;
  D.ws.release();
  D.kt.index.release(); D.kt.store.release(); D.kt.kslot.release(); D.kt.builders.release();
  D.kt.count.release(); D.kt.h_count.release();
  if (D.kt.copied) (void)hipEventDestroy(D.kt.copied);
  D.kt.copied = nullptr;
  D.kt.slots = 0;
  D.vc.release();
  share_release(D);
  D.as.release();
  D.audit.release();
  if (D.btab) (void)hipFree(D.btab);
  if (D.dep_in) (void)hipEventDestroy(D.dep_in);
  if (D.dep_out) (void)hipEventDestroy(D.dep_out);
  if (D.stream) (void)hipStreamDestroy(D.stream);
  if (D.h2d) (void)hipStreamDestroy(D.h2d);
  if (D.d2h) (void)hipStreamDestroy(D.d2h);
  D.btab = nullptr;
  D.stream = D.h2d = D.d2h = nullptr;
  D.ready = false;
}

// A latency-lane launch while the audit is on: counted, not audited.
inline void audit_lane_count(Device& D) {
  if (audit_what()) D.audit.lane_launches.fetch_add(1, std::memory_order_relaxed);
}

// Caller holds D.mu.
inline int ready_locked(Device& D) {
  if (D.ready) return SV_OK;
  int rc = init_device(D);
  if (rc == SV_OK) D.ready = true;
  return rc;
}

// Workspace for a launch (caller holds D.mu, device set).  Growing it frees
// the old one, so the kernel stream is drained first.
inline int ensure_ws(Device& D, size_t bytes) {
  if (bytes <= D.ws.cap) return SV_OK;
  SV_HIP(hipStreamSynchronize(D.stream));
  return D.ws.ensure(bytes);
}

}  // namespace
}  // namespace sv
