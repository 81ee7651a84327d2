// Bulk work of a device slot, on its three streams under Device::mu: the
// throughput-path launch with its per-key tables, the staged host-buffer
// pipeline (host_slice), its kernel-less probe (feed_slice), SHA-256 batches
// (sha_slice), tx-body batches (tx_slice) and hinted tx-body batches, paired
// by hint on the device (hinted_slice).  Included by sv_api.cpp.
//
// The pairs of the hinted, check and decide forms are verified behind the
// slot's verdict cache (launch_cached_locked; off by default).  While it is on,
// every verify launch of those forms waits once more on the kernel stream, for
// its miss count: in the host-buffer chunk loops that is one more wait per
// chunk (two where the chunk has payload pairs), behind the one for its pair
// count, and it also waits out the previous chunk's verify launch.
//
// sv_set_verdict_cache_feed (off by default): what the slot's latency lane journaled (vjournal.h) is drained into
// the table ahead of every cached launch's probe (vc_drain_locked), and with SV_VC_FEED_BULK the keyed chunks of
// host_slice_locked go behind the cache too.
//
// sv_set_verdict_cache_share (off by default; vshare.h): with SV_VC_SHARE_STORES and more than one slot a cached
// launch exports its misses behind its insert (vc_export_locked) and passes on, ahead of its drain, whatever any
// slot's exports have completed (engine_state.h share_pass_all); a host-buffer slice passes its own on before it
// returns (with_slot).
#pragma once

#include <chrono>
#include <cstdio>
#include <functional>
#include <random>
#include <thread>

#include "engine_state.h"
#include "host_image.h"
#include "txacct.h"
#include "txresult.h"
#include "vcache.h"

namespace sv {
namespace {

// Shared mode of the throughput kernels (sv_kernels.hip sv_launch_verify):
// taken by every bulk launch within SV_LAT_SHARE_MS (default 1000) ms of a
// latency-lane batch on the same slot, so SCP-class batches find free
// workgroup slots while a tx set or catchup batch runs.  0 disables it.
inline int64_t share_window_ns() {
  static const int64_t w = (int64_t)env_size("SV_LAT_SHARE_MS", 1000) * 1000000;
  return w;
}
inline size_t share_upload_bytes() {
  static const size_t b = std::max<size_t>(64, env_size("SV_SHARE_UPLOAD_KB", 2048)) * 1024;
  return b;
}
// One-chunk host batches (n <= SV_STAGE_CHUNK) read in place
// (SV_BULK_ZC_IN, default on; 0: one staged H2D copy): the kernels read the
// packed image from mapped pinned memory, so the copy no longer runs before
// the first kernel (a multi-chunk batch overlaps its copies with the previous
// chunk's kernels and stays staged).
inline bool bulk_in_place() {
  static const bool b = env_size("SV_BULK_ZC_IN", 1) != 0;
  return b;
}
// ... and their verdicts are written in place too (SV_BULK_ZC_OUT, default on):
// the kernels store them to mapped memory, so no copy is queued behind them.
inline bool bulk_zc_out() {
  static const bool b = env_size("SV_BULK_ZC_OUT", 1) != 0;
  return b;
}
// One-chunk throughput launches read in place run the prep kernel in its
// decode-first order (sv_kernels.hip sv_prep_kernel DF; SV_DECODE_FIRST=0: the
// device path's order)
inline bool decode_first() {
  static const bool b = env_size("SV_DECODE_FIRST", 1) != 0;
  return b;
}
inline bool share_now(const Device& D) {
  const int64_t w = share_window_ns();
  return w > 0 && now_ns() - D.lat_last_ns.load(std::memory_order_relaxed) < w;
}

inline int audit_strict_locked(Device& D);  // (the verdict audit, below: SV_OK at once unless SV_AUDIT_STRICT is set)

// Runs fn() on the slot: D.mu held, the device set, the slot's resources
// created.  A failing call leaves the slot reusable: nothing of it may still
// be in flight.  Every host-buffer slice of the bulk route runs here, so this
// is where a strict audit answers for the slice's verdicts.
template <class F>
int with_slot(Device& D, F fn) {
  std::lock_guard<std::mutex> g(D.mu);
  SV_HIP(hipSetDevice(D.phys));
  int rc;
  if ((rc = ready_locked(D))) return rc;
  if ((rc = fn()) == SV_OK) rc = audit_strict_locked(D);
  if (rc != SV_OK) {
    (void)hipStreamSynchronize(D.h2d);
    (void)hipStreamSynchronize(D.stream);
    (void)hipStreamSynchronize(D.d2h);
    D.st[0].busy = D.st[1].busy = false;
  }
  // (sv_set_verdict_cache_share: a host-buffer slice passes its own exports on before it returns -- a wait for
  // its own stream's events, which the slice's results have as a rule waited out already)
  if (share_stores()) share_pass(D, true);
  return rc;
}

inline unsigned grid_for(const Device& D, uint64_t n, bool share = false) {
  const uint64_t need = (n + sv_block_threads() - 1) / sv_block_threads();
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(share ? D.grid_share : D.grid, need));
}

// ---------------------------------------------------- per-key tables
// sv_set_key_tables: 0 off, 1 on for every throughput-path launch, 2 (auto,
// the default) on for host-buffer batches whose keys repeat (repeated_keys);
// -1: SV_KEY_TABLES.  Slots: SV_KEY_TABLE_SLOTS (default 2^19; claims stop at
// half of them, when the claim words are cleared).
inline std::atomic<int> g_kt_mode{-1};
inline std::atomic<size_t> g_kt_slots{0};
inline int kt_mode() {
  const int v = g_kt_mode.load();
  if (v >= 0) return v;
  return (int)std::min<size_t>(2, env_size("SV_KEY_TABLES", 2));
}
inline size_t kt_slots() {
  size_t v = g_kt_slots.load();
  if (v == 0) v = env_size("SV_KEY_TABLE_SLOTS", (size_t)1 << 19);
  size_t p = 1024;
  while (p < v && p < ((size_t)1 << 26)) p <<= 1;
  return p;
}

// Readies the slot's key tables for a launch of n (caller holds D.mu, device
// set) and fills *kt; false: tables unavailable (allocation failed), the
// launch runs without them.
inline bool kt_prepare(Device& D, uint64_t n, sv_ktparams* kt) {
  KeyTabs& T = D.kt;
  const size_t want = kt_slots();
  if (T.slots != want) {
    (void)hipStreamSynchronize(D.stream);
    T.index.release();
    T.store.release();
    T.slots = 0;
    if (T.index.ensure(want * 8) || T.store.ensure(want * sv_key_table_entry_bytes()) || T.count.ensure(16) ||
        T.h_count.ensure(16))
      return false;
    if (!T.copied && hipEventCreateWithFlags(&T.copied, hipEventDisableTiming) != hipSuccess) return false;
    if (hipMemsetAsync(T.index.p, 0, want * 8, D.stream) != hipSuccess ||
        hipMemsetAsync(T.count.p, 0, 16, D.stream) != hipSuccess)
      return false;
    std::memset(T.h_count.p, 0, 16);
    T.salt = ((uint64_t)std::random_device{}() << 32) ^ std::random_device{}() ^ (uint64_t)now_ns();
    T.slots = want;
  }
  const uint64_t cap = sv_plan_chunk_max(n);
  if (cap * 4 > T.kslot.cap || cap * 4 > T.builders.cap) {
    (void)hipStreamSynchronize(D.stream);  // (the lists of a running launch)
    if (T.kslot.ensure(cap * 4) || T.builders.ensure(cap * 4)) return false;
  }
  // the claims as of the last launch whose counters have come back
  const uint32_t limit = (uint32_t)(want / 2);
  if (hipEventQuery(T.copied) == hipSuccess) {
    T.claims = ((const uint32_t*)T.h_count.p)[1];
    if (T.claims >= limit) {
      if (hipMemsetAsync(T.index.p, 0, want * 8, D.stream) != hipSuccess ||
          hipMemsetAsync(T.count.p, 0, 16, D.stream) != hipSuccess)
        return false;
      std::memset(T.h_count.p, 0, 16);
      T.claims = 0;
      ++T.clears;
    }
  }
  kt->index = (unsigned long long*)T.index.p;
  kt->store = (sv_u4*)T.store.p;
  kt->kslot = (uint32_t*)T.kslot.p;
  kt->builders = (uint32_t*)T.builders.p;
  kt->count = (uint32_t*)T.count.p;
  kt->mask = want - 1;
  kt->limit = limit;
  kt->salt = T.salt;
  return true;
}

inline size_t audit_ws_need(Device& D, uint64_t n);  // (the verdict audit, below: 0 with the audit off)

// Launch on D.stream (caller holds D.mu and has set the device).  tables:
// the launch may use the per-key tables (kt_mode / repeated_keys).
// kp: SV_KP_* launch hints (SV_KP_IN_PLACE: the inputs are mapped host memory)
inline int launch_locked(Device& D, int mode, int path, const void* pk, const void* sig, const void* msg,
                         const uint64_t* off, const uint32_t* len, uint32_t fixed_len, uint64_t n, void* verdict,
                         void* bitmap, bool tables = false, uint32_t kp = 0) {
  const int rp = resolve_path(path, n);
  const bool share = rp != SV_PATH_LATENCY && share_now(D);
  const unsigned grid = grid_for(D, n, share);
  int rc;
  sv_ktparams ktp{};
  const int geom = launch_geometry(rp, n);
  const bool kt_on = tables && geom == SV_PATH_THROUGHPUT && kt_prepare(D, n, &ktp);
  // (with the audit on, room for its tables too: the pass behind this launch then never grows the workspace)
  if ((rc = ensure_ws(D, std::max(sv_verify_ws_bytes(geom, grid, n), audit_ws_need(D, n))))) return rc;
  if ((rc = D.timer.begin(D.stream))) return rc;
  SV_HIP(sv_launch_verify(mode, geom, grid, pk, sig, msg, off, len, fixed_len, n, verdict, bitmap, D.ws.p, D.btab,
                          (g_dbg.load() & kKernelDbgMask) | (kt_on ? 0u : kp), share ? 1 : 0, kt_on ? &ktp : nullptr,
                          nullptr, D.stream));
  if (share) D.shared_launches.fetch_add(1, std::memory_order_relaxed);
  if (kt_on) {
    ++D.kt.launches;
    SV_HIP(hipMemcpyAsync(D.kt.h_count.p, D.kt.count.p, 8, hipMemcpyDeviceToHost, D.stream));
    SV_HIP(hipEventRecord(D.kt.copied, D.stream));
  }
  return D.timer.end(D.stream, n);
}

// ---------------------------------------------------- verdict audit
// (the setting: engine_state.h audit_what, audit_cfg; the rules: audit.h)

// Workgroups of the audit's verify kernel over a launch of n with `budget`, and the slot workspace they need
// (one table of -A per lane, in D.ws behind the verify kernels that used it).
inline unsigned audit_grid(Device& D, uint64_t n, uint64_t budget) {
  Audit& A = D.audit;
  if (!A.blocks_per_cu) A.blocks_per_cu = sv_audit_blocks_per_cu();
  return sv_audit_grid(n, budget, (unsigned)(D.cus * A.blocks_per_cu));
}
// What the audit of a launch of n adds to the launch's workspace need: 0 with the audit off.
inline size_t audit_ws_need(Device& D, uint64_t n) {
  if (!audit_what() || !n) return 0;
  return sv_audit_ws_bytes(audit_grid(D, n, sv_audit_budget(audit_cfg().budget)));
}

// One audit pass over n claimed verdict bytes, on D.stream (caller holds D.mu, device set): select, scan, fill,
// verify, report (sv_audit.hip).  Nothing is waited for, except where a buffer has to grow: then the kernel stream
// is drained first, as everywhere (a launch sized by presize_ws / launch_locked never grows D.ws here).
inline int audit_pass_locked(Device& D, const AuditCfg& cfg, uint64_t seq, const void* pk, const void* sig,
                             const void* msg, const uint64_t* off, const uint32_t* len, uint32_t fixed_len,
                             uint64_t n, const void* verdict) {
  if (n > SV_AUDIT_MAX_ROWS) return fail(SV_ERR_INVALID_ARG, "audit: more than 2^32 - 1 rows");
  Audit& A = D.audit;
  int rc;
  if (!A.state.p) {
    if ((rc = A.state.ensure(Audit::kStateBytes)) || (rc = A.h_rd.ensure(Audit::kStateBytes))) return rc;
    SV_HIP(hipMemsetAsync(A.state.p, 0, Audit::kStateBytes, D.stream));
  }
  const uint64_t budget = sv_audit_budget(cfg.budget);
  const uint64_t cap = sv_audit_clip(n, budget);
  const size_t o_list = sv_audit_psum_bytes(n), o_av = o_list + al16(4 * cap), bytes = o_av + al16(cap);
  if (bytes > A.buf.cap) {
    SV_HIP(hipStreamSynchronize(D.stream));  // (a running pass reads the old one)
    if ((rc = A.buf.ensure(bytes))) return rc;
  }
  sv_audit_args a;
  a.grid = audit_grid(D, n, budget);
  if ((rc = ensure_ws(D, sv_audit_ws_bytes(a.grid)))) return rc;
  uint8_t* b = (uint8_t*)A.buf.p;
  a.pk = pk;
  a.sig = sig;
  a.msg = msg;
  a.off = off;
  a.len = len;
  a.fixed_len = fixed_len;
  a.what = cfg.what;
  a.one_in = cfg.one_in;
  a.dissent = (g_dbg.load() & SV_DBG_AUDIT_DISSENT) ? 1u : 0u;
  a.seed = cfg.seed;
  a.seq = seq;
  a.n = n;
  a.budget = budget;
  a.verdict = (const uint8_t*)verdict;
  a.psum = (uint64_t*)b;
  a.list = (uint32_t*)(b + o_list);
  a.av = b + o_av;
  a.counters = (uint64_t*)A.state.p;
  a.ring = (sv_audit_record*)((uint8_t*)A.state.p + Audit::kRingOff);
  a.ws = D.ws.p;
  a.btab = D.btab;
  if ((rc = A.timer.begin(D.stream))) return rc;
  SV_HIP(sv_launch_audit(&a, D.stream));
  return A.timer.end(D.stream, cap);
}

// The hook behind a bulk-route verify launch: its n verdict bytes, audited under the process-wide setting as the
// slot's next audited launch.  With the audit off -- the default -- one atomic load and nothing else.  Under
// SV_DBG_PREP_ONLY there are no verdicts, so there is no audit.
inline int audit_locked(Device& D, const void* pk, const void* sig, const void* msg, const uint64_t* off,
                        const uint32_t* len, uint32_t fixed_len, uint64_t n, const void* verdict) {
  if (!audit_what() || n == 0 || (g_dbg.load() & SV_DBG_PREP_ONLY)) return SV_OK;
  const AuditCfg cfg = audit_cfg();
  if (!cfg.what) return SV_OK;
  return audit_pass_locked(D, cfg, D.audit.seq++, pk, sig, msg, off, len, fixed_len, n, verdict);
}

// The slot's `mismatches` now (waits for D.stream; caller holds D.mu, device set); 0 before the first pass.
inline int audit_mismatches_locked(Device& D, uint64_t* out) {
  Audit& A = D.audit;
  *out = 0;
  if (!A.state.p) return SV_OK;
  SV_HIP(hipMemcpyAsync(A.h_rd.p, (const uint64_t*)A.state.p + SV_AC_MISMATCH, 8, hipMemcpyDeviceToHost, D.stream));
  SV_HIP(hipStreamSynchronize(D.stream));
  *out = *(const uint64_t*)A.h_rd.p;
  return SV_OK;
}
// SV_AUDIT_STRICT, at the end of a host-buffer slice that returned SV_OK (its last wait is behind it): SV_ERR_AUDIT
// if the slot's `mismatches` moved since they were last read -- during this slice, or during a device-resident
// call before it, whose mismatches no host call has answered for yet.
inline int audit_strict_locked(Device& D) {
  if (!(audit_what() & SV_AUDIT_STRICT)) return SV_OK;
  Audit& A = D.audit;
  uint64_t now;
  int rc;
  if ((rc = audit_mismatches_locked(D, &now))) return rc;
  const uint64_t before = A.seen;
  A.seen = now;
  if (now != before) return fail(SV_ERR_AUDIT, "audit: the textbook verifier disagrees with a verdict of this call");
  return SV_OK;
}

// launch_locked with the audit behind it: a caller-visible verdict array of the bulk route.
inline int launch_audited_locked(Device& D, int mode, int path, const void* pk, const void* sig, const void* msg,
                                 const uint64_t* off, const uint32_t* len, uint32_t fixed_len, uint64_t n,
                                 void* verdict, void* bitmap, bool tables = false, uint32_t kp = 0) {
  int rc;
  if ((rc = launch_locked(D, mode, path, pk, sig, msg, off, len, fixed_len, n, verdict, bitmap, tables, kp)))
    return rc;
  return audit_locked(D, pk, sig, msg, off, len, fixed_len, n, verdict);
}

// The workspace of the largest launch of a call (m signatures on `path`)
// before its first launch, so it never grows under a running kernel.
inline int presize_ws(Device& D, int path, size_t m) {
  const int rp = resolve_path(path, m);
  return ensure_ws(D, std::max({sv_verify_ws_bytes(rp, grid_for(D, m), m),
                                sv_verify_ws_bytes(launch_geometry(rp, m), grid_for(D, m), m), audit_ws_need(D, m)}));
}

// ---------------------------------------------------- verdict cache
// (the capacity and feed settings: engine_state.h vc_entries, vc_feed)

// An empty table: all-zero entries, every claim word SV_VC_UNCLAIMED (on D.stream; the counters stay).
inline int vc_clear_locked(Device& D) {
  VerdictCache& C = D.vc;
  if (!C.entries) return SV_OK;
  SV_HIP(hipMemsetAsync(C.tab.p, 0, C.entries * sizeof(sv_vc_entry), D.stream));
  SV_HIP(hipMemsetAsync(C.claim.p, 0xFF, C.entries * 4, D.stream));
  return SV_OK;
}
// The slot's table at the capacity in force (caller holds D.mu, device set): a changed capacity drains the kernel
// stream, frees the old table with its workspace and counters, and allocates an empty one.
inline int vc_prepare(Device& D) {
  VerdictCache& C = D.vc;
  const size_t want = vc_entries();
  if (C.entries == want) return SV_OK;
  SV_HIP(hipStreamSynchronize(D.stream));
  C.release();
  if (!want) return SV_OK;
  int rc;
  if ((rc = C.tab.ensure(want * sizeof(sv_vc_entry))) || (rc = C.claim.ensure(want * 4)) ||
      (rc = C.counters.ensure(64)) || (rc = C.h_cnt.ensure(128))) {
    C.release();
    return rc;
  }
  C.entries = want;
  if ((rc = vc_clear_locked(D)) || hipMemsetAsync(C.counters.p, 0, 64, D.stream) != hipSuccess) {
    C.release();
    return rc ? rc : fail(SV_ERR_HIP, "verdict cache: clearing the counters");
  }
  return SV_OK;
}

// The compaction workspace of a cached launch of n in C.ws: keys (32 n, unless the caller has an array for
// them) | miss list | candidate slots (4 n each) | block sums | missed bytes | compacted verdicts (n each) |
// compacted keys (32 n) | signatures (64 n) | messages (32 n; fixed 32-byte messages) or offsets (8 n) and
// lengths (4 n), every section 16-byte aligned.
struct VcBufs {
  size_t o_keys, o_miss, o_slot, o_psum, o_missed, o_cv, o_pk, o_sig, o_msg, o_len, bytes;
  size_t o_exp;  // the export image (33 rows; vshare.h), only while the slots share what they verified
};
inline VcBufs vc_layout(size_t n, bool own_keys, bool fixed32, size_t exp_rows = 0) {
  VcBufs b;
  b.o_exp = 0;
  b.o_keys = 0;
  b.o_miss = own_keys ? 32 * n : 0;
  b.o_slot = b.o_miss + al16(4 * n);
  b.o_psum = b.o_slot + al16(4 * n);
  b.o_missed = b.o_psum + al16(sv_vc_psum_bytes(n));
  b.o_cv = b.o_missed + al16(n);
  b.o_pk = b.o_cv + al16(n);
  b.o_sig = b.o_pk + 32 * n;
  b.o_msg = b.o_sig + 64 * n;
  b.o_len = b.o_msg + (fixed32 ? 32 * n : al16(8 * n));
  b.bytes = b.o_len + (fixed32 ? 0 : al16(4 * n)) + 16;
  if (exp_rows) {  // (behind everything else: with no export the layout is what it always was)
    b.o_exp = al16(b.bytes);
    b.bytes = b.o_exp + al16(share_image_bytes(exp_rows));
  }
  return b;
}

// The slot's journal (vjournal.h) into its table, on D.stream (caller holds D.mu, device set): the held rows are
// taken, copied into the pinned h_feed and from there into the head of C.ws -- keys (32 n) | verdict bytes |
// candidate slots (4 n) -- and the two feed kernels run over them (vcache.h Feed).  An empty journal, or the cache
// off, enqueues nothing.  Nothing is waited for but the previous drain's upload out of h_feed (and, where C.ws
// grows, the kernel stream); work queued on D.stream behind the drain sees the rows in the table.
inline int vc_drain_locked(Device& D) {
  if (!vc_entries() || !D.vj.held()) return SV_OK;
  VerdictCache& C = D.vc;
  int rc;
  if ((rc = vc_prepare(D))) return rc;
  if (!C.fed_up) SV_HIP(hipEventCreateWithFlags(&C.fed_up, hipEventDisableTiming));
  D.vj.take(C.taken);
  const size_t n = C.taken.rows;
  if (!n) return SV_OK;
  const size_t o_v = 32 * n, o_slot = o_v + al16(n), bytes = o_slot + al16(4 * n);
  if (bytes > C.ws.cap) {
    SV_HIP(hipStreamSynchronize(D.stream));  // (a running pass reads the old one)
    if ((rc = C.ws.ensure(bytes))) return rc;
  }
  SV_HIP(hipEventSynchronize(C.fed_up));  // (never recorded: success at once)
  if ((rc = C.h_feed.ensure(o_v + n))) return rc;
  uint8_t* h = (uint8_t*)C.h_feed.p;
  std::memcpy(h, C.taken.keys.data(), 32 * n);
  std::memcpy(h + o_v, C.taken.verdicts.data(), n);
  uint8_t* w = (uint8_t*)C.ws.p;
  SV_HIP(hipMemcpyAsync(w, h, o_v + n, hipMemcpyHostToDevice, D.stream));
  SV_HIP(hipEventRecord(C.fed_up, D.stream));
  sv_vc_feed_args A;
  A.tab = (sv_vc_entry*)C.tab.p;
  A.claim = (uint32_t*)C.claim.p;
  A.sets = C.entries / SV_VC_WAYS;
  A.counters = (uint64_t*)C.counters.p + 4;
  A.keys = (const uint32_t*)w;
  A.verdict = w + o_v;
  A.slot = (uint32_t*)(w + o_slot);
  A.n = n;
  if ((rc = C.timer.begin(D.stream))) return rc;
  SV_HIP(sv_launch_vc_feed(&A, D.stream));
  return C.timer.end(D.stream, 0);
}

// The export of a cached launch behind its insert (vshare.h; caller holds D.mu, device set): the leading
// min(nm, cap) rows of the pass's miss list -- stored or dropped here alike, the peer applies its own policy --
// gathered into d_image (33 rows bytes of C.ws), copied to a pinned buffer of the slot's queue and queued with
// an event behind the copy, all on D.stream.  Nothing is waited for: with every buffer pending the launch skips
// its export and counts the rows (shared_skipped), as it counts the rows beyond `cap`.  Whoever finds the event
// complete passes the rows on (share_pass).  An export that fails leaves nothing queued, counts its rows as skipped
// and does not fail the call.
inline int vc_export_locked(Device& D, const sv_vc_args& A, uint64_t nm, size_t cap, uint8_t* d_image) {
  const size_t rows = share_offer(nm, cap);
  const int b = D.shq.reserve(nm, rows);
  if (b < 0) return SV_OK;
  VerdictCache& C = D.vc;
  int rc = share_buf_ensure(D, b, rows, cap);
  hipError_t e = hipSuccess;
  bool queued = false;
  if (rc == SV_OK && (rc = C.timer.begin(D.stream)) == SV_OK) {
    e = sv_launch_vc_export(&A, nm, rows, d_image, D.stream);
    queued = true;
    if (e == hipSuccess) rc = C.timer.end(D.stream, 0);
    if (e == hipSuccess && rc == SV_OK)
      e = hipMemcpyAsync(D.shb[b].p, d_image, share_image_bytes(rows), hipMemcpyDeviceToHost, D.stream);
    if (e == hipSuccess && rc == SV_OK) e = hipEventRecord(D.shb[b].ev, D.stream);
  }
  if (e != hipSuccess || rc != SV_OK) {
    // An export that cannot be made -- no pinned memory, say -- is no failure of the call: its verdicts, insert and
    // bitmap are queued and valid, and only the amount of work may depend on the setting.  The rows are skipped.
    if (queued) (void)hipStreamSynchronize(D.stream);  // (a copy that did start no longer writes the buffer)
    D.shq.cancel(b, rows);
    return SV_OK;
  }
  D.shq.commit(b, (const uint8_t*)D.shb[b].p, rows);
  return SV_OK;
}

// launch_locked behind the slot's verdict cache (vcache.h): the same arguments, the same verdict bytes and
// bitmap.  With the cache off -- the default -- or under SV_DBG_PREP_ONLY (no verdicts exist, so nothing may be
// inserted) it IS launch_locked: no allocation, no kernel and no wait of its own.  With it on, all on D.stream:
// cache keys -> probe -> scan, fill, gather -> the miss count back in an 8-byte copy and ONE WAIT on D.stream
// (as tx_counted's callers wait for the pair count) -> launch_locked over the compacted misses, skipped when
// there are none -> scatter and claim -> store -> bitmap.  Always the bulk route: the latency lane neither reads
// nor writes the table.  Nothing before the claim kernel writes the table or its claim words, so an error return
// up to there leaves the cache as it was.  hit (optional): n bytes, 1 where the verdict came from the table (all 0
// with the cache off); keys (optional, 16-byte aligned): n x 32, the cache keys (written with the cache off too;
// keys_done: the caller's hash launch, queued on D.stream, has written them already).  With the cache on the
// slot's journal is drained first (vc_drain_locked), so the probe sees what the latency lane verified.
inline int launch_cached_locked(Device& D, int mode, int path, const void* pk, const void* sig, const void* msg,
                                const uint64_t* off, const uint32_t* len, uint32_t fixed_len, uint64_t n,
                                void* verdict, void* bitmap, bool tables = false, uint32_t kp = 0,
                                void* hit = nullptr, void* keys = nullptr, bool keys_done = false) {
  int rc;
  if (!vc_entries() || (g_dbg.load() & SV_DBG_PREP_ONLY) || n == 0 || n > SV_VC_MAX_ITEMS) {
    if (hit && n) SV_HIP(hipMemsetAsync(hit, 0, n, D.stream));
    if (keys && n && !keys_done) SV_HIP(sv_launch_hash(0, D.grid * 2, pk, sig, msg, off, len, fixed_len, n, keys, D.stream));
    return launch_audited_locked(D, mode, path, pk, sig, msg, off, len, fixed_len, n, verdict, bitmap, tables, kp);
  }
  VerdictCache& C = D.vc;
  if ((rc = vc_prepare(D))) return rc;
  // (sv_set_verdict_cache_share: what the other slots' launches exported and is complete goes into the journals
  // first -- this slot's among them -- without a wait; then the drain)
  const bool share = share_stores();
  if (share) share_pass_all(false);
  if ((rc = vc_drain_locked(D))) return rc;
  const bool f32 = fixed_len == 32;
  const size_t share_cap = share ? vc_journal_rows() : 0;
  const VcBufs L = vc_layout(n, !keys, f32, share_offer(n, share_cap));
  if (L.bytes > C.ws.cap) {
    SV_HIP(hipStreamSynchronize(D.stream));  // (a running pass reads the old one)
    if ((rc = C.ws.ensure(L.bytes))) return rc;
  }
  uint8_t* w = (uint8_t*)C.ws.p;
  sv_vc_args A;
  A.tab = (sv_vc_entry*)C.tab.p;
  A.claim = (uint32_t*)C.claim.p;
  A.sets = C.entries / SV_VC_WAYS;
  A.counters = (uint64_t*)C.counters.p;
  A.pk = pk;
  A.sig = sig;
  A.msg = msg;
  A.off = off;
  A.len = len;
  A.fixed_len = fixed_len;
  A.n = n;
  A.keys = (const uint32_t*)(keys ? keys : w + L.o_keys);
  A.verdict = (uint8_t*)verdict;
  A.hit = (uint8_t*)hit;
  A.missed = w + L.o_missed;
  A.psum = (uint64_t*)(w + L.o_psum);
  A.miss = (uint32_t*)(w + L.o_miss);
  A.slot = (uint32_t*)(w + L.o_slot);
  A.cpk = w + L.o_pk;
  A.csig = w + L.o_sig;
  A.cmsg = f32 ? w + L.o_msg : nullptr;
  A.coff = f32 ? nullptr : (uint64_t*)(w + L.o_msg);
  A.clen = f32 ? nullptr : (uint32_t*)(w + L.o_len);
  A.cverdict = w + L.o_cv;
  if ((rc = C.timer.begin(D.stream))) return rc;
  if (!(keys && keys_done))
    SV_HIP(sv_launch_hash(0, D.grid * 2, pk, sig, msg, off, len, fixed_len, n, (void*)A.keys, D.stream));
  SV_HIP(sv_launch_vc_probe(&A, D.stream));
  if ((rc = C.timer.end(D.stream, n))) return rc;
  SV_HIP(hipMemcpyAsync(C.h_cnt.p, A.counters + 3, 8, hipMemcpyDeviceToHost, D.stream));
  // the one wait: how many items the verify launch has is only known on the device
  const auto t0 = std::chrono::steady_clock::now();
  SV_HIP(hipStreamSynchronize(D.stream));
  C.wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  C.lookups += n;
  const uint64_t nm = *(const uint64_t*)C.h_cnt.p;
  if (nm > n) return fail(SV_ERR_HIP, "verdict cache: miss count beyond the batch");
  // (the compacted arrays are device memory: the in-place hints of kp do not apply to them)
  if (nm && (rc = launch_locked(D, f32 ? 0 : 1, path, A.cpk, A.csig, f32 ? (const void*)A.cmsg : msg, A.coff, A.clen,
                                f32 ? 32 : 0, nm, A.cverdict, nullptr, tables, 0)))
    return rc;
  if (nm || bitmap) {
    if ((rc = C.timer.begin(D.stream))) return rc;
    SV_HIP(sv_launch_vc_insert(&A, nm, D.stream));
    if (bitmap) SV_HIP(sv_launch_vc_bitmap(verdict, n, bitmap, D.stream));
    if ((rc = C.timer.end(D.stream, 0))) return rc;
  }
  if (nm && share && (rc = vc_export_locked(D, A, nm, share_cap, w + L.o_exp))) return rc;
  // all n rows against the caller's inputs, the hits among them (the launch over the misses was not audited)
  return audit_locked(D, pk, sig, msg, off, len, fixed_len, n, verdict);
}

// H2D of a whole packed image.  While latency-lane batches are live (shared
// mode) it goes up in pieces of SV_SHARE_UPLOAD_KB (default 2048): a 1k
// batch's 370 KB copy otherwise queues behind the whole 32 MB chunk copy
// (~0.65 ms, once per chunk: profiles/r04/isolation/).
inline int upload_image(const Device& D, void* d, const void* h, size_t bytes, hipStream_t st) {
  const size_t piece = share_now(D) ? share_upload_bytes() : bytes;
  for (size_t o = 0; o < bytes; o += piece)
    SV_HIP(hipMemcpyAsync((uint8_t*)d + o, (const uint8_t*)h + o, std::min(piece, bytes - o), hipMemcpyHostToDevice,
                          st));
  return SV_OK;
}
// H2D of rows [a, b) of a packed image (each section's slice); msg_total: the
// image's message bytes.
inline int upload_rows(const Image& im, size_t m, size_t a, size_t b, uint32_t fixed, size_t msg_total,
                       const uint8_t* h, uint8_t* d, hipStream_t st) {
  SV_HIP(hipMemcpyAsync(d + 32 * a, h + 32 * a, 32 * (b - a), hipMemcpyHostToDevice, st));
  SV_HIP(hipMemcpyAsync(d + im.o_sig + 64 * a, h + im.o_sig + 64 * a, 64 * (b - a), hipMemcpyHostToDevice, st));
  size_t m0, m1;
  if (im.var) {
    SV_HIP(hipMemcpyAsync(d + im.o_off + 8 * a, h + im.o_off + 8 * a, 8 * (b - a), hipMemcpyHostToDevice, st));
    SV_HIP(hipMemcpyAsync(d + im.o_len + 4 * a, h + im.o_len + 4 * a, 4 * (b - a), hipMemcpyHostToDevice, st));
    const uint64_t* offs = (const uint64_t*)(h + im.o_off);
    m0 = offs[a];
    m1 = b < m ? offs[b] : msg_total;
  } else {
    m0 = a * (size_t)fixed;
    m1 = b * (size_t)fixed;
  }
  if (m1 > m0) SV_HIP(hipMemcpyAsync(d + im.o_msg + m0, h + im.o_msg + m0, m1 - m0, hipMemcpyHostToDevice, st));
  return SV_OK;
}

// Collects a finished chunk's results from its pinned slot.
inline int drain_stage(Stage& s, uint8_t* verdict, uint8_t* keys) {
  if (!s.busy) return SV_OK;
  SV_HIP(hipEventSynchronize(s.down));
  if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE down synced @%.1f\n", trace_abs_us());
  s.busy = false;
  const uint8_t* h = (const uint8_t*)s.h_out.p;
  if (verdict) std::memcpy(verdict + s.lo, s.zv ? s.zv : h, s.m);
  if (keys) std::memcpy(keys + 32 * s.lo, h + (verdict ? s.m : 0), 32 * s.m);
  return SV_OK;
}

inline thread_local std::chrono::steady_clock::time_point g_trace_t0;  // (SV_STAGE_TRACE: host_slice entry)

// Runs fn(0), fn(1), ... fn(P - 1) on a thread of its own, fn(k) once piece
// k's events have been recorded (recorded(k + 1)); join() returns the first
// error.  The destructor stops and joins it (an early error return of the
// caller).
class KeyNotifier {
 public:
  ~KeyNotifier() {
    stop_.store(true);
    if (th_.joinable()) th_.join();
  }
  void start(int dev, size_t P, std::function<int(size_t)> fn) {
    fn_ = std::move(fn);
    th_ = std::thread([this, dev, P] {
      // (the caller holds the lifetime lock until this thread is joined)
      t_life_depth = 1;
      (void)hipSetDevice(dev);
      for (size_t k = 0; k < P; ++k) {
        while (rec_.load(std::memory_order_acquire) <= k) {
          if (stop_.load()) return;
          std::this_thread::yield();
        }
        const int rc = fn_(k);
        if (rc != SV_OK) {
          rc_ = rc;
          return;
        }
      }
    });
  }
  void recorded(size_t k) { rec_.store(k, std::memory_order_release); }
  int join() {
    if (th_.joinable()) th_.join();
    return rc_;
  }

 private:
  std::thread th_;
  std::function<int(size_t)> fn_;
  std::atomic<size_t> rec_{0};
  std::atomic<bool> stop_{false};
  int rc_ = SV_OK;
};

// Host-buffer slice on one slot, pipelined over staging chunks: verdicts
// (verdict != null) and/or BLAKE2b cache keys (keys != null) into the
// caller's arrays.  keys_cb (optional, with keys and verdict): called once
// every key is in `keys` -- for a one-chunk batch while the verify kernels
// are still running, so the caller's cache walk overlaps them; *cb_done
// records that it ran.
inline int host_slice_locked(Device& D, const HostIn& in, size_t n, uint8_t* verdict, uint8_t* keys, int path,
                             const KeysCb& kcb, bool* cb_done) {
  KeyNotifier notifier;  // (joined on every return path)
  const size_t chunk = std::min(n, stage_chunk());
  int rc;
  const int ktm = kt_mode();
  // (decided at the first launch: a keyed batch's first pieces go up before it)
  int tables = -1;
  auto trace_at = [](const char* what) {
    if (stage_trace())
      fprintf(stderr, "SV_STAGE_TRACE %s at %.1f us @%.1f\n", what,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - g_trace_t0).count(),
              trace_abs_us());
  };
  if (verdict && (rc = presize_ws(D, path, chunk))) return rc;
  trace_at("workspace");
  const size_t out_per = (verdict ? 1 : 0) + (keys ? 32 : 0);
  // one chunk (latency-bound batches): everything on the kernel stream, no
  // cross-stream event waits
  const bool single = n <= chunk;
  hipStream_t up_s = single ? D.stream : D.h2d, down_s = single ? D.stream : D.d2h;
  if (!single && stage_ramp()) {
    // size both slots for a full chunk up front (the ramped first chunks
    // would otherwise grow the pinned buffers twice)
    size_t mt;
    const Image im = image_of(in, 0, chunk, &mt);
    for (Stage& s : D.st)
      if ((rc = s.h_in.ensure(im.bytes)) || (rc = s.d_in.ensure(im.bytes)) || (rc = s.h_out.ensure(out_per * chunk)))
        return rc;
  }
  size_t c = 0;
  size_t m = 0;
  for (size_t lo = 0; lo < n; lo += m, ++c) {
    Stage& s = D.st[c & 1];
    // slot c & 1 was last used by chunk c - 2: its results are collected
    // (which also means its H2D, kernels and D2H are complete)
    if ((rc = drain_stage(s, verdict, keys))) return rc;
    trace_at("slot drained");
    m = single ? n : chunk_len(c, chunk, n - lo);
    size_t msg_total;
    const Image im = image_of(in, lo, m, &msg_total);
    const bool early = single && kcb && keys && verdict;
    // a one-chunk keyed batch with a keys-ready callback: pack, copy up, hash
    // and copy the keys down in pieces, so the caller's walk starts early
    const std::vector<size_t> pb = early ? key_pieces(m) : std::vector<size_t>{0, m};
    const size_t P = pb.size() - 1;
    const bool in_place = single && P == 1 && bulk_in_place();
    const bool zc_out = in_place && verdict && bulk_zc_out();
    HostBuf& hin = in_place ? D.z_in : s.h_in;
    if ((rc = hin.ensure(im.bytes)) || (!in_place && (rc = s.d_in.ensure(im.bytes))) ||
        (rc = s.h_out.ensure(out_per * m)))
      return rc;
    if (verdict && !zc_out && (rc = s.d_verdict.ensure(m))) return rc;
    if (zc_out && (rc = D.z_out.ensure(m))) return rc;
    if (keys && (rc = s.d_keys.ensure(32 * m))) return rc;
    uint8_t* d = (uint8_t*)(in_place ? D.z_in.dp : s.d_in.p);
    uint8_t* hp = (uint8_t*)hin.p;
    const uint64_t* d_off = im.var ? (const uint64_t*)(d + im.o_off) : nullptr;
    const uint32_t* d_len = im.var ? (const uint32_t*)(d + im.o_len) : nullptr;
    while (s.pev.size() < P) {
      hipEvent_t e;
      SV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      s.pev.push_back(e);
    }
    const auto t_pack = stage_trace() ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    trace_at("staging");
    if (P == 1) {
      pack(in, lo, m, im, hp);
      if (!in_place && (rc = upload_image(D, s.d_in.p, s.h_in.p, im.bytes, up_s))) return rc;
      trace_at("uploads enqueued");
      if (!single) {
        SV_HIP(hipEventRecord(s.up, D.h2d));
        SV_HIP(hipStreamWaitEvent(D.stream, s.up, 0));
      }
      if (keys)
        SV_HIP(sv_launch_hash(0, D.grid * 2, d, d + im.o_sig, d + im.o_msg, d_off, d_len, in.fixed, m, s.d_keys.p,
                              D.stream));
      if (early) {
        // keys down on the D2H stream while the verify kernels run
        SV_HIP(hipEventRecord(s.done, D.stream));
        SV_HIP(hipStreamWaitEvent(D.d2h, s.done, 0));
        SV_HIP(hipMemcpyAsync((uint8_t*)s.h_out.p + m, s.d_keys.p, 32 * m, hipMemcpyDeviceToHost, D.d2h));
        SV_HIP(hipEventRecord(s.pev[0], D.d2h));
      }
    } else {
      // The pieces' keys go to the caller from a notifier thread while this
      // thread packs and uploads the next pieces (every callback runs on that
      // one thread, in order).
      const auto t0 = g_trace_t0;
      auto us = [t0] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
      // (pb and us by value: an error return leaves this scope before the
      // notifier is joined)
      notifier.start(D.phys, P, [&, m, lo, pb, us](size_t k) -> int {
        const size_t a = pb[k], b = pb[k + 1];
        SV_HIP(hipEventSynchronize(s.pev[k]));
        if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE keys piece %zu down at %.1f us\n", k, us());
        std::memcpy(keys + 32 * (lo + a), (uint8_t*)s.h_out.p + m + 32 * a, 32 * (b - a));
        kcb(lo + b);
        if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE keys piece %zu walked at %.1f us\n", k, us());
        return SV_OK;
      });
      uint64_t pos = 0;  // (each piece writes its own message offsets first)
      for (size_t k = 0; k < P; ++k) {
        const size_t a = pb[k], b = pb[k + 1];
        pos = pack_offsets(in, lo, a, b, pos, im, hp);
        if (im.var && b < m) ((uint64_t*)(hp + im.o_off))[b] = pos;  // (upload_rows reads the piece's end there)
        pack_rows(in, lo, a, b, im, hp, 1u << 16);
        if (k == 0) trace_at("piece 0 packed");
        // uploads on the copy stream: piece k + 1 goes up while piece k hashes
        // (the slot's earlier work is complete: drained above)
        if ((rc = upload_rows(im, m, a, b, in.fixed, msg_total, hp, d, D.h2d))) return rc;
        SV_HIP(hipEventRecord(s.up, D.h2d));
        SV_HIP(hipStreamWaitEvent(D.stream, s.up, 0));
        if (k == 0) trace_at("piece 0 uploading");
        SV_HIP(sv_launch_hash(0, D.grid * 2, d + 32 * a, d + im.o_sig + 64 * a,
                              d + im.o_msg + (im.var ? 0 : a * (size_t)in.fixed), d_off ? d_off + a : nullptr,
                              d_len ? d_len + a : nullptr, in.fixed, b - a, (uint8_t*)s.d_keys.p + 32 * a, D.stream));
        SV_HIP(hipEventRecord(s.done, D.stream));
        SV_HIP(hipStreamWaitEvent(D.d2h, s.done, 0));
        SV_HIP(hipMemcpyAsync((uint8_t*)s.h_out.p + m + 32 * a, (uint8_t*)s.d_keys.p + 32 * a, 32 * (b - a),
                              hipMemcpyDeviceToHost, D.d2h));
        SV_HIP(hipEventRecord(s.pev[k], D.d2h));
        notifier.recorded(k + 1);
        if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE piece %zu enqueued at %.1f us\n", k, us());
      }
    }
    if (stage_trace()) g_trace_pack_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_pack).count();
    if (verdict) {
      const int mode = verify_mode(im.var, in.fixed);
      // (only the one-lane geometry uses the tables: a quad-geometry batch
      // skips the key sample, ~4k scattered reads of the caller's keys)
      if (tables < 0)
        tables = launch_geometry(resolve_path(path, chunk), chunk) == SV_PATH_THROUGHPUT &&
                 (ktm == 1 || (ktm == 2 && repeated_keys(in, n)));
      // a keyed chunk with SV_VC_FEED_BULK set goes behind the slot's verdict cache, its keys being on the device
      // already (launch_cached_locked's cache-off test makes the two calls the same launch where the cache is off)
      const bool cached = keys && (vc_feed() & SV_VC_FEED_BULK) && vc_entries();
      void* dv = zc_out ? D.z_out.dp : s.d_verdict.p;
      const uint32_t kp = in_place && decode_first() ? SV_KP_IN_PLACE : 0u;
      if ((rc = cached ? launch_cached_locked(D, mode, path, d, d + im.o_sig, d + im.o_msg, d_off, d_len, in.fixed, m,
                                              dv, nullptr, tables != 0, kp, nullptr, s.d_keys.p, true)
                       : launch_audited_locked(D, mode, path, d, d + im.o_sig, d + im.o_msg, d_off, d_len, in.fixed, m,
                                               dv, nullptr, tables != 0, kp)))
        return rc;
      trace_at("launched");
    }
    if (!single) {
      SV_HIP(hipEventRecord(s.done, D.stream));
      SV_HIP(hipStreamWaitEvent(D.d2h, s.done, 0));
    }
    uint8_t* ho = (uint8_t*)s.h_out.p;
    if (verdict && !zc_out) SV_HIP(hipMemcpyAsync(ho, s.d_verdict.p, m, hipMemcpyDeviceToHost, down_s));
    if (keys && !early)
      SV_HIP(hipMemcpyAsync(ho + (verdict ? m : 0), s.d_keys.p, 32 * m, hipMemcpyDeviceToHost, down_s));
    SV_HIP(hipEventRecord(s.down, down_s));
    s.busy = true;
    s.lo = lo;
    s.m = m;
    s.zv = zc_out ? (const uint8_t*)D.z_out.p : nullptr;
    if (early) {
      if (P == 1) {
        SV_HIP(hipEventSynchronize(s.pev[0]));
        std::memcpy(keys + 32 * lo, ho + m, 32 * m);
        kcb(lo + m);
      } else if ((rc = notifier.join())) {
        return rc;
      }
      *cb_done = true;
    }
  }
  for (Stage& s : D.st)
    if ((rc = drain_stage(s, verdict, keys))) return rc;
  return SV_OK;
}

inline int host_slice(Device& D, const HostIn& in, size_t n, uint8_t* verdict, uint8_t* keys, int path,
                      const KeysCb& kcb = KeysCb(), bool* cb_done = nullptr) {
  return with_slot(D, [&] {
    const auto t0 = std::chrono::steady_clock::now();
    g_trace_t0 = t0;
    g_trace_pack_us = 0;
    const int rc = host_slice_locked(D, in, n, verdict, keys, path, kcb, cb_done);
    if (stage_trace())
      fprintf(stderr, "SV_STAGE_TRACE n=%zu pack %.1f us total %.1f us\n", n, g_trace_pack_us,
              std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    return rc;
  });
}

// Host feed of a slice without kernels (sv_host_feed_probe): host_slice's
// staging loop -- chunks of stage_chunk() with the ramp, packed into the
// slot's two pinned slots by the pack pool, and with `upload` copied up on
// the H2D stream, a slot reused once its copy is done -- and nothing else.
// staging_node: NUMA node of the first pinned slot's pages.
inline int feed_slice(Device& D, const HostIn& in, size_t n, int upload, int* staging_node) {
  std::lock_guard<std::mutex> g(D.mu);
  SV_HIP(hipSetDevice(D.phys));
  int rc;
  if ((rc = ready_locked(D))) return rc;
  const size_t chunk = std::min(n, stage_chunk());
  // (the slots' `busy` flags belong to host_slice's pending verdict copies:
  // the probe tracks its own uploads, and leaves nothing in flight on any
  // return -- the copy stream is drained before an error is reported)
  bool pending[2] = {false, false};
  auto drain = [&] { (void)hipStreamSynchronize(D.h2d); };
  size_t m = 0;
  for (size_t lo = 0, c = 0; lo < n; lo += m, ++c) {
    Stage& s = D.st[c & 1];
    if (pending[c & 1]) {
      const hipError_t e = hipEventSynchronize(s.up);
      pending[c & 1] = false;
      if (e != hipSuccess) {
        drain();
        return hip_fail(e, "feed probe: upload");
      }
    }
    m = n <= chunk ? n : chunk_len(c, chunk, n - lo);
    size_t msg_total;
    const Image im = image_of(in, lo, m, &msg_total);
    if ((rc = s.h_in.ensure(im.bytes)) || (upload && (rc = s.d_in.ensure(im.bytes)))) {
      drain();
      return rc;
    }
    pack(in, lo, m, im, (uint8_t*)s.h_in.p);
    if (upload) {
      hipError_t e = hipMemcpyAsync(s.d_in.p, s.h_in.p, im.bytes, hipMemcpyHostToDevice, D.h2d);
      if (e == hipSuccess) e = hipEventRecord(s.up, D.h2d);
      if (e != hipSuccess) {
        drain();
        return hip_fail(e, "feed probe: upload");
      }
      pending[c & 1] = true;
    }
  }
  SV_HIP(hipStreamSynchronize(D.h2d));
  if (staging_node) *staging_node = page_numa_node(D.st[0].h_in.p);
  return SV_OK;
}

// SHA-256 of a host slice of byte strings on one slot.
inline int sha_slice(Device& D, const uint8_t* data, const uint64_t* off, const uint32_t* len, size_t n, uint8_t* out) {
  std::lock_guard<std::mutex> g(D.mu);
  SV_HIP(hipSetDevice(D.phys));
  int rc;
  if ((rc = ready_locked(D))) return rc;
  size_t total = 0;
  for (size_t i = 0; i < n; ++i) total += len[i];
  const size_t o_len = 8 * n, o_msg = 12 * n, bytes = o_msg + std::max<size_t>(total, 1);
  if ((rc = D.h_sha.ensure(bytes)) || (rc = D.msg.ensure(bytes)) || (rc = D.keys.ensure(n * 32))) return rc;
  uint8_t* h = (uint8_t*)D.h_sha.p;
  uint64_t* offs = (uint64_t*)h;
  size_t pos = 0;
  for (size_t i = 0; i < n; ++i) {
    offs[i] = pos;
    if (len[i]) std::memcpy(h + o_msg + pos, data + off[i], len[i]);
    pos += len[i];
  }
  std::memcpy(h + o_len, len, 4 * n);
  SV_HIP(hipMemcpyAsync(D.msg.p, h, bytes, hipMemcpyHostToDevice, D.stream));
  uint8_t* d = (uint8_t*)D.msg.p;
  SV_HIP(sv_launch_hash(1, D.grid * 2, nullptr, nullptr, d + o_msg, (const uint64_t*)d, (const uint32_t*)(d + o_len),
                        0, n, D.keys.p, D.stream));
  SV_HIP(hipMemcpyAsync(out, D.keys.p, n * 32, hipMemcpyDeviceToHost, D.stream));
  SV_HIP(hipStreamSynchronize(D.stream));
  return SV_OK;
}

// The n x 32 message array a tx-body launch's hash kernel fills (caller
// holds D.mu, device set).  Growing it frees the old array, which earlier
// launches may still read, so the kernel stream is drained first.
inline int ensure_txmsg(Device& D, size_t n) {
  if (32 * n <= D.txmsg.cap) return SV_OK;
  SV_HIP(hipStreamSynchronize(D.stream));
  return D.txmsg.ensure(32 * n);
}

// A chunk's results in its pinned slot: verdicts (m), then digests (32 k).
struct TxPending {
  bool busy = false;
  TxChunk c;
};
inline int tx_drain(Stage& s, TxPending& pd, size_t dig_from, uint8_t* verdict, uint8_t* digests) {
  if (!pd.busy) return SV_OK;
  SV_HIP(hipEventSynchronize(s.down));
  pd.busy = false;
  const TxChunk& c = pd.c;
  const size_t m = c.s1 - c.s0;
  const uint8_t* h = (const uint8_t*)s.h_out.p;
  if (m) std::memcpy(verdict + c.s0, h, m);
  if (digests) {
    // (a body whose signatures straddle the slice's lower boundary was also
    // hashed by the slot before: that slot delivers its digest)
    const size_t from = std::max(c.b0, dig_from);
    if (from < c.b1) std::memcpy(digests + 32 * from, h + m + 32 * (from - c.b0), 32 * (c.b1 - from));
  }
  if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE tx chunk [%zu, %zu) drained @%.1f\n", c.b0, c.b1, trace_abs_us());
  return SV_OK;
}

// Bodies [B0, B1) and signatures [lo, hi) on one slot (caller holds D.mu,
// device set): per chunk pack -> H2D -> hash kernel -> verify launch (mode 0
// over the message array, same stream) -> D2H, over the slot's two staging
// slots as host_slice_locked does, so chunk c + 1 is packed and copied up
// while chunk c hashes and verifies.
inline int tx_slice_locked(Device& D, const TxIn& in, size_t B0, size_t B1, size_t lo, size_t hi, size_t dig_from,
                           uint8_t* verdict, uint8_t* digests, int path) {
  int rc;
  if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE tx slice @%.1f\n", trace_abs_us());
  const std::vector<TxChunk> plan = tx_plan(in, B0, B1, lo, hi, stage_chunk(), txbody_chunk_bytes());
  if (plan.empty()) return SV_OK;
  if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE tx plan: %zu chunks @%.1f\n", plan.size(), trace_abs_us());
  size_t max_m = 0;
  for (const TxChunk& c : plan) max_m = std::max(max_m, c.s1 - c.s0);
  // the message array and the largest launch's workspace first, so neither
  // grows under a running kernel
  if ((rc = ensure_txmsg(D, max_m))) return rc;
  if (max_m && (rc = presize_ws(D, path, max_m))) return rc;
  const bool single = plan.size() == 1;
  hipStream_t up_s = single ? D.stream : D.h2d, down_s = single ? D.stream : D.d2h;
  TxPending pend[2];
  for (size_t ci = 0; ci < plan.size(); ++ci) {
    const TxChunk& c = plan[ci];
    Stage& s = D.st[ci & 1];
    if ((rc = tx_drain(s, pend[ci & 1], dig_from, verdict, digests))) return rc;
    const size_t m = c.s1 - c.s0, k = c.b1 - c.b0;
    if ((rc = s.h_in.ensure(c.bytes)) || (rc = s.d_in.ensure(c.bytes)) || (rc = s.h_out.ensure(m + 32 * k)) ||
        (rc = s.d_verdict.ensure(std::max<size_t>(m, 1))) || (rc = s.d_keys.ensure(32 * k)))
      return rc;
    uint8_t* hp = (uint8_t*)s.h_in.p;
    uint8_t* d = (uint8_t*)s.d_in.p;
    if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE tx chunk %zu staging @%.1f\n", ci, trace_abs_us());
    tx_pack(in, c, lo, hi, hp);
    if (stage_trace())
      fprintf(stderr, "SV_STAGE_TRACE tx chunk %zu packed (%zu B, %zu sigs) @%.1f\n", ci, c.bytes, m, trace_abs_us());
    if ((rc = upload_image(D, d, hp, c.bytes, up_s))) return rc;
    if (!single) {
      SV_HIP(hipEventRecord(s.up, D.h2d));
      SV_HIP(hipStreamWaitEvent(D.stream, s.up, 0));
    }
    SV_HIP(sv_launch_txhash(D.grid * 8, in.nid, d + c.o_body, (const uint64_t*)(d + c.o_off),
                            (const uint32_t*)(d + c.o_len), d + c.o_kind, k, (const uint64_t*)(d + c.o_sb), m,
                            D.txmsg.p, s.d_keys.p, D.stream));
    if (m && (rc = launch_audited_locked(D, 0, path, d, d + c.o_sig, D.txmsg.p, nullptr, nullptr, 32, m,
                                         s.d_verdict.p, nullptr, kt_mode() == 1)))
      return rc;
    if (!single) {
      SV_HIP(hipEventRecord(s.done, D.stream));
      SV_HIP(hipStreamWaitEvent(D.d2h, s.done, 0));
    }
    uint8_t* ho = (uint8_t*)s.h_out.p;
    if (m) SV_HIP(hipMemcpyAsync(ho, s.d_verdict.p, m, hipMemcpyDeviceToHost, down_s));
    if (digests) SV_HIP(hipMemcpyAsync(ho + m, s.d_keys.p, 32 * k, hipMemcpyDeviceToHost, down_s));
    SV_HIP(hipEventRecord(s.down, down_s));
    pend[ci & 1].busy = true;
    pend[ci & 1].c = c;
    if (stage_trace()) fprintf(stderr, "SV_STAGE_TRACE tx chunk %zu enqueued @%.1f\n", ci, trace_abs_us());
  }
  for (int i = 0; i < 2; ++i)
    if ((rc = tx_drain(D.st[i], pend[i], dig_from, verdict, digests))) return rc;
  return SV_OK;
}

inline int tx_slice(Device& D, const TxIn& in, size_t B0, size_t B1, size_t lo, size_t hi, size_t dig_from,
                    uint8_t* verdict, uint8_t* digests, int path) {
  return with_slot(D, [&] { return tx_slice_locked(D, in, B0, B1, lo, hi, dig_from, verdict, digests, path); });
}

// ------------------------------------------------- pairing by hint (hinted tx bodies)
// The gathered key / signature / message arrays of a verify launch over np
// pairs (caller holds D.mu, device set).  Growing frees the old arrays, which
// an earlier launch may still read, so the kernel stream is drained first.
inline int ensure_txpairs(Device& D, size_t np) {
  if (32 * np <= D.txmsg.cap && 32 * np <= D.txpk.cap && 64 * np <= D.txsg.cap) return SV_OK;
  SV_HIP(hipStreamSynchronize(D.stream));
  int rc;
  if ((rc = D.txmsg.ensure(32 * np)) || (rc = D.txpk.ensure(32 * np)) || (rc = D.txsg.ensure(64 * np))) return rc;
  return SV_OK;
}

// The payload pairs of a check call (sv_txpair.hip sv_ppair_*) in D.txpp, np of them: verdicts (np) | pair_sig,
// pair_key (4 np each) | message lengths (4 np) | message offsets (8 np) | keys (32 np) | signatures (64 np) |
// payload rows (64 np), every section 16-byte aligned.  Shared by a call's chunks like the ed25519 pairs' gathered
// arrays: everything that touches it runs on D.stream in order, and growing drains that stream first.
struct PPairBufs {
  size_t o_idx, o_len, o_off, o_key, o_sig, o_msg, bytes;
};
inline PPairBufs ppair_layout(size_t np) {
  PPairBufs b;
  b.o_idx = al16(np);
  b.o_len = b.o_idx + al16(8 * np);
  b.o_off = b.o_len + al16(4 * np);
  b.o_key = b.o_off + al16(8 * np);
  b.o_sig = b.o_key + 32 * np;
  b.o_msg = b.o_sig + 64 * np;
  b.bytes = b.o_msg + 64 * np + 16;
  return b;
}
inline int ensure_txpp(Device& D, size_t bytes) {
  if (bytes <= D.txpp.cap) return SV_OK;
  SV_HIP(hipStreamSynchronize(D.stream));
  return D.txpp.ensure(bytes);
}

// The payload tables of a check call on the device (all device pointers; nq == 0: none).
struct PayloadDev {
  const uint64_t* qb = nullptr;  // n_bodies + 1
  const uint8_t* key = nullptr;
  const uint8_t* payload = nullptr;
  const uint8_t* len = nullptr;
  size_t nq = 0;
};

// ------------------------------------------------- the device sequence of the hinted and check forms
// HintIn's device twin: the body, signature and key arguments of a device-resident call, or of a chunk's image.
struct HintDev {
  const uint8_t* nid;  // (host memory)
  const void* bodies;
  const uint64_t* off;
  const uint32_t* len;
  const uint8_t* kind;
  size_t nb;
  const uint64_t* sb;  // signatures of body t: [sb[t], sb[t + 1]) of m
  const void* hint;
  const void* sig;
  size_t m;
  const uint64_t* kb;  // candidate keys of body t: [kb[t], kb[t + 1]) of q (a by-account call: the expansion's)
  const void* key;
  size_t q;
};
inline HintDev hint_dev_of(const uint8_t* nid, const PairChunk& p, const uint8_t* d) {
  return HintDev{nid, d + p.o_body, (const uint64_t*)(d + p.o_off), (const uint32_t*)(d + p.o_len), d + p.o_kind,
                 p.b1 - p.b0, (const uint64_t*)(d + p.o_sb), d + p.o_hint, d + p.o_sig, p.s1 - p.s0,
                 (const uint64_t*)(d + p.o_kb), d, p.k1 - p.k0};
}
// The check tables on the device.
struct CheckTabs {
  const uint8_t* sig_len = nullptr;  // per signature, or null: all 64
  int clamp = 0;
  const uint64_t* check_begin = nullptr;  // checks of body t
  const int32_t* needed = nullptr;
  size_t nc = 0;
  const uint64_t* signer_begin = nullptr;  // signers of check c
  const uint8_t* type = nullptr;
  const uint32_t* weight = nullptr;
  const uint32_t* key = nullptr;
  size_t ng = 0;
};
// The device view of one call or chunk: the hinted forms have `h` and `digests`, the check forms everything.
struct TxDev {
  HintDev h;
  void* digests;  // nb x 32 B: the contents hashes (tx_enqueue_hash)
  CheckTabs c;
  PayloadDev pl;
};
// The buffers the sequence writes, in one device buffer: the head -- ws, sv_pair_ws_bytes(k) | pair_begin, k + 1
// words -- from its start and, with payload candidates, the tail -- pws, sv_ppair_ws_bytes(k) | ppair_begin, k + 1
// words -- from o_tail, every section 16-byte aligned; h_cnt: the two pinned words the pair counts come back in.
struct TxBufs {
  void* ws;
  uint64_t* pair_begin;
  void* pws;
  uint64_t* ppair_begin;
  void* h_cnt;
  static size_t head(size_t k) { return al16(sv_pair_ws_bytes(k)) + al16(8 * (k + 1)); }
  static size_t tail(size_t k) { return al16(sv_ppair_ws_bytes(k)) + al16(8 * (k + 1)); }
  static TxBufs at(void* base, size_t o_tail, size_t k, void* h_cnt) {
    uint8_t* b = (uint8_t*)base;
    return TxBufs{b, (uint64_t*)(b + al16(sv_pair_ws_bytes(k))), b + o_tail,
                  (uint64_t*)(b + o_tail + al16(sv_ppair_ws_bytes(k))), h_cnt};
  }
};
// What the check kernel writes per check and, for a decide call, what the result kernels read and write
// (sv_launch_txresult; bad, bad_cap and n_bad: the device-resident form's only).
struct ResultDev {
  const uint8_t* role = nullptr;
  const uint8_t* flags = nullptr;
  uint8_t* code = nullptr;
  uint32_t* fail = nullptr;
  void* ws = nullptr;
  uint32_t* bad = nullptr;
  uint64_t bad_cap = 0;
  uint64_t* n_bad = nullptr;
};
struct DecideDev {
  uint8_t* ok;
  uint32_t* weight;
  uint64_t* used;
  const ResultDev* res;  // a decide call's, or null
};

// The contents hashes of T's bodies, on `st`.
inline int tx_enqueue_hash(const Device& D, const TxDev& T, hipStream_t st) {
  const HintDev& h = T.h;
  SV_HIP(sv_launch_txhash(D.grid * 8, h.nid, h.bodies, h.off, h.len, h.kind, h.nb, nullptr, 0, nullptr, T.digests, st));
  return SV_OK;
}

// Enqueue-counts, on `st` (the contents hashes need not be there yet): the pair count and scan, the payload-pair
// count and scan where the call has candidates, and both totals to B.h_cnt in one copy (the payload pairing's
// total is the word behind the ed25519 pairing's).  The caller waits -- a chunk for its upload event, a device call
// for its stream -- and reads the totals with tx_counted.
inline int tx_enqueue_counts(const TxDev& T, const TxBufs& B, hipStream_t st) {
  const HintDev& h = T.h;
  SV_HIP(sv_launch_pair_count(h.sb, h.hint, h.sig, h.m, h.kb, h.key, h.q, h.nb, B.ws, B.pair_begin, st));
  if (T.pl.nq)
    SV_HIP(sv_launch_ppair_count(h.sb, h.hint, h.m, T.pl.qb, T.pl.key, T.pl.payload, T.pl.len, T.pl.nq, h.nb, B.ws,
                                 B.pws, B.ppair_begin, st));
  SV_HIP(hipMemcpyAsync(B.h_cnt, sv_pair_total(B.ws, h.nb), T.pl.nq ? 16 : 8, hipMemcpyDeviceToHost, st));
  return SV_OK;
}
inline void tx_counted(const TxDev& T, const TxBufs& B, size_t* np, size_t* npp) {
  *np = (size_t)((const uint64_t*)B.h_cnt)[0];
  *npp = T.pl.nq ? (size_t)((const uint64_t*)B.h_cnt)[1] : 0;
}

// The np counted pairs on D.stream (caller holds D.mu, device set): the fill into pair_sig / pair_key and the
// gathered arrays, and with `verdict` the verify launch over them (mode 0, 32-byte messages).
inline int tx_enqueue_pairs(Device& D, const TxDev& T, const TxBufs& B, size_t np, uint32_t* pair_sig,
                            uint32_t* pair_key, void* verdict, void* bitmap, int path) {
  const HintDev& h = T.h;
  int rc;
  if ((rc = ensure_txpairs(D, np))) return rc;
  SV_HIP(sv_launch_pair_fill(h.sb, h.hint, h.sig, h.m, h.kb, h.key, h.q, h.nb, B.ws, B.pair_begin, np, pair_sig,
                             pair_key, D.txpk.p, D.txsg.p, D.txmsg.p, T.digests, D.stream));
  if (!np || !verdict) return SV_OK;
  return launch_cached_locked(D, 0, path, D.txpk.p, D.txsg.p, D.txmsg.p, nullptr, nullptr, 32, np, verdict, bitmap,
                              kt_mode() == 1);
}

// Enqueue-decide, on D.stream after the counts came back: the fill and the verify launch, the payload pairs' fill
// and their variable-length verify launch (in D.txpp, ppair_layout(npp)), the check kernel and, with out.res, the
// result kernels.  dv: verdicts (np, padded to 16) | pair_sig | pair_key (4 np each), sized by the caller.
inline int tx_enqueue_decide(Device& D, const TxDev& T, const TxBufs& B, size_t np, size_t npp, uint8_t* dv,
                             const DecideDev& out, int path) {
  const HintDev& h = T.h;
  const CheckTabs& c = T.c;
  int rc;
  uint32_t* d_ps = (uint32_t*)(dv + al16(np));
  uint32_t* d_pk = d_ps + np;
  if (npp && (rc = ensure_txpp(D, ppair_layout(npp).bytes))) return rc;
  if ((rc = tx_enqueue_pairs(D, T, B, np, d_ps, d_pk, dv, nullptr, path))) return rc;
  const PPairBufs L = ppair_layout(npp);
  uint8_t* b = (uint8_t*)D.txpp.p;
  uint32_t* d_pps = (uint32_t*)(b + L.o_idx);
  if (npp) {
    SV_HIP(sv_launch_ppair_fill(h.sb, h.hint, h.sig, h.m, T.pl.qb, T.pl.key, T.pl.payload, T.pl.len, T.pl.nq, h.nb, B.ws,
                                B.pws, B.ppair_begin, npp, d_pps, d_pps + npp, b + L.o_key, b + L.o_sig, b + L.o_msg,
                                (uint64_t*)(b + L.o_off), (uint32_t*)(b + L.o_len), D.stream));
    if ((rc = launch_cached_locked(D, 1, path, b + L.o_key, b + L.o_sig, b + L.o_msg, (const uint64_t*)(b + L.o_off),
                                   (const uint32_t*)(b + L.o_len), 0, npp, b, nullptr)))
      return rc;
  }
  SV_HIP(sv_launch_txcheck_payload(h.sb, h.hint, h.sig, c.sig_len, h.m, h.kb, h.key, h.q, h.nb, B.pair_begin, d_ps, d_pk,
                                   dv, np, T.digests, c.check_begin, c.needed, c.nc, c.signer_begin, c.type, c.weight,
                                   c.key, c.ng, c.clamp, B.ppair_begin, d_pps, d_pps + npp, b, npp, T.pl.qb, T.pl.nq,
                                   out.ok, out.weight, out.used, D.stream));
  if (const ResultDev* R = out.res) {
    const sv_txresult_in I{c.check_begin, h.sb, out.ok, out.used, R->role, R->flags, h.nb, c.nc, h.m};
    SV_HIP(sv_launch_txresult(&I, R->code, R->fail, R->ws, R->bad, R->bad_cap, R->n_bad, D.stream));
  }
  return SV_OK;
}

// Where a slice's pairs go: the caller's arrays (one slot), or vectors of the
// slice's own that grow with the count (several slots: where a slot's pairs
// start in the caller's arrays is only known once the slots before it are
// done).
struct PairSink {
  uint32_t* ps = nullptr;
  uint32_t* pk = nullptr;
  uint8_t* pv = nullptr;
  size_t cap = 0;
  bool own = false;
  std::vector<uint32_t> vs, vk;
  std::vector<uint8_t> vv;
  bool room(size_t total) {
    if (total > cap) return false;
    if (own && total > vv.size()) {
      vs.resize(total);
      vk.resize(total);
      vv.resize(total);
      ps = vs.data();
      pk = vk.data();
      pv = vv.data();
    }
    return true;
  }
};

// A chunk's results in its pinned slot: verdicts (np, padded to 16) | pair_sig
// (4 np) | pair_key (4 np) | pair_begin (8 k, padded) | digests (32 k).
struct PairPending {
  bool busy = false;
  PairChunk c;
  size_t np = 0, base = 0;
};
inline int pair_drain(Stage& s, PairPending& pd, PairSink& sink, uint64_t* pair_begin, uint8_t* digests) {
  if (!pd.busy) return SV_OK;
  SV_HIP(hipEventSynchronize(s.down));
  pd.busy = false;
  const PairChunk& c = pd.c;
  const size_t np = pd.np, k = c.b1 - c.b0;
  const uint8_t* h = (const uint8_t*)s.h_out.p;
  const uint32_t* hs = (const uint32_t*)(h + al16(np));
  const uint32_t* hk = hs + np;
  const uint64_t* hb = (const uint64_t*)(h + al16(np) + al16(8 * np));
  if (np) std::memcpy(sink.pv + pd.base, h, np);
  for (size_t i = 0; i < np; ++i) {
    sink.ps[pd.base + i] = hs[i] + (uint32_t)c.s0;
    sink.pk[pd.base + i] = hk[i] + (uint32_t)c.k0;
  }
  for (size_t i = 0; i < k; ++i) pair_begin[c.b0 + i] = hb[i] + pd.base;
  if (digests) std::memcpy(digests + 32 * c.b0, (const uint8_t*)(hb) + al16(8 * k), 32 * k);
  return SV_OK;
}

// Bodies [B0, B1) with their signatures and keys on one slot (caller holds
// D.mu, device set).  Per chunk: pack -> H2D -> contents hashes -> count and
// scan -> the chunk's pair count back (the one wait: it covers the upload, the
// hash and the pairing, on the upload stream, not a verify) -> fill and the
// verify launch (mode 0 over the gathered arrays) -> D2H, over the slot's two
// staging slots, so chunk c + 1 is packed while chunk c verifies.  pair_begin
// [B0, B1) and the sink's indices count from the slice's first pair; *count:
// the slice's exact number of pairs, also when it exceeds the sink (then the
// remaining chunks only count, and the call returns SV_ERR_PAIR_CAP).
inline int hinted_slice_locked(Device& D, const HintIn& in, size_t B0, size_t B1, PairSink& sink,
                               uint64_t* pair_begin, uint8_t* digests, size_t* count, int path) {
  int rc;
  *count = 0;
  const std::vector<PairChunk> plan = pair_plan(in, B0, B1, stage_chunk(), stage_chunk(), txbody_chunk_bytes());
  if (plan.empty()) return SV_OK;
  const bool single = plan.size() == 1;
  hipStream_t up_s = single ? D.stream : D.h2d, down_s = single ? D.stream : D.d2h;
  PairPending pend[2];
  size_t total = 0;
  bool overflow = false;
  for (size_t ci = 0; ci < plan.size(); ++ci) {
    const PairChunk& c = plan[ci];
    Stage& s = D.st[ci & 1];
    if ((rc = pair_drain(s, pend[ci & 1], sink, pair_begin, digests))) return rc;
    const size_t k = c.b1 - c.b0;
    if ((rc = s.h_in.ensure(c.bytes)) || (rc = s.d_in.ensure(c.bytes)) || (rc = s.d_pair.ensure(TxBufs::head(k))) ||
        (rc = s.d_keys.ensure(32 * k)) || (rc = s.h_cnt.ensure(64)))
      return rc;
    uint8_t* hp = (uint8_t*)s.h_in.p;
    uint8_t* d = (uint8_t*)s.d_in.p;
    pair_pack(in, c, hp);
    if ((rc = upload_image(D, d, hp, c.bytes, up_s))) return rc;
    const TxDev T{hint_dev_of(in.nid, c, d), s.d_keys.p};
    const TxBufs B = TxBufs::at(s.d_pair.p, TxBufs::head(k), k, s.h_cnt.p);  // (no payload candidates: no tail)
    if (!overflow && (rc = tx_enqueue_hash(D, T, up_s))) return rc;
    if ((rc = tx_enqueue_counts(T, B, up_s))) return rc;
    SV_HIP(hipEventRecord(s.up, up_s));
    SV_HIP(hipEventSynchronize(s.up));
    size_t np, npp;
    tx_counted(T, B, &np, &npp);
    const size_t base = total;
    total += np;
    if (overflow || !sink.room(total)) {
      overflow = true;
      continue;
    }
    if (!single) SV_HIP(hipStreamWaitEvent(D.stream, s.up, 0));
    const size_t o_idx = al16(np), o_pb = o_idx + al16(8 * np), o_dig = o_pb + al16(8 * k);
    if ((rc = s.d_verdict.ensure(o_pb + 16)) || (rc = s.h_out.ensure(o_dig + 32 * k))) return rc;
    uint8_t* dv = (uint8_t*)s.d_verdict.p;
    if ((rc = tx_enqueue_pairs(D, T, B, np, (uint32_t*)(dv + o_idx), (uint32_t*)(dv + o_idx) + np, dv, nullptr, path)))
      return rc;
    if (!single) {
      SV_HIP(hipEventRecord(s.done, D.stream));
      SV_HIP(hipStreamWaitEvent(D.d2h, s.done, 0));
    }
    uint8_t* ho = (uint8_t*)s.h_out.p;
    if (np) SV_HIP(hipMemcpyAsync(ho, dv, o_idx + 8 * np, hipMemcpyDeviceToHost, down_s));
    SV_HIP(hipMemcpyAsync(ho + o_pb, B.pair_begin, 8 * k, hipMemcpyDeviceToHost, down_s));
    if (digests) SV_HIP(hipMemcpyAsync(ho + o_dig, s.d_keys.p, 32 * k, hipMemcpyDeviceToHost, down_s));
    SV_HIP(hipEventRecord(s.down, down_s));
    pend[ci & 1].busy = true;
    pend[ci & 1].c = c;
    pend[ci & 1].np = np;
    pend[ci & 1].base = base;
  }
  for (int i = 0; i < 2; ++i)
    if ((rc = pair_drain(D.st[i], pend[i], sink, pair_begin, digests))) return rc;
  *count = total;
  if (overflow) return fail(SV_ERR_PAIR_CAP, "more pairs than pair_cap holds");
  return SV_OK;
}

inline int hinted_slice(Device& D, const HintIn& in, size_t B0, size_t B1, PairSink& sink, uint64_t* pair_begin,
                        uint8_t* digests, size_t* count, int path) {
  return with_slot(D, [&] { return hinted_slice_locked(D, in, B0, B1, sink, pair_begin, digests, count, path); });
}

// ------------------------------------------------- checks decided on the device
// Where a slice's decisions go: the caller's arrays, indexed by global check.
// What a decide call adds to a slice (txresult.h): the caller's roles and flags, indexed by global check and body,
// and where the codes go, indexed by global body.  body_fail is body-local, so chunks and slots rebase nothing.
struct ResultOut {
  const uint8_t* role;   // optional
  const uint8_t* flags;  // optional
  uint8_t* code;
  uint32_t* fail;        // optional
};
struct CheckOut {
  uint8_t* ok;  // (a decide call: each of the three optional)
  uint32_t* weight;
  uint64_t* used;
  uint8_t* digests;  // optional
  const ResultOut* res = nullptr;  // a decide call's; null: a check call, which launches and copies what it always did
};
// does the chunk's 13 bytes per check come back?
inline bool check_arrays_wanted(const CheckOut& out) { return !out.res || out.ok || out.weight || out.used; }

// A decide chunk's roles and flags behind its image (role: nc bytes | flags: k bytes, each only where the caller
// has them), and its results behind the check arrays on the device: body_code (k) | body_fail (4 k) | the result
// kernels' workspace.  Without `res` the image is `img` bytes and nothing else is laid out.
struct ResultBufs {
  size_t o_role, o_flag, img;  // the image
  size_t o_code, o_fail, o_ws, dev;  // s.d_verdict
};
inline ResultBufs result_layout(const ResultOut* res, size_t img, size_t nc, size_t k, size_t dev) {
  ResultBufs b;
  b.o_role = b.o_flag = b.img = img;
  b.o_code = b.o_fail = b.o_ws = b.dev = dev;
  if (!res) return b;
  b.o_role = al16(img);
  b.o_flag = b.o_role + (res->role ? al16(nc) : 0);
  b.img = b.o_flag + (res->flags ? al16(k) : 0);
  b.o_code = al16(dev);
  b.o_fail = b.o_code + al16(k);
  b.o_ws = b.o_fail + al16(4 * k);
  b.dev = b.o_ws + al16(sv_txresult_ws_bytes(k));
  return b;
}
inline void result_pack(const ResultOut* res, const ResultBufs& b, size_t c0, size_t nc, size_t b0, size_t k,
                        uint8_t* h) {
  if (!res) return;
  if (res->role && nc) std::memcpy(h + b.o_role, res->role + c0, nc);
  if (res->flags && k) std::memcpy(h + b.o_flag, res->flags + b0, k);
}
// What the result kernel behind the chunk's check kernel reads and writes: d the chunk's image, dv its s.d_verdict.
inline ResultDev result_dev(const ResultOut& res, const ResultBufs& b, const uint8_t* d, uint8_t* dv) {
  return ResultDev{res.role ? d + b.o_role : nullptr, res.flags ? d + b.o_flag : nullptr, dv + b.o_code,
                   res.fail ? (uint32_t*)(dv + b.o_fail) : nullptr, dv + b.o_ws};
}

// A chunk's results in its pinned slot: check_used (8 nc) | check_weight (4 nc)
// | check_ok (nc, padded to 16) | digests (32 k) and, for a decide call,
// | body_code (k, padded to 16) | body_fail (4 k, only where asked for).
struct CheckPending {
  bool busy = false;
  CheckChunk c;
};
inline int check_drain(Stage& s, CheckPending& pd, const CheckOut& out) {
  if (!pd.busy) return SV_OK;
  SV_HIP(hipEventSynchronize(s.down));
  pd.busy = false;
  const CheckChunk& c = pd.c;
  const size_t nc = c.c1 - c.c0, k = c.p.b1 - c.p.b0;
  const uint8_t* h = (const uint8_t*)s.h_out.p;
  if (nc) {
    if (out.used) std::memcpy(out.used + c.c0, h, 8 * nc);
    if (out.weight) std::memcpy(out.weight + c.c0, h + 8 * nc, 4 * nc);
    if (out.ok) std::memcpy(out.ok + c.c0, h + 12 * nc, nc);
  }
  const size_t o_dig = al16(13 * nc);
  if (out.digests) std::memcpy(out.digests + 32 * c.p.b0, h + o_dig, 32 * k);
  if (out.res) {
    std::memcpy(out.res->code + c.p.b0, h + o_dig + 32 * k, k);
    if (out.res->fail) std::memcpy(out.res->fail + c.p.b0, h + o_dig + 32 * k + al16(k), 4 * k);
  }
  return SV_OK;
}

// The chunk loop of the check forms.  Bodies [B0, B1) with their signatures and checks on one slot (caller holds
// D.mu, device set).  Per chunk: pack -> H2D -> contents hashes -> the form's tables -> pair counts and scans ->
// the counts back (the one wait: it covers the upload, the hash, the tables and the pairing, on the upload
// stream, not a verify) -> fill -> verify launches -> check kernel (-> result kernel), over the slot's two
// staging slots, so chunk c + 1 is packed while chunk c verifies; only the check arrays, the digests and a decide
// call's codes come back.  The pairs live in the stage's d_verdict, sized from the count.  `src` is the form (src.in.h: its HintIn):
//   plan(B0, B1)              its chunks (each with .p, the hinted image, and .c0 / .c1, its checks)
//   begin(D, single)          once, ahead of the first chunk
//   prepare(s, c, &bytes, &nq) the chunk's image size and payload candidates; sizes what else of the stage it uses
//   pack(c, hp)               the image
//   tables(D, s, c, d, st, T) enqueues on `st` what makes the chunk's key, check and payload tables, and names
//                             them in T (T.h, the chunk's hinted image, is filled in)
template <class Src>
inline int check_chunks_locked(Device& D, Src& src, size_t B0, size_t B1, const CheckOut& out, int path) {
  int rc;
  const auto plan = src.plan(B0, B1);
  if (plan.empty()) return SV_OK;
  const bool single = plan.size() == 1;
  hipStream_t up_s = single ? D.stream : D.h2d, down_s = single ? D.stream : D.d2h;
  if ((rc = src.begin(D, single))) return rc;
  CheckPending pend[2];
  for (size_t ci = 0; ci < plan.size(); ++ci) {
    const auto& c = plan[ci];
    Stage& s = D.st[ci & 1];
    if ((rc = check_drain(s, pend[ci & 1], out))) return rc;
    const size_t k = c.p.b1 - c.p.b0, nc = c.c1 - c.c0;
    size_t bytes, nq;
    if ((rc = src.prepare(s, c, &bytes, &nq))) return rc;
    const size_t img = result_layout(out.res, bytes, nc, k, 0).img;
    if ((rc = s.h_in.ensure(img)) || (rc = s.d_in.ensure(img)) ||
        (rc = s.d_pair.ensure(TxBufs::head(k) + (nq ? TxBufs::tail(k) : 0))) || (rc = s.d_keys.ensure(32 * k)) ||
        (rc = s.h_cnt.ensure(64)))
      return rc;
    const TxBufs B = TxBufs::at(s.d_pair.p, TxBufs::head(k), k, s.h_cnt.p);
    uint8_t* hp = (uint8_t*)s.h_in.p;
    uint8_t* d = (uint8_t*)s.d_in.p;
    src.pack(c, hp);
    result_pack(out.res, result_layout(out.res, bytes, nc, k, 0), c.c0, nc, c.p.b0, k, hp);
    if ((rc = upload_image(D, d, hp, img, up_s))) return rc;
    TxDev T{hint_dev_of(src.in.h.nid, c.p, d), s.d_keys.p};
    if ((rc = tx_enqueue_hash(D, T, up_s))) return rc;
    if ((rc = src.tables(D, s, c, d, up_s, &T))) return rc;
    if ((rc = tx_enqueue_counts(T, B, up_s))) return rc;
    SV_HIP(hipEventRecord(s.up, up_s));
    SV_HIP(hipEventSynchronize(s.up));
    size_t np, npp;
    tx_counted(T, B, &np, &npp);
    if (!single) SV_HIP(hipStreamWaitEvent(D.stream, s.up, 0));
    // verdicts (np, padded) | pair_sig, pair_key (4 np each, padded) | used | weight | ok
    const size_t o_res = al16(np) + al16(8 * np), o_dig = al16(13 * nc);
    const ResultBufs RB = result_layout(out.res, bytes, nc, k, o_res + 13 * nc);
    if ((rc = s.d_verdict.ensure(RB.dev + 16)) ||
        (rc = s.h_out.ensure(o_dig + 32 * k + (out.res ? al16(k) + 4 * k : 0))))
      return rc;
    uint8_t* dv = (uint8_t*)s.d_verdict.p;
    const ResultDev R = out.res ? result_dev(*out.res, RB, d, dv) : ResultDev();
    const DecideDev dd{dv + o_res + 12 * nc, (uint32_t*)(dv + o_res + 8 * nc), (uint64_t*)(dv + o_res),
                       out.res ? &R : nullptr};
    if ((rc = tx_enqueue_decide(D, T, B, np, npp, dv, dd, path))) return rc;
    if (!single) {
      SV_HIP(hipEventRecord(s.done, D.stream));
      SV_HIP(hipStreamWaitEvent(D.d2h, s.done, 0));
    }
    uint8_t* ho = (uint8_t*)s.h_out.p;
    if (nc && check_arrays_wanted(out)) SV_HIP(hipMemcpyAsync(ho, dv + o_res, 13 * nc, hipMemcpyDeviceToHost, down_s));
    if (out.digests) SV_HIP(hipMemcpyAsync(ho + o_dig, s.d_keys.p, 32 * k, hipMemcpyDeviceToHost, down_s));
    if (out.res)
      SV_HIP(hipMemcpyAsync(ho + o_dig + 32 * k, dv + RB.o_code, al16(k) + (out.res->fail ? 4 * k : 0),
                            hipMemcpyDeviceToHost, down_s));
    SV_HIP(hipEventRecord(s.down, down_s));
    pend[ci & 1].busy = true;
    pend[ci & 1].c.p = c.p;
    pend[ci & 1].c.c0 = c.c0;
    pend[ci & 1].c.c1 = c.c1;
  }
  for (int i = 0; i < 2; ++i)
    if ((rc = check_drain(D.st[i], pend[i], out))) return rc;
  return SV_OK;
}

// The explicit form: the chunk's tables are sections of its image.
struct CheckSrc {
  const CheckIn& in;
  int clamp;
  PayloadChunk pc{};
  // (a signer is 9 bytes of image against a signature's 68: eight staging chunks of them bound a chunk, so a
  // multisig batch is not cut many times more often than its signatures would cut it -- every chunk waits once
  // for its pair count)
  std::vector<CheckChunk> plan(size_t B0, size_t B1) const {
    return check_plan(in, B0, B1, stage_chunk(), stage_chunk(), txbody_chunk_bytes(), stage_chunk(),
                      8 * stage_chunk());
  }
  int begin(Device&, bool) { return SV_OK; }
  int prepare(Stage&, const CheckChunk& c, size_t* bytes, size_t* nq) {
    pc = payload_chunk(in, c);
    *bytes = pc.bytes;
    *nq = pc.q1 - pc.q0;
    return SV_OK;
  }
  void pack(const CheckChunk& c, uint8_t* hp) const {
    check_pack(in, c, hp);
    payload_pack(in, c, pc, hp);
  }
  int tables(Device&, Stage&, const CheckChunk& c, const uint8_t* d, hipStream_t, TxDev* T) const {
    T->c = CheckTabs{in.sig_len ? d + c.o_sl : nullptr, clamp, (const uint64_t*)(d + c.o_cb),
                     (const int32_t*)(d + c.o_need), c.c1 - c.c0, (const uint64_t*)(d + c.o_gb), d + c.o_gt,
                     (const uint32_t*)(d + c.o_gw), (const uint32_t*)(d + c.o_gk), c.g1 - c.g0};
    if (const size_t nq = pc.q1 - pc.q0)
      T->pl = PayloadDev{(const uint64_t*)(d + pc.o_qb), d + pc.o_qk, d + pc.o_qp, d + pc.o_ql, nq};
    return SV_OK;
  }
};

inline int check_slice(Device& D, const CheckIn& in, size_t B0, size_t B1, int clamp, const CheckOut& out, int path) {
  return with_slot(D, [&] {
    CheckSrc src{in, clamp};
    return check_chunks_locked(D, src, B0, B1, out, path);
  });
}

// ------------------------------------------------- checks by account
// The explicit tables of a by-account check call on the device, in one buffer
// (sv_txacct.hip fills them): the expansion's workspace (ws bytes) | key_begin |
// pkey_begin (8 (k + 1) each) | signer_begin (8 (nc + 1)) | check_needed (4 nc) and, with the row counts known,
// key (32 nk) | pkey (32 nq) | payload rows (64 nq) | signer_weight | signer_key (4 ng each) | pkey_len (nq) |
// signer_type (ng); every section 16-byte aligned.  own_rows: the row sections are a buffer of their own, from
// offset 0 (the device-resident form sizes them after its wait); else they follow the CSR part.
struct AcctBufs {
  size_t o_kb, o_qb, o_gb, o_need, head;                            // the CSR part: [0, head)
  size_t o_key, o_qkey, o_qpay, o_gw, o_gk, o_qlen, o_gt, bytes;  // the rows: [o_key, bytes)
};
inline AcctBufs acct_layout(size_t ws, size_t k, size_t nc, bool own_rows, size_t nk, size_t nq, size_t ng) {
  AcctBufs b;
  b.o_kb = al16(ws);
  b.o_qb = b.o_kb + al16(8 * (k + 1));
  b.o_gb = b.o_qb + al16(8 * (k + 1));
  b.o_need = b.o_gb + al16(8 * (nc + 1));
  b.head = b.o_need + al16(4 * nc) + 16;
  b.o_key = own_rows ? 0 : b.head;
  b.o_qkey = b.o_key + 32 * nk;
  b.o_qpay = b.o_qkey + 32 * nq;
  b.o_gw = b.o_qpay + 64 * nq;
  b.o_gk = b.o_gw + al16(4 * ng);
  b.o_qlen = b.o_gk + al16(4 * ng);
  b.o_gt = b.o_qlen + al16(nq);
  b.bytes = b.o_gt + al16(ng) + 16;
  return b;
}
inline sv_acct_out acct_out(const AcctBufs& L, uint8_t* head, uint8_t* rows, size_t nk, size_t nq, size_t ng) {
  sv_acct_out O;
  O.key_begin = (uint64_t*)(head + L.o_kb);
  O.pkey_begin = (uint64_t*)(head + L.o_qb);
  O.signer_begin = (uint64_t*)(head + L.o_gb);
  O.check_needed = (int32_t*)(head + L.o_need);
  O.key = rows + L.o_key;
  O.pkey = rows + L.o_qkey;
  O.ppay = rows + L.o_qpay;
  O.gweight = (uint32_t*)(rows + L.o_gw);
  O.gkey = (uint32_t*)(rows + L.o_gk);
  O.plen = rows + L.o_qlen;
  O.gtype = rows + L.o_gt;
  O.nk = nk;
  O.nq = nq;
  O.ng = ng;
  return O;
}
// ... as the key, check and payload tables of the device sequence, with what the caller keeps of the check tables
inline void acct_tables(const sv_acct_out& O, const uint8_t* sig_len, int clamp, const uint64_t* check_begin,
                        size_t nc, TxDev* T) {
  T->h.kb = O.key_begin;
  T->h.key = O.key;
  T->h.q = O.nk;
  T->c = CheckTabs{sig_len, clamp, check_begin, O.check_needed, nc, O.signer_begin, O.gtype, O.gweight, O.gkey, O.ng};
  if (O.nq) T->pl = PayloadDev{O.pkey_begin, O.pkey, O.ppay, O.plen, O.nq};
}

// The account table of a host call in D.txatab: key (32 na) | signer keys (32 ns) | payload rows (64 np) |
// asigner_begin (8 (na + 1)) | weights | payload indices (4 ns each) | thresholds (4 na) | types (ns) | payload
// lengths (np) | the per-account counts and ranks (sv_acct_tab_ws_bytes), every section 16-byte aligned.
struct AcctTabBufs {
  size_t o_skey, o_pay, o_sbeg, o_sw, o_sp, o_thr, o_st, o_pl, o_ws, bytes;
};
inline AcctTabBufs acct_tab_layout(size_t na, size_t ns, size_t np) {
  AcctTabBufs b;
  b.o_skey = 32 * na;
  b.o_pay = b.o_skey + 32 * ns;
  b.o_sbeg = b.o_pay + 64 * np;
  b.o_sw = b.o_sbeg + al16(8 * (na + 1));
  b.o_sp = b.o_sw + al16(4 * ns);
  b.o_thr = b.o_sp + al16(4 * ns);
  b.o_st = b.o_thr + al16(4 * na);
  b.o_pl = b.o_st + al16(ns);
  b.o_ws = b.o_pl + al16(np);
  b.bytes = b.o_ws + al16(sv_acct_tab_ws_bytes(na, ns)) + 16;
  return b;
}

// The account table up, once per slot per call, ahead of the first chunk: straight from the caller's arrays (they
// stay valid for the whole call) on D.stream, then the per-account kernel.  *T: the table on the device.  Grown
// like ensure_txpairs: the streams that may still read the old one are drained first.
inline int acct_table_upload(Device& D, const sv_txaccounts& A, sv_acct_tab* T, const void** tab_ws) {
  const size_t na = A.n_accounts, ns = A.n_asigners, np = A.n_apayloads;
  const AcctTabBufs L = acct_tab_layout(na, ns, np);
  if (L.bytes > D.txatab.cap) {
    SV_HIP(hipStreamSynchronize(D.h2d));
    SV_HIP(hipStreamSynchronize(D.stream));
    int rc;
    if ((rc = D.txatab.ensure(L.bytes))) return rc;
  }
  uint8_t* d = (uint8_t*)D.txatab.p;
  auto up = [&](size_t o, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(d + o, src, bytes, hipMemcpyHostToDevice, D.stream) : hipSuccess;
  };
  SV_HIP(up(0, A.acct_key, 32 * na));
  SV_HIP(up(L.o_skey, A.asigner_key, 32 * ns));
  SV_HIP(up(L.o_pay, A.apayload, 64 * np));
  SV_HIP(up(L.o_sbeg, A.asigner_begin, 8 * (na + 1)));
  SV_HIP(up(L.o_sw, A.asigner_weight, 4 * ns));
  if (A.asigner_payload) SV_HIP(up(L.o_sp, A.asigner_payload, 4 * ns));
  SV_HIP(up(L.o_thr, A.acct_thresholds, 4 * na));
  SV_HIP(up(L.o_st, A.asigner_type, ns));
  SV_HIP(up(L.o_pl, A.apayload_len, np));
  T->key = d;
  T->skey = d + L.o_skey;
  T->pay = d + L.o_pay;
  T->sbeg = (const uint64_t*)(d + L.o_sbeg);
  T->sweight = (const uint32_t*)(d + L.o_sw);
  T->spay = A.asigner_payload ? (const uint32_t*)(d + L.o_sp) : nullptr;
  T->thr = d + L.o_thr;
  T->stype = d + L.o_st;
  T->plen = d + L.o_pl;
  T->na = na;
  T->ns = ns;
  T->np = np;
  *tab_ws = d + L.o_ws;
  SV_HIP(sv_launch_acct_table(T, d + L.o_ws, D.stream));
  return SV_OK;
}

// The by-account form of check_chunks_locked: the account table up once, then per chunk the expansion kernels
// between the contents hashes and the pairing -- count, scan, begin, rows, signers (the row counts are the
// planner's: no wait).  A chunk's explicit tables live in the stage's d_acct.
struct AcctSrc {
  const AcctIn& in;
  const sv_txaccounts& A;
  int clamp;
  sv_acct_tab tab{};
  const void* tab_ws = nullptr;
  AcctBufs L{};
  std::vector<AcctChunk> plan(size_t B0, size_t B1) const {
    return acct_plan(in, B0, B1, stage_chunk(), stage_chunk(), txbody_chunk_bytes(), stage_chunk(), 8 * stage_chunk());
  }
  int begin(Device& D, bool single) {
    int rc;
    if ((rc = acct_table_upload(D, A, &tab, &tab_ws))) return rc;
    if (!single) {
      SV_HIP(hipEventRecord(D.dep_in, D.stream));
      SV_HIP(hipStreamWaitEvent(D.h2d, D.dep_in, 0));
    }
    return SV_OK;
  }
  int prepare(Stage& s, const AcctChunk& c, size_t* bytes, size_t* nq) {
    L = acct_layout(sv_acct_ws_bytes(c.p.b1 - c.p.b0, c.e1 - c.e0, c.c1 - c.c0), c.p.b1 - c.p.b0, c.c1 - c.c0, false,
                    c.nk, c.nq, c.ng);
    *bytes = c.bytes;
    *nq = c.nq;
    return s.d_acct.ensure(L.bytes);
  }
  void pack(const AcctChunk& c, uint8_t* hp) const { acct_pack(in, c, hp); }
  int tables(Device&, Stage& s, const AcctChunk& c, const uint8_t* d, hipStream_t st, TxDev* T) const {
    uint8_t* da = (uint8_t*)s.d_acct.p;
    const size_t nc = c.c1 - c.c0;
    const sv_acct_use U{(const uint64_t*)(d + c.o_eb), (const uint32_t*)(d + c.o_ea), (const uint64_t*)(d + c.o_cb),
                        (const uint32_t*)(d + c.o_ca), d + c.o_lvl, (const int32_t*)(d + c.o_need), T->h.nb, c.e1 - c.e0,
                        nc};
    const sv_acct_out O = acct_out(L, da, da, c.nk, c.nq, c.ng);
    SV_HIP(sv_launch_acct_count(&tab, tab_ws, &U, &O, da, st));
    SV_HIP(sv_launch_acct_fill(&tab, tab_ws, &U, &O, da, st));
    acct_tables(O, in.sig_len ? d + c.o_sl : nullptr, clamp, U.cbeg, nc, T);
    return SV_OK;
  }
};

inline int acct_slice(Device& D, const AcctIn& in, const sv_txaccounts& A, size_t B0, size_t B1, int clamp,
                      const CheckOut& out, int path) {
  return with_slot(D, [&] {
    AcctSrc src{in, A, clamp};
    return check_chunks_locked(D, src, B0, B1, out, path);
  });
}

}  // namespace
}  // namespace sv
