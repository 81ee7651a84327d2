// One view across slots (include/stellar_sigverify.h sv_set_verdict_cache_share): what the sharing of verified
// verdicts between device slots needs on the host -- the truncation rule, a slot's queue of pending exports and its
// counters.  Pure host code, as vjournal.h is: the engine (bulk.h exports, engine_state.h passes on) and the tests
// (tests/native/vshare_core.cpp, vshare_stress.cpp) compile this file.
//
// Export    the leading rows of the miss list of one cached launch of a slot, as an image in host memory that the
//           slot owns: keys (32 * rows bytes) followed by verdict bytes (rows) -- what Journal::append takes.  The
//           image is complete some time after the export was committed (the engine: an event behind the copy).
// Offer     share_offer(): a launch with nm misses offers min(nm, journal rows); the rest is `skipped`.
// Queue     at most kSharePending exports per slot, each in an image buffer of its own (0 .. kSharePending - 1).
//           reserve() hands the exporter a free buffer or refuses (every buffer pending: the launch skips its
//           export and counts its rows as skipped -- it never waits); commit() queues the export; cancel() gives
//           the buffer back.  One exporter at a time per queue (the engine: under the slot's Device::mu).
// pass()    takes the queue's exports in order: ready(buf, wait) says whether the head's image is complete (> 0),
//           not yet (0) or lost (< 0: forgotten); a complete one goes to sink(image, rows) -- the appends to the
//           other slots' journals -- and its buffer is free again.  One passer at a time per queue (pass_mu_), so
//           every journal receives an exporter's rows in export order.  A passer that must not wait (a cached
//           launch, a lookup, the stats) gives up when another one is at work or the head is not complete; one
//           that has to see everything committed before its call (sv_verdict_cache_sync) waits for both.
// drop()    marks what is pending as forgotten: its rows reach no journal, its buffers come back through pass().
// Locking   mu_ is a leaf: held for the queue's own words, never across ready() or sink().  pass_mu_ is held
//           across them; under it nothing takes a Device::mu.  Order: Device::mu -> pass_mu_ -> mu_ / a journal's.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <deque>
#include <mutex>

namespace sv {

constexpr int kSharePending = 4;

// The rows of a launch with nm misses that are offered at a journal capacity of cap rows.
inline size_t share_offer(size_t nm, size_t cap) { return nm < cap ? nm : cap; }
// The bytes of an export image of `rows` rows, and where its verdict bytes start.
inline size_t share_image_bytes(size_t rows) { return 33 * rows; }
inline size_t share_image_verdicts(size_t rows) { return 32 * rows; }
// Pinned memory a slot may hold for exports at a journal capacity of cap rows: every buffer a whole page multiple.
constexpr size_t kSharePage = 4096;
inline size_t share_buf_bytes(size_t rows) { return (share_image_bytes(rows) + kSharePage - 1) / kSharePage * kSharePage; }
inline size_t share_pinned_bound(size_t cap) { return (size_t)kSharePending * share_buf_bytes(cap); }

class ShareQueue {
 public:
  // A free buffer for an export of a launch with nm misses, rows of them offered (share_offer); -1: none is free,
  // and the nm rows are counted as skipped.  With a buffer, the nm - rows rows beyond the offer are.
  int reserve(size_t nm, size_t rows) {
    std::lock_guard<std::mutex> g(mu_);
    for (int b = 0; b < kSharePending; ++b)
      if (!busy_[b]) {
        busy_[b] = true;
        skipped_ += nm - rows;
        return b;
      }
    skipped_ += nm;
    return -1;
  }
  // The reserved buffer back: nothing was exported, the rows count as skipped.
  void cancel(int buf, size_t rows) {
    std::lock_guard<std::mutex> g(mu_);
    busy_[buf] = false;
    skipped_ += rows;
  }
  // The export is on its way into image (complete once ready() says so).
  void commit(int buf, const uint8_t* image, size_t rows) {
    std::lock_guard<std::mutex> g(mu_);
    pending_.push_back(Export{image, rows, buf, false});
    out_ += rows;
  }
  // Rows offered without an export of the queue's own (SV_VC_SHARE_FEED: the lane's rows go out at once).
  void count_out(size_t rows) {
    std::lock_guard<std::mutex> g(mu_);
    out_ += rows;
  }

  size_t pending() {
    std::lock_guard<std::mutex> g(mu_);
    return pending_.size();
  }

  // (see above) -> exports handed to sink.  wait: for another passer, and for the exports pending at the call.
  template <class Ready, class Sink>
  size_t pass(bool wait, Ready ready, Sink sink) {
    std::unique_lock<std::mutex> pl(pass_mu_, std::defer_lock);
    if (wait) pl.lock();
    else if (!pl.try_lock()) return 0;
    size_t todo, passed = 0;
    {
      std::lock_guard<std::mutex> g(mu_);
      todo = pending_.size();
    }
    for (; todo; --todo) {
      Export e;
      {
        std::lock_guard<std::mutex> g(mu_);
        e = pending_.front();  // (it stays queued, its buffer busy, until its rows are out)
      }
      const int r = ready(e.buf, wait);
      if (r == 0) break;
      if (r > 0 && !e.dropped) {
        sink(e.image, e.rows);
        ++passed;
      }
      std::lock_guard<std::mutex> g(mu_);
      pending_.pop_front();
      busy_[e.buf] = false;
    }
    return passed;
  }

  void drop() {
    std::lock_guard<std::mutex> pl(pass_mu_);
    std::lock_guard<std::mutex> g(mu_);
    for (Export& e : pending_) e.dropped = true;
  }
  // ... and the counters too; every pending export is complete or lost (the engine: its stream is drained).
  void reset() {
    std::lock_guard<std::mutex> pl(pass_mu_);
    std::lock_guard<std::mutex> g(mu_);
    pending_.clear();
    for (bool& b : busy_) b = false;
    out_ = skipped_ = 0;
  }

  void counters(uint64_t* out, uint64_t* skipped) {
    std::lock_guard<std::mutex> g(mu_);
    *out = out_;
    *skipped = skipped_;
  }

 private:
  struct Export {
    const uint8_t* image;
    size_t rows;
    int buf;
    bool dropped;
  };
  std::mutex pass_mu_, mu_;
  std::deque<Export> pending_;
  bool busy_[kSharePending] = {false, false, false, false};
  uint64_t out_ = 0, skipped_ = 0;
};

}  // namespace sv
