// The verdict journal of a device slot (include/stellar_sigverify.h
// sv_set_verdict_cache_feed): what the slot's latency lane verified, waiting to
// be inserted into the slot's verdict cache (vcache.h).  Pure host code: the
// engine (latlane.h appends, bulk.h drains) and the tests' host model
// (tests/native/vcache_feed_core.cpp, vjournal_stress.cpp) compile this file.
//
// Row       a 32-byte cache key and one verdict byte, both written by a
//           completed verify launch of this engine: nothing a caller claims.
// Bound     `cap` rows.  append() copies a batch's rows in order until the
//           journal is full; the rest of the batch is counted in `overflow` and
//           forgotten (the table then simply does not know them: a later pass
//           verifies them).  Rows whose verdict byte is not 0 or 1 are skipped:
//           they are no verdicts, and count nowhere.
// take()    swaps the filled buffers for the caller's (emptied) ones, so the
//           drain uploads rows no appender can touch; append order is journal
//           order, and the insert pass (vcache.h) is a function of that order.
// Locking   one mutex of the journal's own, held for the copy alone.  An
//           appender may hold its lane's lock, a drainer holds Device::mu; nobody
//           calls into HIP or waits for anything with the journal's mutex held.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

namespace sv {

constexpr size_t kJournalDefaultRows = 65536;         // eight of the mirror's maxBatch 8192: 2.1 MB per slot
constexpr size_t kJournalMaxRows = (size_t)1 << 24;   // (a row index stays far below a claim word's sentinel)

// The rows a take() hands over: keys 32 * rows bytes, verdicts rows bytes.
struct JournalRows {
  std::vector<uint8_t> keys, verdicts;
  size_t rows = 0;
};

class Journal {
 public:
  // Appends the leading rows of the batch that fit a journal of `cap` rows; returns how many it stored.  A
  // capacity other than the one the held rows were stored under empties the journal first.
  size_t append(const uint8_t* keys, const uint8_t* verdicts, size_t n, size_t cap) {
    std::lock_guard<std::mutex> g(mu_);
    if (cap != cap_) {
      cur_.rows = 0;
      cap_ = cap;
    }
    if (cur_.keys.size() < 32 * cap_) {
      cur_.keys.resize(32 * cap_);
      cur_.verdicts.resize(cap_);
    }
    bool clean = true;
    for (size_t i = 0; i < n && clean; ++i) clean = verdicts[i] <= 1;
    size_t stored = 0;
    if (clean) {
      stored = n < cap_ - cur_.rows ? n : cap_ - cur_.rows;
      if (stored) {
        std::memcpy(cur_.keys.data() + 32 * cur_.rows, keys, 32 * stored);
        std::memcpy(cur_.verdicts.data() + cur_.rows, verdicts, stored);
      }
      cur_.rows += stored;
      overflow_ += n - stored;
    } else {
      for (size_t i = 0; i < n; ++i) {
        if (verdicts[i] > 1) continue;
        if (cur_.rows == cap_) {
          ++overflow_;
          continue;
        }
        std::memcpy(cur_.keys.data() + 32 * cur_.rows, keys + 32 * i, 32);
        cur_.verdicts[cur_.rows++] = verdicts[i];
        ++stored;
      }
    }
    fed_ += stored;
    held_.store(cur_.rows, std::memory_order_relaxed);
    return stored;
  }

  // Rows held now (a relaxed read: a drainer that sees 0 has nothing to do).
  size_t held() const { return held_.load(std::memory_order_relaxed); }

  // The held rows into `out` (whatever it held is discarded; its buffers become the journal's empty ones).
  void take(JournalRows& out) {
    out.rows = 0;
    std::lock_guard<std::mutex> g(mu_);
    std::swap(out.keys, cur_.keys);
    std::swap(out.verdicts, cur_.verdicts);
    out.rows = cur_.rows;
    cur_.rows = 0;
    held_.store(0, std::memory_order_relaxed);
  }

  // Forgets the held rows; the counters stay.
  void drop() {
    std::lock_guard<std::mutex> g(mu_);
    cur_.rows = 0;
    held_.store(0, std::memory_order_relaxed);
  }
  // ... and the counters too, with the memory (the capacity of the cache was set).
  void reset() {
    std::lock_guard<std::mutex> g(mu_);
    cur_ = JournalRows();
    cap_ = 0;
    fed_ = overflow_ = 0;
    held_.store(0, std::memory_order_relaxed);
  }

  // fed: rows stored since the last reset; overflow: rows not stored because the journal was full.
  void counters(uint64_t* fed, uint64_t* overflow) {
    std::lock_guard<std::mutex> g(mu_);
    *fed = fed_;
    *overflow = overflow_;
  }

 private:
  std::mutex mu_;
  JournalRows cur_;
  size_t cap_ = 0;
  uint64_t fed_ = 0, overflow_ = 0;
  std::atomic<size_t> held_{0};
};

}  // namespace sv
