// TEST INFRASTRUCTURE: csrc/vshare.h over csrc/vjournal.h under contention, as a stand-alone host program
// (tests/test_vshare_model_cpu.py builds and runs it; it is also the program to build with -fsanitize=thread).
// Four exporter threads, a queue of pending exports each, export batches of numbered rows and pass on whatever is
// complete -- of every queue, as a cached launch does, without waiting -- to three journals, while three drainer
// threads loop on take().  At the end: per exporter every journal received its rows in export order (batch by
// batch, a batch's stored rows its leading ones); no row is torn; every exporter's offered rows are its
// shared_out plus its skipped ones; and every journal's fed + overflow is the sum of all shared_out.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../stellar-core_amd/csrc/vjournal.h"
#include "../../stellar-core_amd/csrc/vshare.h"

namespace {

constexpr int kExporters = 4;
constexpr int kJournals = 3;
constexpr int kBatches = 600;
constexpr size_t kCap = 48;  // journal rows: some batches are truncated, some appends overflow

size_t batch_len(int t, int b) { return 1 + (size_t)((t * 29 + b * 11) % 64); }

void put_key(uint8_t* key, uint32_t t, uint32_t b, uint32_t r) {
  std::memset(key, 0, 32);
  std::memcpy(key, &t, 4);
  std::memcpy(key + 4, &b, 4);
  std::memcpy(key + 8, &r, 4);
  key[31] = (uint8_t)(t ^ b ^ r);
}

struct Exporter {
  sv::ShareQueue q;
  std::vector<uint8_t> image[sv::kSharePending];
  std::atomic<bool> complete[sv::kSharePending];
  uint64_t offered = 0, committed = 0;
};

}  // namespace

int main() {
  static Exporter ex[kExporters];
  static sv::Journal journal[kJournals];
  for (auto& e : ex)
    for (auto& c : e.complete) c.store(false);
  std::atomic<int> running{kExporters};

  auto pass_all = [&](bool wait) {
    for (int t = 0; t < kExporters; ++t) {
      Exporter& e = ex[t];
      e.q.pass(
          wait, [&](int b, bool) -> int { return e.complete[b].load(std::memory_order_acquire) ? 1 : 0; },
          [&](const uint8_t* image, size_t rows) {
            for (auto& j : journal) j.append(image, image + sv::share_image_verdicts(rows), rows, kCap);
          });
    }
  };

  std::vector<std::thread> exporters;
  for (int t = 0; t < kExporters; ++t)
    exporters.emplace_back([&, t] {
      Exporter& e = ex[t];
      for (int b = 0; b < kBatches; ++b) {
        const size_t nm = batch_len(t, b), rows = sv::share_offer(nm, kCap - 16);  // (the longest are truncated)
        e.offered += nm;
        pass_all(false);
        const int buf = e.q.reserve(nm, rows);
        if (buf < 0) continue;  // every buffer pending: skipped, never waited for
        e.image[buf].resize(sv::share_image_bytes(rows));
        for (size_t r = 0; r < rows; ++r) {
          put_key(e.image[buf].data() + 32 * r, (uint32_t)t, (uint32_t)b, (uint32_t)r);
          e.image[buf][sv::share_image_verdicts(rows) + r] = (uint8_t)((t + b + r) & 1);
        }
        e.complete[buf].store(false, std::memory_order_relaxed);
        e.q.commit(buf, e.image[buf].data(), rows);
        e.committed += rows;
        if (b & 1) std::this_thread::yield();  // (the copy takes its time)
        e.complete[buf].store(true, std::memory_order_release);
      }
      running.fetch_sub(1);
    });

  // per journal and exporter: the last (batch, row) seen, and the rows taken
  struct Seen {
    int64_t batch = -1, row = -1;
    uint64_t rows = 0;
  };
  static Seen seen[kJournals][kExporters];
  std::atomic<bool> ok{true};
  std::atomic<bool> stop{false};
  std::vector<std::thread> drainers;
  for (int j = 0; j < kJournals; ++j)
    drainers.emplace_back([&, j] {
      sv::JournalRows rows;
      auto collect = [&] {
        journal[j].take(rows);
        if (rows.rows > kCap) ok = false;
        for (size_t i = 0; i < rows.rows; ++i) {
          const uint8_t* k = rows.keys.data() + 32 * i;
          uint32_t t, b, r;
          std::memcpy(&t, k, 4);
          std::memcpy(&b, k + 4, 4);
          std::memcpy(&r, k + 8, 4);
          if (t >= (uint32_t)kExporters || b >= (uint32_t)kBatches || k[31] != (uint8_t)(t ^ b ^ r) ||
              rows.verdicts[i] != (uint8_t)((t + b + r) & 1)) {
            std::printf("a torn row came out of journal %d\n", j);
            ok = false;
            continue;
          }
          Seen& s = seen[j][t];
          // export order: a later batch starts at its row 0, the same batch continues with the next row
          const bool next = ((int64_t)b > s.batch && r == 0) || ((int64_t)b == s.batch && (int64_t)r == s.row + 1);
          if (!next) ok = false;
          s.batch = b;
          s.row = r;
          ++s.rows;
        }
      };
      while (!stop.load()) collect();
      collect();
    });

  for (auto& th : exporters) th.join();
  pass_all(true);  // (every export is complete by now: the exporters are done)
  stop.store(true);
  for (auto& th : drainers) th.join();

  uint64_t all_out = 0, all_skipped = 0;
  for (auto& e : ex) {
    uint64_t out = 0, skipped = 0;
    e.q.counters(&out, &skipped);
    if (out != e.committed || out + skipped != e.offered || e.q.pending() != 0) ok = false;
    all_out += out;
    all_skipped += skipped;
  }
  uint64_t fed_all = 0, over_all = 0;
  for (int j = 0; j < kJournals; ++j) {
    uint64_t fed = 0, overflow = 0, taken = 0;
    journal[j].counters(&fed, &overflow);
    for (int t = 0; t < kExporters; ++t) taken += seen[j][t].rows;
    if (fed + overflow != all_out || taken != fed || journal[j].held() != 0) ok = false;
    fed_all += fed;
    over_all += overflow;
  }
  std::printf("vshare stress: shared_out %llu skipped %llu; over %d journals fed %llu overflow %llu: %s\n",
              (unsigned long long)all_out, (unsigned long long)all_skipped, kJournals, (unsigned long long)fed_all,
              (unsigned long long)over_all, ok.load() ? "ok" : "FAILED");
  return ok.load() ? 0 : 1;
}
