// TEST INFRASTRUCTURE: csrc/vjournal.h under contention, as a stand-alone host
// program (tests/test_vcache_feed_cpu.py builds it with -fsanitize=thread and
// runs it).  Four appender threads offer batches of numbered rows while one
// thread loops on take().  At the end every offered row was either taken exactly
// once or counted as overflow; the rows a batch stored are its leading rows, in
// order and contiguous in the journal; and the journal's counters say the same.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <thread>
#include <utility>
#include <vector>

#include "../../stellar-core_amd/csrc/vjournal.h"

namespace {

constexpr int kThreads = 4;
constexpr int kBatches = 400;
constexpr size_t kCap = 96;

size_t batch_len(int t, int b) { return 1 + (size_t)((t * 31 + b * 7) % 40); }

void put_key(uint8_t* key, uint32_t t, uint32_t b, uint32_t r) {
  std::memset(key, 0, 32);
  std::memcpy(key, &t, 4);
  std::memcpy(key + 4, &b, 4);
  std::memcpy(key + 8, &r, 4);
  key[31] = (uint8_t)(t ^ b ^ r);
}

}  // namespace

int main() {
  sv::Journal journal;
  std::atomic<int> running{kThreads};
  std::vector<std::vector<size_t>> stored(kThreads, std::vector<size_t>(kBatches, 0));
  std::vector<std::thread> appenders;
  for (int t = 0; t < kThreads; ++t)
    appenders.emplace_back([&, t] {
      std::vector<uint8_t> keys, verdicts;
      for (int b = 0; b < kBatches; ++b) {
        const size_t n = batch_len(t, b);
        keys.resize(32 * n);
        verdicts.resize(n);
        for (size_t r = 0; r < n; ++r) {
          put_key(keys.data() + 32 * r, (uint32_t)t, (uint32_t)b, (uint32_t)r);
          verdicts[r] = (uint8_t)((t + b + r) & 1);
        }
        stored[t][b] = journal.append(keys.data(), verdicts.data(), n, kCap);
        if ((b & 15) == 0) std::this_thread::yield();
      }
      running.fetch_sub(1);
    });
  // (thread, batch) -> the rows taken of it, in the order they came out
  std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> taken;
  uint64_t taken_rows = 0, takes = 0;
  bool ok = true;
  sv::JournalRows rows;
  auto collect = [&] {
    journal.take(rows);
    ++takes;
    if (rows.rows > kCap) ok = false;
    for (size_t i = 0; i < rows.rows; ++i) {
      const uint8_t* k = rows.keys.data() + 32 * i;
      uint32_t t, b, r;
      std::memcpy(&t, k, 4);
      std::memcpy(&b, k + 4, 4);
      std::memcpy(&r, k + 8, 4);
      if (t >= (uint32_t)kThreads || b >= (uint32_t)kBatches || k[31] != (uint8_t)(t ^ b ^ r) ||
          rows.verdicts[i] != (uint8_t)((t + b + r) & 1)) {
        std::printf("a torn row came out of the journal\n");
        ok = false;
        continue;
      }
      auto& v = taken[{t, b}];
      // a batch's rows are stored by one append, contiguously: they come out together, in order
      if (!v.empty() && (i == 0 || v.back() + 1 != r)) ok = false;
      v.push_back(r);
      ++taken_rows;
    }
  };
  while (running.load() > 0) collect();
  for (auto& th : appenders) th.join();
  collect();
  uint64_t offered = 0, kept = 0;
  for (int t = 0; t < kThreads; ++t)
    for (int b = 0; b < kBatches; ++b) {
      offered += batch_len(t, b);
      kept += stored[t][b];
      auto it = taken.find({(uint32_t)t, (uint32_t)b});
      const size_t got = it == taken.end() ? 0 : it->second.size();
      if (got != stored[t][b]) ok = false;  // every stored row taken exactly once ...
      for (size_t r = 0; r < got; ++r)
        if (it->second[r] != r) ok = false;  // ... and they are the batch's leading rows
    }
  uint64_t fed = 0, overflow = 0;
  journal.counters(&fed, &overflow);
  if (fed != kept || fed != taken_rows || fed + overflow != offered || journal.held() != 0) ok = false;
  std::printf("vjournal stress: offered %llu stored %llu overflow %llu in %llu takes: %s\n",
              (unsigned long long)offered, (unsigned long long)fed, (unsigned long long)overflow,
              (unsigned long long)takes, ok ? "ok" : "FAILED");
  return ok ? 0 : 1;
}
