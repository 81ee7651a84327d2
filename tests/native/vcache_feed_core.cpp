// TEST INFRASTRUCTURE: the verdict cache's feed on the host, without the engine
// around it -- csrc/vjournal.h as it is and the insert pass of csrc/vcache.h
// (sv_vc_feed_slot, sv_vc_store) in the order the two feed kernels of
// sv_vcache.hip run it: claim over every row (the table only read), then store
// (the winners), with the same three counters.  The model the tests predict the
// device table with (tests/vcache_feed_model.py; tests/test_vcache_feed_cpu.py
// compares it with a Python restatement, tests/test_gpu_vcache_feed.py the device
// with it).
#include <cstdint>
#include <vector>

#include "../../stellar-core_amd/csrc/vcache.h"
#include "../../stellar-core_amd/csrc/vjournal.h"

extern "C" {

// keys: n x 8 words, verdict: n bytes; counters: present | inserted | dropped, added to.
// claim: 4 * sets words, SV_VC_UNCLAIMED on entry and on return.
void vfm_insert_pass(void* tab_, uint32_t* claim, uint64_t sets, const uint32_t* keys, const uint8_t* verdict,
                     uint64_t n, uint64_t* counters) {
  sv_vc_entry* tab = (sv_vc_entry*)tab_;
  std::vector<uint32_t> slot(n);
  for (uint64_t j = 0; j < n; ++j) {
    bool present;
    slot[j] = sv_vc_feed_slot(tab, sets, keys + 8 * j, verdict[j], &present);
    if (present) ++counters[0];
    if (slot[j] != SV_VC_NO_SLOT && (uint32_t)j < claim[slot[j]]) claim[slot[j]] = (uint32_t)j;
  }
  for (uint64_t j = 0; j < n; ++j) {
    const uint32_t s = slot[j];
    if (s == SV_VC_NO_SLOT) continue;
    if (claim[s] == (uint32_t)j) {
      sv_vc_store(tab, s, keys + 8 * j, verdict[j]);
      claim[s] = SV_VC_UNCLAIMED;
      ++counters[1];
    } else {
      ++counters[2];
    }
  }
}

void* vfm_journal_new(void) { return new sv::Journal(); }
void vfm_journal_free(void* j) { delete (sv::Journal*)j; }
uint64_t vfm_journal_append(void* j, const uint8_t* keys, const uint8_t* verdicts, uint64_t n, uint64_t cap) {
  return ((sv::Journal*)j)->append(keys, verdicts, n, cap);
}
uint64_t vfm_journal_held(void* j) { return ((sv::Journal*)j)->held(); }
void vfm_journal_drop(void* j) { ((sv::Journal*)j)->drop(); }
void vfm_journal_reset(void* j) { ((sv::Journal*)j)->reset(); }
void vfm_journal_counters(void* j, uint64_t* out2) { ((sv::Journal*)j)->counters(out2, out2 + 1); }

// take() and the insert pass over the taken rows; returns how many rows were taken
uint64_t vfm_journal_drain(void* j, void* tab, uint32_t* claim, uint64_t sets, uint64_t* counters) {
  sv::JournalRows rows;
  ((sv::Journal*)j)->take(rows);
  vfm_insert_pass(tab, claim, sets, (const uint32_t*)rows.keys.data(), rows.verdicts.data(), rows.rows, counters);
  return rows.rows;
}

}  // extern "C"
