// TEST INFRASTRUCTURE: csrc/vcache.h instantiated for the host (g++: SV_HD =
// static inline), without the engine around it -- the model the tests predict
// the device table with (tests/test_vcache_cpu.py compares it with a Python
// restatement of the policy, tests/test_gpu_vcache.py the device with it).  A
// pass runs the stages of sv_vcache.hip in their order, each over the whole
// batch before the next one starts, as the kernel boundaries make them run:
// probe (every lookup sees the table as the pass found it), claim (min of the
// item indices per candidate slot), store (the winners), with the same counters.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../stellar-core_amd/csrc/vcache.h"

extern "C" {

uint64_t vcm_entry_bytes(void) { return sizeof(sv_vc_entry); }
uint32_t vcm_state(int verdict) { return verdict ? SV_VC_HOLDS1 : SV_VC_HOLDS0; }

int vcm_lookup(const void* tab, uint64_t sets, const uint32_t* key) {
  return sv_vc_lookup((const sv_vc_entry*)tab, sets, key);
}

uint64_t vcm_candidate(const void* tab, uint64_t sets, const uint32_t* key) {
  return sv_vc_candidate((const sv_vc_entry*)tab, sets, key);
}

// keys: n x 8 words; verify[i]: the verdict byte a verification of item i gives; hit / verdict: n bytes out;
// counters: hits | inserted | dropped, added to.  claim: 4 * sets words, SV_VC_UNCLAIMED on entry and on return.
void vcm_pass(void* tab_, uint32_t* claim, uint64_t sets, const uint32_t* keys, uint64_t n, const uint8_t* verify,
              uint8_t* hit, uint8_t* verdict, uint64_t* counters) {
  sv_vc_entry* tab = (sv_vc_entry*)tab_;
  std::vector<uint32_t> miss;
  for (uint64_t i = 0; i < n; ++i) {
    const int v = sv_vc_lookup(tab, sets, keys + 8 * i);
    hit[i] = v >= 0;
    if (v >= 0) {
      verdict[i] = (uint8_t)v;
      ++counters[0];
    } else {
      miss.push_back((uint32_t)i);
    }
  }
  std::vector<uint32_t> slot(miss.size());
  for (size_t j = 0; j < miss.size(); ++j) {
    const uint32_t i = miss[j];
    verdict[i] = verify[i];
    slot[j] = SV_VC_NO_SLOT;
    if (verify[i] <= 1) {
      slot[j] = (uint32_t)sv_vc_candidate(tab, sets, keys + 8 * i);
      if (i < claim[slot[j]]) claim[slot[j]] = i;
    }
  }
  for (size_t j = 0; j < miss.size(); ++j) {
    const uint32_t i = miss[j], s = slot[j];
    if (s != SV_VC_NO_SLOT && claim[s] == i) {
      sv_vc_store(tab, s, keys + 8 * i, verify[i]);
      claim[s] = SV_VC_UNCLAIMED;
      ++counters[1];
    } else {
      ++counters[2];
    }
  }
}

}  // extern "C"
