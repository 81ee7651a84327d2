// TEST INFRASTRUCTURE: host (g++) build of csrc/sign_core.h in the device's own field form (10 x 25.5-bit
// limbs), for tests/test_sign_cpu.py: the fixed-base multiplication on chosen scalars, against integers.
#include <cstring>
#include <mutex>
#include <vector>

#include "sign_core.h"

namespace {
std::vector<sv_u4> g_ctab;
std::once_flag g_once;
void build() {
  g_ctab.assign((size_t)SV_CB_DW / 4, sv_u4{0, 0, 0, 0});
  for (int id = 0; id < SV_CB_POS * SV_CB_ENT; ++id)
    sv_comb_bentry((uint32_t*)g_ctab.data() + (size_t)id * SV_CE_DW, id / SV_CB_ENT, id % SV_CB_ENT);
}
}  // namespace

// out[i] = encode([s_i]B), s_i < 2^253 (n x 32 bytes each way)
extern "C" void sgc_fixed_base(const uint8_t* s, size_t n, uint8_t* out) {
  std::call_once(g_once, build);
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8], enc[8];
    std::memcpy(w, s + 32 * i, 32);
    sv_fixed_base_encode(enc, w, (const uint32_t*)g_ctab.data());
    std::memcpy(out + 32 * i, enc, 32);
  }
}
