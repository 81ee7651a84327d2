// TEST INFRASTRUCTURE: stand-alone driver of csrc/txresult.h instantiated for
// the host (g++: SV_HD = static inline), without the engine around it -- meant
// to be built with -fsanitize=address,undefined and run directly
// (tests/test_txresults_cpu.py builds it from this file alone).  Every array
// lives in a heap block of exactly its size, so a read or write past a clamp
// is an ASan report.  The fold is compared with plain loops written out here
// (not txresult.h), over random bodies, over the quad's split of a body's checks
// (sv_txresult_step in any lane order), and over CSR arrays that end past their
// tables.  Prints "txresult_core ok" and returns 0, or the first failed check
// and 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../stellar-core_amd/csrc/txresult.h"

namespace {

int g_failed = 0;
#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
      g_failed = 1;                                                  \
    }                                                                \
  } while (0)

// exact-size heap copies (no slack behind any array)
template <class T>
T* exact(const std::vector<T>& v) {
  T* p = (T*)std::malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
  if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

struct Set {
  std::vector<uint64_t> cb, sb, used;
  std::vector<uint8_t> ok, role, flags;
  uint64_t nb = 0, nc = 0, ns = 0;
};

// the definition with plain loops; cb / sb clamped as the header says it clamps
void reference(const Set& s, bool roles, bool flags, std::vector<uint8_t>* code, std::vector<uint32_t>* fail) {
  auto mn = [](uint64_t a, uint64_t b) { return a < b ? a : b; };
  code->assign(s.nb, 0);
  fail->assign(s.nb, 0xFFFFFFFFu);
  for (uint64_t t = 0; t < s.nb; ++t) {
    const uint64_t c1 = mn(s.cb[t + 1], s.nc), c0 = mn(s.cb[t], c1);
    const uint64_t s1 = mn(s.sb[t + 1], s.ns), s0 = mn(s.sb[t], s1);
    uint64_t marks = 0;
    bool failed = false;
    for (uint64_t c = c0; c < c1; ++c) {
      marks |= s.used[c];
      if (s.ok[c] != 1 && !failed) {
        failed = true;
        (*fail)[t] = (uint32_t)(c - c0);
        const unsigned r = roles ? s.role[c] : 0u;
        (*code)[t] = r == 0 ? 1 : 2;
      }
    }
    if (failed) continue;
    const uint64_t n = mn(s1 - s0, 64);
    const uint64_t want = n >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << n) - 1);
    const unsigned f = flags ? s.flags[t] : 0u;
    if ((marks & want) != want && !(f & 1u)) (*code)[t] = 3;
  }
}

Set random_set(std::mt19937_64& rng, uint64_t nb, bool wild) {
  Set s;
  s.nb = nb;
  s.cb.push_back(0);
  s.sb.push_back(0);
  static const int checks[] = {0, 1, 1, 2, 3, 3, 4, 5, 9, 130};
  static const int sigs[] = {0, 1, 1, 2, 3, 63, 64, 70};
  for (uint64_t t = 0; t < nb; ++t) {
    const int k = checks[rng() % 10], n = sigs[rng() % 8];
    const int mode = (int)(rng() % 4);  // 0: all pass and all used, 1: all pass, 2, 3: random
    for (int i = 0; i < k; ++i) {
      s.ok.push_back(mode < 2 ? 1 : (uint8_t)(rng() % 8 < 6 ? 1 : (rng() % 2) * 2));
      s.used.push_back(mode == 0 ? ~(uint64_t)0 : (rng() & rng()) | (rng() % 3 ? 0 : ((uint64_t)1 << (n ? (n - 1) % 64 : 0))));
      s.role.push_back(wild ? (uint8_t)(rng() % 9) : (uint8_t)(rng() % 2));
    }
    s.flags.push_back(wild ? (uint8_t)(rng() % 256) : (uint8_t)(rng() % 4 == 0));
    s.cb.push_back(s.ok.size());
    s.sb.push_back(s.sb.back() + n);
  }
  s.nc = s.ok.size();
  s.ns = s.sb.back();
  return s;
}

void run(const Set& s, bool roles, bool flags, const char* what) {
  std::vector<uint8_t> want_code;
  std::vector<uint32_t> want_fail;
  reference(s, roles, flags, &want_code, &want_fail);
  uint64_t *cb = exact(s.cb), *sb = exact(s.sb), *used = exact(s.used);
  uint8_t *ok = exact(s.ok), *role = exact(s.role), *fl = exact(s.flags);
  const sv_txresult_in I{cb, sb, ok, used, roles ? role : nullptr, flags ? fl : nullptr, s.nb, s.nc, s.ns};
  size_t seen[4] = {0, 0, 0, 0};
  for (uint64_t t = 0; t < s.nb; ++t) {
    uint32_t fail = 7;
    const uint8_t code = sv_txresult_body(I, t, &fail);
    if (code != want_code[t] || fail != want_fail[t]) {
      std::printf("FAILED %s: body %llu: code %u fail %u, expected %u %u\n", what, (unsigned long long)t, code, fail,
                  want_code[t], want_fail[t]);
      g_failed = 1;
      break;
    }
    ++seen[code & 3];
    // the quad's split: four lanes striding over the checks, from the last lane to the first, then joined
    uint64_t c0, c1, u = 0;
    uint32_t f = SV_TXRESULT_NONE;
    sv_txresult_checks(I, t, &c0, &c1);
    for (int lane = 3; lane >= 0; --lane) {
      uint64_t lu = 0;
      uint32_t lf = SV_TXRESULT_NONE;
      for (uint64_t c = c0 + (uint64_t)lane; c < c1; c += 4) sv_txresult_step(I, c0, c, &lf, &lu);
      f = lf < f ? lf : f;
      u |= lu;
    }
    CHECK(f == fail && sv_txresult_code(I, t, c0, f, u) == code);
  }
  if (s.nb >= 500 && roles && flags) CHECK(seen[0] && seen[1] && seen[2] && seen[3]);
  std::free(cb);
  std::free(sb);
  std::free(used);
  std::free(ok);
  std::free(role);
  std::free(fl);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20251);
  for (uint64_t nb : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)600}) {
    const Set s = random_set(rng, nb, false);
    run(s, true, true, "valid");
    run(s, false, true, "no roles");
    run(s, true, false, "no flags");
    run(s, false, false, "neither");
  }
  // roles above 1 read as OP, unknown flag bits are ignored
  run(random_set(rng, 600, true), true, true, "unvalidated roles and flags");
  // CSR arrays that end past their tables: the arrays keep their exact sizes, the ranges are clamped
  {
    Set s = random_set(rng, 300, false);
    s.cb[s.nb] += 9;
    s.sb[s.nb] += 1000;
    s.cb[s.nb / 2] = s.nc + 5;  // (not monotonic: an empty range after the clamp)
    s.sb[s.nb / 3] = s.ns + 1;
    run(s, true, true, "unvalidated CSR arrays");
  }
  // by hand: 64 signatures need all 64 marks, 70 signatures read as 64; a value that is neither 0 nor 1 fails
  {
    Set s;
    s.nb = 4;
    s.cb = {0, 1, 2, 3, 4};
    s.sb = {0, 64, 134, 135, 136};
    s.ok = {1, 1, 2, 1};
    s.used = {~(uint64_t)0 >> 1, ~(uint64_t)0, 1, 1};
    s.role = {0, 0, 1, 0};
    s.flags = {0, 0, 0, 0};
    s.nc = 4;
    s.ns = 136;
    std::vector<uint8_t> code;
    std::vector<uint32_t> fail;
    reference(s, true, true, &code, &fail);
    CHECK(code == (std::vector<uint8_t>{3, 0, 2, 0}));
    run(s, true, true, "by hand");
  }
  if (g_failed) return 1;
  std::printf("txresult_core ok\n");
  return 0;
}
