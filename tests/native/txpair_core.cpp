// TEST INFRASTRUCTURE: stand-alone driver of the hinted tx-body host code --
// the chunk planner, the packer and the slicer of csrc/host_image.h and the
// engine's CPU form sv_ed25519_verify_txbodies_hinted_cpu (csrc/sv_cpu.cpp) --
// meant to be built with -fsanitize=address,undefined and run directly
// (tests/test_txpairs_cpu.py builds it from this file and sv_cpu.cpp).  Every
// packed image lives in a heap block of exactly the planned size, so a write
// past the plan is an ASan report; the checks below compare the image and the
// CPU form's pairs with a plain double loop.  Prints "txpair_core ok" and
// returns 0, or the first failed check and 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/stellar_sigverify.h"
#include "../../stellar-core_amd/csrc/host_image.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

namespace {
struct Set {
  std::vector<uint8_t> bodies, kind, hint, sig, key;
  std::vector<uint64_t> off, sb, kb;
  std::vector<uint32_t> len;
  size_t nb = 0;
};

Set make(size_t nb, unsigned seed) {
  std::mt19937 rng(seed);
  Set s;
  s.nb = nb;
  s.sb.push_back(0);
  s.kb.push_back(0);
  for (size_t t = 0; t < nb; ++t) {
    const uint32_t l = t % 11 == 0 ? 0 : rng() % 300;
    s.off.push_back(s.bodies.size());
    s.len.push_back(l);
    s.kind.push_back((uint8_t)(rng() % 3));
    for (uint32_t i = 0; i < l; ++i) s.bodies.push_back((uint8_t)rng());
    const size_t ns = t % 9 == 0 ? 20 : rng() % 3, nk = t % 9 == 0 ? 20 : rng() % 4;
    // tails from a small alphabet, so hints match several keys and none
    for (size_t i = 0; i < nk; ++i) {
      for (int b = 0; b < 28; ++b) s.key.push_back((uint8_t)rng());
      const uint8_t x = (uint8_t)(rng() % 3);
      for (int b = 0; b < 4; ++b) s.key.push_back(x);
    }
    for (size_t i = 0; i < ns; ++i) {
      const uint8_t x = (uint8_t)(rng() % 4);
      for (int b = 0; b < 4; ++b) s.hint.push_back(x);
      for (int b = 0; b < 64; ++b) s.sig.push_back((uint8_t)rng());
    }
    s.sb.push_back(s.hint.size() / 4);
    s.kb.push_back(s.key.size() / 32);
  }
  s.bodies.push_back(0);  // (never empty)
  return s;
}

int run(size_t nb, unsigned seed) {
  using namespace sv;
  const Set s = make(nb, seed);
  const uint8_t nid[32] = {7};
  const HintIn in{nid,          s.bodies.data(), s.off.data(), s.len.data(), s.kind.data(), nb,
                  s.sb.data(), s.hint.data(),   s.sig.data(), s.kb.data(),  s.key.data()};
  // planner and packer under several bounds
  const size_t bounds[][3] = {{1u << 18, 1u << 18, 64u << 20}, {25, 1u << 18, 64u << 20}, {1u << 18, 7, 64u << 20},
                              {1u << 18, 1u << 18, 512},      {1, 1, 16}};
  for (auto const& b : bounds) {
    const std::vector<PairChunk> plan = pair_plan(in, 0, nb, b[0], b[1], b[2]);
    size_t next = 0;
    for (const PairChunk& c : plan) {
      CHECK(c.b0 == next && c.b1 > c.b0 && c.b1 <= nb);
      CHECK(c.s0 == s.sb[c.b0] && c.s1 == s.sb[c.b1] && c.k0 == s.kb[c.b0] && c.k1 == s.kb[c.b1]);
      const size_t m = c.s1 - c.s0, q = c.k1 - c.k0, k = c.b1 - c.b0;
      if (k > 1) CHECK(m <= b[0] && q <= b[1] && c.body_bytes <= b[2]);
      CHECK(c.o_sig % 16 == 0 && c.o_hint % 16 == 0 && c.o_off % 16 == 0 && c.o_body % 16 == 0);
      uint8_t* h = (uint8_t*)std::malloc(c.bytes);  // exactly the plan: ASan guards its end
      CHECK(h != nullptr);
      pair_pack(in, c, h);
      CHECK(q == 0 || std::memcmp(h, s.key.data() + 32 * c.k0, 32 * q) == 0);
      CHECK(m == 0 || std::memcmp(h + c.o_sig, s.sig.data() + 64 * c.s0, 64 * m) == 0);
      CHECK(m == 0 || std::memcmp(h + c.o_hint, s.hint.data() + 4 * c.s0, 4 * m) == 0);
      const uint64_t* po = (const uint64_t*)(h + c.o_off);
      const uint64_t* ps = (const uint64_t*)(h + c.o_sb);
      const uint64_t* pk = (const uint64_t*)(h + c.o_kb);
      const uint32_t* pl = (const uint32_t*)(h + c.o_len);
      CHECK(ps[0] == 0 && pk[0] == 0 && ps[k] == m && pk[k] == q);
      for (size_t i = 0; i < k; ++i) {
        CHECK(ps[i + 1] == s.sb[c.b0 + i + 1] - c.s0 && pk[i + 1] == s.kb[c.b0 + i + 1] - c.k0);
        CHECK(pl[i] == s.len[c.b0 + i] && h[c.o_kind + i] == s.kind[c.b0 + i] && po[i] % 16 == 0);
        CHECK(c.o_body + po[i] + pl[i] <= c.bytes);
        CHECK(pl[i] == 0 || std::memcmp(h + c.o_body + po[i], s.bodies.data() + s.off[c.b0 + i], pl[i]) == 0);
      }
      std::free(h);
      next = c.b1;
    }
    CHECK(next == nb);
  }
  // slicer: monotone body edges, whole range
  for (size_t G = 1; G <= 5; ++G) {
    const std::vector<size_t> cut = pair_slices(s.sb.data(), nb, G);
    CHECK(cut.size() == G + 1 && cut[0] == 0 && cut[G] == nb);
    for (size_t g = 0; g < G; ++g) CHECK(cut[g] <= cut[g + 1]);
  }
  // the CPU form against a double loop
  std::vector<uint64_t> wb{0};
  std::vector<uint32_t> ws, wk;
  for (size_t t = 0; t < nb; ++t) {
    for (uint64_t i = s.sb[t]; i < s.sb[t + 1]; ++i)
      for (uint64_t k = s.kb[t]; k < s.kb[t + 1]; ++k)
        if (std::memcmp(&s.hint[4 * i], &s.key[32 * k + 28], 4) == 0) {
          ws.push_back((uint32_t)i);
          wk.push_back((uint32_t)k);
        }
    wb.push_back(ws.size());
  }
  const size_t np = ws.size(), ns = s.hint.size() / 4, nk = s.key.size() / 32;
  CHECK(sv_txbodies_pair_bound(s.sb.data(), s.kb.data(), nb) >= np);
  auto call = [&](size_t cap, uint64_t* pb, uint32_t* ps, uint32_t* pk, uint8_t* pv, size_t* n, uint8_t* dig) {
    return sv_ed25519_verify_txbodies_hinted_cpu(nid, s.bodies.data(), s.off.data(), s.len.data(), s.kind.data(), nb,
                                                 s.sb.data(), s.hint.data(), s.sig.data(), ns, s.kb.data(),
                                                 s.key.data(), nk, cap, pb, ps, pk, pv, n, dig, 2);
  };
  {
    // arrays of exactly np entries
    std::vector<uint64_t> pb(nb + 1);
    uint32_t* ps = (uint32_t*)std::malloc(4 * np + 1);
    uint32_t* pk = (uint32_t*)std::malloc(4 * np + 1);
    uint8_t* pv = (uint8_t*)std::malloc(np + 1);
    std::vector<uint8_t> dig(32 * nb + 1);
    size_t n = ~(size_t)0;
    CHECK(call(np, pb.data(), ps, pk, pv, &n, dig.data()) == SV_OK);
    CHECK(n == np && pb == wb);
    CHECK(np == 0 || (std::memcmp(ps, ws.data(), 4 * np) == 0 && std::memcmp(pk, wk.data(), 4 * np) == 0));
    for (size_t i = 0; i < np; ++i) CHECK(pv[i] <= 1);
    if (np) {
      n = 0;
      CHECK(call(np - 1, pb.data(), ps, pk, pv, &n, nullptr) == SV_ERR_PAIR_CAP);
      CHECK(n == np);
    }
    std::free(ps);
    std::free(pk);
    std::free(pv);
  }
  return 0;
}
}  // namespace

int main() {
  if (run(1, 1) || run(40, 2) || run(257, 3)) return 1;
  // zero pairs, pair_cap == 0, null pair arrays
  {
    const uint8_t nid[32] = {0}, body[4] = {1, 2, 3, 4}, kind[1] = {1};
    const uint64_t off[1] = {0}, sb[2] = {0, 0}, kb[2] = {0, 0};
    const uint32_t len[1] = {4};
    uint64_t pb[2] = {9, 9};
    uint8_t dig[32];
    size_t n = 5;
    CHECK(sv_ed25519_verify_txbodies_hinted_cpu(nid, body, off, len, kind, 1, sb, nullptr, nullptr, 0, kb, nullptr, 0,
                                                0, pb, nullptr, nullptr, nullptr, &n, dig, 1) == SV_OK);
    CHECK(n == 0 && pb[0] == 0 && pb[1] == 0);
    const uint64_t bad[2] = {0, 1};
    CHECK(sv_ed25519_verify_txbodies_hinted_cpu(nid, body, off, len, kind, 1, sb, nullptr, nullptr, 0, bad, nullptr, 0,
                                                0, pb, nullptr, nullptr, nullptr, &n, dig, 1) == SV_ERR_INVALID_ARG);
  }
  std::puts("txpair_core ok");
  return 0;
}
