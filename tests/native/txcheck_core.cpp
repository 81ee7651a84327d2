// TEST INFRASTRUCTURE: stand-alone driver of the check entry points' host code
// -- the decision function of csrc/txcheck.h, the check planner and packer of
// csrc/host_image.h and the engine's CPU form sv_ed25519_check_txbodies_cpu
// (csrc/sv_cpu.cpp) -- meant to be built with -fsanitize=address,undefined and
// run directly (tests/test_txchecks_cpu.py builds it from this file and
// sv_cpu.cpp).  Every packed image lives in a heap block of exactly the planned
// size, so a write past the plan is an ASan report.  Prints "txcheck_core ok"
// and returns 0, or the first failed check and 1.
//
// With -DTXCHECK_STAGE_SHIM (and -shared) the same file is instead a small
// library that hands the planner and packer to Python (no main).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/stellar_sigverify.h"
#include "../../stellar-core_amd/csrc/host_image.h"
#include "../../stellar-core_amd/csrc/txcheck.h"

namespace {
struct Set {
  std::vector<uint8_t> bodies, kind, hint, sig, key, sig_len, gtype;
  std::vector<uint64_t> off, sb, kb, cb, gb;
  std::vector<uint32_t> len, gweight, gkey;
  std::vector<int32_t> need;
  size_t nb = 0;
  sv::CheckIn in(const uint8_t* nid, bool with_len) const {
    return sv::CheckIn{{nid, bodies.data(), off.data(), len.data(), kind.data(), nb, sb.data(), hint.data(),
                        sig.data(), kb.data(), key.data()},
                       with_len ? sig_len.data() : nullptr,
                       cb.data(),
                       need.data(),
                       gb.data(),
                       gtype.data(),
                       gweight.data(),
                       gkey.data()};
  }
};

Set make(size_t nb, unsigned seed) {
  std::mt19937 rng(seed);
  Set s;
  s.nb = nb;
  s.sb.push_back(0);
  s.kb.push_back(0);
  s.cb.push_back(0);
  s.gb.push_back(0);
  for (size_t t = 0; t < nb; ++t) {
    const uint32_t l = t % 11 == 0 ? 0 : rng() % 300;
    s.off.push_back(s.bodies.size());
    s.len.push_back(l);
    s.kind.push_back((uint8_t)(rng() % 3));
    for (uint32_t i = 0; i < l; ++i) s.bodies.push_back((uint8_t)rng());
    const size_t ns = t % 9 == 0 ? 20 : rng() % 3, nk = t % 9 == 0 ? 20 : 1 + rng() % 4;
    const size_t k0 = s.key.size() / 32;
    for (size_t i = 0; i < nk; ++i) {
      for (int b = 0; b < 28; ++b) s.key.push_back((uint8_t)rng());
      const uint8_t x = (uint8_t)(rng() % 3);
      for (int b = 0; b < 4; ++b) s.key.push_back(x);
    }
    for (size_t i = 0; i < ns; ++i) {
      const uint8_t x = (uint8_t)(rng() % 4);
      for (int b = 0; b < 4; ++b) s.hint.push_back(x);
      const uint8_t ln = rng() % 5 == 0 ? (uint8_t)(rng() % 65) : 64;
      for (int b = 0; b < 64; ++b) s.sig.push_back(b < ln ? (uint8_t)rng() : 0);
      s.sig_len.push_back(ln);
    }
    const size_t nc = t % 7 == 3 ? 0 : 1 + rng() % 4;  // (bodies without checks among the others)
    for (size_t c = 0; c < nc; ++c) {
      const size_t ng = rng() % 5;
      for (size_t g = 0; g < ng; ++g) {
        s.gtype.push_back((uint8_t)(rng() % 4));
        s.gweight.push_back(1 + rng() % 300);
        s.gkey.push_back((uint32_t)(k0 + rng() % nk));
      }
      s.need.push_back((int32_t)(rng() % 5) - 1);
      s.gb.push_back(s.gtype.size());
    }
    s.sb.push_back(s.hint.size() / 4);
    s.kb.push_back(s.key.size() / 32);
    s.cb.push_back(s.need.size());
  }
  s.bodies.push_back(0);  // (never empty)
  // (data() of an empty vector may be null: the tables are never empty)
  s.gtype.push_back(0);
  s.gweight.push_back(0);
  s.gkey.push_back(0);
  s.need.push_back(0);
  s.hint.resize(s.hint.size() + 4);
  s.sig.resize(s.sig.size() + 64);
  s.sig_len.push_back(0);
  return s;
}
}  // namespace

#ifdef TXCHECK_STAGE_SHIM
static_assert(sizeof(sv::CheckChunk) == 28 * sizeof(uint64_t), "hs_check_plan hands CheckChunk out as 28 words");
namespace {
sv::CheckIn shim_in(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, uint64_t nb,
                    const uint64_t* sb, const uint8_t* hint, const uint8_t* sig, const uint64_t* kb, const uint8_t* key,
                    const uint8_t* sig_len, const uint64_t* cb, const int32_t* need, const uint64_t* gb,
                    const uint8_t* gtype, const uint32_t* gweight, const uint32_t* gkey) {
  return sv::CheckIn{{nullptr, bodies, off, len, kind, (size_t)nb, sb, hint, sig, kb, key},
                     sig_len, cb, need, gb, gtype, gweight, gkey};
}
}  // namespace
extern "C" {
// out: per chunk the 16 words of its PairChunk (b0, b1, s0, s1, k0, k1, body_bytes, o_sig, o_hint, o_off, o_sb,
// o_kb, o_len, o_kind, o_body, bytes), then c0, c1, g0, g1, o_cb, o_gb, o_need, o_gw, o_gk, o_gt, o_sl, bytes
int hs_check_plan(const uint32_t* len, const uint64_t* sb, const uint64_t* kb, const uint64_t* cb, const uint64_t* gb,
                  int with_len, uint64_t B0, uint64_t B1, uint64_t max_s, uint64_t max_k, uint64_t max_b,
                  uint64_t max_c, uint64_t max_g, uint64_t* out, int cap) {
  static const uint8_t one = 0;
  const sv::CheckIn in = shim_in(nullptr, nullptr, len, nullptr, 0, sb, nullptr, nullptr, kb, nullptr,
                                 with_len ? &one : nullptr, cb, nullptr, gb, nullptr, nullptr, nullptr);
  const std::vector<sv::CheckChunk> plan = sv::check_plan(in, B0, B1, max_s, max_k, max_b, max_c, max_g);
  for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) memcpy(out + 28 * i, &plan[i], sizeof(sv::CheckChunk));
  return (int)plan.size();
}
void hs_check_pack(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, uint64_t nb,
                   const uint64_t* sb, const uint8_t* hint, const uint8_t* sig, const uint64_t* kb, const uint8_t* key,
                   const uint8_t* sig_len, const uint64_t* cb, const int32_t* need, const uint64_t* gb,
                   const uint8_t* gtype, const uint32_t* gweight, const uint32_t* gkey, const uint64_t chunk[28],
                   uint8_t* dst) {
  sv::CheckChunk c;
  memcpy(&c, chunk, sizeof(c));
  sv::check_pack(shim_in(bodies, off, len, kind, nb, sb, hint, sig, kb, key, sig_len, cb, need, gb, gtype, gweight,
                         gkey),
                 c, dst);
}
}  // extern "C"
#else

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

namespace {
// planner and packer under several bounds, with and without sig_len
int run_images(size_t nb, unsigned seed) {
  using namespace sv;
  const Set s = make(nb, seed);
  const uint8_t nid[32] = {7};
  const size_t big = (size_t)1 << 18;
  const size_t bounds[][5] = {{big, big, 64u << 20, big, big}, {25, big, 64u << 20, big, big},
                              {big, big, 64u << 20, 3, big},    {big, big, 64u << 20, big, 4},
                              {big, 7, 512, big, big},          {1, 1, 16, 1, 1}};
  for (int with_len = 0; with_len < 2; ++with_len) {
    const CheckIn in = s.in(nid, with_len != 0);
    for (auto const& b : bounds) {
      const std::vector<CheckChunk> plan = check_plan(in, 0, nb, b[0], b[1], b[2], b[3], b[4]);
      size_t next = 0;
      for (const CheckChunk& c : plan) {
        const PairChunk& p = c.p;
        CHECK(p.b0 == next && p.b1 > p.b0 && p.b1 <= nb);
        CHECK(p.s0 == s.sb[p.b0] && p.s1 == s.sb[p.b1] && p.k0 == s.kb[p.b0] && p.k1 == s.kb[p.b1]);
        CHECK(c.c0 == s.cb[p.b0] && c.c1 == s.cb[p.b1] && c.g0 == s.gb[c.c0] && c.g1 == s.gb[c.c1]);
        const size_t m = p.s1 - p.s0, q = p.k1 - p.k0, k = p.b1 - p.b0, nc = c.c1 - c.c0, ng = c.g1 - c.g0;
        if (k > 1) CHECK(m <= b[0] && q <= b[1] && p.body_bytes <= b[2] && nc <= b[3] && ng <= b[4]);
        CHECK(c.o_cb % 16 == 0 && c.o_cb >= p.bytes && c.o_gb % 8 == 0 && c.o_need % 4 == 0 && c.o_gw % 4 == 0 &&
              c.o_gk % 4 == 0);
        uint8_t* h = (uint8_t*)std::malloc(c.bytes);  // exactly the plan: ASan guards its end
        CHECK(h != nullptr);
        check_pack(in, c, h);
        CHECK(q == 0 || std::memcmp(h, s.key.data() + 32 * p.k0, 32 * q) == 0);
        CHECK(m == 0 || std::memcmp(h + p.o_sig, s.sig.data() + 64 * p.s0, 64 * m) == 0);
        const uint64_t* pc = (const uint64_t*)(h + c.o_cb);
        const uint64_t* pg = (const uint64_t*)(h + c.o_gb);
        CHECK(pc[0] == 0 && pc[k] == nc && pg[0] == 0 && pg[nc] == ng);
        for (size_t i = 0; i <= k; ++i) CHECK(pc[i] == s.cb[p.b0 + i] - c.c0);
        for (size_t i = 0; i <= nc; ++i) CHECK(pg[i] == s.gb[c.c0 + i] - c.g0);
        CHECK(nc == 0 || std::memcmp(h + c.o_need, s.need.data() + c.c0, 4 * nc) == 0);
        CHECK(ng == 0 || std::memcmp(h + c.o_gw, s.gweight.data() + c.g0, 4 * ng) == 0);
        CHECK(ng == 0 || std::memcmp(h + c.o_gt, s.gtype.data() + c.g0, ng) == 0);
        for (size_t i = 0; i < ng; ++i) {
          const uint32_t rel = ((const uint32_t*)(h + c.o_gk))[i];
          CHECK(rel == s.gkey[c.g0 + i] - p.k0 && rel < q);
        }
        if (with_len) CHECK(m == 0 || std::memcmp(h + c.o_sl, s.sig_len.data() + p.s0, m) == 0);
        CHECK(c.o_sl + (with_len ? m : 0) <= c.bytes);
        std::free(h);
        next = p.b1;
      }
      CHECK(next == nb);
    }
  }
  return 0;
}

// txcheck.h against pairs and verdicts made up here (no signature is verified)
int run_decisions() {
  // one body: 3 signatures, 4 key rows; key 3 is the contents hash
  uint8_t key[4 * 32], sig[3 * 64] = {0}, hint[3 * 4], digest[32];
  for (int i = 0; i < 4 * 32; ++i) key[i] = (uint8_t)(i * 7 + 1);
  std::memcpy(digest, key + 96, 32);
  for (int s = 0; s < 3; ++s) std::memcpy(hint + 4 * s, key + 32 * s + 28, 4);  // signature s <-> key s
  const uint32_t ps[3] = {0, 1, 2}, pk[3] = {0, 1, 2};
  uint8_t pv[3] = {1, 1, 1};
  sv_txcheck_body b{};
  b.hint = hint;
  b.sig = sig;
  b.sig_len = nullptr;
  b.key = key;
  b.pair_sig = ps;
  b.pair_key = pk;
  b.pair_verdict = pv;
  b.digest = digest;
  b.s0 = 0;
  b.ns = 3;
  b.k0 = 0;
  b.k1 = 4;
  b.p0 = 0;
  b.p1 = 3;
  const uint8_t ed[3] = {0, 0, 0};
  const uint32_t w1[3] = {1, 1, 1}, k012[3] = {0, 1, 2};
  sv_txcheck_result r = sv_txcheck<true>(b, ed, w1, k012, 3, 2, true);
  CHECK(r.ok == 1 && r.total == 2 && r.used == 3);  // early exit: signature 2 stays unmarked
  r = sv_txcheck<true>(b, ed, w1, k012, 3, 9, true);
  CHECK(r.ok == 0 && r.total == 3 && r.used == 7);
  r = sv_txcheck<true>(b, ed, w1, k012, 0, 0, true);
  CHECK(r.ok == 0 && r.total == 0 && r.used == 0);  // needed 0 without a match
  const uint32_t w300[1] = {300}, k0[1] = {0};
  r = sv_txcheck<true>(b, ed, w300, k0, 1, 256, false);
  CHECK(r.ok == 1 && r.total == 300);
  r = sv_txcheck<true>(b, ed, w300, k0, 1, 256, true);
  CHECK(r.ok == 0 && r.total == 255 && r.used == 1);
  pv[0] = 0;  // a rejected pair does not match
  r = sv_txcheck<true>(b, ed, w300, k0, 1, 1, true);
  CHECK(r.ok == 0 && r.total == 0 && r.used == 0);
  pv[0] = 1;
  const uint8_t pre[2] = {1, 0};  // PRE_AUTH_TX on the hash row, then an ed25519 signer
  const uint32_t w35[2] = {3, 5}, k30[2] = {3, 0};
  r = sv_txcheck<true>(b, pre, w35, k30, 2, 3, true);
  CHECK(r.ok == 1 && r.total == 3 && r.used == 0);
  r = sv_txcheck<true>(b, pre, w35, k30, 2, 8, true);
  CHECK(r.ok == 1 && r.total == 8 && r.used == 1);
  const uint32_t out_of_range[1] = {4};  // a key index outside the body matches nothing
  r = sv_txcheck<true>(b, ed, w1, out_of_range, 1, 0, true);
  CHECK(r.ok == 0 && r.used == 0);
  // HASH_X: SHA-256("abc") as key row 1, the preimage as signature 1
  static const uint8_t abc[32] = {0xba, 0x78, 0x16, 0xbf, 0x8f, 0x01, 0xcf, 0xea, 0x41, 0x41, 0x40,
                                  0xde, 0x5d, 0xae, 0x22, 0x23, 0xb0, 0x03, 0x61, 0xa3, 0x96, 0x17,
                                  0x7a, 0x9c, 0xb4, 0x10, 0xff, 0x61, 0xf2, 0x00, 0x15, 0xad};
  std::memcpy(key + 32, abc, 32);
  std::memcpy(hint + 4, abc + 28, 4);
  std::memcpy(sig + 64, "abc", 3);
  const uint8_t lens[3] = {64, 3, 64};
  b.sig_len = lens;
  const uint8_t hx[1] = {2};
  const uint32_t w4[1] = {4}, k1[1] = {1};
  r = sv_txcheck<true>(b, hx, w4, k1, 1, 4, true);
  CHECK(r.ok == 1 && r.total == 4 && r.used == 2);
  // the kernel's fast form gives such a check up (and decides every other one itself)
  r = sv_txcheck<false>(b, hx, w4, k1, 1, 4, true);
  CHECK(r.ok == SV_TXCHECK_DEFER && r.total == 0 && r.used == 0);
  r = sv_txcheck<false>(b, ed, w1, k012, 3, 2, true);
  CHECK(r.ok == 1 && r.total == 2 && r.used == 5);  // (signature 1, three bytes long, matches no ed25519 signer)
  const uint8_t lens4[3] = {64, 4, 64};  // another length is another preimage
  b.sig_len = lens4;
  r = sv_txcheck<true>(b, hx, w4, k1, 1, 4, true);
  CHECK(r.ok == 0 && r.used == 0);
  b.sig_len = lens;
  hint[4] ^= 1;  // the right preimage under a wrong hint
  r = sv_txcheck<true>(b, hx, w4, k1, 1, 4, true);
  CHECK(r.ok == 0 && r.used == 0);
  // a 63-byte signature never matches an ed25519 signer
  const uint8_t lens63[3] = {63, 64, 64};
  b.sig_len = lens63;
  r = sv_txcheck<true>(b, ed, w1, k0, 1, 1, true);
  CHECK(r.ok == 0 && r.used == 0);
  return 0;
}

// the CPU form: limits and argument errors, and a random set end to end
int run_cpu_form() {
  const Set s = make(60, 9);
  const uint8_t nid[32] = {3};
  const size_t nb = s.nb, ns = s.sb[nb], nk = s.kb[nb], nc = s.cb[nb], ng = s.gb[nc];
  sv_txchecks ck;
  ck.struct_size = sizeof ck;
  ck.protocol_version = 21;
  ck.sig_len = s.sig_len.data();
  ck.check_begin = s.cb.data();
  ck.check_needed = s.need.data();
  ck.signer_begin = s.gb.data();
  ck.signer_type = s.gtype.data();
  ck.signer_weight = s.gweight.data();
  ck.signer_key = s.gkey.data();
  ck.n_checks = nc;
  ck.n_signers = ng;
  // outputs of exactly nc entries
  uint8_t* ok = (uint8_t*)std::malloc(nc + 1);
  uint32_t* weight = (uint32_t*)std::malloc(4 * nc + 4);
  uint64_t* used = (uint64_t*)std::malloc(8 * nc + 8);
  std::vector<uint8_t> dig(32 * nb);
  auto call = [&](const sv_txchecks& c) {
    return sv_ed25519_check_txbodies_cpu(nid, s.bodies.data(), s.off.data(), s.len.data(), s.kind.data(), nb,
                                         s.sb.data(), s.hint.data(), s.sig.data(), ns, s.kb.data(), s.key.data(), nk,
                                         &c, ok, weight, used, dig.data(), 2);
  };
  CHECK(call(ck) == SV_OK);
  for (size_t t = 0; t < nb; ++t)
    for (uint64_t c = s.cb[t]; c < s.cb[t + 1]; ++c) {
      CHECK(ok[c] <= 1);
      const uint64_t n = s.sb[t + 1] - s.sb[t];
      CHECK(n >= 64 || (used[c] >> n) == 0);  // marks only on the body's own signatures
    }
  sv_txchecks bad = ck;
  bad.protocol_version = 7;
  CHECK(call(bad) == SV_ERR_INVALID_ARG);
  bad = ck;
  bad.check_begin = nullptr;
  CHECK(call(bad) == SV_ERR_INVALID_ARG);
  bad = ck;
  bad.struct_size = 8;
  CHECK(call(bad) == SV_ERR_INVALID_ARG);
  std::vector<uint8_t> ty = s.gtype;
  ty[0] = 4;
  bad = ck;
  bad.signer_type = ty.data();
  CHECK(ng == 0 || call(bad) == SV_ERR_INVALID_ARG);
  std::vector<uint32_t> gk = s.gkey;
  gk[0] = (uint32_t)nk;  // outside its body
  bad = ck;
  bad.signer_key = gk.data();
  CHECK(ng == 0 || call(bad) == SV_ERR_INVALID_ARG);
  std::vector<uint8_t> sl = s.sig_len;
  sl[0] = 65;
  bad = ck;
  bad.sig_len = sl.data();
  CHECK(call(bad) == SV_ERR_INVALID_ARG);
  std::free(ok);
  std::free(weight);
  std::free(used);
  return 0;
}

// the CPU form on the deterministic edge cases (no valid ed25519 signature needed): PRE_AUTH_TX, HASH_X, needed 0,
// zero counts and the limits
int run_cpu_edges() {
  static const uint8_t abc[32] = {0xba, 0x78, 0x16, 0xbf, 0x8f, 0x01, 0xcf, 0xea, 0x41, 0x41, 0x40,
                                  0xde, 0x5d, 0xae, 0x22, 0x23, 0xb0, 0x03, 0x61, 0xa3, 0x96, 0x17,
                                  0x7a, 0x9c, 0xb4, 0x10, 0xff, 0x61, 0xf2, 0x00, 0x15, 0xad};
  const uint8_t nid[32] = {5};
  // body 0: keys {its contents hash, SHA-256("abc"), a key no signature verifies under}; signatures {"abc" (3
  // bytes) under the hash-x hint, 64 junk bytes under the third key's hint}.  body 1: nothing.  body 2: a key,
  // no signature.
  const uint8_t bodies[12] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
  const uint64_t off[3] = {0, 8, 8}, sb[4] = {0, 2, 2, 2}, kb[4] = {0, 3, 3, 4};
  const uint32_t len[3] = {8, 0, 4};
  const uint8_t kind[3] = {0, 1, 2};
  uint8_t key[4 * 32], hint[2 * 4], sig[2 * 64] = {0};
  for (int i = 0; i < 4 * 32; ++i) key[i] = (uint8_t)(i * 11 + 3);
  std::memcpy(key + 32, abc, 32);
  std::memcpy(hint, abc + 28, 4);
  std::memcpy(hint + 4, key + 64 + 28, 4);
  std::memcpy(sig, "abc", 3);
  for (int i = 0; i < 64; ++i) sig[64 + i] = (uint8_t)(200 - i);
  const uint8_t sig_len[2] = {3, 64};
  //                       c0      c1         c2   c3   c4 |  c5   c6
  const uint64_t cb[4] = {0, 5, 5, 7};
  const int32_t need[7] = {3, 7, 9, 0, 0, 1, 0};
  const uint64_t gb[8] = {0, 1, 3, 4, 5, 5, 6, 7};
  const uint8_t gt[7] = {1, 1, 2, 2, 0, 0, 1};
  const uint32_t gw[7] = {3, 3, 4, 4, 1, 1, 1};
  const uint32_t gk[7] = {0, 0, 1, 1, 2, 3, 3};
  sv_txchecks ck;
  ck.struct_size = sizeof ck;
  ck.protocol_version = 21;
  ck.sig_len = sig_len;
  ck.check_begin = cb;
  ck.check_needed = need;
  ck.signer_begin = gb;
  ck.signer_type = gt;
  ck.signer_weight = gw;
  ck.signer_key = gk;
  ck.n_checks = 7;
  ck.n_signers = 7;
  uint8_t ok[7], dig[3 * 32];
  uint32_t weight[7];
  uint64_t used[7];
  auto call = [&] {
    return sv_ed25519_check_txbodies_cpu(nid, bodies, off, len, kind, 3, sb, hint, sig, 2, kb, key, 4, &ck, ok, weight,
                                         used, dig, 1);
  };
  CHECK(call() == SV_OK);                // (first for body 0's contents hash ...)
  std::memcpy(key, dig, 32);             // ... which becomes its PRE_AUTH_TX key row
  CHECK(call() == SV_OK);
  const uint8_t want_ok[7] = {1, 1, 0, 0, 0, 0, 0};
  const uint32_t want_w[7] = {3, 7, 4, 0, 0, 0, 0};
  const uint64_t want_u[7] = {0, 1, 1, 0, 0, 0, 0};
  for (int c = 0; c < 7; ++c) CHECK(ok[c] == want_ok[c] && weight[c] == want_w[c] && used[c] == want_u[c]);
  // limits: 64 signatures and 64 signers are taken, 65 of either are not
  for (int over = 0; over < 3; ++over) {
    const size_t ns = over == 1 ? 65 : 64, ng = over == 2 ? 65 : 64;
    std::vector<uint8_t> h(4 * ns, 0), sg(64 * ns, 7), ty(ng, 2);
    std::vector<uint32_t> w(ng, 1), k(ng, 0);
    std::memcpy(&h[4 * (ns - 1)], abc + 28, 4);  // the last signature is the preimage
    std::fill(sg.end() - 64, sg.end(), 0);
    std::memcpy(&sg[64 * (ns - 1)], "abc", 3);
    std::vector<uint8_t> sl(ns, 64);
    sl[ns - 1] = 3;
    const uint64_t sb1[2] = {0, ns}, kb1[2] = {0, 1}, cb1[2] = {0, 1}, gb1[2] = {0, ng}, off1[1] = {0};
    const uint32_t len1[1] = {8};
    const uint8_t kind1[1] = {0};
    const int32_t need1[1] = {1};
    sv_txchecks c1 = ck;
    c1.sig_len = sl.data();
    c1.check_begin = cb1;
    c1.check_needed = need1;
    c1.signer_begin = gb1;
    c1.signer_type = ty.data();
    c1.signer_weight = w.data();
    c1.signer_key = k.data();
    c1.n_checks = 1;
    c1.n_signers = ng;
    const int rc = sv_ed25519_check_txbodies_cpu(nid, bodies, off1, len1, kind1, 1, sb1, h.data(), sg.data(), ns, kb1,
                                                 abc, 1, &c1, ok, weight, used, nullptr, 1);
    if (over) CHECK(rc == SV_ERR_INVALID_ARG);
    else CHECK(rc == SV_OK && ok[0] == 1 && weight[0] == 1 && used[0] == (uint64_t)1 << 63);
  }
  return 0;
}
}  // namespace

int main() {
  if (run_decisions()) return 1;
  if (run_cpu_edges()) return 1;
  if (run_images(1, 1) || run_images(40, 2) || run_images(257, 3)) return 1;
  if (run_cpu_form()) return 1;
  std::puts("txcheck_core ok");
  return 0;
}
#endif
