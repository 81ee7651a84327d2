// TEST INFRASTRUCTURE: stand-alone driver of the by-account check entry points'
// host code -- the expansion functions of csrc/txacct.h through the engine's
// CPU form sv_ed25519_check_txbodies_accounts_cpu and its argument check
// (csrc/sv_cpu.cpp), and the by-account planner and packer of
// csrc/host_image.h -- meant to be built with -fsanitize=address,undefined and
// run directly (tests/test_txaccounts_cpu.py builds it from this file and
// sv_cpu.cpp).  Every packed image lives in a heap block of exactly the planned
// size, so a write past the plan is an ASan report.  The CPU form is compared
// with sv_ed25519_check_txbodies_cpu over an expansion written out here with
// plain loops (not txacct.h).  Prints "txacct_core ok" and returns 0, or the
// first failed check and 1.
//
// With -DTXACCT_STAGE_SHIM (and -shared) the same file is instead a small
// library that hands the planner and packer to Python (no main).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/stellar_sigverify.h"
#include "../../stellar-core_amd/csrc/host_image.h"

static_assert(sizeof(sv::AcctChunk) == 31 * sizeof(uint64_t), "hs_acct_plan hands AcctChunk out as 31 words");

#ifdef TXACCT_STAGE_SHIM
namespace {
sv::AcctIn shim_in(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, uint64_t nb,
                   const uint64_t* sb, const uint8_t* hint, const uint8_t* sig, const uint64_t* zeros,
                   const uint8_t* sig_len, const uint64_t* eb, const uint32_t* eacct, const uint64_t* cb,
                   const uint32_t* cacct, const uint8_t* clevel, const int32_t* cneed, const uint32_t* acnt) {
  return sv::AcctIn{{nullptr, bodies, off, len, kind, (size_t)nb, sb, hint, sig, zeros, nullptr},
                    sig_len, eb, eacct, cb, cacct, clevel, cneed, acnt};
}
}  // namespace
extern "C" {
// out: per chunk the 16 words of its PairChunk (b0, b1, s0, s1, k0, k1, body_bytes, o_sig, o_hint, o_off, o_sb,
// o_kb, o_len, o_kind, o_body, bytes), then e0, e1, c0, c1, nk, nq, ng, o_eb, o_cb, o_ea, o_ca, o_need, o_lvl,
// o_sl, bytes.  zeros: nb + 1 zero words (the hinted image's empty key CSR array).
int hs_acct_plan(const uint32_t* len, const uint64_t* sb, const uint64_t* zeros, const uint64_t* eb,
                 const uint32_t* eacct, const uint64_t* cb, const uint32_t* cacct, const uint32_t* acnt, int with_len,
                 uint64_t B0, uint64_t B1, uint64_t max_s, uint64_t max_k, uint64_t max_b, uint64_t max_c,
                 uint64_t max_g, uint64_t* out, int cap) {
  static const uint8_t one = 0;
  const sv::AcctIn in = shim_in(nullptr, nullptr, len, nullptr, 0, sb, nullptr, nullptr, zeros,
                                with_len ? &one : nullptr, eb, eacct, cb, cacct, nullptr, nullptr, acnt);
  const std::vector<sv::AcctChunk> plan = sv::acct_plan(in, B0, B1, max_s, max_k, max_b, max_c, max_g);
  for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) memcpy(out + 31 * i, &plan[i], sizeof(sv::AcctChunk));
  return (int)plan.size();
}
void hs_acct_pack(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, uint64_t nb,
                  const uint64_t* sb, const uint8_t* hint, const uint8_t* sig, const uint64_t* zeros,
                  const uint8_t* sig_len, const uint64_t* eb, const uint32_t* eacct, const uint64_t* cb,
                  const uint32_t* cacct, const uint8_t* clevel, const int32_t* cneed, const uint32_t* acnt,
                  const uint64_t chunk[31], uint8_t* dst) {
  sv::AcctChunk c;
  memcpy(&c, chunk, sizeof(c));
  sv::acct_pack(shim_in(bodies, off, len, kind, nb, sb, hint, sig, zeros, sig_len, eb, eacct, cb, cacct, clevel, cneed,
                        acnt),
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
struct Set {
  // bodies and signatures
  std::vector<uint8_t> bodies, kind, hint, sig, sig_len;
  std::vector<uint64_t> off, sb, zeros;
  std::vector<uint32_t> len;
  size_t nb = 0;
  // the account table
  std::vector<uint8_t> akey, thr, stype, skey, pay, plen;
  std::vector<uint64_t> sbeg;
  std::vector<uint32_t> sweight, spay;
  // the uses
  std::vector<uint64_t> eb, cb;
  std::vector<uint32_t> eacct, cacct;
  std::vector<uint8_t> clevel;
  std::vector<int32_t> cneed;
  size_t na() const { return thr.size() / 4; }
  sv_txaccounts desc() const {
    sv_txaccounts A{};
    A.struct_size = sizeof(A);
    A.protocol_version = 21;
    A.sig_len = sig_len.data();
    A.acct_key = akey.data();
    A.acct_thresholds = thr.data();
    A.asigner_begin = sbeg.data();
    A.asigner_type = stype.data();
    A.asigner_weight = sweight.data();
    A.asigner_key = skey.data();
    A.asigner_payload = spay.data();
    A.apayload = pay.data();
    A.apayload_len = plen.data();
    A.bacct_begin = eb.data();
    A.bacct = eacct.data();
    A.check_begin = cb.data();
    A.check_acct = cacct.data();
    A.check_level = clevel.data();
    A.check_needed = cneed.data();
    A.n_accounts = na();
    A.n_asigners = sbeg.back();
    A.n_apayloads = plen.size() - 1;
    A.n_bacct = eb.back();
    A.n_checks = cb.back();
    return A;
  }
};

// hints and key tails are drawn from four values, so hints collide all the time; HASH_X signers hold the SHA-256 of
// nothing the set signs, ed25519 verifications all fail: what is exercised is every table walk
Set make(size_t nb, size_t na, unsigned seed) {
  std::mt19937 rng(seed);
  Set s;
  s.nb = nb;
  const size_t np = 5;
  for (size_t i = 0; i < np; ++i) {
    const uint8_t l = (uint8_t)(i == 0 ? 0 : i == 1 ? 64 : rng() % 65);
    for (int b = 0; b < 64; ++b) s.pay.push_back(b < l ? (uint8_t)rng() : 0);
    s.plen.push_back(l);
  }
  s.plen.push_back(0);  // (never empty; not counted)
  s.sbeg.push_back(0);
  for (size_t a = 0; a < na; ++a) {
    for (int b = 0; b < 28; ++b) s.akey.push_back((uint8_t)rng());
    for (int b = 0; b < 4; ++b) s.akey.push_back((uint8_t)(a % 4));
    s.thr.push_back((uint8_t)(rng() % 3));  // master weight 0 in a third
    for (int b = 0; b < 3; ++b) s.thr.push_back((uint8_t)(rng() % 4));
    const size_t ng = a % 7 == 0 ? 0 : a % 11 == 3 ? 63 : rng() % 5;
    for (size_t g = 0; g < ng; ++g) {
      const uint8_t ty = (uint8_t)(rng() % 4);
      s.stype.push_back(ty);
      s.sweight.push_back(1 + rng() % 300);
      for (int b = 0; b < 28; ++b) s.skey.push_back((uint8_t)rng());
      for (int b = 0; b < 4; ++b) s.skey.push_back((uint8_t)(rng() % 4));
      s.spay.push_back(ty == 3 ? rng() % np : 0xFFFFFFFFu);
    }
    s.sbeg.push_back(s.stype.size());
  }
  s.sb.push_back(0);
  s.eb.push_back(0);
  s.cb.push_back(0);
  for (size_t t = 0; t < nb; ++t) {
    const uint32_t l = t % 11 == 0 ? 0 : rng() % 300;
    s.off.push_back(s.bodies.size());
    s.len.push_back(l);
    s.kind.push_back((uint8_t)(rng() % 3));
    for (uint32_t i = 0; i < l; ++i) s.bodies.push_back((uint8_t)rng());
    const size_t ns = t % 9 == 0 ? 20 : rng() % 3;
    for (size_t i = 0; i < ns; ++i) {
      const uint8_t x = (uint8_t)(rng() % 4);
      for (int b = 0; b < 4; ++b) s.hint.push_back(x);
      const uint8_t ln = rng() % 5 == 0 ? (uint8_t)(rng() % 65) : 64;
      for (int b = 0; b < 64; ++b) s.sig.push_back(b < ln ? (uint8_t)rng() : 0);
      s.sig_len.push_back(ln);
    }
    const size_t ne = t % 13 == 6 ? 0 : 1 + rng() % 3;
    for (size_t e = 0; e < ne; ++e) s.eacct.push_back((uint32_t)(e == 2 ? s.eacct.back() : rng() % na));
    const size_t nc = ne == 0 || t % 7 == 3 ? 0 : 1 + rng() % 4;
    for (size_t c = 0; c < nc; ++c) {
      s.cacct.push_back((uint32_t)(rng() % ne));
      s.clevel.push_back((uint8_t)(rng() % 4));
      s.cneed.push_back((int32_t)(rng() % 5) - 1);
    }
    s.sb.push_back(s.hint.size() / 4);
    s.eb.push_back(s.eacct.size());
    s.cb.push_back(s.cacct.size());
  }
  s.zeros.assign(nb + 1, 0);
  s.bodies.push_back(0);
  // (data() of an empty vector may be null: the tables are never empty)
  s.hint.resize(s.hint.size() + 4);
  s.sig.resize(s.sig.size() + 64);
  s.sig_len.push_back(0);
  s.stype.push_back(0);
  s.sweight.push_back(0);
  s.spay.push_back(0);
  s.skey.resize(s.skey.size() + 32);
  s.eacct.push_back(0);
  s.cacct.push_back(0);
  s.clevel.push_back(0);
  s.cneed.push_back(0);
  return s;
}

// per account: rows it adds to a key list and to the payload candidates (plain loops)
std::vector<uint32_t> account_rows(const Set& s) {
  std::vector<uint32_t> acnt(2 * s.na() + 2, 0);
  for (size_t a = 0; a < s.na(); ++a) {
    acnt[2 * a] = s.thr[4 * a] ? 1 : 0;
    for (uint64_t g = s.sbeg[a]; g < s.sbeg[a + 1]; ++g) ++acnt[2 * a + (s.stype[g] == 3 ? 1 : 0)];
  }
  return acnt;
}

// planner and packer under several bounds, with and without sig_len
int run_images(size_t nb, unsigned seed) {
  using namespace sv;
  const Set s = make(nb, 40, seed);
  const std::vector<uint32_t> acnt = account_rows(s);
  const uint8_t nid[32] = {7};
  const size_t big = (size_t)1 << 18;
  const size_t bounds[][5] = {{big, big, 64u << 20, big, big}, {25, big, 64u << 20, big, big},
                              {big, big, 64u << 20, 3, big},    {big, big, 64u << 20, big, 4},
                              {big, 7, 512, big, big},          {1, 1, 16, 1, 1}};
  for (int with_len = 0; with_len < 2; ++with_len) {
    const AcctIn in{{nid, s.bodies.data(), s.off.data(), s.len.data(), s.kind.data(), nb, s.sb.data(), s.hint.data(),
                     s.sig.data(), with_len ? nullptr : s.zeros.data(), nullptr},  // (no key CSR array, or a zero one)
                    with_len ? s.sig_len.data() : nullptr,
                    s.eb.data(),
                    s.eacct.data(),
                    s.cb.data(),
                    s.cacct.data(),
                    s.clevel.data(),
                    with_len ? s.cneed.data() : nullptr,
                    acnt.data()};
    for (auto const& b : bounds) {
      const std::vector<AcctChunk> plan = acct_plan(in, 0, nb, b[0], b[1], b[2], b[3], b[4]);
      size_t next = 0;
      for (const AcctChunk& c : plan) {
        const PairChunk& p = c.p;
        CHECK(p.b0 == next && p.b1 > p.b0 && p.b1 <= nb);
        CHECK(p.s0 == s.sb[p.b0] && p.s1 == s.sb[p.b1] && p.k0 == 0 && p.k1 == 0);
        CHECK(c.e0 == s.eb[p.b0] && c.e1 == s.eb[p.b1] && c.c0 == s.cb[p.b0] && c.c1 == s.cb[p.b1]);
        // the expanded rows, from the uses
        size_t nk = 0, nq = 0, ng = 0;
        for (size_t t = p.b0; t < p.b1; ++t) {
          for (uint64_t e = s.eb[t]; e < s.eb[t + 1]; ++e) {
            nk += acnt[2 * s.eacct[e]];
            nq += acnt[2 * s.eacct[e] + 1];
          }
          for (uint64_t k = s.cb[t]; k < s.cb[t + 1]; ++k) {
            const uint32_t a = s.eacct[s.eb[t] + s.cacct[k]];
            ng += acnt[2 * a] + acnt[2 * a + 1];
          }
        }
        CHECK(c.nk == nk && c.nq == nq && c.ng == ng);
        const size_t m = p.s1 - p.s0, k = p.b1 - p.b0, ne = c.e1 - c.e0, nc = c.c1 - c.c0;
        if (k > 1) CHECK(m <= b[0] && nk + nq <= b[1] && p.body_bytes <= b[2] && nc <= b[3] && ng <= b[4]);
        CHECK(c.o_eb % 16 == 0 && c.o_eb >= p.bytes && c.o_cb % 8 == 0 && c.o_ea % 4 == 0 && c.o_ca % 4 == 0 &&
              c.o_need % 4 == 0);
        uint8_t* h = (uint8_t*)std::malloc(c.bytes);  // exactly the plan: ASan guards its end
        CHECK(h != nullptr);
        acct_pack(in, c, h);
        CHECK(m == 0 || std::memcmp(h + p.o_sig, s.sig.data() + 64 * p.s0, 64 * m) == 0);
        const uint64_t* pe = (const uint64_t*)(h + c.o_eb);
        const uint64_t* pc = (const uint64_t*)(h + c.o_cb);
        for (size_t i = 0; i <= k; ++i) CHECK(pe[i] == s.eb[p.b0 + i] - c.e0 && pc[i] == s.cb[p.b0 + i] - c.c0);
        CHECK(ne == 0 || std::memcmp(h + c.o_ea, s.eacct.data() + c.e0, 4 * ne) == 0);
        CHECK(nc == 0 || std::memcmp(h + c.o_ca, s.cacct.data() + c.c0, 4 * nc) == 0);
        CHECK(nc == 0 || std::memcmp(h + c.o_lvl, s.clevel.data() + c.c0, nc) == 0);
        if (with_len) {
          CHECK(nc == 0 || std::memcmp(h + c.o_need, s.cneed.data() + c.c0, 4 * nc) == 0);
          CHECK(m == 0 || std::memcmp(h + c.o_sl, s.sig_len.data() + p.s0, m) == 0);
        }
        CHECK(c.o_sl + (with_len ? m : 0) <= c.bytes);
        std::free(h);
        next = p.b1;
      }
      CHECK(next == nb);
    }
  }
  return 0;
}

// the CPU form against the explicit CPU form over an expansion written out here
int run_cpu_form(size_t nb, unsigned seed) {
  const Set s = make(nb, 40, seed);
  const sv_txaccounts A = s.desc();
  const uint8_t nid[32] = {9, 1};
  const size_t nc = A.n_checks;
  std::vector<uint8_t> ok(nc + 1, 0xA5), dig(32 * nb);
  std::vector<uint32_t> weight(nc + 1, 0xA5A5A5A5u);
  std::vector<uint64_t> used(nc + 1, 0xA5);
  CHECK(sv_ed25519_check_txbodies_accounts_cpu(nid, s.bodies.data(), s.off.data(), s.len.data(), s.kind.data(), nb,
                                               s.sb.data(), s.hint.data(), s.sig.data(), s.sb.back(), &A, ok.data(),
                                               weight.data(), used.data(), dig.data(), 2) == SV_OK);
  CHECK(ok[nc] == 0xA5 && weight[nc] == 0xA5A5A5A5u && used[nc] == 0xA5);
  // the expansion, body by body
  std::vector<uint64_t> kb{0}, qb{0}, gb{0};
  std::vector<uint8_t> key, qkey, qpay, qlen, gt;
  std::vector<uint32_t> gw, gk;
  std::vector<int32_t> need;
  for (size_t t = 0; t < nb; ++t) {
    std::vector<uint32_t> krow, qrow;  // per entry: its first rows
    for (uint64_t e = s.eb[t]; e < s.eb[t + 1]; ++e) {
      const uint32_t a = s.eacct[e];
      krow.push_back((uint32_t)(key.size() / 32));
      qrow.push_back((uint32_t)(qkey.size() / 32));
      if (s.thr[4 * a]) key.insert(key.end(), s.akey.begin() + 32 * a, s.akey.begin() + 32 * a + 32);
      for (uint64_t g = s.sbeg[a]; g < s.sbeg[a + 1]; ++g) {
        std::vector<uint8_t>& dst = s.stype[g] == 3 ? qkey : key;
        dst.insert(dst.end(), s.skey.begin() + 32 * g, s.skey.begin() + 32 * g + 32);
        if (s.stype[g] == 3) {
          qpay.insert(qpay.end(), s.pay.begin() + 64 * s.spay[g], s.pay.begin() + 64 * s.spay[g] + 64);
          qlen.push_back(s.plen[s.spay[g]]);
        }
      }
    }
    for (uint64_t c = s.cb[t]; c < s.cb[t + 1]; ++c) {
      const uint32_t a = s.eacct[s.eb[t] + s.cacct[c]];
      uint32_t k = krow[s.cacct[c]], q = qrow[s.cacct[c]];
      if (s.thr[4 * a]) {
        gt.push_back(0);
        gw.push_back(s.thr[4 * a]);
        gk.push_back(k++);
      }
      for (uint64_t g = s.sbeg[a]; g < s.sbeg[a + 1]; ++g) {
        gt.push_back(s.stype[g]);
        gw.push_back(s.sweight[g]);
        gk.push_back(s.stype[g] == 3 ? q++ : k++);
      }
      need.push_back(s.clevel[c] ? (int32_t)s.thr[4 * a + s.clevel[c]] : s.cneed[c]);
      gb.push_back(gt.size());
    }
    kb.push_back(key.size() / 32);
    qb.push_back(qkey.size() / 32);
  }
  const size_t nk = key.size() / 32, nq = qlen.size(), ng = gt.size();
  key.resize(key.size() + 32);
  qkey.resize(qkey.size() + 32);
  qpay.resize(qpay.size() + 64);
  qlen.push_back(0);
  gt.push_back(0);
  gw.push_back(0);
  gk.push_back(0);
  need.push_back(0);
  sv_txchecks_payload P{};
  P.checks.struct_size = sizeof(P);
  P.checks.protocol_version = 21;
  P.checks.sig_len = s.sig_len.data();
  P.checks.check_begin = s.cb.data();
  P.checks.check_needed = need.data();
  P.checks.signer_begin = gb.data();
  P.checks.signer_type = gt.data();
  P.checks.signer_weight = gw.data();
  P.checks.signer_key = gk.data();
  P.checks.n_checks = nc;
  P.checks.n_signers = ng;
  P.pkey_begin = qb.data();
  P.pkey = qkey.data();
  P.pkey_payload = qpay.data();
  P.pkey_len = qlen.data();
  P.n_pkeys = nq;
  std::vector<uint8_t> ok2(nc + 1), dig2(32 * nb);
  std::vector<uint32_t> weight2(nc + 1);
  std::vector<uint64_t> used2(nc + 1);
  CHECK(sv_ed25519_check_txbodies_cpu(nid, s.bodies.data(), s.off.data(), s.len.data(), s.kind.data(), nb,
                                      s.sb.data(), s.hint.data(), s.sig.data(), s.sb.back(), kb.data(), key.data(), nk,
                                      &P.checks, ok2.data(), weight2.data(), used2.data(), dig2.data(), 2) == SV_OK);
  CHECK(std::memcmp(ok.data(), ok2.data(), nc) == 0 && std::memcmp(weight.data(), weight2.data(), 4 * nc) == 0 &&
        std::memcmp(used.data(), used2.data(), 8 * nc) == 0 && dig == dig2);
  // rejects: each returns before anything is written
  auto refused = [&](sv_txaccounts B) {
    return sv_ed25519_check_txbodies_accounts_cpu(nid, s.bodies.data(), s.off.data(), s.len.data(), s.kind.data(), nb,
                                                  s.sb.data(), s.hint.data(), s.sig.data(), s.sb.back(), &B, ok.data(),
                                                  weight.data(), used.data(), nullptr, 1) == SV_ERR_INVALID_ARG;
  };
  sv_txaccounts B = A;
  B.protocol_version = 7;
  CHECK(refused(B));
  B = A;
  B.struct_size = sizeof(A) - 1;
  CHECK(refused(B));
  B = A;
  B.n_accounts = A.n_accounts - 1;  // (asigner_begin no longer ends at n_asigners; bacct entries out of range)
  CHECK(refused(B));
  B = A;
  B.n_apayloads = 1;  // (type-3 signers index past it)
  CHECK(refused(B));
  B = A;
  B.check_level = nullptr;
  CHECK(refused(B));
  return 0;
}
}  // namespace

int main() {
  for (unsigned seed = 1; seed <= 3; ++seed)
    if (run_images(90 + 17 * seed, seed)) return 1;
  if (run_images(1, 5)) return 1;
  for (unsigned seed = 1; seed <= 2; ++seed)
    if (run_cpu_form(60 + 30 * seed, seed)) return 1;
  std::printf("txacct_core ok\n");
  return 0;
}
#endif
