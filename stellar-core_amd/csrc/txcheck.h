// One SignatureChecker::checkSignature call replayed against inputs that are
// already on hand (reference src/transactions/SignatureChecker.cpp:30-136):
// the body's decorated signatures, its candidate key rows, the pairs the
// pairing stage made of them with the verify launch's verdicts, the body's
// contents hash, and the check's signers and needed weight.  Written once for
// the check kernel (sv_txcheck.hip) and the CPU form (sv_cpu.cpp).
//
// Order, as in the reference:
//   1. PRE_AUTH_TX signers in list order: a signer whose key row equals the
//      contents hash adds its weight; total >= needed succeeds at once.  No
//      signature is marked, no signer erased.
//   2. HASH_X signers, then ED25519 signers, one pass each with the total
//      carried over: for each signature in order, the first signer of the type
//      that is still remaining (list order) and matches marks the signature,
//      adds its weight and either succeeds at once (later signatures stay
//      unmarked) or is erased.
//        HASH_X   hint == bytes 28..31 of the key row and SHA-256 of the
//                 signature's `len` bytes == the row (SignatureUtils.cpp:83-91)
//        ED25519  length 64 and the pair (signature, key index) exists with
//                 verdict 1 (a pair exists iff the hint matched; another
//                 length never verifies, SecretKey.cpp:441-444)
//   3. ED25519_SIGNED_PAYLOAD signers last, one more pass of the same shape with
//      the total carried over (SignatureUtils.cpp:48-61, no protocol gate): the
//      signer's key is an index into the body's payload candidates, and it
//      matches iff the length is 64 and the pair (signature, candidate) exists
//      with verdict 1 -- the payload pairing makes a pair iff the hint equals
//      hint(key) XOR hint(payload), and the pair's verdict is the signature
//      verified over the payload.  The pass runs only for a body that has payload
//      pairs (pp1 > pp0): without the payload tables there are none, type-3
//      signers are skipped, and the returned total and marks are the state a
//      caller continues from.
// The total is kept in 64 bits and returned saturated to 32; the reference (and
// the host mirror) add into a 32-bit int, so the two can only differ where that
// int overflows: unclamped weights (below protocol 10) summing to 2^31 or more,
// which no ledger-valid signer list reaches.
// Success is only tested after a match, so needed <= 0 without a match is
// false.  Remaining signers live in a 64-bit mask: at most 64 signers and the
// body's first 64 signatures are considered (the reference's limits are 20 and
// about 23).  A signer whose key index lies outside the body's key rows
// matches nothing.
#pragma once

#include "hash_dev.h"

#if !defined(__HIPCC__)
#include <string.h>
#endif

enum { SV_SIGNER_ED25519 = 0, SV_SIGNER_PRE_AUTH_TX = 1, SV_SIGNER_HASH_X = 2, SV_SIGNER_SIGNED_PAYLOAD = 3 };
#define SV_TXCHECK_MAX 64


// The arrays are the whole batch's (or chunk's); the body is the ranges.
// Alignment on the device: hint 4, sig / key / digest 16 bytes; any on the host.
struct sv_txcheck_body {
  const uint8_t* hint;          // 4 B per signature
  const uint8_t* sig;           // 64 B rows, zero-padded
  const uint8_t* sig_len;       // one byte per signature, or nullptr: all 64
  const uint8_t* key;           // 32 B rows
  const uint32_t* pair_sig;     // the pairing stage's output, (signature, key) order
  const uint32_t* pair_key;
  const uint8_t* pair_verdict;
  const uint8_t* digest;        // the body's contents hash, 32 B
  uint64_t s0;                  // the body's signatures [s0, s0 + ns), ns <= 64
  uint32_t ns;
  uint64_t k0, k1;              // its key rows
  uint64_t p0, p1;              // its pairs
  // the payload pairing's output, (signature, candidate) order, and the body's
  // payload candidates [q0, q1) and payload pairs [pp0, pp1) (all 0: no tables)
  const uint32_t* ppair_sig;
  const uint32_t* ppair_key;
  const uint8_t* ppair_verdict;
  uint64_t q0, q1;
  uint64_t pp0, pp1;
};

struct sv_txcheck_result {
  uint32_t ok;     // the check reached its needed weight
  uint32_t total;  // the weight after the last pass, saturated
  uint64_t used;   // bit s: body-local signature s was marked
};

SV_HD uint32_t sv_txc_ld32(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const uint32_t*)p;
#else
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
#endif
}

SV_HD bool sv_txc_rows_equal(const uint8_t* a, const uint8_t* b) {
  uint32_t d = 0;
  SV_UNROLL for (int i = 0; i < 8; ++i) d |= sv_txc_ld32(a + 4 * i) ^ sv_txc_ld32(b + 4 * i);
  return d == 0;
}

// The hint a signed-payload signer is found by (SignatureUtils::getSignedPayloadHint): the key's last four
// bytes XOR the payload's (getHint: a payload shorter than four bytes is followed by zeros); len <= 64.
SV_HD uint32_t sv_payload_hint(const uint8_t* key, const uint8_t* payload, uint32_t len) {
  uint32_t h = 0;
  const uint32_t n = len < 4u ? len : 4u;
  SV_UNROLL for (uint32_t i = 0; i < 4; ++i)
    if (i < n) h |= (uint32_t)payload[len - n + i] << (8 * i);
  return h ^ sv_txc_ld32(key + 28);
}

// SHA-256(row[0 .. len)) == key row.
SV_HD bool sv_txc_hashx(const uint8_t* row, uint32_t len, const uint8_t* keyrow) {
  uint32_t d[8];
#if defined(__HIP_DEVICE_COMPILE__)
  sv_sha256(d, row, len);
#else
  // (sv_sha256 reads whole aligned dwords: give it an aligned copy of the row)
  uint32_t copy[16];
  memcpy(copy, row, 64);
  sv_sha256(d, (const uint8_t*)copy, len);
#endif
  uint32_t x = 0;
  SV_UNROLL for (int i = 0; i < 8; ++i) x |= d[i] ^ sv_txc_ld32(keyrow + 4 * i);
  return x == 0;
}

// One pass over pairs: the ED25519 pass over the (signature, key) pairs, the
// signed-payload pass over the (signature, payload candidate) pairs.  For each
// of the body's signatures in order, the first signer of `rem` (list order)
// whose index has a pair with the signature of verdict 1 marks it, adds its
// weight and either succeeds (returns true) or is erased.  A cursor walks the
// pairs, which are sorted by signature.
SV_HD bool sv_txc_pair_pass(const sv_txcheck_body& b, const uint32_t* pair_sig, const uint32_t* pair_key,
                            const uint8_t* pair_verdict, uint64_t p, const uint64_t p1, const uint32_t ns,
                            const uint32_t* sw, const uint32_t* sk, int32_t needed, bool clamp, uint64_t rem,
                            int64_t* total, uint64_t* used) {
  bool done = false;
  SV_NOUNROLL for (uint32_t s = 0; s < ns && !done; ++s) {
    const uint64_t gs = b.s0 + s;
    while (p < p1 && pair_sig[p] < gs) ++p;
    if (p >= p1) break;  // (no pair is left for this or any later signature)
    if (pair_sig[p] != gs) continue;
    if (b.sig_len && b.sig_len[gs] != 64) continue;
    SV_NOUNROLL for (uint64_t m = rem; m; m &= m - 1) {
      const uint32_t g = (uint32_t)__builtin_ctzll(m);
      const uint32_t k = sk[g];
      bool match = false;
      for (uint64_t q = p; q < p1 && pair_sig[q] == gs; ++q)
        if (pair_key[q] == k) {
          match = pair_verdict[q] == 1;
          break;
        }
      if (!match) continue;
      *used |= (uint64_t)1 << s;
      const uint32_t w = sw[g];
      *total += clamp && w > 255u ? 255u : w;
      done = *total >= (int64_t)needed;
      rem &= ~((uint64_t)1 << g);
      break;
    }
  }
  return done;
}

// st / sw / sk: the check's first signer; n signers (the first 64 considered).
// SHA = false is the check kernel's fast form, built without the SHA-256: at the
// first HASH_X signer whose hint matches a signature it gives up and returns
// ok == SV_TXCHECK_DEFER (total and used 0); the caller then runs the check
// again with SHA = true.  HASH_X signers are rare, and with the two
// compressions in it the function needs twice the registers.  PAYLOAD = false
// gives up in the same way when the signed-payload pass would have to run (the
// first three stages did not succeed, and a type-3 signer is live in a body
// that has payload pairs).
#define SV_TXCHECK_DEFER 2u
template <bool SHA, bool PAYLOAD = SHA>
SV_HD sv_txcheck_result sv_txcheck(const sv_txcheck_body& b, const uint8_t* st, const uint32_t* sw, const uint32_t* sk,
                                   uint32_t n, int32_t needed, bool clamp) {
  sv_txcheck_result r;
  r.ok = 0;
  r.used = 0;
  if (n > SV_TXCHECK_MAX) n = SV_TXCHECK_MAX;
  const uint32_t ns = b.ns < SV_TXCHECK_MAX ? b.ns : SV_TXCHECK_MAX;
  int64_t total = 0;  // (64 weights below 2^32 cannot overflow it)
  uint64_t rem_hx = 0, rem_ed = 0, rem_pl = 0;
  const bool payload = b.pp1 > b.pp0;
  bool done = false;
  SV_NOUNROLL for (uint32_t g = 0; g < n && !done; ++g) {
    const uint64_t k = sk[g];
    const uint32_t type = st[g];
    if (type == SV_SIGNER_SIGNED_PAYLOAD) {
      if (payload && k >= b.q0 && k < b.q1) rem_pl |= (uint64_t)1 << g;
      continue;
    }
    if (k < b.k0 || k >= b.k1) continue;
    if (type == SV_SIGNER_ED25519) rem_ed |= (uint64_t)1 << g;
    else if (type == SV_SIGNER_HASH_X) rem_hx |= (uint64_t)1 << g;
    else if (type == SV_SIGNER_PRE_AUTH_TX && sv_txc_rows_equal(b.key + 32 * k, b.digest)) {
      const uint32_t w = sw[g];
      total += clamp && w > 255u ? 255u : w;
      done = total >= (int64_t)needed;
    }
  }
  if (!done && rem_hx) {
    SV_NOUNROLL for (uint32_t s = 0; s < ns && !done; ++s) {
      const uint32_t h = sv_txc_ld32(b.hint + 4 * (b.s0 + s));
      const uint32_t len = b.sig_len ? b.sig_len[b.s0 + s] : 64u;
      SV_NOUNROLL for (uint64_t m = rem_hx; m; m &= m - 1) {
        const uint32_t g = (uint32_t)__builtin_ctzll(m);
        const uint8_t* row = b.key + 32 * (uint64_t)sk[g];
        if (sv_txc_ld32(row + 28) != h) continue;
        if (!SHA) {
          r.ok = SV_TXCHECK_DEFER;
          r.total = 0;
          r.used = 0;
          return r;
        }
        if (!sv_txc_hashx(b.sig + 64 * (b.s0 + s), len > 64u ? 64u : len, row)) continue;
        r.used |= (uint64_t)1 << s;
        const uint32_t w = sw[g];
        total += clamp && w > 255u ? 255u : w;
        done = total >= (int64_t)needed;
        rem_hx &= ~((uint64_t)1 << g);
        break;
      }
    }
  }
  if (!done && rem_ed)
    done = sv_txc_pair_pass(b, b.pair_sig, b.pair_key, b.pair_verdict, b.p0, b.p1, ns, sw, sk, needed, clamp, rem_ed,
                            &total, &r.used);
  if (!done && rem_pl) {
    if (!PAYLOAD) {
      r.ok = SV_TXCHECK_DEFER;
      r.total = 0;
      r.used = 0;
      return r;
    }
    done = sv_txc_pair_pass(b, b.ppair_sig, b.ppair_key, b.ppair_verdict, b.pp0, b.pp1, ns, sw, sk, needed, clamp,
                            rem_pl, &total, &r.used);
  }
  r.ok = done ? 1u : 0u;
  r.total = total > (int64_t)0xffffffffu ? 0xffffffffu : (uint32_t)total;
  return r;
}
