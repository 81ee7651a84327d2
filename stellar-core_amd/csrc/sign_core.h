// Per-lane ed25519 signing core (one lane = one key or one signature), one
// text for gfx950 (sv_sign.hip) and the host (the CPU path sv_cpu.cpp, the
// test builds under tests/native).
//
// Output is byte-exact with libsodium 1.0.18 crypto_sign_seed_keypair and
// crypto_sign_detached (RFC 8032 deterministic signing), the functions behind
// stellar-core's SecretKey::fromSeed / SecretKey::sign
// (src/crypto/SecretKey.cpp:134-146, 286, 309):
//
//   az = SHA-512(seed), az[0..31] clamped;  a = az[0..31] mod L
//   prefix = az[32..63];  pk = encode([a]B)
//   r = SHA-512(prefix || M) mod L;  R = encode([r]B)
//   h = SHA-512(R || pk || M) mod L;  S = (h a + r) mod L;  sig = R || S
//
// [s]B runs over the comb tables of B (comb.h: entry (j, e) = e 256^j B in
// cached form): s < 2^253 is recoded into 32 signed radix-256 digits and the
// 32 entries are added up, starting from the identity, with no doubling.  A
// negative digit swaps the entry's (Y+X, Y-X) pair at load time and negates
// 2dT inside the addition (ge_add_preswapped's neg).
//
// NOT constant-time: the table addresses follow the secret digits.  See the
// header's notes on sv_ed25519_sign_batch for what this signer is meant for.
#pragma once

#include "comb_core.h"

// Expanded key record: a (8 words) | prefix (8 words) | pk (8 words).
#define SV_SIGN_REC_DW 24

// P = [s]B for s < 2^253 (8 little-endian words); ctab: the comb tables of B
// (SV_CB_DW dwords, 16-byte aligned).  The digit string stays packed and is
// consumed from the top (sc_pop_top), so no array is indexed at run time.
SV_HD void sv_fixed_base_p3(ge_p3& P, const uint32_t s[8], const uint32_t* ctab) {
  uint32_t d[8];
  sc_digits_r256(d, s);
  fe_0(P.X); fe_1(P.Y); fe_1(P.Z); fe_0(P.T);
  ge_p1p1 Q;
  SV_NOUNROLL for (int j = SV_CB_POS - 1; j >= 0; --j) {
    const int32_t e = sc_pop_top(d, 8);
    const bool neg = e < 0;
    const sv_u4* ent =
        (const sv_u4*)ctab + ((uint32_t)j * SV_CB_ENT + (uint32_t)(neg ? -e : e)) * (SV_CE_DW / 4);
    fe qa, qb, qz, qt;
    sv_load_fe3(qa, ent + (neg ? 3 : 0), 1);
    sv_load_fe3(qb, ent + (neg ? 0 : 3), 1);
    sv_load_fe3(qz, ent + 6, 1);
    sv_load_fe3(qt, ent + 9, 1);
    ge_add_preswapped(Q, P, qa, qb, qz, qt, neg, false);
    ge_p1p1_to_p3_opt(P, Q, j != 0);
  }
}

// enc = encode([s]B), s < 2^253
SV_HD void sv_fixed_base_encode(uint32_t enc[8], const uint32_t s[8], const uint32_t* ctab) {
  ge_p3 P;
  sv_fixed_base_p3(P, s, ctab);
  ge_p2_tobytes(enc, P.X, P.Y, P.Z);
}

// Message bytes m[mi, mi + 8) as a big-endian SHA-512 word with the padding
// folded in (0x80 at mlen, zeros after).  Device: sv_msg_word, which reads
// only the aligned dwords that hold at least one message byte.  Host: byte
// reads of the message alone, so a message may end where its allocation ends.
SV_HD uint64_t sv_sign_msg_word(const uint8_t* m, uint32_t mlen, uint32_t mi) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sv_msg_word(m, mlen, mi);
#else
  uint64_t v = 0;
  for (uint32_t k = 0; k < 8; ++k) {
    const uint64_t idx = (uint64_t)mi + k;
    const uint64_t b = idx < mlen ? m[idx] : (idx == mlen ? 0x80u : 0u);
    v = (v << 8) | b;
  }
  return v;
#endif
}

// SHA-512(head || M) for a head of HW 8-byte words (HW = 4: the nonce's
// prefix; HW = 8: R || pk) and a message of any length and alignment: the
// 32- and 64-byte-head forms of sha512_ram_var.  Message byte j sits at
// stream offset 8 HW + j; word 15 of the last block is the bit length.
template <int HW>
SV_HD void sha512_head_var(uint32_t out[16], const uint32_t* head, const uint8_t* m, uint32_t mlen) {
  uint64_t st[8], w[16];
  sha512_init(st);
  const uint64_t total = (uint64_t)(8 * HW) + mlen;
  const uint32_t nblocks = (uint32_t)((total + 16u + 1u + 127u) / 128u);
  SV_NOUNROLL for (uint32_t blk = 0; blk < nblocks; ++blk) {
    SV_UNROLL for (int t = 0; t < 16; ++t) {
      uint64_t v;
      if (t < HW && blk == 0) {
        v = sv_be64(head[2 * t], head[2 * t + 1]);
      } else {
        v = sv_sign_msg_word(m, mlen, 128u * blk + 8u * (uint32_t)t - 8u * (uint32_t)HW);
      }
      if (t == 15 && blk == nblocks - 1) v = total * 8u;
      w[t] = v;
    }
    sha512_compress(st, w);
  }
  sha512_digest_le(out, st);
}

// Key expansion: rec = a | prefix | pk from a 32-byte seed.
SV_HD void sv_sign_expand(uint32_t rec[SV_SIGN_REC_DW], const uint32_t seed[8], const uint32_t* ctab) {
  uint32_t az[16], wide[16], a[8], pk[8];
  sha512_words<8>(az, seed);
  az[0] &= ~7u;
  az[7] &= 0x7fffffffu;
  az[7] |= 0x40000000u;
  SV_UNROLL for (int i = 0; i < 16; ++i) wide[i] = i < 8 ? az[i] : 0u;
  sc_reduce512(a, wide);  // [a]B == [clamped]B: B has order L
  sv_fixed_base_encode(pk, a, ctab);
  SV_UNROLL for (int i = 0; i < 8; ++i) {
    rec[i] = a[i];
    rec[8 + i] = az[8 + i];
    rec[16 + i] = pk[i];
  }
}

// One signature from an expanded key record.
SV_HD void sv_sign_msg(uint32_t sig[16], const uint32_t rec[SV_SIGN_REC_DW], const uint8_t* m, uint32_t mlen,
                       const uint32_t* ctab) {
  uint32_t wide[16], r[8], R[8], h[8], S[8];
  sha512_head_var<4>(wide, rec + 8, m, mlen);
  sc_reduce512(r, wide);
  sv_fixed_base_encode(R, r, ctab);
  uint32_t head[16];
  SV_UNROLL for (int i = 0; i < 8; ++i) {
    head[i] = R[i];
    head[8 + i] = rec[16 + i];
  }
  sha512_head_var<8>(wide, head, m, mlen);
  sc_reduce512(h, wide);
  sc_muladd(S, h, rec, r);
  SV_UNROLL for (int i = 0; i < 8; ++i) {
    sig[i] = R[i];
    sig[8 + i] = S[i];
  }
}
