// Transaction contents hash for one lane: SHA-256(prefix || body) with the
// prefix applied in place (nobody materialises the concatenation).
//
//   kind 0 (V1)        prefix = networkID || 00 00 00 02
//   kind 1 (V0)        prefix = networkID || 00 00 00 02 || 00 00 00 00
//   kind 2 (fee bump)  prefix = networkID || 00 00 00 05
//
// The prefix is 9 or 10 dwords, shorter than a block, so there is no midstate;
// schedule word j of block b is dword 16 b + j - P of the body.  The body is
// read in 16-dword windows that start 12 dwords before the block (a whole
// number of 16-byte quads for both P): word j is window dword j + 3 (P = 9) or
// j + 2 (P = 10), one select per word, every register index static.  The last
// quad of a window is the first of the next, so a block costs four loads.
//
// SV_TX_QUADS   16-byte loads; the body's start is 16-byte aligned (an aligned
//               quad never crosses a page, so the quad that holds the last
//               valid byte is safe to read whole; quads past it are not read)
// SV_TX_DWORDS  any alignment on the device: aligned dwords and a funnel shift
// SV_TX_BYTES   the host: reads exactly the body's bytes
#pragma once

#include "hash_dev.h"

#if !defined(__HIPCC__)
#include <string.h>
#endif

enum { SV_TX_QUADS = 0, SV_TX_DWORDS = 1, SV_TX_BYTES = 2 };

// Body dwords [4 q, 4 q + 4) (little-endian) into r[0..3]; dwords that start
// at or past L are 0, bytes past L in the last one are unspecified in
// SV_TX_QUADS (the caller masks them) and 0 otherwise.
template <int LOAD>
SV_HD void sv_tx_quad(uint32_t* r, const uint8_t* body, uint32_t L, int64_t q) {
  r[0] = r[1] = r[2] = r[3] = 0u;
  if (q < 0 || 16 * q >= (int64_t)L) return;
#if defined(__HIPCC__)
  if (LOAD == SV_TX_QUADS) {
    const uint4 v = ((const uint4*)body)[q];
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    return;
  }
#endif
  SV_UNROLL for (int k = 0; k < 4; ++k) {
    const int64_t o = 16 * q + 4 * k, avail = (int64_t)L - o;
    if (avail <= 0) continue;
#if defined(__HIPCC__)
    r[k] = sv_ld32(body + o, avail);
#else
    uint32_t v = 0;
    memcpy(&v, body + o, avail < 4 ? (size_t)avail : 4u);  // (little-endian hosts)
    r[k] = v;
#endif
  }
}

// out: the digest as 8 words whose little-endian bytes are the digest bytes;
// nid: the network id the same way.  kind > 2 hashes as kind 2.
template <int LOAD>
SV_HD void sv_txhash(uint32_t out[8], const uint32_t nid[8], const uint8_t* body, uint32_t L, uint32_t kind) {
  uint32_t st[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                    0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  const bool v0 = kind == 1;
  const int64_t P = v0 ? 10 : 9;  // prefix dwords
  const uint64_t total = 4 * (uint64_t)P + L;
  const uint64_t nb = (total + 9 + 63) / 64;
  uint32_t r[20];  // body dwords 16 b - 12 .. 16 b + 7
  r[0] = r[1] = r[2] = r[3] = 0u;
  SV_NOUNROLL for (uint64_t b = 0; b < nb; ++b) {
    SV_UNROLL for (int k = 1; k < 5; ++k) sv_tx_quad<LOAD>(r + 4 * k, body, L, 4 * (int64_t)b - 3 + k);
    // a block that lies inside the body needs no prefix, mask, padding or length
    const bool plain = b > 0 && 64 * (b + 1) <= total;
    uint32_t w[16];
    SV_UNROLL for (int j = 0; j < 16; ++j) {
      uint32_t v = v0 ? r[j + 2] : r[j + 3];
      if (!plain) {
        const int64_t s = 16 * (int64_t)b + j;  // dword of the padded message
        const int64_t avail = (int64_t)L - 4 * (s - P);
        if (s < 8) v = nid[j];
        else if (s == 8) v = sv_bswap32b(kind >= 2 ? 5u : 2u);
        else if (s < P) v = 0u;
        else if (avail <= 0) v = avail == 0 ? 0x80u : 0u;
        else if (avail < 4) v = (v & ((1u << (8u * (uint32_t)avail)) - 1u)) | (0x80u << (8u * (uint32_t)avail));
      }
      v = sv_bswap32b(v);
      if (b + 1 == nb && j == 14) v = (uint32_t)(total >> 29);
      if (b + 1 == nb && j == 15) v = (uint32_t)(total << 3);
      w[j] = v;
    }
    sha256_compress(st, w);
    SV_UNROLL for (int k = 0; k < 4; ++k) r[k] = r[16 + k];
  }
  SV_UNROLL for (int i = 0; i < 8; ++i) out[i] = sv_bswap32b(st[i]);
}
