// The slot of an account ID in the account store's index (acctstore.h on the
// host, sv_txstore.hip on the device: the same function, so the device finds
// what the host placed).  Account IDs are public keys their owners choose, so
// all eight words go through a seeded multiply-xorshift mix: no prefix, and no
// byte an attacker can steer without knowing the seed, picks the slot.
#pragma once

#include <stdint.h>

#include "sv_common.h"

SV_HD uint64_t sv_acct_hash(const uint32_t w[8], uint64_t seed) {
  uint64_t h = seed;
  SV_UNROLL for (int i = 0; i < 8; ++i) {
    h = (h ^ w[i]) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  h *= 0xD6E8FEB86659FD93ull;
  return h ^ (h >> 32);
}
