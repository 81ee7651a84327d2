// The verdict cache of a device slot (include/stellar_sigverify.h
// sv_set_verdict_cache): the twin of stellar-core's gVerifySigCache
// (PubKeyUtils::verifySig, src/crypto/SecretKey.cpp:446-466) for the calls whose
// signatures never leave the device.  Written once, for the gfx950 kernels
// (sv_vcache.hip) and for the host (tests/native/vcache_core.cpp, the model the
// tests predict the table with): SV_HD is __host__ __device__ under hipcc and
// static inline under g++.
//
// Key       the reference's cache key, BLAKE2b-256(pk || sig || msg)
//           (verifySigCacheKey, :50-61), all 32 bytes, as eight little-endian
//           words k[0..8).
// Geometry  sets of SV_VC_WAYS (4) entries, a power of two of them; the set is
//           k[0] & (sets - 1), the way a search starts at is k[1] & 3.  The
//           smallest table is one set.
// Entry     48 bytes: the key, a state word, three unused words.  State
//           SV_VC_HOLDS0 / SV_VC_HOLDS1: the entry holds verdict 0 / 1 for its
//           key (rejects are cached like accepts, :464-466).  Every other state
//           -- all-zero memory included -- holds nothing: a lookup misses it
//           (the item is verified) and an insert may take it.  A hit needs all
//           eight key words equal; no shorter tag decides anything.
// Insert    A pass over a batch is probe -> verify the misses -> insert, three
//           stages separated by kernel boundaries on the slot's one stream, so
//           every lookup of a pass sees the table as it was when the pass began.
//           A missed item's candidate slot is the first way of its set that
//           holds nothing, searched in rotation from its start way; if every
//           way holds a verdict, the start way itself (its entry is evicted).
//           Every missed item then does atomicMin(claim[slot], item index); in
//           a second kernel the item whose index stands in the claim word writes
//           the whole entry and resets the claim word to SV_VC_UNCLAIMED; an
//           item that lost its claim is not inserted in this pass (it counts as
//           `dropped`).  One writer per slot per pass, no entry assembled from
//           two writers, and the table after a pass a function of the table
//           before it and of the batch in item order -- never of arrival order.
//           Two items with the same key have the same candidate, so a key is
//           never in two slots.  Only verdict bytes 0 and 1 are inserted.
// Cost      52 bytes of device memory per entry (48 + the 4-byte claim word).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "sv_common.h"

#define SV_VC_WAYS 4
#define SV_VC_ENTRY_WORDS 12
#define SV_VC_HOLDS0 0x56430A50u
#define SV_VC_HOLDS1 0x56430A51u
#define SV_VC_UNCLAIMED 0xFFFFFFFFu
#define SV_VC_NO_SLOT 0xFFFFFFFFu
// the largest table (2^24 entries, 832 MB with its claim words) and the largest batch the cache serves (a claim
// word holds an item index below SV_VC_UNCLAIMED); a larger launch runs uncached
#define SV_VC_MAX_ENTRIES ((uint64_t)1 << 24)
#define SV_VC_MAX_ITEMS ((uint64_t)0xFFFFFFFFu)

struct sv_vc_entry {
  uint32_t key[8];
  uint32_t state;
  uint32_t unused[3];
};

// What the kernels of one pass work on (host memory; the arrays device memory, every one 16-byte aligned).
// The compacted arrays hold n_miss <= n rows, the misses in ascending item order.
struct sv_vc_args {
  sv_vc_entry* tab;      // 4 * sets
  uint32_t* claim;       // 4 * sets, SV_VC_UNCLAIMED between passes
  uint64_t sets;
  uint64_t* counters;    // hits | inserted | dropped | the pass's miss count
  // the batch
  const void* pk;        // n x 32
  const void* sig;       // n x 64
  const void* msg;       // fixed32: n x 32 at any alignment; else the bytes off / len point into
  const uint64_t* off;   // n, or null with fixed_len != 0: item i's message is msg + i * fixed_len
  const uint32_t* len;
  uint32_t fixed_len;
  uint64_t n;
  const uint32_t* keys;  // n x 8 words: the cache keys (sv_launch_hash kind 0)
  uint8_t* verdict;      // n
  uint8_t* hit;          // n, or null
  // the compaction workspace
  uint8_t* missed;       // n
  uint64_t* psum;        // blocks(n) + 1
  uint32_t* miss;        // n: the missed items, ascending
  uint32_t* slot;        // n: miss j's candidate slot (SV_VC_NO_SLOT: not inserted)
  void* cpk;             // n x 32
  void* csig;            // n x 64
  void* cmsg;            // n x 32 (fixed_len == 32)
  uint64_t* coff;        // n (every other form)
  uint32_t* clen;        // n
  uint8_t* cverdict;     // n: what the verify launch over the compacted arrays wrote
};

SV_HD bool sv_vc_holds(uint32_t state) { return state == SV_VC_HOLDS0 || state == SV_VC_HOLDS1; }

SV_HD uint64_t sv_vc_set(const uint32_t* k, uint64_t sets) { return (uint64_t)k[0] & (sets - 1); }
SV_HD uint32_t sv_vc_start(const uint32_t* k) { return k[1] & (SV_VC_WAYS - 1); }

SV_HD bool sv_vc_key_equal(const sv_vc_entry& e, const uint32_t* k) {
  uint32_t d = 0;
  SV_UNROLL for (int w = 0; w < 8; ++w) d |= e.key[w] ^ k[w];
  return d == 0;
}

// -1: a miss; else the cached verdict (0 or 1)
SV_HD int sv_vc_lookup(const sv_vc_entry* tab, uint64_t sets, const uint32_t* k) {
  const sv_vc_entry* set = tab + SV_VC_WAYS * sv_vc_set(k, sets);
  int v = -1;
  SV_UNROLL for (int w = 0; w < SV_VC_WAYS; ++w)
    if (sv_vc_holds(set[w].state) && sv_vc_key_equal(set[w], k)) v = (int)(set[w].state - SV_VC_HOLDS0);
  return v;
}

// the slot a missed key may claim
SV_HD uint64_t sv_vc_candidate(const sv_vc_entry* tab, uint64_t sets, const uint32_t* k) {
  const uint64_t base = SV_VC_WAYS * sv_vc_set(k, sets);
  const uint32_t start = sv_vc_start(k);
  uint32_t pick = start;
  bool found = false;
  SV_UNROLL for (uint32_t r = 0; r < SV_VC_WAYS; ++r) {
    const uint32_t w = (start + r) & (SV_VC_WAYS - 1);
    if (!found && !sv_vc_holds(tab[base + w].state)) {
      pick = w;
      found = true;
    }
  }
  return base + pick;
}

// the winner's store of slot s: key k with verdict v (0 or 1)
SV_HD void sv_vc_store(sv_vc_entry* tab, uint64_t s, const uint32_t* k, uint32_t v) {
  SV_UNROLL for (int w = 0; w < 8; ++w) tab[s].key[w] = k[w];
  tab[s].state = SV_VC_HOLDS0 + v;
  SV_UNROLL for (int w = 0; w < 3; ++w) tab[s].unused[w] = 0;
}

// Feed     Rows that arrive WITH their verdicts (vjournal.h: what the slot's
//          latency lane verified) take the insert half of a pass alone, in
//          journal order: a row whose key the table holds is `present` and
//          changes nothing (it evicts nothing and names no slot); every other
//          row names its candidate slot and claims it with its row index, and
//          in a second kernel the winner stores the entry; a loser is dropped.
//          The same one-writer rule, so the table after a drain is a function of
//          the table before it and of the rows in journal order.
//
// What the two feed kernels work on (host memory; the arrays device memory, 16-byte aligned).
struct sv_vc_feed_args {
  sv_vc_entry* tab;
  uint32_t* claim;
  uint64_t sets;
  uint64_t* counters;      // present | inserted | dropped of the drains
  const uint32_t* keys;    // n x 8 words
  const uint8_t* verdict;  // n
  uint32_t* slot;          // n: row j's candidate slot (SV_VC_NO_SLOT: present, or no verdict byte)
  uint64_t n;
};

// the slot a fed row with verdict byte v names: none if v is no verdict or the table holds the key
SV_HD uint32_t sv_vc_feed_slot(const sv_vc_entry* tab, uint64_t sets, const uint32_t* k, uint8_t v, bool* present) {
  *present = false;
  if (v > 1) return SV_VC_NO_SLOT;
  if (sv_vc_lookup(tab, sets, k) >= 0) {
    *present = true;
    return SV_VC_NO_SLOT;
  }
  return (uint32_t)sv_vc_candidate(tab, sets, k);
}
