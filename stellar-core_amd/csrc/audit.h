// The verdict audit (include/stellar_sigverify.h sv_set_audit):
// which rows of a verify launch are verified again by the textbook equation
// (verify_core.h sv_verify_core), how many of them a launch may spend, and what
// a disagreement leaves behind.  Each rule is stated once, here, for the
// kernels (sv_audit.hip), the CPU form (sv_cpu.cpp sv_audit_batch_cpu), the
// engine (bulk.h audit_locked) and the host model of the tests.
//
//   the pick     row i of audited launch seq is picked iff
//                  (what & SV_AUDIT_REJECTS) and verdict[i] == 0, or
//                  (what & SV_AUDIT_SAMPLE) and sv_audit_mix(seed, seq, i) % one_in == 0
//   the budget   picks in ascending row order; the first `budget` of a launch
//                are audited, the rest count as over_budget
//   the record   one sv_audit_record per audited row whose two verdicts differ,
//                in row order, into a ring of SV_AUDIT_RING records that is
//                never overwritten: what does not fit counts as records_lost
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/stellar_sigverify.h"
#include "sv_common.h"

#define SV_AUDIT_BUDGET_DEFAULT ((uint64_t)65536)
#define SV_AUDIT_WHAT_MASK (SV_AUDIT_REJECTS | SV_AUDIT_SAMPLE | SV_AUDIT_STRICT)
// rows of one audited launch: the pick list holds 32-bit row indices
#define SV_AUDIT_MAX_ROWS (((uint64_t)1 << 32) - 1)

// The slot's device counters (64-bit words); the kernels add to them with plain adds from one lane.
#define SV_AC_AUDITED 0
#define SV_AC_REJECTS 1
#define SV_AC_OVER 2
#define SV_AC_MISMATCH 3
#define SV_AC_LOST 4
#define SV_AC_HELD 5   // records in the ring
#define SV_AC_M 6      // the launch in progress: its audited rows (picks clipped to the budget)
#define SV_AC_PICKS 7  // ... and its picks
#define SV_AC_WORDS 8

static_assert(sizeof(sv_audit_record) == 632, "record layout: 24 + 32 + 64 + 512 bytes, no padding");

// splitmix64's output function
SV_HD uint64_t sv_audit_fin(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// (seed, seq) -> the launch's stream, then row i of it: two splitmix64 steps
SV_HD uint64_t sv_audit_mix(uint64_t seed, uint64_t seq, uint64_t i) {
  const uint64_t s = sv_audit_fin(seed + 0x9E3779B97F4A7C15ull * (seq + 1));
  return sv_audit_fin((s ^ i) + 0x9E3779B97F4A7C15ull);
}

SV_HD bool sv_audit_pick(uint32_t what, uint32_t one_in, uint64_t seed, uint64_t seq, uint64_t i, uint8_t verdict) {
  if ((what & SV_AUDIT_REJECTS) && verdict == 0) return true;
  if ((what & SV_AUDIT_SAMPLE) && one_in != 0 && sv_audit_mix(seed, seq, i) % one_in == 0) return true;
  return false;
}

SV_HD uint64_t sv_audit_budget(uint64_t budget) { return budget ? budget : SV_AUDIT_BUDGET_DEFAULT; }
// audited rows of a launch with `picks` picks
SV_HD uint64_t sv_audit_clip(uint64_t picks, uint64_t budget) { return picks < budget ? picks : budget; }

// The ring slot of the launch's rank-th mismatch (row order) with `held` records in the ring before the launch,
// or SV_AUDIT_RING: lost.
SV_HD uint32_t sv_audit_ring_slot(uint64_t held, uint64_t rank) {
  return held + rank < SV_AUDIT_RING ? (uint32_t)(held + rank) : (uint32_t)SV_AUDIT_RING;
}

// One record from the row's bytes (msg may be null where len == 0).
SV_HD void sv_audit_record_fill(sv_audit_record* r, uint64_t seq, uint64_t row, uint8_t engine, uint8_t audit,
                                uint8_t cpu, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t len) {
  r->seq = seq;
  r->row = row;
  r->msg_len = len;
  r->engine_verdict = engine;
  r->audit_verdict = audit;
  r->cpu_verdict = cpu;
  r->flags = len > SV_AUDIT_MSG_MAX ? (uint8_t)SV_AUDIT_REC_TRUNCATED : (uint8_t)0;
  for (int k = 0; k < 32; ++k) r->pk[k] = pk[k];
  for (int k = 0; k < 64; ++k) r->sig[k] = sig[k];
  const uint32_t keep = len < SV_AUDIT_MSG_MAX ? len : (uint32_t)SV_AUDIT_MSG_MAX;
  for (uint32_t k = 0; k < keep; ++k) r->msg[k] = msg[k];
  for (uint32_t k = keep; k < SV_AUDIT_MSG_MAX; ++k) r->msg[k] = 0;
}

// One audit pass, for the launchers of sv_audit.hip (host memory; the arrays device memory).
struct sv_audit_args {
  const void* pk;   // n x 32, 16-byte aligned
  const void* sig;  // n x 64, 16-byte aligned
  const void* msg;
  const uint64_t* off;  // fixed_len == 0
  const uint32_t* len;
  uint32_t fixed_len;
  uint32_t what, one_in;
  uint32_t dissent;  // SV_DBG_AUDIT_DISSENT: the first audited row's audit byte is inverted
  uint64_t seed, seq, n, budget;
  const uint8_t* verdict;  // the n bytes under audit
  uint64_t* psum;          // sv_audit_psum_bytes(n)
  uint32_t* list;          // min(n, budget) picked rows, ascending
  uint8_t* av;             // ... and their audit bytes
  uint64_t* counters;      // SV_AC_WORDS
  sv_audit_record* ring;   // SV_AUDIT_RING
  void* ws;                // sv_audit_ws_bytes(grid): one table of -A per lane
  const void* btab;        // the slot's base-point table
  unsigned grid;           // workgroups of the verify kernel (sv_audit_grid)
};
