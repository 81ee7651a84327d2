// One signature result per transaction body (include/stellar_sigverify.h
// sv_txresults): the fold of a body's check decisions -- check_ok /
// check_used of sv_ed25519_check_txbodies* -- into what
// TransactionFrame::processSignatures, commonValid and checkAllSignaturesUsed
// make of them: the first failing check decides (txBAD_AUTH for the source
// account, the extra signers or a fee bump's fee source; txFAILED with
// opBAD_AUTH for an operation), then "was every signature used".  Written
// once, for the gfx950 kernels (sv_txresult.hip) and for the host
// (sv_cpu.cpp): SV_HD is __host__ __device__ under hipcc and static inline
// under g++.
//
// The reference stops at the first failing check; this fold reads all of them.
// Checks are independent (txcheck.h: a check reads the signatures and writes
// only its own marks), the code depends on the FIRST failure alone and on the
// OR of the marks only when no check failed -- so evaluating the checks behind
// a failing one changes no result.
//
// Nothing here trusts an index: both CSR ranges are clamped to their arrays, a
// check_ok other than 1 is a failure (a value that should never be visible
// there fails closed), a role above 1 reads as SV_TXROLE_OP and unknown flag
// bits are ignored.  (The host forms refuse such roles and flags.)
#pragma once

#include <stdint.h>

#include "sv_common.h"

#define SV_TXRESULT_OK 0
#define SV_TXRESULT_BAD_AUTH 1
#define SV_TXRESULT_OP_BAD_AUTH 2
#define SV_TXRESULT_BAD_AUTH_EXTRA 3
#define SV_TXRESULT_NONE 0xFFFFFFFFu
#define SV_TXROLE_TX 0
#define SV_TXROLE_OP 1
#define SV_TXBODY_SKIP_UNUSED 1

struct sv_txresult_in {
  const uint64_t* check_begin;  // nb + 1
  const uint64_t* sig_begin;    // nb + 1
  const uint8_t* check_ok;      // nc
  const uint64_t* check_used;   // nc
  const uint8_t* check_role;    // nc, or null: every check SV_TXROLE_TX
  const uint8_t* body_flags;    // nb, or null: 0
  uint64_t nb, nc, ns;
};

SV_HD uint64_t sv_txr_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// body t's checks [*c0, *c1), clamped to the check arrays
SV_HD void sv_txresult_checks(const sv_txresult_in& I, uint64_t t, uint64_t* c0, uint64_t* c1) {
  *c1 = sv_txr_min(I.check_begin[t + 1], I.nc);
  *c0 = sv_txr_min(I.check_begin[t], *c1);
}

// the marks a body with its number of signatures must show: ns >= 64 ? ~0 : (1 << ns) - 1
SV_HD uint64_t sv_txresult_want(const sv_txresult_in& I, uint64_t t) {
  const uint64_t s1 = sv_txr_min(I.sig_begin[t + 1], I.ns);
  const uint64_t s0 = sv_txr_min(I.sig_begin[t], s1);
  const uint64_t ns = sv_txr_min(s1 - s0, 64);
  return ns >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << ns) - 1);
}

// One step of the fold, check c (c0 <= c < c1) of a body whose checks begin at c0: *fail is the smallest
// body-local index of a failing check so far (SV_TXRESULT_NONE: none), *used the OR of the marks.  min and OR
// commute, so any order and any split of the checks over lanes gives the same pair.
SV_HD void sv_txresult_step(const sv_txresult_in& I, uint64_t c0, uint64_t c, uint32_t* fail, uint64_t* used) {
  if (I.check_ok[c] != 1) {
    const uint64_t k = c - c0;
    const uint32_t k32 = k < SV_TXRESULT_NONE ? (uint32_t)k : SV_TXRESULT_NONE - 1;
    if (k32 < *fail) *fail = k32;
  }
  *used |= I.check_used[c];
}

// The code of body t from its folded pair.
SV_HD uint8_t sv_txresult_code(const sv_txresult_in& I, uint64_t t, uint64_t c0, uint32_t fail, uint64_t used) {
  if (fail != SV_TXRESULT_NONE) {
    const uint8_t role = I.check_role ? I.check_role[c0 + fail] : (uint8_t)SV_TXROLE_TX;
    return role == SV_TXROLE_TX ? SV_TXRESULT_BAD_AUTH : SV_TXRESULT_OP_BAD_AUTH;
  }
  const uint64_t want = sv_txresult_want(I, t);
  const uint8_t flags = I.body_flags ? I.body_flags[t] : 0;
  if ((used & want) != want && !(flags & SV_TXBODY_SKIP_UNUSED)) return SV_TXRESULT_BAD_AUTH_EXTRA;
  return SV_TXRESULT_OK;
}

// The whole fold of one body (the host, and a lane that owns a body alone).
SV_HD uint8_t sv_txresult_body(const sv_txresult_in& I, uint64_t t, uint32_t* fail_out) {
  uint64_t c0, c1, used = 0;
  uint32_t fail = SV_TXRESULT_NONE;
  sv_txresult_checks(I, t, &c0, &c1);
  SV_NOUNROLL for (uint64_t c = c0; c < c1; ++c) sv_txresult_step(I, c0, c, &fail, &used);
  *fail_out = fail;
  return sv_txresult_code(I, t, c0, fail, used);
}
