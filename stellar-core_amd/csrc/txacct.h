// Checks by account (include/stellar_sigverify.h sv_txaccounts): the expansion
// of an account table plus per-body account lists and per-check (account,
// level) references into the explicit tables sv_ed25519_check_txbodies* takes
// -- each body's candidate keys and payload candidates, each check's signer
// list and needed weight.  Written once, for the gfx950 kernels
// (sv_txacct.hip) and for the host (sv_cpu.cpp, the planner in host_image.h):
// SV_HD is __host__ __device__ under hipcc and static inline under g++.
//
// The expansion (TransactionFrame::checkSignature builds the same list from
// the account entry: the master key with weight thresholds[0] if that is
// non-zero, then acc.signers):
//   account a adds to a body's key list       its key iff thresholds[a][0] > 0,
//                                             then its signers of another type
//                                             than 3, in list order
//   ... and to the body's payload candidates  its type-3 signers, in list order
//   a check's signer list                     (ED25519, master weight, master
//                                             row) iff the master weight is
//                                             > 0, then the signers in list
//                                             order; a signer's key index is the
//                                             global row it got in the body's
//                                             key list / payload candidates
// A signer's row is the account's first row in the body plus its RANK, its
// position among the account's rows of its list (the master, if any, is rank 0
// of the key list).  The ranks depend on the account alone and are made once
// per account (sv_acct_count), not once per use.
//
// Nothing here trusts an index: every CSR range is clamped to its array, an
// account index at or past the table contributes nothing, a check that names
// no account of its body has no signer (and is therefore false), a payload
// index past the payload table reads as the empty payload, and no row is
// written at or past the output's row counts.  Only ranges are clamped, not
// overlaps: with a non-monotonic asigner_begin two accounts' signer ranges
// overlap and their lanes both write those signers' ranks -- inside the
// workspace, and the stores that follow stay inside the row counts, but which
// rank wins is then not a function of the input.  (The host forms refuse such
// a table.)
#pragma once

#include <stdint.h>

#include "sv_common.h"

#if !defined(__HIPCC__)
#include <string.h>
#endif

struct sv_acct_tab {       // the account table
  const uint8_t* key;      // na x 32
  const uint8_t* thr;      // na x 4: master weight, low, med, high
  union {
    const uint64_t* sbeg;  // na + 1
    // The kStride instantiations (an account store's replica: acctstore.h, sv_txstore.hip) read this word as scnt:
    // rows of a fixed stride of SV_ACCT_STRIDE signers, account a's signers at SV_ACCT_STRIDE * a, scnt[a] of
    // them.  The caller picks the instantiation (sv_launch_acct_fill_stride); the struct, and with it the CSR
    // kernels' arguments and code, are what they were without the store.
    const uint32_t* scnt;  // na
  };
  const uint8_t* stype;    // ns
  const uint32_t* sweight; // ns
  const uint8_t* skey;     // ns x 32
  const uint32_t* spay;    // ns: index into pay / plen (type 3 only)
  const uint8_t* pay;      // np x 64, rows zero-padded
  const uint8_t* plen;     // np
  uint64_t na, ns, np;
};
#define SV_ACCT_STRIDE 20  // MAX_SIGNERS of an account entry

struct sv_acct_use {       // who refers to it
  const uint64_t* ebeg;    // nb + 1: body t's account entries (bacct_begin)
  const uint32_t* eacct;   // ne: account index per entry (bacct)
  const uint64_t* cbeg;    // nb + 1: body t's checks
  const uint32_t* cacct;   // nc: position inside the body's entries
  const uint8_t* clevel;   // nc: 0 (needed from cneed) or 1..3 (the account's threshold)
  const int32_t* cneed;    // nc (read at level 0; may be null when no check has level 0)
  uint64_t nb, ne, nc;
};

struct sv_acct_out {       // the explicit tables
  uint64_t* key_begin;     // nb + 1
  uint64_t* pkey_begin;    // nb + 1
  uint64_t* signer_begin;  // nc + 1
  int32_t* check_needed;   // nc
  uint8_t* key;            // nk x 32
  uint8_t* pkey;           // nq x 32
  uint8_t* ppay;           // nq x 64
  uint8_t* plen;           // nq
  uint8_t* gtype;          // ng
  uint32_t* gweight;       // ng
  uint32_t* gkey;          // ng
  uint64_t nk, nq, ng;     // rows the arrays hold
};

SV_HD uint64_t sv_acct_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

// n16 16-byte pieces; both ends 16-byte aligned on the device
SV_HD void sv_acct_copy(uint8_t* d, const uint8_t* s, int n16) {
#if defined(__HIP_DEVICE_COMPILE__)
  SV_UNROLL for (int i = 0; i < n16; ++i) ((uint4*)d)[i] = ((const uint4*)s)[i];
#else
  memcpy(d, s, 16 * (size_t)n16);
#endif
}
SV_HD void sv_acct_zero(uint8_t* d, int n16) {
#if defined(__HIP_DEVICE_COMPILE__)
  SV_UNROLL for (int i = 0; i < n16; ++i) ((uint4*)d)[i] = make_uint4(0, 0, 0, 0);
#else
  memset(d, 0, 16 * (size_t)n16);
#endif
}

// account a's signers [*s0, *s1) and whether its master key is a signer
template <bool kStride = false>
SV_HD uint32_t sv_acct_signers(const sv_acct_tab& T, uint64_t a, uint64_t* s0, uint64_t* s1) {
  if (kStride) {
    *s0 = SV_ACCT_STRIDE * a;
    *s1 = *s0 + sv_acct_min(T.scnt[a], SV_ACCT_STRIDE);
  } else {
    *s1 = sv_acct_min(T.sbeg[a + 1], T.ns);
    *s0 = sv_acct_min(T.sbeg[a], *s1);
  }
  return T.thr[4 * a] != 0 ? 1u : 0u;
}

// Once per account: acnt[2a] the rows it adds to a key list, acnt[2a + 1] to
// the payload candidates (their sum: the signers of a check on it), and every
// signer's rank.
template <bool kStride = false>
SV_HD void sv_acct_count(const sv_acct_tab& T, uint64_t a, uint32_t* acnt, uint32_t* rank) {
  uint64_t s0, s1;
  uint32_t nk = sv_acct_signers<kStride>(T, a, &s0, &s1), nq = 0;
  SV_NOUNROLL for (uint64_t s = s0; s < s1; ++s) rank[s] = T.stype[s] == 3 ? nq++ : nk++;
  acnt[2 * a] = nk;
  acnt[2 * a + 1] = nq;
}

// body t's account entries [*e0, *e1)
SV_HD void sv_acct_entries(const sv_acct_use& U, uint64_t t, uint64_t* e0, uint64_t* e1) {
  *e1 = sv_acct_min(U.ebeg[t + 1], U.ne);
  *e0 = sv_acct_min(U.ebeg[t], *e1);
}

// the rows of body t's key list and payload candidates
SV_HD void sv_acct_body_count(const sv_acct_tab& T, const sv_acct_use& U, const uint32_t* acnt, uint64_t t,
                              uint32_t* nk, uint32_t* nq) {
  uint64_t e0, e1;
  sv_acct_entries(U, t, &e0, &e1);
  uint32_t k = 0, q = 0;
  SV_NOUNROLL for (uint64_t e = e0; e < e1; ++e) {
    const uint64_t a = U.eacct[e];
    if (a >= T.na) continue;
    k += acnt[2 * a];
    q += acnt[2 * a + 1];
  }
  *nk = k;
  *nq = q;
}

// The entry check c of body t names (*e), and its account; T.na: none.
SV_HD uint64_t sv_acct_check_account(const sv_acct_tab& T, const sv_acct_use& U, uint64_t t, uint64_t c, uint64_t* e) {
  uint64_t e0, e1;
  sv_acct_entries(U, t, &e0, &e1);
  const uint64_t p = U.cacct[c];
  *e = e0;
  if (p >= e1 - e0) return T.na;
  *e = e0 + p;
  return sv_acct_min(U.eacct[e0 + p], T.na);
}

// check c of body t: its number of signers and its needed weight
SV_HD uint32_t sv_acct_check_count(const sv_acct_tab& T, const sv_acct_use& U, const uint32_t* acnt, uint64_t t,
                                   uint64_t c, int32_t* needed) {
  uint64_t e;
  const uint64_t a = sv_acct_check_account(T, U, t, c, &e);
  const uint32_t lvl = U.clevel[c] < 3 ? U.clevel[c] : 3u;
  if (lvl == 0) *needed = U.cneed ? U.cneed[c] : 0;
  else *needed = a < T.na ? (int32_t)T.thr[4 * a + lvl] : 0;
  return a < T.na ? acnt[2 * a] + acnt[2 * a + 1] : 0u;
}

// Item j of account a (its master key, if a signer, is item 0, then its
// signers) as a row of a body's key list or payload candidates; krow / qrow:
// the account's first row in either.
template <bool kStride = false>
SV_HD void sv_acct_fill_row(const sv_acct_tab& T, const uint32_t* rank, uint64_t a, uint64_t j, uint64_t krow,
                            uint64_t qrow, const sv_acct_out& O) {
  uint64_t s0, s1;
  const uint32_t hm = sv_acct_signers<kStride>(T, a, &s0, &s1);
  if (j < hm) {
    if (krow < O.nk) sv_acct_copy(O.key + 32 * krow, T.key + 32 * a, 2);
    return;
  }
  const uint64_t s = s0 + (j - hm);
  if (s >= s1) return;
  if (T.stype[s] != 3) {
    const uint64_t row = krow + rank[s];
    if (row < O.nk) sv_acct_copy(O.key + 32 * row, T.skey + 32 * s, 2);
    return;
  }
  const uint64_t row = qrow + rank[s];
  if (row >= O.nq) return;
  sv_acct_copy(O.pkey + 32 * row, T.skey + 32 * s, 2);
  const uint64_t pi = T.spay ? T.spay[s] : T.np;
  if (pi < T.np) {
    sv_acct_copy(O.ppay + 64 * row, T.pay + 64 * pi, 4);
    O.plen[row] = T.plen[pi];
  } else {
    sv_acct_zero(O.ppay + 64 * row, 4);
    O.plen[row] = 0;
  }
}

// ... and as signer g of a check on that account.
template <bool kStride = false>
SV_HD void sv_acct_fill_signer(const sv_acct_tab& T, const uint32_t* rank, uint64_t a, uint64_t j, uint64_t krow,
                               uint64_t qrow, uint64_t g, const sv_acct_out& O) {
  if (g >= O.ng) return;
  uint64_t s0, s1;
  const uint32_t hm = sv_acct_signers<kStride>(T, a, &s0, &s1);
  if (j < hm) {
    O.gtype[g] = 0;
    O.gweight[g] = T.thr[4 * a];
    O.gkey[g] = (uint32_t)krow;
    return;
  }
  const uint64_t s = s0 + (j - hm);
  if (s >= s1) return;
  const uint8_t ty = T.stype[s];
  O.gtype[g] = ty;
  O.gweight[g] = T.sweight[s];
  O.gkey[g] = (uint32_t)((ty == 3 ? qrow : krow) + rank[s]);
}
