// gfx950 check kernels: one SignatureChecker::checkSignature decision per lane
// (txcheck.h), after the hinted pipeline of the same stream has produced the
// bodies' contents hashes (sv_txhash.hip), the (signature, key) pairs
// (sv_txpair.hip) and their verdicts (the verify launch).
//
// One lane per CHECK, not per body: a transaction has one check per operation
// plus its source's, 1 to 100+, so a lane per body would repeat the imbalance
// of the pairing kernels.  Lane c finds its body by an upper-bound binary
// search in check_begin (scan.h sv_csr_owner), replays the check and writes check_ok[c], check_weight[c]
// and check_used[c] with ordinary stores: checks are independent of one
// another, a body's used set is the OR of its checks' masks (the caller's
// job), so there are no atomics and no workgroup waits for another one.
// Device-resident tables are not validated by the host: every CSR range is
// clamped to its array, a key index outside its body matches nothing
// (txcheck.h), and a lane only ever writes its own three outputs.
//
// Two launches.  The SHA-256 a HASH_X signer needs doubles the decision's
// registers, and called out of line it made the common path spill around a
// call it never makes, so the kernel every check runs is
// built without it and defers the rare check that needs it to a second kernel
// behind it on the same stream.  The signed-payload pass goes the same way: in
// the kernel every check runs it cost 20 bytes of scratch at 8 waves/SIMD
// (DESIGN.md 3.13), so that kernel gives up where the pass would have to run --
// the first three stages did not succeed and a type-3 signer is live in a body
// that has payload pairs -- and the second kernel decides the check from the
// start.  Neither has scratch.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "scan.h"
#include "txcheck.h"

#define SV_CHECKBLOCK 256

struct sv_checkparams {
  const uint64_t* sig_begin;     // n_bodies + 1
  const uint64_t* key_begin;     // n_bodies + 1
  const uint64_t* pair_begin;    // n_bodies + 1
  const uint64_t* check_begin;   // n_bodies + 1
  const uint64_t* signer_begin;  // n_checks + 1
  const uint8_t* hint;           // n_sigs x 4
  const uint8_t* sig;            // n_sigs x 64
  const uint8_t* sig_len;        // n_sigs, or nullptr
  const uint8_t* key;            // n_keys x 32
  const uint32_t* pair_sig;      // n_pairs
  const uint32_t* pair_key;
  const uint8_t* pair_verdict;
  const uint8_t* digests;        // n_bodies x 32
  const int32_t* needed;         // n_checks
  const uint8_t* signer_type;    // n_signers
  const uint32_t* signer_weight;
  const uint32_t* signer_key;
  // the payload pairing's output and the candidates' CSR array; ppair_begin == nullptr: no payload pairs in this call
  const uint64_t* ppair_begin;   // n_bodies + 1
  const uint64_t* pkey_begin;    // n_bodies + 1
  const uint32_t* ppair_sig;     // n_ppairs
  const uint32_t* ppair_key;
  const uint8_t* ppair_verdict;
  uint64_t n_ppairs, n_pkeys;
  uint64_t n_bodies, n_sigs, n_keys, n_pairs, n_checks, n_signers;
  uint32_t clamp;
  uint8_t* ok;                   // n_checks
  uint32_t* weight;
  uint64_t* used;
};

__device__ __forceinline__ uint64_t sv_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// One check.  SLOW = false is the kernel every check runs: the decision without
// the SHA-256 and the signed-payload pass, 8 waves/SIMD; a check that meets a
// HASH_X signer whose hint matches, or that needs the payload pass, stores
// SV_TXCHECK_DEFER in check_ok.  SLOW = true, launched right
// after it on the same stream, returns at once for every other check and
// decides the deferred ones with the SHA-256 and the payload pass inlined, at
// whatever registers that takes.
template <bool SLOW>
__device__ __forceinline__ void sv_txcheck_lane(const sv_checkparams& p) {
  const uint64_t c = (uint64_t)blockIdx.x * SV_CHECKBLOCK + threadIdx.x;
  if (c >= p.n_checks) return;
  if (SLOW && p.ok[c] != SV_TXCHECK_DEFER) return;
  const uint64_t t = sv_csr_owner(p.check_begin, p.n_bodies, c);
  sv_txcheck_result r;
  r.ok = 0;
  r.total = 0;
  r.used = 0;
  if (t < p.n_bodies) {  // (else: a check no body owns -- a malformed table -- is false)
    sv_txcheck_body b;
    b.hint = p.hint;
    b.sig = p.sig;
    b.sig_len = p.sig_len;
    b.key = p.key;
    b.pair_sig = p.pair_sig;
    b.pair_key = p.pair_key;
    b.pair_verdict = p.pair_verdict;
    b.digest = p.digests + 32 * t;
    const uint64_t s1 = sv_min64(p.sig_begin[t + 1], p.n_sigs);
    b.s0 = sv_min64(p.sig_begin[t], s1);
    b.ns = (uint32_t)sv_min64(s1 - b.s0, SV_TXCHECK_MAX);
    b.k1 = sv_min64(p.key_begin[t + 1], p.n_keys);
    b.k0 = sv_min64(p.key_begin[t], b.k1);
    b.p1 = sv_min64(p.pair_begin[t + 1], p.n_pairs);
    b.p0 = sv_min64(p.pair_begin[t], b.p1);
    b.ppair_sig = p.ppair_sig;
    b.ppair_key = p.ppair_key;
    b.ppair_verdict = p.ppair_verdict;
    b.q0 = b.q1 = b.pp0 = b.pp1 = 0;
    if (p.ppair_begin) {
      b.pp1 = sv_min64(p.ppair_begin[t + 1], p.n_ppairs);
      b.pp0 = sv_min64(p.ppair_begin[t], b.pp1);
      if (b.pp1 > b.pp0) {
        b.q1 = sv_min64(p.pkey_begin[t + 1], p.n_pkeys);
        b.q0 = sv_min64(p.pkey_begin[t], b.q1);
      }
    }
    const uint64_t g1 = sv_min64(p.signer_begin[c + 1], p.n_signers);
    const uint64_t g0 = sv_min64(p.signer_begin[c], g1);
    r = sv_txcheck<SLOW>(b, p.signer_type + g0, p.signer_weight + g0, p.signer_key + g0,
                         (uint32_t)sv_min64(g1 - g0, SV_TXCHECK_MAX), p.needed[c], p.clamp != 0);
  }
  p.ok[c] = (uint8_t)r.ok;
  p.weight[c] = r.total;
  p.used[c] = r.used;
}

__global__ __launch_bounds__(SV_CHECKBLOCK, 8) void sv_txcheck_kernel(sv_checkparams p) { sv_txcheck_lane<false>(p); }
__global__ __launch_bounds__(SV_CHECKBLOCK) void sv_txcheck_hashx_kernel(sv_checkparams p) { sv_txcheck_lane<true>(p); }

extern "C" {

int sv_check_block(void) { return SV_CHECKBLOCK; }

hipError_t sv_launch_txcheck_payload(const uint64_t* sig_begin, const void* hint, const void* sig,
                                     const uint8_t* sig_len, uint64_t n_sigs, const uint64_t* key_begin,
                                     const void* key, uint64_t n_keys, uint64_t n_bodies, const uint64_t* pair_begin,
                                     const uint32_t* pair_sig, const uint32_t* pair_key, const void* pair_verdict,
                                     uint64_t n_pairs, const void* digests, const uint64_t* check_begin,
                                     const int32_t* check_needed, uint64_t n_checks, const uint64_t* signer_begin,
                                     const uint8_t* signer_type, const uint32_t* signer_weight,
                                     const uint32_t* signer_key, uint64_t n_signers, int clamp,
                                     const uint64_t* ppair_begin, const uint32_t* ppair_sig,
                                     const uint32_t* ppair_key, const void* ppair_verdict, uint64_t n_ppairs,
                                     const uint64_t* pkey_begin, uint64_t n_pkeys, uint8_t* check_ok,
                                     uint32_t* check_weight, uint64_t* check_used, hipStream_t s) {
  if (n_checks == 0) return hipSuccess;
  sv_checkparams p;
  p.sig_begin = sig_begin;
  p.key_begin = key_begin;
  p.pair_begin = pair_begin;
  p.check_begin = check_begin;
  p.signer_begin = signer_begin;
  p.hint = (const uint8_t*)hint;
  p.sig = (const uint8_t*)sig;
  p.sig_len = sig_len;
  p.key = (const uint8_t*)key;
  p.pair_sig = pair_sig;
  p.pair_key = pair_key;
  p.pair_verdict = (const uint8_t*)pair_verdict;
  p.digests = (const uint8_t*)digests;
  p.needed = check_needed;
  p.signer_type = signer_type;
  p.signer_weight = signer_weight;
  p.signer_key = signer_key;
  p.n_bodies = n_bodies;
  p.n_sigs = n_sigs;
  p.n_keys = n_keys;
  p.n_pairs = n_pairs;
  p.n_checks = n_checks;
  p.n_signers = n_signers;
  p.clamp = clamp ? 1u : 0u;
  p.ppair_begin = n_ppairs ? ppair_begin : nullptr;
  p.pkey_begin = pkey_begin;
  p.ppair_sig = ppair_sig;
  p.ppair_key = ppair_key;
  p.ppair_verdict = (const uint8_t*)ppair_verdict;
  p.n_ppairs = n_ppairs;
  p.n_pkeys = n_pkeys;
  p.ok = check_ok;
  p.weight = check_weight;
  p.used = check_used;
  const unsigned blocks = (unsigned)((n_checks + SV_CHECKBLOCK - 1) / SV_CHECKBLOCK);
  hipLaunchKernelGGL(sv_txcheck_kernel, dim3(blocks), dim3(SV_CHECKBLOCK), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sv_txcheck_hashx_kernel, dim3(blocks), dim3(SV_CHECKBLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t sv_launch_txcheck(const uint64_t* sig_begin, const void* hint, const void* sig, const uint8_t* sig_len,
                             uint64_t n_sigs, const uint64_t* key_begin, const void* key, uint64_t n_keys,
                             uint64_t n_bodies, const uint64_t* pair_begin, const uint32_t* pair_sig,
                             const uint32_t* pair_key, const void* pair_verdict, uint64_t n_pairs,
                             const void* digests, const uint64_t* check_begin, const int32_t* check_needed,
                             uint64_t n_checks, const uint64_t* signer_begin, const uint8_t* signer_type,
                             const uint32_t* signer_weight, const uint32_t* signer_key, uint64_t n_signers,
                             int clamp, uint8_t* check_ok, uint32_t* check_weight, uint64_t* check_used,
                             hipStream_t s) {
  return sv_launch_txcheck_payload(sig_begin, hint, sig, sig_len, n_sigs, key_begin, key, n_keys, n_bodies, pair_begin,
                                   pair_sig, pair_key, pair_verdict, n_pairs, digests, check_begin, check_needed,
                                   n_checks, signer_begin, signer_type, signer_weight, signer_key, n_signers, clamp,
                                   nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, check_ok, check_weight,
                                   check_used, s);
}

}  // extern "C"
