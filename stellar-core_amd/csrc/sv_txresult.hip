// gfx950 kernels of the decide calls (txresult.h): one signature result per
// transaction body from the check kernel's per-check decisions, and on request
// the ascending list of the bodies that are not OK.  The scheme is the
// expansion's (sv_txacct.hip): the output order a function of the input only,
// no atomics, no workgroup waits for another one, ordinary stores, every range
// clamped, nothing written outside the outputs and the workspace.
//
//   result  SV_TXR_GROUP lanes per body, SV_TXR_BODIES bodies per workgroup:
//           the group's lanes stride over the body's checks (check_ok,
//           check_used), min-fail and OR-used meet inside the quad through two
//           __shfl_xor steps, the group's first lane stores body_code[t] (and
//           body_fail[t]).  Bodies carry 1 to 100+ checks, most two or three: a
//           lane per body would walk a 100-check body alone while its wave
//           idles (the argument of sv_acct_rows_kernel).  The
//           workgroup's number of non-OK bodies -- __ballot and popcount per
//           wave, summed through LDS -- goes to psum
//   scan    (only with a bad list or its count) one workgroup: psum ->
//           exclusive block offsets in place (scan.h sv_scan_block_sums); the
//           exact total to *n_bad
//   fill    (only with a bad list) a wave per result workgroup: it re-reads
//           that workgroup's body_code, ranks the non-OK bodies by __ballot and
//           stores bad_body[offset + rank] = t where that index is < bad_cap
#include <hip/hip_runtime.h>

#include "launch.h"
#include "scan.h"
#include "sv_common.h"
#include "txresult.h"

#define SV_TXRBLOCK 256
static_assert(SV_TXRBLOCK == SV_SCAN_BLOCK, "the shared scan (scan.h) is written for this block");
#define SV_TXR_GROUP 4
#define SV_TXR_BODIES (SV_TXRBLOCK / SV_TXR_GROUP)  // 64: one fill wave per result workgroup

static_assert(SV_TXR_BODIES == 64, "the fill ranks one result workgroup per 64-lane wave");

struct sv_txrparams {
  sv_txresult_in I;
  uint8_t* code;     // nb
  uint32_t* fail;    // nb, or null
  uint64_t* psum;    // blocks(nb) | total
  uint32_t* bad;     // cap, or null
  uint64_t cap;
  uint64_t* n_bad;   // or null
};

__host__ __device__ __forceinline__ uint64_t sv_txr_blocks(uint64_t nb) {
  return (nb + SV_TXR_BODIES - 1) / SV_TXR_BODIES;
}

__global__ __launch_bounds__(SV_TXRBLOCK) void sv_txresult_kernel(sv_txrparams p) {
  __shared__ uint32_t wsum[SV_TXRBLOCK / 64];
  const uint64_t t = (uint64_t)blockIdx.x * SV_TXR_BODIES + threadIdx.x / SV_TXR_GROUP;
  const unsigned gl = threadIdx.x % SV_TXR_GROUP;
  const bool live = t < p.I.nb;
  uint64_t c0 = 0, c1 = 0, used = 0;
  uint32_t fail = SV_TXRESULT_NONE;
  if (live) sv_txresult_checks(p.I, t, &c0, &c1);
  SV_NOUNROLL for (uint64_t c = c0 + gl; c < c1; c += SV_TXR_GROUP) sv_txresult_step(p.I, c0, c, &fail, &used);
  // (every lane of the wave takes part: a quad never straddles two waves)
  SV_UNROLL for (int d = 1; d < SV_TXR_GROUP; d <<= 1) {
    const uint32_t of = (uint32_t)__shfl_xor((int)fail, d);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)used, d);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(used >> 32), d);
    fail = of < fail ? of : fail;
    used |= sv_pack64(lo, hi);
  }
  bool bad = false;
  if (live && gl == 0) {
    const uint8_t code = sv_txresult_code(p.I, t, c0, fail, used);
    p.code[t] = code;
    if (p.fail) p.fail[t] = fail;
    bad = code != SV_TXRESULT_OK;
  }
  const uint64_t m = __ballot(bad);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x / 64] = (uint32_t)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t n = 0;
    SV_UNROLL for (int w = 0; w < SV_TXRBLOCK / 64; ++w) n += wsum[w];
    p.psum[blockIdx.x] = n;
  }
}

__global__ __launch_bounds__(SV_TXRBLOCK) void sv_txresult_scan_kernel(sv_txrparams p) {
  const uint64_t blocks = sv_txr_blocks(p.I.nb);
  const uint64_t carry = sv_scan_block_sums(p.psum, blocks);
  if (threadIdx.x == 0) {
    p.psum[blocks] = carry;
    if (p.n_bad) *p.n_bad = carry;
  }
}

__global__ __launch_bounds__(SV_TXRBLOCK) void sv_txresult_fill_kernel(sv_txrparams p) {
  const uint64_t rb = (uint64_t)blockIdx.x * (SV_TXRBLOCK / 64) + threadIdx.x / 64;  // the result workgroup
  const unsigned lane = threadIdx.x & 63;
  if (rb >= sv_txr_blocks(p.I.nb)) return;  // (whole waves leave: the ballot below is per wave)
  const uint64_t t = rb * SV_TXR_BODIES + lane;
  const bool bad = t < p.I.nb && p.code[t] != SV_TXRESULT_OK;
  const uint64_t m = __ballot(bad);
  if (!bad) return;
  const uint64_t at = p.psum[rb] + (uint64_t)__popcll(m & (((uint64_t)1 << lane) - 1));
  if (at < p.cap) p.bad[at] = (uint32_t)t;
}

extern "C" {

int sv_txresult_block(void) { return SV_TXR_BODIES; }

size_t sv_txresult_ws_bytes(uint64_t n_bodies) { return sv_a16(8 * (sv_txr_blocks(n_bodies) + 1)) + 16; }

hipError_t sv_launch_txresult(const sv_txresult_in* I, uint8_t* body_code, uint32_t* body_fail, void* ws,
                              uint32_t* bad_body, uint64_t bad_cap, uint64_t* n_bad, hipStream_t s) {
  sv_txrparams p;
  p.I = *I;
  p.code = body_code;
  p.fail = body_fail;
  p.psum = (uint64_t*)ws;
  p.bad = bad_body;
  p.cap = bad_body ? bad_cap : 0;
  p.n_bad = n_bad;
  const uint64_t blocks = sv_txr_blocks(I->nb);
  if (blocks) {
    hipLaunchKernelGGL(sv_txresult_kernel, dim3((unsigned)blocks), dim3(SV_TXRBLOCK), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (!bad_body && !n_bad) return hipSuccess;
  hipLaunchKernelGGL(sv_txresult_scan_kernel, dim3(1), dim3(SV_TXRBLOCK), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !blocks || !p.cap) return e;
  const uint64_t per = SV_TXRBLOCK / 64;
  hipLaunchKernelGGL(sv_txresult_fill_kernel, dim3((unsigned)((blocks + per - 1) / per)), dim3(SV_TXRBLOCK), 0, s, p);
  return hipGetLastError();
}

}  // extern "C"
