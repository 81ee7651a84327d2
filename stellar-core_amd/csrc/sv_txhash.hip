// gfx950 transaction-contents-hash kernel: digest t = SHA-256(prefix(kind t) ||
// body t) (txhash.h), written to digests[t] and, in the same pass, into the
// 32-byte message slot of every signature of body t, so the verify kernels run
// in mode 0 (32-byte messages) over that array on the same stream with no copy
// or sync in between.
//
// One lane per body, grid-stride.  A body whose start is 16-byte aligned (the
// engine's staging always places it so) is read with 16-byte loads, four per
// block; any other start takes the byte-safe dword path.  Loads are register
// loads, not LDS staging: at one body per lane a quad load touches one line
// per lane either way, the second block of a 128-byte line is served by the
// cache, and the kernel is bound by the 64 rounds per block, not by the loads
// ("Transaction bodies").
#include <hip/hip_runtime.h>

#include "launch.h"
#include "txhash.h"

#define SV_TXBLOCK 256

struct sv_txparams {
  const uint8_t* bodies;
  const uint64_t* off;        // body t = bodies + off[t]
  const uint32_t* len;
  const uint8_t* kind;
  const uint64_t* sig_begin;  // n_bodies + 1 entries (read only when msg != nullptr)
  uint64_t n_bodies;
  uint64_t n;                 // signatures: slots of msg
  uint32_t nid[8];            // network id, little-endian words
  uint4* msg;                 // n x 32 B, 16-byte aligned (may be nullptr)
  uint4* digests;             // n_bodies x 32 B, 16-byte aligned (may be nullptr)
};

__global__ __launch_bounds__(SV_TXBLOCK) void sv_txhash_kernel(sv_txparams p) {
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < p.n_bodies;
       t += (uint64_t)gridDim.x * blockDim.x) {
    const uint8_t* body = p.bodies + p.off[t];
    const uint32_t L = p.len[t];
    const uint32_t kind = p.kind[t];
    uint32_t d[8];
    if (((uintptr_t)body & 15u) == 0) sv_txhash<SV_TX_QUADS>(d, p.nid, body, L, kind);
    else sv_txhash<SV_TX_DWORDS>(d, p.nid, body, L, kind);
    const uint4 lo = uint4{d[0], d[1], d[2], d[3]}, hi = uint4{d[4], d[5], d[6], d[7]};
    if (p.digests) {
      p.digests[2 * t] = lo;
      p.digests[2 * t + 1] = hi;
    }
    if (p.msg) {
      // (clamped to the array: a device-resident CSR array is not validated by the host)
      uint64_t s = p.sig_begin[t], e = p.sig_begin[t + 1];
      if (e > p.n) e = p.n;
      SV_NOUNROLL for (; s < e; ++s) {
        p.msg[2 * s] = lo;
        p.msg[2 * s + 1] = hi;
      }
    }
  }
}

extern "C" {

hipError_t sv_launch_txhash(unsigned max_blocks, const uint8_t* nid, const void* bodies, const uint64_t* off,
                            const uint32_t* len, const uint8_t* kind, uint64_t n_bodies, const uint64_t* sig_begin,
                            uint64_t n, void* msg, void* digests, hipStream_t s) {
  if (n_bodies == 0) return hipSuccess;
  sv_txparams p;
  p.bodies = (const uint8_t*)bodies;
  p.off = off;
  p.len = len;
  p.kind = kind;
  p.sig_begin = sig_begin;
  p.n_bodies = n_bodies;
  p.n = n;
  for (int i = 0; i < 8; ++i)
    p.nid[i] = (uint32_t)nid[4 * i] | ((uint32_t)nid[4 * i + 1] << 8) | ((uint32_t)nid[4 * i + 2] << 16) |
               ((uint32_t)nid[4 * i + 3] << 24);
  p.msg = n ? (uint4*)msg : nullptr;
  p.digests = (uint4*)digests;
  const uint64_t need = (n_bodies + SV_TXBLOCK - 1) / SV_TXBLOCK;
  const unsigned grid = (unsigned)(need < max_blocks ? need : (max_blocks ? max_blocks : 1));
  hipLaunchKernelGGL(sv_txhash_kernel, dim3(grid), dim3(SV_TXBLOCK), 0, s, p);
  return hipGetLastError();
}

}  // extern "C"
