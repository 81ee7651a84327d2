// gfx950 batch signer (sign_core.h): RFC 8032 ed25519 signatures, byte-exact
// with libsodium's crypto_sign_seed_keypair / crypto_sign_detached, for any
// message length and with keys shared between messages.
//
//   sv_sign_keys_kernel   one lane per key: seed -> the 96-byte expanded-key
//                         record (a | prefix | pk) in the slot's workspace,
//                         and pk to the caller when asked
//   sv_sign_msgs_kernel   one lane per signature: its key's record through
//                         key_of, the nonce and hram hashes over the message
//                         (fixed- or variable-length), one fixed-base
//                         multiplication ([r]B) and S = h a + r mod L
//
// Both multiply by B over the comb tables of B (comb.h, 32 x 129 cached
// entries, 774 KiB: L2-resident), 32 additions and no doubling.  The old
// dataset signer (sv_kernels.hip sv_sign_kernel) is left as it is.
//
// Not constant-time: entry addresses follow the secret digits.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "sign_core.h"
#include "sv_kparams.h"

#define SV_SIGN_BLOCK 256

struct sv_signkeys_params {
  const sv_u4* seed;  // k x 32 B
  uint32_t k;
  sv_u4* rec;         // k x 96 B out
  sv_u4* pk;          // k x 32 B out (may be nullptr)
  const uint32_t* ctab;
};

struct sv_signmsgs_params {
  const sv_u4* rec;        // k x 96 B
  uint32_t k;
  const uint32_t* key_of;  // n entries (nullptr: key i signs message i)
  const uint8_t* msg;
  const uint64_t* off;     // variable-length mode
  const uint32_t* len;
  uint32_t fixed_len;      // != 0: message i = msg + i * fixed_len
  uint32_t n;
  sv_u4* sig;              // n x 64 B out
  uint32_t* hint;          // n x 4 B out: bytes 28..31 of the signer's pk (may be nullptr)
  const uint32_t* ctab;
};

__global__ __launch_bounds__(SV_SIGN_BLOCK) void sv_sign_keys_kernel(sv_signkeys_params p) {
  const uint32_t i = blockIdx.x * SV_SIGN_BLOCK + threadIdx.x;
  if (i >= p.k) return;
  uint32_t seed[8], rec[SV_SIGN_REC_DW];
  sv_unpack2(seed, p.seed + 2 * (uint64_t)i);
  sv_sign_expand(rec, seed, p.ctab);
  sv_u4* out = p.rec + 6 * (uint64_t)i;
  SV_UNROLL for (int q = 0; q < 6; ++q) out[q] = sv_u4{rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]};
  if (p.pk) {
    p.pk[2 * (uint64_t)i] = sv_u4{rec[16], rec[17], rec[18], rec[19]};
    p.pk[2 * (uint64_t)i + 1] = sv_u4{rec[20], rec[21], rec[22], rec[23]};
  }
}

__global__ __launch_bounds__(SV_SIGN_BLOCK) void sv_sign_msgs_kernel(sv_signmsgs_params p) {
  const uint32_t i = blockIdx.x * SV_SIGN_BLOCK + threadIdx.x;
  if (i >= p.n) return;
  sv_u4* out = p.sig + 4 * (uint64_t)i;
  const uint32_t key = p.key_of ? p.key_of[i] : i;
  if (key >= p.k) {
    // (a device-resident key_of is not validated by the host)
    SV_UNROLL for (int q = 0; q < 4; ++q) out[q] = sv_u4{0u, 0u, 0u, 0u};
    if (p.hint) p.hint[i] = 0u;
    return;
  }
  uint32_t rec[SV_SIGN_REC_DW];
  const sv_u4* in = p.rec + 6 * (uint64_t)key;
  SV_UNROLL for (int q = 0; q < 6; ++q) {
    const sv_u4 v = in[q];
    rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
  }
  const uint8_t* m = p.fixed_len ? p.msg + (uint64_t)i * p.fixed_len : p.msg + p.off[i];
  const uint32_t mlen = p.fixed_len ? p.fixed_len : p.len[i];
  uint32_t sig[16];
  sv_sign_msg(sig, rec, m, mlen, p.ctab);
  SV_UNROLL for (int q = 0; q < 4; ++q) out[q] = sv_u4{sig[4 * q], sig[4 * q + 1], sig[4 * q + 2], sig[4 * q + 3]};
  if (p.hint) p.hint[i] = rec[23];
}

extern "C" {

size_t sv_sign_rec_bytes(uint64_t k) { return (size_t)k * SV_SIGN_REC_DW * 4; }

hipError_t sv_launch_sign_keys(const void* seed, uint32_t k, void* rec, void* pk, const uint32_t* ctab,
                               hipStream_t s) {
  if (k == 0) return hipSuccess;
  sv_signkeys_params p;
  p.seed = (const sv_u4*)seed;
  p.k = k;
  p.rec = (sv_u4*)rec;
  p.pk = (sv_u4*)pk;
  p.ctab = ctab;
  const unsigned grid = (unsigned)(((uint64_t)k + SV_SIGN_BLOCK - 1) / SV_SIGN_BLOCK);
  hipLaunchKernelGGL(sv_sign_keys_kernel, dim3(grid), dim3(SV_SIGN_BLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t sv_launch_sign_msgs(const void* rec, uint32_t k, const uint32_t* key_of, const void* msg,
                               const uint64_t* off, const uint32_t* len, uint32_t fixed_len, uint32_t n, void* sig,
                               void* hint, const uint32_t* ctab, hipStream_t s) {
  if (n == 0) return hipSuccess;
  sv_signmsgs_params p;
  p.rec = (const sv_u4*)rec;
  p.k = k;
  p.key_of = key_of;
  p.msg = (const uint8_t*)msg;
  p.off = off;
  p.len = len;
  p.fixed_len = fixed_len;
  p.n = n;
  p.sig = (sv_u4*)sig;
  p.hint = (uint32_t*)hint;
  p.ctab = ctab;
  const unsigned grid = (unsigned)(((uint64_t)n + SV_SIGN_BLOCK - 1) / SV_SIGN_BLOCK);
  hipLaunchKernelGGL(sv_sign_msgs_kernel, dim3(grid), dim3(SV_SIGN_BLOCK), 0, s, p);
  return hipGetLastError();
}

}  // extern "C"
