// TEST INFRASTRUCTURE: gfx950 probe over csrc/sign_core.h, built with the product's kernel flags, for
// tests/test_gpu_sign.py: the fixed-base multiplication on chosen scalars, one lane per scalar.
#include <hip/hip_runtime.h>

#include "sign_core.h"

__global__ __launch_bounds__(128) void sgp_ctab_kernel(uint32_t* ctab) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= SV_CB_POS * SV_CB_ENT) return;
  sv_comb_bentry(ctab + (size_t)id * SV_CE_DW, id / SV_CB_ENT, id % SV_CB_ENT);
}

__global__ __launch_bounds__(64) void sgp_fixed_base_kernel(const uint32_t* s, uint32_t n, uint32_t* out,
                                                            const uint32_t* ctab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t w[8], enc[8];
  SV_UNROLL for (int k = 0; k < 8; ++k) w[k] = s[8 * i + k];
  sv_fixed_base_encode(enc, w, ctab);
  SV_UNROLL for (int k = 0; k < 8; ++k) out[8 * i + k] = enc[k];
}

// out[i] = encode([s_i]B) for n host scalars < 2^253; returns 0 or the HIP error code
extern "C" int sgp_fixed_base(const uint8_t* s, size_t n, uint8_t* out) {
  if (n == 0) return 0;
  uint32_t *d_ctab = nullptr, *d_s = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_ctab, (size_t)SV_CB_DW * 4);
  if (e == hipSuccess) e = hipMalloc(&d_s, 32 * n);
  if (e == hipSuccess) e = hipMalloc(&d_out, 32 * n);
  if (e == hipSuccess) e = hipMemcpy(d_s, s, 32 * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(sgp_ctab_kernel, dim3((SV_CB_POS * SV_CB_ENT + 127) / 128), dim3(128), 0, 0, d_ctab);
    hipLaunchKernelGGL(sgp_fixed_base_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, d_s, (uint32_t)n,
                       d_out, d_ctab);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, 32 * n, hipMemcpyDeviceToHost);
  (void)hipFree(d_ctab);
  (void)hipFree(d_s);
  (void)hipFree(d_out);
  return (int)e;
}
