// Measurement tool: the result kernel's fold (csrc/txresult.h) with one lane per body against four (the product's
// geometry, csrc/sv_txresult.hip), on synthetic check arrays of the two shapes that matter -- two checks per body
// (the single-signature sets) and 1..6 checks with one body in 64 carrying 130 (the imbalance case).  Both forms
// are checked against the host's fold first; then medians of 21 launches between two events.  DESIGN.md 3.15.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -Istellar-core_amd/csrc -o tools/txresult_lanes tools/txresult_lanes.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "txresult.h"

#define HIPCHECK(x)                                                                  \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));         \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

template <int G>
__global__ __launch_bounds__(256) void fold_kernel(sv_txresult_in I, uint8_t* code, uint32_t* fail) {
  const uint64_t t = (uint64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  const unsigned gl = threadIdx.x % G;
  uint64_t c0 = 0, c1 = 0, used = 0;
  uint32_t f = SV_TXRESULT_NONE;
  if (t < I.nb) sv_txresult_checks(I, t, &c0, &c1);
  SV_NOUNROLL for (uint64_t c = c0 + gl; c < c1; c += G) sv_txresult_step(I, c0, c, &f, &used);
  SV_UNROLL for (int d = 1; d < G; d <<= 1) {
    const uint32_t of = (uint32_t)__shfl_xor((int)f, d);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)used, d);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(used >> 32), d);
    f = of < f ? of : f;
    used |= sv_pack64(lo, hi);
  }
  if (t < I.nb && gl == 0) {
    code[t] = sv_txresult_code(I, t, c0, f, used);
    fail[t] = f;
  }
}

template <class T>
static T* upload(const std::vector<T>& v) {
  T* d = nullptr;
  if (hipMalloc(&d, v.size() * sizeof(T) + 16) != hipSuccess) return nullptr;
  if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return d;
}

static int run(const char* name, uint64_t nb, bool skewed) {
  std::mt19937_64 rng(nb + skewed);
  std::vector<uint64_t> cb{0}, sb{0}, used;
  std::vector<uint8_t> ok, role, flags(nb, 0);
  for (uint64_t t = 0; t < nb; ++t) {
    const int k = !skewed ? 2 : (t % 64 == 7 ? 130 : 1 + (int)(rng() % 6));
    for (int i = 0; i < k; ++i) {
      ok.push_back(rng() % 16 ? 1 : 0);
      used.push_back(rng() % 4 ? ~(uint64_t)0 : rng());
      role.push_back(i ? 1 : 0);
    }
    cb.push_back(ok.size());
    sb.push_back(sb.back() + 1 + rng() % 3);
  }
  const uint64_t nc = ok.size();
  uint64_t *d_cb = upload(cb), *d_sb = upload(sb), *d_used = upload(used);
  uint8_t *d_ok = upload(ok), *d_role = upload(role), *d_flags = upload(flags), *d_code = nullptr;
  uint32_t* d_fail = nullptr;
  if (!d_cb || !d_sb || !d_used || !d_ok || !d_role || !d_flags) return 1;
  HIPCHECK(hipMalloc(&d_code, nb + 16));
  HIPCHECK(hipMalloc(&d_fail, 4 * nb + 16));
  const sv_txresult_in I{d_cb, d_sb, d_ok, d_used, d_role, d_flags, nb, nc, sb.back()};
  const sv_txresult_in H{cb.data(), sb.data(), ok.data(), used.data(), role.data(), flags.data(), nb, nc, sb.back()};
  std::vector<uint8_t> want(nb), got(nb);
  std::vector<uint32_t> wfail(nb), gfail(nb);
  for (uint64_t t = 0; t < nb; ++t) want[t] = sv_txresult_body(H, t, &wfail[t]);
  hipEvent_t e0, e1;
  HIPCHECK(hipEventCreate(&e0));
  HIPCHECK(hipEventCreate(&e1));
  double med[2];
  for (int form = 0; form < 2; ++form) {
    const unsigned per = form ? 64 : 256, blocks = (unsigned)((nb + per - 1) / per);
    auto launch = [&] {
      if (form) hipLaunchKernelGGL(fold_kernel<4>, dim3(blocks), dim3(256), 0, 0, I, d_code, d_fail);
      else hipLaunchKernelGGL(fold_kernel<1>, dim3(blocks), dim3(256), 0, 0, I, d_code, d_fail);
    };
    HIPCHECK(hipMemset(d_code, 0xA5, nb));
    launch();
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpy(got.data(), d_code, nb, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(gfail.data(), d_fail, 4 * nb, hipMemcpyDeviceToHost));
    if (got != want || gfail != wfail) {
      std::printf("%s: form %d differs from the host fold\n", name, form);
      return 1;
    }
    std::vector<float> ms(21);
    for (float& m : ms) {
      HIPCHECK(hipEventRecord(e0, 0));
      launch();
      HIPCHECK(hipEventRecord(e1, 0));
      HIPCHECK(hipEventSynchronize(e1));
      HIPCHECK(hipEventElapsedTime(&m, e0, e1));
    }
    std::sort(ms.begin(), ms.end());
    med[form] = ms[10];
    std::printf("{\"set\": \"%s\", \"bodies\": %llu, \"checks\": %llu, \"lanes_per_body\": %d, \"median_ms\": %.4f, "
                "\"min_ms\": %.4f, \"max_ms\": %.4f}\n",
                name, (unsigned long long)nb, (unsigned long long)nc, form ? 4 : 1, ms[10], ms[0], ms[20]);
  }
  (void)med;
  for (void* p : {(void*)d_cb, (void*)d_sb, (void*)d_used, (void*)d_ok, (void*)d_role, (void*)d_flags, (void*)d_code,
                  (void*)d_fail})
    HIPCHECK(hipFree(p));
  return 0;
}

int main() {
  if (run("two_checks", 1u << 20, false)) return 1;
  if (run("skewed", 1u << 18, true)) return 1;
  return 0;
}
