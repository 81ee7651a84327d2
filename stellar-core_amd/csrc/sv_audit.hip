// gfx950 kernels of the verdict audit (audit.h): behind a verify launch, on the
// same stream, the picked rows of its verdict array are verified again by the
// textbook equation and compared.  No host wait anywhere: the number of picks
// stays in device memory, where the later kernels read it.  All ordering
// between workgroups comes from kernel boundaries; no slot is handed out by an
// atomic.  Ordinary vector stores, every index below the size of its array:
// rows < n, list and audit bytes < min(picks, budget) <= min(n, budget), ring
// slots < SV_AUDIT_RING, workspace lanes < grid x block.
//
//   select   one lane per row: the pick (audit.h sv_audit_pick); the block's
//            picks go to psum[block] through sv_block_exscan
//   scan     ONE block: psum -> exclusive block offsets in place (scan.h
//            sv_scan_block_sums); the launch's picks and its audited rows
//            m = min(picks, budget) into the counters' last two words
//   fill     the block picks again and adds its offset: list[at] = row,
//            ascending, for at < budget
//   verify   persistent and grid-stride, one lane per audited row, shaped like
//            sv_sign_kernel: load, hash R || A || M, sv_verify_core with the
//            lane's table of -A in the workspace (qstride 1) and the slot's
//            table of B, one audit byte.  The lanes read m from device memory;
//            an inactive lane clamps to a valid row so the wave stays uniform.
//   report   ONE block over the m audit bytes: compare with the engine's byte,
//            add to the slot's counters (plain adds from one lane), append the
//            mismatch records to the ring in row order
#include <hip/hip_runtime.h>

#include "audit.h"
#include "launch.h"
#include "scan.h"
#include "sv_kparams.h"

#define SV_AUDIT_BLOCK 256
#define SV_AUDIT_WAVES 2  // per SIMD, as sv_sign_kernel
static_assert(SV_AUDIT_BLOCK == SV_SCAN_BLOCK, "the shared scan (scan.h) is written for this block");

__host__ __device__ __forceinline__ uint64_t sv_audit_blocks(uint64_t n) {
  return (n + SV_AUDIT_BLOCK - 1) / SV_AUDIT_BLOCK;
}

__device__ __forceinline__ bool sv_audit_row_pick(const sv_audit_args& a, uint64_t i) {
  return i < a.n && sv_audit_pick(a.what, a.one_in, a.seed, a.seq, i, a.verdict[i]);
}

__global__ __launch_bounds__(SV_AUDIT_BLOCK) void sv_audit_select_kernel(sv_audit_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_AUDIT_BLOCK + threadIdx.x;
  uint64_t sum;
  (void)sv_block_exscan(sv_audit_row_pick(a, i) ? 1 : 0, &sum);
  if (threadIdx.x == 0) a.psum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(SV_AUDIT_BLOCK) void sv_audit_scan_kernel(sv_audit_args a) {
  const uint64_t blocks = sv_audit_blocks(a.n);
  const uint64_t total = sv_scan_block_sums(a.psum, blocks);
  if (threadIdx.x == 0) {
    a.psum[blocks] = total;
    a.counters[SV_AC_PICKS] = total;
    a.counters[SV_AC_M] = sv_audit_clip(total, a.budget);
  }
}

__global__ __launch_bounds__(SV_AUDIT_BLOCK) void sv_audit_fill_kernel(sv_audit_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_AUDIT_BLOCK + threadIdx.x;
  const bool pick = sv_audit_row_pick(a, i);
  uint64_t sum;
  const uint64_t at = a.psum[blockIdx.x] + sv_block_exscan(pick ? 1 : 0, &sum);
  if (pick && at < a.budget) a.list[at] = (uint32_t)i;
}

// F32: fixed 32-byte messages in a 16-byte aligned array (read as two quads, sha512_ram32); else any fixed length
// and offset/length mode at any alignment (sha512_ram_var)
template <bool F32>
__global__ __launch_bounds__(SV_AUDIT_BLOCK, SV_AUDIT_WAVES) void sv_audit_verify_kernel(sv_audit_args a) {
  const uint64_t m = a.counters[SV_AC_M];
  const sv_u4* pk = (const sv_u4*)a.pk;
  const sv_u4* sg = (const sv_u4*)a.sig;
  const uint8_t* msg = (const uint8_t*)a.msg;
  const sv_u4* btab = (const sv_u4*)a.btab;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  sv_u4* slot = (sv_u4*)a.ws + gtid * SV_SLOT_QUADS_W;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = gtid - lane; base < m; base += stride) {
    const uint64_t j = base + lane;
    const bool active = j < m;
    const uint64_t jj = active ? j : m - 1;
    const uint64_t ii = a.list[jj];
    uint32_t A[8], R[8], S[8], hram[16];
    sv_unpack2(A, pk + 2 * ii);
    sv_unpack2(R, sg + 4 * ii);
    sv_unpack2(S, sg + 4 * ii + 2);
    if (F32) {
      uint32_t M[8];
      sv_unpack2(M, (const sv_u4*)msg + 2 * ii);
      sha512_ram32(hram, R, A, M);
    } else if (a.fixed_len) {
      sha512_ram_var(hram, R, A, msg + ii * (uint64_t)a.fixed_len, a.fixed_len);
    } else {
      sha512_ram_var(hram, R, A, msg + a.off[ii], a.len[ii]);
    }
    const bool ok = sv_verify_core(A, sg + 4 * ii, S, hram, slot, 1, btab);
    uint8_t v = ok ? 1 : 0;
    if (a.dissent && jj == 0) v ^= 1;
    if (active) a.av[j] = v;
  }
}

__global__ __launch_bounds__(SV_AUDIT_BLOCK) void sv_audit_report_kernel(sv_audit_args a) {
  const uint64_t m = a.counters[SV_AC_M];
  const uint64_t picks = a.counters[SV_AC_PICKS];
  const uint64_t held = a.counters[SV_AC_HELD];
  uint64_t rejects = 0, mismatches = 0;
  SV_NOUNROLL for (uint64_t base = 0; base < m; base += SV_AUDIT_BLOCK) {
    const uint64_t j = base + threadIdx.x;
    uint32_t row = 0;
    uint8_t e = 0, v = 0;
    bool differ = false;
    if (j < m) {
      row = a.list[j];
      e = a.verdict[row];
      v = a.av[j];
      differ = e != v;
      rejects += e == 0 ? 1 : 0;
    }
    uint64_t sum;
    const uint64_t rank = mismatches + sv_block_exscan(differ ? 1 : 0, &sum);
    mismatches += sum;
    if (differ) {
      const uint32_t at = sv_audit_ring_slot(held, rank);
      if (at < SV_AUDIT_RING) {
        const uint8_t* mp = (const uint8_t*)a.msg + (a.fixed_len ? (uint64_t)row * a.fixed_len : a.off[row]);
        const uint32_t len = a.fixed_len ? a.fixed_len : a.len[row];
        sv_audit_record_fill(&a.ring[at], a.seq, row, e, v, 0xFF, (const uint8_t*)a.pk + 32 * (uint64_t)row,
                             (const uint8_t*)a.sig + 64 * (uint64_t)row, mp, len);
      }
    }
  }
  uint64_t all_rejects;
  (void)sv_block_exscan(rejects, &all_rejects);
  if (threadIdx.x == 0) {
    const uint64_t room = held < SV_AUDIT_RING ? SV_AUDIT_RING - held : 0;
    const uint64_t kept = mismatches < room ? mismatches : room;
    a.counters[SV_AC_AUDITED] += m;
    a.counters[SV_AC_REJECTS] += all_rejects;
    a.counters[SV_AC_OVER] += picks - m;
    a.counters[SV_AC_MISMATCH] += mismatches;
    a.counters[SV_AC_HELD] = held + kept;
    a.counters[SV_AC_LOST] += mismatches - kept;
  }
}

extern "C" {

size_t sv_audit_psum_bytes(uint64_t n) { return sv_a16(8 * (sv_audit_blocks(n) + 1)); }

int sv_audit_blocks_per_cu(void) {
  int b0 = 0, b1 = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b0, sv_audit_verify_kernel<true>, SV_AUDIT_BLOCK, 0) != hipSuccess)
    b0 = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b1, sv_audit_verify_kernel<false>, SV_AUDIT_BLOCK, 0) != hipSuccess)
    b1 = 1;
  const int b = b0 > b1 ? b0 : b1;
  return b < 1 ? 1 : b;
}

unsigned sv_audit_grid(uint64_t n, uint64_t budget, unsigned max_blocks) {
  const uint64_t need = sv_audit_blocks(sv_audit_clip(n, budget));
  const uint64_t g = need < max_blocks ? need : max_blocks;
  return (unsigned)(g < 1 ? 1 : g);
}

size_t sv_audit_ws_bytes(unsigned grid) {
  return (size_t)grid * SV_AUDIT_BLOCK * SV_SLOT_QUADS_W * sizeof(sv_u4);
}

hipError_t sv_launch_audit(const sv_audit_args* A, hipStream_t s) {
  const uint64_t blocks = sv_audit_blocks(A->n);
  if (!blocks || A->n > SV_AUDIT_MAX_ROWS || !A->budget || !A->grid) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sv_audit_select_kernel, dim3((unsigned)blocks), dim3(SV_AUDIT_BLOCK), 0, s, *A);
  hipLaunchKernelGGL(sv_audit_scan_kernel, dim3(1), dim3(SV_AUDIT_BLOCK), 0, s, *A);
  hipLaunchKernelGGL(sv_audit_fill_kernel, dim3((unsigned)blocks), dim3(SV_AUDIT_BLOCK), 0, s, *A);
  if (A->fixed_len == 32 && ((uintptr_t)A->msg & 15u) == 0)
    hipLaunchKernelGGL(sv_audit_verify_kernel<true>, dim3(A->grid), dim3(SV_AUDIT_BLOCK), 0, s, *A);
  else
    hipLaunchKernelGGL(sv_audit_verify_kernel<false>, dim3(A->grid), dim3(SV_AUDIT_BLOCK), 0, s, *A);
  hipLaunchKernelGGL(sv_audit_report_kernel, dim3(1), dim3(SV_AUDIT_BLOCK), 0, s, *A);
  return hipGetLastError();
}

}  // extern "C"
