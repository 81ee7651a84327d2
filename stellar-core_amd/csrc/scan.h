// The two-level exclusive scan and the CSR owner search that the pairing
// (sv_txpair.hip), the expansion (sv_txacct.hip), the results (sv_txresult.hip)
// and the check kernel (sv_txcheck.hip) share.  "Count, scan, fill" on one
// stream: a count kernel stores each item's count and, through
// sv_block_exscan, its block's sum; ONE block runs sv_scan_block_sums over the
// block sums; the fill scans its block's counts again and adds the block's
// offset.  The output order is a function of the input only: no slot is handed
// out by an atomic and no workgroup waits for another one.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "sv_common.h"

#define SV_SCAN_BLOCK 256

// x rounded up to a multiple of 16: the alignment of every workspace section
SV_HD uint64_t sv_a16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

#if defined(__HIPCC__)

// Exclusive scan of one value per lane over the block (blockDim.x ==
// SV_SCAN_BLOCK, every lane calls); *sum: the block's total.
__device__ __forceinline__ uint64_t sv_block_exscan(uint64_t v, uint64_t* sum) {
  __shared__ uint64_t buf[2][SV_SCAN_BLOCK];
  const unsigned i = threadIdx.x;
  int cur = 0;
  buf[0][i] = v;
  __syncthreads();
  SV_UNROLL for (unsigned d = 1; d < SV_SCAN_BLOCK; d <<= 1) {
    const uint64_t x = buf[cur][i] + (i >= d ? buf[cur][i - d] : 0);
    buf[cur ^ 1][i] = x;
    cur ^= 1;
    __syncthreads();
  }
  const uint64_t incl = buf[cur][i];
  *sum = buf[cur][SV_SCAN_BLOCK - 1];
  __syncthreads();  // (the buffers are reused by the caller's next scan)
  return incl - v;
}

// The second level, called by every lane of ONE block: ps[0 .. blocks) ->
// exclusive offsets in place; returns the total.  Each lane sums a contiguous
// run of blocks (one block up to SV_SCAN_BLOCK^2 first-level items, more above
// it) and the lane totals are scanned in LDS once.  Rounds of SV_SCAN_BLOCK
// with a carried total read coalesced but scan in LDS once per round: over
// 2^20 bodies (16 rounds) count and scan took 47-53 us against this form's
// 37-42 us (profiles/r13/refactor/ab_rounds_form.json).
__device__ __forceinline__ uint64_t sv_scan_block_sums(uint64_t* ps, uint64_t blocks) {
  const uint64_t per = (blocks + SV_SCAN_BLOCK - 1) / SV_SCAN_BLOCK;
  const uint64_t a = per * threadIdx.x < blocks ? per * threadIdx.x : blocks;
  const uint64_t b = a + per < blocks ? a + per : blocks;
  uint64_t mine = 0;
  SV_NOUNROLL for (uint64_t i = a; i < b; ++i) mine += ps[i];
  uint64_t sum;
  uint64_t run = sv_block_exscan(mine, &sum);
  SV_NOUNROLL for (uint64_t i = a; i < b; ++i) {
    const uint64_t v = ps[i];
    ps[i] = run;
    run += v;
  }
  return sum;
}

// The row of a CSR array that owns item c: the first t with begin[t + 1] > c
// (rows without items are repeated entries and are skipped); n: no row owns it.
__device__ __forceinline__ uint64_t sv_csr_owner(const uint64_t* begin, uint64_t n, uint64_t c) {
  uint64_t lo = 0, hi = n;
  SV_NOUNROLL while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (begin[mid + 1] <= c) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

#endif  // __HIPCC__
