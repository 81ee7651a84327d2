// gfx950 kernels of the verdict cache (vcache.h): which items of a verify
// launch the slot's table already holds a verdict for, the compaction of the
// rest into the arrays of a smaller verify launch, and the insert of that
// launch's verdicts.  Everything on the slot's one stream; all ordering between
// workgroups comes from kernel boundaries -- no flag is polled, no workgroup
// waits for another one -- and the only atomics are the claims (atomicMin of an
// item index, whose result does not depend on the order they arrive in) and one
// counter update per workgroup.  Ordinary vector stores, every index below the
// size of its array: items < n, miss rows < the scan's total <= n, slots < 4 sets.
//
//   probe    one lane per item: its key (sv_launch_hash kind 0 wrote it), the
//            four ways of its set; a hit stores the verdict byte (and hit[i]),
//            every lane stores missed[i]; the block's misses go to psum[block]
//            through sv_block_exscan, its hits to the counter
//   scan     ONE block: psum -> exclusive block offsets in place
//            (scan.h sv_scan_block_sums), the total to psum[blocks] and to the
//            word the host reads the miss count from
//   fill     the block scans its missed bytes again and adds its offset:
//            miss[at] = i, ascending
//   gather   one lane per 16-byte quad of a compacted row: two of the key, four
//            of the signature and two of a fixed 32-byte message (read by bytes
//            where the caller's messages are not 16-byte aligned); every other
//            form is not copied: the row's lane 6 stores the message's offset
//            and length in the caller's buffer
//   claim    behind the verify launch, one lane per compacted row j: the
//            verdict to verdict[miss[j]] (the scatter), the key's candidate slot
//            to slot[j] and atomicMin(claim[slot], miss[j])
//   store    the row whose item stands in its claim word writes the whole entry
//            and resets the claim word; every other row is dropped this pass
//   export   behind the store, only while the slots share what they verified
//            (vshare.h): one lane per 16-byte quad of the leading miss rows'
//            keys, gathered with their verdict bytes into the image a journal
//            drain uploads; loads and stores only
//   bitmap   a ballot per wave over the final verdict bytes
//   feed     the drain of the slot's journal (vjournal.h), one lane per row that
//            arrives with its verdict: feed claim (present rows name no slot,
//            the others atomicMin their row index) and feed store (the winner
//            writes the entry); their counters are one atomic add per wave
//   lookup   one lane per key: the held verdict or SV_VC_MISS; reads only
#include <hip/hip_runtime.h>

#include "launch.h"
#include "scan.h"
#include "sv_common.h"
#include "vcache.h"

#define SV_VCBLOCK 256
static_assert(SV_VCBLOCK == SV_SCAN_BLOCK, "the shared scan (scan.h) is written for this block");
static_assert(sizeof(sv_vc_entry) == 4 * SV_VC_ENTRY_WORDS, "an entry is three quads");

__host__ __device__ __forceinline__ uint64_t sv_vc_blocks(uint64_t n) { return (n + SV_VCBLOCK - 1) / SV_VCBLOCK; }

__device__ __forceinline__ void sv_vc_load_key(const uint32_t* keys, uint64_t i, uint32_t* k) {
  const uint4* p = (const uint4*)(keys + 8 * i);
  const uint4 a = p[0], b = p[1];
  k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w;
  k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
}

// the block's sum of one flag per lane, in lane 0 (every lane calls)
__device__ __forceinline__ uint32_t sv_vc_block_count(bool flag) {
  __shared__ uint32_t wsum[SV_VCBLOCK / 64];
  const uint64_t m = __ballot(flag);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x / 64] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t n = 0;
  SV_UNROLL for (int w = 0; w < SV_VCBLOCK / 64; ++w) n += wsum[w];
  __syncthreads();  // (the caller's next count reuses the buffer)
  return n;
}

__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_probe_kernel(sv_vc_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  const bool live = i < a.n;
  uint64_t missed = 0;
  if (live) {
    uint32_t k[8];
    sv_vc_load_key(a.keys, i, k);
    const int v = sv_vc_lookup(a.tab, a.sets, k);
    missed = v < 0 ? 1 : 0;
    if (v >= 0) a.verdict[i] = (uint8_t)v;
    if (a.hit) a.hit[i] = v >= 0 ? 1 : 0;
    a.missed[i] = (uint8_t)missed;
  }
  uint64_t sum;
  (void)sv_block_exscan(missed, &sum);
  if (threadIdx.x == 0) {
    a.psum[blockIdx.x] = sum;
    const uint64_t left = a.n - (uint64_t)blockIdx.x * SV_VCBLOCK;
    const uint64_t hits = (left < SV_VCBLOCK ? left : SV_VCBLOCK) - sum;
    if (hits) atomicAdd((unsigned long long*)&a.counters[0], (unsigned long long)hits);
  }
}

__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_scan_kernel(sv_vc_args a) {
  const uint64_t blocks = sv_vc_blocks(a.n);
  const uint64_t total = sv_scan_block_sums(a.psum, blocks);
  if (threadIdx.x == 0) {
    a.psum[blocks] = total;
    a.counters[3] = total;
  }
}

__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_fill_kernel(sv_vc_args a) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  const uint64_t missed = i < a.n ? a.missed[i] : 0;
  uint64_t sum;
  const uint64_t at = a.psum[blockIdx.x] + sv_block_exscan(missed, &sum);
  if (missed) a.miss[at] = (uint32_t)i;
}

__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_gather_kernel(sv_vc_args a) {
  const uint64_t t = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  const uint64_t j = t >> 3;
  const unsigned q = (unsigned)(t & 7);
  if (j >= a.psum[sv_vc_blocks(a.n)]) return;
  const uint64_t i = a.miss[j];
  if (q < 2) {
    ((uint4*)a.cpk)[2 * j + q] = ((const uint4*)a.pk)[2 * i + q];
  } else if (q < 6) {
    ((uint4*)a.csig)[4 * j + (q - 2)] = ((const uint4*)a.sig)[4 * i + (q - 2)];
  } else if (a.fixed_len == 32) {
    const uint8_t* m = (const uint8_t*)a.msg + 32 * i + 16 * (q - 6);
    uint4 v;
    if (((uintptr_t)a.msg & 15u) == 0) {
      v = *(const uint4*)m;
    } else {
      uint32_t w[4];
      SV_UNROLL for (int x = 0; x < 4; ++x)
        w[x] = (uint32_t)m[4 * x] | ((uint32_t)m[4 * x + 1] << 8) | ((uint32_t)m[4 * x + 2] << 16) |
               ((uint32_t)m[4 * x + 3] << 24);
      v = uint4{w[0], w[1], w[2], w[3]};
    }
    ((uint4*)a.cmsg)[2 * j + (q - 6)] = v;
  } else if (q == 6) {
    a.coff[j] = a.fixed_len ? i * (uint64_t)a.fixed_len : a.off[i];
    a.clen[j] = a.fixed_len ? a.fixed_len : a.len[i];
  }
}

__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_claim_kernel(sv_vc_args a, uint64_t n_miss) {
  const uint64_t j = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  if (j >= n_miss) return;
  const uint32_t i = a.miss[j];
  const uint8_t v = a.cverdict[j];
  a.verdict[i] = v;
  uint32_t s = SV_VC_NO_SLOT;
  if (v <= 1) {  // (anything else is no verdict of the verify kernels: never cached)
    uint32_t k[8];
    sv_vc_load_key(a.keys, i, k);
    s = (uint32_t)sv_vc_candidate(a.tab, a.sets, k);
    atomicMin(&a.claim[s], i);
  }
  a.slot[j] = s;
}

__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_store_kernel(sv_vc_args a, uint64_t n_miss) {
  const uint64_t j = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  const bool live = j < n_miss;
  bool won = false;
  if (live) {
    const uint32_t i = a.miss[j];
    const uint32_t s = a.slot[j];
    // (the winner alone resets the word: a loser reads the winner's index or SV_VC_UNCLAIMED, never its own)
    won = s != SV_VC_NO_SLOT && a.claim[s] == i;
    if (won) {
      uint32_t k[8];
      sv_vc_load_key(a.keys, i, k);
      sv_vc_store(a.tab, s, k, a.cverdict[j]);
      a.claim[s] = SV_VC_UNCLAIMED;
    }
  }
  const uint32_t ins = sv_vc_block_count(won);
  const uint32_t drop = sv_vc_block_count(live && !won);
  if (threadIdx.x == 0) {
    if (ins) atomicAdd((unsigned long long*)&a.counters[1], (unsigned long long)ins);
    if (drop) atomicAdd((unsigned long long*)&a.counters[2], (unsigned long long)drop);
  }
}

// The export of a pass (vshare.h): the leading r rows of the miss list as the image a journal drain uploads -- keys
// (32 r bytes), then verdict bytes (r).  One lane per 16-byte quad of a key, two to a row; the row's lane 0 also
// stores its verdict byte.  r <= the pass's miss count, so j < r names a filled miss row; the image holds 33 r bytes.
__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_export_kernel(sv_vc_args a, uint64_t r, uint8_t* image) {
  const uint64_t t = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  const uint64_t j = t >> 1;
  const unsigned q = (unsigned)(t & 1);
  if (j >= r) return;
  const uint64_t i = a.miss[j];
  ((uint4*)image)[2 * j + q] = ((const uint4*)a.keys)[2 * i + q];
  if (q == 0) image[32 * r + j] = a.cverdict[j];
}

__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_bitmap_kernel(const uint8_t* verdict, uint64_t n, uint64_t* bitmap) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  const bool ok = i < n && verdict[i] == 1;
  const uint64_t m = __ballot(ok);
  const uint64_t base = i & ~(uint64_t)63;
  if ((threadIdx.x & 63) == 0 && base < n) bitmap[base >> 6] = m;
}

// one atomic add per wave of the wave's count of `flag` (every lane of the block calls)
__device__ __forceinline__ void sv_vc_wave_add(uint64_t* counter, bool flag) {
  const uint64_t m = __ballot(flag);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(m));
}

// The drain of the slot's journal (vcache.h Feed), one lane per row.  claim: a row the table holds is present; any
// other names its candidate slot and claims it with its row index.
__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_feed_claim_kernel(sv_vc_feed_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  bool present = false;
  if (j < a.n) {
    uint32_t k[8];
    sv_vc_load_key(a.keys, j, k);
    const uint32_t s = sv_vc_feed_slot(a.tab, a.sets, k, a.verdict[j], &present);
    if (s != SV_VC_NO_SLOT) atomicMin(&a.claim[s], (uint32_t)j);
    a.slot[j] = s;
  }
  sv_vc_wave_add(&a.counters[0], present);
}

// store: the row whose index stands in its claim word writes the entry and resets the word; a row that named a
// slot and lost it is dropped
__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_feed_store_kernel(sv_vc_feed_args a) {
  const uint64_t j = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  bool won = false, lost = false;
  if (j < a.n) {
    const uint32_t s = a.slot[j];
    if (s != SV_VC_NO_SLOT) {
      won = a.claim[s] == (uint32_t)j;
      lost = !won;
      if (won) {
        uint32_t k[8];
        sv_vc_load_key(a.keys, j, k);
        sv_vc_store(a.tab, s, k, a.verdict[j]);
        a.claim[s] = SV_VC_UNCLAIMED;
      }
    }
  }
  sv_vc_wave_add(&a.counters[1], won);
  sv_vc_wave_add(&a.counters[2], lost);
}

// out[i]: the verdict the table holds for key i (0 or 1), or SV_VC_MISS_BYTE; the table is only read
#define SV_VC_MISS_BYTE 0xFFu
__global__ __launch_bounds__(SV_VCBLOCK) void sv_vc_lookup_kernel(const sv_vc_entry* tab, uint64_t sets,
                                                                  const uint32_t* keys, uint64_t n, uint8_t* out) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_VCBLOCK + threadIdx.x;
  if (i >= n) return;
  uint32_t k[8];
  sv_vc_load_key(keys, i, k);
  const int v = sv_vc_lookup(tab, sets, k);
  out[i] = v < 0 ? (uint8_t)SV_VC_MISS_BYTE : (uint8_t)v;
}

extern "C" {

int sv_vc_block(void) { return SV_VCBLOCK; }

size_t sv_vc_psum_bytes(uint64_t n) { return sv_a16(8 * (sv_vc_blocks(n) + 1)); }

hipError_t sv_launch_vc_probe(const sv_vc_args* A, hipStream_t s) {
  const uint64_t blocks = sv_vc_blocks(A->n);
  if (!blocks || A->n > SV_VC_MAX_ITEMS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sv_vc_probe_kernel, dim3((unsigned)blocks), dim3(SV_VCBLOCK), 0, s, *A);
  hipLaunchKernelGGL(sv_vc_scan_kernel, dim3(1), dim3(SV_VCBLOCK), 0, s, *A);
  hipLaunchKernelGGL(sv_vc_fill_kernel, dim3((unsigned)blocks), dim3(SV_VCBLOCK), 0, s, *A);
  hipLaunchKernelGGL(sv_vc_gather_kernel, dim3((unsigned)sv_vc_blocks(8 * A->n)), dim3(SV_VCBLOCK), 0, s, *A);
  return hipGetLastError();
}

hipError_t sv_launch_vc_insert(const sv_vc_args* A, uint64_t n_miss, hipStream_t s) {
  if (!n_miss) return hipSuccess;
  if (n_miss > A->n) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)sv_vc_blocks(n_miss);
  hipLaunchKernelGGL(sv_vc_claim_kernel, dim3(blocks), dim3(SV_VCBLOCK), 0, s, *A, n_miss);
  hipLaunchKernelGGL(sv_vc_store_kernel, dim3(blocks), dim3(SV_VCBLOCK), 0, s, *A, n_miss);
  return hipGetLastError();
}

// behind sv_launch_vc_insert of the same pass: rows <= n_miss of that pass; image: 33 rows bytes, 16-byte aligned
hipError_t sv_launch_vc_export(const sv_vc_args* A, uint64_t n_miss, uint64_t rows, void* image, hipStream_t s) {
  if (!rows) return hipSuccess;
  if (rows > n_miss || n_miss > A->n || !image || ((uintptr_t)image & 15u)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sv_vc_export_kernel, dim3((unsigned)sv_vc_blocks(2 * rows)), dim3(SV_VCBLOCK), 0, s, *A, rows,
                     (uint8_t*)image);
  return hipGetLastError();
}

hipError_t sv_launch_vc_feed(const sv_vc_feed_args* A, hipStream_t s) {
  if (!A->n) return hipSuccess;
  if (A->n >= SV_VC_UNCLAIMED || !A->sets) return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)sv_vc_blocks(A->n);
  hipLaunchKernelGGL(sv_vc_feed_claim_kernel, dim3(blocks), dim3(SV_VCBLOCK), 0, s, *A);
  hipLaunchKernelGGL(sv_vc_feed_store_kernel, dim3(blocks), dim3(SV_VCBLOCK), 0, s, *A);
  return hipGetLastError();
}

hipError_t sv_launch_vc_lookup(const void* tab, uint64_t sets, const void* keys, uint64_t n, void* out,
                               hipStream_t s) {
  if (!n) return hipSuccess;
  if (n > SV_VC_MAX_ITEMS || !sets) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sv_vc_lookup_kernel, dim3((unsigned)sv_vc_blocks(n)), dim3(SV_VCBLOCK), 0, s,
                     (const sv_vc_entry*)tab, sets, (const uint32_t*)keys, n, (uint8_t*)out);
  return hipGetLastError();
}

hipError_t sv_launch_vc_bitmap(const void* verdict, uint64_t n, void* bitmap, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(sv_vc_bitmap_kernel, dim3((unsigned)sv_vc_blocks(n)), dim3(SV_VCBLOCK), 0, s,
                     (const uint8_t*)verdict, n, (uint64_t*)bitmap);
  return hipGetLastError();
}

}  // extern "C"
