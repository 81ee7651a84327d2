// gfx950 pairing kernels: which decorated signature goes with which candidate
// signer key of its transaction, decided by the hint (the last four bytes of
// the key, SignatureUtils::doesHintMatch), and the gather of every pair's key,
// signature and contents hash into the arrays the verify launch reads in its
// 32-byte mode.  Three stages on one stream, one lane per body:
//
//   count  body t compares hint[s] with word 7 of key[k] for its signatures
//          and keys, stores its number of pairs in cnt[t]; the block's sum goes
//          to bsum[block]
//   scan   ONE block turns bsum into exclusive block offsets and the total
//          (scan.h sv_scan_block_sums): no workgroup waits for another one
//   fill   body t scans its block's cnt in LDS, adds the block offset: that is
//          pair_begin[t]; it walks its signatures and keys again in the same
//          order and writes each pair's indices and its gathered rows
//
// So the output order (body, signature, key ascending) is a function of the
// input only: no slot is handed out by an atomic.  The tile sizes of the scan
// are SV_PAIRBLOCK bodies per block and SV_PAIRBLOCK^2 bodies per single-block
// run of the second level (above it each lane of the scan block sums more than
// one block).  Device-resident CSR arrays are not validated by the host: every
// range is clamped to its array, and the fill never writes at or past n_pairs.
//
// The payload pairing (sv_ppair_*) is the same scheme over a body's
// signed-payload candidates (key, payload row, payload length): a pair exists
// iff the signature's hint equals hint(key) XOR hint(payload)
// (txcheck.h sv_payload_hint), the order is (body, signature, candidate), and
// the fill gathers key, signature, the 64-byte payload row as the pair's
// message slot and the slot's offset and length for a variable-length verify
// launch.  Its count kernel writes its own cnt / bsum, the scan kernel above
// runs on them unchanged, and its total lands in the word behind the ed25519
// total, so one 16-byte copy brings both counts back.  Most bodies have no
// payload candidate: such a lane reads its two CSR words and nothing else.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "scan.h"
#include "sv_common.h"
#include "txcheck.h"

#define SV_PAIRBLOCK 256
static_assert(SV_PAIRBLOCK == SV_SCAN_BLOCK, "the shared scan (scan.h) is written for this block");

struct sv_pairparams {
  const uint64_t* sig_begin;  // n_bodies + 1
  const uint64_t* key_begin;  // n_bodies + 1
  const uint32_t* hint;       // n_sigs words
  const uint4* sig;           // n_sigs x 64 B
  const uint4* key;           // n_keys x 32 B
  uint64_t n_bodies, n_sigs, n_keys;
  uint64_t* cnt;              // n_bodies
  uint64_t* bsum;             // blocks (count: sums; after scan: exclusive offsets)
  uint64_t* total;            // 1
  uint64_t* pair_begin;       // n_bodies + 1
};

struct sv_fillparams {
  sv_pairparams q;
  uint64_t n_pairs;           // slots of the pair arrays (the scan's total)
  uint32_t* pair_sig;
  uint32_t* pair_key;
  uint4* gkey;                // n_pairs x 32 B
  uint4* gsig;                // n_pairs x 64 B
  uint4* gmsg;                // n_pairs x 32 B
  const uint4* digests;       // n_bodies x 32 B: the contents hashes (sv_launch_txhash ran before)
};

struct sv_range {
  uint64_t s0, s1, k0, k1;
};

__device__ __forceinline__ sv_range sv_pair_range(const sv_pairparams& q, uint64_t t) {
  sv_range r;
  r.s1 = q.sig_begin[t + 1] < q.n_sigs ? q.sig_begin[t + 1] : q.n_sigs;
  r.s0 = q.sig_begin[t] < r.s1 ? q.sig_begin[t] : r.s1;
  r.k1 = q.key_begin[t + 1] < q.n_keys ? q.key_begin[t + 1] : q.n_keys;
  r.k0 = q.key_begin[t] < r.k1 ? q.key_begin[t] : r.k1;
  return r;
}

// word 7 of key k: its bytes 28..31
__device__ __forceinline__ uint32_t sv_key_tail(const uint4* key, uint64_t k) {
  return ((const uint32_t*)key)[8 * k + 7];
}

__global__ __launch_bounds__(SV_PAIRBLOCK) void sv_pair_count_kernel(sv_pairparams q) {
  const uint64_t t = (uint64_t)blockIdx.x * SV_PAIRBLOCK + threadIdx.x;
  uint64_t c = 0;
  if (t < q.n_bodies) {
    const sv_range r = sv_pair_range(q, t);
    if (r.k1 > r.k0)
      SV_NOUNROLL for (uint64_t s = r.s0; s < r.s1; ++s) {
        const uint32_t h = q.hint[s];
        SV_NOUNROLL for (uint64_t k = r.k0; k < r.k1; ++k) c += sv_key_tail(q.key, k) == h ? 1u : 0u;
      }
    q.cnt[t] = c;
  }
  uint64_t sum;
  (void)sv_block_exscan(c, &sum);
  if (threadIdx.x == 0) q.bsum[blockIdx.x] = sum;
}

// One block: bsum[0 .. blocks) -> exclusive offsets in place, the total to
// *total and pair_begin[n_bodies].
__global__ __launch_bounds__(SV_PAIRBLOCK) void sv_pair_scan_kernel(sv_pairparams q, uint64_t blocks) {
  const uint64_t sum = sv_scan_block_sums(q.bsum, blocks);
  if (threadIdx.x == 0) {
    *q.total = sum;
    q.pair_begin[q.n_bodies] = sum;
  }
}

__global__ __launch_bounds__(SV_PAIRBLOCK) void sv_pair_fill_kernel(sv_fillparams p) {
  const sv_pairparams& q = p.q;
  const uint64_t t = (uint64_t)blockIdx.x * SV_PAIRBLOCK + threadIdx.x;
  const bool live = t < q.n_bodies;
  const uint64_t c = live ? q.cnt[t] : 0;
  uint64_t sum;
  uint64_t i = q.bsum[blockIdx.x] + sv_block_exscan(c, &sum);
  if (!live) return;
  q.pair_begin[t] = i;
  if (c == 0) return;
  const uint4 lo = p.digests[2 * t], hi = p.digests[2 * t + 1];
  const sv_range r = sv_pair_range(q, t);
  SV_NOUNROLL for (uint64_t s = r.s0; s < r.s1; ++s) {
    const uint32_t h = q.hint[s];
    SV_NOUNROLL for (uint64_t k = r.k0; k < r.k1; ++k) {
      if (sv_key_tail(q.key, k) != h) continue;
      if (i >= p.n_pairs) return;  // (the arrays changed under us: never write past them)
      p.pair_sig[i] = (uint32_t)s;
      p.pair_key[i] = (uint32_t)k;
      const uint4 k0 = q.key[2 * k], k1 = q.key[2 * k + 1];
      const uint4 s0 = q.sig[4 * s], s1 = q.sig[4 * s + 1], s2 = q.sig[4 * s + 2], s3 = q.sig[4 * s + 3];
      p.gkey[2 * i] = k0;
      p.gkey[2 * i + 1] = k1;
      p.gsig[4 * i] = s0;
      p.gsig[4 * i + 1] = s1;
      p.gsig[4 * i + 2] = s2;
      p.gsig[4 * i + 3] = s3;
      p.gmsg[2 * i] = lo;
      p.gmsg[2 * i + 1] = hi;
      ++i;
    }
  }
}

// ---- payload pairing
struct sv_ppairparams {
  sv_pairparams q;            // sig_begin, hint, sig, n_bodies, n_sigs; cnt / bsum / total / pair_begin: this pairing's
  const uint64_t* pkey_begin; // n_bodies + 1
  const uint8_t* pkey;        // n_pkeys x 32 B
  const uint8_t* payload;     // n_pkeys x 64 B
  const uint8_t* plen;        // n_pkeys
  uint64_t n_pkeys;
};

struct sv_pfillparams {
  sv_ppairparams pp;
  uint64_t n_pairs;           // slots of the pair arrays (the scan's total)
  uint32_t* pair_sig;
  uint32_t* pair_key;         // the candidate's global index
  uint4* gkey;                // n_pairs x 32 B
  uint4* gsig;                // n_pairs x 64 B
  uint4* gmsg;                // n_pairs x 64 B: the payload rows
  uint64_t* goff;             // n_pairs: 64 i
  uint32_t* glen;             // n_pairs: the payload lengths
};

// Body t's payload candidates [c0, c1) and signatures [s0, s1), clamped; the
// signature words are only read for a body that has candidates.
__device__ __forceinline__ sv_range sv_ppair_range(const sv_ppairparams& pp, uint64_t t) {
  sv_range r;
  r.k1 = pp.pkey_begin[t + 1] < pp.n_pkeys ? pp.pkey_begin[t + 1] : pp.n_pkeys;
  r.k0 = pp.pkey_begin[t] < r.k1 ? pp.pkey_begin[t] : r.k1;
  r.s0 = r.s1 = 0;
  if (r.k1 > r.k0) {
    r.s1 = pp.q.sig_begin[t + 1] < pp.q.n_sigs ? pp.q.sig_begin[t + 1] : pp.q.n_sigs;
    r.s0 = pp.q.sig_begin[t] < r.s1 ? pp.q.sig_begin[t] : r.s1;
  }
  return r;
}

__device__ __forceinline__ uint32_t sv_ppair_len(const sv_ppairparams& pp, uint64_t c) {
  const uint32_t l = pp.plen[c];
  return l > 64u ? 64u : l;
}

__device__ __forceinline__ uint32_t sv_ppair_hint(const sv_ppairparams& pp, uint64_t c) {
  return sv_payload_hint(pp.pkey + 32 * c, pp.payload + 64 * c, sv_ppair_len(pp, c));
}

__global__ __launch_bounds__(SV_PAIRBLOCK) void sv_ppair_count_kernel(sv_ppairparams pp) {
  const sv_pairparams& q = pp.q;
  const uint64_t t = (uint64_t)blockIdx.x * SV_PAIRBLOCK + threadIdx.x;
  uint64_t c = 0;
  if (t < q.n_bodies) {
    const sv_range r = sv_ppair_range(pp, t);
    SV_NOUNROLL for (uint64_t k = r.k0; k < r.k1; ++k) {
      const uint32_t h = sv_ppair_hint(pp, k);
      SV_NOUNROLL for (uint64_t s = r.s0; s < r.s1; ++s) c += q.hint[s] == h ? 1u : 0u;
    }
    q.cnt[t] = c;
  }
  uint64_t sum;
  (void)sv_block_exscan(c, &sum);
  if (threadIdx.x == 0) q.bsum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(SV_PAIRBLOCK) void sv_ppair_fill_kernel(sv_pfillparams p) {
  const sv_ppairparams& pp = p.pp;
  const sv_pairparams& q = pp.q;
  const uint64_t t = (uint64_t)blockIdx.x * SV_PAIRBLOCK + threadIdx.x;
  const bool live = t < q.n_bodies;
  const uint64_t c = live ? q.cnt[t] : 0;
  uint64_t sum;
  uint64_t i = q.bsum[blockIdx.x] + sv_block_exscan(c, &sum);
  if (!live) return;
  q.pair_begin[t] = i;
  if (c == 0) return;
  const sv_range r = sv_ppair_range(pp, t);
  SV_NOUNROLL for (uint64_t s = r.s0; s < r.s1; ++s) {
    const uint32_t h = q.hint[s];
    SV_NOUNROLL for (uint64_t k = r.k0; k < r.k1; ++k) {
      if (sv_ppair_hint(pp, k) != h) continue;
      if (i >= p.n_pairs) return;  // (the arrays changed under us: never write past them)
      p.pair_sig[i] = (uint32_t)s;
      p.pair_key[i] = (uint32_t)k;
      const uint4* key = (const uint4*)pp.pkey;
      const uint4* pay = (const uint4*)pp.payload;
      const uint4 k0 = key[2 * k], k1 = key[2 * k + 1];
      const uint4 s0 = q.sig[4 * s], s1 = q.sig[4 * s + 1], s2 = q.sig[4 * s + 2], s3 = q.sig[4 * s + 3];
      const uint4 m0 = pay[4 * k], m1 = pay[4 * k + 1], m2 = pay[4 * k + 2], m3 = pay[4 * k + 3];
      p.gkey[2 * i] = k0;
      p.gkey[2 * i + 1] = k1;
      p.gsig[4 * i] = s0;
      p.gsig[4 * i + 1] = s1;
      p.gsig[4 * i + 2] = s2;
      p.gsig[4 * i + 3] = s3;
      p.gmsg[4 * i] = m0;
      p.gmsg[4 * i + 1] = m1;
      p.gmsg[4 * i + 2] = m2;
      p.gmsg[4 * i + 3] = m3;
      p.goff[i] = 64 * i;
      p.glen[i] = sv_ppair_len(pp, k);
      ++i;
    }
  }
}

static unsigned sv_pair_blocks(uint64_t n_bodies) { return (unsigned)((n_bodies + SV_PAIRBLOCK - 1) / SV_PAIRBLOCK); }

// the pairing workspace: cnt (8 n_bodies) | bsum (8 blocks) | total (16), each 16-byte aligned
struct sv_pair_ws {
  size_t o_bsum, o_total, bytes;
};
static sv_pair_ws sv_pair_layout(uint64_t n_bodies) {
  sv_pair_ws w;
  w.o_bsum = (size_t)sv_a16(8 * n_bodies);
  w.o_total = w.o_bsum + (size_t)sv_a16(8 * (uint64_t)sv_pair_blocks(n_bodies));
  w.bytes = w.o_total + 16;
  return w;
}

extern "C" {

int sv_pair_block(void) { return SV_PAIRBLOCK; }

size_t sv_pair_ws_bytes(uint64_t n_bodies) { return sv_pair_layout(n_bodies).bytes; }

static sv_pairparams sv_pair_params(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                                    const uint64_t* key_begin, const void* key, uint64_t n_keys, uint64_t n_bodies,
                                    void* ws, uint64_t* pair_begin) {
  sv_pairparams q;
  q.sig_begin = sig_begin;
  q.key_begin = key_begin;
  q.hint = (const uint32_t*)hint;
  q.sig = (const uint4*)sig;
  q.key = (const uint4*)key;
  q.n_bodies = n_bodies;
  q.n_sigs = n_sigs;
  q.n_keys = n_keys;
  const sv_pair_ws w = sv_pair_layout(n_bodies);
  q.cnt = (uint64_t*)ws;
  q.bsum = (uint64_t*)((uint8_t*)ws + w.o_bsum);
  q.total = (uint64_t*)((uint8_t*)ws + w.o_total);
  q.pair_begin = pair_begin;
  return q;
}

// Count and scan: afterwards *sv_pair_total(ws, n_bodies) and
// pair_begin[n_bodies] hold the number of pairs.  n_bodies >= 1.
hipError_t sv_launch_pair_count(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                                const uint64_t* key_begin, const void* key, uint64_t n_keys, uint64_t n_bodies,
                                void* ws, uint64_t* pair_begin, hipStream_t s) {
  const sv_pairparams q = sv_pair_params(sig_begin, hint, sig, n_sigs, key_begin, key, n_keys, n_bodies, ws,
                                         pair_begin);
  const unsigned blocks = sv_pair_blocks(n_bodies);
  hipLaunchKernelGGL(sv_pair_count_kernel, dim3(blocks), dim3(SV_PAIRBLOCK), 0, s, q);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sv_pair_scan_kernel, dim3(1), dim3(SV_PAIRBLOCK), 0, s, q, (uint64_t)blocks);
  return hipGetLastError();
}

const uint64_t* sv_pair_total(const void* ws, uint64_t n_bodies) {
  return (const uint64_t*)((const uint8_t*)ws + sv_pair_layout(n_bodies).o_total);
}

// Fill, after sv_launch_pair_count on the same arguments and stream and after
// sv_launch_txhash has written the bodies' contents hashes to `digests`.
hipError_t sv_launch_pair_fill(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                               const uint64_t* key_begin, const void* key, uint64_t n_keys, uint64_t n_bodies,
                               void* ws, uint64_t* pair_begin, uint64_t n_pairs, uint32_t* pair_sig,
                               uint32_t* pair_key, void* gkey, void* gsig, void* gmsg, const void* digests,
                               hipStream_t s) {
  sv_fillparams p;
  p.q = sv_pair_params(sig_begin, hint, sig, n_sigs, key_begin, key, n_keys, n_bodies, ws, pair_begin);
  p.n_pairs = n_pairs;
  p.pair_sig = pair_sig;
  p.pair_key = pair_key;
  p.gkey = (uint4*)gkey;
  p.gsig = (uint4*)gsig;
  p.gmsg = (uint4*)gmsg;
  p.digests = (const uint4*)digests;
  const unsigned blocks = sv_pair_blocks(n_bodies);
  hipLaunchKernelGGL(sv_pair_fill_kernel, dim3(blocks), dim3(SV_PAIRBLOCK), 0, s, p);
  return hipGetLastError();
}

// ---- payload pairing: its workspace is cnt (8 n_bodies) | bsum (8 blocks), each 16-byte aligned; its total is the
// second word of the ed25519 pairing's total slot in `ws` (sv_pair_total(ws, n_bodies)[1])
size_t sv_ppair_ws_bytes(uint64_t n_bodies) { return sv_pair_layout(n_bodies).o_total; }

static sv_ppairparams sv_ppair_params(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                                      const uint64_t* pkey_begin, const void* pkey, const void* payload,
                                      const uint8_t* plen, uint64_t n_pkeys, uint64_t n_bodies, void* ws, void* pws,
                                      uint64_t* ppair_begin) {
  sv_ppairparams pp;
  pp.q = sv_pair_params(sig_begin, hint, sig, n_sigs, nullptr, nullptr, 0, n_bodies, pws, ppair_begin);
  pp.q.total = (uint64_t*)sv_pair_total(ws, n_bodies) + 1;
  pp.pkey_begin = pkey_begin;
  pp.pkey = (const uint8_t*)pkey;
  pp.payload = (const uint8_t*)payload;
  pp.plen = plen;
  pp.n_pkeys = n_pkeys;
  return pp;
}

// Count and scan, after sv_launch_pair_count on the same `ws` and stream: afterwards sv_pair_total(ws, n_bodies)[1]
// and ppair_begin[n_bodies] hold the number of payload pairs.  n_bodies >= 1.
hipError_t sv_launch_ppair_count(const uint64_t* sig_begin, const void* hint, uint64_t n_sigs,
                                 const uint64_t* pkey_begin, const void* pkey, const void* payload,
                                 const uint8_t* plen, uint64_t n_pkeys, uint64_t n_bodies, void* ws, void* pws,
                                 uint64_t* ppair_begin, hipStream_t s) {
  const sv_ppairparams pp = sv_ppair_params(sig_begin, hint, nullptr, n_sigs, pkey_begin, pkey, payload, plen, n_pkeys,
                                            n_bodies, ws, pws, ppair_begin);
  const unsigned blocks = sv_pair_blocks(n_bodies);
  hipLaunchKernelGGL(sv_ppair_count_kernel, dim3(blocks), dim3(SV_PAIRBLOCK), 0, s, pp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sv_pair_scan_kernel, dim3(1), dim3(SV_PAIRBLOCK), 0, s, pp.q, (uint64_t)blocks);
  return hipGetLastError();
}

// Fill, after sv_launch_ppair_count on the same arguments and stream.
hipError_t sv_launch_ppair_fill(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                                const uint64_t* pkey_begin, const void* pkey, const void* payload,
                                const uint8_t* plen, uint64_t n_pkeys, uint64_t n_bodies, void* ws, void* pws,
                                uint64_t* ppair_begin, uint64_t n_pairs, uint32_t* pair_sig, uint32_t* pair_key,
                                void* gkey, void* gsig, void* gmsg, uint64_t* goff, uint32_t* glen, hipStream_t s) {
  sv_pfillparams p;
  p.pp = sv_ppair_params(sig_begin, hint, sig, n_sigs, pkey_begin, pkey, payload, plen, n_pkeys, n_bodies, ws, pws,
                         ppair_begin);
  p.n_pairs = n_pairs;
  p.pair_sig = pair_sig;
  p.pair_key = pair_key;
  p.gkey = (uint4*)gkey;
  p.gsig = (uint4*)gsig;
  p.gmsg = (uint4*)gmsg;
  p.goff = goff;
  p.glen = glen;
  hipLaunchKernelGGL(sv_ppair_fill_kernel, dim3(sv_pair_blocks(n_bodies)), dim3(SV_PAIRBLOCK), 0, s, p);
  return hipGetLastError();
}

}  // extern "C"
