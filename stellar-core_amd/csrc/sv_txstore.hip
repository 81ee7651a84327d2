// gfx950 kernels of the account store's replica on a device slot (txstore.h;
// the host side is acctstore.h, the only writer of the index): the ledger forms
// of the by-account check calls name store accounts by their 32-byte ID, and
// the expansion kernels (sv_txacct.hip, the stride instantiations) then read
// the replica's rows in place.
//
//   scatter  behind an upsert / erase on the host: a quad of lanes per dirty
//            account row copies the row's staged record into the
//            struct-of-arrays replica in 16-byte pieces (lane 0 also the words
//            that are no multiple of 16 bytes: types, thresholds, counts), a
//            quad per dirty payload row its 64 bytes, and one lane per dirty
//            index slot writes that slot
//   lookup   one lane per account entry of a call: an entry by ID hashes the ID
//            (accthash.h, the host's function) and probes at most max_probe
//            slots, comparing all 32 bytes at every occupied one; an entry
//            that names a local account becomes that account's borrowed row.
//            Out: the row, or `rows` (a value past the table: no account) and
//            a found byte
//   local    one lane per local account of a call: the caller's CSR account
//            into its borrowed row past `accounts` at the store's stride, its
//            type-3 signers' payloads into the borrowed payload rows, and the
//            row's acnt / rank (txacct.h sv_acct_count)
//   gather   sv_account_store_read: a quad per looked-up row, the account in
//            the caller's layout (absent: zeros)
//
// Rules, as in sv_txacct.hip: no atomics; no lane or workgroup waits for
// another; ordering only by kernel boundaries on the slot's one stream, under
// the slot's mutex; every loop bounded by a launch argument or a constant
// (max_probe, 20 signers, the 57 pieces of a row, the row counts); ordinary
// vector stores; every index read from memory -- a staged row or slot number,
// an index word, a payload row -- is checked against its array before it is
// used, so nothing is written or read outside the arrays' stated sizes; no
// scratch.
#include <hip/hip_runtime.h>

#include "accthash.h"
#include "launch.h"
#include "sv_common.h"
#include "txacct.h"
#include "txstore.h"

static_assert(SV_ACCT_STRIDE == 20, "the records and the replica's sections are laid out for 20 signers");

namespace {

__device__ __forceinline__ void copy16(void* d, const void* s) { *(uint4*)d = *(const uint4*)s; }
__device__ __forceinline__ void zero16(void* d) { *(uint4*)d = make_uint4(0, 0, 0, 0); }

// the replica as the expansion's table
__host__ __device__ __forceinline__ sv_acct_tab store_as_tab(const sv_store_tab& R) {
  sv_acct_tab T;
  T.key = R.key;
  T.thr = R.thr;
  T.scnt = R.scnt;
  T.stype = R.stype;
  T.sweight = R.sweight;
  T.skey = R.skey;
  T.spay = R.spay;
  T.pay = R.pay;
  T.plen = R.plen;
  T.na = R.rows;
  T.ns = (uint64_t)SV_ACCT_STRIDE * R.rows;
  T.np = R.prows;
  return T;
}

}  // namespace

__global__ __launch_bounds__(SV_STORE_BLOCK) void sv_store_scatter_kernel(sv_store_tab R, const uint8_t* rec,
                                                                          uint32_t n_rows, uint32_t n_pays,
                                                                          uint32_t n_slots) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_STORE_BLOCK + threadIdx.x;
  const unsigned l = (unsigned)(i & 3);
  const uint64_t q = i >> 2;
  if (q < n_rows) {
    const uint8_t* p = rec + (uint64_t)SV_STORE_ROW_REC * q;
    const uint32_t row = *(const uint32_t*)(p + 932);
    if (row >= R.accounts) return;
    // pieces: key 0-1 | signer keys 2-41 | weights 42-46 | payload rows 47-51 | ranks 52-56
    SV_NOUNROLL for (unsigned k = l; k < 57; k += 4) {
      uint8_t* d;
      if (k < 2) d = R.key + 32 * (uint64_t)row + 16 * k;
      else if (k < 42) d = R.skey + 640 * (uint64_t)row + 16 * (k - 2);
      else if (k < 47) d = (uint8_t*)R.sweight + 80 * (uint64_t)row + 16 * (k - 42);
      else if (k < 52) d = (uint8_t*)R.spay + 80 * (uint64_t)row + 16 * (k - 47);
      else d = (uint8_t*)R.rank + 80 * (uint64_t)row + 16 * (k - 52);
      copy16(d, p + 16 * k);
    }
    if (l == 0) {
      const uint32_t* w = (const uint32_t*)(p + 912);
      uint32_t* ty = (uint32_t*)(R.stype + 20 * (uint64_t)row);
      SV_UNROLL for (int j = 0; j < 5; ++j) ty[j] = w[j];
      const uint32_t* t = (const uint32_t*)(p + 944);
      ((uint32_t*)R.thr)[row] = t[0];
      R.scnt[row] = t[1] < SV_ACCT_STRIDE ? t[1] : SV_ACCT_STRIDE;
      R.acnt[2 * (uint64_t)row] = t[2];
      R.acnt[2 * (uint64_t)row + 1] = t[3];
    }
    return;
  }
  const uint64_t pq = q - n_rows;
  const uint8_t* prec = rec + (uint64_t)SV_STORE_ROW_REC * n_rows;
  if (pq < n_pays) {
    const uint8_t* p = prec + (uint64_t)SV_STORE_PAY_REC * pq;
    const uint32_t idx = *(const uint32_t*)(p + 64);
    if (idx >= R.pays) return;
    copy16(R.pay + 64 * (uint64_t)idx + 16 * l, p + 16 * l);
    if (l == 0) {
      const uint32_t len = *(const uint32_t*)(p + 68);
      R.plen[idx] = (uint8_t)(len < 64 ? len : 64);
    }
    return;
  }
  // one lane per dirty slot, behind the quads
  const uint64_t base = 4 * ((uint64_t)n_rows + n_pays);
  if (i < base) return;
  const uint64_t s = i - base;
  if (s >= n_slots) return;
  const uint32_t* srec = (const uint32_t*)(prec + (uint64_t)SV_STORE_PAY_REC * n_pays) + 2 * s;
  if (srec[0] < R.slots) R.index[srec[0]] = srec[1];
}

// bacct null: every entry is by ID.  ids null: no entry by ID is found.
__global__ __launch_bounds__(SV_STORE_BLOCK) void sv_store_lookup_kernel(sv_store_tab R, const uint32_t* bacct,
                                                                         const uint8_t* ids, uint64_t n,
                                                                         uint32_t n_local, uint32_t max_probe,
                                                                         uint32_t* row_out, uint8_t* found) {
  const uint64_t e = (uint64_t)blockIdx.x * SV_STORE_BLOCK + threadIdx.x;
  if (e >= n) return;
  uint32_t row = R.rows;
  const uint32_t b = bacct ? bacct[e] : 0xFFFFFFFFu;
  if (b != 0xFFFFFFFFu) {
    if (b < n_local) row = R.accounts + b;
  } else if (ids && R.slots) {
    const uint4 a0 = ((const uint4*)(ids + 32 * e))[0], a1 = ((const uint4*)(ids + 32 * e))[1];
    const uint32_t w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    uint32_t s = (uint32_t)sv_acct_hash(w, R.seed) & (R.slots - 1);
    SV_NOUNROLL for (uint32_t i = 0; i < max_probe; ++i, s = (s + 1) & (R.slots - 1)) {
      const uint32_t v = R.index[s];
      if (v == 0) break;
      if (v > R.accounts) continue;
      const uint4 k0 = ((const uint4*)(R.key + 32 * (uint64_t)(v - 1)))[0];
      const uint4 k1 = ((const uint4*)(R.key + 32 * (uint64_t)(v - 1)))[1];
      const uint32_t d = (k0.x ^ a0.x) | (k0.y ^ a0.y) | (k0.z ^ a0.z) | (k0.w ^ a0.w) | (k1.x ^ a1.x) |
                         (k1.y ^ a1.y) | (k1.z ^ a1.z) | (k1.w ^ a1.w);
      if (d == 0) {
        row = v - 1;
        break;
      }
    }
  }
  row_out[e] = row;
  if (found) found[e] = row < R.rows ? 1 : 0;
}

__global__ __launch_bounds__(SV_STORE_BLOCK) void sv_store_local_kernel(sv_store_tab R, sv_acct_tab L,
                                                                        uint32_t n_local) {
  const uint32_t a = blockIdx.x * SV_STORE_BLOCK + threadIdx.x;
  if (a >= n_local || a >= R.rows - R.accounts) return;
  const uint64_t row = (uint64_t)R.accounts + a;
  uint64_t s0, s1;
  (void)sv_acct_signers<false>(L, a, &s0, &s1);
  const uint32_t n = (uint32_t)sv_acct_min(s1 - s0, SV_ACCT_STRIDE);
  copy16(R.key + 32 * row, L.key + 32 * (uint64_t)a);
  copy16(R.key + 32 * row + 16, L.key + 32 * (uint64_t)a + 16);
  SV_UNROLL for (int j = 0; j < 4; ++j) R.thr[4 * row + j] = L.thr[4 * (uint64_t)a + j];
  SV_NOUNROLL for (uint32_t j = 0; j < n; ++j) {
    const uint64_t s = s0 + j, d = SV_ACCT_STRIDE * row + j;
    const uint8_t ty = L.stype[s];
    R.stype[d] = ty;
    R.sweight[d] = L.sweight[s];
    copy16(R.skey + 32 * d, L.skey + 32 * s);
    copy16(R.skey + 32 * d + 16, L.skey + 32 * s + 16);
    if (ty != 3) continue;
    // the signer's own borrowed payload row
    const uint64_t prow = (uint64_t)R.pays + (uint64_t)SV_ACCT_STRIDE * a + j;
    R.spay[d] = (uint32_t)prow;
    if (prow >= R.prows) continue;
    const uint64_t pi = L.spay ? L.spay[s] : L.np;
    if (pi < L.np) {
      SV_UNROLL for (int k = 0; k < 4; ++k) copy16(R.pay + 64 * prow + 16 * k, L.pay + 64 * pi + 16 * k);
      R.plen[prow] = L.plen[pi];
    } else {
      SV_UNROLL for (int k = 0; k < 4; ++k) zero16(R.pay + 64 * prow + 16 * k);
      R.plen[prow] = 0;
    }
  }
  R.scnt[row] = n;
  sv_acct_count<true>(store_as_tab(R), row, R.acnt, R.rank);
}

// The caller's layout of sv_account_store_read, n accounts: thr n x 4 | n_signers n (u32) | type n x 20 |
// weight n x 20 (u32) | key n x 20 x 32 | payload n x 20 x 64 | payload_len n x 20.
struct sv_store_read_out {
  uint8_t* thr;
  uint32_t* n_signers;
  uint8_t* stype;
  uint32_t* sweight;
  uint8_t* skey;
  uint8_t* spayload;
  uint8_t* splen;
};

__global__ __launch_bounds__(SV_STORE_BLOCK) void sv_store_gather_kernel(sv_store_tab R, const uint32_t* rows,
                                                                         uint64_t n, sv_store_read_out O) {
  const uint64_t i = ((uint64_t)blockIdx.x * SV_STORE_BLOCK + threadIdx.x) >> 2;
  const unsigned l = threadIdx.x & 3;
  if (i >= n) return;
  const uint64_t row = rows[i];
  const bool have = row < R.accounts;
  const uint32_t ns = have ? (R.scnt[row] < SV_ACCT_STRIDE ? R.scnt[row] : SV_ACCT_STRIDE) : 0;
  if (l == 0) {
    SV_UNROLL for (int j = 0; j < 4; ++j) O.thr[4 * i + j] = have ? R.thr[4 * row + j] : 0;
    O.n_signers[i] = ns;
  }
  SV_NOUNROLL for (uint32_t j = l; j < SV_ACCT_STRIDE; j += 4) {
    const uint64_t d = SV_ACCT_STRIDE * i + j, s = SV_ACCT_STRIDE * row + j;
    const bool live = j < ns;
    const uint8_t ty = live ? R.stype[s] : 0;
    O.stype[d] = ty;
    O.sweight[d] = live ? R.sweight[s] : 0;
    if (live) {
      copy16(O.skey + 32 * d, R.skey + 32 * s);
      copy16(O.skey + 32 * d + 16, R.skey + 32 * s + 16);
    } else {
      zero16(O.skey + 32 * d);
      zero16(O.skey + 32 * d + 16);
    }
    const uint64_t p = live && ty == 3 ? R.spay[s] : R.pays;
    if (p < R.pays) {
      SV_UNROLL for (int k = 0; k < 4; ++k) copy16(O.spayload + 64 * d + 16 * k, R.pay + 64 * p + 16 * k);
      O.splen[d] = R.plen[p];
    } else {
      SV_UNROLL for (int k = 0; k < 4; ++k) zero16(O.spayload + 64 * d + 16 * k);
      O.splen[d] = 0;
    }
  }
}

extern "C" {

int sv_store_block(void) { return SV_STORE_BLOCK; }

// the bytes of sv_launch_store_gather's output for n accounts, and its sections
size_t sv_store_read_bytes(uint64_t n) { return (size_t)(4 + 4 + 20 + 80 + 640 + 1280 + 20) * n + 16 * 8; }

void sv_store_tab_as_acct(const sv_store_tab* R, sv_acct_tab* T) { *T = store_as_tab(*R); }

hipError_t sv_launch_store_scatter(const sv_store_tab* R, const void* rec, uint32_t n_rows, uint32_t n_pays,
                                   uint32_t n_slots, hipStream_t s) {
  const uint64_t lanes = 4 * ((uint64_t)n_rows + n_pays) + n_slots;
  if (!lanes) return hipSuccess;
  hipLaunchKernelGGL(sv_store_scatter_kernel, dim3((unsigned)((lanes + SV_STORE_BLOCK - 1) / SV_STORE_BLOCK)),
                     dim3(SV_STORE_BLOCK), 0, s, *R, (const uint8_t*)rec, n_rows, n_pays, n_slots);
  return hipGetLastError();
}

hipError_t sv_launch_store_lookup(const sv_store_tab* R, const uint32_t* bacct, const void* ids, uint64_t n,
                                  uint32_t n_local, uint32_t max_probe, uint32_t* row_out, void* found,
                                  hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(sv_store_lookup_kernel, dim3((unsigned)((n + SV_STORE_BLOCK - 1) / SV_STORE_BLOCK)),
                     dim3(SV_STORE_BLOCK), 0, s, *R, bacct, (const uint8_t*)ids, n, n_local, max_probe, row_out,
                     (uint8_t*)found);
  return hipGetLastError();
}

hipError_t sv_launch_store_local(const sv_store_tab* R, const sv_acct_tab* L, uint32_t n_local, hipStream_t s) {
  if (!n_local) return hipSuccess;
  hipLaunchKernelGGL(sv_store_local_kernel, dim3((n_local + SV_STORE_BLOCK - 1) / SV_STORE_BLOCK),
                     dim3(SV_STORE_BLOCK), 0, s, *R, *L, n_local);
  return hipGetLastError();
}

// out: sv_store_read_bytes(n) bytes, 16-byte aligned; the sections in the order of sv_store_read_out, each 16-byte
// aligned (offsets: sv_store_read_offsets)
void sv_store_read_offsets(uint64_t n, size_t off[7]) {
  const size_t sz[7] = {4 * n, 4 * n, 20 * n, 80 * n, 640 * n, 1280 * n, 20 * n};
  size_t o = 0;
  for (int i = 0; i < 7; ++i) {
    off[i] = o;
    o += (sz[i] + 15) & ~(size_t)15;
  }
}

hipError_t sv_launch_store_gather(const sv_store_tab* R, const uint32_t* rows, uint64_t n, void* out, hipStream_t s) {
  if (!n) return hipSuccess;
  size_t off[7];
  sv_store_read_offsets(n, off);
  uint8_t* b = (uint8_t*)out;
  const sv_store_read_out O{b + off[0],         (uint32_t*)(b + off[1]), b + off[2], (uint32_t*)(b + off[3]),
                            b + off[4],         b + off[5],              b + off[6]};
  hipLaunchKernelGGL(sv_store_gather_kernel, dim3((unsigned)((4 * n + SV_STORE_BLOCK - 1) / SV_STORE_BLOCK)),
                     dim3(SV_STORE_BLOCK), 0, s, *R, rows, n, O);
  return hipGetLastError();
}

}  // extern "C"
