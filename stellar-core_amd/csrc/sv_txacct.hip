// gfx950 expansion kernels of the by-account check calls (txacct.h): from an
// account table that is on the device once, per-body account lists and
// per-check (account, level) references to the explicit tables the hinted
// pipeline and the check kernel read -- key_begin / key, pkey_begin / pkey /
// pkey_payload / pkey_len, check_needed, signer_begin / signer_type /
// signer_weight / signer_key.  The scheme is the pairing's (sv_txpair.hip):
// count, scan, fill on one stream, the output order a function of the input
// only, no atomics, no workgroup waits for another one, ordinary stores.
//
//   account  lane a: the rows account a adds to a key list / to the payload
//            candidates, and every signer's rank among them (once per account,
//            however many bodies and checks use it)
//   count    blockIdx.y == 0, lane t: body t's key rows and payload candidates
//            (sums over its account entries); blockIdx.y == 1, lane c: check
//            c's signers and its needed weight (the check finds its body by
//            scan.h's sv_csr_owner in check_begin, as sv_txcheck.hip does).
//            The block's sums go to psum
//   scan     one block per counted array: psum -> exclusive block offsets in
//            place (scan.h sv_scan_block_sums; past 65 536 items a lane sums
//            more than one block), the total to tot[] and to the array's last
//            CSR word
//   begin    the count's geometry again: the block's counts scanned in LDS
//            plus the block offset are key_begin / pkey_begin / signer_begin
//   rows     SV_ACCT_GROUP lanes per body: the body's accounts in entry order
//            (the running first rows go to erow, for the checks), the group's
//            lanes striding over an account's items -- a 32-byte key row, or a
//            candidate's key, 64-byte payload row and length, per lane.  A lane
//            per body would copy a 20-signer account's rows one after another
//            while its neighbours idle (DESIGN.md 3.11 on body-per-lane)
//   signers  SV_ACCT_GROUP lanes per check (its body from the count's search), striding over its signers
// rows and signers exist twice: for the CSR table of a by-account call, and -- the _stride kernels -- for the
// fixed-stride rows of an account store's replica (sv_txstore.hip), which the ledger forms expand in place.
//
// Device-resident tables are not validated by the host: txacct.h clamps every
// range and index, and no row is written at or past the row counts the caller
// sized the outputs for.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "scan.h"
#include "sv_common.h"
#include "txacct.h"

#define SV_ACCTBLOCK 256
static_assert(SV_ACCTBLOCK == SV_SCAN_BLOCK, "the shared scan (scan.h) is written for this block");
#define SV_ACCT_GROUP 4

struct sv_acctparams {
  sv_acct_tab T;
  sv_acct_use U;
  sv_acct_out O;
  uint32_t* acnt;   // 2 na
  uint32_t* rank;   // ns
  uint32_t* cnt_k;  // nb
  uint32_t* cnt_q;  // nb
  uint32_t* cnt_g;  // nc
  uint64_t* psum;   // blocks(nb) | blocks(nb) | blocks(nc)
  uint64_t* tot;    // 3: key rows, payload candidates, signers
  uint32_t* erow;   // 2 ne: entry e's first key row and first payload candidate (global)
  uint32_t* cbody;  // nc: the body that owns check c (the count's search, kept for the fill)
};

__host__ __device__ __forceinline__ uint64_t sv_acct_blocks(uint64_t n) {
  return (n + SV_ACCTBLOCK - 1) / SV_ACCTBLOCK;
}

__global__ __launch_bounds__(SV_ACCTBLOCK) void sv_acct_account_kernel(sv_acctparams p) {
  const uint64_t a = (uint64_t)blockIdx.x * SV_ACCTBLOCK + threadIdx.x;
  if (a < p.T.na) sv_acct_count(p.T, a, p.acnt, p.rank);
}

__global__ __launch_bounds__(SV_ACCTBLOCK) void sv_acct_count_kernel(sv_acctparams p) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_ACCTBLOCK + threadIdx.x;
  const uint64_t bb = sv_acct_blocks(p.U.nb);
  uint64_t sum;
  if (blockIdx.y == 0) {
    if (blockIdx.x >= bb) return;
    uint32_t k = 0, q = 0;
    if (i < p.U.nb) {
      sv_acct_body_count(p.T, p.U, p.acnt, i, &k, &q);
      p.cnt_k[i] = k;
      p.cnt_q[i] = q;
    }
    (void)sv_block_exscan(k, &sum);
    if (threadIdx.x == 0) p.psum[blockIdx.x] = sum;
    (void)sv_block_exscan(q, &sum);
    if (threadIdx.x == 0) p.psum[bb + blockIdx.x] = sum;
    return;
  }
  if (blockIdx.x >= sv_acct_blocks(p.U.nc)) return;
  uint32_t g = 0;
  if (i < p.U.nc) {
    const uint64_t t = sv_csr_owner(p.U.cbeg, p.U.nb, i);
    int32_t needed = 0;
    if (t < p.U.nb) g = sv_acct_check_count(p.T, p.U, p.acnt, t, i, &needed);
    p.cbody[i] = (uint32_t)(t < p.U.nb ? t : 0xffffffffu);
    p.cnt_g[i] = g;
    p.O.check_needed[i] = needed;
  }
  (void)sv_block_exscan(g, &sum);
  if (threadIdx.x == 0) p.psum[2 * bb + blockIdx.x] = sum;
}

__global__ __launch_bounds__(SV_ACCTBLOCK) void sv_acct_scan_kernel(sv_acctparams p) {
  const uint64_t bb = sv_acct_blocks(p.U.nb), cb = sv_acct_blocks(p.U.nc);
  const unsigned w = blockIdx.x;  // 0: key rows, 1: payload candidates, 2: signers
  uint64_t* ps = p.psum + (w == 0 ? 0 : w == 1 ? bb : 2 * bb);
  const uint64_t carry = sv_scan_block_sums(ps, w == 2 ? cb : bb);
  if (threadIdx.x == 0) {
    p.tot[w] = carry;
    if (w == 0) p.O.key_begin[p.U.nb] = carry;
    else if (w == 1) p.O.pkey_begin[p.U.nb] = carry;
    else p.O.signer_begin[p.U.nc] = carry;
  }
}

__global__ __launch_bounds__(SV_ACCTBLOCK) void sv_acct_begin_kernel(sv_acctparams p) {
  const uint64_t i = (uint64_t)blockIdx.x * SV_ACCTBLOCK + threadIdx.x;
  const uint64_t bb = sv_acct_blocks(p.U.nb);
  uint64_t sum;
  if (blockIdx.y == 0) {
    if (blockIdx.x >= bb) return;
    const bool live = i < p.U.nb;
    const uint64_t k = p.psum[blockIdx.x] + sv_block_exscan(live ? p.cnt_k[i] : 0, &sum);
    const uint64_t q = p.psum[bb + blockIdx.x] + sv_block_exscan(live ? p.cnt_q[i] : 0, &sum);
    if (live) {
      p.O.key_begin[i] = k;
      p.O.pkey_begin[i] = q;
    }
    return;
  }
  if (blockIdx.x >= sv_acct_blocks(p.U.nc)) return;
  const bool live = i < p.U.nc;
  const uint64_t g = p.psum[2 * bb + blockIdx.x] + sv_block_exscan(live ? p.cnt_g[i] : 0, &sum);
  if (live) p.O.signer_begin[i] = g;
}

// rows and signers: one body each, written as a kernel for a CSR table (kStride false) and for an account store's
// replica (true: txacct.h sv_acct_tab::scnt; sv_txstore.hip).  The bodies are macros and not inlined functions, so
// the CSR kernels are the plain kernels they were: through a function their instructions come out in another
// order (by reference the signers kernel also needs two more SGPRs).
#define SV_ACCT_ROWS_KERNEL(name, kStride)                                                                         \
  __global__ __launch_bounds__(SV_ACCTBLOCK) void name(sv_acctparams p) {                                          \
    const uint64_t t = (uint64_t)blockIdx.x * (SV_ACCTBLOCK / SV_ACCT_GROUP) + threadIdx.x / SV_ACCT_GROUP;        \
    const unsigned gl = threadIdx.x % SV_ACCT_GROUP;                                                               \
    if (t >= p.U.nb) return;                                                                                       \
    uint64_t e0, e1;                                                                                               \
    sv_acct_entries(p.U, t, &e0, &e1);                                                                             \
    uint64_t krow = p.O.key_begin[t], qrow = p.O.pkey_begin[t];                                                    \
    SV_NOUNROLL for (uint64_t e = e0; e < e1; ++e) {                                                               \
      if (gl == 0) {                                                                                               \
        p.erow[2 * e] = (uint32_t)krow;                                                                            \
        p.erow[2 * e + 1] = (uint32_t)qrow;                                                                        \
      }                                                                                                            \
      const uint64_t a = p.U.eacct[e];                                                                             \
      if (a >= p.T.na) continue;                                                                                   \
      const uint64_t n = (uint64_t)p.acnt[2 * a] + p.acnt[2 * a + 1];                                              \
      SV_NOUNROLL for (uint64_t j = gl; j < n; j += SV_ACCT_GROUP)                                                 \
        sv_acct_fill_row<kStride>(p.T, p.rank, a, j, krow, qrow, p.O);                                             \
      krow += p.acnt[2 * a];                                                                                       \
      qrow += p.acnt[2 * a + 1];                                                                                   \
    }                                                                                                              \
  }

#define SV_ACCT_SIGNERS_KERNEL(name, kStride)                                                                      \
  __global__ __launch_bounds__(SV_ACCTBLOCK) void name(sv_acctparams p) {                                          \
    const uint64_t c = (uint64_t)blockIdx.x * (SV_ACCTBLOCK / SV_ACCT_GROUP) + threadIdx.x / SV_ACCT_GROUP;        \
    const unsigned gl = threadIdx.x % SV_ACCT_GROUP;                                                               \
    if (c >= p.U.nc) return;                                                                                       \
    const uint64_t t = p.cbody[c];                                                                                 \
    if (t >= p.U.nb) return;                                                                                       \
    uint64_t e;                                                                                                    \
    const uint64_t a = sv_acct_check_account(p.T, p.U, t, c, &e);                                                  \
    if (a >= p.T.na) return;                                                                                       \
    const uint64_t n = p.cnt_g[c], g0 = p.O.signer_begin[c];                                                       \
    const uint64_t krow = p.erow[2 * e], qrow = p.erow[2 * e + 1];                                                 \
    SV_NOUNROLL for (uint64_t j = gl; j < n; j += SV_ACCT_GROUP)                                                   \
      sv_acct_fill_signer<kStride>(p.T, p.rank, a, j, krow, qrow, g0 + j, p.O);                                    \
  }

SV_ACCT_ROWS_KERNEL(sv_acct_rows_kernel, false)
SV_ACCT_SIGNERS_KERNEL(sv_acct_signers_kernel, false)
SV_ACCT_ROWS_KERNEL(sv_acct_rows_stride_kernel, true)
SV_ACCT_SIGNERS_KERNEL(sv_acct_signers_stride_kernel, true)

namespace {

// the table's workspace: acnt (8 na) | rank (4 ns)
inline size_t tab_ws_bytes(uint64_t na, uint64_t ns) { return sv_a16(8 * na) + sv_a16(4 * ns) + 16; }

// a call's (or chunk's) workspace: cnt_k | cnt_q | cnt_g | cbody | erow | psum | tot, every section 16-byte aligned
struct AcctWs {
  size_t o_cq, o_cg, o_cbody, o_erow, o_psum, o_tot, bytes;
};
inline AcctWs acct_ws(uint64_t nb, uint64_t ne, uint64_t nc) {
  AcctWs w;
  w.o_cq = sv_a16(4 * nb);
  w.o_cg = w.o_cq + sv_a16(4 * nb);
  w.o_cbody = w.o_cg + sv_a16(4 * nc);
  w.o_erow = w.o_cbody + sv_a16(4 * nc);
  w.o_psum = w.o_erow + sv_a16(8 * ne);
  w.o_tot = w.o_psum + sv_a16(8 * (2 * sv_acct_blocks(nb) + sv_acct_blocks(nc)));
  w.bytes = w.o_tot + 32;
  return w;
}

sv_acctparams acct_params(const sv_acct_tab& T, const void* tab_ws, const sv_acct_use& U, const sv_acct_out& O,
                          void* ws) {
  const AcctWs w = acct_ws(U.nb, U.ne, U.nc);
  uint8_t* b = (uint8_t*)ws;
  sv_acctparams p;
  p.T = T;
  p.U = U;
  p.O = O;
  p.acnt = (uint32_t*)tab_ws;
  p.rank = (uint32_t*)((uint8_t*)tab_ws + sv_a16(8 * T.na));
  p.cnt_k = (uint32_t*)b;
  p.cnt_q = (uint32_t*)(b + w.o_cq);
  p.cnt_g = (uint32_t*)(b + w.o_cg);
  p.cbody = (uint32_t*)(b + w.o_cbody);
  p.erow = (uint32_t*)(b + w.o_erow);
  p.psum = (uint64_t*)(b + w.o_psum);
  p.tot = (uint64_t*)(b + w.o_tot);
  return p;
}

}  // namespace

extern "C" {

int sv_acct_block(void) { return SV_ACCTBLOCK; }

size_t sv_acct_tab_ws_bytes(uint64_t na, uint64_t ns) { return tab_ws_bytes(na, ns); }

size_t sv_acct_ws_bytes(uint64_t nb, uint64_t ne, uint64_t nc) { return acct_ws(nb, ne, nc).bytes; }

const uint64_t* sv_acct_totals(const void* ws, uint64_t nb, uint64_t ne, uint64_t nc) {
  return (const uint64_t*)((const uint8_t*)ws + acct_ws(nb, ne, nc).o_tot);
}

hipError_t sv_launch_acct_table(const sv_acct_tab* T, void* tab_ws, hipStream_t s) {
  if (T->na == 0) return hipSuccess;
  const sv_acctparams p = acct_params(*T, tab_ws, sv_acct_use{}, sv_acct_out{}, nullptr);
  hipLaunchKernelGGL(sv_acct_account_kernel, dim3((unsigned)sv_acct_blocks(T->na)), dim3(SV_ACCTBLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t sv_launch_acct_count(const sv_acct_tab* T, const void* tab_ws, const sv_acct_use* U, const sv_acct_out* O,
                                void* ws, hipStream_t s) {
  const sv_acctparams p = acct_params(*T, tab_ws, *U, *O, ws);
  const uint64_t bb = sv_acct_blocks(U->nb), cb = sv_acct_blocks(U->nc);
  const unsigned blocks = (unsigned)(bb > cb ? bb : cb);
  if (blocks) {
    hipLaunchKernelGGL(sv_acct_count_kernel, dim3(blocks, 2), dim3(SV_ACCTBLOCK), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(sv_acct_scan_kernel, dim3(3), dim3(SV_ACCTBLOCK), 0, s, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !blocks) return e;
  hipLaunchKernelGGL(sv_acct_begin_kernel, dim3(blocks, 2), dim3(SV_ACCTBLOCK), 0, s, p);
  return hipGetLastError();
}

static hipError_t acct_fill(const sv_acct_tab* T, const void* tab_ws, const sv_acct_use* U, const sv_acct_out* O,
                            void* ws, hipStream_t s, bool stride) {
  const sv_acctparams p = acct_params(*T, tab_ws, *U, *O, ws);
  const uint64_t per = SV_ACCTBLOCK / SV_ACCT_GROUP;
  if (U->nb) {
    hipLaunchKernelGGL(stride ? sv_acct_rows_stride_kernel : sv_acct_rows_kernel,
                       dim3((unsigned)((U->nb + per - 1) / per)), dim3(SV_ACCTBLOCK), 0, s, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (U->nc && O->ng)
    hipLaunchKernelGGL(stride ? sv_acct_signers_stride_kernel : sv_acct_signers_kernel,
                       dim3((unsigned)((U->nc + per - 1) / per)), dim3(SV_ACCTBLOCK), 0, s, p);
  return hipGetLastError();
}

hipError_t sv_launch_acct_fill(const sv_acct_tab* T, const void* tab_ws, const sv_acct_use* U, const sv_acct_out* O,
                               void* ws, hipStream_t s) {
  return acct_fill(T, tab_ws, U, O, ws, s, false);
}

hipError_t sv_launch_acct_fill_stride(const sv_acct_tab* T, const void* tab_ws, const sv_acct_use* U,
                                      const sv_acct_out* O, void* ws, hipStream_t s) {
  return acct_fill(T, tab_ws, U, O, ws, s, true);
}

}  // extern "C"
