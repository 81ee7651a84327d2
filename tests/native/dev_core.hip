// TEST INFRASTRUCTURE ONLY: probe kernels over the device arithmetic headers
// of stellar-core_amd/csrc, compiled by hipcc for gfx950 with the product's
// kernel flags, so tests/test_gpu_devcore.py can run the layer's edge cases on
// the hardware as the device compiler issues them (the generated inline-asm
// products, sv_twice, the bitop3 / alignbit builtins, the DPP moves of quad.h,
// the double arithmetic of the Lehmer steps).  Never linked into the product.
//
// Every entry point is  int dc_<name>(..device pointers.., [uniform ints,] int n,
// void* stream): one kernel launch over n cases, returns the hipError_t of the
// launch.  One lane per case; the quad probes one quad per case (64-lane
// blocks, so 16 cases share a wave).  Case i reads and writes only row i of
// each buffer (row widths in dwords are given at each probe); field elements
// travel as raw limbs (10 dwords).
#include "quad.h"
#include "hash_dev.h"

namespace {

__device__ __forceinline__ void dc_ld(fe& f, const uint32_t* p) {
  SV_UNROLL for (int k = 0; k < 10; ++k) f.v[k] = p[k];
}
__device__ __forceinline__ void dc_st(uint32_t* p, const fe& f) {
  SV_UNROLL for (int k = 0; k < 10; ++k) p[k] = f.v[k];
}
template <int N>
__device__ __forceinline__ void dc_ldw(uint32_t (&w)[N], const uint32_t* p) {
  SV_UNROLL for (int k = 0; k < N; ++k) w[k] = p[k];
}
template <int N>
__device__ __forceinline__ void dc_stw(uint32_t* p, const uint32_t (&w)[N]) {
  SV_UNROLL for (int k = 0; k < N; ++k) p[k] = w[k];
}
__device__ __forceinline__ void dc_ld4(ge_p3& P, const uint32_t* p) {
  dc_ld(P.X, p);
  dc_ld(P.Y, p + 10);
  dc_ld(P.Z, p + 20);
  dc_ld(P.T, p + 30);
}
__device__ __forceinline__ void dc_st4(uint32_t* p, const fe& X, const fe& Y, const fe& Z, const fe& T) {
  dc_st(p, X);
  dc_st(p + 10, Y);
  dc_st(p + 20, Z);
  dc_st(p + 30, T);
}

}  // namespace

// one lane per case
#define DC_LANE                                         \
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  \
  if (i >= n) return
// one quad per case: whole quads retire together (c is quad-uniform)
#define DC_QUAD                                                 \
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) >> 2;   \
  if (c >= n) return;                                           \
  const uint32_t role = threadIdx.x & 3u;                       \
  const qd_role q{role == 1, role == 2, role == 3}
#define DC_GO(LANES, KERN, ...)                                                                       \
  if (n <= 0) return 0;                                                                               \
  hipLaunchKernelGGL(KERN, dim3(((LANES) + 63) / 64), dim3(64), 0, (hipStream_t)stream, __VA_ARGS__); \
  return (int)hipGetLastError()

// ------------------------------------------------------------------ field
// out[10] = op(f[10])
#define DC_FE1(NAME, ...)                                                                                    \
  __global__ void k_##NAME(uint32_t* out, const uint32_t* fp, int n) {                                       \
    DC_LANE;                                                                                                 \
    fe f, h;                                                                                                 \
    dc_ld(f, fp + 10 * i);                                                                                   \
    __VA_ARGS__;                                                                                             \
    dc_st(out + 10 * i, h);                                                                                  \
  }                                                                                                          \
  extern "C" int dc_##NAME(uint32_t* out, const uint32_t* fp, int n, void* stream) {                         \
    DC_GO(n, k_##NAME, out, fp, n);                                                                          \
  }
// out[10] = op(f[10], g[10])
#define DC_FE2(NAME, ...)                                                                                    \
  __global__ void k_##NAME(uint32_t* out, const uint32_t* fp, const uint32_t* gp, int n) {                   \
    DC_LANE;                                                                                                 \
    fe f, g, h;                                                                                              \
    dc_ld(f, fp + 10 * i);                                                                                   \
    dc_ld(g, gp + 10 * i);                                                                                   \
    __VA_ARGS__;                                                                                             \
    dc_st(out + 10 * i, h);                                                                                  \
  }                                                                                                          \
  extern "C" int dc_##NAME(uint32_t* out, const uint32_t* fp, const uint32_t* gp, int n, void* stream) {     \
    DC_GO(n, k_##NAME, out, fp, gp, n);                                                                      \
  }

DC_FE2(fe_mul, fe_mul(h, f, g))
DC_FE2(fe_mul2, fe_mul2(h, f, g))
DC_FE2(fe_mul_g19, fe19 t; fe_premul19(t, g); fe_mul_g19(h, f, g, t))
DC_FE1(fe_sq, fe_sq(h, f))
DC_FE1(fe_sq2, fe_sq2(h, f))
// the aliasing forms the code uses
DC_FE2(fe_mul_alias_hf, h = f; fe_mul(h, h, g))
DC_FE2(fe_mul_alias_hg, h = g; fe_mul(h, f, h))
DC_FE1(fe_sq_alias, h = f; fe_sq(h, h))
DC_FE1(fe_mul_same, fe_mul(h, f, f))
DC_FE1(fe_invert, fe_invert(h, f))
DC_FE1(fe_pow22523, fe_pow22523(h, f))
DC_FE2(fe_sub, fe_sub(h, f, g))
DC_FE2(fe_sub4, fe_sub4(h, f, g))
DC_FE1(fe_neg, fe_neg(h, f))
DC_FE1(fe_weak, h = f; fe_weak(h))
DC_FE1(fe_weak_even, h = f; fe_weak_even(h))

// out[70]: fe_sqn for n = 1, 2, 5, 10, 20, 50, 100
__global__ void k_fe_sqn(uint32_t* out, const uint32_t* fp, int n) {
  DC_LANE;
  fe f, h;
  dc_ld(f, fp + 10 * i);
  uint32_t* o = out + 70 * i;
  fe_sqn(h, f, 1);
  dc_st(o, h);
  fe_sqn(h, f, 2);
  dc_st(o + 10, h);
  fe_sqn(h, f, 5);
  dc_st(o + 20, h);
  fe_sqn(h, f, 10);
  dc_st(o + 30, h);
  fe_sqn(h, f, 20);
  dc_st(o + 40, h);
  fe_sqn(h, f, 50);
  dc_st(o + 50, h);
  fe_sqn(h, f, 100);
  dc_st(o + 60, h);
}
extern "C" int dc_fe_sqn(uint32_t* out, const uint32_t* fp, int n, void* stream) { DC_GO(n, k_fe_sqn, out, fp, n); }

// out[8] = fe_tobytes(f[10])
__global__ void k_fe_tobytes(uint32_t* out, const uint32_t* fp, int n) {
  DC_LANE;
  fe f;
  dc_ld(f, fp + 10 * i);
  uint32_t w[8];
  fe_tobytes(w, f);
  dc_stw(out + 8 * i, w);
}
extern "C" int dc_fe_tobytes(uint32_t* out, const uint32_t* fp, int n, void* stream) {
  DC_GO(n, k_fe_tobytes, out, fp, n);
}
// out[1] = fe_iszero(f) | fe_isnegative(f) << 1
__global__ void k_fe_flags(uint32_t* out, const uint32_t* fp, int n) {
  DC_LANE;
  fe f;
  dc_ld(f, fp + 10 * i);
  out[i] = (fe_iszero(f) ? 1u : 0u) | (fe_isnegative(f) << 1);
}
extern "C" int dc_fe_flags(uint32_t* out, const uint32_t* fp, int n, void* stream) { DC_GO(n, k_fe_flags, out, fp, n); }
// out[10] = fe_frombytes(w[8])
__global__ void k_fe_frombytes(uint32_t* out, const uint32_t* wp, int n) {
  DC_LANE;
  uint32_t w[8];
  dc_ldw(w, wp + 8 * i);
  fe h;
  fe_frombytes(h, w);
  dc_st(out + 10 * i, h);
}
extern "C" int dc_fe_frombytes(uint32_t* out, const uint32_t* wp, int n, void* stream) {
  DC_GO(n, k_fe_frombytes, out, wp, n);
}
// out[10] = h[10] after fe_cmov(h, f[10], cond[1] != 0)
__global__ void k_fe_cmov(uint32_t* out, const uint32_t* hp, const uint32_t* fp, const uint32_t* cond, int n) {
  DC_LANE;
  fe f, h;
  dc_ld(h, hp + 10 * i);
  dc_ld(f, fp + 10 * i);
  fe_cmov(h, f, cond[i] != 0);
  dc_st(out + 10 * i, h);
}
extern "C" int dc_fe_cmov(uint32_t* out, const uint32_t* hp, const uint32_t* fp, const uint32_t* cond, int n,
                          void* stream) {
  DC_GO(n, k_fe_cmov, out, hp, fp, cond, n);
}

// ----------------------------------------------------------------- scalars
// out[8] = x[16] mod L
__global__ void k_sc_reduce512(uint32_t* out, const uint32_t* xp, int n) {
  DC_LANE;
  uint32_t x[16], r[8];
  dc_ldw(x, xp + 16 * i);
  sc_reduce512(r, x);
  dc_stw(out + 8 * i, r);
}
extern "C" int dc_sc_reduce512(uint32_t* out, const uint32_t* xp, int n, void* stream) {
  DC_GO(n, k_sc_reduce512, out, xp, n);
}
// out[1] = s[8] < L
__global__ void k_sc_is_canonical(uint32_t* out, const uint32_t* sp, int n) {
  DC_LANE;
  uint32_t s[8];
  dc_ldw(s, sp + 8 * i);
  out[i] = sc_is_canonical(s) ? 1u : 0u;
}
extern "C" int dc_sc_is_canonical(uint32_t* out, const uint32_t* sp, int n, void* stream) {
  DC_GO(n, k_sc_is_canonical, out, sp, n);
}
// out[8] = (neg[1] ? -c1[8] : c1[8]) * S[8] mod L
__global__ void k_sc_mul_signed(uint32_t* out, const uint32_t* c1p, const uint32_t* neg, const uint32_t* Sp, int n) {
  DC_LANE;
  uint32_t c1[8], S[8], s[8];
  dc_ldw(c1, c1p + 8 * i);
  dc_ldw(S, Sp + 8 * i);
  sc_mul_signed(s, c1, neg[i] != 0, S);
  dc_stw(out + 8 * i, s);
}
extern "C" int dc_sc_mul_signed(uint32_t* out, const uint32_t* c1p, const uint32_t* neg, const uint32_t* Sp, int n,
                                void* stream) {
  DC_GO(n, k_sc_mul_signed, out, c1p, neg, Sp, n);
}
// out[8] = a[8] * b[8] + c[8] mod L
__global__ void k_sc_muladd(uint32_t* out, const uint32_t* ap, const uint32_t* bp, const uint32_t* cp, int n) {
  DC_LANE;
  uint32_t a[8], b[8], c[8], s[8];
  dc_ldw(a, ap + 8 * i);
  dc_ldw(b, bp + 8 * i);
  dc_ldw(c, cp + 8 * i);
  sc_muladd(s, a, b, c);
  dc_stw(out + 8 * i, s);
}
extern "C" int dc_sc_muladd(uint32_t* out, const uint32_t* ap, const uint32_t* bp, const uint32_t* cp, int n,
                            void* stream) {
  DC_GO(n, k_sc_muladd, out, ap, bp, cp, n);
}
// out[40] = r16[8], r256[8], r65536[8], lb d0[8], lb d1[8] of s[8]
static_assert(SV_LB_DIGITS == 8, "dc_sc_digits row layout");
__global__ void k_sc_digits(uint32_t* out, const uint32_t* sp, int n) {
  DC_LANE;
  uint32_t s[8], d[8];
  dc_ldw(s, sp + 8 * i);
  uint32_t* o = out + 40 * i;
  sc_digits_r16(d, s);
  dc_stw(o, d);
  sc_digits_r256(d, s);
  dc_stw(o + 8, d);
  sc_digits_r65536(d, s);
  dc_stw(o + 16, d);
  int32_t d0[SV_LB_DIGITS], d1[SV_LB_DIGITS];
  sc_digits_lb(d0, d1, s);
  SV_UNROLL for (int k = 0; k < 8; ++k) {
    o[24 + k] = (uint32_t)d0[k];
    o[32 + k] = (uint32_t)d1[k];
  }
}
extern "C" int dc_sc_digits(uint32_t* out, const uint32_t* sp, int n, void* stream) {
  DC_GO(n, k_sc_digits, out, sp, n);
}
// out[9] = popped digit, d[8] after sc_pop_top(d, bits)
template <int BITS>
__global__ void k_sc_pop_top(uint32_t* out, const uint32_t* dp, int n) {
  DC_LANE;
  uint32_t d[8];
  dc_ldw(d, dp + 8 * i);
  out[9 * i] = (uint32_t)sc_pop_top(d, BITS);
  dc_stw(out + 9 * i + 1, d);
}
extern "C" int dc_sc_pop_top(uint32_t* out, const uint32_t* dp, int bits, int n, void* stream) {
  if (bits == 4) { DC_GO(n, k_sc_pop_top<4>, out, dp, n); }
  if (bits == 8) { DC_GO(n, k_sc_pop_top<8>, out, dp, n); }
  if (bits == 16) { DC_GO(n, k_sc_pop_top<16>, out, dp, n); }
  return (int)hipErrorInvalidValue;
}
// out[18] = c0[8], |c1|[8], c1neg, bits of sc_lattice_reduce(h[8])
__global__ void k_sc_lattice_reduce(uint32_t* out, const uint32_t* hp, int n) {
  DC_LANE;
  uint32_t h[8];
  dc_ldw(h, hp + 8 * i);
  sv_lat lat;
  sc_lattice_reduce(lat, h);
  uint32_t* o = out + 18 * i;
  dc_stw(o, lat.c0);
  dc_stw(o + 8, lat.c1);
  o[16] = lat.c1neg ? 1u : 0u;
  o[17] = (uint32_t)lat.bits;
}
extern "C" int dc_sc_lattice_reduce(uint32_t* out, const uint32_t* hp, int n, void* stream) {
  DC_GO(n, k_sc_lattice_reduce, out, hp, n);
}

// ------------------------------------------------------- points, per lane
// out[40] = p1p1 of ge_dbl(X, Y, Z = p[30])
__global__ void k_ge_dbl(uint32_t* out, const uint32_t* pp, int n) {
  DC_LANE;
  fe X, Y, Z;
  dc_ld(X, pp + 30 * i);
  dc_ld(Y, pp + 30 * i + 10);
  dc_ld(Z, pp + 30 * i + 20);
  ge_p1p1 r;
  ge_dbl(r, X, Y, Z);
  dc_st4(out + 40 * i, r.X, r.Y, r.Z, r.T);
}
extern "C" int dc_ge_dbl(uint32_t* out, const uint32_t* pp, int n, void* stream) { DC_GO(n, k_ge_dbl, out, pp, n); }
// out[40] = p3 of ge_p1p1_convert(p[40], wantT); T = 0 when !wantT
__global__ void k_ge_p1p1_convert(uint32_t* out, const uint32_t* pp, int wantT, int n) {
  DC_LANE;
  ge_p3 in, r;
  dc_ld4(in, pp + 40 * i);
  ge_p1p1 p;
  p.X = in.X;
  p.Y = in.Y;
  p.Z = in.Z;
  p.T = in.T;
  fe_0(r.T);
  ge_p1p1_convert(r, p, wantT != 0);
  dc_st4(out + 40 * i, r.X, r.Y, r.Z, r.T);
}
extern "C" int dc_ge_p1p1_convert(uint32_t* out, const uint32_t* pp, int wantT, int n, void* stream) {
  DC_GO(n, k_ge_p1p1_convert, out, pp, wantT, n);
}
// out[40] = p1p1 of ge_add_preswapped(p[40], q[40] = qa, qb, qZ, qT2d, neg, zone)
__global__ void k_ge_add_preswapped(uint32_t* out, const uint32_t* pp, const uint32_t* qp, int neg, int zone, int n) {
  DC_LANE;
  ge_p3 p, e;
  dc_ld4(p, pp + 40 * i);
  dc_ld4(e, qp + 40 * i);
  ge_p1p1 r;
  ge_add_preswapped(r, p, e.X, e.Y, e.Z, e.T, neg != 0, zone != 0);
  dc_st4(out + 40 * i, r.X, r.Y, r.Z, r.T);
}
extern "C" int dc_ge_add_preswapped(uint32_t* out, const uint32_t* pp, const uint32_t* qp, int neg, int zone, int n,
                                    void* stream) {
  DC_GO(n, k_ge_add_preswapped, out, pp, qp, neg, zone, n);
}
// out[40] = YpX, YmX, Z, T2d of ge_p3_to_cached(p[40])
__global__ void k_ge_p3_to_cached(uint32_t* out, const uint32_t* pp, int n) {
  DC_LANE;
  ge_p3 p;
  dc_ld4(p, pp + 40 * i);
  ge_cached c;
  ge_p3_to_cached(c, p);
  dc_st4(out + 40 * i, c.YpX, c.YmX, c.Z, c.T2d);
}
extern "C" int dc_ge_p3_to_cached(uint32_t* out, const uint32_t* pp, int n, void* stream) {
  DC_GO(n, k_ge_p3_to_cached, out, pp, n);
}
// out[8] = ge_p2_tobytes(X, Y, Z = p[30])
__global__ void k_ge_p2_tobytes(uint32_t* out, const uint32_t* pp, int n) {
  DC_LANE;
  fe X, Y, Z;
  dc_ld(X, pp + 30 * i);
  dc_ld(Y, pp + 30 * i + 10);
  dc_ld(Z, pp + 30 * i + 20);
  uint32_t w[8];
  ge_p2_tobytes(w, X, Y, Z);
  dc_stw(out + 8 * i, w);
}
extern "C" int dc_ge_p2_tobytes(uint32_t* out, const uint32_t* pp, int n, void* stream) {
  DC_GO(n, k_ge_p2_tobytes, out, pp, n);
}
// out[41] = p3, ok of ge_frombytes(w[8], negate)
__global__ void k_ge_frombytes(uint32_t* out, const uint32_t* wp, int negate, int n) {
  DC_LANE;
  uint32_t w[8];
  dc_ldw(w, wp + 8 * i);
  ge_p3 h;
  const bool ok = ge_frombytes(h, w, negate != 0);
  dc_st4(out + 41 * i, h.X, h.Y, h.Z, h.T);
  out[41 * i + 40] = ok ? 1u : 0u;
}
extern "C" int dc_ge_frombytes(uint32_t* out, const uint32_t* wp, int negate, int n, void* stream) {
  DC_GO(n, k_ge_frombytes, out, wp, negate, n);
}

// ------------------------------------------------------- points on a quad
// Every lane of case c's quad writes the point it holds: out[(4 c + role) * 40].
namespace {
// this lane's operand of cached entry ent[40] = YpX, YmX, Z, T2d for qd_add:
// role 0 T2d, role 1 Z, roles 2 / 3 the (Y+X, Y-X) pair swapped when neg
__device__ __forceinline__ void dc_qd_mine(fe& o, const uint32_t* ent, uint32_t role, bool neg) {
  const uint32_t comp = role == 0 ? 3u : role == 1 ? 2u : ((role == 2) != neg ? 0u : 1u);
  dc_ld(o, ent + 10 * comp);
}
__device__ __forceinline__ void dc_stq(uint32_t* out, int c, uint32_t role, const ge_p3& P) {
  dc_st4(out + (4 * c + (int)role) * 40, P.X, P.Y, P.Z, P.T);
}
}  // namespace

// p1p1 p[40] -> p3 (T = 0 when !wantT)
__global__ void k_qd_p1p1_to_p3(uint32_t* out, const uint32_t* pp, int wantT, int n) {
  DC_QUAD;
  ge_p3 in, P;
  dc_ld4(in, pp + 40 * c);
  ge_p1p1 Q;
  Q.X = in.X;
  Q.Y = in.Y;
  Q.Z = in.Z;
  Q.T = in.T;
  fe_0(P.T);
  qd_p1p1_to_p3(P, Q, q, wantT != 0);
  dc_stq(out, c, role, P);
}
extern "C" int dc_qd_p1p1_to_p3(uint32_t* out, const uint32_t* pp, int wantT, int n, void* stream) {
  DC_GO(4 * n, k_qd_p1p1_to_p3, out, pp, wantT, n);
}
// P = 2 p[40] (T kept from the input when !wantT)
__global__ void k_qd_dbl(uint32_t* out, const uint32_t* pp, int wantT, int n) {
  DC_QUAD;
  ge_p3 P;
  dc_ld4(P, pp + 40 * c);
  qd_dbl(P, q, wantT != 0);
  dc_stq(out, c, role, P);
}
extern "C" int dc_qd_dbl(uint32_t* out, const uint32_t* pp, int wantT, int n, void* stream) {
  DC_GO(4 * n, k_qd_dbl, out, pp, wantT, n);
}
// P = p[40] + cached entry e[40], or - when neg
__global__ void k_qd_add(uint32_t* out, const uint32_t* pp, const uint32_t* ep, int neg, int wantT, int n) {
  DC_QUAD;
  ge_p3 P;
  dc_ld4(P, pp + 40 * c);
  fe mine;
  dc_qd_mine(mine, ep + 40 * c, role, neg != 0);
  qd_add(P, mine, q, neg != 0, wantT != 0);
  dc_stq(out, c, role, P);
}
extern "C" int dc_qd_add(uint32_t* out, const uint32_t* pp, const uint32_t* ep, int neg, int wantT, int n,
                         void* stream) {
  DC_GO(4 * n, k_qd_add, out, pp, ep, neg, wantT, n);
}
// 16 steps from p[40]: doubling, then + or - entry j of e[8 * 40] by bit j of mask[1]
__global__ void k_qd_chain(uint32_t* out, const uint32_t* pp, const uint32_t* ep, const uint32_t* mask, int n) {
  DC_QUAD;
  ge_p3 P;
  dc_ld4(P, pp + 40 * c);
  const uint32_t m = mask[c];
  SV_NOUNROLL for (int j = 0; j < 8; ++j) {
    const bool neg = ((m >> j) & 1u) != 0;
    qd_dbl(P, q, true);
    fe mine;
    dc_qd_mine(mine, ep + (8 * c + j) * 40, role, neg);
    qd_add(P, mine, q, neg, j == 7);
  }
  dc_stq(out, c, role, P);
}
extern "C" int dc_qd_chain(uint32_t* out, const uint32_t* pp, const uint32_t* ep, const uint32_t* mask, int n,
                           void* stream) {
  DC_GO(4 * n, k_qd_chain, out, pp, ep, mask, n);
}

// own form: lane r holds coordinate r of p[40]; the result is expanded
__global__ void k_qo_identity(uint32_t* out, int n) {
  DC_QUAD;
  fe h;
  qo_identity(h, q);
  ge_p3 P;
  qo_expand(P, h);
  dc_stq(out, c, role, P);
}
extern "C" int dc_qo_identity(uint32_t* out, int n, void* stream) { DC_GO(4 * n, k_qo_identity, out, n); }
// (also the plain qo_expand probe: ops = 0 expands the input unchanged)
__global__ void k_qo_dbl(uint32_t* out, const uint32_t* pp, int ops, int n) {
  DC_QUAD;
  fe h;
  dc_ld(h, pp + 40 * c + 10 * (int)role);
  SV_NOUNROLL for (int k = 0; k < ops; ++k) qo_dbl(h, q);
  ge_p3 P;
  qo_expand(P, h);
  dc_stq(out, c, role, P);
}
extern "C" int dc_qo_dbl(uint32_t* out, const uint32_t* pp, int ops, int n, void* stream) {
  DC_GO(4 * n, k_qo_dbl, out, pp, ops, n);
}
__global__ void k_qo_add(uint32_t* out, const uint32_t* pp, const uint32_t* ep, int neg, int n) {
  DC_QUAD;
  fe h, mine;
  dc_ld(h, pp + 40 * c + 10 * (int)role);
  qo_load_cached(mine, ep + 40 * c, role, neg != 0);
  qo_add(h, mine, q, neg != 0);
  ge_p3 P;
  qo_expand(P, h);
  dc_stq(out, c, role, P);
}
extern "C" int dc_qo_add(uint32_t* out, const uint32_t* pp, const uint32_t* ep, int neg, int n, void* stream) {
  DC_GO(4 * n, k_qo_add, out, pp, ep, neg, n);
}
__global__ void k_qo_chain(uint32_t* out, const uint32_t* pp, const uint32_t* ep, const uint32_t* mask, int n) {
  DC_QUAD;
  fe h;
  dc_ld(h, pp + 40 * c + 10 * (int)role);
  const uint32_t m = mask[c];
  SV_NOUNROLL for (int j = 0; j < 8; ++j) {
    const bool neg = ((m >> j) & 1u) != 0;
    qo_dbl(h, q);
    fe mine;
    qo_load_cached(mine, ep + (8 * c + j) * 40, role, neg);
    qo_add(h, mine, q, neg);
  }
  ge_p3 P;
  qo_expand(P, h);
  dc_stq(out, c, role, P);
}
extern "C" int dc_qo_chain(uint32_t* out, const uint32_t* pp, const uint32_t* ep, const uint32_t* mask, int n,
                           void* stream) {
  DC_GO(4 * n, k_qo_chain, out, pp, ep, mask, n);
}

// ------------------------------------------------------------------ hashes
// Messages live in one byte buffer; case i's message is buf[off[i], off[i] +
// len[i]).  The device code reads the aligned dwords around a message, so the
// caller keeps >= 8 bytes of buffer on either side of every message.
// out[16] = SHA-512(R[8] || A[8] || msg)
__global__ void k_sha512_ram_var(uint32_t* out, const uint32_t* Rp, const uint32_t* Ap, const uint8_t* buf,
                                 const uint32_t* off, const uint32_t* len, int n) {
  DC_LANE;
  uint32_t R[8], A[8], h[16];
  dc_ldw(R, Rp + 8 * i);
  dc_ldw(A, Ap + 8 * i);
  sha512_ram_var(h, R, A, buf + off[i], len[i]);
  dc_stw(out + 16 * i, h);
}
extern "C" int dc_sha512_ram_var(uint32_t* out, const uint32_t* Rp, const uint32_t* Ap, const uint8_t* buf,
                                 const uint32_t* off, const uint32_t* len, int n, void* stream) {
  DC_GO(n, k_sha512_ram_var, out, Rp, Ap, buf, off, len, n);
}
// out[16] = SHA-512(R[8] || A[8] || M[8])
__global__ void k_sha512_ram32(uint32_t* out, const uint32_t* Rp, const uint32_t* Ap, const uint32_t* Mp, int n) {
  DC_LANE;
  uint32_t R[8], A[8], M[8], h[16];
  dc_ldw(R, Rp + 8 * i);
  dc_ldw(A, Ap + 8 * i);
  dc_ldw(M, Mp + 8 * i);
  sha512_ram32(h, R, A, M);
  dc_stw(out + 16 * i, h);
}
extern "C" int dc_sha512_ram32(uint32_t* out, const uint32_t* Rp, const uint32_t* Ap, const uint32_t* Mp, int n,
                               void* stream) {
  DC_GO(n, k_sha512_ram32, out, Rp, Ap, Mp, n);
}
// out[8] = BLAKE2b-256(pk[8] || sig[16] || msg)
__global__ void k_cache_key(uint32_t* out, const uint32_t* pk, const uint32_t* sig, const uint8_t* buf,
                            const uint32_t* off, const uint32_t* len, int n) {
  DC_LANE;
  uint32_t o[8];
  sv_cache_key(o, pk + 8 * i, sig + 16 * i, buf + off[i], len[i]);
  dc_stw(out + 8 * i, o);
}
extern "C" int dc_cache_key(uint32_t* out, const uint32_t* pk, const uint32_t* sig, const uint8_t* buf,
                            const uint32_t* off, const uint32_t* len, int n, void* stream) {
  DC_GO(n, k_cache_key, out, pk, sig, buf, off, len, n);
}
// out[8] = SHA-256(msg)
__global__ void k_sha256(uint32_t* out, const uint8_t* buf, const uint32_t* off, const uint32_t* len, int n) {
  DC_LANE;
  uint32_t o[8];
  sv_sha256(o, buf + off[i], len[i]);
  dc_stw(out + 8 * i, o);
}
extern "C" int dc_sha256(uint32_t* out, const uint8_t* buf, const uint32_t* off, const uint32_t* len, int n,
                         void* stream) {
  DC_GO(n, k_sha256, out, buf, off, len, n);
}
