// TEST INFRASTRUCTURE ONLY: compiles the device arithmetic headers of
// stellar-core_amd/csrc for the host (g++) so tests can fuzz the field /
// scalar / point layers and run the per-lane verifier on CPU against the
// golden fixtures before the GPU run.  Never linked into the product library.
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../stellar-core_amd/csrc/verify_core.h"
#include "../../stellar-core_amd/csrc/hash_dev.h"

static std::vector<uint32_t> g_btab;
static std::once_flag g_once;

// Half-size path tables e·B and e·(2^128 B), e <= 2^(SV_LB_BITS-1): over a
// million entries, so the host build fills them lazily, only the entries a
// signature's digits select (lat_need_btab) -- test setup only.
static std::vector<uint32_t> g_lb[2];
static std::vector<uint8_t> g_lb_done[2];

static void init_btab() {
  g_btab.assign(SV_BTAB_DWORDS + 8, 0);
  // (the build container has 8 CPUs; the tables are test setup only)
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([t] {
      for (int e = t; e < SV_BTAB_ENTRIES; e += 8) sv_btab_entry(&g_btab[e * SV_BTAB_STRIDE], e);
    });
  for (auto& x : th) x.join();
  for (int t = 0; t < 2; ++t) {
    g_lb[t].assign((size_t)SV_LBTAB_ENTRIES * SV_BTAB_STRIDE + 8, 0);
    g_lb_done[t].assign(SV_LBTAB_ENTRIES, 0);
  }
}

static void lat_need_btab(const sv_lat_digits& D) {
  for (int j = 0; j < SV_LB_DIGITS; ++j) {
    const int32_t d[2] = {D.dB0[j], D.dB1[j]};
    for (int t = 0; t < 2; ++t) {
      const int e = d[t] < 0 ? -d[t] : d[t];
      if (!g_lb_done[t][e]) {
        sv_btab_entry_shift(&g_lb[t][(size_t)e * SV_BTAB_STRIDE], e, 128 * t);
        g_lb_done[t][e] = 1;
      }
    }
  }
}

static void load_words(uint32_t w[8], const uint8_t* b) { memcpy(w, b, 32); }

// Signatures whose final inversions share one exponentiation in the grouped
// host verifier below (the full-length equation; test infrastructure).
#define SV_BATCH_K 4
// Montgomery's simultaneous inversion: zi[k] = 1/z[k] for K field elements
// with one exponentiation and 3(K-1) multiplications (every z[k] != 0).
template <int K>
SV_HD void fe_batch_invert(fe zi[K], const fe z[K]) {
  fe c[K];
  c[0] = z[0];
  SV_UNROLL for (int k = 1; k < K; ++k) fe_mul(c[k], c[k - 1], z[k]);
  fe inv;
  fe_invert(inv, c[K - 1]);
  SV_UNROLL for (int k = K - 1; k > 0; --k) {
    fe_mul(zi[k], inv, c[k - 1]);
    fe_mul(inv, inv, z[k]);
  }
  zi[0] = inv;
}



extern "C" {

// field ops on 32-byte little-endian values (value < 2^255 as input)
// hash_dev.h (f4): BLAKE2b-256 verify-cache key and SHA-256; inputs at any
// byte offset (msg / data may be misaligned on purpose).
void hc_cache_key(uint8_t out[32], const uint8_t pk[32], const uint8_t sig[64], const uint8_t* msg, uint32_t len) {
  uint32_t pkw[8], sgw[16], o[8];
  memcpy(pkw, pk, 32);
  memcpy(sgw, sig, 64);
  sv_cache_key(o, pkw, sgw, msg, len);
  memcpy(out, o, 32);
}
void hc_sha256(uint8_t out[32], const uint8_t* data, uint32_t len) {
  uint32_t o[8];
  sv_sha256(o, data, len);
  memcpy(out, o, 32);
}

void hc_fe_mul(uint8_t out[32], const uint8_t a[32], const uint8_t b[32]) {
  uint32_t wa[8], wb[8], wo[8];
  load_words(wa, a); load_words(wb, b);
  fe fa, fb, fo;
  fe_frombytes(fa, wa); fe_frombytes(fb, wb);
  fe_mul(fo, fa, fb);
  fe_tobytes(wo, fo);
  memcpy(out, wo, 32);
}

// raw-limb entry points: limbs given directly (bounds fuzzing)
void hc_fe_mul_limbs(uint32_t out_bytes[8], const uint32_t a[10], const uint32_t b[10], int dbl) {
  fe fa, fb, fo;
  memcpy(fa.v, a, 40); memcpy(fb.v, b, 40);
  if (dbl) fe_mul2(fo, fa, fb); else fe_mul(fo, fa, fb);
  fe_tobytes(out_bytes, fo);
}
void hc_fe_sq_limbs(uint32_t out_bytes[8], const uint32_t a[10], int dbl) {
  fe fa, fo;
  memcpy(fa.v, a, 40);
  if (dbl) fe_sq2(fo, fa); else fe_sq(fo, fa);
  fe_tobytes(out_bytes, fo);
}
void hc_fe_tobytes_limbs(uint32_t out_bytes[8], const uint32_t a[10]) {
  fe fa;
  memcpy(fa.v, a, 40);
  fe_tobytes(out_bytes, fa);
}
void hc_fe_invert(uint8_t out[32], const uint8_t a[32]) {
  uint32_t wa[8], wo[8];
  load_words(wa, a);
  fe fa, fo;
  fe_frombytes(fa, wa);
  fe_invert(fo, fa);
  fe_tobytes(wo, fo);
  memcpy(out, wo, 32);
}
void hc_sc_reduce512(uint8_t out[32], const uint8_t in[64]) {
  uint32_t x[16], r[8];
  memcpy(x, in, 64);
  sc_reduce512(r, x);
  memcpy(out, r, 32);
}
void hc_sha512_ram(uint8_t out[64], const uint8_t R[32], const uint8_t A[32], const uint8_t* m, uint32_t mlen,
                   int fixed) {
  uint32_t wr[8], wa[8], h[16];
  load_words(wr, R); load_words(wa, A);
  if (fixed) {
    uint32_t wm[8];
    memcpy(wm, m, 32);
    sha512_ram32(h, wr, wa, wm);
  } else {
    sha512_ram_var(h, wr, wa, m, mlen);
  }
  memcpy(out, h, 64);
}
// decompress (negate=0/1): returns ok, writes canonical encoding of the point
int hc_decompress(uint8_t out[32], const uint8_t s[32], int negate) {
  uint32_t w[8], e[8];
  load_words(w, s);
  ge_p3 p;
  bool ok = ge_frombytes(p, w, negate != 0);
  ge_p2_tobytes(e, p.X, p.Y, p.Z);
  memcpy(out, e, 32);
  return ok ? 1 : 0;
}
void hc_btab(uint32_t* out) {
  std::call_once(g_once, init_btab);
  memcpy(out, g_btab.data(), SV_BTAB_DWORDS * 4);
}

// Same grouping as sv_verify_kernel: K = SV_BATCH_K signatures share one
// inversion (fe_batch_invert); rejected rows park Z = 1 (sv_verify_pre).
void hc_verify_batch_grouped(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                             const uint32_t* len, size_t n, uint8_t* verdict) {
  std::call_once(g_once, init_btab);
  std::vector<sv_u4> slot(SV_SLOT_QUADS);
  for (size_t base = 0; base < n; base += SV_BATCH_K) {
    ge_p3 P[SV_BATCH_K];
    bool ok[SV_BATCH_K];
    fe z[SV_BATCH_K], zi[SV_BATCH_K];
    for (int k = 0; k < SV_BATCH_K; ++k) {
      const size_t i = base + k;
      if (i >= n) {
        fe_1(z[k]);
        ok[k] = false;
        continue;
      }
      uint32_t A[8], S[8], hram[16];
      alignas(16) uint32_t R[8];
      load_words(A, pk + 32 * i);
      load_words(R, sig + 64 * i);
      load_words(S, sig + 64 * i + 32);
      sha512_ram_var(hram, R, A, msg + off[i], len[i]);
      ok[k] = sv_verify_pre(P[k], A, (const sv_u4*)R, S, hram, slot.data(), 1, (const sv_u4*)g_btab.data());
      z[k] = P[k].Z;
    }
    fe_batch_invert<SV_BATCH_K>(zi, z);
    for (int k = 0; k < SV_BATCH_K && base + k < n; ++k) {
      alignas(16) uint32_t R[8];
      load_words(R, sig + 64 * (base + k));
      verdict[base + k] = (ok[k] && sv_encode_matches(P[k].X, P[k].Y, zi[k], (const sv_u4*)R)) ? 1 : 0;
    }
  }
}

void hc_verify_batch(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                     const uint32_t* len, size_t n, uint8_t* verdict) {
  std::call_once(g_once, init_btab);
  std::vector<sv_u4> slot(SV_ATAB_ENTRIES * SV_ATAB_QUADS);
  for (size_t i = 0; i < n; ++i) {
    uint32_t A[8], S[8], hram[16];
    alignas(16) uint32_t R[8];
    load_words(A, pk + 32 * i);
    load_words(R, sig + 64 * i);
    load_words(S, sig + 64 * i + 32);
    if (len[i] == 32) {
      uint32_t M[8];
      memcpy(M, msg + off[i], 32);
      sha512_ram32(hram, R, A, M);
    } else {
      sha512_ram_var(hram, R, A, msg + off[i], len[i]);
    }
    verdict[i] = sv_verify_core(A, (const sv_u4*)R, S, hram, slot.data(), 1, (const sv_u4*)g_btab.data()) ? 1 : 0;
  }
}
}

// Half-size (lattice.h) per-lane verifier.  wmin forces at least that many
// windows (the kernel runs every lane of a wave at the wave's maximum), so
// tests can check that verdicts do not depend on W.  stats (optional, n ints):
// the lane's own window count.
extern "C" void hc_verify_batch_lat(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                                    const uint32_t* len, size_t n, uint8_t* verdict, int wmin, int32_t* stats) {
  std::call_once(g_once, init_btab);
  std::vector<sv_u4> slot(SV_SLOT_QUADS_L);
  for (size_t i = 0; i < n; ++i) {
    uint32_t A[8], R[8], S[8], hram[16];
    load_words(A, pk + 32 * i);
    load_words(R, sig + 64 * i);
    load_words(S, sig + 64 * i + 32);
    sha512_ram_var(hram, R, A, msg + off[i], len[i]);
    sv_lat lat;
    sv_u4* tabA = slot.data();
    sv_u4* tabR = tabA + SV_ATAB_ENTRIES * SV_LTAB_QUADS;
    const bool ok = sv_lat_pre(lat, A, R, S, hram, tabA, tabR);
    int W = sv_lat_windows(lat.bits);
    if (stats) stats[i] = W;
    if (W < wmin) W = wmin;
    sv_lat_digits D;
    sv_lat_prepare(D, lat, S, W);
    lat_need_btab(D);
    ge_p3 P;
    sv_lat_scalarmult(P, D, W, tabA, tabR, (const sv_u4*)g_lb[0].data(), (const sv_u4*)g_lb[1].data());
    verdict[i] = (ok && sv_is_identity(P)) ? 1 : 0;
  }
}

// Euclid reduction only: c0, |c1| as 8 words each, c1neg, bits.
extern "C" int hc_lattice_reduce(const uint8_t h[32], uint8_t c0[32], uint8_t c1[32], int* c1neg) {
  uint32_t hw[8];
  load_words(hw, h);
  sv_lat lat;
  sc_lattice_reduce(lat, hw);
  memcpy(c0, lat.c0, 32);
  memcpy(c1, lat.c1, 32);
  *c1neg = lat.c1neg ? 1 : 0;
  return lat.bits;
}

// Table and record twins (tests/test_tables_cpu.py): what the kernels leave in
// memory for one another, built by the same functions on the host.
// Base-point table entry e of the table shifted by `shift` bits (36 dwords).
extern "C" void hc_btab_entry_shift(uint32_t out[SV_BTAB_STRIDE], int e, int shift) {
  sv_btab_entry_shift(out, e, shift);
}
// sv_build_ltab of a decoded encoding (negated as the kernels decode -A and
// -R): 9 entries x 40 dwords; returns whether the encoding decodes.
extern "C" int hc_build_ltab(uint32_t out[SV_ATAB_ENTRIES * SV_LTAB_QUADS * 4], const uint8_t enc[32], int negate) {
  uint32_t w[8];
  load_words(w, enc);
  ge_p3 P;
  const bool ok = ge_frombytes(P, w, negate != 0);
  std::vector<sv_u4> tab(SV_ATAB_ENTRIES * SV_LTAB_QUADS);
  sv_build_ltab(tab.data(), P);
  memcpy(out, tab.data(), tab.size() * sizeof(sv_u4));
  return ok ? 1 : 0;
}
// sv_lat_pre + sv_lat_prepare of one signature at W windows (W <= 0: the
// lane's own count): rec = dA[8] dR[8] dB0[] dB1[] as the prep kernel's record
// holds them; info = rneg, top8A, top8R, ok (sv_lat_pre's verdict of (1)-(5)
// and R's decode), the lane's own window count, the W used; tabs (optional):
// the tables of -A and -R, 2 x 9 x 40 dwords.
extern "C" void hc_lat_record(const uint8_t pk[32], const uint8_t sig[64], const uint8_t* msg, uint32_t len, int W,
                              int trivial, uint32_t* rec, int32_t info[6], uint32_t* tabs) {
  uint32_t A[8], R[8], S[8], hram[16];
  load_words(A, pk);
  load_words(R, sig);
  load_words(S, sig + 32);
  sha512_ram_var(hram, R, A, msg, len);
  std::vector<sv_u4> slot(SV_SLOT_QUADS_L);
  sv_lat lat;
  const bool ok = sv_lat_pre(lat, A, R, S, hram, slot.data(), slot.data() + SV_ATAB_ENTRIES * SV_LTAB_QUADS,
                             trivial != 0);
  const int wl = sv_lat_windows(lat.bits);
  if (W <= 0) W = wl;
  sv_lat_digits D;
  sv_lat_prepare(D, lat, S, W);
  memcpy(rec, D.dA, 32);
  memcpy(rec + 8, D.dR, 32);
  for (int j = 0; j < SV_LB_DIGITS; ++j) {
    rec[16 + j] = (uint32_t)D.dB0[j];
    rec[16 + SV_LB_DIGITS + j] = (uint32_t)D.dB1[j];
  }
  const int32_t v[6] = {D.rneg, D.top8A, D.top8R, ok, wl, W};
  memcpy(info, v, sizeof(v));
  if (tabs) memcpy(tabs, slot.data(), slot.size() * sizeof(sv_u4));
}

// Engine stubs for timing the host mirror's own bookkeeping (no crypto):
// every row valid; keyed stub returns sig[0..32) as the "key" (unique rows).
extern "C" int hc_stub_verify(const uint8_t*, const uint8_t*, const uint8_t*, const uint64_t*, const uint32_t*,
                              size_t n, uint8_t* verdict) {
  memset(verdict, 1, n);
  return 0;
}
extern "C" int hc_stub_keyed(const uint8_t*, const uint8_t* sig, const uint8_t*, const uint64_t*, const uint32_t*,
                             size_t n, uint8_t* verdict, uint8_t* keys) {
  memset(verdict, 1, n);
  for (size_t i = 0; i < n; ++i) memcpy(keys + 32 * i, sig + 64 * i, 32);
  return 0;
}

// ---------------------------------------------------------------------------
// Warm-key latency path (stellar-core_amd/csrc/comb.h): a host model of the
// comb kernel's algorithm over the same table layout -- per-key tables of
// d * 16^j * (-A), base tables of e * 256^j * B, signed digits of h and S,
// the sum of 96 entries (the first one taken as the point 2X:2Y:2Z:2T, as the
// kernel does), and the projective test against the decoded R.  Pins the
// equation and the layout on CPU before the GPU runs the own-form version.
#include "../../stellar-core_amd/csrc/comb_core.h"
#include "../../stellar-core_amd/csrc/keycache.h"

#include <map>
#include <random>
#include <string>

static std::vector<uint32_t> g_cb;
static std::once_flag g_cb_once;


static void init_cb() {
  g_cb.assign(SV_CB_DW, 0);
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([t] {
      for (int id = t; id < SV_CB_POS * SV_CB_ENT; id += 8)
        sv_comb_bentry(&g_cb[(size_t)id * SV_CE_DW], id / SV_CB_ENT, id % SV_CB_ENT);
    });
  for (auto& x : th) x.join();
}

// the comb base table (SV_CB_DW dwords) as init_cb builds it
extern "C" void hc_comb_btab(uint32_t* out) {
  std::call_once(g_cb_once, init_cb);
  memcpy(out, g_cb.data(), (size_t)SV_CB_DW * 4);
}

// tables of -A (layout of one key-cache slot); returns the key status
static uint32_t keytab_host(uint32_t* tab, const uint32_t A[8]) {
  bool ok = sv_point_canonical(A) && !sv_small_order(A);
  ge_p3 P;
  ok = ge_frombytes(P, A, true) && ok;
  ge_p1p1 Q;
  ge_cached id;
  ge_cached_identity(id);
  for (int j = 0; j < SV_KA_POS; ++j) {
    uint32_t* pe = tab + (size_t)j * SV_KA_ENT * SV_CE_DW;
    ge_cached c1, ce;
    ge_p3_to_cached(c1, P);
    sv_ce_put(pe, id);
    sv_ce_put(pe + SV_CE_DW, c1);
    ge_p3 acc = P;
    for (int e = 2; e < SV_KA_ENT; ++e) {
      ge_add_preswapped(Q, acc, c1.YpX, c1.YmX, c1.Z, c1.T2d, false, false);
      ge_p1p1_to_p3(acc, Q);
      ge_p3_to_cached(ce, acc);
      sv_ce_put(pe + e * SV_CE_DW, ce);
    }
    for (int k = 0; k < 4; ++k) {
      ge_dbl(Q, P.X, P.Y, P.Z);
      ge_p1p1_to_p3(P, Q);
    }
  }
  return ok ? SV_KEY_OK : SV_KEY_BAD;
}

static bool comb_verify_one(const uint32_t* ktab, uint32_t kst, const uint8_t* pk, const uint8_t* sig,
                            const uint8_t* msg, uint32_t mlen) {
  uint32_t A[8], R[8], S[8], hram[16], h[8], dA[8], dB[8];
  load_words(A, pk);
  load_words(R, sig);
  load_words(S, sig + 32);
  sha512_ram_var(hram, R, A, msg, mlen);
  sc_reduce512(h, hram);
  const bool s_ok = sc_is_canonical(S);
  S[7] &= 0x1fffffffu;  // (bits 253..255: S >= L is rejected by (1); every S < 2^253 unchanged)
  sc_digits_r16(dA, h);
  sc_digits_r256(dB, S);
  ge_p3 P;
  ge_p1p1 Q;
  bool first = true;
  auto add = [&](const uint32_t* ent, bool neg) {
    ge_cached c;
    sv_ce_get(c, ent, neg);
    if (first) {
      // 2 * the entry's point: ((Y+X)-(Y-X), (Y+X)+(Y-X), 2Z, 2dT / d)
      fe dinv;
      fe_const_dinv(dinv);
      fe_sub(P.X, c.YpX, c.YmX);
      fe_add(P.Y, c.YpX, c.YmX);
      fe_add(P.Z, c.Z, c.Z);
      fe_mul(P.T, c.T2d, dinv);
      if (neg) {
        fe nt;
        fe_neg(nt, P.T);
        P.T = nt;
      }
      fe_weak(P.X); fe_weak(P.Y); fe_weak(P.Z); fe_weak(P.T);
      first = false;
      return;
    }
    ge_add_preswapped(Q, P, c.YpX, c.YmX, c.Z, c.T2d, neg, false);
    ge_p1p1_to_p3(P, Q);
  };
  for (int j = 0; j < SV_KA_POS; ++j) {
    const int32_t d = (int32_t)(dA[j >> 3] << (28 - 4 * (j & 7))) >> 28;
    add(ktab + ((size_t)j * SV_KA_ENT + (uint32_t)(d < 0 ? -d : d)) * SV_CE_DW, d < 0);
  }
  for (int j = 0; j < SV_CB_POS; ++j) {
    const int32_t e = (int32_t)(dB[j >> 2] << (24 - 8 * (j & 3))) >> 24;
    add(&g_cb[((size_t)j * SV_CB_ENT + (uint32_t)(e < 0 ? -e : e)) * SV_CE_DW], e < 0);
  }
  bool r_ok = !sv_small_order(R) && sv_point_canonical(R);
  ge_p3 Rp;
  r_ok = ge_frombytes(Rp, R, false) && r_ok;
  fe t, dx, dy;
  fe_mul(t, Rp.X, P.Z);
  fe_sub(dx, P.X, t);
  fe_mul(t, Rp.Y, P.Z);
  fe_sub(dy, P.Y, t);
  return fe_iszero(dx) && fe_iszero(dy) && r_ok && s_ok && kst == SV_KEY_OK;
}

// [S]B through the comb base tables exactly as comb_verify_one computes it
// (the mask of S's bits 253..255, the signed radix-256 recoding, 32 entries),
// encoded: pins the base half for scalars S in [2^252, L), which no valid
// signature can be built to reach.
extern "C" void hc_comb_base_mul(const uint8_t s_bytes[32], uint8_t out[32]) {
  std::call_once(g_cb_once, init_cb);
  uint32_t S[8], dB[8];
  load_words(S, s_bytes);
  S[7] &= 0x1fffffffu;
  sc_digits_r256(dB, S);
  ge_p3 P;
  fe_0(P.X); fe_1(P.Y); fe_1(P.Z); fe_0(P.T);
  ge_p1p1 Q;
  for (int j = 0; j < SV_CB_POS; ++j) {
    const int32_t e = (int32_t)(dB[j >> 2] << (24 - 8 * (j & 3))) >> 24;
    ge_cached c;
    sv_ce_get(c, &g_cb[((size_t)j * SV_CB_ENT + (uint32_t)(e < 0 ? -e : e)) * SV_CE_DW], e < 0);
    ge_add_preswapped(Q, P, c.YpX, c.YmX, c.Z, c.T2d, e < 0, false);
    ge_p1p1_to_p3(P, Q);
  }
  uint32_t enc[8];
  ge_p2_tobytes(enc, P.X, P.Y, P.Z);
  memcpy(out, enc, 32);
}

extern "C" void hc_comb_verify_batch(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                                     const uint32_t* len, size_t n, uint8_t* out) {
  std::call_once(g_cb_once, init_cb);
  // one table per distinct key, built in parallel
  std::map<std::string, size_t> slot;
  std::vector<size_t> key_of(n);
  for (size_t i = 0; i < n; ++i) {
    auto it = slot.emplace(std::string((const char*)pk + 32 * i, 32), slot.size()).first;
    key_of[i] = it->second;
  }
  const size_t nk = slot.size();
  std::vector<uint32_t> tabs(nk * (size_t)SV_KEY_SLOT_DW), stat(nk);
  std::vector<const uint8_t*> kp(nk);
  for (size_t i = 0; i < n; ++i) kp[key_of[i]] = pk + 32 * i;
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      for (size_t k = t; k < nk; k += 8) {
        uint32_t A[8];
        load_words(A, kp[k]);
        stat[k] = keytab_host(&tabs[k * SV_KEY_SLOT_DW], A);
      }
    });
  for (auto& x : th) x.join();
  th.clear();
  for (int t = 0; t < 8; ++t)
    th.emplace_back([&, t] {
      for (size_t i = t; i < n; i += 8)
        out[i] = comb_verify_one(&tabs[key_of[i] * SV_KEY_SLOT_DW], stat[key_of[i]], pk + 32 * i, sig + 64 * i,
                                 msg + off[i], len[i])
                     ? 1
                     : 0;
    });
  for (auto& x : th) x.join();
}

// KeyIndex (csrc/keycache.h) against a map model under random traffic:
// returns 0, or a nonzero code naming the first inconsistency.
extern "C" int hc_keyindex_fuzz(uint64_t seed, int cap, int ops, int universe) {
  sv::KeyIndex ix;
  ix.reset((size_t)cap);
  std::mt19937_64 rng(seed);
  std::map<std::string, int32_t> model;  // key -> slot (present in the index)
  auto key = [](int k) {
    std::string s(32, '\0');
    uint64_t x = 0x9e3779b97f4a7c15ull * (uint64_t)(k + 1);
    for (int i = 0; i < 32; ++i) {
      x ^= x >> 31;
      x *= 0xbf58476d1ce4e5b9ull;
      s[i] = (char)(x >> 56);
    }
    // adversarial flavour: a quarter of the keys share their first 16 bytes
    if (k % 4 == 0) std::memset(&s[0], 0x5a, 16);
    return s;
  };
  uint64_t now = 0, gen = 0;
  for (int op = 0; op < ops; ++op) {
    ++now;
    const int k = (int)(rng() % (uint64_t)universe);
    const std::string kb = key(k);
    const uint8_t* p = (const uint8_t*)kb.data();
    const int32_t s = ix.find(p);
    auto it = model.find(kb);
    if ((s >= 0) != (it != model.end())) return 1;
    if (s >= 0) {
      if (it->second != s) return 2;
      if (std::memcmp(ix.key(s), p, 32) != 0) return 3;
      ix.touch(s, now);
      if (ix.state(s) == sv::KeyIndex::BUILDING && rng() % 2) ix.set_ready(s, ix.gen(s));
      continue;
    }
    if (!ix.admit(p)) continue;
    bool ev = false;
    const int32_t t = ix.insert(p, ++gen, now, &ev);
    if (t < 0) continue;
    if (ev) {
      // the victim must have left the model (exactly one key maps to t)
      int gone = 0;
      for (auto m = model.begin(); m != model.end();)
        if (m->second == t) {
          m = model.erase(m);
          ++gone;
        } else {
          ++m;
        }
      if (gone != 1) return 4;
    }
    model[kb] = t;
    if ((int)ix.size() != (int)model.size()) return 5;
    if ((int)ix.size() > cap) return 6;
    if (rng() % 8 == 0) ix.drop(t, gen), model.erase(kb);
  }
  // every model key still found, slots distinct
  std::vector<int> used((size_t)cap, 0);
  for (auto& m : model) {
    if (ix.find((const uint8_t*)m.first.data()) != m.second) return 7;
    if (used[(size_t)m.second]++) return 8;
  }
  return (int)ix.size() == (int)model.size() ? 0 : 9;
}

// ---------------------------------------------------------------------------
// Host staging (stellar-core_amd/csrc/host_image.h): the engine's packers and
// planners behind flat entry points, for tests/test_host_staging.py to check
// against the documented layouts.
#include "../../stellar-core_amd/csrc/host_image.h"

// A batch as the tests hold it: SoA arrays; fixed != 0: messages at that
// stride; gather: handed to the engine as pointer arrays built here; uniform:
// through uniform_form first; sub: the engine sees sub(sub) of it.
struct hs_batch {
  const uint8_t* pk;
  const uint8_t* sig;
  const uint8_t* msg;
  const uint64_t* off;
  const uint32_t* len;
  uint64_t n;
  uint32_t fixed, gather, uniform;
  uint64_t sub;
};
namespace {
struct HsIn {
  std::vector<const uint8_t*> ppk, psig, pmsg;
  sv::HostIn in;
  explicit HsIn(const hs_batch& b) {
    if (b.gather) {
      for (uint64_t i = 0; i < b.n; ++i) {
        ppk.push_back(b.pk + 32 * i);
        psig.push_back(b.sig + 64 * i);
        pmsg.push_back(b.msg ? b.msg + b.off[i] : nullptr);
      }
      in = sv::HostIn::gathered(ppk.data(), psig.data(), pmsg.data(), b.len);
    } else if (b.fixed) {
      in = sv::HostIn::fixed_len(b.pk, b.sig, b.msg, b.fixed);
    } else {
      in = sv::HostIn::soa(b.pk, b.sig, b.msg, b.off, b.len);
    }
    if (b.uniform) in = sv::uniform_form(in, b.n);
    if (b.sub) in = in.sub(b.sub);
  }
};
sv::TxIn hs_txin(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, size_t nb,
                 const uint64_t* sb, const uint8_t* pk, const uint8_t* sig) {
  return sv::TxIn{nullptr, bodies, off, len, kind, nb, sb, pk, sig};
}
static_assert(sizeof(sv::TxChunk) == 12 * sizeof(uint64_t), "hs_tx_plan hands TxChunk out as 12 words");
}  // namespace

extern "C" {

// out: o_sig, o_off, o_len, o_msg, bytes, var, msg_total, the form's fixed length
void hs_image(const hs_batch* b, uint64_t lo, uint64_t m, uint64_t out[8]) {
  HsIn h(*b);
  size_t total = 0;
  const sv::Image im = sv::image_of(h.in, lo, m, &total);
  const uint64_t v[8] = {im.o_sig, im.o_off, im.o_len, im.o_msg, im.bytes, im.var ? 1u : 0u, total, h.in.fixed};
  memcpy(out, v, sizeof(v));
}
void hs_pack(const hs_batch* b, uint64_t lo, uint64_t m, uint8_t* dst) {
  HsIn h(*b);
  size_t total = 0;
  sv::pack(h.in, lo, m, sv::image_of(h.in, lo, m, &total), dst);
}
// The early-keys path's packing (bulk.h host_slice_locked): per key_pieces
// piece its offsets, the end offset at the piece's upper bound, its rows.
void hs_pack_pieces(const hs_batch* b, uint64_t m, uint64_t part, uint8_t* dst) {
  HsIn h(*b);
  size_t total = 0;
  const sv::Image im = sv::image_of(h.in, 0, m, &total);
  const std::vector<size_t> pb = sv::key_pieces(m);
  uint64_t pos = 0;
  for (size_t k = 0; k + 1 < pb.size(); ++k) {
    pos = sv::pack_offsets(h.in, 0, pb[k], pb[k + 1], pos, im, dst);
    if (im.var && pb[k + 1] < m) ((uint64_t*)(dst + im.o_off))[pb[k + 1]] = pos;
    sv::pack_rows(h.in, 0, pb[k], pb[k + 1], im, dst, part);
  }
}
int hs_key_pieces(uint64_t m, uint64_t* out, int cap) {
  const std::vector<size_t> pb = sv::key_pieces(m);
  for (size_t i = 0; i < pb.size() && (int)i < cap; ++i) out[i] = pb[i];
  return (int)pb.size();
}
uint64_t hs_chunk_len(uint64_t c, uint64_t chunk, uint64_t left) { return sv::chunk_len(c, chunk, left); }
uint32_t hs_uniform_fixed(const uint32_t* len, uint64_t n) {
  return sv::uniform_form(sv::HostIn::soa(nullptr, nullptr, nullptr, nullptr, len), n).fixed;
}
int hs_repeated_keys(const uint8_t* pk, uint64_t n) {
  return sv::repeated_keys(sv::HostIn::soa(pk, nullptr, nullptr, nullptr, nullptr), n) ? 1 : 0;
}
// out: per chunk b0, b1, s0, s1, body_bytes, o_sig, o_off, o_sb, o_len, o_kind, o_body, bytes
int hs_tx_plan(const uint32_t* len, const uint64_t* sb, uint64_t B0, uint64_t B1, uint64_t lo, uint64_t hi,
               uint64_t max_s, uint64_t max_b, uint64_t* out, int cap) {
  const sv::TxIn in = hs_txin(nullptr, nullptr, len, nullptr, 0, sb, nullptr, nullptr);
  const std::vector<sv::TxChunk> plan = sv::tx_plan(in, B0, B1, lo, hi, max_s, max_b);
  for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) memcpy(out + 12 * i, &plan[i], sizeof(sv::TxChunk));
  return (int)plan.size();
}
void hs_tx_pack(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, uint64_t nb,
                const uint64_t* sb, const uint8_t* pk, const uint8_t* sig, const uint64_t chunk[12], uint64_t lo,
                uint64_t hi, uint8_t* dst) {
  sv::TxChunk c;
  memcpy(&c, chunk, sizeof(c));
  sv::tx_pack(hs_txin(bodies, off, len, kind, nb, sb, pk, sig), c, lo, hi, dst);
}

}  // extern "C"
