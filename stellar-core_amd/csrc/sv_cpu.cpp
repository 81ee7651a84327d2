// CPU path of the engine (include/stellar_sigverify.h sv_ed25519_verify_batch_cpu).
//
// The same per-signature algorithm as the GPU kernels -- checks (1)-(5) of
// libsodium's crypto_sign_verify_detached, SHA-512(R || A || M) mod L, the
// half-size equation [c1 S mod L] B + [c0](-A) + [c1](-R) == O of lattice.h --
// compiled from the same headers for the host (g++: SV_HD = static inline).
// Two things differ: the base-point digit radix is 2^8 instead of 2^16, so the
// two host tables (e B and e 2^128 B, e <= 128) are 2 x 129 entries built in a
// few milliseconds at first use instead of the GPU's 2 x 32769; and the field
// elements are 5 x 51-bit limbs (fe51_host.h) instead of the device's 10 x
// 25.5-bit ones, behind the same interface.
//
// Role: an engine error is never a reject -- the
// caller re-runs the batch here -- and a single verifySig is cheaper here than
// a GPU round trip.  Reference semantics: libsodium 1.0.18
// crypto_sign_verify_detached as called by PubKeyUtils::verifySig
// (src/crypto/SecretKey.cpp:461-463).  Not the oracle: nothing
// under oracle/ is compiled or linked here.
#define SV_LB_BITS 8
// field arithmetic in radix 2^51 with 128-bit products (fe51_host.h): what
// x86-64 multiplies fastest; the device form's 10 x 32-bit limbs would cost 4x
// the multiplications here
#define SV_HOST_FE51 1
#include "verify_core.h"
#include "sign_core.h"
// (hash_dev.h's whole-message hashes are device-side helpers, unused here)
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-function"
#include "txhash.h"
#include "txcheck.h"
#include "txacct.h"
#include "txresult.h"
#pragma GCC diagnostic pop

#include <algorithm>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/stellar_sigverify.h"
#include "audit.h"
#include "launch.h"

namespace {

std::vector<sv_u4> g_tab;  // table t entry e at (t * SV_LBTAB_ENTRIES + e) * SV_BTAB_QUADS
std::once_flag g_once;

void build_tables() {
  g_tab.assign((size_t)2 * SV_LBTAB_ENTRIES * SV_BTAB_QUADS, sv_u4{0, 0, 0, 0});
  const unsigned T = 4;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; ++t)
    th.emplace_back([t] {
      for (int k = (int)t; k < 2 * SV_LBTAB_ENTRIES; k += (int)T) {
        const int tab = k / SV_LBTAB_ENTRIES, e = k % SV_LBTAB_ENTRIES;
        sv_btab_entry_shift((uint32_t*)&g_tab[(size_t)k * SV_BTAB_QUADS], e, 128 * tab);
      }
    });
  for (auto& x : th) x.join();
}

inline void words(uint32_t w[8], const uint8_t* b) { std::memcpy(w, b, 32); }

bool verify_one(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t len, sv_u4* slot) {
  uint32_t A[8], R[8], S[8], hram[16];
  words(A, pk);
  words(R, sig);
  words(S, sig + 32);
  sha512_ram_var(hram, R, A, msg, len);
  sv_u4* tabA = slot;
  sv_u4* tabR = slot + SV_ATAB_ENTRIES * SV_LTAB_QUADS;
  sv_lat lat;
  const bool ok = sv_lat_pre(lat, A, R, S, hram, tabA, tabR);
  const int W = sv_lat_windows(lat.bits);
  sv_lat_digits D;
  sv_lat_prepare(D, lat, S, W);
  ge_p3 P;
  const sv_u4* t0 = g_tab.data();
  const sv_u4* t1 = t0 + (size_t)SV_LBTAB_ENTRIES * SV_BTAB_QUADS;
  sv_lat_scalarmult(P, D, W, tabA, tabR, t0, t1);
  return ok && sv_is_identity(P);
}

// ---------------------------------------------------------------- signing
// The comb tables of B (comb.h) for the host signer (sign_core.h), built at
// first use: 32 x 129 entries, a few tens of milliseconds on four threads.
std::vector<sv_u4> g_ctab;
std::once_flag g_conce;

void build_ctab() {
  g_ctab.assign((size_t)SV_CB_DW / 4, sv_u4{0, 0, 0, 0});
  const unsigned T = 4;
  std::vector<std::thread> th;
  for (unsigned t = 0; t < T; ++t)
    th.emplace_back([t] {
      for (int id = (int)t; id < SV_CB_POS * SV_CB_ENT; id += (int)T)
        sv_comb_bentry((uint32_t*)g_ctab.data() + (size_t)id * SV_CE_DW, id / SV_CB_ENT, id % SV_CB_ENT);
    });
  for (auto& x : th) x.join();
}

template <class F>
void sign_threads(size_t n, int threads, size_t grain, F f) {
  size_t T = threads > 0 ? (size_t)threads : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
  T = std::max<size_t>(1, std::min(T, n / grain));
  std::vector<std::thread> th;
  for (size_t t = 1; t < T; ++t) th.emplace_back([&, t] { f(n * t / T, n * (t + 1) / T); });
  f(0, n / T);
  for (auto& x : th) x.join();
}

// Keys once, then the messages (arguments already checked).  hint (optional):
// n x 4, bytes 28..31 of each signer's public key.
void sign_cpu(const uint8_t* seed, size_t k, const uint32_t* key_of, const uint8_t* msg, const uint64_t* msg_off,
              const uint32_t* msg_len, uint32_t fixed_len, size_t n, uint8_t* sig, uint8_t* pk, uint8_t* hint,
              int threads) {
  std::call_once(g_conce, build_ctab);
  const uint32_t* ctab = (const uint32_t*)g_ctab.data();
  std::vector<uint32_t> rec(k * SV_SIGN_REC_DW);
  sign_threads(k, threads, 8, [&](size_t a, size_t b) {
    for (size_t j = a; j < b; ++j) {
      uint32_t sd[8];
      words(sd, seed + 32 * j);
      sv_sign_expand(&rec[j * SV_SIGN_REC_DW], sd, ctab);
      if (pk) std::memcpy(pk + 32 * j, &rec[j * SV_SIGN_REC_DW + 16], 32);
    }
  });
  sign_threads(n, threads, 8, [&](size_t a, size_t b) {
    for (size_t i = a; i < b; ++i) {
      const uint32_t* r = &rec[(size_t)(key_of ? key_of[i] : i) * SV_SIGN_REC_DW];
      const uint32_t len = fixed_len ? fixed_len : msg_len[i];
      const uint8_t* m = !msg ? nullptr : fixed_len ? msg + (size_t)fixed_len * i : msg + msg_off[i];
      uint32_t s[16];
      sv_sign_msg(s, r, m, len, ctab);
      std::memcpy(sig + 64 * i, s, 64);
      if (hint) std::memcpy(hint + 4 * i, &r[23], 4);
    }
  });
  // (the expanded keys leave no copy behind)
  volatile uint32_t* z = rec.data();
  for (size_t i = 0; i < rec.size(); ++i) z[i] = 0;
}

}  // namespace

extern "C" {

int sv_sign_check(const uint8_t* seed, size_t k, const uint32_t* key_of, const uint8_t* msg, const uint64_t* msg_off,
                  const uint32_t* msg_len, uint32_t fixed_len, size_t n, const uint8_t* sig) {
  if ((uint64_t)k >> 32 || (uint64_t)n >> 32) return SV_ERR_INVALID_ARG;
  if ((k && !seed) || (n && !sig)) return SV_ERR_INVALID_ARG;
  if (n == 0) return SV_OK;
  if (!key_of && k != n) return SV_ERR_INVALID_ARG;
  if (fixed_len) {
    if (!msg) return SV_ERR_INVALID_ARG;
  } else {
    if (!msg_off || !msg_len) return SV_ERR_INVALID_ARG;
    if (!msg)
      for (size_t i = 0; i < n; ++i)
        if (msg_len[i]) return SV_ERR_INVALID_ARG;
  }
  if (key_of)
    for (size_t i = 0; i < n; ++i)
      if (key_of[i] >= k) return SV_ERR_INVALID_ARG;
  return SV_OK;
}

int sv_sign_txbodies_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                           const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                           const uint64_t* sig_begin, const uint8_t* seed, size_t k, const uint32_t* key_of, size_t n,
                           const uint8_t* hint, const uint8_t* sig) {
  if (!network_id || !sig_begin) return SV_ERR_INVALID_ARG;
  if (n_bodies && (!body_off || !body_len || !body_kind)) return SV_ERR_INVALID_ARG;
  if ((uint64_t)k >> 32 || (uint64_t)n >> 32) return SV_ERR_INVALID_ARG;
  if ((k && !seed) || (n && (!key_of || !hint || !sig))) return SV_ERR_INVALID_ARG;
  if (sig_begin[0] != 0 || sig_begin[n_bodies] != n) return SV_ERR_INVALID_ARG;
  for (size_t t = 0; t < n_bodies; ++t) {
    if (sig_begin[t + 1] < sig_begin[t] || body_kind[t] > 2) return SV_ERR_INVALID_ARG;
    if (body_len[t] && !bodies) return SV_ERR_INVALID_ARG;
  }
  for (size_t i = 0; i < n; ++i)
    if (key_of[i] >= k) return SV_ERR_INVALID_ARG;
  return SV_OK;
}

int sv_ed25519_sign_batch_cpu(const uint8_t* seed, size_t k, const uint32_t* key_of, const uint8_t* msg,
                              const uint64_t* msg_off, const uint32_t* msg_len, uint32_t fixed_msg_len, size_t n,
                              uint8_t* sig, uint8_t* pk, int threads) {
  int rc = sv_sign_check(seed, k, key_of, msg, msg_off, msg_len, fixed_msg_len, n, sig);
  if (rc) return rc;
  if (k == 0) return SV_OK;
  sign_cpu(seed, k, key_of, msg, msg_off, msg_len, fixed_msg_len, n, sig, pk, nullptr, threads);
  return SV_OK;
}

int sv_ed25519_sign_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                 const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                 const uint64_t* sig_begin, const uint8_t* seed, size_t k, const uint32_t* key_of,
                                 size_t n, uint8_t* hint, uint8_t* sig, uint8_t* pk, uint8_t* digests, int threads) {
  int rc = sv_sign_txbodies_check(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, seed, k,
                                  key_of, n, hint, sig);
  if (rc) return rc;
  // the digests through the tx-body CPU form (no signatures), then fixed-32 signing over them
  std::vector<uint8_t> own;
  if (!digests && n_bodies) {
    own.resize(32 * n_bodies);
    digests = own.data();
  }
  if (n_bodies) {
    const std::vector<uint64_t> none(n_bodies + 1, 0);
    rc = sv_ed25519_verify_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, n_bodies, none.data(),
                                        nullptr, nullptr, 0, nullptr, digests, threads);
    if (rc) return rc;
  }
  if (k == 0) return SV_OK;
  std::vector<uint8_t> msg(32 * std::max<size_t>(n, 1));
  for (size_t t = 0; t < n_bodies; ++t)
    for (uint64_t s = sig_begin[t]; s < sig_begin[t + 1]; ++s) std::memcpy(&msg[32 * s], digests + 32 * t, 32);
  sign_cpu(seed, k, key_of, msg.data(), nullptr, nullptr, 32, n, sig, pk, hint, threads);
  return SV_OK;
}

int sv_ed25519_verify_batch_cpu(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                                const uint32_t* msg_len, size_t n, uint8_t* verdict, int threads) {
  if (n == 0) return SV_OK;
  if (!pk || !sig || !msg_off || !msg_len || !verdict) return SV_ERR_INVALID_ARG;
  if (!msg)
    for (size_t i = 0; i < n; ++i)
      if (msg_len[i]) return SV_ERR_INVALID_ARG;
  std::call_once(g_once, build_tables);
  size_t T = threads > 0 ? (size_t)threads : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
  T = std::max<size_t>(1, std::min(T, n / 8));
  auto work = [&](size_t t) {
    std::vector<sv_u4> slot(SV_SLOT_QUADS_L);
    const size_t a = n * t / T, b = n * (t + 1) / T;
    for (size_t i = a; i < b; ++i)
      verdict[i] = verify_one(pk + 32 * i, sig + 64 * i, msg ? msg + msg_off[i] : nullptr, msg_len[i], slot.data())
                       ? 1
                       : 0;
  };
  if (T == 1) {
    work(0);
    return SV_OK;
  }
  std::vector<std::thread> th;
  for (size_t t = 1; t < T; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  return SV_OK;
}

// Argument check shared by the three sv_ed25519_verify_txbodies* host-array
// entry points (declared in launch.h: sv_api.cpp calls it too): SV_OK or SV_ERR_INVALID_ARG.
int sv_txbodies_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                      const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies, const uint64_t* sig_begin,
                      const uint8_t* pk, const uint8_t* sig, size_t n, const uint8_t* verdict) {
  if (!network_id || !sig_begin) return SV_ERR_INVALID_ARG;
  if (n_bodies && (!body_off || !body_len || !body_kind)) return SV_ERR_INVALID_ARG;
  if (n && (!pk || !sig || !verdict)) return SV_ERR_INVALID_ARG;
  if (sig_begin[0] != 0 || sig_begin[n_bodies] != n) return SV_ERR_INVALID_ARG;
  for (size_t t = 0; t < n_bodies; ++t) {
    if (sig_begin[t + 1] < sig_begin[t] || body_kind[t] > 2) return SV_ERR_INVALID_ARG;
    if (body_len[t] && !bodies) return SV_ERR_INVALID_ARG;
  }
  return SV_OK;
}

int sv_ed25519_verify_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                   const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                   const uint64_t* sig_begin, const uint8_t* pk, const uint8_t* sig, size_t n,
                                   uint8_t* verdict, uint8_t* digests, int threads) {
  int rc = sv_txbodies_check(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, pk, sig, n,
                             verdict);
  if (rc) return rc;
  if (n_bodies == 0) return SV_OK;
  uint32_t nid[8];
  std::memcpy(nid, network_id, 32);
  // the digests (threaded like the verification), then the signatures over them
  std::vector<uint8_t> own;
  if (!digests) {
    own.resize(32 * n_bodies);
    digests = own.data();
  }
  size_t T = threads > 0 ? (size_t)threads : std::min<size_t>(16, std::max(1u, std::thread::hardware_concurrency()));
  T = std::max<size_t>(1, std::min(T, n_bodies / 64));
  auto work = [&](size_t t) {
    const size_t a = n_bodies * t / T, b = n_bodies * (t + 1) / T;
    for (size_t i = a; i < b; ++i) {
      uint32_t d[8];
      sv_txhash<SV_TX_BYTES>(d, nid, bodies ? bodies + body_off[i] : nullptr, body_len[i], body_kind[i]);
      std::memcpy(digests + 32 * i, d, 32);
    }
  };
  {
    std::vector<std::thread> th;
    for (size_t t = 1; t < T; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
  }
  if (n == 0) return SV_OK;
  std::vector<uint8_t> msg(32 * n);
  std::vector<uint64_t> off(n);
  const std::vector<uint32_t> len(n, 32u);
  for (size_t t = 0; t < n_bodies; ++t)
    for (uint64_t s = sig_begin[t]; s < sig_begin[t + 1]; ++s) {
      std::memcpy(&msg[32 * s], digests + 32 * t, 32);
      off[s] = 32 * s;
    }
  return sv_ed25519_verify_batch_cpu(pk, sig, msg.data(), off.data(), len.data(), n, verdict, threads);
}

size_t sv_txbodies_pair_bound(const uint64_t* sig_begin, const uint64_t* key_begin, size_t n_bodies) {
  if (!sig_begin || !key_begin) return 0;
  unsigned __int128 sum = 0;
  for (size_t t = 0; t < n_bodies; ++t) {
    const uint64_t ns = sig_begin[t + 1] >= sig_begin[t] ? sig_begin[t + 1] - sig_begin[t] : 0;
    const uint64_t nk = key_begin[t + 1] >= key_begin[t] ? key_begin[t + 1] - key_begin[t] : 0;
    sum += (unsigned __int128)ns * nk;
    if (sum > (unsigned __int128)SIZE_MAX) return SIZE_MAX;
  }
  return (size_t)sum;
}

// Argument check shared by the sv_ed25519_verify_txbodies_hinted host-array
// entry points (declared in launch.h): SV_OK or SV_ERR_INVALID_ARG.
int sv_txpairs_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                     const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies, const uint64_t* sig_begin,
                     const uint8_t* hint, const uint8_t* sig, size_t n_sigs, const uint64_t* key_begin,
                     const uint8_t* key, size_t n_keys, size_t pair_cap, const uint64_t* pair_begin,
                     const uint32_t* pair_sig, const uint32_t* pair_key, const uint8_t* pair_verdict,
                     const size_t* n_pairs) {
  if (!network_id || !sig_begin || !key_begin || !pair_begin || !n_pairs) return SV_ERR_INVALID_ARG;
  if (n_bodies && (!body_off || !body_len || !body_kind)) return SV_ERR_INVALID_ARG;
  if ((uint64_t)n_sigs >> 32 || (uint64_t)n_keys >> 32) return SV_ERR_INVALID_ARG;
  if ((n_sigs && (!hint || !sig)) || (n_keys && !key)) return SV_ERR_INVALID_ARG;
  if (pair_cap && (!pair_sig || !pair_key || !pair_verdict)) return SV_ERR_INVALID_ARG;
  if (sig_begin[0] != 0 || sig_begin[n_bodies] != n_sigs) return SV_ERR_INVALID_ARG;
  if (key_begin[0] != 0 || key_begin[n_bodies] != n_keys) return SV_ERR_INVALID_ARG;
  for (size_t t = 0; t < n_bodies; ++t) {
    if (sig_begin[t + 1] < sig_begin[t] || key_begin[t + 1] < key_begin[t] || body_kind[t] > 2)
      return SV_ERR_INVALID_ARG;
    if (body_len[t] && !bodies) return SV_ERR_INVALID_ARG;
  }
  return SV_OK;
}

int sv_ed25519_verify_txbodies_hinted_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                          const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                          const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                          size_t n_sigs, const uint64_t* key_begin, const uint8_t* key, size_t n_keys,
                                          size_t pair_cap, uint64_t* pair_begin, uint32_t* pair_sig,
                                          uint32_t* pair_key, uint8_t* pair_verdict, size_t* n_pairs,
                                          uint8_t* digests, int threads) {
  int rc = sv_txpairs_check(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, hint, sig, n_sigs,
                            key_begin, key, n_keys, pair_cap, pair_begin, pair_sig, pair_key, pair_verdict, n_pairs);
  if (rc) return rc;
  auto word = [](const uint8_t* p) {
    uint32_t w;
    std::memcpy(&w, p, 4);
    return w;
  };
  // pass 1: the counts (pair_begin), so an overflow is reported before anything is written
  uint64_t total = 0;
  for (size_t t = 0; t < n_bodies; ++t) {
    pair_begin[t] = total;
    for (uint64_t s = sig_begin[t]; s < sig_begin[t + 1]; ++s) {
      const uint32_t h = word(hint + 4 * s);
      for (uint64_t k = key_begin[t]; k < key_begin[t + 1]; ++k) total += word(key + 32 * k + 28) == h ? 1 : 0;
    }
  }
  pair_begin[n_bodies] = total;
  *n_pairs = (size_t)total;
  if (total > pair_cap) return SV_ERR_PAIR_CAP;
  // the digests through the tx-body CPU form (no signatures)
  std::vector<uint8_t> own;
  if (!digests && n_bodies) {
    own.resize(32 * n_bodies);
    digests = own.data();
  }
  if (n_bodies) {
    const std::vector<uint64_t> none(n_bodies + 1, 0);
    rc = sv_ed25519_verify_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, n_bodies, none.data(),
                                        nullptr, nullptr, 0, nullptr, digests, threads);
    if (rc) return rc;
  }
  if (total == 0) return SV_OK;
  // pass 2: the pairs in (body, signature, key) order, gathered for the batch verifier
  const size_t np = (size_t)total;
  std::vector<uint8_t> gpk(32 * np), gsig(64 * np), gmsg(32 * np);
  std::vector<uint64_t> off(np);
  const std::vector<uint32_t> len(np, 32u);
  size_t i = 0;
  for (size_t t = 0; t < n_bodies; ++t)
    for (uint64_t s = sig_begin[t]; s < sig_begin[t + 1]; ++s) {
      const uint32_t h = word(hint + 4 * s);
      for (uint64_t k = key_begin[t]; k < key_begin[t + 1]; ++k) {
        if (word(key + 32 * k + 28) != h) continue;
        pair_sig[i] = (uint32_t)s;
        pair_key[i] = (uint32_t)k;
        std::memcpy(&gpk[32 * i], key + 32 * k, 32);
        std::memcpy(&gsig[64 * i], sig + 64 * s, 64);
        std::memcpy(&gmsg[32 * i], digests + 32 * t, 32);
        off[i] = 32 * i;
        ++i;
      }
    }
  return sv_ed25519_verify_batch_cpu(gpk.data(), gsig.data(), gmsg.data(), off.data(), len.data(), np, pair_verdict,
                                     threads);
}

const sv_txchecks_payload* sv_txchecks_tables(const sv_txchecks* ck) {
  if (ck->struct_size < sizeof(sv_txchecks_payload)) return nullptr;
  const sv_txchecks_payload* pt = (const sv_txchecks_payload*)ck;
  return pt->pkey_begin ? pt : nullptr;
}

// Argument check shared by the sv_ed25519_check_txbodies host-array entry
// points (declared in launch.h): SV_OK or SV_ERR_INVALID_ARG.
int sv_txchecks_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                      const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies, const uint64_t* sig_begin,
                      const uint8_t* hint, const uint8_t* sig, size_t n_sigs, const uint64_t* key_begin,
                      const uint8_t* key, size_t n_keys, const sv_txchecks* ck, const uint8_t* check_ok,
                      const uint32_t* check_weight, const uint64_t* check_used) {
  if (!network_id || !sig_begin || !key_begin || !ck || ck->struct_size < sizeof(sv_txchecks))
    return SV_ERR_INVALID_ARG;
  if (n_bodies && (!body_off || !body_len || !body_kind)) return SV_ERR_INVALID_ARG;
  if ((uint64_t)n_sigs >> 32 || (uint64_t)n_keys >> 32) return SV_ERR_INVALID_ARG;
  if ((n_sigs && (!hint || !sig)) || (n_keys && !key)) return SV_ERR_INVALID_ARG;
  if (sig_begin[0] != 0 || sig_begin[n_bodies] != n_sigs) return SV_ERR_INVALID_ARG;
  if (key_begin[0] != 0 || key_begin[n_bodies] != n_keys) return SV_ERR_INVALID_ARG;
  const size_t nc = ck->n_checks, ng = ck->n_signers;
  if (ck->protocol_version == 7) return SV_ERR_INVALID_ARG;
  if (!ck->check_begin || !ck->signer_begin) return SV_ERR_INVALID_ARG;
  if (nc && (!ck->check_needed || !check_ok || !check_weight || !check_used)) return SV_ERR_INVALID_ARG;
  if (ng && (!ck->signer_type || !ck->signer_weight || !ck->signer_key)) return SV_ERR_INVALID_ARG;
  if (ck->check_begin[0] != 0 || ck->check_begin[n_bodies] != nc) return SV_ERR_INVALID_ARG;
  if (ck->signer_begin[0] != 0 || ck->signer_begin[nc] != ng) return SV_ERR_INVALID_ARG;
  // the payload tables, when the struct has them: type-3 signers then index the payload candidates
  const sv_txchecks_payload* pt = sv_txchecks_tables(ck);
  const uint64_t* qb = pt ? pt->pkey_begin : nullptr;
  const size_t nq = pt ? pt->n_pkeys : 0;
  if (qb) {
    if ((uint64_t)nq >> 32 || (nq && (!pt->pkey || !pt->pkey_payload || !pt->pkey_len))) return SV_ERR_INVALID_ARG;
    if (qb[0] != 0 || qb[n_bodies] != nq) return SV_ERR_INVALID_ARG;
  }
  // per body: its CSR entries, signature lengths, limits, and per check of it
  // the signer range, signer types and key indices (every pass here is linear
  // in the batch, so large batches are threaded over bodies)
  auto bodies_ok = [&](size_t t0, size_t t1) {
    for (size_t t = t0; t < t1; ++t) {
      if (sig_begin[t + 1] < sig_begin[t] || key_begin[t + 1] < key_begin[t] || body_kind[t] > 2) return false;
      if (sig_begin[t + 1] > n_sigs || key_begin[t + 1] > n_keys) return false;
      if (body_len[t] && !bodies) return false;
      if (qb) {
        if (qb[t + 1] < qb[t] || qb[t + 1] > nq) return false;
        for (uint64_t i = qb[t]; i < qb[t + 1]; ++i)
          if (pt->pkey_len[i] > 64) return false;
      }
      if (ck->sig_len)
        for (uint64_t i = sig_begin[t]; i < sig_begin[t + 1]; ++i)
          if (ck->sig_len[i] > 64) return false;
      const uint64_t c0 = ck->check_begin[t], c1 = ck->check_begin[t + 1];
      if (c1 < c0 || c1 > nc) return false;
      if (c1 > c0 && sig_begin[t + 1] - sig_begin[t] > SV_TXCHECK_MAX) return false;
      for (uint64_t c = c0; c < c1; ++c) {
        const uint64_t g0 = ck->signer_begin[c], g1 = ck->signer_begin[c + 1];
        if (g1 < g0 || g1 > ng || g1 - g0 > SV_TXCHECK_MAX) return false;
        for (uint64_t g = g0; g < g1; ++g) {
          if (ck->signer_type[g] > 3) return false;
          const bool pl = qb && ck->signer_type[g] == SV_SIGNER_SIGNED_PAYLOAD;
          const uint64_t lo = pl ? qb[t] : key_begin[t], hi = pl ? qb[t + 1] : key_begin[t + 1];
          if (ck->signer_key[g] < lo || ck->signer_key[g] >= hi) return false;
        }
      }
    }
    return true;
  };
  const size_t T = std::max<size_t>(1, std::min<size_t>({(size_t)8, n_bodies / 16384,
                                                         (size_t)std::max(1u, std::thread::hardware_concurrency())}));
  if (T == 1) return bodies_ok(0, n_bodies) ? SV_OK : SV_ERR_INVALID_ARG;
  std::vector<uint8_t> good(T, 0);
  std::vector<std::thread> th;
  for (size_t i = 1; i < T; ++i)
    th.emplace_back([&, i] { good[i] = bodies_ok(n_bodies * i / T, n_bodies * (i + 1) / T) ? 1 : 0; });
  good[0] = bodies_ok(0, n_bodies / T) ? 1 : 0;
  for (auto& x : th) x.join();
  for (uint8_t g : good)
    if (!g) return SV_ERR_INVALID_ARG;
  return SV_OK;
}

int sv_ed25519_check_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                  const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                  const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                                  const uint64_t* key_begin, const uint8_t* key, size_t n_keys,
                                  const sv_txchecks* ck, uint8_t* check_ok, uint32_t* check_weight,
                                  uint64_t* check_used, uint8_t* digests, int threads) {
  int rc = sv_txchecks_check(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, hint, sig, n_sigs,
                             key_begin, key, n_keys, ck, check_ok, check_weight, check_used);
  if (rc) return rc;
  if (n_bodies == 0) return SV_OK;
  // the pairs and their verdicts through the hinted CPU form, the arrays sized by the bound
  const size_t cap = sv_txbodies_pair_bound(sig_begin, key_begin, n_bodies);
  std::vector<uint64_t> pb(n_bodies + 1);
  std::vector<uint32_t> ps(cap + 1), pk(cap + 1);
  std::vector<uint8_t> pv(cap + 1), own;
  if (!digests) {
    own.resize(32 * n_bodies);
    digests = own.data();
  }
  size_t np = 0;
  rc = sv_ed25519_verify_txbodies_hinted_cpu(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin,
                                             hint, sig, n_sigs, key_begin, key, n_keys, cap, pb.data(), ps.data(),
                                             pk.data(), pv.data(), &np, digests, threads);
  if (rc) return rc;
  // the payload pairs: (body, signature, candidate) order, verified over the candidates' payloads
  const sv_txchecks_payload* pt = sv_txchecks_tables(ck);
  const uint64_t* qb = pt ? pt->pkey_begin : nullptr;
  std::vector<uint64_t> ppb(n_bodies + 1, 0);
  std::vector<uint32_t> pps, ppk;
  std::vector<uint8_t> ppv;
  if (qb && pt->n_pkeys) {
    std::vector<uint8_t> gpk, gsig, gmsg;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    for (size_t t = 0; t < n_bodies; ++t) {
      ppb[t] = pps.size();
      if (qb[t + 1] == qb[t]) continue;
      for (uint64_t s = sig_begin[t]; s < sig_begin[t + 1]; ++s)
        for (uint64_t c = qb[t]; c < qb[t + 1]; ++c) {
          const uint32_t l = pt->pkey_len[c];
          if (sv_payload_hint(pt->pkey + 32 * c, pt->pkey_payload + 64 * c, l) != sv_txc_ld32(hint + 4 * s)) continue;
          pps.push_back((uint32_t)s);
          ppk.push_back((uint32_t)c);
          off.push_back(gmsg.size());
          len.push_back(l);
          gpk.insert(gpk.end(), pt->pkey + 32 * c, pt->pkey + 32 * c + 32);
          gsig.insert(gsig.end(), sig + 64 * s, sig + 64 * s + 64);
          gmsg.insert(gmsg.end(), pt->pkey_payload + 64 * c, pt->pkey_payload + 64 * c + 64);
        }
    }
    ppb[n_bodies] = pps.size();
    ppv.resize(pps.size() + 1);
    if (!pps.empty() && (rc = sv_ed25519_verify_batch_cpu(gpk.data(), gsig.data(), gmsg.data(), off.data(), len.data(),
                                                          pps.size(), ppv.data(), threads)))
      return rc;
  }
  const bool clamp = ck->protocol_version >= 10;
  for (size_t t = 0; t < n_bodies; ++t) {
    sv_txcheck_body b;
    b.hint = hint;
    b.sig = sig;
    b.sig_len = ck->sig_len;
    b.key = key;
    b.pair_sig = ps.data();
    b.pair_key = pk.data();
    b.pair_verdict = pv.data();
    b.digest = digests + 32 * t;
    b.s0 = sig_begin[t];
    b.ns = (uint32_t)(sig_begin[t + 1] - sig_begin[t]);
    b.k0 = key_begin[t];
    b.k1 = key_begin[t + 1];
    b.p0 = pb[t];
    b.p1 = pb[t + 1];
    b.ppair_sig = pps.data();
    b.ppair_key = ppk.data();
    b.ppair_verdict = ppv.data();
    b.q0 = qb ? qb[t] : 0;
    b.q1 = qb ? qb[t + 1] : 0;
    b.pp0 = ppb[t];
    b.pp1 = ppb[t + 1];
    for (uint64_t c = ck->check_begin[t]; c < ck->check_begin[t + 1]; ++c) {
      const uint64_t g0 = ck->signer_begin[c];
      const sv_txcheck_result r = sv_txcheck<true>(b, ck->signer_type + g0, ck->signer_weight + g0, ck->signer_key + g0,
                                             (uint32_t)(ck->signer_begin[c + 1] - g0), ck->check_needed[c], clamp);
      check_ok[c] = (uint8_t)r.ok;
      check_weight[c] = r.total;
      check_used[c] = r.used;
    }
  }
  return SV_OK;
}

// Argument check shared by the sv_ed25519_check_txbodies_accounts host-array
// entry points (declared in launch.h): SV_OK or SV_ERR_INVALID_ARG.  The
// account table is walked once per account; the per-body and per-check passes
// read two words per use.
int sv_txaccounts_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                        const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                        const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                        const sv_txaccounts* A, const uint8_t* check_ok, const uint32_t* check_weight,
                        const uint64_t* check_used, uint32_t* acnt) {
  if (!network_id || !sig_begin || !A || A->struct_size < sizeof(sv_txaccounts)) return SV_ERR_INVALID_ARG;
  if (n_bodies && (!body_off || !body_len || !body_kind)) return SV_ERR_INVALID_ARG;
  const size_t na = A->n_accounts, ns = A->n_asigners, np = A->n_apayloads, ne = A->n_bacct, nc = A->n_checks;
  if ((uint64_t)n_sigs >> 32 || (uint64_t)na >> 32 || (uint64_t)ns >> 32 || (uint64_t)np >> 32 ||
      (uint64_t)ne >> 32 || (uint64_t)nc >> 32)
    return SV_ERR_INVALID_ARG;
  if (n_sigs && (!hint || !sig)) return SV_ERR_INVALID_ARG;
  if (A->protocol_version == 7) return SV_ERR_INVALID_ARG;
  if (!A->asigner_begin || !A->bacct_begin || !A->check_begin) return SV_ERR_INVALID_ARG;
  if (na && (!A->acct_key || !A->acct_thresholds)) return SV_ERR_INVALID_ARG;
  if (ns && (!A->asigner_type || !A->asigner_weight || !A->asigner_key)) return SV_ERR_INVALID_ARG;
  if (np && (!A->apayload || !A->apayload_len)) return SV_ERR_INVALID_ARG;
  if (ne && !A->bacct) return SV_ERR_INVALID_ARG;
  if (nc && (!A->check_acct || !A->check_level || !check_ok || !check_weight || !check_used))
    return SV_ERR_INVALID_ARG;
  if (sig_begin[0] != 0 || sig_begin[n_bodies] != n_sigs) return SV_ERR_INVALID_ARG;
  if (A->asigner_begin[0] != 0 || A->asigner_begin[na] != ns) return SV_ERR_INVALID_ARG;
  if (A->bacct_begin[0] != 0 || A->bacct_begin[n_bodies] != ne) return SV_ERR_INVALID_ARG;
  if (A->check_begin[0] != 0 || A->check_begin[n_bodies] != nc) return SV_ERR_INVALID_ARG;
  // once per payload and per account: lengths, types, payload indices, the expanded list's length
  for (size_t i = 0; i < np; ++i)
    if (A->apayload_len[i] > 64) return SV_ERR_INVALID_ARG;
  std::vector<uint32_t> own;
  if (!acnt) {
    own.resize(2 * na + 2);
    acnt = own.data();
  }
  for (size_t a = 0; a < na; ++a) {
    const uint64_t s0 = A->asigner_begin[a], s1 = A->asigner_begin[a + 1];
    if (s1 < s0 || s1 > ns) return SV_ERR_INVALID_ARG;
    uint32_t nk = A->acct_thresholds[4 * a] ? 1u : 0u, nq = 0;
    if (nk + (s1 - s0) > SV_TXCHECK_MAX) return SV_ERR_INVALID_ARG;
    for (uint64_t s = s0; s < s1; ++s) {
      const uint8_t ty = A->asigner_type[s];
      if (ty > 3) return SV_ERR_INVALID_ARG;
      if (ty != 3) {
        ++nk;
        continue;
      }
      if (!A->asigner_payload || A->asigner_payload[s] >= np) return SV_ERR_INVALID_ARG;
      ++nq;
    }
    acnt[2 * a] = nk;
    acnt[2 * a + 1] = nq;
  }
  // per body: its CSR words, signature lengths, account entries and checks (linear in the uses: threaded over
  // bodies like sv_txchecks_check); sums: the expanded rows
  auto bodies_ok = [&](size_t t0, size_t t1, uint64_t* rows) {
    uint64_t nk = 0, nq = 0, ng = 0;
    for (size_t t = t0; t < t1; ++t) {
      if (sig_begin[t + 1] < sig_begin[t] || sig_begin[t + 1] > n_sigs || body_kind[t] > 2) return false;
      if (body_len[t] && !bodies) return false;
      if (A->sig_len)
        for (uint64_t i = sig_begin[t]; i < sig_begin[t + 1]; ++i)
          if (A->sig_len[i] > 64) return false;
      const uint64_t e0 = A->bacct_begin[t], e1 = A->bacct_begin[t + 1];
      if (e1 < e0 || e1 > ne) return false;
      for (uint64_t e = e0; e < e1; ++e) {
        const uint32_t a = A->bacct[e];
        if (a >= na) return false;
        nk += acnt[2 * a];
        nq += acnt[2 * a + 1];
      }
      const uint64_t c0 = A->check_begin[t], c1 = A->check_begin[t + 1];
      if (c1 < c0 || c1 > nc) return false;
      if (c1 > c0 && sig_begin[t + 1] - sig_begin[t] > SV_TXCHECK_MAX) return false;
      for (uint64_t c = c0; c < c1; ++c) {
        if (A->check_acct[c] >= e1 - e0 || A->check_level[c] > 3) return false;
        if (A->check_level[c] == 0 && !A->check_needed) return false;
        const uint32_t a = A->bacct[e0 + A->check_acct[c]];
        ng += acnt[2 * a] + acnt[2 * a + 1];
      }
    }
    rows[0] = nk;
    rows[1] = nq;
    rows[2] = ng;
    return true;
  };
  const size_t T = std::max<size_t>(1, std::min<size_t>({(size_t)8, n_bodies / 16384,
                                                         (size_t)std::max(1u, std::thread::hardware_concurrency())}));
  std::vector<uint64_t> rows(3 * T, 0);
  std::vector<uint8_t> good(T, 0);
  {
    std::vector<std::thread> th;
    for (size_t i = 1; i < T; ++i)
      th.emplace_back(
          [&, i] { good[i] = bodies_ok(n_bodies * i / T, n_bodies * (i + 1) / T, &rows[3 * i]) ? 1 : 0; });
    good[0] = bodies_ok(0, n_bodies / T, &rows[0]) ? 1 : 0;
    for (auto& x : th) x.join();
  }
  uint64_t tot[3] = {0, 0, 0};
  for (size_t i = 0; i < T; ++i) {
    if (!good[i]) return SV_ERR_INVALID_ARG;
    for (int j = 0; j < 3; ++j) tot[j] += rows[3 * i + j];
  }
  if (tot[0] >> 32 || tot[1] >> 32 || tot[2] >> 32) return SV_ERR_INVALID_ARG;
  return SV_OK;
}

int sv_ed25519_check_txbodies_accounts_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                           const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                           const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                           size_t n_sigs, const sv_txaccounts* A, uint8_t* check_ok,
                                           uint32_t* check_weight, uint64_t* check_used, uint8_t* digests,
                                           int threads) {
  int rc = sv_txaccounts_check(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, hint, sig,
                               n_sigs, A, check_ok, check_weight, check_used, nullptr);
  if (rc) return rc;
  if (n_bodies == 0) return SV_OK;
  // the expansion with the functions the device kernels run (txacct.h), in their order: per account, count + scan
  // per body and per check, rows, signers
  const sv_acct_tab T{A->acct_key,        A->acct_thresholds, A->asigner_begin, A->asigner_type,
                      A->asigner_weight,  A->asigner_key,     A->asigner_payload, A->apayload,
                      A->apayload_len,    A->n_accounts,      A->n_asigners,    A->n_apayloads};
  const sv_acct_use U{A->bacct_begin, A->bacct,     A->check_begin, A->check_acct, A->check_level,
                      A->check_needed, n_bodies,    A->n_bacct,     A->n_checks};
  const size_t nb = n_bodies, nc = A->n_checks;
  std::vector<uint32_t> acnt(2 * T.na + 2), rank(T.ns + 1), erow(2 * U.ne + 2);
  for (uint64_t a = 0; a < T.na; ++a) sv_acct_count(T, a, acnt.data(), rank.data());
  std::vector<uint64_t> kb(nb + 1), qb(nb + 1), gb(nc + 1);
  std::vector<int32_t> need(nc + 1);
  uint64_t nk = 0, nq = 0, ng = 0;
  for (size_t t = 0; t < nb; ++t) {
    uint32_t k, q;
    sv_acct_body_count(T, U, acnt.data(), t, &k, &q);
    kb[t] = nk;
    qb[t] = nq;
    nk += k;
    nq += q;
    for (uint64_t c = U.cbeg[t]; c < U.cbeg[t + 1]; ++c) {
      gb[c] = ng;
      ng += sv_acct_check_count(T, U, acnt.data(), t, c, &need[c]);
    }
  }
  kb[nb] = nk;
  qb[nb] = nq;
  gb[nc] = ng;
  std::vector<uint8_t> key(32 * nk + 32), qkey(32 * nq + 32), qpay(64 * nq + 64), qlen(nq + 1), gt(ng + 1);
  std::vector<uint32_t> gw(ng + 1), gk(ng + 1);
  const sv_acct_out O{kb.data(),   qb.data(),   gb.data(), need.data(), key.data(), qkey.data(), qpay.data(),
                      qlen.data(), gt.data(),   gw.data(), gk.data(),   nk,         nq,          ng};
  for (size_t t = 0; t < nb; ++t) {
    uint64_t e0, e1, krow = kb[t], qrow = qb[t];
    sv_acct_entries(U, t, &e0, &e1);
    for (uint64_t e = e0; e < e1; ++e) {
      erow[2 * e] = (uint32_t)krow;
      erow[2 * e + 1] = (uint32_t)qrow;
      const uint64_t a = U.eacct[e];
      if (a >= T.na) continue;
      const uint64_t n = (uint64_t)acnt[2 * a] + acnt[2 * a + 1];
      for (uint64_t j = 0; j < n; ++j) sv_acct_fill_row(T, rank.data(), a, j, krow, qrow, O);
      krow += acnt[2 * a];
      qrow += acnt[2 * a + 1];
    }
    for (uint64_t c = U.cbeg[t]; c < U.cbeg[t + 1]; ++c) {
      uint64_t e;
      const uint64_t a = sv_acct_check_account(T, U, t, c, &e);
      if (a >= T.na) continue;
      for (uint64_t j = 0; j < gb[c + 1] - gb[c]; ++j)
        sv_acct_fill_signer(T, rank.data(), a, j, erow[2 * e], erow[2 * e + 1], gb[c] + j, O);
    }
  }
  sv_txchecks_payload P{};
  P.checks.struct_size = sizeof(sv_txchecks_payload);
  P.checks.protocol_version = A->protocol_version;
  P.checks.sig_len = A->sig_len;
  P.checks.check_begin = A->check_begin;
  P.checks.check_needed = need.data();
  P.checks.signer_begin = gb.data();
  P.checks.signer_type = gt.data();
  P.checks.signer_weight = gw.data();
  P.checks.signer_key = gk.data();
  P.checks.n_checks = nc;
  P.checks.n_signers = ng;
  P.pkey_begin = qb.data();
  P.pkey = qkey.data();
  P.pkey_payload = qpay.data();
  P.pkey_len = qlen.data();
  P.n_pkeys = nq;
  return sv_ed25519_check_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, hint,
                                       sig, n_sigs, kb.data(), key.data(), nk, &P.checks, check_ok, check_weight,
                                       check_used, digests, threads);
}

// Argument check of the decide entry points' sv_txresults (declared in launch.h), the part that needs no table:
// SV_OK or SV_ERR_INVALID_ARG.
int sv_txresults_args(const sv_txresults* res) {
  if (!res || res->struct_size < sizeof(sv_txresults) || !res->body_code) return SV_ERR_INVALID_ARG;
  if (res->bad_cap && !res->bad_body) return SV_ERR_INVALID_ARG;
  return SV_OK;
}

// ... and its roles and flags, once the twin's argument check has vouched for n_checks and n_bodies.
int sv_txresults_check(const sv_txresults* res, size_t n_bodies, size_t n_checks) {
  if (res->check_role)
    for (size_t c = 0; c < n_checks; ++c)
      if (res->check_role[c] > SV_TXROLE_OP) return SV_ERR_INVALID_ARG;
  if (res->body_flags)
    for (size_t t = 0; t < n_bodies; ++t)
      if (res->body_flags[t] & ~(uint8_t)SV_TXBODY_SKIP_UNUSED) return SV_ERR_INVALID_ARG;
  return SV_OK;
}

// The bad list of a host form, from body_code after the last chunk: global indices, ascending; *n_bad is exact
// even where it exceeds bad_cap, and no entry at or past bad_cap is written.
void sv_txresults_bad_list(const sv_txresults* res, size_t n_bodies) {
  if (!res->bad_body && !res->n_bad) return;
  uint64_t n = 0;
  for (size_t t = 0; t < n_bodies; ++t) {
    if (res->body_code[t] == SV_TXRESULT_OK) continue;
    if (res->bad_body && n < res->bad_cap) res->bad_body[n] = (uint32_t)t;
    ++n;
  }
  if (res->n_bad) *res->n_bad = n;
}

// txresult.h over host arrays: body_code and body_fail of every body, then the bad list.
void sv_txresults_fold(const sv_txresults* res, const uint64_t* check_begin, const uint64_t* sig_begin,
                       const uint8_t* check_ok, const uint64_t* check_used, size_t n_bodies, size_t n_checks,
                       size_t n_sigs) {
  const sv_txresult_in I{check_begin, sig_begin, check_ok, check_used, res->check_role, res->body_flags,
                         n_bodies,    n_checks,  n_sigs};
  for (size_t t = 0; t < n_bodies; ++t) {
    uint32_t fail;
    res->body_code[t] = sv_txresult_body(I, t, &fail);
    if (res->body_fail) res->body_fail[t] = fail;
  }
  sv_txresults_bad_list(res, n_bodies);
}

namespace {
// The three check arrays of a decide call on the CPU path: the caller's where it asked for them, else the call's own.
struct DecideBufs {
  std::vector<uint8_t> ok;
  std::vector<uint32_t> weight;
  std::vector<uint64_t> used;
  uint8_t* pok;
  uint32_t* pweight;
  uint64_t* pused;
  DecideBufs(const sv_txresults* res, size_t nc) {
    if (!res->check_ok) ok.resize(nc + 1);
    if (!res->check_weight) weight.resize(nc + 1);
    if (!res->check_used) used.resize(nc + 1);
    pok = res->check_ok ? res->check_ok : ok.data();
    pweight = res->check_weight ? res->check_weight : weight.data();
    pused = res->check_used ? res->check_used : used.data();
  }
};
// (the twin's argument check only asks whether the three outputs are there)
const uint64_t g_present = 0;
}  // namespace

int sv_ed25519_decide_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                   const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                   const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                                   const uint64_t* key_begin, const uint8_t* key, size_t n_keys, const sv_txchecks* ck,
                                   const sv_txresults* res, uint8_t* digests, int threads) {
  int rc = sv_txresults_args(res);
  if (rc) return rc;
  if ((rc = sv_txchecks_check(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, hint, sig, n_sigs,
                              key_begin, key, n_keys, ck, (const uint8_t*)&g_present, (const uint32_t*)&g_present,
                              &g_present)))
    return rc;
  const size_t nc = ck->n_checks;
  if ((rc = sv_txresults_check(res, n_bodies, nc))) return rc;
  DecideBufs b(res, nc);
  if ((rc = sv_ed25519_check_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, hint,
                                          sig, n_sigs, key_begin, key, n_keys, ck, b.pok, b.pweight, b.pused, digests,
                                          threads)))
    return rc;
  sv_txresults_fold(res, ck->check_begin, sig_begin, b.pok, b.pused, n_bodies, nc, n_sigs);
  return SV_OK;
}

int sv_ed25519_decide_txbodies_accounts_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                            const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                            const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                            size_t n_sigs, const sv_txaccounts* A, const sv_txresults* res,
                                            uint8_t* digests, int threads) {
  int rc = sv_txresults_args(res);
  if (rc) return rc;
  if ((rc = sv_txaccounts_check(network_id, bodies, body_off, body_len, body_kind, n_bodies, sig_begin, hint, sig,
                                n_sigs, A, (const uint8_t*)&g_present, (const uint32_t*)&g_present, &g_present,
                                nullptr)))
    return rc;
  const size_t nc = A->n_checks;
  if ((rc = sv_txresults_check(res, n_bodies, nc))) return rc;
  DecideBufs b(res, nc);
  if ((rc = sv_ed25519_check_txbodies_accounts_cpu(network_id, bodies, body_off, body_len, body_kind, n_bodies,
                                                   sig_begin, hint, sig, n_sigs, A, b.pok, b.pweight, b.pused, digests,
                                                   threads)))
    return rc;
  sv_txresults_fold(res, A->check_begin, sig_begin, b.pok, b.pused, n_bodies, nc, n_sigs);
  return SV_OK;
}

// ---------------------------------------------------------------- the verdict audit
// The textbook verifier on the host: verify_core.h sv_verify_core over the radix-2^51 field, with the full-length
// ladder's own table of B (e B for e <= 2^15, as the device's table 0), built at first use on four threads.
int sv_audit_cpu_one(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t len) {
  static std::vector<sv_u4> btab;
  static std::once_flag once;
  std::call_once(once, [] {
    btab.assign((size_t)SV_BTAB_ENTRIES * SV_BTAB_QUADS, sv_u4{0, 0, 0, 0});
    const unsigned T = 4;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t)
      th.emplace_back([t] {
        for (int e = (int)t; e < SV_BTAB_ENTRIES; e += (int)T)
          sv_btab_entry((uint32_t*)&btab[(size_t)e * SV_BTAB_QUADS], e);
      });
    for (auto& x : th) x.join();
  });
  uint32_t A[8], S[8], hram[16];
  sv_u4 R[2];
  words(A, pk);
  std::memcpy(R, sig, 32);
  words(S, sig + 32);
  // sha512_ram_var reads whole aligned dwords (sha512_dev.h sv_msg_word), up to three bytes to either side of the
  // message: a caller's message may begin and end where its allocation does, so it is hashed from an aligned copy
  static thread_local std::vector<uint32_t> copy;
  if (copy.size() < (size_t)len / 4 + 1) copy.resize((size_t)len / 4 + 1);
  if (len) std::memcpy(copy.data(), msg, len);
  sha512_ram_var(hram, (const uint32_t*)R, A, (const uint8_t*)copy.data(), len);
  static thread_local std::vector<sv_u4> slot(SV_SLOT_QUADS_W);
  return sv_verify_core(A, R, S, hram, slot.data(), 1, btab.data()) ? 1 : 0;
}

int sv_audit_batch_cpu(const sv_audit_opts* o, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                       const uint64_t* msg_off, const uint32_t* msg_len, uint32_t fixed_msg_len, size_t n,
                       const uint8_t* claimed, sv_audit_stats* stats, sv_audit_record* rec, size_t cap, size_t* n_rec,
                       int threads) {
  if (!o || o->struct_size < sizeof(sv_audit_opts)) return SV_ERR_INVALID_ARG;
  if ((o->what & ~(SV_AUDIT_REJECTS | SV_AUDIT_SAMPLE)) || ((o->what & SV_AUDIT_SAMPLE) && o->one_in == 0) ||
      o->budget > SV_AUDIT_BUDGET_MAX)
    return SV_ERR_INVALID_ARG;
  if (stats && stats->struct_size < offsetof(sv_audit_stats, what)) return SV_ERR_INVALID_ARG;
  if (cap && !rec) return SV_ERR_INVALID_ARG;
  sv_audit_stats s{};
  s.what = o->what;
  s.seq = o->seq;
  auto done = [&] {
    if (n_rec) *n_rec = (size_t)s.records_held;
    if (stats) {
      s.struct_size = stats->struct_size;
      std::memcpy(stats, &s, std::min<size_t>((size_t)stats->struct_size, sizeof(s)));
    }
    return SV_OK;
  };
  if (n == 0) return done();
  if (!pk || !sig || !claimed || n > SV_AUDIT_MAX_ROWS) return SV_ERR_INVALID_ARG;
  if (fixed_msg_len ? !msg : (!msg_off || !msg_len)) return SV_ERR_INVALID_ARG;
  if (!fixed_msg_len && !msg)
    for (size_t i = 0; i < n; ++i)
      if (msg_len[i]) return SV_ERR_INVALID_ARG;
  // the pick, in row order, clipped to the budget
  const uint64_t budget = sv_audit_budget(o->budget);
  std::vector<uint32_t> list;
  uint64_t picks = 0;
  for (size_t i = 0; i < n; ++i)
    if (sv_audit_pick(o->what, o->one_in, o->seed, o->seq, i, claimed[i])) {
      if (picks < budget) list.push_back((uint32_t)i);
      ++picks;
    }
  const size_t m = list.size();
  auto mptr = [&](size_t i) { return !msg ? nullptr : fixed_msg_len ? msg + (size_t)fixed_msg_len * i : msg + msg_off[i]; };
  auto mlen = [&](size_t i) { return fixed_msg_len ? fixed_msg_len : msg_len[i]; };
  std::vector<uint8_t> av(m);
  sign_threads(m, threads, 8, [&](size_t a, size_t b) {
    for (size_t j = a; j < b; ++j) {
      const size_t i = list[j];
      av[j] = (uint8_t)sv_audit_cpu_one(pk + 32 * i, sig + 64 * i, mptr(i), mlen(i));
    }
  });
  // the report, in row order
  const size_t room = std::min<size_t>(cap, SV_AUDIT_RING);
  uint64_t mismatches = 0;
  for (size_t j = 0; j < m; ++j) {
    const size_t i = list[j];
    s.audited_rejects += claimed[i] == 0 ? 1 : 0;
    if (claimed[i] == av[j]) continue;
    const uint32_t at = sv_audit_ring_slot(SV_AUDIT_RING - room, mismatches);
    if (at < SV_AUDIT_RING)
      sv_audit_record_fill(&rec[at - (SV_AUDIT_RING - room)], o->seq, i, claimed[i], av[j], av[j], pk + 32 * i,
                           sig + 64 * i, mptr(i), mlen(i));
    ++mismatches;
  }
  s.audited = m;
  s.over_budget = picks - m;
  s.mismatches = mismatches;
  s.records_held = std::min<uint64_t>(mismatches, room);
  s.records_lost = mismatches - s.records_held;
  return done();
}

int sv_ed25519_verify_cpu(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_len) {
  if (!pk || !sig || (!msg && msg_len) || msg_len > 0xffffffffu) return SV_ERR_INVALID_ARG;
  std::call_once(g_once, build_tables);
  static thread_local std::vector<sv_u4> slot(SV_SLOT_QUADS_L);
  return verify_one(pk, sig, msg, (uint32_t)msg_len, slot.data()) ? 1 : 0;
}

}  // extern "C"
