// What the kernels read from a host batch, and how it gets there: the batch
// forms (HostIn, TxIn), the layout of their pinned images (Image, TxChunk),
// the packers that fill an image on the pack pool, and the planners that cut
// a batch into staging chunks and key pieces.  Pure host code, no HIP:
// included by the engine (sv_api.cpp, through bulk.h and latlane.h) and by the
// CPU tests (tests/native/host_core.cpp, tests/test_host_staging.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "host_env.h"
#include "pool.h"

namespace sv {
namespace {

inline Pool& pool() {
  // The GPU box's share is 16 CPUs; the staging copies saturate well below.
  static Pool p((unsigned)std::min<size_t>(
      env_size("SV_HOST_THREADS", std::min(8u, std::max(2u, std::thread::hardware_concurrency()))), 64));
  return p;
}
// The pool a pack runs on: a device slot's own workers inside a multi-slot
// call (shard), else the shared pool.
inline thread_local Pool* t_pack_pool = nullptr;
inline thread_local size_t t_pack_parts = 0;  // (multi-slot calls: this slot's share of the CPUs; 0: no cap)
inline Pool& pack_pool() { return t_pack_pool ? *t_pack_pool : pool(); }

inline size_t stage_chunk() {
  static const size_t c = std::max<size_t>(1024, env_size("SV_STAGE_CHUNK", (size_t)1 << 18));
  return c;
}
// Pipeline fill: the first R chunks of a multi-chunk batch grow geometrically
// (chunk / 2^R, ..., chunk / 2), so the first kernel starts after packing and
// copying a small chunk instead of a whole one.  SV_STAGE_RAMP = R (default
// 2: chunk/4 then chunk/2; 0: equal chunks).
inline size_t stage_ramp_steps() {
  static const size_t r = std::min<size_t>(env_size("SV_STAGE_RAMP", 2), 8);
  return r;
}
inline bool stage_ramp() { return stage_ramp_steps() != 0; }
inline size_t chunk_len(size_t c, size_t chunk, size_t left) {
  size_t m = chunk;
  const size_t r = stage_ramp_steps();
  if (c < r) m = std::max<size_t>(1024, chunk >> (r - c));
  return std::min(m, left);
}

// A batch in host memory: contiguous SoA arrays (pk n x 32, sig n x 64,
// messages by offset/length or fixed stride), or pointer arrays (gather).
struct HostIn {
  const uint8_t* pk = nullptr;
  const uint8_t* sig = nullptr;
  const uint8_t* msg = nullptr;
  const uint64_t* off = nullptr;
  const uint32_t* len = nullptr;
  uint32_t fixed = 0;  // != 0: message i = msg + i * fixed, or msg + off[i] when off is set (uniform lengths)
  const uint8_t* const* ppk = nullptr;  // gather form (ppk != nullptr)
  const uint8_t* const* psig = nullptr;
  const uint8_t* const* pmsg = nullptr;

  static HostIn soa(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* off,
                    const uint32_t* len) {
    HostIn in;
    in.pk = pk;
    in.sig = sig;
    in.msg = msg;
    in.off = off;
    in.len = len;
    return in;
  }
  static HostIn fixed_len(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t len) {
    HostIn in = soa(pk, sig, msg, nullptr, nullptr);
    in.fixed = len;
    return in;
  }
  static HostIn gathered(const uint8_t* const* pk, const uint8_t* const* sig, const uint8_t* const* msg,
                         const uint32_t* len) {
    HostIn in;
    in.ppk = pk;
    in.psig = sig;
    in.pmsg = msg;
    in.len = len;
    return in;
  }

  bool gather() const { return ppk != nullptr; }
  uint32_t mlen(size_t i) const { return fixed ? fixed : len[i]; }
  const uint8_t* pkp(size_t i) const { return gather() ? ppk[i] : pk + 32 * i; }
  const uint8_t* sigp(size_t i) const { return gather() ? psig[i] : sig + 64 * i; }
  const uint8_t* msgp(size_t i) const {
    if (gather()) return pmsg[i];
    return off ? msg + off[i] : msg + i * (size_t)fixed;
  }
  // the slice [lo, ...) as a batch of its own
  HostIn sub(size_t lo) const {
    HostIn s = *this;
    if (gather()) {
      s.ppk += lo;
      s.psig += lo;
      s.pmsg += lo;
      s.len += lo;
    } else {
      s.pk += 32 * lo;
      s.sig += 64 * lo;
      if (off) {
        s.off += lo;
        if (len) s.len += lo;
      } else {
        s.msg += lo * (size_t)fixed;
      }
    }
    return s;
  }
};

// Pinned image of m signatures starting at `lo`:
//   pk (32 m) | sig (64 m) | fixed: msgs (m L)   or   var: off (8 m) | len (4 m) | packed msgs
// (pk, sig and a fixed-length message block stay 16-byte aligned).
struct Image {
  size_t o_sig, o_off, o_len, o_msg, bytes;
  bool var;
};

inline Image image_of(const HostIn& in, size_t lo, size_t m, size_t* msg_total) {
  Image im;
  im.var = in.fixed == 0;
  size_t total = 0;
  if (!im.var) total = m * (size_t)in.fixed;
  else
    for (size_t i = 0; i < m; ++i) total += in.len[lo + i];
  im.o_sig = 32 * m;
  im.o_off = 96 * m;
  im.o_len = im.o_off + 8 * m;
  im.o_msg = im.var ? im.o_len + 4 * m : im.o_off;
  im.bytes = im.o_msg + std::max<size_t>(total, 1);
  *msg_total = total;
  return im;
}

// sv_launch_verify's message mode of an image: 0 32-byte messages at stride 32
// (read with 16-byte loads: `aligned`), 1 by offset and length, 2 fixed stride.
inline int verify_mode(bool var, uint32_t fixed, bool aligned = true) {
  return var ? 1 : (fixed == 32 && aligned ? 0 : 2);
}

// Packing [lo, lo + m) into h (layout `im`): the message offsets first, then
// rows [r0, r1) of the chunk, in parallel for large ranges.
// (rows [r0, r1), the first at message offset pos; returns the offset past r1)
inline uint64_t pack_offsets(const HostIn& in, size_t lo, size_t r0, size_t r1, uint64_t pos, const Image& im,
                             uint8_t* h) {
  uint64_t* offs = (uint64_t*)(h + im.o_off);
  if (im.var) {
    for (size_t i = r0; i < r1; ++i) {
      offs[i] = pos;
      pos += in.len[lo + i];
    }
  }
  return pos;
}
// kPart: bytes per helper task, pack_part() or 1 MB when 0 (a keyed batch's pieces take
// smaller ones: the first verify launch waits for the last piece)
inline void pack_rows(const HostIn& in, size_t lo, size_t r0, size_t r1, const Image& im, uint8_t* h,
                      size_t kPart = 0) {
  const uint64_t* offs = (const uint64_t*)(h + im.o_off);
  const size_t m = r1 - r0;
  const size_t est = im.bytes / std::max<size_t>(1, (im.o_sig / 32)) * m;  // (bytes of these rows, roughly)
  if (kPart == 0) kPart = est >= (2u << 20) ? pack_part() : (1u << 20);
  Pool& pp = pack_pool();
  const size_t parts = pack_parts(pp.size(), t_pack_parts, est, kPart);
  pp.run(parts, [&](size_t t) {
    const size_t a = r0 + m * t / parts, b = r0 + m * (t + 1) / parts;
    if (a == b) return;
    const PackCopy cp;
    if (!in.gather()) {
      cp(h + 32 * a, in.pk + 32 * (lo + a), 32 * (b - a));
      cp(h + im.o_sig + 64 * a, in.sig + 64 * (lo + a), 64 * (b - a));
      if (!im.var && !in.off) {
        cp(h + im.o_msg + a * (size_t)in.fixed, in.msg + (lo + a) * (size_t)in.fixed, (b - a) * (size_t)in.fixed);
        return;
      }
      if (!im.var) {  // (uniform lengths, found by offset: packed at the fixed stride)
        for (size_t i = a; i < b; ++i) cp(h + im.o_msg + i * (size_t)in.fixed, in.msg + in.off[lo + i], in.fixed);
        return;
      }
    } else {
      for (size_t i = a; i < b; ++i) {
        cp(h + 32 * i, in.ppk[lo + i], 32);
        cp(h + im.o_sig + 64 * i, in.psig[lo + i], 64);
      }
      if (!im.var) {
        for (size_t i = a; i < b; ++i) cp(h + im.o_msg + i * (size_t)in.fixed, in.pmsg[lo + i], in.fixed);
        return;
      }
    }
    std::memcpy(h + im.o_len + 4 * a, in.len + lo + a, 4 * (b - a));
    for (size_t i = a; i < b; ++i) {
      const uint32_t l = in.len[lo + i];
      if (l) std::memcpy(h + im.o_msg + offs[i], in.msgp(lo + i), l);
    }
  });
}
inline void pack(const HostIn& in, size_t lo, size_t m, const Image& im, uint8_t* h) {
  pack_offsets(in, lo, 0, m, 0, im, h);
  pack_rows(in, lo, 0, m, im, h);
}
// A one-chunk keyed batch of at least kKeyPieceMin rows sends its keys up in
// pieces (key_pieces): the caller's cache walk starts on the first piece while
// later ones are packed, copied and hashed.  The first piece is kKeyPieceFirst
// rows, so the walk starts as early as it can; each later piece is twice the
// one before, at most kKeyPieceMax rows (a piece costs ~10 HIP calls on this
// thread: fewer pieces bring the last one, and the verify launch behind it,
// forward).
constexpr size_t kKeyPieceMin = 8192, kKeyPieceFirst = 2048, kKeyPieceMax = 1 << 15;
// Row bounds of the pieces of an m-row batch: b[0] = 0 < b[1] < ... < b[P] = m.
inline std::vector<size_t> key_pieces(size_t m) {
  if (m < kKeyPieceMin) return {0, m};
  std::vector<size_t> b{0};
  for (size_t len = kKeyPieceFirst; b.back() < m; len = std::min(2 * len, kKeyPieceMax))
    b.push_back(m - b.back() < len + len / 2 ? m : b.back() + len);  // (no runt last piece)
  return b;
}

// Do the keys of a host batch repeat?  A sample of up to 4096 evenly spaced
// rows: with s sampled of n and d repeats among them, K distinct keys give
// d ~ s^2 / 2K, so K <= n / 2 (each key signs twice on average) reads as
// d * n >= s^2 (exact when s = n: n - d <= n / 2).
inline bool repeated_keys(const HostIn& in, size_t n) {
  const size_t s = std::min<size_t>(n, 4096);
  if (s < 2) return false;
  constexpr size_t kSet = 8192;
  std::vector<const uint8_t*> set(kSet, nullptr);
  size_t d = 0;
  for (size_t k = 0; k < s; ++k) {
    const uint8_t* pk = in.pkp(k * n / s);
    uint64_t h;
    std::memcpy(&h, pk, 8);
    h *= 0x9E3779B97F4A7C15ull;
    for (size_t j = (size_t)(h >> 51) & (kSet - 1);; j = (j + 1) & (kSet - 1)) {
      if (!set[j]) {
        set[j] = pk;
        break;
      }
      if (std::memcmp(set[j], pk, 32) == 0) {
        ++d;
        break;
      }
    }
  }
  return s == n ? 2 * (n - d) <= n : (uint64_t)d * n >= (uint64_t)s * s;
}

// A variable-length batch whose messages all have one length L > 0 (tx
// contents hashes: every pair of a tx-set pre-pass) goes to the device as a
// fixed-length batch: messages packed at stride L (found by their offsets
// or pointers), no offset / length arrays in the image, and the kernels' fixed
// modes instead of an offset read before each message (measured: 50-110 us per
// call at 29k-50k signatures, tools/varlen_probe.py).  The scan stops at the
// first other length.
inline HostIn uniform_form(const HostIn& in, size_t n) {
  HostIn u = in;
  if (in.fixed || n == 0 || !in.len) return u;
  const uint32_t L = in.len[0];
  if (L == 0) return u;
  for (size_t i = 1; i < n; ++i)
    if (in.len[i] != L) return u;
  u.fixed = L;
  return u;
}

// sv_ed25519_verify_txbodies: a batch of bodies and their signatures (CSR).
struct TxIn {
  const uint8_t* nid;
  const uint8_t* bodies;
  const uint64_t* off;
  const uint32_t* len;
  const uint8_t* kind;
  size_t nb;
  const uint64_t* sb;
  const uint8_t* pk;
  const uint8_t* sig;
};

// Body bytes per staging chunk (SV_TXBODY_CHUNK_BYTES, default 64 MiB).
inline size_t txbody_chunk_bytes() {
  static const size_t b = std::max<size_t>(4096, env_size("SV_TXBODY_CHUNK_BYTES", (size_t)64 << 20));
  return b;
}
inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// One staging chunk: bodies [b0, b1) and the signatures [s0, s1) of the slice
// they own.  Pinned / device image:
//   pk (32 m) | sig (64 m) | body_off (8 k) | sig_begin (8 (k + 1)) | body_len (4 k) | kind (k) | bodies
// with every body 16-byte aligned (offsets relative to the body section) and
// sig_begin relative to s0.
struct TxChunk {
  size_t b0, b1, s0, s1;
  size_t body_bytes;  // the aligned body section
  size_t o_sig, o_off, o_sb, o_len, o_kind, o_body, bytes;
};

// The chunks of a slice: bodies [B0, B1), signatures [lo, hi) (a body's range
// clipped to the slice).  A chunk is a run of whole bodies of at most max_s
// signatures and max_b body bytes; a body over either bound is a chunk alone.
inline std::vector<TxChunk> tx_plan(const TxIn& in, size_t B0, size_t B1, size_t lo, size_t hi, size_t max_s,
                                    size_t max_b) {
  auto cb = [&](size_t t) { return (size_t)std::min<uint64_t>(std::max<uint64_t>(in.sb[t], lo), hi); };
  std::vector<TxChunk> out;
  size_t t = B0;
  while (t < B1) {
    TxChunk c{};
    c.b0 = t;
    c.s0 = cb(t);
    size_t bytes = 0;
    do {
      bytes += al16(in.len[t]);
      ++t;
    } while (t < B1 && cb(t + 1) - c.s0 <= max_s && bytes + al16(in.len[t]) <= max_b);
    c.b1 = t;
    c.s1 = cb(t);
    c.body_bytes = bytes;
    const size_t m = c.s1 - c.s0, k = c.b1 - c.b0;
    c.o_sig = 32 * m;
    c.o_off = 96 * m;
    c.o_sb = c.o_off + 8 * k;
    c.o_len = c.o_sb + 8 * (k + 1);
    c.o_kind = c.o_len + 4 * k;
    c.o_body = al16(c.o_kind + k);
    c.bytes = c.o_body + std::max<size_t>(bytes, 16);
    out.push_back(c);
  }
  return out;
}

inline void tx_pack(const TxIn& in, const TxChunk& c, size_t lo, size_t hi, uint8_t* h) {
  const size_t m = c.s1 - c.s0, k = c.b1 - c.b0;
  uint64_t* offs = (uint64_t*)(h + c.o_off);
  uint64_t* sb = (uint64_t*)(h + c.o_sb);
  size_t pos = 0;
  for (size_t i = 0; i < k; ++i) {
    offs[i] = pos;
    pos += al16(in.len[c.b0 + i]);
  }
  for (size_t i = 0; i <= k; ++i)
    sb[i] = std::min<uint64_t>(std::max<uint64_t>(in.sb[c.b0 + i], lo), hi) - c.s0;
  std::memcpy(h + c.o_len, in.len + c.b0, 4 * k);
  std::memcpy(h + c.o_kind, in.kind + c.b0, k);
  Pool& pp = pack_pool();
  const size_t parts = pack_parts(pp.size(), t_pack_parts, 96 * m + c.body_bytes, pack_part());
  pp.run(parts, [&](size_t p) {
    const PackCopy cp;
    const size_t a = m * p / parts, b = m * (p + 1) / parts;
    if (b > a) {
      cp(h + 32 * a, in.pk + 32 * (c.s0 + a), 32 * (b - a));
      cp(h + c.o_sig + 64 * a, in.sig + 64 * (c.s0 + a), 64 * (b - a));
    }
    for (size_t i = k * p / parts; i < k * (p + 1) / parts; ++i) {
      const uint32_t l = in.len[c.b0 + i];
      if (l) cp(h + c.o_body + offs[i], in.bodies + in.off[c.b0 + i], l);
    }
  });
}

// sv_ed25519_verify_txbodies_hinted: bodies, their decorated signatures (hint
// + signature) and their candidate keys, both in CSR form.
struct HintIn {
  const uint8_t* nid;
  const uint8_t* bodies;
  const uint64_t* off;
  const uint32_t* len;
  const uint8_t* kind;
  size_t nb;
  const uint64_t* sb;  // signatures of body t: [sb[t], sb[t + 1])
  const uint8_t* hint;
  const uint8_t* sig;
  const uint64_t* kb;  // keys of body t: [kb[t], kb[t + 1])
  const uint8_t* key;
};

// One staging chunk of it: bodies [b0, b1) with all their signatures [s0, s1)
// and keys [k0, k1).  Pinned / device image (k bodies, m signatures, q keys):
//   key (32 q) | sig (64 m) | hint (4 m) | body_off (8 k) | sig_begin (8 (k + 1)) | key_begin (8 (k + 1)) |
//   body_len (4 k) | kind (k) | bodies
// key, sig, hint, the CSR block and the body section start 16-byte aligned,
// every body too (offsets relative to the body section); sig_begin and
// key_begin are relative to s0 / k0.
struct PairChunk {
  size_t b0, b1, s0, s1, k0, k1;
  size_t body_bytes;
  size_t o_sig, o_hint, o_off, o_sb, o_kb, o_len, o_kind, o_body, bytes;
};

// The chunks of bodies [B0, B1): runs of whole bodies of at most max_s
// signatures, max_k keys and max_b body bytes; a body over a bound is a chunk
// alone.
inline std::vector<PairChunk> pair_plan(const HintIn& in, size_t B0, size_t B1, size_t max_s, size_t max_k,
                                        size_t max_b) {
  std::vector<PairChunk> out;
  size_t t = B0;
  while (t < B1) {
    PairChunk c{};
    c.b0 = t;
    c.s0 = (size_t)in.sb[t];
    c.k0 = (size_t)in.kb[t];
    size_t bytes = 0;
    do {
      bytes += al16(in.len[t]);
      ++t;
    } while (t < B1 && in.sb[t + 1] - c.s0 <= max_s && in.kb[t + 1] - c.k0 <= max_k &&
             bytes + al16(in.len[t]) <= max_b);
    c.b1 = t;
    c.s1 = (size_t)in.sb[t];
    c.k1 = (size_t)in.kb[t];
    c.body_bytes = bytes;
    const size_t m = c.s1 - c.s0, q = c.k1 - c.k0, k = c.b1 - c.b0;
    c.o_sig = 32 * q;
    c.o_hint = c.o_sig + 64 * m;
    c.o_off = al16(c.o_hint + 4 * m);
    c.o_sb = c.o_off + 8 * k;
    c.o_kb = c.o_sb + 8 * (k + 1);
    c.o_len = c.o_kb + 8 * (k + 1);
    c.o_kind = c.o_len + 4 * k;
    c.o_body = al16(c.o_kind + k);
    c.bytes = c.o_body + std::max<size_t>(bytes, 16);
    out.push_back(c);
  }
  return out;
}

inline void pair_pack(const HintIn& in, const PairChunk& c, uint8_t* h) {
  const size_t m = c.s1 - c.s0, q = c.k1 - c.k0, k = c.b1 - c.b0;
  uint64_t* offs = (uint64_t*)(h + c.o_off);
  uint64_t* sb = (uint64_t*)(h + c.o_sb);
  uint64_t* kb = (uint64_t*)(h + c.o_kb);
  size_t pos = 0;
  for (size_t i = 0; i < k; ++i) {
    offs[i] = pos;
    pos += al16(in.len[c.b0 + i]);
  }
  for (size_t i = 0; i <= k; ++i) {
    sb[i] = in.sb[c.b0 + i] - c.s0;
    kb[i] = in.kb ? in.kb[c.b0 + i] - c.k0 : 0;  // (no key CSR array: a by-account chunk, its keys made on the device)
  }
  std::memcpy(h + c.o_len, in.len + c.b0, 4 * k);
  std::memcpy(h + c.o_kind, in.kind + c.b0, k);
  Pool& pp = pack_pool();
  const size_t parts = pack_parts(pp.size(), t_pack_parts, 32 * q + 68 * m + c.body_bytes, pack_part());
  pp.run(parts, [&](size_t p) {
    const PackCopy cp;
    size_t a = q * p / parts, b = q * (p + 1) / parts;
    if (b > a) cp(h + 32 * a, in.key + 32 * (c.k0 + a), 32 * (b - a));
    a = m * p / parts, b = m * (p + 1) / parts;
    if (b > a) {
      cp(h + c.o_sig + 64 * a, in.sig + 64 * (c.s0 + a), 64 * (b - a));
      std::memcpy(h + c.o_hint + 4 * a, in.hint + 4 * (c.s0 + a), 4 * (b - a));
    }
    for (size_t i = k * p / parts; i < k * (p + 1) / parts; ++i) {
      const uint32_t l = in.len[c.b0 + i];
      if (l) cp(h + c.o_body + offs[i], in.bodies + in.off[c.b0 + i], l);
    }
  });
}

// sv_ed25519_check_txbodies: the hinted inputs plus each body's checks (signer
// lists with weights, and the needed weight), all in CSR form.
struct CheckIn {
  HintIn h;
  const uint8_t* sig_len;   // per signature, or nullptr: all 64
  const uint64_t* cb;       // checks of body t: [cb[t], cb[t + 1])
  const int32_t* need;      // per check
  const uint64_t* gb;       // signers of check c: [gb[c], gb[c + 1])
  const uint8_t* gtype;     // per signer
  const uint32_t* gweight;
  const uint32_t* gkey;     // global index into h.key (a type-3 signer with payload tables: into qkey)
  // the payload tables (sv_txchecks::pkey_begin ...), or qb == nullptr: none, or no candidate in the call
  const uint64_t* qb = nullptr;   // payload candidates of body t: [qb[t], qb[t + 1])
  const uint8_t* qkey = nullptr;  // 32 B rows
  const uint8_t* qpay = nullptr;  // 64 B rows
  const uint8_t* qlen = nullptr;  // per candidate
};

// One staging chunk of it: the hinted image of bodies [b0, b1) (PairChunk p,
// bytes [0, p.bytes)) followed, 16-byte aligned, by the chunk's check tables
// (nc checks [c0, c1), ng signers [g0, g1), m signatures):
//   check_begin (8 (k + 1)) | signer_begin (8 (nc + 1)) | needed (4 nc) | signer_weight (4 ng) |
//   signer_key (4 ng) | signer_type (ng) | sig_len (m, only with CheckIn::sig_len)
// check_begin, signer_begin and signer_key are relative to c0 / g0 / p.k0.
// With payload tables the type-3 signers' signer_key is relative to the chunk's
// first payload candidate instead.
struct CheckChunk {
  PairChunk p;
  size_t c0, c1, g0, g1;
  size_t o_cb, o_gb, o_need, o_gw, o_gk, o_gt, o_sl, bytes;
};

// A chunk whose bodies have payload candidates [q0, q1) (nq of them) carries
// them behind the CheckChunk image, at its `bytes`:
//   pkey (32 nq) | payload (64 nq) | pkey_begin (8 (k + 1)) | pkey_len (nq)
// with pkey_begin relative to q0; `bytes` is then the whole image.  A chunk
// without candidates has no such section: bytes == the CheckChunk's.
struct PayloadChunk {
  size_t q0, q1, o_qk, o_qp, o_qb, o_ql, bytes;
};
inline PayloadChunk payload_chunk(const CheckIn& in, const CheckChunk& c) {
  PayloadChunk pc{};
  pc.bytes = c.bytes;
  if (!in.qb) return pc;
  pc.q0 = (size_t)in.qb[c.p.b0];
  pc.q1 = (size_t)in.qb[c.p.b1];
  if (const size_t nq = pc.q1 - pc.q0) {
    pc.o_qk = c.bytes;
    pc.o_qp = pc.o_qk + 32 * nq;
    pc.o_qb = pc.o_qp + 64 * nq;
    pc.o_ql = pc.o_qb + 8 * (c.p.b1 - c.p.b0 + 1);
    pc.bytes = al16(pc.o_ql + nq);
  }
  return pc;
}
// (a few rows at most: copied by the caller's thread)
inline void payload_pack(const CheckIn& in, const CheckChunk& c, const PayloadChunk& pc, uint8_t* h) {
  const size_t nq = pc.q1 - pc.q0, k = c.p.b1 - c.p.b0;
  if (!nq) return;
  std::memcpy(h + pc.o_qk, in.qkey + 32 * pc.q0, 32 * nq);
  std::memcpy(h + pc.o_qp, in.qpay + 64 * pc.q0, 64 * nq);
  std::memcpy(h + pc.o_ql, in.qlen + pc.q0, nq);
  uint64_t* qb = (uint64_t*)(h + pc.o_qb);
  for (size_t i = 0; i <= k; ++i) qb[i] = in.qb[c.p.b0 + i] - pc.q0;
  std::memset(h + pc.o_ql + nq, 0, pc.bytes - (pc.o_ql + nq));
}

// The hinted image of exactly bodies [b0, b1): pair_plan's layout for a given run.
inline PairChunk pair_chunk(const HintIn& in, size_t b0, size_t b1, size_t body_bytes) {
  PairChunk c{};
  c.b0 = b0;
  c.b1 = b1;
  c.s0 = (size_t)in.sb[b0];
  c.s1 = (size_t)in.sb[b1];
  c.k0 = in.kb ? (size_t)in.kb[b0] : 0;
  c.k1 = in.kb ? (size_t)in.kb[b1] : 0;
  c.body_bytes = body_bytes;
  const size_t m = c.s1 - c.s0, q = c.k1 - c.k0, k = b1 - b0;
  c.o_sig = 32 * q;
  c.o_hint = c.o_sig + 64 * m;
  c.o_off = al16(c.o_hint + 4 * m);
  c.o_sb = c.o_off + 8 * k;
  c.o_kb = c.o_sb + 8 * (k + 1);
  c.o_len = c.o_kb + 8 * (k + 1);
  c.o_kind = c.o_len + 4 * k;
  c.o_body = al16(c.o_kind + k);
  c.bytes = c.o_body + std::max<size_t>(body_bytes, 16);
  return c;
}

// The chunks of bodies [B0, B1): pair_plan's runs of whole bodies, additionally
// bounded by max_c checks and max_g signers (a body over a bound is a chunk
// alone).  Payload candidates count towards max_k like keys.
inline std::vector<CheckChunk> check_plan(const CheckIn& in, size_t B0, size_t B1, size_t max_s, size_t max_k,
                                          size_t max_b, size_t max_c, size_t max_g) {
  std::vector<CheckChunk> out;
  const HintIn& hi = in.h;
  size_t t = B0;
  while (t < B1) {
    const size_t b0 = t, s0 = (size_t)hi.sb[t], k0 = (size_t)hi.kb[t], c0 = (size_t)in.cb[t], g0 = (size_t)in.gb[c0];
    const size_t q0 = in.qb ? (size_t)in.qb[t] : 0;
    size_t bytes = 0;
    do {
      bytes += al16(hi.len[t]);
      ++t;
    } while (t < B1 && hi.sb[t + 1] - s0 <= max_s &&
             hi.kb[t + 1] - k0 + (in.qb ? in.qb[t + 1] - q0 : 0) <= max_k && in.cb[t + 1] - c0 <= max_c &&
             in.gb[in.cb[t + 1]] - g0 <= max_g && bytes + al16(hi.len[t]) <= max_b);
    CheckChunk c{};
    c.p = pair_chunk(hi, b0, t, bytes);
    c.c0 = c0;
    c.c1 = (size_t)in.cb[t];
    c.g0 = g0;
    c.g1 = (size_t)in.gb[c.c1];
    const size_t k = t - b0, nc = c.c1 - c.c0, ng = c.g1 - c.g0, m = c.p.s1 - c.p.s0;
    c.o_cb = al16(c.p.bytes);
    c.o_gb = c.o_cb + 8 * (k + 1);
    c.o_need = c.o_gb + 8 * (nc + 1);
    c.o_gw = c.o_need + 4 * nc;
    c.o_gk = c.o_gw + 4 * ng;
    c.o_gt = c.o_gk + 4 * ng;
    c.o_sl = c.o_gt + ng;
    c.bytes = al16(c.o_sl + (in.sig_len ? m : 0) + 1);
    out.push_back(c);
  }
  return out;
}

inline void check_pack(const CheckIn& in, const CheckChunk& c, uint8_t* h) {
  pair_pack(in.h, c.p, h);
  const size_t k = c.p.b1 - c.p.b0, nc = c.c1 - c.c0, ng = c.g1 - c.g0, m = c.p.s1 - c.p.s0;
  uint64_t* cb = (uint64_t*)(h + c.o_cb);
  uint64_t* gb = (uint64_t*)(h + c.o_gb);
  uint32_t* gk = (uint32_t*)(h + c.o_gk);
  cb[k] = in.cb[c.p.b1] - c.c0;
  gb[nc] = in.gb[c.c1] - c.g0;
  const size_t q0 = in.qb ? (size_t)in.qb[c.p.b0] : 0;
  // the tables in parts of the pack pool: rebased CSR words and key indices, plain copies of the rest
  Pool& pp = pack_pool();
  const size_t parts = pack_parts(pp.size(), t_pack_parts, 8 * k + 12 * nc + 9 * ng + m, pack_part());
  pp.run(parts, [&](size_t p) {
    for (size_t i = k * p / parts; i < k * (p + 1) / parts; ++i) cb[i] = in.cb[c.p.b0 + i] - c.c0;
    size_t a = nc * p / parts, b = nc * (p + 1) / parts;
    for (size_t i = a; i < b; ++i) gb[i] = in.gb[c.c0 + i] - c.g0;
    if (b > a) std::memcpy(h + c.o_need + 4 * a, in.need + c.c0 + a, 4 * (b - a));
    a = ng * p / parts, b = ng * (p + 1) / parts;
    if (b > a) {
      std::memcpy(h + c.o_gw + 4 * a, in.gweight + c.g0 + a, 4 * (b - a));
      for (size_t i = a; i < b; ++i)
        gk[i] = in.gkey[c.g0 + i] -
                (uint32_t)(in.qb && in.gtype[c.g0 + i] == 3 /* ED25519_SIGNED_PAYLOAD */ ? q0 : c.p.k0);
      std::memcpy(h + c.o_gt + a, in.gtype + c.g0 + a, b - a);
    }
    a = m * p / parts, b = m * (p + 1) / parts;
    if (in.sig_len && b > a) std::memcpy(h + c.o_sl + a, in.sig_len + c.p.s0 + a, b - a);
  });
}

// sv_ed25519_check_txbodies_accounts: bodies and signatures as in the hinted
// call, the keys and signer lists derived on the device from an account table
// that goes up once (sv_txaccounts).  h.kb and h.key are null: a chunk's
// hinted image has no key section (pair_chunk, pair_pack).
struct AcctIn {
  HintIn h;
  const uint8_t* sig_len;  // per signature, or nullptr: all 64
  const uint64_t* eb;      // account entries of body t: [eb[t], eb[t + 1])
  const uint32_t* eacct;   // per entry
  const uint64_t* cb;      // checks of body t
  const uint32_t* cacct;   // per check: position inside the body's entries
  const uint8_t* clevel;
  const int32_t* cneed;    // may be null (no level-0 check)
  const uint32_t* acnt;    // per account, made once: rows it adds to a key list [2a], payload candidates [2a + 1]
  // The ledger forms (accounts named by ID, resolved on the host index): the same two counts per ENTRY, made by
  // the resolve; eacct then holds rows of the account store's replica and acnt is not read (acct_plan<true>).
  const uint32_t* ecnt = nullptr;
};

// The rows body t expands to: key rows, payload candidates, signers of its checks.
inline void acct_body_rows(const AcctIn& in, size_t t, size_t* nk, size_t* nq, size_t* ng) {
  size_t k = 0, q = 0, g = 0;
  const uint64_t e0 = in.eb[t];
  for (uint64_t e = e0; e < in.eb[t + 1]; ++e) {
    k += in.acnt[2 * (size_t)in.eacct[e]];
    q += in.acnt[2 * (size_t)in.eacct[e] + 1];
  }
  for (uint64_t c = in.cb[t]; c < in.cb[t + 1]; ++c) {
    const size_t a = in.eacct[e0 + in.cacct[c]];
    g += in.acnt[2 * a] + in.acnt[2 * a + 1];
  }
  *nk = k;
  *nq = q;
  *ng = g;
}

// ... of a ledger call, from the per-entry counts its resolve made (AcctIn::ecnt).
inline void acct_entry_rows(const AcctIn& in, size_t t, size_t* nk, size_t* nq, size_t* ng) {
  size_t k = 0, q = 0, g = 0;
  const uint64_t e0 = in.eb[t];
  for (uint64_t e = e0; e < in.eb[t + 1]; ++e) {
    k += in.ecnt[2 * e];
    q += in.ecnt[2 * e + 1];
  }
  for (uint64_t c = in.cb[t]; c < in.cb[t + 1]; ++c) {
    const uint64_t e = e0 + in.cacct[c];
    g += in.ecnt[2 * e] + in.ecnt[2 * e + 1];
  }
  *nk = k;
  *nq = q;
  *ng = g;
}

// One staging chunk of it: the hinted image of bodies [b0, b1) without keys
// (PairChunk p), followed, 16-byte aligned, by the chunk's references (ne
// account entries [e0, e1), nc checks [c0, c1), m signatures):
//   bacct_begin (8 (k + 1)) | check_begin (8 (k + 1)) | bacct (4 ne) | check_acct (4 nc) | check_needed (4 nc) |
//   check_level (nc) | sig_len (m, only with AcctIn::sig_len)
// both CSR arrays relative to e0 / c0; bacct holds global account indices (the
// table is on the device whole).  nk / nq / ng: the rows the chunk expands to.
struct AcctChunk {
  PairChunk p;
  size_t e0, e1, c0, c1, nk, nq, ng;
  size_t o_eb, o_cb, o_ea, o_ca, o_need, o_lvl, o_sl, bytes;
};

// The chunks of bodies [B0, B1): check_plan's bounds with the EXPANDED key,
// payload-candidate and signer counts standing in for the explicit ones (a
// body over a bound is a chunk alone).  kEntry: the counts are per entry (acct_entry_rows); the by-account
// instantiation is the code it was without that case.
template <bool kEntry = false>
inline std::vector<AcctChunk> acct_plan(const AcctIn& in, size_t B0, size_t B1, size_t max_s, size_t max_k,
                                        size_t max_b, size_t max_c, size_t max_g) {
  std::vector<AcctChunk> out;
  const HintIn& hi = in.h;
  size_t t = B0;
  size_t k1 = 0, q1 = 0, g1 = 0;  // body t's rows
  auto rows_of = [&](size_t b) {
    kEntry ? acct_entry_rows(in, b, &k1, &q1, &g1) : acct_body_rows(in, b, &k1, &q1, &g1);
  };
  if (t < B1) rows_of(t);
  while (t < B1) {
    const size_t b0 = t, s0 = (size_t)hi.sb[t], c0 = (size_t)in.cb[t];
    size_t bytes = 0, nk = 0, nq = 0, ng = 0;
    do {
      bytes += al16(hi.len[t]);
      nk += k1;
      nq += q1;
      ng += g1;
      ++t;
      if (t < B1) rows_of(t);
    } while (t < B1 && hi.sb[t + 1] - s0 <= max_s && nk + k1 + nq + q1 <= max_k && in.cb[t + 1] - c0 <= max_c &&
             ng + g1 <= max_g && bytes + al16(hi.len[t]) <= max_b);
    AcctChunk c{};
    c.p = pair_chunk(hi, b0, t, bytes);
    c.e0 = (size_t)in.eb[b0];
    c.e1 = (size_t)in.eb[t];
    c.c0 = c0;
    c.c1 = (size_t)in.cb[t];
    c.nk = nk;
    c.nq = nq;
    c.ng = ng;
    const size_t k = t - b0, ne = c.e1 - c.e0, nc = c.c1 - c.c0, m = c.p.s1 - c.p.s0;
    c.o_eb = al16(c.p.bytes);
    c.o_cb = c.o_eb + 8 * (k + 1);
    c.o_ea = c.o_cb + 8 * (k + 1);
    c.o_ca = c.o_ea + 4 * ne;
    c.o_need = c.o_ca + 4 * nc;
    c.o_lvl = c.o_need + 4 * nc;
    c.o_sl = c.o_lvl + nc;
    c.bytes = al16(c.o_sl + (in.sig_len ? m : 0) + 1);
    out.push_back(c);
  }
  return out;
}

inline void acct_pack(const AcctIn& in, const AcctChunk& c, uint8_t* h) {
  pair_pack(in.h, c.p, h);
  const size_t k = c.p.b1 - c.p.b0, ne = c.e1 - c.e0, nc = c.c1 - c.c0, m = c.p.s1 - c.p.s0;
  uint64_t* eb = (uint64_t*)(h + c.o_eb);
  uint64_t* cb = (uint64_t*)(h + c.o_cb);
  eb[k] = in.eb[c.p.b1] - c.e0;
  cb[k] = in.cb[c.p.b1] - c.c0;
  // the references in parts of the pack pool: rebased CSR words, plain copies of the rest
  Pool& pp = pack_pool();
  const size_t parts = pack_parts(pp.size(), t_pack_parts, 16 * k + 4 * ne + 9 * nc + m, pack_part());
  pp.run(parts, [&](size_t p) {
    for (size_t i = k * p / parts; i < k * (p + 1) / parts; ++i) {
      eb[i] = in.eb[c.p.b0 + i] - c.e0;
      cb[i] = in.cb[c.p.b0 + i] - c.c0;
    }
    size_t a = ne * p / parts, b = ne * (p + 1) / parts;
    if (b > a) std::memcpy(h + c.o_ea + 4 * a, in.eacct + c.e0 + a, 4 * (b - a));
    a = nc * p / parts, b = nc * (p + 1) / parts;
    if (b > a) {
      std::memcpy(h + c.o_ca + 4 * a, in.cacct + c.c0 + a, 4 * (b - a));
      if (in.cneed) std::memcpy(h + c.o_need + 4 * a, in.cneed + c.c0 + a, 4 * (b - a));
      else std::memset(h + c.o_need + 4 * a, 0, 4 * (b - a));
      std::memcpy(h + c.o_lvl + a, in.clevel + c.c0 + a, b - a);
    }
    a = m * p / parts, b = m * (p + 1) / parts;
    if (in.sig_len && b > a) std::memcpy(h + c.o_sl + a, in.sig_len + c.p.s0 + a, b - a);
  });
}

// Body boundaries of G slices of bodies [0, nb): boundary g is the body edge
// whose signature count is nearest to g * n / G (ties: the lower edge), kept
// non-decreasing.  cut[0] = 0, cut[G] = nb.
inline std::vector<size_t> pair_slices(const uint64_t* sb, size_t nb, size_t G) {
  std::vector<size_t> cut(G + 1, 0);
  const uint64_t n = sb[nb];
  for (size_t g = 1; g < G; ++g) {
    const uint64_t want = n / G * g + n % G * g / G;
    // first edge with sb[e] >= want, and the one before it
    size_t lo = 0, hi = nb;
    while (lo < hi) {
      const size_t mid = (lo + hi) / 2;
      if (sb[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    size_t e = lo;
    if (e > 0 && want - sb[e - 1] <= sb[e] - want) --e;
    cut[g] = std::max(e, cut[g - 1]);
  }
  cut[G] = nb;
  return cut;
}
}  // namespace
}  // namespace sv
