// See SignatureChecker.h.  Logic restated from
// /root/reference/src/transactions/SignatureChecker.cpp:30-158 and
// /root/reference/src/transactions/SignatureUtils.cpp:30-136.
#include "SignatureChecker.h"

#include <algorithm>
#include <cstring>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "../../../include/stellar_sigverify.h"
#include "HostPool.h"
#include "hashes.h"

namespace stellar {

namespace SignatureUtils {

// last 4 bytes (or the whole slice, zero-padded, if shorter); SignatureUtils.cpp:112-127
SignatureHint getHint(ByteSlice const& bs) {
  SignatureHint res{};
  if (bs.empty()) return res;
  if (res.size() > bs.size()) std::memcpy(res.data(), bs.begin(), bs.size());
  else std::memcpy(res.data(), bs.end() - res.size(), res.size());
  return res;
}

// SignatureUtils.cpp:129-136
bool doesHintMatch(ByteSlice const& bs, SignatureHint const& hint) {
  if (bs.size() < hint.size()) return false;
  return std::memcmp(bs.end() - hint.size(), hint.data(), hint.size()) == 0;
}

// key hint XOR payload hint; SignatureUtils.cpp:95-109
SignatureHint getSignedPayloadHint(SignerKey const& s) {
  SignatureHint a = getHint(ByteSlice(s.key.data(), 32));
  SignatureHint b = getHint(ByteSlice(s.payload.data(), s.payload.size()));
  SignatureHint h;
  for (int i = 0; i < 4; ++i) h[i] = a[i] ^ b[i];
  return h;
}

// SignatureUtils.cpp:38-46
bool verify(DecoratedSignature const& sig, SignerKey const& signerKey, Hash const& hash) {
  if (!doesHintMatch(ByteSlice(signerKey.key.data(), 32), sig.hint)) return false;
  PublicKey pk;
  pk.ed25519() = signerKey.key;
  return PubKeyUtils::verifySig(pk, sig.signature, ByteSlice(hash.data(), hash.size()));
}

// SignatureUtils.cpp:86-93
bool verifyHashX(DecoratedSignature const& sig, SignerKey const& signerKey) {
  if (!doesHintMatch(ByteSlice(signerKey.key.data(), 32), sig.hint)) return false;
  auto h = hostcrypto::sha256(sig.signature.data(), sig.signature.size());
  return std::memcmp(h.data(), signerKey.key.data(), 32) == 0;
}

// SignatureUtils.cpp:48-61
bool verifyEd25519SignedPayload(DecoratedSignature const& sig, SignerKey const& signer) {
  SignatureHint h = getSignedPayloadHint(signer);
  if (!doesHintMatch(ByteSlice(h.data(), 4), sig.hint)) return false;
  PublicKey pk;
  pk.ed25519() = signer.key;
  return PubKeyUtils::verifySig(pk, sig.signature, ByteSlice(signer.payload.data(), signer.payload.size()));
}

}  // namespace SignatureUtils

namespace {
uint32_t clampWeight(uint32_t protocol, uint32_t w) { return (protocol >= 10 && w > 255) ? 255 : w; }
}  // namespace

// ---------------------------------------------------------------- prefetch
void SignatureBatchPrefetch::Storage::clear() {
  pk.clear();
  sig.clear();
  msg.clear();
  hhint.clear();
  hsig.clear();
  hkey.clear();
  off.clear();
  len.clear();
  verdict.clear();
  table.clear();
  txBegin.clear();
}

// A few spares per thread: a call that holds several prefetches at once (the
// pipelined tx-set pre-pass holds two) reuses the storage of each.
std::vector<SignatureBatchPrefetch::Storage>& SignatureBatchPrefetch::spares() {
  thread_local std::vector<Storage> s;
  return s;
}

SignatureBatchPrefetch::SignatureBatchPrefetch() {
  auto& sp = spares();
  if (!sp.empty()) {
    std::swap(st_, sp.back());
    sp.pop_back();
  }
  st_.clear();
}

SignatureBatchPrefetch::~SignatureBatchPrefetch() {
  auto& sp = spares();
  if (sp.size() < kSpares) sp.push_back(std::move(st_));
}
uint64_t SignatureBatchPrefetch::hashOf(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t len) {
  // signatures and keys are uniformly distributed bytes: a few words of each
  // (plus the message's) make a good table hash; lookups compare all bytes
  uint64_t a, b, c = 0;
  std::memcpy(&a, sig, 8);
  std::memcpy(&b, pk + 24, 8);
  if (len >= 8) std::memcpy(&c, msg + len - 8, 8);
  else if (len) std::memcpy(&c, msg, len);
  uint64_t h = a ^ (b * 0x9e3779b97f4a7c15ull) ^ ((c + len) * 0xc2b2ae3d27d4eb4full);
  return h ^ (h >> 29);
}

namespace {
uint32_t hint32(const uint8_t* p) {
  uint32_t h;
  std::memcpy(&h, p, 4);
  return h;
}

// Small vector on the stack (spills to the heap past N): the per-tx scratch
// of add() and checkSignature().  Not thread_local: in a shared library every
// access to a thread_local goes through __tls_get_addr, which inside these
// loops cost more than the work (measured on MI355X hosts: add() 2.3 -> 3.9 ms
// on a 30k-pair set when its scratch was made thread_local).
template <typename T, size_t N>
class InlineVec {
 public:
  size_t size() const { return n_; }
  bool empty() const { return n_ == 0; }
  T* begin() { return data(); }
  T* end() { return data() + n_; }
  T& operator[](size_t i) { return data()[i]; }
  void push_back(T const& v) {
    if (heap_.empty() && n_ < N) {
      buf_[n_++] = v;
      return;
    }
    if (heap_.empty()) heap_.assign(buf_, buf_ + N);
    heap_.push_back(v);
    ++n_;
  }
  T* erase(T* it) {
    T* d = data();
    std::copy(it + 1, d + n_, it);
    --n_;
    if (!heap_.empty()) heap_.pop_back();
    return it;
  }

 private:
  T* data() { return heap_.empty() ? buf_ : heap_.data(); }
  T buf_[N];
  size_t n_ = 0;
  std::vector<T> heap_;
};
}  // namespace

namespace {
// A tx's ed25519 / signed-payload signers with their hints as 32-bit words
// (the signers' hints are formed once per tx and compared as words).
struct TxSigners {
  InlineVec<uint32_t, 48> hints;
  InlineVec<const Signer*, 48> eds;
  explicit TxSigners(std::vector<Signer> const& signers) {
    for (auto const& s : signers) {
      if (s.key.type == SIGNER_KEY_TYPE_ED25519) {
        hints.push_back(hint32(s.key.key.data() + 28));
        eds.push_back(&s);
      } else if (s.key.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD) {
        const SignatureHint h = SignatureUtils::getSignedPayloadHint(s.key);
        hints.push_back(hint32(h.data()));
        eds.push_back(&s);
      }
    }
  }
};

// Visits the pairs SignatureChecker would verify for one tx, in its order
// per signature: hint-matching ED25519 signers (SignatureUtils::verify) and
// ED25519_SIGNED_PAYLOAD signers (verifyEd25519SignedPayload) --
// fn(signature, signer index k in eds).
template <class F>
void forEachPair(TxSigners& ts, std::vector<DecoratedSignature> const& signatures, F fn) {
  if (ts.eds.empty()) return;
  for (auto const& sig : signatures) {
    if (sig.signature.size() != 64) continue;  // verifySig rejects before verifying
    const uint32_t h = hint32(sig.hint.data());
    for (size_t k = 0; k < ts.eds.size(); ++k)
      if (ts.hints[k] == h) fn(sig, k);
  }
}
}  // namespace

uint64_t SignatureBatchPrefetch::enumerate(Storage& st, Hash const& contentsHash,
                                           std::vector<DecoratedSignature> const& signatures,
                                           std::vector<Signer> const& signers) {
  TxSigners ts(signers);
  if (ts.eds.empty()) return ~0ull;
  auto pushMsg = [&](const uint8_t* msg, size_t msgLen) {
    const uint64_t off = st.msg.size();
    st.msg.resize(off + msgLen);
    if (msgLen) std::memcpy(&st.msg[off], msg, msgLen);
    return off;
  };
  // message bytes are stored once per tx (contents hash) / per payload signer
  uint64_t hashOff = ~0ull;
  InlineVec<uint64_t, 48> payOff;
  for (size_t k = 0; k < ts.eds.size(); ++k) payOff.push_back(~0ull);
  forEachPair(ts, signatures, [&](DecoratedSignature const& sig, size_t k) {
    Signer const& s = *ts.eds[k];
    uint64_t mo;
    size_t ml;
    if (s.key.type == SIGNER_KEY_TYPE_ED25519) {
      if (hashOff == ~0ull) hashOff = pushMsg(contentsHash.data(), 32);
      mo = hashOff;
      ml = 32;
    } else {
      if (payOff[k] == ~0ull) payOff[k] = pushMsg(s.key.payload.data(), s.key.payload.size());
      mo = payOff[k];
      ml = s.key.payload.size();
    }
    const size_t i = st.len.size();
    st.pk.resize(32 * (i + 1));
    st.sig.resize(64 * (i + 1));
    std::memcpy(&st.pk[32 * i], s.key.key.data(), 32);
    std::memcpy(&st.sig[64 * i], sig.signature.data(), 64);
    st.off.push_back(mo);
    st.len.push_back((uint32_t)ml);
  });
  return hashOff;
}

void SignatureBatchPrefetch::add(Hash const& contentsHash, std::vector<DecoratedSignature> const& signatures,
                                 std::vector<Signer> const& signers) {
  enumerate(st_, contentsHash, signatures, signers);
}

void SignatureBatchPrefetch::add(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
                                 std::vector<Signer> const& signers) {
  static const Hash kUnknown{};  // (the bytes are patched in runBodies)
  BodyEntry e;
  e.body = body;
  e.pair0 = len_.size();
  e.hashOff = enumerate(st_, kUnknown, signatures, signers);
  e.pair1 = len_.size();
  bodies_.push_back(e);
}

void SignatureBatchPrefetch::runBodies(const uint8_t* networkID, const uint8_t* blob) {
  const size_t n = len_.size(), nb = bodies_.size();
  verdict_.assign(n, 0);
  if (nb == 0) return;
  // the engine's batch: bodies in add() order, their ed25519 pairs (the ones
  // whose message is the body's hash) gathered next to each other; every
  // other pair is a signed-payload pair
  std::vector<uint64_t> off(nb), sigBegin(nb + 1, 0);
  std::vector<uint32_t> len(nb);
  std::vector<uint8_t> kind(nb), digests(32 * nb);
  std::vector<uint32_t> edPair, payPair;
  for (size_t b = 0; b < nb; ++b) {
    BodyEntry const& e = bodies_[b];
    off[b] = e.body.off;
    len[b] = e.body.len;
    kind[b] = e.body.kind;
    for (size_t i = e.pair0; i < e.pair1; ++i) {
      // (an empty payload stored just before the hash shares its offset: the length tells them apart)
      if (e.hashOff != ~0ull && off_[i] == e.hashOff && len_[i] == 32) edPair.push_back((uint32_t)i);
      else payPair.push_back((uint32_t)i);
    }
    sigBegin[b + 1] = edPair.size();
  }
  const size_t ne = edPair.size();
  std::vector<uint8_t> pk(32 * std::max<size_t>(ne, 1)), sig(64 * std::max<size_t>(ne, 1)), v(std::max<size_t>(ne, 1));
  for (size_t k = 0; k < ne; ++k) {
    std::memcpy(&pk[32 * k], &pk_[32 * (size_t)edPair[k]], 32);
    std::memcpy(&sig[64 * k], &sig_[64 * (size_t)edPair[k]], 64);
  }
  PubKeyUtils::verifyTxBodiesUncached(networkID, blob, off.data(), len.data(), kind.data(), nb, sigBegin.data(),
                                      pk.data(), sig.data(), ne, v.data(), digests.data());
  for (size_t b = 0; b < nb; ++b) {
    BodyEntry const& e = bodies_[b];
    if (e.body.hashOut) std::memcpy(e.body.hashOut->data(), &digests[32 * b], 32);
    if (e.hashOff != ~0ull) std::memcpy(&msg_[e.hashOff], &digests[32 * b], 32);
  }
  for (size_t k = 0; k < ne; ++k) verdict_[edPair[k]] = v[k];
  if (const size_t np = payPair.size()) {
    std::vector<uint8_t> ppk(32 * np), psig(64 * np), pv(np);
    std::vector<uint64_t> poff(np);
    std::vector<uint32_t> plen(np);
    for (size_t k = 0; k < np; ++k) {
      const size_t i = payPair[k];
      std::memcpy(&ppk[32 * k], &pk_[32 * i], 32);
      std::memcpy(&psig[64 * k], &sig_[64 * i], 64);
      poff[k] = off_[i];
      plen[k] = len_[i];
    }
    static const uint8_t dummy = 0;
    PubKeyUtils::verifyBatchUncached(ppk.data(), psig.data(), msg_.empty() ? &dummy : msg_.data(), poff.data(),
                                     plen.data(), np, pv.data());
    for (size_t k = 0; k < np; ++k) verdict_[payPair[k]] = pv[k];
  }
  buildTable();  // (after the hashes are in place: the table hashes the message bytes)
}

void SignatureBatchPrefetch::addHinted(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
                                       std::vector<Signer> const& signers) {
  BodyEntry e;
  e.body = body;
  e.hashOff = ~0ull;
  for (auto const& sig : signatures) {
    if (sig.signature.size() != 64) continue;  // verifySig rejects before verifying
    const size_t i = hHint_.size() / 4;
    hHint_.resize(4 * (i + 1));
    hSig_.resize(64 * (i + 1));
    std::memcpy(&hHint_[4 * i], sig.hint.data(), 4);
    std::memcpy(&hSig_[64 * i], sig.signature.data(), 64);
  }
  // the signed-payload pairs of this tx go to the pair storage now (st_); the
  // engine's pairs are put in front of them by runBodiesHinted
  e.pair0 = len_.size();
  for (auto const& s : signers) {
    if (s.key.type == SIGNER_KEY_TYPE_ED25519) {
      const size_t i = hKey_.size() / 32;
      hKey_.resize(32 * (i + 1));
      std::memcpy(&hKey_[32 * i], s.key.key.data(), 32);
    } else if (s.key.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD) {
      const SignatureHint sh = SignatureUtils::getSignedPayloadHint(s.key);
      const uint32_t h = hint32(sh.data());
      uint64_t payOff = ~0ull;
      for (auto const& sig : signatures) {
        if (sig.signature.size() != 64 || hint32(sig.hint.data()) != h) continue;
        if (payOff == ~0ull) {
          payOff = msg_.size();
          msg_.insert(msg_.end(), s.key.payload.begin(), s.key.payload.end());
        }
        const size_t i = len_.size();
        pk_.resize(32 * (i + 1));
        sig_.resize(64 * (i + 1));
        std::memcpy(&pk_[32 * i], s.key.key.data(), 32);
        std::memcpy(&sig_[64 * i], sig.signature.data(), 64);
        off_.push_back(payOff);
        len_.push_back((uint32_t)s.key.payload.size());
      }
    }
  }
  e.pair1 = len_.size();
  bodies_.push_back(e);
  hSigBegin_.push_back(hHint_.size() / 4);
  hKeyBegin_.push_back(hKey_.size() / 32);
}

void SignatureBatchPrefetch::runBodiesHinted(const uint8_t* networkID, const uint8_t* blob) {
  const size_t nb = bodies_.size(), npay = len_.size();
  verdict_.assign(npay, 0);
  if (nb == 0) return;
  std::vector<uint64_t> off(nb), pairBegin(nb + 1, 0);
  std::vector<uint32_t> len(nb);
  std::vector<uint8_t> kind(nb), digests(32 * nb);
  for (size_t b = 0; b < nb; ++b) {
    off[b] = bodies_[b].body.off;
    len[b] = bodies_[b].body.len;
    kind[b] = bodies_[b].body.kind;
  }
  const size_t ns = hHint_.size() / 4, nk = hKey_.size() / 32;
  const size_t cap = sv_txbodies_pair_bound(hSigBegin_.data(), hKeyBegin_.data(), nb);
  std::vector<uint32_t> pairSig(cap), pairKey(cap);
  std::vector<uint8_t> pv(cap);
  const size_t np = PubKeyUtils::verifyTxBodiesHintedUncached(
      networkID, blob, off.data(), len.data(), kind.data(), nb, hSigBegin_.data(), hHint_.data(), hSig_.data(), ns,
      hKeyBegin_.data(), hKey_.data(), nk, cap, pairBegin.data(), pairSig.data(), pairKey.data(), pv.data(),
      digests.data());
  for (size_t b = 0; b < nb; ++b)
    if (bodies_[b].body.hashOut) std::memcpy(bodies_[b].body.hashOut->data(), &digests[32 * b], 32);
  // The pair storage: the engine's np pairs first, in its order (body,
  // signature, key), their messages the digests; behind them the signed-payload
  // pairs enumerated by addHinted, verified as a batch of their own.
  RawVec<uint8_t> ppk, psig, pmsg;
  RawVec<uint64_t> poff;
  RawVec<uint32_t> plen;
  ppk.swap(pk_);
  psig.swap(sig_);
  pmsg.swap(msg_);
  poff.swap(off_);
  plen.swap(len_);
  const size_t n = np + npay;
  pk_.resize(32 * n);
  sig_.resize(64 * n);
  off_.resize(n);
  len_.resize(n);
  msg_.resize(32 * nb + pmsg.size());
  std::memcpy(msg_.data(), digests.data(), 32 * nb);
  if (!pmsg.empty()) std::memcpy(&msg_[32 * nb], pmsg.data(), pmsg.size());
  verdict_.assign(n, 0);
  txBegin_.resize(nb + 1);
  for (size_t b = 0; b < nb; ++b) {
    txBegin_[b] = (uint32_t)pairBegin[b];
    for (size_t i = pairBegin[b]; i < pairBegin[b + 1]; ++i) {
      std::memcpy(&pk_[32 * i], &hKey_[32 * (size_t)pairKey[i]], 32);
      std::memcpy(&sig_[64 * i], &hSig_[64 * (size_t)pairSig[i]], 64);
      off_[i] = 32 * b;
      len_[i] = 32;
      verdict_[i] = pv[i];
    }
  }
  txBegin_[nb] = (uint32_t)np;
  if (npay) {
    std::memcpy(&pk_[32 * np], ppk.data(), 32 * npay);
    std::memcpy(&sig_[64 * np], psig.data(), 64 * npay);
    for (size_t k = 0; k < npay; ++k) {
      off_[np + k] = 32 * nb + poff[k];
      len_[np + k] = plen[k];
    }
    PubKeyUtils::verifyBatchUncached(&pk_[32 * np], &sig_[64 * np], msg_.data(), &off_[np], &len_[np], npay,
                                     &verdict_[np]);
  }
  buildTable();
}

bool SignatureBatchPrefetch::addDecided(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
                                        std::vector<SignatureCheck> const& checks, bool withPayload) {
  if (signatures.size() > 64) return false;
  for (auto const& sig : signatures)
    if (sig.signature.size() > 64) return false;
  for (auto const& c : checks) {
    if (c.signers.size() > 64) return false;
    if (withPayload)
      for (auto const& s : c.signers)
        if (s.key.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD && s.key.payload.size() > 64) return false;
  }
  Decided& d = dec_;
  d.payload = withPayload;
  BodyEntry e;
  e.body = body;
  e.pair0 = e.pair1 = 0;
  e.hashOff = ~0ull;
  bodies_.push_back(e);
  for (auto const& sig : signatures) {
    const size_t i = d.sigLen.size();
    d.hint.resize(4 * (i + 1));
    d.sig.resize(64 * (i + 1), 0);
    std::memcpy(&d.hint[4 * i], sig.hint.data(), 4);
    if (!sig.signature.empty()) std::memcpy(&d.sig[64 * i], sig.signature.data(), sig.signature.size());
    d.sigLen.push_back((uint8_t)sig.signature.size());
  }
  // the body's candidate rows: every distinct 32-byte key its checks name (the
  // source account's signers recur in every operation's check)
  const size_t k0 = d.key.size() / 32, q0 = d.pkeyLen.size();
  for (auto const& c : checks) {
    for (auto const& s : c.signers) {
      if (s.key.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD) {
        if (!withPayload) continue;  // the caller's stage
        // the body's payload candidates: every distinct (key, payload) its checks name
        const size_t n = s.key.payload.size(), q1 = d.pkeyLen.size();
        size_t q = q0;
        while (q < q1 && !(d.pkeyLen[q] == n && std::memcmp(&d.pkey[32 * q], s.key.key.data(), 32) == 0 &&
                           (n == 0 || std::memcmp(&d.pkeyPayload[64 * q], s.key.payload.data(), n) == 0)))
          ++q;
        if (q == q1) {
          d.pkey.resize(32 * (q1 + 1));
          d.pkeyPayload.resize(64 * (q1 + 1), 0);
          std::memcpy(&d.pkey[32 * q1], s.key.key.data(), 32);
          if (n) std::memcpy(&d.pkeyPayload[64 * q1], s.key.payload.data(), n);
          d.pkeyLen.push_back((uint8_t)n);
        }
        d.type.push_back((uint8_t)s.key.type);
        d.weight.push_back(s.weight);
        d.keyIndex.push_back((uint32_t)q);
        continue;
      }
      size_t k = k0;
      const size_t k1 = d.key.size() / 32;
      while (k < k1 && std::memcmp(&d.key[32 * k], s.key.key.data(), 32) != 0) ++k;
      if (k == k1) {
        d.key.resize(32 * (k1 + 1));
        std::memcpy(&d.key[32 * k1], s.key.key.data(), 32);
      }
      d.type.push_back((uint8_t)s.key.type);
      d.weight.push_back(s.weight);
      d.keyIndex.push_back((uint32_t)k);
    }
    d.needed.push_back(c.needed);
    d.signerBegin.push_back(d.type.size());
  }
  d.sigBegin.push_back(d.sigLen.size());
  d.keyBegin.push_back(d.key.size() / 32);
  d.checkBegin.push_back(d.needed.size());
  d.pkeyBegin.push_back(d.pkeyLen.size());
  return true;
}

void SignatureBatchPrefetch::runDecided(const uint8_t* networkID, const uint8_t* blob, uint32_t protocolVersion) {
  Decided& d = dec_;
  const size_t nb = bodies_.size(), nc = d.needed.size();
  d.ok.assign(nc, 0);
  d.outWeight.assign(nc, 0);
  d.used.assign(nc, 0);
  if (nb == 0) return;
  std::vector<uint64_t> off(nb);
  std::vector<uint32_t> len(nb);
  std::vector<uint8_t> kind(nb), digests(32 * nb);
  for (size_t b = 0; b < nb; ++b) {
    off[b] = bodies_[b].body.off;
    len[b] = bodies_[b].body.len;
    kind[b] = bodies_[b].body.kind;
  }
  // (the plain struct unless the payload candidates go along: the engine reads only what struct_size covers)
  sv_txchecks_payload ckp;
  sv_txchecks& ck = ckp.checks;
  ck.struct_size = d.payload ? sizeof ckp : sizeof ck;
  ckp.pkey_begin = d.pkeyBegin.data();
  ckp.pkey = d.pkey.data();
  ckp.pkey_payload = d.pkeyPayload.data();
  ckp.pkey_len = d.pkeyLen.data();
  ckp.n_pkeys = d.pkeyLen.size();
  ck.protocol_version = protocolVersion;
  ck.sig_len = d.sigLen.data();
  ck.check_begin = d.checkBegin.data();
  ck.check_needed = d.needed.data();
  ck.signer_begin = d.signerBegin.data();
  ck.signer_type = d.type.data();
  ck.signer_weight = d.weight.data();
  ck.signer_key = d.keyIndex.data();
  ck.n_checks = nc;
  ck.n_signers = d.type.size();
  PubKeyUtils::checkTxBodiesUncached(networkID, blob, off.data(), len.data(), kind.data(), nb, d.sigBegin.data(),
                                     d.hint.data(), d.sig.data(), d.sigLen.size(), d.keyBegin.data(), d.key.data(),
                                     d.key.size() / 32, ck, d.ok.data(), d.outWeight.data(), d.used.data(),
                                     digests.data());
  for (size_t b = 0; b < nb; ++b)
    if (bodies_[b].body.hashOut) std::memcpy(bodies_[b].body.hashOut->data(), &digests[32 * b], 32);
}

uint32_t SignatureBatchPrefetch::appendAccount(uint256 const* id, uint8_t const* thresholds,
                                               std::vector<Signer> const* signers,
                                               std::vector<SignerKey> const* extra) {
  Accounts& a = acct_;
  const uint32_t index = (uint32_t)(a.thr.size() / 4);
  static const uint8_t kNoAccount[4] = {1, 0, 0, 0}, kExtra[4] = {0, 0, 0, 0};
  const uint8_t* thr = extra ? kExtra : thresholds ? thresholds : kNoAccount;
  a.key.resize(a.key.size() + 32, 0);
  if (id) std::memcpy(&a.key[a.key.size() - 32], id->data(), 32);
  a.thr.insert(a.thr.end(), thr, thr + 4);
  auto add = [&](SignerKey const& k, uint32_t weight) {
    a.stype.push_back((uint8_t)k.type);
    a.sweight.push_back(weight);
    a.skey.insert(a.skey.end(), k.key.begin(), k.key.end());
    uint32_t row = 0;
    if (k.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD) {
      row = (uint32_t)a.plen.size();
      a.pay.resize(a.pay.size() + 64, 0);
      if (!k.payload.empty()) std::memcpy(&a.pay[64 * (size_t)row], k.payload.data(), k.payload.size());
      a.plen.push_back((uint8_t)k.payload.size());
    }
    a.spay.push_back(row);
  };
  if (extra)
    for (auto const& k : *extra) add(k, 1);
  else if (signers)
    for (auto const& g : *signers) add(g.key, g.weight);
  a.sbeg.push_back(a.stype.size());
  return index;
}

bool SignatureBatchPrefetch::addDecidedRefs(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
                                            std::vector<SignatureCheckRef> const& checks, bool skipUnused,
                                            bool listedOk) {
  if (signatures.size() > 64) return false;
  for (auto const& sig : signatures)
    if (sig.signature.size() > 64) return false;
  for (auto const& c : checks) {
    if (c.extra) {
      if (c.extra->size() > 64) return false;
      for (auto const& k : *c.extra)
        if (k.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD && k.payload.size() > 64) return false;
    } else if (c.thresholds) {
      if ((c.thresholds[0] ? 1 : 0) + c.signers->size() > 64) return false;
      for (auto const& g : *c.signers)
        if (g.key.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD && g.key.payload.size() > 64) return false;
    }
  }
  Decided& d = dec_;
  Accounts& a = acct_;
  d.payload = true;  // (the table carries the payloads: every decision is final)
  BodyEntry e;
  e.body = body;
  e.pair0 = e.pair1 = 0;
  e.hashOff = ~0ull;
  bodies_.push_back(e);
  for (auto const& sig : signatures) {
    const size_t i = d.sigLen.size();
    d.hint.resize(4 * (i + 1));
    d.sig.resize(64 * (i + 1), 0);
    std::memcpy(&d.hint[4 * i], sig.hint.data(), 4);
    if (!sig.signature.empty()) std::memcpy(&d.sig[64 * i], sig.signature.data(), sig.signature.size());
    d.sigLen.push_back((uint8_t)sig.signature.size());
  }
  const size_t e0 = a.bacct.size();
  for (auto const& c : checks) {
    size_t pos;
    if (c.thresholds && !c.extra) {
      // a ledger account: once in the table, once in the body's list
      auto it = a.byId.find(*c.id);
      const uint32_t index =
          it != a.byId.end() ? it->second : (a.byId[*c.id] = appendAccount(c.id, c.thresholds, c.signers, nullptr));
      pos = e0;
      while (pos < a.bacct.size() && a.bacct[pos] != index) ++pos;
      if (pos == a.bacct.size()) a.bacct.push_back(index);
    } else {
      pos = a.bacct.size();
      a.bacct.push_back(appendAccount(c.id, nullptr, nullptr, c.extra));
    }
    a.cacct.push_back((uint32_t)(pos - e0));
    a.clevel.push_back(c.level);
    d.needed.push_back(c.needed);
    d.role.push_back(c.role);
  }
  d.bodyFlags.push_back(skipUnused ? SV_TXBODY_SKIP_UNUSED : 0);
  d.listedOk.push_back(listedOk ? 1 : 0);
  d.sigBegin.push_back(d.sigLen.size());
  d.checkBegin.push_back(d.needed.size());
  a.bacctBegin.push_back(a.bacct.size());
  return true;
}

struct SignatureBatchPrefetch::AccountsCall {
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  std::vector<uint8_t> kind, digests;
  sv_txaccounts A{};
};

void SignatureBatchPrefetch::fillAccountsCall(AccountsCall& c, uint32_t protocolVersion) const {
  Decided const& d = dec_;
  Accounts const& a = acct_;
  const size_t nb = bodies_.size(), nc = d.needed.size();
  c.off.resize(nb);
  c.len.resize(nb);
  c.kind.resize(nb);
  c.digests.resize(32 * nb);
  for (size_t b = 0; b < nb; ++b) {
    c.off[b] = bodies_[b].body.off;
    c.len[b] = bodies_[b].body.len;
    c.kind[b] = bodies_[b].body.kind;
  }
  sv_txaccounts& A = c.A;
  A.struct_size = sizeof A;
  A.protocol_version = protocolVersion;
  A.sig_len = d.sigLen.data();
  A.acct_key = a.key.data();
  A.acct_thresholds = a.thr.data();
  A.asigner_begin = a.sbeg.data();
  A.asigner_type = a.stype.data();
  A.asigner_weight = a.sweight.data();
  A.asigner_key = a.skey.data();
  A.asigner_payload = a.spay.data();
  A.apayload = a.pay.data();
  A.apayload_len = a.plen.data();
  A.bacct_begin = a.bacctBegin.data();
  A.bacct = a.bacct.data();
  A.check_begin = d.checkBegin.data();
  A.check_acct = a.cacct.data();
  A.check_level = a.clevel.data();
  A.check_needed = d.needed.data();
  A.n_accounts = a.thr.size() / 4;
  A.n_asigners = a.stype.size();
  A.n_apayloads = a.plen.size();
  A.n_bacct = a.bacct.size();
  A.n_checks = nc;
}

void SignatureBatchPrefetch::runDecidedRefs(const uint8_t* networkID, const uint8_t* blob, uint32_t protocolVersion) {
  Decided& d = dec_;
  const size_t nb = bodies_.size(), nc = d.needed.size();
  d.ok.assign(nc, 0);
  d.outWeight.assign(nc, 0);
  d.used.assign(nc, 0);
  if (nb == 0) return;
  AccountsCall c;
  fillAccountsCall(c, protocolVersion);
  PubKeyUtils::checkTxBodiesAccountsUncached(networkID, blob, c.off.data(), c.len.data(), c.kind.data(), nb,
                                             d.sigBegin.data(), d.hint.data(), d.sig.data(), d.sigLen.size(), c.A,
                                             d.ok.data(), d.outWeight.data(), d.used.data(), c.digests.data());
  for (size_t b = 0; b < nb; ++b)
    if (bodies_[b].body.hashOut) std::memcpy(bodies_[b].body.hashOut->data(), &c.digests[32 * b], 32);
}

void SignatureBatchPrefetch::runDecidedResults(const uint8_t* networkID, const uint8_t* blob,
                                               uint32_t protocolVersion) {
  Decided& d = dec_;
  const size_t nb = bodies_.size();
  // (fail closed: a body the engine never reached is not OK)
  d.bodyCode.assign(nb, SV_TXRESULT_BAD_AUTH);
  d.bodyFail.assign(nb, 0);
  if (nb == 0) return;
  AccountsCall c;
  fillAccountsCall(c, protocolVersion);
  sv_txresults R{};
  R.struct_size = sizeof R;
  R.check_role = d.role.data();
  R.body_flags = d.bodyFlags.data();
  R.body_code = d.bodyCode.data();
  R.body_fail = d.bodyFail.data();
  PubKeyUtils::decideTxBodiesAccountsUncached(networkID, blob, c.off.data(), c.len.data(), c.kind.data(), nb,
                                              d.sigBegin.data(), d.hint.data(), d.sig.data(), d.sigLen.size(), c.A, R,
                                              c.digests.data());
  for (size_t b = 0; b < nb; ++b)
    if (bodies_[b].body.hashOut) std::memcpy(bodies_[b].body.hashOut->data(), &c.digests[32 * b], 32);
}

SignatureBatchPrefetch::BodyResult SignatureBatchPrefetch::bodyResult(size_t body) const {
  if (body >= dec_.bodyCode.size() || body >= dec_.listedOk.size())
    throw std::out_of_range("SignatureBatchPrefetch::bodyResult: no such body (or runDecidedResults has not run)");
  return BodyResult{dec_.bodyCode[body], dec_.bodyFail[body], dec_.listedOk[body] != 0};
}

SignatureBatchPrefetch::Decision SignatureBatchPrefetch::decision(size_t body, size_t check) const {
  const size_t c = (size_t)dec_.checkBegin.at(body) + check;
  if (c >= dec_.checkBegin.at(body + 1) || c >= dec_.ok.size())
    throw std::out_of_range("SignatureBatchPrefetch::decision: no such check (or runDecided has not run)");
  return Decision{dec_.ok[c] != 0, dec_.outWeight[c], dec_.used[c]};
}

void SignatureBatchPrefetch::addBatch(std::vector<TxRef> const& txs, std::function<void(size_t)> const& prepare) {
  const size_t ntx = txs.size();
  if (txBegin_.empty()) txBegin_.push_back((uint32_t)len_.size());
  constexpr size_t kGrain = 256;
  // one contiguous range of txs per thread (the pool's helpers and this one):
  // equal ranges balance well at this grain, where more parts than threads
  // left some threads two parts and the others one (profiles/r06/config3/)
  const size_t parts = std::min(hostPoolThreads(), std::max<size_t>(1, ntx / kGrain));
  if (parts == 1) {
    for (size_t k = 0; k < ntx; ++k) {
      if (prepare) prepare(k);
      enumerate(st_, *txs[k].contentsHash, *txs[k].signatures, *txs[k].signers);
      txBegin_.push_back((uint32_t)len_.size());
    }
    return;
  }
  // Two passes over the set, each one contiguous range of txs per part, and
  // no scratch copy between them: pass 1 prepares (marshals) each tx and
  // counts its pairs and message bytes; after a prefix sum, pass 2 writes
  // every pair straight to its final place.  (The previous single pass
  // enumerated into per-part scratch and then copied it: ~30 % of the phase.)
  // An exception must not leave a pool thread: the first is kept and
  // rethrown here once every part has finished.
  std::exception_ptr failed;
  std::mutex failMu;
  const size_t t0base = txBegin_.size() - 1;  // (this batch's first tx index)
  const size_t pair0 = len_.size(), msg0 = msg_.size();
  std::vector<uint32_t> npairs(ntx), nbytes(ntx);
  std::vector<uint64_t> partPairs(parts + 1, 0), partBytes(parts + 1, 0);
  hostParallelFor(parts, 1, [&](size_t a, size_t b) {
    for (size_t p = a; p < b; ++p) {
      const size_t t0 = ntx * p / parts, t1 = ntx * (p + 1) / parts;
      uint64_t pp = 0, pb = 0;
      try {
        for (size_t t = t0; t < t1; ++t) {
          if (prepare) prepare(t);
          TxSigners ts(*txs[t].signers);
          uint32_t np = 0, nb = 0, hashUsed = 0;
          InlineVec<uint8_t, 48> payUsed;
          for (size_t k = 0; k < ts.eds.size(); ++k) payUsed.push_back(0);
          forEachPair(ts, *txs[t].signatures, [&](DecoratedSignature const&, size_t k) {
            ++np;
            if (ts.eds[k]->key.type == SIGNER_KEY_TYPE_ED25519) {
              if (!hashUsed) nb += 32;
              hashUsed = 1;
            } else if (!payUsed[k]) {
              nb += (uint32_t)ts.eds[k]->key.payload.size();
              payUsed[k] = 1;
            }
          });
          npairs[t] = np;
          nbytes[t] = nb;
          pp += np;
          pb += nb;
        }
      } catch (...) {
        std::lock_guard<std::mutex> g(failMu);
        if (!failed) failed = std::current_exception();
      }
      partPairs[p + 1] = pp;
      partBytes[p + 1] = pb;
    }
  });
  if (failed) std::rethrow_exception(failed);
  for (size_t p = 0; p < parts; ++p) {
    partPairs[p + 1] += partPairs[p];
    partBytes[p + 1] += partBytes[p];
  }
  const size_t n = pair0 + partPairs[parts];
  pk_.resize(32 * n);
  sig_.resize(64 * n);
  off_.resize(n);
  len_.resize(n);
  msg_.resize(msg0 + partBytes[parts]);
  txBegin_.resize(t0base + 1 + ntx);
  hostParallelFor(parts, 1, [&](size_t a, size_t b) {
    for (size_t p = a; p < b; ++p) {
      const size_t t0 = ntx * p / parts, t1 = ntx * (p + 1) / parts;
      size_t i = pair0 + partPairs[p];
      uint64_t mpos = msg0 + partBytes[p];
      for (size_t t = t0; t < t1; ++t) {
        TxSigners ts(*txs[t].signers);
        uint64_t hashOff = ~0ull;
        InlineVec<uint64_t, 48> payOff;
        for (size_t k = 0; k < ts.eds.size(); ++k) payOff.push_back(~0ull);
        Hash const& ch = *txs[t].contentsHash;
        forEachPair(ts, *txs[t].signatures, [&](DecoratedSignature const& sig, size_t k) {
          Signer const& s = *ts.eds[k];
          uint64_t mo;
          uint32_t ml;
          if (s.key.type == SIGNER_KEY_TYPE_ED25519) {
            if (hashOff == ~0ull) {
              hashOff = mpos;
              std::memcpy(&msg_[mpos], ch.data(), 32);
              mpos += 32;
            }
            mo = hashOff;
            ml = 32;
          } else {
            ml = (uint32_t)s.key.payload.size();
            if (payOff[k] == ~0ull) {
              payOff[k] = mpos;
              if (ml) std::memcpy(&msg_[mpos], s.key.payload.data(), ml);
              mpos += ml;
            }
            mo = payOff[k];
          }
          std::memcpy(&pk_[32 * i], s.key.key.data(), 32);
          std::memcpy(&sig_[64 * i], sig.signature.data(), 64);
          off_[i] = mo;
          len_[i] = ml;
          ++i;
        });
        txBegin_[t0base + 1 + t] = (uint32_t)i;
      }
    }
  });
}

void SignatureBatchPrefetch::buildTable() {
  const size_t n = len_.size();
  const uint8_t* msg = msg_.empty() ? nullptr : msg_.data();
  size_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  mask_ = cap - 1;
  table_.assign(cap, 0u);
  for (size_t i = 0; i < n; ++i) {
    size_t s = hashOf(&pk_[32 * i], &sig_[64 * i], msg ? msg + off_[i] : nullptr, len_[i]) & mask_;
    while (table_[s] != 0) s = (s + 1) & mask_;
    table_[s] = (uint32_t)(i + 1);
  }
}

void SignatureBatchPrefetch::run(bool seedCache) {
  const size_t n = len_.size();
  verdict_.assign(n, 0);
#ifdef FUZZING_BUILD_MODE_UNSAFE_FOR_PRODUCTION
  (void)seedCache;
  return;  // the checkers accept without looking (checkSignature): nothing to verify
#endif
  if (n == 0) return;
  const uint8_t* msg = msg_.empty() ? nullptr : msg_.data();
  // the lookup table needs only the pairs' bytes: it is built on a helper
  // thread while the engine verifies (large batches only)
  std::thread tb;
  if (n >= kAsyncTableMin) tb = std::thread([this] { buildTable(); });
  struct Join {
    std::thread& t;
    ~Join() {
      if (t.joinable()) t.join();
    }
  } join{tb};
  if (seedCache) {
    std::vector<PublicKey> keys(n);
    std::vector<PubKeyUtils::VerifyItem> items(n);
    for (size_t i = 0; i < n; ++i) {
      std::memcpy(keys[i].ed25519().data(), &pk_[32 * i], 32);
      items[i] = PubKeyUtils::VerifyItem{&keys[i], ByteSlice(&sig_[64 * i], 64),
                                         ByteSlice(msg ? msg + off_[i] : nullptr, len_[i])};
    }
    std::vector<bool> v = PubKeyUtils::verifySigBatch(items);
    for (size_t i = 0; i < n; ++i) verdict_[i] = v[i] ? 1 : 0;
  } else {
    static const uint8_t dummy = 0;
    PubKeyUtils::verifyBatchUncached(pk_.data(), sig_.data(), msg ? msg : &dummy, off_.data(), len_.data(), n,
                                     verdict_.data());
  }
  if (tb.joinable()) tb.join();
  else buildTable();
}

bool SignatureBatchPrefetch::lookup(uint256 const& pk, Signature const& sig, ByteSlice const& msg, bool& verdict,
                                    size_t tx) const {
  if (sig.size() != 64) return false;
  auto same = [&](size_t i) {
    return len_[i] == msg.size() && std::memcmp(&sig_[64 * i], sig.data(), 64) == 0 &&
           std::memcmp(&pk_[32 * i], pk.data(), 32) == 0 &&
           (msg.size() == 0 || std::memcmp(&msg_[off_[i]], msg.data(), msg.size()) == 0);
  };
  if (tx != kNoTx && tx + 1 < txBegin_.size()) {  // the tx's own pairs, contiguous (addBatch)
    for (size_t i = txBegin_[tx]; i < txBegin_[tx + 1]; ++i)
      if (same(i)) {
        verdict = verdict_[i] != 0;
        return true;
      }
  }
  if (table_.empty()) return false;
  for (size_t s = hashOf(pk.data(), sig.data(), msg.data(), msg.size()) & mask_;; s = (s + 1) & mask_) {
    const uint32_t t = table_[s];
    if (t == 0) return false;
    const size_t i = t - 1;
    if (same(i)) {
      verdict = verdict_[i] != 0;
      return true;
    }
  }
}

// ---------------------------------------------------------------- checker
SignatureChecker::SignatureChecker(uint32_t protocolVersion, Hash const& contentsHash,
                                   std::vector<DecoratedSignature> const& signatures,
                                   SignatureBatchPrefetch const* prefetched, size_t prefetchTx)
    : mProtocolVersion(protocolVersion),
      mContentsHash(contentsHash),
      mSignatures(signatures),
      mUsedSignatures(signatures.size()),
      mPrefetched(prefetched),
      mPrefetchTx(prefetchTx) {}

bool SignatureChecker::verifyEd25519(DecoratedSignature const& sig, uint256 const& key, ByteSlice const& msg) const {
  if (mPrefetched && sig.signature.size() == 64) {
    bool v;
    if (mPrefetched->lookup(key, sig.signature, msg, v, mPrefetchTx)) return v;
  }
  PublicKey pk;
  pk.ed25519() = key;
  return PubKeyUtils::verifySig(pk, sig.signature, msg);
}

bool SignatureChecker::checkSignature(std::vector<Signer> const& signersV, int32_t neededWeight) {
#ifdef FUZZING_BUILD_MODE_UNSAFE_FOR_PRODUCTION
  return true;  // SignatureChecker.cpp:34-36: fuzz builds accept every signature
#endif
  if (mProtocolVersion == 7) return true;  // SignatureChecker.cpp:38-41

  // the reference copies the signers into per-type vectors; the same order
  // and erase semantics over pointers (stack scratch, no allocation)
  using Ptrs = InlineVec<const Signer*, 24>;
  Ptrs byType[4];
  for (auto const& s : signersV) byType[s.key.type].push_back(&s);

  int32_t totalWeight = 0;
  for (const Signer* s : byType[SIGNER_KEY_TYPE_PRE_AUTH_TX]) {  // :54-69
    if (s->key.key == mContentsHash) {
      totalWeight += (int32_t)clampWeight(mProtocolVersion, s->weight);
      if (totalWeight >= neededWeight) return true;
    }
  }

  auto verifyAll = [&](Ptrs& signers, auto&& verify) {  // :73-102
    for (size_t i = 0; i < mSignatures.size(); i++) {
      auto const& sig = mSignatures[i];
      for (auto it = signers.begin(); it != signers.end(); ++it) {
        if (verify(sig, **it)) {
          mUsedSignatures.set(i);
          totalWeight += (int32_t)clampWeight(mProtocolVersion, (*it)->weight);
          if (totalWeight >= neededWeight) return true;
          signers.erase(it);
          break;
        }
      }
    }
    return false;
  };

  if (verifyAll(byType[SIGNER_KEY_TYPE_HASH_X], [&](DecoratedSignature const& sig, Signer const& s) {
        return SignatureUtils::verifyHashX(sig, s.key);
      }))
    return true;

  if (verifyAll(byType[SIGNER_KEY_TYPE_ED25519], [&](DecoratedSignature const& sig, Signer const& s) {
        // SignatureUtils::verify, SignatureUtils.cpp:38-46
        if (std::memcmp(s.key.key.data() + 28, sig.hint.data(), 4) != 0) return false;
        return verifyEd25519(sig, s.key.key, ByteSlice(mContentsHash.data(), 32));
      }))
    return true;

  if (verifyAll(byType[SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD], [&](DecoratedSignature const& sig, Signer const& s) {
        // SignatureUtils::verifyEd25519SignedPayload, SignatureUtils.cpp:48-61
        SignatureHint h = SignatureUtils::getSignedPayloadHint(s.key);
        if (!SignatureUtils::doesHintMatch(ByteSlice(h.data(), 4), sig.hint)) return false;
        return verifyEd25519(sig, s.key.key, ByteSlice(s.key.payload.data(), s.key.payload.size()));
      }))
    return true;

  return false;
}

bool SignatureChecker::checkAllSignaturesUsed() const {  // :138-158
#ifdef FUZZING_BUILD_MODE_UNSAFE_FOR_PRODUCTION
  return true;  // :141-143
#endif
  if (mProtocolVersion == 7) return true;
  return mUsedSignatures.all();
}

}  // namespace stellar
