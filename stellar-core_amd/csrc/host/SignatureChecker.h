// Restatement of stellar-core's multisig signature checker with a GPU batch
// pre-pass.
//
// Reference:
//   SignatureChecker      /root/reference/src/transactions/SignatureChecker.h:18-39,
//                         SignatureChecker.cpp:20-158
//   SignatureUtils        /root/reference/src/transactions/SignatureUtils.cpp:30-61 (verify,
//                         verifyEd25519SignedPayload), :86-93 (verifyHashX),
//                         :95-136 (getSignedPayloadHint, getHint, doesHintMatch)
//
// The checker's decision logic is unchanged (greedy weight accumulation in
// the order PRE_AUTH_TX, HASH_X, ED25519, ED25519_SIGNED_PAYLOAD; a matching
// signer is erased; weight clamped to 255 from protocol 10; protocol 7 always
// passes).  What is new is SignatureBatchPrefetch: it enumerates every
// hint-matching (signature, signer) pair of MANY transactions (a tx set,
// TxSetFrame.cpp:427-457, or a ledger being applied, LedgerManagerImpl.cpp:
// 1582-1648), verifies them in one GPU batch, and hands the verdicts to the
// checkers as a side table -- so the per-tx checkers never wait on the GPU
// one signature at a time, and the 0xffff-entry global cache cannot evict a
// verdict before it is used.  The side table is keyed by the (pk, sig, msg)
// bytes themselves (a cheap hash of them, full compare on lookup), not by the
// BLAKE2b cache key, so a checker's lookup costs no hashing.
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <unordered_map>
#include <utility>
#include <vector>

#include "PubKeyUtils.h"

namespace stellar {

enum SignerKeyType : int32_t {
  SIGNER_KEY_TYPE_ED25519 = 0,
  SIGNER_KEY_TYPE_PRE_AUTH_TX = 1,
  SIGNER_KEY_TYPE_HASH_X = 2,
  SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD = 3,
};

struct SignerKey {
  SignerKeyType type = SIGNER_KEY_TYPE_ED25519;
  uint256 key{};                 // ed25519 / preAuthTx / hashX / signedPayload.ed25519
  std::vector<uint8_t> payload;  // signedPayload.payload (<= 64 bytes)
};

struct Signer {
  SignerKey key;
  uint32_t weight = 0;
};

using SignatureHint = std::array<uint8_t, 4>;

struct DecoratedSignature {
  SignatureHint hint{};
  Signature signature;
};

namespace SignatureUtils {
SignatureHint getHint(ByteSlice const& bs);
bool doesHintMatch(ByteSlice const& bs, SignatureHint const& hint);
SignatureHint getSignedPayloadHint(SignerKey const& signedPayloadSigner);
// SignatureUtils::verify / verifyHashX / verifyEd25519SignedPayload
bool verify(DecoratedSignature const& sig, SignerKey const& signerKey, Hash const& hash);
bool verifyHashX(DecoratedSignature const& sig, SignerKey const& signerKey);
bool verifyEd25519SignedPayload(DecoratedSignature const& sig, SignerKey const& signer);
}  // namespace SignatureUtils

// One checkSignature call: a signer list and the needed weight.
struct SignatureCheck {
  std::vector<Signer> signers;
  int32_t needed = 0;
};

// One checkSignature call by reference -- nothing is copied.  A ledger account: `id` its account ID, `thresholds`
// its four threshold bytes, `signers` its signer list, `level` 1..3 (needed = thresholds[level]).  The key of an
// account that does not exist (checkSignatureNoAccount): `id` alone, level 0, needed 0.  The extra signers
// (checkExtraSigners): `extra`, level 0, needed = their count.  `role` says whose failure a failing check is
// (include/stellar_sigverify.h SV_TXROLE_*): 0 the transaction's (txBAD_AUTH: the source account, the extra
// signers, a fee bump's fee source), 1 an operation's (opBAD_AUTH); only the results form reads it.
struct SignatureCheckRef {
  uint256 const* id;
  uint8_t const* thresholds;
  std::vector<Signer> const* signers;
  std::vector<SignerKey> const* extra;
  uint8_t level;
  int32_t needed;
  uint8_t role = 0;
};

// Verdicts computed ahead of the checkers.
class SignatureBatchPrefetch {
 public:
  // Storage is taken from (and on destruction returned to) per-thread
  // spares, so a node building one prefetch per ledger reuses mapped pages
  // instead of faulting in fresh ones every time (measured: page faults of
  // freshly grown buffers were most of the cost of add() on a 30k-pair set).
  SignatureBatchPrefetch();
  ~SignatureBatchPrefetch();
  SignatureBatchPrefetch(SignatureBatchPrefetch const&) = delete;
  SignatureBatchPrefetch& operator=(SignatureBatchPrefetch const&) = delete;
  // Enumerate the hint-matching ed25519 / signed-payload pairs of one tx.
  void add(Hash const& contentsHash, std::vector<DecoratedSignature> const& signatures,
           std::vector<Signer> const& signers);
  // The same for a whole set of transactions, enumerated in parallel on the
  // host pool (pairs in tx order, as add() per tx would give them).  The
  // pairs of batch tx k are then also found by their position: a checker
  // constructed with prefetchTx = k (the index in txs, counted over every
  // addBatch call of this prefetch) searches them before the table.
  struct TxRef {
    Hash const* contentsHash;
    std::vector<DecoratedSignature> const* signatures;
    std::vector<Signer> const* signers;
  };
  // prepare (optional): called as prepare(k) for batch tx k on the thread that
  // enumerates it, just before, to build the tx's objects in place (the
  // tx-set entry point marshals its C structs there: one pass over each tx,
  // its objects still in that core's cache).  An exception thrown by it is
  // rethrown here once every part has finished.
  void addBatch(std::vector<TxRef> const& txs, std::function<void(size_t)> const& prepare = {});
  // One engine batch over everything added.  seedCache = false: the verdicts
  // go to the side table only (the engine is called directly, no cache
  // interaction); true: through PubKeyUtils::verifySigBatch, which also fills
  // the global verify cache (a later verifySig then hits).  An engine error
  // re-runs the batch on the CPU path.
  void run(bool seedCache = false);
  // Body form (catchup replay: every frame is fresh, so nobody has hashed it
  // yet).  add(TxBody, ...) enumerates a transaction's pairs without knowing
  // its contents hash: the hash is that of the body, prefix || bytes with the
  // kind's prefix (include/stellar_sigverify.h SV_TXBODY_*), off / len a range
  // of the blob given to runBodies.  runBodies sends every ed25519 pair and
  // every body to the engine in one sv_ed25519_verify_txbodies call, stores the
  // digests that come back through hashOut and into the pairs' message bytes,
  // verifies the signed-payload pairs (which carry their own message) as a
  // second, normally empty, batch, and builds the side table: lookups then work
  // as after run(false).  A prefetch takes either form, not both.
  struct TxBody {
    uint64_t off;
    uint32_t len;
    uint8_t kind;
    Hash* hashOut;
  };
  void add(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
           std::vector<Signer> const& signers);
  void runBodies(const uint8_t* networkID, const uint8_t* blob);
  // Hinted body form: the pairing by hint is the engine's too.  addHinted makes
  // one pass over the transaction and compares no hint: every 64-byte signature
  // goes in with its hint (other lengths are skipped, as add() skips them),
  // every ed25519 signer's key goes in as a candidate.  Signed-payload signers
  // are still enumerated here (their hint is XORed with the payload's, their
  // message is the payload): they stay the second, normally empty, batch.
  // runBodiesHinted makes ONE sv_ed25519_verify_txbodies_hinted call (an engine
  // error re-runs it on the _cpu form and counts a fallback), fills the pair
  // storage from the returned indices -- body t's pairs are then also found by
  // position (prefetchTx = t, counted over the addHinted calls) -- stores the
  // digests through hashOut and builds the side table as runBodies does.
  // lookup() is unchanged.  A prefetch takes one of the three forms only.
  void addHinted(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
                 std::vector<Signer> const& signers);
  void runBodiesHinted(const uint8_t* networkID, const uint8_t* blob);
  // Decided form: not verdicts but decisions.  addDecided takes a transaction
  // body, its signatures (every length up to 64) and the checkSignature calls
  // its validation makes, in order; runDecided makes ONE
  // sv_ed25519_check_txbodies call (an engine error re-runs it on the _cpu form
  // and counts a fallback) and stores the digests through hashOut.  No pair
  // storage and no table are built: decision(body, k) is check k of the
  // addDecided call number `body` -- did it reach its needed weight within the
  // PRE_AUTH_TX / HASH_X / ED25519 stages, the weight those stages accumulated
  // and the signatures they marked used.  Signed-payload signers stay with the
  // caller (they are not sent).  addDecided returns false, adding nothing, for
  // what the engine does not take: more than 64 signatures, a signature longer
  // than 64 bytes, a check with more than 64 signers.  With withPayload (every
  // addDecided call of a prefetch, or none) the signed-payload signers go to
  // the engine too, as the body's payload candidates (sv_txchecks_payload:
  // distinct (key, payload) rows; a payload longer than 64 bytes is not
  // taken): the decisions are then those of all four stages and final
  // (decidedFinal()), with nothing left to the caller.  A prefetch takes one
  // form only.
  struct Decision {
    bool ok;
    uint32_t weight;
    uint64_t used;
  };
  bool addDecided(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
                  std::vector<SignatureCheck> const& checks, bool withPayload = false);
  bool decidedFinal() const { return dec_.payload; }
  void runDecided(const uint8_t* networkID, const uint8_t* blob, uint32_t protocolVersion);
  Decision decision(size_t body, size_t check) const;
  // By-account form of the decided form (include/stellar_sigverify.h sv_txaccounts): the checks come as
  // references.  addDecidedRefs puts every ledger account a check names into the prefetch's account table ONCE,
  // found again by its account ID (a pseudo-account -- a missing source's key, the extra signers -- is a row of
  // its own each time), lists the body's accounts and stores (account position, level, needed) per check; no
  // signer list is copied per check or per body.  It returns false, adding nothing, beyond the engine's limits:
  // more than 64 signatures, a signature or payload longer than 64 bytes, an account whose list (master included)
  // exceeds 64 signers.  runDecidedRefs makes ONE sv_ed25519_check_txbodies_accounts call (an engine error re-runs
  // it on the _cpu form and counts a fallback, never a reject); decision() then works as after runDecided, and
  // every decision is final (decidedFinal()): signed-payload signers are in the table.  A prefetch takes one
  // form only.
  // Results form of the by-account form (sv_txresults): addDecidedRefs also records every check's role and, per
  // body, skipUnused (the walk that listed the checks never asks "was every signature used":
  // processSignatures below protocol 10) and listedOk (that walk, with every check true, ended in success -- it
  // met no txNO_ACCOUNT / opNO_ACCOUNT).  runDecidedResults makes ONE sv_ed25519_decide_txbodies_accounts call
  // that requests no per-check output (an engine error re-runs it on the _cpu form and counts a fallback, never a
  // reject); bodyResult(body) is then the body's code, its first failing check and listedOk.  decision() is not
  // available after it.
  bool addDecidedRefs(TxBody const& body, std::vector<DecoratedSignature> const& signatures,
                      std::vector<SignatureCheckRef> const& checks, bool skipUnused = false, bool listedOk = true);
  void runDecidedRefs(const uint8_t* networkID, const uint8_t* blob, uint32_t protocolVersion);
  struct BodyResult {
    uint8_t code;   // SV_TXRESULT_*
    uint32_t fail;  // body-local index of the first failing check, SV_TXRESULT_NONE: none
    bool listedOk;
  };
  void runDecidedResults(const uint8_t* networkID, const uint8_t* blob, uint32_t protocolVersion);
  BodyResult bodyResult(size_t body) const;
  size_t decidedAccounts() const { return acct_.thr.size() / 4; }
  size_t decidedChecks() const { return dec_.needed.size(); }
  // verdict for (pk, sig, msg) if prefetched (tx: see addBatch)
  static constexpr size_t kNoTx = ~size_t(0);
  bool lookup(uint256 const& pk, Signature const& sig, ByteSlice const& msg, bool& verdict,
              size_t tx = kNoTx) const;
  size_t pairs() const { return len_.size(); }
  // verdicts that were 1, after a run (measurement and tests)
  size_t accepted() const {
    size_t a = 0;
    for (uint8_t v : verdict_) a += v != 0;
    return a;
  }

 private:
  void buildTable();
  static constexpr size_t kAsyncTableMin = 4096;
  static uint64_t hashOf(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t len);
  // (growth without zero-filling: every byte of the pair arrays is written
  // right after the resize that makes room for it)
  template <typename T>
  struct NoInit : std::allocator<T> {
    template <typename U>
    struct rebind {
      using other = NoInit<U>;
    };
    NoInit() = default;
    template <typename U>
    NoInit(NoInit<U> const&) {}
    template <typename U>
    void construct(U* p) {
      ::new ((void*)p) U;
    }
    template <typename U, typename... A>
    void construct(U* p, A&&... a) {
      ::new ((void*)p) U(std::forward<A>(a)...);
    }
  };
  template <typename T>
  using RawVec = std::vector<T, NoInit<T>>;
  struct Storage {
    RawVec<uint8_t> pk, sig, msg;
    RawVec<uint8_t> hhint, hsig, hkey;  // hinted body form: what goes to the engine (hints, signatures, keys)
    RawVec<uint64_t> off;
    RawVec<uint32_t> len;
    std::vector<uint8_t> verdict;
    std::vector<uint32_t> table;    // open addressing: pair index + 1, 0 = empty
    std::vector<uint32_t> txBegin;  // addBatch: first pair of batch tx k (k + 1 entries)
    void clear();
  };
  // returns where the contents hash was stored in st.msg (~0: no ed25519 pair)
  static uint64_t enumerate(Storage& st, Hash const& contentsHash, std::vector<DecoratedSignature> const& signatures,
                            std::vector<Signer> const& signers);
  struct BodyEntry {
    TxBody body;
    size_t pair0, pair1;  // the pairs enumerated for it
    uint64_t hashOff;     // its contents hash in msg_ (~0: none)
  };
  std::vector<BodyEntry> bodies_;
  struct Decided {  // the decided form's tables (include/stellar_sigverify.h sv_txchecks) and results
    std::vector<uint8_t> hint, sig, sigLen, key, type, ok;
    std::vector<uint64_t> sigBegin{0}, keyBegin{0}, checkBegin{0}, signerBegin{0}, used;
    std::vector<int32_t> needed;
    std::vector<uint32_t> weight, keyIndex, outWeight;
    // withPayload: the payload candidates (sv_txchecks_payload)
    bool payload = false;
    std::vector<uint64_t> pkeyBegin{0};
    std::vector<uint8_t> pkey, pkeyPayload, pkeyLen;
    // results form: roles per check; flags, the listing's outcome and the results per body
    std::vector<uint8_t> role, bodyFlags, listedOk, bodyCode;
    std::vector<uint32_t> bodyFail;
  } dec_;
  struct IdHash {
    size_t operator()(uint256 const& k) const {
      size_t v;
      std::memcpy(&v, k.data(), sizeof v);
      return v;
    }
  };
  struct Accounts {  // the by-account form's tables (sv_txaccounts); signatures, needed and results live in dec_
    std::vector<uint8_t> key, thr, stype, skey, pay, plen, clevel;
    std::vector<uint64_t> sbeg{0}, bacctBegin{0};
    std::vector<uint32_t> sweight, spay, bacct, cacct;
    std::unordered_map<uint256, uint32_t, IdHash> byId;  // ledger accounts already in the table
  } acct_;
  struct AccountsCall;  // the arguments of one by-account engine call over dec_ / acct_
  void fillAccountsCall(AccountsCall& c, uint32_t protocolVersion) const;
  uint32_t appendAccount(uint256 const* id, uint8_t const* thresholds, std::vector<Signer> const* signers,
                         std::vector<SignerKey> const* extra);
  std::vector<uint64_t> hSigBegin_{0}, hKeyBegin_{0};  // hinted body form: CSR by body, in addHinted order
  static std::vector<Storage>& spares();
  static constexpr size_t kSpares = 4;
  Storage st_;
  RawVec<uint8_t>& pk_ = st_.pk;
  RawVec<uint8_t>& sig_ = st_.sig;
  RawVec<uint8_t>& msg_ = st_.msg;
  RawVec<uint8_t>& hHint_ = st_.hhint;
  RawVec<uint8_t>& hSig_ = st_.hsig;
  RawVec<uint8_t>& hKey_ = st_.hkey;
  RawVec<uint64_t>& off_ = st_.off;
  RawVec<uint32_t>& len_ = st_.len;
  std::vector<uint8_t>& verdict_ = st_.verdict;
  std::vector<uint32_t>& table_ = st_.table;
  std::vector<uint32_t>& txBegin_ = st_.txBegin;
  size_t mask_ = 0;
};

class SignatureChecker {
 public:
  // prefetchTx: the tx's index in the prefetch's addBatch order (its pairs
  // are then found by position), or kNoTx
  SignatureChecker(uint32_t protocolVersion, Hash const& contentsHash,
                   std::vector<DecoratedSignature> const& signatures,
                   SignatureBatchPrefetch const* prefetched = nullptr,
                   size_t prefetchTx = SignatureBatchPrefetch::kNoTx);
  bool checkSignature(std::vector<Signer> const& signersV, int32_t neededWeight);
  bool checkAllSignaturesUsed() const;

 private:
  bool verifyEd25519(DecoratedSignature const& sig, uint256 const& key, ByteSlice const& msg) const;

  uint32_t mProtocolVersion;
  Hash const& mContentsHash;
  std::vector<DecoratedSignature> const& mSignatures;
  // which signatures a match used (the reference's std::vector<bool>); a tx
  // carries at most 20 (xvector<DecoratedSignature, 20>), so the bits live
  // inline and a checker allocates nothing -- one malloc per tx was ~15 % of
  // the pre-passed checkers' time (profiles/r06/config3/)
  class UsedBits {
   public:
    explicit UsedBits(size_t n) : n_(n) {
      if (n > kInline) heap_.assign((n + 63) / 64, 0);
    }
    void set(size_t i) { words()[i >> 6] |= 1ull << (i & 63); }
    bool all() const {
      const uint64_t* w = heap_.empty() ? inline_ : heap_.data();
      for (size_t i = 0; i < n_; i += 64) {
        const size_t k = n_ - i < 64 ? n_ - i : 64;
        const uint64_t want = k == 64 ? ~0ull : ((1ull << k) - 1);
        if ((w[i >> 6] & want) != want) return false;
      }
      return true;
    }

   private:
    static constexpr size_t kInline = 128;
    uint64_t* words() { return heap_.empty() ? inline_ : heap_.data(); }
    size_t n_;
    uint64_t inline_[kInline / 64] = {0, 0};
    std::vector<uint64_t> heap_;
  };
  UsedBits mUsedSignatures;
  SignatureBatchPrefetch const* mPrefetched;
  size_t mPrefetchTx;
};

}  // namespace stellar
