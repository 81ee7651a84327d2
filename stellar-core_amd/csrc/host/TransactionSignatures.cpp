// See TransactionSignatures.h.  Restates the signature checks of
// /root/reference/src/transactions/TransactionFrame.cpp:268-321 (checkSignature,
// checkSignatureNoAccount, checkExtraSigners), :1247-1262 (commonValid),
// :1416-1486 (checkValidWithOptionallyChargedFee),
// OperationFrame.cpp:47-62,173-209 and FeeBumpTransactionFrame.cpp:138-197,267-287.
#include "TransactionSignatures.h"

#include <atomic>

#include "../../../include/stellar_sigverify.h"

namespace stellar {
namespace {

// signer lists built as std::vector<Signer> copies (signerListsBuilt())
std::atomic<uint64_t> gSignerListsBuilt{0};
// transactions of the results form that were not answered by their body's code alone (decidedWalks())
std::atomic<uint64_t> gDecidedWalks{0};

// TransactionFrame::checkSignature: master key (if its weight is non-zero)
// then the account's signers
std::vector<Signer> accountSigners(AccountSigState const& acc) {
  gSignerListsBuilt.fetch_add(1, std::memory_order_relaxed);
  std::vector<Signer> signers;
  if (acc.thresholds[0]) {
    Signer m;
    m.key.type = SIGNER_KEY_TYPE_ED25519;
    m.key.key = acc.accountID;
    m.weight = acc.thresholds[0];
    signers.push_back(m);
  }
  signers.insert(signers.end(), acc.signers.begin(), acc.signers.end());
  return signers;
}

AccountSigState const* find(AccountSnapshot const& accounts, uint256 const& id) {
  auto it = accounts.find(id);
  return it == accounts.end() ? nullptr : &it->second;
}

std::vector<Signer> extraSignerList(std::vector<SignerKey> const& keys) {
  gSignerListsBuilt.fetch_add(1, std::memory_order_relaxed);
  std::vector<Signer> signers;
  for (auto const& k : keys) {
    Signer s;
    s.key = k;
    s.weight = 1;
    signers.push_back(s);
  }
  return signers;
}

Signer noAccountSigner(uint256 const& id) {
  Signer s;
  s.key.type = SIGNER_KEY_TYPE_ED25519;
  s.key.key = id;
  s.weight = 1;
  return s;
}

// The three kinds of check as references (SignatureCheckRef): an account entry at a threshold level, the extra
// signers, and the key of an account that does not exist.
SignatureCheckRef accountRef(AccountSigState const& acc, int level) {
  return SignatureCheckRef{&acc.accountID, acc.thresholds, &acc.signers, nullptr, (uint8_t)level,
                           (int32_t)acc.thresholds[level]};
}
SignatureCheckRef extraRef(std::vector<SignerKey> const& keys) {
  return SignatureCheckRef{nullptr, nullptr, nullptr, &keys, 0, (int32_t)keys.size()};
}
SignatureCheckRef noAccountRef(uint256 const& id) { return SignatureCheckRef{&id, nullptr, nullptr, nullptr, 0, 0}; }
// an operation's check: its failure is opBAD_AUTH (the results form reads the role; every other checker ignores it)
SignatureCheckRef ofOperation(SignatureCheckRef r) {
  r.role = SV_TXROLE_OP;
  return r;
}

// ... and the list a reference stands for, as the copy the reference's checkSignature is handed
SignatureCheck materialize(SignatureCheckRef const& r) {
  if (r.extra) return SignatureCheck{extraSignerList(*r.extra), r.needed};
  if (!r.thresholds) {
    gSignerListsBuilt.fetch_add(1, std::memory_order_relaxed);
    return SignatureCheck{std::vector<Signer>{noAccountSigner(*r.id)}, r.needed};
  }
  // (accountSigners' rule over the referenced parts)
  gSignerListsBuilt.fetch_add(1, std::memory_order_relaxed);
  std::vector<Signer> signers;
  if (r.thresholds[0]) {
    signers.push_back(noAccountSigner(*r.id));  // (the master: the account's key as an ed25519 signer)
    signers.back().weight = r.thresholds[0];
  }
  signers.insert(signers.end(), r.signers->begin(), r.signers->end());
  return SignatureCheck{std::move(signers), r.needed};
}

}  // namespace

uint64_t signerListsBuilt() { return gSignerListsBuilt.load(std::memory_order_relaxed); }
uint64_t decidedWalks() { return gDecidedWalks.load(std::memory_order_relaxed); }

TxSigResult checkFeeBumpSignatures(FeeBumpSigInfo const& tx, AccountSnapshot const& accounts, uint32_t protocol,
                                   SignatureBatchPrefetch const* prefetched, bool forApply) {
  TxSigResult r;
  if (protocol < 13) {
    r.code = txNOT_SUPPORTED;
    return r;
  }
  SignatureChecker checker(protocol, tx.contentsHash, tx.signatures, prefetched);
  AccountSigState const* fee = find(accounts, tx.feeSource);
  if (!fee) {
    r.code = txNO_ACCOUNT;
    return r;
  }
  if (!checker.checkSignature(accountSigners(*fee), fee->thresholds[THRESHOLD_LOW_LEVEL])) {
    r.code = txBAD_AUTH;
    return r;
  }
  if (!checker.checkAllSignaturesUsed()) {
    r.code = txBAD_AUTH_EXTRA;
    return r;
  }
  TxSigResult inner = checkTransactionSignatures(tx.inner, accounts, protocol, prefetched, forApply);
  r.code = inner.code == txSUCCESS ? txFEE_BUMP_INNER_SUCCESS : txFEE_BUMP_INNER_FAILED;
  r.innerCode = inner.code;
  r.failedOp = inner.failedOp;
  r.opCode = inner.opCode;
  return r;
}

namespace {

// The sequence of checks of one transaction -- the one copy of it -- over any
// checker: check(SignatureCheckRef) -> bool, allUsed() -> bool.  A SignatureChecker
// (checkTransactionSignatures), the lists (listTransactionChecks, listTransactionCheckRefs) and the engine's
// decisions (checkTransactionSignaturesDecided, ...DecidedRefs) all walk it; byList adapts a checker that wants
// the signer list as a copy.
template <class Check, class AllUsed>
TxSigResult walkTransaction(TransactionSigInfo const& tx, AccountSnapshot const& accounts, uint32_t protocol,
                            bool forApply, Check&& check, AllUsed&& allUsed) {
  TxSigResult r;
  AccountSigState const* src = find(accounts, tx.sourceAccount);
  if (!src) {  // commonValidPreSeqNum
    r.code = txNO_ACCOUNT;
    return r;
  }
  if (!check(accountRef(*src, THRESHOLD_LOW_LEVEL))) {
    r.code = txBAD_AUTH;
    return r;
  }
  if (protocol >= 19 && !tx.extraSigners.empty() && !check(extraRef(tx.extraSigners))) {
    r.code = txBAD_AUTH;
    return r;
  }
  if (forApply && protocol < 10) return r;  // processSignatures, TransactionFrame.cpp:1100-1103
  for (size_t i = 0; i < tx.operations.size(); ++i) {
    auto const& op = tx.operations[i];
    uint256 const& id = op.sourceAccount ? *op.sourceAccount : tx.sourceAccount;
    AccountSigState const* acc = find(accounts, id);
    bool ok;
    int32_t opc = opINNER;
    if (acc) {
      ok = check(ofOperation(accountRef(*acc, op.level)));
      if (!ok) opc = opBAD_AUTH;
    } else if (!op.sourceAccount) {
      // (processSignatures calls OperationFrame::checkSignature with
      // forApply = false, TransactionFrame.cpp:1130-1131: a missing op-source
      // account is checked by its key alone in BOTH modes; only a missing
      // transaction source gives opNO_ACCOUNT, OperationFrame.cpp:194-198)
      ok = false;
      opc = opNO_ACCOUNT;
    } else {
      ok = check(ofOperation(noAccountRef(id)));
      if (!ok) opc = opBAD_AUTH;
    }
    if (!ok && r.code != txFAILED) {
      r.code = txFAILED;
      r.failedOp = (int32_t)i;
      r.opCode = opc;
      if (!forApply) return r;  // checkValid fast-fails on the first invalid operation
    }
  }
  if (r.code == txFAILED) return r;
  if (!allUsed()) r.code = txBAD_AUTH_EXTRA;
  return r;
}

template <class F>
auto byList(F&& fn) {
  return [&fn](SignatureCheckRef const& r) {
    SignatureCheck c = materialize(r);
    return fn(c.signers, c.needed);
  };
}

// A checker that consumes the engine's decisions of one body in order.
class DecidedChecker {
 public:
  DecidedChecker(uint32_t protocol, std::vector<DecoratedSignature> const& signatures,
                 SignatureBatchPrefetch const& pre, size_t body)
      : mProtocol(protocol), mSignatures(signatures), mPre(pre), mBody(body) {}
  bool check(std::vector<Signer> const& signers, int32_t needed) {
    const SignatureBatchPrefetch::Decision d = mPre.decision(mBody, mNext++);
    mUsed |= d.used;
    if (d.ok) return true;
    if (mPre.decidedFinal()) return false;  // (the engine ran the signed-payload stage too)
    // the reference's last stage, from the state the engine's three left
    std::vector<Signer const*> rest;
    for (auto const& s : signers)
      if (s.key.type == SIGNER_KEY_TYPE_ED25519_SIGNED_PAYLOAD) rest.push_back(&s);
    if (rest.empty()) return false;
    int64_t total = d.weight;
    for (size_t i = 0; i < mSignatures.size(); ++i)
      for (auto it = rest.begin(); it != rest.end(); ++it)
        if (SignatureUtils::verifyEd25519SignedPayload(mSignatures[i], (*it)->key)) {
          mUsed |= 1ull << i;
          const uint32_t w = (*it)->weight;
          total += mProtocol >= 10 && w > 255 ? 255 : w;
          if (total >= needed) return true;
          rest.erase(it);
          break;
        }
    return false;
  }
  // a final decision (decidedFinal()): nothing but the decision is looked at
  bool checkFinal() {
    const SignatureBatchPrefetch::Decision d = mPre.decision(mBody, mNext++);
    mUsed |= d.used;
    return d.ok;
  }
  bool allUsed() const {
    const size_t n = mSignatures.size();
    const uint64_t want = n >= 64 ? ~0ull : (1ull << n) - 1;
    return (mUsed & want) == want;
  }

 private:
  uint32_t mProtocol;
  std::vector<DecoratedSignature> const& mSignatures;
  SignatureBatchPrefetch const& mPre;
  size_t mBody, mNext = 0;
  uint64_t mUsed = 0;
};

}  // namespace

TxSigResult checkTransactionSignatures(TransactionSigInfo const& tx, AccountSnapshot const& accounts,
                                       uint32_t protocol, SignatureBatchPrefetch const* prefetched, bool forApply) {
  SignatureChecker checker(protocol, tx.contentsHash, tx.signatures, prefetched);
  auto check = [&](std::vector<Signer> const& signers, int32_t needed) {
    return checker.checkSignature(signers, needed);
  };
  return walkTransaction(tx, accounts, protocol, forApply, byList(check),
                         [&] { return checker.checkAllSignaturesUsed(); });
}

std::vector<SignatureCheck> listTransactionChecks(TransactionSigInfo const& tx, AccountSnapshot const& accounts,
                                                  uint32_t protocol, bool forApply) {
  std::vector<SignatureCheck> out;
  (void)walkTransaction(
      tx, accounts, protocol, forApply,
      [&](SignatureCheckRef const& r) {
        out.push_back(materialize(r));
        return true;
      },
      [] { return true; });
  return out;
}

std::vector<SignatureCheckRef> listTransactionCheckRefs(TransactionSigInfo const& tx, AccountSnapshot const& accounts,
                                                        uint32_t protocol, bool forApply) {
  std::vector<SignatureCheckRef> out;
  (void)walkTransaction(
      tx, accounts, protocol, forApply,
      [&](SignatureCheckRef const& r) {
        out.push_back(r);
        return true;
      },
      [] { return true; });
  return out;
}

TxSigResult listTransactionCheckRefs(TransactionSigInfo const& tx, AccountSnapshot const& accounts, uint32_t protocol,
                                     bool forApply, std::vector<SignatureCheckRef>& out) {
  out.clear();
  return walkTransaction(
      tx, accounts, protocol, forApply,
      [&](SignatureCheckRef const& r) {
        out.push_back(r);
        return true;
      },
      [] { return true; });
}

std::vector<SignatureCheckRef> listFeeBumpOuterCheckRefs(FeeBumpSigInfo const& tx, AccountSnapshot const& accounts) {
  std::vector<SignatureCheckRef> out;
  if (AccountSigState const* fee = find(accounts, tx.feeSource)) out.push_back(accountRef(*fee, THRESHOLD_LOW_LEVEL));
  return out;
}

std::vector<SignatureCheck> listFeeBumpOuterChecks(FeeBumpSigInfo const& tx, AccountSnapshot const& accounts) {
  std::vector<SignatureCheck> out;
  if (AccountSigState const* fee = find(accounts, tx.feeSource))
    out.push_back(SignatureCheck{accountSigners(*fee), (int32_t)fee->thresholds[THRESHOLD_LOW_LEVEL]});
  return out;
}

TxSigResult checkTransactionSignaturesDecided(TransactionSigInfo const& tx, AccountSnapshot const& accounts,
                                              uint32_t protocol, SignatureBatchPrefetch const& pre, size_t body,
                                              bool forApply) {
  DecidedChecker checker(protocol, tx.signatures, pre, body);
  auto check = [&](std::vector<Signer> const& signers, int32_t needed) { return checker.check(signers, needed); };
  return walkTransaction(tx, accounts, protocol, forApply, byList(check), [&] { return checker.allUsed(); });
}

TxSigResult checkTransactionSignaturesDecidedRefs(TransactionSigInfo const& tx, AccountSnapshot const& accounts,
                                                  uint32_t protocol, SignatureBatchPrefetch const& pre, size_t body,
                                                  bool forApply) {
  DecidedChecker checker(protocol, tx.signatures, pre, body);
  return walkTransaction(
      tx, accounts, protocol, forApply, [&](SignatureCheckRef const&) { return checker.checkFinal(); },
      [&] { return checker.allUsed(); });
}

TxSigResult checkFeeBumpSignaturesDecidedRefs(FeeBumpSigInfo const& tx, AccountSnapshot const& accounts,
                                              uint32_t protocol, SignatureBatchPrefetch const& pre, size_t outerBody,
                                              size_t innerBody, bool forApply) {
  TxSigResult r;
  if (protocol < 13) {
    r.code = txNOT_SUPPORTED;
    return r;
  }
  DecidedChecker checker(protocol, tx.signatures, pre, outerBody);
  if (!find(accounts, tx.feeSource)) {
    r.code = txNO_ACCOUNT;
    return r;
  }
  if (!checker.checkFinal()) {
    r.code = txBAD_AUTH;
    return r;
  }
  if (!checker.allUsed()) {
    r.code = txBAD_AUTH_EXTRA;
    return r;
  }
  TxSigResult inner = checkTransactionSignaturesDecidedRefs(tx.inner, accounts, protocol, pre, innerBody, forApply);
  r.code = inner.code == txSUCCESS ? txFEE_BUMP_INNER_SUCCESS : txFEE_BUMP_INNER_FAILED;
  r.innerCode = inner.code;
  r.failedOp = inner.failedOp;
  r.opCode = inner.opCode;
  return r;
}

TxSigResult checkTransactionSignaturesResults(TransactionSigInfo const& tx, AccountSnapshot const& accounts,
                                              uint32_t protocol, SignatureBatchPrefetch const& pre, size_t body,
                                              bool forApply) {
  const SignatureBatchPrefetch::BodyResult b = pre.bodyResult(body);
  // every check passed, every signature was used (or nobody asks), and the listing met no missing account
  if (b.code == SV_TXRESULT_OK && b.listedOk) return TxSigResult();
  // The first failure decides the walk: with check i false exactly for i = fail it takes the path the decisions
  // themselves would have led it along (a later false check changes nothing once one has failed).
  gDecidedWalks.fetch_add(1, std::memory_order_relaxed);
  size_t next = 0;
  return walkTransaction(
      tx, accounts, protocol, forApply, [&](SignatureCheckRef const&) { return next++ != (size_t)b.fail; },
      [&] { return b.code != SV_TXRESULT_BAD_AUTH_EXTRA; });
}

TxSigResult checkFeeBumpSignaturesResults(FeeBumpSigInfo const& tx, AccountSnapshot const& accounts,
                                          uint32_t protocol, SignatureBatchPrefetch const& pre, size_t outerBody,
                                          size_t innerBody, bool forApply) {
  TxSigResult r;
  auto failed = [&](int32_t code) {
    gDecidedWalks.fetch_add(1, std::memory_order_relaxed);
    r.code = code;
    return r;
  };
  if (protocol < 13) return failed(txNOT_SUPPORTED);
  if (!find(accounts, tx.feeSource)) return failed(txNO_ACCOUNT);
  // the outer body: the fee source at LOW (role TX), then "every outer signature used"
  const SignatureBatchPrefetch::BodyResult outer = pre.bodyResult(outerBody);
  if (outer.code == SV_TXRESULT_BAD_AUTH_EXTRA) return failed(txBAD_AUTH_EXTRA);
  if (outer.code != SV_TXRESULT_OK) return failed(txBAD_AUTH);
  TxSigResult inner = checkTransactionSignaturesResults(tx.inner, accounts, protocol, pre, innerBody, forApply);
  r.code = inner.code == txSUCCESS ? txFEE_BUMP_INNER_SUCCESS : txFEE_BUMP_INNER_FAILED;
  r.innerCode = inner.code;
  r.failedOp = inner.failedOp;
  r.opCode = inner.opCode;
  return r;
}

TxSigResult checkFeeBumpSignaturesDecided(FeeBumpSigInfo const& tx, AccountSnapshot const& accounts,
                                          uint32_t protocol, SignatureBatchPrefetch const& pre, size_t outerBody,
                                          size_t innerBody, bool forApply) {
  TxSigResult r;
  if (protocol < 13) {
    r.code = txNOT_SUPPORTED;
    return r;
  }
  DecidedChecker checker(protocol, tx.signatures, pre, outerBody);
  AccountSigState const* fee = find(accounts, tx.feeSource);
  if (!fee) {
    r.code = txNO_ACCOUNT;
    return r;
  }
  if (!checker.check(accountSigners(*fee), (int32_t)fee->thresholds[THRESHOLD_LOW_LEVEL])) {
    r.code = txBAD_AUTH;
    return r;
  }
  if (!checker.allUsed()) {
    r.code = txBAD_AUTH_EXTRA;
    return r;
  }
  TxSigResult inner = checkTransactionSignaturesDecided(tx.inner, accounts, protocol, pre, innerBody, forApply);
  r.code = inner.code == txSUCCESS ? txFEE_BUMP_INNER_SUCCESS : txFEE_BUMP_INNER_FAILED;
  r.innerCode = inner.code;
  r.failedOp = inner.failedOp;
  r.opCode = inner.opCode;
  return r;
}

void prefetchTransaction(SignatureBatchPrefetch& pre, TransactionSigInfo const& tx, AccountSnapshot const& accounts,
                         SignatureBatchPrefetch::TxBody const* body, bool hinted) {
  std::vector<Signer> all;
  auto addAccount = [&](uint256 const& id, bool noAccountKey) {
    if (AccountSigState const* a = find(accounts, id)) {
      auto s = accountSigners(*a);
      all.insert(all.end(), s.begin(), s.end());
    } else if (noAccountKey) {
      all.push_back(noAccountSigner(id));
    }
  };
  addAccount(tx.sourceAccount, false);
  for (auto const& op : tx.operations)
    if (op.sourceAccount) addAccount(*op.sourceAccount, true);
  auto extra = extraSignerList(tx.extraSigners);
  all.insert(all.end(), extra.begin(), extra.end());
  // the same (key, payload) reached twice would only duplicate pairs
  std::vector<Signer> uniq;
  for (auto const& s : all) {
    bool dup = false;
    for (auto const& u : uniq)
      if (u.key.type == s.key.type && u.key.key == s.key.key && u.key.payload == s.key.payload) {
        dup = true;
        break;
      }
    if (!dup) uniq.push_back(s);
  }
  if (body && hinted) pre.addHinted(*body, tx.signatures, uniq);
  else if (body) pre.add(*body, tx.signatures, uniq);
  else pre.add(tx.contentsHash, tx.signatures, uniq);
}

void prefetchFeeBump(SignatureBatchPrefetch& pre, FeeBumpSigInfo const& tx, AccountSnapshot const& accounts,
                     SignatureBatchPrefetch::TxBody const* outerBody, SignatureBatchPrefetch::TxBody const* innerBody,
                     bool hinted) {
  // (body form: the outer body is added even without a fee-source account, so its hash is still computed)
  AccountSigState const* a = find(accounts, tx.feeSource);
  if (outerBody && hinted) pre.addHinted(*outerBody, tx.signatures, a ? accountSigners(*a) : std::vector<Signer>());
  else if (outerBody) pre.add(*outerBody, tx.signatures, a ? accountSigners(*a) : std::vector<Signer>());
  else if (a) pre.add(tx.contentsHash, tx.signatures, accountSigners(*a));
  prefetchTransaction(pre, tx.inner, accounts, innerBody, hinted);
}

}  // namespace stellar
