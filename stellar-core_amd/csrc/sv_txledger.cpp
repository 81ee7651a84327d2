// Host side of the ledger forms (include/stellar_sigverify.h sv_txledger): the
// process's account store (acctstore.h); the expansion of a ledger call into
// its by-account twin's input over the store's HOST copy, which the CPU forms
// run the twin's CPU path on; and the resolve of a host-buffer call's entries
// into replica rows and their counts on the host index.  Built without the HIP
// headers, like sv_cpu.cpp: nothing here touches a device.  The exported entry
// points are sv_api.cpp's, which owns the error string.
#include "sv_txledger.h"

#include <algorithm>
#include <array>
#include <exception>
#include <map>
#include <thread>

namespace sv {

AcctStore& acct_store() {
  static AcctStore s;
  return s;
}

int ledger_combine(const sv_txledger* L, LedgerCombined* out) {
  AcctStore& S = acct_store();
  if (!L || L->struct_size < sizeof(sv_txledger) || !L->accts || L->accts->struct_size < sizeof(sv_txaccounts))
    return SV_ERR_INVALID_ARG;
  const sv_txaccounts& A = *L->accts;
  const size_t nl = A.n_accounts, ne = A.n_bacct;
  if ((uint64_t)ne >> 32 || (ne && !A.bacct)) return SV_ERR_INVALID_ARG;
  const AcctRows local{A.acct_key,        A.acct_thresholds, A.asigner_begin, A.asigner_type, A.asigner_weight,
                       A.asigner_key,     A.asigner_payload, A.apayload,      A.apayload_len, nl,
                       A.n_asigners,      A.n_apayloads};
  auto held = S.reader();  // (the store cannot change under the expansion)
  if (!S.on() || nl > S.local_accounts() || AcctStore::check_rows(local, kAcctStride) != kAsOk)
    return SV_ERR_INVALID_ARG;
  try {
    AcctCsr& c = out->table;
    // the local accounts first, their payload table as it is
    const size_t ns = nl ? (size_t)A.asigner_begin[nl] : 0, np = nl ? A.n_apayloads : 0;
    if (nl) {
      c.key.assign(A.acct_key, A.acct_key + 32 * nl);
      c.thr.assign(A.acct_thresholds, A.acct_thresholds + 4 * nl);
      c.sbeg.assign(A.asigner_begin, A.asigner_begin + nl + 1);
    }
    if (ns) {
      c.stype.assign(A.asigner_type, A.asigner_type + ns);
      c.sweight.assign(A.asigner_weight, A.asigner_weight + ns);
      c.skey.assign(A.asigner_key, A.asigner_key + 32 * ns);
      if (A.asigner_payload) c.spay.assign(A.asigner_payload, A.asigner_payload + ns);
      else c.spay.assign(ns, 0);
    }
    if (np) {
      c.pay.assign(A.apayload, A.apayload + 64 * np);
      c.plen.assign(A.apayload_len, A.apayload_len + np);
    }
    // then every store account the call names, once
    out->bacct.resize(ne + 1);
    out->found.assign(ne, 0);
    std::map<std::array<uint8_t, 32>, uint32_t> seen;
    for (size_t e = 0; e < ne; ++e) {
      const uint32_t b = A.bacct[e];
      if (b != SV_BACCT_BY_ID) {
        if (b >= nl) return SV_ERR_INVALID_ARG;
        out->bacct[e] = b;
        out->found[e] = 1;
        continue;
      }
      if (!L->bacct_id) return SV_ERR_INVALID_ARG;
      std::array<uint8_t, 32> id;
      std::memcpy(id.data(), L->bacct_id + 32 * e, 32);
      auto it = seen.find(id);
      if (it == seen.end()) {
        const uint32_t at = (uint32_t)c.accounts();
        const bool found = S.append_csr(id.data(), &c);
        it = seen.emplace(id, at | (found ? 0x80000000u : 0u)).first;
      }
      out->bacct[e] = it->second & 0x7FFFFFFFu;
      out->found[e] = (uint8_t)(it->second >> 31);
    }
    c.key.push_back(0), c.thr.push_back(0), c.stype.push_back(0), c.sweight.push_back(0), c.skey.push_back(0);
    c.spay.push_back(0), c.pay.push_back(0), c.plen.push_back(0);  // (no null array)
    sv_txaccounts& C = out->accts;
    C = A;
    C.struct_size = sizeof(sv_txaccounts);
    C.acct_key = c.key.data();
    C.acct_thresholds = c.thr.data();
    C.asigner_begin = c.sbeg.data();
    C.asigner_type = c.stype.data();
    C.asigner_weight = c.sweight.data();
    C.asigner_key = c.skey.data();
    C.asigner_payload = c.spay.data();
    C.apayload = c.pay.data();
    C.apayload_len = c.plen.data();
    C.bacct = out->bacct.data();
    C.n_accounts = c.accounts();
    C.n_asigners = c.stype.size() - 1;
    C.n_apayloads = c.plen.size() - 1;
  } catch (const std::bad_alloc&) {
    return SV_ERR_ALLOC;
  }
  return SV_OK;
}

int ledger_resolve(const sv_txledger* L, std::vector<uint32_t>* rows, std::vector<uint32_t>* ecnt,
                   std::vector<uint8_t>* found, std::vector<uint32_t>* view, std::vector<uint8_t>* vkey,
                   std::vector<uint8_t>* vthr, std::vector<uint64_t>* vsbeg) {
  AcctStore& S = acct_store();
  if (!L || L->struct_size < sizeof(sv_txledger) || !L->accts || L->accts->struct_size < sizeof(sv_txaccounts))
    return SV_ERR_INVALID_ARG;
  const sv_txaccounts& A = *L->accts;
  const size_t nl = A.n_accounts, ne = A.n_bacct;
  if ((uint64_t)ne >> 32 || (ne && !A.bacct)) return SV_ERR_INVALID_ARG;
  const AcctRows local{A.acct_key,        A.acct_thresholds, A.asigner_begin, A.asigner_type, A.asigner_weight,
                       A.asigner_key,     A.asigner_payload, A.apayload,      A.apayload_len, nl,
                       A.n_asigners,      A.n_apayloads};
  auto held = S.reader();
  if (!S.on() || nl > S.local_accounts() || AcctStore::check_rows(local, kAcctStride) != kAsOk)
    return SV_ERR_INVALID_ARG;
  try {
    // the local accounts' counts (txacct.h sv_acct_count)
    std::vector<uint32_t> lcnt(2 * nl + 2, 0);
    for (size_t a = 0; a < nl; ++a) {
      uint32_t nk = A.acct_thresholds[4 * a] ? 1u : 0u, nq = 0;
      for (uint64_t s = A.asigner_begin[a]; s < A.asigner_begin[a + 1]; ++s) A.asigner_type[s] == 3 ? ++nq : ++nk;
      lcnt[2 * a] = nk;
      lcnt[2 * a + 1] = nq;
    }
    const uint32_t cap = (uint32_t)S.capacity(), none = cap + (uint32_t)S.local_accounts();
    rows->assign(ne + 1, none);
    ecnt->assign(2 * ne + 2, 0);
    found->assign(ne + 1, 0);
    view->assign(ne + 1, (uint32_t)nl);
    // per entry, independent of the others: threaded like the twin's argument check (a lookup is a cache miss
    // into the index and one into the keys)
    auto part = [&](size_t e0, size_t e1) {
      for (size_t e = e0; e < e1; ++e) {
        const uint32_t b = A.bacct[e];
        if (b != SV_BACCT_BY_ID) {
          if (b >= nl) return false;
          (*rows)[e] = cap + b;
          (*ecnt)[2 * e] = lcnt[2 * b];
          (*ecnt)[2 * e + 1] = lcnt[2 * b + 1];
          (*found)[e] = 1;
          (*view)[e] = b;
          continue;
        }
        if (!L->bacct_id) return false;
        const uint32_t r = S.find(L->bacct_id + 32 * e);
        if (r == kAcctNone) continue;
        (*rows)[e] = r;
        (*ecnt)[2 * e] = S.acnt()[2 * (size_t)r];
        (*ecnt)[2 * e + 1] = S.acnt()[2 * (size_t)r + 1];
        (*found)[e] = 1;
      }
      return true;
    };
    const size_t T = std::max<size_t>(1, std::min<size_t>({(size_t)8, ne / 16384,
                                                           (size_t)std::max(1u, std::thread::hardware_concurrency())}));
    std::vector<uint8_t> good(T, 0);
    {
      // (a thread that cannot be started: the ones running are joined, then the call fails like an allocation)
      std::vector<std::thread> th;
      bool started = true;
      try {
        th.reserve(T);
        for (size_t i = 1; i < T; ++i)
          th.emplace_back([&, i] { good[i] = part(ne * i / T, ne * (i + 1) / T) ? 1 : 0; });
      } catch (const std::exception&) {
        started = false;
      }
      if (started) good[0] = part(0, ne / T) ? 1 : 0;
      for (auto& x : th) x.join();
      if (!started) return SV_ERR_ALLOC;
    }
    for (size_t i = 0; i < T; ++i)
      if (!good[i]) return SV_ERR_INVALID_ARG;
    vkey->assign(32 * (nl + 1), 0);
    vthr->assign(4 * (nl + 1), 0);
    vsbeg->assign(nl + 2, nl ? A.asigner_begin[nl] : 0);
    if (nl) {
      std::memcpy(vkey->data(), A.acct_key, 32 * nl);
      std::memcpy(vthr->data(), A.acct_thresholds, 4 * nl);
      std::memcpy(vsbeg->data(), A.asigner_begin, 8 * (nl + 1));
    }
  } catch (const std::bad_alloc&) {
    return SV_ERR_ALLOC;
  }
  return SV_OK;
}

}  // namespace sv
