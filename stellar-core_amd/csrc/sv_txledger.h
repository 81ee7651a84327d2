// The ledger forms' expansion on the host (sv_txledger.cpp): a ledger call's
// local accounts followed by the store accounts it names, as the sv_txaccounts
// its by-account twin takes -- "the expansion stays the definition"
// (include/stellar_sigverify.h).
#pragma once

#include <vector>

#include "../../include/stellar_sigverify.h"
#include "acctstore.h"

namespace sv {

static_assert(kAsOk == SV_OK && kAsInvalid == SV_ERR_INVALID_ARG && kAsAlloc == SV_ERR_ALLOC,
              "acctstore.h's codes are the header's");

struct LedgerCombined {
  AcctCsr table;
  std::vector<uint32_t> bacct;
  std::vector<uint8_t> found;  // per entry, as bacct_found (the caller's array is written once the call is accepted)
  sv_txaccounts accts;  // the twin's struct over `table` and `bacct`
};
// SV_OK, SV_ERR_INVALID_ARG (the ledger forms' own refusals) or SV_ERR_ALLOC.
int ledger_combine(const sv_txledger* L, LedgerCombined* out);

// The entries of a host-buffer ledger call resolved on the host index, under the store's shared lock (the caller
// keeps writers out until the call's last chunk: sv_api.cpp g_as_mu): per entry the replica row (a store row, the
// borrowed row of a local account, or accounts + local_accounts: no account), its two counts and found; and, for
// the twin's argument check, a view of the call -- the local accounts plus one empty account (vkey / vthr / vsbeg,
// n_accounts + 1 rows) that every entry by ID names in `view`.  The same refusals as ledger_combine.
int ledger_resolve(const sv_txledger* L, std::vector<uint32_t>* rows, std::vector<uint32_t>* ecnt,
                   std::vector<uint8_t>* found, std::vector<uint32_t>* view, std::vector<uint8_t>* vkey,
                   std::vector<uint8_t>* vthr, std::vector<uint64_t>* vsbeg);

}  // namespace sv
