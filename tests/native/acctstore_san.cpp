// Stand-alone replay of the account store's host side (csrc/acctstore.h)
// against a std::map model, meant to be built with
// -fsanitize=address,undefined and run as a program
// (tests/test_txledger_cpu.py): store semantics, the smallest index with a
// wrapping probe run and backward-shift deletion, and refusals that must
// change nothing.  Prints "acctstore_san ok" and exits 0, or says what differs
// and exits 1.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "acctstore.h"

namespace {

using Id = std::array<uint8_t, 32>;
struct Signer {
  uint8_t type;
  uint32_t weight;
  Id key;
  std::vector<uint8_t> payload;  // type 3
};
struct Account {
  uint8_t thr[4];
  std::vector<Signer> signers;
};
using Model = std::map<Id, Account>;

int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

uint64_t g_rng = 0x1234567;
uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}
Id rand_id() {
  Id k;
  for (auto& b : k) b = (uint8_t)rnd();
  return k;
}
Account make_account(size_t n_signers, bool payloads) {
  Account a;
  for (int i = 0; i < 4; ++i) a.thr[i] = (uint8_t)rnd();
  for (size_t j = 0; j < n_signers; ++j) {
    Signer s;
    s.type = payloads ? 3 : (uint8_t)(rnd() % 3);
    s.weight = rnd();
    s.key = rand_id();
    if (s.type == 3) {
      s.payload.resize(1 + rnd() % 64);
      for (auto& b : s.payload) b = (uint8_t)rnd();
    }
    a.signers.push_back(s);
  }
  return a;
}

// a batch in sv_txaccounts' account-table layout
struct Batch {
  std::vector<uint8_t> key, thr, stype, skey, pay, plen;
  std::vector<uint32_t> sweight, spay;
  std::vector<uint64_t> sbeg{0};
  void add(const Id& id, const Account& a) {
    key.insert(key.end(), id.begin(), id.end());
    thr.insert(thr.end(), a.thr, a.thr + 4);
    for (const Signer& s : a.signers) {
      stype.push_back(s.type);
      sweight.push_back(s.weight);
      skey.insert(skey.end(), s.key.begin(), s.key.end());
      spay.push_back((uint32_t)plen.size());
      if (s.type == 3) {
        std::vector<uint8_t> row(64, 0);
        std::copy(s.payload.begin(), s.payload.end(), row.begin());
        pay.insert(pay.end(), row.begin(), row.end());
        plen.push_back((uint8_t)s.payload.size());
      }
    }
    sbeg.push_back(stype.size());
  }
  sv::AcctRows rows() const {
    return sv::AcctRows{key.data(),  thr.data(), sbeg.data(), stype.data(),    sweight.data(), skey.data(),
                        spay.data(), pay.data(), plen.data(), sbeg.size() - 1, stype.size(),   plen.size()};
  }
};

// every ID of `ids` read back equals the model
void compare(const sv::AcctStore& S, const Model& M, const std::vector<Id>& ids) {
  const size_t n = ids.size();
  std::vector<uint8_t> flat(32 * n + 1), found(n + 1), thr(4 * n + 1), ty(20 * n + 1), key(640 * n + 1),
      pay(1280 * n + 1), plen(20 * n + 1);
  std::vector<uint32_t> ns(n + 1), w(20 * n + 1);
  for (size_t i = 0; i < n; ++i) std::copy(ids[i].begin(), ids[i].end(), flat.begin() + 32 * i);
  S.read(flat.data(), n, sv::AcctReadOut{found.data(), thr.data(), ns.data(), ty.data(), w.data(), key.data(),
                                          pay.data(), plen.data()});
  for (size_t i = 0; i < n; ++i) {
    auto it = M.find(ids[i]);
    CHECK(found[i] == (it != M.end()));
    if (it == M.end()) {
      CHECK(ns[i] == 0);
      continue;
    }
    const Account& a = it->second;
    CHECK(!std::memcmp(&thr[4 * i], a.thr, 4));
    CHECK(ns[i] == a.signers.size());
    for (size_t j = 0; j < 20; ++j) {
      const size_t d = 20 * i + j;
      if (j >= a.signers.size()) {  // no stale signer
        CHECK(ty[d] == 0 && w[d] == 0 && plen[d] == 0);
        for (int b = 0; b < 32; ++b) CHECK(key[32 * d + b] == 0);
        continue;
      }
      const Signer& s = a.signers[j];
      CHECK(ty[d] == s.type && w[d] == s.weight && !std::memcmp(&key[32 * d], s.key.data(), 32));
      if (s.type == 3) {
        CHECK(plen[d] == s.payload.size());
        CHECK(!std::memcmp(&pay[64 * d], s.payload.data(), s.payload.size()));
        for (size_t b = s.payload.size(); b < 64; ++b) CHECK(pay[64 * d + b] == 0);
      } else {
        CHECK(plen[d] == 0);
      }
    }
  }
}

int upsert(sv::AcctStore& S, Model& M, const std::vector<std::pair<Id, Account>>& rows) {
  Batch b;
  for (auto& r : rows) b.add(r.first, r.second);
  sv::AcctDirty d;
  const int rc = S.upsert(b.rows(), &d);
  if (rc == sv::kAsOk) {
    for (auto& r : rows) M[r.first] = r.second;
    sv::AcctStore::Staged st;
    S.stage(d, &st);  // (the records of the replicas' scatter: packed under the sanitizers too)
    CHECK(st.rec.size() == sv::kAcctRowRec * st.rows + sv::kAcctPayRec * st.pays + sv::kAcctSlotRec * st.slots);
  }
  return rc;
}
int erase(sv::AcctStore& S, Model& M, const std::vector<Id>& ids) {
  std::vector<uint8_t> flat(32 * ids.size() + 1);
  for (size_t i = 0; i < ids.size(); ++i) std::copy(ids[i].begin(), ids[i].end(), flat.begin() + 32 * i);
  sv::AcctDirty d;
  const int rc = S.erase(flat.data(), ids.size(), &d);
  if (rc == sv::kAsOk)
    for (auto& id : ids) M.erase(id);
  return rc;
}

void semantics() {
  sv::AcctStore S;
  Model M;
  CHECK(S.configure(16, 2, 4, 99) == sv::kAsOk);
  std::vector<Id> ids;
  for (int i = 0; i < 8; ++i) ids.push_back(rand_id());
  std::vector<std::pair<Id, Account>> rows;
  for (int i = 0; i < 6; ++i) rows.push_back({ids[i], make_account(i == 0 ? 20 : (size_t)i, false)});
  CHECK(upsert(S, M, rows) == sv::kAsOk);
  compare(S, M, ids);
  // 20 -> 1 signers: no stale signer
  CHECK(upsert(S, M, {{ids[0], make_account(1, false)}}) == sv::kAsOk);
  compare(S, M, ids);
  // payload rows are freed and reused: 2 rows survive 50 overwrites of one type-3 signer
  for (int r = 0; r < 50; ++r) CHECK(upsert(S, M, {{ids[1], make_account(1, true)}}) == sv::kAsOk);
  compare(S, M, ids);
  // a duplicate ID inside one batch: the last row wins
  CHECK(upsert(S, M, {{ids[6], make_account(3, false)}, {ids[2], make_account(2, false)}, {ids[6], make_account(5, false)}}) ==
        sv::kAsOk);
  compare(S, M, ids);
  CHECK(erase(S, M, {ids[3], ids[7], ids[3]}) == sv::kAsOk);  // ids[7] was never there; ids[3] twice
  compare(S, M, ids);
  sv::AcctStats st;
  S.stats(&st);
  CHECK(st.accounts == M.size() && st.accounts == 6);
  CHECK(st.inserted == 7 && st.replaced == 1 + 50 + 1 && st.erased == 1 && st.erase_absent == 2);
  CHECK(st.payloads == 1 && st.upsert_calls == 53 && st.erase_calls == 1);
  sv::AcctDirty d;
  S.clear(&d);
  M.clear();
  compare(S, M, ids);
  CHECK(upsert(S, M, rows) == sv::kAsOk);
  compare(S, M, ids);
}

void smallest_index() {
  // 4 accounts, 8 slots: look for 4 IDs with a probe run that wraps past the last slot
  bool wrapped = false;
  for (uint64_t seed = 1; seed < 2000; ++seed) {
    sv::AcctStore S;
    Model M;
    CHECK(S.configure(4, 0, 0, seed) == sv::kAsOk);
    std::vector<Id> ids;
    std::vector<std::pair<Id, Account>> rows;
    for (int i = 0; i < 4; ++i) {
      ids.push_back(rand_id());
      rows.push_back({ids[i], make_account(1, false)});
    }
    CHECK(upsert(S, M, rows) == sv::kAsOk);
    const uint32_t* ix = S.index();
    if (!(ix[7] && ix[0] && S.max_probe() > 1)) continue;  // (a run over the seam with a displaced key)
    compare(S, M, ids);
    // erase every ID in turn from a fresh copy of this store: the others stay found (backward shift)
    for (int e = 0; e < 4; ++e) {
      sv::AcctStore T;
      Model N;
      CHECK(T.configure(4, 0, 0, seed) == sv::kAsOk);
      CHECK(upsert(T, N, rows) == sv::kAsOk);
      CHECK(erase(T, N, {ids[e]}) == sv::kAsOk);
      compare(T, N, ids);
      CHECK(upsert(T, N, {rows[e]}) == sv::kAsOk);
      compare(T, N, ids);
    }
    wrapped = true;
    break;
  }
  CHECK(wrapped);
  // 64 IDs that differ in their last byte only
  sv::AcctStore S;
  Model M;
  CHECK(S.configure(64, 0, 0, 7) == sv::kAsOk);
  std::vector<Id> ids(64, rand_id());
  std::vector<std::pair<Id, Account>> rows;
  for (int i = 0; i < 64; ++i) {
    ids[i][31] = (uint8_t)i;
    rows.push_back({ids[i], make_account(i % 3, false)});
  }
  CHECK(upsert(S, M, rows) == sv::kAsOk);
  compare(S, M, ids);
  CHECK(S.max_probe() < 16);  // (a prefix hash would put all 64 in one run)
  for (int i = 0; i < 64; i += 2) CHECK(erase(S, M, {ids[i]}) == sv::kAsOk);
  compare(S, M, ids);
}

void refusals() {
  sv::AcctStore S;
  Model M;
  CHECK(S.configure(4, 1, 0, 5) == sv::kAsOk);
  std::vector<Id> ids;
  std::vector<std::pair<Id, Account>> rows;
  for (int i = 0; i < 5; ++i) ids.push_back(rand_id());
  for (int i = 0; i < 4; ++i) rows.push_back({ids[i], make_account(i == 3 ? 0 : 2, false)});
  CHECK(upsert(S, M, rows) == sv::kAsOk);
  sv::AcctStats before, after;
  S.stats(&before);
  auto unchanged = [&] {
    S.stats(&after);
    CHECK(!std::memcmp(&before, &after, sizeof before));
    compare(S, M, ids);
  };
  Model scratch = M;
  CHECK(upsert(S, scratch, {{ids[0], make_account(1, false)}, {ids[4], make_account(1, false)}}) == sv::kAsAlloc);
  unchanged();
  CHECK(upsert(S, scratch, {{ids[0], make_account(21, false)}}) == sv::kAsInvalid);
  unchanged();
  CHECK(upsert(S, scratch, {{ids[0], make_account(2, true)}}) == sv::kAsAlloc);  // a payload row too many
  unchanged();
  Account bad = make_account(2, false);
  bad.signers[1].type = 4;
  CHECK(upsert(S, scratch, {{ids[1], make_account(1, false)}, {ids[0], bad}}) == sv::kAsInvalid);
  unchanged();
  // ... and the store still takes what fits
  CHECK(upsert(S, M, {{ids[0], make_account(1, true)}}) == sv::kAsOk);
  compare(S, M, ids);
}

}  // namespace

int main() {
  semantics();
  smallest_index();
  refusals();
  if (g_fail) {
    std::printf("acctstore_san: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("acctstore_san ok\n");
  return 0;
}
