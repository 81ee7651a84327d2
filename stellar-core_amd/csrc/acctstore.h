// The account store (include/stellar_sigverify.h sv_set_account_store): the
// host-authoritative table of ledger accounts whose read-only replicas the
// device slots hold (sv_txstore.hip).  Pure host code: the engine (sv_api.cpp,
// sv_txledger.cpp) and the tests' stand-alone program
// (tests/native/acctstore_san.cpp) compile this file.
//
// Rows      `accounts` rows at a fixed stride of kAcctStride (20, the
//           reference's MAX_SIGNERS) signers, struct-of-arrays, in exactly the
//           layout of the replica: key 32 | thresholds 4 | signer count 4 |
//           type 20 | weight 80 | signer key 640 | payload row 80 | rank 80 |
//           acnt 8 = 948 bytes per account, host and device alike.  acnt / rank
//           are txacct.h's sv_acct_count, made when the row is written.
// Payloads  `payloads` rows of 64 bytes and a length (65 bytes each) for type-3
//           signers, handed out from a free list; a type-3 signer's payload row
//           is private to it and goes back to the list when its account is
//           overwritten or erased.
// Index     open addressing over the 32-byte ID, linear probing, a power of two
//           of 4-byte slots >= 2 * accounts fixed at creation (8 to 16 bytes per
//           account); a slot holds row + 1, 0: empty.  The slot is accthash.h's
//           seeded mix.  Erase shifts the run back (no tombstones), so a live
//           key's displacement only ever shrinks; max_probe, the largest
//           displacement + 1 any insert saw, bounds every lookup's loop.
// Writes    upsert / erase validate and size the whole batch first and change
//           nothing when they refuse.  What a write touched comes back as an
//           AcctDirty (rows, payload rows, index slots) and stage() packs those
//           into the records the replicas' scatter kernel reads.
// Locking   one shared_mutex of the store's own: writers exclusive, readers
//           shared, held for the host work alone -- nobody calls into HIP with
//           it held exclusively.  The engine serialises writers (and their
//           replication) above it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <vector>

#include "accthash.h"

namespace sv {

constexpr int kAsOk = 0, kAsInvalid = -1, kAsAlloc = -4;  // SV_OK, SV_ERR_INVALID_ARG, SV_ERR_ALLOC
constexpr uint32_t kAcctStride = 20;
constexpr uint32_t kAcctNone = 0xFFFFFFFFu;
constexpr size_t kAcctMaxRows = (size_t)1 << 26;  // (row * 20 + 19 and the index words stay far below 2^32)
// the scatter kernel's records (sv_txstore.hip)
constexpr size_t kAcctRowRec = 960;  // key 32 | skey 640 | weight 80 | payload row 80 | rank 80 | type 20, row 4, pad 8 | thr 4, count 4, acnt 8
constexpr size_t kAcctPayRec = 80;   // payload 64 | row 4, length 4, pad 8
constexpr size_t kAcctSlotRec = 8;   // slot 4, value 4

// The account-table fields of an sv_txaccounts.
struct AcctRows {
  const uint8_t* key;
  const uint8_t* thr;
  const uint64_t* sbeg;
  const uint8_t* stype;
  const uint32_t* sweight;
  const uint8_t* skey;
  const uint32_t* spay;
  const uint8_t* pay;
  const uint8_t* plen;
  size_t na, ns, np;
};

// What a write touched (duplicates possible; stage() sorts them out).
struct AcctDirty {
  std::vector<uint32_t> rows, pays, slots;
  bool index_cleared = false;  // clear(): every index word is 0
  bool whole = false;          // the lists are incomplete (no memory for them): a replica must be copied whole
  // (never throws: a write that has begun to change the store always completes)
  static void note(std::vector<uint32_t>& v, uint32_t x, bool* whole) {
    try {
      v.push_back(x);
    } catch (const std::bad_alloc&) {
      *whole = true;
    }
  }
  void reset() {
    whole = false;
    rows.clear();
    pays.clear();
    slots.clear();
    index_cleared = false;
  }
};

struct AcctStats {
  uint64_t capacity = 0, accounts = 0, payload_capacity = 0, payloads = 0, local_accounts = 0, index_slots = 0;
  uint64_t max_probe = 0, upsert_calls = 0, inserted = 0, replaced = 0, erase_calls = 0, erased = 0, erase_absent = 0;
  uint64_t version = 0, host_bytes = 0;  // (a refused write counts nowhere: it changes nothing)
};

// An account in the caller's layout (sv_account_store_read).
struct AcctReadOut {
  uint8_t* found;       // n
  uint8_t* thr;         // n x 4
  uint32_t* n_signers;  // n
  uint8_t* stype;       // n x 20
  uint32_t* sweight;    // n x 20
  uint8_t* skey;        // n x 20 x 32
  uint8_t* spayload;    // n x 20 x 64
  uint8_t* splen;       // n x 20
};

// CSR arrays an account is appended to (the CPU forms' combined table).
struct AcctCsr {
  std::vector<uint8_t> key, thr, stype, skey, pay, plen;
  std::vector<uint32_t> sweight, spay;
  std::vector<uint64_t> sbeg{0};
  size_t accounts() const { return sbeg.size() - 1; }
  void add_empty() {
    key.insert(key.end(), 32, 0);
    thr.insert(thr.end(), 4, 0);
    sbeg.push_back(stype.size());
  }
};

class AcctStore {
 public:
  // (Re)creates the store; accounts == 0: off, everything freed.
  int configure(size_t accounts, size_t payloads, size_t local_accounts, uint64_t seed) {
    if (accounts > kAcctMaxRows || payloads > kAcctMaxRows || local_accounts > kAcctMaxRows) return kAsInvalid;
    std::unique_lock<std::shared_mutex> g(mu_);
    free_all();
    st_ = AcctStats();
    st_.version = ++epoch_ << 32;  // (no replica of an earlier store passes for one of this store)
    if (!accounts) return kAsOk;
    size_t slots = 8;
    while (slots < 2 * accounts) slots <<= 1;
    try {
      key_.assign(32 * accounts, 0);
      thr_.assign(4 * accounts, 0);
      scnt_.assign(accounts, 0);
      stype_.assign(kAcctStride * accounts, 0);
      sweight_.assign(kAcctStride * accounts, 0);
      skey_.assign(32 * kAcctStride * accounts, 0);
      spay_.assign(kAcctStride * accounts, 0);
      rank_.assign(kAcctStride * accounts, 0);
      acnt_.assign(2 * accounts, 0);
      pay_.assign(64 * payloads, 0);
      plen_.assign(payloads, 0);
      index_.assign(slots, 0);
      free_rows_.resize(accounts);
      free_pays_.resize(payloads);
    } catch (const std::bad_alloc&) {
      free_all();
      return kAsAlloc;
    }
    for (size_t i = 0; i < accounts; ++i) free_rows_[i] = (uint32_t)(accounts - 1 - i);
    for (size_t i = 0; i < payloads; ++i) free_pays_[i] = (uint32_t)(payloads - 1 - i);
    cap_ = accounts;
    pcap_ = payloads;
    local_ = local_accounts;
    seed_ = seed;
    mask_ = (uint32_t)(slots - 1);
    max_probe_ = 1;
    return kAsOk;
  }

  bool on() const { return cap_ != 0; }
  size_t capacity() const { return cap_; }
  size_t payload_capacity() const { return pcap_; }
  size_t local_accounts() const { return local_; }
  size_t index_slots() const { return index_.size(); }
  uint64_t seed() const { return seed_; }
  // (the four below: under reader(), or by the one writer)
  uint32_t max_probe() const { return max_probe_; }
  uint64_t version() const { return st_.version; }
  const uint8_t* key() const { return key_.data(); }
  const uint8_t* thr() const { return thr_.data(); }
  const uint32_t* scnt() const { return scnt_.data(); }
  const uint8_t* stype() const { return stype_.data(); }
  const uint32_t* sweight() const { return sweight_.data(); }
  const uint8_t* skey() const { return skey_.data(); }
  const uint32_t* spay() const { return spay_.data(); }
  const uint32_t* rank() const { return rank_.data(); }
  const uint32_t* acnt() const { return acnt_.data(); }
  const uint8_t* pay() const { return pay_.data(); }
  const uint8_t* plen() const { return plen_.data(); }
  const uint32_t* index() const { return index_.data(); }

  std::shared_lock<std::shared_mutex> reader() const { return std::shared_lock<std::shared_mutex>(mu_); }

  // The per-account rules of sv_txaccounts_check plus the stride: kAsOk or kAsInvalid.
  static int check_rows(const AcctRows& B, uint32_t max_signers) {
    if ((uint64_t)B.na >> 32 || (uint64_t)B.ns >> 32 || (uint64_t)B.np >> 32) return kAsInvalid;
    if (B.na && (!B.key || !B.thr || !B.sbeg)) return kAsInvalid;
    if (B.ns && (!B.stype || !B.sweight || !B.skey)) return kAsInvalid;
    if (B.np && (!B.pay || !B.plen)) return kAsInvalid;
    for (size_t i = 0; i < B.np; ++i)
      if (B.plen[i] > 64) return kAsInvalid;
    if (B.na && (B.sbeg[0] != 0 || B.sbeg[B.na] != B.ns)) return kAsInvalid;
    for (size_t a = 0; a < B.na; ++a) {
      const uint64_t s0 = B.sbeg[a], s1 = B.sbeg[a + 1];
      if (s1 < s0 || s1 > B.ns || s1 - s0 > max_signers) return kAsInvalid;
      for (uint64_t s = s0; s < s1; ++s) {
        if (B.stype[s] > 3) return kAsInvalid;
        if (B.stype[s] == 3 && (!B.spay || B.spay[s] >= B.np)) return kAsInvalid;
      }
    }
    return kAsOk;
  }

  // All of the batch or none of it; within the batch the last row of an ID wins.
  int upsert(const AcctRows& B, AcctDirty* dirty) {
    dirty->reset();
    std::unique_lock<std::shared_mutex> g(mu_);
    if (!on() || check_rows(B, kAcctStride) != kAsOk) return kAsInvalid;
    if (!B.na) {
      ++st_.upsert_calls;
      return kAsOk;
    }
    // the winners, in batch order
    std::vector<uint32_t> ord;
    try {
      ord.resize(B.na);
    } catch (const std::bad_alloc&) {
      return kAsAlloc;
    }
    for (size_t i = 0; i < B.na; ++i) ord[i] = (uint32_t)i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) {
      const int c = std::memcmp(B.key + 32 * (size_t)x, B.key + 32 * (size_t)y, 32);
      return c ? c < 0 : x < y;
    });
    size_t w = 0;
    for (size_t i = 0; i < ord.size(); ++i)
      if (i + 1 == ord.size() || std::memcmp(B.key + 32 * (size_t)ord[i], B.key + 32 * (size_t)ord[i + 1], 32))
        ord[w++] = ord[i];
    ord.resize(w);
    std::sort(ord.begin(), ord.end());
    // room: new accounts against the free rows; payload rows after the overwritten accounts' come back
    size_t fresh = 0, pay_need = 0, pay_back = 0;
    for (uint32_t a : ord) {
      const uint32_t row = find_locked(B.key + 32 * (size_t)a);
      if (row == kAcctNone) ++fresh;
      else pay_back += acnt_[2 * row + 1];
      for (uint64_t s = B.sbeg[a]; s < B.sbeg[a + 1]; ++s) pay_need += B.stype[s] == 3;
    }
    if (fresh > free_rows_.size() || pay_need > free_pays_.size() + pay_back) return kAsAlloc;
    try {
      dirty->rows.reserve(ord.size());
      dirty->pays.reserve(pay_need);
      dirty->slots.reserve(fresh);
    } catch (const std::bad_alloc&) {
      return kAsAlloc;
    }
    // (nothing below can fail)  The overwritten accounts' payload rows come back before any row is handed out.
    for (uint32_t a : ord) {
      const uint32_t row = find_locked(B.key + 32 * (size_t)a);
      if (row != kAcctNone) release_payloads(row);
    }
    for (uint32_t a : ord) {
      const uint8_t* id = B.key + 32 * (size_t)a;
      uint32_t row = find_locked(id);
      if (row != kAcctNone) {
        ++st_.replaced;
      } else {
        row = free_rows_.back();
        free_rows_.pop_back();
        std::memcpy(&key_[32 * (size_t)row], id, 32);
        index_insert(row, dirty);
        ++st_.inserted;
      }
      write_row(row, B, a, dirty);
      AcctDirty::note(dirty->rows, row, &dirty->whole);
    }
    ++st_.upsert_calls;
    ++st_.version;
    return kAsOk;
  }

  // Erasing an ID the store does not hold is counted, not refused.
  int erase(const uint8_t* ids, size_t n, AcctDirty* dirty) {
    dirty->reset();
    std::unique_lock<std::shared_mutex> g(mu_);
    if (!on() || (n && !ids)) return kAsInvalid;
    try {  // (a shifted run may need more: AcctDirty::note)
      dirty->slots.reserve(2 * n);
      dirty->rows.reserve(n);
    } catch (const std::bad_alloc&) {
      return kAsAlloc;
    }
    ++st_.erase_calls;
    bool any = false;
    for (size_t i = 0; i < n; ++i) {
      const uint32_t slot = find_slot(ids + 32 * i);
      if (slot == kAcctNone) {
        ++st_.erase_absent;
        continue;
      }
      const uint32_t row = index_[slot] - 1;
      release_payloads(row);
      scnt_[row] = 0;
      acnt_[2 * row] = acnt_[2 * row + 1] = 0;
      free_rows_.push_back(row);
      AcctDirty::note(dirty->rows, row, &dirty->whole);  // (its zeroed counts: a replica stays the host copy's image)
      index_erase(slot, dirty);
      ++st_.erased;
      any = true;
    }
    if (any) ++st_.version;
    return kAsOk;
  }

  void clear(AcctDirty* dirty) {
    dirty->reset();
    std::unique_lock<std::shared_mutex> g(mu_);
    if (!on()) return;
    std::fill(index_.begin(), index_.end(), 0u);
    std::fill(scnt_.begin(), scnt_.end(), 0u);
    std::fill(acnt_.begin(), acnt_.end(), 0u);
    free_rows_.resize(cap_);
    for (size_t i = 0; i < cap_; ++i) free_rows_[i] = (uint32_t)(cap_ - 1 - i);
    free_pays_.resize(pcap_);
    for (size_t i = 0; i < pcap_; ++i) free_pays_[i] = (uint32_t)(pcap_ - 1 - i);
    max_probe_ = 1;
    dirty->index_cleared = true;
    ++st_.version;
  }

  // The row of an ID or kAcctNone (under reader()).
  uint32_t find(const uint8_t* id) const { return find_locked(id); }

  void stats(AcctStats* out) const {
    std::shared_lock<std::shared_mutex> g(mu_);
    *out = st_;
    out->capacity = cap_;
    out->accounts = cap_ - free_rows_.size();
    out->payload_capacity = pcap_;
    out->payloads = pcap_ - free_pays_.size();
    out->local_accounts = local_;
    out->index_slots = index_.size();
    out->max_probe = on() ? max_probe_ : 0;
    out->host_bytes = host_bytes();
  }
  // 948 bytes per account, 65 per payload row, 4 per index slot, and the two free lists.
  size_t host_bytes() const {
    return key_.size() + thr_.size() + stype_.size() + skey_.size() + pay_.size() + plen_.size() +
           4 * (scnt_.size() + sweight_.size() + spay_.size() + rank_.size() + acnt_.size() + index_.size() +
                free_rows_.capacity() + free_pays_.capacity());
  }

  // n accounts by ID in the caller's layout; absent ones read as zeros.
  void read(const uint8_t* ids, size_t n, const AcctReadOut& o) const {
    std::shared_lock<std::shared_mutex> g(mu_);
    for (size_t i = 0; i < n; ++i) {
      const uint32_t row = on() ? find_locked(ids + 32 * i) : kAcctNone;
      if (o.found) o.found[i] = row != kAcctNone;
      if (o.thr) std::memset(o.thr + 4 * i, 0, 4);
      if (o.n_signers) o.n_signers[i] = 0;
      if (o.stype) std::memset(o.stype + kAcctStride * i, 0, kAcctStride);
      if (o.sweight) std::memset(o.sweight + kAcctStride * i, 0, 4 * kAcctStride);
      if (o.skey) std::memset(o.skey + 32 * kAcctStride * i, 0, 32 * kAcctStride);
      if (o.spayload) std::memset(o.spayload + 64 * kAcctStride * i, 0, 64 * kAcctStride);
      if (o.splen) std::memset(o.splen + kAcctStride * i, 0, kAcctStride);
      if (row == kAcctNone) continue;
      const uint32_t ns = scnt_[row];
      const size_t s0 = (size_t)kAcctStride * row;
      if (o.thr) std::memcpy(o.thr + 4 * i, &thr_[4 * (size_t)row], 4);
      if (o.n_signers) o.n_signers[i] = ns;
      for (uint32_t j = 0; j < ns; ++j) {
        const size_t d = kAcctStride * i + j;
        if (o.stype) o.stype[d] = stype_[s0 + j];
        if (o.sweight) o.sweight[d] = sweight_[s0 + j];
        if (o.skey) std::memcpy(o.skey + 32 * d, &skey_[32 * (s0 + j)], 32);
        if (stype_[s0 + j] != 3) continue;
        const uint32_t p = spay_[s0 + j];
        if (o.spayload) std::memcpy(o.spayload + 64 * d, &pay_[64 * (size_t)p], 64);
        if (o.splen) o.splen[d] = plen_[p];
      }
    }
  }

  // Account `id` appended to the CSR arrays `c` (an empty account when the store does not hold it): under reader().
  bool append_csr(const uint8_t* id, AcctCsr* c) const {
    const uint32_t row = find_locked(id);
    if (row == kAcctNone) {
      c->add_empty();
      return false;
    }
    const size_t s0 = (size_t)kAcctStride * row;
    c->key.insert(c->key.end(), id, id + 32);
    c->thr.insert(c->thr.end(), &thr_[4 * (size_t)row], &thr_[4 * (size_t)row] + 4);
    for (uint32_t j = 0; j < scnt_[row]; ++j) {
      c->stype.push_back(stype_[s0 + j]);
      c->sweight.push_back(sweight_[s0 + j]);
      c->skey.insert(c->skey.end(), &skey_[32 * (s0 + j)], &skey_[32 * (s0 + j)] + 32);
      uint32_t pi = 0;
      if (stype_[s0 + j] == 3) {
        const uint32_t p = spay_[s0 + j];
        pi = (uint32_t)c->plen.size();
        c->pay.insert(c->pay.end(), &pay_[64 * (size_t)p], &pay_[64 * (size_t)p] + 64);
        c->plen.push_back(plen_[p]);
      }
      c->spay.push_back(pi);
    }
    c->sbeg.push_back(c->stype.size());
    return true;
  }

  // The scatter records of `d` (sorted, without duplicates, final values): rows | payload rows | index slots.
  struct Staged {
    std::vector<uint8_t> rec;
    size_t rows = 0, pays = 0, slots = 0;
  };
  void stage(AcctDirty& d, Staged* out) const {
    std::shared_lock<std::shared_mutex> g(mu_);
    auto uniq = [](std::vector<uint32_t>& v) {
      std::sort(v.begin(), v.end());
      v.erase(std::unique(v.begin(), v.end()), v.end());
    };
    uniq(d.rows);
    uniq(d.pays);
    uniq(d.slots);
    out->rows = d.rows.size();
    out->pays = d.pays.size();
    out->slots = d.index_cleared ? 0 : d.slots.size();
    out->rec.assign(kAcctRowRec * out->rows + kAcctPayRec * out->pays + kAcctSlotRec * out->slots, 0);
    uint8_t* p = out->rec.data();
    for (uint32_t row : d.rows) {
      const size_t s0 = (size_t)kAcctStride * row;
      std::memcpy(p, &key_[32 * (size_t)row], 32);
      std::memcpy(p + 32, &skey_[32 * s0], 640);
      std::memcpy(p + 672, &sweight_[s0], 80);
      std::memcpy(p + 752, &spay_[s0], 80);
      std::memcpy(p + 832, &rank_[s0], 80);
      std::memcpy(p + 912, &stype_[s0], 20);
      std::memcpy(p + 932, &row, 4);
      std::memcpy(p + 944, &thr_[4 * (size_t)row], 4);
      std::memcpy(p + 948, &scnt_[row], 4);
      std::memcpy(p + 952, &acnt_[2 * (size_t)row], 8);
      p += kAcctRowRec;
    }
    for (uint32_t q : d.pays) {
      std::memcpy(p, &pay_[64 * (size_t)q], 64);
      const uint32_t len = plen_[q];
      std::memcpy(p + 64, &q, 4);
      std::memcpy(p + 68, &len, 4);
      p += kAcctPayRec;
    }
    if (!d.index_cleared)
      for (uint32_t s : d.slots) {
        std::memcpy(p, &s, 4);
        std::memcpy(p + 4, &index_[s], 4);
        p += kAcctSlotRec;
      }
  }

 private:
  uint32_t home(const uint8_t* id) const {
    uint32_t w[8];
    std::memcpy(w, id, 32);
    return (uint32_t)sv_acct_hash(w, seed_) & mask_;
  }
  uint32_t find_slot(const uint8_t* id) const {
    uint32_t s = home(id);
    for (uint32_t i = 0; i < max_probe_; ++i, s = (s + 1) & mask_) {
      const uint32_t v = index_[s];
      if (!v) return kAcctNone;
      if (!std::memcmp(&key_[32 * (size_t)(v - 1)], id, 32)) return s;
    }
    return kAcctNone;
  }
  uint32_t find_locked(const uint8_t* id) const {
    const uint32_t s = find_slot(id);
    return s == kAcctNone ? kAcctNone : index_[s] - 1;
  }
  // (the index has at least twice as many slots as rows: an empty one is always found)
  void index_insert(uint32_t row, AcctDirty* dirty) {
    const uint32_t h = home(&key_[32 * (size_t)row]);
    uint32_t s = h;
    while (index_[s]) s = (s + 1) & mask_;
    index_[s] = row + 1;
    AcctDirty::note(dirty->slots, s, &dirty->whole);
    max_probe_ = std::max(max_probe_, ((s - h) & mask_) + 1);
  }
  // backward-shift deletion: every key of the run behind `i` that may move closer to its home does
  void index_erase(uint32_t i, AcctDirty* dirty) {
    uint32_t j = i;
    for (;;) {
      j = (j + 1) & mask_;
      if (!index_[j]) break;
      const uint32_t k = home(&key_[32 * (size_t)(index_[j] - 1)]);
      // the key at j stays if its home lies cyclically in (i, j]
      if (i <= j ? (i < k && k <= j) : (i < k || k <= j)) continue;
      index_[i] = index_[j];
      AcctDirty::note(dirty->slots, i, &dirty->whole);
      i = j;
    }
    index_[i] = 0;
    AcctDirty::note(dirty->slots, i, &dirty->whole);
  }
  void release_payloads(uint32_t row) {
    const size_t s0 = (size_t)kAcctStride * row;
    for (uint32_t j = 0; j < scnt_[row]; ++j)
      if (stype_[s0 + j] == 3) free_pays_.push_back(spay_[s0 + j]);
  }
  // row <- account a of the batch; the signers past its count read as zeros
  void write_row(uint32_t row, const AcctRows& B, size_t a, AcctDirty* dirty) {
    const size_t s0 = (size_t)kAcctStride * row;
    const uint64_t b0 = B.sbeg[a];
    const uint32_t ns = (uint32_t)(B.sbeg[a + 1] - b0);
    std::memcpy(&thr_[4 * (size_t)row], B.thr + 4 * a, 4);
    std::memset(&stype_[s0], 0, kAcctStride);
    std::memset(&sweight_[s0], 0, 4 * kAcctStride);
    std::memset(&skey_[32 * s0], 0, 32 * kAcctStride);
    std::memset(&spay_[s0], 0, 4 * kAcctStride);
    std::memset(&rank_[s0], 0, 4 * kAcctStride);
    uint32_t nk = B.thr[4 * a] ? 1u : 0u, nq = 0;
    for (uint32_t j = 0; j < ns; ++j) {
      const uint8_t ty = B.stype[b0 + j];
      stype_[s0 + j] = ty;
      sweight_[s0 + j] = B.sweight[b0 + j];
      std::memcpy(&skey_[32 * (s0 + j)], B.skey + 32 * (b0 + j), 32);
      rank_[s0 + j] = ty == 3 ? nq++ : nk++;
      if (ty != 3) continue;
      const uint32_t p = free_pays_.back();
      free_pays_.pop_back();
      const uint32_t src = B.spay[b0 + j];
      const uint8_t len = B.plen[src];
      std::memset(&pay_[64 * (size_t)p], 0, 64);
      std::memcpy(&pay_[64 * (size_t)p], B.pay + 64 * (size_t)src, len);
      plen_[p] = len;
      spay_[s0 + j] = p;
      AcctDirty::note(dirty->pays, p, &dirty->whole);
    }
    scnt_[row] = ns;
    acnt_[2 * (size_t)row] = nk;
    acnt_[2 * (size_t)row + 1] = nq;
  }
  void free_all() {
    auto drop8 = [](std::vector<uint8_t>& v) { std::vector<uint8_t>().swap(v); };
    auto drop32 = [](std::vector<uint32_t>& v) { std::vector<uint32_t>().swap(v); };
    drop8(key_); drop8(thr_); drop8(stype_); drop8(skey_); drop8(pay_); drop8(plen_);
    drop32(scnt_); drop32(sweight_); drop32(spay_); drop32(rank_); drop32(acnt_); drop32(index_);
    drop32(free_rows_); drop32(free_pays_);
    cap_ = pcap_ = local_ = 0;
    mask_ = 0;
    max_probe_ = 1;
  }

  mutable std::shared_mutex mu_;
  std::vector<uint8_t> key_, thr_, stype_, skey_, pay_, plen_;
  std::vector<uint32_t> scnt_, sweight_, spay_, rank_, acnt_, index_, free_rows_, free_pays_;
  size_t cap_ = 0, pcap_ = 0, local_ = 0;
  uint64_t seed_ = 0, epoch_ = 0;
  uint32_t mask_ = 0, max_probe_ = 1;
  AcctStats st_;
};

// The process's store (defined in sv_txledger.cpp).
AcctStore& acct_store();

}  // namespace sv
