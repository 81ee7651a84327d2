// A device slot's replica of the account store (acctstore.h): the arrays the
// kernels of sv_txstore.hip write and look up, and that the by-account
// expansion (txacct.h, the kStride instantiations) reads in place as its
// sv_acct_tab.  Shared by sv_txstore.hip and the engine (sv_api.cpp).
//
// One allocation, every section 256-byte aligned, `rows` = accounts +
// local_accounts rows and `prows` = payloads + 20 * local_accounts payload rows
// long: the rows past `accounts` (and the payload rows past `pays`) are the ones
// a ledger call borrows for its local accounts.  948 bytes per row, 65 per
// payload row, 4 per index slot (2 to 4 slots per account of capacity).
#pragma once

#include <stddef.h>
#include <stdint.h>

#define SV_STORE_BLOCK 256
#define SV_STORE_ROW_REC 960  // acctstore.h kAcctRowRec, kAcctPayRec, kAcctSlotRec
#define SV_STORE_PAY_REC 80
#define SV_STORE_SLOT_REC 8

struct sv_store_tab {
  uint8_t* key;       // rows x 32
  uint8_t* thr;       // rows x 4
  uint32_t* scnt;     // rows
  uint8_t* stype;     // rows x 20
  uint32_t* sweight;  // rows x 20
  uint8_t* skey;      // rows x 20 x 32
  uint32_t* spay;     // rows x 20: payload row
  uint8_t* pay;       // prows x 64
  uint8_t* plen;      // prows
  uint32_t* acnt;     // rows x 2   (acnt | rank: the layout sv_txacct.hip takes as a table's workspace)
  uint32_t* rank;     // rows x 20
  uint32_t* index;    // slots: row + 1, 0: empty
  uint32_t accounts, rows, pays, prows, slots;  // (slots: a power of two)
  uint64_t seed;
};

// The section offsets of a replica in its one allocation.
struct sv_store_layout {
  size_t key, thr, scnt, stype, sweight, skey, spay, pay, plen, acnt, rank, index, bytes;
};
static inline size_t sv_store_a256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline struct sv_store_layout sv_store_layout_of(size_t rows, size_t prows, size_t slots) {
  struct sv_store_layout L;
  size_t o = 0;
  L.key = o, o += sv_store_a256(32 * rows);
  L.thr = o, o += sv_store_a256(4 * rows);
  L.scnt = o, o += sv_store_a256(4 * rows);
  L.stype = o, o += sv_store_a256(20 * rows);
  L.sweight = o, o += sv_store_a256(80 * rows);
  L.skey = o, o += sv_store_a256(640 * rows);
  L.spay = o, o += sv_store_a256(80 * rows);
  L.pay = o, o += sv_store_a256(64 * prows);
  L.plen = o, o += sv_store_a256(prows);
  // acnt | rank as sv_txacct.hip lays a table's workspace out: rank at acnt + align16(8 * rows)
  L.acnt = o, o += (8 * rows + 15) & ~(size_t)15;
  L.rank = o, o += sv_store_a256(80 * rows);
  o = sv_store_a256(o);
  L.index = o, o += sv_store_a256(4 * slots);
  L.bytes = o;
  return L;
}
