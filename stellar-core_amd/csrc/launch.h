// The one declaration of every extern "C" launcher and size query that
// crosses between the kernel files (sv_kernels.hip, sv_comb.hip, sv_hash.hip,
// sv_txhash.hip, sv_txpair.hip, sv_txcheck.hip, sv_txacct.hip, sv_txresult.hip, sv_vcache.hip, sv_sign.hip, sv_audit.hip), sv_cpu.cpp and the engine (sv_api.cpp and its modules).
// Included by the callers and by every definer, so a changed parameter list
// is a compile error instead of arguments corrupted at run time.
#pragma once

#include <cstddef>
#include <cstdint>

#include "keytab.h"

extern "C" {

// Argument check of the host-array tx-body entry points (sv_cpu.cpp).
int sv_txbodies_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                      const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies, const uint64_t* sig_begin,
                      const uint8_t* pk, const uint8_t* sig, size_t n, const uint8_t* verdict);
// ... and of the hinted ones (sv_cpu.cpp): the bodies, the two CSR arrays and
// the pair outputs against pair_cap.
int sv_txpairs_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                     const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies, const uint64_t* sig_begin,
                     const uint8_t* hint, const uint8_t* sig, size_t n_sigs, const uint64_t* key_begin,
                     const uint8_t* key, size_t n_keys, size_t pair_cap, const uint64_t* pair_begin,
                     const uint32_t* pair_sig, const uint32_t* pair_key, const uint8_t* pair_verdict,
                     const size_t* n_pairs);
// ... and of the check entry points (sv_cpu.cpp): the hinted inputs, sig_len,
// the check tables of `checks` (every CSR array, signer types, key indices
// inside their bodies, the 64-signature / 64-signer limits, the protocol) and
// the three outputs.
struct sv_txchecks;
int sv_txchecks_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                      const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies, const uint64_t* sig_begin,
                      const uint8_t* hint, const uint8_t* sig, size_t n_sigs, const uint64_t* key_begin,
                      const uint8_t* key, size_t n_keys, const struct sv_txchecks* checks, const uint8_t* check_ok,
                      const uint32_t* check_weight, const uint64_t* check_used);

// The payload tables of a check call (sv_cpu.cpp): `checks` as an sv_txchecks_payload when its struct_size covers
// one and pkey_begin is set, else nullptr -- whatever lies behind a plain sv_txchecks is not read.
struct sv_txchecks_payload;
const struct sv_txchecks_payload* sv_txchecks_tables(const struct sv_txchecks* checks);

// Argument check of the by-account check entry points (sv_cpu.cpp): the bodies and signatures as above, the
// account table, the per-body account lists and the per-check references of `accts`, the limits on the EXPANDED
// lists (64 signers per account, 2^32 rows) and the three outputs.  The per-account passes run once per account.
// acnt (optional out): 2 x n_accounts words, the rows account a adds to a body's key list and to its payload
// candidates (txacct.h sv_acct_count).
struct sv_txaccounts;
int sv_txaccounts_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                        const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                        const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                        const struct sv_txaccounts* accts, const uint8_t* check_ok, const uint32_t* check_weight,
                        const uint64_t* check_used, uint32_t* acnt);

// Argument checks of the decide entry points' sv_txresults (sv_cpu.cpp): the struct itself (struct_size, body_code,
// bad_body against bad_cap); then, once the twin's check has vouched for the counts, the roles (<= 1) and the flags
// (bit 0 only).  The bad list of a host form from body_code (global indices, *n_bad exact), and txresult.h over
// host arrays: body_code, body_fail, then the bad list.
struct sv_txresults;
int sv_txresults_args(const struct sv_txresults* res);
int sv_txresults_check(const struct sv_txresults* res, size_t n_bodies, size_t n_checks);
void sv_txresults_bad_list(const struct sv_txresults* res, size_t n_bodies);
void sv_txresults_fold(const struct sv_txresults* res, const uint64_t* check_begin, const uint64_t* sig_begin,
                       const uint8_t* check_ok, const uint64_t* check_used, size_t n_bodies, size_t n_checks,
                       size_t n_sigs);

// Argument checks of the signing entry points (sv_cpu.cpp): the host and CPU forms of sv_ed25519_sign_batch
// (null pointers, key_of == NULL with k != n, a key_of[i] >= k, k or n >= 2^32) and of sv_ed25519_sign_txbodies
// (the bodies and sig_begin as in sv_txbodies_check, then the keys).
int sv_sign_check(const uint8_t* seed, size_t k, const uint32_t* key_of, const uint8_t* msg, const uint64_t* msg_off,
                  const uint32_t* msg_len, uint32_t fixed_len, size_t n, const uint8_t* sig);
int sv_sign_txbodies_check(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                           const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                           const uint64_t* sig_begin, const uint8_t* seed, size_t k, const uint32_t* key_of, size_t n,
                           const uint8_t* hint, const uint8_t* sig);

// The textbook verifier on the host (sv_cpu.cpp: verify_core.h sv_verify_core over the radix-2^51 field): 1 accept,
// 0 reject.  The CPU form of the audit and the arbitration of sv_audit_read run it.
int sv_audit_cpu_one(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t len);

}  // extern "C"

// The launchers take HIP types: compiled only where the HIP runtime headers
// are on the include path (sv_cpu.cpp is built without them).
#if defined(__HIP_PLATFORM_AMD__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>

extern "C" {

// throughput and cold-key latency paths, signing (sv_kernels.hip)
size_t sv_ws_bytes(unsigned grid, uint64_t cap);
size_t sv_verify_ws_bytes(int path, unsigned grid, uint64_t n);
size_t sv_btab_bytes(void);
int sv_block_threads(void);
hipError_t sv_launch_btab_init(uint32_t* d_btab, hipStream_t s);
int sv_occupancy_blocks_per_cu(void);
hipError_t sv_launch_verify(int mode, int path, unsigned grid, const void* pk, const void* sig, const void* msg,
                            const uint64_t* off, const uint32_t* len, uint32_t fixed_len, uint64_t n,
                            void* verdict, void* bitmap, void* ws, const void* btab, uint32_t dbg, int share,
                            const sv_ktparams* kt, uint32_t* status, hipStream_t s);
int sv_share_blocks_per_cu(void);
size_t sv_key_table_entry_bytes(void);
uint64_t sv_plan_chunk_max(uint64_t n);
hipError_t sv_launch_sign(unsigned grid, const void* seed, const void* msg, uint64_t n, void* pk, void* sig,
                          void* ws, const void* btab, hipStream_t s);
// cache keys and SHA-256 (sv_hash.hip), tx contents hashes (sv_txhash.hip)
hipError_t sv_launch_hash(int kind, unsigned max_blocks, const void* pk, const void* sig, const void* msg,
                          const uint64_t* off, const uint32_t* len, uint32_t fixed_len, uint64_t n, void* out,
                          hipStream_t s);
hipError_t sv_launch_txhash(unsigned max_blocks, const uint8_t* nid, const void* bodies, const uint64_t* off,
                            const uint32_t* len, const uint8_t* kind, uint64_t n_bodies, const uint64_t* sig_begin,
                            uint64_t n, void* msg, void* digests, hipStream_t s);
// pairing by hint (sv_txpair.hip): count + scan, then fill; `ws` holds
// sv_pair_ws_bytes(n_bodies), the pair count is *sv_pair_total(ws, n_bodies)
int sv_pair_block(void);
size_t sv_pair_ws_bytes(uint64_t n_bodies);
const uint64_t* sv_pair_total(const void* ws, uint64_t n_bodies);
hipError_t sv_launch_pair_count(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                                const uint64_t* key_begin, const void* key, uint64_t n_keys, uint64_t n_bodies,
                                void* ws, uint64_t* pair_begin, hipStream_t s);
hipError_t sv_launch_pair_fill(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                               const uint64_t* key_begin, const void* key, uint64_t n_keys, uint64_t n_bodies,
                               void* ws, uint64_t* pair_begin, uint64_t n_pairs, uint32_t* pair_sig,
                               uint32_t* pair_key, void* gkey, void* gsig, void* gmsg, const void* digests,
                               hipStream_t s);
// payload pairing (sv_txpair.hip): a body's signed-payload candidates against its signatures, after
// sv_launch_pair_count on the same `ws`; `pws` holds sv_ppair_ws_bytes(n_bodies), the count is
// sv_pair_total(ws, n_bodies)[1]; the fill gathers the arrays of a variable-length verify launch
size_t sv_ppair_ws_bytes(uint64_t n_bodies);
hipError_t sv_launch_ppair_count(const uint64_t* sig_begin, const void* hint, uint64_t n_sigs,
                                 const uint64_t* pkey_begin, const void* pkey, const void* payload,
                                 const uint8_t* plen, uint64_t n_pkeys, uint64_t n_bodies, void* ws, void* pws,
                                 uint64_t* ppair_begin, hipStream_t s);
hipError_t sv_launch_ppair_fill(const uint64_t* sig_begin, const void* hint, const void* sig, uint64_t n_sigs,
                                const uint64_t* pkey_begin, const void* pkey, const void* payload,
                                const uint8_t* plen, uint64_t n_pkeys, uint64_t n_bodies, void* ws, void* pws,
                                uint64_t* ppair_begin, uint64_t n_pairs, uint32_t* pair_sig, uint32_t* pair_key,
                                void* gkey, void* gsig, void* gmsg, uint64_t* goff, uint32_t* glen, hipStream_t s);
// one checkSignature decision per check (sv_txcheck.hip), after the pairing and the verify launch on the same
// stream; sig_len may be nullptr (all 64)
int sv_check_block(void);
hipError_t sv_launch_txcheck(const uint64_t* sig_begin, const void* hint, const void* sig, const uint8_t* sig_len,
                             uint64_t n_sigs, const uint64_t* key_begin, const void* key, uint64_t n_keys,
                             uint64_t n_bodies, const uint64_t* pair_begin, const uint32_t* pair_sig,
                             const uint32_t* pair_key, const void* pair_verdict, uint64_t n_pairs,
                             const void* digests, const uint64_t* check_begin, const int32_t* check_needed,
                             uint64_t n_checks, const uint64_t* signer_begin, const uint8_t* signer_type,
                             const uint32_t* signer_weight, const uint32_t* signer_key, uint64_t n_signers,
                             int clamp, uint8_t* check_ok, uint32_t* check_weight, uint64_t* check_used,
                             hipStream_t s);
// ... with the payload pairing's output (sv_launch_ppair_fill) and the candidates' CSR array for the
// signed-payload pass; n_ppairs == 0: no payload pairs, the payload arguments are not read
hipError_t sv_launch_txcheck_payload(const uint64_t* sig_begin, const void* hint, const void* sig,
                                     const uint8_t* sig_len, uint64_t n_sigs, const uint64_t* key_begin,
                                     const void* key, uint64_t n_keys, uint64_t n_bodies, const uint64_t* pair_begin,
                                     const uint32_t* pair_sig, const uint32_t* pair_key, const void* pair_verdict,
                                     uint64_t n_pairs, const void* digests, const uint64_t* check_begin,
                                     const int32_t* check_needed, uint64_t n_checks, const uint64_t* signer_begin,
                                     const uint8_t* signer_type, const uint32_t* signer_weight,
                                     const uint32_t* signer_key, uint64_t n_signers, int clamp,
                                     const uint64_t* ppair_begin, const uint32_t* ppair_sig,
                                     const uint32_t* ppair_key, const void* ppair_verdict, uint64_t n_ppairs,
                                     const uint64_t* pkey_begin, uint64_t n_pkeys, uint8_t* check_ok,
                                     uint32_t* check_weight, uint64_t* check_used, hipStream_t s);
// checks by account (sv_txacct.hip, txacct.h): the per-account counts and ranks into `tab_ws`
// (sv_acct_tab_ws_bytes), once per table; then per call or chunk, on the same stream, count + scan + begin
// (key_begin, pkey_begin, signer_begin, check_needed and the three totals at sv_acct_totals(ws, ...)) and the fill
// of the rows O's nk / nq / ng say its arrays hold; `ws` holds sv_acct_ws_bytes(nb, ne, nc).  The structs are
// host memory, their arrays device memory (key / skey / pay and O's key / pkey / ppay 16-byte aligned).
struct sv_acct_tab;
struct sv_acct_use;
struct sv_acct_out;
int sv_acct_block(void);
size_t sv_acct_tab_ws_bytes(uint64_t na, uint64_t ns);
size_t sv_acct_ws_bytes(uint64_t nb, uint64_t ne, uint64_t nc);
const uint64_t* sv_acct_totals(const void* ws, uint64_t nb, uint64_t ne, uint64_t nc);
hipError_t sv_launch_acct_table(const struct sv_acct_tab* T, void* tab_ws, hipStream_t s);
hipError_t sv_launch_acct_count(const struct sv_acct_tab* T, const void* tab_ws, const struct sv_acct_use* U,
                                const struct sv_acct_out* O, void* ws, hipStream_t s);
hipError_t sv_launch_acct_fill(const struct sv_acct_tab* T, const void* tab_ws, const struct sv_acct_use* U,
                               const struct sv_acct_out* O, void* ws, hipStream_t s);
// ... with T an account store's replica (txacct.h sv_acct_tab::scnt): the rows and signers kernels' stride
// instantiations.  The count launch above serves both layouts (it reads the counts in tab_ws alone).
hipError_t sv_launch_acct_fill_stride(const struct sv_acct_tab* T, const void* tab_ws, const struct sv_acct_use* U,
                                      const struct sv_acct_out* O, void* ws, hipStream_t s);
// the account store's replica (sv_txstore.hip, txstore.h), every launch on the slot's one stream.  scatter: the
// staged records of a host write (acctstore.h stage(): n_rows row records | n_pays payload records | n_slots
// index records) into the replica.  lookup: per entry the row of bacct_id[e] (bacct[e] == SV_BACCT_BY_ID or bacct
// null), of local account bacct[e] < n_local, or R->rows for none; `found` optional.  local: the caller's CSR
// accounts [0, n_local) into the borrowed rows.  gather: the looked-up rows in sv_account_store_read's layout
// (sv_store_read_offsets) into `out` (sv_store_read_bytes).
struct sv_store_tab;
int sv_store_block(void);
size_t sv_store_read_bytes(uint64_t n);
void sv_store_read_offsets(uint64_t n, size_t off[7]);
void sv_store_tab_as_acct(const struct sv_store_tab* R, struct sv_acct_tab* T);
hipError_t sv_launch_store_scatter(const struct sv_store_tab* R, const void* rec, uint32_t n_rows, uint32_t n_pays,
                                   uint32_t n_slots, hipStream_t s);
hipError_t sv_launch_store_lookup(const struct sv_store_tab* R, const uint32_t* bacct, const void* ids, uint64_t n,
                                  uint32_t n_local, uint32_t max_probe, uint32_t* row_out, void* found,
                                  hipStream_t s);
hipError_t sv_launch_store_local(const struct sv_store_tab* R, const struct sv_acct_tab* L, uint32_t n_local,
                                 hipStream_t s);
hipError_t sv_launch_store_gather(const struct sv_store_tab* R, const uint32_t* rows, uint64_t n, void* out,
                                  hipStream_t s);
// one result per body (sv_txresult.hip, txresult.h), after the check kernel on the same stream: body_code (and
// body_fail, optional) from I's check_ok / check_used; with bad_body or n_bad also the scan and, with bad_body and
// bad_cap > 0, the fill of the ascending non-OK bodies (entries at or past bad_cap are never written, *n_bad is
// exact).  `ws` holds sv_txresult_ws_bytes(nb); the struct is host memory, its arrays and the outputs device memory.
struct sv_txresult_in;
int sv_txresult_block(void);
size_t sv_txresult_ws_bytes(uint64_t n_bodies);
hipError_t sv_launch_txresult(const struct sv_txresult_in* I, uint8_t* body_code, uint32_t* body_fail, void* ws,
                              uint32_t* bad_body, uint64_t bad_cap, uint64_t* n_bad, hipStream_t s);
// the verdict cache (sv_vcache.hip, vcache.h), every stage on the slot's one stream.  probe: after
// sv_launch_hash kind 0 wrote A->keys -- the lookups (verdict and hit bytes of the hits), the scan and the fill of
// the miss list and the compacted arrays; the miss count lands in A->counters[3].  insert: behind the verify
// launch over the n_miss compacted rows -- the scatter of their verdicts with the claims, then the winners'
// stores.  bitmap: the layout of sv_launch_verify's, from n final verdict bytes (bits past n are 0).  The struct
// is host memory.
struct sv_vc_args;
int sv_vc_block(void);
size_t sv_vc_psum_bytes(uint64_t n);
hipError_t sv_launch_vc_probe(const struct sv_vc_args* A, hipStream_t s);
hipError_t sv_launch_vc_insert(const struct sv_vc_args* A, uint64_t n_miss, hipStream_t s);
hipError_t sv_launch_vc_bitmap(const void* verdict, uint64_t n, void* bitmap, hipStream_t s);
// The export of a pass behind its insert (vshare.h): the leading rows <= n_miss rows of the miss list -- keys
// (32 rows bytes), then verdict bytes (rows) -- into image (device memory, 33 rows bytes, 16-byte aligned).
hipError_t sv_launch_vc_export(const struct sv_vc_args* A, uint64_t n_miss, uint64_t rows, void* image, hipStream_t s);
// The drain of a slot's journal (vcache.h Feed): the claim and the store kernel over A->n rows with their
// verdicts.  lookup: out[i] = the verdict the table holds for key i (keys n x 32, 16-byte aligned), or 0xFF.
struct sv_vc_feed_args;
hipError_t sv_launch_vc_feed(const struct sv_vc_feed_args* A, hipStream_t s);
hipError_t sv_launch_vc_lookup(const void* tab, uint64_t sets, const void* keys, uint64_t n, void* out, hipStream_t s);
// batch signing (sv_sign.hip, sign_core.h): the keys kernel writes k expanded-key records (sv_sign_rec_bytes(k),
// 16-byte aligned) and, with pk, the public keys; the messages kernel signs n messages, message i with record
// key_of[i] (nullptr: i), 64 zero bytes where key_of[i] >= k; hint (optional): bytes 28..31 of each signer's key.
// ctab: the comb tables of B (sv_launch_comb_btab).  seed / pk / sig 16-byte aligned.
size_t sv_sign_rec_bytes(uint64_t k);
hipError_t sv_launch_sign_keys(const void* seed, uint32_t k, void* rec, void* pk, const uint32_t* ctab,
                               hipStream_t s);
hipError_t sv_launch_sign_msgs(const void* rec, uint32_t k, const uint32_t* key_of, const void* msg,
                               const uint64_t* off, const uint32_t* len, uint32_t fixed_len, uint32_t n, void* sig,
                               void* hint, const uint32_t* ctab, hipStream_t s);
// the verdict audit (sv_audit.hip, audit.h), every kernel on the caller's one stream and no host wait: select,
// scan and fill of the picked rows, the textbook verify over the first A->budget of them on A->grid workgroups
// (sv_audit_grid: sized from min(n, budget), at most max_blocks; A->ws holds sv_audit_ws_bytes(grid)), and the
// report into A->counters and A->ring.  A->psum holds sv_audit_psum_bytes(n).  The struct is host memory.
struct sv_audit_args;
size_t sv_audit_psum_bytes(uint64_t n);
int sv_audit_blocks_per_cu(void);
unsigned sv_audit_grid(uint64_t n, uint64_t budget, unsigned max_blocks);
size_t sv_audit_ws_bytes(unsigned grid);
hipError_t sv_launch_audit(const struct sv_audit_args* A, hipStream_t s);
// warm-key latency path (sv_comb.hip)
size_t sv_comb_btab_bytes(void);
size_t sv_key_slot_bytes(void);
hipError_t sv_launch_comb_btab(uint32_t* d_ctab, hipStream_t s);
hipError_t sv_launch_keytab(const void* d_pks, const uint32_t* d_slots, uint32_t nkeys, uint32_t* d_ktab,
                            uint32_t* d_kstat, hipStream_t s);
int sv_comb_spw(uint64_t n, int cus);
hipError_t sv_launch_comb(int mode, int spw, const void* pk, const void* sig, const void* msg, const uint64_t* off,
                          const uint32_t* len, uint32_t fixed_len, uint64_t n, void* verdict, const uint32_t* kslot,
                          const uint32_t* ktab, const uint32_t* kstat, const uint32_t* ctab, hipStream_t s);

}  // extern "C"
#endif
