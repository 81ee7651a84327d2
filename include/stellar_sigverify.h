/*
 * stellar_sigverify.h — C-ABI of the MI355X (gfx950) batched ed25519
 * signature-verification engine for stellar-core.
 *
 * Drop-in boundary.  stellar-core verifies every ed25519 signature through one
 * synchronous function:
 *
 *   bool stellar::PubKeyUtils::verifySig(PublicKey const&, Signature const&,
 *                                        ByteSlice const&)
 *     declared  /root/reference/src/crypto/SecretKey.h:139-140
 *     defined   /root/reference/src/crypto/SecretKey.cpp:435-468
 *
 * which, on a verify-cache miss, calls libsodium
 *   crypto_sign_verify_detached(sig, msg, msg_len, pk)   (SecretKey.cpp:461-463)
 *
 * The entry points below replace that libsodium call for WHOLE BATCHES of
 * cache misses.  Verdicts are bit-identical to libsodium 1.0.18
 * crypto_sign_verify_detached (cofactorless, S < L, small-order R/A and
 * non-canonical A rejected) on every input.  The size-64 rule of
 * SecretKey.cpp:441-444 is the caller's job (a Signature is an XDR opaque<64>;
 * anything shorter never reaches this API), as is the verify cache
 * (SecretKey.cpp:446-457,464-466) — see the C++ host mirror
 * stellar-core_amd/csrc/host/PubKeyUtils.{h,cpp}.
 *
 * Conventions: plain pointers and sizes, caller-owned memory, no exceptions
 * cross the boundary, every call returns SV_OK (0) or a negative SV_ERR_*.
 * An error is NEVER a reject: on error the verdict buffer content is
 * unspecified and the caller must treat the whole batch as unverified.
 * All entry points are thread-safe; calls that target one device are
 * serialised on that device's internal stream (its per-lane table workspace).
 */
#ifndef STELLAR_SIGVERIFY_H
#define STELLAR_SIGVERIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SV_OK 0
#define SV_ERR_INVALID_ARG (-1)
#define SV_ERR_NO_DEVICE (-2)
#define SV_ERR_HIP (-3)
#define SV_ERR_ALLOC (-4)
#define SV_ERR_NOT_INIT (-5)
#define SV_ERR_ALIGN (-6)
/* A kernel reported that it could not stand behind its verdicts (the
 * three-wave cold-key octet kernel when one of its bounded LDS hand-over waits
 * ran out).  Like every error: the verdict buffer is unspecified and the batch
 * must be re-verified (the C++ mirror re-runs it on the CPU path), never
 * cached as rejects. */
#define SV_ERR_KERNEL (-7)

/* Batch options.  A NULL opts pointer means "all defaults". */
typedef struct sv_opts {
  uint32_t struct_size; /* sizeof(sv_opts), for forward compatibility */
  int32_t device;       /* -1 (default): contiguous slices over the device slots, every slice at least the
                           minimum shard (sv_set_min_shard; smaller batches run on one slot); k >= 0: slot k only */
  uint32_t max_devices; /* 0 (default): no limit; else use at most this many slots when device == -1 */
  uint32_t flags;       /* 0 or one SV_FLAG_PATH_* (kernel path for this call); other bits must be 0 */
} sv_opts;

/* Kernel paths.  THROUGHPUT: one lane per signature, prep + main kernels per
 * 2^20-signature chunk (large batches).  LATENCY: one quad of lanes per
 * signature, every point operation split four ways (small, latency-bound
 * batches such as SCP envelope floods).  AUTO picks LATENCY for batches of at
 * most 12288 signatures (the sizes it runs in one pass over the GPU).
 * Verdicts are identical on every path. */
#define SV_PATH_AUTO 0
#define SV_PATH_THROUGHPUT 1
#define SV_PATH_LATENCY 2
#define SV_FLAG_PATH_THROUGHPUT 0x1u
#define SV_FLAG_PATH_LATENCY 0x2u
#define SV_FLAG_PATH_MASK 0x3u

/* Process-wide default path for calls that do not request one (the device
 * API never does).  Returns the previous default, or SV_ERR_INVALID_ARG. */
int sv_set_kernel_path(int path);

/* Enumerate the device slots (one per visible GPU unless a device map says
 * otherwise).  Idempotent; called implicitly by every entry point.  Per-slot
 * resources (streams, base-point tables, workspace, pinned staging) are
 * created on the slot's first use; the throughput-path workspace is sized to
 * the batch and grows on demand. */
int sv_init(void);
/* Device slots -> physical GPUs, e.g. {0, 0}: two logical slots on GPU 0
 * (tests of the multi-device path on one GPU).  Releases every slot's
 * resources first; count == 0 restores one slot per visible GPU.  The
 * environment variable SV_DEVICE_MAP="0,0" sets the same at first init. */
int sv_set_device_map(const int* physical, int count);
/* Minimum signatures per slot when a batch is sharded (default 65536). */
int sv_set_min_shard(size_t n);
/* Release all device resources.  Safe to call more than once. */
void sv_shutdown(void);
/* Number of usable devices (initialises on first use); negative on error. */
int sv_device_count(void);
/* Thread-local description of the last error on the calling thread. */
const char* sv_last_error_string(void);
const char* sv_version(void);

/*
 * Variable-length batch, host buffers (replaces n calls of
 * crypto_sign_verify_detached made by PubKeyUtils::verifySig, SecretKey.cpp:461-463).
 *   pk       n x 32 bytes   (PublicKey ed25519, uint256)
 *   sig      n x 64 bytes   (R || S)
 *   msg      message bytes; message i = msg[msg_off[i] .. msg_off[i] + msg_len[i])
 *   verdict  n bytes out, 1 = valid, 0 = invalid
 */
int sv_ed25519_verify_batch(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                            const uint64_t* msg_off, const uint32_t* msg_len, size_t n,
                            uint8_t* verdict, const sv_opts* opts);

/*
 * Gather form of sv_ed25519_verify_batch: item i is (pk[i] -> 32 bytes,
 * sig[i] -> 64 bytes, msg[i] -> msg_len[i] bytes), packed by the engine
 * straight into its pinned staging (no intermediate copy by the caller, e.g.
 * PubKeyUtils::verifySigBatch over VerifyItem pointers).  keys (optional, n x
 * 32) also receives each item's verify-cache key BLAKE2b-256(pk || sig ||
 * msg) from the same staging (SecretKey.cpp:50-61).
 */
int sv_ed25519_verify_batch_gather(const uint8_t* const* pk, const uint8_t* const* sig, const uint8_t* const* msg,
                                   const uint32_t* msg_len, size_t n, uint8_t* verdict, uint8_t* keys,
                                   const sv_opts* opts);

/*
 * Same, with a callback for overlapping the caller's work with the GPU:
 * keys_ready(ctx) is called exactly once on success, on the calling thread,
 * as soon as every key is in `keys` -- for a batch that fits one staging chunk
 * on one slot, while the verify kernels are still running -- and the call
 * returns once the verdicts are in `verdict`.  keys_ready must not call into
 * this library.  On an error return keys_ready may or may not have run.
 */
int sv_ed25519_verify_batch_gather_cb(const uint8_t* const* pk, const uint8_t* const* sig,
                                      const uint8_t* const* msg, const uint32_t* msg_len, size_t n, uint8_t* verdict,
                                      uint8_t* keys, void (*keys_ready)(void* ctx), void* ctx, const sv_opts* opts);

/*
 * As sv_ed25519_verify_batch_gather_cb, with the keys delivered in pieces:
 * keys_ready(ctx, ready) runs with keys [0, ready) in `keys`, for increasing
 * `ready`, the last time with ready == n.  For a one-chunk batch of >= 8192
 * signatures the engine packs, copies up and hashes the batch in pieces: the
 * first of 2048 rows, each later one twice the one before, at most 32768 rows,
 * and no runt last piece (a remainder under 1.5 pieces joins the one before;
 * a 100k batch is 6 pieces).  So a caller that walks its cache in item order
 * (verifySigBatch, /root/reference/src/crypto/SecretKey.cpp:446-466 per item)
 * starts on the first rows while the rest is still on its way.  Same threading
 * rules.
 */
int sv_ed25519_verify_batch_gather_progress(const uint8_t* const* pk, const uint8_t* const* sig,
                                            const uint8_t* const* msg, const uint32_t* msg_len, size_t n,
                                            uint8_t* verdict, uint8_t* keys,
                                            void (*keys_ready)(void* ctx, size_t ready), void* ctx,
                                            const sv_opts* opts);

/*
 * CPU path: the engine's own per-signature algorithm (csrc/verify_core.h,
 * the half-size equation of csrc/lattice.h) compiled for the host, on
 * `threads` threads (0: the machine's hardware concurrency, capped at 16).
 * Same verdicts as every GPU path.  It is what a caller runs when a GPU entry
 * point returns an error (an error is never a reject) and what the C++ mirror
 * uses for single-signature verifySig calls, where a GPU round trip costs more
 * than the verification itself.  Message layout as in sv_ed25519_verify_batch.
 */
int sv_ed25519_verify_batch_cpu(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                                const uint32_t* msg_len, size_t n, uint8_t* verdict, int threads);
/* single-signature form (returns 1 valid, 0 invalid) */
int sv_ed25519_verify_cpu(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, size_t msg_len);

/*
 * Fixed-length batch, host buffers: message i = msg[i*msg_len .. (i+1)*msg_len).
 * msg_len == 32 (transaction contents hashes, TransactionFrame.cpp:90-117)
 * takes the single-SHA-512-block fast path.
 */
int sv_ed25519_verify_batch_fixed(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                                  uint32_t msg_len, size_t n, uint8_t* verdict, const sv_opts* opts);

/*
 * Device-resident batch on one device: every pointer is device memory on
 * `device` (16-byte aligned pk/sig; for fixed_msg_len == 32 also msg).
 * If fixed_msg_len != 0, message i = d_msg[i*fixed_msg_len ..] and
 * d_msg_off/d_msg_len are ignored (may be NULL).  d_bitmap (optional, may be
 * NULL) receives one bit per signature, 64 per word, bit (i % 64) of word
 * i / 64 (wave-level ballot compaction of the verdicts); it must hold
 * ceil(n / 64) words, and the bits past n in the last word are written 0.
 * `stream` is a hipStream_t (NULL = legacy default stream): the work is
 * ordered after prior work on `stream` and later work on `stream` is ordered
 * after it; the call itself does not block.
 */
int sv_ed25519_verify_device(int device, const void* d_pk, const void* d_sig, const void* d_msg,
                             const uint64_t* d_msg_off, const uint32_t* d_msg_len,
                             uint32_t fixed_msg_len, size_t n, void* d_verdict, void* d_bitmap,
                             void* stream);

/*
 * Synthetic-workload generator (device-resident): for i in [0, n) derive the
 * keypair from seed i (RFC 8032, == crypto_sign_seed_keypair) and sign the
 * 32-byte message i (== crypto_sign_detached).  Used by the bench to build
 * the 1M..64M-signature datasets on the GPU box; its output is checked
 * against libsodium-generated digests (tests/golden/digests.json).
 */
int sv_ed25519_sign_device(int device, const void* d_seed, const void* d_msg32, size_t n, void* d_pk,
                           void* d_sig, void* stream);

/* ---- Batch signing (src/crypto/SecretKey.cpp:134-146, 286, 309) ----------
 * sig[i] = crypto_sign_detached(message i, sk(seed[key_of[i]])) and
 * pk[j] = crypto_sign_seed_keypair(seed[j]).pk, byte for byte (RFC 8032
 * signing is deterministic), for messages of any length and with keys shared
 * between messages: every key is expanded once per call, not once per
 * signature.  key_of == NULL means k == n and key i signs message i.
 * fixed_msg_len != 0: message i = msg[i*fixed_msg_len ..); 0: msg_off/msg_len
 * as in sv_ed25519_verify_batch.  n == 0 with k > 0 yields only the public
 * keys; k == 0 with n == 0 does nothing.  pk is optional (NULL: not written).
 *
 * What this signer is for: load generation, test networks, benchmarks and
 * dataset building -- the bulk signing of src/simulation/TxGenerator.cpp.  It
 * is NOT constant-time: table addresses follow the secret scalars' digits.
 * In the host and device forms the seeds cross PCIe and they and the expanded
 * keys sit in HBM for the length of the call (the engine's copies are cleared
 * before it returns, on the call's stream in the device form).  A validator's
 * NODE_SEED signing of single messages stays where it is, in libsodium.
 *
 * Host and CPU forms return SV_ERR_INVALID_ARG before any work, with no
 * output byte written, for: a null required pointer; key_of == NULL with
 * k != n (n > 0); a key_of[i] >= k; k or n >= 2^32.
 *
 * Host form: stages through one slot in pieces of at most SV_STAGE_CHUNK
 * signatures (and 256 MiB of message bytes); copy and compute do not overlap.  Signing calls are not
 * sharded: opts->device == -1 is served by one slot (round-robin).
 *
 * Device form: stream semantics as sv_ed25519_verify_device.  d_seed, d_sig
 * and d_pk must be 16-byte aligned (SV_ERR_ALIGN).  The device arrays are not
 * validated: a d_key_of[i] >= k writes 64 zero bytes for row i, and nothing
 * is written outside d_sig (n x 64) and d_pk (k x 32).
 */
int sv_ed25519_sign_batch(const uint8_t* seed /* k x 32 */, size_t k,
                          const uint32_t* key_of /* n; NULL: k == n, key i signs message i */, const uint8_t* msg,
                          const uint64_t* msg_off, const uint32_t* msg_len, uint32_t fixed_msg_len, size_t n,
                          uint8_t* sig /* n x 64 */, uint8_t* pk /* optional, k x 32 */, const sv_opts* opts);
int sv_ed25519_sign_batch_device(int device, const void* d_seed, size_t k, const uint32_t* d_key_of,
                                 const void* d_msg, const uint64_t* d_msg_off, const uint32_t* d_msg_len,
                                 uint32_t fixed_msg_len, size_t n, void* d_sig, void* d_pk /* optional */,
                                 void* stream);
/* The same contract on the engine's CPU path (csrc/sign_core.h compiled for
 * the host; threads as sv_ed25519_verify_batch_cpu). */
int sv_ed25519_sign_batch_cpu(const uint8_t* seed, size_t k, const uint32_t* key_of, const uint8_t* msg,
                              const uint64_t* msg_off, const uint32_t* msg_len, uint32_t fixed_msg_len, size_t n,
                              uint8_t* sig, uint8_t* pk, int threads);

/*
 * Signing over transaction bodies: what SignatureUtils::sign
 * (src/transactions/SignatureUtils.cpp:19-27) produces per (transaction, key).
 * Bodies, kinds and sig_begin as in sv_ed25519_verify_txbodies; signature s of
 * body t (sig_begin[t] <= s < sig_begin[t+1], n = sig_begin[n_bodies]) is made
 * with seed[key_of[s]] over the body's contents hash.  Outputs: hint (n x 4,
 * bytes 28..31 of the signer's public key) and sig (n x 64), which with
 * sig_begin are exactly the inputs of sv_ed25519_verify_txbodies_hinted*;
 * pk (k x 32) and digests (n_bodies x 32) are optional.  key_of is required.
 * Refusals, staging, alignment (d_hint: 4 bytes) and the notes above apply;
 * in the device form a d_key_of[s] >= k also writes a zero hint.
 */
int sv_ed25519_sign_txbodies(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                             const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                             const uint64_t* sig_begin, const uint8_t* seed, size_t k, const uint32_t* key_of,
                             size_t n, uint8_t* hint, uint8_t* sig, uint8_t* pk, uint8_t* digests,
                             const sv_opts* opts);
int sv_ed25519_sign_txbodies_device(int device, const uint8_t* network_id /* host, 32 B */, const void* d_bodies,
                                    const uint64_t* d_body_off, const uint32_t* d_body_len,
                                    const uint8_t* d_body_kind, size_t n_bodies, const uint64_t* d_sig_begin,
                                    const void* d_seed, size_t k, const uint32_t* d_key_of, size_t n, void* d_hint,
                                    void* d_sig, void* d_pk, void* d_digests, void* stream);
int sv_ed25519_sign_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                 const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                 const uint64_t* sig_begin, const uint8_t* seed, size_t k, const uint32_t* key_of,
                                 size_t n, uint8_t* hint, uint8_t* sig, uint8_t* pk, uint8_t* digests, int threads);

/* ---- Batch hashing on the device ----------------------
 * Verify-cache keys: keys[32*i..] = BLAKE2b-256(pk_i || sig_i || msg_i), the key
 * PubKeyUtils::verifySig computes per call before consulting the cache
 * (/root/reference/src/crypto/SecretKey.cpp:50-61, verifySigCacheKey).
 * Message layout as in sv_ed25519_verify_batch. */
int sv_verify_cache_keys(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint64_t* msg_off,
                         const uint32_t* msg_len, size_t n, uint8_t* keys /* n x 32 */, const sv_opts* opts);

/* Verdicts AND cache keys from one staging of the batch (one H2D, two kernels
 * on one stream, one sync): the verifySigBatch miss path without any
 * per-signature host hashing. */
int sv_ed25519_verify_batch_keyed(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                                  const uint64_t* msg_off, const uint32_t* msg_len, size_t n, uint8_t* verdict,
                                  uint8_t* keys /* n x 32 */, const sv_opts* opts);

/* SHA-256 of n byte strings (data + off[i], len[i]): digests[32*i..].  Batch
 * form of the transaction contents hash, sha256(xdr(networkID, ENVELOPE_TYPE_TX,
 * tx)) at /root/reference/src/transactions/TransactionFrame.cpp:90-117. */
int sv_sha256_batch(const uint8_t* data, const uint64_t* off, const uint32_t* len, size_t n,
                    uint8_t* digests /* n x 32 */, const sv_opts* opts);

/* Device-resident forms (stream semantics as sv_ed25519_verify_device; pk, sig
 * and output buffers 4-byte aligned; fixed_len != 0 means item i's message is
 * d_msg + i * fixed_len and d_off / d_len are ignored). */
int sv_verify_cache_keys_device(int device, const void* d_pk, const void* d_sig, const void* d_msg,
                                const uint64_t* d_msg_off, const uint32_t* d_msg_len, uint32_t fixed_msg_len,
                                size_t n, void* d_keys, void* stream);
int sv_sha256_device(int device, const void* d_data, const uint64_t* d_off, const uint32_t* d_len,
                     uint32_t fixed_len, size_t n, void* d_digests, void* stream);

/* ---- Signatures straight from transaction bodies ------------------------
 * One device pass from transaction bytes to verdicts: the engine computes each
 * body's contents hash itself -- sha256(xdr_to_opaque(networkID, ENVELOPE_TYPE_TX,
 * tx)), TransactionFrame::getContentsHash /
 * FeeBumpTransactionFrame::getContentsHash -- and verifies the body's
 * signatures over it (csrc/sv_txhash.hip, then the verify kernels' 32-byte
 * mode on the same stream).  No caller-computed contents hash.
 *
 *   n_bodies bodies  body t = bodies[body_off[t] .. body_off[t] + body_len[t])
 *                    body_kind[t]: the hashed bytes are prefix || body, with
 *                      SV_TXBODY_V1       networkID || 00 00 00 02
 *                      SV_TXBODY_V0       networkID || 00 00 00 02 || 00 00 00 00
 *                      SV_TXBODY_FEE_BUMP networkID || 00 00 00 05
 *   n signatures     pk (n x 32), sig (n x 64), grouped by body in CSR form:
 *                    body t owns signatures sig_begin[t] .. sig_begin[t+1]-1;
 *                    sig_begin has n_bodies + 1 entries, is non-decreasing,
 *                    sig_begin[0] == 0, sig_begin[n_bodies] == n.  A body may
 *                    own no signature; it still gets a digest.
 *   verdict          n bytes out (may be NULL when n == 0)
 *   digests          optional, n_bodies x 32 bytes out
 * n == 0 with n_bodies > 0 is legal: only digests are produced.  A null
 * required pointer, a kind > 2 or a malformed sig_begin is SV_ERR_INVALID_ARG.
 *
 * Host buffers: the bodies go up in chunks of whole bodies, each of at most
 * the staging chunk of signatures (SV_STAGE_CHUNK) and SV_TXBODY_CHUNK_BYTES
 * (default 64 MiB) of body bytes (a larger single body is a chunk of its own),
 * double-buffered: chunk c+1 is packed and copied up while chunk c hashes and
 * verifies.  With opts->device == -1 the signatures are sliced over the slots
 * as for sv_ed25519_verify_batch; each slot hashes the bodies its slice
 * references (a body whose signatures straddle a boundary on both slots). */
#define SV_TXBODY_V1 0
#define SV_TXBODY_V0 1
#define SV_TXBODY_FEE_BUMP 2
int sv_ed25519_verify_txbodies(const uint8_t* network_id /* 32 B */, const uint8_t* bodies, const uint64_t* body_off,
                               const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                               const uint64_t* sig_begin, const uint8_t* pk, const uint8_t* sig, size_t n,
                               uint8_t* verdict, uint8_t* digests /* optional, n_bodies x 32 */,
                               const sv_opts* opts);
/* Device-resident form (stream semantics, d_bitmap and the 16-byte alignment
 * of d_pk / d_sig as sv_ed25519_verify_device; d_digests, optional, 16-byte
 * aligned).  network_id is host memory.  Bodies may start at any alignment
 * (16-byte aligned starts take the kernel's fast loads).  The device arrays
 * are not validated: kinds > 2 hash as fee bumps and signature ranges are
 * clamped to n.  The message array lives in the slot's workspace. */
int sv_ed25519_verify_txbodies_device(int device, const uint8_t* network_id /* host, 32 B */, const void* d_bodies,
                                      const uint64_t* d_body_off, const uint32_t* d_body_len,
                                      const uint8_t* d_body_kind, size_t n_bodies, const uint64_t* d_sig_begin,
                                      const void* d_pk, const void* d_sig, size_t n, void* d_verdict, void* d_bitmap,
                                      void* d_digests, void* stream);
/* The same computation on the engine's CPU path (what a caller runs when one
 * of the two above returns an error; threads as sv_ed25519_verify_batch_cpu). */
int sv_ed25519_verify_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                   const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                   const uint64_t* sig_begin, const uint8_t* pk, const uint8_t* sig, size_t n,
                                   uint8_t* verdict, uint8_t* digests /* optional */, int threads);

/* ---- Pairing by hint on the device --------------------------------------
 * A transaction carries DecoratedSignature{hint[4], signature[64]} and the
 * ledger supplies the candidate signer keys; which signature goes with which
 * key is decided by the hint, the last four bytes of the key
 * (SignatureUtils::doesHintMatch inside SignatureChecker::checkSignature).
 * These entry points take what a transaction has and do the pairing on the
 * device (csrc/sv_txpair.hip) between the contents hash and the verify launch.
 *
 *   bodies           as sv_ed25519_verify_txbodies
 *   n_sigs sigs      hint (n_sigs x 4), sig (n_sigs x 64); body t owns
 *                    signatures sig_begin[t] .. sig_begin[t+1]-1
 *   n_keys keys      key (n_keys x 32): body t's candidate ed25519 keys are
 *                    key_begin[t] .. key_begin[t+1]-1
 *                    (both CSR arrays: n_bodies + 1 entries, non-decreasing,
 *                    first 0, last the count; n_sigs, n_keys < 2^32)
 *   pair_cap         entries the three pair output arrays hold
 *   pair_begin       out, n_bodies + 1: body t's pairs are
 *                    pair_begin[t] .. pair_begin[t+1]-1
 *   pair_sig/key     out, global indices into sig / key
 *   pair_verdict     out, the verdict for (key[pair_key[i]], sig[pair_sig[i]],
 *                    contents hash of the body)
 *   *n_pairs         out, the number of pairs
 *   digests          optional, n_bodies x 32 bytes out
 *
 * A pair (s, k) exists iff s and k belong to the same body and hint[s] equals
 * bytes 28..31 of key[k].  Pairs are ordered by body, then signature, then key,
 * all ascending (a key listed twice in a body gives two pairs): the order is a
 * function of the input only.  n_sigs == 0, n_keys == 0 or zero pairs are legal
 * (digests are still produced; the pair arrays may be NULL when pair_cap == 0).
 * If the batch has more pairs than pair_cap the call returns SV_ERR_PAIR_CAP
 * with the exact number in *n_pairs; the pair outputs are then unspecified
 * (verdicts are never partial).  sv_txbodies_pair_bound gives a capacity that
 * always suffices.  Signatures of another length than 64 and signers that are
 * not ed25519 keys never reach these calls.
 *
 * Host buffers: chunks of whole bodies bounded by signatures and keys
 * (SV_STAGE_CHUNK each) and body bytes (SV_TXBODY_CHUNK_BYTES); per chunk the
 * engine waits once for the chunk's pair count before it launches the verify,
 * and packs the next chunk while that verify runs.  With opts->device == -1
 * the bodies are sliced over the slots at the body boundaries nearest to equal
 * shares of signatures (the minimum shard counts signatures); every body's
 * pairs and digest come from one slot, slot g's pairs follow slot g-1's. */
#define SV_ERR_PAIR_CAP (-8)
/* sum over the bodies of (signatures x keys): a pair_cap that always suffices
 * (0 for null arrays; saturates at SIZE_MAX) */
size_t sv_txbodies_pair_bound(const uint64_t* sig_begin, const uint64_t* key_begin, size_t n_bodies);
int sv_ed25519_verify_txbodies_hinted(const uint8_t* network_id /* 32 B */, const uint8_t* bodies,
                                      const uint64_t* body_off, const uint32_t* body_len, const uint8_t* body_kind,
                                      size_t n_bodies, const uint64_t* sig_begin, const uint8_t* hint,
                                      const uint8_t* sig, size_t n_sigs, const uint64_t* key_begin,
                                      const uint8_t* key, size_t n_keys, size_t pair_cap, uint64_t* pair_begin,
                                      uint32_t* pair_sig, uint32_t* pair_key, uint8_t* pair_verdict, size_t* n_pairs,
                                      uint8_t* digests /* optional, n_bodies x 32 */, const sv_opts* opts);
/* Device-resident form: every array is device memory on `device` (d_hint
 * 4-byte aligned; d_sig, d_key and the optional d_digests 16-byte aligned);
 * network_id and n_pairs are host memory.  d_pair_bitmap (optional) is laid out
 * as in sv_ed25519_verify_device over the n_pairs verdicts.  The number of
 * pairs is only known on the device, so this form WAITS on `stream` once, for
 * the count, after the hash and pairing kernels; it then enqueues the
 * verification and returns without waiting for it (stream ordering as
 * sv_ed25519_verify_device).  If the count exceeds pair_cap it returns
 * SV_ERR_PAIR_CAP (*n_pairs exact) and enqueues nothing more.  With
 * d_pair_verdict NULL (and no bitmap) the call stops after the pairing: the
 * pairs and digests are produced, nothing is verified.  The device
 * arrays are not validated: ranges are clamped to n_sigs / n_keys, kinds > 2
 * hash as fee bumps. */
int sv_ed25519_verify_txbodies_hinted_device(int device, const uint8_t* network_id /* host, 32 B */,
                                             const void* d_bodies, const uint64_t* d_body_off,
                                             const uint32_t* d_body_len, const uint8_t* d_body_kind, size_t n_bodies,
                                             const uint64_t* d_sig_begin, const void* d_hint, const void* d_sig,
                                             size_t n_sigs, const uint64_t* d_key_begin, const void* d_key,
                                             size_t n_keys, size_t pair_cap, uint64_t* d_pair_begin,
                                             uint32_t* d_pair_sig, uint32_t* d_pair_key, void* d_pair_verdict,
                                             void* d_pair_bitmap, size_t* n_pairs /* host */, void* d_digests,
                                             void* stream);
/* The same contract on the engine's CPU path (what a caller runs when one of
 * the two above returns an engine error; threads as sv_ed25519_verify_batch_cpu). */
int sv_ed25519_verify_txbodies_hinted_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                          const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                          const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                          size_t n_sigs, const uint64_t* key_begin, const uint8_t* key, size_t n_keys,
                                          size_t pair_cap, uint64_t* pair_begin, uint32_t* pair_sig,
                                          uint32_t* pair_key, uint8_t* pair_verdict, size_t* n_pairs,
                                          uint8_t* digests /* optional */, int threads);

/* ---- Signature checks decided on the device -----------------------------
 * What a caller wants from a transaction's signatures is not (signature, key,
 * verdict) triples but, per SignatureChecker::checkSignature call, "did this
 * check reach its needed weight" and, per transaction, "was every signature
 * used".  These entry points take each body's checks -- signer lists with
 * weights, and the needed weight -- next to what the hinted calls take, run the
 * hinted pipeline (contents hash, pairing by hint, verification) and then one
 * more kernel (csrc/sv_txcheck.hip, one lane per check) that replays every
 * check literally (csrc/txcheck.h: PRE_AUTH_TX, then HASH_X, then ED25519
 * signers; greedy over the signatures in order; a matched signer is erased;
 * success ends the check at once).  The pairs stay inside the engine: its
 * workspace is sized from the device's count, so there is no pair capacity and
 * no SV_ERR_PAIR_CAP here.
 *
 *   bodies, sigs, keys   as sv_ed25519_verify_txbodies_hinted.  PRE_AUTH_TX and
 *                    HASH_X signers' 32-byte keys sit in the body's key list
 *                    like ed25519 keys (a signature whose hint happens to match
 *                    one costs one wasted verification; only ED25519 signers
 *                    read verdicts)
 *   checks           the tables below
 *   check_ok         out, n_checks bytes: 1 if the check succeeded within the
 *                    PRE_AUTH_TX / HASH_X / ED25519 stages (with the payload
 *                    tables, below: within all four)
 *   check_weight     out, n_checks: the weight accumulated by those stages
 *                    (saturated at 2^32 - 1)
 *   check_used       out, n_checks: bit s set iff the check marked the body's
 *                    signature s (body-local index) used.  Checks are
 *                    independent: a body's used set is the OR over its checks
 *   digests          optional, n_bodies x 32 bytes out
 *
 * ED25519_SIGNED_PAYLOAD signers (type 3) come last in the reference.  Without
 * the payload tables (a plain sv_txchecks, or an sv_txchecks_payload whose
 * pkey_begin == NULL) they are accepted and skipped: for a check that came back 0 the
 * caller continues on the host from check_weight and the marks.  With the
 * tables the engine runs that fourth stage too (CAP-40,
 * SignatureUtils::verifyEd25519SignedPayload): each body has a second candidate
 * list, its signed-payload candidates (key, payload, payload length), a type-3
 * signer's signer_key is a global index into it, and a signer matches a
 * signature iff the signature's hint equals hint(key) XOR hint(payload)
 * (hint(payload): its last 4 bytes, or all of it followed by zeros when it is
 * shorter), the signature is 64 bytes long and it verifies over the payload
 * under the key.  The stage runs after the ED25519 stage with the weight carried
 * over, only if that stage did not succeed, at every protocol version (the
 * reference has no gate there), and check_ok / check_weight / check_used are
 * then the state after all four stages.  The (signature, payload candidate)
 * pairs are made by hint on the device (csrc/sv_txpair.hip) and verified by a
 * second, variable-length launch; like the ed25519 pairs they never leave the
 * engine.  A call whose tables are absent or hold no candidate launches and
 * copies exactly what it did before the tables existed.
 * With needed <= 0 a check without any match is still 0, as in the reference.
 * A check considers at most 64 signers and a body at most 64 signatures.
 *
 * The host forms validate everything before any device work
 * (SV_ERR_INVALID_ARG): a null required pointer, a malformed CSR array, a
 * signer type > 3, a key index outside its body's key range, a sig_len > 64, a
 * body with checks and more than 64 signatures, a check with more than 64
 * signers, protocol_version 7 (every check is true there without the engine);
 * with the payload tables also a malformed pkey_begin, a pkey_len > 64, a null
 * table with n_pkeys > 0, n_pkeys >= 2^32 and a type-3 signer whose index lies
 * outside its body's payload candidates.
 * Host buffers: chunks of whole bodies as in the hinted call, additionally
 * bounded by checks (SV_STAGE_CHUNK) and signers (8 x SV_STAGE_CHUNK); only the three check
 * arrays and the digests come back; a chunk carries its bodies' payload
 * candidates, which count towards its key bound.  With opts->device == -1 the bodies are
 * sliced as in the hinted call and each slot writes its checks' results
 * straight into the caller's arrays. */
typedef struct sv_txchecks {
  uint32_t struct_size;          /* sizeof(sv_txchecks) */
  uint32_t protocol_version;     /* weights clamp to 255 from 10 on; 7 is refused */
  const uint8_t* sig_len;        /* optional, n_sigs: signature lengths (rows stay 64 bytes, zero-padded); NULL: all 64 */
  const uint64_t* check_begin;   /* n_bodies + 1: body t's checks are check_begin[t] .. check_begin[t+1]-1 */
  const int32_t* check_needed;   /* n_checks */
  const uint64_t* signer_begin;  /* n_checks + 1: check c's signers, in list order */
  const uint8_t* signer_type;    /* n_signers: SV_SIGNER_* */
  const uint32_t* signer_weight; /* n_signers */
  const uint32_t* signer_key;    /* n_signers: global index into key, inside the body's key range */
  size_t n_checks;
  size_t n_signers;
} sv_txchecks;
/* sv_txchecks extended at its end by the payload tables.  A caller that has them fills this struct, sets
 * checks.struct_size = sizeof(sv_txchecks_payload) and passes &checks to the entry points below; every one of them
 * accepts struct_size >= sizeof(sv_txchecks) and reads the tables only when struct_size covers them and
 * pkey_begin != NULL.  (The extension has a name of its own so that a caller written against sv_txchecks, which
 * sets struct_size = sizeof(sv_txchecks) and may leave no zeroed bytes behind it, means the same after it is
 * recompiled.)  With the tables a type-3 signer's signer_key is a global index into pkey, inside its body's range. */
typedef struct sv_txchecks_payload {
  sv_txchecks checks;
  const uint64_t* pkey_begin;    /* n_bodies + 1: body t's payload candidates are pkey_begin[t] .. pkey_begin[t+1]-1 */
  const uint8_t* pkey;           /* n_pkeys x 32: signedPayload.ed25519 */
  const uint8_t* pkey_payload;   /* n_pkeys x 64: signedPayload.payload, rows zero-padded */
  const uint8_t* pkey_len;       /* n_pkeys: payload length, <= 64 */
  size_t n_pkeys;
} sv_txchecks_payload;
#define SV_SIGNER_KEY_ED25519 0
#define SV_SIGNER_KEY_PRE_AUTH_TX 1
#define SV_SIGNER_KEY_HASH_X 2
#define SV_SIGNER_KEY_ED25519_SIGNED_PAYLOAD 3
int sv_ed25519_check_txbodies(const uint8_t* network_id /* 32 B */, const uint8_t* bodies, const uint64_t* body_off,
                              const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                              const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                              const uint64_t* key_begin, const uint8_t* key, size_t n_keys, const sv_txchecks* checks,
                              uint8_t* check_ok, uint32_t* check_weight, uint64_t* check_used,
                              uint8_t* digests /* optional, n_bodies x 32 */, const sv_opts* opts);
/* Device-resident form: every array, those `checks` points to included, is
 * device memory on `device` (alignment as the hinted device form; the check
 * tables and outputs naturally aligned); network_id and the sv_txchecks struct
 * itself are host memory.  Stream semantics and the single wait for the pair
 * count are those of sv_ed25519_verify_txbodies_hinted_device; the check kernel
 * is enqueued after the verify launch and the call returns without waiting for
 * either.  The device arrays are not validated: every CSR range and key index
 * is clamped to its array (an out-of-range key index matches nothing, a check
 * no body owns is 0; a pkey_len above 64 is read as 64), and nothing is written
 * outside the three outputs.  With payload candidates the payload pairing runs
 * beside the ed25519 pairing and both counts come back in the one wait; pkey and
 * pkey_payload are 16-byte aligned. */
int sv_ed25519_check_txbodies_device(int device, const uint8_t* network_id /* host, 32 B */, const void* d_bodies,
                                     const uint64_t* d_body_off, const uint32_t* d_body_len,
                                     const uint8_t* d_body_kind, size_t n_bodies, const uint64_t* d_sig_begin,
                                     const void* d_hint, const void* d_sig, size_t n_sigs,
                                     const uint64_t* d_key_begin, const void* d_key, size_t n_keys,
                                     const sv_txchecks* checks /* host struct, device arrays */, void* d_check_ok,
                                     uint32_t* d_check_weight, uint64_t* d_check_used, void* d_digests, void* stream);
/* The same contract on the engine's CPU path (what a caller runs when one of
 * the two above returns an engine error, and the reference on a host without a
 * GPU; threads as sv_ed25519_verify_batch_cpu). */
int sv_ed25519_check_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                  const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                  const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                                  const uint64_t* key_begin, const uint8_t* key, size_t n_keys,
                                  const sv_txchecks* checks, uint8_t* check_ok, uint32_t* check_weight,
                                  uint64_t* check_used, uint8_t* digests /* optional */, int threads);

/* ---- Signature checks against a device-side account table ----------------
 * The calls above take every check spelled out: each body brings its own copy
 * of its candidate key rows and each check its own copy of its account's signer
 * list.  A ledger holds an account once, and a transaction's source check and
 * its operations' checks usually name the same account
 * (TransactionFrame::checkSignature builds the signer list from the account
 * entry: the master key with weight thresholds[0] if that is non-zero, then
 * acc.signers; the needed weight is a threshold level of the same entry).
 * These entry points take each account once, per body the accounts its checks
 * refer to, and per check WHICH account and WHICH threshold level; the engine
 * derives the explicit tables (csrc/txacct.h, on the device csrc/sv_txacct.hip)
 * and runs the pipeline above on them unchanged.
 *
 *   accounts         acct_key (n_accounts x 32, the account ID's ed25519 key),
 *                    acct_thresholds (n_accounts x 4: master weight, LOW, MED,
 *                    HIGH, as AccountEntry.thresholds); account a's signers are
 *                    asigner_begin[a] .. asigner_begin[a+1]-1: asigner_type
 *                    (SV_SIGNER_*), asigner_weight, asigner_key (x 32; for type
 *                    3 signedPayload.ed25519) and, read for type 3 only,
 *                    asigner_payload, an index into apayload (n_apayloads x 64,
 *                    rows zero-padded) / apayload_len (<= 64)
 *   per body         bacct[bacct_begin[t] .. bacct_begin[t+1]-1]: the accounts
 *                    body t's checks refer to, in any order; a duplicate only
 *                    repeats candidate rows and changes no result
 *   per check        check_acct: the position of its account inside its body's
 *                    bacct range; check_level 1, 2, 3: needed =
 *                    acct_thresholds[a][level]; 0: needed = check_needed[c]
 *                    (check_needed is read only there)
 *
 * Level 0 makes the checks without a ledger account pseudo-accounts of the
 * table: checkSignatureNoAccount is (master weight 1, no signers, needed 0),
 * checkExtraSigners is (master weight 0, the extra signers with weight 1,
 * needed = their count).
 *
 * The expansion is the definition.  Body t's candidate key list is, for each
 * of its accounts in bacct order, acct_key iff the master weight is > 0, then
 * the asigner_key of the account's signers of types 0-2 in list order; its
 * payload candidates are its accounts' type-3 signers in the same order, as
 * (key, payload, length).  Check c's signer list is (ED25519, master weight,
 * the master's row) iff the master weight is > 0, then the account's signers
 * in list order, a type-3 signer's signer_key being its index among the body's
 * payload candidates.  check_ok, check_weight, check_used and digests are by
 * definition those of sv_ed25519_check_txbodies* with an sv_txchecks_payload
 * over that expansion; the limits stay 64 signers per check and 64 signatures
 * per body.
 *
 * The host forms validate before any device work (SV_ERR_INVALID_ARG): a null
 * required pointer, a malformed CSR array, a bacct entry >= n_accounts, a
 * check_acct outside its body's range, a level > 3, a type > 3, a type-3
 * asigner_payload >= n_apayloads, an apayload_len > 64, an account whose
 * expanded list exceeds 64 signers, a body with checks and more than 64
 * signatures, a sig_len > 64, protocol 7, 2^32 or more rows of any table and a
 * struct_size that is too small.  The passes over the account table run once
 * per account, not once per use.
 * Host buffers: the account table goes up once per slot per call, ahead of the
 * first chunk; chunks are whole bodies with their signatures, bacct entries and
 * the three per-check arrays, bounded as in sv_ed25519_check_txbodies with the
 * EXPANDED key, payload-candidate and signer counts standing in for the
 * explicit ones.  opts->device == -1 slices the bodies as there. */
typedef struct sv_txaccounts {
  uint32_t struct_size;            /* sizeof(sv_txaccounts) */
  uint32_t protocol_version;       /* as sv_txchecks */
  const uint8_t* sig_len;          /* optional, n_sigs, as sv_txchecks */
  const uint8_t* acct_key;         /* n_accounts x 32 */
  const uint8_t* acct_thresholds;  /* n_accounts x 4 */
  const uint64_t* asigner_begin;   /* n_accounts + 1 */
  const uint8_t* asigner_type;     /* n_asigners */
  const uint32_t* asigner_weight;  /* n_asigners */
  const uint8_t* asigner_key;      /* n_asigners x 32 */
  const uint32_t* asigner_payload; /* n_asigners (may be NULL when no signer has type 3) */
  const uint8_t* apayload;         /* n_apayloads x 64 */
  const uint8_t* apayload_len;     /* n_apayloads */
  const uint64_t* bacct_begin;     /* n_bodies + 1 */
  const uint32_t* bacct;           /* n_bacct */
  const uint64_t* check_begin;     /* n_bodies + 1 */
  const uint32_t* check_acct;      /* n_checks */
  const uint8_t* check_level;      /* n_checks */
  const int32_t* check_needed;     /* n_checks (may be NULL when no check has level 0) */
  size_t n_accounts, n_asigners, n_apayloads, n_bacct, n_checks;
} sv_txaccounts;
int sv_ed25519_check_txbodies_accounts(const uint8_t* network_id /* 32 B */, const uint8_t* bodies,
                                       const uint64_t* body_off, const uint32_t* body_len, const uint8_t* body_kind,
                                       size_t n_bodies, const uint64_t* sig_begin, const uint8_t* hint,
                                       const uint8_t* sig, size_t n_sigs, const sv_txaccounts* accts,
                                       uint8_t* check_ok, uint32_t* check_weight, uint64_t* check_used,
                                       uint8_t* digests /* optional, n_bodies x 32 */, const sv_opts* opts);
/* Device-resident form: every array, those `accts` points to included, is
 * device memory on `device` (d_sig, acct_key, asigner_key, apayload and the
 * optional d_digests 16-byte aligned, the others naturally); network_id and
 * the struct itself are host memory.  Nothing is validated: every range and
 * index is clamped to its array -- a bacct entry >= n_accounts contributes
 * nothing, a check whose check_acct lies outside its body's range or names such
 * an entry has no signer and is 0, a level above 3 reads as 3, a payload index
 * >= n_apayloads reads as the empty payload, a check considers its first 64
 * signers -- and nothing is written outside the three outputs (and d_digests).
 * With asigner_payload or check_needed NULL, type-3 signers read the empty
 * payload and level-0 checks need 0.  The expanded tables live in the slot's
 * workspace.  Their three row counts are only known on the device, so this form
 * WAITS on `stream` once more than sv_ed25519_check_txbodies_device does: once
 * for the three totals (before it sizes the row arrays), then once for the pair
 * counts. */
int sv_ed25519_check_txbodies_accounts_device(int device, const uint8_t* network_id /* host, 32 B */,
                                              const void* d_bodies, const uint64_t* d_body_off,
                                              const uint32_t* d_body_len, const uint8_t* d_body_kind, size_t n_bodies,
                                              const uint64_t* d_sig_begin, const void* d_hint, const void* d_sig,
                                              size_t n_sigs, const sv_txaccounts* accts /* host struct, device arrays */,
                                              void* d_check_ok, uint32_t* d_check_weight, uint64_t* d_check_used,
                                              void* d_digests, void* stream);
/* The same contract on the engine's CPU path: the expansion on the host, then
 * sv_ed25519_check_txbodies_cpu over it. */
int sv_ed25519_check_txbodies_accounts_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                           const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                           const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                           size_t n_sigs, const sv_txaccounts* accts, uint8_t* check_ok,
                                           uint32_t* check_weight, uint64_t* check_used,
                                           uint8_t* digests /* optional */, int threads);

/* ---- One signature result per transaction body -----------------------------
 * A caller of the check calls above folds every body's checks once more: the
 * result code comes from the first failing check, the used marks are ORed over
 * the body's checks (TransactionFrame::processSignatures, commonValid,
 * checkAllSignaturesUsed).  The decide calls make that fold on the device
 * (csrc/txresult.h, csrc/sv_txresult.hip) behind the check kernel and return
 * one byte per body -- and, on request, the ascending list of the bodies that
 * are not OK, which for a valid set is empty.
 *
 * Body t has the checks check_begin[t] .. check_begin[t+1]-1 and
 * ns = min(sig_begin[t+1] - sig_begin[t], 64) signatures.  With
 *   fail   the body-local index of its first check, in list order, whose
 *          check_ok != 1 (anything but 1 fails), or SV_TXRESULT_NONE
 *   used   the OR of check_used over all of its checks
 *   want   ns >= 64 ? ~0 : (1 << ns) - 1
 * body_code[t] is SV_TXRESULT_BAD_AUTH if a check failed and check_role[fail]
 * is SV_TXROLE_TX (the source account at LOW, the extra signers, a fee bump's
 * fee source); SV_TXRESULT_OP_BAD_AUTH if its role is SV_TXROLE_OP (an
 * operation's check: txFAILED with opBAD_AUTH); otherwise
 * SV_TXRESULT_BAD_AUTH_EXTRA if (used & want) != want and body_flags[t] has
 * SV_TXBODY_SKIP_UNUSED clear; otherwise SV_TXRESULT_OK.  body_fail[t] is
 * `fail`.  A body without checks but with signatures is BAD_AUTH_EXTRA.
 * SKIP_UNUSED is processSignatures below protocol 10, which returns before
 * checkAllSignaturesUsed.  All checks are evaluated where the reference stops
 * at the first failing one: checks are independent and only the first failure
 * and the OR are read, so no result changes.  A fee bump's outer and inner
 * body are two bodies here; combining the two bytes stays with the caller.
 *
 * Each entry point has the argument list of its check twin with
 * `const sv_txresults*` in place of the three check outputs, and its results
 * are by definition the fold above of what the twin returns on the same input;
 * requested check_* outputs and the digests are byte-equal to the twin's.
 *
 * Host forms: everything the twin refuses, and before any device work
 * (SV_ERR_INVALID_ARG) a role > 1, a flag bit other than bit 0, a null
 * body_code, a struct_size that is too small, bad_body == NULL with
 * bad_cap > 0.  A chunk carries its roles and flags; the result kernel follows
 * the check kernel on the same stream; only body_code and the outputs that
 * were asked for come back (the 13 bytes per check stay on the device unless
 * requested).  bad_body holds global body indices and is built on the host
 * from body_code after the last chunk; *n_bad is exact even above bad_cap.
 * Device forms: everything `res` points to is device memory, n_bad included;
 * the struct is host memory.  The call waits no more often than its twin.
 * Nothing is validated: a role > 1 reads as OP, unknown flag bits are ignored,
 * ranges are clamped, entries at or past bad_cap are never written.  check_ok
 * and check_used that are not requested live in the slot's workspace.
 * CPU forms: the twin's CPU path, then csrc/txresult.h. */
#define SV_TXRESULT_OK 0
#define SV_TXRESULT_BAD_AUTH 1
#define SV_TXRESULT_OP_BAD_AUTH 2
#define SV_TXRESULT_BAD_AUTH_EXTRA 3
#define SV_TXRESULT_NONE 0xFFFFFFFFu
#define SV_TXROLE_TX 0
#define SV_TXROLE_OP 1
#define SV_TXBODY_SKIP_UNUSED 1
typedef struct sv_txresults {
  uint32_t struct_size;        /* sizeof(sv_txresults) */
  const uint8_t* check_role;   /* n_checks, SV_TXROLE_*; NULL: every check SV_TXROLE_TX */
  const uint8_t* body_flags;   /* n_bodies; NULL: 0 */
  uint8_t* body_code;          /* out, n_bodies, required */
  uint32_t* body_fail;         /* out, n_bodies, optional */
  uint8_t* check_ok;           /* out, optional each: NULL = not returned */
  uint32_t* check_weight;
  uint64_t* check_used;
  uint32_t* bad_body;          /* out, optional: ascending failing bodies */
  size_t bad_cap;
  uint64_t* n_bad;             /* out, optional */
} sv_txresults;
int sv_ed25519_decide_txbodies(const uint8_t* network_id /* 32 B */, const uint8_t* bodies, const uint64_t* body_off,
                               const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                               const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                               const uint64_t* key_begin, const uint8_t* key, size_t n_keys, const sv_txchecks* checks,
                               const sv_txresults* res, uint8_t* digests /* optional, n_bodies x 32 */,
                               const sv_opts* opts);
int sv_ed25519_decide_txbodies_device(int device, const uint8_t* network_id /* host, 32 B */, const void* d_bodies,
                                      const uint64_t* d_body_off, const uint32_t* d_body_len,
                                      const uint8_t* d_body_kind, size_t n_bodies, const uint64_t* d_sig_begin,
                                      const void* d_hint, const void* d_sig, size_t n_sigs,
                                      const uint64_t* d_key_begin, const void* d_key, size_t n_keys,
                                      const sv_txchecks* checks /* host struct, device arrays */,
                                      const sv_txresults* res /* host struct, device arrays */, void* d_digests,
                                      void* stream);
int sv_ed25519_decide_txbodies_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                   const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                   const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig, size_t n_sigs,
                                   const uint64_t* key_begin, const uint8_t* key, size_t n_keys,
                                   const sv_txchecks* checks, const sv_txresults* res,
                                   uint8_t* digests /* optional */, int threads);
int sv_ed25519_decide_txbodies_accounts(const uint8_t* network_id /* 32 B */, const uint8_t* bodies,
                                        const uint64_t* body_off, const uint32_t* body_len, const uint8_t* body_kind,
                                        size_t n_bodies, const uint64_t* sig_begin, const uint8_t* hint,
                                        const uint8_t* sig, size_t n_sigs, const sv_txaccounts* accts,
                                        const sv_txresults* res, uint8_t* digests /* optional, n_bodies x 32 */,
                                        const sv_opts* opts);
int sv_ed25519_decide_txbodies_accounts_device(int device, const uint8_t* network_id /* host, 32 B */,
                                               const void* d_bodies, const uint64_t* d_body_off,
                                               const uint32_t* d_body_len, const uint8_t* d_body_kind, size_t n_bodies,
                                               const uint64_t* d_sig_begin, const void* d_hint, const void* d_sig,
                                               size_t n_sigs, const sv_txaccounts* accts /* host struct, device arrays */,
                                               const sv_txresults* res /* host struct, device arrays */,
                                               void* d_digests, void* stream);
int sv_ed25519_decide_txbodies_accounts_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                            const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                            const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                            size_t n_sigs, const sv_txaccounts* accts, const sv_txresults* res,
                                            uint8_t* digests /* optional */, int threads);

/* ---- Accounts that stay on the device; checks that name them by ID ---------
 * The by-account calls above take the account table per call, and the caller
 * turns every account ID it reads out of a transaction into an index into the
 * table it built for that call.  The reference never rebuilds account state per
 * batch: its checks read ledger entries that live from one ledger to the next
 * (TransactionFrame::loadSourceAccount, OperationFrame::loadSourceAccount,
 * stellar::loadAccount) and change by deltas at ledger close.  The account
 * store is that state for the engine: a host-authoritative table of accounts
 * (csrc/acctstore.h) with one read-only replica per device slot
 * (csrc/sv_txstore.hip), off by default -- nothing is allocated and no new code
 * runs until sv_set_account_store turns it on.
 *
 * sv_set_account_store(accounts, payloads, local_accounts): capacity in
 * accounts (0: off, everything freed), in 64-byte payload rows for type-3
 * signers, and the rows past the capacity a ledger call may borrow for its own
 * local accounts (below).  Process-wide; replaces (and empties) an existing
 * store.  An account has at most 20 signers (MAX_SIGNERS).  Memory: 948 bytes
 * per account, 65 per payload row and 4 per index slot (a power of two of slots
 * >= 2 x accounts, at least 8), on the host and on every slot that has used the
 * store -- there for accounts + local_accounts rows and payloads +
 * 20 x local_accounts payload rows; sv_workspace_bytes and the stats count it.
 * The index is seeded from std::random_device (SV_ACCT_STORE_SEED fixes the
 * seed).
 * sv_account_store_upsert: reads only acct_*, asigner_*, apayload*, n_accounts,
 * n_asigners and n_apayloads of `table`.  An ID the store holds is replaced in
 * place (no stale signer stays visible, its payload rows are freed); within one
 * call the last row of a duplicate ID wins.  sv_account_store_erase: an absent
 * ID is no error (it is counted).  Both are all-or-nothing: SV_ERR_INVALID_ARG
 * for a batch that breaks a per-account rule of the by-account host forms (type
 * > 3, payload index >= n_apayloads, apayload_len > 64, malformed
 * asigner_begin) or has an account with more than 20 signers, or with the store
 * off; SV_ERR_ALLOC when the new accounts or payload rows do not fit; in both
 * cases nothing changes, on the host or on any replica, the counters included.
 * A write returns when every replica holds it (each slot: staged rows up, one
 * scatter kernel on the slot's stream under its lock, wait), so no check call
 * sees half of it; a slot that first uses the store later starts from the host
 * copy.  Writers are serialised.  sv_set_device_map and sv_shutdown drop the
 * replicas AND the store.
 * sv_account_store_read: n accounts by ID in a fixed layout (absent: found 0,
 * zeros), from the host copy (device -1) or from slot `device`'s replica by its
 * lookup kernel and a gather -- how a caller (and the tests) see what the device
 * holds.  Any output may be NULL.  The host side (set, upsert, erase, clear,
 * read with device -1, stats with device -1, the _cpu forms) needs no GPU. */
int sv_set_account_store(size_t accounts, size_t payloads, size_t local_accounts);
int sv_account_store_upsert(const sv_txaccounts* table);
int sv_account_store_erase(const uint8_t* ids /* n x 32 */, size_t n);
int sv_account_store_clear(void);
typedef struct sv_account_store_stats {
  uint64_t struct_size;      /* in: sizeof(sv_account_store_stats) of the caller */
  uint64_t capacity;         /* accounts (0: off) */
  uint64_t accounts;         /* held now */
  uint64_t payload_capacity; /* payload rows */
  uint64_t payloads;         /* in use now */
  uint64_t local_accounts;
  uint64_t index_slots;
  uint64_t max_probe;        /* the bound every lookup's loop gets */
  uint64_t upsert_calls, inserted, replaced; /* accepted upserts; accounts new / overwritten */
  uint64_t erase_calls, erased, erase_absent;
  uint64_t host_bytes;
  /* of slot `device` (0 with device -1, or before the slot's first use of the store) */
  uint64_t device_bytes;
  uint64_t replica_current;  /* 1: the replica holds every write so far */
  uint64_t lookups;          /* entries its lookup kernel resolved */
  double lookup_ms;          /* ... and that kernel's device time (sv_timing_enable) */
} sv_account_store_stats;
int sv_account_store_get_stats(int device /* -1: the host side only */, sv_account_store_stats* out);
int sv_account_store_read(int device /* -1: the host copy */, const uint8_t* ids /* n x 32 */, size_t n,
                          uint8_t* found /* n */, uint8_t* thresholds /* n x 4 */, uint32_t* n_signers /* n */,
                          uint8_t* signer_type /* n x 20 */, uint32_t* signer_weight /* n x 20 */,
                          uint8_t* signer_key /* n x 20 x 32 */, uint8_t* signer_payload /* n x 20 x 64 */,
                          uint8_t* signer_payload_len /* n x 20 */);

/* Checks that name store accounts by ID.  Each entry point has the argument
 * list of its _accounts twin with `const sv_txledger*` in place of
 * `const sv_txaccounts*`.  accts is exactly the twin's struct; its account
 * table is this call's LOCAL accounts (may be empty): the pseudo-accounts of
 * checkSignatureNoAccount and checkExtraSigners, as today.  A bacct entry is
 * a local account's index, or SV_BACCT_BY_ID: the store account whose ID is
 * bacct_id[32 e .. 32 e + 31].
 *
 * The expansion stays the definition.  Let the twin's table be the local
 * accounts followed by the store's accounts; replace every SV_BACCT_BY_ID entry
 * by the index of the account with that ID, and an ID the store does not hold
 * by an empty account (master weight 0, no signers, thresholds 0).  The results
 * are byte for byte the twin's on that input.  An entry that is not found
 * contributes no candidate row and a check that names it has no signer and is
 * 0; bacct_found lets the caller turn that into txNO_ACCOUNT / opNO_ACCOUNT,
 * which the reference decides before it looks at a signature.
 *
 * Host forms (host buffers): a third source of the chunk pipeline beside the
 * explicit and the by-account one.  Before any device work the call's entries
 * are resolved on the HOST index into replica rows, with the per-account row
 * counts read from the host copy, so the planner knows the expanded counts
 * exactly and the form waits no more often than its twin does.  Each slot
 * uploads only the local accounts, once per call, into the borrowed rows; a
 * chunk carries 4 bytes per entry as in the by-account form; the IDs never
 * cross PCIe.  The store cannot be written while such a call runs (a writer
 * waits for it).  opts->device == -1 slices the bodies as in the twin.
 * CPU forms: the expansion on the host over the host copy, then the twin's CPU
 * path; no device is touched.
 * The host and CPU forms refuse (SV_ERR_INVALID_ARG) a call with the store off,
 * more than local_accounts local accounts, a local account with more than 20
 * signers, a bacct entry that is neither SV_BACCT_BY_ID nor a local index, an
 * entry by ID with bacct_id NULL, and everything the twin refuses.  bacct_found
 * is written only by a call that is accepted.
 * Device forms: every array, bacct_id and bacct_found included, is device
 * memory (bacct_id 16-byte aligned); the structs are host memory.  The slot's
 * replica is the account table: the local accounts are written into the
 * borrowed rows by a small kernel, a lookup kernel (one lane per entry, at most
 * max_probe slots probed, all 32 bytes compared) resolves every entry to a row,
 * and the twin's sequence runs unchanged on that table -- no store row is
 * copied per call, and the call waits exactly as often as its twin.  Nothing is
 * validated beyond the store being on (off: SV_ERR_INVALID_ARG): local
 * accounts past local_accounts and signers past an account's first 20 are not
 * read, a bacct entry that is neither by ID nor a local index names no account
 * (found 0), with bacct_id NULL no ID is found, and every other clamp is the
 * twin's.  A write to the store and a
 * device-form call exclude each other by the slot's lock: a call queued after
 * sv_account_store_upsert returned sees the new rows. */
#define SV_BACCT_BY_ID 0xFFFFFFFFu
typedef struct sv_txledger {
  uint32_t struct_size;        /* sizeof(sv_txledger) */
  uint32_t reserved;           /* 0 */
  const sv_txaccounts* accts;
  const uint8_t* bacct_id;     /* n_bacct x 32; read for the entries whose bacct[e] == SV_BACCT_BY_ID */
  uint8_t* bacct_found;        /* out, optional, n_bacct: 1 = local entry or ID held by the store, 0 = not held */
} sv_txledger;
int sv_ed25519_check_txbodies_ledger(const uint8_t* network_id /* 32 B */, const uint8_t* bodies,
                                     const uint64_t* body_off, const uint32_t* body_len, const uint8_t* body_kind,
                                     size_t n_bodies, const uint64_t* sig_begin, const uint8_t* hint,
                                     const uint8_t* sig, size_t n_sigs, const sv_txledger* ledger, uint8_t* check_ok,
                                     uint32_t* check_weight, uint64_t* check_used,
                                     uint8_t* digests /* optional, n_bodies x 32 */, const sv_opts* opts);
int sv_ed25519_decide_txbodies_ledger(const uint8_t* network_id /* 32 B */, const uint8_t* bodies,
                                      const uint64_t* body_off, const uint32_t* body_len, const uint8_t* body_kind,
                                      size_t n_bodies, const uint64_t* sig_begin, const uint8_t* hint,
                                      const uint8_t* sig, size_t n_sigs, const sv_txledger* ledger,
                                      const sv_txresults* res, uint8_t* digests /* optional, n_bodies x 32 */,
                                      const sv_opts* opts);
int sv_ed25519_check_txbodies_ledger_device(int device, const uint8_t* network_id /* host, 32 B */,
                                            const void* d_bodies, const uint64_t* d_body_off,
                                            const uint32_t* d_body_len, const uint8_t* d_body_kind, size_t n_bodies,
                                            const uint64_t* d_sig_begin, const void* d_hint, const void* d_sig,
                                            size_t n_sigs, const sv_txledger* ledger /* host structs, device arrays */,
                                            void* d_check_ok, uint32_t* d_check_weight, uint64_t* d_check_used,
                                            void* d_digests, void* stream);
int sv_ed25519_check_txbodies_ledger_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                         const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                         const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                         size_t n_sigs, const sv_txledger* ledger, uint8_t* check_ok,
                                         uint32_t* check_weight, uint64_t* check_used,
                                         uint8_t* digests /* optional */, int threads);
int sv_ed25519_decide_txbodies_ledger_device(int device, const uint8_t* network_id /* host, 32 B */,
                                             const void* d_bodies, const uint64_t* d_body_off,
                                             const uint32_t* d_body_len, const uint8_t* d_body_kind, size_t n_bodies,
                                             const uint64_t* d_sig_begin, const void* d_hint, const void* d_sig,
                                             size_t n_sigs, const sv_txledger* ledger /* host structs, device arrays */,
                                             const sv_txresults* res /* host struct, device arrays */,
                                             void* d_digests, void* stream);
int sv_ed25519_decide_txbodies_ledger_cpu(const uint8_t* network_id, const uint8_t* bodies, const uint64_t* body_off,
                                          const uint32_t* body_len, const uint8_t* body_kind, size_t n_bodies,
                                          const uint64_t* sig_begin, const uint8_t* hint, const uint8_t* sig,
                                          size_t n_sigs, const sv_txledger* ledger, const sv_txresults* res,
                                          uint8_t* digests /* optional */, int threads);

/* ---- Warm-key latency path (csrc/comb.h, csrc/sv_comb.hip) ---------------
 * Each device slot keeps a bounded cache of per-public-key tables
 * ({0..8} * 16^j * (-A), 108 KiB per key) in HBM.  A latency-path host batch
 * whose keys are all cached runs the comb kernel: libsodium's equation
 * [S]B + [h](-A) == R evaluated as a sum of 96 table entries, no scalar
 * multiplication.  Any other batch runs the octet kernel, after which its
 * keys (on their second sighting) are built on a low-priority stream for the
 * next batch.  Verdicts are identical on both kernels; the cache holds only
 * data derived from public keys.  Default capacity 1024 keys (or the
 * SV_KEY_CACHE environment variable); 0 disables the warm path.  Drains and
 * clears every slot's cache. */
int sv_set_key_cache(size_t capacity);
/* Blocks until every key-table build queued on `device` has finished. */
int sv_key_cache_wait(int device);
typedef struct sv_key_cache_stats {
  uint64_t capacity;     /* keys the cache holds at most */
  uint64_t keys;         /* keys cached or being built */
  uint64_t warm_batches; /* latency-lane batches served by the comb kernel */
  uint64_t cold_batches; /* latency-lane batches served by the octet kernel */
  uint64_t keys_built;   /* key-table builds queued */
  uint64_t evictions;
  uint64_t shared_launches; /* bulk (throughput-path) launches that ran in shared
                               mode because latency batches were live: they leave
                               one workgroup slot per CU to the latency lane
                               (window SV_LAT_SHARE_MS, default 1000; 0: off) */
  uint64_t table_launches;  /* throughput-path launches that used the per-key tables */
  uint64_t table_keys;      /* keys claimed in them since the tables were last cleared
                               (as of the last launch whose counters came back) */
  uint64_t table_clears;    /* times the claim words were cleared (claims reached half the slots) */
  uint64_t table_slots;     /* slots of the per-key tables */
} sv_key_cache_stats;
int sv_key_cache_get_stats(int device, sv_key_cache_stats* out);

/* ---- Verdict cache (csrc/vcache.h, csrc/sv_vcache.hip) --------------------
 * The twin of stellar-core's gVerifySigCache (PubKeyUtils::verifySig) for the
 * calls whose signatures are paired and verified on the device: every
 * sv_ed25519_verify_txbodies_hinted*, sv_ed25519_check_txbodies* and
 * sv_ed25519_decide_txbodies* form, and sv_ed25519_verify_device_cached.  Each
 * device slot keeps a 4-way set-associative table of verdicts in HBM, keyed by
 * all 32 bytes of BLAKE2b-256(pk || sig || msg) (sv_verify_cache_keys); accepts
 * and rejects are both cached.  A launch looks every item up first, verifies
 * only the misses and inserts their verdicts.  Verdicts and every other output
 * are the same for any capacity and any history; only the work changes.
 *
 *   OFF BY DEFAULT (capacity 0, or the SV_VERDICT_CACHE environment variable):
 *   then no call allocates, launches or waits for anything more than before.
 *   Cost: 52 bytes of device memory per entry and slot, plus a compaction
 *   workspace of about 170 bytes per item of the largest cached launch.
 *   While it is on, every cached launch WAITS once on the slot's kernel stream
 *   for its miss count; the host-buffer chunk loops wait once more per chunk.
 *   Per slot: a table only knows what its own slot verified, so a repeated
 *   batch hits only where it is sliced over the slots the same way
 *   (sv_set_verdict_cache_share, below, is the opt-in that lifts this).
 *   The raw host-buffer batch calls and the latency lane look nothing up and,
 *   by default, store nothing.  sv_set_verdict_cache_feed (below) lets keyed
 *   batches FEED the table: what the latency lane verified is journaled and
 *   inserted ahead of the next cached launch, so a tx-body call over pairs
 *   that sv_ed25519_verify_batch_keyed / _gather* already verified on this
 *   slot is a warm pass; keyed bulk-route batches can go behind the cache.
 *
 * sv_set_verdict_cache: entries per slot, rounded up to a power of two >= 4;
 * 0 turns the cache off.  Drains and clears every slot (tables, workspace and
 * counters are freed).  Above SV_VERDICT_CACHE_MAX: SV_ERR_INVALID_ARG.
 * sv_verdict_cache_clear: empties every slot's table (clearVerifySigCache);
 * the counters stay.  sv_verdict_cache_get_stats waits for the slot's kernel
 * stream; the counters count since the capacity was last set
 * (flushVerifySigCacheCounts, without the reset). */
#define SV_VERDICT_CACHE_MAX ((size_t)1 << 24)
int sv_set_verdict_cache(size_t entries);
int sv_verdict_cache_clear(void);
typedef struct sv_verdict_cache_stats {
  uint64_t struct_size; /* in: sizeof(sv_verdict_cache_stats) of the caller */
  uint64_t entries;     /* the capacity in force (0: off) */
  uint64_t lookups;     /* items probed */
  uint64_t hits;        /* ... whose verdict came from the table */
  uint64_t inserted;    /* verdicts stored (an eviction where the set was full) */
  uint64_t dropped;     /* misses not stored: another item of the batch won the slot */
  uint64_t bytes;       /* device memory the slot's cache holds now */
  double kernel_ms;     /* time of the cache's own kernels (only while sv_timing_enable is on) */
  double wait_ms;       /* host time spent waiting for miss counts */
  /* the feed (sv_set_verdict_cache_feed); written only where struct_size covers them.  Journal drains move
   * none of lookups / hits / inserted / dropped. */
  uint64_t fed_rows;     /* rows appended to the slot's journal */
  uint64_t fed_overflow; /* rows not appended because the journal was full */
  uint64_t fed_present;  /* drained rows whose key the table already held */
  uint64_t fed_inserted; /* drained rows stored */
  uint64_t fed_dropped;  /* drained rows that lost their claim to another row of the drain */
  /* one view across slots (sv_set_verdict_cache_share); written only where struct_size covers them */
  /*   shared_out           rows this slot offered to the others, once per row and not once per peer
   *   shared_in            rows other slots appended to this slot's journal (also counted in fed_rows)
   *   shared_skipped       rows of this slot's launches not offered: a launch with more misses than a journal
   *                        holds, every export buffer still pending, or an export that could not be made (it
   *                        never fails the call)
   *   shared_pinned_bytes  pinned host memory this slot holds for exports now
   * (one declaration of four words, in this order: everything above it is the struct as callers built before
   * sv_set_verdict_cache_share know it) */
  uint64_t shared_out, shared_in, shared_skipped, shared_pinned_bytes;
} sv_verdict_cache_stats;
int sv_verdict_cache_get_stats(int device, sv_verdict_cache_stats* out);

/* Feeding the verdict cache from keyed batches.  OFF BY DEFAULT (sources 0, or
 * the SV_VERDICT_CACHE_FEED / SV_VERDICT_CACHE_JOURNAL environment variables):
 * then every call allocates, launches, waits and returns exactly as without it.
 * No verdict ever depends on the feed, and the table still holds only verdict
 * bytes that a completed verify launch of this engine wrote: there is no call
 * that inserts a verdict by key.
 *   SV_VC_FEED_LANE  a keyed latency-lane batch (sv_ed25519_verify_batch_keyed
 *     / _gather* with keys, at most 12,288 signatures on one slot) that returned
 *     SV_OK appends its (key, verdict) rows to the slot's journal: a bounded
 *     array in ordinary host memory, journal_rows rows of 33 bytes per slot
 *     (0: 65,536 rows, 2.1 MB; at most 2^24).  A batch that does not fit
 *     appends its leading rows, the rest counts as fed_overflow and is simply
 *     not cached.  An error return appends nothing; an unkeyed batch appends
 *     nothing.  The journal is DRAINED into the table -- an upload and two
 *     kernels on the slot's bulk stream, nothing when it is empty -- ahead of
 *     the probe of every cached launch, by sv_verdict_cache_sync and by the
 *     lookups below.  The latency lane itself never reads or writes the table.
 *     A drained row whose key the table holds changes nothing (fed_present);
 *     the others are inserted by the policy of csrc/vcache.h, in journal order.
 *   SV_VC_FEED_BULK  keyed host-buffer batches on the bulk route (more than
 *     12,288 signatures, or a forced throughput path) run behind the cache as
 *     the tx-body forms do: probe, verify the misses, insert.  One more wait
 *     per chunk; verdicts, keys and the keys-ready callbacks are unchanged.
 * sv_set_verdict_cache_feed is process-wide; it drops what the journals hold.
 * Unknown bits, or journal_rows above 2^24: SV_ERR_INVALID_ARG.  With the cache
 * off the setting is remembered and nothing else happens.  The journals are
 * also dropped by sv_set_verdict_cache, sv_verdict_cache_clear,
 * sv_set_device_map and sv_shutdown.
 * sv_verdict_cache_sync: drains the slot's journal now and returns when the
 * inserts are done.  With the cache off it does nothing.
 * sv_verdict_cache_lookup*: drain, then per key the verdict the slot's table
 * holds (0 or 1) or SV_VC_MISS.  They change nothing in the table and nothing
 * in lookups / hits.  With the cache off every byte is SV_VC_MISS.  The host
 * form returns when `out` is written; n == 0 is SV_OK, a null pointer
 * SV_ERR_INVALID_ARG, and on a host without a GPU it returns the error every
 * host form returns there (SV_ERR_NO_DEVICE), cache on or off.  The device
 * form (d_keys n x 32 and 16-byte aligned, else SV_ERR_ALIGN; d_out n bytes)
 * is ordered on `stream` like sv_ed25519_verify_device, does not wait for the
 * result or for anything `stream` holds (its drain may wait on the host for the
 * slot's own earlier work: a growing workspace, the previous drain's upload)
 * and writes nothing outside d_out[0, n). */
#define SV_VC_FEED_LANE 1u /* keyed latency-lane batches are journaled */
#define SV_VC_FEED_BULK 2u /* keyed host-buffer batches on the bulk route are cached */
int sv_set_verdict_cache_feed(uint32_t sources, size_t journal_rows);
int sv_verdict_cache_sync(int device);
#define SV_VC_MISS 0xFFu
int sv_verdict_cache_lookup(int device, const uint8_t* keys /* n x 32 */, size_t n, uint8_t* out /* n */);
int sv_verdict_cache_lookup_device(int device, const void* d_keys, size_t n, void* d_out, void* stream);
/* One view across slots (csrc/vshare.h).  A table only knows what its own slot verified; with several slots in
 * one process a keyed lane batch is served by one slot and a tx set is sliced over all of them, and two overlapping
 * sets slice their common transactions differently.  sv_set_verdict_cache_share lets the slots tell each other.
 * OFF BY DEFAULT (0, or the SV_VERDICT_CACHE_SHARE environment variable): then no call allocates, launches,
 * copies, waits or returns anything different.  With one slot both bits do nothing at all.  Verdicts and every
 * other output are the same for any setting; a table still holds only verdict bytes that a completed verify
 * launch of this engine wrote, and every row still enters a table through its slot's journal and drain alone.
 *   SV_VC_SHARE_FEED    (acts only while SV_VC_FEED_LANE is set) a journaled keyed lane batch is appended to every
 *     slot's journal, not only its own, from the same pinned copies; every journal has its own bound and counts
 *     its own fed_overflow.  G journal copies on the batch's return path where there was one.
 *   SV_VC_SHARE_STORES  (needs no feed bit) a cached launch with misses also EXPORTS them: a kernel behind the
 *     insert gathers the leading min(misses, journal_rows) rows of the miss list -- keys and verdict bytes, in
 *     item order, whether this slot stored or dropped them; hits and rows learned through a drain are never
 *     exported, so nothing echoes -- and one copy takes them to pinned host memory, with an event behind it.  Once
 *     the event has completed the rows are appended to every other slot's journal, in export order per exporter,
 *     by whichever cache entry point comes by: a cached launch, a lookup, the stats or a sync on any slot (an event
 *     query that does not block), and the host-buffer forms for their own exports before they return (a wait for
 *     their own stream).  The peers insert them at their next drain, by the policy of every drained row.  Rows are
 *     exported under the conditions under which the insert runs: a failing call and a launch without misses
 *     export nothing.  A cached launch never waits for another slot.  Bounded: a launch offers at most
 *     journal_rows rows and a slot has at most 4 exports pending; what is beyond either counts as
 *     shared_skipped and is simply not shared.  Pinned memory per slot: at most 4 * (33 * journal_rows rounded
 *     up to 4096) bytes, allocated as exports need it (shared_pinned_bytes).
 * sv_verdict_cache_sync(B) with the bit set first waits for the exports pending on any slot at the time of the
 * call and passes them on, then drains B: a cached launch on slot A whose stream work has completed (a
 * host-buffer form: that has returned) is in B's table when it returns, within B's journal bound and the claim
 * policy.  Unknown bits: SV_ERR_INVALID_ARG.  With the cache off the setting is remembered and nothing else
 * happens.  The setter drops pending shared rows (the exports on their way, and what the journals hold); so do
 * sv_set_verdict_cache, sv_verdict_cache_clear, sv_set_verdict_cache_feed, sv_set_device_map and sv_shutdown. */
#define SV_VC_SHARE_FEED 1u   /* a journaled keyed lane batch goes to every slot's journal, not only its own */
#define SV_VC_SHARE_STORES 2u /* what a cached launch verified is handed to the other slots' journals */
int sv_set_verdict_cache_share(uint32_t what);
/* sv_ed25519_verify_device behind the slot's verdict cache: the same inputs
 * (d_pk, d_sig 16-byte aligned), the same d_verdict bytes and d_bitmap.
 * d_hit (optional, n bytes): 1 where the verdict came from the table, all 0
 * with the cache off.  d_keys (optional, n x 32, 16-byte aligned): the cache
 * keys.  Stream semantics as sv_ed25519_verify_txbodies_hinted_device: with the
 * cache on the call WAITS once on `stream`, for the miss count.  Always the bulk
 * route, at any n (the latency lane is not cached). */
int sv_ed25519_verify_device_cached(int device, const void* d_pk, const void* d_sig, const void* d_msg,
                                    const uint64_t* d_msg_off, const uint32_t* d_msg_len,
                                    uint32_t fixed_msg_len, size_t n, void* d_verdict, void* d_bitmap,
                                    void* d_hit /* optional, n bytes */, void* d_keys /* optional, n x 32 */,
                                    void* stream);

/* The verdict audit (csrc/audit.h, csrc/sv_audit.hip).  Behind
 * a verify launch of the bulk route, a deterministic sample of its rows is
 * verified again on the same stream by the textbook equation -- libsodium's
 * steps (1)-(8) with the full-length [h](-A) + [S]B ladder of
 * csrc/verify_core.h sv_verify_core: no half-size equation, no per-key table,
 * no verdict cache -- and compared with the verdict bytes the caller will see.
 * Rows whose verdict came from the verdict cache are sampled like any other.
 *
 *   OFF BY DEFAULT (what == 0, or the SV_AUDIT / SV_AUDIT_ONE_IN / SV_AUDIT_SEED
 *   environment variables, read at first use): then no call allocates,
 *   launches, waits for or returns anything more than before.
 *   The pick: row i of the slot's audited launch number seq is audited iff
 *     (what & SV_AUDIT_REJECTS) and verdict[i] == 0, or
 *     (what & SV_AUDIT_SAMPLE) and mix(seed, seq, i) % one_in == 0
 *   (mix: the 64-bit mixer written out in csrc/audit.h; one_in == 1: every
 *   row).  The picks are taken in ascending row order, only the first `budget`
 *   of a launch are audited (0: 65,536; at most SV_AUDIT_BUDGET_MAX) and the
 *   rest count as over_budget.  Nothing waits on the host: the audit kernels
 *   are queued behind the verify kernels and add to device counters.
 *   A disagreement never changes a verdict byte.  It is counted (mismatches)
 *   and recorded in the slot's ring of SV_AUDIT_RING records, oldest first;
 *   what does not fit counts as records_lost.
 *   Audited: every caller-visible verdict array of the bulk route -- raw
 *   batches, the tx-body, hinted, check, decide, accounts and ledger forms,
 *   the device-resident forms, cached launches with their hits.  NOT audited:
 *   the latency lane (batches of at most 12,288 signatures on the automatic
 *   path); its launches count in lane_launches.  Check decisions and tx
 *   results are not audited, only verify verdicts.
 *
 * sv_set_audit is process-wide; what == 0 turns the audit off and frees its
 * buffers (counters and ring included).  SV_ERR_INVALID_ARG: unknown bits,
 * SV_AUDIT_SAMPLE with one_in == 0, a budget above SV_AUDIT_BUDGET_MAX.
 * SV_AUDIT_STRICT: a host-buffer form on the bulk route -- the raw batches and
 * every tx-body, hinted, check, decide, accounts and ledger form -- returns
 * SV_ERR_AUDIT if its slot's `mismatches` moved during the call, or during any
 * slice of a sharded call (one more 8-byte read-back per slice, after the
 * slice's last wait, and only in strict mode).  The verdicts already copied
 * out are unspecified then, as on any engine error, and the caller re-runs the
 * batch on the CPU path.  Device-resident forms never wait and never return
 * SV_ERR_AUDIT: their mismatches show in the stats, and the slot's next strict
 * host-buffer slice answers for them (the count is compared with its value
 * at the last strict read-back, or at the sv_set_audit that set the bit).
 * sv_audit_get_stats / sv_audit_read wait for the slot's kernel stream.
 * sv_audit_read hands out the ring's records oldest first, at most cap of
 * them, and consumes what it hands out.  Before a record leaves, the engine
 * runs sv_verify_core on the HOST (radix-2^51 field) over the record's bytes
 * and stores the result in cpu_verdict: the arbitration between engine and
 * audit.  A message longer than SV_AUDIT_MSG_MAX is recorded truncated
 * (SV_AUDIT_REC_TRUNCATED) and gets cpu_verdict 0xFF.
 * sv_audit_device: audits n claimed verdict bytes from anywhere against the
 * textbook kernel, into the slot's counters and ring; stream semantics and
 * alignment rules of sv_ed25519_verify_device (d_pk, d_sig 16-byte aligned);
 * no wait.  It works with the process-wide audit off (o->what says what to
 * pick; o->seq names the launch).
 * sv_audit_batch_cpu: the CPU twin -- the same pick, budget and record rules,
 * sv_verify_core on the host; stats / rec are the caller's (rec holds at most
 * min(cap, SV_AUDIT_RING) records, the rest counts as records_lost; every
 * record's cpu_verdict equals its audit_verdict, for a truncated record too:
 * the twin has the whole message).  Fully determined by its arguments.
 * The verify kernel holds 256 VGPRs at two waves per SIMD; its fixed-32 form
 * uses no scratch, the any-length form spills 36 bytes per lane
 * (profiles/r18/audit/kernel_resources.csv). */
#define SV_AUDIT_REJECTS 1u
#define SV_AUDIT_SAMPLE 2u
#define SV_AUDIT_STRICT 4u
#define SV_ERR_AUDIT (-9)
#define SV_AUDIT_BUDGET_MAX ((size_t)1 << 22)
#define SV_AUDIT_MSG_MAX 512
#define SV_AUDIT_RING 64
#define SV_AUDIT_REC_TRUNCATED 1u
int sv_set_audit(uint32_t what, uint32_t one_in, uint64_t seed, size_t budget);
typedef struct sv_audit_stats {
  uint64_t struct_size;     /* in: sizeof(sv_audit_stats) of the caller; fields past it are not written */
  uint64_t what;            /* the setting in force (0: off) */
  uint64_t seq;             /* audited launches of the slot so far: the seq of the next one */
  uint64_t audited;         /* rows verified again */
  uint64_t audited_rejects; /* ... whose engine verdict was a reject */
  uint64_t over_budget;     /* picked rows past the launch's budget: not audited */
  uint64_t mismatches;      /* audited rows where engine and audit disagree */
  uint64_t records_lost;    /* mismatches the full ring could not take */
  uint64_t records_held;    /* records waiting in the ring */
  uint64_t lane_launches;   /* latency-lane launches while the audit was on: not audited */
  uint64_t bytes;           /* device memory the slot's audit holds now */
  double kernel_ms;         /* time of the audit's kernels (only while sv_timing_enable is on) */
} sv_audit_stats;
typedef struct sv_audit_record {
  uint64_t seq; /* the audited launch */
  uint64_t row; /* row of that launch's verdict array */
  uint32_t msg_len;
  uint8_t engine_verdict, audit_verdict, cpu_verdict /* 0xFF: not arbitrated */, flags /* SV_AUDIT_REC_* */;
  uint8_t pk[32];
  uint8_t sig[64];
  uint8_t msg[SV_AUDIT_MSG_MAX]; /* the first min(msg_len, SV_AUDIT_MSG_MAX) bytes, then zeros */
} sv_audit_record;
typedef struct sv_audit_opts {
  uint64_t struct_size; /* sizeof(sv_audit_opts) */
  uint32_t what;        /* SV_AUDIT_REJECTS | SV_AUDIT_SAMPLE */
  uint32_t one_in;
  uint64_t seed;
  uint64_t seq;
  uint64_t budget; /* 0: 65,536 */
} sv_audit_opts;
int sv_audit_get_stats(int device, sv_audit_stats* out);
int sv_audit_read(int device, sv_audit_record* out, size_t cap, size_t* n);
int sv_audit_device(int device, const sv_audit_opts* o, const void* d_pk, const void* d_sig, const void* d_msg,
                    const uint64_t* d_msg_off, const uint32_t* d_msg_len, uint32_t fixed_msg_len, size_t n,
                    const void* d_claimed /* n verdict bytes */, void* stream);
int sv_audit_batch_cpu(const sv_audit_opts* o, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                       const uint64_t* msg_off, const uint32_t* msg_len, uint32_t fixed_msg_len, size_t n,
                       const uint8_t* claimed, sv_audit_stats* stats, sv_audit_record* rec, size_t cap,
                       size_t* n_rec, int threads);

/* Host-side stages of the calling thread's last latency-lane batch (a batch of
 * at most one staging chunk on one slot), in microseconds: out[0] plan + pack,
 * [1] the H2D call (0 while the kernels read the image in place), [2] the kernel launch, [3] the D2H / event record calls,
 * [4] key-table build queueing, [5] the wait for the device (H2D + kernel +
 * verdicts), [6] the whole batch inside the engine, [7] 1 if it ran the
 * warm-key comb kernel, 0 the octet kernel.  Zeros before the first batch.
 * For tail-latency diagnosis (bench.py latency_1k.slow_iterations). */
int sv_lat_last_trace(double out[8]);

/* Per-key tables of the throughput path (replaces, for repeated signers, the
 * per-signature decode of A that libsodium's verify does,
 * /root/reference/src/crypto/SecretKey.cpp:461-463 per call; catchup replays
 * ~16 signatures per account, LedgerManagerImpl.cpp:1546-1609): each key's
 * decoded -A and its 9-entry table are built once on the device and reused
 * by every later signature of that key.  mode 0: off; 1: every throughput-
 * path launch; 2 (default): host-buffer batches whose keys repeat (a sampled
 * estimate; device-resident batches only with 1); -1: the SV_KEY_TABLES
 * environment variable.  slots: table size (0: SV_KEY_TABLE_SLOTS or 2^19,
 * ~1.5 KB of HBM each; claims stop at half, then the tables are cleared).
 * Verdicts never depend on the tables.  Returns the previous mode. */
int sv_set_key_tables(int mode, size_t slots);

/* Test knobs (0 in production).  TRIVIAL_PAIR: every lane verifies through the
 * fallback pair (h, 1) of the half-size equation (lattice.h), i.e. the
 * full-length scalar; MAX_WINDOWS: every wave runs all 64 windows (both only
 * select code paths; verdicts are unchanged).  FAIL: every GPU entry point
 * returns SV_ERR_HIP without touching the device (callers' CPU fallback
 * tests); PREP_ONLY (profiling): throughput-path launches run the
 * per-signature prep kernel only (verdicts are NOT written).  FAIL and
 * PREP_ONLY are refused (SV_ERR_INVALID_ARG) unless the process environment
 * has SV_TEST_KNOBS=1.  Returns the previous flags, or SV_ERR_INVALID_ARG. */
#define SV_DBG_TRIVIAL_PAIR 0x1u
#define SV_DBG_MAX_WINDOWS 0x2u
#define SV_DBG_FAIL 0x4u
#define SV_DBG_PREP_ONLY 0x8u
#define SV_DBG_KEY_COLLIDE 0x10u /* every key gets the same per-key-table fingerprint (collision path) */
/* throughput-path geometry: QUAD runs every throughput-path launch one signature
 * per quad of lanes (the medium-batch kernel), NO_QUAD none (one per lane);
 * by default launches of at most SV_QUAD_MAX signatures (env; default in
 * DESIGN.md) that use no per-key tables take the quad geometry.  Code paths
 * only: verdicts are unchanged. */
#define SV_DBG_QUAD 0x20u
#define SV_DBG_NO_QUAD 0x40u
/* DROP_HANDOVER (needs SV_TEST_KNOBS=1): the three-wave cold-key octet kernel
 * never raises its tables' hand-over flag, so its verify wave's bounded wait
 * (~0.5 s) runs out: the kernel writes fail-closed rejects and raises its
 * failure word, and the call returns SV_ERR_KERNEL (the error path of a lost
 * hand-over). */
#define SV_DBG_DROP_HANDOVER 0x80u
/* AUDIT_DISSENT (needs SV_TEST_KNOBS=1): the audit kernel inverts its OWN
 * verdict byte for the first picked row of every audited launch.  The engine's
 * verdicts are untouched: it exists so that the strict path and the
 * arbitration of sv_audit_read can be tested end to end. */
#define SV_DBG_AUDIT_DISSENT 0x100u
int sv_set_debug_flags(uint32_t flags);

/* Host-feed probe (multi-GPU sizing).  Runs the host
 * side of sv_ed25519_verify_batch_fixed(device = -1, max_devices) over n
 * signatures -- the contiguous slices, each slot's own staging workers
 * (pinned to the GPU's NUMA node), the pack into the slot's two pinned
 * staging slots and, with upload != 0, the H2D copies -- and launches no
 * kernel: no verdicts.  What the G slots' host side can feed, against the
 * rate G GPUs verify at. */
typedef struct sv_feed_stats {
  uint32_t struct_size;      /* sizeof(sv_feed_stats) */
  uint32_t slots;            /* slots the batch was sliced over */
  uint32_t threads_per_slot; /* pack threads per slot (1 slot: the shared pool + caller) */
  uint32_t usable_cpus;      /* affinity limited by the cgroup CPU quota */
  double seconds;            /* wall time of the whole feed */
  int32_t gpu_numa[16];      /* NUMA node of slot g's GPU (-1: unknown) */
  int32_t staging_numa[16];  /* NUMA node of slot g's first pinned staging page (-1: unknown) */
  uint32_t pinned_cpus[16];  /* CPUs slot g's workers are pinned to (0: not pinned) */
} sv_feed_stats;
int sv_host_feed_probe(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, uint32_t msg_len, size_t n,
                       uint32_t max_devices, int upload, sv_feed_stats* out);

/* Bytes of the slot's kernel workspace / pinned staging currently allocated. */
int sv_workspace_bytes(int device, size_t* bytes);
int sv_pinned_bytes(int device, size_t* bytes);

/* Kernel-time accounting for profiling: when enabled, every verify launch is
 * bracketed by HIP events on the device's internal stream and the elapsed
 * times are accumulated (read back with sv_kernel_time). */
int sv_timing_enable(int enable);
int sv_kernel_time(int device, double* total_ms, uint64_t* launches, uint64_t* signatures);
int sv_kernel_time_reset(void);
int sv_device_synchronize(int device);

#ifdef __cplusplus
}
#endif
#endif /* STELLAR_SIGVERIFY_H */
