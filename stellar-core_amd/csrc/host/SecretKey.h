// C++ host mirror of the signing half of stellar-core's SecretKey, re-targeted
// at the engine's batch signer (include/stellar_sigverify.h
// sv_ed25519_sign_batch*).
//
// Reference interface (same names and meaning):
//   static SecretKey SecretKey::fromSeed(ByteSlice const&)   SecretKey.h:91, SecretKey.cpp:300-312
//   PublicKey const& getPublicKey() const                     SecretKey.h:44
//   Signature sign(ByteSlice const&) const                    SecretKey.h:56, SecretKey.cpp:134-146
// New:
//   signBatch(keys, keyOf, msgs): many signatures in one engine call, the
//   bulk signing of src/simulation/TxGenerator.cpp.
//
// sign() runs on the engine's CPU path (a lone signature is cheaper there than
// a GPU round trip, as a lone verifySig miss is); signBatch goes through the
// GPU engine, and an engine error re-runs the batch on
// sv_ed25519_sign_batch_cpu: never an exception for an engine problem and
// never a wrong signature.  Signatures are byte-equal to libsodium's
// crypto_sign_detached.  The signer is not constant-time (see the C header):
// load generation, test networks and benchmarks; a validator's NODE_SEED
// signing stays in libsodium.
#pragma once

#include <vector>

#include "PubKeyUtils.h"

namespace stellar {

class SecretKey {
 public:
  // Throws std::invalid_argument unless the seed is 32 bytes (the reference throws std::runtime_error's kin there).
  static SecretKey fromSeed(ByteSlice const& seed);
  PublicKey const& getPublicKey() const { return mPublicKey; }
  uint256 const& getSeed() const { return mSeed; }
  Signature sign(ByteSlice const& bin) const;

  // out[i] = keys[keyOf[i]].sign(msgs[i]); keyOf empty: keys.size() == msgs.size() and key i signs message i.
  // Throws std::invalid_argument for a keyOf entry out of range or mismatched sizes.
  static std::vector<Signature> signBatch(std::vector<SecretKey> const& keys, std::vector<uint32_t> const& keyOf,
                                          std::vector<ByteSlice> const& msgs);
  // The same over contiguous arrays (message i = msg[off[i] .. off[i] + len[i])): sig n x 64, pk (optional) k x 32.
  static void signBatchRaw(const uint8_t* seed, size_t k, const uint32_t* keyOf, const uint8_t* msg,
                           const uint64_t* off, const uint32_t* len, size_t n, uint8_t* sig, uint8_t* pk);
  // engine errors that signBatch re-ran on the CPU path since the last flush
  static uint64_t flushEngineFallbacks();

 private:
  uint256 mSeed{};
  PublicKey mPublicKey;
};

}  // namespace stellar
