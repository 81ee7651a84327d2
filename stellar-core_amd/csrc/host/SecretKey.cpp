// See SecretKey.h.
#include "SecretKey.h"

#include <atomic>
#include <chrono>
#include <exception>
#include <stdexcept>

#include "../../../include/stellar_host.h"
#include "../../../include/stellar_sigverify.h"

namespace stellar {

namespace {
std::atomic<uint64_t> gSignFallbacks{0};
}

SecretKey SecretKey::fromSeed(ByteSlice const& seed) {
  if (seed.size() != 32) throw std::invalid_argument("seed does not match byte size");
  SecretKey sk;
  std::memcpy(sk.mSeed.data(), seed.data(), 32);
  // the public key alone: k = 1, n = 0
  if (sv_ed25519_sign_batch_cpu(sk.mSeed.data(), 1, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr,
                                sk.mPublicKey.ed25519().data(), 1) != SV_OK)
    throw std::runtime_error("error generating secret key from seed");
  return sk;
}

Signature SecretKey::sign(ByteSlice const& bin) const {
  if (bin.size() > 0xffffffffu) throw std::invalid_argument("message longer than 2^32 - 1 bytes");
  Signature out(64);
  const uint64_t off = 0;
  const uint32_t len = (uint32_t)bin.size();
  if (sv_ed25519_sign_batch_cpu(mSeed.data(), 1, nullptr, bin.data(), &off, &len, 0, 1, out.data(), nullptr, 1) != SV_OK)
    throw std::runtime_error("error while signing");
  return out;
}

void SecretKey::signBatchRaw(const uint8_t* seed, size_t k, const uint32_t* keyOf, const uint8_t* msg,
                             const uint64_t* off, const uint32_t* len, size_t n, uint8_t* sig, uint8_t* pk) {
  int rc = sv_ed25519_sign_batch(seed, k, keyOf, msg, off, len, 0, n, sig, pk, nullptr);
  if (rc == SV_OK) return;
  if (rc != SV_ERR_INVALID_ARG) {
    // an engine error is never an exception and never a wrong signature: the CPU path signs the batch
    gSignFallbacks.fetch_add(1);
    rc = sv_ed25519_sign_batch_cpu(seed, k, keyOf, msg, off, len, 0, n, sig, pk, 0);
    if (rc == SV_OK) return;
  }
  throw std::invalid_argument("signBatch: malformed batch");
}

std::vector<Signature> SecretKey::signBatch(std::vector<SecretKey> const& keys, std::vector<uint32_t> const& keyOf,
                                            std::vector<ByteSlice> const& msgs) {
  const size_t k = keys.size(), n = msgs.size();
  if (keyOf.empty() ? k != n : keyOf.size() != n) throw std::invalid_argument("signBatch: keyOf / msgs size mismatch");
  std::vector<uint8_t> seed(32 * k), blob;
  for (size_t j = 0; j < k; ++j) std::memcpy(&seed[32 * j], keys[j].mSeed.data(), 32);
  std::vector<uint64_t> off(n);
  std::vector<uint32_t> len(n);
  size_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    if (msgs[i].size() > 0xffffffffu) throw std::invalid_argument("message longer than 2^32 - 1 bytes");
    off[i] = total;
    len[i] = (uint32_t)msgs[i].size();
    total += msgs[i].size();
  }
  blob.resize(total + 1);
  for (size_t i = 0; i < n; ++i)
    if (len[i]) std::memcpy(&blob[off[i]], msgs[i].data(), len[i]);
  std::vector<uint8_t> sig(64 * n + 1);
  signBatchRaw(seed.data(), k, keyOf.empty() ? nullptr : keyOf.data(), blob.data(), off.data(), len.data(), n,
               sig.data(), nullptr);
  std::vector<Signature> out(n);
  for (size_t i = 0; i < n; ++i) out[i].assign(&sig[64 * i], &sig[64 * i] + 64);
  // (the seeds' copy leaves nothing behind)
  volatile uint8_t* z = seed.data();
  for (size_t j = 0; j < seed.size(); ++j) z[j] = 0;
  return out;
}

uint64_t SecretKey::flushEngineFallbacks() { return gSignFallbacks.exchange(0); }

}  // namespace stellar

// C entry points (include/stellar_host.h).  They live here, not in host_capi.cpp, so that a build of the mirror
// without the signer links as before.  (svh_last_error_string is the verify side's: it is not set by these.)
using namespace stellar;

namespace {
int sign_exc(std::exception const&) { return SVH_ERR_INVALID_ARG; }
}  // namespace

extern "C" {

int svh_sign_batch(const uint8_t* seed, size_t k, const uint32_t* key_of, const uint8_t* msg, const uint64_t* msg_off,
                   const uint32_t* msg_len, size_t n, uint8_t* sig, uint8_t* pk) {
  try {
    SecretKey::signBatchRaw(seed, k, key_of, msg, msg_off, msg_len, n, sig, pk);
    return SVH_OK;
  } catch (std::exception const& e) {
    return sign_exc(e);
  }
}

int svh_sign(const uint8_t seed[32], const uint8_t* msg, size_t msg_len, uint8_t sig[64], uint8_t pk[32]) {
  try {
    const SecretKey sk = SecretKey::fromSeed(ByteSlice(seed, 32));
    const Signature s = sk.sign(ByteSlice(msg, msg_len));
    std::memcpy(sig, s.data(), 64);
    if (pk) std::memcpy(pk, sk.getPublicKey().ed25519().data(), 32);
    return SVH_OK;
  } catch (std::exception const& e) {
    return sign_exc(e);
  }
}

uint64_t svh_sign_fallbacks(void) { return SecretKey::flushEngineFallbacks(); }

int svh_bench_sign(size_t n_keys, size_t msg_len, int iterations, int batched, double* signs_per_s) {
  try {
    if (!signs_per_s || n_keys == 0 || iterations < 1) return SVH_ERR_INVALID_ARG;
    // the cases of benchmarkOpsPerSecond (SecretKey.cpp:193-212): one key and one msg_len-byte message each
    std::vector<SecretKey> keys;
    std::vector<std::vector<uint8_t>> msgs(n_keys, std::vector<uint8_t>(msg_len));
    for (size_t i = 0; i < n_keys; ++i) {
      uint8_t seed[32];
      for (int b = 0; b < 32; ++b) seed[b] = (uint8_t)(i * 131u + (size_t)b * 29u + (i >> 8));
      keys.push_back(SecretKey::fromSeed(ByteSlice(seed, 32)));
      for (size_t b = 0; b < msg_len; ++b) msgs[i][b] = (uint8_t)(i + b * 7u);
    }
    std::vector<ByteSlice> slices;
    for (auto const& m : msgs) slices.emplace_back(m.data(), m.size());
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    volatile uint8_t sink = 0;  // (keeps the signatures alive)
    for (int it = 0; it < iterations; ++it) {
      if (batched) {
        auto out = SecretKey::signBatch(keys, {}, slices);
        sink = sink ^ out.back()[0];
      } else {
        for (size_t i = 0; i < n_keys; ++i) sink = sink ^ keys[i].sign(slices[i])[0];
      }
    }
    const double dt = std::chrono::duration<double>(clk::now() - t0).count();
    *signs_per_s = (double)n_keys * (double)iterations / dt;
    return SVH_OK;
  } catch (std::exception const& e) {
    return sign_exc(e);
  }
}

}  // extern "C"
