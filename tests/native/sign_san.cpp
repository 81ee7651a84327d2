// TEST INFRASTRUCTURE: a stand-alone program (its own main) over csrc/sign_core.h, built with
// -fsanitize=address,undefined and run by tests/test_sign_cpu.py.  Key expansion and signing for message lengths
// 0..300 at start offsets 0..3, every message ending exactly where its heap block ends, the table of B and the key
// record in heap blocks of their exact sizes: a read outside the message, the table or the record aborts the run.
// The four offsets of a length must give one signature, and RFC 8032's first test vector must come out.
// (The table is built by running addition, 8 doublings and 128 additions per position, so that the run stays
// short under the sanitizers; sv_comb_bentry, the product's builder, is pinned by tests/test_tables_cpu.py.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sign_core.h"

int main() {
  std::vector<sv_u4> ctab((size_t)SV_CB_DW / 4, sv_u4{0, 0, 0, 0});
  {
    const uint32_t benc[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                              0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    ge_p3 base;
    ge_frombytes(base, benc, false);
    ge_p1p1 Q;
    for (int pos = 0; pos < SV_CB_POS; ++pos) {
      ge_cached bc, ce;
      ge_p3_to_cached(bc, base);
      ge_p3 acc;
      fe_0(acc.X); fe_1(acc.Y); fe_1(acc.Z); fe_0(acc.T);
      for (int e = 0; e < SV_CB_ENT; ++e) {
        ge_p3_to_cached(ce, acc);
        sv_ce_put((uint32_t*)ctab.data() + ((size_t)pos * SV_CB_ENT + e) * SV_CE_DW, ce);
        ge_add_preswapped(Q, acc, bc.YpX, bc.YmX, bc.Z, bc.T2d, false, false);
        ge_p1p1_to_p3(acc, Q);
      }
      for (int k = 0; k < 8; ++k) {
        ge_dbl(Q, base.X, base.Y, base.Z);
        ge_p1p1_to_p3(base, Q);
      }
    }
  }
  const uint32_t* tab = (const uint32_t*)ctab.data();
  {
    // RFC 8032 section 7.1, TEST 1 (empty message)
    const uint8_t seed[32] = {0x9d, 0x61, 0xb1, 0x9d, 0xef, 0xfd, 0x5a, 0x60, 0xba, 0x84, 0x4a, 0xf4, 0x92, 0xec, 0x2c, 0xc4,
                              0x44, 0x49, 0xc5, 0x69, 0x7b, 0x32, 0x69, 0x19, 0x70, 0x3b, 0xac, 0x03, 0x1c, 0xae, 0x7f, 0x60};
    const uint8_t pk[32] = {0xd7, 0x5a, 0x98, 0x01, 0x82, 0xb1, 0x0a, 0xb7, 0xd5, 0x4b, 0xfe, 0xd3, 0xc9, 0x64, 0x07, 0x3a,
                            0x0e, 0xe1, 0x72, 0xf3, 0xda, 0xa6, 0x23, 0x25, 0xaf, 0x02, 0x1a, 0x68, 0xf7, 0x07, 0x51, 0x1a};
    const uint8_t sig[64] = {0xe5, 0x56, 0x43, 0x00, 0xc3, 0x60, 0xac, 0x72, 0x90, 0x86, 0xe2, 0xcc, 0x80, 0x6e, 0x82, 0x8a,
                             0x84, 0x87, 0x7f, 0x1e, 0xb8, 0xe5, 0xd9, 0x74, 0xd8, 0x73, 0xe0, 0x65, 0x22, 0x49, 0x01, 0x55,
                             0x5f, 0xb8, 0x82, 0x15, 0x90, 0xa3, 0x3b, 0xac, 0xc6, 0x1e, 0x39, 0x70, 0x1c, 0xf9, 0xb4, 0x6b,
                             0xd2, 0x5b, 0xf5, 0xf0, 0x59, 0x5b, 0xbe, 0x24, 0x65, 0x51, 0x41, 0x43, 0x8e, 0x7a, 0x10, 0x0b};
    uint32_t sd[8], rec[SV_SIGN_REC_DW], got[16];
    std::memcpy(sd, seed, 32);
    sv_sign_expand(rec, sd, tab);
    sv_sign_msg(got, rec, nullptr, 0, tab);
    if (std::memcmp(rec + 16, pk, 32) != 0 || std::memcmp(got, sig, 64) != 0) {
      std::printf("RFC 8032 TEST 1 does not come out\n");
      return 1;
    }
  }
  int signed_rows = 0;
  for (uint32_t len = 0; len <= 300; ++len) {
    uint32_t seed[8];
    for (int i = 0; i < 8; ++i) seed[i] = 0x9e3779b9u * (len + 1) + 0x01010101u * (uint32_t)i;
    uint32_t* rec = (uint32_t*)std::malloc(SV_SIGN_REC_DW * 4);
    sv_sign_expand(rec, seed, tab);
    uint32_t first[16];
    for (uint32_t off = 0; off < 4; ++off) {
      uint8_t* block = (uint8_t*)std::malloc(off + len ? off + len : 1);
      uint8_t* m = block + off;
      for (uint32_t j = 0; j < len; ++j) m[j] = (uint8_t)(len * 7u + j * 13u + 1u);
      uint32_t sig[16];
      sv_sign_msg(sig, rec, len ? m : nullptr, len, tab);
      if (off == 0) std::memcpy(first, sig, 64);
      else if (std::memcmp(first, sig, 64) != 0) {
        std::printf("length %u: offset %u signs differently from offset 0\n", len, off);
        return 1;
      }
      std::free(block);
      ++signed_rows;
    }
    std::free(rec);
  }
  std::printf("sign_san ok: %d signatures\n", signed_rows);
  return 0;
}
