// TEST INFRASTRUCTURE: a stand-alone program (its own main) over the CPU form of the verdict audit
// (csrc/sv_cpu.cpp sv_audit_batch_cpu, csrc/audit.h), built together with sv_cpu.cpp under
// -fsanitize=address,undefined and run by tests/test_audit_cpu.py.  Messages of 0..300 bytes at start offsets 0..3,
// signed here with csrc/sign_core.h, every one ending exactly where its heap block ends: the audit must accept each
// (claimed 1: no mismatch; claimed 0: one record that carries the message), and a read past a message aborts the
// run.  Then the ring's overflow path: 70 mismatches must leave 64 records, in row order, and 6 lost.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sign_core.h"

#include "../../include/stellar_sigverify.h"

static std::vector<sv_u4> comb_table() {
  // (running additions, as tests/native/sign_san.cpp builds it: short under the sanitizers)
  std::vector<sv_u4> ctab((size_t)SV_CB_DW / 4, sv_u4{0, 0, 0, 0});
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
  return ctab;
}

static int fail(const char* what, uint32_t len, uint32_t off) {
  std::printf("audit_san: %s (length %u, offset %u)\n", what, len, off);
  return 1;
}

int main() {
  const std::vector<sv_u4> ctab = comb_table();
  const uint32_t* tab = (const uint32_t*)ctab.data();
  sv_audit_opts o;
  o.struct_size = sizeof(o);
  o.what = SV_AUDIT_REJECTS | SV_AUDIT_SAMPLE;
  o.one_in = 1;
  o.seed = 1;
  o.seq = 2;
  o.budget = 0;
  int rows = 0;
  for (uint32_t len = 0; len <= 300; ++len) {
    uint32_t seed[8], rec[SV_SIGN_REC_DW];
    for (int i = 0; i < 8; ++i) seed[i] = 0x9e3779b9u * (len + 1) + 0x01010101u * (uint32_t)i;
    sv_sign_expand(rec, seed, tab);
    for (uint32_t off = 0; off < 4; ++off) {
      uint8_t* block = (uint8_t*)std::malloc(off + len ? off + len : 1);
      uint8_t* m = block + off;
      for (uint32_t j = 0; j < len; ++j) m[j] = (uint8_t)(len * 7u + j * 13u + 1u);
      uint32_t sig[16];
      sv_sign_msg(sig, rec, len ? m : nullptr, len, tab);
      // exact-size blocks for the key and the signature too
      uint8_t* pk = (uint8_t*)std::malloc(32);
      uint8_t* sg = (uint8_t*)std::malloc(64);
      std::memcpy(pk, rec + 16, 32);
      std::memcpy(sg, sig, 64);
      const uint64_t moff = off;
      for (uint8_t claimed = 0; claimed < 2; ++claimed) {
        sv_audit_stats st;
        st.struct_size = sizeof(st);
        sv_audit_record r;
        size_t nr = 9;
        // (the offset / length form from the block's base, and for the last offset the fixed-length form)
        const int rc = off == 3 && len
                           ? sv_audit_batch_cpu(&o, pk, sg, m, nullptr, nullptr, len, 1, &claimed, &st, &r, 1, &nr, 1)
                           : sv_audit_batch_cpu(&o, pk, sg, block, &moff, &len, 0, 1, &claimed, &st, &r, 1, &nr, 1);
        if (rc != SV_OK) return fail("the CPU form failed", len, off);
        if (st.audited != 1 || st.mismatches != (claimed ? 0u : 1u) || nr != st.mismatches)
          return fail("a valid signature is not audited as valid", len, off);
        if (!claimed) {
          if (r.engine_verdict != 0 || r.audit_verdict != 1 || r.cpu_verdict != 1 || r.msg_len != len || r.row != 0 ||
              r.seq != 2 || r.flags != 0 || std::memcmp(r.msg, m, len) != 0 || std::memcmp(r.sig, sg, 64) != 0)
            return fail("the record does not carry the row", len, off);
        }
      }
      std::free(pk);
      std::free(sg);
      std::free(block);
      ++rows;
    }
  }
  {
    // 70 valid rows claimed as rejects: 64 records in row order, 6 lost
    const uint32_t n = 70, len = 5;
    uint8_t* pk = (uint8_t*)std::malloc(32 * n);
    uint8_t* sg = (uint8_t*)std::malloc(64 * n);
    uint8_t* msg = (uint8_t*)std::malloc(len * n);
    uint8_t* claimed = (uint8_t*)std::calloc(n, 1);
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t seed[8], rec[SV_SIGN_REC_DW], sig[16];
      for (int k = 0; k < 8; ++k) seed[k] = 0x85ebca6bu * (i + 1) + (uint32_t)k;
      sv_sign_expand(rec, seed, tab);
      for (uint32_t j = 0; j < len; ++j) msg[len * i + j] = (uint8_t)(i + 3 * j);
      sv_sign_msg(sig, rec, msg + len * i, len, tab);
      std::memcpy(pk + 32 * i, rec + 16, 32);
      std::memcpy(sg + 64 * i, sig, 64);
    }
    sv_audit_record* rec = (sv_audit_record*)std::malloc(sizeof(sv_audit_record) * SV_AUDIT_RING);
    sv_audit_stats st;
    st.struct_size = sizeof(st);
    size_t nr = 0;
    o.what = SV_AUDIT_REJECTS;
    if (sv_audit_batch_cpu(&o, pk, sg, msg, nullptr, nullptr, len, n, claimed, &st, rec, SV_AUDIT_RING, &nr, 3) != SV_OK)
      return fail("the CPU form failed", len, 0);
    if (st.audited != n || st.mismatches != n || nr != SV_AUDIT_RING || st.records_held != SV_AUDIT_RING ||
        st.records_lost != n - SV_AUDIT_RING)
      return fail("70 mismatches must leave 64 records and 6 lost", len, 0);
    for (uint32_t i = 0; i < SV_AUDIT_RING; ++i)
      if (rec[i].row != i || rec[i].audit_verdict != 1 || std::memcmp(rec[i].msg, msg + len * i, len) != 0)
        return fail("the ring is not in row order", len, i);
    std::free(rec);
    std::free(claimed);
    std::free(msg);
    std::free(sg);
    std::free(pk);
  }
  std::printf("audit_san ok: %d rows\n", rows);
  return 0;
}
