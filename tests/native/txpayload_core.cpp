// TEST INFRASTRUCTURE: the check planner and packer of csrc/host_image.h with
// the payload tables, handed to Python as a small shared library
// (tests/test_txpayload_cpu.py builds it from this file): check_plan with the
// candidates' CSR array, and check_pack followed by payload_pack into one
// image.  Pure host code; no engine library is linked.
#include <cstring>
#include <vector>

#include "../../include/stellar_sigverify.h"
#include "../../stellar-core_amd/csrc/host_image.h"

static_assert(sizeof(sv::CheckChunk) == 28 * sizeof(uint64_t), "a CheckChunk is handed out as 28 words");
static_assert(sizeof(sv::PayloadChunk) == 7 * sizeof(uint64_t), "a PayloadChunk is handed out as 7 words");

namespace {
sv::CheckIn make_in(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, uint64_t nb,
                    const uint64_t* sb, const uint8_t* hint, const uint8_t* sig, const uint64_t* kb, const uint8_t* key,
                    const uint8_t* sig_len, const uint64_t* cb, const int32_t* need, const uint64_t* gb,
                    const uint8_t* gtype, const uint32_t* gweight, const uint32_t* gkey, const uint64_t* qb,
                    const uint8_t* qkey, const uint8_t* qpay, const uint8_t* qlen) {
  sv::CheckIn in{{nullptr, bodies, off, len, kind, (size_t)nb, sb, hint, sig, kb, key},
                 sig_len, cb, need, gb, gtype, gweight, gkey};
  in.qb = qb;
  in.qkey = qkey;
  in.qpay = qpay;
  in.qlen = qlen;
  return in;
}
}  // namespace

extern "C" {
// out: per chunk the 28 words of its CheckChunk, then the 7 of its PayloadChunk
// (q0, q1, o_qk, o_qp, o_qb, o_ql, bytes); qb may be null (no tables)
int hs_payload_plan(const uint32_t* len, const uint64_t* sb, const uint64_t* kb, const uint64_t* cb,
                    const uint64_t* gb, const uint64_t* qb, uint64_t B0, uint64_t B1, uint64_t max_s, uint64_t max_k,
                    uint64_t max_b, uint64_t max_c, uint64_t max_g, uint64_t* out, int cap) {
  const sv::CheckIn in = make_in(nullptr, nullptr, len, nullptr, 0, sb, nullptr, nullptr, kb, nullptr, nullptr, cb,
                                 nullptr, gb, nullptr, nullptr, nullptr, qb, nullptr, nullptr, nullptr);
  const std::vector<sv::CheckChunk> plan = sv::check_plan(in, B0, B1, max_s, max_k, max_b, max_c, max_g);
  for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) {
    const sv::PayloadChunk pc = sv::payload_chunk(in, plan[i]);
    memcpy(out + 35 * i, &plan[i], sizeof(sv::CheckChunk));
    memcpy(out + 35 * i + 28, &pc, sizeof(sv::PayloadChunk));
  }
  return (int)plan.size();
}

void hs_payload_pack(const uint8_t* bodies, const uint64_t* off, const uint32_t* len, const uint8_t* kind, uint64_t nb,
                     const uint64_t* sb, const uint8_t* hint, const uint8_t* sig, const uint64_t* kb, const uint8_t* key,
                     const uint8_t* sig_len, const uint64_t* cb, const int32_t* need, const uint64_t* gb,
                     const uint8_t* gtype, const uint32_t* gweight, const uint32_t* gkey, const uint64_t* qb,
                     const uint8_t* qkey, const uint8_t* qpay, const uint8_t* qlen, const uint64_t chunk[28],
                     uint8_t* dst) {
  const sv::CheckIn in = make_in(bodies, off, len, kind, nb, sb, hint, sig, kb, key, sig_len, cb, need, gb, gtype,
                                 gweight, gkey, qb, qkey, qpay, qlen);
  sv::CheckChunk c;
  memcpy(&c, chunk, sizeof(c));
  sv::check_pack(in, c, dst);
  sv::payload_pack(in, c, sv::payload_chunk(in, c), dst);
}
}  // extern "C"
