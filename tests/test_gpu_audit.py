"""The verdict audit on the GPU (stellar-core_amd/csrc/sv_audit.hip, bulk.h audit_locked): the device form against
its CPU twin, the hook behind every kind of bulk-route verify launch, the sampled pick against the pure-Python
model, off-is-off, and the strict path with the arbitration (through the audit kernel's dissent knob, which
inverts one AUDIT byte: no engine verdict is touched and no fault is provoked).  Exact equality throughout."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_model as am  # noqa: E402
import test_gpu_txpairs as tpairs  # noqa: E402
import test_gpu_txresults as tr  # noqa: E402
import txbodies_pool as tp  # noqa: E402
import txpairs_pool as pp  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K_QUAD_MAX = 32768
STAGE_CHUNK = 1 << 18
BIG = 1 << 22  # the largest budget


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def audit_off_afterwards(sv):
    yield
    sv.set_debug_flags(0)
    sv.set_audit(0)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class Up:
    """A batch in device memory; shift: the message bytes start that many bytes off a 16-byte boundary."""

    def __init__(self, dev, d, shift=0):
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.n = len(d["verdict"])
        self.pk, self.sig = up(d["pk"]), up(d["sig"])
        self._msg = up(np.concatenate([np.zeros(shift, np.uint8), d["msg"], np.zeros(16, np.uint8)]))
        self.msg = self._msg.data_ptr() + shift
        self.off, self.len = up(d["msg_off"].astype(np.uint64)), up(d["msg_len"].astype(np.uint32))
        self.dev = dev

    def var(self):
        return dict(fixed_msg_len=0, d_msg_off=self.off.data_ptr(), d_msg_len=self.len.data_ptr())


def _device_audit(sv, dev, d, claimed, what, fixed=0, shift=0, **kw):
    """sv_audit_device in a fresh audit state -> (stats, records)"""
    sv.set_audit(0)  # (frees the slot's counters and ring)
    u = Up(dev, d, shift)
    tc = torch.from_numpy(np.ascontiguousarray(claimed)).to(dev)
    mode = dict(fixed_msg_len=fixed) if fixed else u.var()
    sv.audit_device(0, u.pk.data_ptr(), u.sig.data_ptr(), u.msg, u.n, tc.data_ptr(), what, stream=_stream(dev),
                    **mode, **kw)
    st = sv.audit_stats(0)
    assert st["records_held"] == min(st["mismatches"], sv.AUDIT_RING)
    recs = sv.audit_read(0)
    assert sv.audit_stats(0)["records_held"] == 0 and sv.audit_read(0) == []  # consumed
    return st, recs


COUNTERS = ("audited", "audited_rejects", "over_budget", "mismatches", "records_lost", "records_held")


def _same_as_cpu(sv, dev, d, claimed, what, fixed=0, shift=0, **kw):
    st, recs = _device_audit(sv, dev, d, claimed, what, fixed, shift, **kw)
    cst, crecs = sv.audit_batch_cpu(d["pk"], d["sig"], d["msg"], None if fixed else d["msg_off"],
                                    None if fixed else d["msg_len"], claimed, what, fixed_msg_len=fixed, **kw)
    assert {k: st[k] for k in COUNTERS} == {k: cst[k] for k in COUNTERS}
    assert len(recs) == len(crecs)
    for r, c in zip(recs, crecs):
        if r["flags"] & sv.AUDIT_REC_TRUNCATED:
            # (the engine arbitrates over the record's bytes alone: a truncated message cannot be verified, the
            # record says so; the CPU twin has the whole message.  Everything else byte for byte.)
            assert r["cpu"] == 0xFF and c["cpu"] == c["audit"]
            raw = bytearray(r["raw"])
            raw[22] = c["cpu"]
            assert bytes(raw) == c["raw"]
        else:
            assert r["raw"] == c["raw"]
    return st, recs


@pytest.mark.parametrize("name", am.SETS)
def test_device_form_equals_cpu_twin_on_fixtures(sv, dev, golden, name):
    d = golden[name]
    n = len(d["verdict"])
    st, recs = _same_as_cpu(sv, dev, d, d["verdict"], am.SAMPLE, one_in=1, budget=BIG)
    assert (st["audited"], st["mismatches"]) == (n, 0) and recs == []
    rows = am.inverted_rows(name, d)
    claimed = d["verdict"].copy()
    claimed[rows] ^= 1
    # (message offsets off the 4-byte grid: the fixtures' own where they have them, and a shifted base)
    st, recs = _same_as_cpu(sv, dev, d, claimed, am.SAMPLE, shift=3, one_in=1, seq=5, budget=BIG)
    assert [r["row"] for r in recs] == rows
    for r in recs:
        want = int(d["verdict"][r["row"]])
        assert (r["engine"], r["audit"]) == (want ^ 1, want)
        assert r["cpu"] == (0xFF if r["msg_len"] > sv.AUDIT_MSG_MAX else want)
    if am.is_fixed32(d):  # the fixed 32-byte form, aligned (quad loads) and unaligned
        for shift in (0, 5):
            st, recs = _same_as_cpu(sv, dev, d, claimed, am.SAMPLE, fixed=32, shift=shift, one_in=1, budget=BIG)
            assert [r["row"] for r in recs] == rows


def test_unaligned_offsets_are_present(golden):
    assert (golden["intree"]["msg_off"] % 4 != 0).any() and (golden["msglen"]["msg_off"] % 4 != 0).any()


def test_device_form_pick_and_budget_equal_cpu_twin(sv, dev, golden):
    adv = golden["adversarial"]
    _same_as_cpu(sv, dev, adv, adv["verdict"], am.REJECTS, seq=3)
    _same_as_cpu(sv, dev, adv, adv["verdict"] ^ 1, am.REJECTS | am.SAMPLE, one_in=3, seed=11, seq=2)
    # n = 65,536 + 300: the second-level scan's per > 1 branch; every claim inverted, so mismatches == audited
    d = am.tiled(golden["valid"], 65536 + 300)
    want, _ = am.audited(am.SAMPLE, 64, 0x5EED, 7, d["verdict"])
    st, recs = _same_as_cpu(sv, dev, d, d["verdict"] ^ 1, am.SAMPLE, one_in=64, seed=0x5EED, seq=7)
    assert st["audited"] == st["mismatches"] == len(want) and [r["row"] for r in recs] == want[:sv.AUDIT_RING]
    assert st["records_lost"] == len(want) - sv.AUDIT_RING
    # the budget: 600 claimed rejects, 300 audited
    v = golden["valid"]
    b = {k: v[k][:600].copy() for k in ("pk", "sig", "msg_off", "msg_len", "verdict")}  # (the fixture stays as it is)
    b["msg"] = v["msg"]
    b["sig"][np.setdiff1d(np.arange(600), [3, 150, 299, 300, 599]), 40] ^= 1
    st, recs = _same_as_cpu(sv, dev, b, np.zeros(600, np.uint8), am.REJECTS, budget=300)
    assert (st["audited"], st["over_budget"]) == (300, 300) and [r["row"] for r in recs] == [3, 150, 299]


# ----------------------------------------------------------------- the hook
class Hooked:
    """Runs call() with the audit off and then on (every row), and checks the audit's account of it."""

    def __init__(self, sv):
        self.sv = sv

    def run(self, call, rows=None, same=None, times=1):
        sv = self.sv
        sv.set_audit(0)
        want = call()
        sv.set_audit(am.REJECTS | am.SAMPLE, one_in=1, seed=4, budget=BIG)
        for _ in range(times):
            before = sv.audit_stats(0)
            got = call()
            after = sv.audit_stats(0)
            n = rows(got) if callable(rows) else rows
            assert after["audited"] - before["audited"] == n, "every verdict row of the call is audited exactly once"
            assert after["mismatches"] == 0 and after["over_budget"] == 0 and after["records_held"] == 0
            assert after["seq"] > before["seq"] and after["lane_launches"] == before["lane_launches"]
            (same or _same_arrays)(got, want)
        return got


def _same_arrays(got, want):
    assert np.asarray(got).tobytes() == np.asarray(want).tobytes()


def _verify_device(sv, dev, u, fixed, cached=False):
    tv = torch.full((u.n,), 7, dtype=torch.uint8, device=dev)
    mode = dict(fixed_msg_len=32) if fixed else u.var()
    fn = sv.verify_device_cached if cached else sv.verify_device
    fn(0, u.pk.data_ptr(), u.sig.data_ptr(), u.msg, u.n, tv.data_ptr(), stream=_stream(dev), **mode)
    torch.cuda.synchronize(dev)
    return tv.cpu().numpy()


@pytest.fixture()
def throughput(sv):
    """The device-resident forms take the bulk route at any n."""
    prev = sv.set_kernel_path(sv.PATH_THROUGHPUT)
    yield
    sv.set_kernel_path(prev)


@pytest.mark.parametrize("n", [300, 40000])
def test_hook_verify_device_fixed32(sv, dev, golden, throughput, n):
    assert 300 <= K_QUAD_MAX < 40000
    d = am.tiled(golden["adversarial"], n)
    u = Up(dev, d)
    got = Hooked(sv).run(lambda: _verify_device(sv, dev, u, True), rows=n)
    assert (got == d["verdict"]).all()


def test_hook_verify_device_offsets(sv, dev, golden, throughput):
    d = golden["msglen"]
    u = Up(dev, d)
    got = Hooked(sv).run(lambda: _verify_device(sv, dev, u, False), rows=u.n)
    assert (got == d["verdict"]).all()


def test_hook_cached_launch_audits_its_hits(sv, dev, golden, throughput):
    d = am.tiled(golden["adversarial"], 300)
    u = Up(dev, d)
    try:
        sv.set_verdict_cache(1024)
        got = Hooked(sv).run(lambda: _verify_device(sv, dev, u, True, cached=True), rows=300, times=2)
        assert (got == d["verdict"]).all() and sv.verdict_cache_stats(0)["hits"] >= 250
    finally:
        sv.set_verdict_cache(0)


def test_hook_hinted_device_form(sv, dev, oracle, throughput):
    s = pp.make_pool(257, 557, tp.device_signer(sv))
    want = pp.expected(s, oracle)
    cap = len(want["pair_sig"]) + 3

    def same(got, ref):
        assert got[2] == ref[2]
        for x, y in zip(got[0], ref[0]):
            assert x.tobytes() == y.tobytes()

    got = Hooked(sv).run(lambda: tpairs._device_call(sv, dev, s, cap), rows=lambda g: g[2], same=same)
    assert got[2] == len(want["pair_sig"]) > 257
    pp.check(got[0], want)


def test_hook_decide_host_form(sv, dev):
    """A decide host call of a few hundred pairs.  Its verdict rows never leave the engine, so their number comes
    from the verdict cache's lookup counter for the same call (one lookup per pair)."""
    s, (code, fail) = tr._big(sv, 300, 20, 2, 1)
    call = lambda: tr._decide_host(sv, s, device=0, bad_cap=300, want_checks=True)  # noqa: E731
    try:
        sv.set_verdict_cache(1 << 12)
        call()
        pairs = sv.verdict_cache_stats(0)["lookups"]
    finally:
        sv.set_verdict_cache(0)
    assert pairs >= 300
    got = Hooked(sv).run(call, rows=pairs, same=tr._same)
    assert (got.body_code == code).all() and (got.body_fail == fail).all()


def test_hook_host_batch_with_a_short_second_chunk(sv, dev, golden):
    n = STAGE_CHUNK + 5
    d = am.tiled(golden["adversarial"], n)
    call = lambda: sv.verify_batch(d["pk"], d["sig"], d["msg"], d["msg_off"], d["msg_len"], device=0,  # noqa: E731
                                   path="throughput")
    got = Hooked(sv).run(call, rows=n)
    assert (got == d["verdict"]).all()


def test_latency_lane_is_counted_not_audited(sv, dev, golden):
    d = am.tiled(golden["valid"], 1024)
    sv.set_audit(am.REJECTS | am.SAMPLE, one_in=1)
    before = sv.audit_stats(0)
    out, keys = sv.verify_batch_keyed(d["pk"], d["sig"], d["msg"], d["msg_off"], d["msg_len"], device=0)
    after = sv.audit_stats(0)
    assert (out == d["verdict"]).all()
    assert after["lane_launches"] == before["lane_launches"] + 1
    assert (after["audited"], after["seq"]) == (before["audited"], before["seq"])


def test_sampled_hook_matches_the_pick_model(sv, dev, golden, throughput):
    d = am.tiled(golden["adversarial"], 4096)
    u = Up(dev, d)
    sv.set_audit(am.SAMPLE, one_in=8, seed=0xABCDEF)
    for _ in range(2):  # (two launches: the pick moves with seq)
        before = sv.audit_stats(0)
        got = _verify_device(sv, dev, u, True)
        after = sv.audit_stats(0)
        want, _ = am.audited(am.SAMPLE, 8, 0xABCDEF, before["seq"], d["verdict"])
        assert after["seq"] == before["seq"] + 1 and 400 < len(want) < 640
        assert after["audited"] - before["audited"] == len(want)
        assert after["audited_rejects"] - before["audited_rejects"] == int((d["verdict"][want] == 0).sum())
        assert after["mismatches"] == 0 and (got == d["verdict"]).all()


def test_off_is_off(sv, dev, golden, throughput):
    d = am.tiled(golden["adversarial"], 40000)

    def fresh_call():
        sv.set_device_map([])  # every slot released and created again
        u = Up(dev, d)
        out = _verify_device(sv, dev, u, True)
        assert (out == d["verdict"]).all()
        return sv.workspace_bytes(0)

    sv.set_audit(0)
    ws_never = fresh_call()
    st = sv.audit_stats(0)
    assert all(st[k] == 0 for k in COUNTERS + ("seq", "bytes", "what", "lane_launches"))
    assert sv.audit_read(0) == []
    sv.set_audit(am.REJECTS | am.SAMPLE, one_in=1, budget=BIG)
    ws_on = fresh_call()
    st = sv.audit_stats(0)
    assert st["audited"] == 40000 and st["bytes"] > 0 and ws_on >= ws_never + st["bytes"]
    sv.set_audit(0)
    assert sv.audit_stats(0)["bytes"] == 0
    assert fresh_call() == ws_never


# ----------------------------------------------------------------- strict mode and the arbitration
def _mirror(sv):
    lib = ctypes.CDLL(sv.HOSTLIB_PATH)
    lib.svh_audit_mismatches.restype = ctypes.c_uint64
    lib.svh_audit_mismatches.argtypes = [ctypes.c_int]
    return lib


def test_strict_mode_and_arbitration(sv, dev, golden, throughput):
    d = am.tiled(golden["adversarial"], 20000)
    call = lambda: sv.verify_batch(d["pk"], d["sig"], d["msg"], d["msg_off"], d["msg_len"], device=0,  # noqa: E731
                                   path="throughput")
    sv.set_audit(am.REJECTS | am.SAMPLE, one_in=16, seed=3)
    sv.set_debug_flags(sv.DBG_AUDIT_DISSENT)
    seq = sv.audit_stats(0)["seq"]
    first = am.audited(am.REJECTS | am.SAMPLE, 16, 3, seq, d["verdict"])[0][0]
    # not strict: SV_OK, correct verdicts, one mismatch
    out = call()
    assert (out == d["verdict"]).all()
    st = sv.audit_stats(0)
    assert st["mismatches"] == 1 and st["records_held"] == 1
    (r,) = sv.audit_read(0)
    want = int(d["verdict"][first])
    assert (r["seq"], r["row"], r["engine"], r["audit"], r["cpu"]) == (seq, first, want, want ^ 1, want)
    assert r["pk"] == d["pk"][first].tobytes() and r["sig"] == d["sig"][first].tobytes()
    # strict: the call errs, the record says the engine was right
    sv.set_audit(am.REJECTS | am.SAMPLE | am.STRICT, one_in=16, seed=3)
    with pytest.raises(sv.SigVerifyError) as e:
        call()
    assert e.value.code == sv.SV_ERR_AUDIT
    (r,) = sv.audit_read(0)
    assert r["engine"] == r["cpu"] != r["audit"]
    # the mirror: the CPU re-run answers, and what it caches is true
    host = _mirror(sv)
    host.svh_cache_clear()
    host.svh_set_cpu_threshold(ctypes.c_size_t(1))
    host.svh_engine_counts_ex(None)
    rows = np.arange(0, 20000, 1)
    for k in range(2):  # (the second pass is served from the mirror's cache: nothing false went in)
        out = np.zeros(len(rows), np.uint8)
        vp = ctypes.c_void_p
        off, ln = d["msg_off"].astype(np.uint64), d["msg_len"].astype(np.uint32)
        assert host.svh_verify_sig_batch(vp(d["pk"].ctypes.data), vp(d["sig"].ctypes.data), None,
                                         vp(d["msg"].ctypes.data), vp(off.ctypes.data), vp(ln.ctypes.data),
                                         ctypes.c_size_t(len(rows)), vp(out.ctypes.data)) == 0
        assert (out == d["verdict"]).all()
        counts = (ctypes.c_uint64 * 4)()
        host.svh_engine_counts_ex(ctypes.cast(counts, ctypes.c_void_p))
        # pass 1: the engine's batch came back as SV_ERR_AUDIT and was re-run on the CPU path.  Pass 2 is served
        # from the mirror's cache, and whatever that no longer holds takes the same route: no signature is ever
        # counted as verified by an engine call that failed.
        assert counts[0] == 0 and counts[1] == 0
        if k == 0:
            assert counts[3] == 1 and counts[2] > 0
    assert host.svh_audit_mismatches(0) == sv.audit_stats(0)["mismatches"] >= 3
    host.svh_cache_clear()
    # without the knob a strict call is SV_OK again
    sv.set_debug_flags(0)
    assert (call() == d["verdict"]).all()
