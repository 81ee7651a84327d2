"""CPU checks over the isolating rows (tests/isolating_rows.py): rows whose
point equation holds while exactly one of libsodium's reject conditions fails,
for every blacklist encoding as A and as R.  A path that lost its small-order
term for A or R, or has one blacklist constant wrong, accepts one of them.

* the generator: its self-check, the counts per (encoding, role), the tries;
* the oracle gives 0 on every iso_* row and 1 on every control;
* the engine's CPU path (1 and 4 threads), the host models of the device
  arithmetic (tests/native/host_core.cpp: the lane verifier, its grouped form,
  the lattice verifier, the comb model) and the C++ mirror's verifySig /
  verifySigBatch on their CPU route give the oracle's verdicts; the mirror is
  asked twice, so its verify cache and key memo answer the second time;
* a census of the committed fixtures: which (encoding, role) pairs they isolate
  (few), so a fixture change cannot silently shift what these rows carry.
"""
import ctypes

import numpy as np
import pytest

import isolating_rows as ir
from conftest import load_golden, oracle_verdicts
from test_host_mirror import EngineStats

MLENS = (32, 33)
vp = ctypes.c_void_p


@pytest.fixture(scope="module", params=MLENS)
def rows(request):
    return ir.generate(request.param)


def _describe(d, bad):
    return [(int(i), str(d["class_names"][d["cls"][i]]), int(d["enc"][i])) for i in bad[:10]]


def _assert_verdicts(d, got, want, what):
    bad = np.nonzero(np.asarray(got) != want)[0]
    assert len(bad) == 0, (what, _describe(d, bad))


def test_generator_counts_and_self_check(rows):
    d = rows
    cls, enc = d["cls"], d["enc"]
    for role in (0, 1):
        for e in range(14):
            assert int(((cls == role) & (enc == e)).sum()) >= 3, (role, e)
    assert int((cls == 2).sum()) >= 3 and int((cls == 3).sum()) >= 3
    assert int((cls == 4).sum()) >= 8 and int((cls == 5).sum()) >= 4
    assert 1 <= int(d["tries"][cls < 2].max()) <= ir.MAX_TRIES
    assert (d["verdict"][cls < 4] == 0).all() and (d["verdict"][cls >= 4] == 1).all()
    # 6 of the 14 encodings are not the canonical encoding of their point
    assert sorted(set(enc[(cls == 1) & (d["canonical_R"] == 0)].tolist())) == [3, 9, 10, 11, 12, 13]
    assert (d["canonical_R"][cls != 1] == 1).all()
    # the S classes: S + L below 2^253 (the comb mask leaves it alone), S + kL at or above
    S = [int.from_bytes(d["sig"][i, 32:].tobytes(), "little") for i in range(len(cls))]
    assert all(ir.L <= S[i] < 1 << 253 for i in np.nonzero(cls == 2)[0])
    assert all(1 << 253 <= S[i] for i in np.nonzero(cls == 3)[0])
    assert {S[i] >> 253 for i in np.nonzero(cls == 3)[0]} >= {1, 7}  # bits 253..255: lowest and all set
    # holds() on every row again, outside the generator (its asserts vanish under python -O)
    for i in range(len(cls)):
        o, ln = int(d["msg_off"][i]), int(d["msg_len"][i])
        eq, failing = ir.holds(d["pk"][i], d["sig"][i], d["msg"][o:o + ln])
        assert eq, i
        assert bool(failing) == (cls[i] < 4), (i, failing)
        assert len(failing - {3}) == (1 if cls[i] < 4 else 0), (i, failing)


def test_holds_sees_a_broken_row(rows):
    """holds() is not vacuous: any change of S, R, A or the message breaks the equation."""
    d = rows
    i = int(np.nonzero(d["cls"] == 4)[0][0])
    o, ln = int(d["msg_off"][i]), int(d["msg_len"][i])
    pk, sig, msg = d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][o:o + ln].tobytes()
    assert ir.holds(pk, sig, msg) == (True, set())
    assert not ir.holds(pk, sig[:40] + bytes([sig[40] ^ 1]) + sig[41:], msg)[0]
    assert not ir.holds(pk, sig, msg[:-1] + bytes([msg[-1] ^ 1]))[0]
    j = int(np.nonzero(d["cls"] == 0)[0][0])
    assert not ir.holds(d["pk"][j], d["sig"][i], msg)[0]


def test_oracle_verdicts(rows, oracle):
    _assert_verdicts(rows, oracle_verdicts(oracle, rows), rows["verdict"], "oracle")


@pytest.mark.parametrize("threads", [1, 4])
def test_engine_cpu_path(rows, sv, oracle, threads):
    d = rows
    out = sv.verify_batch_cpu(d["pk"], d["sig"], d["msg"], d["msg_off"], d["msg_len"], threads=threads)
    _assert_verdicts(d, out, oracle_verdicts(oracle, d), "cpu path")


@pytest.mark.parametrize("model", ["hc_verify_batch", "hc_verify_batch_grouped", "hc_verify_batch_lat",
                                   "hc_comb_verify_batch"])
def test_host_models(rows, hostcore, oracle, model):
    d = rows
    n = len(d["verdict"])
    arrs = [np.ascontiguousarray(d[k]) for k in ("pk", "sig", "msg", "msg_off", "msg_len")]
    out = np.full(n, 7, np.uint8)
    args = [vp(a.ctypes.data) for a in arrs] + [ctypes.c_size_t(n), vp(out.ctypes.data)]
    if model == "hc_verify_batch_lat":
        wins = np.zeros(n, np.int32)
        args += [ctypes.c_int(0), vp(wins.ctypes.data)]
    getattr(hostcore, model)(*args)
    _assert_verdicts(d, out, oracle_verdicts(oracle, d), model)


def test_mirror_cpu_route_twice(rows, sv, oracle):
    """verifySig and verifySigBatch with every miss on the CPU path.  The second
    asking is answered by the verify cache (and the key memo): a cached reject
    stays a reject, a cached accept an accept."""
    d = rows
    n = len(d["verdict"])
    want = oracle_verdicts(oracle, d)
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_verify_sig.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                                    ctypes.c_size_t]
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_set_cpu_threshold.argtypes = [ctypes.c_size_t]
    host.svh_set_test_verifier.argtypes = [vp]
    host.svh_set_test_verifier(None)
    host.svh_set_cpu_threshold(1 << 20)
    stats = EngineStats()
    hits, misses = ctypes.c_uint64(), ctypes.c_uint64()
    try:
        host.svh_cache_clear()
        host.svh_cache_counts(None, None)
        host.svh_engine_counts_ex(ctypes.byref(stats))
        for asking in range(2):
            got = []
            for i in range(n):
                o, ln = int(d["msg_off"][i]), int(d["msg_len"][i])
                got.append(host.svh_verify_sig(d["pk"][i].tobytes(), d["sig"][i].tobytes(), 64,
                                               d["msg"][o:o + ln].tobytes(), ln))
            _assert_verdicts(d, got, want, "verifySig, asking %d" % asking)
            host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
            assert (hits.value, misses.value) == ((0, n) if asking == 0 else (n, 0))
        host.svh_cache_clear()
        host.svh_cache_counts(None, None)
        arrs = [np.ascontiguousarray(d[k]) for k in ("pk", "sig", "msg", "msg_off", "msg_len")]
        for asking in range(2):
            out = np.full(n, 7, np.uint8)
            rc = host.svh_verify_sig_batch(vp(arrs[0].ctypes.data), vp(arrs[1].ctypes.data), None,
                                           vp(arrs[2].ctypes.data), vp(arrs[3].ctypes.data), vp(arrs[4].ctypes.data),
                                           ctypes.c_size_t(n), vp(out.ctypes.data))
            assert rc == 0, host.svh_last_error_string()
            _assert_verdicts(d, out, want, "verifySigBatch, asking %d" % asking)
            host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
            assert (hits.value, misses.value) == ((0, n) if asking == 0 else (n, 0))
        host.svh_engine_counts_ex(ctypes.byref(stats))
        assert stats.gpu_signatures == 0 and stats.fallbacks == 0  # the CPU route, not a failed GPU call
    finally:
        host.svh_set_cpu_threshold(1)
        host.svh_cache_clear()
        host.svh_cache_counts(None, None)


def test_fixture_census_and_coverage():
    """What the committed fixtures isolate, recomputed with holds(): reject rows
    whose equation holds (R canonical, so libsodium's compare holds too) by the
    only condition that fails.  The fixtures isolate S >= L well, and a
    small-order A or R for two encodings only; every pair they leave open must
    be carried by the generated rows."""
    total = {"S": 0, "A": {}, "R": {}, "AR": 0, "noncanonical_R": 0}
    for name in ("adversarial", "intree", "lattice_edge"):
        c = ir.census(load_golden(name))
        for k in ("S", "AR", "noncanonical_R"):
            total[k] += c[k]
        for k in ("A", "R"):
            for e, cnt in c[k].items():
                total[k][e] = total[k].get(e, 0) + cnt
    # the table of the fixtures as committed; a change of the fixtures shows here
    assert total["S"] == 98
    assert total["A"] == {7: 1, 9: 1}  # entry 3 (an order-8 y) and entry 4 (y = p - 1), sign bit set
    assert total["R"] == {7: 1}
    assert total["AR"] == 18
    for mlen in MLENS:
        d = ir.generate(mlen)
        for role, key in ((0, "A"), (1, "R")):
            carried = set(d["enc"][d["cls"] == role].tolist())
            open_pairs = set(range(14)) - set(total[key])
            assert open_pairs <= carried, (key, sorted(open_pairs - carried))
            assert len(open_pairs) >= 12  # (the gap these rows exist for)
