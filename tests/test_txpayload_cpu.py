"""The ED25519_SIGNED_PAYLOAD stage decided by the engine, on a host without a
GPU: the CPU form sv_ed25519_check_txbodies_cpu with the payload tables
(sv_txchecks_payload) against the Python replay of txpayload_pool.py and
by-hand expectations, the skip without the tables, the argument errors, a plain
sv_txchecks with garbage behind it, and the check planner and packer with the
payload section against a numpy restatement.  Every expectation is exact
equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envelope_bodies as eb
import txbodies_pool as tp
import txchecks_pool as cp
import txpayload_pool as pl
import txset_gen as tg

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def edge(sv, oracle):
    bld = pl.PBuilder(3)
    cases = pl.edge_cases(bld)
    s = bld.finish(tp.pysign_signer(oracle), oracle)
    return s, cases, cp.oracle_verify(oracle)


def _cpu(sv, s, protocol=21, tables=True, threads=0):
    return sv.check_txbodies_cpu(*pl.args(s, tables), sig_len=s["sig_len"], protocol_version=protocol, threads=threads,
                                 **(pl.tables(s) if tables else {}))


def test_edge_cases_by_hand(sv, edge):
    s, cases, _ = edge
    assert {"len_%d" % n for n in pl.PAYLOAD_LENGTHS} <= set(cases)
    ok, weight, used, dig = _cpu(sv, s)
    assert (dig == s["digests"]).all()
    for name, (c0, hand) in cases.items():
        got = [(int(ok[c0 + i]), int(weight[c0 + i]), int(used[c0 + i])) for i in range(len(hand))]
        assert got == hand, name


def test_edge_cases_match_the_replay(sv, edge):
    s, _, verify = edge
    for protocol in (21, 9):  # (no protocol gate on the stage: the reference has none)
        want = pl.expected(s, verify, protocol)
        assert want[0].any() and not want[0].all()
        for threads in (1, 4):
            cp.assert_equal(_cpu(sv, s, protocol, threads=threads), want, s)
    c = edge[1]["clamp"][0]
    got = _cpu(sv, s, 9)
    assert (int(got[0][c]), int(got[1][c]), int(got[2][c])) == (1, 300, 1)


def test_without_the_tables_type3_is_skipped(sv, edge, oracle):
    """The same batch with the tables absent: today's results (txchecks_pool's
    three-stage replay), and the two differ exactly where a payload signer matters."""
    s, cases, verify = edge
    for protocol in (21, 9):
        want = pl.expected(s, verify, protocol, tables=False)
        cp.assert_equal(_cpu(sv, s, protocol, tables=False), want, s)
    c = cases["len_32"][0]
    assert want[0][c] == 0 and pl.expected(s, verify)[0][c] == 1
    # a batch without type-3 signers and empty tables: nothing to match, the same results
    bld = cp.Builder(3)
    cp.edge_cases(bld)
    bld.bodies = [b for b in bld.bodies if not any(g[0] == cp.SP for _, gs in b.checks for g in gs)]
    s = bld.finish(tp.pysign_signer(oracle))
    want = cp.expected(s, verify)
    got = sv.check_txbodies_cpu(*cp.args(s), sig_len=s["sig_len"], pkey_begin=np.zeros(s["nb"] + 1, np.uint64))
    cp.assert_equal(got, want, s)


def test_random_pool_matches_the_replay(sv, oracle):
    verify = cp.oracle_verify(oracle)
    for seed in (41, 42):
        bld = pl.PBuilder(seed)
        pl.random_pool(bld, 120)
        s = bld.finish(tp.pysign_signer(oracle), oracle)
        want = pl.expected(s, verify)
        skip = pl.expected(s, verify, tables=False)
        assert s["nq"] > 50 and (want[0] != skip[0]).any() and (want[2] != skip[2]).any()
        cp.assert_equal(_cpu(sv, s), want, s)
        cp.assert_equal(_cpu(sv, s, tables=False), skip, s)
        cp.assert_equal(_cpu(sv, s, 9), pl.expected(s, verify, 9), s)


# ------------------------------------------------ raw C-ABI: errors and struct sizes
class TxChecks(ctypes.Structure):  # sv_txchecks
    _fields_ = [("struct_size", ctypes.c_uint32), ("protocol_version", ctypes.c_uint32)] + [
        (n, ctypes.c_void_p) for n in ("sig_len", "check_begin", "check_needed", "signer_begin", "signer_type",
                                       "signer_weight", "signer_key")] + [
        ("n_checks", ctypes.c_size_t), ("n_signers", ctypes.c_size_t)]


class TxChecksPayload(ctypes.Structure):  # sv_txchecks_payload
    _fields_ = [("checks", TxChecks)] + [(n, ctypes.c_void_p) for n in ("pkey_begin", "pkey", "pkey_payload",
                                                                        "pkey_len")] + [("n_pkeys", ctypes.c_size_t)]


def _raw(sv, s, over=None, struct_size=None, skip_keys=False, garbage=False):
    """sv_ed25519_check_txbodies_cpu through ctypes over a struct of the test's
    own; `over` replaces table pointers / counts.  -> (rc, ok, weight, used),
    the outputs pre-filled with 0xA5."""
    lib = sv.load_library()
    P = lambda a: a.ctypes.data  # noqa: E731
    keep = dict(s)
    keep["gk"] = s["signer_key_skip"] if skip_keys else s["signer_key"]
    ck = TxChecksPayload()
    c = ck.checks
    c.struct_size = ctypes.sizeof(TxChecksPayload) if struct_size is None else struct_size
    c.protocol_version = 21
    c.sig_len, c.check_begin, c.check_needed = P(s["sig_len"]), P(s["check_begin"]), P(s["check_needed"])
    c.signer_begin, c.signer_type, c.signer_weight = P(s["signer_begin"]), P(s["signer_type"]), P(s["signer_weight"])
    c.signer_key, c.n_checks, c.n_signers = P(keep["gk"]), s["nc"], s["ng"]
    ck.pkey_begin, ck.pkey, ck.pkey_payload, ck.pkey_len = (P(s[k]) for k in ("pkey_begin", "pkey", "pkey_payload",
                                                                              "pkey_len"))
    ck.n_pkeys = s["nq"]
    if garbage:
        ctypes.memset(ctypes.addressof(ck) + ctypes.sizeof(TxChecks), 0xEE, ctypes.sizeof(ck) - ctypes.sizeof(TxChecks))
    hold = []
    for k, v in (over or {}).items():
        if isinstance(v, np.ndarray):
            hold.append(v)
            v = P(v)
        setattr(c if hasattr(TxChecks, k) else ck, k, v)
    nc = s["nc"]
    ok, weight, used = np.full(nc, 0xA5, np.uint8), np.full(nc, 0xA5A5A5A5, np.uint32), np.full(nc, 0xA5, np.uint64)
    vp = ctypes.c_void_p
    fn = lib.sv_ed25519_check_txbodies_cpu
    fn.argtypes = [vp] * 5 + [ctypes.c_size_t, vp, vp, vp, ctypes.c_size_t, vp, vp, ctypes.c_size_t, vp, vp, vp, vp, vp,
                   ctypes.c_int]
    nid = np.frombuffer(tp.NETWORK_ID, np.uint8).copy()
    rc = fn(P(nid), P(s["bodies"]), P(s["off"]), P(s["len"]), P(s["kind"]), s["nb"], P(s["sig_begin"]), P(s["hint"]),
            P(s["sig"]), s["ns"], P(s["key_begin"]), P(s["key"]), s["nk"], ctypes.addressof(ck), P(ok), P(weight),
            P(used), None, 0)
    return rc, ok, weight, used


def test_validation_errors_leave_the_outputs_untouched(sv, edge):
    s, cases, verify = edge
    INVALID = -1  # SV_ERR_INVALID_ARG
    rc, ok, weight, used = _raw(sv, s)
    assert rc == 0
    cp.assert_equal((ok, weight, used), pl.expected(s, verify))
    qb = s["pkey_begin"]
    bad = {}
    a = qb.copy(); a[0] = 1; bad["pkey_begin[0] != 0"] = {"pkey_begin": a}  # noqa: E702
    a = qb.copy(); a[-1] += np.uint64(1); bad["pkey_begin[n] != n_pkeys"] = {"pkey_begin": a}  # noqa: E702
    a = qb.copy(); a[3], a[4] = a[4] + np.uint64(1), a[3]; bad["pkey_begin decreasing"] = {"pkey_begin": a}  # noqa: E702
    a = qb.copy(); a[2] = np.uint64(s["nq"] + 5); bad["pkey_begin past n_pkeys"] = {"pkey_begin": a}  # noqa: E702
    a = s["pkey_len"].copy(); a[5] = 65; bad["pkey_len > 64"] = {"pkey_len": a}  # noqa: E702
    for name in ("pkey", "pkey_payload", "pkey_len"):
        bad["null " + name] = {name: None}
    bad["n_pkeys >= 2^32"] = {"n_pkeys": 1 << 32}
    g = int(s["signer_begin"][cases["before_none"][0]])
    assert s["signer_type"][g] == 3
    for name, idx in (("the next body's candidate", int(s["signer_key"][g]) + 1),
                      ("the previous body's candidate", int(s["signer_key"][g]) - 1), ("past the table", s["nq"])):
        a = s["signer_key"].copy()
        a[g] = idx
        bad["type-3 index: " + name] = {"signer_key": a}
    for name, over in bad.items():
        rc, ok, weight, used = _raw(sv, s, over)
        assert rc == INVALID, name
        assert (ok == 0xA5).all() and (weight == 0xA5A5A5A5).all() and (used == 0xA5).all(), name
    # a null pkey_begin is "tables absent", not an error: the skip's key indices are then what is checked
    rc, ok, weight, used = _raw(sv, s, {"pkey_begin": None}, skip_keys=True)
    assert rc == 0
    cp.assert_equal((ok, weight, used), pl.expected(s, verify, tables=False))


def test_plain_struct_with_garbage_behind_it_is_accepted_and_skips(sv, edge):
    s, _, verify = edge
    want = pl.expected(s, verify, tables=False)
    rc, ok, weight, used = _raw(sv, s, struct_size=ctypes.sizeof(TxChecks), skip_keys=True, garbage=True)
    assert rc == 0
    cp.assert_equal((ok, weight, used), want)
    # one byte short of the extension is still the plain struct
    rc, ok, weight, used = _raw(sv, s, struct_size=ctypes.sizeof(TxChecksPayload) - 1, skip_keys=True, garbage=True)
    assert rc == 0
    cp.assert_equal((ok, weight, used), want)
    assert _raw(sv, s, struct_size=ctypes.sizeof(TxChecks) - 1, skip_keys=True)[0] == -1


def test_only_the_payload_signer_can_satisfy_it(sv, edge):
    """Through raw ctypes: the check is 1 with the tables and 0 for an engine that does not read them."""
    s, cases, _ = edge
    c = cases["len_47"][0]
    assert _raw(sv, s)[1][c] == 1
    assert _raw(sv, s, struct_size=ctypes.sizeof(TxChecks), skip_keys=True)[1][c] == 0


def test_binding_defaults_are_the_calls_without_tables(sv, edge):
    s, _, verify = edge
    with pytest.raises(ValueError):
        sv.check_txbodies_cpu(*pl.args(s), pkey=s["pkey"])
    with pytest.raises(ValueError):
        sv.check_txbodies_cpu(*pl.args(s), pkey_begin=s["pkey_begin"], pkey=s["pkey"][:-1],
                              pkey_payload=s["pkey_payload"], pkey_len=s["pkey_len"])
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_INVALID_ARG"):  # (type-3 indices past the key rows, no tables)
        sv.check_txbodies_cpu(*pl.args(s), sig_len=s["sig_len"])


# ------------------------------------------------ planner and packer against numpy
@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """tests/native/txpayload_core.cpp: the planner / packer with the payload section."""
    so = str(tmp_path_factory.mktemp("txpayload") / "libtxpayloadstage.so")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared",
           "-Wno-unknown-pragmas", "-o", so, os.path.join(HERE, "native", "txpayload_core.cpp"),
           "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    lib = ctypes.CDLL(so)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    lib.hs_payload_plan.argtypes = [vp] * 6 + [u64] * 7 + [vp, ctypes.c_int]
    lib.hs_payload_pack.argtypes = [vp] * 4 + [u64] + [vp] * 18
    return lib


def test_plan_and_pack_with_payload_tables(sv, stage):
    """Chunks cut by the key bound, which payload candidates count towards,
    reproduce the unchunked tables after rebasing; without the tables the plan
    and the image are the ones of before."""
    bld = pl.PBuilder(17)
    pl.random_pool(bld, 60, share=0.6)
    # (the layout needs no real signatures: a key per seed, constant signature bytes)
    s = bld.finish(lambda seeds, msgs: (np.ascontiguousarray(seeds[:, ::-1]), np.ones((len(seeds), 64), np.uint8)),
                   None, layout_only=True)
    P = lambda a: a.ctypes.data  # noqa: E731
    nb = s["nb"]
    sb, kb, cb, gb, qb = s["sig_begin"], s["key_begin"], s["check_begin"], s["signer_begin"], s["pkey_begin"]
    al16 = lambda v: (int(v) + 15) & ~15  # noqa: E731
    big = 1 << 18

    def plan_of(qb_arg, max_k):
        out = np.zeros(35 * 128, np.uint64)
        n = stage.hs_payload_plan(P(s["len"]), P(sb), P(kb), P(cb), P(gb), P(qb_arg) if qb_arg is not None else None,
                                  0, nb, big, max_k, 64 << 20, big, big, P(out), 128)
        assert 1 <= n <= 128
        return [[int(x) for x in out[35 * i:35 * i + 35]] for i in range(n)]

    assert len(plan_of(qb, big)) == 1
    cut_without, cut_with = plan_of(None, 12), plan_of(qb, 12)
    assert len(cut_with) > len(cut_without) > 1  # the candidates count towards the key bound
    for c in cut_without:
        assert c[28:34] == [0] * 6 and c[34] == c[27]  # no payload section: the image is the CheckChunk's
    seen_q, crossing = 0, 0
    for i, c in enumerate(cut_with):
        b0, b1, k0, k1 = c[0], c[1], c[4], c[5]
        c0, c1, g0, g1, o_gk, o_gt, bytes_ = c[16], c[17], c[18], c[19], c[24], c[25], c[27]
        q0, q1, o_qk, o_qp, o_qb, o_ql, total = c[28:35]
        k, nq = b1 - b0, q1 - q0
        assert (q0, q1) == (int(qb[b0]), int(qb[b1])) and q0 == seen_q
        seen_q = q1
        assert k == 1 or (k1 - k0) + nq <= 12
        if b1 < nb:
            assert int(kb[b1 + 1]) - k0 + int(qb[b1 + 1]) - q0 > 12
        if nq:
            assert (o_qk, o_qp, o_qb, o_ql, total) == (bytes_, bytes_ + 32 * nq, bytes_ + 96 * nq,
                                                       bytes_ + 96 * nq + 8 * (k + 1),
                                                       al16(bytes_ + 97 * nq + 8 * (k + 1)))
            crossing += i > 0
        else:
            assert total == bytes_
        h = np.full(total + 64, 0xCD, np.uint8)
        chunk = np.asarray(c[:28], np.uint64)
        stage.hs_payload_pack(P(s["bodies"]), P(s["off"]), P(s["len"]), P(s["kind"]), nb, P(sb), P(s["hint"]),
                              P(s["sig"]), P(kb), P(s["key"]), P(s["sig_len"]), P(cb), P(s["check_needed"]), P(gb),
                              P(s["signer_type"]), P(s["signer_weight"]), P(s["signer_key"]), P(qb), P(s["pkey"]),
                              P(s["pkey_payload"]), P(s["pkey_len"]), P(chunk), P(h))
        assert (h[total:] == 0xCD).all()  # nothing past the plan
        # rebasing: the chunk's tables plus its bases are the unchunked ones
        gt = s["signer_type"][g0:g1]
        base = np.where(gt == 3, np.uint32(q0), np.uint32(k0))
        assert np.array_equal(h[o_gk:o_gt].view(np.uint32) + base, s["signer_key"][g0:g1])
        if nq:
            assert np.array_equal(h[o_qk:o_qp], s["pkey"][q0:q1].ravel())
            assert np.array_equal(h[o_qp:o_qb], s["pkey_payload"][q0:q1].ravel())
            assert np.array_equal(h[o_qb:o_ql].view(np.uint64) + np.uint64(q0), qb[b0:b1 + 1])
            assert np.array_equal(h[o_ql:o_ql + nq], s["pkey_len"][q0:q1])
    assert seen_q == s["nq"] and crossing >= 2  # the payload tables cross chunk boundaries



# ------------------------------------------------ host mirror (prefetch 6)
class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    st = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(st))
    return st


def _gpu(sv):
    try:
        return sv.device_count() > 0
    except sv.SigVerifyError:
        return False


def test_mirror_prefetch6_decides_payload_signers_in_the_engine(sv, oracle):
    """The envelope set with its signed-payload unit: prefetch 6 gives the
    results and hashes of prefetch 0 in ONE engine call (without a GPU: one
    fallback to the CPU form), where prefetch 5 finishes the payload account's
    checks with single verifications on the host."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(3, 29, tp.pysign_signer(oracle), with_payload=True)
    npay = s["kinds"].count("payload")
    assert npay == 3

    def call(prefetch, for_apply=0):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch, for_apply=for_apply)

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all(), ref["code"]
    verify = cp.oracle_verify(oracle)
    for for_apply in (0, 1):
        want = [tg.replay_envelope(c, 21, for_apply, verify) for c in pl.envelope_cases(s)]
        got = call(6, for_apply)[0]
        for k in ("code", "inner_code", "failed_op", "op_code"):
            assert got[k].tolist() == [w[k] for w in want], k
    sigs_sent = int(s["envs_blank"]["nsigs"].sum() + s["envs_blank"]["nouter"].sum())
    def counted(prefetch):
        """-> results, checks, hashes, engine stats and verifySig lookups of one call on a cold cache."""
        host.svh_cache_clear()
        hits, misses = ctypes.c_uint64(), ctypes.c_uint64()
        host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
        _stats(host)
        out = call(prefetch)
        host.svh_cache_counts(ctypes.byref(hits), ctypes.byref(misses))
        return out, _stats(host), hits.value + misses.value

    (res5, checks5, _, _), st5, lookups5 = counted(5)
    (res, checks, ch, fb), st, lookups = counted(6)
    assert (res == ref).all() and (res5 == ref).all() and checks == checks5
    assert (ch == ch0).all() and (fb == fb0).all()
    # the engine call's signatures and nothing else: no single verification for the payload signers, which
    # prefetch 5 looks up (and, the cache cold, verifies) one by one
    total = lambda x: x.gpu_signatures + x.cpu_signatures  # noqa: E731
    assert (total(st), lookups) == (sigs_sent, 0)
    assert lookups5 >= npay and total(st5) > sigs_sent
    assert (st.fallbacks == 0 and st.gpu_batches == 1) if _gpu(sv) else st.fallbacks == 1
    assert (call(6, for_apply=1)[0] == call(0, for_apply=1)[0]).all()
