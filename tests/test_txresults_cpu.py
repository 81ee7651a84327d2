"""One signature result per transaction body, on a host without a GPU: both CPU
forms (sv_ed25519_decide_txbodies_cpu, _accounts_cpu) against the numpy fold of
txresults_pool.py over what their check twins return, a constructed body for
every code by hand, the bad list against every capacity with guard words behind
it, every refusal of the host forms alone, csrc/txresult.h instantiated for
the host as a stand-alone program, and the mirror's prefetch 8 against
prefetch 0 with its walk counter.  Every expectation is exact equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envelope_bodies as eb
import envelopes as ev
import txaccounts_pool as ap
import txbodies_pool as tp
import txresults_pool as rp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def pool(sv, oracle):
    """The by-account edge cases, the constructed bodies and a random pool of
    300 bodies in one set, with random roles and flags on all but the
    constructed ones; shared and left unchanged."""
    bld = rp.RBuilder(5)
    ap.edge_cases(bld)
    n_edge = len(bld.bodies)
    ap.random_pool(bld, 300)
    rp.assign(bld, 99)
    cases = rp.code_cases(bld)
    s = bld.finish(tp.pysign_signer(oracle), oracle)
    assert s["nb"] >= 300 + n_edge and (s["check_role"] == rp.OP).any() and (s["body_flags"] == 1).any()
    return s, cases


def _twin_accounts(sv, s, protocol=21):
    return sv.check_txbodies_accounts_cpu(*ap.args(s), sig_len=s["sig_len"], protocol_version=protocol)


def _twin_explicit(sv, s, protocol=21):
    a, kw = ap.explicit_args(s)
    return sv.check_txbodies_cpu(*a, protocol_version=protocol, **kw)


def _decide_accounts(sv, s, protocol=21, **more):
    return sv.decide_txbodies_accounts_cpu(*rp.args(s), protocol_version=protocol, **rp.kwargs(s, **more))


def _decide_explicit(sv, s, protocol=21, **more):
    a, kw = rp.explicit(s)
    kw.update(more)
    return sv.decide_txbodies_cpu(*a, protocol_version=protocol, **kw)


@pytest.mark.parametrize("form", ["accounts", "explicit"])
def test_codes_are_the_fold_of_the_twin(sv, pool, form):
    s, _ = pool
    twin, decide = {"accounts": (_twin_accounts, _decide_accounts), "explicit": (_twin_explicit, _decide_explicit)}[form]
    for protocol in (21, 9):
        ok, weight, used, dig = twin(sv, s, protocol)
        code, fail = rp.fold(s["check_begin"], s["sig_begin"], ok, used, s["check_role"], s["body_flags"])
        assert set(code.tolist()) == {0, 1, 2, 3}  # (every code occurs)
        r = decide(sv, s, protocol, want_checks=True, bad_cap=s["nb"])
        assert (r.body_code == code).all() and (r.body_fail == fail).all()
        assert r.check_ok.tobytes() == ok.tobytes() and r.check_weight.tobytes() == weight.tobytes()
        assert r.check_used.tobytes() == used.tobytes() and r.digests.tobytes() == dig.tobytes()
        bad, n = rp.bad_list(code, s["nb"])
        assert r.n_bad == n and (r.bad_body == bad).all()
        # without the optional outputs: the same codes
        q = decide(sv, s, protocol, want_fail=False)
        assert (q.body_code == code).all() and q.body_fail is None and q.check_ok is None and q.n_bad == n
        assert q.digests.tobytes() == dig.tobytes()


def test_null_roles_and_flags_read_as_tx_and_zero(sv, pool):
    s, _ = pool
    ok, _, used, _ = _twin_accounts(sv, s)
    code, fail = rp.fold(s["check_begin"], s["sig_begin"], ok, used)
    r = _decide_accounts(sv, s, check_role=None, body_flags=None)
    assert (r.body_code == code).all() and (r.body_fail == fail).all() and not (code == rp.OP_BAD_AUTH).any()


def test_constructed_bodies_by_hand(sv, pool):
    s, cases = pool
    assert {"tx_fails_before_op", "op_fails_before_tx", "op_fails_with_unused_signature", "unused_signature",
            "unused_signature_skipped", "no_check_no_signature", "no_check_one_signature",
            "sixty_four_signatures"} <= set(cases)
    for r in (_decide_accounts(sv, s), _decide_explicit(sv, s)):
        for name, (t, code, fail) in cases.items():
            assert (int(r.body_code[t]), int(r.body_fail[t])) == (code, fail), name
    t = cases["sixty_four_signatures"][0]
    assert int(s["sig_begin"][t + 1] - s["sig_begin"][t]) == 64
    ok, _, used, _ = _twin_accounts(sv, s)
    c = int(s["check_begin"][t])
    assert ok[c] == 1 and int(used[c]) == 2**64 - 1


def test_bad_list_capacities(sv, pool):
    """bad_cap 0, 1, exactly n_bad and larger, over arrays of the test's own with
    guard words behind the capacity."""
    s, _ = pool
    full = _decide_accounts(sv, s, bad_cap=s["nb"])
    n = full.n_bad
    assert 2 < n < s["nb"] and (np.diff(full.bad_body.astype(np.int64)) > 0).all()
    assert (full.bad_body == np.flatnonzero(full.body_code != 0)).all()
    for cap in (0, 1, n, n + 7):
        code = np.zeros(s["nb"], np.uint8)
        bad = np.full(cap + 8, 0xA5A5A5A5, np.uint32)
        n_bad = np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64)
        res = sv.results_desc(check_role=s["check_role"].ctypes.data, body_flags=s["body_flags"].ctypes.data,
                              body_code=code.ctypes.data, bad_body=bad.ctypes.data if cap else 0, bad_cap=cap,
                              n_bad=n_bad[1:].ctypes.data)
        _decide_accounts(sv, s, res=res)
        assert (code == full.body_code).all()
        assert int(n_bad[1]) == n and n_bad[0] == n_bad[2] == 0xA5A5A5A5A5A5A5A5
        k = min(cap, n)
        assert (bad[:k] == full.bad_body[:k]).all() and (bad[k:] == 0xA5A5A5A5).all()
    # a list without a count, a count without a list
    code, bad = np.zeros(s["nb"], np.uint8), np.full(n, 0xA5A5A5A5, np.uint32)
    _decide_accounts(sv, s, res=sv.results_desc(s["check_role"].ctypes.data, s["body_flags"].ctypes.data,
                                                code.ctypes.data, bad_body=bad.ctypes.data, bad_cap=n))
    assert (bad == full.bad_body).all()


def test_no_body(sv):
    """No body at all: nothing fails, the count is written."""
    n_bad = np.full(1, 7, np.uint64)
    code = np.zeros(1, np.uint8)
    r = sv.decide_txbodies_accounts_cpu(tp.NETWORK_ID, np.zeros(0, np.uint8), np.zeros(0, np.uint64),
                                        np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(1, np.uint64),
                                        np.zeros((0, 4), np.uint8), np.zeros((0, 64), np.uint8),
                                        np.zeros((0, 32), np.uint8), np.zeros((0, 4), np.uint8), np.zeros(1, np.uint64),
                                        [], [], np.zeros((0, 32), np.uint8), None, None, None, np.zeros(1, np.uint64),
                                        [], np.zeros(1, np.uint64), [], [],
                                        res=sv.results_desc(body_code=code.ctypes.data, n_bad=n_bad.ctypes.data))
    assert r.shape == (0, 32) and int(n_bad[0]) == 0


# ------------------------------------------------ every refusal alone
def _refused(sv, fn, s, explicit=False, **res_over):
    """rc of one host-array decide entry point over an sv_txresults of the test's own."""
    code = np.zeros(s["nb"], np.uint8)
    spec = dict(check_role=s["check_role"].ctypes.data, body_flags=s["body_flags"].ctypes.data,
                body_code=code.ctypes.data)
    keep = [v for v in res_over.values() if isinstance(v, np.ndarray)]
    spec.update({k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in res_over.items()})
    res = sv.results_desc(**spec)
    try:
        if explicit:
            a, kw = ap.explicit_args(s)
            fn(*a, res=res, **kw)
        else:
            fn(*ap.args(s), sig_len=s["sig_len"], res=res)
    except sv.SigVerifyError as e:
        del keep
        return str(e).split(":")[0]
    return "SV_OK"


@pytest.mark.parametrize("form", ["accounts_cpu", "explicit_cpu", "accounts", "explicit"])
def test_every_refusal(sv, pool, form):
    """The GPU host forms refuse before any device work, so they are tested here
    too: a refusal never reaches the engine."""
    s, _ = pool
    fn = {"accounts_cpu": sv.decide_txbodies_accounts_cpu, "explicit_cpu": sv.decide_txbodies_cpu,
          "accounts": sv.decide_txbodies_accounts, "explicit": sv.decide_txbodies}[form]
    ex = form.startswith("explicit")
    bad = "SV_ERR_INVALID_ARG"
    if form.endswith("cpu"):
        assert _refused(sv, fn, s, ex) == "SV_OK"
    role = s["check_role"].copy()
    role[len(role) // 2] = 2
    assert _refused(sv, fn, s, ex, check_role=role) == bad
    flags = s["body_flags"].copy()
    flags[-1] = 2
    assert _refused(sv, fn, s, ex, body_flags=flags) == bad
    flags[-1] = 0x81
    assert _refused(sv, fn, s, ex, body_flags=flags) == bad
    assert _refused(sv, fn, s, ex, body_code=0) == bad
    size = ctypes.sizeof(sv.sv_txresults)
    assert _refused(sv, fn, s, ex, struct_size=size - 8) == bad
    assert _refused(sv, fn, s, ex, struct_size=0) == bad
    assert _refused(sv, fn, s, ex, bad_body=0, bad_cap=1) == bad
    # what the twin refuses: a malformed CSR array, protocol 7 goes the same way
    cb = s["check_begin"].copy()
    cb[1], cb[2] = cb[2] + 1, cb[1]
    code = np.zeros(s["nb"], np.uint8)
    res = sv.results_desc(body_code=code.ctypes.data)
    with pytest.raises(sv.SigVerifyError, match=bad):
        if ex:
            a, kw = ap.explicit_args(s)
            a = list(a)
            a[10] = cb
            fn(*a, res=res, **kw)
        else:
            fn(*ap.args(s, check_begin=cb), sig_len=s["sig_len"], res=res)
    with pytest.raises(sv.SigVerifyError, match=bad):
        if ex:
            a, kw = ap.explicit_args(s)
            fn(*a, res=res, protocol_version=7, **kw)
        else:
            fn(*ap.args(s), sig_len=s["sig_len"], res=res, protocol_version=7)


def test_exported_and_documented(sv):
    lib = sv.load_library()
    for name in ("sv_ed25519_decide_txbodies", "sv_ed25519_decide_txbodies_device", "sv_ed25519_decide_txbodies_cpu",
                 "sv_ed25519_decide_txbodies_accounts", "sv_ed25519_decide_txbodies_accounts_device",
                 "sv_ed25519_decide_txbodies_accounts_cpu"):
        assert name in sv.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sv_txresult_block() == 64
    with open(os.path.join(REPO, "include", "stellar_sigverify.h")) as fh:
        header = fh.read()
    for word in ("sv_txresults", "SV_TXRESULT_BAD_AUTH_EXTRA", "SV_TXBODY_SKIP_UNUSED"):
        assert word in header


def test_native_header_twin(tmp_path):
    """tests/native/txresult_core.cpp: csrc/txresult.h instantiated for the host,
    under the address and undefined-behaviour sanitizers, against plain loops."""
    exe = str(tmp_path / "txresult_core")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
           "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-o", exe, os.path.join(HERE, "native", "txresult_core.cpp")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "txresult_core ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ------------------------------------------------ the mirror: prefetch 8
class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _host_lib(sv):
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_signer_lists_built.restype = ctypes.c_uint64
    host.svh_decided_walks.restype = ctypes.c_uint64
    return host


def _failing_envelopes(oracle):
    """Envelopes that fail in every way a transaction's signatures can, beside two that pass: a signature by a
    key that is no signer (txBAD_AUTH), a surplus signature (txBAD_AUTH_EXTRA), an operation on another account
    that did not sign (txFAILED / opBAD_AUTH at operation 1), an operation whose source account is missing and did
    not sign (the same through the no-account check), a missing transaction source (txNO_ACCOUNT), a missing
    extra signer, fee bumps with an unused outer signature, a wrong outer signer and a failing inner transaction.
    -> (names, envelope arrays with junk hashes, the other arrays, accounts, bodies, ebody)"""
    rng = np.random.default_rng(78)
    A, F, X, E = range(4)
    seeds = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    names = ("ok", "wrong_key", "extra_sig", "op_bad_auth", "op_no_account_unsigned", "no_source",
             "extra_signer_missing", "bump_ok", "bump_extra_sig", "bump_bad_outer", "bump_inner_fails")
    blob, ebody = bytearray(), np.zeros(len(names), eb.ENVELOPE_BODY)
    jobs, plans = [(k, bytes(32)) for k in range(4)], []

    def new_body():
        b = bytes(rng.integers(0, 256, 4 * int(rng.integers(25, 60)), dtype=np.uint8))
        off = len(blob)
        blob.extend(b)
        return off, b

    def job(k, msg):
        jobs.append((k, msg))
        return len(jobs) - 1

    for t, name in enumerate(names):
        off, body = new_body()
        ebody[t]["off"], ebody[t]["len"], ebody[t]["kind"] = off, len(body), tp.V1
        inner = tp.contents_hash(tp.V1, body)
        signer = X if name in ("wrong_key", "no_source", "bump_inner_fails") else A
        plan = {"rows": [job(signer, inner)], "outer_rows": []}
        if name == "extra_sig":
            plan["rows"].append(job(E, inner))
        if name.startswith("bump"):
            ooff, obody = new_body()
            ebody[t]["outer_off"], ebody[t]["outer_len"] = ooff, len(obody)
            outer = tp.contents_hash(tp.FEE_BUMP, obody)
            plan["outer_rows"] = [job(A if name == "bump_bad_outer" else F, outer)]
            if name == "bump_extra_sig":
                plan["outer_rows"].append(job(A, outer))
        plans.append(plan)
    pk, sig = tp.pysign_signer(oracle)(seeds[[k for k, _ in jobs]],
                                       np.array([np.frombuffer(m, np.uint8) for _, m in jobs], np.uint8))
    keys = [pk[k].tobytes() for k in range(4)]
    hx = lambda k: keys[k].hex()  # noqa: E731
    dsig = lambda row: {"hint": pk[row].tobytes()[28:].hex(), "sig": sig[row].tobytes().hex()}  # noqa: E731
    accounts = [{"id": hx(A), "thresholds": [1, 0, 0, 0], "signers": []},
                {"id": hx(F), "thresholds": [1, 0, 0, 0], "signers": []}]
    es = ev.EnvelopeSet()
    for a in accounts:
        es.account(a)
    for t, name in enumerate(names):
        source, ops, extra, fee = hx(A), [{"level": 2}], (), None
        if name == "op_bad_auth":
            ops = [{"level": 1}, {"level": 2, "source": hx(F)}, {"level": 1}]
        if name == "op_no_account_unsigned":
            ops = [{"level": 1}, {"level": 2, "source": hx(X)}]
        if name == "no_source":
            source = hx(X)
        if name == "extra_signer_missing":
            extra = [{"type": 0, "key": hx(E), "weight": 1}]
        if name.startswith("bump"):
            fee = {"hash": (b"\xbb" * 32).hex(), "fee_source": hx(F), "sigs": [dsig(r) for r in plans[t]["outer_rows"]]}
        es.envelope(source, (b"\xaa" * 32).hex(), [dsig(r) for r in plans[t]["rows"]], ops, extra=extra, fee_bump=fee)
    return names, es.arrays(), len(accounts), np.frombuffer(bytes(blob), np.uint8).copy(), ebody


def test_mirror_prefetch8_failing_envelopes(sv, oracle):
    """Prefetch 8 gives prefetch 0's svh_tx_results -- code, inner code, failed operation and its code -- in both
    modes and at protocols on both sides of "no operation checks for_apply below 10", of fee bumps (13) and of
    the extra signers (19); the walk counter moves by exactly the failing transactions; one engine call per call."""
    host = _host_lib(sv)
    names, arrays, naccounts, bodies, ebody = _failing_envelopes(oracle)
    n = len(names)

    def call(prefetch, for_apply=0, protocol=21):
        return eb.check_envelopes_bodies(host, arrays[0], *arrays[1:], n, naccounts, protocol, bodies, ebody,
                                         prefetch=prefetch, for_apply=for_apply)

    ref = call(0)[0]
    assert dict(zip(names, ref["code"].tolist())) == {
        "ok": 0, "wrong_key": -6, "extra_sig": -10, "op_bad_auth": -1, "op_no_account_unsigned": -1, "no_source": -8,
        "extra_signer_missing": -6, "bump_ok": 1, "bump_extra_sig": -10, "bump_bad_outer": -6, "bump_inner_fails": -13}
    assert int(ref["failed_op"][names.index("op_bad_auth")]) == 1
    for protocol in (21, 18, 12, 9):
        for for_apply in (0, 1):
            want = call(0, for_apply, protocol)
            walks, built = host.svh_decided_walks(), host.svh_signer_lists_built()
            got = call(8, for_apply, protocol)
            assert (got[0] == want[0]).all(), (protocol, for_apply, got[0], want[0])
            assert (got[2] == want[2]).all() and (got[3] == want[3]).all()
            failing = int(((want[0]["code"] != 0) & (want[0]["code"] != 1)).sum())
            assert host.svh_decided_walks() - walks == failing, (protocol, for_apply)
            assert host.svh_signer_lists_built() == built
            seven = call(7, for_apply, protocol)
            assert (seven[0] == want[0]).all() and seven[1] == got[1]
    # for_apply below protocol 10: the operations are not checked and nobody asks whether every signature was used
    assert call(8, 1, 9)[0]["code"][names.index("extra_sig")] == 0 == call(8, 1, 9)[0]["code"][names.index("op_bad_auth")]
    # protocol 7: every check is true without the engine
    assert (call(8, 0, 7)[0] == call(0, 0, 7)[0]).all()


@pytest.mark.parametrize("with_payload", [True, False])
def test_mirror_prefetch8_matches_prefetch0(sv, oracle, with_payload):
    """The envelope units of envelope_bodies.py (V1, V0, fee bump, multisig, signed payload, mutated body):
    prefetch 0's results and hashes through ONE engine call (the CPU form on a host without a GPU: one fallback
    counted); the valid envelopes alone move neither the walk counter nor the signer-list counter, the whole set
    moves the walk counter by its failing envelopes."""
    host = _host_lib(sv)
    s = eb.build_set(2, 23, tp.pysign_signer(oracle), with_payload=with_payload)

    def call(prefetch, for_apply=0, idx=None):
        envs, ebody = (s["envs_blank"], s["ebody"]) if idx is None else (s["envs_blank"][idx].copy(),
                                                                          s["ebody"][idx].copy())
        return eb.check_envelopes_bodies(host, envs, *s["rest"], len(envs) if idx is not None else s["n"],
                                         s["naccounts"], 21, s["bodies"], ebody, prefetch=prefetch,
                                         for_apply=for_apply)

    def stats():
        st = EngineStats()
        host.svh_engine_counts_ex(ctypes.byref(st))
        return st

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all() and eb.txBAD_AUTH in ref["code"]
    for for_apply in (0, 1):
        want = call(0, for_apply)
        stats()
        walks = host.svh_decided_walks()
        got = call(8, for_apply)
        st = stats()
        assert (got[0] == want[0]).all() and (got[2] == ch0).all() and (got[3] == fb0).all()
        assert (got[2] == s["contents_hash"]).all() and (got[3] == s["fee_bump_hash"]).all()
        assert got[1] == 2 * s["n"] + s["kinds"].count("fee_bump")
        assert host.svh_decided_walks() - walks == s["kinds"].count("mutated") == 2
        gpu = sv.device_count() > 0 if _can_count(sv) else False
        assert (st.fallbacks, st.gpu_batches) == ((0, 1) if gpu else (1, 0))
    valid = np.array([i for i, k in enumerate(s["kinds"]) if k != "mutated"])
    want = call(0, idx=valid)
    walks, built = host.svh_decided_walks(), host.svh_signer_lists_built()
    got = call(8, idx=valid)
    assert (got[0] == want[0]).all() and set(got[0]["code"].tolist()) == {0, 1}
    assert host.svh_decided_walks() == walks and host.svh_signer_lists_built() == built


def _can_count(sv):
    try:
        sv.device_count()
        return True
    except sv.SigVerifyError:
        return False
