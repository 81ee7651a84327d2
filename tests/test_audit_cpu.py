"""The verdict audit on the host (include/stellar_sigverify.h sv_audit_batch_cpu, sv_set_audit): the textbook
verifier against the fixtures, the pick against a pure-Python model, the budget, the refusals and the stats
layout.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audit_model as am  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cpu(sv, d, claimed, what, **kw):
    return sv.audit_batch_cpu(d["pk"], d["sig"], d["msg"], d["msg_off"], d["msg_len"], claimed, what, **kw)


@pytest.mark.parametrize("name", am.SETS)
def test_textbook_verifier_is_libsodium_exact(sv, golden, name):
    """Every row of every fixture set, claimed = the fixture's (libsodium's) verdict: all audited, none differs."""
    d = golden[name]
    n = len(d["verdict"])
    st, recs = run_cpu(sv, d, d["verdict"], am.SAMPLE, one_in=1, budget=sv.AUDIT_BUDGET_MAX)
    assert (st["audited"], st["mismatches"], st["over_budget"]) == (n, 0, 0)
    assert st["audited_rejects"] == int((d["verdict"] == 0).sum())
    assert recs == []
    if am.is_fixed32(d):  # the fixed-length form over the same bytes
        st, recs = sv.audit_batch_cpu(d["pk"], d["sig"], d["msg"], None, None, d["verdict"], am.SAMPLE, one_in=1,
                                      fixed_msg_len=32, budget=sv.AUDIT_BUDGET_MAX)
        assert (st["audited"], st["mismatches"]) == (n, 0) and recs == []


def test_fixed_and_offset_modes_are_both_covered(golden):
    assert any(am.is_fixed32(golden[s]) for s in am.SETS) and any(not am.is_fixed32(golden[s]) for s in am.SETS)


@pytest.mark.parametrize("name", am.SETS)
def test_inverted_rows_are_found(sv, golden, name):
    d = golden[name]
    rows = am.inverted_rows(name, d)
    claimed = d["verdict"].copy()
    claimed[rows] ^= 1
    st, recs = run_cpu(sv, d, claimed, am.SAMPLE, one_in=1, seq=5, budget=sv.AUDIT_BUDGET_MAX)
    assert st["mismatches"] == len(rows) and st["records_held"] == len(rows) and st["records_lost"] == 0
    assert [r["row"] for r in recs] == rows  # exactly those, ascending
    for r in recs:
        i = r["row"]
        want = int(d["verdict"][i])
        assert (r["engine"], r["audit"], r["cpu"], r["seq"]) == (want ^ 1, want, want, 5)
        assert r["pk"] == d["pk"][i].tobytes() and r["sig"] == d["sig"][i].tobytes()
        ln, off = int(d["msg_len"][i]), int(d["msg_off"][i])
        assert r["msg_len"] == ln and r["flags"] == (1 if ln > sv.AUDIT_MSG_MAX else 0)
        assert r["msg"] == d["msg"][off:off + min(ln, sv.AUDIT_MSG_MAX)].tobytes()


def test_pick_model_rejects_only(sv, golden):
    d = golden["adversarial"]
    st, _ = run_cpu(sv, d, d["verdict"], am.REJECTS, seq=3)
    want, over = am.audited(am.REJECTS, 0, 0, 3, d["verdict"])
    assert st["audited"] == len(want) == int((d["verdict"] == 0).sum()) and st["audited_rejects"] == len(want)
    assert over == st["over_budget"] == 0
    # which rows: an accept claimed as a reject is picked and leaves a record, a reject claimed as an accept is not
    v = d["verdict"]
    acc, rej = int(np.flatnonzero(v == 1)[0]), int(np.flatnonzero(v == 0)[0])
    claimed = v.copy()
    claimed[acc], claimed[rej] = 0, 1
    st, recs = run_cpu(sv, d, claimed, am.REJECTS, seq=3)
    picked = am.picks(am.REJECTS, 0, 0, 3, claimed)
    assert acc in picked and rej not in picked and st["audited"] == len(picked)
    assert [r["row"] for r in recs] == [acc]


def test_pick_model_sample_crosses_second_level_scan(sv, golden):
    """n = 65,536 + 300 rows tiled from `valid`, one_in = 64: about 1,030 picks.  Every claimed verdict is inverted,
    so the mismatch count is the audited count, and the records name the first audited rows."""
    n = 65536 + 300
    d = am.tiled(golden["valid"], n)
    seed, seq = 0x5EED, 7
    want, over = am.audited(am.SAMPLE, 64, seed, seq, d["verdict"])
    assert 900 < len(want) < 1160 and over == 0
    st, recs = run_cpu(sv, d, d["verdict"] ^ 1, am.SAMPLE, one_in=64, seed=seed, seq=seq)
    assert st["audited"] == st["mismatches"] == len(want)
    assert [r["row"] for r in recs] == want[:sv.AUDIT_RING]
    assert st["records_lost"] == len(want) - sv.AUDIT_RING
    # another seq or seed picks other rows
    assert am.picks(am.SAMPLE, 64, seed, seq + 1, d["verdict"]) != want


def test_pick_model_both_bits(sv, golden):
    d = golden["adversarial"]
    seed, seq = 11, 2
    claimed = d["verdict"].copy()
    want, _ = am.audited(am.REJECTS | am.SAMPLE, 3, seed, seq, claimed)
    assert set(np.flatnonzero(claimed == 0)) <= set(want) and len(want) < len(claimed)
    st, recs = run_cpu(sv, d, claimed, am.REJECTS | am.SAMPLE, one_in=3, seed=seed, seq=seq)
    assert st["audited"] == len(want) and st["mismatches"] == 0
    # a wrong accept claim is found iff the sample picks its row
    rej = [int(i) for i in np.flatnonzero(d["verdict"] == 0)]
    c2 = d["verdict"].copy()
    c2[rej] = 1
    want2, _ = am.audited(am.REJECTS | am.SAMPLE, 3, seed, seq, c2)
    st, recs = run_cpu(sv, d, c2, am.REJECTS | am.SAMPLE, one_in=3, seed=seed, seq=seq)
    assert st["audited"] == len(want2)
    assert [r["row"] for r in recs] == [i for i in want2 if i in set(rej)][:sv.AUDIT_RING]


def test_budget(sv, golden):
    """600 claimed rejects, budget 300: the first 300 are audited, 300 are over budget, and of five truly valid rows
    only those among the first 300 are recorded."""
    v = golden["valid"]
    good = np.flatnonzero(v["verdict"] == 1)[:600]
    assert len(good) == 600
    d = {k: v[k][good] for k in ("pk", "sig", "msg_off", "msg_len", "verdict")}
    d["msg"] = v["msg"]
    valid_rows = [3, 150, 299, 300, 599]
    sig = d["sig"].copy()
    bad = np.ones(600, bool)
    bad[valid_rows] = False
    sig[bad, 40] ^= 1  # every other row is a true reject
    d["sig"] = sig
    claimed = np.zeros(600, np.uint8)
    st, recs = run_cpu(sv, d, claimed, am.REJECTS, budget=300)
    assert (st["audited"], st["over_budget"], st["audited_rejects"]) == (300, 300, 300)
    assert [r["row"] for r in recs] == [3, 150, 299] and st["mismatches"] == 3
    assert all((r["engine"], r["audit"], r["cpu"]) == (0, 1, 1) for r in recs)


def test_set_audit_refusals(sv):
    lib = sv.load_library()
    bad = [(8, 1, 0, 0), (0x10 | am.SAMPLE, 1, 0, 0), (am.SAMPLE, 0, 0, 0), (am.SAMPLE | am.STRICT, 0, 0, 0),
           (am.REJECTS, 0, 0, sv.AUDIT_BUDGET_MAX + 1)]
    for what, one_in, seed, budget in bad:
        assert lib.sv_set_audit(what, one_in, seed, budget) == -1, (what, one_in, budget)
    try:
        for what, one_in, seed, budget in [(am.REJECTS, 0, 0, 0), (am.SAMPLE, 1, 9, sv.AUDIT_BUDGET_MAX),
                                           (am.REJECTS | am.SAMPLE | am.STRICT, 64, 1, 1)]:
            assert lib.sv_set_audit(what, one_in, seed, budget) == 0
    finally:
        assert lib.sv_set_audit(0, 0, 0, 0) == 0
    with pytest.raises(ValueError):
        sv.set_audit(-1)
    assert sv.SV_ERRORS[sv.SV_ERR_AUDIT] == "SV_ERR_AUDIT" and sv.SV_ERR_AUDIT == -9


def test_cpu_form_refusals_and_empty_batch(sv, golden):
    d = golden["intree"]
    st, recs = sv.audit_batch_cpu(np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8), np.zeros(0, np.uint8),
                                  np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8), am.REJECTS)
    assert st["audited"] == 0 and recs == []  # n == 0 is SV_OK
    for kw in ({"what": 8}, {"what": am.SAMPLE, "one_in": 0}, {"what": am.STRICT},
               {"what": am.REJECTS, "budget": sv.AUDIT_BUDGET_MAX + 1}):
        what = kw.pop("what")
        with pytest.raises(sv.SigVerifyError):
            run_cpu(sv, d, d["verdict"], what, **kw)


def test_dissent_knob_needs_opt_in(sv):
    """SV_DBG_AUDIT_DISSENT changes what a strict call returns: refused without SV_TEST_KNOBS=1 (a child process:
    this one opted in)."""
    code = ("import ctypes,sys; l=ctypes.CDLL(sys.argv[1]); l.sv_set_debug_flags.argtypes=[ctypes.c_uint32];"
            "print(l.sv_set_debug_flags(0x100), l.sv_set_debug_flags(1), l.sv_set_debug_flags(0x200), "
            "l.sv_set_debug_flags(0))")
    env = {k: v for k, v in os.environ.items() if k != "SV_TEST_KNOBS"}
    env["SV_NO_TORCH"] = "1"
    out = subprocess.run([sys.executable, "-c", code, sv.LIB_PATH], env=env, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["-1", "0", "-1", "1"]
    env["SV_TEST_KNOBS"] = "1"
    out = subprocess.run([sys.executable, "-c", code, sv.LIB_PATH], env=env, capture_output=True, text=True,
                         timeout=120)
    assert out.stdout.split() == ["0", "256", "-1", "1"]


def test_short_stats_struct_is_written_only_up_to_its_size(sv, golden):
    d = golden["intree"]
    lib = sv.load_library()
    n = len(d["verdict"])
    words = ctypes.sizeof(sv.AuditStats) // 8
    keep = 5  # struct_size .. audited_rejects
    buf = (ctypes.c_uint64 * words)(*([0xA5A5A5A5A5A5A5A5] * words))
    buf[0] = 8 * keep
    o = sv.AuditOpts(ctypes.sizeof(sv.AuditOpts), am.SAMPLE, 1, 0, 0, 0)
    nr = ctypes.c_size_t(99)
    a = {k: np.ascontiguousarray(d[k]) for k in d}
    off, ln = a["msg_off"].astype(np.uint64), a["msg_len"].astype(np.uint32)  # (kept alive across the call)
    rc = lib.sv_audit_batch_cpu(ctypes.byref(o), a["pk"].ctypes.data, a["sig"].ctypes.data, a["msg"].ctypes.data,
                                off.ctypes.data, ln.ctypes.data, 0, n, a["verdict"].ctypes.data,
                                ctypes.cast(buf, ctypes.c_void_p), None, 0, ctypes.byref(nr), 1)
    assert rc == 0 and nr.value == 0
    assert list(buf[:keep]) == [8 * keep, am.SAMPLE, 0, n, int((d["verdict"] == 0).sum())]
    assert all(w == 0xA5A5A5A5A5A5A5A5 for w in buf[keep:])
    buf[0] = 0  # too small to name itself
    assert lib.sv_audit_batch_cpu(ctypes.byref(o), a["pk"].ctypes.data, a["sig"].ctypes.data, a["msg"].ctypes.data,
                                  None, None, 0, 0, None, ctypes.cast(buf, ctypes.c_void_p), None, 0, None, 1) == -1


def test_sanitizer_run_of_the_cpu_form(tmp_path):
    """tests/native/audit_san.cpp (its own main) with csrc/sv_cpu.cpp, built with ASan and UBSan and run directly:
    nothing is loaded into Python."""
    exe = str(tmp_path / "audit_san")
    csrc = os.path.join(REPO, "stellar-core_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-Wno-unknown-pragmas", "-I", csrc, "-o", exe,
           os.path.join(REPO, "tests", "native", "audit_san.cpp"), os.path.join(csrc, "sv_cpu.cpp"), "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "audit_san ok: 1204 rows" in r.stdout, r.stdout[-4000:]
