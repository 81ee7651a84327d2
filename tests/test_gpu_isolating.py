"""GPU verdicts on the isolating rows (tests/isolating_rows.py) through the
public entry points: rows whose point equation holds while exactly one of
libsodium's reject conditions fails -- every blacklist encoding as A and as R,
S >= L below and above 2^253 -- interleaved with accepts (valid and
mixed-order rows).  A kernel path that lost its small-order term for A or R,
or whose blacklist has one constant wrong, accepts one of them.

One mixed batch per message length (32: MODE 0 / 1, 33: MODE 2 / 1), n = 195 =
3 * 64 + 3, the iso_* rows on lanes 0, 63, 64 and on the last index; expected
verdicts are the oracle's.  Paths: the throughput path in both geometries and
the default path; the lattice test knobs; the latency path cold (two-wave
through the device API, three-wave narrow and wide through the host API) and
warm (comb kernel: every key, the small-order ones included, has a cache slot
whose status decides (3)-(5)); the per-key tables of the throughput path in
all three message modes (A's status comes from the table); the keyed call and
the gather entry; the device API in its three message forms with the bitmap;
and the mirror's CPU fallback under SV_DBG_FAIL.
"""
import ctypes
import hashlib

import numpy as np
import pytest

import isolating_rows as ir
from conftest import oracle_verdicts
from launchers import check_bitmap
from test_gpu_comb import _warm_up
from test_gpu_keytables import tables  # noqa: F401  (fixture)
from test_host_mirror import EngineStats

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 3 * 64 + 3
MLENS = (32, 33)
_batches = {}


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(params=MLENS)
def batch(request, oracle):
    """(rows, oracle verdicts) of the mixed batch, made once per message length."""
    mlen = request.param
    if mlen not in _batches:
        d = ir.generate(mlen)
        rows = ir.interleaved(d, N)
        assert set(rows.tolist()) == set(range(len(d["cls"])))  # every generated row is in the batch
        b = ir.gather(d, rows)
        assert all(b["cls"][i] < 4 for i in (0, 63, 64, N - 1))
        want = oracle_verdicts(oracle, b)
        assert np.array_equal(want, b["verdict"])  # iso_* rows 0, controls 1
        want.setflags(write=False)
        _batches[mlen] = (b, want)
    return _batches[mlen]


def _check(b, got, want, what=""):
    bad = np.nonzero(np.asarray(got) != want)[0]
    assert len(bad) == 0, (what, [(int(i), str(b["class_names"][b["cls"][i]]), int(b["enc"][i])) for i in bad[:10]])


def _host(sv, b, **kw):
    return sv.verify_batch(b["pk"], b["sig"], b["msg"], b["msg_off"], b["msg_len"], device=0, **kw)


@pytest.mark.parametrize("geom", ["default", "no_quad", "quad"])
def test_throughput_geometries_and_default_path(sv, dev, batch, geom):
    b, want = batch
    prev = sv.set_debug_flags({"default": 0, "no_quad": sv.DBG_NO_QUAD, "quad": sv.DBG_QUAD}[geom])
    try:
        _check(b, _host(sv, b, path="throughput"), want, "throughput")
        if geom == "default":
            _check(b, _host(sv, b), want, "default path")
    finally:
        sv.set_debug_flags(prev)


@pytest.mark.parametrize("knobs", ["trivial_pair", "max_windows", "both"])
def test_lattice_knobs(sv, dev, batch, knobs):
    """The forced fallback pair and 64 windows, on the one-lane, the quad and the cold octet kernels."""
    b, want = batch
    f = {"trivial_pair": sv.DBG_TRIVIAL_PAIR, "max_windows": sv.DBG_MAX_WINDOWS,
         "both": sv.DBG_TRIVIAL_PAIR | sv.DBG_MAX_WINDOWS}[knobs]
    prev = sv.set_debug_flags(f | sv.DBG_NO_QUAD)
    sv.set_key_cache(0)
    try:
        _check(b, _host(sv, b, path="throughput"), want, "one-lane")
        _check(b, _host(sv, b, path="latency"), want, "octet")
        sv.set_debug_flags(f | sv.DBG_QUAD)
        _check(b, _host(sv, b, path="throughput"), want, "quad")
    finally:
        sv.set_debug_flags(prev)
        sv.set_key_cache(1024)


@pytest.mark.parametrize("n", [N, 2048 + N])
def test_latency_cold_three_wave(sv, dev, batch, n):
    """Cold host batches on the lane take the three-wave octet kernel: the
    narrow split up to 2048 signatures, the wide one above."""
    b, want = batch
    rows = np.arange(n) % N
    sv.set_key_cache(0)
    try:
        w0 = sv.key_cache_stats(0)["warm_batches"]
        out = sv.verify_batch(b["pk"][rows], b["sig"][rows], b["msg"], b["msg_off"][rows], b["msg_len"][rows], device=0,
                              path="latency")
        assert sv.key_cache_stats(0)["warm_batches"] == w0
    finally:
        sv.set_key_cache(1024)
    bad = np.nonzero(out != want[rows])[0]
    assert len(bad) == 0, [(int(i), str(b["class_names"][b["cls"][rows[i]]]), int(b["enc"][rows[i]])) for i in bad[:10]]


def test_latency_warm(sv, dev, batch):
    """Served by the comb kernel: every key of the batch, the 14 blacklisted
    encodings included, has a cache slot, and a rejecting key's status alone
    rejects its rows (their equation holds).  That the small-order keys are
    cached as SV_KEY_BAD is inferred, not read: the comb kernel does not test A
    itself, only kstat == SV_KEY_OK (sv_comb.hip), so on a warm batch nothing
    else can reject an iso_small_A row.  Should the comb kernel ever check A
    for small order itself, this test no longer shows the cached status; the
    status is read directly in
    tests/test_gpu_instantiations.py::test_keytab_status_and_guard_slots."""
    b, want = batch
    sv.set_key_cache(8192)
    try:
        r = _warm_up(sv, b, want)
        assert r >= 1  # (the first run is cold)
        w0 = sv.key_cache_stats(0)["warm_batches"]
        _check(b, _host(sv, b, path="latency"), want, "warm")
        assert sv.key_cache_stats(0)["warm_batches"] == w0 + 1
    finally:
        sv.set_key_cache(1024)


def _device_call(sv, dev, b, form, bitmap=True):
    """The batch through sv_ed25519_verify_device: form 0 fixed 32 (16-byte
    aligned: MODE 0), 1 msg_off / msg_len (MODE 1), 2 fixed other length (MODE
    2) -> (verdicts, bitmap words incl. one guard word)."""
    n = len(b["verdict"])
    mlen = int(b["msg_len"][0])
    assert (b["msg_len"] == mlen).all() and b["msg"].size >= n * mlen
    assert (form == 0) == (mlen == 32) or form == 1
    pk = torch.from_numpy(b["pk"].copy()).to(dev)
    sig = torch.from_numpy(b["sig"].copy()).to(dev)
    msg = torch.zeros(n * mlen + 32, dtype=torch.uint8, device=dev)  # (the kernels read whole 16-byte blocks)
    msg[:n * mlen] = torch.from_numpy(b["msg"][:n * mlen].copy()).to(dev)
    assert pk.data_ptr() % 16 == 0 and sig.data_ptr() % 16 == 0 and msg.data_ptr() % 16 == 0
    off = torch.from_numpy(b["msg_off"].astype(np.int64)).to(dev)
    ln = torch.from_numpy(b["msg_len"].astype(np.int32)).to(dev)
    assert int((b["msg_off"] + b["msg_len"]).max()) <= n * mlen
    out = torch.full((n + 64,), 7, dtype=torch.uint8, device=dev)
    words = (n + 63) // 64
    bm = torch.full((words + 1,), -1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    if form == 1:
        sv.verify_device(0, pk.data_ptr(), sig.data_ptr(), msg.data_ptr(), n, out.data_ptr(),
                         bm.data_ptr() if bitmap else 0, st, fixed_msg_len=0, d_msg_off=off.data_ptr(),
                         d_msg_len=ln.data_ptr())
    else:
        sv.verify_device(0, pk.data_ptr(), sig.data_ptr(), msg.data_ptr(), n, out.data_ptr(),
                         bm.data_ptr() if bitmap else 0, st, fixed_msg_len=mlen)
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    assert (got[n:] == 7).all()  # nothing past verdict[n]
    return got[:n], bm.cpu().numpy()


@pytest.mark.parametrize("form", ["fixed", "var"])
@pytest.mark.parametrize("kpath", ["latency", "one_lane", "quad"])
def test_device_api_forms_and_bitmap(sv, dev, batch, kpath, form):
    """fixed: MODE 0 on the 32-byte batch, MODE 2 on the 33-byte one; var: MODE 1."""
    b, want = batch
    prev = sv.set_kernel_path(sv.PATH_LATENCY if kpath == "latency" else sv.PATH_THROUGHPUT)
    prev_dbg = sv.set_debug_flags({"latency": 0, "one_lane": sv.DBG_NO_QUAD, "quad": sv.DBG_QUAD}[kpath])
    try:
        f = 1 if form == "var" else (0 if int(b["msg_len"][0]) == 32 else 2)
        got, bm = _device_call(sv, dev, b, f)
    finally:
        sv.set_kernel_path(prev)
        sv.set_debug_flags(prev_dbg)
    _check(b, got, want, (kpath, form))
    check_bitmap(bm, want)


@pytest.mark.parametrize("form", ["fixed", "var"])
def test_key_tables_decide_A(tables, dev, batch, form):  # noqa: F811
    """Per-key tables on (one-lane kernels): the first call claims and builds
    the keys, the second finds every key built, and A's status -- canonical,
    not small-order, decodable -- is the table entry's, not the lane's.  The
    three message modes (sv_prep_kernel<MODE, KT>)."""
    sv = tables
    b, want = batch
    prev = sv.set_kernel_path(sv.PATH_THROUGHPUT)
    try:
        f = 1 if form == "var" else (0 if int(b["msg_len"][0]) == 32 else 2)
        t0 = sv.key_cache_stats(0)["table_launches"]
        for call in range(2):
            got, bm = _device_call(sv, dev, b, f)
            _check(b, got, want, ("tables", form, call))
            check_bitmap(bm, want)
        assert sv.key_cache_stats(0)["table_launches"] == t0 + 2
    finally:
        sv.set_kernel_path(prev)


def test_keyed_call_and_gather(sv, dev, batch):
    b, want = batch
    n = len(want)
    keys = np.zeros((n, 32), np.uint8)
    items = []
    for i in range(n):
        o, ln = int(b["msg_off"][i]), int(b["msg_len"][i])
        m = b["msg"][o:o + ln].tobytes()
        items.append((b["pk"][i].tobytes(), b["sig"][i].tobytes(), m))
        keys[i] = np.frombuffer(hashlib.blake2b(items[-1][0] + items[-1][1] + m, digest_size=32).digest(), np.uint8)
    out, k = sv.verify_batch_keyed(b["pk"], b["sig"], b["msg"], b["msg_off"], b["msg_len"], device=0)
    _check(b, out, want, "keyed")
    assert np.array_equal(k, keys)
    out, k = sv.verify_gather(items, keys=True, device=0)
    _check(b, out, want, "gather")
    assert np.array_equal(k, keys)
    _check(b, sv.verify_gather(items, device=0), want, "gather, no keys")


def test_forced_engine_error_mirror_falls_back(sv, dev, batch):
    """SV_DBG_FAIL: every GPU entry point errs, the C++ mirror re-runs the
    batch on the CPU path -- the same verdicts, one fallback counted."""
    b, want = batch
    n = len(want)
    vp = ctypes.c_void_p
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    host.svh_set_cpu_threshold.argtypes = [ctypes.c_size_t]
    arrs = [np.ascontiguousarray(b[k]) for k in ("pk", "sig", "msg", "msg_off", "msg_len")]
    stats = EngineStats()
    prev = sv.set_debug_flags(sv.DBG_FAIL)
    host.svh_set_cpu_threshold(0)
    try:
        with pytest.raises(sv.SigVerifyError):
            _host(sv, b)
        host.svh_cache_clear()
        host.svh_engine_counts_ex(ctypes.byref(stats))
        out = np.full(n, 7, np.uint8)
        rc = host.svh_verify_sig_batch(vp(arrs[0].ctypes.data), vp(arrs[1].ctypes.data), None, vp(arrs[2].ctypes.data),
                                       vp(arrs[3].ctypes.data), vp(arrs[4].ctypes.data), ctypes.c_size_t(n),
                                       vp(out.ctypes.data))
        assert rc == 0, host.svh_last_error_string()
        _check(b, out, want, "mirror fallback")
        host.svh_engine_counts_ex(ctypes.byref(stats))
        assert stats.fallbacks == 1 and stats.gpu_signatures == 0 and stats.cpu_signatures > 0
    finally:
        sv.set_debug_flags(prev)
        host.svh_set_cpu_threshold(1)
        host.svh_cache_clear()
        host.svh_cache_counts(None, None)
