"""Pairing by hint on the GPU: the count / scan / fill kernels of sv_txpair.hip
and the verify launch behind sv_ed25519_verify_txbodies_hinted / _device, the
scan's tile seams, the chunking (by signatures, by keys), the slicing over two
slots, the capacity error and the host mirror's prefetch 3.  Expected pairs,
digests and verdicts come from the plain-Python contract in txpairs_pool.py
(double loop, hashlib, the oracle; verdicts by construction for the large
GPU-signed sets), never from the engine."""
import ctypes

import numpy as np
import pytest

import envelope_bodies as eb
import txbodies_pool as tp
import txpairs_pool as pp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = (1, 63, 64, 65, 257)
# the scan's tile sizes (sv_txpair.hip): SV_PAIRBLOCK bodies per block of the
# count / fill kernels, and SV_PAIRBLOCK blocks per lane-run of its one
# second-level block (up to SV_PAIRBLOCK^2 bodies each lane sums one block)
PAIR_BLOCK = 256
SEAMS = (PAIR_BLOCK - 1, PAIR_BLOCK, PAIR_BLOCK + 1, PAIR_BLOCK ** 2 - 1, PAIR_BLOCK ** 2, PAIR_BLOCK ** 2 + 1)


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    assert sv.load_library().sv_pair_block() == PAIR_BLOCK
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def small_sets(sv, dev, oracle):
    """One pool set per size with its expected results; shared and left unchanged."""
    signer = tp.device_signer(sv)
    out = {}
    for nb in SMALL:
        s = pp.make_pool(nb, 300 + nb, signer)
        out[nb] = (s, pp.expected(s, oracle))
    return out


@pytest.fixture(params=["throughput", "quad", "default"])
def kpath(sv, request):
    """The throughput path forced in both geometries, and the default path."""
    if request.param == "default":
        yield
        return
    prev = sv.set_kernel_path(sv.PATH_THROUGHPUT)
    prev_dbg = sv.set_debug_flags({"throughput": sv.DBG_NO_QUAD, "quad": sv.DBG_QUAD}[request.param])
    yield
    sv.set_kernel_path(prev)
    sv.set_debug_flags(prev_dbg)


def _bits(words, n):
    w = np.ascontiguousarray(words).view(np.uint64)
    return ((w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1)[:n]


def _device_call(sv, dev, s, cap):
    """sv_ed25519_verify_txbodies_hinted_device over the set as it is packed ->
    ((pair_begin, pair_sig, pair_key, verdict, digests), bitmap words, n_pairs);
    the pair arrays hold `cap` entries plus a guard that must stay untouched."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    nb, ns, nk = s["nb"], s["ns"], s["nk"]
    t_bodies, t_off, t_len, t_kind = up(s["bodies"]), up(s["off"]), up(s["len"]), up(s["kind"])
    t_sb, t_kb = up(s["sig_begin"]), up(s["key_begin"])
    pad = lambda a, w: a if len(a) else np.zeros((1, w), np.uint8)  # noqa: E731
    t_hint, t_sig, t_key = up(pad(s["hint"], 4)), up(pad(s["sig"], 64)), up(pad(s["key"], 32))
    t_pb = torch.full((nb + 2,), -1, dtype=torch.int64, device=dev)
    t_ps = torch.full((cap + 1,), -1, dtype=torch.int32, device=dev)
    t_pk = torch.full((cap + 1,), -1, dtype=torch.int32, device=dev)
    t_v = torch.full((cap + 1,), 7, dtype=torch.uint8, device=dev)
    t_bm = torch.full(((cap + 63) // 64 + 1,), -1, dtype=torch.int64, device=dev)
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = sv.verify_txbodies_hinted_device(0, tp.NETWORK_ID, t_bodies.data_ptr(), t_off.data_ptr(), t_len.data_ptr(),
                                         t_kind.data_ptr(), nb, t_sb.data_ptr(), t_hint.data_ptr(), t_sig.data_ptr(),
                                         ns, t_kb.data_ptr(), t_key.data_ptr(), nk, cap, t_pb.data_ptr(),
                                         t_ps.data_ptr(), t_pk.data_ptr(), t_v.data_ptr(), t_bm.data_ptr(),
                                         t_dig.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    pb = t_pb.cpu().numpy()
    assert pb[nb + 1] == -1 and t_ps.cpu().numpy()[n:].tolist() == [-1] * (cap + 1 - n)
    assert (t_pk.cpu().numpy()[n:] == -1).all() and (t_v.cpu().numpy()[n:] == 7).all()
    got = (pb[:nb + 1].astype(np.uint64), t_ps.cpu().numpy()[:n].astype(np.uint32),
           t_pk.cpu().numpy()[:n].astype(np.uint32), t_v.cpu().numpy()[:n], t_dig.cpu().numpy())
    return got, t_bm.cpu().numpy(), n


def _check_bitmap(bitmap, want):
    n = len(want["verdict"])
    words = (n + 63) // 64
    assert (_bits(bitmap[:words], n) == want["verdict"]).all()
    assert (_bits(bitmap[:words], 64 * words)[n:] == 0).all()  # the bits past n_pairs
    assert (bitmap[words:] == -1).all()                          # nothing past the last word


@pytest.mark.parametrize("nb", SMALL)
def test_small_batches_host_and_device(sv, dev, small_sets, kpath, nb):
    s, want = small_sets[nb]
    if nb > 1:
        assert want["verdict"].any() and not want["verdict"].all()
    pp.check(sv.verify_txbodies_hinted(*pp.args(s), device=0), want)
    got, bitmap, n = _device_call(sv, dev, s, len(want["pair_sig"]) + 3)
    assert n == len(want["pair_sig"])
    pp.check(got, want)
    _check_bitmap(bitmap, want)


@pytest.fixture(scope="module")
def seam_sets(sv, dev):
    signer = tp.device_signer(sv)
    out = {}
    for nb in SEAMS:
        s = pp.make_sparse(nb, 500 + nb, signer, PAIR_BLOCK)
        out[nb] = (s, pp.expected_fast(s))
    return out


@pytest.mark.parametrize("nb", SEAMS)
def test_scan_seams(sv, dev, seam_sets, nb):
    """One body below, at and above each tile size of the scan; bodies of 0-40
    bytes, about one in 32 with a pair, the first and the last body and the
    first body of every tile among them."""
    s, want = seam_sets[nb]
    pb = want["pair_begin"]
    assert pb[1] == 1 and pb[nb] - pb[nb - 1] == 1 and (np.diff(pb.astype(np.int64))[::PAIR_BLOCK] == 1).all()
    assert 2 <= len(want["pair_sig"]) <= nb // 8 + 4 and want["verdict"].any() and not want["verdict"].all()
    pp.check(sv.verify_txbodies_hinted(*pp.args(s), device=0), want)
    got, bitmap, n = _device_call(sv, dev, s, len(want["pair_sig"]))
    pp.check(got, want)
    _check_bitmap(bitmap, want)


def test_multi_chunk_by_signatures(sv, dev):
    """2^18 + 5000 single-signature bodies of 0-60 bytes, each with its one key:
    more than one staging chunk of signatures; indices and pair_begin global."""
    nb = (1 << 18) + 5000
    s = pp.make_sparse(nb, 7, tp.device_signer(sv), PAIR_BLOCK, max_len=60, one_in=1)
    want = pp.expected_fast(s)
    assert s["ns"] == nb == len(want["pair_sig"]) and int(want["pair_sig"][-1]) == nb - 1
    pp.check(sv.verify_txbodies_hinted(*pp.args(s), device=0), want)
    assert 0 < int(want["verdict"].sum()) < nb


def test_multi_chunk_by_keys(sv, dev):
    """70000 bodies with four candidate keys each: 280000 keys cross the key
    bound of a chunk (2^18) while the signatures stay far below theirs."""
    nb = 70000
    s = pp.make_sparse(nb, 9, tp.device_signer(sv), PAIR_BLOCK, one_in=3, keys_per_body=4)
    want = pp.expected_fast(s)
    assert s["nk"] > (1 << 18) > s["ns"] and int(want["pair_key"].max()) > (1 << 18)
    assert len(want["pair_sig"]) > len(set(want["pair_sig"].tolist()))  # some hints match two keys
    pp.check(sv.verify_txbodies_hinted(*pp.args(s), device=0), want)
    assert 0 < int(want["verdict"].sum()) < len(want["verdict"])


def _boundary_set(sv, oracle):
    """2400 signatures; the body in the middle carries 20 of them, so an equal
    share of signatures ends inside it; bodies without signatures at the start,
    around it and at the end."""
    rng = np.random.default_rng(8)
    counts = [0, 0] + [1] * 1190 + [0, 20, 0] + [1] * 1190 + [0, 0]
    assert sum(counts) == 2400 and sum(counts[:1193]) < 1200 < sum(counts[:1194])
    b = pp._Builder(rng, tp.device_signer(sv))
    P = b.pks
    for t, c in enumerate(counts):
        keys = [P[t % 6], P[(t + 1) % 6]] if t % 4 else [P[t % 6], b.wrong_key(P[t % 6][28:])]
        b.add(int(rng.integers(0, 3)), int(rng.integers(0, 400)), [(t % 6, None)] * c, keys)
    s = b.finish()
    s["sig"][5::11, 7] ^= 2
    return s, pp.expected(s, oracle)


def test_two_slots_on_one_gpu_boundary_at_body_edge(sv, dev, oracle):
    s, want = _boundary_set(sv, oracle)
    assert want["verdict"].any() and not want["verdict"].all()
    one = sv.verify_txbodies_hinted(*pp.args(s), device=0)
    sv.set_device_map([0, 0])
    try:
        sv.set_min_shard(1000)
        assert sv.device_count() == 2
        two = sv.verify_txbodies_hinted(*pp.args(s))
        assert sv.pinned_bytes(0) > 0 and sv.pinned_bytes(1) > 0  # both slots staged a slice
    finally:
        sv.set_min_shard(0)
        sv.set_device_map([])
    pp.check(one, want)
    pp.check(two, want)  # (every digest delivered: the binding's array starts as zeros)
    for a, b in zip(one, two):
        assert (a == b).all()
    assert sv.device_count() >= 1


def test_capacity_error_then_success(sv, dev, small_sets):
    s, want = small_sets[65]
    n = len(want["pair_sig"])
    for cap in (n - 1, 0):
        with pytest.raises(sv.SigVerifyError, match="SV_ERR_PAIR_CAP") as e:
            sv.verify_txbodies_hinted(*pp.args(s), pair_cap=cap, device=0)
        assert e.value.needed == n
        with pytest.raises(sv.SigVerifyError, match="SV_ERR_PAIR_CAP") as e:
            _device_call(sv, dev, s, cap)
        assert e.value.needed == n
    pp.check(sv.verify_txbodies_hinted(*pp.args(s), pair_cap=n, device=0), want)
    got, _, _ = _device_call(sv, dev, s, n)
    pp.check(got, want)


def test_capacity_error_multi_chunk_counts_every_chunk(sv, dev):
    """An overflow in the first chunk: the remaining chunks only count, and the
    count that comes back is that of the whole batch."""
    nb = (1 << 18) + 3000
    s = pp.make_sparse(nb, 11, tp.device_signer(sv), PAIR_BLOCK, max_len=8, one_in=1)
    with pytest.raises(sv.SigVerifyError, match="SV_ERR_PAIR_CAP") as e:
        sv.verify_txbodies_hinted(*pp.args(s), pair_cap=1000, device=0)
    assert e.value.needed == nb


class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    st = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(st))
    return st


def test_mirror_prefetch3(sv, dev):
    """~2000 envelopes (no payload signers): prefetch 3 is ONE engine batch with
    no fallback and gives the results and hashes of prefetch 0 and 1; with the
    engine failing the results are the same through the CPU form."""
    host = ctypes.CDLL(sv.HOSTLIB_PATH)
    host.svh_last_error_string.restype = ctypes.c_char_p
    s = eb.build_set(400, 31, tp.device_signer(sv), with_payload=False)
    assert s["n"] == 2000

    def call(prefetch):
        return eb.check_envelopes_bodies(host, s["envs_blank"], *s["rest"], s["n"], s["naccounts"], 21, s["bodies"],
                                         s["ebody"], prefetch=prefetch)

    ref, _, ch0, fb0 = call(0)
    assert (ref["code"] == s["expect"]).all()
    assert (ch0 == s["contents_hash"]).all() and (fb0 == s["fee_bump_hash"]).all()
    res1, pairs1, ch1, fb1 = call(1)
    assert (res1 == ref).all() and (ch1 == ch0).all() and (fb1 == fb0).all()
    _stats(host)
    res, pairs, ch, fb = call(3)
    st = _stats(host)
    assert st.gpu_batches == 1 and st.fallbacks == 0 and st.gpu_signatures == pairs == pairs1
    assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()
    prev = sv.set_debug_flags(sv.DBG_FAIL)
    try:
        res, _, ch, fb = call(3)
    finally:
        sv.set_debug_flags(prev)
    st = _stats(host)
    assert st.fallbacks >= 1
    assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()
