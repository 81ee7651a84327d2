"""Signatures straight from transaction bodies on the GPU: sv_txhash_kernel and
the verify launch behind sv_ed25519_verify_txbodies / _device, the chunking
(by signatures, by body bytes), the slicing over two slots and the host
mirror's catchup form.  Expected digests are hashlib's, expected verdicts the
oracle's (by construction for the large GPU-signed sets)."""
import ctypes

import numpy as np
import pytest

import envelope_bodies as eb
import envelopes as ev
import txbodies_pool as tp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = (1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def dev(sv):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def small_sets(sv, dev, oracle):
    """One pool set per size, GPU-signed, oracle-judged; shared and left unchanged."""
    signer = tp.device_signer(sv)
    return {nb: tp.make_set(nb, 100 + nb, signer, oracle) for nb in SMALL}


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


def _device_call(sv, dev, s):
    """sv_ed25519_verify_txbodies_device over the set as it is packed (bodies
    back to back: every alignment) -> (verdict, bitmap words, digests)."""
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731
    n, nb = s["n"], s["nb"]
    t_bodies, t_off, t_len, t_kind = up(s["bodies"]), up(s["off"]), up(s["len"]), up(s["kind"])
    t_sb, t_pk, t_sig = up(s["sig_begin"]), up(s["pk"]), up(s["sig"])
    t_v = torch.full((max(n, 1),), 7, dtype=torch.uint8, device=dev)
    t_bm = torch.full(((n + 63) // 64 + 1,), -1, dtype=torch.int64, device=dev)
    t_dig = torch.zeros((nb, 32), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    sv.verify_txbodies_device(0, tp.NETWORK_ID, t_bodies.data_ptr(), t_off.data_ptr(), t_len.data_ptr(),
                              t_kind.data_ptr(), nb, t_sb.data_ptr(), t_pk.data_ptr(), t_sig.data_ptr(), n,
                              t_v.data_ptr(), t_bm.data_ptr(), t_dig.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    return t_v.cpu().numpy()[:n], t_bm.cpu().numpy(), t_dig.cpu().numpy()


@pytest.mark.parametrize("nb", SMALL)
def test_small_batches_host_and_device(sv, dev, small_sets, kpath, nb):
    s = small_sets[nb]
    assert s["verdict"].any() and not s["verdict"].all()
    verdict, digests = sv.verify_txbodies(*tp.args(s), device=0)
    assert (digests == s["digests"]).all()
    assert (verdict == s["verdict"]).all()
    verdict, bitmap, digests = _device_call(sv, dev, s)
    assert (digests == s["digests"]).all()
    assert (verdict == s["verdict"]).all()
    n = s["n"]
    words = (n + 63) // 64
    assert (_bits(bitmap[:words], n) == s["verdict"]).all()
    assert (_bits(bitmap[:words], 64 * words)[n:] == 0).all()  # the bits past n
    assert bitmap[words] == -1                                   # nothing past the last word


def test_digests_only(sv, dev, small_sets):
    """n == 0 with n_bodies > 0: only digests, on both entries."""
    s = dict(small_sets[65])
    s.update(n=0, sig_begin=np.zeros(s["nb"] + 1, np.uint64), pk=np.zeros((0, 32), np.uint8),
             sig=np.zeros((0, 64), np.uint8))
    verdict, digests = sv.verify_txbodies(*tp.args(s), device=0)
    assert verdict.size == 0 and (digests == s["digests"]).all()
    _, _, digests = _device_call(sv, dev, s)
    assert (digests == s["digests"]).all()


def test_multi_chunk_by_signatures(sv, dev):
    """2^18 + 5000 single-signature bodies of 100-300 bytes: more than one
    staging chunk of signatures."""
    nb = (1 << 18) + 5000
    rng = np.random.default_rng(5)
    s = tp.make_custom(rng.integers(0, 3, nb), rng.integers(100, 301, nb), np.ones(nb, np.uint64), rng,
                       tp.device_signer(sv))
    verdict, digests = sv.verify_txbodies(*tp.args(s), device=0)
    assert (digests == s["digests"]).all()
    assert (verdict == s["built"]).all()
    assert 0 < int(verdict.sum()) < s["n"]


def test_multi_chunk_by_bytes(sv, dev, oracle):
    """40 bodies of 2 MiB with small bodies between them: more body bytes than
    one chunk holds (64 MiB)."""
    rng = np.random.default_rng(6)
    length, counts = [], []
    for i in range(40):
        length += [2 << 20, int(rng.integers(0, 200)), int(rng.integers(100, 4097))]
        counts += [1, 20 if i % 8 == 0 else 1, 0 if i % 5 == 0 else 1]
    s = tp.make_custom(rng.integers(0, 3, len(length)), length, counts, rng, tp.device_signer(sv), oracle)
    assert int(s["len"].sum(dtype=np.uint64)) > (64 << 20)
    verdict, digests = sv.verify_txbodies(*tp.args(s), device=0)
    assert (digests == s["digests"]).all()
    assert (verdict == s["verdict"]).all() and (s["verdict"] == s["built"]).all()


def test_two_slots_on_one_gpu_straddling_body(sv, dev, oracle):
    """Signatures sliced over two slots on GPU 0; a 20-signature body straddles
    the boundary (hashed on both slots, its digest delivered once), bodies
    without signatures sit at the start, at the boundary and at the end."""
    rng = np.random.default_rng(8)
    counts = [0, 0] + [1] * 1190 + [0, 20, 0] + [1] * 1190 + [0, 0]
    nb = len(counts)
    assert sum(counts) == 2400 and sum(counts[:1193]) < 1200 < sum(counts[:1194])
    s = tp.make_custom(rng.integers(0, 3, nb), rng.integers(0, 400, nb), counts, rng, tp.device_signer(sv), oracle)
    sv.set_device_map([0, 0])
    try:
        sv.set_min_shard(1000)
        assert sv.device_count() == 2
        verdict, digests = sv.verify_txbodies(*tp.args(s))
        assert sv.pinned_bytes(0) > 0 and sv.pinned_bytes(1) > 0  # both slots staged a slice
    finally:
        sv.set_min_shard(0)
        sv.set_device_map([])
    assert (digests == s["digests"]).all()
    assert (verdict == s["verdict"]).all()
    assert sv.device_count() >= 1


class EngineStats(ctypes.Structure):
    _fields_ = [("gpu_signatures", ctypes.c_uint64), ("gpu_batches", ctypes.c_uint64),
                ("cpu_signatures", ctypes.c_uint64), ("fallbacks", ctypes.c_uint64)]


def _stats(host):
    s = EngineStats()
    host.svh_engine_counts_ex(ctypes.byref(s))
    return s


def test_mirror_catchup_form(sv, dev):
    """~2000 envelopes (no payload signers): prefetch=1 is ONE engine batch with
    no fallback and gives the prefetch=0 results; with the engine failing the
    results are the same through the CPU path."""
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
    hashed, _ = ev.check_envelopes(host, s["envs"], *s["rest"], s["n"], s["naccounts"], 21)
    assert (hashed == ref).all()
    _stats(host)
    res, pairs, ch, fb = call(1)
    st = _stats(host)
    assert st.gpu_batches == 1 and st.fallbacks == 0 and st.gpu_signatures == pairs
    assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()
    prev = sv.set_debug_flags(sv.DBG_FAIL)
    try:
        res, _, ch, fb = call(1)
    finally:
        sv.set_debug_flags(prev)
    st = _stats(host)
    assert st.fallbacks >= 1
    assert (res == ref).all() and (ch == ch0).all() and (fb == fb0).all()
