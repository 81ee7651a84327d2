"""sv_set_verdict_cache_share without needing a GPU: the symbol, the constants,
the validation of the bits and the layout of the four shared_* fields of
sv_verdict_cache_stats behind the older struct, in the header and the binding.
The stats call itself names a slot: on a host without a GPU it answers
SV_ERR_NO_DEVICE, as every slot call does there, and this file then asserts only
that and that nothing was written; where a GPU is present the same test checks
the four keys, all zero, and that a caller passing the old, smaller struct_size
gets nothing written past it."""
import ctypes
import os
import re

import pytest

import vcache_feed_model as fm

NEW = ("shared_out", "shared_in", "shared_skipped", "shared_pinned_bytes")


def _gpus(sv):
    try:
        return sv.device_count()
    except sv.SigVerifyError:
        return 0


@pytest.fixture(autouse=True)
def _off_afterwards(sv):
    yield
    sv.set_verdict_cache_share(0)
    sv.set_verdict_cache_feed(0)
    sv.set_verdict_cache(0)


def test_symbol_and_constants_are_exported(sv):
    lib = sv.load_library()
    assert "sv_set_verdict_cache_share" in sv.EXPORTED_SYMBOLS
    assert lib.sv_set_verdict_cache_share is not None
    assert sv.VC_SHARE_FEED == 1 and sv.VC_SHARE_STORES == 2
    repo = os.path.dirname(os.path.dirname(os.path.abspath(sv.__file__)))
    with open(os.path.join(repo, "include", "stellar_sigverify.h")) as f:
        header = f.read()
    assert "#define SV_VC_SHARE_FEED 1u" in header and "#define SV_VC_SHARE_STORES 2u" in header
    assert "int sv_set_verdict_cache_share(uint32_t what);" in header
    # the C struct ends with the four fields, in the order of the binding's VerdictCacheShareStats
    body = re.search(r"typedef struct sv_verdict_cache_stats \{(.*?)\} sv_verdict_cache_stats;", header, re.S).group(1)
    last = re.findall(r"uint64_t ([\w, ]+);", body)[-1]
    assert tuple(x.strip() for x in last.split(",")) == NEW


def test_unknown_bits_are_refused_and_valid_ones_need_no_gpu(sv):
    lib = sv.load_library()
    for bad in (4, 8, 0x80000001, 0xFFFFFFFF, 7):
        assert lib.sv_set_verdict_cache_share(bad) == -1  # SV_ERR_INVALID_ARG
    with pytest.raises(sv.SigVerifyError):
        sv.set_verdict_cache_share(4)
    with pytest.raises(ValueError):
        sv.set_verdict_cache_share(-1)
    with pytest.raises(ValueError):
        sv.set_verdict_cache_share(1 << 32)
    sv.set_verdict_cache(0)
    for what in (0, 1, 2, 3):  # the cache off: remembered, SV_OK, nothing else
        assert lib.sv_set_verdict_cache_share(what) == 0
    sv.set_verdict_cache(64)
    sv.set_verdict_cache_feed(sv.VC_FEED_LANE)
    for what in (3, 2, 1, 0):  # ... and with it on, still without a device
        sv.set_verdict_cache_share(what)
    sv.verdict_cache_clear()


def test_stats_carry_the_new_fields_behind_struct_size(sv):
    old, new = sv.VerdictCacheStats, sv.VerdictCacheShareStats
    assert [f for f, _ in old._fields_[-5:]] == list(fm.FED)  # (the layout of old callers is untouched)
    assert ctypes.sizeof(new) == ctypes.sizeof(old) + 32
    assert tuple(f for f, _ in new._fields_) == NEW and sv.SHARED == NEW
    lib = sv.load_library()

    class Guarded(ctypes.Structure):
        _fields_ = [("st", new), ("guard", ctypes.c_uint8 * 64)]

    for size in (ctypes.sizeof(old), ctypes.sizeof(new), ctypes.sizeof(old) + 8):
        g = Guarded()
        ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
        g.st.struct_size = size
        rc = lib.sv_verdict_cache_get_stats(0, ctypes.cast(ctypes.byref(g), ctypes.POINTER(old)))
        raw = bytes(g)
        if _gpus(sv) == 0:
            assert rc != 0  # SV_ERR_NO_DEVICE, as every slot call answers there ...
            assert raw[8:] == b"\xA5" * (len(raw) - 8)  # ... and nothing was written
            continue
        assert rc == 0
        written = ctypes.sizeof(new) if size >= ctypes.sizeof(new) else ctypes.sizeof(old)
        assert raw[written:] == b"\xA5" * (len(raw) - written), "written past the caller's struct_size"
        assert g.st.fed_rows == 0  # (the old fields are written for either caller)
        if size >= ctypes.sizeof(new):
            assert [getattr(g.st, f) for f in NEW] == [0, 0, 0, 0]
    if _gpus(sv) > 0:
        st = sv.verdict_cache_stats(0)
        assert all(st[f] == 0 for f in NEW)
    else:
        with pytest.raises(sv.SigVerifyError) as e:
            sv.verdict_cache_stats(0)
        assert "SV_ERR_NO_DEVICE" in str(e.value)
