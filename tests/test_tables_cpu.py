"""CPU twins of tests/test_gpu_tables.py: the table builders and the digit
recoding of csrc/verify_core.h, compiled for the host
(tests/native/host_core.cpp), under the checkers of tests/edwards_ref.py.

  hc_btab_entry_shift   sv_btab_entry_shift, any e, shift 0 and 128 (the CPU
                        path's own base-point tables are built by it)
  hc_comb_btab          the comb base table of sv_comb_bentry
  hc_build_ltab         sv_build_ltab of a decoded key
  hc_lat_record         sv_lat_pre + sv_lat_prepare: digits, flags, tables

This proves the checkers without a GPU: a build with the base-point shift off
by one, an entry stored one carry short, sv_build_ltab storing one entry off,
or the top-digit carry dropped fails here (DESIGN.md section 2.3 names the
tests).  Every comparison is exact; the limb bounds are tests/fe_bounds.py's.
"""
import ctypes
import random

import numpy as np
import pytest

import edwards_ref as er
import isolating_rows as ir
import kernel_defs as kd
import table_rows as tr


@pytest.mark.parametrize("shift", [0, 128])
def test_btab_entry_shift_twin(hostcore, shift):
    """e < 64, every 2^k and 2^k +- 1, 2^15, and 500 seeded positions: the entry is e 2^shift B."""
    top = 1 << 15
    es = set(range(64)) | {top}
    for k in range(16):
        es |= {e for e in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= e <= top}
    es |= set(random.Random("btab twin %d" % shift).sample(range(top + 1), 500))
    es = sorted(es)
    tab = {}
    hostcore.hc_btab_entry_shift.restype = None
    for e in es:
        out = np.zeros(36, np.uint32)
        hostcore.hc_btab_entry_shift(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(e), ctypes.c_int(shift))
        tab[e] = out.tolist()
    assert er.check_btab(tab, shift, es) == len(es) >= 564
    assert 0 in es and top in es  # (e = 0: the identity, y + x = y - x = 1, 2d x y = 0, by the checker)


def test_comb_btab_twin(hostcore):
    """All 32 x 129 entries of the comb base table: e 256^j B, every coordinate carried."""
    tab = np.zeros(32 * 129 * 48, np.uint32)
    hostcore.hc_comb_btab.restype = None
    hostcore.hc_comb_btab(tab.ctypes.data_as(ctypes.c_void_p))
    assert er.check_comb_btab(tab) == 32 * 129


def _ltab(hostcore, enc, negate=1):
    out = np.zeros(9 * 40, np.uint32)
    ok = hostcore.hc_build_ltab(out.ctypes.data_as(ctypes.c_void_p), bytes(enc), ctypes.c_int(negate))
    return ok, out


def _neg(pt):
    return er.ext_neg(er.ext(pt[:3] if len(pt) == 4 else pt))


def test_build_ltab_twin(hostcore, oracle):
    """sv_build_ltab of -A for valid keys, B, mixed-order keys A + [k]T8, every
    blacklist encoding and y >= p: entry e is e (-A), entry 0 the identity;
    the keys left out are exactly the off-curve one built in."""
    valid = [tr.seeded_row(oracle, s, 32)[0] for s in range(6)]
    keys = valid + [ir.B_ENC] + tr.mixed_order_keys(valid[0]) + list(ir.ENCODINGS)
    keys += [(y | (s << 255)).to_bytes(32, "little") for y in (ir.P + 2, ir.P + 10, (1 << 255) - 1) for s in (0, 1)]
    y = 2
    while ir.dec_lenient(y.to_bytes(32, "little")) is not None:
        y += 1
    keys.append(y.to_bytes(32, "little"))
    skipped = 0
    for key in keys:
        pt = ir.dec_lenient(key)
        ok, tab = _ltab(hostcore, key)
        assert bool(ok) == (pt is not None), key.hex()
        if pt is None:
            skipped += 1
            continue
        assert er.check_ltab(tab, _neg(pt), first=0, what=key.hex()) == 9
        assert tab[:40].tolist() == ([1] + [0] * 9) * 3 + [0] * 10
    # y >= p encodings decode iff y - p is on the curve: count what the loop left out by construction
    assert skipped == sum(1 for k in keys if ir.dec_lenient(k) is None) >= 1
    assert skipped == 1 + sum(1 for k in keys[:-1] if ir.dec_lenient(k) is None)


def _record_rows(oracle):
    rows = []
    for mlen in (32, 33):
        d = ir.generate(mlen)
        rows += [(d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][mlen * i:mlen * i + mlen].tobytes())
                 for i in range(len(d["cls"]))]
        rows += tr.top8_rows(oracle, mlen)
    return rows


def _full_record(rec, info):
    flags = sum(bit for bit, name in zip(kd.REC_FLAGS, ("rneg", "top8A", "top8R", "ok")) if info[name])
    return rec.tolist() + [flags, kd.SV_KT_NONE, 0, 0]


def test_lat_record_twin(hostcore, oracle):
    """sv_lat_pre + sv_lat_prepare on every isolating row and the TOP8 rows:
    the record's scalars satisfy a = r h (mod 8L), b = r S (mod L) at the
    lane's own window count, at one more, and at 64; OK is (1)-(5) and R's
    decode; the tables of -A and -R are multiples of the decoded points."""
    assert er.LAT_MIN_WINDOWS == kd.SV_LAT_MIN_WINDOWS
    rows = _record_rows(oracle)
    seen = {"top8A": 0, "top8R": 0, "rneg": 0, "reject": 0}
    tabs_skipped = 0
    for k, (pk, sig, msg) in enumerate(rows):
        rec, info, tabs = tr.lat_record(hostcore, pk, sig, msg, tabs=True)
        W = info["W"]
        a, r, flags = er.check_record(_full_record(rec, info), W, pk, sig, msg, kd.REC_FLAGS, what=("row", k))
        assert W == info["w_lane"] == er.lat_windows(max(a.bit_length(), abs(r).bit_length()))
        assert bool(info["ok"]) == tr.record_ok(pk, sig), ("OK", k)
        for name in ("top8A", "top8R", "rneg"):
            seen[name] += info[name]
        seen["reject"] += 1 - info["ok"]
        for W2 in sorted({min(W + 1, 64), min(W + 7, 64), 64}):
            rec2, info2, _ = tr.lat_record(hostcore, pk, sig, msg, W=W2)
            a2, r2, _ = er.check_record(_full_record(rec2, info2), W2, pk, sig, msg, kd.REC_FLAGS, what=("row", k, W2))
            assert (a2, r2) == (a, r) and not info2["top8A"] and not info2["top8R"]
        rec3, info3, _ = tr.lat_record(hostcore, pk, sig, msg, trivial=True)
        er.check_record(_full_record(rec3, info3), info3["W"], pk, sig, msg, kd.REC_FLAGS, trivial=True,
                        what=("row", k, "trivial"))
        if k % 4 == 0:  # the tables (every fourth row: the arithmetic is test_build_ltab_twin's)
            for half, enc in enumerate((pk, sig[:32])):
                pt = ir.dec_lenient(enc)
                if pt is None:
                    tabs_skipped += 1
                    continue
                er.check_ltab(tabs[360 * half:360 * half + 360], _neg(pt), first=0, what=("row", k, "AR"[half]))
    assert seen["top8A"] >= 1 and seen["top8R"] >= 1 and seen["rneg"] >= 1 and seen["reject"] >= 1
    assert tabs_skipped == sum(1 for k, (pk, sig, _) in enumerate(rows) if k % 4 == 0
                               for enc in (pk, sig[:32]) if ir.dec_lenient(enc) is None)


def test_top8_seeds_raise_their_flags(hostcore, oracle):
    """The committed seeds (tests/table_rows.py): each row is a valid signature
    and raises its flags at its own window count (a launch of n = 1); each is
    the first such seed of its neighbourhood by find_top8."""
    for (mlen, flag), seed in sorted(tr.TOP8_SEEDS.items()):
        pk, sig, msg = tr.seeded_row(oracle, seed, mlen)
        assert oracle.oracle_ed25519_verify(sig, msg, len(msg), pk) == 0
        info = tr.lat_record(hostcore, pk, sig, msg)[1]
        assert (info["top8A"], info["top8R"]) == ((1, 0) if flag == "top8A" else (1, 1)), (mlen, flag)
        assert info["W"] < 64
        assert tr.find_top8(hostcore, oracle, mlen, (info["top8A"], info["top8R"]), start=seed - 50, limit=51) == seed
