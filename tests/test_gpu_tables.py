"""What one kernel leaves in device memory for the next, read back and checked
against Python integers (tests/edwards_ref.py).

tests/test_gpu_devcore.py probes single operations and every other GPU test
sees one verdict bit per signature; nothing else reads the state in between:

  a  the base-point tables of sv_launch_btab_init, all 2 x 32 769 entries;
  b  the comb base table of sv_launch_comb_btab, all 32 x 129 entries;
  c  the per-key comb tables of sv_launch_keytab, 64 x 9 entries per key;
  d  the per-signature tables of -A and -R that sv_prep_kernel<M, false, DF>
     and sv_quad_kernel<M> build into the workspace;
  e  sv_prep_kernel's digit record: the scalars it encodes, the flags, the
     window count per wave, with and without the TRIVIAL_PAIR / MAX_WINDOWS /
     PREP_ONLY knobs;
  f  the per-key store of the throughput path (sv_keyslot_kernel,
     sv_keybuild_kernel, sv_prep_kernel<M, true, false>, sv_main_kernel<true>)
     through an sv_ktparams the test owns.

Every buffer is the test's (tests/launchers.py: preset to 0xA5, 4 KiB of guard
behind it, checked after each launch).  Every comparison is exact -- a value
mod p, mod L or mod 8L -- or a limb bound of tests/fe_bounds.py.  The only
rows or keys left out of a content check are those whose point does not
decode; each test counts them with a criterion of its own (Euler's, on the
curve equation) and asserts that exactly those were left out.  The launches'
verdicts are the oracle's.  tests/test_tables_cpu.py runs the same checkers on
the host build.
"""
import numpy as np
import pytest

import edwards_ref as er
import isolating_rows as ir
import launchers as kl
import table_rows as tr
from test_gpu_instantiations import _batches_and_keys, _same, key_status

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FILL32 = 0xA5A5A5A5
SPARE_SLOTS = 16
NS = (1, 63, 64, 65)  # and the whole batch
LT = 4 * kl.SV_ATAB_ENTRIES * kl.SV_LTAB_QUADS  # dwords of one 9-entry table of the one-lane path (360)
QT = kl.SV_ATAB_ENTRIES * kl.SV_QENT             # ... of the quad path (540)


def on_curve(enc):
    """Euler's criterion on x^2 = (y^2 - 1) / (d y^2 + 1): whether the encoding's y (mod p) has a point."""
    y = (int.from_bytes(enc, "little") & ((1 << 255) - 1)) % er.P
    u, v = (y * y - 1) % er.P, (er.D * y * y + 1) % er.P
    w = u * pow(v, er.P - 2, er.P) % er.P
    return w == 0 or pow(w, (er.P - 1) // 2, er.P) == 1


def neg_point(enc):
    """-(the point of an encoding) in extended coordinates, or None"""
    pt = ir.dec_lenient(bytes(enc))
    return None if pt is None else er.ext_neg(er.ext(pt[:2]))


@pytest.fixture(scope="module")
def tk(sv, golden, oracle):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    k = _batches_and_keys(dev, golden, oracle)
    k.L = kl.Launchers(sv.load_library(), dev)
    k.btab = k.L.btab()
    k.oracle = oracle
    k.neg = {}
    # the TOP8 rows (tests/table_rows.py), one batch per mode, each row launched alone
    k.top8 = {}
    for mode, mlens in ((0, (32,)), (1, (32, 33)), (2, (33,))):
        rows = [r for m in mlens for r in tr.top8_rows(oracle, m)]
        pk = np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(-1, 32)
        sig = np.frombuffer(b"".join(r[1] for r in rows), np.uint8).reshape(-1, 64)
        k.top8[mode] = kl.Batch(dev, pk, sig, [r[2] for r in rows], mode, np.ones(len(rows), np.uint8))
    return k


def _neg(k, enc):
    enc = bytes(enc)
    if enc not in k.neg:
        k.neg[enc] = neg_point(enc)
    return k.neg[enc]


# ------------------------------------------------------- a. base-point tables
@pytest.mark.parametrize("t", [0, 1])
def test_btab_every_entry(tk, t):
    """sv_launch_btab_init: entry e of table t is e 2^(128 t) B in affine form
    -- e = 0 (the identity: 1, 1, 0) to 2^15 -- ypx / ymx within RP, xy2d
    within R, the pad dwords 0."""
    tab = tk.btab.cpu().numpy().view(np.uint32).reshape(2, (1 << 15) + 1, 36)
    assert er.check_btab(tab[t], 128 * t, range((1 << 15) + 1)) == 32769


# --------------------------------------------------------- b. comb base table
def test_comb_btab_every_entry(tk):
    """sv_launch_comb_btab: entry (j, e) is e 256^j B in cached form, carried."""
    ctab = tk.L.comb_btab()
    assert er.check_comb_btab(ctab.cpu().numpy().view(np.uint32)) == 32 * 129


# ----------------------------------------------------- c. per-key comb tables
@pytest.fixture(scope="module")
def keytabs(tk):
    k = tk
    valid = tr.seeded_row(k.oracle, 0, 32)[0]
    keys = sorted(set(k.keys) | set(tr.mixed_order_keys(valid)) | {ir.B_ENC, valid})
    assert set(ir.ENCODINGS) <= set(keys)
    nslots = len(keys) + SPARE_SLOTS
    slots = np.random.default_rng(31).permutation(nslots)[:len(keys)].astype(np.uint32)
    ktab, kstat = k.L.keytab(np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32), slots, nslots)
    return keys, slots, nslots, ktab, kstat.cpu().numpy()


KEY_PARTS = 4


@pytest.mark.parametrize("part", range(KEY_PARTS))
def test_keytab_every_entry(tk, keytabs, part):
    """sv_keytab_kernel: for every key that decodes -- valid keys, all 14
    blacklist encodings, y >= p, mixed-order keys A + [k]T8, B -- entry (j, e)
    is e 16^j (-A), carried, entry 0 the cached identity; the status is the
    rule (3)-(5) for every key; slots no key was built into keep the fill."""
    keys, slots, nslots, ktab, kstat = keytabs
    sb = tk.L.lib.sv_key_slot_bytes()
    tab = ktab.view(nslots, sb)
    mine = range(part, len(keys), KEY_PARTS)
    left_out = 0
    for i in mine:
        key, s = keys[i], int(slots[i])
        assert int(kstat[s]) == key_status(key), key.hex()
        nA = neg_point(key)
        if nA is None:
            left_out += 1
            continue
        assert er.check_keytab(tab[s].cpu().numpy().view(np.uint32), nA, key.hex()) == 64 * 9
    assert left_out == sum(1 for i in mine if not on_curve(keys[i]))
    if part == 0:
        assert sum(1 for key in keys if not on_curve(key)) >= 1
        guards = sorted(set(range(nslots)) - set(slots.tolist()))
        assert len(guards) == SPARE_SLOTS and (kstat[guards] == 0x5A5A5A5A).all()
        assert bool((tab[torch.tensor(guards, device=tk.dev)] == kl.FILL).all())


# ----------------------------------- d, e. per-signature tables and the record
def _records(k, b, n, res, dbg, slots=None):
    """The records and window counts of a one-lane launch of the first n rows
    of b, against Python integers -> (flags seen, slot words)."""
    L = k.L
    w = res.ws.words()
    cap, rec0, rdw, wmax0 = L.ws_layout(n)
    assert rdw == er.REC_DWORDS and cap >= n and cap % 64 == 0
    waves = (n + 63) // 64
    wmax = w[wmax0:wmax0 + cap // 64]
    assert (wmax[waves:] == FILL32).all(), "window counts of waves with no signature were written"
    recs = w[rec0:rec0 + cap * rdw].reshape(cap, rdw)
    assert (recs[64 * waves:] == FILL32).all(), "records of waves with no signature were written"
    assert (recs[n:64 * waves] == recs[n - 1]).all(), "an idle lane's record is not the last signature's"
    seen, own = 0, []
    for li in range(n):
        pk, sig, msg = b.h_pk[li].tobytes(), b.h_sig[li].tobytes(), b.h_msgs[li]
        W = int(wmax[li >> 6])
        a, r, flags = er.check_record(recs[li].tolist(), W, pk, sig, msg, kl.REC_FLAGS,
                                      trivial=bool(dbg & kl.SV_DBG_TRIVIAL_PAIR), what=(b.mode, n, li))
        assert bool(flags & kl.SV_REC_OK) == tr.record_ok(pk, sig), ("SV_REC_OK", b.mode, n, li)
        assert flags & ~sum(kl.REC_FLAGS) == 0
        slot = int(recs[li][33])
        assert slot == kl.SV_KT_NONE or (slots is not None and slot == slots[li]), ("slot word", b.mode, n, li, slot)
        seen |= flags
        own.append(er.lat_windows(max(a.bit_length(), abs(r).bit_length())))
    for g in range(waves):
        want = 64 if dbg & kl.SV_DBG_MAX_WINDOWS else max(own[64 * g:64 * g + 64])
        assert int(wmax[g]) == want >= kl.SV_LAT_MIN_WINDOWS, ("W of wave", g, int(wmax[g]), want)
    return seen, recs[:n, 33].copy()


def _one_lane_tables(k, b, n, res, table_a=None):
    """tabA / tabR of every row at ws + li SV_SLOT_QUADS_L: entries 1..8 are
    e (-A), e (-R); entry 0 is not written by device builds (sv_build_ltab);
    table_a[li] False: the row's table_A is the key store's, its slot untouched.
    -> entries checked."""
    w = res.ws.words()
    cap = k.L.ws_layout(n)[0]
    waves = (n + 63) // 64
    tabs = w[:cap * 2 * LT].reshape(cap, 2, LT)
    assert (tabs[64 * waves:] == FILL32).all(), "table slots of waves with no signature were written"
    assert (tabs[:, :, :40] == FILL32).all(), "entry 0 (the shared identity entry's place) was written"
    assert (tabs[n:64 * waves] == tabs[n - 1]).all(), "an idle lane's tables are not the last signature's"
    checked, left_out, undecodable = 0, 0, 0
    for li in range(n):
        for half, enc in enumerate((b.h_pk[li].tobytes(), b.h_sig[li, :32].tobytes())):
            undecodable += 0 if on_curve(enc) else 1
            if half == 0 and table_a is not None and not table_a[li]:
                assert (tabs[li, 0] == FILL32).all(), "table_A slot of a key-store row was written"
                undecodable -= 0 if on_curve(enc) else 1
                continue
            pt = _neg(k, enc)
            if pt is None:
                left_out += 1
                continue
            checked += er.check_ltab(tabs[li, half].tolist(), pt, first=1, what=(b.mode, n, li, "AR"[half]))
    assert left_out == undecodable
    skipped_a = 0 if table_a is None else int(n - np.count_nonzero(table_a[:n]))
    assert checked == 8 * (2 * n - skipped_a - left_out)
    return checked


def _launch_one_lane(k, b, n, dbg, kt=None):
    ws = k.L.workspace(kl.PATH_ONE_LANE, n)
    res = k.L.verify(b, n, kl.PATH_ONE_LANE, k.btab, dbg, ws=ws, kt=kt)
    assert res.ws is ws and res[2] == 0
    return res


@pytest.mark.parametrize("df", [0, kl.SV_KP_IN_PLACE])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_prep_tables_and_records(tk, mode, df):
    """sv_prep_kernel<mode, false, DF> at n = 1, 63, 64, 65 and the whole
    batch: the tables of -A and -R of every row, the record of every row, W
    per wave, untouched slots of waves with no signature; the verdicts of the
    same launches are the oracle's.  Then the TOP8 rows, each alone."""
    k = tk
    b = k.batch[mode]
    entries = records = 0
    for n in NS + (b.n,):
        res = _launch_one_lane(k, b, n, df)
        _same(b, res[0], b.want[:n], ("prep+main", mode, df, n))
        kl.check_bitmap(res[1], b.want[:n])
        entries += _one_lane_tables(k, b, n, res)
        seen, slots = _records(k, b, n, res, df)
        assert (slots == kl.SV_KT_NONE).all()
        records += n
    assert seen & kl.SV_REC_RNEG and seen & kl.SV_REC_OK
    t8 = k.top8[mode]
    flags = 0
    for i in range(t8.n):
        one = t8.window(k.dev, i, 1)
        res = _launch_one_lane(k, one, 1, df)
        assert res[0][0] == 1, "a TOP8 row (a valid signature) was rejected"
        _one_lane_tables(k, one, 1, res)
        f, _ = _records(k, one, 1, res, df)
        assert f & (kl.SV_REC_TOP8A if i % 2 == 0 else kl.SV_REC_TOP8R), ("TOP8 row", i)
        flags |= f
    assert flags & kl.SV_REC_TOP8A and flags & kl.SV_REC_TOP8R
    assert entries > 15 * records and records == 193 + b.n


@pytest.mark.parametrize("knob", ["trivial_pair", "max_windows", "prep_only"])
@pytest.mark.parametrize("df", [0, kl.SV_KP_IN_PLACE])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_prep_records_under_knobs(tk, mode, df, knob):
    """The record with SV_DBG_TRIVIAL_PAIR ((a, r) = (h, 1)), SV_DBG_MAX_WINDOWS
    (W = 64) and SV_DBG_PREP_ONLY (the same records; no verdict byte and no
    bitmap word is written), at n = 65 and the whole batch."""
    k = tk
    b = k.batch[mode]
    dbg = df | {"trivial_pair": kl.SV_DBG_TRIVIAL_PAIR, "max_windows": kl.SV_DBG_MAX_WINDOWS,
                "prep_only": kl.SV_DBG_PREP_ONLY}[knob]
    for n in (65, b.n):
        res = _launch_one_lane(k, b, n, dbg)
        if knob == "prep_only":
            assert (res[0] == 7).all() and (res[1] == -1).all(), "SV_DBG_PREP_ONLY wrote verdicts"
        else:
            _same(b, res[0], b.want[:n], (knob, mode, df, n))
            kl.check_bitmap(res[1], b.want[:n])
        _records(k, b, n, res, dbg)
    t8 = k.top8[mode].window(k.dev, 0, 1)
    res = _launch_one_lane(k, t8, 1, dbg)
    f, _ = _records(k, t8, 1, res, dbg)
    if knob == "max_windows":
        assert not f & (kl.SV_REC_TOP8A | kl.SV_REC_TOP8R)  # (W = 64: no carry out)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_quad_tables(tk, mode):
    """sv_quad_kernel<mode>: entries 0..8 of both lane-split tables of every
    row at ws + i SV_QSLOT_QUADS (sv_qoff), both copies of the (Y+X, Y-X) pair;
    the idle quads of the last workgroup redo the last row into their own
    slots; the verdicts of the same launches are the oracle's."""
    k = tk
    b = k.batch[mode]
    for n in NS + (b.n,):
        ws = k.L.workspace(kl.PATH_QUAD, n)
        res = k.L.verify(b, n, kl.PATH_QUAD, k.btab, ws=ws)
        assert res[2] == 0
        _same(b, res[0], b.want[:n], ("quad", mode, n))
        kl.check_bitmap(res[1], b.want[:n])
        w = ws.words()
        slots = (n + kl.SV_QSIGS - 1) // kl.SV_QSIGS * kl.SV_QSIGS
        assert w.size == slots * 2 * QT and 4 * kl.SV_QSLOT_QUADS == 2 * QT
        tabs = w.reshape(slots, 2, QT)
        assert (tabs[n:] == tabs[n - 1]).all(), "an idle quad's tables are not the last signature's"
        left_out = undecodable = 0
        for i in range(n):
            for half, enc in enumerate((b.h_pk[i].tobytes(), b.h_sig[i, :32].tobytes())):
                undecodable += 0 if on_curve(enc) else 1
                pt = _neg(k, enc)
                if pt is None:
                    left_out += 1
                    continue
                er.check_qtab(tabs[i, half].tolist(), pt, what=(mode, n, i, "AR"[half]))
        assert left_out == undecodable


# ------------------------------------------------------- f. the per-key store
def _kt_batch(k, mode, nkeys=20):
    """Rows of the mode's batch under ~nkeys distinct keys (rejected keys among them), each row four times."""
    b = k.batch[mode]
    order = []
    for p in b.h_pk:
        if p.tobytes() not in order:
            order.append(p.tobytes())
    bad = [key for key in order if key_status(key) == kl.SV_KEY_BAD]
    chosen = set(bad[:6]) | set(order[::max(1, len(order) // (nkeys - 6))][:nkeys - 6])
    sel = np.array([i for i in range(b.n) if b.h_pk[i].tobytes() in chosen] * 4)
    sel = sel[np.random.default_rng(5 + mode).permutation(len(sel))]
    kb = kl.Batch(k.dev, b.h_pk[sel], b.h_sig[sel], [b.h_msgs[i] for i in sel], mode, b.want[sel])
    return kb, sorted({p.tobytes() for p in kb.h_pk})


def _store_view(ks):
    st = ks.store.words().reshape(ks.mask + 1, ks.entry_bytes // 4)
    index = ks.index.t.cpu().numpy().view(np.uint64)
    count = ks.count.full[:8].cpu().numpy().view(np.uint32)
    return st, index, count


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_key_store(tk, mode):
    """sv_keyslot_kernel + sv_keybuild_kernel + sv_prep_kernel<mode, true,
    false> + sv_main_kernel<true> on an sv_ktparams of the test's: every
    distinct key owns one slot with its 32 bytes, its status and entries 1..8
    = e (-A); unclaimed slots keep the fill; the records point at the key's
    slot; a second launch claims nothing and changes no entry; with limit = 4
    at most 4 slots are claimed.  Verdicts are the oracle's every time."""
    k = tk
    kb, keys = _kt_batch(k, mode)
    assert 12 <= len(keys) <= 24 and kb.n > 64 and 0 < kb.want.sum() < kb.n
    ks = k.L.keystore(kb.n, mask=1023)
    assert ks.limit == 1024 and ks.entry_bytes == 16 * (kl.SV_KT_TQUADS + 3)
    res = _launch_one_lane(k, kb, kb.n, 0, kt=ks)
    _same(kb, res[0], kb.want, ("key store", mode))
    kl.check_bitmap(res[1], kb.want)
    st, index, count = _store_view(ks)
    assert int(count[1]) == len(keys) == int(count[0])
    claimed = np.nonzero(index)[0]
    assert len(claimed) == len(keys)
    tq = 4 * kl.SV_KT_TQUADS
    slot_of, left_out = {}, 0
    for s in claimed:
        key = st[s, tq:tq + 8].tobytes()
        assert key in keys and key not in slot_of, "a slot's key bytes"
        slot_of[key] = int(s)
        assert st[s, tq + 8:tq + 12].tolist() == [1 if key_status(key) == kl.SV_KEY_OK else 0, 0, 0, 0], key.hex()
        assert (st[s, :40] == FILL32).all()  # (entry 0: device builds do not write it)
        pt = _neg(k, key)
        if pt is None:
            left_out += 1
            continue
        er.check_ltab(st[s, :tq].tolist(), pt, first=1, what=("key store", key.hex()))
    assert left_out == sum(1 for key in keys if not on_curve(key))
    free = np.ones(ks.mask + 1, bool)
    free[claimed] = False
    assert (st[free] == FILL32).all(), "an unclaimed slot was written"
    builders = ks.builders.words()
    assert sorted(builders[:len(keys)].tolist()) == sorted(slot_of.values()) and (builders[len(keys):] == FILL32).all()
    want_slot = [slot_of[p.tobytes()] for p in kb.h_pk]
    assert ks.kslot.words()[:kb.n].tolist() == want_slot
    _, rec_slots = _records(k, kb, kb.n, res, 0, slots=want_slot)
    uses = rec_slots != kl.SV_KT_NONE
    assert uses.any(), "no wave read its table_A from the key store"
    _one_lane_tables(k, kb, kb.n, res, table_a=~uses)
    # a second launch on the same arrays: nothing claimed, nothing rebuilt
    before = st.copy()
    res = _launch_one_lane(k, kb, kb.n, 0, kt=ks)
    _same(kb, res[0], kb.want, ("key store, second launch", mode))
    st2, index2, count2 = _store_view(ks)
    assert int(count2[1]) == len(keys) and int(count2[0]) == 0
    assert (index2 == index).all() and (st2 == before).all()
    # fresh arrays, limit = 4
    ks4 = k.L.keystore(kb.n, mask=1023, limit=4)
    res = _launch_one_lane(k, kb, kb.n, 0, kt=ks4)
    _same(kb, res[0], kb.want, ("key store, limit 4", mode))
    st4, index4, count4 = _store_view(ks4)
    assert int(count4[1]) == len(np.nonzero(index4)[0]) <= 4, "more claims than the limit"
    tq4 = 4 * kl.SV_KT_TQUADS
    slot4 = {st4[s, tq4:tq4 + 8].tobytes(): int(s) for s in np.nonzero(index4)[0]}
    assert set(slot4) <= set(keys) and len(slot4) == int(count4[1])
    want4 = [slot4.get(p.tobytes(), kl.SV_KT_NONE) for p in kb.h_pk]
    # (a lane that met the limit before its key's claim landed has no slot: SV_KT_NONE or the key's slot)
    assert all(g in (w, kl.SV_KT_NONE) for g, w in zip(ks4.kslot.words()[:kb.n].tolist(), want4))
    _records(k, kb, kb.n, res, 0, slots=want4)
