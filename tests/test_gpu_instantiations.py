"""Every instantiation of the verify kernels, chosen by the test.

Which template instantiation a public call runs depends on the device's CU
count and on n (sv_comb_spw, the octet kernel's message windows, the hint
bits of the lane), so a suite that only goes through the public entry points
reaches a device-dependent subset.  Here the kernel launchers of
csrc/launch.h are called directly (tests/launchers.py: checked ctypes
wrappers), with the mode, signatures per wave, path and hint bits picked by
the test at tiny n:

  sv_comb_kernel<MODE, SPW>        MODE 0..2 x SPW 1, 2, 4, n around the
                                   workgroup size NS = 3 SPW, tables built by
                                   sv_launch_keytab into scattered slots;
  sv_keytab_kernel                 the slot status by the rule (3)-(5);
  sv_octet_kernel<MODE, MSG, HI>   MODE x both sides of the MSG switch
                                   (8 CUs signatures and one more) x no hint,
                                   SV_KP_OCT_HI, SV_KP_OCT_HI | _WIDE;
  sv_quad_kernel<MODE, MSG>        MODE 0..2;
  sv_prep_kernel<MODE, false, DF>  MODE x {0, SV_KP_IN_PLACE}, sv_main_kernel<false>
  (the KT forms need the engine's tables: tests/test_gpu_isolating.py
   test_key_tables_decide_A).

The batch: the isolating rows (tests/isolating_rows.py), a slice of the
adversarial and lattice_edge fixtures, and message lengths around the SHA-512
block and LDS-window edges; expected verdicts are the oracle's.  DESIGN.md
section 2.2 maps every instantiation to the test that reaches it.
"""
import numpy as np
import pytest

import isolating_rows as ir
import launchers as kl

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MSGLENS = [0, 1, 47, 48, 63, 64, 65, 111, 112] + list(range(496, 513))
SPARE_SLOTS = 16


def _rows_of(d, sel):
    out = []
    for i in sel:
        o, ln = int(d["msg_off"][i]), int(d["msg_len"][i])
        out.append((d["pk"][i].tobytes(), d["sig"][i].tobytes(), d["msg"][o:o + ln].tobytes()))
    return out


def _one_per_pair(d):
    """One row per (encoding, role), two per S class, eight controls."""
    sel, seen = [], {}
    for i in range(len(d["cls"])):
        key = (int(d["cls"][i]), int(d["enc"][i]))
        cap = 1 if key[0] < 2 else (2 if key[0] < 4 else 4)
        if seen.get(key, 0) < cap:
            seen[key] = seen.get(key, 0) + 1
            sel.append(i)
    return sel


def key_status(pk):
    """SV_KEY_OK iff A is canonical, not small-order and decodable ((3)-(5))."""
    y = int.from_bytes(pk, "little") & ((1 << 255) - 1)
    return kl.SV_KEY_OK if y < ir.P and not ir.is_blacklisted(pk) and ir.dec_lenient(pk) is not None else kl.SV_KEY_BAD


class Kit:
    pass


@pytest.fixture(scope="module")
def kit(sv, golden, oracle):
    if sv.device_count() < 1:
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    k = _batches_and_keys(dev, golden, oracle)
    k.L = kl.Launchers(sv.load_library(), dev)
    k.btab = k.L.btab()
    k.ctab = k.L.comb_btab()
    k.ktab, k.kstat = k.L.keytab(np.frombuffer(b"".join(k.keys), np.uint8).reshape(-1, 32), k.slots, k.nslots)
    k.tiled = {}
    return k


def _batches_and_keys(dev, golden, oracle):
    k = Kit()
    k.dev = dev
    a32, a33 = ir.generate(32), ir.generate(33)
    adv, edge, ml = golden["adversarial"], golden["lattice_edge"], golden["msglen"]
    fix = _rows_of(adv, range(0, len(adv["verdict"]), 215)) + _rows_of(edge, range(0, len(edge["verdict"]), 15))
    mls = []
    for j, ln in enumerate(MSGLENS):
        cand = np.nonzero(ml["msg_len"] == ln)[0]
        assert len(cand) >= 1
        mls += _rows_of(ml, [cand[j % len(cand)]])  # (valid and flipped rows alternate)
    rows = {0: _rows_of(a32, range(len(a32["cls"]))) + fix,
            1: _rows_of(a32, _one_per_pair(a32)) + _rows_of(a33, _one_per_pair(a33)) + fix + mls,
            2: _rows_of(a33, range(len(a33["cls"])))}
    rng = np.random.default_rng(20)
    k.batch = {}
    for mode, r in rows.items():
        r = [r[i] for i in rng.permutation(len(r))]  # iso_* rows, controls and fixture rows mixed
        want = np.array([1 if oracle.oracle_ed25519_verify(s, m, len(m), p) == 0 else 0 for p, s, m in r], np.uint8)
        assert 0 < want.sum() < len(r)
        pk = np.frombuffer(b"".join(p for p, _, _ in r), np.uint8).reshape(-1, 32)
        sig = np.frombuffer(b"".join(s for _, s, _ in r), np.uint8).reshape(-1, 64)
        k.batch[mode] = kl.Batch(dev, pk, sig, [m for _, _, m in r], mode, want)
    assert 100 <= k.batch[1].n <= 170 and {len(m) for m in k.batch[1].h_msgs} >= set(MSGLENS)
    # the keys: every key of the batches, every blacklist encoding, y >= p beyond the blacklist, an off-curve y
    keys = {p.tobytes() for b in k.batch.values() for p in b.h_pk} | set(ir.ENCODINGS)
    for y in (ir.P + 2, ir.P + 10, (1 << 255) - 1):
        keys |= {(y | (s << 255)).to_bytes(32, "little") for s in (0, 1)}
    y = 2
    while ir.dec_lenient(y.to_bytes(32, "little")) is not None:
        y += 1
    keys.add(y.to_bytes(32, "little"))
    k.keys = sorted(keys)
    k.nslots = len(k.keys) + SPARE_SLOTS
    k.slots = rng.permutation(k.nslots)[:len(k.keys)].astype(np.uint32)
    k.slot_of = {key: int(s) for key, s in zip(k.keys, k.slots)}
    return k


def _kslot(k, b):
    return np.array([k.slot_of[p.tobytes()] for p in b.h_pk], np.uint32)


def _same(b, got, want, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, [(int(i), b.h_pk[i].tobytes().hex()[:16], int(want[i])) for i in bad[:10]])


def test_keytab_status_and_guard_slots(kit):
    """sv_keytab_kernel: the status of every key by the rule (3)-(5) -- all 14
    blacklist encodings, y >= p, an off-curve y are SV_KEY_BAD, every other key
    SV_KEY_OK -- and the slots no key was built into keep the guard pattern."""
    k = kit
    kstat = k.kstat.cpu().numpy()
    want = {s: key_status(key) for key, s in k.slot_of.items()}
    bad = [(key.hex(), int(kstat[s]), want[s]) for key, s in k.slot_of.items() if int(kstat[s]) != want[s]]
    assert not bad, bad[:5]
    assert sum(1 for v in want.values() if v == kl.SV_KEY_BAD) >= 14 + 6 + 1
    assert all(want[k.slot_of[e]] == kl.SV_KEY_BAD for e in ir.ENCODINGS)
    guards = sorted(set(range(k.nslots)) - set(k.slot_of.values()))
    assert len(guards) == SPARE_SLOTS
    assert (kstat[guards] == 0x5A5A5A5A).all()
    sb = k.L.lib.sv_key_slot_bytes()
    tab = k.ktab.view(k.nslots, sb)
    assert bool((tab[torch.tensor(guards, device=k.dev)] == 0xA5).all())
    used = tab[torch.tensor(sorted(k.slot_of.values()), device=k.dev)]
    assert bool((used != 0xA5).any(dim=1).all())  # (and every key's slot was written)


@pytest.mark.parametrize("spw", [1, 2, 4])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_comb_instantiations(kit, mode, spw):
    """sv_comb_kernel<mode, spw>: the whole batch (many workgroups, a ragged
    last one), then n = 1, NS - 1, NS, NS + 1, 2 NS + 1 on windows of it."""
    k = kit
    b = k.batch[mode]
    got = k.L.comb(b, b.n, spw, _kslot(k, b), k.ktab, k.kstat, k.ctab)
    _same(b, got, b.want, ("comb", mode, spw, b.n))
    ns = kl.SV_COMB_CHAIN_WAVES * spw
    for j, n in enumerate((1, ns - 1, ns, ns + 1, 2 * ns + 1)):
        w = b.window(k.dev, (29 * j + 7 * spw + 3 * mode) % (b.n - n), n)
        got = k.L.comb(w, n, spw, _kslot(k, w), k.ktab, k.kstat, k.ctab)
        _same(w, got, w.want, ("comb", mode, spw, n))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_comb_status_conjunct_alone(kit, mode):
    """The same signatures with the status of half of the accepting keys forced
    to SV_KEY_BAD: every signature under those keys rejects (its equation still
    holds, R and S are fine), every other verdict stays."""
    k = kit
    b = k.batch[mode]
    spw = (1, 2, 4)[mode]
    kslot = _kslot(k, b)
    acc = sorted({int(kslot[i]) for i in np.nonzero(b.want == 1)[0]})
    forced = acc[::2]
    assert forced and len(forced) < len(acc)
    kstat = k.kstat.clone()
    assert bool((kstat[torch.tensor(forced, device=k.dev)] == kl.SV_KEY_OK).all())
    kstat[torch.tensor(forced, device=k.dev)] = kl.SV_KEY_BAD
    want = b.want.copy()
    want[np.isin(kslot, forced)] = 0
    assert 0 < want.sum() < b.want.sum()
    got = k.L.comb(b, b.n, spw, kslot, k.ktab, kstat, k.ctab)
    _same(b, got, want, ("forced bad", mode))


def _tiled(k, mode, n):
    if (mode, n) not in k.tiled:
        k.tiled[(mode, n)] = k.batch[mode].tiled(k.dev, n)
    return k.tiled[(mode, n)]


@pytest.mark.parametrize("hint", ["two_wave", "hi", "hi_wide"])
@pytest.mark.parametrize("side", ["msg_windows", "msg_from_memory"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_octet_instantiations(kit, mode, side, hint):
    """sv_octet_kernel<mode, MSG, HI>: 8 signatures per workgroup, so 8 CUs of
    them are one workgroup per CU (MSG: the messages go through LDS windows)
    and one more signature is past the switch; the larger batch repeats the
    small one.  MODE 0 has no window on either side.  The launch's failure
    word stays 0."""
    k = kit
    n = kl.SV_OSIGS * k.L.cus + (0 if side == "msg_windows" else 1)
    b = _tiled(k, mode, kl.SV_OSIGS * k.L.cus + 1)
    dbg = {"two_wave": 0, "hi": kl.SV_KP_OCT_HI, "hi_wide": kl.SV_KP_OCT_HI | kl.SV_KP_OCT_HI_WIDE}[hint]
    got, bm, status = k.L.verify(b, n, kl.PATH_OCTET, k.btab, dbg)
    assert status == 0
    _same(b, got, b.want[:n], ("octet", mode, side, hint))
    kl.check_bitmap(bm, b.want[:n])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_quad_instantiations(kit, mode):
    """sv_quad_kernel<0, false>, <1, true>, <2, true>."""
    k = kit
    b = k.batch[mode]
    got, bm, status = k.L.verify(b, b.n, kl.PATH_QUAD, k.btab)
    assert status == 0
    _same(b, got, b.want, ("quad", mode))
    kl.check_bitmap(bm, b.want)


@pytest.mark.parametrize("df", [0, kl.SV_KP_IN_PLACE])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_prep_main_instantiations(kit, mode, df):
    """sv_prep_kernel<mode, false, DF> + sv_main_kernel<false>: the measured
    order and the decode-first order (SV_KP_IN_PLACE; the kernel only reorders
    its loads, so device memory serves as well as mapped host memory)."""
    k = kit
    b = k.batch[mode]
    got, bm, status = k.L.verify(b, b.n, kl.PATH_ONE_LANE, k.btab, df)
    assert status == 0
    _same(b, got, b.want, ("prep+main", mode, df))
    kl.check_bitmap(bm, b.want)
