"""CPU checks of the device arithmetic (host g++ build of stellar-core_amd/csrc/*.h).

The GPU kernels are compiled from the same headers; these tests pin the
limb-bound reasoning of fe25519.h/ge25519.h (worst-case limbs at the documented
bounds), the mod-L Barrett reduction, SHA-512 of R||A||M (1 and multi-block)
and the complete per-lane verifier against the golden fixtures, all against
Python big-integer arithmetic, hashlib and libsodium's verdicts.
"""
import ctypes
import hashlib
import random

import numpy as np

from conftest import REPO  # noqa: F401

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
W = [26, 25] * 5


def _val(limbs):
    return sum(x << o for x, o in zip(limbs, OFF))


def _words(o):
    return sum(o[i] << (32 * i) for i in range(8))


def test_fe_mul_random(hostcore):
    rnd = random.Random(1)
    out = ctypes.create_string_buffer(32)
    for _ in range(500):
        a, b = rnd.randrange(2**255), rnd.randrange(2**255)
        hostcore.hc_fe_mul(out, a.to_bytes(32, "little"), b.to_bytes(32, "little"))
        assert int.from_bytes(out.raw, "little") == a * b % P


def test_fe_limb_bounds_worst_case(hostcore):
    """mul/sq accept M3 inputs; mul2/sq2 accept R+ inputs (fe25519.h header)."""
    rnd = random.Random(2)
    o = (ctypes.c_uint32 * 8)()
    for trial in range(600):
        if trial < 20:
            la = [3 * (1 << w) - 1 for w in W]
            lb = [3 * (1 << w) - 1 for w in W]
        else:
            la = [rnd.randrange(3 * (1 << w)) for w in W]
            lb = [rnd.randrange(3 * (1 << w)) for w in W]
        A = (ctypes.c_uint32 * 10)(*la)
        B = (ctypes.c_uint32 * 10)(*lb)
        hostcore.hc_fe_mul_limbs(o, A, B, 0)
        assert _words(o) == _val(la) * _val(lb) % P
        hostcore.hc_fe_sq_limbs(o, A, 0)
        assert _words(o) == _val(la) ** 2 % P
        r1 = [(1 << w) + 1216 if trial < 20 else rnd.randrange((1 << w) + 1217) for w in W]
        r2 = [(1 << w) + 1216 if trial < 20 else rnd.randrange((1 << w) + 1217) for w in W]
        A1 = (ctypes.c_uint32 * 10)(*r1)
        B1 = (ctypes.c_uint32 * 10)(*r2)
        hostcore.hc_fe_mul_limbs(o, A1, B1, 1)
        assert _words(o) == 2 * _val(r1) * _val(r2) % P
        hostcore.hc_fe_sq_limbs(o, A1, 1)
        assert _words(o) == 2 * _val(r1) ** 2 % P
        big = [rnd.randrange(1 << 31) for _ in W]
        hostcore.hc_fe_tobytes_limbs(o, (ctypes.c_uint32 * 10)(*big))
        assert _words(o) == _val(big) % P


def test_fe_mul_m5_f_operand(hostcore):
    """ge_dbl leaves r.X at M5 (= AA + 4p - (YY+XX)); it is only ever the f
    operand of fe_mul (g, the operand pre-multiplied by 19, stays <= M3)."""
    rnd = random.Random(7)
    o = (ctypes.c_uint32 * 8)()
    for trial in range(400):
        if trial < 10:
            lf = [5 * (1 << w) - 1 for w in W]
            lg = [3 * (1 << w) - 1 for w in W]
        else:
            lf = [rnd.randrange(5 * (1 << w)) for w in W]
            lg = [rnd.randrange(3 * (1 << w)) for w in W]
        hostcore.hc_fe_mul_limbs(o, (ctypes.c_uint32 * 10)(*lf), (ctypes.c_uint32 * 10)(*lg), 0)
        assert _words(o) == _val(lf) * _val(lg) % P


def test_fe_mul_partial_carry_g_operand(hostcore):
    """ge_dbl leaves T at M5 and carries only its even limbs 2..8
    (fe_weak_even): T is then the g operand of the conversion products X*T
    (X at M5) and Z*T, with g limb 0 up to M5 and odd limbs up to 5 2^25 + 5."""
    rnd = random.Random(11)
    o = (ctypes.c_uint32 * 8)()
    gmax = [5 * (1 << 26) - 1] + [(1 << 26) - 1 if j % 2 == 0 else 5 * (1 << 25) + 5 for j in range(1, 10)]
    for trial in range(400):
        if trial < 10:
            lf, lg = [5 * (1 << w) - 1 for w in W], list(gmax)
        else:
            lf = [rnd.randrange(5 * (1 << w)) for w in W]
            lg = [rnd.randrange(m + 1) for m in gmax]
        hostcore.hc_fe_mul_limbs(o, (ctypes.c_uint32 * 10)(*lf), (ctypes.c_uint32 * 10)(*lg), 0)
        assert _words(o) == _val(lf) * _val(lg) % P


def test_fe_tobytes_edge_values(hostcore):
    o = (ctypes.c_uint32 * 8)()
    for v in [0, 1, P - 1, P, P + 1, P + 18, 2**255 - 1, 2 * P - 1]:
        limbs = [(v >> off) & ((1 << w) - 1) for off, w in zip(OFF, W)]
        limbs[9] = v >> 230  # may exceed 25 bits for v >= 2^255
        hostcore.hc_fe_tobytes_limbs(o, (ctypes.c_uint32 * 10)(*limbs))
        assert _words(o) == v % P, hex(v)


def test_fe_invert(hostcore):
    rnd = random.Random(3)
    out = ctypes.create_string_buffer(32)
    for _ in range(40):
        a = rnd.randrange(1, P)
        hostcore.hc_fe_invert(out, a.to_bytes(32, "little"))
        assert int.from_bytes(out.raw, "little") * a % P == 1


def test_sc_reduce512(hostcore):
    rnd = random.Random(4)
    out = ctypes.create_string_buffer(32)
    vals = [0, 1, L - 1, L, L + 1, 2 * L, 2**512 - 1, (2**512 - 1) // L * L, (2**512 - 1) // L * L - 1]
    vals += [rnd.randrange(2**512) for _ in range(500)]
    for x in vals:
        hostcore.hc_sc_reduce512(out, x.to_bytes(64, "little"))
        assert int.from_bytes(out.raw, "little") == x % L


def test_sha512_ram_paths(hostcore):
    rnd = np.random.default_rng(5)
    out = ctypes.create_string_buffer(64)
    for n in list(range(0, 140)) + [239, 240, 241, 367, 368, 369, 1000]:
        R, A = rnd.bytes(32), rnd.bytes(32)
        m = rnd.bytes(n)
        hostcore.hc_sha512_ram(out, R, A, m, n, 0)
        assert out.raw == hashlib.sha512(R + A + m).digest(), n
    # message at every alignment inside a larger buffer (the device reads
    # aligned dwords and funnel-shifts them)
    for n in (0, 1, 7, 8, 9, 47, 48, 49, 63, 64, 65, 200):
        for off in range(4):
            R, A = rnd.bytes(32), rnd.bytes(32)
            buf = ctypes.create_string_buffer(rnd.bytes(off + n + 8), off + n + 8)
            hostcore.hc_sha512_ram(out, R, A, ctypes.byref(buf, off), n, 0)
            assert out.raw == hashlib.sha512(R + A + buf.raw[off:off + n]).digest(), (n, off)
    R, A, m = rnd.bytes(32), rnd.bytes(32), rnd.bytes(32)
    hostcore.hc_sha512_ram(out, R, A, m, 32, 1)
    assert out.raw == hashlib.sha512(R + A + m).digest()


def test_decompress_roundtrip(hostcore, golden):
    out = ctypes.create_string_buffer(32)
    pks = golden["valid"]["pk"][:64]
    for pk in pks:
        assert hostcore.hc_decompress(out, pk.tobytes(), 0) == 1
        assert out.raw == pk.tobytes()
        assert hostcore.hc_decompress(out, pk.tobytes(), 1) == 1
        neg = bytearray(pk.tobytes())
        neg[31] ^= 0x80
        assert out.raw == bytes(neg)


def _host_verify(hostcore, d, rows):
    pk = np.ascontiguousarray(d["pk"][rows])
    sig = np.ascontiguousarray(d["sig"][rows])
    msg = np.ascontiguousarray(d["msg"])
    off = np.ascontiguousarray(d["msg_off"][rows])
    ln = np.ascontiguousarray(d["msg_len"][rows])
    out = np.zeros(len(rows), np.uint8)
    hostcore.hc_verify_batch(ctypes.c_void_p(pk.ctypes.data), ctypes.c_void_p(sig.ctypes.data),
                             ctypes.c_void_p(msg.ctypes.data), ctypes.c_void_p(off.ctypes.data),
                             ctypes.c_void_p(ln.ctypes.data), ctypes.c_size_t(len(rows)),
                             ctypes.c_void_p(out.ctypes.data))
    return out


def test_grouped_batch_inversion_matches_golden(hostcore, golden):
    """The kernel's K-signature batch inversion (with rejected rows parked at
    Z = 1) must give the same verdicts: adversarial rows interleave accepts and
    rejects inside every group."""
    for name in ("adversarial", "intree"):
        d = golden[name]
        rows = np.arange(len(d["verdict"]))[::4] if name == "adversarial" else np.arange(len(d["verdict"]))
        pk = np.ascontiguousarray(d["pk"][rows])
        sig = np.ascontiguousarray(d["sig"][rows])
        off = np.ascontiguousarray(d["msg_off"][rows])
        ln = np.ascontiguousarray(d["msg_len"][rows])
        msg = np.ascontiguousarray(d["msg"])
        out = np.zeros(len(rows), np.uint8)
        hostcore.hc_verify_batch_grouped(ctypes.c_void_p(pk.ctypes.data), ctypes.c_void_p(sig.ctypes.data),
                                         ctypes.c_void_p(msg.ctypes.data), ctypes.c_void_p(off.ctypes.data),
                                         ctypes.c_void_p(ln.ctypes.data), ctypes.c_size_t(len(rows)),
                                         ctypes.c_void_p(out.ctypes.data))
        assert np.array_equal(out, d["verdict"][rows]), name


def test_lane_verifier_matches_golden(hostcore, golden):
    for name, d in golden.items():
        rows = np.arange(len(d["verdict"]))
        if name in ("adversarial", "valid"):
            rows = rows[::3]  # keep the CPU suite short; every class is still covered
        got = _host_verify(hostcore, d, rows)
        bad = np.nonzero(got != d["verdict"][rows])[0]
        assert len(bad) == 0, (name, [str(d["class_names"][d["cls"][rows[i]]]) for i in bad[:10]])


def _hash_inputs(rnd, n):
    """Bytes at a random misalignment inside a larger buffer (the device code
    reads aligned dwords around them)."""
    pad = rnd.integers(0, 4)
    buf = bytes(rnd.integers(0, 256, int(pad) + n + 8, dtype=np.uint8))
    return buf, int(pad)


def test_device_blake2b_cache_key(hostcore):
    """hash_dev.h sv_cache_key == BLAKE2b-256(pk || sig || msg) (RFC 7693,
    hashlib), the verify-cache key of SecretKey.cpp:50-61."""
    rnd = np.random.default_rng(11)
    out = ctypes.create_string_buffer(32)
    for n in list(range(0, 70)) + [127, 128, 129, 159, 160, 161, 255, 256, 257, 300, 1000]:
        pk, sig = rnd.bytes(32), rnd.bytes(64)
        buf, pad = _hash_inputs(rnd, n)
        base = ctypes.create_string_buffer(buf, len(buf))
        hostcore.hc_cache_key(out, pk, sig, ctypes.byref(base, pad), ctypes.c_uint32(n))
        assert out.raw == hashlib.blake2b(pk + sig + buf[pad:pad + n], digest_size=32).digest(), n


def test_device_sha256(hostcore):
    """hash_dev.h sv_sha256 == SHA-256 (FIPS 180-4, hashlib) at every padding
    boundary; the tx contents hash of TransactionFrame.cpp:90-117."""
    rnd = np.random.default_rng(12)
    out = ctypes.create_string_buffer(32)
    for n in list(range(0, 140)) + [183, 184, 191, 192, 247, 248, 1000, 4097]:
        buf, pad = _hash_inputs(rnd, n)
        base = ctypes.create_string_buffer(buf, len(buf))
        hostcore.hc_sha256(out, ctypes.byref(base, pad), ctypes.c_uint32(n))
        assert out.raw == hashlib.sha256(buf[pad:pad + n]).digest(), n
    hostcore.hc_sha256(out, b"abc", 3)  # FIPS 180-2 appendix B.1
    assert out.raw.hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"


# ------------------------------------------------ half-size path (lattice.h)
N8 = 8 * L


def test_lattice_reduce_invariants(hostcore):
    """c0 == c1 h (mod 8L), c1 odd, reported bit length exact, short for random h;
    degenerate h fall back to the trivial pair (h, 1)."""
    c0 = ctypes.create_string_buffer(32)
    c1 = ctypes.create_string_buffer(32)
    neg = ctypes.c_int()
    rnd = random.Random(17)
    hs = [0, 1, 2, 7, 8, L - 1, L - 8, 2**128 - 1, 2**128, 2**128 + 1, 2**252, (L - 1) // 8] + \
        [rnd.randrange(L) for _ in range(4000)]
    long_pairs = 0
    for h in hs:
        nb = hostcore.hc_lattice_reduce(h.to_bytes(32, "little"), c0, c1, ctypes.byref(neg))
        a = int.from_bytes(c0.raw, "little")
        b = int.from_bytes(c1.raw, "little")
        b = -b if neg.value else b
        assert (a - b * h) % N8 == 0 and b % 2 == 1 and a >= 0, h
        assert nb == max(a.bit_length(), abs(b).bit_length(), 1), h
        long_pairs += nb > 135
    assert long_pairs <= 12  # only the hand-picked degenerate h need long pairs


def test_lattice_reduce_near_exact_quotients(hostcore):
    """h = ceil(8L / q) + d makes the first quotient 8L / h = q - (tiny), which
    a double rounds UP to q: the exact Euclid step is right only because it
    under-estimates its quotient (the 1 - 2^-40 factor).  For odd q the pair
    is known in closed form, (c0, c1) = (q h - 8L, +q)."""
    from test_gpu_devcore import near_exact_h
    c0 = ctypes.create_string_buffer(32)
    c1 = ctypes.create_string_buffer(32)
    neg = ctypes.c_int()
    for q, h in near_exact_h():
        nb = hostcore.hc_lattice_reduce(h.to_bytes(32, "little"), c0, c1, ctypes.byref(neg))
        a = int.from_bytes(c0.raw, "little")
        b = int.from_bytes(c1.raw, "little")
        sb = -b if neg.value else b
        assert (a - sb * h) % N8 == 0 and b % 2 == 1, (q, h)
        assert nb == max(a.bit_length(), b.bit_length(), 1), (q, h)
        if q & 1:
            assert (a, sb) == (q * h - N8, q), (q, h)


def test_lattice_reduce_pinned_outputs(hostcore):
    """The exact (c0, c1, sign, bit length) of every h in a fixed 20,012-value
    set, as a digest recorded from the round-3/4 implementation: a rewrite of
    the reduction for speed must keep the pairs (and hence every window count
    and digit string the kernels see) unchanged."""
    import hashlib
    c0 = ctypes.create_string_buffer(32)
    c1 = ctypes.create_string_buffer(32)
    neg = ctypes.c_int()
    hs = [0, 1, 2, 7, 8, L - 1, L - 8, 2**128 - 1, 2**128, 2**128 + 1, 2**252, (L - 1) // 8]
    hs += [int.from_bytes(hashlib.sha512(b"lattice-pin" + i.to_bytes(4, "little")).digest(), "little") % L
           for i in range(20000)]
    d = hashlib.sha256()
    for h in hs:
        nb = hostcore.hc_lattice_reduce(h.to_bytes(32, "little"), c0, c1, ctypes.byref(neg))
        d.update(c0.raw + c1.raw + bytes([neg.value & 0xff]) + nb.to_bytes(2, "little"))
    assert d.hexdigest() == "e5e1de0fd871e51b317663861b61ea13cabd81451a20a44e2eac905303444b54"


def _host_verify_lat(hostcore, d, rows, wmin=0):
    pk = np.ascontiguousarray(d["pk"][rows])
    sig = np.ascontiguousarray(d["sig"][rows])
    msg = np.ascontiguousarray(d["msg"])
    off = np.ascontiguousarray(d["msg_off"][rows])
    ln = np.ascontiguousarray(d["msg_len"][rows])
    out = np.zeros(len(rows), np.uint8)
    wins = np.zeros(len(rows), np.int32)
    hostcore.hc_verify_batch_lat(ctypes.c_void_p(pk.ctypes.data), ctypes.c_void_p(sig.ctypes.data),
                                 ctypes.c_void_p(msg.ctypes.data), ctypes.c_void_p(off.ctypes.data),
                                 ctypes.c_void_p(ln.ctypes.data), ctypes.c_size_t(len(rows)),
                                 ctypes.c_void_p(out.ctypes.data), ctypes.c_int(wmin),
                                 ctypes.c_void_p(wins.ctypes.data))
    return out, wins


def test_lattice_lane_verifier_matches_golden(hostcore, golden):
    """The half-size equation gives libsodium's verdict on every fixture class,
    incl. mixed-order keys, torsion in both A and R, and the digit-carry edge
    (pairs of exactly 4W-1 bits)."""
    for name, d in golden.items():
        rows = np.arange(len(d["verdict"]))
        if name in ("adversarial", "valid"):
            rows = rows[1::3]
        got, wins = _host_verify_lat(hostcore, d, rows)
        bad = np.nonzero(got != d["verdict"][rows])[0]
        assert len(bad) == 0, (name, [str(d["class_names"][d["cls"][rows[i]]]) for i in bad[:10]])
        assert wins.min() >= 33 and wins.max() <= 64
    e = golden["lattice_edge"]
    _, wins = _host_verify_lat(hostcore, e, np.arange(len(e["verdict"])))
    assert (wins >= 34).any()  # the W = 34 class is really exercised


def test_lattice_verdicts_independent_of_window_count(hostcore, golden):
    """A wave runs every lane at the wave's maximum W: extra all-zero top windows
    must not change any verdict (W = 64 is the full-length fallback)."""
    for name in ("lattice_edge", "intree"):
        d = golden[name]
        rows = np.arange(len(d["verdict"]))
        for wmin in (34, 41, 64):
            got, _ = _host_verify_lat(hostcore, d, rows, wmin)
            assert np.array_equal(got, d["verdict"][rows]), (name, wmin)


def test_madcount_constants_match_generated_products():
    """SV_MADS_MUL / SV_MADS_SQ (csrc/fe25519.h, the SV_MADCOUNT measurement
    hook behind roofline.hw_mads_per_verify) equal the v_mad_u64_u32 count of
    each generated product statement (csrc/fe_asm_gen.h)."""
    import os
    import re
    csrc = os.path.join(REPO, "stellar-core_amd", "csrc")
    gen = open(os.path.join(csrc, "fe_asm_gen.h")).read()
    fe = open(os.path.join(csrc, "fe25519.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (SV_MADS_MUL|SV_MADS_SQ) (\d+)", fe)}
    bodies = re.split(r"\nSV_HD void ", gen)[1:]
    counts = {b.split("(")[0]: b.count("v_mad_u64_u32") for b in bodies}
    assert counts, "no generated products found"
    for name, c in counts.items():
        want = const["SV_MADS_SQ"] if name.startswith("fe_sq") else const["SV_MADS_MUL"]
        assert c == want, (name, c, want)


# ------------------------------------- the bounds of the real call sites (tests/fe_bounds.py)
def test_fe_cm_forms_at_call_site_maxima(hostcore):
    """fe_mul_cm / fe_sq_cm (the host build's products, and the device's with
    -DSV_FE_ASM_ON=0) at the limb-wise maximum over each form's call sites:
    the quad doublings' M6 partially carried g operand with an M5 f operand
    for fe_mul, the R+ operands of fe_mul2 / fe_sq2, X + Y for fe_sq."""
    import fe_bounds as fb
    o = (ctypes.c_uint32 * 8)()
    u10 = ctypes.c_uint32 * 10
    for fn, dbl in (("fe_mul", 0), ("fe_mul_g19", 0), ("fe_mul2", 1), ("fe_sq", 0), ("fe_sq2", 1)):
        rnd = random.Random("cm" + fn)
        fbound, gbound = fb.function_max(fn)
        for trial in range(400):
            if trial < 200:
                cut = 0 if trial == 0 else 2**8
                lf = [b - rnd.randint(0, cut) for b in fbound]
                lg = None if gbound is None else [b - rnd.randint(0, cut) for b in gbound]
            else:
                lf = [rnd.randint(0, b) for b in fbound]
                lg = None if gbound is None else [rnd.randint(0, b) for b in gbound]
            if gbound is None:
                hostcore.hc_fe_sq_limbs(o, u10(*lf), dbl)
                assert _words(o) == (1 + dbl) * _val(lf) ** 2 % P, (fn, lf)
            else:
                hostcore.hc_fe_mul_limbs(o, u10(*lf), u10(*lg), dbl)
                assert _words(o) == (1 + dbl) * _val(lf) * _val(lg) % P, (fn, lf, lg)


def test_devcore_exports_every_probe():
    """tests/native/libdevcore.so (the probe kernels of tests/test_gpu_devcore.py,
    built for gfx950) builds here and exports every dc_* entry point the GPU
    tests call: a build break shows up before the GPU run."""
    import os
    import subprocess
    import test_gpu_devcore
    d = os.path.join(REPO, "tests", "native")
    subprocess.run(["make", "-s", "libdevcore.so"], cwd=d, check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(d, "libdevcore.so")], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("dc_")}
    assert exported == {"dc_" + k for k in test_gpu_devcore.PROBES}
