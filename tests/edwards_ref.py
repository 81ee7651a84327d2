"""The plain Edwards reference of the GPU and CPU table tests: Python integers
only, never a path of the engine.

  * the affine law (aff_add, aff_mul, aff_from_y, BASE, T8) and the limb
    helpers tests/test_gpu_devcore.py compares single operations with;
  * the same law in extended coordinates (ext_add, multiples), so that a whole
    table's reference costs additions and no inversion: a table entry is
    compared with its reference point cross-multiplied;
  * the checkers of what the kernels leave in memory for one another -- the
    affine base-point entries (verify_core.h sv_btab_entry_shift), the cached
    entries of the comb tables (comb.h) and of the per-signature / per-key
    tables (sv_build_ltab, sv_qbuild), and the digit record of sv_prep_kernel
    (check_record) -- over raw dwords read back from a buffer.

Every comparison is an exact integer comparison mod p, mod L or mod 8L; every
limb bound is a row of tests/fe_bounds.py.  A reference point is (x, y) or
projective (X, Y, Z[, T]).
"""
import hashlib

import fe_bounds as fb
from fe_bounds import OFF, P, value

L = 2**252 + 27742317777372353535851937790883648493
N8 = 8 * L
D = -121665 * pow(121666, P - 2, P) % P
SQRTM1 = pow(2, (P - 1) // 4, P)


def limbs(v):
    """canonical-width limbs of v < 2^255"""
    return [(v >> OFF[i]) & ((1 << fb.WIDTH[i]) - 1) for i in range(10)]


# ------------------------------------------------------------ the affine law
def aff_add(p, q):
    """Edwards addition law on affine points (a = -1), plain."""
    (x1, y1), (x2, y2) = p, q
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def aff_neg(p):
    return (-p[0] % P, p[1])


def aff_mul(k, p):
    q = (0, 1)
    while k:
        if k & 1:
            q = aff_add(q, p)
        p = aff_add(p, p)
        k >>= 1
    return q


def aff_from_y(y, sign):
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    if (v * x * x - u) % P:
        if (v * x * x + u) % P:
            return None
        x = x * SQRTM1 % P
    if x & 1 != sign:
        x = -x % P
    return (x, y)


def aff_enc(p):
    return p[1] | ((p[0] & 1) << 255)


BASE = aff_from_y(4 * pow(5, P - 2, P) % P, 0)
# one of the order-8 encodings on libsodium's small-order list
T8 = aff_from_y(int.from_bytes(bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05"), "little"), 0)


def coords(row):
    return [value(row[10 * k:10 * k + 10]) % P for k in range(len(row) // 10)]


def assert_projective(row, pt, wantT=True, what=""):
    X, Y, Z, T = coords(row)
    assert Z != 0, (what, "Z = 0")
    zi = pow(Z, P - 2, P)
    assert (X * zi % P, Y * zi % P) == pt, (what, "not the reference point")
    if wantT:
        assert T * Z % P == X * Y % P, (what, "T Z != X Y")


# ------------------------------------------- the law in extended coordinates
IDENT = (0, 1, 1, 0)


def ext(pt):
    """(x, y) or (X, Y, Z[, T]) -> (X, Y, Z, T)"""
    if len(pt) == 2:
        return (pt[0], pt[1], 1, pt[0] * pt[1] % P)
    if len(pt) == 3:
        zi = pow(pt[2], P - 2, P)
        x, y = pt[0] * zi % P, pt[1] * zi % P
        return (x, y, 1, x * y % P)
    return tuple(pt)


def ext_add(p, q):
    """The unified addition law (a = -1, complete: any two points of the curve), no inversion."""
    X1, Y1, Z1, T1 = p
    X2, Y2, Z2, T2 = q
    A, B = (Y1 - X1) * (Y2 - X2) % P, (Y1 + X1) * (Y2 + X2) % P
    C, Dd = 2 * D * T1 * T2 % P, 2 * Z1 * Z2 % P
    E, F, G, H = B - A, Dd - C, Dd + C, B + A
    return (E * F % P, G * H % P, F * G % P, E * H % P)


def ext_neg(p):
    return (-p[0] % P, p[1], p[2], -p[3] % P)


def ext_eq(p, q):
    return (p[0] * q[2] - q[0] * p[2]) % P == 0 and (p[1] * q[2] - q[1] * p[2]) % P == 0


def ext_pow2(p, k):
    """[2^k] p"""
    for _ in range(k):
        p = ext_add(p, p)
    return p


def multiples(p, n):
    """[IDENT, p, 2p, .. n p], by running addition"""
    p = ext(p)
    out, acc = [IDENT], IDENT
    for _ in range(n):
        acc = ext_add(acc, p)
        out.append(acc)
    return out


# ------------------------------------------------------- the table checkers
def within(limbs_, bound):
    return all(int(x) <= b for x, b in zip(limbs_, bound))


def check_affine_entry(dw36, pt, what=""):
    """One base-point table entry ypx[12] ymx[12] xy2d[12] (verify_core.h
    sv_btab_entry_shift) against its reference point: the values are y + x,
    y - x, 2d x y; ypx / ymx are fe_weak outputs (RP), xy2d a product (R);
    dwords 10, 11 of each field are 0."""
    X, Y, Z, _ = ext(pt) if len(pt) != 4 else pt
    dw = [int(v) for v in dw36]
    assert len(dw) == 36, (what, "entry size")
    ypx, ymx, xy2d = dw[0:10], dw[12:22], dw[24:34]
    assert dw[10:12] == [0, 0] and dw[22:24] == [0, 0] and dw[34:36] == [0, 0], (what, "pad dwords not 0")
    assert within(ypx, fb.RP), (what, "ypx above RP", ypx)
    assert within(ymx, fb.RP), (what, "ymx above RP", ymx)
    assert fb.is_R(xy2d), (what, "xy2d above R", xy2d)
    assert (value(ypx) * Z - (Y + X)) % P == 0, (what, "y + x")
    assert (value(ymx) * Z - (Y - X)) % P == 0, (what, "y - x")
    assert (value(xy2d) * Z * Z - 2 * D * X * Y) % P == 0, (what, "2d x y")


COMB_BOUNDS = (fb.RP, fb.RP, fb.RP, fb.RP)               # comb.h: every coordinate carried (R+)
LTAB_BOUNDS = (fb.PT_YPX, fb.PT_YMX, fb.RP, fb.R)        # ge_p3_to_cached of an RP point: within fb.ENT
assert all(within(b, fb.ENT) for b in LTAB_BOUNDS)


def check_cached_entry(ypx, ymx, z, t2d, pt, bounds, what=""):
    """One cached entry (Y+X, Y-X, Z, 2dT), ten limbs each, against its
    reference point: with X = (ypx - ymx) / 2, Y = (ypx + ymx) / 2: Z != 0,
    X = x Z, Y = y Z, t2d Z = 2d X Y (mod p), and every field's limbs within
    the bound of its position in `bounds`."""
    fields = [[int(v) for v in f] for f in (ypx, ymx, z, t2d)]
    for name, f, b in zip(("ypx", "ymx", "z", "t2d"), fields, bounds):
        assert len(f) == 10 and within(f, b), (what, name, "limbs above the bound", f)
    X0, Y0, Z0, _ = ext(pt) if len(pt) != 4 else pt
    vp, vm, Z, T2d = (value(f) % P for f in fields)
    assert Z != 0, (what, "Z = 0")
    X2, Y2 = (vp - vm) % P, (vp + vm) % P            # 2X, 2Y
    assert (X2 * Z0 - 2 * X0 * Z) % P == 0, (what, "X != x Z")
    assert (Y2 * Z0 - 2 * Y0 * Z) % P == 0, (what, "Y != y Z")
    assert (2 * T2d * Z - D * X2 * Y2) % P == 0, (what, "2dT Z != 2d X Y")


def check_btab(tab, shift, entries, what="btab"):
    """Entries `entries` of one base-point table (rows of 36 dwords, row e =
    e 2^shift B); -> how many were checked."""
    ref = multiples(ext_pow2(ext(BASE), shift), max(entries))
    rows = tab.tolist() if hasattr(tab, "tolist") else tab
    for e in entries:
        check_affine_entry(rows[e], ref[e], (what, shift, e))
    return len(entries)


def check_comb_btab(tab, positions=None, what="ctab"):
    """The comb base table (comb.h): 32 x 129 entries of 48 dwords, entry
    (j, e) = e 256^j B, every coordinate RP and padded with two zero dwords."""
    rows = tab.reshape(32, 129, 48).tolist()
    g, n = ext(BASE), 0
    for j in range(32):
        if positions is None or j in positions:
            ref = multiples(g, 128)
            for e in range(129):
                check_comb_entry(rows[j][e], ref[e], (what, j, e))
                n += 1
        g = ext_pow2(g, 8)
    return n


def check_comb_entry(dw48, pt, what=""):
    dw = [int(v) for v in dw48]
    assert all(dw[12 * k + 10:12 * k + 12] == [0, 0] for k in range(4)), (what, "pad dwords not 0")
    check_cached_entry(dw[0:10], dw[12:22], dw[24:34], dw[36:46], pt, COMB_BOUNDS, what)


def check_keytab(slot_dw, negA, what="ktab"):
    """One key's comb tables (comb.h): 64 x 9 entries e 16^j (-A); entry 0 is
    the cached identity (1, 1, 1, 0) in canonical limbs."""
    rows = slot_dw.reshape(64, 9, 48).tolist()
    g, n = ext(negA), 0
    one = [1] + [0] * 11
    for j in range(64):
        ref = multiples(g, 8)
        assert rows[j][0] == one + one + one + [0] * 12, (what, j, "entry 0 is not the cached identity")
        for e in range(9):
            check_comb_entry(rows[j][e], ref[e], (what, j, e))
            n += 1
        g = ext_pow2(g, 4)
    return n


def check_ltab(tab_dw, pt, first=1, what="ltab"):
    """Entries first..8 of a 9 x 40-dword table of sv_build_ltab (YpX, YmX, Z,
    T2d back to back): entry e = e pt."""
    rows = [int(v) for v in tab_dw]
    assert len(rows) == 360
    ref = multiples(pt, 8)
    for e in range(first, 9):
        w = rows[40 * e:40 * e + 40]
        check_cached_entry(w[0:10], w[10:20], w[20:30], w[30:40], ref[e], LTAB_BOUNDS, (what, e))
    return 9 - first


def check_qtab(tab_dw, pt, what="qtab"):
    """Entries 0..8 of a lane-split table of sv_quad_kernel (sv_qstore: 60
    dwords per entry: lane 0's (Y+X, Y-X), lane 1's (Y-X, Y+X), lane 2's Z,
    lane 3's 2dT): both copies of the pair are checked, and each is the other
    swapped."""
    rows = [int(v) for v in tab_dw]
    assert len(rows) == 540
    ref = multiples(pt, 8)
    for e in range(9):
        w = rows[60 * e:60 * e + 60]
        assert w[0:10] == w[30:40] and w[10:20] == w[20:30], (what, e, "the two copies of (Y+X, Y-X) differ")
        check_cached_entry(w[0:10], w[10:20], w[40:50], w[50:60], ref[e], LTAB_BOUNDS, (what, e, "lane 0"))
        check_cached_entry(w[30:40], w[20:30], w[40:50], w[50:60], ref[e], LTAB_BOUNDS, (what, e, "lane 1"))
    return 9


# ------------------------------------------------------------- the record
REC_DWORDS = 36          # dA[8] dR[8] dB0[8] dB1[8] flags slot 0 0 (sv_kernels.hip sv_prep_kernel)
LAT_MIN_WINDOWS = 33     # lattice.h SV_LAT_MIN_WINDOWS (checked against the header by the tests)


def hram(pk, sig, msg):
    return int.from_bytes(hashlib.sha512(bytes(sig[:32]) + bytes(pk) + bytes(msg)).digest(), "little") % L


def lat_windows(bits):
    """lattice.h sv_lat_windows"""
    return max(LAT_MIN_WINDOWS, (bits + 1 + 3) // 4)


def _s4(x):
    return x - 16 if x & 8 else x


def _s32(x):
    return x - (1 << 32) if x & (1 << 31) else x


def record_scalars(rec, W, flags_bits):
    """(a, r, b, base digits) of one record at window count W.  Window w's
    digit is nibble w + 64 - W of the string (signed, 4 bits); the top window
    is +8 (not its nibble) when the TOP8 flag is set; r takes RNEG's sign."""
    RNEG, TOP8A, TOP8R, _ = flags_bits
    rec = [int(v) for v in rec]
    assert len(rec) == REC_DWORDS
    flags = rec[32]

    def scalar(words, top8):
        v = 0
        for w in range(W):
            p = w + 64 - W
            d = _s4((words[p >> 3] >> (4 * (p & 7))) & 15)
            if w == W - 1 and top8:
                d = 8
            v += d << (4 * w)
        # nibbles below window 0 are what the shift by 63 - W brought in: zeros
        for p in range(64 - W):
            assert (words[p >> 3] >> (4 * (p & 7))) & 15 == 0, "digits below window 0"
        return v

    a = scalar(rec[0:8], bool(flags & TOP8A))
    r = scalar(rec[8:16], bool(flags & TOP8R))
    if flags & RNEG:
        r = -r
    digits = [_s32(v) for v in rec[16:32]]
    lo, hi = (sum(d << (16 * j) for j, d in enumerate(half)) for half in (digits[:8], digits[8:]))
    b = lo + (hi << 128)
    return a, r, b, digits


def check_record(rec, W, pk, sig, msg, flags_bits, trivial=False, what=""):
    """The invariants of one digit record against Python integers (lattice.h:
    c0 = c1 h mod 8L, c0 >= 0, c1 odd; sv_lat_prepare: s = c1 S mod L with c1's
    sign, recoded in signed radix 2^16).  -> (a, r, flags)."""
    a, r, b, digits = record_scalars(rec, W, flags_bits)
    h = hram(pk, sig, msg)
    S = int.from_bytes(bytes(sig[32:]), "little")
    assert a >= 0, (what, "a < 0")
    assert r & 1, (what, "r even")
    assert (a - r * h) % N8 == 0, (what, "a != r h mod 8L", W, hex(a), hex(r))
    assert 0 <= b < L, (what, "b outside [0, L)")
    assert (b - r * S) % L == 0, (what, "b != r S mod L")
    assert all(-2**15 <= d < 2**15 for d in digits), (what, "base digit outside [-2^15, 2^15)", digits)
    assert a < 1 << (4 * W) and abs(r) < 1 << (4 * W), (what, "scalar needs more than W windows")
    assert W >= lat_windows(max(a.bit_length(), abs(r).bit_length(), 1)), (what, "W below the lane's own count", W)
    if trivial:
        assert (a, r) == (h, 1), (what, "not the trivial pair")
    assert int(rec[34]) == 0 and int(rec[35]) == 0, (what, "record tail not 0")
    return a, r, int(rec[32])
