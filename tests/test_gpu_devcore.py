"""The device arithmetic's edge cases, run on the GPU.

tests/native/dev_core.hip wraps the functions of fe25519.h, ge25519.h,
sc25519.h, lattice.h, sha512_dev.h, hash_dev.h and quad.h in probe kernels
compiled by hipcc for gfx950 with the product's flags, so what runs here is
what the kernels run: the generated inline-asm products, sv_twice, the bitop3 /
alignbit builtins, the DPP moves, the device compiler's double arithmetic.
tests/test_host_arith.py and tests/test_fe_asm_sim.py cover the same layer on
the CPU, where none of those exist.

Every comparison is an exact integer comparison.  The reference is Python big
integers, hashlib and the plain affine Edwards law below -- never another path
of the engine -- except that the lattice pairs must ALSO equal the host
build's, so that the digest pinned in test_host_arith.py holds on the device.

Field elements travel as raw limbs, so both the value mod p and the documented
output bound are checked; operand bounds come from tests/fe_bounds.py.

SV_DEVCORE_LIB=<path> loads that library instead of building
tests/native/libdevcore.so (used to show that the tests fail on a deliberately
broken build).
"""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import fe_bounds as fb
from conftest import REPO
from edwards_ref import (BASE, D, L, N8, SQRTM1, T8, aff_add, aff_enc, aff_from_y, aff_mul, aff_neg,  # noqa: F401
                         assert_projective, coords, limbs)
from fe_bounds import OFF, P, value

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5

# probe -> dwords per output row (tests/native/dev_core.hip); the CPU suite
# checks that the library exports every one (tests/test_host_arith.py)
PROBES = {
    "fe_mul": 10, "fe_mul2": 10, "fe_mul_g19": 10, "fe_sq": 10, "fe_sq2": 10, "fe_mul_alias_hf": 10,
    "fe_mul_alias_hg": 10, "fe_sq_alias": 10, "fe_mul_same": 10, "fe_sqn": 70, "fe_invert": 10, "fe_pow22523": 10,
    "fe_sub": 10, "fe_sub4": 10, "fe_neg": 10, "fe_weak": 10, "fe_weak_even": 10, "fe_tobytes": 8, "fe_flags": 1,
    "fe_frombytes": 10, "fe_cmov": 10,
    "sc_reduce512": 8, "sc_is_canonical": 1, "sc_mul_signed": 8, "sc_muladd": 8, "sc_digits": 40, "sc_pop_top": 9,
    "sc_lattice_reduce": 18,
    "ge_dbl": 40, "ge_p1p1_convert": 40, "ge_add_preswapped": 40, "ge_p3_to_cached": 40, "ge_p2_tobytes": 8,
    "ge_frombytes": 41,
    "qd_p1p1_to_p3": 40, "qd_dbl": 40, "qd_add": 40, "qd_chain": 40, "qo_identity": 40, "qo_dbl": 40, "qo_add": 40,
    "qo_chain": 40,
    "sha512_ram_var": 16, "sha512_ram32": 16, "cache_key": 8, "sha256": 8,
}
QUAD_PROBES = {k for k in PROBES if k.startswith(("qd_", "qo_"))}


class Dev:
    """Launches probes: numpy arrays go to the device and are passed as
    pointers, Python ints as ints; returns the output rows as uint32."""

    def __init__(self, lib):
        import torch
        self.torch, self.lib = torch, lib
        self.dev = torch.device("cuda", 0)

    def run(self, name, *args, n):
        torch = self.torch
        width = PROBES[name]
        rows = 4 * n if name in QUAD_PROBES else n
        # two guard rows behind the output: a probe that writes past case n - 1 shows
        out = torch.full(((rows + 2) * width,), GUARD - (1 << 32), dtype=torch.int32, device=self.dev)
        keep, cargs = [out], [ctypes.c_void_p(out.data_ptr())]
        for a in args:
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a)
                t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(self.dev)
                keep.append(t)
                cargs.append(ctypes.c_void_p(t.data_ptr()))
            else:
                cargs.append(ctypes.c_int(int(a)))
        cargs += [ctypes.c_int(n), ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)]
        fn = getattr(self.lib, "dc_" + name)
        fn.restype = ctypes.c_int
        rc = fn(*cargs)
        assert rc == 0, (name, "launch failed", rc)
        torch.cuda.synchronize(self.dev)
        got = out.cpu().numpy().view(np.uint32).reshape(rows + 2, width)
        assert (got[rows:] == GUARD).all(), (name, "wrote past its last case")
        return got[:rows]


@pytest.fixture(scope="module")
def dc():
    path = os.environ.get("SV_DEVCORE_LIB")
    if not path:
        d = os.path.join(REPO, "tests", "native")
        subprocess.run(["make", "-s", "libdevcore.so"], cwd=d, check=True)
        path = os.path.join(d, "libdevcore.so")
    import torch  # noqa: F401  (one HIP runtime per process: before the library)
    return Dev(ctypes.CDLL(path))


# ------------------------------------------------------------------ helpers
def u32(rows, width):
    return np.array(rows, dtype=np.uint64).astype(np.uint32).reshape(len(rows), width)


def fes(rows):
    return u32(rows, 10)


def limbs_wide(v):
    """limbs of v < 2^256: limb 9 takes the excess"""
    return limbs(v & (2**230 - 1))[:9] + [v >> 230]


def words(v, n=8):
    return [(v >> (32 * i)) & 0xffffffff for i in range(n)]


def unwords(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def patterns(rng, bound, k):
    """The limb patterns of one operand: every limb at its bound, the bound
    minus randint(0, 2^8), uniform below the bound, all-zero, single limbs."""
    out = [list(bound), [0] * 10]
    out += [[b - rng.randint(0, min(b, 2**8)) for b in bound] for _ in range(k)]
    out += [[rng.randint(0, b) for b in bound] for _ in range(k)]
    out += [[bound[j] if j == i else 0 for j in range(10)] for i in range(10)]
    return out


def pairs(rng, fbound, gbound, k=150):
    """Operand pairs of a product: the patterns paired up, and every single
    limb of f against every single limb of g (each partial product alone)."""
    pf, pg = patterns(rng, fbound, k), patterns(rng, gbound, k)
    ps = list(zip(pf, pg))
    ps += [(pf[0], pg[1]), (pf[1], pg[0])]
    single_f, single_g = pf[-10:], pg[-10:]
    ps += [(a, b) for a in single_f for b in single_g]
    ps += [(pf[0], b) for b in single_g] + [(a, pg[0]) for a in single_f]
    return [p[0] for p in ps], [p[1] for p in ps]


def assert_fe(got, want, bound_ok=fb.is_R, what=""):
    """value mod p and limb bound of every row"""
    for i, row in enumerate(got.tolist()):
        assert value(row) % P == want[i] % P, (what, i, row)
        assert bound_ok(row), (what, "limb bound", i, row)


def within(bound):
    return lambda row: all(x <= b for x, b in zip(row, bound))


# =========================================================== A. field products
PRODUCTS = {
    "fe_mul": lambda f, g: f * g,
    "fe_mul2": lambda f, g: 2 * f * g,
    "fe_mul_g19": lambda f, g: f * g,
    "fe_sq": lambda f, g: f * f,
    "fe_sq2": lambda f, g: 2 * f * f,
}


@pytest.mark.parametrize("fn", sorted(PRODUCTS))
def test_field_products_at_call_site_bounds(dc, fn):
    """Each product form as the device issues it, at the maximum over its
    call sites: value mod p, and the output is R."""
    rng = random.Random("A" + fn)
    fbound, gbound = fb.function_max(fn)
    if gbound is None:
        F = patterns(rng, fbound, 300)
        got = dc.run(fn, fes(F), n=len(F))
        G = F
    else:
        F, G = pairs(rng, fbound, gbound)
        got = dc.run(fn, fes(F), fes(G), n=len(F))
    assert_fe(got, [PRODUCTS[fn](value(f), value(g)) for f, g in zip(F, G)], what=fn)


@pytest.mark.parametrize("site", [s for s in fb.SITES if s[1] == "fe_mul" and s[0].startswith(("qd_", "qo_"))],
                         ids=fb.site_id)
def test_field_product_at_quad_site_bounds(dc, site):
    """fe_mul at each quad call site's own bound pair (the doublings' M6 g
    operand with their M5 f operand), not only the limb-wise maximum."""
    label, fn, fbound, gbound, _ = site
    F, G = pairs(random.Random(label), fbound, gbound, 60)
    got = dc.run(fn, fes(F), fes(G), n=len(F))
    assert_fe(got, [value(f) * value(g) for f, g in zip(F, G)], what=label)


def test_field_product_aliasing_forms(dc):
    """fe_mul(h, h, g), fe_mul(h, f, h), fe_sq(h, h), fe_mul(h, f, f): the
    outputs are early-clobber registers, the source may name an input."""
    rng = random.Random("alias")
    fbound, gbound = fb.function_max("fe_mul")
    F, G = pairs(rng, fbound, gbound, 60)
    n = len(F)
    want = [value(f) * value(g) for f, g in zip(F, G)]
    assert_fe(dc.run("fe_mul_alias_hf", fes(F), fes(G), n=n), want, what="fe_mul(h, h, g)")
    assert_fe(dc.run("fe_mul_alias_hg", fes(F), fes(G), n=n), want, what="fe_mul(h, f, h)")
    S = patterns(rng, fb.function_max("fe_sq")[0], 100)
    assert_fe(dc.run("fe_sq_alias", fes(S), n=len(S)), [value(f) ** 2 for f in S], what="fe_sq(h, h)")
    # f is both operands: it must satisfy the (tighter) g bound
    S = patterns(rng, [min(a, b) for a, b in zip(fbound, gbound)], 100)
    assert_fe(dc.run("fe_mul_same", fes(S), n=len(S)), [value(f) ** 2 for f in S], what="fe_mul(h, f, f)")


def test_fe_sqn_against_pow(dc):
    F = patterns(random.Random("sqn"), fb.RP, 40)
    got = dc.run("fe_sqn", fes(F), n=len(F))
    for k, e in enumerate((1, 2, 5, 10, 20, 50, 100)):
        assert_fe(got[:, 10 * k:10 * k + 10], [pow(value(f), 2**e, P) for f in F], what="fe_sqn %d" % e)


def test_fe_invert_and_pow22523(dc):
    rng = random.Random("inv")
    F = [limbs(0), limbs(1), limbs(P - 1), limbs(P), limbs(2), limbs(P - 2)]
    F += patterns(rng, fb.RP, 30)  # uncarried representations
    F += [limbs(rng.randrange(P)) for _ in range(60)]
    v = [value(f) for f in F]
    assert_fe(dc.run("fe_invert", fes(F), n=len(F)), [pow(x, P - 2, P) for x in v], what="fe_invert")
    assert_fe(dc.run("fe_pow22523", fes(F), n=len(F)), [pow(x, (P - 5) // 8, P) for x in v], what="fe_pow22523")


# ================================================= B. housekeeping at the bounds
M3 = [3 * 2**26, 3 * 2**25] * 5


def test_fe_sub_forms_do_not_underflow(dc):
    """Subtrahend at its documented maximum (and at the last value the added
    multiple of p covers), minuend 0: limb i of the result is exactly the
    added limb minus g_i, never a 32-bit wrap."""
    rng = random.Random("sub")
    for fn, added, gmaxes in (("fe_sub", fb.P2, [fb.R, fb.RP, fb.P2]), ("fe_sub4", fb.P4, [M3, fb.DBL_Z, fb.P4]),
                              ("fe_neg", fb.P2, [fb.R, fb.P2])):
        G = []
        for gm in gmaxes:
            G += patterns(rng, gm, 40)
        zero = [[0] * 10] * len(G)
        got = dc.run(fn, fes(G), n=len(G)) if fn == "fe_neg" else dc.run(fn, fes(zero), fes(G), n=len(G))
        for row, g in zip(got.tolist(), G):
            assert row == [a - x for a, x in zip(added, g)], (fn, g)
            assert value(row) % P == -value(g) % P
    # and with a minuend: the value
    F, G = patterns(rng, fb.RP, 50), patterns(rng, fb.R, 50)
    for fn in ("fe_sub", "fe_sub4"):
        got = dc.run(fn, fes(F), fes(G), n=len(F))
        assert_fe(got, [value(f) - value(g) for f, g in zip(F, G)], bound_ok=lambda r: True, what=fn)


def test_fe_weak_and_weak_even(dc):
    rng = random.Random("weak")
    F = patterns(rng, [2**31 - 1] * 10, 200)
    got = dc.run("fe_weak", fes(F), n=len(F))
    # documented: limb 0 <= 2^26 + 19 2^6, even <= 2^26 + 2^6, odd <= 2^25 + 2^6
    assert_fe(got, [value(f) for f in F], bound_ok=within([2**26 + 19 * 64] + [2**25 + 64, 2**26 + 64] * 4 + [2**25 + 64]),
              what="fe_weak")
    # fe_weak_even up to the quad doublings' M6 operand before its carry
    m6 = fb.sub4(fb.add(fb.R, fb.R), fb.DBL_Z)
    F = patterns(rng, m6, 200)
    got = dc.run("fe_weak_even", fes(F), n=len(F))
    for row, f in zip(got.tolist(), F):
        assert value(row) == value(f), f  # the integer, not only its residue
        assert row[0] == f[0] and row[1] == f[1]
        assert all(row[i] < 2**26 for i in range(2, 10, 2)) and within(fb.QDBL_T)(row), row


def test_fe_tobytes_edges(dc):
    rng = random.Random("tobytes")
    V = [0, 1, P - 1, P, P + 1, P + 18, 2**255 - 1, 2 * P - 1]
    F = [limbs_wide(v) for v in V]
    F += [fb.P2, fb.P4] + patterns(rng, [2**31 - 1] * 10, 200) + patterns(rng, fb.RP, 50)
    got = dc.run("fe_tobytes", fes(F), n=len(F))
    for row, f in zip(got.tolist(), F):
        assert unwords(row) == value(f) % P, f


def test_fe_iszero_isnegative_on_real_zeros(dc):
    """The representations of zero the code really produces: fe_sub(x, x),
    fe_sub4(x, x) (computed on the device), p, 2p, 4p in limbs -- and
    non-zero neighbours."""
    rng = random.Random("flags")
    X = patterns(rng, fb.R, 40)
    F = dc.run("fe_sub", fes(X), fes(X), n=len(X)).tolist() + dc.run("fe_sub4", fes(X), fes(X), n=len(X)).tolist()
    assert all(value(f) % P == 0 for f in F)
    F += [limbs(0), limbs(P), fb.P2, fb.P4]
    F += [limbs(1), limbs(P - 1), limbs_wide(P + 1), limbs_wide(P + 2), limbs(2), limbs_wide(2 * P - 1),
          limbs_wide(2**255 - 1)]
    F += [limbs(rng.randrange(P)) for _ in range(40)] + patterns(rng, [2**31 - 1] * 10, 40)
    got = dc.run("fe_flags", fes(F), n=len(F))[:, 0].tolist()
    for g, f in zip(got, F):
        v = value(f) % P
        assert g == (1 if v == 0 else 0) | ((v & 1) << 1), f


def test_fe_frombytes_ignores_bit_255_and_does_not_reduce(dc):
    rng = random.Random("frombytes")
    V = [0, 1, P - 1, P, P + 1, 2**255 - 20, 2**255 - 1, 2**255, 2**255 + 1, 2**255 + P, 2**256 - 1]
    V += [rng.randrange(2**256) for _ in range(100)]
    got = dc.run("fe_frombytes", u32([words(v) for v in V], 8), n=len(V))
    for row, v in zip(got.tolist(), V):
        assert row == limbs(v & (2**255 - 1)), hex(v)


def test_fe_cmov(dc):
    rng = random.Random("cmov")
    H, F = patterns(rng, [2**32 - 1] * 10, 40), patterns(rng, [2**32 - 1] * 10, 40)
    F.reverse()
    cond = [rng.choice((0, 1, 1, 0xffffffff)) for _ in H]
    got = dc.run("fe_cmov", fes(H), fes(F), u32([[c] for c in cond], 1), n=len(H))
    for row, h, f, c in zip(got.tolist(), H, F, cond):
        assert row == (f if c else h)


# ============================================= C. scalars, the half-size reduction
def test_sc_reduce512(dc):
    rng = random.Random(4)
    top = (2**512 - 1) // L * L
    V = [0, 1, L - 1, L, L + 1, 2 * L, 2**512 - 1, top, top - 1, 2**252, 2**256 - 1, 2**256, L << 256]
    V += [rng.randrange(2**512) for _ in range(500)] + [rng.randrange(2**256) for _ in range(50)]
    got = dc.run("sc_reduce512", u32([words(v, 16) for v in V], 16), n=len(V))
    for row, v in zip(got.tolist(), V):
        assert unwords(row) == v % L, hex(v)


def test_sc_is_canonical(dc):
    rng = random.Random("canon")
    V = [0, 1, L - 2, L - 1, L, L + 1, 2**252 - 1, 2**252, 2**252 + 1, 2**253 - 1, 2**253, 2**255, 2**256 - 1,
         (L - 1) | 2**255, (L - 1) | 2**253, L + 2**255, 2**255 + 1, L - 2**32, L + 2**32, L - 2**224]
    V += [rng.randrange(2**256) for _ in range(50)] + [rng.randrange(L) for _ in range(50)]
    got = dc.run("sc_is_canonical", u32([words(v) for v in V], 8), n=len(V))[:, 0].tolist()
    assert got == [1 if v < L else 0 for v in V]


def test_sc_mul_signed_and_muladd(dc):
    rng = random.Random("mul")
    cases = [(L, rng.randrange(2**253), 1), (L, rng.randrange(2**253), 0), (rng.randrange(2**253), 0, 1),
             (0, rng.randrange(2**253), 1), (1, L, 1), (1, 1, 1), (1, 1, 0), (2**253 - 1, 2**253 - 1, 1),
             (2**253 - 1, 2**253 - 1, 0), (L - 1, L - 1, 1), (8, L, 1)]
    cases += [(rng.randrange(2**253), rng.randrange(2**253), rng.randrange(2)) for _ in range(300)]
    cases += [(rng.randrange(2**131) | 1, rng.randrange(L), rng.randrange(2)) for _ in range(100)]
    got = dc.run("sc_mul_signed", u32([words(c) for c, _, _ in cases], 8), u32([[g] for _, _, g in cases], 1),
                 u32([words(s) for _, s, _ in cases], 8), n=len(cases))
    for row, (c, s, neg) in zip(got.tolist(), cases):
        assert unwords(row) == (-c * s if neg else c * s) % L, (c, s, neg)
    tri = [(2**256 - 1,) * 3, (0, 0, 0), (L, L, L), (L - 1, L - 1, L - 1), (0, 5, 2**256 - 1)]
    tri += [tuple(rng.randrange(2**256) for _ in range(3)) for _ in range(300)]
    got = dc.run("sc_muladd", *[u32([words(t[k]) for t in tri], 8) for k in range(3)], n=len(tri))
    for row, (a, b, c) in zip(got.tolist(), tri):
        assert unwords(row) == (a * b + c) % L


def _sdigits(ws, bits):
    """packed two's-complement digits of `bits` bits, little-endian"""
    x, out = unwords(ws), []
    for i in range(256 // bits):
        d = (x >> (bits * i)) & ((1 << bits) - 1)
        out.append(d - (1 << bits) if d >> (bits - 1) else d)
    return out


def _s32(x):
    return x - 2**32 if x >> 31 else x


SCALARS = [0, 1, L - 1, L, 2**252, 2**253 - 1] + [int(c * 64, 16) & (2**253 - 1) for c in "78f"] + \
          [int("8" * 63, 16), int("7f" * 31, 16), int("80" * 31, 16), int("7fff" * 15, 16), int("8000" * 15, 16)]


def test_sc_digit_recodings(dc):
    """Rebuild the scalar from each recoding's digits; every digit in its
    documented range."""
    rng = random.Random("digits")
    S = SCALARS + [rng.randrange(2**253) for _ in range(300)]
    got = dc.run("sc_digits", u32([words(s) for s in S], 8), n=len(S)).tolist()
    for row, s in zip(got, S):
        for k, bits in enumerate((4, 8, 16)):
            d = _sdigits(row[8 * k:8 * k + 8], bits)
            assert sum(x << (bits * i) for i, x in enumerate(d)) == s, (bits, hex(s))
            assert all(-(1 << (bits - 1)) <= x < (1 << (bits - 1)) for x in d)
        d0, d1 = [_s32(x) for x in row[24:32]], [_s32(x) for x in row[32:40]]
        assert sum(x << (16 * i) for i, x in enumerate(d0 + d1)) == s, hex(s)
        assert all(-2**15 <= x < 2**15 for x in d0 + d1)


@pytest.mark.parametrize("bits", [4, 8, 16])
def test_sc_pop_top(dc, bits):
    rng = random.Random("pop%d" % bits)
    Dg = [0, 2**256 - 1, 1 << 255, (1 << 255) - 1, 1, int("8" * 64, 16), int("7" * 64, 16)]
    Dg += [rng.randrange(2**256) for _ in range(100)]
    got = dc.run("sc_pop_top", u32([words(d) for d in Dg], 8), bits, n=len(Dg)).tolist()
    for row, d in zip(got, Dg):
        assert _s32(row[0]) == _sdigits(words(d), bits)[-1], hex(d)
        assert unwords(row[1:]) == (d << bits) & (2**256 - 1), hex(d)


DEGENERATE_H = [0, 1, 2, 7, 8, L - 1, L - 8, 2**128 - 1, 2**128, 2**128 + 1, 2**252, (L - 1) // 8]


def _lattice_device(dc, hs):
    out = []
    for lo in range(0, len(hs), 4096):  # a few thousand lanes per launch
        part = hs[lo:lo + 4096]
        out += dc.run("sc_lattice_reduce", u32([words(h) for h in part], 8), n=len(part)).tolist()
    return [(unwords(r[:8]), unwords(r[8:16]), r[16], r[17]) for r in out]


def _lattice_host(hostcore, hs):
    c0, c1, neg = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32), ctypes.c_int()
    out = []
    for h in hs:
        nb = hostcore.hc_lattice_reduce(h.to_bytes(32, "little"), c0, c1, ctypes.byref(neg))
        out.append((int.from_bytes(c0.raw, "little"), int.from_bytes(c1.raw, "little"), neg.value, nb))
    return out


def _check_lattice(dc, hostcore, hs):
    got, host = _lattice_device(dc, hs), _lattice_host(hostcore, hs)
    for h, g, w in zip(hs, got, host):
        a, b, neg, bits = g
        assert neg in (0, 1)
        sb = -b if neg else b
        assert (a - sb * h) % N8 == 0 and b % 2 == 1, ("c0 == c1 h (mod 8L), c1 odd", h, g)
        assert bits == max(a.bit_length(), b.bit_length(), 1), ("bit length", h, g)
        assert ((a, sb) == (h, 1)) == ((w[0], -w[1] if w[2] else w[1]) == (h, 1)), ("trivial pair", h, g, w)
        assert g == w, ("device pair differs from the host build's", h, g, w)


def test_lattice_reduce_degenerate_and_random(dc, hostcore):
    rnd = random.Random(17)
    _check_lattice(dc, hostcore, DEGENERATE_H + [rnd.randrange(L) for _ in range(4000)])


def near_exact_h():
    """h = ceil(8L / q) + d: the first quotient 8L / h is q - (tiny), which a
    double rounds UP to q, so the exact Euclid step is right only because it
    under-estimates its quotient.  [(q, h)]"""
    qs = list(range(3, 130)) + [2**k + s for k in (12, 16, 20, 24, 30) for s in (-1, 0, 1)]
    return [(q, -(-N8 // q) + d) for q in qs for d in (0, 1, 2)]


def test_lattice_reduce_near_exact_quotients(dc, hostcore):
    """For odd q the pair is known in closed form: the remainders of (8L, h)
    are 8L - (q - 1) h, then q h - 8L (tiny), so (c0, c1) = (q h - 8L, +q)."""
    qh = near_exact_h()
    hs = [h for _, h in qh]
    _check_lattice(dc, hostcore, hs)
    for (q, h), g in zip(qh, _lattice_device(dc, hs)):
        if q & 1:
            c0 = q * h - N8
            assert g == (c0, q, 0, max(c0.bit_length(), q.bit_length())), (q, h, g)


def test_lattice_reduce_pinned_set_equals_host(dc, hostcore):
    """The 20,012 values whose host pairs test_host_arith.py pins by digest:
    the device's pairs are the same, so the digest holds on the device."""
    hs = DEGENERATE_H + [int.from_bytes(hashlib.sha512(b"lattice-pin" + i.to_bytes(4, "little")).digest(), "little") % L
                         for i in range(20000)]
    _check_lattice(dc, hostcore, hs)


# ========================================================== the affine reference
# (the plain Edwards law, BASE, T8 and assert_projective: tests/edwards_ref.py)
TORSION = [aff_mul(k, T8) for k in range(8)]  # the eight small-order points
assert len(set(TORSION)) == 8 and aff_mul(8, T8) == (0, 1)
_POOL = []


def _pool():
    """The small-order points, then multiples of B, every other one with a
    torsion component added (mixed order).  Built once."""
    if not _POOL:
        rng = random.Random("pool")
        q, step = aff_mul(rng.randrange(1, L), BASE), aff_mul(rng.randrange(1, L), BASE)
        assert aff_mul(L, q) == (0, 1)
        _POOL.extend(TORSION)
        for i in range(120):
            q = aff_add(q, step)
            _POOL.append(aff_add(q, TORSION[i % 8]) if i % 2 else q)
    return _POOL


def curve_points(rng, n):
    """n distinct points; from n = 8 on, all small-order points are among them"""
    pool = _pool()
    pts = rng.sample(pool, n) if n < 8 else pool[:8] + rng.sample(pool[8:], n - 8)
    rng.shuffle(pts)
    return pts


def p3_of(rng, pt):
    """extended coordinates with a random Z, canonical limbs"""
    z = rng.randrange(1, P)
    x, y = pt
    return [limbs(x * z % P), limbs(y * z % P), limbs(z), limbs(x * y * z % P)]


def cached_of(rng, pt):
    """(Y+X, Y-X, Z, 2dT) of the point with a random Z"""
    z = rng.randrange(1, P)
    x, y = pt
    return [limbs((y + x) * z % P), limbs((y - x) * z % P), limbs(z), limbs(2 * D * x * y * z % P)]


def flat(rows):
    return [sum(r, []) for r in rows]


# ======================================================== D. points, per lane
def _dbl_formula(X, Y, Z):
    rY, rZ = (Y * Y + X * X) % P, (Y * Y - X * X) % P
    return [2 * X * Y % P, rY, rZ, (2 * Z * Z - rZ) % P]


def _conv_formula(X, Y, Z, T):
    return [X * T % P, Y * Z % P, Z * T % P, X * Y % P]


def _add_formula(p, e, neg, zone):
    X, Y, Z, T = p
    qa, qb, qZ, qT = e
    TT, ZZ2 = T * qT % P, (2 * Z if zone else 2 * Z * qZ) % P
    PP, MM = (Y + X) * qa % P, (Y - X) * qb % P
    zp, zm = (ZZ2 + TT) % P, (ZZ2 - TT) % P
    return [(PP - MM) % P, (PP + MM) % P, zm if neg else zp, zp if neg else zm]


def _rows_at(rng, bounds, k):
    """k rows of len(bounds) field elements, limbs at / near / below each bound"""
    cols = [patterns(rng, b, k)[:2 * k + 2] for b in bounds]
    rows = [[c[i] for c in cols] for i in range(2 * k + 2) if i != 1]  # (drop the all-zero row)
    return rows


def test_ge_dbl_and_convert_formulas_at_bounds(dc):
    """The formulas are polynomial identities: inputs need not be on the
    curve.  Limbs at the documented input bounds; outputs mod p and within
    the documented output bounds."""
    rng = random.Random("gedbl")
    rows = _rows_at(rng, [fb.RP] * 3, 60)
    got = dc.run("ge_dbl", u32(flat(rows), 30), n=len(rows))
    out_b = [fb.DBL_X, fb.DBL_Y, fb.DBL_Z, fb.DBL_T]
    for row, r in zip(got.tolist(), rows):
        assert coords(row) == _dbl_formula(*[value(f) % P for f in r]), r
        assert all(within(out_b[k])(row[10 * k:10 * k + 10]) for k in range(4)), ("ge_dbl output bound", row)
    # conversion: X (M5) and Z f operands, Y and the partially carried T g operands
    in_b = [fb.lmax(fb.DBL_X, fb.ADD_X), fb.lmax(fb.DBL_Y, fb.ADD_Y), fb.lmax(fb.DBL_Z, fb.ADD_ZT),
            fb.lmax(fb.DBL_T, fb.ADD_ZT)]
    rows = _rows_at(rng, in_b, 60)
    for wantT in (1, 0):
        got = dc.run("ge_p1p1_convert", u32(flat(rows), 40), wantT, n=len(rows))
        for row, r in zip(got.tolist(), rows):
            want = _conv_formula(*[value(f) % P for f in r])
            if not wantT:
                want[3] = 0
                assert row[30:] == [0] * 10  # T untouched
            assert coords(row) == want, (wantT, r)
            assert all(fb.is_R(row[10 * k:10 * k + 10]) for k in range(4))


@pytest.mark.parametrize("neg", [0, 1])
@pytest.mark.parametrize("zone", [0, 1])
def test_ge_add_preswapped_formula_at_bounds(dc, neg, zone):
    rng = random.Random("geadd%d%d" % (neg, zone))
    P_rows = _rows_at(rng, [fb.RP] * 4, 60)
    E_rows = _rows_at(rng, [M3, M3, fb.RP, fb.R], 60)  # qa, qb at M3; qZ, qT2d R
    got = dc.run("ge_add_preswapped", u32(flat(P_rows), 40), u32(flat(E_rows), 40), neg, zone, n=len(P_rows))
    out_b = [fb.ADD_X, fb.ADD_Y, fb.ADD_ZT, fb.ADD_ZT]
    for row, p, e in zip(got.tolist(), P_rows, E_rows):
        want = _add_formula([value(f) % P for f in p], [value(f) % P for f in e], neg, zone)
        assert coords(row) == want, (p, e)
        assert all(within(out_b[k])(row[10 * k:10 * k + 10]) for k in range(4)), ("output bound", row)


def test_ge_p3_to_cached_and_tobytes(dc):
    rng = random.Random("cached")
    rows = _rows_at(rng, [fb.RP] * 4, 60)
    got = dc.run("ge_p3_to_cached", u32(flat(rows), 40), n=len(rows))
    for row, r in zip(got.tolist(), rows):
        X, Y, Z, T = [value(f) % P for f in r]
        assert coords(row) == [(Y + X) % P, (Y - X) % P, Z, 2 * D * T % P]
        assert row[20:30] == r[2]  # Z copied
        assert within(fb.PT_YPX)(row[:10]) and within(fb.PT_YMX)(row[10:20]) and fb.is_R(row[30:])
    # encoding of X/Z, Y/Z for any X, Y and Z != 0; curve points with a random Z among them
    rows = [r[:3] for r in rows] + [p3_of(rng, pt)[:3] for pt in curve_points(rng, 40)]
    got = dc.run("ge_p2_tobytes", u32(flat(rows), 30), n=len(rows))
    for row, r in zip(got.tolist(), rows):
        X, Y, Z = [value(f) % P for f in r]
        zi = pow(Z, P - 2, P)
        assert unwords(row) == aff_enc((X * zi % P, Y * zi % P)), r


def test_ge_per_lane_on_curve_points(dc):
    """Doubling and the four addition forms on curve points -- the eight
    small-order points and mixed-order points among them -- against the affine
    law, compared projectively."""
    rng = random.Random("curve")
    n = 48
    pts, qs = curve_points(rng, n), curve_points(rng, n)
    qs[:8] = pts[:8]  # P + P and P - P through the addition law
    P3 = [p3_of(rng, pt) for pt in pts]
    d = dc.run("ge_dbl", u32(flat([r[:3] for r in P3]), 30), n=n)
    for wantT in (1, 0):
        got = dc.run("ge_p1p1_convert", d, wantT, n=n)
        for row, pt in zip(got.tolist(), pts):
            assert_projective(row, aff_add(pt, pt), wantT, "ge_dbl")
    for neg in (0, 1):
        for zone in (0, 1):
            ent = []
            for q in qs:
                c = cached_of(rng, q)
                if zone:
                    c = [limbs((q[1] + q[0]) % P), limbs((q[1] - q[0]) % P), limbs(1), limbs(2 * D * q[0] * q[1] % P)]
                if neg:  # the caller swaps the pair
                    c[0], c[1] = c[1], c[0]
                ent.append(c)
            r = dc.run("ge_add_preswapped", u32(flat(P3), 40), u32(flat(ent), 40), neg, zone, n=n)
            got = dc.run("ge_p1p1_convert", r, 1, n=n)
            for row, pt, q in zip(got.tolist(), pts, qs):
                assert_projective(row, aff_add(pt, aff_neg(q) if neg else q), True, "ge_add neg=%d zone=%d" % (neg, zone))


def _frombytes_ref(s, negate):
    """libsodium 1.0.18 ge25519_frombytes_negate_vartime restated (and its
    non-negating twin): (ok, x, y)"""
    y = (s & (2**255 - 1)) % P  # read mod 2^255, not rejected when >= p
    sign = s >> 255
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    vxx = v * x * x % P
    if (vxx - u) % P:
        if (vxx + u) % P:
            return (0, None, None)
        x = x * SQRTM1 % P
    if ((x & 1) == sign) == bool(negate):
        x = -x % P
    return (1, x, y)


def test_ge_frombytes(dc):
    rng = random.Random("frombytes")
    enc = [aff_enc(pt) for pt in curve_points(rng, 40)]  # valid, small-order and mixed-order
    enc += [e ^ (1 << 255) for e in enc[:20]]
    enc += [1, 1 | 1 << 255, P - 1, (P - 1) | 1 << 255, 0, 1 << 255]  # y = 1, y = p - 1, y = 0; x = 0 with the sign bit
    enc += [P, P + 1, P | 1 << 255, (P + 1) | 1 << 255, 2**255 - 1, 2**256 - 1] + list(range(P + 2, P + 19))  # y >= p
    off = [y for y in range(2, 400) if aff_from_y(y, 0) is None][:30]
    enc += off + [y | 1 << 255 for y in off[:10]]
    enc += [rng.randrange(2**256) for _ in range(100)]
    for negate in (0, 1):
        got = dc.run("ge_frombytes", u32([words(e) for e in enc], 8), negate, n=len(enc)).tolist()
        oks = 0
        for row, e in zip(got, enc):
            ok, x, y = _frombytes_ref(e, negate)
            assert row[40] == ok, (hex(e), negate)
            if ok:
                oks += 1
                assert coords(row[:40]) == [x, y, 1, x * y % P], (hex(e), negate)
                assert row[20:30] == limbs(1) and within(fb.RP)(row[:10]) and fb.is_R(row[30:40])
        assert 60 <= oks <= len(enc) - 40  # (the curve points decode, the off-curve y do not)


# ======================================================= E. points on a quad
QUAD_NS = (1, 15, 16, 17)


def _same_on_all_lanes(got, n, cols=40):
    """rows (4 n, 40): the four lanes of each quad hold identical limbs"""
    g = got.reshape(n, 4, -1)[:, :, :cols]
    assert (g == g[:, :1]).all(), "the lanes of a quad disagree"
    return g[:, 0].tolist()


def _dbl_p3_formula(r):
    X, Y, Z = [value(f) % P for f in r[:3]]
    return _conv_formula(*_dbl_formula(X, Y, Z))


def test_qd_p1p1_to_p3(dc):
    rng = random.Random("qdconv")
    in_b = [fb.lmax(fb.DBL_X, fb.ADD_X), fb.lmax(fb.DBL_Y, fb.ADD_Y), fb.lmax(fb.DBL_Z, fb.ADD_ZT),
            fb.lmax(fb.QDBL_T, fb.ADD_ZT)]
    for n in QUAD_NS:
        rows = _rows_at(rng, in_b, 9)[:n]
        for wantT in (1, 0):
            got = _same_on_all_lanes(dc.run("qd_p1p1_to_p3", u32(flat(rows), 40), wantT, n=n), n)
            for row, r in zip(got, rows):
                want = _conv_formula(*[value(f) % P for f in r])
                if not wantT:
                    want[3] = 0
                assert coords(row) == want, (n, wantT, r)
                assert all(fb.is_R(row[10 * k:10 * k + 10]) for k in range(4))


@pytest.mark.parametrize("form", ["qd", "qo"])
def test_quad_doubling(dc, form):
    """A different point in each quad of the wave; partial waves (n = 1, 15,
    17) run with quads inactive.  Curve points against the affine law, and
    limbs at the R+ maxima (the conversion product then sees the M6 g operand)
    against the formula."""
    rng = random.Random("qdbl" + form)

    def run(rows, n, wantT):
        if form == "qd":
            return dc.run("qd_dbl", u32(flat(rows), 40), wantT, n=n)
        return dc.run("qo_dbl", u32(flat(rows), 40), 1, n=n)

    for n in QUAD_NS:
        pts = curve_points(rng, 24)[:n]
        rows = [p3_of(rng, pt) for pt in pts]
        for wantT in (1, 0) if form == "qd" else (1,):
            got = _same_on_all_lanes(run(rows, n, wantT), n, 40 if wantT else 30)
            for row, pt in zip(got, pts):
                assert_projective(row + [0] * (40 - len(row)), aff_add(pt, pt), bool(wantT), form + "_dbl")
        rows = _rows_at(rng, [fb.RP] * 4, 9)[:n]
        got = _same_on_all_lanes(run(rows, n, 1), n)
        for row, r in zip(got, rows):
            assert coords(row) == _dbl_p3_formula(r), (form, n, r)
            assert all(fb.is_R(row[10 * k:10 * k + 10]) for k in range(4))


@pytest.mark.parametrize("form", ["qd", "qo"])
@pytest.mark.parametrize("neg", [0, 1])
def test_quad_addition(dc, form, neg):
    rng = random.Random("qadd%s%d" % (form, neg))
    for n in QUAD_NS:
        pts, qs = curve_points(rng, 24)[:n], curve_points(rng, 24)[:n]
        if n > 2:
            qs[1] = pts[1]  # P + P, P - P
        rows, ent = [p3_of(rng, pt) for pt in pts], [cached_of(rng, q) for q in qs]
        for wantT in (1, 0) if form == "qd" else (1,):
            if form == "qd":
                got = dc.run("qd_add", u32(flat(rows), 40), u32(flat(ent), 40), neg, wantT, n=n)
            else:
                got = dc.run("qo_add", u32(flat(rows), 40), u32(flat(ent), 40), neg, n=n)
            got = _same_on_all_lanes(got, n, 40 if wantT else 30)
            for row, pt, q in zip(got, pts, qs):
                assert_projective(row + [0] * (40 - len(row)), aff_add(pt, aff_neg(q) if neg else q), bool(wantT),
                                  "%s_add n=%d" % (form, n))
        # limbs at the bounds, against the formula (entry fields: the pair at M3)
        rows = _rows_at(rng, [fb.RP] * 4, 9)[:n]
        ent = _rows_at(rng, [fb.PT_YPX, fb.PT_YMX, fb.RP, fb.R], 9)[:n]
        if form == "qd":
            got = dc.run("qd_add", u32(flat(rows), 40), u32(flat(ent), 40), neg, 1, n=n)
        else:
            got = dc.run("qo_add", u32(flat(rows), 40), u32(flat(ent), 40), neg, n=n)
        for row, p, e in zip(_same_on_all_lanes(got, n), rows, ent):
            ev = [value(f) % P for f in e]
            if neg:  # the probes pick the swapped pair for a negative digit, as the kernels' loads do
                ev[0], ev[1] = ev[1], ev[0]
            assert coords(row) == _conv_formula(*_add_formula([value(f) % P for f in p], ev, neg, 0)), (form, n, p, e)


def test_qo_identity_and_expand(dc):
    rng = random.Random("qoid")
    for n in QUAD_NS:
        got = _same_on_all_lanes(dc.run("qo_identity", n=n), n)
        assert got == [limbs(0) + limbs(1) + limbs(1) + limbs(0)] * n
        rows = _rows_at(rng, [[2**32 - 1] * 10] * 4, 9)[:n]  # expand moves limbs unchanged
        got = _same_on_all_lanes(dc.run("qo_dbl", u32(flat(rows), 40), 0, n=n), n)
        assert got == flat(rows)


@pytest.mark.parametrize("form", ["qd", "qo"])
def test_quad_chain(dc, form):
    """Sixteen steps, doublings and additions alternating, each quad its own
    point, entries and signs."""
    rng = random.Random("chain" + form)
    for n in QUAD_NS:
        pts = curve_points(rng, 24)[:n]
        ents = [curve_points(rng, 8) for _ in range(n)]
        masks = [rng.randrange(256) for _ in range(n)]
        rows = [p3_of(rng, pt) for pt in pts]
        E = [sum(cached_of(rng, q), []) for es in ents for q in es]
        got = dc.run(form + "_chain", u32(flat(rows), 40), u32(E, 40), u32([[m] for m in masks], 1), n=n)
        for row, pt, es, m in zip(_same_on_all_lanes(got, n), pts, ents, masks):
            for j, q in enumerate(es):
                pt = aff_add(pt, pt)
                pt = aff_add(pt, aff_neg(q) if (m >> j) & 1 else q)
            assert_projective(row, pt, True, "%s_chain n=%d" % (form, n))


# ================================================================= F. hashes
def _messages(rng, lens, aligns=(0, 1, 2, 3)):
    """Messages inside one buffer, >= 16 bytes clear on either side of each,
    at every dword alignment: (buffer, offsets, lengths, the messages)."""
    buf, off, ln, msgs = bytearray(rng.randbytes(16)), [], [], []
    for n in lens:
        for a in aligns:
            while len(buf) % 4 != a:
                buf += rng.randbytes(1)
            m = rng.randbytes(n)
            off.append(len(buf))
            ln.append(n)
            msgs.append(m)
            buf += m + rng.randbytes(16)
    buf += rng.randbytes(16)
    return np.frombuffer(bytes(buf), dtype=np.uint8).copy(), u32([[o] for o in off], 1), u32([[x] for x in ln], 1), msgs


def _rand_words(rng, n, k):
    raw = [rng.randbytes(4 * k) for _ in range(n)]
    return np.frombuffer(b"".join(raw), dtype=np.uint32).reshape(n, k).copy(), raw


def _digests(got):
    return [r.astype("<u4").tobytes() for r in got]


def test_sha512_ram(dc):
    rng = random.Random("sha512")
    buf, off, ln, msgs = _messages(rng, list(range(140)) + [239, 240, 241, 367, 368, 369, 1000])
    n = len(msgs)
    R, Rb = _rand_words(rng, n, 8)
    A, Ab = _rand_words(rng, n, 8)
    got = _digests(dc.run("sha512_ram_var", R, A, buf, off, ln, n=n))
    for g, r, a, m in zip(got, Rb, Ab, msgs):
        assert g == hashlib.sha512(r + a + m).digest(), len(m)
    M, Mb = _rand_words(rng, 64, 8)
    got = _digests(dc.run("sha512_ram32", R[:64], A[:64], M, n=64))
    for g, r, a, m in zip(got, Rb, Ab, Mb):
        assert g == hashlib.sha512(r + a + m).digest()


def test_cache_key_and_sha256(dc):
    rng = random.Random("hashes")
    buf, off, ln, msgs = _messages(rng, list(range(70)) + [127, 128, 129, 159, 160, 161, 255, 256, 257, 300, 1000])
    n = len(msgs)
    pk, pkb = _rand_words(rng, n, 8)
    sig, sigb = _rand_words(rng, n, 16)
    got = _digests(dc.run("cache_key", pk, sig, buf, off, ln, n=n))
    for g, p, s, m in zip(got, pkb, sigb, msgs):
        assert g == hashlib.blake2b(p + s + m, digest_size=32).digest(), len(m)
    buf, off, ln, msgs = _messages(rng, list(range(140)) + [183, 184, 191, 192, 247, 248, 1000, 4097])
    got = _digests(dc.run("sha256", buf, off, ln, n=len(msgs)))
    for g, m in zip(got, msgs):
        assert g == hashlib.sha256(m).digest(), len(m)
