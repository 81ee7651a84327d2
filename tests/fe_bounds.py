"""Limb bounds of both operands at every field-product call site of the device
code, derived from the code (DESIGN.md §2 "Limb bounds at the call sites").

One table, read by both test layers: tests/test_fe_asm_sim.py and
tests/test_host_arith.py run each product form at these bounds on the CPU,
tests/test_gpu_devcore.py on the device.  A bound is a list of ten inclusive
limb maxima; they are built with the same steps the code takes (add, the
subtractions that add 2p or 4p, the carry helpers), so each entry's derivation
is the expression that computes it.
"""

P = 2**255 - 19
OFF = [26 * ((i + 1) // 2) + 25 * (i // 2) for i in range(10)]
WIDTH = [26, 25] * 5

# limbs of 2p and 4p as fe_sub / fe_sub4 add them (fe25519.h)
P2 = [0x7ffffda] + [0x3fffffe, 0x7fffffe] * 4 + [0x3fffffe]
P4 = [0xfffffb4] + [0x7fffffc, 0xffffffc] * 4 + [0x7fffffc]

# C: a canonical decode (fe_frombytes, a curve constant): every limb within its width
C = [(1 << w) - 1 for w in WIDTH]
# R: what a product leaves.  Even limbs < 2^26; odd limbs < 2^25 except limb 1,
# which takes the wrap's second carry (< 2^17).  The looser statement of R used
# throughout (even < 2^26, odd <= 2^25 + 2^17) is kept for every odd limb.
R = [2**26 - 1, 2**25 + 2**17] * 5
# RP: anything "carried" a product may be handed: R, or the output of fe_weak on
# limbs < 2^31 (limb 0 <= 2^26 - 1 + 19*63, even <= 2^26 - 1 + 63, odd <= 2^25 - 1 + 31)
RP = [2**26 - 1 + 19 * 64, 2**25 + 2**17] * 5


def add(f, g):  # fe_add
    return [a + b for a, b in zip(f, g)]


def sub(f, g):  # fe_sub: f + 2p - g; g must fit under 2p's limbs
    assert all(b <= m for b, m in zip(g, P2)), "fe_sub subtrahend above 2p's limbs"
    return [a + m for a, m in zip(f, P2)]


def sub4(f, g):  # fe_sub4: f + 4p - g; g must fit under 4p's limbs
    assert all(b <= m for b, m in zip(g, P4)), "fe_sub4 subtrahend above 4p's limbs"
    return [a + m for a, m in zip(f, P4)]


def weak_even(f):  # fe_weak_even: limbs 2, 4, 6, 8 carried into 3, 5, 7, 9
    h = list(f)
    for i in range(2, 10, 2):
        h[i + 1] += h[i] >> 26
        h[i] = min(h[i], 2**26 - 1)
    return h


def lmax(*bs):
    return [max(x) for x in zip(*bs)]


# ---- the completed (p1p1) points the conversions consume
# ge_dbl (ge25519.h): inputs RP
DBL_Y = add(R, R)                       # YY + XX
DBL_Z = sub(R, R)                       # YY + 2p - XX
DBL_X = sub4(R, DBL_Y)                  # AA + 4p - (YY + XX)
DBL_T = weak_even(sub4(R, DBL_Z))       # ZZ2 = fe_sq2 output (R): R + 4p - Z, even limbs carried
# qd_dbl / qo_dbl (quad.h): 2 Z^2 is sq + sq, so T starts one R higher
QDBL_T = weak_even(sub4(add(R, R), DBL_Z))
# ge_add_preswapped / qd_add / qo_add: PP, MM, TT are R; ZZ2 is R (fe_mul2) or RP (zone: fe_weak)
ADD_X = sub(R, R)                       # PP + 2p - MM
ADD_Y = add(R, R)                       # PP + MM
ADD_ZT = lmax(add(RP, R), sub(RP, R))   # ZZ2 + TT | ZZ2 + 2p - TT, by sign either is Z or T
# operands of an addition: the running point is RP; a cached entry holds
# (Y + X, Y + 2p - X, Z, 2dT) of an RP point
PT_YPX = add(RP, RP)
PT_YMX = sub(RP, RP)
ENT = lmax(PT_YPX, PT_YMX, RP)          # any field of a cached / affine entry (documented: the pair <= M3)

# (site, function, f bound, g bound, derivation); g is None for squarings
SITES = [
    # ---- ge25519.h
    ("ge_dbl AA", "fe_sq", add(RP, RP), None, "A = X + Y of an RP point"),
    ("ge_dbl XX", "fe_sq", RP, None, "X of an RP point"),
    ("ge_dbl YY", "fe_sq", RP, None, "Y of an RP point"),
    ("ge_dbl ZZ2", "fe_sq2", RP, None, "Z of an RP point"),
    ("ge_p1p1_convert after dbl T=X*Y", "fe_mul_g19", DBL_X, DBL_Y, "X = AA + 4p - (YY+XX) by Y = YY + XX"),
    ("ge_p1p1_convert after dbl Y=Z*Y", "fe_mul_g19", DBL_Z, DBL_Y, "Z = YY + 2p - XX by Y"),
    ("ge_p1p1_convert after dbl X=X*T", "fe_mul_g19", DBL_X, DBL_T, "X by T = weak_even(ZZ2 + 4p - Z), ZZ2 <= R"),
    ("ge_p1p1_convert after dbl Z=Z*T", "fe_mul_g19", DBL_Z, DBL_T, "Z by T"),
    ("ge_p1p1_convert after add T=X*Y", "fe_mul_g19", ADD_X, ADD_Y, "X = PP + 2p - MM by Y = PP + MM"),
    ("ge_p1p1_convert after add Y=Z*Y", "fe_mul_g19", ADD_ZT, ADD_Y, "Z = ZZ2 +- TT by Y"),
    ("ge_p1p1_convert after add X=X*T", "fe_mul_g19", ADD_X, ADD_ZT, "X by T = ZZ2 -+ TT"),
    ("ge_p1p1_convert after add Z=Z*T", "fe_mul_g19", ADD_ZT, ADD_ZT, "Z by T"),
    ("ge_add_preswapped TT", "fe_mul", RP, R, "T of the point by the entry's 2dT (a product)"),
    ("ge_add_preswapped ZZ2", "fe_mul2", RP, RP, "Z of the point by the entry's Z (a point's Z)"),
    ("ge_add_preswapped PP", "fe_mul", PT_YPX, ENT, "Y + X by the entry's (Y+X | Y-X) side"),
    ("ge_add_preswapped MM", "fe_mul", PT_YMX, ENT, "Y + 2p - X by the entry's other side"),
    ("ge_p3_to_cached T2d", "fe_mul", RP, C, "T by the constant 2d"),
    ("ge_frombytes u", "fe_sq", C, None, "decoded y"),
    ("ge_frombytes v", "fe_mul", R, C, "y^2 by the constant d"),
    ("ge_frombytes v^2", "fe_sq", RP, None, "v after fe_weak"),
    ("ge_frombytes v^3", "fe_mul", R, RP, "v^2 by v"),
    ("ge_frombytes v^6", "fe_sq", R, None, "v^3"),
    ("ge_frombytes v^7", "fe_mul", R, RP, "v^6 by v"),
    ("ge_frombytes uv^7", "fe_mul", R, RP, "v^7 by u after fe_weak"),
    ("ge_frombytes x*v3", "fe_mul", R, R, "the power by v^3"),
    ("ge_frombytes x*u", "fe_mul", R, RP, "by u"),
    ("ge_frombytes_finish x^2", "fe_sq", R, None, "x"),
    ("ge_frombytes_finish vxx", "fe_mul", R, RP, "x^2 by v"),
    ("ge_frombytes_finish xs", "fe_mul", R, C, "x by sqrt(-1)"),
    ("ge_frombytes_finish T", "fe_mul", RP, C, "x after fe_weak by decoded y"),
    ("ge_p2_tobytes_zinv x", "fe_mul", RP, R, "X by 1/Z"),
    ("ge_p2_tobytes_zinv y", "fe_mul", RP, R, "Y by 1/Z"),
    # ---- fe25519.h chains (fe_sqn, fe_pow_2_250_1, fe_pow22523, fe_invert): the
    # argument is RP, every later operand a product
    ("fe_pow chain z^2", "fe_sq", RP, None, "the argument"),
    ("fe_pow chain products", "fe_mul", R, RP, "a power by the argument or another power"),
    ("fe_pow chain squarings", "fe_sq", R, None, "a power"),
    # ---- quad.h
    ("qd_dbl sq", "fe_sq", add(RP, RP), None, "X, Y, Z or X + Y of an RP point, by role"),
    # (one statement, a different operand pair on each lane of the quad)
    ("qd_dbl lane 0 X*T", "fe_mul", DBL_X, QDBL_T, "X (M5) by T = weak_even(sq + sq + 4p - Z): M6"),
    ("qd_dbl lane 1 Y*Z", "fe_mul", DBL_Y, DBL_Z, "Y = YY + XX by Z = YY + 2p - XX"),
    ("qd_dbl lane 2 Z*T", "fe_mul", DBL_Z, QDBL_T, "Z by T (M6)"),
    ("qd_dbl lane 3 X*Y", "fe_mul", DBL_X, DBL_Y, "X (M5) by Y"),
    ("qd_add lane 0 T*2dT", "fe_mul", RP, R, "T of the point by the entry's 2dT"),
    ("qd_add lane 1 2Z*Z", "fe_mul", add(RP, RP), RP, "Z + Z by the entry's Z"),
    ("qd_add lane 2 (Y+X)*side", "fe_mul", PT_YPX, lmax(PT_YPX, PT_YMX), "Y + X by the entry's Y+X (Y-X if neg)"),
    ("qd_add lane 3 (Y-X)*side", "fe_mul", PT_YMX, lmax(PT_YPX, PT_YMX), "Y + 2p - X by the entry's other side"),
    ("qd_add conversion lane 0 X*T", "fe_mul", ADD_X, ADD_ZT, "X = PP + 2p - MM by T = ZZ -+ TT"),
    ("qd_add conversion lane 1 Y*Z", "fe_mul", ADD_Y, ADD_ZT, "Y = PP + MM by Z = ZZ +- TT"),
    ("qd_add conversion lane 2 Z*T", "fe_mul", ADD_ZT, ADD_ZT, "Z by T"),
    ("qd_add conversion lane 3 X*Y", "fe_mul", ADD_X, ADD_Y, "X by Y"),
    ("qo_dbl sq", "fe_sq", add(RP, RP), None, "own coordinate, or X + Y on lane 3"),
    ("qo_dbl lane 0 X*T", "fe_mul", DBL_X, QDBL_T, "as qd_dbl: T is M6"),
    ("qo_dbl lane 1 Y*Z", "fe_mul", DBL_Y, DBL_Z, "as qd_dbl"),
    ("qo_dbl lane 2 Z*T", "fe_mul", DBL_Z, QDBL_T, "as qd_dbl: T is M6"),
    ("qo_dbl lane 3 X*Y", "fe_mul", DBL_X, DBL_Y, "as qd_dbl"),
    ("qo_add lane 0 (X+Y)*side", "fe_mul", PT_YPX, lmax(PT_YPX, PT_YMX), "own X + lane 1's Y by the entry's side"),
    ("qo_add lane 1 (Y-X)*side", "fe_mul", PT_YMX, lmax(PT_YPX, PT_YMX), "own Y + 2p - lane 0's X by the other side"),
    ("qo_add lane 2 2Z*Z", "fe_mul", add(RP, RP), RP, "Z + Z by the entry's Z"),
    ("qo_add lane 3 T*2dT", "fe_mul", RP, R, "T by the entry's 2dT"),
    ("qo_add conversion lane 0 X*T", "fe_mul", ADD_X, ADD_ZT, "as qd_add"),
    ("qo_add conversion lane 1 Y*Z", "fe_mul", ADD_Y, ADD_ZT, "as qd_add"),
    ("qo_add conversion lane 2 Z*T", "fe_mul", ADD_ZT, ADD_ZT, "as qd_add"),
    ("qo_add conversion lane 3 X*Y", "fe_mul", ADD_X, ADD_Y, "as qd_add"),
    # ---- verify_core.h
    ("sv_verify_core 1/Z", "fe_sq", R, None, "fe_invert of a conversion product"),
    ("sv_btab_entry x", "fe_mul", R, R, "X by 1/Z"),
    ("sv_btab_entry y", "fe_mul", R, R, "Y by 1/Z"),
    ("sv_btab_entry xy", "fe_mul", R, R, "x by y"),
    ("sv_btab_entry xy2d", "fe_mul", R, C, "xy by the constant 2d"),
    ("sv_btab_entry_shift x", "fe_mul", R, R, "X by 1/Z"),
    ("sv_btab_entry_shift y", "fe_mul", R, R, "Y by 1/Z"),
    ("sv_btab_entry_shift xy", "fe_mul", R, R, "x by y"),
    ("sv_btab_entry_shift xy2d", "fe_mul", R, C, "xy by the constant 2d"),
    # ---- sv_kernels.hip, sv_comb.hip
    ("sv_kernels first window 2T", "fe_mul", R, C, "the entry's 2dT by the constant 1/d"),
    ("sv_kernels octet hand-over t2d", "fe_mul", R, C, "T by the constant 2d"),
    ("sv_comb qo_from_cached 2T", "fe_mul", ENT, C, "this lane's entry field (any) by the constant 1/d"),
    ("sv_comb qo_to_cached 2dT", "fe_mul", RP, C, "own coordinate by the constant 2d"),
    ("sv_comb root x_R Z", "fe_mul", RP, R, "decoded R coordinate by Z"),
]

STATEMENT = {"fe_mul": "fe_mul_asm", "fe_mul_g19": "fe_mul_g19_asm", "fe_mul2": "fe_mul2_asm", "fe_sq": "fe_sq_asm",
             "fe_sq2": "fe_sq2_asm"}


def site_id(site):
    """pytest id of a table entry"""
    return "_".join("".join(c if c.isalnum() else " " for c in site[0].replace("*", " by ")).split())


def function_max(fn):
    """Limb-wise maximum of (f, g) over the call sites of one product form."""
    rows = [s for s in SITES if s[1] == fn]
    f = lmax(*[s[2] for s in rows])
    g = None if rows[0][3] is None else lmax(*[s[3] for s in rows])
    return f, g


def value(limbs):
    return sum(int(x) << OFF[i] for i, x in enumerate(limbs))


# The product forms' output: even limbs < 2^26, odd limbs <= 2^25 + 2^17
def is_R(limbs):
    return all(int(x) <= (2**26 - 1 if i % 2 == 0 else 2**25 + 2**17) for i, x in enumerate(limbs))
