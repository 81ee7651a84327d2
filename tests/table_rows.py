"""Rows for the table and record tests (tests/test_tables_cpu.py,
tests/test_gpu_tables.py) that no fixture holds by construction.

sv_lat_prepare's top-digit carry (TOP8A / TOP8R: a scalar of 4W - 1 bits whose
signed radix-16 recoding carries out of digit W - 1) needs a lattice pair of
exactly 4W - 1 bits, W > 33: rare, and on an invalid signature a wrong digit
string still rejects.  The rows here are VALID signatures (RFC 8032, signed by
the oracle) of seeded keys and messages; TOP8_SEEDS were found by find_top8
on the host build's sv_lat_prepare (hc_lat_record) and are committed as seeds,
not as rows.  Each seeded row raises its flag at its own window count, i.e.
when it is a wave's only signature (a launch of n = 1).
"""
import ctypes
import hashlib

import numpy as np


def seeded_row(oracle, seed, mlen):
    """(pk, sig, msg): the valid signature of seed's key over seed's mlen-byte message."""
    tag = b"table-row" + int(seed).to_bytes(8, "little") + int(mlen).to_bytes(4, "little")
    sk_seed = hashlib.sha256(tag + b"key").digest()
    msg = hashlib.shake_256(tag + b"msg").digest(mlen)
    pk, sk, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_seed_keypair(pk, sk, sk_seed)
    oracle.oracle_ed25519_sign(sig, msg, mlen, sk)
    return pk.raw, sig.raw, msg


def lat_record(hostcore, pk, sig, msg, W=0, trivial=False, tabs=False):
    """hc_lat_record -> (rec[32] uint32, info dict, tables or None)"""
    rec = np.zeros(32, np.uint32)
    info = (ctypes.c_int32 * 6)()
    t = np.zeros(2 * 9 * 40, np.uint32) if tabs else None
    hostcore.hc_lat_record.restype = None
    hostcore.hc_lat_record(bytes(pk), bytes(sig), bytes(msg), ctypes.c_uint32(len(msg)), ctypes.c_int(W),
                           ctypes.c_int(1 if trivial else 0), rec.ctypes.data_as(ctypes.c_void_p), info,
                           t.ctypes.data_as(ctypes.c_void_p) if tabs else None)
    keys = ("rneg", "top8A", "top8R", "ok", "w_lane", "W")
    return rec, dict(zip(keys, [int(v) for v in info])), t


def find_top8(hostcore, oracle, mlen, flags, start=0, limit=2_000_000):
    """The first seed >= start whose row's (top8A, top8R) at its own window count equal `flags`."""
    for seed in range(start, start + limit):
        pk, sig, msg = seeded_row(oracle, seed, mlen)
        info = lat_record(hostcore, pk, sig, msg)[1]
        if (info["top8A"], info["top8R"]) == tuple(flags):
            return seed
    raise AssertionError("no seed found")


# (mlen, flag) -> seed.  The "top8A" rows raise TOP8A alone; a lattice pair whose c1 has 4W - 1 bits comes from the
# balanced combination, whose c0 then has as many, so the "top8R" rows raise both flags.
TOP8_SEEDS = {(32, "top8A"): 67196, (32, "top8R"): 6910, (33, "top8A"): 167988, (33, "top8R"): 2208}


def top8_rows(oracle, mlen):
    """[(pk, sig, msg)] for mlen: the TOP8A row, then the TOP8R row."""
    return [seeded_row(oracle, TOP8_SEEDS[(mlen, f)], mlen) for f in ("top8A", "top8R")]


def mixed_order_keys(pk):
    """The encodings of A + [k]T8, k = 1..7, for the key pk (a point of the prime-order subgroup)."""
    import edwards_ref as er
    y = int.from_bytes(pk, "little")
    A = er.aff_from_y(y & ((1 << 255) - 1), y >> 255)
    assert A is not None
    out, t = [], (0, 1)
    for _ in range(7):
        t = er.aff_add(t, er.T8)
        out.append(er.aff_enc(er.aff_add(A, t)).to_bytes(32, "little"))
    assert len(set(out)) == 7 and er.aff_add(t, er.T8) == (0, 1)
    return out


def record_ok(pk, sig):
    """What SV_REC_OK stands for (verify_core.h sv_lat_pre): none of the
    conditions (1)-(5) fails, and R is the canonical encoding of a curve point
    (y < p and decodable: otherwise libsodium's byte comparison of step (8)
    can never succeed) -- everything but the group equation."""
    import isolating_rows as ir
    r = bytes(sig[:32])
    y = int.from_bytes(r, "little") & ((1 << 255) - 1)
    return not ir.conditions(pk, sig) and y < ir.P and ir.dec_lenient(r) is not None
