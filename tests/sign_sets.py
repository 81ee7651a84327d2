"""Inputs of the signing tests (test_sign_cpu.py, test_gpu_sign.py).

fixture_set(golden): the ~1600 libsodium signatures of the committed fixtures
whose seeds are derivable (tests/golden/make_golden.py), as ONE mixed-length
signing call: messages packed back to back, so their offsets take every
alignment, with the fixtures' pk and sig as the expected bytes.

chosen_scalars(): the scalars the fixed-base multiplication is pinned on, and
fixed_base_ref(): encode([s]B) by integer arithmetic (edwards_ref.py).
"""
import hashlib
import struct

import numpy as np

import edwards_ref as er

L = er.L


def seed_of(i):
    return hashlib.sha256(b"SVSEED" + struct.pack("<Q", i)).digest()


def msg_of(i):
    return hashlib.sha256(b"SVMSG" + struct.pack("<Q", i)).digest()


_fixture_cache = {}


def fixture_set(golden):
    """dict(seed k x 32, msg, off, len, pk k x 32, sig k x 64): k == n, key i signs message i."""
    if "set" in _fixture_cache:
        return _fixture_cache["set"]
    seeds, msgs, pks, sigs = [], [], [], []

    def take(d, cls_name, seed_index):
        names = [str(x) for x in d["class_names"]]
        rows = np.nonzero(d["cls"] == names.index(cls_name))[0]
        for j, i in enumerate(rows):
            o, ln = int(d["msg_off"][i]), int(d["msg_len"][i])
            seeds.append(seed_of(seed_index(j, ln)))
            msgs.append(d["msg"][o:o + ln].tobytes())
            pks.append(d["pk"][i].tobytes())
            sigs.append(d["sig"][i].tobytes())
        return len(rows)

    assert take(golden["msglen"], "msglen_valid", lambda j, ln: 2_000_000 + ln) == 513
    assert take(golden["valid"], "valid32", lambda j, ln: j) == 1024
    assert take(golden["valid"], "valid256", lambda j, ln: 1_000_000 + j) == 64
    assert take(golden["longmsg"], "long_valid", lambda j, ln: 4_000_000 + j) == 18
    n = len(seeds)
    lens = np.array([len(m) for m in msgs], np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    assert len({int(o) & 3 for o in off}) == 4, "the offsets must take every alignment"
    s = dict(seed=np.frombuffer(b"".join(seeds), np.uint8).reshape(n, 32).copy(),
             msg=np.frombuffer(b"".join(msgs), np.uint8).copy(), off=off, len=lens,
             pk=np.frombuffer(b"".join(pks), np.uint8).reshape(n, 32).copy(),
             sig=np.frombuffer(b"".join(sigs), np.uint8).reshape(n, 64).copy(), n=n)
    _fixture_cache["set"] = s
    return s


def svseed_set(n):
    """The SVSEED / SVMSG set of digests.json: (seeds n x 32, msgs n x 32)."""
    seeds = np.frombuffer(b"".join(seed_of(i) for i in range(n)), np.uint8).reshape(n, 32).copy()
    msgs = np.frombuffer(b"".join(msg_of(i) for i in range(n)), np.uint8).reshape(n, 32).copy()
    return seeds, msgs


def stream_digest(pk, sig, msgs):
    return hashlib.sha256(np.concatenate([pk, sig, msgs], axis=1).tobytes()).hexdigest()


def chosen_scalars():
    """n x 32 little-endian scalars, all < 2^253."""
    m253 = (1 << 253) - 1
    s = [0, 1, 2, L - 1, 1 << 252, m253,
         int.from_bytes(b"\x80" * 32, "little") & m253,   # every radix-256 digit is -128 with a carry
         int.from_bytes(b"\x7f" * 32, "little") & m253,   # every digit is +127
         # a recoding whose carry runs through all 32 digits: 0x80 then 0xff.. (each digit becomes 0 or -128 + carry)
         (int.from_bytes(b"\x80" + b"\xff" * 30 + b"\x0f", "little")) & m253]
    rng = np.random.default_rng(20251021)
    s += [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") & m253 for _ in range(256)]
    return s, np.frombuffer(b"".join(v.to_bytes(32, "little") for v in s), np.uint8).reshape(len(s), 32).copy()


_ref_cache = {}


def fixed_base_ref():
    """encode([s]B) of chosen_scalars() by integer arithmetic, n x 32 bytes (computed once)."""
    if "ref" not in _ref_cache:
        ints, _ = chosen_scalars()
        pow2 = [er.ext(er.BASE)]
        for _ in range(253):
            pow2.append(er.ext_add(pow2[-1], pow2[-1]))
        out = []
        for v in ints:
            acc = er.IDENT
            for b in range(253):
                if (v >> b) & 1:
                    acc = er.ext_add(acc, pow2[b])
            zi = pow(acc[2], er.P - 2, er.P)
            out.append(er.aff_enc((acc[0] * zi % er.P, acc[1] * zi % er.P)).to_bytes(32, "little"))
        _ref_cache["ref"] = np.frombuffer(b"".join(out), np.uint8).reshape(len(out), 32).copy()
    return _ref_cache["ref"]


def tx_signing_set(rng):
    """Bodies of the three kinds, among them one with no signature and one with three signers; k = 5 keys."""
    import txbodies_pool as tp
    kinds = [tp.V1, tp.V0, tp.FEE_BUMP, tp.V1, tp.V0, tp.FEE_BUMP, tp.V1]
    lens = [120, 0, 77, 300, 64, 1, 2049]
    counts = [1, 2, 0, 3, 1, 1, 2]
    length = np.array(lens, np.uint32)
    off = np.zeros(len(lens), np.uint64)
    off[1:] = np.cumsum(length[:-1], dtype=np.uint64)
    blob = rng.integers(0, 256, int(length.sum()) + 1, dtype=np.uint8)
    sig_begin = np.zeros(len(lens) + 1, np.uint64)
    sig_begin[1:] = np.cumsum(counts)
    n = int(sig_begin[-1])
    seeds = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    key_of = np.array([0, 1, 2, 3, 4, 0, 4, 4, 2, 1], np.uint32)[:n]
    assert len(key_of) == n
    digests = np.array([np.frombuffer(tp.contents_hash(kinds[t], blob[int(off[t]):int(off[t]) + lens[t]]), np.uint8)
                        for t in range(len(lens))], np.uint8)
    owner = np.repeat(np.arange(len(lens)), counts)
    return dict(bodies=blob, off=off, len=length, kind=np.array(kinds, np.uint8), sig_begin=sig_begin, n=n,
                nb=len(lens), seed=seeds, key_of=key_of, digests=digests, sig_msgs=digests[owner])
