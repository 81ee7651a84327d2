"""Plain-Python RFC 8032 ed25519 signer for the tests (no signer is installed
where the CPU tests run).  Not constant time, test keys only.  Every signature
made through sign_checked() is asserted valid by the oracle before it is used:
that assertion is this signer's own check."""
import hashlib

P = 2 ** 255 - 19
L = 2 ** 252 + 27742317777372353535851937790883648493
D = -121665 * pow(121666, P - 2, P) % P
_BY = 4 * pow(5, P - 2, P) % P
_BX = 15112221349535400772501151409588531511454012693041857206046113283949847762202
B = (_BX, _BY, 1, _BX * _BY % P)


def _add(p, q):
    a = (p[1] - p[0]) * (q[1] - q[0]) % P
    b = (p[1] + p[0]) * (q[1] + q[0]) % P
    c = 2 * p[3] * q[3] * D % P
    d = 2 * p[2] * q[2] % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def _mul(s, p):
    q = (0, 1, 1, 0)
    while s:
        if s & 1:
            q = _add(q, p)
        p = _add(p, p)
        s >>= 1
    return q


def _enc(p):
    zi = pow(p[2], P - 2, P)
    x, y = p[0] * zi % P, p[1] * zi % P
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def keypair(seed: bytes):
    """(a, prefix, pk) of the 32-byte seed (== crypto_sign_seed_keypair)."""
    h = hashlib.sha512(seed).digest()
    a = (int.from_bytes(h[:32], "little") & ((1 << 254) - 8)) | (1 << 254)
    return a, h[32:], _enc(_mul(a, B))


def sign(key, msg: bytes) -> bytes:
    a, prefix, pk = key
    r = int.from_bytes(hashlib.sha512(prefix + msg).digest(), "little") % L
    R = _enc(_mul(r, B))
    h = int.from_bytes(hashlib.sha512(R + pk + msg).digest(), "little") % L
    return R + ((r + h * a) % L).to_bytes(32, "little")


def sign_checked(oracle, key, msg: bytes) -> bytes:
    sig = sign(key, msg)
    assert oracle.oracle_ed25519_verify(sig, msg, len(msg), key[2]) == 0, "pysign made a signature the oracle rejects"
    return sig
