"""A pure-Python restatement of the audit's pick (stellar-core_amd/csrc/audit.h) and the inputs the audit tests
share: written from the header's comment, not compiled from it."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
REJECTS, SAMPLE, STRICT = 1, 2, 4
DEFAULT_BUDGET = 65536
SETS = ("intree", "valid", "msglen", "longmsg", "adversarial", "lattice_edge")


def fin(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix(seed, seq, i):
    s = fin((seed + GOLD * (seq + 1)) & M64)
    return fin(((s ^ i) + GOLD) & M64)


def picks(what, one_in, seed, seq, verdict):
    """Every picked row, ascending (before the budget)."""
    out = []
    for i, v in enumerate(verdict):
        if (what & REJECTS and v == 0) or (what & SAMPLE and mix(seed, seq, i) % one_in == 0):
            out.append(i)
    return out


def audited(what, one_in, seed, seq, verdict, budget=0):
    """(the audited rows, over_budget)"""
    p = picks(what, one_in, seed, seq, verdict)
    b = budget or DEFAULT_BUDGET
    return p[:b], max(0, len(p) - b)


def tiled(d, n):
    """n rows tiled from fixture set d, as a variable-length batch."""
    k = len(d["verdict"])
    idx = np.arange(n) % k
    ln = d["msg_len"][idx].astype(np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    msg = np.concatenate([d["msg"][int(d["msg_off"][i]):int(d["msg_off"][i]) + int(d["msg_len"][i])] for i in range(k)]
                         * ((n + k - 1) // k))[:int(ln.sum())]
    return {"pk": np.ascontiguousarray(d["pk"][idx]), "sig": np.ascontiguousarray(d["sig"][idx]),
            "msg": np.ascontiguousarray(msg), "msg_off": off, "msg_len": ln,
            "verdict": np.ascontiguousarray(d["verdict"][idx])}


def is_fixed32(d):
    n = len(d["verdict"])
    return bool((d["msg_len"] == 32).all() and (d["msg_off"] == 32 * np.arange(n, dtype=np.uint64)).all())


def inverted_rows(name, d):
    """The rows whose claimed verdict the tests invert: first, last, and for `adversarial` one accept and one
    reject from the middle."""
    n = len(d["verdict"])
    rows = {0, n - 1}
    if name == "adversarial":
        v = d["verdict"]
        rows.add(int(np.flatnonzero(v[1:-1] == 1)[0]) + 1)
        rows.add(int(np.flatnonzero(v[1:-1] == 0)[0]) + 1)
    return sorted(rows)
