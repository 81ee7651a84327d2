"""Input builder and numpy restatement of the decide entry points
(sv_ed25519_decide_txbodies*; test_txresults_cpu.py, test_gpu_txresults.py).

RBuilder extends txaccounts_pool.ABuilder: a check carries a role (TX: the
source account, the extra signers, a fee bump's fee source; OP: an operation)
and a body its flags; finish() adds check_role and body_flags to the set.  The
builders of txaccounts_pool (edge_cases, random_pool) run on it unchanged;
assign() then gives their checks and bodies roles and flags from a generator of
its own.

fold() is the definition of include/stellar_sigverify.h restated over numpy
arrays: per body the first check whose check_ok != 1, the OR of check_used, the
mask of its min(ns, 64) signatures, and from these the code.  Nothing in it
comes from the code under test.
"""
import numpy as np

import txaccounts_pool as ap
import txbodies_pool as tp
import txpayload_pool as pl

OK, BAD_AUTH, OP_BAD_AUTH, BAD_AUTH_EXTRA = 0, 1, 2, 3
NONE = 0xFFFFFFFF
TX, OP = 0, 1
SKIP_UNUSED = 1


class RBody(ap.ABody):
    def __init__(self, kind, data):
        super().__init__(kind, data)
        self.roles, self.flags = [], 0

    def acheck(self, pos, level, needed=0, role=TX):
        self.roles.append(int(role))
        return super().acheck(pos, level, needed)


class RBuilder(ap.ABuilder):
    def body(self, kind=None, length=None):
        kind = int(self.rng.integers(0, 3)) if kind is None else kind
        length = int(self.rng.integers(0, 200)) if length is None else length
        b = RBody(kind, self.rng.integers(0, 256, length, dtype=np.uint8).tobytes())
        self.bodies.append(b)
        return b

    def finish(self, signer, oracle, layout_only=False):
        s = super().finish(signer, oracle, layout_only)
        s["check_role"] = np.array([r for b in self.bodies for r in b.roles], np.uint8).reshape(-1)
        s["body_flags"] = np.array([b.flags for b in self.bodies], np.uint8).reshape(-1)
        assert len(s["check_role"]) == s["nc"] and len(s["body_flags"]) == s["nb"]
        return s


def assign(bld, seed, first=0):
    """Random roles (about one in three OP) and flags (one body in four
    SKIP_UNUSED) for bodies first.. of the builder."""
    rng = np.random.default_rng(seed)
    for b in bld.bodies[first:]:
        b.roles = [int(rng.random() < 0.35) for _ in b.roles]
        b.flags = SKIP_UNUSED if rng.random() < 0.25 else 0


def fold(check_begin, sig_begin, check_ok, check_used, check_role=None, body_flags=None):
    """-> (body_code u8, body_fail u32) by the definition."""
    cb, sb = np.asarray(check_begin).astype(np.int64), np.asarray(sig_begin).astype(np.int64)
    nb = len(cb) - 1
    ok, used = np.asarray(check_ok), np.asarray(check_used, dtype=np.uint64)
    code, fail = np.zeros(nb, np.uint8), np.full(nb, NONE, np.uint32)
    for t in range(nb):
        c0, c1 = cb[t], cb[t + 1]
        bad = np.flatnonzero(ok[c0:c1] != 1)
        if len(bad):
            fail[t] = bad[0]
            role = TX if check_role is None else int(check_role[c0 + bad[0]])
            code[t] = BAD_AUTH if role == TX else OP_BAD_AUTH
            continue
        ns = min(int(sb[t + 1] - sb[t]), 64)
        want = (1 << ns) - 1
        marks = int(np.bitwise_or.reduce(used[c0:c1])) if c1 > c0 else 0
        flags = 0 if body_flags is None else int(body_flags[t])
        if (marks & want) != want and not flags & SKIP_UNUSED:
            code[t] = BAD_AUTH_EXTRA
    return code, fail


def bad_list(code, cap):
    """-> (the ascending failing bodies, at most cap of them; their exact count)."""
    bad = np.flatnonzero(np.asarray(code) != OK).astype(np.uint32)
    return bad[:cap], len(bad)


def args(s, **over):
    """Positional arguments of sv.decide_txbodies_accounts / _cpu; roles and flags go by keyword (kwargs())."""
    return ap.args(s, **over)


def kwargs(s, **more):
    kw = dict(sig_len=s["sig_len"], check_role=s["check_role"], body_flags=s["body_flags"])
    kw.update(more)
    return kw


def explicit(s):
    """... and of sv.decide_txbodies / _cpu over the Python expansion: (positional, keywords)."""
    a, kw = ap.explicit_args(s)
    kw.update(check_role=s["check_role"], body_flags=s["body_flags"])
    return a, kw


# ----------------------------------------------------------------- a body for each code
def code_cases(bld):
    """Adds one constructed body per rule to `bld`; returns {name: (body index,
    code, fail)} by hand.  Account `one` is seed 1's key alone (every level needs
    1), `two` seed 2's."""
    out = {}
    one, two = bld.account(ap.ed(1), (1, 1, 1, 1)), bld.account(ap.ed(2), (1, 1, 1, 1))

    def case(name, code, fail):
        out[name] = (len(bld.bodies), code, fail)
        return bld.body(length=int(bld.rng.integers(1, 90)))

    # the first failing check decides: TX before OP, then OP before TX (a passing check in front of both)
    b = case("tx_fails_before_op", BAD_AUTH, 1)
    p1, p2 = b.use(one), b.use(two)
    b.sig_ed(1)
    b.acheck(p1, 1, role=TX)
    b.acheck(p2, 1, role=TX)
    b.acheck(p2, 2, role=OP)
    b = case("op_fails_before_tx", OP_BAD_AUTH, 1)
    p1, p2 = b.use(one), b.use(two)
    b.sig_ed(1)
    b.acheck(p1, 1, role=TX)
    b.acheck(p2, 2, role=OP)
    b.acheck(p2, 1, role=TX)
    # an operation's failure with an unused signature: the failure, not EXTRA
    b = case("op_fails_with_unused_signature", OP_BAD_AUTH, 1)
    p1, p2 = b.use(one), b.use(two)
    b.sig_ed(1)
    b.sig_ed(3)
    b.acheck(p1, 1, role=TX)
    b.acheck(p2, 2, role=OP)
    # every check passes, one signature unused: EXTRA; with SKIP_UNUSED: OK
    for name, flags, code in (("unused_signature", 0, BAD_AUTH_EXTRA), ("unused_signature_skipped", SKIP_UNUSED, OK)):
        b = case(name, code, NONE)
        b.flags = flags
        p1 = b.use(one)
        b.sig_ed(1)
        b.sig_ed(3)
        b.acheck(p1, 1, role=TX)
        b.acheck(p1, 2, role=OP)
    # all used, over two checks: the OR of the marks
    b = case("used_over_two_checks", OK, NONE)
    p1, p2 = b.use(one), b.use(two)
    b.sig_ed(2)
    b.sig_ed(1)
    b.acheck(p1, 1, role=TX)
    b.acheck(p2, 2, role=OP)
    # no check: without a signature OK, with one EXTRA (a checker nobody asked anything)
    case("no_check_no_signature", OK, NONE)
    b = case("no_check_one_signature", BAD_AUTH_EXTRA, NONE)
    b.sig_ed(1)
    # 64 signatures, all used: the mask is ~0
    big = bld.account(ap.raw(bytes(32)), (0, 0, 0, 0), [(ap.ED, 1, ap.ed(100 + i)) for i in range(64)])
    b = case("sixty_four_signatures", OK, NONE)
    p = b.use(big)
    for i in range(64):
        b.sig_ed(100 + i)
    b.acheck(p, 0, 64, role=TX)
    # ... and the same with the last one not a signer's: bit 63 stays clear
    b = case("sixty_four_signatures_last_unused", BAD_AUTH_EXTRA, NONE)
    p = b.use(big)
    for i in range(63):
        b.sig_ed(100 + i)
    b.sig_ed(3)
    b.acheck(p, 0, 63, role=TX)
    return out
