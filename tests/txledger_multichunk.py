"""A multi-chunk host-buffer ledger call, run as a program by
test_gpu_txledger.py::test_multi_chunk_host_call with SV_STAGE_CHUNK=1024 in
the environment (the engine reads the staging chunk once per process).  One
store account and one local account are used by the first and by the last
body; the set expands to several times 1024 key rows, so the bodies between
them fill several chunks.  The host ledger form must equal the by-account twin
on the combined table -- its host form under the same chunking and its CPU
form.  Prints "multichunk ok"."""
import ctypes
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import torch  # noqa: E402,F401  (one HIP runtime per process)

import txaccounts_pool as ap  # noqa: E402
import txbodies_pool as tp  # noqa: E402
import txledger_pool as lp  # noqa: E402


def main():
    assert os.environ.get("SV_STAGE_CHUNK") == "1024"
    sv = importlib.import_module("stellar-core_amd")
    oracle = ctypes.CDLL(os.path.join(os.path.dirname(HERE), "oracle", "liboracle.so"))
    oracle.oracle_ed25519_verify.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    oracle.oracle_ed25519_sign.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    oracle.oracle_ed25519_seed_keypair.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    bld = lp.LBuilder(77)
    x = bld.account(ap.ed(31), (1, 1, 2, 2), [(lp.ED, 1, ap.ed(2))])
    n = bld.account(ap.ed(5), (1, 0, 0, 0), where=lp.LOCAL)

    def both_ends():
        b = bld.body(length=40)
        b.sig_ed(31)
        b.sig_ed(5)
        b.acheck(b.use(x), 1)
        b.acheck(b.use(n), 0, 0)

    both_ends()
    lp.random_pool(bld, 400, n_store=20, n_local=3, n_absent=2)
    both_ends()
    s = bld.finish(tp.device_signer(sv), oracle)
    lg = bld.ledger(s)
    assert s["nk"] + s["nq"] > 3 * 1024, (s["nk"], s["nq"])  # at least four chunks by the key bound alone
    sv.set_account_store(32, 20 * 20 + 8, lg["nl"])
    sv.account_store_upsert(**lp.batch(list(bld.model().items())))
    kw = dict(sig_len=s["sig_len"])
    want = sv.check_txbodies_accounts(*ap.args(s), device=0, **kw)
    cpu = sv.check_txbodies_accounts_cpu(*ap.args(s), **kw)
    got, found = sv.check_txbodies_ledger(*lp.args(s, lg), device=0, **kw)
    for g, w, c in zip(got, want, cpu):
        assert g.tobytes() == w.tobytes() == c.tobytes()
    assert (found == lg["found"]).all() and want[0].any() and not want[0].all()
    last = s["nc"] - 2
    assert want[0][:2].tolist() == [1, 1] and want[0][last:].tolist() == [1, 1]
    sv.set_account_store(0)
    print("multichunk ok")


if __name__ == "__main__":
    main()
