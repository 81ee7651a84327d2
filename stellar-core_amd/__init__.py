"""Python host binding of the MI355X ed25519 verification engine (stellar-core_amd).

The product is the C-ABI library ``libstellar_sigverify.so`` built in-tree from
``csrc/`` (see ``include/stellar_sigverify.h``).  This module is a thin ctypes
binding used by the tests and ``bench.py``; the C++ integration surface that
mirrors the reference interface (``stellar::PubKeyUtils::verifySig`` /
``verifySigBatch``, /root/reference/src/crypto/SecretKey.{h,cpp}) lives in
``csrc/host/``.

There is deliberately no CPU fallback here: if the HIP library is missing or
no device is present, every entry point raises.

Import it as ``importlib.import_module("stellar-core_amd")`` (the directory
name follows the repository layout contract; it is not a valid identifier).
"""
from __future__ import annotations

import collections
import ctypes
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstellar_sigverify.so")


VERIFY_KERNEL_SOURCES = ("sv_common.h", "fe25519.h", "fe_asm_gen.h", "ge25519.h", "sc25519.h", "lattice.h", "sha512_dev.h",
                         "verify_core.h", "quad.h", "sv_kparams.h", "sv_kernels.hip")

# kernel paths (include/stellar_sigverify.h)
PATH_AUTO, PATH_THROUGHPUT, PATH_LATENCY = 0, 1, 2


def kernel_source_digest() -> str:
    """SHA-256 over the verify kernel's device sources: ties profile-derived
    numbers (profiles/*_traffic.json) to the kernel they were measured on."""
    import hashlib
    h = hashlib.sha256()
    for name in VERIFY_KERNEL_SOURCES:
        h.update(name.encode())
        with open(os.path.join(_HERE, "csrc", name), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


HOSTLIB_PATH = os.path.join(_HERE, "libstellar_host.so")

SV_OK = 0
SV_ERRORS = {
    -1: "SV_ERR_INVALID_ARG",
    -2: "SV_ERR_NO_DEVICE",
    -3: "SV_ERR_HIP",
    -4: "SV_ERR_ALLOC",
    -5: "SV_ERR_NOT_INIT",
    -6: "SV_ERR_ALIGN",
    -7: "SV_ERR_KERNEL",
    -8: "SV_ERR_PAIR_CAP",
    -9: "SV_ERR_AUDIT",
}
SV_ERR_PAIR_CAP = -8
SV_ERR_AUDIT = -9

EXPORTED_SYMBOLS = (
    "sv_init", "sv_shutdown", "sv_device_count", "sv_last_error_string", "sv_version",
    "sv_ed25519_verify_batch", "sv_ed25519_verify_batch_fixed", "sv_ed25519_verify_device",
    "sv_ed25519_sign_device", "sv_timing_enable", "sv_kernel_time", "sv_kernel_time_reset",
    "sv_device_synchronize", "sv_verify_cache_keys", "sv_ed25519_verify_batch_keyed", "sv_sha256_batch",
    "sv_verify_cache_keys_device", "sv_sha256_device", "sv_set_kernel_path",
    "sv_ed25519_verify_batch_gather", "sv_ed25519_verify_batch_gather_cb", "sv_ed25519_verify_batch_cpu", "sv_ed25519_verify_cpu",
    "sv_set_device_map", "sv_set_min_shard", "sv_set_debug_flags", "sv_workspace_bytes", "sv_pinned_bytes",
    "sv_set_key_cache", "sv_key_cache_wait", "sv_key_cache_get_stats", "sv_set_key_tables",
    "sv_ed25519_verify_batch_gather_progress", "sv_host_feed_probe",
    "sv_ed25519_verify_txbodies", "sv_ed25519_verify_txbodies_device", "sv_ed25519_verify_txbodies_cpu",
    "sv_ed25519_verify_txbodies_hinted", "sv_ed25519_verify_txbodies_hinted_device",
    "sv_ed25519_verify_txbodies_hinted_cpu", "sv_txbodies_pair_bound",
    "sv_ed25519_check_txbodies", "sv_ed25519_check_txbodies_device", "sv_ed25519_check_txbodies_cpu",
    "sv_ed25519_check_txbodies_accounts", "sv_ed25519_check_txbodies_accounts_device",
    "sv_ed25519_check_txbodies_accounts_cpu",
    "sv_ed25519_decide_txbodies", "sv_ed25519_decide_txbodies_device", "sv_ed25519_decide_txbodies_cpu",
    "sv_ed25519_decide_txbodies_accounts", "sv_ed25519_decide_txbodies_accounts_device",
    "sv_ed25519_decide_txbodies_accounts_cpu",
    "sv_set_verdict_cache", "sv_verdict_cache_clear", "sv_verdict_cache_get_stats",
    "sv_ed25519_verify_device_cached",
    "sv_set_verdict_cache_feed", "sv_verdict_cache_sync", "sv_verdict_cache_lookup", "sv_verdict_cache_lookup_device",
    "sv_set_verdict_cache_share",
    "sv_set_account_store", "sv_account_store_upsert", "sv_account_store_erase", "sv_account_store_clear",
    "sv_account_store_get_stats", "sv_account_store_read",
    "sv_ed25519_check_txbodies_ledger", "sv_ed25519_decide_txbodies_ledger",
    "sv_ed25519_check_txbodies_ledger_device", "sv_ed25519_check_txbodies_ledger_cpu",
    "sv_ed25519_decide_txbodies_ledger_device", "sv_ed25519_decide_txbodies_ledger_cpu",
    "sv_ed25519_sign_batch", "sv_ed25519_sign_batch_device", "sv_ed25519_sign_batch_cpu",
    "sv_ed25519_sign_txbodies", "sv_ed25519_sign_txbodies_device", "sv_ed25519_sign_txbodies_cpu",
    "sv_set_audit", "sv_audit_get_stats", "sv_audit_read", "sv_audit_device", "sv_audit_batch_cpu",
)

# a bacct entry of the ledger forms that names a store account by its ID (include/stellar_sigverify.h)
BACCT_BY_ID = 0xFFFFFFFF
ACCT_MAX_SIGNERS = 20

# per-body result codes, check roles and body flags of the decide entry points (include/stellar_sigverify.h)
TXRESULT_OK, TXRESULT_BAD_AUTH, TXRESULT_OP_BAD_AUTH, TXRESULT_BAD_AUTH_EXTRA = 0, 1, 2, 3
TXRESULT_NONE = 0xFFFFFFFF
TXROLE_TX, TXROLE_OP = 0, 1
TXBODY_SKIP_UNUSED = 1

# signer key types of the check entry points (include/stellar_sigverify.h)
SIGNER_ED25519, SIGNER_PRE_AUTH_TX, SIGNER_HASH_X, SIGNER_SIGNED_PAYLOAD = 0, 1, 2, 3

# body kinds of the tx-body entry points (include/stellar_sigverify.h)
TXBODY_V1, TXBODY_V0, TXBODY_FEE_BUMP = 0, 1, 2

# test knobs (include/stellar_sigverify.h sv_set_debug_flags)
DBG_TRIVIAL_PAIR, DBG_MAX_WINDOWS, DBG_FAIL, DBG_PREP_ONLY, DBG_KEY_COLLIDE = 0x1, 0x2, 0x4, 0x8, 0x10
# throughput-path geometry: one signature per quad of lanes on every launch / never
DBG_QUAD, DBG_NO_QUAD = 0x20, 0x40
# three-wave cold octet: the tables' hand-over is dropped (its bounded wait runs out: every signature rejects)
DBG_DROP_HANDOVER = 0x80
# the audit kernel inverts its own verdict byte for the first picked row of every audited launch
DBG_AUDIT_DISSENT = 0x100


class SigVerifyError(RuntimeError):
    """A device/allocation error.  Never a reject: the batch is unverified.
    code: the SV_ERR_* value (None when raised by the binding itself);
    needed: for SV_ERR_PAIR_CAP, the exact number of pairs of the batch."""

    def __init__(self, message, code=None, needed=None):
        super().__init__(message)
        self.code = code
        self.needed = needed


class sv_opts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32),
                ("max_devices", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class sv_txchecks(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("protocol_version", ctypes.c_uint32),
                ("sig_len", ctypes.c_void_p), ("check_begin", ctypes.c_void_p), ("check_needed", ctypes.c_void_p),
                ("signer_begin", ctypes.c_void_p), ("signer_type", ctypes.c_void_p),
                ("signer_weight", ctypes.c_void_p), ("signer_key", ctypes.c_void_p),
                ("n_checks", ctypes.c_size_t), ("n_signers", ctypes.c_size_t),
                # sv_txchecks_payload: the same struct extended by the payload tables (read only when struct_size
                # covers them and pkey_begin is set)
                ("pkey_begin", ctypes.c_void_p), ("pkey", ctypes.c_void_p), ("pkey_payload", ctypes.c_void_p),
                ("pkey_len", ctypes.c_void_p), ("n_pkeys", ctypes.c_size_t)]


class sv_txaccounts(ctypes.Structure):
    _fields_ = ([("struct_size", ctypes.c_uint32), ("protocol_version", ctypes.c_uint32)]
                + [(f, ctypes.c_void_p) for f in (
                    "sig_len", "acct_key", "acct_thresholds", "asigner_begin", "asigner_type", "asigner_weight",
                    "asigner_key", "asigner_payload", "apayload", "apayload_len", "bacct_begin", "bacct",
                    "check_begin", "check_acct", "check_level", "check_needed")]
                + [(f, ctypes.c_size_t) for f in ("n_accounts", "n_asigners", "n_apayloads", "n_bacct", "n_checks")])


class sv_txledger(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("accts", ctypes.POINTER(sv_txaccounts)), ("bacct_id", ctypes.c_void_p),
                ("bacct_found", ctypes.c_void_p)]


class AccountStoreStats(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_uint64) for f in (
        "struct_size", "capacity", "accounts", "payload_capacity", "payloads", "local_accounts", "index_slots",
        "max_probe", "upsert_calls", "inserted", "replaced", "erase_calls", "erased", "erase_absent", "host_bytes",
        "device_bytes", "replica_current", "lookups")] + [("lookup_ms", ctypes.c_double)])


class sv_txresults(ctypes.Structure):
    _fields_ = ([("struct_size", ctypes.c_uint32)]
                + [(f, ctypes.c_void_p) for f in ("check_role", "body_flags", "body_code", "body_fail", "check_ok",
                                                  "check_weight", "check_used", "bad_body")]
                + [("bad_cap", ctypes.c_size_t), ("n_bad", ctypes.c_void_p)])


class FeedStats(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_uint32) for f in ("struct_size", "slots", "threads_per_slot", "usable_cpus")]
                + [("seconds", ctypes.c_double), ("gpu_numa", ctypes.c_int32 * 16),
                   ("staging_numa", ctypes.c_int32 * 16), ("pinned_cpus", ctypes.c_uint32 * 16)])


class KeyCacheStats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint64) for f in ("capacity", "keys", "warm_batches", "cold_batches", "keys_built",
                                                "evictions", "shared_launches", "table_launches", "table_keys",
                                                "table_clears", "table_slots")]


class VerdictCacheStats(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_uint64) for f in ("struct_size", "entries", "lookups", "hits", "inserted", "dropped",
                                                 "bytes")]
                + [("kernel_ms", ctypes.c_double), ("wait_ms", ctypes.c_double)]
                + [(f, ctypes.c_uint64) for f in ("fed_rows", "fed_overflow", "fed_present", "fed_inserted",
                                                  "fed_dropped")])


SHARED = ("shared_out", "shared_in", "shared_skipped", "shared_pinned_bytes")


class VerdictCacheShareStats(VerdictCacheStats):
    """sv_verdict_cache_stats as it stands now: VerdictCacheStats (the layout before sv_set_verdict_cache_share,
    which the engine still fills for a caller passing its size) with the shared_* fields behind it."""
    _fields_ = [(f, ctypes.c_uint64) for f in SHARED]


class AuditStats(ctypes.Structure):
    _fields_ = ([(f, ctypes.c_uint64) for f in ("struct_size", "what", "seq", "audited", "audited_rejects",
                                                 "over_budget", "mismatches", "records_lost", "records_held",
                                                 "lane_launches", "bytes")]
                + [("kernel_ms", ctypes.c_double)])


AUDIT_MSG_MAX, AUDIT_RING, AUDIT_BUDGET_MAX, AUDIT_REC_TRUNCATED = 512, 64, 1 << 22, 1


class AuditRecord(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_uint64), ("row", ctypes.c_uint64), ("msg_len", ctypes.c_uint32),
                ("engine_verdict", ctypes.c_uint8), ("audit_verdict", ctypes.c_uint8),
                ("cpu_verdict", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                ("pk", ctypes.c_uint8 * 32), ("sig", ctypes.c_uint8 * 64), ("msg", ctypes.c_uint8 * AUDIT_MSG_MAX)]


class AuditOpts(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint64), ("what", ctypes.c_uint32), ("one_in", ctypes.c_uint32),
                ("seed", ctypes.c_uint64), ("seq", ctypes.c_uint64), ("budget", ctypes.c_uint64)]


_lib: Optional[ctypes.CDLL] = None


def _share_hip_runtime_with_torch() -> None:
    # torch ships its own libamdhip64 (soname libamdhip64.so.7).  Importing it
    # first makes this library bind to that same runtime instead of loading a
    # second copy from /opt/rocm when torch is (or will be) in the process.
    if os.environ.get("SV_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise SigVerifyError(
            "libstellar_sigverify.so not built (%s); run __graft_entry__.build() "
            "or make -C stellar-core_amd" % path)
    _share_hip_runtime_with_torch()
    lib = ctypes.CDLL(path)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    lib.sv_init.restype = ctypes.c_int
    lib.sv_device_count.restype = ctypes.c_int
    lib.sv_last_error_string.restype = ctypes.c_char_p
    lib.sv_version.restype = ctypes.c_char_p
    lib.sv_ed25519_verify_batch.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp]
    lib.sv_ed25519_verify_batch_fixed.argtypes = [vp, vp, vp, ctypes.c_uint32, sz, vp, vp]
    lib.sv_ed25519_verify_device.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_uint32, sz, vp, vp, vp]
    lib.sv_ed25519_sign_device.argtypes = [ctypes.c_int, vp, vp, sz, vp, vp, vp]
    u32 = ctypes.c_uint32
    lib.sv_ed25519_sign_batch.argtypes = [vp, sz, vp, vp, vp, vp, u32, sz, vp, vp, vp]
    lib.sv_ed25519_sign_batch_device.argtypes = [ctypes.c_int, vp, sz, vp, vp, vp, vp, u32, sz, vp, vp, vp]
    lib.sv_ed25519_sign_batch_cpu.argtypes = [vp, sz, vp, vp, vp, vp, u32, sz, vp, vp, ctypes.c_int]
    lib.sv_ed25519_sign_txbodies.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp, vp]
    lib.sv_ed25519_sign_txbodies_device.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp,
                                                    vp, vp, vp]
    lib.sv_ed25519_sign_txbodies_cpu.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp,
                                                 ctypes.c_int]
    lib.sv_timing_enable.argtypes = [ctypes.c_int]
    lib.sv_kernel_time.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.sv_device_synchronize.argtypes = [ctypes.c_int]
    lib.sv_verify_cache_keys.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp]
    lib.sv_ed25519_verify_batch_keyed.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp]
    lib.sv_sha256_batch.argtypes = [vp, vp, vp, sz, vp, vp]
    lib.sv_verify_cache_keys_device.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_uint32, sz, vp, vp]
    lib.sv_sha256_device.argtypes = [ctypes.c_int, vp, vp, vp, ctypes.c_uint32, sz, vp, vp]
    lib.sv_ed25519_verify_batch_gather.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp]
    lib.sv_ed25519_verify_batch_cpu.argtypes = [vp, vp, vp, vp, vp, sz, vp, ctypes.c_int]
    lib.sv_ed25519_verify_cpu.argtypes = [vp, vp, vp, sz]
    lib.sv_set_device_map.argtypes = [vp, ctypes.c_int]
    lib.sv_set_min_shard.argtypes = [sz]
    lib.sv_set_debug_flags.argtypes = [ctypes.c_uint32]
    lib.sv_workspace_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    lib.sv_pinned_bytes.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_size_t)]
    lib.sv_set_key_cache.argtypes = [sz]
    lib.sv_set_key_tables.argtypes = [ctypes.c_int, sz]
    lib.sv_key_cache_wait.argtypes = [ctypes.c_int]
    lib.sv_key_cache_get_stats.argtypes = [ctypes.c_int, ctypes.POINTER(KeyCacheStats)]
    lib.sv_set_verdict_cache.argtypes = [sz]
    lib.sv_verdict_cache_get_stats.argtypes = [ctypes.c_int, ctypes.POINTER(VerdictCacheStats)]
    lib.sv_ed25519_verify_device_cached.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, ctypes.c_uint32, sz, vp, vp,
                                                    vp, vp, vp]
    lib.sv_set_verdict_cache_feed.argtypes = [ctypes.c_uint32, sz]
    lib.sv_set_verdict_cache_share.argtypes = [ctypes.c_uint32]
    lib.sv_verdict_cache_sync.argtypes = [ctypes.c_int]
    lib.sv_verdict_cache_lookup.argtypes = [ctypes.c_int, vp, sz, vp]
    lib.sv_verdict_cache_lookup_device.argtypes = [ctypes.c_int, vp, sz, vp, vp]
    lib.sv_set_audit.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, sz]
    lib.sv_audit_get_stats.argtypes = [ctypes.c_int, vp]
    lib.sv_audit_read.argtypes = [ctypes.c_int, vp, sz, ctypes.POINTER(ctypes.c_size_t)]
    lib.sv_audit_device.argtypes = [ctypes.c_int, ctypes.POINTER(AuditOpts), vp, vp, vp, vp, vp, ctypes.c_uint32, sz,
                                    vp, vp]
    lib.sv_audit_batch_cpu.argtypes = [ctypes.POINTER(AuditOpts), vp, vp, vp, vp, vp, ctypes.c_uint32, sz, vp, vp, vp,
                                       sz, ctypes.POINTER(ctypes.c_size_t), ctypes.c_int]
    lib.sv_lat_last_trace.argtypes = [ctypes.POINTER(ctypes.c_double)]
    lib.sv_host_feed_probe.argtypes = [vp, vp, vp, ctypes.c_uint32, sz, ctypes.c_uint32, ctypes.c_int,
                                       ctypes.POINTER(FeedStats)]
    lib.sv_ed25519_verify_txbodies.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp]
    lib.sv_ed25519_verify_txbodies_device.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, vp,
                                                      vp, vp]
    lib.sv_ed25519_verify_txbodies_cpu.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, ctypes.c_int]
    szp = ctypes.POINTER(ctypes.c_size_t)
    hinted = [vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp]
    lib.sv_ed25519_verify_txbodies_hinted.argtypes = hinted + [szp, vp, vp]
    lib.sv_ed25519_verify_txbodies_hinted_cpu.argtypes = hinted + [szp, vp, ctypes.c_int]
    lib.sv_ed25519_verify_txbodies_hinted_device.argtypes = [ctypes.c_int] + hinted + [vp, szp, vp, vp]
    lib.sv_txbodies_pair_bound.argtypes = [vp, vp, sz]
    checked = [vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, vp, vp, sz, ctypes.POINTER(sv_txchecks), vp, vp, vp, vp]
    lib.sv_ed25519_check_txbodies.argtypes = checked + [vp]
    lib.sv_ed25519_check_txbodies_cpu.argtypes = checked + [ctypes.c_int]
    lib.sv_ed25519_check_txbodies_device.argtypes = [ctypes.c_int] + checked + [vp]
    lib.sv_txbodies_pair_bound.restype = sz
    by_acct = [vp, vp, vp, vp, vp, sz, vp, vp, vp, sz, ctypes.POINTER(sv_txaccounts), vp, vp, vp, vp]
    lib.sv_ed25519_check_txbodies_accounts.argtypes = by_acct + [vp]
    lib.sv_ed25519_check_txbodies_accounts_cpu.argtypes = by_acct + [ctypes.c_int]
    lib.sv_ed25519_check_txbodies_accounts_device.argtypes = [ctypes.c_int] + by_acct + [vp]
    # the decide forms: const sv_txresults* in place of the three check outputs
    resp = ctypes.POINTER(sv_txresults)
    decided = checked[:-4] + [resp, vp]
    lib.sv_ed25519_decide_txbodies.argtypes = decided + [vp]
    lib.sv_ed25519_decide_txbodies_cpu.argtypes = decided + [ctypes.c_int]
    lib.sv_ed25519_decide_txbodies_device.argtypes = [ctypes.c_int] + decided + [vp]
    decided_acct = by_acct[:-4] + [resp, vp]
    lib.sv_ed25519_decide_txbodies_accounts.argtypes = decided_acct + [vp]
    lib.sv_ed25519_decide_txbodies_accounts_cpu.argtypes = decided_acct + [ctypes.c_int]
    lib.sv_ed25519_decide_txbodies_accounts_device.argtypes = [ctypes.c_int] + decided_acct + [vp]
    by_ledger = by_acct[:10] + [ctypes.POINTER(sv_txledger)] + by_acct[11:]
    lib.sv_ed25519_check_txbodies_ledger.argtypes = by_ledger + [vp]
    lib.sv_ed25519_check_txbodies_ledger_cpu.argtypes = by_ledger + [ctypes.c_int]
    lib.sv_ed25519_check_txbodies_ledger_device.argtypes = [ctypes.c_int] + by_ledger + [vp]
    decided_ledger = by_ledger[:-4] + [resp, vp]
    lib.sv_ed25519_decide_txbodies_ledger.argtypes = decided_ledger + [vp]
    lib.sv_ed25519_decide_txbodies_ledger_cpu.argtypes = decided_ledger + [ctypes.c_int]
    lib.sv_ed25519_decide_txbodies_ledger_device.argtypes = [ctypes.c_int] + decided_ledger + [vp]
    lib.sv_set_account_store.argtypes = [sz, sz, sz]
    lib.sv_account_store_upsert.argtypes = [ctypes.POINTER(sv_txaccounts)]
    lib.sv_account_store_erase.argtypes = [vp, sz]
    lib.sv_account_store_get_stats.argtypes = [ctypes.c_int, ctypes.POINTER(AccountStoreStats)]
    lib.sv_account_store_read.argtypes = [ctypes.c_int, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.sv_txresult_block.restype = ctypes.c_int
    lib.sv_txresult_ws_bytes.argtypes = [ctypes.c_uint64]
    lib.sv_txresult_ws_bytes.restype = sz
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != SV_OK:
        msg = _lib.sv_last_error_string().decode(errors="replace") if _lib else ""
        raise SigVerifyError("%s: %s" % (SV_ERRORS.get(rc, rc), msg), code=rc)


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    # (__array_interface__ is several times cheaper than a.ctypes.data: the
    # 1k-batch latency path pays this per array)
    return ctypes.c_void_p(a.__array_interface__["data"][0])


# sv_opts.flags kernel-path requests (include/stellar_sigverify.h)
FLAG_PATH = {None: 0, "auto": 0, "throughput": 0x1, "latency": 0x2}


def _opts(device: int = -1, max_devices: int = 0, path=None):
    o = sv_opts(ctypes.sizeof(sv_opts), device, max_devices, FLAG_PATH[path] if isinstance(path, (str, type(None)))
                else int(path))
    return ctypes.byref(o)


def device_count() -> int:
    lib = load_library()
    n = lib.sv_device_count()
    if n < 0:
        _check(n)
    return n


def version() -> str:
    return load_library().sv_version().decode()


def _u8(a, shape_tail: int) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
    return a.reshape(-1, shape_tail)


def verify_batch(pk, sig, msg, msg_off, msg_len, device: int = -1, max_devices: int = 0, path=None) -> np.ndarray:
    """Variable-length batch: message i = msg[msg_off[i]:msg_off[i]+msg_len[i]].

    Returns a uint8 verdict array (1 = valid), bit-identical to libsodium's
    crypto_sign_verify_detached on every row.  path: None / "auto",
    "throughput" or "latency" (sv_opts.flags; verdicts are identical)."""
    lib = load_library()
    pk = _u8(pk, 32)
    sig = _u8(sig, 64)
    n = pk.shape[0]
    if sig.shape[0] != n:
        raise ValueError("pk/sig row mismatch")
    msg = np.ascontiguousarray(np.asarray(msg, dtype=np.uint8).reshape(-1))
    if msg.size == 0:
        msg = np.zeros(1, np.uint8)
    off = np.ascontiguousarray(np.asarray(msg_off, dtype=np.uint64))
    ln = np.ascontiguousarray(np.asarray(msg_len, dtype=np.uint32))
    if off.shape[0] != n or ln.shape[0] != n:
        raise ValueError("msg_off/msg_len length mismatch")
    if n and int((off + ln).max()) > msg.size:
        raise ValueError("message range out of bounds")
    out = np.zeros(n, np.uint8)
    _check(lib.sv_ed25519_verify_batch(_ptr(pk), _ptr(sig), _ptr(msg), _ptr(off), _ptr(ln), n, _ptr(out),
                                       _opts(device, max_devices, path)))
    return out


def _var_msgs(msg, msg_off, msg_len, n):
    msg = np.ascontiguousarray(np.asarray(msg, dtype=np.uint8).reshape(-1))
    if msg.size == 0:
        msg = np.zeros(1, np.uint8)
    off = np.ascontiguousarray(np.asarray(msg_off, dtype=np.uint64))
    ln = np.ascontiguousarray(np.asarray(msg_len, dtype=np.uint32))
    if off.shape[0] != n or ln.shape[0] != n:
        raise ValueError("msg_off/msg_len length mismatch")
    if n and int((off + ln).max()) > msg.size:
        raise ValueError("message range out of bounds")
    return msg, off, ln


def cache_keys(pk, sig, msg, msg_off, msg_len, device: int = -1, max_devices: int = 0) -> np.ndarray:
    """n x 32 verify-cache keys BLAKE2b-256(pk || sig || msg) computed on the GPU
    (SecretKey.cpp:50-61), SURVEY §8 f4."""
    lib = load_library()
    pk, sig = _u8(pk, 32), _u8(sig, 64)
    n = pk.shape[0]
    msg, off, ln = _var_msgs(msg, msg_off, msg_len, n)
    keys = np.zeros((n, 32), np.uint8)
    _check(lib.sv_verify_cache_keys(_ptr(pk), _ptr(sig), _ptr(msg), _ptr(off), _ptr(ln), n, _ptr(keys),
                                    _opts(device, max_devices)))
    return keys


def verify_batch_keyed(pk, sig, msg, msg_off, msg_len, device: int = -1, max_devices: int = 0):
    """(verdicts, cache keys) from one staging of the batch."""
    lib = load_library()
    pk, sig = _u8(pk, 32), _u8(sig, 64)
    n = pk.shape[0]
    msg, off, ln = _var_msgs(msg, msg_off, msg_len, n)
    out = np.zeros(n, np.uint8)
    keys = np.zeros((n, 32), np.uint8)
    _check(lib.sv_ed25519_verify_batch_keyed(_ptr(pk), _ptr(sig), _ptr(msg), _ptr(off), _ptr(ln), n, _ptr(out),
                                             _ptr(keys), _opts(device, max_devices)))
    return out, keys


def sha256_batch(data, off, length, device: int = -1, max_devices: int = 0) -> np.ndarray:
    """n x 32 SHA-256 digests of data[off[i]:off[i]+length[i]] on the GPU
    (batch tx contents hashes, TransactionFrame.cpp:90-117), SURVEY §8 f4."""
    lib = load_library()
    n = len(off)
    data, o, ln = _var_msgs(data, off, length, n)
    out = np.zeros((n, 32), np.uint8)
    _check(lib.sv_sha256_batch(_ptr(data), _ptr(o), _ptr(ln), n, _ptr(out), _opts(device, max_devices)))
    return out


def verify_messages(pk, sig, messages: Sequence[bytes], **kw) -> np.ndarray:
    lens = np.array([len(m) for m in messages], np.uint32)
    off = np.zeros(len(messages), np.uint64)
    if len(messages) > 1:
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    buf = np.frombuffer(b"".join(messages), np.uint8) if messages else np.zeros(0, np.uint8)
    return verify_batch(pk, sig, buf, off, lens, **kw)


def verify_fixed(pk, sig, msg, msg_len: int = 32, device: int = -1, max_devices: int = 0, path=None) -> np.ndarray:
    """Fixed-length batch (msg is n x msg_len bytes); msg_len 32 = tx contents hashes."""
    lib = load_library()
    pk = _u8(pk, 32)
    sig = _u8(sig, 64)
    n = pk.shape[0]
    msg = np.ascontiguousarray(np.asarray(msg, dtype=np.uint8).reshape(-1))
    if msg.size != n * msg_len:
        raise ValueError("msg must hold n * msg_len bytes")
    if msg.size == 0:
        msg = np.zeros(1, np.uint8)
    out = np.zeros(n, np.uint8)
    _check(lib.sv_ed25519_verify_batch_fixed(_ptr(pk), _ptr(sig), _ptr(msg), msg_len, n, _ptr(out),
                                             _opts(device, max_devices, path)))
    return out


def verify_device(device: int, d_pk: int, d_sig: int, d_msg: int, n: int, d_verdict: int,
                  d_bitmap: int = 0, stream: int = 0, fixed_msg_len: int = 32,
                  d_msg_off: int = 0, d_msg_len: int = 0) -> None:
    """Device-resident batch (raw device pointers, e.g. torch tensor data_ptr())."""
    lib = load_library()
    _check(lib.sv_ed25519_verify_device(device, d_pk, d_sig, d_msg, d_msg_off or None, d_msg_len or None,
                                        fixed_msg_len, n, d_verdict, d_bitmap or None, stream or None))


def sign_device(device: int, d_seed: int, d_msg32: int, n: int, d_pk: int, d_sig: int, stream: int = 0) -> None:
    lib = load_library()
    _check(lib.sv_ed25519_sign_device(device, d_seed, d_msg32, n, d_pk, d_sig, stream or None))


def _sign_args(seed, msg, msg_off, msg_len, key_of, fixed_msg_len):
    seed = _u8(seed, 32)
    k = seed.shape[0]
    if key_of is None:
        n, ko = k, None
    else:
        ko = np.ascontiguousarray(np.asarray(key_of, dtype=np.uint32).reshape(-1))
        n = ko.shape[0]
    if fixed_msg_len:
        msg = np.ascontiguousarray(np.asarray(msg, dtype=np.uint8).reshape(-1))
        if msg.size != n * fixed_msg_len:
            raise ValueError("msg must hold n * fixed_msg_len bytes")
        if msg.size == 0:
            msg = np.zeros(1, np.uint8)
        off = ln = None
    else:
        msg, off, ln = _var_msgs(msg, msg_off, msg_len, n)
    return seed, k, ko, msg, off, ln, n


def _optr(a):
    return None if a is None else _ptr(a)


def sign_batch(seed, msg, msg_off=None, msg_len=None, key_of=None, fixed_msg_len: int = 0, device: int = -1):
    """Batch ed25519 signing on the GPU (sv_ed25519_sign_batch): seed is k x 32,
    message i (msg[msg_off[i]:msg_off[i]+msg_len[i]], or row i of n x fixed_msg_len
    bytes) is signed with seed[key_of[i]] (key_of None: k == n, key i signs
    message i).  Returns (sig n x 64, pk k x 32), byte-equal to libsodium's
    crypto_sign_detached / crypto_sign_seed_keypair.  Not constant-time: for load
    generation, test networks, benchmarks and datasets."""
    lib = load_library()
    seed, k, ko, msg, off, ln, n = _sign_args(seed, msg, msg_off, msg_len, key_of, fixed_msg_len)
    sig = np.zeros((n, 64), np.uint8)
    pk = np.zeros((k, 32), np.uint8)
    _check(lib.sv_ed25519_sign_batch(_ptr(seed), k, _optr(ko), _ptr(msg), _optr(off), _optr(ln), fixed_msg_len, n,
                                     _ptr(sig), _ptr(pk), _opts(device)))
    return sig, pk


def sign_batch_cpu(seed, msg, msg_off=None, msg_len=None, key_of=None, fixed_msg_len: int = 0, threads: int = 0):
    """The same on the engine's CPU path (what a caller runs on an engine error)."""
    lib = load_library()
    seed, k, ko, msg, off, ln, n = _sign_args(seed, msg, msg_off, msg_len, key_of, fixed_msg_len)
    sig = np.zeros((n, 64), np.uint8)
    pk = np.zeros((k, 32), np.uint8)
    _check(lib.sv_ed25519_sign_batch_cpu(_ptr(seed), k, _optr(ko), _ptr(msg), _optr(off), _optr(ln), fixed_msg_len, n,
                                         _ptr(sig), _ptr(pk), int(threads)))
    return sig, pk


def sign_batch_device(device: int, d_seed: int, k: int, d_msg: int, n: int, d_sig: int, d_pk: int = 0,
                      d_key_of: int = 0, fixed_msg_len: int = 32, d_msg_off: int = 0, d_msg_len: int = 0,
                      stream: int = 0) -> None:
    """Device-resident form (raw device pointers; seed / sig / pk 16-byte aligned)."""
    lib = load_library()
    _check(lib.sv_ed25519_sign_batch_device(device, d_seed or None, k, d_key_of or None, d_msg or None,
                                            d_msg_off or None, d_msg_len or None, fixed_msg_len, n, d_sig or None,
                                            d_pk or None, stream or None))


def _sign_tx_args(network_id, bodies, body_off, body_len, body_kind, sig_begin, seed, key_of):
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    kind = np.ascontiguousarray(np.asarray(body_kind, dtype=np.uint8).reshape(-1))
    nb = kind.shape[0]
    bodies, off, ln = _var_msgs(bodies, body_off, body_len, nb)
    sb = _csr(sig_begin, nb, "sig_begin")
    seed = _u8(seed, 32)
    ko = np.ascontiguousarray(np.asarray(key_of, dtype=np.uint32).reshape(-1))
    return nid, bodies, off, ln, kind, nb, sb, seed, seed.shape[0], ko, ko.shape[0]


def _sign_tx_host(fn, last, network_id, bodies, body_off, body_len, body_kind, sig_begin, seed, key_of):
    nid, bodies, off, ln, kind, nb, sb, seed, k, ko, n = _sign_tx_args(network_id, bodies, body_off, body_len,
                                                                      body_kind, sig_begin, seed, key_of)
    hint = np.zeros((n, 4), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    pk = np.zeros((k, 32), np.uint8)
    dig = np.zeros((nb, 32), np.uint8)
    kp = np.zeros(max(n, 1), np.uint32)
    kp[:n] = ko
    _check(fn(_ptr(nid), _ptr(bodies), _ptr(off), _ptr(ln), _ptr(kind), nb, _ptr(sb), _ptr(seed), k, _ptr(kp), n,
              _ptr(hint), _ptr(sig), _ptr(pk), _ptr(dig), last))
    return hint, sig, pk, dig


def sign_txbodies(network_id, bodies, body_off, body_len, body_kind, sig_begin, seed, key_of, device: int = -1):
    """What SignatureUtils::sign produces per (transaction, key), on the GPU
    (sv_ed25519_sign_txbodies): signature s of body t is made with seed[key_of[s]]
    over the body's contents hash.  Returns (hint n x 4, sig n x 64, pk k x 32,
    digests n_bodies x 32); sig_begin, hint and sig feed verify_txbodies_hinted."""
    return _sign_tx_host(load_library().sv_ed25519_sign_txbodies, _opts(device), network_id, bodies, body_off,
                         body_len, body_kind, sig_begin, seed, key_of)


def sign_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, seed, key_of, threads: int = 0):
    """The same on the engine's CPU path."""
    return _sign_tx_host(load_library().sv_ed25519_sign_txbodies_cpu, int(threads), network_id, bodies, body_off,
                         body_len, body_kind, sig_begin, seed, key_of)


def sign_txbodies_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int, d_body_kind: int,
                         n_bodies: int, d_sig_begin: int, d_seed: int, k: int, d_key_of: int, n: int, d_hint: int,
                         d_sig: int, d_pk: int = 0, d_digests: int = 0, stream: int = 0) -> None:
    """Device-resident form (raw device pointers; network_id is 32 host bytes)."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    _check(lib.sv_ed25519_sign_txbodies_device(device, _ptr(nid), d_bodies or None, d_body_off or None,
                                               d_body_len or None, d_body_kind or None, n_bodies, d_sig_begin or None,
                                               d_seed or None, k, d_key_of or None, n, d_hint or None, d_sig or None,
                                               d_pk or None, d_digests or None, stream or None))


def verify_batch_cpu(pk, sig, msg, msg_off, msg_len, threads: int = 0) -> np.ndarray:
    """The engine's CPU path (same algorithm, host build): what a caller runs
    when a GPU entry point fails, and what single verifySig calls use."""
    lib = load_library()
    pk, sig = _u8(pk, 32), _u8(sig, 64)
    n = pk.shape[0]
    msg, off, ln = _var_msgs(msg, msg_off, msg_len, n)
    out = np.zeros(n, np.uint8)
    _check(lib.sv_ed25519_verify_batch_cpu(_ptr(pk), _ptr(sig), _ptr(msg), _ptr(off), _ptr(ln), n, _ptr(out),
                                           int(threads)))
    return out


def _txbodies_args(network_id, bodies, body_off, body_len, body_kind, sig_begin, pk, sig):
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    pk, sig = _u8(pk, 32), _u8(sig, 64)
    n = pk.shape[0]
    if sig.shape[0] != n:
        raise ValueError("pk/sig row mismatch")
    kind = np.ascontiguousarray(np.asarray(body_kind, dtype=np.uint8).reshape(-1))
    nb = kind.shape[0]
    bodies, off, ln = _var_msgs(bodies, body_off, body_len, nb)
    sb = np.ascontiguousarray(np.asarray(sig_begin, dtype=np.uint64).reshape(-1))
    if sb.shape[0] != nb + 1:
        raise ValueError("sig_begin must hold n_bodies + 1 entries")
    return nid, bodies, off, ln, kind, nb, sb, pk, sig, n


def verify_txbodies(network_id, bodies, body_off, body_len, body_kind, sig_begin, pk, sig, device: int = -1,
                    max_devices: int = 0, path=None):
    """Signatures straight from transaction bodies (sv_ed25519_verify_txbodies):
    body t = bodies[body_off[t]:body_off[t]+body_len[t]] of kind body_kind[t]
    (TXBODY_V1 / TXBODY_V0 / TXBODY_FEE_BUMP) owns signatures
    sig_begin[t]..sig_begin[t+1]-1.  The GPU hashes the bodies and verifies the
    signatures over the digests in one pass.  Returns (verdict, digests)."""
    lib = load_library()
    nid, bodies, off, ln, kind, nb, sb, pk, sig, n = _txbodies_args(network_id, bodies, body_off, body_len, body_kind,
                                                                   sig_begin, pk, sig)
    out = np.zeros(n, np.uint8)
    dig = np.zeros((nb, 32), np.uint8)
    _check(lib.sv_ed25519_verify_txbodies(_ptr(nid), _ptr(bodies), _ptr(off), _ptr(ln), _ptr(kind), nb, _ptr(sb),
                                          _ptr(pk), _ptr(sig), n, _ptr(out), _ptr(dig),
                                          _opts(device, max_devices, path)))
    return out, dig


def verify_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, pk, sig, threads: int = 0):
    """The same on the engine's CPU path (what a caller runs on an engine error)."""
    lib = load_library()
    nid, bodies, off, ln, kind, nb, sb, pk, sig, n = _txbodies_args(network_id, bodies, body_off, body_len, body_kind,
                                                                   sig_begin, pk, sig)
    out = np.zeros(n, np.uint8)
    dig = np.zeros((nb, 32), np.uint8)
    _check(lib.sv_ed25519_verify_txbodies_cpu(_ptr(nid), _ptr(bodies), _ptr(off), _ptr(ln), _ptr(kind), nb, _ptr(sb),
                                              _ptr(pk), _ptr(sig), n, _ptr(out), _ptr(dig), int(threads)))
    return out, dig


def verify_txbodies_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int, d_body_kind: int,
                           n_bodies: int, d_sig_begin: int, d_pk: int, d_sig: int, n: int, d_verdict: int,
                           d_bitmap: int = 0, d_digests: int = 0, stream: int = 0) -> None:
    """Device-resident form (raw device pointers; network_id is 32 host bytes).
    The verdicts and digests land in d_verdict (n) / d_digests (n_bodies x 32)."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    _check(lib.sv_ed25519_verify_txbodies_device(device, _ptr(nid), d_bodies or None, d_body_off or None,
                                                 d_body_len or None, d_body_kind or None, n_bodies,
                                                 d_sig_begin or None, d_pk or None, d_sig or None, n,
                                                 d_verdict or None, d_bitmap or None, d_digests or None,
                                                 stream or None))


def _csr(a, nb, what):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1))
    if a.shape[0] != nb + 1:
        raise ValueError("%s must hold n_bodies + 1 entries" % what)
    return a


def txbodies_pair_bound(sig_begin, key_begin) -> int:
    """Sum over the bodies of signatures x keys (sv_txbodies_pair_bound): a
    pair_cap that always suffices."""
    lib = load_library()
    sb = np.ascontiguousarray(np.asarray(sig_begin, dtype=np.uint64).reshape(-1))
    kb = _csr(key_begin, sb.shape[0] - 1, "key_begin")
    return int(lib.sv_txbodies_pair_bound(_ptr(sb), _ptr(kb), sb.shape[0] - 1))


def _hinted_args(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key):
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    hint, sig, key = _u8(hint, 4), _u8(sig, 64), _u8(key, 32)
    ns, nk = sig.shape[0], key.shape[0]
    if hint.shape[0] != ns:
        raise ValueError("hint/sig row mismatch")
    kind = np.ascontiguousarray(np.asarray(body_kind, dtype=np.uint8).reshape(-1))
    nb = kind.shape[0]
    bodies, off, ln = _var_msgs(bodies, body_off, body_len, nb)
    sb, kb = _csr(sig_begin, nb, "sig_begin"), _csr(key_begin, nb, "key_begin")
    for name, a, n in (("sig_begin", sb, ns), ("key_begin", kb, nk)):
        if int(a[0]) != 0 or int(a[-1]) != n or (a[1:] < a[:-1]).any():
            raise ValueError("%s must start at 0, not decrease and end at the row count" % name)
    return nid, bodies, off, ln, kind, nb, sb, hint, sig, ns, kb, key, nk


def _check_pairs(rc: int, n_pairs) -> None:
    if rc == SV_ERR_PAIR_CAP:
        msg = _lib.sv_last_error_string().decode(errors="replace") if _lib else ""
        raise SigVerifyError("SV_ERR_PAIR_CAP: %s (the batch has %d pairs)" % (msg, n_pairs.value), rc,
                             int(n_pairs.value))
    _check(rc)


def _hinted_host(fn, last, network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                 pair_cap):
    nid, bodies, off, ln, kind, nb, sb, hint, sig, ns, kb, key, nk = _hinted_args(
        network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key)
    lib = load_library()
    cap = int(lib.sv_txbodies_pair_bound(_ptr(sb), _ptr(kb), nb)) if pair_cap is None else int(pair_cap)
    pb = np.zeros(nb + 1, np.uint64)
    ps, pk = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    pv = np.zeros(cap, np.uint8)
    dig = np.zeros((nb, 32), np.uint8)
    n_pairs = ctypes.c_size_t(0)
    none = None if cap == 0 else 1
    rc = fn(_ptr(nid), _ptr(bodies), _ptr(off), _ptr(ln), _ptr(kind), nb, _ptr(sb), _ptr(hint), _ptr(sig), ns,
            _ptr(kb), _ptr(key), nk, cap, _ptr(pb), none and _ptr(ps), none and _ptr(pk), none and _ptr(pv),
            ctypes.byref(n_pairs), _ptr(dig), last)
    _check_pairs(rc, n_pairs)
    n = int(n_pairs.value)
    return pb, ps[:n], pk[:n], pv[:n], dig


def verify_txbodies_hinted(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                           pair_cap=None, device: int = -1, max_devices: int = 0, path=None):
    """Pairing by hint on the device (sv_ed25519_verify_txbodies_hinted): body t
    owns the decorated signatures sig_begin[t]..sig_begin[t+1]-1 (hint n x 4,
    sig n x 64) and the candidate keys key_begin[t]..key_begin[t+1]-1 (key
    m x 32).  Returns (pair_begin, pair_sig, pair_key, pair_verdict, digests):
    the hint-matching pairs in (body, signature, key) order with the engine's
    verdict over the body's contents hash.  The outputs are sized by
    txbodies_pair_bound unless pair_cap is given; more pairs than pair_cap
    raise SigVerifyError with .needed set to the exact count."""
    lib = load_library()
    return _hinted_host(lib.sv_ed25519_verify_txbodies_hinted, _opts(device, max_devices, path), network_id, bodies,
                        body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key, pair_cap)


def verify_txbodies_hinted_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                               pair_cap=None, threads: int = 0):
    """The same on the engine's CPU path (what a caller runs on an engine error)."""
    lib = load_library()
    return _hinted_host(lib.sv_ed25519_verify_txbodies_hinted_cpu, int(threads), network_id, bodies, body_off,
                        body_len, body_kind, sig_begin, hint, sig, key_begin, key, pair_cap)


def verify_txbodies_hinted_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int,
                                  d_body_kind: int, n_bodies: int, d_sig_begin: int, d_hint: int, d_sig: int,
                                  n_sigs: int, d_key_begin: int, d_key: int, n_keys: int, pair_cap: int,
                                  d_pair_begin: int, d_pair_sig: int, d_pair_key: int, d_pair_verdict: int,
                                  d_pair_bitmap: int = 0, d_digests: int = 0, stream: int = 0) -> int:
    """Device-resident form (raw device pointers; network_id is 32 host bytes).
    Waits on `stream` once for the pair count, enqueues the verification and
    returns the number of pairs; the results land in the d_pair_* arrays."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    n_pairs = ctypes.c_size_t(0)
    rc = lib.sv_ed25519_verify_txbodies_hinted_device(
        device, _ptr(nid), d_bodies or None, d_body_off or None, d_body_len or None, d_body_kind or None, n_bodies,
        d_sig_begin or None, d_hint or None, d_sig or None, n_sigs, d_key_begin or None, d_key or None, n_keys,
        pair_cap, d_pair_begin or None, d_pair_sig or None, d_pair_key or None, d_pair_verdict or None,
        d_pair_bitmap or None, ctypes.byref(n_pairs), d_digests or None, stream or None)
    _check_pairs(rc, n_pairs)
    return int(n_pairs.value)


TxResults = collections.namedtuple(
    "TxResults", "body_code body_fail bad_body n_bad check_ok check_weight check_used digests")


def results_desc(check_role=0, body_flags=0, body_code=0, body_fail=0, check_ok=0, check_weight=0, check_used=0,
                 bad_body=0, bad_cap=0, n_bad=0, struct_size=None):
    """sv_txresults over raw addresses (host arrays' or device pointers; 0: NULL)."""
    r = sv_txresults()
    r.struct_size = ctypes.sizeof(sv_txresults) if struct_size is None else int(struct_size)
    for name, v in (("check_role", check_role), ("body_flags", body_flags), ("body_code", body_code),
                    ("body_fail", body_fail), ("check_ok", check_ok), ("check_weight", check_weight),
                    ("check_used", check_used), ("bad_body", bad_body), ("n_bad", n_bad)):
        setattr(r, name, v or None)
    r.bad_cap = int(bad_cap)
    return r


def _checked_call(fn, head, nb, nc, last, results):
    """The tail of a host check or decide call: head are the arguments up to the
    table struct.  results None: a check call, (check_ok, check_weight,
    check_used, digests).  Else a decide call: an sv_txresults over the caller's
    own arrays (passed as is; returns the digests), or a dict of check_role,
    body_flags, want_checks, want_fail, bad_cap (None: no list) -> TxResults."""
    dig = np.zeros((nb, 32), np.uint8)
    if results is None:
        ok, weight, used = np.zeros(nc, np.uint8), np.zeros(nc, np.uint32), np.zeros(nc, np.uint64)
        _check(fn(*head, _ptr(ok), _ptr(weight), _ptr(used), _ptr(dig), last))
        return ok, weight, used, dig
    if isinstance(results, sv_txresults):
        _check(fn(*head, ctypes.byref(results), _ptr(dig), last))
        return dig
    a = lambda x: x.__array_interface__["data"][0] if x is not None else 0  # noqa: E731
    role, flags = results.get("check_role"), results.get("body_flags")
    if role is not None:
        role = np.ascontiguousarray(np.asarray(role, dtype=np.uint8).reshape(-1))
        if role.shape[0] != nc:
            raise ValueError("check_role must hold one byte per check")
    if flags is not None:
        flags = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8).reshape(-1))
        if flags.shape[0] != nb:
            raise ValueError("body_flags must hold one byte per body")
    code = np.zeros(nb, np.uint8)
    fail = np.zeros(nb, np.uint32) if results.get("want_fail", True) else None
    ok = weight = used = None
    if results.get("want_checks", False):
        ok, weight, used = np.zeros(nc, np.uint8), np.zeros(nc, np.uint32), np.zeros(nc, np.uint64)
    cap = results.get("bad_cap")
    bad = np.zeros(int(cap), np.uint32) if cap is not None else None
    n_bad = np.zeros(1, np.uint64)
    r = results_desc(a(role), a(flags), a(code), a(fail), a(ok), a(weight), a(used),
                     a(bad) if cap else 0, cap or 0, a(n_bad))
    _check(fn(*head, ctypes.byref(r), _ptr(dig), last))
    n = int(n_bad[0])
    return TxResults(code, fail, bad[:min(n, int(cap))] if bad is not None else None, n, ok, weight, used, dig)


def _checks_desc(protocol_version, sig_len, check_begin, check_needed, signer_begin, signer_type, signer_weight,
                 signer_key, n_checks, n_signers, payload=None):
    """sv_txchecks over raw addresses (host arrays' or device pointers).
    payload: (pkey_begin, pkey, pkey_payload, pkey_len, n_pkeys) or None -- then
    the struct is the one without the payload tables, by its struct_size."""
    ck = sv_txchecks()
    ck.struct_size = ctypes.sizeof(sv_txchecks) if payload is not None else sv_txchecks.pkey_begin.offset
    if payload is not None:
        ck.pkey_begin, ck.pkey, ck.pkey_payload, ck.pkey_len = (x or None for x in payload[:4])
        ck.n_pkeys = int(payload[4])
    ck.protocol_version = int(protocol_version)
    ck.sig_len = sig_len or None
    ck.check_begin, ck.check_needed, ck.signer_begin = check_begin or None, check_needed or None, signer_begin or None
    ck.signer_type, ck.signer_weight, ck.signer_key = signer_type or None, signer_weight or None, signer_key or None
    ck.n_checks, ck.n_signers = int(n_checks), int(n_signers)
    return ck


def _check_host(fn, last, network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                check_begin, check_needed, signer_begin, signer_type, signer_weight, signer_key, sig_len,
                protocol_version, pkey_begin=None, pkey=None, pkey_payload=None, pkey_len=None, results=None):
    nid, bodies, off, ln, kind, nb, sb, hint, sig, ns, kb, key, nk = _hinted_args(
        network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key)
    cb = _csr(check_begin, nb, "check_begin")
    need = np.ascontiguousarray(np.asarray(check_needed, dtype=np.int32).reshape(-1))
    nc = need.shape[0]
    gb = _csr(signer_begin, nc, "signer_begin")
    gt = np.ascontiguousarray(np.asarray(signer_type, dtype=np.uint8).reshape(-1))
    gw = np.ascontiguousarray(np.asarray(signer_weight, dtype=np.uint32).reshape(-1))
    gk = np.ascontiguousarray(np.asarray(signer_key, dtype=np.uint32).reshape(-1))
    ng = gt.shape[0]
    if gw.shape[0] != ng or gk.shape[0] != ng:
        raise ValueError("signer_type / signer_weight / signer_key row mismatch")
    sl = None
    if sig_len is not None:
        sl = np.ascontiguousarray(np.asarray(sig_len, dtype=np.uint8).reshape(-1))
        if sl.shape[0] != ns:
            raise ValueError("sig_len must hold one byte per signature")
    a = lambda x: x.__array_interface__["data"][0]  # noqa: E731
    payload = None
    if pkey_begin is not None:
        qb = _csr(pkey_begin, nb, "pkey_begin")
        qk, qp = _u8(pkey if pkey is not None else [], 32), _u8(pkey_payload if pkey_payload is not None else [], 64)
        ql = np.ascontiguousarray(np.asarray(pkey_len if pkey_len is not None else [], dtype=np.uint8).reshape(-1))
        nq = qk.shape[0]
        if qp.shape[0] != nq or ql.shape[0] != nq:
            raise ValueError("pkey / pkey_payload / pkey_len row mismatch")
        payload = (a(qb), a(qk) if nq else 0, a(qp) if nq else 0, a(ql) if nq else 0, nq)
    elif pkey is not None or pkey_payload is not None or pkey_len is not None:
        raise ValueError("payload tables need pkey_begin")
    ck = _checks_desc(protocol_version, a(sl) if sl is not None else 0, a(cb), a(need), a(gb), a(gt), a(gw), a(gk),
                      nc, ng, payload)
    head = (_ptr(nid), _ptr(bodies), _ptr(off), _ptr(ln), _ptr(kind), nb, _ptr(sb), _ptr(hint), _ptr(sig), ns,
            _ptr(kb), _ptr(key), nk, ctypes.byref(ck))
    return _checked_call(fn, head, nb, nc, last, results)


def check_txbodies(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                   check_begin, check_needed, signer_begin, signer_type, signer_weight, signer_key, sig_len=None,
                   protocol_version: int = 21, device: int = -1, max_devices: int = 0, path=None, pkey_begin=None,
                   pkey=None, pkey_payload=None, pkey_len=None):
    """Signature checks decided on the device (sv_ed25519_check_txbodies): the
    inputs of verify_txbodies_hinted plus body t's checks check_begin[t]..
    check_begin[t+1]-1, each a needed weight and the signers signer_begin[c]..
    signer_begin[c+1]-1 (type, weight, global key index).  Returns (check_ok,
    check_weight, check_used, digests): one SignatureChecker::checkSignature
    decision per check, the weight it accumulated and the mask of the body's
    signatures it marked used.  With the payload tables (pkey_begin: CSR over
    the bodies; pkey n x 32, pkey_payload n x 64 zero-padded, pkey_len n) a
    type-3 signer's key is a global index into pkey and the decision includes
    the ED25519_SIGNED_PAYLOAD stage; without them type-3 signers are skipped."""
    lib = load_library()
    return _check_host(lib.sv_ed25519_check_txbodies, _opts(device, max_devices, path), network_id, bodies, body_off,
                       body_len, body_kind, sig_begin, hint, sig, key_begin, key, check_begin, check_needed,
                       signer_begin, signer_type, signer_weight, signer_key, sig_len, protocol_version, pkey_begin,
                       pkey, pkey_payload, pkey_len)


def check_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                       check_begin, check_needed, signer_begin, signer_type, signer_weight, signer_key, sig_len=None,
                       protocol_version: int = 21, threads: int = 0, pkey_begin=None, pkey=None, pkey_payload=None,
                       pkey_len=None):
    """The same on the engine's CPU path (what a caller runs on an engine error)."""
    lib = load_library()
    return _check_host(lib.sv_ed25519_check_txbodies_cpu, int(threads), network_id, bodies, body_off, body_len,
                       body_kind, sig_begin, hint, sig, key_begin, key, check_begin, check_needed, signer_begin,
                       signer_type, signer_weight, signer_key, sig_len, protocol_version, pkey_begin, pkey,
                       pkey_payload, pkey_len)


def check_txbodies_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int, d_body_kind: int,
                          n_bodies: int, d_sig_begin: int, d_hint: int, d_sig: int, n_sigs: int, d_key_begin: int,
                          d_key: int, n_keys: int, d_check_begin: int, d_check_needed: int, n_checks: int,
                          d_signer_begin: int, d_signer_type: int, d_signer_weight: int, d_signer_key: int,
                          n_signers: int, d_check_ok: int, d_check_weight: int, d_check_used: int,
                          d_sig_len: int = 0, protocol_version: int = 21, d_digests: int = 0, stream: int = 0,
                          d_pkey_begin: int = 0, d_pkey: int = 0, d_pkey_payload: int = 0, d_pkey_len: int = 0,
                          n_pkeys=None) -> None:
    """Device-resident form (raw device pointers; network_id is 32 host bytes).
    Waits on `stream` once for the pair count, enqueues the verification and
    the check kernel and returns; the decisions land in the d_check_* arrays.
    n_pkeys (not None) passes the payload tables d_pkey_*."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    ck = _checks_desc(protocol_version, d_sig_len, d_check_begin, d_check_needed, d_signer_begin, d_signer_type,
                      d_signer_weight, d_signer_key, n_checks, n_signers,
                      None if n_pkeys is None else (d_pkey_begin, d_pkey, d_pkey_payload, d_pkey_len, n_pkeys))
    _check(lib.sv_ed25519_check_txbodies_device(
        device, _ptr(nid), d_bodies or None, d_body_off or None, d_body_len or None, d_body_kind or None, n_bodies,
        d_sig_begin or None, d_hint or None, d_sig or None, n_sigs, d_key_begin or None, d_key or None, n_keys,
        ctypes.byref(ck), d_check_ok or None, d_check_weight or None, d_check_used or None, d_digests or None,
        stream or None))


def _accounts_desc(protocol_version, sig_len, acct_key, acct_thresholds, asigner_begin, asigner_type, asigner_weight,
                   asigner_key, asigner_payload, apayload, apayload_len, bacct_begin, bacct, check_begin, check_acct,
                   check_level, check_needed, n_accounts, n_asigners, n_apayloads, n_bacct, n_checks):
    """sv_txaccounts over raw addresses (host arrays' or device pointers; 0: NULL)."""
    ac = sv_txaccounts()
    ac.struct_size = ctypes.sizeof(sv_txaccounts)
    ac.protocol_version = int(protocol_version)
    for name, v in (("sig_len", sig_len), ("acct_key", acct_key), ("acct_thresholds", acct_thresholds),
                    ("asigner_begin", asigner_begin), ("asigner_type", asigner_type),
                    ("asigner_weight", asigner_weight), ("asigner_key", asigner_key),
                    ("asigner_payload", asigner_payload), ("apayload", apayload), ("apayload_len", apayload_len),
                    ("bacct_begin", bacct_begin), ("bacct", bacct), ("check_begin", check_begin),
                    ("check_acct", check_acct), ("check_level", check_level), ("check_needed", check_needed)):
        setattr(ac, name, v or None)
    ac.n_accounts, ac.n_asigners, ac.n_apayloads = int(n_accounts), int(n_asigners), int(n_apayloads)
    ac.n_bacct, ac.n_checks = int(n_bacct), int(n_checks)
    return ac


def _accounts_host(fn, last, network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                   acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key, asigner_payload,
                   apayload, apayload_len, bacct_begin, bacct, check_begin, check_acct, check_level, check_needed,
                   sig_len, protocol_version, results=None, ledger=None):
    """ledger: None, or a dict for the ledger forms -- in: bacct_id (n_bacct x 32, or None); out: "found", the
    call's bacct_found; the struct passed is then an sv_txledger over the sv_txaccounts."""
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    hint, sig = _u8(hint, 4), _u8(sig, 64)
    ns = sig.shape[0]
    if hint.shape[0] != ns:
        raise ValueError("hint/sig row mismatch")
    kind = np.ascontiguousarray(np.asarray(body_kind, dtype=np.uint8).reshape(-1))
    nb = kind.shape[0]
    bodies, off, ln = _var_msgs(bodies, body_off, body_len, nb)
    sb, eb, cb = _csr(sig_begin, nb, "sig_begin"), _csr(bacct_begin, nb, "bacct_begin"), _csr(check_begin, nb,
                                                                                             "check_begin")

    def arr(x, dt):
        return np.ascontiguousarray(np.asarray(x if x is not None else [], dtype=dt).reshape(-1))
    ak, th = _u8(acct_key, 32), _u8(acct_thresholds, 4)
    na = ak.shape[0]
    if th.shape[0] != na:
        raise ValueError("acct_key / acct_thresholds row mismatch")
    gb = np.ascontiguousarray(np.asarray(asigner_begin, dtype=np.uint64).reshape(-1))
    if gb.shape[0] != na + 1:
        raise ValueError("asigner_begin must hold n_accounts + 1 entries")
    gt, gw, gk = arr(asigner_type, np.uint8), arr(asigner_weight, np.uint32), _u8(asigner_key, 32)
    ng = gt.shape[0]
    gp = arr(asigner_payload, np.uint32) if asigner_payload is not None else None
    if gw.shape[0] != ng or gk.shape[0] != ng or (gp is not None and gp.shape[0] != ng):
        raise ValueError("asigner_type / asigner_weight / asigner_key / asigner_payload row mismatch")
    pay, pl = _u8(apayload if apayload is not None else [], 64), arr(apayload_len, np.uint8)
    npay = pay.shape[0]
    if pl.shape[0] != npay:
        raise ValueError("apayload / apayload_len row mismatch")
    ea, ca, lv = arr(bacct, np.uint32), arr(check_acct, np.uint32), arr(check_level, np.uint8)
    nc = ca.shape[0]
    need = arr(check_needed, np.int32) if check_needed is not None else None
    if lv.shape[0] != nc or (need is not None and need.shape[0] != nc):
        raise ValueError("check_acct / check_level / check_needed row mismatch")
    sl = None
    if sig_len is not None:
        sl = arr(sig_len, np.uint8)
        if sl.shape[0] != ns:
            raise ValueError("sig_len must hold one byte per signature")
    a = lambda x: x.__array_interface__["data"][0] if x is not None and x.size else 0  # noqa: E731
    ac = _accounts_desc(protocol_version, a(sl), a(ak), a(th), gb.__array_interface__["data"][0], a(gt), a(gw), a(gk),
                        a(gp), a(pay), a(pl), a(eb), a(ea), a(cb), a(ca), a(lv), a(need), na, ng, npay, ea.shape[0],
                        nc)
    table = ac
    if ledger is not None:
        ids = ledger.get("bacct_id")
        if ids is not None:
            ids = _u8(ids, 32)
            if ids.shape[0] != ea.shape[0]:
                raise ValueError("bacct_id must hold one 32-byte row per bacct entry")
        ledger["found"] = np.zeros(ea.shape[0], np.uint8)
        table = ledger_desc(ac, a(ids), a(ledger["found"]))
    head = (_ptr(nid), _ptr(bodies), _ptr(off), _ptr(ln), _ptr(kind), nb, _ptr(sb), _ptr(hint), _ptr(sig), ns,
            ctypes.byref(table))
    return _checked_call(fn, head, nb, nc, last, results)


def ledger_desc(accts, bacct_id=0, bacct_found=0, struct_size=None):
    """sv_txledger over an sv_txaccounts and raw addresses (host arrays' or device pointers; 0: NULL).  The
    returned struct keeps `accts` alive."""
    lg = sv_txledger()
    lg.struct_size = ctypes.sizeof(sv_txledger) if struct_size is None else int(struct_size)
    lg.accts = ctypes.pointer(accts)
    lg.bacct_id = bacct_id or None
    lg.bacct_found = bacct_found or None
    return lg


def check_txbodies_accounts(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                            acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key,
                            asigner_payload, apayload, apayload_len, bacct_begin, bacct, check_begin, check_acct,
                            check_level, check_needed=None, sig_len=None, protocol_version: int = 21,
                            device: int = -1, max_devices: int = 0, path=None):
    """Signature checks against an account table (sv_ed25519_check_txbodies_accounts):
    every account once (key, thresholds [master, low, med, high], its signers in
    CSR form; a type-3 signer's asigner_payload indexes apayload / apayload_len),
    per body the accounts its checks refer to (bacct_begin / bacct) and per check
    the position of its account in that list and a threshold level (0: the
    needed weight is check_needed[c]).  Returns (check_ok, check_weight,
    check_used, digests), by definition those of check_txbodies over the
    expansion (include/stellar_sigverify.h)."""
    lib = load_library()
    return _accounts_host(lib.sv_ed25519_check_txbodies_accounts, _opts(device, max_devices, path), network_id, bodies,
                          body_off, body_len, body_kind, sig_begin, hint, sig, acct_key, acct_thresholds,
                          asigner_begin, asigner_type, asigner_weight, asigner_key, asigner_payload, apayload,
                          apayload_len, bacct_begin, bacct, check_begin, check_acct, check_level, check_needed,
                          sig_len, protocol_version)


def check_txbodies_accounts_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                                acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key,
                                asigner_payload, apayload, apayload_len, bacct_begin, bacct, check_begin, check_acct,
                                check_level, check_needed=None, sig_len=None, protocol_version: int = 21,
                                threads: int = 0):
    """The same on the engine's CPU path (what a caller runs on an engine error)."""
    lib = load_library()
    return _accounts_host(lib.sv_ed25519_check_txbodies_accounts_cpu, int(threads), network_id, bodies, body_off,
                          body_len, body_kind, sig_begin, hint, sig, acct_key, acct_thresholds, asigner_begin,
                          asigner_type, asigner_weight, asigner_key, asigner_payload, apayload, apayload_len,
                          bacct_begin, bacct, check_begin, check_acct, check_level, check_needed, sig_len,
                          protocol_version)


def check_txbodies_accounts_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int,
                                   d_body_kind: int, n_bodies: int, d_sig_begin: int, d_hint: int, d_sig: int,
                                   n_sigs: int, d_acct_key: int, d_acct_thresholds: int, d_asigner_begin: int,
                                   d_asigner_type: int, d_asigner_weight: int, d_asigner_key: int,
                                   d_asigner_payload: int, d_apayload: int, d_apayload_len: int, n_accounts: int,
                                   n_asigners: int, n_apayloads: int, d_bacct_begin: int, d_bacct: int, n_bacct: int,
                                   d_check_begin: int, d_check_acct: int, d_check_level: int, d_check_needed: int,
                                   n_checks: int, d_check_ok: int, d_check_weight: int, d_check_used: int,
                                   d_sig_len: int = 0, protocol_version: int = 21, d_digests: int = 0,
                                   stream: int = 0) -> None:
    """Device-resident form (raw device pointers; network_id is 32 host bytes).
    Waits on `stream` for the expansion's row counts and for the pair counts,
    enqueues the verification and the check kernel and returns; the decisions
    land in the d_check_* arrays."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    ac = _accounts_desc(protocol_version, d_sig_len, d_acct_key, d_acct_thresholds, d_asigner_begin, d_asigner_type,
                        d_asigner_weight, d_asigner_key, d_asigner_payload, d_apayload, d_apayload_len, d_bacct_begin,
                        d_bacct, d_check_begin, d_check_acct, d_check_level, d_check_needed, n_accounts, n_asigners,
                        n_apayloads, n_bacct, n_checks)
    _check(lib.sv_ed25519_check_txbodies_accounts_device(
        device, _ptr(nid), d_bodies or None, d_body_off or None, d_body_len or None, d_body_kind or None, n_bodies,
        d_sig_begin or None, d_hint or None, d_sig or None, n_sigs, ctypes.byref(ac), d_check_ok or None,
        d_check_weight or None, d_check_used or None, d_digests or None, stream or None))


def _results_spec(res, check_role, body_flags, want_checks, want_fail, bad_cap):
    if res is not None:
        return res
    return {"check_role": check_role, "body_flags": body_flags, "want_checks": want_checks, "want_fail": want_fail,
            "bad_cap": bad_cap}


def decide_txbodies(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                    check_begin, check_needed, signer_begin, signer_type, signer_weight, signer_key, check_role=None,
                    body_flags=None, sig_len=None, protocol_version: int = 21, device: int = -1, max_devices: int = 0,
                    path=None, pkey_begin=None, pkey=None, pkey_payload=None, pkey_len=None, want_checks=False,
                    want_fail=True, bad_cap=None, res=None):
    """One signature result per body (sv_ed25519_decide_txbodies): the inputs of
    check_txbodies plus check_role (TXROLE_* per check; None: all TXROLE_TX) and
    body_flags (TXBODY_SKIP_UNUSED per body; None: 0).  Returns TxResults:
    body_code (TXRESULT_*), body_fail (the body-local index of the first failing
    check, TXRESULT_NONE: none), with bad_cap the ascending failing bodies (at
    most bad_cap of them) and their exact count n_bad, with want_checks the
    three check arrays of check_txbodies, and the digests.  res: an
    sv_txresults over the caller's own arrays (results_desc), passed as is; the
    call then returns the digests."""
    lib = load_library()
    return _check_host(lib.sv_ed25519_decide_txbodies, _opts(device, max_devices, path), network_id, bodies, body_off,
                       body_len, body_kind, sig_begin, hint, sig, key_begin, key, check_begin, check_needed,
                       signer_begin, signer_type, signer_weight, signer_key, sig_len, protocol_version, pkey_begin,
                       pkey, pkey_payload, pkey_len,
                       results=_results_spec(res, check_role, body_flags, want_checks, want_fail, bad_cap))


def decide_txbodies_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, key_begin, key,
                        check_begin, check_needed, signer_begin, signer_type, signer_weight, signer_key,
                        check_role=None, body_flags=None, sig_len=None, protocol_version: int = 21, threads: int = 0,
                        pkey_begin=None, pkey=None, pkey_payload=None, pkey_len=None, want_checks=False,
                        want_fail=True, bad_cap=None, res=None):
    """The same on the engine's CPU path (what a caller runs on an engine error)."""
    lib = load_library()
    return _check_host(lib.sv_ed25519_decide_txbodies_cpu, int(threads), network_id, bodies, body_off, body_len,
                       body_kind, sig_begin, hint, sig, key_begin, key, check_begin, check_needed, signer_begin,
                       signer_type, signer_weight, signer_key, sig_len, protocol_version, pkey_begin, pkey,
                       pkey_payload, pkey_len,
                       results=_results_spec(res, check_role, body_flags, want_checks, want_fail, bad_cap))


def decide_txbodies_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int, d_body_kind: int,
                           n_bodies: int, d_sig_begin: int, d_hint: int, d_sig: int, n_sigs: int, d_key_begin: int,
                           d_key: int, n_keys: int, d_check_begin: int, d_check_needed: int, n_checks: int,
                           d_signer_begin: int, d_signer_type: int, d_signer_weight: int, d_signer_key: int,
                           n_signers: int, res, d_sig_len: int = 0, protocol_version: int = 21, d_digests: int = 0,
                           stream: int = 0, d_pkey_begin: int = 0, d_pkey: int = 0, d_pkey_payload: int = 0,
                           d_pkey_len: int = 0, n_pkeys=None) -> None:
    """Device-resident form (raw device pointers; network_id is 32 host bytes;
    res: results_desc over device pointers, n_bad included).  Waits no more
    often than check_txbodies_device; the results land in res's arrays."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    ck = _checks_desc(protocol_version, d_sig_len, d_check_begin, d_check_needed, d_signer_begin, d_signer_type,
                      d_signer_weight, d_signer_key, n_checks, n_signers,
                      None if n_pkeys is None else (d_pkey_begin, d_pkey, d_pkey_payload, d_pkey_len, n_pkeys))
    _check(lib.sv_ed25519_decide_txbodies_device(
        device, _ptr(nid), d_bodies or None, d_body_off or None, d_body_len or None, d_body_kind or None, n_bodies,
        d_sig_begin or None, d_hint or None, d_sig or None, n_sigs, d_key_begin or None, d_key or None, n_keys,
        ctypes.byref(ck), ctypes.byref(res), d_digests or None, stream or None))


def decide_txbodies_accounts(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                             acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key,
                             asigner_payload, apayload, apayload_len, bacct_begin, bacct, check_begin, check_acct,
                             check_level, check_needed=None, check_role=None, body_flags=None, sig_len=None,
                             protocol_version: int = 21, device: int = -1, max_devices: int = 0, path=None,
                             want_checks=False, want_fail=True, bad_cap=None, res=None):
    """One signature result per body against an account table
    (sv_ed25519_decide_txbodies_accounts): the inputs of check_txbodies_accounts
    plus check_role and body_flags; returns TxResults as decide_txbodies."""
    lib = load_library()
    return _accounts_host(lib.sv_ed25519_decide_txbodies_accounts, _opts(device, max_devices, path), network_id,
                          bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key, acct_thresholds,
                          asigner_begin, asigner_type, asigner_weight, asigner_key, asigner_payload, apayload,
                          apayload_len, bacct_begin, bacct, check_begin, check_acct, check_level, check_needed,
                          sig_len, protocol_version,
                          results=_results_spec(res, check_role, body_flags, want_checks, want_fail, bad_cap))


def decide_txbodies_accounts_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                                 acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key,
                                 asigner_payload, apayload, apayload_len, bacct_begin, bacct, check_begin, check_acct,
                                 check_level, check_needed=None, check_role=None, body_flags=None, sig_len=None,
                                 protocol_version: int = 21, threads: int = 0, want_checks=False, want_fail=True,
                                 bad_cap=None, res=None):
    """The same on the engine's CPU path (what a caller runs on an engine error)."""
    lib = load_library()
    return _accounts_host(lib.sv_ed25519_decide_txbodies_accounts_cpu, int(threads), network_id, bodies, body_off,
                          body_len, body_kind, sig_begin, hint, sig, acct_key, acct_thresholds, asigner_begin,
                          asigner_type, asigner_weight, asigner_key, asigner_payload, apayload, apayload_len,
                          bacct_begin, bacct, check_begin, check_acct, check_level, check_needed, sig_len,
                          protocol_version,
                          results=_results_spec(res, check_role, body_flags, want_checks, want_fail, bad_cap))


def decide_txbodies_accounts_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int,
                                    d_body_kind: int, n_bodies: int, d_sig_begin: int, d_hint: int, d_sig: int,
                                    n_sigs: int, d_acct_key: int, d_acct_thresholds: int, d_asigner_begin: int,
                                    d_asigner_type: int, d_asigner_weight: int, d_asigner_key: int,
                                    d_asigner_payload: int, d_apayload: int, d_apayload_len: int, n_accounts: int,
                                    n_asigners: int, n_apayloads: int, d_bacct_begin: int, d_bacct: int, n_bacct: int,
                                    d_check_begin: int, d_check_acct: int, d_check_level: int, d_check_needed: int,
                                    n_checks: int, res, d_sig_len: int = 0, protocol_version: int = 21,
                                    d_digests: int = 0, stream: int = 0) -> None:
    """Device-resident form (raw device pointers; res: results_desc over device
    pointers).  Waits as often as check_txbodies_accounts_device."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    ac = _accounts_desc(protocol_version, d_sig_len, d_acct_key, d_acct_thresholds, d_asigner_begin, d_asigner_type,
                        d_asigner_weight, d_asigner_key, d_asigner_payload, d_apayload, d_apayload_len, d_bacct_begin,
                        d_bacct, d_check_begin, d_check_acct, d_check_level, d_check_needed, n_accounts, n_asigners,
                        n_apayloads, n_bacct, n_checks)
    _check(lib.sv_ed25519_decide_txbodies_accounts_device(
        device, _ptr(nid), d_bodies or None, d_body_off or None, d_body_len or None, d_body_kind or None, n_bodies,
        d_sig_begin or None, d_hint or None, d_sig or None, n_sigs, ctypes.byref(ac), ctypes.byref(res),
        d_digests or None, stream or None))


def check_txbodies_ledger_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                              acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key,
                              asigner_payload, apayload, apayload_len, bacct_begin, bacct, bacct_id, check_begin,
                              check_acct, check_level, check_needed=None, sig_len=None, protocol_version: int = 21,
                              threads: int = 0):
    """Signature checks that name the account store's accounts by ID
    (sv_ed25519_check_txbodies_ledger_cpu): the arguments of
    check_txbodies_accounts_cpu, whose account table is this call's LOCAL
    accounts, plus bacct_id (n_bacct x 32), read where bacct[e] == BACCT_BY_ID.
    Returns ((check_ok, check_weight, check_used, digests), bacct_found)."""
    lib = load_library()
    lg = {"bacct_id": bacct_id}
    r = _accounts_host(lib.sv_ed25519_check_txbodies_ledger_cpu, int(threads), network_id, bodies, body_off, body_len,
                       body_kind, sig_begin, hint, sig, acct_key, acct_thresholds, asigner_begin, asigner_type,
                       asigner_weight, asigner_key, asigner_payload, apayload, apayload_len, bacct_begin, bacct,
                       check_begin, check_acct, check_level, check_needed, sig_len, protocol_version, ledger=lg)
    return r, lg["found"]


def decide_txbodies_ledger_cpu(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                               acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key,
                               asigner_payload, apayload, apayload_len, bacct_begin, bacct, bacct_id, check_begin,
                               check_acct, check_level, check_needed=None, check_role=None, body_flags=None,
                               sig_len=None, protocol_version: int = 21, threads: int = 0, want_checks=False,
                               want_fail=True, bad_cap=None, res=None):
    """One result per body over the same input (sv_ed25519_decide_txbodies_ledger_cpu).
    Returns (TxResults as decide_txbodies_accounts_cpu, bacct_found)."""
    lib = load_library()
    lg = {"bacct_id": bacct_id}
    r = _accounts_host(lib.sv_ed25519_decide_txbodies_ledger_cpu, int(threads), network_id, bodies, body_off, body_len,
                       body_kind, sig_begin, hint, sig, acct_key, acct_thresholds, asigner_begin, asigner_type,
                       asigner_weight, asigner_key, asigner_payload, apayload, apayload_len, bacct_begin, bacct,
                       check_begin, check_acct, check_level, check_needed, sig_len, protocol_version,
                       results=_results_spec(res, check_role, body_flags, want_checks, want_fail, bad_cap), ledger=lg)
    return r, lg["found"]


def check_txbodies_ledger(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                          acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key, asigner_payload,
                          apayload, apayload_len, bacct_begin, bacct, bacct_id, check_begin, check_acct, check_level,
                          check_needed=None, sig_len=None, protocol_version: int = 21, device: int = -1,
                          max_devices: int = 0, path=None):
    """The same from host buffers on the GPU (sv_ed25519_check_txbodies_ledger): the
    IDs are resolved on the host index, only the local accounts go up.  Returns
    ((check_ok, check_weight, check_used, digests), bacct_found)."""
    lib = load_library()
    lg = {"bacct_id": bacct_id}
    r = _accounts_host(lib.sv_ed25519_check_txbodies_ledger, _opts(device, max_devices, path), network_id, bodies,
                       body_off, body_len, body_kind, sig_begin, hint, sig, acct_key, acct_thresholds, asigner_begin,
                       asigner_type, asigner_weight, asigner_key, asigner_payload, apayload, apayload_len, bacct_begin,
                       bacct, check_begin, check_acct, check_level, check_needed, sig_len, protocol_version, ledger=lg)
    return r, lg["found"]


def decide_txbodies_ledger(network_id, bodies, body_off, body_len, body_kind, sig_begin, hint, sig, acct_key,
                           acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key, asigner_payload,
                           apayload, apayload_len, bacct_begin, bacct, bacct_id, check_begin, check_acct, check_level,
                           check_needed=None, check_role=None, body_flags=None, sig_len=None,
                           protocol_version: int = 21, device: int = -1, max_devices: int = 0, path=None,
                           want_checks=False, want_fail=True, bad_cap=None, res=None):
    """One result per body from host buffers (sv_ed25519_decide_txbodies_ledger).
    Returns (TxResults as decide_txbodies_accounts, bacct_found)."""
    lib = load_library()
    lg = {"bacct_id": bacct_id}
    r = _accounts_host(lib.sv_ed25519_decide_txbodies_ledger, _opts(device, max_devices, path), network_id, bodies,
                       body_off, body_len, body_kind, sig_begin, hint, sig, acct_key, acct_thresholds, asigner_begin,
                       asigner_type, asigner_weight, asigner_key, asigner_payload, apayload, apayload_len, bacct_begin,
                       bacct, check_begin, check_acct, check_level, check_needed, sig_len, protocol_version,
                       results=_results_spec(res, check_role, body_flags, want_checks, want_fail, bad_cap), ledger=lg)
    return r, lg["found"]


def check_txbodies_ledger_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int,
                                 d_body_kind: int, n_bodies: int, d_sig_begin: int, d_hint: int, d_sig: int,
                                 n_sigs: int, d_acct_key: int, d_acct_thresholds: int, d_asigner_begin: int,
                                 d_asigner_type: int, d_asigner_weight: int, d_asigner_key: int,
                                 d_asigner_payload: int, d_apayload: int, d_apayload_len: int, n_accounts: int,
                                 n_asigners: int, n_apayloads: int, d_bacct_begin: int, d_bacct: int, n_bacct: int,
                                 d_bacct_id: int, d_bacct_found: int, d_check_begin: int, d_check_acct: int,
                                 d_check_level: int, d_check_needed: int, n_checks: int, d_check_ok: int,
                                 d_check_weight: int, d_check_used: int, d_sig_len: int = 0,
                                 protocol_version: int = 21, d_digests: int = 0, stream: int = 0) -> None:
    """Device-resident form (raw device pointers; network_id is 32 host bytes):
    check_txbodies_accounts_device's arguments, the account table being the
    call's local accounts, plus d_bacct_id (n_bacct x 32, 16-byte aligned) and
    the optional d_bacct_found (n_bacct bytes).  Waits as its twin does."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    ac = _accounts_desc(protocol_version, d_sig_len, d_acct_key, d_acct_thresholds, d_asigner_begin, d_asigner_type,
                        d_asigner_weight, d_asigner_key, d_asigner_payload, d_apayload, d_apayload_len, d_bacct_begin,
                        d_bacct, d_check_begin, d_check_acct, d_check_level, d_check_needed, n_accounts, n_asigners,
                        n_apayloads, n_bacct, n_checks)
    lg = ledger_desc(ac, d_bacct_id, d_bacct_found)
    _check(lib.sv_ed25519_check_txbodies_ledger_device(
        device, _ptr(nid), d_bodies or None, d_body_off or None, d_body_len or None, d_body_kind or None, n_bodies,
        d_sig_begin or None, d_hint or None, d_sig or None, n_sigs, ctypes.byref(lg), d_check_ok or None,
        d_check_weight or None, d_check_used or None, d_digests or None, stream or None))


def decide_txbodies_ledger_device(device: int, network_id, d_bodies: int, d_body_off: int, d_body_len: int,
                                  d_body_kind: int, n_bodies: int, d_sig_begin: int, d_hint: int, d_sig: int,
                                  n_sigs: int, d_acct_key: int, d_acct_thresholds: int, d_asigner_begin: int,
                                  d_asigner_type: int, d_asigner_weight: int, d_asigner_key: int,
                                  d_asigner_payload: int, d_apayload: int, d_apayload_len: int, n_accounts: int,
                                  n_asigners: int, n_apayloads: int, d_bacct_begin: int, d_bacct: int, n_bacct: int,
                                  d_bacct_id: int, d_bacct_found: int, d_check_begin: int, d_check_acct: int,
                                  d_check_level: int, d_check_needed: int, n_checks: int, res, d_sig_len: int = 0,
                                  protocol_version: int = 21, d_digests: int = 0, stream: int = 0) -> None:
    """Device-resident decide form (res: results_desc over device pointers)."""
    lib = load_library()
    nid = np.ascontiguousarray(np.frombuffer(bytes(network_id), np.uint8))
    if nid.size != 32:
        raise ValueError("network_id must be 32 bytes")
    ac = _accounts_desc(protocol_version, d_sig_len, d_acct_key, d_acct_thresholds, d_asigner_begin, d_asigner_type,
                        d_asigner_weight, d_asigner_key, d_asigner_payload, d_apayload, d_apayload_len, d_bacct_begin,
                        d_bacct, d_check_begin, d_check_acct, d_check_level, d_check_needed, n_accounts, n_asigners,
                        n_apayloads, n_bacct, n_checks)
    lg = ledger_desc(ac, d_bacct_id, d_bacct_found)
    _check(lib.sv_ed25519_decide_txbodies_ledger_device(
        device, _ptr(nid), d_bodies or None, d_body_off or None, d_body_len or None, d_body_kind or None, n_bodies,
        d_sig_begin or None, d_hint or None, d_sig or None, n_sigs, ctypes.byref(lg), ctypes.byref(res),
        d_digests or None, stream or None))


def set_account_store(accounts: int, payloads: int = 0, local_accounts: int = 0) -> None:
    """The account store (sv_set_account_store): capacity in accounts (0: off),
    in 64-byte payload rows for type-3 signers, and the rows a ledger call may
    borrow for its local accounts.  Replaces (and empties) an existing store."""
    _check(load_library().sv_set_account_store(int(accounts), int(payloads), int(local_accounts)))


def account_store_upsert(acct_key, acct_thresholds, asigner_begin, asigner_type, asigner_weight, asigner_key,
                         asigner_payload=None, apayload=None, apayload_len=None) -> None:
    """Inserts or replaces accounts (sv_account_store_upsert): the account-table
    arrays of check_txbodies_accounts.  All of the batch or none of it."""
    def arr(x, dt):
        return np.ascontiguousarray(np.asarray(x if x is not None else [], dtype=dt).reshape(-1))
    ak, th = _u8(acct_key, 32), _u8(acct_thresholds, 4)
    na = ak.shape[0]
    gb = np.ascontiguousarray(np.asarray(asigner_begin, dtype=np.uint64).reshape(-1))
    if th.shape[0] != na or gb.shape[0] != na + 1:
        raise ValueError("acct_key / acct_thresholds / asigner_begin row mismatch")
    gt, gw, gk = arr(asigner_type, np.uint8), arr(asigner_weight, np.uint32), _u8(asigner_key, 32)
    ng = gt.shape[0]
    gp = arr(asigner_payload, np.uint32) if asigner_payload is not None else None
    if gw.shape[0] != ng or gk.shape[0] != ng or (gp is not None and gp.shape[0] != ng):
        raise ValueError("asigner_type / asigner_weight / asigner_key / asigner_payload row mismatch")
    pay, pl = _u8(apayload if apayload is not None else [], 64), arr(apayload_len, np.uint8)
    if pl.shape[0] != pay.shape[0]:
        raise ValueError("apayload / apayload_len row mismatch")
    a = lambda x: x.__array_interface__["data"][0] if x is not None and x.size else 0  # noqa: E731
    ac = _accounts_desc(0, 0, a(ak), a(th), gb.__array_interface__["data"][0], a(gt), a(gw), a(gk), a(gp), a(pay),
                        a(pl), 0, 0, 0, 0, 0, 0, na, ng, pay.shape[0], 0, 0)
    _check(load_library().sv_account_store_upsert(ctypes.byref(ac)))


def account_store_erase(ids) -> None:
    """Erases accounts by ID (n x 32); an ID the store does not hold is counted, not refused."""
    ids = _u8(ids, 32)
    _check(load_library().sv_account_store_erase(_ptr(ids), ids.shape[0]))


def account_store_clear() -> None:
    _check(load_library().sv_account_store_clear())


def account_store_stats(device: int = -1) -> dict:
    """sv_account_store_get_stats; device -1: the host side only."""
    st = AccountStoreStats()
    st.struct_size = ctypes.sizeof(AccountStoreStats)
    _check(load_library().sv_account_store_get_stats(int(device), ctypes.byref(st)))
    return {f: getattr(st, f) for f, _ in AccountStoreStats._fields_ if f != "struct_size"}


AccountRows = collections.namedtuple(
    "AccountRows", "found thresholds n_signers signer_type signer_weight signer_key signer_payload signer_payload_len")


def account_store_read(ids, device: int = -1) -> AccountRows:
    """n accounts by ID as the store holds them (sv_account_store_read): from the
    host copy (device -1) or from a slot's replica, by its lookup kernel.  Rows
    of 20 signers; an ID that is not held reads as found 0 and zeros."""
    ids = _u8(ids, 32)
    n = ids.shape[0]
    r = AccountRows(np.zeros(n, np.uint8), np.zeros((n, 4), np.uint8), np.zeros(n, np.uint32),
                    np.zeros((n, 20), np.uint8), np.zeros((n, 20), np.uint32), np.zeros((n, 20, 32), np.uint8),
                    np.zeros((n, 20, 64), np.uint8), np.zeros((n, 20), np.uint8))
    _check(load_library().sv_account_store_read(int(device), _ptr(ids), n, *[_ptr(x) for x in r]))
    return r


def verify_gather(items, keys: bool = False, device: int = -1, max_devices: int = 0):
    """Gather form: items = [(pk32, sig64, msg), ...] as bytes objects; the engine
    packs them straight from their buffers.  Returns verdicts (and cache keys)."""
    lib = load_library()
    n = len(items)
    bufs = [(bytes(p), bytes(s), bytes(m)) for p, s, m in items]
    P = (ctypes.c_char_p * max(1, n))(*[b[0] for b in bufs])
    S = (ctypes.c_char_p * max(1, n))(*[b[1] for b in bufs])
    M = (ctypes.c_char_p * max(1, n))(*[b[2] for b in bufs])
    L = np.array([len(b[2]) for b in bufs], np.uint32)
    out = np.zeros(n, np.uint8)
    kb = np.zeros((n, 32), np.uint8) if keys else None
    _check(lib.sv_ed25519_verify_batch_gather(ctypes.cast(P, ctypes.c_void_p), ctypes.cast(S, ctypes.c_void_p),
                                              ctypes.cast(M, ctypes.c_void_p), _ptr(L), n, _ptr(out),
                                              _ptr(kb) if keys else None, _opts(device, max_devices)))
    return (out, kb) if keys else out


def set_device_map(physical) -> None:
    """Device slots -> physical GPUs (e.g. [0, 0]: two slots on GPU 0); [] restores."""
    lib = load_library()
    arr = (ctypes.c_int * max(1, len(physical)))(*physical)
    _check(lib.sv_set_device_map(ctypes.cast(arr, ctypes.c_void_p), len(physical)))


def set_min_shard(n: int) -> None:
    _check(load_library().sv_set_min_shard(int(n)))


def set_debug_flags(flags: int) -> int:
    rc = load_library().sv_set_debug_flags(int(flags))
    if rc < 0:
        _check(rc)
    return rc


def workspace_bytes(device: int = 0) -> int:
    v = ctypes.c_size_t()
    _check(load_library().sv_workspace_bytes(device, ctypes.byref(v)))
    return v.value


def pinned_bytes(device: int = 0) -> int:
    v = ctypes.c_size_t()
    _check(load_library().sv_pinned_bytes(device, ctypes.byref(v)))
    return v.value


def set_kernel_path(path: int) -> int:
    """Process-wide default kernel path (PATH_AUTO / PATH_THROUGHPUT /
    PATH_LATENCY) for calls that do not request one; returns the previous."""
    lib = load_library()
    lib.sv_set_kernel_path.argtypes = [ctypes.c_int]
    rc = lib.sv_set_kernel_path(int(path))
    if rc < 0:
        _check(rc)
    return rc


def timing_enable(on: bool = True) -> None:
    _check(load_library().sv_timing_enable(1 if on else 0))


def kernel_time(device: int = 0):
    lib = load_library()
    ms, la, sg = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib.sv_kernel_time(device, ctypes.byref(ms), ctypes.byref(la), ctypes.byref(sg)))
    return ms.value, la.value, sg.value


def kernel_time_reset() -> None:
    _check(load_library().sv_kernel_time_reset())


def synchronize(device: int = 0) -> None:
    _check(load_library().sv_device_synchronize(device))


def set_key_cache(capacity: int) -> None:
    """Key-cache capacity of the warm-key latency path (0: off); clears it."""
    _check(load_library().sv_set_key_cache(int(capacity)))


def set_key_tables(mode: int, slots: int = 0) -> int:
    """Per-key tables of the throughput path: 0 off, 1 on, 2 auto (host
    batches whose keys repeat), -1 the SV_KEY_TABLES default; slots 0 keeps
    SV_KEY_TABLE_SLOTS / 2^19.  Returns the previous mode."""
    rc = load_library().sv_set_key_tables(int(mode), int(slots))
    if rc < -1:
        _check(rc)
    return rc


def key_cache_wait(device: int = 0) -> None:
    """Blocks until the device's queued key-table builds have finished."""
    _check(load_library().sv_key_cache_wait(device))


def key_cache_stats(device: int = 0) -> dict:
    st = KeyCacheStats()
    _check(load_library().sv_key_cache_get_stats(device, ctypes.byref(st)))
    return {f: int(getattr(st, f)) for f, _ in KeyCacheStats._fields_}


VERDICT_CACHE_MAX = 1 << 24


def set_verdict_cache(entries: int) -> None:
    """Entries of every slot's verdict cache (include/stellar_sigverify.h sv_set_verdict_cache): rounded up to a
    power of two >= 4, 0 (the default) off.  Drains and clears every slot."""
    entries = int(entries)
    if entries < 0 or entries > VERDICT_CACHE_MAX:
        raise ValueError("verdict cache entries must be in [0, 2^24]")
    _check(load_library().sv_set_verdict_cache(entries))


def verdict_cache_clear() -> None:
    """Empties every slot's verdict cache (the twin of clearVerifySigCache); the counters stay."""
    _check(load_library().sv_verdict_cache_clear())


def verdict_cache_stats(device: int = 0) -> dict:
    """The slot's verdict-cache counters since the capacity was last set; waits for the slot's kernel stream."""
    st = VerdictCacheShareStats()
    st.struct_size = ctypes.sizeof(VerdictCacheShareStats)
    _check(load_library().sv_verdict_cache_get_stats(device, ctypes.byref(st)))
    out = {f: int(getattr(st, f)) for f, _ in VerdictCacheStats._fields_[:7]}
    out["kernel_ms"], out["wait_ms"] = float(st.kernel_ms), float(st.wait_ms)
    out.update({f: int(getattr(st, f)) for f, _ in VerdictCacheStats._fields_[9:]})
    out.update({f: int(getattr(st, f)) for f in SHARED})
    return out


VC_FEED_LANE, VC_FEED_BULK = 1, 2
VC_MISS = 0xFF
VC_SHARE_FEED, VC_SHARE_STORES = 1, 2


def set_verdict_cache_share(what: int) -> None:
    """What the slots tell each other about verified verdicts (include/stellar_sigverify.h
    sv_set_verdict_cache_share): VC_SHARE_FEED appends a journaled keyed lane batch to every slot's journal,
    VC_SHARE_STORES hands the misses a cached launch verified to the other slots' journals; 0 (the default)
    neither.  Process-wide; drops pending shared rows."""
    what = int(what)
    if what < 0 or what >> 32:
        raise ValueError("what must fit 32 bits")
    _check(load_library().sv_set_verdict_cache_share(what))


def set_verdict_cache_feed(sources: int, journal_rows: int = 0) -> None:
    """Which keyed batches feed the verdict cache (include/stellar_sigverify.h sv_set_verdict_cache_feed):
    VC_FEED_LANE journals keyed latency-lane batches, VC_FEED_BULK runs keyed bulk-route host batches behind the
    cache; 0 (the default) neither.  journal_rows: rows of a slot's journal (0: 65,536).  Drops what the journals
    hold."""
    sources, journal_rows = int(sources), int(journal_rows)
    if sources < 0 or sources >> 32 or journal_rows < 0:
        raise ValueError("sources must fit 32 bits and journal_rows must be non-negative")
    _check(load_library().sv_set_verdict_cache_feed(sources, journal_rows))


def verdict_cache_sync(device: int = 0) -> None:
    """Drains the slot's journal into its verdict cache and waits for the inserts."""
    _check(load_library().sv_verdict_cache_sync(device))


def verdict_cache_lookup(keys, device: int = 0) -> np.ndarray:
    """Per 32-byte cache key the verdict the slot's table holds (0 or 1) or VC_MISS; drains the journal first and
    changes nothing in the table or its lookup counters."""
    keys = np.ascontiguousarray(keys).view(np.uint8).reshape(-1)
    if keys.size % 32:
        raise ValueError("keys must be n x 32 bytes")
    n = keys.size // 32
    out = np.empty(n, np.uint8)
    _check(load_library().sv_verdict_cache_lookup(device, keys.ctypes.data if n else None, n,
                                                  out.ctypes.data if n else None))
    return out


def verdict_cache_lookup_device(device: int, d_keys: int, n: int, d_out: int, stream: int = 0) -> None:
    """verdict_cache_lookup over device memory (raw pointers; d_keys n x 32 and 16-byte aligned, d_out n bytes),
    ordered on `stream`; does not wait for the result."""
    n = int(n)
    if n < 0:
        raise ValueError("n must be non-negative")
    if n and not (d_keys and d_out):
        raise ValueError("d_keys and d_out must be device pointers")
    if d_keys & 15:
        raise ValueError("d_keys must be 16-byte aligned")
    _check(load_library().sv_verdict_cache_lookup_device(device, d_keys or None, n, d_out or None, stream or None))


def verify_device_cached(device: int, d_pk: int, d_sig: int, d_msg: int, n: int, d_verdict: int,
                         d_bitmap: int = 0, d_hit: int = 0, d_keys: int = 0, stream: int = 0,
                         fixed_msg_len: int = 32, d_msg_off: int = 0, d_msg_len: int = 0) -> None:
    """verify_device behind the slot's verdict cache (raw device pointers).  d_hit (optional, n bytes): 1 where
    the verdict came from the cache; d_keys (optional, n x 32, 16-byte aligned): the cache keys.  With the cache
    on the call waits once on `stream`, for the miss count."""
    n, fixed_msg_len = int(n), int(fixed_msg_len)
    if n < 0 or fixed_msg_len < 0 or fixed_msg_len >> 32:
        raise ValueError("n and fixed_msg_len must be non-negative (fixed_msg_len below 2^32)")
    if n and not (d_pk and d_sig and d_msg and d_verdict):
        raise ValueError("d_pk, d_sig, d_msg and d_verdict must be device pointers")
    if n and fixed_msg_len == 0 and not (d_msg_off and d_msg_len):
        raise ValueError("variable-length messages need d_msg_off and d_msg_len")
    if (d_pk | d_sig | d_keys) & 15:
        raise ValueError("d_pk, d_sig and d_keys must be 16-byte aligned")
    lib = load_library()
    _check(lib.sv_ed25519_verify_device_cached(device, d_pk, d_sig, d_msg, d_msg_off or None, d_msg_len or None,
                                               fixed_msg_len, n, d_verdict, d_bitmap or None, d_hit or None,
                                               d_keys or None, stream or None))


AUDIT_REJECTS, AUDIT_SAMPLE, AUDIT_STRICT = 1, 2, 4


def set_audit(what: int, one_in: int = 0, seed: int = 0, budget: int = 0) -> None:
    """The verdict audit (include/stellar_sigverify.h sv_set_audit), process-wide: behind every bulk-route verify
    launch the rejects (AUDIT_REJECTS) and / or a seeded 1-in-one_in sample of the rows (AUDIT_SAMPLE) are verified
    again by the textbook equation; AUDIT_STRICT makes a host-buffer call that saw a disagreement return
    SV_ERR_AUDIT.  budget: audited rows per launch (0: 65,536).  what == 0 (the default) turns it off and frees
    its buffers."""
    what, one_in, seed, budget = int(what), int(one_in), int(seed), int(budget)
    if min(what, one_in, seed, budget) < 0 or what >> 32 or one_in >> 32 or seed >> 64:
        raise ValueError("what and one_in must fit 32 bits, seed 64 bits, and none may be negative")
    _check(load_library().sv_set_audit(what, one_in, seed, budget))


def _audit_stats_dict(st) -> dict:
    out = {f: int(getattr(st, f)) for f, _ in AuditStats._fields_[:-1]}
    out["kernel_ms"] = float(st.kernel_ms)
    return out


def _audit_records(recs, n) -> list:
    out = []
    for r in recs[:n]:
        keep = min(int(r.msg_len), AUDIT_MSG_MAX)
        out.append({"seq": int(r.seq), "row": int(r.row), "msg_len": int(r.msg_len), "engine": int(r.engine_verdict),
                    "audit": int(r.audit_verdict), "cpu": int(r.cpu_verdict), "flags": int(r.flags),
                    "pk": bytes(r.pk), "sig": bytes(r.sig), "msg": bytes(r.msg)[:keep], "raw": bytes(r)})
    return out


def audit_stats(device: int = 0) -> dict:
    """The slot's audit counters; waits for the slot's kernel stream."""
    st = AuditStats()
    st.struct_size = ctypes.sizeof(AuditStats)
    _check(load_library().sv_audit_get_stats(device, ctypes.byref(st)))
    return _audit_stats_dict(st)


def audit_read(device: int = 0, cap: int = AUDIT_RING) -> list:
    """The mismatch records the slot's ring holds, oldest first, at most `cap`; consumes them.  Each record's `cpu`
    is the host's verdict over the record's bytes (0xFF: the message was truncated)."""
    cap = int(cap)
    if cap < 0:
        raise ValueError("cap must be non-negative")
    recs = (AuditRecord * max(cap, 1))()
    n = ctypes.c_size_t(0)
    _check(load_library().sv_audit_read(device, ctypes.cast(recs, ctypes.c_void_p), cap, ctypes.byref(n)))
    return _audit_records(recs, n.value)


def _audit_opts(what, one_in, seed, seq, budget) -> AuditOpts:
    return AuditOpts(ctypes.sizeof(AuditOpts), int(what), int(one_in), int(seed), int(seq), int(budget))


def audit_device(device: int, d_pk: int, d_sig: int, d_msg: int, n: int, d_claimed: int, what: int,
                 one_in: int = 0, seed: int = 0, seq: int = 0, budget: int = 0, stream: int = 0,
                 fixed_msg_len: int = 32, d_msg_off: int = 0, d_msg_len: int = 0) -> None:
    """Audits n claimed verdict bytes in device memory against the textbook kernel (raw device pointers; d_pk and
    d_sig 16-byte aligned), into the slot's counters and ring; ordered on `stream`, does not wait."""
    n, fixed_msg_len = int(n), int(fixed_msg_len)
    if n < 0 or fixed_msg_len < 0 or fixed_msg_len >> 32:
        raise ValueError("n and fixed_msg_len must be non-negative (fixed_msg_len below 2^32)")
    if n and not (d_pk and d_sig and d_msg and d_claimed):
        raise ValueError("d_pk, d_sig, d_msg and d_claimed must be device pointers")
    if (d_pk | d_sig) & 15:
        raise ValueError("d_pk and d_sig must be 16-byte aligned")
    o = _audit_opts(what, one_in, seed, seq, budget)
    _check(load_library().sv_audit_device(device, ctypes.byref(o), d_pk or None, d_sig or None, d_msg or None,
                                          d_msg_off or None, d_msg_len or None, fixed_msg_len, n, d_claimed or None,
                                          stream or None))


def audit_batch_cpu(pk, sig, msg, msg_off, msg_len, claimed, what: int, one_in: int = 0, seed: int = 0,
                    seq: int = 0, budget: int = 0, fixed_msg_len: int = 0, cap: int = AUDIT_RING, threads: int = 0):
    """The CPU twin of the audit (sv_audit_batch_cpu): the same pick, budget and records over host arrays, the
    textbook verifier on the host.  fixed_msg_len != 0: message i = msg[i * fixed_msg_len:][:fixed_msg_len], and
    msg_off / msg_len are not read.  Returns (stats, records)."""
    pk, sig = _u8(pk, 32), _u8(sig, 64)
    n = pk.shape[0]
    msg = np.ascontiguousarray(np.asarray(msg, dtype=np.uint8)).reshape(-1)
    claimed = np.ascontiguousarray(np.asarray(claimed, dtype=np.uint8)).reshape(-1)
    if sig.shape[0] != n or claimed.size != n:
        raise ValueError("pk / sig / claimed row mismatch")
    off = ln = None
    if not fixed_msg_len:
        off = np.ascontiguousarray(np.asarray(msg_off, dtype=np.uint64)).reshape(-1)
        ln = np.ascontiguousarray(np.asarray(msg_len, dtype=np.uint32)).reshape(-1)
        if off.size != n or ln.size != n:
            raise ValueError("msg_off / msg_len row mismatch")
    o = _audit_opts(what, one_in, seed, seq, budget)
    st = AuditStats()
    st.struct_size = ctypes.sizeof(AuditStats)
    cap = int(cap)
    recs = (AuditRecord * max(cap, 1))()
    nr = ctypes.c_size_t(0)
    p = lambda a: None if a is None or a.size == 0 else _ptr(a)  # noqa: E731
    _check(load_library().sv_audit_batch_cpu(ctypes.byref(o), p(pk), p(sig), p(msg), p(off), p(ln), int(fixed_msg_len),
                                             n, p(claimed), ctypes.byref(st), ctypes.cast(recs, ctypes.c_void_p), cap,
                                             ctypes.byref(nr), int(threads)))
    return _audit_stats_dict(st), _audit_records(recs, nr.value)


LAT_TRACE_FIELDS = ("plan_pack_us", "h2d_call_us", "launch_us", "d2h_rec_us", "build_us", "sync_us", "total_us", "warm")


def host_feed_probe(pk, sig, msg, msg_len: int, max_devices: int = 0, upload: bool = True) -> dict:
    """The host side of a multi-slot fixed-length batch without kernels
    (sv_host_feed_probe, include/stellar_sigverify.h): slices, each slot's
    staging workers, pack into pinned staging, optionally the H2D copies."""
    pk, sig, msg = (np.ascontiguousarray(x, dtype=np.uint8) for x in (pk, sig, msg))
    n = pk.reshape(-1, 32).shape[0]
    if sig.size != 64 * n or msg.size != msg_len * n:
        raise ValueError("pk/sig/msg row mismatch")
    st = FeedStats()
    st.struct_size = ctypes.sizeof(FeedStats)
    _check(load_library().sv_host_feed_probe(pk.ctypes.data, sig.ctypes.data, msg.ctypes.data, msg_len, n,
                                             max_devices, 1 if upload else 0, ctypes.byref(st)))
    G = st.slots
    return {"seconds": st.seconds, "slots": G, "threads_per_slot": st.threads_per_slot,
            "usable_cpus": st.usable_cpus, "gpu_numa": list(st.gpu_numa)[:G],
            "staging_numa": list(st.staging_numa)[:G], "pinned_cpus": list(st.pinned_cpus)[:G]}


def lat_last_trace() -> dict:
    """Host-side stages of this thread's last latency-lane batch
    (sv_lat_last_trace, include/stellar_sigverify.h), in microseconds."""
    buf = (ctypes.c_double * 8)()
    _check(load_library().sv_lat_last_trace(buf))
    return dict(zip(LAT_TRACE_FIELDS, list(buf)))
