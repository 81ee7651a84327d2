"""ctypes prototypes of the kernel launchers (stellar-core_amd/csrc/launch.h)
and checked wrappers over torch tensors, so a test can pick the kernel
instantiation itself -- message mode, signatures per wave, path, hint bits --
at a tiny n instead of leaving it to the device's size and the batch's.

Every wrapper checks on the host, before it launches, that every index the
kernels will use lies inside its buffer (buffer sizes against the launchers'
own size queries, key slots against the table, message ranges against the
message buffer, the 16-byte alignment the kernels' quad loads need): a bad
test input fails as a Python assertion, never as a GPU fault.  Each wrapper
synchronises before it returns, so its tensors outlive the kernels.
"""
import ctypes

import numpy as np
import torch

from kernel_defs import (REC_FLAGS, SV_ATAB_ENTRIES, SV_COMB_CHAIN_WAVES, SV_DBG_MAX_WINDOWS,  # noqa: F401
                         SV_DBG_PREP_ONLY, SV_DBG_TRIVIAL_PAIR, SV_KEY_BAD, SV_KEY_OK, SV_KP_IN_PLACE, SV_KP_OCT_HI,
                         SV_KP_OCT_HI_WIDE, SV_KT_NONE, SV_KT_TQUADS, SV_LAT_MIN_WINDOWS, SV_LTAB_QUADS, SV_OSIGS,
                         SV_QENT, SV_QSIGS, SV_QSLOT_QUADS, SV_REC_OK, SV_REC_RNEG, SV_REC_TOP8A, SV_REC_TOP8R,
                         SV_SLOT_QUADS_L, _define)

PATH_ONE_LANE, PATH_OCTET, PATH_QUAD = 1, 2, 3
GUARD_BYTES, FILL = 4096, 0xA5
MSG_PAD = 32  # bytes after the last message: the latency loaders read whole aligned 16-byte blocks

_vp, _sz, _u32, _u64, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int


class sv_ktparams(ctypes.Structure):
    """keytab.h struct sv_ktparams"""
    _fields_ = [("index", _vp), ("store", _vp), ("kslot", _vp), ("builders", _vp), ("count", _vp), ("mask", _u64),
                ("limit", _u32), ("salt", _u64)]


def prototypes(lib):
    """Sets the launch.h prototypes on the engine library; returns it."""
    lib.sv_btab_bytes.restype = _sz
    lib.sv_btab_bytes.argtypes = []
    lib.sv_launch_btab_init.restype = _int
    lib.sv_launch_btab_init.argtypes = [_vp, _vp]
    lib.sv_comb_btab_bytes.restype = _sz
    lib.sv_comb_btab_bytes.argtypes = []
    lib.sv_key_slot_bytes.restype = _sz
    lib.sv_key_slot_bytes.argtypes = []
    lib.sv_launch_comb_btab.restype = _int
    lib.sv_launch_comb_btab.argtypes = [_vp, _vp]
    lib.sv_launch_keytab.restype = _int
    lib.sv_launch_keytab.argtypes = [_vp, _vp, _u32, _vp, _vp, _vp]
    lib.sv_launch_comb.restype = _int
    lib.sv_launch_comb.argtypes = [_int, _int, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.sv_verify_ws_bytes.restype = _sz
    lib.sv_verify_ws_bytes.argtypes = [_int, ctypes.c_uint, _u64]
    lib.sv_block_threads.restype = _int
    lib.sv_block_threads.argtypes = []
    lib.sv_occupancy_blocks_per_cu.restype = _int
    lib.sv_occupancy_blocks_per_cu.argtypes = []
    lib.sv_launch_verify.restype = _int
    lib.sv_launch_verify.argtypes = [_int, _int, ctypes.c_uint, _vp, _vp, _vp, _vp, _vp, _u32, _u64, _vp, _vp, _vp, _vp,
                                     _u32, _int, ctypes.POINTER(sv_ktparams), _vp, _vp]
    lib.sv_key_table_entry_bytes.restype = _sz
    lib.sv_key_table_entry_bytes.argtypes = []
    lib.sv_plan_chunk_max.restype = _u64
    lib.sv_plan_chunk_max.argtypes = [_u64]
    return lib


def _bytes_of(t):
    return t.numel() * t.element_size()


def _ptr(t):
    return None if t is None else t.data_ptr()


def check_bitmap(bm, want):
    """bm: the bitmap words of a launch of len(want) signatures plus one guard
    word preset to -1.  The bits equal the verdict bytes, the bits past n are
    0, and the word after the last is untouched."""
    n = len(want)
    words = (n + 63) // 64
    w = bm.view(np.uint64)
    bits = np.array([(int(w[i // 64]) >> (i % 64)) & 1 for i in range(64 * words)], np.uint8)
    assert (bits[:n] == want).all()
    assert not bits[n:].any()
    assert bm[words] == -1


class Batch:
    """A signature batch on the device with its host description.  mode 0: 32-byte
    messages at stride 32; 1: msg_off / msg_len; 2: fixed_len-byte messages at
    stride fixed_len.  host_msgs: one bytes object per row."""

    def __init__(self, dev, pk, sig, host_msgs, mode, want):
        n = len(host_msgs)
        assert pk.shape == (n, 32) and sig.shape == (n, 64) and len(want) == n and n > 0
        self.n, self.mode, self.want = n, mode, np.asarray(want, np.uint8)
        lens = np.array([len(m) for m in host_msgs], np.uint32)
        if mode == 0:
            assert (lens == 32).all()
        if mode == 2:
            assert (lens == lens[0]).all() and lens[0] != 32
        self.fixed_len = 0 if mode == 1 else int(lens[0])
        off = np.zeros(n, np.uint64)
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        self.h_off, self.h_len = off, lens
        blob = np.frombuffer(b"".join(host_msgs) + bytes(MSG_PAD), np.uint8)
        self.msg_bytes = int(lens.sum())
        self.pk = torch.from_numpy(np.array(pk, np.uint8)).to(dev)
        self.sig = torch.from_numpy(np.array(sig, np.uint8)).to(dev)
        self.msg = torch.from_numpy(blob.copy()).to(dev)
        self.off = torch.from_numpy(off.astype(np.int64)).to(dev)
        self.len = torch.from_numpy(lens.astype(np.int32)).to(dev)
        self.h_pk, self.h_sig, self.h_msgs = np.ascontiguousarray(pk), np.ascontiguousarray(sig), list(host_msgs)

    def check(self, n):
        """Everything a verify kernel of n signatures reads of the batch is inside its buffers."""
        assert 0 < n <= self.n
        assert _bytes_of(self.pk) >= 32 * n and _bytes_of(self.sig) >= 64 * n
        assert self.pk.data_ptr() % 16 == 0 and self.sig.data_ptr() % 16 == 0 and self.msg.data_ptr() % 16 == 0
        if self.mode == 1:
            assert self.off.numel() >= n and self.len.numel() >= n
            end = int((self.h_off[:n] + self.h_len[:n]).max())
        else:
            end = n * self.fixed_len
        assert end + 16 <= _bytes_of(self.msg), "message range (and its last 16-byte block) out of the buffer"

    def tiled(self, dev, n):
        """The batch repeated up to n rows (row i = row i mod self.n)."""
        r = np.arange(n) % self.n
        return Batch(dev, self.h_pk[r], self.h_sig[r], [self.h_msgs[i] for i in r], self.mode, self.want[r])

    def window(self, dev, start, n):
        """Rows start .. start + n - 1 as a batch of their own."""
        sel = np.arange(start, start + n)
        assert sel[-1] < self.n
        return Batch(dev, self.h_pk[sel], self.h_sig[sel], [self.h_msgs[i] for i in sel], self.mode, self.want[sel])


class Guarded:
    """A device buffer of nbytes, every byte preset to `fill`, with GUARD_BYTES
    of 0xA5 behind it that no kernel may touch.  t: the declared part."""

    def __init__(self, dev, nbytes, fill=FILL):
        self.nbytes = max(16, int(nbytes))
        self.full = torch.full((self.nbytes + GUARD_BYTES,), FILL, dtype=torch.uint8, device=dev)
        self.t = self.full[:self.nbytes]
        if fill != FILL:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0 and self.t.data_ptr() == self.full.data_ptr()

    def check(self, what=""):
        assert bool((self.full[self.nbytes:] == FILL).all()), (what, "bytes behind the buffer were written")

    def words(self):
        """the declared part on the host, as uint32"""
        return self.t.cpu().numpy().view(np.uint32)

    def data_ptr(self):
        return self.t.data_ptr()


class KeyStore:
    """The arrays of one sv_ktparams (keytab.h) for launches of up to n
    signatures: 2^k = mask + 1 slots, claims stop at `limit`.  index and count
    start at 0 (0 is their empty state); store, kslot and builders hold 0xA5."""

    def __init__(self, L, n, mask, limit, salt):
        assert mask + 1 > 0 and (mask + 1) & mask == 0 and 0 < limit <= mask + 1
        self.n, self.mask, self.limit, self.salt = n, mask, limit, salt
        self.entry_bytes = L.lib.sv_key_table_entry_bytes()
        self.chunk = L.lib.sv_plan_chunk_max(n)
        self.index = Guarded(L.dev, 8 * (mask + 1), 0)
        self.store = Guarded(L.dev, (mask + 1) * self.entry_bytes)
        self.kslot = Guarded(L.dev, 4 * self.chunk)
        self.builders = Guarded(L.dev, 4 * self.chunk)
        self.count = Guarded(L.dev, 16, 0)
        self.count.nbytes = 8  # (two words; the buffer cannot be shorter than a quad)

    def params(self, n):
        assert n <= self.n and self.kslot.nbytes >= 4 * self.chunk and self.builders.nbytes >= 4 * self.chunk
        assert self.count.nbytes == 8 and self.index.nbytes == 8 * (self.mask + 1)
        assert self.store.nbytes == (self.mask + 1) * self.entry_bytes and self.store.data_ptr() % 16 == 0
        return sv_ktparams(self.index.data_ptr(), self.store.data_ptr(), self.kslot.data_ptr(),
                           self.builders.data_ptr(), self.count.data_ptr(), self.mask, self.limit, self.salt)

    def check(self):
        for g in (self.index, self.store, self.kslot, self.builders):
            g.check("sv_ktparams")
        assert bool((self.count.full[8:16] == 0).all()) and bool((self.count.full[16:] == FILL).all()), "count[2..]"


class Verdicts(tuple):
    """(verdicts, bitmap words + 1 guard word, status word) of a verify launch; .ws: its workspace (Guarded)."""
    ws = None


class Launchers:
    def __init__(self, lib, dev):
        self.lib, self.dev = prototypes(lib), dev
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def _alloc(self, nbytes, fill=0):
        """A uint8 device tensor of exactly nbytes (at least 16), 16-byte aligned."""
        t = torch.full((max(16, int(nbytes)),), fill, dtype=torch.uint8, device=self.dev)
        assert t.data_ptr() % 16 == 0
        return t

    def _done(self, rc, what):
        assert rc == 0, "%s: hipError %d" % (what, rc)
        torch.cuda.synchronize(self.dev)

    # ---- throughput / cold latency tables and launches (sv_kernels.hip)
    def guarded(self, nbytes, fill=FILL):
        return Guarded(self.dev, nbytes, fill)

    def btab(self):
        """Both base-point tables, built into a buffer preset to 0xA5 with a guard behind it."""
        g = self.guarded(self.lib.sv_btab_bytes())
        assert g.nbytes >= self.lib.sv_btab_bytes()
        self._done(self.lib.sv_launch_btab_init(g.data_ptr(), self.stream), "sv_launch_btab_init")
        g.check("sv_launch_btab_init")
        return g.t

    def workspace(self, path, n):
        """A caller-owned workspace for verify(ws=...) of up to n signatures on `path`."""
        need = self.lib.sv_verify_ws_bytes(path, self._grid(n), n)
        assert need > 0
        return self.guarded(need)

    def keystore(self, n, mask=1023, limit=None, salt=0x5eed5eed5eed5eed):
        return KeyStore(self, n, mask, mask + 1 if limit is None else limit, salt)

    def _grid(self, n):
        bt = self.lib.sv_block_threads()
        return max(1, min(self.cus * self.lib.sv_occupancy_blocks_per_cu(), (n + bt - 1) // bt))

    def ws_layout(self, n):
        """Of a one-lane-path workspace for n signatures: (cap, dword offset of the records, dwords per record,
        dword offset of the wave window counts); the tables of signature li start at dword li * 4 * SV_SLOT_QUADS_L."""
        cap = self.lib.sv_plan_chunk_max(n)
        need = self.lib.sv_verify_ws_bytes(PATH_ONE_LANE, 1, n)
        rec_bytes = (need - cap // 64 * 4) // cap - 16 * SV_SLOT_QUADS_L
        assert rec_bytes % 16 == 0 and cap * (16 * SV_SLOT_QUADS_L + rec_bytes) + cap // 64 * 4 == need
        rec0 = cap * 4 * SV_SLOT_QUADS_L
        return cap, rec0, rec_bytes // 4, rec0 + cap * rec_bytes // 4

    def verify(self, b, n, path, btab, dbg=0, bitmap=True, ws=None, kt=None):
        """sv_launch_verify of the first n rows of b -> Verdicts (verdicts, bitmap words + 1 guard word, status
        word), its .ws the workspace: ws (a Guarded of workspace()) or one allocated here.  kt: a KeyStore."""
        b.check(n)
        assert path in (PATH_ONE_LANE, PATH_OCTET, PATH_QUAD)
        knobs = SV_DBG_TRIVIAL_PAIR | SV_DBG_MAX_WINDOWS | SV_DBG_PREP_ONLY
        assert dbg & ~(SV_KP_OCT_HI | SV_KP_OCT_HI_WIDE | SV_KP_IN_PLACE | knobs) == 0
        assert not (dbg & SV_DBG_PREP_ONLY) or path == PATH_ONE_LANE
        assert kt is None or (path == PATH_ONE_LANE and not dbg & SV_KP_IN_PLACE)
        grid = self._grid(n)
        need = self.lib.sv_verify_ws_bytes(path, grid, n)
        if ws is None:
            ws = self.guarded(need) if need else None
        else:
            # the whole launch is one chunk, so the workspace holds every signature's state afterwards
            assert need > 0 and (path != PATH_ONE_LANE or self.lib.sv_plan_chunk_max(n) >= n)
        assert ws is None or (ws.nbytes >= need and ws.data_ptr() % 16 == 0)
        assert _bytes_of(btab) >= self.lib.sv_btab_bytes()
        ktp = kt.params(n) if kt is not None else None
        out = torch.full((n + 64,), 7, dtype=torch.uint8, device=self.dev)
        words = (n + 63) // 64
        bm = torch.full((words + 1,), -1, dtype=torch.int64, device=self.dev)
        status = torch.zeros(4, dtype=torch.int32, device=self.dev)
        rc = self.lib.sv_launch_verify(b.mode, path, grid, _ptr(b.pk), _ptr(b.sig), _ptr(b.msg),
                                       _ptr(b.off) if b.mode == 1 else None, _ptr(b.len) if b.mode == 1 else None,
                                       b.fixed_len, n, _ptr(out), _ptr(bm) if bitmap else None, _ptr(ws), _ptr(btab),
                                       dbg, 0, ctypes.byref(ktp) if ktp is not None else None, _ptr(status),
                                       self.stream)
        self._done(rc, "sv_launch_verify")
        got = out.cpu().numpy()
        assert (got[n:] == 7).all(), "bytes after verdict[n] were written"
        if ws is not None:
            ws.check("sv_launch_verify workspace")
        if kt is not None:
            kt.check()
        res = Verdicts((got[:n], bm.cpu().numpy(), int(status[0].item())))
        res.ws = ws
        return res

    # ---- warm latency path (sv_comb.hip)
    def comb_btab(self):
        g = self.guarded(self.lib.sv_comb_btab_bytes())
        self._done(self.lib.sv_launch_comb_btab(g.data_ptr(), self.stream), "sv_launch_comb_btab")
        g.check("sv_launch_comb_btab")
        return g.t

    def keytab(self, keys, slots, nslots, guard=0xA5):
        """Builds the tables of `keys` (k x 32 host bytes) into `slots` (k distinct
        slot numbers < nslots) of a table of nslots slots whose every byte is
        first set to `guard` -> (ktab, kstat) device tensors (uint8 / int32)."""
        keys = np.array(keys, np.uint8)
        slots = np.array(slots, np.uint32)
        k = keys.shape[0]
        assert keys.shape == (k, 32) and slots.shape == (k,) and k > 0
        assert len(set(slots.tolist())) == k and int(slots.max()) < nslots
        sb = self.lib.sv_key_slot_bytes()
        gk = self.guarded(nslots * sb, guard)
        ktab = gk.t
        kstat = torch.full((nslots,), 0x5A5A5A5A, dtype=torch.int32, device=self.dev)
        assert _bytes_of(ktab) >= nslots * sb and kstat.numel() >= nslots
        d_keys = torch.from_numpy(keys).to(self.dev)
        d_slots = torch.from_numpy(slots.astype(np.int32)).to(self.dev)
        assert d_keys.data_ptr() % 4 == 0 and _bytes_of(d_keys) >= 32 * k and d_slots.numel() >= k
        rc = self.lib.sv_launch_keytab(d_keys.data_ptr(), d_slots.data_ptr(), k, ktab.data_ptr(), kstat.data_ptr(),
                                       self.stream)
        self._done(rc, "sv_launch_keytab")
        gk.check("sv_launch_keytab")
        return ktab, kstat

    def comb(self, b, n, spw, kslot, ktab, kstat, ctab):
        """sv_launch_comb<b.mode, spw> of the first n rows of b; kslot: host uint32 array, a slot per row."""
        b.check(n)
        assert spw in (1, 2, 4)
        kslot = np.ascontiguousarray(kslot, np.uint32)
        nslots = kstat.numel()
        assert kslot.shape[0] >= n and int(kslot[:n].max()) < nslots, "kslot out of the table"
        assert _bytes_of(ktab) >= nslots * self.lib.sv_key_slot_bytes()
        assert _bytes_of(ctab) >= self.lib.sv_comb_btab_bytes()
        assert ktab.data_ptr() % 16 == 0 and ctab.data_ptr() % 16 == 0 and self.lib.sv_key_slot_bytes() % 16 == 0
        d_kslot = torch.from_numpy(kslot.astype(np.int32)).to(self.dev)
        out = torch.full((n + 64,), 7, dtype=torch.uint8, device=self.dev)
        rc = self.lib.sv_launch_comb(b.mode, spw, _ptr(b.pk), _ptr(b.sig), _ptr(b.msg),
                                     _ptr(b.off) if b.mode == 1 else None, _ptr(b.len) if b.mode == 1 else None,
                                     b.fixed_len, n, _ptr(out), d_kslot.data_ptr(), ktab.data_ptr(), kstat.data_ptr(),
                                     ctab.data_ptr(), self.stream)
        self._done(rc, "sv_launch_comb")
        got = out.cpu().numpy()
        assert (got[n:] == 7).all(), "bytes after verdict[n] were written"
        return got[:n]
