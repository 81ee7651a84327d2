"""Constants of the kernels, read from the sources they are built from
(stellar-core_amd/csrc), for the launch wrappers (tests/launchers.py) and for
the CPU tests that share their record and table layouts (no torch here)."""
import os
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stellar-core_amd", "csrc")


def _define(header, name):
    """The integer value of `#define name <literal>` in csrc/header, read from the source the kernels are built from."""
    with open(os.path.join(_CSRC, header)) as fh:
        m = re.search(r"^#define\s+%s\s+(0[xX][0-9a-fA-F]+|\d+)[uU]?\b" % re.escape(name), fh.read(), re.M)
    assert m, "%s: no #define %s" % (header, name)
    return int(m.group(1), 0)


SV_KP_OCT_HI, SV_KP_OCT_HI_WIDE, SV_KP_IN_PLACE = (_define("keytab.h", n) for n in
                                                   ("SV_KP_OCT_HI", "SV_KP_OCT_HI_WIDE", "SV_KP_IN_PLACE"))
SV_KEY_BAD, SV_KEY_OK = _define("comb.h", "SV_KEY_BAD"), _define("comb.h", "SV_KEY_OK")
SV_COMB_CHAIN_WAVES = _define("comb.h", "SV_COMB_CHAIN_WAVES")  # chain waves per comb workgroup
SV_OSIGS = _define("sv_kernels.hip", "SV_OSIGS")                # signatures per octet workgroup
# test knobs of the throughput launches (sv_kparams::dbg; defined beside the kernels that read them)
SV_DBG_TRIVIAL_PAIR, SV_DBG_MAX_WINDOWS, SV_DBG_PREP_ONLY = (_define("sv_kernels.hip", n) for n in
                                                             ("SV_DBG_TRIVIAL_PAIR", "SV_DBG_MAX_WINDOWS",
                                                              "SV_DBG_PREP_ONLY"))
# the prep kernel's hand-over: record flags, table geometry, the per-key store
SV_REC_RNEG, SV_REC_TOP8A, SV_REC_TOP8R, SV_REC_OK = (_define("sv_kernels.hip", n) for n in
                                                      ("SV_REC_RNEG", "SV_REC_TOP8A", "SV_REC_TOP8R", "SV_REC_OK"))
REC_FLAGS = (SV_REC_RNEG, SV_REC_TOP8A, SV_REC_TOP8R, SV_REC_OK)
SV_ATAB_ENTRIES, SV_LTAB_QUADS = _define("verify_core.h", "SV_ATAB_ENTRIES"), _define("verify_core.h", "SV_LTAB_QUADS")
SV_SLOT_QUADS_L = 2 * SV_ATAB_ENTRIES * SV_LTAB_QUADS
SV_QSIGS, SV_QENT = _define("sv_kernels.hip", "SV_QSIGS"), _define("sv_kernels.hip", "SV_QENT")
SV_QSLOT_QUADS = 2 * SV_ATAB_ENTRIES * SV_QENT // 4
SV_KT_NONE, SV_KT_TQUADS = _define("keytab.h", "SV_KT_NONE"), _define("keytab.h", "SV_KT_TQUADS")
SV_LAT_MIN_WINDOWS = _define("lattice.h", "SV_LAT_MIN_WINDOWS")
