"""ctypes binding of libdmx.so (the C-ABI declared in include/dmx.h).

The product path has exactly one compute backend: the HIP kernels in libdmx.so.  If the
library is missing or no GPU is visible, the calls raise — there is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# DMX_LIBDMX: an alternative in-tree build of the same library (A/B kernel variants)
# DMX_LIBDIR: a directory with another build of every library (host sanitizer builds)
# DMX_DEBUG_BOUNDS=1: the bounds-checking build (every gather and slot access checked; a
#   violation fails the call naming the kernel), dmx/libdmx_bounds.so
BOUNDS = os.environ.get("DMX_DEBUG_BOUNDS", "") not in ("", "0")
LIB_PATH = os.environ.get("DMX_LIBDMX") or os.path.join(
    os.environ.get("DMX_LIBDIR") or HERE, "libdmx_bounds.so" if BOUNDS else "libdmx.so")

DMX_FRONT, DMX_BACK, DMX_RC = 0x01, 0x02, 0x10
DMX_ANCHORED, DMX_NONINTERNAL = 0x04, 0x08   # with DMX_FRONT / DMX_BACK: ^A, A$ / XA, AX
MODE_SINGLE, MODE_TWO_ROUND, MODE_LINKED = 0, 1, 2
PACK_PAD = 64

MATCH_FIELDS = [("rstart", "<i4"), ("rstop", "<i4"), ("astart", "<i2"), ("astop", "<i2"),
                ("score", "<i2"), ("errors", "<i2")]
RESULT_DTYPE = np.dtype([("bin1", "<i2"), ("bin2", "<i2"), ("rc1", "u1"), ("rc2", "u1"),
                         ("flags", "u1"), ("pad", "u1")]
                        + [("m1_" + n, t) for n, t in MATCH_FIELDS]
                        + [("m2_" + n, t) for n, t in MATCH_FIELDS])
assert RESULT_DTYPE.itemsize == 40

EXPORTS = ["dmx_abi_version", "dmx_open", "dmx_close", "dmx_last_error", "dmx_set_panel",
           "dmx_set_panel_mixed", "dmx_set_mode", "dmx_pack_words", "dmx_pack", "dmx_run", "dmx_load", "dmx_exec",
           "dmx_sync", "dmx_fetch", "dmx_counts", "dmx_stats", "dmx_device_count",
           "dmx_run_multi", "dmx_locate", "dmx_chop_set", "dmx_chop_exec", "dmx_chop_fetch",
           "dmx_chop_stats", "dmx_comm_unique_id", "dmx_comm_init_rank", "dmx_comm_init_all",
           "dmx_comm_size", "dmx_allreduce_counts", "dmx_debug_fetch", "dmx_run_sparse",
           "dmx_mask_exceptions", "dmx_host_register", "dmx_host_unregister", "dmx_panel_reach",
           "dmx_debug_bounds_selftest", "dmx_panel_pieces", "dmx_pairdist", "dmx_pairdist_host",
           "dmx_pairdist_group_sizes", "dmx_pairalign", "dmx_pairalign_host",
           "dmx_pairalign_stats", "dmx_groupalign", "dmx_groupalign_host", "dmx_groupalign_stats",
           "dmx_groupalign_strands", "dmx_groupalign_strands_host",
           "dmx_rowdist", "dmx_rowdist_host", "dmx_edgegroups", "dmx_edgegroups_host",
           "dmx_pairhits", "dmx_pairhits_fetch", "dmx_hitgroups", "dmx_pairhits_host",
           "dmx_hitgroups_host", "dmx_hitgroups_stats", "dmx_rowpairdist", "dmx_rowpairdist_host",
           "dmx_rowhits", "dmx_rowhits_host", "dmx_panel_piece_pairs", "dmx_hithist",
           "dmx_pairhits_cross", "dmx_hitgroups_within", "dmx_hithist_host",
           "dmx_pairhits_cross_host", "dmx_hitgroups_within_host", "dmx_panel_near_shared",
           "dmx_rowassign", "dmx_rowassign_host", "dmx_set_panel_ex", "dmx_ends_host",
           "dmx_set_views", "dmx_clear_views", "dmx_chop_views", "dmx_views_fetch",
           "dmx_chop_views_host", "dmx_exec_checked", "dmx_set_operands", "dmx_clear_operands",
           "dmx_operands_fetch", "dmx_operands_check_host", "dmx_result_operands",
           "dmx_result_operands_host"]
ABI_VERSION = 4
COMM_ID_BYTES = 128

LOC_IGNORE_CASE, LOC_ONLY_POSITIVE = 0x1, 0x2
# include/dmx.h dmx_pairdist: modes, the pair flag, the longest read
PD_NW, PD_HW, PD_RC, PD_MAX_LEN = 0, 1, 0x1, 16384
# include/dmx.h dmx_pairalign: the ops of an edit path (edlib's numbering)
PA_MATCH, PA_INSERT, PA_DELETE, PA_MISMATCH = 0, 1, 2, 3
# include/dmx.h dmx_edgegroups / dmx_pairhits: no label, no hit; an outcome's reverse bit
LG_NONE, LG_REV = 0xFFFFFFFF, 0x80000000
HIT_DTYPE = np.dtype([("seq", "<u8"), ("pattern", "<i4"), ("strand", "<i4"), ("start", "<i4"),
                      ("end", "<i4")])
assert HIT_DTYPE.itemsize == 24

# include/dmx.h dmx_chop_hit / dmx_chop_seg (pychopper-style reorientation)
CHOP_HIT_DTYPE = np.dtype([("read", "<u4"), ("label", "<i2"), ("dist", "<i2"), ("start", "<i4"),
                           ("stop", "<i4")])
CHOP_SEG_DTYPE = np.dtype([("read", "<u4"), ("start", "<i4"), ("stop", "<i4"),
                           ("strand", "<i2"), ("rule", "<i2")])
assert CHOP_HIT_DTYPE.itemsize == 16 and CHOP_SEG_DTYPE.itemsize == 16


# internal record layouts exposed by dmx_debug_fetch (csrc/dmx_device.h Window / Cand)
WINDOW_DTYPE = np.dtype([("item", "<u4"), ("o", "u1"), ("lastcol", "u1"), ("strand", "u1"),
                         ("bmin", "u1"), ("j1", "<u4"), ("j2", "<u4"), ("n", "<u4"),
                         ("start", "<u4"), ("len", "<u4"), ("info", "<u4"), ("off", "<u8")])
CAND_DTYPE = np.dtype([("item", "<u4"), ("sub", "<u2"), ("iend", "u1"), ("cost", "u1"),
                       ("j", "<u4"), ("n", "<u4"), ("start", "<u4"), ("len", "<u4"),
                       ("strand", "u1"), ("o", "u1"), ("a", "u1"), ("clean", "u1"), ("pad2", "<u4"),
                       ("off", "<u8")])
assert WINDOW_DTYPE.itemsize == 40 and CAND_DTYPE.itemsize == 40
DBG_WINDOWS, DBG_VERIFIED, DBG_TASKS, DBG_CANDS0, DBG_CANDS1, DBG_FLAGS = range(6)


class DmxError(RuntimeError):
    pass


_lib = None


def load() -> ctypes.CDLL:
    """Load libdmx.so (built by `make -C nanopore-barcoding-orc_amd`); raise if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DmxError(f"{LIB_PATH} not built: run `make -C nanopore-barcoding-orc_amd` "
                       "(the HIP extension is required; there is no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    P, c_int, c_size, c_u64p = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
    L.dmx_abi_version.restype = c_int
    L.dmx_open.argtypes = [c_int, ctypes.POINTER(P)]
    L.dmx_close.argtypes = [P]
    L.dmx_close.restype = None
    L.dmx_last_error.argtypes = [P]
    L.dmx_last_error.restype = ctypes.c_char_p
    L.dmx_set_panel.argtypes = [P, c_int, ctypes.POINTER(ctypes.c_char_p),
                                ctypes.POINTER(c_int), c_int, ctypes.c_double, c_int, c_int]
    L.dmx_set_panel_mixed.argtypes = [P, c_int, ctypes.POINTER(ctypes.c_char_p),
                                      ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int,
                                      ctypes.c_double, c_int, c_int]
    L.dmx_set_mode.argtypes = [P, c_int]
    # (guarded only so that DMX_LIBDMX / DMX_ALLOW_ABI can load an older in-tree build for an
    # A/B run of panels that need neither call; EXPORTS and tests/test_host.py require both)
    if hasattr(L, "dmx_set_panel_ex"):
        L.dmx_set_panel_ex.argtypes = [P, c_int, ctypes.POINTER(ctypes.c_char_p),
                                       ctypes.POINTER(c_int), ctypes.POINTER(c_int), P, c_int,
                                       ctypes.c_double, c_int, c_int]
        L.dmx_ends_host.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int),
                                    ctypes.POINTER(c_int), P, c_int, ctypes.c_double, c_int,
                                    c_int, P, P, c_u64p, P, c_size, P]
    L.dmx_pack_words.argtypes = [ctypes.c_uint64, c_size]
    L.dmx_pack_words.restype = c_size
    L.dmx_pack.argtypes = [P, c_u64p, P, c_size, P, P, c_u64p]
    L.dmx_run.argtypes = [P, P, P, c_u64p, P, c_size, c_size, P]
    L.dmx_load.argtypes = [P, P, P, c_u64p, P, c_size, c_size]
    L.dmx_exec.argtypes = [P]
    L.dmx_sync.argtypes = [P]
    L.dmx_fetch.argtypes = [P, P]
    L.dmx_counts.argtypes = [P, c_u64p, c_size]
    L.dmx_stats.argtypes = [P, ctypes.POINTER(ctypes.c_float), c_int, c_u64p, c_int,
                            ctypes.POINTER(c_int)]
    L.dmx_device_count.restype = c_int
    L.dmx_run_multi.argtypes = [ctypes.POINTER(P), c_int, P, P, c_u64p, P, c_size, c_size, P, c_u64p, c_size]
    L.dmx_locate.argtypes = [P, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int), c_int,
                             c_int, P, c_u64p, P, c_size, P, c_size,
                             ctypes.POINTER(ctypes.c_uint64)]
    L.dmx_chop_set.argtypes = [P, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int), c_int,
                               ctypes.POINTER(c_int), ctypes.POINTER(c_int),
                               ctypes.POINTER(c_int), c_int, ctypes.c_double, c_int]
    L.dmx_chop_exec.argtypes = [P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.dmx_chop_fetch.argtypes = [P, P, P, P, c_size, P, c_size]
    L.dmx_chop_stats.argtypes = [P, ctypes.POINTER(ctypes.c_float), c_int]
    if hasattr(L, "dmx_set_views"):
        L.dmx_set_views.argtypes = [P, P, P, P, P, c_size]
        L.dmx_clear_views.argtypes = [P]
        L.dmx_exec_checked.argtypes = [P]
        L.dmx_chop_views.argtypes = [P, P, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]
        L.dmx_views_fetch.argtypes = [P, P, P, P, P, c_size]
        L.dmx_chop_views_host.argtypes = [P, P, P, ctypes.c_int32, c_size, P, P, P, P, c_size]
    if hasattr(L, "dmx_set_operands"):
        L.dmx_set_operands.argtypes = [P, P, P, P, P, c_size]
        L.dmx_clear_operands.argtypes = [P]
        L.dmx_operands_fetch.argtypes = [P, P, P, P, P, c_size]
        L.dmx_operands_check_host.argtypes = [P, c_size, P, P, P, P, c_size]
        L.dmx_result_operands.argtypes = [P, P, c_size, ctypes.c_int32, c_u64p, c_size,
                                          ctypes.POINTER(ctypes.c_uint64)]
        L.dmx_result_operands_host.argtypes = [P, c_size, P, P, P, P, P, c_size, c_int, P, c_int,
                                               P, c_int, P, c_size, ctypes.c_int32, P, P, P, P,
                                               c_size, c_u64p, c_size,
                                               ctypes.POINTER(ctypes.c_uint64)]
    L.dmx_comm_unique_id.argtypes = [P]
    L.dmx_comm_init_rank.argtypes = [P, P, c_int, c_int]
    L.dmx_comm_init_all.argtypes = [ctypes.POINTER(P), c_int]
    L.dmx_comm_size.argtypes = [P]
    L.dmx_allreduce_counts.argtypes = [P, c_u64p, c_size]
    L.dmx_debug_fetch.argtypes = [P, c_int, c_int, P, c_size]
    L.dmx_run_sparse.argtypes = [P, P, P, P, c_size, c_u64p, P, c_size, c_size, P]
    L.dmx_mask_exceptions.argtypes = [P, c_size, P, P, c_size]
    L.dmx_mask_exceptions.restype = c_size
    L.dmx_host_register.argtypes = [P, c_size]
    L.dmx_host_unregister.argtypes = [P]
    if hasattr(L, "dmx_panel_reach"):
        L.dmx_panel_reach.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int), P,
                                      c_int, ctypes.c_double, c_int, c_int, P, c_int]
        L.dmx_debug_bounds_selftest.argtypes = [P, P]
    if hasattr(L, "dmx_panel_near_shared"):
        L.dmx_panel_near_shared.argtypes = L.dmx_panel_reach.argtypes
    if hasattr(L, "dmx_panel_pieces"):
        L.dmx_panel_pieces.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int),
                                       c_int, ctypes.c_double, c_int, c_int, P, c_int, P, c_int]
    if hasattr(L, "dmx_panel_piece_pairs"):
        L.dmx_panel_piece_pairs.argtypes = [ctypes.POINTER(ctypes.c_char_p),
                                            ctypes.POINTER(c_int), c_int, ctypes.c_double, c_int,
                                            c_int, P, P, P, c_int]
    if hasattr(L, "dmx_pairdist"):
        L.dmx_pairdist.argtypes = [P, c_int, P, P, P, P, c_size, P]
        L.dmx_pairdist_host.argtypes = [c_int, P, P, c_u64p, P, c_size, P, P, P, P, c_size, P,
                                        c_int]
        L.dmx_pairdist_ms.argtypes = [P]
        L.dmx_pairdist_ms.restype = ctypes.c_float
        L.dmx_pairdist_group_sizes.argtypes = [ctypes.POINTER(c_int), c_int]
    if hasattr(L, "dmx_pairalign"):
        L.dmx_pairalign.argtypes = [P, P, P, P, c_size, P, c_u64p, P, c_size]
        L.dmx_pairalign_host.argtypes = [P, P, c_u64p, P, c_size, P, P, P, c_size, P, c_u64p, P,
                                         c_size, c_int]
        L.dmx_pairalign_ms.argtypes = [P]
        L.dmx_pairalign_ms.restype = ctypes.c_float
        L.dmx_pairalign_stats.argtypes = [P, ctypes.POINTER(ctypes.c_float), c_int]
    if hasattr(L, "dmx_groupalign"):
        ga = [c_size, P, c_u64p, P, c_u64p, ctypes.c_uint32, c_u64p, P, P, P, c_size, P, c_u64p, P,
              c_size]
        L.dmx_groupalign.argtypes = [P] + ga
        L.dmx_groupalign_host.argtypes = [P, P, c_u64p, P, c_size] + ga + [c_int]
    if hasattr(L, "dmx_groupalign_strands"):
        gs = ga[:4] + [P] + ga[4:]   # member_flags after members
        L.dmx_groupalign_strands.argtypes = [P] + gs
        L.dmx_groupalign_strands_host.argtypes = [P, P, c_u64p, P, c_size] + gs + [c_int]
        L.dmx_groupalign_stats.argtypes = [P, ctypes.POINTER(ctypes.c_float), c_int,
                                           ctypes.POINTER(c_int)]
    if hasattr(L, "dmx_rowdist"):
        L.dmx_rowdist.argtypes = [P, c_size, P, c_u64p, P, P, P, c_size, P]
        L.dmx_rowdist_host.argtypes = [P, P, c_u64p, P, c_size, c_size, P, c_u64p, P, P, P, c_size,
                                       P, c_int]
        L.dmx_rowdist_ms.argtypes = [P]
        L.dmx_rowdist_ms.restype = ctypes.c_float
    if hasattr(L, "dmx_rowassign"):
        u64 = ctypes.c_uint64
        ra = [c_size, P, c_u64p, P, c_size, P, P, P, c_size, P, c_size, u64, u64, P, P, P,
              ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.dmx_rowassign.argtypes = [P] + ra
        L.dmx_rowassign_host.argtypes = [P, P, c_u64p, P, c_size] + ra + [c_int]
        L.dmx_rowassign_ms.argtypes = [P]
        L.dmx_rowassign_ms.restype = ctypes.c_float
    if hasattr(L, "dmx_edgegroups"):
        L.dmx_edgegroups.argtypes = [P, P, P, c_size, ctypes.c_uint32, P]
        L.dmx_edgegroups_host.argtypes = [P, P, c_size, ctypes.c_uint32, P]
        L.dmx_pairhits.argtypes = [P, P, P, P, P, c_size, P, ctypes.POINTER(ctypes.c_uint64)]
        L.dmx_pairhits_fetch.argtypes = [P, P, P, P, c_size, ctypes.POINTER(c_size)]
        L.dmx_hitgroups.argtypes = [P, P, P]
        L.dmx_pairhits_host.argtypes = [P, P, c_u64p, P, c_size, P, P, P, P, c_size, P, P,
                                        ctypes.POINTER(ctypes.c_uint64), c_int]
        L.dmx_hitgroups_host.argtypes = [P, P, P, c_size, P, c_size, P]
        L.dmx_hitgroups_stats.argtypes = [P, ctypes.POINTER(ctypes.c_float), c_int]
    if hasattr(L, "dmx_hithist"):
        L.dmx_hithist.argtypes = [P, P, P, c_size, ctypes.c_uint32, P]
        L.dmx_pairhits_cross.argtypes = [P, P, P, P, P, P, c_size, ctypes.POINTER(c_size)]
        L.dmx_hitgroups_within.argtypes = [P, P, P, P, P, c_size, ctypes.c_uint32, P]
        L.dmx_hithist_host.argtypes = [P, P, c_size, c_size, P, P, c_size, ctypes.c_uint32, P]
        L.dmx_pairhits_cross_host.argtypes = [P, P, P, c_size, c_size, P, P, P, P, P, c_size,
                                              ctypes.POINTER(c_size)]
        L.dmx_hitgroups_within_host.argtypes = [P, P, P, c_size, c_size, P, P, P, P, c_size,
                                                ctypes.c_uint32, P]
    if hasattr(L, "dmx_rowpairdist"):
        rr = [c_int, c_size, P, c_u64p, P, P]   # mode, n_rows, masks, row_off, q, t
        L.dmx_rowpairdist.argtypes = [P] + rr + [P, P, c_size, P]
        L.dmx_rowpairdist_host.argtypes = rr + [P, P, c_size, P, c_int]
        hits = [P, c_size, P, P, P, c_size, ctypes.POINTER(c_size)]
        L.dmx_rowhits.argtypes = [P] + rr + hits
        L.dmx_rowhits_host.argtypes = rr + hits + [c_int]
        L.dmx_rowhits_ms.argtypes = [P]
        L.dmx_rowhits_ms.restype = ctypes.c_float
    # DMX_ALLOW_ABI=1: load an older in-tree build for a regression A/B (tools/replay_sweep.py)
    if L.dmx_abi_version() != ABI_VERSION and os.environ.get("DMX_ALLOW_ABI") != "1":
        raise DmxError("libdmx ABI mismatch")
    _lib = L
    return L


class Packed:
    """A batch of reads in the device layout: 2-bit codes + no-match mask (see include/dmx.h)."""

    def __init__(self, seq2b: np.ndarray, nmask: np.ndarray, offsets: np.ndarray,
                 lengths: np.ndarray):
        self.seq2b, self.nmask, self.offsets, self.lengths = seq2b, nmask, offsets, lengths

    @property
    def n_reads(self) -> int:
        return int(len(self.lengths))

    def exceptions(self):
        """The no-match mask's nonzero words as (indices, values) (dmx_mask_exceptions)."""
        if getattr(self, "_exc", None) is None:
            L = load()
            n = L.dmx_mask_exceptions(self.nmask.ctypes.data, self.n_words, None, None, 0)
            idx = np.empty(max(n, 1), dtype=np.uint32)
            val = np.empty(max(n, 1), dtype=np.uint32)
            L.dmx_mask_exceptions(self.nmask.ctypes.data, self.n_words, idx.ctypes.data,
                                  val.ctypes.data, n)
            self._exc = (idx[:n], val[:n])
        return self._exc

    @property
    def n_words(self) -> int:
        return int(len(self.seq2b))


def pack(ascii_blob: np.ndarray, offsets: np.ndarray, lengths: np.ndarray) -> Packed:
    """Pack ASCII reads (uint8 blob + per-read offset/length) with the library's host packer."""
    L = load()
    blob = np.ascontiguousarray(ascii_blob, dtype=np.uint8)
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    lens = np.ascontiguousarray(lengths, dtype=np.uint32)
    n = len(lens)
    words = L.dmx_pack_words(int(lens.sum(dtype=np.uint64)), n)
    seq = np.empty(words, dtype=np.uint32)
    nm = np.empty(words, dtype=np.uint32)
    out_offs = np.empty(n, dtype=np.uint64)
    rc = L.dmx_pack(blob.ctypes.data if len(blob) else None, offs.ctypes.data, lens.ctypes.data,
                    n, seq.ctypes.data, nm.ctypes.data, out_offs.ctypes.data)
    if rc != 0:
        raise DmxError(f"dmx_pack failed ({rc})")
    return Packed(seq, nm, out_offs, lens)


def adapter_wheres(ads) -> list:
    """The dmx_set_panel_ex `wheres` of parsed single adapters (dmx.panel.Adapter)."""
    bits = {"": 0, "anchored": DMX_ANCHORED, "noninternal": DMX_NONINTERNAL}
    return [(DMX_FRONT if a.where == "front" else DMX_BACK) | bits[getattr(a, "restrict", "")]
            for a in ads]


def ends_host(seqs, wheres, p: "Packed", rc: bool, max_errors: float = 0.1, min_overlap: int = 3,
              min_overlaps=None) -> np.ndarray:
    """Host only (no GPU): one single round of the panel dmx_set_panel_ex would build, by the
    full-matrix DP of dmx_ends_host; RESULT_DTYPE records as Context.run writes them."""
    L = load()
    arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
    lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
    wh = (ctypes.c_int * len(seqs))(*wheres)
    mo = None
    if min_overlaps is not None:
        mo = (ctypes.c_int * len(seqs))(*[int(min_overlap if x is None else x)
                                          for x in min_overlaps])
    out = np.zeros(p.n_reads, dtype=RESULT_DTYPE)
    rc_ = L.dmx_ends_host(arr, lens, wh, mo, len(seqs), float(max_errors), int(min_overlap),
                          int(bool(rc)), p.seq2b.ctypes.data, p.nmask.ctypes.data,
                          p.offsets.ctypes.data, p.lengths.ctypes.data, p.n_reads,
                          out.ctypes.data)
    if rc_ != 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"dmx_ends_host failed ({rc_}): {msg.decode() if msg else ''}")
    return out


class Context:
    """One device context (include/dmx.h: one per GPU, one host thread per context)."""

    def __init__(self, device: int = 0):
        self._L = load()
        h = ctypes.c_void_p()
        rc = self._L.dmx_open(int(device), ctypes.byref(h))
        if rc != 0:
            raise DmxError(f"dmx_open(device={device}) failed ({rc}): no usable HIP device")
        self._h = h
        self.device = device
        self.panel_sizes = [0, 0]
        self.mode = MODE_SINGLE
        self._n_loaded = 0
        self._n_views = None   # views of a view run (set_views / chop_views), None: whole reads
        self._n_exec = None    # items of the last exec's round 0: what fetch returns

    def close(self):
        if getattr(self, "_h", None):
            self._L.dmx_close(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str) -> int:
        if rc < 0:
            msg = self._L.dmx_last_error(self._h)
            raise DmxError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        return rc

    def set_panel(self, rnd: int, seqs, flags: int, max_errors: float = 0.1,
                  min_overlap: int = 3):
        arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
        lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
        self._check(self._L.dmx_set_panel(self._h, rnd, arr, lens, len(seqs), float(max_errors),
                                          int(min_overlap), int(flags)), "dmx_set_panel")
        self.panel_sizes[rnd] = len(seqs)

    def set_panel_mixed(self, rnd: int, seqs, wheres, rc: bool, max_errors: float = 0.1,
                        min_overlap: int = 3):
        """Per-adapter DMX_FRONT / DMX_BACK (a cutadapt call mixing -g and -a)."""
        arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
        lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
        wh = (ctypes.c_int * len(seqs))(*wheres)
        self._check(self._L.dmx_set_panel_mixed(self._h, rnd, arr, lens, wh, len(seqs),
                                                float(max_errors), int(min_overlap), int(rc)),
                    "dmx_set_panel_mixed")
        self.panel_sizes[rnd] = len(seqs)

    def set_panel_ex(self, rnd: int, seqs, wheres, rc: bool, max_errors: float = 0.1,
                     min_overlap: int = 3, min_overlaps=None):
        """dmx_set_panel_ex: wheres[a] = DMX_FRONT / DMX_BACK, alone or with DMX_ANCHORED /
        DMX_NONINTERNAL; min_overlaps[a] (None entries and None: min_overlap)."""
        arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
        lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
        wh = (ctypes.c_int * len(seqs))(*wheres)
        mo = None
        if min_overlaps is not None:
            mo = (ctypes.c_int * len(seqs))(*[int(min_overlap if x is None else x)
                                              for x in min_overlaps])
        self._check(self._L.dmx_set_panel_ex(self._h, rnd, arr, lens, wh, mo, len(seqs),
                                             float(max_errors), int(min_overlap), int(rc)),
                    "dmx_set_panel_ex")
        self.panel_sizes[rnd] = len(seqs)

    def set_adapters(self, rnd: int, ads, rc: bool, max_errors: float = 0.1,
                     min_overlap: int = 3):
        """Round rnd's panel from parsed single adapters (dmx.panel.Adapter): one uniform
        unrestricted panel is dmx_set_panel, a mix of -g and -a dmx_set_panel_mixed, and a panel
        with anchored / non-internal adapters dmx_set_panel_ex."""
        seqs = [a.seq for a in ads]
        wheres = adapter_wheres(ads)
        if any(w & (DMX_ANCHORED | DMX_NONINTERNAL) for w in wheres):
            self.set_panel_ex(rnd, seqs, wheres, rc, max_errors, min_overlap,
                              [getattr(a, "min_overlap", None) for a in ads])
        elif len(set(wheres)) == 1:
            self.set_panel(rnd, seqs, wheres[0] | (DMX_RC if rc else 0), max_errors, min_overlap)
        else:
            self.set_panel_mixed(rnd, seqs, wheres, rc, max_errors, min_overlap)

    def bounds_selftest(self):
        """DMX_DEBUG_BOUNDS builds: (return code, message, the kernel's 3 outputs)."""
        out = np.zeros(3, dtype=np.uint32)
        rc = self._L.dmx_debug_bounds_selftest(self._h, out.ctypes.data)
        msg = self._L.dmx_last_error(self._h)
        return rc, (msg.decode() if msg else ""), out

    def set_mode(self, mode: int):
        self._check(self._L.dmx_set_mode(self._h, mode), "dmx_set_mode")
        self.mode = mode

    def run(self, p: Packed) -> np.ndarray:
        out = np.zeros(p.n_reads, dtype=RESULT_DTYPE)
        self._check(self._L.dmx_run(self._h, p.seq2b.ctypes.data, p.nmask.ctypes.data,
                                    p.offsets.ctypes.data, p.lengths.ctypes.data, p.n_words,
                                    p.n_reads, out.ctypes.data), "dmx_run")
        self._n_loaded = p.n_reads
        self._ops = None
        self._load_gen = getattr(self, "_load_gen", 0) + 1
        self._n_views = None
        self._n_exec = p.n_reads
        self._resident = None
        return out

    def run_sparse(self, p: Packed) -> np.ndarray:
        """dmx_run with the no-match mask uploaded as its exceptions (dmx_run_sparse)."""
        idx, val = p.exceptions()
        out = np.zeros(p.n_reads, dtype=RESULT_DTYPE)
        self._check(self._L.dmx_run_sparse(self._h, p.seq2b.ctypes.data, idx.ctypes.data,
                                           val.ctypes.data, len(idx), p.offsets.ctypes.data,
                                           p.lengths.ctypes.data, p.n_words, p.n_reads,
                                           out.ctypes.data), "dmx_run_sparse")
        self._n_loaded = p.n_reads
        self._ops = None
        self._load_gen = getattr(self, "_load_gen", 0) + 1
        self._n_views = None
        self._n_exec = p.n_reads
        self._resident = None
        return out

    def load(self, p: Packed):
        self._check(self._L.dmx_load(self._h, p.seq2b.ctypes.data, p.nmask.ctypes.data,
                                     p.offsets.ctypes.data, p.lengths.ctypes.data, p.n_words,
                                     p.n_reads), "dmx_load")
        self._n_loaded = p.n_reads
        self._ops = None
        self._load_gen = getattr(self, "_load_gen", 0) + 1
        self._n_views = None
        self._n_exec = None
        self._lengths = np.array(p.lengths, dtype=np.uint32)   # pairalign sizes its output by them
        self._resident = None   # sorter.assign's tag of the list whose batch is loaded

    def _round0_items(self) -> int:
        return self._n_views if self._n_views is not None else self._n_loaded

    def exec(self):
        self._check(self._L.dmx_exec(self._h), "dmx_exec")
        self._n_exec = self._round0_items()

    def exec_checked(self):
        """exec, waited for, run again with larger lists when one overflowed (what run does)."""
        self._check(self._L.dmx_exec_checked(self._h), "dmx_exec_checked")
        self._n_exec = self._round0_items()

    def sync(self):
        self._check(self._L.dmx_sync(self._h), "dmx_sync")

    def fetch(self) -> np.ndarray:
        """Results of the last exec: as many as its round 0 had items (the reads, or the views
        of a view run), recorded when it ran: a list set or cleared since does not change it."""
        n = self._n_exec   # dmx_fetch copies what the last exec computed, whatever was set since
        if n is None:      # no exec on this batch: the library refuses (DMX_E_STATE)
            n = self._n_loaded
        out = np.zeros(n, dtype=RESULT_DTYPE)
        self._check(self._L.dmx_fetch(self._h, out.ctypes.data if n else None), "dmx_fetch")
        return out

    # ---- views of the resident reads (include/dmx.h dmx_set_views) -----------
    def set_views(self, read, start, stop, strand):
        """Run on views of the resident reads from now on: view k = read[k][start[k]:stop[k]],
        reverse-complemented when strand[k] (Batch.pack_views' convention)."""
        arrs = [np.ascontiguousarray(read, dtype=np.uint32),
                np.ascontiguousarray(start, dtype=np.int32),
                np.ascontiguousarray(stop, dtype=np.int32),
                np.ascontiguousarray(strand, dtype=np.uint8)]
        n = len(arrs[0])
        if any(len(a) != n for a in arrs):
            raise ValueError("set_views: read, start, stop and strand differ in length")
        self._check(self._L.dmx_set_views(self._h, *[a.ctypes.data if n else None for a in arrs],
                                          n), "dmx_set_views")
        self._n_views = n

    def clear_views(self):
        self._check(self._L.dmx_clear_views(self._h), "dmx_clear_views")
        self._n_views = None

    def chop_views(self, qc_ok=None, min_len: int = 0) -> int:
        """The view list made on the device from the last chop_exec: the segment of every read
        with exactly one, qc_ok[r] (None: every read) and at least min_len nt, in read order
        (pychopper's PASS records).  Returns the number of views."""
        qc = None
        if qc_ok is not None:
            qc = np.ascontiguousarray(np.asarray(qc_ok) != 0, dtype=np.uint8)
            if len(qc) != self._n_loaded:
                raise ValueError("chop_views: one qc_ok byte per resident read")
        nv = ctypes.c_uint64()
        self._check(self._L.dmx_chop_views(self._h, qc.ctypes.data if qc is not None and len(qc)
                                           else None, int(min_len), ctypes.byref(nv)),
                    "dmx_chop_views")
        self._n_views = int(nv.value)
        return self._n_views

    def views(self):
        """The current view list as (read u32, start i32, stop i32, strand u8) arrays."""
        n = self._n_views or 0
        out = (np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32),
               np.zeros(n, np.uint8))
        got = self._L.dmx_views_fetch(self._h, *[a.ctypes.data if n else None for a in out], n)
        if got < 0:
            self._check(int(got), "dmx_views_fetch")
        if got != n:
            raise DmxError(f"dmx_views_fetch: {got} views on the device, {n} expected")
        return out

    # ---- operand tables (include/dmx.h dmx_set_operands) -----------------------
    def _n_sort(self) -> int:
        """Entries of the sorting calls' per-read arrays: the operands of a table, else the
        resident reads."""
        ops = getattr(self, "_ops", None)
        return int(ops["n"]) if ops is not None else int(getattr(self, "_n_loaded", 0))

    def _sort_lengths(self):
        """The lengths the sorting calls' indices name (the operands' with a table set)."""
        ops = getattr(self, "_ops", None)
        if ops is None:
            return getattr(self, "_lengths", None)
        if ops.get("lengths") is None:
            _, a, b, _ = self.operands()
            ops["lengths"] = (b - a).astype(np.uint32)
        return ops["lengths"]

    def set_operands(self, read, start, stop, strand):
        """The sorting calls (pairdist, pairhits and what reads its outcomes, groupalign,
        rowdist, rowassign) index operands from now on: operand k = read[k][start[k]:stop[k]] of
        the resident batch, reverse-complemented when strand[k]; their results are those of the
        same call on a batch of the operands' sequences."""
        arrs = [np.ascontiguousarray(read, dtype=np.uint32),
                np.ascontiguousarray(start, dtype=np.int32),
                np.ascontiguousarray(stop, dtype=np.int32),
                np.ascontiguousarray(strand, dtype=np.uint8)]
        n = len(arrs[0])
        if any(len(a) != n for a in arrs):
            raise ValueError("set_operands: read, start, stop and strand differ in length")
        self._check(self._L.dmx_set_operands(self._h, *[a.ctypes.data if n else None
                                                        for a in arrs], n), "dmx_set_operands")
        self._ops = {"n": n, "lengths": (arrs[2] - arrs[1]).astype(np.uint32)}
        self._n_hits = 0
        self._resident = None   # a list tagged resident ran on reads, not on this table

    def clear_operands(self):
        self._check(self._L.dmx_clear_operands(self._h), "dmx_clear_operands")
        self._ops = None
        self._n_hits = 0
        self._resident = None

    def operands(self):
        """The current table as (read u32, start i32, stop i32, strand u8) arrays (empty ones
        without a table)."""
        ops = getattr(self, "_ops", None)
        n = int(ops["n"]) if ops is not None else 0
        out = (np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32),
               np.zeros(n, np.uint8))
        got = self._L.dmx_operands_fetch(self._h, *[a.ctypes.data if n else None for a in out], n)
        if got < 0:
            self._check(int(got), "dmx_operands_fetch")
        if got != n:
            raise DmxError(f"dmx_operands_fetch: {got} operands on the device, {n} expected")
        return out

    def result_operands(self, keep=None, min_len: int = 1):
        """The operand table of the last exec, made on the device: per kept item of round 0 the
        final trimmed, oriented record, grouped by bin (counts()' index) in item order.  keep:
        None (the items matched in every round) or one flag per bin.  Returns bin_first (uint64,
        bins + 1 entries: bin b's operands are bin_first[b] .. bin_first[b + 1])."""
        nb = self.n_counts() - 2
        ka = None
        if keep is not None:
            ka = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        first = np.zeros(nb + 1, dtype=np.uint64)
        n = ctypes.c_uint64(0)
        self._check(self._L.dmx_result_operands(
            self._h, ka.ctypes.data if ka is not None and len(ka) else None,
            len(ka) if ka is not None else 0, int(min_len), first.ctypes.data, len(first),
            ctypes.byref(n)), "dmx_result_operands")
        self._ops = {"n": int(n.value), "lengths": None}
        self._n_hits = 0
        self._resident = None
        return first

    def locate(self, patterns, ascii_blob: np.ndarray, offsets: np.ndarray, lengths: np.ndarray,
               ignore_case: bool = False, only_positive: bool = False) -> np.ndarray:
        """Every exact IUPAC occurrence of every pattern (both strands unless only_positive):
        HIT_DTYPE records sorted as `seqkit locate` prints them — by record, then pattern, '+'
        hits by start, then '-' hits in the order a scan of the reverse complement meets them
        (descending positive-strand end)."""
        pats = [p.encode("ascii") if isinstance(p, str) else bytes(p) for p in patterns]
        arr = (ctypes.c_char_p * max(len(pats), 1))(*pats)
        pl = (ctypes.c_int * max(len(pats), 1))(*[len(p) for p in pats])
        blob = np.ascontiguousarray(ascii_blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        lens = np.ascontiguousarray(lengths, dtype=np.uint32)
        flags = (LOC_IGNORE_CASE if ignore_case else 0) | (LOC_ONLY_POSITIVE if only_positive
                                                           else 0)
        cap = max(1024, len(lens))
        while True:
            hits = np.zeros(cap, dtype=HIT_DTYPE)
            nh = ctypes.c_uint64()
            self._check(self._L.dmx_locate(self._h, arr, pl, len(pats), flags,
                                           blob.ctypes.data if len(blob) else None,
                                           offs.ctypes.data, lens.ctypes.data, len(lens),
                                           hits.ctypes.data, cap, ctypes.byref(nh)),
                        "dmx_locate")
            if nh.value <= cap:
                hits = hits[:nh.value]
                break
            cap = int(nh.value)
        key2 = np.where(hits["strand"] == 0, hits["start"].astype(np.int64),
                        -hits["end"].astype(np.int64))
        order = np.lexsort((key2, hits["strand"], hits["pattern"], hits["seq"]))
        return hits[order]

    # ---- pychopper-style reorientation (include/dmx.h dmx_chop_*) --------------
    def chop_set(self, primers, rules, cutoff: float, keep_primers: bool = True):
        """primers: IUPAC strings (label 2p = primer p, 2p+1 = its reverse complement);
        rules: [(left label, right label, strand 0 '+' / 1 '-')]; cutoff: maximum edit distance
        as a fraction of the primer length; keep_primers: pychopper -p."""
        seqs = [s.encode("ascii") for s in primers]
        arr = (ctypes.c_char_p * max(len(seqs), 1))(*seqs)
        lens = (ctypes.c_int * max(len(seqs), 1))(*[len(s) for s in seqs])
        nr = len(rules)
        rl = (ctypes.c_int * max(nr, 1))(*[int(r[0]) for r in rules])
        rr = (ctypes.c_int * max(nr, 1))(*[int(r[1]) for r in rules])
        rs = (ctypes.c_int * max(nr, 1))(*[int(r[2]) for r in rules])
        self._check(self._L.dmx_chop_set(self._h, arr, lens, len(seqs), rl, rr, rs, nr,
                                         float(cutoff), int(bool(keep_primers))), "dmx_chop_set")

    def chop_exec(self):
        """Hits and segments of the resident batch (after load); returns (n_hits, n_segs)."""
        nh, ns = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._L.dmx_chop_exec(self._h, ctypes.byref(nh), ctypes.byref(ns)),
                    "dmx_chop_exec")
        self._chop_tot = (int(nh.value), int(ns.value))
        return self._chop_tot

    def chop_fetch(self, segs: bool = True, hits: bool = False):
        """(segments per read, hits per read, CHOP_SEG_DTYPE records, CHOP_HIT_DTYPE records),
        records in read order."""
        nh, ns = self._chop_tot
        n = getattr(self, "_n_loaded", 0)
        nseg = np.zeros(n, dtype=np.uint32)
        nhit = np.zeros(n, dtype=np.uint32)
        sg = np.zeros(ns if segs else 0, dtype=CHOP_SEG_DTYPE)
        ht = np.zeros(nh if hits else 0, dtype=CHOP_HIT_DTYPE)
        self._check(self._L.dmx_chop_fetch(self._h, nseg.ctypes.data if n else None,
                                           nhit.ctypes.data if n else None,
                                           sg.ctypes.data if len(sg) else None, len(sg),
                                           ht.ctypes.data if len(ht) else None, len(ht)),
                    "dmx_chop_fetch")
        return nseg, nhit, sg, ht

    def chop_stats(self):
        ms = (ctypes.c_float * 2)()
        nbig = self._check(self._L.dmx_chop_stats(self._h, ms, 2), "dmx_chop_stats")
        return {"chop": float(ms[0]), "order": float(ms[1]), "big_blocks": int(nbig)}

    # ---- pairwise read distance (include/dmx.h dmx_pairdist) ---------------------
    def pairdist(self, q, t, mode: int = PD_NW, flags=None, caps=None) -> np.ndarray:
        """Edit distance of resident read q[i] (query) against t[i] (target): PD_NW whole reads,
        PD_HW query against any substring of the target.  flags: PD_RC per pair (target
        reverse-complemented); caps: out[i] = min(d, caps[i] + 1).  Returns uint32."""
        qa, ta, fa, ca = _pair_arrays(q, t, flags, caps)
        out = np.zeros(len(qa), dtype=np.uint32)
        self._check(self._L.dmx_pairdist(self._h, int(mode), qa.ctypes.data, ta.ctypes.data,
                                         fa.ctypes.data if fa is not None else None,
                                         ca.ctypes.data if ca is not None else None, len(qa),
                                         out.ctypes.data), "dmx_pairdist")
        return out

    def pairdist_ms(self) -> float:
        """Device time (ms) of the last pairdist call."""
        return float(self._L.dmx_pairdist_ms(self._h))

    # ---- global alignment with the edit path (include/dmx.h dmx_pairalign) -------
    def pairalign(self, q, t, flags=None):
        """NW alignment of resident read q[i] (query, rows) against t[i] (target, columns), as
        edlib.align(mode='NW', task='path').  flags: PD_RC per pair.  Returns (dist uint32,
        op_off uint64 of n + 1 entries, ops uint8): pair i's path is ops[op_off[i]:op_off[i + 1]]
        in forward order, PA_MATCH / PA_INSERT / PA_DELETE / PA_MISMATCH (see cigar())."""
        qa, ta, fa, _ = _pair_arrays(q, t, flags, None)
        dist, off, ops = _pairalign_buffers(getattr(self, "_lengths", None), qa, ta)
        self._check(self._L.dmx_pairalign(self._h, qa.ctypes.data, ta.ctypes.data,
                                          fa.ctypes.data if fa is not None else None, len(qa),
                                          dist.ctypes.data, off.ctypes.data, ops.ctypes.data,
                                          len(ops)), "dmx_pairalign")
        return dist, off, ops[:int(off[-1])]

    def pairalign_ms(self) -> float:
        """Device time (ms) of both kernels of the last pairalign call."""
        return float(self._L.dmx_pairalign_ms(self._h))

    def pairalign_stats(self) -> dict:
        """Device time (ms) of the last pairalign call by pass (the forward pass that writes the
        trace, the traceback) and the launches its pair list was cut into (DMX_PA_TRACE_MB)."""
        ms = (ctypes.c_float * 2)()
        n = self._check(self._L.dmx_pairalign_stats(self._h, ms, 2), "dmx_pairalign_stats")
        return {"forward": float(ms[0]), "traceback": float(ms[1]), "launches": int(n)}

    # ---- progressive alignment of read groups (include/dmx.h dmx_groupalign) ----
    def groupalign(self, seeds, groups, max_cols: int = 0, paths: bool = False,
                   strands=None) -> dict:
        """create_alignment's loop for many groups at once: seeds[g] is group g's row 0 (str or
        bytes over A/C/G/T/N/-/IUPAC, or a uint8 array of masks as mask_row makes them),
        groups[g] its members (resident read indices, in alignment order).  Returns a dict:
        col_off (uint64, n + 1), mask (uint8 per column), count and first (uint16, columns x 5:
        members showing A/C/G/T/N in the column, and the 1-based place of the first that did),
        dist (uint32 per member, group after group) and, with paths, op_off / ops as
        pairalign's, one path per member against the row it met.  strands: None, or a list
        parallel to groups of 0 / 1 per member; 1 (PD_RC) takes the member reverse-complemented
        (dmx_groupalign_strands), and dist, ops, count and first are then those of the turned
        read."""
        a = _groupalign_args(self._sort_lengths(), seeds, groups, max_cols, paths,
                             strands=strands)
        if strands is None:
            self._check(self._L.dmx_groupalign(self._h, *a.call), "dmx_groupalign")
        else:
            self._check(self._L.dmx_groupalign_strands(self._h, *a.call),
                        "dmx_groupalign_strands")
        return a.result()

    def groupalign_stats(self) -> dict:
        """Device time (ms) of the last groupalign call by pass, its lock-step rounds and the
        launches (of each of the three kernels) they were cut into."""
        ms = (ctypes.c_float * 3)()
        rounds = ctypes.c_int(0)
        n = self._check(self._L.dmx_groupalign_stats(self._h, ms, 3, ctypes.byref(rounds)),
                        "dmx_groupalign_stats")
        return {"forward": float(ms[0]), "traceback": float(ms[1]), "merge": float(ms[2]),
                "rounds": int(rounds.value), "launches": int(n)}

    # ---- read distance against rows of masks (include/dmx.h dmx_rowdist) --------
    def rowdist(self, rows, q, r, caps=None) -> np.ndarray:
        """NW edit distance of resident read q[i] against rows[r[i]]: a row is a str or bytes
        over A/C/G/T/N/-/IUPAC or a uint8 array of masks as mask_row makes them (a consensus,
        or mask_rc of one for the reverse complement).  caps: out[i] = min(d, caps[i] + 1).
        Returns uint32."""
        masks, off, qa, ra, ca = _rowdist_args(rows, q, r, caps)
        out = np.zeros(len(qa), dtype=np.uint32)
        self._check(self._L.dmx_rowdist(self._h, len(off) - 1, masks.ctypes.data, off.ctypes.data,
                                        qa.ctypes.data, ra.ctypes.data,
                                        ca.ctypes.data if ca is not None else None, len(qa),
                                        out.ctypes.data), "dmx_rowdist")
        return out

    def rowdist_ms(self) -> float:
        """Device time (ms) of the last rowdist call."""
        return float(self._L.dmx_rowdist_ms(self._h))

    # ---- reads assigned to rows of masks (include/dmx.h dmx_rowassign) -----------
    def rowassign(self, rows, reads, cap_hit, cap_half, bin_off, bins, chunk: int = 2_000_000,
                  max_chunks: int = 100):
        """The best row per read, decided on the device: reads[k] (resident read indices; every
        place k is an entry of its own) against every row (as rowdist's) within 5 % of its
        length; cap_hit / cap_half (int32, -1 = none) and bin_off (uint32) are indexed by the
        pair's longer length, bins (uint16) maps bin_off[L] + d to the identity class; the
        generation stops after the place at whose end max_chunks chunks of `chunk` pairs are
        full.  Returns (best_row uint32, LG_NONE = no line; best_d uint32, d or d | LG_REV;
        best_class uint16; n_pairs; n_lines)."""
        a = _rowassign_args(rows, reads, cap_hit, cap_half, bin_off, bins, chunk, max_chunks)
        try:
            self._check(self._L.dmx_rowassign(self._h, *a.call()), "dmx_rowassign")
        except DmxError as e:
            e.outputs = (a.best_row, a.best_d, a.best_class)   # a refusal leaves them untouched
            raise
        return a.result()

    def rowassign_ms(self) -> float:
        """Device time (ms) of the last rowassign call."""
        return float(self._L.dmx_rowassign_ms(self._h))

    # ---- rows of masks against rows of masks (include/dmx.h dmx_rowpairdist) -----
    def rowpairdist(self, rows, q, t, mode: int, flags=None, caps=None) -> np.ndarray:
        """Edit distance of rows[q[i]] (query) against rows[t[i]] (target), PD_NW or PD_HW; rows
        as rowdist's (str / bytes over A/C/G/T/N/-/IUPAC, or uint8 masks), two columns equal iff
        their masks intersect.  flags: PD_RC per pair (the target's reverse complement, mask_rc);
        caps: out[i] = min(d, caps[i] + 1).  Needs no resident batch and leaves one alone.
        Returns uint32."""
        masks, off, qa, ta, fa, ca = _rowpair_args(rows, q, t, flags, caps)
        out = np.zeros(len(qa), dtype=np.uint32)
        self._check(self._L.dmx_rowpairdist(self._h, int(mode), len(off) - 1, masks.ctypes.data,
                                            off.ctypes.data, qa.ctypes.data, ta.ctypes.data,
                                            fa.ctypes.data if fa is not None else None,
                                            ca.ctypes.data if ca is not None else None, len(qa),
                                            out.ctypes.data), "dmx_rowpairdist")
        return out

    def rowhits(self, rows, q, t, cap, mode: int = PD_HW):
        """Per pair the distance on both strands of the target, d = the smaller (ties are
        forward), a hit iff cap[i] >= 0 and d <= cap[i] (cap: int32, -1 = never); decided and
        compacted on the device.  Returns the hits in ascending place in the pair list: (pair
        uint32, d uint32, rev uint8)."""
        masks, off, qa, ta, _, _ = _rowpair_args(rows, q, t, None, None)
        ha = _rowhits_cap(cap, qa)
        n = ctypes.c_size_t(0)
        room = len(qa)
        pair, d = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32)
        rev = np.zeros(room, dtype=np.uint8)
        self._check(self._L.dmx_rowhits(self._h, int(mode), len(off) - 1, masks.ctypes.data,
                                        off.ctypes.data, qa.ctypes.data, ta.ctypes.data,
                                        ha.ctypes.data, len(qa), pair.ctypes.data, d.ctypes.data,
                                        rev.ctypes.data, room, ctypes.byref(n)), "dmx_rowhits")
        return pair[:n.value], d[:n.value], rev[:n.value]

    def rowhits_ms(self) -> float:
        """Device time (ms) of the last rowpairdist or rowhits call."""
        return float(self._L.dmx_rowhits_ms(self._h))

    # ---- gene groups (include/dmx.h dmx_edgegroups .. dmx_hitgroups) -------------
    def edgegroups(self, a, b, n_nodes: int) -> np.ndarray:
        """Connected components of the edges {a[e], b[e]} over n_nodes nodes: per node the
        smallest node of its component, LG_NONE for a node on no edge.  Returns uint32."""
        aa, ba = _edge_arrays(a, b)
        labels = np.zeros(int(n_nodes), dtype=np.uint32)
        self._check(self._L.dmx_edgegroups(self._h, aa.ctypes.data, ba.ctypes.data, len(aa),
                                           int(n_nodes), labels.ctypes.data), "dmx_edgegroups")
        return labels

    def pairhits(self, q, t, cap_hit, cap_half):
        """The similarity pass with the hit decision on the device (dmx_pairhits): per pair of
        resident reads a forward hit (d <= cap_hit), a reverse hit (forward d > cap_half, then
        d against the reverse complement <= cap_hit) or none; caps are int32, -1 = none.  The
        outcomes stay in the context for pairhits_fetch / hitgroups.  Returns (best, n_hits):
        best[r] = the least d over the hits whose target is r (LG_NONE: none), uint32."""
        qa, ta, ha, fa = _pairhits_arrays(q, t, cap_hit, cap_half)
        best = np.zeros(self._n_sort(), dtype=np.uint32)
        n = ctypes.c_uint64(0)
        self._check(self._L.dmx_pairhits(self._h, qa.ctypes.data, ta.ctypes.data, ha.ctypes.data,
                                         fa.ctypes.data, len(qa), best.ctypes.data,
                                         ctypes.byref(n)), "dmx_pairhits")
        self._n_hits = int(n.value)
        return best, int(n.value)

    def pairhits_fetch(self):
        """The hits of the last pairhits in ascending place in its pair list: (pair uint32,
        d uint32, rev uint8)."""
        n = ctypes.c_size_t(0)
        cap = int(getattr(self, "_n_hits", 0))
        pair, d = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        rev = np.zeros(cap, dtype=np.uint8)
        self._check(self._L.dmx_pairhits_fetch(self._h, pair.ctypes.data, d.ctypes.data,
                                               rev.ctypes.data, cap, ctypes.byref(n)),
                    "dmx_pairhits_fetch")
        return pair[:n.value], d[:n.value], rev[:n.value]

    def hitgroups(self, tie) -> np.ndarray:
        """Components of the last pairhits' hits with d <= tie[t] (tie: uint32 per resident
        read): per read the smallest read of its group, LG_NONE for a read on no kept hit."""
        ta = np.ascontiguousarray(tie, dtype=np.uint32)
        if ta.shape != (self._n_sort(),):
            raise DmxError("hitgroups: tie must have one entry per resident read")
        labels = np.zeros(len(ta), dtype=np.uint32)
        self._check(self._L.dmx_hitgroups(self._h, ta.ctypes.data, labels.ctypes.data),
                    "dmx_hitgroups")
        return labels

    def hitgroups_stats(self) -> dict:
        """Device time (ms): the distance launches of the last pairhits, the last compaction, the
        last components run, the last hithist; and the components run's hooking rounds."""
        ms = (ctypes.c_float * 4)()
        n = self._check(self._L.dmx_hitgroups_stats(self._h, ms, 4), "dmx_hitgroups_stats")
        return {"forward": float(ms[0]), "compact": float(ms[1]), "components": float(ms[2]),
                "hist": float(ms[3]), "rounds": int(n)}

    # ---- species groups (include/dmx.h dmx_hithist .. dmx_hitgroups_within) -------
    def hithist(self, bin_off, bins, n_classes: int) -> np.ndarray:
        """The histogram of the last pairhits' hits: hist[bins[bin_off[t] + d]] += 1 per hit with
        distance d and target t (bin_off: uint32 per resident read; bins: uint16 classes below
        n_classes <= 1024).  Returns uint64 counts, one per class."""
        oa, ba = _hist_arrays(bin_off, bins, self._n_sort())
        hist = np.zeros(int(n_classes), dtype=np.uint64)
        self._check(self._L.dmx_hithist(self._h, oa.ctypes.data, ba.ctypes.data, len(ba),
                                        int(n_classes), hist.ctypes.data), "dmx_hithist")
        return hist

    def pairhits_cross(self, label, cap2):
        """The hits of the last pairhits with d <= cap2[t] (int32 per read, -1: none) whose two
        reads carry different labels (uint32 per read, LG_NONE: in no group), in ascending
        place: (pair uint32, d uint32, rev uint8)."""
        la, ca = _label_arrays(label, cap2, self._n_sort())
        n = ctypes.c_size_t(0)
        cap = int(getattr(self, "_n_hits", 0))
        pair, d = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
        rev = np.zeros(cap, dtype=np.uint8)
        self._check(self._L.dmx_pairhits_cross(self._h, la.ctypes.data, ca.ctypes.data,
                                               pair.ctypes.data, d.ctypes.data, rev.ctypes.data,
                                               cap, ctypes.byref(n)), "dmx_pairhits_cross")
        return pair[:n.value].copy(), d[:n.value].copy(), rev[:n.value].copy()

    def hitgroups_within(self, tie2, label, xa=(), xb=(), n_nodes=None) -> np.ndarray:
        """Components over n_nodes nodes (default: the resident reads) of the last pairhits' hits
        with label[q] == label[t] != LG_NONE and d <= tie2[t] (LG_NONE: no edge for t), plus the
        caller's edges {xa, xb}: per node the smallest node of its component, LG_NONE on none."""
        n_reads = self._n_sort()
        ta, _ = _label_arrays(tie2, None, n_reads)
        la, _ = _label_arrays(label, None, n_reads)
        aa, ba = _edge_arrays(xa, xb)
        n_nodes = n_reads if n_nodes is None else int(n_nodes)
        labels = np.zeros(max(n_nodes, 0), dtype=np.uint32)
        self._check(self._L.dmx_hitgroups_within(self._h, ta.ctypes.data, la.ctypes.data,
                                                 aa.ctypes.data, ba.ctypes.data, len(aa), n_nodes,
                                                 labels.ctypes.data), "dmx_hitgroups_within")
        return labels

    def n_counts(self) -> int:
        a1 = 0 if self.mode == MODE_SINGLE else self.panel_sizes[1]
        return (self.panel_sizes[0] + 1) * (a1 + 1) + 2

    def counts(self) -> np.ndarray:
        out = np.zeros(self.n_counts(), dtype=np.uint64)
        self._check(self._L.dmx_counts(self._h, out.ctypes.data, len(out)), "dmx_counts")
        return out

    # ---- RCCL count exchange (include/dmx.h "Multi-GPU count exchange") -----------------------
    def comm_init_rank(self, comm_id: bytes, n_ranks: int, rank: int):
        """Join an n_ranks RCCL communicator (one process per GPU); comm_id from
        comm_unique_id() on rank 0.  Blocks until every rank has joined."""
        buf = ctypes.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        with _stdout_to_stderr():
            rc = self._L.dmx_comm_init_rank(self._h, buf, int(n_ranks), int(rank))
        self._check(rc, "dmx_comm_init_rank")

    def comm_size(self) -> int:
        return self._check(self._L.dmx_comm_size(self._h), "dmx_comm_size")

    def allreduce_counts(self) -> np.ndarray:
        """Per-bin counts of the last exec summed over every rank (RCCL all-reduce in HBM on
        this context's stream; collective)."""
        out = np.zeros(self.n_counts(), dtype=np.uint64)
        self._check(self._L.dmx_allreduce_counts(self._h, out.ctypes.data, len(out)),
                    "dmx_allreduce_counts")
        return out

    def debug_fetch(self, what: int, rnd: int = 0) -> np.ndarray:
        """An intermediate list of the last exec (diagnostics: include/dmx.h dmx_debug_fetch)."""
        nb = self._check(self._L.dmx_debug_fetch(self._h, what, rnd, None, 0), "dmx_debug_fetch")
        buf = np.zeros(nb, dtype=np.uint8)
        self._check(self._L.dmx_debug_fetch(self._h, what, rnd, buf.ctypes.data if nb else None,
                                            nb), "dmx_debug_fetch")
        if what == DBG_FLAGS:
            return buf.view(np.uint32)
        return buf.view(CAND_DTYPE if what in (DBG_CANDS0, DBG_CANDS1) else WINDOW_DTYPE)

    def stats(self):
        ms = (ctypes.c_float * 19)()
        cl = np.zeros(18, dtype=np.uint64)
        fl = ctypes.c_int()
        self._check(self._L.dmx_stats(self._h, ms, 19, cl.ctypes.data, 18, ctypes.byref(fl)),
                    "dmx_stats")
        # filterN: the whole filter stage (with the piece screen, when on: piecesN is its part)
        names = ["scan0", "resolve0", "finalize0", "scan1", "resolve1", "finalize1", "total",
                 "filter0", "verify0", "filter1", "verify1", "screen0", "wscan0", "screen1",
                 "wscan1", "pieces0", "pieces1", "ends0", "ends1"]
        return {"ms": dict(zip(names, list(ms))), "clusters": cl[:2].tolist(),
                "windows": cl[2:4].tolist(), "resolved": cl[4:6].tolist(),
                "traces": cl[6:8].tolist(), "windows_raw": cl[8:10].tolist(),
                "tasks": cl[10:12].tolist(), "filter_tasks": cl[12:14].tolist(),
                # end-window stage: triples that ran the exact DP / that it looked at
                "ends_dp": cl[14:16].tolist(), "ends_seen": cl[16:18].tolist(),
                "flags": fl.value}


def _pair_arrays(q, t, flags, caps):
    qa = np.ascontiguousarray(q, dtype=np.uint32)
    ta = np.ascontiguousarray(t, dtype=np.uint32)
    if qa.ndim != 1 or qa.shape != ta.shape:
        raise DmxError("pairdist: q and t must be one-dimensional and of equal length")
    fa = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
    ca = None if caps is None else np.ascontiguousarray(caps, dtype=np.uint32)
    for a in (fa, ca):
        if a is not None and a.shape != qa.shape:
            raise DmxError("pairdist: flags and caps must have one entry per pair")
    return qa, ta, fa, ca


def pairdist_host(p: "Packed", q, t, mode: int = PD_NW, flags=None, caps=None,
                  n_threads: int = 1) -> np.ndarray:
    """dmx_pairdist's contract on the host, by a plain full-matrix DP (no GPU): the checker of
    the kernel and the CPU baseline of tools/bench_pairdist.py."""
    L = load()
    qa, ta, fa, ca = _pair_arrays(q, t, flags, caps)
    out = np.zeros(len(qa), dtype=np.uint32)
    rc = L.dmx_pairdist_host(int(mode), p.seq2b.ctypes.data, p.nmask.ctypes.data,
                             p.offsets.ctypes.data, p.lengths.ctypes.data, p.n_reads,
                             qa.ctypes.data, ta.ctypes.data,
                             fa.ctypes.data if fa is not None else None,
                             ca.ctypes.data if ca is not None else None, len(qa),
                             out.ctypes.data, int(n_threads))
    if rc < 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"dmx_pairdist_host failed ({rc}): {msg.decode() if msg else ''}")
    return out


def _pairalign_buffers(lengths, qa, ta):
    """dist, op_off and an ops buffer of the sum of both lengths per pair (the library's bound).
    Pairs the library will refuse (an index outside the batch) count as empty here."""
    n = 0 if lengths is None else len(lengths)
    ln = np.zeros(n + 1, dtype=np.int64)
    if n:
        ln[:n] = lengths
    cap = int(ln[np.minimum(qa, n)].sum() + ln[np.minimum(ta, n)].sum())
    return (np.zeros(len(qa), dtype=np.uint32), np.zeros(len(qa) + 1, dtype=np.uint64),
            np.zeros(max(cap, 1), dtype=np.uint8))


def pairalign_host(p: "Packed", q, t, flags=None, n_threads: int = 1, ops_cap=None):
    """dmx_pairalign's contract on the host: a plain full-matrix DP and the tie rule applied
    literally (no GPU).  The checker of the kernels and the CPU baseline of
    tools/bench_pairalign.py.  ops_cap: the room given to the library instead of the sum of
    both lengths per pair (to see it refused).  Returns (dist, op_off, ops) as
    Context.pairalign."""
    L = load()
    qa, ta, fa, _ = _pair_arrays(q, t, flags, None)
    dist, off, ops = _pairalign_buffers(p.lengths, qa, ta)
    rc = L.dmx_pairalign_host(p.seq2b.ctypes.data, p.nmask.ctypes.data, p.offsets.ctypes.data,
                              p.lengths.ctypes.data, p.n_reads, qa.ctypes.data, ta.ctypes.data,
                              fa.ctypes.data if fa is not None else None, len(qa),
                              dist.ctypes.data, off.ctypes.data, ops.ctypes.data,
                              len(ops) if ops_cap is None else int(ops_cap), int(n_threads))
    if rc < 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"dmx_pairalign_host failed ({rc}): {msg.decode() if msg else ''}")
    return dist, off, ops[:int(off[-1])]


# dmx_groupalign's row alphabet: bit c of a mask = the column equals query symbol c (A, C, G, T,
# masked/N); '-' equals nothing; the IUPAC pairs are create_alignment's additionalEqualities
_MASK_OF = {"-": 0, "A": 1, "C": 2, "G": 4, "T": 8, "N": 16, "R": 1 | 4, "Y": 2 | 8, "M": 1 | 2,
            "K": 4 | 8, "S": 4 | 2, "W": 1 | 8}
_MASK_LUT = np.full(256, 255, dtype=np.uint8)
for _ch, _m in _MASK_OF.items():
    _MASK_LUT[ord(_ch)] = _MASK_LUT[ord(_ch.lower())] = _m
_SYM_LUT = np.zeros(32, dtype=np.uint8)
for _ch in "-ACGTN":
    _SYM_LUT[_MASK_OF[_ch]] = ord(_ch)


def mask_row(seq) -> np.ndarray:
    """A row of dmx_groupalign as mask bytes, from str or bytes over A/C/G/T/N, '-' and
    R/Y/M/K/S/W (either case); anything else is refused."""
    b = seq.encode("ascii", "replace") if isinstance(seq, str) else bytes(seq)
    m = _MASK_LUT[np.frombuffer(b, dtype=np.uint8)]
    bad = np.flatnonzero(m == 255)
    if len(bad):
        raise DmxError(f"mask_row: {chr(b[bad[0]])!r} at {int(bad[0])} is not one of "
                       "A/C/G/T/N, '-' or R/Y/M/K/S/W")
    return m


def mask_symbols(mask) -> str:
    """The row a mask array stands for, where that is one symbol per column: '-' and the
    single-bit masks A/C/G/T/N (a mask of several bits is refused)."""
    m = np.asarray(mask, dtype=np.uint8)
    if m.ndim != 1 or (len(m) and int(m.max()) > 31):
        raise DmxError("mask_symbols: a one-dimensional array of masks 0..31")
    s = _SYM_LUT[m]
    if (s == 0).any():
        raise DmxError("mask_symbols: a mask of several symbols has no single letter")
    return s.tobytes().decode()


class _groupalign_args:
    """The packed arguments and caller-sized outputs of dmx_groupalign(_host)."""

    def __init__(self, lengths, seeds, groups, max_cols, paths, ops_cap=None, cols_cap=None,
                 strands=None):
        if len(seeds) != len(groups):
            raise DmxError("groupalign: one seed row per group")
        rows = [np.ascontiguousarray(s, dtype=np.uint8) if isinstance(s, np.ndarray)
                else mask_row(s) for s in seeds]
        mem = [np.ascontiguousarray(g, dtype=np.uint32).reshape(-1) for g in groups]
        n = len(rows)
        self.seed_off = np.zeros(n + 1, dtype=np.uint64)
        self.member_off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            self.seed_off[1:] = np.cumsum([len(r) for r in rows])
            self.member_off[1:] = np.cumsum([len(g) for g in mem])
        self.seeds = np.concatenate(rows + [np.zeros(0, dtype=np.uint8)])
        self.members = np.concatenate(mem + [np.zeros(0, dtype=np.uint32)])
        self.flags = None   # strands: one flag byte per member (dmx_groupalign_strands)
        if strands is not None:
            fl = [np.ascontiguousarray(f, dtype=np.uint8).reshape(-1) for f in strands]
            if len(fl) != n or any(len(f) != len(g) for f, g in zip(fl, mem)):
                raise DmxError("groupalign: strands must be parallel to groups, one per member")
            self.flags = np.concatenate(fl + [np.zeros(0, dtype=np.uint8)])
        # the library's bounds (include/dmx.h): a row grows by a member's length at most
        nr = 0 if lengths is None else len(lengths)
        ln = np.zeros(nr + 1, dtype=np.int64)
        if nr:
            ln[:nr] = lengths
        lim = int(max_cols) if max_cols else PD_MAX_LEN
        cols = ops = 0
        for r, g in zip(rows, mem):
            grow = np.minimum(len(r) + np.cumsum(ln[np.minimum(g, nr)]), lim)
            cols += int(grow[-1]) if len(g) else min(len(r), lim)
            ops += int(grow.sum())
        cols = cols if cols_cap is None else int(cols_cap)
        ops = ops if ops_cap is None else int(ops_cap)
        self.col_off = np.zeros(n + 1, dtype=np.uint64)
        self.mask = np.zeros(max(cols, 1), dtype=np.uint8)
        self.count = np.zeros((max(cols, 1), 5), dtype=np.uint16)
        self.first = np.zeros((max(cols, 1), 5), dtype=np.uint16)
        self.dist = np.zeros(len(self.members), dtype=np.uint32)
        self.op_off = np.zeros(len(self.members) + 1, dtype=np.uint64) if paths else None
        self.ops = np.zeros(max(ops, 1), dtype=np.uint8) if paths else None
        self.call = (n, self.seeds.ctypes.data, self.seed_off.ctypes.data,
                     self.members.ctypes.data) + \
                    (() if self.flags is None else (self.flags.ctypes.data,)) + \
                    (self.member_off.ctypes.data, int(max_cols),
                     self.col_off.ctypes.data, self.mask.ctypes.data, self.count.ctypes.data,
                     self.first.ctypes.data, cols, self.dist.ctypes.data,
                     self.op_off.ctypes.data if paths else None,
                     self.ops.ctypes.data if paths else None, ops)

    def result(self) -> dict:
        n = int(self.col_off[-1])
        out = {"col_off": self.col_off, "mask": self.mask[:n], "count": self.count[:n],
               "first": self.first[:n], "dist": self.dist, "member_off": self.member_off}
        if self.ops is not None:
            out["op_off"] = self.op_off
            out["ops"] = self.ops[:int(self.op_off[-1])]
        return out


def groupalign_host(p: "Packed", seeds, groups, max_cols: int = 0, paths: bool = False,
                    n_threads: int = 1, ops_cap=None, cols_cap=None, strands=None) -> dict:
    """dmx_groupalign's contract on the host, group after group and member after member (no
    GPU): the checker of the kernels and the CPU comparator of tools/bench_groupalign.py.
    ops_cap, cols_cap: the room given to the library instead of its bounds (to see it refused).
    strands: as Context.groupalign's (dmx_groupalign_strands_host).  Returns the dict of
    Context.groupalign."""
    L = load()
    a = _groupalign_args(p.lengths, seeds, groups, max_cols, paths, ops_cap, cols_cap, strands)
    name = "dmx_groupalign_host" if strands is None else "dmx_groupalign_strands_host"
    rc = getattr(L, name)(p.seq2b.ctypes.data, p.nmask.ctypes.data, p.offsets.ctypes.data,
                          p.lengths.ctypes.data, p.n_reads, *a.call, int(n_threads))
    if rc < 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"{name} failed ({rc}): {msg.decode() if msg else ''}")
    return a.result()


# A <-> T and C <-> G of a mask's low four bits (bit order A, C, G, T: the nibble reversed); N
# (bit 4) stays
_MASK_COMP = np.array([(m & 16) | ((m & 1) << 3) | ((m & 2) << 1) | ((m & 4) >> 1) | ((m & 8) >> 3)
                       for m in range(32)], dtype=np.uint8)


def mask_rc(mask) -> np.ndarray:
    """The reverse complement of a row of masks: the columns backwards with bits A <-> T and
    C <-> G swapped, N and gap columns unchanged (mask_rc(mask_row(s)) is mask_row of the
    reverse complement of s, IUPAC pairs included)."""
    m = np.asarray(mask, dtype=np.uint8)
    if m.ndim != 1 or (len(m) and int(m.max()) > 31):
        raise DmxError("mask_rc: a one-dimensional array of masks 0..31")
    return np.ascontiguousarray(_MASK_COMP[m[::-1]])


def _rowdist_args(rows, q, r, caps):
    """(masks, row_off, q, r, caps) of dmx_rowdist(_host), the rows closed up."""
    rr = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1) if isinstance(s, np.ndarray)
          else mask_row(s) for s in rows]
    off = np.zeros(len(rr) + 1, dtype=np.uint64)
    if rr:
        off[1:] = np.cumsum([len(x) for x in rr])
    masks = np.concatenate(rr + [np.zeros(1, dtype=np.uint8)])   # never empty: a valid pointer
    qa = np.ascontiguousarray(q, dtype=np.uint32)
    ra = np.ascontiguousarray(r, dtype=np.uint32)
    if qa.ndim != 1 or qa.shape != ra.shape:
        raise DmxError("rowdist: q and r must be one-dimensional and of equal length")
    ca = None if caps is None else np.ascontiguousarray(caps, dtype=np.uint32)
    if ca is not None and ca.shape != qa.shape:
        raise DmxError("rowdist: caps must have one entry per pair")
    return masks, off, qa, ra, ca


def rowdist_host(p: "Packed", rows, q, r, caps=None, n_threads: int = 1) -> np.ndarray:
    """dmx_rowdist's contract on the host, by a plain full-matrix DP with the mask equality (no
    GPU): the checker of the kernel and the CPU comparator of tools/bench_rowdist.py."""
    L = load()
    masks, off, qa, ra, ca = _rowdist_args(rows, q, r, caps)
    out = np.zeros(len(qa), dtype=np.uint32)
    rc = L.dmx_rowdist_host(p.seq2b.ctypes.data, p.nmask.ctypes.data, p.offsets.ctypes.data,
                            p.lengths.ctypes.data, p.n_reads, len(off) - 1, masks.ctypes.data,
                            off.ctypes.data, qa.ctypes.data, ra.ctypes.data,
                            ca.ctypes.data if ca is not None else None, len(qa), out.ctypes.data,
                            int(n_threads))
    if rc < 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"dmx_rowdist_host failed ({rc}): {msg.decode() if msg else ''}")
    return out


class _rowassign_args:
    """The arrays of dmx_rowassign(_host), checked, and the outputs.  The outputs start as the
    value a refused call must leave in them, so that the tests can see them untouched."""

    def __init__(self, rows, reads, cap_hit, cap_half, bin_off, bins, chunk, max_chunks):
        self.masks, self.off, self.reads, _, _ = _rowdist_args(rows, reads, reads, None)
        self.cap_hit = np.ascontiguousarray(cap_hit, dtype=np.int32)
        self.cap_half = np.ascontiguousarray(cap_half, dtype=np.int32)
        self.bin_off = np.ascontiguousarray(bin_off, dtype=np.uint32)
        self.bins = np.ascontiguousarray(bins, dtype=np.uint16)
        if (self.cap_hit.ndim != 1 or self.cap_half.shape != self.cap_hit.shape
                or self.bin_off.shape != self.cap_hit.shape or self.bins.ndim != 1):
            raise DmxError("rowassign: cap_hit, cap_half and bin_off must be one-dimensional and "
                           "of equal length, bins one-dimensional")
        if int(chunk) < 0 or int(max_chunks) < 0:
            raise DmxError("rowassign: chunk and max_chunks must not be negative")
        self.chunk, self.max_chunks = int(chunk), int(max_chunks)
        n = len(self.reads)
        self.best_row = np.full(n, 0xDEADBEEF, dtype=np.uint32)
        self.best_d = np.full(n, 0xDEADBEEF, dtype=np.uint32)
        self.best_class = np.full(n, 0xBEEF, dtype=np.uint16)
        self.n_pairs, self.n_lines = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(self):
        self._keep = []   # a valid pointer even for an empty array: only the lengths decide
        return [len(self.off) - 1, self.masks.ctypes.data, self.off.ctypes.data,
                _keep_ptr(self, self.reads),
                len(self.reads), _keep_ptr(self, self.cap_hit), _keep_ptr(self, self.cap_half),
                _keep_ptr(self, self.bin_off), len(self.cap_hit), _keep_ptr(self, self.bins),
                len(self.bins), self.chunk, self.max_chunks,
                _keep_ptr(self, self.best_row), _keep_ptr(self, self.best_d),
                _keep_ptr(self, self.best_class), ctypes.byref(self.n_pairs),
                ctypes.byref(self.n_lines)]

    def result(self):
        return (self.best_row, self.best_d, self.best_class, int(self.n_pairs.value),
                int(self.n_lines.value))


def _keep_ptr(owner, a):
    """a's address, or that of a one-element stand-in kept alive by owner when a is empty."""
    if len(a):
        return a.ctypes.data
    owner._keep.append(np.zeros(1, dtype=a.dtype))
    return owner._keep[-1].ctypes.data


def rowassign_host(p: "Packed", rows, reads, cap_hit, cap_half, bin_off, bins,
                   chunk: int = 2_000_000, max_chunks: int = 100, n_threads: int = 1):
    """dmx_rowassign's contract on the host (no GPU), on dmx_rowdist_host's DP with the decision
    and the reduction in sequential C++: the checker of the kernels and ctx=None of
    sorter.assign_best.  Returns what Context.rowassign returns."""
    L = load()
    a = _rowassign_args(rows, reads, cap_hit, cap_half, bin_off, bins, chunk, max_chunks)
    try:
        _host_check(L, L.dmx_rowassign_host(p.seq2b.ctypes.data, p.nmask.ctypes.data,
                                            p.offsets.ctypes.data, p.lengths.ctypes.data,
                                            p.n_reads, *a.call(), int(n_threads)),
                    "dmx_rowassign_host")
    except DmxError as e:
        e.outputs = (a.best_row, a.best_d, a.best_class)
        raise
    return a.result()


def _rowpair_args(rows, q, t, flags, caps):
    """(masks, row_off, q, t, flags, caps) of dmx_rowpairdist(_host) / dmx_rowhits(_host)."""
    masks, off, qa, ta, ca = _rowdist_args(rows, q, t, caps)
    fa = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
    if fa is not None and fa.shape != qa.shape:
        raise DmxError("rowpairdist: flags must have one entry per pair")
    return masks, off, qa, ta, fa, ca


def _rowhits_cap(cap, qa):
    ha = np.ascontiguousarray(cap, dtype=np.int32)
    if ha.shape != qa.shape:
        raise DmxError("rowhits: cap must have one entry per pair")
    return ha


def rowpairdist_host(rows, q, t, mode: int, flags=None, caps=None,
                     n_threads: int = 1) -> np.ndarray:
    """dmx_rowpairdist's contract on the host, by a plain full-matrix DP with the intersect
    equality (no GPU): the checker of the kernel."""
    L = load()
    masks, off, qa, ta, fa, ca = _rowpair_args(rows, q, t, flags, caps)
    out = np.zeros(len(qa), dtype=np.uint32)
    rc = L.dmx_rowpairdist_host(int(mode), len(off) - 1, masks.ctypes.data, off.ctypes.data,
                                qa.ctypes.data, ta.ctypes.data,
                                fa.ctypes.data if fa is not None else None,
                                ca.ctypes.data if ca is not None else None, len(qa),
                                out.ctypes.data, int(n_threads))
    if rc < 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"dmx_rowpairdist_host failed ({rc}): {msg.decode() if msg else ''}")
    return out


def rowhits_host(rows, q, t, cap, mode: int = PD_HW, n_threads: int = 1):
    """dmx_rowhits' contract on the host (no GPU), on rowpairdist_host: (pair, d, rev) as
    Context.rowhits."""
    L = load()
    masks, off, qa, ta, _, _ = _rowpair_args(rows, q, t, None, None)
    ha = _rowhits_cap(cap, qa)
    n = ctypes.c_size_t(0)
    room = len(qa)
    pair, d = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32)
    rev = np.zeros(room, dtype=np.uint8)
    rc = L.dmx_rowhits_host(int(mode), len(off) - 1, masks.ctypes.data, off.ctypes.data,
                            qa.ctypes.data, ta.ctypes.data, ha.ctypes.data, len(qa),
                            pair.ctypes.data, d.ctypes.data, rev.ctypes.data, room,
                            ctypes.byref(n), int(n_threads))
    if rc < 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"dmx_rowhits_host failed ({rc}): {msg.decode() if msg else ''}")
    return pair[:n.value], d[:n.value], rev[:n.value]


def _edge_arrays(a, b):
    aa = np.ascontiguousarray(a, dtype=np.uint32)
    ba = np.ascontiguousarray(b, dtype=np.uint32)
    if aa.ndim != 1 or aa.shape != ba.shape:
        raise DmxError("edgegroups: a and b must be one-dimensional and of equal length")
    return aa, ba


def _pairhits_arrays(q, t, cap_hit, cap_half):
    qa, ta, _, _ = _pair_arrays(q, t, None, None)
    ha = np.ascontiguousarray(cap_hit, dtype=np.int32)
    fa = np.ascontiguousarray(cap_half, dtype=np.int32)
    if ha.shape != qa.shape or fa.shape != qa.shape:
        raise DmxError("pairhits: cap_hit and cap_half must have one entry per pair")
    return qa, ta, ha, fa


def _host_check(L, rc: int, what: str):
    if rc < 0:
        msg = L.dmx_last_error(None)
        raise DmxError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def edgegroups_host(a, b, n_nodes: int) -> np.ndarray:
    """dmx_edgegroups' contract on the host, by a sequential union-find (no GPU)."""
    L = load()
    aa, ba = _edge_arrays(a, b)
    labels = np.zeros(int(n_nodes), dtype=np.uint32)
    _host_check(L, L.dmx_edgegroups_host(aa.ctypes.data, ba.ctypes.data, len(aa), int(n_nodes),
                                         labels.ctypes.data), "dmx_edgegroups_host")
    return labels


class HostHits:
    """The state of pairhits_host: the pair list and per pair the outcome word (d, d | LG_REV or
    LG_NONE); best per read; what Context keeps on the device."""

    def __init__(self, q, t, outcome, best, n_reads):
        self.q, self.t, self.outcome, self.best, self.n_reads = q, t, outcome, best, n_reads

    def fetch(self):
        """(pair, d, rev) as Context.pairhits_fetch returns them."""
        pair = np.flatnonzero(self.outcome != LG_NONE).astype(np.uint32)
        o = self.outcome[pair]
        return pair, o & np.uint32(LG_REV - 1), (o >> np.uint32(31)).astype(np.uint8)


def pairhits_host(p: "Packed", q, t, cap_hit, cap_half, n_threads: int = 1) -> HostHits:
    """dmx_pairhits' contract on the host (dmx_pairdist_host's DP; no GPU).  Returns the state
    hitgroups_host reads."""
    L = load()
    qa, ta, ha, fa = _pairhits_arrays(q, t, cap_hit, cap_half)
    outcome = np.zeros(len(qa), dtype=np.uint32)
    best = np.zeros(p.n_reads, dtype=np.uint32)
    n = ctypes.c_uint64(0)
    _host_check(L, L.dmx_pairhits_host(p.seq2b.ctypes.data, p.nmask.ctypes.data,
                                       p.offsets.ctypes.data, p.lengths.ctypes.data, p.n_reads,
                                       qa.ctypes.data, ta.ctypes.data, ha.ctypes.data,
                                       fa.ctypes.data, len(qa), outcome.ctypes.data,
                                       best.ctypes.data, ctypes.byref(n), int(n_threads)),
                "dmx_pairhits_host")
    assert int(n.value) == int((outcome != LG_NONE).sum())
    return HostHits(qa, ta, outcome, best, p.n_reads)


def hitgroups_host(hits, tie) -> np.ndarray:
    """dmx_hitgroups' contract on the host, on the state of pairhits_host (a HostHits)."""
    L = load()
    if not isinstance(hits, HostHits):
        raise DmxError("hitgroups_host failed (-1): no pairhits_host state")
    ta = np.ascontiguousarray(tie, dtype=np.uint32)
    if ta.shape != (hits.n_reads,):
        raise DmxError("hitgroups: tie must have one entry per read")
    labels = np.zeros(hits.n_reads, dtype=np.uint32)
    _host_check(L, L.dmx_hitgroups_host(hits.q.ctypes.data, hits.t.ctypes.data,
                                        hits.outcome.ctypes.data, len(hits.q), ta.ctypes.data,
                                        hits.n_reads, labels.ctypes.data), "dmx_hitgroups_host")
    return labels


def _hist_arrays(bin_off, bins, n_reads):
    oa = np.ascontiguousarray(bin_off, dtype=np.uint32)
    ba = np.ascontiguousarray(bins, dtype=np.uint16)
    if oa.shape != (n_reads,) or ba.ndim != 1:
        raise DmxError("hithist: bin_off must have one entry per read, bins one dimension")
    return oa, ba


def _label_arrays(label, cap2, n_reads):
    la = np.ascontiguousarray(label, dtype=np.uint32)
    ca = None if cap2 is None else np.ascontiguousarray(cap2, dtype=np.int32)
    if la.shape != (n_reads,) or (ca is not None and ca.shape != (n_reads,)):
        raise DmxError("species groups: the per-read tables must have one entry per read")
    return la, ca


def hithist_host(hits, bin_off, bins, n_classes: int) -> np.ndarray:
    """dmx_hithist's contract on the host, on the state of pairhits_host."""
    L = load()
    oa, ba = _hist_arrays(bin_off, bins, hits.n_reads)
    hist = np.zeros(int(n_classes), dtype=np.uint64)
    _host_check(L, L.dmx_hithist_host(hits.t.ctypes.data, hits.outcome.ctypes.data, len(hits.t),
                                      hits.n_reads, oa.ctypes.data, ba.ctypes.data, len(ba),
                                      int(n_classes), hist.ctypes.data), "dmx_hithist_host")
    return hist


def pairhits_cross_host(hits, label, cap2):
    """dmx_pairhits_cross' contract on the host, on the state of pairhits_host."""
    L = load()
    la, ca = _label_arrays(label, cap2, hits.n_reads)
    cap = int((hits.outcome != LG_NONE).sum())
    pair, d = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    rev = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    _host_check(L, L.dmx_pairhits_cross_host(hits.q.ctypes.data, hits.t.ctypes.data,
                                             hits.outcome.ctypes.data, len(hits.q), hits.n_reads,
                                             la.ctypes.data, ca.ctypes.data, pair.ctypes.data,
                                             d.ctypes.data, rev.ctypes.data, cap,
                                             ctypes.byref(n)), "dmx_pairhits_cross_host")
    return pair[:n.value].copy(), d[:n.value].copy(), rev[:n.value].copy()


def hitgroups_within_host(hits, tie2, label, xa=(), xb=(), n_nodes=None) -> np.ndarray:
    """dmx_hitgroups_within's contract on the host, on the state of pairhits_host."""
    L = load()
    ta, _ = _label_arrays(tie2, None, hits.n_reads)
    la, _ = _label_arrays(label, None, hits.n_reads)
    aa, ba = _edge_arrays(xa, xb)
    n_nodes = hits.n_reads if n_nodes is None else int(n_nodes)
    labels = np.zeros(max(n_nodes, 0), dtype=np.uint32)
    _host_check(L, L.dmx_hitgroups_within_host(hits.q.ctypes.data, hits.t.ctypes.data,
                                               hits.outcome.ctypes.data, len(hits.q),
                                               hits.n_reads, ta.ctypes.data, la.ctypes.data,
                                               aa.ctypes.data, ba.ctypes.data, len(aa), n_nodes,
                                               labels.ctypes.data), "dmx_hitgroups_within_host")
    return labels


def operands_check_host(lengths, read, start, stop, strand) -> None:
    """dmx_set_operands' argument checks against a batch's read lengths, without a device:
    raises DmxError (.code: the library's code) where set_operands would refuse the table."""
    L = load()
    la = np.ascontiguousarray(lengths, dtype=np.uint32)
    arrs = [np.ascontiguousarray(read, dtype=np.uint32), np.ascontiguousarray(start, dtype=np.int32),
            np.ascontiguousarray(stop, dtype=np.int32), np.ascontiguousarray(strand, dtype=np.uint8)]
    n = len(arrs[0])
    if any(len(a) != n for a in arrs):
        raise ValueError("operands_check_host: read, start, stop and strand differ in length")
    rc = L.dmx_operands_check_host(la.ctypes.data if len(la) else None, len(la),
                                   *[a.ctypes.data if n else None for a in arrs], n)
    if rc:
        e = DmxError(f"dmx_set_operands failed ({rc}): "
                     f"{(L.dmx_last_error(None) or b'').decode()}")
        e.code = rc
        raise e


def result_operands_host(res, lengths, mode: int, wheres0, wheres1=None, views=None, keep=None,
                         min_len: int = 1):
    """Context.result_operands in plain sequential C++ on fetch()'s results: lengths are the
    batch's read lengths, wheres0 / wheres1 the panels' adapter types (DMX_FRONT / DMX_BACK per
    adapter), views round 0's item list (read, start, stop, strand) or None for whole reads.
    Returns ((read, start, stop, strand), bin_first)."""
    L = load()
    ra = np.ascontiguousarray(res, dtype=RESULT_DTYPE)
    la = np.ascontiguousarray(lengths, dtype=np.uint32)
    w0 = np.ascontiguousarray(wheres0, dtype=np.int32)
    w1 = np.ascontiguousarray(wheres1 if wheres1 is not None else [], dtype=np.int32)
    va = [None] * 4
    if views is not None:
        va = [np.ascontiguousarray(views[0], dtype=np.uint32),
              np.ascontiguousarray(views[1], dtype=np.int32),
              np.ascontiguousarray(views[2], dtype=np.int32),
              np.ascontiguousarray(views[3], dtype=np.uint8)]
        if any(len(a) != len(ra) for a in va):
            raise ValueError("result_operands_host: one view per result")
        if not len(ra):   # an empty view run: a non-null list all the same
            va = [np.zeros(1, a.dtype) for a in va]
    nb = (len(w0) + 1) * ((len(w1) if mode == MODE_TWO_ROUND else 0) + 1)
    ka = None if keep is None else np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
    n = len(ra)
    out = (np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.int32),
           np.zeros(n, np.uint8))
    first = np.zeros(nb + 1, dtype=np.uint64)
    cnt = ctypes.c_uint64(0)
    rc = L.dmx_result_operands_host(
        ra.ctypes.data if n else None, n, *[a.ctypes.data if a is not None else None for a in va],
        la.ctypes.data if len(la) else None, len(la), int(mode), w0.ctypes.data, len(w0),
        w1.ctypes.data if len(w1) else None, len(w1),
        ka.ctypes.data if ka is not None and len(ka) else None, len(ka) if ka is not None else 0,
        int(min_len), *[a.ctypes.data if n else None for a in out], n, first.ctypes.data,
        len(first), ctypes.byref(cnt))
    if rc:
        e = DmxError(f"dmx_result_operands_host failed ({rc}): "
                     f"{(L.dmx_last_error(None) or b'').decode()}")
        e.code = rc
        raise e
    k = int(cnt.value)
    return tuple(a[:k] for a in out), first


def cigar(ops, extended: bool = False) -> str:
    """edlib's CIGAR of one path (a slice of pairalign's ops), run-length encoded: standard
    (M for a match or a mismatch, I, D) or extended (=, X, I, D)."""
    a = np.asarray(ops, dtype=np.uint8)
    if a.ndim != 1:
        raise DmxError("cigar: one path (a one-dimensional array of ops)")
    if len(a) == 0:
        return ""
    if int(a.max()) > PA_MISMATCH:
        raise DmxError("cigar: an op outside 0..3")
    sym = np.frombuffer(b"=IDX" if extended else b"MIDM", dtype=np.uint8)[a]
    cut = np.flatnonzero(sym[1:] != sym[:-1]) + 1
    start = np.concatenate([[0], cut])
    runs = np.diff(np.concatenate([start, [len(sym)]]))
    return "".join(f"{int(n)}{chr(sym[s0])}" for s0, n in zip(start, runs))


def pairdist_group_sizes() -> list:
    """The lane-group sizes dmx_pairdist's kernel cuts a wave into (dmx_pairdist_group_sizes)."""
    L = load()
    n = L.dmx_pairdist_group_sizes(None, 0)
    out = (ctypes.c_int * n)()
    L.dmx_pairdist_group_sizes(out, n)
    return [int(x) for x in out]


def panel_reach(seqs, flags: int, max_errors: float = 0.1, min_overlap: int = 3,
                wheres=None):
    """Host only: (status, reach) of the panel dmx_set_panel would build — how far the kernels'
    gathers reach around a read view, in nt (include/dmx.h dmx_panel_reach)."""
    L = load()
    arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
    lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
    wh = (ctypes.c_int * len(seqs))(*wheres) if wheres is not None else None
    out = np.zeros(6, dtype=np.int32)
    rc = L.dmx_panel_reach(arr, lens, wh, len(seqs), float(max_errors), int(min_overlap),
                           int(flags), out.ctypes.data, 6)
    return rc, dict(zip(["pre_raw", "pre", "post", "need_pre", "need_post", "guard"],
                        out.tolist()))


def panel_near_shared(seqs, flags: int, max_errors: float = 0.1, min_overlap: int = 3,
                      wheres=None):
    """Host only: (status, info) of the near-start columns that only the first adapter of the
    panel dmx_set_panel would build scans (include/dmx.h dmx_panel_near_shared)."""
    L = load()
    arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
    lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
    wh = (ctypes.c_int * len(seqs))(*wheres) if wheres is not None else None
    out = np.zeros(4, dtype=np.int32)
    rc = L.dmx_panel_near_shared(arr, lens, wh, len(seqs), float(max_errors), int(min_overlap),
                                 int(flags), out.ctypes.data, 4)
    return rc, dict(zip(["near_shared", "filter_len", "jsplit", "kk"], out.tolist()))


PIECE_FIELDS = ["step", "pieces", "keys", "entries", "front_reach", "part_max", "lo_off",
                "dlo_min"]


def panel_pieces(seqs, flags: int, max_errors: float = 0.1, min_overlap: int = 3):
    """Host only: (status, info, entries) of the piece screen dmx_set_panel would build
    (include/dmx.h dmx_panel_pieces).  entries: dicts of the packed (piece, offset) entries."""
    L = load()
    arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
    lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
    out = np.zeros(8, dtype=np.int32)
    ent = np.zeros(4096, dtype=np.uint64)
    rc = L.dmx_panel_pieces(arr, lens, len(seqs), float(max_errors), int(min_overlap), int(flags),
                            out.ctypes.data, 8, ent.ctypes.data, len(ent))
    info = dict(zip(PIECE_FIELDS, out.tolist()))
    ents = []
    for v in ent[:info["entries"]].tolist():
        ents.append({"val": v & 0xFFFFFFFF, "len": (v >> 32) & 31, "o": (v >> 37) & 1,
                     "off": (v >> 38) & 3, "dlo": ((v >> 40) & 255) - 128,
                     "dhi": ((v >> 48) & 255) - 128})
    return rc, info, ents


def panel_piece_pairs(seqs, flags: int, max_errors: float = 0.1, min_overlap: int = 3):
    """Host only: (status, pair, rank_base, keys) of that piece screen (include/dmx.h
    dmx_panel_piece_pairs): the 4096-word pair table of the sampled 8-mers, the rank base per four
    rows, and per key (increasing 8-mer) first entry | count << 16 into panel_pieces' entries."""
    L = load()
    arr = (ctypes.c_char_p * len(seqs))(*[s.encode("ascii") for s in seqs])
    lens = (ctypes.c_int * len(seqs))(*[len(s) for s in seqs])
    pair = np.zeros(4096, dtype=np.uint32)
    rank = np.zeros(1024, dtype=np.uint16)
    keys = np.zeros(2048, dtype=np.uint32)
    rc = L.dmx_panel_piece_pairs(arr, lens, len(seqs), float(max_errors), int(min_overlap),
                                 int(flags), pair.ctypes.data, rank.ctypes.data, keys.ctypes.data,
                                 len(keys))
    return rc, pair, rank, keys


def host_register(arrays) -> list:
    """Page-lock the given numpy arrays (upload sources); returns the registered ones."""
    L = load()
    done = []
    for a in arrays:
        if a.nbytes and L.dmx_host_register(a.ctypes.data, a.nbytes) == 0:
            done.append(a)
    return done


def host_unregister(arrays):
    L = load()
    for a in arrays:
        L.dmx_host_unregister(a.ctypes.data)


def device_count() -> int:
    """Visible HIP devices (0 without a GPU)."""
    return int(load().dmx_device_count())


@contextlib.contextmanager
def _stdout_to_stderr():
    """RCCL prints its version banner on stdout at initialisation; keep stdout for the callers'
    own output (bench.py's one JSON line, CLI reports)."""
    sys.stdout.flush()
    libc = ctypes.CDLL(None)
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        libc.fflush(None)
        os.dup2(saved, 1)
        os.close(saved)


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (rank 0 draws it; every rank passes it to comm_init_rank)."""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    with _stdout_to_stderr():
        rc = load().dmx_comm_unique_id(buf)
    if rc != 0:
        why = load().dmx_last_error(None)   # the context-free message (e.g. RCCL not loadable)
        raise DmxError(f"dmx_comm_unique_id failed ({rc}): "
                       f"{why.decode(errors='replace') if why else 'no message'}")
    return buf.raw


def comm_init_all(ctxs) -> bool:
    """One RCCL communicator over contexts on distinct devices (ncclCommInitAll); run_multi then
    sums its per-bin counts on the devices.  Returns False (no communicator) when contexts share
    a device, where RCCL cannot place two ranks."""
    if len({c.device for c in ctxs}) != len(ctxs):
        return False
    L = load()
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    with _stdout_to_stderr():
        rc = L.dmx_comm_init_all(arr, len(ctxs))
    if rc < 0:
        msg = L.dmx_last_error(ctxs[0]._h)
        raise DmxError(f"dmx_comm_init_all failed ({rc}): {msg.decode() if msg else ''}")
    return True


def open_group(devices) -> list:
    """One context per device; contexts on distinct devices share one RCCL communicator
    (dmx_comm_init_all), so run_batch sums their per-bin counts on the GPUs over xGMI."""
    ctxs = [Context(d) for d in devices]
    if len(ctxs) > 1:
        try:
            comm_init_all(ctxs)
        except DmxError as e:   # dmx_run_multi then sums the shards' counts on the host
            print(f"dmx: RCCL communicator unavailable ({e}); per-bin counts are summed on the "
                  "host", file=sys.stderr)
    return ctxs


def run_batch(ctxs, p: Packed):
    """One packed batch on one or several contexts: (per-read results, per-bin counts).  With
    several contexts the batch is sharded by dmx_run_multi (counts all-reduced by RCCL when the
    contexts are one open_group communicator)."""
    if len(ctxs) == 1:
        res = ctxs[0].run(p)
        return res, ctxs[0].counts()
    return run_multi(ctxs, p)


def bin_totals(counts: np.ndarray, a0: int, a1: int) -> np.ndarray:
    """dmx_counts layout -> matrix [bin1 + 1, bin2 + 1] ((A0+1) x (A1+1); A1 = 0 in SINGLE mode;
    row/column 0 = no match)."""
    return np.asarray(counts[:(a0 + 1) * (a1 + 1)], dtype=np.int64).reshape(a0 + 1, a1 + 1)


def run_multi(ctxs, p: Packed):
    """Shard one packed batch over several contexts (one per GPU); returns (results, counts)."""
    L = load()
    if not ctxs:
        raise DmxError("run_multi needs at least one context")
    out = np.zeros(p.n_reads, dtype=RESULT_DTYPE)
    counts = np.zeros(ctxs[0].n_counts(), dtype=np.uint64)
    arr = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    rc = L.dmx_run_multi(arr, len(ctxs), p.seq2b.ctypes.data, p.nmask.ctypes.data,
                         p.offsets.ctypes.data, p.lengths.ctypes.data, p.n_words, p.n_reads,
                         out.ctypes.data, counts.ctypes.data, len(counts))
    if rc < 0:
        msg = L.dmx_last_error(ctxs[0]._h)
        raise DmxError(f"dmx_run_multi failed ({rc}): {msg.decode() if msg else ''}")
    for c in ctxs:   # every context's batch changed, and its operand table went with it
        c._ops = None
        c._resident = None
        c._load_gen = getattr(c, "_load_gen", 0) + 1
    return out, counts
