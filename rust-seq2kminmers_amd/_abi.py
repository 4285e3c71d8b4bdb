"""The mirror of include/s2k.h: constants, struct layouts, the prototype of every function, and the loader of csrc/libs2k.so."""
import ctypes as C
import enum
import os

import numpy as np

# One HIP runtime per process: torch bundles its own libamdhip64.so.7 and the system ROCm has another; whichever is mapped first
# serves both (same SONAME).  torch is imported before load_library maps the library, so that device memory and streams handed
# over by torch belong to the runtime this library talks to.  Without torch the package still imports; only the tensor calls need it.
try:
    import torch
except ImportError:
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libs2k.so")

ABI_VERSION = 2  # include/s2k.h S2K_ABI_VERSION this mirror was written against


class HashMode(enum.IntEnum):  # src/lib.rs:21-27
    Regular = 0
    Hpc = 1
    Simd = 2
    HpcSimd = 3


FLAG_WANT_MINIMIZERS = 1
FLAG_FORCE_SERIAL = 2
FLAG_LEGACY_PATH = 8  # round-2 records (16 B with the read index, per-read scans) instead of the descriptor path
FLAG_NO_PACK2 = 4  # s2k_extract: bases as ASCII over PCIe instead of 2-bit packed + exception list
HPC_RLE_ALPHABET = 1  # s2k_hpc_device_ex: the run rule of encode_rle (src/hpc.rs:14)
COUNT_SORTED = 1  # s2k_count_device_ex: pairs in ascending order of key
STEP_LINKED = 1  # s2k_thread_out.flags: the step's first item follows a solid item of the same read
WALK_CIRCULAR = 1  # s2k_walk_out.flags: the walk lies on a circular unitig
NO_EDGE = 0xFFFFFFFF  # s2k_walk_out.edge: the step follows no edge
NO_PARTNER = 0xFFFFFFFF  # s2k_graph_resolve_mask: d_partner of an edge that enters no resolved unitig
NO_COPY = 0xFFFFFFFF  # s2k_paths_lift: d_step_copy of a dropped step
ALIGN_OVER = 1  # s2k_align_out.flags: the distance exceeds max_edits
ALIGN_BAD_PATH = 2  # WalkAlignments.flags: s2k_walks_targets called the walk's path bad; it was not aligned
ALIGN_MAX_EDITS = 255  # s2k_align_pairs: the largest max_edits
ALIGN_WAVES = 2048  # s2k_align_pairs: the waves of its persistent grid
BUBBLE_MAX_NODES = 62  # s2k_graph_bubble_mask: the largest max_nodes
BUBBLE_WAVES = 8192  # s2k_graph_bubble_mask: the waves of its bounded grid
CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = 1, 2, 7, 8  # s2k_align_out.ops: len << 4 | op, the BAM codes
CIGAR_CHARS = {CIGAR_I: "I", CIGAR_D: "D", CIGAR_EQ: "=", CIGAR_X: "X"}
PILEUP_MAX_SHIFT = 64  # s2k_walks_pileup: the largest max_shift
PILEUP_PLANES = ("match", "del", "sub0", "sub1", "sub2", "sub3", "ins0", "ins1", "ins2", "ins3", "ins_long")  # s2k_pile, in its order
PILEUP_STATS = ("walks_used", "walks_skipped", "n_other", "n_end_ins", "n_shifted", "n_empty_ins")  # s2k_walks_pileup: stats[0 .. 6)
CONSENSUS_STATS = ("n_low", "n_sub", "n_del", "n_ins", "n_long")  # s2k_pileup_consensus: stats[0 .. 5)
PILEUP_STATS_WORDS = CONSENSUS_STATS_WORDS = 8
CONSENSUS_LONG_STATS = CONSENSUS_STATS + ("n_ins_long", "n_ins_long_bases")  # s2k_pileup_consensus_ex: stats[0 .. 7)
LONG_INS_MIN, LONG_INS_MAX = 2, 12  # s2k_walks_pileup_ex: the I runs that get a vote key
LONG_INS_POS_BITS = 36  # the bits of the position a vote key holds
NO_STEP = 0xFFFFFFFFFFFFFFFF  # s2k_walks_segments: d_src_step of a source step that went into no step of the walks' paths
SEGMENT_LEN = 512  # s2k_walks_segments: the default seg_len, in query bases
SEGMENT_MIN_LEN = 64  # s2k_walks_segments: the smallest seg_len
SEGMENT_STATS = ("candidates", "outside", "admissible", "chosen", "walks_cut")  # s2k_walks_segments: stats[0 .. 5)
SEGMENT_STATS_WORDS = 8


class S2kError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("s2k status %d: %s" % (status, msg))
        self.status = status


class Params(C.Structure):
    _fields_ = [("l", C.c_uint32), ("k", C.c_uint32), ("density", C.c_double), ("mode", C.c_int32), ("flags", C.c_uint32)]


class Counts(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_minimizers", C.c_uint64), ("n_kminmers", C.c_uint64),
                ("xor_hash", C.c_uint64), ("hash_bound", C.c_uint32), ("path", C.c_uint32)]

    def as_dict(self):
        return {f: int(getattr(self, f)) for f, _ in self._fields_}


_u8p, _u32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


class Result(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_kminmers", C.c_uint64), ("km_off", _u64p), ("hash", _u64p), ("start", _u32p),
                ("end", _u32p), ("rev", _u8p), ("n_minimizers", C.c_uint64), ("mn_off", _u64p), ("mn_j", _u32p),
                ("mn_jend", _u32p), ("mn_hash", _u32p), ("counts", Counts), ("_owner", C.c_void_p)]


class DeviceOut(C.Structure):
    _fields_ = [("km_capacity", C.c_uint64), ("km_off", C.c_void_p), ("hash", C.c_void_p), ("start", C.c_void_p),
                ("end", C.c_void_p), ("rev", C.c_void_p), ("mn_capacity", C.c_uint64), ("mn_off", C.c_void_p),
                ("mn_j", C.c_void_p), ("mn_jend", C.c_void_p), ("mn_hash", C.c_void_p)]


class SolidOut(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("km_off", C.c_void_p), ("hash", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p),
                ("rev", C.c_void_p), ("offset", C.c_void_p), ("count", C.c_void_p)]


class UnitigOut(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("uni_off", C.c_void_p), ("members", C.c_void_p), ("node_unitig", C.c_void_p),
                ("node_pos", C.c_void_p), ("circular", C.c_void_p)]


class NodeSeqs(C.Structure):
    _fields_ = [("seq_off", C.c_void_p), ("seq_len", C.c_void_p), ("shift_fwd", C.c_void_p), ("shift_rev", C.c_void_p), ("rev", C.c_void_p),
                ("pool", C.c_void_p), ("pool_capacity", C.c_uint64)]


class ThreadOut(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("path_off", C.c_void_p), ("unitig", C.c_void_p), ("pos", C.c_void_p), ("count", C.c_void_p),
                ("item", C.c_void_p), ("flags", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p)]


class WalkOut(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("walk_off", C.c_void_p), ("first_step", C.c_void_p), ("n_steps", C.c_void_p), ("items", C.c_void_p),
                ("qstart", C.c_void_p), ("qend", C.c_void_p), ("path_len", C.c_void_p), ("path_start", C.c_void_p), ("path_end", C.c_void_p),
                ("flags", C.c_void_p), ("edge", C.c_void_p)]


class AlignOut(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("edits", C.c_void_p), ("flags", C.c_void_p), ("ops_off", C.c_void_p), ("n_ops", C.c_void_p),
                ("matches", C.c_void_p), ("ops", C.c_void_p)]


class SegmentOut(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("seg_off", C.c_void_p), ("q_begin", C.c_void_p), ("q_end", C.c_void_p), ("t_begin", C.c_void_p),
                ("t_end", C.c_void_p)]


class Pile(C.Structure):
    _fields_ = [("match", C.c_void_p), ("del_", C.c_void_p), ("sub", C.c_void_p * 4), ("ins", C.c_void_p * 4), ("ins_long", C.c_void_p)]


STEP_FIELDS = ("unitig", "pos", "count", "item", "flags", "start", "end")  # the per-step arrays of s2k_thread_out: ReadPaths.STEP_FIELDS
WALK_FIELDS = ("first_step", "n_steps", "items", "qstart", "qend", "path_len", "path_start", "path_end", "flags")  # those of s2k_walk_out: ReadWalks.FIELDS

# s2k_node_place: where the forward oriented node 2 i lies on the oriented unitigs
NodePlace = np.dtype([("unitig", np.uint32), ("pos", np.uint32), ("len", np.uint32), ("circular", np.uint32)])


_vp, _u64, _u32, _int, _str, _P = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p, C.POINTER
_n64 = _P(_u64)  # a count or size the call writes

# name -> (restype, argtypes) of every function of include/s2k.h, in its order; tests/test_abi.py compares each with the header.
# A device or host array is a c_void_p whatever its element type; a struct the library reads or fills is a POINTER to its mirror.
PROTOTYPES = {
    "s2k_abi_version": (_int, []),
    "s2k_device_count": (_int, []),
    "s2k_create": (_vp, [_int, _P(_int)]),
    "s2k_destroy": (None, [_vp]),
    "s2k_set_stream": (_int, [_vp, _vp]),
    "s2k_chain_after": (_int, [_vp, _vp]),
    "s2k_set_host_batch": (_int, [_vp, _u64]),
    "s2k_strerror": (_str, [_int]),
    "s2k_last_error": (_str, [_vp]),
    "s2k_hash_bound": (_u32, [C.c_double]),
    "s2k_density_for_bound": (C.c_double, [_u32]),
    "s2k_extract": (_int, [_vp, _vp, _vp, _u64, _P(Params), _P(Result)]),
    "s2k_result_free": (None, [_P(Result)]),
    "s2k_trim": (_int, [_vp]),
    "s2k_extract_device": (_int, [_vp, _vp, _vp, _u64, _u64, _P(Params), _P(DeviceOut), _P(Counts)]),
    "s2k_sync": (_int, [_vp, _P(Counts)]),
    "s2k_hpc_device": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _n64]),
    "s2k_hpc_device_ex": (_int, [_vp, _vp, _vp, _u64, _u64, _u32, _vp, _vp, _vp, _u64, _n64]),
    "s2k_count_device": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _n64]),
    "s2k_count_device_ex": (_int, [_vp, _vp, _u64, _u32, _u32, _vp, _vp, _u64, _n64, _n64]),
    "s2k_count_merge_device": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _u64, _n64, _n64]),
    "s2k_counter_create": (_vp, [_vp, _P(_int)]),
    "s2k_counter_destroy": (None, [_vp]),
    "s2k_counter_add": (_int, [_vp, _vp, _u64]),
    "s2k_counter_finish": (_int, [_vp, _u32, _vp, _vp, _u64, _n64, _n64]),
    "s2k_table_create": (_vp, [_vp, _vp, _vp, _u64, _P(_int)]),
    "s2k_table_destroy": (None, [_vp]),
    "s2k_table_lookup": (_int, [_vp, _vp, _u64, _vp]),
    "s2k_table_filter": (_int, [_vp, _u64, _P(DeviceOut), _u32, _P(SolidOut), _n64]),
    "s2k_table_edges": (_int, [_vp, _u64, _P(DeviceOut), _u32, _vp, _u64, _n64]),
    "s2k_graph_adjacency": (_int, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "s2k_graph_unitigs": (_int, [_vp, _vp, _vp, _u64, _u64, _P(UnitigOut), _n64, _n64]),
    "s2k_graph_unitig_edges": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _n64]),
    "s2k_graph_unitigs_last_steps": (None, [_P(C.c_double), _P(_u32)]),
    "s2k_graph_simplify_mask": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u32, _u32, _vp, _n64, _n64, _n64]),
    "s2k_graph_bubble_mask": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u32, _u32, _vp, _n64, _n64, _n64, _n64]),
    "s2k_graph_induced": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _n64, _n64]),
    "s2k_table_representatives": (_int, [_vp, _u64, _P(DeviceOut), _u64, _vp]),
    "s2k_table_node_sequences": (_int, [_vp, _u64, _P(DeviceOut), _u32, _vp, _vp, _u64, _vp, _P(NodeSeqs), _u64, _n64]),
    "s2k_unitig_sequences": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _P(NodeSeqs), _vp, _vp, _vp, _u64, _n64]),
    "s2k_unitig_node_places": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "s2k_table_thread": (_int, [_vp, _u64, _P(DeviceOut), _u32, _vp, _u64, _P(ThreadOut), _vp, _u64, _n64]),
    "s2k_paths_spans": (_int, [_vp, _u64, _P(ThreadOut), _u64, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _n64, _n64, _n64]),
    "s2k_graph_resolve_mask": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _n64, _n64]),
    "s2k_graph_untangle": (_int, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _n64, _n64]),
    "s2k_unitig_expand": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _n64]),
    "s2k_unitig_member_offsets": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _P(NodeSeqs), _vp, _vp, _vp, _n64]),
    "s2k_paths_walks": (_int, [_vp, _u64, _P(ThreadOut), _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _P(WalkOut), _n64, _n64, _n64]),
    "s2k_paths_bridge": (_int, [_vp, _u64, _P(ThreadOut), _u64, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _u32, _P(ThreadOut), _vp, _vp, _n64, _n64, _n64]),
    "s2k_unitig_copy_places": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _u64, _vp]),
    "s2k_paths_lift": (_int, [_vp, _u64, _P(ThreadOut), _u64, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _P(ThreadOut),
                              _vp, _vp, _vp, _vp, _n64, _n64, _n64, _n64]),
    "s2k_table_vote_keys": (_int, [_vp, _u64, _P(DeviceOut), _u32, _vp, _vp, _vp, _u64, _n64]),
    "s2k_table_vote_representatives": (_int, [_vp, _vp, _u64, _P(DeviceOut), _u32, _vp, _vp, _u64, _vp]),
    "s2k_vote_ordinals": (_int, [_vp, _vp, _u64, _vp]),
    "s2k_walks_targets": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _n64]),
    "s2k_align_pairs": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u32, _P(AlignOut), _n64]),
    "s2k_walks_pileup": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64,
                                _u32, _P(Pile), _n64]),
    "s2k_walks_pileup_ex": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64,
                                   _u32, _P(Pile), _n64, _vp, _u64, _n64, _n64]),
    "s2k_pileup_consensus": (_int, [_vp, _P(Pile), _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _vp, _vp, _n64, _n64]),
    "s2k_pileup_consensus_ex": (_int, [_vp, _P(Pile), _vp, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _vp, _vp, _n64, _n64, _vp, _vp, _u64]),
    "s2k_walks_segments": (_int, [_vp, _u64, _P(WalkOut), _u64, _P(ThreadOut), _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _P(ThreadOut),
                                  _u64, _vp, _vp, _P(DeviceOut), _u32, _P(SegmentOut), _n64, _n64]),
    "s2k_align_join": (_int, [_vp, _u64, _vp, _vp, _u64, _P(AlignOut), _P(AlignOut), _n64]),
    "s2k_walks_gaf": (_int, [_vp, _u64, _P(WalkOut), _u64, _vp, _u64, _vp, _vp, _u64, _u64, _vp, _P(AlignOut), _vp, _u64, _vp, _n64]),
    "s2k_partition_device": (_int, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "s2k_synth_bases_device": (_int, [_vp, _u64, _u64, _u64, _vp]),
    "s2k_synth_hifi_lengths": (None, [_u64, _u64, _u64, _vp]),
    "s2k_synth_hifi_device": (_int, [_vp, _u64, _u64, _u64, _vp, _vp]),
    "s2k_last_kernel_ms": (_int, [_vp, _int, _P(C.c_float)]),
    "s2k_enable_timing": (_int, [_vp, _int]),
    "s2k_timing_total": (_int, [_vp, _int, _P(C.c_double), _P(_u32)]),
    "s2k_fastx_open": (_vp, [_str, _P(_int)]),
    "s2k_fastx_next": (_int, [_vp, _u64, _u64, _P(_vp), _P(_vp), _n64]),
    "s2k_fastx_close": (None, [_vp]),
    "s2k_fastx_parse_device": (_int, [_vp, _vp, _u64, _int, _vp, _u64, _vp, _u64, _n64, _n64]),
    "s2k_run_file": (_int, [_vp, _str, _P(Params), _u64, _P(Counts), _P(C.c_double)]),
    "s2k_run_file_count": (_int, [_vp, _str, _P(Params), _u64, _vp, _P(Counts), _P(C.c_double)]),
}
ABI_SYMBOLS = list(PROTOTYPES)


class _Handle:
    """close() and __del__ of an object that owns one handle of the library (self.lib): _HANDLE names the attribute that holds it,
    _DESTROY the function that frees it.  close() frees once and sets the attribute to None; __del__ swallows errors at interpreter exit."""

    _HANDLE, _DESTROY = "handle", None

    def close(self):
        if getattr(self, self._HANDLE, None):
            getattr(self.lib, self._DESTROY)(getattr(self, self._HANDLE))
            setattr(self, self._HANDLE, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_lib = None


def load_library(path=None):
    """dlopen the C-ABI library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("S2K_LIB") or LIB_PATH  # S2K_LIB: tests load the host-ASan build of the same library
    if not os.path.exists(p):
        raise ImportError("%s is missing: build it with `make -C %s` (or __graft_entry__.build())" % (p, os.path.dirname(p)))
    L = C.CDLL(p)
    if L.s2k_abi_version() != ABI_VERSION:
        raise ImportError("%s has ABI version %d, this binding needs %d: rebuild it (make -C %s)" % (p, L.s2k_abi_version(), ABI_VERSION, os.path.dirname(p)))
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = L
    return L


def hash_bound(density):
    """(density * u32::MAX as f64) as u32 -- src/lib.rs:91"""
    return int(load_library().s2k_hash_bound(float(density)))
