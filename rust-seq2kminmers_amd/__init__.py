"""rust-seq2kminmers_amd -- host-side mirror of the reference's seq -> k-min-mer interface over the
MI355X C ABI (include/s2k.h, built from csrc/ into csrc/libs2k.so).

Reference interface mirrored here (names, argument meaning, error behaviour):
    KminmersIterator::new(seq, l, k, density, mode)   src/lib.rs:89-131
    impl Iterator { type Item = KminmerHash }         src/lib.rs:179-270
    KminmerHash{hash,start,end,offset,rev}, ==/ord by hash only   src/kminmer.rs:128-135,181-204
    HashMode{Regular,Hpc,Simd,HpcSimd}                src/lib.rs:21-27
    hpc(), encode_rle_simd()                          src/hpc.rs:28-41, 44-147

There is no CPU fallback: importing works anywhere (so the CPU test tier can check the ABI), but
creating an Engine without a GPU raises.  The directory name carries a hyphen (as the task names it),
so load it with `import_package()` from s2k_loader.py or importlib.
"""
import ctypes as C
import enum
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libs2k.so")

ABI_VERSION = 2  # include/s2k.h S2K_ABI_VERSION this mirror was written against

ABI_SYMBOLS = [
    "s2k_trim", "s2k_density_for_bound", "s2k_abi_version", "s2k_device_count", "s2k_create", "s2k_destroy", "s2k_set_stream", "s2k_chain_after", "s2k_set_host_batch", "s2k_strerror",
    "s2k_last_error", "s2k_hash_bound", "s2k_extract", "s2k_result_free", "s2k_extract_device", "s2k_sync",
    "s2k_hpc_device", "s2k_hpc_device_ex", "s2k_count_device", "s2k_count_device_ex", "s2k_partition_device", "s2k_synth_bases_device", "s2k_synth_hifi_lengths", "s2k_synth_hifi_device", "s2k_last_kernel_ms", "s2k_enable_timing", "s2k_timing_total", "s2k_fastx_open", "s2k_fastx_next", "s2k_fastx_close", "s2k_run_file", "s2k_fastx_parse_device",
    "s2k_count_merge_device", "s2k_counter_create", "s2k_counter_destroy", "s2k_counter_add", "s2k_counter_finish", "s2k_run_file_count",
    "s2k_table_create", "s2k_table_destroy", "s2k_table_lookup", "s2k_table_filter", "s2k_table_edges", "s2k_graph_adjacency",
    "s2k_graph_unitigs", "s2k_graph_unitig_edges", "s2k_graph_unitigs_last_steps",
    "s2k_table_representatives", "s2k_table_node_sequences", "s2k_unitig_sequences",
    "s2k_graph_simplify_mask", "s2k_graph_induced",
    "s2k_unitig_node_places", "s2k_table_thread",
    "s2k_paths_spans", "s2k_graph_resolve_mask",
    "s2k_graph_untangle", "s2k_unitig_expand",
    "s2k_unitig_member_offsets", "s2k_paths_walks",
    "s2k_paths_bridge",
    "s2k_unitig_copy_places", "s2k_paths_lift",
    "s2k_table_vote_keys", "s2k_table_vote_representatives", "s2k_vote_ordinals",
    "s2k_walks_targets", "s2k_align_pairs",
    "s2k_walks_pileup", "s2k_pileup_consensus",
    "s2k_walks_segments", "s2k_align_join",
]


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
CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X = 1, 2, 7, 8  # s2k_align_out.ops: len << 4 | op, the BAM codes
CIGAR_CHARS = {CIGAR_I: "I", CIGAR_D: "D", CIGAR_EQ: "=", CIGAR_X: "X"}
PILEUP_MAX_SHIFT = 64  # s2k_walks_pileup: the largest max_shift
PILEUP_PLANES = ("match", "del", "sub0", "sub1", "sub2", "sub3", "ins0", "ins1", "ins2", "ins3", "ins_long")  # s2k_pile, in its order
PILEUP_STATS = ("walks_used", "walks_skipped", "n_other", "n_end_ins", "n_shifted", "n_empty_ins")  # s2k_walks_pileup: stats[0 .. 6)
CONSENSUS_STATS = ("n_low", "n_sub", "n_del", "n_ins", "n_long")  # s2k_pileup_consensus: stats[0 .. 5)
PILEUP_STATS_WORDS = CONSENSUS_STATS_WORDS = 8
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


# s2k_node_place: where the forward oriented node 2 i lies on the oriented unitigs
NodePlace = np.dtype([("unitig", np.uint32), ("pos", np.uint32), ("len", np.uint32), ("circular", np.uint32)])


_lib = None


def load_library(path=None):
    """dlopen the C-ABI library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("S2K_LIB") or LIB_PATH  # S2K_LIB: tests load the host-ASan build of the same library
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 and the system ROCm has
    # another; whichever is mapped first serves both (same SONAME).  Import torch first so that device
    # memory and streams handed over by torch belong to the runtime this library talks to.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(p):
        raise ImportError("%s is missing: build it with `make -C %s` (or __graft_entry__.build())" % (p, os.path.dirname(p)))
    L = C.CDLL(p)
    L.s2k_abi_version.restype = C.c_int
    if L.s2k_abi_version() != ABI_VERSION:
        raise ImportError("%s has ABI version %d, this binding needs %d: rebuild it (make -C %s)" % (p, L.s2k_abi_version(), ABI_VERSION, os.path.dirname(p)))
    L.s2k_trim.argtypes = [C.c_void_p]
    L.s2k_device_count.restype = C.c_int
    L.s2k_create.restype = C.c_void_p
    L.s2k_create.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.s2k_destroy.argtypes = [C.c_void_p]
    L.s2k_destroy.restype = None
    L.s2k_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.s2k_chain_after.argtypes = [C.c_void_p, C.c_void_p]
    L.s2k_set_host_batch.argtypes = [C.c_void_p, C.c_uint64]
    L.s2k_set_host_batch.restype = C.c_int
    L.s2k_strerror.restype = C.c_char_p
    L.s2k_strerror.argtypes = [C.c_int]
    L.s2k_last_error.restype = C.c_char_p
    L.s2k_last_error.argtypes = [C.c_void_p]
    L.s2k_hash_bound.restype = C.c_uint32
    L.s2k_hash_bound.argtypes = [C.c_double]
    L.s2k_density_for_bound.restype = C.c_double
    L.s2k_density_for_bound.argtypes = [C.c_uint32]
    L.s2k_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Params), C.POINTER(Result)]
    L.s2k_result_free.argtypes = [C.POINTER(Result)]
    L.s2k_result_free.restype = None
    L.s2k_extract_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(Params),
                                     C.POINTER(DeviceOut), C.POINTER(Counts)]
    L.s2k_sync.argtypes = [C.c_void_p, C.POINTER(Counts)]
    L.s2k_hpc_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_hpc_device_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_count_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_count_device_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_count_merge_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_counter_create.restype = C.c_void_p
    L.s2k_counter_create.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.s2k_counter_destroy.restype = None
    L.s2k_counter_destroy.argtypes = [C.c_void_p]
    L.s2k_counter_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.s2k_counter_finish.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_run_file_count.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Params), C.c_uint64, C.c_void_p, C.POINTER(Counts), C.POINTER(C.c_double)]
    L.s2k_table_create.restype = C.c_void_p
    L.s2k_table_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    L.s2k_table_destroy.restype = None
    L.s2k_table_destroy.argtypes = [C.c_void_p]
    L.s2k_table_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.s2k_table_filter.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DeviceOut), C.c_uint32, C.POINTER(SolidOut), C.POINTER(C.c_uint64)]
    L.s2k_table_edges.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DeviceOut), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_graph_adjacency.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.s2k_graph_unitigs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(UnitigOut), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64)]
    L.s2k_graph_unitig_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_graph_unitigs_last_steps.restype = None
    L.s2k_graph_unitigs_last_steps.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.s2k_graph_simplify_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                          C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_graph_induced.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_table_representatives.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DeviceOut), C.c_uint64, C.c_void_p]
    L.s2k_table_node_sequences.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DeviceOut), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                           C.POINTER(NodeSeqs), C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_unitig_sequences.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(NodeSeqs), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_unitig_node_places.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    L.s2k_table_thread.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DeviceOut), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(ThreadOut), C.c_void_p,
                                   C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_paths_spans.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ThreadOut), C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                  C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_graph_resolve_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_graph_untangle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)]
    L.s2k_unitig_expand.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_unitig_member_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(NodeSeqs), C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.s2k_paths_walks.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ThreadOut), C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                  C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(WalkOut),
                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_paths_bridge.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ThreadOut), C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(ThreadOut), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_unitig_copy_places.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_void_p]
    L.s2k_paths_lift.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(ThreadOut), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                 C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ThreadOut),
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                 C.POINTER(C.c_uint64)]
    L.s2k_table_vote_keys.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(DeviceOut), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64)]
    L.s2k_table_vote_representatives.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(DeviceOut), C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_uint64, C.c_void_p]
    L.s2k_vote_ordinals.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.s2k_walks_targets.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.s2k_align_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_uint32, C.POINTER(AlignOut), C.POINTER(C.c_uint64)]
    L.s2k_walks_pileup.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                   C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(Pile), C.POINTER(C.c_uint64)]
    L.s2k_pileup_consensus.argtypes = [C.c_void_p, C.POINTER(Pile), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_walks_segments.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(WalkOut), C.c_uint64, C.POINTER(ThreadOut), C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(ThreadOut), C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(DeviceOut), C.c_uint32, C.POINTER(SegmentOut),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.s2k_align_join.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(AlignOut), C.POINTER(AlignOut), C.POINTER(C.c_uint64)]
    L.s2k_partition_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    L.s2k_synth_bases_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.s2k_synth_hifi_lengths.restype = None
    L.s2k_synth_hifi_lengths.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    L.s2k_synth_hifi_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.s2k_last_kernel_ms.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    L.s2k_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.s2k_timing_total.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.s2k_fastx_open.restype = C.c_void_p
    L.s2k_fastx_open.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    L.s2k_fastx_next.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.s2k_fastx_close.argtypes = [C.c_void_p]
    L.s2k_fastx_close.restype = None
    L.s2k_run_file.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(Params), C.c_uint64, C.POINTER(Counts), C.POINTER(C.c_double)]
    L.s2k_fastx_parse_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if path is None:
        _lib = L
    return L


def hash_bound(density):
    """(density * u32::MAX as f64) as u32 -- src/lib.rs:91"""
    return int(load_library().s2k_hash_bound(float(density)))


def _as_u8(seq):
    if isinstance(seq, str):
        seq = seq.encode("latin-1")
    if isinstance(seq, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


def pack_reads(reads):
    """list of byte strings -> (bases u8[total], read_off u64[n+1])"""
    arrs = [_as_u8(r) for r in reads]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs], dtype=np.uint64)
    bases = np.concatenate(arrs) if arrs and int(off[-1]) else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(bases, dtype=np.uint8), off


def _p(x, k=1):
    """the device pointer of tensor x as a C argument, NULL when k is 0 (an empty array) or x is None"""
    return C.c_void_p(x.data_ptr() if k and x is not None else 0)


def _paths_struct(paths, fields, capacity):
    """-> (ThreadOut, tensors): the struct that names path_off and those of `fields` a ReadPaths carries, and the contiguous
    tensors behind it by field, which the caller keeps alive over its calls"""
    o = ThreadOut()
    o.capacity = capacity
    keep = {f: getattr(paths, f).contiguous() for f in ("path_off",) + tuple(fields) if getattr(paths, f) is not None}
    for f, x in keep.items():
        setattr(o, f, x.data_ptr() if x.numel() else 0)
    return o, keep


def _paths_out(o, res, keep, m, per_step, n_steps):
    """before the second call of paths_bridge / paths_lift: room for m output steps of the step fields the input carries (named in o) and
    of matched, and for the per_step arrays ({name: dtype}, one entry per input step), all into res"""
    import torch

    dev = res["path_off"].device
    for f in [f for f in ReadPaths.STEP_FIELDS if f in keep] + ["matched"]:
        res[f] = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        if f != "matched":
            setattr(o, f, res[f].data_ptr())
    for f, dt in per_step.items():
        res[f] = torch.empty(max(n_steps, 1), dtype=dt, device=dev)
    o.capacity = m


def _paths_result(res, per_step, m, n_steps, **totals):
    """what paths_bridge / paths_lift return: path_off whole, the per_step arrays cut to n_steps, the rest to m, and the totals"""
    return {**{f: (x if f == "path_off" else x[:n_steps] if f in per_step else x[:m]) for f, x in res.items()}, "n_steps": m, **totals}


def _walk_args(name, walks, step_unitig, out_off, out, overlap):
    """what walks_targets and walks_pileup (name) share -> (n_walks, device, the C arguments n_walks .. n_unitigs, the tensors to keep alive)"""
    rec = [getattr(walks, f).contiguous() for f in ("first_step", "n_steps", "path_start", "path_end", "flags")]
    step_unitig, out_off, out, overlap = keep = [x.contiguous() for x in (step_unitig, out_off, out, overlap)]
    nw, ns, t = rec[0].numel(), step_unitig.numel(), out_off.numel() - 1
    if (any(x.numel() != nw for x in rec) or [x.element_size() for x in rec] != [8, 4, 8, 8, 4] or step_unitig.element_size() != 4
            or out_off.element_size() != 8 or out.element_size() != 1 or overlap.numel() != 2 * t or overlap.element_size() != 4):
        raise ValueError(name + " wants the walk records, one 32-bit unitig per step, and the out_off, out and overlap of the unitig sequences")
    return nw, out_off.device, (nw, *(_p(x, nw) for x in rec), _p(step_unitig, ns), ns, _p(out_off), _p(out, out.numel()), out.numel(), _p(overlap, t), t), rec + keep


def _align_out(n, dev, m=None, res=None, fields=None):
    """the results of align_pairs / align_join over n records -> (AlignOut, res, cut): res holds edits, flags, n_ops, matches (int32 per record),
    ops_off (int64, n + 1) and, once the number of runs m is known, ops; the struct names `fields` (None: all) with capacity m; cut(): res as returned"""
    import torch

    if res is None:
        res = {f: torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for f in ("edits", "flags", "n_ops", "matches")}
        res["ops_off"] = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    o = AlignOut(m or 0)
    if m is not None:
        res["ops"] = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
    for f in fields or res:
        setattr(o, f, res[f].data_ptr())
    return o, res, lambda: {f: (x if f == "ops_off" else x[:m] if f == "ops" else x[:n]) for f, x in res.items()}


class Engine:
    """One s2k_ctx (one per thread and device, like one KminmersIterator per thread in src/main.rs:65-79)."""

    def __init__(self, device=0):
        self.lib = load_library()
        st = C.c_int(0)
        self.ctx = self.lib.s2k_create(int(device), C.byref(st))
        if not self.ctx:
            raise S2kError(st.value, self.lib.s2k_strerror(st.value).decode())
        self.device = device

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.s2k_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise S2kError(st, self.lib.s2k_strerror(st).decode() + " -- " + self.lib.s2k_last_error(self.ctx).decode())

    def set_stream(self, hip_stream_handle):
        self._check(self.lib.s2k_set_stream(self.ctx, C.c_void_p(int(hip_stream_handle))))

    def chain_after(self, prev):
        """Double buffering with two engines on one device: this engine's minimizer kernels wait for those of `prev`'s most recent call (and
        nothing else does), so the tail of one call runs beside the first chunk of the next.  Chain both ways and alternate the calls; None unlinks."""
        self._check(self.lib.s2k_chain_after(self.ctx, prev.ctx if prev is not None else None))

    def set_host_batch(self, bases):
        """Bases per sub-batch of `extract` (host buffers): H2D / kernels / D2H of consecutive sub-batches overlap."""
        self._check(self.lib.s2k_set_host_batch(self.ctx, int(bases)))

    def trim(self):
        """release what the context keeps between calls (idle host result blocks, device workspace)"""
        self._check(self.lib.s2k_trim(self.ctx))

    def enable_timing(self, on=True):
        self._check(self.lib.s2k_enable_timing(self.ctx, 1 if on else 0))

    def last_kernel_ms(self, which):
        ms = C.c_float(0)
        self._check(self.lib.s2k_last_kernel_ms(self.ctx, which, C.byref(ms)))
        return float(ms.value)

    def timing_total(self, which):
        """(sum of HIP-event ms, n_calls) since enable_timing(True); which: 0 pipeline, 1 minimizer kernel, 2 k-min-mer kernel"""
        ms, n = C.c_double(0), C.c_uint32(0)
        self._check(self.lib.s2k_timing_total(self.ctx, which, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    # ---- host-buffer API (s2k_extract) ---------------------------------------------------------------
    def extract(self, bases, read_off, l, k, density, mode=HashMode.Hpc, want_minimizers=False, force_serial=False, pack2=True, legacy=False):
        """Batch counterpart of `for r in reads: KminmersIterator::new(r,l,k,d,mode).collect()`.
        Returns a dict of numpy arrays (copies)."""
        bases = _as_u8(bases)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        if len(read_off) == 0:
            raise ValueError("read_off needs n_reads + 1 entries (at least one)")
        if int(read_off[-1]) > len(bases):
            raise ValueError("read_off[-1] = %d lies past the end of bases (%d bytes)" % (int(read_off[-1]), len(bases)))
        n_reads = len(read_off) - 1  # read_off[0] may be > 0: the library rebases the offsets (bases[read_off[0]:read_off[-1]] is used)
        flags = (FLAG_WANT_MINIMIZERS if want_minimizers else 0) | (FLAG_FORCE_SERIAL if force_serial else 0) | (0 if pack2 else FLAG_NO_PACK2) | (FLAG_LEGACY_PATH if legacy else 0)
        p = Params(int(l), int(k), float(density), int(mode), flags)
        res = Result()
        self._check(self.lib.s2k_extract(self.ctx, bases.ctypes.data_as(C.c_void_p), read_off.ctypes.data_as(C.c_void_p),
                                         n_reads, C.byref(p), C.byref(res)))
        try:
            nk, nm = int(res.n_kminmers), int(res.n_minimizers)

            def take(ptr, n, dt):
                if n == 0:
                    return np.zeros(0, dtype=dt)
                return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)

            out = {
                "n": nk, "km_off": take(res.km_off, n_reads + 1, np.uint64), "hash": take(res.hash, nk, np.uint64),
                "start": take(res.start, nk, np.uint32), "end": take(res.end, nk, np.uint32), "rev": take(res.rev, nk, np.uint8),
                "counts": res.counts.as_dict(),
            }
            if want_minimizers:
                out.update({"n_minimizers": nm, "mn_off": take(res.mn_off, n_reads + 1, np.uint64),
                            "mn_j": take(res.mn_j, nm, np.uint32), "mn_jend": take(res.mn_jend, nm, np.uint32),
                            "mn_hash": take(res.mn_hash, nm, np.uint32)})
            return out
        finally:
            self.lib.s2k_result_free(C.byref(res))

    def extract_reads(self, reads, l, k, density, mode=HashMode.Hpc, **kw):
        bases, off = pack_reads(reads)
        return self.extract(bases, off, l, k, density, mode, **kw)

    # ---- device-resident API (s2k_extract_device); pointers are integers (e.g. torch .data_ptr()) ------
    def extract_device(self, d_bases, d_read_off, n_reads, n_bases, l, k, density, mode, out, sync=True, flags=0):
        p = Params(int(l), int(k), float(density), int(mode), int(flags))
        cnt = Counts()
        st = self.lib.s2k_extract_device(self.ctx, C.c_void_p(d_bases), C.c_void_p(d_read_off), n_reads, n_bases, C.byref(p),
                                         C.byref(out), C.byref(cnt) if sync else None)
        self._check(st)
        return cnt.as_dict() if sync else None

    def sync(self):
        cnt = Counts()
        self._check(self.lib.s2k_sync(self.ctx, C.byref(cnt)))
        return cnt.as_dict()

    def synth_bases_device(self, seed, first_base, n, d_ptr):
        self._check(self.lib.s2k_synth_bases_device(self.ctx, seed, first_base, n, C.c_void_p(d_ptr)))

    def synth_hifi_lengths(self, seed, r0, n_reads):
        """lengths of the HiFi-like synthetic reads r0 .. r0+n_reads-1 (BASELINE configs[3]); host array"""
        out = np.empty(n_reads, dtype=np.uint64)
        self.lib.s2k_synth_hifi_lengths(seed, r0, n_reads, C.c_void_p(out.ctypes.data))
        return out

    def synth_hifi_device(self, seed, r0, n_reads, d_read_off_ptr, d_bases_ptr):
        """read r0+i is written at d_bases + d_read_off[i] (device pointers; read_off = prefix of synth_hifi_lengths)"""
        self._check(self.lib.s2k_synth_hifi_device(self.ctx, seed, r0, n_reads, C.c_void_p(d_read_off_ptr), C.c_void_p(d_bases_ptr)))

    def run_file(self, path, l, k, density, mode=HashMode.Regular, batch_bases=256 << 20, flags=0):
        """FASTA/FASTQ file -> totals; the file mode of the reference's CLI (src/main.rs:51-83) on the GPU."""
        p = Params(int(l), int(k), float(density), int(mode), int(flags))
        cnt, sec = Counts(), C.c_double(0)
        self._check(self.lib.s2k_run_file(self.ctx, os.fsencode(path), C.byref(p), batch_bases, C.byref(cnt), C.byref(sec)))
        d = cnt.as_dict()
        d["seconds"] = float(sec.value)
        return d

    def parse_fastx_device(self, d_text, n_bytes, fastq, d_bases=0, bases_capacity=0, d_read_off=0, off_capacity=0):
        """FASTA/FASTQ text in HBM -> (bases, read_off) in HBM (s2k_fastx_parse_device).  Returns (status, n_reads,
        n_bases); status 7 (capacity) still reports the sizes needed."""
        nr, nb = C.c_uint64(0), C.c_uint64(0)
        st = self.lib.s2k_fastx_parse_device(self.ctx, C.c_void_p(d_text), n_bytes, 1 if fastq else 0, C.c_void_p(d_bases or 0),
                                             bases_capacity, C.c_void_p(d_read_off or 0), off_capacity, C.byref(nr), C.byref(nb))
        if st not in (0, 7):
            self._check(st)
        return st, int(nr.value), int(nb.value)

    def hpc_device(self, d_bases, d_read_off, n_reads, n_bases, d_hpc_off, d_hpc, d_pos, capacity, rle=False):
        """rle=True: the run rule of `encode_rle` (only ACTGactgNn collapse, src/hpc.rs:14); else any repeated byte collapses."""
        n = C.c_uint64(0)
        st = self.lib.s2k_hpc_device_ex(self.ctx, C.c_void_p(d_bases), C.c_void_p(d_read_off), n_reads, n_bases,
                                        HPC_RLE_ALPHABET if rle else 0, C.c_void_p(d_hpc_off), C.c_void_p(d_hpc or 0),
                                        C.c_void_p(d_pos or 0), capacity, C.byref(n))
        self._check(st)
        return int(n.value)


    def count_device(self, d_hash, n, d_keys=0, d_counts=0, capacity=0):
        """distinct k-min-mer hashes of d_hash[0..n) and their multiplicities (unordered); returns n_distinct"""
        nd = C.c_uint64(0)
        st = self.lib.s2k_count_device(self.ctx, C.c_void_p(d_hash or 0), n, C.c_void_p(d_keys or 0), C.c_void_p(d_counts or 0), capacity,
                                       C.byref(nd))
        if st != 7 or capacity:
            self._check(st)
        return int(nd.value)

    def count_device_ex(self, d_hash, n, min_count=1, sorted=True, d_keys=0, d_counts=0, capacity=0):
        """(key, count) pairs of the distinct hashes of d_hash[0..n) that occur at least min_count times, in ascending key order
        with sorted=True (s2k_count_device_ex); returns (n_distinct, n_kept).  Raises S2kError(7) when n_kept exceeds a non-zero
        capacity (the exception's n_distinct / n_kept hold the sizes); no outputs asks for the sizes."""
        nd, nk = C.c_uint64(0), C.c_uint64(0)
        st = self.lib.s2k_count_device_ex(self.ctx, C.c_void_p(d_hash or 0), n, min_count, COUNT_SORTED if sorted else 0,
                                          C.c_void_p(d_keys or 0), C.c_void_p(d_counts or 0), capacity, C.byref(nd), C.byref(nk))
        try:
            self._check(st)
        except S2kError as e:
            e.n_distinct, e.n_kept = int(nd.value), int(nk.value)  # set with status 7: the sizes that were needed
            raise
        return int(nd.value), int(nk.value)

    def count_merge_device(self, d_a_keys, d_a_counts, n_a, d_b_keys=0, d_b_counts=0, n_b=0, min_count=1, d_keys=0, d_counts=0, capacity=0):
        """union of two count tables, each strictly ascending by key (s2k_count_merge_device): counts of a key in both added (saturated at
        2^32-1), pairs under min_count dropped, ascending key order; n_b == 0 filters one table.  Returns (n_distinct, n_kept); raises
        S2kError(7) with the sizes when n_kept exceeds a non-zero capacity, S2kError(1) for an input that is not strictly ascending."""
        nd, nk = C.c_uint64(0), C.c_uint64(0)
        st = self.lib.s2k_count_merge_device(self.ctx, C.c_void_p(d_a_keys or 0), C.c_void_p(d_a_counts or 0), n_a, C.c_void_p(d_b_keys or 0),
                                             C.c_void_p(d_b_counts or 0), n_b, min_count, C.c_void_p(d_keys or 0), C.c_void_p(d_counts or 0),
                                             capacity, C.byref(nd), C.byref(nk))
        try:
            self._check(st)
        except S2kError as e:
            e.n_distinct, e.n_kept = int(nd.value), int(nk.value)
            raise
        return int(nd.value), int(nk.value)

    def run_file_count(self, path, l, k, density, mode=HashMode.Regular, min_count=2, batch_bases=256 << 20, counter=None, flags=0):
        """run_file that also counts the k-min-mers (s2k_run_file_count): the totals dict of run_file plus `keys` / `counts` (torch int64 /
        int32 tensors on the device holding the uint64 keys / uint32 counts, ascending by key) of the k-min-mers that occur at least
        min_count times, `n_distinct` and `n_kept`.  With a KminmerCounter the file is added to it and the results cover everything it
        holds (several files: one counter); without one, a counter lives for this call only."""
        own = counter is None
        ctr = KminmerCounter(self) if own else counter
        try:
            p = Params(int(l), int(k), float(density), int(mode), int(flags))
            cnt, sec = Counts(), C.c_double(0)
            self._check(self.lib.s2k_run_file_count(self.ctx, os.fsencode(path), C.byref(p), batch_bases, C.c_void_p(ctr.handle), C.byref(cnt),
                                                    C.byref(sec)))
            d = cnt.as_dict()
            d["seconds"] = float(sec.value)
            keys, counts = ctr.finish(min_count)
            d.update(keys=keys, counts=counts, n_distinct=ctr.last_sizes[0], n_kept=ctr.last_sizes[1])
            return d
        finally:
            if own:
                ctr.close()

    def graph_adjacency(self, edge_keys, n_nodes):
        """The CSR of a graph over 2 * n_nodes oriented nodes (s2k_graph_adjacency) from its edge keys (1-D 64-bit GPU tensor, strictly
        ascending as uint64, both node ids below 2 * n_nodes; S2kError(1) otherwise) -> (row_off, dst): int64 tensor of 2 * n_nodes + 1
        row offsets and int32 tensor of the destination of every edge, on the device."""
        import torch

        if edge_keys.dim() != 1 or edge_keys.element_size() != 8 or not edge_keys.is_cuda:
            raise ValueError("graph_adjacency wants a 1-D 64-bit tensor on the GPU")
        edge_keys = edge_keys.contiguous()
        n, dev = edge_keys.numel(), edge_keys.device
        row_off = torch.empty(2 * int(n_nodes) + 1, dtype=torch.int64, device=dev)
        dst = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_adjacency(self.ctx, C.c_void_p(edge_keys.data_ptr() if n else 0), n, int(n_nodes),
                                                 C.c_void_p(row_off.data_ptr()), C.c_void_p(dst.data_ptr())))
        return row_off, dst[:n]

    def graph_unitigs(self, row_off, dst, n_nodes):
        """The unitigs of a twin-symmetric graph (s2k_graph_unitigs) from its CSR as graph_adjacency returns it (S2kError(1) when the
        CSR breaks a rule or an edge's twin is missing) -> dict of GPU tensors uni_off (int64, n_unitigs + 1), members (int32, n_nodes
        oriented ids: the kept strands in path order), node_unitig / node_pos (int32, n_nodes), circular (uint8, n_unitigs), and the ints
        n_unitigs, n_links."""
        import torch

        if row_off.numel() != 2 * int(n_nodes) + 1 or row_off.element_size() != 8 or dst.element_size() != 4 or not row_off.is_cuda:
            raise ValueError("graph_unitigs wants the row_off (2 * n_nodes + 1, 64-bit) and dst (32-bit) of graph_adjacency on the GPU")
        row_off, dst = row_off.contiguous(), dst.contiguous()
        n, ne, dev = int(n_nodes), dst.numel(), row_off.device
        res = {"uni_off": torch.empty(n + 1, dtype=torch.int64, device=dev), "members": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
               "node_unitig": torch.empty(max(n, 1), dtype=torch.int32, device=dev), "node_pos": torch.empty(max(n, 1), dtype=torch.int32, device=dev),
               "circular": torch.empty(max(n, 1), dtype=torch.uint8, device=dev)}
        o = UnitigOut()
        o.capacity = n  # at most one unitig per node
        for f, t in res.items():
            setattr(o, f, t.data_ptr())
        nu, nl = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_unitigs(self.ctx, C.c_void_p(row_off.data_ptr()), C.c_void_p(dst.data_ptr() if ne else 0), ne, n,
                                               C.byref(o), C.byref(nu), C.byref(nl)))
        t = int(nu.value)
        return {"uni_off": res["uni_off"][:t + 1], "members": res["members"][:n], "node_unitig": res["node_unitig"][:n],
                "node_pos": res["node_pos"][:n], "circular": res["circular"][:t], "n_unitigs": t, "n_links": int(nl.value)}

    def graph_unitig_edges(self, row_off, dst, n_nodes, unitigs):
        """The edges between the oriented unitigs (s2k_graph_unitig_edges): `unitigs` is what graph_unitigs returned for the same CSR
        -> (keys, src_edge): int64 tensors, keys U << 32 | V strictly ascending (as uint64) and the index of the CSR edge each came from."""
        import torch

        row_off, dst = row_off.contiguous(), dst.contiguous()
        ne, dev = dst.numel(), row_off.device
        cap = ne - unitigs["n_links"]
        keys = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        src = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        no = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_unitig_edges(self.ctx, C.c_void_p(row_off.data_ptr()), C.c_void_p(dst.data_ptr() if ne else 0), ne, int(n_nodes),
                                                    *(C.c_void_p(unitigs[f].data_ptr()) for f in ("uni_off", "members", "node_unitig", "node_pos")),
                                                    unitigs["n_unitigs"], C.c_void_p(keys.data_ptr()), C.c_void_p(src.data_ptr()), cap, C.byref(no)))
        return keys[:int(no.value)], src[:int(no.value)]

    def graph_simplify_mask(self, unitig_graph, max_tip, max_bubble):
        """One round of tip clipping and simple-bubble popping (s2k_graph_simplify_mask; the rules are in include/s2k.h) on a UnitigGraph:
        a tip holds at most max_tip members, a bubble branch at most max_bubble; 0 switches a rule off -> dict: remove (uint8 GPU tensor,
        one byte per unitig) and the ints n_tips, n_bubbles (a unitig that meets both rules counts in both), n_removed."""
        import torch

        ug = unitig_graph
        t, ne, dev = ug.n_unitigs, ug.dst.numel(), ug.row_off.device
        row_off, dst, uni_off, counts = ug.row_off.contiguous(), ug.dst.contiguous(), ug.uni_off.contiguous(), ug.counts.contiguous()
        if counts.element_size() != 8 or counts.numel() != t or uni_off.numel() != t + 1 or row_off.numel() != 2 * t + 1:
            raise ValueError("graph_simplify_mask wants a UnitigGraph: 64-bit counts, one per unitig, and the CSR over its oriented unitigs")
        remove = torch.zeros(max(t, 1), dtype=torch.uint8, device=dev)
        nt, nb, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_simplify_mask(self.ctx, C.c_void_p(row_off.data_ptr()), C.c_void_p(dst.data_ptr() if ne else 0), ne, t,
                                                     C.c_void_p(uni_off.data_ptr()), C.c_void_p(counts.data_ptr() if t else 0), int(max_tip),
                                                     int(max_bubble), C.c_void_p(remove.data_ptr()), C.byref(nt), C.byref(nb), C.byref(nr)))
        return {"remove": remove[:t], "n_tips": int(nt.value), "n_bubbles": int(nb.value), "n_removed": int(nr.value)}

    def graph_induced(self, graph, node_keep=None, node_unitig=None, remove=None):
        """The subgraph of a KminmerGraph that its kept nodes induce (s2k_graph_induced).  Kept: node_keep (uint8 GPU tensor, one byte per
        node, non-zero = kept), or, without it, the nodes whose unitig is not removed: node_unitig (UnitigGraph.node_unitig) and remove
        (graph_simplify_mask's).  -> dict of GPU tensors keys, counts, edge_keys, edge_counts (the kept ones, renumbered) and new_id (int32,
        one per old node: its new id, -1 for a removed node)."""
        import torch

        n, ne, dev = graph.n_nodes, graph.n_edges, graph.keys.device
        null = C.c_void_p(0)
        if node_keep is not None:
            node_keep = node_keep.contiguous()
            if node_keep.numel() != n or node_keep.element_size() != 1:
                raise ValueError("graph_induced: node_keep holds one byte per node")
            mask_args = (C.c_void_p(node_keep.data_ptr()), null, null, 0)
        elif node_unitig is not None and remove is not None:
            node_unitig, remove = node_unitig.contiguous(), remove.contiguous()
            if node_unitig.numel() != n or node_unitig.element_size() != 4 or remove.element_size() != 1:
                raise ValueError("graph_induced: node_unitig holds one 32-bit unitig per node, remove one byte per unitig")
            # the number of unitigs is the length of remove: the device refuses a node_unitig entry beyond it
            mask_args = (null, C.c_void_p(node_unitig.data_ptr()), C.c_void_p(remove.data_ptr()), remove.numel())
        else:
            raise ValueError("graph_induced wants node_keep, or node_unitig and remove")
        keys, counts, ek, ec = (x.contiguous() for x in (graph.keys, graph.counts, graph.edge_keys, graph.edge_counts))
        new_id = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        ok, oc = torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        oek, oec = torch.empty(max(ne, 1), dtype=torch.int64, device=dev), torch.empty(max(ne, 1), dtype=torch.int32, device=dev)
        nn, nne = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_induced(self.ctx, _p(keys, n), _p(counts, n), n, _p(ek, ne), _p(ec, ne), ne, *mask_args,
                                               _p(new_id), _p(ok), _p(oc), n, _p(oek), _p(oec), ne, C.byref(nn), C.byref(nne)))
        a, b = int(nn.value), int(nne.value)
        return {"keys": ok[:a], "counts": oc[:a], "edge_keys": oek[:b], "edge_counts": oec[:b], "new_id": new_id[:n]}

    def unitig_sequences(self, uni_off, members, circular, n_nodes, node_seqs):
        """The unitigs' base-space sequences (s2k_unitig_sequences) from the arrays graph_unitigs returned and a NodeSequences ->
        (out_off, out, overlap): int64 tensor of n_unitigs + 1 offsets, uint8 tensor of the bases (unitig t is out[out_off[t] :
        out_off[t + 1]]), int32 tensor of the overlap that leaves each oriented unitig 2 t + s."""
        import torch

        uni_off, members, circular = uni_off.contiguous(), members.contiguous(), circular.contiguous()
        t, n, dev = circular.numel(), int(n_nodes), uni_off.device
        out_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        overlap = torch.zeros(max(2 * t, 1), dtype=torch.int32, device=dev)
        ns, nb = node_seqs.struct(), C.c_uint64(0)
        args = (self.ctx, C.c_void_p(uni_off.data_ptr()), C.c_void_p(members.data_ptr() if n else 0), C.c_void_p(circular.data_ptr() if t else 0), t, n,
                C.byref(ns), C.c_void_p(out_off.data_ptr()))
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_unitig_sequences(*args, None, C.c_void_p(overlap.data_ptr()), 0, C.byref(nb)))
        total = int(nb.value)
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        if total:
            torch.cuda.synchronize(dev)
            self._check(self.lib.s2k_unitig_sequences(*args, C.c_void_p(out.data_ptr()), C.c_void_p(overlap.data_ptr()), total, C.byref(nb)))
        return out_off, out[:total], overlap[:2 * t]

    def table_vote_keys(self, table, o, k):
        """The vote keys of one batch (s2k_table_vote_keys; the rule is in include/s2k.h): o = the GPU tensors extract_device wrote with
        FLAG_WANT_MINIMIZERS plus the batch's `bases` and `read_off`; table: the CountTable of the nodes.  Two calls: the size, then the
        keys.  -> int64 GPU tensor, three keys (whole, forward end, reverse end) per item of the table, in item order."""
        import torch

        nr = o["km_off"].numel() - 1
        i, nk = _seq_in(o, nr), C.c_uint64(0)
        b, ro = o["bases"], o["read_off"]
        args = (table.handle, nr, C.byref(i), int(k), C.c_void_p(b.data_ptr() if b.numel() else 0), C.c_void_p(ro.data_ptr()))
        torch.cuda.synchronize(ro.device)
        self._check(self.lib.s2k_table_vote_keys(*args, None, 0, C.byref(nk)))
        n = int(nk.value)
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=ro.device)
        if n:
            torch.cuda.synchronize(ro.device)
            self._check(self.lib.s2k_table_vote_keys(*args, C.c_void_p(keys.data_ptr()), n, C.byref(nk)))
        return keys[:n]

    def table_vote_representatives(self, table, vote_table, o, k, ordinal_base, best):
        """best[i] = max(best[i], votes and ordinal of x) over the batch's items x whose hash is key i of `table`
        (s2k_table_vote_representatives); vote_table: the CountTable over the counted vote keys of every batch; best: int64 GPU tensor,
        one entry per key, zeroed before the first batch.  -> the batch's items, to add to ordinal_base."""
        import torch

        nr = o["km_off"].numel() - 1
        i = _seq_in(o, nr)
        b, ro = o["bases"], o["read_off"]
        if best.numel() < table.n or best.element_size() != 8 or not best.is_contiguous():
            raise ValueError("best holds one 64-bit entry per key of the table")
        torch.cuda.synchronize(ro.device)
        self._check(self.lib.s2k_table_vote_representatives(table.handle, vote_table.handle, nr, C.byref(i), int(k),
                                                            C.c_void_p(b.data_ptr() if b.numel() else 0), C.c_void_p(ro.data_ptr()), int(ordinal_base),
                                                            C.c_void_p(best.data_ptr() if table.n else 0)))
        return i.km_capacity

    def vote_ordinals(self, best):
        """-> int64 GPU tensor rep: the ordinal packed into every best[i], all ones where best[i] == 0 (s2k_vote_ordinals): the rep that
        s2k_table_node_sequences takes"""
        import torch

        best = best.contiguous()
        rep = torch.empty(max(best.numel(), 1), dtype=torch.int64, device=best.device)
        torch.cuda.synchronize(best.device)
        self._check(self.lib.s2k_vote_ordinals(self.ctx, C.c_void_p(best.data_ptr() if best.numel() else 0), best.numel(), C.c_void_p(rep.data_ptr())))
        return rep[:best.numel()]

    def unitig_node_places(self, uni_off, members, node_unitig, node_pos, circular):
        """Where every node lies on the oriented unitigs (s2k_unitig_node_places), from the arrays graph_unitigs returned -> int32 GPU
        tensor of shape (n_nodes, 4): row i is the NodePlace record (unitig, pos, len, circular) of the forward oriented node 2 i.
        S2kError(1) when the arrays are not a decomposition of the nodes."""
        import torch

        uni_off, members, node_unitig, node_pos, circular = (x.contiguous() for x in (uni_off, members, node_unitig, node_pos, circular))
        n, t, dev = node_unitig.numel(), circular.numel(), uni_off.device
        if uni_off.numel() != t + 1 or members.numel() != n or node_pos.numel() != n or uni_off.element_size() != 8 or members.element_size() != 4:
            raise ValueError("unitig_node_places wants uni_off (n_unitigs + 1, 64-bit), members / node_unitig / node_pos (n_nodes, 32-bit), circular")
        place = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_unitig_node_places(self.ctx, *(C.c_void_p(x.data_ptr() if x.numel() else 0) for x in (uni_off, members, node_unitig,
                                                                                                                      node_pos, circular)),
                                                    n, t, C.c_void_p(place.data_ptr())))
        return place[:n]

    def paths_spans(self, unitig_graph, paths, edge_support=None):
        """The span keys of one batch's ReadPaths over a UnitigGraph (s2k_paths_spans; the definitions are in include/s2k.h): for every
        step that crosses its whole unitig from an in-edge a to an out-edge b the key a << 32 | b, then its twin's.  Two calls: the
        sizes, then the keys.  edge_support: an int64 GPU tensor of n_edges entries (zeroed by the caller) that gains the steps that
        follow every edge and its twin.  -> (keys, n_followed, n_off_graph): int64 GPU tensor in step order, and the linked steps that
        follow an edge / follow none."""
        import torch

        ug, dev = unitig_graph, paths.path_off.device
        t, ne, ns, nr = ug.n_unitigs, ug.dst.numel(), paths.n_steps, paths.path_off.numel() - 1
        row_off, dst, uni_off = ug.row_off.contiguous(), ug.dst.contiguous(), ug.uni_off.contiguous()
        if row_off.numel() != 2 * t + 1 or row_off.element_size() != 8 or dst.element_size() != 4 or uni_off.numel() != t + 1:
            raise ValueError("paths_spans wants a UnitigGraph: the CSR over its oriented unitigs and uni_off")
        if edge_support is not None and (edge_support.numel() != ne or edge_support.element_size() != 8 or not edge_support.is_contiguous()):
            raise ValueError("edge_support holds one 64-bit entry per edge")
        o, keep = _paths_struct(paths, ("unitig", "pos", "count", "flags"), ns)
        nk, nf, no = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        args = (self.ctx, nr, C.byref(o), ns, _p(row_off), _p(dst, ne), ne, _p(uni_off), t)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_spans(*args, None, 0, None, C.byref(nk), C.byref(nf), C.byref(no)))
        n = int(nk.value)
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_spans(*args, _p(keys), n, _p(edge_support, ne), C.byref(nk), C.byref(nf), C.byref(no)))
        return keys[:n], int(nf.value), int(no.value)

    def graph_resolve_mask(self, unitig_graph, span_keys, span_counts, min_support=2):
        """Which unitigs of a UnitigGraph a span table resolves (s2k_graph_resolve_mask; the rule is in include/s2k.h): span_keys (64-bit,
        strictly ascending as uint64) and span_counts (32-bit) on the GPU -> dict: resolved (uint8 GPU tensor, one byte per unitig),
        partner (int32 GPU tensor, one entry per edge: the out-edge matched to an edge that enters a resolved unitig, -1 = NO_PARTNER
        otherwise) and the ints n_candidates, n_resolved."""
        import torch

        ug = unitig_graph
        t, ne, dev = ug.n_unitigs, ug.dst.numel(), ug.row_off.device
        row_off, dst, sk, sc = ug.row_off.contiguous(), ug.dst.contiguous(), span_keys.contiguous(), span_counts.contiguous()
        n = sk.numel()
        if row_off.numel() != 2 * t + 1 or sk.element_size() != 8 or sc.element_size() != 4 or sc.numel() != n:
            raise ValueError("graph_resolve_mask wants a UnitigGraph and a span table: 64-bit keys, 32-bit counts of the same length")
        resolved = torch.zeros(max(t, 1), dtype=torch.uint8, device=dev)
        partner = torch.full((max(ne, 1),), -1, dtype=torch.int32, device=dev)
        nc, nr = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_resolve_mask(self.ctx, C.c_void_p(row_off.data_ptr()), C.c_void_p(dst.data_ptr() if ne else 0), ne, t,
                                                    C.c_void_p(sk.data_ptr() if n else 0), C.c_void_p(sc.data_ptr() if n else 0), n, int(min_support),
                                                    C.c_void_p(resolved.data_ptr()), C.c_void_p(partner.data_ptr()), C.byref(nc), C.byref(nr)))
        return {"resolved": resolved[:t], "partner": partner[:ne], "n_candidates": int(nc.value), "n_resolved": int(nr.value)}

    def graph_untangle(self, unitig_graph, resolved, partner):
        """Every resolved unitig of a UnitigGraph duplicated once per matched in-edge / out-edge pair (s2k_graph_untangle; the
        definitions are in include/s2k.h): resolved (uint8, one byte per unitig) and partner (int32, one entry per edge) as
        graph_resolve_mask returned them.  Two calls: the sizes, then the arrays.  -> dict of GPU tensors copy_off (int64, n_unitigs + 1),
        origin (int32, the unitig of every copy), copy_count (int64, the unitig's count shared among its copies by edge count), keys
        (int64, the n_edges edges over the oriented copies, strictly ascending as uint64: graph_adjacency takes them) and src_edge
        (int64, the old edge of every key), and the ints n_copies, n_duplicated."""
        import torch

        ug = unitig_graph
        t, ne, dev = ug.n_unitigs, ug.dst.numel(), ug.row_off.device
        row_off, dst, counts, ec = ug.row_off.contiguous(), ug.dst.contiguous(), ug.counts.contiguous(), ug.edge_counts.contiguous()
        resolved, partner = resolved.contiguous(), partner.contiguous()
        if (row_off.numel() != 2 * t + 1 or row_off.element_size() != 8 or dst.element_size() != 4 or resolved.numel() != t or resolved.element_size() != 1
                or partner.numel() != ne or partner.element_size() != 4 or counts.numel() != t or counts.element_size() != 8 or ec.numel() != ne
                or ec.element_size() != 4):
            raise ValueError("graph_untangle wants a UnitigGraph, one resolved byte per unitig and one 32-bit partner per edge")
        args = (self.ctx, _p(row_off), _p(dst, ne), ne, t, _p(resolved, t), _p(partner, ne), _p(counts, t), _p(ec, ne))
        nc, nd = C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_untangle(*args, None, None, None, None, None, 0, C.byref(nc), C.byref(nd)))
        n = int(nc.value)
        copy_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        origin = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        copy_count = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        keys, src = torch.empty(max(ne, 1), dtype=torch.int64, device=dev), torch.empty(max(ne, 1), dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_graph_untangle(*args, _p(copy_off), _p(origin), _p(copy_count), _p(keys), _p(src), n, C.byref(nc), C.byref(nd)))
        return {"copy_off": copy_off, "origin": origin[:n], "copy_count": copy_count[:n], "keys": keys[:ne], "src_edge": src[:ne], "n_copies": n,
                "n_duplicated": int(nd.value)}

    def unitig_expand(self, outer, origin, uni_off, members, circular):
        """The contigs of an untangled graph as node members (s2k_unitig_expand): outer = what graph_unitigs returned with the copies
        as its nodes, origin = graph_untangle's, and uni_off / members / circular = the decomposition the copies came from.  Two
        calls: the size, then the arrays.  -> dict of GPU tensors uni_off (int64, n_contigs + 1), members, node_unitig, node_pos (int32,
        one per node instance; instance m is the oriented node 2 m + its old orientation bit), circular (uint8) and node_origin (int32,
        the old node of every instance), and the int n_members."""
        import torch

        oo, om, oc, origin = (x.contiguous() for x in (outer["uni_off"], outer["members"], outer["circular"], origin))
        uni_off, members, circular = uni_off.contiguous(), members.contiguous(), circular.contiguous()
        nt, ncp, t, n, dev = oc.numel(), origin.numel(), circular.numel(), members.numel(), uni_off.device
        if (oo.numel() != nt + 1 or om.numel() != ncp or uni_off.numel() != t + 1 or oo.element_size() != 8 or uni_off.element_size() != 8
                or om.element_size() != 4 or origin.element_size() != 4 or members.element_size() != 4):
            raise ValueError("unitig_expand wants the outer decomposition over the copies, one 32-bit origin per copy, and the inner decomposition")
        args = (self.ctx, _p(oo), _p(om, ncp), _p(oc, nt), nt, ncp, _p(origin, ncp), _p(uni_off), _p(members, n), _p(circular, t), t, n)
        nm = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_unitig_expand(*args, None, None, None, None, None, None, 0, C.byref(nm)))
        m = int(nm.value)
        res = {"uni_off": torch.zeros(nt + 1, dtype=torch.int64, device=dev), "members": torch.empty(max(m, 1), dtype=torch.int32, device=dev),
               "node_unitig": torch.empty(max(m, 1), dtype=torch.int32, device=dev), "node_pos": torch.empty(max(m, 1), dtype=torch.int32, device=dev),
               "circular": torch.empty(max(nt, 1), dtype=torch.uint8, device=dev), "node_origin": torch.empty(max(m, 1), dtype=torch.int32, device=dev)}
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_unitig_expand(*args, *(_p(res[f]) for f in ("uni_off", "members", "node_unitig", "node_pos", "circular", "node_origin")),
                                               m, C.byref(nm)))
        out = {f: res[f][:m] for f in ("members", "node_unitig", "node_pos", "node_origin")}
        out.update(uni_off=res["uni_off"], circular=res["circular"][:nt], n_members=m)
        return out

    def unitig_member_offsets(self, uni_off, members, circular, n_nodes, node_seqs):
        """Where every member's piece starts in the stitched unitigs (s2k_unitig_member_offsets: the stitch without its copy) ->
        (member_off, out_off, overlap, n_bases): int64 tensors of n_nodes and n_unitigs + 1 entries, the int32 overlap that leaves
        each oriented unitig, and the bases of all unitigs; out_off and overlap equal those of unitig_sequences."""
        import torch

        uni_off, members, circular = uni_off.contiguous(), members.contiguous(), circular.contiguous()
        t, n, dev = circular.numel(), int(n_nodes), uni_off.device
        member_off = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        out_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        overlap = torch.zeros(max(2 * t, 1), dtype=torch.int32, device=dev)
        ns, nb = node_seqs.struct(), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_unitig_member_offsets(self.ctx, C.c_void_p(uni_off.data_ptr()), C.c_void_p(members.data_ptr() if n else 0),
                                                       C.c_void_p(circular.data_ptr() if t else 0), t, n, C.byref(ns), C.c_void_p(member_off.data_ptr()),
                                                       C.c_void_p(out_off.data_ptr()), C.c_void_p(overlap.data_ptr()), C.byref(nb)))
        return member_off[:n], out_off, overlap[:2 * t], int(nb.value)

    def paths_walks(self, unitig_graph, paths, offsets, seq_len, edge=True):
        """The walks of one batch's ReadPaths over a UnitigGraph, with base coordinates (s2k_paths_walks; the definitions are in
        include/s2k.h).  offsets: the (member_off, out_off, overlap, ...) that unitig_member_offsets returned for the graph; seq_len:
        the seq_len of its NodeSequences.  Two calls: the sizes, then the arrays.  -> dict of GPU tensors walk_off (int64, n_reads + 1),
        first_step, items, path_len, path_start, path_end (int64), n_steps, flags (int32), qstart, qend (int32, only when the paths
        carry start and end), edge (int32 per step, -1 = NO_EDGE; only with edge=True), and the ints n_walks, n_followed, n_off_graph."""
        import torch

        ug, dev = unitig_graph, paths.path_off.device
        t, ne, ns, nr, n = ug.n_unitigs, ug.dst.numel(), paths.n_steps, paths.path_off.numel() - 1, ug.members.numel()
        row_off, dst, uni_off, members, circular = (x.contiguous() for x in (ug.row_off, ug.dst, ug.uni_off, ug.members, ug.circular))
        member_off, out_off, overlap, seq_len = (x.contiguous() for x in (offsets[0], offsets[1], offsets[2], seq_len))
        if (row_off.numel() != 2 * t + 1 or row_off.element_size() != 8 or dst.element_size() != 4 or uni_off.numel() != t + 1 or member_off.numel() != n
                or member_off.element_size() != 8 or out_off.numel() != t + 1 or overlap.numel() != 2 * t or overlap.element_size() != 4
                or seq_len.numel() != n or seq_len.element_size() != 4):
            raise ValueError("paths_walks wants a UnitigGraph, the offsets Engine.unitig_member_offsets returned for it and one 32-bit seq_len per node")
        o, keep = _paths_struct(paths, ("unitig", "pos", "count", "flags", "start", "end"), ns)
        args = (self.ctx, nr, C.byref(o), ns, _p(row_off), _p(dst, ne), ne, _p(uni_off), _p(circular, t), t, _p(member_off, n), _p(out_off), _p(overlap, t),
                _p(seq_len, n), _p(members, n), n)
        nw, nf, no = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_walks(*args, None, C.byref(nw), C.byref(nf), C.byref(no)))
        m = int(nw.value)
        res = {"walk_off": torch.zeros(nr + 1, dtype=torch.int64, device=dev)}
        for f in ("first_step", "items", "path_len", "path_start", "path_end"):
            res[f] = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        for f in ("n_steps", "flags") + (("qstart", "qend") if "start" in keep and "end" in keep else ()):
            res[f] = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        if edge:
            res["edge"] = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)
        w = WalkOut()
        w.capacity = m
        for f, x in res.items():
            setattr(w, f, x.data_ptr())
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_walks(*args, C.byref(w), C.byref(nw), C.byref(nf), C.byref(no)))
        out = {f: (x if f == "walk_off" else x[:ns] if f == "edge" else x[:m]) for f, x in res.items()}
        out.update(n_walks=m, n_followed=int(nf.value), n_off_graph=int(no.value))
        return out

    def paths_bridge(self, unitig_graph, paths, max_gap, max_slip, join=False):
        """One batch's ReadPaths with the error gaps bridged over a UnitigGraph (s2k_paths_bridge; the definitions are in include/s2k.h):
        steps at most max_gap items apart on one unitig are merged, steps at most max_gap items apart across one edge are extended to
        the edge, where the gap in the read and the gap on the graph differ by at most max_slip.  Two calls: the sizes, then the arrays.
        -> dict of GPU tensors path_off (int64, n_reads + 1), unitig, pos, count, item, flags, matched (int32; start, end only when the
        paths carry them), join (uint8 per input step: 0 none, 1 the same unitig, 2 across an edge; only with join=True), and the ints
        n_steps, n_merged, n_bridged."""
        import torch

        ug, dev = unitig_graph, paths.path_off.device
        t, ne, ns, nr = ug.n_unitigs, ug.dst.numel(), paths.n_steps, paths.path_off.numel() - 1
        row_off, dst, uni_off, circular = (x.contiguous() for x in (ug.row_off, ug.dst, ug.uni_off, ug.circular))
        if (row_off.numel() != 2 * t + 1 or row_off.element_size() != 8 or dst.element_size() != 4 or uni_off.numel() != t + 1 or uni_off.element_size() != 8
                or circular.element_size() != 1):
            raise ValueError("paths_bridge wants a UnitigGraph: the CSR over its oriented unitigs, uni_off and circular")
        i, keep = _paths_struct(paths, ReadPaths.STEP_FIELDS, ns)
        args = (self.ctx, nr, C.byref(i), ns, _p(row_off), _p(dst, ne), ne, _p(uni_off), _p(circular, t), t, int(max_gap), int(max_slip))
        res = {"path_off": torch.zeros(nr + 1, dtype=torch.int64, device=dev)}
        o = ThreadOut()
        o.path_off = res["path_off"].data_ptr()
        no, nm, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_bridge(*args, C.byref(o), None, None, C.byref(no), C.byref(nm), C.byref(nb)))
        m = int(no.value)
        per_step = {"join": torch.uint8} if join else {}
        _paths_out(o, res, keep, m, per_step, ns)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_bridge(*args, C.byref(o), _p(res["matched"]), _p(res.get("join")), C.byref(no), C.byref(nm), C.byref(nb)))
        return _paths_result(res, per_step, m, ns, n_merged=int(nm.value), n_bridged=int(nb.value))

    def unitig_copy_places(self, outer, origin, uni_off, circular):
        """Where every copy of an untangled graph lies on its contigs (s2k_unitig_copy_places; the definitions are in include/s2k.h):
        outer = what graph_unitigs returned with the copies as its nodes, origin = graph_untangle's, uni_off / circular = the
        decomposition the copies came from -> int32 GPU tensor of shape (n_copies, 4): row c is the NodePlace record (unitig, pos, len,
        circular) of the forward oriented copy 2 c on the oriented contigs."""
        import torch

        oo, om, oc, origin = (x.contiguous() for x in (outer["uni_off"], outer["members"], outer["circular"], origin))
        uni_off, circular = uni_off.contiguous(), circular.contiguous()
        nt, ncp, t, dev = oc.numel(), origin.numel(), circular.numel(), uni_off.device
        if (oo.numel() != nt + 1 or om.numel() != ncp or uni_off.numel() != t + 1 or oo.element_size() != 8 or uni_off.element_size() != 8
                or om.element_size() != 4 or origin.element_size() != 4 or oc.element_size() != 1 or circular.element_size() != 1):
            raise ValueError("unitig_copy_places wants the outer decomposition over the copies, one 32-bit origin per copy, and the inner uni_off and circular")
        place = torch.empty((max(ncp, 1), 4), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_unitig_copy_places(self.ctx, _p(oo), _p(om, ncp), _p(oc, nt), nt, ncp, _p(origin, ncp), _p(uni_off), _p(circular, t), t, _p(place)))
        return place[:ncp]

    def paths_lift(self, unitig_graph, paths, resolved, partner, copy_off, copy_place, n_contigs, contig_items=None, step_copy=False, join=False):
        """One batch's ReadPaths on a UnitigGraph lifted onto the contigs of its untangling (s2k_paths_lift; the definitions are in
        include/s2k.h).  resolved, partner: what graph_untangle took; copy_off: what it returned; copy_place: unitig_copy_places' tensor;
        contig_items: an int64 GPU tensor of n_contigs entries (zeroed by the caller) that gains the items every contig carries.  Two
        calls: the sizes, then the arrays.  -> dict of GPU tensors path_off (int64, n_reads + 1), unitig, pos, count, item, flags,
        matched (int32; start, end only when the paths carry them), step_copy (int32 per input step, -1 = NO_COPY: dropped; only with
        step_copy=True), join (uint8 per input step; only with join=True), and the ints n_steps, n_merged, n_dropped, n_conflicts."""
        import torch

        ug, dev = unitig_graph, paths.path_off.device
        t, ne, ns, nr, ncp = ug.n_unitigs, ug.dst.numel(), paths.n_steps, paths.path_off.numel() - 1, copy_place.shape[0]
        row_off, dst, uni_off, circular = (x.contiguous() for x in (ug.row_off, ug.dst, ug.uni_off, ug.circular))
        resolved, partner, copy_off, copy_place = (x.contiguous() for x in (resolved, partner, copy_off, copy_place))
        if (row_off.numel() != 2 * t + 1 or row_off.element_size() != 8 or dst.element_size() != 4 or uni_off.numel() != t + 1 or uni_off.element_size() != 8
                or circular.element_size() != 1 or resolved.numel() != t or resolved.element_size() != 1 or partner.numel() != ne
                or partner.element_size() != 4 or copy_off.numel() != t + 1 or copy_off.element_size() != 8 or copy_place.element_size() != 4
                or copy_place.numel() != 4 * ncp):
            raise ValueError("paths_lift wants a UnitigGraph, one resolved byte per unitig, one 32-bit partner per edge, copy_off (n_unitigs + 1, 64-bit) "
                             "and the (n_copies, 4) records of unitig_copy_places")
        if contig_items is not None and (contig_items.numel() != n_contigs or contig_items.element_size() != 8 or not contig_items.is_contiguous()):
            raise ValueError("contig_items holds one 64-bit entry per contig")
        i, keep = _paths_struct(paths, ReadPaths.STEP_FIELDS, ns)
        matched_in = paths.matched.contiguous() if paths.matched is not None else None
        args = (self.ctx, nr, C.byref(i), ns, _p(matched_in, ns), _p(row_off), _p(dst, ne), ne, _p(uni_off), _p(circular, t), t, _p(resolved, t), _p(partner, ne),
                _p(copy_off), _p(copy_place, ncp), ncp, int(n_contigs))
        res = {"path_off": torch.zeros(nr + 1, dtype=torch.int64, device=dev)}
        o = ThreadOut()
        o.path_off = res["path_off"].data_ptr()
        tot = [C.c_uint64(0) for _ in range(4)]
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_lift(*args, C.byref(o), None, None, None, None, *(C.byref(x) for x in tot)))
        m = int(tot[0].value)
        per_step = {**({"step_copy": torch.int32} if step_copy else {}), **({"join": torch.uint8} if join else {})}
        _paths_out(o, res, keep, m, per_step, ns)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_paths_lift(*args, C.byref(o), _p(res["matched"]), _p(res.get("step_copy")), _p(res.get("join")),
                                            _p(contig_items, n_contigs), *(C.byref(x) for x in tot)))
        return _paths_result(res, per_step, m, ns, n_merged=int(tot[1].value), n_dropped=int(tot[2].value), n_conflicts=int(tot[3].value))

    def walks_targets(self, walks, step_unitig, out_off, out, overlap):
        """The bases of every walk's path interval (s2k_walks_targets; the definitions are in include/s2k.h).  walks: a ReadWalks (or
        anything with first_step, n_steps, path_start, path_end, flags); step_unitig: the oriented unitig of every step of its paths;
        out_off, out: the pair UnitigGraph.sequences returned; overlap: the graph's.  Two calls: the sizes, then the bytes.  -> dict of
        GPU tensors tgt_off (int64, n_walks + 1), tgt (uint8), bad (uint8 per walk), and the int n_bytes."""
        import torch

        nw, dev, args, keep = _walk_args("walks_targets", walks, step_unitig, out_off, out, overlap)
        tgt_off = torch.zeros(nw + 1, dtype=torch.int64, device=dev)
        bad = torch.zeros(max(nw, 1), dtype=torch.uint8, device=dev)
        nb = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_walks_targets(self.ctx, *args, None, None, None, 0, C.byref(nb)))
        n = int(nb.value)
        tgt = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_walks_targets(self.ctx, *args, _p(tgt_off), _p(tgt), _p(bad), n, C.byref(nb)))
        return {"tgt_off": tgt_off, "tgt": tgt[:n], "bad": bad[:nw], "n_bytes": n}

    def align_pairs(self, query, target, q_begin, q_end, t_begin, t_end, max_edits=ALIGN_MAX_EDITS):
        """Global unit-cost alignment of many pairs of byte intervals (s2k_align_pairs; the rule is in include/s2k.h): pair i aligns
        query[q_begin[i] : q_end[i]] with target[t_begin[i] : t_end[i]] (uint8 GPU tensors; int64 GPU tensors of one length).  Two
        calls: the sizes, then the runs.  -> dict of GPU tensors edits, flags, n_ops, matches (int32 per pair), ops_off (int64, n_pairs
        + 1), ops (int32 per run: len << 4 | op; the CIGAR of pair i is ops[ops_off[i] : ops_off[i] + n_ops[i]]), and the int
        n_ops_bound.  A pair whose distance exceeds max_edits has flags & ALIGN_OVER, edits = max_edits + 1 and no run."""
        import torch

        query, target = query.contiguous(), target.contiguous()
        iv = [x.contiguous() for x in (q_begin, q_end, t_begin, t_end)]
        n, dev = iv[0].numel(), query.device
        if any(x.numel() != n or x.element_size() != 8 for x in iv) or query.element_size() != 1 or target.element_size() != 1:
            raise ValueError("align_pairs wants two byte pools and four 64-bit interval arrays of one length")
        args = (self.ctx, _p(query, query.numel()), query.numel(), _p(target, target.numel()), target.numel(), *(_p(x, n) for x in iv), n, int(max_edits))
        o, res, _ = _align_out(n, dev, fields=("edits", "flags", "ops_off"))
        nb = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_align_pairs(*args, C.byref(o), C.byref(nb)))
        m = int(nb.value)
        o, res, cut = _align_out(n, dev, m, res)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_align_pairs(*args, C.byref(o), C.byref(nb)))
        return {**cut(), "n_ops_bound": m}

    def walks_segments(self, unitig_graph, walks, offsets, seq_len, q_begin, tgt_off, bad, source, outs, src_step=None, src_pos=None, seg_len=SEGMENT_LEN):
        """Every walk cut into segment pairs at a thinned, strictly increasing subset of its anchor k-min-mers (s2k_walks_segments; the
        rule is in include/s2k.h).  walks: a ReadWalks over unitig_graph (its paths give unitig, pos, count per step); offsets, seq_len:
        as paths_walks takes them; q_begin: where every walk's query interval starts in the batch's bases (int64); tgt_off, bad: what
        walks_targets returned; source: the ReadPaths that UnitigGraph.thread wrote for the same reads (path_off, pos, count, item);
        outs: the batch's extraction (km_off, start); src_step (int64 per source step, NO_STEP = -1 for none; None: the identity) and
        src_pos (int32; None: source.pos): where every source step went.  Two calls: the sizes, then the intervals.  -> dict of int64
        GPU tensors seg_off (n_walks + 1), q_begin, q_end, t_begin, t_end (one per segment: Engine.align_pairs takes them unchanged),
        the int n_segments and the SEGMENT_STATS counters in stats."""
        import torch

        ug, paths, dev = unitig_graph, walks.paths, walks.walk_off.device
        if walks.qstart is None or walks.qend is None:
            raise ValueError("walks_segments wants walks whose paths carry start and end")
        t, n, ns, nr = ug.n_unitigs, ug.members.numel(), paths.n_steps, walks.walk_off.numel() - 1
        uni_off, members, circular = (x.contiguous() for x in (ug.uni_off, ug.members, ug.circular))
        member_off, out_off, overlap, seq_len = (x.contiguous() for x in (offsets[0], offsets[1], offsets[2], seq_len))
        rec = {f: getattr(walks, f).contiguous() for f in ("walk_off", "first_step", "n_steps", "qstart", "qend", "path_start", "path_end", "flags")}
        nw = rec["first_step"].numel()
        q_begin, tgt_off, bad = q_begin.contiguous(), tgt_off.contiguous(), bad.contiguous()
        if (uni_off.numel() != t + 1 or member_off.numel() != n or member_off.element_size() != 8 or out_off.numel() != t + 1 or overlap.numel() != 2 * t
                or overlap.element_size() != 4 or seq_len.numel() != n or seq_len.element_size() != 4):
            raise ValueError("walks_segments wants a UnitigGraph, the offsets Engine.unitig_member_offsets returned for it and one 32-bit seq_len per node")
        if (any(rec[f].numel() != nw for f in rec if f != "walk_off") or [rec[f].element_size() for f in rec] != [8, 8, 4, 4, 4, 8, 8, 4]
                or q_begin.numel() != nw or q_begin.element_size() != 8 or tgt_off.numel() != nw + 1 or tgt_off.element_size() != 8
                or bad.numel() != nw or bad.element_size() != 1):
            raise ValueError("walks_segments wants the walk records, one 64-bit q_begin and one bad byte per walk, and tgt_off of n_walks + 1 entries")
        km_off, start = outs["km_off"].contiguous(), outs["start"].contiguous()
        nsrc = source.n_steps
        if source.path_off.numel() != nr + 1 or km_off.numel() != nr + 1 or km_off.element_size() != 8 or start.element_size() != 4:
            raise ValueError("walks_segments wants the source paths and the extraction of the walks' reads")
        maps = [None if x is None else x.contiguous() for x in (src_step, src_pos)]
        if any(x is not None and (x.numel() != nsrc or x.element_size() != sz) for x, sz in zip(maps, (8, 4))):
            raise ValueError("src_step holds one 64-bit entry and src_pos one 32-bit entry per source step")
        wo = WalkOut()
        wo.capacity = nw
        for f, x in rec.items():
            setattr(wo, f, x.data_ptr() if x.numel() else 0)
        po, keep_p = _paths_struct(paths, ("unitig", "pos", "count"), ns)
        so, keep_s = _paths_struct(source, ("pos", "count", "item"), nsrc)
        d = DeviceOut()
        d.km_off, d.start = km_off.data_ptr(), start.data_ptr() if start.numel() else 0
        args = (self.ctx, nr, C.byref(wo), nw, C.byref(po), ns, _p(uni_off), _p(members, n), _p(circular, t), t, _p(member_off, n), _p(out_off), _p(overlap, t),
                _p(seq_len, n), n, _p(q_begin, nw), _p(tgt_off), _p(bad, nw), C.byref(so), nsrc, _p(maps[0], nsrc), _p(maps[1], nsrc), C.byref(d), int(seg_len))
        total, stats = C.c_uint64(0), (C.c_uint64 * SEGMENT_STATS_WORDS)()
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_walks_segments(*args, None, C.byref(total), stats))
        m = int(total.value)
        res = {"seg_off": torch.zeros(nw + 1, dtype=torch.int64, device=dev)}
        for f in ("q_begin", "q_end", "t_begin", "t_end"):
            res[f] = torch.zeros(max(m, 1), dtype=torch.int64, device=dev)
        o = SegmentOut()
        o.capacity = m
        for f, x in res.items():
            setattr(o, f, x.data_ptr())
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_walks_segments(*args, C.byref(o), C.byref(total), stats))
        out = {f: (x if f == "seg_off" else x[:m]) for f, x in res.items()}
        out.update(n_segments=m, stats={f: int(stats[i]) for i, f in enumerate(SEGMENT_STATS)})
        return out

    def align_join(self, seg_off, bad, segments):
        """The segments' alignments put back together, one per walk (s2k_align_join; the rule is in include/s2k.h).  seg_off, bad: what
        walks_segments and walks_targets returned; segments: what align_pairs returned for the segment pairs (anything with edits,
        flags, ops_off, n_ops, matches, ops as attributes or keys).  Two calls: the size, then the runs.  -> dict of GPU tensors edits,
        flags, n_ops, matches (int32 per walk), ops_off (int64, n_walks + 1, compact), ops (int32 per joined run) and the int
        n_ops_total."""
        import torch

        get = segments.get if isinstance(segments, dict) else lambda f: getattr(segments, f)
        sg = {f: get(f).contiguous() for f in ("edits", "flags", "ops_off", "n_ops", "matches", "ops")}
        seg_off, bad = seg_off.contiguous(), bad.contiguous()
        nw, nsg, dev = seg_off.numel() - 1, sg["ops_off"].numel() - 1, seg_off.device
        if (seg_off.element_size() != 8 or bad.numel() != nw or bad.element_size() != 1 or sg["ops_off"].element_size() != 8
                or any(sg[f].element_size() != 4 or sg[f].numel() < nsg for f in ("edits", "flags", "n_ops", "matches")) or sg["ops"].element_size() != 4):
            raise ValueError("align_join wants seg_off, one bad byte per walk and the arrays align_pairs wrote for the segments")
        si = AlignOut()
        si.capacity = sg["ops"].numel()
        for f, x in sg.items():
            setattr(si, f, x.data_ptr() if x.numel() else 0)
        args = (self.ctx, nw, _p(seg_off), _p(bad, nw), nsg, C.byref(si))
        total = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_align_join(*args, None, C.byref(total)))
        m = int(total.value)
        o, _, cut = _align_out(nw, dev, m)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_align_join(*args, C.byref(o), C.byref(total)))
        return {**cut(), "n_ops_total": m}

    @staticmethod
    def _pile_struct(planes, n_bases):
        """the s2k_pile over an (11, n_bases) int32 GPU tensor, rows in the order of PILEUP_PLANES"""
        if planes.dim() != 2 or planes.shape[0] != len(PILEUP_PLANES) or planes.shape[1] != max(n_bases, 1) or planes.element_size() != 4 or not planes.is_contiguous():
            raise ValueError("the pile is a contiguous (11, n_bases) 32-bit tensor, one row per plane of PILEUP_PLANES")
        p = Pile()
        row = [planes[i].data_ptr() for i in range(len(PILEUP_PLANES))]
        p.match, p.del_, p.ins_long = row[0], row[1], row[10]
        for c in range(4):
            p.sub[c], p.ins[c] = row[2 + c], row[6 + c]
        return p

    def walks_pileup(self, walks, step_unitig, out_off, out, overlap, query, q_begin, alignments, planes, max_shift=PILEUP_MAX_SHIFT):
        """The votes of one batch's aligned walks added to a pile (s2k_walks_pileup; the rule is in include/s2k.h).  walks, step_unitig,
        out_off, out, overlap: as walks_targets takes them; query: the batch's bases (uint8 GPU tensor); q_begin: where every walk's
        read interval starts in them (int64); alignments: a WalkAlignments (or anything with flags, ops_off, n_ops, ops) of these
        walks; planes: the (11, n_bases) int32 GPU tensor of the pile, rows in the order of PILEUP_PLANES, zeroed before the first
        batch -- it gains the votes.  -> dict of the PILEUP_STATS counters of this call."""
        import torch

        nw, dev, wargs, keep = _walk_args("walks_pileup", walks, step_unitig, out_off, out, overlap)
        query, q_begin = query.contiguous(), q_begin.contiguous()
        al = [getattr(alignments, f).contiguous() for f in ("flags", "ops_off", "n_ops", "ops")]
        if (query.element_size() != 1 or q_begin.numel() != nw or q_begin.element_size() != 8 or [x.element_size() for x in al] != [4, 8, 4, 4]
                or al[0].numel() < nw or al[2].numel() < nw or al[1].numel() != nw + 1):
            raise ValueError("walks_pileup wants the batch's bases, one 64-bit interval start per walk and the alignment arrays of these walks")
        pile = self._pile_struct(planes, out.numel())
        stats = (C.c_uint64 * PILEUP_STATS_WORDS)()
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_walks_pileup(self.ctx, *wargs, _p(query, query.numel()), query.numel(), _p(q_begin, nw), _p(al[0], nw), _p(al[1]), _p(al[2], nw),
                                              _p(al[3], al[3].numel()), al[3].numel(), int(max_shift), C.byref(pile), stats))
        return {f: int(stats[i]) for i, f in enumerate(PILEUP_STATS)}

    def pileup_consensus(self, planes, out_off, out, overlap, min_cov=3):
        """The polished bases of every unitig from a pile (s2k_pileup_consensus; the rule is in include/s2k.h).  planes: the pile, only
        read; out_off, out, overlap: the draft the pile was taken on.  Two calls: the size, then the bytes.  -> dict of GPU tensors
        out_off (int64, n_unitigs + 1), out (uint8), pos_map (int64, n_bases + 1), overlap (int32, 2 n_unitigs), the int n_bases and
        the CONSENSUS_STATS counters in stats."""
        import torch

        out_off, out, overlap = (x.contiguous() for x in (out_off, out, overlap))
        t, nb, dev = out_off.numel() - 1, out.numel(), out_off.device
        if out_off.element_size() != 8 or out.element_size() != 1 or overlap.numel() != 2 * t or overlap.element_size() != 4:
            raise ValueError("pileup_consensus wants the out_off, out and overlap of the unitig sequences")
        pile = self._pile_struct(planes, nb)
        args = (self.ctx, C.byref(pile), _p(out_off), _p(out, nb), nb, _p(overlap, t), t, int(min_cov))
        n, stats = C.c_uint64(0), (C.c_uint64 * CONSENSUS_STATS_WORDS)()
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_pileup_consensus(*args, None, None, 0, None, None, C.byref(n), stats))
        m = int(n.value)
        new_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        new_out = torch.zeros((max(m, 1) + 7) // 8 * 8, dtype=torch.uint8, device=dev)  # whole 8-byte words: walks_targets can read it
        pos_map = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
        new_ov = torch.zeros(max(2 * t, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self._check(self.lib.s2k_pileup_consensus(*args, _p(new_off), _p(new_out), m, _p(pos_map), _p(new_ov, t), C.byref(n), stats))
        return {"out_off": new_off, "out": new_out[:m], "pos_map": pos_map, "overlap": new_ov[:2 * t], "n_bases": m,
                "stats": {f: int(stats[i]) for i, f in enumerate(CONSENSUS_STATS)}}

    def partition_device(self, d_hash, n, n_parts, d_out, d_part_off):
        """keys grouped by hash prefix into n_parts ranges (the send buffers of the all-to-all)"""
        self._check(self.lib.s2k_partition_device(self.ctx, C.c_void_p(d_hash or 0), n, n_parts, C.c_void_p(d_out or 0), C.c_void_p(d_part_off)))


class KminmerCounter:
    """Accumulating k-min-mer count over batches and files (s2k_counter_*): add device-resident hashes batch by batch, finish(min_count)
    -> the solid pairs in ascending key order, equal to Engine.count_device_ex over the concatenation of everything added.  The counter
    keeps its runs in HBM (about 12 B per distinct key); close() it before its Engine."""

    def __init__(self, engine):
        self.engine = engine
        self.lib = engine.lib
        st = C.c_int(0)
        self.handle = self.lib.s2k_counter_create(engine.ctx, C.byref(st))
        if not self.handle:
            raise S2kError(st.value, self.lib.s2k_strerror(st.value).decode())
        self.last_sizes = (0, 0)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.s2k_counter_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, d_hash, n):
        """hashes d_hash[0..n) (a device pointer; any n): counted now, the buffer may be reused on return"""
        self.engine._check(self.lib.s2k_counter_add(self.handle, C.c_void_p(d_hash or 0), int(n)))

    def add_tensor(self, t):
        """a 1-D int64 / uint64 torch tensor on the engine's device (its bits are the uint64 hashes)"""
        import torch

        if t.dim() != 1 or t.element_size() != 8 or not t.is_cuda:
            raise ValueError("add_tensor wants a 1-D 64-bit tensor on the GPU")
        t = t.contiguous()
        torch.cuda.synchronize(t.device)  # the library's stream does not follow torch's
        self.add(t.data_ptr() if t.numel() else 0, t.numel())

    def sizes(self, min_count=1):
        """(n_distinct, n_kept) of everything added so far"""
        nd, nk = C.c_uint64(0), C.c_uint64(0)
        self.engine._check(self.lib.s2k_counter_finish(self.handle, int(min_count), None, None, 0, C.byref(nd), C.byref(nk)))
        self.last_sizes = (int(nd.value), int(nk.value))
        return self.last_sizes

    def finish(self, min_count=1):
        """-> (keys, counts): torch int64 / int32 tensors on the device with the uint64 keys / uint32 counts of the pairs that occur at least
        min_count times, ascending by key.  add() may go on afterwards."""
        import torch

        nd, nk = self.sizes(min_count)
        dev = torch.device("cuda", self.engine.device)
        keys = torch.empty(max(nk, 1), dtype=torch.int64, device=dev)
        counts = torch.empty(max(nk, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        if nk:
            a, b = C.c_uint64(0), C.c_uint64(0)
            self.engine._check(self.lib.s2k_counter_finish(self.handle, int(min_count), C.c_void_p(keys.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                           nk, C.byref(a), C.byref(b)))
        return keys[:nk], counts[:nk]


class CountTable:
    """Look-ups against a count table (s2k_table_*): keys (1-D 64-bit tensor on the engine's device, strictly ascending as uint64) and
    counts (32-bit tensor of the same length, or None for a membership table), as KminmerCounter.finish or Engine.count_device_ex write
    them.  The table borrows both tensors (it keeps references to them); they must not change until close().  close() it before its
    Engine."""

    def __init__(self, engine, keys, counts=None):
        import torch

        for t, size in ((keys, 8), (counts, 4)):
            if t is not None and (t.dim() != 1 or t.element_size() != size or not t.is_cuda or not t.is_contiguous()):
                raise ValueError("CountTable wants contiguous 1-D GPU tensors: keys of 64-bit, counts of 32-bit elements")
        if counts is not None and counts.numel() != keys.numel():
            raise ValueError("keys and counts differ in length")
        self.engine = engine
        self.lib = engine.lib
        self.keys, self.counts, self.n = keys, counts, keys.numel()
        torch.cuda.synchronize(keys.device)  # the library's stream does not follow torch's
        st = C.c_int(0)
        self.handle = self.lib.s2k_table_create(engine.ctx, C.c_void_p(keys.data_ptr() if self.n else 0),
                                                C.c_void_p(counts.data_ptr() if counts is not None and self.n else 0), self.n, C.byref(st))
        if not self.handle:
            raise S2kError(st.value, self.lib.s2k_strerror(st.value).decode() + " -- " + self.lib.s2k_last_error(engine.ctx).decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.s2k_table_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lookup(self, query):
        """-> int32 tensor (the uint32 counts' bits) of the count of every element of `query` (1-D 64-bit GPU tensor), 0 if absent"""
        import torch

        if query.dim() != 1 or query.element_size() != 8 or not query.is_cuda:
            raise ValueError("lookup wants a 1-D 64-bit tensor on the GPU")
        query = query.contiguous()
        out = torch.empty(max(query.numel(), 1), dtype=torch.int32, device=query.device)
        torch.cuda.synchronize(query.device)
        self.engine._check(self.lib.s2k_table_lookup(self.handle, C.c_void_p(query.data_ptr()), query.numel(), C.c_void_p(out.data_ptr())))
        return out[:query.numel()]

    def filter(self, out_tensors, n_reads, min_count=2):
        """Each read's k-min-mers whose count is at least min_count, in read order (s2k_table_filter).  out_tensors: the GPU tensors
        extract_device wrote (dict with km_off and hash; start / end / rev optional).  -> dict of GPU tensors km_off (n_reads + 1),
        hash, offset (index in the read before filtering), count, and start / end / rev where given; 'n' = kept items."""
        import torch

        dev = out_tensors["km_off"].device
        n_items = int(out_tensors["km_off"][n_reads].item()) if n_reads else 0
        cap = max(n_items, 1)
        res = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
               "offset": torch.empty(cap, dtype=torch.int32, device=dev), "count": torch.empty(cap, dtype=torch.int32, device=dev)}
        i, o = DeviceOut(), SolidOut()
        i.km_capacity = n_items
        i.km_off, i.hash = out_tensors["km_off"].data_ptr(), out_tensors["hash"].data_ptr()
        for f, dt in (("start", torch.int32), ("end", torch.int32), ("rev", torch.uint8)):
            if out_tensors.get(f) is not None:
                res[f] = torch.empty(cap, dtype=dt, device=dev)
                setattr(i, f, out_tensors[f].data_ptr())
        o.capacity = cap
        for f, t in res.items():
            setattr(o, f, t.data_ptr())
        nk = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self.engine._check(self.lib.s2k_table_filter(self.handle, n_reads, C.byref(i), int(min_count), C.byref(o), C.byref(nk)))
        n = int(nk.value)
        out = {f: (t if f == "km_off" else t[:n]) for f, t in res.items()}
        out["n"] = n
        return out

    def edges(self, out_tensors, n_reads, min_count=2):
        """The graph edges that the reads traverse (s2k_table_edges): out_tensors = the GPU tensors extract_device wrote (dict with
        km_off, hash and rev).  Node i is key i of this table, oriented node 2 * i + rev.  -> int64 tensor of the edge keys
        (u << 32 | v as uint64 bits) in emission order: each adjacency of two solid consecutive items of a read, then its twin
        ((v ^ 1) << 32 | u ^ 1) unless it is its own."""
        import torch

        dev = out_tensors["km_off"].device
        n_items = int(out_tensors["km_off"][n_reads].item()) if n_reads else 0
        cap = 2 * n_items  # at most two keys per item
        keys = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        i = DeviceOut()
        i.km_capacity = n_items
        i.km_off, i.hash, i.rev = (out_tensors[f].data_ptr() for f in ("km_off", "hash", "rev"))
        ne = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self.engine._check(self.lib.s2k_table_edges(self.handle, n_reads, C.byref(i), int(min_count), C.c_void_p(keys.data_ptr()), cap,
                                                    C.byref(ne)))
        return keys[:int(ne.value)]


    def thread(self, out_tensors, n_reads, place, n_unitigs, out, min_count=2, uni_items=None):
        """The reads' paths through a unitig decomposition of this table's keys (s2k_table_thread; the definitions are in include/s2k.h).
        out_tensors: the GPU tensors extract_device wrote (km_off, hash, rev; start / end when `out` asks for them); place: what
        Engine.unitig_node_places returned for the decomposition; out: a ThreadOut naming the arrays to fill (path_off required; all step
        arrays 0: the sizes only); uni_items: int64 GPU tensor, one entry per unitig, that gains every step's count.  -> the number of
        steps.  S2kError(7) when out.capacity is short: nothing was written to the step arrays."""
        import torch

        dev = out_tensors["km_off"].device
        if place.numel() != 4 * self.n or place.element_size() != 4 or not place.is_contiguous():
            raise ValueError("thread wants the (n_keys, 4) 32-bit place tensor of Engine.unitig_node_places")
        if uni_items is not None and (uni_items.numel() != int(n_unitigs) or uni_items.element_size() != 8 or not uni_items.is_contiguous()):
            raise ValueError("uni_items holds one 64-bit entry per unitig")
        i = DeviceOut()
        i.km_capacity = int(out_tensors["km_off"][n_reads].item()) if n_reads else 0
        for f in ("km_off", "hash", "rev", "start", "end"):
            if out_tensors.get(f) is not None:
                setattr(i, f, out_tensors[f].data_ptr())
        ns = C.c_uint64(0)
        torch.cuda.synchronize(dev)
        self.engine._check(self.lib.s2k_table_thread(self.handle, n_reads, C.byref(i), int(min_count), C.c_void_p(place.data_ptr() if self.n else 0),
                                                     self.n, C.byref(out), C.c_void_p(uni_items.data_ptr() if uni_items is not None and n_unitigs else 0),
                                                     int(n_unitigs), C.byref(ns)))
        return int(ns.value)


def _seq_in(o, n_reads):
    """the DeviceOut of one batch's extraction outputs for the sequence calls (km_off, hash, rev; mn_off, mn_j, mn_jend when present)"""
    i = DeviceOut()
    i.km_capacity = int(o["km_off"][n_reads].item()) if n_reads else 0
    i.km_off, i.hash = o["km_off"].data_ptr(), o["hash"].data_ptr()
    if o.get("rev") is not None:
        i.rev = o["rev"].data_ptr()
    if o.get("mn_off") is not None:
        i.mn_capacity = int(o["mn_off"][n_reads].item()) if n_reads else 0
        i.mn_off, i.mn_j, i.mn_jend = (o[f].data_ptr() for f in ("mn_off", "mn_j", "mn_jend"))
    return i


class NodeSequences:
    """Base-space records of a graph's nodes (include/s2k.h: s2k_table_representatives, s2k_table_node_sequences):
    per node i the bytes pool[seq_off[i] : seq_off[i] + seq_len[i]] of its representative (the occurrence with the smallest global
    item ordinal), its rev, and the two shifts; rep[i] = that ordinal.  All GPU tensors (int64 / int32 / uint8 holding the unsigned
    values)."""

    FIELDS = ("seq_off", "seq_len", "shift_fwd", "shift_rev", "rev")

    def __init__(self, rep, seq_off, seq_len, shift_fwd, shift_rev, rev, pool, n_bytes, k):
        self.rep, self.seq_off, self.seq_len, self.shift_fwd, self.shift_rev, self.rev = rep, seq_off, seq_len, shift_fwd, shift_rev, rev
        self.pool, self.n_bytes, self.k = pool, n_bytes, k

    def struct(self, pool_capacity=None):
        ns = NodeSeqs()
        for f in self.FIELDS + ("pool",):
            setattr(ns, f, getattr(self, f).data_ptr())
        ns.pool_capacity = self.n_bytes if pool_capacity is None else pool_capacity
        return ns

    def host(self):
        """-> dict of numpy arrays: seq_off uint64, seq_len / shift_fwd / shift_rev uint32, rev uint8, pool uint8, rep uint64"""
        d = {"seq_off": self.seq_off.cpu().numpy().view(np.uint64), "rev": self.rev.cpu().numpy(), "pool": self.pool[:self.n_bytes].cpu().numpy(),
             "rep": self.rep.cpu().numpy().view(np.uint64)}
        for f in ("seq_len", "shift_fwd", "shift_rev"):
            d[f] = getattr(self, f).cpu().numpy().view(np.uint32)
        return d

    def subset(self, node_map):
        """The records of the nodes a simplification kept, under their new ids: node_map is what KminmerGraph.simplify returned (per old
        node its new id, -1 for a removed one; new ids ascend with the old ones).  The record arrays are gathered, the pool is shared,
        not copied."""
        import torch

        old = torch.nonzero(node_map >= 0)[:, 0]
        return type(self)(*(getattr(self, f)[old] for f in ("rep",) + self.FIELDS), self.pool, self.n_bytes, self.k)

    def take(self, node_origin):
        """The records of the node instances of an untangled graph: node_origin is what UnitigGraph.untangle returned (per instance
        its old node).  The counterpart of subset: the record arrays are gathered to the instance ids -- a node of a duplicated unitig
        occurs once per copy -- and the pool is shared, not copied."""
        old = node_origin.long()
        return type(self)(*(getattr(self, f)[old] for f in ("rep",) + self.FIELDS), self.pool, self.n_bytes, self.k)

    @staticmethod
    def _voted(engine, table, outs, k, dev):
        """the voted ordinals of every key of `table` over the batches `outs`: keys -> counter -> vote table -> best -> ordinals"""
        import torch

        counter = KminmerCounter(engine)
        try:
            for o in outs:
                counter.add_tensor(engine.table_vote_keys(table, o, k))
            vkeys, vcounts = counter.finish(1)
        finally:
            counter.close()
        votes = CountTable(engine, vkeys, vcounts)
        try:
            best = torch.zeros(max(table.n, 1), dtype=torch.int64, device=dev)
            base = 0
            for o in outs:
                base += engine.table_vote_representatives(table, votes, o, k, base, best)
        finally:
            votes.close()
        rep = engine.vote_ordinals(best)
        return rep if table.n else torch.full((1,), -1, dtype=torch.int64, device=dev)

    @classmethod
    def build(cls, engine, table_or_graph, outs, k=None, vote=False):
        """outs: per batch the GPU tensors extract_device wrote with FLAG_WANT_MINIMIZERS (km_off, hash, rev, mn_off, mn_j, mn_jend) plus
        the batch's `bases` and `read_off`, in the order the graph was built from; table_or_graph: the CountTable of the nodes, or a
        KminmerGraph (a table over its keys lives for this call).  k (the k-min-mer order) is taken from the first read with items
        when not given; the device checks it against every read.  Three rounds over the batches: representatives, sizes, records.
        vote=True chooses every node's best-supported occurrence instead of its earliest: the batches' vote keys are
        counted (a KminmerCounter and the table over its result live for this call), every batch's items are scored against them, and
        rep holds the voted ordinals; the two record rounds are the same."""
        import torch

        own = isinstance(table_or_graph, KminmerGraph)
        table = CountTable(engine, table_or_graph.keys, table_or_graph.counts) if own else table_or_graph
        try:
            dev = torch.device("cuda", engine.device)
            n_keys = table.n
            ins, bases = [], []
            for o in outs:
                nr = o["km_off"].numel() - 1
                if o.get("mn_off") is None or o.get("bases") is None or o.get("read_off") is None:
                    raise ValueError("NodeSequences.build wants mn_off, mn_j, mn_jend, bases and read_off beside km_off, hash and rev")
                i = _seq_in(o, nr)
                if k is None and i.km_capacity:
                    n_it, n_tr = (o["km_off"][1:] - o["km_off"][:-1]), (o["mn_off"][1:] - o["mn_off"][:-1])
                    r = int(torch.nonzero(n_it)[0, 0])
                    k = int(n_tr[r]) - int(n_it[r]) + 1
                ins.append((i, nr))
                bases.append((o["bases"], o["read_off"]))
            k = 2 if k is None else int(k)
            if vote:
                rep = cls._voted(engine, table, outs, k, dev)
            else:
                rep = torch.full((max(n_keys, 1),), -1, dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                base = 0
                for i, nr in ins:
                    engine._check(engine.lib.s2k_table_representatives(table.handle, nr, C.byref(i), base, C.c_void_p(rep.data_ptr())))
                    base += i.km_capacity

            def round_(ns):
                base, used = 0, 0
                for (i, nr), (b, ro) in zip(ins, bases):
                    nb = C.c_uint64(0)
                    engine._check(engine.lib.s2k_table_node_sequences(table.handle, nr, C.byref(i), k, C.c_void_p(b.data_ptr() if b.numel() else 0),
                                                                      C.c_void_p(ro.data_ptr()), base, C.c_void_p(rep.data_ptr()),
                                                                      C.byref(ns) if ns is not None else None, used, C.byref(nb)))
                    base += i.km_capacity
                    used += int(nb.value)
                return used

            total = round_(None)
            m = max(n_keys, 1)
            res = cls(rep[:n_keys], torch.zeros(m, dtype=torch.int64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev),
                      torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev),
                      torch.zeros(m, dtype=torch.uint8, device=dev), torch.empty(max(total, 1), dtype=torch.uint8, device=dev), total, k)
            torch.cuda.synchronize(dev)
            round_(res.struct())
            for f in cls.FIELDS:
                setattr(res, f, getattr(res, f)[:n_keys])
            return res
        finally:
            if own:
                table.close()


class KminmerGraph:
    """The minimizer-space de Bruijn graph of a read set, built on the device in two passes over its extraction outputs (dicts of the
    GPU tensors extract_device wrote: km_off, hash, rev; n_reads = len(km_off) - 1): pass 1 counts the k-min-mers (KminmerCounter) and
    keeps those seen at least min_count times as the nodes; pass 2 emits every batch's edges (CountTable.edges) into a second counter,
    keeps the edges seen at least min_edge_count times and builds their adjacency (Engine.graph_adjacency).  Node i is k-min-mer
    keys[i] (count counts[i]); oriented node u = 2 * i + o; edge i goes from u = edge_keys[i] >> 32 (as uint64) to v = dst[i] and was
    seen edge_counts[i] times; the out-edges of u are row_off[u] .. row_off[u + 1].  Every edge's twin (v ^ 1, u ^ 1) is present with
    the same count."""

    def __init__(self, keys, counts, edge_keys, edge_counts, row_off, dst):
        self.keys, self.counts, self.edge_keys, self.edge_counts, self.row_off, self.dst = keys, counts, edge_keys, edge_counts, row_off, dst

    @property
    def n_nodes(self):
        return self.keys.numel()

    @property
    def n_edges(self):
        return self.edge_keys.numel()

    @classmethod
    def build(cls, engine, outs, min_count=2, min_edge_count=1):
        nodes = KminmerCounter(engine)
        try:
            for o in outs:
                n = int(o["km_off"][-1].item())
                nodes.add_tensor(o["hash"][:n])
            keys, counts = nodes.finish(min_count)
        finally:
            nodes.close()
        table = CountTable(engine, keys, counts)
        edges = KminmerCounter(engine)
        try:
            for o in outs:
                edges.add_tensor(table.edges(o, o["km_off"].numel() - 1, min_count))
            edge_keys, edge_counts = edges.finish(min_edge_count)
        finally:
            edges.close()
            table.close()
        row_off, dst = engine.graph_adjacency(edge_keys, keys.numel())
        return cls(keys, counts, edge_keys, edge_counts, row_off, dst)

    def write_gfa(self, path, sequences=None):
        """GFA 1: an S line per node (name = node index, sequence *, KC:i: its count, kh:Z: its hash in 16 hex digits) and an L line per
        twin pair, written once, for the edge whose key is not above its twin's (orientation 0 -> +, 1 -> -, overlap *, RC:i: its
        count).  With sequences (a NodeSequences of this graph) the S line carries the bases of the node's orientation 0 and LN:i:
        their number, and the L line the overlap seq_len(u) - shift(u) as <n>M."""
        keys = self.keys.cpu().numpy().view(np.uint64)
        counts = self.counts.cpu().numpy().view(np.uint32)
        ek = self.edge_keys.cpu().numpy().view(np.uint64)
        ec = self.edge_counts.cpu().numpy().view(np.uint32)
        write_gfa(path, keys, counts, ek, ec, sequences=None if sequences is None else sequences.host())

    def unitigs(self, engine):
        """Compacts the non-branching paths on the device (Engine.graph_unitigs, Engine.graph_unitig_edges) -> UnitigGraph"""
        import torch

        n = self.n_nodes
        u = engine.graph_unitigs(self.row_off, self.dst, n)
        t = u["n_unitigs"]
        csum = torch.zeros(n + 1, dtype=torch.int64, device=self.row_off.device)
        if n:  # per unitig the sum of its nodes' counts, in member order
            csum[1:] = torch.cumsum((self.counts[(u["members"] >> 1).long()].long() & 0xFFFFFFFF), 0)
        counts = csum[u["uni_off"][1:]] - csum[u["uni_off"][:-1]]
        ek, src = engine.graph_unitig_edges(self.row_off, self.dst, n, u)
        ec = self.edge_counts[src] if ek.numel() else self.edge_counts[:0]
        row_off, dst = engine.graph_adjacency(ek, t)
        ug = UnitigGraph(u["uni_off"], u["members"], u["node_unitig"], u["node_pos"], u["circular"], counts, ek, ec, row_off, dst, u["n_links"])
        ug.n_nodes = n
        return ug


    def simplify(self, engine, max_tip, max_bubble, max_rounds=16):
        """Clips tips of at most max_tip members and pops simple bubbles whose removed branch holds at most max_bubble members (the rules
        are in include/s2k.h; 0 switches one off), round by round on the device -- unitigs, Engine.graph_simplify_mask,
        Engine.graph_induced, Engine.graph_adjacency -- until a round removes nothing or max_rounds rounds have run.
        -> (graph, node_map, stats): a new KminmerGraph over the kept nodes (self is untouched); node_map, an int32 GPU tensor with the
        final id of every node of self, -1 for a removed one; stats, one dict per round (nodes and unitigs the round started from, tips,
        bubbles and unitigs it removed), the last of which removed nothing when a fixed point was reached."""
        import torch

        g = KminmerGraph(self.keys, self.counts, self.edge_keys, self.edge_counts, self.row_off, self.dst)
        node_map = torch.arange(self.n_nodes, dtype=torch.int32, device=self.keys.device)
        stats = []
        for _ in range(max_rounds):
            ug = g.unitigs(engine)
            m = engine.graph_simplify_mask(ug, max_tip, max_bubble)
            stats.append({"nodes": g.n_nodes, "unitigs": ug.n_unitigs, "tips": m["n_tips"], "bubbles": m["n_bubbles"], "removed": m["n_removed"]})
            if m["n_removed"] == 0:
                break
            ind = engine.graph_induced(g, node_unitig=ug.node_unitig, remove=m["remove"])
            row_off, dst = engine.graph_adjacency(ind["edge_keys"], ind["keys"].numel())
            g = KminmerGraph(ind["keys"], ind["counts"], ind["edge_keys"], ind["edge_counts"], row_off, dst)
            alive = torch.nonzero(node_map >= 0)[:, 0]  # new_id holds -1 for a removed node: the composition keeps it
            node_map[alive] = ind["new_id"][node_map[alive].long()]
        return g, node_map, stats


class UnitigGraph:
    """The compacted graph (KminmerGraph.unitigs; include/s2k.h: s2k_graph_unitigs): unitig t holds the oriented nodes
    members[uni_off[t] : uni_off[t + 1]] (its kept strand, in path order), counts[t] = the sum of its nodes' counts, circular[t] tells a
    cycle; node i lies in unitig node_unitig[i] at position node_pos[i].  Oriented unitig U = 2 t + s (s = 1: the twin strand); edge j
    goes from edge_keys[j] >> 32 to dst[j] and was seen edge_counts[j] times; row_off / dst are the CSR over the oriented unitigs."""

    def __init__(self, uni_off, members, node_unitig, node_pos, circular, counts, edge_keys, edge_counts, row_off, dst, n_links=0):
        self.uni_off, self.members, self.node_unitig, self.node_pos, self.circular, self.counts = uni_off, members, node_unitig, node_pos, circular, counts
        self.edge_keys, self.edge_counts, self.row_off, self.dst, self.n_links = edge_keys, edge_counts, row_off, dst, n_links

    @property
    def n_unitigs(self):
        return self.circular.numel()

    @property
    def n_edges(self):
        return self.edge_keys.numel()

    def sequences(self, engine, node_seqs):
        """The unitigs' base-space sequences stitched on the device (Engine.unitig_sequences) from a NodeSequences of the graph this one
        was compacted from -> (out_off, out): unitig t is out[out_off[t] : out_off[t + 1]] (its kept strand).  The overlap that leaves
        every oriented unitig is kept in self.overlap for write_gfa."""
        n = getattr(self, "n_nodes", self.members.numel())
        out_off, out, self.overlap = engine.unitig_sequences(self.uni_off, self.members, self.circular, n, node_seqs)
        return out_off, out

    def places(self, engine):
        """Where every node of the compacted graph lies on the oriented unitigs (Engine.unitig_node_places), computed once and kept"""
        if getattr(self, "_places", None) is None:
            self._places = engine.unitig_node_places(self.uni_off, self.members, self.node_unitig, self.node_pos, self.circular)
        return self._places

    def thread(self, engine, table, outs, n_reads, min_count=2, coverage=None):
        """One batch of reads threaded through this graph on the device (CountTable.thread) -> ReadPaths.  table: the CountTable over the
        node keys of the KminmerGraph this one was compacted from; outs: the GPU tensors extract_device wrote for the batch (km_off,
        hash, rev; start / end are carried into the steps when present); min_count: the cutoff the graph was built with; coverage: an
        int64 GPU tensor of n_unitigs zeros that gains the items every unitig carries, batch after batch.  Two calls: the sizes, then
        the arrays.
        Through a simplified graph, with no node map: sg, _, _ = graph.simplify(...); t = CountTable(engine, sg.keys, sg.counts);
        sg.unitigs(engine).thread(engine, t, outs, n_reads) -- an item whose node was removed is not in t and breaks the path like any
        non-solid item."""
        import torch

        dev = outs["km_off"].device
        place = self.places(engine)
        o = ThreadOut()
        path_off = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
        o.path_off = path_off.data_ptr()
        n = table.thread(outs, n_reads, place, self.n_unitigs, o, min_count)
        res = {f: torch.empty(max(n, 1), dtype=torch.int32, device=dev) for f in ReadPaths.STEP_FIELDS if f not in ("start", "end") or outs.get(f) is not None}
        o.capacity = n
        for f, t in res.items():
            setattr(o, f, t.data_ptr())
        table.thread(outs, n_reads, place, self.n_unitigs, o, min_count, uni_items=coverage)
        return ReadPaths(path_off, **{f: t[:n] for f, t in res.items()})

    def spans(self, engine, paths, edge_support=None):
        """The span keys of one batch's ReadPaths (Engine.paths_spans) -> (keys, (n_followed, n_off_graph)); edge_support: an int64 GPU
        tensor of n_edges zeros that gains the read support of every edge, batch after batch -- on the reads the graph was built
        from it ends equal to edge_counts."""
        keys, nf, no = engine.paths_spans(self, paths, edge_support)
        return keys, (nf, no)

    def span_table(self, engine, list_of_paths, min_count=1):
        """The span table of several batches' ReadPaths: their span keys counted by a KminmerCounter (which counts any 64-bit keys) ->
        SpanTable(keys, counts), keys strictly ascending, count(a, b) == count(tw b, tw a)."""
        ctr = KminmerCounter(engine)
        try:
            for paths in list_of_paths:
                ctr.add_tensor(self.spans(engine, paths)[0])
            return SpanTable(*ctr.finish(min_count))
        finally:
            ctr.close()

    def resolve(self, engine, span_table, min_support=2):
        """Which repeat unitigs the spans resolve (Engine.graph_resolve_mask) -> (resolved, partner, stats): a uint8 GPU tensor with one
        byte per unitig, an int32 GPU tensor with the matched out-edge of every edge that enters a resolved unitig (-1 otherwise), and
        {"candidates", "resolved"} counted in unitigs.  self.untangle(engine, resolved, partner) duplicates the resolved unitigs and
        compacts the result into contigs."""
        m = engine.graph_resolve_mask(self, span_table.keys, span_table.counts, min_support)
        return m["resolved"], m["partner"], {"candidates": m["n_candidates"], "resolved": m["n_resolved"]}

    def untangle(self, engine, resolved, partner):
        """One round of untangling on the device: every resolved unitig is duplicated once per matched pair of edges
        (Engine.graph_untangle), the untangled graph over the copies is compacted again (graph_adjacency, graph_unitigs,
        graph_unitig_edges, graph_adjacency) and its contigs are expanded back to node members (Engine.unitig_expand).  resolved and
        partner are what self.resolve returned.
        -> (contigs, node_origin, stats): contigs, a UnitigGraph whose nodes are node instances (n_nodes = their number; a node of a
        duplicated unitig has one instance per copy), counts = the summed copy counts, edge counts gathered from self's; node_origin, an
        int32 GPU tensor with the old node of every instance -- contigs.sequences(engine, node_seqs.take(node_origin)), write_gfa and
        write_fasta then work as they are; stats = {"copies", "duplicated", "contigs"}.  self is untouched.
        One round; untangle_map returns the same three and the ContigLift that carries read paths onto the contigs, so that a second
        round can be made by hand on the lifted paths (contigs.span_table, resolve, untangle_map, lift).  There is no driver that loops."""
        return self.untangle_map(engine, resolved, partner)[:3]

    def untangle_map(self, engine, resolved, partner):
        """untangle, and the map of the old graph onto the contigs -> (contigs, node_origin, stats, lift): the first three are exactly
        what untangle returns; lift is a ContigLift: lift.lift(engine, paths) carries the ReadPaths threaded through self (plain or
        bridged) onto the contigs (Engine.unitig_copy_places, Engine.paths_lift), which a count table keyed by hash cannot do: a
        duplicated k-min-mer has two instances, and only the edges a read used tell them apart."""
        import torch

        u = engine.graph_untangle(self, resolved, partner)
        tc, dev = u["n_copies"], self.row_off.device
        ec = self.edge_counts[u["src_edge"]] if self.n_edges else self.edge_counts[:0]
        row_off, dst = engine.graph_adjacency(u["keys"], tc)
        o = engine.graph_unitigs(row_off, dst, tc)
        ek, src = engine.graph_unitig_edges(row_off, dst, tc, o)
        ec = ec[src] if ek.numel() else ec[:0]
        c_row_off, c_dst = engine.graph_adjacency(ek, o["n_unitigs"])
        x = engine.unitig_expand(o, u["origin"], self.uni_off, self.members, self.circular)
        csum = torch.zeros(tc + 1, dtype=torch.int64, device=dev)
        if tc:  # per contig the sum of its copies' counts, in member order
            csum[1:] = torch.cumsum(u["copy_count"][(o["members"] >> 1).long()], 0)
        counts = csum[o["uni_off"][1:]] - csum[o["uni_off"][:-1]]
        contigs = UnitigGraph(x["uni_off"], x["members"], x["node_unitig"], x["node_pos"], x["circular"], counts, ek, ec, c_row_off, c_dst, o["n_links"])
        contigs.n_nodes = x["n_members"]
        place = engine.unitig_copy_places(o, u["origin"], self.uni_off, self.circular)
        lift = ContigLift(self, resolved, partner, u["copy_off"], place, tc, o["n_unitigs"])
        return contigs, x["node_origin"], {"copies": tc, "duplicated": u["n_duplicated"], "contigs": o["n_unitigs"]}, lift

    def bridge(self, engine, paths, max_gap=16, max_slip=2, origin=False):
        """One batch's ReadPaths with the gaps that read errors cut into them bridged along this graph (Engine.paths_bridge;
        include/s2k.h: s2k_paths_bridge) -> (ReadPaths, stats).  Two consecutive steps of a read are joined when they lie on one unitig
        (merged into one step), or on two unitigs that an edge joins (the first extended to its unitig's end, the second back to position
        0 and marked STEP_LINKED), with at most max_gap items missing in the read and at most max_gap positions on the graph, the two
        differing by at most max_slip.  In the returned paths count is the positions a step covers, the gaps included, and the new
        attribute matched is the k-min-mers really found; they work in spans, span_table, walks, write_paths and write_gaf as they are
        (a walk's items then counts positions).  stats = {"steps_in", "steps_out", "merged", "bridged"}.
        The defaults 16 and 2 come from the repeat fixture of the tests at l = 12, k = 5 with 1 % substitutions (one substitution
        removes up to k consecutive k-min-mers); they are not tuned on real data.  Not bridged: a wholly missing unitig between two
        steps, and anything on a circular unitig; a gap is judged in items, not in bases.
        origin=True asks Engine.paths_bridge for join and attaches the attribute origin, a PathOrigin, to the returned paths: the
        source paths and where every source step went, which is what align_segmented needs to find the anchors of the bridged walks."""
        import torch

        b = engine.paths_bridge(self, paths, max_gap, max_slip, join=origin)
        stats = {"steps_in": paths.n_steps, "steps_out": b["n_steps"], "merged": b["n_merged"], "bridged": b["n_bridged"]}
        out = ReadPaths(b["path_off"], **{f: b[f] for f in ReadPaths.STEP_FIELDS + ("matched",) if f in b})
        if origin:  # an output step begins at every source step that is not merged into the one before it
            out.origin = PathOrigin(paths, torch.cumsum(b["join"].ne(1), 0, dtype=torch.int64) - 1, paths.pos)
        return out, stats

    def member_offsets(self, engine, node_seqs):
        """Where every member's piece starts in the unitigs' bases (Engine.unitig_member_offsets) -> (member_off, out_off, overlap,
        n_bases), computed once per NodeSequences and kept"""
        if getattr(self, "_member_offsets", None) is None or self._member_offsets[0] is not node_seqs:
            n = getattr(self, "n_nodes", self.members.numel())
            self._member_offsets = (node_seqs, engine.unitig_member_offsets(self.uni_off, self.members, self.circular, n, node_seqs))
        return self._member_offsets[1]

    def walks(self, engine, paths, node_seqs):
        """One batch's ReadPaths joined into walks along this graph's edges, with base coordinates on the stitched path
        (Engine.paths_walks) -> ReadWalks.  node_seqs: the NodeSequences of this graph's nodes -- of a simplified graph its subset, of
        the contigs that untangle returned node_seqs.take(node_origin).  ReadWalks.write_gaf writes them as GAF."""
        w = engine.paths_walks(self, paths, self.member_offsets(engine, node_seqs), node_seqs.seq_len)
        return ReadWalks(paths, **w)

    def align(self, engine, walks, bases, read_off, sequences, max_edits=ALIGN_MAX_EDITS):
        """Every walk's read bases aligned to its path interval on the device (Engine.walks_targets, Engine.align_pairs;
        include/s2k.h) -> WalkAlignments.  walks: the ReadWalks self.walks returned (its paths must carry start and end); bases,
        read_off: the batch's bases (uint8) and read offsets (int64) on the GPU; sequences: the pair self.sequences returned.  The
        alignment is global between read[qstart, qend) and the path's bases [path_start, path_end): it finds no better walk and moves
        no endpoint.  A walk whose path walks_targets called bad gets ALIGN_BAD_PATH and is not aligned; one whose distance exceeds
        max_edits gets ALIGN_OVER.  It works as it is on simplified graphs and on the contigs of untangle_map with lifted paths."""
        import torch

        if walks.qstart is None or walks.qend is None:
            raise ValueError("align wants walks whose paths carry start and end (extract with start / end kept)")
        if getattr(self, "overlap", None) is None:
            raise ValueError("align wants the pair that self.sequences(engine, node_seqs) returned")
        t = engine.walks_targets(walks, walks.paths.unitig, sequences[0], sequences[1], self.overlap)
        nw = walks.first_step.numel()
        qb, qe = walk_query_intervals(walks, read_off)
        bad = t["bad"].bool()
        qe = torch.where(bad, qb, qe)  # a bad walk is an empty pair: nothing is read for it
        a = engine.align_pairs(bases, t["tgt"], qb, qe, t["tgt_off"][:-1].contiguous(), t["tgt_off"][1:].contiguous(), max_edits)
        flags = torch.where(bad, torch.full_like(a["flags"], ALIGN_BAD_PATH), a["flags"]) if nw else a["flags"]
        zero = lambda x: torch.where(bad, torch.zeros_like(x), x) if nw else x  # noqa: E731
        return WalkAlignments(a["edits"], zero(a["matches"]), zero(a["n_ops"]), a["ops_off"], a["ops"], flags)

    def align_segmented(self, engine, walks, bases, read_off, sequences, node_seqs, outs, source=None, seg_len=SEGMENT_LEN, max_edits=ALIGN_MAX_EDITS):
        """align for long, noisy reads: every walk is cut at anchor k-min-mers into pieces of about seg_len query bases, the pieces are
        aligned by Engine.align_pairs and their CIGARs joined (Engine.walks_targets, Engine.walks_segments, Engine.align_pairs,
        Engine.align_join; include/s2k.h) -> WalkAlignments, as align returns it, with the extra attribute segments: a dict of
        n_segments, the SEGMENT_STATS counters and n_over_segments.  A walk is over only when one of its PIECES passes max_edits.
        walks, bases, read_off, sequences: as for align; node_seqs: the NodeSequences self.walks took; outs: the batch's extraction
        (km_off, start); source: a PathOrigin, the paths the reads were threaded into and where every step of them went -- None takes
        walks.paths.origin where UnitigGraph.bridge(origin=True) left one, and otherwise the walks' own paths with the identity map.
        The joined alignment is a valid global alignment of the walk; it is optimal between its cuts, not over the whole walk.  Walks
        on paths that ContigLift.lift returned have no map yet (include/s2k.h: Not done): use align for them."""
        if walks.qstart is None or walks.qend is None:
            raise ValueError("align_segmented wants walks whose paths carry start and end (extract with start / end kept)")
        if getattr(self, "overlap", None) is None:
            raise ValueError("align_segmented wants the pair that self.sequences(engine, node_seqs) returned")
        src = source or walks.paths.origin or PathOrigin(walks.paths)
        t = engine.walks_targets(walks, walks.paths.unitig, sequences[0], sequences[1], self.overlap)
        qb, _ = walk_query_intervals(walks, read_off)
        sg = engine.walks_segments(self, walks, self.member_offsets(engine, node_seqs), node_seqs.seq_len, qb, t["tgt_off"], t["bad"], src.paths, outs,
                                   src.src_step, src.src_pos, seg_len)
        a = engine.align_pairs(bases, t["tgt"], sg["q_begin"], sg["q_end"], sg["t_begin"], sg["t_end"], max_edits)
        j = engine.align_join(sg["seg_off"], t["bad"], a)
        al = WalkAlignments(j["edits"], j["matches"], j["n_ops"], j["ops_off"], j["ops"], j["flags"])
        al.segments = dict(sg["stats"], n_segments=sg["n_segments"], n_over_segments=int((a["flags"] & ALIGN_OVER).ne(0).sum()))
        return al

    def pileup(self, engine, sequences):
        """An empty pile over this graph's draft bases -> Pileup.  sequences: the pair self.sequences returned.  Pileup.add takes the
        walks and alignments of one batch after self.align; Pileup.consensus gives the polished bases.  It works as it is on
        simplified graphs and on the contigs of untangle_map with lifted paths."""
        if getattr(self, "overlap", None) is None:
            raise ValueError("pileup wants the pair that self.sequences(engine, node_seqs) returned")
        return Pileup(self, sequences)

    def write_gfa(self, path, members=False, sequences=None):
        """GFA 1: an S line per unitig (name = its index, sequence *, LN:i: its number of members, KC:i: the summed count; with
        members=True an nd:Z: tag that lists node index and orientation in path order) and an L line per twin pair of edges, by the rule
        of KminmerGraph.write_gfa (RC:i: the edge count).  With sequences (the pair self.sequences returned) the S line carries the
        bases, LN:i: their number and nm:i: the number of members, and the L line the overlap as <n>M."""
        seq = None
        if sequences is not None:
            if getattr(self, "overlap", None) is None:
                raise ValueError("write_gfa(sequences=...) wants the pair that self.sequences(engine, node_seqs) returned")
            seq = (sequences[0].cpu().numpy().view(np.uint64), sequences[1].cpu().numpy(), self.overlap.cpu().numpy().view(np.uint32))
        write_unitig_gfa(path, self.uni_off.cpu().numpy().view(np.uint64), self.members.cpu().numpy().view(np.uint32), self.counts.cpu().numpy(),
                         self.edge_keys.cpu().numpy().view(np.uint64), self.edge_counts.cpu().numpy().view(np.uint32), members=members, sequences=seq)


class PathOrigin:
    """Where the steps of a batch's ReadPaths came from (UnitigGraph.bridge(origin=True); include/s2k.h: s2k_walks_segments): paths, the
    source ReadPaths that UnitigGraph.thread wrote; src_step (int64 per source step, NO_STEP = -1 for none; None: the identity), the
    step it went into; src_pos (int32; None: paths.pos), the position of its first item on that step's oriented unitig."""

    def __init__(self, paths, src_step=None, src_pos=None):
        self.paths, self.src_step, self.src_pos = paths, src_step, src_pos


class ContigLift:
    """The map of a UnitigGraph onto the contigs of one round of untangling (UnitigGraph.untangle_map): graph, the old graph; resolved
    and partner, what was untangled; copy_off (int64, n_unitigs + 1), the copies of every unitig; copy_place (int32, (n_copies, 4)), the
    NodePlace record of every copy on the oriented contigs; n_copies, n_contigs."""

    def __init__(self, graph, resolved, partner, copy_off, copy_place, n_copies, n_contigs):
        self.graph, self.resolved, self.partner, self.copy_off, self.copy_place = graph, resolved, partner, copy_off, copy_place
        self.n_copies, self.n_contigs = n_copies, n_contigs

    def lift(self, engine, paths, contig_items=None):
        """One batch's ReadPaths on the old graph carried onto the contigs (Engine.paths_lift; include/s2k.h: s2k_paths_lift) ->
        (ReadPaths, stats).  A step on a duplicated unitig goes to the copy whose matched pair of edges the read used; steps that the
        compaction put side by side on one contig become one step; a step on a duplicated unitig that the read neither enters nor
        leaves over an edge cannot be placed and is dropped.  The returned paths carry matched (the k-min-mers really found: the
        paths' own matched summed, or their counts) and go into contigs.spans, contigs.walks(engine, lifted,
        node_seqs.take(node_origin)), write_gaf and write_paths as they are.  contig_items: an int64 GPU tensor of n_contigs zeros that
        gains the items every contig carries, batch after batch.  stats = {"steps_in", "steps_out", "merged", "dropped", "conflicts"};
        conflicts counts the steps whose read left a duplicated unitig by another edge than the one matched to the edge it came by."""
        b = engine.paths_lift(self.graph, paths, self.resolved, self.partner, self.copy_off, self.copy_place, self.n_contigs, contig_items=contig_items)
        stats = {"steps_in": paths.n_steps, "steps_out": b["n_steps"], "merged": b["n_merged"], "dropped": b["n_dropped"], "conflicts": b["n_conflicts"]}
        return ReadPaths(b["path_off"], **{f: b[f] for f in ReadPaths.STEP_FIELDS + ("matched",) if f in b}), stats


class ReadPaths:
    """The paths of one batch of reads (UnitigGraph.thread; include/s2k.h: s2k_table_thread): the steps of read r are path_off[r] ..
    path_off[r + 1]; step s runs along the oriented unitig unitig[s] (2 t + strand) from position pos[s] over count[s] items, its first
    item is item[s] of the read, flags[s] & STEP_LINKED tells that the read entered it over a graph adjacency (not a gap), start[s] /
    end[s] (None when the extraction kept none) are the read's bases it covers.  matched[s] (None but on the paths
    UnitigGraph.bridge and ContigLift.lift returned) is the k-min-mers really found in a step whose count, after bridging, is the positions it covers.
    GPU tensors: path_off int64, the rest int32 holding the uint32 values."""

    STEP_FIELDS = ("unitig", "pos", "count", "item", "flags", "start", "end")

    def __init__(self, path_off, unitig, pos, count, item, flags, start=None, end=None, matched=None):
        self.path_off, self.unitig, self.pos, self.count, self.item, self.flags, self.start, self.end = path_off, unitig, pos, count, item, flags, start, end
        self.matched = matched
        self.origin = None  # a PathOrigin on the paths UnitigGraph.bridge(origin=True) returned

    @property
    def n_steps(self):
        return self.unitig.numel()

    def host(self):
        """-> dict of numpy arrays: path_off uint64, the step arrays uint32 (start / end / matched only when present)"""
        d = {"path_off": self.path_off.cpu().numpy().view(np.uint64)}
        for f in self.STEP_FIELDS + ("matched",):
            if getattr(self, f) is not None:
                d[f] = getattr(self, f).cpu().numpy().view(np.uint32)
        return d

    def write_paths(self, path, first_read=0):
        """One line per read (write_read_paths): read_index <tab> n_steps <tab> path; first_read = the index of the batch's first read"""
        h = self.host()
        write_read_paths(path, h["path_off"], h["unitig"], h["pos"], h["count"], h["flags"], first_read=first_read)


def write_read_paths(path, path_off, unitig, pos, count, flags, first_read=0):
    """ReadPaths.write_paths on host arrays.  One line per read: first_read + r, its number of steps, and its steps concatenated, each
    >t (oriented unitig 2 t) or <t (2 t + 1) followed by :pos+count; a step the read did not enter over a graph adjacency (no
    STEP_LINKED) is preceded by *, except the read's first.  A read without steps gets an empty path."""
    off = np.asarray(path_off).astype(np.int64).tolist()
    u, p, c, f = (np.asarray(x).astype(np.int64).tolist() for x in (unitig, pos, count, flags))
    with open(path, "w") as out:
        for r in range(len(off) - 1):
            a, b = off[r], off[r + 1]
            steps = "".join("%s%s%d:%d+%d" % ("" if s == a or f[s] & STEP_LINKED else "*", "<" if u[s] & 1 else ">", u[s] >> 1, p[s], c[s])
                            for s in range(a, b))
            out.write("%d\t%d\t%s\n" % (first_read + r, b - a, steps))


class ReadWalks:
    """The walks of one batch of reads (UnitigGraph.walks; include/s2k.h: s2k_paths_walks): the walks of read r are walk_off[r] ..
    walk_off[r + 1]; walk w holds the steps first_step[w] .. first_step[w] + n_steps[w] of `paths`, each after the first entered over
    a graph edge; it covers items[w] k-min-mers, the read's bases qstart[w] .. qend[w] (None when the paths carry no start / end) and
    the bases path_start[w] .. path_end[w] of its stitched path of path_len[w] bases; flags[w] & WALK_CIRCULAR tells a walk on a
    circular unitig.  edge[s] = the edge step s follows, -1 for none.  GPU tensors: int64, and int32 holding the uint32 values."""

    FIELDS = ("first_step", "n_steps", "items", "qstart", "qend", "path_len", "path_start", "path_end", "flags")

    def __init__(self, paths, walk_off, first_step, n_steps, items, path_len, path_start, path_end, flags, qstart=None, qend=None, edge=None, n_walks=0,
                 n_followed=0, n_off_graph=0):
        self.paths, self.walk_off, self.first_step, self.n_steps, self.items = paths, walk_off, first_step, n_steps, items
        self.path_len, self.path_start, self.path_end, self.flags, self.qstart, self.qend, self.edge = path_len, path_start, path_end, flags, qstart, qend, edge
        self.n_walks, self.n_followed, self.n_off_graph = n_walks, n_followed, n_off_graph

    def host(self):
        """-> dict of numpy arrays: walk_off and the 64-bit records uint64, the 32-bit ones uint32 (qstart / qend / edge when present)"""
        d = {"walk_off": self.walk_off.cpu().numpy().view(np.uint64)}
        for f in self.FIELDS + ("edge",):
            x = getattr(self, f)
            if x is not None:
                d[f] = x.cpu().numpy().view(np.uint64 if x.element_size() == 8 else np.uint32)
        return d

    def write_gaf(self, path, graph=None, names=None, read_lengths=None, first_read=0, alignments=None):
        """One GAF line per walk (write_gaf_walks).  graph: the UnitigGraph the walks were taken on (only its naming is used: unitig t
        is segment t, as in write_unitig_gfa; may be None); names: one name per read (the index first_read + r when None);
        read_lengths: one length per read (* when None); alignments: the WalkAlignments UnitigGraph.align returned for these walks
        (residue matches, block length, NM:i: and cg:Z: on every walk it aligned)."""
        if self.qstart is None or self.qend is None:
            raise ValueError("write_gaf wants paths that carry start and end (extract with start / end kept)")
        h = self.host()
        write_gaf_walks(path, h, self.paths.unitig.cpu().numpy().view(np.uint32), names=names, read_lengths=read_lengths, first_read=first_read,
                        alignments=None if alignments is None else alignments.host())


def write_gaf_walks(path, walks, step_unitig, names=None, read_lengths=None, first_read=0, alignments=None):
    """ReadWalks.write_gaf on host arrays: walks = the dict ReadWalks.host() returns, step_unitig = the paths' oriented unitig per
    step.  One line per walk, tab-separated: read name, read length (*: unknown), qstart, qend, +, the path as >t (oriented unitig 2
    t) or <t (2 t + 1) per step with the unitig names of write_unitig_gfa, path_len, path_start, path_end, items (the matches column:
    k-min-mers, not bases), max(qend - qstart, path_end - path_start) (the block length), 255, km:i:<items>, ns:i:<n_steps>.  On a
    circular unitig path_end may pass path_len (include/s2k.h).  alignments: the dict WalkAlignments.host() returns (edits, matches,
    n_ops, ops_off, ops, flags per walk); a walk whose flags are 0 then has the residue matches in the matches column, the sum of its
    run lengths as the block length, and NM:i:<edits> and cg:Z:<runs with = X I D> after the two tags; a flagged walk keeps the line
    it has without alignments."""
    off = np.asarray(walks["walk_off"]).astype(np.int64).tolist()
    w = {f: np.asarray(walks[f]).astype(np.int64).tolist() for f in ReadWalks.FIELDS}
    u = np.asarray(step_unitig).astype(np.int64).tolist()
    al = alignments
    if al is not None:
        block = al["block_len"] if "block_len" in al else alignment_block_len(al["ops_off"], al["n_ops"], al["ops"])
    with open(path, "w") as out:
        for r in range(len(off) - 1):
            name = str(first_read + r) if names is None else names[r]
            ln = "*" if read_lengths is None else "%d" % int(read_lengths[r])
            for i in range(off[r], off[r + 1]):
                a = w["first_step"][i]
                steps = "".join("%s%d" % ("<" if x & 1 else ">", x >> 1) for x in u[a: a + w["n_steps"][i]])
                qs, qe, ps, pe = w["qstart"][i], w["qend"][i], w["path_start"][i], w["path_end"][i]
                matches, blen, tags = w["items"][i], max(qe - qs, pe - ps), ""
                if al is not None and int(al["flags"][i]) == 0:
                    o = int(al["ops_off"][i])
                    matches, blen = int(al["matches"][i]), int(block[i])
                    tags = "\tNM:i:%d\tcg:Z:%s" % (int(al["edits"][i]), cigar_string(al["ops"][o: o + int(al["n_ops"][i])]))
                out.write("%s\t%s\t%d\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t255\tkm:i:%d\tns:i:%d%s\n" % (
                    name, ln, qs, qe, steps, w["path_len"][i], ps, pe, matches, blen, w["items"][i], w["n_steps"][i], tags))


def walk_query_intervals(walks, read_off):
    """-> (begin, end): int64 GPU tensors with every walk's read interval [read_off[r] + qstart, read_off[r] + qend) in the batch's
    bases, the read r of a walk from walk_off"""
    import torch

    wo, dev = walks.walk_off.to(torch.int64), read_off.device
    read = torch.repeat_interleave(torch.arange(wo.numel() - 1, device=dev), wo[1:] - wo[:-1])
    base = read_off.to(torch.int64)[read]
    return base + (walks.qstart.to(torch.int64) & 0xFFFFFFFF), base + (walks.qend.to(torch.int64) & 0xFFFFFFFF)


class WalkAlignments:
    """The alignments of one batch's walks (UnitigGraph.align; include/s2k.h: s2k_align_pairs), one entry per walk: edits, matches (the
    bases under =), n_ops, flags (ALIGN_OVER: the distance exceeds max_edits; ALIGN_BAD_PATH: the walk's path could not be stitched),
    ops_off (n_walks + 1) and ops: the CIGAR of walk w is ops[ops_off[w] : ops_off[w] + n_ops[w]], each len << 4 | op with the BAM
    codes CIGAR_I, CIGAR_D, CIGAR_EQ, CIGAR_X.  A flagged walk has no run.  GPU tensors: ops_off int64, the rest int32 holding the
    uint32 values."""

    FIELDS = ("edits", "matches", "n_ops", "ops_off", "ops", "flags")

    def __init__(self, edits, matches, n_ops, ops_off, ops, flags):
        self.edits, self.matches, self.n_ops, self.ops_off, self.ops, self.flags = edits, matches, n_ops, ops_off, ops, flags
        self._host = None

    @property
    def n_over(self):
        return int((self.flags & ALIGN_OVER).ne(0).sum())

    @property
    def n_bad(self):
        return int((self.flags & ALIGN_BAD_PATH).ne(0).sum())

    def host(self):
        """-> dict of numpy arrays: ops_off uint64, the rest uint32; block_len (uint64 per walk) = the sum of the run lengths"""
        if self._host is None:
            d = {f: getattr(self, f).cpu().numpy().view(np.uint64 if f == "ops_off" else np.uint32) for f in self.FIELDS}
            d["block_len"] = alignment_block_len(d["ops_off"], d["n_ops"], d["ops"])
            self._host = d
        return self._host

    @property
    def block_len(self):
        return self.host()["block_len"]

    def cigar(self, w):
        """the CIGAR of walk w with = X I D, "" for a flagged walk"""
        h = self.host()
        return cigar_string(h["ops"][int(h["ops_off"][w]): int(h["ops_off"][w]) + int(h["n_ops"][w])])


def cigar_string(ops):
    """runs len << 4 | op -> text with = X I D"""
    return "".join("%d%s" % (int(x) >> 4, CIGAR_CHARS[int(x) & 15]) for x in ops)


def alignment_block_len(ops_off, n_ops, ops):
    """per alignment the sum of its run lengths (uint64)"""
    ln = np.concatenate([[0], np.cumsum(np.asarray(ops).astype(np.uint64) >> np.uint64(4))]).astype(np.uint64)
    a = np.asarray(ops_off).astype(np.int64)[:-1]
    return ln[a + np.asarray(n_ops).astype(np.int64)] - ln[a]


class Pileup:
    """The votes of aligned read walks on the bases of a UnitigGraph's draft (UnitigGraph.pileup; include/s2k.h: s2k_walks_pileup,
    s2k_pileup_consensus): planes, an (11, n_bases) int32 GPU tensor with one row per plane of PILEUP_PLANES (match, del, sub0..3,
    ins0..3, ins_long), indexed by position in the draft `sequences` = (out_off, out); graph, the UnitigGraph.  add() once per batch,
    from file to file; consensus() whenever wanted, the pile is only read."""

    def __init__(self, graph, sequences):
        import torch

        self.graph, self.sequences = graph, sequences
        self.planes = torch.zeros((len(PILEUP_PLANES), max(sequences[1].numel(), 1)), dtype=torch.int32, device=sequences[1].device)
        self.stats = {f: 0 for f in PILEUP_STATS}

    def add(self, engine, walks, alignments, bases, read_off, max_shift=PILEUP_MAX_SHIFT):
        """One batch's votes: walks, the ReadWalks graph.walks returned; alignments, the WalkAlignments graph.align returned for them;
        bases, read_off: the batch's bases and read offsets on the GPU.  -> the PILEUP_STATS counters of this batch (self.stats sums
        them)."""
        qb, _ = walk_query_intervals(walks, read_off)
        st = engine.walks_pileup(walks, walks.paths.unitig, self.sequences[0], self.sequences[1], self.graph.overlap, bases, qb, alignments, self.planes,
                                 max_shift)
        for f, v in st.items():
            self.stats[f] += v
        return st

    def depth(self):
        """match + the four sub + del per position: the walks whose alignment covers it (int64 GPU tensor)"""
        import torch

        n = self.sequences[1].numel()
        return (self.planes[:6, :n].to(torch.int64) & 0xFFFFFFFF).sum(0)

    def host(self):
        """-> dict of numpy uint32 arrays, one per plane of PILEUP_PLANES"""
        n = self.sequences[1].numel()
        h = self.planes[:, :n].cpu().numpy().view(np.uint32)
        return {f: h[i] for i, f in enumerate(PILEUP_PLANES)}

    def consensus(self, engine, min_cov=3):
        """The polished bases (Engine.pileup_consensus) -> PolishedSequences"""
        import copy

        c = engine.pileup_consensus(self.planes, self.sequences[0], self.sequences[1], self.graph.overlap, min_cov)
        g = copy.copy(self.graph)
        g.overlap = c["overlap"]
        g._member_offsets = None  # member offsets are not remapped onto the polished coordinates
        return PolishedSequences((c["out_off"], c["out"]), c["overlap"], c["pos_map"], c["stats"], g)


class PolishedSequences:
    """What Pileup.consensus returns: sequences, the (out_off, out) pair that write_fasta and write_gfa(sequences=) take; overlap, the
    overlap that leaves every oriented unitig in the new coordinates; pos_map (int64, n_bases + 1), the new position of every draft
    position (an inserted letter belongs to the position it precedes); stats, the CONSENSUS_STATS counters; graph, a shallow copy of
    the unitig graph that carries the new overlaps: graph.write_gfa(path, sequences=polished.sequences)."""

    def __init__(self, sequences, overlap, pos_map, stats, graph):
        self.sequences, self.overlap, self.pos_map, self.stats, self.graph = sequences, overlap, pos_map, stats, graph


class SpanTable:
    """The counted span keys of a read set over a UnitigGraph (UnitigGraph.span_table): keys[i] = a << 32 | b (as uint64, strictly
    ascending; a and b index the graph's edges: a enters the spanned unitig, b leaves it) was seen counts[i] times.  GPU tensors."""

    def __init__(self, keys, counts):
        self.keys, self.counts = keys, counts

    @property
    def n_spans(self):
        return self.keys.numel()

    def write(self, path, edge_keys):
        write_spans(path, self.keys.cpu().numpy().view(np.uint64), self.counts.cpu().numpy().view(np.uint32),
                    (edge_keys.cpu().numpy() if hasattr(edge_keys, "cpu") else np.asarray(edge_keys)).view(np.uint64))


def write_spans(path, span_keys, span_counts, edge_keys):
    """A span table on host arrays, one line per twin pair of spans (the one with a < tw(b)): the three oriented unitigs A, V, C of
    the spanning read, each >t (oriented unitig 2 t) or <t (2 t + 1) as in write_read_paths, and the count, separated by tabs.
    edge_keys: the unitig edge keys U << 32 | V, strictly ascending, that the span keys' halves index."""
    ek = np.asarray(edge_keys, dtype=np.uint64)
    sk, sc = np.asarray(span_keys, dtype=np.uint64), np.asarray(span_counts, dtype=np.uint32)
    src, dst = (ek >> np.uint64(32)).astype(np.int64), (ek & np.uint64(0xFFFFFFFF)).astype(np.int64)
    a, b = (sk >> np.uint64(32)).astype(np.int64), (sk & np.uint64(0xFFFFFFFF)).astype(np.int64)
    twin_of_b = np.searchsorted(ek, ((dst[b] ^ 1).astype(np.uint64) << np.uint64(32)) | (src[b] ^ 1).astype(np.uint64))
    name = lambda u: "%s%d" % ("<" if u & 1 else ">", u >> 1)  # noqa: E731
    with open(path, "w") as f:
        for i in np.nonzero(a < twin_of_b)[0].tolist():
            f.write("%s\t%s\t%s\t%d\n" % (name(int(src[a[i]])), name(int(dst[a[i]])), name(int(dst[b[i]])), int(sc[i])))


_REVCOMP = np.arange(256, dtype=np.uint8)
_REVCOMP[list(b"ACGTacgt")] = list(b"TGCAtgca")


def revcomp(seq):
    """reversed, ACGTacgt -> TGCAtgca, every other byte as it is (the revcomp of include/s2k.h) -> bytes"""
    return _REVCOMP[_as_u8(seq)][::-1].tobytes()


def write_fasta(path, out_off, out):
    """One record per unitig: >index, then its bases on one line (out_off / out: what UnitigGraph.sequences returned, tensors or host
    arrays)"""
    off = np.asarray(out_off.cpu() if hasattr(out_off, "cpu") else out_off).astype(np.int64).tolist()
    text = np.asarray(out.cpu() if hasattr(out, "cpu") else out, dtype=np.uint8).tobytes()
    with open(path, "wb") as f:
        for t in range(len(off) - 1):
            f.write(b">%d\n%s\n" % (t, text[off[t]:off[t + 1]]))


def write_unitig_gfa(path, uni_off, members_arr, counts, edge_keys, edge_counts, members=False, sequences=None):
    """UnitigGraph.write_gfa on host arrays; sequences = (out_off, out, overlap): the offsets and bases of the unitigs and the overlap
    that leaves each oriented unitig"""
    uo, mem = np.asarray(uni_off, dtype=np.uint64).tolist(), np.asarray(members_arr, dtype=np.uint32).tolist()
    ek, ec = np.asarray(edge_keys, dtype=np.uint64), np.asarray(edge_counts, dtype=np.uint32)
    u, v = ek >> np.uint64(32), ek & np.uint64(0xFFFFFFFF)
    twin = ((v ^ np.uint64(1)) << np.uint64(32)) | (u ^ np.uint64(1))
    sel = ek <= twin
    sign = "+-"
    if sequences is not None:
        so, text = np.asarray(sequences[0]).astype(np.int64).tolist(), np.asarray(sequences[1], dtype=np.uint8).tobytes()
        ov = np.asarray(sequences[2]).astype(np.int64).tolist()
    with open(path, "w") as f:
        f.write("H\tVN:Z:1.0\n")
        for t, c in enumerate(np.asarray(counts).tolist()):
            a, b = uo[t], uo[t + 1]
            nd = "\tnd:Z:" + ",".join("%d%s" % (x >> 1, sign[x & 1]) for x in mem[a:b]) if members else ""
            if sequences is None:
                f.write("S\t%d\t*\tLN:i:%d\tKC:i:%d%s\n" % (t, b - a, c, nd))
            else:
                f.write("S\t%d\t%s\tLN:i:%d\tnm:i:%d\tKC:i:%d%s\n" % (t, text[so[t]:so[t + 1]].decode("latin-1"), so[t + 1] - so[t], b - a, c, nd))
        f.writelines("L\t%d\t%s\t%d\t%s\t%s\tRC:i:%d\n" % (a >> 1, sign[a & 1], b >> 1, sign[b & 1], "*" if sequences is None else "%dM" % ov[a], c)
                     for a, b, c in zip(u[sel].tolist(), v[sel].tolist(), ec[sel].tolist()))


def write_gfa(path, keys, counts, edge_keys, edge_counts, sequences=None):
    """KminmerGraph.write_gfa on host arrays: node keys / counts (uint64 / uint32) and edge keys / counts (uint64 / uint32); sequences =
    the dict NodeSequences.host() returns (seq_off, seq_len, shift_fwd, shift_rev, rev, pool)."""
    keys, counts = np.asarray(keys, dtype=np.uint64), np.asarray(counts, dtype=np.uint32)
    ek, ec = np.asarray(edge_keys, dtype=np.uint64), np.asarray(edge_counts, dtype=np.uint32)
    u, v = ek >> np.uint64(32), ek & np.uint64(0xFFFFFFFF)
    twin = ((v ^ np.uint64(1)) << np.uint64(32)) | (u ^ np.uint64(1))
    sel = ek <= twin
    sign = np.array(["+", "-"])
    with open(path, "w") as f:
        f.write("H\tVN:Z:1.0\n")
        su, sv = u[sel], v[sel]
        if sequences is None:
            f.writelines("S\t%d\t*\tKC:i:%d\tkh:Z:%016x\n" % (i, c, h) for i, (h, c) in enumerate(zip(keys.tolist(), counts.tolist())))
            f.writelines("L\t%d\t%s\t%d\t%s\t*\tRC:i:%d\n" % (a >> 1, sign[a & 1], b >> 1, sign[b & 1], c)
                         for a, b, c in zip(su.tolist(), sv.tolist(), ec[sel].tolist()))
            return
        so, sl, rv = (np.asarray(sequences[x]).astype(np.int64).tolist() for x in ("seq_off", "seq_len", "rev"))
        sh = (np.asarray(sequences["shift_fwd"]).astype(np.int64).tolist(), np.asarray(sequences["shift_rev"]).astype(np.int64).tolist())
        pool = np.asarray(sequences["pool"], dtype=np.uint8).tobytes()
        for i, (h, c) in enumerate(zip(keys.tolist(), counts.tolist())):  # orientation 0 of node i: B when rev == 0, else its reverse complement
            b = pool[so[i]:so[i] + sl[i]]
            f.write("S\t%d\t%s\tLN:i:%d\tKC:i:%d\tkh:Z:%016x\n" % (i, (revcomp(b) if rv[i] else b).decode("latin-1") or "*", sl[i], c, h))
        f.writelines("L\t%d\t%s\t%d\t%s\t%dM\tRC:i:%d\n" % (a >> 1, sign[a & 1], b >> 1, sign[b & 1],
                                                              sl[a >> 1] - sh[0 if (a & 1) == rv[a >> 1] else 1][a >> 1], c)
                     for a, b, c in zip(su.tolist(), sv.tolist(), ec[sel].tolist()))


class FastxReader:
    """FASTA/FASTQ batches (bases back to back + read_off), the front-end that replaces parallel_fastx
    (src/main.rs:79).  Host-only: works without a GPU."""

    def __init__(self, path):
        self.lib = load_library()
        st = C.c_int(0)
        self.rd = self.lib.s2k_fastx_open(os.fsencode(path), C.byref(st))
        if not self.rd:
            raise S2kError(st.value, "cannot open %s" % path)

    def next_batch(self, max_bases=256 << 20, max_reads=0):
        """-> (bases u8 copy, read_off u64 copy) or None at end of file"""
        b, o, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        st = self.lib.s2k_fastx_next(self.rd, max_bases, max_reads, C.byref(b), C.byref(o), C.byref(n))
        if st != 0:
            raise S2kError(st, "malformed FASTA/FASTQ record")
        if n.value == 0:
            return None
        off = np.ctypeslib.as_array(C.cast(o, _u64p), shape=(n.value + 1,)).copy()
        nb = int(off[-1])
        bases = np.ctypeslib.as_array(C.cast(b, _u8p), shape=(max(nb, 1),))[:nb].copy()
        return bases, off

    def close(self):
        if getattr(self, "rd", None):
            self.lib.s2k_fastx_close(self.rd)
            self.rd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


class KminmerHash:
    """src/kminmer.rs:128-135; equality and ordering by `hash` only (src/kminmer.rs:181-204)."""
    __slots__ = ("hash", "start", "end", "offset", "rev")

    def __init__(self, hash, start, end, offset, rev):
        self.hash, self.start, self.end, self.offset, self.rev = hash, start, end, offset, rev

    @classmethod
    def new_from_hash(cls, hash, start, end, offset, rev):  # src/kminmer.rs:169-177
        return cls(hash, start, end, offset, rev)

    def get_hash(self):  # src/kminmer.rs:162-164
        return self.hash

    def __eq__(self, o):
        return self.hash == o.hash

    def __lt__(self, o):
        return self.hash < o.hash

    def __hash__(self):
        return hash(self.hash)

    def __repr__(self):  # Debug formatting of the Rust struct
        return "KminmerHash { hash: %d, start: %d, end: %d, offset: %d, rev: %s }" % (
            self.hash, self.start, self.end, self.offset, "true" if self.rev else "false")


class KminmersIterator:
    """Per-read facade with the reference's constructor signature (src/lib.rs:89) and Iterator shape
    (src/lib.rs:179-181).  One GPU call per read is the wrong granularity for throughput -- use
    Engine.extract for batches; this class exists so reference-style call sites and tests read the same.
    Parameter violations that panic in the reference raise S2kError here."""

    def __init__(self, seq, l, k, density, mode=HashMode.Hpc, engine=None):
        eng = engine or default_engine()
        r = eng.extract_reads([seq], l, k, density, mode)
        self._r = r
        self._i = 0

    @classmethod
    def new(cls, seq, l, k, density, mode, engine=None):
        return cls(seq, l, k, density, mode, engine)

    def __iter__(self):
        return self

    def __next__(self):
        i = self._i
        if i >= self._r["n"]:
            raise StopIteration
        self._i += 1
        r = self._r
        return KminmerHash(int(r["hash"][i]), int(r["start"][i]), int(r["end"][i]), i, bool(r["rev"][i]))


class _MinimizerTriples:
    """The crate's minimizer iterators (re-exported at src/lib.rs:6-13) over S2K_FLAG_WANT_MINIMIZERS: one GPU call per
    sequence -- the wrong granularity for throughput (use Engine.extract(..., want_minimizers=True) for batches); these
    classes exist so reference-style call sites read the same.  Like the reference they take the u32 `hash_bound`, not a
    density.  l > len(seq) raises as KSizeOutOfRange does (src/nthash_hpc.rs:117-121); len(seq) == l is accepted as in the reference."""
    _mode = None

    def __init__(self, seq, l, hash_bound, engine=None):
        a = _as_u8(seq)
        if l > len(a):
            raise S2kError(2, "K size %d is out of range for the given sequence size %d" % (l, len(a)))  # src/nthash_hpc.rs:19-22
        eng = engine or default_engine()
        d = float(eng.lib.s2k_density_for_bound(int(hash_bound)))
        keep = None
        if len(a) == l:
            # seq.len() == l is accepted by the reference's iterators (only l > len is KSizeOutOfRange, src/nthash_hpc.rs:117-121):
            # the scalar Hpc iterator then yields nothing (its only l-mer is the last one, dropped at :265-267); the two SIMD
            # iterators may yield the single l-mer.  KminmersIterator never makes this call (src/lib.rs:97), and the kernels
            # follow it (len <= l: nothing) -- so the l-mer is computed ON THE GPU on the sequence plus one base that starts a new
            # run, and only what lies inside the original sequence is kept.
            if self._mode == HashMode.Hpc:
                self._j = self._jend = self._h = np.empty(0, dtype=np.uint32)
                self._i = 0
                return
            a = np.concatenate((a, np.array([ord("C") if a[-1] == ord("A") else ord("A")], dtype=np.uint8)))
            keep = l
        r = eng.extract_reads([a], l, 1, d, self._mode, want_minimizers=True)
        assert r["counts"]["hash_bound"] == int(hash_bound)
        self._j, self._jend, self._h = r["mn_j"], r["mn_jend"], r["mn_hash"]
        if keep is not None:  # the l-mer that starts at 0 and ends inside the original sequence
            m = (self._j == 0) & (self._jend < keep)
            self._j, self._jend, self._h = self._j[m], self._jend[m], self._h[m]
        self._i = 0

    @classmethod
    def new(cls, seq, l, hash_bound, engine=None):
        return cls(seq, l, hash_bound, engine)

    def __iter__(self):
        return self

    def __len__(self):
        return len(self._h) - self._i

    def _item(self, i):
        return int(self._j[i]), int(self._jend[i]), int(self._h[i])

    def __next__(self):
        if self._i >= len(self._h):
            raise StopIteration
        self._i += 1
        return self._item(self._i - 1)


class NtHashHPCIterator(_MinimizerTriples):
    """src/nthash_hpc.rs:99-283: Item = (start, end, hash) in original space; `<=` against the bound; the last HPC l-mer of the
    sequence is never yielded (:265-267); end = last base of the l-mer's last run (:281)."""
    _mode = HashMode.Hpc


class NtHashHPCSIMDIterator(_MinimizerTriples):
    """src/nthash_hpc_simd.rs:17-68: Item = (start, end, hash); the result semantics of the AVX-512 path: strict `<` against a
    bound re-derived through f32, end = START of the last run (:64), the last l-mer kept, the final block of 16 lost when the
    number of l-mers is a multiple of 16."""
    _mode = HashMode.HpcSimd


class NtHashSIMDIterator(_MinimizerTriples):
    """src/nthash_avx512_32.rs:14-164: Item = (pos, hash) over the sequence as it is (no homopolymer compression)."""
    _mode = HashMode.Simd

    def _item(self, i):
        return int(self._j[i]), int(self._h[i])


class RegularMinimizers(_MinimizerTriples):
    """Not a type of the crate: the (j, jend, hash) triples that the Regular arm of KminmersIterator::next makes from the external
    nthash32::NtHashIterator (src/lib.rs:215-230), for symmetry with the three above."""
    _mode = HashMode.Regular


def _hpc_gpu(seq, engine, rle):
    import torch

    eng = engine or default_engine()
    a = _as_u8(seq)
    n = len(a)
    dev = torch.device("cuda", eng.device)
    d_b = torch.from_numpy(a.copy()).to(dev) if n else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    d_ho = torch.zeros(2, dtype=torch.int64, device=dev)
    d_h = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    d_p = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    r = eng.hpc_device(d_b.data_ptr(), d_off.data_ptr(), 1, n, d_ho.data_ptr(), d_h.data_ptr(), d_p.data_ptr(), max(n, 1), rle=rle)
    return d_h[:r].cpu().numpy().tobytes(), d_p[:r].cpu().numpy().astype(np.uint32)


def _no_sentinel(a, who):
    # hpc / encode_rle start from prev_char = '#' (src/hpc.rs:9,30): a '#' in the input is dropped or misplaces the next
    # run's position there.  The device op treats '#' as an ordinary byte, so such input is refused instead of answered differently.
    if len(a) and (a == 0x23).any():
        raise ValueError("%s: input contains '#', the reference's start sentinel (src/hpc.rs:9,30); not supported" % who)


def hpc(seq, engine=None):
    """Homopolymer-compressed string of one read (any equal characters collapse): src/hpc.rs:28-41, on the GPU.
    hpc("") == "#" as in the reference (the sentinel is flushed at the end, src/hpc.rs:39-40)."""
    a = _as_u8(seq)
    if len(a) == 0:
        return b"#"
    _no_sentinel(a, "hpc")
    return _hpc_gpu(a, engine, False)[0]


def encode_rle(seq, engine=None):
    """(compressed string, run-start positions) with the rule of src/hpc.rs:7-25: only runs of ACTGactgNn collapse
    (src/hpc.rs:14), every other character stays.  encode_rle("") == ("#", [0]) as in the reference."""
    a = _as_u8(seq)
    if len(a) == 0:
        return b"#", np.zeros(1, dtype=np.uint32)
    _no_sentinel(a, "encode_rle")
    return _hpc_gpu(a, engine, True)


def encode_rle_simd(seq, engine=None):
    """(compressed string, run-start positions) -- src/hpc.rs:44-147 (any equal bytes collapse) -- computed on the GPU."""
    return _hpc_gpu(seq, engine, False)
