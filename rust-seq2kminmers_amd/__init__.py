"""rust-seq2kminmers_amd -- host-side mirror of the reference's seq -> k-min-mer interface over the
MI355X C ABI (include/s2k.h, built from csrc/ into csrc/libs2k.so).

Reference interface mirrored here (names, argument meaning, error behaviour):
    KminmersIterator::new(seq, l, k, density, mode)   src/lib.rs:89-131
    impl Iterator { type Item = KminmerHash }         src/lib.rs:179-270
    KminmerHash{hash,start,end,offset,rev}, ==/ord by hash only   src/kminmer.rs:128-135,181-204
    HashMode{Regular,Hpc,Simd,HpcSimd}                src/lib.rs:21-27
    hpc(), encode_rle_simd()                          src/hpc.rs:28-41, 44-147

The package: _abi.py mirrors include/s2k.h (constants, structs, one prototype per function) and loads the library; _args.py puts C
arguments together and checks them; engine.py is Engine, one method per call; pipeline.py holds the classes that chain the calls;
writers.py the text formats and the FASTX reader; iterators.py the reference-shaped per-read facades.  Every public name is re-exported here.

There is no CPU fallback: importing works anywhere (so the CPU test tier can check the ABI), but
creating an Engine without a GPU raises.  The directory name carries a hyphen (as the task names it),
so load it with `import_package()` from s2k_loader.py or importlib.
"""
import ctypes as C  # noqa: F401 -- C, enum, os and np were attributes of the package when it was one module
import enum  # noqa: F401
import os  # noqa: F401

import numpy as np  # noqa: F401

from ._abi import (ABI_SYMBOLS, ABI_VERSION, ALIGN_BAD_PATH, ALIGN_MAX_EDITS, ALIGN_OVER, ALIGN_WAVES, BUBBLE_MAX_NODES, BUBBLE_WAVES, CIGAR_CHARS, CIGAR_D, CIGAR_EQ, CIGAR_I,  # noqa: F401
                   CIGAR_X, CONSENSUS_LONG_STATS, CONSENSUS_STATS, CONSENSUS_STATS_WORDS, COUNT_SORTED, FLAG_FORCE_SERIAL, FLAG_LEGACY_PATH, FLAG_NO_PACK2, FLAG_WANT_MINIMIZERS,
                   HPC_RLE_ALPHABET, LIB_PATH, LONG_INS_MAX, LONG_INS_MIN, LONG_INS_POS_BITS, NO_COPY, NO_EDGE, NO_PARTNER, NO_STEP, PILEUP_MAX_SHIFT, PILEUP_PLANES, PILEUP_STATS, PILEUP_STATS_WORDS,
                   PROTOTYPES, SEGMENT_LEN, SEGMENT_MIN_LEN, SEGMENT_STATS, SEGMENT_STATS_WORDS, STEP_LINKED, WALK_CIRCULAR, AlignOut, Counts, DeviceOut,
                   HashMode, NodePlace, NodeSeqs, Params, Pile, Result, S2kError, SegmentOut, SolidOut, ThreadOut, UnitigOut, WalkOut, hash_bound,
                   load_library)
from ._args import extraction_struct, pack_reads  # noqa: F401
from .engine import Engine  # noqa: F401
from .iterators import (KminmerHash, KminmersIterator, NtHashHPCIterator, NtHashHPCSIMDIterator, NtHashSIMDIterator, RegularMinimizers,  # noqa: F401
                        default_engine, encode_rle, encode_rle_simd, hpc)
from .pipeline import (ContigLift, CountTable, KminmerCounter, KminmerGraph, NodeSequences, PathOrigin, Pileup, PolishedSequences, ReadPaths,  # noqa: F401
                       ReadWalks, SpanTable, UnitigGraph, WalkAlignments, decode_long_keys, walk_query_intervals)
from .writers import (FastxReader, alignment_block_len, cigar_string, revcomp, write_fasta, write_gaf_walks, write_gfa, write_read_paths,  # noqa: F401
                      write_spans, write_unitig_gfa)
