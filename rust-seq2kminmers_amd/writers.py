"""The text formats (paths, GAF, spans, FASTA, GFA) on host arrays, and the FASTX reader.  The GAF lines are also formatted on the
device (Engine.walks_gaf, ReadWalks.gaf_text): write_gaf_walks is the specification of that text."""
import ctypes as C
import os

import numpy as np

from ._abi import CIGAR_CHARS, STEP_LINKED, WALK_FIELDS, S2kError, _Handle, _u8p, _u64p, load_library
from ._args import _as_u8


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


def write_gaf_walks(path, walks, step_unitig, names=None, read_lengths=None, first_read=0, alignments=None):
    """ReadWalks.write_gaf on host arrays: walks = the dict ReadWalks.host() returns, step_unitig = the paths' oriented unitig per
    step.  One line per walk, tab-separated: read name, read length (*: unknown), qstart, qend, +, the path as >t (oriented unitig 2
    t) or <t (2 t + 1) per step with the unitig names of write_unitig_gfa, path_len, path_start, path_end, items (the matches column:
    k-min-mers, not bases), max(qend - qstart, path_end - path_start) (the block length), 255, km:i:<items>, ns:i:<n_steps>.  On a
    circular unitig path_end may pass path_len (include/s2k.h).  alignments: the dict WalkAlignments.host() returns (edits, matches,
    n_ops, ops_off, ops, flags per walk); a walk whose flags are 0 then has the residue matches in the matches column, the sum of its
    run lengths as the block length, and NM:i:<edits> and cg:Z:<runs with = X I D> after the two tags; a flagged walk keeps the line
    it has without alignments.  s2k_walks_gaf (include/s2k.h) writes the same bytes on the device."""
    off = np.asarray(walks["walk_off"]).astype(np.int64).tolist()
    w = {f: np.asarray(walks[f]).astype(np.int64).tolist() for f in WALK_FIELDS}
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


def cigar_string(ops):
    """runs len << 4 | op -> text with = X I D"""
    return "".join("%d%s" % (int(x) >> 4, CIGAR_CHARS[int(x) & 15]) for x in ops)


def alignment_block_len(ops_off, n_ops, ops):
    """per alignment the sum of its run lengths (uint64)"""
    ln = np.concatenate([[0], np.cumsum(np.asarray(ops).astype(np.uint64) >> np.uint64(4))]).astype(np.uint64)
    a = np.asarray(ops_off).astype(np.int64)[:-1]
    return ln[a + np.asarray(n_ops).astype(np.int64)] - ln[a]


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


class FastxReader(_Handle):
    """FASTA/FASTQ batches (bases back to back + read_off), the front-end that replaces parallel_fastx
    (src/main.rs:79).  Host-only: works without a GPU."""

    _HANDLE, _DESTROY = "rd", "s2k_fastx_close"

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
