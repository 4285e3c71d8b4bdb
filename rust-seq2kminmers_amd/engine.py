"""Engine: one method per call of the C ABI, over host arrays, raw device pointers or torch tensors."""
import ctypes as C
import os

import numpy as np

from ._abi import (ALIGN_MAX_EDITS, CIGAR_I, CONSENSUS_LONG_STATS, CONSENSUS_STATS, CONSENSUS_STATS_WORDS, COUNT_SORTED, FLAG_FORCE_SERIAL, FLAG_LEGACY_PATH, FLAG_NO_PACK2,
                   FLAG_WANT_MINIMIZERS, HPC_RLE_ALPHABET, LONG_INS_MAX, LONG_INS_MIN, PILEUP_MAX_SHIFT, PILEUP_PLANES, PILEUP_STATS, PILEUP_STATS_WORDS, SEGMENT_LEN, SEGMENT_STATS,
                   SEGMENT_STATS_WORDS, STEP_FIELDS, AlignOut, Counts, DeviceOut, HashMode, Params, Pile, Result, S2kError, SegmentOut, ThreadOut, UnitigOut,
                   WalkOut, _Handle, load_library, torch)
from ._args import (_align_out, _as_u8, _graph_arg, _outer_arg, _p, _paths_out, _paths_result, _paths_struct, _shaped, _stitch_arg, _walk_args,
                    extraction_struct, pack_reads)
from .pipeline import KminmerCounter


class Engine(_Handle):
    """One s2k_ctx (one per thread and device, like one KminmersIterator per thread in src/main.rs:65-79)."""

    _HANDLE, _DESTROY = "ctx", "s2k_destroy"

    def __init__(self, device=0):
        self.lib = load_library()
        st = C.c_int(0)
        self.ctx = self.lib.s2k_create(int(device), C.byref(st))
        if not self.ctx:
            raise S2kError(st.value, self.lib.s2k_strerror(st.value).decode())
        self.device = device

    def _check(self, st):
        if st != 0:
            raise S2kError(st, self.lib.s2k_strerror(st).decode() + " -- " + self.lib.s2k_last_error(self.ctx).decode())

    def _run(self, fn, dev, *args):
        """one library call over torch tensors: the library's stream does not follow torch's, so the device is drained first"""
        torch.cuda.synchronize(dev)
        self._check(fn(*args))

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
        if edge_keys.dim() != 1 or edge_keys.element_size() != 8 or not edge_keys.is_cuda:
            raise ValueError("graph_adjacency wants a 1-D 64-bit tensor on the GPU")
        edge_keys = edge_keys.contiguous()
        n, dev = edge_keys.numel(), edge_keys.device
        row_off = torch.empty(2 * int(n_nodes) + 1, dtype=torch.int64, device=dev)
        dst = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        self._run(self.lib.s2k_graph_adjacency, dev, self.ctx, _p(edge_keys, n), n, int(n_nodes), _p(row_off), _p(dst))
        return row_off, dst[:n]

    def graph_unitigs(self, row_off, dst, n_nodes):
        """The unitigs of a twin-symmetric graph (s2k_graph_unitigs) from its CSR as graph_adjacency returns it (S2kError(1) when the
        CSR breaks a rule or an edge's twin is missing) -> dict of GPU tensors uni_off (int64, n_unitigs + 1), members (int32, n_nodes
        oriented ids: the kept strands in path order), node_unitig / node_pos (int32, n_nodes), circular (uint8, n_unitigs), and the ints
        n_unitigs, n_links."""
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
        self._run(self.lib.s2k_graph_unitigs, dev, self.ctx, _p(row_off), _p(dst, ne), ne, n, C.byref(o), C.byref(nu), C.byref(nl))
        t = int(nu.value)
        return {"uni_off": res["uni_off"][:t + 1], "members": res["members"][:n], "node_unitig": res["node_unitig"][:n],
                "node_pos": res["node_pos"][:n], "circular": res["circular"][:t], "n_unitigs": t, "n_links": int(nl.value)}

    def graph_unitig_edges(self, row_off, dst, n_nodes, unitigs):
        """The edges between the oriented unitigs (s2k_graph_unitig_edges): `unitigs` is what graph_unitigs returned for the same CSR
        -> (keys, src_edge): int64 tensors, keys U << 32 | V strictly ascending (as uint64) and the index of the CSR edge each came from."""
        row_off, dst = row_off.contiguous(), dst.contiguous()
        ne, dev = dst.numel(), row_off.device
        cap = ne - unitigs["n_links"]
        keys = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        src = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        no = C.c_uint64(0)
        self._run(self.lib.s2k_graph_unitig_edges, dev, self.ctx, _p(row_off), _p(dst, ne), ne, int(n_nodes),
                  *(_p(unitigs[f]) for f in ("uni_off", "members", "node_unitig", "node_pos")), unitigs["n_unitigs"], _p(keys), _p(src), cap, C.byref(no))
        return keys[:int(no.value)], src[:int(no.value)]

    def graph_simplify_mask(self, unitig_graph, max_tip, max_bubble):
        """One round of tip clipping and simple-bubble popping (s2k_graph_simplify_mask; the rules are in include/s2k.h) on a UnitigGraph:
        a tip holds at most max_tip members, a bubble branch at most max_bubble; 0 switches a rule off -> dict: remove (uint8 GPU tensor,
        one byte per unitig) and the ints n_tips, n_bubbles (a unitig that meets both rules counts in both), n_removed."""
        g = _graph_arg(unitig_graph, ("csr", "uni_off", "counts"),
                       "graph_simplify_mask wants a UnitigGraph: 64-bit counts, one per unitig, and the CSR over its oriented unitigs")
        t, ne, dev = g.t, g.ne, g.row_off.device
        remove = torch.zeros(max(t, 1), dtype=torch.uint8, device=dev)
        nt, nb, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_graph_simplify_mask, dev, self.ctx, _p(g.row_off), _p(g.dst, ne), ne, t, _p(g.uni_off), _p(g.counts, t), int(max_tip),
                  int(max_bubble), _p(remove), C.byref(nt), C.byref(nb), C.byref(nr))
        return {"remove": remove[:t], "n_tips": int(nt.value), "n_bubbles": int(nb.value), "n_removed": int(nr.value)}

    def graph_bubble_mask(self, unitig_graph, max_nodes, max_bubble):
        """One round of bounded superbubble popping (s2k_graph_bubble_mask; the rule is in include/s2k.h) on a UnitigGraph: a bubble's
        interior holds at most max_nodes unitigs (1 .. BUBBLE_MAX_NODES) and at most max_bubble members in all -> dict: remove (uint8 GPU
        tensor, one byte per unitig) and the ints n_sources (oriented unitigs with out >= 2), n_found (bubbles with something to
        remove), n_applied (those that owned their whole interior), n_removed."""
        g = _graph_arg(unitig_graph, ("csr", "uni_off", "counts"),
                       "graph_bubble_mask wants a UnitigGraph: 64-bit counts, one per unitig, and the CSR over its oriented unitigs")
        t, ne, dev = g.t, g.ne, g.row_off.device
        remove = torch.zeros(max(t, 1), dtype=torch.uint8, device=dev)
        ns, nf, na, nr = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_graph_bubble_mask, dev, self.ctx, _p(g.row_off), _p(g.dst, ne), ne, t, _p(g.uni_off), _p(g.counts, t), int(max_nodes),
                  int(max_bubble), _p(remove), C.byref(ns), C.byref(nf), C.byref(na), C.byref(nr))
        return {"remove": remove[:t], "n_sources": int(ns.value), "n_found": int(nf.value), "n_applied": int(na.value), "n_removed": int(nr.value)}

    def graph_induced(self, graph, node_keep=None, node_unitig=None, remove=None):
        """The subgraph of a KminmerGraph that its kept nodes induce (s2k_graph_induced).  Kept: node_keep (uint8 GPU tensor, one byte per
        node, non-zero = kept), or, without it, the nodes whose unitig is not removed: node_unitig (UnitigGraph.node_unitig) and remove
        (graph_simplify_mask's).  -> dict of GPU tensors keys, counts, edge_keys, edge_counts (the kept ones, renumbered) and new_id (int32,
        one per old node: its new id, -1 for a removed node)."""
        n, ne, dev = graph.n_nodes, graph.n_edges, graph.keys.device
        null = C.c_void_p(0)
        if node_keep is not None:
            node_keep = node_keep.contiguous()
            if node_keep.numel() != n or node_keep.element_size() != 1:
                raise ValueError("graph_induced: node_keep holds one byte per node")
            mask_args = (_p(node_keep), null, null, 0)
        elif node_unitig is not None and remove is not None:
            node_unitig, remove = node_unitig.contiguous(), remove.contiguous()
            if node_unitig.numel() != n or node_unitig.element_size() != 4 or remove.element_size() != 1:
                raise ValueError("graph_induced: node_unitig holds one 32-bit unitig per node, remove one byte per unitig")
            # the number of unitigs is the length of remove: the device refuses a node_unitig entry beyond it
            mask_args = (null, _p(node_unitig), _p(remove), remove.numel())
        else:
            raise ValueError("graph_induced wants node_keep, or node_unitig and remove")
        keys, counts, ek, ec = (x.contiguous() for x in (graph.keys, graph.counts, graph.edge_keys, graph.edge_counts))
        new_id = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        ok, oc = torch.empty(max(n, 1), dtype=torch.int64, device=dev), torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        oek, oec = torch.empty(max(ne, 1), dtype=torch.int64, device=dev), torch.empty(max(ne, 1), dtype=torch.int32, device=dev)
        nn, nne = C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_graph_induced, dev, self.ctx, _p(keys, n), _p(counts, n), n, _p(ek, ne), _p(ec, ne), ne, *mask_args,
                  _p(new_id), _p(ok), _p(oc), n, _p(oek), _p(oec), ne, C.byref(nn), C.byref(nne))
        a, b = int(nn.value), int(nne.value)
        return {"keys": ok[:a], "counts": oc[:a], "edge_keys": oek[:b], "edge_counts": oec[:b], "new_id": new_id[:n]}

    def unitig_sequences(self, uni_off, members, circular, n_nodes, node_seqs):
        """The unitigs' base-space sequences (s2k_unitig_sequences) from the arrays graph_unitigs returned and a NodeSequences ->
        (out_off, out, overlap): int64 tensor of n_unitigs + 1 offsets, uint8 tensor of the bases (unitig t is out[out_off[t] :
        out_off[t + 1]]), int32 tensor of the overlap that leaves each oriented unitig 2 t + s."""
        uni_off, members, circular = uni_off.contiguous(), members.contiguous(), circular.contiguous()
        t, n, dev = circular.numel(), int(n_nodes), uni_off.device
        out_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        overlap = torch.zeros(max(2 * t, 1), dtype=torch.int32, device=dev)
        ns, nb = node_seqs.struct(), C.c_uint64(0)
        args = (self.ctx, _p(uni_off), _p(members, n), _p(circular, t), t, n, C.byref(ns), _p(out_off))
        self._run(self.lib.s2k_unitig_sequences, dev, *args, None, _p(overlap), 0, C.byref(nb))
        total = int(nb.value)
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        if total:
            self._run(self.lib.s2k_unitig_sequences, dev, *args, _p(out), _p(overlap), total, C.byref(nb))
        return out_off, out[:total], overlap[:2 * t]

    def table_vote_keys(self, table, o, k):
        """The vote keys of one batch (s2k_table_vote_keys; the rule is in include/s2k.h): o = the GPU tensors extract_device wrote with
        FLAG_WANT_MINIMIZERS plus the batch's `bases` and `read_off`; table: the CountTable of the nodes.  Two calls: the size, then the
        keys.  -> int64 GPU tensor, three keys (whole, forward end, reverse end) per item of the table, in item order."""
        nr = o["km_off"].numel() - 1
        i, nk = extraction_struct(o, nr, ("rev",), mn=True), C.c_uint64(0)
        b, ro = o["bases"], o["read_off"]
        args = (table.handle, nr, C.byref(i), int(k), _p(b, b.numel()), _p(ro))
        self._run(self.lib.s2k_table_vote_keys, ro.device, *args, None, 0, C.byref(nk))
        n = int(nk.value)
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=ro.device)
        if n:
            self._run(self.lib.s2k_table_vote_keys, ro.device, *args, _p(keys), n, C.byref(nk))
        return keys[:n]

    def table_vote_representatives(self, table, vote_table, o, k, ordinal_base, best):
        """best[i] = max(best[i], votes and ordinal of x) over the batch's items x whose hash is key i of `table`
        (s2k_table_vote_representatives); vote_table: the CountTable over the counted vote keys of every batch; best: int64 GPU tensor,
        one entry per key, zeroed before the first batch.  -> the batch's items, to add to ordinal_base."""
        nr = o["km_off"].numel() - 1
        i = extraction_struct(o, nr, ("rev",), mn=True)
        b, ro = o["bases"], o["read_off"]
        if best.numel() < table.n or best.element_size() != 8 or not best.is_contiguous():
            raise ValueError("best holds one 64-bit entry per key of the table")
        self._run(self.lib.s2k_table_vote_representatives, ro.device, table.handle, vote_table.handle, nr, C.byref(i), int(k), _p(b, b.numel()), _p(ro),
                  int(ordinal_base), _p(best, table.n))
        return i.km_capacity

    def vote_ordinals(self, best):
        """-> int64 GPU tensor rep: the ordinal packed into every best[i], all ones where best[i] == 0 (s2k_vote_ordinals): the rep that
        s2k_table_node_sequences takes"""
        best = best.contiguous()
        rep = torch.empty(max(best.numel(), 1), dtype=torch.int64, device=best.device)
        self._run(self.lib.s2k_vote_ordinals, best.device, self.ctx, _p(best, best.numel()), best.numel(), _p(rep))
        return rep[:best.numel()]

    def unitig_node_places(self, uni_off, members, node_unitig, node_pos, circular):
        """Where every node lies on the oriented unitigs (s2k_unitig_node_places), from the arrays graph_unitigs returned -> int32 GPU
        tensor of shape (n_nodes, 4): row i is the NodePlace record (unitig, pos, len, circular) of the forward oriented node 2 i.
        S2kError(1) when the arrays are not a decomposition of the nodes."""
        uni_off, members, node_unitig, node_pos, circular = (x.contiguous() for x in (uni_off, members, node_unitig, node_pos, circular))
        n, t, dev = node_unitig.numel(), circular.numel(), uni_off.device
        if uni_off.numel() != t + 1 or members.numel() != n or node_pos.numel() != n or uni_off.element_size() != 8 or members.element_size() != 4:
            raise ValueError("unitig_node_places wants uni_off (n_unitigs + 1, 64-bit), members / node_unitig / node_pos (n_nodes, 32-bit), circular")
        place = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
        self._run(self.lib.s2k_unitig_node_places, dev, self.ctx, *(_p(x, x.numel()) for x in (uni_off, members, node_unitig, node_pos, circular)), n, t,
                  _p(place))
        return place[:n]

    def paths_spans(self, unitig_graph, paths, edge_support=None):
        """The span keys of one batch's ReadPaths over a UnitigGraph (s2k_paths_spans; the definitions are in include/s2k.h): for every
        step that crosses its whole unitig from an in-edge a to an out-edge b the key a << 32 | b, then its twin's.  Two calls: the
        sizes, then the keys.  edge_support: an int64 GPU tensor of n_edges entries (zeroed by the caller) that gains the steps that
        follow every edge and its twin.  -> (keys, n_followed, n_off_graph): int64 GPU tensor in step order, and the linked steps that
        follow an edge / follow none."""
        g = _graph_arg(unitig_graph, ("csr", "uni_off"), "paths_spans wants a UnitigGraph: the CSR over its oriented unitigs and uni_off")
        t, ne, ns, nr, dev = g.t, g.ne, paths.n_steps, paths.path_off.numel() - 1, paths.path_off.device
        if edge_support is not None and (edge_support.numel() != ne or edge_support.element_size() != 8 or not edge_support.is_contiguous()):
            raise ValueError("edge_support holds one 64-bit entry per edge")
        o, keep = _paths_struct(paths, ("unitig", "pos", "count", "flags"), ns)
        nk, nf, no = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        args = (self.ctx, nr, C.byref(o), ns, _p(g.row_off), _p(g.dst, ne), ne, _p(g.uni_off), t)
        self._run(self.lib.s2k_paths_spans, dev, *args, None, 0, None, C.byref(nk), C.byref(nf), C.byref(no))
        n = int(nk.value)
        keys = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        self._run(self.lib.s2k_paths_spans, dev, *args, _p(keys), n, _p(edge_support, ne), C.byref(nk), C.byref(nf), C.byref(no))
        return keys[:n], int(nf.value), int(no.value)

    def graph_resolve_mask(self, unitig_graph, span_keys, span_counts, min_support=2):
        """Which unitigs of a UnitigGraph a span table resolves (s2k_graph_resolve_mask; the rule is in include/s2k.h): span_keys (64-bit,
        strictly ascending as uint64) and span_counts (32-bit) on the GPU -> dict: resolved (uint8 GPU tensor, one byte per unitig),
        partner (int32 GPU tensor, one entry per edge: the out-edge matched to an edge that enters a resolved unitig, -1 = NO_PARTNER
        otherwise) and the ints n_candidates, n_resolved."""
        text = "graph_resolve_mask wants a UnitigGraph and a span table: 64-bit keys, 32-bit counts of the same length"
        g, sk, sc = _graph_arg(unitig_graph, ("csr",), text), span_keys.contiguous(), span_counts.contiguous()
        t, ne, n, dev = g.t, g.ne, sk.numel(), g.row_off.device
        if not _shaped([sk, sc], [(n, 8), (n, 4)]):
            raise ValueError(text)
        resolved = torch.zeros(max(t, 1), dtype=torch.uint8, device=dev)
        partner = torch.full((max(ne, 1),), -1, dtype=torch.int32, device=dev)
        nc, nr = C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_graph_resolve_mask, dev, self.ctx, _p(g.row_off), _p(g.dst, ne), ne, t, _p(sk, n), _p(sc, n), n, int(min_support), _p(resolved),
                  _p(partner), C.byref(nc), C.byref(nr))
        return {"resolved": resolved[:t], "partner": partner[:ne], "n_candidates": int(nc.value), "n_resolved": int(nr.value)}

    def graph_untangle(self, unitig_graph, resolved, partner):
        """Every resolved unitig of a UnitigGraph duplicated once per matched in-edge / out-edge pair (s2k_graph_untangle; the
        definitions are in include/s2k.h): resolved (uint8, one byte per unitig) and partner (int32, one entry per edge) as
        graph_resolve_mask returned them.  Two calls: the sizes, then the arrays.  -> dict of GPU tensors copy_off (int64, n_unitigs + 1),
        origin (int32, the unitig of every copy), copy_count (int64, the unitig's count shared among its copies by edge count), keys
        (int64, the n_edges edges over the oriented copies, strictly ascending as uint64: graph_adjacency takes them) and src_edge
        (int64, the old edge of every key), and the ints n_copies, n_duplicated."""
        text = "graph_untangle wants a UnitigGraph, one resolved byte per unitig and one 32-bit partner per edge"
        g, resolved, partner = _graph_arg(unitig_graph, ("csr", "counts", "edge_counts"), text), resolved.contiguous(), partner.contiguous()
        t, ne, dev = g.t, g.ne, g.row_off.device
        if not _shaped([resolved, partner], [(t, 1), (ne, 4)]):
            raise ValueError(text)
        args = (self.ctx, _p(g.row_off), _p(g.dst, ne), ne, t, _p(resolved, t), _p(partner, ne), _p(g.counts, t), _p(g.edge_counts, ne))
        nc, nd = C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_graph_untangle, dev, *args, None, None, None, None, None, 0, C.byref(nc), C.byref(nd))
        n = int(nc.value)
        copy_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        origin = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        copy_count = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        keys, src = torch.empty(max(ne, 1), dtype=torch.int64, device=dev), torch.empty(max(ne, 1), dtype=torch.int64, device=dev)
        self._run(self.lib.s2k_graph_untangle, dev, *args, _p(copy_off), _p(origin), _p(copy_count), _p(keys), _p(src), n, C.byref(nc), C.byref(nd))
        return {"copy_off": copy_off, "origin": origin[:n], "copy_count": copy_count[:n], "keys": keys[:ne], "src_edge": src[:ne], "n_copies": n,
                "n_duplicated": int(nd.value)}

    def unitig_expand(self, outer, origin, uni_off, members, circular):
        """The contigs of an untangled graph as node members (s2k_unitig_expand): outer = what graph_unitigs returned with the copies
        as its nodes, origin = graph_untangle's, and uni_off / members / circular = the decomposition the copies came from.  Two
        calls: the size, then the arrays.  -> dict of GPU tensors uni_off (int64, n_contigs + 1), members, node_unitig, node_pos (int32,
        one per node instance; instance m is the oriented node 2 m + its old orientation bit), circular (uint8) and node_origin (int32,
        the old node of every instance), and the int n_members."""
        text = "unitig_expand wants the outer decomposition over the copies, one 32-bit origin per copy, and the inner decomposition"
        (oo, om, oc, origin, uni_off, circular), nt, ncp, t = _outer_arg(outer, origin, uni_off, circular, text)
        members = members.contiguous()
        n, dev = members.numel(), uni_off.device
        if members.element_size() != 4:
            raise ValueError(text)
        args = (self.ctx, _p(oo), _p(om, ncp), _p(oc, nt), nt, ncp, _p(origin, ncp), _p(uni_off), _p(members, n), _p(circular, t), t, n)
        nm = C.c_uint64(0)
        self._run(self.lib.s2k_unitig_expand, dev, *args, None, None, None, None, None, None, 0, C.byref(nm))
        m = int(nm.value)
        res = {"uni_off": torch.zeros(nt + 1, dtype=torch.int64, device=dev), "members": torch.empty(max(m, 1), dtype=torch.int32, device=dev),
               "node_unitig": torch.empty(max(m, 1), dtype=torch.int32, device=dev), "node_pos": torch.empty(max(m, 1), dtype=torch.int32, device=dev),
               "circular": torch.empty(max(nt, 1), dtype=torch.uint8, device=dev), "node_origin": torch.empty(max(m, 1), dtype=torch.int32, device=dev)}
        self._run(self.lib.s2k_unitig_expand, dev, *args, *(_p(res[f]) for f in ("uni_off", "members", "node_unitig", "node_pos", "circular", "node_origin")),
                  m, C.byref(nm))
        out = {f: res[f][:m] for f in ("members", "node_unitig", "node_pos", "node_origin")}
        out.update(uni_off=res["uni_off"], circular=res["circular"][:nt], n_members=m)
        return out

    def unitig_member_offsets(self, uni_off, members, circular, n_nodes, node_seqs):
        """Where every member's piece starts in the stitched unitigs (s2k_unitig_member_offsets: the stitch without its copy) ->
        (member_off, out_off, overlap, n_bases): int64 tensors of n_nodes and n_unitigs + 1 entries, the int32 overlap that leaves
        each oriented unitig, and the bases of all unitigs; out_off and overlap equal those of unitig_sequences."""
        uni_off, members, circular = uni_off.contiguous(), members.contiguous(), circular.contiguous()
        t, n, dev = circular.numel(), int(n_nodes), uni_off.device
        member_off = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
        out_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        overlap = torch.zeros(max(2 * t, 1), dtype=torch.int32, device=dev)
        ns, nb = node_seqs.struct(), C.c_uint64(0)
        self._run(self.lib.s2k_unitig_member_offsets, dev, self.ctx, _p(uni_off), _p(members, n), _p(circular, t), t, n, C.byref(ns), _p(member_off),
                  _p(out_off), _p(overlap), C.byref(nb))
        return member_off[:n], out_off, overlap[:2 * t], int(nb.value)

    def paths_walks(self, unitig_graph, paths, offsets, seq_len, edge=True):
        """The walks of one batch's ReadPaths over a UnitigGraph, with base coordinates (s2k_paths_walks; the definitions are in
        include/s2k.h).  offsets: the (member_off, out_off, overlap, ...) that unitig_member_offsets returned for the graph; seq_len:
        the seq_len of its NodeSequences.  Two calls: the sizes, then the arrays.  -> dict of GPU tensors walk_off (int64, n_reads + 1),
        first_step, items, path_len, path_start, path_end (int64), n_steps, flags (int32), qstart, qend (int32, only when the paths
        carry start and end), edge (int32 per step, -1 = NO_EDGE; only with edge=True), and the ints n_walks, n_followed, n_off_graph."""
        text = "paths_walks wants a UnitigGraph, the offsets Engine.unitig_member_offsets returned for it and one 32-bit seq_len per node"
        g, dev = _graph_arg(unitig_graph, ("csr", "uni_off", "members", "circular"), text), paths.path_off.device
        member_off, out_off, overlap, seq_len = _stitch_arg(g, offsets, seq_len, text)
        t, ne, n, ns, nr = g.t, g.ne, g.n, paths.n_steps, paths.path_off.numel() - 1
        o, keep = _paths_struct(paths, ("unitig", "pos", "count", "flags", "start", "end"), ns)
        args = (self.ctx, nr, C.byref(o), ns, _p(g.row_off), _p(g.dst, ne), ne, _p(g.uni_off), _p(g.circular, t), t, _p(member_off, n), _p(out_off),
                _p(overlap, t), _p(seq_len, n), _p(g.members, n), n)
        nw, nf, no = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_paths_walks, dev, *args, None, C.byref(nw), C.byref(nf), C.byref(no))
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
        self._run(self.lib.s2k_paths_walks, dev, *args, C.byref(w), C.byref(nw), C.byref(nf), C.byref(no))
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
        g = _graph_arg(unitig_graph, ("csr", "uni_off", "circular"),
                       "paths_bridge wants a UnitigGraph: the CSR over its oriented unitigs, uni_off and circular")
        t, ne, ns, nr, dev = g.t, g.ne, paths.n_steps, paths.path_off.numel() - 1, paths.path_off.device
        i, keep = _paths_struct(paths, STEP_FIELDS, ns)
        args = (self.ctx, nr, C.byref(i), ns, _p(g.row_off), _p(g.dst, ne), ne, _p(g.uni_off), _p(g.circular, t), t, int(max_gap), int(max_slip))
        res = {"path_off": torch.zeros(nr + 1, dtype=torch.int64, device=dev)}
        o = ThreadOut()
        o.path_off = res["path_off"].data_ptr()
        no, nm, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_paths_bridge, dev, *args, C.byref(o), None, None, C.byref(no), C.byref(nm), C.byref(nb))
        m = int(no.value)
        per_step = {"join": torch.uint8} if join else {}
        _paths_out(o, res, keep, m, per_step, ns)
        self._run(self.lib.s2k_paths_bridge, dev, *args, C.byref(o), _p(res["matched"]), _p(res.get("join")), C.byref(no), C.byref(nm), C.byref(nb))
        return _paths_result(res, per_step, m, ns, n_merged=int(nm.value), n_bridged=int(nb.value))

    def unitig_copy_places(self, outer, origin, uni_off, circular):
        """Where every copy of an untangled graph lies on its contigs (s2k_unitig_copy_places; the definitions are in include/s2k.h):
        outer = what graph_unitigs returned with the copies as its nodes, origin = graph_untangle's, uni_off / circular = the
        decomposition the copies came from -> int32 GPU tensor of shape (n_copies, 4): row c is the NodePlace record (unitig, pos, len,
        circular) of the forward oriented copy 2 c on the oriented contigs."""
        text = "unitig_copy_places wants the outer decomposition over the copies, one 32-bit origin per copy, and the inner uni_off and circular"
        (oo, om, oc, origin, uni_off, circular), nt, ncp, t = _outer_arg(outer, origin, uni_off, circular, text)
        dev = uni_off.device
        place = torch.empty((max(ncp, 1), 4), dtype=torch.int32, device=dev)
        self._run(self.lib.s2k_unitig_copy_places, dev, self.ctx, _p(oo), _p(om, ncp), _p(oc, nt), nt, ncp, _p(origin, ncp), _p(uni_off), _p(circular, t), t,
                  _p(place))
        return place[:ncp]

    def paths_lift(self, unitig_graph, paths, resolved, partner, copy_off, copy_place, n_contigs, contig_items=None, step_copy=False, join=False):
        """One batch's ReadPaths on a UnitigGraph lifted onto the contigs of its untangling (s2k_paths_lift; the definitions are in
        include/s2k.h).  resolved, partner: what graph_untangle took; copy_off: what it returned; copy_place: unitig_copy_places' tensor;
        contig_items: an int64 GPU tensor of n_contigs entries (zeroed by the caller) that gains the items every contig carries.  Two
        calls: the sizes, then the arrays.  -> dict of GPU tensors path_off (int64, n_reads + 1), unitig, pos, count, item, flags,
        matched (int32; start, end only when the paths carry them), step_copy (int32 per input step, -1 = NO_COPY: dropped; only with
        step_copy=True), join (uint8 per input step; only with join=True), and the ints n_steps, n_merged, n_dropped, n_conflicts."""
        text = ("paths_lift wants a UnitigGraph, one resolved byte per unitig, one 32-bit partner per edge, copy_off (n_unitigs + 1, 64-bit) "
                "and the (n_copies, 4) records of unitig_copy_places")
        g, dev = _graph_arg(unitig_graph, ("csr", "uni_off", "circular"), text), paths.path_off.device
        t, ne, ns, nr, ncp = g.t, g.ne, paths.n_steps, paths.path_off.numel() - 1, copy_place.shape[0]
        resolved, partner, copy_off, copy_place = (x.contiguous() for x in (resolved, partner, copy_off, copy_place))
        if not _shaped([resolved, partner, copy_off, copy_place], [(t, 1), (ne, 4), (t + 1, 8), (4 * ncp, 4)]):
            raise ValueError(text)
        if contig_items is not None and (contig_items.numel() != n_contigs or contig_items.element_size() != 8 or not contig_items.is_contiguous()):
            raise ValueError("contig_items holds one 64-bit entry per contig")
        i, keep = _paths_struct(paths, STEP_FIELDS, ns)
        matched_in = paths.matched.contiguous() if paths.matched is not None else None
        args = (self.ctx, nr, C.byref(i), ns, _p(matched_in, ns), _p(g.row_off), _p(g.dst, ne), ne, _p(g.uni_off), _p(g.circular, t), t, _p(resolved, t),
                _p(partner, ne), _p(copy_off), _p(copy_place, ncp), ncp, int(n_contigs))
        res = {"path_off": torch.zeros(nr + 1, dtype=torch.int64, device=dev)}
        o = ThreadOut()
        o.path_off = res["path_off"].data_ptr()
        tot = [C.c_uint64(0) for _ in range(4)]
        self._run(self.lib.s2k_paths_lift, dev, *args, C.byref(o), None, None, None, None, *(C.byref(x) for x in tot))
        m = int(tot[0].value)
        per_step = {**({"step_copy": torch.int32} if step_copy else {}), **({"join": torch.uint8} if join else {})}
        _paths_out(o, res, keep, m, per_step, ns)
        self._run(self.lib.s2k_paths_lift, dev, *args, C.byref(o), _p(res["matched"]), _p(res.get("step_copy")), _p(res.get("join")),
                  _p(contig_items, n_contigs), *(C.byref(x) for x in tot))
        return _paths_result(res, per_step, m, ns, n_merged=int(tot[1].value), n_dropped=int(tot[2].value), n_conflicts=int(tot[3].value))

    def walks_targets(self, walks, step_unitig, out_off, out, overlap):
        """The bases of every walk's path interval (s2k_walks_targets; the definitions are in include/s2k.h).  walks: a ReadWalks (or
        anything with first_step, n_steps, path_start, path_end, flags); step_unitig: the oriented unitig of every step of its paths;
        out_off, out: the pair UnitigGraph.sequences returned; overlap: the graph's.  Two calls: the sizes, then the bytes.  -> dict of
        GPU tensors tgt_off (int64, n_walks + 1), tgt (uint8), bad (uint8 per walk), and the int n_bytes."""
        nw, dev, args, keep = _walk_args("walks_targets", walks, step_unitig, out_off, out, overlap)
        tgt_off = torch.zeros(nw + 1, dtype=torch.int64, device=dev)
        bad = torch.zeros(max(nw, 1), dtype=torch.uint8, device=dev)
        nb = C.c_uint64(0)
        self._run(self.lib.s2k_walks_targets, dev, self.ctx, *args, None, None, None, 0, C.byref(nb))
        n = int(nb.value)
        tgt = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self._run(self.lib.s2k_walks_targets, dev, self.ctx, *args, _p(tgt_off), _p(tgt), _p(bad), n, C.byref(nb))
        return {"tgt_off": tgt_off, "tgt": tgt[:n], "bad": bad[:nw], "n_bytes": n}

    def align_pairs(self, query, target, q_begin, q_end, t_begin, t_end, max_edits=ALIGN_MAX_EDITS):
        """Global unit-cost alignment of many pairs of byte intervals (s2k_align_pairs; the rule is in include/s2k.h): pair i aligns
        query[q_begin[i] : q_end[i]] with target[t_begin[i] : t_end[i]] (uint8 GPU tensors; int64 GPU tensors of one length).  Two
        calls: the sizes, then the runs.  -> dict of GPU tensors edits, flags, n_ops, matches (int32 per pair), ops_off (int64, n_pairs
        + 1), ops (int32 per run: len << 4 | op; the CIGAR of pair i is ops[ops_off[i] : ops_off[i] + n_ops[i]]), and the int
        n_ops_bound.  A pair whose distance exceeds max_edits has flags & ALIGN_OVER, edits = max_edits + 1 and no run."""
        query, target = query.contiguous(), target.contiguous()
        iv = [x.contiguous() for x in (q_begin, q_end, t_begin, t_end)]
        n, dev = iv[0].numel(), query.device
        if any(x.numel() != n or x.element_size() != 8 for x in iv) or query.element_size() != 1 or target.element_size() != 1:
            raise ValueError("align_pairs wants two byte pools and four 64-bit interval arrays of one length")
        args = (self.ctx, _p(query, query.numel()), query.numel(), _p(target, target.numel()), target.numel(), *(_p(x, n) for x in iv), n, int(max_edits))
        o, res, _ = _align_out(n, dev, fields=("edits", "flags", "ops_off"))
        nb = C.c_uint64(0)
        self._run(self.lib.s2k_align_pairs, dev, *args, C.byref(o), C.byref(nb))
        m = int(nb.value)
        o, res, cut = _align_out(n, dev, m, res)
        self._run(self.lib.s2k_align_pairs, dev, *args, C.byref(o), C.byref(nb))
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
        paths, dev = walks.paths, walks.walk_off.device
        if walks.qstart is None or walks.qend is None:
            raise ValueError("walks_segments wants walks whose paths carry start and end")
        text = "walks_segments wants a UnitigGraph, the offsets Engine.unitig_member_offsets returned for it and one 32-bit seq_len per node"
        g = _graph_arg(unitig_graph, ("uni_off", "members", "circular"), text)
        member_off, out_off, overlap, seq_len = _stitch_arg(g, offsets, seq_len, text)
        t, n, ns, nr = g.t, g.n, paths.n_steps, walks.walk_off.numel() - 1
        rec = {f: getattr(walks, f).contiguous() for f in ("walk_off", "first_step", "n_steps", "qstart", "qend", "path_start", "path_end", "flags")}
        nw = rec["first_step"].numel()
        q_begin, tgt_off, bad = q_begin.contiguous(), tgt_off.contiguous(), bad.contiguous()
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
        args = (self.ctx, nr, C.byref(wo), nw, C.byref(po), ns, _p(g.uni_off), _p(g.members, n), _p(g.circular, t), t, _p(member_off, n), _p(out_off),
                _p(overlap, t), _p(seq_len, n), n, _p(q_begin, nw), _p(tgt_off), _p(bad, nw), C.byref(so), nsrc, _p(maps[0], nsrc), _p(maps[1], nsrc),
                C.byref(d), int(seg_len))
        total, stats = C.c_uint64(0), (C.c_uint64 * SEGMENT_STATS_WORDS)()
        self._run(self.lib.s2k_walks_segments, dev, *args, None, C.byref(total), stats)
        m = int(total.value)
        res = {"seg_off": torch.zeros(nw + 1, dtype=torch.int64, device=dev)}
        for f in ("q_begin", "q_end", "t_begin", "t_end"):
            res[f] = torch.zeros(max(m, 1), dtype=torch.int64, device=dev)
        o = SegmentOut()
        o.capacity = m
        for f, x in res.items():
            setattr(o, f, x.data_ptr())
        self._run(self.lib.s2k_walks_segments, dev, *args, C.byref(o), C.byref(total), stats)
        out = {f: (x if f == "seg_off" else x[:m]) for f, x in res.items()}
        out.update(n_segments=m, stats={f: int(stats[i]) for i, f in enumerate(SEGMENT_STATS)})
        return out

    def align_join(self, seg_off, bad, segments):
        """The segments' alignments put back together, one per walk (s2k_align_join; the rule is in include/s2k.h).  seg_off, bad: what
        walks_segments and walks_targets returned; segments: what align_pairs returned for the segment pairs (anything with edits,
        flags, ops_off, n_ops, matches, ops as attributes or keys).  Two calls: the size, then the runs.  -> dict of GPU tensors edits,
        flags, n_ops, matches (int32 per walk), ops_off (int64, n_walks + 1, compact), ops (int32 per joined run) and the int
        n_ops_total."""
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
        self._run(self.lib.s2k_align_join, dev, *args, None, C.byref(total))
        m = int(total.value)
        o, _, cut = _align_out(nw, dev, m)
        self._run(self.lib.s2k_align_join, dev, *args, C.byref(o), C.byref(total))
        return {**cut(), "n_ops_total": m}

    def walks_gaf(self, walks, step_unitig, names=None, read_lengths=None, first_read=0, alignments=None):
        """The GAF lines of the walks, formatted on the device (s2k_walks_gaf; the format is in include/s2k.h and is what
        write_gaf_walks writes).  walks: a ReadWalks (or anything with walk_off and the record arrays but flags); step_unitig: the oriented
        unitig of every step of its paths; names: one str (encoded as UTF-8) or bytes per read, None: the index first_read + r;
        read_lengths: one length per read (a sequence or a tensor), None: *; alignments: a WalkAlignments or the dict align_pairs /
        align_join returned for the walks.  Two calls: the sizes, then the bytes.  -> dict of GPU tensors text (uint8), line_off (int64,
        n_walks + 1) and the int n_bytes."""
        rec = {f: getattr(walks, f) for f in ("walk_off", "first_step", "n_steps", "items", "qstart", "qend", "path_len", "path_start", "path_end")}
        if rec["qstart"] is None or rec["qend"] is None:
            raise ValueError("walks_gaf wants walks whose paths carry start and end")
        rec = {f: x.contiguous() for f, x in rec.items()}
        step_unitig = step_unitig.contiguous()
        nr, nw, ns, dev = rec["walk_off"].numel() - 1, rec["first_step"].numel(), step_unitig.numel(), rec["walk_off"].device
        if (any(rec[f].numel() != nw for f in rec if f != "walk_off") or [rec[f].element_size() for f in rec] != [8, 8, 4, 8, 4, 4, 8, 8, 8]
                or step_unitig.element_size() != 4):
            raise ValueError("walks_gaf wants walk_off, the walk records and one 32-bit unitig per step")
        wo = WalkOut()
        wo.capacity = nw
        for f, x in rec.items():
            setattr(wo, f, x.data_ptr() if x.numel() else 0)
        pool = name_off = lens = None
        n_pool = 0
        if names is not None:
            enc = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in names]
            if len(enc) != nr:
                raise ValueError("walks_gaf wants one name per read")
            off = np.zeros(nr + 1, dtype=np.int64)
            np.cumsum([len(x) for x in enc], out=off[1:])
            n_pool = int(off[-1])
            pool = torch.from_numpy(np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()).to(dev)
            name_off = torch.from_numpy(off).to(dev)
        if read_lengths is not None:
            lens = read_lengths.to(device=dev, dtype=torch.int64).contiguous() if torch.is_tensor(read_lengths) else \
                torch.from_numpy(np.asarray(read_lengths).astype(np.uint64).view(np.int64).copy()).to(dev)
            if lens.numel() != nr:
                raise ValueError("walks_gaf wants one length per read")
        ao, keep = None, None
        if alignments is not None:
            get = alignments.get if isinstance(alignments, dict) else lambda f: getattr(alignments, f)
            keep = {f: get(f).contiguous() for f in ("edits", "flags", "ops_off", "n_ops", "matches", "ops")}
            if (keep["ops_off"].numel() != nw + 1 or keep["ops_off"].element_size() != 8 or keep["ops"].element_size() != 4
                    or any(keep[f].element_size() != 4 or keep[f].numel() < nw for f in ("edits", "flags", "n_ops", "matches"))):
                raise ValueError("walks_gaf wants the arrays align_pairs or align_join wrote for the walks")
            ao = AlignOut()
            ao.capacity = keep["ops"].numel()
            for f, x in keep.items():
                setattr(ao, f, x.data_ptr() if x.numel() else 0)
        args = (self.ctx, nr, C.byref(wo), nw, _p(step_unitig, ns), ns, _p(pool, names is not None), _p(name_off, names is not None), n_pool, int(first_read),
                _p(lens, lens is not None), C.byref(ao) if ao is not None else None)
        nb = C.c_uint64(0)
        self._run(self.lib.s2k_walks_gaf, dev, *args, None, 0, None, C.byref(nb))
        n = int(nb.value)
        text = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        line_off = torch.zeros(nw + 1, dtype=torch.int64, device=dev)
        self._run(self.lib.s2k_walks_gaf, dev, *args, _p(text), n, _p(line_off), C.byref(nb))
        return {"text": text[:n], "line_off": line_off, "n_bytes": n}

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

    def _pileup_args(self, name, walks, step_unitig, out_off, out, overlap, query, q_begin, alignments, planes, max_shift):
        """what walks_pileup and walks_pileup_ex (name) share -> (device, the C arguments ctx .. max_shift, the pile, the tensors to keep alive)"""
        nw, dev, wargs, keep = _walk_args(name, walks, step_unitig, out_off, out, overlap)
        query, q_begin = query.contiguous(), q_begin.contiguous()
        al = [getattr(alignments, f).contiguous() for f in ("flags", "ops_off", "n_ops", "ops")]
        if (query.element_size() != 1 or q_begin.numel() != nw or q_begin.element_size() != 8 or [x.element_size() for x in al] != [4, 8, 4, 4]
                or al[0].numel() < nw or al[2].numel() < nw or al[1].numel() != nw + 1):
            raise ValueError(name + " wants the batch's bases, one 64-bit interval start per walk and the alignment arrays of these walks")
        pile = self._pile_struct(planes, out.numel())
        args = (self.ctx, *wargs, _p(query, query.numel()), query.numel(), _p(q_begin, nw), _p(al[0], nw), _p(al[1]), _p(al[2], nw), _p(al[3], al[3].numel()),
                al[3].numel(), int(max_shift))
        return dev, args, pile, (keep, query, q_begin, al)

    def walks_pileup_ex(self, walks, step_unitig, out_off, out, overlap, query, q_begin, alignments, planes, max_shift=PILEUP_MAX_SHIFT):
        """walks_pileup, and the vote keys of the batch's long insertions (s2k_walks_pileup_ex; the key is defined in include/s2k.h).
        The key buffer is sized by a count of the I runs of 2 .. 12 bytes over all run words, which bounds n_candidates.  -> (dict
        of the PILEUP_STATS counters, keys: 1-D int64 GPU tensor whose bits are the uint64 keys, in run-slot order, n_candidates)."""
        dev, args, pile, keep = self._pileup_args("walks_pileup_ex", walks, step_unitig, out_off, out, overlap, query, q_begin, alignments, planes, max_shift)
        ops = keep[3][3]
        n = ops >> 4 & 0x0FFFFFFF  # (the run words are uint32 in an int32 tensor)
        cap = int(((ops & 15) == CIGAR_I).logical_and(n >= LONG_INS_MIN).logical_and(n <= LONG_INS_MAX).sum()) if ops.numel() else 0
        buf = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        stats, nc, nk = (C.c_uint64 * PILEUP_STATS_WORDS)(), C.c_uint64(0), C.c_uint64(0)
        self._run(self.lib.s2k_walks_pileup_ex, dev, *args, C.byref(pile), stats, _p(buf), cap, C.byref(nc), C.byref(nk))
        return {f: int(stats[i]) for i, f in enumerate(PILEUP_STATS)}, buf[:int(nk.value)], int(nc.value)

    def walks_pileup(self, walks, step_unitig, out_off, out, overlap, query, q_begin, alignments, planes, max_shift=PILEUP_MAX_SHIFT):
        """The votes of one batch's aligned walks added to a pile (s2k_walks_pileup; the rule is in include/s2k.h).  walks, step_unitig,
        out_off, out, overlap: as walks_targets takes them; query: the batch's bases (uint8 GPU tensor); q_begin: where every walk's
        read interval starts in them (int64); alignments: a WalkAlignments (or anything with flags, ops_off, n_ops, ops) of these
        walks; planes: the (11, n_bases) int32 GPU tensor of the pile, rows in the order of PILEUP_PLANES, zeroed before the first
        batch -- it gains the votes.  -> dict of the PILEUP_STATS counters of this call."""
        dev, args, pile, keep = self._pileup_args("walks_pileup", walks, step_unitig, out_off, out, overlap, query, q_begin, alignments, planes, max_shift)
        stats = (C.c_uint64 * PILEUP_STATS_WORDS)()
        self._run(self.lib.s2k_walks_pileup, dev, *args, C.byref(pile), stats)
        return {f: int(stats[i]) for i, f in enumerate(PILEUP_STATS)}

    def pileup_consensus_ex(self, planes, out_off, out, overlap, min_cov=3, long_keys=None, long_counts=None):
        """pileup_consensus with a table of long-insertion vote keys (s2k_pileup_consensus_ex): long_keys (64-bit, strictly ascending as
        uint64) and long_counts (32-bit), GPU tensors of one length as KminmerCounter.finish returns them; None or empty: pileup_consensus.
        -> the same dict, stats with the CONSENSUS_LONG_STATS counters."""
        return self._consensus(planes, out_off, out, overlap, min_cov, long_keys, long_counts, True)

    def pileup_consensus(self, planes, out_off, out, overlap, min_cov=3):
        """The polished bases of every unitig from a pile (s2k_pileup_consensus; the rule is in include/s2k.h).  planes: the pile, only
        read; out_off, out, overlap: the draft the pile was taken on.  Two calls: the size, then the bytes.  -> dict of GPU tensors
        out_off (int64, n_unitigs + 1), out (uint8), pos_map (int64, n_bases + 1), overlap (int32, 2 n_unitigs), the int n_bases and
        the CONSENSUS_STATS counters in stats."""
        return self._consensus(planes, out_off, out, overlap, min_cov, None, None, False)

    def _consensus(self, planes, out_off, out, overlap, min_cov, keys, counts, ex):
        out_off, out, overlap = (x.contiguous() for x in (out_off, out, overlap))
        t, nb, dev = out_off.numel() - 1, out.numel(), out_off.device
        if out_off.element_size() != 8 or out.element_size() != 1 or overlap.numel() != 2 * t or overlap.element_size() != 4:
            raise ValueError("pileup_consensus%s wants the out_off, out and overlap of the unitig sequences" % ("_ex" if ex else ""))
        pile = self._pile_struct(planes, nb)
        args = (self.ctx, C.byref(pile), _p(out_off), _p(out, nb), nb, _p(overlap, t), t, int(min_cov))
        n, stats = C.c_uint64(0), (C.c_uint64 * CONSENSUS_STATS_WORDS)()
        fn, tail, names = self.lib.s2k_pileup_consensus, (), CONSENSUS_STATS
        if ex:
            nk = 0 if keys is None else keys.numel()
            if nk:
                keys, counts = keys.contiguous(), counts.contiguous()
                if keys.element_size() != 8 or counts.element_size() != 4 or counts.numel() != nk:
                    raise ValueError("pileup_consensus_ex wants 64-bit keys and as many 32-bit counts")
            fn, tail, names = self.lib.s2k_pileup_consensus_ex, ((_p(keys), _p(counts), nk) if nk else (None, None, 0)), CONSENSUS_LONG_STATS
        self._run(fn, dev, *args, None, None, 0, None, None, C.byref(n), stats, *tail)
        m = int(n.value)
        new_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
        new_out = torch.zeros((max(m, 1) + 7) // 8 * 8, dtype=torch.uint8, device=dev)  # whole 8-byte words: walks_targets can read it
        pos_map = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
        new_ov = torch.zeros(max(2 * t, 1), dtype=torch.int32, device=dev)
        self._run(fn, dev, *args, _p(new_off), _p(new_out), m, _p(pos_map), _p(new_ov, t), C.byref(n), stats, *tail)
        return {"out_off": new_off, "out": new_out[:m], "pos_map": pos_map, "overlap": new_ov[:2 * t], "n_bases": m,
                "stats": {f: int(stats[i]) for i, f in enumerate(names)}}

    def partition_device(self, d_hash, n, n_parts, d_out, d_part_off):
        """keys grouped by hash prefix into n_parts ranges (the send buffers of the all-to-all)"""
        self._check(self.lib.s2k_partition_device(self.ctx, C.c_void_p(d_hash or 0), n, n_parts, C.c_void_p(d_out or 0), C.c_void_p(d_part_off)))
