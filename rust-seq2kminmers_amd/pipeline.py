"""The classes that chain the Engine's calls into the pipeline: count, table, graph, unitigs, paths, walks, alignments, pile."""
import ctypes as C

import numpy as np

from ._abi import (ALIGN_BAD_PATH, ALIGN_MAX_EDITS, ALIGN_OVER, LONG_INS_POS_BITS, PILEUP_MAX_SHIFT, PILEUP_PLANES, PILEUP_STATS, SEGMENT_LEN, STEP_FIELDS, WALK_FIELDS, NodeSeqs,
                   S2kError, SolidOut, ThreadOut, _Handle, torch)
from ._args import _p, extraction_struct
from .writers import alignment_block_len, cigar_string, write_gaf_walks, write_gfa, write_read_paths, write_spans, write_unitig_gfa


class KminmerCounter(_Handle):
    """Accumulating k-min-mer count over batches and files (s2k_counter_*): add device-resident hashes batch by batch, finish(min_count)
    -> the solid pairs in ascending key order, equal to Engine.count_device_ex over the concatenation of everything added.  The counter
    keeps its runs in HBM (about 12 B per distinct key); close() it before its Engine."""

    _DESTROY = "s2k_counter_destroy"

    def __init__(self, engine):
        self.engine = engine
        self.lib = engine.lib
        st = C.c_int(0)
        self.handle = self.lib.s2k_counter_create(engine.ctx, C.byref(st))
        if not self.handle:
            raise S2kError(st.value, self.lib.s2k_strerror(st.value).decode())
        self.last_sizes = (0, 0)

    def add(self, d_hash, n):
        """hashes d_hash[0..n) (a device pointer; any n): counted now, the buffer may be reused on return"""
        self.engine._check(self.lib.s2k_counter_add(self.handle, C.c_void_p(d_hash or 0), int(n)))

    def add_tensor(self, t):
        """a 1-D int64 / uint64 torch tensor on the engine's device (its bits are the uint64 hashes)"""
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
        nd, nk = self.sizes(min_count)
        dev = torch.device("cuda", self.engine.device)
        keys = torch.empty(max(nk, 1), dtype=torch.int64, device=dev)
        counts = torch.empty(max(nk, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        if nk:
            a, b = C.c_uint64(0), C.c_uint64(0)
            self.engine._check(self.lib.s2k_counter_finish(self.handle, int(min_count), _p(keys), _p(counts), nk, C.byref(a), C.byref(b)))
        return keys[:nk], counts[:nk]


class CountTable(_Handle):
    """Look-ups against a count table (s2k_table_*): keys (1-D 64-bit tensor on the engine's device, strictly ascending as uint64) and
    counts (32-bit tensor of the same length, or None for a membership table), as KminmerCounter.finish or Engine.count_device_ex write
    them.  The table borrows both tensors (it keeps references to them); they must not change until close().  close() it before its
    Engine."""

    _DESTROY = "s2k_table_destroy"

    def __init__(self, engine, keys, counts=None):
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
        self.handle = self.lib.s2k_table_create(engine.ctx, _p(keys, self.n), _p(counts, self.n), self.n, C.byref(st))
        if not self.handle:
            raise S2kError(st.value, self.lib.s2k_strerror(st.value).decode() + " -- " + self.lib.s2k_last_error(engine.ctx).decode())

    def lookup(self, query):
        """-> int32 tensor (the uint32 counts' bits) of the count of every element of `query` (1-D 64-bit GPU tensor), 0 if absent"""
        if query.dim() != 1 or query.element_size() != 8 or not query.is_cuda:
            raise ValueError("lookup wants a 1-D 64-bit tensor on the GPU")
        query = query.contiguous()
        out = torch.empty(max(query.numel(), 1), dtype=torch.int32, device=query.device)
        self.engine._run(self.lib.s2k_table_lookup, query.device, self.handle, _p(query), query.numel(), _p(out))
        return out[:query.numel()]

    def filter(self, out_tensors, n_reads, min_count=2):
        """Each read's k-min-mers whose count is at least min_count, in read order (s2k_table_filter).  out_tensors: the GPU tensors
        extract_device wrote (dict with km_off and hash; start / end / rev optional).  -> dict of GPU tensors km_off (n_reads + 1),
        hash, offset (index in the read before filtering), count, and start / end / rev where given; 'n' = kept items."""
        dev = out_tensors["km_off"].device
        i, o = extraction_struct(out_tensors, n_reads, ("start", "end", "rev")), SolidOut()
        cap = max(i.km_capacity, 1)
        res = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
               "offset": torch.empty(cap, dtype=torch.int32, device=dev), "count": torch.empty(cap, dtype=torch.int32, device=dev)}
        for f, dt in (("start", torch.int32), ("end", torch.int32), ("rev", torch.uint8)):
            if out_tensors.get(f) is not None:
                res[f] = torch.empty(cap, dtype=dt, device=dev)
        o.capacity = cap
        for f, t in res.items():
            setattr(o, f, t.data_ptr())
        nk = C.c_uint64(0)
        self.engine._run(self.lib.s2k_table_filter, dev, self.handle, n_reads, C.byref(i), int(min_count), C.byref(o), C.byref(nk))
        n = int(nk.value)
        out = {f: (t if f == "km_off" else t[:n]) for f, t in res.items()}
        out["n"] = n
        return out

    def edges(self, out_tensors, n_reads, min_count=2):
        """The graph edges that the reads traverse (s2k_table_edges): out_tensors = the GPU tensors extract_device wrote (dict with
        km_off, hash and rev).  Node i is key i of this table, oriented node 2 * i + rev.  -> int64 tensor of the edge keys
        (u << 32 | v as uint64 bits) in emission order: each adjacency of two solid consecutive items of a read, then its twin
        ((v ^ 1) << 32 | u ^ 1) unless it is its own."""
        dev = out_tensors["km_off"].device
        i = extraction_struct(out_tensors, n_reads, required=("km_off", "hash", "rev"))
        cap = 2 * i.km_capacity  # at most two keys per item
        keys = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
        ne = C.c_uint64(0)
        self.engine._run(self.lib.s2k_table_edges, dev, self.handle, n_reads, C.byref(i), int(min_count), _p(keys), cap, C.byref(ne))
        return keys[:int(ne.value)]

    def thread(self, out_tensors, n_reads, place, n_unitigs, out, min_count=2, uni_items=None):
        """The reads' paths through a unitig decomposition of this table's keys (s2k_table_thread; the definitions are in include/s2k.h).
        out_tensors: the GPU tensors extract_device wrote (km_off, hash, rev; start / end when `out` asks for them); place: what
        Engine.unitig_node_places returned for the decomposition; out: a ThreadOut naming the arrays to fill (path_off required; all step
        arrays 0: the sizes only); uni_items: int64 GPU tensor, one entry per unitig, that gains every step's count.  -> the number of
        steps.  S2kError(7) when out.capacity is short: nothing was written to the step arrays."""
        dev = out_tensors["km_off"].device
        if place.numel() != 4 * self.n or place.element_size() != 4 or not place.is_contiguous():
            raise ValueError("thread wants the (n_keys, 4) 32-bit place tensor of Engine.unitig_node_places")
        if uni_items is not None and (uni_items.numel() != int(n_unitigs) or uni_items.element_size() != 8 or not uni_items.is_contiguous()):
            raise ValueError("uni_items holds one 64-bit entry per unitig")
        i = extraction_struct(out_tensors, n_reads, ("hash", "rev", "start", "end"), required=("km_off",))
        ns = C.c_uint64(0)
        self.engine._run(self.lib.s2k_table_thread, dev, self.handle, n_reads, C.byref(i), int(min_count), _p(place, self.n), self.n, C.byref(out),
                         _p(uni_items, n_unitigs), int(n_unitigs), C.byref(ns))
        return int(ns.value)


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
                i = extraction_struct(o, nr, ("rev",), mn=True)
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
                    engine._check(engine.lib.s2k_table_representatives(table.handle, nr, C.byref(i), base, _p(rep)))
                    base += i.km_capacity

            def round_(ns):
                base, used = 0, 0
                for (i, nr), (b, ro) in zip(ins, bases):
                    nb = C.c_uint64(0)
                    engine._check(engine.lib.s2k_table_node_sequences(table.handle, nr, C.byref(i), k, _p(b, b.numel()), _p(ro), base, _p(rep),
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


    def simplify(self, engine, max_tip, max_bubble, max_rounds=16, bubble_nodes=0):
        """Clips tips of at most max_tip members and pops simple bubbles whose removed branch holds at most max_bubble members (the rules
        are in include/s2k.h; 0 switches one off), round by round on the device -- unitigs, Engine.graph_simplify_mask,
        Engine.graph_induced, Engine.graph_adjacency -- until a round removes nothing or max_rounds rounds have run.
        bubble_nodes > 0: a round in which those two rules remove nothing runs Engine.graph_bubble_mask(bubble_nodes, max_bubble) on the
        same unitig graph -- bubbles that are not simple, an interior of at most bubble_nodes unitigs and max_bubble members -- and
        applies its mask instead; the loop then ends when both remove nothing.  The two masks are never applied in one round: their
        orders differ (mean count there, summed count here), and their union could remove both branches of one bubble.
        -> (graph, node_map, stats): a new KminmerGraph over the kept nodes (self is untouched); node_map, an int32 GPU tensor with the
        final id of every node of self, -1 for a removed one; stats, one dict per round (nodes and unitigs the round started from, tips,
        bubbles and unitigs it removed; a round that ran the bubble mask also sources, found and applied, and its removed is that
        mask's), the last of which removed nothing when a fixed point was reached."""
        g = KminmerGraph(self.keys, self.counts, self.edge_keys, self.edge_counts, self.row_off, self.dst)
        node_map = torch.arange(self.n_nodes, dtype=torch.int32, device=self.keys.device)
        stats = []
        for _ in range(max_rounds):
            ug = g.unitigs(engine)
            m = engine.graph_simplify_mask(ug, max_tip, max_bubble)
            stats.append({"nodes": g.n_nodes, "unitigs": ug.n_unitigs, "tips": m["n_tips"], "bubbles": m["n_bubbles"], "removed": m["n_removed"]})
            if m["n_removed"] == 0 and bubble_nodes > 0:
                m = engine.graph_bubble_mask(ug, bubble_nodes, max_bubble)
                stats[-1].update(sources=m["n_sources"], found=m["n_found"], applied=m["n_applied"], removed=m["n_removed"])
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

    def pileup(self, engine, sequences, long_ins=False):
        """An empty pile over this graph's draft bases -> Pileup.  sequences: the pair self.sequences returned.  Pileup.add takes the
        walks and alignments of one batch after self.align; Pileup.consensus gives the polished bases.  It works as it is on
        simplified graphs and on the contigs of untangle_map with lifted paths.  long_ins: insertions of 2 .. 12 bases are voted by
        key and called too; the Pileup then owns a KminmerCounter: close() it before the engine."""
        if getattr(self, "overlap", None) is None:
            raise ValueError("pileup wants the pair that self.sequences(engine, node_seqs) returned")
        return Pileup(self, sequences, engine if long_ins else None)

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

    STEP_FIELDS = STEP_FIELDS

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



class ReadWalks:
    """The walks of one batch of reads (UnitigGraph.walks; include/s2k.h: s2k_paths_walks): the walks of read r are walk_off[r] ..
    walk_off[r + 1]; walk w holds the steps first_step[w] .. first_step[w] + n_steps[w] of `paths`, each after the first entered over
    a graph edge; it covers items[w] k-min-mers, the read's bases qstart[w] .. qend[w] (None when the paths carry no start / end) and
    the bases path_start[w] .. path_end[w] of its stitched path of path_len[w] bases; flags[w] & WALK_CIRCULAR tells a walk on a
    circular unitig.  edge[s] = the edge step s follows, -1 for none.  GPU tensors: int64, and int32 holding the uint32 values."""

    FIELDS = WALK_FIELDS

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

    def gaf_text(self, engine, graph=None, names=None, read_lengths=None, first_read=0, alignments=None):
        """The GAF lines of write_gaf as bytes on the device (Engine.walks_gaf; include/s2k.h: s2k_walks_gaf), arguments as write_gaf
        -> dict of GPU tensors text (uint8), line_off (int64, n_walks + 1: where every walk's line starts) and the int n_bytes.  What
        a loop over batches appends to one file."""
        if self.qstart is None or self.qend is None:
            raise ValueError("gaf_text wants paths that carry start and end (extract with start / end kept)")
        return engine.walks_gaf(self, self.paths.unitig, names=names, read_lengths=read_lengths, first_read=first_read, alignments=alignments)

    def write_gaf(self, path, graph=None, names=None, read_lengths=None, first_read=0, alignments=None, engine=None):
        """One GAF line per walk (write_gaf_walks).  graph: the UnitigGraph the walks were taken on (only its naming is used: unitig t
        is segment t, as in write_unitig_gfa; may be None); names: one name per read (the index first_read + r when None);
        read_lengths: one length per read (* when None); alignments: the WalkAlignments UnitigGraph.align returned for these walks
        (residue matches, block length, NM:i: and cg:Z: on every walk it aligned).  engine: an Engine formats the lines on the device
        (gaf_text), then one copy to the host and one write of the bytes; None: the host writer.  The file is the same."""
        if self.qstart is None or self.qend is None:
            raise ValueError("write_gaf wants paths that carry start and end (extract with start / end kept)")
        if engine is not None:
            text = self.gaf_text(engine, graph, names=names, read_lengths=read_lengths, first_read=first_read, alignments=alignments)["text"]
            with open(path, "wb") as out:
                out.write(text.cpu().numpy().data)
            return
        h = self.host()
        write_gaf_walks(path, h, self.paths.unitig.cpu().numpy().view(np.uint32), names=names, read_lengths=read_lengths, first_read=first_read,
                        alignments=None if alignments is None else alignments.host())


def walk_query_intervals(walks, read_off):
    """-> (begin, end): int64 GPU tensors with every walk's read interval [read_off[r] + qstart, read_off[r] + qend) in the batch's
    bases, the read r of a walk from walk_off"""
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


class Pileup:
    """The votes of aligned read walks on the bases of a UnitigGraph's draft (UnitigGraph.pileup; include/s2k.h: s2k_walks_pileup,
    s2k_pileup_consensus): planes, an (11, n_bases) int32 GPU tensor with one row per plane of PILEUP_PLANES (match, del, sub0..3,
    ins0..3, ins_long), indexed by position in the draft `sequences` = (out_off, out); graph, the UnitigGraph.  add() once per batch,
    from file to file; consensus() whenever wanted, the pile is only read.  With long_ins (UnitigGraph.pileup(long_ins=True)) every add()
    also feeds the vote keys of the batch's insertions of 2 .. 12 bases (s2k_walks_pileup_ex) to a KminmerCounter of its own, consensus()
    calls them from its table (s2k_pileup_consensus_ex), and close() frees the counter."""

    def __init__(self, graph, sequences, long_ins_engine=None):
        self.graph, self.sequences = graph, sequences
        self.planes = torch.zeros((len(PILEUP_PLANES), max(sequences[1].numel(), 1)), dtype=torch.int32, device=sequences[1].device)
        self.stats = {f: 0 for f in PILEUP_STATS}
        self.long_ins = long_ins_engine is not None
        self.counter = KminmerCounter(long_ins_engine) if self.long_ins else None
        self.n_long_keys = self.n_long_candidates = 0  # over all batches: keyed runs, and I runs of 2 .. 12 bytes

    def close(self):
        if self.counter is not None:
            self.counter.close()
            self.counter = None

    def add(self, engine, walks, alignments, bases, read_off, max_shift=PILEUP_MAX_SHIFT):
        """One batch's votes: walks, the ReadWalks graph.walks returned; alignments, the WalkAlignments graph.align returned for them;
        bases, read_off: the batch's bases and read offsets on the GPU.  -> the PILEUP_STATS counters of this batch (self.stats sums
        them)."""
        qb, _ = walk_query_intervals(walks, read_off)
        if self.long_ins:
            st, keys, nc = engine.walks_pileup_ex(walks, walks.paths.unitig, self.sequences[0], self.sequences[1], self.graph.overlap, bases, qb, alignments,
                                                  self.planes, max_shift)
            self.counter.add_tensor(keys)
            self.n_long_keys += keys.numel()
            self.n_long_candidates += nc
        else:
            st = engine.walks_pileup(walks, walks.paths.unitig, self.sequences[0], self.sequences[1], self.graph.overlap, bases, qb, alignments, self.planes,
                                     max_shift)
        for f, v in st.items():
            self.stats[f] += v
        return st

    def depth(self):
        """match + the four sub + del per position: the walks whose alignment covers it (int64 GPU tensor)"""
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

        if self.long_ins:  # a called candidate has 2 count > depth >= min_cov: the cutoff drops none of them
            keys, counts = self.counter.finish(min_count=int(min_cov) // 2 + 1)
            c = engine.pileup_consensus_ex(self.planes, self.sequences[0], self.sequences[1], self.graph.overlap, min_cov, keys, counts)
        else:
            c = engine.pileup_consensus(self.planes, self.sequences[0], self.sequences[1], self.graph.overlap, min_cov)
        g = copy.copy(self.graph)
        g.overlap = c["overlap"]
        g._member_offsets = None  # member offsets are not remapped onto the polished coordinates
        return PolishedSequences((c["out_off"], c["out"]), c["overlap"], c["pos_map"], c["stats"], g)


    def long_insertions(self, min_count=1):
        """the candidates voted so far -> [(pos, letters, count)] ascending by draft position, then by length and letters; pos is the
        position the letters would be inserted before"""
        if not self.long_ins:
            raise ValueError("long_insertions wants a Pileup made with long_ins=True")
        keys, counts = self.counter.finish(min_count=min_count)
        return decode_long_keys(keys.cpu().numpy().view(np.uint64), counts.cpu().numpy().view(np.uint32))


def decode_long_keys(keys, counts):
    """vote keys of long insertions (include/s2k.h: s2k_walks_pileup_ex) and their counts -> [(pos, letters, count)] sorted"""
    out = []
    for k, c in zip((int(x) for x in keys), (int(x) for x in counts)):
        rev, n = k >> 28, k >> 24 & 15
        pos = int(format(rev, "0%db" % LONG_INS_POS_BITS)[::-1], 2)
        out.append((pos, bytes(b"ACGT"[k >> (22 - 2 * i) & 3] for i in range(n)), c))
    return sorted(out)


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
