"""Rates of the untangling on the device (s2k_graph_untangle, sizes only and writing, and s2k_unitig_expand), one process, one JSON
file (default profiles/untangle_rate.json).  Times: median of --reps calls, HIP events on the engine's stream (each call ends in a
host wait; the events bracket the whole call).  Beside them, re-measured in the same job on the same graph: s2k_graph_unitigs +
s2k_graph_unitig_edges, the compaction that the untangled graph goes through next; the expectation is that both new calls together
cost less than that.
  genome  : the genome-sampled set of tools/graph_rate.py (random 50 Mbp genome, 10 kbp reads at 30x, half reverse-complemented,
            Regular l=31 k=10 d=0.01) with --repeats segments of --repeat-bases bases each copied to a second place of the genome
            before the reads are drawn, so that reads span the repeats: KminmerGraph.build(min_count 2) -> unitigs -> thread -> span
            table -> resolve -> untangle -> expand.
  config1 : (--config1; off by default, it builds a graph of more than 10^8 nodes) configs[1], 1 000 000 x 10 kbp synthetic reads,
            l=31 k=10 d=0.01, Hpc, min_count 1: random reads, nothing to resolve -- the identity, at the largest size."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from s2k_loader import import_package  # noqa: E402
from table_rate import config1, summary, timed  # noqa: E402


def genome_reads_with_repeats(torch, dev, genome_bp, read_len, coverage, seed, repeats, repeat_bp):
    """genome_reads of tools/graph_rate.py, with `repeats` segments copied inside the genome before the reads are drawn"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp[acgt.long()] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    genome = acgt[torch.randint(0, 4, (genome_bp,), device=dev, generator=g)]
    slot = genome_bp // (2 * max(repeats, 1))  # repeat i: from the start of slot 2 i to the start of slot 2 i + 1
    for i in range(repeats):
        genome[(2 * i + 1) * slot: (2 * i + 1) * slot + repeat_bp] = genome[2 * i * slot: 2 * i * slot + repeat_bp].clone()
    n_reads = genome_bp * coverage // read_len
    starts = torch.randint(0, genome_bp - read_len + 1, (n_reads,), device=dev, generator=g)
    bases = torch.empty(n_reads * read_len + 64, dtype=torch.uint8, device=dev)
    ar = torch.arange(read_len, device=dev)
    step = 8192
    for a in range(0, n_reads, step):
        b = min(a + step, n_reads)
        r = genome[starts[a:b, None] + ar]
        rc = comp[r.flip(1).long()]
        r[1::2] = rc[1::2]  # every second read from the other strand
        bases[a * read_len: b * read_len] = r.reshape(-1)
    read_off = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * read_len
    return bases, read_off, n_reads


def legs(eng, torch, dev, pkg, items, n_reads, n, min_count, reps, warmup):
    """graph -> unitigs -> paths -> resolution, then untangle (sizes only, writing), expand, and the compaction of the same graph"""
    graph = pkg.KminmerGraph.build(eng, [items], min_count=min_count)
    ug = graph.unitigs(eng)
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, items, n_reads, min_count=min_count)
    table.close()
    resolved, partner, stats = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    del paths
    t, ne = ug.n_unitigs, ug.n_edges
    res = {"n_kminmers": n, "n_reads": n_reads, "n_nodes": graph.n_nodes, "n_unitigs": t, "n_edges": ne, "n_candidates": stats["candidates"],
           "n_resolved": stats["resolved"]}
    nc, nd = ctypes.c_uint64(0), ctypes.c_uint64(0)
    args = (eng.ctx, ug.row_off.data_ptr(), ug.dst.data_ptr(), ne, t, resolved.data_ptr(), partner.data_ptr(), ug.counts.data_ptr(),
            ug.edge_counts.data_ptr())
    tail = (ctypes.byref(nc), ctypes.byref(nd))
    torch.cuda.synchronize(dev)
    _, ms_s = timed(torch, dev, lambda: eng._check(eng.lib.s2k_graph_untangle(*args, None, None, None, None, None, 0, *tail)), reps, warmup)
    res["untangle_sizes_only"] = summary(ms_s, 2 * t)
    tc = int(nc.value)
    copy_off = torch.empty(t + 1, dtype=torch.int64, device=dev)
    origin = torch.empty(max(tc, 1), dtype=torch.int32, device=dev)
    copy_count = torch.empty(max(tc, 1), dtype=torch.int64, device=dev)
    keys, src = torch.empty(max(ne, 1), dtype=torch.int64, device=dev), torch.empty(max(ne, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_graph_untangle(*args, copy_off.data_ptr(), origin.data_ptr(), copy_count.data_ptr(), keys.data_ptr(),  # noqa: E731
                                                       src.data_ptr(), tc, *tail))
    _, ms_u = timed(torch, dev, fn, reps, warmup)
    res["untangle"] = summary(ms_u, 2 * tc)
    res["untangle"].update(n_copies=tc, n_duplicated=int(nd.value))
    # the compaction of the untangled graph: the input of the expansion
    row_off, dst = eng.graph_adjacency(keys[:ne], tc)
    o = eng.graph_unitigs(row_off, dst, tc)
    nm = ctypes.c_uint64(0)
    eargs = (eng.ctx, o["uni_off"].data_ptr(), o["members"].data_ptr(), o["circular"].data_ptr(), o["n_unitigs"], tc, origin.data_ptr(),
             ug.uni_off.data_ptr(), ug.members.data_ptr(), ug.circular.data_ptr(), t, graph.n_nodes)
    torch.cuda.synchronize(dev)
    eng._check(eng.lib.s2k_unitig_expand(*eargs, None, None, None, None, None, None, 0, ctypes.byref(nm)))
    m = int(nm.value)
    out = [torch.empty(o["n_unitigs"] + 1, dtype=torch.int64, device=dev)] + [torch.empty(max(m, 1), dtype=torch.int32, device=dev) for _ in range(3)]
    out += [torch.empty(max(o["n_unitigs"], 1), dtype=torch.uint8, device=dev), torch.empty(max(m, 1), dtype=torch.int32, device=dev)]
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_unitig_expand(*eargs, *(x.data_ptr() for x in out), m, ctypes.byref(nm)))  # noqa: E731
    _, ms_x = timed(torch, dev, fn, reps, warmup)
    res["expand"] = summary(ms_x, m)
    res["expand"].update(n_contigs=o["n_unitigs"], n_members=m)
    del out
    # the yardstick: the compaction of the graph the untangling started from, unitigs and their edges
    def compaction():
        u = eng.graph_unitigs(graph.row_off, graph.dst, graph.n_nodes)
        eng.graph_unitig_edges(graph.row_off, graph.dst, graph.n_nodes, u)

    _, ms_c = timed(torch, dev, compaction, reps, warmup)
    res["unitigs_and_edges"] = summary(ms_c, 2 * graph.n_nodes)
    both = statistics.median(ms_u) + statistics.median(ms_x)
    res["untangle_plus_expand_to_compaction"] = round(both / statistics.median(ms_c), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config1", action="store_true")
    ap.add_argument("--skip-genome", action="store_true")
    ap.add_argument("--genome-bases", type=int, default=50_000_000)
    ap.add_argument("--repeats", type=int, default=1000)
    ap.add_argument("--repeat-bases", type=int, default=3000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "untangle_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "untangle_rate", "reps": a.reps}

    if not a.skip_genome:
        bases, read_off, n_reads = genome_reads_with_repeats(torch, dev, a.genome_bases, 10_000, 30, 7, a.repeats, a.repeat_bases)
        n_bases = n_reads * 10_000
        cap = int(n_bases * 0.03)
        out = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
               "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
        o = pkg.DeviceOut()
        o.km_capacity = cap
        o.km_off, o.hash, o.rev = (out[x].data_ptr() for x in ("km_off", "hash", "rev"))
        torch.cuda.synchronize(dev)
        c = eng.extract_device(bases.data_ptr(), read_off.data_ptr(), n_reads, n_bases, 31, 10, 0.01, int(pkg.HashMode.Regular), o)
        del bases
        res["genome"] = legs(eng, torch, dev, pkg, out, n_reads, c["n_kminmers"], 2, a.reps, a.warmup)
        res["genome"].update(genome_bases=a.genome_bases, repeats=a.repeats, repeat_bases=a.repeat_bases)
        del out
        torch.cuda.empty_cache()

    if a.config1:
        items, n_reads, n = config1(eng, torch, dev, pkg)
        res["config1"] = legs(eng, torch, dev, pkg, items, n_reads, n, 1, a.reps, a.warmup)

    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
