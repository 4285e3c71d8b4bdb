"""Rates of the junction spans on the device (s2k_paths_spans, sizes only and writing, and s2k_graph_resolve_mask), one process, one
JSON file (default profiles/span_rate.json).  Times: median of --reps calls, HIP events on the engine's stream (each call ends in a
host wait; the events bracket the whole call).  Beside them, re-measured in the same job on the same input: s2k_table_thread (every
step array written), whose output the spans read, and s2k_table_edges (keys written), the pass the spans pass was modelled on.
  genome  : the genome-sampled set of tools/graph_rate.py (random 50 Mbp genome, 10 kbp reads at 30x, half reverse-complemented,
            Regular l=31 k=10 d=0.01): KminmerGraph.build(min_count 2) -> unitigs -> thread -> spans -> span table -> resolve.
  config1 : (--config1; off by default, it builds a graph of more than 10^8 nodes) configs[1], 1 000 000 x 10 kbp synthetic reads,
            l=31 k=10 d=0.01, Hpc, min_count 1: random reads, so nearly every node is a unitig of its own and every step follows an
            edge found at random in the CSR.
Under `rocprofv3 --kernel-trace --stats` run it with --reps 3 --out /dev/null: the trace's per-kernel totals give the share of the
count pass."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from graph_rate import genome_reads  # noqa: E402
from s2k_loader import import_package  # noqa: E402
from table_rate import config1, summary, timed  # noqa: E402


def legs(eng, torch, dev, pkg, items, n_reads, n, min_count, reps, warmup):
    """graph -> unitigs -> paths, then spans (sizes only, writing), the resolution, thread and edges on one input -> dict"""
    graph = pkg.KminmerGraph.build(eng, [items], min_count=min_count)
    ug = graph.unitigs(eng)
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, items, n_reads, min_count=min_count)
    ns, ne, t = paths.n_steps, ug.n_edges, ug.n_unitigs
    res = {"n_kminmers": n, "n_reads": n_reads, "n_nodes": graph.n_nodes, "n_unitigs": t, "n_edges": ne, "n_steps": ns}
    o = pkg.ThreadOut()
    o.capacity = ns
    for f in ("path_off", "unitig", "pos", "count", "flags"):
        setattr(o, f, getattr(paths, f).data_ptr())
    nk, nf, no = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    args = (eng.ctx, n_reads, ctypes.byref(o), ns, ug.row_off.data_ptr(), ug.dst.data_ptr(), ne, ug.uni_off.data_ptr(), t)
    tail = (ctypes.byref(nk), ctypes.byref(nf), ctypes.byref(no))
    torch.cuda.synchronize(dev)
    _, ms_s = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_spans(*args, None, 0, None, *tail)), reps, warmup)
    res["spans_sizes_only"] = summary(ms_s, ns)
    cap = int(nk.value)
    keys = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    sup = torch.zeros(max(ne, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    _, ms_w = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_spans(*args, keys.data_ptr(), cap, None, *tail)), reps, warmup)
    res["spans"] = summary(ms_w, ns)
    res["spans"].update(n_keys=cap, n_followed=int(nf.value), n_off_graph=int(no.value))
    _, ms_u = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_spans(*args, keys.data_ptr(), cap, sup.data_ptr(), *tail)), reps, warmup)
    res["spans_with_edge_support"] = summary(ms_u, ns)
    st = ug.span_table(eng, [paths])
    nc, nr = ctypes.c_uint64(0), ctypes.c_uint64(0)
    resolved = torch.zeros(max(t, 1), dtype=torch.uint8, device=dev)
    partner = torch.empty(max(ne, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_graph_resolve_mask(eng.ctx, ug.row_off.data_ptr(), ug.dst.data_ptr(), ne, t, st.keys.data_ptr(),  # noqa: E731
                                                           st.counts.data_ptr(), st.n_spans, 2, resolved.data_ptr(), partner.data_ptr(),
                                                           ctypes.byref(nc), ctypes.byref(nr)))
    _, ms_r = timed(torch, dev, fn, reps, warmup)
    res["resolve"] = summary(ms_r, 2 * t)
    res["resolve"].update(n_spans=st.n_spans, n_candidates=int(nc.value), n_resolved=int(nr.value))
    # the yardsticks on the same input
    i = pkg.DeviceOut()
    i.km_capacity = n
    i.km_off, i.hash, i.rev = (items[f].data_ptr() for f in ("km_off", "hash", "rev"))
    to = pkg.ThreadOut()
    bufs = {f: torch.empty(max(ns, 1), dtype=torch.int32, device=dev) for f in ("unitig", "pos", "count", "item", "flags")}
    bufs["path_off"] = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    to.capacity = ns
    for f, x in bufs.items():
        setattr(to, f, x.data_ptr())
    place = ug.places(eng)
    n_st = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_table_thread(table.handle, n_reads, ctypes.byref(i), min_count, place.data_ptr(), table.n,  # noqa: E731
                                                     ctypes.byref(to), None, t, ctypes.byref(n_st)))
    _, ms_t = timed(torch, dev, fn, reps, warmup)
    res["thread"] = summary(ms_t, n)
    del bufs
    ek = torch.empty(2 * n, dtype=torch.int64, device=dev)
    n_e = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_table_edges(table.handle, n_reads, ctypes.byref(i), min_count, ek.data_ptr(), 2 * n, ctypes.byref(n_e)))  # noqa: E731
    _, ms_e = timed(torch, dev, fn, reps, warmup)
    res["edges"] = summary(ms_e, n)
    table.close()
    res["spans_to_thread"] = round(statistics.median(ms_w) / statistics.median(ms_t), 3)
    res["spans_sizes_only_to_thread"] = round(statistics.median(ms_s) / statistics.median(ms_t), 3)
    res["spans_to_edges"] = round(statistics.median(ms_w) / statistics.median(ms_e), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config1", action="store_true")
    ap.add_argument("--skip-genome", action="store_true")
    ap.add_argument("--genome-bases", type=int, default=50_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "span_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "span_rate", "reps": a.reps}

    if not a.skip_genome:
        bases, read_off, n_reads = genome_reads(torch, dev, a.genome_bases, 10_000, 30, 7)
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
        res["genome"]["genome_bases"] = a.genome_bases
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
