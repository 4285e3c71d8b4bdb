"""Rates of the path bridging on the device (s2k_paths_bridge, sizes only and writing), one process, one JSON file (default
profiles/bridge_rate.json).  Times: median of --reps calls, HIP events on the engine's stream (each call ends in a host wait; the
events bracket the whole call).  Beside them, re-measured in the same job on the same input: s2k_paths_spans (keys written), which
does the same one row search per step, and s2k_table_thread (every step array written), whose output both read.
  genome : the genome-sampled set of tools/graph_rate.py (random 50 Mbp genome, 10 kbp reads at 30x, half reverse-complemented, Regular
           l=31 k=10 d=0.01): KminmerGraph.build(min_count 2) -> unitigs -> thread -> bridge(16, 2).  The reads are error-free, so
           every join is an edge already followed and the output equals the input.  A random genome has no repeats: the graph is one
           unitig and a read is one step, so this leg is small and mostly the calls' fixed cost.
  genome_noisy : the same reads with --error-rate substitutions (default 0.5 %) threaded through the graph of the clean reads: many
           steps per read, nearly all of them merged (kind 1).  On one unitig there is no row to search, in the bridge or in the spans.
The ratio to watch is bridge / spans: the extra work is the second scan (over count) and eight arrays written instead of one."""
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
from table_rate import summary, timed  # noqa: E402


def legs(eng, torch, dev, pkg, graph, items, n_reads, n, min_count, reps, warmup, max_gap=16, max_slip=2):
    """graph: the KminmerGraph to thread through; items: the extraction outputs of the reads to thread, n k-min-mers"""
    ug = graph.unitigs(eng)
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, items, n_reads, min_count=min_count)
    ns, ne, t, nn = paths.n_steps, ug.n_edges, ug.n_unitigs, graph.n_nodes
    res = {"n_kminmers": n, "n_reads": n_reads, "n_nodes": nn, "n_unitigs": t, "n_edges": ne, "n_steps": ns, "max_gap": max_gap, "max_slip": max_slip}
    i = pkg.ThreadOut()
    i.capacity = ns
    for f in ("path_off",) + pkg.ReadPaths.STEP_FIELDS:
        setattr(i, f, getattr(paths, f).data_ptr())
    no, nm, nb = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    tail = (ctypes.byref(no), ctypes.byref(nm), ctypes.byref(nb))
    graph_args = (eng.ctx, n_reads, ctypes.byref(i), ns, ug.row_off.data_ptr(), ug.dst.data_ptr(), ne, ug.uni_off.data_ptr())
    args = graph_args + (ug.circular.data_ptr(), t, max_gap, max_slip)
    o = pkg.ThreadOut()
    bufs = {"path_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev)}
    o.path_off = bufs["path_off"].data_ptr()
    torch.cuda.synchronize(dev)
    _, ms_s = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_bridge(*args, ctypes.byref(o), None, None, *tail)), reps, warmup)
    res["bridge_sizes_only"] = summary(ms_s, ns)
    cap = int(no.value)
    o.capacity = cap
    for f in pkg.ReadPaths.STEP_FIELDS + ("matched",):
        bufs[f] = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        if f != "matched":
            setattr(o, f, bufs[f].data_ptr())
    bufs["join"] = torch.empty(max(ns, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_paths_bridge(*args, ctypes.byref(o), bufs["matched"].data_ptr(), bufs["join"].data_ptr(), *tail))  # noqa: E731
    _, ms_w = timed(torch, dev, fn, reps, warmup)
    res["bridge"] = summary(ms_w, ns)
    res["bridge"].update(n_out_steps=cap, n_merged=int(nm.value), n_bridged=int(nb.value))
    # the yardsticks on the same input
    nk, nf, nog = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    stail = (ctypes.byref(nk), ctypes.byref(nf), ctypes.byref(nog))
    eng._check(eng.lib.s2k_paths_spans(*graph_args, t, None, 0, None, *stail))
    kcap = int(nk.value)
    keys = torch.empty(max(kcap, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    _, ms_p = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_spans(*graph_args, t, keys.data_ptr(), kcap, None, *stail)), reps, warmup)
    res["spans"] = summary(ms_p, ns)
    d = pkg.DeviceOut()
    d.km_capacity = n
    d.km_off, d.hash, d.rev, d.start, d.end = (items[f].data_ptr() for f in ("km_off", "hash", "rev", "start", "end"))
    to = pkg.ThreadOut()
    tb = {f: torch.empty(max(ns, 1), dtype=torch.int32, device=dev) for f in pkg.ReadPaths.STEP_FIELDS}
    tb["path_off"] = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    to.capacity = ns
    for f, x in tb.items():
        setattr(to, f, x.data_ptr())
    place = ug.places(eng)
    n_st = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_table_thread(table.handle, n_reads, ctypes.byref(d), min_count, place.data_ptr(), table.n,  # noqa: E731
                                                     ctypes.byref(to), None, t, ctypes.byref(n_st)))
    _, ms_t = timed(torch, dev, fn, reps, warmup)
    res["thread"] = summary(ms_t, n)
    table.close()
    res["bridge_to_spans"] = round(statistics.median(ms_w) / statistics.median(ms_p), 3)
    res["bridge_sizes_only_to_spans"] = round(statistics.median(ms_s) / statistics.median(ms_p), 3)
    res["bridge_to_thread"] = round(statistics.median(ms_w) / statistics.median(ms_t), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-bases", type=int, default=50_000_000)
    ap.add_argument("--error-rate", type=float, default=0.005)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bridge_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "bridge_rate", "reps": a.reps}
    bases, read_off, n_reads = genome_reads(torch, dev, a.genome_bases, 10_000, 30, 7)
    n_bases = n_reads * 10_000
    cap = int(n_bases * 0.03)

    def extract(b):
        out = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev)}
        out["hash"] = torch.empty(cap, dtype=torch.int64, device=dev)
        out["rev"] = torch.empty(cap, dtype=torch.uint8, device=dev)
        for f in ("start", "end"):
            out[f] = torch.empty(cap, dtype=torch.int32, device=dev)
        o = pkg.DeviceOut()
        o.km_capacity = cap
        for f, x in out.items():
            setattr(o, f, x.data_ptr())
        torch.cuda.synchronize(dev)
        c = eng.extract_device(b.data_ptr(), read_off.data_ptr(), n_reads, n_bases, 31, 10, 0.01, int(pkg.HashMode.Regular), o)
        return out, c["n_kminmers"]

    out, n = extract(bases)
    graph = pkg.KminmerGraph.build(eng, [out], min_count=2)
    res["genome"] = legs(eng, torch, dev, pkg, graph, out, n_reads, n, 2, a.reps, a.warmup)
    res["genome"]["genome_bases"] = a.genome_bases
    # substitutions: a base becomes one of the three others
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    code = torch.zeros(256, dtype=torch.int64, device=dev)
    code[torch.tensor(list(b"ACGT"), device=dev)] = torch.arange(4, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    hit = torch.nonzero(torch.rand(n_bases, device=dev, generator=g) < a.error_rate).flatten()
    noisy = bases.clone()
    noisy[hit] = acgt[(code[bases[hit].long()] + torch.randint(1, 4, (hit.numel(),), device=dev, generator=g)) % 4]
    out2, n2 = extract(noisy)
    res["genome_noisy"] = legs(eng, torch, dev, pkg, graph, out2, n_reads, n2, 2, a.reps, a.warmup)
    res["genome_noisy"].update(genome_bases=a.genome_bases, error_rate=a.error_rate, substitutions=int(hit.numel()))
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
