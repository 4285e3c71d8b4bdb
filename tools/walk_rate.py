"""Rates of the read walks on the device (s2k_paths_walks, sizes only and writing, and s2k_unitig_member_offsets), one process, one JSON
file (default profiles/walk_rate.json).  Times: median of --reps calls, HIP events on the engine's stream (each call ends in a host
wait; the events bracket the whole call).  Beside them, re-measured in the same job on the same input: s2k_paths_spans (keys written),
which does the same row searches, and s2k_table_thread (every step array written), whose output both read.
  genome : the genome-sampled set of tools/graph_rate.py (random 50 Mbp genome, 10 kbp reads at 30x, half reverse-complemented, Regular
           l=31 k=10 d=0.01): KminmerGraph.build(min_count 2) -> unitigs -> node sequences -> thread -> member offsets -> walks.
The ratio to watch is walks / spans: the extra work is two scans over the steps and a gather per walk."""
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


def legs(eng, torch, dev, pkg, items, n_reads, n, min_count, reps, warmup):
    graph = pkg.KminmerGraph.build(eng, [items], min_count=min_count)
    ug = graph.unitigs(eng)
    ns_ = pkg.NodeSequences.build(eng, graph, [items])
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, items, n_reads, min_count=min_count)
    ns, ne, t, nn = paths.n_steps, ug.n_edges, ug.n_unitigs, graph.n_nodes
    res = {"n_kminmers": n, "n_reads": n_reads, "n_nodes": nn, "n_unitigs": t, "n_edges": ne, "n_steps": ns}
    _, ms_m = timed(torch, dev, lambda: eng.unitig_member_offsets(ug.uni_off, ug.members, ug.circular, nn, ns_), reps, warmup)
    res["member_offsets"] = summary(ms_m, nn)
    member_off, out_off, overlap, _ = ug.member_offsets(eng, ns_)
    o = pkg.ThreadOut()
    o.capacity = ns
    for f in ("path_off", "unitig", "pos", "count", "flags", "start", "end"):
        setattr(o, f, getattr(paths, f).data_ptr())
    nw, nf, no = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    tail = (ctypes.byref(nw), ctypes.byref(nf), ctypes.byref(no))
    graph_args = (eng.ctx, n_reads, ctypes.byref(o), ns, ug.row_off.data_ptr(), ug.dst.data_ptr(), ne, ug.uni_off.data_ptr())
    args = graph_args + (ug.circular.data_ptr(), t, member_off.data_ptr(), out_off.data_ptr(), overlap.data_ptr(), ns_.seq_len.data_ptr(),
                         ug.members.data_ptr(), nn)
    torch.cuda.synchronize(dev)
    _, ms_s = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_walks(*args, None, *tail)), reps, warmup)
    res["walks_sizes_only"] = summary(ms_s, ns)
    cap = int(nw.value)
    w = pkg.WalkOut()
    w.capacity = cap
    bufs = {f: torch.empty(max(cap, 1), dtype=torch.int64, device=dev) for f in ("first_step", "items", "path_len", "path_start", "path_end")}
    bufs.update({f: torch.empty(max(cap, 1), dtype=torch.int32, device=dev) for f in ("n_steps", "qstart", "qend", "flags")})
    bufs["walk_off"] = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    bufs["edge"] = torch.empty(max(ns, 1), dtype=torch.int32, device=dev)
    for f, x in bufs.items():
        setattr(w, f, x.data_ptr())
    torch.cuda.synchronize(dev)
    _, ms_w = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_walks(*args, ctypes.byref(w), *tail)), reps, warmup)
    res["walks"] = summary(ms_w, ns)
    res["walks"].update(n_walks=cap, n_followed=int(nf.value), n_off_graph=int(no.value))
    # the yardsticks on the same input
    nk = ctypes.c_uint64(0)
    stail = (ctypes.byref(nk), ctypes.byref(nf), ctypes.byref(no))
    eng._check(eng.lib.s2k_paths_spans(*graph_args, t, None, 0, None, *stail))
    kcap = int(nk.value)
    keys = torch.empty(max(kcap, 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    _, ms_p = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_spans(*graph_args, t, keys.data_ptr(), kcap, None, *stail)), reps, warmup)
    res["spans"] = summary(ms_p, ns)
    i = pkg.DeviceOut()
    i.km_capacity = n
    i.km_off, i.hash, i.rev, i.start, i.end = (items[f].data_ptr() for f in ("km_off", "hash", "rev", "start", "end"))
    to = pkg.ThreadOut()
    tb = {f: torch.empty(max(ns, 1), dtype=torch.int32, device=dev) for f in ("unitig", "pos", "count", "item", "flags", "start", "end")}
    tb["path_off"] = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    to.capacity = ns
    for f, x in tb.items():
        setattr(to, f, x.data_ptr())
    place = ug.places(eng)
    n_st = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_table_thread(table.handle, n_reads, ctypes.byref(i), min_count, place.data_ptr(), table.n,  # noqa: E731
                                                     ctypes.byref(to), None, t, ctypes.byref(n_st)))
    _, ms_t = timed(torch, dev, fn, reps, warmup)
    res["thread"] = summary(ms_t, n)
    table.close()
    res["walks_to_spans"] = round(statistics.median(ms_w) / statistics.median(ms_p), 3)
    res["walks_sizes_only_to_spans"] = round(statistics.median(ms_s) / statistics.median(ms_p), 3)
    res["walks_to_thread"] = round(statistics.median(ms_w) / statistics.median(ms_t), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-bases", type=int, default=50_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "walk_rate", "reps": a.reps}
    bases, read_off, n_reads = genome_reads(torch, dev, a.genome_bases, 10_000, 30, 7)
    n_bases = n_reads * 10_000
    cap = int(n_bases * 0.03)
    out = {f: torch.empty(n_reads + 1, dtype=torch.int64, device=dev) for f in ("km_off", "mn_off")}
    out["hash"] = torch.empty(cap, dtype=torch.int64, device=dev)
    out["rev"] = torch.empty(cap, dtype=torch.uint8, device=dev)
    for f in ("start", "end", "mn_j", "mn_jend", "mn_hash"):
        out[f] = torch.empty(cap, dtype=torch.int32, device=dev)
    o = pkg.DeviceOut()
    o.km_capacity = o.mn_capacity = cap
    for f, x in out.items():
        setattr(o, f, x.data_ptr())
    torch.cuda.synchronize(dev)
    c = eng.extract_device(bases.data_ptr(), read_off.data_ptr(), n_reads, n_bases, 31, 10, 0.01, int(pkg.HashMode.Regular), o,
                           flags=pkg.FLAG_WANT_MINIMIZERS)
    out["bases"], out["read_off"] = bases, read_off
    res["genome"] = legs(eng, torch, dev, pkg, out, n_reads, c["n_kminmers"], 2, a.reps, a.warmup)
    res["genome"]["genome_bases"] = a.genome_bases
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
