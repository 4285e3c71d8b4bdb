"""Rates of read threading on the device (s2k_unitig_node_places, s2k_table_thread), one process, one JSON file (default
profiles/thread_rate.json).  Times: median of --reps calls, HIP events on the engine's stream (each call ends in a host wait; the
events bracket the whole call).  Beside them, re-measured in the same job on the same input: s2k_table_edges (keys written), the
yardstick -- the same look-up and a compaction, without the 16-byte gather per solid item and the second mask -- and
s2k_table_filter (every output array).
  genome  : the genome-sampled set of tools/graph_rate.py (random 50 Mbp genome, 10 kbp reads at 30x, half reverse-complemented,
            Regular l=31 k=10 d=0.01): KminmerGraph.build(min_count 2) -> unitigs -> places -> thread.
  config1 : configs[1] (1 000 000 x 10 kbp synthetic reads, l=31 k=10 d=0.01, Hpc) against a table of every second key (min_count 1)
            over a decomposition of the table's nodes into unitigs of eight members: random reads, so nearly every solid item is a
            step of its own and the place array (16 B per node) is gathered at random.
Under `rocprofv3 --kernel-trace --stats` run it with --reps 3 --out /dev/null: the trace's per-kernel totals give the share of the
count pass (profiles/thread_kernel_stats.txt)."""
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


def legs(eng, torch, dev, pkg, table, items, n_reads, n, ug, min_count, reps, warmup):
    """places, thread (sizes only, writing), edges and filter on one input -> dict"""
    res = {"n_kminmers": n, "n_reads": n_reads, "table_keys": table.n, "n_unitigs": ug.n_unitigs, "place_bytes": 16 * table.n}
    _, ms = timed(torch, dev, lambda: eng.unitig_node_places(ug.uni_off, ug.members, ug.node_unitig, ug.node_pos, ug.circular), reps, warmup)
    res["node_places"] = summary(ms, table.n)
    place = ug.places(eng)
    i = pkg.DeviceOut()
    i.km_capacity = n
    for f in ("km_off", "hash", "rev", "start", "end"):
        if items.get(f) is not None:
            setattr(i, f, items[f].data_ptr())
    o = pkg.ThreadOut()
    path_off = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    o.path_off = path_off.data_ptr()
    ns = ctypes.c_uint64(0)
    call = lambda: eng._check(eng.lib.s2k_table_thread(table.handle, n_reads, ctypes.byref(i), min_count, place.data_ptr(), table.n,  # noqa: E731
                                                       ctypes.byref(o), None, ug.n_unitigs, ctypes.byref(ns)))
    torch.cuda.synchronize(dev)
    _, ms_s = timed(torch, dev, call, reps, warmup)
    res["thread_sizes_only"] = summary(ms_s, n)
    steps = int(ns.value)
    bufs = {f: torch.empty(max(steps, 1), dtype=torch.int32, device=dev) for f in pkg.ReadPaths.STEP_FIELDS if f not in ("start", "end") or items.get(f) is not None}
    o.capacity = steps
    for f, t in bufs.items():
        setattr(o, f, t.data_ptr())
    torch.cuda.synchronize(dev)
    _, ms_t = timed(torch, dev, call, reps, warmup)
    res["thread"] = summary(ms_t, n)
    res["thread"].update(n_steps=steps, n_solid=int(bufs["count"].sum()), arrays=sorted(bufs))
    del bufs
    cap = 2 * n
    ek = torch.empty(cap, dtype=torch.int64, device=dev)
    ne = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_table_edges(table.handle, n_reads, ctypes.byref(i), min_count, ek.data_ptr(), cap, ctypes.byref(ne)))  # noqa: E731
    _, ms_e = timed(torch, dev, fn, reps, warmup)
    res["edges"] = summary(ms_e, n)
    res["edges"]["n_edges"] = int(ne.value)
    del ek
    so = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(n, dtype=torch.int64, device=dev),
          "offset": torch.empty(n, dtype=torch.int32, device=dev), "count": torch.empty(n, dtype=torch.int32, device=dev)}
    for f, dt in (("start", torch.int32), ("end", torch.int32), ("rev", torch.uint8)):
        if items.get(f) is not None:
            so[f] = torch.empty(n, dtype=dt, device=dev)
    fo = pkg.SolidOut()
    fo.capacity = n
    for f, t in so.items():
        setattr(fo, f, t.data_ptr())
    nk = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_table_filter(table.handle, n_reads, ctypes.byref(i), min_count, ctypes.byref(fo), ctypes.byref(nk)))  # noqa: E731
    _, ms_f = timed(torch, dev, fn, reps, warmup)
    res["filter"] = summary(ms_f, n)
    res["filter"]["n_kept"] = int(nk.value)
    me = statistics.median(ms_e)
    res["thread_to_edges"] = round(statistics.median(ms_t) / me, 3)
    res["thread_sizes_only_to_edges"] = round(statistics.median(ms_s) / me, 3)
    res["thread_to_filter"] = round(statistics.median(ms_t) / statistics.median(ms_f), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-config1", action="store_true")
    ap.add_argument("--skip-genome", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thread_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "thread_rate", "reps": a.reps}

    if not a.skip_genome:
        bases, read_off, n_reads = genome_reads(torch, dev, 50_000_000, 10_000, 30, 7)
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
        n = c["n_kminmers"]
        graph = pkg.KminmerGraph.build(eng, [out], min_count=2)
        ug = graph.unitigs(eng)
        table = pkg.CountTable(eng, graph.keys, graph.counts)
        res["genome"] = legs(eng, torch, dev, pkg, table, out, n_reads, n, ug, 2, a.reps, a.warmup)
        table.close()
        del out, graph, ug, table
        torch.cuda.empty_cache()

    if not a.skip_config1:
        items, n_reads, n = config1(eng, torch, dev, pkg)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        nd, nk = eng.count_device_ex(items["hash"].data_ptr(), n, 1, True, keys.data_ptr(), counts.data_ptr(), n)
        half_k, half_c = keys[:nk:2].contiguous(), counts[:nk:2].contiguous()
        del keys, counts
        N = half_k.numel()
        T = (N + 7) // 8  # node i is member i % 8 of unitig i // 8, oriented by a bit of its index; every third unitig circular
        ids = torch.arange(N, dtype=torch.int64, device=dev)
        ug = pkg.UnitigGraph(torch.clamp(torch.arange(T + 1, dtype=torch.int64, device=dev) * 8, max=N),
                             (2 * ids + ((ids * 2654435761 >> 9) & 1)).to(torch.int32), (ids // 8).to(torch.int32), (ids % 8).to(torch.int32),
                             (torch.arange(T, device=dev) % 3 == 0).to(torch.uint8), None, None, None, None, None)
        del ids
        table = pkg.CountTable(eng, half_k, half_c)
        res["config1"] = legs(eng, torch, dev, pkg, table, items, n_reads, n, ug, 1, a.reps, a.warmup)
        table.close()

    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
