"""Rates of the graph construction on the device (s2k_table_edges, s2k_graph_adjacency, KminmerGraph.build's steps), one process, one
JSON file (default profiles/graph_rate.json).  Times: median of --reps calls, HIP events on the engine's stream (each call ends in a
host wait; the events bracket the whole call).
  config1 : configs[1] (1 000 000 x 10 kbp synthetic reads, l=31 k=10 d=0.01, Hpc): its 139.6 M k-min-mers against a table of every
            second key (min_count 1), the input of tools/table_rate.py's filter leg.  s2k_table_filter with every output array beside
            s2k_table_edges with its keys written; then the CSR of the sorted distinct edge keys (s2k_graph_adjacency).
  genome  : a random 50 Mbp genome drawn on the device, 10 kbp reads at 30x coverage, half of them reverse-complemented, Regular,
            l=31 k=10 d=0.01: each step of the two-pass build (count nodes, index the table, emit edges, count edges, adjacency), the
            node and edge counts, and the fraction of oriented nodes with out-degree <= 1.
Adjacency: algorithmic bytes = 8 B per edge read + 4 B per edge and 8 B per row offset written, against 8 TB/s."""
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
from table_rate import HBM_PEAK, config1, summary, timed  # noqa: E402


def adjacency_leg(eng, torch, dev, edge_keys, n_nodes, reps, warmup):
    n = edge_keys.numel()
    row_off = torch.empty(2 * n_nodes + 1, dtype=torch.int64, device=dev)
    dst = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_graph_adjacency(eng.ctx, edge_keys.data_ptr(), n, n_nodes, row_off.data_ptr(), dst.data_ptr()))  # noqa: E731
    _, ms = timed(torch, dev, fn, reps, warmup)
    d = summary(ms)
    alg = 8 * n + 4 * n + 8 * (2 * n_nodes + 1)
    d.update(n_edges=n, n_oriented_nodes=2 * n_nodes, alg_bytes=alg, tb_per_s=round(alg / (statistics.median(ms) * 1e-3) / 1e12, 3),
             frac_of_8tb=round(alg / (statistics.median(ms) * 1e-3) / HBM_PEAK, 3))
    return d, row_off


def genome_reads(torch, dev, genome_bp, read_len, coverage, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    comp = torch.zeros(256, dtype=torch.uint8, device=dev)
    comp[acgt.long()] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    genome = acgt[torch.randint(0, 4, (genome_bp,), device=dev, generator=g)]
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


def step_ms(torch, dev, fn):
    st = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    r = fn()
    e1.record(st)
    e1.synchronize()
    return r, round(e0.elapsed_time(e1), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-config1", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "graph_rate", "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK}

    if not a.skip_config1:
        items, n_reads, n = config1(eng, torch, dev, pkg)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        nd, nk = eng.count_device_ex(items["hash"].data_ptr(), n, 1, True, keys.data_ptr(), counts.data_ptr(), n)
        half_k, half_c = keys[:nk:2].contiguous(), counts[:nk:2].contiguous()
        del keys, counts
        half = pkg.CountTable(eng, half_k, half_c)
        c1 = {"n_kminmers": n, "n_reads": n_reads, "table_keys": half.n}
        so = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(n, dtype=torch.int64, device=dev),
              "start": torch.empty(n, dtype=torch.int32, device=dev), "end": torch.empty(n, dtype=torch.int32, device=dev),
              "rev": torch.empty(n, dtype=torch.uint8, device=dev), "offset": torch.empty(n, dtype=torch.int32, device=dev),
              "count": torch.empty(n, dtype=torch.int32, device=dev)}
        i, o = pkg.DeviceOut(), pkg.SolidOut()
        i.km_capacity = n
        for f in ("km_off", "hash", "start", "end", "rev"):
            setattr(i, f, items[f].data_ptr())
        o.capacity = n
        for f, t in so.items():
            setattr(o, f, t.data_ptr())
        nkept = ctypes.c_uint64(0)
        torch.cuda.synchronize(dev)
        fn = lambda: eng._check(eng.lib.s2k_table_filter(half.handle, n_reads, ctypes.byref(i), 1, ctypes.byref(o), ctypes.byref(nkept)))  # noqa: E731
        _, ms_f = timed(torch, dev, fn, a.reps, a.warmup)
        c1["filter_half_table"] = summary(ms_f, n)
        c1["filter_half_table"]["n_kept"] = int(nkept.value)
        del so
        cap = 2 * n
        ek = torch.empty(cap, dtype=torch.int64, device=dev)
        ne = ctypes.c_uint64(0)
        torch.cuda.synchronize(dev)
        fn = lambda: eng._check(eng.lib.s2k_table_edges(half.handle, n_reads, ctypes.byref(i), 1, ek.data_ptr(), cap, ctypes.byref(ne)))  # noqa: E731
        _, ms_e = timed(torch, dev, fn, a.reps, a.warmup)
        c1["edges_half_table"] = summary(ms_e, n)
        c1["edges_half_table"]["n_edges"] = int(ne.value)
        c1["edges_to_filter"] = round(statistics.median(ms_e) / statistics.median(ms_f), 3)
        half.close()
        ne = int(ne.value)
        dk = torch.empty(ne, dtype=torch.int64, device=dev)
        dc = torch.empty(ne, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        _, n_distinct = eng.count_device_ex(ek.data_ptr(), ne, 1, True, dk.data_ptr(), dc.data_ptr(), ne)
        del ek
        c1["adjacency"], _ = adjacency_leg(eng, torch, dev, dk[:n_distinct], half_k.numel(), a.reps, a.warmup)
        res["config1"] = c1
        del items, dk, dc, half_k, half_c
        torch.cuda.empty_cache()

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
    gen = {"genome_bp": 50_000_000, "read_len": 10_000, "coverage": 30, "n_reads": n_reads, "n_kminmers": n, "steps_ms": {}}
    steps = gen["steps_ms"]
    for rep in range(2):  # the first round warms up; the second is reported
        ctr = pkg.KminmerCounter(eng)
        (keys, counts), t_nodes = step_ms(torch, dev, lambda: (ctr.add(out["hash"].data_ptr(), n), ctr.finish(2))[1])
        ctr.close()
        table, t_index = step_ms(torch, dev, lambda: pkg.CountTable(eng, keys, counts))
        e, t_edges = step_ms(torch, dev, lambda: table.edges(out, n_reads, 2))
        table.close()
        ectr = pkg.KminmerCounter(eng)
        (ek, ec), t_ecount = step_ms(torch, dev, lambda: (ectr.add(e.data_ptr(), e.numel()), ectr.finish(1))[1])
        ectr.close()
        (row_off, dst), t_adj = step_ms(torch, dev, lambda: eng.graph_adjacency(ek, keys.numel()))
        steps.update(count_nodes=t_nodes, index_table=t_index, emit_edges=t_edges, count_edges=t_ecount, adjacency=t_adj)
    steps["total"] = round(sum(steps.values()), 4)
    deg = row_off[1:] - row_off[:-1]
    gen.update(n_nodes=keys.numel(), n_edge_keys_emitted=e.numel(), n_edges=ek.numel(), frac_out_degree_le_1=round(float((deg <= 1).double().mean()), 6),
               max_out_degree=int(deg.max()) if deg.numel() else 0)
    gen["adjacency"], _ = adjacency_leg(eng, torch, dev, ek, keys.numel(), a.reps, a.warmup)
    res["genome"] = gen
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
