"""Rates of the unitig compaction on the device (s2k_graph_unitigs, s2k_graph_unitig_edges), one process, one JSON file (default
profiles/unitig_rate.json).  Times of whole calls: median of --reps, HIP events on the engine's stream; times of the steps inside
s2k_graph_unitigs: the library's own host clock between the host waits that end them (s2k_graph_unitigs_last_steps, last rep).
  genome  : the genome-sampled set of tools/graph_rate.py (long chains: the worst case for the number of rounds).  Yardstick: the
            two-pass build in front of it (the sum of its five steps), measured here the way graph_rate.py does.
  config1 : configs[1] against a table of every second key (139.6 M oriented-node slots, short chains: the worst case for bytes per
            round).  Yardstick: the s2k_table_edges call of this run.
Bytes of a ranking round: per oriented node 8 B read + 8 B written, and for an unsettled one an 8-byte dependent load."""
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
from graph_rate import genome_reads, step_ms  # noqa: E402
from table_rate import HBM_PEAK, config1, summary, timed  # noqa: E402


def unitig_leg(eng, pkg, torch, dev, row_off, dst, n_nodes, reps, warmup):
    n, ne = int(n_nodes), dst.numel()
    res = {"uni_off": torch.empty(n + 1, dtype=torch.int64, device=dev), "members": torch.empty(n, dtype=torch.int32, device=dev),
           "node_unitig": torch.empty(n, dtype=torch.int32, device=dev), "node_pos": torch.empty(n, dtype=torch.int32, device=dev),
           "circular": torch.empty(n, dtype=torch.uint8, device=dev)}
    o = pkg.UnitigOut()
    o.capacity = n
    for f, t in res.items():
        setattr(o, f, t.data_ptr())
    nu, nl = ctypes.c_uint64(0), ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_graph_unitigs(eng.ctx, row_off.data_ptr(), dst.data_ptr(), ne, n, ctypes.byref(o), ctypes.byref(nu),  # noqa: E731
                                                      ctypes.byref(nl)))
    _, ms_u = timed(torch, dev, fn, reps, warmup)
    steps, rounds = (ctypes.c_double * 4)(), ctypes.c_uint32(0)
    eng.lib.s2k_graph_unitigs_last_steps(steps, ctypes.byref(rounds))
    t = int(nu.value)
    cap = ne - int(nl.value)
    keys = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    src = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    no = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_graph_unitig_edges(eng.ctx, row_off.data_ptr(), dst.data_ptr(), ne, n, res["uni_off"].data_ptr(),  # noqa: E731
                                                           res["members"].data_ptr(), res["node_unitig"].data_ptr(), res["node_pos"].data_ptr(), t,
                                                           keys.data_ptr(), src.data_ptr(), cap, ctypes.byref(no)))
    _, ms_e = timed(torch, dev, fn, reps, warmup)
    lens = (res["uni_off"][1:t + 1] - res["uni_off"][:t]).sort(descending=True).values
    half = int(torch.searchsorted(torch.cumsum(lens, 0), (n + 1) // 2))
    med_u, med_e = statistics.median(ms_u), statistics.median(ms_e)
    rank_ms = steps[1]
    round_bytes = 16 * 2 * n
    d = {"n_nodes": n, "n_oriented_nodes": 2 * n, "n_edges": ne, "n_unitigs": t, "n_links": int(nl.value), "n_unitig_edges": int(no.value),
         "n50_members": int(lens[half]) if t else 0, "longest_members": int(lens[0]) if t else 0, "circular": int(res["circular"][:t].sum()),
         "unitigs_call": summary(ms_u), "unitig_edges_call": summary(ms_e), "both_calls_ms": round(med_u + med_e, 4),
         "steps_ms": {"check": round(steps[0], 4), "link_and_ranking": round(steps[1], 4), "numbering": round(steps[2], 4),
                      "lengths_and_scatter": round(steps[3], 4), "unitig_edges": round(med_e, 4)},
         "rounds": int(rounds.value), "round_coalesced_bytes": round_bytes,
         "ranking_tb_per_s_coalesced_only": round(round_bytes * max(rounds.value, 1) / (rank_ms * 1e-3) / 1e12, 3) if rank_ms else None,
         "ranking_frac_of_8tb": round(round_bytes * max(rounds.value, 1) / (rank_ms * 1e-3) / HBM_PEAK, 3) if rank_ms else None}
    return d


def verdict(ms, yard):
    return "target met" if ms <= yard else "missed by x%.2f" % (ms / yard)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-config1", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "unitig_rate", "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK}

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
    steps = {}
    for rep in range(2):  # the first round warms up; the second is reported (as tools/graph_rate.py)
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
    gen = unitig_leg(eng, pkg, torch, dev, row_off, dst, keys.numel(), a.reps, a.warmup)
    gen["build_steps_ms"] = steps
    gen["both_calls_to_build"] = round(gen["both_calls_ms"] / steps["total"], 3)
    gen["verdict"] = verdict(gen["both_calls_ms"], steps["total"])
    res["genome"] = gen
    del out, e, ek, ec, row_off, dst, keys, counts
    torch.cuda.empty_cache()

    if not a.skip_config1:
        items, n_reads, n = config1(eng, torch, dev, pkg)
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        nd, nk = eng.count_device_ex(items["hash"].data_ptr(), n, 1, True, keys.data_ptr(), counts.data_ptr(), n)
        half_k, half_c = keys[:nk:2].contiguous(), counts[:nk:2].contiguous()
        del keys, counts
        half = pkg.CountTable(eng, half_k, half_c)
        i = pkg.DeviceOut()
        i.km_capacity = n
        for f in ("km_off", "hash", "start", "end", "rev"):
            setattr(i, f, items[f].data_ptr())
        cap = 2 * n
        ek = torch.empty(cap, dtype=torch.int64, device=dev)
        ne = ctypes.c_uint64(0)
        torch.cuda.synchronize(dev)
        fn = lambda: eng._check(eng.lib.s2k_table_edges(half.handle, n_reads, ctypes.byref(i), 1, ek.data_ptr(), cap, ctypes.byref(ne)))  # noqa: E731
        _, ms_e = timed(torch, dev, fn, a.reps, a.warmup)
        half.close()
        n_nodes = half_k.numel()
        ne = int(ne.value)
        del items, half_k, half_c
        dk = torch.empty(ne, dtype=torch.int64, device=dev)
        dc = torch.empty(ne, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        _, n_distinct = eng.count_device_ex(ek.data_ptr(), ne, 1, True, dk.data_ptr(), dc.data_ptr(), ne)
        del ek, dc
        row_off, dst = eng.graph_adjacency(dk[:n_distinct], n_nodes)
        del dk
        torch.cuda.empty_cache()
        c1 = unitig_leg(eng, pkg, torch, dev, row_off, dst, n_nodes, a.reps, a.warmup)
        c1["table_edges_call"] = summary(ms_e)
        c1["both_calls_to_table_edges"] = round(c1["both_calls_ms"] / statistics.median(ms_e), 3)
        c1["verdict"] = verdict(c1["both_calls_ms"], statistics.median(ms_e))
        res["config1"] = c1
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
