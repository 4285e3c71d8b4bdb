"""Rates of the graph simplification on the device (s2k_graph_simplify_mask, s2k_graph_induced), one process, one JSON file (default
profiles/simplify_rate.json).  Per round, in the same job: the time of the mask call and of the induced call beside the time of the
compaction they follow (s2k_graph_unitigs + s2k_graph_unitig_edges + s2k_graph_adjacency of the same round), each the median of
--reps, HIP events on the engine's stream around the Engine method (its output allocations included, on both sides).
  genome  : the genome-sampled set of tools/graph_rate.py with substitutions injected by a torch step (--rate per base), so that
            there are tips and bubbles to remove.
  config1 : configs[1] against a table of every second key, as tools/unitig_rate.py builds it (short chains, many dead ends).
Tips hold at most 2 k members, bubble branches at most 4 k; both sets are extracted with l = 31, k = 10 (here, and in
tools/table_rate.py:config1), K below.
Expectation to confirm or refute: mask + induced cost less than the compaction of their round."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from s2k_loader import import_package  # noqa: E402
from graph_rate import genome_reads  # noqa: E402
from table_rate import config1, timed  # noqa: E402


K = 10  # the k-min-mer order of both sets


def inject_substitutions(torch, dev, bases, n, rate, seed):
    """every one of the first n bases becomes one of the three other letters with probability `rate`, in place"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    code = torch.zeros(256, dtype=torch.int64, device=dev)
    code[acgt.long()] = torch.arange(4, device=dev)
    step = 1 << 28
    total = 0
    for a in range(0, n, step):
        b = min(a + step, n)
        hit = torch.nonzero(torch.rand(b - a, device=dev, generator=g) < rate)[:, 0] + a
        bases[hit] = acgt[(code[bases[hit].long()] + torch.randint(1, 4, (hit.numel(),), device=dev, generator=g)) % 4]
        total += hit.numel()
    return total


def rounds_leg(eng, pkg, torch, dev, graph, max_tip, max_bubble, max_rounds, reps, warmup):
    med = lambda fn: (lambda r, ms: (r, statistics.median(ms)))(*timed(torch, dev, fn, reps, warmup))  # noqa: E731
    out, g = [], graph
    for _ in range(max_rounds):
        n = g.n_nodes
        u, t_uni = med(lambda: eng.graph_unitigs(g.row_off, g.dst, n))
        (ek, src), t_edges = med(lambda: eng.graph_unitig_edges(g.row_off, g.dst, n, u))
        (uro, ud), t_adj = med(lambda: eng.graph_adjacency(ek, u["n_unitigs"]))
        del u, ek, src, uro, ud
        ug = g.unitigs(eng)  # the same three calls once more, untimed, with the unitig counts
        m, t_mask = med(lambda: eng.graph_simplify_mask(ug, max_tip, max_bubble))
        lens = ug.uni_off[1:] - ug.uni_off[:-1]
        d = {"nodes": n, "edges": g.n_edges, "unitigs": ug.n_unitigs, "unitig_edges": ug.n_edges, "longest_members": int(lens.max()) if n else 0,
             "tips": m["n_tips"], "bubbles": m["n_bubbles"], "removed": m["n_removed"],
             "unitigs_ms": round(t_uni, 4), "unitig_edges_ms": round(t_edges, 4), "unitig_adjacency_ms": round(t_adj, 4),
             "compaction_ms": round(t_uni + t_edges + t_adj, 4), "mask_ms": round(t_mask, 4)}
        if m["n_removed"] == 0:
            out.append(d)
            break
        ind, t_ind = med(lambda: eng.graph_induced(g, node_unitig=ug.node_unitig, remove=m["remove"]))
        (ro, dst), t_adj2 = med(lambda: eng.graph_adjacency(ind["edge_keys"], ind["keys"].numel()))
        d.update(induced_ms=round(t_ind, 4), next_adjacency_ms=round(t_adj2, 4), mask_plus_induced_ms=round(t_mask + t_ind, 4),
                 mask_plus_induced_to_compaction=round((t_mask + t_ind) / (t_uni + t_edges + t_adj), 3),
                 nodes_kept=ind["keys"].numel(), edges_kept=ind["edge_keys"].numel(),
                 # what the induced call has to move: keys and counts in and out, the masks, new_id, two gathers per kept edge
                 induced_algorithmic_bytes=12 * (n + ind["keys"].numel()) + 12 * (g.n_edges + ind["edge_keys"].numel()) + 5 * n + 8 * ind["edge_keys"].numel())
        d["induced_tb_per_s"] = round(d["induced_algorithmic_bytes"] / (t_ind * 1e-3) / 1e12, 3)
        out.append(d)
        g = pkg.KminmerGraph(ind["keys"], ind["counts"], ind["edge_keys"], ind["edge_counts"], ro, dst)
        del ug, m, ind
    tot = {f: round(sum(r.get(f, 0) for r in out), 4) for f in ("compaction_ms", "mask_ms", "induced_ms")}
    tot["mask_plus_induced_to_compaction"] = round((tot["mask_ms"] + tot["induced_ms"]) / tot["compaction_ms"], 3)
    tot["verdict"] = "expectation holds" if tot["mask_ms"] + tot["induced_ms"] < tot["compaction_ms"] else "expectation refuted"
    return {"rounds": out, "fixed_point": out[-1]["removed"] == 0, "totals": tot}


def genome_graph(eng, pkg, torch, dev, rate):
    """the genome-sampled set with substitutions -> (KminmerGraph, substitutions made)"""
    bases, read_off, n_reads = genome_reads(torch, dev, 50_000_000, 10_000, 30, 7)
    n_bases = n_reads * 10_000
    n_subst = inject_substitutions(torch, dev, bases, n_bases, rate, 11)
    cap = int(n_bases * 0.03)
    out = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
           "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = cap
    o.km_off, o.hash, o.rev = (out[x].data_ptr() for x in ("km_off", "hash", "rev"))
    torch.cuda.synchronize(dev)
    eng.extract_device(bases.data_ptr(), read_off.data_ptr(), n_reads, n_bases, 31, 10, 0.01, int(pkg.HashMode.Regular), o)
    del bases
    graph = pkg.KminmerGraph.build(eng, [out], min_count=2)
    del out
    torch.cuda.empty_cache()
    return graph, n_subst


def config1_graph(eng, pkg, torch, dev):
    """configs[1] against a table of every second key -> KminmerGraph"""
    items, n_reads, n = config1(eng, torch, dev, pkg)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    nd, nk = eng.count_device_ex(items["hash"].data_ptr(), n, 1, True, keys.data_ptr(), counts.data_ptr(), n)
    half_k, half_c = keys[:nk:2].contiguous(), counts[:nk:2].contiguous()
    del keys, counts
    half = pkg.CountTable(eng, half_k, half_c)
    e = half.edges(items, n_reads, 1)
    half.close()
    del items
    ne = e.numel()
    dk = torch.empty(ne, dtype=torch.int64, device=dev)
    dc = torch.empty(ne, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _, n_distinct = eng.count_device_ex(e.data_ptr(), ne, 1, True, dk.data_ptr(), dc.data_ptr(), ne)
    del e
    ek, ec = dk[:n_distinct].clone(), dc[:n_distinct].clone()
    del dk, dc
    row_off, dst = eng.graph_adjacency(ek, half_k.numel())
    graph = pkg.KminmerGraph(half_k, half_c, ek, ec, row_off, dst)
    torch.cuda.empty_cache()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rate", type=float, default=0.002)
    ap.add_argument("--max-rounds", type=int, default=6)
    ap.add_argument("--skip-config1", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "simplify_rate", "reps": a.reps, "k": K, "max_tip": 2 * K, "max_bubble": 4 * K}

    graph, n_subst = genome_graph(eng, pkg, torch, dev, a.rate)
    gen = rounds_leg(eng, pkg, torch, dev, graph, 2 * K, 4 * K, a.max_rounds, a.reps, a.warmup)
    gen.update(substitution_rate=a.rate, substitutions=n_subst)
    res["genome"] = gen
    print(json.dumps({"genome": gen}), flush=True)
    del graph
    torch.cuda.empty_cache()

    if not a.skip_config1:
        graph = config1_graph(eng, pkg, torch, dev)
        res["config1"] = rounds_leg(eng, pkg, torch, dev, graph, 2 * K, 4 * K, min(a.max_rounds, 4), a.reps, a.warmup)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
