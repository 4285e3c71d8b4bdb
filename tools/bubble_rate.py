"""s2k_graph_bubble_mask beside s2k_graph_simplify_mask on the same unitig graph, round by round (default profiles/bubble_rate.json),
on the two graphs of tools/simplify_rate.py (genome: the genome-sampled set with injected substitutions; config1: configs[1] against a
table of every second key).  Each round of KminmerGraph.simplify(2 k, 4 k, bubble_nodes=--nodes) is replayed: both mask calls are timed
on the round's unitig graph, each the median of --reps, HIP events on the engine's stream around the whole Engine method (its output
allocation and host wait included, on both sides); then the round goes on as simplify does, with the tip / simple-bubble mask when it
removes something and with the bubble mask otherwise.
No threshold: the yardstick is the existing mask call.  The bubble call does strictly more per source (a source compaction, two
traversals by a whole wave, the claims); the figure to read is bubble_to_mask per round beside sources and unitigs."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from s2k_loader import import_package  # noqa: E402
from simplify_rate import K, config1_graph, genome_graph  # noqa: E402
from table_rate import timed  # noqa: E402


def rounds_leg(eng, pkg, torch, dev, graph, max_tip, max_bubble, nodes, max_rounds, reps, warmup):
    med = lambda fn: (lambda r, ms: (r, statistics.median(ms)))(*timed(torch, dev, fn, reps, warmup))  # noqa: E731
    out, g = [], graph
    for _ in range(max_rounds):
        ug = g.unitigs(eng)
        m, t_mask = med(lambda: eng.graph_simplify_mask(ug, max_tip, max_bubble))
        b, t_bub = med(lambda: eng.graph_bubble_mask(ug, nodes, max_bubble))
        deg = ug.row_off[1:] - ug.row_off[:-1]
        d = {"nodes": g.n_nodes, "unitigs": ug.n_unitigs, "unitig_edges": ug.n_edges, "largest_row": int(deg.max()) if ug.n_unitigs else 0,
             "tips": m["n_tips"], "bubbles": m["n_bubbles"], "mask_removed": m["n_removed"],
             "sources": b["n_sources"], "found": b["n_found"], "applied": b["n_applied"], "bubble_removed": b["n_removed"],
             "mask_ms": round(t_mask, 4), "bubble_mask_ms": round(t_bub, 4), "bubble_to_mask": round(t_bub / t_mask, 3),
             "us_per_1000_sources": round(t_bub * 1e3 / max(b["n_sources"], 1) * 1e3, 3)}
        use = m if m["n_removed"] else b
        d["applied_mask"] = "simplify" if m["n_removed"] else "bubble"
        out.append(d)
        if use["n_removed"] == 0:
            break
        ind = eng.graph_induced(g, node_unitig=ug.node_unitig, remove=use["remove"])
        ro, dst = eng.graph_adjacency(ind["edge_keys"], ind["keys"].numel())
        g = pkg.KminmerGraph(ind["keys"], ind["counts"], ind["edge_keys"], ind["edge_counts"], ro, dst)
        del ug, m, b, ind
    return {"rounds": out, "fixed_point": out[-1]["mask_removed"] == 0 and out[-1]["bubble_removed"] == 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rate", type=float, default=0.002)
    ap.add_argument("--nodes", type=int, default=16)
    ap.add_argument("--max-rounds", type=int, default=8)
    ap.add_argument("--skip-config1", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bubble_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "bubble_rate", "reps": a.reps, "k": K, "max_tip": 2 * K, "max_bubble": 4 * K, "bubble_nodes": a.nodes}
    graph, n_subst = genome_graph(eng, pkg, torch, dev, a.rate)
    res["genome"] = rounds_leg(eng, pkg, torch, dev, graph, 2 * K, 4 * K, a.nodes, a.max_rounds, a.reps, a.warmup)
    res["genome"].update(substitution_rate=a.rate, substitutions=n_subst)
    print(json.dumps({"genome": res["genome"]}), flush=True)
    del graph
    torch.cuda.empty_cache()
    if not a.skip_config1:
        graph = config1_graph(eng, pkg, torch, dev)
        res["config1"] = rounds_leg(eng, pkg, torch, dev, graph, 2 * K, 4 * K, a.nodes, min(a.max_rounds, 6), a.reps, a.warmup)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
