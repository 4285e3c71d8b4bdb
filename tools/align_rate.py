"""Cost of aligning read walks to their paths on the device (s2k_walks_targets, s2k_align_pairs, UnitigGraph.align), one
process, one JSON file (default profiles/align_rate.json).  Times of whole calls: median of --reps, HIP events on the engine's stream.
  genome : the genome-sampled read set of tools/vote_rate.py (tools/graph_rate.py: genome_reads) with every base substituted with
           probability --rate (0.5 %), extracted Regular 12 / 5 / 0.05 -- the setting of the tests' E. coli reads with errors; with
           0.5 % substitutions few of the 31 / 10 / 0.01 k-min-mers of vote_rate would be solid -- then graph, unitigs, sequences, thread,
           bridge(16, 2), walks.  Engine.walks_targets and Engine.align_pairs (each its sizes call and its writing call) separately,
           UnitigGraph.align whole, and beside them Engine.paths_walks (s2k_paths_walks) on the same walks: what the alignment costs
           against the coordinate lift it extends.  Rates in query bases and in walks per second."""
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
from table_rate import summary, timed  # noqa: E402


def substitute(torch, dev, bases, n_bases, rate, seed):
    """every base of bases[:n_bases] becomes another one with probability rate"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    code = torch.zeros(256, dtype=torch.int64, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    code[acgt.long()] = torch.arange(4, device=dev)
    step = 1 << 26
    for a in range(0, n_bases, step):
        x = bases[a: min(a + step, n_bases)]
        hit = torch.rand(x.numel(), device=dev, generator=g) < rate
        shift = torch.randint(1, 4, (x.numel(),), device=dev, generator=g)
        x[hit] = acgt[(code[x.long()] + shift)[hit] % 4]


def extract_all(eng, pkg, torch, dev, bases, read_off, n_reads, n_bases, l, k, d, mode, frac):
    """extract_device with minimizers, start and end kept -> the dict NodeSequences.build and UnitigGraph.thread want"""
    cap = int(n_bases * frac) + 1024
    out = {f: torch.empty(n_reads + 1, dtype=torch.int64, device=dev) for f in ("km_off", "mn_off")}
    out["hash"] = torch.empty(cap, dtype=torch.int64, device=dev)
    out["rev"] = torch.empty(cap, dtype=torch.uint8, device=dev)
    for f in ("start", "end", "mn_j", "mn_jend", "mn_hash"):
        out[f] = torch.empty(cap, dtype=torch.int32, device=dev)
    o = pkg.DeviceOut()
    o.km_capacity = o.mn_capacity = cap
    for f, t in out.items():
        setattr(o, f, t.data_ptr())
    torch.cuda.synchronize(dev)
    eng.extract_device(bases.data_ptr(), read_off.data_ptr(), n_reads, n_bases, l, k, d, mode, o, flags=pkg.FLAG_WANT_MINIMIZERS)
    out["bases"], out["read_off"] = bases, read_off
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-bp", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--rate", type=float, default=0.005)
    ap.add_argument("--max-edits", type=int, default=255)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    l, k, d, mc = 12, 5, 0.05, 2
    bases, read_off, n_reads = genome_reads(torch, dev, a.genome_bp, a.read_len, a.coverage, 7)
    n_bases = n_reads * a.read_len
    substitute(torch, dev, bases, n_bases, a.rate, 8)
    out = extract_all(eng, pkg, torch, dev, bases, read_off, n_reads, n_bases, l, k, d, int(pkg.HashMode.Regular), 0.15)
    graph = pkg.KminmerGraph.build(eng, [out], min_count=mc, min_edge_count=1)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, [out])
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths, bstats = ug.bridge(eng, ug.thread(eng, table, out, n_reads, min_count=mc))
    table.close()
    seqs = ug.sequences(eng, ns)
    offsets = ug.member_offsets(eng, ns)
    med = statistics.median

    _, ms_walks = timed(torch, dev, lambda: eng.paths_walks(ug, paths, offsets, ns.seq_len), a.reps, a.warmup)  # s2k_paths_walks alone
    walks = ug.walks(eng, paths, ns)
    t, ms_targets = timed(torch, dev, lambda: eng.walks_targets(walks, paths.unitig, seqs[0], seqs[1], ug.overlap), a.reps, a.warmup)
    qb, qe = pkg.walk_query_intervals(walks, read_off)
    qe = torch.where(t["bad"].bool(), qb, qe)
    tb, te = t["tgt_off"][:-1].contiguous(), t["tgt_off"][1:].contiguous()
    al, ms_pairs = timed(torch, dev, lambda: eng.align_pairs(bases, t["tgt"], qb, qe, tb, te, a.max_edits), a.reps, a.warmup)
    whole, ms_whole = timed(torch, dev, lambda: ug.align(eng, walks, bases, read_off, seqs, a.max_edits), a.reps, a.warmup)
    assert torch.equal(whole.edits, al["edits"]) and torch.equal(whole.ops, al["ops"])
    n_walks, q_bases = walks.n_walks, int((qe - qb).sum())
    aligned = whole.flags == 0
    edits = whole.edits[aligned].to(torch.int64)
    rate = lambda ms: {"query_gbases_per_s": round(q_bases / (med(ms) * 1e-3) / 1e9, 3), "m_walks_per_s": round(n_walks / (med(ms) * 1e-3) / 1e6, 3)}  # noqa: E731
    res = {"tool": "align_rate", "reps": a.reps,
           "genome": {"genome_bp": a.genome_bp, "read_len": a.read_len, "substitution_rate": a.rate, "l": l, "k": k, "density": d, "max_edits": a.max_edits,
                      "n_reads": n_reads, "n_bases": n_bases, "n_nodes": graph.n_nodes, "n_unitigs": ug.n_unitigs, "n_steps": paths.n_steps,
                      "bridge": bstats, "n_walks": n_walks, "query_bases": q_bases, "target_bytes": t["n_bytes"], "n_over": whole.n_over,
                      "n_bad": whole.n_bad, "edits_sum": int(edits.sum()), "edits_max": int(edits.max()) if edits.numel() else 0,
                      "edits_per_aligned_walk": round(float(edits.double().mean()), 2) if edits.numel() else 0.0, "run_slots": al["n_ops_bound"],
                      "paths_walks": dict(summary(ms_walks), **rate(ms_walks)), "walks_targets": dict(summary(ms_targets), **rate(ms_targets)),
                      "align_pairs": dict(summary(ms_pairs), **rate(ms_pairs)), "unitig_graph_align": dict(summary(ms_whole), **rate(ms_whole)),
                      "align_to_paths_walks": round(med(ms_whole) / med(ms_walks), 2)}}
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
