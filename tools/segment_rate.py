"""Cost of the segmented alignment route on the device (s2k_walks_segments, s2k_align_pairs on the segments, s2k_align_join; DESIGN.md
§3.22) beside the whole-walk alignment it stands in for, one process, one JSON file (default profiles/segment_rate.json).  Times of whole
calls: median of --reps, HIP events on the engine's stream.
  genome : the read set of tools/align_rate.py (genome-sampled reads with 0.5 % substitutions, Regular 12 / 5 / 0.05, graph, unitigs,
           sequences, thread, bridge(16, 2) with its origin kept, walks).  Engine.walks_segments, Engine.align_pairs on the segment pairs
           and Engine.align_join separately (each its sizes call and its writing call), and Engine.align_pairs on the whole walks of the
           same batch.  No ratio is asserted: the file holds the four times and what the batch was."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from s2k_loader import import_package  # noqa: E402
from align_rate import extract_all, substitute  # noqa: E402
from graph_rate import genome_reads  # noqa: E402
from table_rate import summary, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-bp", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--rate", type=float, default=0.005)
    ap.add_argument("--max-edits", type=int, default=255)
    ap.add_argument("--seg-len", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_rate.json"))
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
    src = ug.thread(eng, table, out, n_reads, min_count=mc)
    table.close()
    paths, bstats = ug.bridge(eng, src, origin=True)
    seqs = ug.sequences(eng, ns)
    offsets = ug.member_offsets(eng, ns)
    walks = ug.walks(eng, paths, ns)
    t = eng.walks_targets(walks, paths.unitig, seqs[0], seqs[1], ug.overlap)
    qb, qe = pkg.walk_query_intervals(walks, read_off)
    qe = torch.where(t["bad"].bool(), qb, qe)
    o = paths.origin
    med = statistics.median

    sg, ms_segments = timed(torch, dev, lambda: eng.walks_segments(ug, walks, offsets, ns.seq_len, qb, t["tgt_off"], t["bad"], o.paths, out, o.src_step,
                                                                   o.src_pos, a.seg_len), a.reps, a.warmup)
    al, ms_pairs = timed(torch, dev, lambda: eng.align_pairs(bases, t["tgt"], sg["q_begin"], sg["q_end"], sg["t_begin"], sg["t_end"], a.max_edits), a.reps,
                         a.warmup)
    j, ms_join = timed(torch, dev, lambda: eng.align_join(sg["seg_off"], t["bad"], al), a.reps, a.warmup)
    tb, te = t["tgt_off"][:-1].contiguous(), t["tgt_off"][1:].contiguous()
    whole, ms_whole = timed(torch, dev, lambda: eng.align_pairs(bases, t["tgt"], qb, qe, tb, te, a.max_edits), a.reps, a.warmup)
    both = (j["flags"] == 0) & (whole["flags"] == 0)
    n_walks, q_bases = walks.n_walks, int((qe - qb).sum())
    rate = lambda ms: {"query_gbases_per_s": round(q_bases / (med(ms) * 1e-3) / 1e9, 3), "m_walks_per_s": round(n_walks / (med(ms) * 1e-3) / 1e6, 3)}  # noqa: E731
    res = {"tool": "segment_rate", "reps": a.reps,
           "genome": {"genome_bp": a.genome_bp, "read_len": a.read_len, "substitution_rate": a.rate, "l": l, "k": k, "density": d, "max_edits": a.max_edits,
                      "seg_len": a.seg_len, "n_reads": n_reads, "n_bases": n_bases, "n_unitigs": ug.n_unitigs, "n_source_steps": src.n_steps,
                      "n_steps": paths.n_steps, "bridge": bstats, "n_walks": n_walks, "query_bases": q_bases, "n_segments": sg["n_segments"],
                      "anchors": sg["stats"], "n_over_segments": int((al["flags"] & pkg.ALIGN_OVER).ne(0).sum()),
                      "n_over_whole": int((whole["flags"] & pkg.ALIGN_OVER).ne(0).sum()), "n_over_joined": int((j["flags"] & pkg.ALIGN_OVER).ne(0).sum()),
                      "segment_run_slots": al["n_ops_bound"], "joined_runs": j["n_ops_total"], "whole_run_slots": whole["n_ops_bound"],
                      "edits_joined": int(j["edits"][both].to(torch.int64).sum()), "edits_whole": int(whole["edits"][both].to(torch.int64).sum()),
                      "walks_segments": dict(summary(ms_segments), **rate(ms_segments)), "align_pairs_segments": dict(summary(ms_pairs), **rate(ms_pairs)),
                      "align_join": dict(summary(ms_join), **rate(ms_join)), "align_pairs_whole_walks": dict(summary(ms_whole), **rate(ms_whole)),
                      "segmented_route_ms": round(med(ms_segments) + med(ms_pairs) + med(ms_join), 3)}}
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
