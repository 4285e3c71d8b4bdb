"""Cost of piling the aligned read walks up on the unitigs and calling the consensus on the device (s2k_walks_pileup, s2k_pileup_consensus,
Pileup.add, Pileup.consensus), one process, one JSON file (default profiles/pileup_rate.json).  Times of whole calls:
median of --reps, HIP events on the engine's stream.
  genome : the read set of tools/align_rate.py (50 Mbp, 150 000 reads of 10 000 bases, 0.5 % substitutions, Regular 12 / 5 / 0.05, graph,
           unitigs, sequences, thread, bridge(16, 2), walks, UnitigGraph.align).  Pileup.add by route A (difference planes and a scan for
           the = and D pieces) and, when the library is a `make KNOBS=1` build loaded with S2K_LIB, by route B (S2K_PILEUP_ROUTE=B: one
           atomic add per matched base, consecutive lanes on consecutive positions); Pileup.consensus; and beside them Engine.align_pairs on
           the same walks: what the pile-up costs against the alignment it consumes.  Every add goes to a pile of its own that is zeroed
           outside the timed region; the piles of the two routes are compared.  Then the same add with the vote keys of long insertions
           (UnitigGraph.pileup(long_ins=True): s2k_walks_pileup_ex, the count of the key buffer's size and the KminmerCounter's add,
           DESIGN.md §3.23) and Pileup.consensus with the counter's table (s2k_counter_finish and s2k_pileup_consensus_ex).  The reads
           carry substitutions only: the I runs they key are the aligner's equal-cost choices (about 45 000 keys).  --parent FILE: a JSON
           that this tool wrote on the commit before §3.23, whose Pileup.add is set beside this one's."""
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
    ap.add_argument("--min-cov", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup_rate.json"))
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
    paths, _ = ug.bridge(eng, ug.thread(eng, table, out, n_reads, min_count=mc))
    table.close()
    seqs = ug.sequences(eng, ns)
    walks = ug.walks(eng, paths, ns)
    med = statistics.median

    t = eng.walks_targets(walks, paths.unitig, seqs[0], seqs[1], ug.overlap)
    qb, qe = pkg.walk_query_intervals(walks, read_off)
    qe = torch.where(t["bad"].bool(), qb, qe)
    tb, te = t["tgt_off"][:-1].contiguous(), t["tgt_off"][1:].contiguous()
    _, ms_pairs = timed(torch, dev, lambda: eng.align_pairs(bases, t["tgt"], qb, qe, tb, te), a.reps, a.warmup)
    al = ug.align(eng, walks, bases, read_off, seqs)

    def add_timed(route, long_ins=False):
        """Pileup.add into a fresh pile per repetition, the zeroing outside the events -> (the last pile, its stats, the times)"""
        if route == "B":
            os.environ["S2K_PILEUP_ROUTE"] = "B"
        else:
            os.environ.pop("S2K_PILEUP_ROUTE", None)
        ms, pl, st = [], None, None
        for rep in range(a.warmup + a.reps):
            if pl is not None and long_ins:
                pl.close()
            pl = ug.pileup(eng, seqs, long_ins=True) if long_ins else ug.pileup(eng, seqs)
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = pl.add(eng, walks, al, bases, read_off)
            e1.record()
            torch.cuda.synchronize(dev)
            if rep >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        os.environ.pop("S2K_PILEUP_ROUTE", None)
        return pl, st, ms

    pile_a, stats, ms_a = add_timed("A")
    knobs = os.environ.get("S2K_LIB", "") != ""
    ms_b, same = None, None
    if knobs:
        pile_b, stats_b, ms_b = add_timed("B")
        same = bool(torch.equal(pile_a.planes, pile_b.planes)) and stats == stats_b
    pol, ms_cons = timed(torch, dev, lambda: pile_a.consensus(eng, a.min_cov), a.reps, a.warmup)
    pile_k, stats_k, ms_k = add_timed("A", long_ins=True)
    same_k = bool(torch.equal(pile_a.planes, pile_k.planes)) and stats == stats_k
    pol_k, ms_cons_k = timed(torch, dev, lambda: pile_k.consensus(eng, a.min_cov), a.reps, a.warmup)
    long_keys = {"n_candidates": pile_k.n_long_candidates, "n_keys": pile_k.n_long_keys, "n_distinct": pile_k.counter.sizes(1)[0]}
    pile_k.close()
    parent = None
    if a.parent:
        with open(a.parent) as f:
            parent = json.load(f)["genome"]["pileup_add_route_a"]
    n_walks, n_draft = walks.n_walks, int(seqs[1].numel())
    h = pile_a.planes.to(torch.int64)
    votes = {f: int(h[i].sum()) for i, f in enumerate(pkg.PILEUP_PLANES)}
    votes = {"match": votes["match"], "del": votes["del"], "sub": sum(votes["sub%d" % c] for c in range(4)),
             "ins": sum(votes["ins%d" % c] for c in range(4)), "ins_long": votes["ins_long"]}
    rate = lambda ms: {"g_votes_per_s": round(sum(votes.values()) / (med(ms) * 1e-3) / 1e9, 3), "m_walks_per_s": round(n_walks / (med(ms) * 1e-3) / 1e6, 3)}  # noqa: E731
    res = {"tool": "pileup_rate", "reps": a.reps, "knobs_library": knobs,
           "genome": {"genome_bp": a.genome_bp, "read_len": a.read_len, "substitution_rate": a.rate, "l": l, "k": k, "density": d, "n_reads": n_reads,
                      "n_bases": n_bases, "n_unitigs": ug.n_unitigs, "draft_bases": n_draft, "n_steps": paths.n_steps, "n_walks": n_walks,
                      "run_slots": int(al.ops_off[-1]), "n_over": al.n_over, "n_bad": al.n_bad, "pileup_stats": stats, "votes": votes,
                      "min_cov": a.min_cov, "consensus_stats": pol.stats, "polished_bases": int(pol.sequences[1].numel()),
                      "align_pairs": summary(ms_pairs), "pileup_add_route_a": dict(summary(ms_a), **rate(ms_a)),
                      "pileup_add_route_b": None if ms_b is None else dict(summary(ms_b), **rate(ms_b)), "routes_give_one_pile": same,
                      "pileup_consensus": dict(summary(ms_cons), draft_gbases_per_s=round(n_draft / (med(ms_cons) * 1e-3) / 1e9, 3)),
                      "add_to_align_pairs": round(med(ms_a) / med(ms_pairs), 4),
                      "pileup_add_with_keys": dict(summary(ms_k), **rate(ms_k)), "keys_give_the_same_pile": same_k, "long_keys": long_keys,
                      "pileup_consensus_with_table": dict(summary(ms_cons_k), draft_gbases_per_s=round(n_draft / (med(ms_cons_k) * 1e-3) / 1e9, 3)),
                      "consensus_long_stats": pol_k.stats, "add_with_keys_to_align_pairs": round(med(ms_k) / med(ms_pairs), 4),
                      "parent_pileup_add": parent,
                      "add_with_keys_to_parent_add": None if parent is None else round(med(ms_k) / parent["ms_median"], 4)}}
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
