"""Rates of the base-space sequence calls on the device (s2k_table_representatives, s2k_table_node_sequences, s2k_unitig_sequences),
one process, one JSON file (default profiles/unitig_seq_rate.json).  Times of whole calls: median of --reps, HIP events on the
engine's stream.
  genome : the genome-sampled set of tools/graph_rate.py, extracted with S2K_FLAG_WANT_MINIMIZERS.  Yardsticks, measured in the same
           process: the two-pass graph build of the set (the sum of its five steps, as tools/graph_rate.py measures them) for the three
           new calls together, and s2k_graph_unitigs on the same graph for the stitch alone.
Algorithmic bytes of the stitch's copy kernel: one byte read and one written per output base, 4 B per member, the node records (21 B
per node) and the piece offsets (8 B per member)."""
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
from table_rate import HBM_PEAK, summary, timed  # noqa: E402


def genome_of(torch, dev, genome_bp, seed):
    """the genome genome_reads(torch, dev, genome_bp, ..., seed) sampled its reads from: the same first draw of the same generator"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    return acgt[torch.randint(0, 4, (genome_bp,), device=dev, generator=g)]


def find_in_genome(torch, genome, seq, anchor=24):
    """whether seq (uint8 tensor) equals one slice of genome or of its reverse complement, on the device: candidates from the first
    `anchor` bytes, then a whole comparison of each"""
    comp = torch.arange(256, dtype=torch.uint8, device=genome.device)
    comp[torch.tensor(list(b"ACGT"), device=genome.device).long()] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=genome.device)
    L, G = seq.numel(), genome.numel()
    if L == 0 or L > G:
        return L == 0
    for text in (genome, comp[genome.flip(0).long()]):
        m = torch.ones(G - L + 1, dtype=torch.bool, device=genome.device)
        for j in range(min(anchor, L)):
            m &= text[j: j + G - L + 1] == seq[j]
        for c in torch.nonzero(m)[:, 0].tolist()[:64]:
            if torch.equal(text[c: c + L], seq):
                return True
    return False


def extract_with_minimizers(eng, pkg, torch, dev, bases, read_off, n_reads, n_bases, l, k, d, mode, frac=0.03):
    """extract_device with FLAG_WANT_MINIMIZERS -> the dict of GPU tensors NodeSequences.build wants (bases and read_off included)"""
    cap = int(n_bases * frac) + 1024
    out = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
           "rev": torch.empty(cap, dtype=torch.uint8, device=dev), "mn_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev),
           "mn_j": torch.empty(cap, dtype=torch.int32, device=dev), "mn_jend": torch.empty(cap, dtype=torch.int32, device=dev),
           "mn_hash": torch.empty(cap, dtype=torch.int32, device=dev)}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unitig_seq_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    res = {"tool": "unitig_seq_rate", "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK}

    k = 10
    bases, read_off, n_reads = genome_reads(torch, dev, 50_000_000, 10_000, 30, 7)
    n_bases = n_reads * 10_000
    out = extract_with_minimizers(eng, pkg, torch, dev, bases, read_off, n_reads, n_bases, 31, k, 0.01, int(pkg.HashMode.Regular))
    n = int(out["km_off"][-1])
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
    n_nodes = keys.numel()
    _, ms_uni = timed(torch, dev, lambda: eng.graph_unitigs(row_off, dst, n_nodes), a.reps, a.warmup)
    u = eng.graph_unitigs(row_off, dst, n_nodes)
    t = u["n_unitigs"]

    table = pkg.CountTable(eng, keys, counts)
    i = pkg.extraction_struct(out, n_reads, ("rev",), mn=True)
    rep = torch.full((n_nodes,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    H = ctypes.c_void_p(table.handle)
    _, ms_rep = timed(torch, dev, lambda: eng._check(eng.lib.s2k_table_representatives(H, n_reads, ctypes.byref(i), 0, rep.data_ptr())), a.reps, a.warmup)
    nb = ctypes.c_uint64(0)

    def nodeseq(ns):
        eng._check(eng.lib.s2k_table_node_sequences(H, n_reads, ctypes.byref(i), k, bases.data_ptr(), read_off.data_ptr(), 0, rep.data_ptr(),
                                                    ctypes.byref(ns) if ns is not None else None, 0, ctypes.byref(nb)))

    _, ms_size = timed(torch, dev, lambda: nodeseq(None), a.reps, a.warmup)
    pool_bytes = int(nb.value)
    table.close()
    ns = pkg.NodeSequences.build(eng, pkg.KminmerGraph(keys, counts, ek, ec, row_off, dst), [out], k=k)
    table = pkg.CountTable(eng, keys, counts)
    H = ctypes.c_void_p(table.handle)
    st = ns.struct()
    _, ms_write = timed(torch, dev, lambda: nodeseq(st), a.reps, a.warmup)
    table.close()

    out_off = torch.zeros(t + 1, dtype=torch.int64, device=dev)
    overlap = torch.zeros(2 * t, dtype=torch.int32, device=dev)
    eng._check(eng.lib.s2k_unitig_sequences(eng.ctx, u["uni_off"].data_ptr(), u["members"].data_ptr(), u["circular"].data_ptr(), t, n_nodes,
                                            ctypes.byref(st), out_off.data_ptr(), None, overlap.data_ptr(), 0, ctypes.byref(nb)))
    total = int(nb.value)
    seq = torch.empty(total, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_unitig_sequences(eng.ctx, u["uni_off"].data_ptr(), u["members"].data_ptr(), u["circular"].data_ptr(), t,  # noqa: E731
                                                         n_nodes, ctypes.byref(st), out_off.data_ptr(), seq.data_ptr(), overlap.data_ptr(), total,
                                                         ctypes.byref(nb)))
    _, ms_stitch = timed(torch, dev, fn, a.reps, a.warmup)
    med = statistics.median
    three = med(ms_rep) + med(ms_size) + med(ms_write) + med(ms_stitch)
    copy_bytes = 2 * total + (4 + 8) * n_nodes + 21 * n_nodes
    res["genome"] = {
        "n_items": n, "n_nodes": n_nodes, "n_unitigs": t, "pool_bytes": pool_bytes, "unitig_bases": total,
        "representatives_call": summary(ms_rep), "node_sequences_sizes_call": summary(ms_size), "node_sequences_write_call": summary(ms_write),
        "unitig_sequences_call": summary(ms_stitch), "graph_unitigs_call": summary(ms_uni), "build_steps_ms": steps,
        "sequence_calls_ms": round(three, 4), "sequence_calls_to_build": round(three / steps["total"], 3),
        "stitch_to_graph_unitigs": round(med(ms_stitch) / med(ms_uni), 3),
        "node_pool_tb_per_s": round(2 * pool_bytes / (med(ms_write) * 1e-3) / 1e12, 3),
        "stitch_algorithmic_bytes": copy_bytes,
        "stitch_call_frac_of_8tb": round(copy_bytes / (med(ms_stitch) * 1e-3) / HBM_PEAK, 4),
        "stitched_in_genome": bool(all(find_in_genome(torch, genome_of(torch, dev, 50_000_000, 7), seq[int(out_off[x]): int(out_off[x + 1])])
                                       for x in range(t)))}
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
