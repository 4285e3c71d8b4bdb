"""Cost of the GAF text on the device (s2k_walks_gaf, Engine.walks_gaf) beside the host writer it stands in for, one
process, one JSON file (default profiles/gaf_rate.json).
  genome : the read set, walks and whole-walk alignments of tools/align_rate.py (genome-sampled reads with 0.5 % substitutions, Regular
           12 / 5 / 0.05, graph, unitigs, sequences, thread, bridge(16, 2), walks, UnitigGraph.align).  Engine.walks_gaf (its sizes call
           and its writing call) with and without the alignments: median of --reps, HIP events on the engine's stream; then the copy of
           the text to the host and the write of the bytes to a file, wall clock, median of three.  Beside it ONE run of the host writer,
           ReadWalks.write_gaf without an engine, on the first reads of the batch that hold at most --host-walks walks (the number of
           walks it got is recorded, nothing is scaled), and the device route (format, copy, write) on the same walks.  No ratio is
           asserted."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from s2k_loader import import_package  # noqa: E402
from align_rate import extract_all, substitute  # noqa: E402
from graph_rate import genome_reads  # noqa: E402
from table_rate import summary, timed  # noqa: E402


def head_of(pkg, torch, walks, al, max_walks):
    """the walks of the first reads that hold at most max_walks walks, and their alignments -> (ReadWalks, WalkAlignments, n_reads)"""
    wo = walks.walk_off
    r = int(torch.searchsorted(wo, torch.tensor([max_walks], dtype=wo.dtype, device=wo.device), right=True)[0]) - 1
    nw = int(wo[r])
    cut = {f: getattr(walks, f)[:nw] for f in pkg.ReadWalks.FIELDS}
    # (a read's walks hold its steps in order: the steps of the first reads are a prefix, and so are their run slots)
    ns = int((cut["first_step"] + (cut["n_steps"].to(torch.int64) & 0xFFFFFFFF)).max()) if nw else 0
    sub = pkg.ReadWalks(types.SimpleNamespace(unitig=walks.paths.unitig[:ns]), wo[:r + 1].contiguous(), cut["first_step"], cut["n_steps"], cut["items"],
                        cut["path_len"], cut["path_start"], cut["path_end"], cut["flags"], qstart=cut["qstart"], qend=cut["qend"], n_walks=nw)
    sal = pkg.WalkAlignments(al.edits[:nw], al.matches[:nw], al.n_ops[:nw], al.ops_off[:nw + 1].contiguous(), al.ops[:int(al.ops_off[nw])], al.flags[:nw])
    return sub, sal, r


def host_steps(torch, dev, text, path, reps=3):
    """the copy of the text to the host and the write of the bytes, wall clock -> (ms of the copies, ms of the writes)"""
    copy, write = [], []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        h = text.cpu().numpy()
        t1 = time.perf_counter()
        with open(path, "wb") as f:
            f.write(h.data)
        t2 = time.perf_counter()
        copy.append((t1 - t0) * 1e3)
        write.append((t2 - t1) * 1e3)
    return copy, write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--genome-bp", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=10_000)
    ap.add_argument("--coverage", type=int, default=30)
    ap.add_argument("--rate", type=float, default=0.005)
    ap.add_argument("--max-edits", type=int, default=255)
    ap.add_argument("--host-walks", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaf_rate.json"))
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
    al = ug.align(eng, walks, bases, read_off, seqs, a.max_edits)
    lens = torch.full((n_reads,), a.read_len, dtype=torch.int64, device=dev)
    med = statistics.median
    tmp = tempfile.mkdtemp(prefix="gaf_rate_")
    p_dev, p_host = os.path.join(tmp, "device.gaf"), os.path.join(tmp, "host.gaf")

    def route(w, x):
        """Engine.walks_gaf on the walks w with the alignments x (None: without), the copy and the write"""
        t, ms = timed(torch, dev, lambda: eng.walks_gaf(w, w.paths.unitig, read_lengths=lens[:w.walk_off.numel() - 1], alignments=x), a.reps, a.warmup)
        copy, write = host_steps(torch, dev, t["text"], p_dev)
        n, nw = t["n_bytes"], w.n_walks
        return {"n_walks": nw, "bytes": n, "walks_gaf": dict(summary(ms), text_GB_per_s=round(n / (med(ms) * 1e-3) / 1e9, 3), ns_per_walk=round(med(ms) * 1e6 / max(nw, 1), 2)),
                "copy_to_host_ms": round(med(copy), 3), "file_write_ms": round(med(write), 3),
                "format_copy_write_ms": round(med(ms) + med(copy) + med(write), 3),
                "format_copy_write_us_per_walk": round((med(ms) + med(copy) + med(write)) * 1e3 / max(nw, 1), 4)}

    res = {"tool": "gaf_rate", "reps": a.reps,
           "genome": {"genome_bp": a.genome_bp, "read_len": a.read_len, "substitution_rate": a.rate, "l": l, "k": k, "density": d, "max_edits": a.max_edits,
                      "n_reads": n_reads, "n_steps": paths.n_steps, "n_walks": walks.n_walks, "run_slots": int(al.ops.numel()), "n_over": al.n_over, "n_bad": al.n_bad,
                      "device_plain": route(walks, None), "device_aligned": route(walks, al)}}
    sub, sal, r = head_of(pkg, torch, walks, al, a.host_walks)
    host = {"n_walks_cap": a.host_walks, "n_walks": sub.n_walks, "n_reads": r}
    for tag, x in (("plain", None), ("aligned", sal)):
        res["genome"]["device_%s_head" % tag] = route(sub, x)
        t0 = time.perf_counter()
        sub.write_gaf(p_host, ug, read_lengths=[a.read_len] * r, alignments=x)  # the parent commit's path, once
        s = time.perf_counter() - t0
        same = open(p_host, "rb").read() == open(p_dev, "rb").read()
        host[tag] = {"seconds": round(s, 3), "us_per_walk": round(s * 1e6 / max(sub.n_walks, 1), 3), "bytes": os.path.getsize(p_host), "equals_device_text": same}
    res["genome"]["host_writer"] = host
    for p in (p_dev, p_host):
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(tmp)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
