"""Cost of the majority-vote representatives on the device (s2k_table_vote_keys, s2k_table_vote_representatives, s2k_vote_ordinals;
DESIGN.md §3.19), one process, one JSON file (default profiles/vote_rate.json).  Times of whole calls: median of --reps, HIP events on
the engine's stream.
  genome : the genome-sampled set of tools/graph_rate.py, extracted with S2K_FLAG_WANT_MINIMIZERS (tools/unitig_seq_rate.py).
           NodeSequences.build(vote=True) -- keys, counter add + finish, table create, best, ordinals, then the two record rounds --
           against NodeSequences.build(vote=False), the earliest-occurrence build, measured in the same process; s2k_table_vote_keys
           (the writing call) alone as bytes of read bases per second, and the other steps of the voted build one by one."""
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
from graph_rate import genome_reads  # noqa: E402
from table_rate import HBM_PEAK, summary, timed  # noqa: E402
from unitig_seq_rate import extract_with_minimizers  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vote_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    k = 10
    bases, read_off, n_reads = genome_reads(torch, dev, 50_000_000, 10_000, 30, 7)
    n_bases = n_reads * 10_000
    out = extract_with_minimizers(eng, pkg, torch, dev, bases, read_off, n_reads, n_bases, 31, k, 0.01, int(pkg.HashMode.Regular))
    n = int(out["km_off"][-1])
    ctr = pkg.KminmerCounter(eng)
    ctr.add(out["hash"].data_ptr(), n)
    keys, counts = ctr.finish(2)
    ctr.close()
    table = pkg.CountTable(eng, keys, counts)
    n_nodes = keys.numel()
    med = statistics.median

    _, ms_early = timed(torch, dev, lambda: pkg.NodeSequences.build(eng, table, [out], k=k, vote=False), a.reps, a.warmup)
    voted, ms_voted = timed(torch, dev, lambda: pkg.NodeSequences.build(eng, table, [out], k=k, vote=True), a.reps, a.warmup)
    early = pkg.NodeSequences.build(eng, table, [out], k=k)
    moved = int((voted.rep != early.rep).sum())

    # the steps of the voted build, one by one
    i, nk = pkg.extraction_struct(out, n_reads, ("rev",), mn=True), ctypes.c_uint64(0)
    H = ctypes.c_void_p(table.handle)
    args = (H, n_reads, ctypes.byref(i), k, bases.data_ptr(), read_off.data_ptr())
    _, ms_size = timed(torch, dev, lambda: eng._check(eng.lib.s2k_table_vote_keys(*args, None, 0, ctypes.byref(nk))), a.reps, a.warmup)
    n_keys = int(nk.value)
    vkeys = torch.empty(n_keys, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    _, ms_keys = timed(torch, dev, lambda: eng._check(eng.lib.s2k_table_vote_keys(*args, vkeys.data_ptr(), n_keys, ctypes.byref(nk))), a.reps, a.warmup)

    def count():
        c = pkg.KminmerCounter(eng)
        c.add(vkeys.data_ptr(), n_keys)
        r = c.finish(1)
        c.close()
        return r

    (tk, tc), ms_count = timed(torch, dev, count, a.reps, a.warmup)
    _, ms_table = timed(torch, dev, lambda: pkg.CountTable(eng, tk, tc).close(), a.reps, a.warmup)
    votes = pkg.CountTable(eng, tk, tc)
    best = torch.zeros(n_nodes, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    _, ms_best = timed(torch, dev, lambda: eng.table_vote_representatives(table, votes, out, k, 0, best), a.reps, a.warmup)
    _, ms_ord = timed(torch, dev, lambda: eng.vote_ordinals(best), a.reps, a.warmup)
    assert torch.equal(eng.vote_ordinals(best), voted.rep)
    votes.close()
    table.close()
    res = {"tool": "vote_rate", "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK,
           "genome": {"n_reads": n_reads, "n_bases": n_bases, "n_items": n, "n_nodes": n_nodes, "n_vote_keys": n_keys, "n_distinct_vote_keys": tk.numel(),
                      "representatives_moved_by_the_vote": moved,
                      "build_earliest": summary(ms_early), "build_voted": summary(ms_voted), "voted_to_earliest": round(med(ms_voted) / med(ms_early), 3),
                      "vote_keys_sizes_call": summary(ms_size), "vote_keys_call": summary(ms_keys),
                      "vote_keys_read_bases_gb_per_s": round(n_bases / (med(ms_keys) * 1e-3) / 1e9, 2),
                      "count_keys": summary(ms_count), "vote_table_create": summary(ms_table), "vote_representatives_call": summary(ms_best),
                      "vote_ordinals_call": summary(ms_ord)}}
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
