"""Rates of the count-table look-up and of the per-read filter (s2k_table_create / _lookup / _filter), one process, one JSON file
(default profiles/table_rate.json).  Everything on configs[1] (1 000 000 x 10 kbp synthetic reads, l=31 k=10 d=0.01, Hpc): its
139.6 M k-min-mer hashes, and their table from s2k_count_device_ex (min_count 1, sorted).  Times: median of --reps calls, HIP events
on the engine's stream (each call ends in a host wait; the events bracket the whole call).
  index   : s2k_table_create on the full table (1.7 GB of keys + counts): the one coalesced pass and the directory.
  lookup  : (a) the 139.6 M hashes looked up in the full table (cannot stay in the 256 MiB Infinity Cache); (b) the same queries in a
            table of every 17th key (about 8 M keys, ~100 MB: it can).
  filter  : the configs[1] k-min-mers (km_off, hash, start, end, rev) against a table of every second key (min_count 1), every
            output array written; beside it the look-up alone of the same hashes in the same table.
  --bits-sweep (a `make KNOBS=1` library, loaded with S2K_LIB): look-up (a) and (b) again with the directory width B forced through
            S2K_DEBUG_TABLE_BITS."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from s2k_loader import import_package  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E spec; ~6.3e12 is what a copy reaches


def timed(torch, dev, fn, reps, warmup):
    st = torch.cuda.current_stream(dev)
    for _ in range(warmup):
        fn()
    ms = []
    r = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        r = fn()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return r, ms


def summary(ms, n_queries=None):
    med = statistics.median(ms)
    d = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    if n_queries:
        d["G_queries_per_s"] = round(n_queries / (med * 1e-3) / 1e9, 3)
    return d


def config1(eng, torch, dev, pkg):
    n_reads, L, seed = 1_000_000, 10_000, 1
    d_b = torch.empty(n_reads * L + 64, dtype=torch.uint8, device=dev)
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L
    cap = int(n_reads * L * 0.0215)
    t = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
         "start": torch.empty(cap, dtype=torch.int32, device=dev), "end": torch.empty(cap, dtype=torch.int32, device=dev),
         "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = cap
    o.km_off, o.hash, o.start, o.end, o.rev = (t[x].data_ptr() for x in ("km_off", "hash", "start", "end", "rev"))
    torch.cuda.synchronize(dev)
    eng.synth_bases_device(seed, 0, n_reads * L, d_b.data_ptr())
    c = eng.extract_device(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L, 31, 10, 0.01, int(pkg.HashMode.Hpc), o)
    del d_b
    n = c["n_kminmers"]
    return {f: (x if f == "km_off" else x[:n]) for f, x in t.items()}, n_reads, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bits-sweep", default="", help="comma-separated B values (needs a KNOBS=1 library)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)  # the HIP events bracket the library's work on this stream
    items, n_reads, n = config1(eng, torch, dev, pkg)
    hashes = items["hash"]
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    (nd, nk), ms = timed(torch, dev, lambda: eng.count_device_ex(hashes.data_ptr(), n, 1, True, keys.data_ptr(), counts.data_ptr(), n), 3, 1)
    keys, counts = keys[:nk], counts[:nk]
    res = {"tool": "table_rate", "reps": a.reps, "n_kminmers": n, "n_reads": n_reads, "table_keys": nk, "table_bytes": 12 * nk,
           "count_device_ex_sorted": summary(ms), "hbm_peak_bytes_per_s": HBM_PEAK}

    _, ms = timed(torch, dev, lambda: pkg.CountTable(eng, keys, counts).close(), a.reps, a.warmup)
    res["index_full"] = summary(ms)
    res["index_full"]["alg_bytes"] = 8 * nk

    out = torch.empty(n, dtype=torch.int32, device=dev)

    def lookup_run(table, tag, queries):
        torch.cuda.synchronize(dev)
        fn = lambda: eng._check(eng.lib.s2k_table_lookup(table.handle, queries.data_ptr(), queries.numel(), out.data_ptr()))  # noqa: E731
        _, ms = timed(torch, dev, fn, a.reps, a.warmup)
        hits = int((out[:queries.numel()] != 0).sum())
        d = summary(ms, queries.numel())
        d.update(hits=hits, table_keys=table.n)
        res[tag] = d

    full = pkg.CountTable(eng, keys, counts)
    lookup_run(full, "lookup_full_self", hashes)
    small_k, small_c = keys[::17].contiguous(), counts[::17].contiguous()
    small = pkg.CountTable(eng, small_k, small_c)
    lookup_run(small, "lookup_8M_keys", hashes)
    small.close()
    full.close()

    half_k, half_c = keys[::2].contiguous(), counts[::2].contiguous()
    half = pkg.CountTable(eng, half_k, half_c)
    lookup_run(half, "lookup_half_table", hashes)
    cap = n
    so = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
          "start": torch.empty(cap, dtype=torch.int32, device=dev), "end": torch.empty(cap, dtype=torch.int32, device=dev),
          "rev": torch.empty(cap, dtype=torch.uint8, device=dev), "offset": torch.empty(cap, dtype=torch.int32, device=dev),
          "count": torch.empty(cap, dtype=torch.int32, device=dev)}
    i, o = pkg.DeviceOut(), pkg.SolidOut()
    i.km_capacity = n
    for f in ("km_off", "hash", "start", "end", "rev"):
        setattr(i, f, items[f].data_ptr())
    o.capacity = cap
    for f, t in so.items():
        setattr(o, f, t.data_ptr())
    nkept = ctypes.c_uint64(0)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_table_filter(half.handle, n_reads, ctypes.byref(i), 1, ctypes.byref(o), ctypes.byref(nkept)))  # noqa: E731
    _, ms = timed(torch, dev, fn, a.reps, a.warmup)
    d = summary(ms, n)
    d.update(n_kept=int(nkept.value), ratio_to_lookup=round(statistics.median(ms) / res["lookup_half_table"]["ms_median"], 3))
    res["filter_half_table"] = d
    half.close()

    if a.bits_sweep:
        sweep = {}
        for b in [int(x) for x in a.bits_sweep.split(",")]:
            os.environ["S2K_DEBUG_TABLE_BITS"] = str(b)
            for tag, kk, cc in (("full", keys, counts), ("8M", small_k, small_c)):
                t = pkg.CountTable(eng, kk, cc)
                lookup_run(t, "sweep", hashes)
                sweep["%s_B%d" % (tag, b)] = res.pop("sweep")
                t.close()
        os.environ.pop("S2K_DEBUG_TABLE_BITS", None)
        res["bits_sweep"] = sweep
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
