"""Rates of the merge of sorted count tables and of the accumulating counter (s2k_count_merge_device, s2k_counter_*,
s2k_run_file_count), one process, one JSON file (default profiles/count_merge_rate.json).
  merge   : two tables of --pairs pairs each (non-negative int64 keys, so torch's signed sort is the unsigned order), 0 / 50 / 100 %
            of the smaller one shared; median of --reps calls timed with HIP events on the engine's stream.  Algorithmic bytes:
            12 B per input pair read + 12 B per kept pair written.
  accum   : configs[1]'s k-min-mer hashes (1 000 000 x 10 kbp synthetic reads, l=31 k=10 d=0.01, Hpc) counted once by
            s2k_count_device_ex against the same hashes added to a counter in --batches slices and finished, alternated.
  file    : s2k_run_file against s2k_run_file_count (min_count 2) on one synthetic FASTA of --file-gbp Gbp, alternated; wall time
            of each whole call (file read included; for run_file_count the final finish too)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from s2k_loader import import_package  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E spec; ~6.3e12 is what a copy reaches


def tables(torch, dev, n, overlap, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    shared = int(overlap * n)
    total = 2 * n - shared
    u = torch.unique(torch.randint(0, 2 ** 63 - 1, (total + total // 16 + 1024,), device=dev, generator=g, dtype=torch.int64))
    u = u[torch.randperm(len(u), device=dev, generator=g)[:total]]
    a = torch.sort(u[:n]).values
    b = torch.sort(torch.cat([u[:shared], u[n:]])).values
    ca = torch.randint(1, 6, (n,), device=dev, generator=g, dtype=torch.int32)
    cb = torch.randint(1, 6, (n,), device=dev, generator=g, dtype=torch.int32)
    return a, ca, b, cb


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


def merge_rates(eng, torch, dev, n, reps, warmup):
    out = {"pairs_per_table": n}
    ok = torch.empty(2 * n, dtype=torch.int64, device=dev)
    oc = torch.empty(2 * n, dtype=torch.int32, device=dev)
    for ov in (0.0, 0.5, 1.0):
        a, ca, b, cb = tables(torch, dev, n, ov, 7)
        torch.cuda.synchronize(dev)
        for mc in (1, 2):
            r, ms = timed(torch, dev, lambda m=mc: eng.count_merge_device(a.data_ptr(), ca.data_ptr(), n, b.data_ptr(), cb.data_ptr(), n, m,
                                                                         ok.data_ptr(), oc.data_ptr(), 2 * n), reps, warmup)
            med = statistics.median(ms)
            alg = 12 * 2 * n + 12 * r[1]
            out["overlap%d_min%d" % (int(ov * 100), mc)] = {
                "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "n_distinct": r[0], "n_kept": r[1],
                "alg_bytes": alg, "alg_TBps": round(alg / (med * 1e-3) / 1e12, 3), "hbm_frac_alg": round(alg / (med * 1e-3) / HBM_PEAK, 4),
                # count pass (8 B per key read, 12 with a cutoff) + write pass (12 B per pair read) beside the algorithmic bytes
                "pass_bytes": (8 if mc <= 1 else 12) * 2 * n + 12 * 2 * n + 12 * r[1]}
        del a, ca, b, cb
    return out


def config1_hashes(eng, torch, dev):
    pkg = import_package()
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
    return t["hash"][: c["n_kminmers"]].clone()


def accum_rates(eng, torch, dev, batches, reps):
    pkg = import_package()
    keys = config1_hashes(eng, torch, dev)
    torch.cuda.empty_cache()
    n = keys.numel()
    ok = torch.empty(n, dtype=torch.int64, device=dev)
    oc = torch.empty(n, dtype=torch.int32, device=dev)
    parts = torch.tensor_split(keys, batches)
    torch.cuda.synchronize(dev)

    def one_shot():
        return eng.count_device_ex(keys.data_ptr(), n, 1, True, ok.data_ptr(), oc.data_ptr(), n)

    def counter():
        ctr = pkg.KminmerCounter(eng)
        for p in parts:
            ctr.add(p.data_ptr(), p.numel())
        nd, nk = ctr.sizes(1)
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)  # the pairs into preallocated outputs, as one_shot
        eng._check(eng.lib.s2k_counter_finish(ctypes.c_void_p(ctr.handle), 1, ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(oc.data_ptr()), n,
                                              ctypes.byref(a), ctypes.byref(b)))
        ctr.close()
        return nd, nk

    one_shot(), counter()  # warm-up
    t1, t2 = [], []
    for _ in range(reps):  # alternated, host clock around calls that end in a device synchronisation
        s = time.perf_counter()
        r1 = one_shot()
        t1.append((time.perf_counter() - s) * 1e3)
        s = time.perf_counter()
        r2 = counter()
        t2.append((time.perf_counter() - s) * 1e3)
    assert r1 == r2, (r1, r2)
    m1, m2 = statistics.median(t1), statistics.median(t2)
    return {"n_keys": n, "batches": batches, "n_distinct": r1[0], "one_shot_ms": [round(x, 3) for x in t1], "counter_ms": [round(x, 3) for x in t2],
            "one_shot_ms_median": round(m1, 3), "counter_ms_median": round(m2, 3), "ratio": round(m2 / m1, 3)}


def write_fasta(path, gbp, read_len=10000, seed=3):
    rng = np.random.default_rng(seed)
    n_reads = int(gbp * 1e9) // read_len
    alphabet = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        for r0 in range(0, n_reads, 20000):
            m = min(20000, n_reads - r0)
            rows = np.empty((m, 10 + read_len + 1), dtype=np.uint8)
            for i in range(m):
                rows[i, :10] = np.frombuffer(b">r%07d\n" % ((r0 + i) % 10 ** 7), dtype=np.uint8)
            rows[:, 10:10 + read_len] = alphabet[rng.integers(0, 4, size=(m, read_len), dtype=np.uint8)]
            rows[:, -1] = ord("\n")
            f.write(rows.tobytes())


def file_rates(eng, gbp, reps, tmpdir):
    pkg = import_package()
    path = os.path.join(tmpdir, "count_merge_rate.fa")
    write_fasta(path, gbp)
    args = (path, 31, 10, 0.01, pkg.HashMode.Hpc)
    eng.run_file(*args), eng.run_file_count(*args, min_count=2)  # warm-up (page cache, allocations)
    t1, t2 = [], []
    for _ in range(reps):  # host clock around each whole call (run_file_count: the counter's finish and the output tensors included)
        s = time.perf_counter()
        a = eng.run_file(*args)
        t1.append(time.perf_counter() - s)
        s = time.perf_counter()
        b = eng.run_file_count(*args, min_count=2)
        t2.append(time.perf_counter() - s)
        del b["keys"], b["counts"]
    assert a["n_kminmers"] == b["n_kminmers"] and a["xor_hash"] == b["xor_hash"]
    os.unlink(path)
    m1, m2 = statistics.median(t1), statistics.median(t2)
    return {"gbp": gbp, "file_bytes": a["n_bases"] + 11 * a["n_reads"], "n_kminmers": a["n_kminmers"], "n_distinct": b["n_distinct"],
            "n_kept": b["n_kept"], "run_file_s": [round(x, 4) for x in t1], "run_file_count_s": [round(x, 4) for x in t2],
            "ratio": round(m2 / m1, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("all", "merge", "accum", "file"), default="all")
    ap.add_argument("--pairs", type=int, default=70_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--file-gbp", type=float, default=3.0)
    ap.add_argument("--tmpdir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_merge_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)  # the HIP events bracket the library's work on this stream
    res = {"tool": "count_merge_rate", "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK}
    if a.only in ("all", "merge"):
        res["merge"] = merge_rates(eng, torch, dev, a.pairs, a.reps, a.warmup)
        torch.cuda.empty_cache()
    if a.only in ("all", "accum"):
        res["accum"] = accum_rates(eng, torch, dev, a.batches, max(3, a.reps // 2))
        torch.cuda.empty_cache()
    if a.only in ("all", "file"):
        res["file"] = file_rates(eng, a.file_gbp, 3, a.tmpdir)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
