"""A/B of the two device counts on one process: s2k_count_device (global atomicCAS table, unordered) against s2k_count_device_ex
(partition + LDS count; sorted and unsorted, min_count 1 and 2).  Inputs: the k-min-mer hashes of configs[1] (1 000 000 x 10 kbp
synthetic reads, l=31 k=10 d=0.01, Hpc; extracted into HBM) and a repeat-rich set (ecoli windows resampled, l=21 k=3 d=0.05, Hpc).
Every variant: warm-up, then the median of --reps calls timed with HIP events on the engine's stream.  Prints one JSON line.
Byte model: 8 B per key read + 12 B per kept pair written (algorithmic); the partition passes' extra traffic is reported apart."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from s2k_loader import import_package  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X HBM3E spec; ~6.3e12 is what a copy reaches


def config1_hashes(eng, torch, dev):
    n_reads, L, seed = 1_000_000, 10_000, 1
    d_b = torch.empty(n_reads * L + 64, dtype=torch.uint8, device=dev)
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L
    cap = int(n_reads * L * 0.0215)
    t = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
         "start": torch.empty(cap, dtype=torch.int32, device=dev), "end": torch.empty(cap, dtype=torch.int32, device=dev),
         "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
    pkg = import_package()
    o = pkg.DeviceOut()
    o.km_capacity = cap
    o.km_off, o.hash, o.start, o.end, o.rev = (t[x].data_ptr() for x in ("km_off", "hash", "start", "end", "rev"))
    torch.cuda.synchronize(dev)
    eng.synth_bases_device(seed, 0, n_reads * L, d_b.data_ptr())
    c = eng.extract_device(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L, 31, 10, 0.01, int(pkg.HashMode.Hpc), o)
    return t["hash"][: c["n_kminmers"]].clone()


def repeat_rich_hashes(eng, torch, dev, n_reads):
    pkg = import_package()
    ecoli = open(os.path.join(ROOT, "tests", "golden", "ecoli.genome.100k.fa")).read().split("\n")[1].encode()
    rng = np.random.default_rng(9)
    reads = [bytes(ecoli[a: a + 3000]) for a in rng.integers(0, len(ecoli) - 3000, size=n_reads)]
    got = eng.extract_reads(reads, 21, 3, 0.05, pkg.HashMode.Hpc)
    return torch.from_numpy(got["hash"].view(np.int64)).to(dev)


def measure(eng, torch, dev, keys, reps, warmup):
    n = keys.numel()
    ok = torch.empty(n, dtype=torch.int64, device=dev)
    oc = torch.empty(n, dtype=torch.int32, device=dev)
    variants = [("count_device", None, None)] + [("count_device_ex_%s_min%d" % ("sorted" if s else "unsorted", m), s, m)
                                                 for s in (True, False) for m in (1, 2)]
    out = {"n_keys": n}
    for name, srt, mc in variants:
        if srt is None:
            call = lambda: (eng.count_device(keys.data_ptr(), n, ok.data_ptr(), oc.data_ptr(), n), None)  # noqa: E731
        else:
            call = lambda s=srt, m=mc: eng.count_device_ex(keys.data_ptr(), n, m, s, ok.data_ptr(), oc.data_ptr(), n)  # noqa: E731
        for _ in range(warmup):
            r = call()
        st = torch.cuda.current_stream(dev)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            r = call()
            b.record(st)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        kept = r[0] if srt is None else r[1]
        alg = 8 * n + 12 * kept
        e = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "kept": kept,
             "gkeys_per_s": round(n / med / 1e6, 3), "alg_bytes": alg, "hbm_frac_alg": round(alg / (med * 1e-3) / HBM_PEAK, 4)}
        if srt is not None:
            e["n_distinct"] = r[0]
            # two partition passes (histogram read + scatter read + write: 24 B/key each), pairs written in place and copied out
            e["extra_bytes_partition"] = 48 * n
            e["extra_bytes_pairs"] = 24 * kept
        out[name] = e
    base = out["count_device"]["ms_median"]
    out["speedup_sorted_min1_vs_count_device"] = round(base / out["count_device_ex_sorted_min1"]["ms_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat-reads", type=int, default=40000, help="ecoli windows of 3 kbp in the repeat-rich set")
    ap.add_argument("--skip-config1", action="store_true")
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)  # the HIP events bracket the library's work on this stream
    res = {"tool": "count_rate", "reps": a.reps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_PEAK}
    if not a.skip_config1:
        k1 = config1_hashes(eng, torch, dev)
        torch.cuda.empty_cache()
        res["config1"] = measure(eng, torch, dev, k1, a.reps, a.warmup)
        del k1
    k2 = repeat_rich_hashes(eng, torch, dev, a.repeat_reads)
    res["repeat_rich"] = measure(eng, torch, dev, k2, a.reps, a.warmup)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
