"""Rates of the lift of read paths onto the untangled contigs on the device (s2k_unitig_copy_places, s2k_paths_lift sizes only and
writing), one process, one JSON file (default profiles/lift_rate.json).  Times: median of --reps calls, HIP events on the engine's
stream (each call ends in a host wait; the events bracket the whole call).  Beside them, re-measured in the same job on the same
paths and the same graph: s2k_paths_bridge (16, 2), writing, which has the lift's kernel shape and makes one row search per step where
the lift makes up to three on a step of a resolved unitig.
  ring : the paired ring of tests/test_span.chained_paths, made large: --unitigs unitigs of 1 .. 3 members, edges t -> t + 1 and t ->
         t + 2; --reads reads of --steps whole unitigs, all linked, each taking one kind of edge all along, half of them on the twin
         strand.  Their spans resolve every unitig, so every step lies on a duplicated unitig, the twin search runs on every step of
         an even strand, and each read's steps merge into one.
The ratio to watch is lift / bridge."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from s2k_loader import import_package  # noqa: E402
from table_rate import summary, timed  # noqa: E402


def ring_arrays(T, n_reads, n_steps, seed):
    """host arrays -> (edge keys ascending and closed under twins, uni_off, unitig counts, edge counts, the step arrays by name)"""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.int64)
    a = np.concatenate([2 * t, 2 * t])
    b = np.concatenate([2 * ((t + 1) % T), 2 * ((t + 2) % T)])
    keys = np.unique(np.concatenate([a << 32 | b, (b ^ 1) << 32 | (a ^ 1)]).astype(np.uint64))
    ln = 1 + t % 3
    uni_off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    start = rng.integers(0, T, size=n_reads)
    rev = rng.integers(0, 2, size=n_reads)
    stride = rng.integers(1, 3, size=n_reads)
    i = np.arange(n_steps, dtype=np.int64)
    unit = (start[:, None] + np.where(rev, -1, 1)[:, None] * stride[:, None] * i[None, :]) % T
    count = ln[unit]
    item = np.cumsum(count, axis=1) - count
    flags = np.ones_like(unit)
    flags[:, 0] = 0
    steps = {"unitig": 2 * unit + rev[:, None], "pos": np.zeros_like(unit), "count": count, "item": item, "flags": flags, "start": 7 * item,
             "end": 7 * (item + count - 1) + 30}
    return keys, uni_off, rng.integers(1, 1000, size=T), rng.integers(1, 100, size=len(keys)), {k: v.reshape(-1) for k, v in steps.items()}


def ring(torch, dev, pkg, eng, T, n_reads, n_steps, seed):
    """-> (UnitigGraph, ReadPaths) on the device"""
    keys, uni_off, cnt, ec, steps = ring_arrays(T, n_reads, n_steps, seed)
    tt = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)  # noqa: E731
    edge_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
    row_off, dst = eng.graph_adjacency(edge_keys, T)
    ug = pkg.UnitigGraph(tt(uni_off, torch.int64), tt(2 * np.arange(int(uni_off[-1])), torch.int32), None, None, torch.zeros(T, dtype=torch.uint8, device=dev),
                         tt(cnt, torch.int64), edge_keys, tt(ec, torch.int32), row_off, dst)
    paths = pkg.ReadPaths(tt(np.arange(n_reads + 1, dtype=np.int64) * n_steps, torch.int64), **{k: tt(v, torch.int32) for k, v in steps.items()})
    return ug, paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--unitigs", type=int, default=100_000)
    ap.add_argument("--reads", type=int, default=500_000)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lift_rate.json"))
    a = ap.parse_args()
    import torch

    pkg = import_package()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ug, paths = ring(torch, dev, pkg, eng, a.unitigs, a.reads, a.steps, 7)
    ns, nr, ne, t = paths.n_steps, a.reads, ug.n_edges, ug.n_unitigs
    resolved, partner, rs = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    contigs, node_origin, st, lift = ug.untangle_map(eng, resolved, partner)
    res = {"tool": "lift_rate", "reps": a.reps, "ring": {"n_unitigs": t, "n_edges": ne, "n_reads": nr, "n_steps": ns, "resolved": rs["resolved"],
                                                          "copies": st["copies"], "contigs": st["contigs"]}}
    r = res["ring"]
    # the copy places, again, through the raw call
    u = eng.graph_untangle(ug, resolved, partner)
    row_off, dst = eng.graph_adjacency(u["keys"], u["n_copies"])
    o = eng.graph_unitigs(row_off, dst, u["n_copies"])
    place = torch.empty((u["n_copies"], 4), dtype=torch.int32, device=dev)
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    pargs = (eng.ctx, P(o["uni_off"]), P(o["members"]), P(o["circular"]), o["n_unitigs"], u["n_copies"], P(u["origin"]), P(ug.uni_off), P(ug.circular), t, P(place))
    torch.cuda.synchronize(dev)
    _, ms_p = timed(torch, dev, lambda: eng._check(eng.lib.s2k_unitig_copy_places(*pargs)), a.reps, a.warmup)
    r["copy_places"] = summary(ms_p, u["n_copies"])
    assert torch.equal(place, lift.copy_place)
    # the lift: sizes only, then writing
    i = pkg.ThreadOut()
    i.capacity = ns
    for f in ("path_off",) + pkg.ReadPaths.STEP_FIELDS:
        setattr(i, f, getattr(paths, f).data_ptr())
    tot = [ctypes.c_uint64(0) for _ in range(4)]
    tail = tuple(ctypes.byref(x) for x in tot)
    largs = (eng.ctx, nr, ctypes.byref(i), ns, None, P(ug.row_off), P(ug.dst), ne, P(ug.uni_off), P(ug.circular), t, P(resolved), P(partner), P(lift.copy_off),
             P(lift.copy_place), lift.n_copies, lift.n_contigs)
    lo = pkg.ThreadOut()
    bufs = {"path_off": torch.empty(nr + 1, dtype=torch.int64, device=dev)}
    lo.path_off = bufs["path_off"].data_ptr()
    torch.cuda.synchronize(dev)
    _, ms_s = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_lift(*largs, ctypes.byref(lo), None, None, None, None, *tail)), a.reps, a.warmup)
    r["lift_sizes_only"] = summary(ms_s, ns)
    cap = int(tot[0].value)
    lo.capacity = cap
    for f in pkg.ReadPaths.STEP_FIELDS + ("matched",):
        bufs[f] = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        if f != "matched":
            setattr(lo, f, bufs[f].data_ptr())
    bufs["join"] = torch.empty(ns, dtype=torch.uint8, device=dev)
    bufs["step_copy"] = torch.empty(ns, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    fn = lambda: eng._check(eng.lib.s2k_paths_lift(*largs, ctypes.byref(lo), P(bufs["matched"]), P(bufs["step_copy"]), P(bufs["join"]), None, *tail))  # noqa: E731
    _, ms_w = timed(torch, dev, fn, a.reps, a.warmup)
    r["lift"] = summary(ms_w, ns)
    r["lift"].update(n_out_steps=cap, n_merged=int(tot[1].value), n_dropped=int(tot[2].value), n_conflicts=int(tot[3].value))
    # the yardstick on the same paths: s2k_paths_bridge, writing
    bo = pkg.ThreadOut()
    bb = {"path_off": torch.empty(nr + 1, dtype=torch.int64, device=dev)}
    for f in pkg.ReadPaths.STEP_FIELDS + ("matched",):
        bb[f] = torch.empty(ns, dtype=torch.int32, device=dev)
    bb["join"] = torch.empty(ns, dtype=torch.uint8, device=dev)
    bo.capacity = ns
    for f, x in bb.items():
        if f not in ("matched", "join"):
            setattr(bo, f, x.data_ptr())
    bt = [ctypes.c_uint64(0) for _ in range(3)]
    bargs = (eng.ctx, nr, ctypes.byref(i), ns, P(ug.row_off), P(ug.dst), ne, P(ug.uni_off), P(ug.circular), t, 16, 2, ctypes.byref(bo), P(bb["matched"]),
             P(bb["join"]), *(ctypes.byref(x) for x in bt))
    torch.cuda.synchronize(dev)
    _, ms_b = timed(torch, dev, lambda: eng._check(eng.lib.s2k_paths_bridge(*bargs)), a.reps, a.warmup)
    r["bridge"] = summary(ms_b, ns)
    r["bridge"].update(n_out_steps=int(bt[0].value), n_merged=int(bt[1].value), n_bridged=int(bt[2].value))
    r["lift_to_bridge"] = round(statistics.median(ms_w) / statistics.median(ms_b), 3)
    r["lift_sizes_only_to_bridge"] = round(statistics.median(ms_s) / statistics.median(ms_b), 3)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
