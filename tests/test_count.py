"""Downstream k-min-mer counting (the consumer hinted at in src/lib.rs:256-257).  Oracle = a dictionary
over the oracle's k-min-mer hashes.  GPU: s2k_count_device / s2k_partition_device through the C ABI; multi-GPU logic
(partition by hash prefix -> all-to-all -> local count) rehearsed with two gloo ranks -- on the CPU with numpy stand-ins
for the two device ops, and on one GPU with the real ones."""
import importlib.util
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

pkg = import_package()
spec = importlib.util.spec_from_file_location("s2k_sharding", os.path.join(ROOT, "rust-seq2kminmers_amd", "sharding.py"))
sharding = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sharding)


class NumpyCountOps:
    """test stand-in for the two device ops (same contract as sharding.EngineCountOps), CPU tensors"""

    def partition(self, keys, n_parts):
        import torch

        k = keys.numpy().view(np.uint64)
        part = ((k.astype(object) * n_parts) >> 64).astype(np.int64) if len(k) else np.zeros(0, dtype=np.int64)
        order = np.argsort(part, kind="stable")
        off = np.zeros(n_parts + 1, dtype=np.int64)
        np.cumsum(np.bincount(part, minlength=n_parts), out=off[1:])
        return torch.from_numpy(k[order].view(np.int64).copy()), torch.from_numpy(off)

    def count(self, keys, want_pairs=False):
        import torch

        u, c = np.unique(keys.numpy().view(np.uint64), return_counts=True)
        return len(u), torch.from_numpy(u.view(np.int64).copy()), torch.from_numpy(c.astype(np.int32))


def _worker(rank, world, port, gpu, q):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.default_rng(5)
    allk = rng.integers(0, 2 ** 64, size=60000, dtype=np.uint64)
    allk[::7] = allk[3]                                   # a heavy hitter
    allk[1::11] = rng.integers(0, 50, size=len(allk[1::11]), dtype=np.uint64)  # tiny values: all in part 0
    allk[5] = np.uint64(2 ** 64 - 1)                      # the table's EMPTY sentinel is a legal key
    mine = allk[rank::world].copy()
    if gpu:
        dev = torch.device("cuda", 0)
        eng = pkg.Engine(0)
        ops = sharding.EngineCountOps(eng, dev)
        keys = torch.from_numpy(mine.view(np.int64)).to(dev)
    else:
        ops = NumpyCountOps()
        keys = torch.from_numpy(mine.view(np.int64))
    r = sharding.count_kminmers(keys, ops, dist, collectives_on_device=False, want_pairs=True)
    k = r["keys"].cpu().numpy().view(np.uint64)
    c = r["counts"].cpu().numpy()
    lo = [(int(x) * world) >> 64 for x in k]
    assert all(p == rank for p in lo), "a rank must own exactly its range of the hash space"
    q.put((rank, r["n_keys"], r["n_distinct"], dict(zip(k.tolist(), c.tolist()))))
    dist.destroy_process_group()


def _run_two_ranks(gpu):
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, gpu, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = [q.get(timeout=300) for _ in ps]
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    rng = np.random.default_rng(5)
    allk = rng.integers(0, 2 ** 64, size=60000, dtype=np.uint64)
    allk[::7] = allk[3]
    allk[1::11] = rng.integers(0, 50, size=len(allk[1::11]), dtype=np.uint64)
    allk[5] = np.uint64(2 ** 64 - 1)
    u, c = np.unique(allk, return_counts=True)
    want = dict(zip(u.tolist(), c.tolist()))
    merged = {}
    for _, n_keys, n_distinct, d in res:
        assert n_keys == len(allk) and n_distinct == len(want)
        assert not (set(d) & set(merged))  # ranges are disjoint
        merged.update(d)
    assert merged == want


def test_exchange_by_hash_prefix_two_ranks_cpu():
    _run_two_ranks(False)


@pytest.mark.gpu
def test_exchange_by_hash_prefix_two_ranks_one_gpu():
    _run_two_ranks(True)


@pytest.mark.gpu
def test_count_device_matches_dictionary(oracle, ecoli):
    import torch

    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    ops = sharding.EngineCountOps(eng, dev)
    # k-min-mers of a read set with repeats: the same genome window sequenced many times (what a counting consumer sees)
    rng = np.random.default_rng(9)
    reads = [bytes(ecoli[a: a + 3000]) for a in rng.integers(0, len(ecoli) - 3000, size=400)]
    got = eng.extract_reads(reads, 21, 3, 0.05, pkg.HashMode.Hpc)
    ref = oracle.batch(*pkg.pack_reads(reads), 21, 3, 0.05, 1)
    assert (got["hash"] == ref["hash"]).all()
    want = {}
    for h in ref["hash"].tolist():
        want[h] = want.get(h, 0) + 1
    assert len(want) < len(ref["hash"])  # duplicates exist
    keys = torch.from_numpy(got["hash"].view(np.int64)).to(dev)
    r = sharding.count_kminmers(keys, ops, want_pairs=True)
    assert r["n_distinct"] == len(want) and r["n_keys"] == len(ref["hash"])
    assert dict(zip(r["keys"].cpu().numpy().view(np.uint64).tolist(), r["counts"].cpu().numpy().tolist())) == want
    # sizes only, capacity too small, empty input, partition contract
    assert eng.count_device(keys.data_ptr(), keys.numel()) == len(want)
    k2 = torch.zeros(4, dtype=torch.int64, device=dev)
    c2 = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(pkg.S2kError) as e:
        eng.count_device(keys.data_ptr(), keys.numel(), k2.data_ptr(), c2.data_ptr(), 4)
    assert e.value.status == 7
    assert eng.count_device(0, 0) == 0
    for parts in (1, 3, 8, 64):
        g, off = ops.partition(keys, parts)
        off = off.numpy()
        assert off[0] == 0 and off[-1] == keys.numel() and (np.diff(off) >= 0).all()
        gk = g.cpu().numpy().view(np.uint64)
        assert sorted(gk.tolist()) == sorted(got["hash"].tolist())
        for p in range(parts):
            seg = gk[off[p]: off[p + 1]]
            assert all(((int(x) * parts) >> 64) == p for x in seg)


# ---- s2k_count_device / s2k_partition_device at their seams: second trips of the grid-stride loops, the probe sequence wrapping
# ---- round the table's end, every output form, capacities at the edge ---------------------------------------------------------
M64 = (1 << 64) - 1
GUARD, MARK64, MARK32 = 8, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def _count(eng, keys, want_keys=True, want_counts=True, capacity=None):
    """s2k_count_device on a numpy uint64 array -> (status, n_distinct, keys or None, counts or None); `capacity` entries are offered
    (default: as many as there are distinct keys) and GUARD marked entries behind them must stay as they were"""
    import ctypes as C

    import torch

    dev = torch.device("cuda", 0)
    t = torch.from_numpy(keys.view(np.int64).copy()).to(dev) if len(keys) else None
    if capacity is None:
        capacity = len(np.unique(keys))
    ok = torch.full((capacity + GUARD,), MARK64, dtype=torch.int64, device=dev)
    oc = torch.full((capacity + GUARD,), MARK32, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    nd = C.c_uint64(0)
    st = eng.lib.s2k_count_device(eng.ctx, C.c_void_p(t.data_ptr() if t is not None else 0), len(keys), C.c_void_p(ok.data_ptr() if want_keys else 0),
                                  C.c_void_p(oc.data_ptr() if want_counts else 0), capacity, C.byref(nd))
    k, c = ok.cpu().numpy(), oc.cpu().numpy()
    assert (k[capacity:] == MARK64).all() and (c[capacity:] == MARK32).all(), "guard bands"
    if not want_keys:
        assert (k == MARK64).all()
    if not want_counts:
        assert (c == MARK32).all()
    m = min(capacity, int(nd.value))
    return st, int(nd.value), k[:m].view(np.uint64) if want_keys else None, c[:m].view(np.uint32) if want_counts else None


def _as_dict(k, c):
    d = dict(zip(k.tolist(), c.tolist()))
    assert len(d) == len(k), "a key came back twice"
    return d


def _unique_dict(keys):
    u, c = np.unique(keys, return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


@pytest.mark.gpu
def test_count_second_trip_of_the_grid_stride_loops():
    """more than 65 536 x 256 keys: the insert loop takes a second trip, and with more than 2**24 slots the compaction does too"""
    rng = np.random.default_rng(21)
    n = 2 ** 24 + 257
    vals = rng.integers(0, 2 ** 64, size=150000, dtype=np.uint64)
    keys = vals[rng.integers(0, len(vals), size=n)]
    keys[[0, 5, n // 2, n - 256, n - 1]] = np.uint64(M64)  # the table's EMPTY value is a legal key
    keys[[1, n - 2]] = np.uint64(0)
    want = _unique_dict(keys)
    eng = pkg.Engine(0)
    st, nd, k, c = _count(eng, keys, capacity=len(want))
    assert (st, nd) == (0, len(want))
    assert _as_dict(k, c) == want
    assert want[M64] == 5 and want[0] >= 2
    eng.close()


@pytest.mark.gpu
def test_count_contention_on_one_key():
    eng = pkg.Engine(0)
    st, nd, k, c = _count(eng, np.full(2 ** 20, 0x0123456789ABCDEF, dtype=np.uint64))
    assert (st, nd, k.tolist(), c.tolist()) == (0, 1, [0x0123456789ABCDEF], [2 ** 20])
    eng.close()


# White box: the two functions below mirror slot_hash and the `slots` formula of s2k_count_device (s2k_count.hip); the wrap-around
# test needs them to aim keys at the last slots of the table.  If either changes there, the assertion before the device call fails.
def _slot_hash(k):
    k ^= k >> 32
    k = (k * 0x9E3779B97F4A7C15) & M64
    return k ^ (k >> 29)


def _slots(n):
    return (n + n // 2 + 1024 + 255) & ~255


def _keys_homed_in_last_slots(rng, slots, count, last=8):
    out = set()
    while len(out) < count:
        for k in rng.integers(0, 2 ** 64, size=4096, dtype=np.uint64).tolist():
            if (_slot_hash(k) * slots) >> 64 >= slots - last and k != M64 and len(out) < count:
                out.add(k)
    return np.array(sorted(out), dtype=np.uint64)


@pytest.mark.gpu
def test_count_probe_sequence_wraps_round_the_end_of_the_table():
    rng = np.random.default_rng(22)
    eng = pkg.Engine(0)
    mult = rng.integers(1, 6, size=96)
    for reps in (np.ones(96, dtype=np.int64), mult):
        n = int(reps.sum())
        slots = _slots(n)
        distinct = _keys_homed_in_last_slots(rng, slots, 96)
        assert len(distinct) == 96 and all((_slot_hash(k) * slots) >> 64 >= slots - 8 for k in distinct.tolist())  # 96 keys, 8 slots: 88 wrap
        keys = rng.permutation(np.repeat(distinct, reps))
        assert len(keys) == n
        st, nd, k, c = _count(eng, keys)
        assert (st, nd) == (0, 96)
        assert _as_dict(k, c) == dict(zip(distinct.tolist(), reps.tolist()))
    eng.close()


@pytest.mark.gpu
def test_count_output_forms_and_capacity_at_the_edge():
    rng = np.random.default_rng(23)
    keys = rng.integers(0, 2 ** 64, size=5000, dtype=np.uint64)[rng.integers(0, 5000, size=20001)]
    keys[[3, 4, 20000]] = np.uint64(M64)
    want = _unique_dict(keys)
    nd_want = len(want)
    eng = pkg.Engine(0)
    st, nd, k, c = _count(eng, keys, want_counts=False)
    assert (st, nd, c) == (0, nd_want, None) and sorted(k.tolist()) == sorted(want)
    st, nd, k, c = _count(eng, keys, want_keys=False)
    assert (st, nd, k) == (0, nd_want, None) and sorted(c.tolist()) == sorted(want.values())
    for cap in (0, 3, nd_want):  # neither array: the size only, whatever the capacity says
        assert _count(eng, keys, want_keys=False, want_counts=False, capacity=cap) == (0, nd_want, None, None)
    st, nd, k, c = _count(eng, keys, capacity=nd_want)  # exactly enough, the all-ones key (kept beside the table) included
    assert (st, nd) == (0, nd_want) and _as_dict(k, c) == want and want[M64] == 3
    for wk, wc in ((True, True), (True, False), (False, True)):
        st, nd, k, c = _count(eng, keys, want_keys=wk, want_counts=wc, capacity=nd_want - 1)
        assert (st, nd) == (7, nd_want)
        if wk and wc:  # what fits is still pairs of the reference
            assert len(k) == nd_want - 1 and all(want[a] == b for a, b in zip(k.tolist(), c.tolist()))
    assert _count(eng, np.zeros(0, dtype=np.uint64), capacity=0)[:2] == (0, 0)
    eng.close()


@pytest.mark.gpu
def test_count_small_call_after_a_large_one_on_the_same_context():
    rng = np.random.default_rng(24)
    eng = pkg.Engine(0)
    big = rng.integers(0, 2 ** 64, size=300000, dtype=np.uint64)
    small = np.concatenate((big[:500], big[:200], rng.integers(0, 2 ** 64, size=77, dtype=np.uint64)))
    for keys in (big, small, small[:1]):
        st, nd, k, c = _count(eng, keys)
        want = _unique_dict(keys)
        assert (st, nd) == (0, len(want)) and _as_dict(k, c) == want
    eng.close()


def _part_np(k, parts):
    """(k * parts) >> 64 in 64-bit arithmetic (parts <= 64): the Python-int reference, vectorised; checked against it below"""
    k = k.astype(np.uint64)
    p = np.uint64(parts)
    return ((((k & np.uint64(0xFFFFFFFF)) * p) >> np.uint64(32)) + (k >> np.uint64(32)) * p) >> np.uint64(32)


def _partition_keys(rng, n):
    special = [0, M64]
    for parts in (3, 7, 63):
        for p in range(1, parts):
            b = -((-(p << 64)) // parts)  # ceil(2**64 p / parts): the first key of part p
            special += [b, b - 1]
    special = np.array(special, dtype=np.uint64)
    keys = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    if n:
        keys[rng.choice(n, size=len(special), replace=False)] = special
        assert np.isin(special, keys).all()
    return keys


def _partition(eng, keys, parts):
    import torch

    dev = torch.device("cuda", 0)
    n = len(keys)
    t = torch.from_numpy(keys.view(np.int64).copy()).to(dev) if n else None
    out = torch.full((n + GUARD,), MARK64, dtype=torch.int64, device=dev) if n else None
    off = torch.full((parts + 1 + GUARD,), MARK64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng.partition_device(t.data_ptr() if n else 0, n, parts, out.data_ptr() if n else 0, off.data_ptr())
    o = off.cpu().numpy()
    g = out.cpu().numpy() if n else np.zeros(GUARD, dtype=np.int64) + MARK64
    assert (o[parts + 1:] == MARK64).all() and (g[n:] == MARK64).all(), "guard bands"
    return g[:n].view(np.uint64), o[:parts + 1]


def _check_partition(eng, keys, ks, parts):
    """ks = keys sorted"""
    sample = np.concatenate((keys[:300], ks[[0, -1]])) if len(keys) else keys
    assert _part_np(sample, parts).tolist() == [(int(x) * parts) >> 64 for x in sample.tolist()]
    g, off = _partition(eng, keys, parts)
    want_off = np.zeros(parts + 1, dtype=np.int64)
    np.cumsum(np.bincount(_part_np(keys, parts).astype(np.int64), minlength=parts), out=want_off[1:])
    assert (off == want_off).all(), (len(keys), parts)
    # every key of every segment is in its part ...
    assert (_part_np(g, parts).astype(np.int64) == np.repeat(np.arange(parts), np.diff(want_off))).all(), (len(keys), parts)
    # ... and each segment, sorted, is the reference's segment sorted (the order inside a part is unspecified)
    for p in range(parts):
        assert (np.sort(g[want_off[p]:want_off[p + 1]]) == ks[want_off[p]:want_off[p + 1]]).all(), (len(keys), parts, p)


@pytest.mark.gpu
def test_partition_every_key_in_its_part():
    rng = np.random.default_rng(25)
    eng = pkg.Engine(0)
    for n in (16384 * 256 + 77, 255, 256, 257, 0):  # the first: a second trip of the histogram and scatter loops
        keys = _partition_keys(rng, n)
        ks = np.sort(keys)
        for parts in (1, 2, 3, 7, 63, 64):
            _check_partition(eng, keys, ks, parts)
    # all keys in one part of 64
    lo = -((-(17 << 64)) // 64)
    one = (np.uint64(lo) + rng.integers(0, 2 ** 58, size=70001, dtype=np.uint64)).astype(np.uint64)
    assert set(_part_np(one, 64).tolist()) == {17}
    _check_partition(eng, one, np.sort(one), 64)
    import torch

    off = torch.zeros(80, dtype=torch.int64, device="cuda")
    t = torch.zeros(16, dtype=torch.int64, device="cuda")
    for parts in (0, 65):
        with pytest.raises(pkg.S2kError) as e:
            eng.partition_device(t.data_ptr(), 16, parts, t.data_ptr(), off.data_ptr())
        assert e.value.status == 1
    eng.close()
