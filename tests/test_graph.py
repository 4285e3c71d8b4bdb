"""The minimizer-space graph on the device: s2k_table_edges (the edge keys the reads traverse) and s2k_graph_adjacency (the CSR of a
sorted edge table), include/s2k.h, DESIGN.md §3.9.  The contracts: the edge keys equal `edges_reference` byte for byte, order
included; the CSR equals `adjacency_reference`; end to end, KminmerGraph.build equals the references run on the oracle's k-min-mers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

pkg = import_package()

SYMS = ("s2k_table_edges", "s2k_graph_adjacency")
M32 = np.uint64(0xFFFFFFFF)


def edges_reference(km_off, hash_, rev, keys, counts, min_count):
    """-> uint64 edge keys in emission order: for items j, j + 1 of one read whose hashes are both in the table (keys strictly
    ascending; counts None: 1 per key) with a count of at least max(min_count, 1), key(e) = u << 32 | v (u = 2 * index + rev), then
    key(twin(e)) = (v ^ 1) << 32 | u ^ 1 unless twin(e) == e"""
    km_off = np.asarray(km_off, dtype=np.uint64)
    h = np.asarray(hash_, dtype=np.uint64)
    rv = np.asarray(rev, dtype=np.uint64)
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(h)
    if n < 2 or len(keys) == 0:
        return np.zeros(0, dtype=np.uint64)
    i = np.searchsorted(keys, h)
    ic = np.minimum(i, len(keys) - 1)
    hit = (i < len(keys)) & (keys[ic] == h)
    cnt = np.ones(len(keys), dtype=np.uint32) if counts is None else np.asarray(counts, dtype=np.uint32)
    solid = hit & (cnt[ic] >= max(int(min_count), 1))
    return edges_from_ranks(km_off, ic, solid, rv)


def edges_from_ranks(km_off, rank, solid, rv):
    """edges_reference given each item's table index (rank) and whether it is solid"""
    km_off = np.asarray(km_off, dtype=np.uint64)
    n = len(rank)
    u = 2 * rank.astype(np.uint64) + np.asarray(rv, dtype=np.uint64)
    start = np.zeros(n + 1, dtype=bool)
    start[km_off.astype(np.int64)] = True  # item x starts a read (an empty read marks the item after it)
    j = np.nonzero(solid[:-1] & solid[1:] & ~start[1:n])[0]
    a, b = u[j], u[j + 1]
    two = b != (a ^ np.uint64(1))
    slot = np.concatenate([[0], np.cumsum(1 + two.astype(np.int64))])
    out = np.zeros(int(slot[-1]), dtype=np.uint64)
    out[slot[:-1]] = (a << np.uint64(32)) | b
    out[slot[:-1][two] + 1] = ((b[two] ^ np.uint64(1)) << np.uint64(32)) | (a[two] ^ np.uint64(1))
    return out


def edges_loop(km_off, hash_, rev, keys, counts, min_count):
    """edges_reference as a plain loop, for the CPU tier"""
    pos = {int(k): x for x, k in enumerate(keys)}
    cnt = {int(k): (1 if counts is None else int(c)) for k, c in zip(keys, counts if counts is not None else keys)}
    mc = max(int(min_count), 1)
    out = []
    for r in range(len(km_off) - 1):
        for j in range(int(km_off[r]), int(km_off[r + 1]) - 1):
            x, y = int(hash_[j]), int(hash_[j + 1])
            if x in pos and y in pos and cnt[x] >= mc and cnt[y] >= mc:
                u, v = 2 * pos[x] + int(rev[j]), 2 * pos[y] + int(rev[j + 1])
                out.append(u << 32 | v)
                if v != u ^ 1:
                    out.append((v ^ 1) << 32 | (u ^ 1))
    return np.array(out, dtype=np.uint64)


def adjacency_reference(edge_keys, n_nodes):
    """-> (row_off uint64[2 n_nodes + 1], dst uint32[n_edges]) of strictly ascending edge keys"""
    ek = np.asarray(edge_keys, dtype=np.uint64)
    src = ek >> np.uint64(32)
    row_off = np.searchsorted(src, np.arange(2 * n_nodes + 1, dtype=np.uint64), side="left").astype(np.uint64)
    return row_off, (ek & M32).astype(np.uint32)


def graph_reference(batches, min_count, min_edge_count=1):
    """the KminmerGraph of extraction results (dicts of host arrays km_off, hash, rev), from the references"""
    allh = np.concatenate([np.asarray(b["hash"], dtype=np.uint64) for b in batches])
    keys, counts = np.unique(allh, return_counts=True)
    m = counts >= max(min_count, 1)
    keys, counts = keys[m], counts[m].astype(np.uint32)
    e = np.concatenate([edges_reference(b["km_off"], b["hash"], b["rev"], keys, counts, min_count) for b in batches])
    ek, ec = np.unique(e, return_counts=True)
    m = ec >= max(min_edge_count, 1)
    ek, ec = ek[m], ec[m].astype(np.uint32)
    row_off, dst = adjacency_reference(ek, len(keys))
    return {"keys": keys, "counts": counts, "edge_keys": ek, "edge_counts": ec, "row_off": row_off, "dst": dst}


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS, s
    assert hasattr(pkg.CountTable, "edges") and hasattr(pkg.Engine, "graph_adjacency")
    for m in ("build", "write_gfa"):
        assert hasattr(pkg.KminmerGraph, m)


def test_cpp_graph_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "graph_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "graph_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def _k(u, v):
    return (u << 32) | v


def test_references_hand_made():
    keys, counts = [10, 20, 30], [2, 2, 1]
    # a hairpin (A+ then A-): its own twin, one key
    assert edges_reference([0, 2], [10, 10], [0, 1], keys, counts, 2).tolist() == [_k(0, 1)]
    assert edges_reference([0, 2], [20, 20], [1, 0], keys, counts, 2).tolist() == [_k(3, 2)]
    # a loop (A+ then A+): a distinct twin (A- -> A-)
    assert edges_reference([0, 2], [10, 10], [0, 0], keys, counts, 2).tolist() == [_k(0, 0), _k(1, 1)]
    # an ordinary edge and its twin
    assert edges_reference([0, 2], [10, 20], [0, 1], keys, counts, 2).tolist() == [_k(0, 3), _k(2, 1)]
    # empty and one-item reads: no edge between reads
    km_off = [0, 0, 1, 1, 3, 3]
    assert edges_reference(km_off, [10, 20, 10], [0, 0, 0], keys, counts, 2).tolist() == [_k(2, 0), _k(1, 3)]
    assert edges_reference([0, 1, 2, 3], [10, 20, 10], [0, 0, 0], keys, counts, 2).tolist() == []
    # a non-solid item between two solid ones breaks the chain: absent, or under the cutoff
    assert edges_reference([0, 3], [10, 99, 20], [0, 0, 0], keys, counts, 1).tolist() == []
    assert edges_reference([0, 3], [10, 30, 20], [0, 0, 0], keys, counts, 2).tolist() == []
    for mc in (0, 1):
        assert edges_reference([0, 3], [10, 30, 20], [0, 0, 0], keys, counts, mc).tolist() == [_k(0, 4), _k(5, 1), _k(4, 2), _k(3, 5)]
    # a membership table (counts None)
    assert edges_reference([0, 2], [10, 30], [1, 1], keys, None, 1).tolist() == [_k(1, 5), _k(4, 0)]
    # random, against the loop; every twin present
    rng = np.random.default_rng(3)
    kk = np.unique(rng.integers(0, 2 ** 64, size=300, dtype=np.uint64))
    cc = rng.integers(1, 4, size=len(kk)).astype(np.uint32)
    lens = rng.integers(0, 9, size=300)
    km = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(km[-1])
    h = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    m = rng.random(n) < 0.85
    h[m] = kk[rng.integers(0, 40, size=int(m.sum()))]  # few nodes: loops and hairpins occur
    rv = rng.integers(0, 2, size=n).astype(np.uint8)
    for mc in (0, 2, 3):
        got = edges_reference(km, h, rv, kk, cc, mc)
        assert got.tobytes() == edges_loop(km, h, rv, kk, cc, mc).tobytes()
        u, v = got >> np.uint64(32), got & M32
        twin = ((v ^ np.uint64(1)) << np.uint64(32)) | (u ^ np.uint64(1))
        assert np.array_equal(np.sort(got), np.sort(twin))
    # adjacency: empty rows, node 0 and the last node
    ek = np.array([_k(0, 1), _k(0, 5), _k(3, 0), _k(5, 5)], dtype=np.uint64)
    ro, dst = adjacency_reference(ek, 3)
    assert ro.tolist() == [0, 2, 2, 2, 3, 3, 4] and dst.tolist() == [1, 5, 0, 5]
    ro, dst = adjacency_reference(np.zeros(0, dtype=np.uint64), 2)
    assert ro.tolist() == [0] * 5 and len(dst) == 0


def _gfa_lines(path):
    return [line.rstrip("\n").split("\t") for line in open(path)]


def test_write_gfa_hand_made(tmp_path):
    keys = np.array([0xA, 0xB, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    counts = np.array([3, 4, 5], dtype=np.uint32)
    # read 1: A+ B+ ; read 2: B- A- (the same adjacency, other strand) ; read 3: A+ A- (hairpin) ; read 4: B+ B+ (loop) ; C- A+
    km_off = [0, 2, 4, 6, 8, 10]
    h = [0xA, 0xB, 0xB, 0xA, 0xA, 0xA, 0xB, 0xB, 0xFFFFFFFFFFFFFFFF, 0xA]
    rv = [0, 0, 1, 1, 0, 1, 0, 0, 1, 0]
    e = edges_reference(km_off, h, rv, keys, counts, 1)
    ek, ec = np.unique(e, return_counts=True)
    path = str(tmp_path / "g.gfa")
    pkg.write_gfa(path, keys, counts, ek, ec.astype(np.uint32))
    lines = _gfa_lines(path)
    s = [x for x in lines if x[0] == "S"]
    assert s == [["S", "0", "*", "KC:i:3", "kh:Z:000000000000000a"], ["S", "1", "*", "KC:i:4", "kh:Z:000000000000000b"],
                 ["S", "2", "*", "KC:i:5", "kh:Z:ffffffffffffffff"]]
    links = sorted(tuple(x[1:]) for x in lines if x[0] == "L")
    assert links == sorted([("0", "+", "1", "+", "*", "RC:i:2"),   # A+ -> B+ (and B- -> A-), seen twice
                            ("0", "+", "0", "-", "*", "RC:i:1"),   # the hairpin, its own twin
                            ("1", "+", "1", "+", "*", "RC:i:1"),   # the loop (its twin B- -> B- not written again)
                            ("0", "-", "2", "+", "*", "RC:i:1")])  # C- -> A+ is written as its twin A- -> C+ (the smaller key)
    # one L line per twin pair
    u, v = ek >> np.uint64(32), ek & M32
    pairs = {min(int(k), int(((b ^ 1) << 32) | (a ^ 1))) for k, a, b in zip(ek, u, v)}
    assert len(links) == len(pairs)


def _sample_reads(ecoli, n, seed, lo=2000, hi=4000):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi))
        a = int(rng.integers(0, len(ecoli) - L))
        out.append(bytes(ecoli[a:a + L]))
    return out


_COMP = np.zeros(256, dtype=np.uint8)
_COMP[list(b"ACGTN")] = list(b"TGCAN")


def _revcomp(r):
    return bytes(_COMP[np.frombuffer(r, dtype=np.uint8)][::-1])


def test_oracle_regular_edges_strand_symmetric(oracle, ecoli):
    """Regular: the edge multiset of a read set equals that of its reverse complements (Hpc drops the last l-mer of a read, so it is
    not strand-symmetric at read ends and is not checked)"""
    reads = _sample_reads(ecoli, 150, 5)
    rc = [_revcomp(r) for r in reads]
    for l, k, d in ((21, 3, 0.05), (12, 5, 0.05)):
        a = oracle.batch(*pkg.pack_reads(reads), l, k, d, int(pkg.HashMode.Regular))
        b = oracle.batch(*pkg.pack_reads(rc), l, k, d, int(pkg.HashMode.Regular))
        ga, gb = graph_reference([a], 1), graph_reference([b], 1)
        assert len(ga["edge_keys"]) > 1000
        for f in ga:
            assert np.array_equal(ga[f], gb[f]), (l, k, f)


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def _dev(x, dt):
    import torch

    x = np.ascontiguousarray(x)
    if len(x) == 0:
        return torch.zeros(1, dtype=dt, device="cuda:0")[:0]
    view = {torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8}[dt]
    return torch.from_numpy(x.view(view).copy()).to("cuda:0")


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _table(eng, keys, counts):
    import torch

    dk = _dev(np.asarray(keys, dtype=np.uint64), torch.int64)
    dc = None if counts is None else _dev(np.asarray(counts, dtype=np.uint32), torch.int32)
    return pkg.CountTable(eng, dk, dc)


def _raw_edges(eng, t, km_off, h, rv, mc, capacity=None, keys_out=True, guard=16, null=()):
    """s2k_table_edges through ctypes; the key array gets `guard` extra slots and every slot a marker -> (status, n_edges, keys)"""
    import torch

    n = int(km_off[-1])
    d = {"km_off": _dev(np.asarray(km_off, dtype=np.uint64), torch.int64),
         "hash": _dev(h, torch.int64) if n else torch.zeros(1, dtype=torch.int64, device="cuda:0"),
         "rev": _dev(np.asarray(rv, dtype=np.uint8), torch.uint8) if n else torch.zeros(1, dtype=torch.uint8, device="cuda:0")}
    i = pkg.DeviceOut()
    i.km_capacity = n
    for f in ("km_off", "hash", "rev"):
        setattr(i, f, None if f in null else d[f].data_ptr())
    cap = 2 * n if capacity is None else capacity
    out = torch.full((cap + guard,), -0x5A5A, dtype=torch.int64, device="cuda:0")
    ne = ctypes.c_uint64(12345)
    torch.cuda.synchronize()
    s = eng.lib.s2k_table_edges(ctypes.c_void_p(t.handle), len(km_off) - 1, ctypes.byref(i), mc,
                                ctypes.c_void_p(out.data_ptr()) if keys_out else None, cap, ctypes.byref(ne))
    return s, ne.value, out.cpu().numpy()


def _random_table(rng, n):
    u = np.unique(rng.integers(0, 2 ** 64, size=n + n // 4 + 16, dtype=np.uint64))[:n]
    return u, rng.integers(1, 5, size=len(u)).astype(np.uint32)


def _items(rng, km_off, keys, frac=0.85, pool=None):
    n = int(km_off[-1])
    h = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    m = rng.random(n) < frac
    src = keys if pool is None else keys[:pool]
    h[m] = src[rng.integers(0, len(src), size=int(m.sum()))]
    return h, rng.integers(0, 2, size=n).astype(np.uint8)


def _check_edges(eng, t, keys, cnt, km_off, h, rv, mc):
    s, ne, got = _raw_edges(eng, t, km_off, h, rv, mc)
    want = edges_reference(km_off, h, rv, keys, cnt, mc)
    assert (s, ne) == (0, len(want)), (s, ne, len(want), mc)
    assert got[:ne].view(np.uint64).tobytes() == want.tobytes(), mc
    assert (got[ne:] == -0x5A5A).all()
    return want


@pytest.mark.gpu
def test_edges_hand_made_reads_every_cutoff(eng):
    rng = np.random.default_rng(31)
    keys, cnt = _random_table(rng, 3000)
    t = _table(eng, keys, cnt)
    # read boundaries at items 2047 and 2048 (the first tile boundary), at 4096 after empty reads, 6143 / 6144; one read across
    # several tiles; empty and one-item reads; random short reads; a last read that runs to the batch's last item
    lens = [2047, 1, 2048, 0, 0, 2047, 1, 1, 0, 5000, 1, 0, 2, 3] + list(rng.integers(0, 30, size=1500)) + [0, 700]
    km_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    assert {2047, 2048, 4096, 6143, 6144} <= set(km_off.tolist())
    h, rv = _items(rng, km_off, keys, pool=50)  # few distinct nodes: loops and hairpins occur
    h[-2:] = keys[cnt == 4][:1]  # the last two items: one solid node, an adjacency at the batch's end
    h[2046:2050] = keys[cnt == 4][1]  # a solid run across the read boundaries at 2047 and 2048
    u, v = (int(2 * np.searchsorted(keys, h[x]) + rv[x]) for x in (-2, -1))
    tail = [_k(u, v)] + ([_k(v ^ 1, u ^ 1)] if v != u ^ 1 else [])
    for mc in (0, 1, 2, 3, 4, 5):
        w = _check_edges(eng, t, keys, cnt, km_off, h, rv, mc)
        if mc == 5:
            assert len(w) == 0
        else:
            assert w[-len(tail):].tolist() == tail  # the adjacency of the batch's last two items
    t.close()
    # a membership table, every item present; and an empty table
    t = _table(eng, keys, None)
    hk = keys[rng.integers(0, 200, size=len(h))]
    _check_edges(eng, t, keys, None, km_off, hk, rv, 1)
    t.close()
    t = _table(eng, np.zeros(0, dtype=np.uint64), None)
    _check_edges(eng, t, np.zeros(0, dtype=np.uint64), None, km_off, h, rv, 0)
    t.close()
    # tiles of only single-item and empty reads; many empty reads inside one tile
    t = _table(eng, keys, cnt)
    for lens in ([1] * 5000, [0, 1] * 3000 + [0] * 20000 + [3, 0, 0, 2], [3] * 2000, [2048] * 3):
        km_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        h, rv = _items(rng, km_off, keys, frac=0.95, pool=30)
        _check_edges(eng, t, keys, cnt, km_off, h, rv, 1)
    t.close()


@pytest.mark.gpu
def test_edges_sizes_capacity_and_refusals(eng):
    rng = np.random.default_rng(32)
    keys, cnt = _random_table(rng, 2000)
    t = _table(eng, keys, cnt)
    km_off = np.concatenate([[0], np.cumsum(rng.integers(0, 40, size=300))]).astype(np.uint64)
    h, rv = _items(rng, km_off, keys, pool=100)
    want = edges_reference(km_off, h, rv, keys, cnt, 2)
    ne_want = len(want)
    assert ne_want > 100
    # sizes only
    s, ne, got = _raw_edges(eng, t, km_off, h, rv, 2, keys_out=False)
    assert (s, ne) == (0, ne_want) and (got == -0x5A5A).all()
    # one short: S2K_ERR_CAPACITY with the size, nothing written
    s, ne, got = _raw_edges(eng, t, km_off, h, rv, 2, capacity=ne_want - 1)
    assert (s, ne) == (7, ne_want) and (got == -0x5A5A).all()
    # exactly enough
    s, ne, got = _raw_edges(eng, t, km_off, h, rv, 2, capacity=ne_want, guard=40)
    assert (s, ne) == (0, ne_want) and got[:ne].view(np.uint64).tobytes() == want.tobytes() and (got[ne:] == -0x5A5A).all()
    # NULL arrays refused, n_edges set to 0
    for f in ("km_off", "hash", "rev"):
        s, ne, got = _raw_edges(eng, t, km_off, h, rv, 2, null=(f,))
        assert (s, ne) == (1, 0) and (got == -0x5A5A).all(), f
    ne = ctypes.c_uint64(9)
    i = pkg.DeviceOut()
    assert eng.lib.s2k_table_edges(None, 1, ctypes.byref(i), 1, None, 0, ctypes.byref(ne)) == 1 and ne.value == 0
    assert eng.lib.s2k_table_edges(ctypes.c_void_p(t.handle), 1, None, 1, None, 0, ctypes.byref(ne)) == 1
    assert eng.lib.s2k_table_edges(ctypes.c_void_p(t.handle), 1, ctypes.byref(i), 1, None, 0, None) == 1
    # km_off must start at 0
    s, ne, _ = _raw_edges(eng, t, km_off + np.uint64(1), np.concatenate([h, h[:1]]), np.concatenate([rv, rv[:1]]), 2)
    assert s == 1
    # no items
    for ko in ([0], [0, 0], [0, 0, 0]):
        s, ne, got = _raw_edges(eng, t, np.array(ko, dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint8), 1)
        assert (s, ne) == (0, 0) and (got == -0x5A5A).all()
    t.close()


def _raw_adjacency(eng, ek, n_nodes, want_dst=True, guard=8):
    import torch

    d = _dev(np.asarray(ek, dtype=np.uint64), torch.int64)
    ro = torch.full((2 * n_nodes + 1 + guard,), -3, dtype=torch.int64, device="cuda:0")
    dst = torch.full((len(ek) + guard,), -3, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    s = eng.lib.s2k_graph_adjacency(eng.ctx, ctypes.c_void_p(d.data_ptr()) if len(ek) else None, len(ek), n_nodes,
                                    ctypes.c_void_p(ro.data_ptr()), ctypes.c_void_p(dst.data_ptr()) if want_dst else None)
    return s, ro.cpu().numpy(), dst.cpu().numpy()


def _random_edge_table(rng, n_nodes, m):
    """about m distinct edge keys over 2 n_nodes oriented ids, the smallest and the largest key among them (none when m == 0)"""
    ids = 2 * n_nodes
    if not m:
        return np.zeros(0, dtype=np.uint64)
    e = np.unique(rng.integers(0, ids, size=m, dtype=np.uint64) << np.uint64(32) | rng.integers(0, ids, size=m, dtype=np.uint64))
    return np.unique(np.concatenate([e, [np.uint64(0), np.uint64(ids - 1) << np.uint64(32) | np.uint64(ids - 1)]]))


def _check_adjacency(eng, e, n_nodes):
    """s2k_graph_adjacency against adjacency_reference, with and without d_dst, guards untouched"""
    ids = 2 * n_nodes
    ro_w, dst_w = adjacency_reference(e, n_nodes)
    for want_dst in (True, False):
        s, ro, dst = _raw_adjacency(eng, e, n_nodes, want_dst)
        assert s == 0
        assert ro[:ids + 1].view(np.uint64).tobytes() == ro_w.tobytes() and (ro[ids + 1:] == -3).all()
        if want_dst:
            assert dst[:len(e)].view(np.uint32).tobytes() == dst_w.tobytes() and (dst[len(e):] == -3).all()
        else:
            assert (dst == -3).all()


@pytest.mark.gpu
def test_adjacency_random_tables_and_refusals(eng):
    rng = np.random.default_rng(33)
    for n_nodes, m in ((1, 3), (3, 5), (1000, 3000), (1000, 30), (200000, 900000), (3, 0)):
        _check_adjacency(eng, _random_edge_table(rng, n_nodes, m), n_nodes)
    # an unsorted table, a duplicate, and node ids out of range are refused with nothing written
    e = np.unique(rng.integers(0, 2000, size=5000, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 2000, size=5000, dtype=np.uint64))
    bad = []
    x = e.copy()
    x[[700, 701]] = x[[701, 700]]
    bad.append(x)
    x = e.copy()
    x[300] = x[299]
    bad.append(x)
    x = e.copy()
    x[-1] = np.uint64(2000) << np.uint64(32)  # source == 2 * n_nodes
    bad.append(x)
    x = e.copy()
    x[0] = (x[0] & ~M32) | np.uint64(2000)  # destination == 2 * n_nodes (still ascending)
    bad.append(np.sort(x))
    for x in bad:
        s, ro, dst = _raw_adjacency(eng, x, 1000)
        assert s == 1 and (ro == -3).all() and (dst == -3).all()
    s, ro, dst = _raw_adjacency(eng, e, 1000)
    assert s == 0
    assert eng.lib.s2k_graph_adjacency(eng.ctx, None, 5, 10, None, None) == 1
    assert eng.lib.s2k_graph_adjacency(None, None, 0, 10, None, None) == 1


def _extract_dev(eng, reads, l, k, d, mode):
    import torch

    bases, off = pkg.pack_reads(reads)
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(bases.copy()).to(dev)
    do = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    cap = len(bases) + 1
    t = {"km_off": torch.empty(len(reads) + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
         "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = cap
    o.km_off, o.hash, o.rev = (t[x].data_ptr() for x in ("km_off", "hash", "rev"))
    torch.cuda.synchronize()
    eng.extract_device(db.data_ptr(), do.data_ptr(), len(reads), len(bases), l, k, d, int(mode), o)
    return t


def _graph_host(g):
    return {"keys": _u64(g.keys), "counts": g.counts.cpu().numpy().view(np.uint32), "edge_keys": _u64(g.edge_keys),
            "edge_counts": g.edge_counts.cpu().numpy().view(np.uint32), "row_off": _u64(g.row_off), "dst": g.dst.cpu().numpy().view(np.uint32)}


def _assert_graph(got, want, tag):
    for f in want:
        assert got[f].tobytes() == np.asarray(want[f], dtype=got[f].dtype).tobytes(), (tag, f)


@pytest.mark.gpu
def test_build_matches_oracle_references(eng, oracle, ecoli):
    """ecoli-sampled reads in three batches, Hpc and Regular: extract_device -> KminmerGraph.build == the references on the oracle's
    k-min-mers (node table, CSR, edge counts), at two edge cutoffs; the graph of the three batches == the graph of one"""
    rng = np.random.default_rng(9)
    reads = [bytes(ecoli[a: a + 3000]) for a in rng.integers(0, len(ecoli) - 3000, size=400)]
    batches = [reads[:150], reads[150:270], reads[270:]]
    for mode in (pkg.HashMode.Hpc, pkg.HashMode.Regular):
        outs = [_extract_dev(eng, b, 21, 3, 0.05, mode) for b in batches]
        refs = [oracle.batch(*pkg.pack_reads(b), 21, 3, 0.05, int(mode)) for b in batches]
        for mc, mec in ((2, 1), (2, 2), (1, 1)):
            want = graph_reference(refs, mc, mec)
            assert len(want["keys"]) > 100 and len(want["edge_keys"]) > 100
            g = pkg.KminmerGraph.build(eng, outs, min_count=mc, min_edge_count=mec)
            _assert_graph(_graph_host(g), want, (mode, mc, mec))
        one = pkg.KminmerGraph.build(eng, [_extract_dev(eng, reads, 21, 3, 0.05, mode)], min_count=2)
        _assert_graph(_graph_host(one), graph_reference(refs, 2, 1), (mode, "one batch"))


@pytest.mark.gpu
def test_regular_graph_strand_symmetric_on_device(eng, ecoli, tmp_path):
    """Regular: the graph of a read set and of its reverse complements are identical arrays (and identical GFA files)"""
    reads = _sample_reads(ecoli, 300, 7)
    rc = [_revcomp(r) for r in reads]
    for mc in (1, 2):
        ga = pkg.KminmerGraph.build(eng, [_extract_dev(eng, reads, 21, 3, 0.05, pkg.HashMode.Regular)], min_count=mc)
        gb = pkg.KminmerGraph.build(eng, [_extract_dev(eng, rc, 21, 3, 0.05, pkg.HashMode.Regular)], min_count=mc)
        a, b = _graph_host(ga), _graph_host(gb)
        assert len(a["edge_keys"]) > 1000
        _assert_graph(a, b, mc)
        pa, pb = str(tmp_path / "a.gfa"), str(tmp_path / "b.gfa")
        ga.write_gfa(pa)
        gb.write_gfa(pb)
        assert open(pa).read() == open(pb).read()
        n_l = sum(1 for line in open(pa) if line.startswith("L\t"))
        ek = a["edge_keys"]
        twin = ((ek & M32) ^ np.uint64(1)) << np.uint64(32) | ((ek >> np.uint64(32)) ^ np.uint64(1))
        assert np.array_equal(np.sort(twin), ek)  # symmetric
        assert n_l == int((ek <= twin).sum())


@pytest.mark.gpu
def test_full_size_config1_edges(eng):
    """configs[1] (1 000 000 x 10 kbp synthetic reads, l=31 k=10 d=0.01, Hpc) against a table of every second key (min_count 1):
    n_edges, the XOR and the sum of the keys == the numpy reference on the host copy of km_off / hash / rev and the table"""
    import torch

    n_reads, L, seed = 1_000_000, 10_000, 1
    dev = torch.device("cuda", 0)
    d_b = torch.empty(n_reads * L + 64, dtype=torch.uint8, device=dev)
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L
    cap = int(n_reads * L * 0.0215)
    t = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
         "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = cap
    o.km_off, o.hash, o.rev = (t[x].data_ptr() for x in ("km_off", "hash", "rev"))
    torch.cuda.synchronize()
    eng.synth_bases_device(seed, 0, n_reads * L, d_b.data_ptr())
    c = eng.extract_device(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L, 31, 10, 0.01, int(pkg.HashMode.Hpc), o)
    n = c["n_kminmers"]
    del d_b
    assert n > 100 * 10 ** 6
    k = torch.empty(n, dtype=torch.int64, device=dev)
    cc = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    nd, nk = eng.count_device_ex(t["hash"].data_ptr(), n, 1, True, k.data_ptr(), cc.data_ptr(), n)
    half_k, half_c = k[:nk:2].contiguous(), cc[:nk:2].contiguous()
    table = pkg.CountTable(eng, half_k, half_c)
    e = table.edges(t, n_reads, min_count=1)
    table.close()
    ne = e.numel()
    got_sum = int(e.sum()) % 2 ** 64
    got_xor = int(np.bitwise_xor.reduce(_u64(e))) if ne else 0
    del e
    km_off, h, rv = _u64(t["km_off"]), _u64(t["hash"][:n]), t["rev"][:n].cpu().numpy()
    # the index of every hash in the sorted distinct hashes, by one sort (a search per hash would take minutes on the host); the
    # table holds the even indices, at index // 2, every count >= 1
    order = np.argsort(h)
    hs = h[order]
    new = np.ones(n, dtype=bool)
    new[1:] = hs[1:] != hs[:-1]
    full = np.empty(n, dtype=np.int64)
    full[order] = np.cumsum(new) - 1
    del order
    assert hs[new].tobytes() == _u64(k[:nk]).tobytes()
    assert hs[new][::2].tobytes() == _u64(half_k).tobytes()
    del hs, new
    want = edges_from_ranks(km_off, full // 2, full % 2 == 0, rv)
    assert ne == len(want) and ne > 10 ** 6
    assert got_xor == int(np.bitwise_xor.reduce(want))
    assert got_sum == int(want.sum(dtype=np.uint64))
