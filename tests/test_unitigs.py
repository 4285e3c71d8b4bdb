"""Unitigs on the device: s2k_graph_unitigs (the non-branching paths of the minimizer-space graph compacted) and
s2k_graph_unitig_edges (the graph between them), include/s2k.h, DESIGN.md §3.10.  The reference is `unitig_reference`, a serial walk
written from the header's definitions (follow next from every head, then sweep what is left as cycles; no pointer jumping in it);
the device's arrays equal its arrays exactly, every one of them, in every test."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

pkg = import_package()

SYMS = ("s2k_graph_unitigs", "s2k_graph_unitig_edges")
M32 = np.uint64(0xFFFFFFFF)
FIELDS = ("uni_off", "members", "node_unitig", "node_pos", "circular")
DT = {"uni_off": np.uint64, "members": np.uint32, "node_unitig": np.uint32, "node_pos": np.uint32, "circular": np.uint8}


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def csr_of(n_nodes, edges):
    """-> (row_off uint64, dst uint32) of the edge list closed under twins"""
    s = set()
    for u, v in edges:
        s.add((int(u), int(v)))
        s.add((int(v) ^ 1, int(u) ^ 1))
    e = sorted(s)
    src = np.array([a for a, _ in e], dtype=np.uint64)
    row_off = np.searchsorted(src, np.arange(2 * n_nodes + 1, dtype=np.uint64), side="left").astype(np.uint64)
    return row_off, np.array([b for _, b in e], dtype=np.uint32)


def links_of(ro, d, N):
    nxt = [-1] * N
    for u in range(N):
        if ro[u + 1] - ro[u] == 1:
            v = d[ro[u]]
            if v != u and v != u ^ 1 and ro[(v ^ 1) + 1] - ro[v ^ 1] == 1:
                nxt[u] = v
    return nxt


def unitig_reference(row_off, dst, n_nodes):
    """-> dict: uni_off, members, node_unitig, node_pos, circular, n_unitigs, n_links, edge_keys, src_edge (the definitions of
    include/s2k.h, by a serial walk)"""
    ro, d, N = [int(x) for x in row_off], [int(x) for x in dst], 2 * n_nodes
    nxt = links_of(ro, d, N)
    has_prev = [False] * N
    for u in range(N):
        if nxt[u] >= 0:
            assert not has_prev[nxt[u]]  # next is injective
            has_prev[nxt[u]] = True
    seen = [False] * N
    kept = []  # (members, circular)
    for h in range(N):  # chains: from every head
        if has_prev[h]:
            continue
        path = [h]
        while nxt[path[-1]] >= 0:
            path.append(nxt[path[-1]])
        for x in path:
            seen[x] = True
        if h < (path[-1] ^ 1):
            kept.append((path, 0))
    cyc_min, cycles = {}, []
    for u in range(N):  # what is left is cyclic; ascending u, so u is the smallest id of its cycle
        if seen[u]:
            continue
        cyc = [u]
        while nxt[cyc[-1]] != u:
            cyc.append(nxt[cyc[-1]])
        for x in cyc:
            seen[x] = True
        cyc_min[u] = u
        for x in cyc:
            cyc_min[x] = u
        cycles.append(cyc)
    for cyc in cycles:
        if cyc[0] < cyc_min[cyc[0] ^ 1]:
            kept.append((cyc, 1))
    kept.sort(key=lambda k: k[0][0])
    T = len(kept)
    uni_off = np.zeros(T + 1, dtype=np.uint64)
    members = np.zeros(n_nodes, dtype=np.uint32)
    node_unitig, node_pos = np.zeros(n_nodes, dtype=np.uint32), np.zeros(n_nodes, dtype=np.uint32)
    circular = np.zeros(T, dtype=np.uint8)
    first, at = {}, 0
    filled = np.zeros(n_nodes, dtype=bool)
    for t, (path, c) in enumerate(kept):
        uni_off[t] = at
        members[at: at + len(path)] = path
        for p, x in enumerate(path):
            assert not filled[x >> 1]
            filled[x >> 1] = True
            node_unitig[x >> 1], node_pos[x >> 1] = t, p
        circular[t] = c
        first[path[0]] = 2 * t
        first[path[-1] ^ 1] = 2 * t + 1
        at += len(path)
    uni_off[T] = at
    assert at == n_nodes and filled.all()  # every node once
    keys, src = [], []
    for t, (path, _) in enumerate(kept):
        for s, x in ((0, path[-1]), (1, path[0] ^ 1)):
            row = sorted((first[d[e]], e) for e in range(ro[x], ro[x + 1]) if nxt[x] != d[e])
            keys += [((2 * t + s) << 32) | V for V, _ in row]
            src += [e for _, e in row]
    n_links = sum(1 for x in nxt if x >= 0)
    assert len(keys) == len(d) - n_links
    return {"uni_off": uni_off, "members": members, "node_unitig": node_unitig, "node_pos": node_pos, "circular": circular, "n_unitigs": T,
            "n_links": n_links, "edge_keys": np.array(keys, dtype=np.uint64), "src_edge": np.array(src, dtype=np.uint64)}


def is_twin_symmetric(row_off, dst, n_nodes):
    ro, d = [int(x) for x in row_off], [int(x) for x in dst]
    e = {(u, d[i]) for u in range(2 * n_nodes) for i in range(ro[u], ro[u + 1])}
    return all((v ^ 1, u ^ 1) in e for u, v in e)


def compacted_csr(ref):
    ek = ref["edge_keys"]
    assert (ek[1:] > ek[:-1]).all()  # strictly ascending
    ro = np.searchsorted(ek >> np.uint64(32), np.arange(2 * ref["n_unitigs"] + 1, dtype=np.uint64), side="left").astype(np.uint64)
    return ro, (ek & M32).astype(np.uint32)


def check_compacting_again_links_nothing(ref):
    ro, d = compacted_csr(ref)
    assert is_twin_symmetric(ro, d, ref["n_unitigs"])
    again = unitig_reference(ro, d, ref["n_unitigs"])
    assert again["n_links"] == 0 and again["n_unitigs"] == ref["n_unitigs"]


def _k(u, v):
    return (u << 32) | v


# name -> (n_nodes, edges (twins added), expected: members per unitig, circular, node_unitig, node_pos, n_links, unitig edge keys, src_edge)
HAND = {
    "lone node": (1, [], [[0]], [0], [0], [0], 0, [], []),
    # 4+ 3+ 2+ 1+ 0- : head 8 > twin of the tail 1: the reverse strand is the kept one
    "5-chain kept reversed": (5, [(8, 6), (6, 4), (4, 2), (2, 1)], [[0, 3, 5, 7, 9]], [0], [0] * 5, [0, 1, 2, 3, 4], 8, [], []),
    # 0+ 1+ then a branch to 2+ and 3+.  CSR: (0,2) (2,4) (2,6) (3,1) (5,3) (7,3)
    "Y": (4, [(0, 2), (2, 4), (2, 6)], [[0, 2], [4], [6]], [0, 0, 0], [0, 0, 1, 2], [0, 1, 0, 0], 2,
          [_k(0, 2), _k(0, 4), _k(3, 1), _k(5, 1)], [1, 2, 4, 5]),
    # 0+ -> 1+ -> 4+ -> 3+ and 0+ -> 2+ -> 3+.  CSR: (0,2) (0,4) (2,8) (3,1) (4,6) (5,1) (7,5) (7,9) (8,6) (9,3); row 7 needs its keys reordered
    "bubble": (5, [(0, 2), (2, 8), (8, 6), (0, 4), (4, 6)], [[0], [2, 8], [4], [6]], [0, 0, 0, 0], [0, 1, 2, 3, 1], [0, 0, 0, 0, 1], 2,
               [_k(0, 2), _k(0, 4), _k(2, 6), _k(3, 1), _k(4, 6), _k(5, 1), _k(7, 3), _k(7, 5)], [0, 1, 8, 3, 4, 5, 7, 6]),
    # 0- 1+ 2- 3+ round; the twin cycle 7 4 3 0 holds the smallest id and starts there
    "4-cycle": (4, [(1, 2), (2, 5), (5, 6), (6, 1)], [[0, 7, 4, 3]], [1], [0, 0, 0, 0], [0, 3, 2, 1], 8, [], []),
    "loop": (1, [(0, 0)], [[0]], [0], [0], [0], 0, [_k(0, 0), _k(1, 1)], [0, 1]),
    # 0+ 1+ 1- 0-: without the hairpin rule one chain that is its own twin.  CSR: (0,2) (2,3) (3,1)
    "hairpin splits": (2, [(0, 2), (2, 3), (3, 1)], [[0, 2]], [0], [0, 0], [0, 1], 2, [_k(0, 1)], [1]),
    "mixed orientations": (3, [(0, 3), (3, 4)], [[0, 3, 4]], [0], [0, 0, 0], [0, 1, 2], 4, [], []),
}


def hand_case(name):
    n, edges, mem, circ, nu, npos, nl, ek, se = HAND[name]
    ro, d = csr_of(n, edges)
    off = np.concatenate([[0], np.cumsum([len(m) for m in mem])]).astype(np.uint64)
    want = {"uni_off": off, "members": np.array(sum(mem, []), dtype=np.uint32), "node_unitig": np.array(nu, dtype=np.uint32),
            "node_pos": np.array(npos, dtype=np.uint32), "circular": np.array(circ, dtype=np.uint8), "n_unitigs": len(mem), "n_links": nl,
            "edge_keys": np.array(ek, dtype=np.uint64), "src_edge": np.array(se, dtype=np.uint64)}
    return n, ro, d, want


def same(got, want, tag):
    for f in want:
        if isinstance(want[f], np.ndarray):
            assert np.asarray(got[f]).astype(want[f].dtype).tobytes() == want[f].tobytes(), (tag, f, got[f], want[f])
        else:
            assert got[f] == want[f], (tag, f, got[f], want[f])


def random_symmetric_graph(rng, n, extra, p_cycle=0.3, max_seg=None):
    """random oriented paths and cycles over n nodes, `extra` random edges on top, closed under twins"""
    perm = rng.permutation(n)
    o = rng.integers(0, 2, size=n)
    a = (2 * perm + o).tolist()
    edges, i = [], 0
    while i < n:
        L = int(rng.integers(1, (max_seg or max(2, n // 3)) + 1))
        seg = a[i: i + L]
        edges += list(zip(seg[:-1], seg[1:]))
        if len(seg) > 1 and rng.random() < p_cycle:
            edges.append((seg[-1], seg[0]))
        i += L
    if extra and n:
        x = rng.integers(0, 2 * n, size=(extra, 2))
        x[: extra // 4, 1] = x[: extra // 4, 0] ^ rng.integers(0, 2, size=extra // 4)  # loops and hairpins among them
        edges += [tuple(r) for r in x.tolist()]
    return csr_of(n, edges)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert hasattr(pkg.Engine, "graph_unitigs") and hasattr(pkg.Engine, "graph_unitig_edges") and hasattr(pkg.KminmerGraph, "unitigs")
    assert hasattr(pkg.UnitigGraph, "write_gfa") and hasattr(pkg, "write_unitig_gfa") and hasattr(pkg, "UnitigOut")


def test_cpp_unitig_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "unitig_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "unitig_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_unitig_out_layout_matches_ctypes(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "unitig_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "unitig_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    T = pkg.UnitigOut
    assert facts["sizeof.s2k_unitig_out"] == (ctypes.sizeof(T),)
    assert [f for f, _ in T._fields_] == ["capacity", "uni_off", "members", "node_unitig", "node_pos", "circular"]
    for f, ct in T._fields_:
        assert facts["s2k_unitig_out." + f] == (getattr(T, f).offset, ctypes.sizeof(ct)), f


@pytest.mark.parametrize("name", list(HAND))
def test_reference_hand_made(name):
    n, ro, d, want = hand_case(name)
    assert is_twin_symmetric(ro, d, n)
    ref = unitig_reference(ro, d, n)
    same(ref, want, name)
    check_compacting_again_links_nothing(ref)


def test_reference_random_graphs_invariants():
    rng = np.random.default_rng(11)
    for n, extra in ((1, 0), (2, 1), (7, 3), (40, 10), (200, 0), (200, 40), (500, 300)):
        for _ in range(6):
            ro, d = random_symmetric_graph(rng, n, extra)
            ref = unitig_reference(ro, d, n)
            check_invariants(ro, d, n, ref)
            check_compacting_again_links_nothing(ref)


def check_invariants(ro, d, n, ref):
    """every node once; consecutive members are linked; maximal: no unitig edge U -> V with out(tail U) == 1 and out(head V ^ 1) == 1
    unless V is U or U ^ 1"""
    ro, d = [int(x) for x in ro], [int(x) for x in d]
    nxt = links_of(ro, d, 2 * n)
    mem, off = ref["members"].tolist(), ref["uni_off"].tolist()
    assert sorted(x >> 1 for x in mem) == list(range(n))
    for t in range(ref["n_unitigs"]):
        m = mem[off[t]: off[t + 1]]
        assert all(nxt[a] == b for a, b in zip(m[:-1], m[1:]))
        assert (nxt[m[-1]] == m[0]) == bool(ref["circular"][t])
        for i, x in enumerate(m):
            assert ref["node_unitig"][x >> 1] == t and ref["node_pos"][x >> 1] == i
    for key, e in zip(ref["edge_keys"].tolist(), ref["src_edge"].tolist()):
        U, V = key >> 32, key & 0xFFFFFFFF
        tail = mem[off[(U >> 1) + 1] - 1] if U % 2 == 0 else mem[off[U >> 1]] ^ 1
        head = mem[off[V >> 1]] if V % 2 == 0 else mem[off[(V >> 1) + 1] - 1] ^ 1
        assert ro[tail] <= e < ro[tail + 1] and d[e] == head
        if ro[tail + 1] - ro[tail] == 1 and ro[(head ^ 1) + 1] - ro[head ^ 1] == 1:
            assert V in (U, U ^ 1)


def test_write_unitig_gfa_hand_made(tmp_path):
    n, ro, d, want = hand_case("bubble")
    counts = np.array([3, 4, 5, 6, 7], dtype=np.uint32)  # per node
    ucounts = [3, 4 + 7, 5, 6]
    ec = np.arange(10, 20, dtype=np.uint32)[want["src_edge"].astype(np.int64)]
    assert np.add.reduceat(counts[want["members"] >> 1], want["uni_off"][:-1].astype(np.int64)).tolist() == ucounts
    path = str(tmp_path / "u.gfa")
    pkg.write_unitig_gfa(path, want["uni_off"], want["members"], ucounts, want["edge_keys"], ec, members=True)
    lines = open(path).read().split("\n")
    assert lines == ["H\tVN:Z:1.0",
                     "S\t0\t*\tLN:i:1\tKC:i:3\tnd:Z:0+", "S\t1\t*\tLN:i:2\tKC:i:11\tnd:Z:1+,4+", "S\t2\t*\tLN:i:1\tKC:i:5\tnd:Z:2+",
                     "S\t3\t*\tLN:i:1\tKC:i:6\tnd:Z:3+",
                     # one L line per twin pair, the key not above its twin's: (0,2) (0,4) (2,6) (4,6); RC = the CSR edge's count
                     "L\t0\t+\t1\t+\t*\tRC:i:10", "L\t0\t+\t2\t+\t*\tRC:i:11", "L\t1\t+\t3\t+\t*\tRC:i:18", "L\t2\t+\t3\t+\t*\tRC:i:14", ""]
    pkg.write_unitig_gfa(path, want["uni_off"], want["members"], ucounts, want["edge_keys"], ec)
    assert open(path).read().split("\n")[1:3] == ["S\t0\t*\tLN:i:1\tKC:i:3", "S\t1\t*\tLN:i:2\tKC:i:11"]
    # a hairpin between unitigs is its own twin: one L line
    n, ro, d, want = hand_case("hairpin splits")
    pkg.write_unitig_gfa(path, want["uni_off"], want["members"], [9], want["edge_keys"], [5])
    assert open(path).read().split("\n") == ["H\tVN:Z:1.0", "S\t0\t*\tLN:i:2\tKC:i:9", "L\t0\t+\t0\t-\t*\tRC:i:5", ""]


def _graph_module():
    import test_graph

    return test_graph


def test_oracle_ecoli_unitigs_invariants(oracle, ecoli):
    """the committed E. coli fixture, reads sampled as test_graph._sample_reads does, graph by the numpy references, then unitigs.
    Seed 5, 150 reads of 2-4 kbp (4.5x of the 100 kbp fixture: low enough that min_count 2 leaves gaps), Hpc l=21 k=3 d=0.05."""
    tg = _graph_module()
    reads = tg._sample_reads(ecoli, 150, 5)
    b = oracle.batch(*pkg.pack_reads(reads), 21, 3, 0.05, int(pkg.HashMode.Hpc))
    g = tg.graph_reference([b], 2)
    n = len(g["keys"])
    ref = unitig_reference(g["row_off"], g["dst"], n)
    check_invariants(g["row_off"], g["dst"], n, ref)
    check_compacting_again_links_nothing(ref)
    lens = np.diff(ref["uni_off"].astype(np.int64))
    deg = np.diff(g["row_off"].astype(np.int64))
    odd_start = int((ref["members"][ref["uni_off"][:-1].astype(np.int64)] & 1).sum())
    print("nodes %d edges %d unitigs %d longest %d of >= 3 members %d; out-degree >= 2: %d; kept strands starting on an odd id: %d"
          % (n, len(g["dst"]), ref["n_unitigs"], lens.max(), (lens >= 3).sum(), (deg >= 2).sum(), odd_start))
    # observed: nodes 6513 edges 13002 unitigs 16 longest 1071, 14 of >= 3 members; 2 oriented nodes of out-degree >= 2; 7 odd starts
    assert (lens >= 3).sum() >= 1 and (deg >= 2).sum() >= 1 and odd_start >= 1


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = {"uni_off": -3, "members": -3, "node_unitig": -3, "node_pos": -3, "circular": 0xA5}


def _dev_csr(ro, d):
    import torch

    dro = torch.from_numpy(np.asarray(ro, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")
    dd = torch.from_numpy(np.asarray(d, dtype=np.uint32).view(np.int32).copy()).to("cuda:0") if len(d) else torch.zeros(1, dtype=torch.int32, device="cuda:0")
    return dro, dd


def _raw_unitigs(eng, ro, d, n, n_edges=None, capacity=None, null=(), sizes_only=False, guard=8, ctx=True, dev=None):
    """s2k_graph_unitigs through ctypes, guard words behind every output array -> (status, n_unitigs, n_links, host arrays with guards)"""
    import torch

    dro, dd = dev if dev is not None else _dev_csr(ro, d)
    cap = n if capacity is None else capacity
    tdt = {"uni_off": torch.int64, "members": torch.int32, "node_unitig": torch.int32, "node_pos": torch.int32, "circular": torch.uint8}
    size = {"uni_off": cap + 1, "members": n, "node_unitig": n, "node_pos": n, "circular": cap}
    bufs = {f: torch.full((size[f] + guard,), GUARD[f], dtype=tdt[f], device="cuda:0") for f in FIELDS}
    o = pkg.UnitigOut()
    o.capacity = cap
    for f in FIELDS:
        setattr(o, f, None if (f in null or sizes_only) else bufs[f].data_ptr())
    nu, nl = ctypes.c_uint64(777), ctypes.c_uint64(777)
    torch.cuda.synchronize()
    ne = len(d) if n_edges is None else n_edges
    s = eng.lib.s2k_graph_unitigs(eng.ctx if ctx else None, None if "row_off" in null else ctypes.c_void_p(dro.data_ptr()),
                                  None if ("dst" in null or len(d) == 0) else ctypes.c_void_p(dd.data_ptr()), ne, n,
                                  None if "out" in null else ctypes.byref(o), ctypes.byref(nu), ctypes.byref(nl))
    return s, nu.value, nl.value, {f: bufs[f].cpu().numpy() for f in FIELDS}, bufs, (dro, dd)


def _untouched(host):
    return all((host[f] == np.array(GUARD[f]).astype(host[f].dtype)).all() for f in FIELDS)


def _raw_uedges(eng, dro, dd, n_edges, n, bufs, nu, capacity, keys_out=True, guard=8):
    import torch

    k = torch.full((capacity + guard,), -0x5A5A, dtype=torch.int64, device="cuda:0")
    se = torch.full((capacity + guard,), -0x5A5A, dtype=torch.int64, device="cuda:0")
    no = ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_graph_unitig_edges(eng.ctx, ctypes.c_void_p(dro.data_ptr()), ctypes.c_void_p(dd.data_ptr()) if n_edges else None, n_edges, n,
                                       *(ctypes.c_void_p(bufs[f].data_ptr()) for f in ("uni_off", "members", "node_unitig", "node_pos")), nu,
                                       ctypes.c_void_p(k.data_ptr()) if keys_out else None, ctypes.c_void_p(se.data_ptr()) if keys_out else None,
                                       capacity, ctypes.byref(no))
    return s, no.value, k.cpu().numpy(), se.cpu().numpy()


def device_unitigs(eng, ro, d, n, want, tag):
    """both calls, every output against `want` (a unitig_reference result), guards untouched -> the device CSR (for reuse)"""
    s, nu, nl, host, bufs, dev = _raw_unitigs(eng, ro, d, n)
    assert (s, nu, nl) == (0, want["n_unitigs"], want["n_links"]), (tag, s, nu, nl, want["n_unitigs"], want["n_links"])
    size = {"uni_off": nu + 1, "members": n, "node_unitig": n, "node_pos": n, "circular": nu}
    for f in FIELDS:
        got = host[f]
        assert got[:size[f]].view(DT[f]).tobytes() == want[f].tobytes(), (tag, f)
        assert (got[size[f]:] == np.array(GUARD[f]).astype(got.dtype)).all(), (tag, f, "guard")
    ne = len(d)
    cap = ne - nl
    s, no, k, se = _raw_uedges(eng, dev[0], dev[1], ne, n, bufs, nu, cap)
    assert (s, no) == (0, cap) and cap == len(want["edge_keys"]), (tag, s, no, cap)
    assert k[:no].view(np.uint64).tobytes() == want["edge_keys"].tobytes(), (tag, "edge_keys")
    assert se[:no].view(np.uint64).tobytes() == want["src_edge"].tobytes(), (tag, "src_edge")
    assert (k[no:] == -0x5A5A).all() and (se[no:] == -0x5A5A).all()
    return host, bufs, dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_device_hand_made(eng, name):
    n, ro, d, want = hand_case(name)
    device_unitigs(eng, ro, d, n, want, name)


@pytest.mark.gpu
def test_device_random_symmetric_graphs(eng):
    """>= 200 graphs, all arrays compared: fewer oriented nodes than a wave, exactly a block (128 nodes = 256 lanes), around it, many
    blocks; no edge at all (all nodes isolated); one chain through all nodes; one cycle through all nodes"""
    rng = np.random.default_rng(12)
    done = 0
    for n in (1, 2, 3, 5, 16, 31, 32, 33, 64, 127, 128, 129, 255, 256, 257, 1000, 4097, 20000):
        reps = 14 if n <= 300 else 4 if n <= 5000 else 2
        for r in range(reps):
            extra = (0, n // 10, n // 3, n, 1)[r % 5]
            ro, d = random_symmetric_graph(rng, n, extra, p_cycle=(0.0, 0.3, 0.9)[r % 3], max_seg=(None, 4, n)[(r // 2) % 3])
            device_unitigs(eng, ro, d, n, unitig_reference(ro, d, n), ("random", n, r))
            done += 1
        for shape in ("isolated", "chain", "cycle"):
            a = (2 * rng.permutation(n) + rng.integers(0, 2, size=n)).tolist()
            e = [] if shape == "isolated" else list(zip(a[:-1], a[1:])) + ([(a[-1], a[0])] if shape == "cycle" and n > 1 else [])
            ro, d = csr_of(n, e)
            want = unitig_reference(ro, d, n)
            if shape == "isolated":
                assert len(d) == 0 and want["n_unitigs"] == n
            elif n > 2:
                assert want["n_unitigs"] == 1 and want["circular"][0] == (shape == "cycle")
            device_unitigs(eng, ro, d, n, want, (shape, n))
            done += 1
    assert done >= 200
    # n_nodes == 0
    s, nu, nl, host, _, _ = _raw_unitigs(eng, np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), 0)
    assert (s, nu, nl) == (0, 0, 0) and host["uni_off"][0] == 0 and (host["uni_off"][1:] == -3).all()


def _long_path(n, seed, cycle):
    """one chain (or one cycle) through n nodes, node ids permuted along it, random orientations -> CSR and the expected arrays in
    closed form"""
    rng = np.random.default_rng(seed)
    a = (2 * rng.permutation(n) + rng.integers(0, 2, size=n)).astype(np.int64)  # the forward strand
    src = np.concatenate([a[:-1], a[1:] ^ 1] + ([[a[-1]], [a[0] ^ 1]] if cycle else []))
    dst = np.concatenate([a[1:], a[:-1] ^ 1] + ([[a[0]], [a[-1] ^ 1]] if cycle else []))
    order = np.argsort(src * (4 * n) + dst)
    src, dst = src[order], dst[order]
    ro = np.searchsorted(src, np.arange(2 * n + 1)).astype(np.uint64)
    tw = (a ^ 1)[::-1]
    if cycle:  # the smallest id of the two cycles is 0 (node 0, forward): the kept strand is the one that holds it, and starts there
        strand = a if a[np.argmin(a >> 1)] == 0 else tw
        j = int(np.nonzero(strand == 0)[0][0])
        strand = np.concatenate([strand[j:], strand[:j]])
    else:
        strand = a if a[0] < tw[0] else tw
    pos = np.empty(n, dtype=np.uint32)
    pos[strand >> 1] = np.arange(n, dtype=np.uint32)
    want = {"uni_off": np.array([0, n], dtype=np.uint64), "members": strand.astype(np.uint32), "node_unitig": np.zeros(n, dtype=np.uint32),
            "node_pos": pos, "circular": np.array([1 if cycle else 0], dtype=np.uint8), "n_unitigs": 1, "n_links": len(dst),
            "edge_keys": np.zeros(0, dtype=np.uint64), "src_edge": np.zeros(0, dtype=np.uint64)}
    return ro, dst.astype(np.uint32), want


@pytest.mark.gpu
@pytest.mark.parametrize("cycle", [False, True])
def test_device_long_chain_and_cycle_rounds(eng, cycle):
    """2^21 + 3 nodes in one chain / one cycle and its twin, ids permuted along it: every jump a random load, more than 21 rounds"""
    n = 2 ** 21 + 3
    ro, d, want = _long_path(n, 21 + cycle, cycle)
    small = _long_path(9, 3, cycle)
    same(unitig_reference(small[0], small[1], 9), small[2], "closed form")  # the closed form against the walk, small
    device_unitigs(eng, ro, d, n, want, ("long", cycle))
    rounds = ctypes.c_uint32(0)
    eng.lib.s2k_graph_unitigs_last_steps(None, ctypes.byref(rounds))
    assert rounds.value > 21


@pytest.mark.gpu
def test_device_refusals_capacity_and_sizes(eng):
    rng = np.random.default_rng(13)
    n = 600
    ro, d = random_symmetric_graph(rng, n, 150, max_seg=9)
    want = unitig_reference(ro, d, n)
    assert want["n_unitigs"] > 20 and want["n_links"] > 20 and len(want["edge_keys"]) > 20

    def refused(ro_, d_, n_=n, code=1, **kw):
        s, nu, nl, host, _, _ = _raw_unitigs(eng, ro_, d_, n_, **kw)
        assert s == code and _untouched(host), (s, kw)
        return nu, nl

    ros, ds = [int(x) for x in ro], d.tolist()
    u = next(x for x in range(2 * n) if ros[x + 1] - ros[x] >= 2)  # a row of two or more
    e = ros[u]
    # a missing twin: the last destination of a row replaced by a larger id whose twin's row does not lead back
    edges = {(a, ds[i]) for a in range(2 * n) for i in range(ros[a], ros[a + 1])}
    x = d.copy()
    x[ros[u + 1] - 1] = next(v for v in range(ds[ros[u + 1] - 1] + 1, 2 * n) if (v ^ 1, u ^ 1) not in edges)
    assert refused(ro, x) == (0, 0)
    refused(np.array([0, 1, 1, 1, 1, 1, 1], dtype=np.uint64), np.array([2], dtype=np.uint32), n_=3)  # 0 -> 2 without 3 -> 1
    x = d.copy()  # an unsorted row
    x[[e, e + 1]] = x[[e + 1, e]]
    refused(ro, x)
    x = d.copy()  # a repeated destination
    x[e + 1] = x[e]
    refused(ro, x)
    x = d.copy()  # an id >= 2 n (the last entry of a row: still ascending)
    x[ros[u + 1] - 1] = 2 * n
    refused(ro, x)
    refused(ro, d, n_edges=len(d) + 1)  # row_off[2 n] != n_edges
    refused(ro, d, n_edges=len(d) - 1)
    y = ro.copy()  # row_off not starting at 0, decreasing
    y[0] = 1
    refused(y, d)
    y = ro.copy()
    y[u + 1] = y[u] - np.uint64(1) if y[u] > 0 else y[u + 2] + np.uint64(1)
    refused(y, d)
    assert eng.lib.s2k_graph_unitigs(eng.ctx, ctypes.c_void_p(8), None, 0, 2 ** 31, None, ctypes.byref(ctypes.c_uint64()),
                                     ctypes.byref(ctypes.c_uint64())) == 1  # n >= 2^31, before anything is read
    refused(ro, d, ctx=False)
    refused(ro, d, null=("row_off",))
    refused(ro, d, null=("dst",))
    # one short: S2K_ERR_CAPACITY, the counts still set
    assert refused(ro, d, code=7, capacity=want["n_unitigs"] - 1) == (want["n_unitigs"], want["n_links"])
    # sizes only: out NULL, or every array NULL
    assert refused(ro, d, code=0, null=("out",)) == (want["n_unitigs"], want["n_links"])
    assert refused(ro, d, code=0, sizes_only=True) == (want["n_unitigs"], want["n_links"])
    # exactly enough, and only some of the arrays
    s, nu, nl, host, bufs, dev = _raw_unitigs(eng, ro, d, n, capacity=want["n_unitigs"], null=("node_pos", "circular"))
    assert s == 0 and host["members"][:n].view(np.uint32).tobytes() == want["members"].tobytes()
    assert host["uni_off"][:nu + 1].view(np.uint64).tobytes() == want["uni_off"].tobytes() and (host["uni_off"][nu + 1:] == -3).all()
    assert (host["node_pos"] == -3).all() and (host["circular"] == 0xA5).all()
    # the edges call
    host, bufs, dev = device_unitigs(eng, ro, d, n, want, "full")
    ne, cap = len(d), len(want["edge_keys"])
    s, no, k, se = _raw_uedges(eng, dev[0], dev[1], ne, n, bufs, want["n_unitigs"], cap - 1)
    assert (s, no) == (7, cap) and (k == -0x5A5A).all() and (se == -0x5A5A).all()
    s, no, k, se = _raw_uedges(eng, dev[0], dev[1], ne, n, bufs, want["n_unitigs"], cap, keys_out=False)
    assert (s, no) == (0, cap) and (k == -0x5A5A).all()
    no = ctypes.c_uint64(5)
    assert eng.lib.s2k_graph_unitig_edges(None, None, None, 0, 1, None, None, None, None, 0, None, None, 0, ctypes.byref(no)) == 1 and no.value == 0
    assert eng.lib.s2k_graph_unitig_edges(eng.ctx, None, None, 0, 1, None, None, None, None, 0, None, None, 0, ctypes.byref(no)) == 1


@pytest.mark.gpu
def test_device_deterministic(eng):
    rng = np.random.default_rng(14)
    n = 50000
    ro, d = random_symmetric_graph(rng, n, n // 5, max_seg=40)
    runs = []
    for _ in range(2):
        s, nu, nl, host, bufs, dev = _raw_unitigs(eng, ro, d, n)
        s2, no, k, se = _raw_uedges(eng, dev[0], dev[1], len(d), n, bufs, nu, len(d) - nl)
        assert s == 0 and s2 == 0
        runs.append(b"".join(host[f].tobytes() for f in FIELDS) + k.tobytes() + se.tobytes() + bytes([nu % 251, nl % 251]))
    assert runs[0] == runs[1]


def _unitig_graph_host(ug):
    return {"uni_off": ug.uni_off.cpu().numpy().view(np.uint64), "members": ug.members.cpu().numpy().view(np.uint32),
            "node_unitig": ug.node_unitig.cpu().numpy().view(np.uint32), "node_pos": ug.node_pos.cpu().numpy().view(np.uint32),
            "circular": ug.circular.cpu().numpy(), "counts": ug.counts.cpu().numpy(), "edge_keys": ug.edge_keys.cpu().numpy().view(np.uint64),
            "edge_counts": ug.edge_counts.cpu().numpy().view(np.uint32), "row_off": ug.row_off.cpu().numpy().view(np.uint64),
            "dst": ug.dst.cpu().numpy().view(np.uint32)}


def _unitig_graph_reference(g):
    """the UnitigGraph of a test_graph.graph_reference result"""
    n = len(g["keys"])
    ref = unitig_reference(g["row_off"], g["dst"], n)
    csum = np.concatenate([[0], np.cumsum(g["counts"][ref["members"] >> 1].astype(np.int64))])
    off = ref["uni_off"].astype(np.int64)
    ro, d = compacted_csr(ref)
    want = {f: ref[f] for f in FIELDS}
    want.update(counts=csum[off[1:]] - csum[off[:-1]], edge_keys=ref["edge_keys"], edge_counts=g["edge_counts"][ref["src_edge"].astype(np.int64)],
                row_off=ro, dst=d)
    return want, ref


@pytest.mark.gpu
def test_kminmer_graph_unitigs_match_oracle_references(eng, oracle, ecoli, tmp_path):
    """E. coli-sampled reads, Hpc and Regular, three batches equal one: KminmerGraph.build(...).unitigs(engine) == graph reference ->
    unitig reference; the unitig CSR (graph_adjacency accepted the keys) passes s2k_graph_unitigs' own symmetry check and links nothing"""
    tg = _graph_module()
    rng = np.random.default_rng(9)
    reads = [bytes(ecoli[a: a + 3000]) for a in rng.integers(0, len(ecoli) - 3000, size=400)]
    seen = []
    # 400 reads (12x: a handful of long unitigs) and the first 120 of them (3.6x: min_count 2 leaves gaps), each in three batches
    for mode, batches in ((m, b) for m in (pkg.HashMode.Hpc, pkg.HashMode.Regular)
                          for b in ([reads[:150], reads[150:270], reads[270:]], [reads[:50], reads[50:51], reads[51:120]])):
        refs = [oracle.batch(*pkg.pack_reads(b), 21, 3, 0.05, int(mode)) for b in batches]
        want, ref = _unitig_graph_reference(tg.graph_reference(refs, 2))
        assert ref["n_unitigs"] >= 2 and ref["n_links"] > 100
        seen.append((ref["n_unitigs"], len(ref["edge_keys"])))
        whole = [r for b in batches for r in b]
        for outs in ([tg._extract_dev(eng, b, 21, 3, 0.05, mode) for b in batches], [tg._extract_dev(eng, whole, 21, 3, 0.05, mode)]):
            ug = pkg.KminmerGraph.build(eng, outs, min_count=2).unitigs(eng)
            same(_unitig_graph_host(ug), want, (mode, len(outs)))
            assert ug.n_links == ref["n_links"] and ug.n_unitigs == ref["n_unitigs"]
            again = eng.graph_unitigs(ug.row_off, ug.dst, ug.n_unitigs)
            assert again["n_links"] == 0 and again["n_unitigs"] == ug.n_unitigs
        p = str(tmp_path / "u.gfa")
        ug.write_gfa(p, members=True)
        lines = open(p).read().split("\n")
        assert sum(1 for x in lines if x.startswith("S\t")) == ug.n_unitigs
        tw = ((want["edge_keys"] & M32) ^ np.uint64(1)) << np.uint64(32) | ((want["edge_keys"] >> np.uint64(32)) ^ np.uint64(1))
        assert sum(1 for x in lines if x.startswith("L\t")) == int((want["edge_keys"] <= tw).sum())
    assert max(a for a, _ in seen) > 10 and max(b for _, b in seen) > 10  # (reference: 4 / 13 / 17 / 26 unitigs, 8 / 32 / 0 / 32 edges)


@pytest.mark.gpu
def test_regular_unitigs_strand_symmetric_on_device(eng, ecoli):
    """Regular: reads and their reverse complements give identical unitig arrays (their graphs are identical, test_graph.py)"""
    tg = _graph_module()
    reads = tg._sample_reads(ecoli, 300, 7)
    rc = [tg._revcomp(r) for r in reads]
    a, b = (_unitig_graph_host(pkg.KminmerGraph.build(eng, [tg._extract_dev(eng, x, 21, 3, 0.05, pkg.HashMode.Regular)], min_count=2).unitigs(eng))
            for x in (reads, rc))
    assert len(a["circular"]) > 5 and len(a["members"]) > 1000
    same(a, b, "revcomp")


@pytest.mark.gpu
def test_full_size_genome_sampled_unitigs(eng):
    """the genome-sampled set of tools/graph_rate.py (random 50 Mbp genome, 10 kbp reads at 30x, half reverse-complemented, Regular l=31
    k=10 d=0.01): invariants with torch ops on the device, and every array against the host walk"""
    import sys

    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from graph_rate import genome_reads

    dev = torch.device("cuda", 0)
    bases, read_off, n_reads = genome_reads(torch, dev, 50_000_000, 10_000, 30, 7)
    n_bases = n_reads * 10_000
    cap = int(n_bases * 0.03)
    out = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
           "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = cap
    o.km_off, o.hash, o.rev = (out[x].data_ptr() for x in ("km_off", "hash", "rev"))
    torch.cuda.synchronize(dev)
    eng.extract_device(bases.data_ptr(), read_off.data_ptr(), n_reads, n_bases, 31, 10, 0.01, int(pkg.HashMode.Regular), o)
    del bases
    g = pkg.KminmerGraph.build(eng, [out], min_count=2)
    del out
    ug = g.unitigs(eng)
    n, ne = g.n_nodes, g.n_edges
    assert n > 500_000 and ug.n_unitigs > 0
    ro, dst = g.row_off, g.dst.long() & 0xFFFFFFFF
    mem, off, pos, nu = ug.members.long() & 0xFFFFFFFF, ug.uni_off, ug.node_pos.long(), ug.node_unitig.long()
    assert int(off[-1]) == n and int((off[1:] - off[:-1]).sum()) == n and ug.n_edges == ne - ug.n_links
    assert torch.equal(torch.sort(mem >> 1).values, torch.arange(n, device=dev))  # every node once
    assert torch.equal(mem[off[nu] + pos] >> 1, torch.arange(n, device=dev))
    inner = torch.ones(n, dtype=torch.bool, device=dev)
    inner[off[:-1]] = False  # member j and j - 1 belong to one unitig
    b = mem[inner]
    a = mem[torch.nonzero(inner)[:, 0] - 1]
    deg = ro[1:] - ro[:-1]
    assert bool((deg[a] == 1).all()) and bool((deg[b ^ 1] == 1).all()) and torch.equal(dst[ro[a]], b)
    want, ref = _unitig_graph_reference({"keys": np.zeros(n), "counts": g.counts.cpu().numpy().view(np.uint32),
                                         "edge_counts": g.edge_counts.cpu().numpy().view(np.uint32),
                                         "row_off": g.row_off.cpu().numpy().view(np.uint64), "dst": g.dst.cpu().numpy().view(np.uint32)})
    same(_unitig_graph_host(ug), want, "genome")
    assert ug.n_links == ref["n_links"]
