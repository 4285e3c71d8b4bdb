"""Reads threaded through the unitig graph on the device: s2k_unitig_node_places (where every node lies on the oriented unitigs) and
s2k_table_thread (each read's items compressed into the steps of its path), include/s2k.h, DESIGN.md §3.13.  The references are
`places_reference` and `thread_reference`, serial restatements of the header's definitions (plain loops over reads and items, node
indices from np.searchsorted on the keys); the device's arrays equal theirs exactly, every one of them, in every test."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import gpu_util
import test_graph as tg
import test_simplify as ts
import test_unitigs as tu

pkg = import_package()

SYMS = ("s2k_unitig_node_places", "s2k_table_thread")
STEP = ("unitig", "pos", "count", "item", "flags", "start", "end")
LINKED = 1


# ---- the references ----------------------------------------------------------------------------------------------------------------
def places_reference(uni):
    """uni: uni_off, members, node_unitig, node_pos, circular -> the NodePlace record of every node"""
    off, mem = [int(x) for x in uni["uni_off"]], [int(x) for x in uni["members"]]
    out = np.zeros(len(uni["node_unitig"]), dtype=pkg.NodePlace)
    for i, (t, p) in enumerate(zip(uni["node_unitig"].tolist(), uni["node_pos"].tolist())):
        ln = off[t + 1] - off[t]
        o = mem[off[t] + p] & 1
        out[i] = (2 * t + o, ln - 1 - p if o else p, ln, int(uni["circular"][t]))
    return out


def thread_reference(km_off, hash_, rev, keys, counts, min_count, place, start=None, end=None, n_unitigs=0):
    """-> dict: path_off uint64, unitig / pos / count / item / flags (and start / end when given) uint32, uni_items uint64[n_unitigs],
    n_solid"""
    km = [int(x) for x in km_off]
    h, keys = np.asarray(hash_, dtype=np.uint64), np.asarray(keys, dtype=np.uint64)
    idx = np.searchsorted(keys, h)
    ic = np.minimum(idx, max(len(keys) - 1, 0))
    cnt = np.ones(len(keys), dtype=np.uint32) if counts is None else np.asarray(counts, dtype=np.uint32)
    solid = ((idx < len(keys)) & (keys[ic] == h) & (cnt[ic] >= max(int(min_count), 1))).tolist() if len(keys) else [False] * len(h)
    ic, rv = ic.tolist(), [int(x) for x in rev]
    pu, pp, pl, pc = (place[f].tolist() for f in ("unitig", "pos", "len", "circular"))
    s = {f: [] for f in STEP}
    path_off = [0]
    for r in range(len(km) - 1):
        prev = None  # (U, q) of the item before, when it is solid
        for j in range(km[r], km[r + 1]):
            if not solid[j]:
                prev = None
                continue
            i = ic[j]
            U = pu[i] ^ rv[j]
            q = pl[i] - 1 - pp[i] if rv[j] else pp[i]
            if prev is not None and U == prev[0] and (q == prev[1] + 1 or (pc[i] and prev[1] == pl[i] - 1 and q == 0)):
                s["count"][-1] += 1
                s["end"][-1] = int(end[j]) if end is not None else 0
            else:
                for f, v in (("unitig", U), ("pos", q), ("count", 1), ("item", j - km[r]), ("flags", LINKED if prev is not None else 0),
                             ("start", int(start[j]) if start is not None else 0), ("end", int(end[j]) if end is not None else 0)):
                    s[f].append(v)
            prev = (U, q)
        path_off.append(len(s["unitig"]))
    out = {f: np.array(v, dtype=np.uint32) for f, v in s.items()}
    if start is None:
        del out["start"]
    if end is None:
        del out["end"]
    out["path_off"] = np.array(path_off, dtype=np.uint64)
    out["uni_items"] = np.zeros(n_unitigs, dtype=np.uint64)
    if n_unitigs:
        np.add.at(out["uni_items"], (out["unitig"] >> 1).astype(np.int64), out["count"].astype(np.uint64))
    out["n_solid"] = sum(solid)
    return out


def decomposition(members, circular):
    """hand-made or random unitigs (lists of oriented node ids; every node once) -> the five arrays of s2k_graph_unitigs"""
    n = sum(len(m) for m in members)
    uni = {"uni_off": np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.uint64),
           "members": np.array([x for m in members for x in m], dtype=np.uint32), "node_unitig": np.zeros(n, dtype=np.uint32),
           "node_pos": np.zeros(n, dtype=np.uint32), "circular": np.array(circular, dtype=np.uint8), "n_unitigs": len(members)}
    for t, m in enumerate(members):
        for p, x in enumerate(m):
            uni["node_unitig"][x >> 1], uni["node_pos"][x >> 1] = t, p
    return uni


# ---- hand-made: ten nodes (key 100 (i + 1)) in four unitigs ---------------------------------------------------------------------------
#  unitig 0: 0+ 1+ 2- 3+      unitig 1: 4+ 5+      unitig 2: 6+ 7- 8+ round      unitig 3: 9+ (with a loop in mind)
HAND_UNI = ([[0, 2, 5, 6], [8, 10], [12, 15, 16], [18]], [0, 0, 1, 0])
HAND_PLACES = [(0, 0, 4, 0), (0, 1, 4, 0), (1, 1, 4, 0), (0, 3, 4, 0), (2, 0, 2, 0), (2, 1, 2, 0), (4, 0, 3, 1), (5, 1, 3, 1), (4, 2, 3, 1), (6, 0, 1, 0)]
HAND_COUNTS = [3, 3, 3, 3, 3, 1, 3, 3, 3, 3]  # node 5 is solid at min_count 1 only
# name -> (items: (node, rev) or None for a k-min-mer that is no node, expected path at min_count 2, its first items, at min_count 1)
HAND = {
    "along a unitig": ([(0, 0), (1, 0), (2, 1), (3, 0)], ">0:0+4", [0], None),
    "its reverse complement": ([(3, 1), (2, 0), (1, 1), (0, 1)], "<0:0+4", [0], None),
    "a gap in the middle": ([(0, 0), (1, 0), None, (3, 0)], ">0:0+2*>0:3+1", [0, 3], None),
    "a skipped member is no gap": ([(0, 0), (2, 1)], ">0:0+1>0:2+1", [0, 1], None),
    "across a junction": ([(2, 1), (3, 0), (4, 0), (5, 0)], ">0:2+2>1:0+1", [0, 2], ">0:2+2>1:0+2"),
    "round a circular unitig": ([(7, 1), (8, 0), (6, 0), (7, 1)], ">2:1+4", [0], None),
    "twice round it": ([(6, 0), (7, 1), (8, 0)] * 2 + [(6, 0)], ">2:0+7", [0], None),
    "round its twin": ([(7, 0), (6, 1), (8, 1), (7, 0)], "<2:1+4", [0], None),
    "a loop on one member": ([(9, 0), (9, 0)], ">3:0+1>3:0+1", [0, 1], None),
    "a hairpin": ([(0, 0), (1, 0), (1, 1), (0, 1)], ">0:0+2<0:2+2", [0, 2], None),
    "an empty read": ([], "", [], None),
    "one item": ([(4, 1)], "<1:1+1", [0], None),
    "no node at all": ([None, None], "", [], None),
    "gaps at both ends": ([None, (5, 1), (4, 1), None], "<1:1+1", [2], "<1:0+2"),
}


def hand_batch():
    keys = np.arange(1, 11, dtype=np.uint64) * np.uint64(100)
    km_off, h, rv = [0], [], []
    for items, *_ in HAND.values():
        for it in items:
            h.append(7 if it is None else int(keys[it[0]]))
            rv.append(0 if it is None else it[1])
        km_off.append(len(h))
    return keys, np.array(HAND_COUNTS, dtype=np.uint32), np.array(km_off, dtype=np.uint64), np.array(h, dtype=np.uint64), np.array(rv, dtype=np.uint8)


def hand_lines(mc):
    out = []
    for r, (items, p2, _, p1) in enumerate(HAND.values()):
        p = p1 if mc == 1 and p1 is not None else p2
        out.append("%d\t%d\t%s" % (5 + r, p.count(":"), p))
    return out


def paths_text(tmp_path, ref, first_read=0):
    p = str(tmp_path / "paths.tsv")
    pkg.write_read_paths(p, ref["path_off"], ref["unitig"], ref["pos"], ref["count"], ref["flags"], first_read=first_read)
    return open(p).read().split("\n")


def random_unitigs(rng, n, max_len=40, p_cycle=0.3, lens=None):
    """a random decomposition of n nodes: random order and orientation, cut into unitigs, some of two members or more circular"""
    a = (2 * rng.permutation(n) + rng.integers(0, 2, size=n)).tolist()
    members, i = [], 0
    lens = list(lens or [])
    while i < n:
        L = lens.pop(0) if lens else int(rng.integers(1, max_len + 1))
        members.append(a[i: i + L])
        i += L
    return decomposition(members, [int(len(m) > 1 and rng.random() < p_cycle) for m in members])


def walk_items(rng, km_off, keys, uni, gap=0.04, jump=0.05, t_first=None):
    """reads that walk along the unitigs: each item follows the one before it on its oriented unitig (round a circular one), jumps to a
    random place with probability `jump` or at a linear unitig's end, and is replaced by a k-min-mer that is no node with probability
    `gap`"""
    off, mem, circ = [int(x) for x in uni["uni_off"]], [int(x) for x in uni["members"]], uni["circular"].tolist()
    T = len(off) - 1
    n = int(km_off[-1])
    starts = set(int(x) for x in km_off[:-1])
    h, rv = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    t = s = q = 0
    jumps, gaps, tsel, ssel, qsel = rng.random(n) < jump, rng.random(n) < gap, rng.integers(0, T, size=n), rng.integers(0, 2, size=n), rng.random(n)
    for j in range(n):
        ln = off[t + 1] - off[t] if T else 0
        if j == 0 or j in starts or jumps[j] or (q + 1 >= ln and not circ[t]):
            t = int(tsel[j]) if t_first is None or j else t_first
            s, ln = int(ssel[j]), off[t + 1] - off[t]
            q = int(qsel[j] * ln) if t_first is None or j else 0
        else:
            q = (q + 1) % ln
        m = mem[off[t] + q] if s == 0 else mem[off[t] + ln - 1 - q] ^ 1  # the oriented node at position q of 2 t + s
        h[j], rv[j] = keys[m >> 1], m & 1
    other = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    h[gaps] = other[gaps]
    return h, rv


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert "S2K_ABI_VERSION 2" in header and pkg.ABI_VERSION == 2
    assert hasattr(pkg.Engine, "unitig_node_places") and hasattr(pkg.CountTable, "thread")
    assert hasattr(pkg.UnitigGraph, "places") and hasattr(pkg.UnitigGraph, "thread")
    assert hasattr(pkg.ReadPaths, "host") and hasattr(pkg.ReadPaths, "write_paths") and hasattr(pkg, "write_read_paths")


def test_thread_out_and_place_layouts_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "thread_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "thread_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    T = pkg.ThreadOut
    assert facts["sizeof.s2k_thread_out"] == (ctypes.sizeof(T),)
    assert [f for f, _ in T._fields_] == ["capacity", "path_off"] + list(STEP)
    for f, ct in T._fields_:
        assert facts["s2k_thread_out." + f] == (getattr(T, f).offset, ctypes.sizeof(ct)), f
    P = pkg.NodePlace
    assert facts["sizeof.s2k_node_place"] == (P.itemsize,) == (16,) and P.names == ("unitig", "pos", "len", "circular")
    for f in P.names:
        assert facts["s2k_node_place." + f] == (P.fields[f][1], P.fields[f][0].itemsize), f
    assert facts["S2K_STEP_LINKED"] == (pkg.STEP_LINKED,) == (LINKED,)


def test_cpp_thread_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "thread_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "thread_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    mk = open(os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc", "Makefile")).read()
    assert "s2k_thread.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))


def test_references_hand_made(tmp_path):
    uni = decomposition(*HAND_UNI)
    place = places_reference(uni)
    assert place.tolist() == HAND_PLACES
    keys, cnt, km_off, h, rv = hand_batch()
    for mc in (2, 1):
        ref = thread_reference(km_off, h, rv, keys, cnt, mc, place, n_unitigs=4)
        lines = paths_text(tmp_path, ref, first_read=5)
        assert lines[:-1] == hand_lines(mc) and lines[-1] == "", mc
        assert int(ref["count"].sum()) == ref["n_solid"] == int(ref["uni_items"].sum())
    ref = thread_reference(km_off, h, rv, keys, cnt, 2, place, n_unitigs=4)
    assert ref["item"].tolist() == sum((it for _, _, it, _ in HAND.values()), [])
    assert ref["uni_items"].tolist() == [4 + 4 + 3 + 2 + 2 + 4, 1 + 1 + 1, 4 + 7 + 4, 2]


def test_path_writer_marks_gaps_but_not_a_reads_first_step(tmp_path):
    p = str(tmp_path / "w.tsv")
    pkg.write_read_paths(p, [0, 2, 2, 3], [4, 7, 1], [0, 3, 9], [5, 1, 2], [0, 0, 0])
    assert open(p).read() == "0\t2\t>2:0+5*<3:3+1\n1\t0\t\n2\t1\t<0:9+2\n"
    pkg.write_read_paths(p, [0, 2], [4, 7], [0, 3], [5, 1], [1, 1], first_read=40)
    assert open(p).read() == "40\t2\t>2:0+5<3:3+1\n"


def linked_transitions_follow_edges(ref, place_len, circular, edge_keys):
    """every LINKED step that follows a step of its read wraps a circular unitig, or leaves position len - 1 of U and enters position 0
    of V over a unitig edge U -> V -> the number of such transitions"""
    ek = set(int(x) for x in edge_keys)
    off = [int(x) for x in ref["path_off"]]
    u, p, c, f = (ref[x].tolist() for x in ("unitig", "pos", "count", "flags"))
    n = 0
    for r in range(len(off) - 1):
        for s in range(off[r] + 1, off[r + 1]):
            if not f[s] & LINKED:
                continue
            U, V, ln = u[s - 1], u[s], place_len[u[s - 1] >> 1]
            last = (p[s - 1] + c[s - 1] - 1) % ln if circular[U >> 1] else p[s - 1] + c[s - 1] - 1
            assert last == ln - 1 and p[s] == 0 and ((U == V and circular[U >> 1]) or (U << 32 | V) in ek), (r, s, U, V, last, ln, p[s])
            n += 1
        assert not (off[r + 1] > off[r] and f[off[r]] & LINKED), r  # a read's first step is never linked
    return n


def test_oracle_ecoli_reads_reference_invariants(oracle, ecoli):
    """error-free E. coli reads, Regular l=12 k=5 d=0.05, graph and unitigs by the references: the steps hold every solid item once,
    path_off is monotone, every linked transition is a unitig edge"""
    reads = tg._sample_reads(ecoli, 300, 11)
    b = oracle.batch(*pkg.pack_reads(reads), 12, 5, 0.05, int(pkg.HashMode.Regular))
    for mc in (1, 2):
        g = tg.graph_reference([b], mc, 1)
        uni = tu.unitig_reference(g["row_off"], g["dst"], len(g["keys"]))
        place = places_reference(uni)
        ref = thread_reference(b["km_off"], b["hash"], b["rev"], g["keys"], g["counts"], mc, place, b["start"], b["end"], uni["n_unitigs"])
        assert int(ref["count"].sum()) == ref["n_solid"] > 10000
        po = ref["path_off"].astype(np.int64)
        assert po[0] == 0 and (np.diff(po) >= 0).all() and po[-1] == len(ref["unitig"])
        lens = np.diff(uni["uni_off"].astype(np.int64)).tolist()
        n = linked_transitions_follow_edges(ref, lens, uni["circular"].tolist(), uni["edge_keys"])
        print("min_count %d: %d nodes, %d unitigs, %d steps over %d solid items, %d linked transitions" % (mc, len(g["keys"]), uni["n_unitigs"],
                                                                                                          len(ref["unitig"]), ref["n_solid"], n))


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = 8
MARK = -0x5A5A
_dev, _host, _ptr = ts._dev, ts._host, ts._ptr


def _marked(h, frm=0):
    return (h[frm:].view(np.int32) == MARK).all() if h.dtype.itemsize == 4 else (h[frm:].view(np.int64) == MARK).all()


def raw_places(eng, uni, n_nodes=None, n_unitigs=None, null=(), ctx=True):
    """s2k_unitig_node_places through ctypes, guard records behind d_place -> (status, host int32 (n + GUARD, 4))"""
    import torch

    n = len(uni["node_unitig"]) if n_nodes is None else n_nodes
    T = len(uni["circular"]) if n_unitigs is None else n_unitigs
    d = {f: _dev(uni[f], tu.DT[f]) for f in tu.FIELDS}
    place = torch.full((n + GUARD, 4), MARK, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    s = eng.lib.s2k_unitig_node_places(eng.ctx if ctx else None, *(_ptr(d[f], f in null) for f in tu.FIELDS), n, T, _ptr(place, "place" in null))
    return s, place.cpu().numpy()


def device_places(eng, uni):
    """-> the place tensor (n, 4) on the device, equal to the reference, guards untouched"""
    import torch

    want = places_reference(uni)
    s, got = raw_places(eng, uni)
    n = len(want)
    assert s == 0 and got[:n].tobytes() == want.tobytes() and (got[n:] == MARK).all()
    return torch.from_numpy(got[:max(n, 1)].copy()).to("cuda:0"), want


def raw_thread(eng, table, km_off, h, rv, mc, dplace, n_unitigs, start=None, end=None, capacity=None, null=(), front=0, uni_items=None, n_nodes=None):
    """s2k_table_thread through ctypes, guard words behind (and `front` words before) every step array -> (status, n_steps, host
    arrays with guards).  null: names of `in` / `out` fields, or "place", to pass as NULL; uni_items: an int64 GPU tensor."""
    import torch

    n = int(km_off[-1])
    nr = len(km_off) - 1
    d = {"km_off": _dev(km_off, np.uint64), "hash": _dev(h, np.uint64), "rev": _dev(rv, np.uint8)}
    if start is not None:
        d["start"], d["end"] = _dev(start, np.uint32), _dev(end, np.uint32)
    i = pkg.DeviceOut()
    i.km_capacity = n
    for f, t in d.items():
        if "in." + f not in null:
            setattr(i, f, t.data_ptr())
    cap = n if capacity is None else capacity
    bufs = {f: torch.full((cap + front + GUARD,), MARK, dtype=torch.int32, device="cuda:0") for f in STEP}
    bufs["path_off"] = torch.full((nr + 1 + GUARD,), MARK, dtype=torch.int64, device="cuda:0")
    o = pkg.ThreadOut()
    o.capacity = cap
    for f, t in bufs.items():
        if f not in null and not (f in ("start", "end") and start is None and "force." + f not in null):
            setattr(o, f, t.data_ptr() + (4 * front if f != "path_off" else 0))
    ns = ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_table_thread(ctypes.c_void_p(table.handle) if table is not None else None, nr, ctypes.byref(i), mc, _ptr(dplace, "place" in null),
                                 table.n if n_nodes is None else n_nodes, ctypes.byref(o), None if uni_items is None else _ptr(uni_items), n_unitigs,
                                 ctypes.byref(ns))
    host = {f: _host(t, np.uint32) for f, t in bufs.items() if f != "path_off"}
    host["path_off"] = _host(bufs["path_off"], np.uint64)
    return s, ns.value, host


def device_thread(eng, table, keys, cnt, km_off, h, rv, mc, dplace, place, n_unitigs, tag, start=None, end=None, front=0):
    """the call against the reference, every array, guards untouched; the sizes-only call; d_uni_items"""
    import torch

    ref = thread_reference(km_off, h, rv, keys, cnt, mc, place, start, end, n_unitigs)
    items = torch.zeros(max(n_unitigs, 1), dtype=torch.int64, device="cuda:0")
    want_n = len(ref["unitig"])
    s, n, host = raw_thread(eng, table, km_off, h, rv, mc, dplace, n_unitigs, start, end, front=front, uni_items=items, capacity=want_n)
    assert (s, n) == (0, want_n), (tag, s, n, want_n)
    nr = len(km_off) - 1
    assert host["path_off"][:nr + 1].tobytes() == ref["path_off"].tobytes() and _marked(host["path_off"], nr + 1), (tag, "path_off")
    for f in STEP:
        if f in ref:
            assert host[f][front: front + n].tobytes() == ref[f].tobytes(), (tag, f, host[f][front: front + n][:20], ref[f][:20])
            assert _marked(host[f], front + n) and _marked(host[f][:front]), (tag, f, "guard")
        else:
            assert _marked(host[f]), (tag, f, "not asked for")
    assert items.cpu().numpy().view(np.uint64)[:n_unitigs].tobytes() == ref["uni_items"].tobytes(), (tag, "uni_items")
    s, n, host = raw_thread(eng, table, km_off, h, rv, mc, dplace, n_unitigs, null=STEP)  # the sizes only
    assert (s, n) == (0, want_n) and host["path_off"][:nr + 1].tobytes() == ref["path_off"].tobytes() and all(_marked(host[f]) for f in STEP), (tag, "sizes")
    return ref


@pytest.mark.gpu
def test_device_hand_made(eng, tmp_path):
    uni = decomposition(*HAND_UNI)
    dplace, place = device_places(eng, uni)
    keys, cnt, km_off, h, rv = hand_batch()
    table = tg._table(eng, keys, cnt)
    for mc in (0, 1, 2, 3, 4):
        ref = device_thread(eng, table, keys, cnt, km_off, h, rv, mc, dplace, place, 4, ("hand", mc))
        assert (mc > 3) == (len(ref["unitig"]) == 0)
    table.close()


@pytest.mark.gpu
def test_device_random_decompositions_and_read_shapes(eng):
    """random tables, random unitigs, reads that walk them with gaps and jumps: read boundaries on items 2047 / 2048 / 2049, more than
    64 read starts in a tile, empty and one-item reads, every min_count from 0 to 3, start / end carried, every alignment of the runs"""
    rng = np.random.default_rng(41)
    done = 0
    for n_keys, lens in ((1, [1]), (50, [3, 0, 2, 1]), (3000, [2047, 1, 1, 2048, 0, 0, 2047, 1, 1, 0, 5000, 1, 0, 2, 3] + [0, 700]),
                         (3000, [1] * 3000 + [0, 1] * 1500 + [0] * 5000 + [3, 0, 0, 2] + [30] * 100), (20000, list(rng.integers(0, 400, size=300))),
                         (5000, [2048] * 3), (5000, [2049, 2047, 2048, 1])):
        keys, cnt = tg._random_table(rng, n_keys)
        uni = random_unitigs(rng, len(keys), max_len=1 + len(keys) // 20)
        dplace, place = device_places(eng, uni)
        table = tg._table(eng, keys, cnt)
        km_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        h, rv = walk_items(rng, km_off, keys, uni)
        n = int(km_off[-1])
        start = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
        end = rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
        for mc in (0, 1, 2, 3):
            ref = device_thread(eng, table, keys, cnt, km_off, h, rv, mc, dplace, place, uni["n_unitigs"], (n_keys, len(lens), mc), start, end, front=done % 4)
            done += 1
        assert n < 100 or (ref["count"].max() > 1 and 0 < len(ref["unitig"]) < ref["n_solid"])
        # random items instead of walks: nearly every solid item is a step of its own
        h, rv = tg._items(rng, km_off, keys, frac=0.85)
        device_thread(eng, table, keys, cnt, km_off, h, rv, 1, dplace, place, uni["n_unitigs"], (n_keys, "random items"))
        table.close()


@pytest.mark.gpu
def test_device_one_step_over_several_tiles_and_edge_shapes(eng):
    """a single read of more than three tiles along one long unitig is one step, forwards and on the twin strand, also round a circular
    unitig several times; n_reads == 0; no solid item at all; an empty table"""
    rng = np.random.default_rng(42)
    keys, cnt = tg._random_table(rng, 9000)
    for circ, n_items in ((0, 7000), (1, 7000), (1, 3 * 7000 + 11)):
        uni = random_unitigs(rng, len(keys), lens=[7000], p_cycle=0.0)
        uni["circular"][0] = circ
        dplace, place = device_places(eng, uni)
        table = tg._table(eng, keys, cnt)
        km_off = np.array([0, 0, n_items, n_items + 5], dtype=np.uint64)
        h, rv = walk_items(rng, km_off, keys, uni, gap=0.0, jump=0.0, t_first=0)
        ref = device_thread(eng, table, keys, cnt, km_off, h, rv, 1, dplace, place, uni["n_unitigs"], ("long", circ, n_items))
        assert ref["path_off"][2] == 1 and ref["count"][0] == n_items and n_items > 3 * 2048
        table.close()
    uni = random_unitigs(rng, len(keys))
    dplace, place = device_places(eng, uni)
    table = tg._table(eng, keys, cnt)
    z = np.zeros(0, dtype=np.uint64)
    s, n, host = raw_thread(eng, table, np.zeros(1, dtype=np.uint64), z, z.astype(np.uint8), 1, dplace, uni["n_unitigs"])  # n_reads == 0
    assert (s, n) == (0, 0) and host["path_off"][0] == 0 and _marked(host["path_off"], 1) and all(_marked(host[f]) for f in STEP)
    km_off = np.array([0, 3000, 3000, 5000], dtype=np.uint64)
    h = rng.integers(0, 2 ** 64, size=5000, dtype=np.uint64)  # none of them a key
    ref = device_thread(eng, table, keys, cnt, km_off, h, np.zeros(5000, dtype=np.uint8), 1, dplace, place, uni["n_unitigs"], "no solid item")
    assert len(ref["unitig"]) == 0
    h, rv = walk_items(rng, km_off, keys, uni)
    ref = device_thread(eng, table, keys, cnt, km_off, h, rv, 5, dplace, place, uni["n_unitigs"], "min_count above every count")
    assert len(ref["unitig"]) == 0
    table.close()
    table = tg._table(eng, z, None)
    s, n, host = raw_thread(eng, table, km_off, h, rv, 1, None, 0, null=("place",))
    assert (s, n) == (0, 0) and (host["path_off"][:4] == 0).all()
    table.close()


@pytest.mark.gpu
def test_device_sizes_capacity_refusals_and_batches(eng):
    import torch

    rng = np.random.default_rng(43)
    keys, cnt = tg._random_table(rng, 4000)
    uni = random_unitigs(rng, len(keys))
    T = uni["n_unitigs"]
    dplace, place = device_places(eng, uni)
    table = tg._table(eng, keys, cnt)
    km_off = np.concatenate([[0], np.cumsum(rng.integers(0, 60, size=400))]).astype(np.uint64)
    h, rv = walk_items(rng, km_off, keys, uni)
    n_items = int(km_off[-1])
    se = rng.integers(0, 2 ** 32, size=(2, n_items), dtype=np.uint32)
    ref = thread_reference(km_off, h, rv, keys, cnt, 1, place, se[0], se[1], T)
    ns, nr = len(ref["unitig"]), len(km_off) - 1
    assert 100 < ns < n_items
    items = torch.zeros(T, dtype=torch.int64, device="cuda:0")
    for cap in (ns - 1, 0):  # short: S2K_ERR_CAPACITY, the size and path_off still set, nothing else written, d_uni_items untouched
        s, n, host = raw_thread(eng, table, km_off, h, rv, 1, dplace, T, se[0], se[1], capacity=cap, uni_items=items)
        assert (s, n) == (7, ns) and host["path_off"][:nr + 1].tobytes() == ref["path_off"].tobytes() and all(_marked(host[f]) for f in STEP), cap
        assert int(items.sum()) == 0
    s, n, host = raw_thread(eng, table, km_off, h, rv, 1, dplace, T, null=("unitig", "count", "flags"))  # some of the arrays
    assert (s, n) == (0, ns) and _marked(host["unitig"]) and host["pos"][:ns].tobytes() == ref["pos"].tobytes() and host["item"][:ns].tobytes() == ref["item"].tobytes()
    # d_uni_items over two batches (the reads split in two) == over one; a sizes-only call adds too
    half = nr // 2
    cut = int(km_off[half])
    for lo, hi in ((0, half), (half, nr)):
        a, b = int(km_off[lo]), int(km_off[hi])
        s, n, host = raw_thread(eng, table, km_off[lo:hi + 1] - km_off[lo], h[a:b], rv[a:b], 1, dplace, T, uni_items=items)
        assert s == 0 and n == int(ref["path_off"][hi] - ref["path_off"][lo])
    assert cut and items.cpu().numpy().view(np.uint64).tobytes() == ref["uni_items"].tobytes()
    s, n, host = raw_thread(eng, table, km_off, h, rv, 1, dplace, T, null=STEP, uni_items=items)
    assert s == 0 and items.cpu().numpy().view(np.uint64).tobytes() == (2 * ref["uni_items"]).tobytes()

    def refused(code=1, **kw):
        args = dict(table=table, km_off=km_off, h=h, rv=rv, mc=1, dplace=dplace, n_unitigs=T)
        args.update(kw)
        s, n, host = raw_thread(eng, **args)
        assert s == code and n == 0 and _marked(host["path_off"]) and all(_marked(host[f]) for f in STEP), (s, n, kw)

    refused(table=None, n_nodes=len(keys))
    for f in ("in.km_off", "in.hash", "in.rev", "path_off", "place"):
        refused(null=(f,))
    refused(null=("force.start",))  # out->start without in->start
    refused(null=("force.end",))
    refused(n_nodes=len(keys) - 1)  # not the table's key count
    refused(n_nodes=len(keys) + 1)
    bad = km_off.copy()
    bad[0] = 1
    refused(km_off=bad)
    x = place.copy()  # a record that names a unitig >= n_unitigs / a position outside it, used by a solid item
    node = int(np.searchsorted(keys, h[np.nonzero(np.isin(h, keys))[0][0]]))
    x["unitig"][node] = 2 * T
    refused(dplace=torch.from_numpy(x.view(np.int32).reshape(-1, 4).copy()).to("cuda:0"))
    x = place.copy()
    x["pos"][node] = x["len"][node]
    refused(dplace=torch.from_numpy(x.view(np.int32).reshape(-1, 4).copy()).to("cuda:0"))
    z = ctypes.c_uint64(5)
    assert eng.lib.s2k_table_thread(ctypes.c_void_p(table.handle), 1, None, 1, None, 0, None, None, 0, ctypes.byref(z)) == 1 and z.value == 0
    table.close()

    # places: arrays that are no decomposition are refused with nothing written
    def refused_places(**kw):
        u = dict(uni)
        null = kw.pop("null", ())
        ctx = kw.pop("ctx", True)
        sizes = {k: kw.pop(k) for k in ("n_nodes", "n_unitigs") if k in kw}
        u.update(kw)
        s, got = raw_places(eng, u, null=null, ctx=ctx, **sizes)
        assert s == 1 and (got == MARK).all(), (s, list(kw))

    for f, v in (("node_unitig", T), ("node_unitig", 2 ** 32 - 1), ("node_pos", 2 ** 31)):
        y = uni[f].copy()
        y[17] = v
        refused_places(**{f: y})
    t17 = int(uni["node_unitig"][17])
    y = uni["node_pos"].copy()  # pos == len
    y[17] = int(uni["uni_off"][t17 + 1] - uni["uni_off"][t17])
    refused_places(node_pos=y)
    y = uni["node_unitig"].copy()  # another unitig's node
    y[17] = (t17 + 1) % T
    y2 = uni["node_pos"].copy()
    y2[17] = 0
    refused_places(node_unitig=y, node_pos=y2)
    y = uni["members"].copy()  # the member there is another node
    a = int(uni["uni_off"][t17]) + int(uni["node_pos"][17])
    y[a] = (int(y[a]) + 2) % (2 * len(keys))
    refused_places(members=y)
    y = uni["uni_off"].copy()  # a unitig that runs past the nodes
    y[-1] += np.uint64(5)
    refused_places(uni_off=y)
    refused_places(n_unitigs=T - 1)
    refused_places(ctx=False)
    for f in tu.FIELDS + ("place",):
        refused_places(null=(f,))
    assert eng.lib.s2k_unitig_node_places(eng.ctx, *([ctypes.c_void_p(16)] * 5), 2 ** 31, 1, ctypes.c_void_p(16)) == 1  # before anything is read
    assert eng.lib.s2k_unitig_node_places(eng.ctx, *([None] * 5), 0, 0, None) == 0


@pytest.mark.gpu
def test_device_deterministic(eng):
    rng = np.random.default_rng(44)
    keys, cnt = tg._random_table(rng, 50000)
    uni = random_unitigs(rng, len(keys), max_len=300)
    dplace, place = device_places(eng, uni)
    table = tg._table(eng, keys, cnt)
    km_off = np.concatenate([[0], np.cumsum(rng.integers(0, 900, size=200))]).astype(np.uint64)
    h, rv = walk_items(rng, km_off, keys, uni)
    runs = []
    for _ in range(2):
        import torch

        items = torch.zeros(uni["n_unitigs"], dtype=torch.int64, device="cuda:0")
        s, n, host = raw_thread(eng, table, km_off, h, rv, 2, dplace, uni["n_unitigs"], uni_items=items)
        assert s == 0 and n > 1000
        runs.append(b"".join(host[f].tobytes() for f in sorted(host)) + items.cpu().numpy().tobytes())
    assert runs[0] == runs[1]
    table.close()


def _extract_se(eng, reads, l, k, d, mode):
    """tg._extract_dev with start and end kept"""
    import torch

    bases, off = pkg.pack_reads(reads)
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
    cap = len(bases) + 1
    t = {"km_off": torch.empty(len(reads) + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
         "rev": torch.empty(cap, dtype=torch.uint8, device=dev), "start": torch.empty(cap, dtype=torch.int32, device=dev),
         "end": torch.empty(cap, dtype=torch.int32, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = cap
    for f, x in t.items():
        setattr(o, f, x.data_ptr())
    torch.cuda.synchronize()
    eng.extract_device(db.data_ptr(), do.data_ptr(), len(reads), len(bases), l, k, d, int(mode), o)
    return t


def _same_paths(got, ref, tag):
    for f in ("path_off",) + STEP:
        assert got[f].tobytes() == ref[f].tobytes(), (tag, f)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,l,k", [(pkg.HashMode.Regular, 12, 5), (pkg.HashMode.Hpc, 21, 3)])
def test_ecoli_reads_with_errors_end_to_end(eng, oracle, ecoli, tmp_path, mode, l, k):
    """600 E. coli reads with 0.5 % substitutions, half of them reverse-complemented: KminmerGraph.build -> unitigs -> thread, then
    simplify -> a table over the simplified graph -> unitigs -> thread, both equal to the references run on the oracle's k-min-mers;
    at min_edge_count 1 every linked transition of the device's paths is a unitig edge; Regular: the reverse complement of every read
    has the reversed path on the twin strands"""
    import torch

    d, mc = 0.05, 2
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    b = oracle.batch(*pkg.pack_reads(reads), l, k, d, int(mode))
    outs = _extract_se(eng, reads, l, k, d, mode)
    nr = len(reads)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=mc, min_edge_count=1)
    g = tg.graph_reference([b], mc, 1)
    tg._assert_graph(tg._graph_host(graph), g, "build")
    sg, node_map, _ = graph.simplify(eng, 10, 20)
    final, ref_map, _ = ts.simplify_rounds_reference(g, 10, 20)
    assert node_map.cpu().numpy().tobytes() == ref_map.tobytes() and sg.n_nodes < graph.n_nodes
    for tag, dg, rg in (("built", graph, g), ("simplified", sg, final)):
        uni = tu.unitig_reference(rg["row_off"], rg["dst"], len(rg["keys"]))
        place = places_reference(uni)
        ref = thread_reference(b["km_off"], b["hash"], b["rev"], rg["keys"], rg["counts"], mc, place, b["start"], b["end"], uni["n_unitigs"])
        ug = dg.unitigs(eng)
        assert ug.places(eng).cpu().numpy().tobytes() == place.tobytes() and ug.places(eng) is ug.places(eng)
        table = pkg.CountTable(eng, dg.keys, dg.counts)
        cov = torch.zeros(ug.n_unitigs, dtype=torch.int64, device="cuda:0")
        paths = ug.thread(eng, table, outs, nr, min_count=mc, coverage=cov)
        got = paths.host()
        _same_paths(got, ref, (tag, int(mode)))
        assert cov.cpu().numpy().view(np.uint64).tobytes() == ref["uni_items"].tobytes()
        assert paths.n_steps == len(ref["unitig"]) > 1000 and int(got["count"].sum()) == ref["n_solid"]
        lens = np.diff(uni["uni_off"].astype(np.int64)).tolist()
        n = linked_transitions_follow_edges(got, lens, uni["circular"].tolist(), tg._u64(ug.edge_keys))
        print("%s %s: %d unitigs, %d steps over %d solid items, %d linked transitions" % (mode.name, tag, ug.n_unitigs, paths.n_steps, ref["n_solid"], n))
        assert n > 100
        p = str(tmp_path / "paths.tsv")
        paths.write_paths(p, first_read=3)
        lines = open(p).read().split("\n")
        assert len(lines) == nr + 1 and lines[0].split("\t")[:2] == ["3", str(int(got["path_off"][1]))]
        if mode == pkg.HashMode.Regular:
            rc = _extract_se(eng, [tg._revcomp(r) for r in reads], l, k, d, mode)
            back = ug.thread(eng, table, rc, nr, min_count=mc).host()
            po, qo = got["path_off"].astype(np.int64), back["path_off"].astype(np.int64)
            assert (po == qo).all()
            order = np.concatenate([np.arange(z - 1, a - 1, -1) for a, z in zip(po[:-1], po[1:])]).astype(np.int64)  # each read's steps reversed
            assert (back["unitig"] == got["unitig"][order] ^ 1).all() and (back["count"] == got["count"][order]).all()
            ln = np.array(lens, dtype=np.int64)[got["unitig"][order] >> 1]
            last = got["pos"][order].astype(np.int64) + got["count"][order] - 1
            circ = uni["circular"][got["unitig"][order] >> 1] != 0
            assert (back["pos"] == ln - 1 - np.where(circ, last % ln, last)).all()
        table.close()


@pytest.mark.gpu
def test_error_free_reads_whose_graph_is_one_unitig(eng, ecoli):
    """error-free reads that tile one stretch of the genome: the graph is one unitig, and every read with items is one step that holds
    all of them"""
    rng = np.random.default_rng(12)
    region = ecoli[20000:50000]
    reads = [bytes(region[a: a + 3000]) for a in list(range(0, 27001, 500)) * 2]
    reads = [tg._revcomp(r) if rng.random() < 0.5 else r for r in reads]
    outs = _extract_se(eng, reads, 12, 5, 0.05, pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=2)
    ug = graph.unitigs(eng)
    assert ug.n_unitigs == 1 and graph.n_nodes > 100
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    got = ug.thread(eng, table, outs, len(reads), min_count=2).host()
    table.close()
    n_items = np.diff(tg._u64(outs["km_off"]).astype(np.int64))  # every read occurs twice: every k-min-mer is solid
    has = n_items > 0
    assert has.sum() > 100 and (np.diff(got["path_off"].astype(np.int64))[has] == 1).all() and (got["count"] == n_items[has]).all()
    assert (got["unitig"] >> 1 == 0).all() and (got["flags"] == 0).all() and (got["item"] == 0).all()


@pytest.mark.gpu
def test_full_size_config1_thread(eng, oracle):
    """configs[1] (1 000 000 x 10 kbp synthetic reads, l=31 k=10 d=0.01, Hpc) against a table of every second key (min_count 1), as
    test_graph.test_full_size_config1_edges sets it up, over a decomposition of the table's nodes into unitigs of eight members with
    mixed orientations, every third one circular: the totals equal s2k_table_filter's, and 1 % of the reads equal the reference step
    by step"""
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
    del k, cc
    N = half_k.numel()
    # the decomposition, on the device: node i is member i % 8 of unitig i // 8, oriented by a bit of its index
    T = (N + 7) // 8
    ids = torch.arange(N, dtype=torch.int64, device=dev)
    ug = pkg.UnitigGraph(torch.clamp(torch.arange(T + 1, dtype=torch.int64, device=dev) * 8, max=N), (2 * ids + ((ids * 2654435761 >> 9) & 1)).to(torch.int32),
                         (ids // 8).to(torch.int32), (ids % 8).to(torch.int32), (torch.arange(T, device=dev) % 3 == 0).to(torch.uint8), None, None, None, None, None)
    del ids
    table = pkg.CountTable(eng, half_k, half_c)
    filt = pkg.SolidOut()
    fko = torch.empty(n_reads + 1, dtype=torch.int64, device=dev)
    filt.km_off = fko.data_ptr()
    i = pkg.DeviceOut()
    i.km_capacity = n
    i.km_off, i.hash = t["km_off"].data_ptr(), t["hash"].data_ptr()
    kept = ctypes.c_uint64(0)
    torch.cuda.synchronize()
    eng._check(eng.lib.s2k_table_filter(table.handle, n_reads, ctypes.byref(i), 1, ctypes.byref(filt), ctypes.byref(kept)))
    cov = torch.zeros(T, dtype=torch.int64, device=dev)
    paths = ug.thread(eng, table, t, n_reads, min_count=1, coverage=cov)
    table.close()
    assert int(paths.count.sum()) == kept.value == int(cov.sum()) and kept.value > 40 * 10 ** 6
    assert int(paths.path_off[-1]) == paths.n_steps and int(paths.path_off[0]) == 0 and bool((paths.path_off[1:] >= paths.path_off[:-1]).all())
    # 1 % of the reads against the reference, their items and the table's half of the keys on the host
    ids = gpu_util.spread_sample(n_reads, 0.01, np.random.default_rng(5))
    km = tg._u64(t["km_off"])
    a, z = km[ids].astype(np.int64), km[ids + 1].astype(np.int64)
    sel = torch.from_numpy(np.concatenate([np.arange(x, y) for x, y in zip(a, z)])).to(dev)
    h, rv = tg._u64(t["hash"][sel]), t["rev"][sel].cpu().numpy()
    sub_off = np.concatenate([[0], np.cumsum(z - a)]).astype(np.uint64)
    keys_h = tg._u64(half_k)  # the reference runs on the nodes the sampled items name: a sub-table, and their place records
    at = np.minimum(np.searchsorted(keys_h, h), N - 1)
    used = np.unique(at[keys_h[at] == h])
    place_h = np.ascontiguousarray(ug.places(eng)[torch.from_numpy(used).to(dev)].cpu().numpy()).view(pkg.NodePlace).reshape(-1)
    ref = thread_reference(sub_off, h, rv, keys_h[used], None, 1, place_h)
    got = paths.host()
    po = got["path_off"].astype(np.int64)
    assert (np.diff(ref["path_off"].astype(np.int64)) == po[ids + 1] - po[ids]).all()
    steps = np.concatenate([np.arange(x, y) for x, y in zip(po[ids], po[ids + 1])])
    for f in ("unitig", "pos", "count", "item", "flags"):
        assert got[f][steps].tobytes() == ref[f].tobytes(), f
    assert len(steps) > 400000
