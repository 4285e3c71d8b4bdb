"""Read walks on the unitig graph with base coordinates, and GAF export: s2k_unitig_member_offsets and s2k_paths_walks (include/s2k.h,
DESIGN.md §3.16).  The references are `member_offsets_reference` and `walks_reference`, serial restatements of the header's definitions
built on the references of test_span.py and test_unitig_sequences.py; the device's arrays equal theirs exactly, every one of them, in
every test."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import test_graph as tg
import test_simplify as ts
import test_span as tsp
import test_thread as tt
import test_unitig_sequences as tus
import test_unitigs as tu
import test_untangle as tun
from test_span import repeat_case  # noqa: F401  (the module-scoped fixture of the repeat)

pkg = import_package()

SYMS = ("s2k_unitig_member_offsets", "s2k_paths_walks")
LINKED = 1
NONE = 0xFFFFFFFF
REC64 = ("first_step", "items", "path_len", "path_start", "path_end")
REC32 = ("n_steps", "qstart", "qend", "flags")
WALK_DT = dict({f: np.uint64 for f in REC64 + ("walk_off",)}, **{f: np.uint32 for f in REC32 + ("edge",)})


# ---- the references ----------------------------------------------------------------------------------------------------------------
def member_offsets_reference(uni, nodes):
    """uni: uni_off, members, circular; nodes: seq_len, shift_fwd, shift_rev, rev (numbers only) -> dict member_off, out_off uint64,
    overlap uint32: the piece of a member is shift(u) bases, the whole sequence for the last member of a unitig that is not circular"""
    off, mem = [int(x) for x in uni["uni_off"]], [int(x) for x in uni["members"]]
    sl, sf, sr, rv = ([int(x) for x in nodes[f]] for f in ("seq_len", "shift_fwd", "shift_rev", "rev"))
    shift = lambda u: sf[u >> 1] if (u & 1) == rv[u >> 1] else sr[u >> 1]  # noqa: E731
    T = len(off) - 1
    mo, oo, ov, pos = [], [0], [], 0
    for t in range(T):
        for x in range(off[t], off[t + 1]):
            mo.append(pos)
            pos += sl[mem[x] >> 1] if (x == off[t + 1] - 1 and not uni["circular"][t]) else shift(mem[x])
        oo.append(pos)
        for u in (mem[off[t + 1] - 1], mem[off[t]] ^ 1):
            ov.append(sl[u >> 1] - shift(u))
    return {"member_off": np.array(mo, dtype=np.uint64), "out_off": np.array(oo, dtype=np.uint64), "overlap": np.array(ov, dtype=np.uint32)}


def follow_reference(paths, row_off, dst, uni_off):
    """the edge every step follows (None: none), by the rule of include/s2k.h: what spans_reference computes inside"""
    ro, d, off = [int(x) for x in row_off], [int(x) for x in dst], [int(x) for x in uni_off]
    po = [int(x) for x in paths["path_off"]]
    u, p, c, f = ([int(x) for x in paths[k]] for k in tsp.PATH)
    follow = [None] * len(u)
    for r in range(len(po) - 1):
        for s in range(po[r] + 1, po[r + 1]):
            if f[s] & LINKED and p[s] == 0 and p[s - 1] + c[s - 1] == off[(u[s - 1] >> 1) + 1] - off[u[s - 1] >> 1]:
                follow[s] = tsp._find(ro, d, u[s - 1], u[s])
    return follow


def interval_reference(uni, mo, seq_len, U, q):
    """-> (lo, hi, L, w): the base interval of position q of the oriented unitig U, the unitig's bases, and the raise w that is part of
    lo and hi (the twin strand of a circular unitig only)"""
    t, s = U >> 1, U & 1
    a, ln = int(uni["uni_off"][t]), int(uni["uni_off"][t + 1]) - int(uni["uni_off"][t])
    L = int(mo["out_off"][t + 1]) - int(mo["out_off"][t])
    x = a + (ln - 1 - q if s else q)
    o = int(mo["member_off"][x]) - int(mo["out_off"][t])
    e = o + int(seq_len[int(uni["members"][x]) >> 1])
    if not uni["circular"][t]:
        e = min(e, L)
    if s == 0:
        return o, e, L, 0
    w = 0
    if e > L:
        w = ((e - 1) // L) * L if L else e
    return w + L - e, w + L - o, L, w


def walks_reference(paths, row_off, dst, uni, mo, seq_len):
    """paths: path_off, unitig, pos, count, flags, start, end -> dict of the walk arrays, edge (uint32 per step), n_walks, n_followed,
    n_off_graph"""
    follow = follow_reference(paths, row_off, dst, uni["uni_off"])
    po = [int(x) for x in paths["path_off"]]
    u, p, c, f = ([int(x) for x in paths[k]] for k in tsp.PATH)
    st, en = [int(x) for x in paths["start"]], [int(x) for x in paths["end"]]
    off = [int(x) for x in uni["uni_off"]]
    L = lambda U: int(mo["out_off"][(U >> 1) + 1]) - int(mo["out_off"][U >> 1])  # noqa: E731
    adv = lambda U: L(U) - min(int(mo["overlap"][U]), L(U))  # noqa: E731
    w = {k: [] for k in REC64 + REC32}
    walk_off = [0]
    for r in range(len(po) - 1):
        s = po[r]
        while s < po[r + 1]:
            e = s + 1
            while e < po[r + 1] and follow[e] is not None:
                e += 1
            last = e - 1
            base = sum(adv(u[x]) for x in range(s, last))
            lo, _, _, wr = interval_reference(uni, mo, seq_len, u[s], p[s])
            ln = off[(u[last] >> 1) + 1] - off[u[last] >> 1]
            q = p[last] + c[last] - 1
            _, hi, Lt, w2 = interval_reference(uni, mo, seq_len, u[last], q % ln)
            circ = int(uni["circular"][u[last] >> 1])
            assert q < ln or (circ and s == last)
            for k, v in (("first_step", s), ("n_steps", e - s), ("items", sum(c[s:e])), ("qstart", st[s]), ("qend", en[last] + 1),
                         ("path_len", base + Lt), ("path_start", lo), ("path_end", base + (hi - w2) + wr + (q // ln) * Lt), ("flags", circ)):
                w[k].append(v)
            s = e
        walk_off.append(len(w["first_step"]))
    out = {k: np.array(v, dtype=WALK_DT[k]) for k, v in w.items()}
    out["walk_off"] = np.array(walk_off, dtype=np.uint64)
    out["edge"] = np.array([NONE if x is None else x for x in follow], dtype=np.uint32)
    out["n_walks"] = len(w["first_step"])
    out["n_followed"] = sum(1 for x in follow if x is not None)
    out["n_off_graph"] = sum(1 for s, x in enumerate(f) if x & LINKED and follow[s] is None)
    return out


def check_walk_invariants(ref, paths, tag):
    """every step in exactly one walk, in order; coordinates ordered; the totals those of spans_reference"""
    n = len(paths["unitig"])
    fs, ns = ref["first_step"].astype(np.int64), ref["n_steps"].astype(np.int64)
    assert (fs + ns)[:-1].tolist() == fs[1:].tolist() and (n == 0 or (fs[0] == 0 and fs[-1] + ns[-1] == n)), tag
    assert int(ref["items"].sum()) == int(paths["count"].astype(np.int64).sum()), tag
    lin = ref["flags"] == 0
    assert (ref["path_start"] <= ref["path_end"]).all() and (ref["path_end"][lin] <= ref["path_len"][lin]).all(), tag
    assert (ref["n_steps"][~lin] == 1).all() and ref["n_walks"] + ref["n_followed"] == n, tag


def gaf_text(tmp_path, ref, paths, name="ref.gaf", **kw):
    p = str(tmp_path / name)
    pkg.write_gaf_walks(p, ref, paths["unitig"], **kw)
    return open(p).read()


# ---- hand-made: five unitigs over eleven nodes -------------------------------------------------------------------------------------
#  unitig 0: nodes 0+ 1-; unitig 1: 2+ 3+ 4-; unitig 2: 5- 6+; unitig 3: 7+ 8+ 9- round; unitig 4: 10+, with a hairpin
#  edges: 0+ > 1-, 1- > 2+ (unitig 1 is crossed on its twin strand), 4+ > 4- (its own twin), and their twins
W_MEMBERS = ([[0, 3], [4, 6, 9], [11, 12], [14, 16, 19], [20]], [0, 0, 0, 1, 0])
W_EDGES = [(0, 3), (3, 4), (8, 9)]
W_NODES = {"seq_len": [10, 11, 12, 10, 9, 13, 10, 8, 9, 10, 7], "shift_fwd": [4, 5, 3, 4, 2, 6, 4, 3, 4, 5, 3], "shift_rev": [3, 4, 5, 2, 4, 5, 3, 2, 3, 4, 2],
           "rev": [0, 1, 0, 0, 1, 0, 1, 0, 1, 0, 0]}
L_ = LINKED
# name -> steps (unitig, pos, count, flags, start, end)
W_READS = {
    "no steps": [],
    "a single step": [(2, 1, 2, 0, 5, 30)],
    "two steps joined by an edge": [(0, 0, 2, 0, 0, 13), (3, 0, 3, L_, 4, 27)],
    "two steps linked but off-graph": [(0, 0, 2, 0, 0, 13), (4, 0, 2, L_, 4, 22)],
    "a walk that starts at a gap": [(0, 0, 2, 0, 0, 13), (0, 0, 2, 0, 40, 53), (3, 0, 3, L_, 44, 67)],
    "a reverse-strand unitig in the middle": [(0, 1, 1, 0, 7, 17), (3, 0, 3, L_, 8, 31), (4, 0, 1, L_, 25, 37)],
    "the same on the other strand": [(5, 0, 2, 0, 0, 19), (2, 0, 3, L_, 6, 29), (1, 0, 2, L_, 20, 37)],
    "a circular unitig, twice round": [(6, 1, 7, 0, 3, 40)],
    "its twin strand, past the end": [(7, 2, 3, 0, 2, 20)],
    "a hairpin": [(8, 0, 1, 0, 0, 6), (9, 0, 1, L_, 4, 10)],
}
W_GAF = """\
6\t*\t5\t31\t+\t>1\t16\t3\t16\t2\t26\t255\tkm:i:2\tns:i:1
7\t*\t0\t28\t+\t>0<1\t25\t0\t25\t5\t28\t255\tkm:i:5\tns:i:2
8\t*\t0\t14\t+\t>0\t15\t0\t15\t2\t15\t255\tkm:i:2\tns:i:1
8\t*\t4\t23\t+\t>2\t15\t0\t15\t2\t19\t255\tkm:i:2\tns:i:1
9\t*\t0\t14\t+\t>0\t15\t0\t15\t2\t15\t255\tkm:i:2\tns:i:1
9\t*\t40\t68\t+\t>0<1\t25\t0\t25\t5\t28\t255\tkm:i:5\tns:i:2
10\t*\t7\t38\t+\t>0<1>2\t33\t4\t31\t5\t31\t255\tkm:i:5\tns:i:3
11\t*\t0\t38\t+\t<2>1<0\t32\t0\t32\t7\t38\t255\tkm:i:7\tns:i:3
12\t*\t3\t41\t+\t>3\t10\t3\t32\t7\t38\t255\tkm:i:7\tns:i:1
13\t*\t2\t21\t+\t<3\t10\t2\t17\t3\t19\t255\tkm:i:3\tns:i:1
14\t*\t0\t11\t+\t>4<4\t10\t0\t10\t2\t11\t255\tkm:i:2\tns:i:2
"""


def walk_hand():
    uni = tt.decomposition(*W_MEMBERS)
    ro, d = tu.csr_of(5, W_EDGES)
    nodes = {f: np.array(v, dtype=np.uint8 if f == "rev" else np.uint32) for f, v in W_NODES.items()}
    return uni, ro, d, nodes, member_offsets_reference(uni, nodes)


def walk_paths_of(reads):
    steps = [s for r in reads for s in r]
    out = {f: np.array([s[i] for s in steps], dtype=np.uint32) for i, f in enumerate(tsp.PATH + ("start", "end"))}
    out["path_off"] = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return out


# ---- generators -------------------------------------------------------------------------------------------------------------------
def random_records(rng, n):
    sl = rng.integers(4, 40, size=n)
    return {"seq_len": sl.astype(np.uint32), "shift_fwd": rng.integers(1, sl + 1).astype(np.uint32), "shift_rev": rng.integers(1, sl + 1).astype(np.uint32),
            "rev": rng.integers(0, 2, size=n).astype(np.uint8)}


def cut_paths(paths, n):
    """the first n steps"""
    out = {f: paths[f][:n] for f in tsp.PATH + ("start", "end")}
    out["path_off"] = np.minimum(paths["path_off"], np.uint64(n))
    return out


def walked_case(rng, n_keys, lens, n_steps=None, keep_edges=0.8, max_len=3):
    """tsp.walked_paths with the whole decomposition kept, start / end carried, random node records, cut to n_steps steps"""
    keys, cnt = tg._random_table(rng, n_keys)
    uni = tt.random_unitigs(rng, len(keys), max_len=max_len, p_cycle=0.1)
    km_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    h, rv = tt.walk_items(rng, km_off, keys, uni, gap=0.02, jump=0.02)
    within = np.arange(len(h)) - np.repeat(km_off[:-1].astype(np.int64), np.diff(km_off.astype(np.int64)))
    start = (7 * within).astype(np.uint32)
    paths = tt.thread_reference(km_off, h, rv, keys, cnt, 1, tt.places_reference(uni), start=start, end=start + np.uint32(30), n_unitigs=uni["n_unitigs"])
    if n_steps is not None:
        assert len(paths["unitig"]) >= n_steps, (len(paths["unitig"]), n_steps)
        paths = cut_paths(paths, n_steps)
    u, f, p = paths["unitig"].tolist(), paths["flags"].tolist(), paths["pos"].tolist()
    edges = [(u[s - 1], u[s]) for s in range(1, len(u)) if f[s] & LINKED and not uni["circular"][u[s] >> 1] and not uni["circular"][u[s - 1] >> 1]
             and rng.random() < keep_edges]
    ro, d = tu.csr_of(uni["n_unitigs"], edges)
    nodes = random_records(rng, len(keys))
    return {"paths": paths, "ro": ro, "d": d, "uni": uni, "nodes": nodes, "mo": member_offsets_reference(uni, nodes)}


def chained_case(rng, T, lens, p_break=0.0):
    """tsp.chained_paths over a decomposition whose unitig t holds the nodes uni_off[t] .., start / end made up"""
    paths, ro, d, off, T = tsp.chained_paths(rng, T, lens, p_break)
    n = int(off[-1])
    ln = np.diff(off.astype(np.int64))[paths["unitig"] >> 1]
    paths["pos"] = np.minimum(paths["pos"], ln - paths["count"]).astype(np.uint32)  # a broken step of tsp.chained_paths may lie past a one-member unitig
    uni = tt.decomposition([list(range(2 * int(a), 2 * int(b), 2)) for a, b in zip(off[:-1], off[1:])], [0] * T)
    paths["start"] = (np.arange(len(paths["unitig"])) * 3).astype(np.uint32)
    paths["end"] = paths["start"] + np.uint32(20)
    nodes = random_records(rng, n)
    return {"paths": paths, "ro": ro, "d": d, "uni": uni, "nodes": nodes, "mo": member_offsets_reference(uni, nodes)}


def long_chain_case(T=5000):
    """T one-member unitigs in a chain, one read along it and one along its twin strand: two walks of T steps"""
    rng = np.random.default_rng(T)
    uni = tt.decomposition([[2 * t + (t % 2)] for t in range(T)], [0] * T)
    ro, d = tu.csr_of(T, [(2 * t, 2 * t + 2) for t in range(T - 1)])
    fwd = [(2 * t, 0, 1, L_ if t else 0, 11 * t, 11 * t + 35) for t in range(T)]
    bwd = [(2 * t + 1, 0, 1, L_ if t != T - 1 else 0, 11 * (T - 1 - t), 11 * (T - 1 - t) + 35) for t in range(T - 1, -1, -1)]
    nodes = random_records(rng, T)
    return {"paths": walk_paths_of([fwd, bwd]), "ro": ro, "d": d, "uni": uni, "nodes": nodes, "mo": member_offsets_reference(uni, nodes)}


def reference_of(case):
    return walks_reference(case["paths"], case["ro"], case["d"], case["uni"], case["mo"], case["nodes"]["seq_len"])


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert hasattr(pkg.Engine, "unitig_member_offsets") and hasattr(pkg.Engine, "paths_walks")
    assert all(hasattr(pkg.UnitigGraph, f) for f in ("member_offsets", "walks"))
    assert hasattr(pkg, "ReadWalks") and hasattr(pkg.ReadWalks, "write_gaf") and hasattr(pkg, "write_gaf_walks")


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "walk_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "walk_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    W = pkg.WalkOut
    assert facts["sizeof.s2k_walk_out"] == (ctypes.sizeof(W),)
    for f, t in W._fields_:
        assert facts["s2k_walk_out." + f] == (getattr(W, f).offset, ctypes.sizeof(t)), f
    assert facts["S2K_WALK_CIRCULAR"] == (pkg.WALK_CIRCULAR,) and facts["S2K_NO_EDGE"] == (pkg.NO_EDGE,) == (NONE,)


def test_cpp_walk_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "walk_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "walk_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "s2k_walk.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))
    assert "s2k_walk.hip" in next(line for line in open(os.path.join(csrc, "Makefile.asan")).read().split("\n") if line.startswith("ASAN_SRCS"))


def test_references_hand_made(tmp_path):
    uni, ro, d, nodes, mo = walk_hand()
    assert tu.is_twin_symmetric(ro, d, 5) and len(d) == 5
    #   unitig 0: 0+ fwd 4, 1- whole 11; unitig 1: 2+ 3, 3+ 4, 4- whole 9; unitig 2: 5- 5, 6+ whole 10; unitig 3 (round): 3, 3, 4; unitig 4: 7
    assert mo["member_off"].tolist() == [0, 4, 15, 18, 22, 31, 36, 46, 49, 52, 56] and mo["out_off"].tolist() == [0, 15, 31, 46, 56, 63]
    assert mo["overlap"].tolist() == [6, 7, 7, 7, 7, 7, 6, 6, 4, 5]
    paths = walk_paths_of(list(W_READS.values()))
    ref = walks_reference(paths, ro, d, uni, mo, nodes["seq_len"])
    check_walk_invariants(ref, paths, "hand")
    assert ref["walk_off"].tolist() == [0, 0, 1, 2, 4, 6, 7, 8, 9, 10, 11] and ref["n_followed"] == 7 and ref["n_off_graph"] == 1
    assert ref["edge"].tolist() == [NONE, NONE, 0, NONE, NONE, NONE, NONE, 0, NONE, 0, 2, NONE, 3, 1, NONE, NONE, NONE, 4]
    assert ref["flags"].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0]
    sp = tsp.spans_reference(paths, ro, d, uni["uni_off"])
    assert (sp["n_followed"], sp["n_off_graph"]) == (ref["n_followed"], ref["n_off_graph"])
    # the circular unitig: L = 10, pieces 3, 3, 4.  Seven items from position 1: the six pieces 3 4 3 3 4 3 = 20, then node 8 whole, 9
    # bases: from base 3 to base 32.  Its twin strand from position 2 (members 0, 2, 1; they end at 8, 16, 12, so they begin at 10 - 8 =
    # 2, 4 and 8 of the twin): from base 2 to 8 + 9 = 17
    w = int(ref["walk_off"][7])
    assert [(int(ref[f][w]), int(ref[f][w + 1])) for f in ("path_start", "path_end", "path_len")] == [(3, 2), (32, 17), (10, 10)]
    assert gaf_text(tmp_path, ref, paths, first_read=5) == W_GAF
    named = gaf_text(tmp_path, ref, paths, names=["r%d" % i for i in range(10)], read_lengths=[100 + i for i in range(10)])
    assert named.split("\n")[0].split("\t")[:2] == ["r1", "101"] and named.count("\n") == 11


def test_hand_made_intervals_against_stitched_bytes():
    """the numeric intervals against real bytes: the circle of test_unitig_sequences.py (ACGTTGCAG, three members, the last reaches
    round) on both strands, and a chain; seq(position) == the stitched unitig read round, at the interval"""
    for name in ("circle", "chain ++", "twin -+"):
        batches, strings, _, circ = tus.HAND[name]
        g, uni, nodes, seqs = tus.reference_pipeline(batches, 2, 1)
        mo = member_offsets_reference(uni, nodes)
        assert mo["out_off"].tobytes() == seqs["out_off"].tobytes() and mo["overlap"].tobytes() == seqs["overlap"].tobytes(), name
        for t, s in enumerate(tus.unitig_strings(uni, seqs)):
            ln = int(uni["uni_off"][t + 1] - uni["uni_off"][t])
            for U in (2 * t, 2 * t + 1):
                strand = s if U % 2 == 0 else tus.revcomp(s)
                for q in range(ln):
                    lo, hi, L, w = interval_reference(uni, mo, nodes["seq_len"], U, q)
                    x = int(uni["uni_off"][t]) + (ln - 1 - q if U & 1 else q)
                    m = int(uni["members"][x]) ^ (U & 1)
                    assert 0 <= lo <= hi and L == len(s) and (uni["circular"][t] or hi <= L), (name, U, q)
                    assert (strand * 3)[lo:hi] == tus.oriented(nodes, m)[0], (name, U, q, lo, hi)


def test_reference_random_decompositions_invariants():
    rng = np.random.default_rng(61)
    seen = [0, 0, 0]
    for n_keys, lens in ((40, [30, 0, 1, 25]), (300, [200] * 5), (600, list(rng.integers(0, 60, size=120)))):
        case = walked_case(rng, n_keys, lens)
        ref = reference_of(case)
        check_walk_invariants(ref, case["paths"], n_keys)
        sp = tsp.spans_reference(case["paths"], case["ro"], case["d"], case["uni"]["uni_off"])
        assert (sp["n_followed"], sp["n_off_graph"]) == (ref["n_followed"], ref["n_off_graph"])
        seen = [seen[0] + ref["n_followed"], seen[1] + int((ref["n_steps"] > 1).sum()), seen[2] + int(ref["flags"].sum())]
    case = chained_case(rng, 50, [7] * 100, p_break=0.1)
    ref = reference_of(case)
    check_walk_invariants(ref, case["paths"], "chain")
    assert seen[0] > 50 and seen[1] > 30 and seen[2] > 5 and int(ref["n_steps"].max()) == 7, seen
    ref = reference_of(long_chain_case(300))
    assert ref["n_steps"].tolist() == [300, 300] and ref["path_start"].tolist() == [0, 0] and ref["path_end"].tolist() == ref["path_len"].tolist()


# ---- the repeat fixture, before and after untangling ---------------------------------------------------------------------------------
def stitched_path(strings, overlap, units):
    """the unitig sequences on the walk's strands, each after the first without the overlap that leaves the one before it"""
    out = b""
    for i, U in enumerate(units):
        s = strings[U >> 1] if U % 2 == 0 else tus.revcomp(strings[U >> 1])
        out += s if i == 0 else s[int(overlap[units[i - 1]]):]
    return out


def assert_walks_are_substrings(ref, paths, reads, strings, overlap, tag):
    """read[qstart:qend] == the stitched path [path_start:path_end], for every walk"""
    wo, u = ref["walk_off"].astype(np.int64), paths["unitig"].tolist()
    for r in range(len(wo) - 1):
        for w in range(wo[r], wo[r + 1]):
            a, n = int(ref["first_step"][w]), int(ref["n_steps"][w])
            path = stitched_path(strings, overlap, u[a: a + n])
            assert len(path) == int(ref["path_len"][w]), (tag, r, w)
            assert reads[r][int(ref["qstart"][w]): int(ref["qend"][w])] == path[int(ref["path_start"][w]): int(ref["path_end"][w])], (tag, r, w)


@pytest.fixture(scope="module")
def repeat_walks(repeat_case, oracle, ecoli):
    """the repeat fixture through the references: walks on the unitig graph, and on the two contigs of its untangling.  Nothing
    re-threads reads onto contigs in the library (a count table keyed by hash cannot hold two instances of a node), so the paths on
    the contigs are made here: every read comes from S1 or from S2 by construction, and is threaded against the one contig its
    sequence became, where every node has one instance."""
    c, R = repeat_case, tsp.REPEAT
    b = tus._oracle_batch(oracle, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    uni, g = c["uni"], c["g"]
    paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], g["keys"], g["counts"], R["min_count"], tt.places_reference(uni), start=b["start"],
                                end=b["end"], n_unitigs=c["T"])
    nodes = tus.node_sequences_reference([b], g["keys"], R["k"])
    seqs = tus.unitig_sequences_reference(uni, nodes)
    before = {"paths": paths, "ro": c["uro"], "d": c["ud"], "uni": uni, "nodes": nodes, "mo": member_offsets_reference(uni, nodes),
              "strings": tus.unitig_strings(uni, seqs), "overlap": seqs["overlap"]}
    case, r, _, stitched, (s1, s2) = tun.repeat_contigs(c, oracle, ecoli)
    x = r["x"]
    origin = x["node_origin"].astype(np.int64)
    take = {f: np.asarray(nodes[f])[origin] for f in ("rep", "seq_off", "seq_len", "shift_fwd", "shift_rev", "rev")}
    take["pool"] = nodes["pool"]
    strings = tus.unitig_strings(x, stitched)
    place_all = tt.places_reference(x)
    n_from_s1 = len(range(0, len(s1) - R["read"] + 1, R["step"]))
    parts = []
    for which, (lo, hi) in enumerate(((0, n_from_s1), (n_from_s1, len(c["reads"])))):
        src = (s1, s2)[which]
        t = next(i for i, s in enumerate(strings) if s in src or s in tus.revcomp(src))
        place = np.zeros(len(g["keys"]), dtype=pkg.NodePlace)
        inst = np.nonzero(x["node_unitig"] == t)[0]
        place[origin[inst]] = place_all[inst]
        solid = np.zeros(len(g["keys"]), dtype=np.uint32)
        solid[origin[inst]] = g["counts"][origin[inst]]  # a node without an instance on this contig is not solid
        a, e = int(b["km_off"][lo]), int(b["km_off"][hi])
        parts.append(tt.thread_reference(b["km_off"][lo:hi + 1] - b["km_off"][lo], b["hash"][a:e], b["rev"][a:e], g["keys"], solid, R["min_count"], place,
                                         start=b["start"][a:e], end=b["end"][a:e], n_unitigs=x["n_unitigs"] if "n_unitigs" in x else len(strings)))
    cpaths = {f: np.concatenate([p[f] for p in parts]) for f in tsp.PATH + ("start", "end")}
    cpaths["path_off"] = np.concatenate([parts[0]["path_off"], parts[1]["path_off"][1:] + parts[0]["path_off"][-1]]).astype(np.uint64)
    after = {"paths": cpaths, "ro": r["cro"], "d": r["cd"], "uni": x, "nodes": take, "mo": member_offsets_reference(x, take), "strings": strings,
             "overlap": stitched["overlap"], "origin": x["node_origin"]}
    return {"reads": c["reads"], "before": before, "after": after, "crossing": through_r(c, paths)}


def through_r(c, paths):
    """the reads with a step on the one unitig both sequences share"""
    R, _ = tsp.through_repeat(c)
    po, u = paths["path_off"].astype(np.int64), paths["unitig"]
    return [r for r in range(len(po) - 1) if (u[po[r]:po[r + 1]] >> 1 == R).any()]


def test_repeat_fixture_walks_are_substrings_by_the_references(repeat_walks):
    rw = repeat_walks
    for tag in ("before", "after"):
        k = rw[tag]
        ref = reference_of(k)
        check_walk_invariants(ref, k["paths"], tag)
        assert ref["n_off_graph"] == 0 and not ref["flags"].any()
        assert_walks_are_substrings(ref, k["paths"], rw["reads"], k["strings"], k["overlap"], tag)
        if tag == "before":  # error-free reads on the graph they built: one walk per read
            assert np.diff(ref["walk_off"].astype(np.int64)).tolist() == [1] * len(rw["reads"]) and int(ref["n_steps"].max()) == 3
        else:  # every read that crossed R lies on one contig, in one walk of one step
            wo = ref["walk_off"].astype(np.int64)
            assert len(rw["crossing"]) > 10 and all(wo[r + 1] - wo[r] == 1 and ref["n_steps"][wo[r]] == 1 for r in rw["crossing"])
            assert np.diff(wo).tolist() == [1] * len(rw["reads"])
        print("%s untangling: %d walks of %d steps, %d followed" % (tag, ref["n_walks"], len(k["paths"]["unitig"]), ref["n_followed"]))


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = 8
_dev, _host, _ptr = ts._dev, ts._host, ts._ptr
MARK = {np.uint64: -0x5A5A, np.uint32: -0x5A5A}
TDT = {np.uint64: "int64", np.uint32: "int32"}


def _marked(h, frm=0):
    return bool((h[frm:].view(np.int64 if h.dtype.itemsize == 8 else np.int32) == -0x5A5A).all())


def raw_walks(eng, case, capacity=None, want=REC64 + REC32 + ("walk_off", "edge"), null=(), ctx=True, out=True, **over):
    """s2k_paths_walks through ctypes, guard words behind every output -> (status, n_walks, n_followed, n_off_graph, host arrays with
    guards).  over: paths, ro, d, uni_off, circular, members, member_off, out_off, overlap, seq_len replaced; T, n_edges, n_steps, n_reads,
    n_nodes given.  null: names of inputs to pass as NULL"""
    import torch

    paths, uni, mo = over.get("paths", case["paths"]), case["uni"], case["mo"]
    arr = {"ro": (case["ro"], np.uint64), "d": (case["d"], np.uint32), "uni_off": (uni["uni_off"], np.uint64), "circular": (uni["circular"], np.uint8),
           "members": (uni["members"], np.uint32), "member_off": (mo["member_off"], np.uint64), "out_off": (mo["out_off"], np.uint64),
           "overlap": (mo["overlap"], np.uint32), "seq_len": (case["nodes"]["seq_len"], np.uint32)}
    dv = {k: _dev(over.get(k, a), dt) for k, (a, dt) in arr.items()}
    ns = over.get("n_steps", len(paths["unitig"]))
    nr = over.get("n_reads", len(paths["path_off"]) - 1)
    T, ne, nn = over.get("T", len(uni["uni_off"]) - 1), over.get("n_edges", len(case["d"])), over.get("n_nodes", len(uni["members"]))
    dp = {f: _dev(paths[f], np.uint32) for f in tsp.PATH + ("start", "end")}
    dp["path_off"] = _dev(paths["path_off"], np.uint64)
    o = pkg.ThreadOut()
    o.capacity = ns
    for f, t in dp.items():
        if f not in null:
            setattr(o, f, t.data_ptr())
    cap = max(ns, 1) if capacity is None else capacity
    size = {f: cap for f in REC64 + REC32}
    size.update(walk_off=nr + 1, edge=max(ns, 1))
    res = {f: torch.full((size[f] + GUARD,), -0x5A5A, dtype=getattr(torch, TDT[WALK_DT[f]]), device="cuda:0") for f in want}
    w = pkg.WalkOut()
    w.capacity = cap
    for f, t in res.items():
        setattr(w, f, t.data_ptr())
    nw, nf, no = ctypes.c_uint64(777), ctypes.c_uint64(777), ctypes.c_uint64(777)
    torch.cuda.synchronize()
    P = lambda k, empty=False: _ptr(dv[k], k in null or empty)  # noqa: E731
    s = eng.lib.s2k_paths_walks(eng.ctx if ctx else None, nr, None if "paths" in null else ctypes.byref(o), ns, P("ro"), P("d", len(case["d"]) == 0 and "d" not in over),
                                ne, P("uni_off"), P("circular"), T, P("member_off"), P("out_off"), P("overlap"), P("seq_len"), P("members"), nn,
                                ctypes.byref(w) if out else None, ctypes.byref(nw), ctypes.byref(nf), ctypes.byref(no))
    return s, nw.value, nf.value, no.value, {f: _host(t, WALK_DT[f]) for f, t in res.items()}


def device_walks(eng, case, tag):
    """the call against the reference: every array, the totals, the guards; the sizes-only calls; capacity one short -> the reference"""
    ref = reference_of(case)
    check_walk_invariants(ref, case["paths"], tag)
    n, ns, nr = ref["n_walks"], len(case["paths"]["unitig"]), len(case["paths"]["path_off"]) - 1
    tot = (0, n, ref["n_followed"], ref["n_off_graph"])
    s, nw, nf, no, got = raw_walks(eng, case, capacity=n)
    assert (s, nw, nf, no) == tot, (tag, s, nw, nf, no, tot)
    for f in REC64 + REC32:
        assert got[f][:n].tobytes() == ref[f].tobytes(), (tag, f, got[f][:8], ref[f][:8])
        assert _marked(got[f], n), (tag, f, "guard")
    assert got["walk_off"][:nr + 1].tobytes() == ref["walk_off"].tobytes() and _marked(got["walk_off"], nr + 1), (tag, "walk_off")
    assert got["edge"][:ns].tobytes() == ref["edge"].tobytes() and _marked(got["edge"], ns), (tag, "edge")
    for kw in (dict(out=False), dict(want=()), dict(want=("walk_off", "edge"), capacity=0)):  # the sizes: no record array, no capacity
        s, nw, nf, no, got = raw_walks(eng, case, **kw)
        assert (s, nw, nf, no) == tot, (tag, "sizes", kw)
        if kw.get("out", True) and kw["want"]:
            assert got["walk_off"][:nr + 1].tobytes() == ref["walk_off"].tobytes() and got["edge"][:ns].tobytes() == ref["edge"].tobytes(), (tag, "sizes")
        elif not kw.get("out", True):
            assert all(_marked(x) for x in got.values()), (tag, "out NULL")
    if n:  # one short: nothing written, to any array
        s, nw, nf, no, got = raw_walks(eng, case, capacity=n - 1)
        assert (s, nw, nf, no) == (7,) + tot[1:] and all(_marked(x) for x in got.values()), (tag, "capacity")
    s, nw, nf, no, got = raw_walks(eng, case, want=("items", "path_end", "flags"), capacity=n)  # NULL optional outputs
    assert s == 0 and all(got[f][:n].tobytes() == ref[f].tobytes() and _marked(got[f], n) for f in got), (tag, "some outputs")
    return ref


def hand_case():
    uni, ro, d, nodes, mo = walk_hand()
    return {"paths": walk_paths_of(list(W_READS.values())), "ro": ro, "d": d, "uni": uni, "nodes": nodes, "mo": mo}


@pytest.mark.gpu
def test_device_hand_made(eng, tmp_path):
    case = hand_case()
    ref = device_walks(eng, case, "hand")
    assert gaf_text(tmp_path, ref, case["paths"], first_read=5) == W_GAF
    for name, steps in W_READS.items():  # every read alone
        device_walks(eng, dict(case, paths=walk_paths_of([steps])), name)
    device_walks(eng, dict(case, paths=walk_paths_of([])), "no reads")


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 1])
def test_device_random_decompositions(eng, n_steps):
    """reads that walk random decompositions (circular unitigs among them), with gaps and jumps, over a CSR that holds a part of their
    transitions, cut to n_steps steps: round one wave, one tile, and past three tiles"""
    rng = np.random.default_rng(600 + n_steps)
    lens = list(rng.integers(0, 90, size=3 + n_steps // 12)) + [0, 1, 2]
    case = walked_case(rng, max(40, n_steps // 3), lens, n_steps=n_steps)
    ref = device_walks(eng, case, ("walked", n_steps))
    assert len(case["paths"]["unitig"]) == n_steps and (n_steps < 63 or ref["n_followed"] > 0) and (n_steps < 2047 or ref["flags"].any())
    sp = tsp.spans_reference(case["paths"], case["ro"], case["d"], case["uni"]["uni_off"])
    assert (sp["n_followed"], sp["n_off_graph"]) == (ref["n_followed"], ref["n_off_graph"])


@pytest.mark.gpu
def test_device_one_walk_longer_than_two_tiles(eng):
    """a chain of 5 000 one-member unitigs walked by one read, and by one on the twin strand: each walk's head lies two tiles before
    its tail, the prefix differences span tiles"""
    case = long_chain_case(5000)
    ref = device_walks(eng, case, "long chain")
    assert ref["n_steps"].tolist() == [5000, 5000] and ref["first_step"].tolist() == [0, 5000] and ref["items"].tolist() == [5000, 5000]
    assert ref["path_start"].tolist() == [0, 0] and ref["path_end"].tolist() == ref["path_len"].tolist() and int(ref["path_len"].min()) > 5000


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [[2048], [2047], [1, 2049], [2046, 2048, 4096]])
def test_device_tile_and_read_boundaries(eng, cuts):
    """chains of whole unitigs, so that a read is one walk: a read boundary on a tile boundary (a walk ends on a tile's last step, the
    next starts on the first step of the next tile), one step before it, one step after it; then with broken steps"""
    rng = np.random.default_rng(sum(cuts))
    n_steps = 4097
    edges = [0] + cuts + [n_steps]
    lens = [b - a for a, b in zip(edges[:-1], edges[1:])]
    for p_break in (0.0, 0.1):
        case = chained_case(rng, 37, lens, p_break)
        ref = device_walks(eng, case, (cuts, p_break))
        if p_break == 0.0:
            assert ref["n_steps"].tolist() == lens and ref["first_step"].tolist() == edges[:-1]


@pytest.mark.gpu
def test_device_refusals_nothing_written(eng):
    rng = np.random.default_rng(63)
    case = chained_case(rng, 60, list(rng.integers(0, 40, size=200)), p_break=0.1)
    paths, ro, d, uni, mo = case["paths"], case["ro"], case["d"], case["uni"], case["mo"]
    ns, nr, T, ne, nn = len(paths["unitig"]), len(paths["path_off"]) - 1, 60, len(d), len(uni["members"])
    assert ns > 2048 and device_walks(eng, case, "base")["n_walks"] > 100

    def refused(code=1, **kw):
        s, nw, nf, no, got = raw_walks(eng, case, **kw)
        assert (s, nw, nf, no) == (code, 0, 0, 0) and all(_marked(x) for x in got.values()), (s, nw, nf, no, list(kw))

    refused(ctx=False)
    for f in ("paths", "path_off", "ro", "d", "uni_off", "circular", "member_off", "out_off", "overlap", "seq_len", "members", "start", "end") + tsp.PATH:
        refused(null=(f,))

    def changed(name, i, v, src=None):
        x = (src if src is not None else {"ro": ro, "d": d, "uni_off": uni["uni_off"], "members": uni["members"], "member_off": mo["member_off"],
                                           "out_off": mo["out_off"]}[name]).copy()
        x[i] = v
        return {name: x}

    for r, v in ((0, 1), (5, 10 ** 9), (nr, ns - 1), (nr, ns + 1)):  # path_off: not from 0, decreasing, not ending at n_steps
        refused(paths=dict(paths, **changed("path_off", r, v, paths["path_off"])))
    for f, v in (("unitig", 2 * T), ("unitig", 2 ** 32 - 1), ("count", 0), ("count", 4), ("pos", 3)):  # unitigs hold 1 .. 3 members
        refused(paths=dict(paths, **changed(f, ns // 2, v, paths[f])))
    refused(T=T - 1)
    for i, v in ((0, 1), (7, int(ro[8]) + 1), (2 * T, ne - 1), (2 * T, ne + 1)):
        refused(**changed("ro", i, v))
    refused(**changed("d", ne // 2, 2 * T))
    refused(**changed("uni_off", 11, int(uni["uni_off"][10])))  # a unitig without a member
    refused(**changed("uni_off", 0, 1))
    refused(n_nodes=nn - 1)  # uni_off does not end at n_nodes
    refused(**changed("members", 5, 2 * nn))
    t = 20
    a = int(uni["uni_off"][t])
    refused(**changed("member_off", a, int(mo["out_off"][t]) - 1))  # a member offset outside its unitig's bases
    refused(**changed("member_off", a, int(mo["out_off"][t + 1]) + 1))
    refused(**changed("out_off", t, int(mo["out_off"][t + 1]) + 1))  # out_off decreases
    big = mo["out_off"].copy()
    big[t + 1:] += np.uint64(2 ** 32)  # a unitig of 2^32 bases
    refused(out_off=big)
    z = ctypes.c_uint64(5)
    o = pkg.ThreadOut()
    o.path_off = 16
    P = ctypes.c_void_p(16)
    assert eng.lib.s2k_paths_walks(eng.ctx, 1, ctypes.byref(o), 0, P, P, 2 ** 32, P, P, 1, P, P, P, P, P, 1, None, ctypes.byref(z), ctypes.byref(z),
                                   ctypes.byref(z)) == 1 and z.value == 0  # before anything is read
    assert eng.lib.s2k_paths_walks(eng.ctx, 1, ctypes.byref(o), 0, P, None, 0, P, P, 2 ** 31, P, P, P, P, P, 2 ** 31, None, ctypes.byref(z), ctypes.byref(z),
                                   ctypes.byref(z)) == 1
    circ = dict(case, uni=dict(uni, circular=np.ones(T, dtype=np.uint8)))  # on a circular unitig a step may pass the last member
    s, nw, nf, no, got = raw_walks(eng, circ, paths=dict(paths, **changed("count", ns // 2, 9, paths["count"])))
    assert s == 0 and nw > 0


@pytest.mark.gpu
def test_device_deterministic(eng):
    rng = np.random.default_rng(64)
    case = chained_case(rng, 500, list(rng.integers(0, 200, size=300)), p_break=0.1)
    runs = []
    for _ in range(2):
        s, nw, nf, no, got = raw_walks(eng, case)
        assert s == 0 and nw > 1000
        runs.append(b"".join(got[f].tobytes() for f in sorted(got)) + bytes(str((nw, nf, no)), "ascii"))
    assert runs[0] == runs[1]


def _extract_all(eng, reads, l, k, d, mode):
    """tus._extract_mn with start and end kept too: what NodeSequences.build and UnitigGraph.thread both want"""
    import torch

    bases, off = pkg.pack_reads(reads)
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(bases.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
    cap = len(bases) + 1
    t = {f: torch.empty(len(reads) + 1, dtype=torch.int64, device=dev) for f in ("km_off", "mn_off")}
    t["hash"] = torch.empty(cap, dtype=torch.int64, device=dev)
    t["rev"] = torch.empty(cap, dtype=torch.uint8, device=dev)
    for f in ("start", "end", "mn_j", "mn_jend", "mn_hash"):
        t[f] = torch.empty(cap, dtype=torch.int32, device=dev)
    o = pkg.DeviceOut()
    o.km_capacity = o.mn_capacity = cap
    for f, x in t.items():
        setattr(o, f, x.data_ptr())
    torch.cuda.synchronize()
    eng.extract_device(db.data_ptr(), do.data_ptr(), len(reads), len(bases), l, k, d, int(mode), o, flags=pkg.FLAG_WANT_MINIMIZERS)
    t["bases"], t["read_off"] = db, do
    return t


def _read_paths(paths):
    """host path arrays -> pkg.ReadPaths on the GPU"""
    return pkg.ReadPaths(_dev(paths["path_off"], np.uint64)[:len(paths["path_off"])], *(_dev(paths[f], np.uint32)[:len(paths["unitig"])]
                                                                                      for f in ("unitig", "pos", "count")),
                         _dev(np.zeros(len(paths["unitig"])), np.uint32)[:len(paths["unitig"])], *(_dev(paths[f], np.uint32)[:len(paths["unitig"])]
                                                                                                  for f in ("flags", "start", "end")))


def assert_walks(walks, ref, paths, tmp_path, tag):
    """what UnitigGraph.walks returned against walks_reference: every array, the totals, and the GAF file"""
    got = walks.host()
    for f in REC64 + REC32 + ("walk_off", "edge"):
        assert got[f].tobytes() == ref[f].tobytes(), (tag, f)
    assert (walks.n_walks, walks.n_followed, walks.n_off_graph) == (ref["n_walks"], ref["n_followed"], ref["n_off_graph"]), tag
    p = str(tmp_path / ("dev_%s.gaf" % str(tag).replace(" ", "_")))
    lengths = list(range(1000, 1000 + len(ref["walk_off"]) - 1))
    walks.write_gaf(p, None, read_lengths=lengths, first_read=3)
    assert open(p).read() == gaf_text(tmp_path, ref, paths, read_lengths=lengths, first_read=3), (tag, "gaf")


@pytest.mark.gpu
def test_repeat_fixture_end_to_end_before_and_after_untangling(eng, repeat_case, repeat_walks, tmp_path):
    """extract -> graph -> unitigs -> sequences -> thread -> walks on the device; then resolve -> untangle -> walks on the contigs with
    take(node_origin): every array equal to the reference, read[qstart:qend] == path[path_start:path_end] with the device's bytes"""
    c, R, rw = repeat_case, tsp.REPEAT, repeat_walks
    outs = _extract_all(eng, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=R["min_count"], min_edge_count=1)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, [outs])
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, outs, len(c["reads"]), min_count=R["min_count"])
    table.close()
    k = rw["before"]
    ref = reference_of(k)
    walks = ug.walks(eng, paths, ns)
    assert_walks(walks, ref, k["paths"], tmp_path, "before")
    assert ug.member_offsets(eng, ns) is ug.member_offsets(eng, ns)  # kept
    out_off, out = ug.sequences(eng, ns)
    strings = tus.unitig_strings(k["uni"], {"out_off": tg._u64(out_off), "out": out.cpu().numpy()})
    assert_walks_are_substrings(walks.host(), paths.host(), c["reads"], strings, ug.overlap.cpu().numpy().view(np.uint32), "device, before")
    sp_keys, (nf, no) = ug.spans(eng, paths)
    assert (walks.n_followed, walks.n_off_graph) == (nf, no)
    resolved, partner, _ = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    contigs, node_origin, st = ug.untangle(eng, resolved, partner)
    k = rw["after"]
    assert node_origin.cpu().numpy().view(np.uint32).tobytes() == k["origin"].tobytes() and st["contigs"] == 2
    cns = ns.take(node_origin)
    cwalks = contigs.walks(eng, _read_paths(k["paths"]), cns)
    ref = reference_of(k)
    assert_walks(cwalks, ref, k["paths"], tmp_path, "after")
    out_off, out = contigs.sequences(eng, cns)
    strings = tus.unitig_strings(k["uni"], {"out_off": tg._u64(out_off), "out": out.cpu().numpy()})
    assert_walks_are_substrings(cwalks.host(), k["paths"], c["reads"], strings, contigs.overlap.cpu().numpy().view(np.uint32), "device, after")
    wo = cwalks.host()["walk_off"].astype(np.int64)
    assert all(wo[r + 1] - wo[r] == 1 for r in rw["crossing"])


@pytest.mark.gpu
def test_member_offsets_equal_the_stitch_on_ecoli(eng, ecoli):
    """E. coli, Regular 21/3, error-free reads: out_off and overlap are those s2k_unitig_sequences writes, and the stitched bytes at
    every member's offset begin with the member's oriented sequence"""
    reads = tus._flip(tg._sample_reads(ecoli, 150, 5), True)
    outs = _extract_all(eng, reads, 21, 3, 0.05, pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=2, min_edge_count=1)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, [outs])
    out_off, out = ug.sequences(eng, ns)
    member_off, oo, ov, nb = ug.member_offsets(eng, ns)
    assert tg._u64(oo).tobytes() == tg._u64(out_off).tobytes() and ov.cpu().numpy().tobytes() == ug.overlap.cpu().numpy().tobytes()
    assert nb == out.numel() and member_off.numel() == graph.n_nodes > 100
    nodes, text = ns.host(), out.cpu().numpy().tobytes()
    uni = {"uni_off": tg._u64(ug.uni_off), "members": ug.members.cpu().numpy().view(np.uint32), "circular": ug.circular.cpu().numpy()}
    ref = member_offsets_reference(uni, nodes)
    mo = tg._u64(member_off)
    assert mo.tobytes() == ref["member_off"].tobytes() and tg._u64(oo).tobytes() == ref["out_off"].tobytes()
    ends = np.repeat(ref["out_off"][1:], np.diff(uni["uni_off"].astype(np.int64)))
    for x, m in enumerate(uni["members"].tolist()):
        s = tus.oriented(nodes, m)[0]
        n = min(len(s), int(ends[x]) - int(mo[x]))  # a circular unitig's last members reach round
        assert text[int(mo[x]): int(mo[x]) + n] == s[:n], x
    # the raw call with every output NULL gives the size alone; a member >= 2 n_nodes is refused with nothing written
    import torch

    nbv, st = ctypes.c_uint64(0), ns.struct()
    args = (eng.ctx, ctypes.c_void_p(ug.uni_off.data_ptr()), ctypes.c_void_p(ug.members.data_ptr()), ctypes.c_void_p(ug.circular.data_ptr()), ug.n_unitigs,
            graph.n_nodes, ctypes.byref(st))
    torch.cuda.synchronize()
    assert eng.lib.s2k_unitig_member_offsets(*args, None, None, None, ctypes.byref(nbv)) == 0 and nbv.value == nb
    bad = ug.members.clone()
    bad[3] = 2 * graph.n_nodes
    guard = torch.full((graph.n_nodes + GUARD,), -0x5A5A, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    assert eng.lib.s2k_unitig_member_offsets(args[0], args[1], ctypes.c_void_p(bad.data_ptr()), *args[3:], ctypes.c_void_p(guard.data_ptr()), None, None,
                                             ctypes.byref(nbv)) == 1 and nbv.value == 0 and _marked(guard.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("mode,l,k", tsp.MODES)
def test_ecoli_reads_with_errors_through_the_simplified_graph(eng, oracle, ecoli, tmp_path, mode, l, k):
    """the 600 reads with 0.5 % substitutions through simplify(10, 20): device == reference, every array and the GAF file.  No
    substring claim here: the representatives of erroneous reads differ from the reads that cross them"""
    mc = 2
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    b = tus._oracle_batch(oracle, reads, l, k, 0.05, mode)
    outs = _extract_all(eng, reads, l, k, 0.05, mode)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=mc, min_edge_count=1)
    ns = pkg.NodeSequences.build(eng, graph, [outs])
    sg, node_map, _ = graph.simplify(eng, 10, 20)
    final, ref_map, _ = ts.simplify_rounds_reference(tg.graph_reference([b], mc, 1), 10, 20)
    uni, uro, ud, _ = ts.unitig_view(final)
    ref_paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], final["keys"], final["counts"], mc, tt.places_reference(uni), start=b["start"],
                                    end=b["end"], n_unitigs=uni["n_unitigs"])
    all_nodes = tus.node_sequences_reference([b], tg.graph_reference([b], mc, 1)["keys"], k)
    kept = np.nonzero(ref_map >= 0)[0]
    nodes = {f: np.asarray(all_nodes[f])[kept] for f in ("seq_len", "shift_fwd", "shift_rev", "rev")}
    case = {"paths": ref_paths, "ro": uro, "d": ud, "uni": uni, "nodes": nodes, "mo": member_offsets_reference(uni, nodes)}
    ref = reference_of(case)
    ug = sg.unitigs(eng)
    table = pkg.CountTable(eng, sg.keys, sg.counts)
    paths = ug.thread(eng, table, outs, len(reads), min_count=mc)
    table.close()
    walks = ug.walks(eng, paths, ns.subset(node_map))
    assert_walks(walks, ref, ref_paths, tmp_path, ("simplified", int(mode)))
    assert ref["n_followed"] > 100 and int(ref["n_steps"].max()) > 2
    print("simplified %s: %d steps, %d walks, %d followed, %d off-graph, longest walk %d steps" % (
        mode.name, len(ref_paths["unitig"]), ref["n_walks"], ref["n_followed"], ref["n_off_graph"], int(ref["n_steps"].max())))
