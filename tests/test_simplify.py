"""Simplification of the unitig graph on the device: s2k_graph_simplify_mask (tips clipped, simple bubbles popped) and
s2k_graph_induced (the subgraph of the kept nodes), include/s2k.h, DESIGN.md §3.12.  The references are `simplify_reference` and
`induced_reference`, serial restatements of the header's definitions (plain loops over rows, Python integers for the products); the
device's arrays equal theirs exactly, every one of them, in every test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import test_graph as tg
import test_unitigs as tu

pkg = import_package()

SYMS = ("s2k_graph_simplify_mask", "s2k_graph_induced")
M32 = np.uint64(0xFFFFFFFF)
NONE32 = 0xFFFFFFFF


# ---- the references ----------------------------------------------------------------------------------------------------------------
def simplify_reference(row_off, dst, uni_off, cnt, max_tip, max_bubble):
    """-> (remove uint8[T], n_tips, n_bubbles, n_removed) by the definitions of include/s2k.h"""
    ro, d = [int(x) for x in row_off], [int(x) for x in dst]
    off, cnt = [int(x) for x in uni_off], [int(x) for x in cnt]
    T = len(off) - 1
    ln = [off[t + 1] - off[t] for t in range(T)]
    succ = lambda U: d[ro[U]: ro[U + 1]]
    out = lambda U: ro[U + 1] - ro[U]
    inn = lambda U: out(U ^ 1)
    pred = lambda U: [x ^ 1 for x in succ(U ^ 1)]

    def beats(W, U):
        w, u = W >> 1, U >> 1
        a, b = cnt[w] * ln[u], cnt[u] * ln[w]  # Python integers: exact
        if a != b:
            return a > b
        if ln[w] != ln[u]:
            return ln[w] > ln[u]
        return w < u

    def candidate(U):
        return out(U) == 0 and inn(U) >= 1 and ln[U >> 1] <= max_tip

    def tip(U):
        if not candidate(U):
            return False
        for P in pred(U):
            if P >> 1 == U >> 1:
                return False
            if not any(W >> 1 != U >> 1 and (not candidate(W) or beats(W, U)) for W in succ(P)):
                return False
        return True

    def bubble(U):
        if out(U) != 1 or inn(U) != 1 or ln[U >> 1] > max_bubble:
            return False
        P, S = pred(U)[0], succ(U)[0]
        if P >> 1 == U >> 1 or S >> 1 == U >> 1:
            return False
        return any(W >> 1 != U >> 1 and out(W) == 1 and inn(W) == 1 and succ(W) == [S] and beats(W, U) for W in succ(P))

    tips = [tip(2 * t) or tip(2 * t + 1) for t in range(T)]
    bubbles = [bubble(2 * t) or bubble(2 * t + 1) for t in range(T)]
    remove = np.array([a or b for a, b in zip(tips, bubbles)], dtype=np.uint8)
    return remove, sum(tips), sum(bubbles), int(remove.sum())


def induced_reference(keys, counts, edge_keys, edge_counts, keep):
    """-> dict new_id uint32, keys, counts, edge_keys, edge_counts of the subgraph the kept nodes induce"""
    keep = np.asarray(keep).astype(bool)
    new_id = np.full(len(keep), NONE32, dtype=np.uint32)
    new_id[keep] = np.arange(int(keep.sum()), dtype=np.uint32)
    ek, ec, nid = [], [], new_id.tolist()
    for key, c in zip(np.asarray(edge_keys, dtype=np.uint64).tolist(), np.asarray(edge_counts).tolist()):
        u, v = key >> 32, key & 0xFFFFFFFF
        if keep[u >> 1] and keep[v >> 1]:
            ek.append((2 * nid[u >> 1] + (u & 1)) << 32 | (2 * nid[v >> 1] + (v & 1)))
            ec.append(c)
    return {"new_id": new_id, "keys": np.asarray(keys, dtype=np.uint64)[keep], "counts": np.asarray(counts, dtype=np.uint32)[keep],
            "edge_keys": np.array(ek, dtype=np.uint64), "edge_counts": np.array(ec, dtype=np.uint32)}


def unitig_view(g):
    """what KminmerGraph.unitigs gives for a graph dict (keys, counts, edge_keys, edge_counts, row_off, dst), from the references ->
    (unitig_reference result, row_off and dst over the oriented unitigs, the summed count per unitig)"""
    n = len(g["keys"])
    uni = tu.unitig_reference(g["row_off"], g["dst"], n)
    uro, ud = tu.compacted_csr(uni)
    csum = np.concatenate([[0], np.cumsum(g["counts"][uni["members"] >> 1].astype(np.int64))])
    off = uni["uni_off"].astype(np.int64)
    return uni, uro, ud, (csum[off[1:]] - csum[off[:-1]]).astype(np.uint64)


def round_reference(g, max_tip, max_bubble):
    """one round -> dict: uni, uro, ud, ucnt (the unitig graph), remove, tips, bubbles, removed, keep (per node), ind (induced_reference),
    graph (the next graph dict)"""
    uni, uro, ud, ucnt = unitig_view(g)
    remove, nt, nb, nr = simplify_reference(uro, ud, uni["uni_off"], ucnt, max_tip, max_bubble)
    keep = remove[uni["node_unitig"].astype(np.int64)] == 0 if len(g["keys"]) else np.zeros(0, dtype=bool)
    ind = induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], keep)
    ro, d = tg.adjacency_reference(ind["edge_keys"], len(ind["keys"]))
    nxt = {f: ind[f] for f in ("keys", "counts", "edge_keys", "edge_counts")}
    nxt.update(row_off=ro, dst=d)
    return {"uni": uni, "uro": uro, "ud": ud, "ucnt": ucnt, "remove": remove, "tips": nt, "bubbles": nb, "removed": nr, "keep": keep, "ind": ind,
            "graph": nxt}


def simplify_rounds_reference(g, max_tip, max_bubble, max_rounds=16):
    """KminmerGraph.simplify from the references -> (final graph dict, node_map int32, rounds: the round_reference results)"""
    node_map = np.arange(len(g["keys"]), dtype=np.int32)
    rounds = []
    for _ in range(max_rounds):
        r = round_reference(g, max_tip, max_bubble)
        rounds.append(r)
        if r["removed"] == 0:
            break
        alive = node_map >= 0
        node_map[alive] = r["ind"]["new_id"].view(np.int32)[node_map[alive]]
        g = r["graph"]
    return g, node_map, rounds


def dead_ends_created(r):
    """kept oriented unitigs with out >= 1 that lose every successor in the round r"""
    ro, d, rm = [int(x) for x in r["uro"]], [int(x) for x in r["ud"]], r["remove"]
    return sum(1 for P in range(len(ro) - 1) if not rm[P >> 1] and ro[P + 1] > ro[P] and all(rm[W >> 1] for W in d[ro[P]: ro[P + 1]]))


# ---- hand-made unitig graphs ----------------------------------------------------------------------------------------------------------
# name -> (unitigs, edges between oriented unitigs (twins added), members per unitig, count per unitig, max_tip, max_bubble,
#          expected remove mask, tips, bubbles).  Unitig t forward is 2 t.  Trunks hold 20 members: no tip rule reaches them.
_TIP = [(0, 2), (0, 4)]                                            # trunk 0 -> 1 and 2, both dead ends
_BUB2 = [(0, 2), (0, 4), (2, 6), (4, 6)]                           # 0 -> {1, 2} -> 3
_BUB3 = [(0, 2), (0, 4), (0, 6), (2, 8), (4, 8), (6, 8)]           # 0 -> {1, 2, 3} -> 4
_BOTH = [(0, 2), (0, 4), (4, 6), (4, 8), (6, 10), (8, 10)]         # 0 -> {tip 1, 2}; 2 -> {3, 4} -> 5
HAND = {
    "tip beside a longer branch": (3, _TIP, [20, 2, 10], [200, 6, 100], 4, 8, [0, 1, 0], 1, 0),
    "two tips at one junction, nothing else": (3, _TIP, [20, 2, 3], [200, 4, 30], 4, 8, [0, 1, 0], 1, 0),
    "two equal tips: length, then index": (4, [(0, 2), (0, 4), (0, 6)], [20, 2, 4, 4], [200, 20, 40, 40], 4, 8, [0, 1, 0, 1], 2, 0),
    "tip longer than max_tip": (3, _TIP, [20, 5, 10], [200, 15, 100], 4, 8, [0, 0, 0], 0, 0),
    # 0 -> {1, 2} and 3 -> 1: for 3, the tip 1 is the only continuation
    "tip that is one predecessor's only continuation": (4, [(0, 2), (0, 4), (6, 2)], [20, 2, 10, 20], [200, 6, 100, 200], 4, 8, [0, 0, 0, 0], 0, 0),
    # 0+ -> 0- (a hairpin: its own twin) and 0+ -> 1+: 0- is a dead end of 3 members whose predecessor is its own unitig
    "tip attached to its own unitig": (2, [(0, 1), (0, 2)], [3, 10], [9, 100], 4, 8, [0, 0], 0, 0),
    "isolated unitigs": (2, [], [1, 3], [5, 5], 4, 8, [0, 0], 0, 0),
    "two-branch bubble": (4, _BUB2, [20, 2, 2, 20], [200, 20, 4, 200], 4, 8, [0, 0, 1, 0], 0, 1),
    "three-branch bubble": (5, _BUB3, [20, 2, 2, 2, 20], [200, 20, 4, 10, 200], 4, 8, [0, 0, 1, 1, 0], 0, 2),
    "bubble with equal coverage": (5, _BUB3, [20, 2, 4, 4, 20], [200, 20, 40, 40, 200], 4, 8, [0, 1, 0, 1, 0], 0, 2),
    "bubble branch longer than max_bubble": (4, _BUB2, [20, 2, 9, 20], [200, 20, 18, 200], 4, 8, [0, 0, 0, 0], 0, 0),
    "branches that end at different successors": (5, [(0, 2), (0, 4), (2, 6), (4, 8)], [20, 2, 2, 20, 20], [200, 20, 4, 200, 200], 4, 8,
                                                  [0, 0, 0, 0, 0], 0, 0),
    # 0+ -> {1+, 2+} -> 0-: the twins make succ(0+) = {1+, 1-, 2+, 2-}, every branch is read in both directions
    "bubble where P = S ^ 1": (3, [(0, 2), (0, 4), (2, 1), (4, 1)], [20, 2, 2], [200, 4, 20], 4, 8, [0, 1, 0], 0, 1),
    # cnt[2] * len[1] = 2^64 wraps to 0 in 64 bits, below cnt[1] * len[2] = 2^63: the exact comparison removes 1, a wrapped one 2
    "products beyond 64 bits": (4, _BUB2, [20, 4, 2, 20], [200, 1 << 62, 1 << 62, 200], 4, 8, [0, 1, 0, 0], 0, 1),
    "tip and bubble": (6, _BOTH, [20, 2, 20, 2, 2, 20], [200, 6, 200, 20, 4, 200], 4, 8, [0, 1, 0, 0, 1, 0], 1, 1),
    "tip rule off": (6, _BOTH, [20, 2, 20, 2, 2, 20], [200, 6, 200, 20, 4, 200], 0, 8, [0, 0, 0, 0, 1, 0], 0, 1),
    "bubble rule off": (6, _BOTH, [20, 2, 20, 2, 2, 20], [200, 6, 200, 20, 4, 200], 4, 0, [0, 1, 0, 0, 0, 0], 1, 0),
    "both rules off": (6, _BOTH, [20, 2, 20, 2, 2, 20], [200, 6, 200, 20, 4, 200], 0, 0, [0, 0, 0, 0, 0, 0], 0, 0),
}


def hand_case(name):
    T, edges, lens, cnts, mt, mb, want, nt, nb = HAND[name]
    ro, d = tu.csr_of(T, edges)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return T, ro, d, off, np.array(cnts, dtype=np.uint64), mt, mb, np.array(want, dtype=np.uint8), nt, nb


def hand_node_graph(name):
    """a node-level graph for the induced call from a hand-made case: one node per unitig (keys 10 t + 3, count = t + 1), its edges
    with counts 5 .. 15, an edge and its twin the same; keep = the complement of the expected mask"""
    T, ro, d, off, cnt, mt, mb, want, nt, nb = hand_case(name)
    src = np.repeat(np.arange(2 * T, dtype=np.uint64), np.diff(ro.astype(np.int64)))
    ek = (src << np.uint64(32)) | d.astype(np.uint64)
    pair = np.minimum(ek, ((d.astype(np.uint64) ^ np.uint64(1)) << np.uint64(32)) | (src ^ np.uint64(1)))
    return {"keys": np.arange(T, dtype=np.uint64) * np.uint64(10) + np.uint64(3), "counts": np.arange(1, T + 1, dtype=np.uint32), "edge_keys": ek,
            "edge_counts": (pair % np.uint64(11) + np.uint64(5)).astype(np.uint32), "row_off": ro, "dst": d}, want == 0


def random_graph_with_errors(rng, n, extra, n_tips, n_bubbles):
    """the generator idea of tests/test_unitigs.py (random oriented paths and cycles over n nodes, `extra` random edges, closed under
    twins) with short side paths and short parallel paths on top, as sequencing errors leave them -> a graph dict with counts (the
    first n nodes 20..40, the added ones 2..6, so both rules fire) and edge counts"""
    perm = rng.permutation(n)
    a = (2 * perm + rng.integers(0, 2, size=n)).tolist()
    edges, paths, i = [], [], 0
    while i < n:
        L = int(rng.integers(1, max(2, n // 3) + 1))
        seg = a[i: i + L]
        edges += list(zip(seg[:-1], seg[1:]))
        paths.append(seg)
        if len(seg) > 1 and rng.random() < 0.2:
            edges.append((seg[-1], seg[0]))
        i += L
    nxt = n  # new nodes
    for _ in range(n_tips):  # a chain of 1-3 new nodes that leaves (or enters) a random node
        u = a[int(rng.integers(0, n))] ^ int(rng.integers(0, 2))
        chain = [2 * (nxt + j) + int(rng.integers(0, 2)) for j in range(int(rng.integers(1, 4)))]
        nxt += len(chain)
        edges += list(zip([u] + chain[:-1], chain))
    for _ in range(n_bubbles):  # a chain of 1-3 new nodes beside 1-3 nodes of a path
        seg = paths[int(rng.integers(0, len(paths)))]
        if len(seg) < 3:
            continue
        i = int(rng.integers(0, len(seg) - 2))
        j = min(len(seg) - 1, i + int(rng.integers(2, 5)))
        chain = [2 * (nxt + x) + int(rng.integers(0, 2)) for x in range(int(rng.integers(1, 4)))]
        nxt += len(chain)
        edges += list(zip([seg[i]] + chain, chain + [seg[j]]))
    if extra:
        edges += [tuple(r) for r in rng.integers(0, 2 * nxt, size=(extra, 2)).tolist()]
    ro, d = tu.csr_of(nxt, edges)
    src = np.repeat(np.arange(2 * nxt, dtype=np.uint64), np.diff(ro.astype(np.int64)))
    ek = (src << np.uint64(32)) | d.astype(np.uint64)
    counts = np.concatenate([rng.integers(20, 41, size=n), rng.integers(2, 7, size=nxt - n)]).astype(np.uint32)
    pair = np.minimum(ek, ((d.astype(np.uint64) ^ np.uint64(1)) << np.uint64(32)) | (src ^ np.uint64(1)))  # an edge and its twin: one count
    ec = (pair % np.uint64(7) + np.uint64(1)).astype(np.uint32)
    keys = np.cumsum(rng.integers(1, 1000, size=nxt)).astype(np.uint64)
    return {"keys": keys, "counts": counts, "edge_keys": ek, "edge_counts": ec, "row_off": ro, "dst": d}


_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def sample_reads_with_errors(ecoli, n, seed, rate, lo=2000, hi=4000):
    """n reads of lo..hi bases from random places of the genome, each base substituted with probability `rate`, half of the reads
    reverse-complemented"""
    rng = np.random.default_rng(seed)
    code = np.zeros(256, dtype=np.int64)
    code[list(b"ACGT")] = range(4)
    out = []
    for _ in range(n):
        L = int(rng.integers(lo, hi))
        a = int(rng.integers(0, len(ecoli) - L))
        r = np.frombuffer(ecoli[a:a + L], dtype=np.uint8).copy()
        for i in np.nonzero(rng.random(L) < rate)[0]:
            r[i] = _ACGT[(code[r[i]] + int(rng.integers(1, 4))) % 4]
        out.append(tg._revcomp(r.tobytes()) if rng.random() < 0.5 else r.tobytes())
    return out


# Regular l=12 k=5 d=0.05, 600 reads with 0.5 % substitutions, min_count 2; tips of at most 2 k members, bubble branches of at most 4 k
ECOLI = dict(l=12, k=5, d=0.05, n=600, seed=7, rate=0.005, min_count=2, max_tip=10, max_bubble=20)


def ecoli_error_graph(oracle, ecoli, rate=None):
    c = ECOLI
    reads = sample_reads_with_errors(ecoli, c["n"], c["seed"], c["rate"] if rate is None else rate)
    b = oracle.batch(*pkg.pack_reads(reads), c["l"], c["k"], c["d"], int(pkg.HashMode.Regular))
    return reads, tg.graph_reference([b], c["min_count"])


def is_graph_sound(g):
    ek = g["edge_keys"]
    n = len(g["keys"])
    assert (g["keys"][1:] > g["keys"][:-1]).all() and (ek[1:] > ek[:-1]).all()  # strictly ascending, both
    assert len(ek) == 0 or (int((ek >> np.uint64(32)).max()) < 2 * n and int((ek & M32).max()) < 2 * n)
    tw = ((ek & M32) ^ np.uint64(1)) << np.uint64(32) | ((ek >> np.uint64(32)) ^ np.uint64(1))
    i = np.searchsorted(ek, tw)
    assert len(ek) == 0 or ((i < len(ek)).all() and (ek[np.minimum(i, len(ek) - 1)] == tw).all())  # every twin is there ...
    assert (g["edge_counts"][np.minimum(i, max(len(ek) - 1, 0))] == g["edge_counts"]).all()  # ... with the same count


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert hasattr(pkg.Engine, "graph_simplify_mask") and hasattr(pkg.Engine, "graph_induced")
    assert hasattr(pkg.KminmerGraph, "simplify") and hasattr(pkg.NodeSequences, "subset")


def test_cpp_simplify_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "simplify_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "simplify_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.parametrize("name", list(HAND))
def test_reference_hand_made(name):
    T, ro, d, off, cnt, mt, mb, want, nt, nb = hand_case(name)
    assert tu.is_twin_symmetric(ro, d, T)
    remove, tips, bubbles, removed = simplify_reference(ro, d, off, cnt, mt, mb)
    assert remove.tolist() == want.tolist() and (tips, bubbles, removed) == (nt, nb, int(want.sum())), (name, remove, tips, bubbles)
    g, keep = hand_node_graph(name)
    ind = induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], keep)
    g2 = dict(ind)
    is_graph_sound(g2)
    assert len(ind["keys"]) == int(keep.sum()) and (ind["new_id"][keep] == np.arange(int(keep.sum()))).all() and (ind["new_id"][~keep] == NONE32).all()


def test_reference_induced_hand_made_keys():
    """the two-branch bubble with unitig 2 removed: node 3 becomes node 2, the four edges through node 2 go"""
    g, keep = hand_node_graph("two-branch bubble")
    assert keep.tolist() == [True, True, False, True]
    ind = induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], keep)
    k = lambda u, v: u << 32 | v
    # CSR of the case: (0,2) (0,4) (2,6) (3,1) (4,6) (5,1) (7,3) (7,5): kept (0,2) (2,6)->(2,4) (3,1) (7,3)->(5,3)
    assert ind["edge_keys"].tolist() == [k(0, 2), k(2, 4), k(3, 1), k(5, 3)] and ind["edge_counts"].tolist() == g["edge_counts"][[0, 2, 3, 6]].tolist()
    assert ind["new_id"].tolist() == [0, 1, NONE32, 2] and ind["keys"].tolist() == [3, 13, 33] and ind["counts"].tolist() == [1, 2, 4]


def test_reference_random_graphs_invariants():
    """random graphs with side paths and parallel paths: both rules fire; a round creates no dead end; the induced graph is
    twin-symmetric and strictly ascending; with nothing removed it is the identity; iterating reaches a fixed point"""
    rng = np.random.default_rng(31)
    seen_tips = seen_bubbles = 0
    for n, extra, nt, nb in ((8, 0, 2, 1), (40, 2, 6, 4), (200, 0, 20, 20), (200, 20, 30, 10), (600, 10, 60, 60)):
        for _ in range(4):
            g = random_graph_with_errors(rng, n, extra, nt, nb)
            is_graph_sound(g)
            same = induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], np.ones(len(g["keys"]), dtype=bool))
            assert (same["new_id"] == np.arange(len(g["keys"]))).all()
            for f in ("keys", "counts", "edge_keys", "edge_counts"):
                assert same[f].tobytes() == g[f].tobytes(), f
            final, node_map, rounds = simplify_rounds_reference(g, 4, 8, max_rounds=len(g["keys"]) + 1)
            assert rounds[-1]["removed"] == 0  # a fixed point: every earlier round removed a unitig, and there are finitely many
            for r in rounds:
                assert dead_ends_created(r) == 0
                is_graph_sound(r["graph"])
                assert tu.is_twin_symmetric(r["graph"]["row_off"], r["graph"]["dst"], len(r["graph"]["keys"]))
            seen_tips += sum(r["tips"] for r in rounds)
            seen_bubbles += sum(r["bubbles"] for r in rounds)
            kept = node_map >= 0
            assert int(kept.sum()) == len(final["keys"]) and (final["keys"] == g["keys"][kept]).all()
            assert (node_map[kept] == np.arange(int(kept.sum()))).all()
    assert seen_tips > 50 and seen_bubbles > 50, (seen_tips, seen_bubbles)


def test_oracle_ecoli_reads_with_errors_simplify(oracle, ecoli):
    """the committed E. coli fixture, reads with substitutions, graph by the numpy references, then rounds of the serial reference:
    round 0 removes tips and bubbles, a fixed point comes within 12 rounds, fewer and longer unitigs"""
    c = ECOLI
    _, g = ecoli_error_graph(oracle, ecoli)
    final, node_map, rounds = simplify_rounds_reference(g, c["max_tip"], c["max_bubble"], max_rounds=12)
    for i, r in enumerate(rounds):
        lens = np.diff(r["uni"]["uni_off"].astype(np.int64))
        print("round %d: nodes %d unitigs %d longest %d tips %d bubbles %d removed %d dead ends created %d"
              % (i, len(r["keep"]), r["uni"]["n_unitigs"], lens.max(), r["tips"], r["bubbles"], r["removed"], dead_ends_created(r)))
        assert dead_ends_created(r) == 0
    assert rounds[0]["tips"] >= 1 and rounds[0]["bubbles"] >= 1
    assert rounds[-1]["removed"] == 0 and len(rounds) <= 12
    first, last = rounds[0]["uni"], rounds[-1]["uni"]
    assert last["n_unitigs"] < first["n_unitigs"]
    assert np.diff(last["uni_off"].astype(np.int64)).max() > np.diff(first["uni_off"].astype(np.int64)).max()


def _oracle_batch_mn(oracle, reads):
    import test_unitig_sequences as tus

    c = ECOLI
    return tus, tus._oracle_batch(oracle, reads, c["l"], c["k"], c["d"], pkg.HashMode.Regular)


def subset_records(nodes, node_map):
    """NodeSequences.subset on the host records of test_unitig_sequences.node_sequences_reference"""
    kept = np.asarray(node_map) >= 0
    out = {f: np.asarray(nodes[f])[kept] for f in ("rep", "seq_off", "seq_len", "shift_fwd", "shift_rev", "rev")}
    out["pool"] = nodes["pool"]
    return out


def simplified_sequences_reference(oracle, reads):
    """reads -> graph, rounds of the reference, the subset of the node records, the numpy stitch of the final unitigs"""
    c = ECOLI
    tus, b = _oracle_batch_mn(oracle, reads)
    g = tg.graph_reference([b], c["min_count"])
    final, node_map, rounds = simplify_rounds_reference(g, c["max_tip"], c["max_bubble"])
    nodes = tus.node_sequences_reference([b], g["keys"], c["k"])
    sub = subset_records(nodes, node_map)
    uni = tu.unitig_reference(final["row_off"], final["dst"], len(final["keys"]))
    return tus, b, g, final, node_map, rounds, nodes, sub, uni, tus.unitig_sequences_reference(uni, sub)


def test_error_free_reads_simplified_unitigs_are_slices_of_the_genome(oracle, ecoli):
    """Regular 12/5/0.05 has no node with two readings: with error-free reads every unitig of the simplified graph,
    stitched by the numpy reference from the subset records, is a slice of the genome or of its reverse complement"""
    reads = sample_reads_with_errors(ecoli, ECOLI["n"], ECOLI["seed"], 0.0)
    tus, b, g, final, node_map, rounds, nodes, sub, uni, seqs = simplified_sequences_reference(oracle, reads)
    strings = tus.unitig_strings(uni, seqs)
    rc = tus.revcomp(ecoli)
    missing = [t for t, s in enumerate(strings) if s not in ecoli and s not in rc]
    print("error-free: nodes %d -> %d, unitigs %d -> %d in %d rounds (%s); not a slice: %d"
          % (len(g["keys"]), len(final["keys"]), rounds[0]["uni"]["n_unitigs"], uni["n_unitigs"], len(rounds),
             [(r["tips"], r["bubbles"]) for r in rounds], len(missing)))
    assert missing == []


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = 8
_TDT = {np.uint64: "int64", np.uint32: "int32", np.uint8: "uint8"}
_VIEW = {np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}
_MARK = {np.uint64: -0x5A5A, np.uint32: -0x5A5A, np.uint8: 0xA5}


def _dev(x, dt):
    """host array -> GPU tensor holding the same bits (never empty: a NULL-free pointer for n == 0)"""
    import torch

    x = np.ascontiguousarray(np.asarray(x, dtype=dt))
    if len(x) == 0:
        return torch.zeros(1, dtype=getattr(torch, _TDT[dt]), device="cuda:0")
    return torch.from_numpy(x.view(_VIEW[dt]).copy()).to("cuda:0")


def _out(n, dt):
    import torch

    return torch.full((n + GUARD,), _MARK[dt], dtype=getattr(torch, _TDT[dt]), device="cuda:0")


def _host(t, dt):
    return t.cpu().numpy().view(dt)


def _marked(h, dt, frm=0):
    return (h[frm:] == np.array(_MARK[dt]).astype(_VIEW[dt]).view(dt)).all()


def _ptr(t, null=False):
    return None if null else ctypes.c_void_p(t.data_ptr())


def raw_mask(eng, ro, d, off, cnt, mt, mb, n_edges=None, T=None, want_remove=True, null=(), ctx=True):
    """s2k_graph_simplify_mask through ctypes, guard bytes behind d_remove -> (status, tips, bubbles, removed, host remove with guards)"""
    import torch

    T = len(off) - 1 if T is None else T
    dro, dd, doff, dcnt = _dev(ro, np.uint64), _dev(d, np.uint32), _dev(off, np.uint64), _dev(cnt, np.uint64)
    rem = _out(T, np.uint8)
    a, b, c = ctypes.c_uint64(777), ctypes.c_uint64(777), ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_graph_simplify_mask(eng.ctx if ctx else None, _ptr(dro, "row_off" in null), _ptr(dd, "dst" in null or len(d) == 0),
                                        len(d) if n_edges is None else n_edges, T, _ptr(doff, "uni_off" in null), _ptr(dcnt, "cnt" in null), mt, mb,
                                        _ptr(rem, not want_remove), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return s, a.value, b.value, c.value, _host(rem, np.uint8)


def device_mask(eng, ro, d, off, cnt, mt, mb, want, tag):
    """the call against `want` = (remove, tips, bubbles, removed), guard untouched; and the totals-only call"""
    s, a, b, c, rem = raw_mask(eng, ro, d, off, cnt, mt, mb)
    T = len(off) - 1
    assert (s, a, b, c) == (0,) + tuple(want[1:]), (tag, s, a, b, c, want[1:])
    assert rem[:T].tobytes() == want[0].tobytes(), (tag, rem[:T], want[0])
    assert _marked(rem, np.uint8, T), (tag, "guard")
    s, a, b, c, rem = raw_mask(eng, ro, d, off, cnt, mt, mb, want_remove=False)
    assert (s, a, b, c) == (0,) + tuple(want[1:]) and _marked(rem, np.uint8), (tag, "totals only")


IND = (("new_id", np.uint32), ("keys", np.uint64), ("counts", np.uint32), ("edge_keys", np.uint64), ("edge_counts", np.uint32))


def raw_induced(eng, g, keep=None, node_unitig=None, remove=None, node_cap=None, edge_cap=None, null=(), n_nodes=None, n_edges=None, front=0):
    """s2k_graph_induced through ctypes, guard words behind every output -> (status, n_nodes_out, n_edges_out, host outputs with
    guards).  front: elements the key / count outputs start behind their (16-byte aligned) allocation, to move their alignment."""
    import torch

    n = len(g["keys"]) if n_nodes is None else n_nodes
    ne = len(g["edge_keys"]) if n_edges is None else n_edges
    dk, dc, dek, dec = _dev(g["keys"], np.uint64), _dev(g["counts"], np.uint32), _dev(g["edge_keys"], np.uint64), _dev(g["edge_counts"], np.uint32)
    dkeep = None if keep is None else _dev(np.asarray(keep).astype(np.uint8), np.uint8)
    dnu = None if node_unitig is None else _dev(node_unitig, np.uint32)
    drm = None if remove is None else _dev(remove, np.uint8)
    ncap, ecap = n if node_cap is None else node_cap, ne if edge_cap is None else edge_cap
    size = {"new_id": n, "keys": ncap + front, "counts": ncap + front, "edge_keys": ecap + front, "edge_counts": ecap + front}
    bufs = {f: _out(size[f], dt) for f, dt in IND}
    o = {f: None if f in null else ctypes.c_void_p(bufs[f].data_ptr() + (front * bufs[f].element_size() if f != "new_id" else 0)) for f, _ in IND}
    a, b = ctypes.c_uint64(777), ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_graph_induced(eng.ctx, _ptr(dk, "in_keys" in null), _ptr(dc, "in_counts" in null), n, _ptr(dek, "in_edge_keys" in null or ne == 0),
                                  _ptr(dec, "in_edge_counts" in null), ne, None if dkeep is None else _ptr(dkeep), None if dnu is None else _ptr(dnu),
                                  None if drm is None else _ptr(drm), 0 if remove is None else len(remove), o["new_id"], o["keys"], o["counts"], ncap,
                                  o["edge_keys"], o["edge_counts"], ecap, ctypes.byref(a), ctypes.byref(b))
    return s, a.value, b.value, {f: _host(bufs[f], dt) for f, dt in IND}


def _all_marked(host):
    return all(_marked(host[f], dt) for f, dt in IND)


def device_induced(eng, g, keep, want, tag, front=0, **kw):
    s, a, b, host = raw_induced(eng, g, keep=keep, front=front, **kw)
    assert (s, a, b) == (0, len(want["keys"]), len(want["edge_keys"])), (tag, s, a, b)
    for f, dt in IND:
        lo = 0 if f == "new_id" else front
        assert host[f][lo: lo + len(want[f])].tobytes() == want[f].tobytes(), (tag, f)
        assert _marked(host[f], dt, lo + len(want[f])) and _marked(host[f][:lo], dt), (tag, f, "guard")
    return host


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_device_hand_made(eng, name):
    T, ro, d, off, cnt, mt, mb, want, nt, nb = hand_case(name)
    device_mask(eng, ro, d, off, cnt, mt, mb, (want, nt, nb, int(want.sum())), name)
    g, keep = hand_node_graph(name)
    ind = induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], keep)
    device_induced(eng, g, keep, ind, name)
    # the same through the unitig mask: one node per unitig, so node_unitig is the identity
    s, a, b, host = raw_induced(eng, g, node_unitig=np.arange(T, dtype=np.uint32), remove=want)
    assert (s, a, b) == (0, len(ind["keys"]), len(ind["edge_keys"]))
    for f, dt in IND:
        assert host[f][:len(ind[f])].tobytes() == ind[f].tobytes() and _marked(host[f], dt, len(ind[f])), (name, f)


@pytest.mark.gpu
def test_device_random_graphs_every_round(eng):
    """random graphs with side and parallel paths, sizes around a wave, a block and a compaction tile (2048): every round of the
    reference's iteration -- mask, totals, new_id, the four arrays of the induced graph -- on the device, both sources of the node mask,
    and every alignment of the output runs"""
    rng = np.random.default_rng(32)
    done = rounds_run = 0
    for n, extra, nt, nb in ((1, 0, 0, 0), (3, 0, 1, 0), (20, 0, 3, 2), (31, 2, 4, 4), (60, 0, 6, 6), (128, 4, 10, 10), (500, 0, 50, 50),
                             (1000, 10, 100, 60), (2040, 0, 3, 3), (2047, 0, 1, 0), (4000, 20, 300, 300), (30000, 50, 2000, 2000)):
        for rep in range(3 if n <= 5000 else 1):
            g = random_graph_with_errors(rng, n, extra, nt, nb)
            final, node_map, rounds = simplify_rounds_reference(g, 4, 8, max_rounds=6)
            for i, r in enumerate(rounds):
                tag = ("random", n, rep, i)
                device_mask(eng, r["uro"], r["ud"], r["uni"]["uni_off"], r["ucnt"], 4, 8, (r["remove"], r["tips"], r["bubbles"], r["removed"]), tag)
                device_induced(eng, g, r["keep"], r["ind"], tag, front=(done + i) % 4)
                s, a, b, host = raw_induced(eng, g, node_unitig=r["uni"]["node_unitig"], remove=r["remove"])
                assert (s, a, b) == (0, len(r["ind"]["keys"]), len(r["ind"]["edge_keys"])), tag
                for f, dt in IND:
                    assert host[f][:len(r["ind"][f])].tobytes() == r["ind"][f].tobytes() and _marked(host[f], dt, len(r["ind"][f])), (tag, f)
                g = r["graph"]
                rounds_run += 1
            done += 1
    assert done >= 30 and rounds_run > done


@pytest.mark.gpu
def test_device_edge_shapes(eng):
    """the empty graph, a graph without edges, everything kept (the identity), everything removable, nothing kept"""
    z64, z32 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    s, a, b, c, rem = raw_mask(eng, np.zeros(1, dtype=np.uint64), z32, np.zeros(1, dtype=np.uint64), z64, 4, 8)
    assert (s, a, b, c) == (0, 0, 0, 0) and _marked(rem, np.uint8)
    empty = {"keys": z64, "counts": z32, "edge_keys": z64, "edge_counts": z32}
    s, a, b, host = raw_induced(eng, empty, keep=np.zeros(0, dtype=np.uint8))
    assert (s, a, b) == (0, 0, 0) and _all_marked(host)
    # no edges: 5 isolated unitigs, nothing to remove; the induced call with a mask keeps 3 of the 5 nodes
    ro, off, cnt = np.zeros(11, dtype=np.uint64), np.arange(6, dtype=np.uint64), np.full(5, 9, dtype=np.uint64)
    device_mask(eng, ro, z32, off, cnt, 4, 8, (np.zeros(5, dtype=np.uint8), 0, 0, 0), "no edges")
    g = {"keys": np.arange(5, dtype=np.uint64) + np.uint64(7), "counts": np.arange(5, dtype=np.uint32), "edge_keys": z64, "edge_counts": z32}
    keep = np.array([1, 0, 1, 1, 0], dtype=bool)
    device_induced(eng, g, keep, induced_reference(g["keys"], g["counts"], z64, z32, keep), "no edges")
    rng = np.random.default_rng(33)
    g = random_graph_with_errors(rng, 3000, 10, 200, 200)
    n = len(g["keys"])
    ident = device_induced(eng, g, np.ones(n, dtype=bool), induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], np.ones(n, dtype=bool)),
                           "identity")
    assert ident["new_id"][:n].tolist() == list(range(n)) and ident["edge_keys"][:len(g["edge_keys"])].tobytes() == g["edge_keys"].tobytes()
    none = np.zeros(n, dtype=bool)
    device_induced(eng, g, none, induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], none), "nothing kept")
    # everything removable: a star of tips around a hub that is itself short -- every unitig but the best of each junction goes
    T = 300
    edges = [(0, 2 * t) for t in range(1, T)]
    ro, d = tu.csr_of(T, edges)
    off, cnt = np.arange(T + 1, dtype=np.uint64), np.arange(T, 0, -1).astype(np.uint64)
    want = simplify_reference(ro, d, off, cnt, 4, 8)
    assert want[3] == T - 2  # the hub and the tip with the highest count stay
    device_mask(eng, ro, d, off, cnt, 4, 8, want, "star")


@pytest.mark.gpu
def test_device_refusals_capacity_and_sizes(eng):
    rng = np.random.default_rng(34)
    g = random_graph_with_errors(rng, 1500, 10, 120, 120)
    r = round_reference(g, 4, 8)
    assert r["tips"] > 10 and r["bubbles"] > 10
    ro, d, off, cnt = r["uro"], r["ud"], r["uni"]["uni_off"], r["ucnt"]
    T = len(off) - 1

    def refused(ro_=ro, d_=d, off_=off, code=1, **kw):
        s, a, b, c, rem = raw_mask(eng, ro_, d_, off_, cnt, 4, 8, **kw)
        assert s == code and (a, b, c) == (0, 0, 0) and _marked(rem, np.uint8), (s, kw)

    ros = [int(x) for x in ro]
    u = next(x for x in range(2 * T) if ros[x + 1] - ros[x] >= 2)
    x = d.copy()  # an id >= 2 T
    x[ros[u]] = 2 * T
    refused(d_=x)
    refused(n_edges=len(d) + 1)  # row_off[2 T] != n_edges
    refused(n_edges=len(d) - 1)
    y = ro.copy()  # row_off not starting at 0; decreasing
    y[0] = 1
    refused(ro_=y)
    y = ro.copy()
    y[u + 1] = y[u] - np.uint64(1) if y[u] > 0 else y[u + 2] + np.uint64(1)
    refused(ro_=y)
    y = off.copy()  # a unitig without a member; uni_off decreasing
    y[5] = y[4]
    refused(off_=y)
    y = off.copy()
    y[5] = y[4] - np.uint64(1) if y[4] > 0 else y[6] + np.uint64(1)
    refused(off_=y)
    refused(ctx=False)
    refused(null=("row_off",))
    refused(null=("dst",))
    refused(null=("uni_off",))
    refused(null=("cnt",))
    z = ctypes.c_uint64(5)
    assert eng.lib.s2k_graph_simplify_mask(eng.ctx, ctypes.c_void_p(8), None, 0, 2 ** 31, ctypes.c_void_p(8), ctypes.c_void_p(8), 4, 8, None,
                                           ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == 1  # before anything is read
    assert eng.lib.s2k_graph_simplify_mask(eng.ctx, None, None, 3, 0, None, None, 4, 8, None, ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == 1
    assert eng.lib.s2k_graph_simplify_mask(eng.ctx, None, None, 0, 1, None, None, 4, 8, None, None, ctypes.byref(z), ctypes.byref(z)) == 1
    # the induced call
    ind, keep = r["ind"], r["keep"]
    nn, ne = len(ind["keys"]), len(ind["edge_keys"])
    assert 0 < nn < len(g["keys"]) and 0 < ne < len(g["edge_keys"])
    s, a, b, host = raw_induced(eng, g, keep=keep, null=tuple(f for f, _ in IND))  # sizes only
    assert (s, a, b) == (0, nn, ne) and _all_marked(host)
    for kw in (dict(node_cap=nn - 1), dict(edge_cap=ne - 1), dict(node_cap=0, edge_cap=0)):  # one short: S2K_ERR_CAPACITY, the sizes still set
        s, a, b, host = raw_induced(eng, g, keep=keep, **kw)
        assert (s, a, b) == (7, nn, ne) and _all_marked(host), kw
    device_induced(eng, g, keep, ind, "exactly enough", node_cap=nn, edge_cap=ne)
    s, a, b, host = raw_induced(eng, g, keep=keep, null=("new_id", "counts", "edge_counts"))  # some arrays: new_id lives in the workspace
    assert (s, a, b) == (0, nn, ne) and _marked(host["new_id"], np.uint32) and _marked(host["counts"], np.uint32) and _marked(host["edge_counts"], np.uint32)
    assert host["keys"][:nn].tobytes() == ind["keys"].tobytes() and host["edge_keys"][:ne].tobytes() == ind["edge_keys"].tobytes()
    s, a, b, host = raw_induced(eng, g, keep=keep, null=("keys", "counts", "edge_keys", "edge_counts"))  # new_id alone
    assert (s, a, b) == (0, nn, ne) and host["new_id"][:len(keep)].tobytes() == ind["new_id"].tobytes() and _marked(host["keys"], np.uint64)

    def refused_ind(code=1, sizes=(0, 0), **kw):
        s, a, b, host = raw_induced(eng, **kw)
        assert s == code and (a, b) == sizes and _all_marked(host), (s, a, b, kw)

    x = dict(g)  # an edge that names a node >= n_nodes
    x["edge_keys"] = g["edge_keys"].copy()
    x["edge_keys"][-1] = np.uint64((2 * len(g["keys"])) << 32 | 1)
    refused_ind(g=x, keep=keep)
    x["edge_keys"] = g["edge_keys"].copy()
    x["edge_keys"][3] = (g["edge_keys"][3] & ~M32) | np.uint64(2 * len(g["keys"]) + 1)
    refused_ind(g=x, keep=keep)
    nu = r["uni"]["node_unitig"].copy()  # a node_unitig entry >= n_unitigs
    nu[7] = T
    refused_ind(g=g, node_unitig=nu, remove=r["remove"])
    refused_ind(g=g)  # no source for the mask
    refused_ind(g=g, node_unitig=nu)  # node_unitig without remove
    refused_ind(g=g, keep=keep, null=("in_keys",))  # an output without its input
    refused_ind(g=g, keep=keep, null=("in_counts",))
    refused_ind(g=g, keep=keep, null=("in_edge_counts",))
    refused_ind(g=g, keep=keep, null=("in_edge_keys",))
    refused_ind(g=g, keep=keep[:0], n_nodes=0)  # edges without nodes
    assert eng.lib.s2k_graph_induced(None, *([None] * 2), 0, *([None] * 2), 0, *([None] * 3), 0, *([None] * 3), 0, *([None] * 2), 0, ctypes.byref(z),
                                     ctypes.byref(z)) == 1 and z.value == 0
    assert eng.lib.s2k_graph_induced(eng.ctx, ctypes.c_void_p(8), None, 2 ** 31, None, None, 0, ctypes.c_void_p(8), None, None, 0, None, None, None, 0,
                                     None, None, 0, ctypes.byref(z), ctypes.byref(z)) == 1  # n >= 2^31, before anything is read


_kg_host = tg._graph_host


def _same_graph(got, want, tag):
    for f in ("keys", "counts", "edge_keys", "edge_counts", "row_off", "dst"):
        assert got[f].tobytes() == np.asarray(want[f], dtype=got[f].dtype).tobytes(), (tag, f)


@pytest.fixture(scope="module")
def ecoli_device(eng, oracle, ecoli):
    """the E. coli error set on the device and its reference rounds"""
    import test_unitig_sequences as tus

    c = ECOLI
    reads = sample_reads_with_errors(ecoli, c["n"], c["seed"], c["rate"])
    outs = [tus._extract_mn(eng, reads, c["l"], c["k"], c["d"], pkg.HashMode.Regular)]
    graph = pkg.KminmerGraph.build(eng, outs, min_count=c["min_count"])
    ref = simplified_sequences_reference(oracle, reads)
    return reads, outs, graph, ref


@pytest.mark.gpu
def test_kminmer_graph_simplify_ecoli_every_round(eng, ecoli_device):
    """KminmerGraph.simplify on the E. coli reads with substitutions: the graph equals the reference graph; every round's mask, totals,
    new_id and induced arrays equal the reference's (the rounds replayed through the Engine calls); simplify() returns the reference's
    final graph, node_map and per-round figures; the final graph passes s2k_graph_unitigs' validation and a second simplify removes
    nothing"""
    c = ECOLI
    reads, outs, graph, (tus, b, g, final, node_map, rounds, nodes, sub, uni, seqs) = ecoli_device
    _same_graph(_kg_host(graph), g, "build")
    cur = graph
    for i, r in enumerate(rounds):
        ug = cur.unitigs(eng)
        tu.same(tu._unitig_graph_host(ug), {"uni_off": r["uni"]["uni_off"], "node_unitig": r["uni"]["node_unitig"], "counts": r["ucnt"].astype(np.int64),
                                            "row_off": r["uro"], "dst": r["ud"]}, ("unitigs", i))
        m = eng.graph_simplify_mask(ug, c["max_tip"], c["max_bubble"])
        assert m["remove"].cpu().numpy().tobytes() == r["remove"].tobytes(), i
        assert (m["n_tips"], m["n_bubbles"], m["n_removed"]) == (r["tips"], r["bubbles"], r["removed"]), i
        ind = eng.graph_induced(cur, node_unitig=ug.node_unitig, remove=m["remove"])
        for f, dt in IND:
            assert ind[f].cpu().numpy().view(dt).tobytes() == r["ind"][f].tobytes(), (i, f)
        byte_mask = eng.graph_induced(cur, node_keep=(m["remove"][ug.node_unitig.long()] == 0).to(m["remove"].dtype))
        for f, dt in IND:
            assert byte_mask[f].cpu().numpy().view(dt).tobytes() == r["ind"][f].tobytes(), (i, f, "node_keep")
        ro, d = eng.graph_adjacency(ind["edge_keys"], ind["keys"].numel())
        cur = pkg.KminmerGraph(ind["keys"], ind["counts"], ind["edge_keys"], ind["edge_counts"], ro, d)
        _same_graph(_kg_host(cur), r["graph"], ("round", i))
    before = _kg_host(graph)
    sg, nm, stats = graph.simplify(eng, c["max_tip"], c["max_bubble"])
    _same_graph(_kg_host(graph), before, "self untouched")
    _same_graph(_kg_host(sg), final, "final")
    assert nm.cpu().numpy().tobytes() == node_map.tobytes()
    assert stats == [{"nodes": len(r["keep"]), "unitigs": r["uni"]["n_unitigs"], "tips": r["tips"], "bubbles": r["bubbles"], "removed": r["removed"]}
                     for r in rounds]
    print("device rounds:", stats)
    assert stats[0]["tips"] >= 1 and stats[0]["bubbles"] >= 1 and stats[-1]["removed"] == 0 and len(stats) <= 12
    again = eng.graph_unitigs(sg.row_off, sg.dst, sg.n_nodes)  # its own validation: CSR rules and twin symmetry
    assert again["n_unitigs"] == uni["n_unitigs"] < stats[0]["unitigs"]
    sg2, nm2, stats2 = sg.simplify(eng, c["max_tip"], c["max_bubble"])
    assert len(stats2) == 1 and stats2[0]["removed"] == 0 and nm2.cpu().numpy().tolist() == list(range(sg.n_nodes))
    _same_graph(_kg_host(sg2), final, "second simplify")
    one = graph.simplify(eng, c["max_tip"], c["max_bubble"], max_rounds=1)  # max_rounds ends the loop
    assert len(one[2]) == 1 and one[0].n_nodes == len(rounds[0]["graph"]["keys"])


@pytest.mark.gpu
def test_node_sequences_subset_and_stitch(eng, ecoli_device, tmp_path):
    """NodeSequences.subset: the records gathered to the new ids, the pool shared; the simplified graph's unitig sequences stitched on the
    device equal the numpy stitch from the subset records; write_gfa and write_fasta take them as they are"""
    c = ECOLI
    reads, outs, graph, (tus, b, g, final, node_map, rounds, nodes, sub, uni, seqs) = ecoli_device
    ns = pkg.NodeSequences.build(eng, graph, outs)
    sg, nm, stats = graph.simplify(eng, c["max_tip"], c["max_bubble"])
    ss = ns.subset(nm)
    assert ss.pool.data_ptr() == ns.pool.data_ptr() and ss.n_bytes == ns.n_bytes and ss.k == ns.k
    h = ss.host()
    for f in list(tus.NODE_DT) + ["rep", "pool"]:
        assert h[f].tobytes() == np.asarray(sub[f], dtype=h[f].dtype).tobytes(), f
    ug = sg.unitigs(eng)
    out_off, out = ug.sequences(eng, ss)
    assert tg._u64(out_off).tobytes() == seqs["out_off"].tobytes() and out.cpu().numpy().tobytes() == seqs["out"].tobytes()
    assert ug.overlap.cpu().numpy().view(np.uint32).tobytes() == seqs["overlap"].tobytes()
    p, q = str(tmp_path / "s.gfa"), str(tmp_path / "s.fa")
    ug.write_gfa(p, sequences=(out_off, out))
    pkg.write_fasta(q, out_off, out)
    strings = tus.unitig_strings(uni, seqs)
    s_lines = [x.split("\t") for x in open(p).read().split("\n") if x.startswith("S\t")]
    assert [x[2].encode() for x in s_lines] == strings and open(q).read().split("\n")[1::2][:len(strings)] == [s.decode() for s in strings]
    sg.write_gfa(p, sequences=ss)
    assert sum(1 for x in open(p).read().split("\n") if x.startswith("S\t")) == sg.n_nodes


@pytest.mark.gpu
def test_error_free_simplified_unitigs_on_device_are_slices_of_the_genome(eng, oracle, ecoli):
    """the error-free variant of the same reads: device stitch == numpy stitch, and every simplified unitig is a slice of the genome
    or of its reverse complement"""
    import test_unitig_sequences as tus

    c = ECOLI
    reads = sample_reads_with_errors(ecoli, c["n"], c["seed"], 0.0)
    _, b, g, final, node_map, rounds, nodes, sub, uni, seqs = simplified_sequences_reference(oracle, reads)
    outs = [tus._extract_mn(eng, reads, c["l"], c["k"], c["d"], pkg.HashMode.Regular)]
    graph = pkg.KminmerGraph.build(eng, outs, min_count=c["min_count"])
    sg, nm, stats = graph.simplify(eng, c["max_tip"], c["max_bubble"])
    assert nm.cpu().numpy().tobytes() == node_map.tobytes()
    out_off, out = sg.unitigs(eng).sequences(eng, pkg.NodeSequences.build(eng, graph, outs).subset(nm))
    assert tg._u64(out_off).tobytes() == seqs["out_off"].tobytes() and out.cpu().numpy().tobytes() == seqs["out"].tobytes()
    off, text, rc = tg._u64(out_off).tolist(), out.cpu().numpy().tobytes(), tus.revcomp(ecoli)
    assert all(text[a:z] in ecoli or text[a:z] in rc for a, z in zip(off[:-1], off[1:]))


@pytest.mark.gpu
def test_device_deterministic(eng):
    rng = np.random.default_rng(35)
    g = random_graph_with_errors(rng, 40000, 100, 3000, 3000)
    r = round_reference(g, 4, 8)
    runs = []
    for _ in range(2):
        s, a, b, c, rem = raw_mask(eng, r["uro"], r["ud"], r["uni"]["uni_off"], r["ucnt"], 4, 8)
        s2, nn, ne, host = raw_induced(eng, g, node_unitig=r["uni"]["node_unitig"], remove=rem[:len(r["remove"])])
        assert s == 0 and s2 == 0
        runs.append(rem.tobytes() + b"".join(host[f].tobytes() for f, _ in IND) + repr((a, b, c, nn, ne)).encode())
    assert runs[0] == runs[1]
    assert rem[:len(r["remove"])].tobytes() == r["remove"].tobytes() and host["edge_keys"][:ne].tobytes() == r["ind"]["edge_keys"].tobytes()
