"""Bubbles that are not simple, popped on the device: s2k_graph_bubble_mask (include/s2k.h) and
KminmerGraph.simplify(..., bubble_nodes=...).  The reference is `bubble_reference`, a serial restatement of the header's rule with the
same slots and the same order (plain lists, Python integers); the device's mask and totals equal its results exactly, in every test.

Figures printed by test_reference_ecoli_fixture_rounds (CPU tier, seen there; the device test below asserts that KminmerGraph.simplify
gives the same rounds): DESIGN.md §3.24."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import test_graph as tg
import test_simplify as ts
import test_unitigs as tu

pkg = import_package()

SYM = "s2k_graph_bubble_mask"
M64 = (1 << 64) - 1
MN, MB = 6, 40  # max_nodes and max_bubble of the hand-made cases


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def bubble_traverse(ro, d, cnt, S, cap):
    """the traversal from S with a list of at most cap entries -> None (failure) or (ids in slot order, the sink's slot, bp per slot)"""
    ids, r, best, bp, expanded, slot = [S], [0], [0], [None], [False], {S: 0}
    while True:
        ready = [i for i in range(len(ids)) if r[i] == 0 and not expanded[i]]
        if any(expanded) and len(ready) == 1 and all(expanded[i] or i == ready[0] for i in range(len(ids))):
            return ids, ready[0], bp
        if not ready:
            return None  # an in-edge from outside
        e = ready[0]
        expanded[e] = True
        V = ids[e]
        row = d[ro[V]: ro[V + 1]]
        if not row:
            return None  # a dead end inside
        s = (best[e] + (cnt[V >> 1] if e else 0)) & M64
        for W in row:
            if W >> 1 == S >> 1 or W ^ 1 in slot:
                return None  # a cycle, a hairpin, an inversion
            if W not in slot:
                inn = ro[(W ^ 1) + 1] - ro[W ^ 1]
                if len(ids) == cap or inn == 0:
                    return None
                slot[W] = len(ids)
                ids.append(W), r.append(inn - 1), best.append(s), bp.append(V), expanded.append(False)
            else:
                i = slot[W]
                if r[i] == 0:
                    return None  # not twin-symmetric
                r[i] -= 1
                if s > best[i] or (s == best[i] and V < bp[i]):
                    best[i], bp[i] = s, V


def bubbles_of(row_off, dst, uni_off, cnt, max_nodes, max_bubble):
    """-> (n_sources, the bubbles with a non-empty removable set in source order: dicts S, T, interior and removable (unitigs), applied)"""
    ro, d = [int(x) for x in row_off], [int(x) for x in dst]
    off, cnt = [int(x) for x in uni_off], [int(x) for x in cnt]
    T = len(off) - 1
    n_sources, found, owner = 0, [], {}
    for S in range(2 * T):
        if ro[S + 1] - ro[S] < 2:
            continue
        n_sources += 1
        t = bubble_traverse(ro, d, cnt, S, max_nodes + 2)
        if t is None:
            continue
        ids, tslot, bp = t
        interior = [W for i, W in enumerate(ids) if i != 0 and i != tslot]
        if not interior or sum(off[(W >> 1) + 1] - off[W >> 1] for W in interior) > max_bubble:
            continue
        kept, cur = set(), tslot
        while cur != 0:
            cur = ids.index(bp[cur])
            kept.add(ids[cur])
        removable = [W >> 1 for W in interior if W not in kept]
        if removable:
            found.append({"S": S, "T": ids[tslot], "interior": [W >> 1 for W in interior], "removable": removable})
            for W in interior:
                owner[W >> 1] = min(owner.get(W >> 1, S), S)
    for b in found:
        b["applied"] = all(owner[t] == b["S"] for t in b["interior"])
    return n_sources, found


def bubble_reference(row_off, dst, uni_off, cnt, max_nodes, max_bubble):
    """-> (remove uint8[T], n_sources, n_found, n_applied, n_removed) by the rule of include/s2k.h"""
    n_sources, found = bubbles_of(row_off, dst, uni_off, cnt, max_nodes, max_bubble)
    remove = np.zeros(len(uni_off) - 1, dtype=np.uint8)
    for b in found:
        if b["applied"]:
            assert not remove[b["removable"]].any()  # applied bubbles share no interior unitig
            remove[b["removable"]] = 1
    return remove, n_sources, len(found), sum(b["applied"] for b in found), int(remove.sum())


def bubble_round_reference(g, max_tip, max_bubble, bubble_nodes, alone=False):
    """one round of KminmerGraph.simplify(..., bubble_nodes) from the references -> test_simplify.round_reference's dict with stats
    (the round's stats dict) and, where the bubble mask ran, found (bubbles_of's list).  alone: the bubble mask whatever the tip and
    simple-bubble rules would remove, as a caller of Engine.graph_bubble_mask may apply it"""
    uni, uro, ud, ucnt = ts.unitig_view(g)
    remove, nt, nb, nr = ts.simplify_reference(uro, ud, uni["uni_off"], ucnt, max_tip, max_bubble)
    stats = {"nodes": len(g["keys"]), "unitigs": uni["n_unitigs"], "tips": nt, "bubbles": nb, "removed": nr}
    found = None
    if (nr == 0 or alone) and bubble_nodes > 0:
        ns, found = bubbles_of(uro, ud, uni["uni_off"], ucnt, bubble_nodes, max_bubble)
        remove, ns2, nf, na, nr = bubble_reference(uro, ud, uni["uni_off"], ucnt, bubble_nodes, max_bubble)
        stats.update(sources=ns, found=nf, applied=na, removed=nr)
    keep = remove[uni["node_unitig"].astype(np.int64)] == 0 if len(g["keys"]) else np.zeros(0, dtype=bool)
    ind = ts.induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], keep)
    ro, d = tg.adjacency_reference(ind["edge_keys"], len(ind["keys"]))
    nxt = {f: ind[f] for f in ("keys", "counts", "edge_keys", "edge_counts")}
    nxt.update(row_off=ro, dst=d)
    return {"uni": uni, "uro": uro, "ud": ud, "ucnt": ucnt, "remove": remove, "removed": nr, "keep": keep, "ind": ind, "graph": nxt, "stats": stats,
            "found": found}


def bubble_rounds_reference(g, max_tip, max_bubble, bubble_nodes, max_rounds=16):
    """KminmerGraph.simplify(max_tip, max_bubble, max_rounds, bubble_nodes) from the references -> (final graph, node_map, rounds)"""
    node_map = np.arange(len(g["keys"]), dtype=np.int32)
    rounds = []
    for _ in range(max_rounds):
        r = bubble_round_reference(g, max_tip, max_bubble, bubble_nodes)
        rounds.append(r)
        if r["removed"] == 0:
            break
        alive = node_map >= 0
        node_map[alive] = r["ind"]["new_id"].view(np.int32)[node_map[alive]]
        g = r["graph"]
    return g, node_map, rounds


# ---- hand-made unitig graphs -----------------------------------------------------------------------------------------------------------
def _chain(k):
    """0 -> 1 -> T beside 0 -> 2 -> 3 -> .. -> k + 1 -> T, T = k + 2: an interior of k + 1 unitigs; the chain has the higher sum"""
    T = k + 2
    return T + 1, [(0, 2), (2, 2 * T)] + [(0, 4)] + [(2 * i, 2 * i + 2) for i in range(2, k + 1)] + [(2 * (k + 1), 2 * T)]


def _chain_case(k, lens_interior, found):
    n, edges = _chain(k)
    want = [0] * n
    want[1] = found
    return (n, edges, [20] + lens_interior + [20], [200, 5] + [10] * k + [200], want, 2, 2 * found, found)


_BUB2 = [(0, 2), (0, 4), (2, 6), (4, 6)]  # 0 -> {1, 2} -> 3
# name -> (unitigs, edges between oriented unitigs (twins added), members per unitig, count per unitig, the expected mask, sources,
#          found, applied), all at max_nodes MN = 6 and max_bubble MB = 40.  Unitig t forward is 2 t.
HAND = {
    # 0 -> 1 -> 2 -> 4 beside 0 -> 3 -> 4; found from 0+ and from 4-, the smaller source applies
    "two unitigs against one": (5, [(0, 2), (2, 4), (4, 8), (0, 6), (6, 8)], [20, 2, 2, 3, 20], [200, 10, 10, 15, 200], [0, 0, 0, 1, 0], 2, 2, 1),
    "one unitig against two": (5, [(0, 2), (2, 4), (4, 8), (0, 6), (6, 8)], [20, 2, 2, 3, 20], [200, 10, 10, 50, 200], [0, 1, 1, 0, 0], 2, 2, 1),
    # 0 -> {1, 2, 3}, {1, 2} -> 4 -> 5, 3 -> 5: found from 0+ and from 5-; from 4- the walk
    # stops at 0-, which waits for 3-
    "three branches with an inner join": (6, [(0, 2), (0, 4), (0, 6), (2, 8), (4, 8), (8, 10), (6, 10)], [20, 2, 2, 2, 2, 20], [200, 10, 4, 6, 20, 200],
                                          [0, 0, 1, 1, 0, 0], 3, 2, 1),
    # 0 -> 1 -> {2, 3} -> 4 -> 6 beside 0 -> 5 -> 6: the inner bubble (source 1+ = 2, and 4- = 9) loses its interior to source 0
    "bubble inside a bubble": (7, [(0, 2), (2, 4), (2, 6), (4, 8), (6, 8), (8, 12), (0, 10), (10, 12)], [20, 2, 2, 2, 2, 3, 20],
                               [200, 10, 10, 3, 10, 4, 200], [0, 0, 0, 1, 0, 1, 0], 4, 4, 1),
    # the same with the outer side branch the heavier: the outer bubble removes the whole inner one, the inner verdict (3) is not applied
    "bubble inside a bubble, outer keeps the side": (7, [(0, 2), (2, 4), (2, 6), (4, 8), (6, 8), (8, 12), (0, 10), (10, 12)], [20, 2, 2, 2, 2, 3, 20],
                                                     [200, 10, 10, 3, 10, 100, 200], [0, 1, 1, 1, 1, 0, 0], 4, 4, 1),
    # 0 -> {1, 2} -> 3 -> {4, 5} -> 6: sources 0+, 3+, 3-, 6-; 0+ owns {1, 2}, 3+ owns {4, 5}
    "two bubbles in a chain": (7, [(0, 2), (0, 4), (2, 6), (4, 6), (6, 8), (6, 10), (8, 12), (10, 12)], [20, 2, 2, 20, 2, 2, 20],
                               [200, 10, 3, 200, 2, 9, 200], [0, 0, 1, 0, 1, 0, 0], 4, 4, 2),
    "direct edge beside a detour": (3, [(0, 2), (2, 4), (0, 4)], [20, 2, 20], [200, 10, 200], [0, 0, 0], 2, 0, 0),
    # 0 -> 3 -> 4 (10) beside 0 -> 1 -> 2 -> 4 (4 + 6): 3+ reaches the sink first, 2+ (the smaller id) replaces it on the equal sum
    "equal sums": (5, [(0, 6), (6, 8), (0, 2), (2, 4), (4, 8)], [20, 2, 2, 2, 20], [200, 4, 6, 10, 200], [0, 0, 0, 1, 0], 2, 2, 1),
    "equal sums, two branches": (4, _BUB2, [20, 2, 2, 20], [200, 7, 7, 200], [0, 0, 1, 0], 2, 2, 1),
    "dead end inside": (4, [(0, 2), (0, 4), (2, 6)], [20, 2, 2, 20], [200, 10, 3, 200], [0, 0, 0, 0], 1, 0, 0),
    "in-edge from outside": (5, _BUB2 + [(8, 2)], [20, 2, 2, 20, 20], [200, 10, 3, 200, 200], [0, 0, 0, 0, 0], 3, 0, 0),
    "inversion": (3, [(0, 2), (0, 4), (2, 5)], [20, 2, 2], [200, 10, 3], [0, 0, 0], 1, 0, 0),
    "cycle back to the source": (3, [(0, 2), (0, 4), (2, 0)], [20, 2, 2], [200, 10, 3], [0, 0, 0], 1, 0, 0),
    "hairpin": (3, [(0, 2), (0, 4), (2, 1)], [20, 2, 2], [200, 10, 3], [0, 0, 0], 1, 0, 0),
    "interior of max_nodes unitigs": _chain_case(MN - 1, [2] * MN, 1),
    "interior of max_nodes + 1 unitigs": _chain_case(MN, [2] * (MN + 1), 0),
    "members equal to max_bubble": _chain_case(3, [MB - 6, 2, 2, 2], 1),
    "members equal to max_bubble + 1": _chain_case(3, [MB - 6, 2, 2, 3], 0),
    "the simple bubble of test_simplify": ts.HAND["two-branch bubble"][:4] + ([0, 0, 1, 0], 2, 2, 1),
}


def hand_case(name):
    T, edges, lens, cnts, want, ns, nf, na = HAND[name]
    assert len(lens) == len(cnts) == len(want) == T
    ro, d = tu.csr_of(T, edges)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return T, ro, d, off, np.array(cnts, dtype=np.uint64), (np.array(want, dtype=np.uint8), ns, nf, na, int(sum(want)))


def all_hand_cases():
    """every hand-made case side by side in one graph: the components do not touch, so masks concatenate and totals add up"""
    edges, lens, cnts, want, tot, base = [], [], [], [], [0, 0, 0], 0
    for name in HAND:
        T, e, l, c, w, ns, nf, na = HAND[name]
        edges += [(u + 2 * base, v + 2 * base) for u, v in e]
        lens, cnts, want = lens + list(l), cnts + list(c), want + list(w)
        tot = [tot[0] + ns, tot[1] + nf, tot[2] + na]
        base += T
    ro, d = tu.csr_of(base, edges)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return base, ro, d, off, np.array(cnts, dtype=np.uint64), (np.array(want, dtype=np.uint8), tot[0], tot[1], tot[2], int(sum(want)))


def chain_graph(k):
    """_chain(k) with two members per unitig: an interior of k + 1 unitigs and 2 k + 2 members"""
    n, edges = _chain(k)
    ro, d = tu.csr_of(n, edges)
    return n, ro, d, np.arange(0, 2 * n + 1, 2, dtype=np.uint64), np.array([200, 5] + [10] * k + [200], dtype=np.uint64)


def hub_graph(row=200):
    """source 0 with `row` successors that all join at the last unitig, and a small bubble behind it"""
    T = row + 5
    edges = [(0, 2 * t) for t in range(1, row + 1)] + [(2 * t, 2 * (row + 1)) for t in range(1, row + 1)]
    a = row + 1
    edges += [(2 * a, 2 * (a + 1)), (2 * a, 2 * (a + 2)), (2 * (a + 1), 2 * (a + 3)), (2 * (a + 2), 2 * (a + 3))]
    ro, d = tu.csr_of(T, edges)
    return T, ro, d, np.arange(T + 1, dtype=np.uint64), (np.arange(T, dtype=np.uint64) % np.uint64(7) + np.uint64(3))


def planted_graph(rng, n, extra, n_tips, n_bubbles, n_planted):
    """test_simplify.random_graph_with_errors with bubbles that are not simple on top: beside a walk of 2 .. 5 edges of the graph, a
    side path a -> x1 -> x2 -> x3 -> b whose middle is doubled (x1 -> y -> x3: a bubble inside the bubble) or split in two unitigs by
    an edge that joins it (x2 -> b as well) -> a graph dict"""
    g = ts.random_graph_with_errors(rng, n, extra, n_tips, n_bubbles)
    N = len(g["keys"])
    ro, d = [int(x) for x in g["row_off"]], [int(x) for x in g["dst"]]
    edges = [(u, d[i]) for u in range(2 * N) for i in range(ro[u], ro[u + 1])]
    nxt = N
    for _ in range(n_planted):
        a = b = int(rng.integers(0, 2 * N))
        for _ in range(int(rng.integers(2, 6))):
            if ro[b + 1] == ro[b]:
                break
            b = d[ro[b] + int(rng.integers(0, ro[b + 1] - ro[b]))]
        if b == a:
            continue
        x = [2 * (nxt + j) + int(rng.integers(0, 2)) for j in range(4)]
        nxt += 4
        edges += [(a, x[0]), (x[0], x[1]), (x[1], x[2]), (x[2], b), (x[0], x[3]), (x[3], x[2])]
        if rng.random() < 0.3:
            edges.append((x[1], b))
    ro2, d2 = tu.csr_of(nxt, edges)
    src = np.repeat(np.arange(2 * nxt, dtype=np.uint64), np.diff(ro2.astype(np.int64)))
    ek = (src << np.uint64(32)) | d2.astype(np.uint64)
    pair = np.minimum(ek, ((d2.astype(np.uint64) ^ np.uint64(1)) << np.uint64(32)) | (src ^ np.uint64(1)))
    keys = np.concatenate([g["keys"], g["keys"][-1] + np.cumsum(rng.integers(1, 1000, size=nxt - N)).astype(np.uint64)])
    counts = np.concatenate([g["counts"], rng.integers(2, 7, size=nxt - N).astype(np.uint32)])
    return {"keys": keys, "counts": counts, "edge_keys": ek, "edge_counts": (pair % np.uint64(7) + np.uint64(1)).astype(np.uint32), "row_off": ro2, "dst": d2}


def random_unitig_graph(rng, n_nodes):
    """the unitig graph (row_off, dst, uni_off, cnt) of a planted graph of about n_nodes nodes"""
    g = planted_graph(rng, n_nodes, n_nodes // 50, n_nodes // 10, n_nodes // 8, n_nodes // 8 + 1)
    uni, uro, ud, ucnt = ts.unitig_view(g)
    return uro, ud, uni["uni_off"], ucnt


def check_round(r, tag):
    """the invariants of the header for one round of bubble_rounds_reference"""
    assert ts.dead_ends_created(r) == 0, tag
    ts.is_graph_sound(r["graph"])
    assert tu.is_twin_symmetric(r["graph"]["row_off"], r["graph"]["dst"], len(r["graph"]["keys"])), tag
    if r["found"] is None:
        return
    applied = [b for b in r["found"] if b["applied"]]
    inside = {t for b in applied for t in b["interior"]}
    assert set(np.nonzero(r["remove"])[0].tolist()) <= inside, tag  # every removed unitig lies in an applied bubble's interior
    assert not r["found"] or applied, tag                            # a round that finds a bubble applies one
    ro, d = [int(x) for x in r["uro"]], [int(x) for x in r["ud"]]
    for b in applied:  # the interior has no edge to or from anything outside the bubble
        members = set(b["interior"]) | {b["S"] >> 1, b["T"] >> 1}
        for t in b["interior"]:
            for U in (2 * t, 2 * t + 1):
                assert all(W >> 1 in members for W in d[ro[U]: ro[U + 1]]), (tag, b, U)


# ---- the two read sets of the E. coli fixture -------------------------------------------------------------------------------------------
BUBBLE_NODES = 16
MIXED = dict(n_clean=300, n_noisy=40, seed_clean=7, seed_noisy=8, rate=0.002, min_count=1)  # DESIGN.md §3.12's kind of set


def mixed_reads(ecoli):
    """300 error-free reads, then 40 reads with 0.2 % substitutions (the clean ones first: a node seen in both takes a clean reading)"""
    m = MIXED
    return ts.sample_reads_with_errors(ecoli, m["n_clean"], m["seed_clean"], 0.0) + ts.sample_reads_with_errors(ecoli, m["n_noisy"], m["seed_noisy"], m["rate"])


def fixture_rounds(oracle, ecoli, reads, min_count, bubble_nodes):
    """reads -> the rounds of the reference and the figures of the final graph: unitigs, the longest one in bases, those that are no
    slice of the genome or of its reverse complement"""
    c = ts.ECOLI
    tus, b = ts._oracle_batch_mn(oracle, reads)
    g = tg.graph_reference([b], min_count)
    final, node_map, rounds = bubble_rounds_reference(g, c["max_tip"], c["max_bubble"], bubble_nodes)
    sub = ts.subset_records(tus.node_sequences_reference([b], g["keys"], c["k"]), node_map)
    uni = tu.unitig_reference(final["row_off"], final["dst"], len(final["keys"]))
    strings = tus.unitig_strings(uni, tus.unitig_sequences_reference(uni, sub))
    rc = tus.revcomp(ecoli)
    return g, final, node_map, rounds, {"unitigs": uni["n_unitigs"], "longest": max(len(s) for s in strings),
                                        "not_a_slice": sum(1 for s in strings if s not in ecoli and s not in rc)}


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    assert hasattr(lib, SYM) and SYM in pkg.ABI_SYMBOLS and SYM + "(" in header
    assert "#define S2K_BUBBLE_MAX_NODES %du" % pkg.BUBBLE_MAX_NODES in header and "#define S2K_BUBBLE_WAVES %du" % pkg.BUBBLE_WAVES in header
    assert hasattr(pkg.Engine, "graph_bubble_mask") and "bubble_nodes" in pkg.KminmerGraph.simplify.__code__.co_varnames


def test_cpp_bubble_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "bubble_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bubble_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


@pytest.mark.parametrize("name", list(HAND))
def test_reference_hand_made(name):
    T, ro, d, off, cnt, want = hand_case(name)
    assert tu.is_twin_symmetric(ro, d, T)
    got = bubble_reference(ro, d, off, cnt, MN, MB)
    assert got[0].tolist() == want[0].tolist() and got[1:] == want[1:], (name, got)


def test_reference_hand_made_side_by_side_and_bounds():
    T, ro, d, off, cnt, want = all_hand_cases()
    got = bubble_reference(ro, d, off, cnt, MN, MB)
    assert got[0].tolist() == want[0].tolist() and got[1:] == want[1:]
    assert want[2] >= 20 and want[3] >= 12  # found, applied
    # the nested case in detail: the inner bubble is found from both ends and applied from neither
    T, ro, d, off, cnt, want = hand_case("bubble inside a bubble")
    ns, found = bubbles_of(ro, d, off, cnt, MN, MB)
    assert [(b["S"], b["T"], sorted(b["interior"]), b["applied"]) for b in found] == [
        (0, 12, [1, 2, 3, 4, 5], True), (2, 8, [2, 3], False), (9, 3, [2, 3], False), (13, 1, [1, 2, 3, 4, 5], False)]
    # the bounds of the constant: an interior of 62 and of 63 unitigs at max_nodes 62; max_nodes 1 finds nothing to remove
    for k, mn, found in ((61, 62, 1), (62, 62, 0), (61, 61, 0), (1, 1, 0), (1, 2, 1)):
        n, ro, d, off, cnt = chain_graph(k)
        got = bubble_reference(ro, d, off, cnt, mn, 1000)
        assert got[1:] == (2, 2 * found, found, found) and got[0].tolist() == [0, found] + [0] * (n - 2), (k, mn, got)
    T, ro, d, off, cnt = hub_graph()
    got = bubble_reference(ro, d, off, cnt, 62, 1000)
    assert got[1:] == (4, 2, 1, 1)  # the hub and its mirror fail (a list of 202); the small bubble behind is found from both ends


def test_reference_random_graphs_invariants():
    """random graphs with tips, simple bubbles and planted bubbles that are not simple: every round keeps the header's invariants, and
    the bubble rule finds work that the simple rules leave"""
    rng = np.random.default_rng(41)
    applied = nested_losers = 0
    for n, extra, nt, nb, npl in ((8, 0, 1, 1, 2), (40, 2, 4, 4, 6), (200, 0, 20, 20, 30), (200, 20, 30, 10, 30), (600, 10, 60, 60, 80)):
        for rep in range(3):
            g = planted_graph(rng, n, extra, nt, nb, npl)
            ts.is_graph_sound(g)
            final, node_map, rounds = bubble_rounds_reference(g, 4, 8, 8, max_rounds=len(g["keys"]) + 1)
            assert rounds[-1]["removed"] == 0
            for i, r in enumerate(rounds + [bubble_round_reference(g, 4, 8, 8, alone=True)]):  # and the mask alone on the raw graph
                check_round(r, (n, rep, i))
                if r["found"]:
                    applied += sum(b["applied"] for b in r["found"])
                    nested_losers += sum(not b["applied"] for b in r["found"])
            kept = node_map >= 0
            assert int(kept.sum()) == len(final["keys"]) and (final["keys"] == g["keys"][kept]).all()
            plain = ts.simplify_rounds_reference(g, 4, 8, max_rounds=len(g["keys"]) + 1)[0]
            assert len(final["keys"]) <= len(plain["keys"])
    assert applied > 50 and nested_losers > 50, (applied, nested_losers)


def test_reference_ecoli_fixture_rounds(oracle, ecoli):
    """the two read sets of DESIGN.md §3.12 and §3.24 through the reference rounds without and with the bubble rule: the figures are
    printed; asserted is what holds by construction, and that the rule has work on the mixed set"""
    c = ts.ECOLI
    sets = (("600 reads, 0.5 % substitutions, min_count 2", ts.sample_reads_with_errors(ecoli, c["n"], c["seed"], c["rate"]), c["min_count"]),
            ("300 clean + 40 noisy reads, min_count 1", mixed_reads(ecoli), MIXED["min_count"]))
    applied = []
    for name, reads, min_count in sets:
        g, plain, _, prounds, pfig = fixture_rounds(oracle, ecoli, reads, min_count, 0)
        g, final, node_map, rounds, fig = fixture_rounds(oracle, ecoli, reads, min_count, BUBBLE_NODES)
        print("%s: %d nodes, %d unitigs" % (name, len(g["keys"]), rounds[0]["stats"]["unitigs"]))
        print("  bubble_nodes 0: %s in %d rounds" % (pfig, len(prounds)))
        print("  bubble_nodes %d: %s in %d rounds %s" % (BUBBLE_NODES, fig, len(rounds), [r["stats"] for r in rounds if "found" in r["stats"]]))
        assert all("found" not in r["stats"] for r in prounds) and prounds[-1]["removed"] == 0
        for i, r in enumerate(rounds):
            check_round(r, (name, i))
        ts.is_graph_sound(final)
        assert rounds[-1]["removed"] == 0 and fig["unitigs"] <= pfig["unitigs"] and len(final["keys"]) <= len(plain["keys"])
        applied.append(sum(r["stats"].get("applied", 0) for r in rounds))
    assert max(applied) >= 1, applied


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def raw_bubble(eng, ro, d, off, cnt, mn, mb, n_edges=None, T=None, want_remove=True, null=(), ctx=True):
    """s2k_graph_bubble_mask through ctypes, guard bytes behind d_remove -> (status, sources, found, applied, removed, host remove with
    guards)"""
    import torch

    T = len(off) - 1 if T is None else T
    dro, dd, doff, dcnt = ts._dev(ro, np.uint64), ts._dev(d, np.uint32), ts._dev(off, np.uint64), ts._dev(cnt, np.uint64)
    rem = ts._out(T, np.uint8)
    t = [ctypes.c_uint64(777) for _ in range(4)]
    torch.cuda.synchronize()
    s = eng.lib.s2k_graph_bubble_mask(eng.ctx if ctx else None, ts._ptr(dro, "row_off" in null), ts._ptr(dd, "dst" in null or len(d) == 0),
                                      len(d) if n_edges is None else n_edges, T, ts._ptr(doff, "uni_off" in null), ts._ptr(dcnt, "cnt" in null), mn, mb,
                                      ts._ptr(rem, not want_remove), *(ctypes.byref(x) for x in t))
    return (s,) + tuple(x.value for x in t) + (ts._host(rem, np.uint8),)


def device_bubble(eng, ro, d, off, cnt, mn, mb, want, tag):
    """the call against `want` = (remove, sources, found, applied, removed), guard untouched; and the totals-only call"""
    T = len(off) - 1
    got = raw_bubble(eng, ro, d, off, cnt, mn, mb)
    assert got[:5] == (0,) + tuple(want[1:]), (tag, got[:5], want[1:])
    assert got[5][:T].tobytes() == want[0].tobytes(), (tag, got[5][:T], want[0])
    assert ts._marked(got[5], np.uint8, T), (tag, "guard")
    got = raw_bubble(eng, ro, d, off, cnt, mn, mb, want_remove=False)
    assert got[:5] == (0,) + tuple(want[1:]) and ts._marked(got[5], np.uint8), (tag, "totals only")


@pytest.mark.gpu
def test_device_hand_made(eng):
    for name in HAND:
        T, ro, d, off, cnt, want = hand_case(name)
        device_bubble(eng, ro, d, off, cnt, MN, MB, want, name)
    T, ro, d, off, cnt, want = all_hand_cases()
    device_bubble(eng, ro, d, off, cnt, MN, MB, want, "side by side")


@pytest.mark.gpu
def test_device_bounds_and_hub(eng):
    for k, mn in ((61, 62), (62, 62), (61, 61), (1, 1), (1, 2)):
        n, ro, d, off, cnt = chain_graph(k)
        device_bubble(eng, ro, d, off, cnt, mn, 1000, bubble_reference(ro, d, off, cnt, mn, 1000), ("chain", k, mn))
    T, ro, d, off, cnt = hub_graph()
    device_bubble(eng, ro, d, off, cnt, 62, 1000, bubble_reference(ro, d, off, cnt, 62, 1000), "hub")


def _unitig_graph_of_size(rng, T):
    """a random graph of exactly T unitigs: a planted graph read as a unitig graph (one unitig per node, 1 .. 3 members each; the rule
    does not ask for a compacted graph), isolated unitigs up to T, and the unitigs renumbered at random so that sources, sinks and
    the isolated ones lie anywhere in the waves and tiles"""
    if T < 12:
        N, edges, cnt = 0, [], np.zeros(0, dtype=np.uint64)
    else:
        g = planted_graph(rng, T // 3, T // 100, T // 30, T // 20, T // 12)
        N, ro, d, cnt = len(g["keys"]), [int(x) for x in g["row_off"]], [int(x) for x in g["dst"]], g["counts"].astype(np.uint64)
        edges = [(u, d[i]) for u in range(2 * N) for i in range(ro[u], ro[u + 1])]
    assert N <= T
    perm = rng.permutation(T)
    ro2, d2 = tu.csr_of(T, [(2 * int(perm[u >> 1]) + (u & 1), 2 * int(perm[v >> 1]) + (v & 1)) for u, v in edges])
    lens, cnts = rng.integers(1, 4, size=T), np.full(T, 9, dtype=np.uint64)
    cnts[perm[:N]] = cnt
    return ro2, d2, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), cnts


@pytest.mark.gpu
def test_device_random_graphs(eng):
    """random unitig graphs of 1, 63, 64, 65 and 4 097 unitigs (a wave, a tile of 2 048 oriented ids and its seam) at three bounds"""
    rng = np.random.default_rng(42)
    found = applied = 0
    for T in (1, 63, 64, 65, 4097):
        ro, d, off, cnt = _unitig_graph_of_size(rng, T)
        for mn, mb in ((8, 8), (3, 40), (62, 1000)):
            want = bubble_reference(ro, d, off, cnt, mn, mb)
            device_bubble(eng, ro, d, off, cnt, mn, mb, want, ("random", T, mn, mb))
            found, applied = found + want[2], applied + want[3]
    assert applied > 100 and found > applied, (found, applied)


@pytest.mark.gpu
def test_device_edge_shapes_and_refusals(eng):
    z64, z32 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    got = raw_bubble(eng, np.zeros(1, dtype=np.uint64), z32, np.zeros(1, dtype=np.uint64), z64, MN, MB)  # n_unitigs == 0
    assert got[:5] == (0, 0, 0, 0, 0) and ts._marked(got[5], np.uint8)
    ro, off, cnt = np.zeros(11, dtype=np.uint64), np.arange(6, dtype=np.uint64), np.full(5, 9, dtype=np.uint64)  # n_edges == 0
    device_bubble(eng, ro, z32, off, cnt, MN, MB, (np.zeros(5, dtype=np.uint8), 0, 0, 0, 0), "no edges")
    T, ro, d, off, cnt, want = all_hand_cases()

    def refused(ro_=ro, d_=d, off_=off, mn=MN, code=1, **kw):
        got = raw_bubble(eng, ro_, d_, off_, cnt, mn, MB, **kw)
        assert got[:5] == (code, 0, 0, 0, 0) and ts._marked(got[5], np.uint8), (got[:5], kw)

    refused(mn=0)
    refused(mn=pkg.BUBBLE_MAX_NODES + 1)
    x = d.copy()  # an id >= 2 T
    x[1] = 2 * T
    refused(d_=x)
    refused(n_edges=len(d) + 1)  # row_off[2 T] != n_edges
    refused(n_edges=len(d) - 1)
    y = ro.copy()  # row_off not starting at 0; decreasing
    y[0] = 1
    refused(ro_=y)
    y = ro.copy()
    y[1] = y[2] + np.uint64(1)
    refused(ro_=y)
    y = off.copy()  # a unitig without a member
    y[5] = y[4]
    refused(off_=y)
    refused(ctx=False)
    for f in ("row_off", "dst", "uni_off", "cnt"):
        refused(null=(f,))
    device_bubble(eng, ro, d, off, cnt, MN, MB, want, "after the refusals")  # no flag or total left behind
    z = [ctypes.c_uint64(5) for _ in range(4)]
    refs = [ctypes.byref(x) for x in z]
    assert eng.lib.s2k_graph_bubble_mask(eng.ctx, ctypes.c_void_p(8), None, 0, 2 ** 31, ctypes.c_void_p(8), ctypes.c_void_p(8), MN, MB, None, *refs) == 1
    assert eng.lib.s2k_graph_bubble_mask(eng.ctx, None, None, 3, 0, None, None, MN, MB, None, *refs) == 1  # edges without unitigs
    assert eng.lib.s2k_graph_bubble_mask(eng.ctx, None, None, 0, 1, None, None, MN, MB, None, None, *refs[1:]) == 1
    assert [x.value for x in z] == [0, 0, 0, 0]


@pytest.mark.gpu
def test_device_deterministic_and_poisoned_workspace(eng):
    """two calls are bit-identical, and an engine whose workspace is filled with 0x5a at every hand-out gives the same bytes: every
    word the call reads is one it wrote (owner, found, the sources, the totals)"""
    rng = np.random.default_rng(43)
    ro, d, off, cnt = random_unitig_graph(rng, 6000)
    want = bubble_reference(ro, d, off, cnt, 8, 8)
    assert want[3] > 50
    runs = [raw_bubble(eng, ro, d, off, cnt, 8, 8) for _ in range(2)]
    assert runs[0][:5] == runs[1][:5] == (0,) + want[1:] and runs[0][5].tobytes() == runs[1][5].tobytes()
    os.environ["S2K_POISON_WS"] = str(0x5A)
    try:
        poisoned = pkg.Engine(0)
    finally:
        del os.environ["S2K_POISON_WS"]
    try:
        device_bubble(poisoned, ro, d, off, cnt, 8, 8, want, "poisoned")
        T, hro, hd, hoff, hcnt, hwant = all_hand_cases()
        bad = hd.copy()
        bad[1] = 2 * T
        assert raw_bubble(poisoned, hro, bad, hoff, hcnt, MN, MB)[0] == 1  # a refusal, then the accepted case at once
        device_bubble(poisoned, hro, hd, hoff, hcnt, MN, MB, hwant, "poisoned, after a refusal")
    finally:
        poisoned.close()


@pytest.mark.gpu
def test_kminmer_graph_simplify_with_bubbles_ecoli(eng, oracle, ecoli):
    """KminmerGraph.simplify(..., bubble_nodes) on the two E. coli read sets: stats, final graph and node_map equal the reference
    rounds'; bubble_nodes = 0 is today's result, round for round; Engine.graph_bubble_mask on the first round that runs it equals the
    reference's mask"""
    import test_unitig_sequences as tus

    c = ts.ECOLI
    for reads, min_count in ((ts.sample_reads_with_errors(ecoli, c["n"], c["seed"], c["rate"]), c["min_count"]), (mixed_reads(ecoli), MIXED["min_count"])):
        _, b = ts._oracle_batch_mn(oracle, reads)
        g = tg.graph_reference([b], min_count)
        outs = [tus._extract_mn(eng, reads, c["l"], c["k"], c["d"], pkg.HashMode.Regular)]
        graph = pkg.KminmerGraph.build(eng, outs, min_count=min_count)
        ts._same_graph(ts._kg_host(graph), g, "build")
        final, node_map, rounds = bubble_rounds_reference(g, c["max_tip"], c["max_bubble"], BUBBLE_NODES)
        sg, nm, stats = graph.simplify(eng, c["max_tip"], c["max_bubble"], bubble_nodes=BUBBLE_NODES)
        print("device rounds:", stats)
        assert stats == [r["stats"] for r in rounds]
        ts._same_graph(ts._kg_host(sg), final, "final")
        assert nm.cpu().numpy().tobytes() == node_map.tobytes()
        pfinal, pmap, prounds = ts.simplify_rounds_reference(g, c["max_tip"], c["max_bubble"])
        for kw in ({}, {"bubble_nodes": 0}):
            sg0, nm0, stats0 = graph.simplify(eng, c["max_tip"], c["max_bubble"], **kw)
            assert stats0 == [{"nodes": len(r["keep"]), "unitigs": r["uni"]["n_unitigs"], "tips": r["tips"], "bubbles": r["bubbles"], "removed": r["removed"]}
                              for r in prounds]
            ts._same_graph(ts._kg_host(sg0), pfinal, "bubble_nodes 0")
            assert nm0.cpu().numpy().tobytes() == pmap.tobytes()
        i = next(i for i, r in enumerate(rounds) if r["found"] is not None)  # the graph that round started from, on the device
        cur = graph if i == 0 else graph.simplify(eng, c["max_tip"], c["max_bubble"], max_rounds=i, bubble_nodes=BUBBLE_NODES)[0]
        m = eng.graph_bubble_mask(cur.unitigs(eng), BUBBLE_NODES, c["max_bubble"])
        r = rounds[i]["stats"]
        assert m["remove"].cpu().numpy().tobytes() == rounds[i]["remove"].tobytes()
        assert (m["n_sources"], m["n_found"], m["n_applied"], m["n_removed"]) == (r["sources"], r["found"], r["applied"], r["removed"])
