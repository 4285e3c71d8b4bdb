"""Junction spans from the read paths, and the repeats they resolve: s2k_paths_spans and s2k_graph_resolve_mask (include/s2k.h,
DESIGN.md §3.14).  The references are `spans_reference` and `resolve_reference`, serial restatements of the header's definitions
(plain loops over reads, steps and rows; `find` is a scan of one row); the device's arrays equal theirs exactly, every one of them, in
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
import test_thread as tt
import test_unitigs as tu

pkg = import_package()

SYMS = ("s2k_paths_spans", "s2k_graph_resolve_mask")
LINKED = 1
NONE = 0xFFFFFFFF
PATH = ("unitig", "pos", "count", "flags")


# ---- the references ----------------------------------------------------------------------------------------------------------------
def _find(ro, d, A, B):
    for e in range(ro[A], ro[A + 1]):
        if d[e] == B:
            return e
    return None


def _twin(ro, d, src, e):
    """tw(e) for e = (src[e] -> d[e])"""
    return _find(ro, d, d[e] ^ 1, src[e] ^ 1)


def _sources(ro):
    return [u for u in range(len(ro) - 1) for _ in range(ro[u], ro[u + 1])]


def spans_reference(paths, row_off, dst, uni_off):
    """paths: dict with path_off, unitig, pos, count, flags -> dict: keys (uint64, in step order), edge_support (uint64, one per
    edge), n_followed, n_off_graph, n_linked"""
    ro, d = [int(x) for x in row_off], [int(x) for x in dst]
    off = [int(x) for x in uni_off]
    ln = [off[t + 1] - off[t] for t in range(len(off) - 1)]
    po = [int(x) for x in paths["path_off"]]
    u, p, c, f = ([int(x) for x in paths[k]] for k in PATH)
    src = _sources(ro)
    follow = [None] * len(u)
    for r in range(len(po) - 1):
        for s in range(po[r] + 1, po[r + 1]):  # a read's first step never follows
            if f[s] & LINKED and p[s] == 0 and p[s - 1] + c[s - 1] == ln[u[s - 1] >> 1]:
                follow[s] = _find(ro, d, u[s - 1], u[s])
    support = [0] * len(d)
    for e in follow:
        if e is not None:
            support[e] += 1
            t = _twin(ro, d, src, e)
            if t != e:
                support[t] += 1
    keys = []
    for r in range(len(po) - 1):
        for s in range(po[r], po[r + 1] - 1):  # step s + 1 is in the same read
            a, b = follow[s], follow[s + 1]
            if a is not None and b is not None and c[s] == ln[u[s] >> 1]:
                keys += [a << 32 | b, _twin(ro, d, src, b) << 32 | _twin(ro, d, src, a)]
    n_linked = sum(1 for x in f if x & LINKED)
    n_followed = sum(1 for e in follow if e is not None)
    return {"keys": np.array(keys, dtype=np.uint64), "edge_support": np.array(support, dtype=np.uint64), "n_followed": n_followed,
            "n_off_graph": sum(1 for s, x in enumerate(f) if x & LINKED and follow[s] is None), "n_linked": n_linked}


def count_keys(keys, min_count=1):
    """the span table of emitted keys: (keys strictly ascending, counts uint32)"""
    k, c = np.unique(np.asarray(keys, dtype=np.uint64), return_counts=True)
    sel = c >= min_count
    return k[sel], c[sel].astype(np.uint32)


def resolve_reference(row_off, dst, n_unitigs, span_keys, span_counts, min_support):
    """-> (resolved uint8 per unitig, partner uint32 per edge, n_candidates, n_resolved)"""
    ro, d = [int(x) for x in row_off], [int(x) for x in dst]
    src = _sources(ro)
    ms = max(int(min_support), 1)
    sup = {int(k): int(c) for k, c in zip(span_keys, span_counts)}
    strand, match, cand = [False] * (2 * n_unitigs), {}, [False] * (2 * n_unitigs)
    for V in range(2 * n_unitigs):
        ins = [_twin(ro, d, src, e) for e in range(ro[V ^ 1], ro[(V ^ 1) + 1])]
        outs = list(range(ro[V], ro[V + 1]))
        cand[V] = len(ins) >= 2 and len(outs) >= 2
        if not cand[V] or len(ins) != len(outs):
            continue
        if any(src[a] >> 1 == V >> 1 for a in ins) or any(d[b] >> 1 == V >> 1 for b in outs):
            continue
        by_in = {a: [b for b in outs if sup.get(a << 32 | b, 0) >= ms] for a in ins}
        by_out = {b: [a for a in ins if sup.get(a << 32 | b, 0) >= ms] for b in outs}
        if all(len(x) == 1 for x in by_in.values()) and all(len(x) == 1 for x in by_out.values()):
            strand[V] = True
            match[V] = {a: x[0] for a, x in by_in.items()}
    resolved = np.array([strand[2 * t] and strand[2 * t + 1] for t in range(n_unitigs)], dtype=np.uint8)
    partner = np.full(len(d), NONE, dtype=np.uint32)
    for V, m in match.items():
        if resolved[V >> 1]:
            for a, b in m.items():
                partner[a] = b
    n_cand = sum(1 for t in range(n_unitigs) if cand[2 * t] or cand[2 * t + 1])
    return resolved, partner, n_cand, int(resolved.sum())


def twins_of(row_off, dst):
    ro, d = [int(x) for x in row_off], [int(x) for x in dst]
    src = _sources(ro)
    return [_twin(ro, d, src, e) for e in range(len(d))]


def check_span_invariants(ref, ro, d, T, tag, min_support=1):
    """every key's twin follows it; the counted table is twin-symmetric; partner[tw(partner[a])] == tw(a); resolved is the same for
    both strands (the resolution of either strand alone agrees with the unitig's)"""
    tw = twins_of(ro, d)
    k = ref["keys"].tolist()
    assert len(k) % 2 == 0
    for x, y in zip(k[0::2], k[1::2]):
        assert y == tw[x & NONE] << 32 | tw[x >> 32] and x != y, tag
    sk, sc = count_keys(ref["keys"])
    table = dict(zip(sk.tolist(), sc.tolist()))
    for x, c in table.items():
        assert table[tw[x & NONE] << 32 | tw[x >> 32]] == c, tag
    resolved, partner, nc, nr = resolve_reference(ro, d, T, sk, sc, min_support)
    for a, b in enumerate(partner.tolist()):
        if b != NONE:
            assert partner[tw[b]] == tw[a] and resolved[d[a] >> 1], (tag, a, b)
    for t in range(T):  # a resolved unitig's in-edges on both strands all have partners; an unresolved one's none
        for V in (2 * t, 2 * t + 1):
            ins = [tw[e] for e in range(int(ro[V ^ 1]), int(ro[(V ^ 1) + 1]))]
            assert all((partner[a] != NONE) == bool(resolved[t]) for a in ins), (tag, V)
    return sk, sc, resolved, partner, nc, nr


# ---- hand-made: eight unitigs ---------------------------------------------------------------------------------------------------------
#  A = 0, B = 1 -> R = 2 -> C = 3, D = 4 (the X-shaped repeat); H = 5 with a hairpin H+ -> H-; L = 6, one member, with a loop; O = 7 circular
HAND_LEN = [2, 3, 3, 2, 1, 2, 1, 3]
HAND_EDGES = [(0, 4), (2, 4), (4, 6), (4, 8), (10, 11), (12, 12)]  # closed under twins by tu.csr_of
#  e0 A+>R+  e1 B+>R+  e2 R+>C+  e3 R+>D+  e4 R->A-  e5 R->B-  e6 C->R-  e7 D->R-  e8 H+>H- (its own twin)  e9 L+>L+  e10 L->L-
HAND_TWIN = [4, 5, 6, 7, 0, 1, 2, 3, 8, 10, 9]
L_ = LINKED
# name -> (steps (unitig, pos, count, flags), the edge each step follows, keys it emits as (a, b) pairs, off-graph steps)
HAND_READS = {
    "A-R-C": ([(0, 0, 2, 0), (4, 0, 3, L_), (6, 0, 2, L_)], [None, 0, 2], [(0, 2), (6, 4)], 0),
    "B-R-D, entering B in its middle": ([(2, 1, 2, 0), (4, 0, 3, L_), (8, 0, 1, L_)], [None, 1, 3], [(1, 3), (7, 5)], 0),
    "A-R-C on the other strand": ([(7, 0, 2, 0), (5, 0, 3, L_), (1, 0, 1, L_)], [None, 6, 4], [(6, 4), (0, 2)], 0),
    "B-R-D on the other strand": ([(9, 0, 1, 0), (5, 0, 3, L_), (3, 0, 2, L_)], [None, 7, 5], [(7, 5), (1, 3)], 0),
    "only part of R: an edge, no span": ([(0, 0, 2, 0), (4, 0, 2, L_), (6, 0, 2, L_)], [None, 0, None], [], 1),
    "a jump from the middle of A": ([(0, 0, 1, 0), (4, 0, 3, L_), (6, 0, 2, L_)], [None, None, 2], [], 1),
    "a first step never follows": ([(4, 0, 3, L_), (6, 0, 2, L_)], [None, 2], [], 1),
    "a gap before R": ([(0, 0, 2, 0), (4, 0, 3, 0), (6, 0, 2, L_)], [None, None, 2], [], 0),
    "a hairpin": ([(10, 0, 2, 0), (11, 0, 2, L_)], [None, 8], [], 0),
    "a loop on one member": ([(12, 0, 1, 0), (12, 0, 1, L_), (12, 0, 1, L_)], [None, 9, 9], [(9, 9), (10, 10)], 0),
    "a circular unitig": ([(14, 1, 2, 0), (14, 0, 3, L_)], [None, None], [], 1),
    "an empty read": ([], [], [], 0),
    "one step": ([(6, 0, 2, 0)], [None], [], 0),
}
HAND_EXTRA = {"A-R-D": ([(0, 0, 2, 0), (4, 0, 3, L_), (8, 0, 1, L_)], [None, 0, 3], [(0, 3), (7, 4)], 0)}
#            e0 e1 e2 e3 e4 e5 e6 e7 e8 e9 e10
HAND_SUPPORT = [3, 2, 5, 2, 3, 2, 5, 2, 1, 2, 2]
HAND_TABLE = {(0, 2): 2, (1, 3): 2, (6, 4): 2, (7, 5): 2, (9, 9): 1, (10, 10): 1}
HAND_PARTNER = [2, 3, NONE, NONE, NONE, NONE, 4, 5, NONE, NONE, NONE]


def hand_graph():
    ro, d = tu.csr_of(len(HAND_LEN), HAND_EDGES)
    return ro, d, np.concatenate([[0], np.cumsum(HAND_LEN)]).astype(np.uint64)


def paths_of(reads):
    """lists of (unitig, pos, count, flags) -> the path dict"""
    steps = [s for r in reads for s in r]
    out = {f: np.array([s[i] for s in steps], dtype=np.uint32) for i, f in enumerate(PATH)}
    out["path_off"] = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return out


def hand_paths(extra=False):
    cases = dict(HAND_READS, **(HAND_EXTRA if extra else {}))
    return paths_of([c[0] for c in cases.values()]), cases


def _keys(pairs):
    return [a << 32 | b for a, b in pairs]


# ---- generators -------------------------------------------------------------------------------------------------------------------
def walked_paths(rng, n_keys, lens, max_len=3, keep_edges=0.8):
    """random_unitigs / walk_items of test_thread.py -> thread_reference: a decomposition, the paths of reads that walk it, and a
    twin-symmetric CSR made of a random part of the transitions the paths make between unitigs (the rest go off-graph)"""
    keys, cnt = tg._random_table(rng, n_keys)
    uni = tt.random_unitigs(rng, len(keys), max_len=max_len, p_cycle=0.05)
    km_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    h, rv = tt.walk_items(rng, km_off, keys, uni, gap=0.02, jump=0.02)
    paths = tt.thread_reference(km_off, h, rv, keys, cnt, 1, tt.places_reference(uni), n_unitigs=uni["n_unitigs"])
    u, f = paths["unitig"].tolist(), paths["flags"].tolist()
    edges = [(u[s - 1], u[s]) for s in range(1, len(u)) if f[s] & LINKED and rng.random() < keep_edges]
    ro, d = tu.csr_of(uni["n_unitigs"], edges)
    return paths, ro, d, uni["uni_off"], uni["n_unitigs"]


def chained_paths(rng, T, read_lens, p_break=0.0, paired=False):
    """T unitigs of 1 .. 3 members, edges t+ -> (t + 1)+ and t+ -> (t + 2)+ round the ring; every read walks t, t + 1, .. from a random
    unitig, whole unitigs all linked, so that every inner step of a read spans; with probability p_break a step is cut short, is not
    linked, or is followed by a jump over two unitigs (no edge).  paired: a read takes the same kind of edge all along, so that
    the spans pair every unitig's in-edges with its out-edges one to one"""
    ln = (1 + np.arange(T) % 3).tolist()
    edges = [(2 * t, 2 * ((t + 1) % T)) for t in range(T)] + [(2 * t, 2 * ((t + 2) % T)) for t in range(T)]
    ro, d = tu.csr_of(T, edges)
    reads = []
    for n in read_lens:
        t, rev, steps, stride = int(rng.integers(0, T)), int(rng.integers(0, 2)), [], int(rng.integers(1, 3))
        for i in range(int(n)):
            U, cnt, fl, pos = 2 * t + rev, ln[t], LINKED if i else 0, 0
            x = rng.random()
            if x < p_break / 3:
                cnt, pos = max(ln[t] - 1, 1), int(rng.integers(0, 2))
            elif x < 2 * p_break / 3:
                fl = 0
            steps.append((U, pos, cnt, fl))
            t = (t + (-1 if rev else 1) * (3 if 2 * p_break / 3 <= x < p_break else stride if paired else 2 if rng.random() < 0.3 else 1)) % T
        reads.append(steps)
    return paths_of(reads), ro, d, np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64), T


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert "S2K_ABI_VERSION 2" in header and pkg.ABI_VERSION == 2
    assert hasattr(pkg.Engine, "paths_spans") and hasattr(pkg.Engine, "graph_resolve_mask")
    assert all(hasattr(pkg.UnitigGraph, f) for f in ("spans", "span_table", "resolve"))
    assert hasattr(pkg, "SpanTable") and hasattr(pkg, "write_spans")


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "span_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "span_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    T = pkg.ThreadOut  # the struct s2k_paths_spans reads its paths from
    assert facts["sizeof.s2k_thread_out"] == (ctypes.sizeof(T),)
    for f in ("path_off",) + PATH:
        assert facts["s2k_thread_out." + f] == (getattr(T, f).offset, ctypes.sizeof(dict(T._fields_)[f])), f
    assert facts["S2K_NO_PARTNER"] == (pkg.NO_PARTNER,) == (NONE,) and facts["S2K_STEP_LINKED"] == (pkg.STEP_LINKED,)


def test_cpp_span_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "span_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "span_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    mk = open(os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc", "Makefile")).read()
    assert "s2k_span.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))


def test_references_hand_made():
    ro, d, off = hand_graph()
    assert twins_of(ro, d) == HAND_TWIN and len(d) == 11
    paths, cases = hand_paths()
    ref = spans_reference(paths, ro, d, off)
    assert ref["keys"].tolist() == sum((_keys(c[2]) for c in cases.values()), [])
    assert ref["edge_support"].tolist() == HAND_SUPPORT
    assert ref["n_followed"] == sum(1 for c in cases.values() for e in c[1] if e is not None) == 15
    assert ref["n_off_graph"] == sum(c[3] for c in cases.values()) == 4 and ref["n_followed"] + ref["n_off_graph"] == ref["n_linked"]
    for name, c in cases.items():  # each read alone: the edge every step follows, from its support
        one = spans_reference(paths_of([c[0]]), ro, d, off)
        want = [0] * 11
        for e in c[1]:
            if e is not None:
                want[e] += 1
                want[HAND_TWIN[e]] += HAND_TWIN[e] != e
        assert one["edge_support"].tolist() == want and one["keys"].tolist() == _keys(c[2]) and one["n_off_graph"] == c[3], name
    sk, sc = count_keys(ref["keys"])
    assert dict(zip(sk.tolist(), sc.tolist())) == {a << 32 | b: c for (a, b), c in HAND_TABLE.items()}
    for ms in (0, 1, 2):  # A-R-C and B-R-D twice each: R is resolved
        resolved, partner, nc, nr = resolve_reference(ro, d, 8, sk, sc, ms)
        assert resolved.tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and partner.tolist() == HAND_PARTNER and (nc, nr) == (1, 1), ms
    assert resolve_reference(ro, d, 8, sk, sc, 3)[0].sum() == 0
    # one read A-R-D more: the matching is broken at min_support 1 and restored at 2
    paths, cases = hand_paths(extra=True)
    ref = spans_reference(paths, ro, d, off)
    assert ref["keys"].tolist()[-2:] == _keys([(0, 3), (7, 4)])
    sk, sc = count_keys(ref["keys"])
    resolved, partner, nc, nr = resolve_reference(ro, d, 8, sk, sc, 1)
    assert resolved.sum() == 0 and (partner == NONE).all() and (nc, nr) == (1, 0)
    resolved, partner, nc, nr = resolve_reference(ro, d, 8, sk, sc, 2)
    assert resolved.tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and partner.tolist() == HAND_PARTNER and (nc, nr) == (1, 1)
    check_span_invariants(ref, ro, d, 8, "hand", 2)


def test_write_spans_hand_made(tmp_path):
    ro, d, off = hand_graph()
    ref = spans_reference(hand_paths(extra=True)[0], ro, d, off)
    sk, sc = count_keys(ref["keys"])
    ek = np.array([s << 32 | int(v) for s, v in zip(_sources([int(x) for x in ro]), d)], dtype=np.uint64)
    p = str(tmp_path / "spans.tsv")
    pkg.write_spans(p, sk, sc, ek)
    assert open(p).read() == ">0\t>2\t>3\t2\n>0\t>2\t>4\t1\n>1\t>2\t>4\t2\n>6\t>6\t>6\t1\n"


def test_reference_random_decompositions_invariants():
    rng = np.random.default_rng(51)
    seen = [0, 0, 0]
    for n_keys, lens in ((40, [30, 0, 1, 25]), (300, [200] * 5), (600, list(rng.integers(0, 60, size=120))), (200, [900] * 6)):
        paths, ro, d, off, T = walked_paths(rng, n_keys, lens)
        ref = spans_reference(paths, ro, d, off)
        assert tu.is_twin_symmetric(ro, d, T) and ref["n_followed"] + ref["n_off_graph"] == ref["n_linked"]
        for ms in (1, 2):
            sk, sc, resolved, partner, nc, nr = check_span_invariants(ref, ro, d, T, (n_keys, ms), ms)
        seen = [seen[0] + len(ref["keys"]), seen[1] + ref["n_off_graph"], seen[2] + nc]
    for T, lens in ((9, [40] * 30), (50, [7] * 200)):  # few unitigs, many reads: junctions that the spans resolve
        paths, ro, d, off, T = chained_paths(rng, T, lens, p_break=0.1)
        ref = spans_reference(paths, ro, d, off)
        sk, sc, resolved, partner, nc, nr = check_span_invariants(ref, ro, d, T, ("chain", T), 1)
        assert nc == T and len(ref["keys"]) > 100
    paths, ro, d, off, T = chained_paths(rng, 30, [12] * 150, p_break=0.05, paired=True)
    ref = spans_reference(paths, ro, d, off)
    sk, sc, resolved, partner, nc, nr = check_span_invariants(ref, ro, d, T, "paired", 2)
    assert nc == T and 0 < nr
    assert seen[0] > 200 and seen[1] > 50 and seen[2] > 10, seen


# ---- the repeat fixture: two sequences that share R ------------------------------------------------------------------------------------
REPEAT = dict(l=12, k=5, d=0.05, min_count=2, flank=3000, repeat=600, read=2000, step=150, seed=3)


def repeat_reads(ecoli):
    """X1 + R + Y1 and X2 + R + Y2 from five disjoint slices of the genome, and error-free reads tiled over both, half of them
    reverse-complemented -> (reads, [S1, S2])"""
    c = REPEAT
    rng = np.random.default_rng(c["seed"])
    starts = np.sort(rng.choice(np.arange(0, len(ecoli) - c["flank"], c["flank"] + 500), size=5, replace=False)).tolist()
    x1, y1, x2, y2 = (bytes(ecoli[a: a + c["flank"]]) for a in starts[:4])
    R = bytes(ecoli[starts[4]: starts[4] + c["repeat"]])
    seqs = [x1 + R + y1, x2 + R + y2]
    reads = [s[a: a + c["read"]] for s in seqs for a in range(0, len(s) - c["read"] + 1, c["step"])]
    return [tg._revcomp(r) if rng.random() < 0.5 else r for r in reads], seqs


@pytest.fixture(scope="module")
def repeat_case(oracle, ecoli):
    """the fixture through the oracle and the references alone: graph, unitigs, paths, spans, resolution; and where the two whole
    sequences go through R"""
    c = REPEAT
    reads, seqs = repeat_reads(ecoli)
    mode = int(pkg.HashMode.Regular)
    b = oracle.batch(*pkg.pack_reads(reads), c["l"], c["k"], c["d"], mode)
    g = tg.graph_reference([b], c["min_count"], 1)
    uni, uro, ud, _ = ts.unitig_view(g)
    place = tt.places_reference(uni)
    T = uni["n_unitigs"]
    paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], g["keys"], g["counts"], c["min_count"], place, n_unitigs=T)
    ref = spans_reference(paths, uro, ud, uni["uni_off"])
    sk, sc = count_keys(ref["keys"])
    resolved, partner, nc, nr = resolve_reference(uro, ud, T, sk, sc, 2)
    sb = oracle.batch(*pkg.pack_reads(seqs), c["l"], c["k"], c["d"], mode)
    whole = tt.thread_reference(sb["km_off"], sb["hash"], sb["rev"], g["keys"], g["counts"], c["min_count"], place, n_unitigs=T)
    return {"reads": reads, "b": b, "g": g, "uni": uni, "uro": uro, "ud": ud, "T": T, "paths": paths, "ref": ref, "sk": sk, "sc": sc,
            "resolved": resolved, "partner": partner, "nc": nc, "nr": nr, "whole": whole}


def through_repeat(case):
    """the (in-edge, out-edge) by which each of the two whole sequences crosses the one unitig both visit -> (R, [(a1, b1), (a2, b2)])"""
    w, uro, ud = case["whole"], [int(x) for x in case["uro"]], [int(x) for x in case["ud"]]
    po, u = w["path_off"].tolist(), w["unitig"].tolist()
    shared = set(x >> 1 for x in u[po[0]:po[1]]) & set(x >> 1 for x in u[po[1]:po[2]])
    assert len(shared) == 1, shared  # the fixture's shape: R is one unitig, and nothing else is shared
    R = shared.pop()
    out = []
    for r in (0, 1):
        s = next(s for s in range(po[r] + 1, po[r + 1] - 1) if u[s] >> 1 == R)
        out.append((_find(uro, ud, u[s - 1], u[s]), _find(uro, ud, u[s], u[s + 1])))
    return R, out


def test_repeat_fixture_reference_resolves_r(repeat_case):
    """on the CPU, the references alone: R is a unitig with in = out = 2, the only candidate, and the spans pair (X1, Y1) and (X2, Y2)"""
    c = repeat_case
    R, ((a1, b1), (a2, b2)) = through_repeat(c)
    uro, T = c["uro"].astype(np.int64), c["T"]
    assert None not in (a1, b1, a2, b2) and a1 != a2 and b1 != b2
    for V in (2 * R, 2 * R + 1):
        assert uro[V + 1] - uro[V] == 2 and uro[(V ^ 1) + 1] - uro[V ^ 1] == 2
    assert c["ref"]["n_off_graph"] == 0 and c["ref"]["n_followed"] == c["ref"]["n_linked"] > 20
    assert c["resolved"].tolist() == [int(t == R) for t in range(T)] and (c["nc"], c["nr"]) == (1, 1)
    assert c["partner"][a1] == b1 and c["partner"][a2] == b2 and int((c["partner"] != NONE).sum()) == 4
    table = dict(zip(c["sk"].tolist(), c["sc"].tolist()))
    assert table[a1 << 32 | b1] >= 2 and table[a2 << 32 | b2] >= 2 and (a1 << 32 | b2) not in table and (a2 << 32 | b1) not in table
    check_span_invariants(c["ref"], c["uro"], c["ud"], T, "repeat", 2)
    print("repeat fixture: %d reads, %d nodes, %d unitigs, R = unitig %d of %d members, %d span keys" % (
        len(c["reads"]), len(c["g"]["keys"]), T, R, int(c["uni"]["uni_off"][R + 1] - c["uni"]["uni_off"][R]), len(c["ref"]["keys"])))


MODES = [(pkg.HashMode.Regular, 12, 5), (pkg.HashMode.Hpc, 21, 3)]


def ecoli_reference_paths(oracle, ecoli, mode, l, k, mc=2):
    """the 600 E. coli reads of test_simplify.py (0.5 % substitutions, half reverse-complemented) through the references"""
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    b = oracle.batch(*pkg.pack_reads(reads), l, k, 0.05, int(mode))
    g = tg.graph_reference([b], mc, 1)
    uni, uro, ud, _ = ts.unitig_view(g)
    paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], g["keys"], g["counts"], mc, tt.places_reference(uni), n_unitigs=uni["n_unitigs"])
    return reads, b, g, uni, uro, ud, paths


@pytest.mark.parametrize("mode,l,k", MODES)
def test_oracle_ecoli_reads_reference_invariants(oracle, ecoli, mode, l, k):
    """the 600 E. coli reads and the graph they were built from, unsimplified, min_edge_count 1: the read support of every edge is its
    count (two independent routes), every linked step follows an edge"""
    mc = 2
    reads, b, g, uni, uro, ud, paths = ecoli_reference_paths(oracle, ecoli, mode, l, k)
    ref = spans_reference(paths, uro, ud, uni["uni_off"])
    edge_counts = g["edge_counts"][uni["src_edge"].astype(np.int64)]
    assert ref["edge_support"].tobytes() == edge_counts.astype(np.uint64).tobytes() and len(edge_counts) > 20
    assert ref["n_off_graph"] == 0 and ref["n_followed"] == ref["n_linked"] > 100
    check_span_invariants(ref, uro, ud, uni["n_unitigs"], ("ecoli", mode), 2)
    print("min_count %d: %d unitigs, %d edges, %d followed, %d span keys" % (mc, uni["n_unitigs"], len(ud), ref["n_followed"], len(ref["keys"])))


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
    return bool((h[frm:].view(np.int64 if h.dtype.itemsize == 8 else np.int32 if h.dtype.itemsize == 4 else np.uint8) ==
                 (MARK if h.dtype.itemsize > 1 else 0xA5)).all())


def raw_spans(eng, paths, ro, d, off, T=None, n_edges=None, n_steps=None, n_reads=None, capacity=None, keys_out=True, support=None, null=(), front=0,
              ctx=True):
    """s2k_paths_spans through ctypes, guard words behind (and `front` before) the keys -> (status, n_keys, n_followed, n_off_graph,
    host keys with guards).  support: an int64 GPU tensor; null: names of path arrays, or row_off / dst / uni_off, to pass as NULL"""
    import torch

    T = len(off) - 1 if T is None else T
    ns = len(paths["unitig"]) if n_steps is None else n_steps
    nr = len(paths["path_off"]) - 1 if n_reads is None else n_reads
    dp = {f: _dev(paths[f], np.uint32) for f in PATH}
    dp["path_off"] = _dev(paths["path_off"], np.uint64)
    o = pkg.ThreadOut()
    o.capacity = ns
    for f, t in dp.items():
        if f not in null:
            setattr(o, f, t.data_ptr())
    dro, dd, doff = _dev(ro, np.uint64), _dev(d, np.uint32), _dev(off, np.uint64)
    cap = 2 * ns if capacity is None else capacity
    keys = torch.full((cap + front + GUARD,), MARK, dtype=torch.int64, device="cuda:0")
    nk, nf, no = ctypes.c_uint64(777), ctypes.c_uint64(777), ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_paths_spans(eng.ctx if ctx else None, nr, None if "paths" in null else ctypes.byref(o), ns, _ptr(dro, "row_off" in null),
                                _ptr(dd, "dst" in null or len(d) == 0), len(d) if n_edges is None else n_edges, _ptr(doff, "uni_off" in null), T,
                                ctypes.c_void_p(keys.data_ptr() + 8 * front) if keys_out else None, cap, None if support is None else _ptr(support),
                                ctypes.byref(nk), ctypes.byref(nf), ctypes.byref(no))
    return s, nk.value, nf.value, no.value, _host(keys, np.uint64)


def raw_resolve(eng, ro, d, T, sk, sc, ms, n_edges=None, n_spans=None, null=(), ctx=True):
    """s2k_graph_resolve_mask through ctypes, guards behind both outputs -> (status, n_candidates, n_resolved, resolved, partner)"""
    import torch

    dro, dd, dk, dc = _dev(ro, np.uint64), _dev(d, np.uint32), _dev(sk, np.uint64), _dev(sc, np.uint32)
    res = torch.full((T + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    par = torch.full((len(d) + GUARD,), MARK, dtype=torch.int32, device="cuda:0")
    nc, nr = ctypes.c_uint64(777), ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_graph_resolve_mask(eng.ctx if ctx else None, _ptr(dro, "row_off" in null), _ptr(dd, "dst" in null or len(d) == 0),
                                       len(d) if n_edges is None else n_edges, T, _ptr(dk, "keys" in null or len(sk) == 0),
                                       _ptr(dc, "counts" in null or len(sk) == 0), len(sk) if n_spans is None else n_spans, ms,
                                       _ptr(res, "resolved" in null), _ptr(par, "partner" in null), ctypes.byref(nc), ctypes.byref(nr))
    return s, nc.value, nr.value, _host(res, np.uint8), _host(par, np.uint32)


def device_spans(eng, paths, ro, d, off, tag, front=0):
    """the call against the reference: keys, totals, edge support, guards untouched; the sizes-only call; then the resolution of the
    counted keys at min_support 1 and 2 -> the reference"""
    import torch

    ref = spans_reference(paths, ro, d, off)
    n = len(ref["keys"])
    sup = torch.zeros(max(len(d), 1), dtype=torch.int64, device="cuda:0")
    s, nk, nf, no, keys = raw_spans(eng, paths, ro, d, off, capacity=n, support=sup, front=front)
    assert (s, nk, nf, no) == (0, n, ref["n_followed"], ref["n_off_graph"]), (tag, s, nk, nf, no, n, ref["n_followed"], ref["n_off_graph"])
    assert keys[front: front + n].tobytes() == ref["keys"].tobytes(), (tag, "keys", keys[front: front + n][:8], ref["keys"][:8])
    assert _marked(keys, front + n) and _marked(keys[:front]), (tag, "guard")
    assert sup.cpu().numpy().view(np.uint64)[:len(d)].tobytes() == ref["edge_support"].tobytes(), (tag, "edge_support")
    s, nk, nf, no, keys = raw_spans(eng, paths, ro, d, off, keys_out=False)
    assert (s, nk, nf, no) == (0, n, ref["n_followed"], ref["n_off_graph"]) and _marked(keys), (tag, "sizes")
    T = len(off) - 1
    sk, sc = count_keys(ref["keys"])
    for ms in (1, 2):
        device_resolve(eng, ro, d, T, sk, sc, ms, (tag, ms))
    return ref


def device_resolve(eng, ro, d, T, sk, sc, ms, tag):
    want = resolve_reference(ro, d, T, sk, sc, ms)
    s, nc, nr, res, par = raw_resolve(eng, ro, d, T, sk, sc, ms)
    assert (s, nc, nr) == (0, want[2], want[3]), (tag, s, nc, nr, want[2:])
    assert res[:T].tobytes() == want[0].tobytes() and _marked(res, T), (tag, "resolved")
    assert par[:len(d)].tobytes() == want[1].tobytes() and _marked(par, len(d)), (tag, "partner")
    s, nc, nr, res, par = raw_resolve(eng, ro, d, T, sk, sc, ms, null=("resolved", "partner"))  # the totals only
    assert (s, nc, nr) == (0, want[2], want[3]) and _marked(res) and _marked(par), (tag, "totals only")
    return want


@pytest.mark.gpu
def test_device_hand_made(eng):
    ro, d, off = hand_graph()
    for extra in (False, True):
        paths, cases = hand_paths(extra)
        ref = device_spans(eng, paths, ro, d, off, ("hand", extra))
        sk, sc = count_keys(ref["keys"])
        for ms, want in ((0, not extra), (1, not extra), (2, True), (3, False)):
            got = device_resolve(eng, ro, d, 8, sk, sc, ms, ("hand", extra, ms))
            assert got[0].tolist() == [0, 0, int(want), 0, 0, 0, 0, 0] and got[1].tolist() == (HAND_PARTNER if want else [NONE] * 11)
    for name, c in HAND_READS.items():  # every read alone
        device_spans(eng, paths_of([c[0]]), ro, d, off, name)


@pytest.mark.gpu
def test_device_random_decompositions_and_read_shapes(eng):
    """reads that walk random decompositions, with gaps, jumps, empty and one-step reads, over a CSR that holds a part of their
    transitions; and chains of whole unitigs with steps cut short, not linked, or off the graph"""
    rng = np.random.default_rng(52)
    n_keys = 0
    for nk, lens in ((40, [30, 0, 1, 25, 0, 0, 1, 1]), (300, [200] * 5 + [0, 1, 2]), (900, list(rng.integers(0, 60, size=150))), (300, [2500, 0, 2500])):
        paths, ro, d, off, T = walked_paths(rng, nk, lens)
        ref = device_spans(eng, paths, ro, d, off, ("walked", nk), front=nk % 2)
        n_keys += len(ref["keys"])
        assert nk < 100 or 200 <= len(paths["unitig"]) <= 5000
    for T, lens in ((9, [40] * 30), (50, [7] * 200 + [0, 1, 2, 3] * 20), (400, list(rng.integers(0, 30, size=300)))):
        paths, ro, d, off, T = chained_paths(rng, T, lens, p_break=0.15)
        ref = device_spans(eng, paths, ro, d, off, ("chained", T), front=T % 2)
        n_keys += len(ref["keys"])
    resolved = 0
    for T, lens, pb in ((30, [12] * 150, 0.05), (300, [15] * 300, 0.0), (7, [9] * 40, 0.02)):  # junctions that the spans resolve, some of them
        paths, ro, d, off, T = chained_paths(rng, T, lens, p_break=pb, paired=True)
        ref = device_spans(eng, paths, ro, d, off, ("paired", T))
        resolved += resolve_reference(ro, d, T, *count_keys(ref["keys"]), 2)[3]
    assert n_keys > 3000 and resolved > 30


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", [2047, 2048, 2049, 4097])
def test_device_tile_edges(eng, n_steps):
    """tiles hold 2 048 steps.  One read over all the steps: the spans at steps 2 047 (its successor in the next tile) and 2 048 (its
    predecessor in the tile before) exist where the steps do; then reads cut so that one starts at a tile's first step, one at its
    last, one at the step after it, and with every alignment of the key run"""
    rng = np.random.default_rng(n_steps)
    for cuts in ([], [5], [2047], [2048], [1, 2049], [2046, 2048, 4096]):
        cuts = [0] + [x for x in cuts if x < n_steps] + [n_steps]
        lens = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
        for p_break in (0.0, 0.1):
            paths, ro, d, off, T = chained_paths(rng, 37, lens, p_break)
            assert len(paths["unitig"]) == n_steps
            ref = device_spans(eng, paths, ro, d, off, (n_steps, lens, p_break), front=int(p_break > 0))
            if p_break == 0.0:  # every inner step of a read spans
                assert len(ref["keys"]) == 2 * sum(max(x - 2, 0) for x in lens)


@pytest.mark.gpu
def test_device_sizes_capacity_refusals_and_batches(eng):
    import torch

    rng = np.random.default_rng(53)
    paths, ro, d, off, T = chained_paths(rng, 60, list(rng.integers(0, 40, size=200)), p_break=0.1)
    ref = spans_reference(paths, ro, d, off)
    n, ne, ns, nr = len(ref["keys"]), len(d), len(paths["unitig"]), len(paths["path_off"]) - 1
    assert n > 1000 and ns > 2048
    sup = torch.zeros(ne, dtype=torch.int64, device="cuda:0")
    for cap in (n - 1, 0):  # short: S2K_ERR_CAPACITY, the totals still set, nothing written, the support untouched
        s, nk, nf, no, keys = raw_spans(eng, paths, ro, d, off, capacity=cap, support=sup)
        assert (s, nk, nf, no) == (7, n, ref["n_followed"], ref["n_off_graph"]) and _marked(keys) and int(sup.sum()) == 0, cap
    # two batches (the reads split in two) == one: the keys concatenated, the support accumulated
    half = nr // 2
    got = []
    for lo, hi in ((0, half), (half, nr)):
        a, b = int(paths["path_off"][lo]), int(paths["path_off"][hi])
        part = {f: paths[f][a:b] for f in PATH}
        part["path_off"] = paths["path_off"][lo:hi + 1] - paths["path_off"][lo]
        s, nk, nf, no, keys = raw_spans(eng, part, ro, d, off, support=sup)
        assert s == 0
        got.append(keys[:nk])
    assert np.concatenate(got).tobytes() == ref["keys"].tobytes() and sup.cpu().numpy().view(np.uint64).tobytes() == ref["edge_support"].tobytes()

    def refused(code=1, **kw):
        args = dict(paths=paths, ro=ro, d=d, off=off, support=sup)
        args.update(kw)
        before = sup.clone()
        s, nk, nf, no, keys = raw_spans(eng, **args)
        assert (s, nk, nf, no) == (code, 0, 0, 0) and _marked(keys) and bool((sup == before).all()), (s, nk, nf, no, list(kw))

    refused(ctx=False)
    for f in ("paths", "path_off", "row_off", "dst", "uni_off") + PATH:
        refused(null=(f,))
    for r, v in ((0, 1), (5, 10 ** 9), (nr, ns - 1), (nr, ns + 1)):  # path_off: not from 0, decreasing, not ending at n_steps
        x = dict(paths, path_off=paths["path_off"].copy())
        x["path_off"][r] = v
        refused(paths=x)
    for v in (2 * T, 2 ** 32 - 1):  # a step on a unitig that does not exist
        x = dict(paths, unitig=paths["unitig"].copy())
        x["unitig"][ns // 2] = v
        refused(paths=x)
    refused(T=T - 1)
    for i, v in ((0, 1), (7, int(ro[8]) + 1), (2 * T, ne - 1), (2 * T, ne + 1)):  # row_off: not from 0, decreasing, not ending at n_edges
        x = ro.copy()
        x[i] = v
        refused(ro=x)
    x = d.copy()
    x[ne // 2] = 2 * T
    refused(d=x)
    x = off.copy()  # a unitig without a member
    x[11] = x[10]
    refused(off=x)
    z = ctypes.c_uint64(5)
    o = pkg.ThreadOut()
    o.path_off = 16
    assert eng.lib.s2k_paths_spans(eng.ctx, 1, ctypes.byref(o), 0, ctypes.c_void_p(16), ctypes.c_void_p(16), 2 ** 32, ctypes.c_void_p(16), 1, None, 0, None,
                                   ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == 1 and z.value == 0  # before anything is read
    assert eng.lib.s2k_paths_spans(eng.ctx, 1, ctypes.byref(o), 0, ctypes.c_void_p(16), None, 0, ctypes.c_void_p(16), 2 ** 31, None, 0, None,
                                   ctypes.byref(z), ctypes.byref(z), ctypes.byref(z)) == 1
    # no steps at all, and no reads
    empty = paths_of([[], [], []])
    s, nk, nf, no, keys = raw_spans(eng, empty, ro, d, off)
    assert (s, nk, nf, no) == (0, 0, 0, 0) and _marked(keys)
    s, nk, nf, no, keys = raw_spans(eng, paths_of([]), ro, d, off)
    assert (s, nk, nf, no) == (0, 0, 0, 0) and _marked(keys)

    # the resolution's refusals: nothing written
    sk, sc = count_keys(ref["keys"])
    want = resolve_reference(ro, d, T, sk, sc, 1)

    def refused_resolve(**kw):
        args = dict(ro=ro, d=d, T=T, sk=sk, sc=sc, ms=1)
        args.update(kw)
        s, nc, nr_, res, par = raw_resolve(eng, **args)
        assert (s, nc, nr_) == (1, 0, 0) and _marked(res) and _marked(par), (s, nc, nr_, list(kw))

    refused_resolve(ctx=False)
    for f in ("row_off", "dst", "keys", "counts"):
        refused_resolve(null=(f,))
    x = sk.copy()  # not strictly ascending: equal, then descending
    x[5] = x[4]
    refused_resolve(sk=x)
    x = sk.copy()
    x[[4, 5]] = x[[5, 4]]
    refused_resolve(sk=x)
    x = sk.copy()  # an in half / an out half that is no edge
    x[-1] = np.uint64(ne) << np.uint64(32) | (x[-1] & np.uint64(NONE))
    refused_resolve(sk=x)
    x = sk.copy()
    x[-1] = (x[-1] >> np.uint64(32)) << np.uint64(32) | np.uint64(ne)
    refused_resolve(sk=x)
    a = int(sk[0] >> np.uint64(32))  # an out-edge that does not leave the unitig its in-edge enters
    V = int(d[a])
    wrong = int(ro[V + 1]) % ne if int(ro[V + 1]) < ne else int(ro[V]) - 1
    x = np.sort(np.concatenate([sk[1:], [np.uint64(a << 32 | wrong)]]))
    refused_resolve(sk=x)
    y = ro.copy()
    y[2 * T] = ne + 1
    refused_resolve(ro=y)
    y = d.copy()
    y[3] = 2 * T
    refused_resolve(d=y)
    assert eng.lib.s2k_graph_resolve_mask(eng.ctx, ctypes.c_void_p(16), ctypes.c_void_p(16), 2 ** 32, 1, None, None, 0, 1, None, None, ctypes.byref(z),
                                          ctypes.byref(z)) == 1 and z.value == 0
    s, nc, nr_, res, par = raw_resolve(eng, ro, d, T, sk[:0], sc[:0], 1)  # no spans: candidates, nothing resolved
    assert (s, nc, nr_) == (0, want[2], 0) and not res[:T].any() and (par[:ne] == NONE).all() and _marked(res, T) and _marked(par, ne)


@pytest.mark.gpu
def test_device_deterministic(eng):
    import torch

    rng = np.random.default_rng(54)
    paths, ro, d, off, T = chained_paths(rng, 500, list(rng.integers(0, 200, size=300)), p_break=0.1)
    runs = []
    for _ in range(2):
        sup = torch.zeros(len(d), dtype=torch.int64, device="cuda:0")
        s, nk, nf, no, keys = raw_spans(eng, paths, ro, d, off, support=sup)
        assert s == 0 and nk > 10000
        sk, sc = count_keys(keys[:nk])
        r = raw_resolve(eng, ro, d, T, sk, sc, 2)
        assert r[0] == 0
        runs.append(keys.tobytes() + sup.cpu().numpy().tobytes() + r[3].tobytes() + r[4].tobytes() + bytes(str((nk, nf, no, r[1], r[2])), "ascii"))
    assert runs[0] == runs[1]


def _same_graph(ug, uro, ud, uni):
    assert tg._u64(ug.row_off).tobytes() == uro.tobytes() and ug.dst.cpu().numpy().view(np.uint32).tobytes() == ud.tobytes()
    assert tg._u64(ug.uni_off).tobytes() == uni["uni_off"].tobytes()


def _device_chain(eng, outs, nr, graph, mc, uro, ud, uni, ref_paths, tag, batches=1):
    """unitigs -> thread -> spans -> span table -> resolve on the device, every array against the references -> (ug, resolved, partner,
    stats, span table)"""
    import torch

    ug = graph.unitigs(eng)
    _same_graph(ug, uro, ud, uni)
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, outs, nr, min_count=mc)
    table.close()
    got = paths.host()
    for f in ("path_off",) + PATH:
        assert got[f].tobytes() == ref_paths[f].tobytes(), (tag, f)
    ref = spans_reference(ref_paths, uro, ud, uni["uni_off"])
    sup = torch.zeros(ug.n_edges, dtype=torch.int64, device="cuda:0")
    keys, (nf, no) = ug.spans(eng, paths, edge_support=sup)
    assert tg._u64(keys).tobytes() == ref["keys"].tobytes() and (nf, no) == (ref["n_followed"], ref["n_off_graph"]), (tag, nf, no)
    assert sup.cpu().numpy().view(np.uint64).tobytes() == ref["edge_support"].tobytes(), (tag, "edge_support")
    st = ug.span_table(eng, [paths] * batches)
    sk, sc = count_keys(ref["keys"])
    assert tg._u64(st.keys).tobytes() == sk.tobytes() and st.counts.cpu().numpy().view(np.uint32).tobytes() == (sc * batches).astype(np.uint32).tobytes()
    resolved, partner, stats = ug.resolve(eng, st, min_support=2 * batches)
    want = resolve_reference(uro, ud, ug.n_unitigs, sk, sc, 2)
    assert resolved.cpu().numpy().tobytes() == want[0].tobytes() and partner.cpu().numpy().view(np.uint32).tobytes() == want[1].tobytes(), tag
    assert stats == {"candidates": want[2], "resolved": want[3]}, (tag, stats, want[2:])
    return ug, ref, sup, want, st


@pytest.mark.gpu
def test_repeat_fixture_end_to_end(eng, repeat_case, tmp_path):
    """extract -> count -> graph -> unitigs -> thread -> spans -> span table -> resolve on the device: equal to the references, and R
    is resolved into (X1, Y1) and (X2, Y2)"""
    c = repeat_case
    outs = tt._extract_se(eng, c["reads"], REPEAT["l"], REPEAT["k"], REPEAT["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=REPEAT["min_count"], min_edge_count=1)
    tg._assert_graph(tg._graph_host(graph), c["g"], "repeat")
    ug, ref, sup, want, st = _device_chain(eng, outs, len(c["reads"]), graph, REPEAT["min_count"], c["uro"], c["ud"], c["uni"], c["paths"], "repeat", batches=2)
    assert sup.cpu().numpy().view(np.uint32)[::2].tobytes() == ug.edge_counts.cpu().numpy().view(np.uint32).tobytes()
    R, ((a1, b1), (a2, b2)) = through_repeat(c)
    assert want[0].tolist() == [int(t == R) for t in range(ug.n_unitigs)] and want[1][a1] == b1 and want[1][a2] == b2
    p = str(tmp_path / "spans.tsv")
    st.write(p, ug.edge_keys)
    lines = [x.split("\t") for x in open(p).read().split("\n")[:-1]]
    assert len(lines) == st.n_spans // 2 and sum(1 for x in lines if x[1] in (">%d" % R, "<%d" % R)) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("mode,l,k", MODES)
def test_ecoli_edge_support_equals_edge_counts(eng, oracle, ecoli, mode, l, k):
    """the 600 E. coli reads through the graph they built (unsimplified, min_edge_count 1): the device's d_edge_support equals the
    graph's edge counts entry for entry, and nothing is off-graph"""
    mc = 2
    reads, b, g, uni, uro, ud, ref_paths = ecoli_reference_paths(oracle, ecoli, mode, l, k)
    outs = tt._extract_se(eng, reads, l, k, 0.05, mode)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=mc, min_edge_count=1)
    ug, ref, sup, want, st = _device_chain(eng, outs, len(reads), graph, mc, uro, ud, uni, ref_paths, ("ecoli", int(mode)))
    assert sup.cpu().numpy().view(np.uint32)[::2].tobytes() == ug.edge_counts.cpu().numpy().view(np.uint32).tobytes() and ug.n_edges > 20
    assert not sup.cpu().numpy().view(np.uint32)[1::2].any() and ref["n_off_graph"] == 0


@pytest.mark.gpu
def test_ecoli_reads_with_errors_through_the_simplified_graph(eng, oracle, ecoli):
    """the 600 reads with 0.5 % substitutions through simplify(10, 20): device == reference; the edges of removed branches go
    off-graph, as many as the reference says"""
    mc = 2
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    b = oracle.batch(*pkg.pack_reads(reads), 12, 5, 0.05, int(pkg.HashMode.Regular))
    outs = tt._extract_se(eng, reads, 12, 5, 0.05, pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=mc, min_edge_count=1)
    sg, _, _ = graph.simplify(eng, 10, 20)
    final, _, _ = ts.simplify_rounds_reference(tg.graph_reference([b], mc, 1), 10, 20)
    tg._assert_graph(tg._graph_host(sg), final, "simplified")
    uni, uro, ud, _ = ts.unitig_view(final)
    ref_paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], final["keys"], final["counts"], mc, tt.places_reference(uni), n_unitigs=uni["n_unitigs"])
    ug, ref, sup, want, st = _device_chain(eng, outs, len(reads), sg, mc, uro, ud, uni, ref_paths, "simplified")
    print("simplified: %d unitigs, %d edges, %d followed, %d off-graph, %d span keys, %d candidates, %d resolved" % (
        ug.n_unitigs, ug.n_edges, ref["n_followed"], ref["n_off_graph"], len(ref["keys"]), want[2], want[3]))
    assert ref["n_followed"] > 100
