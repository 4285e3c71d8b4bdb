"""Untangling: resolved unitigs duplicated, the untangled graph compacted again, its contigs expanded to node members --
s2k_graph_untangle and s2k_unitig_expand (include/s2k.h).  The references are `untangle_reference` and
`expand_reference`, serial Python written from the header's definitions.  `untangle_reference` does not use the closed form jA / jB of
the kernel: for every resolved unitig and every j it makes the copy and re-routes a_j, partner[a_j] and their twins to it, then sorts
the keys -- two independent routes.  The device's arrays equal theirs byte for byte, every one of them, in every test."""
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
from test_span import repeat_case  # noqa: F401  (the module-scoped fixture of the repeat)

pkg = import_package()

SYMS = ("s2k_graph_untangle", "s2k_unitig_expand")
NONE = 0xFFFFFFFF
M32 = np.uint64(NONE)
UNT = (("copy_off", np.uint64), ("origin", np.uint32), ("copy_count", np.uint64), ("keys", np.uint64), ("src_edge", np.uint64))
EXP = (("uni_off", np.uint64), ("members", np.uint32), ("node_unitig", np.uint32), ("node_pos", np.uint32), ("circular", np.uint8),
       ("node_origin", np.uint32))


# ---- the references ----------------------------------------------------------------------------------------------------------------
def untangle_reference(row_off, dst, T, resolved, partner, cnt=None, ec=None):
    """-> dict copy_off, origin, copy_count (None without cnt and ec), keys, src_edge, n_copies, n_duplicated"""
    ro, d = [int(x) for x in row_off], [int(x) for x in dst]
    src = tsp._sources(ro)
    tw = [tsp._twin(ro, d, src, e) for e in range(len(d))]
    res, par = [int(x) for x in resolved], [int(x) for x in partner]
    copy_off = [0]
    for t in range(T):
        copy_off.append(copy_off[-1] + (ro[2 * t + 1] - ro[2 * t] if res[t] else 1))
    origin = [t for t in range(T) for _ in range(copy_off[t], copy_off[t + 1])]
    # every end of every edge starts at copy 0 of its unitig; the ends at a resolved unitig are then re-routed, each exactly once
    new_a = [2 * copy_off[src[e] >> 1] + (src[e] & 1) for e in range(len(d))]
    new_b = [2 * copy_off[d[e] >> 1] + (d[e] & 1) for e in range(len(d))]
    routed_a, routed_b = [0] * len(d), [0] * len(d)
    count = None if cnt is None or ec is None else [int(cnt[t]) for t in origin]
    for t in range(T):
        if not res[t]:
            continue
        base, deg = ro[2 * t + 1], ro[2 * t + 2] - ro[2 * t + 1]
        ins = [tw[base + j] for j in range(deg)]
        for j in range(deg):
            c = copy_off[t] + j
            leaves_rev, a = base + j, ins[j]
            b = par[a]
            enters_rev = tw[b]
            assert src[leaves_rev] == 2 * t + 1 and d[a] == 2 * t and src[b] == 2 * t and d[enters_rev] == 2 * t + 1
            new_a[leaves_rev], new_b[a], new_a[b], new_b[enters_rev] = 2 * c + 1, 2 * c, 2 * c, 2 * c + 1
            for lst, e in ((routed_a, leaves_rev), (routed_b, a), (routed_a, b), (routed_b, enters_rev)):
                lst[e] += 1
            if count is not None:
                S = sum(int(ec[x]) for x in ins)
                count[c] = int(cnt[t]) * int(ec[a]) // S if S else 0
    for e in range(len(d)):  # an end is re-routed iff its unitig is resolved
        assert routed_a[e] == res[src[e] >> 1] and routed_b[e] == res[d[e] >> 1], e
    order = sorted(range(len(d)), key=lambda e: (new_a[e], new_b[e]))
    return {"copy_off": np.array(copy_off, dtype=np.uint64), "origin": np.array(origin, dtype=np.uint32),
            "copy_count": None if count is None else np.array(count, dtype=np.uint64),
            "keys": np.array([new_a[e] << 32 | new_b[e] for e in order], dtype=np.uint64), "src_edge": np.array(order, dtype=np.uint64),
            "n_copies": copy_off[-1], "n_duplicated": sum(res)}


def expand_reference(outer, origin, inner):
    """outer / inner: dicts with uni_off, members, circular -> dict of the EXP arrays and n_members"""
    oo, om = [int(x) for x in outer["uni_off"]], [int(x) for x in outer["members"]]
    io, im = [int(x) for x in inner["uni_off"]], [int(x) for x in inner["members"]]
    members, node_origin, node_unitig, node_pos, uni_off, circular = [], [], [], [], [0], []
    for t in range(len(oo) - 1):
        pos = 0
        for C in om[oo[t]: oo[t + 1]]:
            u = int(origin[C >> 1])
            piece = im[io[u]: io[u + 1]]
            for x in ([y ^ 1 for y in reversed(piece)] if C & 1 else piece):
                members.append(2 * len(members) + (x & 1))
                node_origin.append(x >> 1)
                node_unitig.append(t)
                node_pos.append(pos)
                pos += 1
        uni_off.append(len(members))
        alone = oo[t + 1] - oo[t] == 1
        circular.append(int(bool(outer["circular"][t]) or (alone and bool(inner["circular"][int(origin[om[oo[t]] >> 1])]))))
    out = {"uni_off": uni_off, "members": members, "node_unitig": node_unitig, "node_pos": node_pos, "circular": circular, "node_origin": node_origin}
    out = {f: np.array(out[f], dtype=dt) for f, dt in EXP}
    out["n_members"] = len(members)
    return out


def csr_of_keys(keys, n):
    ro = np.searchsorted(keys >> np.uint64(32), np.arange(2 * n + 1, dtype=np.uint64), side="left").astype(np.uint64)
    return ro, (keys & M32).astype(np.uint32)


def contigs_reference(case):
    """what UnitigGraph.untangle computes, from the references -> dict: u (untangle), ro / d (the CSR over the copies), o (its unitigs),
    x (the expansion), counts, edge_keys, edge_counts, and the CSR over the oriented contigs"""
    u = untangle_reference(case["ro"], case["d"], case["T"], case["resolved"], case["partner"], case["cnt"], case["ec"])
    ro2, d2 = csr_of_keys(u["keys"], u["n_copies"])
    o = tu.unitig_reference(ro2, d2, u["n_copies"])
    x = expand_reference(o, u["origin"], case["inner"])
    csum = np.concatenate([[0], np.cumsum(u["copy_count"][o["members"] >> 1].astype(np.uint64))]).astype(np.uint64)
    off = o["uni_off"].astype(np.int64)
    ec = np.asarray(case["ec"], dtype=np.uint32)[u["src_edge"].astype(np.int64)][o["src_edge"].astype(np.int64)]
    cro, cd = tu.compacted_csr(o)
    return {"u": u, "ro": ro2, "d": d2, "o": o, "x": x, "counts": csum[off[1:]] - csum[off[:-1]], "edge_keys": o["edge_keys"], "edge_counts": ec,
            "cro": cro, "cd": cd}


def check_invariants(case, r, tag):
    """the invariants of every reference output"""
    ro, d, T, res = [int(x) for x in case["ro"]], [int(x) for x in case["d"]], case["T"], case["resolved"]
    u, src = r["u"], tsp._sources([int(x) for x in case["ro"]])
    keys, se, origin = u["keys"], u["src_edge"].astype(np.int64), u["origin"].astype(np.int64)
    assert (keys[1:] > keys[:-1]).all(), tag  # strictly ascending
    assert sorted(se.tolist()) == list(range(len(d))), tag  # a permutation of the old edges
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & M32).astype(np.int64)
    assert (2 * origin[a >> 1] + (a & 1)).tolist() == [src[e] for e in se] and (2 * origin[b >> 1] + (b & 1)).tolist() == [d[e] for e in se], tag
    assert tu.is_twin_symmetric(r["ro"], r["d"], u["n_copies"]), tag
    out_deg = np.diff(r["ro"].astype(np.int64))
    for c, t in enumerate(origin.tolist()):
        if res[t]:
            assert out_deg[2 * c] == out_deg[2 * c + 1] == 1, (tag, c)  # in(C) == out(C ^ 1) in a twin-symmetric graph
    if u["copy_count"] is not None:
        for t in range(T):
            got = int(u["copy_count"][int(u["copy_off"][t]): int(u["copy_off"][t + 1])].sum())
            deg = int(u["copy_off"][t + 1] - u["copy_off"][t])
            assert int(case["cnt"][t]) - (deg - 1 if res[t] else 0) <= got <= int(case["cnt"][t]), (tag, t)
    io = case["inner"]["uni_off"].astype(np.int64)
    node_t = np.zeros(int(io[-1]), dtype=np.int64)
    node_t[case["inner"]["members"] >> 1] = np.repeat(np.arange(T), np.diff(io))
    occ = np.bincount(r["x"]["node_origin"], minlength=int(io[-1]))
    want = np.where(np.asarray(res, dtype=bool), np.diff(u["copy_off"].astype(np.int64)), 1)[node_t]
    assert occ.tolist() == want.tolist(), tag  # a node occurs once, or once per copy of its resolved unitig
    x = r["x"]
    assert x["n_members"] == int(x["uni_off"][-1]) and ((x["members"] >> 1) == np.arange(x["n_members"])).all(), tag


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def inner_of(rng, lens, circular=None):
    """a decomposition with the given unitig lengths: node ids in order, a random orientation each"""
    n = int(np.sum(lens))
    return {"uni_off": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
            "members": (2 * np.arange(n) + rng.integers(0, 2, size=n)).astype(np.uint32),
            "circular": np.zeros(len(lens), dtype=np.uint8) if circular is None else np.asarray(circular, dtype=np.uint8)}


def make_case(T, edges, triples, lens=None, circular=None, seed=0, cnt=None, ec=None):
    """edges closed under twins; triples (A, V, C) of oriented unitigs: in-edge A -> V matched with out-edge V -> C (and its twin)"""
    rng = np.random.default_rng(seed)
    ro, d = tu.csr_of(T, edges)
    r, dd = [int(x) for x in ro], [int(x) for x in d]
    src = tsp._sources(r)
    partner, resolved = np.full(len(d), NONE, dtype=np.uint32), np.zeros(T, dtype=np.uint8)
    for A, V, C_ in triples:
        a, b = tsp._find(r, dd, A, V), tsp._find(r, dd, V, C_)
        partner[a], partner[tsp._twin(r, dd, src, b)] = b, tsp._twin(r, dd, src, a)
        resolved[V >> 1] = 1
    lens = (1 + np.arange(T) % 3) if lens is None else lens
    return {"ro": ro, "d": d, "T": T, "resolved": resolved, "partner": partner, "inner": inner_of(rng, lens, circular),
            "cnt": rng.integers(1, 10 ** 6, size=T).astype(np.uint64) if cnt is None else np.asarray(cnt, dtype=np.uint64),
            "ec": rng.integers(1, 100, size=len(d)).astype(np.uint32) if ec is None else np.asarray(ec, dtype=np.uint32)}


X_EDGES = [(0, 4), (2, 4), (4, 6), (4, 8)]  # A = 0, B = 1 -> R = 2 -> C = 3, D = 4


def hand(name):
    if name == "a":  # the plain 2-in / 2-out repeat
        return make_case(5, X_EDGES, [(0, 4, 6), (2, 4, 8)])
    if name == "b":  # Q = 0, A = 1, R = 2, P = 3: A+ enters both strands of R, and the matching sends A+ -> R+ to the later copy
        return make_case(4, [(2, 4), (2, 5), (4, 6), (5, 0)], [(2, 4, 6), (1, 4, 3)])
    if name == "c":  # A, B -> R1 -> {R2, C}; {R1, D} -> R2 -> E, F: two resolved unitigs joined by an edge
        return make_case(8, [(0, 4), (2, 4), (4, 8), (4, 6), (10, 8), (8, 12), (8, 14)], [(0, 4, 8), (2, 4, 6), (4, 8, 12), (10, 8, 14)])
    if name == "d":  # 3 x 3, matched I1 - O2, I2 - O3, I3 - O1; counts that take the 128-bit product
        return make_case(7, [(0, 6), (2, 6), (4, 6), (6, 8), (6, 10), (6, 12)], [(0, 6, 10), (2, 6, 12), (4, 6, 8)],
                         cnt=[5, 6, 7, 2 ** 63 + 12345, 8, 9, 10], ec=[2 ** 32 - 1, 2 ** 32 - 3, 2 ** 31 + 7] * 4)
    if name == "e":  # nothing resolved
        return make_case(5, X_EDGES, [])
    if name == "f":  # a circular unitig (isolated: its closing link is no edge) beside a resolved one
        return make_case(6, X_EDGES, [(0, 4, 6), (2, 4, 8)], lens=[2, 1, 3, 2, 1, 3], circular=[0, 0, 0, 0, 0, 1])
    if name == "g":  # R = 0 -> L1 = 1, L2 = 2 -> R, matched L1 - R - L2 and L2 - R - L1: the copies close one cycle
        return make_case(3, [(0, 2), (0, 4), (2, 0), (4, 0)], [(2, 0, 4), (4, 0, 2)])
    raise KeyError(name)


HAND = "abcdefg"
A_KEYS = [(0, 4), (2, 6), (4, 8), (5, 1), (6, 10), (7, 3), (9, 5), (11, 7)]  # case a: R0 = A .. C (copies 2, 3 are R), R1 = B .. D


def chain_case(rng, T0, n_reads, front=0, n_copies=None, slots=None):
    """a ring of T0 unitigs whose junctions the paired reads of test_span.chained_paths resolve (some of them), behind `front`
    isolated unitigs and before as many more as make T' == n_copies; the last unitig's length makes M == slots when given"""
    paths, ro, d, off, T = tsp.chained_paths(rng, T0, [12] * n_reads, p_break=0.02, paired=True)
    ref = tsp.spans_reference(paths, ro, d, off)
    resolved, partner, _, _ = tsp.resolve_reference(ro, d, T, *tsp.count_keys(ref["keys"]), 2)
    core = sum(int(ro[2 * t + 1] - ro[2 * t]) if resolved[t] else 1 for t in range(T))
    back = 0 if n_copies is None else n_copies - core - front
    assert back >= 0 and (slots is None or back >= 1)
    lens = np.concatenate([1 + np.arange(front) % 3, np.diff(off.astype(np.int64)), 1 + np.arange(back) % 3]).astype(np.int64)
    Tn = front + T + back
    res = np.concatenate([np.zeros(front, np.uint8), resolved, np.zeros(back, np.uint8)])
    if slots is not None:
        m = int((lens * np.where(res, 2, 1))[:-1].sum())  # every junction of the ring has in == out == 2
        assert slots > m
        lens[-1] = slots - m
    circular = np.zeros(Tn, dtype=np.uint8)
    circular[:front] = lens[:front] > 1  # an isolated unitig may be a cycle
    ro = np.concatenate([np.zeros(2 * front, np.uint64), ro, np.full(2 * back, ro[-1], np.uint64)])
    return {"ro": ro, "d": (d + 2 * front).astype(np.uint32), "T": Tn, "resolved": res, "partner": partner, "inner": inner_of(rng, lens, circular),
            "cnt": rng.integers(1, 10 ** 6, size=Tn).astype(np.uint64), "ec": rng.integers(1, 100, size=len(d)).astype(np.uint32)}


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert "S2K_ABI_VERSION 2" in header and pkg.ABI_VERSION == 2
    assert hasattr(pkg.Engine, "graph_untangle") and hasattr(pkg.Engine, "unitig_expand")
    assert hasattr(pkg.UnitigGraph, "untangle") and hasattr(pkg.NodeSequences, "take")
    assert "untangle" in pkg.UnitigGraph.resolve.__doc__


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "untangle_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "untangle_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    U = pkg.UnitigOut
    assert facts["sizeof.s2k_unitig_out"] == (ctypes.sizeof(U),)
    for f, _ in U._fields_:
        assert facts["s2k_unitig_out." + f] == (getattr(U, f).offset, ctypes.sizeof(dict(U._fields_)[f])), f
    assert facts["S2K_NO_PARTNER"] == (pkg.NO_PARTNER,) == (NONE,) and facts["S2K_ABI_VERSION"] == (pkg.ABI_VERSION,)
    assert facts["S2K_ERR_INVALID_ARG"] == (1,) and facts["S2K_ERR_CAPACITY"] == (7,)


def test_cpp_untangle_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "untangle_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "untangle_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    """csrc/Makefile lists it; csrc/Makefile.asan includes that Makefile and links every object of its SRCS"""
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "s2k_untangle.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))
    asan = open(os.path.join(csrc, "Makefile.asan")).read()
    assert "include Makefile" in asan and "$(OBJS)" in asan


@pytest.mark.parametrize("name", HAND)
def test_reference_hand_made(name):
    case = hand(name)
    r = contigs_reference(case)
    check_invariants(case, r, name)
    u, o, x = r["u"], r["o"], r["x"]
    ro, d = [int(v) for v in case["ro"]], [int(v) for v in case["d"]]
    if name == "a":
        assert u["keys"].tolist() == [a << 32 | b for a, b in A_KEYS] and u["copy_off"].tolist() == [0, 1, 2, 4, 5, 6]
        assert u["origin"].tolist() == [0, 1, 2, 2, 3, 4] and (u["n_copies"], u["n_duplicated"], o["n_unitigs"]) == (6, 1, 2)
        assert sorted(len(m) for m in np.split(o["members"], o["uni_off"][1:-1].astype(np.int64))) == [3, 3]
    if name == "b":  # the two edges of A+ leave in the other order: the map is not monotone inside the row
        e1, e2 = tsp._find(ro, d, 2, 4), tsp._find(ro, d, 2, 5)
        row = [int(e) for k, e in zip(u["keys"].tolist(), u["src_edge"].tolist()) if k >> 32 == 2 * int(u["copy_off"][1])]
        assert e1 < e2 and row == [e2, e1], (row, e1, e2)
        R = int(u["copy_off"][2])
        assert 2 * int(u["copy_off"][1]) << 32 | (2 * R + 1) in u["keys"].tolist() and 2 * int(u["copy_off"][1]) << 32 | (2 * R + 2) in u["keys"].tolist()
    if name == "c":  # one new edge joins a copy of R1 to a copy of R2; three contigs: A R1 R2 E, B R1 C, D R2 F
        both = [k for k in u["keys"].tolist() if case["resolved"][u["origin"][(k >> 32) >> 1]] and case["resolved"][u["origin"][(k & NONE) >> 1]]]
        assert len(both) == 2 and (u["n_copies"], o["n_unitigs"]) == (10, 3)  # the edge and its twin
        assert sorted(np.diff(o["uni_off"].astype(np.int64)).tolist()) == [3, 3, 4]
    if name == "d":
        assert (u["n_copies"], u["n_duplicated"], o["n_unitigs"]) == (9, 1, 3)
        contigs = [sorted(u["origin"][m >> 1].tolist()) for m in np.split(o["members"], o["uni_off"][1:-1].astype(np.int64))]
        assert sorted(contigs) == [[0, 3, 5], [1, 3, 6], [2, 3, 4]]
        w, S = [int(v) for v in case["ec"]], None  # the shares of 2^63 + 12345 by the counts of R's in-edges, exactly
        ins = [tsp._find(ro, d, A, 6) for A in (0, 2, 4)]
        S = sum(w[a] for a in ins)
        assert sorted(u["copy_count"][3:6].tolist()) == sorted((2 ** 63 + 12345) * w[a] // S for a in ins) and S >= 2 ** 32
    if name == "e":  # the identity
        ek = np.array([s << 32 | v for s, v in zip(tsp._sources(ro), d)], dtype=np.uint64)
        assert u["keys"].tobytes() == ek.tobytes() and u["src_edge"].tolist() == list(range(len(d))) and u["origin"].tolist() == list(range(5))
        assert u["copy_count"].tobytes() == case["cnt"].tobytes() and (u["n_copies"], u["n_duplicated"]) == (5, 0)
    if name == "f":  # the circular unitig is a contig of one copy, still circular; no other contig is
        t = int(x["node_unitig"][np.nonzero(x["node_origin"] == int(case["inner"]["uni_off"][5]))[0][0]])
        assert x["circular"].tolist() == [int(i == t) for i in range(o["n_unitigs"])] and not o["circular"].any() and o["n_unitigs"] == 3
    if name == "g":  # one circular contig of four copies: R L R L
        assert o["n_unitigs"] == 1 and o["circular"].tolist() == [1] == x["circular"].tolist() and u["n_copies"] == 4
        assert sorted(u["origin"][o["members"] >> 1].tolist()) == [0, 0, 1, 2] and len(r["edge_keys"]) == 0


def test_reference_random_paired_chains_invariants():
    rng = np.random.default_rng(61)
    dup = 0
    for T0, n_reads, front in ((9, 60, 0), (30, 150, 5), (50, 300, 0)):
        case = chain_case(rng, T0, n_reads, front=front)
        r = contigs_reference(case)
        check_invariants(case, r, (T0, n_reads))
        dup += r["u"]["n_duplicated"]
    assert dup > 30


def repeat_contigs(c, oracle, ecoli):
    """the repeat fixture through the references alone -> (case, contigs_reference, node records, stitched strings, [S1, S2])"""
    reads, seqs = tsp.repeat_reads(ecoli)
    R = tsp.REPEAT
    b = tus._oracle_batch(oracle, reads, R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    nodes = tus.node_sequences_reference([b], c["g"]["keys"], R["k"])
    uni = c["uni"]
    _, _, _, cnt = ts.unitig_view(c["g"])
    case = {"ro": c["uro"], "d": c["ud"], "T": c["T"], "resolved": c["resolved"], "partner": c["partner"], "cnt": cnt,
            "ec": c["g"]["edge_counts"][uni["src_edge"].astype(np.int64)], "inner": {f: uni[f] for f in ("uni_off", "members", "circular")}}
    r = contigs_reference(case)
    take = {f: np.asarray(nodes[f])[r["x"]["node_origin"].astype(np.int64)] for f in ("rep", "seq_off", "seq_len", "shift_fwd", "shift_rev", "rev")}
    take["pool"] = nodes["pool"]
    stitched = tus.unitig_sequences_reference(r["x"], take)
    return case, r, nodes, stitched, seqs


def assert_two_contigs_of_the_two_sequences(strings, seqs):
    """each contig is a slice of S1 or of S2 (or of a reverse complement), one of each, and holds all of R"""
    R = seqs[0][tsp.REPEAT["flank"]: tsp.REPEAT["flank"] + tsp.REPEAT["repeat"]]
    assert R == seqs[1][tsp.REPEAT["flank"]: tsp.REPEAT["flank"] + tsp.REPEAT["repeat"]] and len(strings) == 2
    found = [[i for i, s in enumerate(seqs) if x in s or x in tus.revcomp(s)] for x in strings]
    assert sorted(found) == [[0], [1]], found
    assert all(R in x or tus.revcomp(R) in x for x in strings)


def test_repeat_fixture_untangled_by_the_references(repeat_case, oracle, ecoli):
    """5 unitigs -> 6 copies -> 2 contigs of 3 copies each, X1 R Y1 and X2 R Y2: stitched by the numpy reference from the gathered
    records, each is a slice of one of the two sequences and holds all of R"""
    case, r, nodes, stitched, seqs = repeat_contigs(repeat_case, oracle, ecoli)
    check_invariants(case, r, "repeat")
    u, o = r["u"], r["o"]
    assert (case["T"], u["n_copies"], u["n_duplicated"], o["n_unitigs"]) == (5, 6, 1, 2) and np.diff(o["uni_off"].astype(np.int64)).tolist() == [3, 3]
    assert len(r["edge_keys"]) == 0 and not r["x"]["circular"].any()
    strings = tus.unitig_strings(r["x"], stitched)
    assert_two_contigs_of_the_two_sequences(strings, seqs)
    assert int(r["counts"].sum()) <= int(case["cnt"].sum()) and int(case["cnt"].sum()) - int(r["counts"].sum()) <= 1
    print("repeat fixture untangled: contigs of %s bases, %d node instances of %d nodes" % ([len(s) for s in strings], r["x"]["n_members"], len(nodes["rep"])))


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


_dev, _out, _host, _marked, _ptr = ts._dev, ts._out, ts._host, ts._marked, ts._ptr


def raw_untangle(eng, case, capacity=None, null=(), counts=True, ctx=True, n_edges=None, T=None):
    """s2k_graph_untangle through ctypes, guards behind every output -> (status, n_copies, n_duplicated, {name: host array with guards})"""
    import torch

    ne, Tn = len(case["d"]), case["T"]
    cap = Tn + ne // 2 if capacity is None else capacity
    ins = [_dev(case["ro"], np.uint64), _dev(case["d"], np.uint32), _dev(case["resolved"], np.uint8), _dev(case["partner"], np.uint32),
           _dev(case["cnt"], np.uint64), _dev(case["ec"], np.uint32)]
    size = {"copy_off": Tn + 1, "origin": Tn + ne // 2, "copy_count": Tn + ne // 2, "keys": ne, "src_edge": ne}
    outs = {f: _out(size[f], dt) for f, dt in UNT}
    nc, nd = ctypes.c_uint64(777), ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_graph_untangle(eng.ctx if ctx else None, _ptr(ins[0], "row_off" in null), _ptr(ins[1], "dst" in null or ne == 0),
                                   ne if n_edges is None else n_edges, Tn if T is None else T, _ptr(ins[2], "resolved" in null),
                                   _ptr(ins[3], "partner" in null or ne == 0), _ptr(ins[4], not counts), _ptr(ins[5], not counts or ne == 0),
                                   *(_ptr(outs[f], f in null or "outputs" in null) for f, _ in UNT), cap, ctypes.byref(nc), ctypes.byref(nd))
    return s, nc.value, nd.value, {f: _host(outs[f], dt) for f, dt in UNT}


def _untouched(host, fields):
    return all(_marked(host[f], dt) for f, dt in fields)


def device_untangle(eng, case, want, tag):
    """the call against the reference: every array, the totals, the guards; the sizes-only call; capacity one short"""
    n, ne, Tn = want["n_copies"], len(case["d"]), case["T"]
    size = {"copy_off": Tn + 1, "origin": n, "copy_count": n, "keys": ne, "src_edge": ne}
    s, nc, nd, got = raw_untangle(eng, case, capacity=n)
    assert (s, nc, nd) == (0, n, want["n_duplicated"]), (tag, s, nc, nd)
    for f, dt in UNT:
        assert got[f][:size[f]].tobytes() == want[f].tobytes(), (tag, f, got[f][:8], want[f][:8])
        assert _marked(got[f], dt, size[f]), (tag, f, "guard")
    s, nc, nd, got = raw_untangle(eng, case, null=("outputs",))
    assert (s, nc, nd) == (0, n, want["n_duplicated"]) and _untouched(got, UNT), (tag, "sizes")
    s, nc, nd, got = raw_untangle(eng, case, capacity=n - 1)
    assert (s, nc, nd) == (7, n, want["n_duplicated"]) and _untouched(got, UNT), (tag, "capacity")
    s, nc, nd, got = raw_untangle(eng, case, capacity=n, counts=False, null=("origin",))  # without counts: copy_count stays as it was
    assert s == 0 and _marked(got["copy_count"], np.uint64) and _marked(got["origin"], np.uint32) and got["keys"][:ne].tobytes() == want["keys"].tobytes(), tag


def raw_expand(eng, outer, origin, inner, capacity=None, null=(), ctx=True, n_nodes=None):
    """s2k_unitig_expand through ctypes, guards behind every output -> (status, n_members, {name: host array with guards})"""
    import torch

    nt, ncp, Tn, n = len(outer["circular"]), len(origin), len(inner["circular"]), len(inner["members"])
    cap = 2 * n + 8 if capacity is None else capacity
    ins = [_dev(outer["uni_off"], np.uint64), _dev(outer["members"], np.uint32), _dev(outer["circular"], np.uint8), _dev(origin, np.uint32),
           _dev(inner["uni_off"], np.uint64), _dev(inner["members"], np.uint32), _dev(inner["circular"], np.uint8)]
    outs = {f: _out(nt + 1 if f == "uni_off" else nt if f == "circular" else cap, dt) for f, dt in EXP}
    nm = ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_unitig_expand(eng.ctx if ctx else None, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), nt, ncp, _ptr(ins[3]), _ptr(ins[4]), _ptr(ins[5]),
                                  _ptr(ins[6]), Tn, n if n_nodes is None else n_nodes, *(_ptr(outs[f], f in null or "outputs" in null) for f, _ in EXP), cap,
                                  ctypes.byref(nm))
    return s, nm.value, {f: _host(outs[f], dt) for f, dt in EXP}


def device_expand(eng, outer, origin, inner, want, tag):
    m, nt = want["n_members"], len(outer["circular"])
    s, nm, got = raw_expand(eng, outer, origin, inner, capacity=m)
    assert (s, nm) == (0, m), (tag, s, nm, m)
    for f, dt in EXP:
        n = nt + 1 if f == "uni_off" else nt if f == "circular" else m
        assert got[f][:n].tobytes() == want[f].tobytes(), (tag, f, got[f][:8], want[f][:8])
        assert _marked(got[f], dt, n), (tag, f, "guard")
    s, nm, got = raw_expand(eng, outer, origin, inner, null=("outputs",))
    assert (s, nm) == (0, m) and _untouched(got, EXP), (tag, "size")
    s, nm, got = raw_expand(eng, outer, origin, inner, capacity=m - 1)
    assert (s, nm) == (7, m) and _untouched(got, EXP), (tag, "capacity")


def device_case(eng, case, tag, invariants=True):
    r = contigs_reference(case)
    if invariants:
        check_invariants(case, r, tag)
    device_untangle(eng, case, r["u"], tag)
    device_expand(eng, r["o"], r["u"]["origin"], case["inner"], r["x"], tag)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", HAND)
def test_device_hand_made(eng, name):
    device_case(eng, hand(name), name)


# The new oriented copies number 2 T', which is even: the sizes round one wave (64) and one block (256) are 62 / 64 / 66 and 254 / 256 /
# 258.  The expansion's blocks take 256 slots each: M is one short of, equal to and one past a multiple of 256.
@pytest.mark.gpu
@pytest.mark.parametrize("n_ids,delta", [(62, -1), (64, 0), (66, 1), (254, 1), (256, -1), (258, 0)])
def test_device_paired_chains_round_a_wave_and_a_block(eng, n_ids, delta):
    rng = np.random.default_rng(n_ids)
    probe = chain_case(rng, 9, 60, front=n_ids % 3, n_copies=n_ids // 2)
    m = int((np.diff(probe["inner"]["uni_off"].astype(np.int64)) * np.where(probe["resolved"], 2, 1)).sum())
    rng = np.random.default_rng(n_ids)  # the same ring again, its last unitig sized for M
    case = chain_case(rng, 9, 60, front=n_ids % 3, n_copies=n_ids // 2, slots=(m // 256 + 1) * 256 + delta)
    r = device_case(eng, case, (n_ids, delta))
    assert 2 * r["u"]["n_copies"] == n_ids and r["x"]["n_members"] % 256 == delta % 256 and r["u"]["n_duplicated"] > 0


@pytest.mark.gpu
def test_device_more_copies_than_4096_waves(eng):
    """more new oriented copies than 4096 blocks of one wave each (2 T' > 262 144): the resolved ring lies behind the isolated unitigs"""
    rng = np.random.default_rng(62)
    case = chain_case(rng, 30, 150, front=132000)
    r = device_case(eng, case, "big", invariants=False)  # the invariants of this ring are checked on the CPU tier
    assert 2 * r["u"]["n_copies"] > 4096 * 64 and r["u"]["n_duplicated"] > 5


@pytest.mark.gpu
def test_device_more_lanes_than_one_grid_pass(eng):
    """more new oriented copies than the 4096 * 256 lanes of one pass of the grid: the resolved ring is reached in the lanes' second
    pass.  The expansion takes any decomposition of the copies that meets its rules: here every copy is a contig of its own,
    alternately on its forward and on its reverse strand (compacting a million nodes in Python would take the test past a few seconds)"""
    rng = np.random.default_rng(62)
    case = chain_case(rng, 30, 150, front=530000)
    u = untangle_reference(case["ro"], case["d"], case["T"], case["resolved"], case["partner"], case["cnt"], case["ec"])
    n = u["n_copies"]
    assert 2 * n > 4096 * 256 and u["n_duplicated"] > 5
    device_untangle(eng, case, u, "two passes")
    outer = {"uni_off": np.arange(n + 1, dtype=np.uint64), "members": (2 * np.arange(n) + np.arange(n) % 2).astype(np.uint32),
             "circular": np.zeros(n, dtype=np.uint8)}
    device_expand(eng, outer, u["origin"], case["inner"], expand_reference(outer, u["origin"], case["inner"]), "two passes")


def _edges_into(case, V):
    """(the in-edges of the oriented unitig V, the bounds of its row)"""
    ro, d = [int(x) for x in case["ro"]], [int(x) for x in case["d"]]
    src = tsp._sources(ro)
    return [tsp._twin(ro, d, src, f) for f in range(ro[V ^ 1], ro[(V ^ 1) + 1])], (ro[V], ro[V + 1])


@pytest.mark.gpu
def test_device_refusals_nothing_written(eng):
    base = hand("d")  # the 3 x 3 repeat: R = unitig 3, R+ = 6
    want = untangle_reference(base["ro"], base["d"], base["T"], base["resolved"], base["partner"], base["cnt"], base["ec"])
    ins, (oa, ob) = _edges_into(base, 6)

    def refused(**kw):
        case = dict(base)
        call = {k: kw.pop(k) for k in list(kw) if k in ("null", "ctx", "n_edges", "T", "capacity")}
        case.update(kw)
        s, nc, nd, got = raw_untangle(eng, case, **call)
        assert (s, nc, nd) == (1, 0, 0) and _untouched(got, UNT), (s, nc, nd, list(kw), call)

    p = base["partner"].copy()  # a partner outside the row of the strand its edge enters: the row before, and no edge at all
    p[ins[0]] = oa - 1
    refused(partner=p)
    p = base["partner"].copy()
    p[ins[0]] = len(base["d"])
    refused(partner=p)
    p = base["partner"].copy()
    p[ins[1]] = NONE
    refused(partner=p)
    p = base["partner"].copy()  # two in-edges with one partner
    p[ins[1]] = p[ins[0]]
    refused(partner=p)
    p = base["partner"].copy()  # a matching of R+ that the entries of R- do not mirror
    p[ins[0]], p[ins[1]] = p[ins[1]], p[ins[0]]
    refused(partner=p)
    r = base["resolved"].copy()  # a resolved byte of 2
    r[3] = 2
    refused(resolved=r)
    r = base["resolved"].copy()  # a resolved unitig with in != out, and one with in == out == 1
    r[0] = 1
    refused(resolved=r)
    chain = make_case(3, [(0, 2), (2, 4)], [])
    chain["resolved"][1] = 1
    s, nc, nd, got = raw_untangle(eng, chain)
    assert (s, nc, nd) == (1, 0, 0) and _untouched(got, UNT)
    for i, v in ((0, 1), (5, int(base["ro"][6]) + 1), (14, len(base["d"]) + 1)):  # the CSR rules
        x = base["ro"].copy()
        x[i] = v
        refused(ro=x)
    x = base["d"].copy()
    x[2] = 14
    refused(d=x)
    refused(ctx=False)
    for f in ("row_off", "dst", "resolved", "partner"):
        refused(null=(f,))
    z = ctypes.c_uint64(5)
    args = (None,) * 9 + (0, ctypes.byref(z), ctypes.byref(z))
    assert eng.lib.s2k_graph_untangle(eng.ctx, ctypes.c_void_p(16), ctypes.c_void_p(16), 2 ** 32, 1, *args) == 1 and z.value == 0  # before anything is read
    assert eng.lib.s2k_graph_untangle(eng.ctx, ctypes.c_void_p(16), None, 0, 2 ** 31, *args) == 1
    assert eng.lib.s2k_graph_untangle(eng.ctx, None, None, 1, 0, *args) == 1  # edges without unitigs
    assert eng.lib.s2k_graph_untangle(eng.ctx, None, None, 0, 0, *args) == 0 and z.value == 0  # no unitigs: nothing read
    s, nc, nd, got = raw_untangle(eng, base, capacity=want["n_copies"])  # and the call still works
    assert (s, nc, nd) == (0, 9, 1) and got["keys"][:len(base["d"])].tobytes() == want["keys"].tobytes()

    # the expansion
    r = contigs_reference(base)
    o, origin, inner = r["o"], r["u"]["origin"], base["inner"]

    def refused_expand(outer=o, origin=origin, inner=inner, **call):
        s, nm, got = raw_expand(eng, outer, origin, inner, **call)
        assert (s, nm) == (1, 0) and _untouched(got, EXP), (s, nm, call)

    x = o["members"].copy()  # an outer member that is no copy
    x[4] = 2 * len(origin)
    refused_expand(outer=dict(o, members=x))
    x = origin.copy()  # an origin that is no unitig
    x[2] = base["T"]
    refused_expand(origin=x)
    for i, v in ((0, 1), (3, int(inner["uni_off"][2])), (3, int(inner["uni_off"][4])), (base["T"], int(inner["uni_off"][-1]) - 1)):
        x = inner["uni_off"].copy()  # inner uni_off: not from 0, not strictly ascending, not ending at n_nodes
        x[i] = v
        refused_expand(inner=dict(inner, uni_off=x))
    x = o["uni_off"].copy()
    x[1] = x[2]
    refused_expand(outer=dict(o, uni_off=x))
    refused_expand(n_nodes=len(inner["members"]) + 1)
    refused_expand(ctx=False)
    args = (None,) * 6 + (0, ctypes.byref(z))
    assert eng.lib.s2k_unitig_expand(eng.ctx, None, None, None, 0, 2 ** 31, None, None, None, None, 0, 0, *args) == 1
    assert eng.lib.s2k_unitig_expand(eng.ctx, None, None, None, 0, 0, None, None, None, None, 0, 0, *args) == 0 and z.value == 0


@pytest.mark.gpu
def test_device_deterministic(eng):
    rng = np.random.default_rng(63)
    case = chain_case(rng, 300, 900, front=7)
    r = contigs_reference(case)
    runs = []
    for _ in range(2):
        s, nc, nd, got = raw_untangle(eng, case)
        s2, nm, exp = raw_expand(eng, r["o"], r["u"]["origin"], case["inner"])
        assert (s, s2) == (0, 0) and nd > 50
        runs.append(b"".join(got[f].tobytes() for f, _ in UNT) + b"".join(exp[f].tobytes() for f, _ in EXP) + bytes(str((nc, nd, nm)), "ascii"))
    assert runs[0] == runs[1]


def _contigs_host(cg, node_origin):
    h = tu._unitig_graph_host(cg)
    h["node_origin"] = node_origin.cpu().numpy().view(np.uint32)
    return h


def assert_contigs(cg, node_origin, stats, r, tag):
    """what UnitigGraph.untangle returned against contigs_reference: every array"""
    x, u, o = r["x"], r["u"], r["o"]
    assert stats == {"copies": u["n_copies"], "duplicated": u["n_duplicated"], "contigs": o["n_unitigs"]}, (tag, stats)
    for f, dt in EXP:
        got = node_origin if f == "node_origin" else getattr(cg, f)
        assert got.cpu().numpy().view(dt).tobytes() == x[f].tobytes(), (tag, f)
    assert cg.n_nodes == x["n_members"] and cg.n_links == o["n_links"] and cg.n_unitigs == o["n_unitigs"], tag
    assert tg._u64(cg.counts).tobytes() == r["counts"].astype(np.uint64).tobytes(), (tag, "counts")
    assert tg._u64(cg.edge_keys).tobytes() == r["edge_keys"].tobytes() and cg.edge_counts.cpu().numpy().view(np.uint32).tobytes() == r["edge_counts"].tobytes(), tag
    assert tg._u64(cg.row_off).tobytes() == r["cro"].tobytes() and cg.dst.cpu().numpy().view(np.uint32).tobytes() == r["cd"].tobytes(), tag


def _fasta(path):
    lines = open(path).read().split("\n")
    return [x.encode() for x in lines[1::2] if x]


@pytest.mark.gpu
def test_repeat_fixture_untangled_end_to_end(eng, repeat_case, oracle, ecoli, tmp_path):
    """extract -> graph -> unitigs -> thread -> spans -> resolve -> untangle -> sequences on the device: two contigs, X1 R Y1 and X2 R
    Y2, their bytes those of the reference stitch; the GFA and the FASTA of the contigs hold the same two sequences"""
    c, R = repeat_case, tsp.REPEAT
    case, r, nodes, stitched, seqs = repeat_contigs(c, oracle, ecoli)
    outs = tus._extract_mn(eng, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=R["min_count"], min_edge_count=1)
    ug = graph.unitigs(eng)
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, outs, len(c["reads"]), min_count=R["min_count"])
    table.close()
    resolved, partner, stats = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    assert resolved.cpu().numpy().tobytes() == c["resolved"].tobytes() and partner.cpu().numpy().view(np.uint32).tobytes() == c["partner"].tobytes()
    before = tu._unitig_graph_host(ug)
    contigs, node_origin, st = ug.untangle(eng, resolved, partner)
    assert_contigs(contigs, node_origin, st, r, "repeat")
    assert st == {"copies": 6, "duplicated": 1, "contigs": 2} and ug.n_unitigs == 5
    after = tu._unitig_graph_host(ug)
    assert all(np.array_equal(before[f], after[f]) for f in before)  # self is untouched
    ns = pkg.NodeSequences.build(eng, graph, [outs])
    out_off, out = contigs.sequences(eng, ns.take(node_origin))
    assert tg._u64(out_off).tobytes() == stitched["out_off"].tobytes() and out.cpu().numpy().tobytes() == stitched["out"].tobytes()
    assert contigs.overlap.cpu().numpy().view(np.uint32).tobytes() == stitched["overlap"].tobytes()
    strings = tus.unitig_strings(r["x"], {"out_off": tg._u64(out_off), "out": out.cpu().numpy()})
    assert_two_contigs_of_the_two_sequences(strings, seqs)
    p, q = str(tmp_path / "contigs.gfa"), str(tmp_path / "contigs.fa")
    contigs.write_gfa(p, members=True, sequences=(out_off, out))
    pkg.write_fasta(q, out_off, out)
    s_lines = [x.split("\t") for x in open(p).read().split("\n") if x.startswith("S\t")]
    assert [x[2].encode() for x in s_lines] == strings == _fasta(q) and not any(x.startswith("L\t") for x in open(p).read().split("\n"))
    assert [x[4] for x in s_lines] == ["nm:i:%d" % n for n in np.diff(r["x"]["uni_off"].astype(np.int64))]
    place = contigs.places(eng)  # the expansion is a decomposition of the instances: s2k_unitig_node_places accepts it
    assert place.shape == (r["x"]["n_members"], 4)


@pytest.mark.gpu
def test_ecoli_reads_with_errors_simplified_then_untangled(eng, oracle, ecoli):
    """the 600 reads with 0.5 % substitutions, Regular 12/5, through simplify(10, 20), threaded, resolved and untangled: device ==
    reference for whatever the spans resolve there (nothing resolved is the identity, still compared); the counts are printed"""
    mc = 2
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    b = oracle.batch(*pkg.pack_reads(reads), 12, 5, 0.05, int(pkg.HashMode.Regular))
    outs = tt._extract_se(eng, reads, 12, 5, 0.05, pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=mc, min_edge_count=1)
    sg, _, _ = graph.simplify(eng, 10, 20)
    final, _, _ = ts.simplify_rounds_reference(tg.graph_reference([b], mc, 1), 10, 20)
    uni, uro, ud, cnt = ts.unitig_view(final)
    T = uni["n_unitigs"]
    ref_paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], final["keys"], final["counts"], mc, tt.places_reference(uni), n_unitigs=T)
    sk, sc = tsp.count_keys(tsp.spans_reference(ref_paths, uro, ud, uni["uni_off"])["keys"])
    res, par, nc, nr = tsp.resolve_reference(uro, ud, T, sk, sc, 2)
    case = {"ro": uro, "d": ud, "T": T, "resolved": res, "partner": par, "cnt": cnt, "ec": final["edge_counts"][uni["src_edge"].astype(np.int64)],
            "inner": {f: uni[f] for f in ("uni_off", "members", "circular")}}
    r = device_case(eng, case, "ecoli")
    ug = sg.unitigs(eng)
    table = pkg.CountTable(eng, sg.keys, sg.counts)
    paths = ug.thread(eng, table, outs, len(reads), min_count=mc)
    table.close()
    resolved, partner, stats = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    assert resolved.cpu().numpy().tobytes() == res.tobytes() and partner.cpu().numpy().view(np.uint32).tobytes() == par.tobytes()
    contigs, node_origin, st = ug.untangle(eng, resolved, partner)
    assert_contigs(contigs, node_origin, st, r, "ecoli")
    print("simplified and untangled: %d unitigs, %d edges, %d candidates, %d resolved -> %d copies, %d contigs, %d node instances of %d nodes" % (
        T, len(ud), nc, nr, st["copies"], st["contigs"], contigs.n_nodes, len(final["keys"])))
