"""Error gaps in read paths bridged along the graph: s2k_paths_bridge (include/s2k.h).  The reference is
`bridge_reference`, a serial restatement of the header's definition (plain loops over reads and steps; `find` is a scan of one row);
the device's arrays equal its arrays exactly, every one of them, in every test."""
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
import test_walk as twk
from test_span import repeat_case  # noqa: F401  (the module-scoped fixture of the repeat)

pkg = import_package()

LINKED = 1
STEP = ("unitig", "pos", "count", "item", "flags", "start", "end")
OUT32 = STEP + ("matched",)
DEFAULT = (16, 2)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def bridge_reference(paths, row_off, dst, uni_off, circular, max_gap, max_slip):
    """paths: dict with path_off and the seven step arrays -> dict: path_off uint64, the step arrays and matched uint32 (one entry per
    output step), join uint8 (one entry per input step), n_steps, n_merged, n_bridged"""
    ro, d, off = [int(x) for x in row_off], [int(x) for x in dst], [int(x) for x in uni_off]
    circ = [int(x) for x in circular]
    po = [int(x) for x in paths["path_off"]]
    u, p, c, it, fl, st, en = ([int(x) for x in paths[f]] for f in STEP)
    ln = lambda U: off[(U >> 1) + 1] - off[U >> 1]  # noqa: E731
    n = len(u)
    join, slack = [0] * n, [0] * n
    for r in range(len(po) - 1):
        for s in range(po[r] + 1, po[r + 1]):  # a read's first step has join 0
            a, b, endp = u[s - 1], u[s], p[s - 1] + c[s - 1]
            gi = it[s] - (it[s - 1] + c[s - 1])
            assert gi >= 0, (r, s)
            if circ[a >> 1] or circ[b >> 1]:
                continue
            if a == b and p[s] >= endp:
                kind, gp = 1, p[s] - endp
            elif tsp._find(ro, d, a, b) is not None:
                kind, gp = 2, (ln(a) - endp) + p[s]
            else:
                continue
            if gi <= max_gap and gp <= max_gap and abs(gi - gp) <= max_slip:
                join[s], slack[s] = kind, gi + gp
    out = {f: [] for f in OUT32}
    path_off = [0]
    for r in range(len(po) - 1):
        a = po[r]
        while a < po[r + 1]:
            b = a
            while b + 1 < po[r + 1] and join[b + 1] == 1:
                b += 1
            pos = 0 if join[a] == 2 else p[a]
            endpos = ln(u[b]) if b + 1 < po[r + 1] and join[b + 1] == 2 else p[b] + c[b]
            for f, v in (("unitig", u[a]), ("pos", pos), ("count", (endpos - pos) & 0xFFFFFFFF), ("item", it[a]),
                         ("flags", fl[a] | (LINKED if join[a] == 2 else 0)), ("start", st[a]), ("end", en[b]), ("matched", sum(c[a:b + 1]) & 0xFFFFFFFF)):
                out[f].append(v)
            a = b + 1
        path_off.append(len(out["unitig"]))
    res = {f: np.array(v, dtype=np.uint32) for f, v in out.items()}
    res["path_off"] = np.array(path_off, dtype=np.uint64)
    res["join"] = np.array(join, dtype=np.uint8)
    res.update(n_steps=len(out["unitig"]), n_merged=sum(1 for x in join if x == 1), n_bridged=sum(1 for k, x in zip(join, slack) if k == 2 and x > 0))
    return res


def check_bridge_invariants(ref, case, tag):
    """every input step in exactly one output step, in order; matched adds up; a merged step covers at least what was found; the
    bridged paths pass for paths: inside their unitigs, and what was joined across an edge now follows it"""
    paths = case["paths"]
    n = len(paths["unitig"])
    heads = int((ref["join"] != 1).sum())
    assert ref["n_steps"] == heads == n - ref["n_merged"] and int(ref["path_off"][-1]) == heads, tag
    assert int(ref["matched"].astype(np.int64).sum()) == int(paths["count"].astype(np.int64).sum()), tag
    lin = case["circular"][ref["unitig"] >> 1] == 0
    ln = np.diff(case["uni_off"].astype(np.int64))[ref["unitig"] >> 1]
    assert (ref["matched"][lin] <= ref["count"][lin]).all() and (ref["pos"].astype(np.int64) + ref["count"] <= ln)[lin].all(), tag
    follow = twk.follow_reference(ref, case["ro"], case["d"], case["uni_off"])
    heads_in = np.nonzero(ref["join"] != 1)[0]
    for o, s in enumerate(heads_in.tolist()):
        if ref["join"][s] == 2:
            assert follow[o] is not None, (tag, o, s)


# ---- hand-made: six unitigs ------------------------------------------------------------------------------------------------------------
#  A = 0 (10 members) -> R = 1 (40) -> C = 2 (6) -> N = 5 (3); O = 3 (5) circular; P = 4 (30) with a loop P+ -> P+
B_LEN = [10, 40, 6, 5, 30, 3]
B_CIRC = [0, 0, 0, 1, 0, 0]
B_EDGES = [(0, 2), (2, 4), (4, 10), (8, 8)]  # closed under twins by tu.csr_of
B_LIMITS = (4, 1)  # max_gap, max_slip of the hand-made cases
L_ = LINKED


def _s(U, pos, count, item, flags=0):
    """an input step; start and end made up from the items"""
    return (U, pos, count, item, flags, 7 * item, 7 * (item + count - 1) + 30)


def _o(U, pos, count, item, flags, matched, last_item, last_count):
    """an output step: start from its first item, end from the last input step of its run"""
    return (U, pos, count, item, flags, 7 * item, 7 * (last_item + last_count - 1) + 30, matched)


# name -> (input steps, join per input step, output steps, merged, bridged)
B_READS = {
    "no join: no edge from A to C": ([_s(0, 0, 3, 0), _s(4, 0, 2, 5)], [0, 0], [_o(0, 0, 3, 0, 0, 3, 0, 3), _o(4, 0, 2, 5, 0, 2, 5, 2)], 0, 0),
    "kind 1: two steps on R, two positions and two items apart": (
        [_s(2, 3, 4, 0), _s(2, 9, 5, 6)], [0, 1], [_o(2, 3, 11, 0, 0, 9, 6, 5)], 1, 0),
    "kind 2: A left two early, R entered at 1; three positions, two items": (
        [_s(0, 2, 6, 0), _s(2, 1, 4, 8)], [0, 2], [_o(0, 2, 8, 0, 0, 6, 0, 6), _o(2, 0, 5, 8, L_, 4, 8, 4)], 0, 1),
    "kind 2, 1, 2: C becomes a whole-unitig step": (
        [_s(2, 30, 9, 0), _s(4, 1, 2, 10), _s(4, 4, 1, 13), _s(10, 1, 2, 15)], [0, 2, 1, 2],
        [_o(2, 30, 10, 0, 0, 9, 0, 9), _o(4, 0, 6, 10, L_, 3, 13, 1), _o(10, 0, 3, 15, L_, 2, 15, 2)], 1, 2),
    "a step that already follows its edge comes out unchanged": (
        [_s(0, 5, 5, 0), _s(2, 0, 3, 5, L_)], [0, 2], [_o(0, 5, 5, 0, 0, 5, 0, 5), _o(2, 0, 3, 5, L_, 3, 5, 3)], 0, 0),
    "the gap at max_gap": ([_s(2, 0, 2, 0), _s(2, 6, 2, 6)], [0, 1], [_o(2, 0, 8, 0, 0, 4, 6, 2)], 1, 0),
    "the gap on the graph at max_gap + 1": ([_s(2, 0, 2, 0), _s(2, 7, 2, 6)], [0, 0], [_o(2, 0, 2, 0, 0, 2, 0, 2), _o(2, 7, 2, 6, 0, 2, 6, 2)], 0, 0),
    "the gap in the read at max_gap + 1": ([_s(2, 0, 2, 0), _s(2, 6, 2, 7)], [0, 0], [_o(2, 0, 2, 0, 0, 2, 0, 2), _o(2, 6, 2, 7, 0, 2, 7, 2)], 0, 0),
    "the slip at its limit, the read longer": ([_s(2, 0, 2, 0), _s(2, 4, 2, 5)], [0, 1], [_o(2, 0, 6, 0, 0, 4, 5, 2)], 1, 0),
    "the slip at its limit, the graph longer": ([_s(2, 0, 2, 0), _s(2, 5, 2, 4)], [0, 1], [_o(2, 0, 7, 0, 0, 4, 4, 2)], 1, 0),
    "the slip one past it, the read longer": ([_s(2, 0, 2, 0), _s(2, 3, 2, 5)], [0, 0], [_o(2, 0, 2, 0, 0, 2, 0, 2), _o(2, 3, 2, 5, 0, 2, 5, 2)], 0, 0),
    "the slip one past it, the graph longer": ([_s(2, 0, 2, 0), _s(2, 5, 2, 3)], [0, 0], [_o(2, 0, 2, 0, 0, 2, 0, 2), _o(2, 5, 2, 3, 0, 2, 3, 2)], 0, 0),
    "the slip across an edge, at its limit and past it": (
        [_s(0, 0, 9, 0), _s(2, 1, 1, 10), _s(3, 0, 39, 20), _s(1, 2, 1, 60)], [0, 2, 0, 0],
        [_o(0, 0, 10, 0, 0, 9, 0, 9), _o(2, 0, 2, 10, L_, 1, 10, 1), _o(3, 0, 39, 20, 0, 39, 20, 39), _o(1, 2, 1, 60, 0, 1, 60, 1)], 0, 1),
    "a circular unitig is never joined, and may pass its last member": (
        [_s(6, 0, 2, 0), _s(6, 3, 1, 3), _s(6, 4, 4, 5)], [0, 0, 0],
        [_o(6, 0, 2, 0, 0, 2, 0, 2), _o(6, 3, 1, 3, 0, 1, 3, 1), _o(6, 4, 4, 5, 0, 4, 5, 4)], 0, 0),
    "backwards on P: kind 2 over its loop edge": (
        [_s(8, 27, 3, 0), _s(8, 2, 3, 5)], [0, 2], [_o(8, 27, 3, 0, 0, 3, 0, 3), _o(8, 0, 5, 5, L_, 3, 5, 3)], 0, 1),
    "backwards on N, which has no loop edge": ([_s(10, 2, 1, 0), _s(10, 0, 2, 2)], [0, 0], [_o(10, 2, 1, 0, 0, 1, 0, 1), _o(10, 0, 2, 2, 0, 2, 2, 2)], 0, 0),
    "a read that ends on R": ([_s(2, 0, 2, 0)], [0], [_o(2, 0, 2, 0, 0, 2, 0, 2)], 0, 0),
    "the next read goes on where it ended: a read's first step is never joined": (
        [_s(2, 3, 2, 3), _s(2, 6, 1, 6, L_)], [0, 1], [_o(2, 3, 4, 3, 0, 3, 6, 1)], 1, 0),
    "an empty read": ([], [], [], 0, 0),
    "the twin strand: R- to A-, kind 2 with nothing missing in the read": (
        [_s(3, 36, 3, 0), _s(1, 0, 4, 4)], [0, 2], [_o(3, 36, 4, 0, 0, 3, 0, 3), _o(1, 0, 4, 4, L_, 4, 4, 4)], 0, 1),
}


def paths_of(reads):
    """lists of (unitig, pos, count, item, flags, start, end) -> the path dict"""
    steps = [s for r in reads for s in r]
    out = {f: np.array([s[i] for s in steps], dtype=np.uint32) for i, f in enumerate(STEP)}
    out["path_off"] = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    return out


def hand_case(reads=None):
    ro, d = tu.csr_of(len(B_LEN), B_EDGES)
    reads = [c[0] for c in B_READS.values()] if reads is None else reads
    return {"paths": paths_of(reads), "ro": ro, "d": d, "uni_off": np.concatenate([[0], np.cumsum(B_LEN)]).astype(np.uint64),
            "circular": np.array(B_CIRC, dtype=np.uint8)}


def reference_of(case, limits=DEFAULT):
    return bridge_reference(case["paths"], case["ro"], case["d"], case["uni_off"], case["circular"], *limits)


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def with_gaps(rng, case, p=0.35, slip=0.25):
    """a case of test_walk.py (chained_case / walked_case) with gaps cut into its paths: a step is split in two with positions missing
    between the pieces, or loses positions at its end or at its beginning; the items go on through every gap, with as many items
    missing as positions, or (probability `slip`) up to three more or fewer.  start and end are made up from the items."""
    paths = case["paths"]
    po = paths["path_off"].astype(np.int64).tolist()
    u, ps, c, fl = (paths[f].astype(np.int64).tolist() for f in tsp.PATH)
    it = paths["item"].astype(np.int64).tolist() if "item" in paths else None
    circ = case["uni"]["circular"].tolist()
    reads = []
    for r in range(len(po) - 1):
        steps, item, gi_next = [], 0, 0  # gi_next: items missing before the next piece
        for s in range(po[r], po[r + 1]):
            if s > po[r]:
                gi_next += (it[s] - it[s - 1] - c[s - 1]) if it is not None else (0 if fl[s] & LINKED else 1)
            noise = lambda: int(rng.integers(-3, 4)) if rng.random() < slip else 0  # noqa: E731
            pieces = [(ps[s], c[s], fl[s], gi_next)]
            x = rng.random()
            if c[s] >= 2 and x < p and not circ[u[s] >> 1]:  # a step on a circular unitig may go round: left as it is
                g = int(rng.integers(1, c[s]))
                if x < p / 3:  # positions lost at its end: the next piece lies g items further
                    pieces, gi_next = [(ps[s], c[s] - g, fl[s], gi_next)], max(g + noise(), 0)
                elif x < 2 * p / 3:  # at its beginning
                    pieces, gi_next = [(ps[s] + g, c[s] - g, 0, gi_next + max(g + noise(), 0))], 0
                else:  # split: c1 positions, g - 1 missing (none: the pieces only lost their link), the rest
                    c1 = int(rng.integers(1, c[s] - g + 1))
                    gap = max(g - 1 + noise(), 0)
                    pieces, gi_next = [(ps[s], c1, fl[s], gi_next), (ps[s] + c1 + g - 1, c[s] - c1 - g + 1, 0 if gap else LINKED, gap)], 0
            else:
                gi_next = 0
            for q, n, f, gi in pieces:
                item += gi
                steps.append((u[s], q, n, item, f, 7 * item, 7 * (item + n - 1) + 30))
                item += n
        reads.append(steps)
    return dict(case, paths=paths_of(reads), uni_off=case["uni"]["uni_off"], circular=case["uni"]["circular"])


def cut_paths(paths, n):
    """the first n steps"""
    out = {f: paths[f][:n] for f in STEP}
    out["path_off"] = np.minimum(paths["path_off"], np.uint64(n))
    return out


def gapped_case(rng, n_steps, kind):
    """n_steps steps: chains of whole unitigs of 1 .. 3 members with gaps cut in (every gap is short, most are bridged), or reads
    that walk a random decomposition with unitigs of up to 12 members, circular ones among them"""
    if kind == "chained":
        lens = list(rng.integers(0, 40, size=3 + n_steps // 12)) + [0, 1, 2]
        case = with_gaps(rng, twk.chained_case(rng, 37, lens, p_break=0.1))
    else:
        lens = list(rng.integers(0, 90, size=3 + n_steps // 5)) + [0, 1, 2]
        case = with_gaps(rng, twk.walked_case(rng, max(60, n_steps), lens, max_len=12))
    assert len(case["paths"]["unitig"]) >= n_steps, (len(case["paths"]["unitig"]), n_steps)
    return dict(case, paths=cut_paths(case["paths"], n_steps))


def runs_case(n_steps, run_cuts, read_cuts, T=3):
    """steps of one item at every third position of long unitigs (T of them in a chain, the steps spread over them), every step joined
    to the one before it by kind 1, or by kind 2 where the unitig changes -- but at run_cuts, where the read has 100 items more, and at
    read_cuts, where a new read begins"""
    per = (n_steps + T - 1) // T
    ro, d = tu.csr_of(T, [(2 * t, 2 * t + 2) for t in range(T - 1)])
    reads, steps, extra = [], [], 0
    for i in range(n_steps):
        if i in read_cuts and steps:
            reads.append(steps)
            steps, extra = [], -3 * i
        if i in run_cuts:
            extra += 100
        t, q = divmod(i, per)
        steps.append(_s(2 * t, 3 * q, 1, 3 * i + extra, L_ if i % 5 == 0 else 0))
    reads.append(steps)
    return {"paths": paths_of(reads), "ro": ro, "d": d, "uni_off": (np.arange(T + 1) * 3 * per).astype(np.uint64), "circular": np.zeros(T, dtype=np.uint8)}


def substituted(reads, rate, seed):
    """substitutions applied read by read: rng.random(len) < rate marks the bases, each marked base becomes another one"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    code = np.zeros(256, dtype=np.int64)
    code[list(b"ACGT")] = range(4)
    out = []
    for r in reads:
        x = np.frombuffer(r, dtype=np.uint8).copy()
        for i in np.nonzero(rng.random(len(x)) < rate)[0]:
            x[i] = acgt[(code[x[i]] + int(rng.integers(1, 4))) % 4]
        out.append(x.tobytes())
    return out


NOISY = dict(rate=0.01, seed=2)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_point_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    assert hasattr(lib, "s2k_paths_bridge") and "s2k_paths_bridge" in pkg.ABI_SYMBOLS and "s2k_paths_bridge(" in header
    assert "S2K_ABI_VERSION 2" in header and pkg.ABI_VERSION == 2
    assert hasattr(pkg.Engine, "paths_bridge") and hasattr(pkg.UnitigGraph, "bridge")
    p = pkg.ReadPaths(None, *[None] * 5)
    assert p.matched is None and pkg.ReadPaths(None, *[None] * 5, matched=7).matched == 7
    assert "s2k_paths_bridge" in open(os.path.join(ROOT, "include", "s2k.hpp")).read()


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "bridge_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bridge_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    T = pkg.ThreadOut
    assert facts["sizeof.s2k_thread_out"] == (ctypes.sizeof(T),)
    for f, t in T._fields_:
        assert facts["s2k_thread_out." + f] == (getattr(T, f).offset, ctypes.sizeof(t)), f
    assert facts["S2K_STEP_LINKED"] == (pkg.STEP_LINKED,) == (LINKED,) and facts["S2K_ABI_VERSION"] == (pkg.ABI_VERSION,)


def test_cpp_bridge_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "bridge_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bridge_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "s2k_bridge.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))
    assert "s2k_bridge.hip" in next(line for line in open(os.path.join(csrc, "Makefile.asan")).read().split("\n") if line.startswith("ASAN_SRCS"))


def test_reference_hand_made():
    """every join and every resulting step of the hand-made reads, written out by hand: all reads together, and each alone"""
    case = hand_case()
    assert tu.is_twin_symmetric(case["ro"], case["d"], len(B_LEN)) and len(case["d"]) == 8  # the loop's twin is another edge, P- -> P-
    ref = reference_of(case, B_LIMITS)
    check_bridge_invariants(ref, case, "hand")
    want = [o for c in B_READS.values() for o in c[2]]
    for i, f in enumerate(OUT32):
        assert ref[f].tolist() == [o[i] for o in want], f
    assert ref["join"].tolist() == [j for c in B_READS.values() for j in c[1]]
    assert ref["path_off"].tolist() == np.concatenate([[0], np.cumsum([len(c[2]) for c in B_READS.values()])]).tolist()
    assert (ref["n_steps"], ref["n_merged"], ref["n_bridged"]) == (len(want), sum(c[3] for c in B_READS.values()), sum(c[4] for c in B_READS.values()))
    assert ref["n_merged"] == 6 and ref["n_bridged"] == 6
    for name, (steps, join, outs, merged, bridged) in B_READS.items():
        one = reference_of(hand_case([steps]), B_LIMITS)
        assert one["join"].tolist() == join and (one["n_steps"], one["n_merged"], one["n_bridged"]) == (len(outs), merged, bridged), name
        for i, f in enumerate(OUT32):
            assert one[f].tolist() == [o[i] for o in outs], (name, f)
    # limits of 0: only what is already adjacent is joined -- the edge that is followed, nothing else
    zero = reference_of(case, (0, 0))
    assert zero["n_merged"] == 0 and zero["n_bridged"] == 0 and int((zero["join"] == 2).sum()) == 1
    for f in STEP:
        assert zero[f].tobytes() == case["paths"][f].tobytes(), f


def test_reference_random_paths_invariants():
    rng = np.random.default_rng(71)
    seen = [0, 0, 0]
    for kind, n in (("chained", 900), ("walked", 900), ("chained", 300), ("walked", 2500)):
        case = gapped_case(rng, n, kind)
        for limits in ((3, 1), DEFAULT, (0, 0)):
            ref = reference_of(case, limits)
            check_bridge_invariants(ref, case, (kind, n, limits))
        ref = reference_of(case, (3, 1))
        seen = [seen[0] + ref["n_merged"], seen[1] + ref["n_bridged"], seen[2] + int((ref["join"] == 0).sum())]
    assert seen[0] > 200 and seen[1] > 100 and seen[2] > 500, seen
    ref = reference_of(runs_case(5000, [], []), (4, 0))
    assert ref["n_steps"] == 3 and ref["n_merged"] == 4997 and ref["n_bridged"] == 2 and ref["count"].tolist() == [5001, 5001, 4996]


@pytest.fixture(scope="module")
def noisy_case(repeat_case, oracle):
    """the reads of the repeat fixture with substitutions, threaded by the references against the clean fixture's graph"""
    c, R = repeat_case, tsp.REPEAT
    reads = substituted(c["reads"], NOISY["rate"], NOISY["seed"])
    b = tus._oracle_batch(oracle, reads, R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], c["g"]["keys"], c["g"]["counts"], R["min_count"], tt.places_reference(c["uni"]),
                                start=b["start"], end=b["end"], n_unitigs=c["T"])
    return {"reads": reads, "paths": paths, "ro": c["uro"], "d": c["ud"], "uni_off": c["uni"]["uni_off"], "circular": c["uni"]["circular"]}


def _resolution(paths, c):
    sp = tsp.spans_reference(paths, c["uro"], c["ud"], c["uni"]["uni_off"])
    sk, sc = tsp.count_keys(sp["keys"])
    return sp, tsp.resolve_reference(c["uro"], c["ud"], c["T"], sk, sc, 2)


def test_clean_repeat_reads_come_out_as_they_went_in(repeat_case, oracle):
    """error-free reads on the graph they built: every join is an edge already followed, and the bridged paths equal the input field by
    field, matched == count"""
    c, R = repeat_case, tsp.REPEAT
    b = tus._oracle_batch(oracle, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], c["g"]["keys"], c["g"]["counts"], R["min_count"], tt.places_reference(c["uni"]),
                                start=b["start"], end=b["end"], n_unitigs=c["T"])
    ref = bridge_reference(paths, c["uro"], c["ud"], c["uni"]["uni_off"], c["uni"]["circular"], *DEFAULT)
    for f in STEP + ("path_off",):
        assert ref[f].tobytes() == paths[f].tobytes(), f
    assert ref["matched"].tobytes() == paths["count"].tobytes() and (ref["n_merged"], ref["n_bridged"]) == (0, 0)
    assert ref["n_steps"] == len(paths["unitig"]) == 112 and int((ref["join"] == 2).sum()) == ref["n_steps"] - len(c["reads"])


def test_noisy_repeat_reads_resolve_r_only_when_bridged(repeat_case, noisy_case):
    """1 % substitutions, seed 2: the plain paths resolve nothing; bridged (16, 2) they give the clean fixture's resolved and partner
    byte for byte, and no span key the clean reads do not give"""
    c, n = repeat_case, noisy_case
    sp, (resolved, partner, nc, nr) = _resolution(n["paths"], c)
    assert not resolved.any() and nr == 0
    ref = reference_of(n)
    check_bridge_invariants(ref, n, "noisy")
    bsp, (bres, bpar, bnc, bnr) = _resolution(ref, c)
    assert bres.tobytes() == c["resolved"].tobytes() and bpar.tobytes() == c["partner"].tobytes() and bnr == 1
    assert set(bsp["keys"].tolist()) <= set(c["ref"]["keys"].tolist()) and len(bsp["keys"]) > len(sp["keys"])
    print("noisy repeat reads: %d steps and %d span keys plain, %d steps and %d span keys bridged (%d merged, %d bridged)" % (
        len(n["paths"]["unitig"]), len(sp["keys"]), ref["n_steps"], len(bsp["keys"]), ref["n_merged"], ref["n_bridged"]))


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = 8
_dev, _host, _ptr = ts._dev, ts._host, ts._ptr
OUT_DT = dict({f: np.uint32 for f in OUT32}, path_off=np.uint64, join=np.uint8)
TDT = {np.uint64: "int64", np.uint32: "int32", np.uint8: "uint8"}
FILL = {np.uint64: -0x5A5A, np.uint32: -0x5A5A, np.uint8: 0xA5}


def _marked(h, frm=0):
    if h.dtype.itemsize == 1:
        return bool((h[frm:] == 0xA5).all())
    return bool((h[frm:].view(np.int64 if h.dtype.itemsize == 8 else np.int32) == -0x5A5A).all())


def raw_bridge(eng, case, limits=DEFAULT, capacity=None, want=OUT32 + ("path_off", "join"), null=(), ctx=True, **over):
    """s2k_paths_bridge through ctypes, guard words behind every output -> (status, n_out_steps, n_merged, n_bridged, host arrays
    with guards).  over: paths, ro, d, uni_off, circular replaced; T, n_edges, n_steps, n_reads given.  null: names of inputs (or
    `paths`, `out`, a counter) to pass as NULL"""
    import torch

    paths = over.get("paths", case["paths"])
    arr = {"ro": (case["ro"], np.uint64), "d": (case["d"], np.uint32), "uni_off": (case["uni_off"], np.uint64), "circular": (case["circular"], np.uint8)}
    dv = {k: _dev(over.get(k, a), dt) for k, (a, dt) in arr.items()}
    ns = over.get("n_steps", len(paths["unitig"]))
    nr = over.get("n_reads", len(paths["path_off"]) - 1)
    T, ne = over.get("T", len(case["uni_off"]) - 1), over.get("n_edges", len(case["d"]))
    dp = {f: _dev(paths[f], np.uint32) for f in STEP}
    dp["path_off"] = _dev(paths["path_off"], np.uint64)
    i = pkg.ThreadOut()
    i.capacity = ns
    for f, t in dp.items():
        if f not in null:
            setattr(i, f, t.data_ptr())
    cap = max(ns, 1) if capacity is None else capacity
    size = {f: cap for f in OUT32}
    size.update(path_off=nr + 1, join=max(ns, 1))
    res = {f: torch.full((size[f] + GUARD,), FILL[OUT_DT[f]], dtype=getattr(torch, TDT[OUT_DT[f]]), device="cuda:0") for f in want}
    o = pkg.ThreadOut()
    o.capacity = cap
    for f, t in res.items():
        if f not in ("matched", "join"):
            setattr(o, f, t.data_ptr())
    tot = [ctypes.c_uint64(777), ctypes.c_uint64(777), ctypes.c_uint64(777)]
    torch.cuda.synchronize()
    P = lambda k, empty=False: _ptr(dv[k], k in null or empty)  # noqa: E731
    s = eng.lib.s2k_paths_bridge(eng.ctx if ctx else None, nr, None if "paths" in null else ctypes.byref(i), ns, P("ro"),
                                 P("d", len(case["d"]) == 0 and "d" not in over), ne, P("uni_off"), P("circular"), T, limits[0], limits[1],
                                 None if "out" in null else ctypes.byref(o), _ptr(res["matched"]) if "matched" in res else None,
                                 _ptr(res["join"]) if "join" in res else None, *(None if "n%d" % k in null else ctypes.byref(x) for k, x in enumerate(tot)))
    return s, tot[0].value, tot[1].value, tot[2].value, {f: _host(t, OUT_DT[f]) for f, t in res.items()}


def device_bridge(eng, case, tag, limits=DEFAULT):
    """the call against the reference: every array, the totals, the guards; the sizes-only calls; capacity one short; some outputs
    NULL -> the reference"""
    ref = reference_of(case, limits)
    check_bridge_invariants(ref, case, tag)
    n, ns, nr = ref["n_steps"], len(case["paths"]["unitig"]), len(case["paths"]["path_off"]) - 1
    tot = (0, n, ref["n_merged"], ref["n_bridged"])
    s, no, nm, nb, got = raw_bridge(eng, case, limits, capacity=n)
    assert (s, no, nm, nb) == tot, (tag, s, no, nm, nb, tot)
    for f in OUT32:
        assert got[f][:n].tobytes() == ref[f].tobytes(), (tag, f, got[f][:8], ref[f][:8])
        assert _marked(got[f], n), (tag, f, "guard")
    assert got["path_off"][:nr + 1].tobytes() == ref["path_off"].tobytes() and _marked(got["path_off"], nr + 1), (tag, "path_off")
    assert got["join"][:ns].tobytes() == ref["join"].tobytes() and _marked(got["join"], ns), (tag, "join")
    for kw in (dict(want=("path_off",)), dict(want=("path_off", "join"), capacity=0)):  # the sizes: no step array, no capacity
        s, no, nm, nb, got = raw_bridge(eng, case, limits, **kw)
        assert (s, no, nm, nb) == tot, (tag, "sizes", kw)
        assert got["path_off"][:nr + 1].tobytes() == ref["path_off"].tobytes() and _marked(got["path_off"], nr + 1), (tag, "sizes", "path_off")
        assert "join" not in got or (got["join"][:ns].tobytes() == ref["join"].tobytes() and _marked(got["join"], ns)), (tag, "sizes", "join")
    if n:  # one short: nothing written, to any array
        s, no, nm, nb, got = raw_bridge(eng, case, limits, capacity=n - 1)
        assert (s, no, nm, nb) == (7,) + tot[1:] and all(_marked(x) for x in got.values()), (tag, "capacity")
        s, no, nm, nb, got = raw_bridge(eng, case, limits, capacity=n - 1, want=("path_off", "join", "matched"))  # matched alone is a step array too
        assert (s, no, nm, nb) == (7,) + tot[1:] and all(_marked(x) for x in got.values()), (tag, "capacity, matched")
    for want in (("path_off", "count", "flags", "matched"), ("path_off", "unitig", "pos", "item")):  # NULL optional outputs, start and end among them
        s, no, nm, nb, got = raw_bridge(eng, case, limits, want=want, capacity=n, null=("start", "end"))
        assert s == 0 and all(got[f][:len(ref[f])].tobytes() == ref[f].tobytes() and _marked(got[f], len(ref[f])) for f in got), (tag, want)
    return ref


@pytest.mark.gpu
def test_device_hand_made(eng):
    ref = device_bridge(eng, hand_case(), "hand", B_LIMITS)
    assert ref["join"].tolist() == [j for c in B_READS.values() for j in c[1]]
    for name, c in B_READS.items():  # every read alone
        one = device_bridge(eng, hand_case([c[0]]), name, B_LIMITS)
        assert one["join"].tolist() == c[1], name
    device_bridge(eng, hand_case([]), "no reads", B_LIMITS)
    device_bridge(eng, hand_case(), "hand, nothing to bridge", (0, 0))
    device_bridge(eng, hand_case(), "hand, the widest limits", (2 ** 32 - 1, 2 ** 32 - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", [1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 - 1, 3 * 2048 + 1])
def test_device_random_paths(eng, n_steps):
    """chains of short unitigs and walks of a random decomposition, gaps cut into both, cut to n_steps steps: round one wave, one tile
    and three tiles"""
    rng = np.random.default_rng(700 + n_steps)
    merged = bridged = 0
    for kind, limits in (("chained", (3, 1)), ("walked", (3, 1)), ("walked", DEFAULT)):
        case = gapped_case(rng, n_steps, kind)
        ref = device_bridge(eng, case, (kind, n_steps, limits), limits)
        merged, bridged = merged + ref["n_merged"], bridged + ref["n_bridged"]
    assert n_steps < 63 or (merged > 0 and bridged > 0)


@pytest.mark.gpu
def test_device_one_run_longer_than_two_tiles(eng):
    """5 000 steps on one unitig merge into one output step, then the same again in a second read: each run's head lies two tiles
    before its tail, and matched is a prefix difference across tiles"""
    case = runs_case(10000, [], [5000], T=1)
    ref = device_bridge(eng, case, "long run", (4, 0))
    assert ref["n_steps"] == 2 and ref["n_merged"] == 9998 and ref["matched"].tolist() == [5000, 5000] and ref["count"].tolist() == [14998, 14998]
    assert ref["pos"].tolist() == [0, 15000] and ref["path_off"].tolist() == [0, 1, 2]
    ref = device_bridge(eng, runs_case(5000, [], []), "long runs over three unitigs", (4, 0))
    assert ref["n_steps"] == 3 and ref["n_bridged"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [[2048], [2047], [2049], [1, 2049], [2046, 2048, 4096]])
def test_device_tile_run_and_read_boundaries(eng, cuts):
    """a run that ends on a tile's last step while the next starts on the next tile's first step, one step earlier and one later: cut
    by a gap in the read, by a read boundary, and by both at different places; then chains with gaps whose reads are cut there"""
    n_steps = 4097
    for run_cuts, read_cuts in ((cuts, []), ([], cuts), (cuts[:1], cuts[1:] + [2050]), ([c + 1 for c in cuts], cuts)):
        ref = device_bridge(eng, runs_case(n_steps, run_cuts, read_cuts), (cuts, run_cuts, read_cuts), (4, 0))
        assert ref["n_steps"] >= len(set(run_cuts) | set(read_cuts)) + 1
    rng = np.random.default_rng(sum(cuts))
    edges = [0] + cuts + [n_steps]
    case = with_gaps(rng, twk.chained_case(rng, 37, [b - a for a, b in zip(edges[:-1], edges[1:])], 0.05), p=0.2)
    device_bridge(eng, case, (cuts, "chained"), (3, 1))


@pytest.mark.gpu
def test_device_refusals_nothing_written(eng):
    rng = np.random.default_rng(73)
    case = with_gaps(rng, twk.chained_case(rng, 60, list(rng.integers(0, 40, size=200)), p_break=0.1))
    paths, ro, d, off = case["paths"], case["ro"], case["d"], case["uni_off"]
    ns, nr, T, ne = len(paths["unitig"]), len(paths["path_off"]) - 1, 60, len(d)
    assert ns > 2048 and device_bridge(eng, case, "base", (3, 1))["n_merged"] > 100

    def refused(code=1, **kw):
        s, no, nm, nb, got = raw_bridge(eng, case, (3, 1), **kw)
        assert (s, no, nm, nb) == (code, 0, 0, 0) and all(_marked(x) for x in got.values()), (s, no, nm, nb, list(kw))

    refused(ctx=False)
    for f in ("paths", "out", "path_off", "ro", "d", "uni_off", "circular", "unitig", "pos", "count", "item", "flags"):
        refused(null=(f,))
    refused(null=("start",))  # out->start wanted, the input has none
    refused(null=("end",))
    for k in range(3):  # a counter that is NULL: the others are not touched
        s, no, nm, nb, got = raw_bridge(eng, case, (3, 1), null=("n%d" % k,))
        assert s == 1 and sorted((no, nm, nb)) == [0, 0, 777] and all(_marked(x) for x in got.values())

    def changed(name, i, v, src=None):
        x = (src if src is not None else {"ro": ro, "d": d, "uni_off": off}[name]).copy()
        x[i] = v
        return {name: x}

    for r, v in ((0, 1), (5, 10 ** 9), (nr, ns - 1), (nr, ns + 1)):  # path_off: not from 0, decreasing, not ending at n_steps
        refused(paths=dict(paths, **changed("path_off", r, v, paths["path_off"])))
    for f, v in (("unitig", 2 * T), ("unitig", 2 ** 32 - 1), ("count", 0), ("count", 4), ("pos", 3)):  # a bad id; unitigs hold 1 .. 3 members
        refused(paths=dict(paths, **changed(f, ns // 2, v, paths[f])))
    starts = set(paths["path_off"].tolist())
    mid = next(s for s in range(ns // 2, ns) if s not in starts and paths["count"][s - 1] > 1)  # inside a read
    refused(paths=dict(paths, **changed("item", mid, int(paths["item"][mid - 1] + paths["count"][mid - 1]) - 1, paths["item"])))  # overlapping items
    refused(paths=dict(paths, **changed("item", mid, 0, paths["item"])))  # items that go backwards
    refused(paths=dict(paths, **changed("item", mid - 1, 2 ** 32 - 1, paths["item"])))  # item + count past 32 bits inside a read
    first = int(paths["path_off"][np.nonzero(np.diff(paths["path_off"].astype(np.int64)) > 0)[0][3]])
    ok = dict(paths, **changed("item", first, 0, paths["item"]))  # a read's first step may lie before the last of the read before it
    assert int(paths["item"][first - 1]) > 0 and raw_bridge(eng, case, (3, 1), paths=ok)[0] == 0
    refused(T=T - 1)
    for i, v in ((0, 1), (7, int(ro[8]) + 1), (2 * T, ne - 1), (2 * T, ne + 1)):
        refused(**changed("ro", i, v))
    refused(**changed("d", ne // 2, 2 * T))
    refused(**changed("uni_off", 11, int(off[10])))  # a unitig without a member
    big = off.copy()
    big[T] += np.uint64(2 ** 32)  # a unitig of 2^32 members
    refused(uni_off=big)
    z = ctypes.c_uint64(5)
    i, o = pkg.ThreadOut(), pkg.ThreadOut()
    i.path_off = o.path_off = 16
    P = ctypes.c_void_p(16)
    assert eng.lib.s2k_paths_bridge(eng.ctx, 1, ctypes.byref(i), 0, P, P, 2 ** 32, P, P, 1, 16, 2, ctypes.byref(o), None, None, ctypes.byref(z), ctypes.byref(z),
                                    ctypes.byref(z)) == 1 and z.value == 0  # before anything is read
    assert eng.lib.s2k_paths_bridge(eng.ctx, 1, ctypes.byref(i), 0, P, None, 0, P, P, 2 ** 31, 16, 2, ctypes.byref(o), None, None, ctypes.byref(z),
                                    ctypes.byref(z), ctypes.byref(z)) == 1
    # no steps: path_off zeroed, nothing else touched; and no reads
    for reads in ([[], [], []], []):
        empty = dict(case, paths=paths_of(reads))
        s, no, nm, nb, got = raw_bridge(eng, empty, (3, 1))
        assert (s, no, nm, nb) == (0, 0, 0, 0) and not got["path_off"][:len(reads) + 1].any() and _marked(got["path_off"], len(reads) + 1)
        assert all(_marked(got[f]) for f in got if f != "path_off")
    circ = dict(case, circular=np.ones(T, dtype=np.uint8))  # on a circular unitig a step may pass the last member, and nothing is joined
    s, no, nm, nb, got = raw_bridge(eng, circ, (3, 1), paths=dict(paths, **changed("count", first - 1, 9, paths["count"])))  # a read's last step
    assert (s, no, nm, nb) == (0, ns, 0, 0)


@pytest.mark.gpu
def test_device_deterministic(eng):
    rng = np.random.default_rng(74)
    case = with_gaps(rng, twk.chained_case(rng, 500, list(rng.integers(0, 200, size=300)), p_break=0.1))
    runs = []
    for _ in range(2):
        s, no, nm, nb, got = raw_bridge(eng, case, (3, 1))
        assert s == 0 and nm > 1000 and nb > 1000
        runs.append(b"".join(got[f].tobytes() for f in sorted(got)) + bytes(str((no, nm, nb)), "ascii"))
    assert runs[0] == runs[1]


def _read_paths(paths):
    """host path arrays -> pkg.ReadPaths on the GPU"""
    n = len(paths["unitig"])
    return pkg.ReadPaths(_dev(paths["path_off"], np.uint64)[:len(paths["path_off"])], **{f: _dev(paths[f], np.uint32)[:n] for f in STEP})


def _assert_bridged(got, ref, tag):
    h = got.host()
    for f in OUT32 + ("path_off",):
        assert h[f].tobytes() == ref[f].tobytes(), (tag, f)


@pytest.mark.gpu
def test_device_output_is_accepted_downstream(eng, tmp_path):
    """the bridged paths, as the device wrote them, go through s2k_paths_spans and s2k_paths_walks without refusal, and give what the
    references give on the reference's bridged paths; write_paths and write_gaf take them as they are"""
    rng = np.random.default_rng(75)
    base = twk.chained_case(rng, 60, list(rng.integers(0, 40, size=150)), p_break=0.05)
    case = with_gaps(rng, base)
    uni = base["uni"]
    ref = reference_of(case, (3, 1))
    s, no, nm, nb, got = raw_bridge(eng, case, (3, 1), capacity=ref["n_steps"])
    assert s == 0 and nm > 100 and nb > 100
    bridged = {f: got[f][:ref["n_steps"]] for f in STEP}
    bridged["path_off"] = got["path_off"][:len(ref["path_off"])]
    sp = tsp.spans_reference(ref, case["ro"], case["d"], case["uni_off"])
    s, nk, nf, nog, keys = tsp.raw_spans(eng, bridged, case["ro"], case["d"], case["uni_off"])
    assert (s, nk, nf, nog) == (0, len(sp["keys"]), sp["n_followed"], sp["n_off_graph"]) and keys[:nk].tobytes() == sp["keys"].tobytes()
    plain = tsp.spans_reference(case["paths"], case["ro"], case["d"], case["uni_off"])
    assert len(sp["keys"]) > len(plain["keys"]) and sp["n_followed"] > plain["n_followed"]
    wcase = dict(base, paths=bridged)
    wref = twk.reference_of(dict(base, paths=ref))
    s, nw, nf, nog, w = twk.raw_walks(eng, wcase, capacity=wref["n_walks"])
    assert (s, nw, nf, nog) == (0, wref["n_walks"], wref["n_followed"], wref["n_off_graph"])
    for f in twk.REC64 + twk.REC32:
        assert w[f][:nw].tobytes() == wref[f].tobytes(), f
    assert int(wref["items"].sum()) == int(ref["count"].astype(np.int64).sum()) > int(ref["matched"].astype(np.int64).sum())  # positions, not found k-min-mers
    # the Python layer on a graph object made of the same arrays
    ug = pkg.UnitigGraph(_dev(uni["uni_off"], np.uint64), _dev(uni["members"], np.uint32), None, None, _dev(uni["circular"], np.uint8), None,
                         _dev(np.zeros(len(case["d"])), np.uint64)[:len(case["d"])], None, _dev(case["ro"], np.uint64), _dev(case["d"], np.uint32))
    out, stats = ug.bridge(eng, _read_paths(case["paths"]), 3, 1)
    _assert_bridged(out, ref, "UnitigGraph.bridge")
    assert stats == {"steps_in": len(case["paths"]["unitig"]), "steps_out": ref["n_steps"], "merged": ref["n_merged"], "bridged": ref["n_bridged"]}
    keys, (nf, nog) = ug.spans(eng, out)
    assert tg._u64(keys).tobytes() == sp["keys"].tobytes()
    p = str(tmp_path / "bridged.paths")
    out.write_paths(p)
    q = str(tmp_path / "ref.paths")
    pkg.write_read_paths(q, ref["path_off"], ref["unitig"], ref["pos"], ref["count"], ref["flags"])
    assert open(p).read() == open(q).read() and len(open(p).read()) > 1000
    b = eng.paths_bridge(ug, _read_paths(case["paths"]), 3, 1, join=True)
    assert b["join"].cpu().numpy().tobytes() == ref["join"].tobytes()


@pytest.mark.gpu
def test_noisy_repeat_reads_end_to_end(eng, repeat_case, noisy_case, tmp_path):
    """the graph of the clean repeat reads, the reads with 1 % substitutions threaded through it, all on the device: the plain paths
    resolve nothing; after UnitigGraph.bridge the spans resolve R with the clean fixture's partners and untangle gives its two
    contigs; walks and GAF lines come out of the bridged paths as they are"""
    c, R, n = repeat_case, tsp.REPEAT, noisy_case
    clean = twk._extract_all(eng, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [clean], min_count=R["min_count"], min_edge_count=1)
    ug = graph.unitigs(eng)
    tsp._same_graph(ug, c["uro"], c["ud"], c["uni"])
    noisy = tt._extract_se(eng, n["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, noisy, len(n["reads"]), min_count=R["min_count"])
    table.close()
    got = paths.host()
    for f in STEP + ("path_off",):
        assert got[f].tobytes() == n["paths"][f].tobytes(), f
    resolved, partner, stats = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    assert stats == {"candidates": 1, "resolved": 0} and not resolved.cpu().numpy().any()
    bridged, bstats = ug.bridge(eng, paths)
    ref = reference_of(n)
    _assert_bridged(bridged, ref, "noisy")
    assert bstats == {"steps_in": paths.n_steps, "steps_out": ref["n_steps"], "merged": ref["n_merged"], "bridged": ref["n_bridged"]}
    assert bstats["steps_out"] < bstats["steps_in"] // 2
    resolved, partner, stats = ug.resolve(eng, ug.span_table(eng, [bridged]), min_support=2)
    assert stats == {"candidates": 1, "resolved": 1}
    assert resolved.cpu().numpy().tobytes() == c["resolved"].tobytes() and partner.cpu().numpy().view(np.uint32).tobytes() == c["partner"].tobytes()
    contigs, node_origin, ust = ug.untangle(eng, resolved, partner)
    assert ust["contigs"] == 2 and ust["duplicated"] == 1
    ns = pkg.NodeSequences.build(eng, graph, [clean])
    before, after = ug.walks(eng, paths, ns), ug.walks(eng, bridged, ns)
    assert after.n_walks < before.n_walks and after.n_followed > before.n_followed
    p = str(tmp_path / "bridged.gaf")
    after.write_gaf(p, ug)
    assert open(p).read().count("\n") == after.n_walks
    print("noisy repeat reads on the device: %d -> %d steps, %d -> %d walks, resolved 0 -> 1" % (paths.n_steps, bridged.n_steps, before.n_walks, after.n_walks))


@pytest.mark.gpu
def test_ecoli_reads_with_errors_through_the_simplified_graph(eng, ecoli):
    """the 600 reads with 0.5 % substitutions through simplify(10, 20): the device's bridged paths equal the reference's on the paths
    the device threaded; steps, walks, candidates and resolved before and after are printed, none of them asserted"""
    mc, l, k = 2, 12, 5
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    outs = twk._extract_all(eng, reads, l, k, 0.05, pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=mc, min_edge_count=1)
    ns = pkg.NodeSequences.build(eng, graph, [outs])
    sg, node_map, _ = graph.simplify(eng, 10, 20)
    ug = sg.unitigs(eng)
    table = pkg.CountTable(eng, sg.keys, sg.counts)
    paths = ug.thread(eng, table, outs, len(reads), min_count=mc)
    table.close()
    bridged, stats = ug.bridge(eng, paths)
    case = {"paths": paths.host(), "ro": tg._u64(ug.row_off), "d": ug.dst.cpu().numpy().view(np.uint32), "uni_off": tg._u64(ug.uni_off),
            "circular": ug.circular.cpu().numpy()}
    ref = reference_of(case)
    check_bridge_invariants(ref, case, "ecoli")
    _assert_bridged(bridged, ref, "ecoli")
    assert stats["steps_out"] <= stats["steps_in"] and stats == {"steps_in": paths.n_steps, "steps_out": ref["n_steps"], "merged": ref["n_merged"],
                                                                 "bridged": ref["n_bridged"]}
    sub = ns.subset(node_map)
    line = []
    for tag, p in (("plain", paths), ("bridged", bridged)):
        w = ug.walks(eng, p, sub)
        _, _, rs = ug.resolve(eng, ug.span_table(eng, [p]), min_support=2)
        line.append("%s: %d steps, %d walks, %d candidates, %d resolved" % (tag, p.n_steps, w.n_walks, rs["candidates"], rs["resolved"]))
    print("simplified E. coli, 0.5 %% substitutions, bridge(16, 2): %s; %d merged, %d bridged" % ("; ".join(line), stats["merged"], stats["bridged"]))
