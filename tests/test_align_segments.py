"""Segmented alignment (include/s2k.h: s2k_walks_segments, s2k_align_join).  CPU tier: serial references of the two rules
built on the references of test_align.py and test_walk.py, hand cases, properties of the joined alignment, and the conditions on the long
E. coli reads the device test runs on.  GPU tier: every output of the two calls entry for entry against the references, between guards."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import test_align as ta
import test_bridge as tb
import test_graph as tg
import test_simplify as ts
import test_span as tsp
import test_thread as tt
import test_unitig_sequences as tus
import test_unitigs as tu
import test_walk as twk
from test_bridge import noisy_case  # noqa: F401  (module-scoped fixtures of the repeat)
from test_span import repeat_case  # noqa: F401
from test_walk import repeat_walks  # noqa: F401

pkg = import_package()

SYMS = ("s2k_walks_segments", "s2k_align_join")
OVER, BAD_PATH = ta.OVER, ta.BAD_PATH
NO_STEP = 2 ** 64 - 1
SEG_LEN = 512
STATS = ("candidates", "outside", "admissible", "chosen", "walks_cut")
WALK_F = ("walk_off", "first_step", "n_steps", "qstart", "qend", "path_start", "path_end", "flags")
SEG_F = ("seg_off", "q_begin", "q_end", "t_begin", "t_end")


# ---- the references ----------------------------------------------------------------------------------------------------------------
def segments_reference(c, seg_len=SEG_LEN):
    """the rule of include/s2k.h, item by item.  c: walks (the arrays of walks_reference), paths (unitig, pos, count of the walks'
    steps), uni, mo, seq_len, q_begin, tgt_off, bad, src (path_off, pos, count, item), src_step / src_pos (None: identity / src pos),
    km_off, start -> dict seg_off, q_begin, q_end, t_begin, t_end (uint64), stats (list of five), cuts (per walk)"""
    W, uni, mo = c["walks"], c["uni"], c["mo"]
    fs, ns, qs, qe, ps, fl = ([int(x) for x in W[f]] for f in ("first_step", "n_steps", "qstart", "qend", "path_start", "flags"))
    u, p, cn = ([int(x) for x in c["paths"][f]] for f in ("unitig", "pos", "count"))
    oo, uo = [int(x) for x in mo["out_off"]], [int(x) for x in uni["uni_off"]]
    L = lambda U: oo[(U >> 1) + 1] - oo[U >> 1]  # noqa: E731
    A = [0]
    for U in u:
        A.append(A[-1] + L(U) - min(int(mo["overlap"][U]), L(U)))
    toff, bad = [int(x) for x in c["tgt_off"]], [int(x) for x in c["bad"]]
    so, sp, sc, si = ([int(x) for x in c["src"][f]] for f in ("path_off", "pos", "count", "item"))
    if c.get("src_pos") is not None:
        sp = [int(x) for x in c["src_pos"]]
    sstep = None if c.get("src_step") is None else [int(x) for x in c["src_step"]]
    km, start = [int(x) for x in c["km_off"]], [int(x) for x in c["start"]]
    nw = len(fs)
    holder = {S: w for w in range(nw) for S in range(fs[w], fs[w] + ns[w])}
    cand, n_out = [[] for _ in range(nw)], 0
    for R in range(len(so) - 1):
        for r in range(so[R], so[R + 1]):
            S = r if sstep is None else sstep[r]
            w = holder.get(S)  # (NO_STEP is no step of the paths)
            for i in range(sc[r]):
                x = sp[r] + i
                if w is None or not (p[S] <= x < p[S] + cn[S]) or x >= uo[(u[S] >> 1) + 1] - uo[u[S] >> 1] or fl[w] & 1 or bad[w]:
                    n_out += 1
                    continue
                lo = twk.interval_reference(uni, mo, c["seq_len"], u[S], x)[0]
                cand[w].append((start[km[R] + si[r] + i] - qs[w], A[S] - A[fs[w]] + lo - ps[w]))
    seg_off, out, cuts_of = [0], {f: [] for f in SEG_F[1:]}, []
    n_adm = n_chosen = n_cut = 0
    for w in range(nw):
        m, n = qe[w] - qs[w], toff[w + 1] - toff[w]
        mq = mt = None
        adm = []
        for qc, tc in cand[w]:
            if 0 < qc < m and 0 < tc < n and (mq is None or qc > mq) and (mt is None or tc > mt):
                adm.append((qc, tc))
            mq, mt = (qc, tc) if mq is None else (max(mq, qc), max(mt, tc))
        chosen = [a for i, a in enumerate(adm) if a[0] // seg_len >= 1 and (i == 0 or adm[i - 1][0] // seg_len != a[0] // seg_len)]
        n_adm, n_chosen, n_cut = n_adm + len(adm), n_chosen + len(chosen), n_cut + bool(chosen)
        cuts = [(0, 0), (0, 0)] if bad[w] else [(0, 0)] + chosen + [(m, n)]
        cuts_of.append(cuts)
        for a, b in zip(cuts, cuts[1:]):
            out["q_begin"].append(int(c["q_begin"][w]) + a[0])
            out["q_end"].append(int(c["q_begin"][w]) + b[0])
            out["t_begin"].append(toff[w] + a[1])
            out["t_end"].append(toff[w] + b[1])
        seg_off.append(len(out["q_begin"]))
    res = {f: np.array(v, dtype=np.uint64) for f, v in out.items()}
    res.update(seg_off=np.array(seg_off, dtype=np.uint64), stats=[sum(len(x) for x in cand), n_out, n_adm, n_chosen, n_cut], cuts=cuts_of)
    return res


def join_reference(seg_off, bad, seg):
    """the join of include/s2k.h.  seg: what align_many_reference returns for the segments (edits, flags, n_ops, matches, ops per
    segment) -> the same dict per walk, ops_off compact"""
    so = [int(x) for x in seg_off]
    res = []
    for w in range(len(so) - 1):
        ss = range(so[w], so[w + 1])
        if bad[w]:
            res.append((0, BAD_PATH, [], 0))
        elif any(int(seg["flags"][s]) & OVER for s in ss):
            res.append((sum(int(seg["edits"][s]) for s in ss), OVER, [], 0))
        else:
            runs = []
            for s in ss:
                for k, v in enumerate(seg["ops"][s][:int(seg["n_ops"][s])]):
                    ln, op = int(v) >> 4, int(v) & 15
                    if k == 0 and s > so[w] and int(seg["n_ops"][s - 1]) and int(seg["ops"][s - 1][int(seg["n_ops"][s - 1]) - 1]) & 15 == op:
                        runs[-1][0] += ln
                    else:
                        runs.append([ln, op])
            if any(ln >= 2 ** 28 for ln, _ in runs):
                raise ValueError("a joined run of 2^28 bases or more")
            res.append((sum(int(seg["edits"][s]) for s in ss), 0, [(ln, op) for ln, op in runs], sum(int(seg["matches"][s]) for s in ss)))
    return {"edits": np.array([r[0] for r in res], dtype=np.uint32), "flags": np.array([r[1] for r in res], dtype=np.uint32),
            "n_ops": np.array([len(r[2]) for r in res], dtype=np.uint32), "matches": np.array([r[3] for r in res], dtype=np.uint32),
            "ops_off": np.concatenate([[0], np.cumsum([len(r[2]) for r in res])]).astype(np.uint64),
            "ops": [np.array([ln << 4 | op for ln, op in r[2]], dtype=np.uint32) for r in res], "res": res}


def segment_pairs(sg, query, target):
    return [(bytes(query[int(a):int(b)]), bytes(target[int(x):int(y)])) for a, b, x, y in zip(sg["q_begin"], sg["q_end"], sg["t_begin"], sg["t_end"])]


def segmented_reference(c, query, target, seg_len=SEG_LEN, max_edits=ta.MAX_EDITS):
    """what UnitigGraph.align_segmented gives: segments -> align_many_reference on the segment pairs -> join"""
    sg = segments_reference(c, seg_len)
    seg = ta.align_many_reference(segment_pairs(sg, query, target), max_edits)
    al = join_reference(sg["seg_off"], c["bad"], seg)
    al.update(sg=sg, seg=seg)
    return al


# ---- hand-made anchors -----------------------------------------------------------------------------------------------------------------
Q0, P0 = 100, 1000  # qstart and path_start of every hand-made walk


def anchor_case(walks, shift=None, no_step=(), src_step=None, per_read=1):
    """One read and one step per walk on ONE linear unitig whose member offsets are set freely (they need only lie inside the
    unitig's bases), so that every candidate's (qc, tc) is what the case says.  walks: dicts with cand = [(qc, tc)], m, n and
    optionally circular, bad.  Items are the source's items: identity map, the same step -- unless shift[w] = d moves walk w's source
    step d positions to the left (its first d items then lie outside the step), or w is in no_step (its source step has no step).
    per_read: so many consecutive walks share a read."""
    n_items = sum(len(w["cand"]) for w in walks) + 1  # one more member: every step stays inside the unitig
    span = P0 + max([tc for w in walks for _, tc in w["cand"]] + [0]) + 50
    mem_off, steps, start = [], [], []
    for w in walks:
        steps.append((len(mem_off), len(w["cand"])))
        for qc, tc in w["cand"]:
            mem_off.append(P0 + tc)
            start.append(Q0 + qc)
    nw = len(walks)
    rd = list(range(0, nw, per_read)) + [nw]  # the first walk of every read
    item0 = np.array([steps[i][0] - steps[rd[i // per_read]][0] for i in range(nw)], dtype=np.uint32)  # a walk's first item in its read
    km_off = [steps[i][0] for i in rd[:-1]] + [len(start)]
    mem_off.append(span - 30)
    uni = {"uni_off": np.array([0, n_items], dtype=np.uint64), "members": np.arange(0, 2 * n_items, 2, dtype=np.uint32), "circular": np.zeros(1, dtype=np.uint8)}
    mo = {"member_off": np.array(mem_off, dtype=np.uint64), "out_off": np.array([0, span], dtype=np.uint64), "overlap": np.zeros(2, dtype=np.uint32)}
    keep = [i for i in range(nw) if steps[i][1]]  # a walk without a candidate has a step of its own all the same: one item, outside
    pos = np.array([s[0] for s in steps], dtype=np.uint32)
    cnt = np.array([max(s[1], 1) for s in steps], dtype=np.uint32)
    W = {"walk_off": np.array(rd, dtype=np.uint64), "first_step": np.arange(nw, dtype=np.uint64), "n_steps": np.ones(nw, dtype=np.uint32),
         "qstart": np.full(nw, Q0, dtype=np.uint32), "qend": np.array([Q0 + w["m"] for w in walks], dtype=np.uint32),
         "path_start": np.full(nw, P0, dtype=np.uint64), "path_end": np.array([P0 + w["n"] for w in walks], dtype=np.uint64),
         "flags": np.array([int(w.get("circular", 0)) for w in walks], dtype=np.uint32)}
    sh = np.array([(shift or {}).get(i, 0) for i in range(nw)], dtype=np.int64)
    src = {"path_off": np.array(rd, dtype=np.uint64), "pos": (pos - sh).astype(np.uint32), "count": np.array([s[1] for s in steps], dtype=np.uint32),
           "item": item0}
    if not all(steps[i][1] for i in range(nw)):  # a read without an item has no source step
        src = {"path_off": np.concatenate([[0], np.cumsum([1 if steps[i][1] else 0 for i in range(nw)])]).astype(np.uint64)[rd],
               "pos": src["pos"][keep], "count": src["count"][keep], "item": src["item"][keep]}
        src_step = np.array(keep, dtype=np.uint64) if src_step is None else src_step
    if no_step:
        src_step = np.arange(nw, dtype=np.uint64) if src_step is None else src_step.copy()
        for i in no_step:
            src_step[keep.index(i) if len(keep) < nw else i] = NO_STEP
    toff = np.concatenate([[0], np.cumsum([0 if w.get("bad") else w["n"] for w in walks])]).astype(np.uint64)
    return {"walks": W, "paths": {"unitig": np.zeros(nw, dtype=np.uint32), "pos": pos, "count": cnt}, "uni": uni, "mo": mo,
            "seq_len": np.full(n_items, 30, dtype=np.uint32), "q_begin": (7 + 4000 * np.arange(nw)).astype(np.uint64), "tgt_off": toff,
            "bad": np.array([int(w.get("bad", 0)) for w in walks], dtype=np.uint8), "src": src, "src_step": src_step, "src_pos": None,
            "km_off": np.array(km_off, dtype=np.uint64), "start": np.array(start, dtype=np.uint32)}


def _w(cand, m=3000, n=3000, **kw):
    return dict(cand=cand, m=m, n=n, **kw)


# name -> (walks, keyword arguments of anchor_case, the cuts each walk must get between (0, 0) and (m, n), stats)
HAND = {
    "ends are no anchors": ([_w([(0, 600), (600, 0), (700, 700), (2500, 2500), (3000, 2600), (2600, 3000)])], {}, [[(700, 700), (2500, 2500)]],
                            [6, 0, 2, 2, 1]),
    "an anchor behind the ends stops the later ones": ([_w([(600, 600), (3000, 700), (2000, 2000)]), _w([(600, 600), (700, 3000), (2000, 2000)])], {},
                                                       [[(600, 600)], [(600, 600)]], [6, 0, 2, 2, 2]),
    "tc must pass the maximum": ([_w([(600, 900), (1200, 800), (1800, 850), (2400, 900), (2500, 901)])], {}, [[(600, 900), (2500, 901)]], [5, 0, 2, 2, 1]),
    "qc must pass the maximum": ([_w([(1200, 600), (700, 700), (1200, 800), (1800, 900)])], {}, [[(1200, 600), (1800, 900)]], [4, 0, 2, 2, 1]),
    "the first of a bucket wins": ([_w([(520, 500), (530, 510), (1023, 900), (1024, 1000), (1030, 1010)])], {}, [[(520, 500), (1024, 1000)]], [5, 0, 5, 2, 1]),
    "bucket 0 is never chosen": ([_w([(100, 90), (511, 500)]), _w([(100, 90), (511, 500), (512, 501)])], {}, [[], [(512, 501)]], [5, 0, 5, 1, 1]),
    "no candidate, bad, circular": ([_w([]), _w([(600, 600)], bad=1), _w([(600, 600)], circular=1), _w([(600, 600)])], {},
                                    [[], None, [], [(600, 600)]], [1, 2, 1, 1, 1]),
    "outside its step, and no step": ([_w([(600, 600), (1200, 1200)]), _w([(600, 600), (1200, 1200)]), _w([(600, 600)])], dict(shift={1: 1}, no_step=(2,)),
                                      [[(600, 600), (1200, 1200)], [(1200, 600)], []], [3, 2, 3, 3, 2]),
    "negative offsets": ([_w([(-50, 600), (600, -50), (700, 650)])], {}, [[(700, 650)]], [3, 0, 1, 1, 1]),
}


def hand_pairs_for(c, rng):
    """a query pool and a target pool under the intervals of a hand case: random bytes, so the segments align with edits"""
    nq = int(c["q_begin"][-1]) + int(c["walks"]["qend"][-1]) + 8
    return np.frombuffer(ta.random_seq(rng, nq), dtype=np.uint8), np.frombuffer(ta.random_seq(rng, int(c["tgt_off"][-1]) + 8), dtype=np.uint8)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    facade = open(os.path.join(ROOT, "include", "s2k.hpp")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header and s in facade, s
    assert hasattr(pkg.Engine, "walks_segments") and hasattr(pkg.Engine, "align_join") and hasattr(pkg.UnitigGraph, "align_segmented")
    assert "origin" in pkg.UnitigGraph.bridge.__code__.co_varnames and hasattr(pkg, "PathOrigin")


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "segment_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "segment_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    S = pkg.SegmentOut
    assert facts["sizeof.s2k_segment_out"] == (ctypes.sizeof(S),)
    for f, t in S._fields_:
        assert facts["s2k_segment_out." + f] == (getattr(S, f).offset, ctypes.sizeof(t)), f
    assert facts["S2K_NO_STEP"] == (pkg.NO_STEP,) == (NO_STEP,) and facts["S2K_SEGMENT_LEN"] == (pkg.SEGMENT_LEN,) == (SEG_LEN,)
    assert facts["S2K_SEGMENT_MIN_LEN"] == (pkg.SEGMENT_MIN_LEN,) == (64,)
    assert facts["S2K_SEGMENT_STATS"] == (pkg.SEGMENT_STATS_WORDS,) and pkg.SEGMENT_STATS == STATS and len(STATS) <= pkg.SEGMENT_STATS_WORDS


def test_cpp_segment_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "segment_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "segment_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "s2k_segment.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))
    assert "s2k_segment.hip" in next(line for line in open(os.path.join(csrc, "Makefile.asan")).read().split("\n") if line.startswith("ASAN_SRCS"))
    assert os.path.exists(os.path.join(csrc, "s2k_segment.hip"))


def test_segments_reference_hand_cases():
    for name, (walks, kw, want, stats) in HAND.items():
        c = anchor_case(walks, **kw)
        ref = segments_reference(c)
        for w, cuts in enumerate(ref["cuts"]):
            m, n = walks[w]["m"], walks[w]["n"]
            assert cuts == ([(0, 0), (0, 0)] if want[w] is None else [(0, 0)] + want[w] + [(m, n)]), (name, w, cuts)
        assert ref["stats"] == stats, (name, ref["stats"])
        assert ref["seg_off"].tolist() == np.concatenate([[0], np.cumsum([1 if x is None else len(x) + 1 for x in want])]).tolist(), name
        a, b = int(ref["seg_off"][0]), int(ref["seg_off"][1])
        assert int(ref["q_begin"][a]) == 7 and int(ref["t_begin"][a]) == 0 and int(ref["q_end"][b - 1]) == 7 + (0 if want[0] is None else walks[0]["m"]), name
    # another seg_len moves the buckets: 64 takes the first anchor of every 64 query bases
    c = anchor_case([_w([(63, 60), (64, 61), (65, 62), (127, 100), (128, 101), (200, 150)])])
    assert segments_reference(c, 64)["cuts"][0] == [(0, 0), (64, 61), (128, 101), (200, 150), (3000, 3000)]
    assert segments_reference(c, 512)["cuts"][0] == [(0, 0), (3000, 3000)]


def _seg(*cigars, over=()):
    """segments from CIGAR texts -> the dict of align_many_reference (edits = the bases that are not =; an over segment has none)"""
    code = {v: k for k, v in ta.OPS.items()}
    res = []
    for i, text in enumerate(cigars):
        runs, num = [], ""
        for ch in text:
            if ch.isdigit():
                num += ch
            else:
                runs.append((int(num), code[ch]))
                num = ""
        res.append((256, OVER, [], 0) if i in over else (sum(ln for ln, op in runs if op != 7), 0, runs, sum(ln for ln, op in runs if op == 7)))
    slots = [0 if r[1] else 2 * r[0] + 1 for r in res]
    return {"edits": np.array([r[0] for r in res], dtype=np.uint32), "flags": np.array([r[1] for r in res], dtype=np.uint32),
            "n_ops": np.array([len(r[2]) for r in res], dtype=np.uint32), "matches": np.array([r[3] for r in res], dtype=np.uint32),
            "ops_off": np.concatenate([[0], np.cumsum(slots)]).astype(np.uint64),
            "ops": [np.array([ln << 4 | op for ln, op in r[2]], dtype=np.uint32) for r in res]}


# name -> (segment CIGARs, over segments, seg_off, bad, the joined CIGAR / flags per walk, edits per walk)
JOIN_HAND = {
    "= | = merges": (["5=", "7="], (), [0, 2], [0], ["12="], [0]),
    "three all-= segments collapse": (["5=", "7=", "9="], (), [0, 3], [0], ["21="], [0]),
    "I | I merges": (["5=2I", "3I4="], (), [0, 2], [0], ["5=5I4="], [5]),
    "D | I does not merge": (["5=2D", "3I4="], (), [0, 2], [0], ["5=2D3I4="], [5]),
    "X | X merges, = in between does not": (["2=1X", "1X2=", "1X3="], (), [0, 3], [0], ["2=2X2=1X3="], [3]),
    "a walk's first run never merges": (["5=", "7="], (), [0, 1, 2], [0, 0], ["5=", "7="], [0, 0]),
    "an over segment flags the walk": (["5=", "", "7=1X"], (1,), [0, 3], [0], [OVER], [257]),
    "a bad walk": (["5=", "", "7="], (), [0, 1, 2, 3], [0, 1, 0], ["5=", BAD_PATH, "7="], [0, 0, 0]),
    "an empty segment in between keeps the runs apart": (["5=", "", "7="], (), [0, 3], [0], ["5=7="], [0]),
    "a walk without a segment": (["5="], (), [0, 0, 1], [0, 0], ["", "5="], [0, 0]),
}


def test_join_reference_hand_cases():
    for name, (cig, over, seg_off, bad, want, edits) in JOIN_HAND.items():
        j = join_reference(seg_off, bad, _seg(*cig, over=over))
        for w, x in enumerate(want):
            if isinstance(x, str):
                assert (ta.cigar_of(j["res"][w][2]), int(j["flags"][w])) == (x, 0), (name, w, ta.cigar_of(j["res"][w][2]))
                assert int(j["matches"][w]) == sum(ln for ln, op in j["res"][w][2] if op == 7), name
            else:
                assert (int(j["flags"][w]), int(j["n_ops"][w]), int(j["matches"][w])) == (x, 0, 0), (name, w)
        assert j["edits"].tolist() == edits and j["ops_off"].tolist() == np.concatenate([[0], np.cumsum(j["n_ops"])]).tolist(), name
    with pytest.raises(ValueError):
        join_reference([0, 2], [0], _seg("%d=" % (2 ** 27), "%d=" % (2 ** 27)))


def planted_pair(rng, n_blocks, gap=80):
    """a pair with one planted edit in the middle of every block of `gap` bases (a substitution, a base only q has, a base only t has,
    in turn) and the cuts at the block borders, where both strings match for gap / 2 - 1 >= 32 bases to either side"""
    q, t, cuts = bytearray(), bytearray(), []
    for b in range(n_blocks):
        s = bytearray(ta.random_seq(rng, gap))
        x = bytearray(s)
        kind, i = b % 3, gap // 2
        if kind == 0:
            x[i] = b"ACGT"[(b"ACGT".index(x[i]) + 1) % 4]
        elif kind == 1:
            del x[i]
        else:
            x.insert(i, b"ACGT"[(b"ACGT".index(x[i]) + 1) % 4])
        q += s
        t += x
        cuts.append((len(q), len(t)))
    return bytes(q), bytes(t), cuts[:-1]


def joined_over_cuts(q, t, cuts, max_edits=ta.MAX_EDITS):
    cuts = [(0, 0)] + list(cuts) + [(len(q), len(t))]
    seg = ta.align_many_reference([(q[a[0]:b[0]], t[a[1]:b[1]]) for a, b in zip(cuts, cuts[1:])], max_edits)
    return join_reference([0, len(cuts) - 1], [0], seg)


def test_joined_alignments_are_valid_and_optimal_between_planted_cuts():
    rng = np.random.default_rng(220)
    worse = 0
    for it in range(60):  # random pairs, random valid cuts: any strictly increasing cuts give an alignment, seldom the best one
        q = ta.random_seq(rng, int(rng.integers(40, 400)))
        t = ta.mutated(rng, q, int(rng.integers(0, 30)))
        cuts = []
        for qc in sorted(set(rng.integers(1, len(q), size=int(rng.integers(0, 6))).tolist())):  # tc within 12 bases of qc, strictly increasing
            tc = qc + int(rng.integers(-12, 13))
            if 0 < tc < len(t) and (not cuts or tc > cuts[-1][1]):
                cuts.append((qc, tc))
        j = joined_over_cuts(q, t, cuts)
        res = j["res"][0]
        ta.check_alignment(q, t, res, (it, cuts))
        d = ta.edit_distance_dp(q, t)
        assert res[0] >= d, (it, res[0], d)
        worse += res[0] > d
    assert worse > 10
    for it in range(20):  # cuts at planted matches with no edit within 32 bases: the distance itself
        q, t, cuts = planted_pair(rng, int(rng.integers(2, 12)))
        j = joined_over_cuts(q, t, cuts)
        res = j["res"][0]
        ta.check_alignment(q, t, res, ("planted", it))
        assert res[0] == ta.edit_distance_dp(q, t) == len(cuts) + 1, (it, res[0])
        assert len(res[2]) <= 2 * res[0] + 1  # the all-= borders merged: no more runs than one alignment would have


# ---- the long E. coli reads ---------------------------------------------------------------------------------------------------------------
# sample_reads_with_errors(ecoli, n, seed, 0.005, lo, hi), bridged with `limits`.  From 40 reads of 30-50 kbp bridged (16, 2) the references
# gave 774 walks, the longest of 14.7 kbp: a substitution that makes or removes a minimizer shifts the read's items against the graph's
# positions by more than 2, so the paths of long reads break every 2 kbp.  With (32, 8) the walks reach their reads' lengths (68 walks, 39
# above 20 kbp) -- but the solid draft is nearly clean, the walks carry the reads' 0.5 % alone, and 255 edits take 50 kbp: 4 of the 39 were
# over.  Hence reads of 70-95 kbp of the 100 kbp genome.
LONG = dict(n=16, seed=11, lo=70000, hi=95000, limits=(32, 8))


def q_begin_of(walks, read_off):
    wo = walks["walk_off"].astype(np.int64)
    read = np.repeat(np.arange(len(wo) - 1), np.diff(wo))
    return (np.asarray(read_off).astype(np.uint64)[read] + walks["qstart"].astype(np.uint64)).astype(np.uint64)


def bridged_case(graph, b, src, bridged):
    """the case of segments_reference for walks made on `bridged` = bridge_reference(src, ..): graph holds uni, ro, d, nodes, mo,
    strings, overlap; b the oracle's batch of the reads"""
    bpaths = {f: bridged[f] for f in tb.STEP + ("path_off",)}
    walks = twk.reference_of(dict(graph, paths=bpaths))
    toff, tgt, bad = ta.targets_reference(walks, bpaths["unitig"], graph["strings"], graph["overlap"])
    return {"walks": walks, "paths": bpaths, "uni": graph["uni"], "mo": graph["mo"], "seq_len": graph["nodes"]["seq_len"],
            "q_begin": q_begin_of(walks, b["read_off"]), "tgt_off": toff, "bad": bad, "src": src,
            "src_step": (np.cumsum(bridged["join"] != 1) - 1).astype(np.uint64), "src_pos": None, "km_off": b["km_off"], "start": b["start"], "tgt": tgt}


@pytest.fixture(scope="module")
def ecoli_long(oracle, ecoli):
    """the graph of ecoli_reference in test_align.py (600 reads at 0.5 %, Regular 12 / 5, simplify(10, 20)) and a second read set, long
    reads at 0.5 %, threaded and bridged (16, 2) through it by the references: the walks, whole-walk alignments, segmented alignments"""
    mode, l, k = tsp.MODES[0]
    mc = 2
    reads600 = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    b = tus._oracle_batch(oracle, reads600, l, k, 0.05, mode)
    full = tg.graph_reference([b], mc, 1)
    final, ref_map, _ = ts.simplify_rounds_reference(full, 10, 20)
    uni, uro, ud, _ = ts.unitig_view(final)
    all_nodes = tus.node_sequences_reference([b], full["keys"], k)
    kept = np.nonzero(ref_map >= 0)[0]
    nodes = {f: np.asarray(all_nodes[f])[kept] for f in ("rep", "seq_off", "seq_len", "shift_fwd", "shift_rev", "rev")}
    nodes["pool"] = all_nodes["pool"]
    seqs = tus.unitig_sequences_reference(uni, nodes)
    graph = {"ro": uro, "d": ud, "uni": uni, "nodes": nodes, "mo": twk.member_offsets_reference(uni, nodes), "strings": tus.unitig_strings(uni, seqs),
             "overlap": seqs["overlap"]}
    reads = ts.sample_reads_with_errors(ecoli, LONG["n"], LONG["seed"], 0.005, LONG["lo"], LONG["hi"])
    lb = tus._oracle_batch(oracle, reads, l, k, 0.05, mode)
    src = tt.thread_reference(lb["km_off"], lb["hash"], lb["rev"], final["keys"], final["counts"], mc, tt.places_reference(uni), start=lb["start"],
                              end=lb["end"], n_unitigs=uni["n_unitigs"])
    br = tb.bridge_reference(src, uro, ud, uni["uni_off"], uni["circular"], *LONG["limits"])
    case = bridged_case(graph, lb, src, br)
    whole = ta.walk_alignments_reference(case["walks"], case["paths"]["unitig"], graph["strings"], graph["overlap"], reads)
    seg = segmented_reference(case, lb["bases"], np.frombuffer(case["tgt"], dtype=np.uint8))
    return {"reads": reads, "reads600": reads600, "case": case, "whole": whole, "seg": seg, "graph": graph}


def test_ecoli_long_reads_pass_max_edits_whole_and_none_does_in_segments(ecoli_long):
    """conditions on the input of the device test, by the references alone: plain whole-walk alignment flags at least half of the walks
    of more than 20 kbp over; cut at seg_len 512 none of them is over and no segment is; at least 95 % of all walks have flags 0.
    The references say (printed by this test): 37 walks of 16 reads, 16 of them above 20 kbp, all 16 over whole and none segmented;
    2 551 segments, none over, the largest segment distance 11; 6 955 edits in all; 96 687 candidates, 96 650 admissible, 2 514 chosen."""
    e = ecoli_long
    W, whole, seg = e["case"]["walks"], e["whole"], e["seg"]
    n = W["n_walks"]
    long_w = (W["qend"].astype(np.int64) - W["qstart"]) > 20000
    over_whole = (whole["flags"] & OVER) != 0
    over_seg = (seg["flags"] & OVER) != 0
    seg_over = (seg["seg"]["flags"] & OVER) != 0
    print("E. coli, %d long reads: %d walks, %d above 20 kbp of which %d over whole and %d over segmented; %d segments, %d over, the largest segment "
          "distance %d; %d edits in all segmented, %d walks with flags 0, %d bad; anchors: %s" % (
              len(e["reads"]), n, int(long_w.sum()), int((over_whole & long_w).sum()), int((over_seg & long_w).sum()), len(seg_over), int(seg_over.sum()),
              int(seg["seg"]["edits"][~seg_over].max()), int(seg["edits"].sum()), int((seg["flags"] == 0).sum()), int(e["case"]["bad"].sum()),
              dict(zip(STATS, seg["sg"]["stats"]))))
    assert int(long_w.sum()) >= 10 and 2 * int((over_whole & long_w).sum()) >= int(long_w.sum())
    assert not (over_seg & long_w).any() and not seg_over.any()
    assert int((seg["flags"] == 0).sum()) >= 0.95 * n
    for w in np.nonzero(seg["flags"] == 0)[0][::7]:
        q, t = whole["pairs"][w]
        ta.check_alignment(q, t, seg["res"][w], w)
        if not over_whole[w]:  # where the whole walk can be aligned the cuts cost little or nothing
            assert whole["edits"][w] <= seg["edits"][w] <= whole["edits"][w] + 8, (w, whole["edits"][w], seg["edits"][w])


# ---- generators -------------------------------------------------------------------------------------------------------------------
def many_anchors(n, step=20):
    """one walk with n anchors `step` bases apart, all admissible"""
    return anchor_case([_w([(step * (i + 1), step * (i + 1) + i % 3) for i in range(n)], m=step * (n + 2), n=step * (n + 2) + 5)])


def many_walks(rng, nw, per_read=1):
    walks = []
    for _ in range(nw):
        k = int(rng.integers(0, 7))
        qc = np.maximum(np.cumsum(rng.integers(-40, 400, size=k)), -60)  # now and then backwards: not admissible
        tc = qc + rng.integers(-30, 30, size=k)
        walks.append(_w(list(zip(qc.tolist(), tc.tolist())), bad=int(rng.random() < 0.05), circular=int(rng.random() < 0.05)))
    return anchor_case(walks, per_read=per_read)


def walked_segments_case(rng, n_keys, lens, drop=0.08, max_len=6):
    """reads that walk a random decomposition (as twk.walked_case, with its circular unitigs, twin strands and junctions above a length),
    their walks and targets by the references, and a SOURCE made up from the walks' paths: every step cut into one to three source
    steps, some without a step (NO_STEP), some moved a position to the left or right; the reads' starts rise with some noise"""
    keys, cnt = tg._random_table(rng, n_keys)
    uni = tt.random_unitigs(rng, len(keys), max_len=max_len, p_cycle=0.1)
    km_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    h, rv = tt.walk_items(rng, km_off, keys, uni, gap=0.02, jump=0.02)
    n = len(h)
    start = np.zeros(n, dtype=np.int64)
    for a, b in zip(km_off[:-1].astype(np.int64), km_off[1:].astype(np.int64)):
        start[a:b] = 50 + np.cumsum(rng.integers(-3, 40, size=b - a))
    start = np.maximum(start, 0).astype(np.uint32)
    paths = tt.thread_reference(km_off, h, rv, keys, cnt, 1, tt.places_reference(uni), start=start, end=start + np.uint32(30), n_unitigs=uni["n_unitigs"])
    u, f = paths["unitig"].tolist(), paths["flags"].tolist()
    edges = [(u[s - 1], u[s]) for s in range(1, len(u)) if f[s] & twk.LINKED and not uni["circular"][u[s] >> 1] and not uni["circular"][u[s - 1] >> 1]
             and rng.random() < 0.8]
    ro, d = tu.csr_of(uni["n_unitigs"], edges)
    nodes = twk.random_records(rng, len(keys))
    mo = twk.member_offsets_reference(uni, nodes)
    walks = twk.reference_of({"paths": paths, "ro": ro, "d": d, "uni": uni, "mo": mo, "nodes": nodes})
    strings = ta.random_strings(rng, mo)
    toff, tgt, bad = ta.targets_reference(walks, paths["unitig"], strings, mo["overlap"])
    po = paths["path_off"].astype(np.int64)
    src = {f: [] for f in ("pos", "count", "item")}
    sstep, spos, soff = [], [], [0]
    for R in range(len(po) - 1):
        for S in range(po[R], po[R + 1]):
            c, o = int(paths["count"][S]), 0
            while o < c:
                k = int(rng.integers(1, c - o + 1)) if rng.random() < 0.5 else c - o
                src["pos"].append(int(paths["pos"][S]) + o)
                src["count"].append(k)
                src["item"].append(int(paths["item"][S]) + o)
                sstep.append(NO_STEP if rng.random() < drop else S)
                spos.append(max(int(paths["pos"][S]) + o + (int(rng.integers(-1, 2)) if rng.random() < 0.1 else 0), 0))
                o += k
        soff.append(len(sstep))
    src = {f: np.array(v, dtype=np.uint32) for f, v in src.items()}
    src["path_off"] = np.array(soff, dtype=np.uint64)
    return {"walks": walks, "paths": paths, "uni": uni, "mo": mo, "seq_len": nodes["seq_len"], "q_begin": q_begin_of(walks, 100000 * np.arange(len(po))),
            "tgt_off": toff, "bad": bad, "src": src, "src_step": np.array(sstep, dtype=np.uint64), "src_pos": np.array(spos, dtype=np.uint32),
            "km_off": km_off, "start": start, "tgt": tgt}


def test_segments_reference_random_decompositions_invariants():
    rng = np.random.default_rng(221)
    seen = np.zeros(5, dtype=np.int64)
    for it in range(6):
        c = walked_segments_case(rng, 200, list(rng.integers(0, 60, size=40)))
        for seg_len in (64, 512):
            ref = segments_reference(c, seg_len)
            nw = len(c["bad"])
            assert int(ref["seg_off"][-1]) == nw + ref["stats"][3] and (np.diff(ref["seg_off"].astype(np.int64)) >= 1).all(), it
            assert ref["stats"][0] + ref["stats"][1] == int(c["src"]["count"].sum()), it
            assert (ref["q_begin"] <= ref["q_end"]).all() and (ref["t_begin"] <= ref["t_end"]).all(), it
            for w, cuts in enumerate(ref["cuts"]):
                assert all(a[0] < b[0] and a[1] < b[1] for a, b in zip(cuts, cuts[1:])) or len(cuts) == 2, (it, w)
            if seg_len == 64:
                seen += ref["stats"]
    assert (seen > [2000, 300, 500, 100, 50]).all(), seen


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


_dev, _host, _ptr, _marked, _full = ts._dev, ts._host, ts._ptr, ta._marked, ta._full
U64, U32, U8 = np.uint64, np.uint32, np.uint8
IN_DT = dict(walk_off=U64, first_step=U64, n_steps=U32, qstart=U32, qend=U32, path_start=U64, path_end=U64, flags=U32, unitig=U32, pos=U32, count=U32,
             uni_off=U64, members=U32, circular=U8, member_off=U64, out_off=U64, overlap=U32, seq_len=U32, q_begin=U64, tgt_off=U64, bad=U8,
             src_path_off=U64, src_pos=U32, src_count=U32, src_item=U32, src_step=U64, src_pos_map=U32, km_off=U64, start=U32)


def flat(c):
    """the named host arrays of a case, as raw_segments takes and replaces them"""
    a = {f: c["walks"][f] for f in WALK_F}
    a.update({f: c["paths"][f] for f in ("unitig", "pos", "count")})
    a.update({f: c["uni"][f] for f in ("uni_off", "members", "circular")}, **{f: c["mo"][f] for f in ("member_off", "out_off", "overlap")})
    a.update(seq_len=c["seq_len"], q_begin=c["q_begin"], tgt_off=c["tgt_off"], bad=c["bad"], km_off=c["km_off"], start=c["start"])
    a.update({"src_" + f: c["src"][f] for f in ("path_off", "pos", "count", "item")})
    a.update(src_step=c.get("src_step"), src_pos_map=c.get("src_pos"))
    return a


def raw_segments(eng, c, seg_len=SEG_LEN, capacity=None, want=SEG_F, ctx=True, out=True, null=(), totals=True, **over):
    """s2k_walks_segments through ctypes, guards behind every output -> (status, n_segments, stats, host arrays with guards).  over: any
    array of flat(c) replaced, or n_reads, n_walks, n_all_steps, n_unitigs, n_nodes, n_src given"""
    import torch

    a = flat(c)
    n = {"n_reads": len(a["walk_off"]) - 1, "n_walks": len(a["first_step"]), "n_all_steps": len(a["unitig"]), "n_unitigs": len(a["circular"]),
         "n_nodes": len(a["members"]), "n_src": len(a["src_pos"])}
    n.update({k: over.pop(k) for k in list(over) if k in n})
    a.update(over)
    dv = {f: None if x is None else _dev(x, IN_DT[f]) for f, x in a.items()}
    P = lambda f: None if dv[f] is None or f in null else dv[f].data_ptr()  # noqa: E731
    wo, po, so, do = pkg.WalkOut(), pkg.ThreadOut(), pkg.ThreadOut(), pkg.DeviceOut()
    wo.capacity = n["n_walks"]
    for f in WALK_F:
        setattr(wo, f, P(f))
    po.unitig, po.pos, po.count = P("unitig"), P("pos"), P("count")
    so.path_off, so.pos, so.count, so.item = P("src_path_off"), P("src_pos"), P("src_count"), P("src_item")
    do.km_off, do.start = P("km_off"), P("start")
    cap = int(capacity if capacity is not None else 0)
    res = {f: _full(n["n_walks"] + 1 if f == "seg_off" else max(cap, 1), U64) for f in want}
    o = pkg.SegmentOut()
    o.capacity = cap
    for f, x in res.items():
        setattr(o, f, x.data_ptr())
    total, stats = ctypes.c_uint64(777), (ctypes.c_uint64 * 8)(*([777] * 8))
    V = lambda f: ctypes.c_void_p(P(f))  # noqa: E731
    torch.cuda.synchronize()
    s = eng.lib.s2k_walks_segments(eng.ctx if ctx else None, n["n_reads"], None if "walks" in null else ctypes.byref(wo), n["n_walks"],
                                   None if "paths" in null else ctypes.byref(po), n["n_all_steps"], V("uni_off"), V("members"), V("circular"), n["n_unitigs"],
                                   V("member_off"), V("out_off"), V("overlap"), V("seq_len"), n["n_nodes"], V("q_begin"), V("tgt_off"), V("bad"),
                                   None if "src" in null else ctypes.byref(so), n["n_src"], V("src_step"), V("src_pos_map"),
                                   None if "in" in null else ctypes.byref(do), seg_len, ctypes.byref(o) if out else None,
                                   ctypes.byref(total) if totals else None, stats if totals else None)
    return s, total.value, list(stats)[:5], {f: _host(x, U64) for f, x in res.items()}


def assert_segments(got, ref, nw, tag):
    n = int(ref["seg_off"][-1])
    for f in SEG_F:
        k = nw + 1 if f == "seg_off" else n
        assert got[f][:k].tobytes() == ref[f].tobytes(), (tag, f, got[f][:8], ref[f][:8])
        assert _marked(got[f], k), (tag, f, "guard")


def device_segments(eng, c, tag, seg_len=SEG_LEN):
    """the calls against the reference: sizes only (no out; seg_off alone), the writing call, capacity one short -> the reference"""
    ref = segments_reference(c, seg_len)
    nw, n = len(c["bad"]), int(ref["seg_off"][-1])
    s, total, stats, got = raw_segments(eng, c, seg_len, out=False, want=())
    assert (s, total, stats) == (0, n, ref["stats"]), (tag, "sizes", s, total, n, stats, ref["stats"])
    s, total, stats, got = raw_segments(eng, c, seg_len, want=("seg_off",))
    assert (s, total, stats) == (0, n, ref["stats"]) and got["seg_off"][:nw + 1].tobytes() == ref["seg_off"].tobytes() and _marked(got["seg_off"], nw + 1), (tag, "seg_off")
    s, total, stats, got = raw_segments(eng, c, seg_len, capacity=n)
    assert (s, total, stats) == (0, n, ref["stats"]), (tag, s, total, n, stats, ref["stats"])
    assert_segments(got, ref, nw, tag)
    if n:
        s, total, stats, got = raw_segments(eng, c, seg_len, capacity=n - 1)
        assert (s, total) == (7, n) and all(_marked(x) for x in got.values()), (tag, "capacity")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_device_segments_hand_cases(eng, name):
    walks, kw, want, stats = HAND[name]
    ref = device_segments(eng, anchor_case(walks, **kw), name)
    assert ref["stats"] == stats
    for w in range(len(walks)):  # every walk alone
        if not (kw.get("shift") or kw.get("no_step")):
            device_segments(eng, anchor_case(walks[w:w + 1]), (name, w))


@pytest.mark.gpu
@pytest.mark.parametrize("n_walks", [1, 63, 64, 65, 4097])
def test_device_segments_walk_counts(eng, n_walks):
    rng = np.random.default_rng(230 + n_walks)
    ref = device_segments(eng, many_walks(rng, n_walks, per_read=1 + n_walks % 3), n_walks)
    assert n_walks < 63 or (ref["stats"][3] > n_walks // 4 and ref["stats"][1] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_items", [255, 256, 257, 4095, 4096, 4097])
def test_device_segments_items_round_a_block_and_a_tile(eng, n_items):
    """one read of n_items source items, all admissible: the item tiles, and at seg_len 64 the compacted stream's, are cut round 256 and
    round two tiles of 2 048"""
    c = many_anchors(n_items)
    for seg_len in (64, 512):
        ref = device_segments(eng, c, (n_items, seg_len), seg_len)
        assert ref["stats"][:3] == [n_items, 0, n_items] and ref["stats"][3] == (20 * n_items) // seg_len
    if n_items in (257, 4097):  # and the same with the read's last two items outside their step
        c["src"]["count"][0] += 2
        c["km_off"][-1] += 2
        c["start"] = np.concatenate([c["start"], c["start"][-2:] + 40]).astype(np.uint32)
        assert device_segments(eng, c, (n_items, "two more"), 64)["stats"][:2] == [n_items, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("seg_len", [64, 512])
def test_device_segments_anchors_round_a_bucket(eng, seg_len):
    s = seg_len
    c = anchor_case([_w([(s - 1, 10), (s, 20), (s + 1, 30), (2 * s, 40)]), _w([(s - 1, 10), (s + 1, 30), (2 * s - 1, 35)]), _w([(s - 1, 10)]),
                     _w([(2 * s, 40), (2 * s + 1, 41), (3 * s - 1, 50), (3 * s, 60)])])
    ref = device_segments(eng, c, ("bucket", s), s)
    assert [x[1:-1] for x in ref["cuts"]] == [[(s, 20), (2 * s, 40)], [(s + 1, 30)], [], [(2 * s, 40), (3 * s, 60)]]


@pytest.mark.gpu
def test_device_segments_identity_against_a_bridge_made_map(eng, oracle, repeat_case, noisy_case, repeat_walks):
    """the noisy repeat reads: walks made on the threaded paths themselves (identity), and walks made on the bridged paths with the map
    bridge gives; on the bridged walks the anchors of a merged run all fall into one walk"""
    R, n, k = tsp.REPEAT, noisy_case, repeat_walks["before"]
    b = tus._oracle_batch(oracle, n["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = dict(k, strings=k["strings"], overlap=k["overlap"])
    src = {f: n["paths"][f] for f in tb.STEP + ("path_off",)}
    plain = bridged_case(graph, b, src, dict(src, join=np.zeros(len(src["unitig"]), dtype=np.uint8)))
    assert plain["src_step"].tolist() == list(range(len(src["unitig"])))
    a = device_segments(eng, dict(plain, src_step=None), "identity", 64)
    assert device_segments(eng, plain, "identity, spelled out", 64)["stats"] == a["stats"]
    br = tb.reference_of(n)
    bridged = bridged_case(graph, b, src, br)
    c = device_segments(eng, bridged, "bridged", 64)
    assert br["n_merged"] > 0 and c["stats"][0] == a["stats"][0] == int(src["count"].sum()) and c["stats"][1] == a["stats"][1] == 0
    assert len(bridged["bad"]) < len(plain["bad"]) and c["stats"][3] > 0
    print("noisy repeat reads, seg_len 64: identity %s, bridged %s" % (a["stats"], c["stats"]))


@pytest.mark.gpu
def test_device_segments_one_walk_of_2000_steps(eng):
    """twk.long_chain_case with its junctions made sound (as test_align.py does): two walks of 2 000 one-member steps, the second on the
    twin strands; every step is a source step of one item, so G_w runs over all steps"""
    T = 2000
    case = twk.long_chain_case(T)
    rng = np.random.default_rng(T)
    strings = ta.random_strings(rng, case["mo"])
    ln = np.array([len(s) for s in strings], dtype=np.int64)
    ov = case["mo"]["overlap"].astype(np.int64).copy()
    ov[0:-2:2] = np.minimum(ov[0:-2:2], np.minimum(ln[:-1], ln[1:]))
    ov[3::2] = np.minimum(ov[3::2], np.minimum(ln[1:], ln[:-1]))
    case["mo"] = dict(case["mo"], overlap=ov.astype(np.uint32))
    walks = twk.reference_of(case)
    paths = case["paths"]
    toff, tgt, bad = ta.targets_reference(walks, paths["unitig"], strings, case["mo"]["overlap"])
    assert walks["n_steps"].tolist() == [T, T] and bad.tolist() == [0, 0]
    src = {"path_off": paths["path_off"], "pos": paths["pos"], "count": paths["count"], "item": np.concatenate([np.arange(T), np.arange(T)]).astype(np.uint32)}
    c = {"walks": walks, "paths": paths, "uni": case["uni"], "mo": case["mo"], "seq_len": case["nodes"]["seq_len"], "q_begin": np.array([3, 50000], dtype=np.uint64),
         "tgt_off": toff, "bad": bad, "src": src, "src_step": None, "src_pos": None, "km_off": np.array([0, T, 2 * T], dtype=np.uint64), "start": paths["start"]}
    ref = device_segments(eng, c, "long chain", 64)
    assert ref["stats"][0] == 2 * T and ref["stats"][3] > 200 and ref["stats"][4] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("seg_len", [64, 512])
def test_device_segments_random_decompositions(eng, seg_len):
    rng = np.random.default_rng(79)
    c = walked_segments_case(rng, 300, list(rng.integers(0, 60, size=80)))
    ref = device_segments(eng, c, ("walked", seg_len), seg_len)
    assert c["walks"]["flags"].any() and c["bad"].any() and min(ref["stats"][:3]) > 100 and (seg_len == 512 or ref["stats"][3] > 20)
    print("random decomposition, seg_len %d: %d walks, %d segments, %s" % (seg_len, len(c["bad"]), int(ref["seg_off"][-1]), ref["stats"]))


def _changed(src, i, v):
    x = np.array(src).copy()
    x[i] = v
    return x


@pytest.mark.gpu
def test_device_segments_refusals_nothing_written(eng):
    c = anchor_case([_w([(600, 600), (1200, 1200)]), _w([(600, 600)]), _w([(700, 700), (1300, 1300)]), _w([(600, 600)])], per_read=2)
    a = flat(c)
    n = int(device_segments(eng, c, "base")["seg_off"][-1])

    def refused(code=1, **kw):
        s, total, stats, got = raw_segments(eng, c, capacity=n, **kw)
        assert (s, total, stats) == (code, 0, [0] * 5) and all(_marked(x) for x in got.values()), (s, total, stats, list(kw))

    refused(ctx=False)
    for f in ("walks", "src", "in", "walk_off", "first_step", "n_steps", "qstart", "qend", "path_start", "path_end", "flags", "unitig", "pos", "count",
              "uni_off", "members", "circular", "member_off", "out_off", "overlap", "seq_len", "q_begin", "tgt_off", "bad", "src_path_off", "src_pos",
              "src_count", "src_item", "km_off", "start"):
        refused(null=(f,))
    refused(seg_len=63)
    refused(seg_len=1)
    refused(n_walks=2 ** 31)
    refused(n_unitigs=2 ** 31)
    # the checks of s2k_walks_targets
    refused(first_step=_changed(a["first_step"], 3, 5))  # a step index outside the paths
    refused(n_steps=_changed(a["n_steps"], 3, 2))
    refused(unitig=_changed(a["unitig"], 1, 2))  # a unitig >= 2 n_unitigs
    refused(out_off=_changed(a["out_off"], 0, int(a["out_off"][1]) + 1))  # out_off decreases
    refused(out_off=_changed(a["out_off"], 1, 2 ** 32))  # a unitig of 2^32 bases
    # the checks of s2k_paths_walks
    refused(count=_changed(a["count"], 2, 0))
    refused(pos=_changed(a["pos"], 2, len(a["members"])))
    refused(count=_changed(a["count"], 3, len(a["members"])))  # the step passes its unitig's end
    refused(uni_off=_changed(a["uni_off"], 0, 1))
    refused(uni_off=_changed(a["uni_off"], 1, len(a["members"]) - 1))  # uni_off does not end at n_nodes
    refused(members=_changed(a["members"], 4, 2 * len(a["members"])))
    refused(member_off=_changed(a["member_off"], 3, int(a["out_off"][1]) + 1))  # a member offset outside its unitig's bases
    # the offsets of the walks and of the source
    refused(walk_off=_changed(a["walk_off"], 0, 1))
    refused(walk_off=_changed(a["walk_off"], 1, 5))  # decreases behind it
    refused(walk_off=_changed(a["walk_off"], 2, 3))  # does not end at n_walks
    refused(src_path_off=_changed(a["src_path_off"], 0, 1))
    refused(src_path_off=_changed(a["src_path_off"], 2, 5))
    refused(first_step=_changed(a["first_step"], 1, 0))  # two walks hold step 0
    refused(first_step=_changed(a["first_step"], 2, 1))
    refused(qstart=_changed(a["qstart"], 1, int(a["qend"][1]) + 1))
    refused(tgt_off=_changed(a["tgt_off"], 2, int(a["tgt_off"][1]) - 1))
    refused(tgt_off=_changed(_changed(a["tgt_off"], 3, 2 ** 33), 4, 2 ** 33 + 3000))  # a target of 2^32 bytes
    refused(km_off=_changed(a["km_off"], 1, int(a["km_off"][2]) + 1))
    # the items and the map
    refused(src_count=_changed(a["src_count"], 1, 2))  # the read's items end before the step's do
    refused(src_item=_changed(a["src_item"], 3, 3))
    ident = np.arange(4, dtype=np.uint64)
    assert raw_segments(eng, c, capacity=n, src_step=ident)[:2] == (0, n)
    refused(src_step=_changed(ident, 1, 4))  # neither below n_steps nor NO_STEP
    refused(src_step=_changed(ident, 1, 2 ** 63))
    refused(src_step=_changed(ident, 1, 2))  # a step of the other read's walk
    refused(src_step=_changed(ident, 3, 1))
    refused(src_step=np.array([1, 0, 2, 3], dtype=np.uint64))  # decreases inside a read
    three = dict(c, src=dict(path_off=np.array([0, 3, 5], dtype=np.uint64), pos=a["src_pos"][[0, 0, 1, 2, 3]], count=np.array([1, 1, 1, 2, 1], dtype=np.uint32),
                             item=np.array([0, 1, 2, 0, 2], dtype=np.uint32)))
    s, total, stats, got = raw_segments(eng, three, capacity=n, src_step=np.array([0, NO_STEP, 1, 2, 3], dtype=np.uint64))
    assert (s, stats[:2]) == (0, [5, 1])  # (the second source step has no step: its item lies outside)
    s, total, stats, got = raw_segments(eng, three, capacity=n, src_step=np.array([1, NO_STEP, 0, 2, 3], dtype=np.uint64),
                                        src_pos_map=np.array([2, 0, 0, 3, 5], dtype=np.uint32))
    assert (s, total, stats) == (1, 0, [0] * 5) and all(_marked(x) for x in got.values())  # a candidate of walk 0 behind one of walk 1, across the gap
    z = ctypes.c_uint64(5)
    assert eng.lib.s2k_walks_segments(eng.ctx, 0, None, 0, None, 0, None, None, None, 0, None, None, None, None, 0, None, None, None, None, 0, None, None, None, 0,
                                      None, ctypes.byref(z), None) == 1 and z.value == 0
    assert raw_segments(eng, c, capacity=n, totals=False)[0] == 1


@pytest.mark.gpu
def test_device_segments_null_outputs_and_empty_inputs(eng):
    c = anchor_case([_w([(600, 600), (1200, 1200)]), _w([]), _w([(700, 700)])])
    ref = segments_reference(c)
    n = int(ref["seg_off"][-1])
    for want in (("q_begin",), ("t_end", "seg_off"), ("q_end", "t_begin")):  # any subset of the outputs
        s, total, stats, got = raw_segments(eng, c, capacity=n, want=want)
        assert (s, total, stats) == (0, n, ref["stats"]), want
        for f in want:
            k = len(ref[f])
            assert got[f][:k].tobytes() == ref[f].tobytes() and _marked(got[f], k), f
    none = anchor_case([_w([(600, 600)])])
    empty = dict(none, walks={f: (none["walks"][f][:1] if f == "walk_off" else none["walks"][f][:0]) for f in WALK_F}, q_begin=none["q_begin"][:0],
                 tgt_off=none["tgt_off"][:1], bad=none["bad"][:0], paths={f: none["paths"][f][:0] for f in ("unitig", "pos", "count")},
                 src={f: (none["src"][f][:1] if f == "path_off" else none["src"][f][:0]) for f in none["src"]}, km_off=none["km_off"][:1], start=none["start"][:0])
    s, total, stats, got = raw_segments(eng, empty, capacity=4, n_reads=0)
    assert (s, total, stats, int(got["seg_off"][0])) == (0, 0, [0] * 5, 0) and _marked(got["seg_off"], 1) and _marked(got["q_begin"])
    s, total, stats, got = raw_segments(eng, dict(none, src=dict(none["src"], path_off=np.zeros(2, dtype=np.uint64)), src_step=None), capacity=4, n_src=0)
    assert (s, total, stats, got["seg_off"][:2].tolist()) == (0, 1, [0] * 5, [0, 1])  # walks without a source item: one segment each


@pytest.mark.gpu
def test_device_segments_deterministic(eng):
    rng = np.random.default_rng(81)
    c = walked_segments_case(rng, 300, list(rng.integers(0, 60, size=80)))
    n = int(segments_reference(c, 64)["seg_off"][-1])
    runs = [raw_segments(eng, c, 64, capacity=n) for _ in range(2)]
    assert runs[0][:3] == runs[1][:3] and all(runs[0][3][f].tobytes() == runs[1][3][f].tobytes() for f in SEG_F)


# ---- the join on the device --------------------------------------------------------------------------------------------------------------
A32 = ("edits", "flags", "n_ops", "matches", "ops")
A_DT = dict({f: U32 for f in A32}, ops_off=U64)


def flat_segments(seg, junk=0x00C0FFEE):
    """the arrays s2k_align_pairs would have written: the runs at ops_off, the slots behind them left as they were (junk)"""
    ops = np.full(int(seg["ops_off"][-1]), junk, dtype=np.uint32)
    for i, o in enumerate(seg["ops"]):
        ops[int(seg["ops_off"][i]): int(seg["ops_off"][i]) + len(o)] = o
    return dict({f: np.asarray(seg[f]) for f in ("edits", "flags", "n_ops", "matches", "ops_off")}, ops=ops)


def raw_join(eng, seg_off, bad, seg, capacity=None, want=A32 + ("ops_off",), ctx=True, out=True, null=(), total=True, **over):
    """s2k_align_join through ctypes, guards behind every output -> (status, n_ops_total, host arrays with guards).  over: seg_off, bad
    or an array of the segments replaced; n_walks, n_segments, n_runs given"""
    import torch

    a = dict(flat_segments(seg), seg_off=np.asarray(seg_off), bad=np.asarray(bad))
    n = {"n_walks": len(a["bad"]), "n_segments": len(a["edits"]), "n_runs": len(a["ops"])}
    n.update({k: over.pop(k) for k in list(over) if k in n})
    a.update(over)
    dt = dict(A_DT, seg_off=U64, bad=U8)
    dv = {f: _dev(x, dt[f]) for f, x in a.items()}
    si = pkg.AlignOut()
    si.capacity = n["n_runs"]
    for f in A32 + ("ops_off",):
        setattr(si, f, None if f in null else dv[f].data_ptr())
    cap = int(capacity if capacity is not None else 0)
    nw = len(a["bad"])
    res = {f: _full(nw + 1 if f == "ops_off" else max(cap, 1) if f == "ops" else max(nw, 1), A_DT[f]) for f in want}
    o = pkg.AlignOut()
    o.capacity = cap
    for f, x in res.items():
        setattr(o, f, x.data_ptr())
    nb = ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_align_join(eng.ctx if ctx else None, n["n_walks"], _ptr(dv["seg_off"], "seg_off" in null), _ptr(dv["bad"], "bad" in null), n["n_segments"],
                               None if "seg" in null else ctypes.byref(si), ctypes.byref(o) if out else None, ctypes.byref(nb) if total else None)
    return s, nb.value, {f: _host(x, A_DT[f]) for f, x in res.items()}


def assert_joined(got, ref, nw, tag):
    for f in ("edits", "flags", "n_ops", "matches"):
        assert got[f][:nw].tobytes() == ref[f].tobytes(), (tag, f, got[f][:8], ref[f][:8])
        assert nw == 0 or _marked(got[f], nw), (tag, f, "guard")
    assert got["ops_off"][:nw + 1].tobytes() == ref["ops_off"].tobytes() and _marked(got["ops_off"], nw + 1), (tag, "ops_off")
    ops = np.concatenate([np.zeros(0, dtype=np.uint32)] + list(ref["ops"]))
    assert got["ops"][:len(ops)].tobytes() == ops.tobytes() and _marked(got["ops"], len(ops)), (tag, "ops")


def device_join(eng, seg_off, bad, seg, tag):
    ref = join_reference(seg_off, bad, seg)
    nw, n = len(bad), int(ref["ops_off"][-1])
    s, nb, got = raw_join(eng, seg_off, bad, seg, out=False, want=())
    assert (s, nb) == (0, n), (tag, "sizes", s, nb, n)
    s, nb, got = raw_join(eng, seg_off, bad, seg, capacity=n)
    assert (s, nb) == (0, n), (tag, s, nb, n)
    assert_joined(got, ref, nw, tag)
    if n:
        s, nb, got = raw_join(eng, seg_off, bad, seg, capacity=n - 1)
        assert (s, nb) == (7, n) and all(_marked(x) for x in got.values()), (tag, "capacity")
        s, nb, got = raw_join(eng, seg_off, bad, seg, capacity=0, want=("edits", "flags", "ops_off", "n_ops", "matches"))  # without ops: no capacity asked
        assert (s, nb) == (0, n) and got["ops_off"][:nw + 1].tobytes() == ref["ops_off"].tobytes(), (tag, "no ops")
    return ref


@pytest.mark.gpu
def test_device_join_hand_cases(eng):
    for name, (cig, over, seg_off, bad, want, edits) in JOIN_HAND.items():
        ref = device_join(eng, seg_off, bad, _seg(*cig, over=over), name)
        assert [ta.cigar_of(r[2]) if r[1] == 0 else r[1] for r in ref["res"]] == want, name
    every = [(c, o) for c, o, *_ in JOIN_HAND.values()]  # and all of them as the walks of one call
    cig = [x for c, _ in every for x in c]
    over = [sum(len(c) for c, _ in every[:i]) + j for i, (_, o) in enumerate(every) for j in o]
    bad = []
    off = 0
    seg_off = [0]
    for name, (c, o, so, b, want, edits) in JOIN_HAND.items():
        seg_off += [off + x for x in so[1:]]
        bad += b
        off += len(c)
    device_join(eng, seg_off, bad, _seg(*cig, over=over), "all hand cases")


def random_segments(rng, n_walks, max_segs=4, p_over=0.05, p_bad=0.05, p_eq=0.3):
    """walks of 0 .. max_segs segments with random CIGARs: all-= segments (chains collapse), runs that meet equal ops at a border, over
    segments and bad walks mixed in"""
    cig, over, seg_off, bad = [], [], [0], []
    for _ in range(n_walks):
        for _ in range(int(rng.integers(0, max_segs + 1))):
            if rng.random() < p_over:
                over.append(len(cig))
                cig.append("")
            elif rng.random() < p_eq:
                cig.append("%d=" % rng.integers(1, 600))
            else:
                runs, last = [], None
                for _ in range(int(rng.integers(1, 8))):
                    op = str(rng.choice([c for c in "=XID" if c != last]))
                    runs.append("%d%s" % (rng.integers(1, 40), op))
                    last = op
                cig.append("".join(runs))
        seg_off.append(len(cig))
        bad.append(int(rng.random() < p_bad))
    return seg_off, bad, _seg(*cig, over=over)


@pytest.mark.gpu
@pytest.mark.parametrize("n_walks", [1, 63, 64, 65, 1500])
def test_device_join_walk_counts_with_over_and_bad_walks(eng, n_walks):
    rng = np.random.default_rng(240 + n_walks)
    seg_off, bad, seg = random_segments(rng, n_walks)
    ref = device_join(eng, seg_off, bad, seg, n_walks)
    assert n_walks < 1500 or ((ref["flags"] == OVER).any() and (ref["flags"] == BAD_PATH).any() and (ref["flags"] == 0).sum() > n_walks // 2)


@pytest.mark.gpu
def test_device_join_walks_of_1_2_and_300_segments(eng):
    rng = np.random.default_rng(250)
    for k in (1, 2, 300):
        cig = ["%d=%dX" % (rng.integers(1, 50), rng.integers(1, 3)) if i % 5 else "%d=" % rng.integers(1, 50) for i in range(k)]
        ref = device_join(eng, [0, k], [0], _seg(*cig), ("segments", k))
        assert int(ref["flags"][0]) == 0 and int(ref["n_ops"][0]) < sum(c.count("=") + c.count("X") for c in cig) + (k == 1)
    seg_off, bad, seg = random_segments(rng, 3, max_segs=0)
    device_join(eng, [0, 0, 300, 300], [0, 0, 1], _seg(*["7=1X"] * 300), "a walk without a segment on both sides")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [64, 65])
def test_device_join_collapse_chain(eng, k):
    """k all-= segments are one run; with an X segment before and an I segment behind, and the chain again in the next walk"""
    chain = ["%d=" % (i + 1) for i in range(k)]
    ref = device_join(eng, [0, k + 2, 2 * k + 2], [0, 0], _seg(*(["3=1X"] + chain + ["2I5="] + chain)), ("chain", k))
    total = k * (k + 1) // 2
    assert [ta.cigar_of(r[2]) for r in ref["res"]] == ["3=1X%d=2I5=" % total, "%d=" % total]


@pytest.mark.gpu
@pytest.mark.parametrize("n_slots", [255, 256, 257, 2047, 2048, 2049])
def test_device_join_run_slots_round_a_block_and_a_tile(eng, n_slots):
    """segments of one X between two = (three runs in three slots: 2 edits + 1), one 1= segment in a slot of its own when the number is
    not a multiple of three: the slots' tiles end round 256 and 2 048, and every border merges"""
    k, rest = divmod(n_slots, 3)
    cig = ["4=1X4="] * k + ["1="] * rest
    seg = _seg(*cig)
    assert int(seg["ops_off"][-1]) == n_slots
    half = len(cig) // 2
    ref = device_join(eng, [0, half, len(cig)], [0, 0], seg, ("slots", n_slots))
    assert ref["n_ops"].tolist() == [2 * half + 1, 2 * (k - half) + 1]


@pytest.mark.gpu
def test_device_join_refusals_nothing_written(eng):
    seg_off, bad, seg = [0, 2, 3], [0, 0], _seg("5=1X", "1X4=", "7=")
    n = int(device_join(eng, seg_off, bad, seg, "base")["ops_off"][-1])
    f = flat_segments(seg)

    def refused(code=1, **kw):
        s, nb, got = raw_join(eng, kw.pop("seg_off", seg_off), bad, seg, capacity=n, **kw)
        assert (s, nb) == (code, 0) and all(_marked(x) for x in got.values()), (s, nb, list(kw))

    refused(ctx=False)
    for x in ("seg_off", "bad", "seg", "edits", "flags", "n_ops", "matches", "ops", "ops_off"):
        refused(null=(x,))
    refused(n_walks=2 ** 32)
    refused(n_segments=2 ** 32)
    refused(seg_off=np.array([1, 2, 3]))
    refused(seg_off=np.array([0, 4, 3]))
    refused(seg_off=np.array([0, 2, 2]))  # does not end at n_segments
    refused(ops_off=_changed(f["ops_off"], 1, int(f["ops_off"][2]) + 1))
    refused(n_runs=int(f["ops_off"][-1]) - 1)  # ops_off passes the runs there are
    refused(n_ops=_changed(f["n_ops"], 0, 4))  # above the segment's slots
    refused(ops=_changed(f["ops"], 0, 7))  # a run of length 0
    refused(ops=_changed(f["ops"], int(f["ops_off"][1]), 5 << 4 | 3))  # an unknown code
    assert raw_join(eng, seg_off, [0, 1], seg, capacity=n, ops=_changed(f["ops"], int(f["ops_off"][2]), 3))[0] == 0  # (a bad walk's runs are not read)
    big = _seg("%d=" % (2 ** 27), "%d=" % (2 ** 27), "7=")
    assert raw_join(eng, [0, 1, 3], bad, big, capacity=3)[:2] == (0, 2)  # (2^27 + 7 bases: one run)
    s, nb, got = raw_join(eng, seg_off, bad, big, capacity=3)
    assert (s, nb) == (1, 0) and all(_marked(x) for x in got.values())  # the two merge into a run of 2^28 bases
    assert raw_join(eng, seg_off, bad, seg, capacity=n, total=False)[0] == 1


@pytest.mark.gpu
def test_device_join_deterministic(eng):
    seg_off, bad, seg = random_segments(np.random.default_rng(260), 700)
    n = int(join_reference(seg_off, bad, seg)["ops_off"][-1])
    runs = [raw_join(eng, seg_off, bad, seg, capacity=n) for _ in range(2)]
    assert runs[0][:2] == runs[1][:2] and all(runs[0][2][f].tobytes() == runs[1][2][f].tobytes() for f in runs[0][2])


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _assert_walk_alignments(al, ref, tag):
    got = al.host()
    for f in ("edits", "flags", "n_ops", "matches", "ops_off"):
        assert got[f].tobytes() == ref[f].tobytes(), (tag, f)
    assert got["ops"][:int(ref["ops_off"][-1])].tobytes() == np.concatenate([np.zeros(0, dtype=np.uint32)] + list(ref["ops"])).tobytes(), (tag, "ops")
    assert (al.n_over, al.n_bad) == (int((ref["flags"] & OVER != 0).sum()), int((ref["flags"] & BAD_PATH != 0).sum())), tag


@pytest.mark.gpu
def test_ecoli_long_reads_end_to_end(eng, ecoli_long, tmp_path):
    """the long reads through the device's own graph of the 600 reads: thread -> bridge(origin=True) -> walks -> align_segmented equals the
    references field by field, no walk is over; align on the same walks flags what the reference flagged; the pile-up and the GAF
    writer take the joined alignments as they are"""
    e, (mode, l, k) = ecoli_long, tsp.MODES[0]
    outs600 = twk._extract_all(eng, e["reads600"], l, k, 0.05, mode)
    graph = pkg.KminmerGraph.build(eng, [outs600], min_count=2, min_edge_count=1)
    ns = pkg.NodeSequences.build(eng, graph, [outs600])
    sg, node_map, _ = graph.simplify(eng, 10, 20)
    ug = sg.unitigs(eng)
    table = pkg.CountTable(eng, sg.keys, sg.counts)
    outs = twk._extract_all(eng, e["reads"], l, k, 0.05, mode)
    src = ug.thread(eng, table, outs, len(e["reads"]), min_count=2)
    table.close()
    paths, _ = ug.bridge(eng, src, *LONG["limits"], origin=True)
    assert paths.origin.paths is src and paths.origin.src_step.cpu().numpy().view(np.uint64).tobytes() == e["case"]["src_step"].tobytes()
    sns = ns.subset(node_map)
    walks = ug.walks(eng, paths, sns)
    seqs = ug.sequences(eng, sns)
    W = e["case"]["walks"]
    assert all(walks.host()[f].tobytes() == W[f].tobytes() for f in ("first_step", "qstart", "qend", "path_start", "path_end"))
    al = ug.align_segmented(eng, walks, outs["bases"], outs["read_off"], seqs, sns, outs)
    ref = e["seg"]
    _assert_walk_alignments(al, ref, "segmented")
    assert al.n_over == 0 and al.segments == dict(zip(STATS, ref["sg"]["stats"]), n_segments=len(ref["seg"]["edits"]), n_over_segments=0)
    whole = ug.align(eng, walks, outs["bases"], outs["read_off"], seqs)
    assert whole.n_over == int((e["whole"]["flags"] & OVER != 0).sum()) >= 16 and whole.host()["flags"].tobytes() == e["whole"]["flags"].tobytes()
    pile = ug.pileup(eng, seqs)
    st = pile.add(eng, walks, al, outs["bases"], outs["read_off"])  # (a CIGAR that does not consume its target is refused: it raises)
    n0 = int((ref["flags"] == 0).sum())
    assert (st["walks_used"], st["walks_skipped"]) == (n0, walks.n_walks - n0) and int(pile.depth().max()) >= 3
    p = str(tmp_path / "long.gaf")
    walks.write_gaf(p, ug, alignments=al)
    lines = [line.split("\t") for line in open(p).read().split("\n") if line]
    block = pkg.alignment_block_len(ref["ops_off"], ref["n_ops"], np.concatenate(list(ref["ops"])))
    assert len(lines) == walks.n_walks
    for i, f in enumerate(lines):
        assert f[-2:] == ["NM:i:%d" % ref["edits"][i], "cg:Z:" + ta.cigar_of(ref["res"][i][2])] and int(f[10]) == int(block[i]) == int(al.block_len[i]), i
    print("E. coli long reads on the device: %d walks, %d segments, %d edits in all; whole-walk align flags %d over" % (
        walks.n_walks, al.segments["n_segments"], int(al.host()["edits"].sum()), whole.n_over))


@pytest.mark.gpu
def test_repeat_fixture_short_walks_align_as_align_does(eng, repeat_case, noisy_case):
    """the noisy repeat reads on the unitig graph: a walk of fewer than seg_len bases is not cut, and its alignment is align's"""
    c, R, n = repeat_case, tsp.REPEAT, noisy_case
    clean = twk._extract_all(eng, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [clean], min_count=R["min_count"], min_edge_count=1)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, [clean])
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    noisy = twk._extract_all(eng, n["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    src = ug.thread(eng, table, noisy, len(n["reads"]), min_count=R["min_count"])
    table.close()
    seqs = ug.sequences(eng, ns)
    for tag, paths in (("plain", src), ("bridged", ug.bridge(eng, src, origin=True)[0])):
        walks = ug.walks(eng, paths, ns)
        h = walks.host()
        qlen = h["qend"].astype(np.int64) - h["qstart"]
        a = ug.align(eng, walks, noisy["bases"], noisy["read_off"], seqs).host()
        assert a["edits"].sum() > 50
        for seg_len in (512, int(qlen.max()) + 1):
            s = ug.align_segmented(eng, walks, noisy["bases"], noisy["read_off"], seqs, ns, noisy, seg_len=seg_len)
            g = s.host()
            short = np.nonzero(qlen < seg_len)[0]
            assert len(short) > 0 and (seg_len == 512 or (len(short) == walks.n_walks and s.segments["chosen"] == 0)), (tag, seg_len)
            for w in short:
                assert all(g[f][w] == a[f][w] for f in ("edits", "matches", "n_ops", "flags")), (tag, seg_len, w)
                assert s.cigar(w) == pkg.cigar_string(a["ops"][int(a["ops_off"][w]): int(a["ops_off"][w]) + int(a["n_ops"][w])]), (tag, seg_len, w)
