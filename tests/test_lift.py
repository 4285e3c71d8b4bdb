"""Read paths lifted onto the untangled contigs: s2k_unitig_copy_places and s2k_paths_lift (include/s2k.h).  The
references are `copy_places_reference` and `lift_reference`, serial restatements of the header's definitions (plain loops over
contigs, reads and steps; `find` is a scan of one row); the device's arrays equal theirs exactly, every one of them, in every test.
The invariant test checks the mapped positions against `expand_reference` of test_untangle.py, which knows nothing of either."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import test_bridge as tb
import test_graph as tg
import test_simplify as ts
import test_span as tsp
import test_unitig_sequences as tus
import test_untangle as tun
import test_walk as twk
from test_bridge import noisy_case  # noqa: F401  (module-scoped fixtures of the repeat)
from test_span import repeat_case  # noqa: F401
from test_walk import repeat_walks  # noqa: F401

pkg = import_package()

SYMS = ("s2k_unitig_copy_places", "s2k_paths_lift")
LINKED = 1
NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
STEP = tb.STEP
OUT32 = STEP + ("matched",)
TOTALS = ("n_steps", "n_merged", "n_dropped", "n_conflicts")


# ---- the references ----------------------------------------------------------------------------------------------------------------
def copy_places_reference(outer, origin, inner):
    """outer: dict with uni_off, members, circular over the copies; inner: dict with uni_off, circular -> the pkg.NodePlace record of
    every copy"""
    oo, om = [int(x) for x in outer["uni_off"]], [int(x) for x in outer["members"]]
    io = [int(x) for x in inner["uni_off"]]
    ln = lambda c: io[int(origin[c]) + 1] - io[int(origin[c])]  # noqa: E731
    place = np.zeros(len(origin), dtype=pkg.NodePlace)
    for t in range(len(oo) - 1):
        piece = om[oo[t]: oo[t + 1]]
        Lc = sum(ln(C >> 1) for C in piece)
        circ = int(bool(outer["circular"][t]) or (len(piece) == 1 and bool(inner["circular"][int(origin[piece[0] >> 1])])))
        f = 0
        for C in piece:
            c, s, m = C >> 1, C & 1, ln(C >> 1)
            place[c] = (2 * t + s, Lc - f - m if s else f, Lc, circ)
            f += m
    return place


def lift_reference(case):
    """case: dict with paths (path_off and the seven step arrays), matched_in (or None), ro, d, uni_off, resolved, partner, copy_off,
    place, n_contigs -> dict: path_off uint64, the step arrays and matched uint32 (one entry per output step), step_copy uint32, join
    uint8, V and Q uint32 (one entry per input step; NONE for a dropped one), contig_items uint64, and the four totals"""
    paths = case["paths"]
    ro, d, off = [int(x) for x in case["ro"]], [int(x) for x in case["d"]], [int(x) for x in case["uni_off"]]
    res, par, coff = [int(x) for x in case["resolved"]], [int(x) for x in case["partner"]], [int(x) for x in case["copy_off"]]
    place = case["place"]
    po = [int(x) for x in paths["path_off"]]
    u, p, c, it, fl, st, en = ([int(x) for x in paths[f]] for f in STEP)
    mi = c if case.get("matched_in") is None else [int(x) for x in case["matched_in"]]
    ln = lambda U: off[(U >> 1) + 1] - off[U >> 1]  # noqa: E731
    n = len(u)
    find = lambda A, B: tsp._find(ro, d, A, B)  # noqa: E731
    tw = lambda A, B: find(B ^ 1, A ^ 1)  # noqa: E731  (of the edge A -> B)
    follow = [None] * n
    for r in range(len(po) - 1):
        for s in range(po[r] + 1, po[r + 1]):
            if fl[s] & LINKED and p[s] == 0 and p[s - 1] + c[s - 1] == ln(u[s - 1]):
                follow[s] = find(u[s - 1], u[s])
    last = set(x - 1 for x in po[1:])  # the last step of a read
    copy, V, Q, clen, ccirc = [NONE] * n, [NONE] * n, [NONE] * n, [1] * n, [0] * n
    dropped = conflicts = 0
    for s in range(n):
        U = u[s]
        t, base = U >> 1, ro[2 * (U >> 1) + 1]
        j = 0
        if res[t]:
            e_in = follow[s]
            e_out = follow[s + 1] if s not in last and s + 1 < n else None
            j_in = j_out = None
            if e_in is not None:
                x = par[e_in] if U & 1 else tw(u[s - 1], U)
                j_in = ((NONE if x is None else x) - base) & M64
            if e_out is not None:
                if U & 1:
                    x = e_out
                else:
                    w = tw(U, u[s + 1])
                    x = NONE if w is None else par[w]
                j_out = (x - base) & M64
            if j_in is None and j_out is None:
                dropped += 1
                continue
            if j_in is not None and j_out is not None and j_in != j_out:
                conflicts += 1
            j = j_in if j_in is not None else j_out
            if j >= coff[t + 1] - coff[t]:
                j = 0
        copy[s] = coff[t] + j
        rec, m, su = place[copy[s]], ln(U), U & 1
        V[s] = int(rec["unitig"]) ^ su
        Q[s] = int(rec["len"]) - int(rec["pos"]) - m + p[s] if su else int(rec["pos"]) + p[s]
        clen[s], ccirc[s] = int(rec["len"]), int(rec["circular"])
    join = [0] * n
    for s in range(1, n):
        if follow[s] is not None and copy[s] != NONE and copy[s - 1] != NONE and V[s] == V[s - 1]:
            x = Q[s - 1] + c[s - 1]
            join[s] = int((x % clen[s] if ccirc[s] else x) == Q[s])
    out = {f: [] for f in OUT32}
    path_off = [0]
    items = [0] * case["n_contigs"]
    for r in range(len(po) - 1):
        a = po[r]
        while a < po[r + 1]:
            if copy[a] == NONE:
                a += 1
                continue
            b = a
            while b + 1 < po[r + 1] and join[b + 1] == 1:
                b += 1
            cnt = sum(c[a:b + 1])
            for f, v in (("unitig", V[a]), ("pos", Q[a]), ("count", cnt & NONE), ("item", it[a]), ("flags", fl[a]), ("start", st[a]), ("end", en[b]),
                         ("matched", sum(mi[a:b + 1]) & NONE)):
                out[f].append(v)
            items[V[a] >> 1] += cnt
            a = b + 1
        path_off.append(len(out["unitig"]))
    ref = {f: np.array(v, dtype=np.uint32) for f, v in out.items()}
    ref.update(path_off=np.array(path_off, dtype=np.uint64), step_copy=np.array(copy, dtype=np.uint32), join=np.array(join, dtype=np.uint8),
               V=np.array(V, dtype=np.uint32), Q=np.array(Q, dtype=np.uint32), contig_items=np.array(items, dtype=np.uint64),
               n_steps=len(out["unitig"]), n_merged=sum(join), n_dropped=dropped, n_conflicts=conflicts)
    return ref


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def with_items(paths, matched=False):
    """paths with unitig, pos, count and flags only (test_span.py) -> with item, start and end made up: items go on from step to step,
    with a gap before a step that is not linked"""
    po, c, fl = paths["path_off"].astype(np.int64), paths["count"].astype(np.int64), paths["flags"].astype(np.int64)
    item = np.zeros(len(c), dtype=np.int64)
    for r in range(len(po) - 1):
        x = 0
        for s in range(po[r], po[r + 1]):
            x += 0 if s == po[r] or fl[s] & LINKED else 2
            item[s] = x
            x += c[s]
    out = dict(paths, item=item.astype(np.uint32), start=(7 * item).astype(np.uint32), end=(7 * (item + c - 1) + 30).astype(np.uint32))
    return out


def lift_case(ucase, paths, matched_in=None):
    """an untangle case of test_untangle.py (ro, d, T, resolved, partner, inner, cnt, ec) and paths on its unitigs -> the lift's case;
    the contigs come from the references of test_untangle.py, the copy places from copy_places_reference"""
    r = tun.contigs_reference(ucase)
    u, o = r["u"], r["o"]
    place = copy_places_reference(o, u["origin"], ucase["inner"])
    return {"paths": paths, "matched_in": matched_in, "ro": ucase["ro"], "d": ucase["d"], "uni_off": ucase["inner"]["uni_off"],
            "circular": ucase["inner"]["circular"], "T": ucase["T"], "resolved": ucase["resolved"], "partner": ucase["partner"],
            "copy_off": u["copy_off"], "place": place, "n_copies": u["n_copies"], "n_contigs": o["n_unitigs"], "r": r, "inner": ucase["inner"],
            "origin": u["origin"]}


# ---- hand-made paths over the hand-made untangle cases of test_untangle.py ------------------------------------------------------------
# The contigs of every case, as the references lay them out (asserted in test_reference_hand_made):
#  a: A = 0 (1 member), B = 1 (2), R = 2 (3), C = 3 (1), D = 4 (2); copies 0 A, 1 B, 2 R (A - R - C), 3 R (B - R - D), 4 C, 5 D;
#     contig 0 = A R C (5 instances), contig 1 = B R D (7)
#  b: Q = 0 (1), A = 1 (2), R = 2 (3), P = 3 (1); A+ enters R+ (copy 3, with P) and R- (copy 2, with Q); contig 0 = Q- R+ (4), contig 1 = A
#     (2), contig 2 = R+ P+ (4)
#  c: A 0 (1), B 1 (2), R1 2 (3), C 3 (1), R2 4 (2), D 5 (3), E 6 (1), F 7 (2); contig 0 = A R1 R2 E (7), contig 1 = B R1 C (6), contig 2 =
#     D R2 F (7)
#  f: case a with the lengths 2, 1, 3, 2, 1 and O = 5, a circular unitig of 3 members: contig 0 = A R C (7), contig 1 = B R D (5), contig
#     2 = O, circular
#  g: R = 0 (1), L1 = 1 (2), L2 = 2 (3); one circular contig R L2 R L1 of 7 instances; copy 0 of R lies between L1 and L2
_s, L_ = tb._s, LINKED


def _o(V, pos, count, item, flags, last_item, last_count, matched=None):
    """an output step: start from its first item, end from the last input step of its run; matched = count unless given"""
    return (V, pos, count, item, flags, 7 * item, 7 * (last_item + last_count - 1) + 30, count if matched is None else matched)


# case -> name -> (input steps, copy per input step (None: dropped), join per input step, output steps, conflicts)
H_READS = {
    "a": {
        "a step on an unresolved unitig, on its twin strand": ([_s(9, 1, 1, 0)], [5], [0], [_o(3, 1, 1, 0, 0, 0, 1)], 0),
        "A R C on the forward strand: flank, copy and flank merge into one step": (
            [_s(0, 0, 1, 0), _s(4, 0, 3, 1, L_), _s(6, 0, 1, 4, L_)], [0, 2, 4], [0, 1, 1], [_o(0, 0, 5, 0, 0, 4, 1)], 0),
        "C R A on the twin strand": ([_s(7, 0, 1, 0), _s(5, 0, 3, 1, L_), _s(1, 0, 1, 4, L_)], [4, 2, 0], [0, 1, 1], [_o(1, 0, 5, 0, 0, 4, 1)], 0),
        "B R D takes the other copy": ([_s(2, 0, 2, 0), _s(4, 0, 3, 2, L_), _s(8, 0, 2, 5, L_)], [1, 3, 5], [0, 1, 1], [_o(2, 0, 7, 0, 0, 5, 2)], 0),
        "chosen by its entering edge only: the read ends inside R": ([_s(0, 0, 1, 0), _s(4, 0, 2, 1, L_)], [0, 2], [0, 1], [_o(0, 0, 3, 0, 0, 1, 2)], 0),
        "chosen by its leaving edge only: the read begins inside R": ([_s(4, 1, 2, 0), _s(8, 0, 1, 2, L_)], [3, 5], [0, 1], [_o(2, 3, 3, 0, 0, 2, 1)], 0),
        "ambiguous: neither edge, dropped; the next step is kept": ([_s(4, 0, 2, 0), _s(6, 0, 1, 4)], [None, 4], [0, 0], [_o(0, 4, 1, 4, 0, 4, 1)], 0),
        "a conflict: in by A, out to D": (
            [_s(0, 0, 1, 0), _s(4, 0, 3, 1, L_), _s(8, 0, 2, 4, L_)], [0, 2, 5], [0, 1, 0], [_o(0, 0, 4, 0, 0, 1, 3), _o(2, 5, 2, 4, L_, 4, 2)], 1),
        "a read that ends on A": ([_s(0, 0, 1, 0)], [0], [0], [_o(0, 0, 1, 0, 0, 0, 1)], 0),
        "the next read goes on where it ended: a read's first step is never joined": (
            [_s(4, 0, 3, 1, L_), _s(6, 0, 1, 4, L_)], [2, 4], [0, 1], [_o(0, 1, 4, 1, L_, 4, 1)], 0),
        "an empty read": ([], [], [], [], 0),
    },
    "b": {
        "A+ into R+: the edge that comes first in the row of A+ goes to the later copy": (
            [_s(2, 0, 2, 0), _s(4, 0, 3, 2, L_), _s(6, 0, 1, 5, L_)], [1, 3, 4], [0, 0, 1], [_o(2, 0, 2, 0, 0, 0, 2), _o(4, 0, 4, 2, L_, 5, 1)], 0),
        "A+ into R-: the later edge goes to the earlier copy": (
            [_s(2, 0, 2, 0), _s(5, 0, 3, 2, L_), _s(0, 0, 1, 5, L_)], [1, 2, 0], [0, 0, 1], [_o(2, 0, 2, 0, 0, 0, 2), _o(1, 0, 4, 2, L_, 5, 1)], 0),
    },
    "c": {
        "A R1 R2 E: two resolved unitigs joined by an edge": (
            [_s(0, 0, 1, 0), _s(4, 0, 3, 1, L_), _s(8, 0, 2, 4, L_), _s(12, 0, 1, 6, L_)], [0, 2, 5, 8], [0, 1, 1, 1], [_o(0, 0, 7, 0, 0, 6, 1)], 0),
        "R2 R1 A on the twin strand, from inside R2": (
            [_s(9, 0, 2, 0), _s(5, 0, 3, 2, L_), _s(1, 0, 1, 5, L_)], [5, 2, 0], [0, 1, 1], [_o(1, 1, 6, 0, 0, 5, 1)], 0),
        "D R2 F": ([_s(10, 0, 3, 0), _s(8, 0, 2, 3, L_), _s(14, 0, 2, 5, L_)], [7, 6, 9], [0, 1, 1], [_o(4, 0, 7, 0, 0, 5, 2)], 0),
        "a conflict on R1: in by B, out to R2, whose copy the edge alone picks": (
            [_s(2, 0, 2, 0), _s(4, 0, 3, 2, L_), _s(8, 0, 2, 5, L_)], [1, 3, 5], [0, 1, 0], [_o(2, 0, 5, 0, 0, 2, 3), _o(0, 4, 2, 5, L_, 5, 2)], 1),
    },
    "f": {
        "round the circular unitig more than once": ([_s(10, 1, 7, 0)], [6], [0], [_o(4, 1, 7, 0, 0, 0, 7)], 0),
        "and on its twin strand": ([_s(11, 2, 5, 0)], [6], [0], [_o(5, 2, 5, 0, 0, 0, 5)], 0),
        "A R C beside it": ([_s(0, 0, 2, 0), _s(4, 0, 3, 2, L_), _s(6, 0, 2, 5, L_)], [0, 2, 4], [0, 1, 1], [_o(0, 0, 7, 0, 0, 5, 2)], 0),
    },
    "g": {
        "L1 R L2 R L1 R: round the cycle of copies, joined across the contig's end twice": (
            [_s(2, 0, 2, 0), _s(0, 0, 1, 2, L_), _s(4, 0, 3, 3, L_), _s(0, 0, 1, 6, L_), _s(2, 0, 2, 7, L_), _s(0, 0, 1, 9, L_)], [2, 0, 3, 1, 2, 0],
            [0, 1, 1, 1, 1, 1], [_o(0, 5, 10, 0, 0, 9, 1)], 0),
        "R- L1-, from inside: the wrap on the twin strand": ([_s(1, 0, 1, 0), _s(3, 0, 2, 1, L_)], [0, 2], [0, 1], [_o(1, 6, 3, 0, 0, 1, 2)], 0),
    },
}
H_PLACE = {  # the copy records: (oriented contig, pos, len, circular)
    "a": [(0, 0, 5, 0), (2, 0, 7, 0), (0, 1, 5, 0), (2, 2, 7, 0), (0, 4, 5, 0), (2, 5, 7, 0)],
    "b": [(1, 3, 4, 0), (2, 0, 2, 0), (0, 1, 4, 0), (4, 0, 4, 0), (4, 3, 4, 0)],
    "c": [(0, 0, 7, 0), (2, 0, 6, 0), (0, 1, 7, 0), (2, 2, 6, 0), (2, 5, 6, 0), (0, 4, 7, 0), (4, 3, 7, 0), (4, 0, 7, 0), (0, 6, 7, 0), (4, 5, 7, 0)],
    "f": [(0, 0, 7, 0), (2, 0, 5, 0), (0, 2, 7, 0), (2, 1, 5, 0), (0, 5, 7, 0), (2, 4, 5, 0), (4, 0, 3, 1)],
    "g": [(0, 0, 7, 1), (0, 4, 7, 1), (0, 5, 7, 1), (0, 1, 7, 1)],
}


def hand_lift(name, reads=None):
    reads = [c[0] for c in H_READS[name].values()] if reads is None else reads
    return lift_case(tun.hand(name), tb.paths_of(reads))


def assert_hand(ref, cases, tag):
    """a reference (or device) result against the hand-written table of the reads in `cases`"""
    want = [o for c in cases for o in c[3]]
    for i, f in enumerate(OUT32):
        assert ref[f].tolist() == [o[i] for o in want], (tag, f)
    assert ref["step_copy"].tolist() == [NONE if x is None else x for c in cases for x in c[1]], tag
    assert ref["join"].tolist() == [j for c in cases for j in c[2]], tag
    assert ref["path_off"].tolist() == np.concatenate([[0], np.cumsum([len(c[3]) for c in cases])]).tolist(), tag
    tot = (len(want), sum(sum(c[2]) for c in cases), sum(1 for c in cases for x in c[1] if x is None), sum(c[4] for c in cases))
    assert tuple(ref[f] for f in TOTALS) == tot, (tag, tot)


def check_lift_invariants(ref, case, tag):
    """independent of the reference's join logic: every item of every kept step lands on an instance of the node it was on, in the same
    orientation (through expand_reference); a run's steps lie side by side; the counts add up; heads and tails pair"""
    paths, x, inner = case["paths"], case["r"]["x"], case["inner"]
    xo, io = x["uni_off"].astype(np.int64), inner["uni_off"].astype(np.int64)
    kept = ref["step_copy"] != NONE
    for s in np.nonzero(kept)[0].tolist():
        U, q, V, Q = int(paths["unitig"][s]), int(paths["pos"][s]), int(ref["V"][s]), int(ref["Q"][s])
        m, Lc = int(io[(U >> 1) + 1] - io[U >> 1]), int(xo[(V >> 1) + 1] - xo[V >> 1])
        assert case["origin"][ref["step_copy"][s]] == U >> 1, (tag, s)
        for i in range(int(paths["count"][s])):
            a, b = (q + i) % m, (Q + i) % Lc
            assert (inner["circular"][U >> 1] or q + i < m) and (x["circular"][V >> 1] or Q + i < Lc), (tag, s, i)
            old = int(inner["members"][io[U >> 1] + (m - 1 - a if U & 1 else a)]) ^ (U & 1)
            slot = int(xo[V >> 1] + (Lc - 1 - b if V & 1 else b))
            assert int(x["node_origin"][slot]) == old >> 1 and (int(x["members"][slot]) ^ (V & 1)) & 1 == old & 1, (tag, s, i)
    cnt = paths["count"].astype(np.int64)
    assert int(cnt[kept].sum()) == int(ref["count"].astype(np.int64).sum()) == int(ref["contig_items"].sum()), tag
    mi = cnt if case.get("matched_in") is None else case["matched_in"].astype(np.int64)
    assert int(mi[kept].sum()) == int(ref["matched"].astype(np.int64).sum()), tag
    assert ref["n_steps"] == int((kept & (ref["join"] == 0)).sum()) == int(ref["path_off"][-1]) and not ref["join"][~kept].any(), tag
    assert ref["n_dropped"] == int((~kept).sum()) and ref["n_merged"] == int(ref["join"].sum()), tag
    lin = case["r"]["x"]["circular"][ref["unitig"] >> 1] == 0
    assert (ref["pos"].astype(np.int64) + ref["count"] <= np.diff(xo)[ref["unitig"] >> 1])[lin].all(), tag


def _chained(rng, T0, read_lens, p_break, paired):
    paths, ro, d, off, T = tsp.chained_paths(rng, T0, read_lens, p_break=p_break, paired=paired)
    ln = np.diff(off.astype(np.int64))[paths["unitig"] >> 1]
    paths["pos"] = np.minimum(paths["pos"], ln - paths["count"]).astype(np.uint32)  # as test_walk.chained_case: a broken step stays inside
    return paths, ro, d, off, T


def ring_ucase(rng, T0, read_lens, p_break=0.02, unpaired=0):
    """the paired ring of test_untangle.chain_case through the same generator (tsp.chained_paths, paired), with the paths it was resolved
    by -> (untangle case, paths with item, start and end).  unpaired: as many reads more that change the kind of edge as they go: the
    resolution does not see them, and they cross a resolved unitig by pairs it did not keep"""
    paths, ro, d, off, T = _chained(rng, T0, read_lens, p_break, True)
    ref = tsp.spans_reference(paths, ro, d, off)
    if unpaired:
        more = _chained(rng, T0, [12] * unpaired, p_break, False)[0]
        paths = dict({f: np.concatenate([more[f], paths[f]]) for f in tsp.PATH},  # the unpaired reads first: cut_paths keeps them
                     path_off=np.concatenate([more["path_off"], paths["path_off"][1:] + more["path_off"][-1]]).astype(np.uint64))
    resolved, partner, _, _ = tsp.resolve_reference(ro, d, T, *tsp.count_keys(ref["keys"]), 2)
    ucase = {"ro": ro, "d": d, "T": T, "resolved": resolved, "partner": partner, "inner": tun.inner_of(rng, np.diff(off.astype(np.int64))),
             "cnt": rng.integers(1, 10 ** 6, size=T).astype(np.uint64), "ec": rng.integers(1, 100, size=len(d)).astype(np.uint32)}
    return ucase, with_items(paths)


def ring_case(rng, T0, read_lens, p_break=0.02, n_steps=None, unpaired=0):
    ucase, paths = ring_ucase(rng, T0, read_lens, p_break, unpaired)
    if n_steps is not None:
        assert len(paths["unitig"]) >= n_steps
        paths = tb.cut_paths(paths, n_steps)
    return lift_case(ucase, paths)


def designed_case(rng, n_steps, read_cuts=(), run_cuts=(), drops=(), T0=12):
    """a ring whose every junction is resolved (by 40 reads per kind of edge), and one walk of n_steps whole unitigs along the edges t
    -> t + 1, all linked: a new read begins at read_cuts, the step at run_cuts is not linked (it is chosen by its leaving edge), the
    step at drops is a read of its own (neither edge: dropped)"""
    ucase, _ = ring_ucase(rng, T0, [12] * 160, p_break=0.0)
    assert ucase["resolved"].all()
    ln = np.diff(ucase["inner"]["uni_off"].astype(np.int64)).tolist()
    starts = set(read_cuts) | set(drops) | set(x + 1 for x in drops)
    reads, steps, item = [], [], 0
    for i in range(n_steps):
        if i in starts and steps:
            reads.append(steps)
            steps, item = [], 0
        t = i % T0
        item += 0 if not steps or i not in run_cuts else 3
        steps.append(_s(2 * t, 0, ln[t], item, L_ if steps and i not in run_cuts else 0))
        item += ln[t]
    reads.append(steps)
    return lift_case(ucase, tb.paths_of(reads))


def designed_totals(n_steps, read_cuts=(), run_cuts=(), drops=()):
    """(output steps, dropped, conflicts) of designed_case, where no cut leaves a step beside it without an edge: a run begins at step
    0, at every cut and behind every dropped step"""
    heads = ({0} | set(read_cuts) | set(run_cuts) | set(x + 1 for x in drops)) - set(drops)
    return len([x for x in heads if x < n_steps]), len(drops), 0


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    facade = open(os.path.join(ROOT, "include", "s2k.hpp")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header and s in facade, s
    assert "S2K_ABI_VERSION 2" in header and pkg.ABI_VERSION == 2 and "S2K_NO_COPY" in header
    assert hasattr(pkg.Engine, "unitig_copy_places") and hasattr(pkg.Engine, "paths_lift")
    assert hasattr(pkg.UnitigGraph, "untangle_map") and hasattr(pkg.ContigLift, "lift")
    assert "untangle_map" in pkg.UnitigGraph.untangle.__doc__


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "lift_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lift_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    T, P = pkg.ThreadOut, pkg.NodePlace
    assert facts["sizeof.s2k_thread_out"] == (ctypes.sizeof(T),) and facts["sizeof.s2k_node_place"] == (P.itemsize,) == (16,)
    for f, t in T._fields_:
        assert facts["s2k_thread_out." + f] == (getattr(T, f).offset, ctypes.sizeof(t)), f
    for f in P.names:
        assert facts["s2k_node_place." + f] == (P.fields[f][1], P.fields[f][0].itemsize), f
    assert facts["S2K_NO_COPY"] == (pkg.NO_COPY,) == (NONE,) and facts["S2K_STEP_LINKED"] == (pkg.STEP_LINKED,) == (LINKED,)
    assert facts["S2K_ABI_VERSION"] == (pkg.ABI_VERSION,) and facts["S2K_ERR_INVALID_ARG"] == (1,) and facts["S2K_ERR_CAPACITY"] == (7,)


def test_cpp_lift_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "lift_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lift_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "s2k_lift.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))
    assert "s2k_lift.hip" in next(line for line in open(os.path.join(csrc, "Makefile.asan")).read().split("\n") if line.startswith("ASAN_SRCS"))


@pytest.mark.parametrize("name", sorted(H_READS))
def test_reference_hand_made(name):
    """the copy records, and every copy, join and output step of the hand-made reads, written out by hand: all reads of a case
    together, and each alone"""
    case = hand_lift(name)
    assert case["place"].tolist() == H_PLACE[name]
    ref = lift_reference(case)
    check_lift_invariants(ref, case, name)
    assert_hand(ref, list(H_READS[name].values()), name)
    for read, c in H_READS[name].items():
        one = hand_lift(name, [c[0]])
        assert_hand(lift_reference(one), [c], (name, read))
    if name == "a":  # bridged paths: matched_in is summed in place of count
        mi = (case["paths"]["count"] - (case["paths"]["count"] > 1)).astype(np.uint32)
        ref = lift_reference(dict(case, matched_in=mi))
        assert ref["matched"].tolist()[:3] == [1, 4, 4] and ref["count"].tolist()[:3] == [1, 5, 5] and int(ref["matched"].sum()) == int(mi[ref["step_copy"] != NONE].sum())


def test_reference_nothing_resolved_maps_the_unitig_ids_only():
    """case e of test_untangle.py: every unitig is its own contig, so the lifted paths are the input with the ids mapped (and the
    position mirrored where the contig holds its unitig on the twin strand)"""
    reads = [c[0] for c in H_READS["a"].values()]  # case e has case a's unitigs and edges
    case = lift_case(tun.hand("e"), tb.paths_of(reads))
    ref = lift_reference(case)
    check_lift_invariants(ref, case, "e")
    assert tuple(ref[f] for f in TOTALS) == (len(case["paths"]["unitig"]), 0, 0, 0) and not ref["join"].any()
    for f in ("count", "item", "flags", "start", "end", "path_off"):
        assert ref[f].tobytes() == case["paths"][f].tobytes(), f
    assert ref["matched"].tobytes() == case["paths"]["count"].tobytes() and ref["step_copy"].tolist() == (case["paths"]["unitig"] >> 1).tolist()
    rec = case["place"][case["paths"]["unitig"] >> 1]
    assert (ref["unitig"] == (rec["unitig"] ^ (case["paths"]["unitig"] & 1))).all() and (rec["pos"] == 0).all()
    assert (rec["len"] == np.diff(case["uni_off"].astype(np.int64))[case["paths"]["unitig"] >> 1]).all() and ref["pos"].tobytes() == case["paths"]["pos"].tobytes()


def test_reference_random_paired_rings_invariants():
    rng = np.random.default_rng(81)
    seen = np.zeros(4, dtype=np.int64)
    for T0, n_reads, p_break in ((9, 60, 0.02), (30, 150, 0.05), (50, 300, 0.02), (12, 160, 0.0)):
        case = ring_case(rng, T0, [12] * n_reads, p_break, unpaired=n_reads // 10)
        ref = lift_reference(case)
        check_lift_invariants(ref, case, (T0, n_reads))
        seen += [ref[f] for f in TOTALS]
    assert (seen > [500, 3000, 5, 5]).all(), seen
    for kw in (dict(read_cuts=[2048]), dict(run_cuts=[2047, 2049]), dict(drops=[2047]), dict(drops=[2048], read_cuts=[5], run_cuts=[2046])):
        case = designed_case(np.random.default_rng(82), 4097, **kw)
        ref = lift_reference(case)
        check_lift_invariants(ref, case, kw)
        assert (ref["n_steps"], ref["n_dropped"], ref["n_conflicts"]) == designed_totals(4097, **kw), kw


def _repeat_lift_case(c, oracle, ecoli, paths, matched_in=None):
    ucase, r, nodes, stitched, seqs = tun.repeat_contigs(c, oracle, ecoli)
    case = lift_case(ucase, paths, matched_in)
    assert case["r"]["x"]["node_origin"].tobytes() == r["x"]["node_origin"].tobytes()
    return case


def test_repeat_fixture_lifted_by_the_references(repeat_case, repeat_walks, oracle, ecoli):
    """the clean reads of the repeat fixture: 62 reads, 112 steps, 32 of them on R (18 with both edges, 14 with one, none ambiguous);
    lifted, every read is one step on one contig, field for field the path that test_walk.py threads against that contig, and every
    walk's bases are the read's"""
    c, rw = repeat_case, repeat_walks
    before, after = rw["before"], rw["after"]
    case = _repeat_lift_case(c, oracle, ecoli, before["paths"])
    ref = lift_reference(case)
    check_lift_invariants(ref, case, "repeat")
    R, _ = tsp.through_repeat(c)
    paths = before["paths"]
    follow = twk.follow_reference(paths, c["uro"], c["ud"], c["uni"]["uni_off"])
    on_r = np.nonzero(paths["unitig"] >> 1 == R)[0].tolist()
    last = set((paths["path_off"][1:] - np.uint64(1)).tolist())
    edges = [(follow[s] is not None) + (s not in last and follow[s + 1] is not None) for s in on_r]
    assert (len(c["reads"]), len(paths["unitig"]), len(on_r), edges.count(2), edges.count(1), edges.count(0)) == (62, 112, 32, 18, 14, 0)
    assert ref["n_dropped"] == 0 and ref["n_conflicts"] == 0
    po = ref["path_off"].astype(np.int64)
    for r in range(len(po) - 1):
        assert len(set((ref["unitig"][po[r]:po[r + 1]] >> 1).tolist())) == 1, r
    assert ref["n_steps"] == len(c["reads"]) == 62 and ref["n_merged"] == 112 - 62
    for f in tsp.PATH + ("start", "end", "path_off"):
        assert ref[f].tobytes() == after["paths"][f].tobytes(), f
    lifted = {f: ref[f] for f in STEP + ("path_off",)}
    k = dict(after, paths=lifted)
    wref = twk.reference_of(k)
    assert wref["n_walks"] == 62 and wref["n_off_graph"] == 0
    twk.assert_walks_are_substrings(wref, lifted, rw["reads"], after["strings"], after["overlap"], "lifted")
    assert ref["contig_items"].tolist() == [int(ref["count"][ref["unitig"] >> 1 == t].sum()) for t in range(2)] and ref["contig_items"].min() > 0


def test_noisy_repeat_reads_bridged_then_lifted(repeat_case, noisy_case, repeat_walks, oracle, ecoli):
    """the reads with 1 % substitutions, bridged (16, 2) and lifted with their matched; the figures are printed, not fixed (DESIGN.md
    §3.18 records them)"""
    c, n = repeat_case, noisy_case
    bridged = tb.reference_of(n)
    case = _repeat_lift_case(c, oracle, ecoli, {f: bridged[f] for f in STEP + ("path_off",)}, bridged["matched"])
    ref = lift_reference(case)
    check_lift_invariants(ref, case, "noisy")
    wref = twk.reference_of(dict(repeat_walks["after"], paths={f: ref[f] for f in STEP + ("path_off",)}))
    print("noisy repeat reads, bridged (16, 2) then lifted: %d -> %d steps, %d merged, %d dropped, %d conflicts; %d walks on the contigs" % (
        bridged["n_steps"], ref["n_steps"], ref["n_merged"], ref["n_dropped"], ref["n_conflicts"], wref["n_walks"]))


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = 8
_dev, _host, _ptr = ts._dev, ts._host, ts._ptr
_marked = tb._marked
OUT_DT = dict({f: np.uint32 for f in OUT32 + ("step_copy",)}, path_off=np.uint64, join=np.uint8)
ALL = OUT32 + ("path_off", "join", "step_copy", "contig_items")
ITEMS0 = 1000  # what contig_items holds before a call: the call adds to it


def raw_copy_places(eng, outer, origin, inner, null=(), ctx=True, n_copies=None, n_contigs=None, T=None, shift=0):
    """s2k_unitig_copy_places through ctypes, guard words behind the records -> (status, host records (n, 4) with guards); shift: bytes
    by which the records are moved off their alignment"""
    import torch

    ncp, nt, Tn = len(origin), len(outer["circular"]), len(inner["circular"])
    ins = {"outer_off": _dev(outer["uni_off"], np.uint64), "outer_members": _dev(outer["members"], np.uint32), "outer_circular": _dev(outer["circular"], np.uint8),
           "origin": _dev(origin, np.uint32), "uni_off": _dev(inner["uni_off"], np.uint64), "circular": _dev(inner["circular"], np.uint8)}
    out = torch.full((4 * (max(ncp, 1) + GUARD) + 4,), -0x5A5A, dtype=torch.int32, device="cuda:0")
    P = lambda k: _ptr(ins[k], k in null)  # noqa: E731
    torch.cuda.synchronize()
    s = eng.lib.s2k_unitig_copy_places(eng.ctx if ctx else None, P("outer_off"), P("outer_members"), P("outer_circular"), nt if n_contigs is None else n_contigs,
                                       ncp if n_copies is None else n_copies, P("origin"), P("uni_off"), P("circular"), Tn if T is None else T,
                                       None if "place" in null else ctypes.c_void_p(out.data_ptr() + shift))
    return s, out.cpu().numpy().view(np.uint32)


def device_copy_places(eng, outer, origin, inner, tag):
    want = copy_places_reference(outer, origin, inner)
    s, got = raw_copy_places(eng, outer, origin, inner)
    n = 4 * len(origin)
    assert s == 0 and got[:n].tobytes() == want.tobytes() and _marked(got, n), (tag, s)
    return want


def raw_lift(eng, case, capacity=None, want=ALL, null=(), ctx=True, **over):
    """s2k_paths_lift through ctypes, guard words behind every output -> (status, the four totals, host arrays with guards).  over: paths,
    matched_in, ro, d, uni_off, circular, resolved, partner, copy_off, place replaced; T, n_edges, n_steps, n_reads, n_copies, n_contigs
    given.  null: names of inputs (or `paths`, `out`, a counter n0 .. n3) to pass as NULL"""
    import torch

    paths = over.get("paths", case["paths"])
    arr = {"ro": np.uint64, "d": np.uint32, "uni_off": np.uint64, "circular": np.uint8, "resolved": np.uint8, "partner": np.uint32, "copy_off": np.uint64}
    dv = {k: _dev(over.get(k, case[k]), dt) for k, dt in arr.items()}
    dv["place"] = _dev(np.ascontiguousarray(over.get("place", case["place"])).view(np.uint32), np.uint32)
    mi = over.get("matched_in", case.get("matched_in"))
    dmi = None if mi is None else _dev(mi, np.uint32)
    ns = over.get("n_steps", len(paths["unitig"]))
    nr = over.get("n_reads", len(paths["path_off"]) - 1)
    T, ne = over.get("T", len(case["uni_off"]) - 1), over.get("n_edges", len(case["d"]))
    ncp, nct = over.get("n_copies", case["n_copies"]), over.get("n_contigs", case["n_contigs"])
    dp = {f: _dev(paths[f], np.uint32) for f in STEP}
    dp["path_off"] = _dev(paths["path_off"], np.uint64)
    i = pkg.ThreadOut()
    i.capacity = ns
    for f, t in dp.items():
        if f not in null:
            setattr(i, f, t.data_ptr())
    cap = max(ns, 1) if capacity is None else capacity
    size = {f: cap for f in OUT32}
    size.update(path_off=nr + 1, join=max(ns, 1), step_copy=max(ns, 1))
    res = {f: torch.full((size[f] + GUARD,), tb.FILL[OUT_DT[f]], dtype=getattr(torch, tb.TDT[OUT_DT[f]]), device="cuda:0") for f in want if f != "contig_items"}
    if "contig_items" in want:
        res["contig_items"] = torch.full((max(case["n_contigs"], 1) + GUARD,), ITEMS0, dtype=torch.int64, device="cuda:0")
    o = pkg.ThreadOut()
    o.capacity = cap
    for f, t in res.items():
        if f in STEP + ("path_off",):
            setattr(o, f, t.data_ptr())
    tot = [ctypes.c_uint64(777) for _ in range(4)]
    torch.cuda.synchronize()
    P = lambda k, empty=False: _ptr(dv[k], k in null or empty)  # noqa: E731
    R = lambda f: _ptr(res[f]) if f in res else None  # noqa: E731
    no_edges = len(case["d"]) == 0
    s = eng.lib.s2k_paths_lift(eng.ctx if ctx else None, nr, None if "paths" in null else ctypes.byref(i), ns, None if dmi is None else _ptr(dmi), P("ro"),
                               P("d", no_edges and "d" not in over), ne, P("uni_off"), P("circular"), T, P("resolved"), P("partner", no_edges), P("copy_off"),
                               P("place"), ncp, nct, None if "out" in null else ctypes.byref(o), R("matched"), R("step_copy"), R("join"), R("contig_items"),
                               *(None if "n%d" % k in null else ctypes.byref(x) for k, x in enumerate(tot)))
    got = {f: _host(t, np.uint64 if f == "contig_items" else OUT_DT[f]) for f, t in res.items()}
    return s, tuple(x.value for x in tot), got


def _untouched(got):
    return all(bool((x == ITEMS0).all()) if f == "contig_items" else _marked(x) for f, x in got.items())


def _same(got, ref, case, tag, fields):
    """the device's arrays of `fields` against the reference, and their guards"""
    n, ns, nr, nct = ref["n_steps"], len(case["paths"]["unitig"]), len(case["paths"]["path_off"]) - 1, case["n_contigs"]
    for f in fields:
        if f == "contig_items":
            assert (got[f][:nct] - np.uint64(ITEMS0)).tobytes() == ref[f].tobytes() and bool((got[f][nct:] == ITEMS0).all()), (tag, f)
            continue
        k = n if f in OUT32 else nr + 1 if f == "path_off" else ns
        assert got[f][:k].tobytes() == ref[f].tobytes(), (tag, f, got[f][:8], ref[f][:8])
        assert _marked(got[f], k), (tag, f, "guard")


def device_lift(eng, case, tag, invariants=True):
    """the call against the reference: every array, the totals, the guards; the sizes-only calls; capacity one short; some outputs
    NULL -> the reference"""
    ref = lift_reference(case)
    if invariants:
        check_lift_invariants(ref, case, tag)
    n = ref["n_steps"]
    tot = tuple(ref[f] for f in TOTALS)
    s, t, got = raw_lift(eng, case, capacity=n)
    assert (s, t) == (0, tot), (tag, s, t, tot)
    _same(got, ref, case, tag, ALL)
    for kw in (dict(want=("path_off",)), dict(want=("path_off", "join", "step_copy", "contig_items"), capacity=0)):  # the sizes: no step array
        s, t, got = raw_lift(eng, case, **kw)
        assert (s, t) == (0, tot), (tag, "sizes", kw)
        _same(got, ref, case, (tag, "sizes"), kw["want"])
    if n:  # one short: nothing written, to any array
        s, t, got = raw_lift(eng, case, capacity=n - 1)
        assert (s, t) == (7, tot) and _untouched(got), (tag, "capacity")
        s, t, got = raw_lift(eng, case, capacity=n - 1, want=("path_off", "join", "step_copy", "contig_items", "matched"))  # matched alone is a step array too
        assert (s, t) == (7, tot) and _untouched(got), (tag, "capacity, matched")
    for want in (("path_off", "count", "flags", "matched"), ("path_off", "unitig", "pos", "item", "step_copy")):  # NULL optional outputs
        s, t, got = raw_lift(eng, case, want=want, capacity=n, null=("start", "end"))
        assert (s, t) == (0, tot), (tag, want)
        _same(got, ref, case, (tag, want), want)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(H_READS))
def test_device_hand_made(eng, name):
    """the hand-made reads of a case together and one by one, against the reference and the hand-written tables; the copy records of
    the case from the device"""
    case = hand_lift(name)
    r = case["r"]
    place = device_copy_places(eng, r["o"], r["u"]["origin"], case["inner"], name)
    assert place.tolist() == H_PLACE[name]
    assert_hand(device_lift(eng, case, name), list(H_READS[name].values()), name)
    for read, c in H_READS[name].items():
        assert_hand(device_lift(eng, hand_lift(name, [c[0]]), (name, read)), [c], (name, read))
    device_lift(eng, hand_lift(name, []), (name, "no reads"))
    if name == "a":
        mi = (case["paths"]["count"] - (case["paths"]["count"] > 1)).astype(np.uint32)
        ref = device_lift(eng, dict(case, matched_in=mi), "a, matched_in")
        assert ref["matched"].tolist()[:3] == [1, 4, 4]
        s, t, got = raw_lift(eng, dict(case, matched_in=mi), want=("path_off", "count"), capacity=ref["n_steps"])  # matched_in given, matched not wanted
        assert s == 0 and got["count"][:ref["n_steps"]].tobytes() == ref["count"].tobytes()
        e = lift_case(tun.hand("e"), case["paths"])  # nothing resolved
        ref = device_lift(eng, e, "e")
        assert ref["n_merged"] == 0 and ref["count"].tobytes() == e["paths"]["count"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", [63, 64, 65, 2047, 2048, 2049, 3 * 2048 - 1, 3 * 2048, 3 * 2048 + 1])
def test_device_random_paired_rings(eng, n_steps):
    """random paired rings with reads that cross by unmatched pairs among them, cut to n_steps steps: round one wave, one tile and three
    tiles"""
    rng = np.random.default_rng(800 + n_steps)
    T0 = 9 + n_steps % 7
    case = ring_case(rng, T0, [12] * max(n_steps // 11 + 8, 15 * T0), 0.03, n_steps=n_steps, unpaired=n_steps // 100 + 2)
    ref = device_lift(eng, case, n_steps, invariants=n_steps < 3000)
    assert ref["n_merged"] > n_steps // 4 and ref["n_conflicts"] > 0 and (n_steps < 2000 or ref["n_dropped"] > 0)


@pytest.mark.gpu
def test_device_one_run_longer_than_two_tiles(eng):
    """one read of 5 000 whole unitigs round a paired ring whose every junction is resolved: round and round one circular contig, all
    of it one output step, whose head lies two tiles before its tail"""
    rng = np.random.default_rng(83)
    case = ring_case(rng, 31, [12] * 400 + [5000], 0.0)
    assert case["resolved"].all()
    ref = device_lift(eng, case, "long run", invariants=False)
    a = int(ref["path_off"][-2])
    assert int(ref["path_off"][-1]) - a == 1 and ref["n_merged"] == 5000 - 1 + 400 * 11 and ref["n_steps"] == 401
    first = int(case["paths"]["path_off"][-2])
    assert int(ref["count"][a]) == int(case["paths"]["count"][first:].astype(np.int64).sum()) and case["place"]["circular"].all()


@pytest.mark.gpu
@pytest.mark.parametrize("cuts", [[2048], [2047], [2049], [3, 2049], [2045, 2048, 4096]])
def test_device_tile_run_read_and_drop_boundaries(eng, cuts):
    """runs, reads and dropped steps cut on a tile's last step, on the next tile's first step and one step behind it.  A read that
    begins on step 2 047 has its copy chosen by the edge that step 2 048, the first of the next tile, follows; so has a step there that
    is not linked"""
    rng = np.random.default_rng(sum(cuts))
    for kw in (dict(read_cuts=cuts), dict(run_cuts=cuts), dict(drops=cuts), dict(read_cuts=cuts[:1], run_cuts=[c + 2 for c in cuts], drops=[c + 10 for c in cuts]),
               dict(run_cuts=cuts[:1], drops=[c - 1 for c in cuts])):
        ref = device_lift(eng, designed_case(rng, 4110, **kw), (cuts, kw), invariants=False)
        assert (ref["n_steps"], ref["n_dropped"], ref["n_conflicts"]) == designed_totals(4110, **kw), kw


@pytest.mark.gpu
@pytest.mark.parametrize("n_copies", [63, 64, 65, 255, 256, 257])
def test_device_copy_places_round_a_wave_and_a_block(eng, n_copies):
    rng = np.random.default_rng(n_copies)
    ucase = tun.chain_case(rng, 9, 60, front=n_copies % 3, n_copies=n_copies)
    r = tun.contigs_reference(ucase)
    assert r["u"]["n_copies"] == n_copies and r["u"]["n_duplicated"] > 0
    place = device_copy_places(eng, r["o"], r["u"]["origin"], ucase["inner"], n_copies)
    x = r["x"]  # against the expansion: the first instance of every copy's forward strand
    xo = x["uni_off"].astype(np.int64)
    io = ucase["inner"]["uni_off"].astype(np.int64)
    for c, rec in enumerate(place.tolist()):
        V, q, Lc, circ = rec
        t = int(r["u"]["origin"][c])
        slot = int(xo[V >> 1]) + (Lc - 1 - q if V & 1 else q)
        assert Lc == xo[(V >> 1) + 1] - xo[V >> 1] and circ == x["circular"][V >> 1] and x["node_origin"][slot] == ucase["inner"]["members"][io[t]] >> 1, c


@pytest.mark.gpu
def test_device_copy_places_refusals_nothing_written(eng):
    ucase = tun.hand("a")
    r = tun.contigs_reference(ucase)
    o, origin, inner = r["o"], r["u"]["origin"], ucase["inner"]
    device_copy_places(eng, o, origin, inner, "base")

    def refused(outer=o, origin=origin, inner=inner, code=1, **call):
        s, got = raw_copy_places(eng, outer, origin, inner, **call)
        assert s == code and _marked(got), (s, call)

    x = o["members"].copy()  # an outer member that is no copy
    x[4] = 2 * len(origin)
    refused(outer=dict(o, members=x))
    x = o["members"].copy()  # a copy named twice (and another never): a record would have two writers
    x[4] = x[1] ^ 1
    refused(outer=dict(o, members=x))
    x = origin.copy()  # an origin that is no unitig
    x[2] = ucase["T"]
    refused(origin=x)
    for i, v in ((0, 1), (3, int(inner["uni_off"][2])), (3, int(inner["uni_off"][4]))):  # inner uni_off: not from 0, not strictly ascending
        x = inner["uni_off"].copy()
        x[i] = v
        refused(inner=dict(inner, uni_off=x))
    for i, v in ((0, 1), (1, int(o["uni_off"][2])), (2, len(origin) + 1), (2, len(origin) - 1)):  # outer uni_off
        x = o["uni_off"].copy()
        x[i] = v
        refused(outer=dict(o, uni_off=x))
    big = np.concatenate([[0], np.cumsum([2 ** 31, 2, 2 ** 30, 2 ** 30, 2])]).astype(np.uint64)  # contig 0 = A R C: 2^32 instances, no unitig of 2^32
    refused(inner=dict(inner, uni_off=big))
    big = np.concatenate([[0], np.cumsum([1, 2 ** 32, 3, 1, 2])]).astype(np.uint64)  # a unitig of 2^32 members
    refused(inner=dict(inner, uni_off=big))
    ok = np.concatenate([[0], np.cumsum([2 ** 31, 2, 2 ** 30, 2 ** 30 - 1, 2])]).astype(np.uint64)  # one instance fewer: accepted
    s, got = raw_copy_places(eng, o, origin, dict(inner, uni_off=ok))
    assert s == 0 and got[:4 * len(origin)].tobytes() == copy_places_reference(o, origin, dict(inner, uni_off=ok)).tobytes()
    refused(ctx=False)
    for f in ("outer_off", "outer_members", "outer_circular", "origin", "uni_off", "circular", "place"):
        refused(null=(f,))
    refused(shift=4)  # records that are not 16-byte aligned
    refused(n_copies=2 ** 31)
    refused(n_contigs=len(origin) + 1)
    refused(n_contigs=0)
    refused(T=0)
    assert eng.lib.s2k_unitig_copy_places(eng.ctx, None, None, None, 0, 0, None, None, None, 0, None) == 0  # no copies: nothing read


@pytest.mark.gpu
def test_device_refusals_nothing_written(eng):
    rng = np.random.default_rng(84)
    case = ring_case(rng, 40, [12] * 220, 0.03, unpaired=20)
    paths, ro, d, off = case["paths"], case["ro"], case["d"], case["uni_off"]
    ns, nr, T, ne, ncp, nct = len(paths["unitig"]), len(paths["path_off"]) - 1, case["T"], len(d), case["n_copies"], case["n_contigs"]
    base = device_lift(eng, case, "base")
    assert ns > 2048 and base["n_merged"] > 100 and case["resolved"].sum() > 10

    def refused(code=1, **kw):
        s, t, got = raw_lift(eng, case, **kw)
        assert (s, t) == (code, (0, 0, 0, 0)) and _untouched(got), (s, t, list(kw))

    refused(ctx=False)
    for f in ("paths", "out", "path_off", "ro", "d", "uni_off", "circular", "resolved", "partner", "copy_off", "place", "unitig", "pos", "count", "item", "flags"):
        refused(null=(f,))
    refused(null=("start",))  # out->start wanted, the input has none
    refused(null=("end",))
    for k in range(4):  # a counter that is NULL: the others are not touched
        s, t, got = raw_lift(eng, case, null=("n%d" % k,))
        assert s == 1 and sorted(t) == [0, 0, 0, 777] and _untouched(got)

    def changed(name, i, v, src=None):
        x = (src if src is not None else case[name]).copy()
        x[i] = v
        return {name: x}

    for r, v in ((0, 1), (5, 10 ** 9), (nr, ns - 1), (nr, ns + 1)):  # path_off: not from 0, decreasing, not ending at n_steps
        refused(paths=dict(paths, **changed("path_off", r, v, paths["path_off"])))
    for f, v in (("unitig", 2 * T), ("unitig", 2 ** 32 - 1), ("count", 0), ("count", 4), ("pos", 3)):  # a bad id; unitigs hold 1 .. 3 members
        refused(paths=dict(paths, **changed(f, ns // 2, v, paths[f])))
    refused(T=T - 1)
    for i, v in ((0, 1), (7, int(ro[8]) + 1), (2 * T, ne - 1), (2 * T, ne + 1)):  # the CSR rules
        refused(**changed("ro", i, v))
    refused(**changed("d", ne // 2, 2 * T))
    refused(**changed("uni_off", 11, int(off[10])))  # a unitig without a member
    big = off.copy()
    big[T] += np.uint64(2 ** 32)  # a unitig of 2^32 members
    refused(uni_off=big)
    t1 = int(np.nonzero(case["resolved"])[0][3])
    t0 = int(np.nonzero(case["resolved"] == 0)[0][0]) if not case["resolved"].all() else None
    refused(**changed("resolved", t1, 2))  # a resolved byte above 1
    refused(**changed("resolved", t1, 0))  # two copies of a unitig that is not resolved
    if t0 is not None:
        refused(**changed("resolved", t0, 1))  # one copy of a resolved unitig of two out-edges
    co = case["copy_off"]
    refused(**changed("copy_off", 0, 1))  # not from 0
    refused(**changed("copy_off", T, ncp - 1))  # not ending at n_copies
    refused(**changed("copy_off", T, ncp + 1))
    refused(**changed("copy_off", t1 + 1, int(co[t1])))  # a unitig without a copy
    refused(**changed("copy_off", t1 + 1, int(co[t1 + 2]) + 5))  # decreasing behind it
    refused(n_copies=ncp + 1)
    refused(n_copies=T - 1)
    refused(n_contigs=ncp + 1)
    pl = case["place"]
    c1 = int(co[t1])
    for f, v in (("unitig", 2 * nct), ("pos", int(pl["len"][c1]) - int(off[t1 + 1] - off[t1]) + 1), ("len", 0), ("circular", 2)):  # a copy record outside the contigs
        x = pl.copy()
        x[f][c1] = v
        refused(place=x)
    refused(n_contigs=int(pl["unitig"].max() >> 1))  # fewer contigs than the records name
    z = ctypes.c_uint64(5)
    i, o = pkg.ThreadOut(), pkg.ThreadOut()
    i.path_off = o.path_off = 16
    P = ctypes.c_void_p(16)
    zs = (ctypes.byref(z),) * 4
    tail = (P, P, P, P, 1, 1, ctypes.byref(o), None, None, None, None) + zs
    assert eng.lib.s2k_paths_lift(eng.ctx, 1, ctypes.byref(i), 0, None, P, P, 2 ** 32, P, P, 1, *tail) == 1 and z.value == 0  # before anything is read
    assert eng.lib.s2k_paths_lift(eng.ctx, 1, ctypes.byref(i), 0, None, P, None, 0, P, P, 2 ** 31, *tail) == 1
    assert eng.lib.s2k_paths_lift(eng.ctx, 1, ctypes.byref(i), 0, None, P, None, 0, P, P, 1, P, P, P, P, 2 ** 31, 1, *tail[6:]) == 1
    # no steps: path_off zeroed, nothing else touched; and no reads
    for reads in ([[], [], []], []):
        empty = dict(case, paths=tb.paths_of(reads))
        s, t, got = raw_lift(eng, empty)
        assert (s, t) == (0, (0, 0, 0, 0)) and not got["path_off"][:len(reads) + 1].any() and _marked(got["path_off"], len(reads) + 1)
        assert _untouched({f: x for f, x in got.items() if f != "path_off"})
    s, t, got = raw_lift(eng, case, capacity=base["n_steps"])  # and the call still works
    assert (s, t) == (0, tuple(base[f] for f in TOTALS))


@pytest.mark.gpu
def test_device_deterministic(eng):
    rng = np.random.default_rng(85)
    case = ring_case(rng, 200, [12] * 900, 0.03, unpaired=100)
    runs = []
    for _ in range(2):
        s, t, got = raw_lift(eng, case)
        assert s == 0 and t[1] > 3000 and t[2] > 0 and t[3] > 50, t
        runs.append(b"".join(got[f].tobytes() for f in sorted(got)) + bytes(str(t), "ascii"))
    assert runs[0] == runs[1]


def _read_paths(paths, matched=None):
    """host path arrays -> pkg.ReadPaths on the GPU"""
    n = len(paths["unitig"])
    return pkg.ReadPaths(_dev(paths["path_off"], np.uint64)[:len(paths["path_off"])], **{f: _dev(paths[f], np.uint32)[:n] for f in STEP},
                         matched=None if matched is None else _dev(matched, np.uint32)[:n])


def _unitig_graph(ucase):
    """a pkg.UnitigGraph on the GPU from an untangle case"""
    inner, ne = ucase["inner"], len(ucase["d"])
    src = np.array(tsp._sources([int(x) for x in ucase["ro"]]), dtype=np.uint64)
    keys = (src << np.uint64(32)) | ucase["d"].astype(np.uint64)
    return pkg.UnitigGraph(_dev(inner["uni_off"], np.uint64), _dev(inner["members"], np.uint32), None, None, _dev(inner["circular"], np.uint8),
                           _dev(ucase["cnt"], np.uint64)[:ucase["T"]], _dev(keys, np.uint64)[:ne], _dev(ucase["ec"], np.uint32)[:ne], _dev(ucase["ro"], np.uint64),
                           _dev(ucase["d"], np.uint32)[:ne])


def _assert_lifted(got, ref, tag):
    h = got.host()
    for f in OUT32 + ("path_off",):
        assert h[f].tobytes() == ref[f].tobytes(), (tag, f)


def _stats(paths, ref):
    return {"steps_in": len(paths["unitig"]), "steps_out": ref["n_steps"], "merged": ref["n_merged"], "dropped": ref["n_dropped"], "conflicts": ref["n_conflicts"]}


@pytest.mark.gpu
def test_device_output_is_accepted_downstream(eng, tmp_path):
    """the lifted paths, as the device wrote them, go through s2k_paths_spans and s2k_paths_walks on the contig graph without refusal and
    give what those calls' references give on the reference's lifted paths; untangle_map, ContigLift.lift, write_paths and write_gaf"""
    rng = np.random.default_rng(86)
    ucase, paths = ring_ucase(rng, 60, [12] * 300, 0.03, unpaired=30)
    case = lift_case(ucase, paths)
    ref = lift_reference(case)
    r, x = case["r"], case["r"]["x"]
    s, t, got = raw_lift(eng, case, capacity=ref["n_steps"])
    assert s == 0 and t[1] > 500
    lifted = {f: got[f][:ref["n_steps"]] for f in STEP}
    lifted["path_off"] = got["path_off"][:len(ref["path_off"])]
    sp = tsp.spans_reference(ref, r["cro"], r["cd"], x["uni_off"])
    s, nk, nf, nog, keys = tsp.raw_spans(eng, lifted, r["cro"], r["cd"], x["uni_off"])
    assert (s, nk, nf, nog) == (0, len(sp["keys"]), sp["n_followed"], sp["n_off_graph"]) and keys[:nk].tobytes() == sp["keys"].tobytes()
    nodes = twk.random_records(rng, x["n_members"])
    wbase = {"ro": r["cro"], "d": r["cd"], "uni": x, "nodes": nodes, "mo": twk.member_offsets_reference(x, nodes)}
    wref = twk.reference_of(dict(wbase, paths=ref))
    s, nw, nf, nog, w = twk.raw_walks(eng, dict(wbase, paths=lifted), capacity=wref["n_walks"])
    assert (s, nw, nf, nog) == (0, wref["n_walks"], wref["n_followed"], wref["n_off_graph"])
    for f in twk.REC64 + twk.REC32:
        assert w[f][:nw].tobytes() == wref[f].tobytes(), f
    assert int(wref["items"].sum()) == int(ref["count"].astype(np.int64).sum())
    # the Python layer on a graph object made of the same arrays
    ug = _unitig_graph(ucase)
    res, par = _dev(ucase["resolved"], np.uint8)[:ucase["T"]], _dev(ucase["partner"], np.uint32)[:len(ucase["d"])]
    contigs, node_origin, stats, lift = ug.untangle_map(eng, res, par)
    tun.assert_contigs(contigs, node_origin, stats, r, "untangle_map")
    c2, o2, s2 = ug.untangle(eng, res, par)
    tun.assert_contigs(c2, o2, s2, r, "untangle")
    assert lift.copy_place.cpu().numpy().view(np.uint32).tobytes() == case["place"].tobytes() and tg._u64(lift.copy_off).tobytes() == case["copy_off"].tobytes()
    assert (lift.n_copies, lift.n_contigs, lift.graph) == (case["n_copies"], case["n_contigs"], ug) and lift.resolved is res and lift.partner is par
    import torch

    items = torch.zeros(case["n_contigs"], dtype=torch.int64, device="cuda:0")
    out, st = lift.lift(eng, _read_paths(paths), contig_items=items)
    _assert_lifted(out, ref, "ContigLift.lift")
    assert st == _stats(paths, ref) and tg._u64(items).tobytes() == ref["contig_items"].tobytes()
    out2, _ = lift.lift(eng, _read_paths(paths), contig_items=items)  # a second batch adds to it
    assert tg._u64(items).tobytes() == (2 * ref["contig_items"]).tobytes()
    keys, (nf, nog) = contigs.spans(eng, out)
    assert tg._u64(keys).tobytes() == sp["keys"].tobytes()
    p, q = str(tmp_path / "lifted.paths"), str(tmp_path / "ref.paths")
    out.write_paths(p)
    pkg.write_read_paths(q, ref["path_off"], ref["unitig"], ref["pos"], ref["count"], ref["flags"])
    assert open(p).read() == open(q).read() and len(open(p).read()) > 1000
    b = eng.paths_lift(ug, _read_paths(paths), res, par, lift.copy_off, lift.copy_place, lift.n_contigs, step_copy=True, join=True)
    assert b["join"].cpu().numpy().tobytes() == ref["join"].tobytes() and b["step_copy"].cpu().numpy().view(np.uint32).tobytes() == ref["step_copy"].tobytes()


def _substrings_on_device(eng, contigs, cns, lifted, reads, x, tmp_path, tag):
    """walks of the lifted paths on the contigs, their GAF, and read[qstart:qend] == path[path_start:path_end] on the device's bytes"""
    walks = contigs.walks(eng, lifted, cns)
    out_off, out = contigs.sequences(eng, cns)
    strings = tus.unitig_strings(x, {"out_off": tg._u64(out_off), "out": out.cpu().numpy()})
    twk.assert_walks_are_substrings(walks.host(), lifted.host(), reads, strings, contigs.overlap.cpu().numpy().view(np.uint32), tag)
    p = str(tmp_path / ("%s.gaf" % tag))
    walks.write_gaf(p, contigs)
    assert open(p).read().count("\n") == walks.n_walks
    return walks


@pytest.mark.gpu
def test_repeat_fixture_end_to_end(eng, repeat_case, noisy_case, repeat_walks, oracle, ecoli, tmp_path):
    """thread -> (noisy: bridge) -> spans -> resolve -> untangle_map -> lift -> walks -> write_gaf on the device, for the clean reads and
    for the reads with substitutions; then a second round on the contigs, which have no edges"""
    import torch

    c, R, n = repeat_case, tsp.REPEAT, noisy_case
    clean = twk._extract_all(eng, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [clean], min_count=R["min_count"], min_edge_count=1)
    ug = graph.unitigs(eng)
    tsp._same_graph(ug, c["uro"], c["ud"], c["uni"])
    ns = pkg.NodeSequences.build(eng, graph, [clean])
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    noisy = twk._extract_all(eng, n["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    plain = ug.thread(eng, table, clean, len(c["reads"]), min_count=R["min_count"])
    bridged, _ = ug.bridge(eng, ug.thread(eng, table, noisy, len(n["reads"]), min_count=R["min_count"]))
    table.close()
    x = None
    for tag, paths, reads, ref_paths, ref_matched in (("clean", plain, c["reads"], repeat_walks["before"]["paths"], None),
                                                      ("noisy", bridged, n["reads"], None, None)):
        if ref_paths is None:
            b = tb.reference_of(n)
            ref_paths, ref_matched = {f: b[f] for f in STEP + ("path_off",)}, b["matched"]
        case = _repeat_lift_case(c, oracle, ecoli, ref_paths, ref_matched)
        ref, x = lift_reference(case), case["r"]["x"]
        resolved, partner, rs = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
        assert rs == {"candidates": 1, "resolved": 1}
        contigs, node_origin, st, lift = ug.untangle_map(eng, resolved, partner)
        assert st == {"copies": 6, "duplicated": 1, "contigs": 2} and lift.copy_place.cpu().numpy().view(np.uint32).tobytes() == case["place"].tobytes()
        items = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        lifted, ls = lift.lift(eng, paths, contig_items=items)
        _assert_lifted(lifted, ref, tag)
        assert ls == _stats(ref_paths, ref) and tg._u64(items).tobytes() == ref["contig_items"].tobytes()
        cns = ns.take(node_origin)
        if tag == "clean":
            assert (ls["dropped"], ls["conflicts"], ls["steps_out"]) == (0, 0, len(reads))
            walks = _substrings_on_device(eng, contigs, cns, lifted, reads, x, tmp_path, tag)
            assert walks.n_walks == len(reads)
        else:  # a read with errors is no substring; its walks still come out, and their GAF lines
            walks = contigs.walks(eng, lifted, cns)
            walks.write_gaf(str(tmp_path / "noisy.gaf"), contigs)
        print("%s repeat reads on the device: %d -> %d steps (%d merged, %d dropped, %d conflicts), %d walks on the contigs" % (
            tag, ls["steps_in"], ls["steps_out"], ls["merged"], ls["dropped"], ls["conflicts"], walks.n_walks))
        # the second round: the two contigs have no edges, so nothing is a candidate, the untangling is the identity and so is the lift
        r2, p2, rs2 = contigs.resolve(eng, contigs.span_table(eng, [lifted]), min_support=2)
        assert rs2 == {"candidates": 0, "resolved": 0} and contigs.n_edges == 0
        contigs2, origin2, st2, lift2 = contigs.untangle_map(eng, r2, p2)
        assert st2 == {"copies": 2, "duplicated": 0, "contigs": 2}
        again, ls2 = lift2.lift(eng, lifted)
        assert (ls2["steps_out"], ls2["merged"], ls2["dropped"], ls2["conflicts"]) == (ls["steps_out"], 0, 0, 0)
        h, g, rec = lifted.host(), again.host(), lift2.copy_place.cpu().numpy().view(np.uint32).reshape(-1, 4)
        for f in ("pos", "count", "item", "flags", "start", "end", "matched", "path_off"):
            assert g[f].tobytes() == h[f].tobytes(), (tag, "second round", f)
        assert (rec[:, 1] == 0).all() and not (rec[:, 0] & 1).any() and (g["unitig"] == rec[h["unitig"] >> 1, 0] ^ (h["unitig"] & 1)).all()
        assert sorted(origin2.cpu().numpy().tolist()) == list(range(contigs.n_nodes))  # the identity, up to the contigs' numbering


@pytest.mark.gpu
def test_ecoli_reads_with_errors_through_the_simplified_graph(eng, ecoli):
    """the 600 reads with 0.5 % substitutions through simplify(10, 20) and bridge(16, 2): nothing resolves there, so the lift maps the
    unitig ids and nothing else; the device's arrays are compared with the reference's all the same"""
    mc, l, k = 2, 12, 5
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    outs = twk._extract_all(eng, reads, l, k, 0.05, pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=mc, min_edge_count=1)
    sg, node_map, _ = graph.simplify(eng, 10, 20)
    ug = sg.unitigs(eng)
    table = pkg.CountTable(eng, sg.keys, sg.counts)
    paths = ug.thread(eng, table, outs, len(reads), min_count=mc)
    table.close()
    bridged, _ = ug.bridge(eng, paths)
    resolved, partner, rs = ug.resolve(eng, ug.span_table(eng, [bridged]), min_support=2)
    contigs, node_origin, st, lift = ug.untangle_map(eng, resolved, partner)
    lifted, ls = lift.lift(eng, bridged)
    h = bridged.host()
    case = {"paths": h, "matched_in": h["matched"], "ro": tg._u64(ug.row_off), "d": ug.dst.cpu().numpy().view(np.uint32), "uni_off": tg._u64(ug.uni_off),
            "resolved": resolved.cpu().numpy(), "partner": partner.cpu().numpy().view(np.uint32), "copy_off": tg._u64(lift.copy_off),
            "place": lift.copy_place.cpu().numpy().view(np.uint32).reshape(-1).view(pkg.NodePlace), "n_contigs": lift.n_contigs}
    ref = lift_reference(case)
    _assert_lifted(lifted, ref, "ecoli")
    assert ls == _stats(h, ref)
    if rs["resolved"] == 0:
        assert (ls["steps_out"], ls["merged"], ls["dropped"], ls["conflicts"]) == (bridged.n_steps, 0, 0, 0) and st["copies"] == ug.n_unitigs
        for f in ("count", "item", "flags", "start", "end", "matched", "path_off"):
            assert lifted.host()[f].tobytes() == h[f].tobytes(), f
    walks = contigs.walks(eng, lifted, pkg.NodeSequences.build(eng, graph, [outs]).subset(node_map).take(node_origin))
    print("simplified E. coli, 0.5 %% substitutions, bridge(16, 2), lifted: %d resolved of %d candidates, %d -> %d steps, %d dropped, %d conflicts, %d walks" % (
        rs["resolved"], rs["candidates"], ls["steps_in"], ls["steps_out"], ls["dropped"], ls["conflicts"], walks.n_walks))
