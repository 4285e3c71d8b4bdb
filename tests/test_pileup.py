"""Pile-up and consensus: s2k_walks_pileup and s2k_pileup_consensus (include/s2k.h), UnitigGraph.pileup, Pileup and
PolishedSequences.  The references are `pileup_reference` and `consensus_reference`, serial restatements of the header's rules on top of
test_align.walk_alignments_reference and test_walk.stitched_path; the device's arrays equal the references byte for byte, between guards."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import test_align as ta
import test_graph as tg
import test_simplify as ts
import test_span as tsp
import test_unitig_sequences as tus
import test_walk as twk
from test_align import ecoli_reference, noisy_walks  # noqa: F401  (module-scoped fixtures)
from test_bridge import noisy_case  # noqa: F401
from test_span import repeat_case  # noqa: F401
from test_walk import repeat_walks  # noqa: F401

pkg = import_package()

SYMS = ("s2k_walks_pileup", "s2k_pileup_consensus")
I, D, EQ, X = 1, 2, 7, 8
OPC = {"I": I, "D": D, "=": EQ, "X": X}
PLANES = ("match", "del", "sub0", "sub1", "sub2", "sub3", "ins0", "ins1", "ins2", "ins3", "ins_long")
P_STATS = ("walks_used", "walks_skipped", "n_other", "n_end_ins", "n_shifted", "n_empty_ins")
C_STATS = ("n_low", "n_sub", "n_del", "n_ins", "n_long")
MAX_SHIFT = 64
REC = ("first_step", "n_steps", "path_start", "path_end", "flags")
_CODE = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c + 32] = _i
_COMP = np.arange(256, dtype=np.uint8)
_COMP[list(b"ACGTacgt")] = list(b"TGCAtgca")


# ---- the references ----------------------------------------------------------------------------------------------------------------
def draft_of(strings):
    """-> (out_off uint64, out uint8): the unitigs' bases back to back"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint64)
    return off, np.frombuffer(b"".join(strings), dtype=np.uint8)


def walk_sources(walks, w, u, strings, overlap, off):
    """where every byte of walk w's target comes from -> (seg, pos, odd, end): per target byte its step (on a circular walk its round),
    its forward position in the draft, whether the step runs on an odd unitig, and the end of that unitig in the draft; four empty
    arrays for a walk that s2k_walks_targets calls bad"""
    a, n = int(walks["first_step"][w]), int(walks["n_steps"][w])
    ps, pe, circ = int(walks["path_start"][w]), int(walks["path_end"][w]), int(walks["flags"][w]) & 1
    L = lambda U: len(strings[U >> 1])  # noqa: E731
    none = tuple(np.zeros(0, dtype=np.int64) for _ in range(4))
    units = [int(x) for x in u[a:a + n]]
    if ps > pe:
        return none
    seg, pos, odd, end = [], [], [], []

    def take(X, j, U, start):  # the path coordinates X lie in step j, whose string starts at path coordinate `start`
        o, base = X - start, int(off[U >> 1])
        seg.append(np.full(len(X), j, dtype=np.int64))
        pos.append(base + (L(U) - 1 - o if U & 1 else o))
        odd.append(np.full(len(X), U & 1, dtype=np.int64))
        end.append(np.full(len(X), base + L(U), dtype=np.int64))

    if circ:
        if n == 0 or L(units[0]) == 0:
            return none
        L0 = L(units[0])
        for k in range(ps // L0, (pe + L0 - 1) // L0 + 1):  # round k: path coordinates [k L0, (k + 1) L0)
            take(np.arange(max(k * L0, ps), max(min((k + 1) * L0, pe), max(k * L0, ps)), dtype=np.int64), k, units[0], k * L0)
    else:
        if any(int(overlap[units[j - 1]]) > min(L(units[j - 1]), L(units[j])) for j in range(1, n)):
            return none
        start = prev_end = 0
        spans = []
        for j, U in enumerate(units):
            if j:
                start = prev_end - int(overlap[units[j - 1]])
            spans.append((prev_end if j else 0, start + L(U), j, U, start))  # overlapped bytes belong to the earlier step
            prev_end = start + L(U)
        if pe > prev_end:
            return none
        for lo, hi, j, U, start in spans:
            take(np.arange(max(lo, ps), max(min(hi, pe), max(lo, ps)), dtype=np.int64), j, U, start)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64)  # noqa: E731
    return cat(seg), cat(pos), cat(odd), cat(end)


def _pieces(seg, pos, odd, x0, x1):
    """the target bytes [x0, x1) cut where the step changes -> [(x, xe, a, b)]: the piece and its forward interval [a, b)"""
    out, x = [], x0
    while x < x1:
        xe = x + 1
        while xe < x1 and seg[xe] == seg[x]:
            xe += 1
        a, b = (int(pos[xe - 1]), int(pos[x]) + 1) if odd[x] else (int(pos[x]), int(pos[xe - 1]) + 1)
        out.append((x, xe, a, b))
        x = xe
    return out


def new_pile(n_bases):
    return {f: np.zeros(n_bases, dtype=np.uint32) for f in PLANES}


def pileup_reference(walks, step_unitig, strings, overlap, queries, flags, runs, max_shift=MAX_SHIFT, pile=None):
    """the rule of include/s2k.h, walk by walk and run by run.  queries: per walk the bytes its runs consume; flags: per walk the
    alignment's flags; runs: per walk [(len, op code)] -> (pile: dict of uint32 planes, stats dict).  pile: a pile to add to (copied)"""
    off, out = draft_of(strings)
    acc = {f: (pile[f].astype(np.int64) if pile is not None else np.zeros(len(out), dtype=np.int64)) for f in PLANES}
    st = dict.fromkeys(P_STATS, 0)
    u = [int(x) for x in step_unitig]
    for w in range(len(walks["first_step"])):
        if int(flags[w]):
            st["walks_skipped"] += 1
            continue
        st["walks_used"] += 1
        seg, pos, odd, end = walk_sources(walks, w, u, strings, overlap, off)
        T, q, R = len(seg), queries[w], runs[w]
        assert sum(ln for ln, op in R if op != I) == T and sum(ln for ln, op in R if op != D) <= len(q), (w, "the runs consume the target")
        x = qi = 0
        for i, (ln, op) in enumerate(R):
            nxt, prv = (R[i + 1] if i + 1 < len(R) else None), (R[i - 1] if i else None)
            if op == I:
                c = q[qi:qi + ln]
                qi += ln
                if T == 0:
                    st["n_empty_ins"] += 1
                    continue
                xb = x - 1 if x else 0
                o, s = int(odd[xb]), seg[xb]
                g = int(pos[xb]) + ((0 if x else 1) if o else (1 if x else 0))
                nb, e = (nxt if o else prv), 0
                if nb is not None and nb[1] == EQ:  # the neighbour's piece next to the gap, as far as it lies in the gap's step
                    if o:
                        while e < nb[0] and x + e < T and seg[x + e] == s:
                            e += 1
                    else:
                        while e < nb[0] and x - 1 - e >= 0 and seg[x - 1 - e] == s:
                            e += 1
                fwd = bytes(_COMP[np.frombuffer(c, dtype=np.uint8)][::-1]) if o else c
                d = 0
                while d < min(e, max_shift) and out[g - (d + 1)] == fwd[ln - 1 - (d % ln)]:
                    d += 1
                st["n_shifted"] += d > 0
                if g - d == int(end[xb]):
                    st["n_end_ins"] += 1
                    continue
                code = int(_CODE[fwd[0]]) if ln == 1 else 4
                acc["ins%d" % code if code < 4 else "ins_long"][g - d] += 1
                continue
            pcs = _pieces(seg, pos, odd, x, x + ln)
            if op == EQ:
                for _, _, a, b in pcs:
                    acc["match"][a:b] += 1
            elif op == X:
                for y in range(x, x + ln):
                    code = int(_CODE[q[qi + y - x]])
                    if code == 4:
                        st["n_other"] += 1
                    else:
                        acc["sub%d" % (3 - code if odd[y] else code)][int(pos[y])] += 1
            else:
                d = 0
                if len(pcs) == 1:
                    _, _, a, b = pcs[0]
                    o, s = int(odd[x]), seg[x]
                    nb, e = (nxt if o else prv), 0
                    if nb is not None and nb[1] == EQ:
                        if o:
                            while e < nb[0] and x + ln + e < T and seg[x + ln + e] == s:
                                e += 1
                        else:
                            while e < nb[0] and x - 1 - e >= 0 and seg[x - 1 - e] == s:
                                e += 1
                    while d < min(e, max_shift) and out[a - (d + 1)] == out[b - (d + 1)]:
                        d += 1
                    st["n_shifted"] += d > 0
                    acc["del"][a - d:b - d] += 1
                    if d:  # the neighbouring = piece: without [a - d, a), with [b - d, b) in its place
                        acc["match"][a - d:a] -= 1
                        acc["match"][b - d:b] += 1
                else:
                    for _, _, a, b in pcs:
                        acc["del"][a:b] += 1
            x += ln
            qi += ln if op != D else 0
    assert all((v >= 0).all() for v in acc.values())
    return {f: v.astype(np.uint32) for f, v in acc.items()}, st


def depth_of(pile):
    return sum(pile[f].astype(np.int64) for f in PLANES[:6])


def consensus_reference(pile, strings, overlap, min_cov=3):
    """the call of include/s2k.h -> dict: strings (the polished unitigs), out_off, out, pos_map (uint64, n_bases + 1), overlap (uint32)
    and the stats"""
    off, out = draft_of(strings)
    n = len(out)
    P = {f: pile[f].astype(np.int64) for f in PLANES}
    cur = _CODE[out]
    at = np.arange(n)
    tot = np.zeros((5, n), dtype=np.int64)
    ins = np.zeros((4, n), dtype=np.int64)
    for c in range(4):
        tot[c], ins[c] = P["sub%d" % c], P["ins%d" % c]
    tot[cur, at] += P["match"]
    depth = P["match"] + P["del"] + sum(P["sub%d" % c] for c in range(4))
    low = depth < min_cov
    best = ins.argmax(axis=0)  # the smallest code among equals
    do_ins = ~low & (2 * ins[best, at] > depth)
    top = tot.argmax(axis=0)
    drop = ~low & (P["del"] > tot[top, at])
    keep = low | (~drop & (tot[cur, at] == tot[top, at]))
    subst = ~low & ~drop & ~keep
    long_ = ~low & (2 * P["ins_long"] > depth)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    base = np.where(keep, out, letters[np.minimum(top, 3)])
    cnt = do_ins.astype(np.int64) + (~drop).astype(np.int64)
    pm = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    new = np.zeros(int(pm[-1]), dtype=np.uint8)
    new[pm[:-1][do_ins]] = letters[best[do_ins]]
    new[(pm[:-1] + do_ins)[~drop]] = base[~drop]
    new_off = pm[off.astype(np.int64)]
    ov = np.zeros(2 * len(strings), dtype=np.uint32)
    for t, s in enumerate(strings):
        a, L = int(off[t]), len(s)
        e, o = min(int(overlap[2 * t]), L), min(int(overlap[2 * t + 1]), L)
        ov[2 * t], ov[2 * t + 1] = pm[a + L] - pm[a + L - e], pm[a + o] - pm[a]
    text = new.tobytes()
    stats = {"n_low": int(low.sum()), "n_sub": int(subst.sum()), "n_del": int(drop.sum()), "n_ins": int(do_ins.sum()), "n_long": int(long_.sum())}
    return {"strings": [text[int(new_off[t]):int(new_off[t + 1])] for t in range(len(strings))], "out_off": new_off.astype(np.uint64), "out": new,
            "pos_map": pm.astype(np.uint64), "overlap": ov, "stats": stats}


def walk_inputs(walks, step_unitig, strings, overlap, reads, max_edits=ta.MAX_EDITS):
    """walks with walk_off, qstart and qend over `reads` -> (queries, flags, runs) by test_align.walk_alignments_reference"""
    al = ta.walk_alignments_reference(walks, step_unitig, strings, overlap, reads, max_edits)
    return [p[0] for p in al["pairs"]], al["flags"], [r[2] for r in al["res"]], al


def runs_of(cigar):
    """"12=1X3I" -> [(12, 7), (1, 8), (3, 1)]"""
    out, n = [], ""
    for ch in cigar:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), OPC[ch]))
            n = ""
    return out


def query_of(rng, target, runs, alphabet=b"ACGT"):
    """a query that the runs align to the target: = copies, X takes another letter, I takes letters at random"""
    q, x = bytearray(), 0
    for ln, op in runs:
        if op == EQ:
            q += target[x:x + ln]
        elif op == X:
            q += bytes([c for c in alphabet if c != target[x + i]][int(rng.integers(0, len(alphabet) - 1))] for i in range(ln))
        elif op == I:
            q += ta.random_seq(rng, ln, alphabet)
        x += ln if op != I else 0
    assert x == len(target)
    return bytes(q)


def one_walks(specs):
    """specs: [(first_step, n_steps, path_start, path_end, flags)] -> the record arrays"""
    return {f: np.array([s[i] for s in specs], dtype=np.uint64 if f in ("first_step", "path_start", "path_end") else np.uint32) for i, f in enumerate(REC)}


def targets_of(walks, su, strings, overlap):
    toff, tgt, bad = ta.targets_reference(walks, su, strings, overlap)
    return [tgt[int(toff[w]):int(toff[w + 1])] for w in range(len(bad))], bad


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    facade = open(os.path.join(ROOT, "include", "s2k.hpp")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header and s in facade, s
    assert hasattr(pkg.Engine, "walks_pileup") and hasattr(pkg.Engine, "pileup_consensus") and hasattr(pkg.UnitigGraph, "pileup")
    assert all(hasattr(pkg.Pileup, f) for f in ("add", "depth", "consensus", "host"))
    assert pkg.PILEUP_PLANES == PLANES and pkg.PILEUP_STATS == P_STATS and pkg.CONSENSUS_STATS == C_STATS


def test_new_source_is_in_the_build():
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "s2k_pileup.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))
    assert "s2k_pileup.hip" in next(line for line in open(os.path.join(csrc, "Makefile.asan")).read().split("\n") if line.startswith("ASAN_SRCS"))
    assert os.path.exists(os.path.join(csrc, "s2k_pileup.hip"))


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "pileup_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pileup_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    A = pkg.Pile
    assert facts["sizeof.s2k_pile"] == (ctypes.sizeof(A),) == (8 * len(PLANES),)
    for f, t in A._fields_:
        assert facts["s2k_pile." + f.rstrip("_")] == (getattr(A, f).offset, ctypes.sizeof(t)), f
    assert [f.rstrip("_") for f, _ in A._fields_] == ["match", "del", "sub", "ins", "ins_long"]  # the planes in the order of PILEUP_PLANES
    assert facts["S2K_PILEUP_MAX_SHIFT"] == (pkg.PILEUP_MAX_SHIFT,) == (MAX_SHIFT,)
    assert facts["S2K_PILEUP_STATS"] == (pkg.PILEUP_STATS_WORDS,) and facts["S2K_CONSENSUS_STATS"] == (pkg.CONSENSUS_STATS_WORDS,)
    assert len(P_STATS) <= pkg.PILEUP_STATS_WORDS and len(C_STATS) <= pkg.CONSENSUS_STATS_WORDS
    assert facts["S2K_ALIGN_OVER"] == (pkg.ALIGN_OVER,) and facts["S2K_ALIGN_BAD_PATH"] == (pkg.ALIGN_BAD_PATH,)


def test_cpp_pileup_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "pileup_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pileup_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


# two unitigs of 40 and 30 bases; the overlap that leaves 0+ is 6, the one that leaves 1- is 6 (the same junction on the twin strands)
def two_unitigs(seed=90, la=40, lb=30, ov=6):
    rng = np.random.default_rng(seed)
    a = ta.random_seq(rng, la)
    b = a[la - ov:] + ta.random_seq(rng, lb - ov)
    overlap = np.array([ov, 0, 0, ov], dtype=np.uint32)
    return [a, b], overlap, np.array([0, 2, 3, 1], dtype=np.uint32)  # steps 0, 1: 0+ 1+; steps 2, 3: 1- 0-


def junction_cases():
    """for every run kind, a run of three that ends one before, on and one behind the junction of a two-step walk, on even and on odd
    steps -> [(tag, walks, su, strings, overlap, queries, runs)]"""
    strings, overlap, su = two_unitigs()
    rng = np.random.default_rng(91)
    out = []
    for first, name in ((0, "even"), (2, "odd")):
        walks = one_walks([(first, 2, 2, 60, 0)])
        (target,), bad = targets_of(walks, su, strings, overlap)
        assert not bad.any() and len(target) == 58
        J = (40 if first == 0 else 30) - 2  # the first target byte of the second step
        for kind in "=XDI":
            for delta in (-1, 0, 1):
                n = 3
                pre = J + delta - (n if kind != "I" else 0)
                rest = len(target) - pre - (n if kind != "I" else 0)
                mid = "1X" if kind == "=" else ""  # an = run of its own between two X
                cigar = "%d=%s%d%s%s%d=" % (pre - len(mid) // 2, mid, n, kind, mid, rest - len(mid) // 2)
                runs = runs_of(cigar)
                out.append(("%s %s %+d" % (name, kind, delta), walks, su, strings, overlap, [query_of(rng, target, runs)], [runs]))
    return out


def test_reference_junction_cases_by_hand():
    """what the pieces of a run that crosses a junction are, checked against positions counted by hand"""
    cases = {c[0]: c for c in junction_cases()}
    strings, overlap, su = two_unitigs()
    # even: step 0 is unitig 0 forward, target byte x at draft position 2 + x up to x = 37; step 1 gives byte 38 on at 40 + 6 + (x - 38)
    pile, st = pileup_reference(*cases["even D +0"][1:6], [0], cases["even D +0"][6])
    assert np.nonzero(pile["del"])[0].tolist() == [37, 38, 39] and st["n_shifted"] in (0, 1)
    pile, _ = pileup_reference(*cases["even D +1"][1:6], [0], cases["even D +1"][6], max_shift=0)
    assert np.nonzero(pile["del"])[0].tolist() == [38, 39, 46] and pile["match"][40:46].tolist() == [0] * 6  # two pieces; the overlap's second copy gets no vote
    # odd: step 0 is unitig 1 reversed: target byte x at 40 + 29 - (2 + x) up to x = 27; step 1 gives byte 28 on at 39 - 6 - (x - 28)
    pile, _ = pileup_reference(*cases["odd D +1"][1:6], [0], cases["odd D +1"][6], max_shift=0)
    assert np.nonzero(pile["del"])[0].tolist() == [33, 40, 41]
    pile, _ = pileup_reference(*cases["odd I +0"][1:6], [0], cases["odd I +0"][6], max_shift=0)
    assert [np.nonzero(pile[f])[0].tolist() for f in ("ins_long",)] == [[40]]  # between bytes 27 and 28: it belongs to byte 27's step, p(27) = 40
    pile, st = pileup_reference(*cases["even I +0"][1:6], [0], cases["even I +0"][6], max_shift=0)
    assert not pile["ins_long"].any() and st["n_end_ins"] == 1  # p(37) + 1 = 40: the end of unitig 0
    for tag, *c in junction_cases():
        for ms in (0, MAX_SHIFT):
            pile, st = pileup_reference(*c[:5], [0], c[5], max_shift=ms)
            total = sum(int(pile[f].astype(np.int64).sum()) for f in PLANES)
            want = sum(ln if op != I else 1 for ln, op in c[5][0]) - st["n_end_ins"] - st["n_other"]
            assert total == want, (tag, ms, total, want)


def planted_case(seed, alphabet, n=3000, gap=24, read=400, step=50):
    """a clean string, a draft with an edit planted every `gap` bases (substitution, extra base, missing base in turn), and reads of
    the clean string tiled on alternating strands, each one walk of one step on the draft's unitig; the two ends covered four times"""
    rng = np.random.default_rng(seed)
    clean = ta.random_seq(rng, n, alphabet)
    draft, cmap = bytearray(), []
    for i, c in enumerate(clean):
        cmap.append(len(draft))
        kind = (i // gap) % 3 if i and i % gap == 0 else -1
        if kind == 0:
            draft.append([x for x in b"ACGT" if x != c][int(rng.integers(0, 3))])
        elif kind == 1:
            draft += bytes([alphabet[int(rng.integers(0, len(alphabet)))], c])
        elif kind != 2:
            draft.append(c)
    cmap.append(len(draft))
    draft = bytes(draft)
    n_edits = len(range(gap, n, gap))
    starts = list(range(0, n - read + 1, step))
    starts = [0] * 3 + starts + [starts[-1]] * 3
    reads, specs = [], []
    for r, s in enumerate(starts):
        a, b = cmap[s], cmap[s + read]
        if r % 2 == 0:
            reads.append(clean[s:s + read])
            specs.append((0, 1, a, b, 0))
        else:
            reads.append(tus.revcomp(clean[s:s + read]))
            specs.append((1, 1, len(draft) - b, len(draft) - a, 0))
    walks = one_walks(specs)
    walks.update(walk_off=np.arange(len(reads) + 1, dtype=np.uint64), qstart=np.zeros(len(reads), dtype=np.uint32),
                 qend=np.full(len(reads), read, dtype=np.uint32))
    return clean, draft, walks, reads, n_edits


@pytest.mark.parametrize("alphabet", [b"ACGT", b"AACGAA", b"AC"])
def test_planted_edits_are_polished_away_and_only_with_the_shift(alphabet):
    su, ov = np.array([0, 1], dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    left = 0
    for seed in range(6):
        clean, draft, walks, reads, n_edits = planted_case(seed, alphabet)
        q, fl, runs, _ = walk_inputs(walks, su, [draft], ov, reads)
        assert not fl.any() and n_edits == 124
        pile, st = pileup_reference(walks, su, [draft], ov, q, fl, runs)
        c = consensus_reference(pile, [draft], ov, 3)
        assert c["strings"][0] == clean and c["stats"]["n_low"] == 0, (alphabet, seed, c["stats"], st)
        assert c["stats"]["n_sub"] + c["stats"]["n_del"] + c["stats"]["n_ins"] == n_edits and c["stats"]["n_long"] == 0
        plain, st0 = pileup_reference(walks, su, [draft], ov, q, fl, runs, max_shift=0)
        assert st0["n_shifted"] == 0
        c0 = consensus_reference(plain, [draft], ov, 3)
        left += c0["strings"][0] != clean
        print("%s seed %d: %d edits planted, %d gaps shifted; without the shift the polished string %s the clean one" % (
            alphabet.decode(), seed, n_edits, st["n_shifted"], "equals" if c0["strings"][0] == clean else "differs from"))
    assert left >= 3, "without normalisation, edits survive"  # a kernel that skips the shift does not pass the first assertion


def test_reference_invariants_depth_sum_strands_and_batches():
    clean, draft, walks, reads, _ = planted_case(7, b"ACGT")
    su, ov = np.array([0, 1], dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    q, fl, runs, _ = walk_inputs(walks, su, [draft], ov, reads)
    pile, st = pileup_reference(walks, su, [draft], ov, q, fl, runs)
    # depth[p] = the walks whose alignment covers p: a walk's runs tile its whole path interval
    cover = np.zeros(len(draft), dtype=np.int64)
    for w in range(len(reads)):
        ps, pe = int(walks["path_start"][w]), int(walks["path_end"][w])
        a, b = (ps, pe) if walks["first_step"][w] == 0 else (len(draft) - pe, len(draft) - ps)
        cover[a:b] += 1
    assert (depth_of(pile) == cover).all()
    total = sum(int(pile[f].astype(np.int64).sum()) for f in PLANES)
    assert total == sum(ln if op != I else 1 for r in runs for ln, op in r) - st["n_end_ins"] - st["n_other"] - st["n_empty_ins"]
    # two adds equal one add of both batches
    h = len(reads) // 2
    part = lambda a, b: ({f: walks[f][a:b] for f in REC}, q[a:b], fl[a:b], runs[a:b])  # noqa: E731
    w1, q1, f1, r1 = part(0, h)
    w2, q2, f2, r2 = part(h, len(reads))
    p1, s1 = pileup_reference(w1, su, [draft], ov, q1, f1, r1)
    p2, s2 = pileup_reference(w2, su, [draft], ov, q2, f2, r2, pile=p1)
    assert all((p2[f] == pile[f]).all() for f in PLANES) and {k: s1[k] + s2[k] for k in s1} == st
    # without indels: every walk on the other strand gives the same pile
    rng = np.random.default_rng(8)
    draft = ta.random_seq(rng, 500)
    reads = [ta.mutated(rng, draft[s:s + 120], 4, kinds=(0,)) for s in range(0, 380, 20)]
    fwd = one_walks([(0, 1, s, s + 120, 0) for s in range(0, 380, 20)])
    rev = one_walks([(1, 1, 500 - s - 120, 500 - s, 0) for s in range(0, 380, 20)])
    extra = dict(walk_off=np.arange(len(reads) + 1, dtype=np.uint64), qstart=np.zeros(len(reads), dtype=np.uint32), qend=np.full(len(reads), 120, dtype=np.uint32))
    fwd.update(extra)
    rev.update(extra)
    qf, ff, rf, _ = walk_inputs(fwd, su, [draft], ov, reads)
    qr, fr, rr, _ = walk_inputs(rev, su, [draft], ov, [tus.revcomp(r) for r in reads])
    pf, _ = pileup_reference(fwd, su, [draft], ov, qf, ff, rf)
    pr, _ = pileup_reference(rev, su, [draft], ov, qr, fr, rr)
    assert all((pf[f] == pr[f]).all() for f in PLANES) and int(sum(pf["sub%d" % c].astype(np.int64).sum() for c in range(4))) > 40


def test_clean_reads_vote_match_only_and_the_consensus_is_the_draft(repeat_walks):
    rw = repeat_walks
    for tag in ("before", "after"):
        k = rw[tag]
        walks = twk.reference_of(k)
        q, fl, runs, _ = walk_inputs(walks, k["paths"]["unitig"], k["strings"], k["overlap"], rw["reads"])
        pile, st = pileup_reference(walks, k["paths"]["unitig"], k["strings"], k["overlap"], q, fl, runs)
        assert all(not pile[f].any() for f in PLANES[1:]) and pile["match"].any() and st["walks_skipped"] == 0 and st["n_shifted"] == 0
        c = consensus_reference(pile, k["strings"], k["overlap"], 3)
        n = sum(len(s) for s in k["strings"])
        assert c["strings"] == list(k["strings"]) and c["pos_map"].tolist() == list(range(n + 1)), tag
        assert c["overlap"].tolist() == [min(int(o), len(k["strings"][i >> 1])) for i, o in enumerate(k["overlap"])], tag
        assert c["stats"]["n_sub"] == c["stats"]["n_del"] == c["stats"]["n_ins"] == c["stats"]["n_long"] == 0


REPEAT_SPACING = 24


def spoiled(strings, spacing=REPEAT_SPACING):
    """every string with a substitution at every spacing-th base: the lengths stay, so the walks stay valid"""
    out = []
    for s in strings:
        x = bytearray(s)
        for i in range(spacing // 2, len(x), spacing):
            x[i] = b"ACGT"[(b"ACGT".index(bytes([x[i]]).upper()) + 1) % 4]
        out.append(bytes(x))
    return out


def test_repeat_contigs_with_substitutions_are_polished_by_clean_reads(repeat_walks):
    rw = repeat_walks
    k = rw["after"]
    walks = twk.reference_of(k)
    draft = spoiled(k["strings"])
    q, fl, runs, _ = walk_inputs(walks, k["paths"]["unitig"], draft, k["overlap"], rw["reads"])
    assert not fl.any()
    pile, _ = pileup_reference(walks, k["paths"]["unitig"], draft, k["overlap"], q, fl, runs)
    c = consensus_reference(pile, draft, k["overlap"], 3)
    depth, off = depth_of(pile), draft_of(draft)[0].astype(np.int64)
    assert c["stats"]["n_ins"] == c["stats"]["n_del"] == 0 and c["stats"]["n_sub"] > 50
    for t, s in enumerate(k["strings"]):
        deep = depth[off[t]:off[t + 1]] >= 3
        got, want = np.frombuffer(c["strings"][t], dtype=np.uint8), np.frombuffer(s, dtype=np.uint8)
        assert len(got) == len(want) and (got[deep] == want[deep]).all() and deep.sum() > 0.9 * len(s), t
    print("repeat contigs, a substitution every %d bases: %d substituted back, %d positions below min_cov" % (REPEAT_SPACING, c["stats"]["n_sub"], c["stats"]["n_low"]))


@pytest.fixture(scope="module")
def ecoli_pile(ecoli_reference):
    e = ecoli_reference
    al = e["al"]
    q, fl, runs = [p[0] for p in al["pairs"]], al["flags"], [r[2] for r in al["res"]]
    pile, st = pileup_reference(e["walks"], e["paths"]["unitig"], e["strings"], e["overlap"], q, fl, runs)
    return {"pile": pile, "stats": st, "consensus": consensus_reference(pile, e["strings"], e["overlap"], 3)}


def test_ecoli_reads_with_errors_reference_stats(ecoli_reference, ecoli_pile):
    """the figures DESIGN.md §3.21 quotes; the device test below asserts device == reference"""
    st, c = ecoli_pile["stats"], ecoli_pile["consensus"]
    print("E. coli, 600 reads with errors: pile-up %s; consensus at min_cov 3 %s; %d bases -> %d" % (
        st, c["stats"], sum(len(s) for s in ecoli_reference["strings"]), len(c["out"])))
    assert st["walks_used"] + st["walks_skipped"] == ecoli_reference["walks"]["n_walks"]


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = 8
_dev, _host, _ptr = ts._dev, ts._host, ts._ptr
MARK32 = np.array(-0x5A5A).astype(np.int32).view(np.uint32)
JUNK = 0x5A5A0  # a slot behind a walk's runs: length 0x5A5A, code 0 -- never read


def device_pile(n_bases, pile=None):
    """eleven planes of n_bases counts (zeros, or a pile to add to), each with GUARD marked words behind it -> (tensors, s2k_pile)"""
    import torch

    planes, p = [], pkg.Pile()
    for f in PLANES:
        t = torch.full((n_bases + GUARD,), -0x5A5A, dtype=torch.int32, device="cuda:0")
        t[:n_bases] = 0 if pile is None else torch.from_numpy(pile[f].view(np.int32).copy()).to("cuda:0")
        planes.append(t)
    p.match, p.del_, p.ins_long = planes[0].data_ptr(), planes[1].data_ptr(), planes[10].data_ptr()
    for c in range(4):
        p.sub[c], p.ins[c] = planes[2 + c].data_ptr(), planes[6 + c].data_ptr()
    return planes, p


def alignment_arrays(flags, runs, slack=True):
    """the arrays s2k_align_pairs would leave: per walk its slots (more than its runs, junk behind them), n_ops, flags"""
    slots = [0 if fl else len(r) + (w % 3 if slack else 0) for w, (fl, r) in enumerate(zip(flags, runs))]
    off = np.concatenate([[0], np.cumsum(slots)]).astype(np.uint64)
    ops = np.full(int(off[-1]), JUNK, dtype=np.uint32)
    for w, r in enumerate(runs):
        if not flags[w]:
            ops[int(off[w]):int(off[w]) + len(r)] = [ln << 4 | op for ln, op in r]
    n_ops = np.array([0 if fl else len(r) for fl, r in zip(flags, runs)], dtype=np.uint32)
    return off, n_ops, ops


def query_pool(queries, seed=0):
    """the queries in one pool with junk between them -> (pool, q_begin)"""
    rng = np.random.default_rng(seed)
    buf, begin = bytearray(ta.random_seq(rng, 3, b"acgtn")), []
    for i, q in enumerate(queries):
        begin.append(len(buf))
        buf += q
        buf += ta.random_seq(rng, i % 4, b"acgtn")
    return np.frombuffer(bytes(buf), dtype=np.uint8), np.array(begin, dtype=np.uint64)


def pileup_args(P, n_walks, n_steps_all, n_bases, T, nq, n_ops_total, max_shift, pile, stats):
    """the arguments of s2k_walks_pileup behind the context, in the prototype's order (s2k_walks_pileup_ex takes four more); P: name ->
    device pointer"""
    return (n_walks, P("first_step"), P("n_steps"), P("path_start"), P("path_end"), P("flags"), P("unitig"), n_steps_all, P("out_off"), P("out"), n_bases,
            P("overlap"), T, P("query"), nq, P("q_begin"), P("aflags"), P("ops_off"), P("n_ops"), P("ops"), n_ops_total, max_shift, pile, stats)


def consensus_args(pile, d_off, d_out, n_bases, d_ov, T, min_cov, R, capacity, n_new, stats):
    """the arguments of s2k_pileup_consensus behind the context, in the prototype's order (s2k_pileup_consensus_ex takes three more); R:
    output name -> device pointer or None"""
    return (pile, d_off, d_out, n_bases, d_ov, T, min_cov, R("out_off"), R("out"), capacity, R("pos_map"), R("overlap"), n_new, stats)


def raw_pileup(eng, walks, su, strings, overlap, queries, flags, runs, max_shift=MAX_SHIFT, pile=None, ctx=True, null=(), stats=True, **over):
    """s2k_walks_pileup through ctypes, guards behind every plane -> (status, stats list, host planes with guards).  over: any input array
    replaced by name; n_walks, n_steps_all, T, n_bases, nq, n_ops_total given"""
    import torch

    out_off, out = draft_of(strings)
    pool, qb = query_pool(queries)
    ops_off, n_ops, ops = alignment_arrays(flags, runs)
    arr = {"first_step": (walks["first_step"], np.uint64), "n_steps": (walks["n_steps"], np.uint32), "path_start": (walks["path_start"], np.uint64),
           "path_end": (walks["path_end"], np.uint64), "flags": (walks["flags"], np.uint32), "unitig": (su, np.uint32), "out_off": (out_off, np.uint64),
           "out": (out, np.uint8), "overlap": (overlap, np.uint32), "query": (pool, np.uint8), "q_begin": (qb, np.uint64),
           "aflags": (np.asarray(flags), np.uint32), "ops_off": (ops_off, np.uint64), "n_ops": (n_ops, np.uint32), "ops": (ops, np.uint32)}
    dv = {k: _dev(over.get(k, a), dt) for k, (a, dt) in arr.items()}
    nw, ns = over.get("n_walks", len(walks["first_step"])), over.get("n_steps_all", len(su))
    T, nb = over.get("T", len(strings)), over.get("n_bases", len(out))
    planes, p = device_pile(len(out), pile)
    for f in null:
        if f in PLANES:
            i = PLANES.index(f)
            if i < 2 or i == 10:
                setattr(p, {0: "match", 1: "del_", 10: "ins_long"}[i], None)
            else:
                (p.sub if i < 6 else p.ins)[(i - 2) % 4] = None
    st = (ctypes.c_uint64 * pkg.PILEUP_STATS_WORDS)(*([777] * pkg.PILEUP_STATS_WORDS))
    P = lambda k: _ptr(dv[k], k in null)  # noqa: E731
    torch.cuda.synchronize()
    s = eng.lib.s2k_walks_pileup(eng.ctx if ctx else None, *pileup_args(P, nw, ns, nb, T, over.get("nq", len(pool)), over.get("n_ops_total", len(ops)), max_shift,
                                                                        None if "pile" in null else ctypes.byref(p), st if stats else None))
    torch.cuda.synchronize()
    return s, list(st), {f: _host(t, np.uint32) for f, t in zip(PLANES, planes)}


def assert_pile(got, ref, n, tag):
    for f in PLANES:
        if got[f][:n].tobytes() != ref[f].tobytes():
            x = np.nonzero(got[f][:n] != ref[f])[0]
            raise AssertionError((tag, f, "differs at", x[:8].tolist(), "device", got[f][x[:8]].tolist(), "reference", ref[f][x[:8]].tolist()))
        assert (got[f][n:] == MARK32).all(), (tag, f, "guard")


def device_pileup(eng, walks, su, strings, overlap, queries, flags, runs, tag, max_shift=MAX_SHIFT, pile=None):
    ref, rst = pileup_reference(walks, su, strings, overlap, queries, flags, runs, max_shift, pile)
    s, st, got = raw_pileup(eng, walks, su, strings, overlap, queries, flags, runs, max_shift, pile)
    assert s == 0, (tag, s, eng.lib.s2k_last_error(eng.ctx))
    assert_pile(got, ref, sum(len(x) for x in strings), tag)
    assert st[:len(P_STATS)] == [rst[f] for f in P_STATS] and st[len(P_STATS):] == [0] * (len(st) - len(P_STATS)), (tag, st, rst)
    return ref, rst


def aligned_case(walks, su, strings, overlap, rng, n_edits=3, alphabet=b"ACGT", max_edits=ta.MAX_EDITS):
    """every walk's target mutated and aligned to it by test_align.align_reference -> (queries, flags, runs)"""
    targets, bad = targets_of(walks, su, strings, overlap)
    queries, flags, runs = [], [], []
    for t, b in zip(targets, bad):
        q = b"" if b else ta.mutated(rng, t, int(rng.integers(0, n_edits + 1)), alphabet)
        res = ta.align_reference(q, t, max_edits)
        queries.append(q)
        flags.append(2 if b else res[1])
        runs.append(res[2])
    return queries, np.array(flags, dtype=np.uint32), runs


@pytest.mark.gpu
def test_device_pileup_runs_round_a_junction(eng):
    seen = set()
    for tag, *c in junction_cases():
        for ms in (0, MAX_SHIFT):
            ref, st = device_pileup(eng, *c[:5], [0], c[5], (tag, ms), max_shift=ms)
            seen.add((tag.split()[1], st["n_end_ins"], int(ref["del"].sum()) > 0))
    assert ("I", 1, False) in seen and ("D", 0, True) in seen
    walks, su, strings, overlap, q, runs = junction_cases()[0][1:]
    cases = junction_cases()  # and all of them in one call: one pile
    many = one_walks([tuple(int(c[1][f][0]) for f in REC) for c in cases])
    device_pileup(eng, many, su, strings, overlap, [c[5][0] for c in cases], [0] * len(cases), [c[6][0] for c in cases], "all")


@pytest.mark.gpu
def test_device_pileup_hand_graph_walks(eng):
    """the walks of test_align.hand_targets: twin strands, a hairpin, a circular unitig walked three times round and its twin"""
    walks, paths, strings, mo = ta.hand_targets()
    rng = np.random.default_rng(92)
    for n_edits in (0, 6):
        q, fl, runs = aligned_case(walks, paths["unitig"], strings, mo["overlap"], rng, n_edits)
        assert not fl.any()
        for ms in (0, MAX_SHIFT):
            ref, st = device_pileup(eng, walks, paths["unitig"], strings, mo["overlap"], q, fl, runs, ("hand", n_edits, ms), max_shift=ms)
        assert st["walks_used"] == walks["n_walks"] and int(ref["match"].max()) >= 3  # the circular unitig, round after round
    for w in range(walks["n_walks"]):  # every walk alone
        one = {f: walks[f][w:w + 1] for f in REC}
        device_pileup(eng, one, paths["unitig"], strings, mo["overlap"], q[w:w + 1], fl[w:w + 1], runs[w:w + 1], ("hand", w))
    none = {f: walks[f][:0] for f in REC}
    s, st, got = raw_pileup(eng, none, paths["unitig"], strings, mo["overlap"], [], [], [])
    assert s == 0 and st == [0] * 8 and all(not got[f][:-GUARD].any() for f in PLANES)


def _single(strings, specs, cigars, rng, su=(0, 1), overlap=None, alphabet=b"ACGT", queries=None):
    """walks given by their records and their CIGARs -> the arguments of device_pileup"""
    su = np.array(su, dtype=np.uint32)
    overlap = np.zeros(2 * len(strings), dtype=np.uint32) if overlap is None else overlap
    walks = one_walks(specs)
    targets, bad = targets_of(walks, su, strings, overlap)
    runs = [runs_of(c) for c in cigars]
    q = queries or [query_of(rng, t, r, alphabet) for t, r in zip(targets, runs)]
    return walks, su, strings, overlap, q, [0] * len(specs), runs


@pytest.mark.gpu
def test_device_pileup_ends_empty_targets_rounds_and_other_bytes(eng):
    rng = np.random.default_rng(93)
    s = [ta.random_seq(rng, 50)]
    # I at the target's start and end, on both strands, inside the unitig and on its ends
    specs = [(0, 1, 5, 45, 0), (1, 1, 5, 45, 0), (0, 1, 0, 50, 0), (1, 1, 0, 50, 0)]
    c = _single(s, specs, ["2I40=1I", "1I40=2I", "1I50=1I", "1I50=1I"], rng)
    ref, st = device_pileup(eng, *c, "I at the ends")
    assert st["n_end_ins"] == 2 and int(sum(ref[f].sum() for f in PLANES[6:])) == 6
    # an empty target: its I run is dropped, a walk without a run votes nothing
    c = _single(s, [(0, 1, 7, 7, 0), (1, 1, 9, 9, 0), (0, 1, 3, 9, 0)], ["3I", "", "6="], rng)
    ref, st = device_pileup(eng, *c, "empty targets")
    assert st["n_empty_ins"] == 1 and st["walks_used"] == 3 and int(ref["match"].sum()) == 6
    # a circular unitig walked round more than once: runs that end before, on and behind a round's end
    L = 50
    for U in (0, 1):
        for kind in "=XDI":
            for delta in (-1, 0, 1):
                pre = 2 * L - 7 + delta - (3 if kind != "I" else 0)
                rest = 3 * L - pre - (3 if kind != "I" else 0)
                mid = "1X" if kind == "=" else ""
                cig = "%d=%s3%s%s%d=" % (pre - len(mid) // 2, mid, kind, mid, rest - len(mid) // 2)
                c = _single(s, [(U, 1, 7, 7 + 3 * L, 1)], [cig], rng)
                ref, st = device_pileup(eng, *c, ("round", U, kind, delta))
                assert int(ref["match"].max()) == 3
    # bytes without a code and lower-case bytes in the query: X casts no vote for N (n_other), a single n goes to ins_long, c to ins1
    tgt = s[0][10:40]
    q = tgt[:5] + b"N" + tgt[6:10] + b"n" + tgt[10:15] + (b"a" if tgt[15:16] != b"A" else b"c") + tgt[16:20] + b"c" + tgt[20:]
    c = _single(s, [(0, 1, 10, 40, 0)], ["5=1X4=1I5=1X4=1I10="], rng, queries=[q])
    ref, st = device_pileup(eng, *c, "other bytes", max_shift=0)
    assert st["n_other"] == 1 and int(ref["ins_long"].sum()) == 1 and int(ref["ins1"].sum()) == 1 and int(sum(ref["sub%d" % k].sum() for k in range(4))) == 1
    lower = [s[0].lower()]  # a lower-case draft: = compares bytes as they are, so the reads are lower-case too
    device_pileup(eng, *_single(lower, specs[:2], ["20=2D18=", "18=1I22="], rng, alphabet=b"acgt"), "lower case")


def homopolymer(rng, h, left=80, right=30):
    """`left` bases, then h + 1 times the same letter, then `right` bases; the letters next to the run differ from it"""
    a = bytearray(ta.random_seq(rng, left)) + b"A" * (h + 1) + bytearray(ta.random_seq(rng, right))
    a[left - 1] = ord("C")
    a[left + h + 1] = ord("G")
    return bytes(a)


@pytest.mark.gpu
@pytest.mark.parametrize("h", [0, 1, 63, 64, 65])
def test_device_pileup_shifts_along_homopolymers(eng, h):
    """a deleted or inserted A at the right end of h + 1 A: the gap moves h to the left, at most max_shift, on both strands (on the twin
    strand the aligner leaves it at the other end, where it already is leftmost)"""
    rng = np.random.default_rng(94 + h)
    s = [homopolymer(rng, h)]
    n, a = len(s[0]), 80  # the run is [a, a + h + 1)
    for ms in (MAX_SHIFT, 0, 5):
        want = min(h, ms)
        # forward strand: the gap at the run's right end; twin strand: the same forward gap is at the run's start on the walk
        cigs = ["%d=1D%d=" % (a + h, n - a - h - 1), "%d=1D%d=" % (n - a - h - 1, a + h)]
        c = _single(s, [(0, 1, 0, n, 0), (1, 1, 0, n, 0)], cigs, rng)
        ref, st = device_pileup(eng, *c, ("D", h, ms), max_shift=ms)
        assert np.nonzero(ref["del"])[0].tolist() == [a + h - want] and ref["del"][a + h - want] == 2 and st["n_shifted"] == (2 if want else 0)
        assert (ref["match"][:a + h - want] == 2).all() and (ref["match"][a + h - want + 1:] == 2).all() and ref["match"][a + h - want] == 0
        cigs = ["%d=1I%d=" % (a + h + 1, n - a - h - 1), "%d=1I%d=" % (n - a - h - 1, a + h + 1)]
        q = [s[0][:a + h + 1] + b"A" + s[0][a + h + 1:]]
        c = _single(s, [(0, 1, 0, n, 0), (1, 1, 0, n, 0)], cigs, rng, queries=q + [tus.revcomp(q[0])])
        ref, st = device_pileup(eng, *c, ("I", h, ms), max_shift=ms)
        assert np.nonzero(ref["ins0"])[0].tolist() == [a + h + 1 - min(h + 1, ms)] and int(ref["ins0"].sum()) == 2 and (ref["match"] == 2).all()


@pytest.mark.gpu
def test_device_pileup_shifts_stopped_by_a_piece_and_by_a_step(eng):
    rng = np.random.default_rng(95)
    s = [homopolymer(rng, 20)]
    n = len(s[0])
    # the = run before the gap is 6 long (an X before it): the shift stops at 6 although 20 letters agree
    q0 = bytearray(s[0][:100] + s[0][101:])
    q0[93] = ord("C")
    c = _single(s, [(0, 1, 0, n, 0)], ["93=1X6=1D%d=" % (n - 101)], rng, queries=[bytes(q0)])
    ref, st = device_pileup(eng, *c, "stopped by the piece")
    assert np.nonzero(ref["del"])[0].tolist() == [94] and st["n_shifted"] == 1
    # two unitigs whose junction lies inside a homopolymer: the gap stays in its step
    a = ta.random_seq(rng, 30) + b"C" + b"A" * 12
    b = b"A" * 12 + b"G" + ta.random_seq(rng, 20)  # the overlap is 4: the path reads 20 A
    strings, overlap = [a, b], np.array([4, 0, 0, 4], dtype=np.uint32)
    path = twk.stitched_path(strings, overlap, [0, 2])
    assert len(path) == 43 + 33 - 4 and path[31:51] == b"A" * 20
    # the deleted A is byte 50, in step 1 (bytes 43 on): it moves left to byte 43, the step's first, not further
    c = _single(strings, [(0, 2, 0, len(path), 0), (2, 2, 0, len(path), 0)], ["50=1D%d=" % (len(path) - 51), "%d=1D50=" % (len(path) - 51)], rng, su=(0, 2, 3, 1),
                overlap=overlap)
    ref, st = device_pileup(eng, *c, "stopped by the step")
    # forward strand: byte 43 is position 4 of unitig 1 = draft 43 + 4, the first that step 1 owns (the overlap's four belong to step 0).
    # Twin strand: the walk starts in unitig 1, whose step owns all of it: the same gap moves on to the unitig's first base
    assert np.nonzero(ref["del"])[0].tolist() == [43, 47] and st["n_shifted"] == 2
    ref0, st0 = device_pileup(eng, *c, "not shifted", max_shift=0)
    assert np.nonzero(ref0["del"])[0].tolist() == [54] and ref0["del"][54] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("n_walks", [1, 63, 64, 65, 2 * 2048 + 1])
def test_device_pileup_walk_counts(eng, n_walks):
    rng = np.random.default_rng(960 + n_walks)
    strings = [ta.random_seq(rng, 300), ta.random_seq(rng, 41)]
    specs = []
    for _ in range(n_walks):
        U, a = int(rng.integers(0, 4)), 0
        L = len(strings[U >> 1])
        a = int(rng.integers(0, L - 10))
        specs.append((U, 1, a, a + int(rng.integers(0, min(60, L - a))), 0))
    walks = one_walks(specs)
    su = np.arange(4, dtype=np.uint32)
    q, fl, runs = aligned_case(walks, su, strings, np.zeros(4, dtype=np.uint32), rng, 3)
    device_pileup(eng, walks, su, strings, np.zeros(4, dtype=np.uint32), q, fl, runs, ("walks", n_walks))


@pytest.mark.gpu
def test_device_pileup_many_runs_and_a_long_walk(eng):
    rng = np.random.default_rng(97)
    s = [ta.random_seq(rng, 21000)]
    q, t = ta.spaced(rng, 255, 0, gap=9)  # 255 substitutions 9 apart: 511 runs
    s1 = [t + b"ACGT"]
    runs = ta.align_reference(q, t)[2]
    assert len(runs) == 511
    for U in (0, 1):
        spec = (U, 1, 0, len(t), 0) if U == 0 else (1, 1, 4, 4 + len(t), 0)
        qq, rr = (q, runs) if U == 0 else (tus.revcomp(q), ta.align_reference(tus.revcomp(q), tus.revcomp(t))[2])
        walks = one_walks([spec])
        device_pileup(eng, walks, np.array([0, 1], dtype=np.uint32), s1, np.zeros(2, dtype=np.uint32), [qq], [0], [rr], ("511 runs", U))
    walks = one_walks([(0, 1, 500, 20500, 0), (1, 1, 400, 20400, 0)])
    su = np.array([0, 1], dtype=np.uint32)
    q, fl, runs = aligned_case(walks, su, s, np.zeros(2, dtype=np.uint32), rng, 150)
    ref, st = device_pileup(eng, walks, su, s, np.zeros(2, dtype=np.uint32), q, fl, runs, "20 000 bases")
    assert not fl.any() and int(depth_of(ref).max()) == 2


@pytest.mark.gpu
def test_device_pileup_flagged_walks_are_skipped(eng):
    walks, paths, strings, mo = ta.hand_targets()
    rng = np.random.default_rng(98)
    q, fl, runs = aligned_case(walks, paths["unitig"], strings, mo["overlap"], rng, 4)
    fl = fl.copy()
    fl[1::3] = 1
    fl[2::5] = 2
    ref, st = device_pileup(eng, walks, paths["unitig"], strings, mo["overlap"], q, fl, runs, "flagged")
    assert st["walks_skipped"] == int((fl != 0).sum()) > 3 and st["walks_used"] == int((fl == 0).sum()) > 3
    keep = np.nonzero(fl == 0)[0]
    only = {f: walks[f][keep] for f in REC}
    alone, _ = pileup_reference(only, paths["unitig"], strings, mo["overlap"], [q[i] for i in keep], [0] * len(keep), [runs[i] for i in keep])
    assert all((alone[f] == ref[f]).all() for f in PLANES)


def cursor_case():
    """three unitigs by hand -- 0 walked on its twin strand, 1 whose nine bases are both the overlap that enters it and the one that
    leaves it (its step gives the path no byte), 2 walked round as a circular one -- and 65 walks, one past a wave, one of them bad
    -> (walks, su, strings, overlap)"""
    rng = np.random.default_rng(102)
    b = ta.random_seq(rng, 9)
    strings = [tus.revcomp(ta.random_seq(rng, 28) + b), b, b + ta.random_seq(rng, 14)]  # the path of steps 0 .. 2: 28 + 9 + 14 = 51 bytes
    overlap = np.array([0, 9, 9, 0, 0, 0], dtype=np.uint32)
    su = np.array([1, 2, 4, 4, 5], dtype=np.uint32)  # steps 0 .. 2: 0- 1+ 2+; step 3: 2+ and step 4: 2-, each walked round
    specs = [(1, 2, 3, 17, 0),                 # two steps: from inside unitig 1 to inside unitig 2
             (0, 3, 5, 48, 0),                 # through step 1, which adds no byte
             (3, 1, 4, 4 + 2 * 23 + 7, 1),     # two rounds and a part
             (4, 1, 11, 11 + 2 * 23 + 5, 1)]   # and on the twin strand
    while len(specs) < 65:
        if len(specs) == 40:
            specs.append((0, 3, 0, 52, 0))     # the bad one: it ends behind the path
            continue
        first, n, total, circ = ((0, 3, 51, 0), (1, 2, 23, 0), (3, 1, 23, 1), (4, 1, 23, 1))[len(specs) % 4]
        ps = int(rng.integers(0, total))
        specs.append((first, n, ps, ps + int(rng.integers(1, 70)) if circ else int(rng.integers(ps + 1, total + 1)), circ))
    return one_walks(specs), su, strings, overlap


def device_cursor(eng):
    """s2k_walks_targets and s2k_walks_pileup find the step of a path byte alike: byte x of a target is the draft's byte at the forward
    position walk_sources gives x (its complement on an odd unitig), and a walk that matches its whole target votes there once"""
    walks, su, strings, overlap = cursor_case()
    off, out = draft_of(strings)
    u, nw = [int(x) for x in su], len(walks["first_step"])
    src = [walk_sources(walks, w, u, strings, overlap, off) for w in range(nw)]
    lens = [len(s[1]) for s in src]
    bad = [w for w in range(nw) if not lens[w]]
    assert nw == 65 and bad == [40] and set(src[1][0].tolist()) == {0, 2} and len(set(src[2][0].tolist())) == 3
    s, nb, got = ta.raw_targets(eng, walks, su, strings, overlap, capacity=sum(lens))
    assert (s, nb) == (0, sum(lens)), (s, nb, eng.lib.s2k_last_error(eng.ctx))
    toff = np.concatenate([[0], np.cumsum(lens)])
    assert got["tgt_off"][:nw + 1].tolist() == toff.tolist() and got["bad"][:nw].tolist() == [int(w in bad) for w in range(nw)]
    want = np.zeros(len(out), dtype=np.int64)
    queries = []
    for w, (seg, pos, odd, end) in enumerate(src):
        t = got["tgt"][toff[w]:toff[w + 1]]
        assert t.tobytes() == np.where(odd == 1, _COMP[out[pos]], out[pos]).astype(np.uint8).tobytes(), ("walk", w)
        want += np.bincount(pos, minlength=len(out))
        queries.append(t.tobytes())
    flags = [2 * int(w in bad) for w in range(nw)]
    s, st, pile = raw_pileup(eng, walks, su, strings, overlap, queries, flags, [[] if w in bad else [(lens[w], EQ)] for w in range(nw)])
    assert s == 0, (s, eng.lib.s2k_last_error(eng.ctx))
    assert_pile(pile, {**new_pile(len(out)), "match": want.astype(np.uint32)}, len(out), "cursor")
    assert st[:2] == [64, 1] and st[2:] == [0] * (len(st) - 2), st


@pytest.mark.gpu
def test_device_targets_and_pileup_share_the_step_cursor(eng):
    device_cursor(eng)


@pytest.mark.gpu
def test_device_pileup_random_decompositions(eng):
    """random node records give junctions above a length (bad walks, flagged) among sound ones, circular unitigs walked round, both
    strands, steps that add no byte"""
    rng = np.random.default_rng(99)
    case = twk.walked_case(rng, 300, list(rng.integers(0, 60, size=80)))
    walks = twk.reference_of(case)
    strings = ta.random_strings(np.random.default_rng(100), case["mo"])
    su, ov = case["paths"]["unitig"], case["mo"]["overlap"]
    q, fl, runs = aligned_case(walks, su, strings, ov, rng, 5)
    for ms in (0, MAX_SHIFT):
        ref, st = device_pileup(eng, walks, su, strings, ov, q, fl, runs, ("walked", ms), max_shift=ms)
    assert walks["flags"].any() and int(walks["n_steps"].max()) > 1 and st["walks_skipped"] == int((fl != 0).sum()) and st["n_shifted"] > 20
    print("random decomposition: %d walks, %d skipped, depth up to %d, %s" % (len(fl), st["walks_skipped"], int(depth_of(ref).max()), st))
    case = twk.chained_case(rng, 40, list(rng.integers(1, 9, size=90)), p_break=0.1)
    walks = twk.reference_of(case)
    strings = ta.random_strings(np.random.default_rng(101), case["mo"])
    su, ov = case["paths"]["unitig"], case["mo"]["overlap"]
    q, fl, runs = aligned_case(walks, su, strings, ov, rng, 5, alphabet=b"AC")
    device_pileup(eng, walks, su, strings, ov, q, fl, runs, "chained")


@pytest.mark.gpu
def test_device_pileup_two_adds_equal_one_and_two_calls_are_identical(eng):
    clean, draft, walks, reads, _ = planted_case(3, b"AACGAA")
    su, ov = np.array([0, 1], dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    q, fl, runs, _ = walk_inputs(walks, su, [draft], ov, reads)
    rec = {f: walks[f] for f in REC}
    ref, _ = device_pileup(eng, rec, su, [draft], ov, q, fl, runs, "one add")
    s, st, again = raw_pileup(eng, rec, su, [draft], ov, q, fl, runs)
    assert s == 0 and all(again[f].tobytes() == ref[f].tobytes() + MARK32.tobytes() * GUARD for f in PLANES)
    h = len(reads) // 3
    first = {f: walks[f][:h] for f in REC}
    rest = {f: walks[f][h:] for f in REC}
    p1, _ = device_pileup(eng, first, su, [draft], ov, q[:h], fl[:h], runs[:h], "first batch")
    p2, _ = device_pileup(eng, rest, su, [draft], ov, q[h:], fl[h:], runs[h:], "second batch", pile=p1)
    assert all((p2[f] == ref[f]).all() for f in PLANES)
    c = consensus_reference(ref, [draft], ov, 3)
    assert c["strings"][0] == clean


@pytest.mark.gpu
def test_device_pileup_refusals_nothing_written(eng):
    walks, paths, strings, mo = ta.hand_targets()
    su, ov = paths["unitig"], mo["overlap"]
    rng = np.random.default_rng(102)
    q, fl, runs = aligned_case(walks, su, strings, ov, rng, 4)
    base = {f: walks[f] for f in REC}
    device_pileup(eng, base, su, strings, ov, q, fl, runs, "base")
    n = sum(len(s) for s in strings)
    ops_off, n_ops, ops = alignment_arrays(fl, runs)

    def refused(code=1, **kw):
        s, st, got = raw_pileup(eng, base, su, strings, ov, q, fl, runs, **kw)
        assert s == code and st == [0] * 8, (s, st, list(kw))
        for f in PLANES:
            assert not got[f][:n].any() and (got[f][n:] == MARK32).all(), (f, list(kw))

    def changed(name, i, v, src):
        x = np.array(src).copy()
        x[i] = v
        return {name: x}

    refused(ctx=False)
    s, st, got = raw_pileup(eng, base, su, strings, ov, q, fl, runs, stats=False)
    assert s == 1 and all(not got[f][:n].any() for f in PLANES)
    for f in REC + ("unitig", "out_off", "out", "overlap", "query", "q_begin", "aflags", "ops_off", "n_ops", "ops", "pile", "match", "del", "sub2", "ins3", "ins_long"):
        refused(null=(f,))
    refused(max_shift=MAX_SHIFT + 1)
    refused(n_walks=2 ** 32)
    refused(**changed("first_step", 3, len(su), walks["first_step"]))  # the checks of s2k_walks_targets
    refused(**changed("unitig", 4, 2 * len(strings), su))
    refused(T=len(strings) - 1)
    refused(n_bases=n - 1)
    refused(**changed("ops_off", 2, int(ops_off[3]) + 1, ops_off))  # ops_off decreases
    refused(n_ops_total=len(ops) - 1)  # the slots pass the runs given
    refused(**changed("n_ops", 4, int(ops_off[5] - ops_off[4]) + 1, n_ops))  # more runs than slots
    w = next(i for i in range(len(runs)) if len(runs[i]) >= 3)
    o = int(ops_off[w])
    refused(**changed("ops", o, (int(ops[o]) >> 4) << 4 | 3, ops))  # an unknown code
    refused(**changed("ops", o + 1, int(ops[o + 1]) & 15, ops))  # a run of length 0
    refused(**changed("ops", o, int(ops[o]) + 16, ops))  # the runs pass the target
    refused(**changed("path_end", w, int(walks["path_end"][w]) - 1, walks["path_end"]))  # the target is shorter than the runs
    pool, qb = query_pool(q)
    refused(nq=int(qb[-1]) + len(q[-1]) - 1)  # the pool ends inside the last query
    refused(**changed("q_begin", 0, 2 ** 40, qb))
    flagged = fl.copy()
    flagged[w] = 1  # a flagged walk's slots are not looked at
    s, st, got = raw_pileup(eng, base, su, strings, ov, q, fl, runs, aflags=flagged, **changed("ops", o, 3, ops))
    assert s == 0 and st[1] == 1


C_OUT = {"out_off": np.uint64, "out": np.uint8, "pos_map": np.uint64, "overlap": np.uint32}
C_FILL = {np.uint64: -0x5A5A, np.uint32: -0x5A5A, np.uint8: 0xA5}
C_T = {np.uint64: "int64", np.uint32: "int32", np.uint8: "uint8"}


def _cmarked(h, frm=0):
    dt = h.dtype.type
    return bool((h[frm:] == np.array(C_FILL[dt]).astype({np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dt]).view(dt)).all())


def raw_consensus(eng, pile, strings, overlap, min_cov=3, capacity=None, want=("out_off", "out", "pos_map", "overlap"), ctx=True, null=(), stats=True, **over):
    """s2k_pileup_consensus through ctypes, guards behind every output -> (status, n_new_bases, stats, host arrays with guards, planes)"""
    import torch

    out_off, out = draft_of(strings)
    n, T = len(out), len(strings)
    planes, p = device_pile(n, pile)
    before = [t.clone() for t in planes]
    d_off, d_out, d_ov = _dev(over.get("out_off", out_off), np.uint64), _dev(out, np.uint8), _dev(overlap, np.uint32)
    cap = int(capacity if capacity is not None else 0)
    size = {"out_off": T + 1, "out": max(cap, 1) + 15, "pos_map": n + 1, "overlap": max(2 * T, 1)}
    res = {f: torch.full((size[f] + GUARD,), C_FILL[C_OUT[f]], dtype=getattr(torch, C_T[C_OUT[f]]), device="cuda:0") for f in want}
    nn = ctypes.c_uint64(777)
    st = (ctypes.c_uint64 * pkg.CONSENSUS_STATS_WORDS)(*([777] * pkg.CONSENSUS_STATS_WORDS))
    R = lambda f: _ptr(res[f]) if f in res else None  # noqa: E731
    torch.cuda.synchronize()
    s = eng.lib.s2k_pileup_consensus(eng.ctx if ctx else None, *consensus_args(None if "pile" in null else ctypes.byref(p), _ptr(d_off, "out_off" in null),
                                                                               _ptr(d_out, "out" in null), over.get("n_bases", n), _ptr(d_ov, "overlap" in null),
                                                                               over.get("T", T), min_cov, R, cap, ctypes.byref(nn), st if stats else None))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, planes)), "the pile is only read"
    return s, nn.value, list(st), {f: _host(x, C_OUT[f]) for f, x in res.items()}


def device_consensus(eng, pile, strings, overlap, min_cov, tag):
    ref = consensus_reference(pile, strings, overlap, min_cov)
    m, T, n = len(ref["out"]), len(strings), sum(len(s) for s in strings)
    want_st = [ref["stats"][f] for f in C_STATS] + [0] * 3
    s, nn, st, got = raw_consensus(eng, pile, strings, overlap, min_cov, want=())
    assert (s, nn, st) == (0, m, want_st), (tag, "sizes", s, nn, m, st, want_st)
    s, nn, st, got = raw_consensus(eng, pile, strings, overlap, min_cov, want=("out_off", "pos_map", "overlap"))
    assert (s, nn) == (0, m), (tag, "sizes with outputs")
    sizes = {"out_off": T + 1, "out": m, "pos_map": n + 1, "overlap": 2 * T}
    for f in got:
        assert got[f][:sizes[f]].tobytes() == ref[f].tobytes() and _cmarked(got[f], max(sizes[f], 1) if f == "overlap" else sizes[f]), (tag, "sizes", f)
    s, nn, st, got = raw_consensus(eng, pile, strings, overlap, min_cov, capacity=m)
    assert (s, nn, st) == (0, m, want_st), (tag, s, nn, m, st, want_st)
    for f in got:
        if got[f][:sizes[f]].tobytes() != ref[f].tobytes():
            x = np.nonzero(got[f][:sizes[f]] != ref[f])[0]
            raise AssertionError((tag, f, "differs at", x[:8].tolist(), got[f][x[:8]].tolist(), ref[f][x[:8]].tolist()))
        assert _cmarked(got[f], max(sizes[f], 1) if f == "overlap" else sizes[f]), (tag, f, "guard")
    if m:
        s, nn, st, got = raw_consensus(eng, pile, strings, overlap, min_cov, capacity=m - 1)
        assert (s, nn, st) == (7, m, [0] * 8) and all(_cmarked(x) for x in got.values()), (tag, "capacity")
    return ref


def random_pile(rng, strings, p_event=0.08, depth=8):
    """a pile in which most positions are plain matches and some carry a winning or a tying substitution, deletion or insertion"""
    off, out = draft_of(strings)
    n = len(out)
    pile = new_pile(n)
    pile["match"][:] = rng.integers(0, depth, size=n)
    ev = rng.random(n) < p_event
    for f in PLANES[1:]:
        pile[f][:] = np.where(ev & (rng.random(n) < 0.3), rng.integers(0, depth, size=n), 0)
    return pile


@pytest.mark.gpu
def test_device_consensus_unitig_lengths_and_random_piles(eng):
    rng = np.random.default_rng(103)
    lens = [0, 1, 15, 16, 17, 0, 4095, 4096, 4097, 3]
    strings = [ta.random_seq(rng, n, b"ACGTacgtN") for n in lens]
    overlap = np.array([int(rng.integers(0, n + 3)) for n in lens for _ in (0, 1)], dtype=np.uint32)  # some above the length
    seen = dict.fromkeys(C_STATS, 0)
    for min_cov in (0, 3, 6):
        pile = random_pile(rng, strings)
        ref = device_consensus(eng, pile, strings, overlap, min_cov, ("lengths", min_cov))
        for f in C_STATS:
            seen[f] += ref["stats"][f]
        assert len(ref["strings"][0]) == 0 and ref["pos_map"][-1] == len(ref["out"])
    assert all(seen[f] > 20 for f in C_STATS), seen
    for one in ([b""], [b"A"], []):
        device_consensus(eng, new_pile(len(b"".join(one))), one, np.zeros(2 * len(one), dtype=np.uint32), 3, one)


@pytest.mark.gpu
def test_device_consensus_ends_low_coverage_and_both_orientations(eng):
    a, b, c = b"ACGTACGTAC", b"GGGGCCCCTT", b"TTTTTTAAAAAA"
    strings = [a, b, c]
    n = 32
    pile = new_pile(n)
    # unitig 0: its first base deleted, an A inserted before its second, its last base deleted, a T inserted before its last
    pile["match"][:10] = 5
    for p in (0, 9):
        pile["match"][p], pile["del"][p] = 1, 4
    pile["ins0"][1], pile["ins3"][9] = 3, 4
    # unitig 1: wholly below min_cov, whatever its planes say
    pile["match"][10:20], pile["sub0"][10:20], pile["ins1"][10:20] = 0, 2, 2
    # unitig 2: wholly rewritten: every base substituted by C, and a G inserted before each
    pile["sub1"][20:32], pile["match"][20:32], pile["ins2"][20:32], pile["ins_long"][25] = 6, 1, 4, 9
    overlap = np.array([3, 2, 4, 4, 5, 12], dtype=np.uint32)
    ref = device_consensus(eng, pile, strings, overlap, 3, "ends")
    assert ref["strings"][0] == b"A" + b"CGTACGTA" + b"T" and ref["strings"][1] == b and ref["strings"][2] == b"GC" * 12
    assert ref["stats"] == {"n_low": 10, "n_sub": 12, "n_del": 2, "n_ins": 14, "n_long": 1}
    # the overlaps: 0+ leaves by its last 3 old bases (A, the inserted T; C is deleted): 3; 0- by its first 2 (A deleted, then A C): pm(2) = 2
    assert ref["overlap"].tolist() == [3, 2, 4, 4, 10, 24] and ref["pos_map"][:3].tolist() == [0, 0, 2]
    twin = [pkg.revcomp(s) for s in strings]  # the draft on the other strand with the mirrored pile: the polished strings mirror too
    mirror = new_pile(n)
    off = draft_of(strings)[0].astype(np.int64)
    for t in range(3):
        lo, hi = off[t], off[t + 1]
        for f in ("match", "del"):
            mirror[f][lo:hi] = pile[f][lo:hi][::-1]
        for k in range(4):
            mirror["sub%d" % (3 - k)][lo:hi] = pile["sub%d" % k][lo:hi][::-1]
    got = device_consensus(eng, mirror, twin, overlap, 3, "mirrored")
    plain = consensus_reference({f: (pile[f] if not f.startswith("ins") else np.zeros(n, dtype=np.uint32)) for f in PLANES}, strings, overlap, 3)
    assert [pkg.revcomp(s) for s in got["strings"]] == plain["strings"]


@pytest.mark.gpu
def test_device_consensus_refusals_nothing_written(eng):
    rng = np.random.default_rng(104)
    strings = [ta.random_seq(rng, n) for n in (40, 0, 25)]
    overlap = np.array([5, 5, 0, 0, 7, 3], dtype=np.uint32)
    pile = random_pile(rng, strings)
    ref = device_consensus(eng, pile, strings, overlap, 2, "base")
    m = len(ref["out"])

    def refused(code=1, n_out=0, **kw):
        kw.setdefault("capacity", m)
        s, nn, st, got = raw_consensus(eng, pile, strings, overlap, 2, **kw)
        assert (s, nn) == (code, n_out) and st == [0] * 8 and all(_cmarked(x) for x in got.values()), (s, nn, st, list(kw))

    refused(ctx=False)
    for f in ("pile", "out_off", "out", "overlap"):
        refused(null=(f,))
    s, nn, st, got = raw_consensus(eng, pile, strings, overlap, 2, capacity=m, stats=False)
    assert (s, nn) == (1, 0) and all(_cmarked(x) for x in got.values())
    off = draft_of(strings)[0]
    bad = off.copy()
    bad[1] = off[2] + 1
    refused(out_off=bad)  # out_off decreases
    refused(n_bases=int(off[-1]) - 1)
    refused(T=2 ** 31)
    refused(code=7, n_out=m, capacity=m - 1)
    import torch

    planes, p = device_pile(len(b"".join(strings)), pile)  # d_new_out not 16-byte aligned
    d_off, d_out, d_ov = _dev(off, np.uint64), _dev(draft_of(strings)[1], np.uint8), _dev(overlap, np.uint32)
    buf = torch.full((m + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    nn, st = ctypes.c_uint64(5), (ctypes.c_uint64 * 8)()
    s = eng.lib.s2k_pileup_consensus(eng.ctx, ctypes.byref(p), _ptr(d_off), _ptr(d_out), len(b"".join(strings)), _ptr(d_ov), 3, 2, None,
                                     ctypes.c_void_p(buf.data_ptr() + 8), m, None, None, ctypes.byref(nn), st)
    assert s == 1 and nn.value == 0 and bool((buf == 0xA5).all())


def _device_pile_reference(pl, walks, graph, seqs, reads, al):
    """the references over what the device holds: its walks, its draft, its alignments"""
    h, a = walks.host(), al.host()
    strings = tus.unitig_strings(None, {"out_off": tg._u64(seqs[0]), "out": seqs[1].cpu().numpy()})
    overlap = graph.overlap.cpu().numpy().view(np.uint32)
    wo = h["walk_off"].astype(np.int64)
    queries, runs = [], []
    for r in range(len(wo) - 1):
        for w in range(wo[r], wo[r + 1]):
            rr = [(int(x) >> 4, int(x) & 15) for x in a["ops"][int(a["ops_off"][w]):int(a["ops_off"][w]) + int(a["n_ops"][w])]]
            queries.append(reads[r][int(h["qstart"][w]):int(h["qstart"][w]) + sum(ln for ln, op in rr if op != D)])
            runs.append(rr)
    su = walks.paths.unitig.cpu().numpy().view(np.uint32)
    pile, st = pileup_reference(h, su, strings, overlap, queries, a["flags"], runs)
    return pile, st, strings, overlap


def _assert_polished(eng, pl, ref_pile, ref_st, strings, overlap, graph, tmp_path, tag, min_cov=3):
    got = pl.host()
    for f in PLANES:
        assert got[f].tobytes() == ref_pile[f].tobytes(), (tag, f)
    assert pl.stats == ref_st and (pl.depth().cpu().numpy() == depth_of(ref_pile)).all(), (tag, pl.stats, ref_st)
    pol = pl.consensus(eng, min_cov)
    ref = consensus_reference(ref_pile, strings, overlap, min_cov)
    assert pol.stats == ref["stats"], (tag, pol.stats, ref["stats"])
    assert pol.sequences[0].cpu().numpy().view(np.uint64).tobytes() == ref["out_off"].tobytes() and pol.sequences[1].cpu().numpy().tobytes() == ref["out"].tobytes(), tag
    assert pol.pos_map.cpu().numpy().view(np.uint64).tobytes() == ref["pos_map"].tobytes() and pol.overlap.cpu().numpy().view(np.uint32).tobytes() == ref["overlap"].tobytes()
    fa, gfa, rgfa = str(tmp_path / (tag + ".fa")), str(tmp_path / (tag + ".gfa")), str(tmp_path / (tag + "_ref.gfa"))
    pkg.write_fasta(fa, *pol.sequences)
    assert open(fa, "rb").read() == b"".join(b">%d\n%s\n" % (t, s) for t, s in enumerate(ref["strings"])), tag
    pol.graph.write_gfa(gfa, sequences=pol.sequences)
    pkg.write_unitig_gfa(rgfa, graph.uni_off.cpu().numpy().view(np.uint64), graph.members.cpu().numpy().view(np.uint32), graph.counts.cpu().numpy(),
                         graph.edge_keys.cpu().numpy().view(np.uint64), graph.edge_counts.cpu().numpy().view(np.uint32),
                         sequences=(ref["out_off"], ref["out"], ref["overlap"]))
    assert open(gfa).read() == open(rgfa).read() and pol.graph is not graph and graph.overlap is not pol.overlap, tag
    return pol, ref


@pytest.mark.gpu
def test_repeat_fixture_end_to_end(eng, repeat_case, repeat_walks, tmp_path):
    """thread -> spans -> resolve -> untangle_map -> lift -> walks -> align -> pileup -> consensus -> FASTA / GFA on the device: the
    contigs' draft carries a substitution every 24th base, the clean reads polish it wherever three of them cover it; and the unitig
    graph with its own draft as it is"""
    import torch

    c, R = repeat_case, tsp.REPEAT
    outs = twk._extract_all(eng, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=R["min_count"], min_edge_count=1)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, [outs])
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, outs, len(c["reads"]), min_count=R["min_count"])
    table.close()
    resolved, partner, _ = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    contigs, node_origin, st, lift = ug.untangle_map(eng, resolved, partner)
    lifted, _ = lift.lift(eng, paths)
    cns = ns.take(node_origin)
    walks = contigs.walks(eng, lifted, cns)
    seqs = contigs.sequences(eng, cns)
    clean = tus.unitig_strings(None, {"out_off": tg._u64(seqs[0]), "out": seqs[1].cpu().numpy()})
    bad = torch.from_numpy(np.frombuffer(b"".join(spoiled(clean)), dtype=np.uint8).copy()).to(seqs[1].device)
    draft = (seqs[0], bad)
    al = contigs.align(eng, walks, outs["bases"], outs["read_off"], draft)
    assert (al.n_over, al.n_bad) == (0, 0)
    pl = contigs.pileup(eng, draft)
    pl.add(eng, walks, al, outs["bases"], outs["read_off"])
    ref_pile, ref_st, strings, overlap = _device_pile_reference(pl, walks, contigs, draft, c["reads"], al)
    pol, ref = _assert_polished(eng, pl, ref_pile, ref_st, strings, overlap, contigs, tmp_path, "contigs")
    depth, off = depth_of(ref_pile), tg._u64(seqs[0]).astype(np.int64)
    for t, s in enumerate(clean):
        deep = depth[off[t]:off[t + 1]] >= 3
        got = np.frombuffer(ref["strings"][t], dtype=np.uint8)
        assert len(got) == len(s) and (got[deep] == np.frombuffer(s, dtype=np.uint8)[deep]).all() and deep.sum() > 0.9 * len(s), t
    assert pol.stats["n_sub"] > 50 and pol.stats["n_ins"] == pol.stats["n_del"] == 0
    before = ug.walks(eng, paths, ns)  # and on the unitig graph: walks of several steps, the draft as it is
    useqs = ug.sequences(eng, ns)
    ual = ug.align(eng, before, outs["bases"], outs["read_off"], useqs)
    upl = ug.pileup(eng, useqs)
    upl.add(eng, before, ual, outs["bases"], outs["read_off"])
    upile, ust, ustrings, uov = _device_pile_reference(upl, before, ug, useqs, c["reads"], ual)
    upol, uref = _assert_polished(eng, upl, upile, ust, ustrings, uov, ug, tmp_path, "unitigs")
    assert uref["strings"] == ustrings and upol.stats["n_sub"] == 0
    print("repeat fixture polished on the device: contigs %s, %d of %d positions below min_cov" % (pol.stats, pol.stats["n_low"], len(ref["out"])))


@pytest.mark.gpu
def test_ecoli_reads_with_errors_end_to_end(eng, ecoli, ecoli_reference, ecoli_pile, tmp_path):
    """the 600 reads with 0.5 % substitutions through simplify(10, 20) and bridge(16, 2), aligned, piled up and called: the device's pile, stats, polished bases, FASTA and GFA are the references'; and the same reads through untangle_map on the
    contigs, with lifted paths"""
    mode, l, k = tsp.MODES[0]
    reads = ecoli_reference["reads"]
    outs = twk._extract_all(eng, reads, l, k, 0.05, mode)
    graph = pkg.KminmerGraph.build(eng, [outs], min_count=2, min_edge_count=1)
    ns = pkg.NodeSequences.build(eng, graph, [outs])
    sg, node_map, _ = graph.simplify(eng, 10, 20)
    ug = sg.unitigs(eng)
    table = pkg.CountTable(eng, sg.keys, sg.counts)
    paths, _ = ug.bridge(eng, ug.thread(eng, table, outs, len(reads), min_count=2))
    table.close()
    sns = ns.subset(node_map)
    walks = ug.walks(eng, paths, sns)
    seqs = ug.sequences(eng, sns)
    al = ug.align(eng, walks, outs["bases"], outs["read_off"], seqs)
    pl = ug.pileup(eng, seqs)
    st = pl.add(eng, walks, al, outs["bases"], outs["read_off"])
    assert walks.host()["path_end"].tobytes() == ecoli_reference["walks"]["path_end"].tobytes()
    ref_pile, ref_st = ecoli_pile["pile"], ecoli_pile["stats"]
    assert st == ref_st
    pol, ref = _assert_polished(eng, pl, ref_pile, ref_st, ecoli_reference["strings"], ecoli_reference["overlap"], ug, tmp_path, "ecoli")
    assert ref["stats"] == ecoli_pile["consensus"]["stats"]
    resolved, partner, _ = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
    contigs, node_origin, cst, lift = ug.untangle_map(eng, resolved, partner)
    lifted, _ = lift.lift(eng, paths)
    cns = sns.take(node_origin)
    cwalks = contigs.walks(eng, lifted, cns)
    cseqs = contigs.sequences(eng, cns)
    cal = contigs.align(eng, cwalks, outs["bases"], outs["read_off"], cseqs)
    cpl = contigs.pileup(eng, cseqs)
    cpl.add(eng, cwalks, cal, outs["bases"], outs["read_off"])
    cpile, cstats, cstrings, cov = _device_pile_reference(cpl, cwalks, contigs, cseqs, reads, cal)
    cpol, cref = _assert_polished(eng, cpl, cpile, cstats, cstrings, cov, contigs, tmp_path, "ecoli_contigs")
    print("E. coli polished on the device: unitigs %s; %d contigs %s" % (pol.stats, cst["contigs"], cpol.stats))
