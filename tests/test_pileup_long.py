"""Insertions of two or more bases in the pile-up consensus: s2k_walks_pileup_ex and s2k_pileup_consensus_ex (include/s2k.h, DESIGN.md
§3.23), UnitigGraph.pileup(long_ins=True), Pileup.long_insertions.  The references are `long_keys_reference` and
`consensus_long_reference`, serial restatements of the header's rules beside test_pileup.pileup_reference and consensus_reference; the
device's arrays equal them word for word, between guards."""
import collections
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import test_align as ta
import test_pileup as tp
import test_unitig_sequences as tus
from test_pileup import I, D, EQ, MAX_SHIFT, PLANES, REC, consensus_reference, device_pile, pileup_reference, query_of, random_pile, raw_pileup, runs_of

pkg = import_package()

SYMS = ("s2k_walks_pileup_ex", "s2k_pileup_consensus_ex")
C_LONG_STATS = tp.C_STATS + ("n_ins_long", "n_ins_long_bases")
LMIN, LMAX, POS_BITS = 2, 12, 36
_CODE, _COMP = tp._CODE, tp._COMP
SU1, OV1 = np.array([0, 1], dtype=np.uint32), np.zeros(2, dtype=np.uint32)  # one unitig: step 0 walks it forward, step 1 on its twin strand


# ---- the references ----------------------------------------------------------------------------------------------------------------
def rev36(x):
    return int(format(x, "036b")[::-1], 2)


def key_of(at, letters):
    """the vote key of `letters` (upper case ACGT, 2 .. 12 of them) inserted before forward position at"""
    return rev36(at) << 28 | len(letters) << 24 | sum(int(_CODE[c]) << (22 - 2 * i) for i, c in enumerate(letters))


def decode(key):
    key = int(key)
    n = key >> 24 & 15
    return rev36(key >> 28), bytes(b"ACGT"[key >> (22 - 2 * i) & 3] for i in range(n))


def long_keys_reference(walks, step_unitig, strings, overlap, queries, flags, runs, max_shift=MAX_SHIFT):
    """§1 of the rule, walk by walk and run by run, beside pileup_reference (same arguments) -> (keys: uint64 array in run-slot order,
    n_candidates)"""
    off, out = tp.draft_of(strings)
    u = [int(x) for x in step_unitig]
    keys, cand = [], 0
    for w in range(len(walks["first_step"])):
        if int(flags[w]):
            continue
        seg, pos, odd, end = tp.walk_sources(walks, w, u, strings, overlap, off)
        T, q, R = len(seg), queries[w], runs[w]
        x = qi = 0
        for i, (ln, op) in enumerate(R):
            if op != I:
                x += ln
                qi += ln if op != D else 0
                continue
            c = q[qi:qi + ln]
            qi += ln
            cand += LMIN <= ln <= LMAX
            if T == 0:
                continue  # n_empty_ins
            xb = x - 1 if x else 0
            o, s = int(odd[xb]), seg[xb]
            g = int(pos[xb]) + ((0 if x else 1) if o else (1 if x else 0))
            nb, e = ((R[i + 1] if i + 1 < len(R) else None) if o else (R[i - 1] if i else None)), 0
            if nb is not None and nb[1] == EQ:
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
            at = g - d
            if at == int(end[xb]):
                continue  # n_end_ins
            if LMIN <= ln <= LMAX and all(_CODE[b] < 4 for b in fwd):
                shifted = bytes(fwd[(j - d) % ln] for j in range(ln)).upper()
                keys.append(key_of(at, shifted))
    return np.array(keys, dtype=np.uint64), cand


def table_of(keys):
    """what the counter makes of the keys -> (keys ascending, counts uint32)"""
    k, c = np.unique(np.asarray(keys, dtype=np.uint64), return_counts=True)
    return k, c.astype(np.uint32)


def consensus_long_reference(pile, strings, overlap, min_cov=3, keys=(), counts=(), out_off=None):
    """§4 of the rule, position by position -> the dict of consensus_reference, stats with n_ins_long and n_ins_long_bases.  out_off:
    other unitig bounds over the same bases"""
    off, out = tp.draft_of(strings)
    off = off if out_off is None else np.asarray(out_off, dtype=np.uint64)
    n = len(out)
    P = {f: pile[f].astype(np.int64) for f in PLANES}
    cands = collections.defaultdict(list)
    for k, c in zip(keys, counts):
        cands[int(k) >> 28].append((int(k), int(c)))
    lo, hi = (int(off[0]), int(off[-1])) if len(strings) else (0, 0)
    st = dict.fromkeys(C_LONG_STATS, 0)
    new, pm = bytearray(), [0]
    for p in range(n):
        if lo <= p < hi:
            cur = int(_CODE[out[p]])
            tot = [int(P["sub%d" % c][p]) for c in range(4)] + [0]
            tot[cur] += int(P["match"][p])
            depth = int(P["match"][p] + P["del"][p]) + sum(int(P["sub%d" % c][p]) for c in range(4))
            if depth < min_cov:
                st["n_low"] += 1
                new.append(out[p])
            else:
                ins = [int(P["ins%d" % c][p]) for c in range(4)]
                cs = max(ins)
                best = ins.index(cs)
                many, called = 2 * int(P["ins_long"][p]) > depth, False
                if many:  # the table is searched only here: a table made of the keys of the same walks has cl <= ins_long[p]
                    L, cl = None, 0
                    for k, c in sorted(cands.get(rev36(p), [])):
                        if c > cl:
                            L, cl = k, c
                    if cl > cs and 2 * cl > depth:
                        letters = decode(L)[1]
                        new += letters
                        st["n_ins_long"] += 1
                        st["n_ins_long_bases"] += len(letters)
                        called = True
                if not called and 2 * cs > depth:
                    new.append(b"ACGT"[best])
                    st["n_ins"] += 1
                if many and not called:
                    st["n_long"] += 1
                top = tot.index(max(tot))
                if int(P["del"][p]) > tot[top]:
                    st["n_del"] += 1
                elif tot[cur] == tot[top]:
                    new.append(out[p])
                else:
                    new.append(b"ACGT"[top])
                    st["n_sub"] += 1
        pm.append(len(new))
    pm = np.array(pm, dtype=np.int64)
    new_off = pm[off.astype(np.int64)]
    ov = np.zeros(2 * len(strings), dtype=np.uint32)
    for t in range(len(strings)):
        a, L = int(off[t]), int(off[t + 1]) - int(off[t])
        e, o = min(int(overlap[2 * t]), L), min(int(overlap[2 * t + 1]), L)
        ov[2 * t], ov[2 * t + 1] = pm[a + L] - pm[a + L - e], pm[a + o] - pm[a]
    text = bytes(new)
    return {"strings": [text[int(new_off[t]):int(new_off[t + 1])] for t in range(len(strings))], "out_off": new_off.astype(np.uint64),
            "out": np.frombuffer(text, dtype=np.uint8), "pos_map": pm.astype(np.uint64), "overlap": ov, "stats": st}


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def mirrored(strings, specs, cigars, queries):
    """the same walks of a one-unitig draft seen from the twin strand: records, CIGARs and queries mirrored"""
    n = len(strings[0])
    out = []
    for (first, ns, ps, pe, fl), cig, q in zip(specs, cigars, queries):
        runs = runs_of(cig)[::-1]
        out.append(((first ^ 1, ns, n - pe, n - ps, fl), "".join("%d%s" % (ln, {I: "I", D: "D", EQ: "=", tp.X: "X"}[op]) for ln, op in runs), tus.revcomp(q)))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def case_of(strings, specs, cigars, queries, su=SU1, overlap=None, flags=None):
    """-> the arguments of pileup_reference / long_keys_reference"""
    overlap = np.zeros(2 * len(strings), dtype=np.uint32) if overlap is None else overlap
    return tp.one_walks(specs), np.asarray(su, dtype=np.uint32), strings, overlap, list(queries), list(flags or [0] * len(specs)), [runs_of(c) for c in cigars]


def tandem_case(unit, k, pad=20, left=b"T"):
    """a draft whose k bases before the gap continue the tandem repeat of `unit` to the left, one walk that inserts one more unit
    behind them -> (strings, specs, cigars, queries, g): the insertion is given at g and moves min(k, max_shift) to the left"""
    n = len(unit)
    tail = (unit * (k // n + 2))[-k:] if k else b""
    s = left * pad + tail + left * pad
    g = pad + k
    return [s], [(0, 1, 0, len(s), 0)], ["%d=%dI%d=" % (g, n, pad)], [s[:g] + unit + s[g:]], g


def planted_long_case(seed, alphabet, n=3000, spacing=48, read=400, step=50, stretches=(2, 3, 7, 12)):
    """a clean string; a draft that misses a stretch of 2, 3, 7, 12 bases in turn every `spacing` bases; reads of the clean string tiled
    on alternating strands, the two ends covered four times, each one walk of one step with the single-run CIGAR that its missing
    stretches give -> (clean, draft, walks, reads, cigars, n_stretches)"""
    rng = np.random.default_rng(seed)
    clean = ta.random_seq(rng, n, alphabet)
    present = np.ones(n, dtype=bool)
    starts_at = list(range(spacing, n - spacing, spacing))
    for j, a in enumerate(starts_at):
        present[a:a + stretches[j % len(stretches)]] = False
    cmap = np.concatenate([[0], np.cumsum(present)])
    draft = bytes(np.frombuffer(clean, dtype=np.uint8)[present])
    starts = list(range(0, n - read + 1, step))
    starts = [0] * 3 + starts + [starts[-1]] * 3
    reads, specs, cigars = [], [], []
    for r, s in enumerate(starts):
        a, b = int(cmap[s]), int(cmap[s + read])
        runs, x = [], s
        while x < s + read:
            y = x
            while y < s + read and present[y] == present[x]:
                y += 1
            runs.append((y - x, EQ if present[x] else I))
            x = y
        if r % 2 == 0:
            reads.append(clean[s:s + read])
            specs.append((0, 1, a, b, 0))
        else:
            reads.append(tus.revcomp(clean[s:s + read]))
            specs.append((1, 1, len(draft) - b, len(draft) - a, 0))
            runs = runs[::-1]
        cigars.append(runs)
    walks = tp.one_walks(specs)
    walks.update(walk_off=np.arange(len(reads) + 1, dtype=np.uint64), qstart=np.zeros(len(reads), dtype=np.uint32), qend=np.full(len(reads), read, dtype=np.uint32))
    return clean, draft, walks, reads, cigars, len(starts_at)


SPACING = 48  # DESIGN.md §3.23 records it


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported_and_constants():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    facade = open(os.path.join(ROOT, "include", "s2k.hpp")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header and s in facade, s
    assert hasattr(pkg.Engine, "walks_pileup_ex") and hasattr(pkg.Engine, "pileup_consensus_ex")
    assert all(hasattr(pkg.Pileup, f) for f in ("close", "long_insertions"))
    assert (pkg.LONG_INS_MIN, pkg.LONG_INS_MAX, pkg.LONG_INS_POS_BITS) == (LMIN, LMAX, POS_BITS)
    assert pkg.CONSENSUS_LONG_STATS == C_LONG_STATS and len(C_LONG_STATS) <= pkg.CONSENSUS_STATS_WORDS
    assert pkg.decode_long_keys([key_of(77, b"ACGTT")], [5]) == [(77, b"ACGTT", 5)]


def test_cpp_long_facade_compiles_links_and_has_the_constants(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "pileup_long_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pileup_long_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    facts = dict(line.split() for line in subprocess.check_output([exe], text=True).splitlines()[:3])
    assert facts == {"S2K_LONG_INS_MIN": str(pkg.LONG_INS_MIN), "S2K_LONG_INS_MAX": str(pkg.LONG_INS_MAX), "S2K_LONG_INS_POS_BITS": str(pkg.LONG_INS_POS_BITS)}


HAND_DRAFT = b"ACGTACGTAC" * 5


def hand_cases():
    """-> {name: (case, [(at, letters)] expected by hand)}"""
    s = [HAND_DRAFT]
    out = {}
    # an even step: GA between bytes 19 (C) and 20 (A): C != A, no shift
    out["even"] = (case_of(s, [(0, 1, 0, 50, 0)], ["20=2I30="], [HAND_DRAFT[:20] + b"GA" + HAND_DRAFT[20:]]), [(20, b"GA")])
    # the same insertion on the odd step: the walk reads the twin strand, the gap lies behind its byte 29, the query carries TC
    rc = tus.revcomp(HAND_DRAFT)
    out["odd"] = (case_of(s, [(1, 1, 0, 50, 0)], ["30=2I20="], [rc[:30] + b"TC" + rc[30:]]), [(20, b"GA")])
    # AC behind ...GTAC: C == C, A == A, then T != C: two to the left, a whole turn of two letters
    out["turn"] = (case_of(s, [(0, 1, 0, 50, 0)], ["20=2I30="], [HAND_DRAFT[:20] + b"AC" + HAND_DRAFT[20:]]), [(18, b"AC")])
    # a shift that rotates: ACG behind k letters of ...ACGACG
    for k, letters in ((1, b"GAC"), (2, b"CGA"), (3, b"ACG"), (4, b"GAC")):
        strings, specs, cigars, queries, g = tandem_case(b"ACG", k)
        out["rotate %d" % k] = (case_of(strings, specs, cigars, queries), [(g - k, letters)])
        ms, mc, mq = mirrored(strings, specs, cigars, queries)
        out["rotate %d odd" % k] = (case_of(strings, ms, mc, mq), [(g - k, letters)])
    # a run stopped by its piece: six letters agree, the = run before the gap is two long
    t = b"T" * 20 + b"ACGACG" + b"T" * 20
    out["stopped"] = (case_of([t], [(0, 1, 0, 46, 0)], ["23=1X2=3I20="], [b"T" * 20 + b"ACG" + b"C" + b"CG" + b"ACG" + b"T" * 20]), [(24, b"CGA")])
    return out


def test_reference_keys_by_hand():
    for name, (c, want) in hand_cases().items():
        keys, cand = long_keys_reference(*c)
        assert [decode(k) for k in keys] == want and cand == len(want), (name, [decode(k) for k in keys], want)
        pile, st = pileup_reference(*c)
        assert np.nonzero(pile["ins_long"])[0].tolist() == [want[0][0]], name
    k = key_of(20, b"GA")
    assert k == rev36(20) << 28 | 2 << 24 | 2 << 22 | 0 << 20 and rev36(20) == 0b00101 << 31 and rev36(rev36(12345)) == 12345
    assert key_of(2 ** 36 - 1, b"T" * 12) < 2 ** 64 - 1 and (key_of(0, b"TT") >> 24 & 15) == 2


def test_consensus_long_reference_with_an_empty_table_is_the_old_reference():
    rng = np.random.default_rng(301)
    strings = [ta.random_seq(rng, n, b"ACGTacgtN") for n in (0, 1, 15, 16, 17, 300)]
    overlap = np.array([int(rng.integers(0, n + 3)) for n in (0, 1, 15, 16, 17, 300) for _ in (0, 1)], dtype=np.uint32)
    for min_cov in (0, 3, 6):
        pile = random_pile(rng, strings)
        a, b = consensus_long_reference(pile, strings, overlap, min_cov), consensus_reference(pile, strings, overlap, min_cov)
        assert a["strings"] == b["strings"] and all(a[f].tobytes() == b[f].tobytes() for f in ("out_off", "out", "pos_map", "overlap"))
        assert a["stats"] == {**b["stats"], "n_ins_long": 0, "n_ins_long_bases": 0}


def _planted_inputs(seed, alphabet, spacing=SPACING):
    clean, draft, walks, reads, cigars, n_st = planted_long_case(seed, alphabet, spacing=spacing)
    return clean, draft, n_st, (walks, SU1, [draft], OV1, reads, [0] * len(reads), cigars)


def test_reference_invariants_strands_batches_and_ins_long():
    clean, draft, n_st, c = _planted_inputs(5, b"ACGT")
    keys, cand = long_keys_reference(*c)
    pile, st = pileup_reference(*c)
    assert cand == sum(1 for r in c[6] for ln, op in r if op == I and LMIN <= ln <= LMAX) and len(keys) > 6 * n_st
    # per position the keyed counts add up to ins_long: every long run of this case is keyed
    at = np.array([decode(k)[0] for k in keys])
    assert (np.bincount(at, minlength=len(draft)) == pile["ins_long"]).all()
    # a run with an N and a run of 13 are counted in ins_long and have no key
    s = [HAND_DRAFT]
    q = HAND_DRAFT[:10] + b"GNG" + HAND_DRAFT[10:30] + b"G" * 13 + HAND_DRAFT[30:]
    c2 = case_of(s, [(0, 1, 0, 50, 0)], ["10=3I20=13I20="], [q])
    keys2, cand2 = long_keys_reference(*c2)
    p2, _ = pileup_reference(*c2)
    assert len(keys2) == 0 and cand2 == 1 and int(p2["ins_long"].sum()) == 2
    # the same insertion from both strands is one key: the reads alternate, and a full stretch has one key among all reads that hold it whole
    strand = [collections.Counter(long_keys_reference({f: c[0][f][r::2] for f in REC}, c[1], c[2], c[3], c[4][r::2], c[5][r::2], c[6][r::2])[0].tolist()) for r in (0, 1)]
    whole = [{k for k, v in s_.items() if v >= 2} for s_ in strand]  # (a read that ends inside a stretch holds a part of it, once)
    assert whole[0] == whole[1] and len(whole[0]) == n_st
    # two batches give the multiset of one batch
    h = len(c[4]) // 3
    part = lambda a, b: ({f: c[0][f][a:b] for f in REC}, c[1], c[2], c[3], c[4][a:b], c[5][a:b], c[6][a:b])  # noqa: E731
    k1, c1 = long_keys_reference(*part(0, h))
    k2, c2_ = long_keys_reference(*part(h, len(c[4])))
    assert collections.Counter(k1.tolist() + k2.tolist()) == collections.Counter(keys.tolist()) and c1 + c2_ == cand
    assert np.concatenate([k1, k2]).tobytes() == keys.tobytes()  # and in run-slot order


def consensus_hand_case():
    """three unitigs of 16, 10 and 1 bases with depth 6 everywhere but where noted -> (pile, strings, overlap, keys, counts)"""
    strings, overlap = [b"ACGTACGTACGTACGT", b"GGGGCCCCTT", b"T"], np.array([3, 2, 4, 4, 1, 1], dtype=np.uint32)
    pile = tp.new_pile(27)
    pile["match"][:] = 6
    K = {}

    def cand(p, letters, count, ins_long=None):
        K[key_of(p, letters)] = count
        if ins_long is not None:
            pile["ins_long"][p] = ins_long

    cand(0, b"GGA", 4, 4)       # before a unitig's first base
    cand(15, b"CC", 5, 5)       # before its last one
    cand(2, b"TT", 4, 4)        # two candidates with equal counts: the smallest key wins, AC < TT
    cand(2, b"AC", 4)
    cand(4, b"GG", 4, 5)        # cl == cs: the single letter wins
    pile["ins1"][4] = 4
    cand(6, b"GGG", 3, 6)       # 2 cl == depth: not called
    cand(8, b"AAAA", 4, 6)      # 2 cl == depth + 1, with depth 7
    pile["match"][8] = 7
    cand(10, b"CCCCC", 2, 2)    # depth < min_cov: nothing is inserted, the byte is kept
    pile["match"][10] = 2
    cand(12, b"ACGTACGTACGT", 6, 3)  # 2 ins_long == depth: the table is not searched, whatever it holds
    cand(16, b"TG", 5, 5)       # the first base of unitig 1
    for j in range(70):         # 70 distinct candidates at one position: the 41st has the largest count
        cand(20, bytes(b"ACGT"[j >> (2 * i) & 3] for i in range(4)), 3 + (j == 40), 6)
    cand(26, b"AG", 6, 6)       # the last position of all, a unitig of one base
    cand(27, b"AG", 6)          # and past the draft
    keys = np.array(sorted(K), dtype=np.uint64)
    return pile, strings, overlap, keys, np.array([K[int(k)] for k in keys], dtype=np.uint32)


def test_consensus_long_reference_by_hand():
    pile, strings, overlap, keys, counts = consensus_hand_case()
    ref = consensus_long_reference(pile, strings, overlap, 3, keys, counts)
    assert ref["strings"][0] == b"GGA" + b"AC" + b"AC" + b"GT" + b"C" + b"ACGT" + b"AAAA" + b"ACGT" + b"ACG" + b"CC" + b"T"
    assert ref["strings"][1] == b"TG" + b"GGGG" + b"AGGA" + b"CCCCTT" and ref["strings"][2] == b"AG" + b"T"
    assert ref["stats"] == {"n_low": 1, "n_sub": 0, "n_del": 0, "n_ins": 1, "n_long": 2, "n_ins_long": 7, "n_ins_long_bases": 19}
    assert ref["pos_map"][:4].tolist() == [0, 4, 5, 8] and ref["overlap"].tolist()[:2] == [5, 5]  # inserted letters belong to the position they precede
    out = consensus_long_reference(pile, strings, overlap, 3, keys, counts, out_off=[1, 16, 26, 26])
    assert out["strings"] == [ref["strings"][0][4:], ref["strings"][1], b""] and out["stats"]["n_ins_long"] == 5


@pytest.mark.parametrize("alphabet", [b"ACGT", b"AACGAA"])
def test_planted_stretches_are_restored_by_hand_made_cigars(alphabet):
    restored = total = 0
    for seed in range(3):
        clean, draft, n_st, c = _planted_inputs(seed, alphabet)
        keys, _ = long_keys_reference(*c)
        pile, st = pileup_reference(*c)
        assert (tp.depth_of(pile) >= 3).all()  # three reads cover every position
        got = consensus_long_reference(pile, [draft], OV1, 3, *table_of(keys))
        plain = consensus_reference(pile, [draft], OV1, 3)
        print("%s seed %d spacing %d: %d stretches planted, %d called (%d bases), n_long %d; without the table n_long %d" % (
            alphabet.decode(), seed, SPACING, n_st, got["stats"]["n_ins_long"], got["stats"]["n_ins_long_bases"], got["stats"]["n_long"], plain["stats"]["n_long"]))
        assert got["strings"][0] == clean and got["stats"]["n_low"] == 0, (alphabet, seed, got["stats"])
        assert got["stats"]["n_ins_long"] == n_st and got["stats"]["n_long"] == 0
        assert plain["strings"][0] != clean and plain["stats"]["n_long"] > 0  # long_ins=False semantics
        restored += got["stats"]["n_ins_long"]
        total += n_st
    assert restored == total


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = tp.GUARD
_dev, _host, _ptr = tp._dev, tp._host, tp._ptr
KMARK = np.array(-0x5A5A5A5A5A).astype(np.int64).view(np.uint64)


def raw_pileup_ex(eng, walks, su, strings, overlap, queries, flags, runs, max_shift=MAX_SHIFT, pile=None, capacity=None, keys=True, n_bases=None):
    """s2k_walks_pileup_ex through ctypes, guards behind every plane and behind the key buffer -> (status, stats, host planes with
    guards, key buffer with guards, n_candidates, n_long_keys).  capacity None: as many keys as the reference counts candidates"""
    import torch

    out_off, out = tp.draft_of(strings)
    pool, qb = tp.query_pool(queries)
    ops_off, n_ops, ops = tp.alignment_arrays(flags, runs)
    arr = {"first_step": (walks["first_step"], np.uint64), "n_steps": (walks["n_steps"], np.uint32), "path_start": (walks["path_start"], np.uint64),
           "path_end": (walks["path_end"], np.uint64), "flags": (walks["flags"], np.uint32), "unitig": (su, np.uint32), "out_off": (out_off, np.uint64),
           "out": (out, np.uint8), "overlap": (overlap, np.uint32), "query": (pool, np.uint8), "q_begin": (qb, np.uint64),
           "aflags": (np.asarray(flags), np.uint32), "ops_off": (ops_off, np.uint64), "n_ops": (n_ops, np.uint32), "ops": (ops, np.uint32)}
    dv = {k: _dev(a, dt) for k, (a, dt) in arr.items()}
    planes, p = device_pile(len(out), pile)
    if capacity is None:
        capacity = sum(1 for fl, r in zip(flags, runs) if not fl for ln, op in r if op == I and LMIN <= ln <= LMAX)
    buf = torch.full((capacity + GUARD,), -0x5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    st = (ctypes.c_uint64 * pkg.PILEUP_STATS_WORDS)(*([777] * pkg.PILEUP_STATS_WORDS))
    nc, nk = ctypes.c_uint64(777), ctypes.c_uint64(777)
    P = lambda k: _ptr(dv[k])  # noqa: E731
    torch.cuda.synchronize()
    s = eng.lib.s2k_walks_pileup_ex(eng.ctx, len(walks["first_step"]), P("first_step"), P("n_steps"), P("path_start"), P("path_end"), P("flags"), P("unitig"), len(su),
                                    P("out_off"), P("out"), len(out) if n_bases is None else n_bases, P("overlap"), len(strings), P("query"), len(pool), P("q_begin"),
                                    P("aflags"), P("ops_off"), P("n_ops"), P("ops"), len(ops), max_shift, ctypes.byref(p), st,
                                    _ptr(buf) if keys else None, capacity, ctypes.byref(nc), ctypes.byref(nk))
    torch.cuda.synchronize()
    return s, list(st), {f: _host(t, np.uint32) for f, t in zip(PLANES, planes)}, _host(buf, np.uint64), nc.value, nk.value


def device_long(eng, case, tag, max_shift=MAX_SHIFT, pile=None):
    """the _ex call against both references and against s2k_walks_pileup -> (reference pile, stats, keys)"""
    ref, rst = pileup_reference(*case, max_shift, pile)
    want, cand = long_keys_reference(*case, max_shift)
    s, st, got, buf, nc, nk = raw_pileup_ex(eng, *case, max_shift=max_shift, pile=pile)
    assert s == 0, (tag, s, eng.lib.s2k_last_error(eng.ctx))
    tp.assert_pile(got, ref, sum(len(x) for x in case[2]), tag)
    assert st[:len(tp.P_STATS)] == [rst[f] for f in tp.P_STATS] and st[len(tp.P_STATS):] == [0] * (len(st) - len(tp.P_STATS)), (tag, st, rst)
    assert (nc, nk) == (cand, len(want)), (tag, nc, cand, nk, len(want))
    if buf[:nk].tobytes() != want.tobytes():
        x = np.nonzero(buf[:nk] != want)[0]
        raise AssertionError((tag, "keys differ at", x[:8].tolist(), [decode(k) for k in buf[x[:8]]], [decode(k) for k in want[x[:8]]]))
    assert (buf[nk:] == KMARK).all(), (tag, "key guard")
    s0, st0, old = raw_pileup(eng, *case, max_shift, pile)
    assert s0 == 0 and st0 == st and all(old[f].tobytes() == got[f].tobytes() for f in PLANES), (tag, "s2k_walks_pileup")
    return ref, rst, want


def join(*cases):
    """several one-unitig cases over the same draft in one call"""
    walks = tp.one_walks([tuple(int(c[0][f][w]) for f in REC) for c in cases for w in range(len(c[0]["first_step"]))])
    return (walks, cases[0][1], cases[0][2], cases[0][3], [q for c in cases for q in c[4]], [f for c in cases for f in c[5]], [r for c in cases for r in c[6]])


@pytest.mark.gpu
def test_device_keys_hand_cases_run_lengths_and_other_bytes(eng):
    for name, (c, want) in hand_cases().items():
        _, _, keys = device_long(eng, c, name)
        assert [decode(k) for k in keys] == want
    rng = np.random.default_rng(310)
    s = [ta.random_seq(rng, 120)]
    specs, cigars, queries = [], [], []
    for j, n in enumerate((1, 2, 12, 13)):  # on both strands, each walk with one run
        cig = "%d=%dI%d=" % (20 + j, n, 30)
        t = s[0][5 * j:5 * j + 50 + j]
        specs.append((0, 1, 5 * j, 5 * j + 50 + j, 0))
        cigars.append(cig)
        queries.append(query_of(rng, t, runs_of(cig)))
    ms, mc, mq = mirrored(s, specs, cigars, queries)
    c = case_of(s, specs + ms, cigars + mc, queries + mq)
    ref, st, keys = device_long(eng, c, "lengths")
    assert sorted(len(decode(k)[1]) for k in keys) == [2, 2, 12, 12] and int(ref["ins_long"].sum()) == 6
    device_long(eng, c, "lengths, no shift", max_shift=0)
    # a run with an N, a lower-case run (its key is the upper-case one's), an N next to the run
    t = s[0][:60]
    q = [t[:20] + b"GNG" + t[20:], t[:20] + b"gtg" + t[20:], t[:19] + b"N" + b"CC" + t[20:]]
    c = case_of(s, [(0, 1, 0, 60, 0)] * 3, ["20=3I40=", "20=3I40=", "19=1X2I40="], q)
    ref, st, keys = device_long(eng, c, "other bytes", max_shift=0)
    assert [decode(k)[1] for k in keys] == [b"GTG", b"CC"] and st["n_other"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [b"ACG", b"CA", b"ACGGTCATTGCA"])
def test_device_keys_tandem_shifts_on_both_strands(eng, unit):
    n = len(unit)
    for k in sorted({0, 1, n - 1, n, n + 1, 63, 64, 65}):
        nxt = unit[n - 1 - k % n]  # the letter that would continue the repeat to the left: the pad is another one
        strings, specs, cigars, queries, g = tandem_case(unit, k, left=bytes([next(x for x in b"TGAC" if x != nxt)]))
        ms, mc, mq = mirrored(strings, specs, cigars, queries)
        c = case_of(strings, specs + ms, cigars + mc, queries + mq)
        for shift in (MAX_SHIFT, 5, 0):
            d = min(k, shift)
            ref, st, keys = device_long(eng, c, (unit, k, shift), max_shift=shift)
            want = (g - d, bytes(unit[(j - d) % n] for j in range(n)))
            assert [decode(x) for x in keys] == [want, want] and ref["ins_long"][g - d] == 2, (unit, k, shift)


@pytest.mark.gpu
def test_device_keys_ends_empty_targets_flags_and_rounds(eng):
    rng = np.random.default_rng(311)
    strings = [ta.random_seq(rng, 50)]
    # a gap at the unitig's first base (kept) and at its end (dropped unless it moves), on both strands; inside the unitig at a target's ends
    specs = [(0, 1, 0, 50, 0), (1, 1, 0, 50, 0), (0, 1, 5, 45, 0), (1, 1, 5, 45, 0)]
    cigars = ["2I50=3I", "3I50=2I", "4I40=5I", "5I40=4I"]
    q = [query_of(rng, t, runs_of(c)) for t, c in zip(tp.targets_of(tp.one_walks(specs), SU1, strings, OV1)[0], cigars)]
    ref, st, keys = device_long(eng, case_of(strings, specs, cigars, q), "ends")
    assert st["n_end_ins"] >= 1 and len(keys) + st["n_end_ins"] == 8 and sorted(decode(k)[0] for k in keys)[:2] == [0, 0]
    ref, st, keys = device_long(eng, case_of(strings, specs, cigars, q), "ends, no shift", max_shift=0)
    assert st["n_end_ins"] == 2 and len(keys) == 6
    # an empty target: its run is a candidate and has no key; a flagged walk is not looked at
    d = strings[0]
    c = case_of(strings, [(0, 1, 7, 7, 0), (0, 1, 3, 9, 0), (0, 1, 10, 30, 0)], ["3I", "3=2I3=", "10=4I10="], [b"ACG", d[3:6] + b"GG" + d[6:9], d[10:20] + b"ACGT" + d[20:30]],
                flags=[0, 0, 1])
    ref, st, keys = device_long(eng, c, "empty and flagged")
    assert st["n_empty_ins"] == 1 and st["walks_skipped"] == 1 and len(keys) == 1 and long_keys_reference(*c)[1] == 2
    # a circular unitig walked round: a run in the second round, before, on and behind the round's end, on both strands
    L = 50
    for U in (0, 1):
        for delta in (-1, 0, 1):
            pre = 2 * L - 7 + delta
            cig = "%d=3I%d=" % (pre, 3 * L - pre)
            (t,), _ = tp.targets_of(tp.one_walks([(U, 1, 7, 7 + 3 * L, 1)]), SU1, strings, OV1)
            cc = case_of(strings, [(U, 1, 7, 7 + 3 * L, 1)], [cig], [query_of(rng, t, runs_of(cig))])
            ref, st, keys = device_long(eng, cc, ("round", U, delta))
            assert len(keys) + st["n_end_ins"] == 1 and int(ref["match"].max()) == 3


def seam_case(rng, n_runs, n_walks):
    s = [ta.random_seq(rng, 1000)]
    specs, cigars, queries = [], [], []
    for w in range(n_walks):
        k = n_runs // n_walks + (w < n_runs % n_walks)
        U, a = w & 1, int(rng.integers(0, 1000 - 5 * (k + 1)))
        cig = "5=" + "2I5=" * k
        specs.append((U, 1, a, a + 5 * (k + 1), 0))
        cigars.append(cig)
    walks = tp.one_walks(specs)
    targets, _ = tp.targets_of(walks, SU1, s, OV1)
    return case_of(s, specs, cigars, [query_of(rng, t, runs_of(c)) for t, c in zip(targets, cigars)])


@pytest.mark.gpu
@pytest.mark.parametrize("n_runs,n_walks", [(2047, 63), (2048, 64), (2049, 65)])
def test_device_keys_compaction_seams(eng, n_runs, n_walks):
    c = seam_case(np.random.default_rng(320 + n_walks), n_runs, n_walks)
    ref, st, keys = device_long(eng, c, ("seam", n_runs))
    assert len(keys) + st["n_end_ins"] == n_runs


@pytest.mark.gpu
def test_device_keys_null_capacity_two_calls_and_two_adds(eng):
    clean, draft, n_st, c = _planted_inputs(6, b"AACGAA")
    c = ({f: c[0][f] for f in REC},) + c[1:]
    ref, rst, want = device_long(eng, c, "planted")
    n = len(draft)
    # without a key buffer: the old call
    s, st, got, buf, nc, nk = raw_pileup_ex(eng, *c, keys=False, capacity=4)
    assert (s, nk) == (0, 0) and nc == long_keys_reference(*c)[1] and (buf == KMARK).all()
    tp.assert_pile(got, ref, n, "NULL")
    # a short capacity: status 7, the candidates reported, pile and key buffer as they were
    before = {f: np.arange(n, dtype=np.uint32) * (i + 1) for i, f in enumerate(PLANES)}
    s, st, got, buf, nc2, nk = raw_pileup_ex(eng, *c, pile=before, capacity=nc - 1)
    assert (s, nc2, nk) == (7, nc, 0) and st == [0] * 8 and (buf == KMARK).all()
    tp.assert_pile(got, before, n, "short capacity")
    # 2^36 bases with a key buffer: refused on the host
    s, st, got, buf, nc2, nk = raw_pileup_ex(eng, *c, pile=before, n_bases=2 ** 36)
    assert (s, nc2, nk) == (1, 0, 0) and (buf == KMARK).all() and b"2^36" in eng.lib.s2k_last_error(eng.ctx)
    tp.assert_pile(got, before, n, "2^36")
    # two calls are identical
    a, b = raw_pileup_ex(eng, *c), raw_pileup_ex(eng, *c)
    assert a[3].tobytes() == b[3].tobytes() and all(a[2][f].tobytes() == b[2][f].tobytes() for f in PLANES)
    # two adds equal one
    h = len(c[4]) // 3
    part = lambda x, y: ({f: c[0][f][x:y] for f in REC}, c[1], c[2], c[3], c[4][x:y], c[5][x:y], c[6][x:y])  # noqa: E731
    p1, _, k1 = device_long(eng, part(0, h), "first batch")
    p2, _, k2 = device_long(eng, part(h, len(c[4])), "second batch", pile=p1)
    assert all((p2[f] == ref[f]).all() for f in PLANES) and np.concatenate([k1, k2]).tobytes() == want.tobytes()


@pytest.mark.gpu
def test_device_keys_through_the_counter_in_two_batches(eng):
    """a draft of a few hundred bases: every position's high bits are zero, so the unreversed layout would be one radix bucket"""
    import torch

    clean, draft, walks, reads, cigars, n_st = planted_long_case(8, b"ACGT", n=500, read=200, step=25)
    c = ({f: walks[f] for f in REC}, SU1, [draft], OV1, reads, [0] * len(reads), cigars)
    want, _ = long_keys_reference(*c)
    h = len(reads) // 2
    ctr = pkg.KminmerCounter(eng)
    try:
        for x, y in ((0, h), (h, len(reads))):
            part = ({f: c[0][f][x:y] for f in REC}, c[1], c[2], c[3], c[4][x:y], c[5][x:y], c[6][x:y])
            s, st, got, buf, nc, nk = raw_pileup_ex(eng, *part)
            assert s == 0
            ctr.add_tensor(torch.from_numpy(buf[:nk].view(np.int64).copy()).to("cuda:0"))
        for min_count in (1, 2):
            k, cnt = ctr.finish(min_count)
            rk, rc = table_of(want)
            keep = rc >= min_count
            assert k.cpu().numpy().view(np.uint64).tobytes() == rk[keep].tobytes() and cnt.cpu().numpy().view(np.uint32).tobytes() == rc[keep].tobytes(), min_count
    finally:
        ctr.close()
    assert len(table_of(want)[0]) >= n_st and len(draft) < 512


# ---- consensus ------------------------------------------------------------------------------------------------------------------------
C_OUT, C_FILL, C_T, _cmarked = tp.C_OUT, tp.C_FILL, tp.C_T, tp._cmarked


def raw_consensus_ex(eng, pile, strings, overlap, min_cov, keys, counts, capacity=None, want=("out_off", "out", "pos_map", "overlap"), n_keys=None, n_bases=None, out_off=None):
    """s2k_pileup_consensus_ex through ctypes, guards behind every output -> (status, n_new_bases, stats, host arrays with guards)"""
    import torch

    off, out = tp.draft_of(strings)
    n, T = len(out), len(strings)
    planes, p = device_pile(n, pile)
    d_off, d_out, d_ov = _dev(off if out_off is None else out_off, np.uint64), _dev(out, np.uint8), _dev(overlap, np.uint32)
    d_k, d_c = _dev(np.asarray(keys, dtype=np.uint64), np.uint64), _dev(np.asarray(counts, dtype=np.uint32), np.uint32)
    cap = int(capacity if capacity is not None else 0)
    size = {"out_off": T + 1, "out": max(cap, 1) + 15, "pos_map": n + 1, "overlap": max(2 * T, 1)}
    res = {f: torch.full((size[f] + GUARD,), C_FILL[C_OUT[f]], dtype=getattr(torch, C_T[C_OUT[f]]), device="cuda:0") for f in want}
    nn = ctypes.c_uint64(777)
    st = (ctypes.c_uint64 * pkg.CONSENSUS_STATS_WORDS)(*([777] * pkg.CONSENSUS_STATS_WORDS))
    R = lambda f: _ptr(res[f]) if f in res else None  # noqa: E731
    nk = len(keys) if n_keys is None else n_keys
    torch.cuda.synchronize()
    s = eng.lib.s2k_pileup_consensus_ex(eng.ctx, ctypes.byref(p), _ptr(d_off), _ptr(d_out), n if n_bases is None else n_bases, _ptr(d_ov), T, min_cov, R("out_off"),
                                        R("out"), cap, R("pos_map"), R("overlap"), ctypes.byref(nn), st, _ptr(d_k, len(keys) == 0), _ptr(d_c, len(keys) == 0), nk)
    torch.cuda.synchronize()
    return s, nn.value, list(st), {f: _host(x, C_OUT[f]) for f, x in res.items()}


def device_consensus_long(eng, pile, strings, overlap, min_cov, keys, counts, tag, out_off=None):
    """sizes call, full call and one-short capacity against consensus_long_reference -> the reference"""
    ref = consensus_long_reference(pile, strings, overlap, min_cov, keys, counts, out_off)
    m, T, n = len(ref["out"]), len(strings), sum(len(s) for s in strings)
    want_st = [ref["stats"][f] for f in C_LONG_STATS] + [0]
    s, nn, st, got = raw_consensus_ex(eng, pile, strings, overlap, min_cov, keys, counts, want=(), out_off=out_off)
    assert (s, nn, st) == (0, m, want_st), (tag, "sizes", s, nn, m, st, want_st, eng.lib.s2k_last_error(eng.ctx))
    sizes = {"out_off": T + 1, "out": m, "pos_map": n + 1, "overlap": 2 * T}
    s, nn, st, got = raw_consensus_ex(eng, pile, strings, overlap, min_cov, keys, counts, capacity=m, out_off=out_off)
    assert (s, nn, st) == (0, m, want_st), (tag, s, nn, m, st, want_st)
    for f in got:
        if got[f][:sizes[f]].tobytes() != ref[f].tobytes():
            x = np.nonzero(got[f][:sizes[f]] != ref[f])[0]
            raise AssertionError((tag, f, "differs at", x[:8].tolist(), got[f][x[:8]].tolist(), ref[f][x[:8]].tolist()))
        assert _cmarked(got[f], max(sizes[f], 1) if f == "overlap" else sizes[f]), (tag, f, "guard")
    if m:
        s, nn, st, got = raw_consensus_ex(eng, pile, strings, overlap, min_cov, keys, counts, capacity=m - 1, out_off=out_off)
        assert (s, nn, st) == (7, m, [0] * 8) and all(_cmarked(x) for x in got.values()), (tag, "capacity")
    return ref


def random_table(rng, pile, n, p_cand=0.3, many=4):
    """candidates at about p_cand of the positions (one to `many` each, 2 .. 12 letters, counts round the depth), ins_long raised at most of
    them so that the table is searched, and a few candidates past the draft -> (keys ascending, counts)"""
    depth = tp.depth_of(pile)
    keys, counts = {}, {}
    for p in np.nonzero(rng.random(n) < p_cand)[0].tolist() + [n, n + 5]:
        for _ in range(int(rng.integers(1, many + 1))):
            k = key_of(p, ta.random_seq(rng, int(rng.integers(LMIN, LMAX + 1))))
            keys[k] = int(rng.integers(0, (int(depth[p]) if p < n else 4) + 2))
        if p < n and rng.random() < 0.8:
            pile["ins_long"][p] = int(depth[p]) // 2 + int(rng.integers(0, 3))
    ks = np.array(sorted(keys), dtype=np.uint64)
    return ks, np.array([keys[int(k)] for k in ks], dtype=np.uint32)


@pytest.mark.gpu
def test_device_consensus_long_random_tables_and_unitig_lengths(eng):
    rng = np.random.default_rng(330)
    lens = [0, 1, 15, 16, 17, 0, 300, 3]
    strings = [ta.random_seq(rng, n, b"ACGTacgtN") for n in lens]
    overlap = np.array([int(rng.integers(0, n + 3)) for n in lens for _ in (0, 1)], dtype=np.uint32)
    seen = dict.fromkeys(C_LONG_STATS, 0)
    for min_cov in (0, 3, 6):
        pile = random_pile(rng, strings)
        keys, counts = random_table(rng, pile, sum(lens))
        ref = device_consensus_long(eng, pile, strings, overlap, min_cov, keys, counts, ("random", min_cov))
        for f in C_LONG_STATS:
            seen[f] += ref["stats"][f]
    assert seen["n_ins_long"] > 10 and seen["n_long"] > 10 and seen["n_ins_long_bases"] > 2 * seen["n_ins_long"] and seen["n_low"] > 10, seen
    # twelve letters before every second position of unitigs of 15, 16 and 17 bases: the writes straddle every 16-byte boundary
    strings = [ta.random_seq(rng, n) for n in (15, 16, 17)]
    n = 48
    pile = tp.new_pile(n)
    pile["match"][:] = 4
    pile["ins_long"][::2] = 3
    keys = np.array(sorted(key_of(p, ta.random_seq(rng, 12)) for p in range(0, n, 2)), dtype=np.uint64)
    ref = device_consensus_long(eng, pile, strings, np.zeros(6, dtype=np.uint32), 3, keys, np.full(len(keys), 3, dtype=np.uint32), "straddle")
    assert ref["stats"]["n_ins_long"] == 24 and len(ref["out"]) == 48 + 24 * 12 and ref["stats"]["n_long"] == 0


@pytest.mark.gpu
def test_device_consensus_long_hand_cases(eng):
    pile, strings, overlap, keys, counts = consensus_hand_case()
    ref = device_consensus_long(eng, pile, strings, overlap, 3, keys, counts, "hand")
    assert ref["stats"]["n_ins_long"] == 7
    # other bounds over the same bases: positions 0 and 26 lie outside [out_off[0], out_off[T]) and emit nothing, their candidates are not called
    ref = device_consensus_long(eng, pile, strings, overlap, 3, keys, counts, "outside", out_off=[1, 16, 26, 26])
    assert ref["stats"]["n_ins_long"] == 5 and ref["pos_map"][:2].tolist() == [0, 0]
    # the empty table: the old call in all outputs and stats
    rng = np.random.default_rng(331)
    rp = random_pile(rng, strings)
    old = tp.device_consensus(eng, rp, strings, overlap, 3, "old")
    s, nn, st, got = raw_consensus_ex(eng, rp, strings, overlap, 3, [], [], capacity=len(old["out"]))
    assert (s, nn) == (0, len(old["out"])) and st == [old["stats"][f] for f in tp.C_STATS] + [0] * 3
    sizes = {"out_off": 4, "out": len(old["out"]), "pos_map": 28, "overlap": 6}
    assert all(got[f][:sizes[f]].tobytes() == old[f].tobytes() and _cmarked(got[f], sizes[f]) for f in got)


@pytest.mark.gpu
def test_device_consensus_long_outside_the_unitigs_and_refusals(eng):
    rng = np.random.default_rng(332)
    strings = [ta.random_seq(rng, n) for n in (40, 0, 25)]
    overlap = np.array([5, 5, 0, 0, 7, 3], dtype=np.uint32)
    pile = random_pile(rng, strings)
    keys, counts = random_table(rng, pile, 65)
    ref = device_consensus_long(eng, pile, strings, overlap, 2, keys, counts, "base")
    m = len(ref["out"])
    assert ref["stats"]["n_ins_long"] > 0

    def refused(k, c, code=1, **kw):
        s, nn, st, got = raw_consensus_ex(eng, pile, strings, overlap, 2, k, c, capacity=m, **kw)
        assert (s, nn) == (code, 0) and st == [0] * 8 and all(_cmarked(x) for x in got.values()), (s, nn, st, eng.lib.s2k_last_error(eng.ctx))

    swapped = keys.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    refused(swapped, counts)  # the keys do not ascend
    twice = keys.copy()
    twice[7] = twice[6]
    refused(twice, counts)  # not strictly
    for nf in (0, 1, 13):
        bad = keys.copy()
        bad[len(bad) // 2] = (int(bad[len(bad) // 2]) & ~(15 << 24)) | nf << 24
        refused(bad, counts)
    last = keys.copy()
    last[-1] = int(last[-1]) | 15 << 24  # the final key is checked too
    refused(last, counts)
    refused(keys, counts, n_bases=2 ** 36)
    device_consensus_long(eng, pile, strings, overlap, 2, keys, counts, "base again")


# ---- on a poisoned workspace -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_core_cases_on_a_poisoned_workspace():
    """S2K_POISON_WS is read once, in s2k_create: an engine of its own, made as tests/test_workspace_poison.py makes its engines"""
    os.environ["S2K_POISON_WS"] = "90"
    try:
        e = pkg.Engine(0)
    finally:
        del os.environ["S2K_POISON_WS"]
    try:
        for name, (c, want) in hand_cases().items():
            device_long(e, c, name)
        device_long(e, seam_case(np.random.default_rng(340), 2049, 65), "seam")
        clean, draft, n_st, c = _planted_inputs(6, b"AACGAA")
        c = ({f: c[0][f] for f in REC},) + c[1:]
        ref, _, keys = device_long(e, c, "planted")
        s, st, got, buf, nc, nk = raw_pileup_ex(e, *c, capacity=3)  # a refusal, then the base case
        assert s == 7
        device_long(e, c, "planted again")
        k, cnt = table_of(keys)
        got = device_consensus_long(e, ref, [draft], OV1, 3, k, cnt, "planted consensus")
        assert got["strings"][0] == clean
        bad = k.copy()
        bad[0] = int(bad[0]) | 15 << 24
        s, nn, st, _ = raw_consensus_ex(e, ref, [draft], OV1, 3, bad, cnt, capacity=len(clean))
        assert (s, nn) == (1, 0)
        device_consensus_long(e, ref, [draft], OV1, 3, k, cnt, "planted consensus again")
        tp.device_consensus(e, ref, [draft], OV1, 3, "old consensus")
    finally:
        e.close()


# ---- end to end through the Python API ---------------------------------------------------------------------------------------------------
def _api_objects(eng, draft, walks, reads):
    import torch

    T = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt).view({8: np.int64, 4: np.int32, 1: np.uint8}[np.dtype(dt).itemsize]).copy()).to("cuda:0")  # noqa: E731
    graph = types.SimpleNamespace(overlap=T(OV1, np.uint32))
    seqs = (T([0, len(draft)], np.uint64), T(np.frombuffer(draft, dtype=np.uint8), np.uint8))
    bases = T(np.frombuffer(b"".join(reads), dtype=np.uint8), np.uint8)
    read_off = T(np.concatenate([[0], np.cumsum([len(r) for r in reads])]), np.uint64)
    return graph, seqs, bases, read_off, T


def _api_walks(T, walks, a, b, su=SU1):
    w = types.SimpleNamespace(**{f: T(walks[f][a:b], walks[f].dtype) for f in REC + ("qstart", "qend")})
    w.walk_off = T(np.arange(b - a + 1), np.uint64)
    w.paths = types.SimpleNamespace(unitig=T(su, np.uint32))
    return w


def _api_run(eng, draft, walks, reads, cigars_of, tag):
    """two batches through UnitigGraph.pileup(long_ins=True) -> (polished, the references' consensus, n_long_keys); cigars_of(graph,
    walk namespace, bases, read_off, seqs, a, b) -> (WalkAlignments, the runs as lists)"""
    graph, seqs, bases, read_off, T = _api_objects(eng, draft, walks, reads)
    pl = pkg.UnitigGraph.pileup(graph, eng, seqs, long_ins=True)
    plain = pkg.UnitigGraph.pileup(graph, eng, seqs)
    h = len(reads) // 2
    all_runs = []
    try:
        for a, b in ((0, h), (h, len(reads))):
            w = _api_walks(T, walks, a, b)
            ro = read_off[a:b + 1] - read_off[a]
            bs = bases[int(read_off[a]):int(read_off[b])]
            al, runs = cigars_of(graph, w, bs, ro, seqs, a, b)
            all_runs += runs
            st = pl.add(eng, w, al, bs, ro)
            assert plain.add(eng, w, al, bs, ro) == st
        c = ({f: walks[f] for f in REC}, SU1, [draft], OV1, reads, [0] * len(reads), all_runs)
        ref_pile, ref_st = pileup_reference(*c)
        want, cand = long_keys_reference(*c)
        got = pl.host()
        assert all(got[f].tobytes() == ref_pile[f].tobytes() for f in PLANES) and pl.stats == ref_st, tag
        assert all(torch_equal(x, y) for x, y in zip(pl.planes, plain.planes))
        assert (pl.n_long_keys, pl.n_long_candidates) == (len(want), cand)
        k, cnt = table_of(want)
        assert pl.long_insertions() == sorted((decode(x)[0], decode(x)[1], int(y)) for x, y in zip(k, cnt)), tag
        pol = pl.consensus(eng, 3)
        keep = cnt >= 2
        ref = consensus_long_reference(ref_pile, [draft], OV1, 3, k[keep], cnt[keep])
        assert ref["stats"] == consensus_long_reference(ref_pile, [draft], OV1, 3, k, cnt)["stats"]  # the cutoff of min_cov // 2 + 1 changes nothing
        assert pol.stats == ref["stats"], (tag, pol.stats, ref["stats"])
        assert pol.sequences[1].cpu().numpy().tobytes() == ref["out"].tobytes() and pol.pos_map.cpu().numpy().view(np.uint64).tobytes() == ref["pos_map"].tobytes(), tag
        assert pol.sequences[0].cpu().numpy().view(np.uint64).tobytes() == ref["out_off"].tobytes()
        old = plain.consensus(eng, 3)
        assert old.stats == consensus_reference(ref_pile, [draft], OV1, 3)["stats"] and set(old.stats) == set(tp.C_STATS)
        return pol, ref, old
    finally:
        pl.close()
        assert pl.counter is None


def torch_equal(a, b):
    import torch

    return torch.equal(a, b)


@pytest.mark.gpu
def test_planted_stretches_end_to_end_hand_made_and_real_cigars(eng):
    import torch

    clean, draft, walks, reads, cigars, n_st = planted_long_case(2, b"AACGAA")

    def hand(graph, w, bs, ro, seqs, a, b):
        T = lambda x, dt: torch.from_numpy(np.asarray(x).astype(dt).view(np.int64 if dt == np.uint64 else np.int32).copy()).to("cuda:0")  # noqa: E731
        ops_off, n_ops, ops = tp.alignment_arrays([0] * (b - a), cigars[a:b], slack=False)
        z = torch.zeros(b - a, dtype=torch.int32, device="cuda:0")
        return pkg.WalkAlignments(z, z, T(n_ops, np.uint32), T(ops_off, np.uint64), T(ops, np.uint32), z), cigars[a:b]

    pol, ref, old = _api_run(eng, draft, walks, reads, hand, "hand-made")
    assert ref["strings"][0] == clean and pol.stats["n_ins_long"] == n_st and pol.stats["n_long"] == 0
    assert old.sequences[1].cpu().numpy().tobytes() != clean and old.stats["n_long"] > 0

    def real(graph, w, bs, ro, seqs, a, b):
        al = pkg.UnitigGraph.align(graph, eng, w, bs, ro, seqs)
        h = al.host()
        assert not h["flags"].any()
        return al, [[(int(x) >> 4, int(x) & 15) for x in h["ops"][int(h["ops_off"][i]):int(h["ops_off"][i]) + int(h["n_ops"][i])]] for i in range(b - a)]

    pol, ref, old = _api_run(eng, draft, walks, reads, real, "real aligner")
    # how often the unit-cost aligner keeps a planted stretch whole: a figure, not a bound
    same = sum(1 for j in range(n_st) if _stretch_restored(ref["strings"][0], clean, j))
    print("real aligner, AACGAA seed 2 spacing %d: %d of %d planted stretches restored (%d long insertions called, n_long %d, polished %s clean)" % (
        SPACING, same, n_st, pol.stats["n_ins_long"], pol.stats["n_long"], "==" if ref["strings"][0] == clean else "!="))


def _stretch_restored(got, clean, j, stretches=(2, 3, 7, 12)):
    """whether the polished string holds the clean bases round planted stretch j (12 bases to either side)"""
    a = SPACING * (j + 1)
    window = clean[a - 12:a + stretches[j % 4] + 12]
    return window in got
