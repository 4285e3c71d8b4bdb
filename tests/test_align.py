"""Read walks aligned to their paths: s2k_walks_targets and s2k_align_pairs (include/s2k.h), UnitigGraph.align,
WalkAlignments and the alignment columns of the GAF.  The references are `targets_reference` (built on test_walk.stitched_path),
`align_reference` (the header's rule on furthest-reaching points, restated serially) and `edit_distance_dp` (a plain two-row dynamic
program, the independent check); the device's arrays equal the references byte for byte, between guards."""
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
import test_lift as tl
import test_simplify as ts
import test_span as tsp
import test_thread as tt
import test_unitig_sequences as tus
import test_walk as twk
from test_bridge import noisy_case  # noqa: F401  (module-scoped fixtures of the repeat)
from test_span import repeat_case  # noqa: F401
from test_walk import repeat_walks  # noqa: F401

pkg = import_package()

SYMS = ("s2k_walks_targets", "s2k_align_pairs")
OVER, BAD_PATH = 1, 2
OPS = {1: "I", 2: "D", 7: "=", 8: "X"}
MAX_EDITS = 255
HAND_PAIRS = [(b"AAAA", b"AAA", "3=1I"), (b"AAA", b"AAAA", "3=1D"), (b"ACGT", b"AGGT", "1=1X2="), (b"", b"ACG", "3D"), (b"ACG", b"", "3I"),
              (b"ACGTACGT", b"ACGACGT", "3=1I4="), (b"GATTACA", b"GCATGCA", "1=1D2=1I1X2="), (b"", b"", "")]


# ---- the references ----------------------------------------------------------------------------------------------------------------
def _ext(q, t, i, k):
    m, n = len(q), len(t)
    while True:
        c = min(m - i, n - i - k, 64)
        if c <= 0:
            return i
        if q[i:i + c] == t[i + k:i + k + c]:
            i += c
            continue
        while q[i] == t[i + k]:
            i += 1
        return i


def _candidates(prev, k, m, n):
    """the kept candidates of (s, k) from row s - 1, in the order X, I, D: (value or None) * 3"""
    out = []
    for src, add in ((k, 1), (k + 1, 1), (k - 1, 0)):
        v = prev.get(src)
        if v is not None:
            v += add
            if not (v <= m and 0 <= v + k <= n):
                v = None
        out.append(v)
    return out


def align_reference(q, t, max_edits=MAX_EDITS):
    """the rule of include/s2k.h -> (edits, flags, runs [(len, op code)], matches); over: (max_edits + 1, OVER, [], 0)"""
    q, t = bytes(q), bytes(t)
    m, n = len(q), len(t)
    if abs(n - m) > max_edits:
        return max_edits + 1, OVER, [], 0
    H = [{0: _ext(q, t, 0, 0)}]
    while H[-1].get(n - m) != m:
        s = len(H)
        if s > max_edits:
            return max_edits + 1, OVER, [], 0
        row = {}
        for k in range(-s, s + 1):
            c = [v for v in _candidates(H[s - 1], k, m, n) if v is not None]
            if c:
                row[k] = _ext(q, t, max(c), k)
        H.append(row)
    s, k, i, back = len(H) - 1, n - m, m, []
    edits = s
    while True:
        c = _candidates(H[s - 1], k, m, n) if s else [0, None, None]
        v = max(x for x in c if x is not None)
        back += [7] * (i - v)
        i = v
        if s == 0:
            break
        if c[0] == v:
            back.append(8)
            i -= 1
        elif c[1] == v:
            back.append(1)
            i, k = i - 1, k + 1
        else:
            back.append(2)
            k -= 1
        s -= 1
    runs = []
    for op in reversed(back):
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return edits, 0, [(ln, op) for ln, op in runs], sum(ln for ln, op in runs if op == 7)


def cigar_of(runs):
    return "".join("%d%s" % (ln, OPS[op]) for ln, op in runs)


def edit_distance_dp(q, t):
    """unit-cost edit distance by two rows; a row's insertions by a running minimum (numpy)"""
    q, t = np.frombuffer(bytes(q), dtype=np.uint8), np.frombuffer(bytes(t), dtype=np.uint8)
    n = len(t)
    ar = np.arange(n + 1, dtype=np.int64)
    prev = ar.copy()
    for i in range(len(q)):
        cur = np.empty(n + 1, dtype=np.int64)
        cur[0] = i + 1
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (t != q[i]))
        prev = np.minimum.accumulate(cur - ar) + ar
    return int(prev[n])


def check_alignment(q, t, res, tag):
    """the runs consume both strings, = lies over equal bytes and X over unequal ones, the edits are the runs that are not =, and
    there are at most 2 edits + 1 runs"""
    edits, flags, runs, matches = res
    assert flags == 0, tag
    i = j = cost = 0
    for ln, op in runs:
        assert ln > 0, tag
        if op == 7:
            assert q[i:i + ln] == t[j:j + ln], tag
        elif op == 8:
            assert all(q[i + x] != t[j + x] for x in range(ln)), tag
        i += ln if op != 2 else 0
        j += ln if op != 1 else 0
        cost += ln if op != 7 else 0
    assert (i, j, cost) == (len(q), len(t), edits) and len(runs) <= 2 * edits + 1, (tag, i, j, cost, edits)
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])) and matches == sum(ln for ln, op in runs if op == 7), tag


def align_many_reference(pairs, max_edits=MAX_EDITS):
    """pairs [(q, t)] -> dict edits, flags, n_ops, matches (uint32), ops_off (uint64), and ops as a list of uint32 arrays per pair"""
    res = [align_reference(q, t, max_edits) for q, t in pairs]
    slots = [0 if r[1] else 2 * r[0] + 1 for r in res]
    return {"edits": np.array([r[0] for r in res], dtype=np.uint32), "flags": np.array([r[1] for r in res], dtype=np.uint32),
            "n_ops": np.array([len(r[2]) for r in res], dtype=np.uint32), "matches": np.array([r[3] for r in res], dtype=np.uint32),
            "ops_off": np.concatenate([[0], np.cumsum(slots)]).astype(np.uint64),
            "ops": [np.array([ln << 4 | op for ln, op in r[2]], dtype=np.uint32) for r in res], "res": res}


def targets_reference(walks, step_unitig, strings, overlap):
    """walks: the arrays of walks_reference; strings: the unitigs' bases -> (tgt_off uint64, tgt bytes, bad uint8) by the header's rule"""
    u = [int(x) for x in step_unitig]
    L = lambda U: len(strings[U >> 1])  # noqa: E731
    off, out, bad = [0], b"", []
    for w in range(len(walks["first_step"])):
        a, n = int(walks["first_step"][w]), int(walks["n_steps"][w])
        ps, pe, circ = int(walks["path_start"][w]), int(walks["path_end"][w]), int(walks["flags"][w]) & 1
        units = u[a:a + n]
        b = ps > pe
        piece = b""
        if circ:
            b = b or n == 0 or L(units[0]) == 0
            if not b:
                strand = twk.stitched_path(strings, overlap, units[:1])
                piece = bytes(strand[x % len(strand)] for x in range(ps, pe))
        else:
            b = b or any(int(overlap[units[j - 1]]) > min(L(units[j - 1]), L(units[j])) for j in range(1, n))
            if not b:
                path = twk.stitched_path(strings, overlap, units)
                b = pe > len(path)
                piece = path[ps:pe]
        bad.append(1 if b else 0)
        out += b"" if b else piece
        off.append(len(out))
    return np.array(off, dtype=np.uint64), out, np.array(bad, dtype=np.uint8)


def walk_alignments_reference(walks, step_unitig, strings, overlap, reads, max_edits=MAX_EDITS):
    """what UnitigGraph.align gives: a bad walk has flags BAD_PATH and no run (it is an empty pair: one slot), every other walk the
    alignment of read[qstart:qend] to its target"""
    toff, tgt, bad = targets_reference(walks, step_unitig, strings, overlap)
    wo = walks["walk_off"].astype(np.int64)
    pairs = []
    for r in range(len(wo) - 1):
        for w in range(wo[r], wo[r + 1]):
            q = b"" if bad[w] else reads[r][int(walks["qstart"][w]): int(walks["qend"][w])]
            pairs.append((q, tgt[int(toff[w]): int(toff[w + 1])]))
    ref = align_many_reference(pairs, max_edits)
    ref["flags"] = np.where(bad == 1, np.uint32(BAD_PATH), ref["flags"]).astype(np.uint32)
    ref.update(bad=bad, pairs=pairs)
    return ref


def host_alignments(ref):
    """the reference as the dict WalkAlignments.host() returns"""
    ops = np.zeros(int(ref["ops_off"][-1]), dtype=np.uint32)
    for i, o in enumerate(ref["ops"]):
        ops[int(ref["ops_off"][i]): int(ref["ops_off"][i]) + len(o)] = o
    return {"edits": ref["edits"], "flags": ref["flags"], "n_ops": ref["n_ops"], "matches": ref["matches"], "ops_off": ref["ops_off"], "ops": ops}


# ---- generators -------------------------------------------------------------------------------------------------------------------
def random_seq(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def mutated(rng, s, n_edits, alphabet=b"ACGT", kinds=(0, 1, 2)):
    """s with n_edits substitutions (0), insertions (1) and deletions (2) at random places"""
    x = bytearray(s)
    for _ in range(n_edits):
        kind = int(rng.choice(kinds))
        if kind == 0 and x:
            i = int(rng.integers(0, len(x)))
            x[i] = [c for c in alphabet if c != x[i]][int(rng.integers(0, len(alphabet) - 1))] if len(alphabet) > 1 else x[i]
        elif kind == 1:
            x.insert(int(rng.integers(0, len(x) + 1)), alphabet[int(rng.integers(0, len(alphabet)))])
        elif x:
            del x[int(rng.integers(0, len(x)))]
    return bytes(x)


def spaced(rng, d, kind, gap=24):
    """a pair at distance exactly d: d edits of one kind, gap bases apart (0: substitutions, 1: bases only q has, 2: bases only t has)"""
    q = bytearray(random_seq(rng, gap * (d + 1)))
    t = bytearray(q)
    for e in range(d, 0, -1):
        i = e * gap
        if kind == 0:
            t[i] = b"ACGT"[(b"ACGT".index(t[i]) + 1) % 4]
        elif kind == 1:
            del t[i]
        else:
            del q[i]
    return bytes(q), bytes(t)


def random_strings(rng, mo):
    """bytes for the unitigs of a decomposition whose lengths the member offsets give"""
    return [random_seq(rng, int(b - a)) for a, b in zip(mo["out_off"][:-1], mo["out_off"][1:])]


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert hasattr(pkg.Engine, "walks_targets") and hasattr(pkg.Engine, "align_pairs") and hasattr(pkg.UnitigGraph, "align")
    assert all(hasattr(pkg.WalkAlignments, f) for f in ("host", "cigar", "block_len", "n_over", "n_bad"))
    assert "alignments" in pkg.write_gaf_walks.__code__.co_varnames and "alignments" in pkg.ReadWalks.write_gaf.__code__.co_varnames


def test_layouts_and_constants_match_the_mirrors(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "align_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "align_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    A = pkg.AlignOut
    assert facts["sizeof.s2k_align_out"] == (ctypes.sizeof(A),)
    for f, t in A._fields_:
        assert facts["s2k_align_out." + f] == (getattr(A, f).offset, ctypes.sizeof(t)), f
    assert facts["S2K_ALIGN_OVER"] == (pkg.ALIGN_OVER,) == (OVER,) and facts["S2K_ALIGN_BAD_PATH"] == (pkg.ALIGN_BAD_PATH,) == (BAD_PATH,)
    assert facts["S2K_ALIGN_MAX_EDITS"] == (pkg.ALIGN_MAX_EDITS,) and pkg.ALIGN_MAX_EDITS >= 255 and facts["S2K_ALIGN_WAVES"] == (pkg.ALIGN_WAVES,)
    assert [facts["S2K_CIGAR_" + k] for k in ("I", "D", "EQ", "X")] == [(pkg.CIGAR_I,), (pkg.CIGAR_D,), (pkg.CIGAR_EQ,), (pkg.CIGAR_X,)] == [(1,), (2,), (7,), (8,)]


def test_cpp_align_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "align_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "align_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_new_source_is_in_the_build():
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "s2k_align.hip" in next(line for line in mk.split("\n") if line.startswith("SRCS"))
    assert "s2k_align.hip" in next(line for line in open(os.path.join(csrc, "Makefile.asan")).read().split("\n") if line.startswith("ASAN_SRCS"))


def test_reference_equals_the_plain_dp_on_random_pairs():
    rng = np.random.default_rng(70)
    seen = 0
    for alphabet in (b"A", b"AC", b"ACGT", b"ACGTN"):
        for _ in range(800):
            q = random_seq(rng, int(rng.integers(0, 40)), alphabet)
            t = mutated(rng, q, int(rng.integers(0, 8)), alphabet) if rng.random() < 0.7 else random_seq(rng, int(rng.integers(0, 40)), alphabet)
            res = align_reference(q, t)
            assert res[0] == edit_distance_dp(q, t), (q, t)
            check_alignment(q, t, res, (q, t))
            seen += res[0] > 0
    assert seen > 1500


def test_reference_hand_cases():
    for q, t, want in HAND_PAIRS:
        res = align_reference(q, t)
        assert cigar_of(res[2]) == want and res[0] == edit_distance_dp(q, t), (q, t, cigar_of(res[2]))
        check_alignment(q, t, res, (q, t))
    assert align_reference(b"AAAA", b"TTTT", 4) == (4, 0, [(4, 8)], 0)
    assert align_reference(b"AAAA", b"TTTT", 3) == (4, OVER, [], 0)
    assert align_reference(b"A" * 10, b"A" * 4, 5) == (6, OVER, [], 0) and align_reference(b"A" * 10, b"A" * 4, 6)[0] == 6
    assert align_reference(b"ACGN", b"ACGN")[:2] == (0, 0) and align_reference(b"acgt", b"ACGT")[0] == 4  # bytes as they are


def hand_targets():
    uni, ro, d, nodes, mo = twk.walk_hand()
    paths = twk.walk_paths_of(list(twk.W_READS.values()))
    walks = twk.walks_reference(paths, ro, d, uni, mo, nodes["seq_len"])
    strings = random_strings(np.random.default_rng(71), mo)
    return walks, paths, strings, mo


def test_targets_reference_hand_graphs():
    walks, paths, strings, mo = hand_targets()
    toff, tgt, bad = targets_reference(walks, paths["unitig"], strings, mo["overlap"])
    assert not bad.any() and (np.diff(toff.astype(np.int64)) == (walks["path_end"] - walks["path_start"]).astype(np.int64)).all()
    u = paths["unitig"].tolist()
    seen_twin = seen_round = 0
    for w in range(walks["n_walks"]):
        a, n, ps, pe = (int(walks[f][w]) for f in ("first_step", "n_steps", "path_start", "path_end"))
        strand = strings[u[a] >> 1] if u[a] % 2 == 0 else tus.revcomp(strings[u[a] >> 1])
        got = tgt[int(toff[w]): int(toff[w + 1])]
        if walks["flags"][w] & 1:  # the circular unitig walked round: path_end 32 on L = 10, and its twin strand
            assert n == 1 and got == (strand * 4)[ps:pe], w
            seen_round += pe > 3 * len(strand)
        else:
            assert got == twk.stitched_path(strings, mo["overlap"], u[a:a + n])[ps:pe], w
            if n == 1:
                assert got == strand[ps:pe], w
        seen_twin += u[a] & 1
    assert seen_twin >= 2 and seen_round == 1 and int(walks["path_end"].max()) == 32 and len(strings[3]) == 10


def junction_case():
    """two unitigs of 10 and 5 bases: the overlap that leaves 0+ is 7 > min(10, 5), the one that leaves 1- is 3"""
    strings = [b"ACGTACGTAC", b"GGATC"]
    overlap = np.array([7, 0, 0, 3], dtype=np.uint32)
    walks = {"first_step": np.array([0, 2, 4, 5], dtype=np.uint64), "n_steps": np.array([2, 2, 1, 1], dtype=np.uint32),
             "path_start": np.array([0, 1, 2, 4], dtype=np.uint64), "path_end": np.array([8, 11, 11, 3], dtype=np.uint64),
             "flags": np.zeros(4, dtype=np.uint32), "walk_off": np.array([0, 4], dtype=np.uint64)}
    return walks, np.array([0, 2, 3, 1, 0, 1], dtype=np.uint32), strings, overlap


def test_targets_reference_bad_walks():
    walks, su, strings, overlap = junction_case()
    toff, tgt, bad = targets_reference(walks, su, strings, overlap)
    # a junction above a length; a sound two-step walk on twin strands; path_end past the stitched length; path_start > path_end
    assert bad.tolist() == [1, 0, 1, 1] and toff.tolist() == [0, 0, 10, 10, 10]
    assert tgt == (tus.revcomp(strings[1]) + tus.revcomp(strings[0])[3:])[1:11]


def _clean_walk_alignments(k, reads):
    ref = twk.reference_of(k)
    return ref, walk_alignments_reference(ref, k["paths"]["unitig"], k["strings"], k["overlap"], reads)


def test_repeat_fixture_clean_reads_align_without_edits(repeat_walks):
    rw = repeat_walks
    for tag in ("before", "after"):
        walks, al = _clean_walk_alignments(rw[tag], rw["reads"])
        n = (walks["qend"] - walks["qstart"]).astype(np.int64)
        assert not al["flags"].any() and not al["edits"].any() and al["matches"].tolist() == n.tolist(), tag
        assert [cigar_of(r[2]) for r in al["res"]] == ["%d=" % x for x in n], tag


@pytest.fixture(scope="module")
def noisy_walks(repeat_case, noisy_case, repeat_walks, oracle, ecoli):
    """the repeat reads with 1 % substitutions (seed 2), bridged (16, 2) by the reference: their walks on the unitig graph, and, lifted,
    on the contigs"""
    c, n, rw = repeat_case, noisy_case, repeat_walks
    bridged = tb.reference_of(n)
    paths = {f: bridged[f] for f in tl.STEP + ("path_off",)}
    before = dict(rw["before"], paths=paths)
    lifted = tl.lift_reference(tl._repeat_lift_case(c, oracle, ecoli, paths, bridged["matched"]))
    after = dict(rw["after"], paths={f: lifted[f] for f in tl.STEP + ("path_off",)})
    return {"reads": n["reads"], "before": before, "after": after}


def test_repeat_fixture_noisy_reads_align_as_the_plain_dp_says(noisy_walks):
    nw = noisy_walks
    for tag in ("before", "after"):
        walks, al = _clean_walk_alignments(nw[tag], nw["reads"])
        assert not al["flags"].any(), (tag, al["flags"].tolist())  # none over at 255, none bad
        for (q, t), res in zip(al["pairs"], al["res"]):
            check_alignment(q, t, res, tag)
            assert res[0] == edit_distance_dp(q, t), tag
        print("noisy repeat reads %s untangling: %d walks, %d edits in all, %d bases aligned" % (
            tag, walks["n_walks"], int(al["edits"].sum()), int(al["matches"].sum())))
        assert int(al["edits"].sum()) > 100


G_WALKS = {"walk_off": [0, 1, 3], "first_step": [0, 1, 3], "n_steps": [1, 2, 1], "items": [2, 5, 3], "qstart": [5, 0, 40], "qend": [31, 28, 68],
           "path_len": [16, 25, 10], "path_start": [3, 0, 3], "path_end": [16, 25, 32], "flags": [0, 0, 1]}
G_ALIGN = {"edits": [2, 300, 0], "flags": [0, OVER, 0], "n_ops": [4, 0, 1], "matches": [11, 0, 28], "ops_off": [0, 5, 5, 6],
           "ops": [11 << 4 | 7, 1 << 4 | 8, 13 << 4 | 1, 1 << 4 | 2, 0x5A5A, 28 << 4 | 7]}
G_GAF = """\
r0\t90\t5\t31\t+\t>1\t16\t3\t16\t11\t26\t255\tkm:i:2\tns:i:1\tNM:i:2\tcg:Z:11=1X13I1D
r1\t91\t0\t28\t+\t>0<1\t25\t0\t25\t5\t28\t255\tkm:i:5\tns:i:2
r1\t91\t40\t68\t+\t>3\t10\t3\t32\t28\t28\t255\tkm:i:3\tns:i:1\tNM:i:0\tcg:Z:28=
"""


def test_gaf_text_with_alignments(tmp_path):
    walks = {f: np.array(v, dtype=twk.WALK_DT[f]) for f, v in G_WALKS.items()}
    al = {f: np.array(v, dtype=np.uint64 if f == "ops_off" else np.uint32) for f, v in G_ALIGN.items()}
    su = np.array([2, 0, 3, 6], dtype=np.uint32)
    kw = dict(names=["r0", "r1"], read_lengths=[90, 91])
    p = str(tmp_path / "a.gaf")
    pkg.write_gaf_walks(p, walks, su, alignments=al, **kw)
    assert open(p).read() == G_GAF
    plain = twk.gaf_text(tmp_path, walks, {"unitig": su}, **kw)
    assert plain.split("\n")[1] == G_GAF.split("\n")[1]  # the flagged walk keeps its line
    pkg.write_gaf_walks(p, walks, su, alignments=None, **kw)
    assert open(p).read() == plain and "cg:Z" not in plain
    uni, ro, d, nodes, mo = twk.walk_hand()  # and on the hand graph of test_walk.py: None changes nothing
    paths = twk.walk_paths_of(list(twk.W_READS.values()))
    ref = twk.walks_reference(paths, ro, d, uni, mo, nodes["seq_len"])
    pkg.write_gaf_walks(p, ref, paths["unitig"], first_read=5, alignments=None)
    assert open(p).read() == twk.W_GAF
    assert pkg.alignment_block_len(al["ops_off"], al["n_ops"], al["ops"]).tolist() == [26, 0, 28] and pkg.cigar_string(al["ops"][:4]) == "11=1X13I1D"


@pytest.fixture(scope="module")
def ecoli_reference(oracle, ecoli):
    """the 600 E. coli reads with 0.5 % substitutions through simplify(10, 20) and bridge(16, 2) by the references (Regular 12 / 5): the
    walks, the unitig strings, the alignments"""
    mode, l, k = tsp.MODES[0]
    mc = 2
    reads = ts.sample_reads_with_errors(ecoli, 600, 7, 0.005)
    b = tus._oracle_batch(oracle, reads, l, k, 0.05, mode)
    full = tg.graph_reference([b], mc, 1)
    final, ref_map, _ = ts.simplify_rounds_reference(full, 10, 20)
    uni, uro, ud, _ = ts.unitig_view(final)
    paths = tt.thread_reference(b["km_off"], b["hash"], b["rev"], final["keys"], final["counts"], mc, tt.places_reference(uni), start=b["start"],
                                end=b["end"], n_unitigs=uni["n_unitigs"])
    br = tb.bridge_reference(paths, uro, ud, uni["uni_off"], uni["circular"], *tb.DEFAULT)
    bpaths = {f: br[f] for f in tb.STEP + ("path_off",)}
    all_nodes = tus.node_sequences_reference([b], full["keys"], k)
    kept = np.nonzero(ref_map >= 0)[0]
    nodes = {f: np.asarray(all_nodes[f])[kept] for f in ("rep", "seq_off", "seq_len", "shift_fwd", "shift_rev", "rev")}
    nodes["pool"] = all_nodes["pool"]
    seqs = tus.unitig_sequences_reference(uni, nodes)
    case = {"paths": bpaths, "ro": uro, "d": ud, "uni": uni, "nodes": nodes, "mo": twk.member_offsets_reference(uni, nodes)}
    walks = twk.reference_of(case)
    strings = tus.unitig_strings(uni, seqs)
    al = walk_alignments_reference(walks, bpaths["unitig"], strings, seqs["overlap"], reads)
    return {"reads": reads, "walks": walks, "paths": bpaths, "strings": strings, "overlap": seqs["overlap"], "al": al}


def test_ecoli_reads_with_errors_none_over_none_bad_by_the_references(ecoli_reference):
    """a condition on the input: the device test cannot hide a failure behind flags.  About 40 edits per walk of a whole read: two
    strings with 0.5 % substitutions each"""
    e = ecoli_reference
    al, n = e["al"], e["walks"]["n_walks"]
    n_over, n_bad = int((al["flags"] & OVER != 0).sum()), int((al["flags"] & BAD_PATH != 0).sum())
    print("E. coli, 600 reads with errors: %d walks, %d over at 255, %d bad, %d edits in all, %.1f per walk, the largest %d" % (
        n, n_over, n_bad, int(al["edits"].sum()), al["edits"].sum() / max(n, 1), int(al["edits"].max())))
    assert n >= 600 and n_over == 0 and n_bad == 0
    assert int((al["flags"] == 0).sum()) >= 0.95 * n
    for i in range(0, n, 37):
        check_alignment(al["pairs"][i][0], al["pairs"][i][1], al["res"][i], i)


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


GUARD = 8
_dev, _host, _ptr = ts._dev, ts._host, ts._ptr
A32 = ("edits", "flags", "n_ops", "matches", "ops")
A_DT = dict({f: np.uint32 for f in A32}, ops_off=np.uint64)
TDT = {np.uint64: "int64", np.uint32: "int32", np.uint8: "uint8"}
FILL = {np.uint64: -0x5A5A, np.uint32: -0x5A5A, np.uint8: 0xA5}


def _marked(h, frm=0, to=None):
    dt = h.dtype.type
    return bool((h[frm:to] == np.array(FILL[dt]).astype({np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}[dt]).view(dt)).all())


def _full(n, dt):
    import torch

    return torch.full((n + GUARD,), FILL[dt], dtype=getattr(torch, TDT[dt]), device="cuda:0")


def pools_of(pairs, q_at=None, t_at=None, q_tail=3, t_tail=5):
    """the pairs laid out in two pools of junk: pair i's query starts at the next position that is q_at[i] mod 8 (t_at likewise; the
    next free byte when None); *_tail junk bytes behind the last interval -> (query, target, four interval arrays)"""
    rng = np.random.default_rng(len(pairs))
    pools, ivs = [], []
    for which, at, tail in ((0, q_at, q_tail), (1, t_at, t_tail)):
        buf, b, e = bytearray(), [], []
        for i, p in enumerate(pairs):
            if at is not None:
                buf += random_seq(rng, (at[i] - len(buf)) % 8, b"acgtn")
            b.append(len(buf))
            buf += p[which]
            e.append(len(buf))
            buf += random_seq(rng, 1, b"acgtn") if at is None and i % 3 == 0 else b""
        buf += random_seq(rng, tail, b"acgtn")
        pools.append(np.frombuffer(bytes(buf), dtype=np.uint8))
        ivs += [np.array(b, dtype=np.uint64), np.array(e, dtype=np.uint64)]
    return pools[0], pools[1], ivs


def raw_align(eng, q, t, ivs, max_edits=MAX_EDITS, capacity=None, want=A32 + ("ops_off",), ctx=True, out=True, n_pairs=None, nq=None, nt=None, null=()):
    """s2k_align_pairs through ctypes, guard words behind every output -> (status, n_ops_bound, host arrays with guards)"""
    import torch

    real = len(ivs[0])  # the outputs are sized by the pairs there are; an overridden n_pairs goes to the call alone
    n = real if n_pairs is None else n_pairs
    assert n <= real or n >= 2 ** 32, "an n_pairs above the arrays is only for the refusal the host decides"
    dq, dt = _dev(q, np.uint8), _dev(t, np.uint8)
    div = [_dev(x, np.uint64) for x in ivs]
    cap = int(capacity if capacity is not None else 0)
    size = {f: max(real, 1) for f in A32}
    size.update(ops_off=real + 1, ops=max(cap, 1))
    res = {f: _full(size[f], A_DT[f]) for f in want}
    o = pkg.AlignOut()
    o.capacity = cap
    for f, x in res.items():
        setattr(o, f, x.data_ptr())
    nb = ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_align_pairs(eng.ctx if ctx else None, _ptr(dq, "q" in null), len(q) if nq is None else nq, _ptr(dt, "t" in null),
                                len(t) if nt is None else nt, *(_ptr(x, i in null) for i, x in enumerate(div)), n, max_edits,
                                ctypes.byref(o) if out else None, ctypes.byref(nb))
    return s, nb.value, {f: _host(x, A_DT[f]) for f, x in res.items()}


def assert_aligned(got, ref, n, tag):
    """every array equal to the reference, the guards intact, and every slot behind a pair's runs untouched"""
    for f in ("edits", "flags", "n_ops", "matches"):
        assert got[f][:n].tobytes() == ref[f].tobytes(), (tag, f, got[f][:8], ref[f][:8])
        assert _marked(got[f], n), (tag, f, "guard")
    assert got["ops_off"][:n + 1].tobytes() == ref["ops_off"].tobytes() and _marked(got["ops_off"], n + 1), (tag, "ops_off")
    off = ref["ops_off"].astype(np.int64)
    for i in range(n):
        k = len(ref["ops"][i])
        assert got["ops"][off[i]: off[i] + k].tobytes() == ref["ops"][i].tobytes(), (tag, i, "ops")
        assert _marked(got["ops"], off[i] + k, off[i + 1]), (tag, i, "slots behind the runs")
    assert _marked(got["ops"], off[n]), (tag, "ops guard")


def device_align(eng, pairs, tag, max_edits=MAX_EDITS, **layout):
    """the two calls against the reference: the sizes-only call, the writing call, capacity one short -> the reference"""
    ref = align_many_reference(pairs, max_edits)
    q, t, ivs = pools_of(pairs, **layout)
    n, bound = len(pairs), int(ref["ops_off"][-1])
    s, nb, got = raw_align(eng, q, t, ivs, max_edits, want=("edits", "flags", "ops_off"))
    assert (s, nb) == (0, bound), (tag, "sizes", s, nb, bound)
    for f in got:
        assert got[f][:len(ref[f])].tobytes() == ref[f].tobytes() and _marked(got[f], len(ref[f])), (tag, "sizes", f)
    s, nb, got = raw_align(eng, q, t, ivs, max_edits, capacity=bound)
    assert (s, nb) == (0, bound), (tag, s, nb, bound)
    assert_aligned(got, ref, n, tag)
    if bound:
        s, nb, got = raw_align(eng, q, t, ivs, max_edits, capacity=bound - 1)
        assert (s, nb) == (7, bound) and all(_marked(x) for x in got.values()), (tag, "capacity")
    return ref


@pytest.mark.gpu
def test_device_pairs_hand_cases(eng):
    ref = device_align(eng, [(q, t) for q, t, _ in HAND_PAIRS], "hand")
    assert [cigar_of(r[2]) for r in ref["res"]] == [c for _, _, c in HAND_PAIRS]
    for q, t, c in HAND_PAIRS:  # every pair alone
        device_align(eng, [(q, t)], c)
    for me, want in ((4, "4X"), (3, "")):
        ref = device_align(eng, [(b"AAAA", b"TTTT")], ("max_edits", me), max_edits=me)
        assert cigar_of(ref["res"][0][2]) == want and ref["flags"].tolist() == [0 if want else OVER]
    assert device_align(eng, [(b"ACGN", b"ACGN"), (b"acgt", b"ACGT")], "bytes as they are")["edits"].tolist() == [0, 4]


@pytest.mark.gpu
def test_device_pairs_lengths_offsets_and_ends(eng):
    """interval lengths round one and two 8-byte words and a wave, at every offset from an 8-byte boundary in both pools, the first
    mismatch in each of the last 8 bytes, and the last pair ending on both pools' last byte"""
    rng = np.random.default_rng(72)
    pairs, q_at, t_at = [], [], []
    for L in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65):
        for a in range(8):
            for b in range(8):
                q = random_seq(rng, L)
                t = bytearray(q)
                j = (a * 8 + b) % 9  # 8: no mismatch; else the first mismatch j bytes before the end, and more behind it at random
                if j < 8 and L - 1 - j >= 0:
                    t[L - 1 - j] ^= 0x20
                    for x in range(L - j, L):
                        t[x] ^= 0x20 * int(rng.integers(0, 2))
                pairs.append((q, bytes(t)))
                q_at.append(a)
                t_at.append(b)
    device_align(eng, pairs, "offsets", q_at=q_at, t_at=t_at, q_tail=0, t_tail=0)
    device_align(eng, pairs[-70:], "offsets, junk behind", q_at=q_at[-70:], t_at=t_at[-70:], q_tail=1, t_tail=7)
    device_align(eng, [(p[0], p[1] + b"G") for p in pairs[-128:]], "one more base", q_at=t_at[-128:], t_at=q_at[-128:], q_tail=0, t_tail=0)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [31, 32, 33, 63, 64, 65])
def test_device_pairs_wavefront_widths(eng, d):
    """distances that put the 2 s + 1 diagonals of a wavefront at and across 63 / 65 and 127 / 129, with the goal diagonal in the middle
    (substitutions) and at either edge (bases only one side has)"""
    rng = np.random.default_rng(d)
    pairs = [spaced(rng, d, kind) for kind in (0, 1, 2)] + [(random_seq(rng, 3 * d), b"")]
    pairs.append((mutated(rng, pairs[0][0], d), pairs[0][0]))
    ref = device_align(eng, pairs, ("distance", d))
    assert ref["edits"][:4].tolist() == [d, d, d, 3 * d] and [edit_distance_dp(*p) for p in pairs[:3]] == [d, d, d]
    check_alignment(pairs[4][0], pairs[4][1], ref["res"][4], d)


@pytest.mark.gpu
def test_device_pairs_at_and_over_max_edits(eng):
    rng = np.random.default_rng(73)
    for me in (0, 5, 64, MAX_EDITS):
        at, over = spaced(rng, me, 0, gap=9), spaced(rng, me + 1, 0, gap=9)
        far = (random_seq(rng, 10), random_seq(rng, 10 + me + 1))  # decided by the lengths alone
        pairs = [at, over, at, far, (b"ACGT", b"ACGT"), over]
        ref = device_align(eng, pairs, ("max_edits", me), max_edits=me)
        assert ref["flags"].tolist() == [0, OVER, 0, OVER, 0, OVER] and ref["edits"].tolist() == [me, me + 1, me, me + 1, 0, me + 1]
        assert ref["n_ops"][[1, 3, 5]].tolist() == [0, 0, 0] and np.diff(ref["ops_off"].astype(np.int64))[[1, 3, 5]].tolist() == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2 * pkg.ALIGN_WAVES + 1])
def test_device_pairs_counts_round_a_wave_and_past_the_grid(eng, n):
    """tiny pairs, more of them than the persistent grid has waves: every wave takes another pair"""
    rng = np.random.default_rng(n)
    pairs = []
    for _ in range(n):
        q = random_seq(rng, int(rng.integers(0, 12)))
        pairs.append((q, mutated(rng, q, int(rng.integers(0, 3)))))
    device_align(eng, pairs, ("pairs", n), max_edits=3 if n > 65 else MAX_EDITS)


@pytest.mark.gpu
def test_device_pairs_one_long_pair(eng):
    rng = np.random.default_rng(74)
    q = random_seq(rng, 20000)
    t = mutated(rng, q, 150)
    ref = device_align(eng, [(q, t)], "20 000 bases")
    check_alignment(q, t, ref["res"][0], "long")
    assert 100 < ref["edits"][0] <= 150


@pytest.mark.gpu
def test_device_pairs_refusals_sizes_and_null_outputs(eng):
    rng = np.random.default_rng(75)
    pairs = [(random_seq(rng, 30), random_seq(rng, 33)) for _ in range(70)]
    q, t, ivs = pools_of(pairs)
    ref = device_align(eng, pairs, "base")
    n, bound = len(pairs), int(ref["ops_off"][-1])

    def refused(code=1, bound_out=0, **kw):
        kw.setdefault("capacity", bound)
        s, nb, got = raw_align(eng, q, t, kw.pop("ivs", ivs), **kw)
        assert (s, nb) == (code, bound_out) and all(_marked(x) for x in got.values()), (s, nb, list(kw))

    def changed(which, i, v):
        x = [a.copy() for a in ivs]
        x[which][i] = v
        return x

    refused(ctx=False)
    for i in range(4):
        refused(null=(i,))
    refused(null=("q",))
    refused(null=("t",))
    refused(ivs=changed(0, 5, int(ivs[1][5]) + 1))  # a begin above its end
    refused(ivs=changed(3, n - 1, len(t) + 1))  # past the pool's end
    refused(ivs=changed(1, 7, 2 ** 40))
    refused(nq=int(ivs[1][-1]) - 1)  # the pool ends inside the last interval
    refused(ivs=changed(1, 0, int(ivs[0][0]) + 2 ** 31), nq=2 ** 32)  # an interval of 2^31 bytes: refused before a byte is read
    refused(max_edits=pkg.ALIGN_MAX_EDITS + 1)
    refused(n_pairs=2 ** 32)
    for f in ("edits", "flags", "ops_off"):  # the writing call reads them back
        refused(want=tuple(x for x in A32 + ("ops_off",) if x != f))
    refused(code=7, bound_out=bound, capacity=bound - 1)
    # the sizes: out NULL, or no run array; every subset of the other outputs
    s, nb, got = raw_align(eng, q, t, ivs, out=False)
    assert (s, nb) == (0, bound) and all(_marked(x) for x in got.values())
    for want in ((), ("edits",), ("ops_off",), ("flags", "ops_off")):
        s, nb, got = raw_align(eng, q, t, ivs, want=want)
        assert (s, nb) == (0, bound) and all(got[f][:len(ref[f])].tobytes() == ref[f].tobytes() and _marked(got[f], len(ref[f])) for f in got), want
    for want in (("n_ops",), ("matches", "ops"), ("ops",)):  # some of the run outputs
        s, nb, got = raw_align(eng, q, t, ivs, want=want + ("edits", "flags", "ops_off"), capacity=bound)
        assert (s, nb) == (0, bound)
        for f in ("n_ops", "matches"):
            assert f not in got or (got[f][:n].tobytes() == ref[f].tobytes() and _marked(got[f], n)), f
        assert "ops" not in got or got["ops"][:3].tobytes() == ref["ops"][0][:3].tobytes()
    s, nb, got = raw_align(eng, q, t, ivs, n_pairs=0, capacity=4)  # no pairs: nothing is read
    assert (s, nb) == (0, 0) and got["ops_off"][0] == 0 and _marked(got["ops_off"], 1) and all(_marked(got[f]) for f in A32)


@pytest.mark.gpu
def test_device_pairs_deterministic(eng):
    rng = np.random.default_rng(76)
    pairs = []
    for _ in range(3000):
        q = random_seq(rng, int(rng.integers(0, 300)))
        pairs.append((q, mutated(rng, q, int(rng.integers(0, 12)))))
    q, t, ivs = pools_of(pairs)
    runs = []
    for _ in range(2):
        s, nb, got = raw_align(eng, q, t, ivs, capacity=3000 * 25)
        assert s == 0 and 3000 < nb <= 3000 * 25
        runs.append(b"".join(got[f].tobytes() for f in sorted(got)))
    assert runs[0] == runs[1]


T_DT = {"tgt_off": np.uint64, "tgt": np.uint8, "bad": np.uint8}


def raw_targets(eng, walks, su, strings, overlap, capacity=None, want=("tgt_off", "tgt", "bad"), ctx=True, null=(), **over):
    """s2k_walks_targets through ctypes, guards behind every output -> (status, n_bytes, host arrays with guards).  over: first_step,
    n_steps, path_start, path_end, flags, unitig, out_off, overlap replaced; n_walks, n_steps_all, T, n_bases given"""
    import torch

    out_off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint64)
    out = np.frombuffer(b"".join(strings), dtype=np.uint8)
    arr = {"first_step": (walks["first_step"], np.uint64), "n_steps": (walks["n_steps"], np.uint32), "path_start": (walks["path_start"], np.uint64),
           "path_end": (walks["path_end"], np.uint64), "flags": (walks["flags"], np.uint32), "unitig": (su, np.uint32), "out_off": (out_off, np.uint64),
           "out": (out, np.uint8), "overlap": (overlap, np.uint32)}
    dv = {k: _dev(over.get(k, a), dt) for k, (a, dt) in arr.items()}
    nw, ns = over.get("n_walks", len(walks["first_step"])), over.get("n_steps_all", len(su))
    T, nb_in = over.get("T", len(strings)), over.get("n_bases", len(out))
    cap = int(capacity if capacity is not None else 0)
    size = {"tgt_off": nw + 1, "tgt": max(cap, 1) + 15, "bad": max(nw, 1)}
    res = {f: _full(size[f], T_DT[f]) for f in want}
    nbytes = ctypes.c_uint64(777)
    torch.cuda.synchronize()
    P = lambda k: _ptr(dv[k], k in null)  # noqa: E731
    R = lambda f: _ptr(res[f]) if f in res else None  # noqa: E731
    s = eng.lib.s2k_walks_targets(eng.ctx if ctx else None, nw, P("first_step"), P("n_steps"), P("path_start"), P("path_end"), P("flags"), P("unitig"), ns,
                                  P("out_off"), P("out"), nb_in, P("overlap"), T, R("tgt_off"), R("tgt"), R("bad"), cap, ctypes.byref(nbytes))
    return s, nbytes.value, {f: _host(x, T_DT[f]) for f, x in res.items()}


def device_targets(eng, walks, su, strings, overlap, tag):
    toff, tgt, bad = targets_reference(walks, su, strings, overlap)
    nw, n = len(bad), len(tgt)
    s, nb, got = raw_targets(eng, walks, su, strings, overlap, want=("tgt_off", "bad"))
    assert (s, nb) == (0, n), (tag, "sizes", s, nb, n)
    assert got["tgt_off"][:nw + 1].tobytes() == toff.tobytes() and got["bad"][:nw].tobytes() == bad.tobytes(), (tag, "sizes")
    s, nb, got = raw_targets(eng, walks, su, strings, overlap, want=())
    assert (s, nb) == (0, n), (tag, "all NULL")
    s, nb, got = raw_targets(eng, walks, su, strings, overlap, capacity=n)
    assert (s, nb) == (0, n), (tag, s, nb, n)
    assert got["tgt_off"][:nw + 1].tobytes() == toff.tobytes() and _marked(got["tgt_off"], nw + 1), (tag, "tgt_off")
    assert got["bad"][:nw].tobytes() == bad.tobytes() and (nw == 0 or _marked(got["bad"], nw)), (tag, "bad")
    if got["tgt"][:n].tobytes() != tgt:
        x = next(i for i in range(n) if got["tgt"][i] != tgt[i])
        raise AssertionError((tag, "tgt differs from byte", x, "of", n, "walk", int(np.searchsorted(toff, x, side="right")) - 1))
    assert _marked(got["tgt"], n), (tag, "tgt guard")
    if n:
        s, nb, got = raw_targets(eng, walks, su, strings, overlap, capacity=n - 1)
        assert (s, nb) == (7, n) and all(_marked(x) for x in got.values()), (tag, "capacity")
    return toff, tgt, bad


def _case_targets(eng, case, seed, tag, n_walks=None):
    walks = twk.reference_of(case)
    if n_walks is not None:
        assert walks["n_walks"] >= n_walks
        walks = {f: (v[:n_walks] if f in twk.REC64 + twk.REC32 else v) for f, v in walks.items()}
    strings = random_strings(np.random.default_rng(seed), case["mo"])
    return walks, device_targets(eng, walks, case["paths"]["unitig"], strings, case["mo"]["overlap"], tag)


@pytest.mark.gpu
def test_device_targets_hand_graphs(eng):
    walks, paths, strings, mo = hand_targets()
    toff, tgt, bad = device_targets(eng, walks, paths["unitig"], strings, mo["overlap"], "hand")
    assert not bad.any() and len(tgt) == int((walks["path_end"] - walks["path_start"]).sum())
    for w in range(walks["n_walks"]):  # every walk alone
        one = {f: walks[f][w:w + 1] for f in ("first_step", "n_steps", "path_start", "path_end", "flags")}
        device_targets(eng, one, paths["unitig"], strings, mo["overlap"], ("hand", w))
    none = {f: walks[f][:0] for f in ("first_step", "n_steps", "path_start", "path_end", "flags")}
    assert device_targets(eng, none, paths["unitig"], strings, mo["overlap"], "no walks")[0].tolist() == [0]
    walks, su, strings, overlap = junction_case()
    assert device_targets(eng, walks, su, strings, overlap, "junction")[2].tolist() == [1, 0, 1, 1]
    circ = dict(walks, flags=np.ones(4, dtype=np.uint32), path_end=np.array([8, 11, 47, 3], dtype=np.uint64))
    assert device_targets(eng, circ, su, strings, overlap, "circular")[2].tolist() == [0, 0, 0, 1]
    assert device_targets(eng, circ, su, [b"", b"GGATC"], np.zeros(4, dtype=np.uint32), "circular, L = 0")[2].tolist() == [1, 0, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("n_walks", [63, 64, 65])
def test_device_targets_walk_counts(eng, n_walks):
    rng = np.random.default_rng(700 + n_walks)
    case = twk.chained_case(rng, 40, list(rng.integers(1, 9, size=90)), p_break=0.1)
    walks, (toff, tgt, bad) = _case_targets(eng, case, n_walks, ("walks", n_walks), n_walks=n_walks)
    assert len(bad) == n_walks and int(walks["n_steps"].max()) > 2


@pytest.mark.gpu
def test_device_targets_lengths_round_a_store_and_a_block(eng):
    """one unitig of 9 000 bases and its twin strand: targets of 15 / 16 / 17 and 4 095 / 4 096 / 4 097 bytes from odd starts, so that
    a target's end falls before, on and behind a 16-byte store and a 4 KiB block"""
    rng = np.random.default_rng(77)
    strings = [random_seq(rng, 9000), random_seq(rng, 40)]
    for lens in ([15, 16, 17], [4095, 4096, 4097], [16, 4096, 15, 4097, 1, 0, 17, 4095]):
        n = len(lens)
        starts = rng.integers(0, 4000, size=n)
        walks = {"first_step": (np.arange(n) % 2).astype(np.uint64), "n_steps": np.ones(n, dtype=np.uint32), "path_start": starts.astype(np.uint64),
                 "path_end": (starts + np.array(lens)).astype(np.uint64), "flags": np.zeros(n, dtype=np.uint32)}
        device_targets(eng, walks, np.array([0, 1], dtype=np.uint32), strings, np.zeros(4, dtype=np.uint32), lens)


@pytest.mark.gpu
def test_device_targets_walk_of_many_steps(eng):
    """twk.long_chain_case: 5 000 one-member unitigs walked by one read and by one on the twin strand.  Its random node records give
    junctions above a length (both walks are bad); with the overlaps cut to the lengths of both sides the two walks are 5 000 steps of
    sound junctions, some of which add no byte"""
    case = twk.long_chain_case(5000)
    walks, (toff, tgt, bad) = _case_targets(eng, case, 78, "long chain")
    assert walks["n_steps"].tolist() == [5000, 5000] and bad.tolist() == [1, 1] and len(tgt) == 0
    rng = np.random.default_rng(78)
    strings = random_strings(rng, case["mo"])
    ln = np.array([len(s) for s in strings], dtype=np.int64)
    ov = case["mo"]["overlap"].astype(np.int64).copy()
    ov[0:-2:2] = np.minimum(ov[0:-2:2], np.minimum(ln[:-1], ln[1:]))  # 2 t leaves for 2 t + 2
    ov[3::2] = np.minimum(ov[3::2], np.minimum(ln[1:], ln[:-1]))  # 2 t + 1 leaves for 2 t - 1
    ov = ov.astype(np.uint32)
    su = case["paths"]["unitig"]
    total = [len(twk.stitched_path(strings, ov, su[a:a + 5000].tolist())) for a in (0, 5000)]
    sound = dict(walks, path_start=np.array([3, 0], dtype=np.uint64), path_end=np.array([total[0] - 2, total[1]], dtype=np.uint64))
    toff, tgt, bad = device_targets(eng, sound, su, strings, ov, "long chain, sound")
    assert bad.tolist() == [0, 0] and len(tgt) == total[0] - 5 + total[1] > 20000
    past = dict(sound, path_end=np.array([total[0] + 1, total[1]], dtype=np.uint64))
    assert device_targets(eng, past, su, strings, ov, "long chain, past the end")[2].tolist() == [1, 0]


@pytest.mark.gpu
def test_device_targets_random_decompositions(eng):
    """random node records give junctions above a length among sound ones, circular unitigs walked round, both strands"""
    rng = np.random.default_rng(79)
    case = twk.walked_case(rng, 300, list(rng.integers(0, 60, size=80)))
    walks, (toff, tgt, bad) = _case_targets(eng, case, 80, "walked")
    assert walks["flags"].any() and int(walks["n_steps"].max()) > 1 and len(tgt) > 4096
    print("random decomposition: %d walks, %d bad, %d bytes" % (len(bad), int(bad.sum()), len(tgt)))


@pytest.mark.gpu
def test_device_targets_refusals_nothing_written(eng):
    walks, paths, strings, mo = hand_targets()
    su, ov = paths["unitig"], mo["overlap"]
    base = device_targets(eng, walks, su, strings, ov, "base")
    n = len(base[1])

    def refused(code=1, **kw):
        s, nb, got = raw_targets(eng, walks, su, strings, ov, capacity=n, **kw)
        assert (s, nb) == (code, 0) and all(_marked(x) for x in got.values()), (s, nb, list(kw))

    def changed(name, i, v, src):
        x = np.array(src).copy()
        x[i] = v
        return {name: x}

    refused(ctx=False)
    for f in ("first_step", "n_steps", "path_start", "path_end", "flags", "unitig", "out_off", "out", "overlap"):
        refused(null=(f,))
    refused(**changed("first_step", 3, len(su), walks["first_step"]))  # a step index outside the paths
    refused(**changed("n_steps", 3, len(su) + 1, walks["n_steps"]))
    refused(**changed("first_step", 0, 2 ** 63, walks["first_step"]))
    refused(**changed("unitig", 4, 2 * len(strings), su))
    refused(**changed("unitig", 0, 2 ** 32 - 1, su))
    refused(T=len(strings) - 1)
    out_off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.uint64)
    refused(**changed("out_off", 2, int(out_off[3]) + 1, out_off))  # out_off decreases
    refused(n_bases=int(out_off[-1]) - 1)  # the unitigs pass the bytes given
    big = out_off.copy()
    big[3:] += np.uint64(2 ** 32)
    refused(out_off=big, n_bases=2 ** 33)  # a unitig of 2^32 bases: refused before a byte is read
    z = ctypes.c_uint64(5)
    P = ctypes.c_void_p(16)
    assert eng.lib.s2k_walks_targets(eng.ctx, 1, P, P, P, P, P, P, 1, P, P, 1, P, 2 ** 31, None, None, None, 0, ctypes.byref(z)) == 1 and z.value == 0


def _gaf_lines(path):
    return [line.split("\t") for line in open(path).read().split("\n") if line]


def _assert_alignments(al, ref, tag):
    got = al.host()
    want = host_alignments(ref)
    for f in ("edits", "flags", "n_ops", "matches", "ops_off"):
        assert got[f].tobytes() == want[f].tobytes(), (tag, f)
    off = ref["ops_off"].astype(np.int64)
    for i, o in enumerate(ref["ops"]):
        assert got["ops"][off[i]: off[i] + len(o)].tobytes() == o.tobytes(), (tag, i)
        assert al.cigar(i) == cigar_of(ref["res"][i][2]), (tag, i)
    assert (al.n_over, al.n_bad) == (int((ref["flags"] & OVER != 0).sum()), int((ref["flags"] & BAD_PATH != 0).sum())), tag


def _device_reference(walks, contigs, seqs, reads):
    """the references over what the device holds: its walks (equal to walks_reference in test_walk.py and test_lift.py), its bytes"""
    h = walks.host()
    strings = tus.unitig_strings(None, {"out_off": tg._u64(seqs[0]), "out": seqs[1].cpu().numpy()})
    return walk_alignments_reference(h, walks.paths.unitig.cpu().numpy().view(np.uint32), strings, contigs.overlap.cpu().numpy().view(np.uint32), reads)


@pytest.mark.gpu
def test_repeat_fixture_end_to_end(eng, repeat_case, noisy_case, tmp_path):
    """thread -> (noisy: bridge) -> spans -> resolve -> untangle_map -> lift -> walks -> align -> write_gaf, on the device throughout"""
    c, R, n = repeat_case, tsp.REPEAT, noisy_case
    clean = twk._extract_all(eng, c["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    graph = pkg.KminmerGraph.build(eng, [clean], min_count=R["min_count"], min_edge_count=1)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, [clean])
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    noisy = twk._extract_all(eng, n["reads"], R["l"], R["k"], R["d"], pkg.HashMode.Regular)
    plain = ug.thread(eng, table, clean, len(c["reads"]), min_count=R["min_count"])
    bridged, _ = ug.bridge(eng, ug.thread(eng, table, noisy, len(n["reads"]), min_count=R["min_count"]))
    table.close()
    for tag, paths, reads, outs in (("clean", plain, c["reads"], clean), ("noisy", bridged, n["reads"], noisy)):
        resolved, partner, _ = ug.resolve(eng, ug.span_table(eng, [paths]), min_support=2)
        contigs, node_origin, st, lift = ug.untangle_map(eng, resolved, partner)
        assert st["contigs"] == 2
        lifted, _ = lift.lift(eng, paths)
        cns = ns.take(node_origin)
        walks = contigs.walks(eng, lifted, cns)
        seqs = contigs.sequences(eng, cns)
        al = contigs.align(eng, walks, outs["bases"], outs["read_off"], seqs)
        ref = _device_reference(walks, contigs, seqs, reads)
        _assert_alignments(al, ref, tag)
        p = str(tmp_path / (tag + ".gaf"))
        walks.write_gaf(p, contigs, alignments=al)
        lines = _gaf_lines(p)
        h = walks.host()
        assert len(lines) == walks.n_walks and (al.n_over, al.n_bad) == (0, 0)
        if tag == "clean":
            for i, f in enumerate(lines):
                nq = int(h["qend"][i]) - int(h["qstart"][i])
                assert f[-2:] == ["NM:i:0", "cg:Z:%d=" % nq] and f[9] == f[10] == str(nq), (i, f)
        else:
            assert al.host()["edits"].sum() > 100
            for i, f in enumerate(lines):
                assert f[-2:] == ["NM:i:%d" % ref["edits"][i], "cg:Z:" + cigar_of(ref["res"][i][2])] and f[9] == str(ref["matches"][i]), (i, f)
                assert int(f[10]) == sum(ln for ln, _ in ref["res"][i][2]) == int(al.block_len[i]), i
        plain_gaf = str(tmp_path / (tag + "_plain.gaf"))
        walks.write_gaf(plain_gaf, contigs)
        assert [f[:9] + f[11:14] for f in lines] == [f[:9] + f[11:14] for f in _gaf_lines(plain_gaf)]
        before = ug.walks(eng, paths, ns)  # and on the unitig graph, walks of several steps
        useqs = ug.sequences(eng, ns)
        _assert_alignments(ug.align(eng, before, outs["bases"], outs["read_off"], useqs), _device_reference(before, ug, useqs, reads), tag + ", unitigs")
        print("%s repeat reads aligned on the device: %d walks on the contigs, %d edits in all" % (tag, walks.n_walks, int(al.host()["edits"].sum())))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,l,k", tsp.MODES)
def test_ecoli_reads_with_errors_through_the_simplified_graph(eng, ecoli, ecoli_reference, mode, l, k):
    """the 600 reads with 0.5 % substitutions through simplify(10, 20) and bridge(16, 2): walk for walk the reference's edits, runs and
    flags; in Regular 12 / 5 the walks and alignments are those the references alone gave (none over, none bad)"""
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
    if (mode, l, k) == tsp.MODES[0]:
        ref = ecoli_reference["al"]
        assert walks.host()["path_end"].tobytes() == ecoli_reference["walks"]["path_end"].tobytes()
    else:
        ref = _device_reference(walks, ug, seqs, reads)
        assert (al.n_over, al.n_bad) == (0, 1)  # Hpc 21 / 3: one walk crosses a junction whose overlap passes a unitig's length
    _assert_alignments(al, ref, mode.name)
    assert walks.n_walks >= 600 and int((ref["flags"] == 0).sum()) >= 0.95 * walks.n_walks
    print("E. coli %s: %d walks aligned, %d over, %d bad, %d edits in all" % (mode.name, walks.n_walks, al.n_over, al.n_bad, int(ref["edits"].sum())))
