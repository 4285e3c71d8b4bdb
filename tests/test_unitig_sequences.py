"""Base-space sequences of the graph's nodes and unitigs on the device: s2k_table_representatives, s2k_table_node_sequences and
s2k_unitig_sequences (include/s2k.h).  The references are `node_sequences_reference` and
`unitig_sequences_reference`, serial and written from the header's definitions; the device's arrays equal theirs byte for byte.  The
property that needs no reference: for error-free reads every stitched unitig is a substring of the genome or of its reverse
complement."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_graph as tg
import test_unitigs as tu
from conftest import ROOT
from s2k_loader import import_package

pkg = import_package()

SYMS = ("s2k_table_representatives", "s2k_table_node_sequences", "s2k_unitig_sequences")
NODE_DT = {"seq_off": np.uint64, "seq_len": np.uint32, "shift_fwd": np.uint32, "shift_rev": np.uint32, "rev": np.uint8}
NONE64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_RC = np.arange(256, dtype=np.uint8)
_RC[list(b"ACGTacgt")] = list(b"TGCAtgca")


def revcomp(b):
    return bytes(_RC[np.frombuffer(bytes(b), dtype=np.uint8)][::-1])


# ---- the references ----------------------------------------------------------------------------------------------------------------
def node_sequences_reference(batches, keys, k):
    """batches: dicts of host arrays km_off, hash, rev, mn_off, mn_j, mn_jend, bases, read_off, in order; keys: the nodes, ascending.
    -> dict rep, seq_off, seq_len, shift_fwd, shift_rev, rev (one entry per key) and pool, by the definitions of include/s2k.h"""
    assert k >= 2
    index = {int(h): i for i, h in enumerate(keys)}
    n = len(keys)
    rep = np.full(n, NONE64, dtype=np.uint64)
    where = [None] * n
    ordinal = 0
    for bi, b in enumerate(batches):
        km, mn = [int(x) for x in b["km_off"]], [int(x) for x in b["mn_off"]]
        for r in range(len(km) - 1):
            items = km[r + 1] - km[r]
            assert items == 0 or mn[r + 1] - mn[r] == items + k - 1  # the count relation
            for j in range(items):
                i = index.get(int(b["hash"][km[r] + j]))
                if i is not None and rep[i] == NONE64:  # ordinals ascend: the first occurrence is the smallest
                    rep[i] = ordinal
                    where[i] = (bi, r, j)
                ordinal += 1
    out = {f: np.zeros(n, dtype=dt) for f, dt in NODE_DT.items()}
    pool = bytearray()
    for i in sorted((i for i in range(n) if where[i] is not None), key=lambda i: int(rep[i])):
        bi, r, j = where[i]
        b = batches[bi]
        t, x, base = int(b["mn_off"][r]) + j, int(b["km_off"][r]) + j, int(b["read_off"][r])
        first, last = int(b["mn_j"][t]), int(b["mn_jend"][t + k - 1])
        out["seq_off"][i], out["seq_len"][i], out["rev"][i] = len(pool), last - first + 1, int(b["rev"][x])
        out["shift_fwd"][i] = int(b["mn_j"][t + 1]) - first
        out["shift_rev"][i] = last - int(b["mn_jend"][t + k - 2])
        pool += bytes(b["bases"][base + first: base + last + 1])
    out["rep"], out["pool"] = rep, np.frombuffer(bytes(pool), dtype=np.uint8)
    return out


def oriented(nodes, u):
    """-> (seq(u), shift(u)) of the oriented node u = 2 i + o"""
    i, o = u >> 1, u & 1
    a = int(nodes["seq_off"][i])
    b = bytes(nodes["pool"][a: a + int(nodes["seq_len"][i])])
    if o == int(nodes["rev"][i]):
        return b, int(nodes["shift_fwd"][i])
    return revcomp(b), int(nodes["shift_rev"][i])


def unitig_sequences_reference(unitigs, nodes):
    """unitigs: uni_off, members, circular (tu.unitig_reference) -> dict out_off uint64, out uint8, overlap uint32 (per oriented unitig)"""
    off, mem = [int(x) for x in unitigs["uni_off"]], [int(x) for x in unitigs["members"]]
    T = len(off) - 1
    out, out_off, overlap = bytearray(), [0], np.zeros(2 * T, dtype=np.uint32)
    for t in range(T):
        m = mem[off[t]: off[t + 1]]
        for p, u in enumerate(m):
            s, sh = oriented(nodes, u)
            assert sh <= len(s)
            out += s if (p == len(m) - 1 and not unitigs["circular"][t]) else s[:sh]
        out_off.append(len(out))
        for side, u in ((0, m[-1]), (1, m[0] ^ 1)):
            s, sh = oriented(nodes, u)
            overlap[2 * t + side] = len(s) - sh
    return {"out_off": np.array(out_off, dtype=np.uint64), "out": np.frombuffer(bytes(out), dtype=np.uint8), "overlap": overlap}


def reference_pipeline(batches, k, min_count):
    g = tg.graph_reference(batches, min_count)
    uni = tu.unitig_reference(g["row_off"], g["dst"], len(g["keys"]))
    nodes = node_sequences_reference(batches, g["keys"], k)
    return g, uni, nodes, unitig_sequences_reference(uni, nodes)


def unitig_strings(uni, seqs):
    off = [int(x) for x in seqs["out_off"]]
    return [bytes(seqs["out"][off[t]: off[t + 1]]) for t in range(len(off) - 1)]


def multi_reading_nodes(batches, keys, k):
    """the nodes whose occurrences do not all read the same: for every occurrence the triple (seq(2 i), shift(2 i), shift(2 i + 1)) it
    would give as the representative, from the inputs alone -> sorted node indices with more than one distinct triple.  A node is a
    64-bit hash (KminmerHash is Eq by hash alone, src/kminmer.rs:181-204), so distinct k-min-mers whose hashes collide are one node."""
    index = {int(h): i for i, h in enumerate(keys)}
    seen = [set() for _ in keys]
    for b in batches:
        km = [int(x) for x in b["km_off"]]
        for r in range(len(km) - 1):
            base = int(b["read_off"][r])
            for j in range(km[r + 1] - km[r]):
                x = km[r] + j
                i = index.get(int(b["hash"][x]))
                if i is None:
                    continue
                t = int(b["mn_off"][r]) + j
                a, e = int(b["mn_j"][t]), int(b["mn_jend"][t + k - 1])
                B, sf, sr = bytes(b["bases"][base + a: base + e + 1]), int(b["mn_j"][t + 1]) - a, e - int(b["mn_jend"][t + k - 2])
                seen[i].add((B, sf, sr) if int(b["rev"][x]) == 0 else (revcomp(B), sr, sf))
    return [i for i, x in enumerate(seen) if len(x) > 1]


# ---- hand-made inputs: k = 2, every byte written out ----------------------------------------------------------------------------------
def hand_batch(reads):
    """reads: (bytes, [mn_j], [mn_jend], [item hashes], [item revs]) -> a batch dict"""
    km, mn, bases, ro = [0], [0], b"", [0]
    h, rv, j, je = [], [], [], []
    for seq, mj, mje, hs, rvs in reads:
        assert len(mj) == len(mje) and (len(hs) == 0 or len(mj) == len(hs) + 1) and len(hs) == len(rvs)
        bases += seq
        ro.append(len(bases))
        h += hs
        rv += rvs
        j += mj
        je += mje
        km.append(len(h))
        mn.append(len(j))
    return {"km_off": np.array(km, dtype=np.uint64), "hash": np.array(h, dtype=np.uint64), "rev": np.array(rv, dtype=np.uint8),
            "mn_off": np.array(mn, dtype=np.uint64), "mn_j": np.array(j, dtype=np.uint32), "mn_jend": np.array(je, dtype=np.uint32),
            "bases": np.frombuffer(bases, dtype=np.uint8), "read_off": np.array(ro, dtype=np.uint64)}


READ = b"ACGTTGCA"  # minimizers AC@0-1, TT@3-4, GCA@5-7: item 0 = ACGTT (shifts 3, 3), item 1 = TTGCA (shifts 2, 3)


def chain(h0, h1, r0, r1, seq=READ):
    return [hand_batch([(seq, [0, 3, 5], [1, 4, 7], [h0, h1], [r0, r1])])]


# the circle ACGTTGCAG with minimizers at 0, 3 and 6; read B starts at TT and goes once round and on to the second TT
CIRCLE_A = (b"ACGTTGCA", [0, 3, 6], [1, 4, 7], [10, 20], [0, 0])
CIRCLE_B = (b"TTGCAGACGTT", [0, 3, 6, 9], [1, 4, 7, 10], [20, 30, 10], [0, 0, 0])

HAND = {
    # name: (batches, unitig strings, pool, circular)
    "chain ++": (chain(10, 20, 0, 0), [b"ACGTTGCA"], b"ACGTTTTGCA", [0]),
    "chain +-": (chain(10, 20, 0, 1), [b"ACGTTGCA"], b"ACGTTTTGCA", [0]),
    "chain -+ (odd start)": (chain(10, 20, 1, 0), [b"ACGTTGCA"], b"ACGTTTTGCA", [0]),
    "chain --": (chain(10, 20, 1, 1), [b"ACGTTGCA"], b"ACGTTTTGCA", [0]),
    # the first item is the larger key: the kept strand is the twin, read backwards and complemented
    "twin ++": (chain(20, 10, 0, 0), [b"TGCAACGT"], b"ACGTTTTGCA", [0]),
    "twin +- ": (chain(20, 10, 0, 1), [b"TGCAACGT"], b"ACGTTTTGCA", [0]),
    "twin -+": (chain(20, 10, 1, 0), [b"TGCAACGT"], b"ACGTTTTGCA", [0]),
    "twin --": (chain(20, 10, 1, 1), [b"TGCAACGT"], b"ACGTTTTGCA", [0]),
    "other bytes": (chain(20, 10, 0, 0, b"AcNTtGxA"), [b"TxCaANgT"], b"AcNTtTtGxA", [0]),
    "circle": ([hand_batch([CIRCLE_A, CIRCLE_B])], [b"ACGTTGCAG"], b"ACGTTTTGCACAGAC", [1]),
    "circle, two batches": ([hand_batch([CIRCLE_A]), hand_batch([CIRCLE_B])], [b"ACGTTGCAG"], b"ACGTTTTGCACAGAC", [1]),
    "empty reads between": ([hand_batch([(b"", [], [], [], []), CIRCLE_A, (b"GG", [0], [1], [], []), (b"", [], [], [], [])]),
                             hand_batch([(b"T", [], [], [], []), CIRCLE_B])], [b"ACGTTGCAG"], b"ACGTTTTGCACAGAC", [1]),
}


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    assert hasattr(pkg, "NodeSequences") and hasattr(pkg.NodeSequences, "build") and hasattr(pkg.UnitigGraph, "sequences")
    assert hasattr(pkg.Engine, "unitig_sequences") and hasattr(pkg, "write_fasta") and hasattr(pkg, "NodeSeqs") and hasattr(pkg, "revcomp")


def test_cpp_seq_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "seq_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "seq_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_node_seqs_layout_matches_ctypes(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    exe = str(tmp_path / "seq_layout")
    subprocess.check_call([gcc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "seq_layout.c"), "-o", exe])
    facts = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        k, *v = line.split()
        facts[k] = tuple(int(x) for x in v)
    T = pkg.NodeSeqs
    assert facts["sizeof.s2k_node_seqs"] == (ctypes.sizeof(T),)
    assert [f for f, _ in T._fields_] == ["seq_off", "seq_len", "shift_fwd", "shift_rev", "rev", "pool", "pool_capacity"]
    for f, ct in T._fields_:
        assert facts["s2k_node_seqs." + f] == (getattr(T, f).offset, ctypes.sizeof(ct)), f


@pytest.mark.parametrize("name", list(HAND))
def test_reference_hand_made(name):
    batches, want, pool, circ = HAND[name]
    g, uni, nodes, seqs = reference_pipeline(batches, 2, 1)
    assert unitig_strings(uni, seqs) == want, name
    assert bytes(nodes["pool"]) == pool and uni["circular"].tolist() == circ
    if name == "chain -+ (odd start)":
        assert uni["members"].tolist() == [1, 2]
    if name.startswith("chain") or name.startswith("twin"):
        # the overlap that leaves the unitig's last member (TTGCA read forwards: 5 - 2) and the one that leaves its twin's (5 - 3)
        assert nodes["seq_len"].tolist() == [5, 5] and seqs["overlap"].tolist() == ([3, 2] if name.startswith("chain") else [2, 3])
    if name.startswith("chain"):
        assert nodes["shift_fwd"].tolist() == [3, 2] and nodes["shift_rev"].tolist() == [3, 3] and nodes["rep"].tolist() == [0, 1]
    if name.startswith("circle"):
        assert nodes["rep"].tolist() == [0, 1, 3] and nodes["seq_off"].tolist() == [0, 5, 10] and seqs["overlap"].tolist() == [2, 2]
    assert pkg.revcomp(want[0]) == revcomp(want[0])


def test_reference_is_the_definition_not_the_first_item_in_key_order():
    """a node that occurs in both batches takes the occurrence of the first batch; one that occurs twice in a read the first of them"""
    a = hand_batch([(b"GGACGTTGCA", [2, 5, 7], [3, 6, 9], [10, 20], [0, 0])])  # the same minimizers two bytes further on
    b = hand_batch([(READ, [0, 3, 5], [1, 4, 7], [10, 20], [1, 1])])
    n = node_sequences_reference([a, b], [10, 20], 2)
    assert n["rep"].tolist() == [0, 1] and n["rev"].tolist() == [0, 0] and bytes(n["pool"]) == b"ACGTTTTGCA"
    n = node_sequences_reference([b, a], [10, 20], 2)
    assert n["rev"].tolist() == [1, 1]
    n = node_sequences_reference([a], [20, 99], 2)  # a key that never occurs keeps seq_len 0
    assert n["rep"].tolist() == [1, int(NONE64)] and n["seq_len"].tolist() == [5, 0]


def _oracle_batch(oracle, reads, l, k, d, mode):
    bases, off = pkg.pack_reads(reads)
    b = oracle.batch(bases, off, l, k, d, int(mode))
    m = oracle.batch_minimizers(bases, off, l, d, int(mode))
    b.update(mn_off=m["mn_off"], mn_j=m["j"], mn_jend=m["jend"], bases=bases, read_off=off)
    return b


def _flip(reads, flip):
    return [tg._revcomp(r) if (flip and i % 2) else r for i, r in enumerate(reads)]


# (mode, l, k, d, reads, seed, min_count, every second read reverse-complemented, unitigs the Regular graph has)
ECOLI = [("Regular", 21, 3, 0.05, 150, 5, 2, True, 25), ("Regular", 21, 3, 0.05, 600, 7, 2, True, 13), ("Regular", 12, 5, 0.05, 150, 5, 2, True, 13),
         ("Regular", 21, 3, 0.05, 600, 7, 1, False, 13), ("Hpc", 12, 5, 0.05, 150, 5, 2, True, None), ("Hpc", 21, 3, 0.05, 600, 7, 2, True, None),
         ("Hpc", 21, 3, 0.05, 600, 7, 1, False, None)]
ECOLI_EXCEPTION = ("Hpc", 21, 3, 0.05, 150, 5, 2, True, None)  # one inconsistent link: device == reference only


def _links_consistent(uni, nodes):
    off, mem = [int(x) for x in uni["uni_off"]], [int(x) for x in uni["members"]]
    bad = 0
    for t in range(len(off) - 1):
        for a, b in zip(mem[off[t]: off[t + 1] - 1], mem[off[t] + 1: off[t + 1]]):
            s, sh = oriented(nodes, a)
            bad += not oriented(nodes, b)[0].startswith(s[sh:])
    return bad


@pytest.mark.parametrize("case", ECOLI, ids=lambda c: "%s-%d-%d-%dreads-mc%d%s" % (c[0], c[1], c[2], c[4], c[6], "-flip" if c[7] else ""))
def test_error_free_reads_stitch_to_substrings_of_the_genome(oracle, ecoli, case):
    mode, l, k, d, n, seed, mc, flip, n_want = case
    reads = _flip(tg._sample_reads(ecoli, n, seed), flip)
    b = _oracle_batch(oracle, reads, l, k, d, pkg.HashMode[mode])
    km, mn = b["km_off"].astype(np.int64), b["mn_off"].astype(np.int64)
    items, trip = np.diff(km), np.diff(mn)
    assert ((items == 0) | (trip == items + k - 1)).all()  # the count relation, every read
    first = mn[:-1][items > 0]
    assert np.array_equal(b["start"][km[:-1][items > 0]], b["mn_j"][first])  # start[j] == mn_j[j]
    assert np.array_equal(b["end"][km[:-1][items > 0]], b["mn_jend"][first + k - 1])  # end[j] == mn_jend[j + k - 1]
    g, uni, nodes, seqs = reference_pipeline([b], k, mc)
    strings = unitig_strings(uni, seqs)
    print("%s: %d nodes, %d unitigs, %d bases, longest %d" % (case, len(g["keys"]), len(strings), len(seqs["out"]), max(map(len, strings))))
    assert not uni["circular"].any() and len(strings) >= 4
    if n_want is not None:
        assert len(strings) == n_want
    rc = revcomp(ecoli)
    missing = [t for t, s in enumerate(strings) if s not in ecoli and s not in rc]
    assert missing == [] and _links_consistent(uni, nodes) == 0


def test_nodes_with_two_readings_are_hash_collisions(oracle, ecoli):
    """Which bytes a node gets can depend on the order of the input only when its occurrences read differently.  Regular 21/3/0.05 on
    the E. coli fixture has 4 such nodes (the same 4 for 150, 300 and 600 reads), and each is a collision of the 64-bit k-min-mer
    hash: two different triples of minimizer hashes, at windows of one locus a few bases apart, with one hash (the l-mer hash, its
    xorshift mix and the rolling combination over the k minimizers are all linear over GF(2), and the l-mers of minimizers at
    neighbouring positions are linearly related).  Regular 12/5/0.05 has none: there every node has one reading, and the sequences
    cannot depend on the order."""
    reads = _flip(tg._sample_reads(ecoli, 300, 7), True)
    b = _oracle_batch(oracle, reads, 21, 3, 0.05, pkg.HashMode.Regular)
    mh = oracle.batch_minimizers(*pkg.pack_reads(reads), 21, 0.05, int(pkg.HashMode.Regular))["hash"]
    keys = tg.graph_reference([b], 2)["keys"]
    multi = multi_reading_nodes([b], keys, 3)
    assert len(multi) == 4
    km = b["km_off"].astype(np.int64)
    for i in multi:
        tuples = set()
        for x in np.nonzero(b["hash"] == keys[i])[0]:
            r = int(np.searchsorted(km, x, side="right") - 1)
            t = int(b["mn_off"][r]) + int(x - km[r])
            m = tuple(int(v) for v in mh[t: t + 3])
            tuples.add(min(m, m[::-1]))
        assert len(tuples) == 2, (i, tuples)  # two k-min-mers, one hash
    for n, seed in ((150, 5), (300, 7)):
        reads = _flip(tg._sample_reads(ecoli, n, seed), True)
        b = _oracle_batch(oracle, reads, 12, 5, 0.05, pkg.HashMode.Regular)
        assert multi_reading_nodes([b], tg.graph_reference([b], 2)["keys"], 5) == []


def test_write_gfa_and_fasta_with_sequences_hand_made(tmp_path):
    batches = chain(10, 20, 0, 0)
    g, uni, nodes, seqs = reference_pipeline(batches, 2, 1)
    p = str(tmp_path / "g.gfa")
    pkg.write_gfa(p, g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], sequences=nodes)
    assert open(p).read() == ("H\tVN:Z:1.0\nS\t0\tACGTT\tLN:i:5\tKC:i:1\tkh:Z:000000000000000a\nS\t1\tTTGCA\tLN:i:5\tKC:i:1\tkh:Z:0000000000000014\n"
                              "L\t0\t+\t1\t+\t2M\tRC:i:1\n")
    pkg.write_gfa(p, g["keys"], g["counts"], g["edge_keys"], g["edge_counts"])
    assert open(p).read() == "H\tVN:Z:1.0\nS\t0\t*\tKC:i:1\tkh:Z:000000000000000a\nS\t1\t*\tKC:i:1\tkh:Z:0000000000000014\nL\t0\t+\t1\t+\t*\tRC:i:1\n"
    # node 0 seen on the other strand first: orientation 0 is the reverse complement of its bytes, and the edge leaves 0- ... written
    # as the twin pair's smaller key
    g, uni, nodes, seqs = reference_pipeline(chain(10, 20, 1, 0), 2, 1)
    pkg.write_gfa(p, g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], sequences=nodes)
    assert open(p).read().split("\n")[1:4] == ["S\t0\tAACGT\tLN:i:5\tKC:i:1\tkh:Z:000000000000000a", "S\t1\tTTGCA\tLN:i:5\tKC:i:1\tkh:Z:0000000000000014",
                                               "L\t0\t-\t1\t+\t2M\tRC:i:1"]
    # unitigs: a branching graph, two reads that share their first node
    batches = [hand_batch([(READ, [0, 3, 5], [1, 4, 7], [10, 20], [0, 0]), (b"ACGTTAAC", [0, 3, 6], [1, 4, 7], [10, 30], [0, 0])])]
    g, uni, nodes, seqs = reference_pipeline(batches, 2, 1)
    assert unitig_strings(uni, seqs) == [b"ACGTT", b"TTGCA", b"TTAAC"] and seqs["overlap"].tolist() == [2, 2, 3, 2, 2, 2]
    ec = g["edge_counts"][uni["src_edge"].astype(np.int64)]
    pkg.write_unitig_gfa(p, uni["uni_off"], uni["members"], [1, 1, 1], uni["edge_keys"], ec, members=True,
                         sequences=(seqs["out_off"], seqs["out"], seqs["overlap"]))
    assert open(p).read() == ("H\tVN:Z:1.0\nS\t0\tACGTT\tLN:i:5\tnm:i:1\tKC:i:1\tnd:Z:0+\nS\t1\tTTGCA\tLN:i:5\tnm:i:1\tKC:i:1\tnd:Z:1+\n"
                              "S\t2\tTTAAC\tLN:i:5\tnm:i:1\tKC:i:1\tnd:Z:2+\nL\t0\t+\t1\t+\t2M\tRC:i:1\nL\t0\t+\t2\t+\t2M\tRC:i:1\n")
    pkg.write_unitig_gfa(p, uni["uni_off"], uni["members"], [1, 1, 1], uni["edge_keys"], ec)
    assert open(p).read() == ("H\tVN:Z:1.0\nS\t0\t*\tLN:i:1\tKC:i:1\nS\t1\t*\tLN:i:1\tKC:i:1\nS\t2\t*\tLN:i:1\tKC:i:1\n"
                              "L\t0\t+\t1\t+\t*\tRC:i:1\nL\t0\t+\t2\t+\t*\tRC:i:1\n")
    pkg.write_fasta(p, seqs["out_off"], seqs["out"])
    assert open(p).read() == ">0\nACGTT\n>1\nTTGCA\n>2\nTTAAC\n"


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


FRONT = 16  # guard elements in front of every output (16 bytes keep d_out aligned) and behind it
TORCH_DT = {np.uint64: "int64", np.uint32: "int32", np.uint8: "uint8"}


class Guarded:
    """a device array of n elements with FRONT marker elements on either side; the payload starts as `init`"""

    def __init__(self, n, np_dt, init=None, marker=0x5A):
        import torch

        self.n, self.np_dt = n, np_dt
        dt = getattr(torch, TORCH_DT[np_dt])
        self.t = torch.full((FRONT + n + FRONT,), marker, dtype=dt, device="cuda:0")
        self.marker = marker
        if init is not None and n:
            self.t[FRONT: FRONT + n] = init
        self.ptr = self.t.data_ptr() + FRONT * self.t.element_size()

    def host(self):
        return self.t[FRONT: FRONT + self.n].cpu().numpy().view(self.np_dt)

    def intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:FRONT] == self.marker).all() and (h[FRONT + self.n:] == self.marker).all())

    def untouched(self):
        return bool((self.t.cpu().numpy() == self.marker).all())


def _dev_batch(b):
    import torch

    d = {f: tg._dev(np.asarray(b[f], dtype=np.uint64), torch.int64) for f in ("km_off", "mn_off", "read_off")}
    d["hash"] = tg._dev(np.asarray(b["hash"], dtype=np.uint64), torch.int64)
    d["mn_j"], d["mn_jend"] = (tg._dev(np.asarray(b[f], dtype=np.uint32), torch.int32) for f in ("mn_j", "mn_jend"))
    d["rev"], d["bases"] = tg._dev(np.asarray(b["rev"], dtype=np.uint8), torch.uint8), tg._dev(np.asarray(b["bases"], dtype=np.uint8), torch.uint8)
    for f in d:  # a NULL pointer only where the test asks for one
        if d[f].numel() == 0:
            d[f] = torch.zeros(16, dtype=d[f].dtype, device="cuda:0")
    return d


def _in_struct(b, d, null=()):
    i = pkg.DeviceOut()
    i.km_capacity, i.mn_capacity = int(b["km_off"][-1]), int(b["mn_off"][-1])
    for f in ("km_off", "hash", "rev", "mn_off", "mn_j", "mn_jend"):
        if f not in null:
            setattr(i, f, d[f].data_ptr())
    return i


def raw_nodes(eng, batches, keys, k):
    """the three-round protocol through ctypes, every output between guards -> (dict of host arrays like the reference's, guards ok)"""
    import torch

    t = tg._table(eng, keys, None)
    n = len(keys)
    devs = [_dev_batch(b) for b in batches]
    ins = [_in_struct(b, d) for b, d in zip(batches, devs)]
    nr = [len(b["km_off"]) - 1 for b in batches]
    rep = Guarded(n, np.uint64, init=-1)
    torch.cuda.synchronize()
    base = 0
    for b, i, r in zip(batches, ins, nr):
        assert eng.lib.s2k_table_representatives(ctypes.c_void_p(t.handle), r, ctypes.byref(i), base, ctypes.c_void_p(rep.ptr)) == 0
        base += int(b["km_off"][-1])
    sizes, base = [], 0
    for b, d, i, r in zip(batches, devs, ins, nr):
        nb = ctypes.c_uint64(77)
        assert eng.lib.s2k_table_node_sequences(ctypes.c_void_p(t.handle), r, ctypes.byref(i), k, ctypes.c_void_p(d["bases"].data_ptr()),
                                                ctypes.c_void_p(d["read_off"].data_ptr()), base, ctypes.c_void_p(rep.ptr), None, 0, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
        base += int(b["km_off"][-1])
    total = sum(sizes)
    arr = {f: Guarded(n, dt, init=0) for f, dt in NODE_DT.items()}
    pool = Guarded(total, np.uint8)
    ns = pkg.NodeSeqs()
    for f in NODE_DT:
        setattr(ns, f, arr[f].ptr)
    ns.pool, ns.pool_capacity = pool.ptr, total
    torch.cuda.synchronize()
    base = used = 0
    for b, d, i, r, want in zip(batches, devs, ins, nr, sizes):
        nb = ctypes.c_uint64(77)
        s = eng.lib.s2k_table_node_sequences(ctypes.c_void_p(t.handle), r, ctypes.byref(i), k, ctypes.c_void_p(d["bases"].data_ptr()),
                                             ctypes.c_void_p(d["read_off"].data_ptr()), base, ctypes.c_void_p(rep.ptr), ctypes.byref(ns), used,
                                             ctypes.byref(nb))
        assert (s, nb.value) == (0, want)
        base += int(b["km_off"][-1])
        used += nb.value
    t.close()
    got = {f: arr[f].host() for f in NODE_DT}
    got["rep"], got["pool"] = rep.host(), pool.host()
    return got, all(a.intact() for a in list(arr.values()) + [rep, pool]), (arr, pool)


def raw_stitch(eng, uni, n_nodes, arr, pool, capacity=None, want_out=True):
    """s2k_unitig_sequences through ctypes on the guarded node arrays -> (status, n_bases, out_off, out, overlap: Guarded)"""
    import torch

    T = len(uni["uni_off"]) - 1
    d_off = tg._dev(np.asarray(uni["uni_off"], dtype=np.uint64), torch.int64)
    d_mem = tg._dev(np.asarray(uni["members"], dtype=np.uint32), torch.int32)
    d_circ = tg._dev(np.asarray(uni["circular"], dtype=np.uint8), torch.uint8)
    ns = pkg.NodeSeqs()
    for f in NODE_DT:
        setattr(ns, f, arr[f].ptr)
    ns.pool, ns.pool_capacity = pool.ptr, pool.n
    out_off, overlap = Guarded(T + 1, np.uint64), Guarded(2 * T, np.uint32)
    nb = ctypes.c_uint64(77)
    torch.cuda.synchronize()
    args = (eng.ctx, ctypes.c_void_p(d_off.data_ptr()), ctypes.c_void_p(d_mem.data_ptr() if n_nodes else 0),
            ctypes.c_void_p(d_circ.data_ptr() if T else 0), T, n_nodes, ctypes.byref(ns), ctypes.c_void_p(out_off.ptr))
    s = eng.lib.s2k_unitig_sequences(*args, None, ctypes.c_void_p(overlap.ptr), 0, ctypes.byref(nb))
    if not want_out or s != 0:
        return s, nb.value, out_off, None, overlap
    cap = nb.value if capacity is None else capacity
    out = Guarded(cap, np.uint8)
    out_off, overlap = Guarded(T + 1, np.uint64), Guarded(2 * T, np.uint32)
    args = args[:-1] + (ctypes.c_void_p(out_off.ptr),)
    torch.cuda.synchronize()
    s = eng.lib.s2k_unitig_sequences(*args, ctypes.c_void_p(out.ptr), ctypes.c_void_p(overlap.ptr), cap, ctypes.byref(nb))
    return s, nb.value, out_off, out, overlap


def check_device(eng, batches, k, min_count, tag):
    """device == reference for every array, through the raw ABI with guards"""
    g, uni, nodes, seqs = reference_pipeline(batches, k, min_count)
    got, ok, (arr, pool) = raw_nodes(eng, batches, g["keys"], k)
    assert ok, tag
    for f in list(NODE_DT) + ["rep", "pool"]:
        assert got[f].tobytes() == np.asarray(nodes[f], dtype=got[f].dtype).tobytes(), (tag, f)
    s, nb, out_off, out, overlap = raw_stitch(eng, uni, len(g["keys"]), arr, pool)
    assert (s, nb) == (0, len(seqs["out"])), (tag, s, nb)
    assert out_off.host().tobytes() == seqs["out_off"].tobytes() and out.host().tobytes() == seqs["out"].tobytes(), tag
    assert overlap.host().tobytes() == seqs["overlap"].tobytes(), tag
    assert out_off.intact() and out.intact() and overlap.intact(), tag
    return g, uni, nodes, seqs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_device_hand_made(eng, name):
    batches, want, pool, circ = HAND[name]
    g, uni, nodes, seqs = check_device(eng, batches, 2, 1, name)
    assert unitig_strings(uni, seqs) == want


def _extract_mn(eng, reads, l, k, d, mode):
    """extract_device with FLAG_WANT_MINIMIZERS -> dict of GPU tensors: the outs NodeSequences.build wants"""
    import torch

    bases, off = pkg.pack_reads(reads)
    dev = torch.device("cuda", 0)
    db = torch.from_numpy(bases.copy()).to(dev)
    do = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    cap = len(bases) + 1
    t = {"km_off": torch.empty(len(reads) + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
         "rev": torch.empty(cap, dtype=torch.uint8, device=dev), "mn_off": torch.empty(len(reads) + 1, dtype=torch.int64, device=dev),
         "mn_j": torch.empty(cap, dtype=torch.int32, device=dev), "mn_jend": torch.empty(cap, dtype=torch.int32, device=dev),
         "mn_hash": torch.empty(cap, dtype=torch.int32, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = o.mn_capacity = cap
    for f in t:
        setattr(o, f, t[f].data_ptr())
    torch.cuda.synchronize()
    eng.extract_device(db.data_ptr(), do.data_ptr(), len(reads), len(bases), l, k, d, int(mode), o, flags=pkg.FLAG_WANT_MINIMIZERS)
    t["bases"], t["read_off"] = db, do
    return t


def _host_batch(t):
    nk, nm = int(t["km_off"][-1]), int(t["mn_off"][-1])
    return {"km_off": tg._u64(t["km_off"]), "hash": tg._u64(t["hash"][:nk]), "rev": t["rev"][:nk].cpu().numpy(), "mn_off": tg._u64(t["mn_off"]),
            "mn_j": t["mn_j"][:nm].cpu().numpy().view(np.uint32), "mn_jend": t["mn_jend"][:nm].cpu().numpy().view(np.uint32),
            "bases": t["bases"].cpu().numpy(), "read_off": tg._u64(t["read_off"])}


def _split(reads, parts):
    cut = [len(reads) * i // parts for i in range(parts + 1)]
    if parts == 3:
        cut[1] = cut[0] + 1  # a batch of one read
    return [reads[a:b] for a, b in zip(cut[:-1], cut[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ECOLI + [ECOLI_EXCEPTION], ids=lambda c: "%s-%d-%d-%dreads-mc%d%s" % (c[0], c[1], c[2], c[4], c[6], "-flip" if c[7] else ""))
def test_device_ecoli_batches_raw_and_classes(eng, oracle, ecoli, case):
    """the E. coli inputs in one, two and three batches: the device's extraction (with minimizers) equals the oracle's, every array of
    the three calls equals the reference through the raw ABI, and the Python classes give the same bytes"""
    mode, l, k, d, n, seed, mc, flip, _ = case
    reads = _flip(tg._sample_reads(ecoli, n, seed), flip)
    rc = revcomp(ecoli)
    first = None
    for parts in (1, 2, 3):
        outs = [_extract_mn(eng, r, l, k, d, pkg.HashMode[mode]) for r in _split(reads, parts)]
        batches = [_host_batch(t) for t in outs]
        if parts == 1:
            ob = _oracle_batch(oracle, reads, l, k, d, pkg.HashMode[mode])
            for f in ("km_off", "hash", "rev", "mn_off", "mn_j", "mn_jend"):
                assert batches[0][f].tobytes() == ob[f].tobytes(), f
        g, uni, nodes, seqs = check_device(eng, batches, k, mc, (case, parts))
        strings = unitig_strings(uni, seqs)
        if case is not ECOLI_EXCEPTION:
            assert all(s in ecoli or s in rc for s in strings) and not uni["circular"].any()
        if first is None:
            first = sorted(min(s, revcomp(s)) for s in strings)
        assert sorted(min(s, revcomp(s)) for s in strings) == first  # the split changes no sequence
        graph = pkg.KminmerGraph.build(eng, outs, min_count=mc)
        ug = graph.unitigs(eng)
        ns = pkg.NodeSequences.build(eng, graph, outs)
        assert ns.k == k and ns.n_bytes == len(nodes["pool"])
        h = ns.host()
        for f in list(NODE_DT) + ["rep", "pool"]:
            assert h[f].tobytes() == np.asarray(nodes[f], dtype=h[f].dtype).tobytes(), (case, parts, f)
        out_off, out = ug.sequences(eng, ns)
        assert tg._u64(out_off).tobytes() == seqs["out_off"].tobytes() and out.cpu().numpy().tobytes() == seqs["out"].tobytes()
        assert ug.overlap.cpu().numpy().view(np.uint32).tobytes() == seqs["overlap"].tobytes()


@pytest.mark.gpu
def test_device_gfa_and_fasta_from_classes(eng, ecoli, tmp_path):
    reads = _flip(tg._sample_reads(ecoli, 150, 5), True)
    outs = [_extract_mn(eng, reads, 21, 3, 0.05, pkg.HashMode.Regular)]
    graph = pkg.KminmerGraph.build(eng, outs, min_count=2)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, outs)
    out_off, out = ug.sequences(eng, ns)
    p, q = str(tmp_path / "u.gfa"), str(tmp_path / "u.fa")
    ug.write_gfa(p, sequences=(out_off, out))
    pkg.write_fasta(q, out_off, out)
    rc = revcomp(ecoli)
    s_lines = [x.split("\t") for x in open(p).read().split("\n") if x.startswith("S\t")]
    fa = open(q).read().split("\n")
    assert len(s_lines) == ug.n_unitigs == 25
    for t, x in enumerate(s_lines):
        assert (x[2].encode() in ecoli or x[2].encode() in rc) and x[3] == "LN:i:%d" % len(x[2]) and x[4].startswith("nm:i:")
        assert fa[2 * t] == ">%d" % t and fa[2 * t + 1] == x[2]
    assert all(x.split("\t")[5].endswith("M") for x in open(p).read().split("\n") if x.startswith("L\t"))
    graph.write_gfa(p, sequences=ns)
    n_s = [x.split("\t") for x in open(p).read().split("\n") if x.startswith("S\t")]
    assert len(n_s) == graph.n_nodes and all(x[2].encode() in ecoli or x[2].encode() in rc for x in n_s)
    ug.write_gfa(p)
    assert all(x.split("\t")[2] == "*" for x in open(p).read().split("\n") if x.startswith("S\t"))


@pytest.mark.gpu
def test_device_refusals_capacity_and_sizes(eng):
    import torch

    batches = HAND["circle, two batches"][0]
    g, uni, nodes, seqs = reference_pipeline(batches, 2, 1)
    keys, n = g["keys"], len(g["keys"])
    got, ok, (arr, pool) = raw_nodes(eng, batches, keys, 2)
    assert ok
    t = tg._table(eng, keys, None)
    b, d = batches[0], _dev_batch(batches[0])
    rep = tg._dev(nodes["rep"], torch.int64)
    H = ctypes.c_void_p(t.handle)

    def nodeseq(i, k=2, ns=None, used=0, nr=1, dd=d, base=0):
        nb = ctypes.c_uint64(77)
        torch.cuda.synchronize()
        s = eng.lib.s2k_table_node_sequences(H, nr, ctypes.byref(i), k, ctypes.c_void_p(dd["bases"].data_ptr()),
                                             ctypes.c_void_p(dd["read_off"].data_ptr()), base, ctypes.c_void_p(rep.data_ptr()),
                                             ctypes.byref(ns) if ns is not None else None, used, ctypes.byref(nb))
        return s, nb.value

    def fresh(total):
        a = {f: Guarded(n, dt) for f, dt in NODE_DT.items()}
        p = Guarded(total, np.uint8)
        ns = pkg.NodeSeqs()
        for f in NODE_DT:
            setattr(ns, f, a[f].ptr)
        ns.pool, ns.pool_capacity = p.ptr, total
        return a, p, ns

    assert nodeseq(_in_struct(b, d)) == (0, 10)  # sizes only
    for k in (0, 1):
        assert nodeseq(_in_struct(b, d), k=k) == (1, 0)
    assert nodeseq(_in_struct(b, d), k=3) == (1, 0)  # a wrong k: 3 triples are not 2 + 3 - 1
    for f in ("km_off", "hash", "rev", "mn_off", "mn_j", "mn_jend"):
        assert nodeseq(_in_struct(b, d, null=(f,))) == (1, 0), f
    a, p, ns = fresh(9)  # one byte short: nothing written, the size still set
    assert nodeseq(_in_struct(b, d), ns=ns) == (7, 10) and all(x.untouched() for x in list(a.values()) + [p])
    a, p, ns = fresh(12)
    assert nodeseq(_in_struct(b, d), ns=ns, used=3) == (7, 10) and all(x.untouched() for x in list(a.values()) + [p])
    assert nodeseq(_in_struct(b, d), ns=ns, used=2) == (0, 10) and bytes(p.host()) == b"\x5a\x5aACGTTTTGCA" and p.intact()
    assert nodeseq(_in_struct(b, d), nr=0) == (0, 0)  # no reads
    i = _in_struct(b, d)
    assert eng.lib.s2k_table_representatives(H, 0, ctypes.byref(i), 0, ctypes.c_void_p(rep.data_ptr())) == 0
    assert eng.lib.s2k_table_representatives(None, 1, ctypes.byref(i), 0, ctypes.c_void_p(rep.data_ptr())) == 1
    assert eng.lib.s2k_table_representatives(H, 1, ctypes.byref(_in_struct(b, d, null=("hash",))), 0, ctypes.c_void_p(rep.data_ptr())) == 1
    assert rep.cpu().numpy().view(np.uint64).tolist() == nodes["rep"].tolist()
    t.close()
    # an empty table: nothing to write, no bytes
    e = tg._table(eng, np.zeros(0, dtype=np.uint64), None)
    nb = ctypes.c_uint64(77)
    assert eng.lib.s2k_table_representatives(ctypes.c_void_p(e.handle), 1, ctypes.byref(i), 0, None) == 0
    assert eng.lib.s2k_table_node_sequences(ctypes.c_void_p(e.handle), 1, ctypes.byref(i), 2, ctypes.c_void_p(d["bases"].data_ptr()),
                                            ctypes.c_void_p(d["read_off"].data_ptr()), 0, None, None, 0, ctypes.byref(nb)) == 0 and nb.value == 0
    e.close()
    # the stitch: sizes only, one byte short, no unitigs, broken inputs
    s, nb, out_off, out, overlap = raw_stitch(eng, uni, n, arr, pool, want_out=False)
    assert (s, nb) == (0, 9) and out_off.host().tolist() == [0, 9] and overlap.host().tolist() == [2, 2]
    s, nb, out_off, out, overlap = raw_stitch(eng, uni, n, arr, pool, capacity=8)
    assert (s, nb) == (7, 9) and out.untouched() and out_off.untouched() and overlap.untouched()
    s, nb, out_off, out, overlap = raw_stitch(eng, uni, n, arr, pool, capacity=9)
    assert (s, nb) == (0, 9) and bytes(out.host()) == b"ACGTTGCAG" and out.intact()
    none = {"uni_off": np.zeros(1, dtype=np.uint64), "members": np.zeros(0, dtype=np.uint32), "circular": np.zeros(0, dtype=np.uint8)}
    s, nb, out_off, out, overlap = raw_stitch(eng, none, 0, arr, pool, want_out=False)
    assert (s, nb) == (0, 0) and out_off.host().tolist() == [0] and out_off.intact()
    for f, v in (("uni_off", [0, 2]), ("uni_off", [1, 3]), ("members", [0, 2, 6]), ("uni_off", [0, 0])):
        bad = dict(uni)
        bad[f] = np.array(v, dtype=uni[f].dtype)
        if f == "uni_off" and v == [0, 0]:
            bad = {"uni_off": np.array([0, 0, 3], dtype=np.uint64), "members": uni["members"], "circular": np.array([1, 1], dtype=np.uint8)}
        s, nb, out_off, out, overlap = raw_stitch(eng, bad, n, arr, pool, want_out=False)
        assert (s, nb) == (1, 0) and out_off.untouched() and overlap.untouched(), (f, v)
    arr["shift_fwd"].t[FRONT] = 6  # a shift above seq_len
    s, nb, out_off, out, overlap = raw_stitch(eng, uni, n, arr, pool, want_out=False)
    assert (s, nb) == (1, 0) and out_off.untouched()
    nbv = ctypes.c_uint64(77)
    assert eng.lib.s2k_unitig_sequences(None, None, None, None, 0, 0, None, None, None, None, 0, ctypes.byref(nbv)) == 1 and nbv.value == 0


def _class_run(eng, parts, l, k, d, mode, mc):
    outs = [_extract_mn(eng, r, l, k, d, mode) for r in parts]
    graph = pkg.KminmerGraph.build(eng, outs, min_count=mc)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, outs)
    out_off, out = ug.sequences(eng, ns)
    h = ns.host()
    blob = b"".join(h[f].tobytes() for f in sorted(h)) + tg._u64(out_off).tobytes() + out.cpu().numpy().tobytes() + ug.overlap.cpu().numpy().tobytes()
    off, text = tg._u64(out_off).tolist(), out.cpu().numpy().tobytes()
    return blob, sorted(min(s, revcomp(s)) for s in (text[a:b] for a, b in zip(off[:-1], off[1:])))


@pytest.mark.gpu
def test_device_deterministic(eng, ecoli):
    """two runs give identical bytes, every array"""
    parts = _split(_flip(tg._sample_reads(ecoli, 300, 7), True), 3)
    runs = [_class_run(eng, parts, 21, 3, 0.05, pkg.HashMode.Regular, 2) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and len(runs[0][1]) > 5


@pytest.mark.gpu
def test_device_reversed_batch_order_same_sequences(eng, ecoli):
    """The same reads in reversed batch order give the same multiset of unitig sequences up to reverse complement (Regular).  The
    representative of a node depends on the order, so this can hold only where every node's occurrences read the same; that is a
    property of the input and is asserted here from the extraction's own arrays (multi_reading_nodes), not assumed.  Read set: E. coli
    fixture, 150 reads of seed 5 (4.5x: min_count 2 leaves gaps, 13 unitigs), every second one reverse-complemented, 12/5/0.05, three
    batches."""
    parts = _split(_flip(tg._sample_reads(ecoli, 150, 5), True), 3)
    batches = [_host_batch(_extract_mn(eng, r, 12, 5, 0.05, pkg.HashMode.Regular)) for r in parts]
    assert multi_reading_nodes(batches, tg.graph_reference(batches, 2)["keys"], 5) == []
    fwd, back = (_class_run(eng, p, 12, 5, 0.05, pkg.HashMode.Regular, 2)[1] for p in (parts, parts[::-1]))
    rc = revcomp(ecoli)
    assert len(fwd) == 13 and fwd == back and all(s in ecoli or s in rc for s in fwd)


@pytest.mark.gpu
def test_device_reversed_batch_order_with_colliding_hashes(eng, ecoli):
    """Where two k-min-mers share a hash the node takes the bytes of whichever comes first (include/s2k.h says so): Regular 21/3/0.05,
    300 reads of seed 7, has 4 such nodes, and reversing the batches changes 2 of its 14 unitig sequences (single-node unitigs of 23
    and 26 / 27 bases).  Checked here: in either order the device gives what the reference gives for that order, every sequence is
    still a slice of the genome, and the sequences that change are those of unitigs that hold such a node."""
    parts = _split(_flip(tg._sample_reads(ecoli, 300, 7), True), 3)
    rc = revcomp(ecoli)
    got, want, touched = [], [], []
    for order in (parts, parts[::-1]):
        batches = [_host_batch(_extract_mn(eng, r, 21, 3, 0.05, pkg.HashMode.Regular)) for r in order]
        g, uni, nodes, seqs = reference_pipeline(batches, 3, 2)
        multi = multi_reading_nodes(batches, g["keys"], 3)
        assert len(multi) == 4
        strings = unitig_strings(uni, seqs)
        canon = [min(s, revcomp(s)) for s in strings]
        touched.append({canon[int(uni["node_unitig"][i])] for i in multi})
        want.append(sorted(canon))
        got.append(_class_run(eng, order, 21, 3, 0.05, pkg.HashMode.Regular, 2)[1])
        assert all(s in ecoli or s in rc for s in strings)
    assert got == want and len(got[0]) > 5
    assert set(got[0]) - set(got[1]) <= touched[0] and set(got[1]) - set(got[0]) <= touched[1]


@pytest.mark.gpu
def test_full_size_genome_sampled_sequences(eng):
    """the genome-sampled set of tools/graph_rate.py (50 Mbp drawn on the device by the generator of tools/graph_rate.py, 150 000 error-free reads of 10 kbp, every
    second one reverse-complemented, Regular l=31 k=10 d=0.01): every stitched unitig equals one slice of the genome or of its reverse
    complement, compared on the device"""
    import sys

    import torch

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from graph_rate import genome_reads
    from unitig_seq_rate import extract_with_minimizers, find_in_genome, genome_of

    dev = torch.device("cuda", 0)
    G = 50_000_000
    bases, read_off, n_reads = genome_reads(torch, dev, G, 10_000, 30, 7)
    out = extract_with_minimizers(eng, pkg, torch, dev, bases, read_off, n_reads, n_reads * 10_000, 31, 10, 0.01, int(pkg.HashMode.Regular))
    graph = pkg.KminmerGraph.build(eng, [out], min_count=2)
    ug = graph.unitigs(eng)
    ns = pkg.NodeSequences.build(eng, graph, [out])
    assert ns.k == 10 and int((ns.seq_len == 0).sum()) == 0
    out_off, seq = ug.sequences(eng, ns)
    del out, bases
    genome = genome_of(torch, dev, G, 7)  # the generator's first draw again: the genome the reads were cut from
    off = out_off.cpu().tolist()
    lens = [b - a for a, b in zip(off[:-1], off[1:])]
    assert ug.n_unitigs >= 1 and max(lens) > 40_000_000 and int(ug.circular.sum()) == 0
    for t in range(ug.n_unitigs):
        assert find_in_genome(torch, genome, seq[off[t]: off[t + 1]]), (t, lens[t])
