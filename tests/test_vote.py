"""Majority-vote representatives of the graph's nodes on the device: s2k_table_vote_keys, s2k_table_vote_representatives and
s2k_vote_ordinals (include/s2k.h).  The rule, restated serially (`vote_keys_reference`, `vote_reference`):

An occurrence x of node i (an item whose hash is key i) with bytes B, rev, shift_fwd, shift_rev has three readings: whole = B if rev
== 0 else revcomp(B), tag 4 i; forward end = B[:shift_fwd], tag 4 i + 2 + rev; reverse end = revcomp(B[len - shift_rev:]), tag 4 i + 2 +
(1 - rev).  F(s) is the Horner loop F = F * M + s_j + 1 mod 2^64 with M = 0x9E3779B97F4A7C15; the vote key of a reading is mix64(F ^
mix64(tag)) with the splitmix64 finaliser.  votes(key) counts the occurrences of all batches that gave the key; the score of x is
(votes(whole), votes(forward end) + votes(reverse end)); the representative of a node is its occurrence with the largest score, the
smallest global ordinal among equals.  The device packs min(w, 2047) << 52 | min(e, 4095) << 40 | (2^40 - 1 - ordinal) and takes the
maximum, so the reference saturates the same way."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import test_bridge as tb
import test_graph as tg
import test_unitig_sequences as tus
import test_unitigs as tu
from conftest import ROOT
from s2k_loader import import_package

pkg = import_package()

SYMS = ("s2k_table_vote_keys", "s2k_table_vote_representatives", "s2k_vote_ordinals")
M = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
ORD = (1 << 40) - 1
NONE64 = tus.NONE64
revcomp = tus.revcomp


# ---- the references ----------------------------------------------------------------------------------------------------------------
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def horner(s):
    f = 0
    for c in bytes(s):
        f = (f * M + c + 1) & MASK
    return f


_POW = [np.array([1], dtype=np.uint64)]
_F = {}


def _pow(n):
    """M^0 .. M^(n - 1) as uint64 (the products wrap)"""
    if len(_POW[0]) < n:
        p, x = [], 1
        for _ in range(max(n, 2 * len(_POW[0]))):
            p.append(x)
            x = (x * M) & MASK
        _POW[0] = np.array(p, dtype=np.uint64)
    return _POW[0][:n]


def fingerprint(s):
    """F(s) as the sum of (s_j + 1) M^(n - 1 - j), kept per distinct string (test_fingerprint_combines holds it against the loop)"""
    s = bytes(s)
    f = _F.get(s)
    if f is None:
        a = np.frombuffer(s, dtype=np.uint8).astype(np.uint64) + np.uint64(1)
        f = _F[s] = int((a * _pow(len(s))[::-1]).sum(dtype=np.uint64)) if len(s) else 0
    return f


def occurrences(b, k):
    """every item of a batch, in item order -> (hash, B, rev, shift_fwd, shift_rev)"""
    km, mn = [int(x) for x in b["km_off"]], [int(x) for x in b["mn_off"]]
    for r in range(len(km) - 1):
        items = km[r + 1] - km[r]
        assert items == 0 or mn[r + 1] - mn[r] == items + k - 1  # the count relation
        base = int(b["read_off"][r])
        for j in range(items):
            t, x = mn[r] + j, km[r] + j
            first, last = int(b["mn_j"][t]), int(b["mn_jend"][t + k - 1])
            B = bytes(b["bases"][base + first: base + last + 1])
            yield int(b["hash"][x]), B, int(b["rev"][x]), int(b["mn_j"][t + 1]) - first, last - int(b["mn_jend"][t + k - 2])


def reading_keys(i, B, rev, sf, sr):
    whole = B if rev == 0 else revcomp(B)
    fwd, rve = B[:sf], revcomp(B[len(B) - sr:])
    return [mix64(fingerprint(s) ^ mix64(tag)) for s, tag in ((whole, 4 * i), (fwd, 4 * i + 2 + rev), (rve, 4 * i + 2 + (1 - rev)))]


def vote_keys_reference(b, keys, k):
    """the key stream of one batch: whole, forward end, reverse end of every item whose hash is in `keys`, in item order"""
    index = {int(h): i for i, h in enumerate(keys)}
    out = []
    for h, B, rev, sf, sr in occurrences(b, k):
        if h in index:
            out += reading_keys(index[h], B, rev, sf, sr)
    return np.array(out, dtype=np.uint64)


def vote_reference(batches, keys, k):
    """-> dict: streams (per batch), vote_keys / vote_counts (the counted table, ascending), best (the packed words) and rep"""
    streams = [vote_keys_reference(b, keys, k) for b in batches]
    votes = collections.Counter()
    for s in streams:
        votes.update(s.tolist())
    best = [0] * len(keys)
    index = {int(h): i for i, h in enumerate(keys)}
    ordinal = 0
    for b, s in zip(batches, streams):
        p = 0
        for h, *_ in occurrences(b, k):
            if h in index:
                w, e = votes[int(s[p])], votes[int(s[p + 1])] + votes[int(s[p + 2])]
                p += 3
                best[index[h]] = max(best[index[h]], min(w, 2047) << 52 | min(e, 4095) << 40 | (ORD - ordinal))
            ordinal += 1
    vk = sorted(votes)
    return {"streams": streams, "vote_keys": np.array(vk, dtype=np.uint64), "vote_counts": np.array([votes[x] for x in vk], dtype=np.uint32),
            "best": np.array(best, dtype=np.uint64), "rep": np.array([ORD - (x & ORD) if x else int(NONE64) for x in best], dtype=np.uint64)}


def nodes_from_rep(batches, keys, k, rep):
    """the node records and the pool for given representatives (tus.node_sequences_reference with the choice made elsewhere)"""
    want = {int(o): i for i, o in enumerate(rep) if o != NONE64}
    out = {f: np.zeros(len(keys), dtype=dt) for f, dt in tus.NODE_DT.items()}
    pool, ordinal = bytearray(), 0
    for b in batches:
        for h, B, rev, sf, sr in occurrences(b, k):
            i = want.get(ordinal)
            if i is not None:
                assert int(keys[i]) == h
                out["seq_off"][i], out["seq_len"][i], out["rev"][i], out["shift_fwd"][i], out["shift_rev"][i] = len(pool), len(B), rev, sf, sr
                pool += B
            ordinal += 1
    out["rep"], out["pool"] = np.asarray(rep, dtype=np.uint64), np.frombuffer(bytes(pool), dtype=np.uint8)
    return out


# ---- hand-made inputs: k = 2, every byte written out --------------------------------------------------------------------------------
READ = tus.READ  # ACGTTGCA: item 0 = ACGTT (node 10), item 1 = TTGCA (node 20)
ODD = b"ACCTTGCA"  # item 0 reads ACCTT


def fwd(seq, hashes=(10, 20)):
    return (seq, [0, 3, 5], [1, 4, 7], list(hashes), [0, 0])


# the other strand of READ: TGCAACGT, minimizers TGC@0-2, AA@3-4, GT@6-7; item 0 = TGCAA (node 20), item 1 = AACGT (node 10)
TWIN = (b"TGCAACGT", [0, 3, 6], [2, 4, 7], [20, 10], [1, 1])


def mid(seq):
    """one item of two overlapping minimizers @0-5 and @2-7: the ends are seq[:2] and seq[6:], bytes 2 .. 5 are in neither"""
    return (seq, [0, 2], [5, 7], [10], [0])


def _long_read(edit=None):
    rng = np.random.default_rng(11)
    x = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, size=3000)].copy()
    if edit is not None:
        x[edit] = ord("a")
    return (x.tobytes(), [5, 80, 1200, 2900], [9, 84, 1204, 2904], [10, 20, 30], [0, 1, 0])


HB = tus.hand_batch
HANDV = {
    # name: (batches, keys, rep)
    "first occurrence differs": ([HB([fwd(ODD), fwd(READ), fwd(READ)])], [10, 20], [2, 1]),
    "majority on the other strand": ([HB([fwd(ODD), TWIN, TWIN])], [10, 20], [3, 1]),
    "a tie goes to the earliest": ([HB([fwd(ODD), fwd(READ)])], [10, 20], [0, 1]),
    "the ends decide": ([HB([mid(b"AGAAAATT"), mid(b"ACCCCCTT"), mid(b"ACGGGGTT")])], [10], [1]),
    "N inside a piece": ([HB([fwd(READ), fwd(b"ACNTTGCA"), fwd(b"ACNTTGCA")])], [10, 20], [2, 1]),
    "reads without items": ([HB([(b"", [], [], [], []), fwd(ODD), (b"GG", [0], [1], [], []), fwd(READ), (b"", [], [], [], []), fwd(READ)])],
                            [10, 20], [2, 1]),
    "an item that is no node": ([HB([fwd(ODD, (10, 30)), fwd(READ, (10, 30)), fwd(READ)])], [10, 20], [2, 5]),
    "a key that never occurs": ([HB([fwd(ODD), fwd(READ), fwd(READ)])], [10, 15, 20], [2, int(NONE64), 1]),
    "votes over two batches": ([HB([fwd(ODD)]), HB([fwd(READ), fwd(READ)])], [10, 20], [2, 1]),
    "long pieces": ([HB([_long_read(100), _long_read(), _long_read(2000), _long_read()])], [10, 20, 30], [0, 4, 2]),
}


def seam_batch(counts, seed):
    """reads of the given item counts, k = 2: minimizers of 2 bytes every 3, item j = 5 bytes; the bytes repeat with a period of 8 items
    and the node follows them, so that nodes have many occurrences; every 11th item is no node; some bytes are substituted"""
    rng = np.random.default_rng(seed)
    pat = np.frombuffer(b"ACGTTGCAAGGCTTACCGATNACG", dtype=np.uint8)
    reads = []
    for n in counts:
        if n == 0:
            reads.append((b"ACGT", [1], [2], [], []))
            continue
        x = np.tile(pat, (3 * n + 5) // len(pat) + 1)[:3 * n + 5].copy()
        x[rng.random(len(x)) < 0.01] = ord("t")
        j = np.arange(n)
        reads.append((x.tobytes(), (3 * np.arange(n + 1)).tolist(), (3 * np.arange(n + 1) + 1).tolist(),
                      np.where(j % 11 == 10, 999, 100 + j % 8).tolist(), ((j // 8) % 3 == 1).astype(int).tolist()))
    return HB(reads)


SEAM_KEYS = list(range(100, 108))
SEAMS = [[63], [64], [65], [2047], [2048], [2049], [30, 34], [40, 0, 25], [2000, 48], [2040, 9], [1, 2047, 1]]


def saturated():
    """node 10 read 2 101 times, the odd reading first: every other occurrence has w saturated at 2 047, the earliest of them wins"""
    return [HB([fwd(ODD)] + [fwd(READ)] * 2100)], [10, 20], [2, 1]


# ---- CPU tier ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "s2k.h")).read()
    for s in SYMS:
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS and s + "(" in header, s
    for m in ("table_vote_keys", "table_vote_representatives", "vote_ordinals"):
        assert hasattr(pkg.Engine, m), m
    mk = open(os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc", "Makefile")).read()
    assert "s2k_vote.hip" in mk.split("SRCS")[1].split("\n")[0]
    assert "0x9E3779B97F4A7C15" in header and "0xBF58476D1CE4E5B9" in header and "0x94D049BB133111EB" in header


def test_cpp_vote_facade_compiles_and_links(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = str(tmp_path / "vote_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "vote_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_fingerprint_combines():
    """F(a || b) from F(a) and F(b), the reverse-complement reading from the mirrored sum, both against the Horner loop"""
    rng = np.random.default_rng(3)
    assert horner(b"") == 0 and horner(b"A") == 66 and horner(b"AC") == (66 * M + 68) & MASK
    assert mix64(0) == 0 and len({mix64(x) >> 56 for x in range(64)}) > 40  # small tags reach the top bits
    for _ in range(50):
        a = bytes(rng.integers(0, 256, size=int(rng.integers(0, 40)), dtype=np.uint8))
        b = np.frombuffer(b"ACGTacgtNx", dtype=np.uint8)[rng.integers(0, 10, size=int(rng.integers(0, 300)))].tobytes()
        assert fingerprint(a) == horner(a) and fingerprint(b) == horner(b)
        assert horner(a + b) == (horner(a) * pow(M, len(b), 1 << 64) + horner(b)) & MASK
        mirrored = sum((c + 1) * pow(M, j, 1 << 64) for j, c in enumerate(tus._RC[np.frombuffer(b, dtype=np.uint8)].tolist())) & MASK
        assert horner(revcomp(b)) == mirrored


@pytest.mark.parametrize("name", list(HANDV))
def test_reference_hand_made(name):
    batches, keys, rep = HANDV[name]
    ref = vote_reference(batches, keys, 2)
    assert ref["rep"].tolist() == rep, name
    n_items = sum(sum(1 for h, *_ in occurrences(b, 2) if h in keys) for b in batches)
    assert sum(len(s) for s in ref["streams"]) == 3 * n_items == int(ref["vote_counts"].sum())
    if name == "first occurrence differs":
        assert tus.node_sequences_reference(batches, keys, 2)["rep"].tolist() == [0, 1]  # the earliest: what the vote moves
        w, e = int(ref["best"][0]) >> 52, (int(ref["best"][0]) >> 40) & 4095
        assert (w, e) == (2, 4)  # ACGTT twice; ACG twice and revcomp(GTT) twice
        s = ref["streams"][0]
        assert s[0] != s[6] and s[6] == s[12] and s[3] == s[9] == s[15]  # item 0 of the three reads; item 1 reads the same in all
    if name == "majority on the other strand":
        assert nodes_from_rep(batches, keys, 2, ref["rep"])["rev"].tolist() == [1, 0]
    if name == "the ends decide":
        assert [int(x) >> 52 for x in ref["best"]] == [1] and len(set(ref["streams"][0][0::3].tolist())) == 3
    if name == "votes over two batches":
        one = vote_reference([HB([fwd(ODD), fwd(READ), fwd(READ)])], keys, 2)
        assert one["rep"].tolist() == rep and np.array_equal(one["vote_keys"], ref["vote_keys"])


def test_reference_saturates_like_the_packed_word():
    batches, keys, rep = saturated()
    ref = vote_reference(batches, keys, 2)
    assert ref["rep"].tolist() == rep and int(ref["best"][0]) >> 52 == 2047 and (int(ref["best"][0]) >> 40) & 4095 == 4095
    assert int(ref["vote_counts"].max()) == 2101


@pytest.mark.parametrize("case", tus.ECOLI, ids=lambda c: "%s-%d-%d-%dreads-mc%d%s" % (c[0], c[1], c[2], c[4], c[6], "-flip" if c[7] else ""))
def test_error_free_reads_vote_for_the_earliest(oracle, ecoli, case):
    mode, l, k, d, n, seed, mc, flip, _ = case
    b = tus._oracle_batch(oracle, tus._flip(tg._sample_reads(ecoli, n, seed), flip), l, k, d, pkg.HashMode[mode])
    keys = tg.graph_reference([b], mc)["keys"]
    ref, early = vote_reference([b], keys, k), tus.node_sequences_reference([b], keys, k)
    multi = set(tus.multi_reading_nodes([b], keys, k))
    same = [i for i in range(len(keys)) if i not in multi]
    assert len(same) > 100 and np.array_equal(ref["rep"][same], early["rep"][same])


# (mode, l, k, d): 600 reads of the fixture, every second one on the other strand, 0.5 % substitutions, min_count 3
NOISY = [("Regular", 21, 3, 0.05), ("Hpc", 21, 3, 0.05), ("Regular", 12, 5, 0.05)]
CLEAN = ("Regular", 21, 3, 0.05)
_CASES = {}


def ecoli_case(oracle, ecoli, case, noisy=True):
    """one input as one batch and as two, its graph and both choices of representatives, computed once"""
    key = (case, noisy)
    if key not in _CASES:
        mode, l, k, d = case
        reads = tus._flip(tg._sample_reads(ecoli, 600 if noisy else 150, 7), True)
        mc = 3 if noisy else 2
        if noisy:
            reads = tb.substituted(reads, 0.005, 2)
        one = [tus._oracle_batch(oracle, reads, l, k, d, pkg.HashMode[mode])]
        two = [tus._oracle_batch(oracle, r, l, k, d, pkg.HashMode[mode]) for r in (reads[:len(reads) // 2 + 1], reads[len(reads) // 2 + 1:])]
        g = tg.graph_reference(one, mc)
        _CASES[key] = {"reads": reads, "k": k, "mc": mc, "one": one, "two": two, "g": g, "keys": g["keys"],
                       "uni": tu.unitig_reference(g["row_off"], g["dst"], len(g["keys"])),
                       "ref1": vote_reference(one, g["keys"], k), "ref2": vote_reference(two, g["keys"], k)}
    return _CASES[key]


def exact_bases(uni, nodes, ecoli, rc):
    """-> (unitigs, unitigs that are substrings of the genome or its reverse complement, the bases in them, all bases, strings)"""
    strings = tus.unitig_strings(uni, tus.unitig_sequences_reference(uni, nodes))
    ok = [s for s in strings if s in ecoli or s in rc]
    return len(strings), len(ok), sum(map(len, ok)), sum(map(len, strings)), strings


@pytest.mark.parametrize("case", NOISY, ids=lambda c: "%s-%d-%d" % c[:3])
def test_noisy_reads_the_vote_restores_the_genome(oracle, ecoli, case):
    """measured with exact byte strings as vote keys (unitigs / exact unitigs / bases in them of all / inconsistent links), earliest ->
    voted: Regular 21/3: 33: 23 / 11 147 of 99 584 / 6 -> 29 / 99 220 of 99 552 / 0; Hpc 21/3: 25: 11 / 1 318 of 99 459 / 83 -> 22 /
    99 074 of 99 401 / 0; Regular 12/5: 38: 16 / 4 917 of 100 340 / 29 -> 27 / 99 263 of 100 345 / 0"""
    c = ecoli_case(oracle, ecoli, case)
    rc = revcomp(ecoli)
    early = tus.node_sequences_reference(c["one"], c["keys"], c["k"])
    voted = nodes_from_rep(c["one"], c["keys"], c["k"], c["ref1"]["rep"])
    n, ne, be, ae, _ = exact_bases(c["uni"], early, ecoli, rc)
    _, nv, bv, av, _ = exact_bases(c["uni"], voted, ecoli, rc)
    le, lv = tus._links_consistent(c["uni"], early), tus._links_consistent(c["uni"], voted)
    moved = int((early["rep"] != voted["rep"]).sum())
    print("%s: %d unitigs; earliest %d exact, %d of %d bases, %d inconsistent links; voted %d exact, %d of %d bases, %d links; %d representatives "
          "move" % (case, n, ne, be, ae, le, nv, bv, av, lv, moved))
    assert lv == 0 and bv >= 0.95 * av
    assert be < 0.20 * ae
    assert np.array_equal(c["ref1"]["rep"], c["ref2"]["rep"])  # one batch and two: the same representatives
    assert np.array_equal(c["ref1"]["vote_keys"], c["ref2"]["vote_keys"]) and np.array_equal(c["ref1"]["vote_counts"], c["ref2"]["vote_counts"])


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


Guarded = tus.Guarded


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def raw_keys(eng, t, b, d, k, keys_out, capacity, i=None):
    """s2k_table_vote_keys through ctypes -> (status, n_keys)"""
    nk = ctypes.c_uint64(77)
    s = eng.lib.s2k_table_vote_keys(ctypes.c_void_p(t.handle), len(b["km_off"]) - 1, ctypes.byref(i or tus._in_struct(b, d)), k, _ptr(d["bases"]),
                                    _ptr(d["read_off"]), ctypes.c_void_p(keys_out.ptr) if keys_out is not None else None, capacity, ctypes.byref(nk))
    return s, nk.value


def raw_best(eng, t, vt, b, d, k, base, best, i=None):
    return eng.lib.s2k_table_vote_representatives(ctypes.c_void_p(t.handle), ctypes.c_void_p(vt.handle), len(b["km_off"]) - 1,
                                                  ctypes.byref(i or tus._in_struct(b, d)), k, _ptr(d["bases"]), _ptr(d["read_off"]), base,
                                                  ctypes.c_void_p(best.ptr))


def dev_batch(b, shift=0):
    """tus._dev_batch; shift > 0 puts the bases that many bytes past a 16-byte boundary"""
    import torch

    d = tus._dev_batch(b)
    if shift:
        whole = torch.cat([torch.full((16 + shift,), 0x41, dtype=torch.uint8, device="cuda:0"), d["bases"], torch.full((40,), 0x43, dtype=torch.uint8, device="cuda:0")])
        off = (-whole.data_ptr()) % 16 + shift
        d["_whole"], d["bases"] = whole, whole[off: off + len(b["bases"])]
        d["bases"].copy_(torch.from_numpy(np.array(b["bases"], dtype=np.uint8)))
        assert d["bases"].data_ptr() % 16 == shift
    return d


def check_device(eng, batches, keys, k, ref, tag, shift=0):
    """the whole protocol through the raw ABI, every output between guards and equal to the reference byte for byte -> the outputs' bytes"""
    import torch

    t = tg._table(eng, keys, None)
    devs = [dev_batch(b, shift) for b in batches]
    counter = pkg.KminmerCounter(eng)
    torch.cuda.synchronize()
    blob = b""
    for b, d, want in zip(batches, devs, ref["streams"]):
        assert raw_keys(eng, t, b, d, k, None, 0) == (0, len(want)), tag  # the size only
        out = Guarded(len(want), np.uint64)
        torch.cuda.synchronize()  # the library's stream does not follow torch's
        assert raw_keys(eng, t, b, d, k, out, len(want)) == (0, len(want)), tag
        assert out.intact() and out.host().tobytes() == want.tobytes(), tag
        counter.add(out.ptr if len(want) else 0, len(want))
        blob += out.host().tobytes()
    vk, vc = counter.finish(1)
    counter.close()
    assert tg._u64(vk).tobytes() == ref["vote_keys"].tobytes() and vc.cpu().numpy().view(np.uint32).tobytes() == ref["vote_counts"].tobytes(), tag
    vt = pkg.CountTable(eng, vk, vc)
    best = Guarded(len(keys), np.uint64, init=0)
    torch.cuda.synchronize()
    base = 0
    for b, d in zip(batches, devs):
        assert raw_best(eng, t, vt, b, d, k, base, best) == 0, (tag, eng.lib.s2k_last_error(eng.ctx))
        base += int(b["km_off"][-1])
    assert best.intact() and best.host().tobytes() == ref["best"].tobytes(), tag
    rep = Guarded(len(keys), np.uint64)
    torch.cuda.synchronize()
    assert eng.lib.s2k_vote_ordinals(eng.ctx, ctypes.c_void_p(best.ptr), len(keys), ctypes.c_void_p(rep.ptr)) == 0
    assert rep.intact() and rep.host().tobytes() == ref["rep"].tobytes(), tag
    vt.close()
    t.close()
    return blob + best.host().tobytes() + rep.host().tobytes()


@pytest.mark.gpu
def test_cpp_vote_facade_runs(eng, tmp_path):
    test_cpp_vote_facade_compiles_and_links(tmp_path)
    assert subprocess.check_output([str(tmp_path / "vote_facade")], text=True) == "vote ok refused 1 1 0\n"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HANDV))
def test_device_hand_made(eng, name):
    batches, keys, rep = HANDV[name]
    ref = vote_reference(batches, keys, 2)
    first = check_device(eng, batches, keys, 2, ref, name)
    assert check_device(eng, batches, keys, 2, ref, name) == first  # two calls, bit-identical
    for shift in (1, 8, 15):
        assert check_device(eng, batches, keys, 2, ref, (name, shift), shift) == first


@pytest.mark.gpu
@pytest.mark.parametrize("counts", SEAMS, ids=lambda c: "-".join(map(str, c)))
def test_device_wave_and_tile_seams(eng, counts):
    batches = [seam_batch(counts, 5)]
    ref = vote_reference(batches, SEAM_KEYS, 2)
    assert len(ref["streams"][0]) == 3 * (sum(counts) - sum(n // 11 for n in counts))
    first = check_device(eng, batches, SEAM_KEYS, 2, ref, counts)
    assert check_device(eng, batches, SEAM_KEYS, 2, ref, counts, 5) == first
    if len(counts) > 1:  # and reads of the same sizes in two batches
        two = [seam_batch(counts[:1], 5), seam_batch(counts[1:], 6)]
        check_device(eng, two, SEAM_KEYS, 2, vote_reference(two, SEAM_KEYS, 2), (counts, "two"))


@pytest.mark.gpu
def test_device_saturated_votes(eng):
    batches, keys, rep = saturated()
    ref = vote_reference(batches, keys, 2)
    assert ref["rep"].tolist() == rep
    check_device(eng, batches, keys, 2, ref, "saturated")


@pytest.mark.gpu
@pytest.mark.parametrize("case,noisy", [(c, True) for c in NOISY] + [(CLEAN, False)], ids=lambda c: "%s-%d-%d" % c[:3] if isinstance(c, tuple) else str(c))
def test_device_ecoli(eng, oracle, ecoli, case, noisy):
    c = ecoli_case(oracle, ecoli, case, noisy)
    check_device(eng, c["one"], c["keys"], c["k"], c["ref1"], (case, 1))
    check_device(eng, c["two"], c["keys"], c["k"], c["ref2"], (case, 2))


@pytest.mark.gpu
def test_device_refusals_write_nothing(eng):
    import torch

    batches, keys, _ = HANDV["first occurrence differs"]
    b, other = batches[0], seam_batch([7], 1)
    ref = vote_reference(batches, keys, 2)
    n = len(ref["streams"][0])
    t = tg._table(eng, keys, None)
    d, od = dev_batch(b), dev_batch(other)
    out, best = Guarded(n, np.uint64), Guarded(len(keys), np.uint64)
    torch.cuda.synchronize()
    assert raw_keys(eng, t, b, d, 3, out, n) == (1, 0) and raw_keys(eng, t, b, d, 1, out, n) == (1, 0)  # a wrong k
    i = tus._in_struct(b, d)
    i.mn_capacity = int(other["mn_off"][-1])
    for f in ("mn_off", "mn_j", "mn_jend"):
        setattr(i, f, od[f].data_ptr())
    assert raw_keys(eng, t, b, d, 2, out, n, i) == (1, 0)  # the triples of another call
    assert raw_keys(eng, t, b, d, 2, out, n - 1) == (7, n)  # capacity one short
    assert out.untouched()
    assert raw_keys(eng, t, b, d, 2, out, n) == (0, n)
    vk = np.sort(out.host())
    votes_here = pkg.CountTable(eng, tg._dev(vk[:1], torch.int64)[:0], None)  # no key at all
    elsewhere = pkg.CountTable(eng, tg._dev(np.unique(vote_keys_reference(other, SEAM_KEYS, 2))[:5], torch.int64), None)
    good = pkg.CountTable(eng, tg._dev(np.unique(vk), torch.int64), None)
    torch.cuda.synchronize()
    for vt in (votes_here, elsewhere):
        assert raw_best(eng, t, vt, b, d, 2, 0, best) == 1  # a vote table from other batches
    assert raw_best(eng, t, good, b, d, 3, 0, best) == 1 and raw_best(eng, t, good, b, d, 2, 0, best, i) == 1
    assert raw_best(eng, t, good, b, d, 2, (1 << 40) - int(b["km_off"][-1]) + 1, best) == 1  # ordinal_base + items past 2^40
    assert best.untouched()
    zero = Guarded(len(keys), np.uint64, init=0)
    torch.cuda.synchronize()
    assert raw_best(eng, t, good, b, d, 2, (1 << 40) - int(b["km_off"][-1]), zero) == 0 and zero.intact()  # the last ordinals there are
    assert (zero.host() & np.uint64(ORD)).tolist() == [ORD - ((1 << 40) - 6), ORD - ((1 << 40) - 5)]  # every reading once: the earliest
    for x in (votes_here, elsewhere, good, t):
        x.close()


@pytest.mark.gpu
def test_build_with_vote_end_to_end(eng, oracle, ecoli, tmp_path):
    """NodeSequences.build(vote=True) on the noisy Regular 21/3 reads into UnitigGraph.sequences, walks and write_gaf: the stitched
    strings are the reference's; vote=False is what the earliest-occurrence rule gives"""
    import test_walk as tw

    case = NOISY[0]
    c = ecoli_case(oracle, ecoli, case)
    mode, l, k, d = case
    half = len(c["reads"]) // 2 + 1
    outs = [tw._extract_all(eng, r, l, k, d, pkg.HashMode[mode]) for r in (c["reads"][:half], c["reads"][half:])]
    graph = pkg.KminmerGraph.build(eng, outs, min_count=c["mc"], min_edge_count=1)
    assert tg._u64(graph.keys).tobytes() == c["keys"].tobytes()
    ug = graph.unitigs(eng)
    voted = pkg.NodeSequences.build(eng, graph, outs, vote=True)
    want = nodes_from_rep(c["two"], c["keys"], k, c["ref2"]["rep"])
    h = voted.host()
    for f in list(tus.NODE_DT) + ["rep", "pool"]:
        assert h[f].tobytes() == np.asarray(want[f], dtype=h[f].dtype).tobytes(), f
    out_off, out = ug.sequences(eng, voted)
    seqs = tus.unitig_sequences_reference(c["uni"], want)
    assert tg._u64(out_off).tobytes() == seqs["out_off"].tobytes() and out.cpu().numpy().tobytes() == seqs["out"].tobytes()
    rc = revcomp(ecoli)
    strings = tus.unitig_strings(c["uni"], seqs)
    assert sum(len(s) for s in strings if s in ecoli or s in rc) >= 0.95 * sum(map(len, strings))
    table = pkg.CountTable(eng, graph.keys, graph.counts)
    paths = ug.thread(eng, table, outs[0], half, min_count=c["mc"])
    table.close()
    walks = ug.walks(eng, paths, voted)
    w, ph = walks.host(), paths.host()
    lens = np.diff(tg._u64(out_off).astype(np.int64))
    ovl = ug.overlap.cpu().numpy().view(np.uint32).astype(np.int64)
    assert walks.n_walks > 100
    for x in range(walks.n_walks):  # path_len from the stitched lengths: every step but the last advances by L - overlap
        s0, ns = int(w["first_step"][x]), int(w["n_steps"][x])
        u = ph["unitig"][s0: s0 + ns].astype(np.int64)
        adv = lens[u[:-1] >> 1] - np.minimum(ovl[u[:-1]], lens[u[:-1] >> 1])
        assert int(w["path_len"][x]) == int(adv.sum()) + int(lens[u[-1] >> 1]), x
    p = str(tmp_path / "voted.gaf")
    walks.write_gaf(p, ug)
    assert len(open(p).read().split("\n")) == walks.n_walks + 1
    early = pkg.NodeSequences.build(eng, graph, outs, vote=False)
    plain = pkg.NodeSequences.build(eng, graph, outs)
    ref = tus.node_sequences_reference(c["two"], c["keys"], k)
    eh, ph2 = early.host(), plain.host()
    for f in list(tus.NODE_DT) + ["rep", "pool"]:
        assert eh[f].tobytes() == ph2[f].tobytes() == np.asarray(ref[f], dtype=eh[f].dtype).tobytes(), f
