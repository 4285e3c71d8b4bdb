"""The tiles' descriptor words by desc_word_kernel (one lane per tile), field by field against the oracle.

On the descriptor path the Hpc family's tiled minimizer kernel leaves a provisional word per tile (its record count, its read starts, whether
a read continues into it, whether one starts exactly at its end) and the raw offsets of the read starts inside the tile; desc_word_kernel
counts the hits of every read segment from the tile's records (a lower bound over their 14-bit tile offsets) and writes the final word and
TileMeta::segstart, which the scan and the k-min-mer kernel read.  The Regular family's tiled kernel still counts and writes the final word
itself; the same cases run in its modes.  Every case below is a batch of a few tiles (tile = 9216 bases) whose k-min-mers, read offsets and
(with the triples) minimizers depend on those counts: read starts per tile from none to past the limit of the segment list, starts at the
edges of a tile, segments with k-2 .. k+1 minimizers behind every p a tile can inherit, a tile without a hit, tiles whose records live in
the overflow region (and a pool too small for them), any byte value, forced chunk counts, a poisoned workspace.

CPU tier: the flagship instantiation, tile_minimizer_kernel<31, Hpc, descriptor path, TILE_MODE_HPC>, has fewer instructions in its body
than the 7199 the commit before this kernel had (s_ 2404, v_ 4046, ds_ 626, global_ 99, flat_ 24; the same listing, counted the same way)."""
import os

import numpy as np
import pytest

from gpu_util import OMODE, compare, pkg, rand_read
from test_tile_sgpr_budget import FLAGSHIP, _body, _isa

gpu = pytest.mark.gpu
HM = pkg.HashMode
MODES = (HM.Hpc, HM.Regular, HM.Simd, HM.HpcSimd)
MODE_IDS = ["hpc", "regular", "simd", "hpcsimd"]
T = 9216
FLAGSHIP_PARAMS = (31, 10, 0.01)  # l, k, density of the benchmark
DENSE_PARAMS = (13, 10, 0.1)      # short reads have a handful of minimizers: windows appear and vanish with single counts
K = 10
PARENT_BODY_INSTRUCTIONS = 7199


def test_flagship_body_has_fewer_instructions_than_before():
    sym, ins = _body(_isa(), FLAGSHIP)
    assert len(ins) < PARENT_BODY_INSTRUCTIONS, len(ins)


def _engine(env):
    """an engine created under the given S2K_* variables (read once, in s2k_create)"""
    for k, v in env.items():
        os.environ[k] = v
    try:
        return pkg.Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def engines():
    """the default engine and one per forced chunk count of the two-stream pipeline"""
    es = {0: pkg.Engine(0)}
    for c in (1, 2, 3, 7):
        es[c] = _engine({"S2K_DESC_CHUNKS": str(c)})
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines[0]


def _reads_of(rng, lens, **kw):
    return [rand_read(rng, int(n), **kw) for n in lens]


def _both(eng, oracle, reads, mode, tag, expect_path="desc", minimizers=False):
    for l, k, d in (FLAGSHIP_PARAMS, DENSE_PARAMS):
        compare(eng, oracle, reads, l, k, d, mode, expect_path=expect_path, minimizers=minimizers, tag=tag)


# ---- read starts per tile --------------------------------------------------------------------------------------------------------------
def _starts_in_tile_one(rng, n):
    """tile 0: one read that runs 50 bases into tile 1; tile 1: n read starts, the last read runs through tile 2 (no start: a `pass`
    tile) into tile 3"""
    if n == 0:
        return _reads_of(rng, [3 * T + 50 + 700], hp=0.1)
    inner = (T - 100) // n
    lens = [T + 50] + [inner] * (n - 1) + [2 * T + 700]
    assert T + 50 + inner * (n - 1) < 2 * T
    return _reads_of(rng, lens, hp=0.1)


@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 29, 30, 31])
def test_read_starts_per_tile(eng, oracle, mode, n):
    rng = np.random.default_rng(700 + n)
    # 31 starts: more than the segment list holds (NBL - 2 = 30): the tiled kernel sends the call through the legacy path
    _both(eng, oracle, _starts_in_tile_one(rng, n), mode, ("starts", n), expect_path="legacy" if n == 31 else "desc")


# ---- a read start at particular places ---------------------------------------------------------------------------------------------------
PLACES = {
    "tile offset 0": [T, T + 500, 900],                     # rs0 == t0 for tile 1 -- and "exactly at the tile end" for tile 0
    "tile offset 1": [T + 1, T + 500, 900],
    "last byte of a tile": [2 * T - 1, 700, T],
    "two starts, at the end and at the end + 1": [T - 300, 300, 1, 2 * T],
    "stream ends on a tile end": [T + 100, T - 100, T],
    "every tile starts a read": [T, T, T],
    "last tile of 1": [T + 500, 2 * T - 500 + 1],
    "last tile of 31": [T + 500, 2 * T - 500 + 31],
    "last tile of 32": [2 * T - 40, 40 + T + 32],
    "last tile of 145": [3 * T - 20, 20 + 145],
    "a read ends with the stream's last tile of 145": [3 * T, 145],
    "empty reads at a tile end": [T, 0, 0, T - 1, 0, 1, 2000],
}


@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("place", sorted(PLACES))
def test_read_start_places(eng, oracle, mode, place):
    rng = np.random.default_rng(900 + sorted(PLACES).index(place))
    _both(eng, oracle, _reads_of(rng, PLACES[place], hp=0.05), mode, place)


# ---- segments with k-2 .. k+1 minimizers, behind every p a tile can inherit --------------------------------------------------------------
def _short_reads_by_count(rng, oracle, mode, l, d, n=4000):
    """random short reads and what the oracle says about them: {minimizer count: [(read, start positions j)]}"""
    reads = _reads_of(rng, rng.integers(40, 260, size=n))
    bases, off = pkg.pack_reads(reads)
    rm = oracle.batch_minimizers(bases, off, l, d, OMODE[mode])
    by = {}
    for i, r in enumerate(reads):
        a, b = int(rm["mn_off"][i]), int(rm["mn_off"][i + 1])
        by.setdefault(b - a, []).append((r, rm["j"][a:b].astype(np.int64)))
    return by


@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_segments_of_k_minus_two_to_k_plus_one_minimizers(eng, oracle, mode):
    l, k, d = DENSE_PARAMS
    rng = np.random.default_rng(811)
    by = _short_reads_by_count(rng, oracle, mode, l, d)
    counts = (k - 2, k - 1, k, k + 1)
    for c in counts:
        assert len(by.get(c, [])) >= 4, (c, sorted(by))
    # (a) whole reads inside a tile: segments that start a read there (two windows, one, none, none)
    inner = [by[c][i][0] for i in range(3) for c in counts]
    reads = [rand_read(rng, T + 300)] + inner + [rand_read(rng, 2 * T)]
    assert T + 300 + sum(len(r) for r in inner) < 2 * T
    compare(eng, oracle, reads, l, k, d, mode, expect_path="desc", tag="whole segments")
    # (b) the FIRST segment of a tile, `dep` set: a read of p + m minimizers put so that p of them start before the tile's first base
    # and the (p+1)-th exactly on it -- p = 0, 1, k-2, k-1 inherited, m = k-2 .. k+1 in the tile
    for p in (0, 1, k - 2, k - 1):
        for m in counts:
            pick = None
            for r, j in by.get(p + m, []):
                if j[p] >= 1 and (p == 0 or j[p] > j[p - 1]):
                    pick = (r, int(j[p]))
                    break
            assert pick, (p, m)
            r, x = pick
            reads = [rand_read(rng, T - x), r, rand_read(rng, 1500), rand_read(rng, T)]
            got = compare(eng, oracle, reads, l, k, d, mode, expect_path="desc", tag=("dep", p, m))
            a, b = int(got["mn_off"][1]), int(got["mn_off"][2])
            assert b - a == p + m and int((got["mn_j"][a:b] < x).sum()) == p, (p, m)
            assert int(got["km_off"][2] - got["km_off"][1]) == max(0, p + m - (k - 1))


# ---- a tile without a hit ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_tile_without_a_hit_between_tiles_with_hits(eng, oracle, mode):
    rng = np.random.default_rng(822)
    one = rand_read(rng, T - 400) + b"A" * (2 * T + 800) + rand_read(rng, T)  # tile 1 lies inside one homopolymer run
    _both(eng, oracle, [one, rand_read(rng, 300)], mode, "N = 0", minimizers=True)
    _both(eng, oracle, [rand_read(rng, 600), one], mode, "N = 0, a start before")


# ---- slab overflow ------------------------------------------------------------------------------------------------------------------------
def _all_hit_unit(rng, oracle, mode, l, d):
    """a repeat unit without equal neighbours (homopolymer compression leaves it alone) all of whose l-mers are minimizers at density d"""
    for _ in range(400):
        p = int(rng.integers(5, 8))
        u = [int(rng.integers(0, 4))]
        while len(u) < p:
            c = int(rng.integers(0, 4))
            if c != u[-1] and not (len(u) == p - 1 and c == u[0]):
                u.append(c)
        if len(u) != p:
            continue
        unit = bytes(b"ACGT"[c] for c in u)
        s = unit * 40
        rm = oracle.batch_minimizers(np.frombuffer(s, dtype=np.uint8), np.array([0, len(s)], dtype=np.uint64), l, d, OMODE[mode])
        if rm["n"] >= len(s) - l - 16:  # (the Simd family may lose a final block of 16)
            return unit
    raise AssertionError("no all-hit unit found")


def _repeat(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_records_in_the_overflow_region(eng, oracle, mode):
    l, k, d = 13, 10, 0.5
    rng = np.random.default_rng(833)
    unit = _all_hit_unit(rng, oracle, mode, l, d)
    # three tiles of ~9200 hits each (the slab holds ~7400 at this density; batches of 192 listed hits): read starts inside them, one at a tile end
    reads = [_repeat(unit, 5000), _repeat(unit, T - 5000 + 3000), _repeat(unit, 40), _repeat(unit, T - 3040), _repeat(unit, T - 7), rand_read(rng, 500)]
    got = compare(eng, oracle, reads, l, k, d, mode, expect_path="desc", tag="overflow region")
    assert got["n_minimizers"] > 3 * 8700
    assert got["counts"]["path"] == 0


@gpu
@pytest.mark.parametrize("mode", (HM.Hpc, HM.Regular), ids=["hpc", "regular"])
def test_overflow_pool_exhausted_is_reported_and_rerun(oracle, mode, capfd):
    l, k, d = 13, 10, 0.5
    rng = np.random.default_rng(844)
    unit = _all_hit_unit(rng, oracle, mode, l, d)
    # six tiles of ~9200 hits: 55 k records for an overflow region of ~38 k: tiles drop their records, the host runs the call again
    reads = [_repeat(unit, 2 * T + 100), _repeat(unit, 600), _repeat(unit, 4 * T - 700)]
    e = _engine({"S2K_TRACE": "1"})
    try:
        capfd.readouterr()
        compare(e, oracle, reads, l, k, d, mode, expect_path="desc", minimizers=False, tag="pool exhausted")
        err = capfd.readouterr().err
    finally:
        e.close()
    assert "re-run: record pool too small" in err, err


# ---- any byte value ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_any_byte_value(eng, oracle, mode):
    rng = np.random.default_rng(855)
    a = np.frombuffer(rand_read(rng, 4 * T + 145), dtype=np.uint8).copy()
    m = rng.random(len(a)) < 0.1
    a[m] = rng.integers(1, 256, size=int(m.sum()))  # any byte value but 0: the segment test is on offsets, not on letters
    cuts = [0, 300, 301, T - 1, T, T + 4000, T + 4100, 2 * T + 1, 3 * T + 9000, len(a)]
    reads = [a[x:y].tobytes() for x, y in zip(cuts[:-1], cuts[1:])]
    _both(eng, oracle, reads, mode, "any byte", minimizers=True)


# ---- forced chunk counts -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_reads():
    """450 tiles (a forced chunk needs 64): reads of 2 .. 40 k bases, so that chunk boundaries fall inside reads, and a few short ones"""
    rng = np.random.default_rng(866)
    lens, tot = [], 0
    while tot < 450 * T:
        n = int(rng.integers(2000, 40000)) if rng.random() < 0.8 else int(rng.integers(0, 400))
        lens.append(n)
        tot += n
    return _reads_of(rng, lens, hp=0.1)


@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("chunks", [1, 2, 3, 7])
def test_forced_chunk_counts(engines, oracle, chunk_reads, mode, chunks):
    l, k, d = FLAGSHIP_PARAMS
    compare(engines[chunks], oracle, chunk_reads, l, k, d, mode, expect_path="desc", minimizers=(chunks == 3), tag=("chunks", chunks))
    # ... and a small batch on the same engine: starts inside tiles, one at a tile end, a partial last tile
    rng = np.random.default_rng(877)
    _both(engines[chunks], oracle, _reads_of(rng, [T + 50, 3000, 2900, 3266, 2 * T + 31], hp=0.1), mode, ("small", chunks))


# ---- a poisoned workspace --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("byte", [0xFF, 0x5A], ids=["0xff", "0x5a"])
def test_poisoned_workspace(oracle, byte):
    """S2K_POISON_WS: the call's workspace (tile words, TileMeta, states, records) is filled with the byte in front of every call's kernels"""
    e = _engine({"S2K_POISON_WS": str(byte)})
    try:
        rng = np.random.default_rng(888)
        for mode in MODES:
            _both(e, oracle, _starts_in_tile_one(rng, 3), mode, ("poison", byte), minimizers=True)
            _both(e, oracle, _starts_in_tile_one(rng, 0), mode, ("poison, pass tile", byte))
            _both(e, oracle, _reads_of(rng, [T, 0, T - 1, 1, 145]), mode, ("poison, edges", byte))
    finally:
        e.close()
