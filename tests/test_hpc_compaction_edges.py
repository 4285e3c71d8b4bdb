"""GPU tier: edge cases of the Hpc tile kernel's run-head compaction (hpc_compact), field by field against the oracle.

The compaction works on 144-byte lane chunks of 9216-byte tiles: pass 1 flags every byte that differs from its predecessor,
pass 2 packs the run heads of eight bytes per step into aligned dwords (a dense and a sparse variant), and the halo code
collects the run heads that follow the tile.  Each case below puts one of their boundaries under test."""
import numpy as np
import pytest

from gpu_util import compare, pkg, rand_read

pytestmark = pytest.mark.gpu
HM = pkg.HashMode
HPC_MODES = (HM.Hpc, HM.HpcSimd)
T, LANE = 9216, 144


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def _check(eng, oracle, reads, tag):
    for mode in HPC_MODES:
        compare(eng, oracle, reads, 31, 10, 0.01, mode, expect_path=0, tag=tag)  # the flagship's compile-time l
        compare(eng, oracle, reads, 13, 4, 0.1, mode, expect_path=0, tag=tag)  # a run-time l


def test_runs_longer_than_a_lane_and_across_tiles(eng, oracle):
    rng = np.random.default_rng(101)
    parts = [rand_read(rng, 200)]
    for run in (145, 288, 289, 500):  # longer than a lane's chunk
        parts += [b"G" * run, rand_read(rng, int(rng.integers(50, 400)))]
    one = b"".join(parts)
    one += rand_read(rng, T - 70 - len(one)) + b"T" * 140 + rand_read(rng, 3000)  # a run that straddles the first tile boundary
    two = rand_read(rng, T - 1) + b"C" * 2 + rand_read(rng, T - 1) + b"A" * 3 + rand_read(rng, 500)  # runs of 2 and 3 ending a tile's last byte
    _check(eng, oracle, [one, two], "long-runs")


def test_read_starts_at_the_first_and_last_byte_of_a_lane(eng, oracle):
    rng = np.random.default_rng(102)
    # the stream is the concatenation of the reads: read starts at lane offsets 0 and 143, in several lanes and tiles
    lens = [LANE * 3, LANE - 1, 1, LANE * 5 - 1, LANE, T - 10 * LANE, LANE + 143, 5000, LANE * 7, 143, 1, 2000]
    reads = [rand_read(rng, n) for n in lens]
    _check(eng, oracle, reads, "lane-starts")
    # the same with reads that end in the run of the next read's first base
    reads = [r[:-1] + r[:1] * 3 if len(r) > 1 else r for r in reads]
    _check(eng, oracle, reads, "lane-starts-runs")


def test_more_than_63_read_starts_in_a_tile(eng, oracle):
    rng = np.random.default_rng(103)
    reads = [rand_read(rng, int(n), hp=0.2) for n in rng.integers(40, 120, size=400)]
    _check(eng, oracle, reads, "many-starts")


def test_non_acgt_bytes(eng, oracle):
    rng = np.random.default_rng(104)
    a = np.frombuffer(rand_read(rng, 3 * T), dtype=np.uint8).copy()
    m = rng.random(len(a)) < 0.1
    a[m] = rng.integers(1, 256, size=int(m.sum()))  # any byte value but 0
    # neighbours whose bytes differ by XOR 0x0C, 0x80 or 0xFF only (A/M, C/O, G/K, ...)
    for i, (x, y) in enumerate(((0x41, 0x4D), (0x43, 0x4F), (0x47, 0x4B), (0x54, 0x58), (0x41, 0xC1), (0x01, 0xFE), (0x0C, 0x0D))):
        for j in range(50):
            p = 79 * (50 * i + j) + 11  # (< 3 T - 4)
            a[p : p + 4] = (x, y, y, x)
    _check(eng, oracle, [a.tobytes(), rand_read(rng, 700, odd=0.3)], "odd-bytes")


def test_partial_last_tile_and_sparse_tiles(eng, oracle):
    rng = np.random.default_rng(105)
    # sparse tiles (HiFi-like: long runs, < 0.6 run heads per base) and dense ones, and a stream whose last tile is partial
    sparse = [rand_read(rng, int(n), hp=0.95) for n in (T + 77, 2 * T + 1, 12345)]
    dense = [rand_read(rng, int(n)) for n in (T - 1, 3 * T + 143, 100)]
    _check(eng, oracle, sparse, "sparse")
    _check(eng, oracle, dense, "dense")
    _check(eng, oracle, sparse + dense, "mixed")
