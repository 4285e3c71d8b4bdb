"""GPU tier: the static hash loop (hash_loop_static / hash_steps) at every compile-time l and in both scalar families, field by field
against the oracle, on batches of three tiles (27 648 bases).

The loop is one unrolled schedule per l: a first group of seed look-ups in front of it, a warm-up of l steps (Hpc: from the
pre-rotated table, two bases per step), one early exit per 16-position piece for compacted tiles of np = 1, 3, 5, 7 pieces per lane,
and a last position that is tested only.  Its LDS waits are counted ones (tools/isa/check_lgkmcnt.py): a wrong count shows as a
wrong hash, not as a fault, so every one of these paths is compared here.  Shapes:
  * run lengths that make the compacted Hpc tile end in each piece count: runs of 10 equal bases (np = 1), of 4 and 3 (np = 3),
    of 2 (np = 5), uniform ACGT (0.75 run heads per base, np = 7), no two equal neighbours (np = 9);
  * a read that starts in the first and one that starts in the last lane of a tile;
  * a last tile of 1, 31, 32 and 145 bases."""
import re

import numpy as np
import pytest

from conftest import ROOT
from gpu_util import compare, pkg, rand_read

pytestmark = pytest.mark.gpu
HM = pkg.HashMode
T, LANE = 9216, 144
STATIC_LS = [int(x) for x in re.findall(r"X\((\d+)\)", open(ROOT + "/rust-seq2kminmers_amd/csrc/s2k_static_l.h").read())]


def runs(rng, n, run):
    """n bases in runs of `run` equal bases, neighbouring runs different (run = 1: no two equal neighbours)"""
    m = (n + run - 1) // run
    step = rng.integers(1, 4, size=m)  # 1 .. 3: never the base before
    idx = np.cumsum(step) % 4
    return np.repeat(np.frombuffer(b"ACGT", dtype=np.uint8)[idx], run)[:n].tobytes()


def batches():
    rng = np.random.default_rng(1010)
    out = []
    for run in (10, 4, 3, 2, 1):
        out.append(("runs-of-%d" % run, [runs(rng, 3 * T, run)]))
    out.append(("uniform", [rand_read(rng, 3 * T)]))
    # read starts at bytes 5 (lane 0) and 63 * 144 + 10 (lane 63) of the second tile
    out.append(("start-first-lane", [rand_read(rng, T + 5), rand_read(rng, 2 * T - 5)]))
    out.append(("start-last-lane", [rand_read(rng, T + 63 * LANE + 10), rand_read(rng, 2 * T - 63 * LANE - 10)]))
    out.append(("start-last-lane-runs", [runs(rng, T + 63 * LANE + 10, 2), runs(rng, 2 * T - 63 * LANE - 10, 2)]))
    for tail in (1, 31, 32, 145):
        out.append(("tail-%d" % tail, [rand_read(rng, 2 * T + tail)]))
        out.append(("tail-%d-runs" % tail, [runs(rng, 2 * T + tail, 3)]))
    return out


BATCHES = batches()


@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("mode", [HM.Hpc, HM.Regular], ids=["hpc", "regular"])
@pytest.mark.parametrize("l", STATIC_LS)
def test_every_static_l_and_piece_count(eng, oracle, l, mode):
    for tag, reads in BATCHES:
        compare(eng, oracle, reads, l, 4, 0.02, mode, expect_path=0, tag=tag)
