"""Counting with an abundance cutoff, in hash order: s2k_count_device_ex (include/s2k.h).  The contract is np.unique(...,
return_counts=True) followed by the cutoff (`solid_reference`); sorted mode must match it byte for byte, unsorted mode as a set."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

pkg = import_package()
spec = importlib.util.spec_from_file_location("s2k_sharding", os.path.join(ROOT, "rust-seq2kminmers_amd", "sharding.py"))
sharding = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sharding)

U64MAX = np.uint64(2 ** 64 - 1)


def solid_reference(keys, min_count):
    """-> (n_distinct, keys, counts) of the contract: distinct values ascending, those under max(min_count, 1) dropped"""
    u, c = np.unique(np.asarray(keys, dtype=np.uint64), return_counts=True)
    m = c >= max(int(min_count), 1)
    return len(u), u[m], c[m].astype(np.uint32)


def skewed_keys(n=60000, seed=5):
    """the mix of the gloo exchange test: a heavy hitter (a seventh of the input), ~9 % tiny keys, 2^64-1 and 0"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    k[::7] = k[3]
    k[1::11] = rng.integers(0, 50, size=len(k[1::11]), dtype=np.uint64)
    k[5] = U64MAX
    k[9] = 0
    k[13] = U64MAX
    return k


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_point_exported_and_flag_constant():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert hasattr(lib, "s2k_count_device_ex")
    assert "s2k_count_device_ex" in pkg.ABI_SYMBOLS
    assert pkg.COUNT_SORTED == 1
    assert hasattr(pkg.Engine, "count_device_ex")


def test_header_flag_compiles_in_c(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    src = os.path.join(ROOT, "tests", "cpp", "count_solid.c")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "c.o")])


def test_reference_edge_cases():
    assert solid_reference(np.zeros(0, dtype=np.uint64), 1)[0] == 0
    nd, k, c = solid_reference(np.array([7], dtype=np.uint64), 0)
    assert nd == 1 and k.tolist() == [7] and c.tolist() == [1]
    keys = np.array([U64MAX, 0, U64MAX, 5, 0, U64MAX], dtype=np.uint64)
    nd, k, c = solid_reference(keys, 1)
    assert nd == 3 and k.tolist() == [0, 5, 2 ** 64 - 1] and c.tolist() == [2, 1, 3]
    nd, k, c = solid_reference(keys, 2)
    assert nd == 3 and k.tolist() == [0, 2 ** 64 - 1] and c.tolist() == [2, 3]
    nd, k, c = solid_reference(keys, 3)
    assert k.tolist() == [2 ** 64 - 1]
    assert len(solid_reference(keys, 2 ** 32 - 1)[1]) == 0
    sk = skewed_keys()
    nd, k, c = solid_reference(sk, 2)
    assert (np.diff(k.astype(object)) > 0).all() if len(k) > 1 else True
    assert k[-1] == U64MAX and int(c.sum()) <= len(sk)


def test_sharding_min_count_with_numpy_ops():
    """the count_kminmers plumbing for min_count > 1 on one rank, with a numpy stand-in for the device op"""
    import torch

    class Ops:
        def count_ex(self, keys, min_count, want_pairs=False):
            nd, k, c = solid_reference(keys.numpy().view(np.uint64), min_count)
            return nd, len(k), torch.from_numpy(k.view(np.int64).copy()), torch.from_numpy(c.astype(np.int32))

    sk = skewed_keys()
    r = sharding.count_kminmers(torch.from_numpy(sk.view(np.int64)), Ops(), want_pairs=True, min_count=2)
    nd, k, c = solid_reference(sk, 2)
    assert r["n_distinct"] == nd and r["n_kept"] == len(k) and r["n_keys"] == len(sk)
    assert (r["keys"].numpy().view(np.uint64) == k).all()


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def _run(eng, keys_dev, n, min_count, sorted_=True, outputs=True, capacity=None):
    import torch

    dev = keys_dev.device
    cap = max(n, 1) if capacity is None else capacity
    k = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    c = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    nd, nk = eng.count_device_ex(keys_dev.data_ptr() if n else 0, n, min_count, sorted_, k.data_ptr() if outputs else 0,
                                 c.data_ptr() if outputs else 0, cap if outputs else 0)
    return nd, nk, k[:nk].cpu().numpy().view(np.uint64), c[:nk].cpu().numpy().view(np.uint32)


def _check(eng, keys, min_count, sorted_=True, keys_dev=None):
    import torch

    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if keys_dev is None:
        keys_dev = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
    nd, nk, k, c = _run(eng, keys_dev, len(keys), min_count, sorted_)
    rnd, rk, rc = solid_reference(keys, min_count)
    assert (nd, nk) == (rnd, len(rk)), (len(keys), min_count, nd, nk, rnd, len(rk))
    if sorted_:
        assert k.tobytes() == rk.tobytes() and c.tobytes() == rc.tobytes()
    else:
        order = np.argsort(k, kind="stable")
        assert (k[order] == rk).all() and (c[order] == rc).all()
    return k, c


@pytest.mark.gpu
def test_tiny_and_empty(eng):
    import torch

    nd, nk, _, _ = _run(eng, torch.zeros(1, dtype=torch.int64, device="cuda:0"), 0, 1)
    assert (nd, nk) == (0, 0)
    for mc in (0, 1, 2):
        _check(eng, np.array([12345], dtype=np.uint64), mc)
    _check(eng, np.array([2 ** 64 - 1], dtype=np.uint64), 1)
    _check(eng, np.array([0], dtype=np.uint64), 1)


@pytest.mark.gpu
def test_uniform_sizes_straddle_buckets(eng):
    rng = np.random.default_rng(11)
    for n in (1, 63, 64, 65, 10 ** 5, 10 ** 7):
        keys = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
        if n >= 64:
            keys[n // 2:] = keys[: n - n // 2][::-1]  # every key at least twice for half of them
            rng.shuffle(keys)
        for mc in ((1, 2) if n == 10 ** 7 else (0, 1, 2, 3)):
            _check(eng, keys, mc, sorted_=True)
        _check(eng, keys, 2, sorted_=False)


@pytest.mark.gpu
def test_skewed_mix_every_cutoff(eng):
    keys = skewed_keys()
    for mc in (0, 1, 2, 3, 1000, 2 ** 32 - 1):
        _check(eng, keys, mc, sorted_=True)
        _check(eng, keys, mc, sorted_=False)


@pytest.mark.gpu
def test_one_key_ten_million_times(eng):
    for v in (np.uint64(0x0123456789ABCDEF), U64MAX):
        keys = np.full(10 ** 7, v, dtype=np.uint64)
        k, c = _check(eng, keys, 2)
        assert k.tolist() == [int(v)] and c.tolist() == [10 ** 7]
        _check(eng, keys, 10 ** 7 + 1)


@pytest.mark.gpu
def test_one_bucket_overflows_lds(eng):
    """2e6 distinct keys sharing their top 16 bits (one level-2 bucket far beyond the LDS table), plus repeats and other buckets"""
    rng = np.random.default_rng(3)
    low = rng.choice(2 ** 40, size=2 * 10 ** 6, replace=False).astype(np.uint64) << np.uint64(8)
    low |= rng.integers(0, 256, size=len(low), dtype=np.uint64)
    low = np.unique(low)
    top = np.uint64(0xBEEF) << np.uint64(48)
    keys = np.concatenate([top | low, (top | low[:300000]), rng.integers(0, 2 ** 64, size=100000, dtype=np.uint64)])
    rng.shuffle(keys)
    for mc in (1, 2):
        _check(eng, keys, mc, sorted_=True)
    _check(eng, keys, 2, sorted_=False)
    # 3.7e7 keys: a 9-bit second digit, so the re-partition levels step through odd shifts (47, 39, ..., 7, then 7 bits at 0)
    keys = np.concatenate([keys, rng.integers(0, 2 ** 64, size=35 * 10 ** 6, dtype=np.uint64)])
    _check(eng, keys, 2, sorted_=True)


@pytest.mark.gpu
def test_capacity_and_sizes_only(eng):
    import torch

    keys = skewed_keys()
    d = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
    rnd, rk, _ = solid_reference(keys, 2)
    nd, nk, _, _ = _run(eng, d, len(keys), 2, outputs=False)
    assert (nd, nk) == (rnd, len(rk))
    with pytest.raises(pkg.S2kError) as e:
        _run(eng, d, len(keys), 2, capacity=len(rk) - 1)
    assert e.value.status == 7 and e.value.n_kept == len(rk) and e.value.n_distinct == rnd
    nd, nk, k, _ = _run(eng, d, len(keys), 2, capacity=len(rk))  # exactly enough
    assert nk == len(rk) and k.tobytes() == rk.tobytes()
    lib = eng.lib
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.s2k_count_device_ex(eng.ctx, ctypes.c_void_p(d.data_ptr()), len(keys), 1, 2, None, None, 0, ctypes.byref(a), ctypes.byref(b)) == 1
    assert lib.s2k_count_device_ex(eng.ctx, ctypes.c_void_p(d.data_ptr()), 2 ** 32, 1, 1, None, None, 0, ctypes.byref(a), ctypes.byref(b)) == 1


@pytest.mark.gpu
def test_sorted_output_identical_across_calls(eng):
    import torch

    rng = np.random.default_rng(21)
    keys = np.concatenate([skewed_keys(200000, 8), rng.integers(0, 2 ** 64, size=300000, dtype=np.uint64)])
    d = torch.from_numpy(keys.view(np.int64)).to("cuda:0")
    r1 = _run(eng, d, len(keys), 1)
    r2 = _run(eng, d, len(keys), 1)
    assert r1[:2] == r2[:2] and r1[2].tobytes() == r2[2].tobytes() and r1[3].tobytes() == r2[3].tobytes()


@pytest.mark.gpu
def test_extract_then_count_matches_oracle_dictionary(eng, oracle, ecoli):
    import torch

    rng = np.random.default_rng(9)  # the read set of test_count.py::test_count_device_matches_dictionary
    reads = [bytes(ecoli[a: a + 3000]) for a in rng.integers(0, len(ecoli) - 3000, size=400)]
    got = eng.extract_reads(reads, 21, 3, 0.05, pkg.HashMode.Hpc)
    ref = oracle.batch(*pkg.pack_reads(reads), 21, 3, 0.05, 1)
    want = {}
    for h in ref["hash"].tolist():
        want[h] = want.get(h, 0) + 1
    d = torch.from_numpy(got["hash"].view(np.int64)).to("cuda:0")
    for mc in (1, 2, 5):
        nd, nk, k, c = _run(eng, d, len(got["hash"]), mc)
        solid = {h: n for h, n in want.items() if n >= mc}
        assert nd == len(want) and nk == len(solid)
        assert k.tolist() == sorted(solid) and dict(zip(k.tolist(), c.tolist())) == solid


@pytest.mark.gpu
def test_full_size_config1_hashes(eng):
    """configs[1]: 1 000 000 x 10 kbp synthetic reads (10 Gbp), l=31 k=10 d=0.01, Hpc -- the k-min-mer hashes are extracted into HBM
    and counted; np.unique over the same hashes on the host is the reference, s2k_count_device gives n_distinct as well"""
    import torch

    n_reads, L, seed = 1_000_000, 10_000, 1
    dev = torch.device("cuda", 0)
    d_b = torch.empty(n_reads * L + 64, dtype=torch.uint8, device=dev)
    d_o = torch.arange(n_reads + 1, dtype=torch.int64, device=dev) * L
    cap = int(n_reads * L * 0.0215)
    t = {"km_off": torch.empty(n_reads + 1, dtype=torch.int64, device=dev), "hash": torch.empty(cap, dtype=torch.int64, device=dev),
         "start": torch.empty(cap, dtype=torch.int32, device=dev), "end": torch.empty(cap, dtype=torch.int32, device=dev),
         "rev": torch.empty(cap, dtype=torch.uint8, device=dev)}
    o = pkg.DeviceOut()
    o.km_capacity = cap
    o.km_off, o.hash, o.start, o.end, o.rev = (t[x].data_ptr() for x in ("km_off", "hash", "start", "end", "rev"))
    torch.cuda.synchronize()
    eng.synth_bases_device(seed, 0, n_reads * L, d_b.data_ptr())
    c = eng.extract_device(d_b.data_ptr(), d_o.data_ptr(), n_reads, n_reads * L, 31, 10, 0.01, int(pkg.HashMode.Hpc), o)
    n = c["n_kminmers"]
    del d_b, t["start"], t["end"], t["rev"]
    keys = t["hash"][:n]
    host = keys.cpu().numpy().view(np.uint64)
    u, cnt = np.unique(host, return_counts=True)
    torch.cuda.synchronize()
    assert eng.count_device(keys.data_ptr(), n) == len(u)
    for mc in (1, 2):
        nd, nk, k, cc = _run(eng, keys, n, mc)
        m = cnt >= mc
        assert nd == len(u) and nk == int(m.sum())
        assert k.tobytes() == u[m].tobytes() and cc.tobytes() == cnt[m].astype(np.uint32).tobytes()


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    allk = skewed_keys()
    mine = allk[rank::world].copy()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    ops = sharding.EngineCountOps(eng, dev)
    keys = torch.from_numpy(mine.view(np.int64)).to(dev)
    r = sharding.count_kminmers(keys, ops, dist, collectives_on_device=False, want_pairs=True, min_count=2)
    k = r["keys"].cpu().numpy().view(np.uint64)
    c = r["counts"].cpu().numpy()
    assert all(((int(x) * world) >> 64) == rank for x in k), "a rank must own exactly its range of the hash space"
    assert (np.diff(k.astype(object)) > 0).all() if len(k) > 1 else True
    q.put((rank, r["n_keys"], r["n_distinct"], r["n_kept"], k.tobytes(), c.astype(np.uint32).tobytes()))
    eng.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_min_count_matches_unsharded():
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=300) for _ in ps])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    allk = skewed_keys()
    rnd, rk, rc = solid_reference(allk, 2)
    keys = b"".join(r[4] for r in res)  # rank 0 owns the lower half of the hash space: concatenation is ascending
    counts = b"".join(r[5] for r in res)
    for _, n_keys, nd, nk, _, _ in res:
        assert (n_keys, nd, nk) == (len(allk), rnd, len(rk))
    assert keys == rk.tobytes() and counts == rc.tobytes()
