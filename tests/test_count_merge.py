"""Merging sorted count tables and accumulating counts across batches and files: s2k_count_merge_device, s2k_counter_*,
s2k_run_file_count (include/s2k.h).  The contracts: the merge equals `merge_reference` (numpy) byte for byte; a counter fed any
split of a key set equals s2k_count_device_ex on the whole set, sorted, byte for byte."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

pkg = import_package()

U64MAX = 2 ** 64 - 1
SAT = 2 ** 32 - 1
TILE = 3840  # merged items per workgroup of the merge kernel (s2k_count_merge.hip: MG_TILE)


def merge_reference(a, ca, b, cb, min_count):
    """-> (n_distinct, keys, counts): the union of two tables, ascending, counts of shared keys added and saturated at 2^32-1, pairs
    under max(min_count, 1) dropped"""
    u, s = _union_sums(a, ca, b, cb)
    return _cut(u, s, min_count)


def _union_sums(a, ca, b, cb):
    keys = np.concatenate([np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)])
    cnt = np.concatenate([np.asarray(ca, dtype=np.uint64), np.asarray(cb, dtype=np.uint64)])
    u, inv = np.unique(keys, return_inverse=True)
    s = np.bincount(inv.reshape(-1), weights=cnt.astype(np.float64), minlength=len(u)).astype(np.uint64)  # exact: sums < 2^53
    return u, np.minimum(s, np.uint64(SAT))


def _cut(u, s, min_count):
    m = s >= np.uint64(max(int(min_count), 1))
    return len(u), u[m], s[m].astype(np.uint32)


def skewed_keys(n=60000, seed=5):
    """a heavy hitter (a seventh of the input), ~9 % tiny keys, 2^64-1 and 0 (the mix of the sorted-count tests)"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    k[::7] = k[3]
    k[1::11] = rng.integers(0, 50, size=len(k[1::11]), dtype=np.uint64)
    k[5] = U64MAX
    k[9] = 0
    k[13] = U64MAX
    return k


def random_tables(rng, n_a, n_b, overlap, ends=True):
    """two strictly ascending tables with about overlap * min(n_a, n_b) shared keys; 0 and 2^64-1 in both when `ends`; counts 1..5"""
    shared = int(overlap * min(n_a, n_b))
    total = n_a + n_b - shared
    u = np.unique(rng.integers(1, 2 ** 64 - 1, size=total + total // 8 + 16, dtype=np.uint64))[:total]
    while len(u) < total:
        u = np.unique(np.concatenate([u, rng.integers(1, 2 ** 64 - 1, size=total, dtype=np.uint64)]))[:total]
    perm = rng.permutation(total)
    sh, ra, rb = perm[:shared], perm[shared:n_a], perm[n_a:]
    a = np.sort(u[np.concatenate([sh, ra])])
    b = np.sort(u[np.concatenate([sh, rb])])
    if ends:
        if n_a >= 2:
            a[0], a[-1] = 0, U64MAX
            a = np.sort(a)
        if n_b >= 2:
            b[0], b[-1] = 0, U64MAX
            b = np.sort(b)
    assert len(a) == n_a and len(b) == n_b
    return a, rng.integers(1, 6, size=n_a).astype(np.uint32), b, rng.integers(1, 6, size=n_b).astype(np.uint32)


# ---- CPU tier ------------------------------------------------------------------------------------------------------------
def test_entry_points_exported():
    lib = ctypes.CDLL(pkg.LIB_PATH)
    for s in ("s2k_count_merge_device", "s2k_counter_create", "s2k_counter_destroy", "s2k_counter_add", "s2k_counter_finish",
              "s2k_run_file_count"):
        assert hasattr(lib, s) and s in pkg.ABI_SYMBOLS, s
    assert hasattr(pkg.Engine, "count_merge_device") and hasattr(pkg.Engine, "run_file_count")
    for m in ("add", "add_tensor", "finish", "sizes", "close"):
        assert hasattr(pkg.KminmerCounter, m)


def test_header_compiles_in_c(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.fail("no C compiler")
    src = os.path.join(ROOT, "tests", "cpp", "count_merge.c")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "c.o")])


def _build_facade(tmpdir):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    exe = os.path.join(tmpdir, "counter_facade")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "counter_facade.cpp"), "-o", exe, "-L", csrc, "-ls2k", "-Wl,-rpath," + csrc,
                           "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_counter_compiles_and_links(tmp_path):
    assert os.path.exists(_build_facade(str(tmp_path)))


def test_merge_reference_edge_cases():
    e = np.zeros(0, dtype=np.uint64)
    ec = np.zeros(0, dtype=np.uint32)
    nd, k, c = merge_reference(e, ec, e, ec, 1)
    assert nd == 0 and len(k) == 0 and len(c) == 0
    nd, k, c = merge_reference([0, U64MAX], [1, 2], e, ec, 0)
    assert nd == 2 and k.tolist() == [0, U64MAX] and c.tolist() == [1, 2]
    nd, k, c = merge_reference(e, ec, [0, 7, U64MAX], [3, 1, 1], 2)
    assert nd == 3 and k.tolist() == [0] and c.tolist() == [3]
    # full overlap: every count doubles
    nd, k, c = merge_reference([0, 5, U64MAX], [1, 2, 3], [0, 5, U64MAX], [1, 2, 3], 3)
    assert nd == 3 and k.tolist() == [5, U64MAX] and c.tolist() == [4, 6]
    # partial overlap, cutoff between
    nd, k, c = merge_reference([1, 3, 5], [1, 1, 1], [2, 3, 6], [1, 1, 1], 2)
    assert nd == 5 and k.tolist() == [3] and c.tolist() == [2]
    # saturation
    nd, k, c = merge_reference([9], [SAT - 9], [9], [100], 1)
    assert k.tolist() == [9] and c.tolist() == [SAT]
    nd, k, c = merge_reference([9], [SAT], [9], [SAT], SAT)
    assert c.tolist() == [SAT]
    nd, k, c = merge_reference([9], [SAT - 1], [], [], SAT)
    assert nd == 1 and len(k) == 0
    # random tables agree with a dictionary
    rng = np.random.default_rng(1)
    a, ca, b, cb = random_tables(rng, 500, 300, 0.5)
    want = {}
    for x, y in zip(np.concatenate([a, b]).tolist(), np.concatenate([ca, cb]).tolist()):
        want[x] = want.get(x, 0) + y
    for mc in (0, 1, 2, 3):
        nd, k, c = merge_reference(a, ca, b, cb, mc)
        sol = {x: y for x, y in want.items() if y >= max(mc, 1)}
        assert nd == len(want) and k.tolist() == sorted(sol) and dict(zip(k.tolist(), c.tolist())) == sol
    assert (np.diff(a.astype(object)) > 0).all() and a[0] == 0 and a[-1] == U64MAX


def test_random_tables_shape():
    rng = np.random.default_rng(2)
    for na, nb, ov in ((1, 1, 1.0), (0, 5, 0.0), (TILE + 1, TILE - 1, 0.5), (100, 100, 1.0)):
        a, ca, b, cb = random_tables(rng, na, nb, ov)
        assert len(a) == na and len(b) == nb
        for t in (a, b):
            assert len(t) < 2 or (np.diff(t.astype(object)) > 0).all()
        if ov == 1.0 and na == nb and na > 2:
            assert (a == b).all()


# ---- GPU tier ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def _dev(x, dt):
    import torch

    x = np.ascontiguousarray(x)
    if len(x) == 0:
        return torch.zeros(1, dtype=dt, device="cuda:0")
    return torch.from_numpy(x.view(np.int64 if dt == torch.int64 else np.int32).copy()).to("cuda:0")


def _merge(eng, a, ca, b, cb, mc, outputs=True, capacity=None):
    import torch

    da, dca, db, dcb = _dev(a, torch.int64), _dev(ca, torch.int32), _dev(b, torch.int64), _dev(cb, torch.int32)
    cap = len(a) + len(b) if capacity is None else capacity
    ok = torch.empty(max(cap, 1), dtype=torch.int64, device="cuda:0")
    oc = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    nd, nk = eng.count_merge_device(da.data_ptr(), dca.data_ptr(), len(a), db.data_ptr(), dcb.data_ptr(), len(b), mc,
                                    ok.data_ptr() if outputs else 0, oc.data_ptr() if outputs else 0, cap if outputs else 0)
    return nd, nk, ok[:nk].cpu().numpy().view(np.uint64), oc[:nk].cpu().numpy().view(np.uint32)


def _check_merge(eng, a, ca, b, cb, mcs=(0, 1, 2, 3)):
    u, s = _union_sums(a, ca, b, cb)
    for mc in mcs:
        rnd, rk, rc = _cut(u, s, mc)
        for x, cx, y, cy in ((a, ca, b, cb), (b, cb, a, ca)):  # either table as A
            nd, nk, k, c = _merge(eng, x, cx, y, cy, mc)
            assert (nd, nk) == (rnd, len(rk)), (len(a), len(b), mc, nd, nk, rnd, len(rk))
            assert k.tobytes() == rk.tobytes() and c.tobytes() == rc.tobytes(), (len(a), len(b), mc)


@pytest.mark.gpu
def test_merge_sizes_and_overlaps(eng):
    rng = np.random.default_rng(3)
    sizes = [(0, 0), (0, 1), (1, 0), (1, 1), (TILE - 1, 1), (TILE, 0), (TILE + 1, TILE - 1), (TILE - 1, TILE + 1), (3 * TILE + 1, 2 * TILE - 1),
             (100003, 70001)]
    for na, nb in sizes:
        for ov in (0.0, 0.5, 1.0):
            _check_merge(eng, *random_tables(rng, na, nb, ov))


@pytest.mark.gpu
def test_merge_ten_million(eng):
    rng = np.random.default_rng(4)
    for ov in (0.0, 0.5, 1.0):
        _check_merge(eng, *random_tables(rng, 10 ** 7, 10 ** 7 - 12345 if ov < 1 else 10 ** 7, ov), mcs=(0, 2))
    _check_merge(eng, *random_tables(rng, 10 ** 7, 1000, 1.0), mcs=(1, 3))


@pytest.mark.gpu
def test_merge_pairs_straddle_every_tile_boundary(eng):
    """A = [x0] + U, B = U: the merge is x0, then A[i+1], B[i] for each shared key, so the pair (A, B) of a shared key sits at merged
    positions (2i+1, 2i+2) and every tile boundary (a multiple of TILE) falls between the two copies of a key"""
    rng = np.random.default_rng(5)
    for n in (TILE * 3, TILE * 40 + 7):
        u = np.unique(rng.integers(1, 2 ** 64 - 1, size=n + 64, dtype=np.uint64))[:n]
        u[-1] = U64MAX
        u = np.sort(u)
        a = np.concatenate([np.zeros(1, dtype=np.uint64), u])
        ca = rng.integers(1, 3, size=len(a)).astype(np.uint32)
        cu = rng.integers(1, 3, size=len(u)).astype(np.uint32)
        _check_merge(eng, a, ca, u, cu)
        # and the other way round: the extra key (0) first in B
        _check_merge(eng, u, cu, a, ca)
        # shared keys only at tile edges: B holds exactly the keys of A that land at a boundary
        edge = a[TILE - 1::TILE]
        _check_merge(eng, a, ca, edge, np.full(len(edge), 7, dtype=np.uint32))


@pytest.mark.gpu
def test_merge_saturation(eng):
    a = np.array([0, 5, U64MAX], dtype=np.uint64)
    ca = np.array([SAT - 10, SAT - 10, SAT], dtype=np.uint32)
    cb = np.array([100, 10, SAT], dtype=np.uint32)
    nd, nk, k, c = _merge(eng, a, ca, a, cb, 0)
    assert nd == 3 and k.tolist() == [0, 5, U64MAX] and c.tolist() == [SAT, SAT, SAT]
    nd, nk, k, c = _merge(eng, a, ca, a, cb, SAT)
    assert nk == 3
    rng = np.random.default_rng(6)
    x, _, y, _ = random_tables(rng, 50000, 50000, 0.5)
    _check_merge(eng, x, rng.integers(SAT - 200, SAT, size=50000, dtype=np.uint64).astype(np.uint32), y,
                 rng.integers(1, 400, size=50000).astype(np.uint32), mcs=(1, SAT))


def _raw_merge(eng, da, dca, na, db, dcb, nb, ok, oc, cap, mc=1):
    nd, nk = ctypes.c_uint64(7), ctypes.c_uint64(7)
    st = eng.lib.s2k_count_merge_device(eng.ctx, ctypes.c_void_p(da), ctypes.c_void_p(dca), na, ctypes.c_void_p(db), ctypes.c_void_p(dcb), nb,
                                        mc, ctypes.c_void_p(ok), ctypes.c_void_p(oc), cap, ctypes.byref(nd), ctypes.byref(nk))
    return st, int(nd.value), int(nk.value)


@pytest.mark.gpu
def test_merge_refusals_capacity_and_sizes_only(eng):
    import torch

    rng = np.random.default_rng(7)
    a, ca, b, cb = random_tables(rng, 3 * TILE + 5, 2 * TILE, 0.5)
    rnd, rk, rc = merge_reference(a, ca, b, cb, 2)
    # sizes only
    nd, nk, _, _ = _merge(eng, a, ca, b, cb, 2, outputs=False)
    assert (nd, nk) == (rnd, len(rk))
    # capacity one short: refused with the sizes, nothing written; exactly enough works
    with pytest.raises(pkg.S2kError) as e:
        _merge(eng, a, ca, b, cb, 2, capacity=len(rk) - 1)
    assert e.value.status == 7 and e.value.n_kept == len(rk) and e.value.n_distinct == rnd
    nd, nk, k, c = _merge(eng, a, ca, b, cb, 2, capacity=len(rk))
    assert k.tobytes() == rk.tobytes() and c.tobytes() == rc.tobytes()
    # not strictly ascending (a swap inside a tile, a swap across a tile boundary, a duplicate, in A or in B): refused, canary intact
    n = len(a) + len(b)
    canary_k = torch.full((n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    canary_c = torch.full((n,), 0x3C3C3C3C, dtype=torch.int32, device="cuda:0")
    for which, pos, kind in (("a", 100, "swap"), ("a", TILE, "swap"), ("b", TILE - 1, "swap"), ("b", len(b) - 2, "swap"), ("a", 3000, "dup"),
                             ("b", 0, "dup"), ("a", len(a) - 2, "dup")):
        x, y = a.copy(), b.copy()
        t = x if which == "a" else y
        if kind == "swap":
            t[pos], t[pos + 1] = t[pos + 1], t[pos]
        else:
            t[pos + 1] = t[pos]
        dx, dcx, dy, dcy = _dev(x, torch.int64), _dev(ca, torch.int32), _dev(y, torch.int64), _dev(cb, torch.int32)
        torch.cuda.synchronize()
        for ok, oc in ((canary_k.data_ptr(), canary_c.data_ptr()), (0, 0)):
            st, _, _ = _raw_merge(eng, dx.data_ptr(), dcx.data_ptr(), len(x), dy.data_ptr(), dcy.data_ptr(), len(y), ok, oc, n if ok else 0)
            assert st == 1, (which, pos, kind)
        torch.cuda.synchronize()
        assert bool((canary_k == 0x5A5A5A5A5A5A5A5A).all()) and bool((canary_c == 0x3C3C3C3C).all())
    # an output that overlaps an input (keys into A's keys, keys into B's counts, counts into A's counts)
    da, dca, db, dcb = _dev(a, torch.int64), _dev(ca, torch.int32), _dev(b, torch.int64), _dev(cb, torch.int32)
    torch.cuda.synchronize()
    for ok, oc in ((da.data_ptr() + 8, canary_c.data_ptr()), (canary_k.data_ptr(), dcb.data_ptr() + 40), (canary_k.data_ptr(), dca.data_ptr())):
        st, _, _ = _raw_merge(eng, da.data_ptr(), dca.data_ptr(), len(a), db.data_ptr(), dcb.data_ptr(), len(b), ok, oc, n)
        assert st == 1
    torch.cuda.synchronize()
    assert bool((canary_k == 0x5A5A5A5A5A5A5A5A).all())
    # NULL inputs with n > 0, NULL size pointers
    assert _raw_merge(eng, 0, dca.data_ptr(), 5, 0, 0, 0, 0, 0, 0)[0] == 1
    assert eng.lib.s2k_count_merge_device(eng.ctx, None, None, 0, None, None, 0, 1, None, None, 0, None, None) == 1
    # n_b == 0: the cutoff filter of one table
    nd, nk, k, c = _merge(eng, a, ca, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), 3)
    r = merge_reference(a, ca, [], [], 3)
    assert (nd, nk) == (r[0], len(r[1])) and k.tobytes() == r[1].tobytes() and c.tobytes() == r[2].tobytes()


def _one_shot(eng, keys_dev, mc):
    import torch

    n = keys_dev.numel()
    k = torch.empty(max(n, 1), dtype=torch.int64, device=keys_dev.device)
    c = torch.empty(max(n, 1), dtype=torch.int32, device=keys_dev.device)
    torch.cuda.synchronize()
    nd, nk = eng.count_device_ex(keys_dev.data_ptr(), n, mc, True, k.data_ptr(), c.data_ptr(), n)
    return nd, nk, k[:nk], c[:nk]


def _counter_vs_one_shot(eng, keys_dev, n_batches, mcs):
    import torch

    ctr = pkg.KminmerCounter(eng)
    try:
        for part in torch.tensor_split(keys_dev, n_batches):
            ctr.add_tensor(part)
        for mc in mcs:
            nd, nk, k, c = _one_shot(eng, keys_dev, mc)
            assert ctr.sizes(mc) == (nd, nk), (n_batches, mc)
            gk, gc = ctr.finish(mc)
            assert torch.equal(gk, k) and torch.equal(gc, c), (n_batches, mc)
    finally:
        ctr.close()


@pytest.mark.gpu
def test_counter_split_independence(eng):
    import torch

    rng = np.random.default_rng(8)
    sk = torch.from_numpy(skewed_keys().view(np.int64)).to("cuda:0")
    u = rng.integers(0, 2 ** 64, size=20 * 10 ** 6, dtype=np.uint64)
    u[1::5] = u[: len(u[1::5])]  # a fifth of the keys twice
    rng.shuffle(u)
    uk = torch.from_numpy(u.view(np.int64)).to("cuda:0")
    for keys in (sk, uk):
        for nb in (1, 3, 17, 64):
            _counter_vs_one_shot(eng, keys, nb, (0, 2) if keys is uk else (1, 2, 3, 2 ** 32 - 1))
    # the skewed mix against numpy too, byte for byte
    nd, k, c = merge_reference(skewed_keys(), np.ones(60000, dtype=np.uint32), [], [], 2)
    ctr = pkg.KminmerCounter(eng)
    for part in np.array_split(skewed_keys(), 5):
        ctr.add_tensor(torch.from_numpy(part.view(np.int64)).to("cuda:0"))
    gk, gc = ctr.finish(2)
    assert ctr.last_sizes == (nd, len(k))
    assert gk.cpu().numpy().view(np.uint64).tobytes() == k.tobytes() and gc.cpu().numpy().view(np.uint32).tobytes() == c.tobytes()
    ctr.close()


@pytest.mark.gpu
def test_counter_repeatable_finish_and_add_after_finish(eng):
    import torch

    rng = np.random.default_rng(9)
    x = rng.integers(0, 2 ** 20, size=300000, dtype=np.uint64)
    y = np.concatenate([rng.integers(0, 2 ** 20, size=200000, dtype=np.uint64), [0, U64MAX, U64MAX]]).astype(np.uint64)
    ctr = pkg.KminmerCounter(eng)
    assert ctr.sizes(1) == (0, 0)
    k0, c0 = ctr.finish(1)
    assert k0.numel() == 0 and c0.numel() == 0
    ctr.add(0, 0)
    ctr.add_tensor(torch.from_numpy(x.view(np.int64)).to("cuda:0"))
    k1, c1 = ctr.finish(2)
    k2, c2 = ctr.finish(2)
    assert torch.equal(k1, k2) and torch.equal(c1, c2)
    ctr.add_tensor(torch.from_numpy(y.view(np.int64)).to("cuda:0"))
    allk = np.concatenate([x, y])
    for mc in (1, 3):
        nd, rk, rc = merge_reference(allk, np.ones(len(allk), dtype=np.uint32), [], [], mc)
        gk, gc = ctr.finish(mc)
        assert ctr.last_sizes == (nd, len(rk))
        assert gk.cpu().numpy().view(np.uint64).tobytes() == rk.tobytes() and gc.cpu().numpy().view(np.uint32).tobytes() == rc.tobytes()
    # capacity refusal of finish, as s2k_count_device_ex
    nd, nk = ctr.sizes(1)
    out = torch.empty(nk, dtype=torch.int64, device="cuda:0")
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert eng.lib.s2k_counter_finish(ctypes.c_void_p(ctr.handle), 1, ctypes.c_void_p(out.data_ptr()), None, nk - 1, ctypes.byref(a),
                                      ctypes.byref(b)) == 7
    assert (a.value, b.value) == (nd, nk)
    assert eng.lib.s2k_counter_add(ctypes.c_void_p(ctr.handle), None, 5) == 1
    ctr.close()


@pytest.mark.gpu
def test_counter_full_size_config1_hashes(eng):
    """configs[1]: 1 000 000 x 10 kbp synthetic reads, l=31 k=10 d=0.01, Hpc: its k-min-mer hashes extracted into HBM, added in 8 slices,
    equal one s2k_count_device_ex over the whole (compared on the device)"""
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
    assert n > 100 * 10 ** 6
    ctr = pkg.KminmerCounter(eng)
    for part in torch.tensor_split(keys, 8):
        ctr.add_tensor(part)
    for mc in (1, 2):
        nd, nk, k, cc = _one_shot(eng, keys, mc)
        gk, gc = ctr.finish(mc)
        assert ctr.last_sizes == (nd, nk)
        assert torch.equal(gk, k) and torch.equal(gc, cc), mc
    ctr.close()


# ---- file mode ------------------------------------------------------------------------------------------------------------
def _reads(rng, n, maxlen=3000):
    return [bytes(np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5 if i % 7 == 0 else 4, size=int(rng.integers(0, maxlen)))])
            for i in range(n)]


def _write_fasta(path, reads, width=61):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">read%d x\n" % i)
            for j in range(0, len(r), width):
                f.write(r[j:j + width] + b"\n")
            if not r:
                f.write(b"\n")


def _write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, (b"@I" * len(r))[:len(r)]))


def _repeated_reads(seed):
    rng = np.random.default_rng(seed)
    reads = _reads(rng, 900, maxlen=12000) + [bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=3_300_000)])]
    reads += _reads(rng, 50, 5000)
    # repeats: 300 reads again, 60 of them five more times, so that counts of 2, 6 and more occur
    reads += [reads[int(i)] for i in rng.integers(0, 900, size=300)]
    reads += [r for r in reads[-60:] for _ in range(5)]
    order = rng.permutation(len(reads))
    return [reads[int(i)] for i in order]


@pytest.mark.gpu
def test_run_file_count_fasta_fastq_matches_oracle(tmp_path, eng, oracle):
    from oracle import s2k_oracle as so

    reads = _repeated_reads(17)
    bases, off = pkg.pack_reads(reads)
    ref = oracle.batch(bases, off, 31, 7, 0.01, so.HPC, threads=8)
    u, cnt = np.unique(ref["hash"].astype(np.uint64), return_counts=True)
    assert (cnt > 5).any()
    fa, fq = tmp_path / "r.fa", tmp_path / "r.fq"
    _write_fasta(fa, reads)
    _write_fastq(fq, reads)
    for path in (fa, fq):
        plain = eng.run_file(str(path), 31, 7, 0.01, pkg.HashMode.Hpc, batch_bases=1 << 20)
        for mc in (1, 2, 5):
            r = eng.run_file_count(str(path), 31, 7, 0.01, pkg.HashMode.Hpc, min_count=mc, batch_bases=1 << 20)
            for f in ("n_reads", "n_bases", "n_minimizers", "n_kminmers", "xor_hash", "hash_bound", "path"):
                assert r[f] == plain[f], (path.name, mc, f)
            m = cnt >= mc
            assert (r["n_distinct"], r["n_kept"]) == (len(u), int(m.sum())), (path.name, mc)
            assert r["keys"].cpu().numpy().view(np.uint64).tobytes() == u[m].tobytes()
            assert r["counts"].cpu().numpy().view(np.uint32).tobytes() == cnt[m].astype(np.uint32).tobytes()


@pytest.mark.gpu
def test_run_file_count_two_files_one_counter(tmp_path, eng):
    rng = np.random.default_rng(23)
    r1 = _reads(rng, 400, maxlen=9000)
    r2 = _reads(rng, 300, maxlen=9000) + r1[:150]
    f1, f2, f12 = tmp_path / "a.fa", tmp_path / "b.fq", tmp_path / "ab.fa"
    _write_fasta(f1, r1)
    _write_fastq(f2, r2)
    _write_fasta(f12, r1 + r2)
    ctr = pkg.KminmerCounter(eng)
    t1 = eng.run_file_count(str(f1), 31, 7, 0.01, pkg.HashMode.Hpc, min_count=2, batch_bases=1 << 20, counter=ctr)
    t2 = eng.run_file_count(str(f2), 31, 7, 0.01, pkg.HashMode.Hpc, min_count=2, batch_bases=1 << 20, counter=ctr)
    both = eng.run_file_count(str(f12), 31, 7, 0.01, pkg.HashMode.Hpc, min_count=2, batch_bases=1 << 20)
    assert t1["n_kminmers"] + t2["n_kminmers"] == both["n_kminmers"] and (t1["xor_hash"] ^ t2["xor_hash"]) == both["xor_hash"]
    assert (t2["n_distinct"], t2["n_kept"]) == (both["n_distinct"], both["n_kept"]) and both["n_kept"] > 0
    import torch

    assert torch.equal(t2["keys"], both["keys"]) and torch.equal(t2["counts"], both["counts"])
    ctr.close()


@pytest.mark.gpu
def test_cli_and_cpp_counter_print_counts(tmp_path, oracle):
    from oracle import s2k_oracle as so

    reads = _repeated_reads(31)[:700]
    p = tmp_path / "r.fq"
    _write_fastq(p, reads)
    bases, off = pkg.pack_reads(reads)
    ref = oracle.batch(bases, off, 31, 5, 0.01, so.REGULAR, threads=8)
    u, cnt = np.unique(ref["hash"].astype(np.uint64), return_counts=True)
    exe = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc", "s2k_main")
    plain = subprocess.run([exe, str(p)], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    assert "kminmers: %d " % ref["n"] in plain.stdout and "distinct:" not in plain.stdout
    out = subprocess.run([exe, str(p), "31", "5", "0.01", "0", "1", "3"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "kminmers: %d " % ref["n"] in out.stdout
    assert "distinct: %d solid: %d\n" % (len(u), int((cnt >= 3).sum())) in out.stdout
    # the C++ facade (s2k::Counter, Engine::run_file_count, Engine::count_merge)
    ref7 = oracle.batch(bases, off, 31, 7, 0.01, so.HPC, threads=8)
    u7, c7 = np.unique(ref7["hash"].astype(np.uint64), return_counts=True)
    fx = subprocess.run([_build_facade(str(tmp_path)), str(p), "2"], capture_output=True, text=True)
    assert fx.returncode == 0, fx.stderr
    assert fx.stdout.strip() == "distinct %d solid %d kminmers %d empty 0" % (len(u7), int((c7 >= 2).sum()), ref7["n"])
