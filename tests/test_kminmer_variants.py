"""Every k-min-mer kernel the library ships, field by field against the oracle.

launch_desc_kminmers (s2k_desc.hip) picks one of eight instantiations of desc_kminmer_kernel<KT, FULL, COAL>, and the legacy path
(s2k_kminmer.hip) one of two kernels.  VARIANTS names each of them with the calls that reach it; the CPU-tier test at the bottom
keeps the table equal to the kernels in the code object, so a new instantiation without a row fails without a GPU.

Every GPU call goes through the device API with arrays `capacity + GUARD` long and filled with a sentinel: besides every field
(km_off, hash, start, end, rev, the minimizer triples, the counts and the path) each call checks that nothing was written past
the capacity it was given."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
T = 9216  # bases per tile (s2k_dev.h TILE_BASES)
GUARD = T  # guard band in elements: more than the windows or minimizers of any one tile, so that even a wrong write stays inside the allocation
SENT = 0xA5
KM = ("hash", "start", "end", "rev")
MN = ("mn_j", "mn_jend", "mn_hash")
ISZ = {"km_off": 8, "hash": 8, "start": 4, "end": 4, "rev": 1, "mn_off": 8, "mn_j": 4, "mn_jend": 4, "mn_hash": 4}
DT = {8: np.uint64, 4: np.uint32, 1: np.uint8}
S2K_ERR_CAPACITY = 7
FLAG_MN, FLAG_SERIAL, FLAG_LEGACY = 1, 2, 8


def R(eng, k, path=0, hpc_only=False, **opt):
    """one way to reach a kernel: engine ("plain": an unchained context, one chunk per call; "chained": a context chained behind
    another with s2k_chain_after -- an Hpc call's last chunk then does not run alone), k, expected counts.path, options
    (triples: ask for the minimizer triples; arrays: the k-min-mer arrays given, the rest NULL; legacy / serial: flags)"""
    return {"eng": eng, "k": k, "path": path, "hpc_only": hpc_only, **opt}


# kernel -> (how a call reaches it, the routes the matrix runs).  Besides these routes the non-COAL lane-serial kernels
# (<5|10, true, false>) also run as the non-last chunks of a context made with S2K_DESC_CHUNKS=3 (test_forced_chunks_...) and for
# every chunk in a child process with S2K_KM_NO_COAL=1 (test_lane_serial_kernels_without_staged_stores).
VARIANTS = {
    "desc_kminmer_kernel<10,true,true>": ("k = 10, all four arrays, no triples, a call whose k-min-mer kernel runs alone", [R("plain", 10)]),
    "desc_kminmer_kernel<5,true,true>": ("k = 5, all four arrays, no triples, a call whose k-min-mer kernel runs alone", [R("plain", 5)]),
    "desc_kminmer_kernel<10,true,false>": ("k = 10, all four arrays, no triples: chained Hpc call, non-last chunks, S2K_KM_NO_COAL=1",
                                           [R("chained", 10, hpc_only=True)]),
    "desc_kminmer_kernel<5,true,false>": ("k = 5, all four arrays, no triples: chained Hpc call, non-last chunks, S2K_KM_NO_COAL=1",
                                          [R("chained", 5, hpc_only=True)]),
    "desc_kminmer_kernel<0,true,false>": ("any other k <= 32, all four arrays, no triples", [R("plain", 7), R("plain", 32)]),
    "desc_kminmer_kernel<10,false,false>": ("k = 10 with the minimizer triples, or with a k-min-mer array left NULL",
                                            [R("plain", 10, triples=True), R("plain", 10, arrays=("hash", "start", "end"))]),
    "desc_kminmer_kernel<5,false,false>": ("k = 5 with the minimizer triples, or with a k-min-mer array left NULL",
                                           [R("plain", 5, triples=True), R("chained", 5, arrays=("hash", "end", "rev"))]),
    "desc_kminmer_kernel<0,false,false>": ("any other k <= 32 with the triples or a NULL array", [R("plain", 3, triples=True), R("plain", 7, arrays=("start",))]),
    "kminmer_kernel_fast": ("k 33 .. 65, S2K_FLAG_LEGACY_PATH, a tile with > 30 read starts, S2K_FLAG_FORCE_SERIAL (k <= 65)",
                            [R("plain", 40, path=2), R("plain", 10, path=2, legacy=True), R("plain", 5, path=1, serial=True, triples=True)]),
    "kminmer_kernel": ("k > 65 (legacy or serial path)", [R("plain", 70, path=2)]),
}


def _rand(rng, n, **kw):
    from gpu_util import rand_read

    return rand_read(rng, n, **kw)


def inputs():
    """(name, reads, l, densities, modes, more than 30 read starts in some tile, read-serial kernels affordable)"""
    from gpu_util import pkg

    HM = pkg.HashMode
    ALL, SCALAR = (HM.Regular, HM.Hpc, HM.Simd, HM.HpcSimd), (HM.Regular, HM.Hpc)
    rng = np.random.default_rng(2718)
    out = []
    # (a) the ragged lengths of test_ragged_batches_all_tile_alignments
    lens = [0, 1, 30, 31, 32, 33, 143, 144, 145, 0, 0, 5000, T - 5200 - 589, 1, T, T + 1, T - 1, 31, 2 * T + 7, 3, 17, T - 31,
            T - 30, 31, 62, 0, 20000, 288, 289, 9000, 100, 40000, 15, 16, 144 * 3]
    for hp, odd in ((0.0, 0.0), (0.3, 0.02)):
        out.append(("ragged hp=%g" % hp, [_rand(rng, n, hp=hp, odd=odd) for n in lens], 31, (0.01,), ALL, False, True))
    # (b) tiles holding 0, 1, 2, 3, 4, 8, 16, 30 read starts (reads of ceil(T / n) bases), and 31 / 40 (the legacy path)
    for n in (0, 1, 2, 3, 4, 8, 16, 30, 31, 40):
        if n == 0:
            reads = [_rand(rng, 8 * T + 100)]
        else:
            ln = -(-T // n) if n <= 30 else T // n
            reads = [_rand(rng, ln) for _ in range(8 * n)]
        out.append(("%d starts per tile" % n, reads, 31, (0.01, 0.04), SCALAR, n > 30, True))
    # (c) reads shorter than l, of l and l + 1 bases, and with fewer than k minimizers, next to long ones
    for l in (31, 21):
        lens = [l - 1, l, l + 1, 30000, l, l + 1, 120, 400, 900, 25000, l + 2, 250, 600, T, 1500, l - 1, 700, 3 * T + 5, l]
        out.append(("short reads l=%d" % l, [_rand(rng, n) for n in lens], l, (0.01,), SCALAR, False, True))
    # (d) dense: more than 192 minimizers per tile, several batches of the lane-serial kernel, remainders that take RB = 1 and 2
    reads = [_rand(rng, int(n)) for n in rng.integers(2000, 20000, size=30)]
    out.append(("dense", reads, 31, (0.005, 0.05, 0.1, 0.3), ALL, False, True))
    # (e) sparse: the k-1 minimizers before a tile lie many tiles back (at 1e-5: more than 63 tiles back)
    reads = [_rand(rng, int(n)) for n in rng.integers(100000, 300000, size=4)]
    out.append(("sparse", reads, 31, (0.0005, 0.001, 0.002), SCALAR, False, False))
    out.append(("very sparse", [_rand(rng, 1600000), _rand(rng, 300000)], 31, (0.00001,), SCALAR, False, False))
    # (f) low complexity and long homopolymers: records spill out of their tile's slab
    reads = [_rand(rng, int(n), hp=0.97, alphabet=b"AC") for n in rng.integers(5000, 60000, size=8)]
    reads += [b"A" * 70000, _rand(rng, 3000) + b"G" * 40000 + _rand(rng, 3000), _rand(rng, 30000, alphabet=b"A")]
    out.append(("low complexity", reads, 31, (0.05, 0.5), SCALAR, False, True))
    return out


class Dev:
    """device-API calls with guard bands (one per test or child)"""

    def __init__(self, oracle):
        import torch

        from gpu_util import OMODE, pkg

        self.torch, self.pkg, self.OMODE, self.oracle = torch, pkg, OMODE, oracle
        self.dev = torch.device("cuda", 0)
        self.engines = {}

    def engine(self, name):
        if name not in self.engines:
            pkg = self.pkg
            if name == "chained":
                other = self.engine("chained-prev")
                e = pkg.Engine(0)
                e.chain_after(other)
            elif name == "chunks3":  # S2K_DESC_CHUNKS is read when a context is created
                os.environ["S2K_DESC_CHUNKS"] = "3"
                try:
                    e = pkg.Engine(0)
                finally:
                    del os.environ["S2K_DESC_CHUNKS"]
            else:
                e = pkg.Engine(0)
            self.engines[name] = e
        return self.engines[name]

    def close(self):
        for name in ("chained", "chunks3", "plain", "chained-prev"):  # (a chained context before the one it follows)
            if name in self.engines:
                self.engines.pop(name).close()
        for e in self.engines.values():
            e.close()
        self.engines = {}

    def batch(self, reads):
        torch, pkg = self.torch, self.pkg
        bases, off = pkg.pack_reads(reads)
        return {"bases": bases, "off": off, "d_b": torch.from_numpy(bases).to(self.dev), "d_o": torch.from_numpy(off.astype(np.int64)).to(self.dev),
                "refs": {}, "mns": {}}

    def ref(self, b, l, k, d, mode):
        key = (l, k, d, int(mode))
        if key not in b["refs"]:
            b["refs"][key] = self.oracle.batch(b["bases"], b["off"], l, k, d, self.OMODE[mode], threads=16)
        return b["refs"][key]

    def ref_mn(self, b, l, d, mode):
        key = (l, d, int(mode))
        if key not in b["mns"]:
            b["mns"][key] = self.oracle.batch_minimizers(b["bases"], b["off"], l, d, self.OMODE[mode])
        return b["mns"][key]

    def run(self, eng, b, l, k, d, mode, cap=None, arrays=KM, triples=False, mcap=None, legacy=False, serial=False, path=0, tag=""):
        """one s2k_extract_device call, every output checked against the oracle; cap / mcap default to the exact sizes"""
        torch, pkg = self.torch, self.pkg
        ref = self.ref(b, l, k, d, mode)
        rm = self.ref_mn(b, l, d, mode) if triples else None
        n, n_reads = ref["n"], len(b["off"]) - 1
        cap = n if cap is None else cap
        mcap = (max(rm["n"], 1) if mcap is None else mcap) if triples else 0
        bufs = {}
        o = pkg.DeviceOut()

        def buf(name, items):
            bufs[name] = torch.full(((items + GUARD) * ISZ[name],), SENT, dtype=torch.uint8, device=self.dev)
            setattr(o, name, bufs[name].data_ptr())

        o.km_capacity = cap
        buf("km_off", n_reads + 1)
        for f in arrays:
            buf(f, cap)
        if triples:
            o.mn_capacity = mcap
            buf("mn_off", n_reads + 1)
            for f in MN:
                buf(f, mcap)
        torch.cuda.synchronize()
        flags = (FLAG_MN if triples else 0) | (FLAG_SERIAL if serial else 0) | (FLAG_LEGACY if legacy else 0)
        p = pkg.Params(int(l), int(k), float(d), int(mode), flags)
        cnt = pkg.Counts()
        st = eng.lib.s2k_extract_device(eng.ctx, C.c_void_p(b["d_b"].data_ptr()), C.c_void_p(b["d_o"].data_ptr()), n_reads, len(b["bases"]),
                                        C.byref(p), C.byref(o), C.byref(cnt))
        got = {f: t.cpu().numpy() for f, t in bufs.items()}
        c = cnt.as_dict()
        ctx = (tag, int(mode), l, k, d, "cap", cap, "mcap", mcap, "arrays", arrays, "legacy" if legacy else "", "serial" if serial else "")
        short = cap < n or (triples and mcap < rm["n"])
        assert st == (S2K_ERR_CAPACITY if short else 0), ("status", ctx, st, n, rm and rm["n"])
        assert c["n_kminmers"] == n, ("n_kminmers", ctx, c["n_kminmers"], n)
        assert c["xor_hash"] == (int(np.bitwise_xor.reduce(ref["hash"])) if n else 0), ("xor_hash", ctx)
        assert c["n_reads"] == n_reads and c["n_bases"] == len(b["bases"]) and c["hash_bound"] == self.oracle.hash_bound(d), ("counts", ctx, c)
        assert c["path"] == path, ("path", ctx, c["path"])

        def same(name, raw, want, items, where):
            isz = ISZ[name]
            v = raw[: items * isz].view(DT[isz])
            if not (v == want[:items]).all():
                bad = int(np.nonzero(v != want[:items])[0][0])
                raise AssertionError(("mismatch", name, ctx, where, bad, int(v[bad]), int(want[bad])))
            tail = raw[items * isz:]
            if not (tail == SENT).all():  # past what may be written: the guard band (and the unused part of the capacity)
                bad = int(np.nonzero(tail != SENT)[0][0]) // isz + items
                raise AssertionError(("written past the end", name, ctx, where, "element", bad, "of", items))

        same("km_off", got["km_off"], ref["km_off"], n_reads + 1, "km_off")
        for f in arrays:
            same(f, got[f], ref[f], min(cap, n), "k-min-mers")
        if triples:
            assert c["n_minimizers"] == rm["n"], ("n_minimizers", ctx, c["n_minimizers"], rm["n"])
            same("mn_off", got["mn_off"], rm["mn_off"], n_reads + 1, "mn_off")
            for f, g in zip(MN, ("j", "jend", "hash")):
                same(f, got[f], rm[g], min(mcap, rm["n"]), "triples")
        return c


@pytest.fixture
def dv(oracle):
    v = Dev(oracle)
    yield v
    v.close()


def run_matrix(dv, names):
    """every input of inputs() through every route of the rows `names`"""
    HM = dv.pkg.HashMode
    for name, reads, l, ds, modes, many, serial_ok in inputs():
        b = dv.batch(reads)
        for d in ds:
            for mode in modes:
                for row in names:
                    for rt in VARIANTS[row][1]:
                        if rt["hpc_only"] and mode not in (HM.Hpc, HM.HpcSimd):
                            continue
                        if rt.get("serial") and not serial_ok:
                            continue
                        path = 2 if many and rt["path"] == 0 else rt["path"]
                        dv.run(dv.engine(rt["eng"]), b, l, rt["k"], d, mode, arrays=rt.get("arrays", KM), triples=rt.get("triples", False),
                               legacy=rt.get("legacy", False), serial=rt.get("serial", False), path=path, tag=(row, name))


def run_spec_n(dv):
    """(g) sparse -> dense -> sparse calls on one context at k = 5: the k-min-mer kernel fetches as many records per tile as the
    context's last call held (Desc::spec_n); > 64 tiles per call, so that every call updates the guess"""
    HM = dv.pkg.HashMode
    rng = np.random.default_rng(55)
    b = dv.batch([_rand(rng, int(n)) for n in rng.integers(4000, 40000, size=70)])
    eng = dv.pkg.Engine(0)
    try:
        for mode in (HM.Regular, HM.Hpc):
            for d in (0.002, 0.019, 0.05, 0.01, 0.001, 0.03):
                dv.run(eng, b, 31, 5, d, mode, tag="spec_n")
                dv.run(eng, b, 31, 10, d, mode, tag="spec_n")
    finally:
        eng.close()


LANE_SERIAL = ("desc_kminmer_kernel<10,true,true>", "desc_kminmer_kernel<5,true,true>")


@pytest.mark.gpu
@pytest.mark.parametrize("row", sorted(VARIANTS))
def test_variant_matrix(dv, row):
    run_matrix(dv, (row,))


@pytest.mark.gpu
def test_spec_n_guess_sparse_dense_sparse(dv):
    run_spec_n(dv)


@pytest.mark.gpu
def test_forced_chunks_take_the_lane_serial_kernel_without_staged_stores(dv):
    """S2K_DESC_CHUNKS=3: chunks 1 and 2 of a call run <5|10, true, false>, the last one <5|10, true, true> (a forced count still needs 64
    tiles per chunk: >= 192 tiles per call)"""
    HM = dv.pkg.HashMode
    rng = np.random.default_rng(77)
    reads = []
    for _, rs, l, _, _, many, _ in inputs():
        if l == 31 and not many and sum(len(r) for r in rs) < 1000000:
            reads += rs
    while sum(len(r) for r in reads) < 215 * T:
        reads.append(_rand(rng, int(rng.integers(3000, 60000)), hp=0.1))
    b = dv.batch(reads)
    eng = dv.engine("chunks3")
    for mode in (HM.Regular, HM.Hpc):
        for d in (0.01, 0.1, 0.001):
            for k in (5, 10):
                dv.run(eng, b, 31, k, d, mode, tag="chunks3")
        dv.run(eng, b, 31, 7, 0.01, mode, tag="chunks3")


CHILD = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from oracle import s2k_oracle
import test_kminmer_variants as m
dv = m.Dev(s2k_oracle.get())
try:
    m.run_matrix(dv, m.LANE_SERIAL)
    m.run_spec_n(dv)
finally:
    dv.close()
print("no-coal ok")
"""


@pytest.mark.gpu
def test_lane_serial_kernels_without_staged_stores():
    """The routes of the two COAL rows in one child process with S2K_KM_NO_COAL=1 (read once per process): every chunk of every call then runs
    <5|10, true, false>, the Regular family's included"""
    env = dict(os.environ, S2K_KM_NO_COAL="1")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, HERE)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no-coal ok" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-5000:])


SUBSETS = [tuple(f for i, f in enumerate(KM) if m >> i & 1) for m in range(16)]


@pytest.mark.gpu
def test_every_subset_of_the_output_arrays(dv):
    """s2k_device_out.hash / start / end / rev "may be NULL to skip": all 16 subsets (none = counts and km_off only), with and without
    the triples, on the descriptor path (k = 5, 10, 7), the legacy one (k = 40) and the read-serial one"""
    HM = dv.pkg.HashMode
    rng = np.random.default_rng(16)
    lens = [0, 31, 32, 500, T - 1, T, T + 1, 2 * T + 7, 20000, 40000, 144, 145, 3000, 17, 12000]
    b = dv.batch([_rand(rng, n, hp=0.2) for n in lens] + [_rand(rng, int(n)) for n in rng.integers(1000, 30000, size=12)])
    eng = dv.engine("plain")
    for arrays in SUBSETS:
        for triples in (False, True):
            for mode in (HM.Regular, HM.Hpc):
                for k, path in ((5, 0), (10, 0), (7, 0), (40, 2)):
                    dv.run(eng, b, 31, k, 0.02, mode, arrays=arrays, triples=triples, path=path, tag="subset")
                dv.run(eng, b, 31, 10, 0.02, mode, arrays=arrays, triples=triples, serial=True, path=1, tag="subset")


# the capacity routes: (engine, mode, k, options, path) -- COAL, lane-serial without COAL, <0,true,false>, FULL = false (triples / a NULL
# array), the two legacy kernels, S2K_FLAG_LEGACY_PATH and the read-serial path
CAP_ROUTES = [("plain", 0, 10, {}, 0), ("plain", 0, 5, {}, 0), ("chained", 1, 10, {}, 0), ("chained", 1, 5, {}, 0), ("plain", 1, 7, {}, 0),
              ("plain", 0, 10, {"triples": True}, 0), ("plain", 1, 5, {"arrays": ("hash", "start", "rev")}, 0), ("plain", 0, 40, {}, 2),
              ("plain", 1, 70, {}, 2), ("plain", 0, 10, {"legacy": True}, 2), ("plain", 1, 10, {"serial": True}, 1)]


def cap_batch(dv):
    """one read of exactly T bases per tile: the windows of tile r are km_off[r] .. km_off[r+1] of the oracle (minimizers: mn_off)"""
    rng = np.random.default_rng(9)
    return dv.batch([_rand(rng, T) for _ in range(24)])


def edges(off, total):
    c = {0, 1, total - 1, total, total + 1}
    for r in (1, 5, 12, 23):
        c.update((int(off[r]) - 1, int(off[r]), int(off[r]) + 1))
    return sorted(x for x in c if x >= 0)


@pytest.mark.gpu
def test_capacity_contract_with_guard_bands(dv):
    """cap = 0, 1, km_off[r] - 1 / km_off[r] / km_off[r] + 1 (a tile that straddles the capacity, one that ends exactly at it), n - 1, n, n + 1:
    S2K_ERR_CAPACITY exactly when cap < n, complete counts, xor_hash and km_off, the first cap items of every given array, nothing past them"""
    b = cap_batch(dv)
    for eng, mode, k, opt, path in CAP_ROUTES:
        ref = dv.ref(b, 31, k, 0.01, dv.pkg.HashMode(mode))
        assert ref["n"] > 1000
        for cap in edges(ref["km_off"], ref["n"]):
            dv.run(dv.engine(eng), b, 31, k, 0.01, dv.pkg.HashMode(mode), cap=cap, path=path, tag=("capacity", eng), **opt)


@pytest.mark.gpu
def test_minimizer_capacity_contract_with_guard_bands(dv):
    """the same edges for mn_capacity (0 means "no triples": from 1), on the descriptor, legacy and read-serial paths"""
    b = cap_batch(dv)
    for mode in (dv.pkg.HashMode.Regular, dv.pkg.HashMode.Hpc):
        rm = dv.ref_mn(b, 31, 0.01, mode)
        for mcap in edges(rm["mn_off"], rm["n"]):
            if mcap == 0:
                continue
            for k, opt, path in ((10, {}, 0), (7, {"arrays": ("end",)}, 0), (40, {}, 2), (10, {"serial": True}, 1)):
                dv.run(dv.engine("plain"), b, 31, k, 0.01, mode, triples=True, mcap=mcap, path=path, tag="mn capacity", **opt)


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------
def kernel_names(asm):
    """the k-min-mer kernels among the .name: lines of a gfx950 device assembly, in the spelling of VARIANTS"""
    out = set()
    for m in re.finditer(r"^\s*\.name:\s+(\S+)$", asm, re.M):
        s = m.group(1)
        d = re.search(r"19desc_kminmer_kernelILi(\d+)ELb([01])ELb([01])E", s)
        if d:
            out.add("desc_kminmer_kernel<%s,%s,%s>" % (d.group(1), "true" if d.group(2) == "1" else "false", "true" if d.group(3) == "1" else "false"))
        elif re.search(r"\d+(kminmer_kernel(?:_fast)?)E", s):
            out.add(re.search(r"\d+(kminmer_kernel(?:_fast)?)E", s).group(1))
        elif "kminmer" in s:
            out.add("unrecognised: " + s)
    return out


def test_variant_table_lists_every_kernel_in_the_code_object(tmp_path):
    csrc = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    names = set()
    for src in ("s2k_desc.hip", "s2k_kminmer.hip"):
        asm = tmp_path / (src + ".s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", str(asm), src],
                           cwd=csrc, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (src, r.stderr[-3000:])
        names |= kernel_names(asm.read_text())
    assert names == set(VARIANTS), ("kernels without a row", sorted(names - set(VARIANTS)), "rows without a kernel", sorted(set(VARIANTS) - names))
