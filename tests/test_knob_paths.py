"""GPU tier: the kernel and host paths that the shipped library's environment knobs select (README.md, "Environment knobs"), each in a child
process (every knob is read once per process or per context) and each against the oracle or a plain reference:

- S2K_HPC_SINGLE_PASS: standalone hpc / encode_rle in one pass with a decoupled look-back (hpc_segment_index2_kernel, hpc_segment_lb_kernel):
  the existing batches and the fuzz run under it, the look-back's edges, a too-small output, and > 1 Gbp against a torch reference.  Every
  such child runs with S2K_TRACE=1 and must not report a look-back that gave up: the call would then have run the two-pass kernels.
- S2K_DESC_TAIL x S2K_DESC_CHUNKS: tapered chunks of the two-stream descriptor pipeline, tiny and empty chunks included.
- S2K_PIN_RESULTS=0 x S2K_COPY_THREADS, S2K_NUMA_BIND=0: s2k_extract drained through the staging ring, s2k_run_file with 1 / 3 copy threads.

The functions without a test_ prefix are what the children run (python -c "import test_knob_paths as T; T.fn(args)")."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gpu_util import FIELDS, OMODE, pkg, rand_read

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("S2K_HPC_SINGLE_PASS", "S2K_DESC_TAIL", "S2K_DESC_CHUNKS", "S2K_PIN_RESULTS", "S2K_COPY_THREADS", "S2K_NUMA_BIND", "S2K_TRACE", "S2K_FULL_RUNS")
SINGLE_PASS = {"S2K_HPC_SINGLE_PASS": "1", "S2K_TRACE": "1"}
GAVE_UP = "single-pass hpc look-back gave up"  # (s2k_hpc_device_ex under S2K_TRACE)
MN_FIELDS = ("mn_off", "mn_j", "mn_jend", "mn_hash")


def _run(argv, env, timeout):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    p = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, env=e)
    assert p.returncode == 0, (argv[-3:], env, p.returncode, p.stdout[-2000:], p.stderr[-3000:])
    if "S2K_HPC_SINGLE_PASS" in env:
        assert GAVE_UP not in p.stderr, ("a single-pass look-back gave up: the call ran the two-pass path, which is what was tested", p.stderr[-2000:])
    return p


def _child(fn, *args, env=None, timeout=600):
    """T.fn(*args) of this module in a fresh process whose environment holds none of the knobs but `env`"""
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_knob_paths as T\nT.%s(*sys.argv[1:])\n" % (ROOT, TESTS, fn)
    return _run([sys.executable, "-c", code, *[str(a) for a in args]], env or {}, timeout)


# ---- standalone hpc ----------------------------------------------------------------------------------------------------------------------

def _hpc_expect(oracle, reads, rle):
    which = 1 if rle else 2  # encode_rle / encode_rle_simd (any repeated byte collapses)
    exp = [oracle.hpc(r, which) if len(r) else (b"", np.zeros(0, dtype=np.uint64)) for r in reads]
    s = b"".join(e[0] for e in exp)
    p = np.concatenate([np.asarray(e[1], dtype=np.uint32) for e in exp] + [np.zeros(0, dtype=np.uint32)])
    off = np.concatenate([[0], np.cumsum([len(e[0]) for e in exp])]).astype(np.int64)
    return s, p, off


def _upload(reads):
    import torch

    dev = torch.device("cuda", 0)
    bases, off = pkg.pack_reads(reads)
    d_b = torch.zeros(len(bases) + 64, dtype=torch.uint8, device=dev)  # (16-byte aligned: the segment-parallel kernels)
    if len(bases):
        d_b[:len(bases)] = torch.from_numpy(bases).to(dev)
    return d_b, torch.from_numpy(off.astype(np.int64)).to(dev), len(bases)


BYTE_GUARD, POS_GUARD = 0xA5, 0x5A5A5A5A


def hpc_exact(eng, oracle, reads, rle, tag):
    """every output at output offsets 0-3 with the exact capacity, sentinels before and behind the outputs; the sizes-only call"""
    import torch

    dev = torch.device("cuda", 0)
    es, ep, eo = _hpc_expect(oracle, reads, rle)
    n = len(es)
    d_b, d_o, nb = _upload(reads)
    ctx = (tag, rle, len(reads), nb, n)
    for o_shift in (0, 1, 2, 3):
        d_ho = torch.full((len(reads) + 1,), -1, dtype=torch.int64, device=dev)
        d_h = torch.full((n + 4 + 64,), BYTE_GUARD, dtype=torch.uint8, device=dev)
        d_p = torch.full((n + 4 + 64,), POS_GUARD, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        got = eng.hpc_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), nb, d_ho.data_ptr(), d_h.data_ptr() + o_shift, d_p.data_ptr() + 4 * o_shift, n, rle=rle)
        assert got == n, ("runs", ctx, o_shift, got)
        assert (d_ho.cpu().numpy() == eo).all(), ("hpc_off", ctx, o_shift)
        h = d_h.cpu().numpy()
        assert h[o_shift:o_shift + n].tobytes() == es, ("bytes", ctx, o_shift)
        assert (h[:o_shift] == BYTE_GUARD).all() and (h[o_shift + n:] == BYTE_GUARD).all(), ("bytes written outside", ctx, o_shift)
        p = d_p.cpu().numpy()
        assert (p[o_shift:o_shift + n].view(np.uint32) == ep).all(), ("positions", ctx, o_shift)
        assert (p[:o_shift] == POS_GUARD).all() and (p[o_shift + n:] == POS_GUARD).all(), ("positions written outside", ctx, o_shift)
    d_ho = torch.full((len(reads) + 1,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert eng.hpc_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), nb, d_ho.data_ptr(), 0, 0, 0, rle=rle) == n, ("sizes only", ctx)
    assert (d_ho.cpu().numpy() == eo).all(), ("sizes only: hpc_off", ctx)


def hpc_capacity(eng, oracle, reads, rle, tag):
    """capacity n // 2 + {0, 1, 2, 3} at output offsets 0-3: status 7, the first `capacity` outputs exact, hpc_off complete, the guard
    band behind the capacity (and the bytes before the offset) untouched"""
    import torch

    dev = torch.device("cuda", 0)
    es, ep, eo = _hpc_expect(oracle, reads, rle)
    n = len(es)
    assert n > 8
    d_b, d_o, nb = _upload(reads)
    for extra in (0, 1, 2, 3):
        cap = n // 2 + extra
        for o_shift in (0, 1, 2, 3):
            ctx = (tag, rle, cap, o_shift)
            d_ho = torch.full((len(reads) + 1,), -1, dtype=torch.int64, device=dev)
            d_h = torch.full((o_shift + cap + 256,), BYTE_GUARD, dtype=torch.uint8, device=dev)
            d_p = torch.full((o_shift + cap + 256,), POS_GUARD, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            with pytest.raises(pkg.S2kError) as e:
                eng.hpc_device(d_b.data_ptr(), d_o.data_ptr(), len(reads), nb, d_ho.data_ptr(), d_h.data_ptr() + o_shift, d_p.data_ptr() + 4 * o_shift, cap, rle=rle)
            assert e.value.status == 7, ctx
            assert (d_ho.cpu().numpy() == eo).all(), ("hpc_off", ctx)
            h = d_h.cpu().numpy()
            assert h[o_shift:o_shift + cap].tobytes() == es[:cap], ("bytes", ctx)
            assert (h[:o_shift] == BYTE_GUARD).all() and (h[o_shift + cap:] == BYTE_GUARD).all(), ("bytes written outside the capacity", ctx)
            p = d_p.cpu().numpy()
            assert (p[o_shift:o_shift + cap].view(np.uint32) == ep[:cap]).all(), ("positions", ctx)
            assert (p[:o_shift] == POS_GUARD).all() and (p[o_shift + cap:] == POS_GUARD).all(), ("positions written outside the capacity", ctx)


SEG = 4096  # bytes per block of the segment-parallel kernels (HS_SEG)


def _to_total(rng, total, hp, maxlen=9000):
    lens = []
    while sum(lens) < total:
        lens.append(int(rng.integers(0, maxlen)))
    lens[-1] -= sum(lens) - total
    return [rand_read(rng, n, hp=hp, odd=0.05) for n in lens]


def hpc_edge_batches():
    rng = np.random.default_rng(4096)
    out = []
    for k in (1, 2, 5):  # n_bases on and next to a segment end
        for d in (-1, 0, 1):
            out.append(("n_bases=%d*4096%+d" % (k, d), _to_total(rng, k * SEG + d, 0.4, maxlen=2500)))
    # empty reads at n_bases: the last entries of the read table on the end of the data (the end of the last segment, or inside it)
    out.append(("trailing-empty-on-seg-end", _to_total(rng, 3 * SEG, 0.3) + [b""] * 5))
    out.append(("trailing-empty", _to_total(rng, 3 * SEG + 100, 0.3) + [b""] * 3))
    out.append(("tiny-reads-to-seg-end", _to_total(rng, 2 * SEG, 0.5, maxlen=9) + [b""] * 300))  # > 256 table entries in a segment, the end among them
    out.append(("leading-and-trailing-empty", [b"", b""] + _to_total(rng, 2 * SEG - 1, 0.3) + [b""]))
    # runs over whole segments: blocks with no run head publish 0; a read start inside a run of the read before is a head of its own
    out.append(("whole-segment-runs", [rand_read(rng, 1000), b"A" * (3 * SEG + 7), b"A" * 5000, rand_read(rng, 200), b"C" * (3 * SEG),
                                       b"C" * SEG, b"X" * 9000, rand_read(rng, 3000, hp=0.5), b"n" * (2 * SEG + 1)]))
    out.append(("one-read", [rand_read(rng, 10000, hp=0.4)]))
    out.append(("one-base", [b"G"]))
    out.append(("one-base-among-empty", [b"", b"T", b""]))
    out.append(("one-run", [b"A" * (2 * SEG + 3)]))
    # more segments than one look-back window of 256 words (and, in the second, most of them without a run head)
    out.append((">256-segments", _to_total(rng, 300 * SEG + 17, 0.5, maxlen=40000)))
    out.append((">1024-segments-mostly-one-run", [rand_read(rng, 100), b"T" * (1100 * SEG), rand_read(rng, 5000, hp=0.3), b"", b"T" * 70000]))
    return out


def hpc_edges_and_capacity():
    """child: every edge batch through hpc_exact with both run rules; the capacity checks on three of them"""
    from oracle import s2k_oracle

    eng, oracle = pkg.Engine(0), s2k_oracle.get()
    batches = hpc_edge_batches()
    for tag, reads in batches:
        for rle in (False, True):
            hpc_exact(eng, oracle, reads, rle, tag)
    for tag, reads in batches:
        if tag in ("n_bases=5*4096+0", "whole-segment-runs", ">256-segments"):
            for rle in (False, True):
                hpc_capacity(eng, oracle, reads, rle, tag)
    print("ok", len(batches))


def hpc_existing_cases():
    """child: the batches of test_standalone_hpc_batches and test_encode_rle_flavour (s2k_hpc_device / _ex, both run rules)"""
    import test_gpu_parity as G
    from conftest import GOLD
    from oracle import s2k_oracle

    eng, oracle = pkg.Engine(0), s2k_oracle.get()
    ecoli = open(os.path.join(GOLD, "ecoli.genome.100k.fa")).read().split("\n")[1].encode()
    G.test_standalone_hpc(eng, oracle, ecoli)
    G.test_standalone_hpc_batches(eng, oracle)
    G.test_encode_rle_flavour(eng, oracle, ecoli)
    print("ok")


def test_single_pass_hpc_existing_cases_and_fuzz():
    _child("hpc_existing_cases", env=SINGLE_PASS)
    p = _run([sys.executable, os.path.join(ROOT, "tools", "fuzz_hpc.py"), "78", "200"], SINGLE_PASS, 600)
    assert "0 mismatches" in p.stdout, p.stdout[-1500:]


@pytest.mark.parametrize("path", ["single_pass", "two_pass"])
def test_hpc_lookback_edges_and_capacity(path):
    """n_bases on segment ends, the read table's last entries on the end of the data, blocks without a run head, one read, one base,
    more segments than a look-back window; a too-small output at every offset.  Both paths: the capacity checks are new for either."""
    p = _child("hpc_edges_and_capacity", env=SINGLE_PASS if path == "single_pass" else {})
    assert p.stdout.strip().startswith("ok"), p.stdout


# -- at scale: a plain torch restatement of the operation, on the device, in chunks

def _rle_lut(dev):
    import torch

    lut = torch.zeros(256, dtype=torch.bool, device=dev)
    lut[torch.tensor(list(b"ACTGactgNn"), device=dev)] = True
    return lut


def hpc_reference(d_b, n, d_off, rle, visit, chunk=1 << 26):
    """head = a non-empty read starts here, or b[i] != b[i-1], or (encode_rle's rule) b[i] is outside ACTGactgNn; out slot of a head = heads
    before it; byte = b[i], position = i - start of its read; hpc_off[r] = heads before read_off[r].  Calls visit(g0, bytes, positions) for
    every chunk's heads in order; returns (hpc_off, number of heads)."""
    import torch

    dev = d_b.device
    n_reads = d_off.numel() - 1
    starts = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    ne = d_off[1:] > d_off[:-1]
    starts[d_off[:-1][ne]] = True
    lut = _rle_lut(dev) if rle else None
    hpc_off = torch.full((n_reads + 1,), -1, dtype=torch.int64, device=dev)
    g = 0
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        cur = d_b[a:b].to(torch.int16)
        prev = torch.empty_like(cur)
        prev[1:] = cur[:-1]
        prev[0] = int(d_b[a - 1].item()) if a else -1
        h = (cur != prev) | starts[a:b]
        if rle:
            h |= ~lut[d_b[a:b].long()]
        cs = torch.cumsum(h, 0, dtype=torch.int64)
        sel = (d_off >= a) & (d_off < b)
        rel = d_off[sel] - a
        hpc_off[sel] = g + cs[rel] - h[rel].to(torch.int64)
        idx = torch.nonzero(h).squeeze(1) + a
        rstart = d_off[torch.searchsorted(d_off, idx, right=True) - 1]
        visit(g, d_b[idx], idx - rstart)
        g += int(idx.numel())
        del cur, prev, h, cs, idx, rstart
    hpc_off[d_off == n] = g
    return hpc_off, g


def _fold(t, n, chunk=1 << 26):
    """SUM t[i] (2 i + 1) mod 2^64 over i < n"""
    import torch

    acc = 0
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        w = torch.arange(a, b, dtype=torch.int64, device=t.device) * 2 + 1
        acc = (acc + int((t[a:b].to(torch.int64) * w).sum().item())) & ((1 << 64) - 1)
    return acc


def _scale_input(eng, which):
    """(d_b, d_off, n_bases, rle): > 1 Gbp, generated on the device"""
    import torch

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1 if which == "uniform" else 2)
    if which == "uniform":
        lens = rng.integers(0, 40000, size=60000)
        lens[rng.random(len(lens)) < 0.02] = 0
        lens = np.concatenate([lens, [0, 0, 0]])  # empty reads at n_bases
        off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        n = int(off[-1])
        d_b = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        eng.synth_bases_device(11, 0, n, d_b.data_ptr())
        eng.lib.s2k_sync(eng.ctx, None)
        # bytes outside ACTGactgNn (encode_rle keeps their runs), runs of N and n, here and there
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        for ch, cnt in ((ord("X"), n // 3000), (ord("N"), n // 5000), (ord("n"), n // 9000), (ord("-"), n // 20000)):
            p = torch.randint(0, n - 8, (cnt,), device=dev, generator=gen)
            for j in range(int(ch) % 4 + 1):
                d_b[p + j] = ch
        d_off = torch.from_numpy(off).to(dev)
        rle = True
    else:
        lens = eng.synth_hifi_lengths(3, 0, 80000)
        nr = int(np.searchsorted(np.cumsum(lens), 1_000_000_000)) + 1
        off = np.concatenate(([0], np.cumsum(lens[:nr]))).astype(np.int64)
        n = int(off[-1])
        d_b = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        d_off = torch.from_numpy(off).to(dev)
        torch.cuda.synchronize()
        eng.synth_hifi_device(3, 0, nr, d_off.data_ptr(), d_b.data_ptr())
        eng.lib.s2k_sync(eng.ctx, None)
        for a in rng.integers(0, n - 30000, size=300):  # runs longer than a segment: blocks with no run head
            d_b[int(a):int(a) + int(rng.integers(4000, 30000))] = int(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8)))
        rle = False
    torch.cuda.synchronize()
    assert n > 1_000_000_000 and n // SEG > 244_000
    return d_b, d_off, n, rle


def hpc_at_scale(compare):
    """child: both > 1 Gbp batches through s2k_hpc_device_ex; prints one JSON line of whole-run folds per batch.  compare=1: every output
    element against hpc_reference, which is first checked against the oracle on a sample of reads"""
    import torch

    from oracle import s2k_oracle

    eng, oracle = pkg.Engine(0), s2k_oracle.get()
    dev = torch.device("cuda", 0)
    for which in ("uniform", "hifi"):
        d_b, d_off, n, rle = _scale_input(eng, which)
        n_reads = d_off.numel() - 1
        d_ho = torch.full((n_reads + 1,), -1, dtype=torch.int64, device=dev)
        sizes = eng.hpc_device(d_b.data_ptr(), d_off.data_ptr(), n_reads, n, d_ho.data_ptr(), 0, 0, 0, rle=rle)
        d_h = torch.empty(sizes + 64, dtype=torch.uint8, device=dev)
        d_p = torch.empty(sizes + 64, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        runs = eng.hpc_device(d_b.data_ptr(), d_off.data_ptr(), n_reads, n, d_ho.data_ptr(), d_h.data_ptr(), d_p.data_ptr(), sizes, rle=rle)
        assert runs == sizes == int(d_ho[-1].item()), (which, "runs of the sizes-only call / the call / hpc_off[n_reads]", sizes, runs, int(d_ho[-1].item()))
        if int(compare):
            # the reference itself against the oracle, on ~300 reads spread over the batch
            off_h = d_off.cpu().numpy()
            ids = np.unique(np.concatenate([np.random.default_rng(9).choice(n_reads, size=300, replace=False), [0, n_reads - 1]]))
            reads = [d_b[int(off_h[r]):int(off_h[r + 1])].cpu().numpy().tobytes() for r in ids]
            es, ep, eo = _hpc_expect(oracle, reads, rle)
            s_b, s_o, s_n = _upload(reads)
            parts = []
            s_ho, s_g = hpc_reference(s_b, s_n, s_o, rle, lambda g0, bb, pp: parts.append((bb.cpu().numpy(), pp.cpu().numpy())))
            assert s_g == len(es) and (s_ho.cpu().numpy() == eo).all(), (which, "reference vs oracle: hpc_off")
            assert np.concatenate([x[0] for x in parts]).tobytes() == es, (which, "reference vs oracle: bytes")
            assert (np.concatenate([x[1] for x in parts]) == ep.astype(np.int64)).all(), (which, "reference vs oracle: positions")
            bad = []

            def visit(g0, bb, pp):
                m = int(bb.numel())
                if g0 + m > runs:
                    bad.append(("more heads than runs", g0 + m, runs))
                    return
                for f, got, want in (("bytes", d_h[g0:g0 + m], bb), ("positions", d_p[g0:g0 + m].to(torch.int64), pp)):
                    ne = torch.nonzero(got != want)
                    if ne.numel() and len(bad) < 8:
                        i = int(ne[0, 0].item())
                        bad.append((f, "slot", g0 + i, int(got[i].item()), int(want[i].item()), "mismatches in chunk", int(ne.numel())))

            ref_ho, ref_g = hpc_reference(d_b, n, d_off, rle, visit)
            assert not bad, (which, bad)
            assert ref_g == runs, (which, "runs", runs, ref_g)
            ne = torch.nonzero(ref_ho != d_ho)
            assert ne.numel() == 0, (which, "hpc_off", int(ne[0, 0].item()))
        print(json.dumps({"batch": which, "n_bases": n, "n_reads": n_reads, "runs": runs, "fold_hpc": _fold(d_h, runs), "fold_pos": _fold(d_p, runs),
                          "fold_hpc_off": _fold(d_ho, n_reads + 1)}), flush=True)
        del d_b, d_off, d_ho, d_h, d_p
        torch.cuda.empty_cache()


def test_single_pass_hpc_at_scale_equals_reference_and_two_pass():
    """> 1 Gbp (> 244 000 segments, so look-backs over many windows and blocks far apart in time): a uniform batch with bytes outside
    ACTGactgNn under encode_rle's rule, a HiFi-like one with long runs under the any-byte rule.  The single-pass child compares every
    output with the torch reference; the two-pass child's whole-run folds must equal the single-pass child's."""
    one = _child("hpc_at_scale", 1, env=SINGLE_PASS, timeout=900).stdout.strip().splitlines()
    two = _child("hpc_at_scale", 0, timeout=900).stdout.strip().splitlines()
    one = [json.loads(x) for x in one if x.startswith("{")]
    two = [json.loads(x) for x in two if x.startswith("{")]
    assert len(one) == len(two) == 2 and one == two, (one, two)


# ---- tapered chunks of the descriptor pipeline -----------------------------------------------------------------------------------------

def _chunk_inputs():
    rng = np.random.default_rng(7)
    out = {}
    lens = rng.integers(3000, 90000, size=440)  # ~20 Mbp: ~2 200 Hpc tiles, reads straddle every chunk boundary
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(off[-1]))]
    out["main"] = (np.repeat(b, rng.choice([1, 1, 1, 2, 5], size=len(b)))[: int(off[-1])].copy(), off)
    # ~900 tiles: S2K_DESC_CHUNKS=13 still gives 13 chunks, and a tail of 0.999 leaves the twelve before the last less than one tile
    lens = rng.integers(3000, 40000, size=385)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(off[-1]))]
    out["small"] = (np.repeat(b, rng.choice([1, 1, 1, 2, 5], size=len(b)))[: int(off[-1])].copy(), off)
    # low complexity: tiles take space from the overflow region the chunks share
    lens = rng.integers(20000, 400000, size=12)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    b = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(off[-1]))]
    out["lowc"] = (np.repeat(b, rng.choice([1, 1, 3, 60, 700], size=len(b)))[: int(off[-1])].copy(), off)
    return out


CHUNK_CALLS = [("main", m, 31, 10, 0.01) for m in (1, 3, 0)] + [("small", m, 31, 10, 0.01) for m in (1, 3, 0)] + \
              [("lowc", 0, 15, 1, 0.1), ("lowc", 1, 15, 3, 0.5), ("lowc", 3, 15, 10, 0.05)]


COUNT_FIELDS = ("n_reads", "n_bases", "n_minimizers", "n_kminmers", "xor_hash", "hash_bound", "path")


def chunk_calls(out):
    """child: every call of CHUNK_CALLS with minimizer triples; all outputs into one .npz"""
    eng = pkg.Engine(0)
    inputs = _chunk_inputs()
    res = {}
    for i, (name, mode, l, k, d) in enumerate(CHUNK_CALLS):
        bases, off = inputs[name]
        r = eng.extract(bases, off, l, k, d, mode, want_minimizers=True)
        assert r["counts"]["path"] == 0, (name, mode, r["counts"])
        for f in FIELDS + MN_FIELDS:
            res["%d_%s" % (i, f)] = r[f]
        res["%d_counts" % i] = np.array([r["counts"][f] for f in COUNT_FIELDS], dtype=np.uint64)  # (a tile run twice XORs its hashes out again)
    np.savez(out, **res)
    print("ok")


def test_tapered_chunks_equal_the_default(oracle, tmp_path):
    """S2K_DESC_TAIL in {0.05, 0.5, 0.95, 0.999} x S2K_DESC_CHUNKS in {unset, 3, 13}: chunks far below the 64-tile minimum of a forced count,
    empty ones (tail 0.999), Hpc and HpcSimd with triples, the Regular family (one chunk unless forced): byte for byte the default's outputs,
    and the most tapered configuration field by field the oracle's."""
    base = str(tmp_path / "default.npz")
    _child("chunk_calls", base)
    ref = np.load(base)
    for chunks in ("", "3", "13"):
        for tail in ("0.05", "0.5", "0.95", "0.999"):
            env = {"S2K_DESC_TAIL": tail}
            if chunks:
                env = {"S2K_DESC_TAIL": tail, "S2K_DESC_CHUNKS": chunks}
            out = str(tmp_path / ("t%s_c%s.npz" % (tail, chunks or "default")))
            _child("chunk_calls", out, env=env)
            got = np.load(out)
            for key in ref.files:
                assert np.array_equal(got[key], ref[key]), (env, key, CHUNK_CALLS[int(key.split("_")[0])])
    got = np.load(str(tmp_path / "t0.999_c13.npz"))
    inputs = _chunk_inputs()
    for i, (name, mode, l, k, d) in enumerate(CHUNK_CALLS):
        bases, off = inputs[name]
        r = oracle.batch(bases, off, l, k, d, OMODE[pkg.HashMode(mode)], threads=8)
        for f in FIELDS:
            assert np.array_equal(got["%d_%s" % (i, f)], r[f]), ("oracle", CHUNK_CALLS[i], f)
        rm = oracle.batch_minimizers(bases, off, l, d, OMODE[pkg.HashMode(mode)])
        for a, b in zip(MN_FIELDS, ("mn_off", "j", "jend", "hash")):
            assert np.array_equal(got["%d_%s" % (i, a)], rm[b]), ("oracle", CHUNK_CALLS[i], a)
        c = dict(zip(COUNT_FIELDS, (int(x) for x in got["%d_counts" % i])))
        assert (c["n_kminmers"], c["n_reads"], c["n_bases"]) == (r["n"], len(off) - 1, int(off[-1])), ("oracle", CHUNK_CALLS[i], c)
        assert c["xor_hash"] == (int(np.bitwise_xor.reduce(r["hash"])) if r["n"] else 0), ("oracle", CHUNK_CALLS[i], "xor_hash")


# ---- host drain and copy threads --------------------------------------------------------------------------------------------------------

def _drain_input():
    """> 70 Mbp (two 64 MiB ring chunks) with N runs, odd bytes, bytes >= 0x80 and a lower-case stretch (as test_packed_host_transfer_is_exact)"""
    rng = np.random.default_rng(92)
    n = (64 << 20) + 5_000_000
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
    for a in rng.integers(0, n - 100, size=3000):
        s[a:a + int(rng.integers(1, 40))] = ord("N")
    odd = rng.integers(0, n, size=20000)
    s[odd] = np.frombuffer(b"nacgtXR*-\xc1\x00", dtype=np.uint8)[rng.integers(0, 11, size=len(odd))]
    s[(64 << 20) + 100_000:(64 << 20) + 4_600_000] |= 0x20
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.integers(2000, 60000)))
    off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n).astype(np.uint64)
    return s, off


def _big_fasta_reads():
    """several pinned chunks of FASTA text (as test_run_file_many_batches_fasta_and_fastq)"""
    rng = np.random.default_rng(18)
    big = []
    for i in range(12):
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(rng.integers(1_500_000, 3_500_000)))].copy()
        for q in rng.integers(0, len(a) - 200, size=40):
            a[q:q + int(rng.integers(1, 150))] = ord("N")
        if i in (5, 6):
            a |= 0x20
        big.append(a.tobytes())
    return big


def drain_calls(npy_dir, out, fasta):
    """child: s2k_extract host to host with triples (Hpc) on the drain input, and s2k_run_file on the FASTA; totals as one JSON line"""
    eng = pkg.Engine(0)
    s, off = np.load(os.path.join(npy_dir, "s.npy")), np.load(os.path.join(npy_dir, "off.npy"))
    r = eng.extract(s, off, 31, 10, 0.01, pkg.HashMode.Hpc, want_minimizers=True)
    np.savez(out, **{f: r[f] for f in FIELDS + MN_FIELDS})
    tot = eng.run_file(fasta, 31, 7, 0.01, pkg.HashMode.Hpc)
    print(json.dumps({f: tot[f] for f in ("n_reads", "n_bases", "n_kminmers", "xor_hash")}))


def test_host_drain_and_copy_threads(oracle, tmp_path):
    """S2K_PIN_RESULTS in {unset, 0} x S2K_COPY_THREADS in {1, 3, 16}, and S2K_NUMA_BIND=0: s2k_extract's H2D ring (2-bit packing split
    over the copy threads) and its drain (direct DMA into pinned results, or the staging ring and the copy threads) give the oracle's
    fields; s2k_run_file's totals over a multi-chunk FASTA are the oracle's whatever the number of copy threads."""
    from test_fastx import _write_fasta

    s, off = _drain_input()
    np.save(tmp_path / "s.npy", s)
    np.save(tmp_path / "off.npy", off)
    ref = oracle.batch(s, off, 31, 10, 0.01, OMODE[pkg.HashMode.Hpc], threads=8)
    rm = oracle.batch_minimizers(s, off, 31, 0.01, OMODE[pkg.HashMode.Hpc])
    big = _big_fasta_reads()
    fa = tmp_path / "big.fa"
    _write_fasta(fa, big, width=70)
    bb, bo = pkg.pack_reads(big)
    rb = oracle.batch(bb, bo, 31, 7, 0.01, OMODE[pkg.HashMode.Hpc], threads=8)
    want = {"n_reads": len(big), "n_bases": len(bb), "n_kminmers": rb["n"], "xor_hash": int(np.bitwise_xor.reduce(rb["hash"]))}
    envs = [{"S2K_COPY_THREADS": "1"}, {"S2K_COPY_THREADS": "3"}, {"S2K_COPY_THREADS": "16"},
            {"S2K_PIN_RESULTS": "0", "S2K_COPY_THREADS": "1"}, {"S2K_PIN_RESULTS": "0", "S2K_COPY_THREADS": "3"},
            {"S2K_PIN_RESULTS": "0", "S2K_COPY_THREADS": "16"}, {"S2K_NUMA_BIND": "0"}]
    for i, env in enumerate(envs):
        out = str(tmp_path / ("drain%d.npz" % i))
        p = _child("drain_calls", str(tmp_path), out, str(fa), env=env)
        assert json.loads(p.stdout.strip().splitlines()[-1]) == want, (env, p.stdout[-500:])
        got = np.load(out)
        assert len(got["hash"]) == ref["n"], env
        for f in FIELDS:
            assert np.array_equal(got[f], ref[f]), (env, f)
        for a, b in zip(MN_FIELDS, ("mn_off", "j", "jend", "hash")):
            assert np.array_equal(got[a], rm[b]), (env, a)
