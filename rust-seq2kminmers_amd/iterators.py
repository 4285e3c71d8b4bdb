"""The reference's per-read interface over the batch calls: KminmersIterator, the minimizer iterators, hpc and encode_rle."""
import numpy as np

from ._abi import HashMode, S2kError, torch
from ._args import _as_u8
from .engine import Engine

_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


class KminmerHash:
    """src/kminmer.rs:128-135; equality and ordering by `hash` only (src/kminmer.rs:181-204)."""
    __slots__ = ("hash", "start", "end", "offset", "rev")

    def __init__(self, hash, start, end, offset, rev):
        self.hash, self.start, self.end, self.offset, self.rev = hash, start, end, offset, rev

    @classmethod
    def new_from_hash(cls, hash, start, end, offset, rev):  # src/kminmer.rs:169-177
        return cls(hash, start, end, offset, rev)

    def get_hash(self):  # src/kminmer.rs:162-164
        return self.hash

    def __eq__(self, o):
        return self.hash == o.hash

    def __lt__(self, o):
        return self.hash < o.hash

    def __hash__(self):
        return hash(self.hash)

    def __repr__(self):  # Debug formatting of the Rust struct
        return "KminmerHash { hash: %d, start: %d, end: %d, offset: %d, rev: %s }" % (
            self.hash, self.start, self.end, self.offset, "true" if self.rev else "false")


class KminmersIterator:
    """Per-read facade with the reference's constructor signature (src/lib.rs:89) and Iterator shape
    (src/lib.rs:179-181).  One GPU call per read is the wrong granularity for throughput -- use
    Engine.extract for batches; this class exists so reference-style call sites and tests read the same.
    Parameter violations that panic in the reference raise S2kError here."""

    def __init__(self, seq, l, k, density, mode=HashMode.Hpc, engine=None):
        eng = engine or default_engine()
        r = eng.extract_reads([seq], l, k, density, mode)
        self._r = r
        self._i = 0

    @classmethod
    def new(cls, seq, l, k, density, mode, engine=None):
        return cls(seq, l, k, density, mode, engine)

    def __iter__(self):
        return self

    def __next__(self):
        i = self._i
        if i >= self._r["n"]:
            raise StopIteration
        self._i += 1
        r = self._r
        return KminmerHash(int(r["hash"][i]), int(r["start"][i]), int(r["end"][i]), i, bool(r["rev"][i]))


class _MinimizerTriples:
    """The crate's minimizer iterators (re-exported at src/lib.rs:6-13) over S2K_FLAG_WANT_MINIMIZERS: one GPU call per
    sequence -- the wrong granularity for throughput (use Engine.extract(..., want_minimizers=True) for batches); these
    classes exist so reference-style call sites read the same.  Like the reference they take the u32 `hash_bound`, not a
    density.  l > len(seq) raises as KSizeOutOfRange does (src/nthash_hpc.rs:117-121); len(seq) == l is accepted as in the reference."""
    _mode = None

    def __init__(self, seq, l, hash_bound, engine=None):
        a = _as_u8(seq)
        if l > len(a):
            raise S2kError(2, "K size %d is out of range for the given sequence size %d" % (l, len(a)))  # src/nthash_hpc.rs:19-22
        eng = engine or default_engine()
        d = float(eng.lib.s2k_density_for_bound(int(hash_bound)))
        keep = None
        if len(a) == l:
            # seq.len() == l is accepted by the reference's iterators (only l > len is KSizeOutOfRange, src/nthash_hpc.rs:117-121):
            # the scalar Hpc iterator then yields nothing (its only l-mer is the last one, dropped at :265-267); the two SIMD
            # iterators may yield the single l-mer.  KminmersIterator never makes this call (src/lib.rs:97), and the kernels
            # follow it (len <= l: nothing) -- so the l-mer is computed ON THE GPU on the sequence plus one base that starts a new
            # run, and only what lies inside the original sequence is kept.
            if self._mode == HashMode.Hpc:
                self._j = self._jend = self._h = np.empty(0, dtype=np.uint32)
                self._i = 0
                return
            a = np.concatenate((a, np.array([ord("C") if a[-1] == ord("A") else ord("A")], dtype=np.uint8)))
            keep = l
        r = eng.extract_reads([a], l, 1, d, self._mode, want_minimizers=True)
        assert r["counts"]["hash_bound"] == int(hash_bound)
        self._j, self._jend, self._h = r["mn_j"], r["mn_jend"], r["mn_hash"]
        if keep is not None:  # the l-mer that starts at 0 and ends inside the original sequence
            m = (self._j == 0) & (self._jend < keep)
            self._j, self._jend, self._h = self._j[m], self._jend[m], self._h[m]
        self._i = 0

    @classmethod
    def new(cls, seq, l, hash_bound, engine=None):
        return cls(seq, l, hash_bound, engine)

    def __iter__(self):
        return self

    def __len__(self):
        return len(self._h) - self._i

    def _item(self, i):
        return int(self._j[i]), int(self._jend[i]), int(self._h[i])

    def __next__(self):
        if self._i >= len(self._h):
            raise StopIteration
        self._i += 1
        return self._item(self._i - 1)


class NtHashHPCIterator(_MinimizerTriples):
    """src/nthash_hpc.rs:99-283: Item = (start, end, hash) in original space; `<=` against the bound; the last HPC l-mer of the
    sequence is never yielded (:265-267); end = last base of the l-mer's last run (:281)."""
    _mode = HashMode.Hpc


class NtHashHPCSIMDIterator(_MinimizerTriples):
    """src/nthash_hpc_simd.rs:17-68: Item = (start, end, hash); the result semantics of the AVX-512 path: strict `<` against a
    bound re-derived through f32, end = START of the last run (:64), the last l-mer kept, the final block of 16 lost when the
    number of l-mers is a multiple of 16."""
    _mode = HashMode.HpcSimd


class NtHashSIMDIterator(_MinimizerTriples):
    """src/nthash_avx512_32.rs:14-164: Item = (pos, hash) over the sequence as it is (no homopolymer compression)."""
    _mode = HashMode.Simd

    def _item(self, i):
        return int(self._j[i]), int(self._h[i])


class RegularMinimizers(_MinimizerTriples):
    """Not a type of the crate: the (j, jend, hash) triples that the Regular arm of KminmersIterator::next makes from the external
    nthash32::NtHashIterator (src/lib.rs:215-230), for symmetry with the three above."""
    _mode = HashMode.Regular


def _hpc_gpu(seq, engine, rle):
    eng = engine or default_engine()
    a = _as_u8(seq)
    n = len(a)
    dev = torch.device("cuda", eng.device)
    d_b = torch.from_numpy(a.copy()).to(dev) if n else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    d_ho = torch.zeros(2, dtype=torch.int64, device=dev)
    d_h = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
    d_p = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    r = eng.hpc_device(d_b.data_ptr(), d_off.data_ptr(), 1, n, d_ho.data_ptr(), d_h.data_ptr(), d_p.data_ptr(), max(n, 1), rle=rle)
    return d_h[:r].cpu().numpy().tobytes(), d_p[:r].cpu().numpy().astype(np.uint32)


def _no_sentinel(a, who):
    # hpc / encode_rle start from prev_char = '#' (src/hpc.rs:9,30): a '#' in the input is dropped or misplaces the next
    # run's position there.  The device op treats '#' as an ordinary byte, so such input is refused instead of answered differently.
    if len(a) and (a == 0x23).any():
        raise ValueError("%s: input contains '#', the reference's start sentinel (src/hpc.rs:9,30); not supported" % who)


def hpc(seq, engine=None):
    """Homopolymer-compressed string of one read (any equal characters collapse): src/hpc.rs:28-41, on the GPU.
    hpc("") == "#" as in the reference (the sentinel is flushed at the end, src/hpc.rs:39-40)."""
    a = _as_u8(seq)
    if len(a) == 0:
        return b"#"
    _no_sentinel(a, "hpc")
    return _hpc_gpu(a, engine, False)[0]


def encode_rle(seq, engine=None):
    """(compressed string, run-start positions) with the rule of src/hpc.rs:7-25: only runs of ACTGactgNn collapse
    (src/hpc.rs:14), every other character stays.  encode_rle("") == ("#", [0]) as in the reference."""
    a = _as_u8(seq)
    if len(a) == 0:
        return b"#", np.zeros(1, dtype=np.uint32)
    _no_sentinel(a, "encode_rle")
    return _hpc_gpu(a, engine, True)


def encode_rle_simd(seq, engine=None):
    """(compressed string, run-start positions) -- src/hpc.rs:44-147 (any equal bytes collapse) -- computed on the GPU."""
    return _hpc_gpu(seq, engine, False)
