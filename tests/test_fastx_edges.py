"""The FASTA/FASTQ record splitter on the device (s2k_fastx_dev.hip) at its seams: 16 bytes per thread, 4096 bytes per block,
1024 blocks (4 MiB) per round of the scan over the blocks.  A plain byte-role reference (split_reference), a corpus whose lines
start one byte before, on and one byte after those seams, and the file driver with its batch cut falling on every byte of a
record.  The CPU tier proves corpus and reference against the host reader before a GPU sees them."""
import functools

import numpy as np
import pytest

from test_fastx import _collect, pkg

MIB4 = 4 << 20
INVALID_ARG, CAPACITY = 1, 7


# ---- the reference ------------------------------------------------------------------------------------------------------
def _lines(text):
    parts = text.split(b"\n")
    if parts[-1] == b"":  # the final newline ends the last line, it does not begin another
        parts.pop()
    return [p[:-1] if p.endswith(b"\r") else p for p in parts]


def split_reference(text, fastq):
    """The reads of `text`, or None where it is not strict FASTA / FASTQ.  Lines end in "\\n" or "\\r\\n".  FASTA: a line that
    starts with '>' opens a record, other lines append to it, blank lines are ignored.  FASTQ: groups of four lines, '@...',
    sequence, '+...', quality, and nothing but blank lines behind the last group."""
    lines = _lines(text)
    reads = []
    if not fastq:
        for ln in lines:
            if ln.startswith(b">"):
                reads.append([])
            elif ln:
                if not reads:
                    return None
                reads[-1].append(ln)
        return [b"".join(r) for r in reads]
    i = 0
    while i < len(lines):
        if lines[i] == b"":
            if any(lines[i:]):
                return None  # a blank line before or between records
            break
        if i + 4 > len(lines) or not lines[i].startswith(b"@") or not lines[i + 2].startswith(b"+"):
            return None
        reads.append(lines[i + 1])
        i += 4
    return reads


def test_split_reference_by_hand():
    assert split_reference(b">a\nAC\n\n>b\n\nGT\r\nT", False) == [b"AC", b"GTT"]
    assert split_reference(b"AC\n>a\n", False) is None
    assert split_reference(b"@a\nAC\n+\nII\n@b\n\n+b\n\n\n\n", True) == [b"AC", b""]
    assert split_reference(b"@a\r\nAC\r\n+\r\n@I", True) == [b"AC"]
    for bad in (b"@a\nAC\n+\n", b"@a\nAC\n", b"@a\n", b"@a\nAC\nII\n@b\nA\n+\nI\n", b"\n@a\nAC\n+\nII\n", b"@a\nAC\n+\nII\n\n@b\nA\n+\nI\n",
                b"@a\n\n+\n", b"@a\nAC\n+\nII\n\n\n\n\n@b\nA\n+\nI\n"):
        assert split_reference(bad, True) is None, bad
    assert split_reference(b"", True) == [] and split_reference(b"\n\n", True) == [] and split_reference(b"", False) == []


# ---- the corpus -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool():
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(41).integers(0, 4, size=1 << 22)].tobytes()


class _Text:
    """A FASTA or FASTQ text under construction.  place(p, kind) pads the header of a record of its own so that the first byte
    of a line of the asked kind lands on byte p.  Headers carry '>', '@' and '+', FASTA sequence lines carry them away from the
    line start, qualities begin with '@', '+' and '>', and every third '+' line carries a name."""

    KINDS = {False: ("header", "sequence", "continuation", "blank"), True: ("header", "sequence", "plus", "quality")}

    def __init__(self, fastq, crlf=False):
        self.fastq, self.nl = fastq, b"\r\n" if crlf else b"\n"
        self.parts, self.n, self.k, self.placed = [], 0, 0, []

    def add(self, b):
        self.parts.append(b)
        self.n += len(b)

    def _seq(self, n):
        a = (self.k * 7919) % ((1 << 22) - n)
        return _pool()[a:a + n]

    def _record_lines(self, seqlen, pad=0):
        """the lines of one record, without their terminators"""
        self.k += 1
        k, s = self.k, self._seq(seqlen)
        if self.fastq:
            q = (b"@+>"[k % 3:k % 3 + 1] + b"I@+>" * seqlen)[:seqlen]
            return [b"@r%d >@+ x" % k + b"x" * pad, s, b"+r%d" % k if k % 3 == 0 else b"+", q]
        if seqlen >= 8:  # '>', '@' and '+' inside sequence lines, away from the line start
            s = s[:3] + b">@+" + s[6:]
        a, b = seqlen // 3, 2 * seqlen // 3
        return [b">r%d >@+ x" % k + b"x" * pad, s[:a], s[a:b], b"", s[b:]]

    def record(self, seqlen, pad=0):
        self.add(self.nl.join(self._record_lines(seqlen, pad)) + self.nl)

    def fill_to(self, p, margin=30000):
        """whole records up to a little before byte p"""
        while self.n < p - margin:
            self.record(min(20000, max(1, (p - margin - self.n) // 3)))

    def place(self, p, kind, seqlen=40):
        """a padded record, then a record whose line `kind` (index into KINDS) begins on byte p"""
        filler = self._record_lines(seqlen)
        target = self._record_lines(seqlen)
        if not self.fastq and kind == 3:
            pre = target[:3]
        else:
            pre = target[:kind]
        fixed = sum(len(x) + len(self.nl) for x in filler + pre)
        pad = p - self.n - fixed
        assert pad >= 0, (p, self.n, fixed)
        filler[0] += b"x" * pad
        self.add(self.nl.join(filler + pre) + self.nl)
        assert self.n == p
        self.placed.append((p, self.KINDS[self.fastq][kind]))
        self.add(self.nl.join(target[len(pre):]) + self.nl)

    def place_empty(self, p):
        """a record without sequence on byte p: FASTQ its (empty) sequence line, FASTA its header, the next header right behind"""
        filler = self._record_lines(40)
        pre = [b"@e"] if self.fastq else []
        pad = p - self.n - sum(len(x) + len(self.nl) for x in filler + pre)
        assert pad >= 0
        filler[0] += b"x" * pad
        self.add(self.nl.join(filler + pre) + self.nl)
        assert self.n == p
        self.placed.append((p, "empty sequence"))
        self.add(self.nl + b"+" + self.nl + self.nl if self.fastq else b">e" + self.nl)

    def end_at(self, length, final_newline=True):
        """a last record whose header is padded so that the text has exactly `length` bytes"""
        lines = self._record_lines(40)
        pad = length - self.n - sum(len(x) + len(self.nl) for x in lines) + (0 if final_newline else len(self.nl))
        assert pad >= 0
        lines[0] += b"x" * pad
        self.add(self.nl.join(lines) + (self.nl if final_newline else b""))
        assert self.n == length
        return self

    def bytes(self):
        return b"".join(self.parts)


def _next_seam(n, t, need):
    return ((n + need + t - 1) // t) * t


def _placed_small(fastq, t, crlf=False):
    """every kind of line one byte before, on and one byte after a multiple of t (the seams of one size are all alike)"""
    tx = _Text(fastq, crlf)
    tx.record(40)
    for kind in range(4):
        for delta in (-1, 0, 1):
            tx.place(_next_seam(tx.n, t, 400) + delta, kind)
    for delta in (-1, 0, 1):
        tx.place_empty(_next_seam(tx.n, t, 400) + delta)
    tx.record(40)
    return tx


def _placed_big(fastq, delta):
    """the four kinds at 4, 8, 12 and 16 MiB + delta (where the scan over the blocks begins another round: nb 1024 -> 1025), and
    4096 bytes behind each of them two kinds on; more than 3 x 4 MiB, so the line index mod 4 is carried across rounds"""
    tx = _Text(fastq)
    for i in range(4):
        s = (i + 1) * MIB4
        tx.fill_to(s + delta)
        tx.place(s + delta, i)
        tx.place(s + 4096 + delta, (i + 2) % 4)
        tx.place_empty(s + 8192 + delta)
    tx.record(40)
    return tx


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, fastq, text)], well-formed throughout"""
    out = []
    for fastq in (False, True):
        f = "fq" if fastq else "fa"
        for t in (16, 4096, 8192):
            out.append(("%s placed %d" % (f, t), fastq, _placed_small(fastq, t).bytes()))
        out.append(("%s crlf placed 16" % f, fastq, _placed_small(fastq, 16, crlf=True).bytes()))
        out.append(("%s crlf placed 4096" % f, fastq, _placed_small(fastq, 4096, crlf=True).bytes()))
        for delta in (-1, 0, 1):
            out.append(("%s placed 4 MiB %+d" % (f, delta), fastq, _placed_big(fastq, delta).bytes()))
        # headers longer than one and than two blocks
        tx = _Text(fastq)
        tx.record(40)
        tx.record(40, pad=5000)
        tx.record(40, pad=9000)
        tx.record(40)
        out.append(("%s long headers" % f, fastq, tx.bytes()))
        # a header that lies across 4 MiB
        tx = _Text(fastq)
        tx.fill_to(MIB4 - 3000, margin=2000)
        assert MIB4 - 6000 < tx.n < MIB4 - 3000
        tx.record(40, pad=7000)
        tx.record(40)
        out.append(("%s header across 4 MiB" % f, fastq, tx.bytes()))
        # lengths: the residues mod 16, one block and one round of the block scan exactly and one byte more; with and without
        # a final newline
        for length in (1024, 1025, 1039, 4096, 4097, MIB4, MIB4 + 1):
            for final in (True, False):
                if length >= MIB4 and final == ((length == MIB4) != fastq):  # the 4 MiB texts: one ending per format and length
                    continue
                tx = _Text(fastq)
                tx.fill_to(length, margin=min(30000, length // 2))
                out.append(("%s length %d%s" % (f, length, "" if final else " no final newline"), fastq, tx.end_at(length, final).bytes()))
    # empty records alone, trailing blank lines, empty text
    out.append(("fq empty records", True, b"@a\n\n+\n\n@b\n\n+b\n\n@c\nA\n+\n@\n"))
    out.append(("fq trailing blank lines", True, b"@a\nAC\n+\n@I\n\n\n\n\n\n"))
    out.append(("fq trailing blank lines crlf", True, b"@a\r\nAC\r\n+\r\n@I\r\n\r\n\r\n\r\n"))
    out.append(("fq empty", True, b""))
    out.append(("fq blank only", True, b"\n\n\n"))
    out.append(("fa empty records", False, b">a\n>b\n\n>c\nA\n>d"))
    out.append(("fa empty", False, b""))
    names = [n for n, _, _ in out]
    assert len(set(names)) == len(names)
    return out


# malformed FASTQ the device has to refuse (name, text, what the host reader does: None = it refuses too, else the reads it
# returns).  The host reader skips blank lines before and between records: that is its documented behaviour (s2k_fastx_open,
# s2k_fastx_next), the device is strict; the difference is pinned here and not a defect of either.
MALFORMED_FASTQ = [
    ("missing +", b"@r1\nACGT\nIIII\n@r2\nAC\n+\nII\n", None),
    ("ends after the header", b"@r0\nAC\n+\nII\n@r1\n", None),
    ("ends after the header, no newline", b"@r1", None),
    ("ends after the sequence", b"@r1\nACGT\n", None),
    ("ends after the sequence, no newline", b"@r0\nAC\n+\nII\n@r1\nACGT", None),
    ("ends after +", b"@r1\nACGT\n+\n", None),
    ("ends after +, no newline", b"@r1\nACGT\n+", None),
    ("ends after + of an empty read", b"@r0\nAC\n+\nII\n@r1\n\n+\n", None),
    ("blank + line", b"@r1\nACGT\n\nIIII\n@r2\nAC\n+\nII\n", None),
    ("blank between", b"@r1\nACGT\n+\nIIII\n\n@r2\nAC\n+\nII\n", [b"ACGT", b"AC"]),
    ("four blank between", b"@r1\nACGT\n+\nIIII\n\n\n\n\n@r2\nAC\n+\nII\n", [b"ACGT", b"AC"]),
    ("blank between empty reads", b"@a\n\n+\n\n\n@b\n\n+\n\n", [b"", b""]),
    ("blank before the first", b"\n@r1\nACGT\n+\nIIII\n", [b"ACGT"]),
    ("four blank before the first", b"\n\n\n\n@r1\nACGT\n+\nIIII\n", [b"ACGT"]),
    ("crlf blank before the first", b"\r\n@r1\r\nACGT\r\n+\r\nIIII\r\n", [b"ACGT"]),
]


def _truncated_at_seams():
    """truncations whose last line lies on a thread and on a block seam"""
    out = []
    for t in (16, 4096):
        for cut in (1, 2, 3):
            tx = _Text(True)
            tx.record(40)
            tx.place(_next_seam(tx.n, t, 400), cut)  # the line after the cut would begin on the seam
            text = tx.bytes()
            out.append(("truncated %d lines at %d" % (cut, t), text[:tx.placed[0][0]], None))
    return out


def _host_reads(tmp_path, text):
    p = tmp_path / "t.fx"
    p.write_bytes(text)
    return _collect(p, 1 << 30)[0]


def test_corpus_places_lines_on_the_seams():
    """the builder's own claim, checked on the bytes: a line of the kind begins on the byte"""
    seen = set()
    for fastq in (False, True):
        for tx in [_placed_small(fastq, t) for t in (16, 4096, 8192)] + [_placed_big(fastq, d) for d in (-1, 0, 1)]:
            text = tx.bytes()
            for p, kind in tx.placed:
                assert text[p - 1:p] == b"\n"
                want = {"header": b"@" if fastq else b">", "plus": b"+", "blank": b"\n", "empty sequence": b"\n" if fastq else b">"}.get(kind)
                assert want is None or text[p:p + 1] == want, (p, kind)
                for t in (16, 4096, 8192, MIB4):
                    for delta in (-1, 0, 1):
                        if (p - delta) % t == 0:
                            seen.add((fastq, t, delta, kind))
    for fastq in (False, True):
        for kind in _Text.KINDS[fastq] + ("empty sequence",):
            for t in (16, 4096, 8192, MIB4):
                for delta in (-1, 0, 1):
                    if t == MIB4 and kind == "empty sequence":  # (those lie 8192 bytes behind the 4 MiB seams)
                        continue
                    assert (fastq, t, delta, kind) in seen, (fastq, t, delta, kind)


def test_corpus_reference_equals_host_reader(tmp_path):
    for name, fastq, text in corpus():
        ref = split_reference(text, fastq)
        assert ref is not None, name
        assert _host_reads(tmp_path, text) == ref, name
    assert sum(len(t) >= 3 * MIB4 for _, fq, t in corpus() if fq) >= 1


def test_malformed_fastq_reference_and_host_reader(tmp_path):
    for name, text, host in MALFORMED_FASTQ + _truncated_at_seams():
        assert split_reference(text, True) is None, name
        if host is None:
            with pytest.raises(pkg.S2kError):
                _host_reads(tmp_path, text)
        else:  # blank lines before / between records: the host reader is tolerant by its documentation
            assert _host_reads(tmp_path, text) == host, name


# ---- the device ---------------------------------------------------------------------------------------------------------
MARK8, MARK64 = 0xA5, 0x5A5A5A5A5A5A5A5A


def _to_device(text):
    import torch

    if not len(text):
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()


def _device_split(eng, t, n, fastq, ref, name):
    """sizes-only call, then exact capacities with guard bands behind both arrays; everything against `ref`"""
    import torch

    want_off = np.zeros(len(ref) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in ref], out=want_off[1:])
    nr, nb = len(ref), int(want_off[-1])
    st, gr, gb = eng.parse_fastx_device(t.data_ptr(), n, fastq)
    assert (gr, gb) == (nr, nb), (name, "sizes only", gr, gb, nr, nb)
    assert st == CAPACITY, (name, st)  # no output buffers given: sizes only
    d_b = torch.full((nb + 64,), MARK8, dtype=torch.uint8, device="cuda")
    d_o = torch.full((nr + 1 + 8,), MARK64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st, gr, gb = eng.parse_fastx_device(t.data_ptr(), n, fastq, d_b.data_ptr(), nb, d_o.data_ptr(), nr + 1)
    assert (st, gr, gb) == (0, nr, nb), (name, st, gr, gb)
    b, o = d_b.cpu().numpy(), d_o.cpu().numpy()
    assert (b[nb:] == MARK8).all() and (o[nr + 1:] == MARK64).all(), (name, "guard bands")
    if not (o[:nr + 1] == want_off).all():
        bad = int(np.nonzero(o[:nr + 1] != want_off)[0][0])
        raise AssertionError((name, "read_off", bad, int(o[bad]), int(want_off[bad])))
    want_b = np.frombuffer(b"".join(ref), dtype=np.uint8)
    if not (b[:nb] == want_b).all():
        bad = int(np.nonzero(b[:nb] != want_b)[0][0])
        raise AssertionError((name, "bases", bad, int(b[bad]), int(want_b[bad])))
    return d_b, d_o


@pytest.mark.gpu
def test_gpu_split_equals_reference_on_the_corpus():
    eng = pkg.Engine(0)
    for name, fastq, text in corpus():
        _device_split(eng, _to_device(text), len(text), fastq, split_reference(text, fastq), name)
    eng.close()


@pytest.mark.gpu
def test_gpu_split_capacity_contract_and_alignment():
    import torch

    eng = pkg.Engine(0)
    for name, fastq, text in corpus():
        if name.split(" ", 1)[1] not in ("placed 4096", "long headers", "length 4097"):
            continue
        ref = split_reference(text, fastq)
        nr, nb = len(ref), sum(len(r) for r in ref)
        t = _to_device(text)
        for bcap, ocap in ((nb - 1, nr + 1), (nb, nr), (nb - 1, nr)):
            d_b = torch.full((nb + 64,), MARK8, dtype=torch.uint8, device="cuda")
            d_o = torch.full((nr + 1 + 8,), MARK64, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            st, gr, gb = eng.parse_fastx_device(t.data_ptr(), len(text), fastq, d_b.data_ptr(), bcap, d_o.data_ptr(), ocap)
            assert (st, gr, gb) == (CAPACITY, nr, nb), (name, bcap, ocap, st, gr, gb)
            assert (d_b.cpu().numpy()[bcap:] == MARK8).all() and (d_o.cpu().numpy()[ocap:] == MARK64).all(), (name, bcap, ocap)
        # the text has to be 16-byte aligned
        t8 = torch.zeros(len(text) + 16, dtype=torch.uint8, device="cuda")
        t8[8:8 + len(text)] = t
        assert t8.data_ptr() % 16 == 0
        with pytest.raises(pkg.S2kError) as e:
            eng.parse_fastx_device(t8.data_ptr() + 8, len(text), fastq)
        assert e.value.status == INVALID_ARG
    eng.close()


@pytest.mark.gpu
def test_gpu_split_refuses_malformed_fastq():
    """never S2K_OK with reads that are not the reference's: what the reference refuses, the device refuses"""
    eng = pkg.Engine(0)
    for name, text, _ in MALFORMED_FASTQ + _truncated_at_seams():
        assert split_reference(text, True) is None
        t = _to_device(text)
        with pytest.raises(pkg.S2kError) as e:
            eng.parse_fastx_device(t.data_ptr(), len(text), True)
        assert e.value.status == INVALID_ARG, name
    eng.close()


# ---- the file driver with its batch cut on every byte of a record -------------------------------------------------------------
L, K, D = 31, 7, 1.0  # as test_fastx.py's low-complexity case: at density 1 reads of a few dozen bases have k-min-mers
BATCH = 1 << 18       # -> a chunk of the 1 MiB minimum: the first cut is asked for at byte 1 048 576
CUT = 1 << 20


def _sweep_files(fastq):
    """(reads, number of files, file text for the i-th padding of the first header): about 2.5 MiB of short records; over the
    paddings the cut request falls on every byte of a record"""
    rng = np.random.default_rng(43 + fastq)
    lens = rng.integers(30, 61, size=26000) if fastq else rng.integers(70, 131, size=24000)
    pool = _pool()
    reads = [pool[a:a + n] for a, n in zip(rng.integers(0, (1 << 22) - 200, size=len(lens)).tolist(), lens.tolist())]
    recs = []
    for i, r in enumerate(reads):
        if fastq:
            recs.append(b"@r%d\n%s\n+\n%s\n" % (i, r, (b"@I" * len(r))[:len(r)]))
        else:
            recs.append(b">r%d >x\n%s\n" % (i, b"\n".join(r[j:j + 61] for j in range(0, len(r), 61))))
    first, rest = recs[0], b"".join(recs[1:])
    assert 5 * CUT // 2 - (1 << 17) < len(first) + len(rest) < 3 * CUT
    # the record that holds byte CUT without padding, and the one before it: sweep over the longer of the two, and two more
    ends = np.cumsum([len(x) for x in recs])
    at = int(np.searchsorted(ends, CUT, side="right"))
    span = max(len(recs[at]), len(recs[at - 1])) + 2
    nl = first.index(b"\n")
    assert 70 < span < 160
    return reads, span, lambda pad: first[:nl] + b"x" * pad + first[nl:] + rest


@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta61"])
def test_sweep_files_hold_the_reads_and_move_the_cut_across_a_record(fastq):
    reads, n_files, text = _sweep_files(fastq)
    marks = set()
    for pad in (0, n_files // 2, n_files - 1):
        t = text(pad)
        assert split_reference(t, fastq) == reads
    for pad in range(n_files):  # where in its line, and in which line of the record, byte CUT lies
        t = text(pad)[CUT - 200:CUT + 1]
        marks.add((t.count(b"\n", t.rindex(b"@r" if fastq else b">r")), CUT - 200 + t.rindex(b"\n") + 1 == CUT))
    assert {m for m in marks if m[1]} >= {(k, True) for k in ((1, 2, 3) if fastq else (1, 2))}, marks


def _oracle_totals(oracle, reads):
    from oracle import s2k_oracle as so

    bases, off = pkg.pack_reads(reads)
    ref = oracle.batch(bases, off, L, K, D, so.REGULAR, threads=8)
    u, c = np.unique(ref["hash"], return_counts=True)
    return (len(reads), len(bases), ref["n"], int(np.bitwise_xor.reduce(ref["hash"]))), dict(zip(u.tolist(), c.tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta61"])
def test_run_file_cut_on_every_byte_of_a_record(tmp_path, oracle, fastq):
    reads, n_files, text = _sweep_files(fastq)
    want, want_counts = _oracle_totals(oracle, reads)
    assert want[2] > 100000 and len(want_counts) < want[2]
    eng = pkg.Engine(0)
    p = tmp_path / ("s.fq" if fastq else "s.fa")
    for i in range(n_files):
        p.write_bytes(text(i))
        tot = eng.run_file(str(p), L, K, D, pkg.HashMode.Regular, batch_bases=BATCH)
        assert (tot["n_reads"], tot["n_bases"], tot["n_kminmers"], tot["xor_hash"]) == want, ("padding", i)
        if i in (0, n_files // 2, n_files - 1):
            r = eng.run_file_count(str(p), L, K, D, pkg.HashMode.Regular, min_count=1, batch_bases=BATCH)
            got = dict(zip(r["keys"].cpu().numpy().view(np.uint64).tolist(), r["counts"].cpu().numpy().tolist()))
            assert got == want_counts, ("padding", i)
            assert (r["n_reads"], r["n_bases"], r["n_kminmers"], r["xor_hash"]) == want
    eng.close()


@pytest.mark.gpu
def test_run_file_never_ok_with_other_totals_than_the_host_reader(tmp_path):
    """truncated FASTQ and FASTQ with blank lines before the first record through the file driver: an error, or the host reader's
    reads -- never S2K_OK with something else"""
    eng = pkg.Engine(0)
    big = _Text(True)
    big.fill_to(3 * CUT, margin=1000)
    cases = [(n, t) for n, t, _ in MALFORMED_FASTQ + _truncated_at_seams() if n.startswith(("ends", "truncated")) or "before" in n]
    cases.append(("2.9 MiB ending after a sequence line", big.bytes() + b"@last\nACGT\n"))
    cases.append(("blank lines, then 2.9 MiB", b"\n\n" + big.bytes()))
    assert len(cases) >= 14
    for name, text in cases:
        p = tmp_path / "m.fq"
        p.write_bytes(text)
        try:
            host = _collect(p, 1 << 30)[0]
        except pkg.S2kError:
            host = None
        try:
            tot = eng.run_file(str(p), L, K, D, pkg.HashMode.Regular, batch_bases=BATCH)
        except pkg.S2kError as e:
            assert e.status == INVALID_ARG, name
            tot = None
        if host is None:
            assert tot is None, (name, "the host reader refuses this file", tot)
        elif tot is not None:
            assert (tot["n_reads"], tot["n_bases"]) == (len(host), sum(len(r) for r in host)), name
        if name.startswith(("ends", "truncated", "2.9 MiB ending")):
            assert host is None and tot is None, name
    eng.close()
