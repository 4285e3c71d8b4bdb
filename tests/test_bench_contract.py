"""CPU tier: pieces of bench.py that need no GPU -- the id that ties `roofline.traffic` to the kernel sources it was measured on,
and the workloads the command line offers."""
import json
import os
import shutil
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_kernel_source_id_follows_the_device_sources(tmp_path, monkeypatch):
    a = bench.kernel_source_id()
    assert a == bench.kernel_source_id() and len(a) == 16
    # the same function over a copy of the tree in which one kernel source differs by one byte
    dst = tmp_path / "rust-seq2kminmers_amd" / "csrc"
    dst.mkdir(parents=True)
    src = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
    for f in os.listdir(src):
        if f.endswith((".hip", ".h")) or f == "Makefile":
            shutil.copy(os.path.join(src, f), dst / f)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.kernel_source_id() == a  # objects, libraries and listings do not count
    with open(dst / "s2k_tile_impl.h", "a") as f:
        f.write("\n")
    assert bench.kernel_source_id() != a


def test_committed_traffic_file_names_its_sources():
    tj = json.load(open(os.path.join(ROOT, "profiles", "traffic_latest.json")))
    assert tj["mode"] == "hpc" and tj["n_bases"] == 10_000_000_000
    assert isinstance(tj.get("kernel_source_id"), str) and len(tj["kernel_source_id"]) == 16  # bench.py compares it with the tree's
    assert 12e9 < tj["hbm_bytes_per_step"] < 30e9


def test_workloads_on_the_command_line(monkeypatch):
    for wl in ("c2", "ont", "hifi"):
        monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", wl, "--no-other-configs"])
        a = bench.parse_args()
        assert a.workload == wl and a.gpus == 1 and a.no_other_configs


def test_cpu_baselines_build_outside_a_checkout_this_user_cannot_write(tmp_path, monkeypatch):
    """bench.py's cpu_baseline leg compiles the -march=native oracle and the AVX-512 baseline on first use: in a checkout owned by
    another user they go to a private directory under the temporary directory, never into oracle/, and a shared one is refused"""
    import tempfile

    from oracle import s2k_oracle as so

    here = os.path.dirname(so.__file__)
    real_access = os.access
    monkeypatch.setattr(so.os, "access", lambda p, m, *a, **k: False if os.path.realpath(p) == os.path.realpath(here) else real_access(p, m, *a, **k))
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    plain = so.get()  # (the portable oracle: build() put it into oracle/)
    before = sorted(os.listdir(here))
    private = tmp_path / ("s2k_oracle_%d" % os.getuid())
    o = so.Oracle(native=True)
    assert os.path.dirname(o.lib._name) == str(private) and o.hash_bound(0.01) == plain.hash_bound(0.01)
    av = so.build_avx512()
    assert av is None or os.path.dirname(av) == str(private)
    assert sorted(os.listdir(here)) == before
    assert (private.stat().st_mode & 0o777) == 0o700
    private.chmod(0o777)
    with pytest.raises(RuntimeError, match="not a private directory"):
        so.Oracle(native=True)


def test_dump_outputs_exact_sampled_and_repeatable(tmp_path):
    """--dump-outputs on host tensors laid out as the device arrays are: every dumped value equals the output entry it names, the
    sample is fixed, and the largest dump the default cap allows stays within 64 MB"""
    import numpy as np
    import torch

    assert 7 * 8 * bench.DUMP_ITEMS + 4 * bench.DUMP_ITEMS + 8 * 128 <= 64_000_000  # seven float64 arrays, rev in float32, .npy headers
    rng = np.random.default_rng(5)
    n_reads, nk, cap = 400, 5000, 300
    km_off = np.concatenate(([0], np.sort(rng.integers(0, nk, n_reads - 1)), [nk])).astype(np.int64)
    h = rng.integers(0, 1 << 64, nk + 100, dtype=np.uint64)  # (+100: capacity beyond n_kminmers, as in bench.py)
    h[:3] = [0, (1 << 64) - 1, (1 << 63) + 1]
    st = rng.integers(0, 1 << 32, nk + 100, dtype=np.uint64).astype(np.uint32)
    en = rng.integers(0, 1 << 32, nk + 100, dtype=np.uint64).astype(np.uint32)
    rev = rng.integers(0, 2, nk + 100).astype(np.uint8)
    outs = {"km_off": torch.from_numpy(km_off), "hash": torch.from_numpy(h.view(np.int64)), "start": torch.from_numpy(st.view(np.int32)),
            "end": torch.from_numpy(en.view(np.int32)), "rev": torch.from_numpy(rev)}
    nbytes = bench.dump_outputs(str(tmp_path / "a"), outs, nk, cap=cap)
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(d) == ["end", "hash_hi", "hash_lo", "km_off", "kminmer_index", "read_index", "rev", "start"]
    assert sum(a.nbytes for a in d.values()) == nbytes and all(a.dtype in (np.float32, np.float64) for a in d.values())
    for idx, n in ((d["read_index"], n_reads + 1), (d["kminmer_index"], nk)):
        assert 0 < len(idx) <= cap and idx[0] == 0 and idx[-1] == n - 1 and (np.diff(idx) > 0).all()
    ri, ki = d["read_index"].astype(np.int64), d["kminmer_index"].astype(np.int64)
    assert (d["km_off"].astype(np.int64) == km_off[ri]).all()
    got_h = (d["hash_hi"].astype(np.uint64) << np.uint64(32)) | d["hash_lo"].astype(np.uint64)
    assert (got_h == h[ki]).all() and (d["start"] == st[ki]).all() and (d["end"] == en[ki]).all() and (d["rev"] == rev[ki]).all()
    bench.dump_outputs(str(tmp_path / "b"), outs, nk, cap=cap)
    for name, a in d.items():
        assert np.array_equal(np.load(tmp_path / "b" / (name + ".npy")), a), name
    bench.dump_outputs(str(tmp_path / "c"), outs, nk, cap=nk)  # fits: every entry, in order
    assert (np.load(tmp_path / "c" / "kminmer_index.npy") == np.arange(nk)).all()
    assert (np.load(tmp_path / "c" / "km_off.npy") == km_off).all()
