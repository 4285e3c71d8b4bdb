"""CPU tier: the LDS waits of the static hash loop in the ISA hipcc really emitted (cross-compiled for gfx950, no GPU needed).

The loop fetches a group's seed pairs LA positions before it uses them; that hides the LDS round trip only if the wait in front of
a group's first consumer is a counted `s_waitcnt lgkmcnt(n)`.  tools/isa/check_lgkmcnt.py replays the loop's LDS queue on the ISA and
refuses both a wait that drains look-ups still in flight and a consumer that runs ahead of its wait."""
import importlib.util
import os
import subprocess
import sys

from conftest import ROOT

CSRC = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "isa", "check_lgkmcnt.py")


def _tool():
    spec = importlib.util.spec_from_file_location("check_lgkmcnt", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _make(target):
    r = subprocess.run(["make", "-C", CSRC, "-j", "2", target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return os.path.join(CSRC, target)


def _run(path):
    return subprocess.run([sys.executable, TOOL, path], capture_output=True, text=True, timeout=300)


def test_hash_loop_waits_are_counted_in_the_shipped_kernels():
    r = _run(_make("isa/s2k_tile_L31.s"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    rows = [ln for ln in r.stdout.split("\n") if "hash loop" in ln]
    # four instantiations per family: {descriptor, legacy} x {compiled-in mode, run-time mode}
    assert len([x for x in rows if "hpc=1" in x]) == 4 and len([x for x in rows if "hpc=0" in x]) == 4, r.stdout
    for x in rows:
        assert " 0 drain look-ups in flight" in x, x
        assert " 1 lgkmcnt(0)" in x, x  # the last group's and no other


def test_the_flat_load_of_rounds_1_to_9_is_refused():
    """-DS2K_PREVB_FLAT=1: the byte before the next tile by flat_load, in flight across the hash loop.  The Hpc kernels' waits are
    lgkmcnt(0) then, every one; the Regular kernels have no such load and stay as they are."""
    r = _run(_make("isa/s2k_tile_L31_prevb_flat.s"))
    assert r.returncode != 0, r.stdout[-2000:]
    assert "drains" in r.stderr and "hpc=1" in r.stderr, r.stderr[-2000:]
    assert "hpc=0" not in r.stderr, r.stderr[-2000:]
    rows = [ln for ln in r.stdout.split("\n") if "hash loop" in ln and "hpc=1" in ln]
    assert len(rows) == 4 and all(" 0 counted" in x for x in rows), r.stdout


LOOP = """\
ds_read_b64 v[10:11], v1
ds_read_b64 v[12:13], v2
%s
v_xor_b32_e32 v20, v10, v20
ds_read_b64 v[14:15], v3
ds_read_b64 v[16:17], v4
%s
v_xor_b32_e32 v20, v12, v20
"""


def _region(text):
    return [(i + 1, s) for i, s in enumerate(text.strip().split("\n"))]


def test_checker_rules_on_hand_made_loops():
    t = _tool()
    ok, _ = t.check_region(_region(LOOP % ("s_waitcnt lgkmcnt(1)", "s_waitcnt lgkmcnt(2)")), "ok")
    assert ok == []
    drained, _ = t.check_region(_region(LOOP % ("s_waitcnt lgkmcnt(1)", "s_waitcnt lgkmcnt(0)")), "drained")
    assert len(drained) == 1 and "drains 2" in drained[0], drained
    early, _ = t.check_region(_region(LOOP % ("s_waitcnt lgkmcnt(1)", "s_waitcnt lgkmcnt(3)")), "early")
    assert len(early) == 1 and "touches v12" in early[0], early
    # operations without a result count too: the store behind the read lets lgkmcnt(1) retire the read
    st, _ = t.check_region(_region("ds_read_b64 v[10:11], v1\nds_write_b32 v5, v6\ns_waitcnt lgkmcnt(1)\nv_mov_b32_e32 v7, v10"), "store")
    assert st == []
    # a scalar load returns out of order on the same counter
    sm, _ = t.check_region(_region("ds_read_b64 v[10:11], v1\ns_load_dword s4, s[0:1], 0x0\ns_waitcnt lgkmcnt(0)\nv_mov_b32_e32 v7, v10"), "smem")
    assert len(sm) == 1 and "s_load_dword" in sm[0], sm
    # a block entered by a branch: what was in flight before it needs an lgkmcnt(0)
    br = "ds_read_b64 v[10:11], v1\ns_cbranch_scc1 .LBB0_9\n.LBB0_9:\n%sv_mov_b32_e32 v7, v10"
    bad, _ = t.check_region(_region(br % ""), "label")
    assert len(bad) == 1 and "touches v10" in bad[0], bad
    good, _ = t.check_region(_region(br % "s_waitcnt lgkmcnt(0)\n"), "label")
    assert good == []
