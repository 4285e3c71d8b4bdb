"""CPU tier: the scalar budget of the flagship tiled kernel, tile_minimizer_kernel<31, Hpc, descriptor path, TILE_MODE_HPC>, in the ISA
hipcc emits for gfx950 (no GPU needed).

Before the mode was compiled in and the cold arguments were moved behind the kernarg pointer, the kernel held 106 SGPRs and spilled 76 of
them to VGPR lanes: 76 v_writelane_b32 and 150 v_readlane_b32 in the body, 191 s_nop.  Spills to lanes are vector instructions that take
issue turns in a kernel bound by instruction issue."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
FLAGSHIP = "tile_minimizer_kernelILi31ELb1ELb1ELi2E"  # <L = 31, HPC, DESC, TILE_MODE_HPC>


def _isa():
    r = subprocess.run(["make", "-C", CSRC, "isa/s2k_tile_L31.s"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return open(os.path.join(CSRC, "isa", "s2k_tile_L31.s")).read()


def _body(text, name):
    m = re.search(r"^(_Z\S*%s\S*):" % name, text, re.M)
    assert m, "%s not in the ISA" % name
    end = text.index(".Lfunc_end", m.end())
    ins = [ln.split(";")[0].strip() for ln in text[m.end():end].splitlines()]
    return m.group(1), [i.split()[0] for i in ins if i and not i.startswith(".") and not i.endswith(":")]


def _meta(text, sym):
    i = text.index(".name:           " + sym)
    start = text.rindex("  - .agpr_count:", 0, i)
    return text[start:text.find("\n  - ", i) if text.find("\n  - ", i) > 0 else len(text)]


def test_flagship_tile_kernel_spills_no_sgprs():
    text = _isa()
    sym, ins = _body(text, FLAGSHIP)
    meta = _meta(text, sym)
    spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", meta).group(1))
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    assert spills == 0, spills
    assert vgprs <= 128, vgprs  # the k-min-mer kernel's waves run beside it (test_isa_invariants.py)
    # no lane spills left: what remains of v_writelane is what DPP / broadcast code needs (none today)
    assert ins.count("v_writelane_b32") <= 8, ins.count("v_writelane_b32")
    assert ins.count("v_readlane_b32") <= 40, ins.count("v_readlane_b32")  # (broadcasts of lane 63 / a computed lane, was 150)
    assert ins.count("s_nop") <= 175, ins.count("s_nop")  # 191 before; most of the rest sit in the hash loop and around M0


def test_cold_arguments_are_the_first_kernel_argument():
    """The kernel reads TileCold through __builtin_amdgcn_kernarg_segment_ptr(), i.e. at offset 0 of the kernarg segment."""
    text = _isa()
    for m in re.finditer(r"^(_Z\S*tile_minimizer_kernel\S*):", text, re.M):
        meta = _meta(text, m.group(1))
        assert "NS0_8TileColdE" in m.group(1).split("EEEv")[1][:20], m.group(1)
        first = re.search(r"\.args:\s*\n\s*- \.offset:\s+(\d+)\n\s*\.size:\s+(\d+)\n\s*\.value_kind:\s+(\S+)", meta)
        assert first and first.group(1) == "0" and first.group(3) == "by_value", (m.group(1), first and first.groups())


def test_fixed_modes_are_instantiated_beside_the_run_time_one():
    text = _isa()
    for tag in ("ILi31ELb1ELb1ELi2E", "ILi31ELb1ELb1ELi0E", "ILi31ELb0ELb1ELi1E", "ILi31ELb0ELb1ELi0E",
                "ILi31ELb1ELb0ELi2E", "ILi31ELb1ELb0ELi0E", "ILi31ELb0ELb0ELi1E", "ILi31ELb0ELb0ELi0E"):
        assert re.search(r"^_Z\S*tile_minimizer_kernel%s\S*:" % tag, text, re.M), tag
