"""CPU tier: every environment variable the shipped library reads is a documented knob (README.md, "Environment knobs") and is set by at
least one test -- a knob switches a call onto another kernel or host path, and a path no test selects can break unnoticed.

The names come from the string literals of the shipped libs2k.so, not from the sources: getenv() takes a literal, so what the compiler
kept is exactly what the build reads, and reads behind S2K_DEBUG_KNOBS / S2K_STREAM_BUILD (debug builds only) drop out by themselves.
A scan of the sources would have to follow every #if the way the preprocessor does."""
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
HERE = os.path.basename(__file__)


def _shipped_knobs():
    r = subprocess.run(["make", "-C", CSRC, "-j", "6", "libs2k.so"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    data = open(os.path.join(CSRC, "libs2k.so"), "rb").read()
    # whole NUL-terminated strings that are nothing but a name (what `strings | grep -E '^S2K_[A-Z0-9_]+$'` prints)
    return {m.group(1).decode() for m in re.finditer(rb"(?<![\x20-\x7e])(S2K_[A-Z0-9_]+)\x00", data)}


def _readme_knobs():
    text = open(os.path.join(ROOT, "README.md")).read()
    sec = text.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    names = set()
    for line in sec.splitlines():
        if line.startswith("| `"):
            names.update(re.findall(r"`(S2K_[A-Z0-9_]+)`", line.split("|")[1]))
    return names


def _set_in(text, name):
    """env["NAME"] = ..., os.environ["NAME"] = ..., dict(os.environ, NAME=...), {"NAME": ...}: a value is given to the variable"""
    n = re.escape(name)
    return bool(re.search(r"\[\s*[\"']%s[\"']\s*\]\s*=(?!=)|[(,]\s*%s\s*=(?!=)|[\"']%s[\"']\s*:" % (n, n, n), text))


def test_the_string_scan_sees_the_shipped_reads_and_only_those():
    names = _shipped_knobs()
    # read unconditionally by the shipped build: the scan must find them, or every check below passes on nothing
    for n in ("S2K_TRACE", "S2K_DESC_CHUNKS", "S2K_COPY_THREADS", "S2K_HPC_SINGLE_PASS"):
        assert n in names, (n, sorted(names))
    # read only under S2K_DEBUG_KNOBS / S2K_STREAM_BUILD / in s2k_extract's debug trace: absent from the shipped build
    for n in ("S2K_DEBUG_SKIP", "S2K_DEBUG_NOKM", "S2K_DEBUG_KM_LDS", "S2K_DEBUG_BLOCKS_PER_CU"):
        assert n not in names, n


def test_every_shipped_knob_is_documented_and_set_by_a_test():
    names = _shipped_knobs()
    documented = _readme_knobs()
    undocumented = sorted(names - documented)
    assert not undocumented, ("read by libs2k.so but missing from the README knob table", undocumented)
    tests_dir = os.path.join(ROOT, "tests")
    texts = {}
    for dirpath, _, files in os.walk(tests_dir):
        for f in files:
            if f.endswith(".py") and f != HERE:
                texts[os.path.relpath(os.path.join(dirpath, f), tests_dir)] = open(os.path.join(dirpath, f)).read()
    unset = sorted(n for n in names if not any(_set_in(t, n) for t in texts.values()))
    assert not unset, ("read by libs2k.so but set by no test", unset)


def test_the_set_detector():
    assert _set_in('env["S2K_X"] = "1"', "S2K_X") and _set_in("os.environ['S2K_X']='3'", "S2K_X")
    assert _set_in("dict(os.environ, S2K_X=isa)", "S2K_X") and _set_in('{"S2K_X": "0"}', "S2K_X")
    assert not _set_in('"""runs with S2K_X=1"""', "S2K_X") and not _set_in('env.pop("S2K_X", None)', "S2K_X")
    assert not _set_in('if env["S2K_X"] == "1":', "S2K_X") and not _set_in("S2K_XY=1", "S2K_X")
