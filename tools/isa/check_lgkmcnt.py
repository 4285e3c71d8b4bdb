#!/usr/bin/env python3
"""Checks the LDS waits of the static hash loop against the ISA the compiler emitted.

The hash loop fetches the seed pairs of a group of positions LA steps before it uses them (hash_steps, s2k_tile_impl.h): the LDS
round trip of a look-up is meant to pass under the arithmetic of the positions in between.  That only happens if the wait in front
of a group's first consumer is a COUNTED one, `s_waitcnt lgkmcnt(n)` with n = LDS operations issued behind that group: a wave's LDS
operations complete in order, so the newest n may stay in flight.  With lgkmcnt(0) the wave drains the look-ups it has just issued,
once per group, and the look-ahead exists in the source only (rounds 1-9 of the Hpc kernel: a flat_load left in flight across the
loop made the compiler take lgkmcnt for out of order).

Between the `; S2K_MARK hash_begin` and `; S2K_MARK hash_end` comments of every tile_minimizer_kernel instantiation this script
replays the wave's LDS queue in program order -- every ds_ instruction enters it, a ds_read with its destination registers -- and
checks, for the fall-through path that all positions of a full tile take:
  * no instruction touches the destination of a look-up that a wait has not yet retired (a too-large count: wrong hashes);
  * every wait retires no more than its consumer, the first instruction behind it that touches an LDS read in flight, needs
    (a too-small count: the drain described above);
  * nothing but LDS traffic counts in lgkmcnt inside the loop (a scalar load would make the counter out of order).
Blocks that are entered by a branch (the exits of a tile of fewer than nine pieces) start from an unknown queue: there only the
first rule is checked, against everything that was in flight at any point before.

usage: check_lgkmcnt.py [--expect-hpc-la N] <kernel.s> [...]   (isa/s2k_tile_L31.s of `make -C rust-seq2kminmers_amd/csrc isa/s2k_tile_L31.s`)
Validated against: ROCm 7.2.0 (hipcc / AMD clang of /opt/rocm-7.2.0), gfx950."""
import re
import sys

VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
WAIT = re.compile(r"^s_waitcnt\b(.*)$")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")
LABEL = re.compile(r"^\.LBB\d+_\d+:")
OTHER_LGKM = re.compile(r"^(s_load|s_buffer_load|s_memtime|s_memrealtime|s_sendmsg|s_scratch_load|flat_)")


def vregs(text):
    out = set()
    for m in VREG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def split_ops(s):
    """mnemonic, list of operand strings (modifiers such as offset:N stay with the last operand: they name no register)"""
    parts = s.split(None, 1)
    return parts[0], ([o.strip() for o in parts[1].split(",")] if len(parts) > 1 else [])


def check_region(lines, tag):
    """lines: the instructions between the marks (comments and directives dropped).  Returns (errors, statistics)."""
    errors = []
    queue = []       # LDS operations in flight, oldest first: [line number, set of destination registers]
    stale = set()    # after a label: registers that were in flight on some path into the block
    known = True     # False after a label until an lgkmcnt(0)
    waits = []       # (line number, n, needed) of the fall-through path
    insts = [(no, s) for no, s in lines]
    for idx, (no, s) in enumerate(insts):
        if LABEL.match(s):
            for _, regs in queue:
                stale |= regs
            queue, known = [], False
            continue
        m = WAIT.match(s)
        if m:
            g = LGKM.search(m.group(1))
            if not g:
                continue  # vmcnt / expcnt only
            n = int(g.group(1))
            if known:
                # the first instruction behind the wait that touches the queue as it stands is the one the wait is for
                need = -1
                for no2, s2 in insts[idx + 1:]:
                    if LABEL.match(s2) or (WAIT.match(s2) and LGKM.search(s2)) or s2.startswith(("s_branch", "s_cbranch", "s_endpgm")):
                        break
                    t = vregs(s2)
                    for qi, (_, regs) in enumerate(queue):
                        if regs & t:
                            need = max(need, qi)
                    if need >= 0:
                        break
                if need >= 0:
                    allowed = len(queue) - 1 - need
                    waits.append((no, n, allowed))
                    if n < allowed:
                        errors.append("%s: line %d: lgkmcnt(%d) drains %d LDS operations issued behind the values it guards (lgkmcnt(%d) would do)" % (
                            tag, no, n, allowed - n, allowed))
            if n < len(queue):
                queue = queue[len(queue) - n:] if n else []
            if n == 0:
                stale, known = set(), True
            continue
        if OTHER_LGKM.match(s):
            errors.append("%s: line %d: %s counts in lgkmcnt beside the LDS traffic of the hash loop" % (tag, no, s.split()[0]))
            continue
        mn, ops = split_ops(s)
        touched = vregs(s)
        pending = set().union(*[r for _, r in queue]) if queue else set()
        hit = touched & (pending | stale)
        if hit:
            errors.append("%s: line %d: `%s` touches v%d, the destination of an LDS read no wait has retired" % (tag, no, s[:60], min(hit)))
        if mn.startswith("ds_"):
            dest = vregs(ops[0]) if ("read" in mn or "_rtn" in mn or "permute" in mn) and ops else set()
            queue.append([no, dest])
    return errors, waits


def check(path, expect_la=None):
    lines = open(path).read().split("\n")
    errors, report = [], []
    kern, begin, la, seen = None, None, None, 0
    body = []
    for i, ln in enumerate(lines):
        s = ln.strip()
        m = re.match(r"(_Z\S*tile_minimizer_kernel\S*):", s)
        if m:
            short = re.search(r"tile_minimizer_kernelILi(\d+)ELb(\d)ELb(\d)ELi(\d+)", m.group(1))
            kern = "L=%s hpc=%s desc=%s mode=%s" % short.groups() if short else m.group(1)
        m = re.search(r"S2K_MARK hash_(begin|end) la=(\d+)", s)
        if m and kern:
            if m.group(1) == "begin":
                begin, la, body = i, int(m.group(2)), []
            elif begin is not None:
                seen += 1
                e, waits = check_region(body, kern)
                errors += e
                counted = [w for w in waits if w[1] > 0]
                zero = [w for w in waits if w[1] == 0]
                report.append("%s la=%d: hash loop = lines %d..%d, %d waits in front of a look-up's consumer: %d counted (lgkmcnt %s), %d lgkmcnt(0) of which %d drain look-ups in flight" % (
                    kern, la, begin + 1, i + 1, len(waits), len(counted), "/".join(str(n) for n in sorted({w[1] for w in counted})) or "-",
                    len(zero), len([w for w in zero if w[2] > 0])))
                if not counted:
                    errors.append("%s: no counted lgkmcnt wait in the hash loop" % kern)
                if expect_la is not None and "hpc=1" in kern and la != expect_la:
                    errors.append("%s: look-ahead %d, expected %d" % (kern, la, expect_la))
                begin = None
            continue
        if begin is None or not s:
            continue
        if LABEL.match(s):
            body.append((i + 1, s))
        elif not s.startswith((";", ".", "//")):
            body.append((i + 1, s.split(";")[0].strip()))
    if not seen:
        errors.append("%s: no marked hash loop found" % path)
    return errors, report


def main():
    args = sys.argv[1:]
    expect = None
    if args[:1] == ["--expect-hpc-la"]:
        expect, args = int(args[1]), args[2:]
    bad = []
    for p in args:
        e, r = check(p, expect)
        for x in r:
            print(x)
        bad += e
    for x in bad[:40]:
        print("ERROR:", x, file=sys.stderr)
    if len(bad) > 40:
        print("ERROR: ... and %d more" % (len(bad) - 40), file=sys.stderr)
    return 1 if bad or not args else 0


if __name__ == "__main__":
    sys.exit(main())
