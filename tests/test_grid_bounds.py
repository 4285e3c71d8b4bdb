"""Every bounded grid of the graph, read-path and alignment side, taken past its bound.

The element-wise kernels of these families are launched through grid_for(n) (csrc/s2k_graph_dev.h): at most UB_MAX = 4096 blocks of
UT = 256 lanes, the rest left to a grid-stride loop, so past GRID = 1 048 576 items every lane takes a second trip.  The bubble and the
alignment grids are bounded in waves (S2K_BUBBLE_WAVES, S2K_ALIGN_WAVES), the alignment's trace by AL_TRACE_BUDGET as well.  The real
inputs are always past these bounds; the family files' cases almost never are.  Here every call runs on R disjoint copies of one of
its family's small cases (tests/replicas.py), R the smallest number that takes the call's governing counts past the bound, and its
arrays are compared byte for byte with the family's Python reference on one copy, carried to R copies.

CPU tier: the replication commutes with every reference at R = 3; each component makes every counter non-zero; COVERAGE has a row for
every bounded launch the sources hold; the sizes the device tests use lie past the bounds the sources state."""
import functools
import glob
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from s2k_loader import import_package

import replicas as rp
import test_align as ta
import test_align_segments as tas
import test_bridge as tbr
import test_bubbles as tbu
import test_lift as tl
import test_pileup as tp
import test_pileup_long as tpl
import test_simplify as ts
import test_span as tsp
import test_walk as twk

pkg = import_package()

CSRC = os.path.join(ROOT, "rust-seq2kminmers_amd", "csrc")
GRID = 4096 * 256          # lanes of one pass of a grid_for launch
SCAN_SEAM = 256 * 16 * 1024  # entries launch_scan_u32 takes before scan_block_offsets carries a total into its second chunk
NONE = rp.NONE


def past(n_per_copy, bound=GRID):
    """the smallest R for which R * n_per_copy exceeds the bound"""
    return bound // n_per_copy + 1


# ---- the components --------------------------------------------------------------------------------------------------------------------
MASK_BOUNDS = {"s2k_graph_simplify_mask": (4, 8), "s2k_graph_bubble_mask": (8, 8)}  # max_tip, max_bubble; max_nodes, max_bubble


@functools.lru_cache(maxsize=None)
def mask_component():
    """a planted graph of test_bubbles.py read as its unitig graph: 45 unitigs, 102 edges; tips, simple bubbles, and bubbles that are
    not simple, of which some are found from both ends and applied from one"""
    g = tbu.planted_graph(np.random.default_rng(211), 30, 0, 4, 4, 5)
    uni, uro, ud, ucnt = ts.unitig_view(g)
    return {"ro": uro, "d": ud, "off": uni["uni_off"], "cnt": ucnt}


def mask_reference(name, case):
    fn = ts.simplify_reference if name == "s2k_graph_simplify_mask" else tbu.bubble_reference
    return fn(case["ro"], case["d"], case["off"], case["cnt"], *MASK_BOUNDS[name])


@functools.lru_cache(maxsize=None)
def spans_component():
    """the eight hand-made unitigs of test_span.py and their thirteen reads: followed and off-graph steps, keys, a loop, a hairpin"""
    ro, d, off = tsp.hand_graph()
    return {"paths": tsp.hand_paths()[0], "ro": ro, "d": d, "off": off}


def spans_reference(case):
    return tsp.spans_reference(case["paths"], case["ro"], case["d"], case["off"])


@functools.lru_cache(maxsize=None)
def resolve_component():
    """the same graph with the counted keys of its reads, at min_support 1: two candidates' worth of strands, R resolved"""
    c = spans_component()
    sk, sc = tsp.count_keys(spans_reference(c)["keys"])
    return {"ro": c["ro"], "d": c["d"], "T": len(c["off"]) - 1, "sk": sk, "sc": sc, "ms": 1}


def resolve_reference(case):
    return tsp.resolve_reference(case["ro"], case["d"], case["T"], case["sk"], case["sc"], case["ms"])


@functools.lru_cache(maxsize=None)
def lift_component():
    """case a of test_lift.py, the X-shaped repeat untangled into two contigs, with its eleven hand-made reads: merged steps, a dropped
    step, a conflict, steps on both strands"""
    return tl.hand_lift("a")


@functools.lru_cache(maxsize=None)
def copy_places_component():
    c = lift_component()
    return {"outer": {f: c["r"]["o"][f] for f in ("uni_off", "members", "circular")}, "origin": c["origin"],
            "inner": {f: c["inner"][f] for f in ("uni_off", "circular")}}


def copy_places_reference(case):
    return tl.copy_places_reference(case["outer"], case["origin"], case["inner"])


@functools.lru_cache(maxsize=None)
def targets_component():
    """the two unitigs of test_align.junction_case: a sound walk over both on twin strands, a junction above a length, a path_end past the
    stitched length, path_start above path_end"""
    walks, su, strings, overlap = ta.junction_case()
    return {"walks": {f: walks[f] for f in tp.REC}, "su": su, "strings": strings, "overlap": overlap}


def targets_reference(case):
    return ta.targets_reference(case["walks"], case["su"], case["strings"], case["overlap"])


@functools.lru_cache(maxsize=None)
def pileup_component():
    """the two overlapping unitigs of test_pileup.two_unitigs (70 draft bases) under thirty walks -- two-step walks over the junction on
    both strands, one-step walks on every oriented unitig -- whose queries carry up to four random edits; two walks are flagged.  Three
    more as the family's hand cases make them: an insertion behind the last base of a unitig (n_end_ins), an insertion into an empty
    target (n_empty_ins), an N under an X run (n_other).  Every plane gets a vote, ins_long too, and gaps are shifted"""
    strings, overlap, su = tp.two_unitigs()
    rng = np.random.default_rng(308)
    specs = []
    for i in range(30):
        if i % 4 < 2:
            a = int(rng.integers(0, 20))
            specs.append((0 if i % 4 == 0 else 2, 2, a, int(rng.integers(45, 65)), 0))
        else:
            st = int(rng.integers(0, 4))
            L = len(strings[int(su[st]) >> 1])
            a = int(rng.integers(0, L - 12))
            specs.append((st, 1, a, a + int(rng.integers(8, L - a + 1)), 0))
    walks = tp.one_walks(specs)
    q, fl, runs = tp.aligned_case(walks, su, strings, overlap, rng, 4)
    fl = fl.copy()
    fl[5], fl[11] = 1, 2
    more = [(0, 1, 0, 40, 0), (0, 1, 7, 7, 0), (0, 1, 10, 40, 0)]  # on unitig 0, forward
    tgt = strings[0][10:40]
    hand = tp._single(strings, more, ["40=1I", "3I", "5=1X24="], rng, su=su, overlap=overlap, queries=None)
    q = q + [hand[4][0], hand[4][1], tgt[:5] + b"N" + tgt[6:]]
    runs = runs + hand[6]
    fl = np.concatenate([fl, np.zeros(3, dtype=np.uint32)])
    walks = tp.one_walks(specs + more)
    return {"walks": walks, "su": su, "strings": strings, "overlap": overlap, "queries": q, "flags": fl, "runs": runs, "max_shift": tp.MAX_SHIFT}


def pileup_reference(case):
    return tp.pileup_reference(case["walks"], case["su"], case["strings"], case["overlap"], case["queries"], case["flags"], case["runs"], case["max_shift"])


def pileup_arrays(case):
    """the component as the arrays s2k_walks_pileup takes, packed by the family's own helpers"""
    out_off, out = tp.draft_of(case["strings"])
    pool, qb = tp.query_pool(case["queries"])
    ops_off, n_ops, ops = tp.alignment_arrays(case["flags"], case["runs"])
    return dict({f: case["walks"][f] for f in tp.REC}, unitig=case["su"], out_off=out_off, out=out, overlap=case["overlap"], query=pool, q_begin=qb,
                aflags=np.asarray(case["flags"], dtype=np.uint32), ops_off=ops_off, n_ops=n_ops, ops=ops)


JOIN_SEED = 1
CONSENSUS_EX_SEED = 0
CONSENSUS_LENS = (0, 1, 3, 2, 5, 1, 4, 0, 2, 3)


@functools.lru_cache(maxsize=None)
def consensus_component():
    """ten unitigs of 0 .. 5 bases (21 in all: few bases a unitig, so that the unitigs pass one grid pass where the bases pass the scan's
    seam) under a random pile in which most positions carry an event: low coverage, substitutions, deletions, insertions, long ones"""
    rng = np.random.default_rng(8)
    strings = [ta.random_seq(rng, n, b"ACGTacgtN") for n in CONSENSUS_LENS]
    overlap = np.array([int(rng.integers(0, n + 3)) for n in CONSENSUS_LENS for _ in (0, 1)], dtype=np.uint32)
    return {"pile": tp.random_pile(rng, strings, p_event=0.7, depth=8), "strings": strings, "overlap": overlap, "min_cov": 3}


def consensus_reference(case):
    return tp.consensus_reference(case["pile"], case["strings"], case["overlap"], case["min_cov"])


@functools.lru_cache(maxsize=None)
def consensus_ex_component():
    """the consensus component with a table of long insertions over its 21 positions (none past the draft: a copy's positions end where the
    next copy's begin) and ins_long raised where the table is to be searched"""
    c = consensus_component()
    pile = {f: v.copy() for f, v in c["pile"].items()}
    keys, counts = tpl.random_table(np.random.default_rng(CONSENSUS_EX_SEED), pile, sum(CONSENSUS_LENS), p_cand=0.2, many=2)
    inside = rp.rev36(keys >> np.uint64(28)) < sum(CONSENSUS_LENS)
    return dict(c, pile=pile, keys=keys[inside], counts=counts[inside])


def consensus_ex_reference(case):
    return tpl.consensus_long_reference(case["pile"], case["strings"], case["overlap"], case["min_cov"], case["keys"], case["counts"])


def pileup_ex_reference(case):
    return tpl.long_keys_reference(case["walks"], case["su"], case["strings"], case["overlap"], case["queries"], case["flags"], case["runs"], case["max_shift"])


@functools.lru_cache(maxsize=None)
def join_component():
    """sixteen walks of 0 .. 4 segments with random CIGARs (test_align_segments.random_segments): chains of = that collapse, runs that
    meet an equal op at a border, over segments and bad walks"""
    seg_off, bad, seg = tas.random_segments(np.random.default_rng(JOIN_SEED), 16, p_over=0.1, p_bad=0.1)
    return {"seg_off": seg_off, "bad": bad, "seg": seg}


def join_reference(case):
    ref = tas.join_reference(case["seg_off"], case["bad"], case["seg"])
    return dict({f: ref[f] for f in ("edits", "flags", "n_ops", "matches", "ops_off")}, ops=np.concatenate([np.zeros(0, dtype=np.uint32)] + list(ref["ops"])))


@functools.lru_cache(maxsize=None)
def segments_component():
    """every hand case of test_align_segments.py as the walks of one call: anchors outside the ends, behind the maxima, in one bucket, in
    bucket 0, a walk without a candidate, a bad and a circular walk, negative offsets, a source step moved off its step and one without a
    step (items outside)"""
    walks, shift, no_step = [], {}, []
    for ws, kw, _, _ in tas.HAND.values():
        shift.update({len(walks) + i: d for i, d in kw.get("shift", {}).items()})
        no_step += [len(walks) + i for i in kw.get("no_step", ())]
        walks += ws
    return tas.anchor_case(walks, shift=shift, no_step=tuple(no_step))


@functools.lru_cache(maxsize=None)
def segments_one_walk():
    """one walk on one unitig of two nodes: the component of the check's unitig loop, which needs more unitigs than one pass"""
    return tas.anchor_case([tas._w([(600, 600)])])


def segments_reference(case):
    ref = tas.segments_reference(case)
    return {f: ref[f] for f in tas.SEG_F + ("stats",)}


def _same(got, want, tag):
    """two results of a reference, field by field: arrays by their bytes and dtype, everything else by =="""
    if isinstance(want, dict):
        assert set(got) == set(want), tag
        got, want = [got[k] for k in sorted(want)], [want[k] for k in sorted(want)]
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (tag, i)
        elif isinstance(w, (list, tuple, dict)):
            _same(g, w, (tag, i))
        else:
            assert g == w, (tag, i, g, w)


# name -> (component, reference(case), expected(ref, R, case), the counters that must not be 0 on the component: (what, value(ref)))
FAMILIES = {
    "s2k_graph_simplify_mask": (mask_component, functools.partial(mask_reference, "s2k_graph_simplify_mask"), lambda ref, R, case: rp.mask_expected(ref, R),
                                (("tips", lambda r: r[1]), ("bubbles", lambda r: r[2]), ("removed", lambda r: r[3]), ("kept", lambda r: len(r[0]) - r[3]))),
    "s2k_graph_bubble_mask": (mask_component, functools.partial(mask_reference, "s2k_graph_bubble_mask"), lambda ref, R, case: rp.mask_expected(ref, R),
                              (("sources", lambda r: r[1]), ("found", lambda r: r[2]), ("applied", lambda r: r[3]), ("removed", lambda r: r[4]),
                               ("found and not applied", lambda r: r[2] - r[3]), ("sources without a bubble", lambda r: r[1] - r[2]))),
    "s2k_paths_spans": (spans_component, spans_reference, lambda ref, R, case: rp.spans_expected(ref, R, len(case["d"])),
                        (("keys", lambda r: len(r["keys"])), ("followed", lambda r: r["n_followed"]), ("off-graph", lambda r: r["n_off_graph"]),
                         ("edge support", lambda r: int(r["edge_support"].sum())))),
    "s2k_graph_resolve_mask": (resolve_component, resolve_reference, lambda ref, R, case: rp.resolve_expected(ref, R, len(case["d"])),
                               (("candidates", lambda r: r[2]), ("resolved", lambda r: r[3]), ("partners", lambda r: int((r[1] != NONE).sum())),
                                ("unitigs not resolved", lambda r: len(r[0]) - r[3]), ("edges without a partner", lambda r: int((r[1] == NONE).sum())))),
    "s2k_pileup_consensus": (consensus_component, consensus_reference, lambda ref, R, case: rp.consensus_expected(ref, R),
                             tuple((f, lambda r, f=f: r["stats"][f]) for f in tp.C_STATS) +
                             (("bases kept", lambda r: len(r["out"])), ("overlaps", lambda r: int(r["overlap"].sum())))),
    "s2k_walks_segments": (segments_component, segments_reference,
                           lambda ref, R, case: rp.segments_expected(ref, R, rp.query_span(case), int(case["tgt_off"][-1])),
                           tuple((f, lambda r, i=i: r["stats"][i]) for i, f in enumerate(tas.STATS)) + (("segments", lambda r: len(r["q_begin"])),)),
    "s2k_align_join": (join_component, join_reference, lambda ref, R, case: rp.join_expected(dict(ref, ops=[ref["ops"]]), R),
                       (("joined walks", lambda r: int(((r["flags"] == 0) & (r["n_ops"] > 0)).sum())), ("over walks", lambda r: int((r["flags"] & ta.OVER != 0).sum())),
                        ("bad walks", lambda r: int((r["flags"] & tas.BAD_PATH != 0).sum())), ("edits", lambda r: int(r["edits"].sum())),
                        ("matches", lambda r: int(r["matches"].sum())), ("runs", lambda r: len(r["ops"])))),
    "s2k_pileup_consensus_ex": (consensus_ex_component, consensus_ex_reference, lambda ref, R, case: rp.consensus_expected(ref, R),
                                tuple((f, lambda r, f=f: r["stats"][f]) for f in tpl.C_LONG_STATS)),
    "s2k_walks_pileup_ex": (pileup_component, pileup_ex_reference,
                            lambda ref, R, case: rp.pileup_ex_expected(ref, R, sum(len(x) for x in case["strings"])),
                            (("keys", lambda r: len(r[0])), ("candidates", lambda r: r[1]))),
    "s2k_walks_pileup": (pileup_component, pileup_reference, lambda ref, R, case: rp.pileup_expected(ref, R),
                         tuple((f, lambda r, f=f: int(r[0][f].sum())) for f in tp.PLANES) +
                         tuple((f, lambda r, f=f: r[1][f]) for f in tp.P_STATS)),
    "s2k_walks_targets": (targets_component, targets_reference, lambda ref, R, case: rp.targets_expected(ref, R),
                          (("bad walks", lambda r: int(r[2].sum())), ("sound walks", lambda r: int((r[2] == 0).sum())), ("bytes", lambda r: len(r[1])))),
    "s2k_paths_walks": (twk.hand_case, twk.reference_of, lambda ref, R, case: rp.walks_expected(ref, R, len(case["paths"]["unitig"]), len(case["d"])),
                        (("walks", lambda r: r["n_walks"]), ("followed", lambda r: r["n_followed"]), ("off-graph", lambda r: r["n_off_graph"]),
                         ("walks round a circular unitig", lambda r: int(r["flags"].sum())))),
    "s2k_paths_bridge": (tbr.hand_case, tbr.reference_of, lambda ref, R, case: rp.bridge_expected(ref, R, len(case["ro"]) - 1),
                         (("steps", lambda r: r["n_steps"]), ("merged", lambda r: r["n_merged"]), ("bridged", lambda r: r["n_bridged"]))),
    "s2k_unitig_copy_places": (copy_places_component, copy_places_reference, lambda ref, R, case: rp.copy_places_expected(ref, R, len(case["outer"]["circular"])),
                               (("copies", len), ("copies behind their contig's first", lambda r: int((r["pos"] > 0).sum())),
                                ("contigs of several copies", lambda r: int((r["len"] > 1).sum())))),
    "s2k_paths_lift": (lift_component, lambda case: tl.lift_reference(case), lambda ref, R, case: rp.lift_expected(ref, R, case["n_copies"], case["n_contigs"]),
                       (("steps", lambda r: r["n_steps"]), ("merged", lambda r: r["n_merged"]), ("dropped", lambda r: r["n_dropped"]),
                        ("conflicts", lambda r: r["n_conflicts"]), ("contig items", lambda r: int(r["contig_items"].sum())),
                        ("steps on the twin strand", lambda r: int((r["unitig"] & 1).sum())))),
}


# ---- CPU tier: the replication and the components -----------------------------------------------------------------------------------------
def test_every_family_has_its_two_functions():
    assert set(FAMILIES) == set(rp.CALLS)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_reference_commutes_with_the_replication(name):
    """reference(replicate_inputs(case, 3)) == replicate_expected(reference(case), 3), every field: what makes the expectation at a
    million ids trustworthy.  R = 1 gives the case back."""
    component, reference, expected, _ = FAMILIES[name]
    case = component()
    ref = reference(case)
    _same(reference(rp.CALLS[name][0](case, 3)), expected(ref, 3, case), name)
    _same(expected(ref, 1, case), ref, (name, "R = 1"))


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_component_makes_every_counter_non_zero(name):
    component, reference, _, counters = FAMILIES[name]
    ref = reference(component())
    for what, value in counters:
        assert value(ref) > 0, (name, what)


def test_replication_rules():
    assert rp.offsets(np.array([0, 2, 5], dtype=np.uint64), 3).tolist() == [0, 2, 5, 7, 10, 12, 15]
    assert rp.shifted(np.array([1, NONE, 0], dtype=np.uint32), 2, 4, keep=NONE).tolist() == [1, NONE, 0, 5, NONE, 4]
    assert rp.keys32(np.array([1 << 32 | 2], dtype=np.uint64), 2, 10, 10).tolist() == [1 << 32 | 2, 11 << 32 | 12]
    with pytest.raises(AssertionError):
        rp.shifted(np.array([5], dtype=np.uint32), 3, 2 ** 31)  # an id that would not fit its type


# ---- the coverage table ----------------------------------------------------------------------------------------------------------------
ME = "test_grid_bounds.py::"
_OLD_UNITIG = "test_unitigs.py::test_device_long_chain_and_cycle_rounds"
_OLD_UNTANGLE = "test_untangle.py::test_device_more_lanes_than_one_grid_pass"
# (source file, kernel) -> (the count that governs its grid, the test that takes it past the bound or None, a note).  A check kernel
# shows its later trips only by a refusal: its test plants one malformed entry behind the first pass.  None: no test goes there yet,
# and the note says why or what is missing.
COVERAGE = {
    ("s2k_simplify.hip", "simplify_check_kernel"): ("n_ids", ME + "test_device_simplify_check_refuses_in_the_second_pass", "a unitig without a member"),
    ("s2k_simplify.hip", "simplify_mask_kernel"): ("n_ids", ME + "test_device_simplify_mask_past_one_grid_pass", ""),
    ("s2k_bubble.hip", "bubble_kernel"): ("sources / S2K_BUBBLE_WAVES", ME + "test_device_bubble_mask_three_sources_a_wave", "both passes; poisoned as well"),
    ("s2k_span.hip", "spans_check_kernel"): ("n_ids (n_reads + 1 and n_steps stay in one pass)", ME + "test_device_spans_check_refuses_in_the_second_pass",
                                            "a unitig without a member; its step loop checks an id's range alone and is left out"),
    ("s2k_span.hip", "spans_support_kernel"): ("n_steps", ME + "test_device_spans_past_one_grid_pass", ""),
    ("s2k_span.hip", "resolve_check_kernel"): ("n_ids, n_spans", ME + "test_device_resolve_check_refuses_in_the_second_pass",
                                              "a row offset that decreases in range; a span key repeated"),
    ("s2k_span.hip", "resolve_mask_kernel"): ("n_ids", ME + "test_device_resolve_mask_past_one_grid_pass", ""),
    ("s2k_lift.hip", "places_check_kernel"): ("n_unitigs + 1, n_contigs + 1, n_copies", ME + "test_device_copy_places_check_refuses_in_the_second_pass",
                                             "a unitig without a member, a contig without a copy; its copy loop checks two ids' ranges alone and is left out"),
    ("s2k_lift.hip", "places_verify_kernel"): ("n_copies", ME + "test_device_copy_places_verify_refuses_in_the_second_pass", "a copy named by two pieces"),
    ("s2k_lift.hip", "places_contig_kernel"): ("n_contigs", None, "left out: its own rule, a contig of 2^32 instances, cannot be built; an offset that decreases is "
                                                                  "places_check_kernel's finding as well"),
    ("s2k_lift.hip", "places_write_kernel"): ("n_copies", ME + "test_device_copy_places_past_one_grid_pass", ""),
    ("s2k_lift.hip", "lift_check_kernel"): ("n_steps, 2 n_unitigs (n_reads + 1 stays in one pass)", ME + "test_device_lift_check_refuses_in_the_second_pass",
                                           "a step with count = 0; a row offset that decreases in range"),
    ("s2k_lift.hip", "lift_items_kernel"): ("n_steps", ME + "test_device_lift_past_one_grid_pass", "contig_items"),
    ("s2k_bridge.hip", "bridge_check_kernel"): ("n_steps, 2 n_unitigs (n_reads + 1 stays in one pass)", ME + "test_device_bridge_check_refuses_in_the_second_pass",
                                               "a step with count = 0; a row offset that decreases in range"),
    ("s2k_walk.hip", "walks_check_kernel"): ("n_steps, 2 n_unitigs (n_reads + 1 and n_nodes stay in one pass)", ME + "test_device_walks_check_refuses_in_the_second_pass",
                                            "a step with count = 0; a row offset that decreases in range; its node loop is left out: what a member offset "
                                            "outside its unitig would do to the coordinates was not worked out"),
    ("s2k_targets_dev.h", "tg_check_kernel"): ("n_unitigs (n_all_steps and n_walks stay in one pass)", ME + "test_device_targets_check_refuses_in_the_second_pass",
                                               "an out_off that decreases in range; its step loop checks an id's range alone, and its walk loop checks that a walk's "
                                               "steps lie inside the step array: a walk let through would be read outside it, so both are left out"),
    ("s2k_segment.hip", "sg_check_kernel"): ("n_reads (src_off, km_off), n_nodes, n_unitigs", ME + "test_device_segments_check_refuses_in_the_second_pass",
                                            "a source read offset, a km_off and an out_off that decrease in range, a member offset past its unitig's bases; "
                                            "the walk loop's rules (qstart above qend, target offsets) size later loops, so no entry of theirs is planted; walk_off "
                                            "and the steps run inside path_off_ok and steps_ok, pinned by the spans, lift, bridge and walks checks"),
    ("s2k_segment.hip", "sg_steps_kernel"): ("n_src_steps", ME + "test_device_segments_past_one_grid_pass", ""),
    ("s2k_segment.hip", "sg_off_kernel"): ("n_walks + 1", ME + "test_device_segments_past_one_grid_pass", ""),
    ("s2k_segment.hip", "sg_segments_kernel"): ("the segment total", ME + "test_device_segments_past_one_grid_pass", ""),
    ("s2k_segment.hip", "jn_check_kernel"): ("n_walks + 1, n_segments", ME + "test_device_join_past_one_grid_pass", "n_ops above a segment's slots; a segment offset that decreases in range"),
    ("s2k_segment.hip", "jn_over_kernel"): ("n_segments", ME + "test_device_join_past_one_grid_pass", ""),
    ("s2k_segment.hip", "jn_lens_kernel"): ("n_heads, n_walks", ME + "test_device_join_past_one_grid_pass", ""),
    ("s2k_segment.hip", "jn_walks_kernel"): ("n_walks + 1", ME + "test_device_join_past_one_grid_pass", ""),
    ("s2k_segment.hip", "jn_ops_kernel"): ("n_heads", ME + "test_device_join_past_one_grid_pass", ""),
    ("s2k_pileup.hip", "pl_offsets_kernel"): ("n_walks", ME + "test_device_pileup_past_one_grid_pass_and_the_scan_seam", "n_ops above a walk's slots"),
    ("s2k_pileup.hip", "pl_slots_kernel"): ("n_slots", ME + "test_device_pileup_past_one_grid_pass_and_the_scan_seam", ""),
    ("s2k_pileup.hip", "pl_walks_kernel"): ("n_walks", ME + "test_device_pileup_past_one_grid_pass_and_the_scan_seam", ""),
    ("s2k_pileup.hip", "pl_vote_kernel"): ("n_slots", ME + "test_device_pileup_past_one_grid_pass_and_the_scan_seam", "without and with a key buffer"),
    ("s2k_pileup.hip", "pl_match_b_kernel"): ("n_slots", None, "route B: S2K_PILEUP_ROUTE is read only in a build with S2K_DEBUG_KNOBS; no shipped knob or size selects it"),
    ("s2k_pileup.hip", "pl_apply_kernel"): ("n_bases", ME + "test_device_pileup_past_one_grid_pass_and_the_scan_seam", "both difference planes are scanned past SCAN_SEAM"),
    ("s2k_pileup.hip", "pl_keys_kernel"): ("n_slots", ME + "test_device_pileup_past_one_grid_pass_and_the_scan_seam", "s2k_walks_pileup_ex: one key a copy"),
    ("s2k_pileup.hip", "cs_check_kernel"): ("n_unitigs", ME + "test_device_consensus_past_one_grid_pass_and_the_scan_seam", "an offset that decreases in range"),
    ("s2k_pileup.hip", "cs_keys_kernel"): ("the key table's n", ME + "test_device_consensus_ex_past_one_grid_pass_and_the_scan_seam", "a key repeated"),
    ("s2k_pileup.hip", "cs_call_kernel"): ("n_bases", ME + "test_device_consensus_past_one_grid_pass_and_the_scan_seam", "its counts are scanned past SCAN_SEAM: pos_map"),
    ("s2k_pileup.hip", "cs_units_kernel"): ("n_unitigs + 1", ME + "test_device_consensus_past_one_grid_pass_and_the_scan_seam", ""),
    ("s2k_pileup.hip", "cs_write_kernel"): ("n_bases", ME + "test_device_consensus_past_one_grid_pass_and_the_scan_seam", ""),
    # before this file: the two families the device tier already took past one pass
    ("s2k_unitig.hip", "check_kernel"): ("n_ids", _OLD_UNITIG, "2 (2^21 + 3) ids, accepted: no refusal from a second trip"),
    ("s2k_unitig.hip", "link_kernel"): ("n_ids", _OLD_UNITIG, ""),
    ("s2k_unitig.hip", "jump_kernel"): ("n_ids", _OLD_UNITIG, ""),
    ("s2k_unitig.hip", "cyc_init_kernel"): ("n_ids", _OLD_UNITIG, "its cycle case"),
    ("s2k_unitig.hip", "cyc_min_kernel"): ("n_ids", _OLD_UNITIG, "its cycle case"),
    ("s2k_unitig.hip", "cyc_cut_kernel"): ("n_ids", _OLD_UNITIG, "its cycle case"),
    ("s2k_unitig.hip", "head_kernel"): ("n_ids", _OLD_UNITIG, ""),
    ("s2k_unitig.hip", "len_kernel"): ("n_ids", _OLD_UNITIG, ""),
    ("s2k_unitig.hip", "scatter_kernel"): ("n_ids", _OLD_UNITIG, ""),
    ("s2k_unitig.hip", "uedge_count_kernel"): ("2 n_unitigs", None, "the long chain compacts to a few unitigs: not past one pass in any test"),
    ("s2k_unitig.hip", "uedge_write_kernel"): ("2 n_unitigs", None, "as uedge_count_kernel"),
    ("s2k_untangle.hip", "untangle_check_kernel"): ("n_ids", _OLD_UNTANGLE, "2 * 530 030 ids, accepted: no refusal from a second trip"),
    ("s2k_untangle.hip", "copies_kernel"): ("n_unitigs", None, "530 030 unitigs there: half a pass"),
    ("s2k_untangle.hip", "degree_kernel"): ("2 n_copies", _OLD_UNTANGLE, ""),
    ("s2k_untangle.hip", "untangle_write_kernel"): ("2 n_copies", _OLD_UNTANGLE, ""),
    ("s2k_untangle.hip", "expand_check_kernel"): ("max(n_copies, n_unitigs) + 1", None, "about 530 000 copies there: half a pass"),
    ("s2k_untangle.hip", "contig_kernel"): ("n_contigs + 1", None, "about 530 000 contigs there: half a pass"),
    ("s2k_align.hip", "al_check_kernel"): ("n_pairs", ME + "test_device_align_check_refuses_in_the_second_pass", "a query interval past n_query_bytes"),
    ("s2k_align.hip", "al_score_kernel"): ("n_pairs / S2K_ALIGN_WAVES", ME + "test_device_align_trace_under_its_budget", ""),
    ("s2k_align.hip", "al_trace_kernel"): ("n_pairs / the waves AL_TRACE_BUDGET admits", ME + "test_device_align_trace_under_its_budget", ""),
}


# launch_scan_u32 past SCAN_SEAM entries (scan_block_offsets then carries a total from one chunk of 1024 block sums into the next).
# Before this file one test went there: the 50 Mbp case extracts 150 000 reads of 10 kbp at l = 31, k = 10, d = 0.01 in one call, about
# 100 minimizers and so about 91 items a read, and s2k_table_node_sequences scans the lengths of those 13.6 M items; it compares stitched
# unitigs with slices of the genome, not the offsets themselves.  The consensus test here compares pos_map, every entry a scanned sum.
SCAN_SEAM_CROSSED_BY = ("test_unitig_sequences.py::test_full_size_genome_sampled_sequences", ME + "test_device_consensus_past_one_grid_pass_and_the_scan_seam")


def _statement(text, at):
    """the text between the parenthesis at `at` and its partner"""
    depth = 0
    for i in range(at, len(text)):
        depth += text[i] == "("
        depth -= text[i] == ")"
        if depth == 0:
            return text[at + 1: i]
    raise AssertionError("unbalanced")


def _top_level_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "(<[{"
        depth -= ch in ")>]}"
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return [x.strip() for x in out + [cur]]


_BOUNDED = re.compile(r"grid_for\(|S2K_BUBBLE_WAVES|S2K_ALIGN_WAVES")


def bounded_launches(text):
    """the kernels a source launches with a bounded grid: through grid_for(, or with a grid variable that was set from grid_for( or
    from one of the two wave bounds (or from such a variable) -> a set of kernel names, template arguments dropped"""
    events = [(m.start(), "set", m) for m in re.finditer(r"\bunsigned (\w+) =([^;]*);", text)]
    events += [(m.start(), "launch", m) for m in re.finditer(r"\b(hipLaunchKernelGGL|c\.launch)\(", text)]
    bounded, found = {}, set()
    for _, kind, m in sorted(events, key=lambda e: e[0]):
        uses = lambda expr: bool(_BOUNDED.search(expr)) or any(re.search(r"\b%s\b" % v, expr) for v, b in bounded.items() if b)  # noqa: E731
        if kind == "set":
            bounded[m.group(1)] = uses(m.group(2))
            continue
        args = _top_level_args(_statement(text, m.end() - 1))
        if uses(args[1]):
            kernels = set(re.findall(r"\b(\w+_kernel)\b", args[0]))
            assert kernels, args[0]
            found |= kernels
    return found


def launches_in_the_sources():
    out = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))) + [os.path.join(CSRC, "s2k_targets_dev.h")]:
        out |= {(os.path.basename(path), k) for k in bounded_launches(open(path).read())}
    return out


def test_parser_on_the_shapes_the_sources_use():
    text = """
        const unsigned grid = grid_for(n_ids);
        hipLaunchKernelGGL(a_kernel, dim3(grid), dim3(UT), 0, c.st, x);
        c.launch(T ? b_kernel<true> : b_kernel<false>, grid_for(n_bases), UT, *pile,
                 more);
        const unsigned blocks = (unsigned)((std::min<uint64_t>(ns, S2K_BUBBLE_WAVES) + UT / 64 - 1) / (UT / 64));
        const unsigned tblocks = (unsigned)std::min<uint64_t>(blocks, fit / 4);
        c.launch(c_kernel<false>, tblocks, UT, g);
        c.launch(tile_kernel, (unsigned)n_tiles, TB_THREADS, g);
        const unsigned grid = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(free_kernel, dim3(grid), dim3(256), 0, c.st, g);
    """
    assert bounded_launches(text) == {"a_kernel", "b_kernel", "c_kernel"}


def test_every_bounded_launch_has_a_row():
    """a launch through grid_for( or one of the wave bounds without a row fails here, and so does a row whose launch is gone; a row's
    test exists"""
    found = launches_in_the_sources()
    assert len(found) > 40
    missing, stale = sorted(found - set(COVERAGE)), sorted(set(COVERAGE) - found)
    assert not missing and not stale, (missing, stale)
    for key, (count, test, note) in list(COVERAGE.items()) + [("the scan's seam", ("n", t, "")) for t in SCAN_SEAM_CROSSED_BY]:
        assert count and (test or note), key
        if test:
            path, name = test.split("::")
            assert re.search(r"^def %s\(" % name, open(os.path.join(ROOT, "tests", path)).read(), re.M), (key, test)


def constants():
    """the bounds as the sources state them"""
    def one(path, pattern):
        m = re.search(pattern, open(path).read(), re.M)
        assert m, (path, pattern)
        return m

    dev, util = os.path.join(CSRC, "s2k_graph_dev.h"), os.path.join(CSRC, "s2k_util.hip")
    align, header = os.path.join(CSRC, "s2k_align.hip"), os.path.join(ROOT, "include", "s2k.h")
    budget = one(align, r"^constexpr size_t AL_TRACE_BUDGET = (\d+)u << (\d+);")
    assert one(util, r"^constexpr int SCAN_BLOCK = SCAN_THREADS \* SCAN_ITEMS;") and one(util, r"for \(uint64_t base = 0; base < nb; base \+= 1024\)")
    assert one(util, r"__launch_bounds__\(1024\) void scan_block_offsets")
    return {"UT": int(one(dev, r"^constexpr int UT = (\d+);").group(1)), "UB_MAX": int(one(dev, r"^constexpr unsigned UB_MAX = (\d+);").group(1)),
            "SCAN_SEAM": int(one(util, r"^constexpr int SCAN_THREADS = (\d+);").group(1)) * int(one(util, r"^constexpr int SCAN_ITEMS = (\d+);").group(1)) * 1024,
            "AL_TRACE_BUDGET": int(budget.group(1)) << int(budget.group(2)), "AL_T": int(one(align, r"^constexpr int AL_T = (\d+);").group(1)),
            "S2K_BUBBLE_WAVES": int(one(header, r"^#define S2K_BUBBLE_WAVES (\d+)u").group(1)),
            "S2K_ALIGN_WAVES": int(one(header, r"^#define S2K_ALIGN_WAVES (\d+)u").group(1)),
            "S2K_ALIGN_MAX_EDITS": int(one(header, r"^#define S2K_ALIGN_MAX_EDITS (\d+)u").group(1))}


def trace_waves(emax, k):
    """the waves s2k_align_pairs gives its trace pass when the largest distance of a pair that is not over is emax"""
    per_block = k["AL_T"] // 64
    fit = max(k["AL_TRACE_BUDGET"] // (4 * (emax + 1) ** 2), per_block)
    return min(k["S2K_ALIGN_WAVES"] // per_block, fit // per_block) * per_block


def sizes():
    """what the device tests run: call -> (R, the governing counts at R, the bound they have to exceed)"""
    m, s, r = mask_component(), spans_component(), resolve_component()
    n_ids, n_src = len(m["ro"]) - 1, mask_reference("s2k_graph_bubble_mask", m)[1]
    out = {"s2k_graph_simplify_mask": (past(n_ids), [n_ids], GRID),
           "s2k_graph_bubble_mask": (past(n_src, 2 * pkg.BUBBLE_WAVES), [n_src], 2 * pkg.BUBBLE_WAVES),
           "s2k_paths_spans": (past(len(s["paths"]["unitig"])), [len(s["paths"]["unitig"])], GRID),
           "s2k_paths_spans, its check": (past(len(s["ro"]) - 1), [len(s["ro"]) - 1], GRID),
           "s2k_graph_resolve_mask": (past(2 * r["T"]), [2 * r["T"]], GRID),
           "s2k_graph_resolve_mask, its check": (past(min(2 * r["T"], len(r["sk"]))), [2 * r["T"], len(r["sk"])], GRID)}
    p, lf = copy_places_component(), lift_component()
    for name, n in (("s2k_unitig_copy_places", len(p["origin"])), ("s2k_unitig_copy_places, its inner offsets", len(p["inner"]["circular"])),
                    ("s2k_unitig_copy_places, its outer offsets", len(p["outer"]["circular"])), ("s2k_paths_lift", len(lf["paths"]["unitig"])),
                    ("s2k_paths_lift, its check", 2 * lf["T"]), ("s2k_paths_bridge", len(tbr.hand_case()["paths"]["unitig"])),
                    ("s2k_paths_bridge, its unitigs", len(tbr.hand_case()["ro"]) - 1),
                    ("s2k_paths_walks", len(twk.hand_case()["paths"]["unitig"])), ("s2k_paths_walks, its unitigs", len(twk.hand_case()["ro"]) - 1)):
        out[name] = (past(n), [n], GRID)
    for name, case in (("s2k_paths_spans", s), ("s2k_paths_lift", lf), ("s2k_paths_bridge", tbr.hand_case()), ("s2k_paths_walks", twk.hand_case())):
        n = len(case["paths"]["path_off"]) - 1
        out[name + ", its reads"] = (past(n), [n], GRID)
    out["s2k_walks_targets, its unitigs"] = (past(len(targets_component()["strings"])), [len(targets_component()["strings"])], GRID)
    g = segments_component()
    out["s2k_walks_segments"] = (past(min(len(g["bad"]), len(g["src"]["pos"]))), [len(g["bad"]), len(g["src"]["pos"]), len(segments_reference(g)["q_begin"])], GRID)
    for what, n in (("reads", len(g["km_off"]) - 1), ("nodes", len(g["uni"]["members"]))):
        assert n >= min(len(g["bad"]), len(g["src"]["pos"]))  # past one pass at the R of the result loops
        out["s2k_walks_segments, its %s" % what] = (out["s2k_walks_segments"][0], [n], GRID)
    # (the unitig before the last holds the malformed offset: its lane has to lie past the first pass as well)
    out["s2k_walks_segments, its unitigs"] = (past(len(segments_one_walk()["uni"]["circular"]), GRID + 1), [len(segments_one_walk()["uni"]["circular"])], GRID + 1)
    j = join_component()
    out["s2k_align_join"] = (past(len(j["bad"])), [len(j["bad"]), len(j["seg"]["edits"]), len(join_reference(j)["ops"])], GRID)
    n = sum(len(x) for x in pileup_component()["strings"])
    out["s2k_walks_pileup"] = (past(n, SCAN_SEAM), [n], SCAN_SEAM)
    n = len(twk.hand_case()["uni"]["members"])
    out["s2k_paths_walks, its nodes"] = (past(n), [n], GRID)
    out["s2k_pileup_consensus"] = (past(sum(CONSENSUS_LENS), SCAN_SEAM), [sum(CONSENSUS_LENS)], SCAN_SEAM)
    return out


def test_sizes_lie_past_the_bounds_the_sources_state():
    """a changed bound fails here, without a GPU: GRID and the other figures of this file are the sources'; every R is the smallest
    that takes each of its counts past the bound"""
    k = constants()
    assert k["UT"] * k["UB_MAX"] == GRID and k["SCAN_SEAM"] == SCAN_SEAM
    assert k["S2K_BUBBLE_WAVES"] == pkg.BUBBLE_WAVES and k["S2K_ALIGN_WAVES"] == pkg.ALIGN_WAVES and k["S2K_ALIGN_MAX_EDITS"] == pkg.ALIGN_MAX_EDITS == ta.MAX_EDITS
    for name, (R, counts, bound) in sizes().items():
        rides = name in ("s2k_walks_segments, its reads", "s2k_walks_segments, its nodes")  # at the R of the call's result loops
        assert all(R * c > bound for c in counts) and (rides or any((R - 1) * c <= bound for c in counts)), (name, R, counts)
    assert sizes()["s2k_graph_bubble_mask"][0] * sizes()["s2k_graph_bubble_mask"][1][0] <= 3 * pkg.BUBBLE_WAVES  # three sources a wave, not four
    assert ALIGN_PAIRS == 2 * k["S2K_ALIGN_WAVES"] + 1 and ALIGN_CHECK_PAIRS > GRID
    assert k["AL_TRACE_BUDGET"] == 256 << 20 and trace_waves(k["S2K_ALIGN_MAX_EDITS"], k) == 1024 < k["S2K_ALIGN_WAVES"] == 2048
    assert trace_waves(ALIGN_SPREAD, k) == k["S2K_ALIGN_WAVES"]  # without the pair at the bound the trace grid would not shrink


# ---- the alignment cases ------------------------------------------------------------------------------------------------------------------
ALIGN_PAIRS = 2 * pkg.ALIGN_WAVES + 1
ALIGN_CHECK_PAIRS = GRID + 1
ALIGN_SPREAD = 40   # the pairs beside the two at the bound: 0 .. about 40 edits
ALIGN_DISTINCT = 128


@functools.lru_cache(maxsize=None)
def align_case():
    """2 * S2K_ALIGN_WAVES + 1 pairs: pair 1 000 at distance exactly S2K_ALIGN_MAX_EDITS, pair 3 000 one above it (flagged), the others
    drawn from 128 distinct pairs of 60 .. 120 bases with 0 .. 40 random edits -> (pairs, the index of each pair's distinct pair)"""
    rng = np.random.default_rng(77)
    distinct = []
    for i in range(ALIGN_DISTINCT):
        q = ta.random_seq(rng, int(rng.integers(60, 121)))
        distinct.append((q, ta.mutated(rng, q, i * (ALIGN_SPREAD + 1) // ALIGN_DISTINCT)))
    distinct += [ta.spaced(rng, ta.MAX_EDITS, 0, gap=9), ta.spaced(rng, ta.MAX_EDITS + 1, 0, gap=9)]
    which = rng.integers(0, ALIGN_DISTINCT, size=ALIGN_PAIRS)
    which[1000], which[3000] = ALIGN_DISTINCT, ALIGN_DISTINCT + 1
    return distinct, which


def align_expected(distinct, which):
    """align_many_reference on the distinct pairs, carried to the pairs that repeat them: every per-pair field gathered, ops_off summed again"""
    ref = ta.align_many_reference(distinct)
    slots = np.diff(ref["ops_off"].astype(np.int64))[which]
    out = {f: ref[f][which] for f in ("edits", "flags", "n_ops", "matches")}
    out.update(ops_off=np.concatenate([[0], np.cumsum(slots)]).astype(np.uint64), ops=[ref["ops"][i] for i in which], res=[ref["res"][i] for i in which])
    return out


def test_align_case_and_its_replication():
    distinct, which = align_case()
    ref = ta.align_many_reference(distinct)
    assert ref["edits"][-2:].tolist() == [ta.MAX_EDITS, ta.MAX_EDITS + 1] and ref["flags"][-2:].tolist() == [0, ta.OVER]
    e = ref["edits"][:-2]
    assert e.min() == 0 and 30 <= e.max() <= ALIGN_SPREAD and len(set(e.tolist())) > 25 and not ref["flags"][:-2].any()
    sub = which[995:1005]
    _same(align_expected(distinct, sub), ta.align_many_reference([distinct[i] for i in sub]), "gathered")


# ---- GPU tier ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    e = pkg.Engine(0)
    yield e
    e.close()


def _big(name, R=None):
    """the call's component, R times, with the reference's result on it"""
    component, reference, expected, _ = FAMILIES[name]
    case = component()
    R = sizes()[name][0] if R is None else R
    return rp.CALLS[name][0](case, R), expected(reference(case), R, case), R


def _empty_last_unitig(off):
    off = off.copy()
    off[-2] = off[-1]
    return off


@pytest.mark.gpu
def test_device_simplify_mask_past_one_grid_pass(eng):
    big, want, R = _big("s2k_graph_simplify_mask")
    n_ids = len(big["ro"]) - 1
    assert GRID < n_ids <= GRID + len(mask_component()["ro"]) - 1 and want[1] > R and want[2] > R
    ts.device_mask(eng, big["ro"], big["d"], big["off"], big["cnt"], *MASK_BOUNDS["s2k_graph_simplify_mask"], want, ("simplify", R))


@pytest.mark.gpu
def test_device_simplify_check_refuses_in_the_second_pass(eng):
    """the last unitig of the last copy has no member: lane n_ids - 2 of the check, a second trip"""
    big, want, R = _big("s2k_graph_simplify_mask")
    assert len(big["ro"]) - 3 >= GRID
    s, a, b, c, rem = ts.raw_mask(eng, big["ro"], big["d"], _empty_last_unitig(big["off"]), big["cnt"], *MASK_BOUNDS["s2k_graph_simplify_mask"])
    assert (s, a, b, c) == (1, 0, 0, 0) and ts._marked(rem, np.uint8)


@pytest.mark.gpu
def test_device_bubble_mask_three_sources_a_wave(eng):
    """more sources than 2 * S2K_BUBBLE_WAVES: a wave of the bounded grid takes three, in both passes, and the second pass skips the
    sources without a bubble inside that loop; then the same on a context whose workspace is poisoned at every hand-out"""
    big, want, R = _big("s2k_graph_bubble_mask")
    assert 2 * pkg.BUBBLE_WAVES < want[1] <= 3 * pkg.BUBBLE_WAVES and want[2] > want[3] > 0 and want[4] > 0 and want[1] > want[2]
    mn, mb = MASK_BOUNDS["s2k_graph_bubble_mask"]
    tbu.device_bubble(eng, big["ro"], big["d"], big["off"], big["cnt"], mn, mb, want, ("bubble", R))
    os.environ["S2K_POISON_WS"] = str(0x5A)
    try:
        poisoned = pkg.Engine(0)
    finally:
        del os.environ["S2K_POISON_WS"]
    try:
        tbu.device_bubble(poisoned, big["ro"], big["d"], big["off"], big["cnt"], mn, mb, want, ("bubble, poisoned", R))
    finally:
        poisoned.close()


@pytest.mark.gpu
def test_device_spans_past_one_grid_pass(eng):
    """more steps than one pass: the edge support is added up in the second trip (the keys come from the tile kernels)"""
    import torch

    big, want, R = _big("s2k_paths_spans")
    n_steps, n, ne = len(big["paths"]["unitig"]), len(want["keys"]), len(big["d"])
    assert GRID < n_steps <= GRID + len(spans_component()["paths"]["unitig"])
    sup = torch.zeros(ne, dtype=torch.int64, device="cuda:0")
    s, nk, nf, no, keys = tsp.raw_spans(eng, big["paths"], big["ro"], big["d"], big["off"], capacity=n, support=sup)
    assert (s, nk, nf, no) == (0, n, want["n_followed"], want["n_off_graph"])
    assert keys[:n].tobytes() == want["keys"].tobytes() and tsp._marked(keys, n)
    assert sup.cpu().numpy().view(np.uint64).tobytes() == want["edge_support"].tobytes()


@pytest.mark.gpu
def test_device_spans_check_refuses_in_the_second_pass(eng):
    """more oriented unitigs than one pass; the last unitig of the last copy has no member"""
    import torch

    big, want, R = _big("s2k_paths_spans", sizes()["s2k_paths_spans, its check"][0])
    assert len(big["ro"]) - 3 >= GRID
    sup = torch.zeros(len(big["d"]), dtype=torch.int64, device="cuda:0")
    s, nk, nf, no, keys = tsp.raw_spans(eng, big["paths"], big["ro"], big["d"], _empty_last_unitig(big["off"]), capacity=len(want["keys"]), support=sup)
    assert (s, nk, nf, no) == (1, 0, 0, 0) and tsp._marked(keys) and not sup.any().item()
    big, want, R = _big("s2k_paths_spans", sizes()["s2k_paths_spans, its reads"][0])  # the read loop: a path offset that decreases in range
    paths, lane = _decreasing_path_off(big["paths"])
    assert lane >= GRID
    sup = torch.zeros(len(big["d"]), dtype=torch.int64, device="cuda:0")
    s, nk, nf, no, keys = tsp.raw_spans(eng, paths, big["ro"], big["d"], big["off"], capacity=len(want["keys"]), support=sup)
    assert (s, nk, nf, no) == (1, 0, 0, 0) and tsp._marked(keys) and not sup.any().item()


def _resolve(eng, big, **kw):
    return tsp.raw_resolve(eng, big["ro"], big["d"], big["T"], big["sk"], big["sc"], big["ms"], **kw)


@pytest.mark.gpu
def test_device_resolve_mask_past_one_grid_pass(eng):
    big, want, R = _big("s2k_graph_resolve_mask")
    T, ne = big["T"], len(big["d"])
    assert GRID < 2 * T <= GRID + 2 * resolve_component()["T"] and want[3] == R
    s, nc, nr, res, par = _resolve(eng, big)
    assert (s, nc, nr) == (0, want[2], want[3])
    assert res[:T].tobytes() == want[0].tobytes() and tsp._marked(res, T)
    assert par[:ne].tobytes() == want[1].tobytes() and tsp._marked(par, ne)
    s, nc, nr, res, par = _resolve(eng, big, null=("resolved", "partner"))
    assert (s, nc, nr) == (0, want[2], want[3]) and tsp._marked(res) and tsp._marked(par)


@pytest.mark.gpu
def test_device_resolve_check_refuses_in_the_second_pass(eng):
    """both loops of the check past one pass.  In the last copy: the offset behind the row of R+ one below the offset before it (it
    stays in range: whatever read through it would stay inside dst); then the last span key equal to the one before it"""
    big, want, R = _big("s2k_graph_resolve_mask", sizes()["s2k_graph_resolve_mask, its check"][0])
    assert len(big["sk"]) - 1 >= GRID and len(big["ro"]) - 1 - 2 * resolve_component()["T"] >= GRID

    def refused(**kw):
        s, nc, nr, res, par = _resolve(eng, dict(big, **kw))
        assert (s, nc, nr) == (1, 0, 0) and tsp._marked(res) and tsp._marked(par), list(kw)

    u = len(big["ro"]) - 1 - 2 * resolve_component()["T"] + 4  # R+ = 4 of the last copy: two out-edges, edges before it
    ro = big["ro"].copy()
    assert ro[u + 1] - ro[u] == 2 and ro[u] > 0
    ro[u + 1] = ro[u] - np.uint64(1)
    refused(ro=ro)
    sk = big["sk"].copy()
    sk[-1] = sk[-2]
    refused(sk=sk)
    s, nc, nr, res, par = _resolve(eng, big)  # nothing left behind
    assert (s, nc, nr) == (0, want[2], want[3]) and res[:big["T"]].tobytes() == want[0].tobytes()


@pytest.mark.gpu
def test_device_copy_places_past_one_grid_pass(eng):
    big, want, R = _big("s2k_unitig_copy_places")
    n = len(big["origin"])
    assert GRID < n <= GRID + len(copy_places_component()["origin"])
    s, got = tl.raw_copy_places(eng, big["outer"], big["origin"], big["inner"])
    assert s == 0 and got[:4 * n].tobytes() == want.tobytes() and tl._marked(got, 4 * n)


@pytest.mark.gpu
def test_device_copy_places_verify_refuses_in_the_second_pass(eng):
    """the last two pieces of the last contig name the same copy: every rule of the first check holds (the ids are in range), the
    permutation check finds it in its second trip.  A record written twice and one never would be all that follows from missing it."""
    big, want, R = _big("s2k_unitig_copy_places")
    outer = dict(big["outer"], members=big["outer"]["members"].copy())
    assert len(outer["members"]) - 2 >= GRID and outer["uni_off"][-1] - outer["uni_off"][-2] >= 2
    outer["members"][-1] = outer["members"][-2]
    s, got = tl.raw_copy_places(eng, outer, big["origin"], big["inner"])
    assert s == 1 and tl._marked(got)


@pytest.mark.gpu
def test_device_copy_places_check_refuses_in_the_second_pass(eng):
    """the two offset loops of the first check, each with enough copies of the component to take it past one pass: the last unitig
    without a member (its copies would get the length 0), then the last contig without a copy (no copy would look it up)"""
    for which in ("inner", "outer"):
        big, want, R = _big("s2k_unitig_copy_places", sizes()["s2k_unitig_copy_places, its %s offsets" % which][0])
        assert len(big[which]["uni_off"]) - 2 >= GRID
        bad = dict(big, **{which: dict(big[which], uni_off=_empty_last_unitig(big[which]["uni_off"]))})
        s, got = tl.raw_copy_places(eng, bad["outer"], bad["origin"], bad["inner"])
        assert s == 1 and tl._marked(got), which


@pytest.mark.gpu
def test_device_lift_past_one_grid_pass(eng):
    """more steps than one pass: contig_items is added up in the second trip of lift_items_kernel (the steps come from the tile kernels)"""
    big, want, R = _big("s2k_paths_lift")
    assert GRID < len(big["paths"]["unitig"]) <= GRID + len(lift_component()["paths"]["unitig"]) and want["n_dropped"] == R and want["n_conflicts"] == R
    s, t, got = tl.raw_lift(eng, big, capacity=want["n_steps"])
    assert (s, t) == (0, tuple(want[f] for f in tl.TOTALS))
    tl._same(got, want, big, ("lift", R), tl.ALL)


@pytest.mark.gpu
def test_device_lift_check_refuses_in_the_second_pass(eng):
    """the step loop: the last step of the last copy with count = 0.  The loop over the oriented unitigs (more copies: ten ids each): a
    row offset of the last copy that decreases and stays in range"""
    big, want, R = _big("s2k_paths_lift")
    assert len(big["paths"]["unitig"]) - 1 >= GRID

    def refused(case, **over):
        s, t, got = tl.raw_lift(eng, case, capacity=R * lift_component()["paths"]["unitig"].size, **over)
        assert (s, t) == (1, (0, 0, 0, 0)) and tl._untouched(got), list(over)

    count = big["paths"]["count"].copy()
    count[-1] = 0
    refused(big, paths=dict(big["paths"], count=count))
    big, want, R = _big("s2k_paths_lift", sizes()["s2k_paths_lift, its check"][0])
    ro, u = _decreasing_row(big["ro"], 2 * lift_component()["T"])
    assert u >= GRID
    refused(big, ro=ro)
    big, want, R = _big("s2k_paths_lift", sizes()["s2k_paths_lift, its reads"][0])  # the read loop: a path offset that decreases in range
    paths, lane = _decreasing_path_off(big["paths"])
    assert lane >= GRID
    refused(big, paths=paths)


def _decreasing_path_off(paths):
    """the paths with the offset before the last read one below the offset before it: it stays inside the steps, so a kernel that looked a read
    up through it would still stay inside the step arrays -> (the paths, the lane that finds it)"""
    po = paths["path_off"].copy()
    assert po[-3] > 0
    po[-2] = po[-3] - np.uint64(1)
    return dict(paths, path_off=po), len(po) - 3


def _decreasing_row(ro, n_ids0):
    """row_off with the offset behind the last row that has an edge set one below the offset before it -> (it, the row)"""
    u = int(np.nonzero(np.diff(ro.astype(np.int64)) > 0)[0][-1])
    assert u >= len(ro) - 1 - n_ids0
    assert ro[u + 1] > ro[u] > 0
    out = ro.copy()
    out[u + 1] = ro[u] - np.uint64(1)
    return out, u


@pytest.mark.gpu
def test_device_bridge_check_refuses_in_the_second_pass(eng):
    """s2k_paths_bridge writes through tile kernels; its check is a bounded grid.  The step loop: the last step of the last copy with
    count = 0; the loop over the oriented unitigs: a row offset of the last copy that decreases and stays in range"""
    def refused(case, **over):
        s, no, nm, nb, got = tbr.raw_bridge(eng, case, **over)
        assert (s, no, nm, nb) == (1, 0, 0, 0) and all(tbr._marked(x) for x in got.values()), list(over)

    big, want, R = _big("s2k_paths_bridge")
    assert len(big["paths"]["unitig"]) - 1 >= GRID
    count = big["paths"]["count"].copy()
    count[-1] = 0
    refused(big, paths=dict(big["paths"], count=count))
    big, want, R = _big("s2k_paths_bridge", sizes()["s2k_paths_bridge, its unitigs"][0])
    ro, u = _decreasing_row(big["ro"], len(tbr.hand_case()["ro"]) - 1)
    assert u >= GRID
    refused(big, ro=ro)
    big, want, R = _big("s2k_paths_bridge", sizes()["s2k_paths_bridge, its reads"][0])  # the read loop: a path offset that decreases in range
    paths, lane = _decreasing_path_off(big["paths"])
    assert lane >= GRID
    refused(big, paths=paths)


def raw_consensus_arrays(eng, pile, out_off, out, overlap, min_cov, capacity, keys=None, counts=None, held=None):
    """s2k_pileup_consensus (with keys: s2k_pileup_consensus_ex) on arrays as they are (test_pileup.raw_consensus packs Python lists; the
    argument order is test_pileup.consensus_args') ->
    (status, n_new_bases, stats, host arrays with guards).  held: a dict that keeps the planes, the draft and the overlaps on the device from
    one call to the next (the call only reads them)"""
    import ctypes

    import torch

    n, T = len(out), len(out_off) - 1
    held = {} if held is None else held
    if "planes" not in held:
        held.update(planes=[torch.from_numpy(np.ascontiguousarray(pile[f]).view(np.int32)).to("cuda:0") for f in tp.PLANES], out=ts._dev(out, np.uint8),
                    overlap=ts._dev(overlap, np.uint32))
    planes = held["planes"]
    p = pkg.Pile()
    p.match, p.del_, p.ins_long = planes[0].data_ptr(), planes[1].data_ptr(), planes[10].data_ptr()
    for c in range(4):
        p.sub[c], p.ins[c] = planes[2 + c].data_ptr(), planes[6 + c].data_ptr()
    d_off, d_out, d_ov = ts._dev(out_off, np.uint64), held["out"], held["overlap"]
    size = {"out_off": T + 1, "out": max(capacity, 1) + 15, "pos_map": n + 1, "overlap": 2 * T}
    res = {f: torch.full((size[f] + tp.GUARD,), tp.C_FILL[tp.C_OUT[f]], dtype=getattr(torch, tp.C_T[tp.C_OUT[f]]), device="cuda:0") for f in size}
    nn = ctypes.c_uint64(777)
    st = (ctypes.c_uint64 * pkg.CONSENSUS_STATS_WORDS)(*([777] * pkg.CONSENSUS_STATS_WORDS))
    torch.cuda.synchronize()
    args = (eng.ctx,) + tp.consensus_args(ctypes.byref(p), ts._ptr(d_off), ts._ptr(d_out), n, ts._ptr(d_ov), T, min_cov, lambda f: ts._ptr(res[f]), capacity,
                                          ctypes.byref(nn), st)
    if keys is None:
        s = eng.lib.s2k_pileup_consensus(*args)
    else:
        d_k, d_c = ts._dev(keys, np.uint64), ts._dev(counts, np.uint32)
        s = eng.lib.s2k_pileup_consensus_ex(*args, ts._ptr(d_k), ts._ptr(d_c), len(keys))
    torch.cuda.synchronize()
    return s, nn.value, list(st), {f: ts._host(x, tp.C_OUT[f]) for f, x in res.items()}


@pytest.mark.gpu
def test_device_consensus_past_one_grid_pass_and_the_scan_seam(eng):
    """more draft bases than SCAN_SEAM and more unitigs than one pass: the call, write and unit kernels take later trips, and pos_map
    comes from a scan whose block sums fill more than one chunk of 1024, so that the carry between the chunks is in every offset
    behind the seam.  Then the check's second trip: an offset of the last copy that decreases and stays in range."""
    case = consensus_component()
    R = sizes()["s2k_pileup_consensus"][0]
    want = rp.consensus_expected(consensus_reference(case), R)
    d_off, d_out = tp.draft_of(case["strings"])
    out_off, out, pile, overlap = rp.offsets(d_off, R), rp.tiled(d_out, R), {f: rp.tiled(v, R) for f, v in case["pile"].items()}, rp.tiled(case["overlap"], R)
    n, T, m = len(out), len(out_off) - 1, len(want["out"])
    assert SCAN_SEAM < n <= SCAN_SEAM + len(d_out) and T > GRID and m > SCAN_SEAM // 2
    held = {}
    s, nn, st, got = raw_consensus_arrays(eng, pile, out_off, out, overlap, case["min_cov"], m, held=held)
    assert (s, nn, st) == (0, m, [want["stats"][f] for f in tp.C_STATS] + [0] * 3), (s, nn, m, st)
    for f, k in (("out_off", T + 1), ("out", m), ("pos_map", n + 1), ("overlap", 2 * T)):
        assert got[f][:k].tobytes() == want[f].tobytes(), (f, np.nonzero(got[f][:k] != want[f])[0][:8])
        assert tp._cmarked(got[f], k), (f, "guard")
    bad = out_off.copy()
    assert bad[-3] > 0
    bad[-2] = bad[-3] - np.uint64(1)
    s, nn, st, got = raw_consensus_arrays(eng, pile, bad, out, overlap, case["min_cov"], m, held=held)
    assert (s, nn, st) == (1, 0, [0] * 8) and all(tp._cmarked(x) for x in got.values())


@pytest.mark.gpu
def test_device_consensus_ex_past_one_grid_pass_and_the_scan_seam(eng):
    """the same draft with a table of long insertions of more keys than one pass: every copy's keys are those of its own positions (the
    bit-reversed p + c * n_bases, sorted), the called candidates' letters are in the output and in pos_map.  Then cs_keys_kernel's second
    trip: the last key equal to the one before it."""
    case = consensus_ex_component()
    R = sizes()["s2k_pileup_consensus"][0]
    want = rp.consensus_expected(consensus_ex_reference(case), R)
    d_off, d_out = tp.draft_of(case["strings"])
    out_off, out, pile, overlap = rp.offsets(d_off, R), rp.tiled(d_out, R), {f: rp.tiled(v, R) for f, v in case["pile"].items()}, rp.tiled(case["overlap"], R)
    big = rp.consensus_ex_inputs(dict(case, pile={}, strings=[b"x" * len(d_out)]), R)  # the table alone: the planes are tiled above
    keys, counts = big["keys"], big["counts"]
    n, T, m = len(out), len(out_off) - 1, len(want["out"])
    assert SCAN_SEAM < n and len(keys) > GRID and (keys[1:] > keys[:-1]).all() and want["stats"]["n_ins_long"] >= R
    held = {}
    s, nn, st, got = raw_consensus_arrays(eng, pile, out_off, out, overlap, case["min_cov"], m, keys, counts, held=held)
    assert (s, nn, st) == (0, m, [want["stats"][f] for f in tpl.C_LONG_STATS] + [0]), (s, nn, m, st)
    for f, k in (("out_off", T + 1), ("out", m), ("pos_map", n + 1), ("overlap", 2 * T)):
        assert got[f][:k].tobytes() == want[f].tobytes(), (f, np.nonzero(got[f][:k] != want[f])[0][:8])
        assert tp._cmarked(got[f], k), (f, "guard")
    bad = keys.copy()
    bad[-1] = bad[-2]
    s, nn, st, got = raw_consensus_arrays(eng, pile, out_off, out, overlap, case["min_cov"], m, bad, counts, held=held)
    assert (s, nn, st) == (1, 0, [0] * 8) and all(tp._cmarked(x) for x in got.values())


@pytest.mark.gpu
def test_device_segments_past_one_grid_pass(eng):
    """more walks, source steps and segments than one pass: sg_steps, sg_off and sg_segments take later trips with their counters"""
    case = segments_component()
    R = sizes()["s2k_walks_segments"][0]
    want = rp.segments_expected(segments_reference(case), R, rp.query_span(case), int(case["tgt_off"][-1]))
    big = rp.segments_inputs(case, R)
    nw, n = len(big["bad"]), len(want["q_begin"])
    assert min(nw, len(big["src"]["pos"]), n) > GRID and want["stats"][1] >= R
    s, total, st, got = tas.raw_segments(eng, big, capacity=n)
    assert (s, total, st) == (0, n, want["stats"]), (s, total, st)
    tas.assert_segments(got, want, nw, ("segments", R))


@pytest.mark.gpu
def test_device_segments_check_refuses_in_the_second_pass(eng):
    """sg_check_kernel's own loops, one malformed entry of the last copy each.  At the R of the result loops, where reads and nodes pass
    one pass too: a source read offset that decreases in range; a km_off that decreases in range (km_off[R] + item stays inside the
    items); the last member's base offset one past its unitig's bases (the call only computes with member_off: it gives coordinates and
    reads no base).  With more unitigs than one pass (one walk a copy): an out_off that decreases in range.  The walk loop's rules --
    qstart above qend, the target offsets -- size later loops, so none of theirs is planted; walk_off and the steps go through
    path_off_ok and steps_ok, whose later trips the spans, lift, bridge and walks checks pin"""
    def refused(big, **over):
        s, total, st, got = tas.raw_segments(eng, big, capacity=1, **over)
        assert (s, total, st) == (1, 0, [0] * 5) and all(tas._marked(x) for x in got.values()), list(over)

    big = rp.segments_inputs(segments_component(), sizes()["s2k_walks_segments"][0])
    po, lane = _decreasing_path_off({"path_off": big["src"]["path_off"]})
    assert lane >= GRID
    refused(big, src_path_off=po["path_off"])
    km, lane = _decreasing_path_off({"path_off": big["km_off"]})
    assert lane >= GRID
    refused(big, km_off=km["path_off"])
    mo = big["mo"]["member_off"].copy()
    assert len(mo) - 1 >= GRID
    mo[-1] = big["mo"]["out_off"][-1] + np.uint64(1)
    refused(big, member_off=mo)
    big = rp.segments_inputs(segments_one_walk(), sizes()["s2k_walks_segments, its unitigs"][0])
    oo, lane = _decreasing_path_off({"path_off": big["mo"]["out_off"]})
    assert lane >= GRID
    refused(big, out_off=oo["path_off"])


@pytest.mark.gpu
def test_device_join_past_one_grid_pass(eng):
    """more walks, segments and joined runs than one pass: jn_over, jn_lens, jn_walks and jn_ops take later trips.  Then the two loops of the
    check: the last segment with n_ops above its slots; the segment offset before the last walk one below the offset before it"""
    case = join_component()
    R = sizes()["s2k_align_join"][0]
    want = rp.join_expected(dict(join_reference(case), ops=[join_reference(case)["ops"]]), R)
    big = rp.join_arrays(tas.flat_segments(case["seg"]), case["seg_off"], case["bad"], R)
    nw, ns, n = len(big["bad"]), len(big["edits"]), len(want["ops"])
    assert min(nw, ns, n) > GRID
    seg = {f: big[f] for f in ("edits", "flags", "n_ops", "matches", "ops_off", "ops")}

    def call(capacity=n, seg_off=big["seg_off"], **over):
        return tas.raw_join(eng, seg_off, big["bad"], case["seg"], capacity=capacity, n_walks=nw, n_segments=ns, n_runs=len(big["ops"]), **dict(seg, **over))

    s, nb, got = call()
    assert (s, nb) == (0, n)
    for f in ("edits", "flags", "n_ops", "matches"):
        assert got[f][:nw].tobytes() == want[f].tobytes() and tas._marked(got[f], nw), f
    assert got["ops_off"][:nw + 1].tobytes() == want["ops_off"].tobytes() and tas._marked(got["ops_off"], nw + 1)
    assert got["ops"][:n].tobytes() == want["ops"].tobytes() and tas._marked(got["ops"], n)
    n_ops = big["n_ops"].copy()
    n_ops[-1] = np.uint32(int(big["ops_off"][-1] - big["ops_off"][-2]) + 1)
    so = big["seg_off"].copy()
    assert so[-3] > 0
    so[-2] = so[-3] - np.uint64(1)
    for over in (dict(n_ops=n_ops), dict(seg_off=so)):
        s, nb, got = call(**over)
        assert (s, nb) == (1, 0) and all(tas._marked(x) for x in got.values()), list(over)


@pytest.mark.gpu
def test_device_walks_check_refuses_in_the_second_pass(eng):
    """s2k_paths_walks writes through tile kernels; its check is a bounded grid.  The step loop: the last step of the last copy with
    count = 0; the loop over the oriented unitigs: a row offset of the last copy that decreases and stays in range"""
    def refused(case, **over):
        s, nw, nf, no, got = twk.raw_walks(eng, case, **over)
        assert (s, nw, nf, no) == (1, 0, 0, 0) and all(twk._marked(x) for x in got.values()), list(over)

    big, want, R = _big("s2k_paths_walks")
    assert len(big["paths"]["unitig"]) - 1 >= GRID
    count = big["paths"]["count"].copy()
    count[-1] = 0
    refused(big, paths=dict(big["paths"], count=count))
    big, want, R = _big("s2k_paths_walks", sizes()["s2k_paths_walks, its unitigs"][0])
    ro, u = _decreasing_row(big["ro"], len(twk.hand_case()["ro"]) - 1)
    assert u >= GRID
    refused(big, ro=ro)
    big, want, R = _big("s2k_paths_walks", sizes()["s2k_paths_walks, its reads"][0])  # the read loop: a path offset that decreases in range
    paths, lane = _decreasing_path_off(big["paths"])
    assert lane >= GRID
    refused(big, paths=paths)
    # the node loop: the last member's base offset one past its unitig's bases.  s2k_paths_walks only computes with member_off (the
    # intervals of s2k_coords_dev.h go into path_start, path_end and path_len as numbers): no index is made from it
    big, want, R = _big("s2k_paths_walks", sizes()["s2k_paths_walks, its nodes"][0])
    mo = big["mo"]["member_off"].copy()
    assert len(mo) - 1 >= GRID
    mo[-1] = big["mo"]["out_off"][-1] + np.uint64(1)
    refused(big, member_off=mo)


@pytest.mark.gpu
def test_device_targets_check_refuses_in_the_second_pass(eng):
    """more unitigs than one pass (the pile-up and the segment calls launch the same check): the offset before the last unitig one below
    the offset before it.  Every base the offsets name stays inside the draft, which is passed whole."""
    big, want, R = _big("s2k_walks_targets", sizes()["s2k_walks_targets, its unitigs"][0])
    off = np.concatenate([[0], np.cumsum(np.tile([len(x) for x in targets_component()["strings"]], R))]).astype(np.uint64)
    assert len(off) - 3 >= GRID and off[-3] > 0 and len(off) - 1 == len(big["strings"])
    off[-2] = off[-3] - np.uint64(1)
    s, nb, got = ta.raw_targets(eng, big["walks"], big["su"], big["strings"], big["overlap"], capacity=len(want[1]), out_off=off)
    assert (s, nb) == (1, 0) and all(ta._marked(x) for x in got.values())


def raw_pileup_arrays(eng, a, max_shift, key_capacity=None):
    """s2k_walks_pileup (with key_capacity: s2k_walks_pileup_ex) on arrays as they are (test_pileup.raw_pileup packs Python lists), zeroed
    planes with guards -> (status, stats, host planes with guards[, n_candidates, n_long_keys, host keys with guards])"""
    import ctypes

    import torch

    dt = {"first_step": np.uint64, "n_steps": np.uint32, "path_start": np.uint64, "path_end": np.uint64, "flags": np.uint32, "unitig": np.uint32,
          "out_off": np.uint64, "out": np.uint8, "overlap": np.uint32, "query": np.uint8, "q_begin": np.uint64, "aflags": np.uint32, "ops_off": np.uint64,
          "n_ops": np.uint32, "ops": np.uint32}
    dv = {k: ts._dev(a[k], t) for k, t in dt.items()}
    planes, p = tp.device_pile(len(a["out"]))
    st = (ctypes.c_uint64 * pkg.PILEUP_STATS_WORDS)(*([777] * pkg.PILEUP_STATS_WORDS))
    P = lambda k: ts._ptr(dv[k])  # noqa: E731
    torch.cuda.synchronize()
    args = (eng.ctx,) + tp.pileup_args(P, len(a["first_step"]), len(a["unitig"]), len(a["out"]), len(a["out_off"]) - 1, len(a["query"]), len(a["ops"]), max_shift,
                                       ctypes.byref(p), st)
    if key_capacity is None:
        s = eng.lib.s2k_walks_pileup(*args)
        torch.cuda.synchronize()
        return s, list(st), {f: ts._host(t, np.uint32) for f, t in zip(tp.PLANES, planes)}
    kbuf = torch.full((key_capacity + tp.GUARD,), -0x5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    nc, nk = ctypes.c_uint64(777), ctypes.c_uint64(777)
    s = eng.lib.s2k_walks_pileup_ex(*args, ts._ptr(kbuf), key_capacity, ctypes.byref(nc), ctypes.byref(nk))
    torch.cuda.synchronize()
    return s, list(st), {f: ts._host(t, np.uint32) for f, t in zip(tp.PLANES, planes)}, nc.value, nk.value, ts._host(kbuf, np.uint64)


@pytest.mark.gpu
def test_device_pileup_past_one_grid_pass_and_the_scan_seam(eng):
    """more draft bases than SCAN_SEAM, and so more walks and run slots than one pass: the slot, walk and vote kernels take later trips
    with their counters, and the two difference planes of the = and D pieces are scanned across the seam before pl_apply_kernel adds
    them to match and del.  All eleven planes are compared.  Then pl_offsets_kernel's second trip: the last walk with n_ops above its
    slots (no run is read before the check has passed)."""
    case = pileup_component()
    R = sizes()["s2k_walks_pileup"][0]
    want, wst = rp.pileup_expected(pileup_reference(case), R)
    big = rp.pileup_arrays(pileup_arrays(case), R)
    n = len(big["out"])
    assert SCAN_SEAM < n <= SCAN_SEAM + 70 and len(big["first_step"]) > GRID and len(big["ops"]) > GRID
    s, st, got = raw_pileup_arrays(eng, big, case["max_shift"])
    assert s == 0 and st[:len(tp.P_STATS)] == [wst[f] for f in tp.P_STATS], (s, st)
    tp.assert_pile(got, want, n, ("pile-up", R))
    # with a key buffer: the same planes and stats, and every copy's vote keys in run-slot order (pl_vote_kernel<.., true>, pl_keys_kernel)
    wkeys, wcand = rp.pileup_ex_expected(pileup_ex_reference(case), R, 70)
    assert len(wkeys) >= R and wcand >= R
    s, st, got, nc, nk, keys = raw_pileup_arrays(eng, big, case["max_shift"], key_capacity=wcand)
    assert (s, nc, nk) == (0, wcand, len(wkeys)) and st[:len(tp.P_STATS)] == [wst[f] for f in tp.P_STATS], (s, nc, nk, st)
    tp.assert_pile(got, want, n, ("pile-up with keys", R))
    assert keys[:nk].tobytes() == wkeys.tobytes() and (keys[nk:] == tpl.KMARK).all()
    bad = dict(big, n_ops=big["n_ops"].copy())
    assert big["aflags"][-1] == 0
    bad["n_ops"][-1] = np.uint32(int(big["ops_off"][-1] - big["ops_off"][-2]) + 1)
    s, st, got = raw_pileup_arrays(eng, bad, case["max_shift"])
    assert s == 1 and st == [0] * len(st) and all((got[f][:n] == 0).all() and (got[f][n:] == tp.MARK32).all() for f in tp.PLANES)


@pytest.mark.gpu
def test_device_align_trace_under_its_budget(eng):
    """2 * S2K_ALIGN_WAVES + 1 pairs at the default max_edits = S2K_ALIGN_MAX_EDITS = 255, one of them at distance exactly 255: the score
    pass runs S2K_ALIGN_WAVES = 2048 waves; the trace needs 4 (emax + 1)^2 = 4 * 256^2 = 262 144 B a wave, AL_TRACE_BUDGET = 256 MiB
    admits 2^28 / 2^18 = 1024 of them, so the trace grid is half the score grid and the trace's waves, which draw their pairs from one counter as the score's do, take more pairs each.  One pair
    is one edit over the bound (flagged, no runs), the others spread over 0 .. 40 edits."""
    distinct, which = align_case()
    pairs = [distinct[i] for i in which]
    ref = align_expected(distinct, which)
    assert len(pairs) == ALIGN_PAIRS and ref["edits"][1000] == ta.MAX_EDITS and (ref["edits"][3000], ref["flags"][3000]) == (ta.MAX_EDITS + 1, ta.OVER)
    q, t, ivs = ta.pools_of(pairs)
    bound = int(ref["ops_off"][-1])
    s, nb, got = ta.raw_align(eng, q, t, ivs, capacity=bound)
    assert (s, nb) == (0, bound)
    ta.assert_aligned(got, ref, len(pairs), "trace under its budget")


@pytest.mark.gpu
def test_device_align_check_refuses_in_the_second_pass(eng):
    """GRID + 1 pairs over one pool of eight bases; the last pair's query ends at byte 8 of a pool that is said to hold 7 (the
    allocation holds all 8: an interval the check let through would still be read inside it)"""
    n = ALIGN_CHECK_PAIRS
    pool = np.frombuffer(b"ACGTACGA", dtype=np.uint8)
    ivs = [np.zeros(n, dtype=np.uint64), np.full(n, 4, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.full(n, 4, dtype=np.uint64)]
    ivs[0][-1], ivs[1][-1] = 4, 8
    s, nb, got = ta.raw_align(eng, pool, pool, ivs, capacity=n, nq=7)
    assert (s, nb) == (1, 0) and all(ta._marked(x) for x in got.values())
