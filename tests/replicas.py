"""R disjoint copies of a small case, for the tests that take a grid-stride launch past its bounded grid (test_grid_bounds.py).

Every call on the graph and path side is local to a connected component, and every tie-break in it ("the smallest source", "the
smaller id") keeps its order when all ids move by one offset.  So what a call gives on R disjoint copies of a case is what it gives on
the case, repeated, with the same offsets: ids gain c * n_ids in copy c, edge indices c * n_edges, offsets the totals of the copies
before, NONE stays NONE, per-read coordinates stay, totals are multiplied by R.  A Python reference cannot walk a million ids in a
test's time; it can walk the case, and `replicate_expected` carries its result to the R copies.  That the two commute --
reference(replicate_inputs(case, 3)) == replicate_expected(reference(case), 3), field by field -- is asserted on the CPU for every call.

All of it is numpy without a loop over the copies.  For a call NAME: CALLS[NAME] = (replicate_inputs, replicate_expected)."""
import numpy as np

NONE = 0xFFFFFFFF


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
def tiled(a, R):
    """the array as it is, R times"""
    return np.tile(np.asarray(a), R)


def shifted(a, R, step, keep=None):
    """R copies of an id array, copy c's entries + c * step; entries equal to `keep` (NONE) stay"""
    a = np.asarray(a)
    wide = a.astype(np.uint64)[None, :] + (np.arange(R, dtype=np.uint64) * np.uint64(step))[:, None]
    if keep is not None:
        wide = np.where((a == keep)[None, :], np.uint64(keep), wide)
    assert len(a) == 0 or int(wide.max()) <= np.iinfo(a.dtype).max
    return wide.astype(a.dtype).ravel()


def offsets(off, R):
    """R copies of an offset array of n + 1 entries that starts at 0 -> R n + 1 entries, copy c's + c * off[-1]"""
    off = np.asarray(off)
    assert int(off[0]) == 0
    return np.concatenate([shifted(off[:-1], R, int(off[-1])), np.array([R * int(off[-1])], dtype=off.dtype)])


def keys32(keys, R, hi_step, lo_step):
    """R copies of 64-bit keys that hold two 32-bit indices: the upper one gains c * hi_step, the lower one c * lo_step"""
    return shifted(np.asarray(keys, dtype=np.uint64), R, (int(hi_step) << 32) + int(lo_step))


def csr(ro, d, R):
    """R copies of a CSR over oriented ids: (row_off, dst)"""
    return offsets(ro, R), shifted(d, R, len(ro) - 1)


# ---- s2k_graph_simplify_mask and s2k_graph_bubble_mask: case = dict ro, d, off, cnt and the two bounds --------------------------------
def mask_inputs(case, R):
    ro, d = csr(case["ro"], case["d"], R)
    return dict(case, ro=ro, d=d, off=offsets(case["off"], R), cnt=tiled(case["cnt"], R))


def mask_expected(ref, R):
    """(remove, totals ...) of simplify_reference or bubble_reference"""
    return (tiled(ref[0], R),) + tuple(R * int(x) for x in ref[1:])


# ---- s2k_paths_spans: case = dict paths (path_off, unitig, pos, count, flags), ro, d, off ------------------------------------------------
def paths_inputs(paths, R, n_ids):
    """a path dict: the steps' oriented unitigs move, path_off goes on, every other step array (pos, count, flags, item, start, end) stays"""
    out = {f: tiled(v, R) for f, v in paths.items() if f not in ("path_off", "unitig")}
    out.update(path_off=offsets(paths["path_off"], R), unitig=shifted(paths["unitig"], R, n_ids))
    return out


def spans_inputs(case, R):
    ro, d = csr(case["ro"], case["d"], R)
    return dict(case, paths=paths_inputs(case["paths"], R, len(case["ro"]) - 1), ro=ro, d=d, off=offsets(case["off"], R))


def spans_expected(ref, R, n_edges):
    out = {f: R * ref[f] for f in ("n_followed", "n_off_graph", "n_linked")}
    out.update(keys=keys32(ref["keys"], R, n_edges, n_edges), edge_support=tiled(ref["edge_support"], R))
    return out


# ---- s2k_graph_resolve_mask: case = dict ro, d, T, sk, sc, ms --------------------------------------------------------------------------------
def resolve_inputs(case, R):
    ro, d = csr(case["ro"], case["d"], R)
    ne = len(case["d"])
    return dict(case, ro=ro, d=d, T=R * case["T"], sk=keys32(case["sk"], R, ne, ne), sc=tiled(case["sc"], R))


def resolve_expected(ref, R, n_edges):
    """(resolved, partner, n_candidates, n_resolved) of resolve_reference"""
    return tiled(ref[0], R), shifted(ref[1], R, n_edges, keep=NONE), R * ref[2], R * ref[3]


# ---- s2k_unitig_copy_places: case = dict outer (uni_off, members, circular over the copies), origin, inner (uni_off, circular) ---------------
def places(place, R, n_contigs):
    """R copies of copy records (pkg.NodePlace): the oriented contig moves, pos, len and circular stay"""
    out = np.tile(place, R)
    out["unitig"] = shifted(place["unitig"], R, 2 * n_contigs)
    return out


def copy_places_inputs(case, R):
    outer, inner, n_copies = case["outer"], case["inner"], len(case["origin"])
    return {"outer": {"uni_off": offsets(outer["uni_off"], R), "members": shifted(outer["members"], R, 2 * n_copies), "circular": tiled(outer["circular"], R)},
            "origin": shifted(case["origin"], R, len(inner["circular"])),
            "inner": {"uni_off": offsets(inner["uni_off"], R), "circular": tiled(inner["circular"], R)}}


def copy_places_expected(ref, R, n_contigs):
    return places(ref, R, n_contigs)


# ---- s2k_paths_lift: case = the dict of test_lift.lift_case ---------------------------------------------------------------------------------
def lift_inputs(case, R):
    ro, d = csr(case["ro"], case["d"], R)
    assert case.get("matched_in") is None
    return {"paths": paths_inputs(case["paths"], R, len(case["ro"]) - 1), "matched_in": None, "ro": ro, "d": d, "uni_off": offsets(case["uni_off"], R),
            "circular": tiled(case["circular"], R), "T": R * case["T"], "resolved": tiled(case["resolved"], R),
            "partner": shifted(case["partner"], R, len(case["d"]), keep=NONE), "copy_off": offsets(case["copy_off"], R),
            "place": places(case["place"], R, case["n_contigs"]), "n_copies": R * case["n_copies"], "n_contigs": R * case["n_contigs"]}


def lift_expected(ref, R, n_copies, n_contigs):
    """lift_reference's dict: the output steps' oriented contigs and the copies move; a dropped step's NONE stays"""
    out = {f: tiled(ref[f], R) for f in ("pos", "count", "item", "flags", "start", "end", "matched", "join", "Q", "contig_items")}
    out.update({f: R * ref[f] for f in ("n_steps", "n_merged", "n_dropped", "n_conflicts")})
    out.update(unitig=shifted(ref["unitig"], R, 2 * n_contigs), V=shifted(ref["V"], R, 2 * n_contigs, keep=NONE),
               step_copy=shifted(ref["step_copy"], R, n_copies, keep=NONE), path_off=offsets(ref["path_off"], R))
    return out


# ---- s2k_paths_bridge: case = dict paths (with item, start, end), ro, d, uni_off, circular -----------------------------------------------------
def bridge_inputs(case, R):
    ro, d = csr(case["ro"], case["d"], R)
    return dict(case, paths=paths_inputs(case["paths"], R, len(case["ro"]) - 1), ro=ro, d=d, uni_off=offsets(case["uni_off"], R),
                circular=tiled(case["circular"], R))


def bridge_expected(ref, R, n_ids):
    """bridge_reference's dict: the output steps stay on their (moved) oriented unitigs"""
    out = {f: tiled(ref[f], R) for f in ("pos", "count", "item", "flags", "start", "end", "matched", "join")}
    out.update({f: R * ref[f] for f in ("n_steps", "n_merged", "n_bridged")})
    out.update(unitig=shifted(ref["unitig"], R, n_ids), path_off=offsets(ref["path_off"], R))
    return out


# ---- s2k_pileup_consensus: case = dict pile (the eleven planes), strings, overlap, min_cov -----------------------------------------------------
def consensus_inputs(case, R):
    """the draft bases are concatenated (the strings repeat), the planes and the overlaps with them"""
    return dict(case, pile={f: tiled(v, R) for f, v in case["pile"].items()}, strings=list(case["strings"]) * R, overlap=tiled(case["overlap"], R))


def consensus_expected(ref, R):
    """consensus_reference's dict: pos_map and the new offsets gain the copy's polished length, not its draft length"""
    return {"strings": list(ref["strings"]) * R, "out_off": offsets(ref["out_off"], R), "out": tiled(ref["out"], R), "pos_map": offsets(ref["pos_map"], R),
            "overlap": tiled(ref["overlap"], R), "stats": {f: R * v for f, v in ref["stats"].items()}}


# ---- s2k_paths_walks: case = dict paths (with start, end), ro, d, uni (uni_off, members, circular), mo (member_off, out_off, overlap), nodes --
def walks_inputs(case, R):
    """the members' oriented nodes move by 2 * n_nodes, their base offsets by the copy's bases; seq_len repeats with the nodes"""
    ro, d = csr(case["ro"], case["d"], R)
    uni, mo, n_nodes = case["uni"], case["mo"], len(case["uni"]["members"])
    assert len(mo["member_off"]) == n_nodes and len(case["nodes"]["seq_len"]) == n_nodes
    return {"paths": paths_inputs(case["paths"], R, len(case["ro"]) - 1), "ro": ro, "d": d,
            "uni": {"uni_off": offsets(uni["uni_off"], R), "members": shifted(uni["members"], R, 2 * n_nodes), "circular": tiled(uni["circular"], R)},
            "mo": {"member_off": shifted(mo["member_off"], R, int(mo["out_off"][-1])), "out_off": offsets(mo["out_off"], R), "overlap": tiled(mo["overlap"], R)},
            "nodes": {"seq_len": tiled(case["nodes"]["seq_len"], R)}}


def walks_expected(ref, R, n_steps, n_edges):
    """walks_reference's dict: a walk's first step and the steps' edges move; its coordinates are its own"""
    out = {f: tiled(ref[f], R) for f in ("n_steps", "items", "qstart", "qend", "flags", "path_len", "path_start", "path_end")}
    out.update({f: R * ref[f] for f in ("n_walks", "n_followed", "n_off_graph")})
    out.update(first_step=shifted(ref["first_step"], R, n_steps), walk_off=offsets(ref["walk_off"], R), edge=shifted(ref["edge"], R, n_edges, keep=NONE))
    return out


# ---- s2k_walks_targets: case = dict walks (first_step, n_steps, path_start, path_end, flags), su, strings, overlap ------------------------------
def walk_records(walks, R, n_all_steps):
    """walk records: the first step moves, the coordinates along the walk's own path stay"""
    out = {f: tiled(walks[f], R) for f in ("n_steps", "path_start", "path_end", "flags")}
    out["first_step"] = shifted(walks["first_step"], R, n_all_steps)
    return out


def targets_inputs(case, R):
    return {"walks": walk_records(case["walks"], R, len(case["su"])), "su": shifted(case["su"], R, 2 * len(case["strings"])),
            "strings": list(case["strings"]) * R, "overlap": tiled(case["overlap"], R)}


def targets_expected(ref, R):
    """(tgt_off, tgt bytes, bad) of targets_reference"""
    return offsets(ref[0], R), ref[1] * R, tiled(ref[2], R)


# ---- s2k_walks_pileup: case = dict walks, su, strings, overlap, queries, flags, runs (lists, as pileup_reference takes them), max_shift ------
def pileup_inputs(case, R):
    """the case as the reference takes it: the lists repeat, the steps' unitigs and the walks' first steps move"""
    t = targets_inputs(case, R)
    return dict(case, walks=t["walks"], su=t["su"], strings=t["strings"], overlap=t["overlap"], queries=list(case["queries"]) * R,
                flags=tiled(case["flags"], R), runs=list(case["runs"]) * R)


def pileup_arrays(arr, R):
    """the same case as the arrays the call takes (first_step .. flags of the walks, unitig, out_off, out, overlap, query, q_begin,
    aflags, ops_off, n_ops, ops), R times: read and draft bases are concatenated, q_begin gains the copy's query bytes, ops_off its slots"""
    out = {f: tiled(arr[f], R) for f in ("n_steps", "path_start", "path_end", "flags", "out", "overlap", "query", "aflags", "n_ops", "ops")}
    out.update(first_step=shifted(arr["first_step"], R, len(arr["unitig"])), unitig=shifted(arr["unitig"], R, 2 * (len(arr["out_off"]) - 1)),
               out_off=offsets(arr["out_off"], R), q_begin=shifted(arr["q_begin"], R, len(arr["query"])), ops_off=offsets(arr["ops_off"], R))
    return out


def pileup_expected(ref, R):
    """(the eleven planes, the stats) of pileup_reference"""
    return {f: tiled(v, R) for f, v in ref[0].items()}, {f: R * v for f, v in ref[1].items()}


# ---- long-insertion vote keys (include/s2k.h): bits 63 .. 28 hold the bit-reversed 36-bit draft position, the rest length and letters ----------
def rev36(x):
    """the 36-bit reversal of every entry of a uint64 array: the 64 bits reversed by swapping halves of halves, then the top 36 kept"""
    x = np.asarray(x, dtype=np.uint64).copy()
    for sh, m in ((1, 0x5555555555555555), (2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> np.uint64(sh)) & np.uint64(m)) | ((x & np.uint64(m)) << np.uint64(sh))
    return ((x >> np.uint64(32)) | (x << np.uint64(32))) >> np.uint64(28)


def long_keys(keys, R, n_bases):
    """R copies of vote keys, copy c's for position p + c * n_bases: not affine, the position is recomputed and reversed again -> copy by
    copy in the order given (the table wants them sorted: consensus_ex_inputs)"""
    keys = np.asarray(keys, dtype=np.uint64)
    pos = rev36(keys >> np.uint64(28))
    assert len(keys) == 0 or (int(pos.max()) < n_bases and R * n_bases < 1 << 36)
    wide = pos[None, :] + (np.arange(R, dtype=np.uint64) * np.uint64(n_bases))[:, None]
    return (rev36(wide) << np.uint64(28) | (keys & np.uint64((1 << 28) - 1))[None, :]).ravel()


# ---- s2k_pileup_consensus_ex: the consensus case with keys (ascending) and counts ---------------------------------------------------------------
def consensus_ex_inputs(case, R):
    k = long_keys(case["keys"], R, sum(len(x) for x in case["strings"]))
    order = np.argsort(k, kind="stable")
    return dict(consensus_inputs(case, R), keys=k[order], counts=tiled(case["counts"], R)[order])


def pileup_ex_expected(ref, R, n_bases):
    """(keys in run-slot order, n_candidates) of long_keys_reference"""
    return long_keys(ref[0], R, n_bases), R * ref[1]


# ---- s2k_align_join: case = dict seg_off, bad, seg (align_many_reference's dict over the segments) ---------------------------------------------
def join_inputs(case, R):
    """the case as join_reference takes it: the walks' segment offsets go on, the segments repeat"""
    seg = case["seg"]
    big = {f: tiled(seg[f], R) for f in ("edits", "flags", "n_ops", "matches")}
    big.update(ops_off=offsets(seg["ops_off"], R), ops=list(seg["ops"]) * R)
    return {"seg_off": offsets(np.asarray(case["seg_off"], dtype=np.uint64), R), "bad": tiled(np.asarray(case["bad"], dtype=np.uint8), R), "seg": big}


def join_arrays(flat, seg_off, bad, R):
    """the same as the arrays the call takes, from the flat run array of one copy (junk behind a segment's runs included)"""
    out = {f: tiled(flat[f], R) for f in ("edits", "flags", "n_ops", "matches", "ops")}
    out.update(ops_off=offsets(flat["ops_off"], R), seg_off=offsets(np.asarray(seg_off, dtype=np.uint64), R), bad=tiled(np.asarray(bad, dtype=np.uint8), R))
    return out


def join_expected(ref, R):
    """join_reference's dict per walk; ops as one array, walk after walk"""
    out = {f: tiled(ref[f], R) for f in ("edits", "flags", "n_ops", "matches")}
    out.update(ops_off=offsets(ref["ops_off"], R), ops=tiled(np.concatenate([np.zeros(0, dtype=np.uint32)] + list(ref["ops"])), R))
    return out


# ---- s2k_walks_segments: case = the dict of test_align_segments.anchor_case ---------------------------------------------------------------------
def segments_inputs(case, R):
    """walks, steps, unitigs, nodes, reads' items and source steps all repeat.  A walk's q_begin is a place in the query pool: copy c's
    gain c * query_span(case); its target offsets gain the copy's target bytes; start, qstart, qend and the path coordinates are the read's
    and the walk's own"""
    W, uni, mo, src = case["walks"], case["uni"], case["mo"], case["src"]
    n_steps, n_nodes = len(case["paths"]["unitig"]), len(uni["members"])
    assert case.get("src_pos") is None
    walks = {f: tiled(W[f], R) for f in ("n_steps", "qstart", "qend", "path_start", "path_end", "flags")}
    walks.update(walk_off=offsets(W["walk_off"], R), first_step=shifted(W["first_step"], R, n_steps))
    sstep = case.get("src_step")
    return {"walks": walks, "paths": {"unitig": shifted(case["paths"]["unitig"], R, 2 * len(uni["circular"])), "pos": tiled(case["paths"]["pos"], R),
                                      "count": tiled(case["paths"]["count"], R)},
            "uni": {"uni_off": offsets(uni["uni_off"], R), "members": shifted(uni["members"], R, 2 * n_nodes), "circular": tiled(uni["circular"], R)},
            "mo": {"member_off": shifted(mo["member_off"], R, int(mo["out_off"][-1])), "out_off": offsets(mo["out_off"], R), "overlap": tiled(mo["overlap"], R)},
            "seq_len": tiled(case["seq_len"], R), "q_begin": shifted(case["q_begin"], R, query_span(case)), "tgt_off": offsets(case["tgt_off"], R),
            "bad": tiled(case["bad"], R),
            "src": {"path_off": offsets(src["path_off"], R), "pos": tiled(src["pos"], R), "count": tiled(src["count"], R), "item": tiled(src["item"], R)},
            "src_step": None if sstep is None else shifted(sstep, R, n_steps, keep=2 ** 64 - 1), "src_pos": None,
            "km_off": offsets(case["km_off"], R), "start": tiled(case["start"], R)}


def query_span(case):
    """bytes of query pool one copy's walks lie in"""
    return int((case["q_begin"].astype(np.int64) + case["walks"]["qend"] - case["walks"]["qstart"]).max()) + 1


def segments_expected(ref, R, q_span, t_span):
    """segments_reference's dict (cuts left out: they are the same intervals, relative)"""
    return {"seg_off": offsets(ref["seg_off"], R), "q_begin": shifted(ref["q_begin"], R, q_span), "q_end": shifted(ref["q_end"], R, q_span),
            "t_begin": shifted(ref["t_begin"], R, t_span), "t_end": shifted(ref["t_end"], R, t_span), "stats": [R * x for x in ref["stats"]]}


CALLS = {
    "s2k_walks_segments": (segments_inputs, segments_expected),
    "s2k_align_join": (join_inputs, join_expected),
    "s2k_pileup_consensus_ex": (consensus_ex_inputs, consensus_expected),
    "s2k_walks_pileup_ex": (pileup_inputs, pileup_ex_expected),
    "s2k_walks_pileup": (pileup_inputs, pileup_expected),
    "s2k_walks_targets": (targets_inputs, targets_expected),
    "s2k_paths_walks": (walks_inputs, walks_expected),
    "s2k_pileup_consensus": (consensus_inputs, consensus_expected),
    "s2k_paths_bridge": (bridge_inputs, bridge_expected),
    "s2k_unitig_copy_places": (copy_places_inputs, copy_places_expected),
    "s2k_paths_lift": (lift_inputs, lift_expected),
    "s2k_graph_simplify_mask": (mask_inputs, mask_expected),
    "s2k_graph_bubble_mask": (mask_inputs, mask_expected),
    "s2k_paths_spans": (spans_inputs, spans_expected),
    "s2k_graph_resolve_mask": (resolve_inputs, resolve_expected),
}
