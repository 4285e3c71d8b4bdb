"""What the Engine and the pipeline classes share in putting a C call together: host arrays, device pointers, the structs over tensors,
and the checks of the arguments that several calls take."""
import ctypes as C
import types

import numpy as np

from ._abi import STEP_FIELDS, AlignOut, DeviceOut, ThreadOut, torch


def _as_u8(seq):
    if isinstance(seq, str):
        seq = seq.encode("latin-1")
    if isinstance(seq, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


def pack_reads(reads):
    """list of byte strings -> (bases u8[total], read_off u64[n+1])"""
    arrs = [_as_u8(r) for r in reads]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs], dtype=np.uint64)
    bases = np.concatenate(arrs) if arrs and int(off[-1]) else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(bases, dtype=np.uint8), off


def _p(x, k=1):
    """the device pointer of tensor x as a C argument, NULL when k is 0 (an empty array) or x is None"""
    return C.c_void_p(x.data_ptr() if k and x is not None else 0)


def _paths_struct(paths, fields, capacity):
    """-> (ThreadOut, tensors): the struct that names path_off and those of `fields` a ReadPaths carries, and the contiguous
    tensors behind it by field, which the caller keeps alive over its calls"""
    o = ThreadOut()
    o.capacity = capacity
    keep = {f: getattr(paths, f).contiguous() for f in ("path_off",) + tuple(fields) if getattr(paths, f) is not None}
    for f, x in keep.items():
        setattr(o, f, x.data_ptr() if x.numel() else 0)
    return o, keep


def _paths_out(o, res, keep, m, per_step, n_steps):
    """before the second call of paths_bridge / paths_lift: room for m output steps of the step fields the input carries (named in o) and
    of matched, and for the per_step arrays ({name: dtype}, one entry per input step), all into res"""
    dev = res["path_off"].device
    for f in [f for f in STEP_FIELDS if f in keep] + ["matched"]:
        res[f] = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        if f != "matched":
            setattr(o, f, res[f].data_ptr())
    for f, dt in per_step.items():
        res[f] = torch.empty(max(n_steps, 1), dtype=dt, device=dev)
    o.capacity = m


def _paths_result(res, per_step, m, n_steps, **totals):
    """what paths_bridge / paths_lift return: path_off whole, the per_step arrays cut to n_steps, the rest to m, and the totals"""
    return {**{f: (x if f == "path_off" else x[:n_steps] if f in per_step else x[:m]) for f, x in res.items()}, "n_steps": m, **totals}


def _walk_args(name, walks, step_unitig, out_off, out, overlap):
    """what walks_targets and walks_pileup (name) share -> (n_walks, device, the C arguments n_walks .. n_unitigs, the tensors to keep alive)"""
    rec = [getattr(walks, f).contiguous() for f in ("first_step", "n_steps", "path_start", "path_end", "flags")]
    step_unitig, out_off, out, overlap = keep = [x.contiguous() for x in (step_unitig, out_off, out, overlap)]
    nw, ns, t = rec[0].numel(), step_unitig.numel(), out_off.numel() - 1
    if (any(x.numel() != nw for x in rec) or [x.element_size() for x in rec] != [8, 4, 8, 8, 4] or step_unitig.element_size() != 4
            or out_off.element_size() != 8 or out.element_size() != 1 or overlap.numel() != 2 * t or overlap.element_size() != 4):
        raise ValueError(name + " wants the walk records, one 32-bit unitig per step, and the out_off, out and overlap of the unitig sequences")
    return nw, out_off.device, (nw, *(_p(x, nw) for x in rec), _p(step_unitig, ns), ns, _p(out_off), _p(out, out.numel()), out.numel(), _p(overlap, t), t), rec + keep


def _align_out(n, dev, m=None, res=None, fields=None):
    """the results of align_pairs / align_join over n records -> (AlignOut, res, cut): res holds edits, flags, n_ops, matches (int32 per record),
    ops_off (int64, n + 1) and, once the number of runs m is known, ops; the struct names `fields` (None: all) with capacity m; cut(): res as returned"""
    if res is None:
        res = {f: torch.zeros(max(n, 1), dtype=torch.int32, device=dev) for f in ("edits", "flags", "n_ops", "matches")}
        res["ops_off"] = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    o = AlignOut(m or 0)
    if m is not None:
        res["ops"] = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
    for f in fields or res:
        setattr(o, f, res[f].data_ptr())
    return o, res, lambda: {f: (x if f == "ops_off" else x[:m] if f == "ops" else x[:n]) for f, x in res.items()}


def extraction_struct(o, n_reads, optional=(), mn=False, required=("km_off", "hash")):
    """The DeviceOut over one batch's extraction tensors o (a dict) as the table calls read it: km_capacity = km_off[n_reads], the item
    count; the `required` fields and those of `optional` that o carries; with mn, when o carries mn_off, also mn_off, mn_j, mn_jend and
    mn_capacity = mn_off[n_reads]"""
    i = DeviceOut()
    i.km_capacity = int(o["km_off"][n_reads].item()) if n_reads else 0
    for f in tuple(required) + tuple(f for f in optional if o.get(f) is not None):
        setattr(i, f, o[f].data_ptr())
    if mn and o.get("mn_off") is not None:
        i.mn_capacity = int(o["mn_off"][n_reads].item()) if n_reads else 0
        i.mn_off, i.mn_j, i.mn_jend = (o[f].data_ptr() for f in ("mn_off", "mn_j", "mn_jend"))
    return i


def _shaped(tensors, shapes):
    """every tensor has its (length, bytes per element) of `shapes`"""
    return [(x.numel(), x.element_size()) for x in tensors] == list(shapes)


def _graph_arg(ug, parts, text):
    """The parts of a UnitigGraph that a C call reads, made contiguous and checked -> a namespace of t, ne, n (unitigs, edges, members) and
    the tensors that `parts` name: csr (row_off and dst), uni_off, circular, counts, edge_counts, members.  ValueError(text) when the
    length or the element size of one of them is not what include/s2k.h gives it."""
    t, ne, n = ug.n_unitigs, ug.dst.numel(), ug.members.numel()
    shape = {"row_off": (2 * t + 1, 8), "dst": (ne, 4), "uni_off": (t + 1, 8), "circular": (t, 1), "counts": (t, 8), "edge_counts": (ne, 4), "members": (n, 4)}
    g = types.SimpleNamespace(t=t, ne=ne, n=n)
    for f in [f for p in parts for f in (("row_off", "dst") if p == "csr" else (p,))]:
        setattr(g, f, getattr(ug, f).contiguous())
        if not _shaped([getattr(g, f)], [shape[f]]):
            raise ValueError(text)
    return g


def _stitch_arg(g, offsets, seq_len, text):
    """The stitch offsets of the graph g (a _graph_arg) -> contiguous [member_off, out_off, overlap, seq_len]: offsets = what
    Engine.unitig_member_offsets returned for it, seq_len = its NodeSequences'.  ValueError(text) when a length or an element size is off."""
    out = [x.contiguous() for x in (offsets[0], offsets[1], offsets[2], seq_len)]
    if not _shaped(out, [(g.n, 8), (g.t + 1, 8), (2 * g.t, 4), (g.n, 4)]):
        raise ValueError(text)
    return out


def _outer_arg(outer, origin, uni_off, circular, text):
    """The decomposition of an untangled graph's copies -> (contiguous [outer uni_off, outer members, outer circular, origin, uni_off,
    circular], n_contigs, n_copies, n_unitigs): outer = what graph_unitigs returned over the copies, origin = graph_untangle's, uni_off
    and circular = the inner decomposition's.  ValueError(text) when a length or an element size is off."""
    out = [x.contiguous() for x in (outer["uni_off"], outer["members"], outer["circular"], origin, uni_off, circular)]
    nt, ncp, t = out[2].numel(), out[3].numel(), out[5].numel()
    if not _shaped(out, [(nt + 1, 8), (ncp, 4), (nt, 1), (ncp, 4), (t + 1, 8), (t, 1)]):
        raise ValueError(text)
    return out, nt, ncp, t
