"""GPU tier: no call may read a word of the shared call workspace that it did not write itself.

Every count, table, graph, read-path, alignment and pile-up entry point carves its scratch memory from one grow-only buffer of the context
(`ctx_count_table`, mostly through `Layout::alloc` of s2k_call.h), always from offset 0, and the buffer is never cleared.  A fresh
buffer is usually zero, and a module-scoped engine hands a stage the remains of its own earlier call, so a forgotten zero, a mask word
read past n, a counter that is never reset or a flag left by a refused call all pass the per-stage suites.  Here the engine is created
under S2K_POISON_WS=<byte>: the library then fills the WHOLE buffer with that byte at every hand-out, on the context's stream.
0xFF makes every mask full, every flag set and every index -1; 0x5A makes masks half full and every count large and positive.

No reference of its own: every stage runs through the `device_*` / `check_*` helper of its own module (guarded outputs, the
sizes-only and one-short-capacity variants, every array and total against the module's plain Python reference) on the poisoned engine:
the stage's hand-made cases, one case each at 65, 2049 and 3 * 2048 + 1 of the stage's units (a wave seam, a tile seam, a scan over
several tiles with a ragged last word), its "one run longer than two tiles" case, and a refused call followed at once by the accepted
base case (a flag word or totals left behind).  Where a stage's first refusal is decided on the host before the workspace is taken, the
first one that the device decides is made as well."""
import ctypes
import os

import numpy as np
import pytest

import test_align as ta
import test_align_segments as tas
import test_bridge as tb
import test_count as tc
import test_count_merge as tcm
import test_count_solid as tcs
import test_count_table as tct
import test_graph as tg
import test_lift as tl
import test_pileup as tp
import test_simplify as ts
import test_span as tsp
import test_thread as tt
import test_unitig_sequences as tus
import test_unitigs as tu
import test_untangle as tun
import test_vote as tv
import test_walk as twk
from s2k_loader import import_package

pkg = import_package()
pytestmark = pytest.mark.gpu

SIZES = (65, 2049, 3 * 2048 + 1)
POISON_LINE = "s2k: workspace poisoned: "


def _engine(env):
    """an engine created under the given S2K_* variables; they are read once, in s2k_create, and removed again at once"""
    for k, v in env.items():
        os.environ[k] = v
    try:
        return pkg.Engine(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module", params=[0xFF, 0x5A], ids=["0xff", "0x5a"])
def eng(request):
    os.environ["S2K_POISON_WS"] = str(request.param)
    try:
        e = pkg.Engine(0)
    finally:
        del os.environ["S2K_POISON_WS"]
    yield e
    e.close()


def _lens(n):
    """read lengths that add up to n items: a long read, an empty one, a one-item read, the rest"""
    return [n // 3, 0, 1, n - n // 3 - 1]


def _km_off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)


def _changed(src, i, v):
    x = np.array(src).copy()
    x[i] = v
    return x


# ---- count: s2k_count_device, s2k_count_device_ex (sorted and not), s2k_partition_device, s2k_count_merge_device ----------------------
def count_cases():
    rng = np.random.default_rng(901)
    M = np.uint64(tc.M64)
    out = [np.array([12345], dtype=np.uint64), np.array([M], dtype=np.uint64), np.array([0], dtype=np.uint64),
           np.array([5, 5, 7, M, 0, 5, M, 9, 0], dtype=np.uint64)]
    for n in SIZES:
        vals = rng.integers(0, 2 ** 64, size=n // 3 + 1, dtype=np.uint64)
        keys = vals[rng.integers(0, len(vals), size=n)]
        keys[0], keys[-1] = M, 0  # the table's EMPTY value and 0 are legal keys
        out.append(keys)
    return out


def merge_cases():
    rng = np.random.default_rng(902)
    T = tcm.TILE
    return [tcm.random_tables(rng, na, nb, 0.5) for na, nb in ((0, 1), (1, 1), (65, 33), (2049, 2049), (3 * 2048 + 1, 100), (T + 1, T - 1))]


def _count_ok(eng, keys):
    want = tc._unique_dict(keys)
    st, nd, k, c = tc._count(eng, keys)
    assert (st, nd) == (0, len(want)) and tc._as_dict(k, c) == want, len(keys)
    return want


def test_count(eng):
    import torch

    cases = count_cases()
    for keys in cases:
        _count_ok(eng, keys)
        for mc in (1, 2):
            tcs._check(eng, keys, mc, sorted_=True)
            tcs._check(eng, keys, mc, sorted_=False)
        ks = np.sort(keys)
        for parts in (3, 64):
            tc._check_partition(eng, keys, ks, parts)
    a = np.array([0, 5, tcm.U64MAX], dtype=np.uint64)  # the hand-made saturating tables of test_count_merge.py
    ca, cb = np.array([tcm.SAT - 10, tcm.SAT - 10, tcm.SAT], dtype=np.uint32), np.array([100, 10, tcm.SAT], dtype=np.uint32)
    tcm._check_merge(eng, a, ca, a, cb, mcs=(0, tcm.SAT))
    merges = merge_cases()
    for m in merges:
        tcm._check_merge(eng, *m, mcs=(1, 2))
    # a refused call, then the base case at once
    keys = cases[-2]
    want = tc._unique_dict(keys)
    st, nd, k, c = tc._count(eng, keys, capacity=len(want) - 1)
    assert (st, nd) == (7, len(want))
    _count_ok(eng, keys)
    rnd, rk, _ = tcs.solid_reference(keys, 2)
    d = torch.from_numpy(keys.view(np.int64).copy()).to("cuda:0")
    with pytest.raises(pkg.S2kError) as e:
        tcs._run(eng, d, len(keys), 2, capacity=len(rk) - 1)
    assert e.value.status == 7 and e.value.n_kept == len(rk) and e.value.n_distinct == rnd
    tcs._check(eng, keys, 2, sorted_=True)
    t16, off = torch.zeros(16, dtype=torch.int64, device="cuda"), torch.zeros(80, dtype=torch.int64, device="cuda")
    with pytest.raises(pkg.S2kError) as e:
        eng.partition_device(t16.data_ptr(), 16, 0, t16.data_ptr(), off.data_ptr())
    assert e.value.status == 1
    tc._check_partition(eng, keys, np.sort(keys), 7)
    x, cx, y, cy = merges[3]  # not strictly ascending: the device decides, the canaries stay
    bad = x.copy()
    bad[[100, 101]] = bad[[101, 100]]
    n = len(x) + len(y)
    canary_k = torch.full((n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    canary_c = torch.full((n,), 0x3C3C3C3C, dtype=torch.int32, device="cuda:0")
    dx, dcx, dy, dcy = tcm._dev(bad, torch.int64), tcm._dev(cx, torch.int32), tcm._dev(y, torch.int64), tcm._dev(cy, torch.int32)
    torch.cuda.synchronize()
    st, _, _ = tcm._raw_merge(eng, dx.data_ptr(), dcx.data_ptr(), len(x), dy.data_ptr(), dcy.data_ptr(), len(y), canary_k.data_ptr(), canary_c.data_ptr(), n)
    torch.cuda.synchronize()
    assert st == 1 and bool((canary_k == 0x5A5A5A5A5A5A5A5A).all()) and bool((canary_c == 0x3C3C3C3C).all())
    tcm._check_merge(eng, x, cx, y, cy, mcs=(1, 2))


# ---- table: s2k_table_filter, s2k_table_edges ----------------------------------------------------------------------------------------
FILTER_HAND = [0, 3, 0, 0, 5000, 1, 0, 2, 64, 63, 65, 0, 7000, 0, 0]  # the hand-made reads of test_count_table.py, without the random short ones
EDGES_HAND = [2047, 1, 2048, 0, 0, 2047, 1, 1, 0, 5000, 1, 0, 2, 3, 0, 700]  # ... of test_graph.py


def table_cases():
    rng = np.random.default_rng(903)
    keys, cnt = tg._random_table(rng, 3000)
    filt, edges = [], []
    for lens in [FILTER_HAND] + [_lens(n) for n in SIZES]:
        km_off = _km_off(lens)
        h = tct._items(rng, km_off, keys)
        n = len(h)
        filt.append((km_off, h, rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32),
                     rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2, size=n).astype(np.uint8)))
    for lens in [EDGES_HAND] + [_lens(n) for n in SIZES]:
        km_off = _km_off(lens)
        edges.append((km_off,) + tg._items(rng, km_off, keys, pool=50))
    return keys, cnt, filt, edges


def test_table(eng):
    keys, cnt, filt, edges = table_cases()
    t = tg._table(eng, keys, cnt)
    for km_off, h, st, en, rv in filt:
        for mc in (1, 2, 5):
            tct._assert_filter(eng, t, keys, cnt, km_off, h, st, en, rv, mc)
    for km_off, h, rv in edges:
        for mc in (1, 3):
            tg._check_edges(eng, t, keys, cnt, km_off, h, rv, mc)
    # capacity one short (the size set, nothing written), then the base case
    km_off, h, st, en, rv = filt[2]
    want = tct.filter_reference(km_off, h, tct.lookup_reference(keys, cnt, h), 1, {"start": st})
    s, nk, got = tct._raw_filter(eng, t, km_off, h, st, mc=1, capacity=len(want["hash"]) - 1, outputs=("hash", "start", "offset", "count"))
    assert (s, nk) == (7, len(want["hash"])) and all((got[f] == 0x5A).all() for f in ("hash", "start", "offset", "count"))
    s, nk, _ = tct._raw_filter(eng, t, km_off + np.uint64(1), np.concatenate([h, h[:1]]), mc=1, outputs=("hash",))  # km_off must start at 0
    assert s == 1
    tct._assert_filter(eng, t, keys, cnt, km_off, h, st, en, rv, 1)
    km_off, h, rv = edges[2]
    ne = len(tg.edges_reference(km_off, h, rv, keys, cnt, 2))
    s, n, got = tg._raw_edges(eng, t, km_off, h, rv, 2, capacity=ne - 1)
    assert ne > 100 and (s, n) == (7, ne) and (got == -0x5A5A).all()
    tg._check_edges(eng, t, keys, cnt, km_off, h, rv, 2)
    t.close()


# ---- graph: s2k_graph_adjacency --------------------------------------------------------------------------------------------------------
def adjacency_cases():
    rng = np.random.default_rng(904)
    out = [(n, tg._random_edge_table(rng, n, m)) for n, m in ((1, 3), (3, 5), (3, 0))]
    for m in SIZES:
        n = max(m // 3, 12)
        e = tg._random_edge_table(rng, n, 2 * m)
        assert len(e) > m
        out.append((n, np.concatenate([e[:m - 1], e[-1:]])))  # exactly m keys, the largest one kept
    return out


def graph_batches():
    """two batches of reads over few distinct k-min-mers (so nodes and edges repeat), as the host arrays graph_reference takes"""
    rng = np.random.default_rng(914)
    keys, _ = tg._random_table(rng, 300)
    out = []
    for lens in (_lens(2049), [0, 65, 1, 700, 0]):
        km_off = _km_off(lens)
        h, rv = tg._items(rng, km_off, keys, frac=0.9, pool=60)
        out.append({"km_off": km_off, "hash": h, "rev": rv})
    return out


def test_graph(eng):
    import torch

    cases = adjacency_cases()
    for n, e in cases:
        tg._check_adjacency(eng, e, n)
    # the whole build on the poisoned context: two counters, the table's edges, the adjacency
    batches = graph_batches()
    outs = [{"km_off": tg._dev(b["km_off"], torch.int64), "hash": tg._dev(b["hash"], torch.int64), "rev": tg._dev(b["rev"], torch.uint8)} for b in batches]
    torch.cuda.synchronize()
    for mc, mec in ((2, 1), (2, 2), (1, 1)):
        want = tg.graph_reference(batches, mc, mec)
        assert len(want["keys"]) > 20 and len(want["edge_keys"]) > 100
        tg._assert_graph(tg._graph_host(pkg.KminmerGraph.build(eng, outs, min_count=mc, min_edge_count=mec)), want, (mc, mec))
    n, e = cases[-2]
    x = e.copy()
    x[[700, 701]] = x[[701, 700]]  # an unsorted table: refused with nothing written
    s, ro, dst = tg._raw_adjacency(eng, x, n)
    assert s == 1 and (ro == -3).all() and (dst == -3).all()
    tg._check_adjacency(eng, e, n)


# ---- unitigs: s2k_graph_unitigs, s2k_graph_unitig_edges -------------------------------------------------------------------------------
def unitig_cases():
    rng = np.random.default_rng(905)
    out = []
    for n in SIZES:
        ro, d = tu.random_symmetric_graph(rng, n, n // 3, max_seg=9)
        out.append((n, ro, d, tu.unitig_reference(ro, d, n)))
    return out


def test_unitigs(eng):
    for name in tu.HAND:
        n, ro, d, want = tu.hand_case(name)
        tu.device_unitigs(eng, ro, d, n, want, name)
    cases = unitig_cases()
    for n, ro, d, want in cases:
        tu.device_unitigs(eng, ro, d, n, want, ("random", n))
    # a missing twin (the last destination of a row replaced by a larger id whose twin's row does not lead back), then the base case
    n, ro, d, want = cases[1]
    ros, ds = [int(x) for x in ro], d.tolist()
    u = next(x for x in range(2 * n) if ros[x + 1] - ros[x] >= 2)
    edges = {(a, ds[i]) for a in range(2 * n) for i in range(ros[a], ros[a + 1])}
    x = d.copy()
    x[ros[u + 1] - 1] = next(v for v in range(ds[ros[u + 1] - 1] + 1, 2 * n) if (v ^ 1, u ^ 1) not in edges)
    s, nu, nl, host, _, _ = tu._raw_unitigs(eng, ro, x, n)
    assert (s, nu, nl) == (1, 0, 0) and tu._untouched(host)
    s, nu, nl, host, _, _ = tu._raw_unitigs(eng, ro, d, n, capacity=want["n_unitigs"] - 1)  # one short: the counts still set
    assert (s, nu, nl) == (7, want["n_unitigs"], want["n_links"]) and tu._untouched(host)
    tu.device_unitigs(eng, ro, d, n, want, "base")


# ---- sequences: s2k_table_representatives, s2k_table_node_sequences, s2k_unitig_sequences --------------------------------------------
def test_sequences(eng):
    for name, (batches, want, pool, circ) in tus.HAND.items():
        g, uni, nodes, seqs = tus.check_device(eng, batches, 2, 1, name)
        assert tus.unitig_strings(uni, seqs) == want
    for n in SIZES:  # the seam batches of test_vote.py: reads of n items, nodes with many occurrences
        tus.check_device(eng, [tv.seam_batch([n], 5)], 2, 1, ("seam", n))
    tus.check_device(eng, [tv.seam_batch([40, 0, 25], 5), tv.seam_batch([2040, 9], 6)], 2, 1, "two batches")
    # the stitch: one byte short, then inputs that are no decomposition, then the base case
    batches = tus.HAND["circle, two batches"][0]
    g, uni, nodes, seqs = tus.reference_pipeline(batches, 2, 1)
    n = len(g["keys"])
    got, ok, (arr, pool) = tus.raw_nodes(eng, batches, g["keys"], 2)
    assert ok
    s, nb, out_off, out, overlap = tus.raw_stitch(eng, uni, n, arr, pool, capacity=8)
    assert (s, nb) == (7, 9) and out.untouched() and out_off.untouched() and overlap.untouched()
    bad = dict(uni, uni_off=np.array([0, 2], dtype=uni["uni_off"].dtype))
    s, nb, out_off, out, overlap = tus.raw_stitch(eng, bad, n, arr, pool, want_out=False)
    assert (s, nb) == (1, 0) and out_off.untouched() and overlap.untouched()
    tus.check_device(eng, batches, 2, 1, "base")


# ---- vote: s2k_table_vote_keys, s2k_table_vote_representatives, s2k_vote_ordinals ----------------------------------------------------
def test_vote(eng):
    import torch

    for name, (batches, keys, rep) in tv.HANDV.items():
        tv.check_device(eng, batches, keys, 2, tv.vote_reference(batches, keys, 2), name)
    for counts in ([65], [2049], [3 * 2048 + 1], [1, 2047, 1]):
        batches = [tv.seam_batch(counts, 5)]
        tv.check_device(eng, batches, tv.SEAM_KEYS, 2, tv.vote_reference(batches, tv.SEAM_KEYS, 2), counts)
    # a wrong k, the triples of another call, capacity one short: nothing written; then the base case
    batches, keys, _ = tv.HANDV["first occurrence differs"]
    b, other = batches[0], tv.seam_batch([7], 1)
    ref = tv.vote_reference(batches, keys, 2)
    n = len(ref["streams"][0])
    t = tg._table(eng, keys, None)
    d, od = tv.dev_batch(b), tv.dev_batch(other)
    out = tv.Guarded(n, np.uint64)
    torch.cuda.synchronize()
    assert tv.raw_keys(eng, t, b, d, 3, out, n) == (1, 0)
    i = tus._in_struct(b, d)
    i.mn_capacity = int(other["mn_off"][-1])
    for f in ("mn_off", "mn_j", "mn_jend"):
        setattr(i, f, od[f].data_ptr())
    assert tv.raw_keys(eng, t, b, d, 2, out, n, i) == (1, 0)
    assert tv.raw_keys(eng, t, b, d, 2, out, n - 1) == (7, n)
    assert out.untouched()
    t.close()
    tv.check_device(eng, batches, keys, 2, ref, "base")


# ---- simplify: s2k_graph_simplify_mask, s2k_graph_induced -----------------------------------------------------------------------------
def simplify_cases():
    rng = np.random.default_rng(906)
    out = []
    for n in SIZES:
        g = ts.random_graph_with_errors(rng, n, n // 200, n // 10, n // 10)
        out.append((n, g, ts.round_reference(g, 4, 8)))
    return out


def _simplify_round(eng, g, r, tag):
    ts.device_mask(eng, r["uro"], r["ud"], r["uni"]["uni_off"], r["ucnt"], 4, 8, (r["remove"], r["tips"], r["bubbles"], r["removed"]), tag)
    ts.device_induced(eng, g, r["keep"], r["ind"], tag)
    s, a, b, host = ts.raw_induced(eng, g, node_unitig=r["uni"]["node_unitig"], remove=r["remove"])  # the node mask from the unitig mask
    assert (s, a, b) == (0, len(r["ind"]["keys"]), len(r["ind"]["edge_keys"])), tag
    for f, dt in ts.IND:
        assert host[f][:len(r["ind"][f])].tobytes() == r["ind"][f].tobytes() and ts._marked(host[f], dt, len(r["ind"][f])), (tag, f)


def test_simplify(eng):
    for name in ts.HAND:
        T, ro, d, off, cnt, mt, mb, want, nt, nb = ts.hand_case(name)
        ts.device_mask(eng, ro, d, off, cnt, mt, mb, (want, nt, nb, int(want.sum())), name)
        g, keep = ts.hand_node_graph(name)
        ts.device_induced(eng, g, keep, ts.induced_reference(g["keys"], g["counts"], g["edge_keys"], g["edge_counts"], keep), name)
    cases = simplify_cases()
    for n, g, r in cases:
        assert n < 2049 or (r["tips"] > 10 and r["bubbles"] > 10)
        _simplify_round(eng, g, r, ("random", n))
    # an id >= 2 T in dst: refused, totals 0, nothing written; an induced call one short; then the base case
    n, g, r = cases[1]
    ro, d, off, cnt = r["uro"], r["ud"], r["uni"]["uni_off"], r["ucnt"]
    T = len(off) - 1
    ros = [int(x) for x in ro]
    u = next(x for x in range(2 * T) if ros[x + 1] - ros[x] >= 2)
    s, a, b, c, rem = ts.raw_mask(eng, ro, _changed(d, ros[u], 2 * T), off, cnt, 4, 8)
    assert (s, a, b, c) == (1, 0, 0, 0) and ts._marked(rem, np.uint8)
    nn, ne = len(r["ind"]["keys"]), len(r["ind"]["edge_keys"])
    s, a, b, host = ts.raw_induced(eng, g, keep=r["keep"], node_cap=nn - 1)
    assert (s, a, b) == (7, nn, ne) and ts._all_marked(host)
    _simplify_round(eng, g, r, "base")


# ---- thread: s2k_unitig_node_places, s2k_table_thread ------------------------------------------------------------------------------------
def thread_cases():
    rng = np.random.default_rng(907)
    out = []
    for n in SIZES:
        keys, cnt = tg._random_table(rng, max(50, n // 2))
        uni = tt.random_unitigs(rng, len(keys), max_len=1 + len(keys) // 20)
        km_off = _km_off(_lens(n))
        h, rv = tt.walk_items(rng, km_off, keys, uni)
        se = rng.integers(0, 2 ** 32, size=(2, n), dtype=np.uint32)
        out.append((("random", n), keys, cnt, uni, km_off, h, rv, se[0], se[1]))
    keys, cnt = tg._random_table(rng, 9000)  # one read of more than three tiles along one unitig: one step
    uni = tt.random_unitigs(rng, len(keys), lens=[7000], p_cycle=0.0)
    km_off = np.array([0, 0, 7000, 7005], dtype=np.uint64)
    h, rv = tt.walk_items(rng, km_off, keys, uni, gap=0.0, jump=0.0, t_first=0)
    out.append(("long", keys, cnt, uni, km_off, h, rv, None, None))
    return out


def _thread_hand(eng, mcs=(1, 2)):
    uni = tt.decomposition(*tt.HAND_UNI)
    dplace, place = tt.device_places(eng, uni)
    keys, cnt, km_off, h, rv = tt.hand_batch()
    table = tg._table(eng, keys, cnt)
    for mc in mcs:
        tt.device_thread(eng, table, keys, cnt, km_off, h, rv, mc, dplace, place, 4, ("hand", mc))
    table.close()


def test_thread(eng):
    import torch

    _thread_hand(eng, (0, 1, 2, 3, 4))
    cases = thread_cases()
    for i, (tag, keys, cnt, uni, km_off, h, rv, st, en) in enumerate(cases):
        dplace, place = tt.device_places(eng, uni)
        table = tg._table(eng, keys, cnt)
        for mc in ((1,) if tag == "long" else (1, 2)):
            ref = tt.device_thread(eng, table, keys, cnt, km_off, h, rv, mc, dplace, place, uni["n_unitigs"], (tag, mc), st, en, front=i % 4)
        if tag == "long":
            assert ref["path_off"][2] == 1 and ref["count"][0] == 7000
        table.close()
    # a place record that names a unitig >= n_unitigs, used by a solid item: refused, nothing written; then the base case
    tag, keys, cnt, uni, km_off, h, rv, st, en = cases[1]
    T = uni["n_unitigs"]
    dplace, place = tt.device_places(eng, uni)
    table = tg._table(eng, keys, cnt)
    x = place.copy()
    node = int(np.searchsorted(keys, h[np.nonzero(np.isin(h, keys))[0][0]]))
    x["unitig"][node] = 2 * T
    s, n, host = tt.raw_thread(eng, table, km_off, h, rv, 1, torch.from_numpy(x.view(np.int32).reshape(-1, 4).copy()).to("cuda:0"), T)
    assert s == 1 and n == 0 and tt._marked(host["path_off"]) and all(tt._marked(host[f]) for f in tt.STEP)
    y = uni["node_pos"].copy()  # places: a position outside its unitig
    y[17] = 2 ** 31
    s, got = tt.raw_places(eng, dict(uni, node_pos=y))
    assert s == 1 and (got == tt.MARK).all()
    tt.device_places(eng, uni)
    tt.device_thread(eng, table, keys, cnt, km_off, h, rv, 1, dplace, place, T, "base", st, en)
    table.close()


# ---- span: s2k_paths_spans, s2k_graph_resolve_mask ------------------------------------------------------------------------------------
def span_cases():
    rng = np.random.default_rng(908)
    out = []
    for n in SIZES:
        for paired in (False, True):
            out.append(((n, paired),) + tsp.chained_paths(rng, 37, _lens(n), p_break=0.1 if not paired else 0.02, paired=paired))
    return out


def test_span(eng):
    import torch

    ro, d, off = tsp.hand_graph()
    for extra in (False, True):
        paths, cases = tsp.hand_paths(extra)
        ref = tsp.device_spans(eng, paths, ro, d, off, ("hand", extra))
        sk, sc = tsp.count_keys(ref["keys"])
        for ms in (0, 1, 2, 3):
            tsp.device_resolve(eng, ro, d, 8, sk, sc, ms, ("hand", extra, ms))
    cases = span_cases()
    for i, (tag, paths, ro, d, off, T) in enumerate(cases):
        assert len(paths["unitig"]) == tag[0]
        tsp.device_spans(eng, paths, ro, d, off, tag, front=i % 2)
    # path_off that does not start at 0: refused, totals 0, nothing written, the support as it was; then the base case
    tag, paths, ro, d, off, T = cases[2]
    sup = torch.zeros(len(d), dtype=torch.int64, device="cuda:0")
    s, nk, nf, no, keys = tsp.raw_spans(eng, dict(paths, path_off=_changed(paths["path_off"], 0, 1)), ro, d, off, support=sup)
    assert (s, nk, nf, no) == (1, 0, 0, 0) and tsp._marked(keys) and int(sup.sum()) == 0
    ref = tsp.device_spans(eng, paths, ro, d, off, "base")
    sk, sc = tsp.count_keys(ref["keys"])
    x = sk.copy()  # the resolution: keys that are not strictly ascending
    x[5] = x[4]
    s, nc, nr, res, par = tsp.raw_resolve(eng, ro, d, T, x, sc, 1)
    assert (s, nc, nr) == (1, 0, 0) and tsp._marked(res) and tsp._marked(par)
    tsp.device_resolve(eng, ro, d, T, sk, sc, 1, "base")


# ---- untangle: s2k_graph_untangle, s2k_unitig_expand ----------------------------------------------------------------------------------
def untangle_cases():
    return [(n, tun.chain_case(np.random.default_rng(909 + n), 9, 60, front=n % 3, n_copies=n)) for n in SIZES]


def test_untangle(eng):
    for name in tun.HAND:
        tun.device_case(eng, tun.hand(name), name)
    for n, case in untangle_cases():
        r = tun.device_case(eng, case, ("copies", n), invariants=n < 3000)
        assert r["u"]["n_copies"] == n and r["u"]["n_duplicated"] > 0
    # a partner outside the row of the strand its edge enters: refused, nothing written; then the base case
    base = tun.hand("d")
    ins, (oa, ob) = tun._edges_into(base, 6)
    s, nc, nd, got = tun.raw_untangle(eng, dict(base, partner=_changed(base["partner"], ins[0], oa - 1)))
    assert (s, nc, nd) == (1, 0, 0) and tun._untouched(got, tun.UNT)
    r = tun.device_case(eng, base, "base")
    o = r["o"]
    s, nm, got = tun.raw_expand(eng, dict(o, members=_changed(o["members"], 4, 2 * len(r["u"]["origin"]))), r["u"]["origin"], base["inner"])  # no copy
    assert (s, nm) == (1, 0) and tun._untouched(got, tun.EXP)
    tun.device_expand(eng, o, r["u"]["origin"], base["inner"], r["x"], "base")


# ---- walk: s2k_unitig_member_offsets, s2k_paths_walks ---------------------------------------------------------------------------------
def device_member_offsets(eng, uni, nodes, tag):
    """s2k_unitig_member_offsets against twk.member_offsets_reference, guards behind the three outputs; node records without bytes"""
    import torch

    ref = twk.member_offsets_reference(uni, nodes)
    n, T = len(uni["members"]), len(uni["uni_off"]) - 1
    sl = np.asarray(nodes["seq_len"], dtype=np.uint32)
    d = {"seq_off": ts._dev(np.concatenate([[0], np.cumsum(sl.astype(np.uint64))[:-1]]).astype(np.uint64), np.uint64), "seq_len": ts._dev(sl, np.uint32),
         "shift_fwd": ts._dev(nodes["shift_fwd"], np.uint32), "shift_rev": ts._dev(nodes["shift_rev"], np.uint32), "rev": ts._dev(nodes["rev"], np.uint8)}
    ns = pkg.NodeSeqs()
    for f, x in d.items():
        setattr(ns, f, x.data_ptr())
    ns.pool, ns.pool_capacity = None, int(sl.astype(np.uint64).sum())
    du = [ts._dev(uni["uni_off"], np.uint64), ts._dev(uni["members"], np.uint32), ts._dev(uni["circular"], np.uint8)]
    mo, oo, ov = ts._out(n, np.uint64), ts._out(T + 1, np.uint64), ts._out(2 * T, np.uint32)
    nb = ctypes.c_uint64(777)
    torch.cuda.synchronize()
    s = eng.lib.s2k_unitig_member_offsets(eng.ctx, *(ts._ptr(x) for x in du), T, n, ctypes.byref(ns), ts._ptr(mo), ts._ptr(oo), ts._ptr(ov), ctypes.byref(nb))
    assert (s, nb.value) == (0, int(ref["out_off"][-1])), (tag, s, nb.value, eng.lib.s2k_last_error(eng.ctx))
    for t, f, dt in ((mo, "member_off", np.uint64), (oo, "out_off", np.uint64), (ov, "overlap", np.uint32)):
        h = ts._host(t, dt)
        assert h[:len(ref[f])].tobytes() == ref[f].tobytes() and ts._marked(h, dt, len(ref[f])), (tag, f)


def walk_cases():
    out = []
    for n in SIZES:
        rng = np.random.default_rng(600 + n)
        lens = list(rng.integers(0, 90, size=3 + n // 12)) + [0, 1, 2]
        out.append((("walked", n), twk.walked_case(rng, max(40, n // 3), lens, n_steps=n)))
    out.append(("long chain", twk.long_chain_case(5000)))
    return out


def test_walk(eng):
    case = twk.hand_case()
    twk.device_walks(eng, case, "hand")
    device_member_offsets(eng, case["uni"], case["nodes"], "hand")
    cases = walk_cases()
    for tag, case in cases:
        device_member_offsets(eng, case["uni"], case["nodes"], tag)
        ref = twk.device_walks(eng, case, tag)
        if tag == "long chain":
            assert ref["n_steps"].tolist() == [5000, 5000]
    # path_off that does not start at 0: refused, nothing written; then the base case
    tag, case = cases[1]
    s, nw, nf, no, got = twk.raw_walks(eng, case, paths=dict(case["paths"], path_off=_changed(case["paths"]["path_off"], 0, 1)))
    assert (s, nw, nf, no) == (1, 0, 0, 0) and all(twk._marked(x) for x in got.values())
    twk.device_walks(eng, case, "base")


# ---- bridge: s2k_paths_bridge --------------------------------------------------------------------------------------------------------------
def bridge_cases():
    out = [(("chained", n), tb.gapped_case(np.random.default_rng(700 + n), n, "chained"), (3, 1)) for n in SIZES]
    out.append((("walked", 2049), tb.gapped_case(np.random.default_rng(699), 2049, "walked"), tb.DEFAULT))
    out.append(("long run", tb.runs_case(10000, [], [5000], T=1), (4, 0)))
    return out


def test_bridge(eng):
    tb.device_bridge(eng, tb.hand_case(), "hand", tb.B_LIMITS)
    tb.device_bridge(eng, tb.hand_case([]), "no reads", tb.B_LIMITS)
    cases = bridge_cases()
    for tag, case, limits in cases:
        ref = tb.device_bridge(eng, case, tag, limits)
        if tag == "long run":
            assert ref["n_steps"] == 2 and ref["n_merged"] == 9998 and ref["matched"].tolist() == [5000, 5000]
    # path_off that does not start at 0: refused, totals 0, nothing written; then the base case
    tag, case, limits = cases[1]
    paths = case["paths"]
    s, no, nm, nb, got = tb.raw_bridge(eng, case, limits, paths=dict(paths, path_off=_changed(paths["path_off"], 0, 1)))
    assert (s, no, nm, nb) == (1, 0, 0, 0) and all(tb._marked(x) for x in got.values())
    tb.device_bridge(eng, case, "base", limits)


# ---- lift: s2k_unitig_copy_places, s2k_paths_lift ------------------------------------------------------------------------------------
def lift_cases():
    out = []
    for n in SIZES:
        rng = np.random.default_rng(800 + n)
        T0 = 9 + n % 7
        out.append((n, tl.ring_case(rng, T0, [12] * max(n // 11 + 8, 15 * T0), 0.03, n_steps=n, unpaired=n // 100 + 2)))
    out.append(("long run", tl.ring_case(np.random.default_rng(83), 31, [12] * 400 + [5000], 0.0)))
    return out


def test_lift(eng):
    for name in sorted(tl.H_READS):
        case = tl.hand_lift(name)
        r = case["r"]
        place = tl.device_copy_places(eng, r["o"], r["u"]["origin"], case["inner"], name)
        assert place.tolist() == tl.H_PLACE[name]
        tl.assert_hand(tl.device_lift(eng, case, name), list(tl.H_READS[name].values()), name)
    for n, ucase in tun_copy_cases():
        r = tun.contigs_reference(ucase)
        assert r["u"]["n_copies"] == n
        tl.device_copy_places(eng, r["o"], r["u"]["origin"], ucase["inner"], ("copies", n))
    cases = lift_cases()
    for tag, case in cases:
        ref = tl.device_lift(eng, case, tag, invariants=False)
        if tag == "long run":
            assert ref["n_merged"] == 5000 - 1 + 400 * 11 and ref["n_steps"] == 401
    # path_off that does not start at 0: refused, the four totals 0, nothing written; then the base case
    tag, case = cases[1]
    paths = case["paths"]
    s, t, got = tl.raw_lift(eng, case, paths=dict(paths, path_off=_changed(paths["path_off"], 0, 1)))
    assert (s, t) == (1, (0, 0, 0, 0)) and tl._untouched(got)
    tl.device_lift(eng, case, "base", invariants=False)
    ucase = tun.hand("a")  # the copy records: an outer member that is no copy
    r = tun.contigs_reference(ucase)
    o, origin = r["o"], r["u"]["origin"]
    s, got = tl.raw_copy_places(eng, dict(o, members=_changed(o["members"], 4, 2 * len(origin))), origin, ucase["inner"])
    assert s == 1 and tl._marked(got)
    tl.device_copy_places(eng, o, origin, ucase["inner"], "base")


def tun_copy_cases():
    return [(n, tun.chain_case(np.random.default_rng(n), 9, 60, front=n % 3, n_copies=n)) for n in SIZES]


# ---- align: s2k_walks_targets, s2k_align_pairs --------------------------------------------------------------------------------------------
def one_step_walks(rng, n_walks, strings):
    """n_walks walks of one step on either strand of the given unitigs, of 0 .. 59 bases (the walks of test_pileup.py's walk counts)"""
    specs = []
    for _ in range(n_walks):
        U = int(rng.integers(0, 2 * len(strings)))
        L = len(strings[U >> 1])
        a = int(rng.integers(0, L - 10))
        specs.append((U, 1, a, a + int(rng.integers(0, min(60, L - a))), 0))
    return tp.one_walks(specs), np.arange(2 * len(strings), dtype=np.uint32)


def pair_cases():
    rng = np.random.default_rng(910)
    out = [("hand", [(q, t) for q, t, _ in ta.HAND_PAIRS], ta.MAX_EDITS)]
    for n in SIZES:
        pairs = []
        for _ in range(n):
            q = ta.random_seq(rng, int(rng.integers(0, 12)))
            pairs.append((q, ta.mutated(rng, q, int(rng.integers(0, 3)))))
        out.append((("pairs", n), pairs, 3 if n > 65 else ta.MAX_EDITS))
    for d in (1, 64):  # wavefronts of 3 and of 129 diagonals
        pairs = [ta.spaced(rng, d, kind) for kind in (0, 1, 2)] + [(ta.random_seq(rng, 3 * d), b"")]
        out.append((("distance", d), pairs + [(ta.mutated(rng, pairs[0][0], d), pairs[0][0])], ta.MAX_EDITS))
    for me in (0, ta.MAX_EDITS):
        at, over = ta.spaced(rng, me, 0, gap=9), ta.spaced(rng, me + 1, 0, gap=9)
        far = (ta.random_seq(rng, 10), ta.random_seq(rng, 10 + me + 1))
        out.append((("max_edits", me), [at, over, at, far, (b"ACGT", b"ACGT"), over], me))
    return out


def test_align(eng):
    walks, paths, strings, mo = ta.hand_targets()
    ta.device_targets(eng, walks, paths["unitig"], strings, mo["overlap"], "hand")
    jw, jsu, jstrings, jov = ta.junction_case()
    assert ta.device_targets(eng, jw, jsu, jstrings, jov, "junction")[2].tolist() == [1, 0, 1, 1]
    rng = np.random.default_rng(911)
    two = [ta.random_seq(rng, 300), ta.random_seq(rng, 41)]
    for n in SIZES:
        w, su = one_step_walks(rng, n, two)
        ta.device_targets(eng, w, su, two, np.zeros(4, dtype=np.uint32), ("walks", n))
    crng = np.random.default_rng(765)  # walks of several steps over junctions, twin strands among them
    ta._case_targets(eng, twk.chained_case(crng, 40, list(crng.integers(1, 9, size=90)), p_break=0.1), 65, "chained", n_walks=65)
    cases = pair_cases()
    for tag, pairs, me in cases:
        ref = ta.device_align(eng, pairs, tag, max_edits=me)
        if tag[0] == "max_edits":
            assert ref["flags"].tolist() == [0, ta.OVER, 0, ta.OVER, 0, ta.OVER]
    # a step index outside the paths: refused, nothing written; then the base case
    su, ov = paths["unitig"], mo["overlap"]
    n = len(ta.targets_reference(walks, su, strings, ov)[1])
    s, nb, got = ta.raw_targets(eng, walks, su, strings, ov, capacity=n, first_step=_changed(walks["first_step"], 3, len(su)))
    assert (s, nb) == (1, 0) and all(ta._marked(x) for x in got.values())
    ta.device_targets(eng, walks, su, strings, ov, "base")
    # a begin above its end: refused, the bound 0, nothing written; then the base case
    pairs = cases[1][1]
    q, t, ivs = ta.pools_of(pairs)
    bound = int(ta.align_many_reference(pairs)["ops_off"][-1])
    bad = [a.copy() for a in ivs]
    bad[0][5] = int(ivs[1][5]) + 1
    s, nb, got = ta.raw_align(eng, q, t, bad, capacity=bound)
    assert (s, nb) == (1, 0) and all(ta._marked(x) for x in got.values())
    ta.device_align(eng, pairs, "base")


# ---- pileup: s2k_walks_pileup, s2k_pileup_consensus ---------------------------------------------------------------------------------------
def _pileup_junctions(eng):
    for tag, *c in tp.junction_cases():
        tp.device_pileup(eng, *c[:5], [0], c[5], tag)


def test_pileup(eng):
    _pileup_junctions(eng)
    walks, paths, strings, mo = ta.hand_targets()
    rng = np.random.default_rng(92)
    su, ov = paths["unitig"], mo["overlap"]
    q, fl, runs = tp.aligned_case(walks, su, strings, ov, rng, 6)
    for ms in (0, tp.MAX_SHIFT):
        tp.device_pileup(eng, walks, su, strings, ov, q, fl, runs, ("hand", ms), max_shift=ms)
    tp.device_cursor(eng)
    two = [ta.random_seq(rng, 300), ta.random_seq(rng, 41)]
    z4 = np.zeros(4, dtype=np.uint32)
    for n in SIZES:
        w, wsu = one_step_walks(rng, n, two)
        wq, wfl, wruns = tp.aligned_case(w, wsu, two, z4, rng, 3)
        tp.device_pileup(eng, w, wsu, two, z4, wq, wfl, wruns, ("walks", n))
    # two adds equal one: the pile is the caller's memory and accumulates, only the workspace is poisoned
    clean, draft, pw, reads, _ = tp.planted_case(3, b"AACGAA")
    psu, pov = np.array([0, 1], dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    pq, pfl, pruns, _ = tp.walk_inputs(pw, psu, [draft], pov, reads)
    rec = {f: pw[f] for f in tp.REC}
    ref, _ = tp.device_pileup(eng, rec, psu, [draft], pov, pq, pfl, pruns, "one add")
    h = len(reads) // 3
    p1, _ = tp.device_pileup(eng, {f: pw[f][:h] for f in tp.REC}, psu, [draft], pov, pq[:h], pfl[:h], pruns[:h], "first batch")
    p2, _ = tp.device_pileup(eng, {f: pw[f][h:] for f in tp.REC}, psu, [draft], pov, pq[h:], pfl[h:], pruns[h:], "second batch", pile=p1)
    assert all((p2[f] == ref[f]).all() for f in tp.PLANES)
    assert tp.device_consensus(eng, ref, [draft], pov, 3, "planted")["strings"][0] == clean
    # the consensus: unitig lengths round a store and a block, random piles, the empty shapes
    lens = [0, 1, 15, 16, 17, 0, 4095, 4096, 4097, 3]
    cs = [ta.random_seq(rng, n, b"ACGTacgtN") for n in lens]
    cov = np.array([int(rng.integers(0, n + 3)) for n in lens for _ in (0, 1)], dtype=np.uint32)
    for min_cov in (0, 3):
        tp.device_consensus(eng, tp.random_pile(rng, cs), cs, cov, min_cov, ("lengths", min_cov))
    for one in ([b""], [b"A"], []):
        tp.device_consensus(eng, tp.new_pile(len(b"".join(one))), one, np.zeros(2 * len(one), dtype=np.uint32), 3, one)
    # a step index outside the paths: refused, the stats 0, the pile as it was; then the base case
    base = {f: walks[f] for f in tp.REC}
    nb = sum(len(s) for s in strings)
    s, st, got = tp.raw_pileup(eng, base, su, strings, ov, q, fl, runs, first_step=_changed(walks["first_step"], 3, len(su)))
    assert s == 1 and st == [0] * 8 and all(not got[f][:nb].any() and (got[f][nb:] == tp.MARK32).all() for f in tp.PLANES)
    tp.device_pileup(eng, base, su, strings, ov, q, fl, runs, "base")
    # out_off that decreases: refused, nothing written; then the base case
    rs = [ta.random_seq(rng, n) for n in (40, 0, 25)]
    rov = np.array([5, 5, 0, 0, 7, 3], dtype=np.uint32)
    pile = tp.random_pile(rng, rs)
    m = len(tp.device_consensus(eng, pile, rs, rov, 2, "base")["out"])
    off = tp.draft_of(rs)[0]
    s, nn, st, got = tp.raw_consensus(eng, pile, rs, rov, 2, capacity=m, out_off=_changed(off, 1, int(off[2]) + 1))
    assert (s, nn) == (1, 0) and st == [0] * 8 and all(tp._cmarked(x) for x in got.values())
    tp.device_consensus(eng, pile, rs, rov, 2, "base again")


# ---- segment: s2k_walks_segments, s2k_align_join ------------------------------------------------------------------------------------------
def test_segment(eng):
    for name, (walks, kw, want, stats) in tas.HAND.items():
        assert tas.device_segments(eng, tas.anchor_case(walks, **kw), name)["stats"] == stats
    for n in SIZES:
        tas.device_segments(eng, tas.many_walks(np.random.default_rng(230 + n), n, per_read=1 + n % 3), ("walks", n))
    for n_items in (257, 4097):  # one read of so many source items: the item tiles, and the compacted stream's at seg_len 64
        c = tas.many_anchors(n_items)
        for seg_len in (64, 512):
            tas.device_segments(eng, c, (n_items, seg_len), seg_len)
    for name, (cig, over, seg_off, bad, want, edits) in tas.JOIN_HAND.items():
        tas.device_join(eng, seg_off, bad, tas._seg(*cig, over=over), name)
    for n in SIZES:
        seg_off, bad, seg = tas.random_segments(np.random.default_rng(240 + n), n)
        tas.device_join(eng, seg_off, bad, seg, ("walks", n))
    k, rest = divmod(2049, 3)  # run slots round a tile: every border merges
    cig = ["4=1X4="] * k + ["1="] * rest
    tas.device_join(eng, [0, len(cig) // 2, len(cig)], [0, 0], tas._seg(*cig), "slots")
    # a step index outside the paths: refused, totals and stats 0, nothing written; then the base case
    c = tas.anchor_case([tas._w([(600, 600), (1200, 1200)]), tas._w([(600, 600)]), tas._w([(700, 700), (1300, 1300)]), tas._w([(600, 600)])], per_read=2)
    n = int(tas.device_segments(eng, c, "base")["seg_off"][-1])
    s, total, stats, got = tas.raw_segments(eng, c, capacity=n, first_step=_changed(tas.flat(c)["first_step"], 3, 5))
    assert (s, total, stats) == (1, 0, [0] * 5) and all(tas._marked(x) for x in got.values())
    tas.device_segments(eng, c, "base again")
    # seg_off that does not start at 0: refused, nothing written; then the base case
    seg_off, bad, seg = [0, 2, 3], [0, 0], tas._seg("5=1X", "1X4=", "7=")
    n = int(tas.device_join(eng, seg_off, bad, seg, "base")["ops_off"][-1])
    s, nb, got = tas.raw_join(eng, np.array([1, 2, 3]), bad, seg, capacity=n)
    assert (s, nb) == (1, 0) and all(tas._marked(x) for x in got.values())
    tas.device_join(eng, seg_off, bad, seg, "base again")


# ---- one context, stage after stage: a large layout followed by a small one of another stage ------------------------------------------
def test_stages_back_to_back_on_one_context(eng):
    _thread_hand(eng)
    twk.device_walks(eng, twk.hand_case(), "walk")
    _pileup_junctions(eng)
    _thread_hand(eng)
    ta.device_align(eng, [(q, t) for q, t, _ in ta.HAND_PAIRS], "align")
    tb.device_bridge(eng, tb.hand_case(), "bridge", tb.B_LIMITS)


# ---- the knob is live, and off when it is not set ---------------------------------------------------------------------------------------
def _small_adjacency(e):
    n, edges = adjacency_cases()[1]
    tg._check_adjacency(e, edges, n)


def test_poisoned_hand_outs_are_traced(capfd):
    e = _engine({"S2K_POISON_WS": "90", "S2K_TRACE": "1"})
    try:
        capfd.readouterr()
        _small_adjacency(e)
        err = capfd.readouterr().err
    finally:
        e.close()
    lines = [x for x in err.splitlines() if x.startswith(POISON_LINE)]
    assert lines, err
    for x in lines:
        byte, times, count, unit = x[len(POISON_LINE):].split()
        assert (byte, times, unit) == ("0x5a", "x", "bytes") and int(count) >= 256, x


def test_no_poison_without_the_variable(capfd):
    assert "S2K_POISON_WS" not in os.environ
    e = _engine({"S2K_TRACE": "1"})
    try:
        capfd.readouterr()
        _small_adjacency(e)
        err = capfd.readouterr().err
    finally:
        e.close()
    assert "poisoned" not in err, err
