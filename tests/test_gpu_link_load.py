"""The link load (linkload.hip) against tests/load_reference.py, through srt_build_link_load (run
on an MI355X with -m gpu).

Every case compares (tail, head, load) and through with the reference bit for bit, the three
demand totals, max_hops, and the identity sum(load) == sum(c * hops). Integers only: no tolerance
anywhere.
"""
import contextlib
import functools

import numpy as np
import pytest

from conftest import form_env
import load_reference as lr
import route_graphs
from shadow_amd import graphs
from shadow_amd._lib import ALGO_AUTO, ALGO_DENSE_FW, ALGO_SPARSE_SSSP, lib
from shadow_amd.topology import build_link_load, build_routes

pytestmark = pytest.mark.gpu
MS = 1_000_000


def canon_arcs(g):
    """The arcs of the canonical graph: the distinct pairs off the diagonal, both ways when the
    graph is undirected."""
    off = g.src != g.dst
    a, b = g.src[off].astype(np.int64), g.dst[off].astype(np.int64)
    if g.directed:
        return len(np.unique(a * g.n + b))
    return 2 * len(np.unique(np.minimum(a, b) * g.n + np.maximum(a, b)))


def check(g, algo=ALGO_AUTO, sources=None, demand=None, load_arcs=None):
    """Build on the device, compare with the reference; returns (arcs dict, through, stats).
    load_arcs: the arcs of the CSR the load is indexed by. When given, the build runs under
    SRT_FORM memcap=1: 1 MiB free is below the reserve, so the budget is half of what the u64 load
    leaves of it, and the rows must come in three chunks or more with a short last one."""
    with form_env(memcap=1) if load_arcs is not None else contextlib.nullcontext():
        got = build_link_load(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                              sources=None if isinstance(demand, tuple) else sources,
                              demand=demand, algo=algo)
        chunks = lib().srt_last_row_chunks()
    tail, head, load, through, st = got
    if load_arcs is not None:
        # per row and vertex: pred, hops and the u64 demand; a sparse build's distance and
        # reliability rows too
        rows = g.n if sources is None else len(sources)
        row_bytes = (16 if algo == ALGO_DENSE_FW else 28) * g.n
        chunk = ((1 << 20) - 8 * load_arcs) // 2 // row_bytes
        print(f"{g.name} algo={algo}: {rows} rows, {chunk} a chunk, {chunks} chunks")
        assert chunks >= 3 and chunks == -(-rows // chunk) and rows % chunk != 0, (chunks, chunk)
    ref = lr.reference(g, sources, demand)
    wt, wh, wl, wthr = ref.arrays()
    what = f"{g.name} algo={algo}"
    assert load.dtype == np.uint64 and through.dtype == np.uint64
    assert np.array_equal(tail, wt) and np.array_equal(head, wh), (what, len(tail), len(wt))
    bad = np.flatnonzero(load != wl)
    assert bad.size == 0, (what, [(int(tail[i]), int(head[i]), int(load[i]), int(wl[i]))
                                  for i in bad[:5]])
    bad = np.flatnonzero(through != wthr)
    assert bad.size == 0, (what, [(int(v), int(through[v]), int(wthr[v])) for v in bad[:5]])
    assert (st.routed, st.unrouted, st.self_demand) == (ref.routed, ref.unrouted, ref.self_demand)
    assert sum(int(x) for x in load) == ref.hop_weighted, what
    assert st.max_hops == ref.max_hops, (what, st.max_hops, ref.max_hops)
    assert st.narcs == len(tail) and st.ms_load > 0.0
    arcs = {(int(u), int(t)): int(x) for u, t, x in zip(tail, head, load)}
    return arcs, through, st


def test_dense_small_uniform(gpu):
    """Case 1. C1 and the tie graphs, uniform demand, every source."""
    arcs, _, st = check(route_graphs.c1())
    assert len(arcs) == 260 and sum(arcs.values()) == 7_812 and max(arcs.values()) == 165
    assert st.forms == 1 and st.self_demand == 50
    for g in route_graphs.tie_graphs():
        check(g)


def test_dense_source_list_at_an_offset(gpu):
    """Case 1, second half. C1, sources 10..30 only, random demand: a dense source list whose
    rows start at a non-zero row of the tables."""
    g = route_graphs.c1()
    srcs = np.arange(10, 31)
    dem = lr.issue_demand(g.n)[10:31]
    _, _, st = check(g, ALGO_DENSE_FW, sources=srcs, demand=dem)
    assert st.forms == 1 and st.routed > 0


def test_dense_directed_free_order_in_lists(gpu):
    """Case 2. The essential in-lists of a directed dense graph are in no fixed order, so the arc
    of (pred, t) is found by search; a third of the edges are gone, so some demand is unrouted."""
    g = route_graphs.complete_directed_holes()
    _, _, st = check(g, ALGO_DENSE_FW, demand=lr.issue_demand(g.n))
    assert st.unrouted > 0 and st.forms == 1


@pytest.mark.parametrize("ring", [True, False])
def test_sparse_directed(gpu, ring):
    """Case 3."""
    g = route_graphs.directed_random(ring)
    arcs, _, st = check(g, ALGO_SPARSE_SSSP, demand=lr.issue_demand(g.n))
    assert st.self_demand == 84_584
    assert st.unrouted == (0 if ring else 376_938)
    assert len(arcs) == (2_021 if ring else 1_881)


def _wide_flows():
    g = graphs.random_geometric(2000, seed=3)
    srcs = np.unique(np.random.default_rng(5).integers(0, g.n, 60))[:37]
    assert len(srcs) == 37
    rng = np.random.default_rng(8)
    dsrc = np.repeat(srcs, 40).astype(np.int32)
    dtgt = rng.integers(0, g.n, len(dsrc)).astype(np.int32)
    dtgt[::40] = srcs                      # self demand
    dtgt[1::40] = dtgt[2::40]              # a duplicate pair per source
    dval = rng.integers(1 << 32, 1 << 45, len(dsrc), dtype=np.uint64)
    return g, srcs, (dsrc, dtgt, dval)


def test_sparse_source_list_wide_flows(gpu):
    """Case 4. 37 scattered sources and COO demands of 2^32 .. 2^45 each (duplicates and self
    demand among them): every row's total is at least 2^32, so every row keeps u64 flow words in
    LDS (form 2)."""
    g, srcs, dem = _wide_flows()
    _, through, st = check(g, ALGO_SPARSE_SSSP, sources=srcs, demand=dem)
    assert st.forms == 2, st.forms
    assert st.self_demand >= 37 << 32 and int(through.max()) >= 1 << 32


def test_several_row_chunks_dense_free_order(gpu):
    """Case 2 with room for a few rows at a time: the load of every chunk adds into the same
    unsorted in-lists (the essential arcs, which the route export counts)."""
    g = route_graphs.complete_directed_holes()
    ess = build_routes(g.n, True, g.src, g.dst, g.lat_ns, g.loss, algo=ALGO_DENSE_FW)[3].ess_arcs
    _, _, st = check(g, ALGO_DENSE_FW, demand=lr.issue_demand(g.n), load_arcs=ess)
    assert st.unrouted > 0 and st.forms == 1


@pytest.mark.parametrize("ring", [True, False])
def test_several_row_chunks_sparse(gpu, ring):
    """Case 3 with room for a few rows at a time: every chunk's COO demand is re-based to its
    first row."""
    g = route_graphs.directed_random(ring)
    _, _, st = check(g, ALGO_SPARSE_SSSP, demand=lr.issue_demand(g.n), load_arcs=canon_arcs(g))
    assert st.self_demand == 84_584 and st.unrouted == (0 if ring else 376_938)


def test_several_row_chunks_source_list(gpu):
    """Case 4 with room for a few rows at a time: a source list and COO entries (duplicates and
    self demand among them) cut at chunk boundaries; the flow words stay u64."""
    g, srcs, dem = _wide_flows()
    _, through, st = check(g, ALGO_SPARSE_SSSP, sources=srcs, demand=dem, load_arcs=canon_arcs(g))
    assert st.forms == 2, st.forms
    assert st.self_demand >= 37 << 32 and int(through.max()) >= 1 << 32


def test_ring_depth(gpu):
    """Case 5. 1,500 levels, two targets each."""
    g = route_graphs.ring3000()
    arcs, _, st = check(g, sources=np.array([0, 1499]))
    for arc in ((0, 1), (0, 2999), (1499, 1500), (1499, 1498)):
        assert arcs[arc] == 1_500, arc
    assert sum(arcs.values()) == 4_500_000
    assert st.self_demand == 2 and st.max_hops == 1_500 and st.forms == 1


@pytest.mark.parametrize("second,form", [(1, 1), (2, 2)])
def test_form_boundary(gpu, second, form):
    """Case 6. A row total of 2^32 - 1 still fits u32 flow words; 2^32 does not."""
    g = route_graphs.ring3000()
    dem = (np.array([0, 0], np.int32), np.array([10, 11], np.int32),
           np.array([(1 << 32) - 2, second], np.uint64))
    arcs, through, st = check(g, sources=[0], demand=dem)
    assert st.routed == (1 << 32) - 2 + second and st.forms == form, (st.routed, st.forms)
    assert arcs[(0, 1)] == st.routed and arcs[(10, 11)] == second
    assert int(through[10]) == second and int(through[5]) == st.routed


@functools.lru_cache(maxsize=None)
def _ba_past_form1():
    n = lib().srt_routes_stage_max_n(1) + 2000
    assert n > lib().srt_link_load_stage_max_n(1)
    return graphs.barabasi_albert(n, m=3, seed=5)


def test_form_3_and_hubs(gpu):
    """Case 7. A row too long for LDS flow words: u64 words in the workgroup's scratch row. The
    sources are the hubs, whose long in-lists take the wave-wide search."""
    g = _ba_past_form1()
    assert np.bincount(np.concatenate([g.src, g.dst]))[:8].min() >= 32
    _, _, st = check(g, ALGO_SPARSE_SSSP, sources=np.arange(8))
    assert st.forms == 4, st.forms


def test_forms_by_demand_between_the_lds_limits(gpu):
    """Case 7, second half. n between the u64 and the u32 LDS limits: small demands stay in LDS as
    u32 (form 1), demands of 2^32 and more go to scratch (form 3)."""
    L = lib()
    g = graphs.barabasi_albert(20_500, m=3)
    assert L.srt_link_load_stage_max_n(2) < g.n <= L.srt_link_load_stage_max_n(1)
    srcs = np.array([0, 1, 777, 20_499])
    _, _, st = check(g, ALGO_SPARSE_SSSP, sources=srcs)
    assert st.forms == 1, st.forms
    rng = np.random.default_rng(4)
    dsrc = np.repeat(srcs, 50).astype(np.int32)
    dtgt = rng.integers(0, g.n, len(dsrc)).astype(np.int32)
    dval = rng.integers(1 << 32, 1 << 40, len(dsrc), dtype=np.uint64)
    _, _, st = check(g, ALGO_SPARSE_SSSP, sources=srcs, demand=(dsrc, dtgt, dval))
    assert st.forms == 4, st.forms


def test_deep_row_past_the_lds_levels(gpu):
    """A row too long for LDS flow words AND deeper than the levels counted in LDS (4,096): a
    4,100-vertex path hung off the centre of a 36,000-leaf star, from the centre. The level
    counters live in scratch."""
    path, leaves = 4_100, 36_000
    n = 1 + path + leaves
    assert n > lib().srt_link_load_stage_max_n(1)
    chain = np.arange(path)
    src = np.concatenate([chain, np.zeros(leaves, np.int64)]).astype(np.int32)
    dst = np.concatenate([chain + 1, 1 + path + np.arange(leaves)]).astype(np.int32)
    g = graphs.Graph(n, False, src, dst, np.full(len(src), MS, np.int64), np.zeros(len(src)),
                     "lollipop40101")
    arcs, through, st = check(g, ALGO_SPARSE_SSSP, sources=[0])
    assert st.max_hops == path and st.forms == 4
    assert arcs[(0, 1)] == path and arcs[(path - 1, path)] == 1 and int(through[1]) == path - 1


def fan(k, j):
    """Source 0, middles 1..k, target k + 1 and a 3-vertex chain behind it, directed. Arcs middle ->
    target take 1 ms, arcs 0 -> middle 2 ms, except 0 -> j at 1 ms: the target's in-list has k arcs
    and only j's is on a route."""
    t = k + 1
    mids = np.arange(1, k + 1)
    src = np.concatenate([np.zeros(k, np.int64), mids, [t, t + 1, t + 2]]).astype(np.int32)
    dst = np.concatenate([mids, np.full(k, t), [t + 1, t + 2, t + 3]]).astype(np.int32)
    lat = np.concatenate([np.where(mids == j, 1, 2), np.ones(k + 3, np.int64)]) * MS
    return graphs.Graph(k + 5, True, src, dst, lat.astype(np.int64), np.zeros(len(src)),
                        f"fan{k}_{j}")


@pytest.mark.parametrize("algo", [ALGO_DENSE_FW, ALGO_SPARSE_SSSP])
@pytest.mark.parametrize("k", [31, 32, 33, 64, 65])
def test_in_list_lengths_around_the_wave_switch(gpu, k, algo):
    """Case 8. In-lists of 31 arcs are searched by a lane, of 32 and more by the wave, 64 arcs a
    step; the arc looked for is the first or the last of the list."""
    for j in (1, k):
        g = fan(k, j)
        arcs, through, st = check(g, algo, sources=[0])
        t = k + 1
        assert arcs[(j, t)] == 4 and arcs[(0, j)] == 5, (k, j)
        assert [u for (u, v) in arcs if v == t] == [j]
        assert int(through[t]) == 3 and int(through[j]) == 4 and st.max_hops == 5


def test_total_demand_past_u64_is_refused(gpu):
    """Case 9."""
    g = route_graphs.c1()
    dem = (np.array([3, 4, 4], np.int32), np.array([9, 9, 10], np.int32),
           np.array([(1 << 64) - 2, 1, 1], np.uint64))
    with pytest.raises(RuntimeError, match="SRT_E_RANGE"):
        build_link_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss, demand=dem)
    ok = (dem[0], dem[1], np.array([(1 << 64) - 3, 1, 1], np.uint64))
    _, _, st = check(g, sources=[3, 4], demand=ok)
    assert st.routed == (1 << 64) - 1 and st.forms == 3  # row 3 in u64 words, row 4 in u32
