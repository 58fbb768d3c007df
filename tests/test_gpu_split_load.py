"""The split load (splitload.hip) against tests/split_reference.py, through srt_build_split_load,
the device entry points and the drop-in layer (run on an MI355X with -m gpu).

Every case builds its expectation on the CPU first and, unless it says otherwise, asserts there
that the graph has tied pairs and that the split load differs from the canonical load of
load_reference, so no case passes by walking one route per pair. It then compares tail and head
exactly, load and through within the derived tolerance

    rtol = 4 * (arcs + n + nsrc) * 2^-53,  atol = 0          (split_reference.rtol)

(every word is built from non-negative inputs by f64 additions and divisions by positive integers:
at most arcs + n + nsrc roundings on a dependency chain; arcs is the count of the CSR the pass
walks), zeros exactly, and the three totals and tied_pairs exactly. Bitwise comparisons are made
only where every partial sum is exact in any order (dyadic values).
"""
import contextlib
import ctypes

import numpy as np
import pytest

import envelope_reference as er
import level_graphs
import load_reference as lr
import route_graphs
import split_graphs as sg
import split_reference as sr
from conftest import form_env
from route_reference import InArcs
from shadow_amd import graphs
from shadow_amd._lib import (ALGO_AUTO, ALGO_DENSE_FW, ALGO_SPARSE_SSSP, SplitLoadStats, check, lib)
from shadow_amd.topology import (SparseGraph, Topology, build_routes,
                                 build_split_load, ip_to_net)

pytestmark = pytest.mark.gpu
MS = 1_000_000
_EXPECT = {}


def coo_sources(demand):
    return np.unique(np.asarray(demand[0])).astype(np.int64)


def expect(g, sources=None, demand=None, tag="uniform", differs=True):
    """The reference Split of g (cached per graph, source set and demand tag, never modified).
    differs: asserts tied pairs and a split load that is not the canonical one."""
    if isinstance(demand, tuple):
        sources = coo_sources(demand)
    key = (g.name, None if sources is None else tuple(int(s) for s in sources), tag)
    if key not in _EXPECT:
        ref = sr.by_distance(g, sg.distances(g, sources), sources, demand)
        if differs:
            assert ref.tied_pairs > 0, f"{g.name}: no tied pair, the case shows nothing"
            tail, head, load, through = ref.arrays()
            ct, ch, cl, cthr, _ = sr.canonical(g, sources, demand)
            same = (np.array_equal(tail, ct) and np.array_equal(head, ch) and
                    np.array_equal(load, cl) and np.array_equal(through, cthr))
            assert not same, f"{g.name}: the split load is the canonical one"
        _EXPECT[key] = ref
    return _EXPECT[key]


def csr_arcs(g, algo):
    """The arcs of the CSR the pass walks: the canonical in-arcs (sparse) or the essential arcs."""
    if algo == ALGO_DENSE_FW:
        return int(build_routes(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                sources=np.array([0]), algo=ALGO_DENSE_FW)[3].ess_arcs)
    return len(InArcs(g).u)


def assert_split(got, ref, arcs, nsrc, what, bitwise=False):
    tail, head, load, through, st = got
    wt, wh, wl, wthr = ref.arrays()
    assert load.dtype == np.float64 and through.dtype == np.float64
    assert np.array_equal(tail, wt) and np.array_equal(head, wh), (what, len(tail), len(wt))
    assert (load > 0.0).all()
    assert np.array_equal(through == 0.0, wthr == 0.0), what
    rtol = sr.rtol(arcs, ref.n, nsrc)
    for name, a, b in (("load", load, wl), ("through", through, wthr)):
        err = np.abs(a - b) / np.maximum(b, 1e-300)
        print(f"{what}: {name} max rel err {err.max() if len(err) else 0.0:.3g} (rtol {rtol:.3g})")
        if bitwise:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, name)
        else:
            assert np.allclose(a, b, rtol=rtol, atol=0.0), (what, name, float(err.max()))
    assert (st.routed, st.unrouted, st.self_demand) == (ref.routed, ref.unrouted, ref.self_demand), what
    assert st.tied_pairs == ref.tied_pairs, (what, st.tied_pairs, ref.tied_pairs)
    assert st.narcs == len(tail)


def run(g, algo=ALGO_AUTO, sources=None, demand=None, tag="uniform", differs=True, bitwise=False,
        row_bytes=None):
    """row_bytes: what the pass adds per pair to a source row of the chunk budget, the distance
    and reliability rows of a sparse build included. When given, the build runs under SRT_FORM
    memcap=1 (half of what the f64 load words leave of 1 MiB) and must take several chunks with a
    short last one."""
    ref = expect(g, sources, demand, tag, differs)  # on the CPU, before any GPU work
    dense = algo == ALGO_DENSE_FW or (algo == ALGO_AUTO and g.n <= 2048)
    arcs = csr_arcs(g, ALGO_DENSE_FW if dense else ALGO_SPARSE_SSSP)
    with form_env(memcap=1) if row_bytes else contextlib.nullcontext():
        got = build_split_load(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                               sources=None if isinstance(demand, tuple) else sources,
                               demand=demand, algo=algo)
        chunks = lib().srt_last_row_chunks()
    rows = g.n if sources is None and not isinstance(demand, tuple) else len(
        coo_sources(demand) if isinstance(demand, tuple) else sources)
    assert_split(got, ref, arcs, rows, f"{g.name} algo={algo}", bitwise)
    if row_bytes:
        chunk = ((1 << 20) - 8 * arcs) // 2 // (row_bytes * g.n)
        print(f"{g.name} algo={algo}: {rows} rows, {chunk} a chunk, {chunks} chunks")
        assert chunks > 1 and chunks == -(-rows // chunk) and rows % chunk != 0, (chunks, chunk)
    return got, ref


BOTH = pytest.mark.parametrize("algo", [ALGO_SPARSE_SSSP, ALGO_DENSE_FW])


# ---- case 1 ------------------------------------------------------------------------------------
@BOTH
def test_c1_all_rows(gpu, algo):
    """C1 has self-loops: the tables' diagonal holds the path-to-self rule, so D[s][s] must be
    taken as 0 or no direct neighbour of s has a tight arc from it."""
    (_, _, _, _, st), _ = run(route_graphs.c1(), algo)
    assert st.self_demand == 50 and st.unrouted == 0 and st.forms == 1 and st.ms_split > 0.0


# ---- case 2 ------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("name", ["grid56", "hand12"])
def test_dyadic_graphs_bitwise(gpu, name, algo):
    """Every |M| is 1 or 2 and the demand uniform: every partial sum is exact, in any order."""
    g = {"grid56": sg.grid56, "hand12": sg.hand12}[name]()
    (_, _, _, _, st), _ = run(g, algo, bitwise=True)
    if name == "hand12":  # M(0, 3) = {1}: 2 -> 3 is tight from 0 too, and gets nothing from 0
        assert st.unrouted == 12 * 8
        (tail, head, load, _, st), _ = run(g, algo, sources=np.array([0]), differs=False,
                                           bitwise=True)
        assert list(zip(tail.tolist(), head.tolist(), load.tolist())) == [
            (0, 1, 2.0), (0, 2, 1.0), (1, 3, 1.0)] and st.tied_pairs == 0


# ---- case 3 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("directed", [False, True])
def test_core_tail(gpu, directed):
    """Tied at every rung of the braided tail, a chain of 12 members and more; the directed form's
    essential in-lists come in free order."""
    g = level_graphs.core_tail(18, directed=directed)
    assert 220 <= g.n <= 240, g.n
    D = sg.distances(g)
    assert er.envelope(g, D).max_sweeps >= 12, "a chain of members at least 12 deep"
    run(g, ALGO_DENSE_FW)


# ---- case 4 ------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("k", [31, 32, 33, 64, 65, 130])
def test_fan(gpu, k, algo):
    """|M| = k on both sides of the switch to the wave-wide walk (32 arcs) and of a 64-arc step:
    one unit to each fan's t puts 1 / k on every arm."""
    g, srcs, tgts = sg.fans(k)
    dem = (srcs.astype(np.int32), tgts.astype(np.int32), np.ones(2, np.uint64))
    (tail, head, load, through, st), ref = run(g, algo, demand=dem, tag="fan_t",
                                               bitwise=k in (32, 64))
    assert len(load) == 4 * k and st.routed == 2 and st.tied_pairs == 2
    assert (ref.arrays()[2] == 1.0 / k).all()
    assert np.allclose(load, 1.0 / k, rtol=sr.rtol(4 * k, g.n, 2), atol=0.0)
    arms = np.ones(g.n, bool)
    arms[srcs] = arms[tgts] = False
    assert np.allclose(through[arms], 1.0 / k, rtol=sr.rtol(4 * k, g.n, 2), atol=0.0)
    assert not through[~arms].any()


# ---- case 5 ------------------------------------------------------------------------------------
@BOTH
@pytest.mark.parametrize("which", [0, 1])
def test_untied_is_the_link_load(gpu, which, algo):
    """No tied pair: every |M| is 1 and the split load is the link load's integers, bitwise."""
    g = sg.untied()[which]
    dem = lr.issue_demand(g.n)
    (tail, head, load, through, st), ref = run(g, algo, demand=dem, tag="issue", differs=False,
                                               bitwise=True)
    assert st.tied_pairs == 0
    ct, ch, cl, cthr, cref = sr.canonical(g, demand=dem)
    assert np.array_equal(tail, ct) and np.array_equal(head, ch)
    assert np.array_equal(load.view(np.uint64), cl.view(np.uint64))
    assert np.array_equal(through.view(np.uint64), cthr.view(np.uint64))
    assert (st.routed, st.unrouted, st.self_demand) == (cref.routed, cref.unrouted, cref.self_demand)


# ---- case 6 ------------------------------------------------------------------------------------
def test_zero_flows_release_their_members(gpu):
    """The ring of 3,000: one unit per row, at the antipode for source 0 (tied), so every other
    target carries f == 0 and must still release its members, 1,500 sweeps deep."""
    g = route_graphs.ring3000()
    dem = (np.array([0, 1, 1499, 2999], np.int32), np.array([1500, 10, 1400, 2990], np.int32),
           np.ones(4, np.uint64))
    (tail, head, load, through, st), _ = run(g, demand=dem, tag="one_unit", bitwise=True)
    arcs = {(int(u), int(t)): float(x) for u, t, x in zip(tail, head, load)}
    for arc in ((0, 1), (700, 701), (1499, 1500), (0, 2999), (2300, 2299), (1501, 1500)):
        assert arcs[arc] == 0.5, arc
    assert through[700] == 0.5 and through[2300] == 0.5 and through[1500] == 0.0
    assert st.routed == 4 and st.forms == 1


# ---- case 7 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["directed_noring", "holes"])
def test_unreachable_and_self_demand(gpu, name):
    """Demand at unreachable targets and at the source itself is counted exactly and carries no
    load."""
    if name == "holes":
        g, algo = route_graphs.complete_directed_holes(), ALGO_DENSE_FW
    else:
        g, algo = route_graphs.directed_random(False), ALGO_SPARSE_SSSP
    dem = lr.issue_demand(g.n)
    (_, _, load, _, st), ref = run(g, algo, demand=dem, tag="issue")
    assert st.self_demand == int(np.diagonal(dem).sum()) and st.self_demand > 0
    assert st.unrouted > 0 and st.routed + st.unrouted + st.self_demand == int(dem.sum())


# ---- case 8 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sparse", "dense", "source_list"])
def test_several_row_chunks(gpu, case):
    """Room for a few rows at a time: the pass adds 8 B a pair (the u64 demand row) beside a sparse
    build's distance and reliability rows (12 B); the sums across the chunks match the one-chunk
    reference."""
    if case == "sparse":
        run(route_graphs.directed_random(True), ALGO_SPARSE_SSSP, demand=lr.issue_demand(300),
            tag="issue", row_bytes=20)
    elif case == "dense":
        run(graphs.complete_graph(300, seed=11, lat_max=3), ALGO_DENSE_FW, row_bytes=8)
    else:
        g = graphs.random_geometric(2000, seed=3)
        srcs = np.unique(np.random.default_rng(5).integers(0, g.n, 60))[:37]
        run(g, ALGO_SPARSE_SSSP, sources=srcs, row_bytes=20)


# ---- case 9 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,past", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_staging_form_boundaries(gpu, form, past):
    """n at srt_split_load_stage_max_n(form) and just past it, on a graph whose hubs' long in-lists
    are walked by the wave."""
    n = lib().srt_split_load_stage_max_n(form) + past
    g = graphs.barabasi_albert(n, m=3, seed=5)
    (_, _, _, _, st), _ = run(g, ALGO_SPARSE_SSSP, sources=np.arange(4))
    assert st.forms == 1 << (form + past - 1), st.forms


def test_staging_form_3_at_its_limit(gpu):
    """n = srt_split_load_stage_max_n(3): the bitmaps fill the dynamic LDS exactly. Four sources on
    a hub graph (in-lists of up to 33,000 arcs, walked by the wave). graphs.barabasi_albert takes
    half a minute at this size, so the graph is split_graphs.skewed_attachment, and the canonical
    load (a Python loop per target) is not built: the case asserts tied pairs alone."""
    n = lib().srt_split_load_stage_max_n(3)
    g = sg.skewed_attachment(n, m=3, seed=5)
    assert np.bincount(np.concatenate([g.src, g.dst]))[:4].min() >= 2048
    (_, _, _, _, st), ref = run(g, ALGO_SPARSE_SSSP, sources=np.arange(4), differs=False)
    assert ref.tied_pairs > 0 and st.forms == 4, st.forms


def test_staging_form_3_is_the_limit(gpu):
    """The pass's own limit is not below the envelope's, and a graph just past it is refused."""
    import torch
    L = lib()
    top = L.srt_split_load_stage_max_n(3)
    assert top >= L.srt_envelope_stage_max_n(3) and L.srt_split_load_stage_max_n(4) == 0
    n = top + 1
    idx = np.arange(n - 1, dtype=np.int32)
    g = SparseGraph(n, False, idx, idx + 1, np.full(n - 1, MS, np.int64), np.zeros(n - 1))
    try:
        lat = torch.zeros((1, n), dtype=torch.int32, device="cuda")
        dem = torch.ones((1, n), dtype=torch.int64, device="cuda")
        load = torch.zeros(g.arcs, dtype=torch.float64, device="cuda")
        thr = torch.zeros(n, dtype=torch.float64, device="cuda")
        tot = torch.zeros(3, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError, match="SRT_E_RANGE"):
            g.split_load_rows(lat.data_ptr(), 1, dem.data_ptr(), load.data_ptr(), thr.data_ptr(),
                              tot.data_ptr())
    finally:
        g.free()


# ---- case 10 -----------------------------------------------------------------------------------
def by_arc(rowptr, tails, load):
    """{(tail, head): load} of the CSR positions with load > 0."""
    head = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    on = np.flatnonzero(load > 0.0)
    return {(int(tails[k]), int(head[k])): float(load[k]) for k in on}


def assert_arcs(got, ref, rtol, what):
    tail, head, load, _ = ref.arrays()
    want = {(int(u), int(t)): float(x) for u, t, x in zip(tail, head, load)}
    assert got.keys() == want.keys(), (what, len(got), len(want))
    a = np.array([got[k] for k in want])
    assert np.allclose(a, load, rtol=rtol, atol=0.0), what


def test_dense_device_row_range(gpu):
    """srt_split_load_dense_device on rows [128, 300) of the n = 300 graph, device resident: the
    essential CSR comes out beside the load."""
    import torch
    n, ld, row0 = 300, 384, 128
    g = graphs.complete_graph(n, seed=11, lat_max=3)
    srcs = np.arange(row0, n)
    ref = expect(g, srcs)
    L = lib()
    w = torch.empty((ld, ld), dtype=torch.int32, device="cuda")
    r = torch.empty((ld, ld), dtype=torch.float64, device="cuda")
    assert L.srt_gen_complete_device(n, ld, 0, ld, 11, 3, 10, 500, w.data_ptr(), r.data_ptr(),
                                     None) == 0
    lat = torch.empty_like(w)
    rel = torch.empty_like(r)
    assert L.srt_dense_build_device(n, ld, 0, w.data_ptr(), r.data_ptr(), lat.data_ptr(),
                                    rel.data_ptr(), None, 0, None) == 0
    cap = n * n
    dem = torch.ones((n - row0, n), dtype=torch.int64, device="cuda")
    rowptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    tails = torch.empty(cap, dtype=torch.int32, device="cuda")
    load = torch.full((cap,), -5.0, dtype=torch.float64, device="cuda")
    thr = torch.full((n,), -5.0, dtype=torch.float64, device="cuda")
    tot = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    narcs = ctypes.c_int64()
    st = SplitLoadStats()
    check(L.srt_split_load_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), row0, n - row0,
                                        dem.data_ptr(), n, cap, rowptr.data_ptr(), tails.data_ptr(),
                                        load.data_ptr(), ctypes.byref(narcs), thr.data_ptr(),
                                        tot.data_ptr(), None, ctypes.byref(st)),
          "srt_split_load_dense_device")
    torch.cuda.synchronize()
    k = narcs.value
    rp = rowptr.cpu().numpy()
    assert 0 < k <= cap and rp[0] == 0 and rp[n] == k
    rtol = sr.rtol(k, n, n - row0)
    assert_arcs(by_arc(rp, tails.cpu().numpy()[:k], load.cpu().numpy()[:k]), ref, rtol, "dense rows")
    assert np.allclose(thr.cpu().numpy(), ref.through, rtol=rtol, atol=0.0)
    assert tot.cpu().numpy().tolist() == [ref.routed, ref.unrouted, ref.self_demand]
    assert st.tied_pairs == ref.tied_pairs and st.forms == 1 and st.ms_split > 0.0


def test_sparse_device_rows(gpu):
    """SparseGraph.split_load_rows over rows srt_sparse_graph_rows_list made: a source list, rows of
    stride > n; two calls on disjoint source sets add up to the reference of their union; a single
    source sends out what it routes."""
    import torch
    g = route_graphs.directed_random(True)
    n, ldl, ldd = g.n, g.n + 20, g.n + 12
    srcs = np.array([3, 17, 18, 250, 299], np.int32)
    ref = expect(g, srcs)
    graph = SparseGraph(n, True, g.src, g.dst, g.lat_ns, g.loss)
    try:
        rp_ptr, tl_ptr = graph.in_arcs()
        arcs = graph.arcs
        dsrc = torch.tensor(srcs, device="cuda")
        lat_n = torch.empty((len(srcs), n), dtype=torch.int32, device="cuda")
        rel = torch.empty((len(srcs), n), dtype=torch.float64, device="cuda")
        graph.rows_list(dsrc.data_ptr(), len(srcs), lat_n.data_ptr(), rel.data_ptr())
        lat = torch.full((len(srcs), ldl), -1, dtype=torch.int32, device="cuda")
        lat[:, :n] = lat_n
        dem = torch.full((len(srcs), ldd), 99, dtype=torch.int64, device="cuda")
        dem[:, :n] = 1
        load = torch.zeros(arcs, dtype=torch.float64, device="cuda")
        thr = torch.zeros(n, dtype=torch.float64, device="cuda")
        tot = torch.zeros(3, dtype=torch.int64, device="cuda")
        tied = 0
        for a, b in ((0, 2), (2, 5)):
            st = SplitLoadStats()
            graph.split_load_rows(lat[a:].data_ptr(), b - a, dem[a:].data_ptr(), load.data_ptr(),
                                  thr.data_ptr(), tot.data_ptr(), srcs_ptr=dsrc[a:].data_ptr(),
                                  ldl=ldl, ldd=ldd, stats=st)
            tied += st.tied_pairs
            assert st.forms == 1
        torch.cuda.synchronize()
        ia = InArcs(g)
        assert arcs == len(ia.u)
        rtol = sr.rtol(arcs, n, len(srcs))
        got = load.cpu().numpy()
        assert np.array_equal(got == 0.0, ref.load == 0.0)  # the graph's own in-arc order
        assert np.allclose(got, ref.load, rtol=rtol, atol=0.0)
        assert np.allclose(thr.cpu().numpy(), ref.through, rtol=rtol, atol=0.0)
        assert tot.cpu().numpy().tolist() == [ref.routed, ref.unrouted, ref.self_demand]
        assert tied == ref.tied_pairs
        # one source: what leaves s is what it routes
        load.zero_(), thr.zero_(), tot.zero_()
        graph.split_load_rows(lat[1:].data_ptr(), 1, dem[1:].data_ptr(), load.data_ptr(),
                              thr.data_ptr(), tot.data_ptr(), srcs_ptr=dsrc[1:].data_ptr(), ldl=ldl,
                              ldd=ldd)
        torch.cuda.synchronize()
        out = float(load.cpu().numpy()[ia.u == 17].sum())
        routed = int(tot.cpu().numpy()[0])
        assert routed == n - 1 and abs(out - routed) <= rtol * routed, (out, routed)
    finally:
        graph.free()


# ---- case 11 -----------------------------------------------------------------------------------
def test_refusals_and_direct_mode(gpu):
    g = route_graphs.c1()
    dem = (np.array([3, 4, 4], np.int32), np.array([9, 9, 10], np.int32),
           np.array([(1 << 53) - 2, 1, 1], np.uint64))
    with pytest.raises(RuntimeError, match="SRT_E_RANGE"):
        build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss, demand=dem)
    ok = (dem[0], dem[1], np.array([(1 << 53) - 3, 1, 1], np.uint64))
    (_, _, _, _, st), _ = run(g, demand=ok, tag="2^53-1", differs=False)
    assert st.routed == (1 << 53) - 1
    # distances that need u64 rows (test_gpu_wide.py's chain: ~4 ms hops in odd nanoseconds)
    rng = np.random.default_rng(5)
    n = 600
    a = np.arange(n - 1)
    wide = graphs.Graph(n, False, a.astype(np.int32), (a + 1).astype(np.int32),
                        (rng.integers(3_500_000, 4_500_000, n - 1) | 1).astype(np.int64),
                        np.zeros(n - 1), "split_wide600")
    with pytest.raises(RuntimeError, match="SRT_E_RANGE"):
        build_split_load(wide.n, False, wide.src, wide.dst, wide.lat_ns, wide.loss,
                         sources=np.array([0]))
    # direct mode: every pair is its own arc
    srcs = np.array([0, 7, 49])
    tail, head, load, through, st = build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                     sources=srcs, use_shortest_path=False)
    want = [(int(s), t) for s in srcs for t in range(g.n) if t != s]
    assert list(zip(tail.tolist(), head.tolist())) == want and (load == 1.0).all()
    assert not through.any() and (st.routed, st.unrouted, st.self_demand) == (3 * 49, 0, 3)
    ring = route_graphs.ring3000()  # not complete: the table build's error
    with pytest.raises(RuntimeError, match="SRT_E_INVALID"):
        build_split_load(ring.n, False, ring.src, ring.dst, ring.lat_ns, ring.loss,
                         use_shortest_path=False)


# ---- case 12 -----------------------------------------------------------------------------------
def test_topology_split_load(gpu):
    """Topology.split_load() after a few send_packets equals build_split_load on the COO demand of
    the counters, and leaves Topology.link_load() and its build counter as they were."""
    grid = sg.grid56()
    verts = list(range(grid.n))
    ip = lambda v: f"100.8.{v}.1"
    top = Topology.from_gml(graphs.to_gml(grid))
    try:
        n, directed, src, dst, lat_ns, loss = top.edges()
        for v in verts:
            assert top.attach(ip(v), 1, ip_hint=f"11.0.0.{v + 1}")[0] == v
        rng = np.random.default_rng(21)
        a, b = rng.integers(0, len(verts), 3000), rng.integers(0, len(verts), 3000)
        delivered, _ = top.send_packets(np.array([ip_to_net(ip(verts[i])) for i in a], np.uint32),
                                        np.array([ip_to_net(ip(verts[i])) for i in b], np.uint32),
                                        rng.random(3000))
        assert delivered.any()
        dem = {}
        for i, u in enumerate(verts):
            for v in verts[i:]:
                cnt = top.packet_count(ip(u), ip(v))
                if cnt:
                    frm = top.path_source(ip(u), ip(v))
                    dem[(frm, v if frm == u else u)] = cnt
        keys = sorted(dem)
        coo = (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32),
               np.array([dem[k] for k in keys], np.uint64))
        before = top.link_load()
        builds = top.link_load_builds()
        got = top.split_load()
        want = build_split_load(n, directed, src, dst, lat_ns, loss, demand=coo)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        g = graphs.Graph(n, directed, src, dst, lat_ns, loss, "split_grid5x6.gml")
        arcs = csr_arcs(g, ALGO_DENSE_FW)
        rtol = sr.rtol(arcs, n, len(np.unique(coo[0])))
        assert np.allclose(got[2], want[2], rtol=rtol, atol=0.0)
        assert np.allclose(got[3], want[3], rtol=rtol, atol=0.0)
        assert np.array_equal(got[3] == 0.0, want[3] == 0.0)
        for name in ("routed", "unrouted", "self_demand", "tied_pairs", "narcs"):
            assert getattr(got[4], name) == getattr(want[4], name), name
        assert got[4].routed > 0 and got[4].self_demand > 0 and got[4].tied_pairs > 0
        ref = expect(g, demand=coo, tag="counters")
        assert_split(got, ref, arcs, len(np.unique(coo[0])), "topology")
        assert top.link_load_builds() == builds
        after = top.link_load()
        assert all(np.array_equal(x, y) for x, y in zip(before[:4], after[:4]))
        assert top.link_load_builds() == builds + 1
    finally:
        top.free()
