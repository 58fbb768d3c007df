"""The route export (routes.hip) against the CPU oracle, through srt_build_routes and the device
entry points (run on an MI355X with -m gpu).

pred is compared with oracle.sssp_rows(want_pred=True)["pred"] exactly, over every row asked;
first and hops with route_reference.walk of the oracle's predecessors; stats.max_hops with the
reference's maximum. Integers only: no tolerance anywhere.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import oracle
from conftest import form_env
import route_graphs
import route_reference as rr
from shadow_amd import graphs
from shadow_amd._lib import (ALGO_AUTO, ALGO_DENSE_FW, ALGO_SPARSE_SSSP, BuildOpts, Edges,
                             RouteStats, check, lib)
from shadow_amd.topology import build_routes, build_tables

pytestmark = pytest.mark.gpu
MS = 1_000_000
_EXPECT = {}


def expect(g, sources=None):
    """(pred, first, hops) int32 [k, n] of the oracle for `sources` (None: every vertex), cached
    per graph and source set."""
    key = (g.name, None if sources is None else tuple(int(s) for s in sources))
    if key not in _EXPECT:
        el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
        if sources is None:
            srcs = np.arange(g.n)
            pred = oracle.sssp_rows(el, nthreads=8, want_pred=True)["pred"]
        else:  # sssp_list returns no predecessors: one row at a time
            srcs = np.asarray(sources)
            pred = np.concatenate([oracle.sssp_rows(el, int(s), int(s) + 1, want_pred=True)["pred"]
                                   for s in srcs])
        walks = [rr.walk(pred[i], int(s)) for i, s in enumerate(srcs)]
        _EXPECT[key] = (pred, np.stack([w[1] for w in walks]), np.stack([w[0] for w in walks]))
    return _EXPECT[key]


def assert_routes(got, want, what, stats=None):
    for name, a, b in zip(("pred", "first", "hops"), got, want):
        bad = np.argwhere(a != b)
        assert bad.size == 0, (f"{what}: {len(bad)} {name} entries differ, first "
                               f"{[(int(i), int(j), int(a[i, j]), int(b[i, j])) for i, j in bad[:5]]}")
    if stats is not None:
        assert stats.max_hops == int(want[2].max()), (what, stats.max_hops, int(want[2].max()))


def run(g, algo=ALGO_AUTO, sources=None, row_bytes=None, **kw):
    """row_bytes: what one source row takes of the chunk budget per vertex. When given, the build
    runs under SRT_FORM memcap=1: 1 MiB free is below the reserve, so the budget is half of it, and
    the rows must come in three chunks or more with a short last one."""
    with form_env(memcap=1) if row_bytes else contextlib.nullcontext():
        pred, first, hops, st = build_routes(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                             sources=sources, algo=algo, **kw)
        chunks = lib().srt_last_row_chunks()
    assert_routes((pred, first, hops), expect(g, sources), f"{g.name} algo={algo}", st)
    if row_bytes:
        rows, chunk = len(pred), (1 << 19) // (row_bytes * g.n)
        print(f"{g.name} algo={algo}: {rows} rows, {chunk} a chunk, {chunks} chunks")
        assert chunks >= 3 and chunks == -(-rows // chunk) and rows % chunk != 0, (chunks, chunk)
    return pred, first, hops, st


def test_c1_all_rows(gpu):
    """Case 1. C1 has self-loops: the tables' diagonal holds the path-to-self rule, and a kernel
    that read D[s][s] raw would miss every direct neighbour's predecessor."""
    g = route_graphs.c1()
    pred, first, hops, st = run(g)
    assert st.stage_forms == 1 and st.ess_arcs > 0
    lat, rel, _ = build_tables(g.n, False, g.src, g.dst, g.lat_ns, g.loss)
    arcs = rr.InArcs(g)
    for s in range(g.n):
        got = rr.rel_along(g, pred[s], s, arcs)
        off = np.arange(g.n) != s
        assert np.array_equal(got[off], rel[s][off]), f"reliability along the routes of {s}"
    # a tight direct arc s -> t offers the key (0, s): nothing ties with distance 0, so pred == s
    W = np.full((g.n, g.n), -1, np.int64)
    off = g.src != g.dst
    W[g.src[off], g.dst[off]] = g.lat_ns[off]
    W[g.dst[off], g.src[off]] = g.lat_ns[off]
    tight = (W == lat.astype(np.int64)) & ~np.eye(g.n, dtype=bool)
    assert tight.sum() > g.n
    assert (pred[tight] == np.nonzero(tight)[0]).all()
    assert (first[tight] == np.nonzero(tight)[1]).all() and (hops[tight] == 1).all()


@pytest.mark.parametrize("n", [640, 300])
def test_dense_tied_complete(gpu, n):
    """Case 2. 1-3 ms complete graph: about half the pairs are tied, so a wrong tie order shows at
    once; n = 300 has ld 384, padding rows and columns."""
    g = graphs.complete_graph(n, seed=11, lat_max=3)
    _, _, _, st = run(g, ALGO_DENSE_FW)
    assert 0 < st.ess_arcs <= n * (n - 1)


@pytest.mark.parametrize("holes", [False, True])
def test_dense_directed(gpu, holes):
    """Case 3. Directed dense graph (the in-lists come from the transpose of the rows); with a
    third of the edges removed some pairs are unreachable: -1 in all three outputs."""
    g = route_graphs.complete_directed_holes() if holes else graphs.complete_directed(
        300, seed=12, lat_max=20)
    pred, first, hops, _ = run(g, ALGO_DENSE_FW)
    none = pred < 0
    np.fill_diagonal(none, False)
    assert none.any() == holes
    assert (first[none] == -1).all() and (hops[none] == -1).all()


@pytest.mark.parametrize("ring", [True, False])
def test_sparse_directed(gpu, ring):
    """Case 4."""
    g = route_graphs.directed_random(ring)
    pred, first, hops, _ = run(g, ALGO_SPARSE_SSSP)
    none = pred < 0
    np.fill_diagonal(none, False)
    assert none.any() == (not ring)
    assert (first[none] == -1).all() and (hops[none] == -1).all()


def test_sparse_scattered_sources(gpu):
    """Case 5. A source list, and a row count that is no multiple of 64."""
    g = graphs.random_geometric(2000, seed=3)
    srcs = np.unique(np.random.default_rng(5).integers(0, g.n, 60))[:37]
    assert len(srcs) == 37
    run(g, ALGO_SPARSE_SSSP, sources=srcs)


@pytest.mark.parametrize("case", ["sparse", "dense", "source_list"])
def test_several_row_chunks(gpu, case):
    """Cases 4, 2 and 5 with room for a few rows at a time: the chunks' row offsets, the short last
    chunk and the per-chunk downloads. A sparse row takes its distance and reliability (12 B a
    vertex) beside the three outputs; a dense build's tables are already on the device."""
    if case == "sparse":
        run(route_graphs.directed_random(True), ALGO_SPARSE_SSSP, row_bytes=24)
    elif case == "dense":
        run(graphs.complete_graph(300, seed=11, lat_max=3), ALGO_DENSE_FW, row_bytes=12)
    else:
        g = graphs.random_geometric(2000, seed=3)
        srcs = np.unique(np.random.default_rng(5).integers(0, g.n, 60))[:37]
        run(g, ALGO_SPARSE_SSSP, sources=srcs, row_bytes=24)


@functools.lru_cache(maxsize=None)
def _ba_past_form1():
    n = lib().srt_routes_stage_max_n(1) + 2000
    assert n <= lib().srt_routes_stage_max_n(2)
    return graphs.barabasi_albert(n, m=3, seed=5)


def test_staging_form_2(gpu):
    """Case 6. A row that does not fit the LDS as u32 and stays below 0xFFFF quanta: form 2 only.
    Sources [0, 8) are the hubs (long in-lists: the wave-wide walk)."""
    g = _ba_past_form1()
    _, _, _, st = run(g, ALGO_SPARSE_SSSP, sources=np.arange(8))
    assert st.stage_forms == 2, st.stage_forms


def test_staging_form_3(gpu):
    """Case 6, with one more vertex hung off vertex 5 by a 70 s edge: its distance passes 0xFFFF
    quanta in every row, so every row is read from global memory."""
    b = _ba_past_form1()
    g = graphs.Graph(b.n + 1, False, np.append(b.src, 5).astype(np.int32),
                     np.append(b.dst, b.n).astype(np.int32), np.append(b.lat_ns, 70_000 * MS),
                     np.append(b.loss, 0.01), b.name + "_far")
    _, _, hops, st = run(g, ALGO_SPARSE_SSSP, sources=np.arange(8))
    assert st.stage_forms == 4, st.stage_forms
    assert (hops[:, b.n] >= 1).all()


def test_ring_depth(gpu):
    """Case 7. 1,500 hops deep; the tied antipode takes the lower neighbour."""
    g = route_graphs.ring3000()
    pred, first, hops, st = run(g, sources=np.array([0, 1499]))
    assert st.max_hops == 1500 and hops[0].max() == 1500
    assert pred[0][1500] == 1499 and first[0][1500] == 1
    # 1499's antipode 2999 is tied between 2998 and 0 (both 1,499 away): the lower index wins
    assert pred[1][2999] == 0 and hops[1][2999] == 1500 and first[1][2999] == 1498


def test_direct_mode(gpu):
    """Case 8. use_shortest_path = 0: every pair is its own edge."""
    g = route_graphs.c1()
    pred, first, hops, _ = build_routes(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                        use_shortest_path=False)
    s, t = np.meshgrid(np.arange(g.n), np.arange(g.n), indexing="ij")
    diag = s == t
    assert np.array_equal(pred, np.where(diag, -1, s))
    assert np.array_equal(first, np.where(diag, -1, t))
    assert np.array_equal(hops, np.where(diag, 0, 1))
    ring = route_graphs.ring3000()  # not complete: the table build's error
    with pytest.raises(RuntimeError, match="SRT_E_INVALID"):
        build_routes(ring.n, False, ring.src, ring.dst, ring.lat_ns, ring.loss,
                     use_shortest_path=False)


def test_submillisecond_quanta(gpu):
    """Case 9. 0.3-0.7 ms edges: the quantum is 100 us, the routes follow the integer quanta."""
    g = route_graphs.submillisecond()
    run(g)
    run(g, ALGO_SPARSE_SSSP)


def test_dense_device_row_range(gpu):
    """Case 10. srt_routes_dense_device on rows [128, 300) of the n = 300 graph, device resident:
    the asked rows exact, every other row and the columns >= n untouched."""
    import torch
    n, ld, row0 = 300, 384, 128
    L = lib()
    w = torch.empty((ld, ld), dtype=torch.int32, device="cuda")
    r = torch.empty((ld, ld), dtype=torch.float64, device="cuda")
    assert L.srt_gen_complete_device(n, ld, 0, ld, 11, 3, 10, 500, w.data_ptr(), r.data_ptr(),
                                     None) == 0
    lat = torch.empty_like(w)
    rel = torch.empty_like(r)
    assert L.srt_dense_build_device(n, ld, 0, w.data_ptr(), r.data_ptr(), lat.data_ptr(),
                                    rel.data_ptr(), None, 0, None) == 0
    SENT = -77
    outs = [torch.full((ld, ld), SENT, dtype=torch.int32, device="cuda") for _ in range(3)]
    st = RouteStats()
    check(L.srt_routes_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), row0, n - row0,
                                    *[o[row0:].data_ptr() for o in outs], ld, None,
                                    ctypes.byref(st)), "srt_routes_dense_device")
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    want = expect(graphs.complete_graph(n, seed=11, lat_max=3))
    assert_routes([a[row0:n, :n] for a in got], [b[row0:n] for b in want], "row range")
    assert st.max_hops == int(want[2][row0:n].max()) and st.stage_forms == 1 and st.ess_arcs > 0
    for a in got:
        assert (a[:row0] == SENT).all() and (a[n:] == SENT).all() and (a[row0:n, n:] == SENT).all()


def _raw_build(g, algo, which, sources=None):
    """srt_build_routes with only output `which` (0 pred, 1 first, 2 hops) given."""
    e = Edges(g.n, int(bool(g.directed)), len(g.src), g.src.ctypes.data, g.dst.ctypes.data,
              g.lat_ns.ctypes.data, g.loss.ctypes.data)
    o = BuildOpts(0, algo, 1, 0)
    out = np.full((g.n, g.n), -5, np.int32)
    ptrs = [None, None, None]
    ptrs[which] = out.ctypes.data
    st = RouteStats()
    check(lib().srt_build_routes(ctypes.byref(e), ctypes.byref(o), g.n, None, *ptrs,
                                 ctypes.byref(st)), "srt_build_routes")
    return out, st


@pytest.mark.parametrize("which", [0, 1, 2])
def test_null_outputs(gpu, which):
    """Case 11. Each output alone, the other two NULL: dense and sparse front ends."""
    for g, algo in ((route_graphs.c1(), ALGO_DENSE_FW),
                    (route_graphs.directed_random(False), ALGO_SPARSE_SSSP)):
        out, st = _raw_build(g, algo, which)
        want = expect(g)
        assert np.array_equal(out, want[which]), (g.name, which)
        assert st.max_hops == int(want[2].max())


def test_sparse_device_rows(gpu):
    """srt_routes_rows_device (SparseGraph.routes_rows) over rows srt_sparse_graph_rows_list made:
    a source list with lat rows of stride > n and outputs of stride > n."""
    import torch
    from shadow_amd.topology import SparseGraph
    g = route_graphs.directed_random(True)
    n, ldo = g.n, g.n + 20
    sg = SparseGraph(n, True, g.src, g.dst, g.lat_ns, g.loss)
    srcs = np.array([3, 17, 18, 250, 299], np.int32)
    dsrc = torch.tensor(srcs, device="cuda")
    lat = torch.empty((len(srcs), n), dtype=torch.int32, device="cuda")
    rel = torch.empty((len(srcs), n), dtype=torch.float64, device="cuda")
    sg.rows_list(dsrc.data_ptr(), len(srcs), lat.data_ptr(), rel.data_ptr())
    outs = [torch.full((len(srcs), ldo), -9, dtype=torch.int32, device="cuda") for _ in range(3)]
    st = RouteStats()
    sg.routes_rows(lat.data_ptr(), len(srcs), *[o.data_ptr() for o in outs],
                   srcs_ptr=dsrc.data_ptr(), ldo=ldo, stats=st)
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    want = expect(g)
    assert_routes([a[:, :n] for a in got], [b[srcs] for b in want], "device rows")
    assert all((a[:, n:] == -9).all() for a in got)
    assert st.max_hops == int(want[2][srcs].max()) and st.stage_forms == 1
    sg.free()
