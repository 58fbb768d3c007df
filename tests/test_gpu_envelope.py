"""The reliability envelope (envelope.hip) against tests/envelope_reference.py, through
srt_build_rel_envelope and the device entry points (run on an MI355X with -m gpu).

Every comparison is bitwise, on u64 views of lo and hi, plus the three counts of the stats. Every
graph is first checked on the CPU (expect) to have sensitive pairs, so no case passes by computing
one path per pair; where a case needs more of its graph, its helper asserts that too.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import envelope_reference as er
import level_graphs
import oracle
import route_graphs
import route_reference as rr
from conftest import form_env
from shadow_amd import graphs
from shadow_amd._lib import (ALGO_AUTO, ALGO_DENSE_FW, ALGO_SPARSE_SSSP, EnvelopeStats, check, lib)
from shadow_amd.topology import build_rel_envelope, build_tables

pytestmark = pytest.mark.gpu
MS = 1_000_000
_EXPECT = {}


def expect(g, sources=None):
    """The reference Envelope of g for `sources` (None: every vertex), cached per graph and source
    set; asserts that some pair of it is sensitive."""
    key = (g.name, None if sources is None else tuple(int(s) for s in sources))
    if key not in _EXPECT:
        el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
        if sources is None:
            srcs = np.arange(g.n)
            lat = oracle.table(el, True, oracle.ORC_INT_NS, 8, raw=True)["lat_int"]
        else:
            srcs = np.asarray(sources)
            lat = oracle.sssp_list(el, srcs, nthreads=8)["lat_int"]
        env = er.envelope(g, rr.distances_of_oracle(lat, srcs), srcs)
        assert env.sensitive_pairs > 0, f"{g.name}: no sensitive pair, the case shows nothing"
        assert env.sensitive_pairs <= env.exposed_pairs and env.tied_pairs <= env.exposed_pairs
        for a in (env.lo, env.hi):
            a.setflags(write=False)
        _EXPECT[key] = env
    return _EXPECT[key]


def assert_envelope(lo, hi, st, env, what):
    for name, a, b in (("lo", lo, env.lo), ("hi", hi, env.hi)):
        if a is None:
            continue
        bad = np.argwhere(a.view(np.uint64) != b.view(np.uint64))
        assert bad.size == 0, (f"{what}: {len(bad)} {name} entries differ, first "
                               f"{[(int(i), int(j), float(a[i, j]), float(b[i, j])) for i, j in bad[:5]]}")
    if st is not None:
        got = (st.tied_pairs, st.exposed_pairs, st.sensitive_pairs, st.max_sweeps)
        want = (env.tied_pairs, env.exposed_pairs, env.sensitive_pairs, env.max_sweeps)
        assert got == want, f"{what}: (tied, exposed, sensitive, max_sweeps) {got}, reference {want}"


def run(g, algo=ALGO_AUTO, sources=None, row_bytes=None):
    """row_bytes: what one source row takes of the chunk budget per vertex. When given, the build
    runs under SRT_FORM memcap=1 (a budget of 1 << 19 bytes, as test_gpu_routes.py) and must take
    several chunks with a short last one."""
    env = expect(g, sources)  # on the CPU, before any GPU work
    with form_env(memcap=1) if row_bytes else contextlib.nullcontext():
        lo, hi, st = build_rel_envelope(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                        sources=sources, algo=algo)
        chunks = lib().srt_last_row_chunks()
    assert_envelope(lo, hi, st, env, f"{g.name} algo={algo}")
    if row_bytes:
        rows, chunk = len(lo), (1 << 19) // (row_bytes * g.n)
        print(f"{g.name} algo={algo}: {rows} rows, {chunk} a chunk, {chunks} chunks")
        assert chunks > 1 and chunks == -(-rows // chunk) and rows % chunk != 0, (chunks, chunk)
    return lo, hi, st, env


# ---- case 1 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [ALGO_SPARSE_SSSP, ALGO_DENSE_FW])
def test_c1_all_rows(gpu, algo):
    """C1 has self-loops: the tables' diagonal holds the path-to-self rule, so D[s][s] must be
    taken as 0 or no direct neighbour of s has a tight arc from it."""
    lo, hi, st, _ = run(route_graphs.c1(), algo)
    assert st.stage_forms == 1
    assert (np.diagonal(lo) == 1.0).all() and (np.diagonal(hi) == 1.0).all()


# ---- case 2 ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _core_tail(directed):
    g = level_graphs.core_tail(18, directed=directed)
    assert 220 <= g.n <= 240, g.n
    env = expect(g)
    assert env.exposed_pairs > env.tied_pairs, "untied targets downstream of tied ones"
    assert env.max_sweeps >= 12, "a deep chain"
    return g


@pytest.mark.parametrize("directed", [False, True])
def test_core_tail(gpu, directed):
    """Tied at every rung of the braided tail; the directed form's essential in-lists come in free
    order."""
    g = _core_tail(directed)
    run(g, ALGO_DENSE_FW)


# ---- case 3 ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fans(k):
    """One fan per placement of the extreme arms: s - {k arms} - t, every edge 1 ms, so |M(s, t)| =
    k and t's in-list holds the arms in vertex order. Arm i has losses a_i (from s) and b_i (into
    t), all distinct; the arm `zero` ends in an arc of loss 1.0 (lo = 0.0), the arm `best` in one
    of loss 0 (hi = 1 - a_best, above every other arm's product). The placements put the two at
    the first arc, the last arc and arc 64 of the list (where the list has one)."""
    spots = [0, k - 1] + ([64] if k > 64 else [])
    places = [(z, b) for z in spots for b in spots if z != b]
    src, dst, loss, fans = [], [], [], []
    v = 0
    for zero, best in places:
        s, arms, t = v, np.arange(v + 1, v + 1 + k), v + 1 + k
        v = t + 1
        a = 0.01 + 0.001 * np.arange(k)
        b = 0.3 + 0.002 * np.arange(k)
        b[zero], b[best] = 1.0, 0.0
        assert len(np.unique(np.concatenate([a, b]))) == 2 * k
        src += [np.full(k, s), arms]
        dst += [arms, np.full(k, t)]
        loss += [a, b]
        fans.append((s, t, 1.0 * (1.0 - a[best])))
    src, dst, loss = np.concatenate(src), np.concatenate(dst), np.concatenate(loss)
    g = graphs.Graph(v, False, src.astype(np.int32), dst.astype(np.int32),
                     np.full(len(src), MS, np.int64), loss, f"fans{k}")
    srcs = np.array([f[0] for f in fans])
    env = expect(g, srcs)
    arcs = rr.InArcs(g)
    head = np.repeat(np.arange(g.n), np.diff(arcs.ptr))
    for i, (s, t, top) in enumerate(fans):
        assert env.lo[i][t] == 0.0 and env.hi[i][t] == top and env.tied[i][t], (k, i)
        m = er.members(arcs, head, _fan_row(g.n, s, k), s)
        assert m[arcs.ptr[t]:arcs.ptr[t + 1]].sum() == k, "|M(s, t)| = k"
    return g, srcs


def _fan_row(n, s, k):
    """The distance row of a fan's source in ns: the arms at 1 ms, t at 2 ms, the rest unreachable."""
    d = np.full(n, rr.NO_DIST, np.int64)
    d[s] = 0
    d[s + 1:s + 1 + k] = MS
    d[s + 1 + k] = 2 * MS
    return d


@pytest.mark.parametrize("algo", [ALGO_SPARSE_SSSP, ALGO_DENSE_FW])
@pytest.mark.parametrize("k", [31, 32, 33, 64, 65, 130])
def test_fan(gpu, k, algo):
    """|M| = k on both sides of the switch to the wave-wide walk (32 arcs) and of a 64-arc step."""
    g, srcs = _fans(k)
    run(g, algo, sources=srcs)


# ---- cases 4, 5, 6 -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hand():
    """Three components. 0-3: the square 2+3 / 3+2, both in-arcs of 3 tight from 0 at different
    distances. 4-7: a diamond whose arms give bit-equal products. 8-11: a diamond whose arms do
    not (the graph's sensitive pairs)."""
    e = [(0, 1, 2, 0.1), (1, 3, 3, 0.1), (0, 2, 3, 0.0), (2, 3, 2, 0.0),
         (4, 5, 1, 0.25), (4, 6, 1, 0.5), (5, 7, 1, 0.5), (6, 7, 1, 0.25),
         (8, 9, 1, 0.01), (8, 10, 1, 0.02), (9, 11, 1, 0.03), (10, 11, 1, 0.05)]
    a = np.array(e, np.float64)
    g = graphs.Graph(12, False, a[:, 0].astype(np.int32), a[:, 1].astype(np.int32),
                     (a[:, 2] * MS).astype(np.int64), a[:, 3].copy(), "hand12")
    env = expect(g)
    # case 4: the product over 2 (1.0) lies outside [lo, hi] = 0.81
    assert env.lo[0][3] == env.hi[0][3] == (1.0 - 0.1) * (1.0 - 0.1) != 1.0 and not env.tied[0][3]
    # case 5
    assert env.tied[4][7] and env.exposed[4][7] and not env.sensitive[4][7]
    assert env.lo[4][7] == env.hi[4][7] == 0.375
    # case 6
    assert env.sensitive[8][11] and env.lo[0][4] == env.hi[0][4] == 0.0
    return g


@pytest.mark.parametrize("algo", [ALGO_SPARSE_SSSP, ALGO_DENSE_FW])
def test_hand_graph(gpu, algo):
    """Cases 4, 5 and 6: M is not "all tight arcs"; a tied pair need not be sensitive; unreachable
    pairs give 0.0 / 0.0 and enter no count."""
    g = _hand()
    lo, hi, st, env = run(g, algo)
    unreach = np.arange(g.n)[:, None] // 4 != np.arange(g.n)[None, :] // 4
    assert not lo[unreach].any() and not hi[unreach].any()
    assert not (env.tied | env.exposed | env.sensitive)[unreach].any()


# ---- case 7 ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ring():
    n = 3000
    idx = np.arange(n)
    g = graphs.Graph(n, False, idx.astype(np.int32), ((idx + 1) % n).astype(np.int32),
                     np.full(n, MS, np.int64), (idx % 7) / 1000.0, "ring3000_losses")
    srcs = np.array([0, 1, 1499, 2999])
    env = expect(g, srcs)
    assert env.max_sweeps == 1500 and env.tied[0][1500] and env.sensitive[0][1500]
    return g, srcs


def test_ring_sweeps(gpu):
    """1,500 sweeps; the antipodal target is tied."""
    g, srcs = _ring()
    _, _, st, _ = run(g, sources=srcs)
    assert st.max_sweeps == 1500


# ---- case 8 ------------------------------------------------------------------------------------
def test_staging_form_3(gpu):
    """A row that does not fit the LDS beside the bitmaps: read from global memory."""
    n = lib().srt_envelope_stage_max_n(1) + 2000
    assert n <= lib().srt_envelope_stage_max_n(3)
    g = graphs.barabasi_albert(n, m=3, seed=5)
    _, _, st, _ = run(g, ALGO_SPARSE_SSSP, sources=np.arange(4))
    assert st.stage_forms == 4, st.stage_forms


# ---- case 9 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["sparse", "dense", "source_list"])
def test_several_row_chunks(gpu, case):
    """Room for a few rows at a time: 16 B a pair for lo and hi, beside a sparse build's distance
    and reliability rows (12 B)."""
    if case == "sparse":
        run(route_graphs.directed_random(True), ALGO_SPARSE_SSSP, row_bytes=28)
    elif case == "dense":
        run(graphs.complete_graph(300, seed=11, lat_max=3), ALGO_DENSE_FW, row_bytes=16)
    else:
        g = graphs.random_geometric(2000, seed=3)
        srcs = np.unique(np.random.default_rng(5).integers(0, g.n, 60))[:37]
        run(g, ALGO_SPARSE_SSSP, sources=srcs, row_bytes=28)


# ---- case 10 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lo", "hi"])
def test_dense_device_row_range(gpu, which):
    """srt_envelope_dense_device on rows [128, 300) of the n = 300 graph, device resident, one
    output NULL: the asked rows exact, every other row and the columns >= n untouched."""
    import torch
    n, ld, row0 = 300, 384, 128
    env = expect(graphs.complete_graph(n, seed=11, lat_max=3))
    L = lib()
    w = torch.empty((ld, ld), dtype=torch.int32, device="cuda")
    r = torch.empty((ld, ld), dtype=torch.float64, device="cuda")
    assert L.srt_gen_complete_device(n, ld, 0, ld, 11, 3, 10, 500, w.data_ptr(), r.data_ptr(),
                                     None) == 0
    lat = torch.empty_like(w)
    rel = torch.empty_like(r)
    assert L.srt_dense_build_device(n, ld, 0, w.data_ptr(), r.data_ptr(), lat.data_ptr(),
                                    rel.data_ptr(), None, 0, None) == 0
    SENT = -77.0
    out = torch.full((ld, ld), SENT, dtype=torch.float64, device="cuda")
    st = EnvelopeStats()
    ptrs = (out[row0:].data_ptr(), None) if which == "lo" else (None, out[row0:].data_ptr())
    check(L.srt_envelope_dense_device(n, ld, 0, w.data_ptr(), r.data_ptr(), lat.data_ptr(), row0,
                                      n - row0, *ptrs, ld, None, ctypes.byref(st)),
          "srt_envelope_dense_device")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = (env.lo if which == "lo" else env.hi)[row0:n]
    assert np.array_equal(got[row0:n, :n].view(np.uint64), want.view(np.uint64))
    assert (got[:row0] == SENT).all() and (got[n:] == SENT).all() and (got[row0:n, n:] == SENT).all()
    assert (st.tied_pairs, st.exposed_pairs, st.sensitive_pairs) == (
        int(env.tied[row0:].sum()), int(env.exposed[row0:].sum()), int(env.sensitive[row0:].sum()))
    assert st.max_sweeps == int(env.depth[row0:].max()) and st.stage_forms == 1


def test_sparse_device_rows(gpu):
    """srt_envelope_rows_device (SparseGraph.envelope_rows) over rows srt_sparse_graph_rows_list
    made: a source list, outputs of stride > n, then each output alone."""
    import torch
    from shadow_amd.topology import SparseGraph
    g = route_graphs.directed_random(True)
    env = expect(g)
    n, ldo = g.n, g.n + 20
    sg = SparseGraph(n, True, g.src, g.dst, g.lat_ns, g.loss)
    srcs = np.array([3, 17, 18, 250, 299], np.int32)
    dsrc = torch.tensor(srcs, device="cuda")
    lat = torch.empty((len(srcs), n), dtype=torch.int32, device="cuda")
    rel = torch.empty((len(srcs), n), dtype=torch.float64, device="cuda")
    sg.rows_list(dsrc.data_ptr(), len(srcs), lat.data_ptr(), rel.data_ptr())
    for which in ("both", "lo", "hi"):
        lo, hi = (torch.full((len(srcs), ldo), -9.0, dtype=torch.float64, device="cuda")
                  for _ in range(2))
        st = EnvelopeStats()
        sg.envelope_rows(lat.data_ptr(), len(srcs), lo.data_ptr() if which != "hi" else None,
                         hi.data_ptr() if which != "lo" else None, srcs_ptr=dsrc.data_ptr(),
                         ldo=ldo, stats=st)
        torch.cuda.synchronize()
        lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
        if which != "hi":
            assert np.array_equal(lo[:, :n].view(np.uint64), env.lo[srcs].view(np.uint64)), which
        else:
            assert (lo == -9.0).all()
        if which != "lo":
            assert np.array_equal(hi[:, :n].view(np.uint64), env.hi[srcs].view(np.uint64)), which
        else:
            assert (hi == -9.0).all()
        assert (lo[:, n:] == -9.0).all() and (hi[:, n:] == -9.0).all()
        assert (st.tied_pairs, st.exposed_pairs, st.sensitive_pairs, st.max_sweeps) == (
            int(env.tied[srcs].sum()), int(env.exposed[srcs].sum()),
            int(env.sensitive[srcs].sum()), int(env.depth[srcs].max())), which
        assert st.stage_forms == 1
    sg.free()


# ---- case 11 -----------------------------------------------------------------------------------
def test_direct_mode(gpu):
    """use_shortest_path = 0: every pair is its own arc, lo = hi = r(s, t)."""
    g = route_graphs.c1()
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    want = oracle.table(el, False, oracle.ORC_INT_NS, 1, raw=True)["rel"].copy()
    np.fill_diagonal(want, 1.0)
    srcs = np.array([0, 7, 49])
    for ss in (None, srcs):
        lo, hi, st = build_rel_envelope(g.n, False, g.src, g.dst, g.lat_ns, g.loss, sources=ss,
                                        use_shortest_path=False)
        w = want if ss is None else want[ss]
        assert np.array_equal(lo.view(np.uint64), w.view(np.uint64))
        assert np.array_equal(hi.view(np.uint64), w.view(np.uint64))
        assert st.tied_pairs == st.exposed_pairs == st.sensitive_pairs == 0
    ring, _ = _ring()  # not complete: the table build's error
    with pytest.raises(RuntimeError, match="SRT_E_INVALID"):
        build_rel_envelope(ring.n, False, ring.src, ring.dst, ring.lat_ns, ring.loss,
                           use_shortest_path=False)


# ---- case 12 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [ALGO_AUTO, ALGO_SPARSE_SSSP])
def test_submillisecond_quanta(gpu, algo):
    """0.3-0.7 ms edges: the quantum is 100 us, the pass runs on the integer quanta."""
    run(route_graphs.submillisecond(), algo)


# ---- case 13 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "core_tail", "directed_rgg"])
def test_contains_the_tables(gpu, name):
    """The product's own reliability (the canonical tie order is one feasible order) lies within
    the bounds of every off-diagonal pair, equals both bitwise where they coincide, and the pass
    counts the tied pairs a count_ties build counts."""
    g = {"c1": route_graphs.c1, "core_tail": lambda: _core_tail(False),
         "directed_rgg": lambda: graphs.directed_rgg(300, seed=3, lat_max=3)}[name]()
    lo, hi, st, _ = run(g)
    _, rel, _ = build_tables(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    off = ~np.eye(g.n, dtype=bool)
    assert (lo[off] <= rel[off]).all() and (rel[off] <= hi[off]).all()
    same = off & (lo.view(np.uint64) == hi.view(np.uint64))
    assert same.any() and np.array_equal(rel[same].view(np.uint64), lo[same].view(np.uint64))
    _, _, bs = level_graphs.build(g, ALGO_AUTO, count_ties=1)
    assert st.tied_pairs == bs.tied_pairs, (st.tied_pairs, bs.tied_pairs)
