"""lvl_pred_near_kernel (levels.hip): the predecessor pass's Delta_1 arc groups resolved from the
in-arc runs into per-(target, chunk) buckets, which lvl_pred_kernel's units take instead of
gathering the group's plane slices. SRT_FORM bcap=<k> forces the pre-pass at any size with buckets
of k entries (2,048, a chunk's sources, cannot overflow; a bucket past a smaller k falls back to
the walk) and bcap=-1 turns it off; srt_build_stats.pred_near is the capacity used and
pred_near_over the overflowed buckets.

Small graphs against the CPU oracle's Dijkstra (latency bit-exact, reliability within 1e-12
relative, as tests/test_gpu_levels.py); a graph of three source chunks, the last one partial,
against sampled oracle rows and bit for bit against the build without the pre-pass."""
import ctypes

import numpy as np
import pytest
from conftest import set_form

import oracle
from shadow_amd import _lib, graphs
from shadow_amd._lib import ALGO_DENSE_FW
from shadow_amd.topology import build_tables

pytestmark = pytest.mark.gpu
REL_TOL = 1e-12
MS = 1_000_000
LEVELS = 12


def _check(g, lat, rel, what):
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    exp = oracle.table(el, True, oracle.ORC_INT_NS, 8, raw=True)
    bad = np.argwhere(lat != np.asarray(exp["lat_int"], np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} latency mismatches, first {bad[:5].tolist()}"
    err = np.abs(rel - exp["rel"]) / np.maximum(np.abs(exp["rel"]), 1e-300)
    assert float(err.max()) <= REL_TOL, f"{what}: max rel error {err.max()}"


def _directed_dense(n, seed, wmax):
    """The directed graph of test_gpu_levels.py::test_levels_match_oracle."""
    rng = np.random.default_rng(seed)
    i, j = np.nonzero(rng.random((n, n)) < 0.35)
    keep = i != j
    i, j = i[keep], j[keep]
    ring = np.arange(n)  # strongly connected
    src = np.concatenate([i, ring]).astype(np.int32)
    dst = np.concatenate([j, (ring + 1) % n]).astype(np.int32)
    lat = (rng.integers(1, wmax + 1, len(src)) * MS).astype(np.int64)
    loss = rng.integers(0, 300, len(src)) / 10000.0
    return graphs.Graph(n, True, src, dst, lat, loss, f"directed{n}")


def _manyrel():
    g0 = graphs.complete_graph(300, seed=9)
    loss = np.random.default_rng(9).random(g0.m) * 0.05
    return graphs.Graph(g0.n, False, g0.src, g0.dst, g0.lat_ns, loss, "manyrel")


def _forced(monkeypatch, g, what, ngpus=None, **form):
    set_form(monkeypatch, levels="1", bcap="2048", **form)
    lat, rel, st = build_tables(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                algo=ALGO_DENSE_FW, ngpus=ngpus)
    assert st.dist_enc == LEVELS, st.dist_enc
    assert st.pred_near > 0, st.pred_near
    _check(g, lat, rel, what)
    return st


@pytest.mark.parametrize("kind", ["complete300", "ties", "directed"])
def test_pred_near_forced_small(gpu, monkeypatch, kind):
    """One partial chunk (nw < 64); 1-3 ms arcs (a dense Delta_1 and many equal-length paths: the
    arc order and the test-and-clear decide the predecessor); in-arcs of a directed graph."""
    if kind == "complete300":
        g = graphs.complete_graph(300, seed=7)
    elif kind == "ties":
        g = graphs.complete_graph(640, seed=11, lat_max=3)
    else:
        g = _directed_dense(500, 5, 40)
    _forced(monkeypatch, g, kind)


@pytest.mark.parametrize("ranks", [2, 3])
def test_pred_near_virtual_ranks(gpu, monkeypatch, ranks):
    """Row shards: src0 != 0, and a run's sources of other ranks must be filtered out."""
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    _forced(monkeypatch, graphs.complete_graph(1000, seed=2), f"virtual x{ranks}", ngpus=1)


@pytest.mark.parametrize("kind", ["int16", "int32"])
def test_pred_near_output_forms(gpu, monkeypatch, kind):
    """The int16 rows (SRT_FORM pkw=0) and the f64-reliability rows (more distinct losses than the
    table holds) of lvl_pred_kernel take the buckets' claims as the packed words do."""
    if kind == "int16":
        _forced(monkeypatch, graphs.complete_graph(300, seed=7), kind, pkw="0")
    else:
        _forced(monkeypatch, _manyrel(), kind)


# ---- three source chunks, the last one partial: n = 4,096 + 96 ----------------------------------
N3, SEED3, LATMAX3 = 4096 + 96, 17, 120
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()  # the device tensors of the shared builds


def _graph3():
    import torch
    if "w" not in _cache:
        L = _lib.lib()
        ld = (N3 + 255) // 256 * 256
        w = torch.empty((ld, ld), dtype=torch.int32, device="cuda")
        r = torch.empty((ld, ld), dtype=torch.float64, device="cuda")
        _lib.check(L.srt_gen_complete_device(N3, ld, 0, ld, SEED3, LATMAX3, 10, 500, w.data_ptr(),
                                             r.data_ptr(), None), "generate")
        _cache["w"], _cache["r"] = w, r
    return _cache["w"], _cache["r"]


def _build3(monkeypatch, **form):
    """The tables of the three-chunk graph under SRT_FORM `form` (device tensors, cached)."""
    import torch
    key = tuple(sorted(form.items()))
    if key not in _cache:
        w, r = _graph3()
        set_form(monkeypatch, levels="1", **form)
        lat = torch.empty_like(w)
        rel = torch.empty_like(r)
        st = _lib.BuildStats()
        _lib.check(_lib.lib().srt_dense_build_device(N3, w.shape[0], 0, w.data_ptr(), r.data_ptr(),
                                                     lat.data_ptr(), rel.data_ptr(), None, 0,
                                                     ctypes.byref(st)), "build")
        torch.cuda.synchronize()
        assert st.dist_enc == LEVELS, st.dist_enc
        _cache[key] = (lat, rel, st)
    return _cache[key]


def test_pred_near_chunks_match_oracle(gpu, monkeypatch):
    """The first and last row and a row either side of each 2,048 boundary against the oracle."""
    import torch
    lat, rel, st = _build3(monkeypatch, bcap="2048")
    assert st.pred_near == 2048 and st.pred_near_over == 0, (st.pred_near, st.pred_near_over)
    rows = np.array([0, 2047, 2048, 4095, 4096, N3 - 1], np.int32)
    idx = torch.from_numpy(rows.astype(np.int64)).cuda()
    glat = lat.index_select(0, idx)[:, :N3].cpu().numpy().view(np.uint32).astype(np.uint64) \
        * np.uint64(MS)
    grel = rel.index_select(0, idx)[:, :N3].cpu().numpy()
    clat, crel, _, _ = oracle.complete_sample(N3, SEED3, LATMAX3, 10, 500, rows, 8)
    off = np.arange(N3)[None, :] != rows[:, None]
    bad = np.argwhere(np.where(off, glat, 0) != np.where(off, clat, 0))
    assert bad.size == 0, f"{len(bad)} latency mismatches, first {bad[:5].tolist()}"
    err = np.abs(grel - crel) / np.maximum(crel, 1e-300)
    assert float(err[off].max()) <= REL_TOL


def test_pred_near_bit_equal_to_walk(gpu, monkeypatch):
    import torch
    lat0, rel0, st0 = _build3(monkeypatch, bcap="-1")
    lat2, rel2, st2 = _build3(monkeypatch, bcap="2048")
    assert st0.pred_near == 0 and st2.pred_near == 2048
    assert torch.equal(lat0, lat2)
    assert torch.equal(rel0, rel2)


@pytest.mark.parametrize("pncap", [8, 256])
def test_pred_near_overflow_falls_back(gpu, monkeypatch, pncap):
    """bcap=8: every bucket overflows (with ~35 one-ms in-arcs per vertex the pre-pass settles
    about half of all pairs: hundreds of a full chunk's 2,048 sources, ~48 +- 7 of the last
    chunk's 96), and every unit walks the groups itself. bcap=256: the last chunk's buckets cannot
    overflow (96 sources < 256), the full chunks' do (each level's candidates cover ~29% of 2,048 sources), so
    overflowed and kept buckets are mixed. Both bit-equal to the build without the pre-pass."""
    import torch
    lat0, rel0, _ = _build3(monkeypatch, bcap="-1")
    lat, rel, st = _build3(monkeypatch, bcap=str(pncap))
    units = N3 * 3
    assert st.pred_near == pncap
    if pncap == 8:
        assert st.pred_near_over == units, (st.pred_near_over, units)
    else:
        assert 0 < st.pred_near_over < units, (st.pred_near_over, units)
    assert torch.equal(lat0, lat)
    assert torch.equal(rel0, rel)


def test_pred_near_tie_count_unchanged(gpu, monkeypatch):
    """count_ties = 1: the pre-pass is not launched (a tied pair is seen only by the full walk);
    tied_pairs of the 1-3 ms graph is the same with the pre-pass off and forced."""
    g = graphs.complete_graph(640, seed=11, lat_max=3)
    src = np.ascontiguousarray(g.src, np.int32)
    dst = np.ascontiguousarray(g.dst, np.int32)
    lat_ns = np.ascontiguousarray(g.lat_ns, np.int64)
    loss = np.ascontiguousarray(g.loss, np.float64)
    e = _lib.Edges(g.n, int(bool(g.directed)), len(src), src.ctypes.data, dst.ctypes.data,
                   lat_ns.ctypes.data, loss.ctypes.data)
    o = _lib.BuildOpts(0, ALGO_DENSE_FW, 1, 0)
    tied = {}
    for mode in ("-1", "2048"):
        set_form(monkeypatch, levels="1", bcap=mode)
        lat = np.empty((g.n, g.n), np.uint32)
        rel = np.empty((g.n, g.n), np.float64)
        q = ctypes.c_uint64()
        st = _lib.BuildStats()
        st.count_ties = 1
        _lib.check(_lib.lib().srt_build_tables(ctypes.byref(e), ctypes.byref(o), lat.ctypes.data,
                                               ctypes.byref(q), rel.ctypes.data, ctypes.byref(st)),
                   "srt_build_tables")
        assert st.dist_enc == LEVELS and st.pred_near == 0, (st.dist_enc, st.pred_near)
        tied[mode] = int(st.tied_pairs)
    assert tied["-1"] > 0 and tied["-1"] == tied["2048"], tied


def test_pred_near_default_rule(gpu):
    """n = 16,384 with latencies U{1..500} ms (~33 one-ms in-arcs per vertex, C4's density): the
    default schedule takes the pre-pass (no SRT_FORM); sampled rows against the oracle."""
    import torch
    L = _lib.lib()
    n, seed, lat_max = 16384, 43, 500
    ld = n
    w = torch.empty((ld, ld), dtype=torch.int32, device="cuda")
    r = torch.empty((ld, ld), dtype=torch.float64, device="cuda")
    _lib.check(L.srt_gen_complete_device(n, ld, 0, ld, seed, lat_max, 10, 500, w.data_ptr(),
                                         r.data_ptr(), None), "generate")
    lat = torch.empty_like(w)
    rel = torch.empty_like(r)
    st = _lib.BuildStats()
    _lib.check(L.srt_dense_build_device(n, ld, 0, w.data_ptr(), r.data_ptr(), lat.data_ptr(),
                                        rel.data_ptr(), None, 0, ctypes.byref(st)), "build")
    torch.cuda.synchronize()
    del w, r
    assert st.dist_enc == LEVELS, st.dist_enc
    assert st.pred_near > 0, st.pred_near
    rows = np.array([0, 2047, 2048, 8191, n // 2 + 7, n - 1], np.int32)
    idx = torch.from_numpy(rows.astype(np.int64)).cuda()
    glat = lat.index_select(0, idx).cpu().numpy().view(np.uint32).astype(np.uint64) * np.uint64(MS)
    grel = rel.index_select(0, idx).cpu().numpy()
    del lat, rel
    clat, crel, _, _ = oracle.complete_sample(n, seed, lat_max, 10, 500, rows, 16)
    off = np.arange(n)[None, :] != rows[:, None]
    bad = np.argwhere(np.where(off, glat, 0) != np.where(off, clat, 0))
    assert bad.size == 0, f"{len(bad)} latency mismatches, first {bad[:5].tolist()}"
    err = np.abs(grel - crel) / np.maximum(crel, 1e-300)
    assert float(err[off].max()) <= REL_TOL
