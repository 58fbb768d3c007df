"""lvl_pred_rows_kernel (levels.hip): the level build's packed predecessor words written
source-major by narrow units -- a wave covers 4 targets x 16 words (512 sources), a workgroup 32
targets of one 512-source sub-chunk -- straight into the rows rel_pk_kernel streams, with no
target-major slab and no transpose. SRT_FORM pkw=1 (the default) takes it, pkw=2 keeps
lvl_pred_kernel's target-major words and the transpose, pkw=0 the int16 rows.

Every build is forced through the levels (SRT_FORM levels=1) and checked against the CPU oracle's
Dijkstra (latency bit-exact, reliability within 1e-12 relative) and, where both are built, bit for
bit against the pkw=2 build. The shapes are the ones at which the mapping can go wrong: target
counts that are no multiple of 4, 32 or 128, a partial last sub-chunk, ties, directed in-arcs,
adjacent targets with very different in-arc counts, the pre-pass's buckets (never, always and
sometimes overflowing), row shards, 31 levels and unreachable pairs."""
import ctypes

import numpy as np
import pytest
from conftest import set_form

import level_graphs as lg
import oracle
from shadow_amd import _lib, graphs
from shadow_amd._lib import ALGO_DENSE_FW
from shadow_amd.topology import build_tables

pytestmark = pytest.mark.gpu
REL_TOL = 1e-12
MS = 1_000_000
LEVELS = 12


def _check(g, lat, rel, what):
    exp = lg.oracle_table(g)
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


def _core_and_leaves():
    """A complete core of 200 vertices (1-3 ms arcs: ~66 in-arcs of each weight per vertex), 60
    leaves on one 1-ms edge, 60 on one 2-ms edge and 40 on one 3-ms edge, the vertex ids shuffled:
    the four targets of a wave have 0, 1 and > 64 in-arcs of one weight side by side."""
    core = graphs.complete_graph(200, seed=5, lat_max=3)
    rng = np.random.default_rng(5)
    leaves = np.arange(200, 360)
    hub = rng.integers(0, 200, len(leaves))
    wl = np.concatenate([np.full(60, 1), np.full(60, 2), np.full(40, 3)])
    src = np.concatenate([core.src, hub])
    dst = np.concatenate([core.dst, leaves])
    lat = np.concatenate([core.lat_ns, wl * MS]).astype(np.int64)
    loss = np.concatenate([core.loss, rng.integers(0, 300, len(leaves)) / 10000.0])
    perm = rng.permutation(360)
    return graphs.Graph(360, False, perm[src].astype(np.int32), perm[dst].astype(np.int32), lat,
                        loss, "core_and_leaves")


_graphs = {}


def _graph(kind):
    if kind not in _graphs:
        if kind.startswith("complete"):
            _graphs[kind] = graphs.complete_graph(int(kind[8:]), seed=7)
        elif kind == "shards":
            _graphs[kind] = graphs.complete_graph(1000, seed=2)
        elif kind == "ties":
            _graphs[kind] = graphs.complete_graph(640, seed=11, lat_max=3)
        elif kind == "directed":
            _graphs[kind] = _directed_dense(500, 5, 40)
        elif kind == "divergent":
            _graphs[kind] = _core_and_leaves()
        elif kind == "deep31":
            _graphs[kind] = lg.core_tail(31)
        elif kind == "manyrel":
            _graphs[kind] = _manyrel()
        else:
            raise KeyError(kind)
    return _graphs[kind]


def _require_kernel():
    """A library without lvl_pred_rows_kernel reads pkw=1 as its target-major form and would pass
    every comparison below unchanged: the tests refuse it (the kernel's name is in the library's
    registration strings)."""
    if "have" not in _graphs:
        with open(_lib.LIB_PATH, "rb") as f:
            _graphs["have"] = b"lvl_pred_rows_kernel" in f.read()
    assert _graphs["have"], "this library has no lvl_pred_rows_kernel: pkw=1 cannot take the narrow units"


def _build(monkeypatch, g, ngpus=None, **form):
    _require_kernel()
    set_form(monkeypatch, levels="1", **form)
    lat, rel, st = build_tables(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                algo=ALGO_DENSE_FW, ngpus=ngpus)
    assert st.dist_enc == LEVELS, st.dist_enc
    return lat, rel, st


def _rows_and_reference(monkeypatch, g, what, ngpus=None, **form):
    """The build through the narrow units against the oracle and bit for bit against pkw=2."""
    lat, rel, st = _build(monkeypatch, g, ngpus=ngpus, pkw="1", **form)
    _check(g, lat, rel, what)
    lat2, rel2, _ = _build(monkeypatch, g, ngpus=ngpus, pkw="2", **form)
    assert np.array_equal(lat, lat2), what
    assert np.array_equal(rel.view(np.uint64), rel2.view(np.uint64)), \
        (what, np.argwhere(rel.view(np.uint64) != rel2.view(np.uint64))[:5])
    return st


@pytest.mark.parametrize("kind", ["complete130", "complete300", "complete1000", "ties", "directed",
                                  "divergent", "deep31"])
def test_pred_rows_match_oracle(gpu, monkeypatch, kind):
    """Target-group borders (n = 130, 300, 1000: the last workgroup has empty waves and groups);
    1-3 ms arcs (a dense Delta_1, many equal-length paths); directed in-arcs (groups of very
    different arc counts in one wave); leaves beside core vertices (0, 1 and > 64 arcs of one
    weight in one wave); largest distance 31 (all five level bit planes)."""
    g = _graph(kind)
    st = _rows_and_reference(monkeypatch, g, kind)
    if kind == "deep31":
        assert st.levels == 31, st.levels


@pytest.mark.parametrize("bcap", ["2048", "1", "-1"])
@pytest.mark.parametrize("kind", ["complete300", "ties", "directed"])
def test_pred_rows_buckets(gpu, monkeypatch, kind, bcap):
    """The pre-pass's buckets, keyed by 2,048-source chunks, read by 512-source units: buckets
    that cannot overflow, buckets that all do (the group walks w = d - 1 itself), none."""
    g = _graph(kind)
    lat, rel, st = _build(monkeypatch, g, pkw="1", bcap=bcap)
    _check(g, lat, rel, f"{kind} bcap={bcap}")
    if bcap == "2048":
        assert st.pred_near == 2048 and st.pred_near_over == 0, (st.pred_near, st.pred_near_over)
    elif bcap == "1":
        assert st.pred_near == 1 and st.pred_near_over > 0, (st.pred_near, st.pred_near_over)
    else:
        assert st.pred_near == 0, st.pred_near


@pytest.mark.parametrize("kind,ranks", [("shards", 2), ("shards", 3), ("directed", 2)])
def test_pred_rows_virtual_ranks(gpu, monkeypatch, kind, ranks):
    """Row shards: src0 != 0, nsrc a multiple of 128, the last shard's rows past n."""
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    _rows_and_reference(monkeypatch, _graph(kind), f"{kind} x{ranks}", ngpus=1, bcap="2048")


def test_pred_rows_unreachable(gpu, monkeypatch):
    """Two disjoint complete graphs forced through the levels. The level build of a graph with
    unreachable pairs never completes and hands the build to Floyd-Warshall (dist_enc != 12, as
    tests/test_gpu_level_unreached.py asserts), so no packed words are written for it; the tables
    must still be the oracle's and equal under pkw=1 and pkw=2."""
    _require_kernel()
    g = lg.two_complete()
    out = {}
    for pkw in ("1", "2"):
        set_form(monkeypatch, levels="1", pkw=pkw)
        lat, rel, st = lg.build(g)
        assert st.dist_enc != LEVELS and st.levels == 0, (st.dist_enc, st.levels)
        lg.check_tables(g, lat, rel, f"two_complete pkw={pkw}", reachable_only=True)
        out[pkw] = (lat, rel)
    assert np.array_equal(out["1"][0], out["2"][0])
    assert np.array_equal(out["1"][1].view(np.uint64), out["2"][1].view(np.uint64))


@pytest.mark.parametrize("kind", ["int16", "manyrel"])
def test_pred_rows_other_forms(gpu, monkeypatch, kind):
    """pkw=0 (int16 rows) and more distinct reliabilities than the table holds (f64 rows) keep
    lvl_pred_kernel and still match the oracle."""
    if kind == "int16":
        g = _graph("complete300")
        lat, rel, _ = _build(monkeypatch, g, pkw="0")
    else:
        g = _graph("manyrel")
        lat, rel, st = _build(monkeypatch, g)
        assert st.rel_table == 0, st.rel_table
    _check(g, lat, rel, kind)


def test_pred_rows_tie_count(gpu, monkeypatch):
    """count_ties = 1 keeps lvl_pred_kernel and the transpose: the same tables bit for bit as the
    plain pkw=1 build, and the same tied_pairs as under pkw=2."""
    _require_kernel()
    g = _graph("ties")
    set_form(monkeypatch, levels="1", pkw="1")
    lat, rel, st = lg.build(g)
    latt, relt, stt = lg.build(g, count_ties=1)
    assert st.dist_enc == LEVELS and stt.dist_enc == LEVELS
    assert np.array_equal(lat, latt)
    assert np.array_equal(rel.view(np.uint64), relt.view(np.uint64))
    set_form(monkeypatch, levels="1", pkw="2")
    _, _, st2 = lg.build(g, count_ties=1)
    assert int(stt.tied_pairs) > 0 and int(stt.tied_pairs) == int(st2.tied_pairs)


# ---- three 2,048-source chunks, the last 512-source sub-chunk partial: n = 4,096 + 96 -----------
N3, SEED3, LATMAX3 = 4096 + 96, 17, 120
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()  # the device tensors of the shared builds
    _graphs.clear()


def _build3(monkeypatch, **form):
    """The tables of the three-chunk device-generated graph under SRT_FORM `form` (cached)."""
    import torch
    _require_kernel()
    if "w" not in _cache:
        ld = (N3 + 255) // 256 * 256
        w = torch.empty((ld, ld), dtype=torch.int32, device="cuda")
        r = torch.empty((ld, ld), dtype=torch.float64, device="cuda")
        _lib.check(_lib.lib().srt_gen_complete_device(N3, ld, 0, ld, SEED3, LATMAX3, 10, 500,
                                                      w.data_ptr(), r.data_ptr(), None), "generate")
        _cache["w"], _cache["r"] = w, r
    key = tuple(sorted(form.items()))
    if key not in _cache:
        w, r = _cache["w"], _cache["r"]
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


def test_pred_rows_chunks_match_oracle(gpu, monkeypatch):
    """The first and last row, a row either side of each 2,048 boundary and of the last
    512 boundary against the oracle."""
    import torch
    lat, rel, _ = _build3(monkeypatch, pkw="1")
    rows = np.array([0, 511, 512, 2047, 2048, 4095, 4096, N3 - 1], np.int32)
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


@pytest.mark.parametrize("bcap", ["0", "2048", "256", "-1"])
def test_pred_rows_chunks_bit_equal(gpu, monkeypatch, bcap):
    """Bit for bit the pkw=2 build, with the default pre-pass rule, buckets that cannot overflow,
    mixed overflowed and kept buckets (256) and no pre-pass."""
    import torch
    lat1, rel1, st1 = _build3(monkeypatch, pkw="1", bcap=bcap)
    lat2, rel2, st2 = _build3(monkeypatch, pkw="2", bcap=bcap)
    assert (st1.pred_near, st1.pred_near_over) == (st2.pred_near, st2.pred_near_over)
    if bcap == "256":
        assert 0 < st1.pred_near_over < N3 * 3, st1.pred_near_over
    assert torch.equal(lat1, lat2)
    assert torch.equal(rel1, rel2)
