"""lvl_pred_rows_kernel's four-wave unit (levels.hip): a workgroup is 256 threads, 16 consecutive
targets of one 512-source sub-chunk, the output stage stores one 64-B run of every source's row,
and a lane keeps 22 LDS words -- the target's group bounds in the words that are idle during the
walk, the five level planes over them afterwards.

Every build is forced through the levels (SRT_FORM levels=1, dist_enc 12) and checked against the
CPU oracle's Dijkstra (latency bit-exact, reliability within 1e-12 relative) and bit for bit
against the pkw=2 build (lvl_pred_kernel's target-major words and the transpose). The shapes are
the smallest at which the 16-target mapping can go wrong and that test_gpu_pred_rows.py does not
pin: a target count that ends on a 16-target border inside a 32-target span; one whose last
workgroup has one full wave, one partial group and two empty waves, with the scalar tail stores
inside a 64-B run; the pre-pass's 2,048-source buckets filtered per 512 sources on a dense Delta_1;
row shards with 64-B runs; 31 levels, which take every bound word and all five planes."""
import numpy as np
import pytest
from conftest import set_form

import level_graphs as lg
from shadow_amd import _lib, graphs
from shadow_amd._lib import ALGO_DENSE_FW
from shadow_amd.topology import build_tables

pytestmark = pytest.mark.gpu
REL_TOL = 1e-12
LEVELS = 12

_graphs = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _graphs.clear()


def _graph(kind):
    if kind not in _graphs:
        if kind == "complete144":
            _graphs[kind] = graphs.complete_graph(144, seed=7)
        elif kind == "complete150":
            _graphs[kind] = graphs.complete_graph(150, seed=7)
        elif kind == "ties":
            _graphs[kind] = graphs.complete_graph(640, seed=11, lat_max=3)
        elif kind == "shards":
            _graphs[kind] = graphs.complete_graph(1000, seed=2)
        elif kind == "deep31":
            _graphs[kind] = lg.core_tail(31)
        else:
            raise KeyError(kind)
    return _graphs[kind]


def _require_kernel():
    """A library without lvl_pred_rows_kernel would read pkw=1 as its target-major form and pass
    every comparison below unchanged."""
    if "have" not in _graphs:
        with open(_lib.LIB_PATH, "rb") as f:
            _graphs["have"] = b"lvl_pred_rows_kernel" in f.read()
    assert _graphs["have"], "this library has no lvl_pred_rows_kernel"


def _build(monkeypatch, g, ngpus=None, **form):
    _require_kernel()
    set_form(monkeypatch, levels="1", **form)
    lat, rel, st = build_tables(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                algo=ALGO_DENSE_FW, ngpus=ngpus)
    assert st.dist_enc == LEVELS, st.dist_enc
    return lat, rel, st


def _both_ways(monkeypatch, g, what, ngpus=None, **form):
    """The pkw=1 build against the oracle and bit for bit against the pkw=2 build."""
    lat, rel, st = _build(monkeypatch, g, ngpus=ngpus, pkw="1", **form)
    exp = lg.oracle_table(g)
    bad = np.argwhere(lat != np.asarray(exp["lat_int"], np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} latency mismatches, first {bad[:5].tolist()}"
    err = np.abs(rel - exp["rel"]) / np.maximum(np.abs(exp["rel"]), 1e-300)
    assert float(err.max()) <= REL_TOL, f"{what}: max rel error {err.max()}"
    lat2, rel2, _ = _build(monkeypatch, g, ngpus=ngpus, pkw="2", **form)
    assert np.array_equal(lat, lat2), what
    diff = np.argwhere(rel.view(np.uint64) != rel2.view(np.uint64))
    assert diff.size == 0, (what, diff[:5].tolist())
    return st


@pytest.mark.parametrize("kind", ["complete144", "complete150"])
def test_w4_target_borders(gpu, monkeypatch, kind):
    """n = 144: n % 32 == 16, the last 32-target span ends exactly on a 16-target workgroup
    border. n = 150: n % 16 == 6 and n % 4 == 2, the last workgroup has one full wave, one partial
    group and two empty waves, and the scalar tail stores land inside a 64-B run."""
    _both_ways(monkeypatch, _graph(kind), kind)


@pytest.mark.parametrize("bcap", ["2048", "1", "-1"])
def test_w4_buckets_dense_near(gpu, monkeypatch, bcap):
    """1-3 ms arcs on 640 vertices (a dense Delta_1, many ties): buckets that cannot overflow,
    buckets that all do, no pre-pass -- read per 2,048-source chunk, filtered per 512."""
    st = _both_ways(monkeypatch, _graph("ties"), f"ties bcap={bcap}", bcap=bcap)
    if bcap == "2048":
        assert st.pred_near == 2048 and st.pred_near_over == 0, (st.pred_near, st.pred_near_over)
    elif bcap == "1":
        assert st.pred_near == 1 and st.pred_near_over > 0, (st.pred_near, st.pred_near_over)
    else:
        assert st.pred_near == 0, st.pred_near


def test_w4_virtual_ranks(gpu, monkeypatch):
    """Two row shards of n = 1000: src0 != 0 and rows past n in the last shard, with 64-B runs."""
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", "2")
    _both_ways(monkeypatch, _graph("shards"), "shards x2", ngpus=1, bcap="2048")


def test_w4_deep31(gpu, monkeypatch):
    """Largest distance 31: bounds off[t][0..32] and all five level planes through the 22-word
    layout."""
    st = _both_ways(monkeypatch, _graph("deep31"), "deep31")
    assert st.levels == 31, st.levels
