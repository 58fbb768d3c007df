"""srt_build_stats.ess_arcs of a dense build (shadow_amd/csrc/dense.hip): the essential-arc total
of the Floyd-Warshall post pass, on each of the ways it reaches the stats.

An arc (u, t), u != t, is essential when its latency is the distance: W[u][t] == D[u][t], with W
the smallest latency among the edges of the pair. The CPU count takes D from the oracle table. The
graphs are a complete graph with 1-300 ms arcs at n = 300 and, at n = 2,100, a preferential-
attachment graph of 8 edges per new vertex with 1-100 ms arcs (the dense build takes any graph as
a matrix; the oracle's 2,100 Dijkstra runs over a complete graph's 2.2 M edges would take ten
seconds and more). On both some arcs are beaten by longer paths and some are not, so the count is
neither 0 nor n (n - 1) (asserted before anything is built).

The total is read three ways: n <= 2,048 on one GPU sizes the lists for n (n - 1) arcs, lets the
kernels read the total on the device and copies it back after the build's final wait; a larger n
reads it in the middle of the pass; a row-sharded build all-reduces the per-row counts, after which
every rank holds the global lists and reports the global total -- srt_build_tables_multi hands
out rank 0's stats (it adds up the ranks' tied pairs and pre-pass overflows only), so R ranks
report 1 x the count, as one GPU does. A level build keeps no essential-arc lists and reports 0.
Every case also holds the tables to the oracle (check_tables)."""
import numpy as np
import pytest
from conftest import form_env

import level_graphs as lg
from level_graphs import check_tables
from shadow_amd import graphs
from shadow_amd._lib import ALGO_DENSE_FW
from shadow_amd.topology import build_tables

pytestmark = pytest.mark.gpu

_cache = {}


def _complete(n, directed=False, lat_max=300):
    """complete_graph(n); directed: the same arcs, each orientation an arc of its own."""
    key = (n, directed, lat_max)
    if key not in _cache:
        g = graphs.complete_graph(n, 7, lat_max=lat_max)
        if directed:
            off = g.src != g.dst
            g = graphs.Graph(n, True, np.concatenate([g.src, g.dst[off]]),
                             np.concatenate([g.dst, g.src[off]]),
                             np.concatenate([g.lat_ns, g.lat_ns[off]]),
                             np.concatenate([g.loss, g.loss[off]]), f"complete{n}_dir")
        _cache[key] = g
    return _cache[key]


def _sparse(n):
    if ("ba", n) not in _cache:
        _cache[("ba", n)] = graphs.barabasi_albert(n, m=8, seed=5)
    return _cache[("ba", n)]


def _essential(g):
    """Ordered pairs u != t with an edge whose smallest latency is lat_int[u][t]."""
    w = np.full((g.n, g.n), lg.U64_MAX, np.uint64)
    np.minimum.at(w, (g.src, g.dst), g.lat_ns.astype(np.uint64))
    if not g.directed:
        np.minimum.at(w, (g.dst, g.src), g.lat_ns.astype(np.uint64))
    hit = (w == lg.oracle_table(g)["lat_int"]) & (w != lg.U64_MAX)
    np.fill_diagonal(hit, False)
    count = int(hit.sum())
    assert 0 < count < g.n * (g.n - 1), count
    return count


def _build(g, ngpus=None):
    return build_tables(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss, algo=ALGO_DENSE_FW,
                        ngpus=ngpus)


@pytest.mark.parametrize("n", [300, 2100])
def test_ess_total_one_gpu(gpu, monkeypatch, n):
    """n = 300: the total read after the build's final wait; n = 2,100 (> 2,048, below the level
    build's 4,096): read in the middle of the pass."""
    monkeypatch.delenv("SRT_FORM", raising=False)
    monkeypatch.delenv("SRT_VIRTUAL_RANKS", raising=False)
    g = _complete(n) if n == 300 else _sparse(n)
    lat, rel, st = _build(g)
    assert st.dist_enc != lg.LEVELS, st.dist_enc
    assert st.ess_arcs == _essential(g), (st.ess_arcs, _essential(g))
    check_tables(g, lat, rel, f"ess total n={n}")


@pytest.mark.parametrize("directed", [False, True])
def test_ess_total_two_ranks(gpu, monkeypatch, directed):
    """The gather hook (directed: and the transposed in-arc lists). Every rank holds the global
    lists after the gather and srt_build_tables_multi reports rank 0's total: 1 x the count."""
    monkeypatch.delenv("SRT_FORM", raising=False)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", "2")
    g = _complete(300, directed)
    lat, rel, st = _build(g, ngpus=1)
    assert st.dist_enc != lg.LEVELS, st.dist_enc
    assert st.ess_arcs == _essential(g), (st.ess_arcs, _essential(g))
    check_tables(g, lat, rel, f"ess total x2 directed={directed}")


def test_ess_total_level_build(gpu, monkeypatch):
    """1-3 ms arcs under SRT_FORM levels=1: the level build, which keeps no essential-arc lists."""
    monkeypatch.delenv("SRT_VIRTUAL_RANKS", raising=False)
    g = _complete(300, lat_max=3)
    with form_env(levels="1"):
        lat, rel, st = _build(g)
    assert st.dist_enc == 12, st.dist_enc
    assert st.ess_arcs == 0, st.ess_arcs
    check_tables(g, lat, rel, "ess total levels")
