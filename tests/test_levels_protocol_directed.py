"""The numpy restatement of the directed N-rank level build's extraction
(tests/levels_protocol_directed.py) against the dense weights themselves -- it is the yardstick
tests/test_gpu_directed_ranks.py holds the C build's collective log to, so it is held to the
definition here: after the placement and the sort every rank has, for every target, the column of
w restricted to 1 <= w <= lw and sorted by (weight, source), and the ranks' blocks add up to the
weight histogram. No GPU, no oracle: the graphs' weights only."""
import numpy as np
import pytest

import level_graphs as lg
import levels_protocol_directed as lpd
from level_graphs import MS
from shadow_amd import graphs


def _dense_weights(g):
    """w[k, j] quanta of the arc k -> j (the lightest of parallel arcs), INF where there is none."""
    w = np.full((g.n, g.n), lpd.INF, np.int64)
    np.minimum.at(w, (g.src, g.dst), g.lat_ns // MS)
    return w


def _directed_dense(n=500, seed=5, wmax=40):
    rng = np.random.default_rng(seed)
    i, j = np.nonzero(rng.random((n, n)) < 0.35)
    keep = i != j
    i, j = i[keep], j[keep]
    ring = np.arange(n)
    src = np.concatenate([i, ring]).astype(np.int32)
    dst = np.concatenate([j, (ring + 1) % n]).astype(np.int32)
    lat = (rng.integers(1, wmax + 1, len(src)) * MS).astype(np.int64)
    loss = rng.integers(0, 300, len(src)) / 10000.0
    return graphs.Graph(n, True, src, dst, lat, loss, f"directed{n}")


@pytest.fixture(scope="module", params=["dense500", "core_tail12"])
def weights(request):
    g = _directed_dense() if request.param == "dense500" else lg.core_tail(12, core=300, directed=True)
    return _dense_weights(g)


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("lw", [8, 12])
def test_merged_in_arcs_are_the_columns(weights, ranks, lw):
    arcw = lpd.arc_weights(weights)
    n = arcw.shape[0]
    off, wt, src = lpd.merged_in_arcs(arcw, ranks, lw)
    assert off[n] == wt.size == int(((arcw >= 1) & (arcw <= lw)).sum())
    for j in range(n):
        col = arcw[:, j]
        ks = np.nonzero((col >= 1) & (col <= lw))[0]
        o = np.lexsort((ks, col[ks]))  # by (weight, source)
        assert np.array_equal(src[off[j]:off[j + 1]], ks[o]), j
        assert np.array_equal(wt[off[j]:off[j + 1]], col[ks][o]), j


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("lw", [8, 12])
def test_block_sizes_add_up_to_the_histogram(weights, ranks, lw):
    arcw = lpd.arc_weights(weights)
    hist = np.bincount(arcw.ravel(), minlength=256)
    sizes = lpd.block_sizes(arcw, ranks, lw)
    assert sum(sizes) == int(hist[1:lw + 1].sum())
    assert lpd.wire_arcs(arcw, ranks, lw) % 2 == 0 and lpd.wire_arcs(arcw, ranks, lw) >= max(sizes)
    # a block holds the rank's own rows' arcs only
    for q in range(ranks):
        b, e = lpd.shard(lpd.padded(arcw.shape[0]), ranks, q)
        s = lpd.rank_block(arcw, ranks, q, lw)[2]
        assert s.size == 0 or (s.min() >= b and s.max() < e)
