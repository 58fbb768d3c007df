"""Unreachable pairs through a forced level build (SRT_FORM levels=1), on one rank and on virtual
ranks. A level build whose sources never complete runs its whole budget, must then report "not
done" on every rank together, and Floyd-Warshall must give the table: the build returns OK,
dist_enc is not 12, latency is bit-exact against the CPU oracle (SRT_INF for the oracle's
UINT64_MAX), reliability is within 1e-12 on the reachable pairs, and the whole table -- the
unreachable pairs' reliability included -- is bit-equal to the build without levels=1.

Two kinds of graph (tests/level_graphs.py): two disjoint complete graphs (150 + 170 vertices,
1-4 ms), and a directed dense graph whose first vertices have no in-arcs from the rest, so the
block's sources reach everything and the other sources do not. With a block of 128 vertices
rank 0's rows are exactly the sources that complete. (A sharded build of a directed graph does not
take the levels at all -- a rank holds the out-arcs of its rows only -- so there it is the early
return of srt_levels_build that every rank must take alike.)

The same graphs without SRT_FORM through the dense and the sparse build: tests/test_gpu_parity.py's
directed graph carries a ring, so it has no unreachable pair."""
import numpy as np
import pytest
from conftest import set_form

import level_graphs as lg
from level_graphs import LEVELS, check_tables
from shadow_amd._lib import ALGO_DENSE_FW, ALGO_SPARSE_SSSP

pytestmark = pytest.mark.gpu


def _graph(kind):
    if kind == "two_complete":
        return lg.two_complete()
    return lg.closed_block(block=128 if kind == "closed_block128" else 40)


@pytest.mark.parametrize("ranks", [1, 2, 3])
@pytest.mark.parametrize("kind", ["two_complete", "closed_block", "closed_block128"])
def test_unreached_forced_levels(gpu, monkeypatch, kind, ranks):
    g = _graph(kind)
    ngpus = None
    if ranks > 1:
        monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
        ngpus = 1
        assert all(b < e for b, e in lg.shard_rows(g.n, ranks))
    monkeypatch.delenv("SRT_FORM", raising=False)
    lat0, rel0, st0 = lg.build(g, ngpus=ngpus)
    assert st0.dist_enc != LEVELS and st0.levels == 0, (st0.dist_enc, st0.levels)
    check_tables(g, lat0, rel0, f"{kind} x{ranks} FW", reachable_only=True)
    set_form(monkeypatch, levels="1")
    lat, rel, st = lg.build(g, ngpus=ngpus)  # (a failure on any rank raises here)
    assert st.dist_enc != LEVELS and st.levels == 0, (st.dist_enc, st.levels)
    check_tables(g, lat, rel, f"{kind} x{ranks} levels=1", reachable_only=True)
    assert np.array_equal(lat, lat0)
    assert np.array_equal(rel.view(np.uint64), rel0.view(np.uint64)), \
        np.argwhere(rel.view(np.uint64) != rel0.view(np.uint64))[:5]


@pytest.mark.parametrize("algo,kernel", [(ALGO_DENSE_FW, None), (ALGO_SPARSE_SSSP, None),
                                         (ALGO_SPARSE_SSSP, "ms"), (ALGO_SPARSE_SSSP, "wave")])
@pytest.mark.parametrize("kind", ["two_complete", "closed_block", "closed_block128"])
def test_unreached_plain_builds(gpu, monkeypatch, kind, algo, kernel):
    """No forced level build. The sparse default takes the multi-source kernel on these graphs
    (their relabelled arcs are local), whose source clusters are cut off a breadth-first sweep
    over out-arcs: in the directed graphs the sweep from the far end of the block's reach does
    not lead back into the block, and the block's sources must still land in a cluster (they
    were left out, their rows never written)."""
    monkeypatch.delenv("SRT_FORM", raising=False)
    if kernel:
        set_form(monkeypatch, kernel=kernel)
    g = _graph(kind)
    lat, rel, st = lg.build(g, algo=algo)
    unreached = lg.oracle_table(g)["lat_int"] == lg.U64_MAX
    assert unreached.any()
    if kernel:
        assert st.dist_enc == (1 if kernel == "wave" else 3), st.dist_enc
    check_tables(g, lat, rel, f"{kind} algo={algo} kernel={kernel}", reachable_only=True)
