"""The fixtures of test_gpu_fw_edges.py (tests/fw_graphs.py) at the parameters the GPU tests use,
on the CPU: every helper measures what it promises with the oracle and asserts it, so a graph
that misses its distance fails here, before any build runs on it."""
import numpy as np
import pytest

import fw_graphs as fg
import level_graphs as lg


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("e", fg.CAP_EDGES + [fg.ROWS_FAR])
def test_heavy_tail_measures_its_distance(native, e, directed):
    g = fg.heavy_tail(e, directed=directed)
    assert g.n == 261 and bool(g.directed) == directed
    assert lg.largest_distance(g) == e
    s, t = fg.farthest_pair(g)
    d = lg.oracle_table(g)["lat_int"]
    assert s != t and int(d[s, t]) == e * lg.MS
    assert (d != lg.U64_MAX).all()
    # the tail's rungs stay tied: both rails' vertices of a rung are equally far from the core
    a = g.core + 2 * np.arange(fg.RUNGS)
    assert np.array_equal(d[1, a], d[1, a + 1])


def test_heavy_tail_mid_rows_stay_below_the_rows_cap(native):
    g = fg.heavy_tail(fg.ROWS_FAR)
    v = fg.mid_tail_rows(g, fg.CAP_F - 1, g.n // 12)
    ecc = lg.row_eccentricity(g)
    assert 2 <= len(v) <= g.n // 12 and (v >= g.core).all()
    assert int(ecc[v].max()) <= fg.CAP_F - 1 < fg.CAP_F < int(ecc.max()) == fg.ROWS_FAR


@pytest.mark.parametrize("e_near,e_far", fg.FAR_PAIRS)
def test_one_rank_far_keeps_the_far_rows_in_the_last_block(native, e_near, e_far):
    g = fg.one_rank_far(e_far, e_near)
    ecc = lg.row_eccentricity(g)
    assert g.n == 384 and g.directed
    assert int(ecc[:256].max()) <= e_near and int(ecc[256:].max()) == e_far
    for ranks in (2, 3):
        b, e = lg.shard_rows(g.n, ranks)[-1]
        assert b <= 256 and e == 384
        assert int(ecc[:b].max()) <= e_near


def test_long_arc_traps_are_off_every_shortest_path(native):
    g = fg.long_arc_traps()
    assert g.n == 261 and lg.largest_distance(g) < 254
    d = lg.oracle_table(g)["lat_int"] // np.uint64(lg.MS)
    w = {(int(s), int(t)): int(l) // lg.MS for s, t, l in zip(g.src, g.dst, g.lat_ns)}
    assert sorted({w[p] for p in g.long_arcs if p not in g.traps}) == [fg.CAP_F, fg.CAP_U,
                                                                           0xFFFF, 0x10001]
    for u, t in g.traps:
        assert w[(u, t)] == 0x10000 + int(d[u, t]) and (w[(u, t)] & 0xFFFF) == int(d[u, t]) >= 2
    v = fg.trap_rows(g)  # the few-rows case: both ends of every 0x10000 + d arc among them
    assert len(v) <= g.n // 12 and {x for p in g.traps for x in p} <= set(v.tolist())
