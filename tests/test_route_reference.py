"""The route reference (tests/route_reference.py) pinned against the CPU oracle, before it judges
the kernels (test_gpu_routes.py): its predecessors equal oracle.sssp_rows(want_pred=True)["pred"]
exactly, and the left-to-right reliability product along its chains equals the oracle's `rel` bit
for bit."""
import numpy as np
import pytest

import oracle
import route_graphs
import route_reference as rr


def _oracle_rows(g, s0=0, s1=None):
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    return oracle.sssp_rows(el, s0, s1, want_pred=True)


def _check_pred(g, s0=0, s1=None):
    s1 = g.n if s1 is None else s1
    exp = _oracle_rows(g, s0, s1)
    srcs = np.arange(s0, s1)
    D = rr.distances_of_oracle(exp["lat_int"], srcs)
    pred = rr.pred_from_distances(g, D, srcs)
    bad = np.argwhere(pred != exp["pred"])
    assert bad.size == 0, f"{g.name}: {len(bad)} predecessors differ, first {bad[:5].tolist()}"
    return exp, pred


def _check_rel(g, exp, pred, s0=0):
    arcs = rr.InArcs(g)
    for i in range(pred.shape[0]):
        s = s0 + i
        rel = rr.rel_along(g, pred[i], s, arcs)
        off = np.arange(g.n) != s  # the diagonal holds the path-to-self rule
        assert np.array_equal(rel[off], exp["rel"][i][off]), (g.name, s)


def test_c1_pred_and_rel():
    g = route_graphs.c1()
    exp, pred = _check_pred(g)
    _check_rel(g, exp, pred)


def test_tie_graphs_pred_and_rel():
    for g in route_graphs.tie_graphs():
        exp, pred = _check_pred(g)
        _check_rel(g, exp, pred)


@pytest.mark.parametrize("ring", [True, False])
def test_directed_random_pred(ring):
    g = route_graphs.directed_random(ring)
    exp, pred = _check_pred(g)
    unreachable = exp["lat_int"] == oracle.U64_MAX
    assert unreachable.any() == (not ring)
    assert (pred[unreachable] == -1).all()
    hops, first = rr.walk(pred[0], 0)
    assert ((hops < 0) == unreachable[0]).all() and ((first < 0) == (pred[0] < 0)).all()


def test_ring_depth_and_tied_antipode():
    g = route_graphs.ring3000()
    exp, pred = _check_pred(g, 0, 1)
    hops, first = rr.walk(pred[0], 0)
    assert hops.max() == 1500 and pred[0][1500] == 1499
    assert first[1500] == 1 and first[1501] == 2999 and hops[1] == 1 and first[1] == 1


def test_walk_and_chain_small():
    #      0 -> 1 -> 2, 0 -> 3, 4 unreachable
    pred = np.array([-1, 0, 1, 0, -1], np.int32)
    hops, first = rr.walk(pred, 0)
    assert hops.tolist() == [0, 1, 2, 1, -1] and first.tolist() == [-1, 1, 1, 3, -1]
    assert rr.chain(pred, 0, 2) == [0, 1, 2] and rr.chain(pred, 0, 0) == [0]
    assert rr.chain(pred, 0, 4) is None
