"""The link-load reference (tests/load_reference.py) pinned before it judges the kernel
(test_gpu_link_load.py): its two formulations -- the level-order subtree sum and the brute-force
walk of every pair's route -- agree, hand-built graphs give the loads worked out by hand, and the
recorded figures of C1 and the 3,000-ring hold. Direct mode (use_shortest_path = 0) needs no device
and runs through the library here."""
import os

import numpy as np
import pytest

import load_reference as lr
import route_graphs
from conftest import GOLDEN
from shadow_amd import graphs
from shadow_amd.topology import Topology, build_link_load

MS = 1_000_000


def both(g, sources=None, demand=None):
    srcs, pred, hops = lr.routes_of(g, sources)
    a = lr.subtree(g.n, srcs, pred, hops, demand)
    b = lr.brute(g.n, srcs, pred, demand)
    assert a.same(b), g.name
    assert a.max_hops == b.max_hops
    assert sum(a.arcs.values()) == a.hop_weighted  # the identity of the issue
    return a


def graph(n, directed, edges, name):
    e = np.array(edges, dtype=np.int64)
    return graphs.Graph(n, directed, e[:, 0].astype(np.int32), e[:, 1].astype(np.int32),
                        e[:, 2] * MS, np.zeros(len(e)), name)


def test_formulations_agree_c1_and_ties():
    g = route_graphs.c1()
    both(g)
    both(g, demand=lr.issue_demand(g.n))
    for t in route_graphs.tie_graphs():
        both(t)
        both(t, demand=lr.issue_demand(t.n))


@pytest.mark.parametrize("ring", [True, False])
def test_formulations_agree_directed_random(ring):
    g = route_graphs.directed_random(ring)
    res = both(g, demand=lr.issue_demand(g.n))
    assert res.self_demand == 84_584
    assert res.unrouted == (0 if ring else 376_938)
    assert len(res.arcs) == (2_021 if ring else 1_881)


def test_path_of_four():
    g = graph(4, False, [(0, 1, 1), (1, 2, 1), (2, 3, 1)], "path4")
    res = both(g)
    assert res.arcs == {(0, 1): 3, (1, 0): 3, (1, 2): 4, (2, 1): 4, (2, 3): 3, (3, 2): 3}
    assert res.through == [0, 4, 4, 0]
    assert (res.routed, res.unrouted, res.self_demand) == (12, 0, 4)
    assert res.hop_weighted == 20 and res.max_hops == 3


def test_star():
    g = graph(5, False, [(0, i, 1) for i in range(1, 5)], "star5")
    res = both(g)
    assert res.arcs == {**{(0, i): 4 for i in range(1, 5)}, **{(i, 0): 4 for i in range(1, 5)}}
    assert res.through == [12, 0, 0, 0, 0]
    assert res.hop_weighted == 32 and res.max_hops == 2


def test_diamond_tie_takes_the_lower_index():
    g = graph(4, False, [(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1)], "diamond")
    dem = (np.array([0], np.int32), np.array([3], np.int32), np.array([7], np.uint64))
    res = both(g, sources=[0], demand=dem)
    assert res.arcs == {(0, 1): 7, (1, 3): 7}
    assert res.through == [0, 7, 0, 0] and res.routed == 7


def test_unreachable_demand_is_counted():
    g = graph(3, True, [(0, 1, 1), (2, 0, 1)], "oneway3")
    dem = np.array([[4, 3, 5]])
    res = both(g, sources=[0], demand=dem)
    assert res.arcs == {(0, 1): 3}
    assert (res.routed, res.unrouted, res.self_demand) == (3, 5, 4)
    assert res.through == [0, 0, 0]


def test_duplicate_coo_entries_add():
    g = graph(4, False, [(0, 1, 1), (1, 2, 1), (2, 3, 1)], "path4")
    dem = (np.array([0, 0, 2], np.int32), np.array([3, 3, 2], np.int32),
           np.array([2, 5, 9], np.uint64))
    res = both(g, sources=[0, 2], demand=dem)
    assert res.arcs == {(0, 1): 7, (1, 2): 7, (2, 3): 7}
    assert res.through == [0, 7, 7, 0]
    assert (res.routed, res.unrouted, res.self_demand) == (7, 0, 9)


def test_c1_uniform_pin():
    res = both(route_graphs.c1())
    assert len(res.arcs) == 260
    assert sum(res.arcs.values()) == 7_812 == res.hop_weighted
    assert max(res.arcs.values()) == 165
    assert res.self_demand == 50 and res.unrouted == 0


def test_ring3000_pin():
    g = route_graphs.ring3000()
    srcs, pred, hops = lr.routes_of(g, [0, 1499])
    res = lr.subtree(g.n, srcs, pred, hops)
    for arc in ((0, 1), (0, 2999), (1499, 1500), (1499, 1498)):
        assert res.arcs[arc] == 1_500, arc
    assert sum(res.arcs.values()) == 4_500_000 == res.hop_weighted
    assert res.self_demand == 2 and res.max_hops == 1_500


def test_build_link_load_direct_mode():
    """load(s -> t) = c(s, t), through = 0, computed on the host."""
    g = route_graphs.c1()
    srcs = np.array([0, 7, 49], np.int32)
    tail, head, load, through, st = build_link_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                    sources=srcs, use_shortest_path=False)
    want = [(int(s), t) for s in srcs for t in range(g.n) if t != s]
    assert list(zip(tail.tolist(), head.tolist())) == want
    assert (load == 1).all() and load.dtype == np.uint64
    assert not through.any() and len(through) == g.n
    assert (st.routed, st.unrouted, st.self_demand) == (3 * 49, 0, 3)
    assert st.ms_load == 0.0 and st.forms == 0 and st.max_hops == 1
    dem = np.zeros((3, g.n), np.int64)
    dem[0, 5], dem[1, 7], dem[2, 0], dem[2, 48] = 11, 6, 1 << 40, 3
    tail, head, load, through, st = build_link_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                    sources=srcs, demand=dem,
                                                    use_shortest_path=False)
    assert list(zip(tail.tolist(), head.tolist(), load.tolist())) == [(0, 5, 11), (49, 0, 1 << 40),
                                                                      (49, 48, 3)]
    assert (st.routed, st.self_demand) == ((1 << 40) + 14, 6) and not through.any()
    # duplicates add; the total must fit u64
    coo = (np.array([3, 3], np.int32), np.array([9, 9], np.int32), np.array([5, 6], np.uint64))
    tail, head, load, _, _ = build_link_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss, demand=coo,
                                             use_shortest_path=False)
    assert (tail.tolist(), head.tolist(), load.tolist()) == ([3], [9], [11])
    big = (np.array([3, 4], np.int32), np.array([9, 9], np.int32),
           np.array([(1 << 64) - 1, 1], np.uint64))
    with pytest.raises(RuntimeError, match="SRT_E_RANGE"):
        build_link_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss, demand=big,
                        use_shortest_path=False)
    unsorted = (np.array([4, 3], np.int32), np.array([9, 9], np.int32), np.array([1, 1], np.uint64))
    with pytest.raises(RuntimeError, match="SRT_E_ARG"):
        build_link_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss, demand=unsorted,
                        use_shortest_path=False)
    ring = route_graphs.ring3000()
    with pytest.raises(RuntimeError, match="complete graph"):
        build_link_load(ring.n, False, ring.src, ring.dst, ring.lat_ns, ring.loss,
                        use_shortest_path=False)


def test_build_link_load_empty_demand():
    """A COO demand with no entry has no source: nothing is routed, and no device is asked for."""
    g = route_graphs.c1()
    coo = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint64))
    tail, head, load, through, st = build_link_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                    demand=coo, use_shortest_path=True)
    assert len(tail) == len(head) == len(load) == 0
    assert (tail.dtype, head.dtype, load.dtype) == (np.int32, np.int32, np.uint64)
    assert through.dtype == np.uint64 and len(through) == g.n and not through.any()
    assert (st.routed, st.unrouted, st.self_demand) == (0, 0, 0)


def test_topology_link_load_direct_mode():
    """No packet has been counted (a lookup needs the tables, and those a device): the answer is
    empty, costs one build call and leaves the lookup side alone."""
    top = Topology.from_gml(open(os.path.join(GOLDEN, "c1.gml")).read(), use_shortest_path=False)
    ips = {v: f"100.9.{v}.1" for v in (2, 9, 30)}
    for v, ip in ips.items():
        assert top.attach(ip, 1, ip_hint=f"11.0.0.{v + 1}")[0] == v
    assert top.link_load_builds() == 0
    before = top.path_counts()
    tail, head, load, through, st = top.link_load()
    assert len(tail) == len(head) == len(load) == 0
    assert len(through) == top.n and not through.any()
    assert (st.routed, st.unrouted, st.self_demand) == (0, 0, 0)
    assert top.link_load_builds() == 1 and top.route_builds() == 0
    assert top.path_counts() == before
    assert all(top.path_source(ips[a], ips[b]) == -1 for a in ips for b in ips)
    top.free()
