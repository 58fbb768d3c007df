"""tests/split_reference.py itself (CPU: the oracle's distances, numpy and plain Python): its two
formulations held to each other, to the canonical link load where nothing is tied, and to hand
values. The GPU tests (test_gpu_split_load.py) hold splitload.hip to `by_distance`. Direct mode
(use_shortest_path = 0) and an empty demand need no device and run through the library here."""
import numpy as np
import pytest

import load_reference as lr
import route_graphs
import split_graphs as sg
import split_reference as sr
from route_reference import InArcs
from shadow_amd.topology import build_split_load


def both(g, demand=None):
    D = sg.distances(g)
    a, b = sr.by_distance(g, D, demand=demand), sr.brute(g, D, demand=demand)
    assert (a.routed, a.unrouted, a.self_demand, a.tied_pairs) == (
        b.routed, b.unrouted, b.self_demand, b.tied_pairs), g.name
    return a, b


def close(a, b, g):
    """load and through within the derived tolerance, zeros exact."""
    rtol = sr.rtol(len(a.load), g.n, g.n)
    for x, y in ((a.load, b.load), (a.through, b.through)):
        assert np.array_equal(x == 0.0, y == 0.0), g.name
        assert np.allclose(x, y, rtol=rtol, atol=0.0), (g.name, np.abs(x - y).max())


def bitwise(a, b, g):
    assert np.array_equal(a.load.view(np.uint64), b.load.view(np.uint64)), g.name
    assert np.array_equal(a.through.view(np.uint64), b.through.view(np.uint64)), g.name


def test_grid_bitwise():
    """Every |M| is 1 or 2 and the demand is uniform, so every value is dyadic and the recursion
    equals the exact fractions bit for bit."""
    g = sg.grid56()
    a, b = both(g)
    assert a.tied_pairs > 0
    close(a, b, g)
    bitwise(a, b, g)
    assert a.routed == g.n * (g.n - 1) and a.self_demand == g.n and a.unrouted == 0


@pytest.mark.parametrize("g", sg.diamonds() + [sg.three_arms()], ids=lambda g: g.name)
def test_small_tied_graphs(g):
    a, b = both(g)
    assert a.tied_pairs > 0
    close(a, b, g)


def test_three_arms_values():
    g = sg.three_arms()
    a = sr.by_distance(g, sg.distances(g, [0]), sources=[0], demand=(np.zeros(1, np.int32),
                                                                   np.array([4], np.int32),
                                                                   np.array([1], np.uint64)))
    tail, head, load, through = a.arrays()
    third = 1.0 / 3.0
    assert [(int(u), int(t)) for u, t in zip(tail, head)] == [(0, 1), (0, 2), (0, 3), (1, 4), (2, 4),
                                                               (3, 4)]
    assert (load == third).all() and (through[1:4] == third).all() and through[0] == through[4] == 0.0


@pytest.mark.parametrize("g", route_graphs.tie_graphs(), ids=lambda g: g.name)
def test_golden_tie_graphs(g):
    a, b = both(g, demand=lr.issue_demand(g.n))
    close(a, b, g)


@pytest.mark.parametrize("g", sg.untied(), ids=lambda g: g.name)
def test_untied_equals_the_canonical_load(g):
    """Without a tied pair every |M| is 1: the split load is the link load, bitwise."""
    dem = lr.issue_demand(g.n)
    a = sr.by_distance(g, sg.distances(g), demand=dem)
    assert a.tied_pairs == 0
    tail, head, load, through = a.arrays()
    wt, wh, wl, wthr, ref = sr.canonical(g, demand=dem)
    assert np.array_equal(tail, wt) and np.array_equal(head, wh)
    assert np.array_equal(load.view(np.uint64), wl.view(np.uint64))
    assert np.array_equal(through.view(np.uint64), wthr.view(np.uint64))
    assert (a.routed, a.unrouted, a.self_demand) == (ref.routed, ref.unrouted, ref.self_demand)


def test_hand12_members_are_not_all_tight_arcs():
    """From 0 both in-arcs of 3 are tight, but only 1 -> 3 is in M: nothing goes over 2 -> 3."""
    g = sg.hand12()
    a, b = both(g)
    close(a, b, g)
    bitwise(a, b, g)
    one = sr.by_distance(g, sg.distances(g, [0]), sources=[0])
    arcs = InArcs(g)
    k = arcs.ptr[3] + int(np.searchsorted(arcs.u[arcs.ptr[3]:arcs.ptr[4]], 2))
    assert arcs.u[k] == 2 and one.load[k] == 0.0
    assert one.load[arcs.ptr[3] + 0] == 1.0 and arcs.u[arcs.ptr[3]] == 1
    assert one.unrouted == 8 and one.routed == 3 and one.self_demand == 1


def test_build_split_load_direct_mode():
    """load(s -> t) = (double)c(s, t), through = 0, computed on the host."""
    g = route_graphs.c1()
    srcs = np.array([0, 7, 49], np.int32)
    tail, head, load, through, st = build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                     sources=srcs, use_shortest_path=False)
    want = [(int(s), t) for s in srcs for t in range(g.n) if t != s]
    assert list(zip(tail.tolist(), head.tolist())) == want
    assert (load == 1.0).all() and load.dtype == np.float64
    assert not through.any() and len(through) == g.n and through.dtype == np.float64
    assert (st.routed, st.unrouted, st.self_demand) == (3 * 49, 0, 3)
    assert st.ms_split == 0.0 and st.forms == 0 and st.tied_pairs == 0
    dem = np.zeros((3, g.n), np.int64)
    dem[0, 5], dem[1, 7], dem[2, 0], dem[2, 48] = 11, 6, 1 << 40, 3
    tail, head, load, through, st = build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                     sources=srcs, demand=dem,
                                                     use_shortest_path=False)
    assert list(zip(tail.tolist(), head.tolist(), load.tolist())) == [
        (0, 5, 11.0), (49, 0, float(1 << 40)), (49, 48, 3.0)]
    assert load.dtype == np.float64 and through.dtype == np.float64
    assert (st.routed, st.self_demand) == ((1 << 40) + 14, 6) and not through.any()
    # duplicates add; the total must stay below 2^53, where every sum is exact in f64
    coo = (np.array([3, 3], np.int32), np.array([9, 9], np.int32), np.array([5, 6], np.uint64))
    tail, head, load, through, _ = build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                    demand=coo, use_shortest_path=False)
    assert (tail.tolist(), head.tolist(), load.tolist()) == ([3], [9], [11.0])
    assert load.dtype == np.float64 and not through.any()
    most = (np.array([3, 4], np.int32), np.array([9, 9], np.int32),
            np.array([(1 << 53) - 2, 1], np.uint64))
    _, _, load, _, st = build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss, demand=most,
                                         use_shortest_path=False)
    assert load.tolist() == [float((1 << 53) - 2), 1.0] and st.routed == (1 << 53) - 1
    big = (most[0], most[1], np.array([(1 << 53) - 1, 1], np.uint64))
    with pytest.raises(RuntimeError, match="SRT_E_RANGE"):
        build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss, demand=big,
                         use_shortest_path=False)
    ring = route_graphs.ring3000()  # the 2^53 refusal comes first, the completeness check after it
    with pytest.raises(RuntimeError, match="SRT_E_RANGE"):
        build_split_load(ring.n, False, ring.src, ring.dst, ring.lat_ns, ring.loss, demand=big,
                         use_shortest_path=False)
    with pytest.raises(RuntimeError, match="complete graph"):
        build_split_load(ring.n, False, ring.src, ring.dst, ring.lat_ns, ring.loss,
                         use_shortest_path=False)


def test_build_split_load_empty_demand():
    """A COO demand with no entry has no source: nothing is routed, and no device is asked for."""
    g = route_graphs.c1()
    coo = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint64))
    tail, head, load, through, st = build_split_load(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                     demand=coo, use_shortest_path=True)
    assert len(tail) == len(head) == len(load) == 0
    assert (tail.dtype, head.dtype, load.dtype) == (np.int32, np.int32, np.float64)
    assert through.dtype == np.float64 and len(through) == g.n and not through.any()
    assert (st.routed, st.unrouted, st.self_demand) == (0, 0, 0)
