"""Route queries in direct mode (use_shortest_path = 0): every pair is its own edge, so the routes
need no device and the drop-in layer's cache, walk and string run in the CPU suite."""
import os

import numpy as np
import pytest

import route_graphs
import route_reference as rr
from conftest import GOLDEN
from shadow_amd import graphs
from shadow_amd.topology import Topology, build_routes


def test_build_routes_direct_mode():
    g = route_graphs.c1()
    srcs = np.array([0, 7, 49], np.int32)
    pred, first, hops, st = build_routes(g.n, False, g.src, g.dst, g.lat_ns, g.loss, sources=srcs,
                                         use_shortest_path=False)
    t = np.arange(g.n)[None, :]
    own = t == srcs[:, None]
    assert np.array_equal(pred, np.where(own, -1, srcs[:, None]))
    assert np.array_equal(first, np.where(own, -1, t))
    assert np.array_equal(hops, np.where(own, 0, 1))
    assert st.ms_routes == 0.0 and st.max_hops == 0
    with pytest.raises(RuntimeError, match="SRT_E_ARG"):
        build_routes(g.n, False, g.src, g.dst, g.lat_ns, g.loss, sources=[7, 3],
                     use_shortest_path=False)
    ring = route_graphs.ring3000()
    with pytest.raises(RuntimeError, match="complete graph"):
        build_routes(ring.n, False, ring.src, ring.dst, ring.lat_ns, ring.loss,
                     use_shortest_path=False)


def test_topology_routes_direct_mode():
    top = Topology.from_gml(open(os.path.join(GOLDEN, "c1.gml")).read(), use_shortest_path=False)
    n, directed, src, dst, lat_ns, loss = top.edges()
    arcs = rr.InArcs(graphs.Graph(n, directed, src, dst, lat_ns, loss))
    ips = {v: f"100.9.{v}.1" for v in (2, 9, 30)}
    for v, ip in ips.items():
        assert top.attach(ip, 1, ip_hint=f"11.0.0.{v + 1}")[0] == v
    assert top.route_builds() == 0
    for a in ips:
        for b in ips:
            want = [a] if a == b else [a, b]
            assert top.route(ips[a], ips[b]) == want
            text = top.route_string(ips[a], ips[b])
            if a == b:
                assert text == str(a)
            else:
                _, e = arcs.arc(a, b)
                assert text == "%d<--[%f,%f]-->%d" % (a, lat_ns[e] / 1e6, 1.0 - (1.0 - loss[e]), b)
    assert top.route_builds() == 1  # one build: the asked source and the attached vertices
    assert top.route_vertices(17, 2) == [17, 2] and top.route_builds() == 2
    assert top.route(ips[2], ips[9], cap=1) == [2] and top.route_count == 2
    assert top.path_counts()["shortest_paths"] == 0
    assert all(top.path_source(ips[a], ips[b]) == -1 for a in ips for b in ips)
    top.free()
