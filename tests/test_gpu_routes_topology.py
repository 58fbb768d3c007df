"""The drop-in layer's route queries (srt_topology_route*, include/topology.h) on C1 with 12
attached hosts (run on an MI355X with -m gpu): routes equal the chains of the oracle's
predecessors, the string equals the reference's `path:` format (topology.c:1322, :1368-1369), and
a route query leaves every lookup-side state as it was."""
import os
import threading

import numpy as np
import pytest

import oracle
import route_reference as rr
from conftest import GOLDEN
from shadow_amd import graphs
from shadow_amd._lib import lib
from shadow_amd.topology import Topology, ip_to_net, set_min_time_jump_hook

pytestmark = pytest.mark.gpu
VERTS = [0, 3, 7, 11, 12, 20, 25, 31, 38, 42, 47, 49]


def host_ip(v):
    return f"100.7.{v}.1"


@pytest.fixture(scope="module")
def c1(gpu):
    """(topology with 12 hosts attached, its graph, the oracle's predecessor rows, in-arc index)"""
    top = Topology.from_gml(open(os.path.join(GOLDEN, "c1.gml")).read())
    n, directed, src, dst, lat_ns, loss = top.edges()
    g = graphs.Graph(n, directed, src, dst, lat_ns, loss, "c1.gml")
    for v in VERTS:
        vert, _, _, _ = top.attach(host_ip(v), 1, ip_hint=f"11.0.0.{v + 1}")
        assert vert == v
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    pred = oracle.sssp_rows(el, nthreads=8, want_pred=True)["pred"]
    yield top, g, pred, rr.InArcs(g)
    top.free()


def render(g, arcs, verts):
    """The reference's path string: "%li", then "%s[%f,%f]-->%li" per hop; c1.gml's ids are the
    vertex indices."""
    out = "%d" % verts[0]
    for u, t in zip(verts, verts[1:]):
        _, e = arcs.arc(u, t)
        out += "%s[%f,%f]-->%d" % ("--" if g.directed else "<--", float(g.lat_ns[e]) / 1e6,
                                   1.0 - (1.0 - float(g.loss[e])), t)
    return out


def lookup_state(top):
    pairs = [(a, b) for a in VERTS for b in VERTS]
    return (top.path_counts(),
            [top.packet_count(host_ip(a), host_ip(b)) for a, b in pairs],
            [top.path_source(host_ip(a), host_ip(b)) for a, b in pairs])


def test_routes_strings_and_no_side_effects(c1):
    top, g, pred, arcs = c1
    calls = []
    cb = set_min_time_jump_hook(lambda ms: calls.append(ms))
    try:
        # some lookup-side state to preserve: a few served pairs and counted packets
        top.get_latency(host_ip(3), host_ip(42))
        top.increment_path_packet_counter(host_ip(7), host_ip(11))
        before, ncalls = lookup_state(top), len(calls)
        assert any(x >= 0 for x in before[2]) and any(x < 0 for x in before[2])
        long_routes = 0
        for a in VERTS:
            for b in VERTS:
                if a == b:
                    continue
                want = rr.chain(pred[a], a, b)
                assert top.route(host_ip(a), host_ip(b)) == want, (a, b)
                assert top.route_count == len(want)
                assert top.route_string(host_ip(a), host_ip(b)) == render(g, arcs, want), (a, b)
                long_routes += len(want) > 2
        assert long_routes > 0  # routes through intermediate (mostly unattached) vertices
        assert lookup_state(top) == before and len(calls) == ncalls
    finally:
        set_min_time_jump_hook(None)
        del cb


def test_self_unattached_and_truncation(c1):
    top, g, pred, arcs = c1
    L = lib()
    assert top.route(host_ip(7), host_ip(7)) == [7] and top.route_count == 1
    assert top.route_string(host_ip(7), host_ip(7)) == "7"
    none = ip_to_net("9.9.9.9")
    assert L.srt_topology_route_ip(top._h, none, ip_to_net(host_ip(3)), None, 0) == -9
    assert L.srt_topology_route_ip(top._h, ip_to_net(host_ip(3)), none, None, 0) == -9
    assert L.srt_topology_route_string_ip(top._h, none, ip_to_net(host_ip(3)), None, 0) == -9
    assert L.srt_topology_route(top._h, 0, g.n, None, 0) == -1  # SRT_E_ARG
    a, b = next((a, b) for a in VERTS for b in VERTS
                if a != b and len(rr.chain(pred[a], a, b)) >= 3)
    want = rr.chain(pred[a], a, b)
    assert top.route(host_ip(a), host_ip(b), cap=2) == want[:2] and top.route_count == len(want)
    # snprintf semantics: the full length comes back, at most cap bytes are written
    full = render(g, arcs, want)
    import ctypes
    buf = ctypes.create_string_buffer(b"\xaa" * 32, 32)
    k = L.srt_topology_route_string_ip(top._h, ip_to_net(host_ip(a)), ip_to_net(host_ip(b)), buf, 10)
    assert k == len(full) and buf.value.decode() == full[:9] and buf.raw[10:] == b"\xaa" * 22
    # unattached intermediate vertices route too, by vertex index
    u = next(v for v in range(g.n) if v not in VERTS)
    assert top.route_vertices(u, 0) == rr.chain(pred[u], u, 0)


def test_rows_built_once_and_for_later_hosts(c1):
    """One build covers the asked source and every attached vertex; a host attached afterwards at
    a new vertex costs one more build and leaves the earlier rows alone."""
    top, g, pred, arcs = c1
    for a in VERTS:
        top.route(host_ip(a), host_ip(VERTS[0]))
    builds = top.route_builds()
    assert builds >= 1
    new = 5
    assert new not in VERTS
    top.attach(host_ip(new), 1, ip_hint=f"11.0.0.{new + 1}")
    assert top.route(host_ip(new), host_ip(49)) == rr.chain(pred[new], new, 49)
    assert top.route_builds() == builds + 1
    assert top.route(host_ip(49), host_ip(new)) == rr.chain(pred[49], 49, new)
    for a in VERTS:
        assert top.route(host_ip(a), host_ip(new)) == rr.chain(pred[a], a, new)
    assert top.route_builds() == builds + 1


def test_first_build_covers_the_attached_set(gpu):
    top = Topology.from_gml(open(os.path.join(GOLDEN, "c1.gml")).read())
    for v in VERTS:
        top.attach(host_ip(v), 1, ip_hint=f"11.0.0.{v + 1}")
    assert top.route_builds() == 0
    for a in VERTS:
        for b in VERTS:
            top.route(host_ip(a), host_ip(b))
    assert top.route_builds() == 1
    top.free()


def test_concurrent_queries(gpu):
    """Eight threads on a fresh topology (the first queries race for the build) get the
    single-threaded answers."""
    top = Topology.from_gml(open(os.path.join(GOLDEN, "c1.gml")).read())
    ref = Topology.from_gml(open(os.path.join(GOLDEN, "c1.gml")).read())
    for t in (top, ref):
        for v in VERTS:
            t.attach(host_ip(v), 1, ip_hint=f"11.0.0.{v + 1}")
    want = {(a, b): ref.route_vertices(a, b) for a in range(ref.n) for b in VERTS}
    errors = []

    def worker(seed):
        rng = np.random.default_rng(seed)
        try:
            for _ in range(300):
                a, b = int(rng.integers(0, top.n)), VERTS[int(rng.integers(0, len(VERTS)))]
                got = top.route_vertices(a, b)
                if got != want[(a, b)]:
                    errors.append((a, b, got))
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(s,)) for s in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    top.free()
    ref.free()


def test_directed_strings_and_no_unreachable_topology(gpu):
    """A directed topology renders "--[" hops. SRT_E_NOPATH cannot be provoked through a loaded
    topology: validation refuses a directed graph that is not strongly connected
    (topology.c:671-713), so the code is covered below the drop-in layer (test_gpu_routes.py:
    -1 in every output for unreachable pairs)."""
    idx = np.arange(6)
    g = graphs.Graph(6, True, np.concatenate([idx, idx]).astype(np.int32),
                     np.concatenate([(idx + 1) % 6, (idx + 2) % 6]).astype(np.int32),
                     (np.array([1, 2, 3, 1, 2, 3, 5, 5, 5, 5, 5, 5]) * 1_000_000).astype(np.int64),
                     np.arange(12) / 100.0, "dring6")
    top = Topology.from_gml(graphs.to_gml(g))
    for v in range(6):
        top.attach(host_ip(v), 1, ip_hint=f"11.0.0.{v + 1}")
    el = oracle.EdgeList(g.n, 1, g.src, g.dst, g.lat_ns, g.loss)
    pred = oracle.sssp_rows(el, want_pred=True)["pred"]
    arcs = rr.InArcs(g)
    for a in range(6):
        for b in range(6):
            want = rr.chain(pred[a], a, b)
            assert top.route(host_ip(a), host_ip(b)) == want
            assert top.route_string(host_ip(a), host_ip(b)) == render(g, arcs, want)
    assert "--[" in top.route_string(host_ip(0), host_ip(3))
    assert "<--" not in top.route_string(host_ip(0), host_ip(3))
    top.free()
    one_way = graphs.Graph(3, True, np.array([0, 1, 0], np.int32), np.array([1, 2, 2], np.int32),
                           np.full(3, 1_000_000, np.int64), np.zeros(3), "oneway")
    assert Topology.try_from_gml(graphs.to_gml(one_way)) is None
