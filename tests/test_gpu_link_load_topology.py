"""The drop-in layer's link load (srt_topology_link_load, include/topology.h) on C1 with 12
attached hosts and on a small directed topology (run on an MI355X with -m gpu): after a replayed
packet trace the loads equal the reference's over the demand read back from packet_count and
path_source -- each pair's packets charged along the route of its serving source -- and the call
leaves every lookup-side state as it was."""
import os

import numpy as np
import pytest

import load_reference as lr
from conftest import GOLDEN
from shadow_amd import graphs
from shadow_amd.topology import Topology, ip_to_net, set_min_time_jump_hook

pytestmark = pytest.mark.gpu
VERTS = [0, 3, 7, 11, 12, 20, 25, 31, 38, 42, 47, 49]


def host_ip(v):
    return f"100.8.{v}.1"


def replay(top, verts, k, seed):
    """k random packets between the hosts of `verts` (self packets among them)."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, len(verts), k)
    b = rng.integers(0, len(verts), k)
    src = np.array([ip_to_net(host_ip(verts[i])) for i in a], np.uint32)
    dst = np.array([ip_to_net(host_ip(verts[i])) for i in b], np.uint32)
    delivered, _ = top.send_packets(src, dst, rng.random(k))
    assert delivered.any()


def lookup_state(top, verts):
    pairs = [(a, b) for a in verts for b in verts]
    return (top.path_counts(),
            [top.packet_count(host_ip(a), host_ip(b)) for a, b in pairs],
            [top.path_source(host_ip(a), host_ip(b)) for a, b in pairs],
            top.min_latency_ms(), top.route_builds())


def demand_of_counters(top, verts):
    """The COO demand the counters stand for: a pair has one Path and one counter, whichever way it
    was looked up, and its packets run from the serving source to the other end."""
    dem = {}
    for i, a in enumerate(verts):
        for b in verts[i:]:
            cnt = top.packet_count(host_ip(a), host_ip(b))
            assert cnt == top.packet_count(host_ip(b), host_ip(a))
            if not cnt:
                continue
            frm = top.path_source(host_ip(a), host_ip(b))
            assert frm in (a, b)
            dem[(frm, b if frm == a else a)] = cnt
    keys = sorted(dem)
    return (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32),
            np.array([dem[k] for k in keys], np.uint64))


def assert_link_load(top, g, verts):
    dem = demand_of_counters(top, verts)
    ref = lr.reference(g, sorted(set(dem[0].tolist())), dem)
    wt, wh, wl, wthr = ref.arrays()
    tail, head, load, through, st = top.link_load()
    assert np.array_equal(tail, wt) and np.array_equal(head, wh)
    assert np.array_equal(load, wl) and np.array_equal(through, wthr)
    assert (st.routed, st.unrouted, st.self_demand) == (ref.routed, ref.unrouted, ref.self_demand)
    assert sum(int(x) for x in load) == ref.hop_weighted and st.max_hops == ref.max_hops
    return dem, st


def test_counters_to_link_load_and_no_side_effects(gpu):
    top = Topology.from_gml(open(os.path.join(GOLDEN, "c1.gml")).read())
    n, directed, src, dst, lat_ns, loss = top.edges()
    g = graphs.Graph(n, directed, src, dst, lat_ns, loss, "c1.gml")
    for v in VERTS:
        assert top.attach(host_ip(v), 1, ip_hint=f"11.0.0.{v + 1}")[0] == v
    calls = []
    cb = set_min_time_jump_hook(lambda ms: calls.append(ms))
    try:
        replay(top, VERTS, 4000, seed=21)
        before, ncalls = lookup_state(top, VERTS), len(calls)
        assert top.link_load_builds() == 0
        dem, st = assert_link_load(top, g, VERTS)
        assert st.self_demand > 0 and st.routed > 0          # self packets are counted apart
        assert st.self_demand == int(dem[2][dem[0] == dem[1]].sum())
        assert lookup_state(top, VERTS) == before and len(calls) == ncalls
        assert top.link_load_builds() == 1
        # more packets: a second call answers the new counters
        replay(top, VERTS, 1500, seed=22)
        dem2, st2 = assert_link_load(top, g, VERTS)
        assert st2.routed > st.routed and top.link_load_builds() == 2
    finally:
        set_min_time_jump_hook(None)
        del cb
        top.free()


def test_directed_topology(gpu):
    """A strongly connected directed topology: a pair's packets follow the serving source's own
    route, which differs from the reverse one."""
    idx = np.arange(8)
    g = graphs.Graph(8, True, np.concatenate([idx, idx]).astype(np.int32),
                     np.concatenate([(idx + 1) % 8, (idx + 3) % 8]).astype(np.int32),
                     (np.array([1, 2, 3, 1, 2, 3, 1, 2, 7, 7, 7, 7, 7, 7, 7, 7]) * 1_000_000)
                     .astype(np.int64), np.arange(16) / 200.0, "dring8")
    top = Topology.from_gml(graphs.to_gml(g))
    verts = list(range(8))
    for v in verts:
        top.attach(host_ip(v), 1, ip_hint=f"11.0.0.{v + 1}")
    replay(top, verts, 600, seed=23)
    before = lookup_state(top, verts)
    dem, st = assert_link_load(top, g, verts)
    assert st.routed > 0 and st.unrouted == 0
    assert lookup_state(top, verts) == before
    top.free()
