"""The graphs of the route tests (test_route_reference.py, test_gpu_routes.py), built once each."""
import functools
import json
import os

import numpy as np

from shadow_amd import graphs

MS = 1_000_000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def c1():
    """C1: complete, n = 50, self-loops, 1-300 ms (tests/golden/c1.gml holds the same graph)."""
    return graphs.complete_graph(50, seed=1)


def tie_graphs():
    out = []
    for c in json.load(open(os.path.join(GOLDEN, "ties.json"))):
        e = np.array(c["edges"], dtype=np.float64)
        out.append(graphs.Graph(c["n"], bool(c["directed"]), e[:, 0].astype(np.int32),
                                e[:, 1].astype(np.int32), (e[:, 2] * MS).astype(np.int64), e[:, 3],
                                c["name"]))
    return out


@functools.lru_cache(maxsize=None)
def directed_random(ring=True):
    """test_gpu_parity.py::test_directed_random's graph: 300 vertices, 2,400 random arcs, a ring as
    the strongly connected backbone and a self-loop per vertex; ring=False leaves out the ring and
    (the random arcs alone still connect everything) every arc into the last five vertices, so
    some pairs are unreachable."""
    rng = np.random.default_rng(11)
    n, m = 300, 2400
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    idx = np.arange(n)
    src = np.concatenate([src, idx, idx]).astype(np.int32)
    dst = np.concatenate([dst, (idx + 1) % n, idx]).astype(np.int32)
    lat = (rng.integers(1, 20, len(src)) * MS).astype(np.int64)
    loss = rng.integers(0, 300, len(src)) / 10000.0
    if not ring:
        keep = np.ones(len(src), bool)
        keep[m:m + n] = False
        keep &= (dst < n - 5) | (src == dst)
        src, dst, lat, loss = src[keep], dst[keep], lat[keep], loss[keep]
    return graphs.Graph(n, True, src, dst, lat, loss, "directed300" + ("" if ring else "_noring"))


@functools.lru_cache(maxsize=None)
def ring3000():
    """3,000-ring, 1 ms edges, loss 0.001: from vertex 0 the deepest route has 1,500 hops and the
    antipode 1,500 is tied between 1,499 and 1,501."""
    n = 3000
    idx = np.arange(n)
    return graphs.Graph(n, False, idx.astype(np.int32), ((idx + 1) % n).astype(np.int32),
                        np.full(n, MS, np.int64), np.full(n, 0.001), "ring3000")


@functools.lru_cache(maxsize=None)
def complete_directed_holes():
    """complete_directed(300, lat_max=20) with a third of its edges removed -- every arc into the
    last ten vertices among them, so those are unreachable from everywhere else."""
    g = graphs.complete_directed(300, seed=12, lat_max=20)
    e = np.arange(g.m)
    keep = (e % 3 != 0) & ~((g.dst >= 290) & (g.src < 290))
    keep |= g.src == g.dst
    return graphs.Graph(g.n, True, g.src[keep], g.dst[keep], g.lat_ns[keep], g.loss[keep],
                        "dcomplete300_holes")


@functools.lru_cache(maxsize=None)
def submillisecond():
    """200 vertices, 0.3-0.7 ms edges: the quantum is 100 us, routes follow the integer quanta."""
    rng = np.random.default_rng(9)
    n = 200
    idx = np.arange(n)
    src = np.concatenate([idx, rng.integers(0, n, 900)]).astype(np.int32)
    dst = np.concatenate([(idx + 1) % n, rng.integers(0, n, 900)]).astype(np.int32)
    lat = (rng.integers(3, 8, len(src)) * 100_000).astype(np.int64)
    loss = rng.integers(0, 200, len(src)) / 10000.0
    return graphs.Graph(n, False, src, dst, lat, loss, "submillisecond200")
