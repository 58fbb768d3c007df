"""Small graphs of the split-load tests (test_split_reference.py, test_gpu_split_load.py) and the
oracle's distance rows of a graph. The grid, the hand graph and the fans restate the shapes of the
envelope tests: the same ties, losses left out where they do not matter."""
import numpy as np

import oracle
import route_reference as rr
from shadow_amd import graphs

MS = 1_000_000


def graph(n, directed, edges, name):
    """edges: (u, v, ms)."""
    e = np.array(edges, np.int64)
    return graphs.Graph(n, directed, e[:, 0].astype(np.int32), e[:, 1].astype(np.int32),
                        e[:, 2] * MS, np.zeros(len(e)), name)


def distances(g, sources=None):
    """int64 [k, n]: the oracle's distance rows of `sources` (None: every vertex), the source's own
    entry 0, NO_DIST where unreachable."""
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    if sources is None:
        srcs = np.arange(g.n)
        lat = oracle.table(el, True, oracle.ORC_INT_NS, 8, raw=True)["lat_int"]
    else:
        srcs = np.asarray(sources)
        lat = oracle.sssp_list(el, srcs, nthreads=8)["lat_int"]
    return rr.distances_of_oracle(lat, srcs)


def grid56(seed=7):
    """5 x 6 grid, 1-2 ms edges: every |M| is 1 or 2."""
    rng = np.random.default_rng(seed)
    edges = []
    for y in range(5):
        for x in range(6):
            v = y * 6 + x
            if x < 5:
                edges.append((v, v + 1))
            if y < 4:
                edges.append((v, v + 6))
    lat = rng.integers(1, 3, len(edges))
    return graph(30, False, [(u, v, int(l)) for (u, v), l in zip(edges, lat)], "split_grid5x6")


def hand12():
    """Three components. 0-3: the square 2+3 / 3+2, both in-arcs of 3 tight from 0 at different
    distances, so M(0, 3) = {1}. 4-7 and 8-11: diamonds."""
    e = [(0, 1, 2), (1, 3, 3), (0, 2, 3), (2, 3, 2), (4, 5, 1), (4, 6, 1), (5, 7, 1), (6, 7, 1),
         (8, 9, 1), (8, 10, 1), (9, 11, 1), (10, 11, 1)]
    return graph(12, False, e, "split_hand12")


DIAMOND = [(0, 1, 1), (0, 2, 1), (1, 3, 1), (2, 3, 1)]


def diamonds():
    """The diamond undirected and directed, and a directed chain of two diamonds with a tail."""
    two = DIAMOND + [(3, 4, 1), (3, 5, 1), (4, 6, 1), (5, 6, 1), (6, 7, 1)]
    return [graph(4, False, DIAMOND, "split_diamond"), graph(4, True, DIAMOND, "split_diamond_dir"),
            graph(8, True, two, "split_two_diamonds")]


def three_arms():
    e = [(0, a, 1) for a in (1, 2, 3)] + [(a, 4, 1) for a in (1, 2, 3)]
    return graph(5, False, e, "split_three_arms")


def untied():
    """Graphs without a tied pair: a directed ring, and an odd undirected ring (the two ways
    round differ by at least one edge)."""
    n = 41
    idx = np.arange(n)
    ring = [(int(i), int((i + 1) % n), 1) for i in idx]
    return [graph(n, True, ring, "split_ring41_dir"), graph(n, False, ring, "split_ring41")]


def fans(k):
    """(g, sources, targets): two fans s - {k arms} - t, every edge 1 ms, so |M(s, t)| = k and t's
    in-list holds the arms in vertex order; k >= 32 takes the wave-wide walk."""
    edges, srcs, tgts = [], [], []
    v = 0
    for _ in range(2):
        s, arms, t = v, range(v + 1, v + 1 + k), v + 1 + k
        v = t + 1
        edges += [(s, a, 1) for a in arms] + [(a, t, 1) for a in arms]
        srcs.append(s)
        tgts.append(t)
    return graph(v, False, edges, f"split_fans{k}"), np.array(srcs), np.array(tgts)


def skewed_attachment(n, m=3, seed=5, lat_max=100):
    """A preferential-attachment-like graph built in one numpy pass: vertex v >= 1 links to m
    earlier vertices floor(v * r^3), r uniform, so low ids become hubs with in-lists of thousands
    of arcs, 1 .. lat_max ms edges. graphs.barabasi_albert draws vertex by vertex and takes half a
    minute at the sizes this one is for."""
    rng = np.random.default_rng(seed)
    v = np.repeat(np.arange(1, n, dtype=np.int64), m)
    u = (v * rng.random(len(v)) ** 3).astype(np.int64)
    lat = rng.integers(1, lat_max + 1, len(v)) * MS
    return graphs.Graph(n, False, v.astype(np.int32), u.astype(np.int32), lat.astype(np.int64),
                        np.zeros(len(v)), f"split_skewed{n}_{m}_{seed}")
