"""tests/envelope_reference.py itself (CPU: the oracle's distances, numpy and plain Python), held to
the enumeration of every feasible path on small graphs. The GPU tests (test_gpu_envelope.py) hold
envelope.hip to this reference bit for bit."""
import numpy as np
import pytest

import oracle
import route_graphs
import route_reference as rr
import tie_reference
from envelope_reference import envelope
from shadow_amd import graphs

MS = 1_000_000


def graph(n, directed, edges, name="hand"):
    """edges: (u, v, ms, loss)."""
    e = np.array(edges, np.float64)
    return graphs.Graph(n, directed, e[:, 0].astype(np.int32), e[:, 1].astype(np.int32),
                        (e[:, 2] * MS).astype(np.int64), e[:, 3].copy(), name)


def distances(g):
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    tab = oracle.table(el, True, oracle.ORC_INT_NS, 1, raw=True)
    return rr.distances_of_oracle(tab["lat_int"], np.arange(g.n)), tab


def grid56(seed=7):
    """5 x 6 grid, 1-2 ms edges, distinct losses."""
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
    loss = rng.permutation(len(edges)) / 1000.0
    return graph(30, False, [(u, v, int(l), float(p)) for (u, v), l, p in zip(edges, lat, loss)],
                 "grid5x6")


def brute(g, D):
    """Every feasible path enumerated, in plain Python: per pair the smallest and largest
    left-to-right product and how many paths there are; the canonical arcs found here too."""
    n = g.n
    arc = {}
    for e in range(len(g.src)):
        ends = [(int(g.src[e]), int(g.dst[e]))]
        if not g.directed:
            ends.append((ends[0][1], ends[0][0]))
        for u, t in ends:
            if u != t and ((u, t) not in arc or int(g.lat_ns[e]) < arc[(u, t)][0]):
                arc[(u, t)] = (int(g.lat_ns[e]), 1.0 - float(g.loss[e]))
    lo, hi = np.zeros((n, n)), np.zeros((n, n))
    npaths = np.zeros((n, n), np.int64)
    for s in range(n):
        d = [0 if t == s else int(D[s][t]) for t in range(n)]
        M = {}
        for t in range(n):
            if t == s or d[t] >= rr.NO_DIST:
                continue
            tight = [u for u in range(n) if (u, t) in arc and d[u] < rr.NO_DIST
                     and d[u] + arc[(u, t)][0] == d[t]]
            M[t] = [u for u in tight if d[u] == min(d[x] for x in tight)]
        memo = {s: [[s]]}

        def paths(t):
            if t not in memo:
                memo[t] = [p + [t] for u in M[t] for p in paths(u)]
            return memo[t]

        lo[s][s] = hi[s][s] = 1.0
        for t in M:
            prods = []
            for p in paths(t):
                x = 1.0
                for a, b in zip(p[:-1], p[1:]):
                    x = x * arc[(a, b)][1]
                prods.append(x)
            lo[s][t], hi[s][t], npaths[s][t] = min(prods), max(prods), len(prods)
    return lo, hi, npaths


def check(g):
    D, _ = distances(g)
    env = envelope(g, D)
    lo, hi, npaths = brute(g, D)
    assert np.array_equal(env.lo.view(np.uint64), lo.view(np.uint64)), g.name
    assert np.array_equal(env.hi.view(np.uint64), hi.view(np.uint64)), g.name
    assert env.tied_pairs == tie_reference.tied_pairs(g.n, g.directed, g.src, g.dst, g.lat_ns, D)
    assert env.sensitive_pairs <= env.exposed_pairs and env.tied_pairs <= env.exposed_pairs
    assert np.array_equal(env.exposed, npaths >= 2), "exposed: more than one feasible path"
    assert not (env.sensitive & ~env.exposed).any() and not (env.tied & ~env.exposed).any()
    return env


def test_grid():
    """Untied targets downstream of tied ones inherit the dependence: exposed > tied."""
    env = check(grid56())
    assert 0 < env.tied_pairs < env.exposed_pairs and env.sensitive_pairs > 0
    assert (env.lo <= env.hi).all()


DIAMOND = [(0, 1, 1, 0.01), (0, 2, 1, 0.02), (1, 3, 1, 0.03), (2, 3, 1, 0.05)]


def test_diamonds():
    env = check(graph(4, False, DIAMOND))
    assert env.tied_pairs == 4 and env.sensitive_pairs == 4
    assert env.hi[0][3] == (1.0 * (1.0 - 0.01)) * (1.0 - 0.03)
    assert env.lo[0][3] == (1.0 * (1.0 - 0.02)) * (1.0 - 0.05)
    env = check(graph(4, True, DIAMOND))
    assert env.tied_pairs == 1 and env.exposed_pairs == 1 and env.max_sweeps == 2
    assert env.lo[1][0] == 0.0 and env.hi[1][0] == 0.0  # unreachable
    # a chain of two diamonds and a tail: the tail is exposed, not tied
    two = DIAMOND + [(3, 4, 1, 0.0), (3, 5, 1, 0.1), (4, 6, 1, 0.2), (5, 6, 1, 0.0), (6, 7, 1, 0.3)]
    env = check(graph(8, True, two))
    assert env.tied[0].sum() == 2 and env.exposed[0].sum() == 5 and env.depth[0][7] == 5
    # one arm longer: nothing tied
    env = check(graph(4, False, [(0, 1, 1, 0.01), (0, 2, 1, 0.02), (1, 3, 2, 0.03), (2, 3, 1, 0.05)]))
    assert env.tied_pairs == 0 and env.exposed_pairs == 0 and env.sensitive_pairs == 0


def test_equal_products_are_tied_and_exposed_but_not_sensitive():
    e = [(0, 1, 1, 0.25), (0, 2, 1, 0.5), (1, 3, 1, 0.5), (2, 3, 1, 0.25)]
    env = check(graph(4, True, e))
    assert env.tied[0][3] and env.exposed[0][3] and not env.sensitive[0][3]
    assert env.lo[0][3] == env.hi[0][3] == 0.375


def test_three_equal_arms():
    e = [(0, a, 1, 0.01 * a) for a in (1, 2, 3)] + [(a, 4, 1, 0.1 * a) for a in (1, 2, 3)]
    env = check(graph(5, False, e))
    assert env.tied_pairs == 2 + 6
    assert env.hi[0][4] == (1.0 - 0.01) * (1.0 - 0.1) and env.lo[0][4] == (1.0 - 0.03) * (1.0 - 0.3)


def test_two_tight_predecessors_at_different_distances():
    """The square 2+3 / 3+2: both in-arcs of 3 are tight from 0, but only 1 (D = 2) is in M: the
    product over 2 lies outside the bounds."""
    env = check(graph(4, False, [(0, 1, 2, 0.1), (1, 3, 3, 0.1), (0, 2, 3, 0.0), (2, 3, 2, 0.0)]))
    assert env.lo[0][3] == env.hi[0][3] == (1.0 - 0.1) * (1.0 - 0.1) and not env.exposed[0][3]


@pytest.mark.parametrize("g", route_graphs.tie_graphs(), ids=lambda g: g.name)
def test_golden_tie_graphs(g):
    check(g)


def test_c1_contains_the_oracle():
    """The oracle's own reliability (its tie rule is one heap order) lies within the bounds of
    every off-diagonal pair and equals both where they coincide."""
    g = route_graphs.c1()
    D, tab = distances(g)
    env = envelope(g, D)
    off = ~np.eye(g.n, dtype=bool)
    rel = tab["rel"]
    assert (env.lo[off] <= rel[off]).all() and (rel[off] <= env.hi[off]).all()
    same = off & ~env.sensitive
    assert np.array_equal(rel[same].view(np.uint64), env.lo[same].view(np.uint64))
    assert env.tied_pairs == tie_reference.tied_pairs(g.n, False, g.src, g.dst, g.lat_ns, D)
    assert env.sensitive_pairs <= env.exposed_pairs and env.tied_pairs <= env.exposed_pairs
