"""A plain numpy / Python-int reference for the link load (linkload.hip), sharing no
code with any kernel.

Given the canonical predecessor rows (oracle.sssp_rows(..., want_pred=True)), their hop counts
(route_reference.walk) and a demand c(s, t):
  load(u -> t)  = the sum of c(s, x) over the pairs whose route from s crosses the arc u -> t
  through(v)    = the sum of c(s, x) over the pairs whose route has v strictly inside
  self_demand   = the demand at t == s, unrouted = the demand at unreachable t, routed = the rest
Two formulations: `subtree` sums each source's predecessor tree level by level, deepest first;
`brute` walks route_reference.chain of every pair with demand. They must agree.
"""
import numpy as np

import oracle
import route_reference as rr

_ROUTES = {}


def routes_of(g, sources=None):
    """(sources int64 [k], pred int32 [k, n], hops int32 [k, n]) of the oracle for `sources` (None:
    every vertex), cached per graph and source set and never modified."""
    key = (g.name, None if sources is None else tuple(int(s) for s in sources))
    if key not in _ROUTES:
        el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
        if sources is None:
            srcs = np.arange(g.n)
            pred = oracle.sssp_rows(el, nthreads=8, want_pred=True)["pred"]
        else:
            srcs = np.asarray(sources, np.int64)
            pred = np.concatenate([oracle.sssp_rows(el, int(s), int(s) + 1, want_pred=True)["pred"]
                                   for s in srcs])
        hops = np.stack([rr.walk(pred[i], int(s))[0] for i, s in enumerate(srcs)])
        pred.setflags(write=False)
        hops.setflags(write=False)
        _ROUTES[key] = (srcs, pred, hops)
    return _ROUTES[key]


class Load:
    """arcs: {(tail, head): load} with load > 0 (Python ints); through: Python ints [n]."""

    def __init__(self, n):
        self.n = n
        self.arcs = {}
        self.through = [0] * n
        self.routed = self.unrouted = self.self_demand = 0
        self.hop_weighted = 0  # the sum of c(s, t) * hops(s, t) over the routed pairs
        self.max_hops = 0      # the deepest route of the rows that carry routed demand

    def arrays(self):
        """(tail int32, head int32, load u64) by (tail, head), through u64."""
        keys = sorted(self.arcs)
        return (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32),
                np.array([self.arcs[k] for k in keys], np.uint64),
                np.array(self.through, np.uint64))

    def same(self, other):
        return (self.arcs == other.arcs and self.through == other.through and
                (self.routed, self.unrouted, self.self_demand, self.hop_weighted) ==
                (other.routed, other.unrouted, other.self_demand, other.hop_weighted))


def dense_demand(demand, k, n):
    """rows(i) -> the u64 demand row of source i, from None (uniform), a [k, n] array or a COO
    triple (dsrc, dtgt, dval) whose distinct sources, in order, are the k sources."""
    if demand is None:
        one = np.ones(n, np.uint64)
        return lambda i: one
    if isinstance(demand, tuple):
        dsrc, dtgt, dval = (np.asarray(a) for a in demand)
        starts = np.flatnonzero(np.r_[True, dsrc[1:] != dsrc[:-1]]) if len(dsrc) else np.zeros(0, int)
        assert len(starts) == k
        ends = np.r_[starts[1:], len(dsrc)]

        def row(i):
            out = np.zeros(n, np.uint64)
            np.add.at(out, dtgt[starts[i]:ends[i]], dval[starts[i]:ends[i]].astype(np.uint64))
            return out
        return row
    d = np.asarray(demand)
    assert d.shape == (k, n)
    return lambda i: d[i].astype(np.uint64)


def subtree(n, sources, pred, hops, demand=None):
    """The level-order subtree sums: flow(t) = c(s, t) + the flow of t's children."""
    res = Load(n)
    row_of = dense_demand(demand, len(sources), n)
    for i, s in enumerate(sources):
        s = int(s)
        c = row_of(i)
        h = np.asarray(hops[i], np.int64)
        p = np.asarray(pred[i], np.int64)
        on = h >= 1
        res.self_demand += int(c[s])
        res.unrouted += sum(int(x) for x in c[(h < 0)])
        routed = sum(int(x) for x in c[on])
        res.routed += routed
        if not routed:
            continue
        res.hop_weighted += sum(int(x) * int(y) for x, y in zip(c[on], h[on]) if x)
        res.max_hops = max(res.max_hops, int(h.max()))
        flow = np.where(on, c, np.uint64(0)).astype(np.uint64)
        for level in range(int(h.max()), 0, -1):
            ts = np.flatnonzero(h == level)
            ts = ts[flow[ts] > 0]
            for t in ts:
                key = (int(p[t]), int(t))
                res.arcs[key] = res.arcs.get(key, 0) + int(flow[t])
            if level > 1:
                np.add.at(flow, p[ts], flow[ts])
        inner = np.flatnonzero(on & (flow > c))
        for v in inner:
            res.through[v] += int(flow[v]) - int(c[v])
    return res


def brute(n, sources, pred, demand=None):
    """Every pair's route walked: route_reference.chain, one pair at a time."""
    res = Load(n)
    row_of = dense_demand(demand, len(sources), n)
    for i, s in enumerate(sources):
        s = int(s)
        c = row_of(i)
        deepest, routed = 0, 0
        for t in range(n):
            path = rr.chain(pred[i], s, t)
            if path is not None and len(path) - 1 > deepest:
                deepest = len(path) - 1
            x = int(c[t])
            if not x:
                continue
            if t == s:
                res.self_demand += x
            elif path is None:
                res.unrouted += x
            else:
                routed += x
                res.hop_weighted += x * (len(path) - 1)
                for u, v in zip(path, path[1:]):
                    res.arcs[(u, v)] = res.arcs.get((u, v), 0) + x
                for v in path[1:-1]:
                    res.through[v] += x
        res.routed += routed
        if routed:
            res.max_hops = max(res.max_hops, deepest)
    return res


def reference(g, sources=None, demand=None):
    """The subtree formulation over the oracle's routes of g."""
    srcs, pred, hops = routes_of(g, sources)
    return subtree(g.n, srcs, pred, hops, demand)


def issue_demand(n):
    """The random demand of the directed tests: about half the pairs, below 1,000 each."""
    rng = np.random.default_rng(3)
    return rng.integers(0, 1000, (n, n)) * (rng.random((n, n)) < 0.5)
