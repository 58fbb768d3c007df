"""A plain numpy / Python reference for the split load (splitload.hip), sharing no
code with any kernel.

The rule, over the canonical arcs (route_reference.InArcs) and the oracle's integer distances with
the source's own taken as 0: with M(s, t) the set of envelope_reference.members and c(s, t) the u64
demand, every reachable t != s has
    inflow_s(t) = sum of share_s(v) over the v with t in M(s, v)
    f_s(t)      = float(c(s, t)) + inflow_s(t)
    share_s(t)  = f_s(t) / |M(s, t)|
and the source adds share_s(t) to load(u -> t) for every u in M(s, t) and inflow_s(t) to
through(t); a share that reaches s adds to no through word. self_demand is the demand at t == s,
unrouted the demand at unreachable t, routed the rest: Python ints.

Two formulations: `by_distance` runs the recursion over the targets in decreasing distance (every
member of M is strictly nearer, so all targets of one distance are final at once); `brute`
enumerates every feasible path of every pair with demand, weighs it by the product of 1 / |M| along
it in fractions.Fraction and rounds each sum once.
"""
from fractions import Fraction

import numpy as np

import load_reference as lr
from envelope_reference import members
from route_reference import NO_DIST, InArcs


class Split:
    """load f64 [arcs] by InArcs position, through f64 [n]; the totals and tied_pairs as ints."""

    def __init__(self, arcs):
        self.in_arcs = arcs
        self.n = arcs.n
        self.load = np.zeros(len(arcs.u), np.float64)
        self.through = np.zeros(arcs.n, np.float64)
        self.routed = self.unrouted = self.self_demand = 0
        self.tied_pairs = 0

    def arrays(self):
        """(tail int32, head int32, load f64) of the arcs with load > 0 by (tail, head), through."""
        head = np.repeat(np.arange(self.n), np.diff(self.in_arcs.ptr))
        on = np.flatnonzero(self.load > 0.0)
        order = on[np.lexsort((head[on], self.in_arcs.u[on]))]
        return (self.in_arcs.u[order].astype(np.int32), head[order].astype(np.int32),
                self.load[order], self.through)

    def freeze(self):
        self.load.setflags(write=False)
        self.through.setflags(write=False)
        return self


def _rows(D, sources, n):
    sources = np.arange(n) if sources is None else np.asarray(sources)
    D = np.array(D, np.int64)
    assert D.shape == (len(sources), n)
    return D, sources


def by_distance(g, D, sources=None, demand=None, arcs=None):
    """The Split of `sources` (default: every vertex) from their distance rows D (int64 [k, n], the
    edge list's unit, NO_DIST where unreachable; the source's own entry is treated as 0) and a
    demand as load_reference.dense_demand takes it (None: uniform)."""
    arcs = arcs or InArcs(g)
    n = arcs.n
    D, sources = _rows(D, sources, n)
    head = np.repeat(np.arange(n), np.diff(arcs.ptr))
    row_of = lr.dense_demand(demand, len(sources), n)
    out = Split(arcs)
    for i, s in enumerate(sources):
        s = int(s)
        Dr = D[i]
        Dr[s] = 0
        c = row_of(i)
        reach = Dr < NO_DIST
        reach[s] = False
        out.self_demand += int(c[s])
        out.unrouted += sum(int(x) for x in c[~reach] if x) - int(c[s])
        routed = sum(int(x) for x in c[reach] if x)
        out.routed += routed
        m = np.flatnonzero(members(arcs, head, Dr, s))
        mu, mt = arcs.u[m], head[m]
        cnt = np.bincount(mt, minlength=n)
        assert (cnt[reach] > 0).all() and not cnt[~reach].any(), "D is no distance row of g"
        out.tied_pairs += int((cnt >= 2).sum())
        if not routed:
            continue
        order = np.argsort(-Dr[mt], kind="stable")       # decreasing distance of the target
        m, mu, mt = m[order], mu[order], mt[order]
        inflow = np.zeros(n, np.float64)
        share = np.zeros(n, np.float64)
        cuts = np.flatnonzero(np.diff(Dr[mt])) + 1
        for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(mt)]])):
            k, u, t = m[a:b], mu[a:b], mt[a:b]           # one distance: every inflow is final
            ts = np.unique(t)
            share[ts] = (c[ts].astype(np.float64) + inflow[ts]) / cnt[ts].astype(np.float64)
            out.load[k] += share[t]                      # an arc is met once per source
            inner = u != s
            np.add.at(inflow, u[inner], share[t[inner]])
        out.through += inflow
    return out.freeze()


def brute(g, D, sources=None, demand=None, arcs=None):
    """Every feasible path of every pair with demand, in exact fractions, rounded once per word."""
    arcs = arcs or InArcs(g)
    n = arcs.n
    D, sources = _rows(D, sources, n)
    head = np.repeat(np.arange(n), np.diff(arcs.ptr))
    row_of = lr.dense_demand(demand, len(sources), n)
    pos = {(int(u), int(t)): k for k, (u, t) in enumerate(zip(arcs.u, head))}
    load = [Fraction(0)] * len(arcs.u)
    through = [Fraction(0)] * n
    out = Split(arcs)
    for i, s in enumerate(sources):
        s = int(s)
        Dr = D[i]
        Dr[s] = 0
        c = row_of(i)
        m = members(arcs, head, Dr, s)
        M = {}
        for k in np.flatnonzero(m):
            M.setdefault(int(head[k]), []).append(int(arcs.u[k]))
        out.tied_pairs += sum(len(v) >= 2 for v in M.values())
        memo = {s: [([s], Fraction(1))]}

        def paths(t):
            if t not in memo:
                memo[t] = [(p + [t], w / len(M[t])) for u in M[t] for p, w in paths(u)]
            return memo[t]

        for t in range(n):
            x = int(c[t])
            if not x:
                continue
            if t == s:
                out.self_demand += x
            elif t not in M:
                out.unrouted += x
            else:
                out.routed += x
                ps = paths(t)
                assert sum(w for _, w in ps) == 1
                for p, w in ps:
                    for a, b in zip(p, p[1:]):
                        load[pos[(a, b)]] += x * w
                    for v in p[1:-1]:
                        through[v] += x * w
    out.load[:] = [float(x) for x in load]
    out.through[:] = [float(x) for x in through]
    return out.freeze()


def rtol(arcs, n, nsrc):
    """The tolerance of the issue: every word is built from non-negative inputs by f64 additions
    and divisions by positive integers, at most arcs + n + nsrc roundings on a dependency chain;
    twice the two-sided first-order bound."""
    return 4.0 * (arcs + n + nsrc) * 2.0 ** -53


def canonical(g, sources=None, demand=None):
    """load_reference.reference's integers as a Split-like (tail, head, load f64, through f64):
    what the split load equals bitwise where no pair is tied."""
    ref = lr.reference(g, sources, demand)
    tail, head, load, through = ref.arrays()
    return tail, head, load.astype(np.float64), through.astype(np.float64), ref
