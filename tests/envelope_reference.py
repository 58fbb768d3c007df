"""A plain numpy reference for the reliability envelope (envelope.hip), sharing no
code with any kernel.

The rule, over the canonical arcs (route_reference.InArcs) and the oracle's integer distances with
the source's own taken as 0: M(s, t) is the set of tight in-arcs u -> t (D[s][u] + w(u, t) ==
D[s][t]) whose D[s][u] is the smallest among the tight ones -- the predecessors the reference's
Dijkstra can give t, its heap order deciding among them. Then
    hi(s, t) = max over u in M(s, t) of hi(s, u) * r(u, t)
    lo(s, t) = min over u in M(s, t) of lo(s, u) * r(u, t),    hi(s, s) = lo(s, s) = 1.0
with r = 1 - loss of the arc's edge, one f64 multiply each. Unreachable t: 0.0 / 0.0. Every member
of M is strictly nearer than t, so the targets are resolved in increasing distance: all targets of
one distance at once, their members final by then.

Per row the reference also gives, for every target, whether it is tied (|M| >= 2), exposed (tied,
or some member of M exposed) and sensitive (lo != hi bitwise), and its depth: the longest chain of
members from s, which is the sweep of the kernel that resolves it.
"""
import numpy as np

from route_reference import NO_DIST, InArcs


class Envelope:
    """lo, hi f64 [k, n]; tied, exposed, sensitive bool [k, n]; depth int64 [k, n] (0 at s and
    where there is no path); the counts and max_sweeps over all rows."""

    def __init__(self, k, n):
        self.lo = np.zeros((k, n), np.float64)
        self.hi = np.zeros((k, n), np.float64)
        self.tied = np.zeros((k, n), bool)
        self.exposed = np.zeros((k, n), bool)
        self.depth = np.zeros((k, n), np.int64)

    def finish(self):
        self.sensitive = self.lo.view(np.uint64) != self.hi.view(np.uint64)
        self.tied_pairs = int(self.tied.sum())
        self.exposed_pairs = int(self.exposed.sum())
        self.sensitive_pairs = int(self.sensitive.sum())
        self.max_sweeps = int(self.depth.max())
        return self


def members(arcs, head, Drow, s):
    """bool [arcs]: the arcs u -> t in M(s, t), from one distance row (the source's own entry 0)."""
    du, dt = Drow[arcs.u], Drow[head]
    tight = (du < NO_DIST) & (dt < NO_DIST) & (du + arcs.w == dt) & (head != s)
    key = np.where(tight, du, NO_DIST)
    dmin = np.full(arcs.n, NO_DIST, np.int64)
    np.minimum.at(dmin, head, key)
    return tight & (key == dmin[head])


def envelope(g, D, sources=None, arcs=None):
    """The Envelope of `sources` (default: every vertex) from their distance rows D (int64 [k, n],
    the edge list's unit, NO_DIST where unreachable; the source's own entry is treated as 0)."""
    arcs = arcs or InArcs(g)
    n = arcs.n
    sources = np.arange(n) if sources is None else np.asarray(sources)
    D = np.array(D, np.int64)
    assert D.shape == (len(sources), n)
    head = np.repeat(np.arange(n), np.diff(arcs.ptr))
    rel = 1.0 - arcs.loss[arcs.e]
    out = Envelope(len(sources), n)
    for i, s in enumerate(sources):
        Dr = D[i]
        Dr[s] = 0
        m = members(arcs, head, Dr, s)
        mu, mt, mr = arcs.u[m], head[m], rel[m]
        order = np.argsort(Dr[mt], kind="stable")        # increasing distance of the target
        mu, mt, mr = mu[order], mt[order], mr[order]
        cnt = np.bincount(mt, minlength=n)
        reach = Dr < NO_DIST
        reach[s] = False
        assert (cnt[reach] > 0).all() and not cnt[~reach].any(), "D is no distance row of g"
        lo, hi = out.lo[i], out.hi[i]
        lo[reach], hi[reach] = np.inf, -np.inf
        lo[s] = hi[s] = 1.0
        out.tied[i] = cnt >= 2
        exposed, depth = out.exposed[i], out.depth[i]
        exposed[:] = out.tied[i]
        cuts = np.flatnonzero(np.diff(Dr[mt])) + 1
        for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(mt)]])):
            u, t, r = mu[a:b], mt[a:b], mr[a:b]          # one distance: every member is final
            np.minimum.at(lo, t, lo[u] * r)
            np.maximum.at(hi, t, hi[u] * r)
            np.logical_or.at(exposed, t, exposed[u])
            np.maximum.at(depth, t, depth[u] + 1)
    return out.finish()
