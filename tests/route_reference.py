"""A plain numpy reference for the route export (routes.hip), sharing no code with
any kernel.

The rule: over the canonical arcs (one arc per ordered pair (u, t), u != t: the minimum latency
over parallel edges, then the lowest edge index; both directions of an undirected edge; self-loops
ignored), pred(s, t) = argmin (D[s][u], u) among the tight in-arcs u -> t, D[s][u] + w(u, t) ==
D[s][t], with the source's own distance taken as 0. pred is -1 for t == s and for unreachable t.
Distances are the oracle's integers; everything is int64.
"""
import numpy as np

NO_DIST = np.int64(1) << 60  # unreachable: far above any distance, no overflow in a sum
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


class InArcs:
    """In-arc CSR of the canonical arcs: for target t, arcs ptr[t]:ptr[t+1] give the tails `u`
    (ascending), their latencies `w` (the edge list's unit) and the edge index `e` they come from."""

    def __init__(self, g):
        src = np.asarray(g.src, np.int64)
        dst = np.asarray(g.dst, np.int64)
        lat = np.asarray(g.lat_ns, np.int64)
        idx = np.arange(len(src), dtype=np.int64)
        off = src != dst
        u, t, w, e = src[off], dst[off], lat[off], idx[off]
        if not g.directed:
            u, t, w, e = (np.concatenate([u, t]), np.concatenate([t, u]), np.concatenate([w, w]),
                          np.concatenate([e, e]))
        order = np.lexsort((e, w, u, t))  # by target, tail, latency, edge index
        u, t, w, e = u[order], t[order], w[order], e[order]
        keep = np.ones(len(u), bool)
        keep[1:] = (t[1:] != t[:-1]) | (u[1:] != u[:-1])
        self.n = int(g.n)
        self.u, self.w, self.e = u[keep], w[keep], e[keep]
        self.ptr = np.searchsorted(t[keep], np.arange(self.n + 1), side="left")
        self.loss = np.asarray(g.loss, np.float64)

    def arc(self, u, t):
        """(latency, edge index) of the canonical arc u -> t."""
        a, b = self.ptr[t], self.ptr[t + 1]
        k = a + int(np.searchsorted(self.u[a:b], u))
        assert k < b and self.u[k] == u, f"no arc {u} -> {t}"
        return int(self.w[k]), int(self.e[k])


def distances_of_oracle(lat_int, sources):
    """The oracle's u64 rows (UINT64_MAX = unreachable; row i belongs to sources[i]) as int64 with
    the source's own entry 0 (the oracle's diagonal holds the path-to-self rule)."""
    lat_int = np.asarray(lat_int, np.uint64)
    D = np.where(lat_int == U64_MAX, np.uint64(NO_DIST), lat_int).astype(np.int64)
    D[np.arange(len(sources)), np.asarray(sources)] = 0
    return D


def pred_from_distances(g, D, sources=None, arcs=None):
    """int32 [k, n]: the canonical predecessor rows of `sources` (default: every vertex) from their
    distance rows D (int64, the edge list's unit, the source's own entry treated as 0)."""
    arcs = arcs or InArcs(g)
    n = arcs.n
    sources = np.arange(n) if sources is None else np.asarray(sources)
    D = np.array(D, np.int64)
    assert D.shape == (len(sources), n)
    D[np.arange(len(sources)), sources] = 0
    pred = np.full(D.shape, -1, np.int32)
    for t in range(n):
        a, b = arcs.ptr[t], arcs.ptr[t + 1]
        if a == b:
            continue
        us = arcs.u[a:b]
        du = D[:, us]                                                   # [source, arc]
        dt = D[:, t]
        tight = (du < NO_DIST) & (dt < NO_DIST)[:, None] & (du + arcs.w[a:b][None, :] == dt[:, None])
        key = np.where(tight, du, NO_DIST)
        best = key.min(axis=1)
        cand = np.where(tight & (key == best[:, None]), us[None, :], n)  # the lowest u among the nearest
        p = cand.min(axis=1)
        pred[:, t] = np.where(best < NO_DIST, p, -1)
    pred[np.arange(len(sources)), sources] = -1
    return pred


def walk(pred_row, s):
    """(hops, first) int32 [n] of one predecessor row: the edges on the path (0 at s, -1 where
    there is none) and the first vertex after s (t itself when pred == s, -1 where pred is -1)."""
    pred_row = np.asarray(pred_row, np.int64)
    n = len(pred_row)
    hops = np.full(n, -1, np.int32)
    first = np.full(n, -1, np.int32)
    hops[s] = 0
    has = pred_row >= 0
    safe = np.where(has, pred_row, 0)
    ts = np.arange(n)
    while True:
        ready = has & (hops < 0) & (hops[safe] >= 0)
        if not ready.any():
            return hops, first
        hops[ready] = hops[safe[ready]] + 1
        first[ready] = np.where(safe[ready] == s, ts[ready], first[safe[ready]])


def rel_along(g, pred_row, s, arcs=None):
    """f64 [n]: the product of (1 - loss) over the canonical arcs of each route, multiplied left
    to right from s (1.0 at s, 0.0 where there is no route) -- the order of topology.c:1364-1365."""
    arcs = arcs or InArcs(g)
    hops, _ = walk(pred_row, s)
    rel = np.zeros(arcs.n, np.float64)
    rel[s] = 1.0
    for t in np.argsort(hops, kind="stable"):
        if hops[t] <= 0:
            continue
        p = int(pred_row[t])
        _, e = arcs.arc(p, int(t))
        rel[t] = rel[p] * (1.0 - arcs.loss[e])
    return rel


def chain(pred_row, s, t):
    """The vertices of the route s -> t (s first), or None when there is none."""
    if s == t:
        return [s]
    if pred_row[t] < 0:
        return None
    out = [t]
    while out[-1] != s:
        out.append(int(pred_row[out[-1]]))
        assert len(out) <= len(pred_row)
    return out[::-1]
