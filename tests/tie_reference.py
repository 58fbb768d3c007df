"""A plain numpy count of the tied pairs (srt_build_stats.tied_pairs), independent of every kernel
that counts them: DESIGN §2 and the comment above tie_count_kernel (tables.hip).

Inputs are the oracle's integer distances and the graph's edge list. The canonical arcs are one
arc per ordered pair (u, t), u != t: the minimum latency over parallel edges, both directions of
an undirected edge, self-loops ignored. A pair (s, t), t != s and reachable, is tied when the
smallest D[s][u] over the tight in-arcs u -> t (D[s][u] + w(u, t) == D[s][t], with D[s][s] = 0) is
reached by two or more u. An unreachable pair is never tied. Everything is int64.
"""
import numpy as np

NO_ARC = np.int64(1) << 60  # "no arc" / "unreachable": far above any distance, no overflow in a sum
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def canonical_arcs(n, directed, src, dst, lat):
    """W[u, t] = the smallest latency of an edge u -> t (NO_ARC where there is none), u != t."""
    src = np.asarray(src, np.int64)
    dst = np.asarray(dst, np.int64)
    lat = np.asarray(lat, np.int64)
    W = np.full((n, n), NO_ARC, np.int64)
    off = src != dst
    np.minimum.at(W, (src[off], dst[off]), lat[off])
    if not directed:
        np.minimum.at(W, (dst[off], src[off]), lat[off])
    return W


def distances_of_oracle(lat_int):
    """The oracle's u64 table (UINT64_MAX = unreachable) as int64 distances with D[s][s] = 0."""
    lat_int = np.asarray(lat_int, np.uint64)
    D = np.where(lat_int == U64_MAX, np.uint64(NO_ARC), lat_int).astype(np.int64)
    np.fill_diagonal(D, 0)
    return D


def tied_per_source(n, directed, src, dst, lat, D):
    """int64 [n]: the tied pairs (s, t) of every source s. `lat` and `D` share one unit."""
    W = canonical_arcs(n, directed, src, dst, lat)
    D = np.asarray(D, np.int64)
    assert D.shape == (n, n) and not np.diagonal(D).any()
    out = np.zeros(n, np.int64)
    for t in range(n):  # one vectorised pass per target: every source at once
        us = np.nonzero(W[:, t] < NO_ARC)[0]
        if us.size == 0:
            continue
        du = D[:, us]                                             # [s, u]
        dt = D[:, t]
        tight = (du < NO_ARC) & (du + W[us, t][None, :] == dt[:, None]) & (dt < NO_ARC)[:, None]
        key = np.where(tight, du, NO_ARC)
        best = key.min(axis=1)
        tied = (best < NO_ARC) & ((key == best[:, None]).sum(axis=1) >= 2)
        tied[t] = False
        out += tied
    return out


def tied_pairs(n, directed, src, dst, lat, D, rows=None):
    """The tied pairs over every source, or over the sources [rows[0], rows[1])."""
    per = tied_per_source(n, directed, src, dst, lat, D)
    return int(per.sum() if rows is None else per[rows[0]:rows[1]].sum())
