"""Graphs for test_gpu_pred_rows_chunk.py: lvl_pred_rows_kernel's units of several 512-source
sub-chunks (levels.hip), each graph with its oracle table computed once (level_graphs.oracle_table).

deep_middle(): n = 1,056 = 33 plane words, sub-chunks of 16, 16 and 1 words. A complete core with
1-3 ms arcs and two braided two-rail tails of 1-ms hops off vertex 0 (level_graphs' tail, twice),
all of whose vertices are numbered 512 .. 512 + 4 * hops - 1, inside the middle sub-chunk. A
source on the core is at most hops + 3 quanta from anything; a source on one tail is up to
2 * hops from the other tail's end. So only sources of the middle sub-chunk have pairs at the deep
levels, and only there are the claimed word, the level bits and the walk's bounds of those levels
in use: state carried over from a neighbouring sub-chunk of the same unit shows there or next door.
"""
import numpy as np

import level_graphs as lg
from shadow_amd import graphs

MS = lg.MS
_cache = {}


def _rails(first, hops):
    """A braided two-rail tail off vertex 0: rails a_i = first + 2i, b_i = a_i + 1."""
    a = first + 2 * np.arange(hops)
    b = a + 1
    src = [np.array([0, 0]), a[:-1], b[:-1], a[:-1], b[:-1]]
    dst = [np.array([a[0], b[0]]), a[1:], b[1:], b[1:], a[1:]]
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)


def deep_middle(n=1056, lo=512, hops=10, seed=41):
    key = ("deep_middle", n, lo, hops, seed)
    if key not in _cache:
        tail = 4 * hops
        assert lo % 512 == 0 and lo + tail <= lo + 512 <= n
        c = graphs.complete_graph(n - tail, seed, lat_max=3)
        ids = np.concatenate([np.arange(lo), np.arange(lo + tail, n)])  # the core's numbering
        s1, d1 = _rails(lo, hops)
        s2, d2 = _rails(lo + 2 * hops, hops)
        ts, td = np.concatenate([s1, s2]), np.concatenate([d1, d2])
        src = np.concatenate([ids[c.src], ts]).astype(np.int32)
        dst = np.concatenate([ids[c.dst], td]).astype(np.int32)
        lat = np.concatenate([c.lat_ns, np.full(len(ts), MS, np.int64)])
        tl = (graphs.hash_u64(seed, 11, ts.astype(np.uint64), td.astype(np.uint64))
              % np.uint64(300)).astype(np.float64) / 10000.0
        g = graphs.Graph(n, False, src, dst, lat, np.concatenate([c.loss, tl]), "deep_middle")
        ecc = lg.row_eccentricity(g)
        inside = np.zeros(n, bool)
        inside[lo:lo + 512] = True
        assert ecc[inside].max() == 2 * hops, ecc[inside].max()
        assert ecc[~inside].max() <= hops + 3 < 2 * hops, ecc[~inside].max()
        _cache[key] = g
    return _cache[key]


def complete(n, seed, lat_max):
    key = ("complete", n, seed, lat_max)
    if key not in _cache:
        _cache[key] = graphs.complete_graph(n, seed=seed, lat_max=lat_max)
    return _cache[key]


def clear():
    _cache.clear()
