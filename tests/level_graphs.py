"""Graphs for the level build's edge tests (test_gpu_level_edges.py, test_gpu_level_unreached.py,
test_gpu_ties.py), each with its oracle table computed once on the CPU and cached.

core_tail(E): a graph whose largest off-diagonal distance is exactly E quanta. The core is a small
complete graph with 1-3 ms arcs and self-loops (many equal-length paths); a braided two-rail tail
of 1-ms hops hangs off vertex 0: rails a_1..a_L and b_1..b_L after the core, in the order a_1, b_1,
a_2, b_2, ..., with the edges 0-a_1, 0-b_1, a_i-a_(i+1), b_i-b_(i+1), a_i-b_(i+1), b_i-a_(i+1).
Both a_i and b_i precede a_(i+1) at the same distance from every source on the core's side, so
every such pair is tied and its reliability depends on the canonical predecessor at every level.
Row eccentricities run from about E/2 (the middle of the tail) to E (the core and the tail's end).
The tail's length sets E; the helper measures E with the oracle and asserts it -- no test rests
on an assumed E.
"""
import ctypes

import numpy as np

import oracle
from shadow_amd import _lib, graphs

MS = 1_000_000
REL_TOL = 1e-12
LEVELS = 12  # srt_build_stats.dist_enc of a level build
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)

_cache = {}


def oracle_table(g):
    """The oracle's raw table of g (every source's own row), computed once per graph object."""
    if getattr(g, "_exp", None) is None:
        el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
        g._exp = oracle.table(el, True, oracle.ORC_INT_NS, 8, raw=True)
        for a in g._exp.values():
            a.setflags(write=False)
    return g._exp


def quantum(g):
    return int(np.gcd.reduce(g.lat_ns[g.lat_ns > 0]))


def largest_distance(g):
    """The largest finite off-diagonal distance of g in quanta, from the oracle."""
    d = oracle_table(g)["lat_int"]
    off = ~np.eye(g.n, dtype=bool) & (d != U64_MAX)
    return int(d[off].max()) // quantum(g)


def row_eccentricity(g):
    """int64 [n]: every source's largest finite off-diagonal distance in quanta."""
    d = oracle_table(g)["lat_int"].copy()
    d[d == U64_MAX] = 0
    np.fill_diagonal(d, 0)
    return (d.max(axis=1) // np.uint64(quantum(g))).astype(np.int64)


def unreached_as_oracle(lat_ns, g):
    """The tables mark an unreachable pair SRT_INF quanta; the oracle marks it UINT64_MAX ns."""
    return np.where(lat_ns == np.uint64(_lib.SRT_INF * quantum(g)), U64_MAX, lat_ns)


def check_tables(g, lat, rel, what, reachable_only=False):
    """The whole table, diagonal included: latency bit-exact (unreachable pairs as the oracle
    marks them), reliability within 1e-12 relative -- on the reachable pairs alone when asked."""
    exp = oracle_table(g)
    bad = np.argwhere(unreached_as_oracle(lat, g) != exp["lat_int"])
    assert bad.size == 0, f"{what}: {len(bad)} latency mismatches, first {bad[:5].tolist()}"
    err = np.abs(rel - exp["rel"]) / np.maximum(np.abs(exp["rel"]), 1e-300)
    if reachable_only:
        err = np.where(exp["lat_int"] == U64_MAX, 0.0, err)
    assert float(err.max()) <= REL_TOL, \
        f"{what}: max rel error {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"


def _tail_edges(core, hops):
    """The braided two-rail tail of `hops` rungs off vertex 0 (vertex ids from `core` on)."""
    a = core + 2 * np.arange(hops)
    b = a + 1
    if hops == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    src = [np.array([0, 0]), a[:-1], b[:-1], a[:-1], b[:-1]]
    dst = [np.array([a[0], b[0]]), a[1:], b[1:], b[1:], a[1:]]
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)


def _build_core_tail(core, hops, seed, directed, many_losses, quantum_ns):
    c = graphs.complete_directed(core, seed, lat_max=3) if directed else \
        graphs.complete_graph(core, seed, lat_max=3)
    ts, td = _tail_edges(core, hops)
    if directed:  # both orientations as separate arcs (independent losses below)
        ts, td = np.concatenate([ts, td]), np.concatenate([td, ts])
    n = core + 2 * hops
    # self-loops on rail a only: the diagonal rule with and without one
    loops = core + 2 * np.arange(hops, dtype=np.int64)
    src = np.concatenate([c.src, ts, loops]).astype(np.int32)
    dst = np.concatenate([c.dst, td, loops]).astype(np.int32)
    lat_ms = np.concatenate([c.lat_ns // MS, np.ones(len(ts), np.int64),
                             1 + (loops % 7)]).astype(np.int64)
    if many_losses:  # more distinct values than the level build's table holds (2,048): f64 rows
        loss = np.random.default_rng(seed).random(len(src)) * 0.05
        assert len(np.unique(loss)) > 2048
    else:            # a small grid: 300 distinct values, the packed form applies
        loss = (graphs.hash_u64(seed, 11, src.astype(np.uint64), dst.astype(np.uint64))
                % np.uint64(300)).astype(np.float64) / 10000.0
    return graphs.Graph(n, directed, src, dst, lat_ms * quantum_ns, loss,
                        f"core{core}_tail{hops}{'_dir' if directed else ''}")


def core_tail(target, core=200, seed=23, directed=False, many_losses=False, quantum_ns=MS):
    """The core + tail graph whose largest off-diagonal distance is exactly `target` quanta
    (target >= 2), asserted against the oracle before it is handed out."""
    key = (target, core, seed, directed, many_losses, quantum_ns)
    if key not in _cache:
        g0 = _build_core_tail(core, 0, seed, directed, many_losses, quantum_ns)
        d0 = oracle_table(g0)["lat_int"] // np.uint64(quantum_ns)
        # the farthest core vertex from the tail's end: over vertex 0, both ways round
        reach = int(max(d0[1:, 0].max(), d0[0, 1:].max()))
        hops = max(0, target - reach)
        g = _build_core_tail(core, hops, seed, directed, many_losses, quantum_ns) if hops else g0
        e = largest_distance(g)
        assert e == target, f"core_tail({target}): the oracle measures E = {e} (hops {hops})"
        _cache[key] = g
    return _cache[key]


def all_ones(n=160, seed=29):
    """E = 1: a complete graph whose arcs are all 1 ms (every pair settled by its own arc)."""
    key = ("ones", n, seed)
    if key not in _cache:
        c = graphs.complete_graph(n, seed, lat_max=1)
        loss = (graphs.hash_u64(seed, 11, c.src.astype(np.uint64), c.dst.astype(np.uint64))
                % np.uint64(300)).astype(np.float64) / 10000.0
        g = graphs.Graph(c.n, False, c.src, c.dst, c.lat_ns, loss, "ones")
        assert largest_distance(g) == 1
        _cache[key] = g
    return _cache[key]


def two_complete(na=150, nb=170, seed=31):
    """Two disjoint complete graphs (1-4 ms arcs, undirected): every pair across is unreachable."""
    key = ("two", na, nb, seed)
    if key not in _cache:
        a = graphs.complete_graph(na, seed, lat_max=4)
        b = graphs.complete_graph(nb, seed + 1, lat_max=4)
        g = graphs.Graph(na + nb, False, np.concatenate([a.src, b.src + na]).astype(np.int32),
                         np.concatenate([a.dst, b.dst + na]).astype(np.int32),
                         np.concatenate([a.lat_ns, b.lat_ns]), np.concatenate([a.loss, b.loss]),
                         "two_complete")
        d = oracle_table(g)["lat_int"]
        assert (d[:na, na:] == U64_MAX).all() and (d[na:, :na] == U64_MAX).all()
        assert (d[:na, :na] != U64_MAX).all() and (d[na:, na:] != U64_MAX).all()
        _cache[key] = g
    return _cache[key]


def closed_block(n=320, block=40, seed=37, p=0.5, wmax=4):
    """A directed dense graph whose first `block` vertices have no in-arcs from the rest: the
    block's sources reach everything, every other source reaches no vertex of the block."""
    key = ("block", n, block, seed, p, wmax)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        i, j = np.nonzero(rng.random((n, n)) < p)
        keep = (i != j) & ~((i >= block) & (j < block))
        i, j = i[keep], j[keep]
        ring_b = np.arange(block)          # the block and the rest each strongly connected,
        ring_r = np.arange(block, n)       # one arc from the block into the rest
        src = np.concatenate([i, ring_b, ring_r, [0], np.arange(n)]).astype(np.int32)
        dst = np.concatenate([j, np.roll(ring_b, -1), np.roll(ring_r, -1), [block],
                              np.arange(n)]).astype(np.int32)
        lat = (rng.integers(1, wmax + 1, len(src)) * MS).astype(np.int64)
        loss = rng.integers(0, 300, len(src)) / 10000.0
        g = graphs.Graph(n, True, src, dst, lat, loss, f"closed_block{block}")
        d = oracle_table(g)["lat_int"]
        assert (d[:block] != U64_MAX).all() and (d[block:, block:] != U64_MAX).all()
        assert (d[block:, :block] == U64_MAX).all()
        _cache[key] = g
    return _cache[key]


def build(g, algo=_lib.ALGO_DENSE_FW, ngpus=None, count_ties=0):
    """srt_build_tables / srt_build_tables_multi with srt_build_stats.count_ties as given (the
    wrapper of shadow_amd.topology leaves it 0) -> (lat_ns u64, rel f64, stats)."""
    src = np.ascontiguousarray(g.src, np.int32)
    dst = np.ascontiguousarray(g.dst, np.int32)
    lat_ns = np.ascontiguousarray(g.lat_ns, np.int64)
    loss = np.ascontiguousarray(g.loss, np.float64)
    e = _lib.Edges(g.n, int(bool(g.directed)), len(src), src.ctypes.data, dst.ctypes.data,
                   lat_ns.ctypes.data, loss.ctypes.data)
    o = _lib.BuildOpts(0, algo, 1, 0)
    lat = np.empty((g.n, g.n), np.uint32)
    rel = np.empty((g.n, g.n), np.float64)
    q = ctypes.c_uint64()
    st = _lib.BuildStats()
    st.count_ties = count_ties
    L = _lib.lib()
    if ngpus is None:
        _lib.check(L.srt_build_tables(ctypes.byref(e), ctypes.byref(o), lat.ctypes.data,
                                      ctypes.byref(q), rel.ctypes.data, ctypes.byref(st)),
                   "srt_build_tables")
    else:
        _lib.check(L.srt_build_tables_multi(ctypes.byref(e), ctypes.byref(o), int(ngpus),
                                            lat.ctypes.data, ctypes.byref(q), rel.ctypes.data,
                                            ctypes.byref(st)), "srt_build_tables_multi")
    return lat.astype(np.uint64) * np.uint64(q.value), rel, st


def shard_rows(n, ranks):
    """The row blocks [begin, end) of a build over `ranks` ranks (srt_shard_rows on the padded
    edge srt_build_tables_multi uses), clipped to n."""
    L = _lib.lib()
    ld = (n + 127) // 128 * 128
    out = []
    for r in range(ranks):
        b, e = ctypes.c_int32(), ctypes.c_int32()
        L.srt_shard_rows(ld, 128, ranks, r, ctypes.byref(b), ctypes.byref(e))
        out.append((min(b.value, n), min(e.value, n)))
    return out
