"""Graphs for the sparse SSSP kernels' edge tests (test_gpu_sparse_edges.py), each measured with
the CPU oracle or with the canonical arc form (graph.c srt_canon_build, which needs no GPU) before
it is handed out; test_sparse_graphs.py runs every assertion without a GPU.

The sparse kernels (wsssp.hip, msssp.hip, sparse.hip, derive.hip) pack values into narrow fields
that seeded random graphs never fill: the workgroup kernel's 10-bit distances (1023 = unreached),
its 15-bit and 12-bit degree fields, the 256 64-arc blocks of a chunk's owner index, the 256-bucket
ring, the compact arcs' 7-bit weight, 20-bit row begin and 256-entry reliability table, and the
multi-source kernel's 16-bit rows. Every graph here sits on one of those edges:

two_part(E, n_losses)   a Barabasi-Albert component holding vertex 0 (the workgroup kernel's probe
                        source, small eccentricity) and, with no edge between them, level_graphs'
                        core + braided tail whose largest distance is exactly E quanta.
fan(...)                vertex 0 - 12 hubs - 3,000 leaves: the hubs settle in one chunk of more
                        than 16,384 arcs, so chunk owners start past the 256th 64-arc block.
star(d, ...)            a hub of degree exactly d over a ring of leaves.
heavy_pendants(w)       pendant vertices on arcs of exactly w quanta, the largest weight.
loss_table(k)           exactly k distinct reliabilities among the canonical arcs.
many_arcs(arcs)         exactly `arcs` canonical arcs on 16,384 vertices.
bound_path(total, dir)  a path whose distance bound (graph.c dist_bound) is exactly `total`.

Losses lie on the k / 10000 grid; latencies are whole milliseconds and every helper asserts that
the quantum comes out as 1 ms.
"""
import ctypes

import numpy as np

import level_graphs as lg
from level_graphs import MS, U64_MAX, oracle_table, row_eccentricity
from shadow_amd import _lib, graphs
from test_canon import Canon

_cache = {}


def canon(g):
    """srt_canon_build of g on the CPU: quantum, largest weight, distance bound, arc count, row
    pointers, arc heads (columns), weights and reliabilities (computed once per graph object)."""
    if getattr(g, "_canon", None) is None:
        L = _lib.lib()
        src = np.ascontiguousarray(g.src, np.int32)
        dst = np.ascontiguousarray(g.dst, np.int32)
        lat = np.ascontiguousarray(g.lat_ns, np.int64)
        loss = np.ascontiguousarray(g.loss, np.float64)
        e = _lib.Edges(g.n, int(bool(g.directed)), len(src), src.ctypes.data, dst.ctypes.data,
                       lat.ctypes.data, loss.ctypes.data)
        c = Canon()
        L.srt_canon_build.restype = ctypes.c_int
        L.srt_canon_build.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        assert L.srt_canon_build(ctypes.byref(e), ctypes.byref(c)) == 0
        rp = np.ctypeslib.as_array(c.rowptr, (g.n + 1,)).copy()
        m = int(rp[-1])
        g._canon = {"q": int(c.quantum_ns), "max_w_q": int(c.max_w_q),
                    "dist_bound": int(c.dist_bound), "wide": int(c.wide), "arcs": int(c.arcs),
                    "rp": rp, "deg": np.diff(rp),
                    "col": np.ctypeslib.as_array(c.col, (max(m, 1),))[:m].copy(),
                    "w":np.ctypeslib.as_array(c.w, (max(m, 1),))[:m].copy(),
                    "r": np.ctypeslib.as_array(c.r, (max(m, 1),))[:m].copy()}
        L.srt_canon_free.argtypes = [ctypes.c_void_p]
        L.srt_canon_free(ctypes.byref(c))
        assert g._canon["arcs"] == m
    return g._canon


def distinct_reliabilities(g):
    """The number of bitwise-distinct reliabilities among the canonical arcs (self-loops apart)."""
    return len(np.unique(canon(g)["r"].view(np.uint64)))


def max_arc_weight(g):
    """The largest canonical arc weight in quanta (self-loops apart): the kernels' max_w."""
    return int(canon(g)["w"].max())


def _grid(seed, stream, a, b, k):
    """k-value loss grid, hashed per (a, b)."""
    return (graphs.hash_u64(seed, stream, np.asarray(a, np.uint64), np.asarray(b, np.uint64))
            % np.uint64(k)).astype(np.float64) / 10000.0


def _u(seed, stream, a, b, k):
    """U{1..k}, hashed per (a, b)."""
    return 1 + (graphs.hash_u64(seed, stream, np.asarray(a, np.uint64), np.asarray(b, np.uint64))
                % np.uint64(k)).astype(np.int64)


def _join(parts, n, directed, name):
    src, dst, lat_ms, loss = (np.concatenate([p[i] for p in parts]) for i in range(4))
    return graphs.Graph(n, directed, src.astype(np.int32), dst.astype(np.int32),
                        lat_ms.astype(np.int64) * MS, loss.astype(np.float64), name)


# -------------------------------------------------------------------------------------------------
HEAD = 300  # two_part: the probe's component


def _build_two_part(hops, n_losses, seed):
    a = graphs.barabasi_albert(HEAD, seed=41, lat_max=20)
    b = lg._build_core_tail(40, hops, seed, False, False, MS)
    src = np.concatenate([a.src, b.src + HEAD])
    dst = np.concatenate([a.dst, b.dst + HEAD])
    loss = _grid(seed, 21, src, dst, n_losses)
    return graphs.Graph(a.n + b.n, False, src.astype(np.int32), dst.astype(np.int32),
                        np.concatenate([a.lat_ns, b.lat_ns]), loss,
                        f"two_part_h{hops}_l{n_losses}")


def two_part(target, n_losses=200, seed=43):
    """Vertices [0, 300): barabasi_albert(300, seed=41, lat_max=20). After them, with no edge
    between the two, level_graphs' core (40) + braided tail whose largest distance is exactly
    `target` quanta. g.ecc: the oracle's row eccentricities; g.head: 300. Asserted: the target,
    that no pair across the components is reachable and every pair inside one is, the quantum,
    2 ecc(0) <= 1022 (the workgroup kernel's probe passes) and which side of 256 the number of
    distinct reliabilities falls (<= 256: compact arcs; > 256: 16-byte arcs)."""
    key = ("two", target, n_losses, seed)
    if key not in _cache:
        g0 = _build_two_part(0, n_losses, seed)
        d0 = oracle_table(g0)["lat_int"][HEAD:, HEAD:] // np.uint64(MS)
        reach = int(max(d0[1:, 0].max(), d0[0, 1:].max()))  # the core's farthest from its vertex 0
        hops = target - reach
        assert hops >= 1, (target, reach)
        g = _build_two_part(hops, n_losses, seed)
        d = oracle_table(g)["lat_int"]
        assert (d[:HEAD, HEAD:] == U64_MAX).all() and (d[HEAD:, :HEAD] == U64_MAX).all()
        assert (d[:HEAD, :HEAD] != U64_MAX).all() and (d[HEAD:, HEAD:] != U64_MAX).all()
        ecc = row_eccentricity(g)
        assert canon(g)["q"] == MS
        assert int(ecc[HEAD:].max()) == target, \
            f"two_part({target}): the oracle measures E = {int(ecc[HEAD:].max())} (hops {hops})"
        assert 2 * int(ecc[0]) <= 1022 and int(ecc[:HEAD].max()) < 1022 - 20, int(ecc[0])
        assert max_arc_weight(g) == 20
        k = distinct_reliabilities(g)
        assert (k <= 256) == (n_losses <= 256) and k <= n_losses, (k, n_losses)
        g.ecc, g.head = ecc, HEAD
        _cache[key] = g
    return _cache[key]


# -------------------------------------------------------------------------------------------------
def fan(hubs=12, leaves=3000, p=0.6, wmax=20, n_losses=200, seed=47):
    """Vertex 0 joined to hubs 1..hubs by 1-ms arcs; every hub-leaf edge present with probability
    p (hashed), latency U{1..wmax}, a loss of its own; self-loops on every third vertex. The
    vertices at distance exactly 1 from vertex 0 settle in one chunk of the workgroup kernel;
    asserted: their degrees sum to more than 16,384 (the 256 indexed 64-arc blocks) plus the largest
    of them, so at least one chunk entry's arcs start past the indexed blocks. Leaves hang on
    several hubs at different distances and losses: a mis-assigned arc owner changes a distance or
    a predecessor."""
    key = ("fan", hubs, leaves, p, wmax, n_losses, seed)
    if key not in _cache:
        n = 1 + hubs + leaves
        h = np.arange(1, hubs + 1, dtype=np.int64)
        hh = np.repeat(h, leaves)
        ll = np.tile(np.arange(hubs + 1, n, dtype=np.int64), hubs)
        keep = (graphs.hash_u64(seed, 22, hh.astype(np.uint64), ll.astype(np.uint64))
                % np.uint64(10000)).astype(np.int64) < int(p * 10000)
        hh, ll = hh[keep], ll[keep]
        loops = np.arange(0, n, 3, dtype=np.int64)
        g = _join([(np.zeros(hubs, np.int64), h, np.ones(hubs, np.int64),
                    _grid(seed, 23, np.zeros(hubs), h, n_losses)),
                   (hh, ll, _u(seed, 24, hh, ll, wmax), _grid(seed, 23, hh, ll, n_losses)),
                   (loops, loops, 1 + loops % 7, _grid(seed, 25, loops, loops, n_losses))],
                  n, False, f"fan{hubs}x{leaves}_l{n_losses}")
        c = canon(g)
        assert c["q"] == MS and max_arc_weight(g) == wmax
        d = oracle_table(g)["lat_int"][0] // np.uint64(MS)
        first = np.nonzero(d == 1)[0]
        first = first[first != 0]
        assert set(first.tolist()) == set(h.tolist()), first
        deg = c["deg"][first]
        assert int(deg.sum()) > 16384 + int(deg.max()), (int(deg.sum()), int(deg.max()))
        assert int(deg.max()) < 4095  # neither degree clamp: star() has those
        k = distinct_reliabilities(g)
        assert (k <= 256) == (n_losses <= 256), (k, n_losses)
        # a leaf on several hubs at different distances from vertex 0
        multi = np.bincount(ll, minlength=n)
        assert int((multi >= 2).sum()) > leaves // 2
        g.first = first
        _cache[key] = g
    return _cache[key]


# -------------------------------------------------------------------------------------------------
def star(hub_degree, n_losses=200, wmax=20, seed=53):
    """Vertex 0 joined to every other vertex (n = hub_degree + 1, latencies U{1..wmax}); the
    leaves 1..n-1 also form a ring (U{1..wmax}), so leaf-leaf routes compete with the hub;
    self-loops on every fifth vertex. Asserted on the canonical arcs: the hub's degree is exactly
    hub_degree, every leaf's is 3."""
    key = ("star", hub_degree, n_losses, wmax, seed)
    if key not in _cache:
        assert hub_degree >= 4
        n = hub_degree + 1
        leaf = np.arange(1, n, dtype=np.int64)
        nxt = np.where(leaf + 1 < n, leaf + 1, 1)
        loops = np.arange(0, n, 5, dtype=np.int64)
        g = _join([(np.zeros(hub_degree, np.int64), leaf, _u(seed, 26, 0 * leaf, leaf, wmax),
                    _grid(seed, 27, 0 * leaf, leaf, n_losses)),
                   (leaf, nxt, _u(seed, 28, leaf, nxt, wmax), _grid(seed, 29, leaf, nxt, n_losses)),
                   (loops, loops, 1 + loops % 7, _grid(seed, 30, loops, loops, n_losses))],
                  n, False, f"star{hub_degree}_l{n_losses}")
        c = canon(g)
        assert c["q"] == MS and max_arc_weight(g) <= wmax
        assert int(c["deg"][0]) == hub_degree and (c["deg"][1:] == 3).all()
        assert c["arcs"] == 4 * hub_degree
        k = distinct_reliabilities(g)
        assert (k <= 256) == (n_losses <= 256), (k, n_losses)
        _cache[key] = g
    return _cache[key]


# -------------------------------------------------------------------------------------------------
def heavy_pendants(max_w, base=1200, pendants=300, seed=59):
    """barabasi_albert(base, lat_max=3) plus `pendants` vertices, each hanging by one arc of exactly
    max_w quanta: the heavy arcs are tight (a pendant's only way in) and the bucket ring wraps at
    every pendant. Asserted: the quantum, max_w_q == max_w == the largest arc weight, and
    2 ecc(0) <= 1022 (the workgroup kernel's probe passes)."""
    key = ("pend", max_w, base, pendants, seed)
    if key not in _cache:
        a = graphs.barabasi_albert(base, seed=seed, lat_max=3)
        pv = np.arange(base, base + pendants, dtype=np.int64)
        at = (graphs.hash_u64(seed, 31, pv.astype(np.uint64), 0) % np.uint64(base)).astype(np.int64)
        g = _join([(a.src, a.dst, a.lat_ns // MS, a.loss),
                   (at, pv, np.full(pendants, max_w, np.int64), _grid(seed, 32, at, pv, 101))],
                  base + pendants, False, f"pendants_w{max_w}")
        c = canon(g)
        assert c["q"] == MS and c["max_w_q"] == max_w == max_arc_weight(g)
        assert (c["deg"][base:] == 1).all()
        ecc = row_eccentricity(g)
        assert 2 * int(ecc[0]) <= 1022, int(ecc[0])
        assert int(ecc.max()) <= 1022  # every row fits the 10-bit field
        assert (oracle_table(g)["lat_int"] != U64_MAX).all()
        assert distinct_reliabilities(g) <= 256
        _cache[key] = g
    return _cache[key]


# -------------------------------------------------------------------------------------------------
def loss_table(k, n=2000, seed=61):
    """barabasi_albert(n, lat_max=20) with the off-diagonal losses reassigned to exactly k values
    of the grid (the first k edges take one each, the rest are hashed). Asserted on
    srt_canon_build's r: exactly k distinct reliabilities."""
    key = ("loss", k, n, seed)
    if key not in _cache:
        a = graphs.barabasi_albert(n, seed=seed, lat_max=20)
        off = np.nonzero(a.src != a.dst)[0]
        assert len(off) >= k
        idx = (graphs.hash_u64(seed, 33, a.src[off].astype(np.uint64), a.dst[off].astype(np.uint64))
               % np.uint64(k)).astype(np.int64)
        idx[:k] = np.arange(k)
        loss = a.loss.copy()
        loss[off] = idx / 10000.0
        g = graphs.Graph(n, False, a.src, a.dst, a.lat_ns, loss, f"loss_table{k}")
        assert canon(g)["q"] == MS and max_arc_weight(g) <= 20
        assert distinct_reliabilities(g) == k
        assert canon(g)["arcs"] == 2 * len(off)  # no parallel edges: every edge is canonical
        _cache[key] = g
    return _cache[key]


# -------------------------------------------------------------------------------------------------
def many_arcs(arcs, n=16384, seed=67):
    """n vertices, arcs / 2 distinct undirected non-loop edges (a ring, so the graph is connected,
    and hashed pairs), latencies U{1..20}, 200 losses. Asserted: the canonical arc count == arcs
    (the compact arcs keep a row's begin in 20 bits: arcs < 2^20)."""
    key = ("arcs", arcs, n, seed)
    if key not in _cache:
        assert arcs % 2 == 0 and arcs // 2 >= n
        need = arcs // 2 - n
        ring = np.arange(n, dtype=np.int64)
        ring_key = np.minimum(ring, (ring + 1) % n) * n + np.maximum(ring, (ring + 1) % n)
        i = np.arange(int(need * 1.2) + 1024, dtype=np.uint64)
        u = (graphs.hash_u64(seed, 34, i, 0) % np.uint64(n)).astype(np.int64)
        v = (graphs.hash_u64(seed, 35, i, 0) % np.uint64(n)).astype(np.int64)
        keys = np.unique((np.minimum(u, v) * n + np.maximum(u, v))[u != v])
        keys = np.setdiff1d(keys, ring_key)
        assert len(keys) >= need, (len(keys), need)
        order = np.argsort(graphs.hash_u64(seed, 36, keys.astype(np.uint64), 0), kind="stable")
        keys = np.sort(keys[order[:need]])
        s = np.concatenate([ring, keys // n])
        t = np.concatenate([(ring + 1) % n, keys % n])
        g = _join([(s, t, _u(seed, 37, s, t, 20), _grid(seed, 38, s, t, 200))], n, False,
                  f"many_arcs{arcs}")
        c = canon(g)
        assert c["q"] == MS and c["arcs"] == arcs, c["arcs"]
        assert max_arc_weight(g) == 20 and int(c["deg"].max()) < 4095
        assert distinct_reliabilities(g) <= 256
        _cache[key] = g
    return _cache[key]


# -------------------------------------------------------------------------------------------------
def bound_path(total, directed=False, seed=71):
    """Undirected: a path 0 - 1 - ... whose hop weights lie in 1..255 and sum to exactly `total`
    quanta; its MST weight is its end-to-end distance, so graph.c's dist_bound and the largest real
    distance both equal `total` (asserted, the first on srt_canon_build, the second on the oracle).
    Directed: `total` must be h * 151: a bidirected path of h hops of 151 quanta and one 1-ms
    self-loop (the quantum stays 1 ms); dist_bound = (n - 1) * max_w = h * 151 = the largest real
    distance."""
    key = ("path", total, directed, seed)
    if key not in _cache:
        if directed:
            assert total % 151 == 0
            h = total // 151
            w = np.full(h, 151, np.int64)
        else:
            w, left, i = [], total, 0
            while left > 255:
                x = 128 + int(graphs.hash_u64(seed, 39, i, 0)) % 128  # 128..255
                w.append(x)
                left -= x
                i += 1
            w.append(left)
            w = np.array(w, np.int64)
            h = len(w)
            assert w.min() >= 1 and w.max() <= 255 and int(w.sum()) == total
        a = np.arange(h, dtype=np.int64)
        parts = [(a, a + 1, w, _grid(seed, 40, a, a + 1, 200))]
        if directed:
            parts += [(a + 1, a, w, _grid(seed, 41, a + 1, a, 200)),
                      (np.array([h // 2]), np.array([h // 2]), np.array([1]), np.array([0.0007]))]
        else:  # two self-loops: the diagonal rule with and without one
            lp = np.array([0, h // 2], np.int64)
            parts += [(lp, lp, np.array([2, 3]), np.array([0.0003, 0.0011]))]
        g = _join(parts, h + 1, directed, f"bound_path{total}{'_dir' if directed else ''}")
        c = canon(g)
        assert c["q"] == MS, c["q"]
        assert c["dist_bound"] == total, (c["dist_bound"], total)
        assert c["wide"] == 0
        assert lg.largest_distance(g) == total
        assert (oracle_table(g)["lat_int"] != U64_MAX).all()
        _cache[key] = g
    return _cache[key]
