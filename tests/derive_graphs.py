"""Graphs for the neighbour-row derivation's edge tests (test_gpu_derive_edges.py), each measured
with the CPU oracle and the canonical arc form before it is handed out; test_derive_graphs.py runs
every assertion, and the CPU model of the derivation, without a GPU.

derive.hip forms the rows of an independent set I of vertices of degree 1..4 (build.hip
derive_sets) from their neighbours' rows. Barabasi-Albert graphs with m = 3, the only family the
other tests derive on, give it degree-3 sources, predecessor trees ~8 hops deep and no two adjacent
low-degree vertices. Every graph here leaves that family on one side:

grid(a, b, wmax)     a 4-neighbour lattice: degrees 2, 3 and 4 in I, adjacent low-degree vertices
                     (half of them stay in the core), trees ~90 hops deep, most pairs tied.
ring(n, wmax)        degree 2 everywhere; unit latencies on an even ring: trees n / 2 hops deep and
                     every antipode tied; an odd ring of odd length: no tie at all, and two
                     adjacent core vertices where the greedy pass closes.
ba(m)                Barabasi-Albert with m = 1 (degree-1 sources), 2, 4 (degree 4 only) and 5 (I
                     is empty: no derivation).
pendants(w)          sparse_graphs.heavy_pendants(w): degree-1 sources on direct arcs of the
                     largest compact weight (127) and one past it (128: no derivation).
pendant_losses()     exactly 256 distinct reliabilities, every one on a degree-1 source's direct
                     arc: every table index, 255 included, in the direct-arc code's top field.
islands()            vertex 0 in a BA component; apart from it an isolated vertex, a single edge, a
                     3-vertex path and a 7-ring; parallel edges and self-loops at members of I.

independent_set(g) restates derive_sets; every builder stores g.inI, g.nI and g.deg_hist (the
degree histogram of I). prepare() asserts what the workgroup kernel's compact-arc form needs
(undirected, 1-ms quantum, 2 ecc(0) <= 1022, max_w < 128, <= 256 distinct reliabilities, arcs <
2^20) and that a wrong tie-break always shows: on 60 sampled derived rows no tied target has a
second tight predecessor whose path-order product is bitwise the canonical one's.

model_check() is the CPU model of DESIGN §5.9 (tools/c5_derive_model.py prints it for a BA graph):
distances as neighbour minimums, predecessors as the best of the optimal neighbours' canonical
arcs and the direct arc, against the oracle's Dijkstra rows.
"""
import numpy as np

import oracle
import sparse_graphs as sgr
from level_graphs import MS, U64_MAX, oracle_table, row_eccentricity
from shadow_amd import graphs
from sparse_graphs import _grid, _join, _u, canon

MAXDEG = 4      # build.hip DERIVE_MAXDEG
INF = 1 << 40   # an unreachable pair's distance in the int64 quanta rows used here
SAMPLE = 60     # derived rows sampled for the tie figures

_cache = {}


def independent_set(g):
    """build.hip derive_sets in plain Python: the vertices of canonical degree 1..MAXDEG in stable
    (degree, index) order, each taken unless blocked, then blocking its neighbours -> bool [n]."""
    c = canon(g)
    deg, rp, col = c["deg"], c["rp"], c["col"]
    inI = np.zeros(g.n, bool)
    blocked = np.zeros(g.n, bool)
    for v in np.argsort(deg, kind="stable"):
        if deg[v] > MAXDEG:
            break
        if deg[v] < 1 or blocked[v]:
            continue
        inI[v] = blocked[v] = True
        blocked[col[rp[v]:rp[v + 1]]] = True
    return inI


def oracle_rows(g):
    """Every source's Dijkstra row with its predecessors -> (D int64 [n, n] in quanta with INF for
    an unreachable pair, rel f64, pred i32), computed once per graph object."""
    if getattr(g, "_rows", None) is None:
        el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
        r = oracle.sssp_rows(el, 0, g.n, nthreads=8, want_pred=True)
        q = np.uint64(canon(g)["q"])
        D = np.where(r["lat_int"] == U64_MAX, np.uint64(INF), r["lat_int"] // q).astype(np.int64)
        g._rows = (D, r["rel"], r["pred"])
        for a in g._rows:
            a.setflags(write=False)
    return g._rows


def sampled(g, k=SAMPLE):
    """k members of I, evenly spaced over it, the first and the last among them."""
    I = np.nonzero(g.inI)[0]
    return I if len(I) <= k else I[np.unique(np.linspace(0, len(I) - 1, k).astype(np.int64))]


def tree_depth(g, s):
    """The depth in hops of the oracle's predecessor tree of source s."""
    D, _, P = oracle_rows(g)
    hops = np.zeros(g.n, np.int64)
    for t in np.argsort(D[s], kind="stable"):
        if t != s and D[s, t] < INF:
            hops[t] = hops[P[s, t]] + 1
    return int(hops.max())


def tie_figures(g, rows):
    """Over the given sources: (reachable pairs off the diagonal, tied pairs -- two or more tight
    in-arcs --, tight in-arcs other than the canonical predecessor's whose path-order product
    rel[s][u'] * r(u', t) is bitwise rel[s][t])."""
    c = canon(g)
    D, R, P = oracle_rows(g)
    u = np.repeat(np.arange(g.n), c["deg"])
    t, w, r = c["col"].astype(np.int64), c["w"].astype(np.int64), c["r"]
    pairs = tied = same = 0
    for s in rows:
        tight = (D[s, u] < INF) & (D[s, u] + w == D[s, t]) & (t != s)
        cnt = np.bincount(t[tight], minlength=g.n)
        pairs += int((D[s] < INF).sum()) - 1
        tied += int((cnt >= 2).sum())
        alt = tight & (u != P[s, t])
        same += int(((R[s, u] * r).view(np.uint64) == R[s, t].view(np.uint64))[alt].sum())
    return pairs, tied, same


def model_check(rp, col, w, inI, D, P, rows):
    """The two claims of DESIGN §5.9 for the sources `rows` (members of the independent set inI of
    the canonical CSR rp / col / w), against Dijkstra rows D (int64 quanta, >= INF: unreachable)
    and their predecessors P (every vertex's row: a neighbour's is read):
      D[s][t] = min_k w(s, k) + D[k][t]
      pred(s, t) = the best, by (largest w, smallest u), of the optimal neighbours' canonical arcs
                   into t and of the direct arc when t is a neighbour.
    Unreachable targets are skipped. -> (wrong distances, wrong predecessors)."""
    n = len(rp) - 1
    col = np.asarray(col, np.int64)
    w = np.asarray(w, np.int64)
    key = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp)) * n + col  # ascending: CSR order
    W = int(w.max()) + 1
    tt = np.arange(n, dtype=np.int64)
    bad_d = bad_p = 0
    for s in rows:
        nb, ws = col[rp[s]:rp[s + 1]], w[rp[s]:rp[s + 1]]
        assert inI[s] and not inI[nb].any(), "not independent"
        cand = ws[:, None] + D[nb]  # [deg, n]
        dd = cand.min(axis=0)
        ok = (dd < INF) & (tt != s)
        bad_d += int(((dd != D[s]) & ok).sum()) + int(((D[s] < INF) != (dd < INF))[tt != s].sum())
        best = np.full(n, np.iinfo(np.int64).max)
        for i, k in enumerate(nb):
            u = P[k].astype(np.int64)
            u[k] = s  # the direct arc (s, k)
            have = ok & (cand[i] == dd) & (u >= 0)
            uw = np.zeros(n, np.int64)
            uw[have] = w[np.searchsorted(key, u[have] * n + tt[have])]
            uw[k] = ws[i]
            best = np.where(have, np.minimum(best, (W - uw) * n + u), best)
        bad_p += int(((best % n != P[s]) & ok).sum())
    return bad_d, bad_p


def check_model(g):
    """model_check on every derived row of g (n <= 1,500) or 120 sampled ones."""
    c = canon(g)
    D, _, P = oracle_rows(g)
    rows = np.nonzero(g.inI)[0] if g.n <= 1500 else sampled(g, 120)
    return model_check(c["rp"], c["col"], c["w"], g.inI, D, P, rows) + (len(rows),)


def prepare(g, compact=True):
    """The conditions every graph here meets, asserted, and the figures the tests print: g.inI,
    g.nI, g.deg_hist ({degree: members of I}), g.ties (tie_figures of 60 sampled derived rows).
    compact=False: the one graph whose largest weight is past the compact arcs' 7 bits."""
    c = canon(g)
    assert not g.directed
    assert c["q"] == MS, c["q"]
    ecc0 = int(row_eccentricity(g)[0])
    assert 2 * ecc0 <= 1022, ecc0  # the workgroup kernel's probe passes
    assert (sgr.max_arc_weight(g) < 128) == compact, sgr.max_arc_weight(g)
    assert sgr.distinct_reliabilities(g) <= 256
    assert c["arcs"] < 2 ** 20
    g.inI = independent_set(g)
    g.nI = int(g.inI.sum())
    d, k = np.unique(c["deg"][g.inI], return_counts=True)
    g.deg_hist = dict(zip(d.tolist(), k.tolist()))
    g.ecc0 = ecc0
    # independent, and within the degree cap
    for v in np.nonzero(g.inI)[0]:
        assert not g.inI[c["col"][c["rp"][v]:c["rp"][v + 1]]].any(), v
    assert all(1 <= x <= MAXDEG for x in g.deg_hist)
    g.ties = tie_figures(g, sampled(g))
    assert g.ties[2] == 0, f"{g.name}: {g.ties[2]} tied pairs whose tie-break the reliability hides"
    return g


def describe(g):
    """n, |I|, I's degree histogram and the sampled tie figures, for the tests' printed line."""
    return f"n={g.n} |I|={g.nI} degrees={g.deg_hist} 2ecc(0)={2 * g.ecc0} " \
           f"sampled pairs/tied={g.ties[0]}/{g.ties[1]}"


# -------------------------------------------------------------------------------------------------
def grid(a=40, b=50, wmax=1, seed=73):
    """An a x b lattice (vertex i * b + j; edges to the right and down), latencies U{1..wmax},
    250 hashed losses. Asserted: I holds vertices of degree 2, 3 and 4; more than 1,000 vertices of
    degree <= 4 stay in the core (every vertex is low-degree and half of them are blocked); the
    first derived row's tree is >= 80 hops deep; of the sampled derived rows' reachable pairs,
    >= 90% are tied at wmax = 1 and >= 25% at wmax = 2."""
    key = ("grid", a, b, wmax, seed)
    if key not in _cache:
        v = np.arange(a * b, dtype=np.int64).reshape(a, b)
        s = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
        t = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
        g = prepare(_join([(s, t, _u(seed, 50, s, t, wmax), _grid(seed, 51, s, t, 250))], a * b,
                          False, f"grid{a}x{b}_w{wmax}"))
        deg = canon(g)["deg"]
        assert set(g.deg_hist) == {2, 3, 4}, g.deg_hist
        assert int(((deg <= MAXDEG) & ~g.inI).sum()) > 1000
        g.depth = tree_depth(g, int(np.nonzero(g.inI)[0][0]))
        assert g.depth >= 80, g.depth
        frac = g.ties[1] / g.ties[0]
        assert frac >= {1: 0.90, 2: 0.25}.get(wmax, 0.0), frac
        _cache[key] = g
    return _cache[key]


def ring(n=1000, wmax=1, seed=81):
    """The cycle 0 - 1 - ... - (n - 1) - 0, latencies U{1..wmax}, 250 hashed losses. Asserted:
    every degree is 2. Even n with unit latencies: I is every other vertex, 2 ecc(0) = n, every
    tree is n / 2 hops deep and every source's antipode is tied. Odd n: the greedy pass closes on
    two adjacent core vertices (n - 2 and n - 1), and, the cycle's length being odd (asserted: the
    seed is chosen for it), no pair is tied."""
    key = ("ring", n, wmax, seed)
    if key not in _cache:
        s = np.arange(n, dtype=np.int64)
        t = (s + 1) % n
        g = prepare(_join([(s, t, _u(seed, 52, s, t, wmax), _grid(seed, 53, s, t, 250))], n, False,
                          f"ring{n}_w{wmax}"))
        c = canon(g)
        D = oracle_rows(g)[0]
        assert (c["deg"] == 2).all()
        I = np.nonzero(g.inI)[0]
        if n % 2 == 0:
            assert wmax == 1 and np.array_equal(I, np.arange(0, n, 2))
            assert 2 * g.ecc0 == n
            assert all(tree_depth(g, int(x)) == n // 2 for x in I[::50])
            anti = (s + n // 2) % n
            assert (D[s, anti] == n // 2).all()
            assert (D[s, (anti + 1) % n] == n // 2 - 1).all()
            assert (D[s, (anti - 1) % n] == n // 2 - 1).all()
            assert g.ties[1] == len(sampled(g))  # the antipode, and it alone
        else:
            assert np.array_equal(I, np.arange(0, n - 2, 2))
            assert not g.inI[n - 2] and not g.inI[n - 1]  # adjacent, both in the core
            assert int(c["w"].sum()) // 2 % 2 == 1, "an even cycle length: choose another seed"
            assert tie_figures(g, I)[1] == 0
            g.depth = tree_depth(g, 0)
            assert g.depth >= n // 4
        _cache[key] = g
    return _cache[key]


def ba(m, n=1500, seed=86):
    """graphs.barabasi_albert(n, m, lat_max=4) with 251 hashed losses. Asserted: m = 1: more than
    95% of I has degree 1; m = 2: most of I has degree 2; m = 4: I has degree 4 only; m = 5: I is
    empty (every degree is >= 5)."""
    key = ("ba", m, n, seed)
    if key not in _cache:
        g = prepare(graphs.barabasi_albert(n, m=m, seed=seed, lat_max=4, loss_max=250,
                                           name=f"ba{n}_m{m}"))
        h = g.deg_hist
        if m == 1:
            assert h.get(1, 0) > 0.95 * g.nI, h
        elif m == 2:
            assert h.get(2, 0) > 0.5 * g.nI and 1 not in h, h
        elif m == 4:
            assert set(h) == {4}, h
        elif m == 5:
            assert g.nI == 0 and int(canon(g)["deg"].min()) >= 5
        _cache[key] = g
    return _cache[key]


def pendants(max_w):
    """sparse_graphs.heavy_pendants(max_w) with the derivation's figures. 127: asserted that all
    300 pendants are in I, with degree 1 -- their direct arcs carry the 7-bit field's largest
    weight. 128: the off-case (max_w < 128 fails; no derivation on the GPU)."""
    key = ("pend", max_w)
    if key not in _cache:
        g = prepare(sgr.heavy_pendants(max_w), compact=max_w < 128)
        base = g.n - 300
        assert g.inI[base:].all() and g.deg_hist[1] == 300, g.deg_hist
        _cache[key] = g
    return _cache[key]


def pendant_losses(base=1200, n_pend=300, seed=59):
    """heavy_pendants' base graph (barabasi_albert(1200, seed=59, lat_max=3)) with 300 pendants on
    arcs of 5 quanta. Losses k / 10000, k < 256: hashed on the base's edges and on the pendants'
    arcs, but the first 256 pendants take one value each. Asserted: exactly 256 distinct
    reliabilities among the canonical arcs, every one of them on a pendant's arc, every pendant in
    I with degree 1 -- so each table index, 255 included (the largest reliability), sits in the
    direct-arc code of a derived vertex."""
    key = ("pendloss", base, n_pend, seed)
    if key not in _cache:
        a = graphs.barabasi_albert(base, seed=seed, lat_max=3)
        off = a.src != a.dst
        bs, bd = a.src[off].astype(np.int64), a.dst[off].astype(np.int64)
        pv = np.arange(base, base + n_pend, dtype=np.int64)
        at = (graphs.hash_u64(seed, 54, pv.astype(np.uint64), 0) % np.uint64(base)).astype(np.int64)
        pl = _grid(seed, 55, at, pv, 256)
        pl[:256] = np.arange(256) / 10000.0
        lp = np.nonzero(~off)[0]
        g = prepare(_join([(bs, bd, a.lat_ns[off] // MS, _grid(seed, 56, bs, bd, 256)),
                           (a.src[lp], a.dst[lp], a.lat_ns[lp] // MS, a.loss[lp]),
                           (at, pv, np.full(n_pend, 5, np.int64), pl)],
                          base + n_pend, False, "pendant_losses"))
        c = canon(g)
        assert sgr.distinct_reliabilities(g) == 256
        assert g.inI[base:].all() and (c["deg"][base:] == 1).all()
        pr = c["r"][c["rp"][base:-1]]  # a pendant's only arc
        assert (c["w"][c["rp"][base:-1]] == 5).all()
        every = np.unique(c["r"].view(np.uint64))
        assert np.array_equal(np.unique(pr.view(np.uint64)), every)
        assert float(c["r"].max()) in pr.tolist()  # table index 255
        _cache[key] = g
    return _cache[key]


def islands(head=800, seed=89):
    """Vertices [0, 800): barabasi_albert(800, m=3, lat_max=20), 251 losses, a self-loop on every
    vertex. Disjoint from it: the isolated vertex 800, the single edge 801 - 802, the path
    803 - 804 - 805 and the 7-ring 806..812, self-loops on 801, 803 and 806. 24 members of I in
    the head get a second edge to their first neighbour, alternately 1 ms dearer and 1 ms cheaper
    than the first (the cheaper becomes the canonical arc) with a loss of its own. g.comp: every
    vertex's component. Asserted from the oracle: a pair is reachable exactly when both ends are
    in one component; I holds one end of the single edge, both ends of the path and three ring
    vertices, not the isolated vertex; >= 20 members of I carry a self-loop and >= 20 a parallel
    edge of another latency."""
    key = ("islands", head, seed)
    if key not in _cache:
        a = graphs.barabasi_albert(head, m=3, seed=seed, lat_max=20, loss_max=250)
        ring7 = head + 6 + np.arange(7, dtype=np.int64)
        xs = np.concatenate([[head + 1, head + 3, head + 4], ring7, [head + 1, head + 3, head + 6]])
        xd = np.concatenate([[head + 2, head + 4, head + 5], np.roll(ring7, -1),
                             [head + 1, head + 3, head + 6]])
        n = head + 13
        parts = [(a.src.astype(np.int64), a.dst.astype(np.int64), a.lat_ns // MS, a.loss),
                 (xs, xd, _u(seed, 57, xs, xd, 3), _grid(seed, 58, xs, xd, 250))]
        g0 = _join(parts, n, False, "islands0")
        c0 = canon(g0)
        m0 = np.nonzero(independent_set(g0)[:head])[0][:24]
        nb = c0["col"][c0["rp"][m0]].astype(np.int64)
        w0 = c0["w"][c0["rp"][m0]].astype(np.int64)
        w1 = np.where((np.arange(24) % 2 == 1) & (w0 > 1), w0 - 1, w0 + 1)
        parts.append((nb, m0, w1, _grid(seed, 60, nb, m0, 250)))
        g = prepare(_join(parts, n, False, "islands"))
        c = canon(g)
        assert np.array_equal(g.inI, independent_set(g0))  # parallel edges change no degree
        assert (c["w"][c["rp"][m0]] == np.minimum(w0, w1)).all() and (w1 < w0).sum() >= 8
        comp = np.zeros(n, np.int64)
        comp[head] = 1
        comp[head + 1:head + 3] = 2
        comp[head + 3:head + 6] = 3
        comp[head + 6:] = 4
        d = oracle_table(g)["lat_int"]
        assert np.array_equal(d != U64_MAX, comp[:, None] == comp[None, :])
        inI = g.inI
        assert not inI[head] and int(inI[head + 1:head + 3].sum()) == 1
        assert inI[head + 3] and not inI[head + 4] and inI[head + 5]
        assert int(inI[head + 6:].sum()) == 3
        loops = np.unique(g.src[g.src == g.dst])
        assert int(inI[loops].sum()) >= 20 and len(m0) == 24 and inI[m0].all()
        g.comp, g.head = comp, head
        _cache[key] = g
    return _cache[key]


# every graph of the GPU cases, by the name the tests print
CASES = {
    "grid_w1": lambda: grid(40, 50, 1), "grid_w2": lambda: grid(40, 50, 2),
    "grid_w3": lambda: grid(40, 50, 3), "ring1000": lambda: ring(1000),
    "ring601_w2": lambda: ring(601, 2), "ba_m1": lambda: ba(1), "ba_m2": lambda: ba(2),
    "ba_m4": lambda: ba(4), "pendants127": lambda: pendants(127),
    "pendant_losses": pendant_losses, "islands": islands,
}
OFF_CASES = {"ba_m5": lambda: ba(5), "pendants128": lambda: pendants(128)}
