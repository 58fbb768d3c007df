"""Graphs for the dense builds' reliability chain (test_gpu_rel_forms.py), each classified with the
CPU oracle before it is handed out (test_rel_graphs.py runs every assertion without a GPU).

Which kernel of shadow_amd/csrc/dense.hip finishes a row's rel(s,t) = rel(s,pred) * r(pred,t)
depends on the row's distance range (its largest finite off-diagonal distance in quanta), on the
number of its parents (targets other than s that are some reachable target's predecessor) and on
a size class of n. The graphs here are trees: every predecessor is unique, so the parent counts
do not depend on the tie rule, and they can be set to the unit.

spider(chains, length, extra, ecc0): vertex 0 with `chains` paths of `length` vertices each and
`extra` paths of two. Row 0 has chains * (length - 1) + extra parents (the inner vertices) and
the range ecc0; every inner vertex's row has as many (vertex 0 for itself) and a wider range;
every path end's row has one more. So one spider whose row 0 sits on a parent cap holds rows
with cap and with cap + 1 parents.

caterpillar(): a spine with leaves; the spine rows' parents are the rest of the spine, the leaf
rows' the whole spine, and the ranges run from half the spine's length (the middle) to all of it.

Latencies are whole milliseconds (quantum 1 ms), arcs of 1-3 quanta placed by a seeded generator,
so that a row has many distinct distances with uneven counts; a path that must be longer than
3 quanta an arc takes the rest on one arc. Losses lie on the k / 10000 grid (300 values) as in
sparse_graphs.py; many_losses gives more than 2,048 distinct reliabilities.

classify(g, path) restates the hand-over rules once, each with the dense.hip line it mirrors."""
import numpy as np

import oracle
from shadow_amd import graphs

MS = 1_000_000
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)

# the stages a row can end in
TREE, LEVELS, DEEP, ORDER, SWEEPS, PK = "tree", "levels", "deep", "order", "sweeps", "pk"
# the chains: Floyd-Warshall post pass (A), the same under SRT_FORM reltree=0, few attached rows
# (D), level build with packed level words (B), level build with u8 rows and packed words or int16
# predecessors (C)
FW, FW_LEVELS, ROWS, LV_PK, LV_TREE_PK, LV_TREE_16 = "fw", "fw_levels", "rows", "lv_pk", \
    "lv_tree_pk", "lv_tree_16"

_cache = {}


def ld_of(n):
    return (n + 127) // 128 * 128


def tree_cap(n, packed=False):
    """rel_tree_launch (dense.hip:1274-1295): the slots of rel_tree_kernel's size classes."""
    return 1024 if n <= 1024 else 4096 if n <= 4096 else 8192 if packed else 7168


def deep_cap(n):
    """rel_fw_rows (dense.hip:1874-1875): rel_deep_kernel's slots, 14 B each in 160 KB less
    1 KB of static LDS, the bitmap with its prefix and the 1,024 buckets."""
    fixed = 8 * (ld_of(n) >> 5) + 4 * 1024
    return min(n, (160 * 1024 - 1024 - fixed) // 14) & ~63


def pk_cap(n, ntab):
    """rel_pk_launch (dense.hip:1486-1487): rel_pk_kernel's slots, 12 B each in 80 KB less the
    bitmap with its prefix and the reliability table."""
    fixed = 8 * (ld_of(n) >> 5) + 8 * ((ntab + 2) & ~1)
    return min(n, (80 * 1024 - fixed) // 12) & ~63


def pk_width(n):
    """rel_pk_launch (dense.hip:1490-1493): the 16-byte pieces per thread, K of rel_pk_kernel<K>."""
    k = (ld_of(n) + 2047) // 2048
    return next(x for x in (1, 2, 4, 8, 16) if k <= x)


def distinct_rel(g):
    """The distinct reliabilities of g's arcs: the level build's table (st.rel_table)."""
    off = g.src != g.dst
    return len(np.unique(1.0 - g.loss[off]))


def stage_of(path, n, mx, parents, ntab=0):
    """The kernel that finishes a row of range mx with `parents` parents."""
    if path == FW:
        if mx <= 64 and parents <= tree_cap(n):           # rel_tree_kernel's bail, dense.hip:1196
            return TREE
        if mx < 1024 and parents <= deep_cap(n):          # rel_deep_kernel's, dense.hip:1716
            return DEEP
        return ORDER if mx < 1024 else SWEEPS             # rel_order_kernel's, dense.hip:1562
    if path == FW_LEVELS:                                 # rel_levels_kernel's, dense.hip:1036
        return LEVELS if mx <= 64 else SWEEPS
    if path == ROWS:                                      # no deep or order stage, dense.hip:2627
        return TREE if mx <= 64 and parents <= tree_cap(n) else SWEEPS
    if path == LV_PK:                                     # rel_pk_kernel's bail, dense.hip:1406
        return PK if parents <= pk_cap(n, ntab) else SWEEPS
    if path in (LV_TREE_PK, LV_TREE_16):                  # dense.hip:1289, 1196
        return TREE if mx <= 64 and parents <= tree_cap(n, path == LV_TREE_PK) else SWEEPS
    raise ValueError(path)


def edge_list(g):
    return oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)


def row_facts(g, rows=None):
    """(mx, parents) int64 arrays over the source rows `rows` (None: every row), from the oracle's
    distances and predecessors: the largest finite off-diagonal distance in quanta, and the number
    of distinct predecessors other than the source. Computed once per graph for rows=None."""
    if rows is None and getattr(g, "_facts", None) is not None:
        return g._facts
    el = edge_list(g)
    idx = np.arange(g.n) if rows is None else np.asarray(rows, np.int64)
    mx = np.zeros(len(idx), np.int64)
    par = np.zeros(len(idx), np.int64)
    step = max(1, (1 << 22) // g.n)
    for b in range(0, len(idx), step):
        srcs = idx[b:b + step]
        if rows is None:
            out = oracle.sssp_rows(el, int(srcs[0]), int(srcs[-1]) + 1, nthreads=8, want_pred=True)
            chunks = [(out, srcs, b)]
        else:  # a source list: one row at a time (the list form returns no predecessors)
            chunks = [(oracle.sssp_rows(el, int(s), int(s) + 1, want_pred=True), srcs[i:i + 1],
                       b + i) for i, s in enumerate(srcs)]
        for out, ss, at in chunks:
            d, p = out["lat_int"], out["pred"]
            k = np.arange(len(ss))
            reach = d != U64_MAX
            reach[k, ss] = False
            mx[at:at + len(ss)] = np.where(reach, d, 0).max(axis=1) // np.uint64(MS)
            mark = np.zeros(d.shape, bool)
            r, t = np.nonzero(reach & (p >= 0))
            mark[r, p[r, t]] = True
            mark[k, ss] = False
            par[at:at + len(ss)] = mark.sum(axis=1)
    if rows is None:
        g._facts = (mx, par)
    return mx, par


def classify(g, path, rows=None):
    """Per source row: (mx, parents, stage) -- int64 [k], int64 [k], list of stage names."""
    mx, par = row_facts(g, rows)
    ntab = distinct_rel(g)
    return mx, par, [stage_of(path, g.n, int(m), int(p), ntab) for m, p in zip(mx, par)]


def rows_in(g, path, stage, mx=None, parents=None):
    """The rows of g that `path` finishes in `stage` (with that range / parent count, if given)."""
    m, p, st = classify(g, path)
    keep = np.array([s == stage for s in st])
    if mx is not None:
        keep &= m == mx
    if parents is not None:
        keep &= p == parents
    return np.nonzero(keep)[0]


def _loss(seed, src, dst, many_losses):
    if many_losses:
        loss = np.random.default_rng(seed).random(len(src)) * 0.05
        assert len(np.unique(1.0 - loss)) > 2048
        return loss
    return (graphs.hash_u64(seed, 11, src.astype(np.uint64), dst.astype(np.uint64))
            % np.uint64(300)).astype(np.float64) / 10000.0


def _graph(n, src, dst, w, seed, many_losses, name):
    src, dst = np.asarray(src, np.int32), np.asarray(dst, np.int32)
    g = graphs.Graph(n, False, src, dst, np.asarray(w, np.int64) * MS,
                     _loss(seed, src, dst, many_losses), name)
    assert len(src) == n - 1  # a tree
    return g


def _path_weights(rng, arcs, depth):
    """`arcs` weights from {1, 2, 3} that sum to `depth`, the increments at random places; what
    3 * arcs cannot hold goes onto the last arc."""
    assert depth >= arcs >= 1, (depth, arcs)
    w = np.ones(arcs, np.int64)
    rest = depth - arcs
    for i in rng.permutation(arcs):
        if rest <= 0:
            break
        add = min(rest, int(rng.integers(1, 3)))
        w[i] += add
        rest -= add
    w[-1] += rest
    return w


def _build_spider(chains, length, extra, ecc0, seed, many_losses):
    rng = np.random.default_rng(seed)
    src, dst, w = [], [], []
    v = 1
    for c in range(chains):
        # path 0 reaches ecc0 exactly, the others end up to 7 quanta short of it
        depth = ecc0 if c == 0 else max(length, ecc0 - int(rng.integers(0, 8)))
        ids = np.arange(v, v + length)
        src.append(np.concatenate([[0], ids[:-1]]))
        dst.append(ids)
        # path 0 ends in an arc of 1: row 0 has a parent one quantum below its range, so the
        # last pass over the parents' distances has work to do
        w.append(np.append(_path_weights(rng, length - 1, depth - 1), 1) if c == 0 else
                 _path_weights(rng, length, depth))
        v += length
    for _ in range(extra):  # paths of two: one parent and one end each
        src.append(np.array([0, v]))
        dst.append(np.array([v, v + 1]))
        w.append(rng.integers(1, 3, 2))
        v += 2
    return _graph(v, np.concatenate(src), np.concatenate(dst), np.concatenate(w), seed,
                  many_losses, f"spider{chains}x{length}+{extra}e{ecc0}")


def spider(chains, length, extra=0, ecc0=None, seed=43, many_losses=False):
    """Vertex 0 with `chains` paths of `length` vertices and `extra` paths of two; row 0 has the
    range ecc0 (default: 2 * length) and chains * (length - 1) + extra parents, the inner
    vertices' rows as many and the path ends' rows one more; row 0's farthest target (path 0's
    end) hangs on a parent at ecc0 - 1 -- all asserted with the oracle."""
    ecc0 = 2 * length if ecc0 is None else ecc0
    key = ("spider", chains, length, extra, ecc0, seed, many_losses)
    if key not in _cache:
        assert chains >= 2 and length >= 2 and ecc0 >= max(length, 3)
        g = _build_spider(chains, length, extra, ecc0, seed, many_losses)
        assert g.n == 1 + chains * length + 2 * extra
        g.parents0 = chains * (length - 1) + extra
        ends = np.concatenate([length * (1 + np.arange(chains)),
                               1 + chains * length + 2 * np.arange(extra) + 1]).astype(np.int64)
        g.ends = ends
        g.extra_ends = ends[chains:]
        inner = np.setdiff1d(np.arange(1, g.n), ends)
        probe = np.unique(np.concatenate([[0], inner[[0, len(inner) // 2, -1]], ends[[0, -1]]]))
        mx, par = row_facts(g, probe) if g.n > 3000 else row_facts(g)
        if g.n <= 3000:
            mx, par = mx[probe], par[probe]
        at = {int(v): i for i, v in enumerate(probe)}
        assert mx[at[0]] == ecc0 and par[at[0]] == g.parents0, (mx[at[0]], par[at[0]])
        row0 = oracle.sssp_rows(edge_list(g), 0, 1, want_pred=True)
        far = int(row0["lat_int"][0].argmax())
        assert far == length and int(row0["lat_int"][0, row0["pred"][0, far]]) == (ecc0 - 1) * MS
        for v in inner[[0, len(inner) // 2, -1]]:
            assert par[at[int(v)]] == g.parents0, int(v)
        for v in ends[[0, -1]]:
            assert par[at[int(v)]] == g.parents0 + 1 and mx[at[int(v)]] > ecc0, int(v)
        _cache[key] = g
    return _cache[key]


def two_spiders(a, b):
    """Two spiders side by side: every row has unreachable targets. g.off: b's first vertex."""
    key = ("two", a.name, b.name)
    if key not in _cache:
        g = graphs.Graph(a.n + b.n, False, np.concatenate([a.src, b.src + a.n]).astype(np.int32),
                         np.concatenate([a.dst, b.dst + a.n]).astype(np.int32),
                         np.concatenate([a.lat_ns, b.lat_ns]), np.concatenate([a.loss, b.loss]),
                         f"{a.name}+{b.name}")
        g.off = a.n
        el = edge_list(g)
        d = oracle.sssp_rows(el, 0, 1)["lat_int"][0]
        assert (d[:a.n] != U64_MAX).all() and (d[a.n:] == U64_MAX).all()
        d = oracle.sssp_rows(el, a.n, a.n + 1)["lat_int"][0]
        assert (d[:a.n] == U64_MAX).all() and (d[a.n:] != U64_MAX).all()
        _cache[key] = g
    return _cache[key]


def caterpillar(spine=1153, leaves=40, at=1023, seed=47):
    """A spine of `spine` vertices (0 .. spine - 1: arcs of 1-3 quanta over its first half, of 1
    over the rest) with a leaf at either end and the other leaves on consecutive spine vertices
    around the one whose row has the range `at`: spine rows with the ranges at and at + 1 and
    spine - 1 parents, leaf rows with the same ranges and `spine` parents -- asserted."""
    key = ("cat", spine, leaves, at, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        ws = np.ones(spine - 1, np.int64)
        half = (spine - 1) // 2
        ws[:half] = 1 + (rng.random(half) < 0.15) * rng.integers(1, 3, half)
        pos = np.concatenate([[0], np.cumsum(ws)])       # spine vertex i lies pos[i] from vertex 0
        wl = rng.integers(1, 4, leaves)                  # leaf arcs; leaf 0 hangs on vertex 0
        ecc_left = pos + wl[0]                           # a spine row's distance to leaf 0
        i0 = int(np.searchsorted(ecc_left, at))
        assert ecc_left[i0] == at and half < i0 - leaves and i0 + leaves < spine - 1, i0
        host = np.concatenate([[0, spine - 1], i0 - (leaves - 2) // 2 + np.arange(leaves - 2)])
        leaf = spine + np.arange(leaves)
        src = np.concatenate([np.arange(spine - 1), host])
        dst = np.concatenate([np.arange(1, spine), leaf])
        g = _graph(spine + leaves, src, dst, np.concatenate([ws, wl]), seed, False,
                   f"caterpillar{spine}+{leaves}")
        g.spine, g.at = spine, at
        mx, par = row_facts(g)
        assert (par[:spine] == spine - 1).all() and (par[spine:] == spine).all()
        for rows, p in ((slice(0, spine), spine - 1), (slice(spine, g.n), spine)):
            for e in (at, at + 1):
                assert ((mx[rows] == e) & (par[rows] == p)).any(), (p, e)
        _cache[key] = g
    return _cache[key]


# --- the cases' graphs, each asserting the property its case is about -------------------------

def _named(g, path, row, stage, mx=None, parents=None):
    m, p, st = classify(g, path, [row])
    assert st[0] == stage, (g.name, path, row, st[0], stage, int(m[0]), int(p[0]))
    assert mx is None or m[0] == mx, (g.name, row, int(m[0]), mx)
    assert parents is None or p[0] == parents, (g.name, row, int(p[0]), parents)


F1_SHAPES = {261: (10, 26, 0), 1025: (32, 32, 0), 4097: (128, 32, 0)}


def f1_range(n, ecc0):
    """Row 0 of range 64 (rel_tree_kernel) | 65 (rel_deep_kernel) at n = 261, 1025, 4097."""
    g = spider(*F1_SHAPES[n], ecc0=ecc0)
    assert g.n == n and g.parents0 <= min(tree_cap(n), deep_cap(n))
    _named(g, FW, 0, TREE if ecc0 <= 64 else DEEP, mx=ecc0)
    _named(g, FW_LEVELS, 0, LEVELS if ecc0 <= 64 else SWEEPS, mx=ecc0)
    return g


def f2_caterpillar():
    """Ranges 1023 | 1024 at n = 1193 (deep cap 1152): spine rows of 1023 take rel_deep_kernel
    (1152 parents), leaf rows of 1023 rel_order_kernel (1153), both kinds of 1024 the sweeps.
    g.named: one row of each."""
    g = caterpillar()
    assert g.n == 1193 and deep_cap(g.n) == 1152 == g.spine - 1
    g.named = {}
    for stage, mx, par in ((DEEP, 1023, 1152), (ORDER, 1023, 1153), (SWEEPS, 1024, 1152),
                           (SWEEPS, 1024, 1153)):
        rows = rows_in(g, FW, stage, mx=mx, parents=par)
        assert len(rows), (stage, mx, par)
        g.named[(stage, mx, par)] = int(rows[0])
    return g


def f3_tree_cap(over):
    """Row 0 within 64 quanta with 7168 (rel_tree_kernel's cap above n = 4096) | 7169 parents;
    the second must reach rel_deep_kernel, whose cap at this n is above it."""
    g = spider(128, 57, extra=over, ecc0=64)
    assert tree_cap(g.n) == 7168 and g.parents0 == 7168 + over < deep_cap(g.n)
    _named(g, FW, 0, DEEP if over else TREE, mx=64, parents=7168 + over)
    _named(g, FW_LEVELS, 0, LEVELS)
    return g


def f4_deep_cap_small():
    """n = 261, deep cap 256 (n binds it): row 0 and the inner rows hold 256 parents
    (rel_deep_kernel), the path ends' rows 257 (rel_order_kernel); every range in [65, 1023]."""
    g = spider(4, 65, ecc0=100)
    assert g.n == 261 and deep_cap(261) == 256 == g.parents0
    mx, par, st = classify(g, FW)
    assert 65 <= mx.min() and mx.max() <= 1023
    assert all((s == DEEP) == (p == 256) and (s == ORDER) == (p == 257) for s, p in zip(st, par))
    assert (par == 256).any() and (par == 257).any()
    return g


def f4_deep_cap_large():
    """n = 11,419 (ld = 11,520): the LDS formula binds the deep cap at 11,072. Row 0 and the inner
    rows hold exactly that (rel_deep_kernel at its largest LDS request), the ends' rows one more
    (rel_order_kernel)."""
    g = spider(346, 33, ecc0=40)
    assert ld_of(g.n) == 11520 and deep_cap(g.n) == 11072 == g.parents0 < g.n & ~63
    _named(g, FW, 0, DEEP, mx=40, parents=11072)             # over rel_tree_kernel's 7168 slots
    _named(g, FW, 17, DEEP, parents=11072)
    _named(g, FW, int(g.ends[0]), ORDER, parents=11073)
    _named(g, FW, int(g.ends[-1]), ORDER, parents=11073)
    return g


F5_SHAPES = {1024: (33, 31, 0), 1025: (32, 32, 0), 4096: (91, 45, 0), 4097: (128, 32, 0)}


def f5_border(n):
    """n = 1024 | 1025 | 4096 | 4097: the size classes' borders. Row 0 within 64 quanta, the last
    vertex (a path's end: target index n - 1) past it."""
    g = spider(*F5_SHAPES[n], ecc0=64)
    assert g.n == n and int(g.ends[-1]) == n - 1
    _named(g, FW, 0, TREE, mx=64)
    _named(g, FW, n - 1, DEEP if g.parents0 + 1 <= deep_cap(n) else ORDER)
    _named(g, FW_LEVELS, n - 1, SWEEPS)
    return g


def f6_mixed():
    """n = 261 for the few-rows build: the hub's row spans 48 quanta and the rows near it stay
    within 64 (tree, or levels), the rows towards the paths' ends pass it (sweeps); many of each."""
    g = spider(20, 13, ecc0=48)
    assert g.n == 261
    for path, short in ((ROWS, TREE), (FW_LEVELS, LEVELS)):
        _, _, st = classify(g, path)
        assert min(st.count(short), st.count(SWEEPS)) >= 100, (path, st.count(short))
    return g


def f8_disjoint():
    """Two spiders, n = 317 (deep cap 256): the first holds 256-parent rows (deep), the short
    paths' ends with 257 and ranges below 1024 (order) and the long paths' ends with 257 and
    ranges past 1023 (sweeps); the second is small and its row 0 stays within 64 quanta (tree)."""
    a = spider(4, 64, extra=4, ecc0=600, seed=53)
    b = spider(3, 17, ecc0=40, seed=59)
    g = two_spiders(a, b)
    assert g.n == 317 and deep_cap(g.n) == 256 == a.parents0
    _named(g, FW, 0, DEEP, mx=600, parents=256)
    _named(g, FW, int(a.extra_ends[0]), ORDER, parents=257)
    _named(g, FW, int(a.ends[0]), SWEEPS, parents=257)
    _named(g, FW, g.off, TREE, mx=40)
    g.named = [0, int(a.extra_ends[0]), int(a.ends[0]), g.off]
    return g


def _level_spider(chains, length, extra, ecc0, lo, hi, **kw):
    """A spider whose largest distance E (between two path ends) lies in [lo, hi]."""
    g = spider(chains, length, extra, ecc0, **kw)
    mx, _ = row_facts(g, g.ends)
    g.E = int(mx.max())
    assert lo <= g.E <= hi and g.E <= 2 * ecc0, (g.name, g.E)
    return g


L1_SHAPES = {168: (12, 15, 0), 128: (16, 9, 0), 129: (16, 9, 1)}


def l1_pk_cap_small(parents):
    """E <= 31, the cap of rel_pk_kernel bound by n (128): row 0 with 168 | 128 | 129 parents."""
    g = _level_spider(*L1_SHAPES[parents], ecc0=15, lo=2, hi=31)
    cap = pk_cap(g.n, distinct_rel(g))
    assert cap == 128 == g.n & ~63 and g.parents0 == parents
    _named(g, LV_PK, 0, PK if parents <= cap else SWEEPS, parents=parents)
    _named(g, LV_PK, int(g.ends[0]), SWEEPS, parents=parents + 1)
    return g


def l2_pk_cap_formula():
    """E <= 31 at n = 6,965 (ld = 7,040, K = 4): the LDS formula binds rel_pk_kernel's cap (6,464
    with the 300 reliabilities of the grid). Row 0 holds exactly that, the ends' rows one more."""
    g = _level_spider(497, 14, 3, ecc0=15, lo=2, hi=31)
    ntab = distinct_rel(g)
    assert ntab == 300 and ld_of(g.n) == 7040 and pk_width(g.n) == 4
    assert pk_cap(g.n, ntab) == 6464 == g.parents0 < g.n & ~63
    _named(g, LV_PK, 0, PK, parents=6464)
    _named(g, LV_PK, int(g.ends[0]), SWEEPS, parents=6465)
    return g


L3_SHAPES = {2048: (157, 13, 3), 2176: (167, 13, 2), 4096: (315, 13, 0), 4224: (323, 13, 12)}


def l3_pk_width(n):
    """E <= 31 at n = ld = 2048 (K = 1), 2176 (K = 2), 4096 (K = 2), 4224 (K = 4): the last target
    fills the last lane's last piece. No row of such a graph can pass the cap (see
    test_gpu_rel_forms.py): every row takes rel_pk_kernel, asserted."""
    g = _level_spider(*L3_SHAPES[n], ecc0=15, lo=2, hi=31)
    assert g.n == n == ld_of(n) and pk_width(n) == {2048: 1, 2176: 2, 4096: 2, 4224: 4}[n]
    assert g.parents0 + 1 <= pk_cap(n, distinct_rel(g))
    _named(g, LV_PK, 0, PK)
    _named(g, LV_PK, n - 1, PK)
    return g


def l4_tree_cap(over, many_losses=False):
    """32 <= E <= 64 above n = 4096: row 0 with 8192 | 8193 parents (packed words), or with
    7168 | 7169 and more than 2,048 distinct reliabilities (int16 predecessors)."""
    if many_losses:
        g = _level_spider(256, 29, over, ecc0=32, lo=32, hi=64, many_losses=True)
        path, cap = LV_TREE_16, 7168
        assert distinct_rel(g) > 2048
    else:
        g = _level_spider(303, 28, 11 + over, ecc0=32, lo=32, hi=64)
        path, cap = LV_TREE_PK, 8192
        assert distinct_rel(g) <= 2048
    assert g.n > 4096 and tree_cap(g.n, not many_losses) == cap and g.parents0 == cap + over
    _named(g, path, 0, SWEEPS if over else TREE, mx=32, parents=cap + over)
    _named(g, path, 1, SWEEPS if over else TREE, parents=cap + over)
    _named(g, path, int(g.ends[0]), SWEEPS, parents=cap + over + 1)
    return g


def self_pair(g, v):
    """(latency ns, reliability) of the pair (v, v) in a graph without self-loops: out and back
    over v's cheapest edge, the first in (neighbour, edge) order among equals."""
    e = np.nonzero((g.src == v) | (g.dst == v))[0]
    nb = np.where(g.src[e] == v, g.dst[e], g.src[e])
    best = e[np.lexsort((e, nb, g.lat_ns[e]))[0]]
    r = 1.0 - g.loss[best]
    return 2 * int(g.lat_ns[best]), r * r
