"""Graphs for the dense Floyd-Warshall tiers' edge tests (test_gpu_fw_edges.py), each measured
with the CPU oracle before it is handed out (test_fw_graphs.py runs every assertion without a GPU).

The u16 forms of shadow_amd/csrc/fw16.hip are exact only below a cap (0x3DFF for the f16-compare
rounds, the squaring and the few-rows build, 0x7FFF for the pk_min rounds): a real pair that ends
on the cap sends the build one tier wider, and distances <= 254 switch the post pass to bytes.

heavy_tail(E): level_graphs.core_tail's shape -- a complete core (1-3 ms arcs, self-loops, so the
quantum stays 1 ms) and the braided two-rail tail off vertex 0 -- with RUNGS heavy rungs instead
of 1-ms ones: every arc into rung i weighs the same (both rails' vertices of rung i stay tied
from every source on the core's side, so reliability depends on the canonical predecessor), and
the last rung is tuned so that the oracle's largest off-diagonal distance is exactly E. The rung
count is fixed (n = core + 2 * RUNGS = 261: ld = 384, three tile rows, six 64-pivot rounds, n % 8
!= 0 so padding columns share a 16-byte group with real ones); the rungs' weight follows from E:
about E / RUNGS quanta, ~500 at the f16-compare cap, ~1,100 at the pk_min cap, 8 at E = 254.

one_rank_far(E_far, E_near): directed, n = 384. A heavy chain t_L -> ... -> t_1 -> 0 leads into a
complete core that reaches every chain vertex over 1-3 ms arcs, so only the chain vertices' own
rows (indices >= 256: the last rank's block on 2 and 3 ranks) hold a distance above E_near.

long_arc_traps(): level_graphs' core + 1-ms tail (E < 254) with extra edges at and past every
cap; those of 0x10000 + d(u, t) quanta would be exactly tight after a 16-bit truncation.
"""
import numpy as np

import level_graphs as lg
import oracle
from level_graphs import MS, largest_distance, oracle_table, row_eccentricity
from shadow_amd import graphs

CAP_F = 0x3DFF     # fw16.hip CAP_F (f16-compare rounds, squaring) and dense.hip ROWS_CAP
CAP_U = 0x7FFF     # fw16.hip CAP_U (pk_min rounds)
RUNGS = 30
CAP_EDGES = [254, 255, CAP_F - 1, CAP_F, CAP_F + 1, CAP_U - 1, CAP_U, CAP_U + 1]
FAR_PAIRS = [(200, 255), (200, CAP_F - 1), (200, CAP_F), (200, CAP_U)]
ROWS_FAR = 20000   # heavy_tail's E of the few-rows case whose attached rows stay below ROWS_CAP

_cache = {}


def _grid_loss(seed, src, dst):
    """level_graphs' small grid: 300 distinct losses, hashed per (src, dst)."""
    return (graphs.hash_u64(seed, 11, src.astype(np.uint64), dst.astype(np.uint64))
            % np.uint64(300)).astype(np.float64) / 10000.0


def _build_heavy_tail(core, rung_w, seed, directed):
    hops = len(rung_w)
    c = graphs.complete_directed(core, seed, lat_max=3) if directed else \
        graphs.complete_graph(core, seed, lat_max=3)
    ts, td = lg._tail_edges(core, hops)
    w = np.asarray(rung_w, np.int64)[(td - core) // 2] if hops else np.zeros(0, np.int64)
    if directed:  # both orientations as separate arcs of one weight (independent losses below)
        ts, td, w = np.concatenate([ts, td]), np.concatenate([td, ts]), np.concatenate([w, w])
    loops = core + 2 * np.arange(hops, dtype=np.int64)  # self-loops on rail a only
    src = np.concatenate([c.src, ts, loops]).astype(np.int32)
    dst = np.concatenate([c.dst, td, loops]).astype(np.int32)
    lat_ms = np.concatenate([c.lat_ns // MS, w, 1 + (loops % 7)]).astype(np.int64)
    g = graphs.Graph(core + 2 * hops, directed, src, dst, lat_ms * MS, _grid_loss(seed, src, dst),
                     f"core{core}_heavy{hops}{'_dir' if directed else ''}")
    g.core = core
    return g


def heavy_tail(target, core=201, seed=23, directed=False):
    """The core + heavy tail graph whose largest off-diagonal distance is exactly `target`
    quanta, asserted against the oracle before it is handed out."""
    key = ("heavy", target, core, seed, directed)
    if key not in _cache:
        g0 = _build_heavy_tail(core, [], seed, directed)
        d0 = oracle_table(g0)["lat_int"] // np.uint64(MS)
        # the farthest core vertex from the tail's end: over vertex 0, both ways round
        reach = int(max(d0[1:, 0].max(), d0[0, 1:].max()))
        total = target - reach
        base = total // RUNGS
        assert base >= 1, (target, reach)
        rung_w = [base] * (RUNGS - 1) + [total - base * (RUNGS - 1)]
        g = _build_heavy_tail(core, rung_w, seed, directed)
        assert g.n % 8 != 0 and (g.n + 127) // 128 * 128 == 384, g.n
        assert lg.quantum(g) == MS
        e = largest_distance(g)
        assert e == target, f"heavy_tail({target}): the oracle measures E = {e} (rungs {rung_w})"
        _cache[key] = g
    return _cache[key]


def farthest_pair(g):
    """(s, t) of one pair at the oracle's largest finite off-diagonal distance."""
    d = oracle_table(g)["lat_int"].copy()
    d[d == lg.U64_MAX] = 0
    np.fill_diagonal(d, 0)
    s, t = np.unravel_index(int(d.argmax()), d.shape)
    return int(s), int(t)


def _build_one_rank_far(core, chain_w, seed):
    L = len(chain_w)
    c = graphs.complete_directed(core, seed, lat_max=3)
    t = core + np.arange(L, dtype=np.int64)                # t_1 .. t_L
    into = np.concatenate([[0], t[:-1]])                   # t_1 -> 0, t_i -> t_(i-1)
    feeders = np.repeat(np.arange(3, dtype=np.int64), L)   # core vertices 0, 1, 2 -> every t_i
    fed = np.tile(t, 3)
    cheap = 1 + (graphs.hash_u64(seed, 12, feeders.astype(np.uint64), fed.astype(np.uint64))
                 % np.uint64(3)).astype(np.int64)
    loops = t[::2]
    src = np.concatenate([c.src, t, feeders, loops]).astype(np.int32)
    dst = np.concatenate([c.dst, into, fed, loops]).astype(np.int32)
    lat_ms = np.concatenate([c.lat_ns // MS, np.asarray(chain_w, np.int64), cheap,
                             1 + (loops % 7)]).astype(np.int64)
    return graphs.Graph(core + L, True, src, dst, lat_ms * MS, _grid_loss(seed, src, dst),
                        f"one_rank_far{core}_{L}")


def one_rank_far(e_far, e_near, core=352, chain=32, seed=41):
    """Directed, n = 384: rows [0, 256) have eccentricity <= e_near, the largest eccentricity of
    the last rank's block (2 and 3 ranks) is exactly e_far -- both asserted with the oracle."""
    key = ("far", e_far, e_near, core, chain, seed)
    if key not in _cache:
        assert core >= 256 and core + chain == 384
        base = (e_far - 6) // chain
        assert base >= 1, e_far
        w = [base] * chain
        ecc = row_eccentricity(_build_one_rank_far(core, w, seed))
        w[-1] += e_far - int(ecc.max())  # t_L -> t_(L-1): the first arc of the longest path
        assert w[-1] >= 1, w[-1]
        g = _build_one_rank_far(core, w, seed)
        assert g.n == 384 and lg.quantum(g) == MS
        ecc = row_eccentricity(g)
        assert int(ecc[:256].max()) <= e_near, int(ecc[:256].max())
        for ranks in (2, 3):
            rows = lg.shard_rows(g.n, ranks)
            assert all(b < e for b, e in rows), rows
            for b, e in rows[:-1]:
                assert int(ecc[b:e].max()) <= e_near, (ranks, b, e, int(ecc[b:e].max()))
            b, e = rows[-1]
            assert b <= 256 and int(ecc[b:e].max()) == e_far == largest_distance(g), \
                (ranks, b, e, int(ecc[b:e].max()))
        assert (oracle_table(g)["lat_int"] != lg.U64_MAX).all()
        _cache[key] = g
    return _cache[key]


def long_arc_traps(core=201, hops=30, seed=23):
    """level_graphs' core + 1-ms tail (n = 261, E < 254) with extra edges (u, t), u in the core and
    t in the tail (no edge of the base graph joins them): 0x3DFF, 0x7FFF and 0xFFFF quanta -- at
    each u16 cap and at the top of 16 bits --, 0x10001 (a 16-bit truncation leaves 1 quantum,
    shorter than any path to the tail) and 0x10000 + d(u, t), each of the last with a loss
    of its own off the grid. None of them is on a shortest path; truncated to 16 bits the last
    kind is exactly tight, and u itself (distance 0 on its own row) the canonical predecessor.
    g.traps: the (u, t) pairs of the 0x10000 + d arcs; g.long_arcs: every extra pair."""
    key = ("traps", core, hops, seed)
    if key not in _cache:
        g0 = lg._build_core_tail(core, hops, seed, False, False, MS)
        d = oracle_table(g0)["lat_int"] // np.uint64(MS)
        a = lambda i: core + 2 * (i - 1)      # a_i, b_i: the rails' vertices of rung i
        b = lambda i: a(i) + 1
        fixed = [(5, a(3), CAP_F), (17, b(10), CAP_F), (29, a(hops), CAP_U), (90, b(7), CAP_U),
                 (8, a(12), 0xFFFF), (133, b(hops), 0xFFFF), (3, a(1), 0xFFFF),
                 # low 16 bits 1: a truncation shortens d(u, t) itself (>= 2 over vertex 0)
                 (61, b(20), 0x10001), (170, a(hops), 0x10001)]
        traps = [(3, b(1)), (40, a(2)), (77, b(15)), (150, a(hops)), (199, a(1)), (12, b(hops))]
        base = set(zip(g0.src.tolist(), g0.dst.tolist()))
        for u, t, _ in fixed + [(u, t, 0) for u, t in traps]:
            assert 0 < u < core <= t < g0.n and (u, t) not in base and (t, u) not in base
        for u, t in traps:  # d(u, t) comes over an intermediate vertex
            assert int(d[u, t]) >= 2 and int(d[u, t]) == int(d[t, u])
        es = np.array([u for u, _, _ in fixed] + [u for u, _ in traps], np.int32)
        et = np.array([t for _, t, _ in fixed] + [t for _, t in traps], np.int32)
        ew = np.array([w for _, _, w in fixed] + [0x10000 + int(d[u, t]) for u, t in traps],
                      np.int64)
        eloss = np.concatenate([_grid_loss(seed + 1, es[:len(fixed)], et[:len(fixed)]),
                                (311 + 7 * np.arange(len(traps))) / 10000.0])
        g = graphs.Graph(g0.n, False, np.concatenate([g0.src, es]), np.concatenate([g0.dst, et]),
                         np.concatenate([g0.lat_ns, ew * MS]), np.concatenate([g0.loss, eloss]),
                         "long_arc_traps")
        assert g.n % 8 != 0 and (g.n + 127) // 128 * 128 == 384 and lg.quantum(g) == MS
        assert largest_distance(g) < 254
        # not one of the extra arcs is on a shortest path: the table is the base graph's
        e0, e1 = oracle_table(g0), oracle_table(g)
        assert np.array_equal(e0["lat_int"], e1["lat_int"])
        assert np.array_equal(e0["rel"].view(np.uint64), e1["rel"].view(np.uint64))
        # armed: a truncated trap arc would make u the predecessor of t on row u, and u is below
        # the true one (so it wins under a smallest-index rule as well as by its distance 0)
        el = oracle.EdgeList(g0.n, False, g0.src, g0.dst, g0.lat_ns, g0.loss)
        armed = 0
        for u, t in traps:
            pred = int(oracle.sssp_rows(el, u, u + 1, want_pred=True)["pred"][0, t])
            assert pred not in (u, -1), (u, t, pred)
            armed += u < pred
        assert armed >= 1
        g.traps = traps
        g.long_arcs = [(u, t) for u, t, _ in fixed] + traps
        _cache[key] = g
    return _cache[key]


def trap_rows(g):
    """The vertices the few-rows case of long_arc_traps attaches: both ends of every
    0x10000 + d arc, then ends of the other long arcs up to n / 12 vertices, increasing."""
    v = list(dict.fromkeys([x for p in g.traps for x in p] +
                           [x for p in g.long_arcs for x in p]))[:g.n // 12]
    return np.unique(np.array(v, np.int32))


def mid_tail_rows(g, limit, count):
    """Up to `count` tail vertices of a heavy_tail graph whose rows' eccentricity is <= limit
    (the middle of the tail), increasing."""
    ecc = row_eccentricity(g)
    v = np.nonzero(ecc[g.core:] <= limit)[0] + g.core
    assert len(v) >= 2, len(v)
    keep = v[np.linspace(0, len(v) - 1, min(count, len(v))).astype(np.int64)]
    return np.unique(keep).astype(np.int32)
