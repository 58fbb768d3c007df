"""The dense Floyd-Warshall tiers (shadow_amd/csrc/fw16.hip, dense.hip) on either side of every
distance cap, with graphs whose largest distance E is exact and oracle-checked (tests/fw_graphs.py).

The u16 forms are exact only below their cap: the f16-compare rounds and the min-plus squaring
below CAP_F = 0x3DFF, the pk_min rounds below CAP_U = 0x7FFF, the few-rows Bellman-Ford below
ROWS_CAP = 0x3DFF. fw16_finish_kernel reports a build inexact when a real pair holds exactly the
cap, and the callers rerun one tier wider, so E = cap - 1 is the last distance a tier serves and
E = cap the first the next one does; its second flag (every real distance <= 254) switches the
post pass to byte distances (pack_uk_kernel, pred_cols3_kernel, the u8 transpose), so E = 254 | 255
is a switch of its own. The graphs have n = 261 (ld = 384: padding columns at the cap in the same
16-byte group as real ones) or n = 384 exactly.

Every case holds the whole table to the CPU oracle, diagonal included -- latency bit-exact,
reliability within 1e-12 relative -- and asserts srt_build_stats.dist_enc: 11 squaring, 4
symmetric 64-pivot rounds, 3 every tile / directed, 8 symmetric row-sharded rounds, 2 u16 pk_min,
1 u32, 10 few rows. All builds keep n < 4,096, so the default dispatch never tries the levels."""
import numpy as np
import pytest
from conftest import set_form

import fw_graphs as fg
import level_graphs as lg
import oracle
from level_graphs import check_tables
from shadow_amd import graphs
from shadow_amd._lib import ALGO_AUTO, SRT_INF
from shadow_amd.topology import build_tables_subset

pytestmark = pytest.mark.gpu

# SRT_FORM keys, directed graph, the f16 encoding of the form (E <= CAP_F - 1)
FORMS = {
    "square": ({}, False, 11),
    "rounds": ({"square": "0"}, False, 4),
    "tiles": ({"square": "0", "sym": "0"}, False, 3),
    "directed": ({}, True, 11),
    "directed_rounds": ({"square": "0"}, True, 3),
}


def _tier(e, f16):
    return f16 if e <= fg.CAP_F - 1 else 2 if e <= fg.CAP_U - 1 else 1


def _form(monkeypatch, **kv):
    monkeypatch.delenv("SRT_FORM", raising=False)
    monkeypatch.delenv("SRT_VIRTUAL_RANKS", raising=False)
    if kv:
        set_form(monkeypatch, **kv)


@pytest.mark.parametrize("e_near,e_far,enc", [p + (t,) for p, t in zip(fg.FAR_PAIRS, [3, 3, 2, 1])])
@pytest.mark.parametrize("ranks", [2, 3])
def test_one_rank_alone_past_a_switch(gpu, monkeypatch, ranks, e_near, e_far, enc):
    """Only the last rank's rows pass 254 quanta, or reach a cap: the exact-flag all-reduce must
    put every rank on the wider tier together, and each rank's byte-distance switch is its own
    (at E_far = 255 every rank but the last reads bytes)."""
    _form(monkeypatch)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    g = fg.one_rank_far(e_far, e_near)
    lat, rel, st = lg.build(g, ngpus=1)
    assert st.dist_enc == enc, (st.dist_enc, enc)
    check_tables(g, lat, rel, f"one rank far x{ranks} E={e_far}")


@pytest.mark.parametrize("e", fg.CAP_EDGES)
@pytest.mark.parametrize("form", list(FORMS))
def test_cap_edges_one_gpu(gpu, monkeypatch, form, e):
    keys, directed, f16 = FORMS[form]
    _form(monkeypatch, **keys)
    g = fg.heavy_tail(e, directed=directed)
    lat, rel, st = lg.build(g)
    assert st.dist_enc == _tier(e, f16), (st.dist_enc, _tier(e, f16))
    check_tables(g, lat, rel, f"{form} E={e}")
    if e <= 255:  # the tie count keeps pred_cols2_kernel on the byte distances: the same table
        lat1, rel1, st1 = lg.build(g, count_ties=1)
        assert st1.dist_enc == st.dist_enc, (st1.dist_enc, st.dist_enc)
        assert np.array_equal(lat1, lat)
        assert np.array_equal(rel1.view(np.uint64), rel.view(np.uint64)), \
            np.argwhere(rel1.view(np.uint64) != rel.view(np.uint64))[:5]


@pytest.mark.parametrize("e", fg.CAP_EDGES)
@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("ranks", [2, 3])
def test_cap_edges_virtual_ranks(gpu, monkeypatch, ranks, directed, e):
    """Row shards of 128 | 256 rows over ld = 384; with 3 ranks the last holds 5 real rows."""
    _form(monkeypatch)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    g = fg.heavy_tail(e, directed=directed)
    lat, rel, st = lg.build(g, ngpus=1)
    want = _tier(e, 3 if directed else 8)
    assert st.dist_enc == want, (st.dist_enc, want)
    check_tables(g, lat, rel, f"x{ranks} {'directed ' if directed else ''}E={e}")


def _ring_with_chords(n, hop_ms=1):
    """test_dense_distance_encoding_tiers's graph on n vertices: an undirected ring with hop
    latencies hop_ms / hop_ms + 1 alternating, plus 12 chords of hop_ms * n // 3."""
    rng = np.random.default_rng(hop_ms)
    src = list(range(n))
    dst = [(i + 1) % n for i in range(n)]
    lat = [(hop_ms + (i % 2)) * lg.MS for i in range(n)]
    for _ in range(12):
        a, b = (int(x) for x in rng.choice(n, 2, replace=False))
        src.append(a)
        dst.append(b)
        lat.append(int(hop_ms * n // 3) * lg.MS)
    loss = rng.integers(0, 100, len(src)) * 1e-4
    return graphs.Graph(n, 0, np.array(src, np.int32), np.array(dst, np.int32),
                        np.array(lat, np.int64), loss)


@pytest.mark.parametrize("n", [100, 200])
def test_sharded_rounds_with_one_or_two_bands(gpu, monkeypatch, n):
    """The row-sharded symmetric rounds where the prologue sends every band there is: n = 100 is
    ld = 128, one band and one round, and the second of the two ranks holds no rows; n = 200 is
    ld = 256, two bands. Distances stay below ~150 quanta, so the f16-compare tier serves both."""
    _form(monkeypatch)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", "2")
    g = _ring_with_chords(n)
    lat, rel, st = lg.build(g, ngpus=1)
    assert st.dist_enc == 8, st.dist_enc
    check_tables(g, lat, rel, f"ring n={n} x2")


def _check_subset(g, verts, lat, rel, what):
    """test_dense_rows_few_attached's check: the oracle's rows of the attached sources off the
    diagonal, and the full oracle table's sub-table, diagonal included; bit for bit."""
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    rows = oracle.sssp_list(el, verts, nthreads=8)
    ix = np.ix_(np.arange(len(verts)), verts)
    off = ~np.eye(len(verts), dtype=bool)
    assert np.array_equal(lat[off], rows["lat_int"][ix][off]), what
    assert np.array_equal(rel[off], rows["rel"][ix][off]), what
    full = lg.oracle_table(g)
    sub = np.ix_(verts, verts)
    assert np.array_equal(lat, full["lat_int"][sub]), what
    assert np.array_equal(rel, full["rel"][sub]), what


def _subset(g, verts):
    assert 1 <= len(verts) <= g.n // 12
    lat, rel, _, _, st = build_tables_subset(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                             verts=verts, algo=ALGO_AUTO)
    return lat, rel, st


@pytest.mark.parametrize("form", ["square", "rounds", "x2", "rows"])
def test_long_arcs_do_not_widen_or_shorten(gpu, monkeypatch, form):
    """Arcs of 0x3DFF, 0x7FFF, 0xFFFF, 0x10001 and 0x10000 + d(u, t) quanta, E < 254: the
    narrowing to u16 clamps them (fw16_init_kernel, rows_w16_kernel), so the build stays on its
    narrowest tier, and none of them becomes a path or a predecessor."""
    _form(monkeypatch, **({"square": "0"} if form == "rounds" else {}))
    g = fg.long_arc_traps()
    if form == "rows":
        verts = fg.trap_rows(g)
        lat, rel, st = _subset(g, verts)
        assert st.dist_enc == 10, st.dist_enc
        _check_subset(g, verts, lat, rel, "long arcs, few rows")
        return
    if form == "x2":
        monkeypatch.setenv("SRT_VIRTUAL_RANKS", "2")
    lat, rel, st = lg.build(g, ngpus=1 if form == "x2" else None)
    assert st.dist_enc == {"square": 11, "rounds": 4, "x2": 8}[form], st.dist_enc
    check_tables(g, lat, rel, f"long arcs {form}")


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("e,enc", [(fg.CAP_F - 1, 10), (fg.CAP_F, 2)])
def test_few_rows_at_the_cap(gpu, monkeypatch, e, enc, directed):
    """The two ends of a pair at distance E attached: E = ROWS_CAP - 1 builds by rows, E =
    ROWS_CAP falls back to the all-pairs build (whose squaring saturates as well: pk_min rounds).
    The directed form takes the u16 transpose for the candidate lists."""
    _form(monkeypatch)
    g = fg.heavy_tail(e, directed=directed)
    s, t = fg.farthest_pair(g)
    verts = np.unique(np.array([s, t, g.n - 1, g.n - 2, 7], np.int32))
    lat, rel, st = _subset(g, verts)
    assert st.dist_enc == enc, (st.dist_enc, enc)
    assert int(lat.max()) == e * lg.MS
    _check_subset(g, verts, lat, rel, f"few rows E={e}")


def test_few_rows_ignore_rows_nobody_asked_for(gpu, monkeypatch):
    """E = 20,000 > ROWS_CAP, but the attached rows (the middle of the tail) stay below it: the
    rows build must serve them, whatever the unattached rows would reach."""
    _form(monkeypatch)
    g = fg.heavy_tail(fg.ROWS_FAR)
    verts = fg.mid_tail_rows(g, fg.CAP_F - 1, g.n // 12)
    assert int(lg.row_eccentricity(g)[verts].max()) <= fg.CAP_F - 1
    lat, rel, st = _subset(g, verts)
    assert st.dist_enc == 10, st.dist_enc
    _check_subset(g, verts, lat, rel, "few rows, far rows unattached")


@pytest.mark.parametrize("ranks", [2, 3])
def test_unreachable_pairs_end_on_u32_at_ranks(gpu, monkeypatch, ranks):
    """An unreachable pair holds the cap of either u16 tier: every rank ends on the u32 rounds,
    with SRT_INF where the oracle has no path."""
    _form(monkeypatch)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    g = lg.two_complete()
    lat, rel, st = lg.build(g, ngpus=1)
    assert st.dist_enc == 1, st.dist_enc
    unreached = lg.oracle_table(g)["lat_int"] == lg.U64_MAX
    assert unreached.any() and (lat[unreached] == np.uint64(SRT_INF * lg.quantum(g))).all()
    check_tables(g, lat, rel, f"two_complete x{ranks}", reachable_only=True)
