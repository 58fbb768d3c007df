"""The level build (shadow_amd/csrc/levels.hip, dist_enc 12) on either side of every switch it
takes on the last level D, with graphs whose largest distance E is exact and oracle-checked
(tests/level_graphs.py: core + braided tail).

The switches, from srt_levels_build and dense_post_levels: the level batches (1-5, single levels to
8, then 8 at a time), the second arc extraction past level 8, lvl_out8_kernel against
lvl_out_kernel at 16 levels, the packed 5-bit-level post pass up to 31 levels, level-order
reliability for rows spanning <= 64 quanta and sweeps for the rest, and the budget of 254 levels
with 0xFF as the u8 "unreached" mark: E = 254 builds by levels, E = 255 leaves for Floyd-Warshall.
Row eccentricities run from E/2 to E, so a build with 64 < E mixes level-order and sweep rows.

Every test holds the whole table to the CPU oracle, diagonal included: latency bit-exact,
reliability within 1e-12 relative. srt_build_stats.levels is the first level after which every
source of the rank is complete; level 1 never reports completion (levels.hip: "a graph settled
at level 1 reports 2 levels"), so it is max(E, 2)."""
import numpy as np
import pytest
from conftest import set_form

import level_graphs as lg
from level_graphs import LEVELS, check_tables
from shadow_amd._lib import ALGO_DENSE_FW

pytestmark = pytest.mark.gpu

BY_LEVELS = [1, 2, 5, 6, 8, 9, 16, 17, 31, 32, 33, 64, 65, 254]
OVER_BUDGET = [255, 300]


def _graph(e, **kw):
    return lg.all_ones() if e == 1 else lg.core_tail(e, **kw)


def _distinct_rel(g):
    """The distinct reliabilities 1 - loss of g's arcs (no parallel edges in these graphs; the
    self-loops are no arcs of the level build)."""
    off = g.src != g.dst
    return len(np.unique(1.0 - g.loss[off]))


def _levels_of(g, rows=None):
    ecc = lg.row_eccentricity(g)
    return max(2, int((ecc if rows is None else ecc[rows[0]:rows[1]]).max()))


def _assert_level_build(g, st, what, table=True, rows=None):
    assert st.dist_enc == LEVELS, (what, st.dist_enc)
    assert st.levels == _levels_of(g, rows), (what, st.levels, _levels_of(g, rows))
    assert st.rel_table == (_distinct_rel(g) if table else 0), (what, st.rel_table)


@pytest.mark.parametrize("e", BY_LEVELS)
def test_edge_builds_by_levels(gpu, monkeypatch, e):
    """Default form on each side of every switch: packed words up to E = 31, the u8 level rows
    from 32 (lvl_out8_kernel cannot apply there: lvl_out_kernel), sweeps past 64."""
    set_form(monkeypatch, levels="1")
    g = _graph(e)
    lat, rel, st = lg.build(g)
    _assert_level_build(g, st, f"E={e}")
    check_tables(g, lat, rel, f"E={e}")


@pytest.mark.parametrize("e", OVER_BUDGET)
def test_edge_over_budget_leaves_for_fw(gpu, monkeypatch, e):
    """E = 255 is one level past the budget (and the first distance the u8 rows cannot hold): the
    forced build runs its 254 levels, reports "not done" and the FW gives the table."""
    set_form(monkeypatch, levels="1")
    g = _graph(e)
    lat, rel, st = lg.build(g)
    assert st.dist_enc != LEVELS and st.levels == 0, (st.dist_enc, st.levels)
    check_tables(g, lat, rel, f"E={e}")


@pytest.mark.parametrize("e,core,budget", [(32, 280, 32), (32, 268, 33), (33, 268, 33),
                                           (33, 280, 31)])
def test_edge_budget_at_the_stash_width(gpu, monkeypatch, e, core, budget):
    """The arc fill takes the count pass's stash while the level budget is <= 32 (LVL_STASH_W)
    and the segmented sort past it. A forced build's budget is 254, so SRT_FORM memcap=1 (MiB)
    stands in for a smaller one: half of it over the plane's bytes (n x ld / 32 words), which the
    core's size sets to 32 | 33 levels here -- at and past the stash width with E = 32 and 33 --
    and to 31 < E = 33, which must leave for the FW."""
    set_form(monkeypatch, levels="1", memcap="1")
    g = _graph(e, core=core)
    ld = (g.n + 127) // 128 * 128
    assert (1 << 19) // (g.n * (ld // 32) * 4) == budget, g.n
    lat, rel, st = lg.build(g)
    if e <= budget:
        _assert_level_build(g, st, f"budget {budget} E={e}")
    else:
        assert st.dist_enc != LEVELS and st.levels == 0, (st.dist_enc, st.levels)
    check_tables(g, lat, rel, f"budget {budget} E={e}")


@pytest.mark.parametrize("e", [16, 17, 31, 32])
def test_edge_unpacked_form(gpu, monkeypatch, e):
    """SRT_FORM pkw=0: the u8 level rows by lvl_out8_kernel (E <= 16) and lvl_out_kernel (17 on),
    predecessor | reliability-index words and rel_tree_kernel; at 31 | 32 the form the default
    build falls into."""
    set_form(monkeypatch, levels="1", pkw="0")
    g = _graph(e)
    lat, rel, st = lg.build(g)
    _assert_level_build(g, st, f"pkw=0 E={e}")
    check_tables(g, lat, rel, f"pkw=0 E={e}")


@pytest.mark.parametrize("e", [16, 17, 65])
def test_edge_many_losses(gpu, monkeypatch, e):
    """More distinct losses than the reliability table holds (2,048): the f64 rows, with both
    lvl_out* kernels and, at E = 65, level-order rows and sweep rows in one build."""
    set_form(monkeypatch, levels="1")
    g = _graph(e, many_losses=True)
    lat, rel, st = lg.build(g)
    _assert_level_build(g, st, f"many losses E={e}", table=False)
    check_tables(g, lat, rel, f"many losses E={e}")


@pytest.mark.parametrize("e", [33, 254])
def test_edge_pred_near_across_many_levels(gpu, monkeypatch, e):
    """The predecessor pre-pass (lvl_pred_near_kernel) forced past the first arc batch: buckets
    that cannot overflow (bcap=2048) and buckets of 8 entries, bit-equal to the build without it."""
    g = _graph(e)
    out = {}
    for bcap in ("-1", "2048", "8"):
        set_form(monkeypatch, levels="1", bcap=bcap)
        lat, rel, st = lg.build(g)
        assert st.dist_enc == LEVELS and st.levels == e, (bcap, st.dist_enc, st.levels)
        assert st.pred_near == max(int(bcap), 0), (bcap, st.pred_near)
        out[bcap] = (lat, rel, st)
    assert out["2048"][2].pred_near_over == 0, out["2048"][2].pred_near_over
    check_tables(g, *out["-1"][:2], f"bcap=-1 E={e}")
    for bcap in ("2048", "8"):
        assert np.array_equal(out[bcap][0], out["-1"][0]), bcap
        assert np.array_equal(out[bcap][1].view(np.uint64), out["-1"][1].view(np.uint64)), bcap


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("e", [9, 32, 254, 255])
def test_edge_virtual_ranks(gpu, monkeypatch, ranks, e):
    """Row shards with the tail in the last rank's rows (a core of 300 vertices, so that every
    rank has rows): the ranks' own sources settle at different levels -- the middle of the tail
    first -- and the per-batch vote decides. At E = 255 every rank must leave for the FW together. The stats are
    rank 0's: its own sources' last level."""
    set_form(monkeypatch, levels="1")
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    g = _graph(e, core=300)
    rows = lg.shard_rows(g.n, ranks)
    assert all(b < end for b, end in rows), rows  # no rank without rows
    lat, rel, st = lg.build(g, ngpus=1)
    if e <= 254:
        _assert_level_build(g, st, f"x{ranks} E={e}", rows=rows[0])
    else:
        assert st.dist_enc != LEVELS and st.levels == 0, (st.dist_enc, st.levels)
    check_tables(g, lat, rel, f"x{ranks} E={e}")


@pytest.mark.parametrize("e", [32, 254])
def test_edge_directed(gpu, monkeypatch, e):
    """Independent weights and losses per direction on the core's arcs and the tail's."""
    set_form(monkeypatch, levels="1")
    g = _graph(e, directed=True)
    lat, rel, st = lg.build(g)
    _assert_level_build(g, st, f"directed E={e}")
    check_tables(g, lat, rel, f"directed E={e}")


def test_edge_sub_ms_path_order(gpu, monkeypatch):
    """E = 33 quanta of 100 us: past the packed form, the f64 ms table summed in path order along
    the level pass's predecessors must be the reference's hop sums bit for bit."""
    from shadow_amd.topology import build_tables_subset
    set_form(monkeypatch, levels="1")
    g = _graph(33, quantum_ns=100_000)
    lat, rel, ms, _, st = build_tables_subset(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                              algo=ALGO_DENSE_FW, want_ms=True)
    _assert_level_build(g, st, "sub-ms E=33")
    check_tables(g, lat, rel, "sub-ms E=33")
    exp = lg.oracle_table(g)["lat_ms"]
    assert np.array_equal(ms, exp), np.argwhere(ms != exp)[:5]
