"""The fixtures of test_gpu_rel_forms.py (tests/rel_graphs.py) at the parameters the GPU tests use,
on the CPU: every constructor classifies its rows with the oracle (distance range, parent count,
the kernel the hand-over rules assign) and asserts what its case is about, so a graph that misses
its cap or its range fails here, before any build runs on it."""
import numpy as np
import pytest

import level_graphs as lg
import rel_graphs as rg


def test_cap_formulas_at_the_sizes_the_cases_name():
    assert [rg.tree_cap(n) for n in (1024, 1025, 4096, 4097)] == [1024, 4096, 4096, 7168]
    assert rg.tree_cap(4097, packed=True) == 8192
    assert rg.deep_cap(261) == 256 and rg.deep_cap(11419) == 11072 and rg.deep_cap(7299) == 7296
    assert rg.pk_cap(181, 300) == 128 and rg.pk_cap(6965, 300) == 6464
    assert [rg.pk_width(n) for n in (2048, 2049, 4096, 4097, 6965)] == [1, 2, 2, 4, 4]


def test_stage_rules_on_either_side_of_every_bound():
    s = rg.stage_of
    assert s(rg.FW, 7299, 64, 7168) == rg.TREE and s(rg.FW, 7299, 65, 7168) == rg.DEEP
    assert s(rg.FW, 7299, 64, 7169) == rg.DEEP and s(rg.FW, 261, 100, 257) == rg.ORDER
    assert s(rg.FW, 261, 1023, 256) == rg.DEEP and s(rg.FW, 261, 1024, 256) == rg.SWEEPS
    assert s(rg.FW, 261, 1023, 257) == rg.ORDER and s(rg.FW, 261, 1024, 257) == rg.SWEEPS
    assert s(rg.FW_LEVELS, 261, 64, 999) == rg.LEVELS and s(rg.FW_LEVELS, 261, 65, 1) == rg.SWEEPS
    assert s(rg.ROWS, 261, 64, 250) == rg.TREE and s(rg.ROWS, 261, 65, 250) == rg.SWEEPS
    assert s(rg.LV_PK, 181, 30, 128, 300) == rg.PK and s(rg.LV_PK, 181, 30, 129, 300) == rg.SWEEPS
    for path, n, cap in ((rg.LV_TREE_PK, 8507, 8192), (rg.LV_TREE_16, 7425, 7168)):
        assert s(path, n, 64, cap) == rg.TREE and s(path, n, 64, cap + 1) == rg.SWEEPS
        assert s(path, n, 65, cap) == rg.SWEEPS


def test_row_facts_agree_with_the_oracle_table(native):
    """The range is level_graphs' row eccentricity; the parents are the distinct predecessors."""
    g = rg.f4_deep_cap_small()
    mx, par = rg.row_facts(g)
    assert np.array_equal(mx, lg.row_eccentricity(g))
    some = [0, 1, 64, 65, 130, 260]
    m2, p2 = rg.row_facts(g, some)
    assert np.array_equal(m2, mx[some]) and np.array_equal(p2, par[some])
    lat, rel = rg.self_pair(g, 65)
    exp = lg.oracle_table(g)
    assert lat == int(exp["lat_int"][65, 65]) and rel == exp["rel"][65, 65]


@pytest.mark.parametrize("ecc0", [64, 65])
@pytest.mark.parametrize("n", list(rg.F1_SHAPES))
def test_f1_range(native, n, ecc0):
    g = rg.f1_range(n, ecc0)
    assert g.n == n and lg.quantum(g) == rg.MS


def test_f2_caterpillar(native):
    g = rg.f2_caterpillar()
    mx, par, st = rg.classify(g, rg.FW)
    for (stage, m, p), row in g.named.items():
        assert (st[row], mx[row], par[row]) == (stage, m, p)
    assert {rg.DEEP, rg.ORDER, rg.SWEEPS} == set(st)
    assert len(np.unique(lg.oracle_table(g)["lat_int"][g.named[(rg.DEEP, 1023, 1152)]])) > 900


@pytest.mark.parametrize("over", [0, 1])
def test_f3_tree_cap(native, over):
    g = rg.f3_tree_cap(over)
    assert 4096 < g.n <= 7500


def test_f4_deep_cap(native):
    assert rg.f4_deep_cap_small().n == 261
    g = rg.f4_deep_cap_large()
    # the kernel's LDS request at this cap: all of the 160 KB less the 1 KB it leaves free
    assert 159 * 1024 - 14 < 8 * (rg.ld_of(g.n) >> 5) + 4096 + 14 * (rg.deep_cap(g.n) + 63) \
        and 8 * (rg.ld_of(g.n) >> 5) + 4096 + 14 * rg.deep_cap(g.n) <= 159 * 1024


@pytest.mark.parametrize("n", list(rg.F5_SHAPES))
def test_f5_border(native, n):
    assert rg.f5_border(n).n == n


def test_f6_mixed(native):
    g = rg.f6_mixed()
    mx, _ = rg.row_facts(g)
    assert mx[0] == 48 and (mx <= 64).sum() >= 100 and (mx > 64).sum() >= 100


def test_f8_last_shard_holds_every_stage(native):
    g = rg.f8_disjoint()
    for ranks in (2, 3):
        b = lg.shard_rows(g.n, ranks)[-1][0]
        assert 0 < b <= g.off
        assert {rg.TREE, rg.DEEP, rg.ORDER, rg.SWEEPS} == set(rg.classify(g, rg.FW)[2][b:])
        assert {rg.LEVELS, rg.SWEEPS} == set(rg.classify(g, rg.FW_LEVELS)[2][b:])


def test_f8_disjoint(native):
    g = rg.f8_disjoint()
    _, _, st = rg.classify(g, rg.FW)
    assert {rg.TREE, rg.DEEP, rg.ORDER, rg.SWEEPS} == set(st)
    d = lg.oracle_table(g)["lat_int"]
    assert ((d == lg.U64_MAX).sum(axis=1) > 0).all()


@pytest.mark.parametrize("parents", list(rg.L1_SHAPES))
def test_l1_pk_cap_small(native, parents):
    g = rg.l1_pk_cap_small(parents)
    assert lg.largest_distance(g) == g.E <= 31


def test_l2_pk_cap_formula(native):
    assert rg.l2_pk_cap_formula().E <= 31


@pytest.mark.parametrize("n", list(rg.L3_SHAPES))
def test_l3_pk_width(native, n):
    g = rg.l3_pk_width(n)
    # no tree of n vertices and diameter <= 31 has more than n - (n - 1) / 15 inner vertices: the
    # cap (n & ~63 here) is out of every row's reach at these sizes
    assert g.n - (g.n - 1) // 15 <= rg.pk_cap(g.n, rg.distinct_rel(g))


@pytest.mark.parametrize("many_losses", [False, True])
@pytest.mark.parametrize("over", [0, 1])
def test_l4_tree_cap(native, over, many_losses):
    assert 32 <= rg.l4_tree_cap(over, many_losses).E <= 64
