"""The dense builds' path-order reliability pass, rel(s,t) = rel(s,pred) * r(pred,t), at the
hand-overs of its kernel chain (shadow_amd/csrc/dense.hip), with trees whose rows sit on either
side of every bound: the parent counts and distance ranges are exact and oracle-checked
(tests/rel_graphs.py, whose classify() restates the rules and names the kernel of every row).

The chains: after Floyd-Warshall, rel_tree_kernel (range <= 64 and parents <= 1024 | 4096 | 7168
by n's size class), rel_deep_kernel (range <= 1023, parents <= its LDS cap), rel_order_kernel
(range <= 1023), rel_sweeps_kernel; under SRT_FORM reltree=0, rel_levels_kernel (range <= 64) and
the sweeps. After a level build, rel_pk_kernel<K> (E <= 31; parents <= its LDS cap) or
rel_tree_kernel on the u8 level rows (packed words: 8192 slots above n = 4096; int16 predecessors
when the reliabilities outnumber the table: 7168), each followed by the sweeps. With a source list
(few attached rows), tree or levels and the sweeps alone.

Every case (1) holds the whole table to the CPU oracle, diagonal included -- latency bit-exact,
reliability within 1e-12 relative; above n = 8,000 the named rows and 40 others through
oracle.sssp_list --, (2) compares every entry bit for bit with a second form that forms the same
left-to-right product (Floyd-Warshall cases: the same build under reltree=0; level cases: the same
graph by Floyd-Warshall), so no pair is left out where the oracle is sampled, and (3) asserts with
the CPU classification that the rows it names end in the kernel it means.

L3 as arithmetic allows it: a graph of diameter <= 31 has at least (n - 1) / 15 path ends, so no
row holds more than n - (n - 1) / 15 parents, and rel_pk_kernel's cap is n & ~63 up to n = 6,582:
from n = 945 on no row of a packed-level build passes the cap until the LDS formula binds it. At
ld = 2048 .. 4224 every row therefore takes rel_pk_kernel<K>; the sweeps read K-wide rows at
K = 1 (L1) and K = 4 (L2).

Out of scope: n > 32768 (rel_levels_kernel<1024, 65536>, srt_rel_sweeps_rows of tables.hip),
n = 65535 for the deep and order stages, real multi-GPU ranks (virtual ranks stand in), and the
sparse builds' reliability."""
import numpy as np
import pytest
from conftest import form_env

import level_graphs as lg
import oracle
import rel_graphs as rg
from level_graphs import LEVELS, REL_TOL, check_tables
from shadow_amd._lib import ALGO_DENSE_FW, SRT_INF
from shadow_amd.topology import build_tables_subset

pytestmark = pytest.mark.gpu

FW_ENCS = {1, 2, 3, 4, 5, 6, 7, 8, 9, 11}  # srt_device.h: every Floyd-Warshall tier's dist_enc
ROWS_ENC = 10
FULL_ORACLE_MAX = 8000


def _clean(monkeypatch, ranks=None):
    monkeypatch.delenv("SRT_FORM", raising=False)
    monkeypatch.delenv("SRT_VIRTUAL_RANKS", raising=False)
    if ranks:
        monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))


def _same_bits(g, a, b, what):
    """Every entry of two builds' tables, f64 as bits; the first differing pair in the message."""
    (lat_a, rel_a), (lat_b, rel_b) = a, b
    assert lat_a.shape == rel_a.shape == lat_b.shape == rel_b.shape == (g.n, g.n), what
    ne = lat_a != lat_b
    assert not ne.any(), f"{what}: latency differs at {np.argwhere(ne)[0].tolist()}"
    ne = rel_a.view(np.uint64) != rel_b.view(np.uint64)
    if ne.any():
        s, t = np.argwhere(ne)[0].tolist()
        raise AssertionError(f"{what}: {int(ne.sum())} reliabilities differ, first ({s}, {t}): "
                             f"{rel_a[s, t]!r} != {rel_b[s, t]!r}")


def _check_oracle(g, lat, rel, what, named=(), reachable_only=False):
    if g.n <= FULL_ORACLE_MAX:
        check_tables(g, lat, rel, what, reachable_only=reachable_only)
        if g.n > 4200:
            g._exp = None  # 2 GB a graph: not kept for the session
        return
    rows = np.unique(np.concatenate([np.asarray(named, np.int64),
                                     np.linspace(0, g.n - 1, 40).astype(np.int64)]))
    exp = oracle.sssp_list(rg.edge_list(g), rows, nthreads=8)
    exp_lat, exp_rel = exp["lat_int"], exp["rel"]
    for i, v in enumerate(rows):
        exp_lat[i, v], exp_rel[i, v] = rg.self_pair(g, int(v))
    bad = np.argwhere(lg.unreached_as_oracle(lat[rows], g) != exp_lat)
    assert bad.size == 0, f"{what}: latency mismatches, first (row, t) {rows[bad[0][0]], bad[0][1]}"
    err = np.abs(rel[rows] - exp_rel) / np.maximum(np.abs(exp_rel), 1e-300)
    i, t = np.unravel_index(err.argmax(), err.shape)
    assert float(err.max()) <= REL_TOL, f"{what}: max rel error {err.max()} at ({rows[i]}, {t})"


def _expect(g, path, stages):
    """The CPU classification of the named rows: {row: stage}."""
    rows = sorted(stages)
    mx, par, st = rg.classify(g, path, rows)
    got = dict(zip(rows, st))
    assert got == stages, (g.name, path, got, stages, mx.tolist(), par.tolist())


def _fw_forms(g, monkeypatch, what, named=(), ranks=None, reachable_only=False):
    """Forced Floyd-Warshall under reltree=1 and reltree=0: both Floyd-Warshall encodings, bit
    for bit the same table, held to the oracle."""
    _clean(monkeypatch, ranks)
    out = []
    for reltree in ("1", "0"):
        with form_env(levels="0", reltree=reltree):
            lat, rel, st = lg.build(g, ALGO_DENSE_FW, ngpus=1 if ranks else None)
        assert st.dist_enc in FW_ENCS and st.levels == 0, (what, reltree, st.dist_enc, st.levels)
        out.append((lat, rel))
        print(f"{what} reltree={reltree}: n={g.n} dist_enc={st.dist_enc} max_depth={st.max_depth}")
    _same_bits(g, out[0], out[1], f"{what}: reltree=1 | reltree=0")
    del out[1]
    _check_oracle(g, *out[0], what, named, reachable_only)
    return out[0]


def _level_forms(g, monkeypatch, what, table=True):
    """A forced level build, then the same graph by Floyd-Warshall: bit for bit the same table."""
    _clean(monkeypatch)
    with form_env(levels="1"):
        lat, rel, st = lg.build(g, ALGO_DENSE_FW)
    assert st.dist_enc == LEVELS and st.levels == max(g.E, 2), (what, st.dist_enc, st.levels, g.E)
    assert st.rel_table == (rg.distinct_rel(g) if table else 0), (what, st.rel_table)
    print(f"{what} levels: n={g.n} E={g.E} rel_table={st.rel_table} max_depth={st.max_depth}")
    with form_env(levels="0"):
        lat0, rel0, st0 = lg.build(g, ALGO_DENSE_FW)
    assert st0.dist_enc in FW_ENCS and st0.levels == 0, (what, st0.dist_enc)
    _same_bits(g, (lat, rel), (lat0, rel0), f"{what}: levels | Floyd-Warshall")
    del lat0, rel0
    _check_oracle(g, lat, rel, what, named=[0, int(g.ends[0]), int(g.ends[-1])])
    return st


# --- Floyd-Warshall chain ---------------------------------------------------------------------

@pytest.mark.parametrize("ecc0", [64, 65])
@pytest.mark.parametrize("n", list(rg.F1_SHAPES))
def test_f1_range_64_tree_65_deep(gpu, monkeypatch, n, ecc0):
    """Row 0 spans 64 | 65 quanta at n = 261, 1025 and 4097 (each size class of rel_tree_kernel):
    the tree's last pass, or the hand-over to rel_deep_kernel (to the sweeps under reltree=0)."""
    g = rg.f1_range(n, ecc0)
    _expect(g, rg.FW, {0: rg.TREE if ecc0 == 64 else rg.DEEP, 1: rg.DEEP})
    _expect(g, rg.FW_LEVELS, {0: rg.LEVELS if ecc0 == 64 else rg.SWEEPS})
    _fw_forms(g, monkeypatch, f"F1 n={n} range {ecc0}")


def test_f2_range_1023_deep_order_1024_sweeps(gpu, monkeypatch):
    """A caterpillar at n = 1193: rows spanning 1023 quanta take rel_deep_kernel (1152 parents, its
    cap) or rel_order_kernel (1153), rows spanning 1024 the sweeps -- the last bucket of both
    counting sorts."""
    g = rg.f2_caterpillar()
    _expect(g, rg.FW, {row: stage for (stage, _, _), row in g.named.items()})
    assert len(set(g.named.values())) == 4
    _fw_forms(g, monkeypatch, "F2 caterpillar")


@pytest.mark.parametrize("over", [0, 1])
def test_f3_tree_cap_7168(gpu, monkeypatch, over):
    """Row 0 within 64 quanta with 7168 | 7169 parents at n = 7297 | 7299: every slot of
    rel_tree_kernel<1024, 32> filled, or the hand-over to rel_deep_kernel (cap 7296 here)."""
    g = rg.f3_tree_cap(over)
    _expect(g, rg.FW, {0: rg.DEEP if over else rg.TREE, int(g.ends[0]): rg.DEEP})
    _fw_forms(g, monkeypatch, f"F3 parents {7168 + over}")


def test_f4_deep_cap_where_n_binds(gpu, monkeypatch):
    """n = 261: rows with 256 parents (rel_deep_kernel's cap, every slot) and with 257
    (rel_order_kernel), ranges in [65, 1023]."""
    g = rg.f4_deep_cap_small()
    _expect(g, rg.FW, {0: rg.DEEP, 1: rg.DEEP, int(g.ends[0]): rg.ORDER, g.n - 1: rg.ORDER})
    _fw_forms(g, monkeypatch, "F4 n=261")


def test_f4_deep_cap_where_lds_binds(gpu, monkeypatch):
    """n = 11,419: rel_deep_kernel's LDS formula gives 11,072 slots (its request of 159 KB is the
    largest it makes); rows with exactly as many parents, and with one more (rel_order_kernel).
    Both forms' whole tables come to the host and are compared there; the oracle is sampled."""
    g = rg.f4_deep_cap_large()
    named = {0: rg.DEEP, 17: rg.DEEP, int(g.ends[0]): rg.ORDER, int(g.ends[-1]): rg.ORDER}
    _expect(g, rg.FW, named)
    _fw_forms(g, monkeypatch, "F4 n=11419", named=list(named))


@pytest.mark.parametrize("n", list(rg.F5_SHAPES))
def test_f5_size_class_borders(gpu, monkeypatch, n):
    """n = 1024 | 1025 | 4096 | 4097: the last target index of a size class (tid + i * NT = n - 1)
    and the buffer descriptors' bound, in rel_tree_kernel and (reltree=0) rel_levels_kernel; row 0
    within 64 quanta, the last vertex's row past it."""
    g = rg.f5_border(n)
    _expect(g, rg.FW, {0: rg.TREE, n - 1: rg.DEEP})
    _expect(g, rg.FW_LEVELS, {0: rg.LEVELS, n - 1: rg.SWEEPS})
    _fw_forms(g, monkeypatch, f"F5 n={n}")


def _source_list(g, must, count):
    """Exactly `count` increasing vertices: `must` and others spread over the rest of the graph."""
    rest = np.setdiff1d(np.arange(g.n), must)
    pick = rest[np.linspace(0, len(rest) - 1, count - len(must)).astype(np.int64)]
    verts = np.unique(np.concatenate([np.asarray(must, np.int64), pick])).astype(np.int32)
    assert len(verts) == count and set(must) <= set(verts.tolist()), (len(verts), count)
    return verts


@pytest.mark.parametrize("which", ["f2", "f4", "f1", "mixed"])
def test_f6_source_list(gpu, monkeypatch, which):
    """The few-rows build (no deep or order stage: rel_tree_kernel, or rel_levels_kernel under
    reltree=0, with a source list, then the sweeps) on the F2 and F4 graphs, F1's range-64 one and
    a spider whose attached rows lie on both sides of 64 quanta, several on each: the two forms'
    rows bit for bit the same, and bit for bit the full table's. The build takes at most n / 12
    sources: 40 at n = 1193, 21 at n = 261."""
    g = {"f2": rg.f2_caterpillar, "f4": rg.f4_deep_cap_small,
         "f1": lambda: rg.f1_range(261, 64), "mixed": rg.f6_mixed}[which]()
    must = sorted(g.named.values()) if which == "f2" else [0, int(g.ends[0])]
    verts = _source_list(g, must, min(40, g.n // 12))
    assert len(verts) * 12 <= g.n < (len(verts) + 1) * 12 or len(verts) == 40
    for path, short in ((rg.ROWS, rg.TREE), (rg.FW_LEVELS, rg.LEVELS)):
        _, _, st = rg.classify(g, path, verts)
        want = {"f2": 0, "f4": 0, "f1": 1}.get(which)
        assert st.count(short) == want if want is not None else st.count(short) >= 5, (path, st)
        assert st.count(rg.SWEEPS) >= 5, (path, st)
    _clean(monkeypatch)
    sub = np.ix_(verts, verts)
    with form_env(levels="0"):
        full_lat, full_rel, fst = lg.build(g, ALGO_DENSE_FW)
    assert fst.dist_enc in FW_ENCS, fst.dist_enc
    check_tables(g, full_lat, full_rel, f"F6 {which} full")
    out = []
    for reltree in ("1", "0"):
        with form_env(levels="0", reltree=reltree):
            lat, rel, _, _, st = build_tables_subset(g.n, g.directed, g.src, g.dst, g.lat_ns,
                                                     g.loss, verts=verts, algo=ALGO_DENSE_FW)
        assert st.dist_enc == ROWS_ENC, (reltree, st.dist_enc)  # the rows build ran
        assert lat.shape == rel.shape == (len(verts), len(verts))
        assert np.array_equal(lat, full_lat[sub]), (reltree, np.argwhere(lat != full_lat[sub])[:5])
        ne = rel.view(np.uint64) != full_rel[sub].view(np.uint64)
        assert not ne.any(), (reltree, np.argwhere(ne)[:5], verts)
        out.append(rel)
    assert np.array_equal(out[0].view(np.uint64), out[1].view(np.uint64))


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("which", ["f1_64", "f1_65", "f4", "f8"])
def test_f7_virtual_ranks(gpu, monkeypatch, which, ranks):
    """Row shards of the n = 261 graphs of F1 and F4 and of F8's two spiders (n = 317), whose last
    rank holds rows that end in every kernel of the chain: row0 != 0 where rel_tree_kernel,
    rel_levels_kernel, rel_deep_kernel, rel_order_kernel and the sweeps each finish rows."""
    g = {"f1_64": lambda: rg.f1_range(261, 64), "f1_65": lambda: rg.f1_range(261, 65),
         "f4": rg.f4_deep_cap_small, "f8": rg.f8_disjoint}[which]()
    rows = lg.shard_rows(g.n, ranks)
    assert all(b < e for b, e in rows) and rows[-1][0] > 0, rows
    b = rows[-1][0]
    last = g.n - 1  # a path's end in the last rank's rows
    if which == "f8":
        _, _, st = rg.classify(g, rg.FW)
        assert {rg.TREE, rg.DEEP, rg.ORDER, rg.SWEEPS} == set(st[b:]), (b, set(st[b:]))
        _, _, st = rg.classify(g, rg.FW_LEVELS)
        assert {rg.LEVELS, rg.SWEEPS} == set(st[b:]), (b, set(st[b:]))
    else:
        _expect(g, rg.FW, {last: rg.ORDER if which == "f4" else rg.DEEP})
    _fw_forms(g, monkeypatch, f"F7 {which} x{ranks}", ranks=ranks, reachable_only=which == "f8")


def test_f8_unreachable_targets_in_every_stage(gpu, monkeypatch):
    """Two disjoint spiders, n = 317: every row has targets without a path (x >= SRT_INF, p < 0),
    and the rows end in the tree, the deep, the order and the sweeps kernel. A pair without a path
    holds SRT_INF and, as in the oracle, the reliability 0."""
    g = rg.f8_disjoint()
    _expect(g, rg.FW, dict(zip(g.named, [rg.DEEP, rg.ORDER, rg.SWEEPS, rg.TREE])))
    lat, rel = _fw_forms(g, monkeypatch, "F8 disjoint", reachable_only=True)
    exp = lg.oracle_table(g)
    unreached = exp["lat_int"] == lg.U64_MAX
    assert unreached.any(axis=1).all() and (exp["rel"][unreached] == 0.0).all()
    assert (lat[unreached] == np.uint64(SRT_INF * lg.quantum(g))).all()
    print("F8 reliabilities of pairs without a path:", np.unique(rel[unreached])[:8])
    assert (rel[unreached] == 0.0).all(), np.unique(rel[unreached])[:8]


# --- level build ------------------------------------------------------------------------------

@pytest.mark.parametrize("parents", list(rg.L1_SHAPES))
def test_l1_pk_cap_where_n_binds(gpu, monkeypatch, parents):
    """E = 30, cap 128 (n = 181 | 145 | 147): row 0 with 168 parents (every row to the sweeps),
    with exactly 128 (rel_pk_kernel, every slot) and with 129."""
    g = rg.l1_pk_cap_small(parents)
    _expect(g, rg.LV_PK, {0: rg.PK if parents == 128 else rg.SWEEPS, int(g.ends[0]): rg.SWEEPS})
    _level_forms(g, monkeypatch, f"L1 parents {parents}")


def test_l2_pk_cap_where_lds_binds(gpu, monkeypatch):
    """E = 30 at n = 6,965 (K = 4): the cap from rel_pk_launch's formula with the build's own
    table size is the graph's 6,464; row 0 fills it, the path ends' rows pass it by one."""
    g = rg.l2_pk_cap_formula()
    _expect(g, rg.LV_PK, {0: rg.PK, 1: rg.PK, int(g.ends[0]): rg.SWEEPS, g.n - 1: rg.SWEEPS})
    st = _level_forms(g, monkeypatch, "L2")
    assert rg.pk_cap(g.n, st.rel_table) == g.parents0 == 6464, (st.rel_table, g.parents0)


@pytest.mark.parametrize("n", list(rg.L3_SHAPES))
def test_l3_pk_row_widths(gpu, monkeypatch, n):
    """n = ld = 2048 (K = 1) | 2176 (K = 2) | 4096 (K = 2) | 4224 (K = 4): the row's last 16-byte
    piece holds real targets up to the last lane."""
    g = rg.l3_pk_width(n)
    _expect(g, rg.LV_PK, {0: rg.PK, n - 1: rg.PK})
    _level_forms(g, monkeypatch, f"L3 n={n}")


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("many_losses", [False, True])
def test_l4_tree_on_level_rows(gpu, monkeypatch, many_losses, over):
    """E = 64 above n = 4096: the u8 level rows with packed words (8192 slots: row 0 with 8192 |
    8193 parents, n = 8,507 | 8,509) or, past 2,048 distinct reliabilities, int16 predecessors
    (7168 slots: 7168 | 7169 parents, n = 7,425 | 7,427; no table)."""
    g = rg.l4_tree_cap(over, many_losses)
    path = rg.LV_TREE_16 if many_losses else rg.LV_TREE_PK
    _expect(g, path, {0: rg.SWEEPS if over else rg.TREE, int(g.ends[0]): rg.SWEEPS})
    _level_forms(g, monkeypatch, f"L4 many_losses={many_losses} over={over}", table=not many_losses)
