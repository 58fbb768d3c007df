"""Neighbour-row derivation (derive.hip, build.hip derive_sets and the gate in sparse_rows) on
the constructed graphs of tests/derive_graphs.py, away from the Barabasi-Albert m = 3 family of
test_gpu_derive.py: derived sources of degree 1, 2 and 4 (DV_MAXDEG's masks), a greedy independent
set over adjacent low-degree vertices, predecessor chains hundreds of hops deep (phase B's
on-demand climb), direct arcs at the largest 7-bit weight and at every one of 256 reliability
indices, tiny components, an isolated vertex, self-loops and parallel edges, and the gate's
off-side (an empty set, max_w = 128, a partial row range). Each builder asserts its property
against the oracle first (test_derive_graphs.py: no GPU), with the CPU model of the derivation.

Every case is one full table of n <= 2,000 on the workgroup kernel: against the oracle (latency
bit for bit, reliability within 1e-12, unreachable pairs as the oracle marks them, the diagonal
included), the form from srt_build_stats (n_derived equal to the Python restatement of
derive_sets), and against the same build with SRT_FORM derive=0: latency equal, reliability
bitwise equal, the tied-pair count equal."""
import numpy as np
import pytest
from conftest import set_form

import derive_graphs as dg
import level_graphs as lg
from shadow_amd._lib import ALGO_SPARSE_SSSP, SRT_INF, BuildStats
from shadow_amd.topology import SparseGraph

pytestmark = pytest.mark.gpu
DERIVED = 64  # srt_build_stats.fw_block bit of a build with derived rows


def _build(g, what):
    """The full sparse table of g, checked against the oracle -> (lat, rel, stats); the figures a
    failure report needs are printed first."""
    lat, rel, st = lg.build(g, ALGO_SPARSE_SSSP, count_ties=1)
    print(f"{what}: {dg.describe(g)} dist_enc={st.dist_enc} fw_block={st.fw_block} "
          f"ess_arcs={st.ess_arcs} n_derived={st.n_derived} tied_pairs={st.tied_pairs}")
    lg.check_tables(g, lat, rel, what)
    return lat, rel, st


def _derived_and_all_kernel(g, monkeypatch, what):
    set_form(monkeypatch, kernel="wg", derive=1)
    lat, rel, st = _build(g, what)
    assert st.dist_enc == 2 and st.fw_block & 7 == 7 and st.fw_block & DERIVED, \
        (st.dist_enc, st.fw_block)
    assert st.ess_arcs == 0
    assert st.n_derived == g.nI, (st.n_derived, g.nI)  # the device's set is the restated one
    set_form(monkeypatch, derive=0)
    lat0, rel0, st0 = _build(g, what + " derive=0")
    assert not st0.fw_block & DERIVED and st0.n_derived == 0, (st0.fw_block, st0.n_derived)
    assert np.array_equal(lat, lat0)
    bad = np.argwhere(rel.view(np.uint64) != rel0.view(np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} reliabilities differ from the all-kernel build's, " \
                          f"first {bad[:5].tolist()}"
    assert st.tied_pairs == st0.tied_pairs, (st.tied_pairs, st0.tied_pairs)
    return lat, rel


@pytest.mark.parametrize("name", list(dg.CASES))
def test_derived_rows_on_constructed_graph(gpu, monkeypatch, name):
    """grid_w1..3: degrees 2 / 3 / 4 in I, 1,043 low-degree core vertices, trees 88 hops deep,
    96% / 32% / 23% of the pairs tied. ring1000: degree 2, chains 500 hops deep, every antipode
    tied; ring601_w2: no tie, two adjacent core vertices. ba_m1 / m2 / m4: degree 1 / 2 / 4.
    pendants127: 300 degree-1 sources whose direct arc weighs 127, the 7-bit field's largest.
    pendant_losses: every reliability index 0..255 on a direct arc. islands: components of 1, 2, 3
    and 7 vertices beside the probe's, self-loops and parallel edges at members of I."""
    g = dg.CASES[name]()
    lat, rel = _derived_and_all_kernel(g, monkeypatch, name)
    if name == "islands":
        inf_ns = np.uint64(SRT_INF * lg.MS)
        apart = g.comp[:, None] != g.comp[None, :]
        assert (lat[apart] == inf_ns).all() and (rel[apart] == 0.0).all()
        same = ~apart & ~np.eye(g.n, dtype=bool)  # (the diagonal rule: check_tables, above)
        assert (lat[same] < inf_ns).all() and (rel[same] > 0.0).all()
        h, others = g.head, np.arange(g.n) != g.head  # the isolated vertex
        assert (lat[h, others] == inf_ns).all() and (rel[h, others] == 0.0).all()
        assert (lat[others, h] == inf_ns).all() and (rel[others, h] == 0.0).all()


@pytest.mark.parametrize("name", list(dg.OFF_CASES))
def test_derivation_switches_off(gpu, monkeypatch, name):
    """ba_m5: every degree is >= 5, the independent set is empty. pendants128: the largest arc
    weight is one past the compact arcs' 7 bits (16-byte arcs, no codes). The build takes the
    kernel for every row, without an error, and the table is the oracle's."""
    set_form(monkeypatch, kernel="wg", derive=1)
    g = dg.OFF_CASES[name]()
    _, _, st = _build(g, name)
    assert st.dist_enc == 2 and st.ess_arcs == 0 and st.fw_block & 4, (st.dist_enc, st.fw_block)
    assert not st.fw_block & DERIVED and st.n_derived == 0, (st.fw_block, st.n_derived)
    if name == "ba_m5":
        assert g.nI == 0 and st.fw_block & 7 == 7, st.fw_block
    else:
        assert g.nI > 0 and st.fw_block & 2 == 0, st.fw_block


def test_partial_row_range_is_not_derived(gpu, monkeypatch):
    """grid(40, 50, 2) through srt_sparse_graph_rows: rows [0, n) are derived; [1, n) and
    [0, n - 1) are not (a derived row needs every neighbour's row in the call), and hold
    bitwise what the same rows of the full derived table hold."""
    import torch
    set_form(monkeypatch, kernel="wg", derive=1)
    g = dg.grid(40, 50, 2)
    n = g.n
    sg = SparseGraph(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    assert sg.quantum_ns == lg.MS
    try:
        def rows(s0, s1):
            st = BuildStats()
            lat = torch.empty((s1 - s0, n), dtype=torch.int32, device="cuda")
            rel = torch.empty((s1 - s0, n), dtype=torch.float64, device="cuda")
            sg.rows(s0, s1, lat.data_ptr(), rel.data_ptr(), None, st)
            torch.cuda.synchronize()
            print(f"grid_w2 rows [{s0}, {s1}): dist_enc={st.dist_enc} fw_block={st.fw_block} "
                  f"ess_arcs={st.ess_arcs} n_derived={st.n_derived}")
            assert st.dist_enc == 2 and st.fw_block & 7 == 7 and st.ess_arcs == 0
            return lat, rel.view(torch.int64), st
        lat, rel, st = rows(0, n)
        assert st.fw_block & DERIVED and st.n_derived == g.nI, (st.fw_block, st.n_derived)
        lg.check_tables(g, lat.cpu().numpy().view(np.uint32).astype(np.uint64) * np.uint64(lg.MS),
                        rel.view(torch.float64).cpu().numpy(), "grid_w2 rows [0, n)")
        for s0, s1 in [(1, n), (0, n - 1)]:
            lat1, rel1, st1 = rows(s0, s1)
            assert not st1.fw_block & DERIVED and st1.n_derived == 0, (st1.fw_block, st1.n_derived)
            assert torch.equal(lat1, lat[s0:s1]) and torch.equal(rel1, rel[s0:s1]), (s0, s1)
    finally:
        sg.free()
