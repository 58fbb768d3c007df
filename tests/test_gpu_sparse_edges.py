"""The sparse SSSP kernels (wsssp.hip, msssp.hip, sparse.hip, derive.hip) at their packing and
range edges, on the constructed graphs of tests/sparse_graphs.py (each asserts its own property
against the oracle or srt_canon_build before it is handed out; test_sparse_graphs.py runs those
assertions without a GPU).

Every case compares with the CPU oracle: latency bit-exact in integer ns (an unreachable pair is
SRT_INF quanta in the tables, UINT64_MAX in the oracle), reliability within 1e-12 relative -- the
whole table where n <= ~4,100, else sampled rows of srt_sparse_graph_rows against
oracle.sssp_rows off the diagonal. Every case also asserts the form it means to test from
srt_build_stats: dist_enc (1 wave, 2 workgroup, 3 multi-source kernel), fw_block (1 LDS row /
original order, 2 relabelled reliability / compact arcs, 4 workgroup, 8 multi-source, 16 u16 rows,
64 derived), ess_arcs (sources recomputed after a flag) and n_derived. The block kernel documents
no form: there the tables alone are asserted.
"""
import numpy as np
import pytest
from conftest import set_form

import level_graphs as lg
import oracle
import sparse_graphs as sgr
from shadow_amd import _lib, graphs
from shadow_amd._lib import ALGO_SPARSE_SSSP, SRT_INF, BuildStats
from shadow_amd.topology import SparseGraph

pytestmark = pytest.mark.gpu
REL_TOL = lg.REL_TOL
WG_INF = 1023  # wsssp.hip: the workgroup kernel's 10-bit code of an unreached vertex


def _table(g, what):
    """The full sparse build of g -> stats, after the whole table is checked against the oracle
    (the figures a failure report needs are printed first)."""
    lat, rel, st = lg.build(g, ALGO_SPARSE_SSSP)
    print(f"{what}: n={g.n} dist_enc={st.dist_enc} fw_block={st.fw_block} ess_arcs={st.ess_arcs} "
          f"n_derived={st.n_derived}")
    lg.check_tables(g, lat, rel, what)
    return lat, rel, st


def _rows(g, ranges, torch, what):
    """Row ranges of srt_sparse_graph_rows against oracle.sssp_rows, off the diagonal -> the
    stats of every range."""
    sg = SparseGraph(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    assert sg.quantum_ns == lg.MS
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    out = []
    try:
        for s0, s1 in ranges:
            st = BuildStats()
            lat = torch.empty((s1 - s0, g.n), dtype=torch.int32, device="cuda")
            rel = torch.empty((s1 - s0, g.n), dtype=torch.float64, device="cuda")
            sg.rows(s0, s1, lat.data_ptr(), rel.data_ptr(), None, st)
            torch.cuda.synchronize()
            print(f"{what} rows [{s0}, {s1}): dist_enc={st.dist_enc} fw_block={st.fw_block} "
                  f"ess_arcs={st.ess_arcs}")
            lat = lat.cpu().numpy().view(np.uint32).astype(np.uint64) * np.uint64(sg.quantum_ns)
            lat = lg.unreached_as_oracle(lat, g)
            rel = rel.cpu().numpy()
            exp = oracle.sssp_rows(el, s0, s1, nthreads=8)
            off = np.arange(g.n)[None, :] != np.arange(s0, s1)[:, None]
            bad = np.argwhere((lat != exp["lat_int"]) & off)
            assert bad.size == 0, f"{what} [{s0}, {s1}): {len(bad)} latency mismatches, " \
                                  f"first (row - {s0}, t) {bad[:5].tolist()}"
            err = np.abs(rel - exp["rel"]) / np.maximum(np.abs(exp["rel"]), 1e-300)
            assert float(err[off].max()) <= REL_TOL, (what, s0, s1, float(err[off].max()))
            out.append(st)
    finally:
        sg.free()
    return out


# ------------------------------------------------------------------------------------------------
# a. the workgroup kernel's 10-bit distance field, with the probe blind to a component
@pytest.mark.parametrize("arcs", ["compact_derive", "compact", "wide"])
@pytest.mark.parametrize("target", [1022, 1023, 1024])
def test_workgroup_packed_row_second_component_past_10_bits(gpu, monkeypatch, target, arcs):
    """two_part(E): vertex 0, the probe source, sits in a component of small eccentricity
    (2 ecc(0) <= 1022: the workgroup kernel is taken), the other component's largest distance is
    E. A distance of 1023 quanta and more does not fit the packed row: the kernel must flag such a
    source (its output pass finds a vertex left unreached beside a reached one), and the caller
    recomputes it. Flags on rows that would have fitted are allowed (the fallback is exact),
    missed ones are not: #(rows with ecc >= 1023) <= ess_arcs <= #(rows with ecc >= 1023 - max_w)
    -- a candidate of 1023 needs a settled vertex within max_w of it, and buckets hold n entries
    (no overflow). With derivation on, an overflowed core row sends the independent set's rows to
    the kernel. (The kernel's only guard used to sit inside `nd < du`, with du a 10-bit field, so
    it never ran: at E = 1023 the build returned SRT_INF / 0.0 with ess_arcs == 0 for 108 pairs,
    the first (301, 2380), and derived 1,163 rows from such core rows.)"""
    set_form(monkeypatch, kernel="wg", derive=1 if arcs == "compact_derive" else 0)
    g = sgr.two_part(target, 300 if arcs == "wide" else 200)
    max_w = sgr.max_arc_weight(g)
    lo = int((g.ecc >= WG_INF).sum())
    hi = int((g.ecc >= WG_INF - max_w).sum())
    what = f"two_part({target}, {arcs})"
    print(f"{what}: rows past the field {lo}, rows within max_w={max_w} of it {hi}")
    lat, rel, st = _table(g, what)
    h, inf_ns = g.head, np.uint64(SRT_INF * lg.MS)
    assert (lat[:h, h:] == inf_ns).all() and (lat[h:, :h] == inf_ns).all()
    assert (rel[:h, h:] == 0.0).all() and (rel[h:, :h] == 0.0).all()
    assert (lat[h:, h:] < inf_ns).all() and (rel[h:, h:] > 0.0).all()
    assert st.fw_block & 7 == (5 if arcs == "wide" else 7), st.fw_block
    assert lo <= st.ess_arcs <= hi, (lo, st.ess_arcs, hi)
    if target == 1022:
        assert lo == 0 and st.dist_enc == 2, (lo, st.dist_enc)
    else:
        assert lo > 0
        if arcs == "compact_derive":
            assert st.n_derived == 0, st.n_derived


# ------------------------------------------------------------------------------------------------
# b. hub degrees and the chunk block index
@pytest.mark.parametrize("kernel", ["wave", "wg_compact", "wg_compact_derive", "wg_wide", "ms",
                                    "block"])
def test_fan_chunk_past_the_indexed_blocks(gpu, monkeypatch, kernel):
    """fan(): twelve hubs of ~1,800 arcs settle in one chunk of > 16,384 arcs -- the workgroup
    kernel's owner search past its 256 indexed 64-arc blocks (WG_NBLK, both arc forms), the wave
    kernel's cover path for rows longer than 64 arcs, and ~3,000 candidates in one pass of the
    multi-source kernel (MS_LCAP = 2,048). That chunk is vertex 0's row's: derivation is off
    where the kernel itself must write every row, and on in one case of its own (the hubs' rows
    are core rows, low-degree rows derive from them)."""
    set_form(monkeypatch, kernel=kernel.split("_")[0], derive=int(kernel.endswith("derive")))
    g = sgr.fan(n_losses=300 if kernel == "wg_wide" else 200)
    _, _, st = _table(g, f"fan({kernel})")
    if kernel == "wave":
        assert st.dist_enc == 1 and st.fw_block & 1, (st.dist_enc, st.fw_block)
    elif kernel.startswith("wg"):
        assert st.dist_enc == 2 and st.ess_arcs == 0
        assert st.fw_block & 7 == (5 if kernel == "wg_wide" else 7), st.fw_block
        assert (st.n_derived > 0) == kernel.endswith("derive"), st.n_derived
    elif kernel == "ms":
        assert st.dist_enc == 3 and st.fw_block & 8, (st.dist_enc, st.fw_block)


@pytest.mark.parametrize("d", [4094, 4095, 4096])
def test_star_hub_degree_at_the_compact_clamp(gpu, monkeypatch, d):
    """The compact arcs carry the head's degree in 12 bits, clamped at 4095 and widened back to
    WG_DEGC (reloaded at pop): a hub of degree 4094, 4095 (the clamp's own value) and 4096."""
    set_form(monkeypatch, kernel="wg", derive=0)
    g = sgr.star(d, n_losses=200)
    _, _, st = _table(g, f"star({d})")
    assert st.dist_enc == 2 and st.ess_arcs == 0
    assert st.fw_block & 7 == 7, st.fw_block


@pytest.mark.parametrize("d", [32766, 32767, 32768])
def test_star_hub_degree_at_the_bucket_entry_clamp(gpu, monkeypatch, d):
    """A bucket entry carries the degree in 15 bits (WG_DEGC = 32767: reloaded at pop), 16-byte
    arcs (300 losses). 48 sampled rows, the hub's own among them. AUTO dispatch gives the
    workgroup kernel only past 32,768 vertices (d = 32768: n = 32,769, and a star is not local);
    the two smaller stars are below that size, so kernel=wg is forced for them."""
    import torch
    set_form(monkeypatch, kernel="auto" if d + 1 > 32768 else "wg")
    g = sgr.star(d, n_losses=300)
    n = g.n
    for st in _rows(g, [(0, 16), (n // 2, n // 2 + 16), (n - 16, n)], torch, f"star({d})"):
        assert st.dist_enc == 2, st.dist_enc
        assert st.fw_block & 7 == 5, st.fw_block
        assert st.ess_arcs == 0


# ------------------------------------------------------------------------------------------------
# c. ring size and arc-form switches
@pytest.mark.parametrize("kernel", ["wg", "wave"])
@pytest.mark.parametrize("w", [127, 128, 254, 255, 256])
def test_heavy_pendants_bucket_ring(gpu, monkeypatch, w, kernel):
    """Tight arcs of exactly max_w quanta: 127 is the largest compact-arc weight, 254 the largest
    with two-level steps (max_w + 2 <= 256 buckets), 255 fills the 256-bucket ring, 256 is past
    it (both kernels hand the graph to the block kernel)."""
    set_form(monkeypatch, kernel=kernel, derive=0)
    g = sgr.heavy_pendants(w)
    _, _, st = _table(g, f"heavy_pendants({w}, {kernel})")
    if w <= 255:
        assert st.dist_enc == (2 if kernel == "wg" else 1), st.dist_enc
        assert st.ess_arcs == 0
        if kernel == "wg":
            assert st.fw_block & 4 and bool(st.fw_block & 2) == (w == 127), st.fw_block


# ------------------------------------------------------------------------------------------------
# d. table and arc-count limits of the compact form
@pytest.mark.parametrize("k", [256, 257])
def test_reliability_table_limit(gpu, monkeypatch, k):
    """256 distinct reliabilities fill the 8-bit index (compact arcs, derived rows); 257 take the
    16-byte arcs and no derivation."""
    set_form(monkeypatch, kernel="wg")
    g = sgr.loss_table(k)
    _, _, st = _table(g, f"loss_table({k})")
    assert st.dist_enc == 2 and st.ess_arcs == 0
    if k == 256:
        assert st.fw_block & 7 == 7 and st.n_derived > 0 and st.fw_block & 64, \
            (st.fw_block, st.n_derived)
    else:
        assert st.fw_block & 7 == 5 and st.n_derived == 0 and not st.fw_block & 64, \
            (st.fw_block, st.n_derived)


@pytest.mark.parametrize("arcs", [2 ** 20 - 2, 2 ** 20])
def test_arc_count_limit(gpu, monkeypatch, arcs):
    """The compact arcs keep the head's row begin in 20 bits: 2^20 - 2 arcs is the largest even
    count that fits (the last rows' begins use the top of the field), 2^20 takes 16-byte arcs."""
    import torch
    set_form(monkeypatch, kernel="wg")
    g = sgr.many_arcs(arcs)
    for st in _rows(g, [(0, 32), (g.n - 32, g.n)], torch, f"many_arcs({arcs})"):
        assert st.dist_enc == 2 and st.ess_arcs == 0
        assert st.fw_block & 7 == (7 if arcs < 2 ** 20 else 5), st.fw_block


# ------------------------------------------------------------------------------------------------
# e. the multi-source kernel's 16-bit rows
@pytest.mark.parametrize("directed,total", [(False, 65534), (False, 65535),
                                            (True, 434 * 151), (True, 435 * 151)])
def test_multi_source_u16_bound(gpu, monkeypatch, directed, total):
    """dist_bound < 0xFFFF takes the u16 rows. 65,534 is a real distance at 0xFFFE, the
    saturation value itself; one quantum (undirected) or one hop (directed) more and the bound
    no longer fits, so the rows stay u32."""
    set_form(monkeypatch, kernel="ms")
    g = sgr.bound_path(total, directed)
    _, _, st = _table(g, f"bound_path({total}, directed={directed})")
    assert st.dist_enc == 3 and st.fw_block & 8, (st.dist_enc, st.fw_block)
    assert bool(st.fw_block & 16) == (total < 0xFFFF), st.fw_block


# ------------------------------------------------------------------------------------------------
# f. small switches
@pytest.mark.parametrize("n", [4096, 4097])
def test_wave_kernel_lds_row_limit(gpu, monkeypatch, n):
    """The wave kernel keeps its working row in LDS while eight rows fit a CU: n <= 4,096."""
    import torch
    set_form(monkeypatch, kernel="wave")
    g = graphs.random_geometric(n, seed=13)
    for st in _rows(g, [(0, 32), (n - 32, n)], torch, f"rgg{n} wave"):
        assert st.dist_enc == 1
        assert bool(st.fw_block & 1) == (n <= 4096), st.fw_block


@pytest.mark.parametrize("over", [0, 1])
def test_block_kernel_lds_working_set_limit(gpu, monkeypatch, over):
    """The block kernel's working set in LDS up to srt_sparse_max_n() vertices, in an HBM slot
    from one vertex more."""
    import torch
    set_form(monkeypatch, kernel="block")
    n = _lib.lib().srt_sparse_max_n() + over
    g = graphs.random_geometric(n, seed=17)
    _rows(g, [(0, 32), (n - 32, n)], torch, f"rgg{n} block")
