"""The source-sharded sparse build at 4 and 8 ranks: each rank settles its block of
sources with the sparse kernels, then the rows are all-gathered (srt_sparse_allgather /
ncclAllGather). Ranks are virtual (SRT_VIRTUAL_RANKS: R ranks on device 0, collectives as device
copies), so the schedule, the shard boundaries and the gather run as they would on R GPUs.

Against oracle.sssp_list (the restatement of topology.c:1578-1814's per-source Dijkstra):
latency bit-exact in integer ns, reliability within 1e-12 relative (north_star)."""
import ctypes

import numpy as np
import pytest

from conftest import form_env
import oracle
from shadow_amd import graphs
from shadow_amd._lib import ALGO_AUTO, ALGO_SPARSE_SSSP, BuildOpts, BuildStats, Edges, check, lib
from shadow_amd.topology import build_tables, build_tables_subset

pytestmark = pytest.mark.gpu
REL_TOL = 1e-12


def _el(g):
    return oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)


def _rel_err(got, exp):
    return float((np.abs(got - exp) / np.maximum(np.abs(exp), 1e-300)).max())


def test_c5_attached_2000_eight_virtual_ranks(gpu, monkeypatch):
    """C5 (100,000-vertex BA graph) with ~2,000 attached vertices on 8 ranks: each rank builds
    ~250 sources' rows over the whole graph, the sub-table is all-gathered; the same sub-table as
    one GPU and as the oracle."""
    g = graphs.barabasi_albert(100_000, seed=5)
    rng = np.random.default_rng(808)
    verts = np.unique(np.concatenate([rng.choice(g.n, 2000, replace=False), [0, 1, 99_999]]))
    verts = verts.astype(np.int32)
    lat1, rel1, _, mn1, st1 = build_tables_subset(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                  verts=verts, algo=ALGO_AUTO)
    assert st1.algo == ALGO_SPARSE_SSSP
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", "8")
    lat8, rel8, _, mn8, st8 = build_tables_subset(g.n, False, g.src, g.dst, g.lat_ns, g.loss,
                                                  verts=verts, algo=ALGO_AUTO, ngpus=8)
    assert st8.algo == ALGO_SPARSE_SSSP
    assert np.array_equal(lat1, lat8) and np.array_equal(rel1, rel8) and mn1 == mn8
    rows = oracle.sssp_list(_el(g), verts, nthreads=16)
    elat = rows["lat_int"][:, verts]
    erel = rows["rel"][:, verts]
    off = ~np.eye(len(verts), dtype=bool)
    assert np.array_equal(lat8[off], elat[off])
    assert _rel_err(rel8[off], erel[off]) <= REL_TOL


def test_c3_full_table_four_virtual_ranks(gpu, monkeypatch):
    """C3 (20,000-vertex RGG, the multi-source kernel) full table on 4 ranks: 5,000 source rows
    per rank, all-gathered into the 20,000 x 20,000 table; every row against the oracle (in
    blocks of 2,000 rows)."""
    g = graphs.random_geometric(20000, seed=3)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", "4")
    lat, rel, st = build_tables(g.n, False, g.src, g.dst, g.lat_ns, g.loss, algo=ALGO_AUTO,
                                ngpus=1)
    assert st.algo == ALGO_SPARSE_SSSP
    el = _el(g)
    worst = 0.0
    for s0 in range(0, g.n, 2000):
        s1 = min(g.n, s0 + 2000)
        exp = oracle.sssp_rows(el, s0, s1, nthreads=16)
        off = np.arange(g.n)[None, :] != np.arange(s0, s1)[:, None]
        assert np.array_equal(np.where(off, lat[s0:s1], 0), np.where(off, exp["lat_int"], 0)), \
            f"latency mismatch in rows {s0}..{s1}"
        worst = max(worst, _rel_err(np.where(off, rel[s0:s1], 1.0),
                                    np.where(off, exp["rel"], 1.0)))
    assert worst <= REL_TOL, worst


def _subset_counting_ties(g, verts, ngpus=1, want_ms=False):
    """srt_build_tables_subset with srt_build_stats.count_ties set (build_tables_subset leaves it
    0) -> (lat quanta [k, k], rel, lat_ms or None, min quanta, stats, row chunks)."""
    e = Edges(g.n, int(g.directed), len(g.src), g.src.ctypes.data, g.dst.ctypes.data,
              g.lat_ns.ctypes.data, g.loss.ctypes.data)
    o = BuildOpts(0, ALGO_SPARSE_SSSP, 1, 0)
    k = len(verts)
    lat = np.empty((k, k), np.uint32)
    rel = np.empty((k, k), np.float64)
    ms = np.empty((k, k), np.float64) if want_ms else None
    q, mn, st = ctypes.c_uint64(), ctypes.c_uint32(), BuildStats()
    st.count_ties = 1
    check(lib().srt_build_tables_subset(ctypes.byref(e), ctypes.byref(o), ngpus, k,
                                        verts.ctypes.data, lat.ctypes.data, ctypes.byref(q),
                                        rel.ctypes.data, None if ms is None else ms.ctypes.data,
                                        ctypes.byref(mn), ctypes.byref(st)),
          "srt_build_tables_subset")
    return lat.astype(np.uint64) * np.uint64(q.value), rel, ms, mn.value, st, \
        lib().srt_last_row_chunks()


def test_attached_rows_in_several_chunks(gpu, monkeypatch):
    """101 attached vertices of a 2,000-vertex RGG with room for a few source rows at a time
    (SRT_FORM memcap=1: 1 MiB free is below the reserve, so the budget is half of it, shared by
    the virtual ranks): on one GPU, with the f64 ms rows beside them, and on 2 virtual ranks. The
    chunks' offsets into the sub-table, the short last chunk and the statistics added over the
    chunks: the same tables, minimum and tied pairs as the build that takes every row at once,
    and the oracle's rows."""
    g = graphs.random_geometric(2000, seed=3)
    verts = np.unique(np.random.default_rng(17).integers(0, g.n, 150))[:101].astype(np.int32)
    assert len(verts) == 101
    lat0, rel0, ms0, mn0, st0, chunks0 = _subset_counting_ties(g, verts, want_ms=True)
    assert chunks0 == 1 and st0.tied_pairs > 0

    def chunked(rows, sharers=1, row_bytes=12, **kw):
        with form_env(memcap=1):
            lat, rel, ms, mn, st, chunks = _subset_counting_ties(g, verts, **kw)
        chunk = (1 << 19) // sharers // (row_bytes * g.n)
        print(f"{kw}: {rows} rows, {chunk} a chunk, {chunks} chunks, tied {st.tied_pairs}")
        assert chunks >= 3 and chunks == -(-rows // chunk) and rows % chunk != 0, (chunks, chunk)
        assert np.array_equal(lat, lat0) and np.array_equal(rel, rel0) and mn == mn0
        assert st.algo == ALGO_SPARSE_SSSP and st.tied_pairs == st0.tied_pairs
        return ms

    chunked(101)
    assert np.array_equal(chunked(101, row_bytes=20, want_ms=True), ms0)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", "2")
    chunked(51, sharers=2, ngpus=2)  # rank 0 holds 51 of the 101 slots
    rows = oracle.sssp_list(_el(g), verts, nthreads=16)
    off = ~np.eye(len(verts), dtype=bool)
    assert np.array_equal(lat0[off], rows["lat_int"][:, verts][off])
    assert _rel_err(rel0[off], rows["rel"][:, verts][off]) <= REL_TOL
