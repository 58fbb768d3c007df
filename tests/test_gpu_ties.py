"""srt_build_stats.tied_pairs of every path that counts it against tests/tie_reference.py (numpy
over the CPU oracle's distances), over all pairs: the dense FW in each distance tier
(pred_cols2_kernel on byte distances, pred_cols_kernel<u16> and <u32>), the squaring path, the
level build in its three post-pass forms (lvl_pred_kernel's tie form), and the sparse kernels
(tie_count_kernel over the wave, workgroup, multi-source and block kernels' rows and the derived
rows). Unreachable pairs are never tied.

A count_ties = 1 build runs other kernels than the plain build (no pred_cols3_kernel, no
lvl_pred_near_kernel): every case also builds with count_ties = 0 and requires the same tables
bit for bit.

Sharded builds: srt_build_tables_multi reports the sum over the ranks; srt_dense_build_sharded
reports each rank's count over its own rows."""
import ctypes

import numpy as np
import pytest
from conftest import set_form

import level_graphs as lg
import tie_reference
from shadow_amd import _lib, graphs
from shadow_amd._lib import ALGO_DENSE_FW, ALGO_SPARSE_SSSP

pytestmark = pytest.mark.gpu
MS = lg.MS
LEVELS = lg.LEVELS
DERIVED = 64  # srt_build_stats.fw_block bit of a sparse build with derived rows

_ref = {}
_graphs = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _ref.clear()
    _graphs.clear()


def _reference(g, key=None):
    """The reference's tied pairs per source of g (cached: `key` names graphs that share their
    edges' latencies, so their ties)."""
    key = key or g.name
    if key not in _ref:
        q = lg.quantum(g)
        D = tie_reference.distances_of_oracle(lg.oracle_table(g)["lat_int"])
        D = np.where(D < tie_reference.NO_ARC, D // q, D)
        per = tie_reference.tied_per_source(g.n, g.directed, g.src, g.dst, g.lat_ns // q, D)
        per.setflags(write=False)
        _ref[key] = per
    return _ref[key]


def _ties640(many_losses=False):
    """The 1-3 ms complete graph of test_gpu_levels.py ("ties"), optionally with more distinct
    losses than the level build's table holds (same latencies, so the same ties)."""
    key = ("ties640", many_losses)
    if key not in _graphs:
        g = graphs.complete_graph(640, seed=11, lat_max=3, name="ties640")
        if many_losses:
            loss = np.random.default_rng(11).random(g.m) * 0.05
            g = graphs.Graph(g.n, False, g.src, g.dst, g.lat_ns, loss, "ties640")
        _graphs[key] = g
    return _graphs[key]


def _with_far_vertex(g, ms=40_000):
    """g plus one vertex 40 s away from vertex 5: distances past the u16 tiers' caps."""
    key = ("far", g.name)
    if key not in _graphs:
        _graphs[key] = graphs.Graph(
            g.n + 1, g.directed, np.append(g.src, 5).astype(np.int32),
            np.append(g.dst, g.n).astype(np.int32), np.append(g.lat_ns, ms * MS),
            np.append(g.loss, 0.0123), g.name + "_far")
    return _graphs[key]


def _directed_random():
    """The directed graph of test_gpu_parity.py::test_directed_random."""
    if "dr" not in _graphs:
        rng = np.random.default_rng(11)
        n, m = 300, 2400
        src = rng.integers(0, n, m)
        dst = rng.integers(0, n, m)
        ring = np.arange(n)
        src = np.concatenate([src, ring, ring]).astype(np.int32)
        dst = np.concatenate([dst, (ring + 1) % n, ring]).astype(np.int32)
        lat = (rng.integers(1, 20, len(src)) * MS).astype(np.int64)
        loss = rng.integers(0, 300, len(src)) / 10000.0
        _graphs["dr"] = graphs.Graph(n, True, src, dst, lat, loss, "directed_random")
    return _graphs["dr"]


def _reweighted(g, lo, hi, seed=9):
    rng = np.random.default_rng(seed)
    lat = g.lat_ns.copy()
    off = g.src != g.dst
    lat[off] = rng.integers(lo, hi + 1, int(off.sum())) * MS
    return graphs.Graph(g.n, g.directed, g.src, g.dst, lat, g.loss, f"{g.name}_w{lo}_{hi}")


def _sparse_graph(which):
    if which not in _graphs:
        if which == "rgg":
            g = graphs.random_geometric(700, seed=3)
        elif which == "ba":
            g = graphs.barabasi_albert(700, seed=5)
        else:  # 1-2 ms: nearly every pair tied
            g = _reweighted(graphs.random_geometric(700, seed=3), 1, 2)
        _graphs[which] = g
    return _graphs[which]


def _counted(g, what, key=None, algo=ALGO_DENSE_FW, ngpus=None):
    """Build with and without the tie count: the count equals the reference over all pairs, the
    tables are the same bit for bit and match the oracle. Returns the counting build's stats."""
    lat1, rel1, st1 = lg.build(g, algo=algo, ngpus=ngpus, count_ties=1)
    lat0, rel0, st0 = lg.build(g, algo=algo, ngpus=ngpus, count_ties=0)
    expect = int(_reference(g, key).sum())
    print(f"{what}: tied_pairs {st1.tied_pairs}, reference {expect}")
    assert st1.tied_pairs == expect, (what, st1.tied_pairs, expect)
    assert st0.tied_pairs == 0, (what, st0.tied_pairs)
    assert st0.dist_enc == st1.dist_enc, (what, st0.dist_enc, st1.dist_enc)
    assert np.array_equal(lat0, lat1), what
    assert np.array_equal(rel0.view(np.uint64), rel1.view(np.uint64)), what
    lg.check_tables(g, lat1, rel1, what, reachable_only=True)
    return st1


# ---- dense FW: the three distance tiers, and the squaring path ----------------------------------
@pytest.mark.parametrize("tier", ["u8", "u8_254", "u16_255", "u32"])
def test_ties_dense_fw_tiers(gpu, monkeypatch, tier):
    """SRT_FORM square=0: the FW rounds. Byte distances (every distance <= 254 quanta:
    pred_cols2_kernel) on the 1-3 ms graph and at E = 254 exactly; E = 255 is the first graph of
    the u16 search; a vertex 40 s away takes the u32 kernels (encoding 1)."""
    set_form(monkeypatch, square="0")
    if tier == "u8":
        g, key = _ties640(), "ties640"
    elif tier == "u8_254":
        g, key = lg.core_tail(254), None
    elif tier == "u16_255":
        g, key = lg.core_tail(255), None
    else:
        g, key = _with_far_vertex(lg.core_tail(32)), None
    st = _counted(g, tier, key)
    assert st.dist_enc == (1 if tier == "u32" else 4), st.dist_enc


@pytest.mark.parametrize("which", ["ties640", "E32", "directed", "two_complete"])
def test_ties_dense_squaring(gpu, monkeypatch, which):
    """The default dense build of a small matrix: min-plus squaring (encoding 11). With
    unreachable pairs the squaring cannot finish in its u16 range and the default build ends on
    the u32 kernels (encoding 1) -- counted all the same."""
    monkeypatch.delenv("SRT_FORM", raising=False)
    g = {"ties640": _ties640, "E32": lambda: lg.core_tail(32), "directed": _directed_random,
         "two_complete": lg.two_complete}[which]()
    st = _counted(g, f"squaring {which}", "ties640" if which == "ties640" else None)
    assert st.dist_enc == (1 if which == "two_complete" else 11), st.dist_enc


# ---- the level build ------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "unpacked", "many_losses"])
@pytest.mark.parametrize("which", ["ties640", "E32", "E254"])
def test_ties_level_build(gpu, monkeypatch, which, form):
    """lvl_pred_kernel's tie form under the packed words (up to 31 levels), SRT_FORM pkw=0 and
    the f64 rows."""
    set_form(monkeypatch, levels="1", **({"pkw": "0"} if form == "unpacked" else {}))
    many = form == "many_losses"
    if which == "ties640":
        g, key = _ties640(many), "ties640"
    else:
        e = int(which[1:])
        g, key = lg.core_tail(e, many_losses=many), f"core_tail{e}"
    st = _counted(g, f"levels {which} {form}", key)
    assert st.dist_enc == LEVELS, st.dist_enc
    assert (st.rel_table == 0) == many, st.rel_table


@pytest.mark.parametrize("which", ["directed", "closed_block", "two_complete"])
def test_ties_forced_levels_directed_and_unreached(gpu, monkeypatch, which):
    """The directed random graph by levels; the graphs with unreachable pairs run the level
    budget out and are counted by the FW's kernels."""
    set_form(monkeypatch, levels="1")
    g = {"directed": _directed_random, "closed_block": lg.closed_block,
         "two_complete": lg.two_complete}[which]()
    st = _counted(g, f"levels=1 {which}")
    assert (st.dist_enc == LEVELS) == (which == "directed"), st.dist_enc


# ---- the sparse kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["wave", "wg", "wg_noderive", "ms", "block"])
@pytest.mark.parametrize("which", ["rgg", "ba", "w1_2"])
def test_ties_sparse_kernels(gpu, monkeypatch, which, kernel):
    g = _sparse_graph(which)
    set_form(monkeypatch, kernel=kernel.split("_")[0])
    if kernel == "wg_noderive":
        set_form(monkeypatch, derive="0")
    st = _counted(g, f"sparse {which} {kernel}", algo=ALGO_SPARSE_SSSP)
    if kernel == "wave":
        assert st.dist_enc == 1, st.dist_enc
    elif kernel == "ms":
        assert st.dist_enc == 3, st.dist_enc
    elif kernel.startswith("wg") and 2 * int(lg.row_eccentricity(g).max()) <= 1022:
        # (the workgroup kernel's packed row holds distances up to 1,022 quanta)
        assert st.dist_enc == 2, st.dist_enc
        if which == "ba":
            assert bool(st.fw_block & DERIVED) == (kernel == "wg"), st.fw_block
            assert (st.n_derived > 0) == (kernel == "wg"), st.n_derived


@pytest.mark.parametrize("which", ["directed", "closed_block", "closed_block128", "two_complete"])
def test_ties_sparse_directed_and_unreached(gpu, monkeypatch, which):
    monkeypatch.delenv("SRT_FORM", raising=False)
    g = {"directed": _directed_random, "closed_block": lg.closed_block,
         "closed_block128": lambda: lg.closed_block(block=128),
         "two_complete": lg.two_complete}[which]()
    _counted(g, f"sparse {which}", algo=ALGO_SPARSE_SSSP)


# ---- sharded builds -------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("which", ["levels_E32", "levels_E254", "fw_E255", "fw_two_complete"])
def test_ties_virtual_ranks_sum(gpu, monkeypatch, which, ranks):
    """srt_build_tables_multi: tied_pairs is the sum of the ranks' counts, so the reference over
    all pairs."""
    set_form(monkeypatch, levels="1")
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    if which == "fw_two_complete":
        g, key = lg.two_complete(), None
    else:
        e = int(which.split("E")[1])
        g, key = lg.core_tail(e, core=300), f"core300_tail{e}"
    assert all(b < end for b, end in lg.shard_rows(g.n, ranks))
    st = _counted(g, f"x{ranks} {which}", key, ngpus=1)
    assert (st.dist_enc == LEVELS) == which.startswith("levels"), st.dist_enc


def _sharded_complete(n, ld, ranks, seed, lat_max, count_ties):
    """srt_dense_build_sharded on `ranks` virtual ranks of device 0 over the device-generated
    complete graph (graphs.complete_graph's, bit for bit) -> (lat quanta, rel, stats, shards)."""
    import threading
    import torch
    L = _lib.lib()
    comms = (ctypes.c_void_p * ranks)()
    _lib.check(L.srt_comm_init_virtual(ranks, 0, comms), "srt_comm_init_virtual")
    shards, bufs, streams = [], [], []
    try:
        for r in range(ranks):
            b, e = ctypes.c_int32(), ctypes.c_int32()
            L.srt_shard_rows(ld, 128, ranks, r, ctypes.byref(b), ctypes.byref(e))
            b, e = b.value, e.value
            w = torch.empty((e - b, ld), dtype=torch.int32, device="cuda")
            rr = torch.empty((e - b, ld), dtype=torch.float64, device="cuda")
            st = torch.cuda.Stream()
            _lib.check(L.srt_gen_complete_device(n, ld, b, e - b, seed, lat_max, 10, 500,
                                                 w.data_ptr(), rr.data_ptr(),
                                                 ctypes.c_void_p(st.cuda_stream)), "generate")
            shards.append((b, min(e, n)))
            bufs.append((w, rr, torch.empty_like(w), torch.empty_like(rr)))
            streams.append(st)
        torch.cuda.synchronize()
        rcs = [None] * ranks
        stats = [_lib.BuildStats() for _ in range(ranks)]
        for s in stats:
            s.count_ties = count_ties

        def work(r):
            L.srt_virtual_rank_bind(r, 0)
            w, rr, lat, rel = bufs[r]
            rcs[r] = L.srt_dense_build_sharded(ctypes.c_void_p(comms[r]), n, ld, 0, w.data_ptr(),
                                               rr.data_ptr(), lat.data_ptr(), rel.data_ptr(),
                                               ctypes.c_void_p(streams[r].cuda_stream), 0,
                                               ctypes.byref(stats[r]))
            L.srt_virtual_rank_bind(-1, 0)

        th = [threading.Thread(target=work, args=(r,)) for r in range(ranks)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        for r in range(ranks):
            _lib.check(rcs[r], f"rank {r}")
        lat = np.concatenate([bufs[r][2].cpu().numpy() for r in range(ranks)])[:n, :n]
        rel = np.concatenate([bufs[r][3].cpu().numpy() for r in range(ranks)])[:n, :n]
    finally:
        for r in range(ranks):
            L.srt_comm_free(ctypes.c_void_p(comms[r]))
    return lat.view(np.uint32), rel, stats, shards


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("levels", ["1", "0"])
def test_ties_sharded_per_rank(gpu, monkeypatch, levels, ranks):
    """srt_dense_build_sharded: every rank reports the tied pairs of its own rows -- the
    reference restricted to them (n = ld = 640: at 3 ranks the row blocks are 128 | 256 | 256) --
    by levels and by the sharded FW rounds; the tables are those of the plain build."""
    set_form(monkeypatch, levels=levels)
    g = _ties640()
    per = _reference(g, "ties640")
    lat1, rel1, st1, shards = _sharded_complete(g.n, 640, ranks, 11, 3, 1)
    lat0, rel0, st0, _ = _sharded_complete(g.n, 640, ranks, 11, 3, 0)
    got = [int(s.tied_pairs) for s in st1]
    expect = [int(per[b:e].sum()) for b, e in shards]
    print(f"x{ranks} levels={levels}: per-rank tied_pairs {got}, reference {expect}")
    assert got == expect
    assert [int(s.tied_pairs) for s in st0] == [0] * ranks
    assert all((s.dist_enc == LEVELS) == (levels == "1") for s in st1), [s.dist_enc for s in st1]
    assert np.array_equal(lat0, lat1)
    assert np.array_equal(rel0.view(np.uint64), rel1.view(np.uint64))
    lg.check_tables(g, lat1.astype(np.uint64) * np.uint64(MS), rel1, f"sharded x{ranks}")
