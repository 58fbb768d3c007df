"""The level build of a directed dense graph on more than one rank (shadow_amd/csrc/levels.hip,
"directed graph, N > 1"): a rank holds the out-arcs of its rows, so every target's in-arcs are
counted per rank, gathered once and merged on every rank, and the levels then run as on one GPU
with the rank's source window.

Virtual ranks on one device (SRT_VIRTUAL_RANKS through the public build, srt_comm_init_virtual for
the collective log). Everything is held to the CPU oracle: latency bit-exact, reliability within
1e-12 relative, the diagonal rule included (check_tables). The graphs (tests/level_graphs.py
core_tail with a 300-vertex core, and a 35 %-dense directed graph of 500 vertices) have ld a
multiple of 128 and no empty shard for the rank counts used; on the dense graph two thirds of the
ordered pairs have d(s, t) != d(t, s), so a build that took out-arcs for in-arcs fails on it, and
its last shard has 12 padding rows."""
import ctypes
import threading

import numpy as np
import pytest
from conftest import form_env, set_form

import level_graphs as lg
import levels_protocol_directed as lpd
from level_graphs import LEVELS, MS, check_tables
from shadow_amd import _lib, graphs

pytestmark = pytest.mark.gpu
JOIN_S = 120


def _directed_dense(n=500, seed=5, wmax=40):
    """tests/test_gpu_levels.py's 35 %-dense directed graph over a ring, restated."""
    key = ("ddense", n, seed, wmax)
    if key not in lg._cache:
        rng = np.random.default_rng(seed)
        i, j = np.nonzero(rng.random((n, n)) < 0.35)
        keep = i != j
        i, j = i[keep], j[keep]
        ring = np.arange(n)
        src = np.concatenate([i, ring]).astype(np.int32)
        dst = np.concatenate([j, (ring + 1) % n]).astype(np.int32)
        lat = (rng.integers(1, wmax + 1, len(src)) * MS).astype(np.int64)
        loss = rng.integers(0, 300, len(src)) / 10000.0
        lg._cache[key] = graphs.Graph(n, True, src, dst, lat, loss, f"directed{n}")
    return lg._cache[key]


def _own_levels(g, ranks):
    """Each rank's last level: the largest distance from its own sources, 2 at the least (level 1
    never reports completion) -- own_levels of tests/levels_protocol.py."""
    ecc = lg.row_eccentricity(g)
    return [max(2, int(ecc[b:e].max())) for b, e in lg.shard_rows(g.n, ranks)]


def _public_build(monkeypatch, g, ranks, **form):
    set_form(monkeypatch, **form)
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", str(ranks))
    assert all(b < e for b, e in lg.shard_rows(g.n, ranks))
    return lg.build(g, ngpus=1)


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("e", [4, 5, 7, 9, 12, 33])
def test_directed_ranks_core_tail(gpu, monkeypatch, e, ranks):
    """(a) E inside the first batch (4, 5), in the one-level batches (7), past the first
    extraction (9, 12) and past the packed post pass (33). The stats are rank 0's."""
    g = lg.core_tail(e, core=300, directed=True)
    lat, rel, st = _public_build(monkeypatch, g, ranks, levels="1")
    assert st.dist_enc == LEVELS and st.levels >= 1, (st.dist_enc, st.levels)
    assert st.levels == _own_levels(g, ranks)[0], (st.levels, _own_levels(g, ranks))
    check_tables(g, lat, rel, f"directed E={e} x{ranks}")


@pytest.mark.parametrize("ranks", [2, 3, 4])
def test_directed_ranks_dense(gpu, monkeypatch, ranks):
    """(a) the 35 %-dense graph: largest distance 7, asymmetric distances, 12 padding rows."""
    g = _directed_dense()
    d = lg.oracle_table(g)["lat_int"]
    assert lg.largest_distance(g) == 7 and float((d != d.T).mean()) > 0.5
    lat, rel, st = _public_build(monkeypatch, g, ranks, levels="1")
    assert st.dist_enc == LEVELS and st.levels >= 1, (st.dist_enc, st.levels)
    assert st.levels == _own_levels(g, ranks)[0], (st.levels, _own_levels(g, ranks))
    check_tables(g, lat, rel, f"directed dense x{ranks}")


def test_directed_ranks_many_losses(gpu, monkeypatch):
    """(b) more distinct reliabilities than the table holds: the f64 rows."""
    g = lg.core_tail(5, core=300, directed=True, many_losses=True)
    lat, rel, st = _public_build(monkeypatch, g, 2, levels="1")
    assert st.dist_enc == LEVELS and st.levels >= 1 and st.rel_table == 0, \
        (st.dist_enc, st.levels, st.rel_table)
    check_tables(g, lat, rel, "directed many losses x2")


def test_directed_ranks_unpacked(gpu, monkeypatch):
    """(b) SRT_FORM pkw=0: the u8 level rows and the transposed post pass."""
    g = lg.core_tail(5, core=300, directed=True, many_losses=True)
    lat, rel, st = _public_build(monkeypatch, g, 3, levels="1", pkw="0")
    assert st.dist_enc == LEVELS and st.levels >= 1, (st.dist_enc, st.levels)
    check_tables(g, lat, rel, "directed pkw=0 x3")


# ---- srt_dense_build_sharded on virtual ranks, with the collective log ---------------------------

def _dense_of_directed(g):
    """(w quanta u32, r f64) of a directed whole-millisecond graph without parallel arcs."""
    assert g.directed
    pair = g.src.astype(np.int64) * g.n + g.dst
    assert len(np.unique(pair)) == len(pair)
    w = np.full((g.n, g.n), lpd.INF, np.uint32)
    r = np.zeros((g.n, g.n))
    q = (g.lat_ns // MS).astype(np.uint32)
    assert np.all(q.astype(np.int64) * MS == g.lat_ns)
    w[g.src, g.dst] = q
    r[g.src, g.dst] = 1.0 - g.loss
    return w, r


def _sharded_logged(L, w, r, n, R):
    """srt_dense_build_sharded (directed) on R virtual ranks with the collective log on; returns
    the tables (ld x ld), each rank's log and stats. Every rank's thread must join in time."""
    import torch
    ld = lpd.padded(n)
    W = np.full((ld, ld), lpd.INF, np.uint32)
    Rr = np.zeros((ld, ld))
    W[:n, :n] = w
    Rr[:n, :n] = r
    comms = (ctypes.c_void_p * R)()
    _lib.check(L.srt_comm_init_virtual(R, 0, comms), "srt_comm_init_virtual")
    try:
        bufs, streams = [], []
        for q in range(R):
            b, e = lpd.shard(ld, R, q)
            wt = torch.from_numpy(np.ascontiguousarray(W[b:e]).view(np.int32)).cuda()
            rt = torch.from_numpy(np.ascontiguousarray(Rr[b:e])).cuda()
            bufs.append((wt, rt, torch.empty_like(wt), torch.empty_like(rt)))
            streams.append(torch.cuda.Stream())
            _lib.check(L.srt_comm_log_enable(ctypes.c_void_p(comms[q]), 1), "srt_comm_log_enable")
        torch.cuda.synchronize()
        rcs = [None] * R
        stats = [_lib.BuildStats() for _ in range(R)]

        def work(q):
            L.srt_virtual_rank_bind(q, 0)
            wt, rt, lat, rel = bufs[q]
            rcs[q] = L.srt_dense_build_sharded(ctypes.c_void_p(comms[q]), n, ld, 1, wt.data_ptr(),
                                               rt.data_ptr(), lat.data_ptr(), rel.data_ptr(),
                                               ctypes.c_void_p(streams[q].cuda_stream), 0,
                                               ctypes.byref(stats[q]))
            L.srt_virtual_rank_bind(-1, 0)

        th = [threading.Thread(target=work, args=(q,), daemon=True) for q in range(R)]
        for t in th:
            t.start()
        for t in th:
            t.join(JOIN_S)
            assert not t.is_alive(), "a virtual rank did not return (collectives paired wrongly?)"
        torch.cuda.synchronize()
        for q in range(R):
            _lib.check(rcs[q], f"rank {q}")
        logs = []
        for q in range(R):
            k = L.srt_comm_log_read(ctypes.c_void_p(comms[q]), None, 0)
            buf = np.zeros(3 * max(k, 1), np.int64)
            L.srt_comm_log_read(ctypes.c_void_p(comms[q]), buf.ctypes.data, k)
            logs.append(buf[:3 * k].reshape(k, 3).tolist())
        lat = np.concatenate([bufs[q][2].cpu().numpy() for q in range(R)]).view(np.uint32)
        rel = np.concatenate([bufs[q][3].cpu().numpy() for q in range(R)])
    finally:
        for q in range(R):
            L.srt_comm_free(ctypes.c_void_p(comms[q]))
    return lat, rel, logs, stats


def _check_sharded_tables(g, lat, rel, what, by_levels=False):
    n = g.n
    check_tables(g, lat[:n, :n].astype(np.uint64) * np.uint64(MS), rel[:n, :n], what)
    assert n < lat.shape[0]  # the padding rows of the last shard: no path
    assert np.all(lat[n:, :n] == lpd.INF), what
    if by_levels:
        assert np.all(rel[n:, :n] == 0.0), what


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("e", [5, 12])
def test_directed_protocol(gpu, monkeypatch, e, ranks):
    """(d) one extraction and one vote (E = 5); the second extraction and several votes (E = 12):
    every rank logs the same calls, the ones of levels_protocol_directed.directed_calls."""
    set_form(monkeypatch, levels="1")
    g = lg.core_tail(e, core=300, directed=True)
    w, r = _dense_of_directed(g)
    outcome, calls, own = lpd.directed_calls(w, ranks)
    assert outcome == "levels" and own == _own_levels(g, ranks), (outcome, own)
    lat, rel, logs, stats = _sharded_logged(gpu, w, r, g.n, ranks)
    assert all(lg_ == logs[0] for lg_ in logs), logs
    assert logs[0] == calls, (logs[0], calls)
    assert {int(s.dist_enc) for s in stats} == {LEVELS}
    assert [int(s.levels) for s in stats] == own, ([int(s.levels) for s in stats], own)
    _check_sharded_tables(g, lat, rel, f"protocol E={e} x{ranks}", by_levels=True)


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("hook", ["lcap_r1", "memcap"])
def test_directed_fallbacks_stay_collective(gpu, monkeypatch, hook, ranks):
    """(c), and (d)'s fallback case: rank 1's budget of one level (lcap_r1=1), or no memory for a
    single plane on any rank (memcap=0), sends every rank to the Floyd-Warshall after the
    agreement: the log is the level build's two all-reduces, then exactly the calls of the build
    that never tried the levels."""
    g = lg.core_tail(5, core=300, directed=True)
    w, r = _dense_of_directed(g)
    with form_env(levels="0"):
        _, _, fw_logs, _ = _sharded_logged(gpu, w, r, g.n, ranks)
    set_form(monkeypatch, levels="1", **({"lcap_r1": "1"} if hook == "lcap_r1" else {"memcap": "0"}))
    lat, rel, logs, stats = _sharded_logged(gpu, w, r, g.n, ranks)
    assert all(lg_ == logs[0] for lg_ in logs), logs
    outcome, calls, _ = lpd.directed_calls(w, ranks, {1: 1})
    assert outcome == "fw" and len(calls) == 2
    assert logs[0] == calls + fw_logs[0], (logs[0][:4], calls)
    assert LEVELS not in {int(s.dist_enc) for s in stats}
    assert all(int(s.levels) == 0 for s in stats)
    _check_sharded_tables(g, lat, rel, f"{hook} x{ranks}")


def _auto_rows(n, seed=41):
    """Dense rows made directly: weights 1..16 quanta, independent per direction; reliabilities
    from a grid of 300 values; a self-loop on every vertex."""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 17, (n, n)).astype(np.uint32)
    r = 1.0 - rng.integers(0, 300, (n, n)) / 10000.0
    return w, r


def test_directed_ranks_automatic(gpu, monkeypatch):
    """(e) no SRT_FORM: n = 4,096 on 2 ranks takes the level build by the automatic rule (n >=
    4,096, budget under half the predicted FW time), and gives the tables of the FW build."""
    n, ranks = 4096, 2
    w, r = _auto_rows(n)
    monkeypatch.delenv("SRT_FORM", raising=False)
    lat, rel, logs, stats = _sharded_logged(gpu, w, r, n, ranks)
    assert all(lg_ == logs[0] for lg_ in logs)
    assert [int(s.dist_enc) for s in stats] == [LEVELS] * ranks, [int(s.dist_enc) for s in stats]
    set_form(monkeypatch, levels="0")
    lat0, rel0, _, stats0 = _sharded_logged(gpu, w, r, n, ranks)
    assert LEVELS not in {int(s.dist_enc) for s in stats0}
    assert np.array_equal(lat, lat0)
    err = np.abs(rel - rel0) / np.maximum(np.abs(rel0), 1e-300)
    assert float(err.max()) <= 1e-12, float(err.max())
