"""Multi-process (world_size 2, gloo, CPU) rehearsal of the sharded builds' decomposition.

The GPU path (srt_dense_build_sharded / srt_sparse_allgather) runs one process per GPU over
RCCL. Here the same schedule -- the library's own srt_shard_rows partition, the owner of each
64-row pivot block, one pivot-panel broadcast per round in the lookahead order (panel k+1 is
produced from a partially updated round k), the essential-arc all-reduce/broadcast and the
sparse source-shard all-gather -- is replayed with numpy compute and gloo collectives, and the
assembled tables must equal the CPU oracle's raw per-source rows (no mirror exchange: each rank's
rows are its own sources', and the lookup layer picks the serving row, pairorder.c). The row-sharded symmetric rounds (kept-tile
checkerboard, panel blocks broadcast by their holders, final transpose fill) are replayed the
same way.
"""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from shadow_amd import graphs

INF = 0x7FFFFFFF
KB = 64
ALIGN = 128


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(lib, ld, R, r):
    b, e = ctypes.c_int32(), ctypes.c_int32()
    lib.srt_shard_rows(ld, ALIGN, R, r, ctypes.byref(b), ctypes.byref(e))
    return b.value, e.value


def _minplus(A, B):
    """min over m of A[:, m] + B[m, :] (int64 to avoid overflow)."""
    return (A[:, :, None].astype(np.int64) + B[None, :, :].astype(np.int64)).min(axis=1)


def _dense_worker(rank, R, port, n, seed, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=R)
    from shadow_amd._lib import lib
    L = lib()
    ld = (n + ALIGN - 1) // ALIGN * ALIGN
    b, e = _shard(L, ld, R, rank)
    w, r = graphs.complete_dense(n, seed)
    W = np.full((ld, ld), INF, np.int64)
    W[:n, :n] = w
    Rm = np.zeros((ld, ld))
    Rm[:n, :n] = r
    D = W[b:e].copy()
    for i in range(b, e):
        D[i - b, i] = 0
    owners = [_shard(L, ld, R, x) for x in range(R)]

    def owner(k0):
        return [x for x, (qb, qe) in enumerate(owners) if qb <= k0 < qe][0]

    def produce(k0):
        """diagonal closure + pivot-row panel of block k0 (owner), broadcast to every rank"""
        P = torch.zeros((KB, ld), dtype=torch.int64)
        if owner(k0) == rank:
            Pk = D[k0 - b:k0 - b + KB]
            T = Pk[:, k0:k0 + KB]
            for m in range(KB):  # diagonal closure
                T = np.minimum(T, T[:, m:m + 1] + T[m:m + 1, :])
            Pk[:, k0:k0 + KB] = T
            Pk[:] = np.minimum(Pk, _minplus(T, Pk))  # row panel
            P = torch.from_numpy(Pk.copy())
        dist.broadcast(P, owner(k0))
        return P.numpy()

    def update(Pn, k0, rows):
        sel = np.zeros(e - b, bool)
        sel[rows] = True
        D[sel] = np.minimum(D[sel], _minplus(D[sel][:, k0:k0 + KB], Pn))

    # lookahead order of srt_fw16_build (fw16.hip): the owner of block k+1 updates the 128-row
    # tile row holding it first, produces and broadcasts panel k+1, then updates the other rows
    Pn = produce(0)
    for k0 in range(0, ld, KB):
        Dkk = Pn[:, k0:k0 + KB]
        mine = np.array([not (k0 <= b + i < k0 + KB) for i in range(e - b)])
        col = D[:, k0:k0 + KB]
        col[mine] = np.minimum(col[mine], _minplus(col[mine], Dkk))  # column panel
        k1 = k0 + KB
        rows = np.arange(e - b)
        if k1 < ld and owner(k1) == rank:
            t0 = (k1 - b) // ALIGN * ALIGN
            first = rows[t0:t0 + ALIGN]
            update(Pn, k0, first)
            Pnext = produce(k1)
            update(Pn, k0, np.setdiff1d(rows, first))
        else:
            update(Pn, k0, rows)
            Pnext = produce(k1) if k1 < ld else None
        Pn = Pnext
    # essential arcs (W[u][t] == D[u][t], u != t) of the local rows; all-reduce the counts
    cnt = torch.zeros(ld, dtype=torch.int64)
    arcs = {}
    for i in range(e - b):
        u = b + i
        if u >= n:
            continue
        ts = [t for t in range(n) if t != u and W[u, t] < INF and W[u, t] == D[i, t]]
        arcs[u] = ts
        cnt[u] = len(ts)
    dist.all_reduce(cnt)
    # every rank broadcasts its rows' arcs (same segments as the RCCL broadcasts)
    inarc = {}
    for x, (qb, qe) in enumerate(owners):
        seg = torch.zeros(int(cnt[qb:qe].sum()), dtype=torch.int64)
        if x == rank:
            seg = torch.tensor([t for u in range(qb, min(qe, n)) for t in arcs[u]], dtype=torch.int64)
        dist.broadcast(seg, x)
        o = 0
        for u in range(qb, min(qe, n)):
            inarc[u] = seg[o:o + int(cnt[u])].tolist()
            o += int(cnt[u])
    # canonical predecessor + path-order reliability for local rows (undirected: In* = Out*)
    Dfull = np.zeros((ld, ld), np.int64)
    Dt = torch.from_numpy(np.ascontiguousarray(D))
    parts = [torch.zeros((qe - qb, ld), dtype=torch.int64) for qb, qe in owners]
    dist.all_gather(parts, Dt)
    Dfull = torch.cat(parts).numpy()  # only the lat check below uses the assembled D
    rel = np.zeros((e - b, ld))
    for i in range(e - b):
        s = b + i
        if s >= n:
            continue
        pred = {}
        for t in range(n):
            if t == s:
                continue
            best = None
            for u in inarc[t]:
                if D[i, u] + W[u, t] == D[i, t]:
                    key = (D[i, u], u)
                    best = key if best is None or key < best else best
            pred[t] = best[1]
        order = sorted(range(n), key=lambda t: D[i, t])
        rr = np.full(n, -1.0)
        rr[s] = 1.0
        for t in order:
            if t != s:
                rr[t] = rr[pred[t]] * Rm[pred[t], t]
        rel[i, :n] = rr
    for i in range(e - b):  # diagonal rule
        s = b + i
        if s >= n:
            continue
        cands = [((W[s, u] if u == s else 2 * W[s, u]), u) for u in range(n)]
        lat_d, u = min(cands)
        D[i, s] = lat_d
        rel[i, s] = Rm[s, s] if u == s else Rm[s, u] * Rm[s, u]
    q.put((rank, b, e, D[:, :n].copy(), rel[:, :n].copy(), Dfull[:n, :n].copy()))
    dist.barrier()
    dist.destroy_process_group()


def _dense_sym_worker(rank, R, port, n, seed, q, rp=KB):
    """The row-sharded symmetric rounds of fw16.hip srt_fw16_build_sym_sharded (its band
    broadcast is sym_send, its closure sym_close; the library runs the rp = 128 form only, the
    64-pivot model stays as the plainer statement of the same rounds), distances only: each
    rank keeps one orientation of every 128-tile pair (sym_kept); every rank broadcasts the
    pivot-panel blocks it holds (its kept row blocks, or transposed 64 x 128 slices of its tiles
    in the pivot column), every rank closes the diagonal block and the row panel itself and the
    owner writes them back; every rank updates its kept tiles with A = P^T and B = P, the next
    pivot block's tile row / column first; at the end each rank receives the transposes of the
    tiles it does not keep.
    rp = 128 (encoding 8): a round's pivot block is one tile row K; its band is staged as two
    half-panels (rows a, then rows b, two broadcasts per contributor); every rank closes P_a,
    applies it to the staged b rows (sym_cross_stage_kernel), closes P_b, and the kept tiles take
    both panels (min-plus over the 128 rows of P = P_a over P_b, as the four stages do)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=R)
    from shadow_amd._lib import lib
    L = lib()
    ld = (n + ALIGN - 1) // ALIGN * ALIGN
    T = ld // ALIGN
    b, e = _shard(L, ld, R, rank)
    tb, te = b // ALIGN, e // ALIGN
    w, _ = graphs.complete_dense(n, seed)
    W = np.full((ld, ld), INF, np.int64)
    W[:n, :n] = w
    D = W[b:e].copy()
    for i in range(b, e):
        D[i - b, i] = 0
    ranges = [_shard(L, ld, R, x) for x in range(R)]
    own = {K: x for x, (qb, qe) in enumerate(ranges) for K in range(qb // ALIGN, qe // ALIGN)}

    def kept(I, J):
        return I == J or ((I < J) == ((I + J) % 2 == 0))

    def tile(I, J):  # view of this rank's tile (I, J)
        return D[(I - tb) * ALIGN:(I - tb + 1) * ALIGN, J * ALIGN:(J + 1) * ALIGN]

    def produce(k0):
        """P_k from every rank's blocks (one broadcast per contributor, in (contributor, J)
        order); every rank closes the diagonal block and the row panel itself"""
        K, o = k0 // ALIGN, own[k0 // ALIGN]
        contrib = [o if kept(K, J) else own[J] for J in range(T)]
        P = np.zeros((KB, ld), np.int64)
        for x in range(R):
            js = [J for J in range(T) if contrib[J] == x]
            if not js:
                continue
            buf = torch.zeros((KB, ALIGN * len(js)), dtype=torch.int64)
            if x == rank:
                blocks = [D[k0 - b:k0 - b + KB, J * ALIGN:(J + 1) * ALIGN] if kept(K, J) else
                          D[(J - tb) * ALIGN:(J - tb + 1) * ALIGN, k0:k0 + KB].T for J in js]
                buf = torch.from_numpy(np.ascontiguousarray(np.concatenate(blocks, axis=1)))
            dist.broadcast(buf, x)
            for i, J in enumerate(js):
                P[:, J * ALIGN:(J + 1) * ALIGN] = buf[:, i * ALIGN:(i + 1) * ALIGN].numpy()
        Tk = P[:, k0:k0 + KB]
        for m in range(KB):  # diagonal closure
            Tk = np.minimum(Tk, Tk[:, m:m + 1] + Tk[m:m + 1, :])
        P[:, k0:k0 + KB] = Tk
        P[:] = np.minimum(P, _minplus(Tk, P))  # row panel
        if rank == o:
            D[k0 - b:k0 - b + KB] = P
        return P

    def close(X, k0):
        """diagonal closure of columns k0..k0+63 of the 64-row block X, then its row panel"""
        Tk = X[:, k0:k0 + KB]
        for m in range(KB):
            Tk = np.minimum(Tk, Tk[:, m:m + 1] + Tk[m:m + 1, :])
        X[:, k0:k0 + KB] = Tk
        X[:] = np.minimum(X, _minplus(Tk, X))
        return X

    def produce128(k0):
        K, o = k0 // ALIGN, own[k0 // ALIGN]
        contrib = [o if kept(K, J) else own[J] for J in range(T)]
        Pa = np.zeros((KB, ld), np.int64)
        Xb = np.zeros((KB, ld), np.int64)
        for x in range(R):
            js = [J for J in range(T) if contrib[J] == x]
            if not js:
                continue
            for half, out in ((0, Pa), (KB, Xb)):
                buf = torch.zeros((KB, ALIGN * len(js)), dtype=torch.int64)
                if x == rank:
                    r0 = k0 + half
                    blocks = [D[r0 - b:r0 - b + KB, J * ALIGN:(J + 1) * ALIGN] if kept(K, J) else
                              D[(J - tb) * ALIGN:(J - tb + 1) * ALIGN, r0:r0 + KB].T for J in js]
                    buf = torch.from_numpy(np.ascontiguousarray(np.concatenate(blocks, axis=1)))
                dist.broadcast(buf, x)
                for i, J in enumerate(js):
                    out[:, J * ALIGN:(J + 1) * ALIGN] = buf[:, i * ALIGN:(i + 1) * ALIGN].numpy()
        close(Pa, k0)
        Xb[:] = np.minimum(Xb, _minplus(Xb[:, k0:k0 + KB], Pa))  # the b rows take pivot block a
        close(Xb, k0 + KB)
        P = np.concatenate([Pa, Xb])
        if rank == o:
            D[k0 - b:k0 - b + ALIGN] = P
        return P

    def update(P, tiles):
        for I, J in tiles:
            C = tile(I, J)
            C[:] = np.minimum(C, _minplus(P[:, I * ALIGN:(I + 1) * ALIGN].T,
                                          P[:, J * ALIGN:(J + 1) * ALIGN]))

    mine = [(I, J) for I in range(tb, te) for J in range(T) if kept(I, J)]
    make = produce128 if rp == 128 else produce
    P = make(0)
    for k0 in range(0, ld, rp):
        k1 = k0 + rp
        if k1 < ld:
            K1 = k1 // ALIGN
            cross = [t for t in mine if K1 in t]
            update(P, cross)
            Pn = make(k1)
            update(P, [t for t in mine if K1 not in t])
        else:
            update(P, mine)
            Pn = None
        P = Pn
    # fill: x sends the transposes of its kept tiles (I in x, J in y) to y, in one global order
    for x, (xb, xe) in enumerate(ranges):
        for y, (yb, ye) in enumerate(ranges):
            pairs = [(I, J) for I in range(xb // ALIGN, xe // ALIGN)
                     for J in range(yb // ALIGN, ye // ALIGN) if I != J and kept(I, J)]
            if not pairs:
                continue
            if x == y == rank:
                for I, J in pairs:
                    tile(J, I)[:] = tile(I, J).T
            elif rank == x:
                dist.send(torch.from_numpy(np.ascontiguousarray(
                    np.concatenate([tile(I, J).T for I, J in pairs], axis=1))), y)
            elif rank == y:
                buf = torch.zeros((ALIGN, ALIGN * len(pairs)), dtype=torch.int64)
                dist.recv(buf, x)
                for i, (I, J) in enumerate(pairs):
                    tile(J, I)[:] = buf[:, i * ALIGN:(i + 1) * ALIGN].numpy()
    q.put((rank, D[:, :n].copy()))
    dist.barrier()
    dist.destroy_process_group()


def _sparse_worker(rank, R, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=R)
    g = graphs.random_geometric(300, seed=3)
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    n = g.n
    per = (n + R - 1) // R
    s0, s1 = rank * per, min(n, (rank + 1) * per)
    rows = oracle.sssp_rows(el, s0, s1)  # stands in for this rank's GPU rows
    lat = torch.zeros((per, n), dtype=torch.int64)
    rel = torch.zeros((per, n), dtype=torch.float64)
    lat[:s1 - s0] = torch.from_numpy(rows["lat_int"].astype(np.int64))
    rel[:s1 - s0] = torch.from_numpy(rows["rel"])
    lat_all = [torch.zeros_like(lat) for _ in range(R)]
    rel_all = [torch.zeros_like(rel) for _ in range(R)]
    dist.all_gather(lat_all, lat)  # ncclAllGather layout: rank-major row slices
    dist.all_gather(rel_all, rel)
    q.put((rank, torch.cat(lat_all)[:n].numpy(), torch.cat(rel_all)[:n].numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_dense_sharded_schedule_gloo(native):
    n, seed, R = 400, 6, 2  # ld 512: two 128-row tile rows per rank, so the split update is real
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dense_worker, args=(r, R, port, n, seed, q)) for r in range(R)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(R)])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    lat = np.concatenate([x[3] for x in res])[:n].astype(np.uint64) * np.uint64(1_000_000)
    rel = np.concatenate([x[4] for x in res])[:n]
    g = graphs.complete_graph(n, seed=seed)
    exp = oracle.table(oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss), raw=True)
    assert np.array_equal(lat, exp["lat_int"])
    assert np.array_equal(rel, exp["rel"])


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n,R,rp", [(400, 2, 64), (700, 3, 64), (400, 2, 128), (700, 3, 128)])
def test_dense_symmetric_sharded_schedule_gloo(native, n, R, rp):
    seed = 7
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dense_sym_worker, args=(r, R, port, n, seed, q, rp))
             for r in range(R)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(R)], key=lambda x: x[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    D = np.concatenate([x[1] for x in res])[:n].astype(np.uint64) * np.uint64(1_000_000)
    g = graphs.complete_graph(n, seed=seed)
    exp = oracle.table(oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss))
    off = ~np.eye(n, dtype=bool)  # the diagonal follows its own rule after the rounds
    assert np.array_equal(D[off], exp["lat_int"][off])


@pytest.mark.timeout(300)
def test_sparse_source_shard_allgather_gloo(native):
    R = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sparse_worker, args=(r, R, port, q)) for r in range(R)]
    for p in procs:
        p.start()
    res = [q.get(timeout=250) for _ in range(R)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    g = graphs.random_geometric(300, seed=3)
    el = oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss)
    full = oracle.sssp_rows(el)
    for _, lat, rel in res:
        assert np.array_equal(lat.astype(np.uint64), full["lat_int"])
        assert np.array_equal(rel, full["rel"])


# ---- the row-sharded Dial level build (levels.hip srt_levels_build), its collectives in order --
# The protocol is restated in tests/levels_protocol.py; its sequences are the fixture the C
# library's collective logs are checked against (tests/test_gpu_protocol.py).
import json  # noqa: E402
import sys  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import levels_protocol as lp  # noqa: E402

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levels_protocol.json")


def _run_levels(name):
    R = lp.CASES[name][1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=lp.gloo_worker, args=(r, R, port, name, q)) for r in range(R)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(R)], key=lambda x: x[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", list(lp.CASES))
def test_dense_level_build_protocol_gloo(native, name):
    """VERDICT r04 #4 / r05 #4, ADVICE r05 (high): the level build's N-rank protocol over gloo --
    uneven row shards, ranks with different level caps (complete*: the min agreement; capfall: a
    budget of 1 sends every rank to the FW together), and ranks whose own sources settle on either
    side of the first batch of levels (hubleaf*: hubs at level 5, leaves at 10 -- every rank takes
    the batch decision from the summed vote, fetches the heavier arcs and runs batch 2). Every rank
    makes the same collective calls in the same order with the same sizes, the sequence is the
    committed fixture's (the one the C library's log must equal), and the rows equal the oracle's."""
    spec, R, _, outcome = lp.CASES[name]
    res = _run_levels(name)
    assert len({str(x[2]) for x in res}) == 1, [x[2] for x in res]  # identical collective sequence
    assert {x[1] for x in res} == {outcome}
    with open(_GOLDEN) as f:
        gold = json.load(f)[name]
    assert [list(c) for c in res[0][2]] == gold["calls"]
    assert [int(x[6]) for x in res] == gold["own_levels"]
    if name.startswith("hubleaf"):  # the ranks' own sources settle on either side of level 8
        assert min(gold["own_levels"]) <= lp.BATCH < max(gold["own_levels"])
    if outcome != "levels":
        return
    g, _, _ = lp.case_graph(spec)
    exp = oracle.table(oracle.EdgeList(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss), raw=True)
    n = g.n
    for _, _, _, b, D, rel, _ in res:
        rows = slice(b, b + D.shape[0])
        off = np.arange(n)[None, :] != np.arange(b, b + D.shape[0])[:, None]
        lat = D.astype(np.uint64) * np.uint64(1_000_000)
        assert np.array_equal(np.where(off, lat, 0), np.where(off, exp["lat_int"][rows], 0))
        assert np.array_equal(rel[off], exp["rel"][rows][off])
