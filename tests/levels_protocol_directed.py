"""The N-rank protocol of the level build of a DIRECTED dense graph on row shards
(shadow_amd/csrc/levels.hip, srt_levels_build, "directed graph, N > 1"), restated in plain numpy --
test infrastructure, no process group: every rank's part is computed here in one process.

A rank holds the out-arcs of its rows; a target's in-arcs are spread over every rank's rows. A
forced build (SRT_FORM levels=1) makes, on every rank alike, in the collective log's encoding
(srt_comm_log_read: (op, a, b) -- 2 all-reduce (count, op_min), 3 all-gather (bytes per rank, 0)):

  1. one sum all-reduce of the exchange: the weight histogram in 20-bit limbs, the allocation-
     failure count (+ 1 pad), and every rank's arcs per weight, all 256 weights as 16-bit halves;
  2. one min all-reduce of (budget, allocations, wire) -- the budget is 254 levels or the rank's
     lcap; a budget below 2 ends the level build here (the Floyd-Warshall's calls follow);
  3. every rank's (target, weight <= lx) counts, lx = min(budget, 8): one all-gather of u16
     blocks [weight][target] over all ld targets;
  4. the arcs of weight <= lx: one all-gather of every rank's block, 12 B per arc (source |
     weight << 16, then the f64 reliabilities), padded to the largest rank's arcs (made even);
  5. per batch of levels (1-5, then 6, 7, 8 one at a time, then 8 at a time) the vote (sum
     all-reduce of 4 int32); after the batch ending at lx < budget, 3 and 4 again for the weights
     lx + 1..budget (3) and every arc of weight <= budget (4).

Inside a rank's block the arcs run target by target, weight by weight inside a target. The
receiver copies the ranks' runs of a target one after the other into the target's segment and
sorts the segment by (weight, source): merged_in_arcs() restates that, and
tests/test_levels_protocol_directed.py holds it to the columns of the dense weights.
"""
import numpy as np

ALIGN, LVL_STRIDE, LVL_WMAX, BATCH, B1 = 128, 256, 254, 8, 5
X_LIMBS, X_DCNT = 2 * 256 + 2, 2 * 256  # levels.hip LVL_X_LIMBS, LVL_X_DCNT
INF = 0x7FFFFFFF
ALLREDUCE, ALLGATHER = 2, 3


def shard(ld, R, rank):
    nb = (ld + ALIGN - 1) // ALIGN
    return nb * rank // R * ALIGN, nb * (rank + 1) // R * ALIGN


def padded(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def arc_weights(w):
    """int64 [n, n]: the weight of the arc k -> j at [k, j] when it takes part in a level build
    (off the diagonal, 1..254 quanta), else 0. Row k holds k's out-arcs, column j j's in-arcs."""
    w = np.asarray(w).astype(np.int64)
    n = w.shape[0]
    return np.where(~np.eye(n, dtype=bool) & (w >= 1) & (w <= LVL_WMAX), w, 0)


def rank_block(arcw, R, q, lw):
    """Rank q's block of the arcs of weight <= lw, in wire order: (target, weight, source) int64
    arrays -- its targets in order, the weights in order inside a target."""
    n = arcw.shape[0]
    b, e = shard(padded(n), R, q)
    sub = arcw[b:min(e, n)]
    ks, js = np.nonzero((sub >= 1) & (sub <= lw))
    wt = sub[ks, js]
    o = np.lexsort((ks, wt, js))
    return js[o], wt[o], ks[o] + b


def block_sizes(arcw, R, lw):
    return [int(rank_block(arcw, R, q, lw)[0].size) for q in range(R)]


def wire_arcs(arcw, R, lw):
    """Arcs of one rank's padded block on the wire: the largest rank's, made even."""
    return (max(block_sizes(arcw, R, lw)) + 1) // 2 * 2


def merged_in_arcs(arcw, R, lw):
    """What every rank holds after the placement and the segmented sort: (off [n + 1], weight,
    source) -- target j's in-arcs of weight <= lw at off[j]..off[j + 1]."""
    n = arcw.shape[0]
    blocks = [rank_block(arcw, R, q, lw) for q in range(R)]
    tgt = np.concatenate([b[0] for b in blocks])
    wt = np.concatenate([b[1] for b in blocks])
    src = np.concatenate([b[2] for b in blocks])
    rk = np.concatenate([np.full(b[0].size, q) for q, b in enumerate(blocks)])
    pos = np.concatenate([np.arange(b[0].size) for b in blocks])
    placed = np.lexsort((pos, rk, tgt))  # a target's segment: the ranks' runs one after the other
    tgt, wt, src = tgt[placed], wt[placed], src[placed]
    key = (wt << 16) | src  # the sort's 24-bit key inside a segment
    o = np.lexsort((key, tgt))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(tgt, minlength=n))
    return off, wt[o], src[o]


def distances(arcw):
    """All-pairs distances in quanta (Floyd-Warshall over the arcs), INF where unreachable."""
    n = arcw.shape[0]
    d = np.where(arcw > 0, arcw, INF).astype(np.int64)
    np.fill_diagonal(d, 0)
    for k in range(n):
        np.minimum(d, d[:, k:k + 1] + d[k:k + 1, :], out=d)
    return np.minimum(d, INF)


def directed_calls(w, R, lcaps=None):
    """The collectives a forced directed level build logs on every rank of R, for the dense
    weights w (n x n quanta) and the per-rank level caps {rank: cap}: (outcome "levels" | "fw",
    the list of [op, a, b], each rank's own last level or 0)."""
    lcaps = lcaps or {}
    arcw = arc_weights(w)
    n = arcw.shape[0]
    ld = padded(n)
    calls = [[ALLREDUCE, X_LIMBS + R * X_DCNT, 0], [ALLREDUCE, 3, 1]]
    hist = np.bincount(arcw.ravel(), minlength=LVL_STRIDE)[:LVL_STRIDE]
    lmax = min([LVL_WMAX] + [int(c) for q, c in lcaps.items() if q < R])
    nz = np.nonzero(hist[1:])[0]
    wmin = int(nz[0]) + 1 if nz.size else 0
    if lmax < 2 or not wmin or wmin > lmax:
        return "fw", calls, [0] * R
    lx = min(lmax, BATCH)

    def extraction(w0, w1):
        calls.append([ALLGATHER, ld * (w1 - w0 + 1) * 2, 0])
        calls.append([ALLGATHER, wire_arcs(arcw, R, w1) * 12, 0])

    extraction(1, lx)
    d = distances(arcw)
    own = []
    for q in range(R):
        b, e = shard(ld, R, q)
        rows = d[b:min(e, n)]
        own.append(0 if rows.size and (rows >= INF).any() else max(2, int(rows.max())) if rows.size else 2)
    need = 0 if 0 in own else max(own)  # the level after which every rank is done (0: never)
    d0, done = 1, False
    while d0 <= lmax:
        d1 = min(lmax, B1) if d0 == 1 else d0 if d0 <= BATCH else min(lmax, d0 + BATCH - 1)
        calls.append([ALLREDUCE, 4, 0])
        if need and need <= d1:
            done = True
            break
        if d1 == lx and lx < lmax:
            extraction(lx + 1, lmax)
        d0 = d1 + 1
    if not done:
        return "fw", calls, [0] * R
    return "levels", calls, own
