/*
 * levels.hip -- exact all-pairs shortest distances on dense graphs by bit-parallel Dial levels.
 *
 * Replaces, when it is cheaper, the blocked Floyd-Warshall of fw16.hip for the distance phase of
 * _topology_computeSourcePaths (/root/reference/src/main/routing/topology.c:1578-1814, the igraph
 * Dijkstra of :1679-1701) on complete / dense graphs. Edge weights are integer quanta >= 1, so
 * Dijkstra's settle order is Dial's bucket order, and one bucket (distance level d) of EVERY source
 * can be settled at once with bit operations:
 *
 *   Delta_d[j] = ( OR over in-arcs (k -> j, w <= d) of Delta_{d-w}[k] )  AND NOT  R_{d-1}[j]
 *   R_d[j]     = R_{d-1}[j] OR Delta_d[j]
 *
 * where Delta_d[j] is the bit set of sources s with D[s][j] == d, R_d[j] those with D[s][j] <= d,
 * and Delta_0[k] = R_0[k] = {k}. This is the last-hop decomposition D[s][j] = min_k D[s][k] +
 * w(k, j) (every weight >= 1, so Delta_{d-w} is final when level d is formed), i.e. the same
 * distances Dijkstra settles; the canonical predecessors and path-order reliabilities are formed
 * afterwards from the distances by the dense post pass exactly as after Floyd-Warshall.
 *
 * Only arcs with w <= lmax take part. If every pair is settled by level D <= lmax, every arc with
 * w > lmax >= D is longer than the distance it joins, so it lies on no shortest path and the
 * result is exact. Otherwise the build falls back to Floyd-Warshall (the caller's).
 *
 * Layout (HBM). Bit sets run over this rank's sources (nsrc, a multiple of 128): nw = nsrc / 32
 * words per vertex. lev[d - 1][j][word] for d = 1..lmax, R[j][word]; one wave owns a (target j,
 * 64-word source chunk) unit, so every arc costs one coalesced 256-B gather of Delta_{d-w}[k].
 * In-arcs come from the rows of w (undirected: row j holds j's in-arcs, and a row-sharded rank has
 * them for its rows) or its columns (directed), grouped by (target, weight). On one GPU the columns
 * are whole; a row-sharded rank of a directed graph has its rows' part of every column, so the
 * ranks' parts are gathered and merged on every rank ("directed graph, N > 1" below). After the
 * extraction every form is the same: each target's in-arcs up to the extracted weight, sorted by
 * (weight, source), read with the rank's source window.
 */
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <vector>

#include "srt_device.h"

#define LVL_STRIDE 256 /* per-target offsets: weight 0..255 */
/* levels enqueued per host round trip: a batch's levels past the one that settles every pair
 * return at once (lvl_step_kernel's prev test); the first batch is LVL_B1 levels (C4's distances
 * end at 4-5: one vote), then one level per batch up to LVL_BATCH, then LVL_BATCH per batch */
#define LVL_BATCH 8
#define LVL_B1 5
#define LVL_WMAX 254   /* largest level budget (distances stay u8: the post pass's small path) */
#define LVL_PB 12 /* lvl_pred_kernel: gathers per pipelined batch */
#define LVL_NEAR_NW 2048 /* lvl_near_kernel: a target's plane row in LDS, four per workgroup */
#define LVL_NEAR_MIN_NW 512 /* ... and only for shares of at least 16,384 sources */
#define LVL_ROWS_MIN_ROUNDS 16u /* lvl_pred_rows_kernel: multi-sub-chunk units keep this many rounds */

/* ---- in-arc extraction ------------------------------------------------------------------- */
/* COUNT: per (target, weight) histogram of arcs with 1 <= w <= LVL_WMAX; FILL: the arcs (k | w << 16)
 * at cursor positions from off (weights above lmax were masked out of off). Rows form: local row
 * jj of w is target row0 + jj's in-arc row (undirected). */
/* The count pass also keeps each row's light arcs (w <= LVL_STASH_W; C4: ~1,050 per row) in a
 * stash, so the fill reads them instead of the whole w row again (when lmax <= LVL_STASH_W and
 * the row's arcs fit). Wave q of the row's workgroup scans the row's q-th quarter and appends
 * its light arcs in vertex order (a ballot prefix per step) to its own LVL_STASH_SEG-entry
 * segment, so the stash holds the row's light arcs in vertex order. The fill then places them by
 * weight in that order (per-wave counts, then a ballot rank per weight): every target's in-arcs
 * come out sorted by (weight, source) with no sort pass. A segment that overflows marks the
 * row (-1) and counts in *sovf: that build takes the full-row fill and the segmented sort. */
#define LVL_STASH_W 32
#define LVL_STASH_SEG 512
#define LVL_STASH_CAP (4 * LVL_STASH_SEG)
template <bool FILL>
__global__ __launch_bounds__(256) void lvl_arcs_rows_kernel(int n, int ld, int row0,
                                                            const uint32_t* __restrict__ w,
                                                            int32_t* __restrict__ cnt, int lmax,
                                                            const int32_t* __restrict__ off,
                                                            uint32_t* __restrict__ arcs,
                                                            const double* __restrict__ r = nullptr,
                                                            double* __restrict__ ar = nullptr,
                                                            unsigned long long* __restrict__ dkey = nullptr,
                                                            uint32_t* __restrict__ stash = nullptr,
                                                            int32_t* __restrict__ scnt = nullptr,
                                                            unsigned long long* __restrict__ sovf = nullptr) {
    __shared__ int h[LVL_STRIDE];
    __shared__ unsigned long long s_key[4];
    __shared__ int wc[4][LVL_STASH_W + 1];
    const int jj = blockIdx.x, j = row0 + jj;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (FILL && stash && j < n && lmax <= LVL_STASH_W &&
        min(min(scnt[(size_t)jj * 4], scnt[(size_t)jj * 4 + 1]),
            min(scnt[(size_t)jj * 4 + 2], scnt[(size_t)jj * 4 + 3])) >= 0) {
        for (int i = tid; i <= lmax; i += 256) h[i] = off[(size_t)j * LVL_STRIDE + i];
        for (int i = tid; i < 4 * (LVL_STASH_W + 1); i += 256) wc[i / (LVL_STASH_W + 1)][i % (LVL_STASH_W + 1)] = 0;
        __syncthreads();
        const uint32_t* sr = stash + (size_t)jj * LVL_STASH_CAP + wv * LVL_STASH_SEG;
        const int m = scnt[(size_t)jj * 4 + wv];
        for (int q = lane; q < m; q += 64) {
            const uint32_t x = sr[q] >> 16;
            if (x <= (uint32_t)lmax) atomicAdd(&wc[wv][x], 1);
        }
        __syncthreads();
        /* lane x (x <= lmax <= 32) keeps this wave's next position for weight x: the weight's
         * start plus the earlier waves' arcs of that weight */
        int run = 0;
        if (lane <= lmax) {
            run = h[lane];
            for (int v = 0; v < wv; ++v) run += wc[v][lane];
        }
        for (int q0 = 0; q0 < m; q0 += 64) {
            const int q = q0 + lane;
            const uint32_t e = q < m ? sr[q] : 0u, x = e >> 16;
            const bool valid = q < m && x >= 1u && x <= (uint32_t)lmax;
            unsigned long long pend = __ballot(valid);
            int pos = 0;
            while (pend) {
                const int x0 = __builtin_amdgcn_readlane((int)x, __builtin_ctzll(pend));
                const unsigned long long mm = __ballot(valid && (int)x == x0);
                const int base = __builtin_amdgcn_readlane(run, x0);
                if (valid && (int)x == x0) pos = base + __popcll(mm & lt);
                if (lane == x0) run += __popcll(mm);
                pend &= ~mm;
            }
            if (valid) {
                arcs[pos] = e;
                ar[pos] = r[(size_t)jj * ld + (e & 0xFFFFu)]; /* undirected: r(k -> j) = r(j -> k) */
            }
        }
        return;
    }
    /* COUNT also takes the diagonal rule's key from the same row reads (topology.c:1431-1576, as
     * dense_diag_kernel): min over the row's out-edges of (self-loop L, other 2L) << 32 | u */
    unsigned long long best = ~0ull;
    for (int i = tid; i < LVL_STRIDE; i += 256)
        h[i] = FILL ? (j < n ? off[(size_t)j * LVL_STRIDE + i] : 0) : 0;
    __syncthreads();
    const int wmax = FILL ? lmax : LVL_WMAX;
    if (FILL) {
        if (j < n) {
            const uint32_t* row = w + (size_t)jj * ld;
            for (int k4 = tid * 4; k4 < n; k4 += 1024) {
                const uint4 v = *reinterpret_cast<const uint4*>(row + k4);
                const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = k4 + q;
                    if (k < n && k != j && x[q] >= 1u && x[q] <= (uint32_t)wmax) {
                        const int p = atomicAdd(&h[x[q]], 1);
                        arcs[p] = (uint32_t)k | (x[q] << 16);
                        ar[p] = r[(size_t)jj * ld + k]; /* undirected: r(k -> j) = r(j -> k) */
                    }
                }
            }
        }
        return;
    }
    int run = 0;
    if (j < n) {
        const uint32_t* row = w + (size_t)jj * ld;
        const int Q = ((n + 1023) >> 10) << 8; /* a wave's quarter of the row, 256-aligned */
        const int lo = wv * Q, hi = min(n, lo + Q);
        uint32_t* seg = stash ? stash + (size_t)jj * LVL_STASH_CAP + wv * LVL_STASH_SEG : nullptr;
        for (int b0 = lo; b0 < hi; b0 += 256) {
            const int k4 = b0 + lane * 4;
            uint4 v = make_uint4(SRT_INF, SRT_INF, SRT_INF, SRT_INF);
            if (k4 < hi) v = *reinterpret_cast<const uint4*>(row + k4);
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
            int c = 0;
            bool cand[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k4 + q;
                if (k < n && x[q] < SRT_INF) {
                    const unsigned long long lat = k == j ? x[q] : 2ull * x[q];
                    best = min(best, (lat << 32) | (uint32_t)k);
                }
                const bool arc = k < n && k != j && x[q] >= 1u && x[q] <= (uint32_t)wmax;
                if (arc) atomicAdd(&h[x[q]], 1);
                cand[q] = arc && x[q] <= LVL_STASH_W;
                c += cand[q];
            }
            if (seg) { /* vertex order: the lane's exclusive prefix of the counts (0..4) */
                const unsigned long long b1 = __ballot(c & 1), b2 = __ballot(c & 2), b4 = __ballot(c & 4);
                int p = run + __popcll(b1 & lt) + 2 * __popcll(b2 & lt) + 4 * __popcll(b4 & lt);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (cand[q]) {
                        if (p < LVL_STASH_SEG) seg[p] = (uint32_t)(k4 + q) | (x[q] << 16);
                        ++p;
                    }
                run += __popcll(b1) + 2 * __popcll(b2) + 4 * __popcll(b4);
            }
        }
    }
    if (stash && lane == 0) {
        const bool over = run > LVL_STASH_SEG;
        scnt[(size_t)jj * 4 + wv] = over ? -1 : run;
        if (over) atomicAdd(sovf, 1ull);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(best, o);
        best = y < best ? y : best;
    }
    if (lane == 0) s_key[wv] = best;
    __syncthreads();
    for (int i = tid; i < LVL_STRIDE; i += 256) cnt[(size_t)j * LVL_STRIDE + i] = h[i];
    if (tid == 0 && dkey)
        dkey[jj] = min(min(s_key[0], s_key[1]), min(s_key[2], s_key[3]));
}

/* The diagonal rule of the held rows from the keys the count pass took: D[s][s] = the key's
 * latency (0 with no out-edge), rel = r or r^2 (0.0), as dense_diag_kernel */
__global__ void lvl_diag_kernel(int n, int ld, int row0, int lrows,
                                const unsigned long long* __restrict__ dkey,
                                const double* __restrict__ r, uint32_t* __restrict__ d,
                                double* __restrict__ rel) {
    const int jj = blockIdx.x * blockDim.x + threadIdx.x;
    if (jj >= lrows) return;
    const int v = row0 + jj;
    const unsigned long long best = dkey[jj];
    const size_t ix = (size_t)jj * ld + v;
    if (best == ~0ull) {
        d[ix] = 0;
        rel[ix] = 0.0;
    } else {
        const int u = (int)(best & 0xFFFFFFFFu);
        const double x = r[(size_t)jj * ld + u];
        d[ix] = (uint32_t)(best >> 32);
        rel[ix] = u == v ? x : x * x;
    }
}

/* Columns form (directed graph on one GPU): workgroup of 64 target columns j0.., lane = column,
 * the four waves sweep the rows k (one coalesced 256-B segment of a row per wave and step). */
template <bool FILL>
__global__ __launch_bounds__(256) void lvl_arcs_cols_kernel(int n, int ld,
                                                            const uint32_t* __restrict__ w,
                                                            int32_t* __restrict__ cnt, int lmax,
                                                            const int32_t* __restrict__ off,
                                                            uint32_t* __restrict__ arcs,
                                                            const double* __restrict__ r = nullptr,
                                                            double* __restrict__ ar = nullptr) {
    __shared__ int h[64 * LVL_STRIDE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 64, j = j0 + lane;
    for (int i = threadIdx.x; i < 64 * LVL_STRIDE; i += 256) {
        const int c = i / LVL_STRIDE, ww = i % LVL_STRIDE;
        h[i] = FILL ? (j0 + c < n ? off[(size_t)(j0 + c) * LVL_STRIDE + ww] : 0) : 0;
    }
    __syncthreads();
    const int wmax = FILL ? lmax : LVL_WMAX;
    if (j < n) {
        for (int k = wv; k < n; k += 4) {
            const uint32_t x = w[(size_t)k * ld + j];
            if (k != j && x >= 1u && x <= (uint32_t)wmax) {
                if (FILL) {
                    const int p = atomicAdd(&h[lane * LVL_STRIDE + x], 1);
                    arcs[p] = (uint32_t)k | (x << 16);
                    ar[p] = r[(size_t)k * ld + j];
                } else
                    atomicAdd(&h[lane * LVL_STRIDE + x], 1);
            }
        }
    }
    if (FILL) return;
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * LVL_STRIDE; i += 256) {
        const int c = i / LVL_STRIDE, ww = i % LVL_STRIDE;
        if (j0 + c < ld) cnt[(size_t)(j0 + c) * LVL_STRIDE + ww] = h[i];
    }
}

/* weight histogram over the count rows (for the level budget) */
__global__ void lvl_hist_kernel(size_t count, const int32_t* __restrict__ cnt,
                                unsigned long long* __restrict__ hist, unsigned mult = 1) {
    __shared__ unsigned long long s[LVL_STRIDE];
    for (int i = threadIdx.x; i < LVL_STRIDE; i += blockDim.x) s[i] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (size_t)gridDim.x * blockDim.x)
        if (cnt[i]) atomicAdd(&s[i % LVL_STRIDE], (unsigned long long)cnt[i]);
    __syncthreads();
    for (int i = threadIdx.x; i < LVL_STRIDE; i += blockDim.x)
        if (s[i]) atomicAdd(&hist[i], s[i] * mult);
}

/* N > 1: the histogram all-reduced in 20-bit limbs (int32 sums of R ranks cannot overflow), then
 * only the (target, weight <= lmax) counts -- the in-arc offsets need no heavier weight: 2.9 MB
 * on C4 instead of the 33.5-MB (target x 256 weights) block */
__global__ void lvl_hist_limbs_kernel(int to, unsigned long long* __restrict__ hist,
                                      int32_t* __restrict__ limbs) {
    const int i = threadIdx.x;
    if (i >= LVL_STRIDE) return;
    if (to) {
        limbs[i] = (int32_t)(hist[i] & 0xFFFFFull);
        limbs[LVL_STRIDE + i] = (int32_t)(hist[i] >> 20);
    } else {
        hist[i] = (unsigned long long)(uint32_t)limbs[i] +
                  ((unsigned long long)(uint32_t)limbs[LVL_STRIDE + i] << 20);
    }
}
/* N > 1: every target's counts of weights w0..w1 from its owner: each rank's block holds its own
 * targets' counts as u16 ([weight][row], padded to the largest shard), all-gathered (2 B per
 * (target, weight) instead of the int32 sum all-reduce of every column up to lmax + 1) */
__global__ void lvl_cnt_gpack_kernel(int row0, int nrows, int max_rows, int w0, int w1, int me,
                                     const int32_t* __restrict__ cnt, uint16_t* __restrict__ cg) {
    const int jj = blockIdx.x * blockDim.x + threadIdx.x;
    if (jj >= nrows) return;
    uint16_t* blk = cg + (size_t)me * max_rows * (w1 - w0 + 1);
    for (int w = w0; w <= w1; ++w)
        blk[(size_t)(w - w0) * max_rows + jj] = (uint16_t)cnt[(size_t)(row0 + jj) * LVL_STRIDE + w];
}
__global__ void lvl_cnt_gunpack_kernel(int ld, int R, int max_rows, int w0, int w1,
                                       const uint16_t* __restrict__ cg, int32_t* __restrict__ cnt) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ld) return;
    const long long nb = ld / SRT_SHARD_ALIGN; /* the owner of row j (srt_shard_rows) */
    int q = 0;
    while (q + 1 < R && (int)(nb * (q + 1) / R) * SRT_SHARD_ALIGN <= j) ++q;
    const int jj = j - (int)(nb * q / R) * SRT_SHARD_ALIGN;
    const uint16_t* blk = cg + (size_t)q * max_rows * (w1 - w0 + 1);
    for (int w = w0; w <= w1; ++w) cnt[(size_t)j * LVL_STRIDE + w] = blk[(size_t)(w - w0) * max_rows + jj];
}

/* ---- directed graph, N > 1 --------------------------------------------------------------------- *
 * A rank holds the out-arcs of its rows, and a target's in-arcs are spread over every rank's
 * rows. Each rank counts and fills the columns of its own rows (lvl_arcs_colwin_kernel), every
 * rank's (target, weight) counts are all-gathered (u16, [weight][target]), each rank packs its
 * arcs of weight <= lw into one block -- its targets in order, the weights in order inside a
 * target, 4 B of source | weight << 16 and 8 B of reliability per arc -- the blocks are
 * all-gathered once, padded to the largest rank's, and lvl_dplace_kernel copies every rank's run
 * of a target into the target's segment of the (target, weight)-major arcs, the ranks in order.
 * The segmented sort of the one-GPU directed build then orders each segment by (weight, source):
 * the keys of a segment are distinct, so the result does not depend on where the cursors' atomics
 * put an arc inside its run. */
/* Row-window columns form: workgroup = 64 target columns x a chunk of the rank's rows, lane =
 * column, the four waves sweep the chunk's rows (one coalesced 256-B segment of a row per wave and
 * step) into a per-workgroup LDS histogram. COUNT adds the histogram to cnt (zeroed before);
 * FILL takes the chunk's runs from the cursors in cnt (atomically, each (target, weight) run of
 * the rank is shared by the chunks) and places the arcs in a second sweep. */
#define LVL_DROWS 256 /* rows per workgroup */
template <bool FILL>
__global__ __launch_bounds__(256) void lvl_arcs_colwin_kernel(int n, int ld, int row0, int lrows,
                                                              const uint32_t* __restrict__ w,
                                                              int32_t* __restrict__ cnt, int lmax,
                                                              uint32_t* __restrict__ arcs = nullptr,
                                                              const double* __restrict__ r = nullptr,
                                                              double* __restrict__ ar = nullptr) {
    __shared__ int h[64 * LVL_STRIDE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 64, j = j0 + lane;
    const int k0 = blockIdx.y * LVL_DROWS, k1 = min(lrows, k0 + LVL_DROWS);
    for (int i = threadIdx.x; i < 64 * LVL_STRIDE; i += 256) h[i] = 0;
    __syncthreads();
    const int wmax = FILL ? lmax : LVL_WMAX;
    if (j < n)
        for (int kk = k0 + wv; kk < k1; kk += 4) {
            const uint32_t x = w[(size_t)kk * ld + j];
            if (row0 + kk != j && x >= 1u && x <= (uint32_t)wmax) atomicAdd(&h[lane * LVL_STRIDE + x], 1);
        }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * LVL_STRIDE; i += 256) {
        const int v = h[i];
        if (!v) continue;
        int32_t* g = cnt + (size_t)(j0 + i / LVL_STRIDE) * LVL_STRIDE + i % LVL_STRIDE;
        if (FILL) h[i] = atomicAdd(g, v); /* the chunk's run inside the rank's (target, weight) run */
        else atomicAdd(g, v);
    }
    if (!FILL) return;
    __syncthreads();
    if (j < n)
        for (int kk = k0 + wv; kk < k1; kk += 4) {
            const uint32_t x = w[(size_t)kk * ld + j];
            if (row0 + kk != j && x >= 1u && x <= (uint32_t)wmax) {
                const int p = atomicAdd(&h[lane * LVL_STRIDE + x], 1);
                arcs[p] = (uint32_t)(row0 + kk) | (x << 16);
                ar[p] = r[(size_t)kk * ld + j];
            }
        }
}
/* this rank's arcs per weight (its own histogram, before the exchange sums it) into its slot of
 * the exchange as 16-bit halves: every weight, so both extractions' block sizes come from it */
__global__ void lvl_drank_counts_kernel(const unsigned long long* __restrict__ hist, int32_t* __restrict__ slot) {
    const int w = threadIdx.x;
    if (w < 1 || w >= LVL_STRIDE) return;
    const uint32_t t = (uint32_t)hist[w];
    slot[2 * w] = (int32_t)(t & 0xFFFFu);
    slot[2 * w + 1] = (int32_t)(t >> 16);
}
/* every rank's (target, weight) counts, as gathered: weights 1..wa in a ([rank][weight][target]),
 * weights wa + 1..wb in b (the second extraction's; NULL before it) */
struct lvl_dcnt {
    const uint16_t* a;
    const uint16_t* b;
    int wa, wb, ld;
    __device__ __forceinline__ int at(int q, int w, int j) const {
        return w <= wa ? a[((size_t)q * wa + (w - 1)) * ld + j]
                       : b[((size_t)q * (wb - wa) + (w - wa - 1)) * ld + j];
    }
};
/* this rank's counts of the weights w0..w1 into its block ([weight][target], u16: a rank holds
 * fewer than 65,536 rows) */
__global__ void lvl_dcnt_pack_kernel(int ld, int w0, int w1, const int32_t* __restrict__ cnt,
                                     uint16_t* __restrict__ blk) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ld) return;
    for (int w = w0; w <= w1; ++w) blk[(size_t)(w - w0) * ld + j] = (uint16_t)cnt[(size_t)j * LVL_STRIDE + w];
}
/* the global counts of the weights w0..w1: the ranks' blocks summed */
__global__ void lvl_dcnt_sum_kernel(int ld, int R, int w0, int w1, const uint16_t* __restrict__ cg,
                                    int32_t* __restrict__ cnt) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ld) return;
    const int nwt = w1 - w0 + 1;
    for (int w = w0; w <= w1; ++w) {
        int s = 0;
        for (int q = 0; q < R; ++q) s += cg[((size_t)q * nwt + (w - w0)) * ld + j];
        cnt[(size_t)j * LVL_STRIDE + w] = s;
    }
}
/* tq[q (ld + 1) + j]: rank q's arcs of weight <= lw into target j (0 at j == ld and at the end);
 * its exclusive scan gives every run's start inside rank q's block (less the scan at j == 0) */
__global__ void lvl_dtot_kernel(int R, int lw, lvl_dcnt dc, int32_t* __restrict__ tq) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)R * (dc.ld + 1);
    if (i > nt) return;
    const int q = (int)(i / (size_t)(dc.ld + 1)), j = (int)(i % (size_t)(dc.ld + 1));
    int t = 0;
    if (i < nt && j < dc.ld)
        for (int w = 1; w <= lw; ++w) t += dc.at(q, w, j);
    tq[i] = t;
}
/* the fill's cursors: the start of this rank's (target, weight) runs inside its block */
__global__ void lvl_dcur_kernel(int me, int lw, lvl_dcnt dc, const int32_t* __restrict__ oq,
                                int32_t* __restrict__ cur) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= dc.ld) return;
    const size_t b = (size_t)me * (dc.ld + 1);
    int run = oq[b + j] - oq[b];
    for (int w = 1; w <= lw; ++w) {
        cur[(size_t)j * LVL_STRIDE + w] = run;
        run += dc.at(me, w, j);
    }
}
/* the gathered blocks (rank q's at wire + q * blk bytes: blk / 12 arcs, then their f64s) into the
 * (target, weight)-major arcs: a wave per target, the ranks' runs one after the other */
__global__ void lvl_dplace_kernel(int n, int ld, int R, size_t blk, const int32_t* __restrict__ off,
                                  const int32_t* __restrict__ tq, const int32_t* __restrict__ oq,
                                  const char* __restrict__ wire, uint32_t* __restrict__ arcs,
                                  double* __restrict__ ar) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n) return;
    int dst = off[(size_t)j * LVL_STRIDE];
    for (int q = 0; q < R; ++q) {
        const size_t b = (size_t)q * (ld + 1);
        const int c = tq[b + j], s = oq[b + j] - oq[b];
        const uint32_t* wa = reinterpret_cast<const uint32_t*>(wire + (size_t)q * blk);
        const double* wr = reinterpret_cast<const double*>(wire + (size_t)q * blk + blk / 3);
        for (int i = lane; i < c; i += 64) {
            arcs[dst + i] = wa[s + i];
            ar[dst + i] = wr[s + i];
        }
        dst += c;
    }
}

/* ---- the arcs' distinct reliabilities (packed post pass) ------------------------------------ *
 * The post pass carries r(pred, t) per pair as a 16-bit index into a table of the distinct arc
 * reliabilities instead of the f64 itself (C4: 501 values): the predecessor and the index share one
 * 4-B word (10 B per pair before, plus their two transposes). The table is exact -- each entry is
 * an arc's double, bit for bit. An open-addressing hash over the value bits (LVL_RT_SLOTS slots,
 * linear probing) gives each arc a slot, one workgroup numbers the occupied slots in slot order,
 * and the arcs' slots become dense indices. More than LVL_RT_CAP distinct values (or a probe run
 * past LVL_RT_PROBE) keeps the f64 form. */
#define LVL_RT_SLOTS 8192 /* global slots: <= 2048 values at a load of 1/4 */
#define LVL_RT_PROBE 256
#define LVL_RT_CAP 2048
#define LVL_RT_LDS 2048 /* a workgroup's private table */
static __device__ __forceinline__ unsigned lvl_rt_hash(unsigned long long b) {
    b ^= b >> 33;
    b *= 0xff51afd7ed558ccdull;
    b ^= b >> 33;
    return (unsigned)b & (LVL_RT_SLOTS - 1u);
}
static __device__ __forceinline__ int lvl_rt_global_slot(unsigned long long v, unsigned long long* H) {
    unsigned h = lvl_rt_hash(v);
    for (int p = 0; p < LVL_RT_PROBE; ++p, h = (h + 1u) & (LVL_RT_SLOTS - 1u)) {
        unsigned long long x = __hip_atomic_load(&H[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (x == ~0ull) x = atomicCAS(&H[h], ~0ull, v); /* ~0: empty (a NaN, never a reliability) */
        if (x == ~0ull || x == v) return (int)h;
    }
    return -1;
}
/* Each arc of [lo, hi) (device-held bounds when lo_p / hi_p are given) gets its value's global
 * slot. A workgroup takes a contiguous run of arcs and dedupes it in a private LDS table first, so
 * the global table sees each distinct value once per workgroup instead of once per arc: every arc
 * probing the global table hammered its ~500 hot lines (C4: 87 us for 1.07 M arcs). Values past
 * the LDS table's probe go to the global table directly (marked 0x8000 in the first pass). */
__global__ __launch_bounds__(256) void lvl_rt_hash_kernel(const int32_t* __restrict__ lo_p,
                                                          const int32_t* __restrict__ hi_p, int lo, int hi,
                                                          const double* __restrict__ ar,
                                                          unsigned long long* __restrict__ H,
                                                          uint16_t* __restrict__ rix, int* __restrict__ ovf) {
    __shared__ unsigned long long key[LVL_RT_LDS];
    __shared__ uint16_t gs[LVL_RT_LDS];
    const int a = lo_p ? *lo_p : lo, b = hi_p ? *hi_p : hi, tid = threadIdx.x;
    const int per = max(0, (b - a + (int)gridDim.x - 1) / (int)gridDim.x);
    const int c0 = a + (int)blockIdx.x * per, c1 = min(b, c0 + per);
    for (int s = tid; s < LVL_RT_LDS; s += 256) key[s] = ~0ull;
    __syncthreads();
    bool bad = false;
    for (int i = c0 + tid; i < c1; i += 256) {
        const unsigned long long v = (unsigned long long)__double_as_longlong(ar[i]);
        unsigned h = lvl_rt_hash(v) & (LVL_RT_LDS - 1u);
        int p = 0;
        for (; p < 64; ++p, h = (h + 1u) & (LVL_RT_LDS - 1u)) {
            unsigned long long x = __hip_atomic_load(&key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (x == ~0ull) x = atomicCAS(&key[h], ~0ull, v);
            if (x == ~0ull || x == v) break;
        }
        uint16_t out = (uint16_t)h;
        if (p == 64) {
            const int g = lvl_rt_global_slot(v, H);
            bad |= g < 0;
            out = (uint16_t)(0x8000u | (unsigned)max(g, 0));
        }
        rix[i] = out;
    }
    __syncthreads();
    for (int s = tid; s < LVL_RT_LDS; s += 256) {
        const unsigned long long v = key[s];
        if (v == ~0ull) continue;
        const int g = lvl_rt_global_slot(v, H);
        bad |= g < 0;
        gs[s] = (uint16_t)max(g, 0);
    }
    if (bad) *ovf = 1;
    __syncthreads();
    for (int i = c0 + tid; i < c1; i += 256) { /* (this thread's own first-pass entries) */
        const uint16_t x = rix[i];
        rix[i] = (x & 0x8000u) ? (uint16_t)(x & 0x7FFFu) : gs[x];
    }
}
static unsigned lvl_rt_grid(int64_t count) {
    const int64_t g = (count + 4095) / 4096;
    return (unsigned)(g < 1 ? 1 : g > 512 ? 512 : g);
}
/* one workgroup: dense index of every occupied slot (slot order), the table, its size */
__global__ __launch_bounds__(1024) void lvl_rt_compact_kernel(const unsigned long long* __restrict__ H,
                                                              uint16_t* __restrict__ map,
                                                              double* __restrict__ rtab,
                                                              int* __restrict__ ntab) {
    constexpr int PER = LVL_RT_SLOTS / 1024;
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63;
    int c = 0;
    for (int k = 0; k < PER; ++k) c += H[tid * PER + k] != ~0ull;
    int inc = c;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    if (lane == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    int base = inc - c, total = 0;
    for (int w = 0; w < 16; ++w) {
        base += w < (tid >> 6) ? wsum[w] : 0;
        total += wsum[w];
    }
    for (int k = 0; k < PER; ++k) {
        const unsigned long long v = H[tid * PER + k];
        if (v == ~0ull) continue;
        map[tid * PER + k] = (uint16_t)base;
        if (base < LVL_RT_CAP) rtab[base] = __longlong_as_double((long long)v);
        ++base;
    }
    if (tid == 0) *ntab = total;
}
__global__ void lvl_rt_remap_kernel(int total, const uint16_t* __restrict__ map,
                                    uint16_t* __restrict__ rix) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) rix[i] = map[rix[i]];
}

/* N > 1 (numbered segments): each arc's index into the union table, sorted by value bits, of
 * every rank's distinct reliabilities -- the same numbering on every rank */
__global__ void lvl_rt_index_kernel(int total, const double* __restrict__ ar,
                                    const unsigned long long* __restrict__ tab, int ntab,
                                    uint16_t* __restrict__ rix) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const unsigned long long b = (unsigned long long)__double_as_longlong(ar[i]);
    int lo = 0, hi = ntab - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    rix[i] = (uint16_t)lo;
}

/* ---- timing-only solo rank (srt_comm_init_solo*, tools/solo_rank.py) ------------------------ *
 * A solo rank runs exactly one real rank's work on its own rows; what a real rank would receive
 * from its peers it synthesises from its own rows instead (the collectives only charge the wire
 * model). Peer target j = js + shift (js one of the rank's own rows) takes js's counts, then js's
 * in-arc segment with every source moved by the same shift (mod n; each weight's run rotated so
 * it stays sorted by source). The graph is then a union of shifted copies of the rank's rows:
 * every vertex keeps distinct random in-neighbours, and on C4 its distances match the real
 * graph's (sampled: max 4, mean 3.292 against 3.290); plain copies (no shift) collapsed the
 * vertices onto the rank's rows and stretched the distances to 6. */
__global__ void lvl_solo_counts_kernel(int n, int row0, int nrows, int lrows, int32_t* __restrict__ cnt) {
    const int j = blockIdx.x;
    if (j >= n || (j >= row0 && j < row0 + nrows)) return;
    const int js = row0 + ((j - row0) % lrows + lrows) % lrows;
    for (int x = threadIdx.x; x < LVL_STRIDE; x += blockDim.x)
        cnt[(size_t)j * LVL_STRIDE + x] = cnt[(size_t)js * LVL_STRIDE + x];
}
__global__ void lvl_solo_arcs_kernel(int n, int row0, int nrows, int lrows, int w0, int w1, int nw,
                                     const int32_t* __restrict__ off, uint32_t* __restrict__ arcs,
                                     uint16_t* __restrict__ rix, double* __restrict__ ar,
                                     uint32_t* __restrict__ aoff) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n || (j >= row0 && j < row0 + nrows)) return;
    const int js = row0 + ((j - row0) % lrows + lrows) % lrows;
    const int shift = ((j - js) % n + n) % n;
    for (int x = w0; x <= w1; ++x) {
        const int g0 = off[(size_t)j * LVL_STRIDE + x], c = off[(size_t)j * LVL_STRIDE + x + 1] - g0;
        if (c <= 0) continue;
        const int s0 = off[(size_t)js * LVL_STRIDE + x];
        int nwr = 0; /* sources that wrap past n: the run's tail, which goes first */
        for (int i0 = 0; i0 < c; i0 += 64) {
            const int i = i0 + lane;
            nwr += __popcll(__ballot(i < c && (int)(arcs[s0 + i] & 0xFFFFu) + shift >= n));
        }
        for (int i = lane; i < c; i += 64) {
            const uint32_t e = arcs[s0 + i];
            int k = (int)(e & 0xFFFFu) + shift;
            const bool wr = k >= n;
            if (wr) k -= n;
            const int d = g0 + (wr ? i - (c - nwr) : nwr + i);
            arcs[d] = (uint32_t)k | (e & 0xFFFF0000u);
            if (rix) rix[d] = rix[s0 + i];
            if (ar) ar[d] = ar[s0 + i];
            if (aoff) aoff[d] = (uint32_t)k * (uint32_t)nw * 4u;
        }
    }
}

/* N > 1, streamed: the arcs of weight d from this rank's own sources (Delta_0) set as bits of
 * plane d - 1 before the levels, so level d needs none of its peers' weight-d arcs. The targets
 * j0..j1 are this rank's rows and the graph is undirected, so an in-arc (k, w) of own target j is
 * the arc j -> k: bit j of row k. Weight 1 also goes into R (level 1 is these bits alone). */
__global__ void lvl_direct_kernel(int j0, int j1, int nw, int lw, size_t plane, const int32_t* __restrict__ off,
                                  const uint32_t* __restrict__ arcs, uint32_t* __restrict__ lev,
                                  uint32_t* __restrict__ R) {
    const int j = j0 + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= j1) return;
    const int a0 = off[(size_t)j * LVL_STRIDE + 1], a1 = off[(size_t)j * LVL_STRIDE + lw + 1];
    const int s = j - j0;
    const uint32_t bit = 1u << (s & 31);
    for (int i = a0 + lane; i < a1; i += 64) {
        const uint32_t e = arcs[i];
        const int k = (int)(e & 0xFFFFu), w = (int)(e >> 16);
        const size_t o = (size_t)k * nw + (s >> 5);
        atomicOr(lev + (size_t)(w - 1) * plane + o, bit);
        if (w == 1) atomicOr(R + o, bit);
    }
}

/* The solo rank's Delta_0 bits without synthesising its peers' segments first: peer target j's
 * runs are own row js's, every source moved by shift (lvl_solo_arcs_kernel), so its own-source
 * arcs are row js's arcs whose moved source falls in [row0, row0 + nrows). A wave per target, a
 * lane per arc of weight <= lw (as lvl_direct_kernel; a binary search per (target, weight) ran
 * 63 us on one rank of N = 8). */
__global__ void lvl_solo_direct_kernel(int n, int row0, int nrows, int lrows, int nw, int lw, size_t plane,
                                       const int32_t* __restrict__ off, const uint32_t* __restrict__ arcs,
                                       uint32_t* __restrict__ lev, uint32_t* __restrict__ R) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n) return;
    const bool own = j >= row0 && j < row0 + nrows;
    const int js = own ? j : row0 + ((j - row0) % lrows + lrows) % lrows;
    const int shift = own ? 0 : ((j - js) % n + n) % n;
    const int a0 = off[(size_t)js * LVL_STRIDE + 1], a1 = off[(size_t)js * LVL_STRIDE + lw + 1];
    for (int i = a0 + lane; i < a1; i += 64) {
        const uint32_t e = arcs[i];
        int k = (int)(e & 0xFFFFu) + shift;
        if (k >= n) k -= n;
        const int s = k - row0, w = (int)(e >> 16);
        if (s < 0 || s >= nrows) continue;
        const size_t o = (size_t)j * nw + (s >> 5);
        const uint32_t bit = 1u << (s & 31);
        atomicOr(lev + (size_t)(w - 1) * plane + o, bit);
        if (w == 1) atomicOr(R + o, bit);
    }
}

/* ---- N > 1: the first batch's in-arcs streamed weight by weight ----------------------------- *
 * Level d reads its peers' arcs of weight < d only (an arc of weight d matters to its own source
 * alone), so the segments travel one weight at a time on a second stream and level d waits for
 * weight d - 1 alone: the wire of weight d runs under level d's gathers. On the wire the arcs of
 * one weight are rank-major, target-major within (offw: the exclusive scan of the counts in
 * [weight][target] order, lvl_offsets_kernel), one u32 per arc -- its source and its
 * index into the union table of distinct reliabilities (or the source alone, with the f64 beside
 * it when the union passes the table) -- and each receiver places them into its (target,
 * weight)-major arcs (4 B per arc on the wire instead of 6). */
/* The wire of weight w: one block of maxc[w] u32 per rank (rank q's arcs of weight w, its targets
 * in order, then padding), all-gathered; wtab[2 (w - 1)] = the weight's base in the wire,
 * wtab[2 (w - 1) + 1] = maxc[w]; zw[(w - 1) (R + 1) + q] = offw at rank q's first target */
__global__ void lvl_wire_pack_kernel(int ld, int row0, int lrows, int lw, int R, int me,
                                     const int32_t* __restrict__ off, const int32_t* __restrict__ offw,
                                     const int32_t* __restrict__ zw, const int32_t* __restrict__ wtab,
                                     const uint32_t* __restrict__ arcs, const uint16_t* __restrict__ rix,
                                     const double* __restrict__ ar, uint32_t* __restrict__ wire,
                                     double* __restrict__ wire64) {
    const int jj = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (jj >= lrows) return;
    const int j = row0 + jj;
    for (int w = 1; w <= lw; ++w) {
        const int a0 = off[(size_t)j * LVL_STRIDE + w], c = off[(size_t)j * LVL_STRIDE + w + 1] - a0;
        const size_t o = (size_t)wtab[2 * (w - 1)] + (size_t)me * wtab[2 * (w - 1) + 1] +
                         (offw[(size_t)(w - 1) * ld + j] - zw[(w - 1) * (R + 1) + me]);
        for (int i = lane; i < c; i += 64) {
            wire[o + i] = (arcs[a0 + i] & 0xFFFFu) | (rix ? (uint32_t)rix[a0 + i] << 16 : 0u);
            if (wire64) wire64[o + i] = ar[a0 + i];
        }
    }
}
__global__ void lvl_wire_unpack_kernel(int n, int ld, int row0, int nrows, int w, int nw, int R,
                                       const int32_t* __restrict__ off, const int32_t* __restrict__ offw,
                                       const int32_t* __restrict__ zw, const int32_t* __restrict__ wtab,
                                       const uint32_t* __restrict__ wire, const double* __restrict__ wire64,
                                       uint32_t* __restrict__ arcs, uint16_t* __restrict__ rix,
                                       double* __restrict__ ar, uint32_t* __restrict__ aoff) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n || (j >= row0 && j < row0 + nrows)) return;
    const long long nb = ld / SRT_SHARD_ALIGN; /* the owner of row j (srt_shard_rows) */
    int q = 0;
    while (q + 1 < R && (int)(nb * (q + 1) / R) * SRT_SHARD_ALIGN <= j) ++q;
    const int a0 = off[(size_t)j * LVL_STRIDE + w], c = off[(size_t)j * LVL_STRIDE + w + 1] - a0;
    const size_t o = (size_t)wtab[2 * (w - 1)] + (size_t)q * wtab[2 * (w - 1) + 1] +
                     (offw[(size_t)(w - 1) * ld + j] - zw[(w - 1) * (R + 1) + q]);
    for (int i = lane; i < c; i += 64) {
        const uint32_t e = wire[o + i], k = e & 0xFFFFu;
        arcs[a0 + i] = k | ((uint32_t)w << 16);
        if (rix) rix[a0 + i] = (uint16_t)(e >> 16);
        if (wire64) ar[a0 + i] = wire64[o + i];
        aoff[a0 + i] = k * (uint32_t)nw * 4u;
    }
}
/* Offsets of the (target, weight <= lw) in-arcs without masking the counts or scanning all 256
 * weight columns: per target its arcs up to lw (lvl_tot_kernel), one scan over the targets, then
 * the target's weight prefixes (lvl_off_kernel writes off[j][0 .. lw + 1]; columns past lw + 1
 * are never read: every reader stops at lw + 1). The counts stay whole for a later, heavier
 * extraction. */
__global__ void lvl_tot_kernel(int ld, int lw, const int32_t* __restrict__ cnt, int32_t* __restrict__ tot) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > ld) return;
    int t = 0;
    if (j < ld)
        for (int w = 1; w <= lw; ++w) t += cnt[(size_t)j * LVL_STRIDE + w];
    tot[j] = t;
}
__global__ void lvl_off_kernel(int ld, int lw, const int32_t* __restrict__ cnt, const int32_t* __restrict__ base,
                               int32_t* __restrict__ off) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > ld) return;
    int run = base[j];
    off[(size_t)j * LVL_STRIDE] = run;
    if (j == ld) return;
    for (int w = 1; w <= lw; ++w) {
        off[(size_t)j * LVL_STRIDE + w] = run;
        run += cnt[(size_t)j * LVL_STRIDE + w];
    }
    off[(size_t)j * LVL_STRIDE + lw + 1] = run;
}

/* The offsets of a first extraction (lw <= LVL_BATCH) in two launches: per target the (target,
 * weight)-major starts off[j][0..lw + 1] and (offw != NULL, the streamed wire) the
 * [weight][target] scan offw with its values at the shard starts (dsz). A workgroup takes 256
 * targets, a thread one target. The first kernel sums each workgroup's columns (the target
 * totals and the lw weights); the second adds the earlier workgroups' sums, scans its targets and
 * writes. They replace seven launches (totals, two scans, offsets, columns, two scans, sizes).
 * (One workgroup doing it all ran ~0.4 ms: one CU's latency on a rank's critical path.) */
static __device__ __forceinline__ void lvl_off_cols(int ld, int lw, int j, const int32_t* __restrict__ cnt,
                                                    int (&x)[LVL_BATCH + 1]) {
    x[0] = 0;
#pragma unroll
    for (int w = 1; w <= LVL_BATCH; ++w) {
        x[w] = j < ld && w <= lw ? cnt[(size_t)j * LVL_STRIDE + w] : 0;
        x[0] += x[w];
    }
}
__global__ __launch_bounds__(256) void lvl_off_part_kernel(int ld, int lw, const int32_t* __restrict__ cnt,
                                                           int32_t* __restrict__ part) {
    __shared__ int ws[4][LVL_BATCH + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int x[LVL_BATCH + 1];
    lvl_off_cols(ld, lw, blockIdx.x * 256 + tid, cnt, x);
#pragma unroll
    for (int c = 0; c <= LVL_BATCH; ++c) {
        int v = x[c];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) ws[wv][c] = v;
    }
    __syncthreads();
    if (tid <= LVL_BATCH) part[blockIdx.x * (LVL_BATCH + 1) + tid] = ws[0][tid] + ws[1][tid] + ws[2][tid] + ws[3][tid];
}
__global__ __launch_bounds__(256) void lvl_offsets_kernel(int ld, int lw, int R, const int32_t* __restrict__ cnt,
                                                          const int32_t* __restrict__ part, int32_t* __restrict__ off,
                                                          int32_t* __restrict__ offw, int32_t* __restrict__ dsz) {
    __shared__ int pre[LVL_BATCH + 1], tot[LVL_BATCH + 1], colB[LVL_BATCH + 2], ws[4][LVL_BATCH + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x, nb = gridDim.x;
    if (tid < 4 * (LVL_BATCH + 1)) { /* four threads per column: the earlier blocks' sums, all sums */
        const int c = tid >> 2, k = tid & 3;
        int p = 0, t = 0;
        for (int q = k; q < nb; q += 4) {
            const int v = part[q * (LVL_BATCH + 1) + c];
            t += v;
            if (q < b) p += v;
        }
        p += __shfl_xor(p, 1);
        p += __shfl_xor(p, 2);
        t += __shfl_xor(t, 1);
        t += __shfl_xor(t, 2);
        if (k == 0) {
            pre[c] = p;
            tot[c] = t;
        }
    }
    __syncthreads();
    if (tid == 0) { /* offw's base of each weight */
        int r = 0;
        for (int w = 1; w <= lw; ++w) {
            colB[w] = r;
            r += tot[w];
        }
        colB[lw + 1] = r;
    }
    const int j = b * 256 + tid;
    int x[LVL_BATCH + 1], ex[LVL_BATCH + 1];
    lvl_off_cols(ld, lw, j, cnt, x);
#pragma unroll
    for (int c = 0; c <= LVL_BATCH; ++c) {
        int v = x[c];
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(v, o);
            if (lane >= o) v += y;
        }
        ex[c] = v - x[c];
        if (lane == 63) ws[wv][c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c <= LVL_BATCH; ++c) {
        int add = pre[c];
        for (int v = 0; v < wv; ++v) add += ws[v][c];
        ex[c] += add;
    }
    if (j < ld) {
        int32_t* oj = off + (size_t)j * LVL_STRIDE;
        int r = ex[0];
        oj[0] = r;
#pragma unroll
        for (int w = 1; w <= LVL_BATCH; ++w)
            if (w <= lw) {
                oj[w] = r;
                r += x[w];
            }
        oj[lw + 1] = r;
        if (offw) {
#pragma unroll
            for (int w = 1; w <= LVL_BATCH; ++w)
                if (w <= lw) offw[(size_t)(w - 1) * ld + j] = colB[w] + ex[w];
            if (dsz && j % SRT_SHARD_ALIGN == 0) { /* a shard start (srt_shard_rows) */
                const long long nbs = ld / SRT_SHARD_ALIGN;
                for (int q = 0; q < R; ++q)
                    if ((int)(nbs * q / R) * SRT_SHARD_ALIGN == j)
                        for (int w = 1; w <= lw; ++w) dsz[(w - 1) * (R + 1) + q] = colB[w] + ex[w];
            }
        }
    } else if (j == ld) {
        off[(size_t)ld * LVL_STRIDE] = tot[0];
        if (offw) {
            offw[(size_t)lw * ld] = colB[lw + 1];
            if (dsz) /* q == R: the weight's end, the next weight's start */
                for (int w = 1; w <= lw; ++w) dsz[(w - 1) * (R + 1) + R] = colB[w + 1];
        }
    }
}

/* N > 1, the one exchange ahead of every decision (a sum all-reduce of int32; each rank fills
 * its own slots, the others stay zero): the weight histogram's 20-bit limbs (512) and the
 * allocation-failure count (+1 pad), every rank's own arcs per weight w <= LVL_BATCH as 16-bit
 * halves (R x 16), and every rank's distinct light reliabilities -- a header (probe overflow,
 * count) then up to LVL_RT_CAP values, as int32 pairs (R x (LVL_RT_CAP + 1) x 2). */
#define LVL_X_LIMBS (2 * LVL_STRIDE + 2)
#define LVL_X_CNT (2 * LVL_BATCH)
static size_t lvl_x_words(int R) { return LVL_X_LIMBS + (size_t)R * LVL_X_CNT + (size_t)R * (LVL_RT_CAP + 1) * 2; }
/* directed, N > 1: the limbs and the failure count, then every rank's arcs per weight, all 256
 * weights as 16-bit halves (both extractions' block sizes); no reliability blocks (no stash) */
#define LVL_X_DCNT (2 * LVL_STRIDE)
static size_t lvl_xd_words(int R) { return LVL_X_LIMBS + (size_t)R * LVL_X_DCNT; }
/* per rank q in [q0, q1) and weight w <= LVL_BATCH: its shard's arcs of weight w, into the
 * exchange as 16-bit halves (a rank counts its own shard; a solo rank every shard of its
 * synthesised counts) */
__global__ void lvl_rank_counts_kernel(int n, int ld, int R, int q0, const int32_t* __restrict__ cnt,
                                       int32_t* __restrict__ xcnt) {
    const int q = q0 + (int)blockIdx.y, w = 1 + (int)blockIdx.x;
    const long long nb = ld / SRT_SHARD_ALIGN;
    const int b = (int)(nb * q / R) * SRT_SHARD_ALIGN, e = min(n, (int)(nb * (q + 1) / R) * SRT_SHARD_ALIGN);
    unsigned s = 0;
    for (int j = b + threadIdx.x; j < e; j += blockDim.x) s += (unsigned)cnt[(size_t)j * LVL_STRIDE + w];
    for (int o = 32; o > 0; o >>= 1) s += (unsigned)__shfl_xor((int)s, o);
    __shared__ unsigned ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = ws[0] + ws[1] + ws[2] + ws[3];
        xcnt[(size_t)q * LVL_X_CNT + (w - 1) * 2] = (int32_t)(t & 0xFFFFu);
        xcnt[(size_t)q * LVL_X_CNT + (w - 1) * 2 + 1] = (int32_t)(t >> 16);
    }
}
/* the distinct reliabilities of this rank's light arcs (1 <= w <= wl) straight from the count
 * pass's stash: each workgroup dedupes a run of rows in its LDS table and writes the table out
 * whole (tabs[block], coalesced); lvl_rt_merge_kernel folds the tables into the global table H.
 * Inserting each workgroup's values straight into H (agent-scope atomics on ~500 hot lines, from
 * every workgroup) took 72 us on a rank of C4 at N = 8. */
__global__ __launch_bounds__(256) void lvl_rt_hash_stash_kernel(int nrows, int ld, int wl,
                                                                const uint32_t* __restrict__ stash,
                                                                const int32_t* __restrict__ scnt,
                                                                const double* __restrict__ r,
                                                                unsigned long long* __restrict__ H,
                                                                unsigned long long* __restrict__ tabs,
                                                                int* __restrict__ ovf) {
    __shared__ unsigned long long key[LVL_RT_LDS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int per = (nrows + (int)gridDim.x - 1) / (int)gridDim.x;
    const int r0 = (int)blockIdx.x * per, r1 = min(nrows, r0 + per);
    for (int k = tid; k < LVL_RT_LDS; k += 256) key[k] = ~0ull;
    __syncthreads();
    bool bad = false;
    constexpr int PL = LVL_STASH_SEG / 64; /* a segment's entries per lane, loaded together */
    for (int jj = r0; jj < r1; ++jj) { /* wave wv: the row's segment wv */
        const int m = scnt[(size_t)jj * 4 + wv];
        const uint32_t* sg = stash + (size_t)jj * LVL_STASH_CAP + wv * LVL_STASH_SEG;
        uint32_t e[PL];
#pragma unroll
        for (int q = 0; q < PL; ++q) e[q] = q * 64 + lane < m ? sg[q * 64 + lane] : 0u;
        unsigned long long v[PL];
#pragma unroll
        for (int q = 0; q < PL; ++q) {
            const uint32_t x = e[q] >> 16;
            v[q] = x >= 1u && x <= (uint32_t)wl
                       ? (unsigned long long)__double_as_longlong(r[(size_t)jj * ld + (e[q] & 0xFFFFu)])
                       : ~0ull;
        }
#pragma unroll
        for (int q = 0; q < PL; ++q) {
            if (v[q] == ~0ull) continue;
            unsigned h = lvl_rt_hash(v[q]) & (LVL_RT_LDS - 1u);
            int p = 0;
            for (; p < 64; ++p, h = (h + 1u) & (LVL_RT_LDS - 1u)) {
                unsigned long long y = __hip_atomic_load(&key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (y == ~0ull) y = atomicCAS(&key[h], ~0ull, v[q]);
                if (y == ~0ull || y == v[q]) break;
            }
            if (p == 64) bad |= lvl_rt_global_slot(v[q], H) < 0;
        }
    }
    __syncthreads();
    for (int k = tid; k < LVL_RT_LDS; k += 256) tabs[(size_t)blockIdx.x * LVL_RT_LDS + k] = key[k];
    if (bad) *ovf = 1;
}
/* slot k of every workgroup table mostly holds the same value (the same hash, the same probe):
 * thread (k, chunk) walks LVL_RT_MC tables' slot k (independent loads) and inserts each value it
 * has not just inserted into H -- a few inserts per slot and chunk instead of one per table */
#define LVL_RT_MC 16
__global__ __launch_bounds__(256) void lvl_rt_merge_kernel(int ntab, const unsigned long long* __restrict__ tabs,
                                                           unsigned long long* __restrict__ H,
                                                           int* __restrict__ ovf) {
    const int k = (blockIdx.x * 256 + threadIdx.x) % LVL_RT_LDS;
    const int t0 = (blockIdx.x * 256 + threadIdx.x) / LVL_RT_LDS * LVL_RT_MC;
    if (t0 >= ntab) return;
    unsigned long long v[LVL_RT_MC];
#pragma unroll
    for (int t = 0; t < LVL_RT_MC; ++t) v[t] = t0 + t < ntab ? tabs[(size_t)(t0 + t) * LVL_RT_LDS + k] : ~0ull;
    unsigned long long seen[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    bool bad = false;
#pragma unroll
    for (int t = 0; t < LVL_RT_MC; ++t) {
        if (v[t] == ~0ull || v[t] == seen[0] || v[t] == seen[1] || v[t] == seen[2] || v[t] == seen[3]) continue;
        bad |= lvl_rt_global_slot(v[t], H) < 0;
        seen[3] = seen[2];
        seen[2] = seen[1];
        seen[1] = seen[0];
        seen[0] = v[t];
    }
    if (bad) *ovf = 1;
}

/* the own arcs in [*lo, *hi): each one's byte offset of its source row (aoff) and its index into
 * the sorted table of distinct reliabilities (by value bits, binary search) -- one pass */
__global__ void lvl_own_index_kernel(const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int nw,
                                     const uint32_t* __restrict__ arcs, const double* __restrict__ ar,
                                     const unsigned long long* __restrict__ tab, int ntab,
                                     uint32_t* __restrict__ aoff, uint16_t* __restrict__ rix) {
    const int a = *lo, b = *hi;
    for (int i = a + blockIdx.x * blockDim.x + threadIdx.x; i < b; i += gridDim.x * blockDim.x) {
        aoff[i] = (arcs[i] & 0xFFFFu) * (uint32_t)nw * 4u;
        const unsigned long long v = (unsigned long long)__double_as_longlong(ar[i]);
        int l = 0, h = ntab - 1;
        while (l < h) {
            const int mid = (l + h) >> 1;
            if (tab[mid] < v) l = mid + 1;
            else h = mid;
        }
        rix[i] = (uint16_t)l;
    }
}

/* the second stream and the per-weight events of the streamed extraction, per state slot (made
 * once, kept: a stream's creation costs more than a build's host work) */
static hipStream_t g_lvl_cs[SRT_STATE_SLOTS];
static hipEvent_t g_lvl_ev[SRT_STATE_SLOTS][LVL_BATCH + 2];
static int lvl_side_stream(hipStream_t* cs, hipEvent_t** ev) {
    const int k = srt_state_slot();
    if (!g_lvl_cs[k]) {
        SRT_HIPCHK(hipStreamCreateWithFlags(&g_lvl_cs[k], hipStreamNonBlocking));
        for (int i = 0; i < LVL_BATCH + 2; i++)
            SRT_HIPCHK(hipEventCreateWithFlags(&g_lvl_ev[k][i], hipEventDisableTiming));
    }
    *cs = g_lvl_cs[k];
    *ev = g_lvl_ev[k];
    return SRT_OK;
}
/* the host-side set that deduplicates the exchanged reliability blocks, per slot */
static std::vector<unsigned long long> g_lvl_uset[SRT_STATE_SLOTS];
/* ... and their sorted union (lvl_union) */
static std::vector<unsigned long long> g_lvl_union[SRT_STATE_SLOTS];
/* The build's host round trips (the exchange, the agreement, one vote per batch) go through
 * pinned staging, per slot, made once and grown when a larger exchange needs it: a copy to or
 * from pageable memory is staged by the runtime and blocks the calling thread. Layout (u64
 * words): the one-GPU histogram, the agreement and failure flag, the vote's read-back, then the
 * exchange, the union table and the wire's per-weight bases. */
#define LVL_PIN_HIST 0
#define LVL_PIN_AG LVL_STRIDE
#define LVL_PIN_HW (LVL_PIN_AG + 4)
#define LVL_PIN_X (LVL_PIN_HW + LVL_H_WORDS - LVL_H_INC)
static unsigned long long* g_lvl_pin[SRT_STATE_SLOTS];
static size_t g_lvl_pin_words[SRT_STATE_SLOTS];
static hipEvent_t g_lvl_wev[SRT_STATE_SLOTS];
static int lvl_pinned(size_t words, unsigned long long** p) {
    const int k = srt_state_slot();
    if (g_lvl_pin_words[k] < words) {
        if (g_lvl_pin[k]) SRT_HIPCHK(hipHostFree(g_lvl_pin[k]));
        g_lvl_pin[k] = NULL;
        g_lvl_pin_words[k] = 0;
        SRT_HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&g_lvl_pin[k]), words * sizeof(unsigned long long),
                                 hipHostMallocDefault));
        g_lvl_pin_words[k] = words;
    }
    *p = g_lvl_pin[k];
    return SRT_OK;
}
/* Wait for the stream with the calling thread spinning on an event. hipStreamSynchronize sleeps
 * on the completion interrupt past a short active window, and the wake-up cost 30-60 us per round
 * trip in the traces of one rank of N = 8 (three or four per build). */
static int lvl_wait(hipStream_t st) {
    hipEvent_t& e = g_lvl_wev[srt_state_slot()];
    if (!e) SRT_HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    SRT_HIPCHK(hipEventRecord(e, st));
    hipError_t r;
    while ((r = hipEventQuery(e)) == hipErrorNotReady) {
    }
    SRT_HIPCHK(r);
    return SRT_OK;
}

/* byte offset of each arc's source row inside a level plane (k * nw * 4; nw is this rank's) */
__global__ void lvl_aoff_kernel(int total, int nw, const uint32_t* __restrict__ arcs,
                                uint32_t* __restrict__ aoff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) aoff[i] = (arcs[i] & 0xFFFFu) * (uint32_t)nw * 4u;
}

/* lvl_pred_rows_kernel's output stage: each arc's source vertex | index into rtab << 16, the low
 * 27 bits of a packed word, so a pair costs one gather where arcs[] and rix[] were two */
__global__ void lvl_apk_kernel(int total, const uint32_t* __restrict__ arcs,
                               const uint16_t* __restrict__ rix, uint32_t* __restrict__ apk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) apk[i] = (arcs[i] & 0xFFFFu) | (uint32_t)rix[i] << 16;
}

/* ---- the levels ---------------------------------------------------------------------------- */
/* R = {j} for the local sources j (distance 0), everything else empty */
__global__ void lvl_init_kernel(int n, int src0, int nsrc, int nw, uint32_t* __restrict__ R) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsrc) return;
    const int j = src0 + i;
    if (j < n) R[(size_t)j * nw + (i >> 5)] = 1u << (i & 31);
}

/* Level 1 without the unit walk: Delta_1[j] = {s : w(s, j) = 1} (every arc is >= 1 quantum), so
 * the level is j's weight-1 in-arcs set as bits (~33 per C4 target) in a zeroed plane and in R.
 * A wave owns target j (its row of both), a lane an arc; the arcs are sorted by source, so lanes
 * of one word are adjacent: a segmented OR (shuffle-up scan) leaves each word's bits in its last
 * lane, which stores them. No atomics: a same-address counter atomic per wave alone cost 0.40 ms
 * on C4 (serialised at the memory side), so the host counts the level's pairs from the weight
 * histogram instead. */
__global__ __launch_bounds__(256) void lvl_first_kernel(int n, int nw, int src0, int nsrc,
                                                        const int32_t* __restrict__ off,
                                                        const uint32_t* __restrict__ arcs,
                                                        uint32_t* __restrict__ lev0,
                                                        uint32_t* __restrict__ R) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j < n) {
        const int a0 = off[(size_t)j * LVL_STRIDE + 1], a1 = off[(size_t)j * LVL_STRIDE + 2];
        for (int i0 = a0; i0 < a1; i0 += 64) {
            const int i = i0 + lane;
            const int ks = i < a1 ? (int)(arcs[i] & 0xFFFFu) - src0 : -1;
            const bool in = ks >= 0 && ks < nsrc;
            const int wd = in ? ks >> 5 : -1 - lane; /* out-of-range lanes: words of their own */
            uint32_t bits = in ? 1u << (ks & 31) : 0u;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t yb = (uint32_t)__shfl_up((int)bits, o);
                const int yw = __shfl_up(wd, o);
                if (lane >= o && yw == wd) bits |= yb;
            }
            const int nwd = __shfl_down(wd, 1);
            if (in && (lane == 63 || nwd != wd)) {
                const size_t o = (size_t)j * nw + wd;
                lev0[o] |= bits;
                R[o] |= bits;
            }
        }
    }
}

/* Levels 2 and 3, the near part: the bits that arcs of weight d (Delta_0: the own source itself)
 * and of weight d - 1 (Delta_1) contribute to Delta_d[t], set into plane d - 1 before
 * lvl_step_kernel, which then skips that weight group (its gathers read a plane that is nearly
 * empty: Delta_1[u] is u's ~33 weight-1 in-arcs among n sources). Delta_1[u] is exactly u's
 * weight-1 run of in-arcs, so a wave per target t reads, for each in-arc (u, d - 1), u's run
 * (~130 B, coalesced) instead of one 256-B plane slice per source chunk, and ORs the sources
 * into an LDS copy of t's plane row, which it then writes whole. add: the row already holds the
 * own-arc bits (streamed N > 1, lvl_direct_kernel), so it is read first and the weight-d run is
 * not scanned. */
__global__ __launch_bounds__(256) void lvl_near_kernel(int d, int n, int nw, int src0, int nsrc, int add,
                                                       const int32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ arcs,
                                                       uint32_t* __restrict__ lev) {
    extern __shared__ uint32_t near_row[]; /* per wave: nw words */
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wv;
    uint32_t* row = near_row + (size_t)wv * nw;
    const size_t plane = (size_t)n * nw;
    uint32_t* prow = lev + (size_t)(d - 1) * plane + (size_t)(t < n ? t : 0) * nw;
    for (int i = lane; i < nw; i += 64) row[i] = t < n && add ? prow[i] : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (t < n) {
        const int32_t* ot = off + (size_t)t * LVL_STRIDE;
        if (!add) /* the own sources' arcs of weight d into t */
            for (int i = ot[d] + lane; i < ot[d + 1]; i += 64) {
                const int ks = (int)(arcs[i] & 0xFFFFu) - src0;
                if (ks >= 0 && ks < nsrc) atomicOr(&row[ks >> 5], 1u << (ks & 31));
            }
        /* each in-arc (u, d - 1): u's weight-1 run. The runs' bounds of 64 arcs come in one
         * vector load per lane, then four runs are read at a time (their first 64 entries in
         * flight together; a longer run's tail after) */
        const int a1 = ot[d];
        for (int c0 = ot[d - 1]; c0 < a1; c0 += 64) {
            int ub0 = 0, ub1 = 0;
            if (c0 + lane < a1) {
                const int u = (int)(arcs[c0 + lane] & 0xFFFFu);
                ub0 = off[(size_t)u * LVL_STRIDE + 1];
                ub1 = off[(size_t)u * LVL_STRIDE + 2];
            }
            const int na = min(64, a1 - c0);
            for (int k = 0; k < na; k += 4) {
                uint32_t e[4];
                int b0[4], b1[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    b0[q] = k + q < na ? __builtin_amdgcn_readlane(ub0, k + q) : 0;
                    b1[q] = k + q < na ? __builtin_amdgcn_readlane(ub1, k + q) : 0;
                    e[q] = b0[q] + lane < b1[q] ? arcs[b0[q] + lane] : 0xFFFFFFFFu;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ks = (int)(e[q] & 0xFFFFu) - src0;
                    if (e[q] != 0xFFFFFFFFu && ks >= 0 && ks < nsrc) atomicOr(&row[ks >> 5], 1u << (ks & 31));
                    for (int i = b0[q] + 64 + lane; i < b1[q]; i += 64) { /* (runs past 64) */
                        const int kt = (int)(arcs[i] & 0xFFFFu) - src0;
                        if (kt >= 0 && kt < nsrc) atomicOr(&row[kt >> 5], 1u << (kt & 31));
                    }
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (t < n)
        for (int i = lane; i < nw; i += 64) prow[i] = row[i];
}

/* Level d: one wave per (target j, 64-word source chunk c). Units are handed out XCD-major (each
 * XCD takes a contiguous run of chunk-major units), so an XCD works on one source chunk at a time
 * and the Delta rows of that chunk are the only gathered data in its L2. */
static __device__ __forceinline__ uint32_t lvl_step_unit(unsigned g, int d, int direct, int n, int nw,
                                                       int nchunk, int src0, int nsrc, uint32_t& gath,
                                                       const int32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ arcs,
                                                       const uint32_t* __restrict__ aoff,
                                                       uint32_t* __restrict__ lev,
                                                       uint32_t* __restrict__ R,
                                                       uint8_t* __restrict__ done,
                                                       int* __restrict__ incomplete) {
    const int tgrp = (n + 3) >> 2;
    const int c = (int)(g / (unsigned)tgrp);
    /* the wave index through readfirstlane: j is then wave-uniform to the compiler, so the offsets
     * and the arcs come through scalar loads and every gather's row address is an SGPR */
    const int j = (int)(g % (unsigned)tgrp) * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (c >= nchunk || j >= n) return 0u;
    const int lane = threadIdx.x & 63, word = c * 64 + lane;
    const bool valid = word < nw;
    const size_t plane = (size_t)n * nw; /* words per level */
    uint32_t* out = lev + (size_t)(d - 1) * plane + (size_t)j * nw + word;
    const size_t u = (size_t)j * nchunk + c;
    if (done[u]) {
        if (valid) *out = 0u;
        return 0u;
    }
    uint32_t acc = 0;
    const int32_t* oj = off + (size_t)j * LVL_STRIDE;
    /* arcs of weight d: the path (k, j) itself, Delta_0[k] = {k}; 64 arcs per step, one per lane,
     * and the few whose source lies in this unit's chunk go to the lane owning its word (direct:
     * lvl_direct_kernel left them in the plane) */
    if (direct) {
        if (valid) acc = *out;
    } else {
        const int a0 = oj[d], a1 = oj[d + 1], cw0 = c * 64 * 32;
        for (int i0 = a0; i0 < a1; i0 += 64) {
            const int i = i0 + lane;
            const int ks = i < a1 ? (int)(arcs[i] & 0xFFFFu) - src0 : -1;
            unsigned long long m = __ballot(ks >= 0 && ks < nsrc && (unsigned)(ks - cw0) < 64u * 32u);
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1ull;
                const int kj = __builtin_amdgcn_readlane(ks, j);
                if ((kj >> 5) == word) acc |= 1u << (kj & 31);
            }
        }
    }
    /* arcs of weight w < d: Delta_{d-w}[k], one weight group at a time so the group's plane base is
     * one scalar pointer and an arc costs one VALU add (its row's byte offset k * nw * 4, aoff, plus
     * the lane's) and one gather; sixteen gathers in flight. Lanes past nw read word 0 of the row
     * (a valid address) and drop it, so the loop has no per-lane branch. */
    const uint32_t lane4 = (uint32_t)(valid ? word : 0) * 4u;
    /* The unit's settled sources, read before the gathers: once every source of the unit is
     * settled or found, the later gathers cannot change the level's new bits (acc & ~r), so the
     * walk stops. On C4 a source at distance 4 is nearly always found through a weight-1 arc from
     * a vertex at distance 3, so level 4 needs the first weight group alone wherever the unit
     * holds no source at distance 5. Sources past n (padding of the last shard) never appear:
     * they count as settled. */
    uint32_t* rp = R + (size_t)j * nw + word;
    const uint32_t r = valid ? *rp : 0u;
    const int s0 = src0 + word * 32;
    const uint32_t full = !valid ? 0u : s0 + 32 <= n ? 0xFFFFFFFFu : s0 >= n ? 0u : (1u << (n - s0)) - 1u;
    constexpr int LVL_SB = 16; /* (8 measured the same, 32/48 slower; pipelined batches did not help) */
    for (int w = 1; w < d; ++w) {
        if (direct == 2 && w == d - 1) continue; /* lvl_near_kernel set this group's bits */
        if (!__any(((acc | r) & full) != full)) break;
        const int g1 = oj[w + 1];
        const char* base = reinterpret_cast<const char*>(lev + (size_t)(d - w - 1) * plane);
        for (int i = oj[w]; i < g1; i += LVL_SB) { /* LVL_SB in flight, the tail predicated */
            uint32_t a[LVL_SB], v[LVL_SB];
#pragma unroll
            for (int q = 0; q < LVL_SB; ++q) a[q] = aoff[i + q]; /* padded: one scalar burst */
#pragma unroll
            for (int q = 0; q < LVL_SB; ++q)
                v[q] = i + q < g1 ? *reinterpret_cast<const uint32_t*>(base + (a[q] + lane4)) : 0u;
#pragma unroll
            for (int q = 0; q < LVL_SB; ++q) acc |= v[q];
            if (valid) gath += (uint32_t)min(LVL_SB, g1 - i); /* the lane's 4-B gathers */
            if (i + LVL_SB < g1 && !__any(((acc | r) & full) != full)) break;
        }
    }
    if (!valid) acc = 0;
    bool inc = false;
    uint32_t settled = 0;
    if (valid) {
        const uint32_t nb = acc & ~r;
        settled = (uint32_t)__builtin_popcount(nb);
        *out = nb;
        if (nb) *rp = r | nb;
        inc = ((r | nb) & full) != full;
    }
    /* completion: a flag, not a count -- one same-address atomic per wave serialised at the memory
     * side (~6 ms per level at C4's 524k units); the flag is read first (an L2 hit once set), so
     * only the first few waves of a level store it */
    const unsigned long long m = __ballot(inc);
    if (lane == 0) {
        if (!m)
            done[u] = 1;
        else if (!__hip_atomic_load(incomplete, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            __hip_atomic_store(incomplete, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return settled;
}

/* Persistent grid (a few workgroups per CU, each looping over unit blocks): the units live only a
 * few microseconds, so a one-shot grid of 131k workgroups was bound by workgroup dispatch. Block p
 * of XCD p % 8 takes that XCD's contiguous run of unit blocks (chunk-major): 0.69 ms per C4 level
 * against 0.80 when all XCDs walk the same chunk together (lvl_pred_kernel's order). */
__global__ __launch_bounds__(256) void lvl_step_kernel(int d, int direct, int n, int nw, int nchunk, int src0,
                                                       int nsrc, unsigned nblk,
                                                       const int32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ arcs,
                                                       const uint32_t* __restrict__ aoff,
                                                       uint32_t* __restrict__ lev,
                                                       uint32_t* __restrict__ R,
                                                       uint8_t* __restrict__ done,
                                                       int* __restrict__ incomplete,
                                                       const int* __restrict__ prev,
                                                       unsigned long long* __restrict__ nset,
                                                       unsigned long long* __restrict__ ngath) {
    /* the levels are enqueued in batches without a host round trip per level: a level whose
     * predecessor settled every pair (prev == 0) has nothing to do */
    if (prev && !__hip_atomic_load(prev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const unsigned x = blockIdx.x & 7u, per = nblk >> 3, L = gridDim.x >> 3;
    uint32_t settled = 0; /* pairs this lane settled (one add per block at the end) */
    uint32_t gath = 0;    /* 4-B words this lane gathered (the early exit makes it data-dependent) */
    for (unsigned u = blockIdx.x >> 3; u < per; u += L)
        settled += lvl_step_unit(x * per + u, d, direct, n, nw, nchunk, src0, nsrc, gath, off, arcs, aoff, lev, R,
                                 done, incomplete);
    unsigned long long c = settled, gb = gath;
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o);
        gb += __shfl_xor(gb, o);
    }
    __shared__ unsigned long long s_c[4], s_g[4];
    if ((threadIdx.x & 63) == 0) {
        s_c[threadIdx.x >> 6] = c;
        s_g[threadIdx.x >> 6] = gb;
    }
    __syncthreads();
    if (threadIdx.x == 0 && (s_c[0] | s_c[1] | s_c[2] | s_c[3]))
        atomicAdd(nset, s_c[0] + s_c[1] + s_c[2] + s_c[3]);
    if (threadIdx.x == 0 && (s_g[0] | s_g[1] | s_g[2] | s_g[3]))
        atomicAdd(ngath, 4ull * (s_g[0] + s_g[1] + s_g[2] + s_g[3]));
}

/* Distance rows of the local sources from the levels: the u32 table rows (SRT_INF on padding) and
 * the u8 level rows the reliability pass reads (0 on the diagonal and padding) -- the FW finish
 * pass folded in: every settled distance is <= the level budget (<= 254), so the rows are exact
 * and small by construction. Thread = four consecutive targets t0..t0 + 3 (256 threads = 1,024
 * targets per workgroup), looping over 16 source words: per word it reads the four targets' word
 * of every level (the same lines for the 16 words of a workgroup row), keeps the 32 sources' four
 * distances as bytes (0xFF: none; 32 VGPRs, 8 waves per SIMD) and writes 16 B of u32 and 4 B of u8
 * per source row. */
__global__ __launch_bounds__(256) void lvl_out_kernel(int n, int ld, int nw, int src0, int nlev,
                                                      const uint32_t* __restrict__ lev,
                                                      uint32_t* __restrict__ lat,
                                                      uint8_t* __restrict__ l8) {
    const int t0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t0 >= ld) return;
    const size_t plane = (size_t)n * nw;
    const int sw1 = min(nw, (int)(blockIdx.y + 1) * 16);
    for (int sw = blockIdx.y * 16; sw < sw1; ++sw) {
        uint32_t v[32]; /* per source: the distances to t0..t0 + 3, one byte each */
        const int sg0 = src0 + sw * 32;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const int sg = sg0 + s;
            uint32_t x = 0xFFFFFFFFu;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (sg == t0 + q) x &= ~(0xFFu << (8 * q));
            v[s] = x;
        }
        for (int d = 1; d <= nlev; ++d) {
            uint32_t m[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                m[q] = t0 + q < n ? lev[(size_t)(d - 1) * plane + (size_t)(t0 + q) * nw + sw] : 0u;
            if (!(m[0] | m[1] | m[2] | m[3])) continue;
#pragma unroll
            for (int s = 0; s < 32; ++s) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if ((m[q] >> s) & 1u)
                        v[s] = (v[s] & ~(0xFFu << (8 * q))) | ((uint32_t)d << (8 * q));
            }
        }
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const size_t o = (size_t)(sw * 32 + s) * ld + t0;
            uint32_t x[4], b = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t y = (v[s] >> (8 * q)) & 0xFFu;
                x[q] = y == 0xFFu ? SRT_INF : y;
                b |= (y == 0xFFu ? 0u : y) << (8 * q);
            }
            *reinterpret_cast<uint4*>(lat + o) = make_uint4(x[0], x[1], x[2], x[3]);
            *reinterpret_cast<uint32_t*>(l8 + o) = b;
        }
    }
}

/* The same rows for builds of at most LVL_OUT_L levels, without lvl_out_kernel's re-fetches (its
 * 4-B plane reads come back 16 times per 64-B sector: C4 fetched 8.9 GB for 0.65 GB of planes).
 * Workgroup = 256 targets x 8 source words: every level's 8 words of every target are staged in
 * LDS with one 32-B read per (target, level), then thread = one target runs over the 8 words (256
 * sources) from LDS, keeping a word's 32 distances as bytes, and writes 4 B of u32 and 1 B of u8
 * per source row (a wave's 64 consecutive targets: 256 B / 64 B runs). */
#define LVL_OUT_L 16
__global__ __launch_bounds__(256) void lvl_out8_kernel(int n, int ld, int nw, int src0, int nlev,
                                                       const uint32_t* __restrict__ lev,
                                                       uint32_t* __restrict__ lat,
                                                       uint8_t* __restrict__ l8) {
    extern __shared__ uint4 smo[]; /* [level][half][target]: words w0..w0+3 | +4..+7 (8 KB per level) */
    auto sm = reinterpret_cast<uint4(*)[2][256]>(smo);
    const int tid = threadIdx.x, t = blockIdx.x * 256 + tid;
    const int w0 = blockIdx.y * 8;
    const size_t plane = (size_t)n * nw;
    const bool tv = t < n;
    for (int d = 0; d < nlev; ++d) {
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
        if (tv) { /* nw is a multiple of 4 (nsrc % 128 == 0): 16-B aligned words */
            const uint4* p = reinterpret_cast<const uint4*>(lev + (size_t)d * plane + (size_t)t * nw + w0);
            a = p[0];
            b = w0 + 4 < nw ? p[1] : make_uint4(0u, 0u, 0u, 0u);
        }
        sm[d][0][tid] = a;
        sm[d][1][tid] = b;
    }
    /* (thread tid reads back only its own entries: no barrier needed) */
    if (t >= ld) return;
    const int k1 = min(8, nw - w0);
    for (int k = 0; k < k1; ++k) {
        uint32_t v[8]; /* sources 4i..4i+3 of the word, one byte each (0xFF: none) */
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0xFFFFFFFFu;
        const int sg0 = src0 + (w0 + k) * 32;
        if (t >= sg0 && t < sg0 + 32) { /* the diagonal */
            const int sd = t - sg0;
            v[sd >> 2] &= ~(0xFFu << (8 * (sd & 3)));
        }
        for (int d = 0; d < nlev; ++d) {
            const uint4 q = sm[d][k >> 2][tid];
            const uint32_t m = (k & 3) == 0 ? q.x : (k & 3) == 1 ? q.y : (k & 3) == 2 ? q.z : q.w;
            if (!m) continue;
#pragma unroll
            for (int sidx = 0; sidx < 32; ++sidx)
                if ((m >> sidx) & 1u)
                    v[sidx >> 2] = (v[sidx >> 2] & ~(0xFFu << (8 * (sidx & 3)))) |
                                   ((uint32_t)(d + 1) << (8 * (sidx & 3)));
        }
#pragma unroll
        for (int sidx = 0; sidx < 32; ++sidx) {
            const size_t o = (size_t)((w0 + k) * 32 + sidx) * ld + t;
            const uint32_t y = (v[sidx >> 2] >> (8 * (sidx & 3))) & 0xFFu;
            lat[o] = y == 0xFFu ? SRT_INF : y;
            l8[o] = (uint8_t)(y == 0xFFu ? 0u : y);
        }
    }
}

/* per-target segment starts of the (target, weight) offsets, for the segmented sort */
__global__ void lvl_segs_kernel(int ld, const int32_t* __restrict__ off, int32_t* __restrict__ seg) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= ld) seg[j] = off[(size_t)j * LVL_STRIDE];
}

/* The predecessor pass's Delta_1 groups from the in-arc runs, before lvl_pred_kernel (the form of
 * lvl_near_kernel: one wave per target t, every chunk at once). At level d the walk's group
 * w = d - 1 reads Delta_1[u] for each in-arc (u, d - 1) -- u's weight-1 run of in-arcs, ~97% zero
 * words as a plane row on C4 -- and cannot stop early, so it is most of a unit's gathers. Here the
 * wave keeps Delta_d[t] in LDS, clears the sources of t's own weight-d arcs (the direct arc wins),
 * then takes the arcs (u, d - 1) in arc order and each run's sources s one per lane: a
 * test-and-clear of s's bit (the LDS unit applies a wave's atomics in issue order, and a run's
 * sources are distinct) leaves the bit to the first arc that is tight for (s, t) -- the walk's
 * canonical arc, largest weight after the direct one and smallest u inside it. Each winner goes
 * to the bucket of (t, chunk of s) as source-in-chunk | (arc - off[t][0]) << 11, the u16 arc
 * index the walk keeps in sidx; the order inside a bucket is free (a source appears once). A
 * bucket holds cap entries: an append past cap only leaves the unit's count above cap, and
 * lvl_pred_unit then walks that unit's Delta_1 groups itself. LDS per wave: nw row words and
 * nchunk counters. */
__global__ __launch_bounds__(256) void lvl_pred_near_kernel(int n, int nw, int nchunk, int src0, int nsrc,
                                                            int nlev, int cap,
                                                            const int32_t* __restrict__ off,
                                                            const uint32_t* __restrict__ arcs,
                                                            const uint32_t* __restrict__ lev,
                                                            uint32_t* __restrict__ bkt,
                                                            uint32_t* __restrict__ bcnt,
                                                            int32_t* __restrict__ nover) {
    extern __shared__ uint32_t pn_lds[]; /* per wave: nw row words, then nchunk counters */
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wv;
    if (t >= n) return; /* (no workgroup barrier below: a wave works alone) */
    uint32_t* row = pn_lds + (size_t)wv * (nw + nchunk);
    uint32_t* cnt = row + nw;
    const size_t plane = (size_t)n * nw;
    const int32_t* ot = off + (size_t)t * LVL_STRIDE;
    const int a_t = ot[0];
    uint32_t* tb = bkt + (size_t)t * nchunk * cap;
    for (int i = lane; i < nchunk; i += 64) cnt[i] = 0u;
    /* s (local index ks) found through arc i: its bit test-and-cleared, the winner appended */
    auto claim = [&](int ks, int i) {
        const uint32_t bit = 1u << (ks & 31);
        if (atomicAnd(&row[ks >> 5], ~bit) & bit) {
            const int c = ks >> 11;
            const uint32_t pos = atomicAdd(&cnt[c], 1u);
            if (pos < (uint32_t)cap) tb[(size_t)c * cap + pos] = (uint32_t)(ks & 2047) | (uint32_t)(i - a_t) << 11;
        }
    };
    for (int d = 2; d <= nlev; ++d) {
        const uint32_t* prow = lev + (size_t)(d - 1) * plane + (size_t)t * nw;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t any = 0;
        for (int i = lane; i < nw; i += 64) any |= (row[i] = prow[i]);
        if (!__any(any != 0u)) continue; /* no source at this level */
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = ot[d] + lane; i < ot[d + 1]; i += 64) { /* the direct arcs keep their sources */
            const int ks = (int)(arcs[i] & 0xFFFFu) - src0;
            if (ks >= 0 && ks < nsrc) atomicAnd(&row[ks >> 5], ~(1u << (ks & 31)));
        }
        /* the runs' bounds of 64 arcs in one vector load per lane, four runs' first 64 entries in
         * flight together (lvl_near_kernel's schedule), their updates strictly in arc order */
        const int a1 = ot[d];
        for (int c0 = ot[d - 1]; c0 < a1; c0 += 64) {
            int ub0 = 0, ub1 = 0;
            if (c0 + lane < a1) {
                const int u = (int)(arcs[c0 + lane] & 0xFFFFu);
                ub0 = off[(size_t)u * LVL_STRIDE + 1];
                ub1 = off[(size_t)u * LVL_STRIDE + 2];
            }
            const int na = min(64, a1 - c0);
            for (int k = 0; k < na; k += 4) {
                uint32_t e[4];
                int b0[4], b1[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    b0[q] = k + q < na ? __builtin_amdgcn_readlane(ub0, k + q) : 0;
                    b1[q] = k + q < na ? __builtin_amdgcn_readlane(ub1, k + q) : 0;
                    e[q] = b0[q] + lane < b1[q] ? arcs[b0[q] + lane] : 0xFFFFFFFFu;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ks = (int)(e[q] & 0xFFFFu) - src0;
                    if (e[q] != 0xFFFFFFFFu && ks >= 0 && ks < nsrc) claim(ks, c0 + k + q);
                    for (int i = b0[q] + 64 + lane; i < b1[q]; i += 64) { /* (runs past 64) */
                        const int kt = (int)(arcs[i] & 0xFFFFu) - src0;
                        if (kt >= 0 && kt < nsrc) claim(kt, c0 + k + q);
                    }
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int over = 0;
    for (int i = lane; i < nchunk; i += 64) {
        const uint32_t k = cnt[i];
        bcnt[(size_t)t * nchunk + i] = k;
        over += k > (uint32_t)cap;
    }
    for (int m = 32; m > 0; m >>= 1) over += __shfl_xor(over, m);
    if (lane == 0 && over) atomicAdd(nover, over);
}

/* PT = uint32_t: the packed form -- one word per pair, (u16) predecessor | reliability index << 16
 * (the arc's reliability is rtab[index], lvl_rtab_*), written into predT; rT and ar unused */
/* Canonical predecessors from the levels (the rule of every build kernel: among the tight in-arcs
 * u -> t, D[s][u] + w = D[s][t], the smallest (D[s][u], u) -- so the largest w, then the smallest u;
 * Dijkstra with a (dist, vertex) heap, topology.c:1679-1701 up to igraph's tie order).
 * One wave per (target t, 64-word source chunk), the same units as lvl_step_kernel. For the
 * sources at level d (Delta_d[t]) the arcs are taken by weight w = d, d - 1, ..., 1 and, inside a
 * weight, by ascending u (the in-arcs are sorted so): the arc (u, w) is tight for exactly the
 * sources in Delta_{d-w}[u] (u itself when w = d), and a source takes its first tight arc. A source
 * hit by two arcs of its winning weight is a tied pair (srt_build_stats.tied_pairs). A level stops
 * as soon as every source of the wave has its arc. Outputs, target-major as pred_cols*_kernel's
 * (stride ldp): predT[t][sl] = u (-1 on the diagonal), rT[t][sl] = r(u, t). */
template <typename PT>
static __device__ __forceinline__ void lvl_pred_unit(unsigned g, uint16_t (*sidx)[64 * 40],
                                                     int n,
                                                     int nw, int nchunk, int src0, int nsrc, int nlev,
                                                       const int32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ arcs,
                                                       const uint32_t* __restrict__ aoff,
                                                       const double* __restrict__ ar,
                                                       const uint16_t* __restrict__ rix,
                                                       const uint32_t* __restrict__ lev,
                                                       PT* __restrict__ predT,
                                                       double* __restrict__ rT, size_t ldp,
                                                       unsigned long long* __restrict__ ties,
                                                       const uint32_t* __restrict__ bkt,
                                                       const uint32_t* __restrict__ bcnt, int cap) {
    constexpr bool PK = std::is_same_v<PT, uint32_t>;
    const int tgrp = (n + 3) >> 2;
    const int c = (int)(g / (unsigned)tgrp);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int t = (int)(g % (unsigned)tgrp) * 4 + wv;
    if (c >= nchunk || t >= n) return;
    const int lane = threadIdx.x & 63, word = c * 64 + lane;
    const bool valid = word < nw;
    const size_t plane = (size_t)n * nw;
    uint16_t* my = &sidx[wv][lane * 40];
#pragma unroll
    for (int q = 0; q < 32; q += 8)
        *reinterpret_cast<uint4*>(my + q) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    const int32_t* ot = off + (size_t)t * LVL_STRIDE;
    const int a_t = ot[0];
    const uint32_t lane4 = (uint32_t)(valid ? word : 0) * 4u;
    unsigned tied = 0;
    /* lvl_pred_near_kernel's bucket of this unit: the pairs whose arc is in a Delta_1 group
     * (w = d - 1), each into its source's sidx slot and its bit into the claimed word of the
     * lane that owns the source -- u16 slots 32-33 of the lane's 40 in sidx, which the read-back
     * leaves spare: no LDS added, and the word is re-read per level through the lane's sidx
     * address (no register held across the walk). A bucket that
     * overflowed is ignored and the groups are walked as without the pre-pass. */
    bool pn = false;
    if (bkt) {
        const size_t un = (size_t)t * nchunk + c;
        const int k = __builtin_amdgcn_readfirstlane((int)bcnt[un]);
        pn = k <= cap;
        if (pn) {
            *reinterpret_cast<uint32_t*>(my + 32) = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const uint32_t* ub = bkt + un * cap;
            for (int i = lane; i < k; i += 64) {
                const uint32_t e = ub[i], sl = e & 2047u;
                sidx[wv][(sl >> 5) * 40 + (sl & 31u)] = (uint16_t)(e >> 11);
                atomicOr(reinterpret_cast<uint32_t*>(&sidx[wv][(sl >> 5) * 40 + 32]), 1u << (sl & 31u));
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    /* one arc's candidates: x = its tight sources among the pending ones */
    auto take = [&](uint32_t x, uint32_t& H, uint32_t& T, int i) {
        uint32_t nb = x & ~H;
        T |= x & H;
        H |= x;
        while (nb) {
            my[__builtin_ctz(nb)] = (uint16_t)(i - a_t);
            nb &= nb - 1u;
        }
    };
    uint32_t lvb[5] = {0u, 0u, 0u, 0u, 0u};
    for (int d = 1; d <= nlev; ++d) {
        uint32_t pend = valid ? lev[(size_t)(d - 1) * plane + (size_t)t * nw + word] : 0u;
        if constexpr (PK) {
#pragma unroll
            for (int k = 0; k < 5; ++k)
                if ((d >> k) & 1) lvb[k] |= pend;
        }
        if (pn) pend &= ~*reinterpret_cast<const uint32_t*>(my + 32);
        if (!__any(pend != 0u)) continue;
        const int skip = pn ? d - 1 : 0; /* (w >= 1) */
        for (int w = d; w >= 1; --w) {
            if (w == skip) continue; /* lvl_pred_near_kernel took this group's pairs */
            const int g0 = ot[w], g1 = ot[w + 1];
            if (g0 == g1) continue;
            uint32_t H = 0, T = 0;
            if (w == d) {
                /* the direct arc (u, t): tight for the source u itself. 64 arcs per step, one per
                 * lane; the few whose source lies in this unit's chunk (~2 of C4's ~33 per
                 * weight) go to the lane owning the source's word. Distinct arcs have distinct
                 * sources, so there are no ties here and the order does not matter. */
                const int cw0 = c * 64 * 32; /* the chunk's first source (local index) */
                for (int i0 = g0; i0 < g1; i0 += 64) {
                    const int i = i0 + lane;
                    const int us = i < g1 ? (int)(arcs[i] & 0xFFFFu) - src0 : -1;
                    unsigned long long m =
                        __ballot(us >= 0 && us < nsrc && (unsigned)(us - cw0) < 64u * 32u);
                    while (m) {
                        const int j = __builtin_ctzll(m);
                        m &= m - 1ull;
                        const int uj = __builtin_amdgcn_readlane(us, j);
                        if ((uj >> 5) == word) take(pend & (1u << (uj & 31)), H, T, i0 + j);
                    }
                }
            }
            else { /* sixteen gathers in flight (a predicated tail), then their candidates in
                      * arc order */
                const char* base = reinterpret_cast<const char*>(lev + (size_t)(d - w - 1) * plane);
                /* LVL_PB gathers per batch, software-pipelined: the next batch's gathers are in
                 * flight while this batch's candidates are taken (C4: 7.2 -> 5.1 ms against 16
                 * unpipelined; 12 keeps 7 waves per SIMD -- 16 pipelined, 84 VGPRs and 5 waves,
                 * measured 6.2) */
                uint32_t v[LVL_PB], vn[LVL_PB];
                {
                    uint32_t a[LVL_PB];
#pragma unroll
                    for (int q = 0; q < LVL_PB; ++q) a[q] = aoff[g0 + q];
#pragma unroll
                    for (int q = 0; q < LVL_PB; ++q)
                        v[q] = g0 + q < g1 ? *reinterpret_cast<const uint32_t*>(base + (a[q] + lane4)) : 0u;
                }
                for (int i = g0; i < g1; i += LVL_PB) {
                    const int i2 = i + LVL_PB;
                    if (i2 < g1) {
                        uint32_t a[LVL_PB];
#pragma unroll
                        for (int q = 0; q < LVL_PB; ++q) a[q] = aoff[i2 + q];
#pragma unroll
                        for (int q = 0; q < LVL_PB; ++q)
                            vn[q] = i2 + q < g1 ? *reinterpret_cast<const uint32_t*>(base + (a[q] + lane4)) : 0u;
                    }
#pragma unroll
                    for (int q = 0; q < LVL_PB; ++q) take(v[q] & pend, H, T, i + q);
#pragma unroll
                    for (int q = 0; q < LVL_PB; ++q) v[q] = vn[q];
                    /* without the tie count the first tight arc is all a source needs: the walk
                     * of the weight ends once every pending source has one */
                    if (!ties && !__any((pend & ~H) != 0u)) break;
                }

            }
            tied += __builtin_popcount(T);
            pend &= ~H;
            if (!__any(pend != 0u)) break;
        }
    }
    if (ties) {
        for (int m = 32; m > 0; m >>= 1) tied += __shfl_xor(tied, m);
        if (lane == 0 && tied) atomicAdd(&ties[blockIdx.x & 1023u], (unsigned long long)tied);
    }
    /* Output, coalesced: the wave writes its 2,048 sources in four quarters of 512, lane l taking
     * 8 consecutive sources (another lane's entries, back from LDS), so every store instruction
     * covers one contiguous run (1 KB of int16 predecessors, 4 KB of reliabilities per quarter)
     * instead of 64 strided 16-B pieces. The walk's LDS writes are the wave's own. */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int cs0 = c * 64 * 32; /* the chunk's first local source */
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int sl0 = cs0 + q * 512 + lane * 8;
        /* the levels of sources sl0 .. sl0 + 7: bits (lane & 3) * 8.. of word q * 16 + lane / 4,
         * which lane q * 16 + lane / 4 holds (every lane takes part in the shuffles) */
        uint32_t lq[5];
#pragma unroll
        for (int k = 0; k < 5; ++k)
            lq[k] = PK ? ((uint32_t)__shfl((int)lvb[k], q * 16 + (lane >> 2)) >> ((lane & 3) * 8)) : 0u;
        if (sl0 >= nsrc) continue; /* nsrc is a multiple of 128: whole groups of 8 */
        const uint4 raw =
            *reinterpret_cast<const uint4*>(&sidx[wv][(q * 16 + (lane >> 2)) * 40 + (lane & 3) * 8]);
        const uint32_t ix[4] = {raw.x, raw.y, raw.z, raw.w};
        int32_t pv[8];
        double rv[8];
        uint32_t kv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t x = (ix[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
            const int sg = src0 + sl0 + e;
            const bool h = sg < n && sg != t && x != 0xFFFFu;
            const int k = a_t + (h ? (int)x : 0);
            pv[e] = h ? (int)(arcs[k] & 0xFFFFu) : -1;
            if constexpr (PK) {
                uint32_t l = 0;
#pragma unroll
                for (int kk = 0; kk < 5; ++kk) l |= ((lq[kk] >> e) & 1u) << kk;
                kv[e] = ((uint32_t)pv[e] & 0xFFFFu) | (h ? (uint32_t)rix[k] << 16 : 0u) |
                        (h ? l << 27 : 0u);
            }
            else
                rv[e] = h ? ar[k] : 0.0;
        }
        PT* pp = predT + (size_t)t * ldp + sl0;
        if constexpr (PK) { /* 32 B per lane: a wave's quarter is one 2-KB run */
            /* non-temporal: the words do not displace the gathered plane slices from the MALL
             * (5.16 against 5.31-5.36 ms with plain stores, r05pn) */
            typedef unsigned u32x4n __attribute__((ext_vector_type(4)));
            __builtin_nontemporal_store((u32x4n){kv[0], kv[1], kv[2], kv[3]}, reinterpret_cast<u32x4n*>(pp));
            __builtin_nontemporal_store((u32x4n){kv[4], kv[5], kv[6], kv[7]}, reinterpret_cast<u32x4n*>(pp + 4));
            continue;
        }
        double* rp = rT + (size_t)t * ldp + sl0;
        if constexpr (sizeof(PT) == 2) { /* -1 -> 0xFFFF, read back as int16 -1 */
            uint32_t w2[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                w2[e] = ((uint32_t)pv[2 * e] & 0xFFFFu) | ((uint32_t)pv[2 * e + 1] << 16);
            *reinterpret_cast<uint4*>(pp) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
        } else {
            *reinterpret_cast<int4*>(pp) = make_int4(pv[0], pv[1], pv[2], pv[3]);
            *reinterpret_cast<int4*>(pp + 4) = make_int4(pv[4], pv[5], pv[6], pv[7]);
        }
#pragma unroll
        for (int e = 0; e < 8; e += 2)
            *reinterpret_cast<double2*>(rp + e) = make_double2(rv[e], rv[e + 1]);
    }
}

template <typename PT>
/* The units walked chunk-major by all eight XCDs together (block u * 8 + XCD): the planes'
 * gathered slices are one source chunk's at a time for the whole GPU (8 MB per plane, in the
 * MALL), where XCD-private runs of chunks had 16 chunks' slices in flight (~384 MB on C4): 8.16
 * against 8.40 ms on C4.
 * Seven waves per SIMD are asked for: with the bucket code the register allocator, left alone,
 * settles at 77 VGPRs (six waves: 5.66 against 5.14 ms on C4 without the pre-pass); at 72 it
 * spills two registers of the packed form (12 B of scratch per lane) and the walk keeps its
 * rate (5.20). The level bit planes stay in registers: reading the plane words a second time in
 * the output stage instead (70 VGPRs, no spill) measured 7.9 ms. */
__global__ __launch_bounds__(256, 7) void lvl_pred_kernel(int n, int nw, int nchunk, int src0, int nsrc,
                                                       int nlev, unsigned nblk,
                                                       const int32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ arcs,
                                                       const uint32_t* __restrict__ aoff,
                                                       const double* __restrict__ ar,
                                                       const uint16_t* __restrict__ rix,
                                                       const uint32_t* __restrict__ lev,
                                                       PT* __restrict__ predT,
                                                       double* __restrict__ rT, size_t ldp,
                                                       unsigned long long* __restrict__ ties,
                                                       const uint32_t* __restrict__ bkt,
                                                       const uint32_t* __restrict__ bcnt, int cap) {
    /* per wave and lane: the winning arc of each of its 32 sources (index into t's arcs), 40 u16
     * per lane so the read-back is four 16-B loads */
    __shared__ __attribute__((aligned(16))) uint16_t sidx[4][64 * 40];
    const unsigned x = blockIdx.x & 7u, per = nblk >> 3, L = gridDim.x >> 3;
    for (unsigned u = blockIdx.x >> 3; u < per; u += L)
        lvl_pred_unit<PT>(u * 8u + x, sidx, n, nw, nchunk, src0, nsrc, nlev, off, arcs, aoff, ar,
                          rix, lev, predT, rT, ldp, ties, bkt, bcnt, cap);
}

/* The packed words source-major, no transpose (the packed form without the tie count): narrow
 * units, a template over the unit shape -- TPW targets per wave (64 / TPW words, lanes, per
 * target), NWV waves per workgroup, PB gathers per pipelined batch. The shape in use is <4, 4, 8>:
 * a wave covers 4 targets x 16 words (512 sources), 16 lanes per target: lane (g, l) owns word
 * c16 * 16 + l of target 16 * tg + 4 * wave + g. A workgroup's four waves hold 16 consecutive
 * targets of one 512-source sub-chunk, so after the walk each source has a 64-B run of its row
 * (16 targets x 4 B) in the workgroup: the walk's sidx entries are the staging tile, and the
 * output stage stores whole runs of pk[source][target] (row stride ld).
 * The gathered slices are 64 B, and a pass over all targets touches n x 64 B per plane (2 MB on
 * C4) where the 2,048-source units touch 8 MB; the walk itself is slower than the wide one (four
 * times the units re-read the arc offsets and the buckets) by less than the 1.65-ms transpose it
 * removes. The walk is bound by gather latency times waves in flight, so the shape is the one
 * that holds seven waves per SIMD: 256-thread workgroups of 22,784 B of LDS (seven per CU) and
 * 70 VGPRs without scratch (C4 5.5-5.6 ms against 5.9-6.0 for eight-wave workgroups
 * at six waves per SIMD; PB 10 and 12 and 8 targets x 8 words per wave measured and dropped).
 * The rule, the words and the walk's order are lvl_pred_unit's; what differs:
 *  - the in-arc group bounds and the walk's position are per lane group of a target; a group past
 *    its bound or without a pending source has its gathers predicated off; the wave leaves a
 *    weight when every group has, and a level when no lane has a pending source;
 *  - a group's next PB arc offsets come with one vector load (lane l takes arc l of its
 *    group) and reach the lanes by a cross-lane read inside the group (ds_bpermute), so no
 *    register is held per in-flight gather for them;
 *  - the direct arcs (w == d): lane l tests arc i0 + l of its group against the pending word of
 *    the lane that owns the arc's source (one ds_bpermute) and writes that lane's sidx entry and
 *    claimed bit through LDS;
 *  - lvl_pred_near_kernel's buckets stay keyed by (target, 2,048-source chunk): a group reads
 *    the bucket of its enclosing chunk and keeps the entries of its sub-chunk's sources;
 *  - a workgroup walks up to four sub-chunks of one chunk back to back for its 16 targets (the
 *    unit loop below; the rule for the run length is srt_levels_pred's);
 *  - the output stage reads one word per pair, apk[k] = source | rix << 16 (lvl_apk_kernel, once
 *    per build), where lvl_pred_unit gathers arcs[k] and rix[k]. C4, the kernel per launch as
 *    bench.py times it: 5.60 ms, 5.45 with the arc word, 5.37 with whole-chunk units on top
 *    (which alone measured no gain: DESIGN 5.7).
 * LDS per lane, LVL_RW_LANE = 22 words: 16 of sidx (32 u16) and the claimed word; words 17.. are
 * idle during the walk and hold the target's group bounds off[t][0 .. 32] (31 levels at most:
 * weight w's bound is in lane w % WPT, word 17 + w / WPT); after the walk, behind a wave-level
 * sync (a target never leaves its wave), the five level planes take words 16..20. A target's
 * lanes are followed by 4 words of padding, the first of which keeps off[t][0] for the output
 * stage. A lane's words are 8-B aligned (88 B apart), so the tile is accessed in 8-B pieces; the
 * 16 lanes of a target start on the 16 even banks of 32 (24 words apart they shared 4), two
 * targets of a 32-lane group 4 banks apart share them two ways. The output stage's 8-B plane
 * reads are conflict-free (quads 4 x 356 words apart: 16 banks of 64; words 22 apart), its 4-B
 * sidx reads two-way (quads 16 banks of 32 apart). */
#define LVL_RW_LANE 22
template <int TPW, int NWV, int PB>
__global__ __launch_bounds__(NWV * 64, NWV == 4 ? 7 : 6) void lvl_pred_rows_kernel(
    int n, int nw, int nchunk, int src0, int nsrc, int nlev, unsigned ntg, unsigned nunit, int S,
    const int32_t* __restrict__ off, const uint32_t* __restrict__ arcs, const uint32_t* __restrict__ aoff,
    const uint32_t* __restrict__ apk, const uint32_t* __restrict__ lev, uint32_t* __restrict__ pk, size_t ld,
    const uint32_t* __restrict__ bkt, const uint32_t* __restrict__ bcnt, int cap) {
    constexpr int WPT = 64 / TPW;                /* words (lanes) per target */
    constexpr int NT = TPW * NWV;                  /* targets per workgroup */
    constexpr int SUB = WPT * 32;                  /* sources per sub-chunk */
    constexpr int TGT = WPT * LVL_RW_LANE + 4;     /* a target's words: its lanes' and the padding */
    constexpr int NB = (33 + WPT - 1) / WPT;       /* bound words per lane: off[t][0 .. 32] */
    static_assert(PB <= WPT && NB <= 5 && NT % 4 == 0 && (NT / 4) * (SUB / 8) == NWV * 64, "unit shape");
    __shared__ __attribute__((aligned(16))) uint32_t sw[NT * TGT];
    const int lane = threadIdx.x & 63, l = lane & (WPT - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int gl = wv * TPW + lane / WPT; /* the lane's target inside the workgroup's NT */
    uint32_t* tgt = sw + gl * TGT;
    uint32_t* mine = tgt + l * LVL_RW_LANE;
    uint16_t* my = reinterpret_cast<uint16_t*>(mine);
    const size_t plane = (size_t)n * nw;
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    /* p anywhere in the lane's WPT-lane group (every lane of the wave calls it) */
    auto gany = [&](bool p) -> bool {
        return ((__ballot(p) >> (lane & (64 - WPT))) & ((1ull << WPT) - 1ull)) != 0ull;
    };
    /* A unit is (target group, run of S consecutive sub-chunks of one 2,048-source chunk; S 1, 2
     * or 4, so a run never leaves its chunk): the workgroup keeps its NT targets and walks the
     * run's sub-chunks back to back, so the bounds, the arc offsets, the bucket and the arcs[] /
     * rix[] lines of its targets, the same for every sub-chunk of the chunk, are read again by
     * the workgroup that had them moments ago. Run-major, consecutive workgroups (one per XCD
     * in turn) on consecutive target groups: the whole GPU gathers from one run's slices at a
     * time. Everything a sub-chunk leaves in the tile or in registers is rebuilt for the next. */
    const int nsub = (nw + WPT - 1) / WPT;
    for (unsigned u = blockIdx.x; u < nunit; u += gridDim.x) {
        const int run = (int)(u / ntg), tg = (int)(u % ntg);
        const int t = tg * NT + gl;
        const bool tv = t < n;
        for (int c16 = run * S, ce = min(c16 + S, nsub); c16 < ce; ++c16) {
            const int word = c16 * WPT + l;
            const bool act = tv && word < nw;
            const int cs0 = c16 * SUB; /* the sub-chunk's first local source */
#pragma unroll
            for (int q = 0; q < 16; q += 2) /* (a lane's words are 8-B aligned: 22 words apart) */
                *reinterpret_cast<uint2*>(mine + q) = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
            mine[16] = 0u;
            {
                const int32_t* ot = off + (size_t)(tv ? t : 0) * LVL_STRIDE;
#pragma unroll
                for (int k = 0; k < NB; ++k) mine[17 + k] = tv ? (uint32_t)ot[k * WPT + l] : 0u;
                if (l == 0) tgt[WPT * LVL_RW_LANE] = tv ? (uint32_t)ot[0] : 0u;
            }
            wave_sync();
            auto otl = [&](int w) -> int { return (int)tgt[(w & (WPT - 1)) * LVL_RW_LANE + 17 + w / WPT]; };
            const int a_t = otl(0);
            const uint32_t lane4 = (uint32_t)(act ? word : 0) * 4u;
            /* the bucket of (t, enclosing chunk): the entries of this sub-chunk's sources into
             * their owners' sidx slots and claimed words. An overflowed bucket is ignored. */
            bool pn = false;
            if (bkt) {
                const size_t un = (size_t)(tv ? t : 0) * nchunk + c16 / (2048 / SUB);
                const int k = tv ? (int)bcnt[un] : cap + 1;
                pn = k <= cap;
                const uint32_t* ub = bkt + un * cap;
                for (int i = l; pn && i < k; i += WPT) {
                    const uint32_t e = ub[i], sl = e & 2047u;
                    if ((int)(sl / SUB) != (c16 & (2048 / SUB - 1))) continue;
                    uint32_t* o = tgt + ((sl >> 5) & (uint32_t)(WPT - 1)) * LVL_RW_LANE;
                    reinterpret_cast<uint16_t*>(o)[sl & 31u] = (uint16_t)(e >> 11);
                    atomicOr(&o[16], 1u << (sl & 31u));
                }
                wave_sync();
            }
            uint32_t lvb[5] = {0u, 0u, 0u, 0u, 0u};
            for (int d = 1; d <= nlev; ++d) {
                uint32_t pend = act ? lev[(size_t)(d - 1) * plane + (size_t)t * nw + word] : 0u;
#pragma unroll
                for (int k = 0; k < 5; ++k)
                    if ((d >> k) & 1) lvb[k] |= pend;
                pend &= ~mine[16];
                if (!__any(pend != 0u)) continue;
                for (int w = d; w >= 1; --w) {
                    const bool gp = gany(pend != 0u);
                    const int g0 = otl(w);
                    int g1 = otl(w + 1);
                    if (!gp || (pn && w == d - 1)) g1 = g0; /* nothing pending, or the pre-pass took this group */
                    if (!__any(g0 < g1)) continue;
                    if (w == d) {
                        /* the direct arc (u, t): tight for the source u itself; distinct arcs have
                         * distinct sources, so the order does not matter */
                        for (int i0 = g0; __any(i0 < g1); i0 += WPT) {
                            const int i = i0 + l;
                            const int us = i < g1 ? (int)(arcs[i] & 0xFFFFu) - src0 : -1;
                            const bool in = us >= 0 && us < nsrc && (unsigned)(us - cs0) < (unsigned)SUB;
                            const int ow = in ? (us >> 5) & (WPT - 1) : 0;
                            const uint32_t op = (uint32_t)__shfl((int)pend, ow, WPT);
                            if (in && ((op >> (us & 31)) & 1u)) {
                                uint32_t* o = tgt + ow * LVL_RW_LANE;
                                reinterpret_cast<uint16_t*>(o)[us & 31] = (uint16_t)(i - a_t);
                                atomicOr(&o[16], 1u << (us & 31));
                            }
                        }
                        wave_sync();
                        pend &= ~mine[16];
                    } else {
                        /* PB gathers per batch, software-pipelined as lvl_pred_unit's; e is the
                         * group's end of the walk, pulled in once none of its sources is pending */
                        const char* base = reinterpret_cast<const char*>(lev + (size_t)(d - w - 1) * plane);
                        int i = g0, e = g1;
                        uint32_t v[PB], vn[PB];
                        {
                            const uint32_t aq = l < PB && i + l < e ? aoff[i + l] : 0u;
#pragma unroll
                            for (int q = 0; q < PB; ++q) {
                                const uint32_t a = (uint32_t)__shfl((int)aq, q, WPT);
                                v[q] = i + q < e ? *reinterpret_cast<const uint32_t*>(base + (a + lane4)) : 0u;
                            }
                        }
                        while (__any(i < e)) {
                            const int i2 = i + PB;
                            {
                                const uint32_t aq = l < PB && i2 + l < e ? aoff[i2 + l] : 0u;
#pragma unroll
                                for (int q = 0; q < PB; ++q) {
                                    const uint32_t a = (uint32_t)__shfl((int)aq, q, WPT);
                                    vn[q] = i2 + q < e ? *reinterpret_cast<const uint32_t*>(base + (a + lane4)) : 0u;
                                }
                            }
#pragma unroll
                            for (int q = 0; q < PB; ++q) { /* a source takes its first tight arc */
                                uint32_t nb = v[q] & pend;
                                pend &= ~nb;
                                while (nb) {
                                    my[__builtin_ctz(nb)] = (uint16_t)(i + q - a_t);
                                    nb &= nb - 1u;
                                }
                            }
#pragma unroll
                            for (int q = 0; q < PB; ++q) v[q] = vn[q];
                            i = i2;
                            if (!gany(pend != 0u)) e = min(e, i);
                        }
                    }
                    if (!__any(pend != 0u)) break;
                }
            }
            wave_sync(); /* the bounds' last read (another lane's words 17..) before the planes */
#pragma unroll
            for (int k = 0; k < 5; ++k) mine[16 + k] = lvb[k];
            __syncthreads();
            /* Output: thread (tq = thread % NQ, octet = thread / NQ) takes 8 consecutive sources --
             * bits oct * 8.. of word wd, octet = 4 * wd + oct -- of targets 4 * tq .. + 3: one 16-B
             * piece per source, the NQ tq lanes one source's run of NT * 4 B, so every store
             * instruction writes 64 / NQ whole runs with consecutive lanes consecutive in memory.
             * nsrc is a multiple of 128: whole groups of 8. */
            {
                constexpr int NQ = NT / 4;
                const int tq = (int)threadIdx.x % NQ, kq = (int)threadIdx.x / NQ;
                const int wd = kq >> 2, oct = kq & 3;
                const int sl0 = cs0 + wd * 32 + oct * 8, t0 = tg * NT + 4 * tq;
                if (sl0 < nsrc && t0 < n) {
                    uint32_t lq[4][5];
                    int at[4];
                    const uint32_t* ps = sw + (4 * tq) * TGT + wd * LVL_RW_LANE + oct * 4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint32_t* p = sw + (4 * tq + j) * TGT;
                        at[j] = (int)p[WPT * LVL_RW_LANE];
                        p += wd * LVL_RW_LANE;
                        const uint2 b0 = *reinterpret_cast<const uint2*>(p + 16);
                        const uint2 b1 = *reinterpret_cast<const uint2*>(p + 18);
                        lq[j][0] = b0.x >> (oct * 8), lq[j][1] = b0.y >> (oct * 8);
                        lq[j][2] = b1.x >> (oct * 8), lq[j][3] = b1.y >> (oct * 8);
                        lq[j][4] = p[20] >> (oct * 8);
                    }
                    /* the sidx entries come from the tile a source pair at a time: held in registers
                     * for all eight sources they are 12 more VGPRs than seven waves per SIMD leave */
#pragma unroll 1
                    for (int e = 0; e < 8; ++e) {
                        const int sg = src0 + sl0 + e;
                        uint32_t kv[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint32_t x = (ps[j * TGT + (e >> 1)] >> (16 * (e & 1))) & 0xFFFFu;
                            const bool h = sg < n && sg != t0 + j && t0 + j < n && x != 0xFFFFu;
                            const int k = at[j] + (h ? (int)x : 0);
                            uint32_t lv = 0;
#pragma unroll
                            for (int kk = 0; kk < 5; ++kk) lv |= ((lq[j][kk] >> e) & 1u) << kk;
                            kv[j] = h ? (apk[k] | lv << 27) : 0xFFFFu;
                        }
                        uint32_t* pp = pk + (size_t)(sl0 + e) * ld + t0;
                        if (t0 + 3 < n) { /* non-temporal, as lvl_pred_unit's words */
                            typedef unsigned u32x4n __attribute__((ext_vector_type(4)));
                            __builtin_nontemporal_store((u32x4n){kv[0], kv[1], kv[2], kv[3]},
                                                        reinterpret_cast<u32x4n*>(pp));
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (t0 + j < n) pp[j] = kv[j];
                        }
                    }
                }
            }
            __syncthreads(); /* the next sub-chunk's walk rewrites the tile */
        }
    }
}

__global__ void lvl_sum_kernel(const unsigned long long* __restrict__ v, int k,
                               unsigned long long* __restrict__ out) {
    unsigned long long s = 0;
    for (int i = threadIdx.x; i < k; i += blockDim.x) s += v[i];
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    __shared__ unsigned long long w[16];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long x = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); i++) x += w[i];
        *out += x;
    }
}

/* ---- host ----------------------------------------------------------------------------------- */
/* Streaming-gather rate assumed by the level budget (bytes per ms) and the cost of one level's
 * launch + completion read-back. */
#define LVL_BYTES_PER_MS 4.0e9
#define LVL_LEVEL_MS 0.03

/* Estimated time of levels 1..L (ms): every level gathers one 4-B word per (arc of weight < d,
 * source word) and reads/writes R and Delta once. */
/* the largest level budget L whose predicted time stays within limit_ms: level d gathers a row of
 * nw words per arc of weight < d and touches three planes (one running sum, not a sum per L: the
 * budget of a graph like C4 passes 200 levels, and the quadratic form cost ~30 us of host time
 * on every build's critical path) */
static int lvl_budget(const unsigned long long* hist, double ntgt, double nw, double limit_ms) {
    double t = 0, below = 0; /* arcs with weight < d */
    int L = 0;
    for (int d = 1; d <= LVL_WMAX; ++d) {
        if (d >= 2) below += (double)hist[d - 1];
        t += (below * nw * 4.0 + ntgt * nw * 4.0 * 3.0) / LVL_BYTES_PER_MS + LVL_LEVEL_MS;
        if (t > limit_ms) break;
        L = d;
    }
    return L;
}

/* Bucket capacity of lvl_pred_near_kernel from the weight histogram: the expected entries of a
 * unit (one target, up to 2,048 sources) with headroom, as a power of two. A pair (s, t) enters a
 * bucket at level d when some in-arc (u, d - 1) of t has s in u's weight-1 run -- probability
 * c_d = a[d-1] * a[1] / n with a[w] = hist[w] / n arcs of weight w into a vertex -- and no walk
 * shorter than d joins the pair. The walks of total weight k between a pair are taken as Poisson
 * with mean N[k] = hist[k] / n^2 + sum_w a[w] * N[k-w] (random arcs), so the pair is still open at
 * level d with probability exp(-sum_{k<d} N[k]). On C4 (a ~ 33, n = 32,768) this gives 3.3% at
 * levels 2 and 3 and 1.0% at level 4, 155 entries per unit; six standard deviations of headroom
 * make it 256. A unit past its capacity only falls back to the walk, so the model need not be
 * safe, and a dense Delta_1 gives a capacity past 1,024, which turns the pre-pass off. */
static int lvl_pn_cap(const unsigned long long* hist, int n, int nsrc, int D) {
    const double dn = (double)n;
    double N[LVL_WMAX + 2], below = 0, mean = 0;
    D = min(D, LVL_WMAX);
    for (int d = 1; d <= D; ++d) {
        double x = (double)hist[d] / (dn * dn);
        for (int w = 1; w < d; ++w) x += (double)hist[w] / dn * N[d - w];
        N[d] = x;
        if (d >= 2) mean += fmin(1.0, (double)hist[d - 1] / dn * (double)hist[1] / dn / dn) * exp(-below);
        below += x;
    }
    mean *= (double)min(2048, nsrc);
    const double need = mean + 6.0 * sqrt(mean);
    int cap = 16;
    while (cap < 2048 && (double)cap < need) cap <<= 1;
    return (double)cap < need ? 4096 : cap; /* (4096: more than a bucket can ever hold) */
}

/* persistent grid of a unit kernel (workgroups of `threads`): its resident workgroups per CU x the
 * CUs, a multiple of 8 (one share per XCD), at most the unit blocks */
static unsigned lvl_grid(const void* fn, unsigned nblk, int reserve_cus = 0, int threads = 256) {
    int dev = 0, cus = 256, per = 4;
    if (hipGetDevice(&dev) == hipSuccess)
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    cus = max(8, cus - reserve_cus);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn, threads, 0) != hipSuccess || per < 1) per = 4;
    (void)hipGetLastError();
    unsigned g = (unsigned)(cus * per) & ~7u;
    if (g < 8) g = 8;
    return g < nblk ? g : nblk;
}

/* The state a successful level build keeps for its post pass (srt_levels_pred), per state slot:
 * the sorted in-arcs with their reliabilities and the level planes. The build (lvl_build) fills it
 * in place and sets `held` last; until then the fields are the build's own (arcs, ar and total are
 * its extraction cursor). Freed by srt_levels_release (stream-ordered). */
typedef struct {
    int held;
    int n, nw, nchunk, row0, nrows, D;
    unsigned nblk;
    int32_t* off;
    uint32_t* arcs;
    uint32_t* aoff;
    double* ar;
    uint16_t* rix; /* packed form: each arc's index into rtab (NULL: more than LVL_RT_CAP values) */
    uint32_t* apk; /* source-major packed form: each arc's source | rix << 16 (lvl_apk_kernel) */
    double* rtab;
    int ntab;
    uint32_t* lev;
    uint8_t* l8; /* u8 distance rows (nrows x ld) for the reliability pass */
    srt_lvl_post_form post; /* the post pass: packed words with levels + rel_pk (no lat / l8 rows), or u8 */
    int fpkw;    /* SRT_FORM pkw as the build read it: 3 / 4 force the narrow units' length */
    int fbcap;   /* SRT_FORM bcap as the build read it: the pre-pass's bucket hook */
    int total;   /* in-arcs held (w <= lmax) */
    int pn_cap;  /* lvl_pred_near_kernel: the bucket capacity the weight histogram asks for */
    unsigned long long* dkey; /* the diagonal rule's key per local row (undirected rows form) */
    const double* r_rows;
    void* p[40]; /* every allocation of the build (LVL_ALLOC), freed together */
    int k;
    hipStream_t st;
    hipEvent_t wlast; /* the streamed extraction's last weight (side stream), or NULL */
} lvl_state;
static lvl_state g_lvl[SRT_STATE_SLOTS];

static void lvl_free(lvl_state* L, hipStream_t st) {
    if (L->wlast) (void)hipStreamWaitEvent(st, L->wlast, 0); /* the side stream is done with them */
    for (int i = 0; i < L->k; i++)
        if (L->p[i]) (void)hipFreeAsync(L->p[i], st);
    memset(L, 0, sizeof(*L));
}

void srt_levels_release(hipStream_t st) { lvl_free(&g_lvl[srt_state_slot()], st); }

/* the diagonal rule of the held build's rows into d / rel (row stride ld); 0 = applied, 1 = the
 * build kept no keys (directed: the caller's dense_diag_kernel) */
int srt_levels_diag(int n, int ld, uint32_t* d, double* rel, hipStream_t st, int* applied) {
    const lvl_state* L = &g_lvl[srt_state_slot()];
    *applied = 0;
    if (!L->held || !L->dkey) return SRT_OK;
    const int lrows = max(0, min(L->nrows, n - L->row0));
    if (lrows > 0)
        lvl_diag_kernel<<<srt_ceil_div(lrows, 256), 256, 0, st>>>(n, ld, L->row0, lrows, L->dkey,
                                                                  L->r_rows, d, rel);
    SRT_HIPCHK(hipGetLastError());
    *applied = 1;
    return SRT_OK;
}

/* the held build's table of distinct arc reliabilities (packed form), NULL when it has none */
const double* srt_levels_rtab(int* ntab) {
    const lvl_state* L = &g_lvl[srt_state_slot()];
    *ntab = L->held && L->rix ? L->ntab : 0;
    return L->held && L->rix ? L->rtab : NULL;
}

const uint8_t* srt_levels_l8(void) {
    const lvl_state* L = &g_lvl[srt_state_slot()];
    return L->held ? L->l8 : NULL;
}

#define LVL_ALLOC(ptr, bytes)                                      \
    do {                                                           \
        if (L->k >= (int)(sizeof(L->p) / sizeof(L->p[0]))) {       \
            srt_set_error("levels: allocation table full");        \
            return SRT_E_NOMEM;                                    \
        }                                                          \
        SRT_HIPCHK(srt_malloc_async(&(ptr), (bytes), st));         \
        L->p[L->k++] = (void*)(ptr);                               \
    } while (0)
/* the same, but a failed allocation only clears *ok (the caller agrees on a verdict first) */
#define LVL_TRY_ALLOC(ptr, bytes, ok)                                                   \
    do {                                                                                \
        (ptr) = NULL;                                                                   \
        if (*(ok) && L->k < (int)(sizeof(L->p) / sizeof(L->p[0])) &&                    \
            srt_malloc_async(&(ptr), (bytes), st) == hipSuccess) {                      \
            L->p[L->k++] = (void*)(ptr);                                                \
        } else {                                                                        \
            (void)hipGetLastError();                                                    \
            (ptr) = NULL;                                                               \
            *(ok) = 0;                                                                  \
        }                                                                               \
    } while (0)

/* One stream-ordered allocation for a group of buffers (each 256-B aligned): a build's ~20
 * scratch buffers cost one pool call instead of twenty on the host's critical path */
struct lvl_arena {
    void** p[24];
    size_t b[24];
    int k = 0;
    template <typename T>
    void add(T** ptr, size_t bytes) {
        p[k] = reinterpret_cast<void**>(ptr);
        b[k++] = bytes;
    }
    size_t total() const {
        size_t t = 0;
        for (int i = 0; i < k; i++) t += (b[i] + 255) & ~(size_t)255;
        return t;
    }
    void carve(char* base) const {
        for (int i = 0; i < k; i++) {
            *p[i] = base;
            base += (b[i] + 255) & ~(size_t)255;
        }
    }
};

/* bytes the build can still take from the device: free memory plus what the library's scratch
 * pool holds unused (its release threshold keeps freed blocks mapped) */
static size_t lvl_avail_bytes(void) {
    const int cap_mb = srt_form_int("memcap", -1); /* test hook: a nearly full device */
    if (cap_mb >= 0) return (size_t)cap_mb << 20;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    uint64_t res = 0, used = 0;
    hipMemPool_t pool = srt_scratch_pool();
    if (hipMemPoolGetAttribute(pool, hipMemPoolAttrReservedMemCurrent, &res) == hipSuccess &&
        hipMemPoolGetAttribute(pool, hipMemPoolAttrUsedMemCurrent, &used) == hipSuccess && res > used)
        fr += (size_t)(res - used);
    (void)hipGetLastError();
    return fr;
}

/* settled fraction of all pairs the first batch must reach for the build to go on */
#define LVL_MIN_SETTLED 0.25

/* The host-side words of a build (one allocation, zeroed): the weight histogram, the completion
 * flags, the agreement words and the settled-pair counter, and the batch vote. Offsets in u64. */
#define LVL_H_INC 256                            /* int dinc[LVL_WMAX + 1], then dflag[2] */
#define LVL_H_AGREE 512                          /* int32 agreement words [3]; u64 nset at +2 */
#define LVL_H_VOTE 520                           /* int32 [4] */
#define LVL_H_WORDS (LVL_H_VOTE + 2)

/* N > 1, the end of a batch of levels: this rank's vote -- not done (its last level left a pair
 * unsettled) and its settled-pair count in 21-bit limbs -- for one sum all-reduce, so every rank
 * takes the batch's decision (stop, continue, extract heavier arcs, or Floyd-Warshall) from the
 * same numbers */
__global__ void lvl_vote_kernel(const int* __restrict__ inc_last,
                                const unsigned long long* __restrict__ nset,
                                int32_t* __restrict__ vote) {
    if (threadIdx.x) return;
    const unsigned long long s = *nset;
    vote[0] = *inc_last != 0;
    vote[1] = (int32_t)(s & 0x1FFFFFull);
    vote[2] = (int32_t)((s >> 21) & 0x1FFFFFull);
    vote[3] = (int32_t)(s >> 42);
}

/* u64 words of one rank's block of distinct reliabilities: two int32 flags (probe overflow, count),
 * then up to LVL_RT_CAP values */
constexpr size_t LVL_GB = LVL_RT_CAP + 1;
/* wev[LVL_PREP]: the side stream's preparation (lvl_agree); wev[w]: weight w's arcs have arrived */
#define LVL_PREP (LVL_BATCH + 1)

/* What the phases of one srt_levels_build share. It lives on that function's stack and owns
 * nothing: device memory belongs to the held state L (LVL_ALLOC), which the phases also fill in
 * place -- L->off, aoff, lev, rix, rtab, dkey from the arenas, L->arcs / ar / total as the cursor
 * of the current extraction, L->D and nblk from the levels. */
struct lvl_build {
    lvl_state* L;
    /* the shape (dr: directed and N > 1; solo: a timing-only communicator) and the caller's rows */
    int n, ld, row0, nrows, lrows, max_rows, nw, nchunk, R, me, fpkw;
    bool directed, dr, solo;
    size_t plane, ncnt, xn, dnt; /* words of a level plane, counts, exchange words, directed runs */
    double fw_ms;
    const srt_comm* comm;
    hipStream_t st, wcs; /* wcs: the side stream, wev its events */
    hipEvent_t* wev;
    evpool_t* evp;
    const uint32_t* w_rows;
    const double* r_rows;
    uint32_t* lat_rows;
    /* the host-side words (LVL_H_*); dflag: [0] probe overflow, [1] distinct values */
    unsigned long long* dhist;
    int32_t *dinc, *dflag, *dagree, *dvote;
    /* arena 1, the count pass (with L->off and L->dkey) */
    int32_t *cnt, *tb, *xbuf, *scnt;
    uint32_t* stash;
    unsigned long long* H;
    uint16_t *map, *cg;
    /* arena 2, the extraction and the levels (with L->aoff, lev, rix, rtab); arena 3, the wire */
    uint32_t *arcsA, *arcs2, *Rb, *wire;
    double *arA, *ar2, *gat;
    int32_t *seg, *packed, *tq, *oq, *dcur, *offw;
    void *tmp, *stmp;
    size_t tmp_bytes, sb;
    uint8_t* done;
    char* dwire;
    /* pinned host views: the exchange, the agreement, the wire's bases, the union table + flags */
    int32_t *hx, *hag, *hwt;
    unsigned long long *pin, *ht;
    unsigned long long hist[LVL_STRIDE]; /* summed over the ranks; [0] the stash overflows */
    int32_t wmax[LVL_BATCH + 1];         /* undirected N > 1: the largest rank's arcs of weight w */
    std::vector<unsigned long long>* u;  /* the union of the exchanged reliability blocks (per slot) */
    /* this rank's plan, then the agreed values; the levels' outcome */
    int failed, lx_own, lmax, lx, ok, stream_ok, all_done, hflag[2];
    bool fit, want_rt, prepped;
    int64_t gathered;
    /* the extraction cursor (with L->arcs, ar, total): the weights the side stream delivers, their
     * arcs carry table indices, the weights enqueued / placed so far, the directed ranks' counts */
    int streamed, wnum, wq, wp;
    lvl_dcnt dcn;
};

/* a group of buffers in one allocation (soft: a failure clears *okp) */
static void lvl_commit(lvl_build& b, const lvl_arena& a, int* okp) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    char* base = NULL;
    if (a.k) LVL_TRY_ALLOC(base, a.total(), okp);
    if (base) a.carve(base);
}

/* the arcs of weight <= lw (global: the summed histogram) */
static int64_t lvl_arcs_upto(const unsigned long long* hist, int lw) {
    int64_t t = 0;
    for (int x = 1; x <= lw; ++x) t += (int64_t)hist[x];
    return t;
}

/* from the exchange: the largest rank's arcs of the weights w0..w1 (alike on every rank) */
static uint64_t lvl_largest_block(const lvl_build& b, int w0, int w1) {
    uint64_t mx = 0;
    for (int q = 0; q < b.R; q++) {
        uint64_t t = 0;
        for (int w = w0; w <= w1; ++w) {
            const int32_t* c = b.hx + LVL_X_LIMBS +
                               (b.dr ? (size_t)q * LVL_X_DCNT + 2 * w : (size_t)q * LVL_X_CNT + 2 * (w - 1));
            t += (uint32_t)c[0] | ((uint32_t)c[1] << 16);
        }
        mx = t > mx ? t : mx;
    }
    return mx;
}
/* directed, N > 1: arcs of the largest rank's block of the weights <= lw, made even */
static size_t lvl_dblock(const lvl_build& b, int lw) { return (lvl_largest_block(b, 1, lw) + 1) & ~(uint64_t)1; }

/* The sorted union of R reliability blocks (LVL_GB words each; only >= 0: that block stands for
 * every rank, a solo rank's peers) into u: the same table on every rank. -> it can number the
 * arcs: no probe overflow, 1..LVL_RT_CAP values. The blocks come in hash-slot order and mostly
 * repeat each other (C4: ~500 values per rank, the same ones), so they are deduplicated through
 * an open-addressing set first and only the distinct values sorted: sorting the concatenation
 * (4,000 values at N = 8) cost ~0.1-0.2 ms of host time on the critical path. A solo rank's peers
 * hold its own values (their rows are shifted copies of its rows), so it pays the same. */
static bool lvl_union(const unsigned long long* blocks, int R, int only, std::vector<unsigned long long>& u) {
    u.clear();
    size_t all = 0;
    for (int q = 0; q < R; q++) {
        const int32_t* hd = reinterpret_cast<const int32_t*>(blocks + (size_t)(only >= 0 ? only : q) * LVL_GB);
        if (hd[0] || hd[1] > LVL_RT_CAP) return false;
        all += (size_t)max(hd[1], 0);
    }
    size_t cap = 64;
    while (cap < 2 * all) cap <<= 1;
    std::vector<unsigned long long>& set = g_lvl_uset[srt_state_slot()];
    set.assign(cap, ~0ull); /* (a NaN pattern: never a reliability's bits) */
    int shift = 64;
    for (size_t c = cap; c > 1; c >>= 1) --shift;
    for (int q = 0; q < R; q++) {
        const unsigned long long* v = blocks + (size_t)(only >= 0 ? only : q) * LVL_GB;
        const int nv = reinterpret_cast<const int32_t*>(v)[1];
        for (int k = 1; k <= nv; ++k) {
            size_t h = (size_t)((v[k] * 0x9E3779B97F4A7C15ull) >> shift);
            while (set[h] != ~0ull && set[h] != v[k]) h = (h + 1) & (cap - 1);
            if (set[h] == ~0ull) {
                set[h] = v[k];
                u.push_back(v[k]);
            }
        }
    }
    std::sort(u.begin(), u.end());
    return !u.empty() && u.size() <= (size_t)LVL_RT_CAP;
}

/* Step 1: the count pass and, N > 1, this rank's slots of the exchange. Its buffers are taken
 * softly: a rank short of memory sends every rank to the FW through the failure count it adds to
 * the exchange (its slots stay zero). */
static int lvl_count_pass(lvl_build& b) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int n = b.n, ld = b.ld, row0 = b.row0, nrows = b.nrows, lrows = b.lrows, R = b.R, me = b.me;
    const size_t ncnt = b.ncnt;
    LVL_ALLOC(b.dhist, LVL_H_WORDS * sizeof(unsigned long long));
    SRT_HIPCHK(hipMemsetAsync(b.dhist, 0, LVL_H_WORDS * sizeof(unsigned long long), st));
    b.dinc = reinterpret_cast<int*>(b.dhist + LVL_H_INC);
    b.dagree = reinterpret_cast<int32_t*>(b.dhist + LVL_H_AGREE);
    b.dvote = reinterpret_cast<int32_t*>(b.dhist + LVL_H_VOTE);
    b.dflag = b.dinc + LVL_WMAX + 1;
    lvl_arena a1;
    a1.add(&b.cnt, (ncnt + 1) * sizeof(int32_t));
    a1.add(&L->off, (ncnt + 1) * sizeof(int32_t));
    a1.add(&b.tb, 2 * ((size_t)ld + 1) * sizeof(int32_t)); /* per-target totals, their scan */
    a1.add(&b.H, LVL_RT_SLOTS * sizeof(unsigned long long));
    a1.add(&b.map, LVL_RT_SLOTS * sizeof(uint16_t));
    if (!b.directed) {
        a1.add(&L->dkey, (size_t)nrows * sizeof(unsigned long long));
        a1.add(&b.stash, (size_t)nrows * LVL_STASH_CAP * sizeof(uint32_t));
        a1.add(&b.scnt, (size_t)nrows * 4 * sizeof(int32_t));
    }
    b.xn = b.dr ? lvl_xd_words(R) : R > 1 ? lvl_x_words(R) : 0;
    if (R > 1) a1.add(&b.xbuf, b.xn * sizeof(int32_t));
    lvl_commit(b, a1, &b.ok);
    if (!b.ok) return SRT_OK;
    int32_t* const cnt = b.cnt;
    SRT_HIPCHK(hipMemsetAsync(cnt, 0, (ncnt + 1) * sizeof(int32_t), st));
    if (b.dr) { /* this rank's rows' contribution to every target's counts */
        if (lrows > 0)
            lvl_arcs_colwin_kernel<false><<<dim3(ld / 64, srt_ceil_div(lrows, LVL_DROWS)), 256, 0, st>>>(
                n, ld, row0, lrows, b.w_rows, cnt, 0);
    } else if (b.directed)
        lvl_arcs_cols_kernel<false><<<ld / 64, 256, 0, st>>>(n, ld, b.w_rows, cnt, 0, NULL, NULL);
    else
        lvl_arcs_rows_kernel<false><<<nrows, 256, 0, st>>>(n, ld, row0, b.w_rows, cnt, 0, NULL, NULL, NULL,
                                                           NULL, L->dkey, b.stash, b.scnt, b.dhist);
    if (b.solo && lrows > 0) lvl_solo_counts_kernel<<<n, 256, 0, st>>>(n, row0, nrows, lrows, cnt);
    SRT_HIPCHK(hipGetLastError());
    /* this rank's rows (a solo rank: every row of its synthesised counts, which are its own
     * rows' n / lrows times over when that divides) */
    const bool rep = b.solo && lrows > 0 && lrows == nrows && n % lrows == 0;
    const bool own = R > 1 && !b.dr && (!b.solo || rep); /* (directed: every target's row) */
    lvl_hist_kernel<<<own ? 256 : 1024, 256, 0, st>>>(own ? (size_t)(rep ? lrows : nrows) * LVL_STRIDE : ncnt,
                                                     own ? cnt + (size_t)row0 * LVL_STRIDE : cnt, b.dhist,
                                                     rep ? (unsigned)(n / lrows) : 1u);
    SRT_HIPCHK(hipGetLastError());
    if (R == 1) return SRT_OK;
    int32_t* const xcnt = b.xbuf + LVL_X_LIMBS;
    SRT_HIPCHK(hipMemsetAsync(b.xbuf, 0, b.xn * sizeof(int32_t), st));
    lvl_hist_limbs_kernel<<<1, LVL_STRIDE, 0, st>>>(1, b.dhist, b.xbuf);
    if (b.dr)
        lvl_drank_counts_kernel<<<1, LVL_STRIDE, 0, st>>>(b.dhist, xcnt + (size_t)me * LVL_X_DCNT);
    else
        lvl_rank_counts_kernel<<<dim3(LVL_BATCH, b.solo ? R : 1), 256, 0, st>>>(n, ld, R, b.solo ? 0 : me, cnt, xcnt);
    if (!b.directed && lrows > 0) { /* this rank's distinct light reliabilities, its block */
        int32_t* hd = xcnt + (size_t)R * LVL_X_CNT + (size_t)me * LVL_GB * 2;
        SRT_HIPCHK(hipMemsetAsync(b.H, 0xFF, LVL_RT_SLOTS * sizeof(unsigned long long), st));
        /* the workgroup tables in the offsets' buffer (free until the offsets) */
        size_t ntb = (ncnt + 1) * sizeof(int32_t) / (LVL_RT_LDS * sizeof(unsigned long long));
        ntb = ntb < 512 ? ntb : 512;
        ntb = ntb < (size_t)lrows ? ntb : (size_t)lrows;
        const int nt = (int)(ntb > 0 ? ntb : 1);
        unsigned long long* tabs = reinterpret_cast<unsigned long long*>(L->off);
        lvl_rt_hash_stash_kernel<<<nt, 256, 0, st>>>(lrows, ld, LVL_BATCH, b.stash, b.scnt, b.r_rows, b.H, tabs,
                                                     hd);
        lvl_rt_merge_kernel<<<LVL_RT_LDS / 256 * srt_ceil_div(nt, LVL_RT_MC), 256, 0, st>>>(nt, tabs, b.H, hd);
        lvl_rt_compact_kernel<<<1, 1024, 0, st>>>(b.H, b.map, reinterpret_cast<double*>(hd + 2), hd + 1);
    }
    SRT_HIPCHK(hipGetLastError());
    return SRT_OK;
}

/* Step 1, second half: the exchange (one sum all-reduce) and its read-back, in pinned memory; the
 * summed histogram, the failure count and, for the streamed wire, the largest rank's arcs per
 * weight. One GPU: the histogram's read-back alone. */
static int lvl_exchange(lvl_build& b) {
    const hipStream_t st = b.st;
    const int R = b.R;
    const size_t xn = b.xn;
    int rc;
    if ((rc = lvl_pinned(LVL_PIN_X + (R > 1 ? (xn + 1) / 2 + LVL_RT_CAP + 2 * LVL_BATCH + 4 : 4), &b.pin)))
        return rc;
    b.hx = reinterpret_cast<int32_t*>(b.pin + LVL_PIN_X);
    b.ht = b.pin + LVL_PIN_X + (xn + 1) / 2;
    b.hwt = reinterpret_cast<int32_t*>(b.ht + LVL_RT_CAP + 2);
    b.hag = reinterpret_cast<int32_t*>(b.pin + LVL_PIN_AG);
    b.failed = !b.ok;
    if (R > 1) {
        b.hag[3] = b.failed;
        SRT_HIPCHK(hipMemcpyAsync(b.xbuf + 2 * LVL_STRIDE, &b.hag[3], sizeof(int32_t), hipMemcpyHostToDevice, st));
        if ((rc = srt_coll_allreduce_i32(b.comm, b.xbuf, xn, 0, st))) return rc;
        SRT_HIPCHK(hipMemcpyAsync(b.hx, b.xbuf, xn * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    } else {
        SRT_HIPCHK(hipMemcpyAsync(b.pin + LVL_PIN_HIST, b.dhist, sizeof(b.hist), hipMemcpyDeviceToHost, st));
    }
    if ((rc = lvl_wait(st))) return rc;
    if (R == 1) {
        memcpy(b.hist, b.pin + LVL_PIN_HIST, sizeof(b.hist));
        return SRT_OK;
    }
    /* the summed histogram from its limbs, on the host (one read-back) */
    b.failed = b.hx[2 * LVL_STRIDE];
    for (int i = 0; i < LVL_STRIDE; i++)
        b.hist[i] = (unsigned long long)(uint32_t)b.hx[i] + ((unsigned long long)(uint32_t)b.hx[LVL_STRIDE + i] << 20);
    for (int w = 1; w <= LVL_BATCH && !b.dr; ++w) b.wmax[w] = (int32_t)lvl_largest_block(b, w, w);
    return SRT_OK;
}

/* This rank's level budget, from global quantities (the summed histogram, the largest shard's
 * words): the largest L whose predicted time stays under half the FW time; and by memory: the
 * planes (L x n x nw words) within half of what the device has left. */
static int lvl_own_budget(const lvl_build& b) {
    int lmax = lvl_budget(b.hist, (double)b.n, (double)b.max_rows / 32.0, 0.5 * b.fw_ms);
    if (b.plane > 0) {
        const size_t cap = lvl_avail_bytes() / 2 / (b.plane * sizeof(uint32_t));
        if ((size_t)lmax > cap) lmax = (int)cap;
    }
    if (b.R > 1) { /* test hook: this rank's memory stands in for a smaller budget (lcap_r<rank>) */
        char key[32];
        snprintf(key, sizeof(key), "lcap_r%d", b.me);
        const int lc = srt_form_int(key, -1);
        if (lc >= 0 && lc < lmax) lmax = lc;
    }
    return lmax;
}

/* Every allocation of the build up front, softly (b.ok), sized by THIS rank's budget b.lmax: the
 * agreed budget is the ranks' minimum, so the buffers fit it. Then the streamed wire, where that
 * form applies (b.stream_ok): step 2 agrees all three. */
static int lvl_alloc_all(lvl_build& b) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int n = b.n, ld = b.ld, R = b.R;
    const size_t ncnt = b.ncnt, plane = b.plane;
    const int lmax_own = max(b.lmax, 0);
    const int64_t total64 = lvl_arcs_upto(b.hist, lmax_own);
    const int32_t total_own = (int32_t)(total64 < 0x7FFFFFF0ll ? total64 : 0x7FFFFFF0ll);
    SRT_HIPCHK(hipcub::DeviceScan::ExclusiveSum(NULL, b.tmp_bytes, b.cnt, L->off, (int)(ncnt + 1), st));
    b.dnt = (size_t)R * ((size_t)ld + 1) + 1; /* directed, N > 1: the runs' totals */
    if (b.dr) {
        size_t tb2 = 0;
        SRT_HIPCHK(hipcub::DeviceScan::ExclusiveSum(NULL, tb2, b.cnt, L->off, (int)b.dnt, st));
        b.tmp_bytes = max(b.tmp_bytes, tb2);
    }
    const bool need_sort_own = total_own > 0 && !(!b.directed && lmax_own <= LVL_STASH_W && b.hist[0] == 0);
    if (need_sort_own)
        SRT_HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(NULL, b.sb, b.arcsA, b.arcs2, b.arA, b.ar2,
                                                               total_own, ld, b.seg, b.seg + 1, 0, 24, st));
    lvl_arena a2;
    if (total64 <= 0x7FFFFFF0ll && lmax_own >= 2) {
        a2.add(&b.tmp, b.tmp_bytes);
        a2.add(&b.arcsA, ((size_t)total_own + 8) * sizeof(uint32_t));
        a2.add(&b.arA, ((size_t)total_own + 8) * sizeof(double));
        if (need_sort_own) {
            a2.add(&b.arcs2, ((size_t)total_own + 8) * sizeof(uint32_t));
            a2.add(&b.ar2, ((size_t)total_own + 8) * sizeof(double));
            a2.add(&b.seg, ((size_t)ld + 1) * sizeof(int32_t));
            a2.add(&b.stmp, b.sb);
        }
        a2.add(&L->aoff, ((size_t)total_own + 64) * sizeof(uint32_t)); /* + a gather batch's tail */
        a2.add(&L->lev, (size_t)lmax_own * plane * sizeof(uint32_t) + 16);
        a2.add(&b.Rb, plane * sizeof(uint32_t) + 16);
        a2.add(&b.done, (size_t)n * b.nchunk + 16);
    }
    /* the distinct arc reliabilities (packed post pass, n <= 32768) */
    if (total_own > 0 && n <= 32768) {
        a2.add(&L->rix, ((size_t)total_own + 8) * sizeof(uint16_t));
        a2.add(&L->rtab, LVL_RT_CAP * sizeof(double));
    }
    /* N > 1: the segments' reliability blocks (lvl_bcast_segments), the counts' all-gather blocks
     * (u16, every weight up to the budget), and the streamed wire's offsets at the shard starts */
    if (total_own > 0 && n <= 32768 && R > 1 && !b.dr) a2.add(&b.gat, (size_t)R * LVL_GB * sizeof(double));
    if (R > 1 && !b.dr) {
        a2.add(&b.cg, ((size_t)R * b.max_rows * max(lmax_own, 1) + 8) * sizeof(uint16_t));
        a2.add(&b.packed, (size_t)4 * LVL_BATCH * 65 * sizeof(int32_t));
    }
    /* directed, N > 1: every rank's (target, weight <= budget) counts, the runs' totals and their
     * scan, the fill's cursors, and the gathered blocks of arcs (12 B per arc, every rank's block
     * padded to the largest; the ranks' arcs per weight are in the exchange) */
    if (b.dr) {
        a2.add(&b.cg, ((size_t)R * ld * max(lmax_own, 1) + 8) * sizeof(uint16_t));
        a2.add(&b.tq, b.dnt * sizeof(int32_t));
        a2.add(&b.oq, b.dnt * sizeof(int32_t));
        a2.add(&b.dcur, (ncnt + 1) * sizeof(int32_t));
        a2.add(&b.dwire, (size_t)R * lvl_dblock(b, lmax_own) * 12 + 16);
    }
    lvl_commit(b, a2, &b.ok);
    /* the streamed first extraction's wire (lvl_extract_streamed): every rank's block of a weight
     * padded to the largest; needs the union table (fit) and at most 2 GB */
    b.lx_own = min(lmax_own, LVL_BATCH);
    size_t wire_words = 0;
    for (int w = 1; w <= b.lx_own && R > 1; ++w) wire_words += (size_t)R * b.wmax[w];
    b.stream_ok = R > 1 && !b.directed && b.hist[0] == 0 && b.fit && n <= 32768 && b.lx_own >= 1 &&
                  b.fpkw != 0 && (double)wire_words * 4.0 < 2e9;
    if (b.stream_ok && b.ok) {
        int sok = 1;
        lvl_arena a3;
        a3.add(&b.offw, ((size_t)b.lx_own * ld + 1) * sizeof(int32_t));
        /* (also the [weight][target] counts before their scan) */
        a3.add(&b.wire, max(wire_words + 8, (size_t)b.lx_own * ld + 1) * sizeof(uint32_t));
        lvl_commit(b, a3, &sok);
        b.stream_ok = sok;
    }
    return SRT_OK;
}

/* Step 2: one min all-reduce agrees the budget, the allocation outcome and the wire. What needs
 * no agreed value is done on the side stream while the main stream carries the agreement and the
 * count all-gather (on the main stream it delayed them): the level state's zeroing and, for the
 * streamed extraction, the union table and the wire's per-weight bases, sized by this rank's
 * budget (lx_own >= the agreed lx; the entries of the weights up to lx are the same either way).
 * The main stream waits for it (wev[LVL_PREP]) before the extraction; wasted when a rank falls
 * back. */
static int lvl_agree(lvl_build& b) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int R = b.R;
    int rc;
    if (R > 1 && b.ok && b.Rb && b.done) { /* (not allocated under a budget below 2) */
        if ((rc = lvl_side_stream(&b.wcs, &b.wev))) return rc;
        SRT_HIPCHK(hipEventRecord(b.wev[LVL_PREP], st)); /* the allocations are ordered on st */
        SRT_HIPCHK(hipStreamWaitEvent(b.wcs, b.wev[LVL_PREP], 0));
        b.prepped = true;
    }
    if (R > 1) { /* the agreement goes out first; the side stream's calls are made under it */
        b.hag[0] = b.lmax;
        b.hag[1] = b.ok;
        b.hag[2] = b.stream_ok;
        SRT_HIPCHK(hipMemcpyAsync(b.dagree, b.hag, 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if ((rc = srt_coll_allreduce_i32(b.comm, b.dagree, 3, 1, st))) return rc;
        SRT_HIPCHK(hipMemcpyAsync(b.hag, b.dagree, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (b.prepped) {
        SRT_HIPCHK(hipMemsetAsync(b.Rb, 0, b.plane * sizeof(uint32_t), b.wcs));
        SRT_HIPCHK(hipMemsetAsync(b.done, 0, (size_t)b.n * b.nchunk, b.wcs));
        lvl_init_kernel<<<srt_ceil_div(b.nrows, 256), 256, 0, b.wcs>>>(b.n, b.row0, b.nrows, b.nw, b.Rb);
        SRT_HIPCHK(hipGetLastError());
    }
    if (b.prepped && b.stream_ok && L->lev && L->rtab) {
        SRT_HIPCHK(hipMemsetAsync(L->lev, 0, (size_t)b.lx_own * b.plane * sizeof(uint32_t), b.wcs));
        const int nu = (int)b.u->size();
        memcpy(b.ht, b.u->data(), b.u->size() * sizeof(unsigned long long));
        const int hf[2] = {0, nu};
        memcpy(b.ht + LVL_RT_CAP, hf, sizeof(hf));
        SRT_HIPCHK(hipMemcpyAsync(L->rtab, b.ht, (size_t)nu * sizeof(double), hipMemcpyHostToDevice, b.wcs));
        SRT_HIPCHK(hipMemcpyAsync(b.dflag, b.ht + LVL_RT_CAP, 2 * sizeof(int), hipMemcpyHostToDevice, b.wcs));
        /* the wire: per weight every rank's block padded to the largest rank's arcs: the weight's
         * base and that block size */
        size_t base = 0;
        for (int w = 1; w <= b.lx_own; ++w) {
            b.hwt[2 * (w - 1)] = (int32_t)base;
            b.hwt[2 * (w - 1) + 1] = b.wmax[w];
            base += (size_t)R * b.wmax[w];
        }
        SRT_HIPCHK(hipMemcpyAsync(b.packed + LVL_BATCH * 65, b.hwt, 2 * (size_t)b.lx_own * sizeof(int32_t),
                                  hipMemcpyHostToDevice, b.wcs));
    }
    if (b.prepped) SRT_HIPCHK(hipEventRecord(b.wev[LVL_PREP], b.wcs));
    if (R > 1) {
        if ((rc = lvl_wait(st))) return rc;
        b.lmax = b.hag[0];
        b.ok = b.hag[1];
        b.stream_ok = b.hag[2];
    }
    return SRT_OK;
}

/* Step 3, directed: every rank's contribution to every target's counts of the weights w0..w1, one
 * all-gather of u16 blocks [weight][target]: summed into cnt, and kept per rank (dcn) for the
 * placement */
static int lvl_share_counts_directed(lvl_build& b, int w0, int w1) {
    const hipStream_t st = b.st;
    const int ld = b.ld, R = b.R;
    const size_t dblk = (size_t)ld * (w1 - w0 + 1);
    uint16_t* reg = b.cg + (size_t)R * ld * (w0 - 1); /* weights 1..lx, then lx + 1..lmax */
    lvl_dcnt_pack_kernel<<<srt_ceil_div(ld, 256), 256, 0, st>>>(ld, w0, w1, b.cnt, reg + (size_t)b.me * dblk);
    SRT_HIPCHK(hipGetLastError());
    int rc = srt_coll_allgather(b.comm, reg, dblk * sizeof(uint16_t), st);
    if (rc) return rc;
    lvl_dcnt_sum_kernel<<<srt_ceil_div(ld, 256), 256, 0, st>>>(ld, R, w0, w1, reg, b.cnt);
    SRT_HIPCHK(hipGetLastError());
    if (w0 == 1) b.dcn = lvl_dcnt{reg, NULL, w1, w1, ld};
    else b.dcn.b = reg, b.dcn.wb = w1;
    return SRT_OK;
}

/* Step 3, undirected: every target's counts of the weights w0..w1 on every rank, one all-gather of
 * the ranks' u16 blocks (a solo rank has them: synthesised) */
static int lvl_share_counts_rows(lvl_build& b, int w0, int w1) {
    const hipStream_t st = b.st;
    const size_t blk = (size_t)b.max_rows * (w1 - w0 + 1);
    if (b.nrows > 0)
        lvl_cnt_gpack_kernel<<<srt_ceil_div(b.nrows, 256), 256, 0, st>>>(b.row0, b.nrows, b.max_rows, w0, w1, b.me,
                                                                       b.cnt, b.cg);
    SRT_HIPCHK(hipGetLastError());
    int rc = srt_coll_allgather(b.comm, b.cg, blk * sizeof(uint16_t), st);
    if (rc) return rc;
    if (!b.solo)
        lvl_cnt_gunpack_kernel<<<srt_ceil_div(b.ld, 256), 256, 0, st>>>(b.ld, b.R, b.max_rows, w0, w1, b.cg, b.cnt);
    SRT_HIPCHK(hipGetLastError());
    return SRT_OK;
}

static int lvl_share_counts(lvl_build& b, int w0, int w1) {
    if (b.R == 1 || w1 < w0) return SRT_OK;
    return b.dr ? lvl_share_counts_directed(b, w0, w1) : lvl_share_counts_rows(b, w0, w1);
}

/* Step 4: offsets of the (target, weight <= lw) in-arcs: narrow scan, counts untouched. ow, osz
 * (the streamed form): the wire's offsets and their values at the shard starts. */
static int lvl_offsets(lvl_build& b, int lw, int32_t* ow = NULL, int32_t* osz = NULL) {
    const hipStream_t st = b.st;
    const int ld = b.ld;
    int32_t* const off = b.L->off;
    if (lw <= LVL_BATCH) { /* a first extraction: two launches (with the wire's offsets) */
        const int nb = (ld + 1 + 255) / 256; /* (the thread of target ld writes the totals) */
        lvl_off_part_kernel<<<nb, 256, 0, st>>>(ld, lw, b.cnt, b.tb);
        lvl_offsets_kernel<<<nb, 256, 0, st>>>(ld, lw, b.R, b.cnt, b.tb, off, ow, osz);
        SRT_HIPCHK(hipGetLastError());
        return SRT_OK;
    }
    lvl_tot_kernel<<<srt_ceil_div(ld + 1, 256), 256, 0, st>>>(ld, lw, b.cnt, b.tb);
    SRT_HIPCHK(hipGetLastError());
    SRT_HIPCHK(hipcub::DeviceScan::ExclusiveSum(b.tmp, b.tmp_bytes, b.tb, b.tb + ld + 1, ld + 1, st));
    lvl_off_kernel<<<srt_ceil_div(ld + 1, 256), 256, 0, st>>>(ld, lw, b.cnt, b.tb + ld + 1, off);
    SRT_HIPCHK(hipGetLastError());
    return SRT_OK;
}

/* Step 4, directed, N > 1: this rank's arcs of weight <= lw into its block (12 B per arc), the
 * blocks all-gathered once, then placed (lvl_dplace_kernel) */
static int lvl_fill_directed_ranks(lvl_build& b, int lw) {
    const hipStream_t st = b.st;
    const int n = b.n, ld = b.ld, R = b.R;
    const size_t blk = lvl_dblock(b, lw) * 12; /* (from the exchange: alike on every rank) */
    lvl_dtot_kernel<<<(unsigned)((b.dnt + 255) / 256), 256, 0, st>>>(R, lw, b.dcn, b.tq);
    SRT_HIPCHK(hipGetLastError());
    SRT_HIPCHK(hipcub::DeviceScan::ExclusiveSum(b.tmp, b.tmp_bytes, b.tq, b.oq, (int)b.dnt, st));
    lvl_dcur_kernel<<<srt_ceil_div(ld, 256), 256, 0, st>>>(b.me, lw, b.dcn, b.oq, b.dcur);
    char* mine = b.dwire + (size_t)b.me * blk;
    if (b.lrows > 0)
        lvl_arcs_colwin_kernel<true><<<dim3(ld / 64, srt_ceil_div(b.lrows, LVL_DROWS)), 256, 0, st>>>(
            n, ld, b.row0, b.lrows, b.w_rows, b.dcur, lw, reinterpret_cast<uint32_t*>(mine), b.r_rows,
            reinterpret_cast<double*>(mine + blk / 3));
    SRT_HIPCHK(hipGetLastError());
    int rc = srt_coll_allgather(b.comm, b.dwire, blk, st);
    if (rc) return rc;
    lvl_dplace_kernel<<<srt_ceil_div(n, 4), 256, 0, st>>>(n, ld, R, blk, b.L->off, b.tq, b.oq, b.dwire, b.arcsA,
                                                         b.arA);
    SRT_HIPCHK(hipGetLastError());
    return SRT_OK;
}

/* Step 4, every other form: this rank's arcs of weight <= lw into (target, weight)-major order,
 * from the columns (directed, one GPU) or from its rows (undirected: its rows' segment) */
static int lvl_fill_own(lvl_build& b, int lw) {
    const hipStream_t st = b.st;
    if (b.directed)
        lvl_arcs_cols_kernel<true><<<b.ld / 64, 256, 0, st>>>(b.n, b.ld, b.w_rows, NULL, lw, b.L->off, b.arcsA,
                                                              b.r_rows, b.arA);
    else
        lvl_arcs_rows_kernel<true><<<b.nrows, 256, 0, st>>>(b.n, b.ld, b.row0, b.w_rows, NULL, lw, b.L->off,
                                                            b.arcsA, b.r_rows, b.arA, NULL, b.stash, b.scnt);
    SRT_HIPCHK(hipGetLastError());
    return SRT_OK;
}

/* Step 4, undirected N > 1, the broadcast form: every rank filled its rows' segment; one
 * broadcast group sends the segments. *numbered: they travelled as arcs + table indices.
 * Numbered segments: the packed post pass needs each arc's index into the table of distinct
 * reliabilities, not its f64. Each rank numbers its own segment's values (hash + compact), the
 * blocks are all-gathered (16 KB per rank), every rank takes the union sorted by value bits -- the
 * same table everywhere -- and the segments travel as arcs + u16 indices: 6 B per arc instead of
 * 12. Taken when the post pass will be the packed one (levels <= lw <= 31, pkw) and the fill needs
 * no sort (the sort carries the f64s); more than LVL_RT_CAP values in the union (or a probe
 * overflow) keeps the f64 segments, on every rank alike. */
static int lvl_bcast_segments(lvl_build& b, int lw, int sorted_w, int* numbered) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int R = b.R, ld = b.ld;
    int rc;
    int32_t hoff[65];
    for (int q = 0; q <= R; q++) {
        int32_t s = ld, e = ld;
        if (q < R) srt_shard_rows(ld, SRT_SHARD_ALIGN, R, q, &s, &e);
        SRT_HIPCHK(hipMemcpyAsync(&hoff[q], L->off + (size_t)s * LVL_STRIDE, sizeof(int32_t),
                                  hipMemcpyDeviceToHost, st));
    }
    if ((rc = lvl_wait(st))) return rc;
    const int nb0 = hoff[b.me], nb1 = hoff[b.me + 1]; /* the arcs this process numbers: its segment */
    if (b.gat && sorted_w && lw <= 31 && b.fpkw != 0) {
        double* const mine = b.gat + b.me * LVL_GB;
        SRT_HIPCHK(hipMemsetAsync(b.gat, 0, (size_t)R * LVL_GB * sizeof(double), st));
        if (nb1 > nb0) {
            SRT_HIPCHK(hipMemsetAsync(b.dflag, 0, 2 * sizeof(int), st));
            SRT_HIPCHK(hipMemsetAsync(b.H, 0xFF, LVL_RT_SLOTS * sizeof(unsigned long long), st));
            lvl_rt_hash_kernel<<<lvl_rt_grid(nb1 - nb0), 256, 0, st>>>(NULL, NULL, nb0, nb1, b.arA, b.H, L->rix,
                                                                      b.dflag);
            lvl_rt_compact_kernel<<<1, 1024, 0, st>>>(b.H, b.map, mine + 1, b.dflag + 1);
            SRT_HIPCHK(hipGetLastError());
            SRT_HIPCHK(hipMemcpyAsync(mine, b.dflag, 2 * sizeof(int), hipMemcpyDeviceToDevice, st));
        }
        if ((rc = srt_coll_allgather(b.comm, b.gat, LVL_GB * sizeof(double), st))) return rc;
        std::vector<unsigned long long> hg((size_t)R * LVL_GB);
        SRT_HIPCHK(hipMemcpyAsync(hg.data(), b.gat, hg.size() * sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, st));
        if ((rc = lvl_wait(st))) return rc;
        std::vector<unsigned long long>& u = *b.u;
        if (lvl_union(hg.data(), R, -1, u)) {
            const int nu = (int)u.size(), hf[2] = {0, nu};
            SRT_HIPCHK(hipMemcpyAsync(L->rtab, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice, st));
            SRT_HIPCHK(hipMemcpyAsync(b.dflag, hf, sizeof(hf), hipMemcpyHostToDevice, st));
            if (nb1 > nb0)
                lvl_rt_index_kernel<<<srt_ceil_div(nb1 - nb0, 256), 256, 0, st>>>(
                    nb1 - nb0, b.arA + nb0, reinterpret_cast<const unsigned long long*>(L->rtab), nu,
                    L->rix + nb0);
            SRT_HIPCHK(hipGetLastError());
            if ((rc = lvl_wait(st))) return rc; /* hf leaves scope, u may be rewritten */
            *numbered = 1;
        }
    }
    rc = srt_coll_group_begin(b.comm);
    for (int q = 0; q < R && !rc; q++)
        if (hoff[q + 1] > hoff[q]) {
            const size_t c = (size_t)(hoff[q + 1] - hoff[q]);
            rc = srt_coll_bcast(b.comm, b.arcsA + hoff[q], c * sizeof(uint32_t), q, st);
            if (!rc)
                rc = *numbered ? srt_coll_bcast(b.comm, L->rix + hoff[q], c * sizeof(uint16_t), q, st)
                               : srt_coll_bcast(b.comm, b.arA + hoff[q], c * sizeof(double), q, st);
        }
    const int rc2 = srt_coll_group_end(b.comm);
    if (rc || rc2) return rc ? rc : rc2;
    if (b.solo && b.lrows > 0) {
        lvl_solo_arcs_kernel<<<srt_ceil_div(b.n, 4), 256, 0, st>>>(b.n, b.row0, b.nrows, b.lrows, 1, lw, b.nw,
                                                                 L->off, b.arcsA, *numbered ? L->rix : NULL,
                                                                 *numbered ? NULL : b.arA, NULL);
        SRT_HIPCHK(hipGetLastError());
    }
    return SRT_OK;
}

/* Step 4, the broadcast form (and every one-GPU build): the in-arcs of weight <= lw, from arcsA /
 * arA again (not from an earlier sort's output), into L->arcs / ar with their plane offsets and
 * the reliability table */
static int lvl_extract(lvl_build& b, int lw) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int ld = b.ld;
    int numbered = 0, rc;
    L->total = (int32_t)lvl_arcs_upto(b.hist, lw);
    const int sorted_w = !b.directed && lw <= LVL_STASH_W && b.hist[0] == 0; /* global values */
    if ((rc = lvl_offsets(b, lw))) return rc; /* (target, weight <= lw)-major */
    if (b.dr) {
        if ((rc = lvl_fill_directed_ranks(b, lw))) return rc;
    } else {
        if ((rc = lvl_fill_own(b, lw))) return rc;
        if (b.R > 1 && (rc = lvl_bcast_segments(b, lw, sorted_w, &numbered))) return rc;
    }
    /* in-arcs of each target sorted by (weight, source vertex): the order the predecessor search
     * walks them in (the full-row fill's atomics leave the order inside a weight arbitrary; the
     * ordered stash fill needs no sort) */
    L->arcs = b.arcsA;
    L->ar = b.arA;
    if (L->total > 0 && !sorted_w) {
        lvl_segs_kernel<<<srt_ceil_div(ld + 1, 256), 256, 0, st>>>(ld, L->off, b.seg);
        SRT_HIPCHK(hipGetLastError());
        SRT_HIPCHK(hipcub::DeviceSegmentedRadixSort::SortPairs(b.stmp, b.sb, b.arcsA, b.arcs2, b.arA, b.ar2,
                                                               L->total, ld, b.seg, b.seg + 1, 0, 24, st));
        L->arcs = b.arcs2;
        L->ar = b.ar2;
    }
    if (L->total > 0) {
        lvl_aoff_kernel<<<srt_ceil_div(L->total, 256), 256, 0, st>>>(L->total, b.nw, L->arcs, L->aoff);
        SRT_HIPCHK(hipGetLastError());
    }
    /* the reliability table: its flags are read with the levels' completion (no round trip) */
    if (b.want_rt && L->total > 0 && !numbered) {
        SRT_HIPCHK(hipMemsetAsync(b.dflag, 0, 2 * sizeof(int), st));
        SRT_HIPCHK(hipMemsetAsync(b.H, 0xFF, LVL_RT_SLOTS * sizeof(unsigned long long), st));
        lvl_rt_hash_kernel<<<lvl_rt_grid(L->total), 256, 0, st>>>(NULL, NULL, 0, L->total, L->ar, b.H, L->rix,
                                                                 b.dflag);
        lvl_rt_compact_kernel<<<1, 1024, 0, st>>>(b.H, b.map, L->rtab, b.dflag + 1);
        lvl_rt_remap_kernel<<<srt_ceil_div(L->total, 256), 256, 0, st>>>(L->total, b.map, L->rix);
        SRT_HIPCHK(hipGetLastError());
    }
    return SRT_OK;
}

/* Step 4, undirected N > 1, the streamed form of the first extraction: the arcs of weight <= lw
 * travel weight by weight on the side stream (lvl_stream_weight, lvl_place_weight); level d then
 * waits for wev[d - 1] only. Taken when the fill is the ordered stash and the reliabilities can be
 * numbered from the exchange (stream_ok); otherwise lvl_extract. No host round trip: the union
 * table and the wire's per-weight bases are on the device since the agreement. */
static int lvl_extract_streamed(lvl_build& b, int lw) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int n = b.n, ld = b.ld, row0 = b.row0, nrows = b.nrows, lrows = b.lrows, nw = b.nw;
    int rc;
    L->total = (int32_t)lvl_arcs_upto(b.hist, lw);
    /* offsets over the arcs with w <= lw, (target, weight)-major, and the wire's: offw, the
     * [weight][target] scan of every target's counts (gathered), dsz its values at the shard
     * starts */
    int32_t* const dsz = b.packed;
    const int32_t* dwt = b.packed + LVL_BATCH * 65;
    if ((rc = lvl_offsets(b, lw, b.offw, dsz))) return rc;
    lvl_arcs_rows_kernel<true><<<nrows, 256, 0, st>>>(n, ld, row0, b.w_rows, NULL, lw, L->off, b.arcsA, b.r_rows,
                                                      b.arA, NULL, b.stash, b.scnt);
    const int32_t* lo = L->off + (size_t)row0 * LVL_STRIDE;
    const int32_t* hi = L->off + (size_t)(row0 + nrows) * LVL_STRIDE;
    /* each own arc's row offset and its index into the union table */
    lvl_own_index_kernel<<<512, 256, 0, st>>>(lo, hi, nw, b.arcsA, b.arA,
                                              reinterpret_cast<const unsigned long long*>(L->rtab),
                                              (int)b.u->size(), L->aoff, L->rix);
    if (lrows > 0)
        lvl_wire_pack_kernel<<<srt_ceil_div(lrows, 4), 256, 0, st>>>(ld, row0, lrows, lw, b.R, b.me, L->off, b.offw,
                                                                    dsz, dwt, b.arcsA, L->rix, b.arA, b.wire, NULL);
    SRT_HIPCHK(hipGetLastError());
    SRT_HIPCHK(hipEventRecord(b.wev[0], st));
    SRT_HIPCHK(hipStreamWaitEvent(b.wcs, b.wev[0], 0));
    /* while weight 1 travels: the own sources' arcs into their planes (zeroed since the
     * agreement) */
    if (b.solo && lrows > 0)
        lvl_solo_direct_kernel<<<srt_ceil_div(n, 4), 256, 0, st>>>(n, row0, nrows, lrows, nw, lw, b.plane, L->off,
                                                                   b.arcsA, L->lev, b.Rb);
    else if (!b.solo && lrows > 0)
        lvl_direct_kernel<<<srt_ceil_div(lrows, 4), 256, 0, st>>>(row0, row0 + lrows, nw, lw, b.plane, L->off,
                                                                 b.arcsA, L->lev, b.Rb);
    SRT_HIPCHK(hipGetLastError());
    b.wnum = 1;
    L->arcs = b.arcsA;
    L->ar = b.arA;
    b.streamed = lw;
    return SRT_OK;
}

/* Step 4, weight w of the streamed extraction on the side stream: the all-gather of the blocks.
 * Enqueued just before level w, so the host's calls for weight w + 1 overlap the levels on the
 * GPU. */
static int lvl_stream_weight(lvl_build& b, int w) {
    const size_t base = (size_t)b.hwt[2 * (w - 1)], mx = (size_t)b.hwt[2 * (w - 1) + 1];
    int rc = srt_coll_allgather(b.comm, b.wire + base, mx * sizeof(uint32_t), b.wcs);
    if (rc) return rc;
    SRT_HIPCHK(hipEventRecord(b.wev[w], b.wcs));
    return SRT_OK;
}

/* Step 4, weight w's placement (the solo rank synthesises its peers' arcs instead), on the main
 * stream between two levels: the all-gather finished under the previous level, and the whole GPU
 * places the arcs in ~12 us. On the side stream the placement got only the CUs the persistent
 * level grid left free and ended with the level it ran beside (72-135 us per weight on one rank
 * of N = 8), and the last weight's all-gather queued behind it. */
static int lvl_place_weight(lvl_build& b, int w) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int32_t* dsz = b.packed;
    const int32_t* dwt = b.packed + LVL_BATCH * 65;
    SRT_HIPCHK(hipStreamWaitEvent(st, b.wev[w], 0));
    if (b.solo && b.lrows > 0)
        lvl_solo_arcs_kernel<<<srt_ceil_div(b.n, 4), 256, 0, st>>>(b.n, b.row0, b.nrows, b.lrows, w, w, b.nw, L->off,
                                                                 L->arcs, b.wnum ? L->rix : NULL,
                                                                 b.wnum ? NULL : L->ar, L->aoff);
    else if (!b.solo)
        lvl_wire_unpack_kernel<<<srt_ceil_div(b.n, 4), 256, 0, st>>>(b.n, b.ld, b.row0, b.nrows, w, b.nw, b.R, L->off,
                                                                   b.offw, dsz, dwt, b.wire, NULL, L->arcs, L->rix,
                                                                   L->ar, L->aoff);
    SRT_HIPCHK(hipGetLastError());
    return SRT_OK;
}

/* Step 5, level d of a batch ending at d1 on the main stream, between two kernel-time events:
 * first the streamed weights it is due (sent one ahead) and needs (placed) */
static int lvl_level(lvl_build& b, int d, int d1, unsigned pgrid) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    evpool_t* const evp = b.evp;
    const int n = b.n, nw = b.nw;
    int rc;
    /* weights go out one ahead of the levels (every rank alike: a settled rank still sends its
     * arcs), but not past the batch they are for: a weight nobody's level needs is never sent (C4
     * ends at level 5) */
    while (b.wq < min(b.streamed, min(d + 1, d1)))
        if ((rc = lvl_stream_weight(b, ++b.wq))) return rc;
    if (L->D && d > L->D) return SRT_OK; /* this rank's sources are settled: nothing to run */
    /* Level d reads the arcs of weight < d only: an arc of weight d counts for its own source
     * alone (Delta_0), and lvl_direct_kernel put those into the planes from this rank's rows. So
     * level d waits for weight d - 1, and level 1 for nothing. */
    while (b.wp < min(d - 1, b.wq))
        if ((rc = lvl_place_weight(b, ++b.wp))) return rc;
    if (evp) SRT_HIPCHK(hipEventRecord(evp->ev[evp->used++], st));
    if (d == 1) { /* the weight-1 arcs as bits; level 2 takes up the completion flags (dinc[1]
                   * stays set: a graph settled at level 1 reports 2 levels). Streamed:
                   * lvl_direct_kernel has set them. */
        SRT_HIPCHK(hipMemsetAsync(b.dinc + 1, 0xFF, sizeof(int), st));
        if (!b.streamed) {
            SRT_HIPCHK(hipMemsetAsync(L->lev, 0, b.plane * sizeof(uint32_t), st));
            lvl_first_kernel<<<srt_ceil_div(n, 4), 256, 0, st>>>(n, nw, b.row0, b.nrows, L->off, L->arcs, L->lev,
                                                                  b.Rb);
        }
    } else {
        /* levels 2 and 3: the weight-d and weight-(d - 1) groups from the in-arc runs
         * (lvl_near_kernel); later levels stop after their first group almost everywhere (the
         * early exit), so they keep the gathers. The runs are read whole for every target
         * whatever a rank's share of the sources, so they pay only for a wide share (C4: 14.5 ->
         * 14.1 ms on one GPU; a rank of N = 8, 128 words, went 2.55 -> 2.86 ms) */
        const bool near = d <= 3 && d <= b.lx && nw >= LVL_NEAR_MIN_NW && nw <= LVL_NEAR_NW;
        unsigned long long* nset = reinterpret_cast<unsigned long long*>(b.dagree + 4);
        if (near)
            lvl_near_kernel<<<srt_ceil_div(n, 4), 256, 4 * (size_t)nw * sizeof(uint32_t), st>>>(
                d, n, nw, b.row0, b.nrows, d <= b.streamed, L->off, L->arcs, L->lev);
        lvl_step_kernel<<<pgrid, 256, 0, st>>>(d, near ? 2 : d <= b.streamed, n, nw, b.nchunk, b.row0, b.nrows,
                                              L->nblk, L->off, L->arcs, L->aoff, L->lev, b.Rb, b.done,
                                              b.dinc + d, b.dinc + d - 1, nset, nset + 1);
    }
    if (evp) SRT_HIPCHK(hipEventRecord(evp->ev[evp->used++], st));
    return SRT_OK;
}

/* Step 5, the end of the batch d0..d1: its weights in place, the vote (N > 1, one sum
 * all-reduce) and the one read-back. Sets L->D (this rank's last level), b.all_done (the verdict)
 * and *settled (the pairs settled at levels >= 2: over all ranks from the vote). */
static int lvl_batch_end(lvl_build& b, int d0, int d1, unsigned long long* settled) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    int rc;
    /* the batch's weights in place before anything after its levels (the post pass reads every
     * arc up to the last level) */
    while (b.wp < b.wq)
        if ((rc = lvl_place_weight(b, ++b.wp))) return rc;
    if (b.R > 1) {
        lvl_vote_kernel<<<1, 64, 0, st>>>(b.dinc + d1, reinterpret_cast<unsigned long long*>(b.dagree + 4), b.dvote);
        SRT_HIPCHK(hipGetLastError());
        if ((rc = srt_coll_allreduce_i32(b.comm, b.dvote, 4, 0, st))) return rc;
    }
    /* one read-back: the completion flags, the table flags, the settled pairs, the gathered bytes
     * and the vote are neighbours in the host-side words (four copies cost ~20 us each of round
     * trip) */
    unsigned long long* const hw = b.pin + LVL_PIN_HW;
    SRT_HIPCHK(hipMemcpyAsync(hw, b.dhist + LVL_H_INC, (LVL_H_WORDS - LVL_H_INC) * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, st));
    if ((rc = lvl_wait(st))) return rc;
    const int* hinc = reinterpret_cast<const int*>(hw);
    const int32_t* vote = reinterpret_cast<const int32_t*>(hw + (LVL_H_VOTE - LVL_H_INC));
    b.hflag[0] = hinc[LVL_WMAX + 1];
    b.hflag[1] = hinc[LVL_WMAX + 2];
    for (int d = d0; d <= d1 && !L->D; ++d)
        if (hinc[d] == 0) L->D = d;
    if (b.R > 1) {
        b.all_done = vote[0] == 0;
        *settled = (unsigned long long)(uint32_t)vote[1] + ((unsigned long long)(uint32_t)vote[2] << 21) +
                   ((unsigned long long)(uint32_t)vote[3] << 42);
    } else {
        b.all_done = L->D != 0;
        *settled = hw[LVL_H_AGREE + 2 - LVL_H_INC];
    }
    return SRT_OK;
}

/* Step 5: the levels in batches, one host round trip per batch. After the first batch the settled
 * fraction decides whether the rest is worth it: a graph with far-apart vertices (metric
 * latencies, C4metric: 0.2% settled after 8 levels, distances of hundreds of quanta) goes to the
 * FW at once instead of spending its whole budget first (77 ms there). At N > 1 the decision is
 * taken from the summed vote (lvl_vote_kernel): the fraction of all n^2 pairs, the same number on
 * every rank and the one a single GPU would see. A rank whose own sources settled early runs the
 * later levels as no-ops (lvl_step_kernel's prev test) and keeps its D. */
static int lvl_levels(lvl_build& b) {
    lvl_state* const L = b.L;
    evpool_t* const evp = b.evp;
    const int lmax = b.lmax, lx = b.lx;
    int rc;
    L->nblk = ((unsigned)(((b.n + 3) / 4) * b.nchunk) + 7u) & ~7u;
    /* while the streamed arcs are still arriving, one CU per XCD stays free for the broadcast
     * (RCCL's kernels, the unpack) beside the persistent level grid */
    const unsigned pgrid = lvl_grid((const void*)lvl_step_kernel, L->nblk, b.streamed ? 8 : 0);
    const int ev0 = evp ? evp->used : 0;
    if (evp && (rc = evpool_reserve(evp, ev0 + 2 * lmax))) return rc;
    for (int d0 = 1, d1 = 0; d0 <= lmax; d0 = d1 + 1) {
        /* batches: levels 1-5 (C4's distances end at 4-5), then one level at a time up to
         * LVL_BATCH (a level nobody needs is never launched, nor its weight waited for), then
         * LVL_BATCH at a time */
        d1 = d0 == 1 ? min(lmax, LVL_B1) : d0 <= LVL_BATCH ? d0 : min(lmax, d0 + LVL_BATCH - 1);
        for (int d = d0; d <= d1; ++d)
            if ((rc = lvl_level(b, d, d1, pgrid))) return rc;
        SRT_HIPCHK(hipGetLastError());
        unsigned long long settled = 0;
        if ((rc = lvl_batch_end(b, d0, d1, &settled))) return rc;
        if (b.all_done) break;
        /* settled pairs of all sources: the levels >= 2 counted by lvl_step_kernel, every source's
         * own vertex (level 0) and the weight-1 arcs (level 1, lvl_first_kernel counts none) */
        const double frac = ((double)settled + (double)b.n + (double)b.hist[1]) / ((double)b.n * (double)b.n);
        /* at the end of the first LVL_BATCH levels (a forced level build, fw_ms = 1e30 from
         * SRT_FORM levels=1, runs its whole budget) */
        if (d1 == lx && d1 < lmax && frac < LVL_MIN_SETTLED && b.fw_ms < 1e29)
            break; /* -> Floyd-Warshall, every rank */
        if (d1 == lx && lx < lmax) { /* the heavier arcs: their counts, then every arc up to lmax */
            while (b.wq < b.streamed) /* (the first extraction's last weights, for the collectives) */
                if ((rc = lvl_stream_weight(b, ++b.wq))) return rc;
            while (b.wp < b.wq) /* its writes come first */
                if ((rc = lvl_place_weight(b, ++b.wp))) return rc;
            if ((rc = lvl_share_counts(b, lx + 1, lmax)) || (rc = lvl_extract(b, lmax))) return rc;
        }
    }
    /* the side stream's last weight before anything frees the wire (lvl_free waits for it too) */
    if (b.wq) L->wlast = b.wev[b.wq];
    if (evp && L->D) evp->used = ev0 + 2 * L->D; /* the levels that did work */
    /* the bytes the level kernels gathered, counted on the device (the early exit skips the later
     * weight groups of a unit, so the model -- every arc of weight < d for every level -- would
     * overstate them): dhist word 515, in the last batch's read-back */
    b.gathered = (int64_t)(b.pin + LVL_PIN_HW)[LVL_H_AGREE + 3 - LVL_H_INC];
    return SRT_OK;
}

/* The choice of the post pass and the hand-over: the build is held for srt_levels_pred.
 * Source-major packed words (SRT_FORM pkw=1, the default; 3, 4: the same with srt_levels_pred's
 * units forced to one sub-chunk, to whole chunks) where the arcs are numbered, at most 31 levels
 * and u16 vertices: lvl_pred_rows_kernel's words with the level, then rel_pk_kernel, which writes
 * the u32 rows too. pkw=2: lvl_pred_kernel's target-major words and one transpose before
 * rel_pk_kernel. Past the packed form, or pkw=0: lvl_out8 rows + the predecessor rows +
 * rel_tree_kernel. */
static int lvl_hand_over(lvl_build& b, int* levels, int64_t* gather_bytes) {
    lvl_state* const L = b.L;
    const hipStream_t st = b.st;
    const int D = L->D;
    if (b.want_rt && !b.hflag[0] && b.hflag[1] <= LVL_RT_CAP)
        L->ntab = b.hflag[1];
    else
        L->rix = NULL, L->rtab = NULL; /* (freed with the state) */
    L->post = !L->rix || D > 31 || b.n > 32768 || b.fpkw == 0 ? SRT_LVL_POST_U8
              : b.fpkw == 2                                    ? SRT_LVL_POST_PK_COLS
                                                               : SRT_LVL_POST_PK_ROWS;
    if (L->post == SRT_LVL_POST_PK_ROWS && L->total > 0) { /* 4 B per held arc (34 MB on C4) */
        LVL_ALLOC(L->apk, (size_t)L->total * sizeof(uint32_t));
        lvl_apk_kernel<<<srt_ceil_div(L->total, 256), 256, 0, st>>>(L->total, L->arcs, L->rix, L->apk);
        SRT_HIPCHK(hipGetLastError());
    }
    if (L->post == SRT_LVL_POST_U8) {
        LVL_ALLOC(L->l8, (size_t)b.nrows * b.ld);
        if (D <= LVL_OUT_L) {
            const int lds = D * 2 * 256 * (int)sizeof(uint4);
            SRT_HIPCHK(hipFuncSetAttribute((const void*)lvl_out8_kernel,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            lvl_out8_kernel<<<dim3(srt_ceil_div(b.ld, 256), srt_ceil_div(b.nw, 8)), 256, lds, st>>>(
                b.n, b.ld, b.nw, b.row0, D, L->lev, b.lat_rows, L->l8);
        } else {
            lvl_out_kernel<<<dim3(srt_ceil_div(b.ld, 1024), srt_ceil_div(b.nw, 16)), 256, 0, st>>>(
                b.n, b.ld, b.nw, b.row0, D, L->lev, b.lat_rows, L->l8);
        }
        SRT_HIPCHK(hipGetLastError());
    }
    L->pn_cap = lvl_pn_cap(b.hist, b.n, b.nrows, D);
    *levels = D;
    *gather_bytes = b.gathered;
    L->held = 1;
    return SRT_OK;
}

/* One build of the local rows' distances (nrows x ld). comm (NULL on one GPU): row
 * shards, every rank sees every target's in-arcs after the segment broadcasts (undirected) or the
 * all-gather of the ranks' blocks (directed). fw_ms: the
 * predicted Floyd-Warshall time (of the largest shard); the level budget keeps the predicted level
 * time under half of it. *levels = the level that settled every pair (0: not applicable / over
 * budget / out of memory -- the caller runs Floyd-Warshall). *gather_bytes: the Delta words
 * gathered (the kernel's algorithmic bytes). On success the slot keeps the arcs and the planes for
 * the post pass until srt_levels_release; lat_rows hold the u32 rows, unless the post pass writes
 * them itself (srt_levels_pkw_ready).
 *
 * The N > 1 protocol. Every branch after the first collective is taken on values every rank holds
 * alike -- the exchanged histogram and blocks, the agreed budget, allocation outcome and wire, and
 * each batch's summed vote -- so every rank makes the same collective calls in the same order and
 * no rank leaves while its peers wait in one. In order (each step's functions cite its number):
 *   1. one sum all-reduce of the exchange (lvl_x_words): the histogram limbs, the allocation-
 *      failure count, every rank's arcs per weight w <= LVL_BATCH, every rank's distinct light
 *      reliabilities (so the union table and the wire's block sizes need no later round trip);
 *   2. one min all-reduce of (budget, allocation outcome, wire allocated) -- each rank allocated
 *      for its own budget, which is at least the agreed one;
 *   3. the (target, weight <= lmax) counts (sum);
 *   4. the first batch's arcs: streamed (lvl_extract_streamed), one all-gather per weight w <= lx
 *      (every rank's block padded to the largest), sent one weight ahead of the levels on the side
 *      stream; or, where that form does not apply, lvl_extract: the reliability blocks' all-gather
 *      and one broadcast group of the segments (lvl_bcast_segments);
 *   5. per batch of levels (1-5, then 6, 7, 8 one at a time, then 8 at a time) the vote
 *      (sum); after the batch ending at lx < lmax, lvl_extract(lmax) as in 4's second form.
 * The vote's "all done" is the verdict. tests/test_dist_gloo.py rehearses this sequence over gloo
 * and tests/test_gpu_protocol.py checks every rank's collective log (srt_comm_log_*) against it.
 *
 * Directed graph, N > 1 (a timing-only communicator keeps the FW, decided before any collective):
 * the same order with its own blocks, never streamed (stream_ok stays 0):
 *   1. the exchange (lvl_xd_words): the limbs of the histogram of this rank's rows' arcs (the sum
 *      is the global histogram), the failure count, and every rank's arcs per weight for all 256
 *      weights -- the block sizes of both extractions, so neither needs a read-back; no
 *      reliability blocks (there is no stash for the columns form);
 *   2. the agreement, as above; every buffer of the path is in the arenas it covers;
 *   3. every rank's (target, weight <= lx) counts: one all-gather of u16 blocks [weight][target]
 *      over all ld targets; their sum is the global count, and the parts stay for the placement;
 *   4. the arcs of weight <= lx: one all-gather of every rank's block (12 B per arc: source |
 *      weight << 16, then the f64 reliabilities; padded to the largest rank's arcs, made even),
 *      lvl_dplace_kernel, the segmented sort, the rank-local reliability table;
 *   5. the votes as above; after the batch ending at lx < lmax, 3 for the weights lx + 1..lmax and
 *      4 for every arc of weight <= lmax.
 * tests/levels_protocol_directed.py restates it and tests/test_gpu_directed_ranks.py checks every
 * rank's log against that. */
int srt_levels_build(const srt_comm* comm, int n, int ld, int row0, int nrows, int directed,
                     const uint32_t* w_rows, const double* r_rows, uint32_t* lat_rows, double fw_ms,
                     hipStream_t st, evpool_t* evp, int* levels, int64_t* gather_bytes) {
    *levels = 0;
    *gather_bytes = 0;
    lvl_state* L = &g_lvl[srt_state_slot()];
    if (L->held) lvl_free(L, st);
    const int R = comm ? srt_comm_size(comm) : 1;
    /* rank-independent applicability: the shards are SRT_SHARD_ALIGN (128) aligned, so nrows %
     * 128 == 0 on every rank once ld % 128 == 0; the 32-bit plane offsets are checked against the
     * largest shard */
    if (n > 65535 || ld % 128 || nrows % 128 || row0 % 128 || R > 64) return SRT_OK;
    /* directed, N > 1: the extraction of the header's "directed graph, N > 1" section; a
     * timing-only communicator has no synthesis for it and keeps the FW (before any collective) */
    if (R > 1 && directed && srt_comm_is_solo(comm)) return SRT_OK;
    int max_rows = nrows;
    for (int q = 0; q < R && R > 1; q++) {
        int32_t s = 0, e = 0;
        srt_shard_rows(ld, SRT_SHARD_ALIGN, R, q, &s, &e);
        max_rows = max(max_rows, e - s);
    }
    if ((size_t)n * (size_t)(max_rows / 32) * 4 > 0xFFFFFFFFull) return SRT_OK; /* 32-bit offsets */
    lvl_build b{};
    b.L = L, b.comm = comm, b.st = st, b.evp = evp;
    b.w_rows = w_rows, b.r_rows = r_rows, b.lat_rows = lat_rows, b.fw_ms = fw_ms;
    b.n = n, b.ld = ld, b.row0 = row0, b.nrows = nrows, b.max_rows = max_rows, b.R = R;
    b.nw = nrows / 32, b.nchunk = (b.nw + 63) / 64, b.plane = (size_t)n * b.nw;
    b.lrows = min(nrows, max(0, n - row0));
    b.ncnt = (size_t)ld * LVL_STRIDE;
    b.directed = directed != 0, b.dr = R > 1 && directed;
    /* a timing-only communicator (srt_comm_init_solo*, tools/solo_rank.py): the rank does a real
     * rank's work on its own rows and synthesises what its peers would send (lvl_solo_*) */
    b.solo = R > 1 && srt_comm_is_solo(comm);
    b.me = R > 1 ? srt_comm_rank(comm) : 0;
    b.dcn.ld = ld;
    b.u = &g_lvl_union[srt_state_slot()];
    b.ok = 1;
    /* SRT_FORM pkw and bcap are read here alone; the post pass takes them from the held state */
    b.fpkw = L->fpkw = srt_form_int("pkw", 1);
    L->fbcap = srt_form_int("bcap", 0);
    L->st = st, L->n = n, L->nw = b.nw, L->nchunk = b.nchunk, L->row0 = row0, L->nrows = nrows;
    L->r_rows = r_rows;
    /* on any early return below the allocations go back (lvl_free), unless the build is held */
    struct guard {
        lvl_state* L;
        hipStream_t st;
        ~guard() {
            if (!L->held) lvl_free(L, st);
        }
    } gd{L, st};
    int rc;
    /* step 1: the counts and the exchange */
    if ((rc = lvl_count_pass(b)) || (rc = lvl_exchange(b))) return rc;
    if (b.failed) return SRT_OK; /* out of device memory somewhere: Floyd-Warshall on every rank */
    /* this rank's plan: the union table, the budget, every buffer; step 2 agrees it */
    b.fit = R > 1 && !b.dr && /* (the directed exchange carries no reliability blocks) */
            lvl_union(reinterpret_cast<const unsigned long long*>(b.hx + LVL_X_LIMBS + (size_t)R * LVL_X_CNT), R,
                      b.solo ? b.me : -1, *b.u);
    b.lmax = lvl_own_budget(b);
    if ((rc = lvl_alloc_all(b)) || (rc = lvl_agree(b))) return rc;
    /* From here every branch reads agreed or global values only: hist is summed over the ranks
     * (hist[0] is the stash-overflow count), the budget, the allocation outcome and the wire are
     * agreed. In-arcs come out of the ordered stash already in (weight, source) order, on every
     * rank, when no row overflowed its stash: no sort. */
    int wmin = 0;
    for (int x = 1; x <= LVL_WMAX && !wmin; ++x)
        if (b.hist[x]) wmin = x;
    if (b.lmax < 2 || !wmin || wmin > b.lmax) return SRT_OK;
    const int64_t total64 = lvl_arcs_upto(b.hist, b.lmax);
    if (total64 > 0x7FFFFFF0ll) return SRT_OK; /* int32 arc offsets (global) */
    if (!b.ok) return SRT_OK; /* out of device memory somewhere: Floyd-Warshall on every rank */
    b.want_rt = total64 > 0 && n <= 32768;
    /* The in-arcs are extracted for the first batch of levels only (w <= lx = min(lmax, LVL_BATCH):
     * levels d <= lx use no heavier arc) and again up to lmax if the levels run past it: C4 ends
     * at level 5, and its ~20-quantum budget would extract, number and (N > 1) send 2.5x the arcs
     * it uses. The counts stay whole (narrow offsets) for the second extraction. */
    b.lx = min(b.lmax, LVL_BATCH);
    if ((rc = lvl_share_counts(b, 1, b.lx))) return rc; /* step 3: the first extraction's weights */
    if (R == 1) { /* (N > 1: zeroed on the side stream since the agreement) */
        SRT_HIPCHK(hipMemsetAsync(b.Rb, 0, b.plane * sizeof(uint32_t), st));
        SRT_HIPCHK(hipMemsetAsync(b.done, 0, (size_t)n * b.nchunk, st));
        lvl_init_kernel<<<srt_ceil_div(nrows, 256), 256, 0, st>>>(n, row0, nrows, b.nw, b.Rb);
        SRT_HIPCHK(hipGetLastError());
    }
    if (b.prepped) SRT_HIPCHK(hipStreamWaitEvent(st, b.wev[LVL_PREP], 0));
    /* step 4, then step 5 */
    if ((rc = b.stream_ok ? lvl_extract_streamed(b, b.lx) : lvl_extract(b, b.lx))) return rc;
    if ((rc = lvl_levels(b))) return rc;
    if (!b.all_done) return SRT_OK; /* the verdict, alike on every rank (the summed vote) */
    return lvl_hand_over(b, levels, gather_bytes);
}

/* the held build's post pass (see lvl_hand_over; SRT_LVL_POST_U8 when none is held) */
srt_lvl_post_form srt_levels_pkw_ready(void) {
    const lvl_state* L = &g_lvl[srt_state_slot()];
    return L->held ? L->post : SRT_LVL_POST_U8;
}

/* lvl_pred_kernel's words of type PT (int32, int16 or the packed u32), target-major */
template <typename PT>
static void lvl_pred_launch(const lvl_state* L, void* predT, double* rT, size_t ldp, unsigned long long* part,
                            uint32_t* bkt, uint32_t* bcnt, int cap, hipStream_t st) {
    lvl_pred_kernel<PT><<<lvl_grid((const void*)lvl_pred_kernel<PT>, L->nblk), 256, 0, st>>>(
        L->n, L->nw, L->nchunk, L->row0, L->nrows, L->D, L->nblk, L->off, L->arcs, L->aoff, L->ar, L->rix,
        L->lev, (PT*)predT, rT, ldp, part, bkt, bcnt, cap);
}

/* Canonical predecessors and their arc reliabilities of the held level build in the layout `out`
 * (srt_device.h): target-major (predT[t][sl], rT[t][sl], row stride ldp), as pred_cols*_kernel
 * leave them for the transposes and the reliability passes, or the packed words source-major,
 * predT the rows pk[local source][target] of stride ldp (lvl_pred_rows_kernel; no tie count).
 * ties != NULL adds the tied pairs. */
int srt_levels_pred(void* predT, srt_lvl_pred_layout out, double* rT, size_t ldp, unsigned long long* ties,
                    int32_t* pn_over, int* pn_cap, hipStream_t st) {
    lvl_state* L = &g_lvl[srt_state_slot()];
    if (!L->held) {
        srt_set_error("levels: no held level build for the predecessor pass");
        return SRT_E_ARG;
    }
    unsigned long long* part = NULL;
    if (ties) {
        SRT_HIPCHK(srt_malloc_async(&part, 1024 * sizeof(unsigned long long), st));
        SRT_HIPCHK(hipMemsetAsync(part, 0, 1024 * sizeof(unsigned long long), st));
    }
    const bool packed = out == SRT_LVL_PRED_PK_COLS || out == SRT_LVL_PRED_PK_ROWS;
    if (out != SRT_LVL_PRED_I32 && L->n > 32768) {
        srt_set_error("levels: int16 predecessors need n <= 32768 (n = %d)", L->n);
        return SRT_E_ARG;
    }
    if (packed && !L->rix) {
        srt_set_error("levels: the packed form needs the reliability table");
        return SRT_E_ARG;
    }
    if (out == SRT_LVL_PRED_PK_ROWS && (ties || L->D > 31 || (!L->apk && L->total > 0))) {
        srt_set_error("levels: the source-major packed words take no tie count, at most 31 levels and "
                      "the build's arc words (pkw 1)");
        return SRT_E_ARG;
    }
    /* The Delta_1 groups from the in-arc runs first (lvl_pred_near_kernel), where the runs pay:
     * a wide share of the sources, as lvl_near_kernel's (the runs are read whole whatever the
     * share), few levels (a plane row is read per level: the first arc batch, D <= 8) and a
     * sparse Delta_1 (the histogram's capacity <= 1,024; past that the plane slices are dense
     * enough to gather). SRT_FORM bcap (the bucket capacity hook of the sparse kernels, which a
     * level build does not otherwise read; the key budget of SRT_FORM is spent; as the build
     * read it): k > 0 takes the pre-pass always, with buckets of min(k, 2,048) entries -- 2,048
     * cannot overflow, a small k makes the tests' overflowing buckets --, k < 0 never. Not with
     * the tie count: a tied pair is seen only by walking the whole group. */
    uint32_t *bkt = NULL, *bcnt = NULL;
    int cap = 0;
    *pn_cap = 0;
    if (L->fbcap > 0)
        cap = min(L->fbcap, 2048);
    else if (L->fbcap == 0 && L->nw >= LVL_NEAR_MIN_NW && L->D <= LVL_BATCH && L->pn_cap <= 1024)
        cap = L->pn_cap;
    if (ties || !pn_over || L->D < 2 || L->nw > LVL_NEAR_NW) cap = 0;
    if (cap) {
        const size_t units = (size_t)L->n * L->nchunk;
        int ok = 1; /* no room for the buckets: the walk as it is (pred_near reports 0) */
        LVL_TRY_ALLOC(bkt, units * cap * sizeof(uint32_t), &ok);
        LVL_TRY_ALLOC(bcnt, units * sizeof(uint32_t), &ok);
        if (!ok) bkt = bcnt = NULL, cap = 0;
    }
    if (cap) {
        const size_t lds = 4 * (size_t)(L->nw + L->nchunk) * sizeof(uint32_t);
        lvl_pred_near_kernel<<<srt_ceil_div(L->n, 4), 256, lds, st>>>(
            L->n, L->nw, L->nchunk, L->row0, L->nrows, L->D, cap, L->off, L->arcs, L->lev, bkt, bcnt, pn_over);
        SRT_HIPCHK(hipGetLastError());
        *pn_cap = cap;
    }
    if (out == SRT_LVL_PRED_PK_ROWS) { /* narrow units: the packed words straight into the rows */
        constexpr int TPW = 4, NWV = 4; /* 16 targets x 512 sources per workgroup of 256 threads */
        const auto kern = lvl_pred_rows_kernel<TPW, NWV, 8>;
        const unsigned ntg = (unsigned)srt_ceil_div(L->n, TPW * NWV);
        const unsigned nsub = (unsigned)srt_ceil_div(L->nw, 64 / TPW);
        /* The sub-chunks a unit walks back to back, of the four of a 2,048-source chunk: the
         * longest run that still leaves LVL_ROWS_MIN_ROUNDS rounds of units to the grid (the
         * units are S times coarser, and a narrow share would pay for them in its last round:
         * C4 on one GPU takes 4 and on N = 2 takes 2, at 18 rounds each; N >= 4 keeps 1).
         * SRT_FORM pkw=3 / 4 (tests, A/B): one sub-chunk / whole chunks at any share. */
        const unsigned full = lvl_grid((const void*)kern, ~0u, 0, NWV * 64);
        unsigned S = L->fpkw == 3 ? 1u : 4u;
        while (L->fpkw != 4 && S > 1 && ntg * ((nsub + S - 1) / S) < LVL_ROWS_MIN_ROUNDS * full) S >>= 1;
        const unsigned nunit = ntg * ((nsub + S - 1) / S);
        kern<<<min(full, nunit), NWV * 64, 0, st>>>(
            L->n, L->nw, L->nchunk, L->row0, L->nrows, L->D, ntg, nunit, (int)S, L->off, L->arcs, L->aoff,
            L->apk, L->lev, (uint32_t*)predT, ldp, bkt, bcnt, cap);
    } else if (out == SRT_LVL_PRED_PK_COLS)
        lvl_pred_launch<uint32_t>(L, predT, rT, ldp, part, bkt, bcnt, cap, st);
    else if (out == SRT_LVL_PRED_I16)
        lvl_pred_launch<int16_t>(L, predT, rT, ldp, part, bkt, bcnt, cap, st);
    else
        lvl_pred_launch<int32_t>(L, predT, rT, ldp, part, bkt, bcnt, cap, st);
    SRT_HIPCHK(hipGetLastError());
    if (ties) {
        lvl_sum_kernel<<<1, 1024, 0, st>>>(part, 1024, ties);
        SRT_HIPCHK(hipGetLastError());
        SRT_HIPCHK(hipFreeAsync(part, st));
    }
    return SRT_OK;
}
