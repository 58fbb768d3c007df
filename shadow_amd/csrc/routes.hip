/*
 * routes.hip -- the routes behind finished distance rows, gfx950: per source s and target t the
 * canonical predecessor, the first hop (the forwarding-table entry) and the hop count.
 *
 * Reference: /root/reference/src/main/routing/topology.c:1322, :1368-1369 (the `path:` field a
 * source run logs for every path it stores), :1770-1773 (the log line).
 *
 * The pass is independent of the build that made the rows: it reads u32 distance rows (quanta)
 * and an in-arc CSR, nothing else. The rule is the one every build applies (SURVEY §8a-4,
 * path_sweeps_kernel<HAS_PRED = false> in tables.hip): pred(s, t) = argmin (D[s][u], u) over the
 * tight in-arcs u -> t, D[s][u] + w(u, t) == D[s][t], with D[s][s] taken as 0 (the tables'
 * diagonal holds the path-to-self rule, not 0).
 *
 * Front ends: the original-order in-arc CSR of a sparse graph, or (dense graphs) the essential
 * in-arc CSR compacted here from the public w and lat matrices -- an arc (u, t), u != t, with
 * w[u][t] == lat[u][t]; only those can be tight.
 */
#include "srt_pass.h"

#include <string.h>

#define RT_THREADS 1024
/* dynamic LDS of the route kernel: the staged row (160 KiB per CU, the kernel's few static words
 * left out) */
#define RT_LDS_BYTES (156 * 1024)
/* in-lists of at least this many arcs are walked by the whole wave (64 arcs per step, a 64-bit
 * minimum across the lanes) instead of by their target's lane */
#define RT_WAVE_ARCS 32
/* such lists a wave reads at the same time */
#define RT_GROUP 4
/* the largest n the pass takes */
#define RT_MAX_N (1 << 22)

static size_t rt_row_bytes(int n, int form) {
    return form == 1 ? (size_t)n * 4 : form == 2 ? (((size_t)n * 2 + 3) & ~(size_t)3) : 0;
}

/* largest n of staging form 1 (u32 row in LDS; its jump words carry 16-bit vertices, and 39,936
 * is below that too), 2 (u16 row in LDS) and 3 (row read from global memory: the pass's own
 * limit) */
extern "C" int srt_routes_stage_max_n(int form) {
    if (form < 1 || form > 3) return 0;
    return form == 3 ? RT_MAX_N : (int)(RT_LDS_BYTES / (form == 1 ? 4 : 2));
}

static __device__ __forceinline__ int32_t ld_wg(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ void st_wg(int32_t* p, int32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/* the staged distance of vertex u as u32 quanta (>= SRT_INF: unreachable), the source's own 0 */
template <int FORM>
static __device__ __forceinline__ uint32_t rt_dist(const uint32_t* rowL, const uint32_t* Dr, int s,
                                                   int u) {
    if constexpr (FORM == 1) {
        return rowL[u];
    } else if constexpr (FORM == 2) {
        const uint32_t x = ((const uint16_t*)rowL)[u];
        return x == 0xFFFFu ? (uint32_t)SRT_INF : x;
    } else {
        return u == s ? 0u : Dr[u];
    }
}

/* Phase 1: targets across the threads (coalesced stores); each in-arc offers the key
 * (du << 32) | u, the 64-bit minimum wins. Lists of RT_WAVE_ARCS arcs or more are left to the
 * wave: their lanes are balloted, and each such list is read 64 arcs at a time. icol[0] and
 * iw[0] must be readable (every caller allocates at least one arc). */
template <int FORM>
static __device__ void rt_pred_phase(int n, int s, const uint32_t* rowL, const uint32_t* Dr,
                                     const int32_t* __restrict__ irp,
                                     const int32_t* __restrict__ icol,
                                     const uint32_t* __restrict__ iw, int32_t* P) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int t0 = tid & ~63; t0 < n; t0 += RT_THREADS) { /* wave-uniform trip count */
        const int t = t0 + lane;
        int bu = -1, kb = 0, ke = 0;
        uint32_t dt = SRT_INF;
        bool wide = false;
        if (t < n) {
            dt = rt_dist<FORM>(rowL, Dr, s, t);
            if (t != s && dt < SRT_INF) {
                kb = irp[t];
                ke = irp[t + 1];
                wide = ke - kb >= RT_WAVE_ARCS;
                if (!wide) {
                    uint64_t best = ~0ull;
                    for (int k = kb; k < ke; ++k) {
                        const int u = icol[k];
                        const uint32_t du = rt_dist<FORM>(rowL, Dr, s, u);
                        if (du < SRT_INF && du + iw[k] == dt) {
                            const uint64_t key = ((uint64_t)du << 32) | (uint32_t)u;
                            best = key < best ? key : best;
                        }
                    }
                    if (best != ~0ull) bu = (int)(uint32_t)best;
                }
            }
        }
        /* RT_GROUP lists at a time: their arcs are loaded by straight-line code (indices past a
         * list's end clamped to arc 0 and masked out of the compare), so the loads of the group
         * are in flight together instead of one list's latency after the other's */
        unsigned long long m = __ballot(wide);
        while (m) {
            int lj[RT_GROUP], bj[RT_GROUP], ej[RT_GROUP], span = 0;
            uint32_t dj[RT_GROUP];
            unsigned long long best[RT_GROUP];
#pragma unroll
            for (int j = 0; j < RT_GROUP; ++j) {
                const int l = m ? __ffsll(m) - 1 : -1; /* -1: the slot stays empty */
                m &= m - 1ull;
                lj[j] = l;
                bj[j] = __shfl(kb, l < 0 ? 0 : l);
                ej[j] = l < 0 ? bj[j] : __shfl(ke, l);
                dj[j] = (uint32_t)__shfl((int)dt, l < 0 ? 0 : l);
                best[j] = ~0ull;
                span = ej[j] - bj[j] > span ? ej[j] - bj[j] : span;
            }
            for (int c = lane; c - lane < span; c += 64) {
                int u[RT_GROUP];
                uint32_t wv[RT_GROUP];
                bool in[RT_GROUP];
#pragma unroll
                for (int j = 0; j < RT_GROUP; ++j) {
                    in[j] = bj[j] + c < ej[j];
                    const int k = in[j] ? bj[j] + c : 0;
                    u[j] = icol[k];
                    wv[j] = iw[k];
                }
#pragma unroll
                for (int j = 0; j < RT_GROUP; ++j) {
                    const uint32_t du = rt_dist<FORM>(rowL, Dr, s, u[j]);
                    const unsigned long long key = ((unsigned long long)du << 32) | (uint32_t)u[j];
                    const bool tight = in[j] && du < SRT_INF && du + wv[j] == dj[j];
                    best[j] = tight && key < best[j] ? key : best[j];
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int j = 0; j < RT_GROUP; ++j) {
                    const unsigned long long o = __shfl_xor(best[j], off);
                    best[j] = o < best[j] ? o : best[j];
                }
            }
#pragma unroll
            for (int j = 0; j < RT_GROUP; ++j)
                if (lane == lj[j] && best[j] != ~0ull) bu = (int)(uint32_t)best[j];
        }
        if (t < n) st_wg(P + t, bu);
    }
}

/* Phase 2: hops and first hop by pointer jumping. words[t] = (a << SHIFT | h): a is an ancestor
 * of t, h hops above it. The children of s are the roots (a == t, h = 0); a jump replaces (a, h)
 * by (a', h + h') of a's word, and whichever word of a the jump meets keeps that meaning, so the
 * jumps run in place without a second buffer. Every arc is >= 1 quantum, so the predecessors form
 * a tree and the rounds end after about log2(depth) of them with a = the first hop and h + 1 =
 * the hop count. Returns the calling thread's deepest route. */
template <typename W, int SHIFT>
static __device__ int rt_jump_phase(int n, int s, const int32_t* P, W* words, int32_t* F,
                                    int32_t* H, int* s_any) {
    constexpr W NONE = ~(W)0, LOW = ((W)1 << SHIFT) - 1;
    const int tid = threadIdx.x;
    for (int t = tid; t < n; t += RT_THREADS) {
        const int p = ld_wg(P + t);
        words[t] = p < 0 ? NONE : p == s ? (W)t << SHIFT : ((W)p << SHIFT) | 1u;
    }
    __threadfence_block();
    __syncthreads();
    for (;;) {
        if (tid == 0) *s_any = 0;
        __syncthreads();
        int any = 0;
        for (int t = tid; t < n; t += RT_THREADS) {
            const W w = __hip_atomic_load(words + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const W a = w >> SHIFT;
            if (w == NONE || a == (W)t) continue;
            const W wa = __hip_atomic_load(words + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if ((wa >> SHIFT) == a) continue; /* a is a root: t is resolved */
            __hip_atomic_store(words + t, (wa & ~LOW) | ((w & LOW) + (wa & LOW)), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
            any = 1;
        }
        if (any) *s_any = 1;
        __threadfence_block();
        __syncthreads();
        if (!*s_any) break;
        __syncthreads();
    }
    int depth = 0;
    for (int t = tid; t < n; t += RT_THREADS) {
        const W w = words[t];
        const int h = w == NONE ? (t == s ? 0 : -1) : (int)(w & LOW) + 1;
        if (F) F[t] = w == NONE ? -1 : (int)(w >> SHIFT);
        if (H) H[t] = h;
        depth = h > depth ? h : depth;
    }
    return depth;
}

/* One workgroup per source row (persistent grid). Row r belongs to source s = srcs[r] (or
 * src_begin + r); its distances are row s (by_src) or row r of D.
 * NFORM 1: the row as u32 in LDS; after phase 1 the jump words (16 + 16 bits: n < 0xFFFF here)
 * take its place. NFORM 2: the row as u16 in LDS when every finite entry is below 0xFFFF, else
 * read from global memory (form 3) -- decided per row while it is staged. NFORM 3: always from
 * global memory. Forms 2 and 3 jump over 32 + 32-bit words in the block's scratch row (jump).
 * P: the pred output's row, or the block's scratch row where that output is NULL. */
template <int NFORM>
__global__ __launch_bounds__(RT_THREADS) void routes_kernel(
    int n, int nrows, const int32_t* __restrict__ srcs, int src_begin, int by_src,
    const uint32_t* __restrict__ D, size_t ldd, const int32_t* __restrict__ irp,
    const int32_t* __restrict__ icol, const uint32_t* __restrict__ iw, int32_t* pred,
    int32_t* first, int32_t* hops, size_t ldo, int32_t* ws_pred, unsigned long long* ws_jump,
    int32_t* max_hops, uint32_t* forms) {
    extern __shared__ uint32_t rowL[];
    __shared__ int s_any;
    __shared__ uint32_t s_max;
    const int tid = threadIdx.x;
    int depth_max = 0;
    uint32_t form_mask = 0u;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int s = srcs ? srcs[r] : src_begin + r;
        if (s < 0 || s >= n) continue; /* not a vertex (block-uniform): the row is left alone */
        const uint32_t* Dr = D + (size_t)(by_src ? s : r) * ldd;
        int32_t* P = pred ? pred + (size_t)r * ldo : ws_pred + (size_t)blockIdx.x * n;
        int32_t* F = first ? first + (size_t)r * ldo : NULL;
        int32_t* H = hops ? hops + (size_t)r * ldo : NULL;
        /* ---- stage the row, the source's own entry as 0 -------------------------------- */
        int form = NFORM;
        if constexpr (NFORM == 1) {
            for (int t = tid; t < n; t += RT_THREADS) rowL[t] = t == s ? 0u : Dr[t];
        } else if constexpr (NFORM == 2) {
            if (tid == 0) s_max = 0u;
            __syncthreads();
            uint16_t* row16 = (uint16_t*)rowL;
            uint32_t mx = 0u;
            for (int t = tid; t < n; t += RT_THREADS) {
                const uint32_t d = t == s ? 0u : Dr[t];
                if (d < SRT_INF) mx = d > mx ? d : mx;
                row16[t] = (uint16_t)(d < 0xFFFFu ? d : 0xFFFFu);
            }
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)mx, off);
                mx = o > mx ? o : mx;
            }
            if ((tid & 63) == 0 && mx) atomicMax(&s_max, mx);
            __syncthreads();
            if (s_max >= 0xFFFFu) form = 3;
        }
        __syncthreads();
        form_mask |= 1u << (form - 1);
        /* ---- phase 1: predecessors ----------------------------------------------------- */
        if (form == 1)
            rt_pred_phase<1>(n, s, rowL, Dr, irp, icol, iw, P);
        else if (form == 2)
            rt_pred_phase<2>(n, s, rowL, Dr, irp, icol, iw, P);
        else
            rt_pred_phase<3>(n, s, rowL, Dr, irp, icol, iw, P);
        __threadfence_block();
        __syncthreads(); /* the staged distances are dead from here */
        /* ---- phase 2: hops and first hop ------------------------------------------------ */
        int depth;
        if constexpr (NFORM == 1)
            depth = rt_jump_phase<uint32_t, 16>(n, s, P, rowL, F, H, &s_any);
        else
            depth = rt_jump_phase<unsigned long long, 32>(n, s, P, ws_jump + (size_t)blockIdx.x * n, F,
                                                          H, &s_any);
        depth_max = depth > depth_max ? depth : depth_max;
        __syncthreads();
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(depth_max, off);
        depth_max = o > depth_max ? o : depth_max;
    }
    if ((tid & 63) == 0) srt_max_once(max_hops, depth_max);
    if (tid == 0 && form_mask) atomicOr(forms, form_mask);
}

/* The route pass over nrows distance rows (see routes_kernel); any output may be NULL. Adds the
 * deepest route to *max_hops and the staging forms taken to *forms; returns after the stream. */
int srt_routes_rows(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                    const uint32_t* D, size_t ldd, const int32_t* irp, const int32_t* icol,
                    const uint32_t* iw, int32_t* pred, int32_t* first, int32_t* hops, size_t ldo,
                    hipStream_t st, int32_t* max_hops, int32_t* forms) {
    if (nrows <= 0) return SRT_OK;
    if (n < 1 || !D || !irp || !icol || !iw || ldd < (size_t)n ||
        ((pred || first || hops) && ldo < (size_t)n)) {
        srt_set_error("route pass: bad arguments (n = %d, ldd = %zu, ldo = %zu)", n, ldd, ldo);
        return SRT_E_ARG;
    }
    if (n > srt_routes_stage_max_n(3)) {
        srt_set_error("route pass: n = %d beyond its range (%d)", n, srt_routes_stage_max_n(3));
        return SRT_E_RANGE;
    }
    const int nform = n <= srt_routes_stage_max_n(1) ? 1 : n <= srt_routes_stage_max_n(2) ? 2 : 3;
    const size_t lds = rt_row_bytes(n, nform);
    /* per-block scratch: the predecessor row where that output is NULL, the jump words of forms 2
     * and 3; the grid shrinks where it would pass SRT_PASS_SCRATCH_BYTES */
    const size_t per_block = (size_t)n * ((pred ? 0 : sizeof(int32_t)) + (nform == 1 ? 0 : 8));
    const int grid = srt_pass_grid(lds, per_block, nrows, false);
    srt_pass_scratch sc;
    int32_t* ws_pred = NULL;
    unsigned long long* ws_jump = NULL;
    int32_t hstat[2] = {0, 0};
    int rc = sc.open("route pass", st, (size_t)grid * per_block, sizeof(hstat));
    if (rc) return rc;
    char* const ws = sc.ws;
    int32_t* const dstat = (int32_t*)sc.dstat;
    if (nform != 1) ws_jump = (unsigned long long*)ws; /* the 8-byte words first: aligned */
    if (!pred) ws_pred = (int32_t*)(ws + (nform == 1 ? 0 : (size_t)grid * n * 8));
    if (nform == 1) {
        SRT_PASS_TRY(hipFuncSetAttribute((const void*)routes_kernel<1>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        routes_kernel<1><<<grid, RT_THREADS, lds, st>>>(n, nrows, srcs, src_begin, by_src, D, ldd, irp,
                                                        icol, iw, pred, first, hops, ldo, ws_pred,
                                                        ws_jump, dstat, (uint32_t*)dstat + 1);
    } else if (nform == 2) {
        SRT_PASS_TRY(hipFuncSetAttribute((const void*)routes_kernel<2>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        routes_kernel<2><<<grid, RT_THREADS, lds, st>>>(n, nrows, srcs, src_begin, by_src, D, ldd, irp,
                                                        icol, iw, pred, first, hops, ldo, ws_pred,
                                                        ws_jump, dstat, (uint32_t*)dstat + 1);
    } else {
        routes_kernel<3><<<grid, RT_THREADS, 0, st>>>(n, nrows, srcs, src_begin, by_src, D, ldd, irp,
                                                      icol, iw, pred, first, hops, ldo, ws_pred,
                                                      ws_jump, dstat, (uint32_t*)dstat + 1);
    }
    SRT_PASS_TRY(hipGetLastError());
out:
    rc = sc.finish(rc, hstat);
    if (!rc) {
        if (max_hops && hstat[0] > *max_hops) *max_hops = hstat[0];
        if (forms) *forms |= hstat[1];
    }
    return rc;
}

/* ------------------------------------------------------------------------------------------ */
/* Dense front end: the essential in-arc CSR from the public matrices. One wave per matrix row,  */
/* 64 columns per step (coalesced), rows and columns >= n (the ld padding) never read.           */
/* Undirected: row t is t's in-list (w and lat are symmetric), ballot-compacted in column order. */
/* Directed: row u holds u's out-arcs; each is counted at, then filled into, its head's list     */
/* through a per-head cursor (the order inside an in-list is free: the key carries u).           */
/* ------------------------------------------------------------------------------------------ */
template <bool FILL>
__global__ __launch_bounds__(256) void rt_ess_kernel(int n, int ld, int directed,
                                                     const uint32_t* __restrict__ w,
                                                     const uint32_t* __restrict__ lat,
                                                     int32_t* __restrict__ cnt,
                                                     const int32_t* __restrict__ rp,
                                                     int32_t* __restrict__ cur,
                                                     int32_t* __restrict__ icol,
                                                     uint32_t* __restrict__ iw) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    for (int u = wave; u < n; u += nwaves) {
        const uint32_t* wr = w + (size_t)u * ld;
        const uint32_t* lr = lat + (size_t)u * ld;
        int base = FILL && !directed ? rp[u] : 0;
        for (int c0 = 0; c0 < n; c0 += 64) {
            const int c = c0 + lane;
            uint32_t wv = SRT_INF;
            bool ess = false;
            if (c < n && c != u) {
                wv = wr[c];
                ess = wv < SRT_INF && wv == lr[c];
            }
            if (directed) {
                if (ess) {
                    if constexpr (FILL) {
                        const int pos = atomicAdd(&cur[c], 1);
                        icol[pos] = u;
                        iw[pos] = wv;
                    } else {
                        atomicAdd(&cnt[c], 1);
                    }
                }
            } else {
                const unsigned long long m = __ballot(ess);
                if constexpr (FILL) {
                    if (ess) {
                        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
                        icol[pos] = c;
                        iw[pos] = wv;
                    }
                }
                base += __popcll(m);
            }
        }
        if (!FILL && !directed && lane == 0) cnt[u] = base;
    }
}

/* exclusive scan of cnt[0, n) into rp[0, n], rp[n] = the total, cur = a copy of rp (one block) */
__global__ __launch_bounds__(1024) void rt_scan_kernel(int n, const int32_t* __restrict__ cnt,
                                                       int32_t* __restrict__ rp,
                                                       int32_t* __restrict__ cur) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int b = tid * per < n ? tid * per : n, e = b + per < n ? b + per : n;
    int sum = 0;
    for (int i = b; i < e; ++i) sum += cnt[i];
    part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int i = b; i < e; ++i) {
        rp[i] = run;
        cur[i] = run;
        run += cnt[i];
    }
    if (tid == 1023) rp[n] = part[1023];
}

/* irp (n + 1), icol, iw of the essential in-arcs on the device; *arcs = their number, *ms += the
 * HIP-event time of the compaction. The arrays come from the scratch pool: srt_routes_ess_free
 * returns them (stream-ordered). */
int srt_routes_ess_build(int n, int ld, int directed, const uint32_t* w, const uint32_t* lat,
                         hipStream_t st, int32_t** irp, int32_t** icol, uint32_t** iw,
                         int64_t* arcs, double* ms) {
    *irp = NULL;
    *icol = NULL;
    *iw = NULL;
    int32_t* cnt = NULL;
    int32_t total = 0;
    srt_event_span span;
    int rc = span.begin(st);
    if (rc) return rc;
    const int grid = srt_ceil_div(n, 4) < 4096 ? srt_ceil_div(n, 4) : 4096;
    /* cnt: n counters, then n cursors */
    SRT_PASS_TRY(srt_malloc_async((void**)&cnt, 2 * (size_t)n * sizeof(int32_t), st));
    SRT_PASS_TRY(srt_malloc_async((void**)irp, ((size_t)n + 1) * sizeof(int32_t), st));
    SRT_PASS_TRY(hipMemsetAsync(cnt, 0, 2 * (size_t)n * sizeof(int32_t), st));
    rt_ess_kernel<false><<<grid, 256, 0, st>>>(n, ld, directed, w, lat, cnt, NULL, NULL, NULL, NULL);
    SRT_PASS_TRY(hipGetLastError());
    rt_scan_kernel<<<1, 1024, 0, st>>>(n, cnt, *irp, cnt + n);
    SRT_PASS_TRY(hipGetLastError());
    SRT_PASS_TRY(hipMemcpyAsync(&total, *irp + n, sizeof(total), hipMemcpyDeviceToHost, st));
    SRT_PASS_TRY(hipStreamSynchronize(st));
    SRT_PASS_TRY(srt_malloc_async((void**)icol, ((size_t)total + 1) * sizeof(int32_t), st));
    SRT_PASS_TRY(srt_malloc_async((void**)iw, ((size_t)total + 1) * sizeof(uint32_t), st));
    rt_ess_kernel<true><<<grid, 256, 0, st>>>(n, ld, directed, w, lat, NULL, *irp, cnt + n, *icol, *iw);
    SRT_PASS_TRY(hipGetLastError());
    *arcs = total;
    rc = span.end(st, ms);
out:
    if (cnt) (void)hipFreeAsync(cnt, st);
    if (rc) {
        if (*irp) (void)hipFreeAsync(*irp, st);
        if (*icol) (void)hipFreeAsync(*icol, st);
        if (*iw) (void)hipFreeAsync(*iw, st);
        *irp = NULL;
        *icol = NULL;
        *iw = NULL;
    }
    return rc;
}

void srt_routes_ess_free(int32_t* irp, int32_t* icol, uint32_t* iw, hipStream_t st) {
    if (irp) (void)hipFreeAsync(irp, st);
    if (icol) (void)hipFreeAsync(icol, st);
    if (iw) (void)hipFreeAsync(iw, st);
}

/* the timed route pass of the public entry points: adds to *stats (the caller zeroes it) */
int srt_routes_rows_timed(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                          const uint32_t* D, size_t ldd, const int32_t* irp, const int32_t* icol,
                          const uint32_t* iw, int32_t* pred, int32_t* first, int32_t* hops,
                          size_t ldo, hipStream_t st, srt_route_stats* stats) {
    srt_event_span span;
    int rc = span.begin(st);
    if (rc) return rc;
    int32_t mh = 0, forms = 0;
    rc = srt_routes_rows(n, nrows, srcs, src_begin, by_src, D, ldd, irp, icol, iw, pred, first, hops,
                         ldo, st, &mh, &forms);
    if (rc) return rc;
    double ms = 0;
    rc = span.end(st, &ms);
    if (!rc && stats) {
        stats->ms_routes += ms;
        stats->max_hops = mh > stats->max_hops ? mh : stats->max_hops;
        stats->stage_forms |= forms;
    }
    return rc;
}

extern "C" int srt_routes_dense_device(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                                       const uint32_t* lat, int32_t row0, int32_t nrows,
                                       int32_t* pred, int32_t* first, int32_t* hops, size_t ldo,
                                       void* stream, srt_route_stats* stats) {
    if (n < 1 || ld < n || !w || !lat || row0 < 0 || nrows < 1 || (int64_t)row0 + nrows > n ||
        ((pred || first || hops) && ldo < (size_t)n)) {
        srt_set_error("srt_routes_dense_device: bad arguments (n = %d, ld = %d, rows [%d, %d))", n, ld,
                      row0, row0 + nrows);
        return SRT_E_ARG;
    }
    if (n > SRT_DENSE_MAX_N) {
        srt_set_error("srt_routes_dense_device: n = %d beyond the dense limit %d (int32 arc offsets)",
                      n, SRT_DENSE_MAX_N);
        return SRT_E_RANGE;
    }
    hipStream_t st = (hipStream_t)stream;
    srt_route_stats local;
    memset(&local, 0, sizeof(local));
    int32_t *irp = NULL, *icol = NULL;
    uint32_t* iw = NULL;
    /* the compaction counts as the route pass */
    int rc = srt_routes_ess_build(n, ld, directed, w, lat, st, &irp, &icol, &iw, &local.ess_arcs,
                                  &local.ms_routes);
    if (!rc)
        rc = srt_routes_rows_timed(n, nrows, NULL, row0, 0, lat + (size_t)row0 * ld, (size_t)ld, irp,
                                   icol, iw, pred, first, hops, ldo, st, &local);
    srt_routes_ess_free(irp, icol, iw, st);
    if (!rc && stats) *stats = local;
    return rc;
}
