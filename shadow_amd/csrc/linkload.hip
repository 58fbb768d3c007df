/*
 * linkload.hip -- link load, gfx950: how much demand crosses every canonical arc, and how much
 * passes through every vertex, given the routes of routes.hip.
 *
 * Per source s the canonical predecessors form a tree. With c(s, t) the demand of the pair,
 *   flow_s(t) = c(s, t) + sum of flow_s over t's children,
 * the arc (pred(s, t), t) carries flow_s(t) and the vertex v != s lets flow_s(v) - c(s, v) through.
 * The pass reads the pred and hops rows the route pass wrote, a u64 demand row per source and the
 * in-arc CSR the route pass used; it adds into load[k] (one u64 per CSR position), through[v] and
 * three demand totals (routed, unrouted, self) with 64-bit integer atomics, so the sums do not
 * depend on the order the rows arrive in.
 *
 * One 1,024-thread workgroup per source row (persistent grid). The subtree sums run by hop level,
 * deepest first: the targets are ordered by hop count once per row (a counting sort inside the
 * workgroup), then every level is one contiguous segment of that order and costs one barrier.
 */
#include "srt_pass.h"

#include <string.h>

#define LL_THREADS 1024
/* dynamic LDS of the kernel: the row's flow words (the route kernel's figure) */
#define LL_LDS_BYTES (156 * 1024)
/* in-lists of at least this many arcs are searched by the whole wave, LL_GROUP of them at once
 * (the route pass's pattern and figures; the threshold is reasoned there, not measured here) */
#define LL_WAVE_ARCS 32
#define LL_GROUP 4
/* distinct hop counts per wave and step that share one counter add before the rest add alone */
#define LL_AGG 4
/* hop levels counted in LDS by rows too long for LDS flow words; deeper rows count in scratch */
#define LL_BIG_LEVELS 4096
#define LL_MAX_N (1 << 22)

typedef unsigned long long ull;

/* largest n of flow form 1 (u32 words in LDS: rows whose routed demand is below 2^32), 2 (u64
 * words in LDS) and 3 (u64 words in the workgroup's scratch row: the pass's own limit) */
extern "C" int srt_link_load_stage_max_n(int form) {
    if (form < 1 || form > 3) return 0;
    return form == 3 ? LL_MAX_N : (int)(LL_LDS_BYTES / (form == 1 ? 4 : 8));
}

#define LL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define LL_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

/* Level counters: LDS words, or scratch words that the atomics change at the memory side -- those
 * are read and written past the L1 (agent-scope atomic loads and stores; every access to such a
 * word is an atomic one). */
template <bool GLOB>
static __device__ __forceinline__ uint32_t cnt_ld(const uint32_t* c, int i) {
    if constexpr (GLOB) return __hip_atomic_load(c + i, LL_RLX_AGENT);
    return c[i];
}
template <bool GLOB>
static __device__ __forceinline__ void cnt_st(uint32_t* c, int i, uint32_t v) {
    if constexpr (GLOB)
        __hip_atomic_store(c + i, v, LL_RLX_AGENT);
    else
        c[i] = v;
}
/* The barrier between two phases. GLOB: the phases meet in scratch words of this workgroup that
 * only atomics touch, so nothing has to leave a cache: each wave waits until its own stores and
 * adds are done, then the barrier. (An agent-scope fence here writes back the XCD's whole L2,
 * ~100 us a level with 32 workgroups staging rows beside each other: C5 took 113 ms with it.) */
template <bool GLOB>
static __device__ __forceinline__ void ll_sync() {
    if constexpr (GLOB) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

/* cnt[h] += 1 for every valid lane, returning the value before the lane's own add. Lanes of a wave
 * with the same h share one add (up to LL_AGG distinct values per call: a row has few levels, or
 * few targets per level). Called by whole waves. */
static __device__ __forceinline__ int ll_take(uint32_t* cnt, int h, bool valid) {
    const int lane = threadIdx.x & 63;
    int pos = -1;
    bool mine = valid;
    for (int it = 0; it < LL_AGG; ++it) {
        const ull todo = __ballot(mine);
        if (!todo) break;
        const int h0 = __shfl(h, __ffsll(todo) - 1);
        const bool hit = mine && h == h0;
        const ull m = __ballot(hit);
        const int lead = __ffsll(m) - 1;
        int base = 0;
        if (lane == lead) base = (int)atomicAdd(cnt + h0, (uint32_t)__popcll(m));
        base = __shfl(base, lead);
        if (hit) {
            pos = base + __popcll(m & ((1ull << lane) - 1ull));
            mine = false;
        }
    }
    if (mine) pos = (int)atomicAdd(cnt + h, 1u);
    return pos;
}

/* Flow words of one row. FORM 1: u32 in LDS, 2: u64 in LDS, 3: u64 in the scratch row (atomics at
 * the memory side, reads past the L1). */
template <int FORM>
struct ll_flow {
    static __device__ __forceinline__ void set(void* p, int t, ull v) {
        if constexpr (FORM == 1)
            ((uint32_t*)p)[t] = (uint32_t)v;
        else if constexpr (FORM == 2)
            ((ull*)p)[t] = v;
        else
            __hip_atomic_store((ull*)p + t, v, LL_RLX_AGENT);
    }
    static __device__ __forceinline__ ull get(const void* p, int t) {
        if constexpr (FORM == 1)
            return ((const uint32_t*)p)[t];
        else if constexpr (FORM == 2)
            return ((const ull*)p)[t];
        else
            return __hip_atomic_load((const ull*)p + t, LL_RLX_AGENT);
    }
    static __device__ __forceinline__ void add(void* p, int t, ull v) {
        if constexpr (FORM == 1)
            atomicAdd((uint32_t*)p + t, (uint32_t)v);
        else
            atomicAdd((ull*)p + t, v);
    }
};

/* the hop count of t as the pass takes it: anything outside [0, n) counts as unreachable */
static __device__ __forceinline__ int ll_hops(const int32_t* H, int n, int t) {
    const int h = H[t];
    return h >= n ? -1 : h;
}

/* The row's targets ordered by hop count into order[]; lvl[h] = the end of level h's segment (its
 * begin is lvl[h - 1], lvl[0] = 0). cnt: maxh + 1 counters, LDS or (GLOB) lvl itself. */
template <bool GLOB>
static __device__ void ll_order_phase(int n, int s, int maxh, const int32_t* H, uint32_t* cnt,
                                      int32_t* order, uint32_t* lvl, uint32_t* s_part) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = maxh + 1;
    for (int i = tid; i < L; i += LL_THREADS) cnt_st<GLOB>(cnt, i, 0u);
    ll_sync<GLOB>();
    for (int t0 = tid & ~63; t0 < n; t0 += LL_THREADS) { /* wave-uniform trip count */
        const int t = t0 + lane;
        const int h = t < n && t != s ? ll_hops(H, n, t) : -1;
        (void)ll_take(cnt, h, h >= 1);
    }
    ll_sync<GLOB>();
    /* exclusive scan in place: a contiguous piece per thread, the waves' sums through LDS */
    {
        const int per = (L + LL_THREADS - 1) / LL_THREADS;
        const int b = tid * per < L ? tid * per : L, e = b + per < L ? b + per : L;
        uint32_t sum = 0;
        for (int i = b; i < e; ++i) sum += cnt_ld<GLOB>(cnt, i);
        uint32_t inc = sum;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)inc, off);
            if (lane >= off) inc += v;
        }
        if (lane == 63) s_part[wave] = inc;
        __syncthreads();
        uint32_t run = inc - sum;
        for (int w = 0; w < wave; ++w) run += s_part[w];
        for (int i = b; i < e; ++i) {
            const uint32_t c = cnt_ld<GLOB>(cnt, i);
            cnt_st<GLOB>(cnt, i, run);
            run += c;
        }
    }
    ll_sync<GLOB>();
    /* scatter: each counter is its level's cursor and ends as the level's end */
    for (int t0 = tid & ~63; t0 < n; t0 += LL_THREADS) {
        const int t = t0 + lane;
        const int h = t < n && t != s ? ll_hops(H, n, t) : -1;
        const int pos = ll_take(cnt, h, h >= 1);
        if (h >= 1) __hip_atomic_store(order + pos, t, LL_RLX_WG);
    }
    ll_sync<GLOB>();
    if constexpr (!GLOB) {
        for (int i = tid; i < L; i += LL_THREADS) __hip_atomic_store(lvl + i, cnt[i], LL_RLX_AGENT);
        ll_sync<true>();
    }
}

/* One level's segment [sb, se) of the order, in-lists with ascending tails: the arc (pred(t), t)
 * by the lane's binary search. */
template <int FORM>
static __device__ __forceinline__ void ll_level_sorted(int n, int s, int sb, int se,
                                                       const int32_t* __restrict__ P,
                                                       const ull* __restrict__ C,
                                                       const int32_t* __restrict__ irp,
                                                       const int32_t* __restrict__ icol,
                                                       void* flow, const int32_t* order, ull* load,
                                                       ull* through) {
    for (int i = sb + (int)threadIdx.x; i < se; i += LL_THREADS) {
        const int t = __hip_atomic_load(order + i, LL_RLX_WG);
        const ull f = ll_flow<FORM>::get(flow, t);
        if (!f) continue;
        const int p = P[t];
        const ull c = C[t];
        if (p >= 0 && p < n) {
            const int ke = irp[t + 1];
            int lo = irp[t], hi = ke;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (icol[mid] < p)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < ke && icol[lo] == p) atomicAdd(load + lo, f);
            if (p != s) ll_flow<FORM>::add(flow, p, f);
        }
        if (f != c) atomicAdd(through + t, f - c);
    }
}

/* The same over in-lists in no order (the essential lists of a directed dense graph): a list
 * shorter than LL_WAVE_ARCS is scanned by its target's lane, a longer one by the wave. */
template <int FORM>
static __device__ __forceinline__ void ll_level_scan(int n, int s, int sb, int se,
                                                     const int32_t* __restrict__ P,
                                                     const ull* __restrict__ C,
                                                     const int32_t* __restrict__ irp,
                                                     const int32_t* __restrict__ icol, void* flow,
                                                     const int32_t* order, ull* load,
                                                     ull* through) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i0 = sb + (tid & ~63); i0 < se; i0 += LL_THREADS) { /* wave-uniform trip count */
        const int i = i0 + lane;
        ull f = 0ull;
        int p = -1, kb = 0, ke = 0, pos = -1;
        bool wide = false;
        if (i < se) {
            const int t = __hip_atomic_load(order + i, LL_RLX_WG);
            f = ll_flow<FORM>::get(flow, t);
            if (f) {
                p = P[t];
                if (p >= 0 && p < n) {
                    kb = irp[t];
                    ke = irp[t + 1];
                    wide = ke - kb >= LL_WAVE_ARCS;
                    if (!wide)
                        for (int k = kb; k < ke; ++k)
                            if (icol[k] == p) pos = k;
                    if (p != s) ll_flow<FORM>::add(flow, p, f);
                }
                const ull c = C[t];
                if (f != c) atomicAdd(through + t, f - c);
            }
        }
        /* LL_GROUP long lists at a time, 64 arcs of each per step: indices past a list's end are
         * clamped to arc 0 and masked out, so the group's loads are in flight together */
        ull m = __ballot(wide);
        while (m) {
            int lj[LL_GROUP], bj[LL_GROUP], ej[LL_GROUP], pj[LL_GROUP], fj[LL_GROUP], span = 0;
#pragma unroll
            for (int j = 0; j < LL_GROUP; ++j) {
                const int l = m ? __ffsll(m) - 1 : -1; /* -1: the slot stays empty */
                m &= m - 1ull;
                lj[j] = l;
                bj[j] = __shfl(kb, l < 0 ? 0 : l);
                ej[j] = l < 0 ? bj[j] : __shfl(ke, l);
                pj[j] = __shfl(p, l < 0 ? 0 : l);
                fj[j] = -1;
                span = ej[j] - bj[j] > span ? ej[j] - bj[j] : span;
            }
            for (int c = lane; c - lane < span; c += 64) {
#pragma unroll
                for (int j = 0; j < LL_GROUP; ++j) {
                    const bool in = bj[j] + c < ej[j];
                    const int k = in ? bj[j] + c : 0;
                    if (icol[k] == pj[j] && in) fj[j] = k;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
                for (int j = 0; j < LL_GROUP; ++j) {
                    const int o = __shfl_xor(fj[j], off);
                    fj[j] = o > fj[j] ? o : fj[j];
                }
            }
#pragma unroll
            for (int j = 0; j < LL_GROUP; ++j)
                if (lane == lj[j]) pos = fj[j];
        }
        if (f && pos >= 0) atomicAdd(load + pos, f);
    }
}

/* The subtree sums of one row, deepest level first; adds the arcs' and the vertices' shares. The
 * level ends come 64 at a time into a register per lane (lane j: lvl[base - j]) and are handed
 * round by shuffles, so a level costs its segment and one barrier, not a trip to memory. */
template <int FORM, bool SORTED>
static __device__ void ll_reduce_phase(int n, int s, int maxh, const int32_t* __restrict__ P,
                                       const int32_t* __restrict__ H, const ull* __restrict__ C,
                                       const int32_t* __restrict__ irp,
                                       const int32_t* __restrict__ icol, void* flow,
                                       const int32_t* order, const uint32_t* lvl, ull* load,
                                       ull* through) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int t = tid; t < n; t += LL_THREADS)
        ll_flow<FORM>::set(flow, t, t != s && ll_hops(H, n, t) >= 1 ? C[t] : 0ull);
    ll_sync<FORM == 3>();
    int base = -1;
    uint32_t lv = 0u;
    for (int h = maxh; h >= 1; --h) {
        if (base < 0 || h - 1 < base - 63) { /* block-uniform */
            base = h;
            lv = base - lane >= 0 ? __hip_atomic_load(lvl + (base - lane), LL_RLX_AGENT) : 0u;
        }
        const int se = __shfl((int)lv, base - h), sb = __shfl((int)lv, base - h + 1);
        if constexpr (SORTED)
            ll_level_sorted<FORM>(n, s, sb, se, P, C, irp, icol, flow, order, load, through);
        else
            ll_level_scan<FORM>(n, s, sb, se, P, C, irp, icol, flow, order, load, through);
        ll_sync<FORM == 3>();
    }
}

/* One workgroup per source row (persistent grid). Row r belongs to source s = srcs[r] (or
 * src_begin + r); pred, hops (stride ldp) and dem (stride ldd) are its rows. lds_words: the u32
 * words of dynamic LDS. Scratch per workgroup: order (n), lvl (n + 1), and (flow != NULL) n u64
 * flow words. totals: routed, unrouted, self. */
template <bool SORTED>
__global__ __launch_bounds__(LL_THREADS) void link_load_kernel(
    int n, int nrows, const int32_t* __restrict__ srcs, int src_begin, const int32_t* pred,
    const int32_t* hops, size_t ldp, const ull* dem, size_t ldd, const int32_t* __restrict__ irp,
    const int32_t* __restrict__ icol, ull* load, ull* through, ull* totals, int32_t* ws_order,
    uint32_t* ws_lvl, ull* ws_flow, int lds_words, int32_t* max_hops, uint32_t* forms) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ldsw[];
    __shared__ ull s_red[16][3];
    __shared__ int s_mh[16];
    __shared__ uint32_t s_part[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int max1 = LL_LDS_BYTES / 4, max2 = LL_LDS_BYTES / 8;
    int32_t* order = ws_order + (size_t)blockIdx.x * n;
    uint32_t* lvl = ws_lvl + (size_t)blockIdx.x * ((size_t)n + 1);
    ull* gflow = ws_flow ? ws_flow + (size_t)blockIdx.x * n : NULL;
    ull tot[3] = {0ull, 0ull, 0ull}; /* thread 0: the block's rows */
    int depth_max = 0;
    uint32_t form_mask = 0u;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int s = srcs ? srcs[r] : src_begin + r;
        if (s < 0 || s >= n) continue; /* not a vertex (block-uniform): the row is left alone */
        const int32_t* P = pred + (size_t)r * ldp;
        const int32_t* H = hops + (size_t)r * ldp;
        const ull* C = dem + (size_t)r * ldd;
        /* ---- the row's demand totals and its deepest route ------------------------------ */
        ull a[3] = {0ull, 0ull, 0ull};
        int mh = 0;
        for (int t = tid; t < n; t += LL_THREADS) {
            const ull c = C[t];
            const int h = ll_hops(H, n, t);
            if (t == s) {
                a[2] += c;
            } else if (h < 1) {
                a[1] += c;
            } else {
                a[0] += c;
                mh = h > mh ? h : mh;
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j) a[j] += __shfl_xor(a[j], off);
            const int o = __shfl_xor(mh, off);
            mh = o > mh ? o : mh;
        }
        if (lane == 0) {
            s_red[wave][0] = a[0];
            s_red[wave][1] = a[1];
            s_red[wave][2] = a[2];
            s_mh[wave] = mh;
        }
        __syncthreads();
        ull routed = 0ull, unrouted = 0ull, selfd = 0ull;
        int maxh = 0;
        for (int w = 0; w < LL_THREADS / 64; ++w) {
            routed += s_red[w][0];
            unrouted += s_red[w][1];
            selfd += s_red[w][2];
            maxh = s_mh[w] > maxh ? s_mh[w] : maxh;
        }
        __syncthreads();
        tot[0] += routed;
        tot[1] += unrouted;
        tot[2] += selfd;
        if (routed == 0ull) continue; /* nothing to carry (block-uniform): the row takes no form */
        depth_max = maxh > depth_max ? maxh : depth_max;
        /* ---- the targets by hop count ---------------------------------------------------- */
        if (maxh + 1 <= lds_words)
            ll_order_phase<false>(n, s, maxh, H, ldsw, order, lvl, s_part);
        else
            ll_order_phase<true>(n, s, maxh, H, lvl, order, lvl, s_part);
        /* ---- the subtree sums ------------------------------------------------------------ */
        const int form = (routed >> 32) == 0ull && n <= max1 ? 1 : n <= max2 ? 2 : 3;
        form_mask |= 1u << (form - 1);
        if (form == 1)
            ll_reduce_phase<1, SORTED>(n, s, maxh, P, H, C, irp, icol, ldsw, order, lvl, load, through);
        else if (form == 2)
            ll_reduce_phase<2, SORTED>(n, s, maxh, P, H, C, irp, icol, ldsw, order, lvl, load, through);
        else
            ll_reduce_phase<3, SORTED>(n, s, maxh, P, H, C, irp, icol, gflow, order, lvl, load, through);
    }
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (tot[j]) atomicAdd(totals + j, tot[j]);
        if (form_mask) atomicOr(forms, form_mask);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(depth_max, off);
        depth_max = o > depth_max ? o : depth_max;
    }
    if (lane == 0) srt_max_once(max_hops, depth_max);
}

/* Demand rows of a chunk: row r (stride ldd) <- 1 everywhere (uniform), or the COO entries
 * [rowptr[r], rowptr[r + 1]) added into a zeroed row (duplicates add). One workgroup per row. */
__global__ __launch_bounds__(256) void ll_demand_kernel(int n, int nrows, int uniform,
                                                        const int64_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ tgt,
                                                        const ull* __restrict__ val, ull* dem,
                                                        size_t ldd) {
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        ull* row = dem + (size_t)r * ldd;
        for (int t = threadIdx.x; t < n; t += 256) row[t] = uniform ? 1ull : 0ull;
        if (uniform) continue;
        __threadfence();
        __syncthreads();
        const int64_t b = rowptr[r], e = rowptr[r + 1];
        for (int64_t k = b + threadIdx.x; k < e; k += 256) {
            const int t = tgt[k];
            if (t >= 0 && t < n) atomicAdd(row + t, val[k]);
        }
        __syncthreads();
    }
}

int srt_link_load_demand_rows(int n, int nrows, const int64_t* rowptr, const int32_t* tgt,
                              const uint64_t* val, uint64_t* dem, size_t ldd, hipStream_t st) {
    if (nrows <= 0) return SRT_OK;
    if (n < 1 || !dem || ldd < (size_t)n || (rowptr && (!tgt || !val))) {
        srt_set_error("link load: bad demand arguments");
        return SRT_E_ARG;
    }
    const int grid = nrows < 4096 ? nrows : 4096;
    ll_demand_kernel<<<grid, 256, 0, st>>>(n, nrows, rowptr ? 0 : 1, rowptr, tgt, (const ull*)val,
                                           (ull*)dem, ldd);
    SRT_HIPCHK(hipGetLastError());
    return SRT_OK;
}

/* The load pass over nrows rows (see link_load_kernel): adds into load, through and totals (the
 * caller zeroes them); sorted != 0 promises in-lists with ascending tails; raises *max_hops, ors
 * the flow forms taken into *forms, adds the HIP-event time of the pass to *ms. Returns after the
 * stream. */
int srt_link_load_rows(int n, int nrows, const int32_t* srcs, int src_begin, const int32_t* pred,
                       const int32_t* hops, size_t ldp, const uint64_t* dem, size_t ldd,
                       const int32_t* irp, const int32_t* icol, uint64_t* load, uint64_t* through,
                       int sorted, uint64_t* totals, hipStream_t st, int32_t* max_hops,
                       int32_t* forms, double* ms) {
    if (nrows <= 0) return SRT_OK;
    if (n < 1 || !pred || !hops || !dem || !irp || !icol || !load || !through || !totals ||
        ldp < (size_t)n || ldd < (size_t)n) {
        srt_set_error("link load: bad arguments (n = %d, ldp = %zu, ldd = %zu)", n, ldp, ldd);
        return SRT_E_ARG;
    }
    if (n > srt_link_load_stage_max_n(3)) {
        srt_set_error("link load: n = %d beyond its range (%d)", n, srt_link_load_stage_max_n(3));
        return SRT_E_RANGE;
    }
    const int max1 = srt_link_load_stage_max_n(1), max2 = srt_link_load_stage_max_n(2);
    const size_t lds = n <= max2 ? (size_t)n * 8 : n <= max1 ? (size_t)n * 4 : (size_t)LL_BIG_LEVELS * 4;
    const bool gflow = n > max2; /* some row may take form 3 */
    /* per workgroup: order (n int32), lvl (n + 1 u32), the form-3 flow words (n u64) */
    const size_t per_block = (size_t)n * 4 + ((size_t)n + 1) * 4 + (gflow ? (size_t)n * 8 : 0);
    const int grid = srt_pass_grid(lds, per_block, nrows, false);
    srt_pass_scratch sc;
    srt_event_span span;
    int32_t hstat[2] = {0, 0};
    double span_ms = 0;
    /* the u64 words first (aligned), then lvl, then order */
    const size_t off_lvl = gflow ? (size_t)grid * n * 8 : 0;
    const size_t off_order = off_lvl + (size_t)grid * ((size_t)n + 1) * 4;
    int rc = sc.open("link load", st, (size_t)grid * per_block, sizeof(hstat));
    if (rc) return rc;
    char* const ws = sc.ws;
    int32_t* const dstat = (int32_t*)sc.dstat;
    SRT_PASS_TRY(hipFuncSetAttribute((const void*)link_load_kernel<true>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SRT_PASS_TRY(hipFuncSetAttribute((const void*)link_load_kernel<false>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if ((rc = span.begin(st)) != SRT_OK) goto out;
    if (sorted)
        link_load_kernel<true><<<grid, LL_THREADS, lds, st>>>(
            n, nrows, srcs, src_begin, pred, hops, ldp, (const ull*)dem, ldd, irp, icol, (ull*)load,
            (ull*)through, (ull*)totals, (int32_t*)(ws + off_order), (uint32_t*)(ws + off_lvl),
            gflow ? (ull*)ws : NULL, (int)(lds / 4), dstat, (uint32_t*)dstat + 1);
    else
        link_load_kernel<false><<<grid, LL_THREADS, lds, st>>>(
            n, nrows, srcs, src_begin, pred, hops, ldp, (const ull*)dem, ldd, irp, icol, (ull*)load,
            (ull*)through, (ull*)totals, (int32_t*)(ws + off_order), (uint32_t*)(ws + off_lvl),
            gflow ? (ull*)ws : NULL, (int)(lds / 4), dstat, (uint32_t*)dstat + 1);
    SRT_PASS_TRY(hipGetLastError());
    rc = span.stop(st); /* the span ends with the kernel, before the stat words travel */
out:
    rc = sc.finish(rc, hstat);
    if (!rc) rc = span.read(&span_ms);
    if (!rc) {
        if (max_hops && hstat[0] > *max_hops) *max_hops = hstat[0];
        if (forms) *forms |= hstat[1];
        if (ms) *ms += span_ms;
    }
    return rc;
}
