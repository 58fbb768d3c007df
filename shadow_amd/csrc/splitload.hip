/*
 * splitload.hip -- link load with every shortest-path tie split evenly, gfx950: the
 * expected traffic per arc and per vertex when each target's predecessor is drawn uniformly from
 * the set M(s, t) of the reliability envelope (envelope.hip).
 *
 * The rule, over the canonical arcs, in integer quanta, D[s][s] taken as 0: M(s, t) is the set of
 * tight in-arcs u -> t (D[s][u] + w(u, t) == D[s][t]) whose D[s][u] is the smallest among the tight
 * ones. With c(s, t) the u64 demand of the pair, for every reachable t != s
 *   inflow_s(t) = sum over v with t in M(s, v) of share_s(v)
 *   f_s(t)      = (double)c(s, t) + inflow_s(t)
 *   share_s(t)  = f_s(t) / (double)|M(s, t)|                       one f64 division
 * and a source adds share_s(t) to load(u -> t) for every u in M(s, t) and inflow_s(t) to
 * through(t). A share that reaches s adds to no through word. The demand totals (routed, unrouted,
 * self) are u64 and exact; an arc or vertex without flow gets no add and stays +0.0.
 *
 * Every member of M(s, t) is strictly nearer to s than t, so the recursion runs from the far end:
 * a target fires once all the targets it is a member of have fired (a children counter per
 * target), which needs no order of the targets by distance. The members form a DAG, not a tree.
 *
 * Like the envelope pass it reads u32 distance rows and an in-arc CSR, whichever build made the
 * rows, and like the load pass a u64 demand row per source; it adds into load (one f64 word per
 * CSR position) and through with f64 atomics in device memory, so two runs may differ in the last
 * bits where the partial sums are not exact.
 */
#include "srt_pass.h"

#include <string.h>

#define SL_THREADS 1024
/* dynamic LDS: the two bitmaps and what the staging form keeps on chip */
#define SL_LDS_BYTES (156 * 1024)
/* in-lists of at least this many arcs are walked by the whole wave, SL_GROUP lists in flight (the
 * route pass's RT_WAVE_ARCS and RT_GROUP) */
#define SL_WAVE_ARCS 32
#define SL_GROUP 4

typedef unsigned long long ull;

/* LDS bytes per 64 targets: the pending and the ready bitmap (8 B each), then per target the f64
 * inflow word and the u32 children counter (form 1) and the u32 distance (forms 1 and 2) */
static int sl_per64(int form) { return 16 + 64 * (form == 1 ? 16 : form == 2 ? 4 : 0); }

/* largest n of staging form 1 (distance row, children counters and inflow words in LDS), 2 (the
 * row in LDS, the counters and inflow words in the workgroup's scratch rows) and 3 (the row read
 * from global memory too, the bitmaps alone in LDS: the pass's own limit) */
extern "C" int srt_split_load_stage_max_n(int form) {
    if (form < 1 || form > 3) return 0;
    return (SL_LDS_BYTES / sl_per64(form)) * 64;
}

#define SL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

/* The words other targets change. FORM 1: LDS. FORM 2, 3: the workgroup's scratch rows, which
 * atomics alone touch -- changed at the memory side, read and written past the L1 (agent-scope
 * atomic loads and stores), as the load pass's form-3 flow words. */
template <int FORM>
struct sl_words {
    uint32_t* kids;
    double* inflow;
    __device__ __forceinline__ void init(int t) const {
        if constexpr (FORM != 1) {
            __hip_atomic_store(kids + t, 0u, SL_RLX_AGENT);
            __hip_atomic_store(inflow + t, 0.0, SL_RLX_AGENT);
        } else {
            kids[t] = 0u;
            inflow[t] = 0.0;
        }
    }
    __device__ __forceinline__ uint32_t kids_of(int t) const {
        if constexpr (FORM != 1) return __hip_atomic_load(kids + t, SL_RLX_AGENT);
        return kids[t];
    }
    __device__ __forceinline__ double inflow_of(int t) const {
        if constexpr (FORM != 1) return __hip_atomic_load(inflow + t, SL_RLX_AGENT);
        return inflow[t];
    }
    __device__ __forceinline__ void kid(int u) const { atomicAdd(kids + u, 1u); }
    /* 1 off u's counter; true when that was its last child */
    __device__ __forceinline__ bool release(int u) const { return atomicSub(kids + u, 1u) == 1u; }
    __device__ __forceinline__ void give(int u, double v) const { atomicAdd(inflow + u, v); }
};

/* The barrier between two steps. FORM 2, 3: the steps meet in scratch words of this workgroup that
 * only atomics touch, so nothing has to leave a cache: each wave waits until its own stores and
 * adds are done, then the barrier (linkload.hip's ll_sync; no agent-scope fence). */
template <int FORM>
static __device__ __forceinline__ void sl_sync() {
    if constexpr (FORM != 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

/* the staged distance of vertex u as u32 quanta (>= SRT_INF: unreachable), the source's own 0 */
template <int FORM>
static __device__ __forceinline__ uint32_t sl_dist(const uint32_t* rowL, const uint32_t* Dr, int s,
                                                   int u) {
    if constexpr (FORM != 3)
        return rowL[u];
    else
        return u == s ? 0u : Dr[u];
}

/* The members of up to SL_GROUP long lists [bj, ej) (empty: bj == ej) walked by the wave, 64 arcs of
 * each a step, the group's loads in flight together: the tight arcs into a target at distance dj
 * whose tail is at distance mj; the member s keeps no counter and no inflow word. !FIRE: 1 more on
 * each member's children counter. FIRE: the firing target's share shj goes to the arc's load word
 * and to the member's inflow word, and 1 comes off the member's counter -- with a zero share too;
 * a member that lost its last child gets its bit in nxt, the next sweep's ready targets. */
template <int FORM, bool FIRE>
static __device__ __forceinline__ void sl_wide_members(
    int s, const uint32_t* rowL, const uint32_t* Dr, const int32_t* __restrict__ icol,
    const uint32_t* __restrict__ iw, const int (&bj)[SL_GROUP], const int (&ej)[SL_GROUP],
    const uint32_t (&dj)[SL_GROUP], const uint32_t (&mj)[SL_GROUP], const double (&shj)[SL_GROUP],
    int span, const sl_words<FORM> W, double* load, ull* nxt) {
    const int lane = threadIdx.x & 63;
    for (int c = lane; c - lane < span; c += 64) {
        int u[SL_GROUP], kk[SL_GROUP];
        uint32_t wv[SL_GROUP];
        bool in[SL_GROUP];
#pragma unroll
        for (int j = 0; j < SL_GROUP; ++j) {
            in[j] = bj[j] + c < ej[j];
            kk[j] = in[j] ? bj[j] + c : 0;
            u[j] = icol[kk[j]];
            wv[j] = iw[kk[j]];
        }
#pragma unroll
        for (int j = 0; j < SL_GROUP; ++j) {
            const uint32_t du = sl_dist<FORM>(rowL, Dr, s, u[j]);
            if (in[j] && du == mj[j] && du + wv[j] == dj[j]) {
                if constexpr (FIRE) {
                    if (shj[j] > 0.0) {
                        atomicAdd(load + kk[j], shj[j]);
                        if (u[j] != s) W.give(u[j], shj[j]);
                    }
                    if (u[j] != s && W.release(u[j]))
                        atomicOr(nxt + (u[j] >> 6), 1ull << (u[j] & 63));
                } else if (u[j] != s) {
                    W.kid(u[j]);
                }
            }
        }
    }
}

/* Phase A over the row's targets, targets across the lanes: each reachable t != s walks its
 * in-list once for the smallest tight D[s][u] and |M| (lists of SL_WAVE_ARCS arcs or more by the
 * whole wave, SL_GROUP lists at a time: rt_pred_phase's pattern), keeps both in the block's
 * scratch (dminS, cntS: read and written by the target's own lane alone) and, with `kids`, walks it
 * once more to add 1 to the children counter of every member. The words of the bitmaps that cover
 * targets t0 .. t0 + 63 belong to one wave. Returns the lane's targets with |M| >= 2. */
template <int FORM>
static __device__ int sl_members(int n, int s, bool kids, const uint32_t* rowL, const uint32_t* Dr,
                                 const int32_t* __restrict__ irp, const int32_t* __restrict__ icol,
                                 const uint32_t* __restrict__ iw, uint32_t* dminS, uint32_t* cntS,
                                 ull* pend, ull* rdy, const sl_words<FORM> W) {
    const int tid = threadIdx.x, lane = tid & 63;
    int tied = 0;
    for (int t0 = tid & ~63; t0 < n; t0 += SL_THREADS) { /* wave-uniform trip count */
        const int t = t0 + lane;
        int kb = 0, ke = 0;
        uint32_t dt = SRT_INF, dmin = ~0u, cnt = 0u;
        bool live = false, wide = false;
        if (t < n && t != s) {
            dt = sl_dist<FORM>(rowL, Dr, s, t);
            live = dt < SRT_INF;
        }
        if (live) {
            kb = irp[t];
            ke = irp[t + 1];
            wide = ke - kb >= SL_WAVE_ARCS;
            if (!wide)
                for (int k = kb; k < ke; ++k) {
                    const uint32_t du = sl_dist<FORM>(rowL, Dr, s, icol[k]);
                    if (du < SRT_INF && du + iw[k] == dt && du <= dmin) {
                        cnt = du < dmin ? 1u : cnt + 1u;
                        dmin = du;
                    }
                }
        }
        /* ---- the wide lists, SL_GROUP at a time ------------------------------------------ */
        ull m = __ballot(wide);
        while (m) {
            int lj[SL_GROUP], bj[SL_GROUP], ej[SL_GROUP], span = 0;
            uint32_t dj[SL_GROUP], best[SL_GROUP], num[SL_GROUP];
#pragma unroll
            for (int j = 0; j < SL_GROUP; ++j) {
                const int l = m ? __ffsll(m) - 1 : -1; /* -1: the slot stays empty */
                m &= m - 1ull;
                lj[j] = l;
                bj[j] = __shfl(kb, l < 0 ? 0 : l);
                ej[j] = l < 0 ? bj[j] : __shfl(ke, l);
                dj[j] = (uint32_t)__shfl((int)dt, l < 0 ? 0 : l);
                best[j] = ~0u;
                num[j] = 0u;
                span = ej[j] - bj[j] > span ? ej[j] - bj[j] : span;
            }
            for (int c = lane; c - lane < span; c += 64) {
                int u[SL_GROUP];
                uint32_t wv[SL_GROUP];
                bool in[SL_GROUP];
#pragma unroll
                for (int j = 0; j < SL_GROUP; ++j) {
                    in[j] = bj[j] + c < ej[j];
                    const int k = in[j] ? bj[j] + c : 0;
                    u[j] = icol[k];
                    wv[j] = iw[k];
                }
#pragma unroll
                for (int j = 0; j < SL_GROUP; ++j) {
                    const uint32_t du = sl_dist<FORM>(rowL, Dr, s, u[j]);
                    if (in[j] && du < SRT_INF && du + wv[j] == dj[j] && du <= best[j]) {
                        num[j] = du < best[j] ? 1u : num[j] + 1u;
                        best[j] = du;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < SL_GROUP; ++j) {
                uint32_t g = best[j];
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)g, off);
                    g = o < g ? o : g;
                }
                uint32_t c = best[j] == g ? num[j] : 0u;
                for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
                if (lane == lj[j]) {
                    dmin = g;
                    cnt = g == ~0u ? 0u : c;
                }
                best[j] = g; /* wave-uniform from here on */
                if (g == ~0u) ej[j] = bj[j];
            }
            /* the members' children counters, the same lists again (they are in the cache) */
            if (kids) { /* block-uniform */
                const double none[SL_GROUP] = {0.0, 0.0, 0.0, 0.0};
                sl_wide_members<FORM, false>(s, rowL, Dr, icol, iw, bj, ej, dj, best, none, span, W,
                                             NULL, NULL);
            }
        }
        /* a reachable target without a tight arc (rows that are no distances of these arcs) is
         * left out like an unreachable one */
        live = live && cnt > 0u;
        if (live) {
            dminS[t] = dmin;
            cntS[t] = cnt;
            tied += cnt >= 2u;
        } else if (t < n) {
            cntS[t] = 0u; /* never fires, even where a malformed row names it a member */
        }
        const ull lm = __ballot(live);
        if (lane == 0) {
            pend[t0 >> 6] = lm;
            rdy[t0 >> 6] = 0ull;
        }
        /* ---- the members' children counters of the short lists ---------------------------- */
        if (kids && live && !wide)
            for (int k = kb; k < ke; ++k) {
                const int u = icol[k];
                const uint32_t du = sl_dist<FORM>(rowL, Dr, s, u);
                if (u != s && du == dmin && du + iw[k] == dt) W.kid(u);
            }
    }
    return tied;
}

/* The first sweep's ready targets: the live targets (pend) that are nobody's member. Leaves rdy
 * with their bits and pend all zero: the two bitmaps then take turns as this sweep's ready
 * targets and the next one's. Returns whether a target of this thread's wave is ready. */
template <int FORM>
static __device__ bool sl_first(int n, ull* pend, ull* rdy, const sl_words<FORM> W) {
    const int tid = threadIdx.x, lane = tid & 63;
    bool any = false;
    for (int t0 = tid & ~63; t0 < n; t0 += SL_THREADS) {
        const ull pw = pend[t0 >> 6];
        if (!pw) continue;
        const bool ready = ((pw >> lane) & 1ull) && W.kids_of(t0 + lane) == 0u;
        const ull rm = __ballot(ready);
        if (lane == 0) {
            rdy[t0 >> 6] = rm;
            pend[t0 >> 6] = 0ull;
        }
        any = any || rm != 0ull;
    }
    return any;
}

/* A sweep: every ready target (cur) forms its share, walks its members again, adds the share to
 * the member's inflow word (unless the member is s) and to the arc's load word, and takes 1 off
 * the member's counter -- with f == 0 too, or its ancestors never fire; the decrement that takes a
 * counter to 0 sets the member's bit in nxt (an LDS atomic), which is read behind the sweep's
 * barrier, when every add into the member's inflow word is done. Its own inflow goes to through.
 * The words of cur belong to waves, which clear them. Lists of SL_WAVE_ARCS arcs or more are
 * walked by the wave, SL_GROUP in flight. */
template <int FORM>
static __device__ void sl_fire(int n, int s, const uint32_t* rowL, const uint32_t* Dr,
                               const ull* __restrict__ C, const int32_t* __restrict__ irp,
                               const int32_t* __restrict__ icol, const uint32_t* __restrict__ iw,
                               const uint32_t* dminS, const uint32_t* cntS, ull* cur, ull* nxt,
                               const sl_words<FORM> W, double* load, double* through) {
    const int tid = threadIdx.x, lane = tid & 63;
    for (int t0 = tid & ~63; t0 < n; t0 += SL_THREADS) {
        const ull rm = cur[t0 >> 6];
        if (!rm) continue;
        const int t = t0 + lane;
        const uint32_t cnt = (rm >> lane) & 1ull ? cntS[t] : 0u;
        const bool ready = cnt > 0u;
        int kb = 0, ke = 0;
        uint32_t dt = 0u, dmin = 0u;
        double share = 0.0;
        bool wide = false;
        if (ready) {
            const double in = W.inflow_of(t);
            share = ((double)C[t] + in) / (double)cnt;
            if (in > 0.0) atomicAdd(through + t, in);
            dt = sl_dist<FORM>(rowL, Dr, s, t);
            dmin = dminS[t];
            kb = irp[t];
            ke = irp[t + 1];
            wide = ke - kb >= SL_WAVE_ARCS;
            if (!wide)
                for (int k = kb; k < ke; ++k) {
                    const int u = icol[k];
                    const uint32_t du = sl_dist<FORM>(rowL, Dr, s, u);
                    if (du == dmin && du + iw[k] == dt) {
                        if (share > 0.0) {
                            atomicAdd(load + k, share);
                            if (u != s) W.give(u, share);
                        }
                        if (u != s && W.release(u)) atomicOr(nxt + (u >> 6), 1ull << (u & 63));
                    }
                }
        }
        ull m = __ballot(wide);
        while (m) {
            int bj[SL_GROUP], ej[SL_GROUP], span = 0;
            uint32_t dj[SL_GROUP], mj[SL_GROUP];
            double shj[SL_GROUP];
#pragma unroll
            for (int j = 0; j < SL_GROUP; ++j) {
                const int l = m ? __ffsll(m) - 1 : -1; /* -1: the slot stays empty */
                m &= m - 1ull;
                bj[j] = __shfl(kb, l < 0 ? 0 : l);
                ej[j] = l < 0 ? bj[j] : __shfl(ke, l);
                dj[j] = (uint32_t)__shfl((int)dt, l < 0 ? 0 : l);
                mj[j] = (uint32_t)__shfl((int)dmin, l < 0 ? 0 : l);
                shj[j] = __shfl(share, l < 0 ? 0 : l);
                span = ej[j] - bj[j] > span ? ej[j] - bj[j] : span;
            }
            sl_wide_members<FORM, true>(s, rowL, Dr, icol, iw, bj, ej, dj, mj, shj, span, W, load,
                                        nxt);
        }
        if (lane == 0) cur[t0 >> 6] = 0ull;
    }
}

/* One workgroup per source row (persistent grid). Row r belongs to source s = srcs[r] (or
 * src_begin + r); its distances are row s (by_src) or row r of D, its demand row r of dem (stride
 * ldc). Scratch per workgroup: dmin and |M| of every target (n u32 each) and, FORM 2 and 3, the
 * children counters (n u32) and the inflow words (n f64). Phase A once, then sweeps from the far
 * end, a barrier after each and one more around the "any target ready?" word -- a target fires in
 * the sweep after the last target it is a member of, so the sweeps number the longest chain of
 * members. Workgroup-scope ordering throughout. A row without routed demand is only counted (tied
 * pairs). totals: routed, unrouted, self. */
template <int FORM>
__global__ __launch_bounds__(SL_THREADS) void split_load_kernel(
    int n, int nrows, const int32_t* __restrict__ srcs, int src_begin, int by_src,
    const uint32_t* __restrict__ D, size_t ldd, const ull* __restrict__ dem, size_t ldc,
    const int32_t* __restrict__ irp, const int32_t* __restrict__ icol,
    const uint32_t* __restrict__ iw, double* load, double* through, ull* totals, uint32_t* ws_dmin,
    uint32_t* ws_cnt, uint32_t* ws_kids, double* ws_inflow, ull* tied_pairs, int32_t* max_sweeps,
    uint32_t* forms) {
    extern __shared__ ull sl_lds[];
    __shared__ ull s_red[SL_THREADS / 64][3];
    __shared__ int s_tied;
    __shared__ int s_any[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nw = (n + 63) >> 6;
    ull* pend = sl_lds;
    ull* rdy = pend + nw;
    sl_words<FORM> W;
    uint32_t* rowL = NULL;
    if constexpr (FORM == 1) {
        W.inflow = (double*)(rdy + nw);
        W.kids = (uint32_t*)(W.inflow + n);
        rowL = W.kids + n;
    } else {
        W.kids = ws_kids + (size_t)blockIdx.x * n;
        W.inflow = ws_inflow + (size_t)blockIdx.x * n;
        rowL = (uint32_t*)(rdy + nw);
    }
    uint32_t* dminS = ws_dmin + (size_t)blockIdx.x * n;
    uint32_t* cntS = ws_cnt + (size_t)blockIdx.x * n;
    ull tot[3] = {0ull, 0ull, 0ull}, tied_all = 0ull; /* thread 0: the block's rows */
    int sweeps_max = 0;
    bool ran = false;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int s = srcs ? srcs[r] : src_begin + r;
        if (s < 0 || s >= n) continue; /* not a vertex (block-uniform): the row is left alone */
        const uint32_t* Dr = D + (size_t)(by_src ? s : r) * ldd;
        const ull* C = dem + (size_t)r * ldc;
        ran = true;
        /* ---- stage the row; the row's demand totals -------------------------------------- */
        ull a[3] = {0ull, 0ull, 0ull};
        if (tid == 0) s_tied = 0;
        if (tid < 2) s_any[tid] = 0;
        for (int t = tid; t < n; t += SL_THREADS) {
            const uint32_t d = t == s ? 0u : Dr[t];
            if constexpr (FORM != 3) rowL[t] = d;
            W.init(t);
            const ull c = C[t];
            a[0] += t != s && d < SRT_INF ? c : 0ull;
            a[1] += t != s && d >= SRT_INF ? c : 0ull;
            a[2] += t == s ? c : 0ull;
        }
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j) a[j] += __shfl_xor(a[j], off);
        }
        if (lane == 0) {
            s_red[wave][0] = a[0];
            s_red[wave][1] = a[1];
            s_red[wave][2] = a[2];
        }
        sl_sync<FORM>();
        ull routed = 0ull;
        for (int w = 0; w < SL_THREADS / 64; ++w) {
            routed += s_red[w][0];
            tot[1] += s_red[w][1];
            tot[2] += s_red[w][2];
        }
        tot[0] += routed;
        /* ---- phase A ---------------------------------------------------------------------- */
        int tied = sl_members<FORM>(n, s, routed != 0ull, rowL, Dr, irp, icol, iw, dminS, cntS, pend,
                                    rdy, W);
        for (int off = 32; off > 0; off >>= 1) tied += __shfl_xor(tied, off);
        if (lane == 0 && tied) atomicAdd(&s_tied, tied);
        sl_sync<FORM>();
        tied_all += (ull)s_tied;
        /* ---- phase B: sweeps from the far end -------------------------------------------- */
        int sweeps = 0;
        if (routed != 0ull) { /* block-uniform */
            ull *cur = rdy, *nxt = pend;
            bool any = sl_first<FORM>(n, pend, rdy, W);
            for (;; ++sweeps) {
                if (any) s_any[sweeps & 1] = 1;
                __syncthreads();
                if (!s_any[sweeps & 1]) break;
                if (tid == 0) s_any[(sweeps + 1) & 1] = 0;
                sl_fire<FORM>(n, s, rowL, Dr, C, irp, icol, iw, dminS, cntS, cur, nxt, W, load,
                              through);
                sl_sync<FORM>();
                ull* const was = cur;
                cur = nxt;
                nxt = was; /* all zero: every word of it that held a bit was cleared */
                any = false;
                for (int w = tid; w < nw; w += SL_THREADS) any = any || cur[w] != 0ull;
            }
        }
        sweeps_max = sweeps > sweeps_max ? sweeps : sweeps_max;
        __syncthreads(); /* s_red, s_tied and s_any are set again by the next row */
    }
    if (tid == 0 && ran) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (tot[j]) atomicAdd(totals + j, tot[j]);
        if (tied_all) atomicAdd(tied_pairs, tied_all);
        srt_max_once(max_sweeps, sweeps_max);
        atomicOr(forms, 1u << (FORM - 1));
    }
}

template <int FORM>
static hipError_t sl_launch(int grid, size_t lds, hipStream_t st, int n, int nrows,
                            const int32_t* srcs, int src_begin, int by_src, const uint32_t* D,
                            size_t ldd, const ull* dem, size_t ldc, const int32_t* irp,
                            const int32_t* icol, const uint32_t* iw, double* load, double* through,
                            ull* totals, uint32_t* ws_dmin, uint32_t* ws_cnt, uint32_t* ws_kids,
                            double* ws_inflow, ull* dstat) {
    const hipError_t e = hipFuncSetAttribute((const void*)split_load_kernel<FORM>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    split_load_kernel<FORM><<<grid, SL_THREADS, lds, st>>>(
        n, nrows, srcs, src_begin, by_src, D, ldd, dem, ldc, irp, icol, iw, load, through, totals,
        ws_dmin, ws_cnt, ws_kids, ws_inflow, dstat, (int32_t*)(dstat + 1), (uint32_t*)(dstat + 1) + 1);
    return hipGetLastError();
}

/* The split-load pass over nrows distance rows (see split_load_kernel): ADDS into load (one f64
 * word per CSR position), through (n) and totals (routed, unrouted, self; the caller zeroes
 * them). Adds the HIP-event time, the tied pairs, the sweeps and the staging forms to *stats (the
 * caller zeroes it); returns after the stream. */
int srt_split_load_rows(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                        const uint32_t* D, size_t ldd, const uint64_t* dem, size_t ldc,
                        const int32_t* irp, const int32_t* icol, const uint32_t* iw, double* load,
                        double* through, uint64_t* totals, hipStream_t st,
                        srt_split_load_stats* stats) {
    if (nrows <= 0) return SRT_OK;
    if (n < 1 || !D || !dem || !irp || !icol || !iw || !load || !through || !totals ||
        ldd < (size_t)n || ldc < (size_t)n) {
        srt_set_error("split load: bad arguments (n = %d, ldd = %zu, ldc = %zu)", n, ldd, ldc);
        return SRT_E_ARG;
    }
    if (n > srt_split_load_stage_max_n(3)) {
        srt_set_error("split load: n = %d beyond its range (%d)", n, srt_split_load_stage_max_n(3));
        return SRT_E_RANGE;
    }
    const int form = n <= srt_split_load_stage_max_n(1) ? 1 : n <= srt_split_load_stage_max_n(2) ? 2 : 3;
    const size_t nw = (size_t)srt_ceil_div(n, 64);
    const size_t lds = nw * 16 + (size_t)n * (form == 1 ? 16 : form == 2 ? 4 : 0);
    /* per workgroup: dmin and |M| (n u32 each); forms 2 and 3: the inflow words (n f64: first,
     * aligned) and the children counters (n u32); the grid shrinks to fit */
    const size_t per_block = (size_t)n * (8 + (form != 1 ? 12 : 0));
    /* one workgroup a CU: the kernel takes 128 VGPRs, so its 16 waves fill the CU's four SIMDs
     * (4 waves each) whatever LDS is left; a second one would only queue and double the scratch */
    const int grid = srt_pass_grid(lds, per_block, nrows, true);
    srt_pass_scratch sc;
    ull hstat[2] = {0, 0}; /* the tied pairs, then max_sweeps and forms (32 bits each) */
    double* ws_inflow = NULL;
    uint32_t *ws_dmin = NULL, *ws_cnt = NULL, *ws_kids = NULL;
    double ms = 0;
    hipError_t le = hipSuccess;
    srt_event_span span;
    int rc = span.begin(st);
    if (rc) return rc;
    rc = sc.open("split load", st, (size_t)grid * per_block, sizeof(hstat));
    if (rc) return rc;
    ull* const dstat = (ull*)sc.dstat;
    {
        char* p = sc.ws;
        if (form != 1) {
            ws_inflow = (double*)p;
            p += (size_t)grid * n * 8;
            ws_kids = (uint32_t*)p;
            p += (size_t)grid * n * 4;
        }
        ws_dmin = (uint32_t*)p;
        ws_cnt = ws_dmin + (size_t)grid * n;
    }
#define SL_ARGS                                                                                    \
    grid, lds, st, n, nrows, srcs, src_begin, by_src, D, ldd, (const ull*)dem, ldc, irp, icol, iw, \
        load, through, (ull*)totals, ws_dmin, ws_cnt, ws_kids, ws_inflow, dstat
    le = form == 1 ? sl_launch<1>(SL_ARGS) : form == 2 ? sl_launch<2>(SL_ARGS) : sl_launch<3>(SL_ARGS);
#undef SL_ARGS
    SRT_PASS_TRY(le);
out:
    rc = sc.finish(rc, hstat);
    if (!rc) rc = span.end(st, &ms);
    if (!rc && stats) {
        const int32_t sweeps = (int32_t)(uint32_t)hstat[1];
        stats->ms_split += ms;
        stats->tied_pairs += (int64_t)hstat[0];
        stats->max_sweeps = sweeps > stats->max_sweeps ? sweeps : stats->max_sweeps;
        stats->forms |= (int32_t)(hstat[1] >> 32);
    }
    return rc;
}
