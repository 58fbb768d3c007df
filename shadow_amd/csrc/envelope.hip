/*
 * envelope.hip -- the reliability bounds of every pair over every shortest-path tie order, gfx950
 * (DESIGN §5.12).
 *
 * Reference: src/main/routing/topology.c:1682-1699 (the Dijkstra behind the paths
 * updates a parent on a strictly smaller distance only, so the predecessor of t is the first tight
 * in-neighbour popped from the heap: one of those with the smallest D[s][u], the heap order
 * deciding among equals), :1309 and :1365 (the reliability of a path is the left-to-right product
 * of its arcs' reliabilities).
 *
 * The rule, over the canonical arcs, in integer quanta, D[s][s] taken as 0: M(s, t) is the set of
 * tight in-arcs u -> t (D[s][u] + w(u, t) == D[s][t]) whose D[s][u] is the smallest among the tight
 * ones; a feasible path takes every vertex's predecessor from that vertex's own M. Then
 *   hi(s, t) = max over u in M(s, t) of hi(s, u) * r(u, t)
 *   lo(s, t) = min over u in M(s, t) of lo(s, u) * r(u, t),   hi(s, s) = lo(s, s) = 1.0
 * one f64 multiply each. Multiplication by r >= 0 is monotone in f64, so these are bit for bit the
 * largest and the smallest left-to-right product over all feasible paths. Unreachable t: 0.0 / 0.0.
 * Per call the pass counts the pairs with |M| >= 2 (tied), those whose path depends on the heap
 * order (exposed: tied, or some member of M exposed) and those with lo != hi (sensitive).
 *
 * Like the route pass it reads u32 distance rows and an in-arc CSR (here with the arcs'
 * reliabilities), whichever build made the rows; the front ends are the same two.
 */
#include "srt_pass.h"

#include <string.h>

#define EV_THREADS 1024
/* dynamic LDS: the staged row (form 1) and the three bitmaps */
#define EV_LDS_BYTES (156 * 1024)
/* in-lists of at least this many arcs are walked by the whole wave, EV_GROUP lists in flight (the
 * route pass's RT_WAVE_ARCS and RT_GROUP) */
#define EV_WAVE_ARCS 32
#define EV_GROUP 4

/* the bitmaps (done, fresh, exposed): one 64-bit word per 64 targets each */
static size_t ev_bitmap_bytes(int n) { return 3 * (size_t)srt_ceil_div(n, 64) * 8; }

/* largest n of staging form 1 (u32 row in LDS beside the bitmaps) and 3 (row read from global
 * memory, the bitmaps alone in LDS: the pass's own limit); there is no form 2 */
extern "C" int srt_envelope_stage_max_n(int form) {
    if (form == 1) {
        const int per64 = 64 * 4 + 24, full = EV_LDS_BYTES / per64, rest = EV_LDS_BYTES - full * per64;
        return full * 64 + (rest > 24 ? (rest - 24) / 4 : 0);
    }
    return form == 3 ? (EV_LDS_BYTES / 24) * 64 : 0;
}

static __device__ __forceinline__ double ld_wg(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ void st_wg(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/* the staged distance of vertex u as u32 quanta (>= SRT_INF: unreachable), the source's own 0 */
template <int FORM>
static __device__ __forceinline__ uint32_t ev_dist(const uint32_t* rowL, const uint32_t* Dr, int s,
                                                   int u) {
    if constexpr (FORM == 1)
        return rowL[u];
    else
        return u == s ? 0u : Dr[u];
}

static __device__ __forceinline__ bool ev_bit(const unsigned long long* bm, int u) {
    return (((const uint32_t*)bm)[u >> 5] >> (u & 31)) & 1u;
}

/* what the members of M give a target: the bounds, how many they are, whether one is exposed */
struct ev_acc {
    double lo, hi;
    int cnt;
    bool exp;
};

/* One sweep over the pending targets of a row, targets across the lanes. A pending target walks
 * its in-list for the smallest tight D[s][u] and whether every member of M is done (pass A: the
 * staged distances and the done bitmap only); one that is ready walks it once more and gathers
 * its members' lo and hi from the output rows (pass B: once per target over the whole pass).
 * Lists of EV_WAVE_ARCS arcs or more take both passes with the whole wave, pass A EV_GROUP lists at
 * a time (rt_pred_phase's pattern). A target that is not ready leaves one open member of its M in
 * hint[t] (the block's scratch, read and written by the target's own lane alone) and walks again
 * only once that member is done: most sweeps cost a pending target one coalesced word and one
 * bit. The words of a bitmap that cover targets t0 .. t0 + 63 belong to one wave: it alone writes
 * them, from its ballots. Returns whether a target resolved; adds to cnt (tied, exposed,
 * sensitive). icol[0] and iw[0] must be readable. */
template <int FORM>
static __device__ bool ev_sweep(int n, int s, const uint32_t* rowL, const uint32_t* Dr,
                                const int32_t* __restrict__ irp, const int32_t* __restrict__ icol,
                                const uint32_t* __restrict__ iw, const double* __restrict__ ir,
                                double* LO, double* HI, int32_t* hint,
                                const unsigned long long* done, unsigned long long* fresh,
                                unsigned long long* expo, int cnt[3]) {
    const int tid = threadIdx.x, lane = tid & 63;
    bool any = false;
    for (int t0 = tid & ~63; t0 < n; t0 += EV_THREADS) { /* wave-uniform trip count */
        const unsigned long long dw = done[t0 >> 6];
        if (dw == ~0ull) continue;
        const int t = t0 + lane;
        bool pend = !((dw >> lane) & 1ull); /* the bits past n are set */
        if (pend) { /* still waiting for the member it met open? */
            const int h = hint[t];
            pend = h < 0 || ev_bit(done, h);
        }
        int kb = 0, ke = 0, ob = -1; /* ob: an open member of M, -1 when there is none */
        uint32_t dt = 0u, dmin = ~0u;
        bool wide = false, ready = false;
        if (pend) {
            dt = ev_dist<FORM>(rowL, Dr, s, t);
            kb = irp[t];
            ke = irp[t + 1];
            wide = ke - kb >= EV_WAVE_ARCS;
            if (!wide) {
                for (int k = kb; k < ke; ++k) {
                    const int u = icol[k];
                    const uint32_t du = ev_dist<FORM>(rowL, Dr, s, u);
                    if (du < SRT_INF && du + iw[k] == dt && du <= dmin) {
                        const int o = ev_bit(done, u) ? -1 : u;
                        ob = du < dmin || ob < 0 ? o : ob;
                        dmin = du;
                    }
                }
                ready = dmin != ~0u && ob < 0;
            }
        }
        /* ---- pass A of the wide lists, EV_GROUP at a time --------------------------------- */
        unsigned long long m = __ballot(wide);
        while (m) {
            int lj[EV_GROUP], bj[EV_GROUP], ej[EV_GROUP], span = 0;
            uint32_t dj[EV_GROUP], best[EV_GROUP];
            int open[EV_GROUP]; /* this lane's open member at best[j], -1: none */
#pragma unroll
            for (int j = 0; j < EV_GROUP; ++j) {
                const int l = m ? __ffsll(m) - 1 : -1; /* -1: the slot stays empty */
                m &= m - 1ull;
                lj[j] = l;
                bj[j] = __shfl(kb, l < 0 ? 0 : l);
                ej[j] = l < 0 ? bj[j] : __shfl(ke, l);
                dj[j] = (uint32_t)__shfl((int)dt, l < 0 ? 0 : l);
                best[j] = ~0u;
                open[j] = -1;
                span = ej[j] - bj[j] > span ? ej[j] - bj[j] : span;
            }
            for (int c = lane; c - lane < span; c += 64) {
                int u[EV_GROUP];
                uint32_t wv[EV_GROUP];
                bool in[EV_GROUP];
#pragma unroll
                for (int j = 0; j < EV_GROUP; ++j) {
                    in[j] = bj[j] + c < ej[j];
                    const int k = in[j] ? bj[j] + c : 0;
                    u[j] = icol[k];
                    wv[j] = iw[k];
                }
#pragma unroll
                for (int j = 0; j < EV_GROUP; ++j) {
                    const uint32_t du = ev_dist<FORM>(rowL, Dr, s, u[j]);
                    if (in[j] && du < SRT_INF && du + wv[j] == dj[j] && du <= best[j]) {
                        const int o = ev_bit(done, u[j]) ? -1 : u[j];
                        open[j] = du < best[j] || open[j] < 0 ? o : open[j];
                        best[j] = du;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < EV_GROUP; ++j) {
                uint32_t g = best[j];
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)g, off);
                    g = o < g ? o : g;
                }
                const unsigned long long stuck = __ballot(open[j] >= 0 && best[j] == g);
                const int o = __shfl(open[j], stuck ? __ffsll(stuck) - 1 : 0);
                if (lane == lj[j]) {
                    dmin = g;
                    ob = stuck ? o : -1;
                    ready = g != ~0u && !stuck;
                }
            }
        }
        /* ---- pass B: the ready targets gather their members ------------------------------- */
        ev_acc a = {0.0, 0.0, 0, false};
        if (ready && !wide) {
            for (int k = kb; k < ke; ++k) {
                const int u = icol[k];
                const uint32_t du = ev_dist<FORM>(rowL, Dr, s, u);
                if (du == dmin && du + iw[k] == dt) {
                    const double r = ir[k], l = ld_wg(LO + u) * r, h = ld_wg(HI + u) * r;
                    a.lo = !a.cnt || l < a.lo ? l : a.lo;
                    a.hi = !a.cnt || h > a.hi ? h : a.hi;
                    a.exp = a.exp || ev_bit(expo, u);
                    ++a.cnt;
                }
            }
        }
        m = __ballot(ready && wide);
        while (m) {
            const int l = __ffsll(m) - 1;
            m &= m - 1ull;
            const int b = __shfl(kb, l), e = __shfl(ke, l);
            const uint32_t d = (uint32_t)__shfl((int)dt, l), dm = (uint32_t)__shfl((int)dmin, l);
            ev_acc x = {0.0, 0.0, 0, false};
            for (int k = b + lane; k < e; k += 64) {
                const int u = icol[k];
                const uint32_t du = ev_dist<FORM>(rowL, Dr, s, u);
                if (du == dm && du + iw[k] == d) {
                    const double r = ir[k], lw = ld_wg(LO + u) * r, h = ld_wg(HI + u) * r;
                    x.lo = !x.cnt || lw < x.lo ? lw : x.lo;
                    x.hi = !x.cnt || h > x.hi ? h : x.hi;
                    x.exp = x.exp || ev_bit(expo, u);
                    ++x.cnt;
                }
            }
            for (int off = 32; off > 0; off >>= 1) {
                const double ol = __shfl_xor(x.lo, off), oh = __shfl_xor(x.hi, off);
                const int oc = __shfl_xor(x.cnt, off);
                x.lo = oc && (!x.cnt || ol < x.lo) ? ol : x.lo;
                x.hi = oc && (!x.cnt || oh > x.hi) ? oh : x.hi;
                x.cnt += oc;
            }
            x.exp = __ballot(x.exp) != 0ull;
            if (lane == l) a = x;
        }
        if (pend && !ready) hint[t] = ob; /* -1 (no tight arc at all): walks again */
        if (ready) {
            st_wg(LO + t, a.lo);
            st_wg(HI + t, a.hi);
            a.exp = a.exp || a.cnt >= 2;
            cnt[0] += a.cnt >= 2;
            cnt[1] += a.exp;
            cnt[2] += __double_as_longlong(a.lo) != __double_as_longlong(a.hi);
        }
        const unsigned long long fm = __ballot(ready), em = __ballot(ready && a.exp);
        if (lane == 0 && fm) {
            fresh[t0 >> 6] = fm;
            if (em) expo[t0 >> 6] |= em;
        }
        any = any || fm != 0ull;
    }
    return any;
}

/* One workgroup per source row (persistent grid). Row r belongs to source s = srcs[r] (or
 * src_begin + r); its distances are row s (by_src) or row r of D. FORM 1: the row as u32 in LDS;
 * FORM 3: read from global memory. LO, HI: the output rows, which are the pass's only f64 state
 * (16 B per target do not fit on chip), or the block's scratch rows where an output is NULL;
 * hint: the block's scratch row of ev_sweep.
 * Sweeps to a fixed point: a target resolves in the sweep after the last member of its M has, so
 * the sweeps number the longest feasible chain. What a sweep writes is read from the next one on
 * (done |= fresh behind a barrier), workgroup-scope ordering throughout. */
template <int FORM>
__global__ __launch_bounds__(EV_THREADS) void envelope_kernel(
    int n, int nrows, const int32_t* __restrict__ srcs, int src_begin, int by_src,
    const uint32_t* __restrict__ D, size_t ldd, const int32_t* __restrict__ irp,
    const int32_t* __restrict__ icol, const uint32_t* __restrict__ iw,
    const double* __restrict__ ir, double* lo, double* hi, size_t ldo, double* ws_lo, double* ws_hi,
    int32_t* ws_hint, unsigned long long* counts, int32_t* max_sweeps, uint32_t* forms) {
    extern __shared__ unsigned long long ev_lds[];
    __shared__ int s_any;
    __shared__ int s_cnt[3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (n + 63) >> 6;
    unsigned long long* done = ev_lds;
    unsigned long long* fresh = done + nw;
    unsigned long long* expo = fresh + nw;
    const uint32_t* rowL = (const uint32_t*)(expo + nw);
    int sweeps_max = 0;
    bool ran = false;
    for (int r = blockIdx.x; r < nrows; r += gridDim.x) {
        const int s = srcs ? srcs[r] : src_begin + r;
        if (s < 0 || s >= n) continue; /* not a vertex (block-uniform): the row is left alone */
        const uint32_t* Dr = D + (size_t)(by_src ? s : r) * ldd;
        double* LO = lo ? lo + (size_t)r * ldo : ws_lo + (size_t)blockIdx.x * n;
        double* HI = hi ? hi + (size_t)r * ldo : ws_hi + (size_t)blockIdx.x * n;
        int32_t* hint = ws_hint + (size_t)blockIdx.x * n;
        ran = true;
        /* ---- stage the row; s and the unreachable targets are done from the start ------- */
        if (tid < 3) s_cnt[tid] = 0;
        for (int t0 = tid & ~63; t0 < n; t0 += EV_THREADS) {
            const int t = t0 + lane;
            bool fin = true;
            if (t < n) {
                const uint32_t d = t == s ? 0u : Dr[t];
                if constexpr (FORM == 1) ((uint32_t*)rowL)[t] = d;
                fin = t == s || d >= SRT_INF;
                hint[t] = -1;
                if (fin) {
                    st_wg(LO + t, t == s ? 1.0 : 0.0);
                    st_wg(HI + t, t == s ? 1.0 : 0.0);
                }
            }
            const unsigned long long fm = __ballot(fin);
            if (lane == 0) {
                done[t0 >> 6] = fm;
                fresh[t0 >> 6] = 0ull;
                expo[t0 >> 6] = 0ull;
            }
        }
        __threadfence_block();
        __syncthreads();
        int cnt[3] = {0, 0, 0}, sweeps = 0;
        for (;;) {
            if (tid == 0) s_any = 0;
            __syncthreads();
            if (ev_sweep<FORM>(n, s, rowL, Dr, irp, icol, iw, ir, LO, HI, hint, done, fresh, expo, cnt))
                s_any = 1;
            __threadfence_block();
            __syncthreads();
            if (!s_any) break;
            ++sweeps;
            for (int w = tid; w < nw; w += EV_THREADS) {
                done[w] |= fresh[w];
                fresh[w] = 0ull;
            }
            __syncthreads();
        }
        /* rows that are no shortest-path distances of these arcs leave targets behind: no path */
        for (int t = tid; t < n; t += EV_THREADS)
            if (!((done[t >> 6] >> (t & 63)) & 1ull)) {
                LO[t] = 0.0;
                HI[t] = 0.0;
            }
        sweeps_max = sweeps > sweeps_max ? sweeps : sweeps_max;
        /* ---- the row's counts: one 64-bit atomic each -------------------------------------- */
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            int c = cnt[i];
            for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
            if (lane == 0 && c) atomicAdd(&s_cnt[i], c);
        }
        __syncthreads();
        if (tid < 3 && s_cnt[tid]) atomicAdd(counts + tid, (unsigned long long)s_cnt[tid]);
        __syncthreads();
    }
    if (tid == 0 && ran) {
        srt_max_once(max_sweeps, sweeps_max);
        atomicOr(forms, 1u << (FORM - 1));
    }
}

/* The envelope pass over nrows distance rows (see envelope_kernel); either output may be NULL.
 * Adds the HIP-event time, the counts, the sweeps and the staging forms to *stats (the caller
 * zeroes it); returns after the stream. */
int srt_envelope_rows(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                      const uint32_t* D, size_t ldd, const int32_t* irp, const int32_t* icol,
                      const uint32_t* iw, const double* ir, double* lo, double* hi, size_t ldo,
                      hipStream_t st, srt_envelope_stats* stats) {
    if (nrows <= 0) return SRT_OK;
    if (n < 1 || !D || !irp || !icol || !iw || !ir || ldd < (size_t)n ||
        ((lo || hi) && ldo < (size_t)n)) {
        srt_set_error("envelope pass: bad arguments (n = %d, ldd = %zu, ldo = %zu)", n, ldd, ldo);
        return SRT_E_ARG;
    }
    if (n > srt_envelope_stage_max_n(3)) {
        srt_set_error("envelope pass: n = %d beyond its range (%d)", n, srt_envelope_stage_max_n(3));
        return SRT_E_RANGE;
    }
    const int form = n <= srt_envelope_stage_max_n(1) ? 1 : 3;
    const size_t lds = ev_bitmap_bytes(n) + (form == 1 ? (size_t)n * 4 : 0);
    /* per-block scratch: the hint row and the row of an output that is NULL (the 8-byte words
     * first: aligned); the grid shrinks to fit */
    const size_t per_block = (size_t)n * (8 * ((lo ? 0 : 1) + (hi ? 0 : 1)) + 4);
    const int grid = srt_pass_grid(lds, per_block, nrows, false);
    srt_pass_scratch sc;
    double *ws_lo = NULL, *ws_hi = NULL;
    int32_t* ws_hint = NULL;
    /* the three counts, then max_sweeps and forms (32 bits each) */
    unsigned long long hstat[4] = {0, 0, 0, 0};
    double ms = 0;
    srt_event_span span;
    int rc = span.begin(st);
    if (rc) return rc;
    rc = sc.open("envelope pass", st, (size_t)grid * per_block, sizeof(hstat));
    if (rc) return rc;
    char* const ws = sc.ws;
    unsigned long long* const dstat = (unsigned long long*)sc.dstat;
    if (!lo) ws_lo = (double*)ws;
    if (!hi) ws_hi = (double*)ws + (lo ? 0 : (size_t)grid * n);
    ws_hint = (int32_t*)((double*)ws + (size_t)grid * n * ((lo ? 0 : 1) + (hi ? 0 : 1)));
    if (form == 1) {
        SRT_PASS_TRY(hipFuncSetAttribute((const void*)envelope_kernel<1>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        envelope_kernel<1><<<grid, EV_THREADS, lds, st>>>(
            n, nrows, srcs, src_begin, by_src, D, ldd, irp, icol, iw, ir, lo, hi, ldo, ws_lo, ws_hi,
            ws_hint, dstat, (int32_t*)(dstat + 3), (uint32_t*)(dstat + 3) + 1);
    } else {
        SRT_PASS_TRY(hipFuncSetAttribute((const void*)envelope_kernel<3>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        envelope_kernel<3><<<grid, EV_THREADS, lds, st>>>(
            n, nrows, srcs, src_begin, by_src, D, ldd, irp, icol, iw, ir, lo, hi, ldo, ws_lo, ws_hi,
            ws_hint, dstat, (int32_t*)(dstat + 3), (uint32_t*)(dstat + 3) + 1);
    }
    SRT_PASS_TRY(hipGetLastError());
out:
    rc = sc.finish(rc, hstat);
    if (!rc) rc = span.end(st, &ms);
    if (!rc && stats) {
        const int32_t sweeps = (int32_t)(uint32_t)hstat[3];
        stats->ms_envelope += ms;
        stats->tied_pairs += (int64_t)hstat[0];
        stats->exposed_pairs += (int64_t)hstat[1];
        stats->sensitive_pairs += (int64_t)hstat[2];
        stats->max_sweeps = sweeps > stats->max_sweeps ? sweeps : stats->max_sweeps;
        stats->stage_forms |= (int32_t)(hstat[3] >> 32);
    }
    return rc;
}

/* ------------------------------------------------------------------------------------------ */
/* Dense front end: r[u][t] of every essential arc, beside srt_routes_ess_build's lists (one     */
/* thread per arc position; the head of a position by binary search in irp).                     */
/* ------------------------------------------------------------------------------------------ */
__global__ __launch_bounds__(256) void ev_ess_rel_kernel(int n, int ld, int arcs,
                                                         const int32_t* __restrict__ irp,
                                                         const int32_t* __restrict__ icol,
                                                         const double* __restrict__ r,
                                                         double* __restrict__ ir) {
    for (int k = blockIdx.x * 256 + threadIdx.x; k < arcs; k += gridDim.x * 256) {
        int a = 0, b = n; /* the last t with irp[t] <= k */
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (irp[mid] <= k)
                a = mid;
            else
                b = mid;
        }
        ir[k] = r[(size_t)icol[k] * ld + a];
    }
}

/* ir (arcs + 1 words from the scratch pool; hipFreeAsync returns it): the reliabilities of the
 * essential in-arcs irp / icol of a dense graph with the ld x ld matrix r; *ms += the HIP-event
 * time of the gather */
int srt_envelope_ess_rel(int n, int ld, int64_t arcs, const int32_t* irp, const int32_t* icol,
                         const double* r, hipStream_t st, double** ir, double* ms) {
    *ir = NULL;
    srt_event_span span;
    int rc = span.begin(st);
    if (rc) return rc;
    const int grid = srt_ceil_div(arcs, 256) < 8192 ? (arcs ? srt_ceil_div(arcs, 256) : 1) : 8192;
    SRT_PASS_TRY(srt_malloc_async((void**)ir, ((size_t)arcs + 1) * sizeof(double), st));
    ev_ess_rel_kernel<<<grid, 256, 0, st>>>(n, ld, (int)arcs, irp, icol, r, *ir);
    SRT_PASS_TRY(hipGetLastError());
    rc = span.end(st, ms);
out:
    if (rc && *ir) {
        (void)hipFreeAsync(*ir, st);
        *ir = NULL;
    }
    return rc;
}

extern "C" int srt_envelope_dense_device(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                                         const double* r, const uint32_t* lat, int32_t row0,
                                         int32_t nrows, double* rel_lo, double* rel_hi, size_t ldo,
                                         void* stream, srt_envelope_stats* stats) {
    if (n < 1 || ld < n || !w || !r || !lat || row0 < 0 || nrows < 1 || (int64_t)row0 + nrows > n ||
        ((rel_lo || rel_hi) && ldo < (size_t)n)) {
        srt_set_error("srt_envelope_dense_device: bad arguments (n = %d, ld = %d, rows [%d, %d))", n,
                      ld, row0, row0 + nrows);
        return SRT_E_ARG;
    }
    if (n > SRT_DENSE_MAX_N) {
        srt_set_error("srt_envelope_dense_device: n = %d beyond the dense limit %d (int32 arc offsets)",
                      n, SRT_DENSE_MAX_N);
        return SRT_E_RANGE;
    }
    hipStream_t st = (hipStream_t)stream;
    srt_envelope_stats local;
    memset(&local, 0, sizeof(local));
    int32_t *irp = NULL, *icol = NULL;
    uint32_t* iw = NULL;
    double* ir = NULL;
    int64_t arcs = 0;
    /* the compaction and the gather count as the pass */
    int rc = srt_routes_ess_build(n, ld, directed, w, lat, st, &irp, &icol, &iw, &arcs,
                                  &local.ms_envelope);
    if (!rc) rc = srt_envelope_ess_rel(n, ld, arcs, irp, icol, r, st, &ir, &local.ms_envelope);
    if (!rc)
        rc = srt_envelope_rows(n, nrows, NULL, row0, 0, lat + (size_t)row0 * ld, (size_t)ld, irp, icol,
                               iw, ir, rel_lo, rel_hi, ldo, st, &local);
    if (ir) (void)hipFreeAsync(ir, st);
    srt_routes_ess_free(irp, icol, iw, st);
    if (!rc && stats) *stats = local;
    return rc;
}
