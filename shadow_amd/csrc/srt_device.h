/*
 * srt_device.h -- shared device-side definitions for the gfx950 kernels.
 */
#ifndef SRT_DEVICE_H
#define SRT_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "srt_internal.h"

/* a running maximum many workgroups raise once each (per-row depth counters): read it first, so
 * the same-address atomic -- serialised at the memory side, ~12 ns each -- runs only to raise it */
static __device__ __forceinline__ void srt_max_once(int32_t* p, int v) {
    if (v > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, v);
}

#define SRT_HIPCHK(expr)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            srt_set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__,   \
                          __LINE__, #expr);                                                \
            return SRT_E_DEVICE;                                                           \
        }                                                                                  \
    } while (0)

/* a HIP-event pair around a span of a stream (the row passes' own times) */
struct srt_event_span {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~srt_event_span() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    int begin(hipStream_t st) {
        SRT_HIPCHK(hipEventCreate(&e[0]));
        SRT_HIPCHK(hipEventCreate(&e[1]));
        SRT_HIPCHK(hipEventRecord(e[0], st));
        return SRT_OK;
    }
    int end(hipStream_t st, double* ms) {
        const int rc = stop(st);
        return rc ? rc : read(ms);
    }
    /* end in two halves, for a span that closes before more work joins the stream: stop marks
     * the span's end, read (any time later) waits for it and adds the span to *ms */
    int stop(hipStream_t st) {
        SRT_HIPCHK(hipEventRecord(e[1], st));
        return SRT_OK;
    }
    int read(double* ms) {
        float a = 0;
        SRT_HIPCHK(hipEventSynchronize(e[1]));
        SRT_HIPCHK(hipEventElapsedTime(&a, e[0], e[1]));
        *ms += a;
        return SRT_OK;
    }
};

/* the CUs of the current device (256 when it cannot be asked): the persistent grids' unit */
static inline int srt_cu_count(void) {
    int cus = 256, dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
        cus = prop.multiProcessorCount;
    return cus;
}

/* Per-thread slot of the static per-device state (workspaces, event pools, FW buffers and
 * streams): the current device (0..63), or 64 + r for virtual rank r when several ranks share
 * one device inside one process (srt_build_tables_multi with SRT_VIRTUAL_RANKS, comm.hip). */
#define SRT_STATE_SLOTS 128
/* the neighbour-row derivation's largest source degree (build.hip picks I, derive.hip sizes its
 * per-thread neighbour arrays by it) */
#define SRT_DERIVE_MAXDEG 4
int srt_state_slot(void);
/* stream-ordered scratch from the library's private pool of the current device (comm.hip) */
hipMemPool_t srt_scratch_pool(void);
#define srt_malloc_async(ptr, bytes, st) \
    hipMallocFromPoolAsync((void**)(ptr), (bytes), srt_scratch_pool(), (st))
void srt_set_virtual_slot(int rank); /* -1: back to the device slot */

/* Collectives over an srt_comm: RCCL, or (virtual ranks on one device) device-to-device copies
 * ordered by events and host barriers. Every rank calls the same sequence. */
int srt_coll_bcast(const srt_comm* c, void* buf, size_t bytes, int root, hipStream_t st);
int srt_coll_allreduce_i32(const srt_comm* c, int32_t* buf, size_t count, int op_min,
                           hipStream_t st);
int srt_coll_group_begin(const srt_comm* c);
int srt_coll_group_end(const srt_comm* c);
/* point-to-point exchange: to each peer q send send_bytes[q] from send[q], receive
 * recv_bytes[q] into recv[q] (arrays of comm size; zero bytes skip the pair) */
int srt_coll_exchange(const srt_comm* c, void* const* send, const size_t* send_bytes,
                      void* const* recv, const size_t* recv_bytes, hipStream_t st);
int srt_comm_rank(const srt_comm* c);
int srt_comm_is_solo(const srt_comm* c); /* timing-only communicator (srt_comm_init_solo) */
int srt_comm_size(const srt_comm* c);
/* ms_comm: on = 1 starts timing every collective (or group) of c with an event pair;
 * srt_comm_timing_ms waits for the last one and returns the summed spans (ms) */
void srt_comm_timing(const srt_comm* c, int on);
double srt_comm_timing_ms(const srt_comm* c);

/* pivot-block edge of the blocked Floyd-Warshall and the output-tile edge of its kernels */
#define SRT_FW_B 64
/* row-shard alignment of every sharded dense build (the u16 update tile is 128 rows) */
#define SRT_SHARD_ALIGN 128
/* LDS row stride (u32) of a 64-wide tile: +4 keeps 16-byte alignment for ds_read_b128 */
#define SRT_FW_LDT (SRT_FW_B + 4)

/* counter-based generator hash (shadow_amd/graphs.py restates it bit for bit) */
__host__ __device__ static inline uint64_t srt_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ static inline uint64_t srt_hash(uint64_t seed, uint64_t stream, uint32_t i,
                                                    uint32_t j) {
    return srt_splitmix64(srt_splitmix64(seed * 4ull + stream) ^ (((uint64_t)i << 32) | j));
}

static inline int srt_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

/* internal (C++ linkage) entry points shared between translation units */
/* HIP events bracketing every FW update launch (stats->time_kernels): the per-launch duration
 * of the dominant kernel that bench.py reports against the roofline. */
typedef struct {
    hipEvent_t* ev;
    int cap, used;
    /* 2: (start, end) per timed launch; 4: (start A, start B, end A, end B) per round for the
     * launch pairs of two update streams, which drift apart and overlap across rounds: the unit's
     * time is their period, (last end - first start) / pairs */
    int group;
} evpool_t;

evpool_t* srt_evpool(int dev);


static inline int evpool_begin(evpool_t** out, int rounds) {
    evpool_t* p = srt_evpool(srt_state_slot());
    if (p->cap < 4 * rounds) {
        hipEvent_t* ne = (hipEvent_t*)realloc(p->ev, sizeof(hipEvent_t) * 4 * rounds);
        if (!ne) return SRT_E_NOMEM;
        p->ev = ne;
        for (int i = p->cap; i < 4 * rounds; i++) SRT_HIPCHK(hipEventCreate(&p->ev[i]));
        p->cap = 4 * rounds;
    }
    p->used = 0;
    p->group = 2;
    *out = p;
    return SRT_OK;
}

/* grow the pool to at least n events without resetting what it holds */
static inline int evpool_reserve(evpool_t* p, int n) {
    if (p->cap >= n) return SRT_OK;
    hipEvent_t* ne = (hipEvent_t*)realloc(p->ev, sizeof(hipEvent_t) * n);
    if (!ne) return SRT_E_NOMEM;
    p->ev = ne;
    for (int i = p->cap; i < n; i++) SRT_HIPCHK(hipEventCreate(&p->ev[i]));
    p->cap = n;
    return SRT_OK;
}

static inline int evpool_sum(evpool_t* p, hipEvent_t last, srt_build_stats* stats) {
    SRT_HIPCHK(hipEventSynchronize(last));
    double tot = 0;
    const int g = p->group == 4 ? 4 : 2;
    if (g == 2) {
        for (int i = 0; i + 1 < p->used; i += 2) {
            float ms = 0;
            SRT_HIPCHK(hipEventElapsedTime(&ms, p->ev[i], p->ev[i + 1]));
            tot += ms;
        }
    } else if (p->used >= 4) { /* relative to the first start A */
        const int l = p->used - 4;
        float sb = 0, ea = 0, eb = 0;
        SRT_HIPCHK(hipEventElapsedTime(&sb, p->ev[0], p->ev[1]));
        SRT_HIPCHK(hipEventElapsedTime(&ea, p->ev[0], p->ev[l + 2]));
        SRT_HIPCHK(hipEventElapsedTime(&eb, p->ev[0], p->ev[l + 3]));
        tot = (ea > eb ? ea : eb) - (sb < 0 ? sb : 0);
    }
    stats->ms_update = tot;
    stats->n_update = p->used / g;
    return SRT_OK;
}


typedef int (*srt_panel_bcast_fn)(void* ctx, void* panel, size_t bytes, int owner, hipStream_t st);
typedef int (*srt_owner_fn)(void* ctx, int k0);
/* row-sharded symmetric rounds (undirected, f16-compare path, >= 2 ranks; fw16.hip) */
int srt_fw16_build_sym_sharded(const srt_comm* comm, int n, int ld, int row0, int nrows,
                               const uint32_t* w_rows, uint32_t* lat_rows, hipStream_t st,
                               evpool_t* evp, int* exact);
/* packed-u16 Floyd-Warshall over a row shard (fw16.hip). d16: nrows x ld u16. symmetric = 1
 * (undirected, symmetric w) lets a single-shard f16-compare build update only upper-triangle
 * tiles. fm = 1 selects the f16-compare instruction mix (cap 0x3DFF), fm = 0 the v_pk_min_u16 mix
 * (cap 0x7FFF). *enc (may be NULL) receives the SRT_DENC_* value of the form that ran. Returns
 * SRT_OK and *exact = 1 when every distance is below the cap (else the caller reruns with the
 * next wider path). lat_rows receives the distances widened to u32 quanta. */
int srt_fw16_build(int n, int ld, int row0, int nrows, const uint32_t* w_rows, uint32_t* lat_rows,
                   hipStream_t st, evpool_t* evp, srt_owner_fn owner_of, srt_panel_bcast_fn bcast,
                   void* ctx, int rank, int fm, int symmetric, int* enc, int* exact);
/* levels.hip: distance rows of the local sources by bit-parallel Dial levels (see there) */
int srt_levels_build(const srt_comm* comm, int n, int ld, int row0, int nrows, int directed,
                     const uint32_t* w_rows, const double* r_rows, uint32_t* lat_rows, double fw_ms,
                     hipStream_t st, evpool_t* evp, int* levels, int64_t* gather_bytes);
/* what srt_levels_pred writes: predecessors + arc reliabilities (rT) target-major with row stride
 * ldp, or one packed word per pair (pred | reliability index << 16 | level << 27, no rT) */
typedef enum {
    SRT_LVL_PRED_I32 = 0,     /* int32 predecessors + f64 reliabilities, target-major */
    SRT_LVL_PRED_I16 = 1,     /* int16 predecessors (n <= 32768) + f64 reliabilities, target-major */
    SRT_LVL_PRED_PK_COLS = 2, /* packed words, target-major (needs srt_levels_rtab) */
    SRT_LVL_PRED_PK_ROWS = 3, /* packed words source-major, predT[local source][target] with row
                               * stride ldp: no transpose after it; ties must be NULL */
} srt_lvl_pred_layout;
/* the post pass a held level build was made for */
typedef enum {
    SRT_LVL_POST_U8 = 0,      /* the u8 level rows + srt_levels_pred + rel_tree_kernel */
    SRT_LVL_POST_PK_ROWS = 1, /* packed words source-major (SRT_LVL_PRED_PK_ROWS), then rel_pk_kernel,
                               * which writes the u32 rows too */
    SRT_LVL_POST_PK_COLS = 2, /* packed words target-major (SRT_LVL_PRED_PK_COLS), one transpose,
                               * rel_pk_kernel */
} srt_lvl_post_form;
/* predecessors + arc reliabilities of the held level build in the layout `out`. *pn_cap: the
 * bucket capacity of lvl_pred_near_kernel's pre-pass (0: not taken); it adds its overflowed
 * buckets to the device word pn_over. */
int srt_levels_pred(void* predT, srt_lvl_pred_layout out, double* rT, size_t ldp,
                    unsigned long long* ties, int32_t* pn_over, int* pn_cap, hipStream_t st);
/* the held level build's post pass (SRT_LVL_POST_U8 when none is held) */
srt_lvl_post_form srt_levels_pkw_ready(void);
/* frees the held level build (stream-ordered) */
void srt_levels_release(hipStream_t st);
/* the held build's u8 distance rows (nrows x ld, 0 on the diagonal), NULL if none */
const uint8_t* srt_levels_l8(void);
/* the held level build's distinct arc reliabilities (the packed post pass: predecessor | index << 16
 * words, SRT_LVL_PRED_PK_COLS / PK_ROWS); NULL (ntab 0) when the build keeps the f64 form */
const double* srt_levels_rtab(int* ntab);
/* the diagonal rule of the held build's rows (keys from its row reads); *applied = 0 when it kept
 * none (directed builds: dense_diag_kernel) */
int srt_levels_diag(int n, int ld, uint32_t* d, double* rel, hipStream_t st, int* applied);
/* the same into this slot's FW matrix + the finish pass (fw16.hip); *nlev = 0: FW instead */
int srt_fw16_levels(const srt_comm* comm, int n, int ld, int row0, int nrows, int directed,
                    const uint32_t* w_rows, const double* r_rows, uint32_t* lat_rows,
                    hipStream_t st, evpool_t* evp, double fw_ms, int* nlev, int64_t* bytes);
/* the u16 working matrix of the last srt_fw16_build on the current device (row shard x ld) */
const uint16_t* srt_fw16_matrix(void);
/* 1 when every real distance of that build is <= 254 quanta (the post pass then reads u8) */
int srt_fw16_small(void);
/* distance encodings of the dense build, reported (negated) in srt_build_stats.fw_block */
enum {
    SRT_DENC_U32 = 1,
    SRT_DENC_U16 = 2,
    SRT_DENC_F16CMP = 3,
    SRT_DENC_F16CMP_SYM = 4,      /* one GPU, upper triangle, 64-pivot rounds on one stream */
    SRT_DENC_F16CMP_SYM2 = 5,     /* retired: 64-pivot rounds on two update streams */
    SRT_DENC_F16CMP_SYM128 = 6,   /* one GPU, upper triangle on two update streams, 128-pivot
                                   * rounds (4 stages per tile) */
    SRT_DENC_F16CMP_SYM256 = 7,   /* the same with 256-pivot rounds (8 stages per tile) */
    SRT_DENC_F16CMP_SYMSH128 = 8, /* row-sharded kept tiles (>= 2 ranks), 128-pivot rounds */
    SRT_DENC_F16CMP_SYMSH256 = 9, /* retired: row-sharded 256-pivot rounds */
    SRT_DENC_ROWS = 10,           /* a few source rows by Bellman-Ford passes, no FW */
    SRT_DENC_SQUARE = 11,         /* ld <= 2048 on one GPU: min-plus squaring to a fixed point */
    SRT_DENC_LEVELS = 12          /* bit-parallel Dial levels (levels.hip), no FW rounds */
};
int srt_dense_rows_build_device(int32_t n, int32_t ld, int32_t nsub, const int32_t* dverts,
                                const uint32_t* w, const double* r, uint32_t* lat_rows,
                                double* rel_rows, double* lms_rows, uint64_t quantum_ns,
                                int32_t directed, hipStream_t st, srt_build_stats* stats, int* used);
/* distance rows of nsub sources on a dense graph by Bellman-Ford passes on u16 quanta (fw16.hip);
 * w16: ld x ld scratch, ds: (nsub rounded up to 128) x ld scratch, lat_rows: nsub x ld u32 */
int srt_fw16_rows(int n, int ld, int nsub, const int32_t* dverts, const uint32_t* w, uint16_t* w16,
                  uint16_t* ds, uint32_t* lat_rows, hipStream_t st, int* exact, int* small,
                  int* passes);

/* Largest dense n: the predecessor keys pack a 16-bit rank and the essential-arc offsets are
 * int32 (n^2 < 2^31), rounded down to the 128 tile. */
#define SRT_DENSE_MAX_N 46336
/* Dense builds with the optional f64 path-order ms table (lat_ms / lms_rows may be NULL). */
int srt_dense_build_device_ms(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                              const double* r, uint32_t* lat, double* rel, double* lat_ms,
                              uint64_t quantum_ns, hipStream_t st, int32_t fw_block,
                              srt_build_stats* stats);
int srt_dense_build_sharded_ms(srt_comm* comm, int32_t n, int32_t ld, int32_t directed,
                               const uint32_t* w_rows, const double* r_rows, uint32_t* lat_rows,
                               double* rel_rows, double* lms_rows, uint64_t quantum_ns,
                               hipStream_t st, int32_t fw_block, srt_build_stats* stats);

/* tables.hip: path-order passes, sub-table gathers, table minimum */
int srt_path_sweeps_max_n(void);
/* out rows (f64 ms, path order) of nrows sources (srcs[r], or src_begin + r) from their distance
 * rows D (diagonal rule applied) and either predecessor rows or the in-arc CSR */
int srt_path_ms_rows(int n, int nrows, const int32_t* srcs, int src_begin, const uint32_t* D,
                     size_t ldd, const int32_t* pred, size_t ldp, const int32_t* irp,
                     const int32_t* icol, const uint32_t* iw, uint64_t quantum_ns, double* out,
                     size_t ldo, hipStream_t st);
int srt_rel_sweeps_rows(int n, int nrows, int row0, const int32_t* pred, size_t ldp, double* rel,
                        size_t ldr, const int32_t* only, int32_t* max_depth, hipStream_t st);
int srt_gather_sub_u32(int nr, int nc, const int32_t* rows, const int32_t* cols, const uint32_t* in,
                       size_t ldi, uint32_t* out, size_t ldo, hipStream_t st);
int srt_gather_sub_f64(int nr, int nc, const int32_t* rows, const int32_t* cols, const double* in,
                       size_t ldi, double* out, size_t ldo, hipStream_t st);
int srt_table_min(int rows, int cols, const uint32_t* t, size_t ld, uint32_t* dmin, hipStream_t st);
/* dense matrices from the edge list on the device (tables.hip): prepare (all-ones), the minimum
 * latency per pair into r's bits, the lowest index among the minima into w, then in place the
 * quanta / reliabilities (SRT_INF / 0 where no edge) with the off-diagonal arcs counted */
int srt_scatter_prepare(int nrows, int ld, uint32_t* w, double* r, hipStream_t st);
int srt_scatter_min(int64_t m, const int32_t* src, const int32_t* dst, const int64_t* lat, int directed,
                    int32_t row0, int nrows, int ld, double* r, hipStream_t st);
int srt_scatter_idx(int64_t m, const int32_t* src, const int32_t* dst, const int64_t* lat, int directed,
                    int32_t row0, int nrows, int ld, const double* r, uint32_t* w, hipStream_t st);
int srt_scatter_final(int32_t row0, int nrows, int ld, uint64_t q, const double* loss, uint32_t* w,
                      double* r, unsigned long long* arcs, hipStream_t st);
/* adds the tied pairs of nrows distance rows (diagonal rule applied) to *tied */
int srt_tie_count_rows(int n, int nrows, const int32_t* srcs, int src_begin, const uint32_t* D,
                       size_t ldd, const int32_t* irp, const int32_t* icol, const uint32_t* iw,
                       int64_t* tied, hipStream_t st);
int srt_quanta_to_ms(int rows, int cols, const uint32_t* w, size_t ldw, uint64_t q, double* out,
                     size_t ldo, hipStream_t st);
/* routes.hip: predecessor / first hop / hop count rows from distance rows and an in-arc CSR (any
 * output NULL). Row r is source srcs[r] (or src_begin + r), its distances row s (by_src) or row r
 * of D. Returns after the stream; raises *max_hops, ors the staging forms taken into *forms */
int srt_routes_rows(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                    const uint32_t* D, size_t ldd, const int32_t* irp, const int32_t* icol,
                    const uint32_t* iw, int32_t* pred, int32_t* first, int32_t* hops, size_t ldo,
                    hipStream_t st, int32_t* max_hops, int32_t* forms);
/* the same between HIP events, added to *stats (ms_routes, max_hops, stage_forms) */
int srt_routes_rows_timed(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                          const uint32_t* D, size_t ldd, const int32_t* irp, const int32_t* icol,
                          const uint32_t* iw, int32_t* pred, int32_t* first, int32_t* hops,
                          size_t ldo, hipStream_t st, srt_route_stats* stats);
/* the essential in-arc CSR of a dense graph and its finished lat table (both ld x ld), from the
 * scratch pool (*ms += the compaction's HIP-event time); srt_routes_ess_free returns it
 * (stream-ordered) */
int srt_routes_ess_build(int n, int ld, int directed, const uint32_t* w, const uint32_t* lat,
                         hipStream_t st, int32_t** irp, int32_t** icol, uint32_t** iw,
                         int64_t* arcs, double* ms);
void srt_routes_ess_free(int32_t* irp, int32_t* icol, uint32_t* iw, hipStream_t st);
/* linkload.hip: the load pass over nrows rows of pred / hops (stride ldp) and u64 demand (stride
 * ldd) against an in-arc CSR: ADDS into load (one word per CSR position), through (n) and totals
 * (routed, unrouted, self); sorted != 0 promises in-lists with ascending tails (a sparse graph's,
 * an undirected dense graph's: binary search; else the lists are scanned); raises *max_hops, ors
 * the flow forms into *forms, adds the HIP-event time of the kernel to *ms. Returns after the
 * stream. */
int srt_link_load_rows(int n, int nrows, const int32_t* srcs, int src_begin, const int32_t* pred,
                       const int32_t* hops, size_t ldp, const uint64_t* dem, size_t ldd,
                       const int32_t* irp, const int32_t* icol, uint64_t* load, uint64_t* through,
                       int sorted, uint64_t* totals, hipStream_t st, int32_t* max_hops,
                       int32_t* forms, double* ms);
/* demand rows of a chunk: 1 everywhere (rowptr NULL), or the COO entries [rowptr[r], rowptr[r + 1])
 * of row r added into zeroed rows (tgt, val: device arrays those offsets index) */
int srt_link_load_demand_rows(int n, int nrows, const int64_t* rowptr, const int32_t* tgt,
                              const uint64_t* val, uint64_t* dem, size_t ldd, hipStream_t st);
/* envelope.hip: the reliability bounds lo / hi (either NULL) of nrows distance rows over an in-arc
 * CSR with the arcs' reliabilities ir; rows, sources and strides as srt_routes_rows. Adds the
 * HIP-event time, the counts, the sweeps and the staging forms to *stats; returns after the
 * stream */
int srt_envelope_rows(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                      const uint32_t* D, size_t ldd, const int32_t* irp, const int32_t* icol,
                      const uint32_t* iw, const double* ir, double* lo, double* hi, size_t ldo,
                      hipStream_t st, srt_envelope_stats* stats);
/* r[u][t] of the essential in-arcs of srt_routes_ess_build, from the scratch pool (hipFreeAsync
 * returns it); *ms += the gather's HIP-event time */
int srt_envelope_ess_rel(int n, int ld, int64_t arcs, const int32_t* irp, const int32_t* icol,
                         const double* r, hipStream_t st, double** ir, double* ms);
/* splitload.hip: the load with every tie split evenly, over nrows distance rows (rows, sources and
 * strides as srt_routes_rows) and u64 demand rows (stride ldc) against an in-arc CSR: ADDS into
 * load (one f64 word per CSR position), through (n f64) and totals (routed, unrouted, self). Adds
 * the HIP-event time, the tied pairs, the sweeps and the staging forms to *stats; returns after
 * the stream */
int srt_split_load_rows(int n, int nrows, const int32_t* srcs, int src_begin, int by_src,
                        const uint32_t* D, size_t ldd, const uint64_t* dem, size_t ldc,
                        const int32_t* irp, const int32_t* icol, const uint32_t* iw, double* load,
                        double* through, uint64_t* totals, hipStream_t st,
                        srt_split_load_stats* stats);
/* collectives: all-gather of equal byte blocks, rank q's block at buf + q * bytes */
int srt_coll_allgather(const srt_comm* c, void* buf, size_t bytes, hipStream_t st);

#endif
