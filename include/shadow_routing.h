/*
 * shadow_routing.h -- C-ABI of the MI355X-native routing-table build for Shadow.
 *
 * Drop-in boundary: Shadow's routing module, /root/reference/src/main/routing/topology.h:17-28.
 * The reference-signature entry points (topology_new, topology_attach, topology_getLatency, ...)
 * are declared in include/topology.h and implemented on top of the srt_* functions below.
 * Everything here uses plain C types (no glib, no torch): pointers, sizes, status codes.
 *
 * Table layout: row-major lat[n][n] in u32 quanta of `quantum_ns` nanoseconds
 * and rel[n][n] f64, indexed by graph vertex index (GML order). The diagonal holds the
 * "shortest path to self" rule (topology.c:1431-1576); undirected graphs are symmetric.
 */
#ifndef SHADOW_ROUTING_H
#define SHADOW_ROUTING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ----------------------------------------------------------------------- */
enum {
    SRT_OK = 0,
    SRT_E_ARG = -1,       /* bad argument / shape */
    SRT_E_PARSE = -2,     /* GML or unit parse error */
    SRT_E_INVALID = -3,   /* graph failed validation (topology.c:659-1038) */
    SRT_E_NOMEM = -4,     /* host or device allocation failed */
    SRT_E_DEVICE = -5,    /* HIP error (never a silent CPU fallback) */
    SRT_E_RANGE = -6,     /* path latencies exceed the u32-quantum table range */
    SRT_E_COMM = -7,      /* RCCL error */
    SRT_E_NOPATH = -8,    /* pair has no path (reference: utility_panic, topology.c:1970-1976) */
    SRT_E_UNATTACHED = -9 /* address not attached (reference: returns -1, topology.c:1905-1915) */
};

/* ---- units grammar (restates src/main/core/support/units.rs:404-437, :776-837) ----------- */
/* Nanoseconds, or -1 on a parse error / value > i64::MAX, or -2 where the reference's
 * `.unwrap()` on the unit conversion would panic (u64 overflow, units.rs:821). */
int64_t srt_parse_time_nanosec(const char* s);
/* Bits per second, or -1 / -2 with the same meaning (units.rs:776-805). */
int64_t srt_parse_bandwidth(const char* s);

/* ---- device build ------------------------------------------------------------------------ */
enum { SRT_ALGO_AUTO = 0, SRT_ALGO_DENSE_FW = 1, SRT_ALGO_SPARSE_SSSP = 2 };

/* Graph handed over as canonical arrays (one arc per ordered vertex pair, see srt_canon_*). */
typedef struct srt_edges {
    int32_t n;
    int32_t directed;
    int64_t m;
    const int32_t* src;    /* edge source vertex index (GML order) */
    const int32_t* dst;    /* edge target vertex index */
    const int64_t* lat_ns; /* parse_time_nanosec(latency) */
    const double* loss;    /* packet_loss */
} srt_edges;

typedef struct srt_build_opts {
    int32_t device;            /* HIP device ordinal */
    int32_t algo;              /* SRT_ALGO_* */
    int32_t use_shortest_path; /* network.use_shortest_path (configuration.rs:204-209) */
    int32_t fw_block;          /* 0 = default pivot-block edge */
} srt_build_opts;

typedef struct srt_build_stats {
    int32_t time_kernels; /* input: 1 = bracket every FW update launch with HIP events */
    int32_t algo;        /* algorithm actually used */
    int32_t fw_block;    /* dense: pivot-block edge used by FW; sparse: the kernel's form --
                          * wave kernel 1 = working row in LDS | 2 = private relabelled
                          * reliability row; workgroup kernel 4 | 1 = original vertex order
                          * | 2 = compact 8-byte arcs; multi-source kernel 8 | 16 = 16-bit
                          * working distances */
    int64_t ess_arcs;    /* essential arcs found by the predecessor pass (dense) */
    double ms_total;     /* wall time of the device build (HIP events), excl. host copies */
    double ms_fw;        /* shortest-distance kernels */
    double ms_post;      /* predecessor / reliability / diagonal / symmetry kernels */
    int32_t max_depth;   /* deepest shortest-path tree seen by the reliability pass */
    int32_t n_update;    /* FW update-kernel launches timed (time_kernels = 1) */
    double ms_update;    /* summed HIP-event duration of those launches */
    double ms_comm;      /* sharded builds (time_kernels = 1): device time the streams spent inside
                          * collectives, an event pair around each collective or group, waits for
                          * the peers included (they overlap the update on their own stream) */
    int32_t dist_enc;    /* sparse builds: 4 = u64 distances (wide.hip; the graph's range passes
                          * SRT_INF quanta), 3 = multi-source kernel (64 sources per workgroup),
                          * 2 = workgroup-per-source kernel (LDS-packed rows),
                          * 1 = wave-per-source kernel, 0 = workgroup kernel for every source.
                          * Dense: the distance encoding the build finished with: 12 = bit-parallel
                          * Dial levels (no FW rounds; levels.hip), (9: retired 256-pivot
                          * sharded rounds), 8 = u16
                          * f16-compare row-sharded symmetric rounds of 128 pivots (N > 1),
                          * 7 = 4 on two update streams with
                          * 256-pivot rounds (four panels per C-tile residency; one GPU,
                          * ld >= 8192), 6 = the same with
                          * 128-pivot rounds (two panels per C-tile residency), (5: retired
                          * 64-pivot rounds on two update streams), 4 = u16 with
                          * f16-compare mins, upper-triangle 64-pivot rounds (undirected, one
                          * GPU),
                          * 3 = u16 f16-compare (cap 0x3DFF), 2 = u16 pk_min (cap 0x7FFF), 1 = u32 */
    int32_t count_ties;  /* input: 1 = count tied pairs (below) */
    int64_t tied_pairs;  /* pairs (s, t), s != t, whose smallest D[s][u] over the tight
                          * predecessors u of t is reached by two or more u: igraph's heap order
                          * picks the reference's predecessor there (topology.c:1679-1701), the
                          * build takes the smallest u -- the class where reliability can differ.
                          * Unreachable pairs are never tied. Sharded builds: each rank of
                          * srt_dense_build_sharded reports the pairs of its own source rows;
                          * srt_build_tables_multi / _subset report the sum over the ranks */
    int32_t levels;      /* dense level builds (dist_enc 12): the Dial level that settled every pair */
    int64_t work_bytes;  /* algorithmic bytes of the timed launches (level builds: the Delta words
                          * gathered over all levels, counted on the device -- a unit stops early
                          * once its sources are settled), 0 where the bench models them itself */
    double ms_pred;      /* level builds (time_kernels = 1): HIP-event time of the predecessor pass
                          * (lvl_pred_kernel, with lvl_pred_near_kernel's pre-pass when taken) */
    double ms_rel;       /* ... and of the path-order reliability pass (rel_tree_kernel and the
                          * sweeps of the rows it hands over) */
    int32_t n_derived;   /* sparse full-table builds with derived rows (fw_block bit 64): the rows
                          * formed from their neighbours' (derive.hip), the rest by the kernel;
                          * work_bytes = the derivation's algorithmic bytes */
    double ms_core;      /* ... HIP-event time of the core rows' kernel (with their canonical arcs) */
    double ms_derive;    /* ... and of the derivation (or of the kernel for the set's rows, when a
                          * core row overflowed its buckets: n_derived = 0) */
    int32_t rel_table;   /* dense level builds: the distinct arc reliabilities of the packed post
                          * pass (predecessor | reliability index words); 0 = f64 rows */
    double ms_canon;     /* host clock: the canonical graph (srt_canon_build) */
    double ms_upload;    /* ... the dense matrices filled from it and moved to the device (pinned
                          * two-slot staging; the slowest rank of a sharded build) */
    double ms_download;  /* ... the tables moved into the caller's buffers (same staging) */
    int32_t pred_near;   /* dense level builds: the bucket capacity of the predecessor pre-pass
                          * (lvl_pred_near_kernel: the Delta_1 arc groups resolved from the in-arc
                          * runs), 0 = not taken */
    int32_t pred_near_over; /* ... its buckets that passed the capacity (their units walk the
                             * groups as without the pre-pass) */
} srt_build_stats;

/* Build the full tables for an edge list on one GPU; outputs are host buffers of n*n entries.
 * quantum_ns: the latency quantum (gcd of all edge latencies). Thread-safe per call. */
int srt_build_tables(const srt_edges* g, const srt_build_opts* opts, uint32_t* lat_q,
                     uint64_t* quantum_ns, double* rel, srt_build_stats* stats);

/* srt_build_tables over `ngpus` GPUs of this process (one host thread per GPU, RCCL over xGMI):
 * dense graphs shard rows with the pivot-panel broadcast, sparse graphs shard sources and
 * all-gather. The in-process form Shadow (one process) uses; bench.py runs the same kernels one
 * process per GPU. */
int srt_build_tables_multi(const srt_edges* g, const srt_build_opts* opts, int32_t ngpus,
                           uint32_t* lat_q, uint64_t* quantum_ns, double* rel,
                           srt_build_stats* stats);

/* Tables over a vertex subset -- the vertices with attached hosts, which are the only targets the
 * reference ever computes paths to (topology.c:1604-1656): outputs are nsub x nsub host tables
 * whose entry [i][j] is the pair (verts[i], verts[j]); verts strictly increasing (NULL with
 * nsub = n: every vertex). ngpus > 1 shards the build like srt_build_tables_multi.
 * lat_ms (optional, may be NULL): the path latency as the reference's f64 millisecond sum in path
 * order (topology.c:1308, :1364) -- differs from lat_q * quantum / 1e6 only when some edge latency
 * has a sub-millisecond part. min_lat_q (optional): the smallest table entry, diagonal included
 * (the runahead minimum, topology.c:1253-1264). */
int srt_build_tables_subset(const srt_edges* g, const srt_build_opts* opts, int32_t ngpus,
                            int32_t nsub, const int32_t* verts, uint32_t* lat_q,
                            uint64_t* quantum_ns, double* rel, double* lat_ms, uint32_t* min_lat_q,
                            srt_build_stats* stats);

/* Largest n of the dense (Floyd-Warshall) form; SRT_ALGO_AUTO sends larger graphs, and sparse
 * ones of any size, to the SSSP; an explicit SRT_ALGO_DENSE_FW beyond it fails with SRT_E_RANGE
 * before any work. */
int srt_dense_max_n(void);

/* Quantum and u32-range check used by srt_build_tables. Returns SRT_OK or SRT_E_RANGE. */
int srt_latency_quantum(const srt_edges* g, uint64_t* quantum_ns, uint32_t* max_w_q);

/* ---- device-resident dense build (benchmark / zero-copy path) ----------------------------
 * All pointers are HIP device pointers on the current device; `stream` is a hipStream_t (NULL =
 * default stream). Every matrix is ld x ld row-major with ld % 64 == 0 and ld >= n (rows and
 * columns >= n are padding). w: u32 quanta, diagonal = self-loop (SRT_INF = no edge);
 * r: f64 edge reliability (1 - loss). Outputs lat (u32 quanta) and rel (f64).
 * The predecessor-pass workspace is allocated on first use and cached per device. */
#define SRT_INF 0x7FFFFFFFu
int srt_dense_build_device(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                           const double* r, uint32_t* lat, double* rel, void* stream,
                           int32_t fw_block, srt_build_stats* stats);

/* Synthetic graph generators on the device (seeded counter-based hash; identical to
 * shadow_amd/graphs.py so tests can rebuild the same graph on the host). */
/* Rows of nsub sources (device vertex list dverts) on a dense device graph (w, r: ld x ld, as for
 * srt_dense_build_device) without the all-pairs FW: Bellman-Ford passes on u16 quanta, canonical
 * predecessors, path-order reliability, the diagonal rule. lat_rows / rel_rows: nsub x ld (row i =
 * source dverts[i]). SRT_E_RANGE when n > 32768 or a distance reaches the u16 cap. The table
 * builds take this path by themselves when at most n / 12 vertices are attached. */
int srt_dense_rows_build(int32_t n, int32_t ld, int32_t nsub, const int32_t* dverts,
                         const uint32_t* w, const double* r, uint32_t* lat_rows, double* rel_rows,
                         void* stream, srt_build_stats* stats);
int srt_gen_complete_device(int32_t n, int32_t ld, int32_t row0, int32_t nrows, uint64_t seed,
                            uint32_t lat_max_ms, uint32_t self_max_ms, uint32_t loss_max_e4,
                            uint32_t* w, double* r, void* stream);
/* the metric complete graph (Tor-atlas-like): n points of the unit square, latency
 * max(1, round(scale_ms * dist)) ms (scale_ms <= 1024), loss and self-loops as above;
 * oracle/oracle.c orc_metric_sample generates the same weights */
int srt_gen_metric_device(int32_t n, int32_t ld, int32_t row0, int32_t nrows, uint64_t seed,
                          uint32_t scale_ms, uint32_t self_max_ms, uint32_t loss_max_e4,
                          uint32_t* w, double* r, void* stream);

/* ---- device-resident sparse build (CSR of canonical arcs, self-loops excluded) ----------
 * Computes rows [src_begin, src_end) (row r of lat_rows/rel_rows = source src_begin + r, row
 * stride n) with one workgroup per source. The per-source working set (distance row, frontier
 * queue, bitmaps: ~8n + n/8 bytes) is LDS-resident for n <= srt_sparse_max_n() and lives in a
 * per-workgroup HBM slot beyond (persistent grid of 2 workgroups per CU; environment variable
 * SRT_FORM hbm=1 forces the HBM form for testing). delta = bucket width in quanta
 * (0 = default). Each row is its own source's (no symmetry rule is applied: see
 * srt_pair_order). */
int srt_sparse_max_n(void);
int srt_sparse_build_device(int32_t n, int32_t directed, const int32_t* rowptr,
                            const int32_t* col, const uint32_t* w, const double* r,
                            const int32_t* in_rowptr, const int32_t* in_col,
                            const uint32_t* in_w, const double* in_r, const uint32_t* self_w,
                            const double* self_r, int32_t src_begin, int32_t src_end,
                            uint32_t delta, uint32_t* lat_rows, double* rel_rows, void* stream,
                            srt_build_stats* stats);
/* Canonical CSR built on the host from an edge list and uploaded once to `device`; rows of any
 * source range can then be computed on that device (one shard per rank in a sharded build).
 * Replaces the per-source igraph Dijkstra of topology.c:1578-1814 (_topology_computeSourcePaths). */
typedef struct srt_sparse_graph srt_sparse_graph;
int srt_sparse_graph_new(const srt_edges* g, int32_t device, srt_sparse_graph** out);
int srt_sparse_graph_info(const srt_sparse_graph* g, int32_t* n, int32_t* directed, int64_t* arcs,
                          uint64_t* quantum_ns);
int srt_sparse_graph_rows(const srt_sparse_graph* g, int32_t src_begin, int32_t src_end,
                          uint32_t* lat_rows, double* rel_rows, void* stream,
                          srt_build_stats* stats);
/* Rows of an arbitrary source list (srcs: nsrc device ints; row r = source srcs[r], stride n),
 * e.g. the attached vertices. lat_ms_rows (optional): the f64 path-order ms rows -- required when
 * the graph's distances may pass the u32 range (SRT_E_RANGE without it; srt_sparse_graph_rows
 * refuses such a graph the same way). */
int srt_sparse_graph_rows_list(const srt_sparse_graph* g, int32_t nsrc, const int32_t* srcs,
                               uint32_t* lat_rows, double* rel_rows, double* lat_ms_rows,
                               void* stream, srt_build_stats* stats);
void srt_sparse_graph_free(srt_sparse_graph* g);

/* ---- routes: which way the paths go (routes.hip) ------------------------------------------
 * One optional pass over finished distance rows, whichever build made them. Per source s and
 * target t, three int32 values:
 *   pred[s][t]  the canonical predecessor, argmin (D[s][u], u) over the tight in-arcs u -> t
 *               (D[s][s] taken as 0); -1 for t == s and for unreachable t
 *   first[s][t] the first vertex after s on the path (the forwarding-table entry): t itself
 *               when pred == s, -1 where pred is -1
 *   hops[s][t]  the edges on the path: 0 for t == s, -1 for unreachable t
 * Following pred from t back to s gives the reference's `path:` (topology.c:1322, :1368-1369);
 * the reliability tables equal the left-to-right product of the arcs' reliabilities along it.
 * The routes of the path-to-self rule on the diagonal are not exported. */
typedef struct srt_route_stats {
    double ms_tables;    /* distance rows (whatever build made them); srt_build_routes only */
    double ms_routes;    /* HIP events around the route pass alone (dense: the essential-arc
                          * compaction included) */
    int64_t ess_arcs;    /* dense: essential arcs compacted */
    int32_t max_hops;    /* deepest route over the rows of the call */
    int32_t stage_forms; /* bit f-1 set when some row took staging form f */
} srt_route_stats;

/* Largest n whose distance row is staged on chip in form 1 (u32 row in LDS) or 2 (u16 row in LDS:
 * rows that do not fit as u32 and whose finite entries are all below 0xFFFF); form 3 reads the row
 * from global memory, and its value is the largest n the pass takes at all. */
int srt_routes_stage_max_n(int form);
/* Test diagnostic: the largest number of row chunks any row loop of the last srt_build_* call
 * took (tables, routes or link load; the rank threads of a multi-rank build included). Each
 * srt_build_* entry resets it, so it is not meaningful while builds run concurrently. */
int srt_last_row_chunks(void);
/* Device entry points: every pointer is a device pointer, any of the three outputs may be NULL,
 * outputs have row stride ldo (>= n; columns >= n are never written), `stream` as above. The
 * calls return after their work on the stream has finished.
 * Rows of a sparse graph: row i (of lat_rows, stride ldl, and of the outputs) belongs to srcs[i],
 * or src_begin + i when srcs is NULL. SRT_E_RANGE for a graph whose distances need u64 rows. */
int srt_routes_rows_device(const srt_sparse_graph* g, int32_t nsrc, const int32_t* srcs,
                           int32_t src_begin, const uint32_t* lat_rows, size_t ldl,
                           int32_t* pred, int32_t* first, int32_t* hops, size_t ldo,
                           void* stream, srt_route_stats* stats);
/* Rows [row0, row0 + nrows) of a dense device graph and its finished lat table (both ld x ld, as
 * for srt_dense_build_device): output row i belongs to source row0 + i. */
int srt_routes_dense_device(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                            const uint32_t* lat, int32_t row0, int32_t nrows, int32_t* pred,
                            int32_t* first, int32_t* hops, size_t ldo, void* stream,
                            srt_route_stats* stats);
/* Routes of nsrc sources (srcs strictly increasing; NULL with nsrc = n: every vertex) towards
 * every vertex: host outputs nsrc x n, any of them NULL. One GPU. The distance rows come from
 * the table build's own choice of algorithm, the routes from the pass above in every case.
 * use_shortest_path = 0: pred = s, first = t, hops = 1 for every t != s (SRT_E_INVALID unless the
 * graph is complete, as the table build). */
int srt_build_routes(const srt_edges* g, const srt_build_opts* opts, int32_t nsrc,
                     const int32_t* srcs, int32_t* pred, int32_t* first_hop, int32_t* hops,
                     srt_route_stats* stats);

/* ---- link load: traffic per arc from the routes and a demand (linkload.hip) -----------------
 * Given demands c(s, t) (u64) and the canonical routes above:
 *   load(u -> t)  the sum of c(s, x) over the pairs whose route from s crosses the arc u -> t
 *   through(v)    the sum of c(s, x) over the pairs whose route has v strictly inside
 * Demand that carries no load is counted, not dropped: at t == s it goes to self_demand (the
 * diagonal's path-to-self routes are not exported), at an unreachable t to unrouted; routed is the
 * rest, and the sum of load over the arcs equals the sum of c(s, t) * hops(s, t) over the routed
 * pairs. Every sum is u64; a demand whose total does not fit u64 is refused (SRT_E_RANGE), so
 * nothing wraps. */
typedef struct srt_link_load {
    int64_t narcs;
    int32_t *tail, *head;
    uint64_t* load;    /* arcs with load > 0, by (tail, head) */
    uint64_t* through; /* n */
    uint64_t routed, unrouted, self_demand;
    double ms_tables, ms_routes, ms_load; /* ms_load: HIP events around the load pass alone */
    int32_t max_hops; /* deepest route of the rows that carried routed demand */
    int32_t forms;    /* bit f-1 set when some row's flow words took form f */
} srt_link_load;
/* the load pass of a device entry point */
typedef struct srt_link_load_stats {
    double ms_load;
    int32_t max_hops, forms;
} srt_link_load_stats;

/* Largest n whose flow words (one per target of a row) live in LDS as u32 (form 1: rows whose
 * routed demand is below 2^32) or as u64 (form 2); form 3 keeps u64 words in device memory, and
 * its value is the largest n the pass takes at all. A row without routed demand takes no form. */
int srt_link_load_stage_max_n(int form);
/* Device entry point: every pointer is a device pointer. Row i of pred and hops (stride ldp: the
 * rows srt_routes_rows_device wrote for the same sources) and of the u64 demand rows dem (stride
 * ldd) belongs to srcs[i], or src_begin + i when srcs is NULL. The pass ADDS into load (one word
 * per in-arc of the graph, srt_sparse_graph_info's arc count, in the order of
 * srt_sparse_graph_in_arcs), through (n words) and totals (routed, unrouted, self): the caller
 * zeroes them before the first call and keeps the total demand within u64. Returns after the
 * stream. */
int srt_link_load_rows_device(const srt_sparse_graph* g, int32_t nsrc, const int32_t* srcs,
                              int32_t src_begin, const int32_t* pred, const int32_t* hops,
                              size_t ldp, const uint64_t* dem, size_t ldd, uint64_t* load,
                              uint64_t* through, uint64_t* totals, void* stream,
                              srt_link_load_stats* stats);
/* the in-arc CSR load is indexed by: device pointers owned by the graph (rowptr: n + 1 offsets by
 * head, tails: the tail of every position) */
int srt_sparse_graph_in_arcs(const srt_sparse_graph* g, const int32_t** rowptr,
                             const int32_t** tails);
/* Rows [row0, row0 + nrows) of a dense device graph and its finished lat table (as for
 * srt_routes_dense_device, whose pred and hops rows, stride ldp, it takes): load is indexed by the
 * essential in-arc CSR, which the call compacts and copies out -- rowptr (n + 1 offsets by head),
 * tails and load hold arc_cap positions (SRT_E_RANGE when the graph has more essential arcs:
 * srt_route_stats.ess_arcs says how many; *narcs receives the number). The call zeroes load,
 * through and totals itself. */
int srt_link_load_dense_device(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                               const uint32_t* lat, int32_t row0, int32_t nrows,
                               const int32_t* pred, const int32_t* hops, size_t ldp,
                               const uint64_t* dem, size_t ldd, int64_t arc_cap, int32_t* rowptr,
                               int32_t* tails, uint64_t* load, int64_t* narcs, uint64_t* through,
                               uint64_t* totals, void* stream, srt_link_load_stats* stats);
/* The link load of a demand on a host edge list. One GPU; the same choice of algorithm, chunks,
 * front ends and refusals as srt_build_routes (a graph whose distances need u64 rows:
 * SRT_E_RANGE).
 *   ndem < 0   uniform: demand 1 from every source of srcs (nsrc of them, strictly increasing;
 *              NULL with nsrc = n: every vertex) to every vertex
 *   ndem >= 0  COO demands (dsrc, dtgt, dval), grouped by source in increasing order (targets in
 *              any order, duplicates add); the sources are the distinct dsrc; srcs must be NULL
 *              and nsrc is ignored
 * The demand rows are built chunk by chunk on the device: no nsrc x n host matrix exists.
 * use_shortest_path = 0: load(s -> t) = c(s, t), through = 0, on the host (SRT_E_INVALID unless
 * the graph is complete). *out is freed with srt_link_load_free. */
int srt_build_link_load(const srt_edges* g, const srt_build_opts* opts, int32_t nsrc,
                        const int32_t* srcs, int64_t ndem, const int32_t* dsrc,
                        const int32_t* dtgt, const uint64_t* dval, srt_link_load** out);
void srt_link_load_free(srt_link_load* ll);

/* ---- reliability envelope: the bounds over every shortest-path tie order (envelope.hip) -----
 * The reference's Dijkstra takes as predecessor of t the first tight in-neighbour its heap pops:
 * one of those with the smallest D[s][u], the heap order deciding among equals. With M(s, t) that
 * set (the tight in-arcs u -> t of the canonical arcs with the smallest D[s][u], D[s][s] taken as
 * 0) and r(u, t) the arc reliability of the table build:
 *   hi(s, t) = max over u in M(s, t) of hi(s, u) * r(u, t)
 *   lo(s, t) = min over u in M(s, t) of lo(s, u) * r(u, t),   hi(s, s) = lo(s, s) = 1.0
 * one f64 multiply each: bit for bit the largest and smallest left-to-right product over every
 * path a heap order can yield (f64 multiplication by r >= 0 is monotone). The tables' own
 * reliability lies in [lo, hi]. Unreachable t: lo = hi = 0.0; t == s: lo = hi = 1.0 (the
 * path-to-self rule is not exported). The containment statement holds on graphs of whole-ms
 * edges, where the reference's ties are ties of equal integers too. */
typedef struct srt_envelope_stats {
    double ms_tables;        /* distance rows; srt_build_rel_envelope only */
    double ms_envelope;      /* HIP events around the pass alone (dense: the essential-arc
                              * compaction and the reliability gather included) */
    int64_t tied_pairs;      /* |M| >= 2: srt_build_stats.tied_pairs over the same rows */
    int64_t exposed_pairs;   /* tied, or some member of M exposed: the path depends on heap order */
    int64_t sensitive_pairs; /* lo != hi bitwise: the value does */
    int32_t max_sweeps;      /* the longest chain of the rows of the call, in arcs */
    int32_t stage_forms;     /* bit f-1 set when some row took staging form f */
} srt_envelope_stats;

/* Largest n whose distance row is staged in LDS as u32 beside the pass's bitmaps (form 1); form 3
 * reads the row from global memory, and its value is the largest n the pass takes at all. There
 * is no form 2 (0). */
int srt_envelope_stage_max_n(int form);
/* Device entry points, with the conventions of the route entries: every pointer is a device
 * pointer, either output may be NULL, outputs have row stride ldo (>= n; columns >= n are never
 * written), the calls return after their work on the stream has finished.
 * Rows of a sparse graph: row i (of lat_rows, stride ldl, and of the outputs) belongs to srcs[i],
 * or src_begin + i when srcs is NULL. SRT_E_RANGE for a graph whose distances need u64 rows. */
int srt_envelope_rows_device(const srt_sparse_graph* g, int32_t nsrc, const int32_t* srcs,
                             int32_t src_begin, const uint32_t* lat_rows, size_t ldl,
                             double* rel_lo, double* rel_hi, size_t ldo, void* stream,
                             srt_envelope_stats* stats);
/* Rows [row0, row0 + nrows) of a dense device graph (w, r) and its finished lat table (all
 * ld x ld, as for srt_dense_build_device): output row i belongs to source row0 + i. */
int srt_envelope_dense_device(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                              const double* r, const uint32_t* lat, int32_t row0, int32_t nrows,
                              double* rel_lo, double* rel_hi, size_t ldo, void* stream,
                              srt_envelope_stats* stats);
/* The envelope of nsrc sources (srcs strictly increasing; NULL with nsrc = n: every vertex)
 * towards every vertex: host outputs nsrc x n, either of them NULL. One GPU; the same choice of
 * algorithm, chunks, front ends and refusals as srt_build_routes (a graph whose distances need u64
 * rows: SRT_E_RANGE). use_shortest_path = 0: lo = hi = r(s, t) for t != s (SRT_E_INVALID unless the
 * graph is complete, as the table build). */
int srt_build_rel_envelope(const srt_edges* g, const srt_build_opts* opts, int32_t nsrc,
                           const int32_t* srcs, double* rel_lo, double* rel_hi,
                           srt_envelope_stats* stats);

/* ---- split load: the link load with every shortest-path tie split evenly (splitload.hip) -----
 * The link load above charges a pair's demand to its canonical route, one arbitrary choice among
 * the paths the reference's Dijkstra can return. Here each target's predecessor is drawn uniformly
 * from M(s, t), the set of the envelope above, and the outputs are the expected traffic. For a
 * source s with the demand row c(s, .), every reachable t != s has
 *   inflow_s(t) = the sum of share_s(v) over the v with t in M(s, v)
 *   f_s(t)      = (double)c(s, t) + inflow_s(t)
 *   share_s(t)  = f_s(t) / (double)|M(s, t)|                       one f64 division
 * and the source adds share_s(t) to load(u -> t) for every u in M(s, t) and inflow_s(t) to
 * through(t) (a share that reaches s adds to no through word). Where no pair is tied this is the
 * link load exactly. load and through are f64, summed with atomic adds across the sources, so two
 * runs may differ in the last bits unless every partial sum is exact; an arc in no M, or whose
 * targets carry no flow, gets no add: the arcs reported (load > 0) are an exact set. The totals
 * are u64 and exact, as the link load's; a total demand of 2^53 or more is refused (SRT_E_RANGE),
 * so every demand converts to f64 exactly. */
typedef struct srt_split_load {
    int64_t narcs;
    int32_t *tail, *head;
    double* load;    /* arcs with load > 0, by (tail, head) */
    double* through; /* n */
    uint64_t routed, unrouted, self_demand;
    double ms_tables, ms_split; /* ms_split: HIP events around the pass alone */
    int64_t tied_pairs; /* |M| >= 2 over every row of the call, with demand or without: the
                         * envelope's tied_pairs over the same rows */
    int32_t forms;      /* bit f-1 set when some row took staging form f */
} srt_split_load;
/* the pass of a device entry point */
typedef struct srt_split_load_stats {
    double ms_split;
    int64_t tied_pairs;
    int32_t max_sweeps; /* the longest chain of members of the rows that carried routed demand */
    int32_t forms;
} srt_split_load_stats;

/* Largest n whose distance row, children counters and f64 inflow words live in LDS (form 1), or
 * the row alone, the counters and inflow words in device memory (form 2); form 3 reads the row
 * from device memory too, and its value is the largest n the pass takes at all. */
int srt_split_load_stage_max_n(int form);
/* Device entry point: every pointer is a device pointer. Row i of lat_rows (u32 quanta, stride
 * ldl: the rows srt_sparse_graph_rows made) and of the u64 demand rows dem (stride ldd) belongs to
 * srcs[i], or src_begin + i when srcs is NULL. The pass ADDS into load (one f64 word per in-arc of
 * the graph, in the order of srt_sparse_graph_in_arcs), through (n f64 words) and totals (routed,
 * unrouted, self; u64): the caller zeroes them before the first call and keeps the total demand
 * below 2^53. SRT_E_RANGE for a graph whose distances need u64 rows. Returns after the stream. */
int srt_split_load_rows_device(const srt_sparse_graph* g, int32_t nsrc, const int32_t* srcs,
                               int32_t src_begin, const uint32_t* lat_rows, size_t ldl,
                               const uint64_t* dem, size_t ldd, double* load, double* through,
                               uint64_t* totals, void* stream, srt_split_load_stats* stats);
/* Rows [row0, row0 + nrows) of a dense device graph and its finished lat table (as for
 * srt_routes_dense_device; row i of dem belongs to source row0 + i): load is indexed by the
 * essential in-arc CSR, which the call compacts and copies out -- rowptr (n + 1 offsets by head),
 * tails and load hold arc_cap positions (SRT_E_RANGE when the graph has more essential arcs;
 * *narcs receives the number). The call zeroes load, through and totals itself. */
int srt_split_load_dense_device(int32_t n, int32_t ld, int32_t directed, const uint32_t* w,
                                const uint32_t* lat, int32_t row0, int32_t nrows,
                                const uint64_t* dem, size_t ldd, int64_t arc_cap, int32_t* rowptr,
                                int32_t* tails, double* load, int64_t* narcs, double* through,
                                uint64_t* totals, void* stream, srt_split_load_stats* stats);
/* The split load of a demand on a host edge list: the arguments, demand conventions, choice of
 * algorithm, chunks, front ends and refusals of srt_build_link_load (ndem < 0 uniform, else COO;
 * one GPU; a graph whose distances need u64 rows: SRT_E_RANGE), and SRT_E_RANGE before any device
 * work for a total demand of 2^53 or more. No route is computed: the pass reads the distance rows.
 * use_shortest_path = 0: load(s -> t) = c(s, t), through = 0, on the host (SRT_E_INVALID unless
 * the graph is complete). *out is freed with srt_split_load_free. */
int srt_build_split_load(const srt_edges* g, const srt_build_opts* opts, int32_t nsrc,
                         const int32_t* srcs, int64_t ndem, const int32_t* dsrc,
                         const int32_t* dtgt, const uint64_t* dval, srt_split_load** out);
void srt_split_load_free(srt_split_load* sl);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI) ----------------------------------- */
typedef struct srt_comm srt_comm;
/* 128-byte RCCL unique id, created on rank 0 and shared by the caller (e.g. torch.distributed). */
int srt_comm_unique_id(uint8_t out[128]);
int srt_comm_init(const uint8_t id[128], int32_t nranks, int32_t rank, int32_t device,
                  srt_comm** comm);
void srt_comm_free(srt_comm* comm);
/* In-process communicators for `ndev` devices (ncclCommInitAll): comms[i] drives devices[i]. */
int srt_comm_init_all(int32_t ndev, const int32_t* devices, srt_comm** comms);
/* `nranks` virtual ranks of one process on one device (tests of the sharded schedules on one
 * GPU): each comms[i] is driven by its own host thread; collectives become device-to-device
 * copies ordered by events and host barriers. srt_build_tables_multi uses them when the
 * environment sets SRT_VIRTUAL_RANKS. */
/* Timing only (tools/solo_rank.py): rank `rank` of `nranks` alone on `device`, every collective a
 * no-op, so one rank's compute and critical chain at N ranks is measured without the wire. The
 * tables it produces are NOT correct. */
int srt_comm_init_solo(int32_t nranks, int32_t rank, int32_t device, srt_comm** comm);
/* srt_comm_init_solo with a wire model: each collective holds its stream for lat_us + the bytes
 * this rank receives / gbps (GB/s), spun on the device wall clock; a group pays once, at its end.
 * srt_comm_wire_ms: the modelled wire time issued so far. Timing only, like srt_comm_init_solo. */
int srt_comm_init_solo_wire(int32_t nranks, int32_t rank, int32_t device, double gbps,
                            double lat_us, srt_comm** comm);
double srt_comm_wire_ms(const srt_comm* comm);
/* Collective log: with on != 0 every srt_coll_* call of the communicator appends (op, a, b) --
 * 1 broadcast (bytes, root), 2 all-reduce (count, op_min), 3 all-gather (bytes per rank, 0),
 * 4 exchange (0, 0), 5 group begin, 6 group end, 7 sparse all-gather (rows per rank, n).
 * Enabling clears the log. srt_comm_log_read copies up to cap entries (3 int64 each) into out
 * and returns the number logged. The ranks' logs of one build must be identical (SPMD). */
int srt_comm_log_enable(srt_comm* comm, int32_t on);
int64_t srt_comm_log_read(const srt_comm* comm, int64_t* out, int64_t cap);
/* ranks of the communicator: ncclCommCount for RCCL, nranks for virtual / timing-only ranks */
int srt_comm_count(const srt_comm* comm, int32_t* count);
int srt_comm_init_virtual(int32_t nranks, int32_t device, srt_comm** comms);
/* Bind the calling host thread to virtual rank `rank` on `device` (its own workspaces and
 * streams) before it drives that rank's srt_dense_build_sharded / srt_sparse_graph_rows;
 * rank < 0 returns the thread to the per-device state. */
int srt_virtual_rank_bind(int32_t rank, int32_t device);
/* Row-block partition used by every sharded build: rank r owns rows [begin, end). */
void srt_shard_rows(int32_t n, int32_t align, int32_t nranks, int32_t rank, int32_t* begin,
                    int32_t* end);
/* Dense FW over row shards: each rank passes its rows [begin,end) of w/r (ld columns) and gets
 * the same rows of lat/rel. Pivot-row panels are broadcast with RCCL once per round. */
int srt_dense_build_sharded(srt_comm* comm, int32_t n, int32_t ld, int32_t directed,
                            const uint32_t* w_rows, const double* r_rows, uint32_t* lat_rows,
                            double* rel_rows, void* stream, int32_t fw_block,
                            srt_build_stats* stats);
/* Sparse: each rank computes its source rows, then ncclAllGather assembles the full tables
 * (lat_all: n x n u32, rel_all: n x n f64, each rank's slice written in place). */
int srt_sparse_allgather(srt_comm* comm, int32_t n, int32_t rows_per_rank, uint32_t* lat_all,
                         double* rel_all, void* stream);

/* ---- misc ------------------------------------------------------------------------------ */
const char* srt_version(void);
const char* srt_last_error(void); /* thread-local message for the last failing call */
/* ---- pair order: which cached path the reference serves (pairorder.c) -------------------
 * Restates the lazy cache of topology.c:1166-1265 + :1900-1981 over tables holding every
 * source's raw row: a pair is served, in both directions, from the first source run (or, with
 * use_shortest_path = false, the first direct-edge lookup) that stored it. per_source = 1 for
 * shortest-path mode (a miss runs source s for every attached target, :1578-1814), 0 for direct
 * mode (a miss stores the pair s -> t, :1816-1858). Thread-safe; lookups are lock-free once
 * their pair is stored. */
typedef struct srt_pair_order srt_pair_order;
/* called (under the object's lock) with the paths a lookup stored: src -> targets[i] */
typedef void (*srt_pair_store_fn)(void* ctx, int32_t src, const int32_t* targets, int32_t count);
srt_pair_order* srt_pair_order_new(int32_t n, int32_t directed, int32_t per_source);
void srt_pair_order_free(srt_pair_order* po);
/* v joins the attached set (verticesWithAttachedHosts, topology.c:2231); idempotent */
int srt_pair_order_attach(srt_pair_order* po, int32_t v);
/* lookup (s, t): the source vertex of the path served (s or t), after recording the run or store
 * a miss causes; SRT_E_UNATTACHED if an end is not attached, SRT_E_NOPATH if no stored path
 * joins them (neither end reaches the other) */
int32_t srt_pair_order_lookup(srt_pair_order* po, int32_t s, int32_t t, srt_pair_store_fn on_store,
                              void* ctx);
/* the same without recording anything: -1 while the pair is not stored */
int32_t srt_pair_order_peek(srt_pair_order* po, int32_t s, int32_t t);
/* optional reachability predicate (1: s reaches t); a source run stores only the targets it reaches
 * (topology.c:1744-1753), so on a directed graph that is not strongly connected a pair is decided
 * by the first run from an end that reaches the other. NULL (the default): every pair reachable.
 * Set before the first lookup. */
typedef int (*srt_pair_reach_fn)(void* ctx, int32_t s, int32_t t);
void srt_pair_order_set_reach(srt_pair_order* po, srt_pair_reach_fn fn, void* ctx);
/* recorded source runs of v (one per attach epoch it ran in) */
int32_t srt_pair_order_runs(srt_pair_order* po, int32_t v);
/* the reference's path counters (topology.c:78-79): lookups that would have run a source's
 * Dijkstra (shortestPathCount, :1719; on a directed graph every lookup not served s's own path) and
 * the self paths computed (selfPathCount, :1536); shortest-path mode only */
void srt_pair_order_counts(srt_pair_order* po, uint32_t* source_runs, uint32_t* self_paths);
/* k more source runs (shortest-path mode): a caller that answers with one lookup what the
 * reference does with several -- worker_sendPacket's getReliability, getLatency and
 * incrementPathPacketCounter (worker.c:541-555), each a cache probe that, on a directed graph,
 * runs the source again while the pair is served the other end's path */
void srt_pair_order_add_source_runs(srt_pair_order* po, uint32_t k);

int srt_device_count(void);
int srt_device_sync(int32_t device);

#ifdef __cplusplus
}
#endif

#endif
