/*
 * geo_hip.h -- C ABI of libgeo_hip.so, the MI355X (gfx950) implementation of the geodesic-codebook
 * hot path of m4rch1n0/vqvae (src/geo + src/scripts/build_codebook.py).
 *
 * The reference has no FFI boundary of its own: its boundary is the Python API of src/geo, whose
 * numerics are executed by scipy / scikit-learn / torch.autograd on the CPU.  Each entry point below
 * replaces one of those third-party call sites (cited as reference file:line) and is what a binding
 * in the reference's src/geo modules would call (see INTEGRATION.md for the ctypes stubs).
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer unless the parameter is marked [host];
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it.  Functions marked
 *     "synchronises" call hipStreamSynchronize(stream) before returning (they need a host decision);
 *   - no allocation crosses the ABI: the caller owns inputs, outputs and the workspace `ws`
 *     (size from the matching *_workspace_bytes query, any 256-byte aligned device buffer);
 *   - return value: 0 = ok, negative = error (GEO_E_*); geo_last_error() gives the text;
 *   - concurrency: calls from DIFFERENT host threads may run at the same time provided each uses its own stream, its own
 *     workspace and its own output buffers (bench.py pipelines two builds that way); geo_last_error's buffer, the sweep
 *     profile of geo_sssp_last_profile and its HIP events are per host thread.  The options of geo_set_option are
 *     process-global: change them only while no call is in flight.
 */
#ifndef GEO_HIP_H
#define GEO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEO_OK 0
#define GEO_E_ARG (-1)      /* invalid argument (shape, null pointer, unsupported size) */
#define GEO_E_WORKSPACE (-2) /* workspace too small */
#define GEO_E_HIP (-3)      /* a HIP runtime call failed */
#define GEO_E_NOCONV (-4)   /* iteration limit reached without convergence */

int geo_version(void);
const char *geo_last_error(void);

/* Experiment switches ("sssp_group", "knn_filter", "kpp_profile", ...: the table in DESIGN.md).  They are seeded from
 * the GEO_* environment variables ONCE, when the library is first called; afterwards only this call changes them.
 * Process-wide and not synchronised (like the rest of the library: one call at a time).  GEO_E_ARG: unknown name. */
int geo_set_option(const char *name, int32_t value);

/* ------------------------------------------------------------------------------------------
 * Shortest paths.  Replaces scipy.sparse.csgraph.dijkstra as called from
 * src/geo/geo_shortest_paths.py:36-49 (dijkstra_multi_source) and, through it,
 * src/geo/kmeans_optimized.py:43,97,125.
 *
 * The graph is a "pull" CSR: row v lists the nodes u with an edge u->v and its weight.  For an
 * undirected solve on a symmetric matrix that is the matrix itself.  Path sums are accumulated in
 * fp64 source-outward, one rounding per hop, and the label-correcting iteration is run to its fixed
 * point, so the fp64 distances equal Dijkstra's; they are rounded to f32 on output exactly like
 * geo_shortest_paths.py:50.  weights == NULL means unit weights (unweighted=True, :32-34).
 * Unreachable = +inf; predecessor sentinel -9999.
 * ------------------------------------------------------------------------------------------ */
size_t geo_sssp_workspace_bytes(int32_t n, int64_t nnz, int32_t n_sources);

/* S sources -> any of: D_out f32 [S][n]; P_out i32 [S][n]; dmin_out f32 [n] + argmin_out i32 [n]
 * (column minimum over the S rows of the f32 matrix and the FIRST row index attaining it,
 * = D.argmin(axis=0) of kmeans_optimized.py:100; all-inf column -> 0).  Any output may be NULL.
 * sweeps_out [host, may be NULL] receives the number of relaxation sweeps launched.
 * Internally the sources may be relaxed in another order than given (batches of neighbouring sources on graphs
 * with long geodesics); every output is in the caller's order and does not depend on that.
 * Synchronises. */
int geo_sssp_multi(const int32_t *indptr, const int32_t *indices, const float *weights,
                   int32_t n, int64_t nnz, const int32_t *sources, int32_t n_sources,
                   float *D_out, int32_t *P_out, float *dmin_out, int32_t *argmin_out,
                   void *ws, size_t ws_bytes, int32_t *sweeps_out, void *stream);

/* Nearest source per node in ONE label-carrying solve (what assign_points_to_medoids, kmeans_optimized.py:77-106, keeps of the
 * K x N matrix): dmin_out[v] = min_s D[s][v] and argmin_out[v] = D.argmin(axis=0)[v] of the FLOAT32 matrix dijkstra_multi_source
 * returns (geo_shortest_paths.py:50 casts before kmeans_optimized.py:100 compares): the lowest source row whose distance ROUNDS
 * to the column's float32 minimum -- not necessarily the exactly nearest one.  An unreachable node gets (+inf, 0).
 * The CSR must be symmetric (undirected graph, what the reference's callers pass): nodes whose two nearest sources round to the
 * same float32 ("suspects") are resolved by a solve from those nodes read at the sources.
 * status_out (host, int32 [4]): [0] = 0 answered / 1 declined (nothing usable written: call geo_sssp_multi with dmin_out /
 * argmin_out instead), [1] = sweeps, [2] = suspect nodes found, [3] = reason when declined (1 weights outside 28 bits of their
 * common power-of-two unit, negative or non-finite; 2 a distance reached 2^39 units; 3 more than 32 suspects; 4 n_sources >= 2^24 - 1).
 * Either output may be NULL.  Synchronises. */
size_t geo_sssp_nearest_workspace_bytes(int32_t n, int64_t nnz);
int geo_sssp_nearest_source(const int32_t *indptr, const int32_t *indices, const float *weights, int32_t n, int64_t nnz,
                            const int32_t *sources, int32_t n_sources, float *dmin_out, int32_t *argmin_out, void *ws,
                            size_t ws_bytes, int32_t *status_out, void *stream);

/* Device time (ms, HIP events on the call's stream) spent in the relaxation sweeps of the last
 * geo_sssp_multi call, and how many sweep kernels it launched.  Used by bench.py's roofline.
 * Returns the layout that call used: sources per batch (16 or 64), +1000 for the chunked 16-source kernel,
 * 2032 for the exact 32-bit fixed-point kernel (32 sources per row), 4016 for the near-far push solve
 * (long geodesics: sources ordered along landmark distances, 16 per batch, delta-stepping buckets; one launch per sweep). */
int geo_sssp_last_profile(double *sweep_ms, int32_t *sweep_launches);

/* The layout geo_sssp_multi would START with for a graph of n nodes and n_sources sources (host arithmetic only, no GPU
 * call): sources per batch (16 or 64), +1000 when the 16-edge-chunk kernels run, +2000 more when the exact 32-bit
 * fixed-point solve is tried first.  The 16- / 32-source row layouts address a batch with 32-bit byte offsets and are
 * therefore never chosen for n >= 2^25 nodes.  Negative on bad arguments. */
int geo_sssp_plan(int32_t n, int32_t n_sources);

/* One source; fused k-means++ bookkeeping of kmeans_optimized.py:43-44 and the single-pass
 * assignment: d32 = f32(dist(source, .)); where d32 < dmin: dmin = d32, argmin = center_pos.
 * d_out f32 [n] may be NULL, dmin_inout/argmin_inout may be NULL.  Synchronises. */
int geo_sssp_single_update(const int32_t *indptr, const int32_t *indices, const float *weights,
                           int32_t n, int32_t source, float *d_out,
                           float *dmin_inout, int32_t *argmin_inout, int32_t center_pos,
                           void *ws, size_t ws_bytes, int32_t *sweeps_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * k-means++ seeding chain, device resident.  Replaces the loop of src/geo/kmeans_optimized.py:40-71:
 * iteration t in [it0, it1) solves from centers[t], folds the f32 distances into dmin/argmin (position t)
 * and, when t+1 < n_centers_total, draws centers[t+1] with numpy's legacy RandomState.choice semantics
 * (float32 D^2 weights, float32 add.reduce, fp64 cdf, searchsorted) from the uniform deviate u_host[t]
 * the caller took from the same RandomState stream.  centers i32 [n_centers_total] (centers[it0] set by
 * the caller), is_center u8 [n] (set for centers[0..it0]), dmin f32 [n] / argmin i32 [n] carried state.
 * sweeps_per_solve relaxation sweeps are enqueued per solve (they exit early once converged); 0 (needs
 * assume_finite) runs the chain as one step kernel launched until done: no budget, reason 1 only past 4094 sweeps;
 * -1 (needs assume_finite and n <= geo_kpp_resident_max_nodes()) runs iterations [it0, it1) inside ONE resident
 * workgroup in a single launch (solve in an LDS hash table, incremental float32 reduction tree, draw): the mode for
 * small cells; a centre whose cell outgrows the table is run by the step kernel inside the call.
 * assume_finite != 0 promises that d_min has no inf entry left (status_out[2] of an earlier call): the
 * per-iteration maximum pass is skipped.
 * status_out [host, 4 ints]: {abort_iter or -1, reason, inf entries of d_min at the last maximum pass (0 in resident
 * mode), a count that depends on the mode}:
 * reason 1 = solve not converged (nothing of that iteration is applied), 2 = u too close to a cdf boundary,
 * 3 = degenerate weights (for 2 and 3 the solve of that iteration IS applied, the draw is not).  The caller
 * repeats that step another way and resumes.  Reason 4 (cell too large for the resident table) never leaves the call.
 * status_out[3] is, with sweeps_per_solve >= 2 (budgeted): the most sweeps any solve of this call needed;
 * 0 (step kernel): launches that did work; -1 (resident): centres handed to the step kernel.
 * One synchronisation at the end.
 * ------------------------------------------------------------------------------------------ */
size_t geo_kpp_workspace_bytes(int32_t n);
int32_t geo_kpp_resident_max_nodes(void);
int geo_kpp_chain(const int32_t *indptr, const int32_t *indices, const float *weights, int32_t n,
                  int32_t *centers, uint8_t *is_center, float *dmin, int32_t *argmin, const double *u_host,
                  int32_t it0, int32_t it1, int32_t n_centers_total, int32_t sweeps_per_solve,
                  int32_t assume_finite,
                  void *ws, size_t ws_bytes, int32_t *status_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Medoid update over a resident all-pairs matrix (extension: the reference stops after seeding + assignment,
 * src/geo/kmeans_optimized.py:141-183).  D f32 [n][ld] holds geodesic distances (rows filled by
 * geo_sssp_multi).  geo_cluster_costs: cost_out[i] = sum over the members j of i's cluster of D[i][j]^power
 * (power 1 or 2, fp64; members of cluster c = order[offsets[c] .. offsets[c+1]), `assign` i32 [n]).
 * geo_rows_argmin: for every column j the smallest D[rows[m]][j] and the first m attaining it (np.argmin's tie rule),
 * i.e. the re-assignment to the medoids `rows`.
 * ------------------------------------------------------------------------------------------ */
int geo_cluster_costs(const float *D, int64_t ld, const int32_t *assign, const int32_t *order,
                      const int32_t *offsets, int32_t n, int32_t power, double *cost_out, void *stream);
int geo_rows_argmin(const float *D, int64_t ld, const int32_t *rows, int32_t n_rows, int32_t n,
                    float *dmin_out, int32_t *argmin_out, void *stream);
/* geo_pam_swap_deltas: PAM's SWAP evaluation over the resident matrix (extension; FastPAM1 form).  For every
 * non-medoid candidate x: the medoid whose replacement by x lowers the total cost sum_j D[nearest(j)][j]^power most (first
 * medoid on ties) and that change.  nearest i32 [n]: position (0..K-1) of every node's nearest medoid; d1 / d2 f32 [n]:
 * distance to its nearest / second-nearest medoid; base f64 [K]: sum over the nodes of medoid i of (d2^power - d1^power);
 * is_medoid u8 [n].  K >= 2.  best_delta_out f64 [n] (+inf for medoids),
 * best_medoid_out i32 [n] (position in 0..K-1).  Reads D exactly once, row by row (n^2 * 4 bytes): HBM-bound.  K <= 3584. */
int geo_pam_swap_deltas(const float *D, int64_t ld, const int32_t *nearest, const float *d1, const float *d2,
                        const double *base, const uint8_t *is_medoid, int32_t n, int32_t K, int32_t power, double *best_delta_out,
                        int32_t *best_medoid_out, void *stream);
/* geo_attach_argmin: geodesic assignment of points outside the graph (the step the reference's notes call
 * assign_codes_val_geodesic.py, docs/results/cifar10_quantization_analysis.md:147; not in its repository).  Point v is
 * joined to graph nodes nbr[v][0..k) by edges of length len[v][0..k) (nbr < 0: no edge); Dt f32 [n][ld] holds the medoids'
 * distance rows transposed ([node][medoid]).  dist_out[v] = min over medoids m and edges u of len[v][u] + Dt[nbr[v][u]][m],
 * arg_out[v] = the first medoid attaining it (0 if none is reachable). */
int geo_attach_argmin(const float *Dt, int64_t ld, int32_t K, const int32_t *nbr, const float *len, int32_t k,
                      int64_t n_new, float *dist_out, int32_t *arg_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Cell-restricted medoid costs (extension; DESIGN.md "Cell-restricted medoid update"): the medoid update without the
 * all-pairs matrix, at any graph size.  (indptr, indices, weights): symmetric pull CSR, float32 weights >= 0, n < 2^27 nodes,
 * nnz < 2^31.  assign i32 [n] in [-1, K); order / offsets as for geo_cluster_costs: the members of cell c are
 * order[offsets[c] .. offsets[c+1]), ascending node index, offsets[K] = nodes with assign >= 0 (a node with assign < 0 is in
 * no cell).  The CUT graph keeps the entries whose two ends share a cell; d_c(i, j) is the shortest path in it under
 * geo_sssp_multi's rule (fp64 sums source-outward, run to the fixed point, rounded to float32, +inf when j cannot be
 * reached inside the cell).  cost_out f64 [n]: cost[i] = sum over the members j of i's cell, ascending, of
 * (double)d_c(i, j)^power with geo_cluster_costs's summation tree -- bit for bit geo_cluster_costs over the all-pairs matrix
 * of the cut graph -- and +inf for assign[i] < 0.  The unit of work is (cell, tile of geo_cell_costs_tile() sources); cells
 * of at most resident_nodes_max nodes (0 = geo_cell_costs_resident_max_nodes(), also the most it can be) keep a unit's
 * distance rows in LDS, larger cells in a slice of ws.  cost_out does not depend on the run, the stream, ws_bytes or
 * resident_nodes_max.  status_out (host i32 [4]): cells solved in LDS, cells solved through the workspace, most sweeps
 * of a unit, 0.  Before any launch: GEO_E_ARG for a null pointer, power outside {1, 2}, K < 1, n outside [1, 2^27);
 * GEO_E_WORKSPACE below geo_cell_costs_min_workspace_bytes(n, nnz, K, 0).  After the plan (one synchronisation): GEO_E_ARG when offsets[K] > n
 * or order / offsets / assign contradict each other, GEO_E_WORKSPACE below geo_cell_costs_min_workspace_bytes for the
 * largest cell found (one slice; geo_cell_costs_workspace_bytes sizes a slice for every workgroup in flight -- fewer slices
 * mean fewer large-cell units in flight, never another result).  GEO_E_NOCONV when a unit needs more than 65 536 sweeps (a
 * cell of m nodes needs at most m).  A failed call writes nothing to cost_out.  Synchronises.
 * ------------------------------------------------------------------------------------------ */
int32_t geo_cell_costs_tile(void);
int32_t geo_cell_costs_resident_max_nodes(void);
size_t geo_cell_costs_workspace_bytes(int32_t n, int64_t nnz, int32_t K, int32_t max_cell);
size_t geo_cell_costs_min_workspace_bytes(int32_t n, int64_t nnz, int32_t K, int32_t max_cell);
int geo_cell_costs(const int32_t *indptr, const int32_t *indices, const float *weights, int32_t n, int64_t nnz,
                   const int32_t *assign, const int32_t *order, const int32_t *offsets, int32_t K, int32_t power,
                   int32_t resident_nodes_max, double *cost_out, void *ws, size_t ws_bytes, int32_t *status_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * kNN search.  Replaces sklearn NearestNeighbors.kneighbors as called from
 * src/geo/knn_graph_optimized.py:40-42: exact n_neighbors nearest corpus rows (self included) of the
 * query rows [row0,row1) of z, ranked on fp64 squared distances, ties ordered by index.
 * form = 1: |x|^2 - 2 x.y + |y|^2 clamped at 0 (sklearn brute force, d > 15); form = 0: sum of squared
 * differences (sklearn kd-tree, d <= 15).  idx_out i32 [rows][n_neighbors], d2_out f64 likewise,
 * both sorted ascending.  n_neighbors <= GEO_KNN_MAX_NEIGHBORS (lists of up to 64 entries live one
 * per lane of the query's wave, longer ones two or four per lane; the float32 pre-filter serves
 * lists <= 64), d <= 128.
 * ------------------------------------------------------------------------------------------ */
#define GEO_KNN_MAX_NEIGHBORS 256
size_t geo_knn_workspace_bytes(int64_t n, int32_t d);
int geo_knn_topk(const float *z, int64_t n, int32_t d, int32_t n_neighbors, int32_t form,
                 int64_t row0, int64_t row1, int32_t *idx_out, double *d2_out,
                 void *ws, size_t ws_bytes, void *stream);

/* geo_knn_query: the same search for queries that are NOT rows of the corpus (sklearn's kneighbors(X)): for each of the m rows
 * of q (f32 [m][d]) the n_neighbors corpus rows of z with the smallest fp64 key, ordered by (key, corpus index).  The key is
 * the fma chain geo_knn_topk forms for `form` with the query in the place of the corpus' own row: form 0  sum (q - x)^2,
 * form 1  (|q|^2 + (-2 q.x)) + |x|^2 clamped at 0 with the fma-chain norms -- a query that is a copy of corpus row r gets
 * exactly row r's list of geo_knn_topk.  Same limits (d <= 128, n_neighbors <= min(GEO_KNN_MAX_NEIGHBORS, n), n, m < 2^31;
 * m = 0 is GEO_OK without a launch) and the same paths, chosen from n, d, n_neighbors and the option knn_filter alone.
 * The corpus is prepared once per call; the queries are prepared and searched in slices of as many rows as the workspace holds
 * behind the corpus side (candidate lists are per slice row, not per corpus row).  The result does not depend on ws_bytes.
 * geo_knn_query_workspace_bytes(n, m, d): one slice for all m queries; geo_knn_query_min_workspace_bytes(n, d): the corpus side
 * and one slice of 128 queries -- less is GEO_E_WORKSPACE before any launch. */
size_t geo_knn_query_workspace_bytes(int64_t n, int64_t m, int32_t d);
size_t geo_knn_query_min_workspace_bytes(int64_t n, int32_t d);
int geo_knn_query(const float *z, int64_t n, const float *q, int64_t m, int32_t d, int32_t n_neighbors, int32_t form,
                  int32_t *idx_out, double *d2_out, void *ws, size_t ws_bytes, void *stream);

/* The path the calling thread's last geo_knn_topk or geo_knn_query call took (host state only, no GPU call; 0 before any call,
 * after an empty row range / m = 0 or an argument error).  A geo_knn_query call that ran in several slices reports one path:
 * the one-level filter if any slice's first level overflowed, the OVERFLOW flag if any slice fell back to the exact scan.  The paths:
 *   GEO_KNN_PATH_EXACT        the exact fp64 scan of every pair (n_neighbors <= 64);
 *   GEO_KNN_PATH_EXACT_WIDE   the exact scan with lists of two or four entries per lane (n_neighbors > 64);
 *   GEO_KNN_PATH_FILTER_BF16  thresholds from a strided corpus subset (a bound), bf16 hi/lo matrix-core scan, fp64 refinement;
 *   GEO_KNN_PATH_FILTER_F32   the same with the float32 matrix-core scan (option knn_filter = 2);
 *   GEO_KNN_PATH_TWO_LEVEL    the bf16 filter whose thresholds come from a filtered pass over that subset themselves
 *                             (n >= 200 000);
 *   | GEO_KNN_PATH_OVERFLOW   added to a filter path when some query kept more candidates than its list holds and the
 *                             whole call was answered by the exact scan instead. */
#define GEO_KNN_PATH_EXACT 1
#define GEO_KNN_PATH_EXACT_WIDE 2
#define GEO_KNN_PATH_FILTER_BF16 3
#define GEO_KNN_PATH_FILTER_F32 4
#define GEO_KNN_PATH_TWO_LEVEL 5
#define GEO_KNN_PATH_OVERFLOW 16
int geo_knn_last_path(void);

/* The filter's thresholds on their own, for tests: tau_out f64 [row1 - row0] = the bound the filter paths take from every
 * stride-th corpus row (rows 0, stride, 2 stride, ...) for the query rows [row0,row1), before the eps margin.  Each lane of a
 * query's wave keeps the two (n_neighbors <= 24) or three smallest keys among the subset rows p with p % 64 = lane; tau is
 * the n_neighbors-th smallest of those 128 or 192 values: the key of a subset row, at least the n_neighbors-th smallest key
 * over the subset, hence over the corpus.  Runs at any n; n_neighbors <= min(64, subset rows); a workspace of 2 geo_knn_workspace_bytes(n, d) suffices. */
int geo_knn_thresholds(const float *z, int64_t n, int32_t d, int32_t n_neighbors, int32_t form,
                       int64_t row0, int64_t row1, int32_t stride, double *tau_out,
                       void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Bridging the components of a kNN graph (extension: the reference keeps the largest component and drops the rest).
 * z f32 [n][d], labels i32 [n] component numbers, form as for geo_knn_topk.  The PAIR KEY of nodes a != b is the fp64 key
 * geo_knn_topk gives corpus row hi = max(a, b) in the list of query row lo = min(a, b): form 0 the fma chain of
 * (lo_c - hi_c)^2, form 1 (|lo|^2 + (-2 lo.hi)) + |hi|^2 clamped at 0 -- in form 1 the norm added first is the one of the
 * lower index, whichever end asks.  Pairs are totally ordered by (key, lo, hi).
 *
 * geo_nearest_foreign: for each of the m query rows q = rows[i] (i32, any order, repeats allowed) the node x with
 * labels[x] != labels[q] that minimises (pair key, x): nbr_out i32 [m], key_out f64 [m]; a query whose label is every
 * node's gets -1 and +inf.  An exact fp64 scan of all m n pairs with knn_kernel's mapping (one wave owns a few queries,
 * every lane one candidate per 64-candidate step, one running (key, index) minimum per lane and query, a wave reduction at
 * the end).  Limits as geo_knn_topk: d <= 128, n < 2^31; m = 0 is GEO_OK without a launch; rows outside [0, n) are the
 * caller's error (not checked).  Workspace: geo_nearest_foreign_workspace_bytes(n, d), GEO_E_WORKSPACE below it.  The result
 * does not depend on ws_bytes, the stream or the run.
 *
 * geo_bridge_components: the edges of the minimum spanning tree of the component graph under that order (Kruskal over all
 * pairs with different labels): exactly C - 1 undirected edges, edges_out i32 [C-1][2] = (lo, hi) and keys_out f64 [C-1]
 * (both on the device), sorted by (key, lo, hi).  Computed by Boruvka rounds that leave the currently largest component
 * (lowest label on ties) out of the queries: query list from the current labels, geo_nearest_foreign's kernel, a
 * per-component (key, lo, hi) minimum with 64-bit integer atomicMin (key bits first, then the packed pair: no float
 * atomics, the same bits every run), one small read per round, union-find over the component numbers on the host, a
 * relabel on the device; at most ceil(log2 C) rounds.  labels must lie in [0, C) (GEO_E_ARG otherwise, found by the plan's
 * histogram before any output is written), every label in [0, C) must occur.  status_out i32 [4] ON THE HOST: rounds,
 * queries of the first round, queries of all rounds, 0.  C = 1: no edge, status 0 0 0 0.  Synchronises.  A failed call
 * writes nothing to the outputs.  Workspace: geo_bridge_components_workspace_bytes(n, d, C).
 * ------------------------------------------------------------------------------------------ */
size_t geo_nearest_foreign_workspace_bytes(int64_t n, int32_t d);
int geo_nearest_foreign(const float *z, int64_t n, int32_t d, int32_t form, const int32_t *labels, const int32_t *rows,
                        int64_t m, int32_t *nbr_out, double *key_out, void *ws, size_t ws_bytes, void *stream);
size_t geo_bridge_components_workspace_bytes(int64_t n, int32_t d, int32_t C);
int geo_bridge_components(const float *z, int64_t n, int32_t d, int32_t form, const int32_t *labels, int32_t C,
                          int32_t *edges_out, double *keys_out, int32_t *status_out, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Symmetrisation.  Replaces csr_matrix(...) + W.maximum/minimum(W.T) + setdiag(0) +
 * eliminate_zeros() of src/geo/knn_graph_optimized.py:54-66.
 * nbr_idx i32 [n][k] / nbr_w f32 [n][k] (NULL = connectivity, all ones) are the directed lists.
 * mode 0 = union (max), 1 = mutual (min).  Output is canonical CSR (columns ascending, no diagonal,
 * no stored zeros).  Two calls: geo_symmetrize_count fills indptr_out [n+1] and returns nnz through
 * nnz_out [host] (synchronises); the caller allocates indices/data and calls geo_symmetrize_fill
 * with the same workspace (its contents carry over).
 * An id outside [0, n) in nbr_idx (a padded list: -1, n, ...) is no entry: it is skipped, with its weight, as an out entry of
 * its row and never counted as an in entry of anything -- the result is that of the lists without it; a row may consist of
 * such ids only.  A row listing itself gives no entry (zero diagonal).  Inside one row the valid ids must be distinct (kNN
 * lists are; scipy would sum a repeated column).  Limits: n, k >= 1, n k < 2^30, mode 0 or 1 (GEO_E_ARG outside) and a
 * workspace of at least geo_symmetrize_workspace_bytes(n, k) (GEO_E_WORKSPACE below it), all checked before any launch.
 * The other calls of this group that take a workspace refuse one below their size query in the same way:
 * geo_connected_components and geo_upper_edges_count (which has no query of its own) are sized by geo_cc_workspace_bytes(n),
 * geo_csr_compact_count by geo_csr_compact_workspace_bytes(n).
 * Every array argument of these calls must be a non-NULL pointer even when it has no element (a graph without an entry:
 * indices / data of length 0, src / dst of no edge) -- NULL is GEO_E_ARG; such an array is never read or written, any valid
 * device address will do.  NULL is accepted only where a parameter says so (nbr_w, data, keep_node, entry_edge_out, data_out of geo_csr_compact_fill).
 * ------------------------------------------------------------------------------------------ */
size_t geo_symmetrize_workspace_bytes(int32_t n, int32_t k);
int geo_symmetrize_count(const int32_t *nbr_idx, const float *nbr_w, int32_t n, int32_t k, int32_t mode,
                         int32_t *indptr_out, int64_t *nnz_out, void *ws, size_t ws_bytes, void *stream);
int geo_symmetrize_fill(const int32_t *nbr_idx, const float *nbr_w, int32_t n, int32_t k, int32_t mode,
                        const int32_t *indptr, int32_t *indices_out, float *data_out,
                        void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Upper-triangle edge list in row-major order.  Replaces W.nonzero() + rows<cols of
 * src/scripts/build_codebook.py:43-45.  upper_ptr_out i32 [n+1] = exclusive count of entries with
 * col > row; n_edges through [host] pointer (synchronises).  geo_upper_edges_fill writes
 * src/dst i32 [E] and entry_edge i32 [nnz]: for every stored entry the index of its undirected
 * edge (so that W_geo = U + U^T of build_codebook.py:53-54 is a gather).  entry_edge is -1 for a stored diagonal entry and
 * for an entry below the diagonal whose mirror (col, row) is not stored; geo_gather_edge_weights writes 0.0 there.  Rows
 * must have ascending columns.
 * ------------------------------------------------------------------------------------------ */
int geo_upper_edges_count(const int32_t *indptr, const int32_t *indices, int32_t n,
                          int32_t *upper_ptr_out, int64_t *n_edges_out, void *ws, size_t ws_bytes, void *stream);
int geo_upper_edges_fill(const int32_t *indptr, const int32_t *indices, int32_t n, const int32_t *upper_ptr,
                         int32_t *src_out, int32_t *dst_out, int32_t *entry_edge_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Connected components.  Replaces scipy.sparse.csgraph.connected_components(directed=False) of
 * src/geo/knn_graph_optimized.py:175,187 for a structurally symmetric CSR.
 * labels_out i32 [n]: component numbers in order of each component's lowest node (scipy's order).
 * n_components through [host] pointer.  Synchronises.
 * ------------------------------------------------------------------------------------------ */
size_t geo_cc_workspace_bytes(int32_t n);
int geo_connected_components(const int32_t *indptr, const int32_t *indices, int32_t n,
                             int32_t *labels_out, int32_t *n_components_out,
                             void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * CSR filtering / compaction.  Replaces the scipy.sparse arithmetic of build_codebook.py:53-54
 * (entries that sum to exactly zero vanish) and the LCC sub-matrix W[mask][:, mask] (:59).
 * keep_node u8 [n] (NULL = all) selects rows/columns, entries with weight == 0 are dropped when
 * drop_zero != 0.  new_index_out i32 [n] = position of each kept node (-1 otherwise).
 * Two calls like symmetrize (count synchronises).
 * ------------------------------------------------------------------------------------------ */
size_t geo_csr_compact_workspace_bytes(int32_t n);
int geo_csr_compact_count(const int32_t *indptr, const int32_t *indices, const float *data, int32_t n,
                          const uint8_t *keep_node, int32_t drop_zero, int32_t *new_index_out,
                          int32_t *indptr_out, int32_t *n_out, int64_t *nnz_out,
                          void *ws, size_t ws_bytes, void *stream);
int geo_csr_compact_fill(const int32_t *indptr, const int32_t *indices, const float *data, int32_t n,
                         const uint8_t *keep_node, int32_t drop_zero, const int32_t *new_index,
                         const int32_t *indptr_new, int32_t *indices_out, float *data_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Inserting a few undirected edges into a canonical CSR (the bridges of geo_bridge_components).  src / dst i32 [E] and
 * w f32 [E] on the device; both directions of every edge are merged into the rows: columns stay ascending, existing
 * entries keep their weights, a pair that is already stored adds nothing, an edge listed twice counts once (its first
 * weight).  src == dst or an index outside [0, n) is GEO_E_ARG before any launch (the E edges are read back first: E is
 * tiny, nnz is not).  Two calls like symmetrize: geo_csr_insert_count fills indptr_out [n+1] and returns the new nnz through
 * nnz_out [host] (synchronises); geo_csr_insert_fill, with the same workspace (its contents carry over), writes
 * indices_out / data_out in one pass over the rows (data NULL = all ones).  E = 0 copies the graph.
 * Workspace: geo_csr_insert_workspace_bytes(n, E), GEO_E_WORKSPACE below it.
 * ------------------------------------------------------------------------------------------ */
size_t geo_csr_insert_workspace_bytes(int32_t n, int64_t E);
int geo_csr_insert_count(const int32_t *indptr, const int32_t *indices, int32_t n, const int32_t *src, const int32_t *dst,
                         const float *w, int64_t E, int32_t *indptr_out, int64_t *nnz_out,
                         void *ws, size_t ws_bytes, void *stream);
int geo_csr_insert_fill(const int32_t *indptr, const int32_t *indices, const float *data, int32_t n, int64_t E,
                        const int32_t *indptr_new, int32_t *indices_out, float *data_out,
                        void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Decoder pull-back edge lengths.  Replaces torch.autograd.functional.jvp through SpatialDecoder
 * (src/geo/riemannian_metric.py:12-35,37-66; src/models/spatial_vae.py:47-81):
 *   len[e] = 0.5 * ( |J(z[src[e]]) dz| + |J(z[dst[e]]) dz| ),  dz = z[dst[e]] - z[src[e]],
 * J = Jacobian of sigmoid(decoder(.)) at a 1x1 latent, edges processed in chunks of `batch_size`
 * consecutive edges (each endpoint side of a chunk is one BatchNorm batch when bn_train != 0).
 * ------------------------------------------------------------------------------------------ */
typedef struct geo_decoder_desc {
    int32_t latent_dim;        /* d */
    int32_t c0, c1, c2;        /* dec_channels */
    int32_t out_channels;      /* image channels */
    int32_t out_size;          /* 28 or 32 */
    int32_t norm;              /* 0 none, 1 batch, 2 group */
    int32_t bn_train;          /* batch statistics (decoder.training) */
    int32_t groups1, groups2;  /* GroupNorm group counts */
    float eps;
    /* device pointers, f32, torch layouts */
    const float *w_in, *b_in;              /* conv_in.weight [c0][d], bias [c0] */
    const float *w1, *b1;                  /* deconv_layers.0 weight [c0][c1][4][4], bias [c1] */
    const float *g1, *be1, *rm1, *rv1;     /* deconv_layers.1 (norm) weight, bias, running_mean, running_var */
    const float *w2, *b2;                  /* deconv_layers.3 weight [c1][c2][4][4], bias [c2] */
    const float *g2, *be2, *rm2, *rv2;     /* deconv_layers.4 */
    const float *w3, *b3;                  /* deconv_layers.6 weight [c2][out_channels][4][4], bias */
    /* train-mode BatchNorm also folds every batch into its running statistics (torch: momentum 0.1), once per decoder
     * call of riemannian_metric.py:57-58, i.e. per (chunk, start | end side) in order.  update_running != 0 (with
     * norm == 1, bn_train != 0 and the four rm / rv pointers non-null) does the same IN PLACE on rm1, rv1, rm2, rv2
     * (unbiased batch variance); num_batches_tracked (+2 per chunk) is the caller's to advance. */
    int32_t update_running;
    float momentum;
} geo_decoder_desc;

size_t geo_jvp_workspace_bytes(const geo_decoder_desc *dec, int64_t n_edges, int32_t batch_size);
/* Workspace of geo_decoder_jvp_edges including the per-latent buffers (primal ConvT2 output and output sigmoids of every
 * latent) that decoders with fixed statistics use: the primal pass then runs once per latent instead of once per edge end
 * (what riemannian_metric.py:57-58 recomputes for every edge).  With fixed statistics, latent_dim <= 16 and at least
 * 0.75 * latent_dim edges per latent the call goes one step further and computes the decoder Jacobian once per latent (its
 * latent_dim columns, n_nodes * latent_dim * 32 or 192 floats of this workspace), each edge end from those columns: same
 * quantity, another summation order (within 1e-6 of the per-edge-end lengths; option jvp_node_jacobian = 0 turns it off).
 * A workspace of geo_jvp_workspace_bytes() still works: the call then takes the per-edge-end path.
 * The edges-per-latent rule counts the edges of the call.  A caller that computes a graph's lengths in several calls (the ranks of
 * a sharded build, or slices in one process) uses the *_part forms below and tells each call the edge count of the whole build:
 * the two routes differ in their last bits, and only then do all parts take the route the whole graph would. */
size_t geo_jvp_edges_workspace_bytes(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int32_t batch_size);
int geo_decoder_jvp_edges(const geo_decoder_desc *dec, const float *z, int64_t n_nodes,
                          const int32_t *src, const int32_t *dst, int64_t n_edges, int32_t batch_size,
                          float *len_out, void *ws, size_t ws_bytes, void *stream);
/* The same call for n_edges edges that are a part of a build of build_edges edges over the same latents (build_edges >= n_edges,
 * else GEO_E_ARG before any launch; build_edges = n_edges is geo_decoder_jvp_edges itself).  build_edges enters the
 * edges-per-latent rule above and nothing else: passes, slots and the workspace are sized by the call's own n_edges.  For decoders
 * with fixed statistics the lengths then do not depend on how the edges of a build are divided among calls or ranks, provided every
 * call is told the build's edge count AND is given at least the workspace its own geo_jvp_edges_part_workspace_bytes query sizes
 * (the route also depends on ws_bytes: a part with less room, e.g. geo_jvp_workspace_bytes() only, falls back to the per-edge-end
 * path whatever the build's count): both routes compute an edge from its own two latents alone.  (Train-mode BatchNorm never
 * takes the Jacobian route; its lengths depend on the chunks, which a caller keeps whole.) */
size_t geo_jvp_edges_part_workspace_bytes(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int64_t build_edges,
                                          int32_t batch_size);
int geo_decoder_jvp_edges_part(const geo_decoder_desc *dec, const float *z, int64_t n_nodes,
                               const int32_t *src, const int32_t *dst, int64_t n_edges, int64_t build_edges, int32_t batch_size,
                               float *len_out, void *ws, size_t ws_bytes, void *stream);

/* Which kernels a geo_decoder_jvp_edges (graph_edges != 0) or geo_decoder_jvp_pairs (graph_edges = 0, n_nodes ignored) call with
 * these sizes runs under the current options: the decision the call itself makes, host arithmetic only (no GPU call).
 * ws_bytes = 0: a workspace as sized by the matching *_workspace_bytes query.  Negative (GEO_E_*, text in geo_last_error)
 * where the call would refuse the decoder or the workspace. */
#define GEO_JVP_FRONT_VALU 0        /* front_kernel */
#define GEO_JVP_FRONT_MFMA 1        /* front_mfma_kernel */
#define GEO_JVP_MID_PIPE 0          /* mid_pipe_kernel over every tile */
#define GEO_JVP_MID_PIPE_DEDUP 1    /* mid_pipe_kernel over the end side + mid_start_kernel (start rows once per run of equal src) */
#define GEO_JVP_MID_ALL 2           /* mid_all_kernel */
#define GEO_JVP_MID_ALL_TANGENT 3   /* mid_all_kernel, tangent only, behind the per-node primal pass */
#define GEO_JVP_MID_CHUNK 4         /* mid_bf16_kernel */
#define GEO_JVP_BACK_MFMA 0         /* back_mfma_kernel, primal + tangent per slot */
#define GEO_JVP_BACK_PER_NODE 1     /* back_mfma_kernel: primal once per latent, tangent per slot */
#define GEO_JVP_BACK_DEDUP 2        /* back_mfma_kernel: end side per slot, start-side primal once per run of equal src */
#define GEO_JVP_BACK_VALU 3         /* back_kernel */
#define GEO_JVP_PLAN_FRONT(p) ((p) & 3)
#define GEO_JVP_PLAN_DMAX(p) (16 << (((p) >> 2) & 3))   /* compiled latent width of the front kernel: 16, 32, 64 */
#define GEO_JVP_PLAN_MID(p) (((p) >> 4) & 15)
#define GEO_JVP_PLAN_BACK(p) (((p) >> 8) & 15)
#define GEO_JVP_PER_NODE 0x1000      /* flag: primal pass once per latent */
#define GEO_JVP_NODE_JACOBIAN 0x2000 /* flag: decoder Jacobian once per latent, edge ends from its columns */
#define GEO_JVP_DEDUP 0x4000         /* flag: start-side primal rows once per run of equal src */
#define GEO_JVP_FRONT_ONCE 0x8000    /* flag: front_edge_kernel, the first layer once per edge (tangent) and per run of equal src (start primal) */
#define GEO_JVP_PLAN_PASSES(p) ((p) >> 16)              /* passes over the (pseudo-)edges, capped at 32767 */
int geo_jvp_plan(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int32_t batch_size, int32_t graph_edges,
                 size_t ws_bytes);
/* ... of a geo_decoder_jvp_edges_part call (graph_edges != 0; build_edges >= n_edges, else GEO_E_ARG) */
int geo_jvp_plan_part(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int64_t build_edges, int32_t batch_size,
                      int32_t graph_edges, size_t ws_bytes);
/* Does that call (workspace as sized by the matching query) run ConvT3 with head_stream_kernel?  1: the 16-output head without
 * GroupNorm on back route MFMA or DEDUP with option jvp_head_stream != 0 (default; GEO_JVP_HEAD_STREAM); 0: back_mfma_kernel /
 * back_kernel.  Both compute the same bits.  Negative (GEO_E_*) where geo_jvp_plan is.  The plan code has no free bit for it. */
int geo_jvp_head_stream(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int32_t batch_size, int32_t graph_edges);

/* Same quantity for explicit endpoint arrays (edge_lengths_riemannian's own signature):
 * z_start / z_end f32 [E][d]. */
int geo_decoder_jvp_pairs(const geo_decoder_desc *dec, const float *z_start, const float *z_end,
                          int64_t n_edges, int32_t batch_size, float *len_out,
                          void *ws, size_t ws_bytes, void *stream);

/* The pull-back metric tensor itself, per latent: G(z) = J(z)^T J(z), J as above (p_out x d, float32 columns from the tangent pass
 * over the d unit tangents -- the column pass of the per-latent Jacobian route, run on its own), its eigenvalues, the volume
 * element and the numerical rank.
 *   G_out      [n][d][d] fp64: G[a][b] = sum over o < p_out of (double)J[a][o] * (double)J[b][o], o ascending (each product is
 *              exact in fp64); the upper triangle is computed and mirrored, so G[a][b] and G[b][a] are the same bits
 *   eig_out    [n][d] fp64, ascending: cyclic Jacobi on G in a fixed rotation order (may be null)
 *   logvol_out [n] fp64: 0.5 * log det G = 0.5 * sum_i log(eig_i) if every eigenvalue is > 0, else -inf (may be null)
 *   rank_out   [n] int32: #{ i : sqrt(eig_i) > max(p_out, d) * FLT_EPSILON * sqrt(eig_max) }, numpy's matrix_rank rule on the
 *              singular values of the float32 Jacobian (may be null)
 * G = 0 gives eig = 0, rank = 0, logvol = -inf.  Float32 columns determine G's entries and its large eigenvalues; where G is nearly
 * singular (16 outputs from 16 latent dimensions: cond(G) up to 1e9) they do not determine the smallest eigenvalues or logvol.
 * Covered: what the per-latent Jacobian route covers -- fixed statistics (norm 0, norm 1 with bn_train == 0, norm 2 with 32
 * groups per layer), latent_dim <= 16, c1 in {32, 64, 128}, c2 == 64, 16, 32 or 192 outputs.  Not covered: train-mode BatchNorm (a
 * sample's Jacobian depends on its batch), latent_dim > 16, other widths: geo_metric_tensor_workspace_bytes and
 * geo_metric_tensor_min_workspace_bytes answer 0 and the call returns GEO_E_ARG before any launch, as it does for a null pointer
 * and for a workspace below geo_metric_tensor_min_workspace_bytes (the columns of one 32-latent slice; a call with n < 32 also
 * takes its own geo_metric_tensor_workspace_bytes(dec, n)).  The call always runs the column pass: it reads neither the option
 * jvp_node_jacobian nor an edges-per-latent rule, and where another option switches off a kernel the pass needs (jvp_per_node = 0,
 * jvp_mid = 2, jvp_back_valu) the queries answer 0 and the call refuses likewise instead of changing route.
 * Latents are processed in slices sized from ws_bytes (at most 2^18 latents, which is what the query sizes for a larger n).  A
 * latent's outputs are a function of its own row of z alone: the same bits for any n, position, slice length, stream and earlier
 * workspace contents.  n == 0 returns GEO_OK without a launch.  No atomics. */
size_t geo_metric_tensor_workspace_bytes(const geo_decoder_desc *dec, int64_t n);
size_t geo_metric_tensor_min_workspace_bytes(const geo_decoder_desc *dec);
int geo_decoder_metric_tensor(const geo_decoder_desc *dec, const float *z, int64_t n, double *G_out, double *eig_out,
                              double *logvol_out, int32_t *rank_out, void *ws, size_t ws_bytes, void *stream);

/* Curves under the pull-back metric: the discrete energy of C curves of F frames each, and its monotone relaxation with the ends
 * fixed.  x is f32 [C][F][d], 2 <= F <= 64.  Same decoder, same J and same output sigmoids g as
 * geo_decoder_metric_tensor: the per-node primal pass and the column pass over the C * F latents; coverage and refusals as there.
 * Evaluate(x), a function of the curve's own F rows, every sum one fp64 accumulator over ascending indices, nothing contracted:
 *   seg_sq[f]  = sum_o ((double)g[f+1][o] - (double)g[f][o])^2, f = 0 .. F-2;      E = sum_f seg_sq[f]
 *   grad[f][k] = 2 * sum_o (double)J[f][k][o] * (((double)g[f][o] - g[f-1][o]) - ((double)g[f+1][o] - g[f][o])), interior f;
 *                grad[0] = grad[F-1] = 0 exactly
 *   tr[f]      = sum_k (sum_o (double)J[f][k][o]^2)
 * and E = NaN for a curve with a NaN or an inf among its F * d coordinates, whatever the passes made of it.
 * geo_curve_energy: energy_out f64 [C]; seg_sq_out f64 [C][F-1], grad_out f64 [C][F][d], g_out f32 [C][F][p_out] and jac_out
 * f32 [C][F][d][p_out] (unpadded) may each be null.
 * geo_curve_relax: x_inout is relaxed in place, n_iters trial steps per curve, each curve on its own and decided on the device.
 * The call evaluates x (energy0_out, may be null).  step_inout f64 [C]: a step < 0 becomes 1 / (8 * max over interior f of tr[f]),
 * 0 where that maximum is 0 (also with n_iters == 0).  Each iteration: y[f] = (float)((double)x[f] - step * grad[f]) for interior f,
 * the ends copied; Evaluate(y); if E_y < E (a NaN on either side is a rejection) then x, E, grad <- y's, step *= 2 and
 * accepted += 1, else step /= 4.  energy_out f64 [C] and accepted_out i32 [C] are required, seg_sq_out f64 [C][F-1] may be null.
 * E can only fall; n iterations of one call leave the bits n calls of one iteration leave.  F == 2 or n_iters == 0 evaluates only.
 * GEO_E_ARG before any launch, the reason in geo_last_error: a decoder geo_decoder_metric_tensor does not cover (train-mode
 * BatchNorm included; both queries answer 0 for it), F outside [2, 64], n_iters < 0, C < 0, a null required pointer, a workspace
 * below geo_curve_min_workspace_bytes (one curve's).  C == 0 returns GEO_OK without a launch.
 * Slices are whole curves, sized from ws_bytes (at most 2^18 latents, which is what the query sizes for more); the packed weights
 * are written once per slice, not once per iteration.  A curve's outputs are a function of its own rows: the same bits for any
 * C, position, slice length, stream and earlier workspace contents; a NaN or inf stays in its curve, which comes back unchanged
 * with accepted == 0.  No atomics. */
size_t geo_curve_workspace_bytes(const geo_decoder_desc *dec, int64_t C, int32_t F);
size_t geo_curve_min_workspace_bytes(const geo_decoder_desc *dec, int32_t F);
int geo_curve_energy(const geo_decoder_desc *dec, const float *x, int64_t C, int32_t F, double *energy_out, double *seg_sq_out,
                     double *grad_out, float *g_out, float *jac_out, void *ws, size_t ws_bytes, void *stream);
int geo_curve_relax(const geo_decoder_desc *dec, float *x_inout, int64_t C, int32_t F, int32_t n_iters, double *step_inout,
                    double *energy0_out, double *energy_out, double *seg_sq_out, int32_t *accepted_out, void *ws, size_t ws_bytes,
                    void *stream);

/* ------------------------------------------------------------------------------------------
 * K-quad weights and the chain order, shared by the native pull-back, decode, encode and LPIPS below.
 * A convolution weight read as a matrix [K][N] (K = input channels of one tap, N = output channels) is packed
 * [K / 4][N][4]: element (q, n, r) = weight (k = 4 q + r, column n); the descriptors give each tensor's own element formula.
 * An output value is one chain from 0 over the taps, then over the input channels in blocks of 8, within a block in the
 * order 0 4 1 5 2 6 3 7 ("the K-quad chain order" below); bias, folded norm and ReLU come after the chain.
 * ------------------------------------------------------------------------------------------ */

/* ------------------------------------------------------------------------------------------
 * The same quantity for the vanilla (vector-latent) VAE decoder with FIXED statistics (src/models/vae.py:53-85 in eval mode:
 * BatchNorm with running statistics, or no normalisation):
 *   fc: Linear(d, c0 16) -> view c0x4x4 -> ConvT(c0,c1,k3,s2,p1[,output_padding]) -> norm -> ReLU
 *       -> ConvT(c1,c2,k4,s2,p1) -> norm -> ReLU -> ConvT(c2,C,k4,s2,p1) -> sigmoid;   4 -> 7 -> 14 -> 28 px | 4 -> 8 -> 16 -> 32 px.
 * Everything up to the first norm's scale and shift is affine in z and arrives composed (in fp64, rounded once):
 *   pre1[n] = c[n] + sum_k z[k] At[k][n],  n = (y s1 + x) c1 + channel,  s1 = out_size / 4,  n1 = s1^2 c1.
 * Covered: 1 <= latent_dim <= 128, (c1, c2) = (128, 64) or (64, 32), out_channels 1 or 3, out_size 28 or 32.
 * ------------------------------------------------------------------------------------------ */
typedef struct geo_vanilla_decoder_desc {
    int32_t latent_dim;        /* d */
    int32_t c1, c2;            /* dec_channels[1], dec_channels[2] */
    int32_t out_channels;      /* C */
    int32_t out_size;          /* 28 or 32 */
    /* device pointers, f32 */
    const float *At;           /* [d rounded up to even][n1]; the padding row is zero */
    const float *c;            /* [n1] */
    const float *w2p;          /* ConvT2 weight w2 [c1][c2][4][4] as [parity 2 py + px][tap 2 a + b][c1 / 4][c2][4]:
                                  element (.., q, co, r) = w2[4 q + r][co][2 a + 1 - py][2 b + 1 - px] */
    const float *scale2;       /* [c2] second norm folded: pre2 = scale2 * ConvT2(h1) + shift2 (ConvT2's bias inside shift2) */
    const float *shift2;       /* [c2] */
    const float *w3p;          /* ConvT3 weight w3 [c2][C][4][4] as [parity][tap][C][c2], same parity / tap meaning */
    const float *b3;           /* [C] */
    /* the transposed packs of geo_vanilla_vjp alone; every other entry point ignores them and accepts them null */
    const float *w2t;          /* w2 as [tap 4 ky + kx][c2 / 4][c1][4]: element (tap, q, ci, r) = w2[ci][4 q + r][ky][kx] */
    const float *w3t;          /* w3 as [tap 4 ky + kx][C][c2]: element (tap, c, ci) = w3[ci][c][ky][kx] */
    const float *Atq;          /* At as [n1 / 4][dn][4], dn = d rounded up to a multiple of 32: element (q, k, r) = At[k][4 q + r],
                                  0 for k >= d */
} geo_vanilla_decoder_desc;

/* Workspace of geo_vanilla_jvp_pairs for n_edges edges; 0 for a descriptor outside the coverage above (host arithmetic).
 * The calls cut the edges into passes that fit the workspace they are given: any size from
 * geo_vanilla_jvp_workspace_bytes(dec, 1) (the minimum: one edge per pass) upwards is legal for BOTH calls, a smaller
 * workspace only means more passes, and no length depends on the number of passes. */
size_t geo_vanilla_jvp_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n_edges);
/* Workspace with which geo_vanilla_jvp_edges runs the per-point work (ReLU masks, sigmoid') once per latent when
 * n_nodes <= 2 n_edges (it holds every latent's masks); with less, or with fewer edges, once per edge end. */
size_t geo_vanilla_jvp_edges_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n_nodes, int64_t n_edges);
/* z_start / z_end f32 [E][d] -> len_out f32 [E].  batch_size is accepted and ignored: with fixed statistics the value does
 * not depend on it.  Fixed-order f32 chains, no atomics: bit-identical across runs, streams, workspace sizes and between the
 * two entry points; z_start[e] == z_end[e] gives exactly 0.  Asynchronous on `stream`. */
int geo_vanilla_jvp_pairs(const geo_vanilla_decoder_desc *dec, const float *z_start, const float *z_end, int64_t n_edges,
                          int32_t batch_size, float *len_out, void *ws, size_t ws_bytes, void *stream);
/* z f32 [n_nodes][d] resident, src / dst i32 [E] in [0, n_nodes) (the caller checks them). */
int geo_vanilla_jvp_edges(const geo_vanilla_decoder_desc *dec, const float *z, int64_t n_nodes, const int32_t *src,
                          const int32_t *dst, int64_t n_edges, int32_t batch_size, float *len_out, void *ws, size_t ws_bytes,
                          void *stream);

/* Vector-Jacobian product of the same decoder: with g(z) = sigmoid(decoder(z)) flattened to
 * nout = C S S values ([C][S][S]) and J = dg/dz,  out[i] = J(z_i)^T u_i,  z_i = z[index ? index[i] : i].
 * z f32 [.][d], index NULL or i32 [n], u f32 [n][nout], out f64 [n][d]; the descriptor's w2t, w3t and Atq are required.
 * The masks and sigmoid' come from the point pass of geo_vanilla_jvp_pairs; the three layers are walked backwards in f32 and
 * the last product is summed in fp64, every value a fixed-order chain of its own item, no atomics: a row's bits do not depend
 * on n, its position, index, the pass size, the stream or earlier workspace contents; u_i = 0 gives exactly 0.  The items are
 * cut into passes that fit the workspace: any size from geo_vanilla_vjp_min_workspace_bytes(dec) upwards is legal (a smaller
 * one: GEO_E_WORKSPACE).  The queries answer 0 for a descriptor outside the coverage and the call rejects it (GEO_E_ARG) before
 * any launch.  n == 0 returns GEO_OK without a launch; n < 2^31.  Asynchronous on `stream`. */
size_t geo_vanilla_vjp_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n);
size_t geo_vanilla_vjp_min_workspace_bytes(const geo_vanilla_decoder_desc *dec);
int geo_vanilla_vjp(const geo_vanilla_decoder_desc *dec, const float *z, const int32_t *index, int64_t n, const float *u, double *out,
                    void *ws, size_t ws_bytes, void *stream);

/* Curve energy and relaxation under the vanilla decoder: the definitions, the loop and the rules of
 * geo_curve_energy / geo_curve_relax above (section 26), with g(z) = sigmoid(decoder(z)) [nout] and the gradient by
 * geo_vanilla_vjp's passes instead of a Jacobian.  x f32 [C][F][d], 2 <= F <= 64:
 *   seg_sq[f] = |g[f+1] - g[f]|^2 from the f32 outputs in fp64: thread t of 256 adds the squares of outputs t, t + 256, ... in
 *               ascending order (one accumulator from 0, product and sum separate), then p[t] += p[t + s], s = 128, 64, .., 1
 *   E = sum_f seg_sq[f] ascending;  NaN for a curve with a NaN or an inf among its coordinates
 *   r[f] = (g[f] - g[f-1]) - (g[f+1] - g[f]) in fp64, rounded once to f32;  grad[f] = 2 J(x[f])^T r[f], 0 at the ends
 *   trace[f] = sum_k |J(x[f]) e_k|^2, each square norm in f32 by the tangent kernels of geo_vanilla_jvp_pairs, summed over k
 *              ascending in fp64
 * energy f64 [C]; seg_sq f64 [C][F-1], grad f64 [C][F][d], g_out f32 [C][F][nout], trace_out f64 [C][F] may each be null.  The
 * trace (d tangents per frame) is computed only where asked for: by trace_out, or in geo_vanilla_curve_relax for a slice that
 * holds a curve with step_inout < 0, which then starts from 1 / (8 max interior trace).  Curves are cut into slices of whole
 * curves that fit the workspace: any size from geo_vanilla_curve_min_workspace_bytes(dec, F) upwards is legal and no bit depends
 * on it, nor on C, a curve's position, the stream or earlier workspace contents.  geo_vanilla_curve_relax reads step_inout once
 * on the host before its first launch (it synchronises the stream there) and decides every iteration on the device; n iterations
 * in one call are the bits of n calls of one iteration continued through step_inout.  Uncovered descriptor: queries 0, calls
 * GEO_E_ARG before any launch. */
size_t geo_vanilla_curve_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t C, int32_t F);
size_t geo_vanilla_curve_min_workspace_bytes(const geo_vanilla_decoder_desc *dec, int32_t F);
int geo_vanilla_curve_energy(const geo_vanilla_decoder_desc *dec, const float *x, int64_t C, int32_t F, double *energy_out,
                             double *seg_sq_out, double *grad_out, float *g_out, double *trace_out, void *ws, size_t ws_bytes,
                             void *stream);
int geo_vanilla_curve_relax(const geo_vanilla_decoder_desc *dec, float *x_inout, int64_t C, int32_t F, int32_t n_iters,
                            double *step_inout, double *energy0_out, double *energy_out, double *seg_sq_out, int32_t *accepted_out,
                            void *ws, size_t ws_bytes, void *stream);

/* The pull-back metric tensor of the same decoder per latent: with g and J as for geo_vanilla_vjp,
 *   G(z_i) = J(z_i)^T J(z_i),  z_i = z[index ? index[i] : i].
 * z f32 [.][d], index NULL or i32 [n]; G_out f64 [n][d][d], required; jac_out f32 [n][d][nout], the columns J[.][k] themselves,
 * may be null; eig_out f64 [n][d], logvol_out f64 [n], rank_out i32 [n]: all three or none (a mixed triple: GEO_E_ARG).
 * Coverage is geo_vanilla_jvp_pairs's; the transposed packs are not read.  The columns are the unit tangents of
 * geo_vanilla_curve_energy's trace pushed through the tangent kernels in f32; G[a][b] = sum over o of
 * (double)J[a][o] * (double)J[b][o], exact products added in an order that depends on (d, nout) alone (outputs in chunks of
 * 64 ascending, each chunk in groups of four on v_mfma_f64_16x16x4_f64), the lower triangle written from the upper: G == G^T
 * bit for bit, and no bit of G, jac_out or the spectrum depends on n, a latent's position, index, the workspace size, the
 * stream or earlier workspace contents.  The spectrum is geo_sym_spectrum's on G with p_out = nout.  Latents run in slices
 * (pairs of latents) sized from ws_bytes: any size from geo_vanilla_metric_min_workspace_bytes(dec) -- one pair -- upwards is
 * legal (a smaller one: GEO_E_WORKSPACE).  The queries answer 0 for a descriptor outside the coverage and the call rejects it
 * (GEO_E_ARG, as a null required pointer) before any launch.  n == 0 returns GEO_OK without a launch; n < 2^31.
 * Asynchronous on `stream`: no atomics, no host synchronisation. */
size_t geo_vanilla_metric_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n);
size_t geo_vanilla_metric_min_workspace_bytes(const geo_vanilla_decoder_desc *dec);
int geo_vanilla_metric_tensor(const geo_vanilla_decoder_desc *dec, const float *z, const int32_t *index, int64_t n, double *G_out,
                              float *jac_out, double *eig_out, double *logvol_out, int32_t *rank_out, void *ws, size_t ws_bytes,
                              void *stream);

/* Eigenvalues of n symmetric matrices G f64 [n][d][d], 1 <= d <= 128 (csrc/sym_spectrum.hip); only the
 * upper triangle a <= b of each matrix is read.  eig_out f64 [n][d] ascending; with emax the largest,
 *   rank   = #{ i : eig_i > 0 and sqrt(eig_i) > max(p_out, d) * FLT_EPSILON * sqrt(emax) },
 *   logvol = 0.5 * sum_i log(eig_i), ascending, if every eigenvalue is > 0, else -inf
 * (the rules of geo_decoder_metric_tensor).  G = 0 gives eig = 0, rank = 0, logvol = -inf.  One workgroup holds a matrix in LDS
 * and runs parallel-order cyclic Jacobi on a fixed round-robin schedule until every off-diagonal entry is exactly 0 (at most
 * geo_sym_spectrum_sweep_cap() sweeps); a matrix's results are a function of the matrix alone.  A matrix with a NaN or an inf
 * among the entries read gives eig NaN, logvol NaN, rank 0 and leaves the other matrices' results untouched.  d outside
 * [1,128], n < 0, p_out < 1 or (n > 0) a null pointer: GEO_E_ARG before any launch; n == 0: GEO_OK.  Asynchronous on `stream`.
 * Diagnostics, for tests and measurements, not for pipelines: geo_sym_spectrum_sweeps is the same call and also writes the sweeps
 * each matrix took to sweeps_out i32 [n]; geo_sym_spectrum_sweep_cap() is the kernel's sweep cap. */
int geo_sym_spectrum(const double *G, int64_t n, int32_t d, int32_t p_out, double *eig_out, double *logvol_out, int32_t *rank_out,
                     void *stream);
int geo_sym_spectrum_sweeps(const double *G, int64_t n, int32_t d, int32_t p_out, double *eig_out, double *logvol_out,
                            int32_t *rank_out, int32_t *sweeps_out, void *stream);
int32_t geo_sym_spectrum_sweep_cap(void);

/* ------------------------------------------------------------------------------------------
 * Image decode: latents or codes -> the decoder's raw output (before any sigmoid), f32 NCHW
 * [n][C][S][S].  Only the primal chain of the kernels above: no masks, no sigmoid'; the workspace is the two activation
 * buffers of a pass.  Rules of both entries: every output value is a fixed-order fmaf chain of its own row, no atomics; a
 * row's logits do not depend on n, its position in the batch, the pass size, the workspace size, the stream or the run, nor
 * on whether its latent arrived directly or through index / (table, codes).  Any workspace from *_workspace_bytes(dec, 1)
 * upwards is legal (a smaller one: GEO_E_WORKSPACE); *_workspace_bytes answers 0 for a descriptor outside the coverage and
 * the call rejects it (GEO_E_ARG, as a null pointer, before any launch).  n == 0 returns GEO_OK without a launch;
 * n < 2^31.  Index and code ranges are the caller's duty.  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------ */
size_t geo_vanilla_decode_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n);
/* The vanilla decoder (geo_vanilla_decoder_desc, same coverage): row i decodes z[index ? index[i] : i]; z f32 [.][d],
 * index NULL or i32 [n].  A quantized batch is z = z_medoid, index = codes: no gathered copy. */
int geo_vanilla_decode(const geo_vanilla_decoder_desc *dec, const float *z, const int32_t *index, int64_t n, float *logits_out,
                       void *ws, size_t ws_bytes, void *stream);

/* The spatial decoder with FIXED statistics (src/models/spatial_vae.py:47-81 in eval mode: BatchNorm with running
 * statistics, or no normalisation), decoding whole 4 x 4 latent grids:
 *   conv_in: Conv(d,c0,1) -> ConvT(c0,c1,k4,s2,p1) -> norm -> ReLU -> ConvT(c1,c2,k4,s2,p1) -> norm -> ReLU
 *       -> ConvT(c2,C,k4,s2,p 1 | 3);   4 -> 8 -> 16 -> 32 px, or 28 px = rows and columns 2 .. 29 of the 32-px output.
 * conv_in arrives composed into ConvT1 (in fp64, rounded once), per output-pixel parity and tap as for w2p.  conv_in's bias
 * reaches an 8 x 8 pixel only through the taps that lie inside the 4 x 4 grid, so it is no per-channel constant: it rides
 * as input channel d, held at 1 inside the grid (and, like every channel, 0 outside it).  With dp = d + 1 rounded up to a
 * multiple of 8 (the padding channels are zero):
 *   pre1[(2 y + py, 2 x + px)][co] = shift1[co] + scale1[co] * sum over taps (a, b), k < dp of
 *                                    in[(y + py - a, x + px - b)][k] * W[2 py + px][2 a + b][k][co].
 * Covered: 1 <= latent_dim <= 64, (c1, c2) = (128, 64) or (64, 32) (any c0), out_channels 1 or 3, out_size 28 or 32. */
typedef struct geo_spatial_image_decoder_desc {
    int32_t latent_dim;        /* d */
    int32_t c1, c2;            /* dec_channels[1], dec_channels[2] */
    int32_t out_channels;      /* C */
    int32_t out_size;          /* 28 or 32 */
    /* device pointers, f32 */
    const float *w1p;          /* W as [parity][tap][dp / 4][c1][4]: element (.., q, co, r) = W[..][4 q + r][co];
                                  W[..][k][co] = sum_c0 w_in[c0][k] w1[c0][co][2 a + 1 - py][2 b + 1 - px] for k < d,
                                  sum_c0 b_in[c0] w1[c0][co][..][..] for k = d, 0 above */
    const float *scale1;       /* [c1] first norm folded (ConvT1's bias inside shift1) */
    const float *shift1;       /* [c1] */
    const float *w2p;          /* as in geo_vanilla_decoder_desc */
    const float *scale2;       /* [c2] */
    const float *shift2;       /* [c2] */
    const float *w3p;          /* [parity][tap][C][c2] */
    const float *b3;           /* [C] */
    /* the transposed packs of geo_spatial_vjp and the grid curves alone; geo_spatial_decode ignores them and accepts them null */
    const float *w1t;          /* the composed first stage as [tap 4 ky + kx][c1 / 4][dn][4], dn = d rounded up to a multiple of 32:
                                  element (tap, q, k, r) = scale1[4 q + r] * sum_c0 w_in[c0][k] w1[c0][4 q + r][ky][kx] for k < d
                                  (in fp64, rounded once), 0 above; the bias channel has no gradient */
    const float *w2t;          /* as in geo_vanilla_decoder_desc */
    const float *w3t;          /* as in geo_vanilla_decoder_desc */
} geo_spatial_image_decoder_desc;

size_t geo_spatial_decode_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int64_t n);
/* Exactly one of z (f32 [n][d][4][4], NCHW) and (table f32 [K][d], codes i32 [n][16] in (y, x) order) is given; with the
 * latter, position p of image i is table[codes[i][p]] -- how build_codebook's codes quantize a grid. */
int geo_spatial_decode(const geo_spatial_image_decoder_desc *dec, const float *z, const float *table, const int32_t *codes,
                       int64_t n, float *logits_out, void *ws, size_t ws_bytes, void *stream);

/* Vector-Jacobian product of the same decoder on whole grids: with g(z) = sigmoid(decoder(z)) of a 4 x 4
 * grid z, flattened to nout = C S S values ([C][S][S], S = out_size; at 28 px rows and columns 2 .. 29 of the 32-px output) and
 * J = dg/dz over the grid's 16 d coordinates,  out[i] = J(z_i)^T u_i,  z_i = z[index ? index[i] : i].
 * z f32 [.][d][4][4], index NULL or i32 [n], u f32 [n][nout], out f64 [n][d][4][4]; the descriptor's w1t, w2t and w3t are required.
 * The masks and sigmoid' come from a point pass of geo_spatial_decode's chains; the second and third layer are walked backwards by
 * geo_vanilla_vjp's kernels, the first by a K-quad chain over the c1 channels of each 8 x 8 pixel (2 y - 1 + ky, 2 x - 1 + kx)
 * inside the image, the pixels of a grid position added in fp64 in ascending (ky, kx) order.  No atomics, every value a
 * fixed-order chain of its own item: a row's bits do not depend on n, its position, index, the pass size, the stream or earlier
 * workspace contents; u_i = 0 gives exactly 0.  Any workspace from geo_spatial_vjp_min_workspace_bytes(dec) upwards is legal (a
 * smaller one: GEO_E_WORKSPACE).  The queries answer 0 for a descriptor outside geo_spatial_decode's coverage and the call rejects
 * it (GEO_E_ARG) before any launch.  n == 0 returns GEO_OK without a launch; n < 2^31.  Asynchronous on `stream`. */
size_t geo_spatial_vjp_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int64_t n);
size_t geo_spatial_vjp_min_workspace_bytes(const geo_spatial_image_decoder_desc *dec);
int geo_spatial_vjp(const geo_spatial_image_decoder_desc *dec, const float *z, const int32_t *index, int64_t n, const float *u,
                    double *out, void *ws, size_t ws_bytes, void *stream);

/* Curve energy and relaxation of image curves under the whole spatial decoder: the definitions, the loop
 * and the rules of geo_vanilla_curve_energy / geo_vanilla_curve_relax above with a frame = one grid, d := 16 d coordinates in NCHW
 * order, g and J as for geo_spatial_vjp.  x f32 [C][F][d][4][4], 2 <= F <= 64; energy f64 [C]; seg_sq f64 [C][F-1],
 * grad f64 [C][F][d][4][4], g_out f32 [C][F][nout], probe_out f64 [C][F] may each be null.  One rule differs, the first step: in
 * place of the trace,
 *   probe[f] = sum over the 16 d coordinates k, ascending, in fp64, of (J(x[f])^T s)[k]^2,
 *   s[c][y][x] = +1 where c + y + x is even, else -1 (indices of the S x S output),
 * a one-sample estimate of tr J J^T (not a bound), and a step_inout < 0 becomes 1 / (8 max over interior f of probe[f]), 0 where
 * that maximum is 0 (a NaN is ignored).  The probe (one more VJP per frame) is computed only where asked for: by probe_out, or in
 * geo_spatial_curve_relax for a slice that holds a curve with step_inout < 0.  Slices, the workspace rule, the host read of
 * step_inout, "n iterations in one call are the bits of n calls of one" and the refusals are geo_vanilla_curve_relax's. */
size_t geo_spatial_curve_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int64_t C, int32_t F);
size_t geo_spatial_curve_min_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int32_t F);
int geo_spatial_curve_energy(const geo_spatial_image_decoder_desc *dec, const float *x, int64_t C, int32_t F, double *energy_out,
                             double *seg_sq_out, double *grad_out, float *g_out, double *probe_out, void *ws, size_t ws_bytes,
                             void *stream);
int geo_spatial_curve_relax(const geo_spatial_image_decoder_desc *dec, float *x_inout, int64_t C, int32_t F, int32_t n_iters,
                            double *step_inout, double *energy0_out, double *energy_out, double *seg_sq_out, int32_t *accepted_out,
                            void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Image encode: images -> (mu, logvar) of the encoder of either VAE with FIXED statistics
 * (src/models/vae.py:22-50, src/models/spatial_vae.py:22-44 in eval mode: BatchNorm with running statistics, or none):
 *   Conv(C,e1,k3,s2,p1) -> norm -> ReLU -> Conv(e1,e2,k3,s2,p1) -> norm -> ReLU -> Conv(e2,e3,k3,s2,p1) -> norm -> ReLU,
 *   28 -> 14 -> 7 -> 4 px or 32 -> 16 -> 8 -> 4 px, then the head: fc_mu, fc_logvar = Linear(16 e3, d) on the NCHW flatten
 *   (spatial_head 0; mu, logvar f32 [n][d]) or Conv(e3, d, 1) (spatial_head 1; mu, logvar f32 NCHW [n][d][4][4]).
 * Activations are f32 [item][pixel][channel]; layer i computes relu(scale_i[co] * sum + shift_i[co]) with the sum a chain
 * from 0 (layer 1: over (c, ky, kx); layers 2, 3: over tap 3 ky + kx in the K-quad chain order), output pixel (oy, ox)
 * reading input pixel (2 oy - 1 + ky, 2 ox - 1 + kx), nothing outside the image.  A head value is bh[col] added to the sum, in segment order, of one such chain per segment: 16
 * segments (the 4 x 4 pixels) of e3 channels for the vanilla head, one for the spatial head.
 * Covered: (C, in_size) = (1, 28) or (3, 32); (e1, e2, e3) = (64, 128, 256) or (32, 64, 128); 1 <= latent_dim <= 128
 * (spatial_head 0) or <= 64 (spatial_head 1).  The rules are those of the image decode above: passes of at most 4096
 * items shrunk to fit any workspace from geo_image_encode_workspace_bytes(enc, 1) upwards (the three activation buffers of
 * a pass; below it GEO_E_WORKSPACE); the query answers 0 and the call GEO_E_ARG for a descriptor outside the coverage, as
 * for a null pointer or n >= 2^31, before any launch; n == 0 returns GEO_OK without a launch.  No atomics: a row's
 * (mu, logvar) does not depend on n, its position, the pass or workspace size, the stream or the run.  Asynchronous on
 * `stream`.  x is the tensor the module would be given (normalisation is the caller's).
 * ------------------------------------------------------------------------------------------ */
typedef struct geo_image_encoder_desc {
    int32_t in_channels;       /* C */
    int32_t in_size;           /* 28 or 32 */
    int32_t e1, e2, e3;        /* enc_channels */
    int32_t latent_dim;        /* d */
    int32_t spatial_head;      /* 0: Linear heads on the flatten, 1: 1 x 1 convolution heads */
    /* device pointers, f32 */
    const float *w1p;          /* [9 C][e1]: row (c 3 + ky) 3 + kx, element = conv1.weight[co][c][ky][kx] */
    const float *scale1;       /* [e1] norm i folded, convolution i's bias inside shift_i */
    const float *shift1;       /* [e1] */
    const float *w2p;          /* [9][e1 / 4][e2][4]: element (tap, q, co, r) = conv2.weight[co][4 q + r][ky][kx], tap = 3 ky + kx */
    const float *scale2;       /* [e2] */
    const float *shift2;       /* [e2] */
    const float *w3p;          /* [9][e2 / 4][e3][4], as w2p */
    const float *scale3;       /* [e3] */
    const float *shift3;       /* [e3] */
    const float *whp;          /* [segments][e3 / 4][npad][4], npad = 2 d rounded up to a multiple of 32, columns 0 .. d-1 mu,
                                  d .. 2d-1 logvar, 0 above: element (p, q, col, r) = fc.weight[col][(4 q + r) 16 + p] (vanilla, 16
                                  segments: the module's flatten index is channel * 16 + pixel) or fc.weight[col][4 q + r] (spatial) */
    const float *bh;           /* [npad] the two biases, 0 above 2 d */
} geo_image_encoder_desc;

size_t geo_image_encode_workspace_bytes(const geo_image_encoder_desc *enc, int64_t n);   /* 0: not covered */
int geo_image_encode(const geo_image_encoder_desc *enc, const float *x /* [n][C][S][S] */, int64_t n, float *mu_out,
                     float *logvar_out, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * LPIPS: LPIPS v0.1, AlexNet backbone, normalize = False, spatial = False, of n pairs of f32
 * 3 x 64 x 64 images in [-1, 1] (what lpips.LPIPS(net='alex') returns for them; src/eval/evaluate_model.py:110-142):
 *   scaled = (x - shift) / scale per channel, shift = (-.030, -.088, -.188), scale = (.458, .448, .450), zero-padded AFTER scaling;
 *   Conv(3,64,k11,s4,p2) ReLU -> f1 (15 x 15); MaxPool(3,s2) Conv(64,192,k5,p2) ReLU -> f2 (7 x 7); MaxPool(3,s2)
 *   Conv(192,384,k3,p1) ReLU -> f3 (3 x 3); Conv(384,256,k3,p1) ReLU -> f4; Conv(256,256,k3,p1) ReLU -> f5;
 *   d_l = mean over pixels of sum_c lin_l[c] (u0 - u1)^2 with u = f / (sqrt(sum_c f^2) + 1e-10); value = d_1 + ... + d_5.
 * The features are f32 [image][pixel][channel], each value one chain from 0 (layer 1: over c, ky, then the kx pairs (0, 1) ..
 * (10, -); layers 2 .. 5: over tap KS ky + kx in the K-quad chain order), the bias added last; the distance is fp64 from
 * those features: channel sums folded by an xor butterfly of 64 partials, the pixel mean in pixel order, the layer sum in layer order.  total_out f64 [n]; layer_out f64 [n][5] or
 * NULL.  The rules are those of the image encode above: passes of at most 4096 pairs shrunk to fit any workspace from
 * geo_lpips_alex_workspace_bytes(1) upwards (the five feature buffers of both images of a pass, 254 976 bytes per pair; below
 * it GEO_E_WORKSPACE); a null pointer or n >= 2^31 returns GEO_E_ARG before any launch; n == 0 returns GEO_OK without a
 * launch.  No atomics: a pair's result does not depend on n, its position, which image is x0, the pass or workspace size,
 * the stream or the run.  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------ */
typedef struct geo_lpips_alex_desc {
    /* device pointers, f32 */
    const float *w1p;          /* [33 = c 11 + ky][2 = h][64 = co][8]: element s < 6 = conv1.weight[co][c][ky][2 s + h], 0 where
                                  2 s + h = 11 and for s = 6, 7 */
    const float *b1;           /* [64] */
    const float *w2p;          /* [25][64 / 4][192][4]: element (tap, q, co, r) = conv2.weight[co][4 q + r][ky][kx], tap = 5 ky + kx */
    const float *b2;           /* [192] */
    const float *w3p;          /* [9][192 / 4][384][4], as w2p with tap = 3 ky + kx */
    const float *b3;           /* [384] */
    const float *w4p;          /* [9][384 / 4][256][4] */
    const float *b4;           /* [256] */
    const float *w5p;          /* [9][256 / 4][256][4] */
    const float *b5;           /* [256] */
    const float *lin1, *lin2, *lin3, *lin4, *lin5;   /* [64] [192] [384] [256] [256] */
} geo_lpips_alex_desc;

size_t geo_lpips_alex_workspace_bytes(int64_t n);
int geo_lpips_alex(const geo_lpips_alex_desc *net, const float *x0, const float *x1 /* [n][3][64][64] */, int64_t n,
                   double *total_out /* [n] */, double *layer_out /* [n][5] or NULL */, void *ws, size_t ws_bytes, void *stream);

/* Gather: data_out[e] = len[entry_edge[e]] for every stored entry (W_geo = U + U^T). */
int geo_gather_edge_weights(const float *len, const int32_t *entry_edge, int64_t nnz, float *data_out, void *stream);

/* ---- the code prior's training step (src/models/transformer.py:98-133, src/scripts/train_transformer.py:39-66) ----
 * Fused causal multi-head attention for sequences of at most 16 tokens.  qkv f32 [B][T][3][H][head_dim] (the c_attn
 * projection's output), head_dim in {16, 32, 64}; out f32 [B][T][H*head_dim]; probs f32 [B][H][T][T] receives the softmax
 * rows (kept for the backward pass); keep u8 [B][H][T][T] (1 = kept) or NULL applies dropout to them with
 * keep_scale = 1 / (1 - p).  Replaces q @ k^T * scale -> masked_fill(-inf) -> softmax -> dropout -> @ v
 * (transformer.py:121-129).  Asynchronous on `stream`. */
int geo_prior_attention_fwd(const float *qkv, const uint8_t *keep, float keep_scale, int32_t B, int32_t T, int32_t H,
                            int32_t head_dim, float *out, float *probs, void *stream);
/* Gradient of the above with respect to qkv: dqkv f32 [B][T][3][H][head_dim] from dout f32 [B][T][H*head_dim]. */
int geo_prior_attention_bwd(const float *qkv, const float *probs, const uint8_t *keep, float keep_scale, const float *dout,
                            int32_t B, int32_t T, int32_t H, int32_t head_dim, float *dqkv, void *stream);
/* torch.optim.AdamW's update (train_transformer.py:39-43,64-66: decoupled weight decay, bias-corrected moments) over ONE
 * flat buffer of n floats in a single pass.  lr_dev f32 [1] and step_dev i64 [1] (the 1-based step count of THIS update) are
 * read on the device, so the launch does not change from step to step.  The hyper-parameters are doubles, as torch holds
 * them: 1 - beta is formed in double before it is rounded to float.  Asynchronous on `stream`. */
int geo_prior_adamw(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, const float *lr_dev,
                    const int64_t *step_dev, double beta1, double beta2, double eps, double weight_decay, void *stream);

/* ---- sampling from the code prior (src/scripts/generate_samples.py:12-31: sample, top_k_logits) ----
 * The model: dims, the flat f32 parameter arena (vqvae_amd/prior/transformer.py, Transformer.layout) and the float offsets of
 * its tensors.  Every weight matrix starts on 16 bytes.  class_emb = -1 for an unconditional model. */
typedef struct {
    int32_t num_tokens, embed_dim, n_layers, n_head, max_seq_len, num_classes;
    const float *arena;
    int64_t pos_emb, token_emb, class_emb, ln_f_w, ln_f_b, head_w;
    /* [host] n_layers x 12 offsets: ln1.weight, ln1.bias, ln2.weight, ln2.bias, attn.c_attn.weight, attn.c_attn.bias,
     * attn.c_proj.weight, attn.c_proj.bias, mlp.0.weight, mlp.0.bias, mlp.2.weight, mlp.2.bias */
    const int64_t *block;
} geo_prior_desc;

/* Workspace of geo_prior_sample for B rows and n_positions = T0 + steps - 1 decoded positions (KV cache, activations,
 * logits).  0 for invalid arguments. */
size_t geo_prior_sample_workspace_bytes(const geo_prior_desc *model, int32_t B, int32_t n_positions);

/* KV-cached autoregressive decode of B rows: tokens_out i64 [B][T0 + steps] = the prompt i64 [B][T0] followed by `steps`
 * drawn tokens, the standard causal mask, dropout off (eval).  y i64 [B] class labels or NULL.  uniforms f32 [B][steps] in
 * [0, 1) pick the tokens by the draw rule: l = logits / temperature; with top_k > 0 keep every l_i >= the k-th largest
 * (ties kept); p = exp(l - max l) over the kept set; the token is the smallest i whose prefix sum exceeds u * sum(p), else
 * the last kept index.  top_k = 0: no filter.  logits_out f32 [B][T0 + steps - 1][V] or NULL receives the logits of every
 * position (teacher-forced over the prompt).  Covered: max_seq_len <= 16, head_dim in {16, 32, 64}, embed_dim a multiple
 * of 64 and <= 512, num_tokens <= 1024; T0 >= 1, T0 + steps - 1 <= max_seq_len.  Prompt tokens and labels must be in
 * range (the caller checks; the kernels clamp their embedding lookups).  No global state: concurrent calls on different
 * streams with their own workspaces and outputs are independent.  Asynchronous on `stream`. */
int geo_prior_sample(const geo_prior_desc *model, const int64_t *prompt, int32_t T0, int32_t steps, const int64_t *y,
                     const float *uniforms, float temperature, int32_t top_k, int64_t *tokens_out, float *logits_out,
                     int32_t B, void *ws, size_t ws_bytes, void *stream);

/* ---- Euclidean k-means (sklearn.cluster.KMeans, lloyd, k-means++; the reference's demos/codebook_comparison.py:73-77) ----
 * X f32 [n][d] (row-major, 1 <= d <= 128), centres f32 [K][d], 1 <= K <= min(n, 4096).  The key of row x and centre c is the
 * fp64 fma chain of (x_k - c_k)^2 over k ascending; labels are argmin_j key with ties to the lowest j.  One workspace query
 * serves all three calls (n_starts / n_trials as given to geo_kmeans_pp; 1 / 1 for the other two).  No float atomics: every
 * output is bit-identical across runs, streams and workspace sizes.  0 for invalid arguments. */
size_t geo_kmeans_workspace_bytes(int64_t n, int32_t d, int32_t K, int32_t n_starts, int32_t n_trials);

/* labels_out i32 [n], keys_out f64 [n] (may be NULL) = the key of the chosen centre.  A float32 matrix-core screen decides
 * most rows; rows within its proven error margin (kmeans.hip) are re-keyed exactly against every centre ("fallback rows"):
 * n_fallback_out [host, may be NULL] receives their number (synchronises when given).  Non-finite input is outside the
 * covered envelope; the fallback still ranks a NaN key first, so every label is in [0, K). */
int geo_kmeans_assign(const float *X, int64_t n, int32_t d, const float *C, int32_t K, int32_t *labels_out, double *keys_out,
                      int64_t *n_fallback_out, void *ws, size_t ws_bytes, void *stream);

/* k-means++ seeding of n_starts starts at once (sklearn _kmeans_plusplus, unit weights).  first_host [host] i32 [n_starts]
 * = the first centre of each start (rs.choice), u_host [host] f64 [n_starts][K-1][n_trials] = the uniforms of each later
 * step.  Step c: closest = f32(key) min-folded over the chosen centres; candidate t = the first row i whose fp64 cumulative
 * sum of closest (fixed association: 1024-row segments) reaches u * pot, clipped to n - 1; candidate pots = f32 of the
 * fixed-order fp64 sum of min(closest, f32(key to the candidate)); the first minimum wins and becomes pot.  pot of step 1
 * = f32 of the fp64 sum of closest.  indices_out i32 [n_starts][K] (device), centers_out f32 [n_starts][K][d] or NULL.
 * 1 <= n_trials <= 64, n <= 7 000 000.  Synchronises once, after taking the host arrays; the rest is asynchronous. */
int geo_kmeans_pp(const float *X, int64_t n, int32_t d, int32_t K, int32_t n_starts, int32_t n_trials, const int32_t *first_host,
                  const double *u_host, int32_t *indices_out, float *centers_out, void *ws, size_t ws_bytes, void *stream);

/* Lloyd iterations of sklearn _kmeans_single_lloyd for each of n_starts starts, init f32 [n_starts][K][d].  Iteration: exact
 * labels; per-cluster fp64 sums in ascending row order; empty clusters (ascending) take the rows farthest from their old
 * centre by (key descending, row ascending) unless every key is 0; centre = f32(sum / count), a cluster left empty takes the
 * row sklearn's _average_centers gives it (the biggest cluster's, kmeans.hip); shift2 = fp64 |new - old|^2.
 * Stops on unchanged labels (strict; never in the first iteration), else when the fp64 sum of shift2 <= tol, else at
 * max_iter; without strict convergence the rows are relabelled once with the final centres.  centers_out f32
 * [n_starts][K][d], labels_out i32 [n_starts][n] (device); inertia_out f64 (fp64 sum of the keys), n_iter_out i32,
 * strict_out i32 (may be NULL) [host] [n_starts]; n_fallback_out [host, may be NULL] = fallback rows over all assignments.
 * Synchronises once per batch of iterations. */
int geo_kmeans_lloyd(const float *X, int64_t n, int32_t d, int32_t K, int32_t n_starts, const float *init, int32_t max_iter,
                     double tol, float *centers_out, int32_t *labels_out, double *inertia_out, int32_t *n_iter_out,
                     int32_t *strict_out, int64_t *n_fallback_out, void *ws, size_t ws_bytes, void *stream);

/* ---- Evaluation metrics: per-image pair moments (the reductions of PSNR and SSIM; reference src/eval/metrics.py) ----
 * x, y f32 [n_images][n_pix] (device, contiguous), 1 <= n_pix <= 16384, 0 <= n_images < 2^31.  mom_out f64 [n_images][6] =
 * mean_x, mean_y, var_x, var_y, cov_xy (biased, centred on the fp64 means in a second pass), sse = sum (x - y)^2, all
 * accumulated in fp64.  Fixed reduction order that depends on n_pix alone, no atomics: bit-identical across runs, streams,
 * batch sizes and positions in the batch.  Asynchronous on `stream`. */
int geo_image_pair_moments(const float *x, const float *y, int64_t n_images, int64_t n_pix, double *mom_out, void *stream);

/* ---- Geodesic k-medoids analysis (the reference's demos/kmedoids_geodesic_analysis.py) ----
 * geo_cluster_label_scores: assign i32 [n] (codes in [0, K); negative = not assigned, skipped), labels i32 [n] (classes in
 * [0, C)), 1 <= K <= 4096, 1 <= C <= 1024, 0 <= n < 2^31 (GEO_E_ARG outside, before any launch: every pair count below is at
 * most C(n, 2) < 2^61 and a workgroup's int32 cells cannot wrap).  grid_blocks = workgroups of the counting kernel, 0 =
 * chosen from n.  table_out i64 [K][C] = the contingency table n_kc; row_counts_out i64 [K] = a_k (code usage);
 * col_counts_out i64 [C] = b_c; isums_out i64 [6] = rows counted, sum_k max_c n_kc (purity numerator), sum C(n_kc, 2),
 * sum C(a_k, 2), sum C(b_c, 2), rows skipped because a code >= K or a label lay outside [0, C) (the caller's error: they are
 * in no count); fsums_out f64 [3] = sum n_kc log n_kc, sum a_k log a_k, sum b_c log b_c.  Integer counting (LDS per
 * workgroup, 64-bit integer merge), fp64 sums in an association fixed by (K, C): every output is bit-identical across
 * runs, streams and grid sizes.  Asynchronous. */
int geo_cluster_label_scores(const int32_t *assign, const int32_t *labels, int64_t n, int32_t K, int32_t C, int32_t grid_blocks,
                             int64_t *table_out, int64_t *row_counts_out, int64_t *col_counts_out, int64_t *isums_out,
                             double *fsums_out, void *stream);

/* PCA of the distance-to-medoid features X = D^T (plot_pca_with_clusters of the demo): D f32 [K][ld], row k = distances from
 * medoid k to the n nodes (geo_sssp_multi's D_out), 1 <= K <= 4096, 1 <= n < 2^31, ld >= n.  A non-finite entry of row k
 * counts as fill[k] = fl32(fl32(1.1) m_k), m_k = the row's largest finite value, 1 when that is 0 (or the row has no finite
 * entry): numpy's float32 arithmetic on the reference's float32 X.  One workspace query serves colstats and gram.
 * geo_feature_colstats: colmax_out f32 [K] = m_k (0 for a row without finite entries), fill_out f32 [K], mean_out f64 [K] =
 *   fp64 mean of the row after replacement (16 384-column slices, fixed tree, slices in order).
 * geo_feature_gram: gram_out f64 [K][K] = sum_v (x_iv - mean_i)(x_jv - mean_j), v_mfma_f64_16x16x4_f64 on 64 x 64 tiles of the
 *   upper block triangle, the n columns cut into slices fixed by (n, K) whose partial matrices are added in slice order;
 *   the lower triangle is the mirror image, so gram_out is exactly symmetric.
 * geo_feature_project: Z_out f32 [n][n_components] = (x_v - mean) V, V f64 [K][n_components], 1 <= n_components <= min(K, 8),
 *   fp64 fma chain over k ascending, rounded once.
 * No atomics anywhere: bit-identical across runs and streams.  Asynchronous. */
size_t geo_feature_workspace_bytes(int64_t n, int32_t K);
int geo_feature_colstats(const float *D, int64_t ld, int32_t K, int64_t n, float *colmax_out, float *fill_out, double *mean_out,
                         void *ws, size_t ws_bytes, void *stream);
int geo_feature_gram(const float *D, int64_t ld, int32_t K, int64_t n, const float *fill, const double *mean, double *gram_out,
                     void *ws, size_t ws_bytes, void *stream);
int geo_feature_project(const float *D, int64_t ld, int32_t K, int64_t n, const float *fill, const double *mean, const double *V,
                        int32_t n_components, float *Z_out, void *stream);

/* ---- Riemannian graph experiments (the reference's experiments/geo/run_riemann_experiments.py) ----
 * geo_path_stats: D f32 [n_rows][ld] (geo_sssp_multi's D_out, or any rows of it), n_rows >= 1, n >= 1 columns read per row,
 * ld >= n; a row may start at any 4-byte aligned address.  Per row r: sum_out f64 [r] = the fp64 sum of the entries that are
 * finite and > 0, n_pos_out i64 [r] = how many those are, n_unreached_out i64 [r] = the number of +inf entries, max_out f32 [r]
 * = the largest finite entry (0 when the row has none).  One workgroup per row; the association of the fp64 sum depends on
 * n alone, there are no atomics: a row's outputs are bit-identical across runs, streams and whatever other rows share the
 * call.  Asynchronous. */
int geo_path_stats(const float *D, int64_t ld, int32_t n_rows, int64_t n, double *sum_out, int64_t *n_pos_out,
                   int64_t *n_unreached_out, float *max_out, void *stream);

/* geo_csr_set_symmetric: data[(src[t], dst[t])] = data[(dst[t], src[t])] = val[t] for t < m on a CSR of n rows whose rows are
 * sorted by column (binary search).  The m pairs must be unique as unordered pairs (the caller's contract: two threads
 * would otherwise store to one entry).  A pair with either entry absent, or an endpoint outside [0, n), stores nothing and
 * adds one to n_missing_out i32 [1] (device; set to 0 first).  0 <= m < 2^31; m = 0 only clears the counter.  Asynchronous. */
int geo_csr_set_symmetric(const int32_t *indptr, const int32_t *indices, float *data, int32_t n, const int32_t *src,
                          const int32_t *dst, const float *val, int64_t m, int32_t *n_missing_out, void *stream);

/* ---- Geodesic paths and points along them (an extension) ----
 * The walk inputs: P i32, S rows of leading dimension ld >= n (geo_sssp_multi's P_out, or a strided view of it), sources i32 [S]
 * (the solve's), and M pairs rows i32 [M] (a row of P) / targets i32 [M] (a node).  Pair m starts at targets[m] and follows
 * P[rows[m]][.] until sources[rows[m]].
 * geo_sssp_paths_count: hops_out i32 [M] = the number of edges (0 when the target is the source), status_out i32 [M] =
 *   0 source reached | 1 unreachable: a node other than the source whose predecessor is the sentinel -9999, at the target or
 *   in mid-walk | 2 malformed: max_hops edges walked without reaching the source, a predecessor outside [0, n), or a row /
 *   target / source that is no index.  hops_out = -1 for status 1 and 2.  Status 2 is a real outcome on graphs with
 *   zero-weight edges (or weights below one ulp of the distance): two nodes at equal distance can name each other.
 *   0 <= max_hops <= n - 1.  Every predecessor is checked before it is used: nothing outside P's S x ld block is read.
 * geo_sssp_paths_fill: offsets i64 [M + 1] = the exclusive prefix sum of hops + 1 over the status-0 pairs (0 slots for the
 *   others), T = offsets[M].  For a status-0 pair, nodes_out i32 [T] holds on [offsets[m], offsets[m + 1]) the path's nodes
 *   source -> target and cum_out f64 [T] its running length: cum[0] = 0, cum[i] = cum[i - 1] + (double)w_i, one rounding per
 *   hop, w_i = the minimum weight among the entries of row node[i] of the pull CSR (indptr / indices / weights, the graph the
 *   solve ran on; weights == NULL = unit weights) whose index is node[i - 1] (+inf when there is none).  That is the solver's
 *   accumulation order: (float)cum[hops] == D[row][target] bit for bit.
 * geo_polyline_resample: z f32 [n][d]; frames_out f32 [M][F][d], F >= 2, receives F points per path at equal arc length:
 *   frame 0 = z[node[0]] and frame F - 1 = z[node[hops]] exactly; frame f between them sits at s = cum[hops] * f / (F - 1)
 *   (fp64, the product first), in segment i = the largest i <= hops - 1 with cum[i] <= s, at u = (s - cum[i]) / (cum[i + 1] -
 *   cum[i]) (0 when the denominator is 0), and is a + u * (b - a) of the two node latents in fp64 without contraction,
 *   rounded once to f32.  A path of 0 hops repeats its latent; a pair with an empty slice leaves its F d outputs untouched.
 *   The straight chord of two nodes is the polyline nodes = [a, b], cum = [0, 1].
 * Limits: n, S >= 1, 0 <= M < 2^31, M F < 2^32; GEO_E_ARG outside and for a null pointer, before any launch; M == 0 returns
 * GEO_OK without a launch.  No workspace, no atomics: outputs are bit-identical across runs and streams.  Asynchronous. */
int geo_sssp_paths_count(const int32_t *P, int64_t ld, int32_t S, const int32_t *sources, const int32_t *rows,
                         const int32_t *targets, int64_t M, int32_t n, int32_t max_hops, int32_t *hops_out, int32_t *status_out,
                         void *stream);
int geo_sssp_paths_fill(const int32_t *P, int64_t ld, int32_t S, const int32_t *sources, const int32_t *rows,
                        const int32_t *targets, int64_t M, int32_t n, const int32_t *indptr, const int32_t *indices,
                        const float *weights, const int64_t *offsets, int64_t T, int32_t *nodes_out, double *cum_out,
                        void *stream);
int geo_polyline_resample(const float *z, int64_t n, int32_t d, const int32_t *nodes, const int64_t *offsets, const double *cum,
                          int64_t M, int32_t F, float *frames_out, void *stream);

/* ---- EMA vector quantizer (the reference's baseline VQ-VAE, VectorQuantizerEMA) ----
 * z_e [B][C][HW] (NCHW, contiguous) f32 (half = 0) or f16 (half = 1), 1 <= C <= 128, 1 <= K <= 4096, any n = B HW >= 1 (K > n
 * allowed).  Rows are z_e's positions (b, h, w) in that order, upcast to f32.  idx_out i64 [n] = geo_kmeans_assign's labels
 * of the rows against embed f32 [K][C] (fp64 key, ties to the lowest code; a NaN key comes first, so a row holding a NaN or
 * an infinity -- every key NaN or +inf -- gets code 0, and every label is in [0, K)).  z_q_out f32 NCHW = embed[idx] before the
 * update; z_q_st_out f32 NCHW = fl32(z_e + fl32(z_q - z_e)).  loss_out f32 [1] = fl32(beta) * fl32(mean (z_q_st - z_e)^2);
 * stats_out f32 [4] = q_mse (mean (z_q - z_e)^2), perplexity exp(-sum p log(p + 1e-12)), usage, dead of the batch's counts;
 * the means are fp64 sums in a fixed association.  counts_out i32 [K] or NULL.  training != 0: the EMA update of
 * cluster_size f32 [K], embed_avg f32 [K][C] and embed, in place, from the integer counts and the fp64 per-code sums in
 * ascending row order.  No float atomics: bit-identical across runs, streams and workspace sizes.  Asynchronous. */
size_t geo_vq_workspace_bytes(int64_t n, int32_t d, int32_t K);
int geo_vq_forward(const void *z_e, int32_t half, int32_t B, int32_t C, int32_t HW, float *embed, float *cluster_size,
                   float *embed_avg, int32_t K, int32_t training, double decay, double eps, double beta, float *z_q_out,
                   float *z_q_st_out, int64_t *idx_out, float *loss_out, float *stats_out, int32_t *counts_out, void *ws,
                   size_t ws_bytes, void *stream);
/* grad_out (z_e's dtype) = cast(g_st + fl32(fl32(g_loss beta) fl32(2 / numel)) (z_e - z_q_st)), evaluated in f32 and rounded
 * once.  g_st f32 [numel] and g_loss f32 [1] (device) may be NULL (zero).  Asynchronous. */
int geo_vq_backward(const float *g_st, const float *g_loss, double beta, const void *z_e, int32_t half, const float *z_q_st,
                    int64_t numel, void *grad_out, void *stream);

/* ---- ELBO of the vanilla VAE (reference src/models/vae.py VAE.loss) ----
 * x_logits, x f32 [B][P]; mu, logvar f32 [B][d] (device, contiguous); 1 <= B, P, d < 2^31.
 *   recon = (1 / B) sum of  BCE: max(l, 0) - l x + log1p(exp(-|l|))  |  MSE_SIGMOID: (sigmoid(l) - x)^2  |  MSE_LOGITS: (l - x)^2
 *   kl    = (1 / B) sum of  max(k, free_bits) when has_free_bits, else k;   k = -0.5 (1 + logvar - mu^2 - exp(logvar))
 *   reg   = kl (capacity OFF)  |  |kl - capacity_target| (ABS)  |  max(kl - capacity_target, 0) (CLIPPED)
 * geo_vae_elbo_forward: out f64 [4] (device) = recon + beta reg, recon, kl, reg.  Terms in fp64 from the f32 inputs;
 *   per-workgroup partials in ws, then one ordered pass; no atomics: bit-identical across runs and streams.
 * geo_vae_elbo_backward: grad_total f64 [1] (device) = the gradient of out[0]; out = the forward's (kl is read on the device).
 *   d_logits f32 [B][P], d_mu, d_logvar f32 [B][d], each an fp64 value rounded once.  Free bits: zero where k < free_bits,
 *   passed at equality (torch.clamp's backward); ABS: sign(kl - target), 0 at 0; CLIPPED: passed where kl - target >= 0.
 * geo_vae_elbo_workspace_bytes: 0 for shapes outside the limits.  Neither call synchronises. */
#define GEO_VAE_RECON_BCE 0
#define GEO_VAE_RECON_MSE_SIGMOID 1
#define GEO_VAE_RECON_MSE_LOGITS 2
#define GEO_VAE_CAPACITY_OFF 0
#define GEO_VAE_CAPACITY_ABS 1
#define GEO_VAE_CAPACITY_CLIPPED 2
size_t geo_vae_elbo_workspace_bytes(int64_t B, int64_t P, int64_t d);
int geo_vae_elbo_forward(const float *x_logits, const float *x, const float *mu, const float *logvar, int64_t B, int64_t P,
                         int64_t d, int32_t recon_mode, int32_t has_free_bits, double free_bits, double beta,
                         double capacity_target, int32_t capacity_mode, double *out, void *ws, size_t ws_bytes, void *stream);
int geo_vae_elbo_backward(const double *grad_total, const double *out, const float *x_logits, const float *x, const float *mu,
                          const float *logvar, int64_t B, int64_t P, int64_t d, int32_t recon_mode, int32_t has_free_bits,
                          double free_bits, double beta, double capacity_target, int32_t capacity_mode, float *d_logits,
                          float *d_mu, float *d_logvar, void *stream);

/* ---- Training batches from resident uint8 images (the reference's src/data/factory.py transforms) ----
 * u8 [N][H][W][C] (device), rows i64 [B] in [0, N) (device; the caller checks them on the host -- an index outside the range
 * reads as a black image), offset i32 [B][2] = (oy, ox) or NULL, flip u8 [B] (non-zero = mirror) or NULL, mean, std f32 [C]
 * (device), out f32 [B][C][H][W].
 *   out[b][c][y][x] = ((p * fl32(1 / 255)) - mean[c]) / std[c],  p = u8[rows[b]][y + oy - pad][sx0 + ox - pad][c],
 *   sx0 = flip[b] ? W - 1 - x : x;  p = 0 where the source position lies outside the image.  offset == NULL means
 *   (oy, ox) = (pad, pad): with flip == NULL too, the plain batch.  RandomCrop(H, padding = pad) draws (oy, ox) in [0, 2 pad]^2.
 * Three float32 roundings, no contraction: bit for bit torch's x.to(float32).div(255).sub_(mean).div_(std) on the device
 * (a division by a host scalar is torch's product with the scalar's float32 reciprocal).
 * Limits: 1 <= C <= 4, 1 <= H, W <= 256, 0 <= pad <= 16, N, B >= 1, B C H ceil(W / 4) < 2^31; GEO_E_ARG outside, before any
 * launch.  One kernel, 16-byte stores when W % 4 == 0 and out is 16-byte aligned, scalar stores otherwise.  Asynchronous. */
int geo_batch_assemble(const uint8_t *u8, int64_t N, int32_t H, int32_t W, int32_t C, const int64_t *rows, int32_t B,
                       const int32_t *offset, const uint8_t *flip, int32_t pad, const float *mean, const float *std, float *out,
                       void *stream);

/* ---- Scores of a generated sample set: kNN radii and ball membership (DESIGN.md section "Precision, recall, density,
 * coverage") ----
 * THE KEY of a pair of float32 rows x, y of width d is geo_knn_query's form 0 chain:
 *   acc = 0;  for c = 0 .. d-1 in this order:  t = (double)x[c] - (double)y[c];  acc = fma(t, t, acc).
 * It is symmetric in x and y, and no tile, slice, corpus range, workspace size or stream enters it: one sequential chain per
 * pair, kept in a register across the dimension chunks.
 *
 * geo_kth_radius: a f32 [n][d] -> r2_out f64 [n]: r2_out[i] = the k-th smallest key between row i and the OTHER rows (self is
 * left out by index: a duplicate of row i is a neighbour at key 0).  An order statistic of a multiset: no tie rule.
 * geo_ball_count: corpus z f32 [n][d] with radii r2 f64 [n], queries q f32 [m][d] -> any of (each may be NULL)
 *   count_out i32 [m]:  #{ i : key(q_j, z_i) <= r2[i] }  (equality counts),
 *   near_key_out f64 [m]:  min_i key(q_j, z_i),   near_idx_out i32 [m]:  the lowest i attaining it.
 * Limits: 1 <= d <= 1024, 1 <= n < 2^31, 0 <= m < 2^31, 1 <= k <= GEO_PRDC_MAX_K and k <= n - 1; GEO_E_ARG outside and for a
 * null z / a / q / r2 / r2_out / ws, GEO_E_WORKSPACE below geo_prdc_min_workspace_bytes(d); both before any launch, nothing is
 * written.  m == 0 (arguments in range) returns GEO_OK without a launch, whatever ws_bytes is.  Asynchronous, no atomics:
 * the corpus is cut into S contiguous ranges per
 * tile of 64 query rows, every range writes its partial (count, nearest pair, k smallest keys) to the workspace and a second
 * kernel folds the ranges in ascending order.
 * Workspace: geo_prdc_workspace_bytes(n, m, d) = all m query rows against n corpus rows in one slice (geo_kth_radius: m = n);
 * geo_prdc_min_workspace_bytes(d) = one tile of 64 query rows, one range.  Anything in between means more slices of query rows
 * or fewer ranges, never another result.  Both queries answer 0 outside the limits. */
#define GEO_PRDC_MAX_K 64
size_t geo_prdc_workspace_bytes(int64_t n, int64_t m, int32_t d);
size_t geo_prdc_min_workspace_bytes(int32_t d);
int geo_kth_radius(const float *a, int64_t n, int32_t d, int32_t k, double *r2_out, void *ws, size_t ws_bytes, void *stream);
int geo_ball_count(const float *z, const double *r2, int64_t n, const float *q, int64_t m, int32_t d, int32_t *count_out,
                   double *near_key_out, int32_t *near_idx_out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GEO_HIP_H */
