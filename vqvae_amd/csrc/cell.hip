// cell.hip -- cell-restricted medoid costs: many small shortest-path solves, batched (gfx950).
//
// A medoid update needs the distances between members of ONE cluster only.  For a geodesic Voronoi cell the shortest path
// from the medoid to a member stays inside the cell (float32 ties apart, DESIGN.md "Cell-restricted medoid update"), so
// the update is solved on the CUT graph: the entries of the symmetric pull CSR whose two ends share a cell.  That is
// sum_c m_c^2 distance entries instead of n^2 and no N x N or K x N matrix, so the update runs at any graph size.
//
//   cost[i] = sum over the members j of i's cell, ascending node order, of (double)d_c(i, j)^power
//
// with d_c the shortest path inside the cell under geo_sssp_multi's rule (fp64 sums source-outward, one rounding per hop,
// run to the fixed point, rounded to float32 at the end, +inf where unreachable) and the summation tree of
// geo_cluster_costs (64 strided partial sums, xor butterfly 32..1): the result equals geo_cluster_costs over the all-pairs
// matrix of the cut graph bit for bit.
//
// Passes of one call, all on the caller's stream:
//   cell_plan_kernel   cells ranked by size (largest first, lower cell first among equals) and the first unit of every
//                      rank; a UNIT is (cell, tile of CELL_S sources of that cell).  No host loop over cells.
//   cell_pos_kernel    pos[v] = position of node v in `order` (-1: in no cell).
//   cell_cut_kernel    the cut graph in place: the kept entries of node v, renumbered to positions inside its cell, packed
//                      to the front of v's own row range [indptr[v], ...) of an nnz-long scratch copy (no scan needed).
//   cell_solve_kernel  persistent workgroups take units from two counters.  A unit relaxes its CELL_S distance rows in
//                      place (chaotic relaxation from +inf only ever stores sums of real paths and stops when a whole sweep
//                      stored nothing: the fixed point, Dijkstra's fp64 values), then reduces each row with the fixed tree.
//                      RESIDENT route (cells of at most resident_nodes_max nodes): the rows live in LDS, one workgroup owns
//                      the CU's 160 KiB.  WORKSPACE route (larger cells): the rows live in the workgroup's slice of `ws`;
//                      only workgroups that have a slice take such units, so a smaller `ws` means fewer of them in flight.
//   cell_commit_kernel copies the staged costs to cost_out (+inf outside every cell) unless a unit failed: a failed call
//                      writes nothing.
// Rows are laid out node-major, [node][CELL_S] doubles: the 16 lanes that share a node read 128 contiguous bytes of a
// neighbour's entry (ds_read_b64: a 32-lane group touches two such runs, at worst a 2-way conflict), the edge itself is one
// broadcast 8-byte load.  No float atomics: every cost has one writer, the integer atomics are the two unit counters and the
// sweep maximum.
#include "geo_common.h"

namespace {

constexpr int CELL_S = 16;                  // sources per unit
constexpr int CELL_THREADS = 1024;          // 64 node groups x CELL_S lanes
constexpr int CELL_GROUPS = CELL_THREADS / CELL_S;
constexpr int CELL_U = 8;                   // entries of a node's row in flight per lane
constexpr int CELL_LDS_NODES = 1264;        // 1264 x 16 x 8 B = 161 792 B of the 163 840 B a workgroup may declare
constexpr int CELL_MIN_SLICE_NODES = 64;    // the reduction parks 64 x CELL_S partial sums in the rows' storage
constexpr int CELL_GRID = 256;              // persistent workgroups the workspace query sizes slices for (one per CU)
constexpr int CELL_SWEEP_CAP = 1 << 16;     // sweeps of one unit before GEO_E_NOCONV (a cell of m nodes needs at most m)

static_assert(CELL_GROUPS == 64, "the cost reduction maps one thread per (butterfly lane, source)");

enum { H_NEXT_WS = 0, H_NEXT_RES, H_UNITS_WS, H_UNITS, H_FAIL, H_SWEEPS, H_RES_CELLS, H_WS_CELLS, H_MAX_CELL, H_MEMBERS, H_WORDS = 64 };
enum { FAIL_ARG = 1, FAIL_NOCONV = 2 };

__device__ __forceinline__ int32_t tiles_of(int32_t m) { return (m + CELL_S - 1) / CELL_S; }

// One thread per cell c: rank = cells that come before c (larger, or equal and lower index), start = their units.
__global__ __launch_bounds__(256) void cell_plan_kernel(const int32_t *__restrict__ offsets, int32_t K, int32_t n, int32_t resident,
                                                       int32_t *__restrict__ cell_sorted, int32_t *__restrict__ unit_start,
                                                       int32_t *__restrict__ hdr) {
    __shared__ int32_t s_m[256];
    const int32_t c = blockIdx.x * 256 + threadIdx.x;
    const int32_t total = offsets[K];
    const bool bad_total = offsets[0] != 0 || total < 0 || total > n;
    const int32_t mc = c < K ? offsets[c + 1] - offsets[c] : 0;
    int32_t rank = 0, start = 0, units_ws = 0, res_cells = 0, ws_cells = 0, max_cell = 0;
    bool bad = bad_total || mc < 0;
    for (int32_t b = 0; b < K; b += 256) {
        __syncthreads();
        s_m[threadIdx.x] = b + threadIdx.x < K ? offsets[b + threadIdx.x + 1] - offsets[b + threadIdx.x] : 0;
        __syncthreads();
        const int32_t lim = K - b < 256 ? K - b : 256;
        for (int32_t i = 0; i < lim; ++i) {
            const int32_t m = s_m[i] < 0 ? 0 : s_m[i], o = b + i;
            const bool before = m > mc || (m == mc && o < c);
            rank += before ? 1 : 0;
            start += before ? tiles_of(m) : 0;
            units_ws += m > resident ? tiles_of(m) : 0;
            res_cells += (m > 0 && m <= resident) ? 1 : 0;
            ws_cells += m > resident ? 1 : 0;
            max_cell = m > max_cell ? m : max_cell;
        }
    }
    if (bad) atomicOr(&hdr[H_FAIL], FAIL_ARG);
    if (c >= K || bad) return;
    cell_sorted[rank] = c;
    unit_start[rank] = start;
    if (rank == K - 1) {
        unit_start[K] = start + tiles_of(mc);
        hdr[H_UNITS] = start + tiles_of(mc);
    }
    if (c == 0) {
        hdr[H_UNITS_WS] = units_ws;
        hdr[H_RES_CELLS] = res_cells;
        hdr[H_WS_CELLS] = ws_cells;
        hdr[H_MAX_CELL] = max_cell;
        hdr[H_MEMBERS] = total;
    }
}

__global__ __launch_bounds__(256) void cell_pos_kernel(const int32_t *__restrict__ order, const int32_t *__restrict__ offsets, int32_t K,
                                                      int32_t n, int32_t *__restrict__ pos, int32_t *__restrict__ hdr) {
    const int32_t total = offsets[K];
    if (total < 0 || total > n) return;                         // cell_plan_kernel reports it
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
        const int32_t v = order[p];
        if (v < 0 || v >= n) atomicOr(&hdr[H_FAIL], FAIL_ARG);
        else pos[v] = (int32_t)p;
    }
}

// One thread per member position p: the entries of node order[p] whose other end lies in the same cell, as
// (position inside the cell, weight bits), packed from indptr[order[p]] on.  Everything the solve indexes with is checked
// here, so an inconsistent (assign, order, offsets) fails the call instead of reaching past a cell.
__global__ __launch_bounds__(256) void cell_cut_kernel(const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                      const float *__restrict__ weights, int32_t n, int64_t nnz,
                                                      const int32_t *__restrict__ assign, const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ offsets, int32_t K, const int32_t *__restrict__ pos,
                                                      int32_t *__restrict__ rowstart, int32_t *__restrict__ cnt, int2 *__restrict__ cut,
                                                      int32_t *__restrict__ hdr) {
    const int32_t total = offsets[K];
    if (total < 0 || total > n) return;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < total; p += (int64_t)gridDim.x * 256) {
        rowstart[p] = 0;
        cnt[p] = 0;
        const int32_t v = order[p];
        if (v < 0 || v >= n) continue;                          // reported by cell_pos_kernel
        const int32_t c = assign[v];
        if (c < 0 || c >= K || pos[v] != (int32_t)p) { atomicOr(&hdr[H_FAIL], FAIL_ARG); continue; }
        const int32_t o0 = offsets[c], m = offsets[c + 1] - o0;
        const int32_t e0 = indptr[v], e1 = indptr[v + 1];
        if (p < o0 || p - o0 >= m || e0 < 0 || e1 < e0 || (int64_t)e1 > nnz) { atomicOr(&hdr[H_FAIL], FAIL_ARG); continue; }
        int32_t k = 0;
        for (int32_t e = e0; e < e1; ++e) {
            const int32_t u = indices[e];
            if (u < 0 || u >= n || u == v || assign[u] != c) continue;
            const int32_t loc = pos[u] - o0;
            if (pos[u] < 0 || loc < 0 || loc >= m) continue;
            cut[e0 + k++] = make_int2(loc, __float_as_int(weights[e]));
        }
        rowstart[p] = e0;
        cnt[p] = k;
    }
}

// One unit on rows d[node][CELL_S] (LDS or the workgroup's slice): relax to the fixed point, reduce, stage the costs.
// Returns the sweeps it took, or -1 beyond CELL_SWEEP_CAP.  All threads of the workgroup call it together.
__device__ __forceinline__ int32_t cell_unit(double *d, int32_t *s_flag, const int32_t *__restrict__ rowstart, const int32_t *__restrict__ cnt,
                                            const int2 *__restrict__ cut, int32_t off, int32_t m, int32_t s0, int32_t ns, int32_t power,
                                            double *__restrict__ stage) {
    const int tid = threadIdx.x, s = tid & (CELL_S - 1), g = tid / CELL_S;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    for (int32_t i = tid; i < m * CELL_S; i += CELL_THREADS) d[i] = inf;
    if (tid < 3) s_flag[tid] = 0;
    __syncthreads();
    if (tid < ns) d[(s0 + tid) * CELL_S + tid] = 0.0;
    __syncthreads();
    int32_t sweep = 0;
    for (;;) {
        bool changed = false;
        if (s < ns)
            for (int32_t j = g; j < m; j += CELL_GROUPS) {
                const int32_t e0 = rowstart[off + j], k = cnt[off + j];
                const double cur = d[j * CELL_S + s];
                double best = cur;
                // CELL_U entries in flight; a chunk past the row's end repeats the last entry (min is exact and idempotent:
                // any order, any repeats, the same value), so there is no serial tail
                for (int32_t e = 0; e < k; e += CELL_U) {
                    int2 ed[CELL_U];
#pragma unroll
                    for (int q = 0; q < CELL_U; ++q) ed[q] = cut[e0 + (e + q < k ? e + q : k - 1)];   // one address per group of CELL_S lanes
                    double x[CELL_U];
#pragma unroll
                    for (int q = 0; q < CELL_U; ++q) x[q] = d[ed[q].x * CELL_S + s] + (double)__int_as_float(ed[q].y);
#pragma unroll
                    for (int q = 0; q < CELL_U; ++q) best = fmin(best, x[q]);
                }
                if (best < cur) {
                    d[j * CELL_S + s] = best;
                    changed = true;
                }
            }
        // three flags in rotation: the one reset here was last read two barriers ago
        if (changed) s_flag[sweep % 3] = 1;
        if (tid == 0) s_flag[(sweep + 1) % 3] = 0;
        __syncthreads();
        const int32_t any = s_flag[sweep % 3];
        ++sweep;
        if (!any) break;
        if (sweep >= CELL_SWEEP_CAP) return -1;
    }
    // cost of source s: thread (g, s) is butterfly lane g; members g, g + 64, ... in that order, as cluster_cost_kernel
    double acc = 0.0;
    for (int32_t j = g; j < m; j += CELL_GROUPS) {
        const double x = (double)(float)d[j * CELL_S + s];
        acc += power == 2 ? x * x : x;
    }
    __syncthreads();
    d[g * CELL_S + s] = acc;                                   // the rows are done with: their first 64 entries hold the partials
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;                // wave w folds source w
    double a = d[lane * CELL_S + wave];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0 && wave < ns) stage[off + s0 + wave] = a;
    __syncthreads();
    return sweep;
}

__global__ __launch_bounds__(CELL_THREADS) void cell_solve_kernel(const int32_t *__restrict__ offsets, int32_t K, const int32_t *__restrict__ cell_sorted,
                                                                  const int32_t *__restrict__ unit_start, const int32_t *__restrict__ rowstart,
                                                                  const int32_t *__restrict__ cnt, const int2 *__restrict__ cut, int32_t power,
                                                                  int32_t resident, double *slices, int64_t slice_doubles, int32_t n_slices,
                                                                  double *__restrict__ stage, int32_t *hdr) {
    __shared__ double s_rows[CELL_LDS_NODES * CELL_S];
    __shared__ int32_t s_flag[3];
    __shared__ int32_t s_unit;
    const int32_t units_ws = hdr[H_UNITS_WS], units = hdr[H_UNITS];
    double *slice = slices + (int64_t)blockIdx.x * slice_doubles;
    int32_t most = 0;
    for (int phase = (int)blockIdx.x < n_slices ? 0 : 1; phase < 2;) {
        if (threadIdx.x == 0) s_unit = atomicAdd(&hdr[phase == 0 ? H_NEXT_WS : H_NEXT_RES], 1);
        __syncthreads();
        const int32_t taken = s_unit;
        __syncthreads();
        const int32_t u = phase == 0 ? taken : units_ws + taken;
        if (taken < 0 || u >= (phase == 0 ? units_ws : units)) { ++phase; continue; }
        int32_t lo = 0, hi = K - 1;                             // the last rank whose first unit is <= u (empty cells come last)
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (unit_start[mid] <= u) lo = mid; else hi = mid - 1;
        }
        const int32_t c = cell_sorted[lo], off = offsets[c], m = offsets[c + 1] - off, s0 = (u - unit_start[lo]) * CELL_S;
        const int32_t ns = m - s0 < CELL_S ? m - s0 : CELL_S;
        int32_t sw;
        if (m <= resident) sw = cell_unit(s_rows, s_flag, rowstart, cnt, cut, off, m, s0, ns, power, stage);
        else if (phase == 0 && m <= slice_doubles / CELL_S) sw = cell_unit(slice, s_flag, rowstart, cnt, cut, off, m, s0, ns, power, stage);
        else sw = -2;                                           // cannot happen with the plan the host launched from
        if (sw < 0) {
            if (threadIdx.x == 0) atomicOr(&hdr[H_FAIL], sw == -1 ? FAIL_NOCONV : FAIL_ARG);
            break;
        }
        most = sw > most ? sw : most;
    }
    if (threadIdx.x == 0 && most > 0) atomicMax(&hdr[H_SWEEPS], most);
}

__global__ __launch_bounds__(256) void cell_commit_kernel(const int32_t *__restrict__ pos, const double *__restrict__ stage, int32_t n,
                                                         const int32_t *__restrict__ hdr, double *__restrict__ cost) {
    if (hdr[H_FAIL] != 0) return;
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int32_t p = pos[v];
    cost[v] = p >= 0 ? stage[p] : __longlong_as_double(0x7ff0000000000000LL);
}

size_t slice_bytes(int32_t max_cell) {
    const int64_t nodes = max_cell > CELL_MIN_SLICE_NODES ? max_cell : CELL_MIN_SLICE_NODES;
    return geo::align_up((size_t)nodes * CELL_S * sizeof(double));
}

// Everything but the slices: measured by the queries, carved by geo_cell_costs.
struct CellWs { int32_t *hdr, *pos, *rowstart, *cnt, *cell_sorted, *unit_start; double *stage; int2 *cut; };
CellWs carve_fixed(geo::Arena &ar, int32_t n, int64_t nnz, int32_t K) {
    const size_t N = n < 1 ? 1 : (size_t)n, E = nnz < 1 ? 1 : (size_t)nnz, C = K < 1 ? 1 : (size_t)K;
    CellWs o;
    ar.take(o.hdr, H_WORDS); ar.take(o.pos, N); ar.take(o.rowstart, N); ar.take(o.cnt, N);
    ar.take(o.cell_sorted, C); ar.take(o.unit_start, C + 1);
    ar.take(o.stage, N);
    ar.take(o.cut, E);
    return o;
}
size_t fixed_bytes(int32_t n, int64_t nnz, int32_t K) { return geo::measure(carve_fixed, n, nnz, K); }

}  // namespace

extern "C" int32_t geo_cell_costs_tile(void) { return CELL_S; }
extern "C" int32_t geo_cell_costs_resident_max_nodes(void) { return CELL_LDS_NODES; }

extern "C" size_t geo_cell_costs_min_workspace_bytes(int32_t n, int64_t nnz, int32_t K, int32_t max_cell) {
    return fixed_bytes(n, nnz, K) + slice_bytes(max_cell);
}

extern "C" size_t geo_cell_costs_workspace_bytes(int32_t n, int64_t nnz, int32_t K, int32_t max_cell) {
    const int64_t tiles = (int64_t)(n < 1 ? 1 : n) / CELL_S + (K < 1 ? 1 : K);
    return fixed_bytes(n, nnz, K) + (size_t)(tiles < CELL_GRID ? tiles : CELL_GRID) * slice_bytes(max_cell);
}

extern "C" int geo_cell_costs(const int32_t *indptr, const int32_t *indices, const float *weights, int32_t n, int64_t nnz,
                              const int32_t *assign, const int32_t *order, const int32_t *offsets, int32_t K, int32_t power,
                              int32_t resident_nodes_max, double *cost_out, void *ws, size_t ws_bytes, int32_t *status_out, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(indptr && indices && weights && assign && order && offsets && cost_out && ws && status_out, "geo_cell_costs: null pointer");
    GEO_REQUIRE(n >= 1 && n < (1 << 27) && nnz >= 0 && nnz < ((int64_t)1 << 31) && K >= 1 && (power == 1 || power == 2) && resident_nodes_max >= 0,
                "geo_cell_costs: bad n=%d nnz=%lld K=%d power=%d resident_nodes_max=%d", n, (long long)nnz, K, power, resident_nodes_max);
    status_out[0] = status_out[1] = status_out[2] = status_out[3] = 0;
    const int32_t resident = resident_nodes_max == 0 || resident_nodes_max > CELL_LDS_NODES ? CELL_LDS_NODES : resident_nodes_max;
    geo::Arena ar(ws, ws_bytes);
    const CellWs w = carve_fixed(ar, n, nnz, K);
    if (ws_bytes < ar.off + slice_bytes(0)) {
        geo::set_error("geo_cell_costs: workspace of %zu bytes is below the minimum of %zu", ws_bytes, ar.off + slice_bytes(0));
        return GEO_E_WORKSPACE;
    }
    int32_t *hdr = w.hdr, *pos = w.pos, *rowstart = w.rowstart, *cnt = w.cnt, *cell_sorted = w.cell_sorted, *unit_start = w.unit_start;
    double *stage = w.stage;
    int2 *cut = w.cut;
    GEO_HIP_CHECK(hipMemsetAsync(hdr, 0, H_WORDS * sizeof(int32_t), stream));
    GEO_HIP_CHECK(hipMemsetAsync(pos, 0xff, (size_t)n * sizeof(int32_t), stream));
    cell_plan_kernel<<<(unsigned)((K + 255) / 256), 256, 0, stream>>>(offsets, K, n, resident, cell_sorted, unit_start, hdr);
    GEO_LAUNCH_CHECK();
    cell_pos_kernel<<<geo::grid_for(n, 256), 256, 0, stream>>>(order, offsets, K, n, pos, hdr);
    GEO_LAUNCH_CHECK();
    cell_cut_kernel<<<geo::grid_for(n, 256), 256, 0, stream>>>(indptr, indices, weights, n, nnz, assign, order, offsets, K, pos, rowstart, cnt,
                                                              cut, hdr);
    GEO_LAUNCH_CHECK();
    int32_t h[H_WORDS];
    GEO_HIP_CHECK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
    GEO_HIP_CHECK(hipStreamSynchronize(stream));
    GEO_REQUIRE(h[H_FAIL] == 0, "geo_cell_costs: order / offsets / assign / indptr are inconsistent (offsets[K] = %d of n = %d)", h[H_MEMBERS], n);
    const size_t slice = slice_bytes(h[H_MAX_CELL]);
    if (ws_bytes < ar.off + slice) {
        geo::set_error("geo_cell_costs: workspace of %zu bytes is below the minimum of %zu (largest cell %d)", ws_bytes, ar.off + slice,
                       h[H_MAX_CELL]);
        return GEO_E_WORKSPACE;
    }
    if (h[H_UNITS] > 0) {
        int dev = 0, cus = CELL_GRID;
        GEO_HIP_CHECK(hipGetDevice(&dev));
        GEO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int32_t grid = h[H_UNITS] < cus ? h[H_UNITS] : cus;
        const size_t fit = (ws_bytes - ar.off) / slice;
        const int32_t n_slices = h[H_UNITS_WS] == 0 ? 0 : (int32_t)(fit < (size_t)grid ? fit : (size_t)grid);
        cell_solve_kernel<<<(unsigned)grid, CELL_THREADS, 0, stream>>>(offsets, K, cell_sorted, unit_start, rowstart, cnt, cut, power, resident,
                                                                      reinterpret_cast<double *>(static_cast<char *>(ws) + ar.off),
                                                                      (int64_t)(slice / sizeof(double)), n_slices, stage, hdr);
        GEO_LAUNCH_CHECK();
    }
    cell_commit_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(pos, stage, n, hdr, cost_out);
    GEO_LAUNCH_CHECK();
    GEO_HIP_CHECK(hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, stream));
    GEO_HIP_CHECK(hipStreamSynchronize(stream));
    if (h[H_FAIL] & FAIL_NOCONV) {
        geo::set_error("geo_cell_costs: a unit did not converge within %d sweeps", CELL_SWEEP_CAP);
        return GEO_E_NOCONV;
    }
    GEO_REQUIRE(h[H_FAIL] == 0, "geo_cell_costs: inconsistent plan");
    status_out[0] = h[H_RES_CELLS];
    status_out[1] = h[H_WS_CELLS];
    status_out[2] = h[H_SWEEPS];
    return GEO_OK;
}
