// analysis.hip -- the reductions of the geodesic k-medoids analysis (the reference's demos/kmedoids_geodesic_analysis.py) on gfx950.
//
// geo_cluster_label_scores: contingency table of (code, class label) and the sums purity / NMI / ARI are made of.
//   Counting is integer only: a workgroup counts its rows in an int32 LDS table (K C <= 16 384 cells; larger tables are
//   counted in the int64 global table directly) and adds its non-zero cells to the global table with 64-bit integer
//   atomics.  Integer addition is associative, so the table does not depend on the grid, the stream or the run.  The fp64
//   sums are then formed by ONE workgroup in an association fixed by (K, C) alone: wave w owns the rows w, w + 16, ...,
//   a row's cells go lane-strided through an xor butterfly, the 16 wave totals are added in wave order.
//
// geo_feature_colstats / geo_feature_gram / geo_feature_project: PCA of the "distance to every medoid" features
//   X = D^T (n x K) of a K x n row-major float32 matrix D.  A non-finite entry of medoid row k is replaced by
//   fill[k] = fl32(fl32(1.1) * m_k), m_k the row's largest finite value (1 when that is 0 or the row has none): float32
//   arithmetic, as numpy does it on the reference's float32 X.  Everything after the replacement is fp64.
//   colstats: rows are cut into slices of 16 384 columns; per slice the float32 maximum, then the fp64 sum (lane-strided,
//             fixed tree), slice partials added in slice order.
//   gram:     G = Dc Dc^T (K x K, centred on the means) with v_mfma_f64_16x16x4_f64.  A workgroup owns one 64 x 64 tile of the
//             upper block triangle and one slice of the n columns; it stages 64 x 32 pieces of both row blocks in LDS
//             (replacement and centring applied on the way in), each of its 4 waves accumulates a 32 x 32 quarter (2 x 2 MFMA
//             tiles).  The slice partials are added in slice order and mirrored to the lower triangle.  No atomics.
//   project:  Z = Xc V, one thread per column of D, k ascending, fp64 accumulation, float32 out.
#include "geo_common.h"

#include <cmath>

namespace {

constexpr int WAVE = 64;
constexpr int MAX_K = 4096;           // the ABI's limit on codebook sizes
constexpr int MAX_C = 1024;
constexpr int LDS_CELLS = 16384;      // int32 cells of the per-workgroup contingency table (64 KB)
constexpr int COUNT_THREADS = 256;
constexpr int COUNT_ROWS_PER_BLOCK = COUNT_THREADS * 16;
constexpr int STAT_THREADS = 1024;
constexpr int STAT_WAVES = STAT_THREADS / WAVE;

constexpr int SLICE = 16384;          // columns of D per colstats slice
constexpr int RED_THREADS = 256;
constexpr int GT = 64;                // Gram tile: 64 x 64 outputs per workgroup
constexpr int GC = 32;                // columns of D staged per step
constexpr int GLD = GC + 2;           // LDS row stride in doubles
constexpr int GRAM_MIN_SLICE = 4096;  // columns per Gram slice, at least
constexpr int GRAM_TARGET_BLOCKS = 8192;
constexpr int MAX_COMPONENTS = 8;

using f64x4 = __attribute__((ext_vector_type(4))) double;

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}
__device__ __forceinline__ long long wave_max(long long v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const long long o = __shfl_xor(v, off, WAVE);
        v = o > v ? o : v;
    }
    return v;
}

// ---- contingency table -----------------------------------------------------------------------------------------------------
template <bool LDS>
__global__ __launch_bounds__(COUNT_THREADS) void contingency_kernel(const int32_t *__restrict__ assign,
                                                                    const int32_t *__restrict__ labels, int64_t n, int K, int C,
                                                                    unsigned long long *__restrict__ table,
                                                                    unsigned long long *__restrict__ bad) {
    __shared__ int32_t cnt[LDS ? LDS_CELLS : 1];
    const int cells = K * C;
    if (LDS) {
        for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) cnt[i] = 0;
        __syncthreads();
    }
    unsigned long long nbad = 0;
    const int64_t stride = (int64_t)gridDim.x * COUNT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * COUNT_THREADS + threadIdx.x; i < n; i += stride) {
        const int32_t a = assign[i], l = labels[i];
        if (a < 0) continue;                                      // not assigned
        if (a >= K || l < 0 || l >= C) {
            ++nbad;
            continue;
        }
        if (LDS) atomicAdd(&cnt[a * C + l], 1);
        else atomicAdd(&table[(size_t)a * C + l], 1ull);
    }
    if (nbad) atomicAdd(bad, nbad);
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += COUNT_THREADS) {
            const int32_t v = cnt[i];
            if (v) atomicAdd(&table[i], (unsigned long long)v);
        }
    }
}

__device__ __forceinline__ double xlogx(long long v) { return v > 1 ? (double)v * log((double)v) : 0.0; }
__device__ __forceinline__ long long pairs(long long v) { return v * (v - 1) / 2; }

// One workgroup.  isums: n_used, purity numerator, sum C(n_kc,2), sum C(a_k,2), sum C(b_c,2), rows out of range.
// fsums: sum n_kc log n_kc, sum a_k log a_k, sum b_c log b_c.
__global__ __launch_bounds__(STAT_THREADS) void label_stats_kernel(const long long *__restrict__ table, int K, int C,
                                                                   long long *__restrict__ row_counts,
                                                                   long long *__restrict__ col_counts,
                                                                   long long *__restrict__ isums, double *__restrict__ fsums) {
    __shared__ double fred[3][STAT_WAVES];
    __shared__ long long ired[5][STAT_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    double f_kc = 0.0, f_k = 0.0;
    long long p_kc = 0, p_k = 0, pur = 0, tot = 0;
    for (int k = wave; k < K; k += STAT_WAVES) {
        double s = 0.0;
        long long a = 0, p = 0, mx = 0;
        for (int c = lane; c < C; c += WAVE) {
            const long long v = table[(size_t)k * C + c];
            a += v;
            p += pairs(v);
            mx = v > mx ? v : mx;
            s += xlogx(v);
        }
        s = wave_sum(s), a = wave_sum(a), p = wave_sum(p), mx = wave_max(mx);
        f_kc += s, p_kc += p, pur += mx, tot += a;
        p_k += pairs(a);
        f_k += xlogx(a);
        if (lane == 0) row_counts[k] = a;
    }
    // columns: thread c owns column c (C <= 1024 = the workgroup), rows ascending
    double f_c = 0.0;
    long long p_c = 0;
    if ((int)threadIdx.x < C) {
        long long b = 0;
        for (int k = 0; k < K; ++k) b += table[(size_t)k * C + threadIdx.x];
        col_counts[threadIdx.x] = b;
        f_c = xlogx(b);
        p_c = pairs(b);
    }
    f_c = wave_sum(f_c), p_c = wave_sum(p_c);
    if (lane == 0) {
        fred[0][wave] = f_kc, fred[1][wave] = f_k, fred[2][wave] = f_c;
        ired[0][wave] = tot, ired[1][wave] = pur, ired[2][wave] = p_kc, ired[3][wave] = p_k, ired[4][wave] = p_c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 0; j < 3; ++j) {
            double s = fred[j][0];
            for (int w = 1; w < STAT_WAVES; ++w) s += fred[j][w];
            fsums[j] = s;
        }
        for (int j = 0; j < 5; ++j) {
            long long s = 0;
            for (int w = 0; w < STAT_WAVES; ++w) s += ired[j][w];
            isums[j] = s;
        }
    }
}

// ---- feature statistics ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite32(float x) { return fabsf(x) < INFINITY; }       // false for NaN too

// grid (S, K): float32 maximum of the finite entries of slice s of row k (-inf when it has none)
__global__ __launch_bounds__(RED_THREADS) void slice_max_kernel(const float *__restrict__ D, int64_t ld, int64_t n, int S,
                                                                float *__restrict__ pmax) {
    __shared__ float red[RED_THREADS / WAVE];
    const int s = blockIdx.x, k = blockIdx.y;
    const int64_t c0 = (int64_t)s * SLICE, c1 = c0 + SLICE < n ? c0 + SLICE : n;
    const float *row = D + (int64_t)k * ld;
    float m = -INFINITY;
    for (int64_t c = c0 + threadIdx.x; c < c1; c += RED_THREADS) {
        const float x = row[c];
        if (finite32(x)) m = fmaxf(m, x);
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, WAVE));
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RED_THREADS / WAVE; ++w) m = fmaxf(m, red[w]);
        pmax[(size_t)k * S + s] = m;
    }
}

// grid K: row maximum over the slices and the replacement value
__global__ __launch_bounds__(RED_THREADS) void row_fill_kernel(const float *__restrict__ pmax, int S, float *__restrict__ colmax,
                                                               float *__restrict__ fill) {
    __shared__ float red[RED_THREADS / WAVE];
    const int k = blockIdx.x;
    float m = -INFINITY;
    for (int s = threadIdx.x; s < S; s += RED_THREADS) m = fmaxf(m, pmax[(size_t)k * S + s]);
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, WAVE));
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RED_THREADS / WAVE; ++w) m = fmaxf(m, red[w]);
        const float base = (m == -INFINITY || m == 0.0f) ? 1.0f : m;
        colmax[k] = m == -INFINITY ? 0.0f : m;
        fill[k] = base * 1.1f;                                    // one float32 product: numpy's col_max * 1.1 on float32
    }
}

// sum of v over the workgroup, one fixed association; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < RED_THREADS / WAVE; ++w) s += red[w];
    return s;
}

// grid (S, K): fp64 sum of slice s of row k with the replacement applied
__global__ __launch_bounds__(RED_THREADS) void slice_sum_kernel(const float *__restrict__ D, int64_t ld, int64_t n, int S,
                                                                const float *__restrict__ fill, double *__restrict__ psum) {
    __shared__ double red[RED_THREADS / WAVE];
    const int s = blockIdx.x, k = blockIdx.y;
    const int64_t c0 = (int64_t)s * SLICE, c1 = c0 + SLICE < n ? c0 + SLICE : n;
    const float *row = D + (int64_t)k * ld;
    const float f = fill[k];
    double acc = 0.0;
    for (int64_t c = c0 + threadIdx.x; c < c1; c += RED_THREADS) {
        const float x = row[c];
        acc += (double)(finite32(x) ? x : f);
    }
    const double tot = block_sum(acc, red);
    if (threadIdx.x == 0) psum[(size_t)k * S + s] = tot;
}

// grid K: slice sums added in slice order (lane-strided, then the fixed tree), divided by n
__global__ __launch_bounds__(RED_THREADS) void row_mean_kernel(const double *__restrict__ psum, int S, int64_t n,
                                                               double *__restrict__ mean) {
    __shared__ double red[RED_THREADS / WAVE];
    const int k = blockIdx.x;
    double acc = 0.0;
    for (int s = threadIdx.x; s < S; s += RED_THREADS) acc += psum[(size_t)k * S + s];
    const double tot = block_sum(acc, red);
    if (threadIdx.x == 0) mean[k] = tot / (double)n;
}

// ---- centred Gram matrix ---------------------------------------------------------------------------------------------------
// grid (T, S): tile pair p = (bi, bj), bi <= bj, of the upper block triangle; slice s = columns [s len, (s + 1) len) of D.
__global__ __launch_bounds__(256) void gram_kernel(const float *__restrict__ D, int64_t ld, int K, int64_t n,
                                                   const float *__restrict__ fill, const double *__restrict__ mean, int nbt,
                                                   int64_t slice_len, double *__restrict__ partial) {
    __shared__ double As[GT][GLD], Bs[GT][GLD];
    int bi = 0, p = blockIdx.x;
    while (p >= nbt - bi) p -= nbt - bi, ++bi;
    const int bj = bi + p;
    const bool diag = bi == bj;
    const int s = blockIdx.y;
    const int64_t n0 = (int64_t)s * slice_len, n1 = n0 + slice_len < n ? n0 + slice_len : n;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int wi = wave >> 1, wj = wave & 1;
    const int scol = threadIdx.x % GC, srow = threadIdx.x / GC;            // staging: 8 row groups x 32 columns
    f64x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int64_t c0 = n0; c0 < n1; c0 += GC) {
        const int64_t col = c0 + scol;
#pragma unroll
        for (int i = 0; i < GT / 8; ++i) {
            const int r = srow + 8 * i;
            const int ka = bi * GT + r, kb = bj * GT + r;
            double va = 0.0, vb = 0.0;                                     // rows past K and columns past the slice add zeros
            if (col < n1) {
                if (ka < K) {
                    const float x = D[(int64_t)ka * ld + col];
                    va = (double)(finite32(x) ? x : fill[ka]) - mean[ka];
                }
                if (!diag && kb < K) {
                    const float x = D[(int64_t)kb * ld + col];
                    vb = (double)(finite32(x) ? x : fill[kb]) - mean[kb];
                }
            }
            As[r][scol] = va;
            if (!diag) Bs[r][scol] = vb;
        }
        __syncthreads();
        const double(*Bt)[GLD] = diag ? As : Bs;
#pragma unroll
        for (int kk = 0; kk < GC / 4; ++kk) {
            const int k = kk * 4 + (lane >> 4);                            // A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15]
            const double a0 = As[wi * 32 + (lane & 15)][k], a1 = As[wi * 32 + 16 + (lane & 15)][k];
            const double b0 = Bt[wj * 32 + (lane & 15)][k], b1 = Bt[wj * 32 + 16 + (lane & 15)][k];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg
    double *out = partial + (size_t)s * K * K;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = bi * GT + wi * 32 + x * 16 + (lane >> 4) + 4 * reg;
                const int gj = bj * GT + wj * 32 + y * 16 + (lane & 15);
                if (gi < K && gj < K) out[(size_t)gi * K + gj] = acc[x][y][reg];
            }
}

// G[i][j] = G[j][i] = sum over the slices, in slice order, of the partial of (i, j), i <= j
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double *__restrict__ partial, int K, int S,
                                                          double *__restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)K * K) return;
    const int i = (int)(e / K), j = (int)(e % K);
    if (i > j) return;
    double sum = partial[e];
    for (int s = 1; s < S; ++s) sum += partial[(size_t)s * K * K + e];
    G[(size_t)i * K + j] = sum;
    G[(size_t)j * K + i] = sum;
}

// ---- projection ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void project_kernel(const float *__restrict__ D, int64_t ld, int K, int64_t n,
                                                      const float *__restrict__ fill, const double *__restrict__ mean,
                                                      const double *__restrict__ V, int nc, float *__restrict__ Z) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double acc[MAX_COMPONENTS];
#pragma unroll
    for (int j = 0; j < MAX_COMPONENTS; ++j) acc[j] = 0.0;
    for (int k = 0; k < K; ++k) {
        const float x = D[(int64_t)k * ld + c];
        const double v = (double)(finite32(x) ? x : fill[k]) - mean[k];
#pragma unroll
        for (int j = 0; j < MAX_COMPONENTS; ++j)
            if (j < nc) acc[j] = fma(v, V[(size_t)k * nc + j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < MAX_COMPONENTS; ++j)
        if (j < nc) Z[c * nc + j] = (float)acc[j];
}

struct GramPlan {
    int nbt, tiles, slices;
    int64_t slice_len;
};
GramPlan gram_plan(int64_t n, int K) {
    GramPlan g;
    g.nbt = (K + GT - 1) / GT;
    g.tiles = g.nbt * (g.nbt + 1) / 2;
    int64_t want = (n + GRAM_MIN_SLICE - 1) / GRAM_MIN_SLICE;
    const int64_t cap = GRAM_TARGET_BLOCKS / g.tiles > 1 ? GRAM_TARGET_BLOCKS / g.tiles : 1;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    g.slice_len = ((n + want - 1) / want + GC - 1) / GC * GC;
    g.slices = (int)((n + g.slice_len - 1) / g.slice_len);
    return g;
}
int64_t stat_slices(int64_t n) { return (n + SLICE - 1) / SLICE; }

// The layouts of geo_feature_colstats and geo_feature_gram; geo_feature_workspace_bytes answers the larger plus its reserve.
struct StatsWs { float *pmax; double *psum; };
StatsWs carve_stats(geo::Arena &ar, int64_t n, int32_t K) {
    const size_t count = (size_t)stat_slices(n) * K;
    return {ar.take<float>(count), ar.take<double>(count)};
}
double *carve_gram(geo::Arena &ar, const GramPlan &g, int32_t K) { return ar.take<double>((size_t)g.slices * K * K); }
constexpr size_t FEATURE_RESERVE = 256;

bool feature_shape_ok(const float *D, int64_t ld, int32_t K, int64_t n) {
    return D && K >= 1 && K <= MAX_K && n >= 1 && n <= INT32_MAX && ld >= n;
}

}  // namespace

extern "C" int geo_cluster_label_scores(const int32_t *assign, const int32_t *labels, int64_t n, int32_t K, int32_t C,
                                        int32_t grid_blocks, int64_t *table_out, int64_t *row_counts_out,
                                        int64_t *col_counts_out, int64_t *isums_out, double *fsums_out, void *stream_) {
    GEO_REQUIRE(assign && labels && table_out && row_counts_out && col_counts_out && isums_out && fsums_out,
                "geo_cluster_label_scores: null pointer");
    GEO_REQUIRE(K >= 1 && K <= MAX_K && C >= 1 && C <= MAX_C, "geo_cluster_label_scores: K=%d, C=%d outside [1, %d] x [1, %d]", K,
                C, MAX_K, MAX_C);
    GEO_REQUIRE(n >= 0 && n <= INT32_MAX, "geo_cluster_label_scores: n %lld outside [0, 2^31) (int64 pair counts, int32 cells)",
                (long long)n);
    GEO_REQUIRE(grid_blocks >= 0 && grid_blocks <= 65536, "geo_cluster_label_scores: grid_blocks %d outside [0, 65536]",
                grid_blocks);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GEO_HIP_CHECK(hipMemsetAsync(table_out, 0, (size_t)K * C * sizeof(int64_t), stream));
    GEO_HIP_CHECK(hipMemsetAsync(isums_out, 0, 6 * sizeof(int64_t), stream));
    if (n > 0) {
        const int grid = grid_blocks ? grid_blocks : geo::grid_for(n, COUNT_ROWS_PER_BLOCK, 1024);
        auto *table = reinterpret_cast<unsigned long long *>(table_out);
        auto *bad = reinterpret_cast<unsigned long long *>(isums_out + 5);
        if (K * C <= LDS_CELLS)
            hipLaunchKernelGGL(contingency_kernel<true>, dim3(grid), dim3(COUNT_THREADS), 0, stream, assign, labels, n, K, C,
                               table, bad);
        else
            hipLaunchKernelGGL(contingency_kernel<false>, dim3(grid), dim3(COUNT_THREADS), 0, stream, assign, labels, n, K, C,
                               table, bad);
        GEO_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(label_stats_kernel, dim3(1), dim3(STAT_THREADS), 0, stream,
                       reinterpret_cast<const long long *>(table_out), K, C, reinterpret_cast<long long *>(row_counts_out),
                       reinterpret_cast<long long *>(col_counts_out), reinterpret_cast<long long *>(isums_out), fsums_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" size_t geo_feature_workspace_bytes(int64_t n, int32_t K) {
    if (K < 1 || K > MAX_K || n < 1 || n > INT32_MAX) return 0;
    const size_t stats = geo::measure(carve_stats, n, K), gram = geo::measure(carve_gram, gram_plan(n, K), K);
    return (stats > gram ? stats : gram) + FEATURE_RESERVE;
}

extern "C" int geo_feature_colstats(const float *D, int64_t ld, int32_t K, int64_t n, float *colmax_out, float *fill_out,
                                    double *mean_out, void *ws, size_t ws_bytes, void *stream_) {
    GEO_REQUIRE(feature_shape_ok(D, ld, K, n), "geo_feature_colstats: bad shape (K=%d in [1, %d], n=%lld in [1, 2^31), ld >= n)",
                K, MAX_K, (long long)n);
    GEO_REQUIRE(colmax_out && fill_out && mean_out && ws, "geo_feature_colstats: null pointer");
    const int S = (int)stat_slices(n);
    geo::Arena ar(ws, ws_bytes);
    const auto [pmax, psum] = carve_stats(ar, n, K);
    if (!ar.ok()) {
        geo::set_error("geo_feature_colstats: workspace %zu too small (%zu needed)", ws_bytes, ar.off);
        return GEO_E_WORKSPACE;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(slice_max_kernel, dim3(S, K), dim3(RED_THREADS), 0, stream, D, ld, n, S, pmax);
    GEO_LAUNCH_CHECK();
    hipLaunchKernelGGL(row_fill_kernel, dim3(K), dim3(RED_THREADS), 0, stream, pmax, S, colmax_out, fill_out);
    GEO_LAUNCH_CHECK();
    hipLaunchKernelGGL(slice_sum_kernel, dim3(S, K), dim3(RED_THREADS), 0, stream, D, ld, n, S, fill_out, psum);
    GEO_LAUNCH_CHECK();
    hipLaunchKernelGGL(row_mean_kernel, dim3(K), dim3(RED_THREADS), 0, stream, psum, S, n, mean_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" int geo_feature_gram(const float *D, int64_t ld, int32_t K, int64_t n, const float *fill, const double *mean,
                                double *gram_out, void *ws, size_t ws_bytes, void *stream_) {
    GEO_REQUIRE(feature_shape_ok(D, ld, K, n), "geo_feature_gram: bad shape (K=%d in [1, %d], n=%lld in [1, 2^31), ld >= n)", K,
                MAX_K, (long long)n);
    GEO_REQUIRE(fill && mean && gram_out && ws, "geo_feature_gram: null pointer");
    const GramPlan g = gram_plan(n, K);
    geo::Arena ar(ws, ws_bytes);
    double *partial = carve_gram(ar, g, K);
    if (!ar.ok()) {
        geo::set_error("geo_feature_gram: workspace %zu too small (%zu needed)", ws_bytes, ar.off);
        return GEO_E_WORKSPACE;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(gram_kernel, dim3(g.tiles, g.slices), dim3(256), 0, stream, D, ld, K, n, fill, mean, g.nbt, g.slice_len,
                       partial);
    GEO_LAUNCH_CHECK();
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)(((int64_t)K * K + 255) / 256)), dim3(256), 0, stream, partial, K,
                       g.slices, gram_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" int geo_feature_project(const float *D, int64_t ld, int32_t K, int64_t n, const float *fill, const double *mean,
                                   const double *V, int32_t n_components, float *Z_out, void *stream_) {
    GEO_REQUIRE(feature_shape_ok(D, ld, K, n), "geo_feature_project: bad shape (K=%d in [1, %d], n=%lld in [1, 2^31), ld >= n)",
                K, MAX_K, (long long)n);
    GEO_REQUIRE(fill && mean && V && Z_out, "geo_feature_project: null pointer");
    GEO_REQUIRE(n_components >= 1 && n_components <= MAX_COMPONENTS && n_components <= K,
                "geo_feature_project: n_components %d outside [1, min(K, %d)]", n_components, MAX_COMPONENTS);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, D, ld, K, n, fill, mean, V,
                       n_components, Z_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}
