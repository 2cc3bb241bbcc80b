// graph_effects.hip -- the two device steps of the Riemannian graph experiments (the reference's
// experiments/geo/run_riemann_experiments.py) on gfx950; DESIGN.md section 16.
//
// geo_path_stats: reduces every row of an S x n block of shortest-path distances (geo_sssp_multi's D_out) to the four
//   numbers "mean of the finite, positive entries" is made of, so the block never goes to the host.  One workgroup of
//   1024 threads owns one row.  Thread t reads the columns t, t + 1024, ... (plain 4-byte loads: a wave reads 256
//   consecutive bytes whatever the row's alignment) and adds its qualifying entries to one fp64 accumulator in ascending
//   column order; the 64 lanes of a wave go through an xor butterfly, the 16 wave totals are added in wave order by
//   thread 0.  The association depends on n alone -- not on the number of rows, the grid, the stream or the row's
//   address -- and there is no atomic: every output is bit-identical across runs.
//
// geo_csr_set_symmetric: W[i, j] = W[j, i] = v for a list of unique pairs on a CSR with sorted rows.  One thread per
//   pair: a binary search of row i for column j and of row j for column i, two plain 4-byte stores when both entries
//   exist, otherwise no store and one 32-bit integer atomic on the miss counter.
#include "geo_common.h"

#include <cmath>

namespace {

constexpr int WAVE = 64;
constexpr int STAT_THREADS = 1024;
constexpr int STAT_WAVES = STAT_THREADS / WAVE;
constexpr int SET_THREADS = 256;

__global__ __launch_bounds__(STAT_THREADS) void path_stats_kernel(const float *__restrict__ D, int64_t ld, int64_t n,
                                                                  double *__restrict__ sum_out, long long *__restrict__ n_pos_out,
                                                                  long long *__restrict__ n_unreached_out,
                                                                  float *__restrict__ max_out) {
    __shared__ double sred[STAT_WAVES];
    __shared__ long long pred[STAT_WAVES], ured[STAT_WAVES];
    __shared__ float mred[STAT_WAVES];
    const float *row = D + (int64_t)blockIdx.x * ld;
    double sum = 0.0;
    long long n_pos = 0, n_inf = 0;
    float mx = -INFINITY;
    auto take = [&](float x) {
        const bool fin = fabsf(x) < INFINITY;                             // false for NaN too
        if (fin && x > 0.0f) sum += (double)x, ++n_pos;
        if (fin) mx = fmaxf(mx, x);
        if (x == INFINITY) ++n_inf;
    };
    int64_t c = threadIdx.x;
    for (; c + 3 * (int64_t)STAT_THREADS < n; c += 4 * (int64_t)STAT_THREADS) {         // four loads in flight, added in column order
        const float x0 = row[c], x1 = row[c + STAT_THREADS], x2 = row[c + 2 * STAT_THREADS], x3 = row[c + 3 * STAT_THREADS];
        take(x0), take(x1), take(x2), take(x3);
    }
    for (; c < n; c += STAT_THREADS) take(row[c]);
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, WAVE);
        n_pos += __shfl_xor(n_pos, off, WAVE);
        n_inf += __shfl_xor(n_inf, off, WAVE);
        mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
    }
    const int wave = threadIdx.x / WAVE;
    if (threadIdx.x % WAVE == 0) sred[wave] = sum, pred[wave] = n_pos, ured[wave] = n_inf, mred[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < STAT_WAVES; ++w) sum += sred[w], n_pos += pred[w], n_inf += ured[w], mx = fmaxf(mx, mred[w]);
        sum_out[blockIdx.x] = sum;
        n_pos_out[blockIdx.x] = n_pos;
        n_unreached_out[blockIdx.x] = n_inf;
        max_out[blockIdx.x] = mx == -INFINITY ? 0.0f : mx;
    }
}

// position of column `col` in the sorted row [lo, hi) of `indices`, or -1
__device__ __forceinline__ int32_t find_entry(const int32_t *__restrict__ indices, int32_t lo, int32_t hi, int32_t col) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        const int32_t v = indices[mid];
        if (v == col) return mid;
        if (v < col) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

__global__ __launch_bounds__(SET_THREADS) void csr_set_symmetric_kernel(const int32_t *__restrict__ indptr,
                                                                        const int32_t *__restrict__ indices,
                                                                        float *__restrict__ data, int32_t n,
                                                                        const int32_t *__restrict__ src,
                                                                        const int32_t *__restrict__ dst,
                                                                        const float *__restrict__ val, int64_t m,
                                                                        int32_t *__restrict__ n_missing) {
    const int64_t t = (int64_t)blockIdx.x * SET_THREADS + threadIdx.x;
    if (t >= m) return;
    const int32_t i = src[t], j = dst[t];
    int32_t a = -1, b = -1;
    if (i >= 0 && i < n && j >= 0 && j < n) {                            // an endpoint outside the graph is a missing entry
        a = find_entry(indices, indptr[i], indptr[i + 1], j);
        b = find_entry(indices, indptr[j], indptr[j + 1], i);
    }
    if (a < 0 || b < 0) {
        atomicAdd(n_missing, 1);
        return;
    }
    const float v = val[t];
    data[a] = v;
    data[b] = v;
}

}  // namespace

extern "C" int geo_path_stats(const float *D, int64_t ld, int32_t n_rows, int64_t n, double *sum_out, int64_t *n_pos_out,
                              int64_t *n_unreached_out, float *max_out, void *stream_) {
    GEO_REQUIRE(D && sum_out && n_pos_out && n_unreached_out && max_out, "geo_path_stats: null pointer");
    GEO_REQUIRE(n_rows >= 1 && n >= 1 && ld >= n, "geo_path_stats: bad shape (n_rows=%d >= 1, n=%lld >= 1, ld=%lld >= n)", n_rows,
                (long long)n, (long long)ld);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(path_stats_kernel, dim3((unsigned)n_rows), dim3(STAT_THREADS), 0, stream, D, ld, n, sum_out,
                       reinterpret_cast<long long *>(n_pos_out), reinterpret_cast<long long *>(n_unreached_out), max_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" int geo_csr_set_symmetric(const int32_t *indptr, const int32_t *indices, float *data, int32_t n, const int32_t *src,
                                     const int32_t *dst, const float *val, int64_t m, int32_t *n_missing_out, void *stream_) {
    GEO_REQUIRE(n_missing_out, "geo_csr_set_symmetric: null pointer");
    GEO_REQUIRE(n >= 0 && m >= 0 && m <= INT32_MAX, "geo_csr_set_symmetric: n=%d or m=%lld outside [0, 2^31)", n, (long long)m);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GEO_HIP_CHECK(hipMemsetAsync(n_missing_out, 0, sizeof(int32_t), stream));
    if (m == 0) return GEO_OK;
    GEO_REQUIRE(indptr && indices && data && src && dst && val, "geo_csr_set_symmetric: null pointer");
    hipLaunchKernelGGL(csr_set_symmetric_kernel, dim3((unsigned)((m + SET_THREADS - 1) / SET_THREADS)), dim3(SET_THREADS), 0,
                       stream, indptr, indices, data, n, src, dst, val, m, n_missing_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}
