// paths.hip -- geodesic paths from geo_sssp_multi's predecessor rows, and points at equal arc length along them (gfx950);
// DESIGN.md section 25.
//
// geo_sssp_paths_count / geo_sssp_paths_fill: the chase from a target back to its source is serial and latency-bound, and pairs
//   are independent, so one lane owns one pair: 64 chases in flight per wave.  count walks and answers hops / status; the caller
//   turns hops + 1 into offsets (a device cumsum); fill walks again and stores the nodes source -> target (walk_fill_kernel),
//   looks the hop weights up with one lane per (pair, hop) slot (hop_weight_kernel: the minimum over the parallel entries of
//   the CSR row) and ends with one sequential fp64 prefix per pair (prefix_kernel) -- the solver's own accumulation order, so
//   (float)cum[hops] is D[row][target] bit for bit.  Every predecessor is checked against [0, n) before it is used as an index:
//   whatever P holds, nothing outside P's S x ld block, the CSR's n rows or the caller's slices is touched.
//
// geo_polyline_resample: one wave per (path, frame).  The segment search is wave-uniform (a bisection of the path's cum
//   slice), the lanes stride over the d coordinates.  a + u (b - a) in fp64 without contraction, rounded once to f32.
//
// Plain vector stores only, no atomics: every output is bit-identical across runs and streams.
#include "geo_common.h"

#include <cmath>

namespace {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int32_t SENTINEL = -9999;          // geo_sssp_multi's "no predecessor"

// The pair's row and target when both are usable as indices, with the row's source; false otherwise (status 2).
__device__ __forceinline__ bool load_pair(const int32_t *__restrict__ sources, const int32_t *__restrict__ rows,
                                          const int32_t *__restrict__ targets, int64_t m, int32_t S, int32_t n, int32_t &r,
                                          int32_t &t, int32_t &src) {
    r = rows[m], t = targets[m];
    if (r < 0 || r >= S || t < 0 || t >= n) return false;
    src = sources[r];
    return src >= 0 && src < n;
}

__global__ __launch_bounds__(THREADS) void walk_count_kernel(const int32_t *__restrict__ P, int64_t ld, int32_t S,
                                                             const int32_t *__restrict__ sources,
                                                             const int32_t *__restrict__ rows,
                                                             const int32_t *__restrict__ targets, int64_t M, int32_t n,
                                                             int32_t max_hops, int32_t *__restrict__ hops_out,
                                                             int32_t *__restrict__ status_out) {
    const int64_t m = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    int32_t r, v, src, hops = 0, status = 2;
    if (load_pair(sources, rows, targets, m, S, n, r, v, src)) {
        const int32_t *__restrict__ row = P + (int64_t)r * ld;
        for (;;) {
            if (v == src) { status = 0; break; }
            if (hops == max_hops) break;                                  // max_hops edges walked, source not reached
            const int32_t p = row[v];
            if (p == SENTINEL) { status = 1; break; }
            if (p < 0 || p >= n) break;
            v = p, ++hops;
        }
    }
    hops_out[m] = status == 0 ? hops : -1;
    status_out[m] = status;
}

// Nodes of pair m into its slice, source -> target; cum gets 0 at the slice's first slot and -1 at the others, which is how
// hop_weight_kernel tells a path's start (no hop ends there) from a hop without searching the offsets.
__global__ __launch_bounds__(THREADS) void walk_fill_kernel(const int32_t *__restrict__ P, int64_t ld, int32_t S,
                                                            const int32_t *__restrict__ sources,
                                                            const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ targets, int64_t M, int32_t n,
                                                            const int64_t *__restrict__ offsets, int64_t T,
                                                            int32_t *__restrict__ nodes_out, double *__restrict__ cum_out) {
    const int64_t m = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    const int64_t off = offsets[m], len = offsets[m + 1] - off;
    if (len <= 0 || off < 0 || len > T || off > T - len) return;         // empty slice, or offsets that are no prefix sum
    int32_t r, v, src;
    const bool ok = load_pair(sources, rows, targets, m, S, n, r, v, src);
    const int32_t *__restrict__ row = P + (int64_t)(ok ? r : 0) * ld;
    if (!ok) v = -1;
    for (int64_t i = len - 1; i >= 0; --i) {
        nodes_out[off + i] = v;                                           // -1 from where the walk left [0, n)
        cum_out[off + i] = i == 0 ? 0.0 : -1.0;
        if (i > 0 && v >= 0) {
            const int32_t p = row[v];
            v = p >= 0 && p < n ? p : -1;
        }
    }
}

// Slot t > a path's start: the weight of the hop nodes[t - 1] -> nodes[t], the minimum over the entries of pull-CSR row nodes[t]
// whose index is nodes[t - 1] (+inf when there is none, NaN when a node is no index).
__global__ __launch_bounds__(THREADS) void hop_weight_kernel(const int32_t *__restrict__ indptr,
                                                             const int32_t *__restrict__ indices,
                                                             const float *__restrict__ weights, int32_t n, int64_t T,
                                                             const int32_t *__restrict__ nodes, double *__restrict__ cum) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t >= T || t == 0 || cum[t] == 0.0) return;                      // slot 0 starts a path whatever it holds
    const int32_t v = nodes[t], u = nodes[t - 1];
    if (v < 0 || v >= n || u < 0 || u >= n) {
        cum[t] = NAN;
        return;
    }
    float w = INFINITY;
    for (int32_t e = indptr[v], e1 = indptr[v + 1]; e < e1; ++e)
        if (indices[e] == u) w = fminf(w, weights ? weights[e] : 1.0f);
    cum[t] = (double)w;
}

// cum[i] = cum[i - 1] + w_i, source outward, one rounding per hop: the order in which the solver built the distance.
__global__ __launch_bounds__(THREADS) void prefix_kernel(const int64_t *__restrict__ offsets, int64_t M, int64_t T,
                                                         double *__restrict__ cum) {
    const int64_t m = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    const int64_t off = offsets[m], len = offsets[m + 1] - off;
    if (len <= 0 || off < 0 || len > T || off > T - len) return;
    double acc = 0.0;
    for (int64_t i = 1; i < len; ++i) {
        acc += cum[off + i];
        cum[off + i] = acc;
    }
}

__global__ __launch_bounds__(THREADS) void resample_kernel(const float *__restrict__ z, int64_t n, int32_t d,
                                                           const int32_t *__restrict__ nodes,
                                                           const int64_t *__restrict__ offsets,
                                                           const double *__restrict__ cum, int64_t M, int32_t F,
                                                           float *__restrict__ frames_out) {
#pragma clang fp contract(off)      // plain operators below: the pragma governs them (not the bodies of inlined intrinsics)
    const int64_t item = (int64_t)blockIdx.x * (THREADS / WAVE) + threadIdx.x / WAVE;      // (path, frame), one per wave
    if (item >= M * F) return;
    const int64_t m = item / F;
    const int32_t f = (int32_t)(item % F);
    const int64_t off = offsets[m], len = offsets[m + 1] - off;
    if (len <= 0) return;                                                 // no path: the caller's fill value stays
    const int64_t hops = len - 1;
    const double *__restrict__ c = cum + off;
    int64_t i = 0;
    double u = 0.0;
    if (f == F - 1) {
        i = hops;                                                         // the target itself, not a rounded product
    } else if (f > 0 && hops > 0) {
        const double s = c[hops] * (double)f / (double)(F - 1);
        int64_t lo = 0, hi = hops - 1;                                    // largest i <= hops - 1 with cum[i] <= s; cum[0] = 0 <= s
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if (c[mid] <= s) lo = mid;
            else hi = mid - 1;
        }
        i = lo;
        const double den = c[i + 1] - c[i];
        u = den == 0.0 ? 0.0 : (s - c[i]) / den;
    }
    const int32_t na = nodes[off + i], nb = nodes[off + (i < hops ? i + 1 : i)];
    if (na < 0 || na >= n || nb < 0 || nb >= n) return;
    const float *__restrict__ za = z + (int64_t)na * d, *__restrict__ zb = z + (int64_t)nb * d;
    float *__restrict__ out = frames_out + item * d;
    for (int32_t k = threadIdx.x % WAVE; k < d; k += WAVE) {
        const double a = (double)za[k], b = (double)zb[k];
        out[k] = (float)(a + u * (b - a));                                // three roundings in fp64, then one to f32
    }
}

unsigned blocks_for(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

int check_walk_args(const char *who, const void *P, int64_t ld, int32_t S, const void *sources, const void *rows,
                    const void *targets, int64_t M, int32_t n) {
    GEO_REQUIRE(M >= 0 && M < ((int64_t)1 << 31), "%s: M=%lld outside [0, 2^31)", who, (long long)M);
    GEO_REQUIRE(n >= 1 && S >= 1 && ld >= n, "%s: bad shape (n=%d >= 1, S=%d >= 1, ld=%lld >= n)", who, n, S, (long long)ld);
    GEO_REQUIRE(M == 0 || (P && sources && rows && targets), "%s: null pointer", who);
    return GEO_OK;
}

}  // namespace

extern "C" int geo_sssp_paths_count(const int32_t *P, int64_t ld, int32_t S, const int32_t *sources, const int32_t *rows,
                                    const int32_t *targets, int64_t M, int32_t n, int32_t max_hops, int32_t *hops_out,
                                    int32_t *status_out, void *stream_) {
    if (int rc = check_walk_args("geo_sssp_paths_count", P, ld, S, sources, rows, targets, M, n)) return rc;
    GEO_REQUIRE(max_hops >= 0 && max_hops <= n - 1, "geo_sssp_paths_count: max_hops=%d outside [0, n - 1 = %d]", max_hops, n - 1);
    if (M == 0) return GEO_OK;
    GEO_REQUIRE(hops_out && status_out, "geo_sssp_paths_count: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream_);
    walk_count_kernel<<<blocks_for(M, THREADS), THREADS, 0, s>>>(P, ld, S, sources, rows, targets, M, n, max_hops, hops_out,
                                                                 status_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" int geo_sssp_paths_fill(const int32_t *P, int64_t ld, int32_t S, const int32_t *sources, const int32_t *rows,
                                   const int32_t *targets, int64_t M, int32_t n, const int32_t *indptr, const int32_t *indices,
                                   const float *weights, const int64_t *offsets, int64_t T, int32_t *nodes_out, double *cum_out,
                                   void *stream_) {
    if (int rc = check_walk_args("geo_sssp_paths_fill", P, ld, S, sources, rows, targets, M, n)) return rc;
    GEO_REQUIRE(T >= 0 && T < ((int64_t)1 << 40), "geo_sssp_paths_fill: T=%lld outside [0, 2^40)", (long long)T);
    if (M == 0 || T == 0) return GEO_OK;
    GEO_REQUIRE(indptr && indices && offsets && nodes_out && cum_out, "geo_sssp_paths_fill: null pointer");
    GEO_REQUIRE((T + THREADS - 1) / THREADS < ((int64_t)1 << 31), "geo_sssp_paths_fill: T=%lld too large for one grid",
                (long long)T);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    walk_fill_kernel<<<blocks_for(M, THREADS), THREADS, 0, s>>>(P, ld, S, sources, rows, targets, M, n, offsets, T, nodes_out,
                                                                cum_out);
    GEO_LAUNCH_CHECK();
    hop_weight_kernel<<<blocks_for(T, THREADS), THREADS, 0, s>>>(indptr, indices, weights, n, T, nodes_out, cum_out);
    GEO_LAUNCH_CHECK();
    prefix_kernel<<<blocks_for(M, THREADS), THREADS, 0, s>>>(offsets, M, T, cum_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

extern "C" int geo_polyline_resample(const float *z, int64_t n, int32_t d, const int32_t *nodes, const int64_t *offsets,
                                     const double *cum, int64_t M, int32_t F, float *frames_out, void *stream_) {
    GEO_REQUIRE(M >= 0 && M < ((int64_t)1 << 31) && F >= 2 && d >= 1 && n >= 1,
                "geo_polyline_resample: bad shape (0 <= M=%lld < 2^31, F=%d >= 2, d=%d >= 1, n=%lld >= 1)", (long long)M, F, d,
                (long long)n);
    GEO_REQUIRE(M * F < ((int64_t)1 << 32), "geo_polyline_resample: M F = %lld frames, 2^32 at most", (long long)(M * F));
    if (M == 0) return GEO_OK;
    GEO_REQUIRE(z && nodes && offsets && cum && frames_out, "geo_polyline_resample: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream_);
    resample_kernel<<<blocks_for(M * F, THREADS / WAVE), THREADS, 0, s>>>(z, n, d, nodes, offsets, cum, M, F, frames_out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}
