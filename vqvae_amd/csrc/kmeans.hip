// kmeans.hip -- Euclidean k-means (sklearn.cluster.KMeans, algorithm="lloyd", k-means++ seeding) on gfx950.
//
// Replaces the CPU KMeans(n_clusters=K, random_state=seed, n_init=10) of the reference's demos/codebook_comparison.py:73-77.
// Three entry points (include/geo_hip.h):
//
//   geo_kmeans_assign  labels = argmin_j key(x, c_j), key = fp64 fma chain of (x_c - c_jc)^2 over c ascending, ties to the
//                      lowest j.  A float32 MFMA screen (v_mfma_f32_32x32x2_f32) of |c_j|^2 - 2 x.c_j decides a row alone
//                      when its second-best screened value lies more than the margin above its best; every other
//                      row ("fallback row") is re-keyed exactly against all K centres.
//   geo_kmeans_pp      k-means++ seeding, all n_init starts at once, from host-supplied draws (sklearn's _kmeans_plusplus).
//   geo_kmeans_lloyd   the Lloyd loop of sklearn's _kmeans_single_lloyd for each start: exact labels, per-cluster fp64 sums in
//                      ascending row order, empty-cluster relocation, centre shift, strict / tol / max_iter stopping.
// and the EMA vector quantizer of the baseline VQ-VAE (geo_vq_forward / geo_vq_backward, end of the file), built on the same
// assignment and cluster-sum kernels.
//
// Screening margin (geo_kmeans_assign).  Let u = 2^-24, x and c float32 vectors of dimension d, X = |x|^2, C = max_j |c_j|^2.
//   screen  s_j = fl(fma(-2, dot_j, n_j)), dot_j the f32 fma chain of x.c_j (the MFMA is bit-for-bit that chain), n_j the f32
//           fma chain of |c_j|^2.  With T_j = |c_j|^2 - 2 x.c_j (exact):
//             |dot_j - x.c_j| <= gamma_d sum|x_k c_jk| <= gamma_d |x||c_j|,   |n_j - |c_j|^2| <= gamma_d |c_j|^2,
//             |s_j - T_j| <= gamma_d (|c_j|^2 + 2|x||c_j|) + u (1 + gamma_d)(|c_j|^2 + 2|x||c_j|) <= gamma_{d+1} * 2 (X + C),
//           gamma_m = m u / (1 - m u), using 2|x||c_j| <= X + |c_j|^2.
//   key     E_j = fp64 chain over d terms; each difference rounds once, each fma once: |E_j - D_j| <= gamma64_{d+2} D_j with
//           D_j = |x - c_j|^2 <= 2 (X + C) and gamma64 built on 2^-53 -- below 2^-25 of the f32 term for every d <= 128.
//   claim   j* = argmin E_j is among {j : s_j <= s_min + M}.  With s_min = s_m:
//             s_j* - s_m <= (T_j* - T_m) + 4 gamma_{d+1} (X + C) = (D_j* - D_m) + ... <= (E_j* - E_m) + 2 gamma64_{d+2} 2 (X + C)
//                           + 4 gamma_{d+1} (X + C) <= 4 (d + 2) u (X + C) (1 + 2^-20)   since E_j* <= E_m.
//   M = 8 (d + 2) u (X~ + C~), X~ and C~ the float32 norms (each >= (1 - gamma_d) times the exact one, C~ rounded up), evaluated
//   in float32: the factor 2 covers those shortfalls, the rounding of M itself and of s_min + M (|s_min| <= 2 (X + C)).
//   A row is decided by the screen alone iff its second-smallest screened value s_(2) > s_min + M: then only the screen's
//   argmin can be j*, and its key is evaluated exactly.  Otherwise (near ties, exact ties, duplicate centres, inf / overflow)
//   the row is a fallback row: one wave evaluates E_j for all K centres and takes the lexicographic minimum of (E_j, j).
//
// Determinism: no float atomics.  Integer atomics only count (order-free); every floating sum has a fixed association
// that depends on the shapes alone.
#include "geo_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int CHUNK = 1024;        // rows per histogram / scatter chunk and per k-means++ segment
constexpr int MAX_K = 4096;
constexpr int MAX_D = 128;
constexpr int MAX_TRIALS = 64;

__device__ __forceinline__ double exact_key(const float *__restrict__ x, const float *__restrict__ c, int d) {
    double acc = 0.0;
    for (int k = 0; k < d; ++k) {
        const double t = (double)x[k] - (double)c[k];
        acc = fma(t, t, acc);
    }
    return acc;
}

// Order of (key, index) in the exact fallback: ascending key, ties to the lower index, a NaN key before every number (the
// rule of torch.argmin).  On finite keys it is the plain (key, index) order; it also gives a row whose keys are all +inf or
// NaN (a non-finite row or centre) a real index -- the first one -- instead of the loop's start value.
__device__ __forceinline__ bool key_before(double a, int ia, double b, int ib) {
    const bool na = isnan(a), nb = isnan(b);
    if (na != nb) return na;
    if (na) return ia < ib;
    return a < b || (a == b && ia < ib);
}

// Loop status of one start, device resident.  The kernels of an iteration return at once when `done` is set, so the host
// enqueues iterations in batches and synchronises once per batch.
struct Status {
    int32_t iter;       // index of the iteration now running
    int32_t done;
    int32_t strict;
    int32_t n_iter;
    int32_t n_changed;  // rows whose label changed in this iteration
    int32_t n_empty;
    uint32_t cmax_bits; // float bits of max_j |c_j|^2 (rounded up), atomicMax on non-negative floats
    int32_t pad;
    unsigned long long n_fallback;
};

// ---------------------------------------------------------------------------------------------------------------------
// Centre packing: A-operand image Ap[tile][s][lane] = c[tile*32 + (lane & 31)][2s + (lane >> 5)] (0 outside), and the f32
// norms in the accumulator's row order: cnp[tile][h*16 + r] = n of centre tile*32 + (r & 3) + 8 (r >> 2) + 4 h (+inf for pads).
// ---------------------------------------------------------------------------------------------------------------------
__global__ void km_pack_kernel(const float *__restrict__ C, int K, int d, int ns, int ntiles, float *__restrict__ Ap,
                               float *__restrict__ cnp, Status *st, int gated) {
    if (gated && st->done) return;
    const int64_t total = (int64_t)ntiles * ns * 64;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e & 63);
        const int64_t ts = e >> 6;
        const int s = (int)(ts % ns), tile = (int)(ts / ns);
        const int j = tile * 32 + (lane & 31), k = 2 * s + (lane >> 5);
        Ap[e] = (j < K && k < d) ? C[(size_t)j * d + k] : 0.f;
    }
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < (int64_t)ntiles * 32; e += (int64_t)gridDim.x * blockDim.x) {
        const int tile = (int)(e >> 5), hr = (int)(e & 31), h = hr >> 4, r = hr & 15;
        const int j = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float n = INFINITY;
        if (j < K) {
            const float *c = C + (size_t)j * d;
            float a = 0.f;
            double a64 = 0.0;
            for (int k = 0; k < d; ++k) {
                a = fmaf(c[k], c[k], a);
                a64 = fma((double)c[k], (double)c[k], a64);
            }
            n = a;
            const float up = (float)(a64 * (1.0 + 0x1p-20));
            atomicMax(&st->cmax_bits, __float_as_uint(isfinite(up) ? up : INFINITY));
        }
        cnp[e] = n;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Assignment.  One wave = 32 rows; B operand = the rows (lane: row l & 31, dims 2s + (l >> 5)), A operand = 32 centres, so
// D[i = centre][j = row]: each lane holds one row and 16 of the tile's centres.
// labels_io: when count_changes != 0 it holds the previous labels, compared and overwritten in place.
// ---------------------------------------------------------------------------------------------------------------------
template <int NS>
__global__ __launch_bounds__(256) void km_assign_kernel(const float *__restrict__ X, int64_t n, int d, const float *__restrict__ Ap,
                                                        const float *__restrict__ cnp, const float *__restrict__ C, int K,
                                                        int ntiles, int32_t *__restrict__ labels_io, double *__restrict__ keys,
                                                        int count_changes, Status *st, int gated) {
    if (gated && st->done) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
    if (row0 >= n) return;
    const int r = lane & 31, h = lane >> 5;
    const int64_t row = row0 + r;
    const bool valid = row < n;
    float xb[NS];
    float xn = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int k = 2 * s + h;
        xb[s] = (valid && k < d) ? X[row * d + k] : 0.f;
        xn = fmaf(xb[s], xb[s], xn);
    }
    xn += __shfl_xor(xn, 32);
    float s1 = INFINITY, s2 = INFINITY;
    int j1 = 0;
    for (int tile = 0; tile < ntiles; ++tile) {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float *ap = Ap + (size_t)tile * NS * 64 + lane;
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[s * 64], xb[s], acc, 0, 0, 0);
        const float4 *cp = reinterpret_cast<const float4 *>(cnp + (size_t)tile * 32 + h * 16);
        float cn[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = cp[q];
            cn[4 * q] = v.x; cn[4 * q + 1] = v.y; cn[4 * q + 2] = v.z; cn[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float sv = fmaf(-2.f, acc[q], cn[q]);
            const int j = tile * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
            if (sv < s1) {
                s2 = s1; s1 = sv; j1 = j;
            } else if (sv < s2) {
                s2 = sv;
            }
        }
    }
    const float os1 = __shfl_xor(s1, 32), os2 = __shfl_xor(s2, 32);
    const int oj1 = __shfl_xor(j1, 32);
    const float m1 = fminf(s1, os1), m2 = fminf(fminf(s2, os2), fmaxf(s1, os1));
    const int jm = (s1 < os1 || (s1 == os1 && j1 < oj1)) ? j1 : oj1;
    const float cmax = __uint_as_float(st->cmax_bits);
    const float margin = 8.f * (float)(d + 2) * 0x1p-24f * (xn + cmax);
    const bool fallback = valid && h == 0 && !(m2 > m1 + margin);
    int label = jm;
    double key = 0.0;
    if (valid && h == 0 && !fallback) key = exact_key(X + row * d, C + (size_t)jm * d, d);
    unsigned long long fb = __ballot(fallback);
    if (lane == 0 && fb) atomicAdd(&st->n_fallback, (unsigned long long)__popcll(fb));
    while (fb) {
        const int rr = __ffsll((long long)fb) - 1;
        fb &= fb - 1;
        const float *xr = X + (row0 + rr) * d;
        double bk = INFINITY;
        int bj = 0x7fffffff;
        for (int j = lane; j < K; j += 64) {
            const double kj = exact_key(xr, C + (size_t)j * d, d);
            if (key_before(kj, j, bk, bj)) { bk = kj; bj = j; }   // ascending j per lane: the first minimum stays
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ok = __shfl_xor(bk, off);
            const int oj = __shfl_xor(bj, off);
            if (key_before(ok, oj, bk, bj)) { bk = ok; bj = oj; }
        }
        if (lane == rr) { label = bj; key = bk; }
    }
    bool changed = false;
    if (valid && h == 0) {
        if (count_changes) changed = labels_io[row] != label;
        labels_io[row] = label;
        if (keys) keys[row] = key;
    }
    const unsigned long long ch = __ballot(changed);
    if (lane == 0 && ch) atomicAdd(&st->n_changed, __popcll(ch));
}

// Keys of given labels: keys[i] = key(x_i, c_labels[i]).
__global__ void km_label_keys_kernel(const float *__restrict__ X, int64_t n, int d, const float *__restrict__ C,
                                     const int32_t *__restrict__ labels, double *__restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        keys[i] = exact_key(X + i * d, C + (size_t)labels[i] * d, d);
}

// Fixed-order fp64 sum of v[0..n): thread t sums t, t + 1024, ... ascending, then the 1024 partials are summed ascending.
__global__ __launch_bounds__(1024) void km_sum_kernel(const double *__restrict__ v, int64_t n, double *__restrict__ out) {
    __shared__ double part[1024];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) a += v[i];
    part[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < 1024; ++t) s += part[t];
        *out = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Update: stable counting sort of the rows by label (chunk histograms -> per-cluster chunk offsets -> cluster offsets ->
// scatter with the rank inside the chunk), then per-cluster sums in ascending row order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void km_hist_kernel(const int32_t *__restrict__ labels, int64_t n, int K,
                                                      int32_t *__restrict__ chunk_hist, const Status *st) {
    if (st->done) return;
    extern __shared__ int32_t hist[];
    for (int k = threadIdx.x; k < K; k += 256) hist[k] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * CHUNK;
    for (int t = threadIdx.x; t < CHUNK; t += 256)
        if (base + t < n) atomicAdd(&hist[labels[base + t]], 1);
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) chunk_hist[(size_t)blockIdx.x * K + k] = hist[k];
}

// Per cluster: exclusive offsets over the chunks (in place) and the count.  64 clusters per block, 16 waves over chunk ranges.
__global__ __launch_bounds__(1024) void km_colscan_kernel(int32_t *__restrict__ chunk_hist, int nchunk, int K,
                                                          int32_t *__restrict__ counts, const Status *st) {
    if (st->done) return;
    __shared__ int32_t wsum[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    const int per = (nchunk + 15) / 16, c0 = w * per, c1 = min(nchunk, c0 + per);
    int32_t a = 0;
    if (k < K)
        for (int c = c0; c < c1; ++c) a += chunk_hist[(size_t)c * K + k];
    wsum[w][lane] = a;
    __syncthreads();
    int32_t off = 0;
    for (int q = 0; q < w; ++q) off += wsum[q][lane];
    if (k < K) {
        for (int c = c0; c < c1; ++c) {
            const int32_t v = chunk_hist[(size_t)c * K + k];
            chunk_hist[(size_t)c * K + k] = off;
            off += v;
        }
        if (w == 15) counts[k] = off;
    }
}

// Cluster offsets (exclusive, offs[K] = n) and the number of empty clusters.  One block.
__global__ __launch_bounds__(1024) void km_offsets_kernel(const int32_t *__restrict__ counts, int K, int32_t *__restrict__ offs,
                                                          Status *st) {
    if (st->done) return;
    __shared__ int32_t tsum[1024];
    __shared__ int32_t nempty;
    if (threadIdx.x == 0) nempty = 0;
    const int per = (K + 1023) / 1024, k0 = threadIdx.x * per, k1 = min(K, k0 + per);
    int32_t a = 0, e = 0;
    for (int k = k0; k < k1; ++k) { a += counts[k]; e += counts[k] == 0; }
    tsum[threadIdx.x] = a;
    __syncthreads();
    if (e) atomicAdd(&nempty, e);
    if (threadIdx.x == 0) {
        int32_t s = 0;
        for (int t = 0; t < 1024; ++t) { const int32_t v = tsum[t]; tsum[t] = s; s += v; }
        offs[K] = s;
    }
    __syncthreads();
    int32_t off = tsum[threadIdx.x];
    for (int k = k0; k < k1; ++k) { offs[k] = off; off += counts[k]; }
    if (threadIdx.x == 0) st->n_empty = nempty;
}

__global__ __launch_bounds__(CHUNK) void km_scatter_kernel(const int32_t *__restrict__ labels, int64_t n, int K,
                                                           const int32_t *__restrict__ chunk_off, const int32_t *__restrict__ offs,
                                                           int32_t *__restrict__ order, const Status *st) {
    if (st->done) return;
    __shared__ int32_t lab[CHUNK];
    const int64_t base = (int64_t)blockIdx.x * CHUNK;
    const int t = threadIdx.x;
    const int my = base + t < n ? labels[base + t] : -1;
    lab[t] = my;
    __syncthreads();
    if (my < 0) return;
    int rank = 0;
    for (int q = 0; q < t; ++q) rank += lab[q] == my;
    order[offs[my] + chunk_off[(size_t)blockIdx.x * K + my] + rank] = (int32_t)(base + t);
}

// sums[k][c] = sum over the members of k, ascending row order split round-robin over G = 256 / d groups, groups summed ascending.
__global__ __launch_bounds__(256) void km_csum_kernel(const float *__restrict__ X, int d, const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ offs, double *__restrict__ sums, const Status *st) {
    if (st->done) return;
    __shared__ double part[256];
    const int k = blockIdx.x, G = 256 / d, t = threadIdx.x;
    const int g = t / d, c = t % d;
    const int32_t m0 = offs[k], cnt = offs[k + 1] - m0;
    double a = 0.0;
    if (g < G)
        for (int m = g; m < cnt; m += G) a += (double)X[(int64_t)order[m0 + m] * d + c];
    part[t] = a;
    __syncthreads();
    if (t < d) {
        double s = 0.0;
        for (int q = 0; q < G; ++q) s += part[q * d + t];
        sums[(size_t)k * d + t] = s;
    }
}

// Empty-cluster relocation (sklearn _relocate_empty_clusters_dense): the empty clusters, ascending, take the rows farthest
// from their old centre (keys), ordered by (key descending, row ascending); skipped when every key is 0.  One block.
__global__ __launch_bounds__(1024) void km_relocate_kernel(const float *__restrict__ X, int64_t n, int d, int K,
                                                           const int32_t *__restrict__ labels, const double *__restrict__ keys,
                                                           double *__restrict__ sums, int32_t *__restrict__ counts, Status *st) {
    if (st->done || st->n_empty == 0) return;
    __shared__ double bk[1024];
    __shared__ int64_t bi[1024];
    __shared__ int64_t pick;
    __shared__ double pick_key;
    __shared__ uint8_t was_empty[MAX_K];   // sklearn fixes the list of empty clusters before moving any row
    for (int k = threadIdx.x; k < K; k += 1024) was_empty[k] = counts[k] == 0;
    __syncthreads();
    double prev_key = INFINITY;
    int64_t prev_idx = -1;
    int e_next = 0;
    for (int round = 0; round < st->n_empty; ++round) {
        double best = -1.0;
        int64_t besti = -1;
        for (int64_t i = threadIdx.x; i < n; i += 1024) {
            const double kv = keys[i];
            const bool after = kv < prev_key || (kv == prev_key && i > prev_idx);
            if (after && (kv > best)) { best = kv; besti = i; }   // ascending i per thread: the first maximum stays
        }
        bk[threadIdx.x] = best;
        bi[threadIdx.x] = besti;
        __syncthreads();
        if (threadIdx.x == 0) {
            double b = -1.0;
            int64_t bj = -1;
            for (int t = 0; t < 1024; ++t)
                if (bi[t] >= 0 && (bk[t] > b || (bk[t] == b && bi[t] < bj))) { b = bk[t]; bj = bi[t]; }
            pick = bj;
            pick_key = b;
        }
        __syncthreads();
        const int64_t r = pick;
        const double rk = pick_key;
        __syncthreads();
        if (round == 0 && !(rk > 0.0)) return;   // max distance 0 (more clusters than distinct rows): nothing to do
        if (r < 0) return;
        prev_key = rk;
        prev_idx = r;
        // next empty cluster in ascending order
        while (e_next < K && !was_empty[e_next]) ++e_next;
        __syncthreads();
        if (e_next >= K) return;
        const int ne = e_next, old = labels[r];
        for (int c = threadIdx.x; c < d; c += 1024) {
            const double xv = (double)X[r * d + c];
            sums[(size_t)old * d + c] -= xv;
            sums[(size_t)ne * d + c] = xv;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            counts[ne] = 1;
            counts[old] -= 1;
        }
        __syncthreads();
        ++e_next;
    }
}

// New centres f32(sum / count) and shift2[k] = fp64 |new - old|^2.  A cluster left with no member (no relocation: every key 0,
// or a relocation emptied its donor) goes where sklearn's _average_centers puts it: onto the biggest cluster (first maximum of
// the counts), whose row it copies as it stands at that point of sklearn's ascending loop -- still the plain sum when the
// biggest cluster comes later, its mean when it came earlier.
__global__ __launch_bounds__(128) void km_finalize_kernel(const double *__restrict__ sums, const int32_t *__restrict__ counts,
                                                          int K, int d, const float *__restrict__ Cold, float *__restrict__ Cnew,
                                                          double *__restrict__ shift2, const Status *st) {
    if (st->done) return;
    __shared__ double df[MAX_D];
    __shared__ int32_t big;
    const int k = blockIdx.x, c = threadIdx.x;
    const int32_t cnt = counts[k];
    if (cnt <= 0) {
        if (c == 0) {
            int32_t b = 0;
            for (int j = 1; j < K; ++j)
                if (counts[j] > counts[b]) b = j;
            big = b;
        }
        __syncthreads();
    }
    if (c < d) {
        float v;
        if (cnt > 0) {
            v = (float)(sums[(size_t)k * d + c] / (double)cnt);
        } else {
            const int b = big;
            const double sb = sums[(size_t)b * d + c];
            v = (k < b || counts[b] <= 0) ? (float)sb : (float)(sb / (double)counts[b]);
        }
        Cnew[(size_t)k * d + c] = v;
        df[c] = (double)v - (double)Cold[(size_t)k * d + c];
    }
    __syncthreads();
    if (c == 0) {
        double a = 0.0;
        for (int q = 0; q < d; ++q) a = fma(df[q], df[q], a);
        shift2[k] = a;
    }
}

// End of iteration: stopping rule of _kmeans_single_lloyd, reset of the per-iteration counters.  One block.
__global__ __launch_bounds__(256) void km_status_kernel(const double *__restrict__ shift2, int K, double tol, int max_iter,
                                                        Status *st) {
    if (st->done) return;
    __shared__ double part[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < K; k += 256) a += shift2[k];
    part[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    for (int t = 0; t < 256; ++t) tot += part[t];
    const int i = st->iter;
    st->n_iter = i + 1;
    if (st->n_changed == 0) {
        st->strict = 1;
        st->done = 1;
    } else if (tot <= tol) {
        st->done = 1;
    } else if (i + 1 >= max_iter) {
        st->done = 1;
    }
    st->iter = i + 1;
    st->n_changed = 0;
    st->n_empty = 0;
    if (!st->done) st->cmax_bits = 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// k-means++ (sklearn _kmeans_plusplus), all starts at once (blockIdx.y = start).
//   closest_s = f32(key) min-folded; cumsum C[i] = fl(O_b + P_b[i]) with b = i / 1024 the segment, P_b the in-segment
//   inclusive fp64 prefix (4 rows per thread ascending, then a fixed wave / block scan), O_b the exclusive fp64 prefix of the
//   segment totals (fixed scan); draw = first i < n with C[i] >= u * pot, else n - 1.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

__global__ __launch_bounds__(256) void pp_update_scan_kernel(const float *__restrict__ X, int64_t n, int d, int K, int c,
                                                             const int32_t *__restrict__ idx, float *__restrict__ closest,
                                                             double *__restrict__ P, double *__restrict__ segT,
                                                             double *__restrict__ segMax, int nseg) {
    __shared__ double wtot[4];
    __shared__ float cx[MAX_D];
    const int s = blockIdx.y, b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int32_t src = idx[(size_t)s * K + c - 1];
    for (int q = t; q < d; q += 256) cx[q] = X[(int64_t)src * d + q];
    __syncthreads();
    float *cl = closest + (size_t)s * n;
    double *Ps = P + (size_t)s * n;
    double loc[4];
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = (int64_t)b * CHUNK + 4 * t + q;
        float v = 0.f;
        if (i < n) {
            const float kf = (float)exact_key(X + i * d, cx, d);
            v = c == 1 ? kf : fminf(cl[i], kf);
            cl[i] = v;
        }
        a += (double)v;
        loc[q] = a;
    }
    const double inc = wave_incl_scan(a, lane);
    if (lane == 63) wtot[w] = inc;
    __syncthreads();
    double off = __shfl_up(inc, 1);   // exclusive within the wave: the previous lane's inclusive value
    if (lane == 0) off = 0.0;
    double wo = 0.0;
    for (int q = 0; q < w; ++q) wo += wtot[q];
    const double ex = wo + off;
    double mx = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t i = (int64_t)b * CHUNK + 4 * t + q;
        const double p = ex + loc[q];
        if (i < n) { Ps[i] = p; mx = fmax(mx, p); }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    __shared__ double wmx[4];
    if (lane == 0) wmx[w] = mx;
    __syncthreads();
    if (t == 255) segT[(size_t)s * nseg + b] = ex + loc[3];
    if (t == 0) segMax[(size_t)s * nseg + b] = fmax(fmax(wmx[0], wmx[1]), fmax(wmx[2], wmx[3]));
}

// One block per start: segment offsets, then the L draws of step c.
__global__ __launch_bounds__(1024) void pp_search_kernel(int64_t n, int K, int c, int L, const double *__restrict__ P,
                                                         const double *__restrict__ segT, const double *__restrict__ segMax,
                                                         int nseg, const double *__restrict__ u, float *__restrict__ pot,
                                                         int32_t *__restrict__ cand) {
    extern __shared__ double O[];   // nseg + 1
    __shared__ double tsum[1024];
    __shared__ int64_t first;
    const int s = blockIdx.x, t = threadIdx.x;
    const double *T = segT + (size_t)s * nseg, *M = segMax + (size_t)s * nseg;
    const int per = (nseg + 1023) / 1024, b0 = t * per, b1 = min(nseg, b0 + per);
    double a = 0.0;
    for (int b = b0; b < b1; ++b) a += T[b];
    tsum[t] = a;
    __syncthreads();
    if (t == 0) {
        double x = 0.0;
        for (int q = 0; q < 1024; ++q) { const double v = tsum[q]; tsum[q] = x; x += v; }
        O[nseg] = x;
    }
    __syncthreads();
    double o = tsum[t];
    for (int b = b0; b < b1; ++b) { O[b] = o; o += T[b]; }
    __syncthreads();
    if (c == 1 && t == 0) pot[s] = (float)O[nseg];
    __syncthreads();
    const double cur = (double)pot[s];
    const double *Ps = P + (size_t)s * n;
    for (int tr = 0; tr < L; ++tr) {
        const double v = u[((size_t)s * (K - 1) + (c - 1)) * L + tr] * cur;
        if (t == 0) first = INT64_MAX;
        __syncthreads();
        for (int b = t; b < nseg; b += 1024)
            if (O[b] + M[b] >= v) atomicMin((unsigned long long *)&first, (unsigned long long)b);
        __syncthreads();
        const int64_t sb = first;
        __syncthreads();
        if (t == 0) first = INT64_MAX;
        __syncthreads();
        if (sb != INT64_MAX) {
            const int64_t i = sb * CHUNK + t;
            if (t < CHUNK && i < n && O[sb] + Ps[i] >= v) atomicMin((unsigned long long *)&first, (unsigned long long)i);
        }
        __syncthreads();
        if (t == 0) cand[(size_t)s * L + tr] = (int32_t)(first == INT64_MAX ? n - 1 : first);
        __syncthreads();
    }
}

// Candidate pots: partial[s][tr][chunk] = fixed-order fp64 sum over the chunk of min(closest, f32(key(x_i, x_cand))).
__global__ __launch_bounds__(256) void pp_cand_kernel(const float *__restrict__ X, int64_t n, int d, int L,
                                                      const int32_t *__restrict__ cand, const float *__restrict__ closest,
                                                      double *__restrict__ partial, int nseg) {
    extern __shared__ float cx[];   // L x d
    __shared__ double wp[4];
    const int s = blockIdx.y, b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int q = t; q < L * d; q += 256) cx[q] = X[(int64_t)cand[(size_t)s * L + q / d] * d + q % d];
    __syncthreads();
    const float *cl = closest + (size_t)s * n;
    for (int tr = 0; tr < L; ++tr) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = (int64_t)b * CHUNK + 4 * t + q;
            if (i < n) a += (double)fminf(cl[i], (float)exact_key(X + i * d, cx + tr * d, d));
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) wp[w] = a;
        __syncthreads();
        if (t == 0) partial[((size_t)s * L + tr) * nseg + b] = ((wp[0] + wp[1]) + wp[2]) + wp[3];
        __syncthreads();
    }
}

// Best candidate: pot_tr = f32(fixed-order sum of the chunk partials: lane-strided, then a butterfly); the first minimum wins.
__global__ __launch_bounds__(1024) void pp_select_kernel(int K, int c, int L, const int32_t *__restrict__ cand,
                                                         const double *__restrict__ partial, int nseg, float *__restrict__ pot,
                                                         int32_t *__restrict__ idx) {
    __shared__ float pots[MAX_TRIALS];
    const int s = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int tr = w; tr < L; tr += 16) {
        const double *p = partial + ((size_t)s * L + tr) * nseg;
        double a = 0.0;
        for (int b = lane; b < nseg; b += 64) a += p[b];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) pots[tr] = (float)a;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float best = pots[0];
    int bt = 0;
    for (int tr = 1; tr < L; ++tr)
        if (pots[tr] < best) { best = pots[tr]; bt = tr; }
    pot[s] = best;
    idx[(size_t)s * K + c] = cand[(size_t)s * L + bt];
}

__global__ void gather_rows_kernel(const float *__restrict__ X, int d, const int32_t *__restrict__ idx, int64_t rows,
                                   float *__restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < rows * d; e += (int64_t)gridDim.x * blockDim.x)
        out[e] = X[(int64_t)idx[e / d] * d + e % d];
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------------------------------
int ns_for(int d) {
    int ns = 1;
    while (2 * ns < d) ns *= 2;
    return ns;
}

struct Plan {
    // assignment / Lloyd
    float *Ap, *cnp, *C0, *C1;
    double *keys, *sums, *shift2, *scal;
    int32_t *chunk_hist, *counts, *offs, *order;
    Status *st;
    // k-means++
    float *closest, *pot;
    double *P, *segT, *segMax, *partial, *u;
    int32_t *cand;
};

// What the k-means calls and the vector quantizer both keep, as two sub-layouts: the centre packing and the status of the
// assignment, and the counting sort with the per-cluster sums.
void lay_out_assign(geo::Arena &ar, Plan *p, int d, int K) {
    const int ns = ns_for(d), ntiles = (K + 31) / 32;
    ar.take(p->Ap, (size_t)ntiles * ns * 64);
    ar.take(p->cnp, (size_t)ntiles * 32);
    ar.take(p->st, 1);
}

void lay_out_sort(geo::Arena &ar, Plan *p, int64_t n, int d, int K) {
    const int64_t nchunk = (n + CHUNK - 1) / CHUNK;
    ar.take(p->chunk_hist, (size_t)nchunk * K);
    ar.take(p->counts, (size_t)K);
    ar.take(p->offs, (size_t)(K + 1));
    ar.take(p->order, (size_t)n);
    ar.take(p->sums, (size_t)K * d);
}

// The one workspace of geo_kmeans_assign / _pp / _lloyd (S starts, L trials): measured by geo_kmeans_workspace_bytes.
Plan lay_out(geo::Arena &ar, int64_t n, int d, int K, int S, int L) {
    Plan p;
    const int64_t nchunk = (n + CHUNK - 1) / CHUNK;
    lay_out_assign(ar, &p, d, K);
    ar.take(p.C0, (size_t)K * d);
    ar.take(p.C1, (size_t)K * d);
    ar.take(p.keys, (size_t)n);
    ar.take(p.shift2, (size_t)K);
    ar.take(p.scal, 8);
    lay_out_sort(ar, &p, n, d, K);
    ar.take(p.closest, (size_t)S * n);
    ar.take(p.pot, (size_t)S);
    ar.take(p.P, (size_t)S * n);
    ar.take(p.segT, (size_t)S * nchunk);
    ar.take(p.segMax, (size_t)S * nchunk);
    ar.take(p.partial, (size_t)S * L * nchunk);
    ar.take(p.u, (size_t)S * (K > 1 ? K - 1 : 1) * L);
    ar.take(p.cand, (size_t)S * L);
    return p;
}

int check_common(const char *who, const float *X, int64_t n, int d, int K, void *ws, bool k_le_n = true) {
    GEO_REQUIRE(X, "%s: null X", who);
    GEO_REQUIRE(n >= 1 && n < ((int64_t)1 << 31) - CHUNK, "%s: n=%lld", who, (long long)n);
    GEO_REQUIRE(d >= 1 && d <= MAX_D, "%s: d=%d (1..%d)", who, d, MAX_D);
    GEO_REQUIRE(K >= 1 && K <= MAX_K && (!k_le_n || K <= n), "%s: K=%d (1..min(n, %d))", who, K, MAX_K);
    GEO_REQUIRE(ws && ((uintptr_t)ws) % 256 == 0, "%s: workspace null or not 256-byte aligned", who);
    return GEO_OK;
}

int launch_pack(const float *C, int K, int d, const Plan &p, bool gated, hipStream_t stream) {
    const int ns = ns_for(d), ntiles = (K + 31) / 32;
    km_pack_kernel<<<geo::grid_for((int64_t)ntiles * ns * 64, 256, 1024), 256, 0, stream>>>(C, K, d, ns, ntiles, p.Ap, p.cnp, p.st,
                                                                                           gated ? 1 : 0);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

int launch_assign(const float *X, int64_t n, int d, const float *C, int K, const Plan &p, int32_t *labels, double *keys,
                  int count_changes, int gated, hipStream_t stream) {
    const int ns = ns_for(d), ntiles = (K + 31) / 32;
    const unsigned grid = (unsigned)((n + 127) / 128);
#define KM_ASSIGN(NSV)                                                                                                  \
    case NSV:                                                                                                           \
        km_assign_kernel<NSV><<<grid, 256, 0, stream>>>(X, n, d, p.Ap, p.cnp, C, K, ntiles, labels, keys, count_changes, \
                                                        p.st, gated);                                                  \
        break;
    switch (ns) {
        KM_ASSIGN(1) KM_ASSIGN(2) KM_ASSIGN(4) KM_ASSIGN(8) KM_ASSIGN(16) KM_ASSIGN(32) KM_ASSIGN(64)
        default: geo::set_error("kmeans: d=%d", d); return GEO_E_ARG;
    }
#undef KM_ASSIGN
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

}  // namespace

extern "C" size_t geo_kmeans_workspace_bytes(int64_t n, int32_t d, int32_t K, int32_t n_starts, int32_t n_trials) {
    if (n < 1 || n >= ((int64_t)1 << 31) - CHUNK || d < 1 || d > MAX_D || K < 1 || K > MAX_K || n_starts < 1 || n_trials < 1 || n_trials > MAX_TRIALS) return 0;
    return geo::measure(lay_out, n, d, K, n_starts, n_trials);
}

extern "C" int geo_kmeans_assign(const float *X, int64_t n, int32_t d, const float *C, int32_t K, int32_t *labels_out,
                                 double *keys_out, int64_t *n_fallback_out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = check_common("geo_kmeans_assign", X, n, d, K, ws, false)) return e;
    GEO_REQUIRE(C && labels_out, "geo_kmeans_assign: null C or labels_out");
    geo::Arena ar(ws, ws_bytes);
    const Plan p = lay_out(ar, n, d, K, 1, 1);
    GEO_REQUIRE_WORKSPACE("geo_kmeans_assign", ar, ar.off);
    GEO_HIP_CHECK(hipMemsetAsync(p.st, 0, sizeof(Status), stream));
    if (int e = launch_pack(C, K, d, p, false, stream)) return e;
    if (int e = launch_assign(X, n, d, C, K, p, labels_out, keys_out, 0, 0, stream)) return e;
    if (n_fallback_out) {
        Status h;
        GEO_HIP_CHECK(hipMemcpyAsync(&h, p.st, sizeof(Status), hipMemcpyDeviceToHost, stream));
        GEO_HIP_CHECK(hipStreamSynchronize(stream));
        *n_fallback_out = (int64_t)h.n_fallback;
    }
    return GEO_OK;
}

extern "C" int geo_kmeans_pp(const float *X, int64_t n, int32_t d, int32_t K, int32_t n_starts, int32_t n_trials,
                             const int32_t *first_host, const double *u_host, int32_t *indices_out, float *centers_out,
                             void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = check_common("geo_kmeans_pp", X, n, d, K, ws)) return e;
    GEO_REQUIRE(n_starts >= 1 && n_starts <= 65535, "geo_kmeans_pp: n_starts=%d", n_starts);
    GEO_REQUIRE(n_trials >= 1 && n_trials <= MAX_TRIALS, "geo_kmeans_pp: n_trials=%d (1..%d)", n_trials, MAX_TRIALS);
    GEO_REQUIRE(first_host && indices_out && (K == 1 || u_host), "geo_kmeans_pp: null first, u or indices_out");
    const int S = n_starts, L = n_trials;
    for (int s = 0; s < S; ++s)
        GEO_REQUIRE(first_host[s] >= 0 && first_host[s] < n, "geo_kmeans_pp: first[%d]=%d", s, first_host[s]);
    geo::Arena ar(ws, ws_bytes);
    const Plan p = lay_out(ar, n, d, K, S, L);
    GEO_REQUIRE_WORKSPACE("geo_kmeans_pp", ar, ar.off);
    std::vector<int32_t> first((size_t)S * K, 0);
    for (int s = 0; s < S; ++s) first[(size_t)s * K] = first_host[s];
    GEO_HIP_CHECK(hipMemcpyAsync(indices_out, first.data(), first.size() * 4, hipMemcpyHostToDevice, stream));
    if (K > 1)
        GEO_HIP_CHECK(hipMemcpyAsync(p.u, u_host, (size_t)S * (K - 1) * L * 8, hipMemcpyHostToDevice, stream));
    GEO_HIP_CHECK(hipStreamSynchronize(stream));   // the host arrays may go away once this call returns
    const int nseg = (int)((n + CHUNK - 1) / CHUNK);
    const size_t search_lds = (size_t)(nseg + 1) * 8;
    GEO_REQUIRE(search_lds <= 56 * 1024, "geo_kmeans_pp: n=%lld too large for the segment table", (long long)n);
    for (int c = 1; c < K; ++c) {
        pp_update_scan_kernel<<<dim3(nseg, S), 256, 0, stream>>>(X, n, d, K, c, indices_out, p.closest, p.P, p.segT, p.segMax,
                                                                nseg);
        GEO_LAUNCH_CHECK();
        pp_search_kernel<<<S, 1024, search_lds, stream>>>(n, K, c, L, p.P, p.segT, p.segMax, nseg, p.u, p.pot, p.cand);
        GEO_LAUNCH_CHECK();
        pp_cand_kernel<<<dim3(nseg, S), 256, (size_t)L * d * 4, stream>>>(X, n, d, L, p.cand, p.closest, p.partial, nseg);
        GEO_LAUNCH_CHECK();
        pp_select_kernel<<<S, 1024, 0, stream>>>(K, c, L, p.cand, p.partial, nseg, p.pot, indices_out);
        GEO_LAUNCH_CHECK();
    }
    if (centers_out) {
        gather_rows_kernel<<<geo::grid_for((int64_t)S * K * d, 256, 4096), 256, 0, stream>>>(X, d, indices_out, (int64_t)S * K,
                                                                                            centers_out);
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}

extern "C" int geo_kmeans_lloyd(const float *X, int64_t n, int32_t d, int32_t K, int32_t n_starts, const float *init,
                                int32_t max_iter, double tol, float *centers_out, int32_t *labels_out, double *inertia_out,
                                int32_t *n_iter_out, int32_t *strict_out, int64_t *n_fallback_out, void *ws, size_t ws_bytes,
                                void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = check_common("geo_kmeans_lloyd", X, n, d, K, ws)) return e;
    GEO_REQUIRE(init && centers_out && labels_out && inertia_out && n_iter_out, "geo_kmeans_lloyd: null argument");
    GEO_REQUIRE(n_starts >= 1 && max_iter >= 1 && tol >= 0.0, "geo_kmeans_lloyd: n_starts=%d max_iter=%d tol=%g", n_starts,
                max_iter, tol);
    geo::Arena ar(ws, ws_bytes);
    const Plan p = lay_out(ar, n, d, K, 1, 1);
    GEO_REQUIRE_WORKSPACE("geo_kmeans_lloyd", ar, ar.off);
    const int64_t nchunk = (n + CHUNK - 1) / CHUNK;
    const size_t Kd = (size_t)K * d;
    int64_t fallback_total = 0;
    for (int s = 0; s < n_starts; ++s) {
        int32_t *lab = labels_out + (size_t)s * n;
        float *Cs[2] = {p.C0, p.C1};
        GEO_HIP_CHECK(hipMemsetAsync(p.st, 0, sizeof(Status), stream));
        GEO_HIP_CHECK(hipMemsetAsync(lab, 0xff, (size_t)n * 4, stream));   // labels_old = -1: the first iteration never converges
        GEO_HIP_CHECK(hipMemcpyAsync(p.C0, init + (size_t)s * Kd, Kd * 4, hipMemcpyDeviceToDevice, stream));
        Status h{};
        int launched = 0, batch = 4;
        while (true) {
            for (int b = 0; b < batch && launched < max_iter; ++b, ++launched) {
                const float *Cold = Cs[launched & 1];
                float *Cnew = Cs[(launched + 1) & 1];
                if (int e = launch_pack(Cold, K, d, p, true, stream)) return e;
                if (int e = launch_assign(X, n, d, Cold, K, p, lab, p.keys, 1, 1, stream)) return e;
                km_hist_kernel<<<(unsigned)nchunk, 256, (size_t)K * 4, stream>>>(lab, n, K, p.chunk_hist, p.st);
                km_colscan_kernel<<<(K + 63) / 64, 1024, 0, stream>>>(p.chunk_hist, (int)nchunk, K, p.counts, p.st);
                km_offsets_kernel<<<1, 1024, 0, stream>>>(p.counts, K, p.offs, p.st);
                km_scatter_kernel<<<(unsigned)nchunk, CHUNK, 0, stream>>>(lab, n, K, p.chunk_hist, p.offs, p.order, p.st);
                km_csum_kernel<<<K, 256, 0, stream>>>(X, d, p.order, p.offs, p.sums, p.st);
                km_relocate_kernel<<<1, 1024, 0, stream>>>(X, n, d, K, lab, p.keys, p.sums, p.counts, p.st);
                km_finalize_kernel<<<K, 128, 0, stream>>>(p.sums, p.counts, K, d, Cold, Cnew, p.shift2, p.st);
                km_status_kernel<<<1, 256, 0, stream>>>(p.shift2, K, tol, max_iter, p.st);
                GEO_LAUNCH_CHECK();
            }
            GEO_HIP_CHECK(hipMemcpyAsync(&h, p.st, sizeof(Status), hipMemcpyDeviceToHost, stream));
            GEO_HIP_CHECK(hipStreamSynchronize(stream));
            if (h.done) break;
            if (launched >= max_iter) {
                geo::set_error("geo_kmeans_lloyd: loop ended without a decision");
                return GEO_E_HIP;
            }
            batch = batch < 32 ? batch * 2 : 32;
        }
        const float *Cfin = Cs[h.n_iter & 1];
        if (!h.strict) {
            // relabel once with the final centres (sklearn's closing E-step)
            GEO_HIP_CHECK(hipMemsetAsync(&p.st->cmax_bits, 0, 4, stream));
            GEO_HIP_CHECK(hipMemsetAsync(&p.st->done, 0, 4, stream));
            if (int e = launch_pack(Cfin, K, d, p, false, stream)) return e;
            if (int e = launch_assign(X, n, d, Cfin, K, p, lab, nullptr, 0, 0, stream)) return e;
        }
        km_label_keys_kernel<<<geo::grid_for(n, 256, 4096), 256, 0, stream>>>(X, n, d, Cfin, lab, p.keys);
        km_sum_kernel<<<1, 1024, 0, stream>>>(p.keys, n, p.scal);
        GEO_LAUNCH_CHECK();
        GEO_HIP_CHECK(hipMemcpyAsync(centers_out + (size_t)s * Kd, Cfin, Kd * 4, hipMemcpyDeviceToDevice, stream));
        Status h2{};
        double inertia = 0.0;
        GEO_HIP_CHECK(hipMemcpyAsync(&inertia, p.scal, 8, hipMemcpyDeviceToHost, stream));
        GEO_HIP_CHECK(hipMemcpyAsync(&h2, p.st, sizeof(Status), hipMemcpyDeviceToHost, stream));
        GEO_HIP_CHECK(hipStreamSynchronize(stream));
        inertia_out[s] = inertia;
        n_iter_out[s] = h.n_iter;
        if (strict_out) strict_out[s] = h.strict;
        fallback_total += (int64_t)h2.n_fallback;
    }
    if (n_fallback_out) *n_fallback_out = fallback_total;
    return GEO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// EMA vector quantizer (VectorQuantizerEMA of the reference's baseline VQ-VAE, models/vqvae.py:53-115), DESIGN.md section 11.
// Same translation unit as the k-means kernels so that it launches their packing, screened assignment, counting sort and
// cluster sums unchanged.  z_e is NCHW (f32 or f16), rows are its (b, h, w) positions in that order, d = C.
//   forward   rows = f32(z_e) transposed; labels = geo_kmeans_assign's; z_q = embed[label] (pre-update); z_q_st =
//             fl32(z_e + fl32(z_q - z_e)); fp64 sums of (z_q_st - z_e)^2 and (z_q - z_e)^2 per fixed block range, summed in
//             a fixed order; counts; in training, the EMA update on the fp64 per-code sums in ascending row order (the
//             counting sort of k-means, then tile runs summed in ascending tile order: balanced when a few codes take most
//             rows, where k-means' one-block-per-cluster sum serialises).
//   backward  grad = g_st + fl32(fl32(g_loss beta) fl32(2 / numel)) (z_e - z_q_st), rounded once to z_e's dtype.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int VQ_OUT_BLOCKS = 1024;   // most blocks of the fused output kernel (its fixed partition of the elements)

// rows[(b HW + p) C + c] = f32(z[(b C + c) HW + p]) through a 32 x 32 LDS tile.  grid.x = B * ceil(HW / 32), grid.y = ceil(C / 32).
template <typename T>
__global__ __launch_bounds__(256) void vq_rows_kernel(const T *__restrict__ z, int C, int HW, int ptiles, float *__restrict__ rows) {
    __shared__ float tile[32][33];
    const int b = blockIdx.x / ptiles, p0 = (blockIdx.x % ptiles) * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int q = ty; q < 32; q += 8) {
        const int c = c0 + q, p = p0 + tx;
        if (c < C && p < HW) tile[q][tx] = (float)z[((int64_t)b * C + c) * HW + p];
    }
    __syncthreads();
    for (int q = ty; q < 32; q += 8) {
        const int p = p0 + q, c = c0 + tx;
        if (p < HW && c < C) rows[((int64_t)b * HW + p) * C + c] = tile[tx][q];
    }
}

// Sum of the block's per-thread values: butterfly inside each wave, then the four waves in ascending order (thread 0 returns it).
__device__ __forceinline__ double block_sum_256(double v, double *wsum) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// z_q, z_q_st (f32 NCHW), idx (i64) and per-block fp64 partials of (z_q_st - z_e)^2 and (z_q - z_e)^2.  Block blk covers the
// elements [blk per, (blk + 1) per), thread t the ones t, t + 256, ... ascending: the association depends on the shape alone.
template <typename T>
__global__ __launch_bounds__(256) void vq_out_kernel(const T *__restrict__ z, int C, int HW, int64_t total, int64_t per,
                                                     const int32_t *__restrict__ labels, const float *__restrict__ E,
                                                     float *__restrict__ zq_out, float *__restrict__ st_out,
                                                     int64_t *__restrict__ idx_out, int64_t n, double *__restrict__ partial) {
    __shared__ double wsum[2][4];
    const int64_t e0 = (int64_t)blockIdx.x * per, e1 = min(total, e0 + per);
    const int64_t chw = (int64_t)C * HW;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const int64_t b = e / chw, rem = e - b * chw;
        const int c = (int)(rem / HW), p = (int)(rem - (int64_t)c * HW);
        const float ze = (float)z[e];
        const float zq = E[(int64_t)labels[b * HW + p] * C + c];
        const float st = ze + (zq - ze);
        zq_out[e] = zq;
        st_out[e] = st;
        const double d1 = (double)st - (double)ze, d2 = (double)zq - (double)ze;
        a1 = fma(d1, d1, a1);
        a2 = fma(d2, d2, a2);
    }
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) idx_out[r] = labels[r];
    const double s1 = block_sum_256(a1, wsum[0]);
    const double s2 = block_sum_256(a2, wsum[1]);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s1;
        partial[2 * blockIdx.x + 1] = s2;
    }
}

// One block of 256: loss = fl32(fl32(beta) fl32(S1 / numel)); stats = (q_mse, perplexity, usage, dead) of the batch, from the
// partials (ascending per thread, then block_sum_256) and the counts (usage = used / K, p = count / max(n, 1), perplexity =
// exp(-sum p log(p + 1e-12)) in fp64).
__global__ __launch_bounds__(256) void vq_metrics_kernel(const double *__restrict__ partial, int nblk, int64_t numel,
                                                         const int32_t *__restrict__ counts, int K, int64_t n, float beta,
                                                         float *__restrict__ loss_out, float *__restrict__ stats_out) {
    __shared__ double wsum[4][4];
    double a1 = 0.0, a2 = 0.0, h = 0.0, used = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) { a1 += partial[2 * b]; a2 += partial[2 * b + 1]; }
    const double tot = (double)(n > 1 ? n : 1);
    for (int k = threadIdx.x; k < K; k += 256) {
        const double p = (double)counts[k] / tot;
        h += p * log(p + 1e-12);
        used += counts[k] > 0 ? 1.0 : 0.0;
    }
    const double s1 = block_sum_256(a1, wsum[0]);
    const double s2 = block_sum_256(a2, wsum[1]);
    const double sh = block_sum_256(h, wsum[2]);
    const double su = block_sum_256(used, wsum[3]);
    if (threadIdx.x == 0) {
        *loss_out = beta * (float)(s1 / (double)numel);
        const float usage = (float)(su / (double)K);
        stats_out[0] = (float)(s2 / (double)numel);
        stats_out[1] = (float)exp(-sh);
        stats_out[2] = usage;
        stats_out[3] = 1.f - usage;
    }
}

// Per-code fp64 sums over the rows sorted by code (order, offs from the counting sort), balanced for skewed codes: the sorted
// rows are cut into tiles of VQ_SEG positions; vq_seg_kernel sums each code's run inside a tile in ascending row order and
// stores it at the run's first position; vq_seg_sum_kernel adds a code's runs in ascending tile order.
constexpr int VQ_SEG = 64;

__global__ __launch_bounds__(128) void vq_seg_kernel(const float *__restrict__ X, int d, const int32_t *__restrict__ order,
                                                     const int32_t *__restrict__ labels, int64_t n, double *__restrict__ seg) {
    const int c = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * VQ_SEG, p1 = min(n, p0 + VQ_SEG);
    if (c >= d || p0 >= n) return;
    double a = 0.0;
    int64_t start = p0;
    int32_t cur = labels[order[p0]];
    for (int64_t pos = p0; pos < p1; ++pos) {
        const int32_t r = order[pos];
        const int32_t lab = labels[r];
        if (lab != cur) {
            seg[start * d + c] = a;
            a = 0.0;
            start = pos;
            cur = lab;
        }
        a += (double)X[(int64_t)r * d + c];
    }
    seg[start * d + c] = a;
}

__global__ __launch_bounds__(128) void vq_seg_sum_kernel(const double *__restrict__ seg, const int32_t *__restrict__ offs, int d,
                                                         double *__restrict__ sums) {
    const int k = blockIdx.x, c = threadIdx.x;
    if (c >= d) return;
    const int64_t m0 = offs[k], m1 = offs[k + 1];
    double s = 0.0;
    if (m1 > m0) {
        const int64_t t0 = m0 / VQ_SEG, t1 = (m1 - 1) / VQ_SEG;
#pragma unroll 8
        for (int64_t t = t0; t <= t1; ++t) s += seg[max(m0, t * VQ_SEG) * d + c];
    }
    sums[(size_t)k * d + c] = s;
}

// EMA cluster sizes, one block of 1024: cs = fma(count, 1 - decay, fl32(cs decay)) in place; n = fl32(fp64 sum of the new cs,
// ascending per thread then over the threads); norm[k] = max(fl32(fl32(fl32(cs + eps) / fl32(n + K eps)) n), eps).
__global__ __launch_bounds__(1024) void vq_ema_size_kernel(float *__restrict__ cluster_size, const int32_t *__restrict__ counts,
                                                           int K, float decay, float omd, float eps, float keps,
                                                           float *__restrict__ norm) {
    __shared__ double tsum[1024];
    __shared__ float n_sh;
    double a = 0.0;
    for (int k = threadIdx.x; k < K; k += 1024) {
        const float cs = fmaf((float)counts[k], omd, cluster_size[k] * decay);
        cluster_size[k] = cs;
        a += (double)cs;
    }
    tsum[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < 1024; ++t) s += tsum[t];
        n_sh = (float)s;
    }
    __syncthreads();
    const float n = n_sh, denom = n + keps;
    for (int k = threadIdx.x; k < K; k += 1024) norm[k] = fmaxf(((cluster_size[k] + eps) / denom) * n, eps);
}

// EMA embedding, one block per code: embed_avg = fma(f32(sum), 1 - decay, fl32(embed_avg decay)); embed = clamp(nan_to_num(
// embed_avg / norm, nan 0, +inf 1, -inf -1), -2, 2).
__global__ __launch_bounds__(128) void vq_ema_embed_kernel(const double *__restrict__ sums, const float *__restrict__ norm, int d,
                                                           float decay, float omd, float *__restrict__ embed_avg,
                                                           float *__restrict__ embed) {
    const int k = blockIdx.x;
    const float nk = norm[k];
    for (int c = threadIdx.x; c < d; c += 128) {
        const size_t i = (size_t)k * d + c;
        const float ea = fmaf((float)sums[i], omd, embed_avg[i] * decay);
        embed_avg[i] = ea;
        float v = ea / nk;
        if (isnan(v)) v = 0.f;
        else if (isinf(v)) v = v > 0.f ? 1.f : -1.f;
        embed[i] = fminf(fmaxf(v, -2.f), 2.f);
    }
}

// grad = cast(g_st + coef (z_e - z_q_st)), coef = fl32(fl32(g_loss beta) fl32(2 / numel)); null g_st / g_loss count as zero.
template <typename T>
__global__ __launch_bounds__(256) void vq_backward_kernel(const float *__restrict__ g_st, const float *__restrict__ g_loss, float beta,
                                                          float two_over_n, const T *__restrict__ z, const float *__restrict__ st,
                                                          int64_t numel, T *__restrict__ grad) {
    const float coef = g_loss ? (*g_loss * beta) * two_over_n : 0.f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < numel; e += (int64_t)gridDim.x * 256) {
        const float g = g_st ? g_st[e] : 0.f;
        grad[e] = (T)(g + coef * ((float)z[e] - st[e]));
    }
}

struct VqPlan {
    Plan km;
    float *rows, *norm;
    int32_t *labels;
    double *partial, *seg;
};

// Of k-means only what the quantizer's launches touch (lay_out_assign, lay_out_sort), then its own buffers.
VqPlan vq_lay_out(geo::Arena &ar, int64_t n, int d, int K) {
    VqPlan v{};
    lay_out_assign(ar, &v.km, d, K);
    lay_out_sort(ar, &v.km, n, d, K);
    ar.take(v.rows, (size_t)n * d);
    ar.take(v.labels, (size_t)n);
    ar.take(v.partial, (size_t)VQ_OUT_BLOCKS * 2);
    ar.take(v.norm, (size_t)K);
    ar.take(v.seg, (size_t)n * d);
    return v;
}

int vq_check(const char *who, int64_t B, int C, int64_t HW, int K) {
    GEO_REQUIRE(B >= 1 && HW >= 1 && B * HW < ((int64_t)1 << 31) - CHUNK, "%s: B=%lld HW=%lld", who, (long long)B, (long long)HW);
    GEO_REQUIRE(C >= 1 && C <= MAX_D, "%s: C=%d (1..%d)", who, C, MAX_D);
    GEO_REQUIRE(K >= 1 && K <= MAX_K, "%s: K=%d (1..%d)", who, K, MAX_K);
    return GEO_OK;
}

}  // namespace

extern "C" size_t geo_vq_workspace_bytes(int64_t n, int32_t d, int32_t K) {
    if (n < 1 || n >= ((int64_t)1 << 31) - CHUNK || d < 1 || d > MAX_D || K < 1 || K > MAX_K) return 0;
    return geo::measure(vq_lay_out, n, d, K);
}

extern "C" int geo_vq_forward(const void *z_e, int32_t half, int32_t B, int32_t C, int32_t HW, float *embed, float *cluster_size,
                              float *embed_avg, int32_t K, int32_t training, double decay, double eps, double beta, float *z_q_out,
                              float *z_q_st_out, int64_t *idx_out, float *loss_out, float *stats_out, int32_t *counts_out,
                              void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int e = vq_check("geo_vq_forward", B, C, HW, K)) return e;
    GEO_REQUIRE(z_e && embed && z_q_out && z_q_st_out && idx_out && loss_out && stats_out, "geo_vq_forward: null argument");
    GEO_REQUIRE(!training || (cluster_size && embed_avg), "geo_vq_forward: training needs cluster_size and embed_avg");
    GEO_REQUIRE(ws && ((uintptr_t)ws) % 256 == 0, "geo_vq_forward: workspace null or not 256-byte aligned");
    const int64_t n = (int64_t)B * HW, total = n * C;
    geo::Arena ar(ws, ws_bytes);
    const VqPlan v = vq_lay_out(ar, n, C, K);
    GEO_REQUIRE_WORKSPACE("geo_vq_forward", ar, ar.off);
    const Plan &p = v.km;
    GEO_HIP_CHECK(hipMemsetAsync(p.st, 0, sizeof(Status), stream));
    const int ptiles = (HW + 31) / 32;
    const dim3 rgrid((unsigned)(B * ptiles), (unsigned)((C + 31) / 32));
    if (half) vq_rows_kernel<_Float16><<<rgrid, 256, 0, stream>>>(static_cast<const _Float16 *>(z_e), C, HW, ptiles, v.rows);
    else vq_rows_kernel<float><<<rgrid, 256, 0, stream>>>(static_cast<const float *>(z_e), C, HW, ptiles, v.rows);
    GEO_LAUNCH_CHECK();
    if (int e = launch_pack(embed, K, C, p, false, stream)) return e;
    if (int e = launch_assign(v.rows, n, C, embed, K, p, v.labels, nullptr, 0, 0, stream)) return e;
    const int nblk = (int)std::min<int64_t>(VQ_OUT_BLOCKS, (total + 2047) / 2048);
    const int64_t per = (total + nblk - 1) / nblk;
    if (half)
        vq_out_kernel<_Float16><<<nblk, 256, 0, stream>>>(static_cast<const _Float16 *>(z_e), C, HW, total, per, v.labels, embed,
                                                          z_q_out, z_q_st_out, idx_out, n, v.partial);
    else
        vq_out_kernel<float><<<nblk, 256, 0, stream>>>(static_cast<const float *>(z_e), C, HW, total, per, v.labels, embed, z_q_out,
                                                       z_q_st_out, idx_out, n, v.partial);
    GEO_LAUNCH_CHECK();
    const int64_t nchunk = (n + CHUNK - 1) / CHUNK;
    km_hist_kernel<<<(unsigned)nchunk, 256, (size_t)K * 4, stream>>>(v.labels, n, K, p.chunk_hist, p.st);
    km_colscan_kernel<<<(K + 63) / 64, 1024, 0, stream>>>(p.chunk_hist, (int)nchunk, K, p.counts, p.st);
    GEO_LAUNCH_CHECK();
    if (training) {
        const float decay_f = (float)decay, omd = (float)(1.0 - decay), eps_f = (float)eps, keps = (float)((double)K * eps);
        km_offsets_kernel<<<1, 1024, 0, stream>>>(p.counts, K, p.offs, p.st);
        km_scatter_kernel<<<(unsigned)nchunk, CHUNK, 0, stream>>>(v.labels, n, K, p.chunk_hist, p.offs, p.order, p.st);
        vq_seg_kernel<<<(unsigned)((n + VQ_SEG - 1) / VQ_SEG), 128, 0, stream>>>(v.rows, C, p.order, v.labels, n, v.seg);
        vq_seg_sum_kernel<<<K, 128, 0, stream>>>(v.seg, p.offs, C, p.sums);
        vq_ema_size_kernel<<<1, 1024, 0, stream>>>(cluster_size, p.counts, K, decay_f, omd, eps_f, keps, v.norm);
        vq_ema_embed_kernel<<<K, 128, 0, stream>>>(p.sums, v.norm, C, decay_f, omd, embed_avg, embed);
        GEO_LAUNCH_CHECK();
    }
    vq_metrics_kernel<<<1, 256, 0, stream>>>(v.partial, nblk, total, p.counts, K, n, (float)beta, loss_out, stats_out);
    GEO_LAUNCH_CHECK();
    if (counts_out) GEO_HIP_CHECK(hipMemcpyAsync(counts_out, p.counts, (size_t)K * 4, hipMemcpyDeviceToDevice, stream));
    return GEO_OK;
}

extern "C" int geo_vq_backward(const float *g_st, const float *g_loss, double beta, const void *z_e, int32_t half,
                               const float *z_q_st, int64_t numel, void *grad_out, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(z_e && z_q_st && grad_out && numel >= 1, "geo_vq_backward: null argument or numel=%lld", (long long)numel);
    const float two_over_n = (float)(2.0 / (double)numel);
    const int grid = geo::grid_for(numel, 256, 8192);
    if (half)
        vq_backward_kernel<_Float16><<<grid, 256, 0, stream>>>(g_st, g_loss, (float)beta, two_over_n,
                                                               static_cast<const _Float16 *>(z_e), z_q_st, numel,
                                                               static_cast<_Float16 *>(grad_out));
    else
        vq_backward_kernel<float><<<grid, 256, 0, stream>>>(g_st, g_loss, (float)beta, two_over_n, static_cast<const float *>(z_e),
                                                            z_q_st, numel, static_cast<float *>(grad_out));
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}
