// knn.hip -- exact fp64-ranked k-nearest-neighbour search (gfx950).
//
// Replaces sklearn NearestNeighbors(...).kneighbors as called from the reference's
// src/geo/knn_graph_optimized.py:40-42.  The ranking key is the fp64 squared distance, formed
// either by the expansion |x|^2 - 2 x.y + |y|^2 clamped at 0 (sklearn's brute-force path,
// _argkmin.pyx.tp:492-502, used for d > 15) or directly as sum (x-y)^2 (kd-tree path, d <= 15);
// both are fma chains over the dimensions in ascending order, ties are ordered by index.
//
// THE KEY is stated once, in f32x4_to_f64 / key_chain / key_close below: the candidate's float32 coordinates converted to fp64,
// the chain over the zero-padded dimensions a chunk at a time, the expansion form closed by (n_a + (-2 acc)) + n_b and clamped
// at 0, the direct form its chain.  Every search kernel of this file (knn_kernel, knn_bound_kernel, knn_refine_kernel,
// nearest_foreign_kernel) forms its keys with these three and differs only in its schedule around them; a new one does the same.
// (One exception, with its reason where it stands: nearest_foreign_kernel writes the closing out around its branch on the order of
// the two norms.)
//
// Mapping: one wave owns Q query rows; every lane owns ONE candidate row per step (64 candidates
// per step, coordinates converted f32->f64 once and reused for the Q queries).  Query coordinates
// are wave-uniform and stream through the scalar cache (fp64 copy in the workspace), so the
// inner loop is v_fma_f64 with one SGPR-pair operand -- no LDS traffic.  The k best of a query
// live one per lane (lane i = i-th smallest), so a hit is inserted with one ballot, one popcount
// and a one-lane shift of the whole wave: no per-lane divergence.  Hits are rare after the first
// steps (k * ln(N/k) per query), the loop is bound by the fp64 FMA rate.
#include "geo_common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

constexpr int KNN_WAVES = 4;

__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Four float32 coordinates of a candidate row (one 16-byte load, issued by the caller on its own schedule) as fp64.  A row chunk
// is DCH / 4 of these, looped over in the caller: a chunk-wide helper with the loop inside is unrolled on its own before it is
// inlined, and the kernels then allocate differently (knn_bound_kernel<16, 8, 2, true> 108 -> 114 VGPRs, knn_kernel<8, 4, false, 1>
// 54 -> 101 with SGPRs spilled to lanes); this way they compile to the instructions they had with the conversion written out.
__device__ __forceinline__ void f32x4_to_f64(const float4 &f, double *c) {
    c[0] = (double)f.x; c[1] = (double)f.y; c[2] = (double)f.z; c[3] = (double)f.w;
}

// the chain over DCH consecutive dimensions: qv = the query's fp64 coordinates there (a wave-uniform address in every caller)
template <int DCH, bool EXPANSION>
__device__ __forceinline__ double key_chain(const double *qv, const double (&cj)[DCH], double acc) {
#pragma unroll
    for (int k = 0; k < DCH; ++k) {
        if (EXPANSION) {
            acc = fma(qv[k], cj[k], acc);
        } else {
            const double t = qv[k] - cj[k];
            acc = fma(t, t, acc);
        }
    }
    return acc;
}

// the finished chain -> the key.  Expansion form: the two squared norms in the caller's order (sklearn adds the query's first;
// the sum is not symmetric in them), clamped at 0 -- a norm of +inf added last stays +inf.  Direct form: the chain itself.
template <bool EXPANSION>
__device__ __forceinline__ double key_close(double acc, double n_first, double n_last) {
    if (!EXPANSION) return acc;
    double d2 = (n_first + (-2.0 * acc)) + n_last;
    if (!(d2 > 0.0)) d2 = 0.0;
    return d2;
}

// zp32 [n][dp] f32 zero padded, zq64 [n][dp] f64 zero padded, nrm [n] fp64 fma-chain squared norms
__global__ __launch_bounds__(256) void knn_prep_kernel(const float *__restrict__ z, int64_t n, int d, int dp,
                                                      float *__restrict__ zp32, double *__restrict__ zq64,
                                                      double *__restrict__ nrm) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int c = 0; c < dp; ++c) {
            const float x = c < d ? z[i * d + c] : 0.0f;
            zp32[i * dp + c] = x;
            zq64[i * dp + c] = (double)x;
            s = fma((double)x, (double)x, s);
        }
        nrm[i] = s;
    }
}

template <int DCH, int Q, bool EXPANSION, int LR = 1>
__global__ __launch_bounds__(256) void knn_kernel(const float *__restrict__ zp32, const double *__restrict__ zq64,
                                                 const double *__restrict__ nrm, const double *__restrict__ nrm_q,
                                                 int64_t n, int nch, int kq, int64_t row0, int64_t row1,
                                                 int32_t *__restrict__ idx_out, double *__restrict__ d2_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = row0 + ((int64_t)blockIdx.x * KNN_WAVES + wave) * Q;
    if (q0 >= row1) return;
    const int dp = nch * DCH;

    // list position p = 64 r + lane holds the p-th smallest squared distance seen so far for query q (LR registers
    // per lane: lists of up to 64 LR entries) and its corpus index
    double lv[Q][LR];
    int32_t li[Q][LR];
    double tau[Q];     // wave-uniform: current kq-th smallest
    const int tau_reg = (kq - 1) >> 6, tau_lane = (kq - 1) & 63;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        tau[q] = inf64();
#pragma unroll
        for (int r = 0; r < LR; ++r) { lv[q][r] = inf64(); li[q][r] = -1; }
    }

    for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const int64_t j = c0 + lane;
        const bool valid = j < n;
        const int64_t jc = valid ? j : n - 1;
        double acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = 0.0;
        for (int ch = 0; ch < nch; ++ch) {
            double cj[DCH];
            const float4 *src = reinterpret_cast<const float4 *>(zp32 + jc * dp + ch * DCH);
#pragma unroll
            for (int v = 0; v < DCH / 4; ++v) f32x4_to_f64(src[v], cj + 4 * v);
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                int64_t qr = q0 + q;
                if (qr >= row1) qr = row1 - 1;
                acc[q] = key_chain<DCH, EXPANSION>(zq64 + qr * dp + ch * DCH, cj, acc[q]);
            }
        }
        const double nj = EXPANSION ? nrm[jc] : 0.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            int64_t qr = q0 + q;
            if (qr >= row1) qr = row1 - 1;
            const double d2 = key_close<EXPANSION>(acc[q], EXPANSION ? nrm_q[qr] : 0.0, nj);
            unsigned long long hits = __ballot(valid && d2 < tau[q]);
            while (hits) {
                const int src_lane = __builtin_ctzll(hits);
                hits &= hits - 1;
                const double val = readlane_f64(d2, src_lane);
                if (!(val < tau[q])) continue;             // tau shrank since the ballot
                const int32_t id = (int32_t)(c0 + src_lane);
                // stable insertion behind equal keys: candidates arrive in ascending index order
                int pos = 0;
#pragma unroll
                for (int r = 0; r < LR; ++r) pos += __builtin_popcountll(__ballot(lv[q][r] <= val));
#pragma unroll
                for (int r = LR - 1; r >= 0; --r) {            // top register first: it takes lane 63 of the one below
                    double up_v = __shfl_up(lv[q][r], 1, 64);
                    int32_t up_i = __shfl_up(li[q][r], 1, 64);
                    if (r > 0) {
                        const double carry_v = readlane_f64(lv[q][r - 1], 63);
                        const int32_t carry_i = __builtin_amdgcn_readlane(li[q][r - 1], 63);
                        if (lane == 0) { up_v = carry_v; up_i = carry_i; }
                    }
                    const int g = 64 * r + lane;
                    if (g > pos) { lv[q][r] = up_v; li[q][r] = up_i; }
                    if (g == pos) { lv[q][r] = val; li[q][r] = id; }
                }
#pragma unroll
                for (int r = 0; r < LR; ++r)
                    if (r == tau_reg) tau[q] = readlane_f64(lv[q][r], tau_lane);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int64_t qr = q0 + q;
#pragma unroll
        for (int r = 0; r < LR; ++r) {
            const int g = 64 * r + lane;
            if (qr < row1 && g < kq) {
                idx_out[(qr - row0) * kq + g] = li[q][r];
                d2_out[(qr - row0) * kq + g] = lv[q][r];
            }
        }
    }
}

// ---- exact search behind a float32 matrix-core filter (large corpora) -----------------------------------------------
// 1. tau[i] = an upper bound of the kq-th smallest exact distance from query i to every S-th corpus row, itself an upper
//    bound of the kq-th smallest over the whole corpus (knn_bound_kernel on the subset; the two-level path tightens it to the
//    subset's exact kq-th distance).  S = filter_stride(kq) (FILTER_STRIDE for short lists).
// 2. knn_scan_kernel: approximate squared distances of ALL pairs on the matrix cores (v_mfma_f32_32x32x2_f32, expansion
//    form with the fp64 norms); pair (i, j) is kept when  approx <= tau[i] + eps * (|x_i|^2 + |x_j|^2),  eps far above
//    the rounding of a d-term float32 dot product -- every true neighbour is kept, plus ~S * kq others.
// 3. knn_refine_kernel: the kept candidates are re-evaluated with the fp64 key and ranked
//    by (distance, index): the result is the one knn_kernel gives.  A query whose list overflows FILTER_CAP (heavily
//    duplicated points) is reported and the caller falls back to knn_kernel.
constexpr int FILTER_STRIDE = 8, FILTER_STRIDE_MIN = 4, FILTER_CAP = 1024;
// A query keeps ~S * kq candidates on average (about S kq corpus rows lie at or below the kq-th distance to every S-th row),
// with a tail of a few hundred more: at S = 16 and kq = 64 the mean was the cap itself, half the queries overflowed and the
// whole call fell back to the exact scan.  Denser subsets for longer lists keep S * kq <= 384 (kq <= 64 here).
// Short lists took S = 16 while the thresholds were an exact ranking of the subset (1.0 ms at 60 000 x 16, kq = 21).  With
// knn_bound_kernel they cost 0.32 ms at S = 16, 0.57 at 8 and 1.08 at 4, and the candidates -- the scan's slow path and the
// refinement -- shrink with S: thresholds + scan + refinement per build 1.88 / 1.62 / 1.91 ms at S = 16 / 8 / 4 (five builds
// each, spread 0.06), and 136.3 / 134.6 / 179.7 ms at one million rows (two levels: every 64th row at S = 8).  Hence 8.
constexpr int filter_stride(int kq) { return kq <= 40 ? FILTER_STRIDE : FILTER_STRIDE_MIN; }
constexpr int64_t TWO_LEVEL_MIN = 200000;      // from here on the thresholds themselves come from a filtered pass (below)
typedef float f32x16v __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void knn_subset_kernel(const float *__restrict__ zp32, const double *__restrict__ nrm,
                                                        int64_t n, int dp, int stride, int64_t m,
                                                        float *__restrict__ zs32, double *__restrict__ nrm_s) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m * dp; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / dp;
        const int c = (int)(i % dp);
        zs32[i] = zp32[r * stride * dp + c];
        if (c == 0) nrm_s[r] = nrm[r * stride];
    }
}

// ---- what the scans compare, stated once: pair (i, j) is kept when  |x_j|^2 (1 - eps) - 2 x_i.x_j <= u[i]  with
// u[i] = tau[i] - |x_i|^2 (1 - eps).  In float32 u is rounded UP and the norm column DOWN, so rounding only ever keeps more.
__device__ __forceinline__ double scan_threshold(double tau, double nq, double eps) { return tau + eps * nq - nq; }

__device__ __forceinline__ float f32_round_up(double x) {
    float r = (float)x;
    if ((double)r < x) r = nextafterf(r, 3.4e38f);
    return r;
}

__device__ __forceinline__ float f32_round_down(double x) {
    float r = (float)x;
    if ((double)r > x) r = nextafterf(r, -3.4e38f);
    return r;
}

// |x_j|^2 (1 - eps) of the norm column
__device__ __forceinline__ float scan_norm(double nrm, double eps) { return f32_round_down(nrm * (1.0 - eps)); }

// the corpus tiles [lo, hi) of SCAN_CT candidates that slice `split` of `splits` scans (empty when lo >= hi)
struct TileRange { int64_t lo, hi; };
__device__ __forceinline__ TileRange split_tiles(int64_t n, int scan_ct, int splits, int split) {
    const int64_t all_tiles = (n + scan_ct - 1) / scan_ct, per_split = (all_tiles + splits - 1) / splits;
    const int64_t lo = per_split * split;
    return {lo, lo + per_split < all_tiles ? lo + per_split : all_tiles};
}

// ---- the kept-pair queue of the scans.  Kept pairs go to a per-wave LDS queue first (the returning global atomic that reserves
// a list slot costs microseconds, too much inside the MFMA stream; the queue is flushed at tile ends).  A lane holds the pairs it
// keeps as set bits of one word (each scan packs its own); lanes take their set bits one per round and get queue positions from
// the round's ballot: no LDS atomics, a handful of branches per tile with something to keep.
constexpr int EQ_CAP = 128;
struct KeptQueue {
    unsigned long long *eb;            // this wave's EQ_CAP entries in LDS: (local query row << 32) | candidate
    int32_t *cnt, *list;               // [rows], [rows][FILTER_CAP]
    int qn;                            // pairs queued by this wave (wave-uniform)

    __device__ __forceinline__ void to_list(int32_t row, int32_t cand) const {
        const int32_t slot = atomicAdd(&cnt[row], 1);
        if (slot < FILTER_CAP) list[(int64_t)row * FILTER_CAP + slot] = cand;
    }
    __device__ __forceinline__ void flush(int lane) {           // wave-uniform call
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const int m = qn < EQ_CAP ? qn : EQ_CAP;
        for (int i = lane; i < m; i += 64) {
            const unsigned long long e = eb[i];
            to_list((int32_t)(e >> 32), (int32_t)(e & 0xffffffffu));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        qn = 0;
    }
    // pair_of(b) = the (row, candidate) of this lane's bit b
    template <class PairOf>
    __device__ __forceinline__ void take(unsigned bits, PairOf pair_of) {
        for (;;) {
            const unsigned long long hit = __ballot(bits != 0);
            if (!hit) break;
            if (bits != 0) {
                const int b = __builtin_ctz(bits);
                bits &= bits - 1;
                const int pos = qn + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hit >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hit, 0u));
                const int2 rc = pair_of(b);
                if (pos < EQ_CAP) eb[pos] = ((unsigned long long)(unsigned)rc.x << 32) | (unsigned)rc.y;
                else to_list(rc.x, rc.y);                     // queue full (masses of duplicates): straight to the list
            }
            qn += __builtin_popcountll(hit);
        }
    }
};

// the two-level path's thresholds: tau from the kq-th entry of the refined subset lists (knn_bound_kernel writes u itself)
__global__ __launch_bounds__(256) void knn_tau_kernel(const double *__restrict__ d2_sub, const double *__restrict__ nrm,
                                                     int64_t row0, int64_t rows, int kq, double eps,
                                                     double *__restrict__ u, int32_t *__restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        u[i] = scan_threshold(d2_sub[i * kq + (kq - 1)], nrm[row0 + i], eps);
        cnt[i] = 0;
    }
}

// ---- thresholds of the filter: a bound from per-lane minima, not a ranking -----------------------------------------------
// The filter needs tau[i] >= the kq-th smallest key of query i over the corpus and nothing more: the refinement re-evaluates
// every kept pair and ranks it, so the lists are exact under any valid bound.  Ranking the subset exactly (knn_kernel: a sorted
// list, one ballot + popcount + whole-wave shift per hit, ~120 serial insertions per query on a 3 750-row subset) cost as much
// as the scan of all pairs.  Here subset row p belongs to lane p % 64, and a lane keeps the TWO smallest keys it has seen per
// query: two fmin and one fmax per key, no ballots, no indices.  The 128 per-lane values of a query are keys of 128 distinct
// subset rows (of all m rows when m <= 128, +inf in the empty slots), so their kq-th smallest (kq <= 64, kq <= m) has at least kq
// corpus rows at or below it.  It is the exact subset threshold unless three of the kq best share a lane: 1.5 % more
// candidates than the exact one at (kq, S) = (21, 16), 5 % at (40, 8), 14 % at (64, 4) (20 000 normal rows, d = 16); one
// minimum per lane loses 20 % - 5x.  Lists longer than 24 keep THREE per lane (192 values, 0.6 % and 2 % more candidates).
//
// One workgroup owns Q queries; its four waves take the subset's 64-row steps round robin (query coordinates wave-uniform
// through the scalar cache, the next step's row in flight under the fmas),
// leave their minima in LDS, and each wave then merges and selects for Q / 4 of the queries.  30 000 waves of 15 steps at
// 60 000 queries x 3 750 rows where knn_kernel<.., 16> had 3 750 of 59, and a rank's share of the rows still fills the chip.
constexpr int BOUND_Q = 8;
constexpr int bound_minima(int kq) { return kq <= 24 ? 2 : 3; }

// v[0] <= v[1] <= .. stay the NM smallest of themselves and x
template <int NM>
__device__ __forceinline__ void keep_smallest(double (&v)[NM], double x) {
#pragma unroll
    for (int r = NM - 1; r > 0; --r) v[r] = fmin(v[r], fmax(v[r - 1], x));
    v[0] = fmin(v[0], x);
}

// the kq-th smallest (1 <= kq <= 64 NM) of the wave's 64 NM values (keys >= 0 or +inf): quickselect in registers -- a pivot
// from inside the window (lo, hi) (fewer than kq values <= lo, at least kq <= hi), NM ballots to count, ~10 rounds
template <int NM>
__device__ __forceinline__ double kth_of_wave(const double (&v)[NM], int kq) {
    double lo = -1.0, hi = inf64();
    int rot = 0;
    for (int guard = 0; guard < 64 * NM + 2; ++guard) {       // every round takes its pivot out of the window
        double cand = inf64();                                 // this lane's first value strictly inside the window
#pragma unroll
        for (int r = NM - 1; r >= 0; --r)
            if (v[r] > lo && v[r] < hi) cand = v[r];
        unsigned long long has = __ballot(cand < inf64());
        if (!has) break;                                       // nothing strictly inside: the answer is hi
        has = (has >> rot) | (rot ? has << (64 - rot) : 0ull);
        const int src = (__builtin_ctzll(has) + rot) & 63;
        rot = (rot + 23) & 63;
        const double pivot = readlane_f64(cand, src);
        int c = 0;
#pragma unroll
        for (int r = 0; r < NM; ++r) c += __builtin_popcountll(__ballot(v[r] <= pivot));
        if (c >= kq) hi = pivot; else lo = pivot;
    }
    return hi;
}

// u[i] = tau[i] - |x_i|^2 (1 - eps) and cnt[i] = 0 for the scan (when u is given), tau[i] itself when tau_out is given
template <int DCH, int Q, int NM, bool EXPANSION>
__global__ __launch_bounds__(256) void knn_bound_kernel(const float *__restrict__ zs32, const double *__restrict__ zq64,
                                                       const double *__restrict__ nrm_s, const double *__restrict__ nrm_q,
                                                       int64_t m, int nch, int kq, int64_t row0, int64_t row1, double eps,
                                                       double *__restrict__ u, int32_t *__restrict__ cnt,
                                                       double *__restrict__ tau_out) {
    static_assert(Q % KNN_WAVES == 0, "every wave selects for Q / KNN_WAVES queries");
    __shared__ double mins[KNN_WAVES][Q][NM][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = row0 + (int64_t)blockIdx.x * Q;
    const int dp = nch * DCH;
    const int64_t steps = (m + 63) / 64;
    double mn[Q][NM];                                          // this lane's NM smallest keys per query, ascending
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int r = 0; r < NM; ++r) mn[q][r] = inf64();

    double nq[Q];                                              // wave-uniform
#pragma unroll
    for (int q = 0; q < Q; ++q) nq[q] = EXPANSION ? nrm_q[q0 + q < row1 ? q0 + q : row1 - 1] : 0.0;

    float4 f[DCH / 4];                                         // the row chunk in flight
    // A lane past the subset's end must not enter the minima: its key is made +inf by the arithmetic itself, with no select
    // per query -- the expansion form adds a norm of +inf last (the clamp keeps +inf), the direct form starts its sum at +inf.
    double nj_next = 0.0;
    auto fetch = [&](int64_t s, int ch) {
        const int64_t j = s * 64 + lane;
        const int64_t jc = j < m ? j : m - 1;
        const float4 *src = reinterpret_cast<const float4 *>(zs32 + jc * dp + ch * DCH);
#pragma unroll
        for (int v = 0; v < DCH / 4; ++v) f[v] = src[v];
        if (ch == 0) nj_next = j < m ? (EXPANSION ? nrm_s[jc] : 0.0) : inf64();
    };
    double acc[Q];
    double nj = 0.0;
    int64_t s = wave;
    int ch = 0;
    if (s < steps) fetch(s, 0);
    while (s < steps) {
        double cj[DCH];
#pragma unroll
        for (int v = 0; v < DCH / 4; ++v) f32x4_to_f64(f[v], cj + 4 * v);
        if (ch == 0) {
            nj = nj_next;
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[q] = EXPANSION ? 0.0 : nj;
        }
        int64_t s_n = s;
        int ch_n = ch + 1;
        if (ch_n == nch) { ch_n = 0; s_n = s + KNN_WAVES; }
        if (s_n < steps) fetch(s_n, ch_n);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            int64_t qr = q0 + q;
            if (qr >= row1) qr = row1 - 1;
            acc[q] = key_chain<DCH, EXPANSION>(zq64 + qr * dp + ch * DCH, cj, acc[q]);
        }
        if (ch == nch - 1) {
#pragma unroll
            for (int q = 0; q < Q; ++q) keep_smallest<NM>(mn[q], key_close<EXPANSION>(acc[q], nq[q], nj));
        }
        s = s_n;
        ch = ch_n;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int r = 0; r < NM; ++r) mins[wave][q][r][lane] = mn[q][r];
    __syncthreads();
    // the waves' sets merge elementwise (a lane's rows are its own in every wave): the NM smallest of the four sets
    for (int t = 0; t < Q / KNN_WAVES; ++t) {
        const int q = wave * (Q / KNN_WAVES) + t;
        const int64_t qr = q0 + q;
        if (qr >= row1) break;
        double a[NM];
#pragma unroll
        for (int r = 0; r < NM; ++r) a[r] = mins[0][q][r][lane];
#pragma unroll
        for (int w = 1; w < KNN_WAVES; ++w)
#pragma unroll
            for (int r = 0; r < NM; ++r) keep_smallest<NM>(a, mins[w][q][r][lane]);
        const double tau = kth_of_wave<NM>(a, kq);
        if (lane == 0) {
            if (u) {
                u[qr - row0] = scan_threshold(tau, nrm_q[qr], eps);
                cnt[qr - row0] = 0;
            }
            if (tau_out) tau_out[qr - row0] = tau;
        }
    }
}

template <int DP, int SCAN_CT>
__global__ __launch_bounds__(256) void knn_scan_kernel(const float *__restrict__ zp32, const double *__restrict__ nrm,
                                                      const double *__restrict__ u, int64_t n, int64_t row0, int64_t rows,
                                                      double eps, int splits, int32_t *__restrict__ cnt,
                                                      int32_t *__restrict__ list) {
    // The whole test runs on the matrix cores: with A = [-2 x_i, 1, -u_i] and B = [x_j, |x_j|^2 (1 - eps), 1] the
    // product is  |x_j|^2 (1 - eps) - 2 x_i.x_j - u_i,  negative exactly for the pairs to keep (u rounded up, the norm
    // rounded down to float32; eps covers the float32 roundings of the accumulation).
    constexpr int KI = DP / 2 + 1;                             // MFMA steps (2-deep each), the last one carries the test
    __shared__ float Bs[2][SCAN_CT / 32][KI][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t qbase = (int64_t)(blockIdx.x / splits) * 128 + wave * 32;   // this wave's 32 queries (local row numbers)
    const int split = blockIdx.x % splits;                                  // ... against one slice of the corpus
    // A operand: lane holds A[m = r][k = 2i + h]
    float a[KI];
    {
        const bool live = qbase + r < rows;
        const int64_t q = live ? qbase + r : rows - 1;
#pragma unroll
        for (int i = 0; i < KI - 1; ++i) a[i] = -2.0f * zp32[(row0 + q) * DP + 2 * i + h];
        const float ur = live ? f32_round_up(u[q]) : -3.0e38f;  // padded queries keep nothing
        a[KI - 1] = h == 0 ? 1.0f : -ur;
    }
    const TileRange tiles = split_tiles(n, SCAN_CT, splits, split);
    const int64_t tile_lo = tiles.lo, n_tiles = tiles.hi;
    if (tile_lo >= n_tiles) return;
    // staging in two halves: the global loads of the next tile are issued before the MFMAs of the current one and
    // written to the other LDS buffer after them
    constexpr int PER = SCAN_CT * DP / 256;                    // floats per thread: (candidate, slice of its row)
    const int sc = (threadIdx.x * PER) / DP, sk0 = (threadIdx.x * PER) % DP;
    float vals[PER];
    float nval = 3.0e38f;
    auto fetch = [&](int64_t tile) {
        const int64_t c0 = tile * SCAN_CT;
        const int64_t j = c0 + sc < n ? c0 + sc : n - 1;
#pragma unroll
        for (int k = 0; k < PER; k += 4) {
            const float4 f = *reinterpret_cast<const float4 *>(zp32 + j * DP + sk0 + k);
            vals[k] = f.x; vals[k + 1] = f.y; vals[k + 2] = f.z; vals[k + 3] = f.w;
        }
        if (threadIdx.x < SCAN_CT) {
            const int64_t jj = c0 + threadIdx.x;
            nval = jj < n ? scan_norm(nrm[jj], eps) : 3.0e38f;  // beyond the corpus: never kept
        }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int kk = sk0 + k;
            Bs[buf][sc >> 5][kk >> 1][(kk & 1) * 32 + (sc & 31)] = vals[k];
        }
        if (threadIdx.x < SCAN_CT) {
            Bs[buf][threadIdx.x >> 5][KI - 1][threadIdx.x & 31] = nval;
            Bs[buf][threadIdx.x >> 5][KI - 1][32 + (threadIdx.x & 31)] = 1.0f;
        }
    };
    __shared__ unsigned long long eb[4][EQ_CAP];
    KeptQueue kept = {eb[wave], cnt, list, 0};
    // The signs of a lane's 32 accumulator entries (two column tiles) are packed into one word for the queue: a handful of
    // branches per 2 048 pairs.
    const int32_t rowb = (int32_t)qbase + 4 * h;               // local row of accumulator entry q: rowb + (q & 3) + 8 (q >> 2)
    auto keep_pairs = [&](const f32x16v &acc0, const f32x16v &acc1, int64_t cand0) {
        unsigned any = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) any |= __float_as_uint(acc0[q]) | __float_as_uint(acc1[q]);
        if (!__ballot((any & 0x80000000u) != 0)) return;       // wave-uniform: nothing to keep in these 2 048 pairs
        unsigned bits = 0;                                     // bit q: acc0[q] < 0, bit 16 + q: acc1[q] < 0
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            bits |= (__float_as_uint(acc0[q]) >> 31) << q;
            bits |= (__float_as_uint(acc1[q]) >> 31) << (16 + q);
        }
        kept.take(bits, [&](int b) {
            const int q = b & 15;
            return make_int2(rowb + (q & 3) + 8 * (q >> 2), (int32_t)(cand0 + (b >> 4) * 32 + r));
        });
    };
    fetch(tile_lo);
    put((int)(tile_lo & 1));
    __syncthreads();
    for (int64_t tile = tile_lo; tile < n_tiles; ++tile) {
        const int buf = (int)(tile & 1);
        if (tile + 1 < n_tiles) fetch(tile + 1);
#pragma unroll
        for (int t = 0; t < SCAN_CT / 32; t += 2) {           // two column tiles in flight: independent accumulators
            f32x16v acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll
            for (int i = 0; i < KI; ++i) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], Bs[buf][t][i][lane], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], Bs[buf][t + 1][i][lane], acc1, 0, 0, 0);
            }
            keep_pairs(acc0, acc1, tile * SCAN_CT + t * 32);       // a negative entry = a pair to keep
        }
        if (kept.qn >= EQ_CAP / 2) kept.flush(lane);
        if (tile + 1 < n_tiles) put(buf ^ 1);
        __syncthreads();
    }
    kept.flush(lane);
}

// ---- the same filter on the bf16 matrix cores ---------------------------------------------------------------------------
// x = hi + lo with hi = bf16(x), lo = bf16(x - hi): 16 significant bits.  x_i.x_j ~ hi_i.hi_j + hi_i.lo_j + lo_i.hi_j on
// v_mfma_f32_32x32x16_bf16 (three 32-cycle instructions per 32 x 32 pairs and 16 dimensions, against DP/2+1 64-cycle
// float32 ones); the dropped lo.lo term and the parts' own roundings are below 2^-16 |x_i||x_j|, which the caller's eps
// (relative to |x_i|^2 + |x_j|^2) covers.  The accumulator starts at -u_i; a lane's 16 entries belong to one candidate j, so
// the test is acc < -|x_j|^2 (1 - eps): the lane's minimum against one value (round 4; before, |x_j|^2 entered through a fourth
// MFMA and the sign was the test, as in knn_scan_kernel).  The kept pairs take the same queue.
typedef __bf16 bf16x8k __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned short bf16_rne(float x) {
    unsigned u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// zb [n][2][dpb] bf16 bit patterns: the two parts of every coordinate (dpb = dp rounded up to 16, zero padded)
__global__ __launch_bounds__(256) void knn_split_kernel(const float *__restrict__ zp32, const double *__restrict__ nrm,
                                                       int64_t n, int64_t n_pad, int dp, int dpb, double eps,
                                                       unsigned short *__restrict__ zb, float *__restrict__ negn) {
    // rows n .. n_pad - 1 (the scan reads whole tiles of 256 candidates): zeros, and a threshold nothing falls below
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad * dpb; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / dpb;
        const int c = (int)(i % dpb);
        const float x = (c < dp && r < n) ? zp32[r * dp + c] : 0.0f;
        const unsigned short hi = bf16_rne(x);
        const float rest = x - __uint_as_float((unsigned)hi << 16);      // exact
        zb[(r * 2 + 0) * dpb + c] = hi;
        zb[(r * 2 + 1) * dpb + c] = bf16_rne(rest);
        if (c == 0) {
            // -|x_j|^2 (1 - eps), the magnitude rounded DOWN to float32 (the scan keeps a pair when acc < this)
            negn[r] = -(r < n ? scan_norm(nrm[r], eps) : 3.0e38f);
        }
    }
}

template <int DPB, int SCAN_CT>
__global__ __launch_bounds__(256) void knn_scan_bf16_kernel(const unsigned short *__restrict__ zb,
                                                           const unsigned short *__restrict__ zbq,
                                                           const float *__restrict__ negn, const double *__restrict__ u,
                                                           int64_t n, int64_t row0, int64_t rows, int splits,
                                                           int32_t *__restrict__ cnt, int32_t *__restrict__ list) {
    constexpr int KST = DPB / 16;                              // MFMA k-steps
    // bytes per candidate in LDS: the hi row, the lo row, no padding -- the 16-byte pieces of a row are XOR-swizzled with the row
    // number instead, so that 16 consecutive candidates' reads of one piece spread over all banks (round 3 padded the rows to
    // 80 bytes at d <= 16: 47 KB per workgroup, three per CU; 38 KB fit four, and the scan is bound by the waves' serial latency)
    constexpr int ROWB = 2 * DPB * 2, PR = ROWB / 16;          // PR = 4 / 8 / 16 pieces per row
    auto swz = [](int row) { return (row / (16 / PR)) & (PR - 1); };
    __shared__ __attribute__((aligned(16))) unsigned char Ts[2][SCAN_CT * ROWB];
    // -|x_j|^2 (1 - eps), |.| rounded down to float32: a lane's accumulator entries all belong to ONE candidate (its column), so
    // "distance below the threshold" is acc < -n_j with acc = -u_i - 2 x_i.x_j -- the minimum of the lane's 16 entries against one
    // value (8 v_min3 + 1 compare per 1 024 pairs).  Round 3 added n_j inside the accumulator through one more MFMA (A = ones,
    // B = n_j in three bf16 parts): a quarter of the kernel's matrix-core time, and 16 ORs for the sign test on top.
    __shared__ float Nf[2][SCAN_CT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int64_t qbase = (int64_t)(blockIdx.x / splits) * 128 + wave * 32;   // this wave's 32 queries (local row numbers)
    const int split = blockIdx.x % splits;                                  // ... against one slice of the corpus
    const int sw = swz(r);                                     // swizzle of the candidate rows this lane reads (row = 32 t + r)
    // A operand: lane holds A[m = r][k = 16 ks + 8 h .. + 7] = -2 x (both parts: the scaling is exact)
    bf16x8k ahi[KST], alo[KST];
    float uq[16];                                              // u of the 16 rows this lane's accumulator entries belong to
    {
        const bool live = qbase + r < rows;
        const int64_t q = live ? qbase + r : rows - 1;
#pragma unroll
        for (int ks = 0; ks < KST; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = __uint_as_float((unsigned)zbq[((row0 + q) * 2 + 0) * DPB + ks * 16 + h * 8 + e] << 16);
                const float xl = __uint_as_float((unsigned)zbq[((row0 + q) * 2 + 1) * DPB + ks * 16 + h * 8 + e] << 16);
                ahi[ks][e] = (__bf16)(-2.0f * xh);
                alo[ks][e] = (__bf16)(-2.0f * xl);
            }
#pragma unroll
        for (int qq = 0; qq < 16; ++qq) {
            const int64_t row = qbase + (qq & 3) + 8 * (qq >> 2) + 4 * h;
            const float ur = row < rows ? f32_round_up(u[row]) : -3.0e38f;   // padded queries keep nothing
            uq[qq] = -ur;                                      // the accumulator starts at -u (the MFMA's C operand)
        }
    }
    f32x16v negu;
#pragma unroll
    for (int qq = 0; qq < 16; ++qq) negu[qq] = uq[qq];
    const TileRange tiles = split_tiles(n, SCAN_CT, splits, split);
    const int64_t tile_lo = tiles.lo, n_tiles = tiles.hi;
    if (tile_lo >= n_tiles) return;
    // staging: a tile's candidates are one contiguous run of SCAN_CT x 4 DPB bytes in zb (rows padded to whole tiles by
    // knn_split_kernel, so no index is clamped): piece k * 256 + tid of 16 bytes per thread and k, from a wave-uniform base
    constexpr int PIECES = SCAN_CT * PR;                       // 16-byte pieces per tile
    constexpr int PER = PIECES / 256;
    static_assert(PIECES % 256 == 0, "tile pieces divide among the threads");
    unsigned vals[PER][4];                                     // (scalars: an array of uint4 stays in scratch memory)
    float nval = 0.f;
    auto fetch = [&](int64_t tile) {
        const uint4 *tp = reinterpret_cast<const uint4 *>(zb + tile * SCAN_CT * 2 * DPB);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const uint4 f = tp[k * 256 + threadIdx.x];
            vals[k][0] = f.x; vals[k][1] = f.y; vals[k][2] = f.z; vals[k][3] = f.w;
        }
        if (threadIdx.x < SCAN_CT) nval = negn[tile * SCAN_CT + threadIdx.x];
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int piece = k * 256 + threadIdx.x;
            const int sc = piece / PR, off = piece % PR;
            *reinterpret_cast<uint4 *>(&Ts[buf][sc * ROWB + (off ^ swz(sc)) * 16]) = make_uint4(vals[k][0], vals[k][1], vals[k][2], vals[k][3]);
        }
        if (threadIdx.x < SCAN_CT) Nf[buf][threadIdx.x] = nval;
    };
    __shared__ unsigned long long eb[4][EQ_CAP];
    KeptQueue kept = {eb[wave], cnt, list, 0};
    // One 32 x 32 tile at a time: the lane's minimum against -n_j decides wave-wide whether anything is kept (8 v_min3 + a
    // compare; ~70 % of the tiles end here).  Otherwise the signs of acc - (-n_j) of a lane's 16 entries are packed into one word
    // for the queue (the sign of a float32 difference is the sign of the exact difference, denormals included).
    const int32_t rowb = (int32_t)qbase + 4 * h;               // local row of accumulator entry q: rowb + (q & 3) + 8 (q >> 2)
    auto keep_tile = [&](const f32x16v &acc, float negn, int32_t cand) {
        // (the two halves of the lane's entries separately: a tile that keeps something builds the sign word of one half only)
        float ma = __builtin_fminf(__builtin_fminf(acc[0], acc[1]), acc[2]);
        float mb = __builtin_fminf(__builtin_fminf(acc[8], acc[9]), acc[10]);
        ma = __builtin_fminf(__builtin_fminf(ma, acc[3]), acc[4]);
        mb = __builtin_fminf(__builtin_fminf(mb, acc[11]), acc[12]);
        ma = __builtin_fminf(__builtin_fminf(ma, acc[5]), acc[6]);
        mb = __builtin_fminf(__builtin_fminf(mb, acc[13]), acc[14]);
        ma = __builtin_fminf(ma, acc[7]);
        mb = __builtin_fminf(mb, acc[15]);
        if (!__ballot(__builtin_fminf(ma, mb) < negn)) return;  // wave-uniform: nothing to keep in these 1 024 pairs
        unsigned bits = 0;                                     // bit 15 - q: acc[q] < -n
        if (__ballot(ma < negn)) {
            unsigned w = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) w = __builtin_amdgcn_alignbit(w, __float_as_uint(acc[q] - negn), 31);   // (w << 1) | sign
            bits = w << 8;
        }
        if (__ballot(mb < negn)) {
            unsigned w = 0;
#pragma unroll
            for (int q = 8; q < 16; ++q) w = __builtin_amdgcn_alignbit(w, __float_as_uint(acc[q] - negn), 31);
            bits |= w;
        }
        kept.take(bits, [&](int b) {
            const int q = 15 - b;
            return make_int2(rowb + (q & 3) + 8 * (q >> 2), cand);
        });
    };
    fetch(tile_lo);
    put((int)(tile_lo & 1));
    __syncthreads();
    for (int64_t tile = tile_lo; tile < n_tiles; ++tile) {
        const int buf = (int)(tile & 1);
        if (tile + 1 < n_tiles) fetch(tile + 1);
        // One 32-candidate column tile per step, software-pipelined inside the wave: the fragments of tile t + 1 are requested
        // from LDS, the three MFMAs of tile t issued, and only then the keep test of tile t - 1 runs -- vector work and branches
        // of one tile under the matrix-core time of the next, instead of MFMAs -> wait -> test -> branch in sequence.
        constexpr int NT = SCAN_CT / 32;
        bf16x8k yh[2][KST], yl[2][KST];
        f32x16v accs[2];
        float negns[2];
        auto frags = [&](int t2, int slot) {
            const unsigned char *b = &Ts[buf][(t2 * 32 + r) * ROWB];
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                const int ph = ((2 * ks + h) ^ sw) * 16, pl = ((PR / 2 + 2 * ks + h) ^ sw) * 16;   // this lane's hi / lo piece
                yh[slot][ks] = *reinterpret_cast<const bf16x8k *>(b + ph);
                yl[slot][ks] = *reinterpret_cast<const bf16x8k *>(b + pl);
            }
            negns[slot] = Nf[buf][t2 * 32 + r];
        };
        const int32_t cand_t0 = (int32_t)(tile * SCAN_CT) + r;           // this lane's candidate in column tile 0
        frags(0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int cur = t & 1;
            const float negn_prev = negns[cur ^ 1];                    // (tile t - 1's, before the slot is refilled)
            if (t + 1 < NT) frags(t + 1, cur ^ 1);
            f32x16v acc = negu;
#pragma unroll
            for (int ks = 0; ks < KST; ++ks) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi[ks], yh[cur][ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi[ks], yl[cur][ks], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo[ks], yh[cur][ks], acc, 0, 0, 0);
            }
            accs[cur] = acc;
            __builtin_amdgcn_sched_barrier(0);
            if (t > 0) keep_tile(accs[cur ^ 1], negn_prev, cand_t0 + (t - 1) * 32);   // an entry below -n_j = a pair to keep
        }
        keep_tile(accs[(NT - 1) & 1], negns[(NT - 1) & 1], cand_t0 + (NT - 1) * 32);
        if (kept.qn >= EQ_CAP / 2) kept.flush(lane);
        if (tile + 1 < n_tiles) put(buf ^ 1);
        __syncthreads();
    }
    kept.flush(lane);
}

// one wave per query: the keys of its kept candidates into LDS, then the
// kq smallest in (distance, index) order -- the lists are a few hundred entries, unordered
template <int DCH, bool EXPANSION>
__global__ __launch_bounds__(256) void knn_refine_kernel(const float *__restrict__ zp32, const double *__restrict__ zq64,
                                                        const double *__restrict__ nrm, const double *__restrict__ nrm_q,
                                                        int nch, int kq, int64_t row0,
                                                        int64_t rows, const int32_t *__restrict__ cnt,
                                                        const int32_t *__restrict__ list, int32_t *__restrict__ idx_out,
                                                        double *__restrict__ d2_out, int32_t *__restrict__ overflow) {
    __shared__ double sv[KNN_WAVES][FILTER_CAP];
    // (the index of entry e is list[row][e]: no copy of it in LDS -- 35 KB per workgroup instead of 51, four per CU)
    __shared__ double cv[KNN_WAVES][64];                       // the entries at or below the kq-th distance, compacted
    __shared__ int32_t ci[KNN_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t row = (int64_t)blockIdx.x * KNN_WAVES + wave;
    if (row >= rows) return;
    const int dp = nch * DCH;
    const int32_t m_all = cnt[row];
    if (m_all > FILTER_CAP) { if (lane == 0) atomicAdd(overflow, 1); return; }
    const int64_t qr = row0 + row;
    // U candidates per lane at a time, all of their row loads in flight before the first fma: the rows are random 64- to 256-byte
    // gathers from a corpus far larger than the L2, and one candidate per lane and trip (round 3) paid that latency six times
    // over per query (27 ms of the 172 ms stage at one million latents).  Per candidate the fma chain is unchanged.
    constexpr int U = DCH <= 16 ? 4 : 2;
    for (int32_t c0 = 0; c0 < m_all; c0 += 64 * U) {
        int32_t j[U];
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            valid[u] = c0 + u * 64 + lane < m_all;
            j[u] = valid[u] ? list[row * FILTER_CAP + c0 + u * 64 + lane] : 0;
        }
        double acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = 0.0;
        for (int ch = 0; ch < nch; ++ch) {
            float4 f[U][DCH / 4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float4 *src = reinterpret_cast<const float4 *>(zp32 + (int64_t)j[u] * dp + ch * DCH);
#pragma unroll
                for (int v = 0; v < DCH / 4; ++v) f[u][v] = src[v];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int v = 0; v < DCH / 4; ++v) {
                    double c4[4];
                    f32x4_to_f64(f[u][v], c4);
                    acc[u] = key_chain<4, EXPANSION>(zq64 + qr * dp + ch * DCH + 4 * v, c4, acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double d2 = key_close<EXPANSION>(acc[u], EXPANSION ? nrm_q[qr] : 0.0, EXPANSION ? nrm[j[u]] : 0.0);
            if (valid[u]) sv[wave][c0 + u * 64 + lane] = d2;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // the wave's own LDS writes, read back below
    __builtin_amdgcn_wave_barrier();
    // Selection.  First the value of the kq-th smallest distance by quickselect over the wave's entries: a pivot from the window
    // (lo, hi) (lo: fewer than kq entries <= lo; hi: at least kq entries <= hi), one counting pass, ~2 ln(m) rounds of ~35
    // instructions.  Then the entries <= that value -- kq of them unless distances tie at the threshold -- are compacted (cv / ci)
    // and ordered by (distance, index) with a rank count, one entry per lane.  (Round 3 extracted the kq minima one by one: kq
    // rounds of an LDS rescan + a three-value butterfly, ~1 900 instructions per query, the bulk of this kernel's time.)
    // More than 64 entries at or below the threshold (masses of duplicates): the extraction loop below, as before.
    if (m_all >= kq) {
        double lo = -1.0, hi = inf64();                        // distances are >= 0 and finite
        int rot = 0;
        for (int guard = 0; guard < 2048; ++guard) {
            // pivot: the first entry inside (lo, hi) of the first lane (from a rotating start) that has one
            double cand = inf64();
            for (int32_t e = lane; e < m_all; e += 64) {
                const double v = sv[wave][e];
                if (v > lo && v < hi && !(cand < inf64())) cand = v;
            }
            unsigned long long has = __ballot(cand < inf64());
            if (!has) break;                                   // nothing strictly inside: the threshold is hi
            has = (has >> rot) | (rot ? has << (64 - rot) : 0ull);
            const int src = (__ffsll((long long)has) - 1 + rot) & 63;
            rot = (rot + 23) & 63;
            const double pivot = __shfl(cand, src, 64);
            int c = 0;
            for (int32_t e = lane; e < m_all; e += 64) c += sv[wave][e] <= pivot ? 1 : 0;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
            if (c >= kq) hi = pivot; else lo = pivot;
        }
        // hi == inf: fewer than kq finite entries (cannot happen); otherwise compact the entries <= hi
        int c_le = 0;
        for (int32_t e = lane; e < m_all; e += 64) c_le += sv[wave][e] <= hi ? 1 : 0;
        int incl = c_le;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        const int total = __shfl(incl, 63, 64);
        if (hi < inf64() && total <= 64) {
            int at = incl - c_le;
            for (int32_t e = lane; e < m_all; e += 64) {
                const double v = sv[wave][e];
                if (v <= hi) { cv[wave][at] = v; ci[wave][at] = list[row * FILTER_CAP + e]; ++at; }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            // rank of this lane's entry among the `total` compacted ones in (distance, index) order
            const double myv = lane < total ? cv[wave][lane] : inf64();
            const int32_t myi = lane < total ? ci[wave][lane] : 0x7fffffff;
            int rank = 0;
            for (int t2 = 0; t2 < total; ++t2) {
                const double ov = cv[wave][t2];
                const int32_t oi = ci[wave][t2];
                rank += (ov < myv || (ov == myv && oi < myi)) ? 1 : 0;
            }
            if (lane < total && rank < kq) {
                idx_out[row * kq + rank] = myi;
                d2_out[row * kq + rank] = myv;
            }
            return;
        }
    }
    // kq rounds of "extract the minimum in (distance, index) order": every lane scans its own strided entries,
    // a butterfly finds the wave's minimum, its owner retires it
    for (int round = 0; round < kq; ++round) {
        double bv = inf64();
        int32_t bi = 0x7fffffff, bpos = -1;
        for (int32_t e = lane; e < m_all; e += 64) {
            const double v = sv[wave][e];
            const int32_t id = list[row * FILTER_CAP + e];
            if (v < bv || (v == bv && id < bi)) { bv = v; bi = id; bpos = e; }
        }
        // the wave's smallest distance first (one 8-byte value through the butterfly), then its owner: almost always one lane;
        // equal distances in several lanes (duplicate latents) -> the lowest index among them
        double mv = bv;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mv = fmin(mv, __shfl_xor(mv, off, 64));
        if (!(mv < inf64())) break;                            // fewer candidates than kq (cannot happen: subset >= kq rows)
        const unsigned long long tied = __ballot(bv == mv);
        int owner = __ffsll((long long)tied) - 1;
        if (tied & (tied - 1)) {                               // wave-uniform
            int32_t mi = bv == mv ? bi : 0x7fffffff;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) mi = min(mi, __shfl_xor(mi, off, 64));
            owner = __ffsll((long long)__ballot(bv == mv && bi == mi)) - 1;
        }
        bi = __shfl(bi, owner, 64);
        bpos = __shfl(bpos, owner, 64);
        if (lane == owner) sv[wave][bpos] = inf64();           // retired (real distances are finite)
        if (lane == 0) {
            idx_out[row * kq + round] = bi;
            d2_out[row * kq + round] = mv;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- nearest node of another component (geo_nearest_foreign, geo_bridge_components) -------------------------------------------
// knn_kernel's mapping with the k-list replaced by ONE running (key, index) minimum per lane and query: the wave's Q queries
// are gathered through `rows`, their coordinates stay wave-uniform fp64 through the scalar cache, every lane owns one candidate
// per 64-candidate step.  Candidates arrive in ascending index, so `<` keeps the lowest index among equal keys; a butterfly by
// (key, index) closes each query.  The pair key is the one geo_knn_topk gives row max(q, x) in the list of row min(q, x): the
// fma chains are symmetric in the two rows, only the order of the two norms of the expansion form is not -- the norm of the
// LOWER index is added first.  A 64-candidate step lies wholly below or wholly above the query row except the one that holds
// it, so the order is a wave-uniform branch and costs a per-lane select in that one step only.
// What keeps a candidate out:
//  - a lane past the corpus' end: its key is made +inf by the arithmetic itself, as in knn_bound_kernel (no select per query);
//  - a candidate of the query's own component: when the wave's Q queries share one label (always at Q = 1; runs of one
//    component in a query list) the same +inf, one compare per candidate for all Q queries; otherwise one v_cmp_ne_u32 against
//    the query's label in an SGPR, and-ed into the update mask on the scalar unit.
// The update itself is one v_cmp_lt_f64 and three v_cndmask per candidate and query against ~DCH v_fma_f64.
template <int DCH, int Q, bool EXPANSION>
__global__ __launch_bounds__(256) void nearest_foreign_kernel(const float *__restrict__ zp32, const double *__restrict__ zq64,
                                                             const double *__restrict__ nrm, const int32_t *__restrict__ labels,
                                                             const int32_t *__restrict__ rows, int64_t m, int64_t n, int nch,
                                                             int32_t *__restrict__ nbr_out, double *__restrict__ key_out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t q0 = ((int64_t)blockIdx.x * KNN_WAVES + wave) * Q;
    if (q0 >= m) return;
    const int dp = nch * DCH;
    int32_t qrow[Q], ql[Q];                                    // wave-uniform (the queries' norms are re-read through the scalar
    bool uniform = true;                                       // cache where they are used, as in knn_kernel: 2 Q SGPRs less)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int64_t qi = q0 + q < m ? q0 + q : m - 1;        // (a padded slot repeats the last query)
        qrow[q] = __builtin_amdgcn_readfirstlane(rows[qi]);
        ql[q] = __builtin_amdgcn_readfirstlane(labels[qrow[q]]);
        uniform = uniform && ql[q] == ql[0];
    }
    double bk[Q];
    int32_t bi[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) { bk[q] = inf64(); bi[q] = -1; }

    // (n < 2^31: 32-bit step and row numbers keep the order test below on the scalar unit, which compares no 64-bit integers)
    const uint32_t n32 = (uint32_t)n;
    for (uint32_t c0 = 0; c0 < n32; c0 += 64) {
        const uint32_t j = c0 + (uint32_t)lane;
        const bool valid = j < n32;
        const int64_t jc = valid ? j : n32 - 1;
        const int32_t lab = labels[jc];
        const double nrm_j = EXPANSION ? nrm[jc] : 0.0;        // requested before the fma chains, not behind a branch after them
        const bool out = !valid || (uniform && lab == ql[0]);
        double acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = (!EXPANSION && out) ? inf64() : 0.0;
        for (int ch = 0; ch < nch; ++ch) {
            double cj[DCH];
            const float4 *src = reinterpret_cast<const float4 *>(zp32 + jc * dp + ch * DCH);
#pragma unroll
            for (int v = 0; v < DCH / 4; ++v) f32x4_to_f64(src[v], cj + 4 * v);
#pragma unroll
            for (int q = 0; q < Q; ++q)
                acc[q] = key_chain<DCH, EXPANSION>(zq64 + (int64_t)qrow[q] * dp + ch * DCH, cj, acc[q]);
        }
        const double nj = out ? inf64() : nrm_j;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double d2 = acc[q];
            if (EXPANSION) {
                const uint32_t qr = (uint32_t)qrow[q];
                const double nq = nrm[qrow[q]];
                // key_close written out, the one copy: -2 acc before and the clamp after the wave-uniform branch on the order of
                // the norms.  With key_close in each arm the arms each multiply and clamp (<16, 4, true> 1 272 -> 1 316
                // instructions, the first round's scan at 60 000 x 16 mutual k = 10 1.108 -> 1.140 ms); with the norms picked
                // in the arms and one key_close after them the compiler selects per lane in every step (<8, 8, true> 69 -> 82 VGPRs)
                const double t = -2.0 * d2;
                if (c0 > qr) d2 = (nq + t) + nj;                               // the query is the lower row of every pair
                else if (c0 + 63 < qr) d2 = (nj + t) + nq;                     // ... the higher row of every pair
                else d2 = j < qr ? (nj + t) + nq : (nq + t) + nj;
                if (!(d2 > 0.0)) d2 = 0.0;
            }
            bool upd = d2 < bk[q];
            if (!uniform) upd = upd && lab != ql[q];
            bk[q] = upd ? d2 : bk[q];
            bi[q] = upd ? (int32_t)j : bi[q];
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        double k = bk[q];
        int32_t i = bi[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ok = __shfl_xor(k, off, 64);
            const int32_t oi = __shfl_xor(i, off, 64);
            if (ok < k || (ok == k && oi < i)) { k = ok; i = oi; }
        }
        if (lane == 0 && q0 + q < m) {
            nbr_out[q0 + q] = i;
            key_out[q0 + q] = k;
        }
    }
}

// ---- Boruvka bookkeeping of geo_bridge_components (everything but the scan: O(n) per round) ---------------------------------------
__global__ __launch_bounds__(256) void bridge_hist_kernel(const int32_t *__restrict__ labels, int64_t n, int32_t C,
                                                         int32_t *__restrict__ cur, int32_t *__restrict__ sizes,
                                                         int32_t *__restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t l = labels[i];
        cur[i] = l;
        if (l < 0 || l >= C) *bad = 1;
        else atomicAdd(&sizes[l], 1);
    }
}

__global__ __launch_bounds__(256) void bridge_flag_kernel(const int32_t *__restrict__ cur, int64_t n, int32_t big,
                                                         int32_t *__restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        flag[i] = cur[i] != big ? 1 : 0;
}

__global__ __launch_bounds__(256) void bridge_rows_kernel(const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                         int64_t n, int32_t *__restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (flag[i]) rows[pos[i]] = (int32_t)i;
}

// keys are >= +0 or +inf: their bit patterns order as unsigned integers
__global__ __launch_bounds__(256) void bridge_minkey_kernel(const int32_t *__restrict__ cur, const int32_t *__restrict__ rows,
                                                           const double *__restrict__ key, int64_t m,
                                                           unsigned long long *__restrict__ minkey) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        atomicMin(&minkey[cur[rows[i]]], (unsigned long long)__double_as_longlong(key[i]));
}

__global__ __launch_bounds__(256) void bridge_minedge_kernel(const int32_t *__restrict__ cur, const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ nbr, const double *__restrict__ key,
                                                            int64_t m, const unsigned long long *__restrict__ minkey,
                                                            unsigned long long *__restrict__ minedge) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = rows[i], b = nbr[i], c = cur[a];
        if (b < 0 || (unsigned long long)__double_as_longlong(key[i]) != minkey[c]) continue;
        const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
        atomicMin(&minedge[c], ((unsigned long long)lo << 32) | hi);
    }
}

// the component at the other end of every component's chosen edge (one writer per component: the edge's own end)
__global__ __launch_bounds__(256) void bridge_other_kernel(const int32_t *__restrict__ cur, const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ nbr, const double *__restrict__ key,
                                                          int64_t m, const unsigned long long *__restrict__ minkey,
                                                          const unsigned long long *__restrict__ minedge,
                                                          int32_t *__restrict__ other) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t a = rows[i], b = nbr[i], c = cur[a];
        if (b < 0 || (unsigned long long)__double_as_longlong(key[i]) != minkey[c]) continue;
        const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
        if ((((unsigned long long)lo << 32) | hi) == minedge[c]) other[c] = cur[b];
    }
}

__global__ __launch_bounds__(256) void bridge_relabel_kernel(int32_t *__restrict__ cur, int64_t n,
                                                            const int32_t *__restrict__ map) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        cur[i] = map[cur[i]];
}

struct KnnPlan { int dch, nch, dp; };

KnnPlan plan_for(int d) {
    KnnPlan p;
    if (d <= 8) { p.dch = 8; p.nch = 1; }
    else if (d <= 16) { p.dch = 16; p.nch = 1; }
    else { p.dch = 32; p.nch = (d + 31) / 32; }
    p.dp = p.dch * p.nch;
    return p;
}

// ---- one dispatch of the search kernels' template instances ----------------------------------------------------------------
// The run-time (p.dch, expansion) as compile-time constants: f(int_c<DCH>, std::bool_constant<EXPANSION>).  Every launch of a
// search kernel goes through here; what else a kernel is instantiated on (queries per wave, list registers, minima per lane) its
// launcher passes the same way, so a generic lambda instantiates the combinations its launcher's routes reach and no others.
template <int V>
using int_c = std::integral_constant<int, V>;

template <class F>
void with_key_form(const KnnPlan &p, bool expansion, F &&f) {
    auto with_form = [&](auto dch) {
        if (expansion) f(dch, std::true_type{});
        else f(dch, std::false_type{});
    };
    if (p.dch == 8) with_form(int_c<8>{});
    else if (p.dch == 16) with_form(int_c<16>{});
    else with_form(int_c<32>{});
}

// the path the calling thread's last geo_knn_topk took (GEO_KNN_PATH_* of include/geo_hip.h), for tests and profiles
thread_local int32_t g_last_path = 0;

bool filter_applies(int64_t n, int dp) {
    if (geo::options().knn_filter == 0) return false;
    // worth it from ~40 000 rows at 16 dimensions; the exact scan costs in proportion to the dimension
    const int64_t n_min = 640000 / dp > 16384 ? 640000 / dp : 16384;
    return n >= n_min && (dp == 8 || dp == 16 || dp == 32 || dp == 64);
}

// ---- one dispatch for both entry points ---------------------------------------------------------------------------------
// geo_knn_topk (queries = rows of the corpus) and geo_knn_query (queries of their own) differ in where the query side of the
// kernels points, nothing else: the corpus side is prepared once (KnnCorpus), a range of query rows is described by KnnQuery
// and searched by search_rows, which picks the path from n, dp, kq and the knn_filter option alone.

// the corpus side of one pass: the rows a kernel searches (zb / negn: their bf16 parts and norm column, where a scan reads them)
struct KnnSide { const float *z32; const double *nrm; const unsigned short *zb; const float *negn; int64_t rows; };

struct KnnCorpus {
    const float *zp32;                 // [n][dp] zero padded
    const double *nrm;                 // [n]
    int64_t n;
    // the filter paths (prepare_filter_corpus)
    int S, dpb;
    int64_t m, m0, n_pad, m_pad;       // subset rows (every S-th), subset of the subset, rows padded to whole scan tiles
    bool bf16_scan, two_level;
    double eps;
    float *zs32; double *nrm_s;        // [m][dp], [m]
    unsigned short *zb; float *negn;   // [n_pad][2][dpb], [n_pad]
    float *zs0; double *nrm_s0;        // [m0][dp], [m0]                 (two levels)
    unsigned short *zb_s; float *negn_s;
    KnnSide all() const { return {zp32, nrm, zb, negn, n}; }
    KnnSide subset() const { return {zs32, nrm_s, zb_s, negn_s, m}; }
    KnnSide subset0() const { return {zs0, nrm_s0, nullptr, nullptr, m0}; }
};

// query rows [row0, row1) of the arrays below; outputs and the per-query buffers are indexed from row0
struct KnnQuery {
    const double *zq64;                // [..][dp]
    const double *nrm_q;
    const unsigned short *zbq;         // [..][2][dpb] (bf16 scan)
    int64_t row0, row1;
    int64_t f32_row0;                  // the row of corpus.zp32 where query row0's float32 copy lies: knn_scan_kernel reads its
};                                     // queries from the corpus array (row0 itself in a self-search)

struct KnnLists { double *u; int32_t *cnt, *list, *overflow; };      // per query row of a range: [rows], [rows], [rows][FILTER_CAP]

// ---- the workspace layouts, each run by its *_workspace_bytes query on a measuring arena and by its entry point on the caller's
// memory.  The queries size the filter's arrays for the densest subset, the one of the longest lists:
constexpr int KQ_DENSEST = 64;
static_assert(filter_stride(KQ_DENSEST) == FILTER_STRIDE_MIN, "the queries measure the filter corpus at the smallest stride");

// the padded float32 corpus, its fp64 copy and the squared norms (knn_prep_kernel)
struct PlainCorpus { float *zp32; double *zq64, *nrm; };
PlainCorpus carve_plain_corpus(geo::Arena &ar, const KnnPlan &p, int64_t n) {
    return {ar.take<float>((size_t)n * p.dp), ar.take<double>((size_t)n * p.dp), ar.take<double>((size_t)n)};
}

// the filter's corpus-side arrays out of the arena, in geo_knn_topk's order (its u / cnt / list lie between nrm_s and overflow)
void carve_filter_corpus(geo::Arena &ar, const KnnPlan &p, int64_t n, int kq, KnnCorpus &c, KnnLists &lists, int64_t list_rows) {
    c.S = filter_stride(kq);
    c.m = (n + c.S - 1) / c.S;
    ar.take(c.zs32, (size_t)c.m * p.dp);
    ar.take(c.nrm_s, (size_t)c.m);
    if (list_rows > 0) {                                  // (geo_knn_query keeps them per slice, behind the corpus)
        ar.take(lists.u, (size_t)list_rows);
        ar.take(lists.cnt, (size_t)list_rows);
        ar.take(lists.list, (size_t)list_rows * FILTER_CAP);
    }
    ar.take(lists.overflow, 16);
    c.dpb = p.dp < 16 ? 16 : p.dp;
    c.bf16_scan = geo::options().knn_filter != 2;         // 2: the float32 matrix-core scan (comparison runs)
    c.n_pad = (n + 255) / 256 * 256;                      // the scan reads whole tiles
    c.m_pad = (c.m + 255) / 256 * 256;
    ar.take(c.zb, (size_t)c.n_pad * 2 * c.dpb);
    ar.take(c.negn, (size_t)c.n_pad);
    c.m0 = (c.m + c.S - 1) / c.S;
    // the second level's arrays, an optional group: a caller with a smaller workspace gets one level
    const size_t one_level = ar.mark();
    ar.take(c.zs0, (size_t)c.m0 * p.dp);
    ar.take(c.nrm_s0, (size_t)c.m0);
    ar.take(c.zb_s, (size_t)c.m_pad * 2 * c.dpb);
    ar.take(c.negn_s, (size_t)c.m_pad);
    if (!ar.ok()) { ar.rewind(one_level); c.zs0 = nullptr; c.nrm_s0 = nullptr; c.zb_s = nullptr; c.negn_s = nullptr; }
    // a d-term float32 dot product errs by < (d + 2) 2^-24 |x||y|, |x||y| <= (|x|^2 + |y|^2) / 2, and the float32
    // test adds a few more roundings of the same size: 16x margin
    // (the bf16 scan keeps 16 bits of every coordinate: its products err by < 2^-16 (|x|^2 + |y|^2) on top, 4x margin)
    c.eps = 16.0 * (p.dp + 2) * 5.9604644775390625e-08 + (c.bf16_scan ? 4.0 * 1.52587890625e-05 : 0.0);
    // Large inputs: the pass over every S-th row is itself N^2 / S fp64 work (S = 16: 100 ms of 255 at a million latents).
    // Two levels instead: thresholds from every S-th row of every S-th row (knn_bound_kernel), with them the SAME filter +
    // refinement over the every-S-th-row subset gives the exact kq-th distance to that subset -- at least as tight as the
    // threshold of the one-level scheme; the same candidate counts at both levels.
    c.two_level = c.bf16_scan && c.zs0 && n >= TWO_LEVEL_MIN && c.m0 >= kq;
}

// the corpus-side launches of the filter paths: the threshold subset(s) and the bf16 parts
int prepare_filter_corpus(const KnnPlan &p, const KnnCorpus &c, hipStream_t stream) {
    knn_subset_kernel<<<geo::grid_for(c.m * p.dp, 256, 4096), 256, 0, stream>>>(c.zp32, c.nrm, c.n, p.dp, c.S, c.m, c.zs32, c.nrm_s);
    GEO_LAUNCH_CHECK();
    if (c.bf16_scan) {
        knn_split_kernel<<<geo::grid_for(c.n_pad * c.dpb, 256, 4096), 256, 0, stream>>>(c.zp32, c.nrm, c.n, c.n_pad, p.dp, c.dpb, c.eps,
                                                                                          c.zb, c.negn);
        GEO_LAUNCH_CHECK();
    }
    if (c.two_level) {
        knn_subset_kernel<<<geo::grid_for(c.m0 * p.dp, 256, 4096), 256, 0, stream>>>(c.zs32, c.nrm_s, c.m, p.dp, c.S, c.m0, c.zs0, c.nrm_s0);
        GEO_LAUNCH_CHECK();
        knn_split_kernel<<<geo::grid_for(c.m_pad * c.dpb, 256, 4096), 256, 0, stream>>>(c.zs32, c.nrm_s, c.m, c.m_pad, p.dp, c.dpb, c.eps,
                                                                                          c.zb_s, c.negn_s);
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}

// ---- the launches of a search: each takes the corpus side it runs against and the query range ---------------------------------
// The exact scan.  Lists longer than one wave (64 < kq <= 256) take 2 or 4 list registers per lane at 4 queries per wave; of the
// one-register lists, fewer queries per wave keep the chip busy on small inputs.
int launch_knn_exact(const KnnPlan &p, bool ex, int kq, const KnnSide &c, const KnnQuery &q, int32_t *idx_out, double *d2_out,
                     hipStream_t s) {
    auto launch = [&](auto q_c, auto lr_c) {
        constexpr int Q = decltype(q_c)::value, LR = decltype(lr_c)::value;
        const int64_t waves = (q.row1 - q.row0 + Q - 1) / Q;
        const unsigned grid = (unsigned)((waves + KNN_WAVES - 1) / KNN_WAVES);
        with_key_form(p, ex, [&](auto dch, auto form) {
            knn_kernel<decltype(dch)::value, Q, decltype(form)::value, LR><<<grid, 256, 0, s>>>(
                c.z32, q.zq64, c.nrm, q.nrm_q, c.rows, p.nch, kq, q.row0, q.row1, idx_out, d2_out);
        });
    };
    if (kq > 128) launch(int_c<4>{}, int_c<4>{});
    else if (kq > 64) launch(int_c<4>{}, int_c<2>{});
    else if (q.row1 - q.row0 < 16384) launch(int_c<4>{}, int_c<1>{});
    else launch(int_c<16>{}, int_c<1>{});
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// thresholds bounded over the rows of `sub`: u / cnt for a scan, tau_out for geo_knn_thresholds (either may be null)
int launch_knn_bound(const KnnPlan &p, bool ex, int kq, const KnnSide &sub, const KnnQuery &q, double eps, double *u, int32_t *cnt,
                     double *tau_out, hipStream_t s) {
    const unsigned grid = (unsigned)((q.row1 - q.row0 + BOUND_Q - 1) / BOUND_Q);
    auto launch = [&](auto nm_c) {
        with_key_form(p, ex, [&](auto dch, auto form) {
            knn_bound_kernel<decltype(dch)::value, BOUND_Q, decltype(nm_c)::value, decltype(form)::value><<<grid, 256, 0, s>>>(
                sub.z32, q.zq64, sub.nrm, q.nrm_q, sub.rows, p.nch, kq, q.row0, q.row1, eps, u, cnt, tau_out);
        });
    };
    if (bound_minima(kq) == 2) launch(int_c<2>{});
    else launch(int_c<3>{});
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// corpus slices per 128-query block of a scan: enough workgroups, tiles to spare
int scan_splits(int64_t rows, int64_t corpus) {
    const int64_t qb = (rows + 127) / 128;
    int64_t sp = 16384 / qb;
    if (sp > 64) sp = 64;
    if (sp > (corpus + 255) / 256) sp = (corpus + 255) / 256;
    return (int)(sp > 1 ? sp : 1);
}

int launch_scan_bf16(int dpb, const KnnSide &c, const KnnQuery &q, const KnnLists &l, hipStream_t s) {
    const int64_t rows = q.row1 - q.row0;
    const int splits = scan_splits(rows, c.rows);
    const unsigned grid = (unsigned)((rows + 127) / 128) * (unsigned)splits;
    auto launch = [&](auto dpb_c, auto ct_c) {
        knn_scan_bf16_kernel<decltype(dpb_c)::value, decltype(ct_c)::value><<<grid, 256, 0, s>>>(
            c.zb, q.zbq, c.negn, l.u, c.rows, q.row0, rows, splits, l.cnt, l.list);
    };
    if (dpb == 16) launch(int_c<16>{}, int_c<256>{});
    else if (dpb == 32) launch(int_c<32>{}, int_c<256>{});
    else launch(int_c<64>{}, int_c<128>{});
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// (reads its queries from the corpus array, from row q.f32_row0)
int launch_scan_f32(int dp, const KnnSide &c, const KnnQuery &q, double eps, const KnnLists &l, hipStream_t s) {
    const int64_t rows = q.row1 - q.row0;
    const int splits = scan_splits(rows, c.rows);
    const unsigned grid = (unsigned)((rows + 127) / 128) * (unsigned)splits;
    auto launch = [&](auto dp_c, auto ct_c) {
        knn_scan_kernel<decltype(dp_c)::value, decltype(ct_c)::value><<<grid, 256, 0, s>>>(
            c.z32, c.nrm, l.u, c.rows, q.f32_row0, rows, eps, splits, l.cnt, l.list);
    };
    if (dp == 8) launch(int_c<8>{}, int_c<256>{});
    else if (dp == 16) launch(int_c<16>{}, int_c<256>{});
    else if (dp == 32) launch(int_c<32>{}, int_c<256>{});
    else launch(int_c<64>{}, int_c<128>{});
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

int launch_knn_refine(const KnnPlan &p, bool ex, int kq, const KnnSide &c, const KnnQuery &q, const KnnLists &l, int32_t *idx_out,
                      double *d2_out, hipStream_t s) {
    const int64_t rows = q.row1 - q.row0;
    const unsigned grid = (unsigned)((rows + KNN_WAVES - 1) / KNN_WAVES);
    with_key_form(p, ex, [&](auto dch, auto form) {
        knn_refine_kernel<decltype(dch)::value, decltype(form)::value><<<grid, 256, 0, s>>>(
            c.z32, q.zq64, c.nrm, q.nrm_q, p.nch, kq, q.row0, rows, l.cnt, l.list, idx_out, d2_out, l.overflow);
    });
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// One pass of the filter over the rows of `side`: thresholds -> scan -> refinement -> the overflow word read back (the pass' one
// stream synchronisation).  The thresholds are a bound over the rows of `thr`, or, with thr null, the kq-th entries that the pass
// before left in d2_out.  *overflowed: some query kept more than FILTER_CAP candidates (masses of near-duplicates), the lists
// are not valid.  The caller has cleared the overflow word.
int filter_pass(const KnnPlan &p, bool ex, int kq, const KnnCorpus &c, const KnnSide *thr, const KnnSide &side, const KnnQuery &q,
                const KnnLists &l, int32_t *idx_out, double *d2_out, hipStream_t stream, bool *overflowed) {
    int rc;
    if (thr) {
        rc = launch_knn_bound(p, ex, kq, *thr, q, c.eps, l.u, l.cnt, nullptr, stream);
        if (rc) return rc;
    } else {
        const int64_t rows = q.row1 - q.row0;
        knn_tau_kernel<<<geo::grid_for(rows, 256, 4096), 256, 0, stream>>>(d2_out, q.nrm_q, q.row0, rows, kq, c.eps, l.u, l.cnt);
        GEO_LAUNCH_CHECK();
    }
    rc = c.bf16_scan ? launch_scan_bf16(c.dpb, side, q, l, stream) : launch_scan_f32(p.dp, side, q, c.eps, l, stream);
    if (rc) return rc;
    rc = launch_knn_refine(p, ex, kq, side, q, l, idx_out, d2_out, stream);
    if (rc) return rc;
    int32_t h_over = 0;
    GEO_HIP_CHECK(hipMemcpyAsync(&h_over, l.overflow, 4, hipMemcpyDeviceToHost, stream));
    GEO_HIP_CHECK(hipStreamSynchronize(stream));
    *overflowed = h_over != 0;
    return GEO_OK;
}

// The kq nearest corpus rows of the query rows q, into idx_out / d2_out [row1 - row0][kq]; *path = the GEO_KNN_PATH_* taken.
// l = the range's candidate buffers when the filter applies (corpus prepared by prepare_filter_corpus), else null.
int search_rows(const KnnPlan &p, bool ex, int kq, const KnnCorpus &c, const KnnQuery &q, const KnnLists *l, int32_t *idx_out,
                double *d2_out, hipStream_t stream, int32_t *path) {
    if (kq > 64) {                                // no float32 filter here: its candidate lists are sized for kq <= 64
        *path = GEO_KNN_PATH_EXACT_WIDE;
        return launch_knn_exact(p, ex, kq, c.all(), q, idx_out, d2_out, stream);
    }
    if (l) {
        const KnnSide subset0 = c.subset0(), subset = c.subset(), all = c.all();
        GEO_HIP_CHECK(hipMemsetAsync(l->overflow, 0, 4, stream));
        bool over = false, tau_done = false;
        if (c.two_level) {                        // the kq smallest exact distances to the subset -> d2_out
            const int rc = filter_pass(p, ex, kq, c, &subset0, subset, q, *l, idx_out, d2_out, stream, &over);
            if (rc) return rc;
            tau_done = !over;
            if (over) GEO_HIP_CHECK(hipMemsetAsync(l->overflow, 0, 4, stream));
        }
        *path = tau_done ? GEO_KNN_PATH_TWO_LEVEL : c.bf16_scan ? GEO_KNN_PATH_FILTER_BF16 : GEO_KNN_PATH_FILTER_F32;
        const int rc = filter_pass(p, ex, kq, c, tau_done ? nullptr : &subset, all, q, *l, idx_out, d2_out, stream, &over);
        if (rc) return rc;
        if (!over) return GEO_OK;
        // some query kept more than FILTER_CAP candidates: exact scan for everything
        *path |= GEO_KNN_PATH_OVERFLOW;
    } else {
        *path = GEO_KNN_PATH_EXACT;
    }
    return launch_knn_exact(p, ex, kq, c.all(), q, idx_out, d2_out, stream);
}

// what one query row of a slice keeps in geo_knn_query's workspace, in 4-byte elements (geo::plan_passes): the padded
// float32 row (first: it continues the corpus array, see KnnQuery::f32_row0), the fp64 row, the norm; on the filter paths the
// bf16 parts, the split kernel's unused norm column, u, cnt and the candidate list
constexpr int QUERY_BUFS = 8;
int query_per_item(const KnnPlan &p, bool filter, size_t *per_item) {
    const size_t dpb = p.dp < 16 ? 16 : p.dp;
    per_item[0] = (size_t)p.dp; per_item[1] = 2 * (size_t)p.dp; per_item[2] = 2;
    if (!filter) return 3;
    per_item[3] = dpb; per_item[4] = 1; per_item[5] = 2; per_item[6] = 1; per_item[7] = FILTER_CAP;
    return QUERY_BUFS;
}
constexpr int64_t QUERY_MIN_SLICE = 128, QUERY_PREP_CHUNK = 65536;

// the corpus side of geo_knn_query's workspace: what geo_knn_topk keeps without its fp64 copy and per-row buffers, a
// QUERY_PREP_CHUNK-row fp64 scratch for knn_prep_kernel instead (the corpus' fp64 rows are not read), the padded float32
// corpus last: it ends where the slices' buffers begin
struct QueryCorpus { double *nrm, *z64_scratch; float *zp_block; int64_t chunk; };
QueryCorpus carve_query_corpus(geo::Arena &ar, const KnnPlan &p, int64_t n, bool filter, int kq, KnnCorpus *c, KnnLists *lists) {
    QueryCorpus o;
    o.chunk = n < QUERY_PREP_CHUNK ? n : QUERY_PREP_CHUNK;
    ar.take(o.nrm, (size_t)n);
    ar.take(o.z64_scratch, (size_t)o.chunk * p.dp);
    if (filter) carve_filter_corpus(ar, p, n, kq, *c, *lists, 0);
    ar.take(o.zp_block, (size_t)n * p.dp);
    return o;
}

// what the geo_knn, geo_nearest_foreign and geo_bridge_components queries answer beyond their measured layouts
constexpr size_t KNN_RESERVE = 1024, FOREIGN_RESERVE = 1024, BRIDGE_RESERVE = 1024;

}  // namespace

extern "C" size_t geo_knn_workspace_bytes(int64_t n, int32_t d) {
    if (n <= 0 || d <= 0) return 1024;
    const KnnPlan p = plan_for(d);
    geo::Arena ar;
    carve_plain_corpus(ar, p, n);
    if (filter_applies(n, p.dp)) {
        KnnCorpus c = {};
        KnnLists lists = {};
        carve_filter_corpus(ar, p, n, KQ_DENSEST, c, lists, n);
    }
    return ar.off + KNN_RESERVE;
}

extern "C" int geo_knn_topk(const float *z, int64_t n, int32_t d, int32_t n_neighbors, int32_t form, int64_t row0,
                            int64_t row1, int32_t *idx_out, double *d2_out, void *ws, size_t ws_bytes,
                            void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    g_last_path = 0;
    GEO_REQUIRE(z && idx_out && d2_out && ws, "geo_knn_topk: null pointer");
    GEO_REQUIRE(n > 0 && n < (int64_t)1 << 31, "geo_knn_topk: n=%lld out of range", (long long)n);
    GEO_REQUIRE(d > 0 && d <= 128, "geo_knn_topk: d=%d not in [1,128]", d);
    GEO_REQUIRE(n_neighbors > 0 && n_neighbors <= GEO_KNN_MAX_NEIGHBORS && n_neighbors <= n,
                "geo_knn_topk: n_neighbors=%d not in [1, min(%d, n)]", n_neighbors, GEO_KNN_MAX_NEIGHBORS);
    GEO_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= n, "geo_knn_topk: bad row range");
    if (row0 == row1) return GEO_OK;
    const KnnPlan p = plan_for(d);
    const int S = filter_stride(n_neighbors);
    const bool filter = n_neighbors <= 64 && filter_applies(n, p.dp) && (n + S - 1) / S >= n_neighbors;
    geo::Arena ar(ws, ws_bytes);
    const PlainCorpus pc = carve_plain_corpus(ar, p, n);
    KnnCorpus c = {};
    KnnLists lists = {};
    if (filter) carve_filter_corpus(ar, p, n, n_neighbors, c, lists, n);
    if (!ar.ok()) {
        geo::set_error("geo_knn_topk: workspace %zu too small (%zu needed)", ws_bytes, ar.off);
        return GEO_E_WORKSPACE;
    }
    c.zp32 = pc.zp32; c.nrm = pc.nrm; c.n = n;
    knn_prep_kernel<<<geo::grid_for(n, 256, 4096), 256, 0, stream>>>(z, n, d, p.dp, pc.zp32, pc.zq64, pc.nrm);
    GEO_LAUNCH_CHECK();
    if (filter) {
        const int rc = prepare_filter_corpus(p, c, stream);
        if (rc) return rc;
    }
    const KnnQuery q = {pc.zq64, pc.nrm, c.zb, row0, row1, row0};     // the corpus' own rows
    int32_t path = 0;
    const int rc = search_rows(p, form != 0, n_neighbors, c, q, filter ? &lists : nullptr, idx_out, d2_out, stream, &path);
    g_last_path = path;
    return rc;
}

extern "C" size_t geo_knn_query_min_workspace_bytes(int64_t n, int32_t d) {
    return geo_knn_query_workspace_bytes(n, 0, d);        // one slice of QUERY_MIN_SLICE rows
}

extern "C" size_t geo_knn_query_workspace_bytes(int64_t n, int64_t m, int32_t d) {
    if (n <= 0 || d <= 0) return 1024;
    const KnnPlan p = plan_for(d);
    size_t per_item[QUERY_BUFS];
    const bool filter = filter_applies(n, p.dp);
    const int nb = query_per_item(p, filter, per_item);
    KnnCorpus c = {};
    KnnLists lists = {};
    return geo::measure(carve_query_corpus, p, n, filter, KQ_DENSEST, &c, &lists) +
           geo::pass_bytes(per_item, nb, m > QUERY_MIN_SLICE ? m : QUERY_MIN_SLICE);
}

extern "C" int geo_knn_query(const float *z, int64_t n, const float *q, int64_t m, int32_t d, int32_t n_neighbors, int32_t form,
                             int32_t *idx_out, double *d2_out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    g_last_path = 0;
    GEO_REQUIRE(z && q && idx_out && d2_out && ws, "geo_knn_query: null pointer");
    GEO_REQUIRE(n > 0 && n < (int64_t)1 << 31, "geo_knn_query: n=%lld out of range", (long long)n);
    GEO_REQUIRE(m >= 0 && m < (int64_t)1 << 31, "geo_knn_query: m=%lld out of range", (long long)m);
    GEO_REQUIRE(d > 0 && d <= 128, "geo_knn_query: d=%d not in [1,128]", d);
    GEO_REQUIRE(n_neighbors > 0 && n_neighbors <= GEO_KNN_MAX_NEIGHBORS && n_neighbors <= n,
                "geo_knn_query: n_neighbors=%d not in [1, min(%d, n)]", n_neighbors, GEO_KNN_MAX_NEIGHBORS);
    if (m == 0) return GEO_OK;
    const KnnPlan p = plan_for(d);
    const size_t need = geo_knn_query_min_workspace_bytes(n, d);
    if (ws_bytes < need) {
        geo::set_error("geo_knn_query: workspace of %zu bytes is below the minimum of %zu", ws_bytes, need);
        return GEO_E_WORKSPACE;
    }
    // corpus side, prepared once for all slices
    geo::Arena ar(ws, ws_bytes);
    KnnCorpus c = {};
    c.n = n;
    const int S = filter_stride(n_neighbors);
    const bool filter_ws = filter_applies(n, p.dp);                       // what the workspace was sized for
    const bool filter = n_neighbors <= 64 && filter_ws && (n + S - 1) / S >= n_neighbors;
    KnnLists lists = {};
    const QueryCorpus qc = carve_query_corpus(ar, p, n, filter, n_neighbors, &c, &lists);
    if (!ar.ok()) {
        geo::set_error("geo_knn_query: workspace %zu too small (%zu needed)", ws_bytes, ar.off);
        return GEO_E_WORKSPACE;
    }
    const int64_t chunk = qc.chunk;
    double *nrm = qc.nrm, *z64_scratch = qc.z64_scratch;
    // the float32 scan reads its queries from the corpus array, so that ends flush with its block
    const size_t zp_bytes = (size_t)n * p.dp * sizeof(float);
    float *zp32 = qc.zp_block + (geo::align_up(zp_bytes) - zp_bytes) / sizeof(float);   // (a multiple of 32 bytes: dp >= 8)
    c.zp32 = zp32; c.nrm = nrm;
    // query side: slices of the rows that fit what is left
    size_t per_item[QUERY_BUFS];
    const int nb = query_per_item(p, filter_ws, per_item);
    int64_t slice = 0;
    float *bufs[QUERY_BUFS] = {};
    int rc = geo::plan_passes("geo_knn_query", per_item, nb, m, m, static_cast<char *>(ws) + ar.off, ws_bytes - ar.off, &slice, bufs);
    if (rc) return rc;
    float *qz32 = bufs[0];
    double *qz64 = reinterpret_cast<double *>(bufs[1]);
    double *nrm_q = reinterpret_cast<double *>(bufs[2]);
    unsigned short *zbq = filter ? reinterpret_cast<unsigned short *>(bufs[3]) : nullptr;
    float *negn_q = filter ? bufs[4] : nullptr;
    if (filter) {
        lists.u = reinterpret_cast<double *>(bufs[5]);
        lists.cnt = reinterpret_cast<int32_t *>(bufs[6]);
        lists.list = reinterpret_cast<int32_t *>(bufs[7]);
    }
    if (qz32 != zp32 + (size_t)n * p.dp) {
        geo::set_error("geo_knn_query: internal: the query rows do not continue the corpus array");
        return GEO_E_ARG;
    }
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t cr = n - c0 < chunk ? n - c0 : chunk;
        knn_prep_kernel<<<geo::grid_for(cr, 256, 4096), 256, 0, stream>>>(z + c0 * d, cr, d, p.dp, zp32 + c0 * p.dp, z64_scratch, nrm + c0);
        GEO_LAUNCH_CHECK();
    }
    if (filter) {
        rc = prepare_filter_corpus(p, c, stream);
        if (rc) return rc;
    }
    int32_t path_all = 0;
    for (int64_t s0 = 0; s0 < m; s0 += slice) {
        const int64_t rows = m - s0 < slice ? m - s0 : slice;
        knn_prep_kernel<<<geo::grid_for(rows, 256, 4096), 256, 0, stream>>>(q + s0 * d, rows, d, p.dp, qz32, qz64, nrm_q);
        GEO_LAUNCH_CHECK();
        if (filter && c.bf16_scan) {                           // the queries' bf16 parts: no padding rows (the scan clamps its queries)
            knn_split_kernel<<<geo::grid_for(rows * c.dpb, 256, 4096), 256, 0, stream>>>(qz32, nrm_q, rows, rows, p.dp, c.dpb, c.eps, zbq, negn_q);
            GEO_LAUNCH_CHECK();
        }
        const KnnQuery qs = {qz64, nrm_q, zbq, 0, rows, n};
        int32_t path = 0;
        rc = search_rows(p, form != 0, n_neighbors, c, qs, filter ? &lists : nullptr, idx_out + s0 * n_neighbors,
                         d2_out + s0 * n_neighbors, stream, &path);
        if (rc) return rc;
        // one answer for the call: a slice whose first level overflowed makes it the one-level path, any fallback sets the flag
        if (s0 == 0) path_all = path;
        else {
            const int32_t over = (path_all | path) & GEO_KNN_PATH_OVERFLOW;
            int32_t base = path_all & ~GEO_KNN_PATH_OVERFLOW;
            if ((path & ~GEO_KNN_PATH_OVERFLOW) != base) base = GEO_KNN_PATH_FILTER_BF16;
            path_all = base | over;
        }
    }
    g_last_path = path_all;
    return GEO_OK;
}

extern "C" int geo_knn_last_path(void) { return g_last_path; }

extern "C" int geo_knn_thresholds(const float *z, int64_t n, int32_t d, int32_t n_neighbors, int32_t form, int64_t row0,
                                  int64_t row1, int32_t stride, double *tau_out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(z && tau_out && ws, "geo_knn_thresholds: null pointer");
    GEO_REQUIRE(n > 0 && n < (int64_t)1 << 31, "geo_knn_thresholds: n=%lld out of range", (long long)n);
    GEO_REQUIRE(d > 0 && d <= 128, "geo_knn_thresholds: d=%d not in [1,128]", d);
    GEO_REQUIRE(stride >= 1, "geo_knn_thresholds: stride=%d", stride);
    const int64_t m = (n + stride - 1) / stride;
    GEO_REQUIRE(n_neighbors > 0 && n_neighbors <= 64 && n_neighbors <= m,
                "geo_knn_thresholds: n_neighbors=%d not in [1, min(64, subset rows)]", n_neighbors);
    GEO_REQUIRE(0 <= row0 && row0 <= row1 && row1 <= n, "geo_knn_thresholds: bad row range");
    if (row0 == row1) return GEO_OK;
    const KnnPlan p = plan_for(d);
    geo::Arena ar(ws, ws_bytes);
    const PlainCorpus pc = carve_plain_corpus(ar, p, n);
    float *zs32 = ar.take<float>((size_t)m * p.dp);             // the subset: every stride-th row
    double *nrm_s = ar.take<double>((size_t)m);
    if (!ar.ok()) {
        geo::set_error("geo_knn_thresholds: workspace %zu too small (%zu needed)", ws_bytes, ar.off);
        return GEO_E_WORKSPACE;
    }
    float *zp32 = pc.zp32;
    double *zq64 = pc.zq64, *nrm = pc.nrm;
    knn_prep_kernel<<<geo::grid_for(n, 256, 4096), 256, 0, stream>>>(z, n, d, p.dp, zp32, zq64, nrm);
    GEO_LAUNCH_CHECK();
    knn_subset_kernel<<<geo::grid_for(m * p.dp, 256, 4096), 256, 0, stream>>>(zp32, nrm, n, p.dp, stride, m, zs32, nrm_s);
    GEO_LAUNCH_CHECK();
    const KnnSide sub = {zs32, nrm_s, nullptr, nullptr, m};
    const KnnQuery q = {zq64, nrm, nullptr, row0, row1, row0};
    return launch_knn_bound(p, form != 0, n_neighbors, sub, q, 0.0, nullptr, nullptr, tau_out, stream);
}

// ---- nearest foreign node / component bridges -----------------------------------------------------------------------------------
namespace {

// few queries: one per wave fills more of the chip (and every wave's label is trivially uniform); many: 4, then 8 per wave.
// Not knn_kernel's 16: the gathered rows cost an address pair, a row number and a label in SGPRs per query, and at 16 the
// scalar registers spill -- measured on 74 679 / 217 456 queries of 960 000 x 16 / 800 000 x 32 latents, in 10^12 fp64 FMA/s:
// Q = 4: 6.9 / 6.8, Q = 8: 10.9 / 9.7, Q = 16: 9.1 / 6.7 (knn_kernel's exact scan of as many rows: 11.4 / 13.3).
int launch_nearest_foreign(const KnnPlan &p, bool ex, const PlainCorpus &c, int64_t n, const int32_t *labels, const int32_t *rows,
                           int64_t m, int32_t *nbr, double *key, hipStream_t s) {
    auto launch = [&](auto q_c) {
        constexpr int Q = decltype(q_c)::value;
        const int64_t waves = (m + Q - 1) / Q;
        const unsigned grid = (unsigned)((waves + KNN_WAVES - 1) / KNN_WAVES);
        with_key_form(p, ex, [&](auto dch, auto form) {
            nearest_foreign_kernel<decltype(dch)::value, Q, decltype(form)::value><<<grid, 256, 0, s>>>(
                c.zp32, c.zq64, c.nrm, labels, rows, m, n, p.nch, nbr, key);
        });
    };
    if (m <= 2048) launch(int_c<1>{});
    else if (m < 16384) launch(int_c<4>{});
    else launch(int_c<8>{});
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// geo_bridge_components' layout: the corpus and the Boruvka rounds' buffers
struct BridgeWs { PlainCorpus pc; int32_t *cur, *flag, *pos, *rows, *nbr, *sizes, *map; double *key; char *sel, *scan_tmp; size_t scan_bytes; };
BridgeWs carve_bridge(geo::Arena &ar, const KnnPlan &p, int64_t n, int32_t C) {
    const size_t n1 = (size_t)n + 1;
    BridgeWs o;
    o.pc = carve_plain_corpus(ar, p, n);
    ar.take(o.cur, n1); ar.take(o.flag, n1); ar.take(o.pos, n1); ar.take(o.rows, n1); ar.take(o.nbr, n1);
    ar.take(o.key, (size_t)n);
    ar.take(o.sel, (size_t)C * 20 + 64);         // what a round reads back, in one block: minkey u64 [C], minedge u64 [C], other i32 [C]
    ar.take(o.sizes, (size_t)C + 16);            // sizes [C], then the bad-label flag
    ar.take(o.map, (size_t)C + 16);
    o.scan_bytes = geo::scan_tmp_bytes(n + 1);
    ar.take(o.scan_tmp, o.scan_bytes);
    return o;
}

struct BridgeEdge {
    double key;
    int32_t lo, hi;
    bool operator<(const BridgeEdge &o) const {
        if (key != o.key) return key < o.key;
        if (lo != o.lo) return lo < o.lo;
        return hi < o.hi;
    }
};

int32_t uf_find(int32_t *par, int32_t a) {
    while (par[a] != a) { par[a] = par[par[a]]; a = par[a]; }
    return a;
}

}  // namespace

extern "C" size_t geo_nearest_foreign_workspace_bytes(int64_t n, int32_t d) {
    if (n <= 0 || d <= 0) return 1024;
    return geo::measure(carve_plain_corpus, plan_for(d), n) + FOREIGN_RESERVE;
}

extern "C" int geo_nearest_foreign(const float *z, int64_t n, int32_t d, int32_t form, const int32_t *labels, const int32_t *rows,
                                   int64_t m, int32_t *nbr_out, double *key_out, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(z && labels && rows && nbr_out && key_out && ws, "geo_nearest_foreign: null pointer");
    GEO_REQUIRE(n > 0 && n < (int64_t)1 << 31, "geo_nearest_foreign: n=%lld out of range", (long long)n);
    GEO_REQUIRE(m >= 0 && m < (int64_t)1 << 31, "geo_nearest_foreign: m=%lld out of range", (long long)m);
    GEO_REQUIRE(d > 0 && d <= 128, "geo_nearest_foreign: d=%d not in [1,128]", d);
    if (m == 0) return GEO_OK;
    const KnnPlan p = plan_for(d);
    geo::Arena ar(ws, ws_bytes);
    const PlainCorpus pc = carve_plain_corpus(ar, p, n);
    GEO_REQUIRE_WORKSPACE("geo_nearest_foreign", ar, geo_nearest_foreign_workspace_bytes(n, d));
    knn_prep_kernel<<<geo::grid_for(n, 256, 4096), 256, 0, stream>>>(z, n, d, p.dp, pc.zp32, pc.zq64, pc.nrm);
    GEO_LAUNCH_CHECK();
    return launch_nearest_foreign(p, form != 0, pc, n, labels, rows, m, nbr_out, key_out, stream);
}

extern "C" size_t geo_bridge_components_workspace_bytes(int64_t n, int32_t d, int32_t C) {
    if (n <= 0 || d <= 0 || C <= 0) return 1024;
    return geo::measure(carve_bridge, plan_for(d), n, C) + BRIDGE_RESERVE;
}

extern "C" int geo_bridge_components(const float *z, int64_t n, int32_t d, int32_t form, const int32_t *labels, int32_t C,
                                     int32_t *edges_out, double *keys_out, int32_t *status_out, void *ws, size_t ws_bytes,
                                     void *stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    GEO_REQUIRE(z && labels && edges_out && keys_out && status_out && ws, "geo_bridge_components: null pointer");
    GEO_REQUIRE(n > 0 && n < (int64_t)1 << 31, "geo_bridge_components: n=%lld out of range", (long long)n);
    GEO_REQUIRE(d > 0 && d <= 128, "geo_bridge_components: d=%d not in [1,128]", d);
    GEO_REQUIRE(C >= 1 && C <= n, "geo_bridge_components: C=%d not in [1, n]", C);
    const KnnPlan p = plan_for(d);
    geo::Arena ar(ws, ws_bytes);
    const BridgeWs w = carve_bridge(ar, p, n, C);
    GEO_REQUIRE_WORKSPACE("geo_bridge_components", ar, geo_bridge_components_workspace_bytes(n, d, C));
    float *zp32 = w.pc.zp32;
    double *zq64 = w.pc.zq64, *nrm = w.pc.nrm, *key = w.key;
    int32_t *cur = w.cur, *flag = w.flag, *pos = w.pos, *rows = w.rows, *nbr = w.nbr, *sizes = w.sizes, *map = w.map;
    char *sel = w.sel;
    void *st = w.scan_tmp;
    const size_t sb = w.scan_bytes;
    // the plan: labels in range, component sizes
    const int gn = geo::grid_for(n, 256, 4096);
    GEO_HIP_CHECK(hipMemsetAsync(sizes, 0, ((size_t)C + 1) * 4, stream));
    bridge_hist_kernel<<<gn, 256, 0, stream>>>(labels, n, C, cur, sizes, sizes + C);
    GEO_LAUNCH_CHECK();
    int32_t *h_sizes = static_cast<int32_t *>(malloc(((size_t)C + 1) * 4 * 3));      // sizes + bad, parents, map
    char *h_sel = static_cast<char *>(malloc((size_t)C * 20));
    BridgeEdge *found = static_cast<BridgeEdge *>(malloc(((size_t)C + 1) * 2 * sizeof(BridgeEdge)));
    struct Free { void *a, *b, *c; ~Free() { free(a); free(b); free(c); } } guard = {h_sizes, h_sel, found};
    if (!h_sizes || !h_sel || !found) {
        geo::set_error("geo_bridge_components: out of host memory");
        return GEO_E_ARG;
    }
    int32_t *par = h_sizes + (C + 1), *h_map = par + (C + 1);
    GEO_HIP_CHECK(hipMemcpyAsync(h_sizes, sizes, ((size_t)C + 1) * 4, hipMemcpyDeviceToHost, stream));
    GEO_HIP_CHECK(hipStreamSynchronize(stream));
    GEO_REQUIRE(h_sizes[C] == 0, "geo_bridge_components: a label lies outside [0, %d)", C);
    for (int32_t c = 0; c < C; ++c) GEO_REQUIRE(h_sizes[c] > 0, "geo_bridge_components: label %d does not occur", c);
    int32_t status[4] = {0, 0, 0, 0};
    int64_t n_found = 0;
    if (C > 1) {
        knn_prep_kernel<<<gn, 256, 0, stream>>>(z, n, d, p.dp, zp32, zq64, nrm);
        GEO_LAUNCH_CHECK();
    }
    int32_t cc = C;                                            // components left
    while (cc > 1) {
        int32_t big = 0;
        for (int32_t c = 1; c < cc; ++c)
            if (h_sizes[c] > h_sizes[big]) big = c;            // lowest label among the largest
        const int64_t m = n - h_sizes[big];
        bridge_flag_kernel<<<gn, 256, 0, stream>>>(cur, n, big, flag);
        GEO_LAUNCH_CHECK();
        if (int rc = geo::exclusive_scan_i32(flag, pos, n, st, sb, nullptr, stream)) return rc;
        bridge_rows_kernel<<<gn, 256, 0, stream>>>(flag, pos, n, rows);
        GEO_LAUNCH_CHECK();
        if (int rc = launch_nearest_foreign(p, form != 0, w.pc, n, cur, rows, m, nbr, key, stream)) return rc;
        unsigned long long *minkey = reinterpret_cast<unsigned long long *>(sel), *minedge = minkey + cc;
        int32_t *other = reinterpret_cast<int32_t *>(minedge + cc);
        GEO_HIP_CHECK(hipMemsetAsync(sel, 0xff, (size_t)cc * 20, stream));
        const int gm = geo::grid_for(m, 256, 4096);
        bridge_minkey_kernel<<<gm, 256, 0, stream>>>(cur, rows, key, m, minkey);
        GEO_LAUNCH_CHECK();
        bridge_minedge_kernel<<<gm, 256, 0, stream>>>(cur, rows, nbr, key, m, minkey, minedge);
        GEO_LAUNCH_CHECK();
        bridge_other_kernel<<<gm, 256, 0, stream>>>(cur, rows, nbr, key, m, minkey, minedge, other);
        GEO_LAUNCH_CHECK();
        GEO_HIP_CHECK(hipMemcpyAsync(h_sel, sel, (size_t)cc * 20, hipMemcpyDeviceToHost, stream));
        GEO_HIP_CHECK(hipStreamSynchronize(stream));
        status[0] += 1;
        if (status[0] == 1) status[1] = (int32_t)m;
        status[2] += (int32_t)m;
        const unsigned long long *h_minkey = reinterpret_cast<const unsigned long long *>(h_sel), *h_minedge = h_minkey + cc;
        const int32_t *h_other = reinterpret_cast<const int32_t *>(h_minedge + cc);
        for (int32_t c = 0; c < cc; ++c) par[c] = c;
        for (int32_t c = 0; c < cc; ++c) {
            if (c == big) continue;
            const int32_t o = h_other[c];
            if (o < 0 || o >= cc || o == c || h_minedge[c] == ~0ull) {
                geo::set_error("geo_bridge_components: internal: component %d found no foreign node", c);
                return GEO_E_ARG;
            }
            const int32_t ra = uf_find(par, c), rb = uf_find(par, o);
            if (ra != rb) {                                    // (equal: the other end chose the same edge earlier in this loop)
                if (ra < rb) par[rb] = ra; else par[ra] = rb;  // the root is the lowest label: numbering by lowest node stays
                long long kb = (long long)h_minkey[c];
                BridgeEdge e;
                memcpy(&e.key, &kb, 8);
                e.lo = (int32_t)(h_minedge[c] >> 32);
                e.hi = (int32_t)(h_minedge[c] & 0xffffffffu);
                found[n_found++] = e;
            }
        }
        int32_t next = 0;
        for (int32_t c = 0; c < cc; ++c)
            if (par[c] == c) h_map[c] = next++;
        for (int32_t c = 0; c < cc; ++c) {
            const int32_t r = uf_find(par, c);
            if (r != c) { h_map[c] = h_map[r]; h_sizes[r] += h_sizes[c]; }
        }
        for (int32_t c = 0; c < cc; ++c)
            if (par[c] == c) h_sizes[h_map[c]] = h_sizes[c];   // h_map[c] <= c: never overwrites a root still to be read
        GEO_HIP_CHECK(hipMemcpyAsync(map, h_map, (size_t)cc * 4, hipMemcpyHostToDevice, stream));
        bridge_relabel_kernel<<<gn, 256, 0, stream>>>(cur, n, map);
        GEO_LAUNCH_CHECK();
        GEO_HIP_CHECK(hipStreamSynchronize(stream));           // h_map is rewritten next round
        if (next >= cc) {
            geo::set_error("geo_bridge_components: internal: a round merged nothing");
            return GEO_E_ARG;
        }
        cc = next;
    }
    if (n_found != (int64_t)C - 1) {
        geo::set_error("geo_bridge_components: internal: %lld edges for %d components", (long long)n_found, C);
        return GEO_E_ARG;
    }
    if (C > 1) {
        std::sort(found, found + n_found);
        int32_t *h_edges = reinterpret_cast<int32_t *>(h_sel);           // 20 C bytes: 8 (C - 1) + 8 (C - 1) fit
        double *h_keys = reinterpret_cast<double *>(h_sel + (size_t)(C - 1) * 8);
        for (int64_t e = 0; e < n_found; ++e) { h_edges[2 * e] = found[e].lo; h_edges[2 * e + 1] = found[e].hi; h_keys[e] = found[e].key; }
        GEO_HIP_CHECK(hipMemcpyAsync(edges_out, h_edges, (size_t)(C - 1) * 8, hipMemcpyHostToDevice, stream));
        GEO_HIP_CHECK(hipMemcpyAsync(keys_out, h_keys, (size_t)(C - 1) * 8, hipMemcpyHostToDevice, stream));
        GEO_HIP_CHECK(hipStreamSynchronize(stream));
    }
    for (int i = 0; i < 4; ++i) status_out[i] = status[i];
    return GEO_OK;
}
