// prdc.hip -- kNN radii and ball membership for precision / recall / density / coverage of a generated sample set (gfx950).
//
// Two questions over all pairs of a query set and a corpus, both on THE KEY of include/geo_hip.h (geo_knn_query's form 0 chain:
// fp64 differences, one fma chain over the dimensions in ascending order):
//   geo_kth_radius  the k-th smallest key from each row to the other rows of its own set,
//   geo_ball_count  how many corpus balls (key <= r2[i]) hold each query, and the query's nearest corpus row.
// Widths go to 1024 (a flattened spatial mu), where knn.hip's wave-per-query mapping stops at 128: here a workgroup owns a
// tile of 64 query rows and walks the corpus 64 rows at a time, the dimensions staged through LDS 16 at a time as fp64
// (converted once per tile, not once per pair), every thread a 4 x 4 block of pair accumulators.  The chain of a pair stays in
// its register from dimension 0 to d-1: chunks continue it, nothing is split and re-added, so a key does not depend on the
// tiling.  Rows and dimensions past the end are staged as zeros (fma(0, 0, acc) = acc exactly) and masked in the epilogue.
//
// The corpus is cut into S contiguous tile ranges per query tile (grid.y) where the query tiles alone would not fill the chip.
// Every range writes its partial to the workspace -- also for S = 1: one path -- and prdc_fold_*_kernel fold the ranges in
// ascending order: integer sums, the lexicographic minimum of (key, index), the k smallest of a multiset.  None of the three
// depends on S or on the order of arrival, and there is no atomic anywhere.
#include "geo_common.h"

#include <climits>

namespace {

constexpr int TQ = 64, TZ = 64, DC = 16;       // query rows, corpus rows, dimensions per staged chunk
constexpr int LIST = GEO_PRDC_MAX_K;           // entries a row's list of smallest keys holds (one per lane of a wave)
constexpr int MAX_SPLIT = 32;
constexpr int TARGET_BLOCKS = 512;             // two workgroups for each of the 256 CUs
static_assert(LIST == 64 && TQ == 64 && TZ == 64, "a row's list and a row of the key tile are one register across a wave");

__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7ff0000000000000LL); }

__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Lane p of `lv` holds the p-th smallest key seen (ascending, +inf where none yet), tau = lane k-1.  The lanes of `cand` below
// tau are inserted one by one; their order does not matter to the values kept.  Returns the new tau.
__device__ __forceinline__ double list_insert(double &lv, double cand, double tau, int k, int lane) {
    unsigned long long hits = __ballot(cand < tau);
    while (hits) {
        const int src = __builtin_ctzll(hits);
        hits &= hits - 1;
        const double val = readlane_f64(cand, src);
        if (!(val < tau)) continue;                          // tau shrank since the ballot
        const int pos = __builtin_popcountll(__ballot(lv <= val));
        const double up = __shfl_up(lv, 1, 64);
        if (lane > pos) lv = up;
        if (lane == pos) lv = val;
        tau = readlane_f64(lv, k - 1);
    }
    return tau;
}

// up to four float32 coordinates of row `row` from dimension c on, zeros past the row's end and for row < 0
__device__ __forceinline__ float4 load_quad(const float *__restrict__ x, int64_t row, int d, int c, bool vec4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < 0 || c >= d) return v;
    const float *p = x + row * d + c;
    if (vec4) return *reinterpret_cast<const float4 *>(p);   // d % 4 == 0 and a 16-byte aligned base: c + 3 < d
    v.x = p[0];
    if (c + 1 < d) v.y = p[1];
    if (c + 2 < d) v.z = p[2];
    if (c + 3 < d) v.w = p[3];
    return v;
}

// partials of one slice, carved from the one buffer of lay(): RADIUS keeps LIST doubles per (range, row); COUNT its first
// doubles as key [S rows_pad], behind them idx and cnt as int32 [S rows_pad] each (16 of the 512 bytes per (range, row))
struct Partials {
    double *buf;
    int64_t rows_pad;
    int S;
    __host__ __device__ double *list(int s, int64_t r) const { return buf + ((int64_t)s * rows_pad + r) * LIST; }
    __host__ __device__ double *key() const { return buf; }
    __host__ __device__ int32_t *idx() const { return reinterpret_cast<int32_t *>(buf + (int64_t)S * rows_pad); }
    __host__ __device__ int32_t *cnt() const { return idx() + (int64_t)S * rows_pad; }
};

// RADIUS: q == z, self left out by index, the k smallest keys of each row.  !RADIUS: count against r2, nearest corpus row.
template <bool RADIUS>
__global__ __launch_bounds__(256) void prdc_pair_kernel(const float *__restrict__ q, int64_t row0, int64_t row1,
                                                        const float *__restrict__ z, const double *__restrict__ r2, int64_t n,
                                                        int d, int k, int vec4, Partials part) {
    __shared__ double stage[2][DC][64];                      // the chunk's query and corpus coordinates, [dimension][row]
    __shared__ double lists[RADIUS ? TQ : 1][LIST];          // RADIUS: each query's smallest keys so far, ascending
    __shared__ double taus[TQ];                              //         and its k-th
    double (*sq)[64] = stage[0], (*sz)[64] = stage[1];
    double (*keys)[TZ] = stage[0];                           //         the keys of 32 query rows of a finished tile (below)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid & 15, ty = tid >> 4;                  // pairs (query row 4 ty + a, corpus row tx + 16 b) of the tile
    const int64_t qbase = row0 + (int64_t)blockIdx.x * TQ;
    const int64_t ztiles = (n + TZ - 1) / TZ;
    const int64_t t0 = ztiles * blockIdx.y / gridDim.y, t1 = ztiles * (blockIdx.y + 1) / gridDim.y;
    const int nch = (d + DC - 1) / DC;

    if (RADIUS) {
        for (int i = tid; i < TQ * LIST; i += 256) (&lists[0][0])[i] = inf64();
        if (tid < TQ) taus[tid] = inf64();
    }
    int32_t cnt[4] = {0, 0, 0, 0}, best_i[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    double best[4] = {inf64(), inf64(), inf64(), inf64()};

    // staging: this thread converts four dimensions (4 wave + 0..3 of the chunk) of query row `lane` and corpus row `lane`
    const int64_t my_q = qbase + lane < row1 ? qbase + lane : -1;
    float4 fq = load_quad(q, my_q, d, 4 * wave, vec4);
    float4 fz;
    {
        const int64_t zr = t0 * TZ + lane;
        fz = load_quad(z, t0 < t1 && zr < n ? zr : -1, d, 4 * wave, vec4);
    }
    double acc[4][4];
    const int64_t steps = (t1 - t0) * nch;
    int64_t tile = t0;
    int ch = 0;
    for (int64_t s = 0; s < steps; ++s) {
        __syncthreads();                                     // the previous chunk's reads, the previous tile's epilogue
        sq[4 * wave + 0][lane] = (double)fq.x; sq[4 * wave + 1][lane] = (double)fq.y;
        sq[4 * wave + 2][lane] = (double)fq.z; sq[4 * wave + 3][lane] = (double)fq.w;
        sz[4 * wave + 0][lane] = (double)fz.x; sz[4 * wave + 1][lane] = (double)fz.y;
        sz[4 * wave + 2][lane] = (double)fz.z; sz[4 * wave + 3][lane] = (double)fz.w;
        __syncthreads();
        if (s + 1 < steps) {                                 // the next chunk's loads fly while this one is multiplied
            const bool wrap = ch + 1 == nch;
            const int c = (wrap ? 0 : (ch + 1) * DC) + 4 * wave;
            const int64_t zr = (wrap ? tile + 1 : tile) * TZ + lane;
            fq = load_quad(q, my_q, d, c, vec4);
            fz = load_quad(z, zr < n ? zr : -1, d, c, vec4);
        }
        if (ch == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
        }
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            double qv[4], zv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) qv[a] = sq[c][4 * ty + a];
#pragma unroll
            for (int b = 0; b < 4; ++b) zv[b] = sz[c][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double t = qv[a] - zv[b];
                    acc[a][b] = fma(t, t, acc[a][b]);
                }
        }
        if (++ch < nch) continue;
        ch = 0;
        // ---- the tile's keys are complete
        const int64_t zb = tile * TZ;
        ++tile;
        if (!RADIUS) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t j = zb + tx + 16 * b;
                if (j >= n) continue;
                const double rj = r2[j];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const double key = acc[a][b];
                    cnt[a] += key <= rj ? 1 : 0;
                    if (key < best[a] || (key == best[a] && (int32_t)j < best_i[a])) { best[a] = key; best_i[a] = (int32_t)j; }
                }
            }
        } else {
            bool hit = false;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int64_t i = qbase + 4 * ty + a;
                const double tau = taus[4 * ty + a];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int64_t j = zb + tx + 16 * b;
                    if (j >= n || j == i) acc[a][b] = inf64();
                    hit |= acc[a][b] < tau;
                }
            }
            if (__syncthreads_or(hit)) {                     // rare once the lists have seen a few tiles
                // The staged chunk is spent: its 16 KiB take the keys of 32 query rows at a time, rows 16 w + 8 h .. + 7 of
                // wave w in half h, which is the wave that owns them: wave w computed query rows 16 w .. 16 w + 15.
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const int row = 4 * ty + a;
                        if (((row >> 3) & 1) != h) continue;
#pragma unroll
                        for (int b = 0; b < 4; ++b) keys[8 * wave + (row & 7)][tx + 16 * b] = acc[a][b];
                    }
                    __syncthreads();
                    for (int rr = 0; rr < 8; ++rr) {
                        const int row = 16 * wave + 8 * h + rr;
                        const double cand = keys[8 * wave + rr][lane];
                        const double tau = taus[row];
                        if (!__ballot(cand < tau)) continue;
                        double lv = lists[row][lane];
                        const double now = list_insert(lv, cand, tau, k, lane);
                        lists[row][lane] = lv;
                        if (lane == 0) taus[row] = now;
                    }
                    __syncthreads();
                }
            }
        }
    }
    __syncthreads();
    if (RADIUS) {
        for (int rr = 0; rr < 16; ++rr) {
            const int row = 16 * wave + rr;
            if (qbase + row < row1) part.list(blockIdx.y, qbase - row0 + row)[lane] = lists[row][lane];
        }
    } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {         // the 16 lanes tx = 0..15 of one ty
                cnt[a] += __shfl_xor(cnt[a], off, 16);
                const double ok = __shfl_xor(best[a], off, 16);
                const int32_t oi = __shfl_xor(best_i[a], off, 16);
                if (ok < best[a] || (ok == best[a] && oi < best_i[a])) { best[a] = ok; best_i[a] = oi; }
            }
            const int64_t i = qbase + 4 * ty + a;
            if (tx == 0 && i < row1) {
                const int64_t at = (int64_t)blockIdx.y * part.rows_pad + (i - row0);
                part.key()[at] = best[a];
                part.idx()[at] = best_i[a];
                part.cnt()[at] = cnt[a];
            }
        }
    }
}

// the ranges of a slice folded in ascending order.  RADIUS: a wave per row; otherwise a thread per row.
__global__ __launch_bounds__(256) void prdc_fold_radius_kernel(Partials part, int64_t rows, int k, double *__restrict__ r2_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    double lv = part.list(0, r)[lane];
    double tau = readlane_f64(lv, k - 1);
    for (int s = 1; s < part.S; ++s) tau = list_insert(lv, part.list(s, r)[lane], tau, k, lane);
    if (lane == 0) r2_out[r] = tau;
}

__global__ __launch_bounds__(256) void prdc_fold_count_kernel(Partials part, int64_t rows, int32_t *__restrict__ count_out,
                                                             double *__restrict__ key_out, int32_t *__restrict__ idx_out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int32_t cnt = 0, bi = INT_MAX;
    double best = inf64();
    for (int s = 0; s < part.S; ++s) {
        const int64_t at = (int64_t)s * part.rows_pad + r;
        cnt += part.cnt()[at];
        const double key = part.key()[at];
        const int32_t i = part.idx()[at];
        if (key < best || (key == best && i < bi)) { best = key; bi = i; }
    }
    if (count_out) count_out[r] = cnt;
    if (key_out) key_out[r] = best;
    if (idx_out) idx_out[r] = bi;
}

int64_t pad_rows(int64_t rows) { return (rows + TQ - 1) / TQ * TQ; }

// corpus ranges for a slice of `rows` query rows: enough workgroups to fill the chip, or what the option asks for
int ranges_for(int64_t rows, int64_t n) {
    const int64_t qt = (rows + TQ - 1) / TQ, zt = (n + TZ - 1) / TZ;
    const int opt = geo::options().prdc_split;
    int64_t S = opt >= 1 ? opt : (TARGET_BLOCKS + qt - 1) / qt;
    if (S > MAX_SPLIT) S = MAX_SPLIT;
    if (S > zt) S = zt;
    return S < 1 ? 1 : (int)S;
}

// The one workspace layout: the partials of a slice of `rows` query rows in S ranges.
void lay(geo::Arena &ar, int64_t rows, int S, Partials *part) {
    part->rows_pad = pad_rows(rows);
    part->S = S;
    ar.take(part->buf, (size_t)part->rows_pad * S * LIST);
}
size_t lay_bytes(int64_t rows, int S) { Partials p; return geo::measure(lay, rows, S, &p); }

// The slice of query rows and its ranges that fit ws_bytes (>= the minimum): whole tiles, shrinking from all m rows; at one
// tile, fewer ranges.
void plan(int64_t n, int64_t m, size_t ws_bytes, int64_t *rows, int *S) {
    int64_t r = m;
    int s = ranges_for(r, n);
    while (lay_bytes(r, s) > ws_bytes && r > TQ) {
        const int64_t less = pad_rows(geo::shrink_pass(r));
        r = less < r ? less : r - TQ;
        if (r < TQ) r = TQ;
        s = ranges_for(r, n);
    }
    while (s > 1 && lay_bytes(r, s) > ws_bytes) --s;
    *rows = r;
    *S = s;
}

bool in_limits(int64_t n, int64_t m, int32_t d) {
    return d >= 1 && d <= 1024 && n >= 1 && n < (int64_t)1 << 31 && m >= 0 && m < (int64_t)1 << 31;
}

template <bool RADIUS>
int run(const char *who, const float *q, int64_t m, const float *z, const double *r2, int64_t n, int32_t d, int32_t k,
        double *r2_out, int32_t *count_out, double *key_out, int32_t *idx_out, void *ws, size_t ws_bytes, hipStream_t stream) {
    if (m == 0) return GEO_OK;                               // nothing to do: the workspace is not looked at
    const size_t need = geo_prdc_min_workspace_bytes(d);
    if (ws_bytes < need) {
        geo::set_error("%s: workspace of %zu bytes is below the minimum of %zu", who, ws_bytes, need);
        return GEO_E_WORKSPACE;
    }
    int64_t slice;
    int S;
    plan(n, m, ws_bytes, &slice, &S);
    geo::Arena ar(ws, ws_bytes);
    Partials part;
    lay(ar, slice, S, &part);
    GEO_REQUIRE_WORKSPACE("geo_prdc", ar, ar.off);
    const int vec4 = d % 4 == 0 && (uintptr_t)q % 16 == 0 && (uintptr_t)z % 16 == 0;
    for (int64_t row0 = 0; row0 < m; row0 += slice) {
        const int64_t row1 = row0 + slice < m ? row0 + slice : m, rows = row1 - row0;
        const dim3 grid((unsigned)((rows + TQ - 1) / TQ), (unsigned)S);
        prdc_pair_kernel<RADIUS><<<grid, 256, 0, stream>>>(q, row0, row1, z, r2, n, d, k, vec4, part);
        GEO_LAUNCH_CHECK();
        if (RADIUS)
            prdc_fold_radius_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, stream>>>(part, rows, k, r2_out + row0);
        else
            prdc_fold_count_kernel<<<(unsigned)((rows + 255) / 256), 256, 0, stream>>>(
                part, rows, count_out ? count_out + row0 : nullptr, key_out ? key_out + row0 : nullptr,
                idx_out ? idx_out + row0 : nullptr);
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}

}  // namespace

extern "C" size_t geo_prdc_min_workspace_bytes(int32_t d) {
    return d >= 1 && d <= 1024 ? lay_bytes(TQ, 1) : 0;
}

extern "C" size_t geo_prdc_workspace_bytes(int64_t n, int64_t m, int32_t d) {
    if (!in_limits(n, m, d)) return 0;
    const int64_t rows = m < 1 ? 1 : m;
    return lay_bytes(rows, ranges_for(rows, n));
}

extern "C" int geo_kth_radius(const float *a, int64_t n, int32_t d, int32_t k, double *r2_out, void *ws, size_t ws_bytes,
                              void *stream) {
    GEO_REQUIRE(a && r2_out && ws, "geo_kth_radius: null pointer");
    GEO_REQUIRE(in_limits(n, n, d), "geo_kth_radius: n=%lld, d=%d outside 1 <= n < 2^31, 1 <= d <= 1024", (long long)n, d);
    GEO_REQUIRE(k >= 1 && k <= GEO_PRDC_MAX_K && k <= n - 1, "geo_kth_radius: k=%d not in [1, min(%d, n - 1)]", k, GEO_PRDC_MAX_K);
    return run<true>("geo_kth_radius", a, n, a, nullptr, n, d, k, r2_out, nullptr, nullptr, nullptr, ws, ws_bytes,
                     static_cast<hipStream_t>(stream));
}

extern "C" int geo_ball_count(const float *z, const double *r2, int64_t n, const float *q, int64_t m, int32_t d,
                              int32_t *count_out, double *near_key_out, int32_t *near_idx_out, void *ws, size_t ws_bytes,
                              void *stream) {
    GEO_REQUIRE(z && r2 && ws && (q || m == 0), "geo_ball_count: null pointer");
    GEO_REQUIRE(in_limits(n, m, d), "geo_ball_count: n=%lld, m=%lld, d=%d outside 1 <= n < 2^31, 0 <= m < 2^31, 1 <= d <= 1024",
                (long long)n, (long long)m, d);
    return run<false>("geo_ball_count", q, m, z, r2, n, d, 0, nullptr, count_out, near_key_out, near_idx_out, ws, ws_bytes,
                      static_cast<hipStream_t>(stream));
}
