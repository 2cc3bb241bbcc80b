// jvp.hip -- decoder pull-back edge lengths by forward-mode tangent propagation (gfx950).
//
// Replaces torch.autograd.functional.jvp through SpatialDecoder in the reference
// (src/geo/riemannian_metric.py:12-35,37-66 over src/models/spatial_vae.py:47-81):
//     len[e] = 0.5 * ( |J(z_i) dz| + |J(z_j) dz| ),  dz = z_j - z_i,  J = d sigmoid(decoder(z)) / dz
// with the decoder applied to a 1x1 latent "image":
//     conv1x1(d->c0) -> ConvT(c0->c1,k4,s2,p1): 1x1 -> 2x2 -> norm -> ReLU
//                    -> ConvT(c1->c2,k4,s2,p1): 2x2 -> 4x4 -> norm -> ReLU
//                    -> ConvT(c2->co,k4,s2,p=3|1): 4x4 -> 4x4 | 8x8 -> sigmoid.
// The tangent is pushed through next to the primal (one pass instead of autograd's forward +
// double backward).  Edges are processed in chunks of `batch_size` consecutive edges; each
// (chunk, endpoint side) is one BatchNorm batch, exactly the batches riemannian_metric.py:50-58
// feeds to the decoder, so train-mode batch statistics see the same samples.
//
// Kernels (activations: [slot][pixel][channel], slot = padded sample position) and the route that picks them (make_route, once
// per call; geo_jvp_plan reports it):
//   front  pre1 = z . M01 + b01, M01 = conv_in o ConvT1 composed once in fp64; per-tile partial BN sums in fp64.
//            front_kernel (VALU)   d <= 16, or jvp_front_valu
//            front_edge_kernel     the VALU front on the dedup route (jvp_front_once): one workgroup per tile of edges, the
//                                  tangent row once per edge, the start-side primal row once per run of equal src
//            front_mfma_kernel     d > 16: v_mfma_f32_32x32x2_f32, the same k-ordered fmaf chain
//   mid    ConvT2 as a block-sparse product over (input pixel -> output pixel) blocks on the bf16 matrix cores (f32 operands split
//          exactly into three bf16 parts); prologue = norm1 + ReLU while staging A into LDS; epilogue = bias, store, BN sums.
//            mid_pipe_kernel       PIPE: 256-128-64 with BatchNorm / no norm, persistent and skewed over the tiles; with dedup
//                                  over the end side only, mid_start_kernel runs the start side once per run of equal src
//            mid_all_kernel        ALL: c2 = 64 otherwise (GroupNorm, c1 = 64 / 32, jvp_mid = 3), one tile per workgroup;
//                                  ALL_TANGENT: tangent only, behind the per-node primal pass
//            mid_bf16_kernel       CHUNK: c2 != 64 or jvp_mid = 2, one workgroup per (tile, chunk of output pixels)
//   back   norm2 + ReLU, ConvT3, sigmoid', squared norm per sample.
//            back_mfma_kernel      c2 = 64 and 16 or 192 outputs: MODE 0 primal + tangent; MODE 2 then 1: the primal rows once
//                                  (per latent: per_node; per run of equal src: dedup), then the tangents
//            head_stream_kernel    the 16-output head without GroupNorm, per slot and the dedup route's end side / start tangents
//                                  (jvp_head_stream): back_mfma_kernel's arithmetic with the next K block's rows in flight
//            back_kernel (VALU)    every other head, or jvp_back_valu
//   node_jacobian: the per_node kernels over unit tangents, then jacobian_lengths_kernel.
//   geo_decoder_metric_tensor: the same column pass over slices of latents, then jacobian_gram_kernel (G = J^T J per latent, fp64)
//                              and metric_spectrum_kernel (eigenvalues, rank, 0.5 log det G) -- DESIGN.md section 24.
//   geo_curve_energy / geo_curve_relax: the per-node primal pass and the column pass over slices of whole curves, then
//                              curve_reduce_kernel (energy, gradient, trace per curve, fp64) and curve_step_kernel (the accept /
//                              reject decision and the next trial, per curve on the device) -- DESIGN.md section 26.
#include "geo_common.h"
#include "curve_step.h"

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

namespace {

constexpr int TS = 32;          // samples per tile (= one 32-row MFMA slice for primal, one for tangent)
constexpr int NC = 128;         // output columns per mid-kernel workgroup (4 waves x 32)
constexpr int MAX_BLOCKS = 4;   // input pixels feeding one output pixel (2x2 input)
constexpr int FRONT_MAX_N1 = 1024;   // columns of the first pre-activation (4 pixels x c1 <= 256 channels)
constexpr int BACK_TS = 8;      // samples per back-kernel workgroup

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

struct Shape {
    int d, c0, c1, c2, co, s_out, pad3, p_out;   // p_out = co * s_out * s_out
    int n1, n2;                                   // 4*c1, 16*c2
    int opix_per_chunk, n_chunks;
};

struct ChunkTable {
    int nblk[16];
    int ipix[16][MAX_BLOCKS];
    int opix[16][16];
};

// prologue constants per (stat row, channel): y = (x - mu) * sc + beta ; t' = sc * (t - mt - (x - mu) * c5)
struct NormConst { float mu, sc, beta, mt, c5; };

// ---------------------------------------------------------------------------------- weight prep
// M01[k][n], n = px*c1 + co, px = oy*2+ox: composition of conv_in and ConvT1 (taps ky=oy+1,kx=ox+1)
__global__ __launch_bounds__(256) void compose_front_kernel(const float *__restrict__ w_in, const float *__restrict__ b_in,
                                                           const float *__restrict__ w1, const float *__restrict__ b1,
                                                           int d, int c0, int c1, float *__restrict__ M01,
                                                           float *__restrict__ b01) {
    const int n1 = 4 * c1;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (d + 1) * n1; i += gridDim.x * blockDim.x) {
        const int k = i / n1, n = i % n1;
        const int px = n / c1, co = n % c1;
        const int ky = (px >> 1) + 1, kx = (px & 1) + 1;
        double s = 0.0;
        for (int c8 = 0; c8 < c0; c8 += 8) {               // 16 strided loads in flight, then the fma chain in ci order
            float m1[8], a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ci = c8 + j < c0 ? c8 + j : c0 - 1;
                m1[j] = w1[(((size_t)ci * c1 + co) * 4 + ky) * 4 + kx];
                a[j] = k < d ? w_in[(size_t)ci * d + k] : b_in[ci];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c8 + j < c0) s = fma((double)a[j], (double)m1[j], s);
        }
        if (k < d) M01[(size_t)k * n1 + n] = (float)s;
        else b01[n] = (float)(s + (double)b1[co]);
    }
}

// B2p[chunk][blk][k = ci][col], col = local output pixel * c2 + co; zero where the tap is out of range
__global__ __launch_bounds__(256) void pack_mid_kernel(const float *__restrict__ w2, int c1, int c2, ChunkTable tab,
                                                      int n_chunks, int opix_per_chunk, float *__restrict__ B2p) {
    const size_t per_blk = (size_t)c1 * NC;
    const size_t total = (size_t)n_chunks * MAX_BLOCKS * per_blk;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % NC);
        const int ci = (int)((i / NC) % c1);
        const int blk = (int)((i / per_blk) % MAX_BLOCKS);
        const int ch = (int)(i / (per_blk * MAX_BLOCKS));
        float v = 0.0f;
        const int lo = col / c2, co = col % c2;
        if (blk < tab.nblk[ch] && lo < opix_per_chunk) {
            const int op = tab.opix[ch][lo], ip = tab.ipix[ch][blk];
            const int ky = (op >> 2) + 1 - 2 * (ip >> 1), kx = (op & 3) + 1 - 2 * (ip & 1);
            if (ky >= 0 && ky < 4 && kx >= 0 && kx < 4) v = w2[(((size_t)ci * c2 + co) * 4 + ky) * 4 + kx];
        }
        B2p[i] = v;
    }
}

// W3p[ky][kx][co][ci]
__global__ __launch_bounds__(256) void pack_back_kernel(const float *__restrict__ w3, int c2, int co_n,
                                                       float *__restrict__ W3p) {
    const int total = 16 * co_n * c2;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int ci = i % c2, co = (i / c2) % co_n, t = i / (c2 * co_n);
        W3p[i] = w3[(((size_t)ci * co_n + co) * 4 + (t >> 2)) * 4 + (t & 3)];
    }
}

// ---------------------------------------------------------------------------------- front
// One workgroup = one tile of TS sample slots.  Thread owns output columns n = tid + 256*j for
// all TS samples, so per-column sums need no cross-thread reduction.
template <int DMAX>
__global__ __launch_bounds__(256) void front_kernel(const float *__restrict__ z, const int32_t *__restrict__ src,
                                                   const int32_t *__restrict__ dst, const float *__restrict__ z_start,
                                                   const float *__restrict__ z_end, int64_t e_base, int64_t n_edges,
                                                   int batch, int tiles_per_group, int d, int n1,
                                                   const float *__restrict__ M01, const float *__restrict__ b01,
                                                   float *__restrict__ pre, float *__restrict__ tpre,
                                                   double *__restrict__ partial, int want_stats, int unit_d = 0) {
    // unit_d > 0 (per-latent Jacobians, run_node_jacobian): "edge" e is (latent pair e / unit_d, latent dimension e % unit_d);
    // the tangent of both sides is the unit vector of that dimension instead of the latent difference.
    // [latent dimension][sample]: two neighbouring samples of a dimension are one 8-byte broadcast read feeding one packed fma
    __shared__ __attribute__((aligned(8))) float zp[DMAX][TS];
    __shared__ __attribute__((aligned(8))) float dz[DMAX][TS];
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    __shared__ int valid_s[TS];
    __shared__ double ps[FRONT_MAX_N1][4];                  // per-column statistics before the pixel reduction
    const int tile = blockIdx.x;
    const int group = tile / tiles_per_group, tg = tile % tiles_per_group;
    const int chunk = group >> 1, side = group & 1;
    for (int i = threadIdx.x; i < TS * d; i += 256) {
        const int s = i / d, k = i % d;
        const int within = tg * TS + s;
        const int64_t e = e_base + (int64_t)chunk * batch + within;
        float a = 0.f, b = 0.f;
        const bool ok = within < batch && e < n_edges;
        if (ok) {
            if (src) {
                a = z[(int64_t)src[e] * d + k];
                b = z[(int64_t)dst[e] * d + k];
            } else {
                a = z_start[e * d + k];
                b = z_end[e * d + k];
            }
        }
        zp[k][s] = side == 0 ? a : b;
        dz[k][s] = unit_d ? ((ok && k == (int)(e % unit_d)) ? 1.f : 0.f) : b - a;
        if (k == 0) valid_s[s] = ok ? 1 : 0;
    }
    for (int i = threadIdx.x; i < TS * (DMAX - d); i += 256) {      // padded latent columns: zeros, not stale LDS
        const int s = i / (DMAX - d), k = d + i % (DMAX - d);
        zp[k][s] = 0.f;
        dz[k][s] = 0.f;
    }
    __syncthreads();
    const size_t slot0 = (size_t)tile * TS;
    for (int n = threadIdx.x; n < n1; n += 256) {
        float m[DMAX];
#pragma unroll
        for (int k = 0; k < DMAX; ++k) m[k] = k < d ? M01[(size_t)k * n1 + n] : 0.f;
        const float bias = b01[n];
        double sx = 0, sxx = 0, st = 0, sxt = 0;
        for (int s = 0; s < TS; s += 2) {                      // two samples per packed fma (v_pk_fma_f32): the same fmaf chains
            f32x2 x2 = {bias, bias}, t2 = {0.f, 0.f};
#pragma unroll
            for (int k = 0; k < DMAX; ++k) {
                const f32x2 mk = {m[k], m[k]};
                x2 = __builtin_elementwise_fma(*reinterpret_cast<const f32x2 *>(&zp[k][s]), mk, x2);
                t2 = __builtin_elementwise_fma(*reinterpret_cast<const f32x2 *>(&dz[k][s]), mk, t2);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float x = u ? x2.y : x2.x, t = u ? t2.y : t2.x;
                pre[(slot0 + s + u) * n1 + n] = x;
                tpre[(slot0 + s + u) * n1 + n] = t;
                if (valid_s[s + u]) {
                    sx += x; sxx += (double)x * x; st += t; sxt += (double)x * t;
                }
            }
        }
        if (want_stats) { ps[n][0] = sx; ps[n][1] = sxx; ps[n][2] = st; ps[n][3] = sxt; }
    }
    if (want_stats) {                                       // the four pixels of a channel, in pixel order: [tile][c1][4]
        __syncthreads();
        const int c1 = n1 / 4;
        for (int c = threadIdx.x; c < c1; c += 256) {
            double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
            for (int px = 0; px < 4; ++px) { a0 += ps[px * c1 + c][0]; a1 += ps[px * c1 + c][1]; a2 += ps[px * c1 + c][2]; a3 += ps[px * c1 + c][3]; }
            double *p = partial + ((size_t)tile * c1 + c) * 4;
            p[0] = a0; p[1] = a1; p[2] = a2; p[3] = a3;
        }
    }
}

// A start slot opens a run of equal src (jvp_start_dedup): the one rule behind start_runs_kernel's rep[] and the start-side primal
// rows front_edge_kernel keeps.  `within` = the slot's position in its chunk, e = its (valid) edge.
__device__ __forceinline__ bool start_run_head(const int32_t *__restrict__ src, int64_t e, int within) {
    return within == 0 || src[e] != src[e - 1];
}

// The first layer once per EDGE (jvp_front_once: train-mode BatchNorm over graph edges with the start-side dedup, c1 = 128).
// One workgroup = one tile of TS edges = start tile (chunk, 0, tg) and end tile (chunk, 1, tg) of front_kernel.  The tangent
// dz . M01 is the same row on both sides of an edge, and the start-side primal is the same row for every slot of a run of equal
// src, so of the four rows per edge only these reach memory (pre / tpre keep their slot-indexed layout):
//     pre, tpre of the END slot;  pre of a START slot that heads a run (start_run_head: the rows rep[] points at).
// Nothing on this route reads any other start-side row of pre1 / tpre1: mid_start_kernel<false> gathers pre1 through rep[],
// mid_start_kernel<true, true> takes the primal from rep[row_map[slot]] and the tangent from the partner end slot,
// mid_pipe_kernel<true> walks the end tiles only, and ConvT3 (back_mfma_kernel) reads pre2 / tpre2 (it reuses pre1 as sg_compact,
// written before read).  The unwritten rows hold whatever the last pass left.
// Same fmaf chains as front_kernel (bias first, k ascending; v_pk_fma_f32 over two samples), now three per sample pair -- end
// primal, start primal, tangent -- and over the thread's TWO columns at once: one LDS broadcast read feeds two packed FMAs
// (front_kernel is bound by those reads, one per FMA).  BN1 partial sums of both tiles in front_kernel's association (per column
// the samples ascending under `valid`, then the four pixels in order) into the same partial[tile][c1][4] entries: bit-identical.
constexpr int FRONT_EDGE_N1 = 512;   // 4 pixels x c1 = 128: the only width of the dedup route (mid_pipe_kernel)
template <int DMAX>
__global__ __launch_bounds__(256) void front_edge_kernel(const float *__restrict__ z, const int32_t *__restrict__ src,
                                                        const int32_t *__restrict__ dst, int64_t e_base, int64_t n_edges,
                                                        int batch, int tiles_per_group, int d, const float *__restrict__ M01,
                                                        const float *__restrict__ b01, float *__restrict__ pre,
                                                        float *__restrict__ tpre, double *__restrict__ partial) {
    constexpr int N1 = FRONT_EDGE_N1, C1 = N1 / 4;
    constexpr int NCOL = DMAX == 16 ? 2 : 1;                // columns a thread runs together (wider latents: registers)
    __shared__ __attribute__((aligned(8))) float za[DMAX][TS];   // [latent dimension][sample], as front_kernel
    __shared__ __attribute__((aligned(8))) float zb[DMAX][TS];
    __shared__ __attribute__((aligned(8))) float dz[DMAX][TS];
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    __shared__ int valid_s[TS], head_s[TS];
    __shared__ double ps[2][N1][4];                         // [side][column]: statistics before the pixel reduction
    const int chunk = blockIdx.x / tiles_per_group, tg = blockIdx.x % tiles_per_group;
    const size_t tile_s = (size_t)(2 * chunk) * tiles_per_group + tg, tile_e = tile_s + tiles_per_group;
    for (int i = threadIdx.x; i < TS * d; i += 256) {
        const int s = i / d, k = i % d;
        const int within = tg * TS + s;
        const int64_t e = e_base + (int64_t)chunk * batch + within;
        float a = 0.f, b = 0.f;
        const bool ok = within < batch && e < n_edges;
        if (ok) {
            a = z[(int64_t)src[e] * d + k];
            b = z[(int64_t)dst[e] * d + k];
        }
        za[k][s] = a;
        zb[k][s] = b;
        dz[k][s] = b - a;
        if (k == 0) {
            valid_s[s] = ok ? 1 : 0;
            head_s[s] = ok && start_run_head(src, e, within) ? 1 : 0;
        }
    }
    for (int i = threadIdx.x; i < TS * (DMAX - d); i += 256) {      // padded latent columns: zeros, not stale LDS
        const int s = i / (DMAX - d), k = d + i % (DMAX - d);
        za[k][s] = 0.f;
        zb[k][s] = 0.f;
        dz[k][s] = 0.f;
    }
    __syncthreads();
    float *__restrict__ pre_s = pre + tile_s * TS * N1;
    float *__restrict__ pre_e = pre + tile_e * TS * N1;
    float *__restrict__ tpre_e = tpre + tile_e * TS * N1;
    for (int n0 = threadIdx.x; n0 < N1; n0 += 256 * NCOL) {
        float m[NCOL][DMAX], bias[NCOL];
#pragma unroll
        for (int c = 0; c < NCOL; ++c) {
#pragma unroll
            for (int k = 0; k < DMAX; ++k) m[c][k] = k < d ? M01[(size_t)k * N1 + n0 + 256 * c] : 0.f;
            bias[c] = b01[n0 + 256 * c];
        }
        double se[NCOL][4], ss[NCOL][4];                    // sx, sxx, st, sxt of the end / start tile
#pragma unroll
        for (int c = 0; c < NCOL; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) { se[c][j] = 0; ss[c][j] = 0; }
        for (int s = 0; s < TS; s += 2) {
            f32x2 xe[NCOL], xs[NCOL], t2[NCOL];
#pragma unroll
            for (int c = 0; c < NCOL; ++c) { xe[c] = {bias[c], bias[c]}; xs[c] = {bias[c], bias[c]}; t2[c] = {0.f, 0.f}; }
#pragma unroll
            for (int k = 0; k < DMAX; ++k) {
                const f32x2 a2 = *reinterpret_cast<const f32x2 *>(&za[k][s]);
                const f32x2 b2 = *reinterpret_cast<const f32x2 *>(&zb[k][s]);
                const f32x2 d2 = *reinterpret_cast<const f32x2 *>(&dz[k][s]);
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    const f32x2 mk = {m[c][k], m[c][k]};
                    xe[c] = __builtin_elementwise_fma(b2, mk, xe[c]);
                    xs[c] = __builtin_elementwise_fma(a2, mk, xs[c]);
                    t2[c] = __builtin_elementwise_fma(d2, mk, t2[c]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bool valid = valid_s[s + u] != 0, head = head_s[s + u] != 0;     // (workgroup-uniform)
#pragma unroll
                for (int c = 0; c < NCOL; ++c) {
                    const size_t o = (size_t)(s + u) * N1 + n0 + 256 * c;
                    const float x = u ? xe[c].y : xe[c].x, y = u ? xs[c].y : xs[c].x, t = u ? t2[c].y : t2[c].x;
                    pre_e[o] = x;
                    tpre_e[o] = t;
                    if (head) pre_s[o] = y;
                    if (valid) {
                        se[c][0] += x; se[c][1] += (double)x * x; se[c][2] += t; se[c][3] += (double)x * t;
                        ss[c][0] += y; ss[c][1] += (double)y * y; ss[c][2] += t; ss[c][3] += (double)y * t;
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NCOL; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) { ps[0][n0 + 256 * c][j] = ss[c][j]; ps[1][n0 + 256 * c][j] = se[c][j]; }
    }
    __syncthreads();                                        // the four pixels of a channel, in pixel order: [tile][c1][4]
    {
        const int side = threadIdx.x / C1, c = threadIdx.x % C1;        // 256 threads = 2 sides x C1 channels
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            a0 += ps[side][px * C1 + c][0]; a1 += ps[side][px * C1 + c][1]; a2 += ps[side][px * C1 + c][2]; a3 += ps[side][px * C1 + c][3];
        }
        double *p = partial + ((side ? tile_e : tile_s) * C1 + c) * 4;
        p[0] = a0; p[1] = a1; p[2] = a2; p[3] = a3;
    }
}

// The same product on the float32 matrix cores for wide latents (d > 16: the VALU kernel spends 2 x d FMAs per value,
// 7.3 ms of the 50 000 x 64 configuration's step).  v_mfma_f32_32x32x2_f32 is a k-ordered fmaf chain into the accumulator,
// which starts at the bias: bit for bit the chain of front_kernel (x = bias; x = fmaf(z_k, m_k, x), k ascending).
// One wave = 32 samples x 32 columns at a time (primal and tangent accumulators), a workgroup = 4 waves over the n1 / 32
// column tiles; A (latents, differences) from LDS, B (M01) from L2; statistics from the accumulators (lane = column).
template <int DMAX>
__global__ __launch_bounds__(256) void front_mfma_kernel(const float *__restrict__ z, const int32_t *__restrict__ src,
                                                        const int32_t *__restrict__ dst, const float *__restrict__ z_start,
                                                        const float *__restrict__ z_end, int64_t e_base, int64_t n_edges,
                                                        int batch, int tiles_per_group, int d, int n1,
                                                        const float *__restrict__ M01, const float *__restrict__ b01,
                                                        float *__restrict__ pre, float *__restrict__ tpre,
                                                        double *__restrict__ partial, int want_stats) {
    __shared__ float zp[TS][DMAX + 1];
    __shared__ float dz[TS][DMAX + 1];
    __shared__ int valid_s[TS];
    __shared__ double ps[FRONT_MAX_N1][4];
    const int tile = blockIdx.x;
    const int group = tile / tiles_per_group, tg = tile % tiles_per_group;
    const int chunk = group >> 1, side = group & 1;
    for (int i = threadIdx.x; i < TS * DMAX; i += 256) {
        const int s = i / DMAX, k = i % DMAX;
        const int within = tg * TS + s;
        const int64_t e = e_base + (int64_t)chunk * batch + within;
        float a = 0.f, b = 0.f;
        const bool ok = within < batch && e < n_edges;
        if (ok && k < d) {
            if (src) {
                a = z[(int64_t)src[e] * d + k];
                b = z[(int64_t)dst[e] * d + k];
            } else {
                a = z_start[e * d + k];
                b = z_end[e * d + k];
            }
        }
        zp[s][k] = side == 0 ? a : b;
        dz[s][k] = b - a;
        if (k == 0) valid_s[s] = ok ? 1 : 0;
    }
    __syncthreads();
    const size_t slot0 = (size_t)tile * TS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    for (int ct = wave; ct * 32 < n1; ct += 4) {
        const int n = ct * 32 + r;                              // this lane's column
        f32x16 accp, acct;
        const float bias = b01[n];
#pragma unroll
        for (int q = 0; q < 16; ++q) { accp[q] = bias; acct[q] = 0.f; }
#pragma unroll 8
        for (int i = 0; i < DMAX / 2; ++i) {
            const int k = 2 * i + h;
            const float bm = k < d ? M01[(size_t)k * n1 + n] : 0.f;
            accp = __builtin_amdgcn_mfma_f32_32x32x2f32(zp[r][k], bm, accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[r][k], bm, acct, 0, 0, 0);
        }
        double sx = 0, sxx = 0, st = 0, sxt = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
            const float x = accp[q], t = acct[q];
            pre[(slot0 + row) * n1 + n] = x;
            tpre[(slot0 + row) * n1 + n] = t;
            if (valid_s[row]) { sx += x; sxx += (double)x * x; st += t; sxt += (double)x * t; }
        }
        if (want_stats) {
            sx += __shfl_xor(sx, 32, 64); sxx += __shfl_xor(sxx, 32, 64);
            st += __shfl_xor(st, 32, 64); sxt += __shfl_xor(sxt, 32, 64);
            if (lane < 32) { ps[n][0] = sx; ps[n][1] = sxx; ps[n][2] = st; ps[n][3] = sxt; }
        }
    }
    if (want_stats) {                                       // the four pixels of a channel, in pixel order: [tile][c1][4]
        __syncthreads();
        const int c1 = n1 / 4;
        for (int c = threadIdx.x; c < c1; c += 256) {
            double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
            for (int px = 0; px < 4; ++px) { a0 += ps[px * c1 + c][0]; a1 += ps[px * c1 + c][1]; a2 += ps[px * c1 + c][2]; a3 += ps[px * c1 + c][3]; }
            double *p = partial + ((size_t)tile * c1 + c) * 4;
            p[0] = a0; p[1] = a1; p[2] = a2; p[3] = a3;
        }
    }
}

// ---------------------------------------------------------------------------------- norm constants
// mode 1 (batch statistics): reduce the per-tile partial sums of a group over tiles and pixels.
// partial: [tile][npx_stored*C][4] fp64 (npx_stored = 1 when the producer summed a tile's pixels).  consts: [group][C].
__global__ __launch_bounds__(256) void finalize_batch_kernel(const double *__restrict__ partial, int tiles_per_group,
                                                            int npx_stored, int npx, int C, int64_t e_base, int64_t n_edges,
                                                            int batch, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, float eps,
                                                            NormConst *__restrict__ consts, int n_groups,
                                                            float2 *__restrict__ stats_out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_groups * C; i += gridDim.x * blockDim.x) {
        const int g = i / C, c = i % C;
        const int chunk = g >> 1;
        int64_t cnt = n_edges - (e_base + (int64_t)chunk * batch);
        if (cnt > batch) cnt = batch;
        if (cnt < 0) cnt = 0;
        double sx = 0, sxx = 0, st = 0, sxt = 0;
        for (int t = 0; t < tiles_per_group; ++t)
            for (int px = 0; px < npx_stored; ++px) {      // (1 when the producing kernel already summed a tile's pixels)
                const double *p = partial + (((size_t)(g * tiles_per_group + t)) * npx_stored * C + (size_t)px * C + c) * 4;
                sx += p[0]; sxx += p[1]; st += p[2]; sxt += p[3];
            }
        const double n = (double)cnt * npx;
        NormConst k;
        if (n > 0) {
            const double mu = sx / n;
            double var = sxx / n - mu * mu;
            if (var < 0) var = 0;
            const double inv = 1.0 / sqrt(var + (double)eps);
            const double mt = st / n;
            const double mxt = (sxt - mu * st) * inv / n;      // mean(xhat * t)
            k.mu = (float)mu; k.sc = (float)(inv * gamma[c]); k.beta = beta[c];
            k.mt = (float)mt; k.c5 = (float)(inv * mxt);
            // batch mean and UNBIASED variance, what torch folds into running_mean / running_var (n = 1: no update)
            if (stats_out) stats_out[i] = make_float2((float)mu, n > 1 ? (float)(var * n / (n - 1.0)) : -1.0f);
        } else {
            k.mu = 0; k.sc = 0; k.beta = 0; k.mt = 0; k.c5 = 0;
            if (stats_out) stats_out[i] = make_float2(0.f, -1.0f);
        }
        consts[i] = k;
    }
}

// BatchNorm2d in training mode also folds every batch into its running statistics (momentum m):
//   running = (1 - m) * running + m * batch_stat, once per forward call, i.e. per (chunk, endpoint side) group IN ORDER
// (riemannian_metric.py:57-58 calls the decoder for the start side, then the end side of each chunk).  One thread per
// channel walks the groups of a pass sequentially (the rounding of every step is torch's).
__global__ __launch_bounds__(256) void running_update_kernel(const float2 *__restrict__ stats, int n_groups, int C, float m,
                                                            float *__restrict__ running_mean, float *__restrict__ running_var) {
    // One workgroup per 8 channels (one CU reading all 3.8 MB of a 60 000-latent build's statistics took 0.46 ms): all
    // threads stage blocks of 512 groups x 8 channels in LDS, then 8 threads apply the block's updates in order.
    constexpr int CH = 8, GB = 512;
    __shared__ float2 blk[GB * CH];                        // 32 KB
    const int c0 = blockIdx.x * CH;
    const int nc = C - c0 < CH ? C - c0 : CH;
    float rm = 0.f, rv = 0.f;
    if ((int)threadIdx.x < nc) { rm = running_mean[c0 + threadIdx.x]; rv = running_var[c0 + threadIdx.x]; }
    for (int g0 = 0; g0 < n_groups; g0 += GB) {
        const int ng = n_groups - g0 < GB ? n_groups - g0 : GB;
        float2 ld[GB * CH / 256];                           // all 16 loads of the thread in flight together
#pragma unroll
        for (int k = 0; k < GB * CH / 256; ++k) {
            const int i = k * 256 + threadIdx.x, g = i / CH, c = i % CH;
            ld[k] = (g < ng && c < nc) ? stats[(size_t)(g0 + g) * C + c0 + c] : make_float2(0.f, -1.f);
        }
#pragma unroll
        for (int k = 0; k < GB * CH / 256; ++k) blk[k * 256 + threadIdx.x] = ld[k];
        __syncthreads();
        if ((int)threadIdx.x < nc) {
            for (int g = 0; g < ng; g += 8) {              // 8 LDS reads in flight, then their dependent updates
                float2 st[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) st[j] = blk[(g + j) * CH + threadIdx.x];    // (rows past ng hold the skip mark)
#pragma unroll
                for (int j = 0; j < 8; ++j) {              // (selects, not branches: the chain is the critical path)
                    const bool live = st[j].y >= 0.f;      // else: empty or single-element batch (or past the end)
                    const float nm = (1.0f - m) * rm + m * st[j].x, nv = (1.0f - m) * rv + m * st[j].y;
                    rm = live ? nm : rm;
                    rv = live ? nv : rv;
                }
            }
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < nc) { running_mean[c0 + threadIdx.x] = rm; running_var[c0 + threadIdx.x] = rv; }
}

// mode 0 (none) / running statistics: one row of constants shared by every group.
__global__ void finalize_fixed_kernel(int C, int norm, const float *__restrict__ gamma, const float *__restrict__ beta,
                                      const float *__restrict__ rm, const float *__restrict__ rv, float eps,
                                      NormConst *__restrict__ consts) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        NormConst k;
        if (norm == 1) {
            const double inv = 1.0 / sqrt((double)rv[c] + (double)eps);
            k.mu = rm[c]; k.sc = (float)(inv * gamma[c]); k.beta = beta[c];
        } else if (norm == 2) {                               // GroupNorm: per-channel affine only, statistics per sample
            k.mu = 0.f; k.sc = gamma[c]; k.beta = beta[c];
        } else {
            k.mu = 0.f; k.sc = 1.f; k.beta = 0.f;
        }
        k.mt = 0.f; k.c5 = 0.f;
        consts[c] = k;
    }
}

__device__ __forceinline__ void norm_relu(const NormConst &k, float x, float t, float *a, float *ta) {
    const float xc = x - k.mu;
    const float y = fmaf(xc, k.sc, k.beta);
    const float tt = k.sc * (t - k.mt - xc * k.c5);
    *a = y > 0.f ? y : 0.f;
    *ta = y > 0.f ? tt : 0.f;
}

// GroupNorm (spatial_vae.py:13-16): statistics per (sample, group) over the group's channels and all pixels.
// g = {mean, 1/sqrt(var+eps), mean(t), inv * mean(xhat * t)}; gamma/beta per channel.
__device__ __forceinline__ void norm_relu_gn(const float4 &g, float gamma, float beta, float x, float t, float *a,
                                             float *ta) {
    const float xc = x - g.x;
    const float sc = g.y * gamma;
    const float y = fmaf(xc, sc, beta);
    const float tt = sc * (t - g.z - xc * g.w);
    *a = y > 0.f ? y : 0.f;
    *ta = y > 0.f ? tt : 0.f;
}

// pre / tpre: [slot][npx][C]; out: [slot][G].  fp64 accumulation, rounded once.
// `prim_row` (per-node primal): the primal row of slot s is pre[prim_row[s]] (its latent's row), the tangent row stays tpre[s].
__global__ __launch_bounds__(256) void group_stats_kernel(const float *__restrict__ pre, const float *__restrict__ tpre,
                                                         int64_t n_slots, int npx, int C, int G, float eps,
                                                         float4 *__restrict__ out, const int32_t *__restrict__ prim_row = nullptr) {
    const int cpg = C / G;
    const int64_t total = n_slots * G;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(i % G);
        const int64_t slot = i / G;
        const float *x = pre + (size_t)(prim_row ? prim_row[slot] : slot) * npx * C + (size_t)g * cpg;
        const float *t = tpre + (size_t)slot * npx * C + (size_t)g * cpg;
        double sx = 0.0, sxx = 0.0, st = 0.0, sxt = 0.0;
        for (int px = 0; px < npx; ++px)
            for (int k = 0; k < cpg; ++k) {
                const double xv = (double)x[(size_t)px * C + k], tv = (double)t[(size_t)px * C + k];
                sx += xv; sxx += xv * xv; st += tv; sxt += xv * tv;
            }
        const double n = (double)npx * cpg;
        const double mu = sx / n;
        double var = sxx / n - mu * mu;
        if (var < 0) var = 0;
        const double inv = 1.0 / sqrt(var + (double)eps);
        const double mt = st / n;
        const double mxt = (sxt - mu * st) * inv / n;
        out[i] = make_float4((float)mu, (float)inv, (float)mt, (float)(inv * mxt));
    }
}

// ---------------------------------------------------------------------------------- mid, bf16 x 3 split
// The f32 MFMA runs at 1/16 of the bf16 rate.  Every f32 operand is split exactly into three bf16 parts
// (a = a1 + a2 + a3, each part the truncated leading 8 mantissa bits of the remainder) and the product is
// formed as a1b1 + a1b2 + a2b1 + a2b2 + a1b3 + a3b1 with f32 accumulation inside v_mfma_f32_32x32x16_bf16:
// the dropped terms are below 2^-23 |a||b|, the level of one f32 rounding, for 6/16 of the matrix time.
__device__ __forceinline__ void split3(float a, unsigned short &p1, unsigned short &p2, unsigned short &p3) {
    const unsigned b1 = __float_as_uint(a) & 0xffff0000u;
    const float r1 = a - __uint_as_float(b1);                 // exact
    const unsigned b2 = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(b2);                // exact
    p1 = (unsigned short)(b1 >> 16);
    p2 = (unsigned short)(b2 >> 16);
    p3 = (unsigned short)(__float_as_uint(r2) >> 16);
}

// the same split for two values, the parts packed pairwise (low half = first value): 3 byte permutes instead of shifts and ors
__device__ __forceinline__ void split3_pair(float a0, float a1, unsigned &w1, unsigned &w2, unsigned &w3) {
    const unsigned u0 = __float_as_uint(a0), u1 = __float_as_uint(a1);
    w1 = __builtin_amdgcn_perm(u1, u0, 0x07060302u);
    const float r0 = a0 - __uint_as_float(u0 & 0xffff0000u), r1 = a1 - __uint_as_float(u1 & 0xffff0000u);   // exact
    const unsigned v0 = __float_as_uint(r0), v1 = __float_as_uint(r1);
    w2 = __builtin_amdgcn_perm(v1, v0, 0x07060302u);
    const float q0 = r0 - __uint_as_float(v0 & 0xffff0000u), q1 = r1 - __uint_as_float(v1 & 0xffff0000u);   // exact
    w3 = __builtin_amdgcn_perm(__float_as_uint(q1), __float_as_uint(q0), 0x07060302u);
}

// B3[chunk][blk][ks][h][part][col][8] bf16: lane (col, h) of the 32x32x16 B operand reads 16 contiguous bytes; the three parts of
// a (block, k-step, half) lie 2 KB apart -- one address register and the immediate offsets -2048 / 0 / +2048 reach all three
__global__ __launch_bounds__(256) void pack_mid_bf16_kernel(const float *__restrict__ B2p, int c1, int n_chunks,
                                                           unsigned short *__restrict__ B3) {
    const size_t per_blk = (size_t)c1 * NC;
    const size_t total = (size_t)n_chunks * MAX_BLOCKS * per_blk;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int col = (int)(i % NC);
        const int k = (int)((i / NC) % c1);
        const size_t cb = i / per_blk;                        // chunk * MAX_BLOCKS + blk
        unsigned short p[3];
        split3(B2p[i], p[0], p[1], p[2]);
        const int ks = k >> 4, h = (k >> 3) & 1, j = k & 7;
        for (int part = 0; part < 3; ++part)
            B3[(((cb * (c1 / 16) + ks) * 2 + h) * 3 + part) * (size_t)NC * 8 + (size_t)col * 8 + j] = p[part];
    }
}

template <int C1>
__global__ __launch_bounds__(256) void mid_bf16_kernel(const float *__restrict__ pre1, const float *__restrict__ tpre1,
                                                      const NormConst *__restrict__ consts1, int consts_per_group,
                                                      int tiles_per_group, ChunkTable tab, int opix_per_chunk, int c2,
                                                      const unsigned short *__restrict__ B3, const float *__restrict__ b2,
                                                      float *__restrict__ pre2, float *__restrict__ tpre2,
                                                      double *__restrict__ partial2, int want_stats,
                                                      const int32_t *__restrict__ slot_valid) {
    constexpr int LDK = C1 + 8;                               // bf16 elements per row (+16 B pad)
    constexpr int KS = C1 / 16;                               // 16-deep MFMA steps per input pixel
    __shared__ __attribute__((aligned(16))) unsigned short A3[3][2][TS][LDK];   // [part][primal|tangent][row][k]
    __shared__ NormConst kc[C1];
    const int tile = blockIdx.x, chunk = blockIdx.y;
    const int group = tile / tiles_per_group;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n1 = 4 * C1, n2 = 16 * c2;
    const size_t slot0 = (size_t)tile * TS;
    for (int c = threadIdx.x; c < C1; c += 256) kc[c] = consts1[(size_t)(consts_per_group ? group : 0) * C1 + c];

    f32x16 accp, acct;
#pragma unroll
    for (int i = 0; i < 16; ++i) { accp[i] = 0.f; acct[i] = 0.f; }

    const int nblk = tab.nblk[chunk];
    const int r = lane & 31, h = lane >> 5;
    for (int blk = 0; blk < nblk; ++blk) {
        const int ip = tab.ipix[chunk][blk];
        __syncthreads();
        {   // stage A: thread -> (sample = tid/8, C1/8 consecutive channels); norm1 + ReLU, then the 3-way split
            const int s = threadIdx.x >> 3, k0 = (threadIdx.x & 7) * (C1 / 8);
            const float *xp = pre1 + (slot0 + s) * n1 + (size_t)ip * C1 + k0;
            const float *xt = tpre1 + (slot0 + s) * n1 + (size_t)ip * C1 + k0;
#pragma unroll
            for (int k = 0; k < C1 / 8; ++k) {
                float a, ta;
                norm_relu(kc[k0 + k], xp[k], xt[k], &a, &ta);
                split3(a, A3[0][0][s][k0 + k], A3[1][0][s][k0 + k], A3[2][0][s][k0 + k]);
                split3(ta, A3[0][1][s][k0 + k], A3[1][1][s][k0 + k], A3[2][1][s][k0 + k]);
            }
        }
        // B fragments of this block, all three parts: lane (col r of the wave's 32, half h)
        bf16x8 b[3][KS];
        const unsigned short *bsrc = B3 + ((size_t)(chunk * MAX_BLOCKS + blk) * 3 * KS * 2) * (size_t)NC * 8;
#pragma unroll
        for (int part = 0; part < 3; ++part)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                b[part][ks] = *reinterpret_cast<const bf16x8 *>(
                    bsrc + (((size_t)ks * 2 + h) * 3 + part) * (size_t)NC * 8 + (size_t)(wave * 32 + r) * 8);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            bf16x8 ap[3], at[3];
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                ap[part] = *reinterpret_cast<const bf16x8 *>(&A3[part][0][r][ks * 16 + h * 8]);
                at[part] = *reinterpret_cast<const bf16x8 *>(&A3[part][1][r][ks * 16 + h * 8]);
            }
            // smallest terms first
            accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[2], b[0][ks], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[2], b[0][ks], acct, 0, 0, 0);
            accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[2][ks], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[2][ks], acct, 0, 0, 0);
            accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[1][ks], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[1][ks], acct, 0, 0, 0);
            accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[0][ks], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[0][ks], acct, 0, 0, 0);
            accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[1][ks], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[1][ks], acct, 0, 0, 0);
            accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[0][ks], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[0][ks], acct, 0, 0, 0);
        }
    }

    // epilogue: C[row = (r&3) + 8*(r>>2) + 4*(lane>>5)][col = lane&31]  (same map as the f32 MFMA)
    const int col = wave * 32 + (lane & 31);
    const int lo = col / c2, co = col % c2;
    const bool col_ok = lo < opix_per_chunk;
    const int op = col_ok ? tab.opix[chunk][lo] : 0;
    const float bias = col_ok ? b2[co] : 0.f;
    double sx = 0, sxx = 0, st_ = 0, sxt = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        const float x = accp[q] + bias, t = acct[q];
        if (col_ok) {
            pre2[(slot0 + row) * n2 + (size_t)op * c2 + co] = x;
            tpre2[(slot0 + row) * n2 + (size_t)op * c2 + co] = t;
            if (slot_valid[slot0 + row]) { sx += x; sxx += (double)x * x; st_ += t; sxt += (double)x * t; }
        }
    }
    if (want_stats) {
        sx += __shfl_xor(sx, 32, 64); sxx += __shfl_xor(sxx, 32, 64);
        st_ += __shfl_xor(st_, 32, 64); sxt += __shfl_xor(sxt, 32, 64);
        if (lane < 32 && col_ok) {
            double *p = partial2 + ((size_t)tile * n2 + (size_t)op * c2 + co) * 4;
            p[0] = sx; p[1] = sxx; p[2] = st_; p[3] = sxt;
        }
    }
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding global load and
// store of the wave (s_waitcnt vmcnt(0)): that drains the prefetched pre-activations of the next input pixel
// (and, in a persistent kernel, the epilogue's stores) at every phase.  Nothing here communicates through global memory inside a launch.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- static geometry of ConvT2 (k4 s2 p1, 2x2 -> 4x4) in 8 chunks of two output pixels -- what make_chunks builds for
// n_chunks == 8, opix_per_chunk == 2 (the host checks its table against these before taking the mid_all path) -------------
//   chunk : output pixels      input pixels (block order)
//     0   : (0,1) (0,2)        0 1          4 : (1,1) (1,2)   0 1 2 3
//     1   : (3,1) (3,2)        2 3          5 : (2,1) (2,2)   0 1 2 3
//     2   : (1,0) (2,0)        0 2          6 : (0,0) (0,3)   0 1
//     3   : (1,3) (2,3)        1 3          7 : (3,0) (3,3)   2 3
// Wave group 0 owns chunks {0,3,4,7}, group 1 {1,2,5,6}: ten (input pixel, chunk) products each, 2 or 3 per input pixel.
struct MidGeom {
    static __host__ __device__ constexpr int chunk_of(int wg, int lc) {
        constexpr int t[2][4] = {{0, 3, 4, 7}, {1, 2, 5, 6}};
        return t[wg][lc];
    }
    static __host__ __device__ constexpr int opix(int ch, int lo) {
        constexpr int t[8][2] = {{1, 2}, {13, 14}, {4, 8}, {7, 11}, {5, 6}, {9, 10}, {0, 3}, {12, 15}};
        return t[ch][lo];
    }
    // position of input pixel ip in the chunk's block list, -1 = the chunk does not read it
    static __host__ __device__ constexpr int blk_of(int ch, int ip) {
        constexpr int t[8][4] = {{0, 1, -1, -1}, {-1, -1, 0, 1}, {0, -1, 1, -1}, {-1, 0, -1, 1},
                                 {0, 1, 2, 3},   {0, 1, 2, 3},   {0, 1, -1, -1}, {-1, -1, 0, 1}};
        return t[ch][ip];
    }
    static __host__ __device__ constexpr int n_prod(int wg, int ip) {
        int n = 0;
        for (int lc = 0; lc < 4; ++lc) n += blk_of(chunk_of(wg, lc), ip) >= 0 ? 1 : 0;
        return n;
    }
    static __host__ __device__ constexpr int prod_lc(int wg, int ip, int j) {   // j-th chunk slot of the group that reads pixel ip
        int n = 0;
        for (int lc = 0; lc < 4; ++lc)
            if (blk_of(chunk_of(wg, lc), ip) >= 0) { if (n == j) return lc; ++n; }
        return 0;
    }
    static __host__ __device__ constexpr int prod_cb(int wg, int ip, int j) {   // chunk * MAX_BLOCKS + block of that product
        const int ch = chunk_of(wg, prod_lc(wg, ip, j));
        return ch * MAX_BLOCKS + blk_of(ch, ip);
    }
    // The input pixels are processed in the order 3, 2, 1, 0: group 0 then ends a tile with a two-product pixel and group 1 starts it
    // with one -- the light pixel shares its interval with the group's epilogue in mid_pipe_kernel (19 900 instead of 23 000
    // cycles for those two intervals).  Both ConvT2 kernels use this order, so their pre-activations stay bit-identical.
    static __host__ __device__ constexpr int pix(int pos) { return 3 - pos; }
    // ring slot of the first step of the pixel at position pos: steps are numbered through the four pixels of a tile, slot = step % 3
    static __host__ __device__ constexpr int ring_off(int wg, int pos, int ks_per_pixel) {
        int n = 0;
        for (int i = 0; i < pos; ++i) n += n_prod(wg, pix(i)) * ks_per_pixel;
        return n % 3;
    }
};

// The products of ONE input pixel for one wave: steps s = (k-step ks, product j), ks outer.  The A fragments of a k-step (three
// split parts, primal and tangent: six 16-byte LDS reads) are read ONCE and feed every product of the pixel (2 or 3 chunks) --
// the chunk-outer order of rounds 1-3 read them again per chunk -- and the NEXT k-step's are read while this one multiplies
// (two register sets).  The B fragments (weights: L2 -> registers, 3 x 16 bytes per lane and step) run through a ring of three
// register sets, issued two steps (24 MFMAs, ~770 cycles) before their use; the first two steps of the NEXT pixel are issued
// before this pixel's last MFMAs so that the staging phase / barrier between pixels covers their latency.
// Accumulation order per accumulator is unchanged (pixel, k-step, the six split products): results are bit-identical.
template <int C1, bool TONLY, int WG, int POS>
__device__ __forceinline__ void mid_products(const unsigned short *__restrict__ a3, unsigned a_idx,   // &A3[0]..., element index of [buf][0][0][r][h * 8]
                                             __amdgpu_buffer_rsrc_t b_rsrc,                 // descriptor of B3 (wave-uniform)
                                             unsigned b_lane,                               // this lane's BYTE offset inside a triple
                                             f32x16 (&accp)[4], f32x16 (&acct)[4], bf16x8 (&ring)[3][3]) {
    constexpr int KS = C1 / 16, LDK = C1 + 8;
    constexpr int IP = MidGeom::pix(POS);                         // the input pixel at this position of the tile's sequence
    constexpr int NP = MidGeom::n_prod(WG, IP);
    constexpr int NSTEP = KS * NP;
    constexpr int OFF = MidGeom::ring_off(WG, POS, KS);           // ring slot of this pixel's step 0
    constexpr ptrdiff_t PART = (ptrdiff_t)NC * 8;                 // elements between the parts of a fragment triple
    constexpr size_t A_PT = (size_t)TS * LDK, A_PART = 2 * A_PT;  // A3[buf][part][primal|tangent][row][k]
    auto b_load = [&](int wg, int ip, int s, bf16x8 (&dst)[3]) {
        const int ks = s / MidGeom::n_prod(wg, ip), j = s % MidGeom::n_prod(wg, ip);
        // buffer loads: the descriptor and the block's byte offset are scalar, ONE per-lane 32-bit offset register serves every
        // load of the kernel -- no vector address arithmetic, no 64-bit address pairs
        const int soff = (int)((((ptrdiff_t)MidGeom::prod_cb(wg, ip, j) * KS + ks) * 2) * 3 * PART * 2);
        dst[0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, soff, 0));
        dst[1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, soff + (int)(PART * 2), 0));
        dst[2] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, soff + (int)(PART * 4), 0));
    };
    // ONE register set for the A fragments.  Within a step the six split products of an accumulator run in the order
    // a3 b1, a2 b2, a2 b1, a1 b3, a1 b2, a1 b1 (small terms first), so a3 is free after the first pair of MFMAs of a k-step's
    // LAST product, a2 after the third, a1 after the sixth: each part of the NEXT k-step is read into the registers its
    // predecessor just left, at least six MFMAs (190 cycles) before its first use.
    bf16x8 ap[3], at[3];
    // (the index passes through an empty asm: the compiler can then neither fold it with the buffer's constant into offsets beyond
    // the 16-bit immediate of ds_read, nor hoist one address register per read out of a persistent kernel's tile loop)
    asm volatile("" : "+v"(a_idx));
    const unsigned short *a_base = a3 + a_idx;
    auto a_part = [&](int ks, int part) {
        if (!TONLY) ap[part] = *reinterpret_cast<const bf16x8 *>(a_base + part * A_PART + ks * 16);
        at[part] = *reinterpret_cast<const bf16x8 *>(a_base + part * A_PART + A_PT + ks * 16);
    };
    a_part(0, 2); a_part(0, 1); a_part(0, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, TONLY ? 3 : 6, 0);    // (the pipeline below starts behind these reads)
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
        const int ks = s / NP, j = s % NP, slot = (OFF + s) % 3;
        const int lc = MidGeom::prod_lc(WG, IP, j);
        const bool reload = j == NP - 1 && ks + 1 < KS;          // last product of the k-step: refill A behind its last uses
        if (s + 2 < NSTEP) b_load(WG, IP, s + 2, ring[(OFF + s + 2) % 3]);
        else if (POS < 3) b_load(WG, MidGeom::pix(POS + 1), s + 2 - NSTEP, ring[(OFF + s + 2) % 3]);   // the next pixel's first two steps
        const bf16x8 (&b)[3] = ring[slot];
        if (!TONLY) accp[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[2], b[0], accp[lc], 0, 0, 0);
        acct[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[2], b[0], acct[lc], 0, 0, 0);
        if (reload) a_part(ks + 1, 2);
        if (!TONLY) accp[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[1], accp[lc], 0, 0, 0);
        acct[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[1], acct[lc], 0, 0, 0);
        if (!TONLY) accp[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[0], accp[lc], 0, 0, 0);
        acct[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[0], acct[lc], 0, 0, 0);
        if (reload) a_part(ks + 1, 1);
        if (!TONLY) accp[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[2], accp[lc], 0, 0, 0);
        acct[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[2], acct[lc], 0, 0, 0);
        if (!TONLY) accp[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[1], accp[lc], 0, 0, 0);
        acct[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[1], acct[lc], 0, 0, 0);
        if (!TONLY) accp[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[0], accp[lc], 0, 0, 0);
        acct[lc] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[0], acct[lc], 0, 0, 0);
        if (reload) a_part(ks + 1, 0);
        // pin the pipeline: left alone, the scheduler sinks every load to a few MFMAs before its use (register pressure
        // heuristics) and the prefetch distance is gone.  Per step: the weight loads (for step s + 2) first, then the MFMAs with
        // the LDS reads of the next k-step behind the pairs that free their registers.
        constexpr int PAIR_M = TONLY ? 1 : 2, DS = TONLY ? 1 : 2;
        if (s + 2 < NSTEP || POS < 3) __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
        if (reload) {
            __builtin_amdgcn_sched_group_barrier(0x008, PAIR_M, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, DS, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * PAIR_M, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, DS, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 3 * PAIR_M, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, DS, 0);
        } else {
            __builtin_amdgcn_sched_group_barrier(0x008, 6 * PAIR_M, 0);
        }
        // every step is a scheduling region of its own: the order ACROSS steps is program order (what the ring needs), and the
        // group solver sees 20 instructions instead of a pixel's 2 000 (compile time: minutes -> seconds)
        __builtin_amdgcn_sched_barrier(0);
    }
}

#ifdef GEO_MID_PROF
// per wave group (waves 0 and 4 report): [0] prologue + first staging, [1..4] the four pixel intervals up to their barrier,
// [5] time parked in those barriers, [6] epilogue, [7] tiles
__device__ unsigned long long g_mid_prof[2][8];
#define GEO_MP_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define GEO_MP_ADD(slot, val) do { if (lane == 0 && wq == 0) atomicAdd(&g_mid_prof[wg][slot], (unsigned long long)(val)); } while (0)
#else
#define GEO_MP_STAMP(v)
#define GEO_MP_ADD(slot, val)
#endif

// ---- all eight 128-column chunks of a tile in ONE workgroup (dec_channels[2] = 64) ----------------
// Staging an input pixel's A block (norm1 + ReLU + 3-way split of 32 x C1 primal and tangent values) costs
// about as much VALU time as the 96 bf16 MFMAs one chunk spends on it.  Here the block is staged once (by
// 512 threads) and used by the five chunks that need it.  Waves 0-3 own chunks {0,3,4,7}, waves 4-7 chunks
// {1,2,5,6} (10 of the 20 (pixel, chunk) products each, 2 or 3 per pixel): 4 x 2 accumulator tiles = 128
// registers per wave, so two waves share a SIMD and one's weight-fragment loads (L2) hide behind the other's
// MFMAs.
// TONLY: tangent stream only -- decoders with fixed statistics (no norm, BatchNorm in eval mode) get the primal ConvT2 output
// once per LATENT from a separate launch over the nodes (run_jvp, "per-node primal"); here the primal pre-activation only
// decides the ReLU mask of the tangent.
template <int C1, bool GN, bool TONLY = false>
__global__ __launch_bounds__(512, 2) void mid_all_kernel(const float *__restrict__ pre1, const float *__restrict__ tpre1,
                                                        const NormConst *__restrict__ consts1, int consts_per_group,
                                                        int tiles_per_group, int c2,
                                                        const unsigned short *__restrict__ B3,
                                                        const float *__restrict__ b2, float *__restrict__ pre2,
                                                        float *__restrict__ tpre2, double *__restrict__ partial2,
                                                        int want_stats, const int32_t *__restrict__ slot_valid,
                                                        const float4 *__restrict__ gs1, int64_t e_base, int64_t n_edges,
                                                        int batch) {
    // BatchNorm / no norm at 128 channels: a lane stages a channel PAIR of 4 samples (constants in registers, the packed
    // pairs leave as conflict-free 4-byte stores); GroupNorm and the narrower decoders keep (sample, C1/16 channels)
    constexpr bool PAIR = C1 == 128 && !GN;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    constexpr int LDK = C1 + 8;
    constexpr int KS = C1 / 16;
    constexpr int NL = 4;                                      // chunks per wave group
    constexpr int CPT = C1 / 16;                               // channels staged per thread
    __shared__ __attribute__((aligned(16))) unsigned short A3[2][3][2][TS][LDK];   // double buffered over input pixels
    __shared__ NormConst kc[C1];
    GEO_MP_STAMP(mp0);
    const int tile = blockIdx.x;
    const int group = tile / tiles_per_group;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wq = wave & 3, wg = wave >> 2;                   // column quarter, chunk group
    const int n1 = 4 * C1, n2 = 16 * c2;
    const size_t slot0 = (size_t)tile * TS;
    for (int c = threadIdx.x; c < C1; c += 512) kc[c] = consts1[(size_t)(consts_per_group ? group : 0) * C1 + c];

    f32x16 accp[NL], acct[NL];
#pragma unroll
    for (int lc = 0; lc < NL; ++lc)
#pragma unroll
        for (int i = 0; i < 16; ++i) { accp[lc][i] = 0.f; acct[lc][i] = 0.f; }

    const int r = lane & 31, h = lane >> 5;
    // staging: thread -> (sample = tid/16, CPT consecutive channels).  The raw pre-activations of the NEXT input
    // pixel are fetched (HBM) while the MFMAs of the current one run; one barrier per pixel.
    const int ss = threadIdx.x >> 4, k0 = (threadIdx.x & 15) * CPT;
    float rawp[CPT], rawt[CPT];
    const int k0p = 2 * lane, s0p = 4 * wave;
    f32x2 rp[4], rt[4];
    NormConst kA = {0.f, 0.f, 0.f, 0.f, 0.f}, kB = kA;
    if (PAIR) {
        const NormConst *kp = consts1 + (size_t)(consts_per_group ? group : 0) * C1 + k0p;
        kA = kp[0];
        kB = kp[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rp[i] = *reinterpret_cast<const f32x2 *>(pre1 + (slot0 + s0p + i) * n1 + (size_t)MidGeom::pix(0) * C1 + k0p);
            rt[i] = *reinterpret_cast<const f32x2 *>(tpre1 + (slot0 + s0p + i) * n1 + (size_t)MidGeom::pix(0) * C1 + k0p);
        }
    } else {
        const float *xp = pre1 + (slot0 + ss) * n1 + (size_t)MidGeom::pix(0) * C1 + k0, *xt = tpre1 + (slot0 + ss) * n1 + (size_t)MidGeom::pix(0) * C1 + k0;
#pragma unroll
        for (int k = 0; k < CPT; ++k) { rawp[k] = xp[k]; rawt[k] = xt[k]; }
    }
    const int colw = wq * 32 + (lane & 31);
    const int lo = colw / c2, co = colw % c2;
    const float bias = b2[co];
    // GroupNorm (32 groups): the thread's CPT = C1/16 channels span exactly two groups of C1/32 channels
    float4 gg0 = make_float4(0.f, 0.f, 0.f, 0.f), gg1 = gg0;
    if (GN) {
        gg0 = gs1[(slot0 + ss) * 32 + (threadIdx.x & 15) * 2];
        gg1 = gs1[(slot0 + ss) * 32 + (threadIdx.x & 15) * 2 + 1];
    }
    __syncthreads();                                           // kc visible
    // stage_px(buf, nx): normalise + ReLU + split the raw values held in registers into A3[buf], then fetch those of the pixel at
    // position nx of the sequence (nx < 4)
    auto stage_px = [&](int buf, int nx) {
        if (PAIR) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float a0, t0, a1, t1;
                norm_relu(kA, rp[i].x, rt[i].x, &a0, &t0);
                norm_relu(kB, rp[i].y, rt[i].y, &a1, &t1);
                unsigned wa[3], wt[3];
                if (!TONLY) split3_pair(a0, a1, wa[0], wa[1], wa[2]);
                split3_pair(t0, t1, wt[0], wt[1], wt[2]);
#pragma unroll
                for (int part = 0; part < 3; ++part) {
                    if (!TONLY) *reinterpret_cast<unsigned *>(&A3[buf][part][0][s0p + i][k0p]) = wa[part];
                    *reinterpret_cast<unsigned *>(&A3[buf][part][1][s0p + i][k0p]) = wt[part];
                }
            }
            if (nx < 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    rp[i] = *reinterpret_cast<const f32x2 *>(pre1 + (slot0 + s0p + i) * n1 + (size_t)MidGeom::pix(nx) * C1 + k0p);
                    rt[i] = *reinterpret_cast<const f32x2 *>(tpre1 + (slot0 + s0p + i) * n1 + (size_t)MidGeom::pix(nx) * C1 + k0p);
                }
                // (a scheduling group of their own: otherwise these eight loads fill the first load groups of mid_products'
                // pipeline and push every weight load two steps late)
                __builtin_amdgcn_sched_group_barrier(0x020, 8, 0);
            }
        } else {
            unsigned short pp[3][CPT], pt[3][CPT];
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                float a, ta;
                if (GN) norm_relu_gn(k < CPT / 2 ? gg0 : gg1, kc[k0 + k].sc, kc[k0 + k].beta, rawp[k], rawt[k], &a, &ta);
                else norm_relu(kc[k0 + k], rawp[k], rawt[k], &a, &ta);
                if (!TONLY) split3(a, pp[0][k], pp[1][k], pp[2][k]);
                split3(ta, pt[0][k], pt[1][k], pt[2][k]);
            }
#pragma unroll
            for (int part = 0; part < 3; ++part)
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    if (!TONLY) A3[buf][part][0][ss][k0 + k] = pp[part][k];
                    A3[buf][part][1][ss][k0 + k] = pt[part][k];
                }
            if (nx < 4) {
                const float *xp = pre1 + (slot0 + ss) * n1 + (size_t)MidGeom::pix(nx) * C1 + k0;
                const float *xt = tpre1 + (slot0 + ss) * n1 + (size_t)MidGeom::pix(nx) * C1 + k0;
#pragma unroll
                for (int k = 0; k < CPT; ++k) { rawp[k] = xp[k]; rawt[k] = xt[k]; }
                __builtin_amdgcn_sched_group_barrier(0x020, 2 * ((CPT + 3) / 4), 0);
            }
        }
    };
    // The two waves of a SIMD (w and w + 4 = the two chunk groups) take the phases of an input pixel in opposite order: waves 0-3
    // multiply pixel ip and then stage pixel ip + 1 into the other buffer, waves 4-7 stage first and multiply afterwards -- one
    // partner's vector / LDS-store work runs beside the other's MFMAs instead of both reaching the matrix pipe together.
    bf16x8 ring[3][3];
    const unsigned b_lane = (unsigned)(h * 3 * NC * 8 + (wq * 32 + r) * 8) * 2u;      // bytes
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short *>(B3), 0, (int)((size_t)8 * MAX_BLOCKS * C1 * NC * 3 * 2), 0x00020000);
    {   // the first two steps' weight fragments of pixel 0 (both wave groups): in flight during the first staging
        const int cb0 = wg == 0 ? MidGeom::prod_cb(0, MidGeom::pix(0), 0) : MidGeom::prod_cb(1, MidGeom::pix(0), 0);
        const int cb1 = wg == 0 ? MidGeom::prod_cb(0, MidGeom::pix(0), 1) : MidGeom::prod_cb(1, MidGeom::pix(0), 1);
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            ring[0][part] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, (cb0 * KS * 2 * 3 + part) * NC * 8 * 2, 0));
            ring[1][part] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, (cb1 * KS * 2 * 3 + part) * NC * 8 * 2, 0));
        }
    }
    stage_px(0, 1);
    if (wg == 1) __builtin_amdgcn_s_setprio(1);                // the later-dispatched half loses every issue arbitration otherwise
    lds_barrier();                                             // (LDS only: the next pixel's loads stay in flight)
    GEO_MP_STAMP(mp1);
    GEO_MP_ADD(0, mp1 - mp0);
    const unsigned short *a3 = &A3[0][0][0][0][0];
    const unsigned a_lane = (unsigned)(r * LDK + h * 8);
    constexpr unsigned A_BUF = 3u * 2u * TS * LDK;
    // (ring slots run through the four pixels of a tile: MidGeom::ring_off gives every pixel body its first slot)
#define GEO_MID_PIXEL(WGV, IPV)                                                                                        \
    mid_products<C1, TONLY, WGV, IPV>(a3, a_lane + ((IPV) & 1) * A_BUF, b_rsrc, b_lane, accp, acct, ring)
#ifdef GEO_MID_PROF
    unsigned long long mp_prev = mp1, mp_wait = 0;
#define GEO_MP_INTERVAL(slot, with_barrier)                                                                            \
    { const unsigned long long t_a = __builtin_amdgcn_s_memtime();                                                      \
      if (with_barrier) { lds_barrier(); }                                                                              \
      const unsigned long long t_b = __builtin_amdgcn_s_memtime();                                                      \
      GEO_MP_ADD(slot, t_a - mp_prev); mp_wait += t_b - t_a; mp_prev = t_b; }
#else
#define GEO_MP_INTERVAL(slot, with_barrier) { if (with_barrier) { lds_barrier(); } }
#endif
    if (wg == 0) {
        GEO_MID_PIXEL(0, 0); stage_px(1, 2); GEO_MP_INTERVAL(1, true)
        GEO_MID_PIXEL(0, 1); stage_px(0, 3); GEO_MP_INTERVAL(2, true)
        GEO_MID_PIXEL(0, 2); stage_px(1, 4); GEO_MP_INTERVAL(3, true)
        GEO_MID_PIXEL(0, 3); GEO_MP_INTERVAL(4, false)
    } else {
        stage_px(1, 2); GEO_MID_PIXEL(1, 0); GEO_MP_INTERVAL(1, true)
        stage_px(0, 3); GEO_MID_PIXEL(1, 1); GEO_MP_INTERVAL(2, true)
        stage_px(1, 4); GEO_MID_PIXEL(1, 2); GEO_MP_INTERVAL(3, true)
        GEO_MID_PIXEL(1, 3); GEO_MP_INTERVAL(4, false)
    }
#undef GEO_MP_INTERVAL
#undef GEO_MID_PIXEL

    // rows of the tile that hold edges of the chunk (slot_valid_kernel's rule, computed here: no loads in the epilogue)
    int64_t cnt_g = n_edges - (e_base + (int64_t)(group >> 1) * batch);
    if (cnt_g > batch) cnt_g = batch;
    const int n_valid = (int)cnt_g - (tile - group * tiles_per_group) * TS;
    // batch statistics: a lane's column is the same channel co in all four chunks of its wave, so their (and the two row
    // halves') sums are added in registers; the four waves holding channel co (column quarters wq and wq ^ 2 of both wave
    // groups) meet in LDS and are added in wave order: partial2 is [tile][c2][4], the tile's 16 pixels already summed
    __shared__ double red[8][32][4];
    double sx = 0, sxx = 0, st_ = 0, sxt = 0;
#pragma unroll
    for (int lc = 0; lc < NL; ++lc) {
        const int ch = wg == 0 ? MidGeom::chunk_of(0, lc) : MidGeom::chunk_of(1, lc);
        const int op = lo == 0 ? MidGeom::opix(ch, 0) : MidGeom::opix(ch, 1);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
            const float x = accp[lc][q] + bias, t = acct[lc][q];
            if (!TONLY) pre2[(slot0 + row) * n2 + (size_t)op * c2 + co] = x;
            tpre2[(slot0 + row) * n2 + (size_t)op * c2 + co] = t;
            if (!TONLY && row < n_valid) { sx += x; sxx += (double)x * x; st_ += t; sxt += (double)x * t; }
        }
    }
    if (want_stats) {
        sx += __shfl_xor(sx, 32, 64); sxx += __shfl_xor(sxx, 32, 64);
        st_ += __shfl_xor(st_, 32, 64); sxt += __shfl_xor(sxt, 32, 64);
        if (lane < 32) { red[wave][lane][0] = sx; red[wave][lane][1] = sxx; red[wave][lane][2] = st_; red[wave][lane][3] = sxt; }
        __syncthreads();
        if (threadIdx.x < 64) {                                // thread = channel
            const int w0 = threadIdx.x >> 5, l = threadIdx.x & 31;
            double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { a0 += red[w0 + 2 * w][l][0]; a1 += red[w0 + 2 * w][l][1]; a2 += red[w0 + 2 * w][l][2]; a3 += red[w0 + 2 * w][l][3]; }
            double *p = partial2 + ((size_t)tile * c2 + threadIdx.x) * 4;
            p[0] = a0; p[1] = a1; p[2] = a2; p[3] = a3;
        }
    }
#ifdef GEO_MID_PROF
    { const unsigned long long t_e = __builtin_amdgcn_s_memtime();
      GEO_MP_ADD(6, t_e - mp_prev); GEO_MP_ADD(5, mp_wait); GEO_MP_ADD(7, 1); }
#endif
}

// BN2 partial sums of one lane of a ConvT2 wave (mid_pipe_kernel's layout): bn2_add over rows (q & 3) + 8 (q >> 2) + 4 h of the
// tile, the wave's four chunks in order (lc outer, q inner), then bn2_store adds the two row halves, one [tile][wave slot][channel]
// entry per lane < 32.  The primal comes from the accumulators (mid_pipe_kernel) or is gathered from the start side's compact rows
// (mid_start_kernel): the same terms in the same order, bit-identical sums.
struct Bn2Sums { double sx = 0, sxx = 0, st = 0, sxt = 0; };
__device__ __forceinline__ void bn2_add(Bn2Sums &a, float x, float t, bool live) {
    // (no branch per element: rows beyond the chunk's edges contribute zeros; all but a batch's last tile are full)
    const double xd = live ? (double)x : 0.0, td = live ? (double)t : 0.0;
    a.sx += xd; a.sxx = fma(xd, xd, a.sxx); a.st += td; a.sxt = fma(xd, td, a.sxt);
}
__device__ __forceinline__ void bn2_store(Bn2Sums a, double *__restrict__ partial2, int tile, int wslot, int co, int lane) {
    a.sx += __shfl_xor(a.sx, 32, 64); a.sxx += __shfl_xor(a.sxx, 32, 64);
    a.st += __shfl_xor(a.st, 32, 64); a.sxt += __shfl_xor(a.sxt, 32, 64);
    if (lane < 32) {                                           // wave slot = (chunk group, column half): channels (wq & 1) * 32 + lane
        double *pp = partial2 + (((size_t)tile * 4 + wslot) * 64 + co) * 4;
        pp[0] = a.sx; pp[1] = a.sxx; pp[2] = a.st; pp[3] = a.sxt;
    }
}

// ---- ConvT2, persistent and skewed (dec_channels 128 -> 64, BatchNorm or no norm): the default for the shipped decoder ------
// In-kernel stamps of mid_all_kernel (one tile per workgroup, -DGEO_MID_PROF): the four pixel intervals keep the matrix pipe 85 %
// busy, but the tile's prologue (constants, first staging: 9 100 cycles) and epilogue (128 stores per wave + fp64 statistics:
// 13 800) run with NO MFMA beside them -- a quarter of the 95 600 cycles of a tile.  Here ONE workgroup per CU walks over its tiles
// and the two wave groups (waves 0-3 / 4-7 = the two chunk groups, one wave of each per SIMD) trade those phases:
//     interval 0 : group 0  P0, stage pixel 1 (all 32 samples)      group 1  EPILOGUE of the previous tile, P0
//     interval 1 : group 0  P1, stage half of pixel 2                 group 1  stage half of pixel 2, P1
//     interval 2 : group 0  P2, stage half of pixel 3                 group 1  stage half of pixel 3, P2
//     interval 3 : group 0  P3, EPILOGUE of this tile                 group 1  stage pixel 0 of the NEXT tile (all samples), P3
// (one LDS-only barrier after each interval; Pk = the products of the k-th input pixel of the sequence 3, 2, 1, 0, mid_products).  One group's stores / statistics /
// staging always run beside the other group's MFMAs.  The statistics leave per wave (partial2 [tile][4 wave slots][channel],
// finalize_batch_kernel adds them: npx_stored = 4), so no epilogue needs a workgroup barrier.  Same products in the same order as
// mid_all_kernel: pre-activations are bit-identical; the fp64 statistic sums associate differently (last-bit differences).
template <bool END_ONLY>
__global__ __launch_bounds__(512, 2) void mid_pipe_kernel(const float *__restrict__ pre1, const float *__restrict__ tpre1,
                                                         const NormConst *__restrict__ consts1, int consts_per_group,
                                                         int tiles_per_group, int n_tiles, int /*c2 == 64*/,
                                                         const unsigned short *__restrict__ B3, const float *__restrict__ b2,
                                                         float *__restrict__ pre2, float *__restrict__ tpre2,
                                                         double *__restrict__ partial2, int want_stats, int64_t e_base,
                                                         int64_t n_edges, int batch) {
    // END_ONLY: the n_tiles work tiles are the END-side tiles of the pass (the start side runs in mid_start_kernel)
    constexpr int C1 = 128, LDK = C1 + 8, KS = C1 / 16, NL = 4, c2 = 64;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) unsigned short A3[2][3][2][TS][LDK];   // double buffered over input pixels
    // (readfirstlane: everything derived from the wave number is then provably wave-uniform -- scalar branches on the chunk group,
    // scalar offsets for the buffer loads / stores below instead of a 64-bit address pair per access)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wq = wave & 3, wg = wave >> 2;                   // column quarter, chunk group
    constexpr int n1 = 4 * C1, n2 = 16 * c2;
    const int r = lane & 31, h = lane >> 5;
    const int k0p = 2 * lane;                                  // the lane's channel pair when staging
    const int lo = wq >> 1, co = (wq & 1) * 32 + r;            // output pixel of the chunk (wave-uniform), channel
    const float bias = b2[co];
    const unsigned v_out = (unsigned)(4 * h * n2 + co) * 4u;    // the lane's byte offset inside a tile of pre2 / tpre2
    const int my_tiles = (n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    if (my_tiles <= 0) return;

    f32x16 accp[NL], acct[NL];
    auto zero_acc = [&]() {
#pragma unroll
        for (int lc = 0; lc < NL; ++lc)
#pragma unroll
            for (int i = 0; i < 16; ++i) { accp[lc][i] = 0.f; acct[lc][i] = 0.f; }
    };
    zero_acc();
    // staging state of this wave: constants of the tile it stages next, and raw pre-activations in flight
    NormConst kA, kB;
    f32x2 rp[4], rt[4];
    auto phys = [&](int t) { return END_ONLY ? ((t / tiles_per_group) * 2 + 1) * tiles_per_group + t % tiles_per_group : t; };
    auto load_consts = [&](int tile) {
        tile = phys(tile);
        const NormConst *kp = consts1 + (size_t)(consts_per_group ? tile / tiles_per_group : 0) * C1 + k0p;
        kA = kp[0];
        kB = kp[1];
    };
    // raw values of NS samples (sample0 ...) of input pixel px of a tile -> rp / rt (in flight until stage())
    // (per-tile buffer descriptors: the tile's base is scalar arithmetic, the lane contributes ONE loop-invariant 32-bit offset)
    const unsigned v_pair = (unsigned)k0p * 4u;
    auto fetch = [&](int tile, int px, int sample0, auto ns_tag) {
        constexpr int NS = decltype(ns_tag)::value;
        const size_t tbase = (size_t)phys(tile) * TS * n1;
        const __amdgpu_buffer_rsrc_t rp_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pre1 + tbase), 0, TS * n1 * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rt_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(tpre1 + tbase), 0, TS * n1 * 4, 0x00020000);
        const int soff = (sample0 * n1 + MidGeom::pix(px) * C1) * 4;      // (px = position in the tile's pixel sequence)
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            rp[i] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rp_src, v_pair, soff + i * n1 * 4, 0));
            rt[i] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rt_src, v_pair, soff + i * n1 * 4, 0));
        }
        __builtin_amdgcn_sched_group_barrier(0x020, 2 * NS, 0);  // (a group of their own: see mid_all_kernel's stage_px)
    };
    // norm1 + ReLU + 3-way split of the fetched values into A3[buf]
    auto stage = [&](int buf, int sample0, auto ns_tag) {
        constexpr int NS = decltype(ns_tag)::value;
        // one address register per call (empty asm: not folded, not hoisted out of the tile loop), everything else immediates
        unsigned w_idx = (unsigned)((buf * 3 * 2 * TS + sample0) * LDK + k0p);
        asm volatile("" : "+v"(w_idx));
        unsigned short *w = &A3[0][0][0][0][0] + w_idx;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            float a0, t0, a1, t1;
            norm_relu(kA, rp[i].x, rt[i].x, &a0, &t0);
            norm_relu(kB, rp[i].y, rt[i].y, &a1, &t1);
            unsigned wa[3], wt[3];
            split3_pair(a0, a1, wa[0], wa[1], wa[2]);
            split3_pair(t0, t1, wt[0], wt[1], wt[2]);
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                *reinterpret_cast<unsigned *>(w + (part * 2 + 0) * TS * LDK + i * LDK) = wa[part];
                *reinterpret_cast<unsigned *>(w + (part * 2 + 1) * TS * LDK + i * LDK) = wt[part];
            }
        }
    };
    std::integral_constant<int, 4> HALF;
    const int s_half = 4 * wave, s_full = 8 * wq;              // first sample a wave stages in the two modes

    // weight fragments: buffer descriptor + ring (mid_products)
    bf16x8 ring[3][3];
    const unsigned b_lane = (unsigned)(h * 3 * NC * 8 + (wq * 32 + r) * 8) * 2u;      // bytes
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short *>(B3), 0, (int)((size_t)8 * MAX_BLOCKS * C1 * NC * 3 * 2), 0x00020000);
    auto ring_init = [&]() {                                   // the first two steps of pixel 0 (ring slots 0, 1)
        const int cb0 = wg == 0 ? MidGeom::prod_cb(0, MidGeom::pix(0), 0) : MidGeom::prod_cb(1, MidGeom::pix(0), 0);
        const int cb1 = wg == 0 ? MidGeom::prod_cb(0, MidGeom::pix(0), 1) : MidGeom::prod_cb(1, MidGeom::pix(0), 1);
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            ring[0][part] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, (cb0 * KS * 2 * 3 + part) * NC * 8 * 2, 0));
            ring[1][part] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, (cb1 * KS * 2 * 3 + part) * NC * 8 * 2, 0));
        }
    };
    // stores + statistics of one tile's accumulators (this wave's four chunks), then the accumulators start over
    auto epilogue = [&](int tile) {
        tile = phys(tile);
        const int group = tile / tiles_per_group;
        int64_t cnt_g = n_edges - (e_base + (int64_t)(group >> 1) * batch);
        if (cnt_g > batch) cnt_g = batch;
        const int n_valid = (int)cnt_g - (tile - group * tiles_per_group) * TS;
        const size_t tbase = (size_t)tile * TS * n2;
        const __amdgpu_buffer_rsrc_t p_dst = __builtin_amdgcn_make_buffer_rsrc(pre2 + tbase, 0, TS * n2 * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t t_dst = __builtin_amdgcn_make_buffer_rsrc(tpre2 + tbase, 0, TS * n2 * 4, 0x00020000);
        Bn2Sums sums;
#pragma unroll
        for (int lc = 0; lc < NL; ++lc) {
            const int ch = wg == 0 ? MidGeom::chunk_of(0, lc) : MidGeom::chunk_of(1, lc);
            const int op = lo == 0 ? MidGeom::opix(ch, 0) : MidGeom::opix(ch, 1);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
                const float x = accp[lc][q] + bias, t = acct[lc][q];
                const int soff = (((q & 3) + 8 * (q >> 2)) * n2 + op * c2) * 4;          // scalar; the lane adds v_out
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(x), p_dst, v_out, soff, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(t), t_dst, v_out, soff, 0);
                bn2_add(sums, x, t, row < n_valid);
            }
        }
        if (want_stats) bn2_store(sums, partial2, tile, wg * 2 + (wq >> 1), co, lane);
        zero_acc();
    };

    const unsigned short *a3 = &A3[0][0][0][0][0];
    const unsigned a_lane = (unsigned)(r * LDK + h * 8);
    constexpr unsigned A_BUF = 3u * 2u * TS * LDK;
#define GEO_PIPE_PIXEL(WGV, IPV)                                                                                       \
    mid_products<C1, false, WGV, IPV>(a3, a_lane + ((IPV) & 1) * A_BUF, b_rsrc, b_lane, accp, acct, ring)

    // "all samples" by one group = two passes of four samples per wave through the same registers: the first four were fetched
    // an interval ago, the second four are fetched behind the first staging and their latency is exposed -- in a group that has
    // 10 000 cycles of slack in that interval (the other group is in its epilogue)
#define GEO_PIPE_SEP() __builtin_amdgcn_sched_barrier(0)
#define GEO_STAGE_FULL(BUF, TILE, PX)                                                                                   \
    { stage(BUF, s_full, HALF); fetch(TILE, PX, s_full + 4, HALF); GEO_PIPE_SEP(); stage(BUF, s_full + 4, HALF); }

    // ---- prologue: pixel 0 of the first tile, staged by halves; group 0 already fetches the first half of its pixel 1
    int tile = blockIdx.x;
    load_consts(tile);
    fetch(tile, 0, s_half, HALF);
    ring_init();
    stage(0, s_half, HALF);
    if (wg == 0) fetch(tile, 1, s_full, HALF);
    else fetch(tile, 2, s_half, HALF);
    // Matrix-pipe priority to the group whose vector work (staging, epilogue) FOLLOWS its products in an interval -- group 0 in all
    // four: its MFMAs go first and its tail runs beside group 1's MFMAs.  (Measured the other way round, -DGEO_MID_PROF: group 1's
    // products first, then group 0's, then group 0's staging alone: 18 400 cycles for an interval whose pipe work is 15 300.)
    if (wg == 0) __builtin_amdgcn_s_setprio(1);
    lds_barrier();
    // (one tile loop per wave group: both run the same number of barriers per tile; separate loops keep the register allocator
    // from reconciling the two groups' live ranges at every iteration)
#ifdef GEO_MID_PROF
    unsigned long long pb_prev = __builtin_amdgcn_s_memtime(), pb_wait = 0;
#define GEO_PB(slot)                                                                                                   \
    { const unsigned long long t_a = __builtin_amdgcn_s_memtime();                                                      \
      lds_barrier();                                                                                                    \
      const unsigned long long t_b = __builtin_amdgcn_s_memtime();                                                      \
      if (lane == 0 && wq == 0) { atomicAdd(&g_mid_prof[wg][1 + slot], t_a - pb_prev); atomicAdd(&g_mid_prof[wg][5], t_b - t_a);   \
                                  if (slot == 3) atomicAdd(&g_mid_prof[wg][7], 1ull); }                                 \
      pb_prev = t_b; }
#else
#define GEO_PB(slot) lds_barrier();
#endif
    if (wg == 0) {
        for (int it = 0; it < my_tiles; ++it) {
            const int next = tile + (int)gridDim.x;
            const bool has_next = it + 1 < my_tiles;
            GEO_PIPE_PIXEL(0, 0); GEO_PIPE_SEP();
            GEO_STAGE_FULL(1, tile, 1); fetch(tile, 2, s_half, HALF); GEO_PB(0);
            GEO_PIPE_PIXEL(0, 1); GEO_PIPE_SEP(); stage(0, s_half, HALF); fetch(tile, 3, s_half, HALF); GEO_PB(1);
            GEO_PIPE_PIXEL(0, 2); GEO_PIPE_SEP(); stage(1, s_half, HALF); GEO_PB(2);
            GEO_PIPE_PIXEL(0, 3); GEO_PIPE_SEP();
            epilogue(tile);
            GEO_PIPE_SEP();
            if (has_next) { load_consts(next); fetch(next, 1, s_full, HALF); ring_init(); }
            GEO_PB(3);
            tile = next;
        }
    } else {
        // (raising group 1's priority for its vector phases -- staging, epilogue -- was measured: 18.0 ms against 17.7 ms, they slow
        // group 0's product stream more than they gain)
        for (int it = 0; it < my_tiles; ++it) {
            const int next = tile + (int)gridDim.x;
            const bool has_next = it + 1 < my_tiles;
            if (it > 0) { epilogue(tile - (int)gridDim.x); GEO_PIPE_SEP(); ring_init(); }
            GEO_PIPE_PIXEL(1, 0); GEO_PB(0);
            stage(0, s_half, HALF); fetch(tile, 3, s_half, HALF); GEO_PIPE_SEP();
            GEO_PIPE_PIXEL(1, 1); GEO_PB(1);
            stage(1, s_half, HALF);
            if (has_next) { load_consts(next); fetch(next, 0, s_full, HALF); }
            GEO_PIPE_SEP();
            GEO_PIPE_PIXEL(1, 2); GEO_PB(2);
            if (has_next) { GEO_STAGE_FULL(0, next, 0); fetch(next, 2, s_half, HALF); }
            GEO_PIPE_SEP();
            GEO_PIPE_PIXEL(1, 3); GEO_PB(3);
            tile = next;
        }
        epilogue(tile - (int)gridDim.x);                         // the last tile of group 1
    }
#undef GEO_STAGE_FULL
#undef GEO_PIPE_SEP
#undef GEO_PB
#undef GEO_PIPE_PIXEL
}

// ---- start side of train-mode BatchNorm, graph edges (jvp_start_dedup) ------------------------------------------------------
// The edge list is row-major (src ascending), so a chunk's start-side slots hold runs of one latent.  Their primal rows are the same
// function of (latent, the group's BatchNorm constants): ConvT2 / ConvT3 run them once per run.  Per start group (= chunk):
//   row_map[slot]      absolute index of the slot's compact primal row (compact row k of group g lives at slot position g * spg + k,
//                      where the start side no longer keeps per-slot primal rows; padding slots: compact row 0)
//   rep[g * spg + k]   the slot whose pre-activations feed compact row k (the first slot of its run); rows k in [cnt, cnt rounded up
//                      to TS) repeat the group's first slot (padding of the last compact tile)
//   n_compact[chunk]   cnt, the number of runs
// No sorting: an unsorted list only has shorter runs.
__global__ __launch_bounds__(256) void start_runs_kernel(const int32_t *__restrict__ src, int64_t e_base, int64_t n_edges, int batch,
                                                        int slots_per_group, int32_t *__restrict__ row_map, int32_t *__restrict__ rep,
                                                        int32_t *__restrict__ n_compact) {
    __shared__ int wsum[4];
    __shared__ int carry_s;
    const int chunk = blockIdx.x;
    const size_t g0 = (size_t)chunk * 2 * slots_per_group;     // first slot of the start group
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;                                             // runs before this block of 256 slots
    for (int w0 = 0; w0 < slots_per_group; w0 += 256) {
        const int within = w0 + (int)threadIdx.x;
        const int64_t e = e_base + (int64_t)chunk * batch + within;
        const bool valid = within < slots_per_group && within < batch && e < n_edges;
        const bool head = valid && start_run_head(src, e, within);
        const unsigned long long m = __ballot(head);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int before = carry, total = carry;
        for (int w = 0; w < 4; ++w) { if (w < wave) before += wsum[w]; total += wsum[w]; }
        const int k = before + below + (head ? 1 : 0) - 1;     // index of the run this slot belongs to
        if (within < slots_per_group) {
            row_map[g0 + within] = (int32_t)(g0 + (valid ? k : 0));
            if (head) rep[g0 + k] = (int32_t)(g0 + within);
        }
        carry = total;
        __syncthreads();                                       // wsum reused
    }
    if (threadIdx.x == 0) { carry_s = carry; n_compact[chunk] = carry; }
    __syncthreads();
    const int cnt = carry_s, padded = (cnt + TS - 1) / TS * TS;
    for (int k = cnt + (int)threadIdx.x; k < padded; k += 256) rep[g0 + k] = (int32_t)g0;
}

// ConvT2 of the start side in full 64-row tiles of two independent 32-row halves, both of one start group (one set of constants):
//   TT = true   halves = the tangents of start tiles 2j and 2j + 1 of the group (their own pre1 rows give the BN1 / ReLU terms);
//               tangent rows -> tpre2, and the tiles' BN2 partial sums with the primal gathered from the compact rows (bn2_partial),
//               so this launch follows the TT = false one.  ONCE (jvp_front_once, front_edge_kernel): a start slot has no rows
//               of its own; its primal is the row of its run's head, rep[row_map[slot]] (~33 L2-resident rows per chunk, padding
//               slots: the group's first head), its tangent the row of the partner end slot, one group further on
//   TT = false  halves = compact primal tiles 2j and 2j + 1 (rows gathered through rep) -> the compact rows of pre2
// Same staging arithmetic, products (mid_products) and order as mid_all_kernel / mid_pipe_kernel: every row is bit-identical to the
// row those kernels compute for the same inputs.  grid = (ceil(tiles_per_group / 2), chunks of the pass), 512 threads.
template <bool TT, bool ONCE = false>
__global__ __launch_bounds__(512, 2) void mid_start_kernel(const float *__restrict__ pre1, const float *__restrict__ tpre1,
                                                          const NormConst *__restrict__ consts1, int tiles_per_group,
                                                          const unsigned short *__restrict__ B3, const float *__restrict__ b2,
                                                          float *__restrict__ pre2, float *__restrict__ tpre2,
                                                          double *__restrict__ partial2, const int32_t *__restrict__ row_map,
                                                          const int32_t *__restrict__ rep, const int32_t *__restrict__ n_compact,
                                                          int64_t e_base, int64_t n_edges, int batch) {
    constexpr int C1 = 128, LDK = C1 + 8, KS = C1 / 16, NL = 4, c2 = 64, n1 = 4 * C1, n2 = 16 * c2;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) unsigned short A3[2][3][2][TS][LDK];   // [buf][part][half][row][k]
    const int chunk = blockIdx.y, group = 2 * chunk;
    const int ncomp = TT ? 0 : n_compact[chunk];
    // (the compact launch runs one workgroup per chunk over its few tile pairs: empty workgroups are not free -- a launch is bound by
    // the wave dispatch rate, ~25 ns per wave across the chip, and a per-pair grid is 8 mostly empty 8-wave workgroups per chunk)
    auto run = [&](int item) {
    const int lt0 = 2 * item;                                   // local tile of half 0 (half 1: lt0 + 1)
    const bool live1 = TT ? lt0 + 1 < tiles_per_group : (lt0 + 1) * TS < ncomp;
    const int tile0 = group * tiles_per_group + lt0, tile1 = live1 ? tile0 + 1 : tile0;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wq = wave & 3, wg = wave >> 2;
    const int r = lane & 31, h = lane >> 5;
    f32x16 accp[NL], acct[NL];
#pragma unroll
    for (int lc = 0; lc < NL; ++lc)
#pragma unroll
        for (int i = 0; i < 16; ++i) { accp[lc][i] = 0.f; acct[lc][i] = 0.f; }

    // staging (mid_all_kernel's channel-pair layout): lane -> channels 2 lane, 2 lane + 1; wave -> rows 4 wave .. 4 wave + 3 of both halves
    const int k0p = 2 * lane, s0p = 4 * wave;
    const NormConst *kp = consts1 + (size_t)group * C1 + k0p;
    const NormConst kA = kp[0], kB = kp[1];
    static_assert(TT || !ONCE, "ONCE selects where the tangent launch reads");
    size_t xrow[2][4];                                          // pre1 rows feeding the wave's staging rows (wave-uniform)
    // ONCE: both row sets as scalar byte offsets into two buffer descriptors, the start group's pre1 (the heads) and the end
    // group's tpre1 (the partner slots); the lane adds one loop-invariant offset (mid_pipe_kernel's fetch)
    const size_t g0 = (size_t)group * tiles_per_group * TS, group_slots = (size_t)tiles_per_group * TS;
    unsigned xoff[2][4], toff[2];
    __amdgpu_buffer_rsrc_t x_src, t_src;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const size_t s0 = (size_t)tile0 * TS + s0p + i, s1 = (size_t)tile1 * TS + s0p + i;
        if (ONCE) {
            xoff[0][i] = (unsigned)(__builtin_amdgcn_readfirstlane(rep[__builtin_amdgcn_readfirstlane(row_map[s0])]) - (int)g0) * (n1 * 4u);
            xoff[1][i] = (unsigned)(__builtin_amdgcn_readfirstlane(rep[__builtin_amdgcn_readfirstlane(row_map[s1])]) - (int)g0) * (n1 * 4u);
        } else {
            xrow[0][i] = TT ? s0 : (size_t)__builtin_amdgcn_readfirstlane(rep[s0]);
            xrow[1][i] = TT ? s1 : (size_t)__builtin_amdgcn_readfirstlane(rep[s1]);
        }
    }
    if (ONCE) {
        x_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pre1 + g0 * n1), 0, (int)(group_slots * n1 * 4), 0x00020000);
        t_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(tpre1 + (g0 + group_slots) * n1), 0, (int)(group_slots * n1 * 4), 0x00020000);
        toff[0] = (unsigned)(lt0 * TS + s0p) * (n1 * 4u);
        toff[1] = (unsigned)((live1 ? lt0 + 1 : lt0) * TS + s0p) * (n1 * 4u);
    }
    const unsigned v_pair = (unsigned)k0p * 4u;
    f32x2 rx[2][4], rt[2][4];
    auto fetch = [&](int nx) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (ONCE) {
                    const int px_off = MidGeom::pix(nx) * C1 * 4;
                    rx[hh][i] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(x_src, v_pair, xoff[hh][i] + px_off, 0));
                    rt[hh][i] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(t_src, v_pair, toff[hh] + i * n1 * 4 + px_off, 0));
                    continue;
                }
                const size_t off = xrow[hh][i] * n1 + (size_t)MidGeom::pix(nx) * C1 + k0p;
                rx[hh][i] = *reinterpret_cast<const f32x2 *>(pre1 + off);
                if (TT) rt[hh][i] = *reinterpret_cast<const f32x2 *>(tpre1 + off);
            }
    };
    fetch(0);
    auto stage_px = [&](int buf, int nx) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float a0, t0, a1, t1;
                norm_relu(kA, rx[hh][i].x, TT ? rt[hh][i].x : 0.f, &a0, &t0);
                norm_relu(kB, rx[hh][i].y, TT ? rt[hh][i].y : 0.f, &a1, &t1);
                unsigned w[3];
                if (TT) split3_pair(t0, t1, w[0], w[1], w[2]);
                else split3_pair(a0, a1, w[0], w[1], w[2]);
#pragma unroll
                for (int part = 0; part < 3; ++part) *reinterpret_cast<unsigned *>(&A3[buf][part][hh][s0p + i][k0p]) = w[part];
            }
        if (nx < 4) {
            fetch(nx);
            __builtin_amdgcn_sched_group_barrier(0x020, TT ? 16 : 8, 0);
        }
    };
    bf16x8 ring[3][3];
    const unsigned b_lane = (unsigned)(h * 3 * NC * 8 + (wq * 32 + r) * 8) * 2u;      // bytes
    const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned short *>(B3), 0, (int)((size_t)8 * MAX_BLOCKS * C1 * NC * 3 * 2), 0x00020000);
    {
        const int cb0 = wg == 0 ? MidGeom::prod_cb(0, MidGeom::pix(0), 0) : MidGeom::prod_cb(1, MidGeom::pix(0), 0);
        const int cb1 = wg == 0 ? MidGeom::prod_cb(0, MidGeom::pix(0), 1) : MidGeom::prod_cb(1, MidGeom::pix(0), 1);
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            ring[0][part] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, (cb0 * KS * 2 * 3 + part) * NC * 8 * 2, 0));
            ring[1][part] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_lane, (cb1 * KS * 2 * 3 + part) * NC * 8 * 2, 0));
        }
    }
    stage_px(0, 1);
    if (wg == 1) __builtin_amdgcn_s_setprio(1);
    lds_barrier();
    const unsigned short *a3 = &A3[0][0][0][0][0];
    const unsigned a_lane = (unsigned)(r * LDK + h * 8);
    constexpr unsigned A_BUF = 3u * 2u * TS * LDK;
#define GEO_MID_PIXEL(WGV, IPV) mid_products<C1, false, WGV, IPV>(a3, a_lane + ((IPV) & 1) * A_BUF, b_rsrc, b_lane, accp, acct, ring)
    if (wg == 0) {
        GEO_MID_PIXEL(0, 0); stage_px(1, 2); lds_barrier();
        GEO_MID_PIXEL(0, 1); stage_px(0, 3); lds_barrier();
        GEO_MID_PIXEL(0, 2); stage_px(1, 4); lds_barrier();
        GEO_MID_PIXEL(0, 3);
    } else {
        stage_px(1, 2); GEO_MID_PIXEL(1, 0); lds_barrier();
        stage_px(0, 3); GEO_MID_PIXEL(1, 1); lds_barrier();
        stage_px(1, 4); GEO_MID_PIXEL(1, 2); lds_barrier();
        GEO_MID_PIXEL(1, 3);
    }
#undef GEO_MID_PIXEL

    // epilogue: C[row = (q & 3) + 8 (q >> 2) + 4 h][col = lane & 31]; column -> (output pixel lo of the chunk, channel co)
    const int lo = wq >> 1, co = (wq & 1) * 32 + r;
    const float bias = TT ? 0.f : b2[co];                       // (the primal rows carry the bias, the tangents do not)
    float *dst = TT ? tpre2 : pre2;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        if (hh == 1 && !live1) break;
        const size_t tbase = (size_t)(hh ? tile1 : tile0) * TS;
#pragma unroll
        for (int lc = 0; lc < NL; ++lc) {
            const int ch = wg == 0 ? MidGeom::chunk_of(0, lc) : MidGeom::chunk_of(1, lc);
            const int op = lo == 0 ? MidGeom::opix(ch, 0) : MidGeom::opix(ch, 1);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
                const float v = hh ? acct[lc][q] : accp[lc][q];
                dst[(tbase + row) * n2 + (size_t)op * c2 + co] = TT ? v : v + bias;
            }
        }
    }
    if (TT) {                                                  // BN2 partial sums of both tiles, primal from the compact rows
        int64_t cnt_g = n_edges - (e_base + (int64_t)chunk * batch);
        if (cnt_g > batch) cnt_g = batch;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            if (hh == 1 && !live1) break;
            const int tile = hh ? tile1 : tile0;
            const size_t tbase = (size_t)tile * TS;
            const int n_valid = (int)cnt_g - (tile - group * tiles_per_group) * TS;
            Bn2Sums sums;
#pragma unroll
            for (int lc = 0; lc < NL; ++lc) {
                const int ch = wg == 0 ? MidGeom::chunk_of(0, lc) : MidGeom::chunk_of(1, lc);
                const int op = lo == 0 ? MidGeom::opix(ch, 0) : MidGeom::opix(ch, 1);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
                    const float x = pre2[(size_t)row_map[tbase + row] * n2 + (size_t)op * c2 + co];
                    bn2_add(sums, x, hh ? acct[lc][q] : accp[lc][q], row < n_valid);
                }
            }
            bn2_store(sums, partial2, tile, wg * 2 + (wq >> 1), co, lane);
        }
    }
    };
    if (TT) {
        run((int)blockIdx.x);
    } else {
        for (int item = 0; 2 * item * TS < ncomp; ++item) {
            if (item > 0) { __builtin_amdgcn_s_setprio(0); __syncthreads(); }   // (A3 is staged again by the next pair)
            run(item);
        }
    }
}

__global__ __launch_bounds__(256) void slot_valid_kernel(int64_t e_base, int64_t n_edges, int batch, int tiles_per_group,
                                                        int64_t n_slots, int32_t *__restrict__ slot_valid) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t per_group = (int64_t)tiles_per_group * TS;
        const int64_t g = i / per_group, within = i % per_group;
        const int64_t e = e_base + (g >> 1) * batch + within;
        slot_valid[i] = (within < batch && e < n_edges) ? 1 : 0;
    }
}

// per-node primal: the latent of every slot (start side: src, end side: dst; padding slots: latent 0)
__global__ __launch_bounds__(256) void slot_node_kernel(const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                                       int64_t e_base, int64_t n_edges, int batch, int tiles_per_group,
                                                       int64_t n_slots, int32_t *__restrict__ slot_node) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t per_group = (int64_t)tiles_per_group * TS;
        const int64_t g = i / per_group, within = i % per_group;
        const int64_t e = e_base + (g >> 1) * batch + within;
        slot_node[i] = (within < batch && e < n_edges) ? ((g & 1) ? dst[e] : src[e]) : 0;
    }
}

// ---------------------------------------------------------------------------------- back
// One workgroup = BACK_TS sample slots.  LDS (dynamic): a2 / ta2 [BACK_TS][16 px][c2] after norm2 + ReLU,
// the packed ConvT3 taps W3p [16][co][c2], and the squared tangent outputs.  A work item is
// (sample, output element, channel quarter): the 4 quarters of a dot product sit in adjacent lanes and are
// summed with two shuffles, so all 256 threads are busy even for the 16-pixel FashionMNIST head.
__global__ __launch_bounds__(256) void back_kernel(const float *__restrict__ pre2, const float *__restrict__ tpre2,
                                                  const NormConst *__restrict__ consts2, int consts_per_group,
                                                  int slots_per_group, int c2, int co_n, int s_out, int pad3,
                                                  const float *__restrict__ W3p, const float *__restrict__ b3,
                                                  float *__restrict__ norms) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n2 = 16 * c2;
    const int p_out = co_n * s_out * s_out;
    const int ldc = c2 + 4;                             // padded pixel row: neighbouring pixels / taps start on
    const int lds_n2 = 16 * ldc;                        // different LDS banks (c2 is a multiple of the bank cycle)
    float *a2 = smem;                                   // [BACK_TS][16][ldc]
    float *ta2 = a2 + (size_t)BACK_TS * lds_n2;         // [BACK_TS][16][ldc]
    float *w3 = ta2 + (size_t)BACK_TS * lds_n2;         // [16 taps * co_n][ldc]
    float *jt2 = w3 + (size_t)16 * co_n * ldc;          // [BACK_TS][p_out]
    const size_t slot0 = (size_t)blockIdx.x * BACK_TS;
    const int group = (int)(slot0 / slots_per_group);
    const NormConst *kc = consts2 + (size_t)(consts_per_group ? group : 0) * c2;
    {
        const float4 *xp4 = reinterpret_cast<const float4 *>(pre2 + slot0 * n2);
        const float4 *xt4 = reinterpret_cast<const float4 *>(tpre2 + slot0 * n2);
        const int c4n = c2 / 4;
        for (int i = threadIdx.x; i < BACK_TS * n2 / 4; i += 256) {
            const float4 x = xp4[i], t = xt4[i];
            const int c = (i % c4n) * 4, row = i / c4n;              // row = s*16 + px
            float4 a, ta;
            norm_relu(kc[c], x.x, t.x, &a.x, &ta.x);
            norm_relu(kc[c + 1], x.y, t.y, &a.y, &ta.y);
            norm_relu(kc[c + 2], x.z, t.z, &a.z, &ta.z);
            norm_relu(kc[c + 3], x.w, t.w, &a.w, &ta.w);
            *reinterpret_cast<float4 *>(a2 + (size_t)row * ldc + c) = a;
            *reinterpret_cast<float4 *>(ta2 + (size_t)row * ldc + c) = ta;
        }
        for (int i = threadIdx.x; i < 16 * co_n * c2; i += 256) w3[(size_t)(i / c2) * ldc + (i % c2)] = W3p[i];
    }
    __syncthreads();
    const int qlen = c2 / 4;                             // c2 is a multiple of 16 (checked on the host)
    for (int item = threadIdx.x; item < BACK_TS * p_out * 4; item += 256) {
        const int q = item & 3, so = item >> 2;
        const int s = so / p_out, o = so % p_out;
        const int co = o / (s_out * s_out), oy = (o / s_out) % s_out, ox = o % s_out;
        float x = 0.f, t = 0.f;
        for (int iy = 0; iy < 4; ++iy) {
            const int ky = oy + pad3 - 2 * iy;
            if (ky < 0 || ky > 3) continue;
            for (int ix = 0; ix < 4; ++ix) {
                const int kx = ox + pad3 - 2 * ix;
                if (kx < 0 || kx > 3) continue;
                const float4 *w = reinterpret_cast<const float4 *>(w3 + ((size_t)(ky * 4 + kx) * co_n + co) * ldc + q * qlen);
                const float4 *pa = reinterpret_cast<const float4 *>(a2 + ((size_t)s * 16 + iy * 4 + ix) * ldc + q * qlen);
                const float4 *pt = reinterpret_cast<const float4 *>(ta2 + ((size_t)s * 16 + iy * 4 + ix) * ldc + q * qlen);
                for (int c4 = 0; c4 < qlen / 4; ++c4) {
                    const float4 wv = w[c4], av = pa[c4], tv = pt[c4];
                    x = fmaf(av.x, wv.x, x); x = fmaf(av.y, wv.y, x); x = fmaf(av.z, wv.z, x); x = fmaf(av.w, wv.w, x);
                    t = fmaf(tv.x, wv.x, t); t = fmaf(tv.y, wv.y, t); t = fmaf(tv.z, wv.z, t); t = fmaf(tv.w, wv.w, t);
                }
            }
        }
        x += __shfl_xor(x, 1, 64); t += __shfl_xor(t, 1, 64);
        x += __shfl_xor(x, 2, 64); t += __shfl_xor(t, 2, 64);
        if (q == 0) {
            x += b3[co];
            const float sg = 1.0f / (1.0f + expf(-x));
            const float j = t * sg * (1.0f - sg);
            jt2[so] = j * j;
        }
    }
    __syncthreads();
    // fixed-order fp64 sum per sample by one wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < BACK_TS; s += 4) {
        double acc = 0.0;
        for (int o = lane; o < p_out; o += 64) acc += (double)jt2[s * p_out + o];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) norms[slot0 + s] = (float)sqrt(acc);
    }
}

// ---------------------------------------------------------------------------------- back on the matrix cores
// ConvT3 as a [32 samples x 1024] x [1024 x P] product (P = 16 or 192 outputs, padded to 32-column tiles; taps that
// fall outside the 4x4 kernel are zeros in the packed weights), same exact bf16 x 3 split as the mid kernel.
// The 1024-deep reduction is cut into 8 blocks of 128 (two input pixels); inside a block the four waves take two
// 16-deep steps each, and their partial tiles are summed through LDS before sigmoid' and the squared norm.
// W3b[kb 8][part 3][ks 8][h 2][NP][8] bf16
__global__ __launch_bounds__(256) void pack_back_bf16_kernel(const float *__restrict__ w3, int c2, int co_n, int s_out,
                                                            int pad3, int np, unsigned short *__restrict__ W3b) {
    const int K = 16 * c2, P = co_n * s_out * s_out;
    const size_t total = (size_t)K * np;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int o = (int)(i % np), k = (int)(i / np);
        float v = 0.f;
        if (o < P) {
            const int ip = k / c2, ci = k % c2, iy = ip >> 2, ix = ip & 3;
            const int co = o / (s_out * s_out), oy = (o / s_out) % s_out, ox = o % s_out;
            const int ky = oy + pad3 - 2 * iy, kx = ox + pad3 - 2 * ix;
            if (ky >= 0 && ky < 4 && kx >= 0 && kx < 4) v = w3[(((size_t)ci * co_n + co) * 4 + ky) * 4 + kx];
        }
        unsigned short q[3];
        split3(v, q[0], q[1], q[2]);
        const int kb = k >> 7, kk = k & 127, ks = kk >> 4, h = (kk >> 3) & 1, j = kk & 7;
        for (int part = 0; part < 3; ++part)
            W3b[((((size_t)kb * 3 + part) * 8 + ks) * 2 + h) * (size_t)np * 8 + (size_t)o * 8 + j] = q[part];
    }
}

// MODE 0: primal + tangent of every slot -> |J dz| per slot.
// Start side with compact primal rows (jvp_start_dedup, start_runs_kernel): MODE 2 runs over the compact tiles (n_compact), MODE 1 over the start tiles with row_map as the slot -> primal row map; sg_node is then indexed by the
// compact row.  side_only: 0 = every tile of the pass, 1 = start-side tiles only, 2 = end-side tiles only (grid = half the tiles);
// with n_compact the grid is one workgroup per chunk.
// Per-node primal (decoders with fixed statistics; run_jvp): MODE 2 runs over the LATENTS, primal only, and stores the
// sigmoid of every output (sg_node [node][NP]); MODE 1 runs over the edge slots, tangent only: the ReLU mask comes from the
// slot's node row of pre2 (gathered), sigmoid' from sg_node -- the same products in the same order as MODE 0.
template <int NT, bool GN, int MODE = 0>
__global__ __launch_bounds__(256, 2) void back_mfma_kernel(const float *__restrict__ pre2, const float *__restrict__ tpre2,
                                                       const NormConst *__restrict__ consts2, int consts_per_group,
                                                       int tiles_per_group, int co_n, int s_out,
                                                       const unsigned short *__restrict__ W3b,
                                                       const float *__restrict__ b3, float *__restrict__ norms,
                                                       const float4 *__restrict__ gs2, float *__restrict__ sg_node = nullptr,
                                                       const int32_t *__restrict__ src = nullptr,
                                                       const int32_t *__restrict__ dst = nullptr, int64_t e_base = 0,
                                                       int64_t n_edges = 0, int batch = 1, float *__restrict__ jac_node = nullptr,
                                                       int unit_d = 0, const int32_t *__restrict__ row_map = nullptr,
                                                       const int32_t *__restrict__ n_compact = nullptr, int side_only = 0) {
    constexpr int C2 = 64, KB = 128, LDK = KB + 8, NP = NT * 32;
    __shared__ __attribute__((aligned(16))) unsigned short A3[3][2][TS][LDK];     // 52 KB, reused for the reduction
    __shared__ NormConst kc[C2];
    __shared__ float4 gsl[GN ? TS : 1][32];                                       // GroupNorm: per (sample, group)
    // (n_compact: one workgroup per chunk walks the chunk's compact tiles -- see mid_start_kernel on empty workgroups)
    const int n_iter = MODE == 2 && n_compact ? (n_compact[blockIdx.x] + TS - 1) / TS : 1;
    for (int it = 0; it < n_iter; ++it) {
    if (it > 0) __syncthreads();                               // (LDS staged again)
    const int tile = MODE == 2 && n_compact ? (int)blockIdx.x * 2 * tiles_per_group + it
                   : side_only ? (((int)blockIdx.x / tiles_per_group) * 2 + side_only - 1) * tiles_per_group +
                                     (int)blockIdx.x % tiles_per_group
                               : (int)blockIdx.x;
    const int group = tile / tiles_per_group;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n2 = 16 * C2, P = co_n * s_out * s_out;
    const size_t slot0 = (size_t)tile * TS;
    for (int c = threadIdx.x; c < C2; c += 256) kc[c] = consts2[(size_t)(consts_per_group ? group : 0) * C2 + c];
    if (GN)
        for (int i = threadIdx.x; i < TS * 32; i += 256) gsl[i >> 5][i & 31] = gs2[slot0 * 32 + i];

    f32x16 accp[NT], acct[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 16; ++i) { accp[nt][i] = 0.f; acct[nt][i] = 0.f; }

    const int r = lane & 31, h = lane >> 5;
    const int ss = threadIdx.x >> 3, k0 = (threadIdx.x & 7) * 16;
    // MODE 1: the latent a slot belongs to (start side: src, end side: dst; padding slots read latent 0, their result is unused)
    auto edge_of = [&](int sample) -> int64_t {                   // -1: padding slot
        const int tg = tile - group * tiles_per_group;
        const int64_t e = e_base + (int64_t)(group >> 1) * batch + (int64_t)tg * TS + sample;
        return (tg * TS + sample >= batch || e >= n_edges) ? -1 : e;
    };
    auto node_of = [&](int sample) -> size_t {
        const int64_t e = edge_of(sample);
        return e < 0 ? 0 : (size_t)((group & 1) ? dst[e] : src[e]);
    };
    const size_t prow = MODE == 1 ? (row_map ? (size_t)row_map[slot0 + ss] : node_of(ss)) : slot0 + ss;   // row of the primal this thread stages
    for (int kb = 0; kb < 8; ++kb) {
        __syncthreads();
        {
            const float *xp = pre2 + prow * n2 + (size_t)kb * KB + k0;
            const float *xt = (MODE == 2 ? pre2 : tpre2) + (slot0 + ss) * n2 + (size_t)kb * KB + k0;
#pragma unroll
            for (int k8 = 0; k8 < 16; k8 += 8) {
                u16x8 pp[3], pt[3];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float a, ta;
                    const int c = (k0 + k8 + k) & (C2 - 1);
                    if (GN) norm_relu_gn(gsl[GN ? ss : 0][c >> 1], kc[c].sc, kc[c].beta, xp[k8 + k], xt[k8 + k], &a, &ta);
                    else norm_relu(kc[c], xp[k8 + k], xt[k8 + k], &a, &ta);
                    unsigned short q1, q2, q3;
                    if (MODE != 1) { split3(a, q1, q2, q3); pp[0][k] = q1; pp[1][k] = q2; pp[2][k] = q3; }
                    if (MODE != 2) { split3(ta, q1, q2, q3); pt[0][k] = q1; pt[1][k] = q2; pt[2][k] = q3; }
                }
#pragma unroll
                for (int part = 0; part < 3; ++part) {
                    if (MODE != 1) *reinterpret_cast<u16x8 *>(&A3[part][0][ss][k0 + k8]) = pp[part];
                    if (MODE != 2) *reinterpret_cast<u16x8 *>(&A3[part][1][ss][k0 + k8]) = pt[part];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int kq = 0; kq < 2; ++kq) {
            const int ks = wave * 2 + kq;                     // this wave's 16-deep steps of the block
            bf16x8 ap[3], at[3];
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                if (MODE != 1) ap[part] = *reinterpret_cast<const bf16x8 *>(&A3[part][0][r][ks * 16 + h * 8]);
                if (MODE != 2) at[part] = *reinterpret_cast<const bf16x8 *>(&A3[part][1][r][ks * 16 + h * 8]);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                bf16x8 b[3];
#pragma unroll
                for (int part = 0; part < 3; ++part)
                    b[part] = *reinterpret_cast<const bf16x8 *>(
                        W3b + ((((size_t)kb * 3 + part) * 8 + ks) * 2 + h) * (size_t)NP * 8 + (size_t)(nt * 32 + r) * 8);
                if (MODE != 1) accp[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[2], b[0], accp[nt], 0, 0, 0);
                if (MODE != 2) acct[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[2], b[0], acct[nt], 0, 0, 0);
                if (MODE != 1) accp[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[2], accp[nt], 0, 0, 0);
                if (MODE != 2) acct[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[2], acct[nt], 0, 0, 0);
                if (MODE != 1) accp[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[1], accp[nt], 0, 0, 0);
                if (MODE != 2) acct[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[1], acct[nt], 0, 0, 0);
                if (MODE != 1) accp[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[0], accp[nt], 0, 0, 0);
                if (MODE != 2) acct[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[0], acct[nt], 0, 0, 0);
                if (MODE != 1) accp[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[1], accp[nt], 0, 0, 0);
                if (MODE != 2) acct[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[1], acct[nt], 0, 0, 0);
                if (MODE != 1) accp[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[0], accp[nt], 0, 0, 0);
                if (MODE != 2) acct[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[0], acct[nt], 0, 0, 0);
            }
        }
    }
    // sum the four waves' partial tiles through LDS (one 32-column tile at a time), then sigmoid' and the norm
    float *red = reinterpret_cast<float *>(&A3[0][0][0][0]);     // [wave 4][p|t 2][32 rows][33]
    const int row = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    const size_t nrow = MODE == 1 ? (row_map ? (size_t)row_map[slot0 + row] : node_of(row)) : slot0 + row;   // sg_node row: the slot's latent / compact row (1), this row (2)
    // unit tangents: this slot's outputs are column e % unit_d of its latent's Jacobian, kept as jac_node[latent][dimension][NP]
    float *jrow = nullptr;
    if (MODE == 1 && jac_node) {
        const int64_t e = edge_of(row);
        if (e >= 0) jrow = jac_node + (nrow * unit_d + (size_t)(e % unit_d)) * NP;
    }
    double sumsq = 0.0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int rr = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
            if (MODE != 1) red[((wave * 2 + 0) * 32 + rr) * 33 + (lane & 31)] = accp[nt][q];
            if (MODE != 2) red[((wave * 2 + 1) * 32 + rr) * 33 + (lane & 31)] = acct[nt][q];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int o = nt * 32 + c4 + c;
            if (o < P) {
                float x = b3[o / (s_out * s_out)], t = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    if (MODE != 1) x += red[((w * 2 + 0) * 32 + row) * 33 + c4 + c];
                    if (MODE != 2) t += red[((w * 2 + 1) * 32 + row) * 33 + c4 + c];
                }
                const float sg = MODE == 1 ? sg_node[nrow * NP + o] : 1.0f / (1.0f + expf(-x));
                if (MODE == 2) sg_node[nrow * NP + o] = sg;
                const float j = t * sg * (1.0f - sg);
                if (MODE == 1 && jrow) jrow[o] = j;
                sumsq += (double)(j * j);
            }
        }
    }
    sumsq += __shfl_xor(sumsq, 1, 64);
    sumsq += __shfl_xor(sumsq, 2, 64);
    sumsq += __shfl_xor(sumsq, 4, 64);
    if (MODE != 2 && (threadIdx.x & 7) == 0) norms[slot0 + row] = (float)sqrt(sumsq);
    }
}

// The 16-output head without GroupNorm (route `head_stream`): back_mfma_kernel<1, false, MODE>'s staged values, products and epilogue
// bit for bit, scheduled so that the rows stream.  MODE 0: primal + tangent per slot (side_only as above).  MODE 1: the start-side
// tangents of the dedup route -- ReLU mask from the compact primal row (row_map), sigmoid' from sg_compact.
//   staging map   lane l of wave w stages channels 4 (l & 15) .. + 3 of pixel (l >> 4) & 1 of the K block, for the rows
//                 8 w + 2 i + (l >> 5), i = 0..3: one 16-byte load per row and operand, a wave's load covers two whole 512-byte row
//                 segments, and the four NormConst stay in registers for the tile (channel = k mod 64, the same in all 8 blocks).
//   loads         block kb + 1's rows are requested into a second register set while block kb is converted (rows 0, 1 before, rows
//                 2, 3 half way, into what rows 0, 1 of block kb leave free); the weights of block kb are requested before that, so
//                 waiting for them leaves the rows in flight (loads return in order).  Nothing is requested past the tile's own
//                 rows: block 7 prefetches nothing.
template <int MODE>
__global__ __launch_bounds__(256, 3) void head_stream_kernel(const float *__restrict__ pre2, const float *__restrict__ tpre2,
                                                         const NormConst *__restrict__ consts2, int consts_per_group,
                                                         int tiles_per_group, int co_n, int s_out,
                                                         const unsigned short *__restrict__ W3b, const float *__restrict__ b3,
                                                         float *__restrict__ norms, const float *__restrict__ sg_compact,
                                                         const int32_t *__restrict__ row_map, int side_only) {
    constexpr int C2 = 64, KB = 128, LDK = KB + 8, NP = 32, N2 = 16 * C2;
    __shared__ __attribute__((aligned(16))) unsigned short A3[3][2][TS][LDK];     // 52 KB, reused for the reduction
    const int tile = side_only ? (((int)blockIdx.x / tiles_per_group) * 2 + side_only - 1) * tiles_per_group +
                                     (int)blockIdx.x % tiles_per_group
                               : (int)blockIdx.x;
    const int group = tile / tiles_per_group;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = co_n * s_out * s_out;
    const size_t slot0 = (size_t)tile * TS;

    const int c0 = (lane & 15) * 4, kcol = ((lane >> 4) & 1) * C2 + c0, row0 = wave * 8 + (lane >> 5);
    NormConst kn[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) kn[c] = consts2[(size_t)(consts_per_group ? group : 0) * C2 + c0 + c];
    // Buffer descriptors (scalar) and one 32-bit lane offset each.  Tangents and MODE 0's primal: the tile's 32 rows.  MODE 1's primal:
    // the start group's rows, where row_map points (make_route keeps a group's rows below 2 GB).  The weights: W3b.
    const __amdgpu_buffer_rsrc_t t_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(tpre2 + slot0 * N2), 0, TS * N2 * 4, 0x00020000);
    const size_t g0 = (size_t)group * tiles_per_group * TS;
    const __amdgpu_buffer_rsrc_t p_src = MODE == 1
        ? __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pre2 + g0 * N2), 0, tiles_per_group * TS * N2 * 4, 0x00020000)
        : __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pre2 + slot0 * N2), 0, TS * N2 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t b_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(W3b), 0, 16 * C2 * NP * 3 * 2, 0x00020000);
    const unsigned t_lane = (unsigned)(row0 * N2 + kcol) * 4u;                    // row i: + i * 2 rows
    unsigned p_lane[MODE == 1 ? 4 : 1];
    if (MODE == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            p_lane[MODE == 1 ? i : 0] = (unsigned)(((size_t)row_map[slot0 + row0 + 2 * i] - g0) * N2 + kcol) * 4u;
    }
    auto load_rows = [&](int kb, int i0, float4 (&p)[4], float4 (&t)[4]) {     // rows i0, i0 + 1 of block kb
#pragma unroll
        for (int i = i0; i < i0 + 2; ++i) {
            const int soff = (i * 2 * N2 + kb * KB) * 4;
            p[i] = MODE == 1 ? __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(p_src, p_lane[MODE == 1 ? i : 0], kb * KB * 4, 0))
                             : __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(p_src, t_lane, soff, 0));
            t[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(t_src, t_lane, soff, 0));
        }
    };

    f32x16 accp, acct;
#pragma unroll
    for (int i = 0; i < 16; ++i) { accp[i] = 0.f; acct[i] = 0.f; }
    const int r = lane & 31, h = lane >> 5;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    const unsigned b_lane = (unsigned)(h * NP * 8 + r * 8) * 2u;

    // one K block: `p`, `t` hold its rows, `pn`, `tn` take the next block's
    auto block = [&](int kb, const float4 (&p)[4], const float4 (&t)[4], float4 (&pn)[4], float4 (&tn)[4]) {
        const bool more = kb + 1 < 8;
        bf16x8 b[2][3];
        __builtin_amdgcn_sched_barrier(0);                        // (not among the previous block's products: registers)
#pragma unroll
        for (int kq = 0; kq < 2; ++kq)
#pragma unroll
            for (int part = 0; part < 3; ++part)
                b[kq][part] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(
                    b_src, b_lane, (((kb * 3 + part) * 8 + wave_s * 2 + kq) * 2 * NP * 8) * 2, 0));
        if (more) load_rows(kb + 1, 0, pn, tn);
        __syncthreads();                                          // the previous block's operand reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i == 2) {                                         // rows 0, 1 are converted: their registers take the other half
                __builtin_amdgcn_sched_barrier(0);
                if (more) load_rows(kb + 1, 2, pn, tn);
                __builtin_amdgcn_sched_barrier(0);
            }
            float a[4], ta[4];
            norm_relu(kn[0], p[i].x, t[i].x, &a[0], &ta[0]);
            norm_relu(kn[1], p[i].y, t[i].y, &a[1], &ta[1]);
            norm_relu(kn[2], p[i].z, t[i].z, &a[2], &ta[2]);
            norm_relu(kn[3], p[i].w, t[i].w, &a[3], &ta[3]);
            const int row = row0 + 2 * i;
            unsigned lo[3], hi[3];
            if (MODE != 1) {
                split3_pair(a[0], a[1], lo[0], lo[1], lo[2]);
                split3_pair(a[2], a[3], hi[0], hi[1], hi[2]);
#pragma unroll
                for (int part = 0; part < 3; ++part)
                    *reinterpret_cast<uint2 *>(&A3[part][0][row][kcol]) = make_uint2(lo[part], hi[part]);
            }
            split3_pair(ta[0], ta[1], lo[0], lo[1], lo[2]);
            split3_pair(ta[2], ta[3], hi[0], hi[1], hi[2]);
#pragma unroll
            for (int part = 0; part < 3; ++part)
                *reinterpret_cast<uint2 *>(&A3[part][1][row][kcol]) = make_uint2(lo[part], hi[part]);
        }
        __syncthreads();
#pragma unroll
        for (int kq = 0; kq < 2; ++kq) {
            const int ks = wave * 2 + kq;                         // this wave's 16-deep steps of the block
            bf16x8 ap[3], at[3];
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                if (MODE != 1) ap[part] = *reinterpret_cast<const bf16x8 *>(&A3[part][0][r][ks * 16 + h * 8]);
                at[part] = *reinterpret_cast<const bf16x8 *>(&A3[part][1][r][ks * 16 + h * 8]);
            }
            if (MODE != 1) accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[2], b[kq][0], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[2], b[kq][0], acct, 0, 0, 0);
            if (MODE != 1) accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[kq][2], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[kq][2], acct, 0, 0, 0);
            if (MODE != 1) accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[kq][1], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[kq][1], acct, 0, 0, 0);
            if (MODE != 1) accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[1], b[kq][0], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[1], b[kq][0], acct, 0, 0, 0);
            if (MODE != 1) accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[kq][1], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[kq][1], acct, 0, 0, 0);
            if (MODE != 1) accp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap[0], b[kq][0], accp, 0, 0, 0);
            acct = __builtin_amdgcn_mfma_f32_32x32x16_bf16(at[0], b[kq][0], acct, 0, 0, 0);
        }
    };

    float4 pa[4], ta[4], pb[4], tb[4];
    load_rows(0, 0, pa, ta);
    load_rows(0, 2, pa, ta);
#pragma unroll                                                    // (unrolled: the register sets alternate by name, no copies)
    for (int kb = 0; kb < 8; kb += 2) {
        block(kb, pa, ta, pb, tb);
        block(kb + 1, pb, tb, pa, ta);
    }

    // sum the four waves' partial tiles through LDS, then sigmoid' and the norm (back_mfma_kernel's epilogue for NT = 1)
    float *red = reinterpret_cast<float *>(&A3[0][0][0][0]);     // [wave 4][p|t 2][32 rows][33]
    const int row = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    const size_t nrow = MODE == 1 ? (size_t)row_map[slot0 + row] : slot0 + row;   // sg_compact row: the slot's compact row
    double sumsq = 0.0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int rr = (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
        if (MODE != 1) red[((wave * 2 + 0) * 32 + rr) * 33 + (lane & 31)] = accp[q];
        red[((wave * 2 + 1) * 32 + rr) * 33 + (lane & 31)] = acct[q];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int o = c4 + c;
        if (o < P) {
            float x = b3[o / (s_out * s_out)], t = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (MODE != 1) x += red[((w * 2 + 0) * 32 + row) * 33 + c4 + c];
                t += red[((w * 2 + 1) * 32 + row) * 33 + c4 + c];
            }
            const float sg = MODE == 1 ? sg_compact[nrow * NP + o] : 1.0f / (1.0f + expf(-x));
            const float j = t * sg * (1.0f - sg);
            sumsq += (double)(j * j);
        }
    }
    sumsq += __shfl_xor(sumsq, 1, 64);
    sumsq += __shfl_xor(sumsq, 2, 64);
    sumsq += __shfl_xor(sumsq, 4, 64);
    if ((threadIdx.x & 7) == 0) norms[slot0 + row] = (float)sqrt(sumsq);
}

__global__ __launch_bounds__(256) void combine_kernel(const float *__restrict__ norms, int64_t e_base, int64_t e_count,
                                                     int batch, int slots_per_group, float *__restrict__ len_out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e_count; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t chunk = i / batch, within = i % batch;
        const float a = norms[(chunk * 2 + 0) * slots_per_group + within];
        const float b = norms[(chunk * 2 + 1) * slots_per_group + within];
        len_out[e_base + i] = 0.5f * (a + b);
    }
}

// ---------------------------------------------------------------------------------- per-latent Jacobians
// Decoders with FIXED statistics and a narrow latent (d <= 16): the decoder Jacobian J(z) (p_out x d) is a function of the
// latent alone, and an edge end's pulled-back length is |J(z_node) (z_dst - z_src)|.  With more than ~d/2 neighbours per latent
// it is cheaper to push the d unit tangents of every latent through the tangent-only pass ONCE (N d slots instead of 2 E) and
// to form the edge ends from the stored columns (SURVEY 2.1 K4': "one metric tensor per latent").  The columns, not the Gram
// matrix G = J^T J: dz^T G dz squares J's condition number into the rounding error, J dz does not, and at p_out = 16 both cost
// d^2 multiply-adds per edge end.
// Pseudo-edge i = (latent pair i / d, dimension i % d): start side latent 2 * pair, end side latent 2 * pair + 1 (an odd last
// latent is its own partner: both sides then write the same column with the same bits).
__global__ __launch_bounds__(256) void pair_edges_kernel(int64_t n_nodes, int d, int64_t n_pseudo, int32_t *__restrict__ src,
                                                        int32_t *__restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pseudo; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = 2 * (i / d), b = a + 1 < n_nodes ? a + 1 : n_nodes - 1;
        src[i] = (int32_t)a;
        dst[i] = (int32_t)b;
    }
}

// 16 lanes per edge (lane = output element, strided), both ends: v = J(node) dz as an fmaf chain over the latent dimensions
// (ascending), |v| accumulated in fp64 like back_mfma_kernel's norm, length = the mean of the two ends (combine_kernel).
__global__ __launch_bounds__(256) void jacobian_lengths_kernel(const float *__restrict__ z, const int32_t *__restrict__ src,
                                                              const int32_t *__restrict__ dst, int64_t n_edges, int d, int p_out,
                                                              int np, const float *__restrict__ jac_node,
                                                              float *__restrict__ len_out) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int l = (int)(gid & 15);
    int64_t e = gid >> 4;
    const bool live = e < n_edges;
    if (!live) e = n_edges - 1;                               // whole 16-lane teams are live or not; shuffles stay uniform
    const int64_t a = src[e], b = dst[e];
    float dz[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) dz[k] = k < d ? z[b * d + k] - z[a * d + k] : 0.f;
    float end_norm[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const float *J = jac_node + (size_t)(side ? b : a) * d * np;
        double sumsq = 0.0;
        for (int o = l; o < p_out; o += 16) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < d) v = fmaf(dz[k], J[(size_t)k * np + o], v);
            sumsq += (double)(v * v);
        }
        sumsq += __shfl_xor(sumsq, 1, 64);
        sumsq += __shfl_xor(sumsq, 2, 64);
        sumsq += __shfl_xor(sumsq, 4, 64);
        sumsq += __shfl_xor(sumsq, 8, 64);
        end_norm[side] = (float)sqrt(sumsq);
    }
    if (live && l == 0) len_out[e] = 0.5f * (end_norm[0] + end_norm[1]);
}

// ---------------------------------------------------------------------------------- per-latent metric tensor
// geo_decoder_metric_tensor: the same columns, reduced to G = J^T J per latent instead of to edge lengths.
// G[a][b] = sum over o < p_out of (double)J[a][o] * (double)J[b][o], o ascending.  The product of two float32 values is exact in
// fp64 (48 significant bits), so every partial sum is the correctly rounded fp64 sum of exact terms whether or not the compiler
// contracts the multiply-add.  One workgroup per latent at a time: the d columns staged in LDS (coalesced), one thread per
// entry of the upper triangle, which also writes the mirrored entry -- G[a][b] and G[b][a] are the same bits.  No atomics; the
// padding of a column (o >= p_out, up to np) is never read: back_mfma_kernel never wrote it.
constexpr int GRAM_MAX_D = 16, GRAM_MAX_P = 192, GRAM_LD = GRAM_MAX_P + 1;
__global__ __launch_bounds__(256) void jacobian_gram_kernel(const float *__restrict__ jac_node, int64_t n_nodes, int d, int p_out,
                                                           int np, double *__restrict__ G) {
    __shared__ float Js[GRAM_MAX_D][GRAM_LD];
    const int n_pairs = d * (d + 1) / 2;
    int a = 0, b = (int)threadIdx.x;                          // entry threadIdx.x of the upper triangle, rows in order
    while (a < d && b >= d - a) { b -= d - a; ++a; }
    b += a;
    for (int64_t node = blockIdx.x; node < n_nodes; node += gridDim.x) {
        __syncthreads();                                       // (the last latent's entries are read)
        const float *J = jac_node + (size_t)node * d * np;
        for (int i = threadIdx.x; i < d * p_out; i += 256) {
            const int k = i / p_out, o = i - k * p_out;
            Js[k][o] = J[(size_t)k * np + o];
        }
        __syncthreads();
        if ((int)threadIdx.x < n_pairs) {
            double s = 0.0;
            for (int o = 0; o < p_out; ++o) s += (double)Js[a][o] * (double)Js[b][o];
            double *Gn = G + (size_t)node * d * d;
            Gn[a * d + b] = s;
            Gn[b * d + a] = s;
        }
    }
}

// Spectrum of one G per thread, fp64: cyclic Jacobi on the upper triangle (kept in LDS, [entry][thread]: a thread's entries lie
// in its own bank pair, and nothing is shared, so the kernel has no barrier).  Fixed order: sweeps over (p, q), p < q, rows in
// order; a rotation is skipped when the off-diagonal entry is exactly 0 and, from the fifth sweep on, set to 0 when it no longer
// changes either diagonal entry in fp64; the sweeps end when every off-diagonal entry is exactly 0 (at most SPEC_SWEEPS).  All of
// it is a function of the matrix alone: the same G gives the same bits on every run.  Eigenvalues sorted ascending;
//   rank   = #{ i : eig_i > 0 and sqrt(eig_i) > max(p_out, d) * FLT_EPSILON * sqrt(eig_max) }  (numpy's matrix_rank rule on J's
//            singular values),
//   logvol = 0.5 * sum_i log(eig_i), ascending, if every eigenvalue is > 0, else -inf.
// G = 0 gives eig = 0, rank = 0, logvol = -inf; no NaN from a finite G.
constexpr int SPEC_THREADS = 64, SPEC_TRI = GRAM_MAX_D * (GRAM_MAX_D + 1) / 2, SPEC_SWEEPS = 32;
__device__ __forceinline__ int tri_at(int i, int j, int d) {      // entry (i, j) = (j, i) of the packed upper triangle
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo * d - lo * (lo - 1) / 2 + (hi - lo);
}
__global__ __launch_bounds__(SPEC_THREADS) void metric_spectrum_kernel(const double *__restrict__ G, int64_t n_nodes, int d,
                                                                      int p_out, double *__restrict__ eig_out,
                                                                      double *__restrict__ logvol_out,
                                                                      int32_t *__restrict__ rank_out) {
    __shared__ double A[SPEC_TRI][SPEC_THREADS];
    const int t = threadIdx.x;
    const int64_t node = (int64_t)blockIdx.x * SPEC_THREADS + t;
    if (node >= n_nodes) return;
    const double *Gn = G + (size_t)node * d * d;
    for (int i = 0; i < d; ++i)
        for (int j = i; j < d; ++j) A[tri_at(i, j, d)][t] = Gn[i * d + j];
    for (int sweep = 0; sweep < SPEC_SWEEPS; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < d - 1; ++p)
            for (int q = p + 1; q < d; ++q) off += fabs(A[tri_at(p, q, d)][t]);
        if (off == 0.0) break;
        for (int p = 0; p < d - 1; ++p)
            for (int q = p + 1; q < d; ++q) {
                const int ipq = tri_at(p, q, d), ipp = tri_at(p, p, d), iqq = tri_at(q, q, d);
                const double apq = A[ipq][t];
                if (apq == 0.0) continue;
                const double app = A[ipp][t], aqq = A[iqq][t], g = 100.0 * fabs(apq);
                if (sweep >= 4 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { A[ipq][t] = 0.0; continue; }
                const double h = aqq - app;
                double tn;                                      // tan of the rotation angle, the smaller root
                if (fabs(h) + g == fabs(h)) tn = apq / h;
                else {
                    const double theta = 0.5 * h / apq;
                    tn = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) tn = -tn;
                }
                const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c, tau = s / (1.0 + c);
                A[ipp][t] = app - tn * apq;
                A[iqq][t] = aqq + tn * apq;
                A[ipq][t] = 0.0;
                for (int k = 0; k < d; ++k) {
                    if (k == p || k == q) continue;
                    const int ikp = tri_at(k, p, d), ikq = tri_at(k, q, d);
                    const double akp = A[ikp][t], akq = A[ikq][t];
                    A[ikp][t] = akp - s * (akq + akp * tau);
                    A[ikq][t] = akq + s * (akp - akq * tau);
                }
            }
    }
    // the diagonal into entries 0 .. d-1 (row 0: of these only entry 0 is a diagonal entry, and it stays), insertion sort
    for (int i = 1; i < d; ++i) A[i][t] = A[tri_at(i, i, d)][t];
    for (int i = 1; i < d; ++i) {
        const double v = A[i][t];
        int j = i - 1;
        while (j >= 0 && A[j][t] > v) { A[j + 1][t] = A[j][t]; --j; }
        A[j + 1][t] = v;
    }
    const double emax = A[d - 1][t];
    const double tol = (double)(p_out > d ? p_out : d) * (double)FLT_EPSILON * (emax > 0.0 ? sqrt(emax) : 0.0);
    int rank = 0;
    bool positive = true;
    double logdet = 0.0;
    for (int i = 0; i < d; ++i) {
        const double e = A[i][t];
        if (eig_out) eig_out[(size_t)node * d + i] = e;
        if (e > 0.0) { logdet += log(e); if (sqrt(e) > tol) ++rank; }
        else positive = false;
    }
    if (rank_out) rank_out[node] = rank;
    if (logvol_out) logvol_out[node] = positive ? 0.5 * logdet : -(double)INFINITY;
}

// ---------------------------------------------------------------------------------- curve energy and relaxation
// geo_curve_energy / geo_curve_relax: a curve is F consecutive latents of a slice, so the per-node primal
// pass leaves its output sigmoids g[f] in sg_node and the column pass its Jacobians J[f] in jac, rows c * F + f.
// curve_reduce_kernel, one workgroup per curve at a time, g staged in LDS ([F][p_out + 1]: the odd row length keeps threads of
// different frames on different banks), every sum one fp64 accumulator over o ascending, nothing contracted:
//   seg_sq[f] = sum_o ((double)g[f+1][o] - (double)g[f][o])^2                                  one thread per segment
//   grad[f][k] = 2 * sum_o (double)J[f][k][o] * r[o],  r[o] = (g[f][o] - g[f-1][o]) - (g[f+1][o] - g[f][o]) in fp64; 0 at the ends
//   row[f][k]  = sum_o (double)J[f][k][o]^2 (exact products)                                   one thread per (f, k) for both
//   E = sum_f seg_sq[f], tr[f] = sum_k row[f][k], ascending, one thread each
// A curve with a NaN or an inf among its F * d coordinates has E = NaN, whatever the passes made of it (their ReLU is a maximum,
// which drops a NaN): every comparison with that E is false, so geo_curve_relax never moves such a curve.
// A thread reads its own column of J from global memory (768 contiguous bytes at most); the padding o >= p_out is never read.
__global__ __launch_bounds__(CURVE_THREADS) void curve_reduce_kernel(const float *__restrict__ sg_node, int sg_ld,
                                                                    const float *__restrict__ jac_node,
                                                                    const float *__restrict__ x, int64_t n_curves, int F,
                                                                    int d, int p_out, int np, double *__restrict__ energy,
                                                                    double *__restrict__ seg_sq, double *__restrict__ grad,
                                                                    double *__restrict__ tr) {
#pragma clang fp contract(off)      // plain operators below: the pragma governs them
    extern __shared__ float curve_g[];
    __shared__ double seg_s[CURVE_MAX_F];
    __shared__ double row_s[CURVE_MAX_F * GRAM_MAX_D];
    __shared__ int not_finite;
    const int ld = p_out + 1;
    for (int64_t c = blockIdx.x; c < n_curves; c += gridDim.x) {
        __syncthreads();                                       // (the last curve's sums are read)
        if (threadIdx.x == 0) not_finite = 0;
        const float *g = sg_node + (size_t)c * F * sg_ld;
        for (int i = threadIdx.x; i < F * p_out; i += CURVE_THREADS) {
            const int f = i / p_out, o = i - f * p_out;
            curve_g[f * ld + o] = g[(size_t)f * sg_ld + o];
        }
        __syncthreads();
        for (int f = threadIdx.x; f < F - 1; f += CURVE_THREADS) {
            const float *g0 = curve_g + f * ld, *g1 = g0 + ld;
            double s = 0.0;
            for (int o = 0; o < p_out; ++o) {
                const double dg = (double)g1[o] - (double)g0[o];
                s += dg * dg;
            }
            seg_s[f] = s;
            if (seg_sq) seg_sq[(size_t)c * (F - 1) + f] = s;
        }
        for (int i = threadIdx.x; i < F * d; i += CURVE_THREADS) {
            const int f = i / d, k = i - f * d;
            const float *J = jac_node + (((size_t)c * F + f) * d + k) * np;
            const bool interior = f > 0 && f < F - 1;
            const float *gm = curve_g + (interior ? f - 1 : f) * ld, *g0 = curve_g + f * ld,
                        *gp = curve_g + (interior ? f + 1 : f) * ld;
            double s = 0.0, sq = 0.0;
            for (int o = 0; o < p_out; ++o) {
                const double j = (double)J[o];
                const double r = ((double)g0[o] - (double)gm[o]) - ((double)gp[o] - (double)g0[o]);
                s += j * r;
                sq += j * j;
            }
            row_s[i] = sq;
            if ((__float_as_uint(x[(size_t)c * F * d + i]) & 0x7f800000u) == 0x7f800000u) not_finite = 1;      // (all writers: 1)
            if (grad) grad[(size_t)c * F * d + i] = interior ? 2.0 * s : 0.0;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double e = 0.0;
            for (int f = 0; f < F - 1; ++f) e += seg_s[f];
            energy[c] = not_finite ? (double)NAN : e;
        }
        if (tr)
            for (int f = threadIdx.x; f < F; f += CURVE_THREADS) {
                double t = 0.0;
                for (int k = 0; k < d; ++k) t += row_s[f * d + k];
                tr[(size_t)c * F + f] = t;
            }
    }
}

// g_out [n][p_out] and jac_out [n][d][p_out] of a slice, without the padding of sg_node's and jac's rows (either may be null)
__global__ __launch_bounds__(256) void curve_export_kernel(const float *__restrict__ sg_node, int sg_ld,
                                                          const float *__restrict__ jac_node, int64_t n_nodes, int d, int p_out,
                                                          int np, float *__restrict__ g_out, float *__restrict__ jac_out) {
    const int64_t rows = n_nodes * d, stride = (int64_t)gridDim.x * 256;
    if (g_out)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_nodes * p_out; i += stride)
            g_out[i] = sg_node[(size_t)(i / p_out) * sg_ld + i % p_out];
    if (jac_out)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows * p_out; i += stride)
            jac_out[i] = jac_node[(size_t)(i / p_out) * np + i % p_out];
}

// ---------------------------------------------------------------------------------- host side: shape, plan, route
bool make_shape(const geo_decoder_desc *dc, Shape *s) {
    s->d = dc->latent_dim; s->c0 = dc->c0; s->c1 = dc->c1; s->c2 = dc->c2; s->co = dc->out_channels;
    if (dc->out_size == 28) { s->s_out = 4; s->pad3 = 3; }
    else if (dc->out_size == 32) { s->s_out = 8; s->pad3 = 1; }
    else return false;
    s->p_out = s->co * s->s_out * s->s_out;
    s->n1 = 4 * s->c1; s->n2 = 16 * s->c2;
    if (s->c2 <= 0 || NC % s->c2 != 0) return false;
    if (s->c1 <= 0 || 4 * s->c1 > FRONT_MAX_N1) return false;
    s->opix_per_chunk = NC / s->c2;
    if (s->opix_per_chunk > 16) s->opix_per_chunk = 16;
    s->n_chunks = 16 / s->opix_per_chunk;
    return true;
}

// Output pixels ordered so that neighbours in the list are fed by the same input pixels.
void make_chunks(const Shape &s, ChunkTable *t) {
    static const int order[16][2] = {{0, 1}, {0, 2}, {3, 1}, {3, 2}, {1, 0}, {2, 0}, {1, 3}, {2, 3},
                                     {1, 1}, {1, 2}, {2, 1}, {2, 2}, {0, 0}, {0, 3}, {3, 0}, {3, 3}};
    for (int ch = 0; ch < 16; ++ch) { t->nblk[ch] = 0; for (int i = 0; i < 16; ++i) t->opix[ch][i] = 0; }
    for (int ch = 0; ch < s.n_chunks; ++ch) {
        bool used[4] = {false, false, false, false};
        for (int lo = 0; lo < s.opix_per_chunk; ++lo) {
            const int oy = order[ch * s.opix_per_chunk + lo][0], ox = order[ch * s.opix_per_chunk + lo][1];
            t->opix[ch][lo] = oy * 4 + ox;
            for (int iy = 0; iy < 2; ++iy)
                for (int ix = 0; ix < 2; ++ix) {
                    const int ky = oy + 1 - 2 * iy, kx = ox + 1 - 2 * ix;
                    if (ky >= 0 && ky < 4 && kx >= 0 && kx < 4) used[iy * 2 + ix] = true;
                }
        }
        for (int ip = 0; ip < 4; ++ip)
            if (used[ip]) t->ipix[ch][t->nblk[ch]++] = ip;
    }
}

// mid_all_kernel / mid_pipe_kernel / mid_start_kernel have the chunk table compiled in (MidGeom): it must be this table
bool chunks_match_mid_geom(const ChunkTable &tab, int *bad_chunk) {
    for (int ch = 0; ch < 8; ++ch) {
        int nb = 0;
        bool ok = true;
        for (int ip = 0; ip < 4; ++ip) {
            const int blk = MidGeom::blk_of(ch, ip);
            if (blk >= 0) { ok = ok && tab.ipix[ch][blk] == ip; ++nb; }
        }
        ok = ok && nb == tab.nblk[ch] && tab.opix[ch][0] == MidGeom::opix(ch, 0) && tab.opix[ch][1] == MidGeom::opix(ch, 1);
        if (!ok) { *bad_chunk = ch; return false; }
    }
    return true;
}

// ---- the workspace.  Three groups of buffers, each described once by a layout function over a geo::Arena: the sizes make_route
// compares are measurements of these functions, and run_jvp carves the caller's memory with the same three.
struct Buffers {
    float *M01, *b01, *B2p, *W3p, *pre1, *tpre1, *pre2, *tpre2, *norms;
    unsigned short *B3, *W3b;
    double *part1, *part2; NormConst *k1, *k2;                // partial sums and norm constants of layers 1, 2
    float2 *stats;                                              // batch statistics on their way into the running ones
    int32_t *slot_valid;
    float4 *gs1, *gs2;                                          // GroupNorm
    float *pre2_node, *sg_node;                                 // per_node
    int32_t *row_map, *rep, *n_compact;                         // dedup
    float *sg_compact;                                          // dedup
    int32_t *psrc, *pdst; float *jac;                           // node_jacobian: pseudo-edge lists, columns
    ChunkTable tab;
};

struct Tiling { size_t slots, tiles, groups; };                 // of one pass: padded sample positions, tiles of TS, chunk sides

constexpr int64_t MAX_SLOTS_PER_PASS = 1 << 20;      // bounds the activation workspace (~12.5 GB; the C2 graph takes two passes)
constexpr size_t JVP_PASS_RESERVE = 4096;            // what Plan::bytes holds beyond the measured layout of a pass

size_t round_up_to_tile(int64_t n) { return n > 0 ? ((size_t)n + TS - 1) / TS * TS : 0; }
size_t part1_count(const Shape &s, const Tiling &t) { return t.tiles * s.n1 * 4; }      // layer 1's partial sums, [tile][n1][4]

// the buffers of a pass of chunks: packed weights, activations, partial sums, norm constants and statistics
void lay_out_pass(geo::Arena &ar, Buffers *b, const Shape &s, const Tiling &t, bool group_norm) {
    ar.take(b->M01, (size_t)s.d * s.n1); ar.take(b->b01, (size_t)s.n1);
    ar.take(b->B2p, (size_t)s.n_chunks * MAX_BLOCKS * s.c1 * NC);
    ar.take(b->B3, (size_t)s.n_chunks * MAX_BLOCKS * s.c1 * NC * 3);                       // bf16 x 3
    ar.take(b->W3p, (size_t)16 * s.co * s.c2);
    ar.take(b->W3b, (size_t)16 * s.c2 * 192 * 3);                                          // bf16 x 3
    ar.take(b->pre1, t.slots * s.n1); ar.take(b->tpre1, t.slots * s.n1);
    ar.take(b->pre2, t.slots * s.n2); ar.take(b->tpre2, t.slots * s.n2);
    ar.take(b->part1, part1_count(s, t)); ar.take(b->part2, t.tiles * s.n2 * 4);
    ar.take(b->k1, (t.groups + 1) * s.c1); ar.take(b->k2, (t.groups + 1) * s.c2);
    ar.take(b->norms, t.slots);
    ar.take(b->stats, (t.groups + 1) * (size_t)(s.c1 > s.c2 ? s.c1 : s.c2));
    ar.take(b->slot_valid, t.slots);
    if (group_norm) { ar.take(b->gs1, t.slots * 32); ar.take(b->gs2, t.slots * 32); }
}

// the per-node primal buffers: pre2 of every latent and the sigmoid of every output
void lay_out_nodes(geo::Arena &ar, Buffers *b, const Shape &s, int64_t n_nodes) {
    const size_t node_slots = round_up_to_tile(n_nodes);
    ar.take(b->pre2_node, node_slots * s.n2);
    ar.take(b->sg_node, node_slots * (size_t)((s.p_out + 31) / 32) * 32);
}

// node_jacobian: the pseudo-edge lists and the Jacobian's columns, jac_np padded outputs each
void lay_out_jacobian(geo::Arena &ar, Buffers *b, const Shape &s, int64_t n_nodes, int64_t n_pseudo, size_t jac_np) {
    ar.take(b->psrc, (size_t)n_pseudo); ar.take(b->pdst, (size_t)n_pseudo);
    ar.take(b->jac, (size_t)n_nodes * s.d * jac_np);
}

// What the dedup route keeps inside buffers of the pass that are dead by then.  The run maps (row_map and rep per slot, n_compact
// per group) live in part1, dead after finalize_batch_kernel; on the front_once route start_runs_kernel runs before the front, so
// there they sit behind the front's partial sums, [tile][c1][4] at the head of part1.  The compact rows' output sigmoids live in
// pre1, dead after ConvT2.  make_route asks whether these fit, run_jvp takes the pointers.
struct StartRuns {
    size_t slots, n1, part1_bytes, front_bytes, maps_bytes;
    StartRuns(const Shape &s, const Tiling &t)
        : slots(t.slots), n1((size_t)s.n1), part1_bytes(part1_count(s, t) * sizeof(double)), front_bytes(t.tiles * s.c1 * 4 * sizeof(double)),
          maps_bytes((2 * t.slots + t.groups) * sizeof(int32_t)) {}
    size_t maps_at(bool front_once) const { return front_once ? front_bytes : 0; }
    bool maps_fit(bool front_once) const { return maps_at(front_once) + maps_bytes <= part1_bytes; }
    bool sigmoids_fit(size_t padded_outputs) const { return padded_outputs <= n1; }      // a row of pre1 holds a row's sigmoids
    void place(Buffers *b, bool front_once) const {
        b->row_map = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(b->part1) + maps_at(front_once));
        b->rep = b->row_map + slots; b->n_compact = b->rep + slots;
        b->sg_compact = b->pre1;
    }
};

struct Plan {
    Shape sh;
    int batch, tiles_per_group, slots_per_group;
    int64_t chunks_per_pass;
    size_t bytes;                                               // lay_out_pass measured, plus JVP_PASS_RESERVE
    size_t pass_slots() const { return (size_t)chunks_per_pass * 2 * slots_per_group; }
    Tiling tiling() const { return {pass_slots(), pass_slots() / TS, (size_t)chunks_per_pass * 2}; }
};

size_t node_bytes(const Shape &s, int64_t n_nodes) { Buffers b; return geo::measure(lay_out_nodes, &b, s, n_nodes); }

bool make_plan(const geo_decoder_desc *dc, int64_t n_edges, int batch, Plan *p) {
    if (!make_shape(dc, &p->sh)) return false;
    p->batch = batch;
    p->tiles_per_group = (batch + TS - 1) / TS;
    p->slots_per_group = p->tiles_per_group * TS;
    const int64_t chunks = (n_edges + batch - 1) / batch;
    int64_t cpp = MAX_SLOTS_PER_PASS / (2 * (int64_t)p->slots_per_group);
    if (cpp < 1) cpp = 1;
    if (cpp > chunks) cpp = chunks > 0 ? chunks : 1;
    p->chunks_per_pass = cpp;
    Buffers b;
    p->bytes = geo::measure(lay_out_pass, &b, p->sh, p->tiling(), dc->norm == 2) + JVP_PASS_RESERVE;
    return true;
}

// Every decision of a call, made once by make_route (host arithmetic: no GPU call, no global): which kernels run, over what
// tiling, in how much workspace.  The sizing queries, the run and geo_jvp_plan all read it from here.
//   per_node       Fixed statistics (no norm layer, BatchNorm in eval mode, GroupNorm's primal) over graph edges: the primal is a
//                  function of the latent, not of the edge -- 60 000 rows instead of 1.89 M edge ends.  One launch sequence over
//                  the latents keeps pre2 and the output sigmoids per node; the edge slots carry the tangent alone and take the
//                  ReLU masks and sigmoid' from their node's rows.  Same products in the same order: bit-identical to per slot.
//                  (GroupNorm: the primal's statistics per latent, the tangent's own per slot.)
//   node_jacobian  per_node and d <= 16: the passes run over pseudo-edges (latent pair, latent dimension) with unit tangents and
//                  leave the Jacobian's columns per latent; each edge end is then |J(z_node) dz| from those columns.
//   dedup          Train-mode BatchNorm over graph edges: the start side's primal rows once per run of equal src.  The maps live
//                  in part1 (dead after finalize_batch_kernel), the compact rows' output sigmoids in pre1 (dead after ConvT2).
//   front_once     dedup with the VALU front (jvp_front_once): front_edge_kernel, the first layer once per edge.  start_runs_kernel
//                  then runs before the front, so the maps sit behind the quarter of part1 the front's partial sums take.
enum { BACK_NODE_PRIMAL = 15 };      // launch_back only: ConvT3 of the per-node primal pass (never a route's `back`)

struct Route {
    int status = GEO_OK;             // what the run answers for this decoder / workspace; `error` is geo_last_error's text
    char error[192] = "";
    Plan pl = {};                    // shape and tiling of the passes (node_jacobian: over the pseudo-edges)
    int64_t run_edges = 0, passes = 0;                          // edges the passes cover (node_jacobian: pseudo-edges)
    bool batch_stats = false, track = false, group_norm = false;
    int front = GEO_JVP_FRONT_VALU, dmax = 16;                  // GEO_JVP_FRONT_*, compiled latent width of the front kernel
    int mid = GEO_JVP_MID_CHUNK, back = GEO_JVP_BACK_VALU;      // GEO_JVP_MID_*, GEO_JVP_BACK_*
    int back_nt = 0;                                            // 32-column output tiles of the matrix-core ConvT3 (1 or 6)
    int parts2 = 16;                 // partial-sum rows per tile that the ConvT2 kernel leaves for finalize_batch_kernel
    bool per_node = false, node_jacobian = false, dedup = false, front_once = false;
    bool head_stream = false;        // ConvT3 of the 16-output head without GroupNorm: head_stream_kernel (geo_jvp_head_stream)
    size_t back_lds = 0;             // dynamic LDS of back_kernel
    size_t jac_np = 0, jac_extra_bytes = 0;                     // node_jacobian: padded outputs per column; pseudo-edge lists + columns
    size_t bytes = 0;                // workspace as the matching *_workspace_bytes query sizes it (0: no answer)
};

bool route_error(Route *r, int status, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r->error, sizeof(r->error), fmt, ap);
    va_end(ap);
    r->status = status;
    return false;
}

// ws_bytes = nullptr: the workspace is what the matching query returns.  The sizes are filled in whenever the shape parses, also for a
// decoder the run refuses (status != GEO_OK): the queries answer for those as they always have.
// build_edges: the edges of the whole build this call computes a part of (>= n_edges; the plain entry points pass n_edges).  It
// enters in one place, the edges-per-latent rule of node_jacobian, so that every part of a build takes the route the whole takes;
// passes, slots and workspace are the call's own.
bool make_route(const geo_decoder_desc *dc, const geo::Options &o, bool graph_edges, int64_t n_nodes, int64_t n_edges,
                int64_t build_edges, int batch, const size_t *ws_bytes, Route *r) {
    *r = Route{};
    if (!dc) return route_error(r, GEO_E_ARG, "geo_decoder_jvp: null pointer");
    if (batch <= 0) return route_error(r, GEO_E_ARG, "geo_decoder_jvp: batch_size must be positive");
    if (build_edges < n_edges)
        return route_error(r, GEO_E_ARG, "geo_decoder_jvp: build_edges %lld < n_edges %lld", (long long)build_edges,
                           (long long)n_edges);
    Plan base;
    if (n_edges < 0 || n_nodes < 0 || !make_plan(dc, n_edges, batch, &base))
        return route_error(r, GEO_E_ARG, "geo_decoder_jvp: unsupported decoder (out_size %d, c2=%d must divide %d)", dc->out_size,
                           dc->c2, NC);
    const Shape &s = base.sh;

    // ---- kernels by decoder shape and options
    r->batch_stats = dc->norm == 1 && dc->bn_train;
    // train-mode BatchNorm with tracked statistics: the batches are folded into running_mean / running_var in call order
    r->track = r->batch_stats && dc->update_running && dc->rm1 && dc->rv1 && dc->rm2 && dc->rv2;
    r->group_norm = dc->norm == 2;
    r->dmax = s.d <= 16 ? 16 : (s.d <= 32 ? 32 : 64);
    r->front = s.d > 16 && s.n1 % 32 == 0 && o.jvp_front_valu == 0 ? GEO_JVP_FRONT_MFMA : GEO_JVP_FRONT_VALU;
    r->back_nt = (s.p_out + 31) / 32;
    // the one-tile-per-workgroup / persistent ConvT2 kernels: 8 chunks of 2 output pixels (c2 = 64); jvp_mid = 2 keeps the per-chunk one
    const bool mid_all = s.c1 % 16 == 0 && s.c1 >= 32 && s.n_chunks == 8 && s.opix_per_chunk == 2 && o.jvp_mid != 2;
    // the shipped widths with BatchNorm / no norm: the persistent skewed kernel (jvp_mid = 3: mid_all_kernel)
    const bool mid_pipe = mid_all && !r->group_norm && s.c1 == 128 && s.c2 == 64 && o.jvp_mid != 3;
    const bool back_mfma = s.c1 % 16 == 0 && s.c2 == 64 && (r->back_nt == 1 || r->back_nt == 6) && !o.jvp_back_valu;
    const bool per_node_kernels = graph_edges && !r->batch_stats && mid_all && back_mfma && o.jvp_per_node != 0;

    // ---- workspace of the call, and what a given workspace leaves room for
    const size_t node_slots = round_up_to_tile(n_nodes);
    const size_t per_edge_end_bytes = base.bytes + (graph_edges ? node_bytes(s, n_nodes) : 0);
    // per-latent Jacobians: worth it from ~1.5 x fewer slots (the columns pass stores and the edge pass re-reads p_out x d floats
    // per latent); option 2 takes the route whenever it applies
    Plan jpl;
    const int64_t n_pseudo = (n_nodes + 1) / 2 * s.d;
    size_t jac_bytes = 0;
    if (per_node_kernels && n_nodes > 0 && n_edges > 0 && s.d <= 16 && o.jvp_node_jacobian != 0 &&
        (o.jvp_node_jacobian != 1 || 4 * build_edges >= 3 * n_nodes * s.d) && n_pseudo < (int64_t)1 << 31 &&
        make_plan(dc, n_pseudo, batch, &jpl) && node_slots <= jpl.pass_slots()) {
        r->jac_np = (size_t)r->back_nt * 32;
        Buffers b;
        r->jac_extra_bytes = geo::measure(lay_out_jacobian, &b, s, n_nodes, n_pseudo, r->jac_np);
        jac_bytes = r->jac_extra_bytes + jpl.bytes + node_bytes(s, n_nodes);
    }
    r->bytes = jac_bytes > per_edge_end_bytes ? jac_bytes : per_edge_end_bytes;
    const size_t ws = ws_bytes ? *ws_bytes : r->bytes;
    r->node_jacobian = jac_bytes && ws >= jac_bytes;
    r->pl = r->node_jacobian ? jpl : base;
    r->run_edges = r->node_jacobian ? n_pseudo : n_edges;
    const int64_t chunks = (r->run_edges + batch - 1) / batch;
    r->passes = (chunks + r->pl.chunks_per_pass - 1) / r->pl.chunks_per_pass;
    // a workspace of geo_jvp_workspace_bytes() only, or more latents than a pass has slots: the per-edge-end path
    const size_t run_ws = ws - (r->node_jacobian ? r->jac_extra_bytes : 0);
    r->per_node = per_node_kernels && node_slots && node_slots <= r->pl.pass_slots() &&
                  run_ws >= r->pl.bytes + node_bytes(s, n_nodes);
    const StartRuns runs(s, r->pl.tiling());
    r->dedup = r->batch_stats && graph_edges && mid_pipe && back_mfma && o.jvp_start_dedup != 0 && runs.maps_fit(false) &&
               runs.sigmoids_fit((size_t)r->back_nt * 32);
    // (dedup implies c1 = 128, the width front_edge_kernel is compiled for, and the maps fit behind the front's partial sums:
    // 4 KB of the 16 KB a tile has in part1, the maps take 260 B; mid_start_kernel addresses a group's rows through one buffer
    // descriptor with 32-bit offsets: all spelled out)
    r->front_once = r->dedup && r->front == GEO_JVP_FRONT_VALU && o.jvp_front_once != 0 && s.n1 == FRONT_EDGE_N1 &&
                    runs.maps_fit(true) && (size_t)base.slots_per_group * s.n1 * 4 < ((size_t)1 << 31);

    r->mid = r->per_node ? GEO_JVP_MID_ALL_TANGENT
           : mid_pipe    ? (r->dedup ? GEO_JVP_MID_PIPE_DEDUP : GEO_JVP_MID_PIPE)
           : mid_all     ? GEO_JVP_MID_ALL
                         : GEO_JVP_MID_CHUNK;
    r->parts2 = mid_pipe && !r->per_node ? 4 : (mid_all ? 1 : 16);
    r->back = r->dedup ? GEO_JVP_BACK_DEDUP : r->per_node ? GEO_JVP_BACK_PER_NODE : back_mfma ? GEO_JVP_BACK_MFMA : GEO_JVP_BACK_VALU;
    // the streaming 16-output head: per slot (mfma), and on the dedup route the end side and the start-side tangents
    r->head_stream = back_mfma && r->back_nt == 1 && !r->group_norm && (r->back == GEO_JVP_BACK_DEDUP || r->back == GEO_JVP_BACK_MFMA) &&
                     o.jvp_head_stream != 0 &&
                     (!r->dedup || (size_t)base.slots_per_group * s.n2 * 4 < ((size_t)1 << 31));   // (one descriptor per group's rows)
    r->back_lds = ((size_t)2 * BACK_TS * 16 * (s.c2 + 4) + (size_t)16 * s.co * (s.c2 + 4) + (size_t)BACK_TS * s.p_out) * 4;

    // ---- what the run refuses
    if (!(s.d >= 1 && s.d <= 64)) return route_error(r, GEO_E_ARG, "geo_decoder_jvp: latent_dim %d not in [1,64]", s.d);
    if (!(s.c1 == 128 || s.c1 == 64 || s.c1 == 32))
        return route_error(r, GEO_E_ARG, "geo_decoder_jvp: dec_channels[1]=%d not in {32,64,128}", s.c1);
    if (!(dc->norm >= 0 && dc->norm <= 2)) return route_error(r, GEO_E_ARG, "geo_decoder_jvp: unknown norm code %d", dc->norm);
    if (s.c2 % 16 != 0) return route_error(r, GEO_E_ARG, "geo_decoder_jvp: dec_channels[2]=%d must be a multiple of 16", s.c2);
    if (r->back_lds > 160 * 1024)
        return route_error(r, GEO_E_ARG, "geo_decoder_jvp: decoder too wide for the back kernel (%zu B LDS)", r->back_lds);
    if (run_ws < r->pl.bytes) return route_error(r, GEO_E_WORKSPACE, "geo_decoder_jvp: workspace %zu < %zu", run_ws, r->pl.bytes);
    // the GroupNorm path exists for the 32-group layouts of the matrix-core kernels (reference default decoder)
    if (r->group_norm && !(dc->groups1 == 32 && dc->groups2 == 32 && s.c2 == 64 && back_mfma && mid_all))
        return route_error(r, GEO_E_ARG,
                           "geo_decoder_jvp: GroupNorm needs 32 groups per layer and dec_channels[2] == 64 (got %d/%d groups, c2=%d)",
                           dc->groups1, dc->groups2, s.c2);
    return true;
}

int encode_route(const Route &r) {
    const int64_t passes = r.passes < 0x7fff ? r.passes : 0x7fff;
    return r.front | (r.dmax == 16 ? 0 : (r.dmax == 32 ? 1 : 2)) << 2 | r.mid << 4 | r.back << 8 |
           (r.per_node ? GEO_JVP_PER_NODE : 0) | (r.node_jacobian ? GEO_JVP_NODE_JACOBIAN : 0) | (r.dedup ? GEO_JVP_DEDUP : 0) |
           (r.front_once ? GEO_JVP_FRONT_ONCE : 0) | (int)passes << 16;
}

// ---------------------------------------------------------------------------------- host side: launchers
// One launch sequence front -> ConvT2 -> ConvT3: a pass of chunks over the edges, or the per-node primal pass over the latents
// (one group: every latent on the "start" side).
struct Pass {
    int mid, back;                                              // GEO_JVP_MID_*, GEO_JVP_BACK_* | BACK_NODE_PRIMAL
    int64_t tiles, e_base, n_edges;
    int tiles_per_group, batch, unit_d, stat;                   // stat 1: batch statistics (constants per group, partial sums)
    const float *z, *z_start, *z_end;                           // latents + edge list, or explicit end points
    const int32_t *src, *dst;
    float *mid_pre2;                                            // where ConvT2's primal rows go
    const float *back_pre2;                                     // the primal rows ConvT3 (and GroupNorm 2) reads
    int64_t slots() const { return tiles * TS; }
    int64_t groups() const { return tiles / tiles_per_group; }
};

// template arguments from run-time values: f(std::integral_constant) of the matching one
template <int... Vs, class F>
void pick_int(int v, F &&f) { ((v == Vs ? (void)f(std::integral_constant<int, Vs>{}) : (void)0), ...); }
template <class F>
void pick_bool(bool v, F &&f) { if (v) f(std::true_type{}); else f(std::false_type{}); }

int cu_count(int *n) {
    static int n_cu = 0;
    if (n_cu == 0) {
        int devid = 0, cus = 0;
        GEO_HIP_CHECK(hipGetDevice(&devid));
        GEO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devid));
        n_cu = cus > 0 ? cus : 256;
    }
    *n = n_cu;
    return GEO_OK;
}

// the start side's run maps of a dedup pass (row_map, rep, n_compact)
int launch_start_runs(const Pass &p, const Buffers &b, hipStream_t stream) {
    start_runs_kernel<<<(unsigned)(p.groups() / 2), 256, 0, stream>>>(p.src, p.e_base, p.n_edges, p.batch, p.tiles_per_group * TS,
                                                                     b.row_map, b.rep, b.n_compact);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

int launch_front(const Route &r, const Pass &p, const Buffers &b, hipStream_t stream) {
    const Shape &s = r.pl.sh;
    if (r.front_once)                                           // one workgroup per tile of edges: both sides of the pass
        pick_int<16, 32, 64>(r.dmax, [&](auto dm) {
            front_edge_kernel<decltype(dm)::value><<<(unsigned)(p.tiles / 2), 256, 0, stream>>>(
                p.z, p.src, p.dst, p.e_base, p.n_edges, p.batch, p.tiles_per_group, s.d, b.M01, b.b01, b.pre1, b.tpre1, b.part1);
        });
    else if (r.front == GEO_JVP_FRONT_MFMA)
        pick_int<32, 64>(r.dmax, [&](auto dm) {
            front_mfma_kernel<decltype(dm)::value><<<(unsigned)p.tiles, 256, 0, stream>>>(
                p.z, p.src, p.dst, p.z_start, p.z_end, p.e_base, p.n_edges, p.batch, p.tiles_per_group, s.d, s.n1, b.M01, b.b01,
                b.pre1, b.tpre1, b.part1, p.stat);
        });
    else
        pick_int<16, 32, 64>(r.dmax, [&](auto dm) {
            front_kernel<decltype(dm)::value><<<(unsigned)p.tiles, 256, 0, stream>>>(
                p.z, p.src, p.dst, p.z_start, p.z_end, p.e_base, p.n_edges, p.batch, p.tiles_per_group, s.d, s.n1, b.M01, b.b01,
                b.pre1, b.tpre1, b.part1, p.stat, p.unit_d);
        });
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// Norm constants of layer 1 (after the front) or 2 (after ConvT2): batch statistics from the partial sums, folded into the
// running statistics where tracked; GroupNorm's per-sample statistics.  Fixed statistics were set once per call.
int launch_stats(const Route &r, const geo_decoder_desc *dc, int layer, const Pass &p, const Buffers &b, hipStream_t stream) {
    const Shape &s = r.pl.sh;
    const bool l1 = layer == 1;
    const int C = l1 ? s.c1 : s.c2, npx = l1 ? 4 : 16;
    if (p.stat) {
        finalize_batch_kernel<<<geo::grid_for(p.groups() * C, 256), 256, 0, stream>>>(
            l1 ? b.part1 : b.part2, p.tiles_per_group, l1 ? 1 : r.parts2, npx, C, p.e_base, p.n_edges, p.batch, l1 ? dc->g1 : dc->g2,
            l1 ? dc->be1 : dc->be2, dc->eps, l1 ? b.k1 : b.k2, (int)p.groups(), r.track ? b.stats : nullptr);
        if (r.track)
            running_update_kernel<<<(unsigned)((C + 7) / 8), 256, 0, stream>>>(
                b.stats, (int)p.groups(), C, dc->momentum, const_cast<float *>(l1 ? dc->rm1 : dc->rm2),
                const_cast<float *>(l1 ? dc->rv1 : dc->rv2));
        GEO_LAUNCH_CHECK();
    }
    if (r.group_norm) {
        const int32_t *prim_row = nullptr;
        if (!l1 && p.back == GEO_JVP_BACK_PER_NODE) {      // (slot_valid is not read on this path: it carries the slot -> latent map)
            slot_node_kernel<<<geo::grid_for(p.slots(), 256), 256, 0, stream>>>(p.src, p.dst, p.e_base, p.n_edges, p.batch,
                                                                                p.tiles_per_group, p.slots(), b.slot_valid);
            prim_row = b.slot_valid;
        }
        group_stats_kernel<<<geo::grid_for(p.slots() * 32, 256), 256, 0, stream>>>(
            l1 ? b.pre1 : p.back_pre2, l1 ? b.tpre1 : b.tpre2, p.slots(), npx, C, 32, dc->eps, l1 ? b.gs1 : b.gs2, prim_row);
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}

int launch_mid(const Route &r, const geo_decoder_desc *dc, const Pass &p, const Buffers &b, hipStream_t stream) {
    const Shape &s = r.pl.sh;
    if (p.mid == GEO_JVP_MID_PIPE || p.mid == GEO_JVP_MID_PIPE_DEDUP) {
        const bool dedup = p.mid == GEO_JVP_MID_PIPE_DEDUP;
        const int64_t chunks = p.groups() / 2;
        if (dedup && !r.front_once)                             // (front_once: before the front, launch_pass)
            if (const int rc = launch_start_runs(p, b, stream)) return rc;
        int n_cu = 0;
        if (const int rc = cu_count(&n_cu)) return rc;
        const int64_t pipe_tiles = dedup ? p.tiles / 2 : p.tiles;                        // (dedup: the end side only)
        const unsigned grid = (unsigned)std::min<int64_t>(pipe_tiles, n_cu);             // persistent workgroups, one resident per CU
        pick_bool(dedup, [&](auto end_only) {
            mid_pipe_kernel<decltype(end_only)::value><<<grid, 512, 0, stream>>>(
                b.pre1, b.tpre1, b.k1, p.stat, p.tiles_per_group, (int)pipe_tiles, s.c2, b.B3, dc->b2, p.mid_pre2, b.tpre2, b.part2,
                p.stat, p.e_base, p.n_edges, p.batch);
        });
        GEO_LAUNCH_CHECK();
        if (dedup) {                                            // compact primal rows first: the tangent launch gathers them
            mid_start_kernel<false><<<dim3(1, (unsigned)chunks), 512, 0, stream>>>(
                b.pre1, b.tpre1, b.k1, p.tiles_per_group, b.B3, dc->b2, p.mid_pre2, b.tpre2, b.part2, b.row_map, b.rep, b.n_compact,
                p.e_base, p.n_edges, p.batch);
            GEO_LAUNCH_CHECK();
            pick_bool(r.front_once, [&](auto once) {
                mid_start_kernel<true, decltype(once)::value>
                    <<<dim3((unsigned)((p.tiles_per_group + 1) / 2), (unsigned)chunks), 512, 0, stream>>>(
                        b.pre1, b.tpre1, b.k1, p.tiles_per_group, b.B3, dc->b2, p.mid_pre2, b.tpre2, b.part2, b.row_map, b.rep,
                        b.n_compact, p.e_base, p.n_edges, p.batch);
            });
            GEO_LAUNCH_CHECK();
        }
    } else if (p.mid == GEO_JVP_MID_ALL || p.mid == GEO_JVP_MID_ALL_TANGENT) {
        pick_int<128, 64, 32>(s.c1, [&](auto c1) {
            pick_bool(r.group_norm, [&](auto gn) {
                pick_bool(p.mid == GEO_JVP_MID_ALL_TANGENT, [&](auto tangent_only) {
                    mid_all_kernel<decltype(c1)::value, decltype(gn)::value, decltype(tangent_only)::value>
                        <<<(unsigned)p.tiles, 512, 0, stream>>>(b.pre1, b.tpre1, b.k1, p.stat, p.tiles_per_group, s.c2, b.B3, dc->b2,
                                                                p.mid_pre2, b.tpre2, b.part2, p.stat, b.slot_valid, b.gs1, p.e_base,
                                                                p.n_edges, p.batch);
                });
            });
        });
        GEO_LAUNCH_CHECK();
    } else {                                                    // other widths: one workgroup per (tile, chunk of output pixels)
        pick_int<128, 64, 32>(s.c1, [&](auto c1) {
            mid_bf16_kernel<decltype(c1)::value><<<dim3((unsigned)p.tiles, (unsigned)s.n_chunks), 256, 0, stream>>>(
                b.pre1, b.tpre1, b.k1, p.stat, p.tiles_per_group, b.tab, s.opix_per_chunk, s.c2, b.B3, dc->b2, p.mid_pre2, b.tpre2,
                b.part2, p.stat, b.slot_valid);
        });
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}

int launch_back(const Route &r, const geo_decoder_desc *dc, const Pass &p, const Buffers &b, hipStream_t stream) {
    const Shape &s = r.pl.sh;
    if (p.back == GEO_JVP_BACK_VALU) {
        back_kernel<<<(unsigned)(p.slots() / BACK_TS), 256, r.back_lds, stream>>>(
            p.back_pre2, b.tpre2, b.k2, p.stat, p.tiles_per_group * TS, s.c2, s.co, s.s_out, s.pad3, b.W3p, dc->b3, b.norms);
        GEO_LAUNCH_CHECK();
        return GEO_OK;
    }
    const unsigned tiles = (unsigned)p.tiles, side_tiles = (unsigned)(p.tiles / 2), chunks = (unsigned)(p.groups() / 2);
    if (r.head_stream) {                          // (make_route: 16 outputs, no GroupNorm, back dedup or mfma)
        if (p.back == GEO_JVP_BACK_DEDUP) {       // as below, the compact primal rows stay on back_mfma_kernel
            head_stream_kernel<0><<<side_tiles, 256, 0, stream>>>(p.back_pre2, b.tpre2, b.k2, 1, p.tiles_per_group, s.co, s.s_out, b.W3b,
                                                                  dc->b3, b.norms, nullptr, nullptr, 2);
            back_mfma_kernel<1, false, 2><<<chunks, 256, 0, stream>>>(
                p.back_pre2, b.tpre2, b.k2, 1, p.tiles_per_group, s.co, s.s_out, b.W3b, dc->b3, b.norms, nullptr, b.sg_compact, nullptr,
                nullptr, 0, 0, 1, nullptr, 0, nullptr, b.n_compact, 1);
            head_stream_kernel<1><<<side_tiles, 256, 0, stream>>>(p.back_pre2, b.tpre2, b.k2, 1, p.tiles_per_group, s.co, s.s_out, b.W3b,
                                                                  dc->b3, b.norms, b.sg_compact, b.row_map, 1);
        } else {
            head_stream_kernel<0><<<tiles, 256, 0, stream>>>(p.back_pre2, b.tpre2, b.k2, p.stat, p.tiles_per_group, s.co, s.s_out, b.W3b,
                                                             dc->b3, b.norms, nullptr, nullptr, 0);
        }
        GEO_LAUNCH_CHECK();
        return GEO_OK;
    }
    pick_int<1, 6>(r.back_nt, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        if (p.back == GEO_JVP_BACK_DEDUP) {       // end side per slot; start side: the compact primal rows, then the tangents
            back_mfma_kernel<NT, false, 0><<<side_tiles, 256, 0, stream>>>(
                p.back_pre2, b.tpre2, b.k2, 1, p.tiles_per_group, s.co, s.s_out, b.W3b, dc->b3, b.norms, nullptr, nullptr, nullptr,
                nullptr, 0, 0, 1, nullptr, 0, nullptr, nullptr, 2);
            back_mfma_kernel<NT, false, 2><<<chunks, 256, 0, stream>>>(
                p.back_pre2, b.tpre2, b.k2, 1, p.tiles_per_group, s.co, s.s_out, b.W3b, dc->b3, b.norms, nullptr, b.sg_compact, nullptr,
                nullptr, 0, 0, 1, nullptr, 0, nullptr, b.n_compact, 1);
            back_mfma_kernel<NT, false, 1><<<side_tiles, 256, 0, stream>>>(
                p.back_pre2, b.tpre2, b.k2, 1, p.tiles_per_group, s.co, s.s_out, b.W3b, dc->b3, b.norms, nullptr, b.sg_compact, nullptr,
                nullptr, 0, 0, 1, nullptr, 0, b.row_map, nullptr, 1);
            return;
        }
        pick_bool(r.group_norm, [&](auto gn) {
            constexpr bool GN = decltype(gn)::value;
            if (p.back == GEO_JVP_BACK_MFMA)
                back_mfma_kernel<NT, GN, 0><<<tiles, 256, 0, stream>>>(p.back_pre2, b.tpre2, b.k2, p.stat, p.tiles_per_group, s.co,
                                                                      s.s_out, b.W3b, dc->b3, b.norms, b.gs2);
            else if (p.back == GEO_JVP_BACK_PER_NODE)           // tangent only, the primal from the slot's latent
                back_mfma_kernel<NT, GN, 1><<<tiles, 256, 0, stream>>>(p.back_pre2, b.tpre2, b.k2, 0, p.tiles_per_group, s.co, s.s_out,
                                                                      b.W3b, dc->b3, b.norms, b.gs2, b.sg_node, p.src, p.dst, p.e_base,
                                                                      p.n_edges, p.batch, b.jac, p.unit_d);
            else                                                // BACK_NODE_PRIMAL: primal only, keeps the output sigmoids
                back_mfma_kernel<NT, GN, 2><<<tiles, 256, 0, stream>>>(p.back_pre2, b.tpre2, b.k2, 0, p.tiles_per_group, s.co, s.s_out,
                                                                      b.W3b, dc->b3, b.norms, b.gs2, b.sg_node);
        });
    });
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

int launch_pass(const Route &r, const geo_decoder_desc *dc, const Pass &p, const Buffers &b, hipStream_t stream) {
    if (r.front_once)
        if (const int rc = launch_start_runs(p, b, stream)) return rc;
    if (const int rc = launch_front(r, p, b, stream)) return rc;
    if (const int rc = launch_stats(r, dc, 1, p, b, stream)) return rc;
    if (const int rc = launch_mid(r, dc, p, b, stream)) return rc;
    if (const int rc = launch_stats(r, dc, 2, p, b, stream)) return rc;
    return launch_back(r, dc, p, b, stream);
}

// ---------------------------------------------------------------------------------- host side: the run
// what geo_decoder_metric_tensor keeps of a slice of latents (eig / logvol / rank: all three null = no spectrum)
struct MetricOut { double *G, *eig, *logvol; int32_t *rank; };

// run_jvp is three steps, each a function of its own so that geo_curve_relax can carve and pack once and run the passes once per
// iteration: jvp_carve, jvp_pack, jvp_passes -- the same launches in the same order as ever.
int jvp_carve(const Route &r, int64_t n_nodes, void *ws, size_t ws_bytes, Buffers *bp) {
    const Plan &pl = r.pl;
    const Shape &s = pl.sh;
    const Tiling t = pl.tiling();
    Buffers &b = *bp;

    // ---- carve the workspace: the groups in the order make_route subtracts them (Jacobian columns, pass, per-node rows)
    geo::Arena ar(ws, ws_bytes);
    b = Buffers{};
    if (r.node_jacobian) lay_out_jacobian(ar, &b, s, n_nodes, r.run_edges, r.jac_np);
    lay_out_pass(ar, &b, s, t, r.group_norm);
    if (r.per_node) lay_out_nodes(ar, &b, s, n_nodes);
    // (unreachable: make_route took each route only where the measurements of these same functions fit in ws_bytes)
    GEO_REQUIRE(ar.ok(), "geo_decoder_jvp: workspace carve failed");
    if (r.dedup) StartRuns(s, t).place(&b, r.front_once);
    return GEO_OK;
}

// the packed weights and the fixed norm constants: functions of the decoder alone, read by every pass and written by none
int jvp_pack(const geo_decoder_desc *dc, const Route &r, Buffers *bp, hipStream_t stream) {
    const Shape &s = r.pl.sh;
    Buffers &b = *bp;
    make_chunks(s, &b.tab);
    int bad_chunk = 0;
    GEO_REQUIRE(!(s.n_chunks == 8 && s.opix_per_chunk == 2) || chunks_match_mid_geom(b.tab, &bad_chunk),
                "geo_decoder_jvp: chunk table / MidGeom mismatch (chunk %d)", bad_chunk);
    compose_front_kernel<<<geo::grid_for((int64_t)(s.d + 1) * s.n1, 256), 256, 0, stream>>>(
        dc->w_in, dc->b_in, dc->w1, dc->b1, s.d, s.c0, s.c1, b.M01, b.b01);
    GEO_LAUNCH_CHECK();
    pack_mid_kernel<<<geo::grid_for((int64_t)s.n_chunks * MAX_BLOCKS * s.c1 * NC, 256), 256, 0, stream>>>(
        dc->w2, s.c1, s.c2, b.tab, s.n_chunks, s.opix_per_chunk, b.B2p);
    GEO_LAUNCH_CHECK();
    pack_back_kernel<<<geo::grid_for(16 * s.co * s.c2, 256), 256, 0, stream>>>(dc->w3, s.c2, s.co, b.W3p);
    GEO_LAUNCH_CHECK();
    if (r.back != GEO_JVP_BACK_VALU) {
        pack_back_bf16_kernel<<<geo::grid_for((int64_t)16 * s.c2 * r.back_nt * 32, 256), 256, 0, stream>>>(
            dc->w3, s.c2, s.co, s.s_out, s.pad3, r.back_nt * 32, b.W3b);
        GEO_LAUNCH_CHECK();
    }
    pack_mid_bf16_kernel<<<geo::grid_for((int64_t)s.n_chunks * MAX_BLOCKS * s.c1 * NC, 256), 256, 0, stream>>>(
        b.B2p, s.c1, s.n_chunks, b.B3);
    GEO_LAUNCH_CHECK();
    if (!r.batch_stats) {
        finalize_fixed_kernel<<<1, 256, 0, stream>>>(s.c1, dc->norm, dc->g1, dc->be1, dc->rm1, dc->rv1, dc->eps, b.k1);
        GEO_LAUNCH_CHECK();
        finalize_fixed_kernel<<<1, 256, 0, stream>>>(s.c2, dc->norm, dc->g2, dc->be2, dc->rm2, dc->rv2, dc->eps, b.k2);
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}

int jvp_passes(const geo_decoder_desc *dc, const Route &r, const Buffers &b, const float *z, int64_t n_nodes, const int32_t *src,
               const int32_t *dst, const float *z_start, const float *z_end, int64_t n_edges, float *len_out, hipStream_t stream,
               const MetricOut *metric, bool columns_only = false) {
    const Plan &pl = r.pl;
    const Shape &s = pl.sh;
    const int batch = pl.batch;
    const size_t node_slots = round_up_to_tile(n_nodes);

    // ---- per-node primal pass: every latent once, its ConvT2 rows and output sigmoids kept
    if (r.per_node) {
        Pass np = {};                                          // (no edge list: "end points" z, z)
        np.mid = GEO_JVP_MID_ALL; np.back = BACK_NODE_PRIMAL;
        np.tiles = (int64_t)(node_slots / TS); np.tiles_per_group = (int)np.tiles;
        np.n_edges = n_nodes; np.batch = (int)node_slots;
        np.z_start = np.z_end = z; np.mid_pre2 = b.pre2_node; np.back_pre2 = b.pre2_node;
        if (const int rc = launch_pass(r, dc, np, b, stream)) return rc;
    }

    // ---- passes over the edges (node_jacobian: over the pseudo-edges, unit tangents, columns to b.jac instead of lengths)
    if (r.node_jacobian) {
        pair_edges_kernel<<<geo::grid_for(r.run_edges, 256), 256, 0, stream>>>(n_nodes, s.d, r.run_edges, b.psrc, b.pdst);
        GEO_LAUNCH_CHECK();
    }
    const int64_t total_chunks = (r.run_edges + batch - 1) / batch;
    for (int64_t c0 = 0; c0 < total_chunks; c0 += pl.chunks_per_pass) {
        const int64_t nch = std::min<int64_t>(total_chunks - c0, pl.chunks_per_pass);
        Pass ep = {};
        ep.mid = r.mid; ep.back = r.back;
        ep.tiles = nch * 2 * pl.tiles_per_group; ep.tiles_per_group = pl.tiles_per_group;
        ep.e_base = c0 * batch; ep.n_edges = r.run_edges; ep.batch = batch; ep.stat = r.batch_stats ? 1 : 0;
        ep.z = z; ep.src = r.node_jacobian ? b.psrc : src; ep.dst = r.node_jacobian ? b.pdst : dst;
        ep.z_start = z_start; ep.z_end = z_end;
        ep.unit_d = r.node_jacobian ? s.d : 0;
        ep.mid_pre2 = b.pre2; ep.back_pre2 = r.per_node ? b.pre2_node : b.pre2;
        slot_valid_kernel<<<geo::grid_for(ep.slots(), 256), 256, 0, stream>>>(ep.e_base, ep.n_edges, batch, pl.tiles_per_group,
                                                                             ep.slots(), b.slot_valid);
        GEO_LAUNCH_CHECK();
        if (const int rc = launch_pass(r, dc, ep, b, stream)) return rc;
        if (!r.node_jacobian) {
            const int64_t e_count = std::min<int64_t>(n_edges - ep.e_base, nch * batch);
            combine_kernel<<<geo::grid_for(e_count, 256), 256, 0, stream>>>(b.norms, ep.e_base, e_count, batch, pl.slots_per_group,
                                                                            len_out);
            GEO_LAUNCH_CHECK();
        }
    }
    if (columns_only) return GEO_OK;                            // (geo_curve_*: the columns and sigmoids are the result)
    if (r.node_jacobian && metric) {                            // G = J^T J per latent, then its spectrum
        jacobian_gram_kernel<<<geo::grid_for(n_nodes, 1), 256, 0, stream>>>(b.jac, n_nodes, s.d, s.p_out, (int)r.jac_np, metric->G);
        GEO_LAUNCH_CHECK();
        if (metric->eig || metric->logvol || metric->rank) {
            metric_spectrum_kernel<<<(unsigned)((n_nodes + SPEC_THREADS - 1) / SPEC_THREADS), SPEC_THREADS, 0, stream>>>(
                metric->G, n_nodes, s.d, s.p_out, metric->eig, metric->logvol, metric->rank);
            GEO_LAUNCH_CHECK();
        }
    } else if (r.node_jacobian) {                               // each edge end from its latent's columns
        const int64_t teams = (n_edges * 16 + 255) / 256;
        GEO_REQUIRE(teams < ((int64_t)1 << 31), "geo_decoder_jvp_edges: too many edges for one launch (%lld)", (long long)n_edges);
        jacobian_lengths_kernel<<<(unsigned)teams, 256, 0, stream>>>(z, src, dst, n_edges, s.d, s.p_out, (int)r.jac_np, b.jac, len_out);
        GEO_LAUNCH_CHECK();
    }
    return GEO_OK;
}

// graph edges (z, src, dst) or explicit end points (z_start, z_end); `r` is make_route's answer for exactly this call.
// metric (node_jacobian routes only): no edges are read and no lengths written; the columns are reduced to G and its spectrum.
int run_jvp(const geo_decoder_desc *dc, const Route &r, const float *z, int64_t n_nodes, const int32_t *src, const int32_t *dst,
            const float *z_start, const float *z_end, int64_t n_edges, float *len_out, void *ws, size_t ws_bytes,
            hipStream_t stream, const MetricOut *metric = nullptr) {
    Buffers b;
    if (const int rc = jvp_carve(r, n_nodes, ws, ws_bytes, &b)) return rc;
    if (const int rc = jvp_pack(dc, r, &b, stream)) return rc;
    return jvp_passes(dc, r, b, z, n_nodes, src, dst, z_start, z_end, n_edges, len_out, stream, metric);
}

// validation shared by the two entry points, then the route and the run
int decoder_jvp(const geo_decoder_desc *dc, const geo::Options &opt, bool graph_edges, const float *z, int64_t n_nodes,
                const int32_t *src, const int32_t *dst, const float *z_start, const float *z_end, int64_t n_edges,
                int64_t build_edges, int32_t batch, float *len_out, void *ws, size_t ws_bytes, void *stream) {
    GEO_REQUIRE(dc && len_out && ws, "geo_decoder_jvp: null pointer");
    GEO_REQUIRE(batch > 0, "geo_decoder_jvp: batch_size must be positive");
    if (n_edges == 0) return GEO_OK;
    Route r;
    if (!make_route(dc, opt, graph_edges, n_nodes, n_edges, build_edges, batch, &ws_bytes, &r)) {
        geo::set_error("%s", r.error);
        return r.status;
    }
    return run_jvp(dc, r, z, n_nodes, src, dst, z_start, z_end, n_edges, len_out, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------------- host side: metric tensor per latent
// The column pass of the node_jacobian route on its own, over slices of latents sized from the workspace.  The route of a slice is
// make_route's for a graph over the slice's latents with the Jacobian route forced (the edges-per-latent rule and the option
// jvp_node_jacobian do not enter); every other option acts as it does on geo_decoder_jvp_edges, and where one switches off a
// kernel the pass needs the call refuses instead of changing route.
constexpr int METRIC_BATCH = 512;                     // pseudo-edges per chunk (fixed statistics: tiling only)
constexpr int64_t METRIC_MAX_SLICE = 1 << 18;         // latents per slice at most (d = 1: one pass of slots holds them)
constexpr int64_t METRIC_MIN_SLICE = TS;              // the slice geo_metric_tensor_min_workspace_bytes sizes

bool metric_route(const geo_decoder_desc *dc, const geo::Options &o, int64_t n_slice, const size_t *ws_bytes, Route *r) {
    geo::Options forced = o;
    forced.jvp_node_jacobian = 2;
    return make_route(dc, forced, true, n_slice, 1, 1, METRIC_BATCH, ws_bytes, r) && r->node_jacobian && r->per_node;
}

// whether the call takes this decoder under these options; if not, why: status and text in `r`
bool metric_covers(const geo_decoder_desc *dc, const geo::Options &o, Route *r) {
    *r = Route{};
    if (!dc) return route_error(r, GEO_E_ARG, "geo_decoder_metric_tensor: null pointer");
    if (dc->norm == 1 && dc->bn_train)
        return route_error(r, GEO_E_ARG, "geo_decoder_metric_tensor: train-mode BatchNorm is not covered (a sample's Jacobian "
                                         "depends on its batch)");
    if (dc->latent_dim < 1 || dc->latent_dim > GRAM_MAX_D)
        return route_error(r, GEO_E_ARG, "geo_decoder_metric_tensor: latent_dim %d not in [1,%d]", dc->latent_dim, GRAM_MAX_D);
    if (metric_route(dc, o, METRIC_MIN_SLICE, nullptr, r) && r->pl.sh.p_out <= GRAM_MAX_P) return true;
    if (r->status != GEO_OK) { r->status = GEO_E_ARG; return false; }        // (make_route's text)
    return route_error(r, GEO_E_ARG, "geo_decoder_metric_tensor: no per-latent column pass for this decoder (c2 == 64 and 16, 32 or "
                                     "192 outputs), or an option (jvp_per_node, jvp_mid, jvp_back_valu) switches it off");
}

size_t metric_slice_bytes(const geo_decoder_desc *dc, const geo::Options &o, int64_t n_slice) {
    Route r;
    return metric_route(dc, o, n_slice, nullptr, &r) ? r.bytes : 0;
}

int decoder_metric_tensor(const geo_decoder_desc *dc, const float *z, int64_t n, const MetricOut &out, void *ws, size_t ws_bytes,
                          hipStream_t stream) {
    const geo::Options opt = geo::options();
    Route probe;
    if (!metric_covers(dc, opt, &probe)) {
        geo::set_error("%s", probe.error);
        return probe.status;
    }
    GEO_REQUIRE(n >= 0, "geo_decoder_metric_tensor: n %lld < 0", (long long)n);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(z && out.G && ws, "geo_decoder_metric_tensor: null pointer");
    const int d = dc->latent_dim;

    // ---- the slice length: everything (up to the cap) when it fits, else the largest whole number of tiles that does
    const int64_t cap = n < METRIC_MAX_SLICE ? n : METRIC_MAX_SLICE;
    int64_t slice = cap;
    const size_t cap_bytes = metric_slice_bytes(dc, opt, cap);
    if (!cap_bytes || ws_bytes < cap_bytes) {
        const size_t min_bytes = metric_slice_bytes(dc, opt, METRIC_MIN_SLICE);
        GEO_REQUIRE(min_bytes && ws_bytes >= min_bytes, "geo_decoder_metric_tensor: workspace of %zu bytes is below the minimum of %zu",
                    ws_bytes, min_bytes);
        int64_t lo = 1, hi = (cap + TS - 1) / TS;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            const size_t bytes = metric_slice_bytes(dc, opt, mid * TS);
            if (bytes && bytes <= ws_bytes) lo = mid; else hi = mid - 1;
        }
        slice = lo * TS;
    }
    // ---- the routes of a whole slice and of the last, shorter one: both settled before the first launch
    Route whole, last;
    const int64_t n_whole = n / slice, n_last = n % slice;
    GEO_REQUIRE(n_whole == 0 || metric_route(dc, opt, slice, &ws_bytes, &whole),
                "geo_decoder_metric_tensor: no column pass for a slice of %lld latents in %zu bytes", (long long)slice, ws_bytes);
    GEO_REQUIRE(n_last == 0 || metric_route(dc, opt, n_last, &ws_bytes, &last),
                "geo_decoder_metric_tensor: no column pass for a slice of %lld latents in %zu bytes", (long long)n_last, ws_bytes);

    for (int64_t base = 0; base < n; base += slice) {
        const int64_t ns = n - base < slice ? n - base : slice;
        const MetricOut so = {out.G + (size_t)base * d * d, out.eig ? out.eig + (size_t)base * d : nullptr,
                              out.logvol ? out.logvol + base : nullptr, out.rank ? out.rank + base : nullptr};
        if (const int rc = run_jvp(dc, ns == slice ? whole : last, z + (size_t)base * d, ns, nullptr, nullptr, nullptr, nullptr, 1,
                                   nullptr, ws, ws_bytes, stream, &so))
            return rc;
    }
    return GEO_OK;
}

// ---------------------------------------------------------------------------------- host side: curve energy and relaxation
// geo_curve_energy / geo_curve_relax.  C curves of F frames are C * F latents, curve after curve; a slice is
// whole curves, as many as fit in the workspace (at most METRIC_MAX_SLICE latents).  The workspace of a slice: the relaxation's
// state (lay_out_curves), then what the column pass of geo_decoder_metric_tensor takes for the slice's latents.  A slice is
// carved and its weights packed once; every evaluation after that is jvp_passes alone, then curve_reduce_kernel.
size_t curve_state_bytes(const geo_decoder_desc *dc, int64_t n_curves, int F) {
    CurveState st;
    return geo::measure(lay_out_curves, &st, n_curves, F, dc->latent_dim);
}

size_t curve_slice_bytes(const geo_decoder_desc *dc, const geo::Options &o, int64_t n_curves, int F) {
    const size_t columns = metric_slice_bytes(dc, o, n_curves * F);
    return columns ? curve_state_bytes(dc, n_curves, F) + columns : 0;
}

int64_t curve_slice_cap(int64_t C, int F) {
    const int64_t cap = METRIC_MAX_SLICE / F;
    return C < 1 ? 1 : (C < cap ? C : cap);
}

// one slice, carved and packed
struct CurveSlice {
    Route route;
    CurveState st;
    Buffers b;
    int64_t n_curves;
};

// what both entry points check before anything else, in the issue's order: coverage (train-mode BatchNorm included), F
int curve_check(const char *who, const geo_decoder_desc *dc, const geo::Options &opt, int64_t C, int F) {
    Route probe;
    if (!metric_covers(dc, opt, &probe)) {
        geo::set_error("%s: no column pass (%s)", who, probe.error);
        return GEO_E_ARG;
    }
    GEO_REQUIRE(F >= 2 && F <= CURVE_MAX_F, "%s: F %d not in [2,%d]", who, F, CURVE_MAX_F);
    GEO_REQUIRE(C >= 0, "%s: C %lld < 0", who, (long long)C);
    return GEO_OK;
}

// the curves per slice a workspace holds: everything (up to the cap) when it fits, else the largest count that does
int curve_slice_length(const char *who, const geo_decoder_desc *dc, const geo::Options &opt, int64_t C, int F, size_t ws_bytes,
                       int64_t *slice) {
    const int64_t cap = curve_slice_cap(C, F);
    const size_t cap_bytes = curve_slice_bytes(dc, opt, cap, F);
    *slice = cap;
    if (cap_bytes && ws_bytes >= cap_bytes) return GEO_OK;
    const size_t min_bytes = curve_slice_bytes(dc, opt, 1, F);
    GEO_REQUIRE(min_bytes && ws_bytes >= min_bytes, "%s: workspace of %zu bytes is below the minimum of %zu", who, ws_bytes, min_bytes);
    int64_t lo = 1, hi = cap;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        const size_t bytes = curve_slice_bytes(dc, opt, mid, F);
        if (bytes && bytes <= ws_bytes) lo = mid; else hi = mid - 1;
    }
    *slice = lo;
    return GEO_OK;
}

// host arithmetic only: the route and the carve of a slice of n_curves in this workspace
int curve_slice_plan(const char *who, const geo_decoder_desc *dc, const geo::Options &opt, int64_t n_curves, int F, void *ws,
                     size_t ws_bytes, CurveSlice *sl) {
    sl->n_curves = n_curves;
    geo::Arena ar(ws, ws_bytes);
    lay_out_curves(ar, &sl->st, n_curves, F, dc->latent_dim);
    GEO_REQUIRE(ar.ok(), "%s: workspace of %zu bytes does not hold the state of %lld curves", who, ws_bytes, (long long)n_curves);
    const size_t rest = ws_bytes - ar.off;
    GEO_REQUIRE(metric_route(dc, opt, n_curves * F, &rest, &sl->route), "%s: no column pass for a slice of %lld latents in %zu bytes",
                who, (long long)(n_curves * F), rest);
    return jvp_carve(sl->route, n_curves * F, static_cast<char *>(ws) + ar.off, rest, &sl->b);
}

// Evaluate: the primal and column passes over the slice's latents z, reduced per curve (tr / seg_sq / grad may be null)
int curve_evaluate(const geo_decoder_desc *dc, const CurveSlice &sl, const float *z, int F, double *energy, double *seg_sq,
                   double *grad, double *tr, hipStream_t stream) {
    const Shape &s = sl.route.pl.sh;
    if (const int rc = jvp_passes(dc, sl.route, sl.b, z, sl.n_curves * F, nullptr, nullptr, nullptr, nullptr, 1, nullptr, stream,
                                  nullptr, true))
        return rc;
    curve_reduce_kernel<<<geo::grid_for(sl.n_curves, 1), CURVE_THREADS, (size_t)F * (s.p_out + 1) * sizeof(float), stream>>>(
        sl.b.sg_node, (int)sl.route.jac_np, sl.b.jac, z, sl.n_curves, F, s.d, s.p_out, (int)sl.route.jac_np, energy, seg_sq, grad, tr);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

int curve_energy(const geo_decoder_desc *dc, const float *x, int64_t C, int F, double *energy_out, double *seg_sq_out,
                 double *grad_out, float *g_out, float *jac_out, void *ws, size_t ws_bytes, hipStream_t stream) {
    static const char who[] = "geo_curve_energy";
    const geo::Options opt = geo::options();
    if (const int rc = curve_check(who, dc, opt, C, F)) return rc;
    if (C == 0) return GEO_OK;
    GEO_REQUIRE(x && energy_out && ws, "%s: null pointer", who);
    int64_t slice = 0;
    if (const int rc = curve_slice_length(who, dc, opt, C, F, ws_bytes, &slice)) return rc;
    CurveSlice whole, last;
    const int64_t n_whole = C / slice, n_last = C % slice;
    if (n_whole)
        if (const int rc = curve_slice_plan(who, dc, opt, slice, F, ws, ws_bytes, &whole)) return rc;
    if (n_last)
        if (const int rc = curve_slice_plan(who, dc, opt, n_last, F, ws, ws_bytes, &last)) return rc;
    const int d = dc->latent_dim;
    for (int64_t base = 0; base < C; base += slice) {
        CurveSlice &sl = C - base < slice ? last : whole;
        const Shape &s = sl.route.pl.sh;
        const size_t at = (size_t)base * F;                       // the slice's first latent
        if (const int rc = jvp_pack(dc, sl.route, &sl.b, stream)) return rc;
        if (const int rc = curve_evaluate(dc, sl, x + at * d, F, energy_out + base,
                                          seg_sq_out ? seg_sq_out + (size_t)base * (F - 1) : nullptr,
                                          grad_out ? grad_out + at * d : nullptr, nullptr, stream))
            return rc;
        if (g_out || jac_out) {
            const int64_t n = sl.n_curves * F;
            curve_export_kernel<<<geo::grid_for(n * d * s.p_out, 256), 256, 0, stream>>>(
                sl.b.sg_node, (int)sl.route.jac_np, sl.b.jac, n, d, s.p_out, (int)sl.route.jac_np,
                g_out ? g_out + at * s.p_out : nullptr, jac_out ? jac_out + at * d * s.p_out : nullptr);
            GEO_LAUNCH_CHECK();
        }
    }
    return GEO_OK;
}

int curve_relax(const geo_decoder_desc *dc, float *x, int64_t C, int F, int n_iters, double *step, double *energy0_out,
                double *energy_out, double *seg_sq_out, int32_t *accepted_out, void *ws, size_t ws_bytes, hipStream_t stream) {
    static const char who[] = "geo_curve_relax";
    const geo::Options opt = geo::options();
    if (const int rc = curve_check(who, dc, opt, C, F)) return rc;
    GEO_REQUIRE(n_iters >= 0, "%s: n_iters %d < 0", who, n_iters);
    if (C == 0) return GEO_OK;
    GEO_REQUIRE(x && step && energy_out && accepted_out && ws, "%s: null pointer", who);
    int64_t slice = 0;
    if (const int rc = curve_slice_length(who, dc, opt, C, F, ws_bytes, &slice)) return rc;
    CurveSlice whole, last;
    const int64_t n_whole = C / slice, n_last = C % slice;
    if (n_whole)
        if (const int rc = curve_slice_plan(who, dc, opt, slice, F, ws, ws_bytes, &whole)) return rc;
    if (n_last)
        if (const int rc = curve_slice_plan(who, dc, opt, n_last, F, ws, ws_bytes, &last)) return rc;
    const int d = dc->latent_dim;
    const int iters = F == 2 ? 0 : n_iters;                       // no interior frame: nothing can move
    for (int64_t base = 0; base < C; base += slice) {
        CurveSlice &sl = C - base < slice ? last : whole;
        const CurveState &st = sl.st;
        float *xs = x + (size_t)base * F * d;
        double *seg_s = seg_sq_out ? seg_sq_out + (size_t)base * (F - 1) : nullptr;
        if (const int rc = jvp_pack(dc, sl.route, &sl.b, stream)) return rc;        // once per slice, not per iteration
        for (int it = -1; it < iters; ++it) {                     // it = -1: the curve itself
            if (it >= 0 && opt.curve_repack)                      // (measurement switch: what packing per iteration would cost)
                if (const int rc = jvp_pack(dc, sl.route, &sl.b, stream)) return rc;
            if (const int rc = curve_evaluate(dc, sl, it < 0 ? xs : st.y, F, st.e_ev, st.seg_ev, st.grad_ev, st.tr, stream)) return rc;
            curve_step_kernel<<<(unsigned)sl.n_curves, CURVE_THREADS, 0, stream>>>(
                st, xs, F, d, it < 0, it == iters - 1, step + base, energy0_out ? energy0_out + base : nullptr, energy_out + base,
                seg_s, accepted_out + base);
            GEO_LAUNCH_CHECK();
        }
    }
    return GEO_OK;
}

}  // namespace

#ifdef GEO_MID_PROF
extern "C" int geo_debug_mid_prof(unsigned long long *out, int reset) {
    if (reset) { unsigned long long z[16] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_mid_prof), z, sizeof(z)); }
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mid_prof), sizeof(unsigned long long) * 16);
}
#endif

extern "C" size_t geo_jvp_workspace_bytes(const geo_decoder_desc *dec, int64_t n_edges, int32_t batch_size) {
    const geo::Options opt = geo::options();
    Route r;
    make_route(dec, opt, false, 0, n_edges, n_edges, batch_size, nullptr, &r);
    return r.bytes;
}

extern "C" size_t geo_jvp_edges_part_workspace_bytes(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges,
                                                     int64_t build_edges, int32_t batch_size) {
    const geo::Options opt = geo::options();
    Route r;
    make_route(dec, opt, true, n_nodes, n_edges, build_edges, batch_size, nullptr, &r);
    return r.bytes;
}

extern "C" size_t geo_jvp_edges_workspace_bytes(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges,
                                                int32_t batch_size) {
    return geo_jvp_edges_part_workspace_bytes(dec, n_nodes, n_edges, n_edges, batch_size);
}

extern "C" int geo_jvp_plan_part(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int64_t build_edges,
                                 int32_t batch_size, int32_t graph_edges, size_t ws_bytes) {
    const geo::Options opt = geo::options();
    Route r;
    if (!make_route(dec, opt, graph_edges != 0, graph_edges ? n_nodes : 0, n_edges, build_edges, batch_size,
                    ws_bytes ? &ws_bytes : nullptr, &r)) {
        geo::set_error("%s", r.error);
        return r.status;
    }
    return encode_route(r);
}

extern "C" int geo_jvp_plan(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int32_t batch_size,
                            int32_t graph_edges, size_t ws_bytes) {
    return geo_jvp_plan_part(dec, n_nodes, n_edges, n_edges, batch_size, graph_edges, ws_bytes);
}

extern "C" int geo_jvp_head_stream(const geo_decoder_desc *dec, int64_t n_nodes, int64_t n_edges, int32_t batch_size,
                                   int32_t graph_edges) {
    const geo::Options opt = geo::options();
    Route r;
    if (!make_route(dec, opt, graph_edges != 0, graph_edges ? n_nodes : 0, n_edges, n_edges, batch_size, nullptr, &r)) {
        geo::set_error("%s", r.error);
        return r.status;
    }
    return r.head_stream ? 1 : 0;
}

extern "C" int geo_decoder_jvp_edges_part(const geo_decoder_desc *dec, const float *z, int64_t n_nodes, const int32_t *src,
                                          const int32_t *dst, int64_t n_edges, int64_t build_edges, int32_t batch_size,
                                          float *len_out, void *ws, size_t ws_bytes, void *stream) {
    GEO_REQUIRE(build_edges >= n_edges, "geo_decoder_jvp_edges_part: build_edges %lld < n_edges %lld", (long long)build_edges,
                (long long)n_edges);
    GEO_REQUIRE(n_edges == 0 || (z && src && dst && n_nodes > 0), "geo_decoder_jvp_edges: null pointer");
    const geo::Options opt = geo::options();
    return decoder_jvp(dec, opt, true, z, n_nodes, src, dst, nullptr, nullptr, n_edges, build_edges, batch_size, len_out, ws,
                       ws_bytes, stream);
}

extern "C" int geo_decoder_jvp_edges(const geo_decoder_desc *dec, const float *z, int64_t n_nodes, const int32_t *src,
                                     const int32_t *dst, int64_t n_edges, int32_t batch_size, float *len_out, void *ws,
                                     size_t ws_bytes, void *stream) {
    return geo_decoder_jvp_edges_part(dec, z, n_nodes, src, dst, n_edges, n_edges, batch_size, len_out, ws, ws_bytes, stream);
}

extern "C" int geo_decoder_jvp_pairs(const geo_decoder_desc *dec, const float *z_start, const float *z_end,
                                     int64_t n_edges, int32_t batch_size, float *len_out, void *ws, size_t ws_bytes,
                                     void *stream) {
    GEO_REQUIRE(n_edges == 0 || (z_start && z_end), "geo_decoder_jvp_pairs: null pointer");
    const geo::Options opt = geo::options();
    return decoder_jvp(dec, opt, false, nullptr, 0, nullptr, nullptr, z_start, z_end, n_edges, n_edges, batch_size, len_out, ws,
                       ws_bytes, stream);
}

extern "C" size_t geo_metric_tensor_workspace_bytes(const geo_decoder_desc *dec, int64_t n) {
    const geo::Options opt = geo::options();
    Route probe;
    if (!metric_covers(dec, opt, &probe)) return 0;
    return metric_slice_bytes(dec, opt, n < 1 ? 1 : (n < METRIC_MAX_SLICE ? n : METRIC_MAX_SLICE));
}

extern "C" size_t geo_metric_tensor_min_workspace_bytes(const geo_decoder_desc *dec) {
    const geo::Options opt = geo::options();
    Route probe;
    if (!metric_covers(dec, opt, &probe)) return 0;
    return metric_slice_bytes(dec, opt, METRIC_MIN_SLICE);
}

extern "C" int geo_decoder_metric_tensor(const geo_decoder_desc *dec, const float *z, int64_t n, double *G_out, double *eig_out,
                                         double *logvol_out, int32_t *rank_out, void *ws, size_t ws_bytes, void *stream) {
    const MetricOut out = {G_out, eig_out, logvol_out, rank_out};
    return decoder_metric_tensor(dec, z, n, out, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" size_t geo_curve_workspace_bytes(const geo_decoder_desc *dec, int64_t C, int32_t F) {
    const geo::Options opt = geo::options();
    Route probe;
    if (!metric_covers(dec, opt, &probe) || F < 2 || F > CURVE_MAX_F) return 0;
    return curve_slice_bytes(dec, opt, curve_slice_cap(C, F), F);
}

extern "C" size_t geo_curve_min_workspace_bytes(const geo_decoder_desc *dec, int32_t F) {
    const geo::Options opt = geo::options();
    Route probe;
    if (!metric_covers(dec, opt, &probe) || F < 2 || F > CURVE_MAX_F) return 0;
    return curve_slice_bytes(dec, opt, 1, F);
}

extern "C" int geo_curve_energy(const geo_decoder_desc *dec, const float *x, int64_t C, int32_t F, double *energy_out,
                                double *seg_sq_out, double *grad_out, float *g_out, float *jac_out, void *ws, size_t ws_bytes,
                                void *stream) {
    return curve_energy(dec, x, C, F, energy_out, seg_sq_out, grad_out, g_out, jac_out, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int geo_curve_relax(const geo_decoder_desc *dec, float *x_inout, int64_t C, int32_t F, int32_t n_iters,
                               double *step_inout, double *energy0_out, double *energy_out, double *seg_sq_out,
                               int32_t *accepted_out, void *ws, size_t ws_bytes, void *stream) {
    return curve_relax(dec, x_inout, C, F, n_iters, step_inout, energy0_out, energy_out, seg_sq_out, accepted_out, ws, ws_bytes,
                       static_cast<hipStream_t>(stream));
}
