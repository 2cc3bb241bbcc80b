// vanilla_jvp.hip -- pull-back edge lengths of the vanilla (vector-latent) VAE decoder with FIXED statistics on gfx950.
//
//   fc: Linear(d, c0*16) -> view c0x4x4 -> ConvT(c0,c1,k3,s2,p1[,op]) -> norm -> ReLU -> ConvT(c1,c2,k4,s2,p1) -> norm -> ReLU
//       -> ConvT(c2,C,k4,s2,p1) -> sigmoid,     4 -> 7 -> 14 -> 28 px  |  4 -> 8 -> 16 -> 32 px
//   len[e] = 0.5 (|J(z_a) dz| + |J(z_b) dz|),  dz = z_b - z_a                              
//
// With eval-mode BatchNorm (or no norm) everything up to the first norm's scale and shift is affine in z; the export composes
// it once in fp64: pre1 = z . At + c, At [d_even][n1], n1 = s1^2 c1, column = pixel * c1 + channel.  What the tangent needs
// from a point are the two ReLU sign masks (bits) and sigmoid' of the output.  Two passes over one layout:
//
//   point pass (per latent slot)   vj_front_kernel<false>  pre1 on v_mfma_f32_32x32x2_f32 -> mask1 bits, relu(pre1)
//                                  vj_mid_kernel<.., false> ConvT2 + folded norm2 -> mask2 bits, relu
//                                  vj_back_kernel<.., false> ConvT3 + bias -> sigmoid'
//   edge pass (per edge)           vj_front_kernel<true>   t1 = dz . At, once per edge (the same at both ends)
//                                  vj_mid_kernel<.., true>  per end: mask1 -> ConvT2 tangent -> scale2 -> mask2
//                                  vj_back_kernel<.., true> per end: ConvT3 tangent -> sigmoid' scale -> sum of squares; len[e]
//
// The image decode at the end of this file (geo_vanilla_decode, geo_spatial_decode) runs the point pass's
// front and mid without the masks and writes the logits instead of sigmoid'.
// The vector-Jacobian product (geo_vanilla_vjp) and the curve energy and relaxation built on it (geo_vanilla_curve_energy,
// geo_vanilla_curve_relax) run the point pass as it is and then the three layers backwards.
// The same for whole 4 x 4 grids under the spatial decoder (geo_spatial_vjp, geo_spatial_curve_energy, geo_spatial_curve_relax;
// DESIGN.md section 29): the image decode's first stage with the mask bits, the two shared layers at s1 = 8, and a first-stage
// adjoint of its own.
// The metric tensor per latent (geo_vanilla_metric_tensor) runs the point pass and the edge pass over unit
// tangents, keeps the columns vj_back_kernel forms and reduces them to G = J^T J in fp64 (vm_gram_kernel); its eigenvalues are
// csrc/sym_spectrum.hip's.
//
// ConvT2 (k4, s2, p1) is four implicit GEMMs, one per output-pixel parity: out[(2y+py, 2x+px)][co] = sum over the taps
// (a, b) in {0,1}^2 and ci of in[(y+py-a, x+px-b)][ci] w2[ci][co][2a+1-py][2b+1-px]; M = (item, pixel) rows, K = 4 c1, N = c2, on
// the exact-f32 matrix instruction.  Every value is a fixed-order fmaf chain of its own row, no atomics: a length does not
// depend on the pass size, the position in a pass, the entry point, the run or the stream.  dz = 0 gives exactly 0.
#include "geo_common.h"
#include "mfma_conv.h"
#include "curve_step.h"

#include <vector>

namespace {

using mfma_conv::f32x16;

constexpr int MAX_D = 128;
constexpr int64_t EDGES_PER_PASS = 2048;        // at most this many edges (twice as many items) per pass
constexpr int FRONT_ROWS = 64, FRONT_SPLIT = 4;
constexpr int MID_ROWS = 256;                   // (item, pixel) rows of one mid workgroup: 4 items at 8x8, 5 at 7x7

struct Shape {
    int d, dp, c1, c2, co, s1, s2, S, n1, n2, nout, G;
};

bool make_shape(const geo_vanilla_decoder_desc *dc, Shape *s) {
    if (!dc) return false;
    if (dc->latent_dim < 1 || dc->latent_dim > MAX_D) return false;
    if (!((dc->c1 == 128 && dc->c2 == 64) || (dc->c1 == 64 && dc->c2 == 32))) return false;
    if (dc->out_channels != 1 && dc->out_channels != 3) return false;
    if (dc->out_size != 28 && dc->out_size != 32) return false;
    s->d = dc->latent_dim;
    s->dp = (s->d + 1) & ~1;
    s->c1 = dc->c1;
    s->c2 = dc->c2;
    s->co = dc->out_channels;
    s->S = dc->out_size;
    s->s2 = s->S / 2;
    s->s1 = s->S / 4;
    s->n1 = s->s1 * s->s1 * s->c1;
    s->n2 = s->s2 * s->s2 * s->c2;
    s->nout = s->co * s->S * s->S;
    s->G = MID_ROWS / (s->s1 * s->s1);
    return true;
}

// Workspace: per point slot the two masks and sigmoid'; per pass of EB edges the front's and the mid's outputs of 2 EB items.
// One layout: the queries and run()'s shrink loop measure it, run() carves with it.
struct Workspace { uint32_t *mask1, *mask2; float *sigp, *buf1, *buf2; };
Workspace lay_out(geo::Arena &ar, const Shape &s, int64_t slots, int64_t eb) {
    Workspace w;
    ar.take(w.mask1, (size_t)slots * (s.n1 / 32)); ar.take(w.mask2, (size_t)slots * (s.n2 / 32));
    ar.take(w.sigp, (size_t)slots * s.nout);
    ar.take(w.buf1, (size_t)2 * eb * s.n1); ar.take(w.buf2, (size_t)2 * eb * s.n2);
    return w;
}
size_t layout_bytes(const Shape &s, int64_t slots, int64_t eb) { return geo::measure(lay_out, s, slots, eb); }

// Where the latents of a pass come from.  List A holds the start points, list B the end points: entry i of a list is row
// (index ? index[base + i] : base + i) of its array.  The points of a point pass are A[0 .. nA) followed by B[0 ..).
struct Ends {
    const float *zA, *zB;
    const int32_t *iA, *iB;
    int64_t base;
    int nA;
};

__device__ __forceinline__ const float *row_a(const Ends &s, int64_t i, int d) {
    return s.zA + (size_t)(s.iA ? (int64_t)s.iA[s.base + i] : s.base + i) * d;
}
__device__ __forceinline__ const float *row_b(const Ends &s, int64_t i, int d) {
    return s.zB + (size_t)(s.iB ? (int64_t)s.iB[s.base + i] : s.base + i) * d;
}
// The slot of item (edge l, side): the latent's own index when the point pass ran over the resident latents, else its
// position in the pass's point list.
__device__ __forceinline__ int64_t item_slot(const Ends &s, int resident, int64_t l, int side) {
    if (resident) return side ? (int64_t)s.iB[s.base + l] : (int64_t)s.iA[s.base + l];
    return side ? (int64_t)s.nA + l : l;
}

// ---- front: rows of z (points) or of dz (edges) times At on the f32 matrix cores; a workgroup = 64 rows x a quarter of
// the column tiles, a wave = two 32 x 32 tiles sharing the B operand.  The chain starts at c (points) or 0 (edges).
// MASKS = false (the image decode): relu(pre1) only, no sign bits.
template <bool EDGE, bool MASKS = true>
__global__ __launch_bounds__(256) void vj_front_kernel(Ends s, int count, int d, int dp, int n1, const float *__restrict__ At,
                                                       const float *__restrict__ c, float *__restrict__ out,
                                                       uint32_t *__restrict__ mask1, int64_t slot0) {
    __shared__ float zs[FRONT_ROWS][MAX_D + 1];
    const int64_t tile0 = (int64_t)blockIdx.x * FRONT_ROWS;
    for (int q = threadIdx.x; q < FRONT_ROWS * dp; q += 256) {
        const int r = q / dp, k = q - r * dp;
        const int64_t p = tile0 + r;
        float v = 0.f;
        if (p < count && k < d) {
            if (EDGE) v = row_b(s, p, d)[k] - row_a(s, p, d)[k];
            else v = p < s.nA ? row_a(s, p, d)[k] : row_b(s, p - s.nA, d)[k];
        }
        zs[r][k] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int ntiles = n1 / 32;
    for (int ct = blockIdx.y * 4 + wave; ct < ntiles; ct += 4 * gridDim.y) {
        const int n = ct * 32 + r;
        const float init = EDGE ? 0.f : c[n];
        f32x16 acc0, acc1;
#pragma unroll
        for (int q = 0; q < 16; ++q) { acc0[q] = init; acc1[q] = init; }
        for (int i = 0; i < dp / 2; ++i) {
            const int k = 2 * i + h;
            const float bm = At[(size_t)k * n1 + n];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(zs[r][k], bm, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(zs[32 + r][k], bm, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = mfma_conv::acc_row(q, h, m * 32);
                const int64_t p = tile0 + row;
                const float x = m ? acc1[q] : acc0[q];
                if (EDGE) {
                    if (p < count) out[(size_t)p * n1 + n] = x;
                } else if (MASKS) {
                    const unsigned long long bits = __ballot(x > 0.f);     // low half: the h = 0 row, high half: the h = 1 row
                    if (p < count) {
                        out[(size_t)p * n1 + n] = x > 0.f ? x : 0.f;
                        if (r == 0) mask1[(size_t)(slot0 + p) * ntiles + ct] = (uint32_t)(h ? bits >> 32 : bits);
                    }
                } else if (p < count) {
                    out[(size_t)p * n1 + n] = x > 0.f ? x : 0.f;
                }
            }
        }
    }
}

// ---- mid: ConvT2 of G items.  The items' inputs ([pixel][c1], masked for the tangent) are staged in LDS in mfma_conv.h's
// layout.  8 waves: wave = (N tile, M tiles sharing the B read); K runs over (tap, 8-channel block).
// w2p: [parity][tap][c1 / 4][c2][4].
// MASKS = false (the image decode, primal only): no sign bits, mask1 / mask2 may be null.
template <int C1, int C2, bool TANGENT, bool MASKS = true>
__global__ __launch_bounds__(512) void vj_mid_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                     const uint32_t *__restrict__ mask1, uint32_t *__restrict__ mask2, Ends s,
                                                     int resident, int64_t slot0, int64_t n_items, int s1, int G,
                                                     const float *__restrict__ w2p, const float *__restrict__ sc2,
                                                     const float *__restrict__ sh2) {
    constexpr int LD = C1 + 4, TN = C2 / 32, WPN = 8 / TN, MT = TN;
    __shared__ __attribute__((aligned(16))) float lds[(MID_ROWS + 1) * LD];
    __shared__ int64_t slot_s[8];
    const int P = s1 * s1, s2 = 2 * s1, n1 = P * C1, n2 = 4 * P * C2;
    const int rows = G * P, ZR = rows;
    const int64_t item0 = (int64_t)blockIdx.x * G;
    const int tid = threadIdx.x;
    if (tid < G) {
        const int64_t it = item0 + tid;
        int64_t slot = -1;
        if (it < n_items) slot = TANGENT ? item_slot(s, resident, it >> 1, (int)(it & 1)) : slot0 + it;
        slot_s[tid] = slot;
    }
    __syncthreads();
    for (int g = 0; g < G; ++g) {
        const int64_t slot = slot_s[g], it = item0 + g;
        const float4 *src = reinterpret_cast<const float4 *>(in + (size_t)(TANGENT ? it >> 1 : it) * n1);
        const uint32_t *mk = mask1 + (size_t)(slot < 0 ? 0 : slot) * (n1 / 32);
        for (int q = tid; q < n1 / 4; q += 512) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (slot >= 0) {
                v = src[q];
                if (TANGENT) {
                    const uint32_t nib = mk[q >> 3] >> ((q & 7) * 4);
                    if (!(nib & 1)) v.x = 0.f;
                    if (!(nib & 2)) v.y = 0.f;
                    if (!(nib & 4)) v.z = 0.f;
                    if (!(nib & 8)) v.w = 0.f;
                }
            }
            const int pix = (q * 4) / C1, ci = (q * 4) % C1;
            *reinterpret_cast<float4 *>(lds + (size_t)(g * P + pix) * LD + ci) = v;
        }
    }
    mfma_conv::fill_zero_row<512>(lds, ZR, LD, tid);
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int nt = wave % TN, m0 = wave / TN;
    int rg[MT], ry[MT], rx[MT];
    bool rv[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r = (m0 + m * WPN) * 32 + j;
        rv[m] = r < rows;
        rg[m] = rv[m] ? r / P : 0;
        const int pq = rv[m] ? r - rg[m] * P : 0;
        ry[m] = pq / s1;
        rx[m] = pq - ry[m] * s1;
    }
    const int co = nt * 32 + j;
    const float scale = sc2[co], shift = sh2[co];
    for (int par = 0; par < 4; ++par) {
        const int py = par >> 1, px = par & 1;
        f32x16 acc[MT];
        mfma_conv::clear(acc);
        for (int tap = 0; tap < 4; ++tap) {
            const int a = tap >> 1, b = tap & 1;
            const float *ap[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
                ap[m] = mfma_conv::tap_row(lds, LD, ZR, rv[m], rg[m], ry[m] + py - a, rx[m] + px - b, s1, P, h);
            const float4 *wp = reinterpret_cast<const float4 *>(w2p) + ((size_t)(par * 4 + tap) * (C1 / 4) + h) * C2 + co;
            mfma_conv::k_chain<MT, 4>(acc, ap, wp, C1 / 8, C2);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = mfma_conv::acc_row(q, h, (m0 + m * WPN) * 32);
                const int g = r < rows ? r / P : 0;
                const int64_t slot = r < rows ? slot_s[g] : -1;
                const bool valid = slot >= 0;
                const int pq = r - g * P, y = pq / s1, x = pq - y * s1;
                const int opix = (2 * y + py) * s2 + 2 * x + px;
                const size_t o = (size_t)(item0 + g) * n2 + (size_t)opix * C2 + co;
                const size_t w = (size_t)(valid ? slot : 0) * (n2 / 32) + (size_t)opix * TN + nt;
                if (TANGENT) {
                    if (valid) out[o] = (mask2[w] >> j) & 1u ? scale * acc[m][q] : 0.f;
                } else if (MASKS) {
                    const float x2 = fmaf(scale, acc[m][q], shift);
                    const unsigned long long bits = __ballot(x2 > 0.f);
                    if (valid) {
                        out[o] = x2 > 0.f ? x2 : 0.f;
                        if (j == 0) mask2[w] = (uint32_t)(h ? bits >> 32 : bits);
                    }
                } else if (valid) {
                    const float x2 = fmaf(scale, acc[m][q], shift);
                    out[o] = x2 > 0.f ? x2 : 0.f;
                }
            }
        }
    }
}

// ---- back: ConvT3 (same parity form, w3p [parity][tap][C][c2]: uniform reads) of one item per workgroup, the input
// ([pixel][c2]) in LDS.  Point pass: sigmoid' = e / (1 + e)^2, e = exp(-|logit|), to the slot.  Edge pass: both ends of one
// edge in turn; squares summed per thread in position order, then a fixed tree over the wave and the four waves in order.
// SQ (edge pass): len_out [2 E] takes each end's sum of squares instead of the edge's length.  G_OUT (point pass): g_out takes
// the sigmoid itself beside sigmoid', from the same e: 1 / (1 + e) for a logit >= 0, else e / (1 + e); g_out [slot][C][So][So] is the
// window of rows and columns crop .. S - crop - 1 (crop = 2: the spatial decoder at 28 px), sigmoid' always the whole S x S.
// COLS (edge pass): g_out [2 E][nout] also takes the columns themselves, v = sigmoid' * tangent, per item (edge, end), before they
// are squared (geo_vanilla_metric_tensor); nothing else changes.
template <int C2, int CO, bool TANGENT, bool SQ = false, bool G_OUT = false, bool COLS = false>
__global__ __launch_bounds__(256) void vj_back_kernel(const float *__restrict__ in, float *__restrict__ sigp, Ends s,
                                                      int resident, int64_t slot0, int s2, const float *__restrict__ w3p,
                                                      const float *__restrict__ b3, float *__restrict__ len_out,
                                                      float *__restrict__ g_out, int crop) {
    constexpr int LD = C2 + 4;
    __shared__ __attribute__((aligned(16))) float lds[(MID_ROWS + 1) * LD];
    __shared__ float wsum[4];
    const int P2 = s2 * s2, S = 2 * s2, n2 = P2 * C2, nout = CO * S * S, ZR = P2;
    const int tid = threadIdx.x;
    float norm[2] = {0.f, 0.f};
    for (int side = 0; side < (TANGENT ? 2 : 1); ++side) {
        const int64_t it = TANGENT ? 2 * (int64_t)blockIdx.x + side : (int64_t)blockIdx.x;
        const int64_t slot = TANGENT ? item_slot(s, resident, blockIdx.x, side) : slot0 + it;
        float *sg = sigp + (size_t)slot * nout;
        __syncthreads();
        mfma_conv::stage_rows<C2, 256>(lds, in + (size_t)it * n2, P2, tid);
        mfma_conv::fill_zero_row<256>(lds, ZR, LD, tid);
        __syncthreads();
        float ss = 0.f;
        for (int par = 0; par < 4; ++par) {
            const int py = par >> 1, px = par & 1;
            for (int pos = tid; pos < P2; pos += 256) {
                const int y = pos / s2, x = pos - y * s2;
                float acc[CO];
#pragma unroll
                for (int c = 0; c < CO; ++c) acc[c] = TANGENT ? 0.f : b3[c];
                for (int tap = 0; tap < 4; ++tap) {
                    const int iy = y + py - (tap >> 1), ix = x + px - (tap & 1);
                    const bool ok = iy >= 0 && iy < s2 && ix >= 0 && ix < s2;
                    const float *ar = lds + (size_t)(ok ? iy * s2 + ix : ZR) * LD;
                    const float *wr = w3p + (size_t)(par * 4 + tap) * CO * C2;
#pragma unroll 4
                    for (int cb = 0; cb < C2 / 4; ++cb) {
                        const float4 av = *reinterpret_cast<const float4 *>(ar + cb * 4);
#pragma unroll
                        for (int c = 0; c < CO; ++c) {
                            const float *w = wr + c * C2 + cb * 4;
                            acc[c] = fmaf(av.x, w[0], acc[c]);
                            acc[c] = fmaf(av.y, w[1], acc[c]);
                            acc[c] = fmaf(av.z, w[2], acc[c]);
                            acc[c] = fmaf(av.w, w[3], acc[c]);
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < CO; ++c) {
                    const size_t o = ((size_t)c * S + (2 * y + py)) * S + 2 * x + px;
                    if (TANGENT) {
                        const float v = sg[o] * acc[c];
                        if (COLS) g_out[(size_t)it * nout + o] = v;
                        ss = fmaf(v, v, ss);
                    } else {
                        const float e = expf(-fabsf(acc[c]));
                        sg[o] = e / ((1.f + e) * (1.f + e));
                        if (G_OUT) {
                            const int So = S - 2 * crop, oy = 2 * y + py - crop, ox = 2 * x + px - crop;
                            if (oy >= 0 && oy < So && ox >= 0 && ox < So)
                                g_out[((size_t)(slot * CO + c) * So + oy) * So + ox] = acc[c] >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
                        }
                    }
                }
            }
        }
        if (TANGENT) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
            if ((tid & 63) == 0) wsum[tid >> 6] = ss;
            __syncthreads();
            if (SQ) { if (tid == 0) len_out[it] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]; }
            else norm[side] = sqrtf(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
        }
    }
    if (TANGENT && !SQ && tid == 0) len_out[blockIdx.x] = 0.5f * (norm[0] + norm[1]);
}

template <int C1, int C2, bool TANGENT>
int launch_mid(const Shape &sh, const geo_vanilla_decoder_desc *dc, const float *in, float *out, const uint32_t *mask1,
               uint32_t *mask2, const Ends &e, int resident, int64_t slot0, int64_t n_items, hipStream_t st) {
    const unsigned grid = (unsigned)((n_items + sh.G - 1) / sh.G);
    vj_mid_kernel<C1, C2, TANGENT><<<grid, 512, 0, st>>>(in, out, mask1, mask2, e, resident, slot0, n_items, sh.s1, sh.G, dc->w2p,
                                                         dc->scale2, dc->shift2);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

template <bool TANGENT>
int run_mid(const Shape &sh, const geo_vanilla_decoder_desc *dc, const float *in, float *out, const uint32_t *mask1, uint32_t *mask2,
            const Ends &e, int resident, int64_t slot0, int64_t n_items, hipStream_t st) {
    if (sh.c1 == 128) return launch_mid<128, 64, TANGENT>(sh, dc, in, out, mask1, mask2, e, resident, slot0, n_items, st);
    return launch_mid<64, 32, TANGENT>(sh, dc, in, out, mask1, mask2, e, resident, slot0, n_items, st);
}

template <bool TANGENT, bool SQ = false, bool G_OUT = false, bool COLS = false>
int run_back(const Shape &sh, const geo_vanilla_decoder_desc *dc, const float *in, float *sigp, const Ends &e, int resident,
             int64_t slot0, int64_t blocks, float *len_out, hipStream_t st, float *g_out = nullptr, int crop = 0) {
    const unsigned grid = (unsigned)blocks;
#define VJ_BACK(C2_, CO_)                                                                                                     \
    vj_back_kernel<C2_, CO_, TANGENT, SQ, G_OUT, COLS><<<grid, 256, 0, st>>>(in, sigp, e, resident, slot0, sh.s2, dc->w3p, dc->b3,     \
                                                                        len_out, g_out, crop)
    if (sh.c2 == 64 && sh.co == 1) VJ_BACK(64, 1);
    else if (sh.c2 == 64) VJ_BACK(64, 3);
    else if (sh.co == 1) VJ_BACK(32, 1);
    else VJ_BACK(32, 3);
#undef VJ_BACK
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// The point pass over `count` latents of e's lists: masks and sigmoid' to slots slot0 .., the activations through w.buf1 / w.buf2;
// g_out (may be null): the sigmoids [slot][nout] as well.
int run_point_pass(const geo_vanilla_decoder_desc *dc, const Shape &sh, const Workspace &w, const Ends &e, int64_t count,
                   int64_t slot0, hipStream_t st, float *g_out = nullptr) {
    const dim3 grid((unsigned)((count + FRONT_ROWS - 1) / FRONT_ROWS), FRONT_SPLIT);
    vj_front_kernel<false><<<grid, 256, 0, st>>>(e, (int)count, sh.d, sh.dp, sh.n1, dc->At, dc->c, w.buf1, w.mask1, slot0);
    GEO_LAUNCH_CHECK();
    int rc = run_mid<false>(sh, dc, w.buf1, w.buf2, w.mask1, w.mask2, e, 0, slot0, count, st);
    if (rc != GEO_OK) return rc;
    if (g_out) return run_back<false, false, true>(sh, dc, w.buf2, w.sigp, e, 0, slot0, count, nullptr, st, g_out);
    return run_back<false>(sh, dc, w.buf2, w.sigp, e, 0, slot0, count, nullptr, st);
}

// n_resident > 0: the point pass runs once over the latents z[0 .. n_resident) and the edges index them (iA = src, iB = dst);
// 0: every pass runs the point pass over its own 2 EB edge ends.  The same kernels and the same chains either way.
int run(const geo_vanilla_decoder_desc *dc, const Shape &sh, const float *zA, const float *zB, const int32_t *iA, const int32_t *iB,
        int64_t n_resident, int64_t n_edges, float *len_out, void *ws, size_t ws_bytes, hipStream_t st, const char *who) {
    const int resident = n_resident > 0;
    int64_t eb = n_edges < EDGES_PER_PASS ? n_edges : EDGES_PER_PASS;
    while (eb >= 1 && layout_bytes(sh, resident ? n_resident : 2 * eb, eb) > ws_bytes) eb = geo::shrink_pass(eb);
    if (eb < 1) {
        geo::set_error("%s: workspace of %zu bytes is below the minimum of %zu", who, ws_bytes,
                       layout_bytes(sh, resident ? n_resident : 2, 1));
        return GEO_E_WORKSPACE;
    }
    const int64_t slots = resident ? n_resident : 2 * eb;
    geo::Arena ar(ws, ws_bytes);
    const Workspace w = lay_out(ar, sh, slots, eb);
    if (!ar.ok()) {                                             // (unreachable: the shrink loop measured this layout)
        geo::set_error("%s: workspace too small", who);
        return GEO_E_WORKSPACE;
    }
    auto point_pass = [&](const Ends &e, int64_t count, int64_t slot0) -> int { return run_point_pass(dc, sh, w, e, count, slot0, st); };
    if (resident)
        for (int64_t p0 = 0; p0 < n_resident; p0 += 2 * eb) {
            const int64_t cnt = n_resident - p0 < 2 * eb ? n_resident - p0 : 2 * eb;
            const Ends e{zA, zA, nullptr, nullptr, p0, (int)cnt};
            int rc = point_pass(e, cnt, p0);
            if (rc != GEO_OK) return rc;
        }
    for (int64_t e0 = 0; e0 < n_edges; e0 += eb) {
        const int64_t ne = n_edges - e0 < eb ? n_edges - e0 : eb;
        const Ends e{zA, zB, iA, iB, e0, (int)ne};
        if (!resident) {
            int rc = point_pass(e, 2 * ne, 0);
            if (rc != GEO_OK) return rc;
        }
        const dim3 grid((unsigned)((ne + FRONT_ROWS - 1) / FRONT_ROWS), FRONT_SPLIT);
        vj_front_kernel<true><<<grid, 256, 0, st>>>(e, (int)ne, sh.d, sh.dp, sh.n1, dc->At, dc->c, w.buf1, nullptr, 0);
        GEO_LAUNCH_CHECK();
        int rc = run_mid<true>(sh, dc, w.buf1, w.buf2, w.mask1, w.mask2, e, resident, 0, 2 * ne, st);
        if (rc != GEO_OK) return rc;
        rc = run_back<true>(sh, dc, w.buf2, w.sigp, e, resident, 0, ne, len_out + e0, st);
        if (rc != GEO_OK) return rc;
    }
    return GEO_OK;
}

int check_desc(const geo_vanilla_decoder_desc *dc, Shape *sh, const char *who) {
    GEO_REQUIRE(make_shape(dc, sh), "%s: decoder configuration not covered (see geo_hip.h)", who);
    GEO_REQUIRE(dc->At && dc->c && dc->w2p && dc->w3p && dc->scale2 && dc->shift2 && dc->b3, "%s: null pointer in the descriptor", who);
    return GEO_OK;
}

// ================================ image decode ================================
// The primal chain alone, kept whole: front -> mid -> an image-writing ConvT3.  The vanilla decoder reuses the point
// pass's front and mid with MASKS = false; the spatial decoder (conv_in 1x1 -> ConvT1 k4 s2 p1 -> norm -> ReLU, then the same
// two layers at 8x8 -> 16x16 -> 32x32) has a first stage of its own and shares the other two.  Workspace: the two
// activation buffers of a pass, nothing else.

constexpr int64_t ITEMS_PER_PASS = 4096;
constexpr int SD_MAX_D = 64;
constexpr int SD_MAX_DP = (SD_MAX_D + 1 + 7) & ~7;      // latent channels + the constant-one channel, in 8-channel K blocks
constexpr int SD_ITEMS = MID_ROWS / 16;                 // 16 grids of 4 x 4 per first-stage workgroup

// ---- ConvT3 of one item per workgroup, as vj_back_kernel's point pass computes the logit (the same chain: b3, then taps
// 0..3, channels in order), written to logits [C][So][So], So = 2 s2 - 2 crop: output rows and columns crop .. 2 s2 - crop - 1
// (crop = 2 is the spatial decoder's padding 3 at 28 px: exactly the 32-px output without a border of two).
template <int C2, int CO>
__global__ __launch_bounds__(256) void vj_image_kernel(const float *__restrict__ in, float *__restrict__ logits, int s2, int crop,
                                                       const float *__restrict__ w3p, const float *__restrict__ b3) {
    constexpr int LD = C2 + 4;
    __shared__ __attribute__((aligned(16))) float lds[(MID_ROWS + 1) * LD];
    const int P2 = s2 * s2, S = 2 * s2, So = S - 2 * crop, n2 = P2 * C2, ZR = P2;
    const int tid = threadIdx.x;
    float *img = logits + (size_t)blockIdx.x * CO * So * So;
    mfma_conv::stage_rows<C2, 256>(lds, in + (size_t)blockIdx.x * n2, P2, tid);
    mfma_conv::fill_zero_row<256>(lds, ZR, LD, tid);
    __syncthreads();
    for (int par = 0; par < 4; ++par) {
        const int py = par >> 1, px = par & 1;
        for (int pos = tid; pos < P2; pos += 256) {
            const int y = pos / s2, x = pos - y * s2;
            const int oy = 2 * y + py - crop, ox = 2 * x + px - crop;
            if (oy < 0 || oy >= So || ox < 0 || ox >= So) continue;
            float acc[CO];
#pragma unroll
            for (int c = 0; c < CO; ++c) acc[c] = b3[c];
            for (int tap = 0; tap < 4; ++tap) {
                const int iy = y + py - (tap >> 1), ix = x + px - (tap & 1);
                const bool ok = iy >= 0 && iy < s2 && ix >= 0 && ix < s2;
                const float *ar = lds + (size_t)(ok ? iy * s2 + ix : ZR) * LD;
                const float *wr = w3p + (size_t)(par * 4 + tap) * CO * C2;
#pragma unroll 4
                for (int cb = 0; cb < C2 / 4; ++cb) {
                    const float4 av = *reinterpret_cast<const float4 *>(ar + cb * 4);
#pragma unroll
                    for (int c = 0; c < CO; ++c) {
                        const float *w = wr + c * C2 + cb * 4;
                        acc[c] = fmaf(av.x, w[0], acc[c]);
                        acc[c] = fmaf(av.y, w[1], acc[c]);
                        acc[c] = fmaf(av.z, w[2], acc[c]);
                        acc[c] = fmaf(av.w, w[3], acc[c]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < CO; ++c) img[((size_t)c * So + oy) * So + ox] = acc[c];
        }
    }
}

// ---- the spatial decoder's first stage: conv_in composed into ConvT1 (w1p), four parity GEMMs in vj_mid_kernel's form.
// M = (item, pixel of the 4 x 4 grid) rows, K = (tap, channel) with the channels in 8-blocks, N = c1.  Channel d of every
// staged row is the constant 1 that carries conv_in's bias through ConvT1: a tap outside the grid reads the zero row, whose
// constant channel is 0 too, so the border sees the bias through exactly the taps it has.  Channels d+1 .. dp-1 are zero.
// A row is a latent grid's position (z, NCHW) or a table row (table[codes[item][pixel]]): the same staged values, hence
// the same logits.  w1p: [parity][tap][dp / 4][c1][4]; out [item][8 x 8 pixel][c1] = relu(scale1 * acc + shift1).
// MASKS (the point pass of the grid VJP, section 29): the sign bits of pre1 go to mask1 [item][8 x 8 pixel][c1 / 32] as well, and
// item i of a z pass is grid (index ? index[base + i] : base + i).  The image decode runs MASKS = false, index null.
template <int C1, bool MASKS = false>
__global__ __launch_bounds__(512) void sd_front_kernel(const float *__restrict__ z, const float *__restrict__ table,
                                                       const int32_t *__restrict__ codes, int64_t base, int64_t n_items, int d,
                                                       int dp, const float *__restrict__ w1p, const float *__restrict__ sc1,
                                                       const float *__restrict__ sh1, float *__restrict__ out,
                                                       const int32_t *__restrict__ index = nullptr,
                                                       uint32_t *__restrict__ mask1 = nullptr) {
    constexpr int TN = C1 / 32, WPN = 8 / TN, MT = TN, P = 16, ZR = MID_ROWS;
    __shared__ __attribute__((aligned(16))) float lds[(MID_ROWS + 1) * (SD_MAX_DP + 4)];
    const int LD = dp + 4;
    const int64_t item0 = (int64_t)blockIdx.x * SD_ITEMS;
    const int tid = threadIdx.x;
    const int live = (int)(n_items - item0 < SD_ITEMS ? n_items - item0 : SD_ITEMS);
    for (int q = tid; q < (MID_ROWS + 1) * LD; q += 512) {              // the constant channel, the padding, the zero row
        const int r = q / LD, k = q - r * LD;
        if (k >= d || r >= live * P) lds[q] = (k == d && r < live * P) ? 1.f : 0.f;
    }
    if (z) {
        for (int q = tid; q < live * d * P; q += 512) {                 // [item][d][pixel]
            const int g = q / (d * P), e = q - g * d * P, k = e / P, pix = e % P;
            const int64_t row = MASKS && index ? (int64_t)index[base + item0 + g] : base + item0 + g;
            lds[(size_t)(g * P + pix) * LD + k] = z[(size_t)row * d * P + e];
        }
    } else {
        for (int q = tid; q < live * P * d; q += 512) {
            const int r = q / d, k = q - r * d;
            lds[(size_t)r * LD + k] = table[(size_t)codes[(size_t)(base + item0) * P + r] * d + k];
        }
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int nt = wave % TN, m0 = wave / TN;
    const int co = nt * 32 + j;
    const float scale = sc1[co], shift = sh1[co];
    for (int par = 0; par < 4; ++par) {
        const int py = par >> 1, px = par & 1;
        f32x16 acc[MT];
        mfma_conv::clear(acc);
        for (int tap = 0; tap < 4; ++tap) {
            const int a = tap >> 1, b = tap & 1;
            const float *ap[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int r = (m0 + m * WPN) * 32 + j;                  // < MID_ROWS: 8 M tiles of 32 rows
                const int iy = ((r >> 2) & 3) + py - a, ix = (r & 3) + px - b;
                const bool ok = iy >= 0 && iy < 4 && ix >= 0 && ix < 4;
                ap[m] = lds + (size_t)(ok ? (r & ~15) + iy * 4 + ix : ZR) * LD + 4 * h;
            }
            const float4 *wp = reinterpret_cast<const float4 *>(w1p) + ((size_t)(par * 4 + tap) * (dp / 4) + h) * C1 + co;
            for (int cb = 0; cb < dp / 8; ++cb) mfma_conv::k_block<MT>(acc, ap, cb, wp[(size_t)cb * 2 * C1]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = mfma_conv::acc_row(q, h, (m0 + m * WPN) * 32);
                const int g = r >> 4, y = (r >> 2) & 3, x = r & 3;
                const int opix = (2 * y + py) * 8 + 2 * x + px;
                const float x1 = fmaf(scale, acc[m][q], shift);
                if (MASKS) {
                    const unsigned long long bits = __ballot(x1 > 0.f);    // low half: the h = 0 row, high half: the h = 1 row
                    if (g < live && j == 0)
                        mask1[(size_t)(item0 + g) * (2 * C1) + (size_t)opix * TN + nt] = (uint32_t)(h ? bits >> 32 : bits);
                }
                if (g < live) out[(size_t)(item0 + g) * (64 * C1) + (size_t)opix * C1 + co] = x1 > 0.f ? x1 : 0.f;
            }
        }
    }
}

// The primal ConvT2 of `count` items (no masks) and the image-writing ConvT3, shared by the two decoders.
int decode_tail(int c1, int c2, int co, int s1, int crop, const float *w2p, const float *sc2, const float *sh2, const float *w3p,
                const float *b3, const float *buf1, float *buf2, int64_t count, float *logits, hipStream_t st) {
    const int G = MID_ROWS / (s1 * s1);
    const unsigned grid = (unsigned)((count + G - 1) / G);
    const Ends none{nullptr, nullptr, nullptr, nullptr, 0, 0};
    if (c1 == 128)
        vj_mid_kernel<128, 64, false, false><<<grid, 512, 0, st>>>(buf1, buf2, nullptr, nullptr, none, 0, 0, count, s1, G, w2p, sc2, sh2);
    else
        vj_mid_kernel<64, 32, false, false><<<grid, 512, 0, st>>>(buf1, buf2, nullptr, nullptr, none, 0, 0, count, s1, G, w2p, sc2, sh2);
    GEO_LAUNCH_CHECK();
#define VJ_IMAGE(C2_, CO_) vj_image_kernel<C2_, CO_><<<(unsigned)count, 256, 0, st>>>(buf2, logits, 2 * s1, crop, w3p, b3)
    if (c2 == 64 && co == 1) VJ_IMAGE(64, 1);
    else if (c2 == 64) VJ_IMAGE(64, 3);
    else if (co == 1) VJ_IMAGE(32, 1);
    else VJ_IMAGE(32, 3);
#undef VJ_IMAGE
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

struct SpatialShape {
    int d, dp, c1, c2, co, So, crop;
    size_t per_item[2];        // floats per item of the two activation buffers
};

bool make_spatial_shape(const geo_spatial_image_decoder_desc *dc, SpatialShape *s) {
    if (!dc) return false;
    if (dc->latent_dim < 1 || dc->latent_dim > SD_MAX_D) return false;
    if (!((dc->c1 == 128 && dc->c2 == 64) || (dc->c1 == 64 && dc->c2 == 32))) return false;
    if (dc->out_channels != 1 && dc->out_channels != 3) return false;
    if (dc->out_size != 28 && dc->out_size != 32) return false;
    s->d = dc->latent_dim;
    s->dp = (s->d + 1 + 7) & ~7;
    s->c1 = dc->c1;
    s->c2 = dc->c2;
    s->co = dc->out_channels;
    s->So = dc->out_size;
    s->crop = (32 - s->So) / 2;
    s->per_item[0] = (size_t)64 * s->c1;
    s->per_item[1] = (size_t)256 * s->c2;
    return true;
}

// ================================ vector-Jacobian product ================================
// out[i] = J(z_i)^T u_i, J = d sigmoid(decoder(z)) / dz: the point pass above for the two masks and sigmoid', then the three
// layers backwards.  A transposed convolution's adjoint is the convolution with the same kernel: input pixel (iy, ix) collects
// output pixels (2 iy - 1 + ky, 2 ix - 1 + kx), ky, kx = 0 .. 3, nothing outside the image.
//
//   vv_back_kernel    u3 = sigmoid' * u ([C][S][S]) -> u2 [s2 s2][c2] = mask2 * scale2 * conv(u3, w3)        VALU, K = 16 C
//   vv_mid_kernel     u2 -> u1 [s1 s1][c1] = mask1 * conv(u2, w2)                                             MFMA, K = 16 c2
//   vv_final_kernel   part[row y][i][k] = sum over the pixels of row y and the channels of At[k][n] u1[i][n]   MFMA, K = s1 c1
//   vv_sum_kernel     out[i][k] = sum over y of part[y][i][k]                                                  fp64
//
// Fixed orders: u2 is one fmaf chain from 0 over (ky, kx, c) ascending; u1 is the K-quad chain over tap 4 ky + kx and the c2
// channels; a pixel's share of out is the K-quad chain over its c1 channels in f32, the pixels of a row are added in fp64 in
// ascending order, then the rows in ascending order.  No atomics; every value belongs to one item.
constexpr int64_t VJP_ITEMS_PER_PASS = 1024;
constexpr int VV_MID_ITEMS = 2;                 // items of one vv_mid workgroup: 2 x 256 input rows in LDS, 4 M tiles of outputs

struct VjpWorkspace { Workspace pt; double *part; };
VjpWorkspace lay_out_vjp(geo::Arena &ar, const Shape &s, int64_t pb) {
    VjpWorkspace w;
    ar.take(w.pt.mask1, (size_t)pb * (s.n1 / 32)); ar.take(w.pt.mask2, (size_t)pb * (s.n2 / 32));
    ar.take(w.pt.sigp, (size_t)pb * s.nout);
    ar.take(w.pt.buf1, (size_t)pb * s.n1); ar.take(w.pt.buf2, (size_t)pb * s.n2);
    ar.take(w.part, (size_t)s.s1 * pb * ((s.d + 31) & ~31));
    return w;
}
size_t vjp_layout_bytes(const Shape &s, int64_t pb) { return geo::measure(lay_out_vjp, s, pb); }

// w3t: [tap 4 ky + kx][C][c2].  A thread owns one channel ci of c2 and keeps its 16 C weights in registers; u3 sits in LDS
// with a border of one zero pixel, so no tap tests a bound.  One item per workgroup.  u [.][C][So][So], So = S - 2 crop, is the
// window of rows and columns crop .. S - crop - 1 of the output (zero outside it); row i of the pass is u + (row0 + i) u_stride
// (u_stride = 0: one row for every item).
template <int C2, int CO>
__global__ __launch_bounds__(256) void vv_back_kernel(const float *__restrict__ u, const float *__restrict__ sigp,
                                                      const uint32_t *__restrict__ mask2, float *__restrict__ out, int64_t row0,
                                                      int s2, const float *__restrict__ w3t, const float *__restrict__ sc2,
                                                      int crop, int64_t u_stride) {
    constexpr int NPG = 256 / C2, TN = C2 / 32;
    __shared__ float us[CO * 34 * 34];
    const int S = 2 * s2, SP = S + 2, P2 = s2 * s2, n2 = P2 * C2, nout = CO * S * S;
    const int tid = threadIdx.x;
    const int64_t it = blockIdx.x;
    const int So = S - 2 * crop;
    const float *ui = u + (size_t)(row0 + it) * u_stride, *sg = sigp + (size_t)it * nout;
    for (int q = tid; q < CO * SP * SP; q += 256) {
        const int c = q / (SP * SP), rem = q - c * SP * SP, py = rem / SP, px = rem - py * SP;
        const bool in = py >= 1 + crop && py <= S - crop && px >= 1 + crop && px <= S - crop;
        us[q] = in ? sg[(c * S + py - 1) * S + px - 1] * ui[(c * So + py - 1 - crop) * So + px - 1 - crop] : 0.f;
    }
    const int ci = tid % C2, pg = tid / C2;
    float w[16 * CO];
#pragma unroll
    for (int t = 0; t < 16 * CO; ++t) w[t] = w3t[(size_t)t * C2 + ci];
    const float scale = sc2[ci];
    __syncthreads();
    for (int pix = pg; pix < P2; pix += NPG) {
        const int y = pix / s2, x = pix - y * s2;
        float acc = 0.f;
#pragma unroll
        for (int tap = 0; tap < 16; ++tap)
#pragma unroll
            for (int c = 0; c < CO; ++c)
                acc = fmaf(us[(c * SP + 2 * y + (tap >> 2)) * SP + 2 * x + (tap & 3)], w[tap * CO + c], acc);
        const uint32_t bits = mask2[(size_t)it * (n2 / 32) + (size_t)pix * TN + (ci >> 5)];
        out[(size_t)it * n2 + (size_t)pix * C2 + ci] = (bits >> (ci & 31)) & 1u ? scale * acc : 0.f;
    }
}

// w2t: [tap 4 ky + kx][c2 / 4][c1][4], element (tap, q, ci, r) = w2[ci][4 q + r][ky][kx].  M = (item, pixel of s1 x s1) rows, the
// items' u2 ([pixel of s2 x s2][c2]) staged in mfma_conv.h's layout; 8 waves: wave = (N tile, M tiles sharing the B read).
template <int C1, int C2>
__global__ __launch_bounds__(512) void vv_mid_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                     const uint32_t *__restrict__ mask1, int64_t n_items, int s1,
                                                     const float *__restrict__ w2t) {
    constexpr int LD = C2 + 4, TN = C1 / 32, WPN = 8 / TN, MT = 4 / WPN, G = VV_MID_ITEMS;
    __shared__ __attribute__((aligned(16))) float lds[(G * 256 + 1) * LD];
    const int P = s1 * s1, s2 = 2 * s1, P2 = 4 * P, n1 = P * C1, n2 = P2 * C2;
    const int rows = G * P, ZR = G * P2;
    const int64_t item0 = (int64_t)blockIdx.x * G;
    const int tid = threadIdx.x;
    for (int g = 0; g < G; ++g)
        if (item0 + g < n_items) mfma_conv::stage_rows<C2, 512>(lds + (size_t)g * P2 * LD, in + (size_t)(item0 + g) * n2, P2, tid);
    mfma_conv::fill_zero_row<512>(lds, ZR, LD, tid);
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int nt = wave % TN, m0 = wave / TN;
    int rg[MT], ry[MT], rx[MT];
    bool rv[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int r = (m0 + m * WPN) * 32 + j;
        const int g = r < rows ? r / P : 0;
        rv[m] = r < rows && item0 + g < n_items;
        rg[m] = g;
        const int pq = r < rows ? r - g * P : 0;
        ry[m] = pq / s1;
        rx[m] = pq - ry[m] * s1;
    }
    const int ci = nt * 32 + j;
    mfma_conv::f32x16 acc[MT];
    mfma_conv::clear(acc);
    for (int tap = 0; tap < 16; ++tap) {
        const int ky = tap >> 2, kx = tap & 3;
        const float *ap[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            ap[m] = mfma_conv::tap_row(lds, LD, ZR, rv[m], rg[m], 2 * ry[m] - 1 + ky, 2 * rx[m] - 1 + kx, s2, P2, h);
        const float4 *wp = reinterpret_cast<const float4 *>(w2t) + ((size_t)tap * (C2 / 4) + h) * C1 + ci;
        mfma_conv::k_chain<MT, 4>(acc, ap, wp, C2 / 8, C1);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = mfma_conv::acc_row(q, h, (m0 + m * WPN) * 32);
            const int g = r < rows ? r / P : 0;
            const int64_t it = item0 + g;
            if (r < rows && it < n_items) {
                const int pix = r - g * P;
                const uint32_t bits = mask1[(size_t)it * (n1 / 32) + (size_t)pix * TN + nt];
                out[(size_t)it * n1 + (size_t)pix * C1 + ci] = (bits >> j) & 1u ? acc[m][q] : 0.f;
            }
        }
    }
}

// Atq: [n1 / 4][dn][4], dn = d rounded up to a multiple of 32, element (q, k, r) = At[k][4 q + r], 0 for k >= d.  A workgroup is
// 32 items x one pixel row of the s1 x s1 grid, a wave one tile of 32 latent dimensions; A straight from global memory (a lane
// reads 16 consecutive bytes of its own item).  A row past `cnt` reads the last item's and is not written.
__global__ __launch_bounds__(256) void vv_final_kernel(const float *__restrict__ u1, int cnt, int n1, int c1, int s1, int dn,
                                                       const float *__restrict__ Atq, double *__restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int tile0 = blockIdx.x * 32, y = blockIdx.y;
    const int row = tile0 + j < cnt ? tile0 + j : cnt - 1;
    const int col = wave * 32 + j;
    const float *ar = u1 + (size_t)row * n1 + 4 * h;
    const float4 *bq = reinterpret_cast<const float4 *>(Atq) + (size_t)h * dn + col;
    double sum[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) sum[q] = 0.0;
    for (int x = 0; x < s1; ++x) {
        const int k0 = (y * s1 + x) * c1;
        mfma_conv::f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        for (int cb = 0; cb < c1 / 8; ++cb) {
            const float4 av = *reinterpret_cast<const float4 *>(ar + k0 + cb * 8);
            const float4 bv = bq[(size_t)(k0 / 4 + 2 * cb) * dn];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) sum[q] += (double)acc[q];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int r = tile0 + mfma_conv::acc_row(q, h);
        if (r < cnt) part[((size_t)y * cnt + r) * dn + col] = sum[q];
    }
}

// F = 0: out = the sum.  F >= 2 (the items are curves of F frames): out = twice the sum at an interior frame, 0 at the ends.
__global__ __launch_bounds__(256) void vv_sum_kernel(const double *__restrict__ part, int cnt, int d, int dn, int s1, int F,
                                                     double *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)cnt * d) return;
    const int i = (int)(q / d), k = (int)(q - (int64_t)i * d);
    double s = 0.0;
    for (int y = 0; y < s1; ++y) s += part[((size_t)y * cnt + i) * dn + k];
    if (F) {
        const int f = i % F;
        s = f > 0 && f < F - 1 ? 2.0 * s : 0.0;
    }
    out[q] = s;
}

// u f32 [.][nout] rows row0 .. row0 + cnt of the call -> out f64 [cnt][d], with the masks and sigmoid' of slots 0 .. cnt - 1.
int run_vjp_tail(const geo_vanilla_decoder_desc *dc, const Shape &sh, const VjpWorkspace &w, const float *u, int64_t row0,
                 int64_t cnt, double *out, hipStream_t st, int F = 0) {
#define VV_BACK(C2_, CO_)                                                                                                     \
    vv_back_kernel<C2_, CO_><<<(unsigned)cnt, 256, 0, st>>>(u, w.pt.sigp, w.pt.mask2, w.pt.buf2, row0, sh.s2, dc->w3t, dc->scale2, \
                                                            0, (int64_t)sh.nout)
    if (sh.c2 == 64 && sh.co == 1) VV_BACK(64, 1);
    else if (sh.c2 == 64) VV_BACK(64, 3);
    else if (sh.co == 1) VV_BACK(32, 1);
    else VV_BACK(32, 3);
#undef VV_BACK
    GEO_LAUNCH_CHECK();
    const unsigned mid_grid = (unsigned)((cnt + VV_MID_ITEMS - 1) / VV_MID_ITEMS);
    if (sh.c1 == 128) vv_mid_kernel<128, 64><<<mid_grid, 512, 0, st>>>(w.pt.buf2, w.pt.buf1, w.pt.mask1, cnt, sh.s1, dc->w2t);
    else vv_mid_kernel<64, 32><<<mid_grid, 512, 0, st>>>(w.pt.buf2, w.pt.buf1, w.pt.mask1, cnt, sh.s1, dc->w2t);
    GEO_LAUNCH_CHECK();
    const int dn = (sh.d + 31) & ~31;
    const dim3 grid((unsigned)((cnt + 31) / 32), (unsigned)sh.s1);
    vv_final_kernel<<<grid, 2 * dn, 0, st>>>(w.pt.buf1, (int)cnt, sh.n1, sh.c1, sh.s1, dn, dc->Atq, w.part);
    GEO_LAUNCH_CHECK();
    vv_sum_kernel<<<(unsigned)((cnt * sh.d + 255) / 256), 256, 0, st>>>(w.part, (int)cnt, sh.d, dn, sh.s1, F, out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// ================================ curve energy and relaxation ================================
// geo_vanilla_curve_energy / geo_vanilla_curve_relax: section 26's definitions and loop (curve_step.h) over this decoder.  C curves
// of F frames are C F latents, curve after curve; a slice is whole curves, as many as the workspace holds.  Evaluate(z):
//   point pass with G_OUT          masks, sigmoid' and g [frame][nout]
//   vc_residual_kernel             per frame: seg_sq[f] = |g[f+1] - g[f]|^2 and r[f] = (g[f] - g[f-1]) - (g[f+1] - g[f]) in fp64,
//                                  r rounded once to f32 (0 at the ends)
//   vc_energy_kernel               per curve: E = sum of seg_sq ascending; NaN for a curve with a NaN or an inf
//   the VJP tail with F            grad[f] = 2 J(x[f])^T r[f], 0 at the ends
// The order of a segment's sum depends on nout alone: thread t of 256 adds the squares of outputs t, t + 256, t + 512, ... in
// ascending order into one fp64 accumulator (from 0, product and sum separate operations), then the 256 partial sums are folded
// p[t] += p[t + s] for s = 128, 64, ..., 1.
// The trace tr J^T J of a frame is the sum over k ascending, in fp64, of |J e_k|^2 in f32: unit tangent e_k enters the tangent
// kernels as row k of At (what vj_front_kernel<true> makes of e_k, exactly), an "edge" is (pair of frames, k), its two ends the
// two frames, and the back kernel with SQ writes each end's sum of squares.
constexpr int64_t CURVE_SLICE_ITEMS = 4096;      // at most this many frames per slice
constexpr int TRACE_EDGES = 512;                 // about this many (pair of frames, k) per trace pass

struct CurveWorkspace {
    CurveState st;
    VjpWorkspace v;
    float *g, *r, *sq;
    int32_t *ia, *ib;
    int64_t trace_pairs;        // pairs of frames per trace pass
};

int64_t trace_pairs_for(const Shape &s, int64_t n) {
    const int64_t pairs = (n + 1) / 2, fit = TRACE_EDGES / s.d < 1 ? 1 : TRACE_EDGES / s.d;
    return pairs < fit ? pairs : fit;
}

CurveWorkspace lay_out_curve_slice(geo::Arena &ar, const Shape &s, int64_t n_curves, int F) {
    CurveWorkspace w;
    const int64_t n = n_curves * F;
    w.trace_pairs = trace_pairs_for(s, n);
    const int64_t eb = w.trace_pairs * s.d;                   // the trace pass: eb tangent rows, 2 eb items
    lay_out_curves(ar, &w.st, n_curves, F, s.d);
    ar.take(w.v.pt.mask1, (size_t)n * (s.n1 / 32)); ar.take(w.v.pt.mask2, (size_t)n * (s.n2 / 32));
    ar.take(w.v.pt.sigp, (size_t)n * s.nout);
    ar.take(w.v.pt.buf1, (size_t)(n > eb ? n : eb) * s.n1); ar.take(w.v.pt.buf2, (size_t)(n > 2 * eb ? n : 2 * eb) * s.n2);
    ar.take(w.v.part, (size_t)s.s1 * n * ((s.d + 31) & ~31));
    ar.take(w.g, (size_t)n * s.nout); ar.take(w.r, (size_t)n * s.nout);
    ar.take(w.sq, (size_t)2 * eb); ar.take(w.ia, (size_t)eb); ar.take(w.ib, (size_t)eb);
    return w;
}
size_t curve_slice_bytes(const Shape &s, int64_t n_curves, int F) { return geo::measure(lay_out_curve_slice, s, n_curves, F); }

int64_t curve_slice_cap(int64_t C, int F) {
    const int64_t cap = CURVE_SLICE_ITEMS / F;
    return C < 1 ? 1 : (C < cap ? C : cap);
}

// one workgroup per frame p = c F + f of the slice
__global__ __launch_bounds__(256) void vc_residual_kernel(const float *__restrict__ g, int F, int nout, double *__restrict__ seg_sq,
                                                          float *__restrict__ r) {
#pragma clang fp contract(off)      // plain operators below: the pragma governs them
    __shared__ double part_s[256];
    const int64_t p = blockIdx.x, c = p / F;
    const int f = (int)(p - c * F), tid = threadIdx.x;
    const bool interior = f > 0 && f < F - 1;
    const float *g0 = g + (size_t)p * nout, *gm = f > 0 ? g0 - nout : g0, *gp = f < F - 1 ? g0 + nout : g0;
    float *rp = r + (size_t)p * nout;
    double part = 0.0;
    for (int o = tid; o < nout; o += 256) {
        const double ahead = (double)gp[o] - (double)g0[o];
        part += ahead * ahead;
        rp[o] = interior ? (float)(((double)g0[o] - (double)gm[o]) - ahead) : 0.f;
    }
    part_s[tid] = part;
    for (int s = 128; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s) part_s[tid] += part_s[tid + s];
    }
    if (tid == 0 && f < F - 1) seg_sq[(size_t)c * (F - 1) + f] = part_s[0];
}

// one wave per curve
__global__ __launch_bounds__(64) void vc_energy_kernel(const double *__restrict__ seg_sq, const float *__restrict__ x, int F, int d,
                                                       double *__restrict__ energy) {
#pragma clang fp contract(off)
    const int64_t c = blockIdx.x;
    bool bad = false;
    for (int i = threadIdx.x; i < F * d; i += 64)
        bad |= (__float_as_uint(x[(size_t)c * F * d + i]) & 0x7f800000u) == 0x7f800000u;
    const bool any_bad = __ballot(bad) != 0ull;
    if (threadIdx.x == 0) {
        double e = 0.0;
        for (int f = 0; f < F - 1; ++f) e += seg_sq[(size_t)c * (F - 1) + f];
        energy[c] = any_bad ? (double)NAN : e;
    }
}

// the tangent rows and slots of a trace pass: row l = (pair q, k) is At[k], its two ends frames p0 + 2 q and p0 + 2 q + 1 (the
// last frame again where the slice ends on an odd count; that end's result is not read)
__global__ __launch_bounds__(256) void vc_unit_kernel(const float *__restrict__ At, int d, int n1, int64_t p0, int64_t n,
                                                      float *__restrict__ rows, int32_t *__restrict__ ia, int32_t *__restrict__ ib) {
    const int64_t l = blockIdx.x, q = l / d;
    const int k = (int)(l - q * d);
    const float4 *src = reinterpret_cast<const float4 *>(At + (size_t)k * n1);
    float4 *dst = reinterpret_cast<float4 *>(rows + (size_t)l * n1);
    for (int i = threadIdx.x; i < n1 / 4; i += 256) dst[i] = src[i];
    if (threadIdx.x == 0) {
        const int64_t a = p0 + 2 * q, b = a + 1 < n ? a + 1 : n - 1;
        ia[l] = (int32_t)a;
        ib[l] = (int32_t)b;
    }
}

// tr[p0 + j] = sum over k ascending of (double)sq[2 ((j / 2) d + k) + (j & 1)], one thread per frame of the pass
__global__ __launch_bounds__(256) void vc_trace_kernel(const float *__restrict__ sq, int d, int64_t p0, int64_t frames,
                                                       double *__restrict__ tr) {
#pragma clang fp contract(off)
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= frames) return;
    double t = 0.0;
    for (int k = 0; k < d; ++k) t += (double)sq[2 * ((j >> 1) * d + k) + (j & 1)];
    tr[p0 + j] = t;
}

// Evaluate(z) over a slice of n_curves: energy [n_curves], seg_sq [n_curves][F-1], grad [n_curves][F][d]; g (the slice's own
// buffer or the caller's) [n][nout]; tr [n] or null (the masks and sigmoid' it reads are this evaluation's)
int curve_evaluate(const geo_vanilla_decoder_desc *dc, const Shape &sh, const CurveWorkspace &w, const float *z, int64_t n_curves,
                   int F, double *energy, double *seg_sq, double *grad, float *g, double *tr, hipStream_t st) {
    const int64_t n = n_curves * F;
    const Ends e{z, z, nullptr, nullptr, 0, (int)n};
    int rc = run_point_pass(dc, sh, w.v.pt, e, n, 0, st, g);
    if (rc != GEO_OK) return rc;
    vc_residual_kernel<<<(unsigned)n, 256, 0, st>>>(g, F, sh.nout, seg_sq, w.r);
    GEO_LAUNCH_CHECK();
    vc_energy_kernel<<<(unsigned)n_curves, 64, 0, st>>>(seg_sq, z, F, sh.d, energy);
    GEO_LAUNCH_CHECK();
    if (tr) {
        for (int64_t p0 = 0; p0 < n; p0 += 2 * w.trace_pairs) {
            const int64_t frames = n - p0 < 2 * w.trace_pairs ? n - p0 : 2 * w.trace_pairs;
            const int64_t ne = (frames + 1) / 2 * sh.d;
            vc_unit_kernel<<<(unsigned)ne, 256, 0, st>>>(dc->At, sh.d, sh.n1, p0, n, w.v.pt.buf1, w.ia, w.ib);
            GEO_LAUNCH_CHECK();
            const Ends t{z, z, w.ia, w.ib, 0, (int)ne};
            rc = run_mid<true>(sh, dc, w.v.pt.buf1, w.v.pt.buf2, w.v.pt.mask1, w.v.pt.mask2, t, 1, 0, 2 * ne, st);
            if (rc != GEO_OK) return rc;
            rc = run_back<true, true>(sh, dc, w.v.pt.buf2, w.v.pt.sigp, t, 1, 0, ne, w.sq, st);
            if (rc != GEO_OK) return rc;
            vc_trace_kernel<<<(unsigned)((frames + 255) / 256), 256, 0, st>>>(w.sq, sh.d, p0, frames, tr);
            GEO_LAUNCH_CHECK();
        }
    }
    return run_vjp_tail(dc, sh, w.v, w.r, 0, n, grad, st, F);
}

int curve_check(const char *who, const geo_vanilla_decoder_desc *dc, Shape *sh, int64_t C, int F) {
    int rc = check_desc(dc, sh, who);
    if (rc != GEO_OK) return rc;
    GEO_REQUIRE(dc->w2t && dc->w3t && dc->Atq, "%s: null transposed pack in the descriptor", who);
    GEO_REQUIRE(F >= 2 && F <= CURVE_MAX_F, "%s: F %d not in [2,%d]", who, F, CURVE_MAX_F);
    GEO_REQUIRE(C >= 0, "%s: C %lld < 0", who, (long long)C);
    return GEO_OK;
}

// the curves per slice a workspace holds: everything (up to the cap) when it fits, else the largest count that does;
// bytes(n_curves) measures a slice's layout
template <typename Bytes>
int curve_slice_length(const char *who, Bytes bytes, int64_t C, int F, size_t ws_bytes, int64_t *slice) {
    const int64_t cap = curve_slice_cap(C, F);
    *slice = cap;
    if (ws_bytes >= bytes(cap)) return GEO_OK;
    const size_t min_bytes = bytes(1);
    if (ws_bytes < min_bytes) {
        geo::set_error("%s: workspace of %zu bytes is below the minimum of %zu", who, ws_bytes, min_bytes);
        return GEO_E_WORKSPACE;
    }
    int64_t lo = 1, hi = cap;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (bytes(mid) <= ws_bytes) lo = mid; else hi = mid - 1;
    }
    *slice = lo;
    return GEO_OK;
}

int curve_energy(const geo_vanilla_decoder_desc *dc, const float *x, int64_t C, int F, double *energy_out, double *seg_sq_out,
                 double *grad_out, float *g_out, double *trace_out, void *ws, size_t ws_bytes, hipStream_t st) {
    static const char who[] = "geo_vanilla_curve_energy";
    Shape sh;
    if (const int rc = curve_check(who, dc, &sh, C, F)) return rc;
    if (C == 0) return GEO_OK;
    GEO_REQUIRE(x && energy_out && ws, "%s: null pointer", who);
    int64_t slice = 0;
    if (const int rc = curve_slice_length(who, [&](int64_t nc) { return curve_slice_bytes(sh, nc, F); }, C, F, ws_bytes, &slice)) return rc;
    for (int64_t base = 0; base < C; base += slice) {
        const int64_t nc = C - base < slice ? C - base : slice;
        geo::Arena ar(ws, ws_bytes);
        const CurveWorkspace w = lay_out_curve_slice(ar, sh, nc, F);
        GEO_REQUIRE_WORKSPACE("geo_vanilla_curve_energy", ar, curve_slice_bytes(sh, nc, F));
        const size_t at = (size_t)base * F;
        if (const int rc = curve_evaluate(dc, sh, w, x + at * sh.d, nc, F, energy_out + base,
                                          seg_sq_out ? seg_sq_out + (size_t)base * (F - 1) : w.st.seg_ev,
                                          grad_out ? grad_out + at * sh.d : w.st.grad_ev, g_out ? g_out + at * sh.nout : w.g,
                                          trace_out ? trace_out + at : nullptr, st))
            return rc;
    }
    return GEO_OK;
}

int curve_relax(const geo_vanilla_decoder_desc *dc, float *x, int64_t C, int F, int n_iters, double *step, double *energy0_out,
                double *energy_out, double *seg_sq_out, int32_t *accepted_out, void *ws, size_t ws_bytes, hipStream_t st) {
    static const char who[] = "geo_vanilla_curve_relax";
    Shape sh;
    if (const int rc = curve_check(who, dc, &sh, C, F)) return rc;
    GEO_REQUIRE(n_iters >= 0, "%s: n_iters %d < 0", who, n_iters);
    if (C == 0) return GEO_OK;
    GEO_REQUIRE(x && step && energy_out && accepted_out && ws, "%s: null pointer", who);
    int64_t slice = 0;
    if (const int rc = curve_slice_length(who, [&](int64_t nc) { return curve_slice_bytes(sh, nc, F); }, C, F, ws_bytes, &slice)) return rc;
    // the trace costs d tangents per frame: only for a slice with a curve whose step the caller left to the call (one copy of the
    // steps to the host, before the first launch; nothing is read back per iteration)
    std::vector<double> step_h((size_t)C);
    GEO_HIP_CHECK(hipMemcpyAsync(step_h.data(), step, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, st));
    GEO_HIP_CHECK(hipStreamSynchronize(st));
    const int iters = F == 2 ? 0 : n_iters;                       // no interior frame: nothing can move
    for (int64_t base = 0; base < C; base += slice) {
        const int64_t nc = C - base < slice ? C - base : slice;
        geo::Arena ar(ws, ws_bytes);
        const CurveWorkspace w = lay_out_curve_slice(ar, sh, nc, F);
        GEO_REQUIRE_WORKSPACE("geo_vanilla_curve_relax", ar, curve_slice_bytes(sh, nc, F));
        bool need_trace = false;
        for (int64_t c = base; c < base + nc; ++c) need_trace |= step_h[(size_t)c] < 0.0;
        const CurveState &cs = w.st;
        float *xs = x + (size_t)base * F * sh.d;
        double *seg_s = seg_sq_out ? seg_sq_out + (size_t)base * (F - 1) : nullptr;
        for (int it = -1; it < iters; ++it) {                     // it = -1: the curve itself
            if (const int rc = curve_evaluate(dc, sh, w, it < 0 ? xs : cs.y, nc, F, cs.e_ev, cs.seg_ev, cs.grad_ev, w.g,
                                              it < 0 && need_trace ? cs.tr : nullptr, st))
                return rc;
            curve_step_kernel<<<(unsigned)nc, CURVE_THREADS, 0, st>>>(cs, xs, F, sh.d, it < 0, it == iters - 1, step + base,
                                                                      energy0_out ? energy0_out + base : nullptr, energy_out + base,
                                                                      seg_s, accepted_out + base);
            GEO_LAUNCH_CHECK();
        }
    }
    return GEO_OK;
}

// ================================ the spatial decoder on whole grids: VJP and curves ================================
// geo_spatial_vjp, geo_spatial_curve_energy, geo_spatial_curve_relax: section 27 for the decoder of geo_spatial_decode.  A point is a
// 4 x 4 grid of d-vectors (16 d coordinates, NCHW), its image the whole S x S output.  From the 8 x 8 stage on this is the 32-px
// vanilla geometry, so the point pass and the walk backwards are the kernels above at s1 = 8; the first stage is its own:
//   sd_front_kernel<.., true>      conv_in . ConvT1 -> mask1 bits, relu(pre1) [8 x 8][c1]
//   vj_mid_kernel, vj_back_kernel  as in the vanilla point pass; at 28 px g is the window 2 .. 29 of the 32-px output
//   vv_back_kernel (crop)          u lives on the window and is zero outside it
//   vv_mid_kernel                  as it is
//   sv_final_kernel                out[i][k][y][x] = sum over (ky, kx) of the K-quad chain over c1 of u1[(2y-1+ky, 2x-1+kx)][co] w1t
// Fixed orders beyond section 27's: a pixel's c1 channels are one f32 K-quad chain from 0; the up to 16 pixels of a grid position
// are added in fp64 in ascending (ky, kx) order (a pixel outside the 8 x 8 image adds 0).  No atomics; every value belongs to one
// item.  The first step of a relaxation is the sign probe below instead of the trace.
constexpr int SV_ITEMS = 4;                      // grids of one sv_final workgroup: two M tiles of 32 (grid, position) rows

struct GridShape {
    SpatialShape sp;
    Shape sh;                                    // the tail at s1 = 8: n1 = 64 c1, n2 = 256 c2, nout = C 32 32 (sigmoid' is kept whole)
    geo_vanilla_decoder_desc tail;               // what run_mid / run_back read: the second and third layer's packs
    int dn, dz, nout;                            // d rounded up to 32; 16 d; C So So
};

bool make_grid_shape(const geo_spatial_image_decoder_desc *dc, GridShape *g) {
    if (!make_spatial_shape(dc, &g->sp)) return false;
    g->tail = geo_vanilla_decoder_desc{dc->latent_dim, dc->c1, dc->c2, dc->out_channels, 32, nullptr, nullptr, dc->w2p, dc->scale2,
                                       dc->shift2, dc->w3p, dc->b3, dc->w2t, dc->w3t, nullptr};
    if (!make_shape(&g->tail, &g->sh)) return false;
    g->dn = (g->sp.d + 31) & ~31;
    g->dz = 16 * g->sp.d;
    g->nout = g->sp.co * g->sp.So * g->sp.So;
    return true;
}

int check_grid_desc(const geo_spatial_image_decoder_desc *dc, GridShape *g, const char *who) {
    GEO_REQUIRE(make_grid_shape(dc, g), "%s: decoder configuration not covered (see geo_hip.h)", who);
    GEO_REQUIRE(dc->w1p && dc->scale1 && dc->shift1 && dc->w2p && dc->scale2 && dc->shift2 && dc->w3p && dc->b3,
                "%s: null pointer in the descriptor", who);
    GEO_REQUIRE(dc->w1t && dc->w2t && dc->w3t, "%s: null transposed pack in the descriptor", who);
    return GEO_OK;
}

// per item of a pass: the two masks, sigmoid' (32 x 32) and the two activation buffers
Workspace lay_out_grid(geo::Arena &ar, const GridShape &g, int64_t pb) {
    Workspace w;
    ar.take(w.mask1, (size_t)pb * (g.sh.n1 / 32)); ar.take(w.mask2, (size_t)pb * (g.sh.n2 / 32));
    ar.take(w.sigp, (size_t)pb * g.sh.nout);
    ar.take(w.buf1, (size_t)pb * g.sh.n1); ar.take(w.buf2, (size_t)pb * g.sh.n2);
    return w;
}
size_t grid_layout_bytes(const GridShape &g, int64_t pb) { return geo::measure(lay_out_grid, g, pb); }

// w1t: [tap 4 ky + kx][c1 / 4][dn][4], element (tap, q, k, r) = scale1[4 q + r] W[ky][kx][k][4 q + r] (conv_in composed into ConvT1,
// the first norm's scale folded in), 0 for k >= d.  M = (grid, position) rows, N = dn, K = c1 per pixel.  A workgroup stages the u1
// ([8 x 8 pixel][c1]) of SV_ITEMS grids in mfma_conv.h's layout; wave = (M tile, N tile), a wave past dn / 32 N tiles only stages.
// F = 0: out = the sum.  F >= 2 (the grids are curves of F frames): twice the sum at an interior frame, 0 at the ends.
template <int C1>
__global__ __launch_bounds__(256) void sv_final_kernel(const float *__restrict__ u1, int64_t cnt, int d, int dn,
                                                       const float *__restrict__ w1t, int F, double *__restrict__ out) {
    constexpr int LD = C1 + 4, ZR = SV_ITEMS * 64;
    __shared__ __attribute__((aligned(16))) float lds[(SV_ITEMS * 64 + 1) * LD];
    const int tid = threadIdx.x;
    const int64_t item0 = (int64_t)blockIdx.x * SV_ITEMS;
    for (int g = 0; g < SV_ITEMS; ++g)
        if (item0 + g < cnt) mfma_conv::stage_rows<C1, 256>(lds + (size_t)g * 64 * LD, u1 + (size_t)(item0 + g) * 64 * C1, 64, tid);
    mfma_conv::fill_zero_row<256>(lds, ZR, LD, tid);
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int mt = wave & 1, nt = wave >> 1;
    if (nt * 32 >= dn) return;
    const int r = mt * 32 + j, g = r >> 4, y = (r >> 2) & 3, x = r & 3;
    const bool rv = item0 + g < cnt;
    const int col = nt * 32 + j;
    double sum[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) sum[q] = 0.0;
    for (int tap = 0; tap < 16; ++tap) {
        const int ky = tap >> 2, kx = tap & 3;
        const float *ap[1] = {mfma_conv::tap_row(lds, LD, ZR, rv, g, 2 * y - 1 + ky, 2 * x - 1 + kx, 8, 64, h)};
        mfma_conv::f32x16 acc[1];
        mfma_conv::clear(acc);
        const float4 *wp = reinterpret_cast<const float4 *>(w1t) + ((size_t)tap * (C1 / 4) + h) * dn + col;
        mfma_conv::k_chain<1, 4>(acc, ap, wp, C1 / 8, dn);
#pragma unroll
        for (int q = 0; q < 16; ++q) sum[q] += (double)acc[0][q];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ro = mfma_conv::acc_row(q, h, mt * 32);
        const int64_t it = item0 + (ro >> 4);
        if (it < cnt && col < d) {
            double s = sum[q];
            if (F) {
                const int f = (int)(it % F);
                s = f > 0 && f < F - 1 ? 2.0 * s : 0.0;
            }
            out[((size_t)it * d + col) * 16 + (ro & 15)] = s;
        }
    }
}

// The point pass over grids base .. base + cnt of z (through index, if given): masks and sigmoid' to slots 0 .. cnt - 1; g_out (may
// be null): the sigmoids [slot][nout].
int run_grid_point_pass(const geo_spatial_image_decoder_desc *dc, const GridShape &gs, const Workspace &w, const float *z,
                        const int32_t *index, int64_t base, int64_t cnt, hipStream_t st, float *g_out) {
    const unsigned grid = (unsigned)((cnt + SD_ITEMS - 1) / SD_ITEMS);
    if (gs.sp.c1 == 128)
        sd_front_kernel<128, true><<<grid, 512, 0, st>>>(z, nullptr, nullptr, base, cnt, gs.sp.d, gs.sp.dp, dc->w1p, dc->scale1,
                                                         dc->shift1, w.buf1, index, w.mask1);
    else
        sd_front_kernel<64, true><<<grid, 512, 0, st>>>(z, nullptr, nullptr, base, cnt, gs.sp.d, gs.sp.dp, dc->w1p, dc->scale1,
                                                        dc->shift1, w.buf1, index, w.mask1);
    GEO_LAUNCH_CHECK();
    const Ends none{nullptr, nullptr, nullptr, nullptr, 0, 0};
    int rc = run_mid<false>(gs.sh, &gs.tail, w.buf1, w.buf2, w.mask1, w.mask2, none, 0, 0, cnt, st);
    if (rc != GEO_OK) return rc;
    if (g_out) return run_back<false, false, true>(gs.sh, &gs.tail, w.buf2, w.sigp, none, 0, 0, cnt, nullptr, st, g_out, gs.sp.crop);
    return run_back<false>(gs.sh, &gs.tail, w.buf2, w.sigp, none, 0, 0, cnt, nullptr, st);
}

// u f32 rows u + (row0 + i) u_stride of nout values -> out f64 [cnt][d][4][4], with the masks and sigmoid' of slots 0 .. cnt - 1.
int run_grid_tail(const geo_spatial_image_decoder_desc *dc, const GridShape &gs, const Workspace &w, const float *u, int64_t row0,
                  int64_t u_stride, int64_t cnt, double *out, hipStream_t st, int F = 0) {
#define VV_BACK(C2_, CO_)                                                                                                     \
    vv_back_kernel<C2_, CO_><<<(unsigned)cnt, 256, 0, st>>>(u, w.sigp, w.mask2, w.buf2, row0, gs.sh.s2, dc->w3t, dc->scale2,     \
                                                            gs.sp.crop, u_stride)
    if (gs.sh.c2 == 64 && gs.sh.co == 1) VV_BACK(64, 1);
    else if (gs.sh.c2 == 64) VV_BACK(64, 3);
    else if (gs.sh.co == 1) VV_BACK(32, 1);
    else VV_BACK(32, 3);
#undef VV_BACK
    GEO_LAUNCH_CHECK();
    const unsigned mid_grid = (unsigned)((cnt + VV_MID_ITEMS - 1) / VV_MID_ITEMS);
    if (gs.sh.c1 == 128) vv_mid_kernel<128, 64><<<mid_grid, 512, 0, st>>>(w.buf2, w.buf1, w.mask1, cnt, gs.sh.s1, dc->w2t);
    else vv_mid_kernel<64, 32><<<mid_grid, 512, 0, st>>>(w.buf2, w.buf1, w.mask1, cnt, gs.sh.s1, dc->w2t);
    GEO_LAUNCH_CHECK();
    const unsigned fin_grid = (unsigned)((cnt + SV_ITEMS - 1) / SV_ITEMS);
    if (gs.sh.c1 == 128) sv_final_kernel<128><<<fin_grid, 256, 0, st>>>(w.buf1, cnt, gs.sp.d, gs.dn, dc->w1t, F, out);
    else sv_final_kernel<64><<<fin_grid, 256, 0, st>>>(w.buf1, cnt, gs.sp.d, gs.dn, dc->w1t, F, out);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

// ---- curves of grids: section 27's evaluation with d := 16 d.  The first step: instead of the trace (16 d tangents per frame), one
// more VJP per frame with the fixed sign probe s[c][y][x] = +1 for c + y + x even, else -1 (indices of the S x S output):
// probe[f] = sum over the 16 d coordinates, ascending, in fp64, of (J(x[f])^T s)[k]^2, a one-sample estimate of tr J J^T, not a bound.
// It lands where curve_step_kernel reads the trace, so the step rule and the loop are curve_step.h's, unchanged.
struct GridCurveWorkspace {
    CurveState st;
    Workspace pt;
    float *g, *r, *sgn;
};

GridCurveWorkspace lay_out_grid_curve_slice(geo::Arena &ar, const GridShape &gs, int64_t n_curves, int F) {
    GridCurveWorkspace w;
    const int64_t n = n_curves * F;
    lay_out_curves(ar, &w.st, n_curves, F, gs.dz);
    w.pt = lay_out_grid(ar, gs, n);
    ar.take(w.g, (size_t)n * gs.nout); ar.take(w.r, (size_t)n * gs.nout);
    ar.take(w.sgn, (size_t)gs.nout);
    return w;
}
size_t grid_curve_slice_bytes(const GridShape &gs, int64_t n_curves, int F) {
    return geo::measure(lay_out_grid_curve_slice, gs, n_curves, F);
}

__global__ __launch_bounds__(256) void sv_sign_kernel(int So, int nout, float *__restrict__ s) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= nout) return;
    const int c = o / (So * So), rem = o - c * So * So, y = rem / So, x = rem - y * So;
    s[o] = ((c + y + x) & 1) ? -1.f : 1.f;
}

// probe[p] = sum over k ascending of v[p][k]^2, one thread per frame
__global__ __launch_bounds__(256) void sv_probe_kernel(const double *__restrict__ v, int dz, int64_t n, double *__restrict__ probe) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    double t = 0.0;
    for (int k = 0; k < dz; ++k) {
        const double a = v[(size_t)p * dz + k];
        t += a * a;
    }
    probe[p] = t;
}

// Evaluate(z) over a slice of n_curves, as curve_evaluate above; probe [n] or null (through grad, which the gradient then overwrites)
int grid_curve_evaluate(const geo_spatial_image_decoder_desc *dc, const GridShape &gs, const GridCurveWorkspace &w, const float *z,
                        int64_t n_curves, int F, double *energy, double *seg_sq, double *grad, float *g, double *probe,
                        hipStream_t st) {
    const int64_t n = n_curves * F;
    int rc = run_grid_point_pass(dc, gs, w.pt, z, nullptr, 0, n, st, g);
    if (rc != GEO_OK) return rc;
    vc_residual_kernel<<<(unsigned)n, 256, 0, st>>>(g, F, gs.nout, seg_sq, w.r);
    GEO_LAUNCH_CHECK();
    vc_energy_kernel<<<(unsigned)n_curves, 64, 0, st>>>(seg_sq, z, F, gs.dz, energy);
    GEO_LAUNCH_CHECK();
    if (probe) {
        sv_sign_kernel<<<(unsigned)((gs.nout + 255) / 256), 256, 0, st>>>(gs.sp.So, gs.nout, w.sgn);
        GEO_LAUNCH_CHECK();
        rc = run_grid_tail(dc, gs, w.pt, w.sgn, 0, 0, n, grad, st);
        if (rc != GEO_OK) return rc;
        sv_probe_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(grad, gs.dz, n, probe);
        GEO_LAUNCH_CHECK();
    }
    return run_grid_tail(dc, gs, w.pt, w.r, 0, gs.nout, n, grad, st, F);
}

int grid_curve_check(const char *who, const geo_spatial_image_decoder_desc *dc, GridShape *gs, int64_t C, int F) {
    if (const int rc = check_grid_desc(dc, gs, who)) return rc;
    GEO_REQUIRE(F >= 2 && F <= CURVE_MAX_F, "%s: F %d not in [2,%d]", who, F, CURVE_MAX_F);
    GEO_REQUIRE(C >= 0, "%s: C %lld < 0", who, (long long)C);
    return GEO_OK;
}

int grid_curve_energy(const geo_spatial_image_decoder_desc *dc, const float *x, int64_t C, int F, double *energy_out,
                      double *seg_sq_out, double *grad_out, float *g_out, double *probe_out, void *ws, size_t ws_bytes,
                      hipStream_t st) {
    static const char who[] = "geo_spatial_curve_energy";
    GridShape gs;
    if (const int rc = grid_curve_check(who, dc, &gs, C, F)) return rc;
    if (C == 0) return GEO_OK;
    GEO_REQUIRE(x && energy_out && ws, "%s: null pointer", who);
    int64_t slice = 0;
    const auto bytes = [&](int64_t nc) { return grid_curve_slice_bytes(gs, nc, F); };
    if (const int rc = curve_slice_length(who, bytes, C, F, ws_bytes, &slice)) return rc;
    for (int64_t base = 0; base < C; base += slice) {
        const int64_t nc = C - base < slice ? C - base : slice;
        geo::Arena ar(ws, ws_bytes);
        const GridCurveWorkspace w = lay_out_grid_curve_slice(ar, gs, nc, F);
        GEO_REQUIRE_WORKSPACE("geo_spatial_curve_energy", ar, bytes(nc));
        const size_t at = (size_t)base * F;
        if (const int rc = grid_curve_evaluate(dc, gs, w, x + at * gs.dz, nc, F, energy_out + base,
                                               seg_sq_out ? seg_sq_out + (size_t)base * (F - 1) : w.st.seg_ev,
                                               grad_out ? grad_out + at * gs.dz : w.st.grad_ev, g_out ? g_out + at * gs.nout : w.g,
                                               probe_out ? probe_out + at : nullptr, st))
            return rc;
    }
    return GEO_OK;
}

int grid_curve_relax(const geo_spatial_image_decoder_desc *dc, float *x, int64_t C, int F, int n_iters, double *step,
                     double *energy0_out, double *energy_out, double *seg_sq_out, int32_t *accepted_out, void *ws, size_t ws_bytes,
                     hipStream_t st) {
    static const char who[] = "geo_spatial_curve_relax";
    GridShape gs;
    if (const int rc = grid_curve_check(who, dc, &gs, C, F)) return rc;
    GEO_REQUIRE(n_iters >= 0, "%s: n_iters %d < 0", who, n_iters);
    if (C == 0) return GEO_OK;
    GEO_REQUIRE(x && step && energy_out && accepted_out && ws, "%s: null pointer", who);
    int64_t slice = 0;
    const auto bytes = [&](int64_t nc) { return grid_curve_slice_bytes(gs, nc, F); };
    if (const int rc = curve_slice_length(who, bytes, C, F, ws_bytes, &slice)) return rc;
    // the probe costs one more VJP per frame: only for a slice with a curve whose step the caller left to the call (one copy of the
    // steps to the host, before the first launch; nothing is read back per iteration)
    std::vector<double> step_h((size_t)C);
    GEO_HIP_CHECK(hipMemcpyAsync(step_h.data(), step, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, st));
    GEO_HIP_CHECK(hipStreamSynchronize(st));
    const int iters = F == 2 ? 0 : n_iters;                       // no interior frame: nothing can move
    for (int64_t base = 0; base < C; base += slice) {
        const int64_t nc = C - base < slice ? C - base : slice;
        geo::Arena ar(ws, ws_bytes);
        const GridCurveWorkspace w = lay_out_grid_curve_slice(ar, gs, nc, F);
        GEO_REQUIRE_WORKSPACE("geo_spatial_curve_relax", ar, bytes(nc));
        bool need_probe = false;
        for (int64_t c = base; c < base + nc; ++c) need_probe |= step_h[(size_t)c] < 0.0;
        const CurveState &cs = w.st;
        float *xs = x + (size_t)base * F * gs.dz;
        double *seg_s = seg_sq_out ? seg_sq_out + (size_t)base * (F - 1) : nullptr;
        for (int it = -1; it < iters; ++it) {                     // it = -1: the curve itself
            if (const int rc = grid_curve_evaluate(dc, gs, w, it < 0 ? xs : cs.y, nc, F, cs.e_ev, cs.seg_ev, cs.grad_ev, w.g,
                                                   it < 0 && need_probe ? cs.tr : nullptr, st))
                return rc;
            curve_step_kernel<<<(unsigned)nc, CURVE_THREADS, 0, st>>>(cs, xs, F, gs.dz, it < 0, it == iters - 1, step + base,
                                                                      energy0_out ? energy0_out + base : nullptr, energy_out + base,
                                                                      seg_s, accepted_out + base);
            GEO_LAUNCH_CHECK();
        }
    }
    return GEO_OK;
}

// ================================ the metric tensor per latent ================================
// geo_vanilla_metric_tensor: G(z) = J(z)^T J(z), J = d sigmoid(decoder(z)) / dz.  A slice of latents runs the point pass, then
// the unit-tangent passes of curve_evaluate's trace branch over pseudo-edges (pair of latents, k) -- vc_unit_kernel,
// vj_mid_kernel<.., true>, vj_back_kernel<.., true, SQ, false, COLS> -- which leave the columns J[.][k] of item (edge, end) in
// `cols`; vm_gram_kernel reduces a latent's d columns to G in fp64 (and copies them to jac_out), and geo_sym_spectrum
// (csrc/sym_spectrum.hip) takes the eigenvalues of all n matrices at the end.
//
// Gram order.  One workgroup per latent.  The outputs go through LDS in chunks of GRAM_OC = 64, o ascending (the last chunk
// padded with zeros, which add nothing); the upper triangle of 16 x 16 tiles of G, tile t on wave t mod 4, each accumulated by
// v_mfma_f64_16x16x4_f64 over the chunk's 16 groups of four outputs in order.  A product of two float32 values is exact in
// fp64, so an entry is a sum of exact terms whose order is a function of (d, nout) alone: it does not depend on n, the
// latent's position, `index`, the slice, the stream or what the workspace held.  The lower triangle is written from the upper.
// (latent, k) tangent items of a slice at most.  The tangent kernels carry a call: at 8192 items vj_mid_kernel launches 1 600 to
// 2 048 workgroups and vj_back_kernel 4 096 on 256 CUs, and the slice's buffers are 0.9 GB at d = 128, 32 px x 3 (they grow in
// proportion).  The point pass and vm_gram_kernel see 8192 / d latents a slice: at d = 128 their 64 workgroups (4 for the front)
// leave most CUs idle and cost 35 % of a call in the kernel trace of DESIGN.md section 30 -- the follow-up named there.
constexpr int64_t METRIC_SLICE_ITEMS = 8192;
constexpr int GRAM_OC = 64, GRAM_LD = GRAM_OC + 4;
constexpr int GRAM_DT = MAX_D / 16, GRAM_WAVE_TILES = (GRAM_DT * (GRAM_DT + 1) / 2 + 3) / 4;
using f64x4 = __attribute__((__vector_size__(4 * sizeof(double)))) double;

struct MetricWorkspace {
    Workspace pt;
    int32_t *ia, *ib;
    float *sq, *cols;
};
MetricWorkspace lay_out_metric(geo::Arena &ar, const Shape &s, int64_t pairs) {
    MetricWorkspace w;
    const int64_t ne = pairs * s.d;                           // pseudo-edges (pair, k): two items each
    w.pt = lay_out(ar, s, 2 * pairs, ne);
    ar.take(w.ia, (size_t)ne); ar.take(w.ib, (size_t)ne);
    ar.take(w.sq, (size_t)2 * ne); ar.take(w.cols, (size_t)2 * ne * s.nout);
    return w;
}
size_t metric_bytes(const Shape &s, int64_t pairs) { return geo::measure(lay_out_metric, s, pairs); }
int64_t metric_pair_cap(const Shape &s, int64_t n) {
    const int64_t cap = METRIC_SLICE_ITEMS / (2 * s.d) < 1 ? 1 : METRIC_SLICE_ITEMS / (2 * s.d), need = n < 2 ? 1 : (n + 1) / 2;
    return need < cap ? need : cap;
}

// latent `node` of the slice: its column k is item 2 ((node / 2) d + k) + (node & 1) of cols
__global__ __launch_bounds__(256) void vm_gram_kernel(const float *__restrict__ cols, int d, int nout, int64_t node0,
                                                      double *__restrict__ G, float *__restrict__ jac_out) {
    __shared__ float Js[MAX_D][GRAM_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t node = blockIdx.x, q = node >> 1;
    const int side = (int)(node & 1);
    const int dt = (d + 15) / 16, ntiles = dt * (dt + 1) / 2;
    int bi[GRAM_WAVE_TILES], bj[GRAM_WAVE_TILES];
    f64x4 acc[GRAM_WAVE_TILES];
#pragma unroll
    for (int ti = 0; ti < GRAM_WAVE_TILES; ++ti) {
        int a = 0, p = wave + 4 * ti;
        if (p >= ntiles) p = 0;                               // (not used)
        while (p >= dt - a) p -= dt - a, ++a;
        bi[ti] = a;
        bj[ti] = a + p;
        acc[ti] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    for (int o0 = 0; o0 < nout; o0 += GRAM_OC) {
        __syncthreads();
        for (int i = tid; i < dt * 16 * GRAM_OC; i += 256) {
            const int k = i / GRAM_OC, oo = i - k * GRAM_OC, o = o0 + oo;
            float v = 0.f;
            if (k < d && o < nout) {
                v = cols[(2 * ((size_t)q * d + k) + side) * nout + o];
                if (jac_out) jac_out[((size_t)(node0 + node) * d + k) * nout + o] = v;
            }
            Js[k][oo] = v;
        }
        __syncthreads();
        for (int kk = 0; kk < GRAM_OC / 4; ++kk) {
            const int k = kk * 4 + (lane >> 4);               // A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15]
#pragma unroll
            for (int ti = 0; ti < GRAM_WAVE_TILES; ++ti)
                if (wave + 4 * ti < ntiles) {
                    const double a = (double)Js[bi[ti] * 16 + (lane & 15)][k], b = (double)Js[bj[ti] * 16 + (lane & 15)][k];
                    acc[ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ti], 0, 0, 0);
                }
        }
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg
    double *Gn = G + (size_t)(node0 + node) * d * d;
#pragma unroll
    for (int ti = 0; ti < GRAM_WAVE_TILES; ++ti)
        if (wave + 4 * ti < ntiles) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int gi = bi[ti] * 16 + (lane >> 4) + 4 * reg, gj = bj[ti] * 16 + (lane & 15);
                if (gi <= gj && gj < d) {
                    Gn[(size_t)gi * d + gj] = acc[ti][reg];
                    Gn[(size_t)gj * d + gi] = acc[ti][reg];
                }
            }
        }
}

int metric_tensor(const geo_vanilla_decoder_desc *dc, const float *z, const int32_t *index, int64_t n, double *G_out, float *jac_out,
                  double *eig_out, double *logvol_out, int32_t *rank_out, void *ws, size_t ws_bytes, hipStream_t st) {
    static const char who[] = "geo_vanilla_metric_tensor";
    Shape sh;
    if (const int rc = check_desc(dc, &sh, who)) return rc;
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "%s: n %lld", who, (long long)n);
    const bool spectrum = eig_out || logvol_out || rank_out;
    GEO_REQUIRE(!spectrum || (eig_out && logvol_out && rank_out), "%s: eig_out, logvol_out and rank_out go together", who);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(z && G_out && ws, "%s: null pointer", who);
    // the pairs of latents per slice: everything (up to the cap) when it fits, else the largest count that does
    int64_t pairs = metric_pair_cap(sh, n);
    if (ws_bytes < metric_bytes(sh, pairs)) {
        if (ws_bytes < metric_bytes(sh, 1)) {
            geo::set_error("%s: workspace of %zu bytes is below the minimum of %zu", who, ws_bytes, metric_bytes(sh, 1));
            return GEO_E_WORKSPACE;
        }
        int64_t lo = 1, hi = pairs;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (metric_bytes(sh, mid) <= ws_bytes) lo = mid; else hi = mid - 1;
        }
        pairs = lo;
    }
    for (int64_t base = 0; base < n; base += 2 * pairs) {
        const int64_t ns = n - base < 2 * pairs ? n - base : 2 * pairs, np = (ns + 1) / 2, ne = np * sh.d;
        geo::Arena ar(ws, ws_bytes);
        const MetricWorkspace w = lay_out_metric(ar, sh, np);
        GEO_REQUIRE_WORKSPACE("geo_vanilla_metric_tensor", ar, metric_bytes(sh, np));
        const Ends e{z, z, index, nullptr, base, (int)ns};
        int rc = run_point_pass(dc, sh, w.pt, e, ns, 0, st);
        if (rc != GEO_OK) return rc;
        vc_unit_kernel<<<(unsigned)ne, 256, 0, st>>>(dc->At, sh.d, sh.n1, 0, ns, w.pt.buf1, w.ia, w.ib);
        GEO_LAUNCH_CHECK();
        const Ends t{z, z, w.ia, w.ib, 0, (int)ne};
        rc = run_mid<true>(sh, dc, w.pt.buf1, w.pt.buf2, w.pt.mask1, w.pt.mask2, t, 1, 0, 2 * ne, st);
        if (rc != GEO_OK) return rc;
        rc = run_back<true, true, false, true>(sh, dc, w.pt.buf2, w.pt.sigp, t, 1, 0, ne, w.sq, st, w.cols);
        if (rc != GEO_OK) return rc;
        vm_gram_kernel<<<(unsigned)ns, 256, 0, st>>>(w.cols, sh.d, sh.nout, base, G_out, jac_out);
        GEO_LAUNCH_CHECK();
    }
    if (!spectrum) return GEO_OK;
    return geo_sym_spectrum(G_out, n, sh.d, sh.nout, eig_out, logvol_out, rank_out, st);
}

}  // namespace

extern "C" size_t geo_vanilla_metric_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n) {
    Shape sh;
    if (!make_shape(dec, &sh) || n < 0) return 0;
    return metric_bytes(sh, metric_pair_cap(sh, n));
}

extern "C" size_t geo_vanilla_metric_min_workspace_bytes(const geo_vanilla_decoder_desc *dec) {
    Shape sh;
    return make_shape(dec, &sh) ? metric_bytes(sh, 1) : 0;
}

extern "C" int geo_vanilla_metric_tensor(const geo_vanilla_decoder_desc *dec, const float *z, const int32_t *index, int64_t n,
                                         double *G_out, float *jac_out, double *eig_out, double *logvol_out, int32_t *rank_out,
                                         void *ws, size_t ws_bytes, void *stream) {
    return metric_tensor(dec, z, index, n, G_out, jac_out, eig_out, logvol_out, rank_out, ws, ws_bytes,
                         static_cast<hipStream_t>(stream));
}

extern "C" size_t geo_spatial_vjp_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int64_t n) {
    GridShape gs;
    if (!make_grid_shape(dec, &gs) || n < 0) return 0;
    return grid_layout_bytes(gs, n < 1 ? 1 : (n < VJP_ITEMS_PER_PASS ? n : VJP_ITEMS_PER_PASS));
}

extern "C" size_t geo_spatial_vjp_min_workspace_bytes(const geo_spatial_image_decoder_desc *dec) {
    GridShape gs;
    return make_grid_shape(dec, &gs) ? grid_layout_bytes(gs, 1) : 0;
}

extern "C" int geo_spatial_vjp(const geo_spatial_image_decoder_desc *dec, const float *z, const int32_t *index, int64_t n,
                               const float *u, double *out, void *ws, size_t ws_bytes, void *stream) {
    GridShape gs;
    if (const int rc = check_grid_desc(dec, &gs, "geo_spatial_vjp")) return rc;
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "geo_spatial_vjp: n %lld", (long long)n);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(z && u && out && ws, "geo_spatial_vjp: null pointer");
    int64_t pb = n < VJP_ITEMS_PER_PASS ? n : VJP_ITEMS_PER_PASS;
    while (pb >= 1 && grid_layout_bytes(gs, pb) > ws_bytes) pb = geo::shrink_pass(pb);
    if (pb < 1) {
        geo::set_error("geo_spatial_vjp: workspace of %zu bytes is below the minimum of %zu", ws_bytes, grid_layout_bytes(gs, 1));
        return GEO_E_WORKSPACE;
    }
    geo::Arena ar(ws, ws_bytes);
    const Workspace w = lay_out_grid(ar, gs, pb);
    GEO_REQUIRE_WORKSPACE("geo_spatial_vjp", ar, grid_layout_bytes(gs, pb));
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t p0 = 0; p0 < n; p0 += pb) {
        const int64_t cnt = n - p0 < pb ? n - p0 : pb;
        if (const int rc = run_grid_point_pass(dec, gs, w, z, index, p0, cnt, st, nullptr)) return rc;
        if (const int rc = run_grid_tail(dec, gs, w, u, p0, gs.nout, cnt, out + (size_t)p0 * gs.dz, st)) return rc;
    }
    return GEO_OK;
}

extern "C" size_t geo_spatial_curve_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int64_t C, int32_t F) {
    GridShape gs;
    if (!make_grid_shape(dec, &gs) || C < 0 || F < 2 || F > CURVE_MAX_F) return 0;
    return grid_curve_slice_bytes(gs, curve_slice_cap(C, F), F);
}

extern "C" size_t geo_spatial_curve_min_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int32_t F) {
    GridShape gs;
    if (!make_grid_shape(dec, &gs) || F < 2 || F > CURVE_MAX_F) return 0;
    return grid_curve_slice_bytes(gs, 1, F);
}

extern "C" int geo_spatial_curve_energy(const geo_spatial_image_decoder_desc *dec, const float *x, int64_t C, int32_t F,
                                        double *energy_out, double *seg_sq_out, double *grad_out, float *g_out, double *probe_out,
                                        void *ws, size_t ws_bytes, void *stream) {
    return grid_curve_energy(dec, x, C, F, energy_out, seg_sq_out, grad_out, g_out, probe_out, ws, ws_bytes,
                             static_cast<hipStream_t>(stream));
}

extern "C" int geo_spatial_curve_relax(const geo_spatial_image_decoder_desc *dec, float *x_inout, int64_t C, int32_t F, int32_t n_iters,
                                       double *step_inout, double *energy0_out, double *energy_out, double *seg_sq_out,
                                       int32_t *accepted_out, void *ws, size_t ws_bytes, void *stream) {
    return grid_curve_relax(dec, x_inout, C, F, n_iters, step_inout, energy0_out, energy_out, seg_sq_out, accepted_out, ws, ws_bytes,
                            static_cast<hipStream_t>(stream));
}

extern "C" size_t geo_vanilla_curve_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t C, int32_t F) {
    Shape sh;
    if (!make_shape(dec, &sh) || C < 0 || F < 2 || F > CURVE_MAX_F) return 0;
    return curve_slice_bytes(sh, curve_slice_cap(C, F), F);
}

extern "C" size_t geo_vanilla_curve_min_workspace_bytes(const geo_vanilla_decoder_desc *dec, int32_t F) {
    Shape sh;
    if (!make_shape(dec, &sh) || F < 2 || F > CURVE_MAX_F) return 0;
    return curve_slice_bytes(sh, 1, F);
}

extern "C" int geo_vanilla_curve_energy(const geo_vanilla_decoder_desc *dec, const float *x, int64_t C, int32_t F, double *energy_out,
                                        double *seg_sq_out, double *grad_out, float *g_out, double *trace_out, void *ws,
                                        size_t ws_bytes, void *stream) {
    return curve_energy(dec, x, C, F, energy_out, seg_sq_out, grad_out, g_out, trace_out, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int geo_vanilla_curve_relax(const geo_vanilla_decoder_desc *dec, float *x_inout, int64_t C, int32_t F, int32_t n_iters,
                                       double *step_inout, double *energy0_out, double *energy_out, double *seg_sq_out,
                                       int32_t *accepted_out, void *ws, size_t ws_bytes, void *stream) {
    return curve_relax(dec, x_inout, C, F, n_iters, step_inout, energy0_out, energy_out, seg_sq_out, accepted_out, ws, ws_bytes,
                       static_cast<hipStream_t>(stream));
}

extern "C" size_t geo_vanilla_vjp_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n) {
    Shape sh;
    if (!make_shape(dec, &sh) || n < 0) return 0;
    return vjp_layout_bytes(sh, n < 1 ? 1 : (n < VJP_ITEMS_PER_PASS ? n : VJP_ITEMS_PER_PASS));
}

extern "C" size_t geo_vanilla_vjp_min_workspace_bytes(const geo_vanilla_decoder_desc *dec) {
    Shape sh;
    return make_shape(dec, &sh) ? vjp_layout_bytes(sh, 1) : 0;
}

extern "C" int geo_vanilla_vjp(const geo_vanilla_decoder_desc *dec, const float *z, const int32_t *index, int64_t n, const float *u,
                               double *out, void *ws, size_t ws_bytes, void *stream) {
    Shape sh;
    int rc = check_desc(dec, &sh, "geo_vanilla_vjp");
    if (rc != GEO_OK) return rc;
    GEO_REQUIRE(dec->w2t && dec->w3t && dec->Atq, "geo_vanilla_vjp: null transposed pack in the descriptor");
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "geo_vanilla_vjp: n %lld", (long long)n);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(z && u && out && ws, "geo_vanilla_vjp: null pointer");
    int64_t pb = n < VJP_ITEMS_PER_PASS ? n : VJP_ITEMS_PER_PASS;
    while (pb >= 1 && vjp_layout_bytes(sh, pb) > ws_bytes) pb = geo::shrink_pass(pb);
    if (pb < 1) {
        geo::set_error("geo_vanilla_vjp: workspace of %zu bytes is below the minimum of %zu", ws_bytes, vjp_layout_bytes(sh, 1));
        return GEO_E_WORKSPACE;
    }
    geo::Arena ar(ws, ws_bytes);
    const VjpWorkspace w = lay_out_vjp(ar, sh, pb);
    GEO_REQUIRE_WORKSPACE("geo_vanilla_vjp", ar, vjp_layout_bytes(sh, pb));
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t p0 = 0; p0 < n; p0 += pb) {
        const int64_t cnt = n - p0 < pb ? n - p0 : pb;
        const Ends e{z, z, index, nullptr, p0, (int)cnt};
        rc = run_point_pass(dec, sh, w.pt, e, cnt, 0, st);
        if (rc != GEO_OK) return rc;
        rc = run_vjp_tail(dec, sh, w, u, p0, cnt, out + (size_t)p0 * sh.d, st);
        if (rc != GEO_OK) return rc;
    }
    return GEO_OK;
}

extern "C" size_t geo_vanilla_jvp_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n_edges) {
    Shape sh;
    if (!make_shape(dec, &sh) || n_edges < 0) return 0;
    const int64_t eb = n_edges < 1 ? 1 : (n_edges < EDGES_PER_PASS ? n_edges : EDGES_PER_PASS);
    return layout_bytes(sh, 2 * eb, eb);
}

extern "C" size_t geo_vanilla_jvp_edges_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n_nodes, int64_t n_edges) {
    Shape sh;
    if (!make_shape(dec, &sh) || n_edges < 0 || n_nodes < 0) return 0;
    const int64_t eb = n_edges < 1 ? 1 : (n_edges < EDGES_PER_PASS ? n_edges : EDGES_PER_PASS);
    return layout_bytes(sh, n_nodes >= 1 && n_nodes <= 2 * n_edges ? n_nodes : 2 * eb, eb);
}

extern "C" int geo_vanilla_jvp_pairs(const geo_vanilla_decoder_desc *dec, const float *z_start, const float *z_end, int64_t n_edges,
                                     int32_t batch_size, float *len_out, void *ws, size_t ws_bytes, void *stream) {
    (void)batch_size;
    Shape sh;
    int rc = check_desc(dec, &sh, "geo_vanilla_jvp_pairs");
    if (rc != GEO_OK) return rc;
    GEO_REQUIRE(n_edges >= 0, "geo_vanilla_jvp_pairs: n_edges %lld", (long long)n_edges);
    if (n_edges == 0) return GEO_OK;
    GEO_REQUIRE(z_start && z_end && len_out && ws, "geo_vanilla_jvp_pairs: null pointer");
    return run(dec, sh, z_start, z_end, nullptr, nullptr, 0, n_edges, len_out, ws, ws_bytes, static_cast<hipStream_t>(stream),
               "geo_vanilla_jvp_pairs");
}

extern "C" int geo_vanilla_jvp_edges(const geo_vanilla_decoder_desc *dec, const float *z, int64_t n_nodes, const int32_t *src,
                                     const int32_t *dst, int64_t n_edges, int32_t batch_size, float *len_out, void *ws,
                                     size_t ws_bytes, void *stream) {
    (void)batch_size;
    Shape sh;
    int rc = check_desc(dec, &sh, "geo_vanilla_jvp_edges");
    if (rc != GEO_OK) return rc;
    GEO_REQUIRE(n_edges >= 0 && n_nodes >= 0 && n_nodes < ((int64_t)1 << 31), "geo_vanilla_jvp_edges: n_nodes %lld, n_edges %lld",
                (long long)n_nodes, (long long)n_edges);
    if (n_edges == 0) return GEO_OK;
    GEO_REQUIRE(z && src && dst && len_out && ws && n_nodes >= 1, "geo_vanilla_jvp_edges: null pointer or no latents");
    // once per latent when that is less work than once per edge end and the workspace holds every latent's masks
    const bool resident = n_nodes <= 2 * n_edges && layout_bytes(sh, n_nodes, 1) <= ws_bytes;
    return run(dec, sh, z, z, src, dst, resident ? n_nodes : 0, n_edges, len_out, ws, ws_bytes, static_cast<hipStream_t>(stream),
               "geo_vanilla_jvp_edges");
}

extern "C" size_t geo_vanilla_decode_workspace_bytes(const geo_vanilla_decoder_desc *dec, int64_t n) {
    Shape sh;
    if (!make_shape(dec, &sh) || n < 0) return 0;
    const size_t per_item[2] = {(size_t)sh.n1, (size_t)sh.n2};      // the two activation buffers of the image decode
    return geo::pass_query_bytes(per_item, 2, ITEMS_PER_PASS, n);
}

extern "C" int geo_vanilla_decode(const geo_vanilla_decoder_desc *dec, const float *z, const int32_t *index, int64_t n,
                                  float *logits_out, void *ws, size_t ws_bytes, void *stream) {
    Shape sh;
    int rc = check_desc(dec, &sh, "geo_vanilla_decode");
    if (rc != GEO_OK) return rc;
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "geo_vanilla_decode: n %lld", (long long)n);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(z && logits_out && ws, "geo_vanilla_decode: null pointer");
    const size_t per_item[2] = {(size_t)sh.n1, (size_t)sh.n2};
    int64_t pb;
    float *buf[2];
    rc = geo::plan_passes("geo_vanilla_decode", per_item, 2, ITEMS_PER_PASS, n, ws, ws_bytes, &pb, buf);
    if (rc != GEO_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t p0 = 0; p0 < n; p0 += pb) {
        const int64_t cnt = n - p0 < pb ? n - p0 : pb;
        const Ends e{z, z, index, nullptr, p0, (int)cnt};
        const dim3 grid((unsigned)((cnt + FRONT_ROWS - 1) / FRONT_ROWS), FRONT_SPLIT);
        vj_front_kernel<false, false><<<grid, 256, 0, st>>>(e, (int)cnt, sh.d, sh.dp, sh.n1, dec->At, dec->c, buf[0], nullptr, 0);
        GEO_LAUNCH_CHECK();
        rc = decode_tail(sh.c1, sh.c2, sh.co, sh.s1, 0, dec->w2p, dec->scale2, dec->shift2, dec->w3p, dec->b3, buf[0], buf[1], cnt,
                         logits_out + (size_t)p0 * sh.nout, st);
        if (rc != GEO_OK) return rc;
    }
    return GEO_OK;
}

extern "C" size_t geo_spatial_decode_workspace_bytes(const geo_spatial_image_decoder_desc *dec, int64_t n) {
    SpatialShape sh;
    if (!make_spatial_shape(dec, &sh) || n < 0) return 0;
    return geo::pass_query_bytes(sh.per_item, 2, ITEMS_PER_PASS, n);
}

extern "C" int geo_spatial_decode(const geo_spatial_image_decoder_desc *dec, const float *z, const float *table, const int32_t *codes,
                                  int64_t n, float *logits_out, void *ws, size_t ws_bytes, void *stream) {
    SpatialShape sh;
    GEO_REQUIRE(make_spatial_shape(dec, &sh), "geo_spatial_decode: decoder configuration not covered (see geo_hip.h)");
    GEO_REQUIRE(dec->w1p && dec->scale1 && dec->shift1 && dec->w2p && dec->scale2 && dec->shift2 && dec->w3p && dec->b3,
                "geo_spatial_decode: null pointer in the descriptor");
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "geo_spatial_decode: n %lld", (long long)n);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE((z != nullptr) != (table != nullptr || codes != nullptr) && (table != nullptr) == (codes != nullptr),
                "geo_spatial_decode: give either z or (table, codes), not both and not neither");
    GEO_REQUIRE(logits_out && ws, "geo_spatial_decode: null pointer");
    int64_t pb;
    float *buf[2];
    int rc = geo::plan_passes("geo_spatial_decode", sh.per_item, 2, ITEMS_PER_PASS, n, ws, ws_bytes, &pb, buf);
    if (rc != GEO_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nout = (size_t)sh.co * sh.So * sh.So;
    for (int64_t p0 = 0; p0 < n; p0 += pb) {
        const int64_t cnt = n - p0 < pb ? n - p0 : pb;
        const unsigned grid = (unsigned)((cnt + SD_ITEMS - 1) / SD_ITEMS);
        if (sh.c1 == 128)
            sd_front_kernel<128><<<grid, 512, 0, st>>>(z, table, codes, p0, cnt, sh.d, sh.dp, dec->w1p, dec->scale1, dec->shift1, buf[0]);
        else
            sd_front_kernel<64><<<grid, 512, 0, st>>>(z, table, codes, p0, cnt, sh.d, sh.dp, dec->w1p, dec->scale1, dec->shift1, buf[0]);
        GEO_LAUNCH_CHECK();
        rc = decode_tail(sh.c1, sh.c2, sh.co, 8, sh.crop, dec->w2p, dec->scale2, dec->shift2, dec->w3p, dec->b3, buf[0], buf[1], cnt,
                         logits_out + (size_t)p0 * nout, st);
        if (rc != GEO_OK) return rc;
    }
    return GEO_OK;
}
