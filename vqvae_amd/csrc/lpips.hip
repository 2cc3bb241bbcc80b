// lpips.hip -- LPIPS v0.1 with the AlexNet backbone (normalize = False, spatial = False) of pairs of 3 x 64 x 64 images on
// gfx950.
//
//   scaled = (x - shift) / scale per channel
//   Conv(3,64,k11,s4,p2) ReLU -> f1 (15 x 15) | MaxPool(3,s2) Conv(64,192,k5,p2) ReLU -> f2 (7 x 7)
//   MaxPool(3,s2) Conv(192,384,k3,p1) ReLU -> f3 (3 x 3) | Conv(384,256,k3,p1) ReLU -> f4 | Conv(256,256,k3,p1) ReLU -> f5
//   d_l = mean over pixels of sum_c lin_l[c] (u0 - u1)^2,  u = f / (sqrt(sum_c f^2) + 1e-10);  the pair's value = sum_l d_l
//
// A pass of `cnt` pairs is 2 cnt images: image i < cnt is x0[i], image cnt + i is x1[i].  Activations are f32, channels last
// ([image][pixel][channel]), and all five of them stay in the workspace for the distance step.
//
//   lpips_conv1_kernel     one image per workgroup: the scaled image with its two rows and columns of zeros on every side in
//                          LDS (3 x 68 x 68 floats), implicit GEMM on v_mfma_f32_32x32x2_f32, M = 225 output pixels in 8 tiles
//                          (one per wave), N = 64 channels in 2 tiles (both in the wave, sharing A), K = (c, ky, kx) with kx
//                          padded from 11 to 12 (a zero weight and a zero A value)
//   lpips_conv_kernel      layers 2 to 5: G images per group, their input in LDS (the 3 x 3 stride-2 max-pool is applied while
//                          staging: layers 2 and 3 read the un-pooled ReLU output of the layer before), M = (image, pixel), K =
//                          (tap, input channel), N = output channels.  One 32 x 32 tile per wave, a group's tiles spread over
//                          several workgroups, so that a batch of 32 pairs already fills the CUs; a tap in the padding and a
//                          row past the last image read a row of zeros
//   lpips_distance_kernel  one pair per workgroup of 16 waves, fp64 from the f32 features: one wave per pixel (lanes over channels, an xor
//                          butterfly for the three channel sums), then the pixel mean in pixel order and the layer sum in layer
//                          order by one thread
//
// Every feature value is one fixed-order chain of its own image and every reduction has one association: no atomics, nothing
// split across workgroups.  (u0 - u1)^2 is the same bits as (u1 - u0)^2, so a pair's result does not depend on which image is
// x0, nor on n, its position, the pass or workspace size, the stream or the run.
#include "geo_common.h"
#include "mfma_conv.h"

namespace {

using mfma_conv::f32x16;

constexpr int64_t PAIRS_PER_PASS = 4096;
constexpr int WAVE = 64;
constexpr int IMG = 3 * 64 * 64;
constexpr int P1 = 225, P2 = 49, P3 = 9;                     // pixels of f1, f2, f3 .. f5
constexpr int C1 = 64, C2 = 192, C3 = 384, C4 = 256, C5 = 256;
constexpr size_t N1 = (size_t)P1 * C1, N2 = (size_t)P2 * C2, N3 = (size_t)P3 * C3, N4 = (size_t)P3 * C4, N5 = (size_t)P3 * C5;
constexpr int DIST_PIX = P1 + P2 + 3 * P3;                   // 301 pixels of the five layers
constexpr int DIST_WAVES = 16;

constexpr size_t PER_PAIR[5] = {2 * N1, 2 * N2, 2 * N3, 2 * N4, 2 * N5};     // floats of a pair's two images in the five buffers

// ---- layer 1.  w1p: [(c 11 + ky)][h][co 64][8]: element s < 6 = conv1.weight[co][c][ky][2 s + h] (0 for kx = 11), 0 for
// s = 6, 7; lane half h of the MFMA takes the even (h = 0) or odd (h = 1) kx.  The chain of an output value runs over c, ky
// and the six kx pairs from 0; the bias is added last.
__global__ __launch_bounds__(512) void lpips_conv1_kernel(const float *__restrict__ x0, const float *__restrict__ x1, int64_t cnt,
                                                          float *__restrict__ f1, const float *__restrict__ w1p,
                                                          const float *__restrict__ b1) {
    constexpr int SP = 68, SO = 15;
    __shared__ __attribute__((aligned(16))) float img[3 * SP * SP];
    const int tid = threadIdx.x;
    const int64_t im = blockIdx.x;
    const float *src = im < cnt ? x0 + (size_t)im * IMG : x1 + (size_t)(im - cnt) * IMG;
    for (int q = tid; q < 3 * SP * SP; q += 512) {
        const int c = q / (SP * SP), rem = q - c * SP * SP, yy = rem / SP, xx = rem - yy * SP;
        float v = 0.f;
        if (yy >= 2 && yy < 66 && xx >= 2 && xx < 66) {
            const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
            const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
            v = (src[(c * 64 + yy - 2) * 64 + xx - 2] - shift) / scale;
        }
        img[q] = v;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int r = wave * 32 + j;
    const bool rv = r < P1;
    const int oy = rv ? r / SO : 0, ox = rv ? r - oy * SO : 0;
    f32x16 acc0, acc1;
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc0[q] = 0.f; acc1[q] = 0.f; }
    for (int c = 0; c < 3; ++c) {
        for (int ky = 0; ky < 11; ++ky) {
            const float *ap = img + (c * SP + 4 * oy + ky) * SP + 4 * ox + h;
            const float4 *bp = reinterpret_cast<const float4 *>(w1p) + ((size_t)((c * 11 + ky) * 2 + h) * C1 + j) * 2;
            const float4 b0l = bp[0], b0h = bp[1], b1l = bp[64], b1h = bp[65];        // channels j and 32 + j
            const float b0[6] = {b0l.x, b0l.y, b0l.z, b0l.w, b0h.x, b0h.y};
            const float b1v[6] = {b1l.x, b1l.y, b1l.z, b1l.w, b1h.x, b1h.y};
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                float a = ap[2 * s];
                if (s == 5 && h == 1) a = 0.f;                                          // kx = 11 does not exist
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1v[s], acc1, 0, 0, 0);
            }
        }
    }
    const float bias0 = b1[j], bias1 = b1[32 + j];
    float *dst = f1 + (size_t)im * N1;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ro = mfma_conv::acc_row(q, h, wave * 32);
        if (ro < P1) {
            const float v0 = acc0[q] + bias0, v1 = acc1[q] + bias1;
            dst[(size_t)ro * C1 + j] = v0 > 0.f ? v0 : 0.f;
            dst[(size_t)ro * C1 + 32 + j] = v1 > 0.f ? v1 : 0.f;
        }
    }
}

// ---- layers 2 to 5: Conv(CIN, COUT, k KS, s1, p KS / 2) on S x S pixels of G images per group.  SRC is the side of the
// input as stored: SRC == S reads it as it is, SRC == 2 S + 1 takes the 3 x 3 stride-2 maximum while staging.  LDS rows are
// [image, pixel][CIN] in mfma_conv.h's layout.  The group's MT x NT tiles of 32 x 32 are spread over gridDim.y workgroups of NW
// waves, one tile per wave (every workgroup stages the group's input).  wp: [tap][CIN / 4][COUT][4], element (tap, q, co, r) =
// weight[co][4 q + r][ky][kx], tap = KS ky + kx.  The chain runs over the taps, then the 8-channel blocks, from 0; the bias is
// added last.
template <int CIN, int COUT, int KS, int S, int SRC, int G, int NW>
__global__ __launch_bounds__(NW * 64) void lpips_conv_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t n_img,
                                                             const float *__restrict__ wp, const float *__restrict__ bias) {
    constexpr int LD = CIN + 4, P = S * S, ROWS = G * P, ZR = ROWS, MT = (ROWS + 31) / 32, NT = COUT / 32;
    constexpr int PAD = KS / 2, PSRC = SRC * SRC, NTHR = NW * 64;
    static_assert(SRC == S || SRC == 2 * S + 1, "the input is read as stored or max-pooled 3 x 3 stride 2");
    static_assert((ROWS + 1) * LD * 4 <= 128 * 1024, "LDS of one workgroup");
    __shared__ __attribute__((aligned(16))) float lds[(ROWS + 1) * LD];
    const int64_t item0 = (int64_t)blockIdx.x * G;
    const int live = (int)(n_img - item0 < G ? n_img - item0 : G);
    const int tid = threadIdx.x;
    for (int q = tid; q < live * P * (CIN / 4); q += NTHR) {
        const int row = q / (CIN / 4), ci = (q - row * (CIN / 4)) * 4;
        const int g = row / P, p = row - g * P;
        const float *s = in + (size_t)(item0 + g) * PSRC * CIN + ci;
        float4 v;
        if constexpr (SRC == S) {
            v = *reinterpret_cast<const float4 *>(s + (size_t)p * CIN);
        } else {
            const int py = p / S, px = p - py * S;
            v = *reinterpret_cast<const float4 *>(s + (size_t)(2 * py * SRC + 2 * px) * CIN);
#pragma unroll
            for (int t = 1; t < 9; ++t) {
                const float4 u = *reinterpret_cast<const float4 *>(s + (size_t)((2 * py + t / 3) * SRC + 2 * px + t % 3) * CIN);
                v.x = fmaxf(v.x, u.x);
                v.y = fmaxf(v.y, u.y);
                v.z = fmaxf(v.z, u.z);
                v.w = fmaxf(v.w, u.w);
            }
        }
        *reinterpret_cast<float4 *>(lds + (size_t)row * LD + ci) = v;
    }
    mfma_conv::fill_zero_row<NTHR>(lds, ZR, LD, tid);
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int rows = live * P;
    const int task = blockIdx.y * NW + wave;                        // (wave-uniform; no barrier follows)
    const int nt = task % NT, mt = task / NT;
    if (mt >= MT || mt * 32 >= rows) return;
    const int r = mt * 32 + j;
    const bool rv = r < rows;
    const int g = rv ? r / P : 0, pq = rv ? r - g * P : 0;
    const int oy = pq / S, ox = pq - oy * S;
    const int co = nt * 32 + j;
    f32x16 acc[1];
    mfma_conv::clear(acc);
    for (int tap = 0; tap < KS * KS; ++tap) {
        const int ky = tap / KS, kx = tap - ky * KS;
        const float *ap[1] = {mfma_conv::tap_row(lds, LD, ZR, rv, g, oy - PAD + ky, ox - PAD + kx, S, P, h)};
        const float4 *bp = reinterpret_cast<const float4 *>(wp) + ((size_t)tap * (CIN / 4) + h) * COUT + co;
        mfma_conv::k_chain<1, 4>(acc, ap, bp, CIN / 8, COUT);
    }
    const float b = bias[co];
    float *dst = out + (size_t)item0 * P * COUT;                    // row r of the group = (image, pixel), contiguous
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ro = mfma_conv::acc_row(q, h, mt * 32);
        if (ro < rows) {
            const float v = acc[0][q] + b;
            dst[(size_t)ro * COUT + co] = v > 0.f ? v : 0.f;
        }
    }
}

// ---- the distance, in fp64 from the f32 features.
struct DistArgs {
    const float *f[5];
    const float *lin[5];
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

__global__ __launch_bounds__(DIST_WAVES * 64) void lpips_distance_kernel(DistArgs a, int64_t cnt, double *__restrict__ total,
                                                             double *__restrict__ layer) {
    __shared__ double pix[DIST_PIX];
    __shared__ double lay[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pair = blockIdx.x;
    for (int gp = wave; gp < DIST_PIX; gp += DIST_WAVES) {                   // (wave-uniform)
        int l, p, P, C;
        if (gp < P1) { l = 0, p = gp, P = P1, C = C1; }
        else if (gp < P1 + P2) { l = 1, p = gp - P1, P = P2, C = C2; }
        else { l = 2 + (gp - P1 - P2) / P3, p = (gp - P1 - P2) % P3, P = P3, C = l == 2 ? C3 : C4; }
        const float *u0 = a.f[l] + ((size_t)pair * P + p) * C, *u1 = a.f[l] + ((size_t)(cnt + pair) * P + p) * C;
        const float *lin = a.lin[l];
        double s0 = 0.0, s1 = 0.0;
        for (int c = lane; c < C; c += WAVE) {
            const double v0 = u0[c], v1 = u1[c];
            s0 += v0 * v0;
            s1 += v1 * v1;
        }
        const double n0 = sqrt(wave_sum(s0)) + 1e-10, n1 = sqrt(wave_sum(s1)) + 1e-10;
        double d = 0.0;
        for (int c = lane; c < C; c += WAVE) {
            const double diff = (double)u0[c] / n0 - (double)u1[c] / n1;
            d += (double)lin[c] * (diff * diff);
        }
        d = wave_sum(d);
        if (lane == 0) pix[gp] = d;
    }
    __syncthreads();
    if (tid < 5) {
        const int first = tid == 0 ? 0 : (tid == 1 ? P1 : P1 + P2 + (tid - 2) * P3), P = tid == 0 ? P1 : (tid == 1 ? P2 : P3);
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += pix[first + p];
        lay[tid] = s / P;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int l = 0; l < 5; ++l) {
            s += lay[l];
            if (layer) layer[pair * 5 + l] = lay[l];
        }
        total[pair] = s;
    }
}

// One layer: a grid of (groups of G images) x (the workgroups that share a group's tiles).
template <int CIN, int COUT, int KS, int S, int SRC, int G, int NW>
void launch_conv(const float *in, float *out, int64_t ni, const float *wp, const float *bias, hipStream_t st) {
    constexpr int MT = (G * S * S + 31) / 32, NT = COUT / 32;
    const dim3 grid((unsigned)((ni + G - 1) / G), (MT * NT + NW - 1) / NW);
    lpips_conv_kernel<CIN, COUT, KS, S, SRC, G, NW><<<grid, NW * 64, 0, st>>>(in, out, ni, wp, bias);
}

int run_pass(const geo_lpips_alex_desc *net, const float *x0, const float *x1, int64_t cnt, float *const f[5], double *total,
             double *layer, hipStream_t st) {
    const int64_t ni = 2 * cnt;
    lpips_conv1_kernel<<<(unsigned)ni, 512, 0, st>>>(x0, x1, cnt, f[0], net->w1p, net->b1);
    GEO_LAUNCH_CHECK();
    launch_conv<C1, C2, 5, 7, 15, 4, 8>(f[0], f[1], ni, net->w2p, net->b2, st);
    GEO_LAUNCH_CHECK();
    launch_conv<C2, C3, 3, 3, 7, 7, 4>(f[1], f[2], ni, net->w3p, net->b3, st);
    GEO_LAUNCH_CHECK();
    launch_conv<C3, C4, 3, 3, 3, 7, 8>(f[2], f[3], ni, net->w4p, net->b4, st);
    GEO_LAUNCH_CHECK();
    launch_conv<C4, C5, 3, 3, 3, 7, 8>(f[3], f[4], ni, net->w5p, net->b5, st);
    GEO_LAUNCH_CHECK();
    DistArgs a;
    for (int l = 0; l < 5; ++l) a.f[l] = f[l];
    a.lin[0] = net->lin1, a.lin[1] = net->lin2, a.lin[2] = net->lin3, a.lin[3] = net->lin4, a.lin[4] = net->lin5;
    lpips_distance_kernel<<<(unsigned)cnt, DIST_WAVES * 64, 0, st>>>(a, cnt, total, layer);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

}  // namespace

extern "C" size_t geo_lpips_alex_workspace_bytes(int64_t n) {
    if (n < 0) return 0;
    return geo::pass_query_bytes(PER_PAIR, 5, PAIRS_PER_PASS, n);
}

extern "C" int geo_lpips_alex(const geo_lpips_alex_desc *net, const float *x0, const float *x1, int64_t n, double *total_out,
                              double *layer_out, void *ws, size_t ws_bytes, void *stream) {
    GEO_REQUIRE(net, "geo_lpips_alex: null descriptor");
    GEO_REQUIRE(net->w1p && net->b1 && net->w2p && net->b2 && net->w3p && net->b3 && net->w4p && net->b4 && net->w5p && net->b5 &&
                    net->lin1 && net->lin2 && net->lin3 && net->lin4 && net->lin5,
                "geo_lpips_alex: null pointer in the descriptor");
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "geo_lpips_alex: n %lld", (long long)n);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(x0 && x1 && total_out && ws, "geo_lpips_alex: null pointer");
    int64_t pb;
    float *f[5];
    int rc = geo::plan_passes("geo_lpips_alex", PER_PAIR, 5, PAIRS_PER_PASS, n, ws, ws_bytes, &pb, f);
    if (rc != GEO_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t p0 = 0; p0 < n; p0 += pb) {
        const int64_t cnt = n - p0 < pb ? n - p0 : pb;
        rc = run_pass(net, x0 + (size_t)p0 * IMG, x1 + (size_t)p0 * IMG, cnt, f, total_out + p0,
                      layer_out ? layer_out + p0 * 5 : nullptr, st);
        if (rc != GEO_OK) return rc;
    }
    return GEO_OK;
}
