// encode.hip -- images -> (mu, logvar): the encoders of both VAEs with FIXED statistics on gfx950.
//
//   Conv(C,e1,k3,s2,p1) -> norm -> ReLU -> Conv(e1,e2,k3,s2,p1) -> norm -> ReLU -> Conv(e2,e3,k3,s2,p1) -> norm -> ReLU
//       28 -> 14 -> 7 -> 4 px  |  32 -> 16 -> 8 -> 4 px,   (e1, e2, e3) = (64, 128, 256) | (32, 64, 128)
//   vanilla head: fc_mu, fc_logvar = Linear(16 e3, d) on the NCHW flatten;  spatial head: Conv(e3, d, 1) -> (n, d, 4, 4)
//
// Activations are f32, channels last ([item][pixel][channel]); each norm and its convolution's bias arrive folded into one
// scale and one shift per channel (composed in fp64, rounded once) and are applied as one fmaf before the ReLU.
//
//   enc_first_kernel   layer 1 (K = 9 C <= 27): vector fmafs, the padded image in LDS, one item per workgroup
//   enc_conv_kernel    layers 2 and 3: implicit GEMM on v_mfma_f32_32x32x2_f32, M = (item, output pixel), K = (tap, input
//                      channel), N = output channels; the items' inputs in LDS, a tap in the padding reads a zero row
//   enc_head_kernel    both heads as one GEMM over the rows of the last activation read as a matrix [rows][K]: vanilla rows are
//                      items (K = 16 e3 in 16 per-pixel segments), spatial rows are (item, pixel) (K = e3, one segment); a
//                      segment is one chain from 0, the segments are added in pixel order, then the bias
//
// Every output value is a fixed-order chain of its own item, no atomics, no split across workgroups: a row's (mu, logvar) does
// not depend on the batch, its position in it, the pass size, the workspace, the stream or the run.
#include "geo_common.h"
#include "mfma_conv.h"

namespace {

using mfma_conv::f32x16;

constexpr int64_t ITEMS_PER_PASS = 4096;
constexpr int MAX_D_VANILLA = 128, MAX_D_SPATIAL = 64;
constexpr int HEAD_ROWS = 32;

struct Shape {
    int C, S, e1, e2, e3, d, spatial, npad;
    size_t per_item[3];        // floats per item of the three activation buffers
};

bool make_shape(const geo_image_encoder_desc *e, Shape *s) {
    if (!e) return false;
    if (!((e->in_channels == 1 && e->in_size == 28) || (e->in_channels == 3 && e->in_size == 32))) return false;
    if (!((e->e1 == 64 && e->e2 == 128 && e->e3 == 256) || (e->e1 == 32 && e->e2 == 64 && e->e3 == 128))) return false;
    if (e->spatial_head != 0 && e->spatial_head != 1) return false;
    if (e->latent_dim < 1 || e->latent_dim > (e->spatial_head ? MAX_D_SPATIAL : MAX_D_VANILLA)) return false;
    s->C = e->in_channels;
    s->S = e->in_size;
    s->e1 = e->e1;
    s->e2 = e->e2;
    s->e3 = e->e3;
    s->d = e->latent_dim;
    s->spatial = e->spatial_head;
    s->npad = (2 * s->d + 31) & ~31;
    s->per_item[0] = (size_t)(s->S / 2) * (s->S / 2) * s->e1;
    s->per_item[1] = (size_t)(s->S / 4) * (s->S / 4) * s->e2;
    s->per_item[2] = (size_t)16 * s->e3;
    return true;
}

// ---- layer 1: one image per workgroup.  The image is staged with one row and one column of zeros in front (the only padding
// a stride-2 k3 p1 convolution of an even size reads).  A thread owns one output channel (its 9 C weights in registers) and
// every (256 / E1)-th output pixel; the chain runs over (channel, ky, kx) from 0.  w1p: [(c, ky, kx)][e1].
template <int C, int S, int E1>
__global__ __launch_bounds__(256) void enc_first_kernel(const float *__restrict__ x, float *__restrict__ out,
                                                        const float *__restrict__ w1p, const float *__restrict__ sc1,
                                                        const float *__restrict__ sh1) {
    constexpr int SP = S + 1, SO = S / 2, P = SO * SO, K = 9 * C;
    __shared__ float img[C * SP * SP];
    const int tid = threadIdx.x;
    const float *src = x + (size_t)blockIdx.x * C * S * S;
    for (int q = tid; q < C * SP * SP; q += 256) {
        const int c = q / (SP * SP), rem = q - c * SP * SP, yy = rem / SP, xx = rem - yy * SP;
        img[q] = (yy > 0 && xx > 0) ? src[(c * S + yy - 1) * S + xx - 1] : 0.f;
    }
    const int co = tid % E1;
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = w1p[k * E1 + co];
    const float scale = sc1[co], shift = sh1[co];
    __syncthreads();
    float *dst = out + (size_t)blockIdx.x * P * E1;
    for (int pix = tid / E1; pix < P; pix += 256 / E1) {
        const int oy = pix / SO, ox = pix - oy * SO;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    acc = fmaf(img[(c * SP + 2 * oy + ky) * SP + 2 * ox + kx], w[(c * 3 + ky) * 3 + kx], acc);
        const float v = fmaf(scale, acc, shift);
        dst[pix * E1 + co] = v > 0.f ? v : 0.f;
    }
}

// ---- layers 2 and 3: Conv(CIN, COUT, k3, s2, p1) of G items per workgroup, sin x sin -> so x so pixels (so = ceil(sin / 2)).
// The items' inputs ([pixel][CIN]) are staged in LDS in mfma_conv.h's layout.  8 waves, one 32 x 32 tile each: wave = (N tile,
// M tile), G and the sizes are chosen so that the workgroup has exactly 8 tiles.  K runs over (tap 0..8, 8-channel block).
// wp: [tap][CIN / 4][COUT][4].
template <int CIN, int COUT, int G, int PIN_MAX>
__global__ __launch_bounds__(512) void enc_conv_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t n_items, int sin,
                                                       const float *__restrict__ wp, const float *__restrict__ sc,
                                                       const float *__restrict__ sh) {
    constexpr int LD = CIN + 4, TN = COUT / 32, ZR = G * PIN_MAX;
    static_assert((G * (PIN_MAX / 4) / 32) * TN == 8, "a workgroup is 8 tiles of 32 x 32");
    static_assert((G * PIN_MAX + 1) * LD * 4 <= 80 * 1024, "two workgroups share a CU's LDS");
    __shared__ __attribute__((aligned(16))) float lds[(G * PIN_MAX + 1) * LD];
    const int so = (sin + 1) / 2, pin = sin * sin, pout = so * so;
    const int64_t item0 = (int64_t)blockIdx.x * G;
    const int live = (int)(n_items - item0 < G ? n_items - item0 : G);
    const int tid = threadIdx.x;
    mfma_conv::stage_rows<CIN, 512>(lds, in + (size_t)item0 * pin * CIN, live * pin, tid);       // contiguous over the live items
    mfma_conv::fill_zero_row<512>(lds, ZR, LD, tid);
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int nt = wave % TN, mt = wave / TN;
    const int rows = live * pout;
    if (mt * 32 >= rows) return;                                    // (wave-uniform; no barrier follows)
    const int r = mt * 32 + j;
    const bool rv = r < rows;
    const int g = rv ? r / pout : 0, pq = rv ? r - g * pout : 0;
    const int oy = pq / so, ox = pq - oy * so;
    const int co = nt * 32 + j;
    f32x16 acc[1];
    mfma_conv::clear(acc);
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const float *ap[1] = {mfma_conv::tap_row(lds, LD, ZR, rv, g, 2 * oy - 1 + ky, 2 * ox - 1 + kx, sin, pin, h)};
        const float4 *bp = reinterpret_cast<const float4 *>(wp) + ((size_t)tap * (CIN / 4) + h) * COUT + co;
        mfma_conv::k_chain<1, 4>(acc, ap, bp, CIN / 8, COUT);
    }
    const float scale = sc[co], shift = sh[co];
    float *dst = out + (size_t)item0 * pout * COUT;                 // row r of the workgroup = (item, pixel), contiguous too
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int ro = mfma_conv::acc_row(q, h, mt * 32);
        if (ro < rows) {
            const float v = fmaf(scale, acc[0][q], shift);
            dst[(unsigned)(ro * COUT + co)] = v > 0.f ? v : 0.f;     // (32-bit: the store keeps dst as its scalar base)
        }
    }
}

// ---- the heads: out[row][col] = bh[col] + sum over segments s (in order) of (sum over k < E3 of a[row][s E3 + k] whp[s][k][col]),
// a = the last activation as a matrix [n_rows][nseg E3].  A workgroup = 32 rows x every column: 4 waves, wave w takes the
// column tiles w and w + 4.  Per segment the 32 rows' E3 values are staged in LDS (rows padded by four floats), each wave runs
// one chain from 0 per tile over them and adds it to its running sum: the 4096-term vanilla head is 16 chains of 256 added in
// pixel order, not one chain.  whp: [segment][E3 / 4][npad][4], npad = 2 d rounded up to 32 (zero columns above 2 d); columns
// 0 .. d-1 are mu, d .. 2d-1 logvar.  Row = item * pix + pixel; element (item, col, pixel) goes to [item][col][pixel]
// (pix = 1: [n][d]; pix = 16: NCHW [n][d][4][4]).
template <int E3>
__global__ __launch_bounds__(256) void enc_head_kernel(const float *__restrict__ a, int64_t n_rows, int nseg, int d, int npad, int pix,
                                                       const float *__restrict__ whp, const float *__restrict__ bh,
                                                       float *__restrict__ mu, float *__restrict__ logvar) {
    constexpr int LD = E3 + 4;
    __shared__ __attribute__((aligned(16))) float lds[HEAD_ROWS * LD];
    const int64_t row0 = (int64_t)blockIdx.x * HEAD_ROWS;
    const int live = (int)(n_rows - row0 < HEAD_ROWS ? n_rows - row0 : HEAD_ROWS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int ntiles = npad / 32;
    const bool two = wave + 4 < ntiles;
    const int col0 = wave * 32 + j, col1 = col0 + 128;
    const size_t ktot = (size_t)nseg * E3;
    f32x16 tot0, tot1;
#pragma unroll
    for (int q = 0; q < 16; ++q) { tot0[q] = 0.f; tot1[q] = 0.f; }
    for (int s = 0; s < nseg; ++s) {
        __syncthreads();
        for (int q = tid; q < HEAD_ROWS * (E3 / 4); q += 256) {
            const int row = q / (E3 / 4), ci = (q - row * (E3 / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < live) v = *reinterpret_cast<const float4 *>(a + (size_t)(row0 + row) * ktot + (size_t)s * E3 + ci);
            *reinterpret_cast<float4 *>(lds + (size_t)row * LD + ci) = v;
        }
        __syncthreads();
        if (wave < ntiles) {
            f32x16 acc0, acc1;
#pragma unroll
            for (int q = 0; q < 16; ++q) { acc0[q] = 0.f; acc1[q] = 0.f; }
            const float *ap = lds + (size_t)j * LD + 4 * h;
            const float4 *bp = reinterpret_cast<const float4 *>(whp) + ((size_t)s * (E3 / 4) + h) * npad;
#pragma unroll 2
            for (int cb = 0; cb < E3 / 8; ++cb) {
                const float4 av = *reinterpret_cast<const float4 *>(ap + cb * 8);
                const float4 b0 = bp[(size_t)cb * 2 * npad + col0];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0.x, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b0.y, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b0.z, acc0, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b0.w, acc0, 0, 0, 0);
                if (two) {
                    const float4 b1 = bp[(size_t)cb * 2 * npad + col1];
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b1.x, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1.y, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b1.z, acc1, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b1.w, acc1, 0, 0, 0);
                }
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) { tot0[q] += acc0[q]; tot1[q] += acc1[q]; }
        }
    }
    if (wave >= ntiles) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (t == 1 && !two) break;
        const int col = t ? col1 : col0;
        if (col >= 2 * d) continue;
        const float bias = bh[col];
        float *dst = col < d ? mu : logvar;
        const int c = col < d ? col : col - d;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int ro = mfma_conv::acc_row(q, h);
            if (ro < live) {
                const int64_t row = row0 + ro, item = row / pix;
                const int p = (int)(row - item * pix);
                dst[((size_t)item * d + c) * pix + p] = (t ? tot1[q] : tot0[q]) + bias;
            }
        }
    }
}

template <int E1, int E2, int E3>
int run_pass(const geo_image_encoder_desc *e, const Shape &s, const float *x, int64_t cnt, float *buf1, float *buf2, float *buf3,
             float *mu, float *logvar, hipStream_t st) {
    constexpr int G2 = 64 / E1, G3 = 256 / E2;     // items per workgroup: 1 | 2 (layer 2), 2 | 4 (layer 3)
    if (s.C == 1)
        enc_first_kernel<1, 28, E1><<<(unsigned)cnt, 256, 0, st>>>(x, buf1, e->w1p, e->scale1, e->shift1);
    else
        enc_first_kernel<3, 32, E1><<<(unsigned)cnt, 256, 0, st>>>(x, buf1, e->w1p, e->scale1, e->shift1);
    GEO_LAUNCH_CHECK();
    enc_conv_kernel<E1, E2, G2, 256><<<(unsigned)((cnt + G2 - 1) / G2), 512, 0, st>>>(buf1, buf2, cnt, s.S / 2, e->w2p, e->scale2,
                                                                                     e->shift2);
    GEO_LAUNCH_CHECK();
    enc_conv_kernel<E2, E3, G3, 64><<<(unsigned)((cnt + G3 - 1) / G3), 512, 0, st>>>(buf2, buf3, cnt, s.S / 4, e->w3p, e->scale3,
                                                                                    e->shift3);
    GEO_LAUNCH_CHECK();
    const int64_t rows = s.spatial ? cnt * 16 : cnt;
    enc_head_kernel<E3><<<(unsigned)((rows + HEAD_ROWS - 1) / HEAD_ROWS), 256, 0, st>>>(buf3, rows, s.spatial ? 1 : 16, s.d, s.npad,
                                                                                         s.spatial ? 16 : 1, e->whp, e->bh, mu, logvar);
    GEO_LAUNCH_CHECK();
    return GEO_OK;
}

}  // namespace

extern "C" size_t geo_image_encode_workspace_bytes(const geo_image_encoder_desc *enc, int64_t n) {
    Shape s;
    if (!make_shape(enc, &s) || n < 0) return 0;
    return geo::pass_query_bytes(s.per_item, 3, ITEMS_PER_PASS, n);
}

extern "C" int geo_image_encode(const geo_image_encoder_desc *enc, const float *x, int64_t n, float *mu_out, float *logvar_out,
                                void *ws, size_t ws_bytes, void *stream) {
    Shape s;
    GEO_REQUIRE(make_shape(enc, &s), "geo_image_encode: encoder configuration not covered (see geo_hip.h)");
    GEO_REQUIRE(enc->w1p && enc->scale1 && enc->shift1 && enc->w2p && enc->scale2 && enc->shift2 && enc->w3p && enc->scale3 &&
                    enc->shift3 && enc->whp && enc->bh,
                "geo_image_encode: null pointer in the descriptor");
    GEO_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "geo_image_encode: n %lld", (long long)n);
    if (n == 0) return GEO_OK;
    GEO_REQUIRE(x && mu_out && logvar_out && ws, "geo_image_encode: null pointer");
    int64_t pb;
    float *buf[3];
    int rc = geo::plan_passes("geo_image_encode", s.per_item, 3, ITEMS_PER_PASS, n, ws, ws_bytes, &pb, buf);
    if (rc != GEO_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t nin = (size_t)s.C * s.S * s.S, nout = (size_t)s.d * (s.spatial ? 16 : 1);
    for (int64_t p0 = 0; p0 < n; p0 += pb) {
        const int64_t cnt = n - p0 < pb ? n - p0 : pb;
        if (s.e1 == 64)
            rc = run_pass<64, 128, 256>(enc, s, x + (size_t)p0 * nin, cnt, buf[0], buf[1], buf[2], mu_out + (size_t)p0 * nout,
                                        logvar_out + (size_t)p0 * nout, st);
        else
            rc = run_pass<32, 64, 128>(enc, s, x + (size_t)p0 * nin, cnt, buf[0], buf[1], buf[2], mu_out + (size_t)p0 * nout,
                                       logvar_out + (size_t)p0 * nout, st);
        if (rc != GEO_OK) return rc;
    }
    return GEO_OK;
}
