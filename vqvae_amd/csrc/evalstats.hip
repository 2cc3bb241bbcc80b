// evalstats.hip -- per-image pair moments for the evaluation metrics (PSNR, SSIM) on gfx950.
//
// geo_image_pair_moments: for each image pair (x_i, y_i) of n_pix float32 values, in fp64,
//   mean_x, mean_y                      = sum / n_pix
//   var_x, var_y, cov_xy                = sum of (x - mean_x)^2, (y - mean_y)^2, (x - mean_x)(y - mean_y), over n_pix
//   sse                                 = sum of (x - y)^2
// The second-order moments are centred on the fp64 means (two passes over the values each lane keeps in registers), never
// sum x^2 - (sum x)^2 / n: the centred form loses nothing to cancellation when the variance is small against the mean.
//
// Launch shape.  An image is handled by a team of W = ceil(n_pix / 1024) waves; each lane keeps at most 16 values of x and 16
// of y (W <= 16 because n_pix <= 16384).  W == 1 (n_pix <= 1024, e.g. a 784-pixel FashionMNIST image): four images per
// 256-lane workgroup, one wave each.  W > 1: one workgroup of 64 W lanes per image.  Loads are float4 when n_pix % 4 == 0 and
// both bases are 16-byte aligned (the team's lanes take consecutive float4 chunks, slot by slot), scalar otherwise.
//
// Determinism.  No atomics.  Every sum has one association fixed by n_pix alone: each lane adds its own values in slot order,
// the wave folds its 64 partials with an xor butterfly (offsets 32, 16, ..., 1; both partners form the same sum, since fp
// addition commutes, so every lane ends with the wave total), and the W wave totals go through LDS and are added in wave
// order by every lane.  An image's moments therefore do not depend on n_images, on where the image sits in the batch or the
// workgroup, on the stream or on the run.
#include "geo_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int PER_LANE = 16;                            // values of x (and of y) one lane keeps
constexpr int MAX_PIX = 16384;
constexpr int MAX_WAVES = MAX_PIX / (WAVE * PER_LANE);  // 16
constexpr int SMALL_IMAGES_PER_BLOCK = 4;               // W == 1: one image per wave, four waves per workgroup

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// Sum of the team's per-lane partials v[0..N), returned to every lane.  W == 1: the butterfly alone.  W > 1: the wave totals
// go to red[.][wave] and every lane adds them in wave order (one barrier; the caller's rows of `red` are not reused).
template <int N>
__device__ __forceinline__ void team_sum(double (&v)[N], int W, int wave, int lane, double (*red)[MAX_WAVES]) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
    if (W == 1) return;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double s = red[k][0];
        for (int w = 1; w < W; ++w) s += red[k][w];
        v[k] = s;
    }
}

template <bool VEC>
__global__ __launch_bounds__(1024) void pair_moments_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                            int64_t n_images, int n_pix, int W, double *__restrict__ out) {
    __shared__ double red[6][MAX_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t img = W == 1 ? (int64_t)blockIdx.x * SMALL_IMAGES_PER_BLOCK + wave : (int64_t)blockIdx.x;
    if (img >= n_images) return;                        // W == 1 only (no barrier on that path); W > 1 grids are exact
    const int team_lane = W == 1 ? lane : (int)threadIdx.x;
    const int L = WAVE * W;                             // lanes of the team
    const float *xi = x + img * n_pix, *yi = y + img * n_pix;

    float xv[PER_LANE], yv[PER_LANE];
    if constexpr (VEC) {
        const int n4 = n_pix / 4;
#pragma unroll
        for (int s = 0; s < PER_LANE / 4; ++s) {
            const int c = s * L + team_lane;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (c < n4) {
                a = reinterpret_cast<const float4 *>(xi)[c];
                b = reinterpret_cast<const float4 *>(yi)[c];
            }
            xv[4 * s] = a.x, xv[4 * s + 1] = a.y, xv[4 * s + 2] = a.z, xv[4 * s + 3] = a.w;
            yv[4 * s] = b.x, yv[4 * s + 1] = b.y, yv[4 * s + 2] = b.z, yv[4 * s + 3] = b.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < PER_LANE; ++s) {
            const int e = s * L + team_lane;
            xv[s] = e < n_pix ? xi[e] : 0.f;
            yv[s] = e < n_pix ? yi[e] : 0.f;
        }
    }
    // value j of this lane is element index_of(j); it exists iff index_of(j) < n_pix
    auto valid = [&](int j) {
        const int e = VEC ? ((j / 4) * L + team_lane) * 4 + (j % 4) : j * L + team_lane;
        return e < n_pix;
    };

    const double n = (double)n_pix;
    double s1[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        s1[0] += (double)xv[j];                          // padding values are 0.f: they add exact zeros
        s1[1] += (double)yv[j];
    }
    team_sum(s1, W, wave, lane, red);
    const double mx = s1[0] / n, my = s1[1] / n;

    double s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        if (!valid(j)) continue;
        const double dx = (double)xv[j] - mx, dy = (double)yv[j] - my, d = (double)xv[j] - (double)yv[j];
        s2[0] = fma(dx, dx, s2[0]);
        s2[1] = fma(dy, dy, s2[1]);
        s2[2] = fma(dx, dy, s2[2]);
        s2[3] = fma(d, d, s2[3]);
    }
    team_sum(s2, W, wave, lane, red + 2);

    if (team_lane == 0) {
        double *o = out + img * 6;
        o[0] = mx;
        o[1] = my;
        o[2] = s2[0] / n;
        o[3] = s2[1] / n;
        o[4] = s2[2] / n;
        o[5] = s2[3];
    }
}

}  // namespace

extern "C" int geo_image_pair_moments(const float *x, const float *y, int64_t n_images, int64_t n_pix, double *mom_out,
                                      void *stream_) {
    GEO_REQUIRE(x && y && mom_out, "geo_image_pair_moments: null pointer");
    GEO_REQUIRE(n_pix >= 1 && n_pix <= MAX_PIX, "geo_image_pair_moments: n_pix %lld outside [1, %d]", (long long)n_pix,
                MAX_PIX);
    GEO_REQUIRE(n_images >= 0 && n_images <= INT32_MAX, "geo_image_pair_moments: n_images %lld outside [0, 2^31)",
                (long long)n_images);
    if (n_images == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int P = static_cast<int>(n_pix);
    const int W = (P + WAVE * PER_LANE - 1) / (WAVE * PER_LANE);
    const dim3 block(W == 1 ? WAVE * SMALL_IMAGES_PER_BLOCK : WAVE * W);
    const dim3 grid(W == 1 ? static_cast<unsigned>((n_images + SMALL_IMAGES_PER_BLOCK - 1) / SMALL_IMAGES_PER_BLOCK)
                           : static_cast<unsigned>(n_images));
    const bool vec = P % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
    if (vec) hipLaunchKernelGGL(pair_moments_kernel<true>, grid, block, 0, stream, x, y, n_images, P, W, mom_out);
    else hipLaunchKernelGGL(pair_moments_kernel<false>, grid, block, 0, stream, x, y, n_images, P, W, mom_out);
    GEO_LAUNCH_CHECK();
    return 0;
}
