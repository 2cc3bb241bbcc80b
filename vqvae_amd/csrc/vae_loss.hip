// vae_loss.hip -- the vanilla VAE's ELBO (reference src/models/vae.py:130-198) as one forward pair and one backward kernel on
// gfx950.
//
// Forward.  out f64 [4] = total, recon, kl, regulated kl, with
//   recon = (1 / B) sum over [B][P] of   BCE   max(l, 0) - l x + log1p(exp(-|l|))
//                                        MSE   (sigmoid(l) - x)^2   or   (l - x)^2
//   kl    = (1 / B) sum over [B][d] of   max(k, free_bits),   k = -0.5 (1 + logvar - mu^2 - exp(logvar))
//   reg   = kl | |kl - target| | max(kl - target, 0)          total = recon + beta reg
// Every term is formed in fp64 from the float32 inputs.  elbo_partials_kernel: workgroups [0, Gr) stride over the B P
// reconstruction terms, workgroups [Gr, Gr + Gk) over the B d KL terms, each leaving ONE fp64 partial in the workspace;
// elbo_finish_kernel (one workgroup) adds the partials and writes out.
//
// Determinism.  No atomics.  Gr and Gk depend on the element counts alone.  A lane adds its terms in index order, a wave folds
// its 64 partials with an xor butterfly (both partners form the same sum), the four wave totals are added in wave order, the
// finish kernel's lanes add partials g = lane, lane + 256, ... in that order and fold the same way: one association per
// (B, P, d), so out is bit-identical across runs and streams.
//
// Backward.  elbo_backward_kernel reads the upstream gradient g (f64, device) and the forward's out (sign of kl - target)
// and writes, rounded once from fp64 to f32,
//   d x_logits = (g / B)   (sigmoid(l) - x)  |  2 (s - x) s (1 - s)  |  2 (l - x)
//   d mu       = (g beta c / B) m mu            d logvar = (g beta c / B) m 0.5 (exp(logvar) - 1)
// m = 1 without free bits, else [k >= free_bits]: torch.clamp(min=)'s backward passes the gradient at equality.  c = 1 (capacity
// off), sign(kl - target) with 0 at 0 (abs: torch.abs's subgradient), [kl - target >= 0] (clipped: torch.clamp(min=0) again).
// k is evaluated by the same device function in both directions, so mask and clamp agree.
//
// Both directions are memory-bound streams (float4 when B P % 4 == 0 and the bases are 16-byte aligned): forward reads
// 8 B P bytes, backward reads 8 B P and writes 4 B P.
#include "geo_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / WAVE;
constexpr int MAX_GRID = 4096;       // partials per part; a workgroup then strides over >= 1 float4 per lane

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
    return v;
}

// Sum of the workgroup's 256 per-lane values, returned to every lane: butterfly per wave, wave totals added in wave order.
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = wave_sum(v);
    if (threadIdx.x % WAVE == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w];
    __syncthreads();                                    // red may be reused by the caller
    return s;
}

__device__ __forceinline__ double sigmoid64(double l) {
    // no overflow for either sign: exp of a non-positive argument only
    const double e = exp(-fabs(l));
    return l >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

template <int MODE>
__device__ __forceinline__ double recon_term(float lf, float xf) {
    const double l = (double)lf, x = (double)xf;
    if constexpr (MODE == GEO_VAE_RECON_BCE) {
        return fmax(l, 0.0) - l * x + log1p(exp(-fabs(l)));
    } else if constexpr (MODE == GEO_VAE_RECON_MSE_SIGMOID) {
        const double d = sigmoid64(l) - x;
        return d * d;
    } else {
        const double d = l - x;
        return d * d;
    }
}

template <int MODE>
__device__ __forceinline__ float recon_grad(float lf, float xf, double scale) {
    const double l = (double)lf, x = (double)xf;
    if constexpr (MODE == GEO_VAE_RECON_BCE) {
        return (float)(scale * (sigmoid64(l) - x));
    } else if constexpr (MODE == GEO_VAE_RECON_MSE_SIGMOID) {
        const double s = sigmoid64(l);
        return (float)(scale * (2.0 * (s - x) * (s * (1.0 - s))));
    } else {
        return (float)(scale * (2.0 * (l - x)));
    }
}

// KL of one latent dimension, in the reference's operation order (mu^2 of a float32 is exact in fp64).
__device__ __forceinline__ double kl_dim(float muf, float lvf) {
    const double mu = (double)muf, lv = (double)lvf;
    return -0.5 * (((1.0 + lv) - mu * mu) - exp(lv));
}

static inline int part_grid(int64_t items_per_lane_unit) {
    return geo::grid_for(items_per_lane_unit, BLOCK, MAX_GRID);
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(BLOCK) void elbo_partials_kernel(const float *__restrict__ logits, const float *__restrict__ x,
                                                              const float *__restrict__ mu, const float *__restrict__ logvar,
                                                              int64_t n_rec, int64_t n_lat, int has_free_bits, double free_bits,
                                                              int Gr, int Gk, double *__restrict__ partials) {
    __shared__ double red[WAVES];
    double acc = 0.0;
    if ((int)blockIdx.x < Gr) {
        const int64_t stride = (int64_t)Gr * BLOCK;
        if constexpr (VEC) {
            const int64_t n4 = n_rec / 4;
            for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n4; i += stride) {
                const float4 l = reinterpret_cast<const float4 *>(logits)[i];
                const float4 t = reinterpret_cast<const float4 *>(x)[i];
                acc += recon_term<MODE>(l.x, t.x);
                acc += recon_term<MODE>(l.y, t.y);
                acc += recon_term<MODE>(l.z, t.z);
                acc += recon_term<MODE>(l.w, t.w);
            }
        } else {
            for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_rec; i += stride)
                acc += recon_term<MODE>(logits[i], x[i]);
        }
    } else {
        const int b = (int)blockIdx.x - Gr;
        const int64_t stride = (int64_t)Gk * BLOCK;
        for (int64_t i = (int64_t)b * BLOCK + threadIdx.x; i < n_lat; i += stride) {
            const double k = kl_dim(mu[i], logvar[i]);
            acc += has_free_bits ? fmax(k, free_bits) : k;
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(BLOCK) void elbo_finish_kernel(const double *__restrict__ partials, int Gr, int Gk, double inv_B,
                                                            double beta, double target, int capacity_mode,
                                                            double *__restrict__ out) {
    __shared__ double red[WAVES];
    double a = 0.0, b = 0.0;
    for (int g = threadIdx.x; g < Gr; g += BLOCK) a += partials[g];
    for (int g = threadIdx.x; g < Gk; g += BLOCK) b += partials[Gr + g];
    const double recon = block_sum(a, red) * inv_B;
    const double kl = block_sum(b, red) * inv_B;
    if (threadIdx.x == 0) {
        double reg = kl;
        if (capacity_mode == GEO_VAE_CAPACITY_ABS) reg = fabs(kl - target);
        else if (capacity_mode == GEO_VAE_CAPACITY_CLIPPED) reg = fmax(kl - target, 0.0);
        out[0] = recon + beta * reg;
        out[1] = recon;
        out[2] = kl;
        out[3] = reg;
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(BLOCK) void elbo_backward_kernel(const double *__restrict__ g_total, const double *__restrict__ out,
                                                              const float *__restrict__ logits, const float *__restrict__ x,
                                                              const float *__restrict__ mu, const float *__restrict__ logvar,
                                                              int64_t n_rec, int64_t n_lat, double inv_B, int has_free_bits,
                                                              double free_bits, double beta, double target, int capacity_mode,
                                                              int Gr, int Gk, float *__restrict__ d_logits,
                                                              float *__restrict__ d_mu, float *__restrict__ d_logvar) {
    const double g = g_total[0];
    if ((int)blockIdx.x < Gr) {
        const double scale = g * inv_B;
        const int64_t stride = (int64_t)Gr * BLOCK;
        if constexpr (VEC) {
            const int64_t n4 = n_rec / 4;
            for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n4; i += stride) {
                const float4 l = reinterpret_cast<const float4 *>(logits)[i];
                const float4 t = reinterpret_cast<const float4 *>(x)[i];
                float4 r;
                r.x = recon_grad<MODE>(l.x, t.x, scale);
                r.y = recon_grad<MODE>(l.y, t.y, scale);
                r.z = recon_grad<MODE>(l.z, t.z, scale);
                r.w = recon_grad<MODE>(l.w, t.w, scale);
                reinterpret_cast<float4 *>(d_logits)[i] = r;
            }
        } else {
            for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_rec; i += stride)
                d_logits[i] = recon_grad<MODE>(logits[i], x[i], scale);
        }
    } else {
        double c = 1.0;
        const double diff = out[2] - target;
        if (capacity_mode == GEO_VAE_CAPACITY_ABS) c = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
        else if (capacity_mode == GEO_VAE_CAPACITY_CLIPPED) c = diff >= 0.0 ? 1.0 : 0.0;
        const double scale = g * beta * c * inv_B;
        const int b = (int)blockIdx.x - Gr;
        const int64_t stride = (int64_t)Gk * BLOCK;
        for (int64_t i = (int64_t)b * BLOCK + threadIdx.x; i < n_lat; i += stride) {
            const float m = mu[i], lv = logvar[i];
            const bool pass = !has_free_bits || kl_dim(m, lv) >= free_bits;
            d_mu[i] = pass ? (float)(scale * (double)m) : 0.f;
            d_logvar[i] = pass ? (float)(scale * (0.5 * (exp((double)lv) - 1.0))) : 0.f;
        }
    }
}

struct Shape {
    int64_t n_rec, n_lat;
    int Gr, Gk;
};

static inline bool shape_of(int64_t B, int64_t P, int64_t d, Shape &s) {
    if (B < 1 || P < 1 || d < 1 || B > INT32_MAX || P > INT32_MAX || d > INT32_MAX) return false;
    if (P > INT64_MAX / B || d > INT64_MAX / B) return false;
    s.n_rec = B * P;
    s.n_lat = B * d;
    s.Gr = part_grid((s.n_rec + 3) / 4);               // one float4 (or four scalars' worth of stride) per lane and pass
    s.Gk = part_grid(s.n_lat);
    return true;
}

static inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" size_t geo_vae_elbo_workspace_bytes(int64_t B, int64_t P, int64_t d) {
    Shape s;
    if (!shape_of(B, P, d, s)) return 0;
    return geo::align_up(static_cast<size_t>(s.Gr + s.Gk) * sizeof(double));
}

#define GEO_VAE_DISPATCH(KERNEL, ...)                                                                              \
    do {                                                                                                           \
        if (recon_mode == GEO_VAE_RECON_BCE) {                                                                     \
            if (vec) hipLaunchKernelGGL((KERNEL<GEO_VAE_RECON_BCE, true>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);  \
            else hipLaunchKernelGGL((KERNEL<GEO_VAE_RECON_BCE, false>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);     \
        } else if (recon_mode == GEO_VAE_RECON_MSE_SIGMOID) {                                                      \
            if (vec) hipLaunchKernelGGL((KERNEL<GEO_VAE_RECON_MSE_SIGMOID, true>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);  \
            else hipLaunchKernelGGL((KERNEL<GEO_VAE_RECON_MSE_SIGMOID, false>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);     \
        } else {                                                                                                   \
            if (vec) hipLaunchKernelGGL((KERNEL<GEO_VAE_RECON_MSE_LOGITS, true>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);   \
            else hipLaunchKernelGGL((KERNEL<GEO_VAE_RECON_MSE_LOGITS, false>), grid, dim3(BLOCK), 0, stream, __VA_ARGS__);      \
        }                                                                                                          \
    } while (0)

static int check_common(const char *who, int32_t recon_mode, int32_t has_free_bits, double free_bits, int32_t capacity_mode) {
    GEO_REQUIRE(recon_mode >= GEO_VAE_RECON_BCE && recon_mode <= GEO_VAE_RECON_MSE_LOGITS, "%s: recon_mode %d outside [0, 2]",
                who, recon_mode);
    GEO_REQUIRE(capacity_mode >= GEO_VAE_CAPACITY_OFF && capacity_mode <= GEO_VAE_CAPACITY_CLIPPED,
                "%s: capacity_mode %d outside [0, 2]", who, capacity_mode);
    GEO_REQUIRE(!has_free_bits || free_bits == free_bits, "%s: free_bits is NaN", who);
    return 0;
}

extern "C" int geo_vae_elbo_forward(const float *x_logits, const float *x, const float *mu, const float *logvar, int64_t B,
                                    int64_t P, int64_t d, int32_t recon_mode, int32_t has_free_bits, double free_bits,
                                    double beta, double capacity_target, int32_t capacity_mode, double *out, void *ws,
                                    size_t ws_bytes, void *stream_) {
    GEO_REQUIRE(x_logits && x && mu && logvar && out && ws, "geo_vae_elbo_forward: null pointer");
    Shape s;
    GEO_REQUIRE(shape_of(B, P, d, s), "geo_vae_elbo_forward: B=%lld P=%lld d=%lld outside [1, 2^31)", (long long)B, (long long)P,
                (long long)d);
    if (int e = check_common("geo_vae_elbo_forward", recon_mode, has_free_bits, free_bits, capacity_mode)) return e;
    GEO_REQUIRE(ws_bytes >= geo_vae_elbo_workspace_bytes(B, P, d), "geo_vae_elbo_forward: workspace of %zu bytes, need %zu",
                ws_bytes, geo_vae_elbo_workspace_bytes(B, P, d));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    double *partials = static_cast<double *>(ws);
    const bool vec = s.n_rec % 4 == 0 && aligned16(x_logits) && aligned16(x);
    const dim3 grid(static_cast<unsigned>(s.Gr + s.Gk));
    GEO_VAE_DISPATCH(elbo_partials_kernel, x_logits, x, mu, logvar, s.n_rec, s.n_lat, (int)has_free_bits, free_bits, s.Gr, s.Gk,
                     partials);
    GEO_LAUNCH_CHECK();
    hipLaunchKernelGGL(elbo_finish_kernel, dim3(1), dim3(BLOCK), 0, stream, partials, s.Gr, s.Gk, 1.0 / (double)B, beta,
                       capacity_target, (int)capacity_mode, out);
    GEO_LAUNCH_CHECK();
    return 0;
}

extern "C" int geo_vae_elbo_backward(const double *grad_total, const double *out, const float *x_logits, const float *x,
                                     const float *mu, const float *logvar, int64_t B, int64_t P, int64_t d, int32_t recon_mode,
                                     int32_t has_free_bits, double free_bits, double beta, double capacity_target,
                                     int32_t capacity_mode, float *d_logits, float *d_mu, float *d_logvar, void *stream_) {
    GEO_REQUIRE(grad_total && out && x_logits && x && mu && logvar && d_logits && d_mu && d_logvar,
                "geo_vae_elbo_backward: null pointer");
    Shape s;
    GEO_REQUIRE(shape_of(B, P, d, s), "geo_vae_elbo_backward: B=%lld P=%lld d=%lld outside [1, 2^31)", (long long)B, (long long)P,
                (long long)d);
    if (int e = check_common("geo_vae_elbo_backward", recon_mode, has_free_bits, free_bits, capacity_mode)) return e;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const bool vec = s.n_rec % 4 == 0 && aligned16(x_logits) && aligned16(x) && aligned16(d_logits);
    const dim3 grid(static_cast<unsigned>(s.Gr + s.Gk));
    GEO_VAE_DISPATCH(elbo_backward_kernel, grad_total, out, x_logits, x, mu, logvar, s.n_rec, s.n_lat, 1.0 / (double)B,
                     (int)has_free_bits, free_bits, beta, capacity_target, (int)capacity_mode, s.Gr, s.Gk, d_logits, d_mu,
                     d_logvar);
    GEO_LAUNCH_CHECK();
    return 0;
}
