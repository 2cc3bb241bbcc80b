// batch.hip -- one training batch, float32 NCHW and normalised, straight from the resident uint8 NHWC images on gfx950
// (ToTensor -> [RandomCrop(H, padding=pad) -> RandomHorizontalFlip] -> Normalize of the reference's src/data/factory.py).
//
//   out[b][c][y][x] = ((p * fl32(1 / 255)) - mean[c]) / std[c]          p = u8[rows[b]][sy][sx][c], 0 outside the image
//   sy = y + oy - pad,   sx = (flip[b] ? W - 1 - x : x) + ox - pad;   offset == NULL: (oy, ox) = (pad, pad); flip == NULL: none
//
// Arithmetic.  Three float32 operations, each rounded to nearest on its own: the product, the difference, the quotient.
// These are the operations torch runs on the device for `x.to(float32).div(255).sub_(mean).div_(std)` -- its division of a
// tensor by a host scalar is the product with the float32 reciprocal of that scalar, its division by a tensor is the
// IEEE quotient -- and the batch has to equal that expression bit for bit (training/data.py keeps the torch path next to
// this one).  Contraction is switched off for the whole file: the product and the difference must not become one fma.
//
// Mapping.  A lane produces XPL = 4 consecutive x of one (b, c, y) output row; consecutive lanes take consecutive groups of a
// row, then the next row, so with W % 4 == 0 a wave stores 1 KiB of contiguous output as 16-byte vectors.  Any other W takes
// the same kernel with scalar stores and a partial last group.  The reads are byte gathers with stride C from one NHWC image
// row; the C lanes that need the same bytes for the other channels find them in the cache.  No LDS, no atomics, no
// synchronisation: 1 byte read and 4 bytes written per element.
#include "geo_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = 256;
constexpr int XPL = 4;

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void batch_assemble_kernel(const uint8_t *__restrict__ u8, int64_t N, int H, int W, int C,
                                                               const int64_t *__restrict__ rows,
                                                               const int32_t *__restrict__ offset,
                                                               const uint8_t *__restrict__ flip, int pad,
                                                               const float *__restrict__ mean, const float *__restrict__ stdv,
                                                               float *__restrict__ out, int Wg, uint32_t total) {
    const float inv255 = 1.0f / 255.0f;
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < total; i += gridDim.x * BLOCK) {
        const uint32_t g = i % Wg, r = i / Wg;                 // r = (b C + c) H + y: the output row
        const uint32_t y = r % H, bc = r / H;
        const uint32_t c = bc % C, b = bc / C;
        const int64_t row = rows[b];
        const int oy = offset ? offset[2 * b] : pad, ox = offset ? offset[2 * b + 1] : pad;
        const bool mirror = flip && flip[b];
        const int sy = (int)y + oy - pad;
        // an index outside [0, N) reads nothing: the callers check theirs on the host, this keeps a wrong one inside the buffer
        const bool row_ok = row >= 0 && row < N && sy >= 0 && sy < H;
        const int64_t src = row_ok ? ((row * H + sy) * (int64_t)W) * C + c : 0;
        const float m = mean[c], s = stdv[c];
        const int x0 = (int)g * XPL;
        float v[XPL];
#pragma unroll
        for (int k = 0; k < XPL; ++k) {
            const int x = x0 + k;
            const int sx = (mirror ? W - 1 - x : x) + ox - pad;
            uint8_t p = 0;
            if (row_ok && x < W && sx >= 0 && sx < W) p = u8[src + (int64_t)sx * C];
            v[k] = ((float)p * inv255 - m) / s;
        }
        float *dst = out + (int64_t)r * W + x0;
        if (VEC) {
            *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < XPL; ++k)
                if (x0 + k < W) dst[k] = v[k];
        }
    }
}

}  // namespace

extern "C" int geo_batch_assemble(const uint8_t *u8, int64_t N, int32_t H, int32_t W, int32_t C, const int64_t *rows, int32_t B,
                                  const int32_t *offset, const uint8_t *flip, int32_t pad, const float *mean, const float *std,
                                  float *out, void *stream_) {
    GEO_REQUIRE(u8 && rows && mean && std && out, "geo_batch_assemble: null pointer");
    GEO_REQUIRE(N >= 1 && B >= 1, "geo_batch_assemble: N=%lld B=%d", (long long)N, B);
    GEO_REQUIRE(C >= 1 && C <= 4 && H >= 1 && H <= 256 && W >= 1 && W <= 256 && pad >= 0 && pad <= 16,
                "geo_batch_assemble: limits are 1 <= C <= 4, 1 <= H, W <= 256, 0 <= pad <= 16; got C=%d H=%d W=%d pad=%d", C, H, W,
                pad);
    const int Wg = (W + XPL - 1) / XPL;
    const int64_t total = (int64_t)B * C * H * Wg;
    GEO_REQUIRE(total < (int64_t(1) << 31), "geo_batch_assemble: B C H ceil(W / 4) = %lld, limit 2^31", (long long)total);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid(geo::grid_for(total, BLOCK, 1 << 16));
    const bool vec = W % XPL == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(batch_assemble_kernel<true>, grid, dim3(BLOCK), 0, stream, u8, N, (int)H, (int)W, (int)C, rows, offset,
                           flip, (int)pad, mean, std, out, Wg, (uint32_t)total);
    else
        hipLaunchKernelGGL(batch_assemble_kernel<false>, grid, dim3(BLOCK), 0, stream, u8, N, (int)H, (int)W, (int)C, rows, offset,
                           flip, (int)pad, mean, std, out, Wg, (uint32_t)total);
    GEO_LAUNCH_CHECK();
    return 0;
}
