// mfma_conv.h -- the K-quad implicit-GEMM convolution core that encode.hip, lpips.hip and vanilla_jvp.hip share (device only;
// DESIGN.md section 20 defines the format once).
//
//   instruction   v_mfma_f32_32x32x2_f32, exact f32: lane = (j = lane & 31, h = lane >> 5) supplies A[row j][k = h] and
//                 B[k = h][column j]; accumulator entry q of the lane is tile row acc_row(q, h), column j
//   A             activations channels-last in LDS, one row per (item, pixel), rows padded by four floats (conflict-free
//                 16-byte reads), plus ONE row of zeros that a tap in the padding, or a row past the last item, reads
//   B             weights packed [...][K / 4][N][4]: element (q, n, r) is weight (k = 4 q + r, column n), so a lane's 16-byte
//                 read is four consecutive k of its column and consecutive lanes read consecutive columns
//   K chain       over (tap, 8-channel block) from 0.  In a block lane half h takes channels 4 h .. 4 h + 3: one 16-byte read
//                 of B and one of A per M tile feed four MFMAs, so a value's chain adds the block's channels in the order
//                 0 4 1 5 2 6 3 7.  MT M tiles share the B read; within a block the m loop runs inside the B read
//
// The kernels keep what is their own: launch shape, which (tap, channel) ranges they chain, staging with masks, pooling or
// gathers, and the epilogue.
#pragma once
#include <hip/hip_runtime.h>

namespace mfma_conv {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// GEMM row of accumulator entry q (0 .. 15) in lane half h, for the 32-row tile that starts at row0.
__device__ __forceinline__ int acc_row(int q, int h, int row0 = 0) { return row0 + (q & 3) + 8 * (q >> 2) + 4 * h; }

// One 8-channel block: ap[m] points at the block's channel 4 h of tile m's A row, bv is the lane's B quad.
template <int MT>
__device__ __forceinline__ void k_block(f32x16 (&acc)[MT], const float *const (&ap)[MT], int cb, const float4 bv) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const float4 av = *reinterpret_cast<const float4 *>(ap[m] + cb * 8);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[m], 0, 0, 0);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[m], 0, 0, 0);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[m], 0, 0, 0);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[m], 0, 0, 0);
    }
}

// The chain over one tap's `blocks` 8-channel blocks.  ap[m]: tile m's A row at channel 4 h (tap_row); bp: the lane's B quad
// of block 0, i.e. packed weights + (q = h, n = column); n: the packed N.  (A kernel whose block count is not a compile-time
// constant writes this loop itself, without the unroll factor.)
template <int MT, int UNROLL>
__device__ __forceinline__ void k_chain(f32x16 (&acc)[MT], const float *const (&ap)[MT], const float4 *bp, int blocks, int n) {
#pragma unroll UNROLL
    for (int cb = 0; cb < blocks; ++cb) k_block<MT>(acc, ap, cb, bp[(size_t)cb * 2 * n]);
}

template <int MT>
__device__ __forceinline__ void clear(f32x16 (&acc)[MT]) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[m][q] = 0.f;
}

// The row of zeros: LDS row `zero_row` of `ld` floats, by NTHR threads (before the barrier that ends the staging).
template <int NTHR>
__device__ __forceinline__ void fill_zero_row(float *lds, int zero_row, int ld, int tid) {
    for (int k = tid; k < ld; k += NTHR) lds[(size_t)zero_row * ld + k] = 0.f;
}

// Plain staging: `rows` rows of C floats, contiguous in global memory, to LDS rows 0 .. rows - 1 of C + 4 floats.
template <int C, int NTHR>
__device__ __forceinline__ void stage_rows(float *lds, const float *src, int rows, int tid) {
    const float4 *s = reinterpret_cast<const float4 *>(src);
    for (int q = tid; q < rows * (C / 4); q += NTHR) {
        const int row = q / (C / 4), ci = (q - row * (C / 4)) * 4;
        *reinterpret_cast<float4 *>(lds + (size_t)row * (C + 4) + ci) = s[q];
    }
}

// The A row a tap reads, at lane half h's channel 4 h: input pixel (iy, ix) of item g when the GEMM row is valid and the pixel
// inside the side x side input of `pix` pixels, else the zero row.
__device__ __forceinline__ const float *tap_row(const float *lds, int ld, int zero_row, bool valid, int g, int iy, int ix, int side,
                                                int pix, int h) {
    const bool ok = valid && iy >= 0 && iy < side && ix >= 0 && ix < side;
    return lds + (size_t)(ok ? g * pix + iy * side + ix : zero_row) * ld + 4 * h;
}

}  // namespace mfma_conv
