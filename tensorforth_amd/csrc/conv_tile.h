// conv_tile.h - MFMA tile bodies the convolution engines share, written once (the conv counterpart of gemm_tile.h): __forceinline__ templates, instantiated
// only by the kernels of conv_big.hip and conv_geo.hip that launch them.  A kernel keeps what is its own - the tile decode, the gather addressing (its
// load_tiles / store_tiles) and the epilogue - and hands the body its callables:
//   conv_df_tile4   4 waves, 64 x 64 dF slab tile, both operands k-major, acc0 / acc1     k_convbig_df (conv_big.hip), k_geo_dft (conv_geo.hip)
// The summation order of these kernels is the body's: a change here changes all of its users alike.
// The other two pipelines - the 4-wave 128 x BN x 32 forward / dX tile of k_convbig and k_geo, the 8-wave LDS-DMA stage loops of k_convbig8 and
// k_convbig_dfw - and k_geo_df's copy of this one were tried on shared bodies too and stay written out in their kernels: inlined from a header they are
// scheduled differently, and rows of the timing A/B came out slower than the parent beyond the two spreads (profiles/conv_tile_ab.txt).
#pragma once
#include "conv_types.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));

// element r of a 32x32 MFMA accumulator in lane half h (= lane >> 5) is row frag_row(r, h), column lane & 31
__device__ __forceinline__ constexpr int frag_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ------------------------------------------------------------------ 4 waves, 64 x 64 dF slab tile, 32 pixels per stage
// Both operands k-major (k = the slice's pixels): A[k][m] and B[k][n] at pitch 64 floats; a wave's 32x32 block is summed on the accumulator PAIR
// acc0 (even k pairs) / acc1 (odd), added by the caller's epilogue.  load_tiles(kt) and store_tiles(buf) are the kernel's: how a stage reaches the
// registers, and how they are laid into the stage buffer sA + buf 32 64 | sB + buf 32 64
template <typename Load, typename Store>
__device__ __forceinline__ void conv_df_tile4(const float *sA, const float *sB, const int nst, f32x16 &acc0, f32x16 &acc1, Load &&load_tiles, Store &&store_tiles) {
    constexpr int BM = 64, BN = 64, BKP = 32;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wm = w >> 1, wn = w & 1, h = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }
    if (nst > 0) { load_tiles(0); store_tiles(0); }
    __syncthreads();
    for (int kt = 0; kt < nst; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nst) load_tiles(kt + 1);
        const float *a = sA + buf * BKP * BM, *b = sB + buf * BKP * BN;
        const int ra_ = wm * 32 + l31, rb_ = wn * 32 + l31;
#pragma unroll
        for (int ci = 0; ci < BKP / 8; ci++) {
            float av[4], bv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { av[j] = a[(ci * 8 + 4 * h + j) * BM + ra_]; bv[j] = b[(ci * 8 + 4 * h + j) * BN + rb_]; }
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], bv[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], bv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], bv[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], bv[3], acc1, 0, 0, 0);
        }
        if (kt + 1 < nst) store_tiles(buf ^ 1);
        __syncthreads();
    }
}

} // namespace
