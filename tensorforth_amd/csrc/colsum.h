// colsum.h - deterministic column sums and slab folds, shared by the convolution units (dF | dB partial slabs, the bias gradient of the
// many-channel path and of the transposed convolution) and the linear layers (their bias gradient).  The kernels live in colsum.hip; the fold
// BODY lives here because the dX kernels of conv.hip and conv_few.hip run it in their first workgroups (the fold rides the dX launch).
#pragma once
#include "t4k_common.h"

namespace t4k {
// OUT[e] += sum_rows X[row][e], deterministic (t4k_linear_bwd, t4k_conv2d_bwd2's many-channel dB, t4k_dconv2d_bwd)
int colsum_add(const float *X, float *OUT, long rows, int E, hipStream_t hs);
// OUT[i] += sum_k part[k][i], one thread per output walking the slices: few slices x many outputs
void launch_fold_add(const float *part, float *OUT, int n, int nslice, hipStream_t hs);
// the wave-per-output fold as a launch of its own (k_conv_df_fold): outputs [0, ndf) go to DF, [ndf, ntot) to DB
void launch_df_fold(const float *part, float *DF, float *DB, int nslice, int ndf, int ntot, hipStream_t hs);
}

namespace {
// fold the slabs: DF[i] += sum_slice part[slice][i], DB likewise.  One wave per output: lane l adds slices l, l+64, ...
// (all loads of a lane are independent), then a fixed xor-tree across the wave => deterministic, and the
// ~1000 slices of a LeNet-size layer are summed in two load rounds instead of a 200-deep dependent chain.
__device__ __forceinline__ void conv_df_fold_body(const float *__restrict__ part, float *DF, float *DB, int nslice, int ndf, int ntot, int bx) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = bx * 4 + w;
    if (i >= ntot) return;
    float s = 0.f;
#pragma unroll 4
    for (int k = lane; k < nslice; k += 64) s += part[(long)k * ntot + i];
    s = t4k::wave_sum_all(s);
    if (lane == 0) { if (i < ndf) DF[i] += s; else DB[i - ndf] += s; }
}
}
