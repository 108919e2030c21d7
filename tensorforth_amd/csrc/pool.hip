// pool.hip - pooling and up-sampling layers (avg / max / min pool, usample) for NHWC fp32 tensors, kernel size 2 or 3.
// Reference: k_pool / k_dpool, src/nn/nmath.tcu:400-568.
#include "t4k_common.h"
#include <float.h>

using namespace t4k;

namespace {

// ------------------------------------------------------------------ pooling
template <int KS>
__global__ void __launch_bounds__(BLK) k_pool(int layer, const float *__restrict__ I, float *__restrict__ O,
                                              int N, int H1, int W1, int H0, int W0, int C) {
    const long total = (long)N * H0 * W0 * C;
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < total; z += (long)gridDim.x * BLK) {
        int c, j0, i0, n; long t; split2(z, C, c, t); split3(t, W0, H0, j0, i0, n);
        float v = 0.f; bool first = true;
#pragma unroll
        for (int y = 0; y < KS; y++)
#pragma unroll
            for (int x = 0; x < KS; x++) {
                const int gi = i0 * KS + y, gj = j0 * KS + x;
                if (gi >= H1 || gj >= W1) continue;                 // defined edge (reference: UB)
                const float e = I[(((long)n * H1 + gi) * W1 + gj) * C + c];
                if (layer == T4K_L_MAXPOOL)      v = first ? e : fmaxf(e, v);
                else if (layer == T4K_L_MINPOOL) v = first ? e : fminf(e, v);
                else                             v += e;
                first = false;
            }
        if (layer == T4K_L_AVGPOOL || layer == T4K_L_USAMPLE) v /= (float)(KS * KS);
        O[z] = v;
    }
}
template <int KS>
__global__ void __launch_bounds__(BLK) k_dpool(int layer, float *I, const float *__restrict__ DY,
                                               int N, int H1, int W1, int H0, int W0, int C) {
    const long total = (long)N * H0 * W0 * C;
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < total; z += (long)gridDim.x * BLK) {
        int c, j0, i0, n; long t; split2(z, C, c, t); split3(t, W0, H0, j0, i0, n);
        const float dy = DY[z];
        float best = 0.f; long arg = -1;
#pragma unroll
        for (int y = 0; y < KS; y++)
#pragma unroll
            for (int x = 0; x < KS; x++) {
                const int gi = i0 * KS + y, gj = j0 * KS + x;
                if (gi >= H1 || gj >= W1) continue;
                const long a = (((long)n * H1 + gi) * W1 + gj) * C + c;
                if (layer == T4K_L_AVGPOOL)      I[a] = dy / (float)(KS * KS);
                else if (layer == T4K_L_USAMPLE) I[a] = dy;
                else {
                    const float dx = I[a]; I[a] = 0.f;
                    const bool better = (layer == T4K_L_MAXPOOL) ? (dx > best) : (dx < best);
                    if (arg < 0 || better) { best = dx; arg = a; }       // first extreme wins
                }
            }
        if (arg >= 0) I[arg] = dy;
    }
}

} // namespace

extern "C" {

int t4k_pool(int layer, const float *I, float *O, int N, int H1, int W1, int H0, int W0, int C, int KS, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (KS != 2 && KS != 3) return fail(T4K_ERR_UNSUPPORTED, "nn#fpool kernel_size=%d not supported", KS);
    if (layer != T4K_L_AVGPOOL && layer != T4K_L_MAXPOOL && layer != T4K_L_MINPOOL && layer != T4K_L_USAMPLE)
        return fail(T4K_ERR_UNSUPPORTED, "t4k_pool: layer %d", layer);
    const long total = (long)N * H0 * W0 * C; if (total <= 0) return T4K_OK;
    if (KS == 2) T4K_LAUNCH(k_pool<2>, dim3(grid_for(total)), dim3(BLK), 0, t4k::S(s), layer, I, O, N, H1, W1, H0, W0, C);
    else         T4K_LAUNCH(k_pool<3>, dim3(grid_for(total)), dim3(BLK), 0, t4k::S(s), layer, I, O, N, H1, W1, H0, W0, C);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}
int t4k_dpool(int layer, float *I, const float *DY, int N, int H1, int W1, int H0, int W0, int C, int KS, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (KS != 2 && KS != 3) return fail(T4K_ERR_UNSUPPORTED, "nn#bpool kernel_size=%d not supported", KS);
    if (layer != T4K_L_AVGPOOL && layer != T4K_L_MAXPOOL && layer != T4K_L_MINPOOL && layer != T4K_L_USAMPLE)
        return fail(T4K_ERR_UNSUPPORTED, "t4k_dpool: layer %d", layer);
    const long total = (long)N * H0 * W0 * C; if (total <= 0) return T4K_OK;
    if (KS == 2) T4K_LAUNCH(k_dpool<2>, dim3(grid_for(total)), dim3(BLK), 0, t4k::S(s), layer, I, DY, N, H1, W1, H0, W0, C);
    else         T4K_LAUNCH(k_dpool<3>, dim3(grid_for(total)), dim3(BLK), 0, t4k::S(s), layer, I, DY, N, H1, W1, H0, W0, C);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

} // extern "C"
