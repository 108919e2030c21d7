// colsum.hip - column sums of a row-major matrix and the folds of partial slabs, every one in a fixed order (no atomics): see colsum.h.
// A unit of its own because three families call it - conv.hip / dconv.hip for dB and the dF slabs, linear.hip for the bias gradient -
// and none of them owns it.
#include "colsum.h"

using namespace t4k;

namespace {

__global__ void __launch_bounds__(256) k_conv_df_fold(const float *__restrict__ part, float *DF, float *DB,
                                                      int nslice, int ndf, int ntot) {
    conv_df_fold_body(part, DF, DB, nslice, ndf, ntot, blockIdx.x);
}

// ------------------------------------------------------------------ generic column sums
__global__ void __launch_bounds__(BLK) k_fold_add(const float *__restrict__ part, float *OUT, int n, int nchunk) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < nchunk; k++) s += part[(long)k * n + i];
    OUT[i] += s;
}
__global__ void __launch_bounds__(BLK) k_colsum_part(const float *__restrict__ X, float *__restrict__ part,
                                                     long rows, int E, int rows_per_chunk, float *direct) {
    __shared__ float sm[4][64];
    const int ex = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int e = blockIdx.y * 64 + ex;
    const long r0 = (long)blockIdx.x * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
    float acc = 0.f;
    if (e < E) {
#pragma unroll 4
        for (long r = r0 + ry; r < r1; r += 4) acc += X[r * E + e];
    }
    sm[ry][ex] = acc;
    __syncthreads();
    if (ry == 0 && e < E) {
        const float t = (sm[0][ex] + sm[1][ex]) + (sm[2][ex] + sm[3][ex]);
        if (direct) direct[e] += t;                       // single chunk: accumulate in place
        else part[(long)blockIdx.x * E + e] = t;
    }
}

} // namespace

namespace t4k {
// OUT[e] += sum_rows X[row][e], deterministic (used by t4k_linear_bwd / t4k_dlinear_db)
int colsum_add(const float *X, float *OUT, long rows, int E, hipStream_t hs) {
    if (rows <= 0 || E <= 0) return T4K_OK;
    // ~256 rows per chunk (each of the 4 row groups then sums 64 rows), up to 2048 chunks: a 262144 x 64 matrix
    // (the dO of a CIFAR-size conv layer) spreads over 1024 workgroups instead of 64
    long want = (rows + 255) / 256; if (want > 2048) want = 2048; if (want < 1) want = 1;
    if (rows <= 1024) want = 1;                       // small: single chunk accumulates in place (one launch)
    const int rpc = (int)((rows + want - 1) / want);
    const int nchunk = (int)((rows + rpc - 1) / rpc);
    float *part = ws_for(hs) + (8 << 20);            // second 32 MiB half of the workspace
    if ((size_t)nchunk * E * sizeof(float) > st().ws_bytes / 2) return fail(T4K_ERR_NOMEM, "colsum workspace");
    conv_plan_note("colsum<%d>%s", nchunk, nchunk > 1 ? "+fold" : "");
    if (nchunk == 1) {
        T4K_LAUNCH(k_colsum_part, dim3(1, (E + 63) / 64), dim3(BLK), 0, hs, X, part, rows, E, rpc, OUT);
        return T4K_OK;
    }
    T4K_LAUNCH(k_colsum_part, dim3(nchunk, (E + 63) / 64), dim3(BLK), 0, hs, X, part, rows, E, rpc, (float *)nullptr);
    T4K_LAUNCH(k_conv_df_fold, dim3((E + 3) / 4), dim3(256), 0, hs, part, OUT, OUT, nchunk, E, E);   // one wave per output, fixed xor tree
    return T4K_OK;
}
void launch_fold_add(const float *part, float *OUT, int n, int nslice, hipStream_t hs) {
    T4K_LAUNCH(k_fold_add, dim3((n + BLK - 1) / BLK), dim3(BLK), 0, hs, part, OUT, n, nslice);
}
void launch_df_fold(const float *part, float *DF, float *DB, int nslice, int ndf, int ntot, hipStream_t hs) {
    T4K_LAUNCH(k_conv_df_fold, dim3((ntot + 3) / 4), dim3(256), 0, hs, part, DF, DB, nslice, ndf, ntot);
}
}
