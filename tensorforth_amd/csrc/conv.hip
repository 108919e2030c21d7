// conv.hip - conv2d forward / backward as implicit GEMMs on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32) for NHWC fp32 tensors:
// the gather-MFMA kernels, and the t4k_conv2d_* entry points with their dispatch over the other engines (conv_few.hip, conv_img.hip, conv_big.hip).
// Reference: k_conv2d / k_dconv2d, src/nn/nmath.tcu:34-338;
// host wrappers Model::_fconv src/nn/forward.cu:125-155, Model::_bconv src/nn/backprop.cu:152-191.
//
// The reference launches one 16x16 block per (n, c1, c0) plane tile, re-stages the same input
// patch for every c0 and accumulates across c1 with fp32 atomicAdd into a pre-zeroed output.
// Here each of the three contractions is one dense MFMA GEMM whose A operand is gathered on the
// fly (implicit im2col):
//   forward  O [pix0 , c0]  = sum_{ky,kx,c1} I [pix0 shifted, c1] * F [c1,ky,kx,c0]      (+ bias)
//   dX       dX[pix1 , c1]  = sum_{ky,kx,c0} dO[pix1 shifted, c0] * F [c1,K-1-ky,K-1-kx,c0]
//   dF|dB    dF[tap  , c0] += sum_{pix0}     I [pix0 shifted by tap] * dO[pix0, c0]   (row `ntaps` = dB)
// One wave owns a 32 (pixels or taps) x 32 (channels) accumulator.  The filter slice is staged in
// LDS in MFMA-B order; the k-pair of one MFMA is two adjacent channels of the same tap, so the two
// lane halves read adjacent floats.  Every output element is written once (no memset, no atomics);
// dF/dB are reduced wave -> workgroup (LDS) -> workspace slabs -> one fold launch, in fixed order.
#include "conv_types.h"
#include <float.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));


// element-wise run that follows the convolution (dropout/activation -> 2x2 pool -> activation -> flatten copy, see fused.hip),
// applied in the conv epilogue: with a window-major pixel order the four positions of a pool window are four consecutive
// accumulator registers of one lane, so the whole run is register-local
struct PoolEpi {
    float *P, *Q, *R, *R2, *Fpre, *Fpost;
    int pre, pool, post; float a_pre, a_post;
    RngArg rng;
};

// component j of the Philox block held by lane SRC of this lane's quad, as a uniform (0,1] draw
template <int SRC>
__device__ __forceinline__ float quad_pick(const uint32_t r[4], int j) {
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)r[0], SRC * 0x55, 0xf, 0xf, true);
    const uint32_t t1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)r[1], SRC * 0x55, 0xf, 0xf, true);
    const uint32_t t2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)r[2], SRC * 0x55, 0xf, 0xf, true);
    const uint32_t t3 = (uint32_t)__builtin_amdgcn_mov_dpp((int)r[3], SRC * 0x55, 0xf, 0xf, true);
    return u01(j == 0 ? t0 : (j == 1 ? t1 : (j == 2 ? t2 : t3)));
}

// ------------------------------------------------------------------ forward / dX gather-GEMM
// BWD = false: forward (Cin = C1 of I, Cout = C0);  BWD = true: dX (Cin = C0 of dO, Cout = C1)
template <int K, int S, int P, bool BWD, bool POOL = false>
__device__ __forceinline__ void conv_gemm_body(const float *__restrict__ X, float *__restrict__ Y, float *__restrict__ Y2,
                                               const float *__restrict__ F, const float *__restrict__ B,
                                               int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout,
                                               int C0 /* filter inner dim */, int pairs_per_chunk, int bx, int by, int ksplit = 1,
                                               const PoolEpi *pe = nullptr, float *__restrict__ XC = nullptr) {
    __shared__ float Bl[LDS_FILTER_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const long npix = (long)N * Hy * Wy;
    // ksplit == 2 (small layers that would leave SIMDs empty): two waves share one 32x32 tile, each takes alternate
    // blocks of channel pairs, the halves meet in LDS - twice the waves, half the dependent loads / MFMAs per wave
    const int kh = (ksplit == 2) ? (w & 1) : 0;
    const long tile = (ksplit == 2) ? (long)bx * 2 + (w >> 1) : (long)bx * 4 + w;
    const long pix  = tile * 32 + l31;                       // this lane's A-row pixel
    const int  co0  = by * 32;                               // output-channel tile
    const bool pok  = pix < npix;
    int jy = 0, iy = 0, n = 0;
    if (pok) {
        if (POOL) {                                          // window-major: row m = 4 * window + position (Hy, Wy even)
            const long wdx = pix >> 2; const int pos = (int)(pix & 3), W2 = Wy >> 1, H2 = Hy >> 1;
            int j0, i0; split3(wdx, W2, H2, j0, i0, n);
            iy = 2 * i0 + (pos >> 1); jy = 2 * j0 + (pos & 1);
        } else split3(pix, Wy, Hy, jy, iy, n);
    }
    const float *nX = X + (long)n * Hx * Wx * Cin;
    if (POOL && XC && pok && by == 0 && kh == 0 && h == 0) {     // layer 0 keeps a COPY of the batch (forward.cu:39); same-size conv: shared pixel grid
        const long o = (((long)n * Hy + iy) * Wy + jy) * Cin;
        for (int ci = 0; ci < Cin; ci++) XC[o + ci] = X[o + ci];
    }

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;

    // per-tap element offsets of this lane's pixel (-1 = outside the image): computed once, so the loads below are
    // unconditional (clamped address + select) and the compiler can keep a whole chunk of them in flight
    int off[K * K];
#pragma unroll
    for (int ky = 0; ky < K; ky++) {
        int gi; bool iok;
        if (!BWD) { gi = iy * S + ky - P; iok = gi >= 0 && gi < Hx; }
        else { const int ti = iy + P - ky; gi = ti / S; iok = ti >= 0 && (ti % S) == 0 && gi < Hx; }
#pragma unroll
        for (int kx = 0; kx < K; kx++) {
            int gj; bool jok;
            if (!BWD) { gj = jy * S + kx - P; jok = gj >= 0 && gj < Wx; }
            else { const int tj = jy + P - kx; gj = tj / S; jok = tj >= 0 && (tj % S) == 0 && gj < Wx; }
            off[ky * K + kx] = (pok && iok && jok) ? (gi * Wx + gj) * Cin : -1;
        }
    }
    const int npairs = (Cin + 1) >> 1;
    // Small filters (the whole [C1][K][K][C0] tensor fits the LDS stage) are copied verbatim with coalesced 16 B loads -
    // one round trip - and indexed in place; the per-element gather into MFMA-B order below costs a dependent global
    // load per LDS entry and dominated the LeNet-size layers.
    const int nF = (BWD ? Cout : Cin) * K * K * C0;
    const bool raw = nF <= LDS_FILTER_FLOATS;
    if (raw) {
        pairs_per_chunk = npairs;
        if ((((uintptr_t)F) & 15) == 0) {
            const int n4 = nF >> 2;
            for (int e = tid; e < n4; e += 256) reinterpret_cast<float4 *>(Bl)[e] = reinterpret_cast<const float4 *>(F)[e];
            for (int e = (n4 << 2) + tid; e < nF; e += 256) Bl[e] = F[e];
        } else for (int e = tid; e < nF; e += 256) Bl[e] = F[e];
        __syncthreads();
    }
    for (int cp0 = 0; cp0 < npairs; cp0 += pairs_per_chunk) {
        const int cpn = min(pairs_per_chunk, npairs - cp0);
        if (!raw) {
        // ---- stage the filter slice: Bl[((cp*K+ky)*K+kx)*2+hh][col] ----
        __syncthreads();
        const int nent = cpn * K * K * 2 * 32;
        for (int e = tid; e < nent; e += 256) {
            const int col = e & 31; int t = e >> 5;
            const int hh = t & 1; t >>= 1;
            const int kx = t % K; t /= K; const int ky = t % K; const int cp = t / K;
            const int ci = 2 * (cp0 + cp) + hh, co = co0 + col;
            float v = 0.f;
            if (ci < Cin && co < Cout) {
                if (!BWD) v = F[((long)(ci * K + ky) * K + kx) * C0 + co];                          // F[c1=ci][ky][kx][c0=co]
                else      v = F[((long)(co * K + (K - 1 - ky)) * K + (K - 1 - kx)) * C0 + ci];      // F[c1=co][flip][c0=ci]
            }
            Bl[e] = v;
        }
        __syncthreads();
        }
        for (int cpb = kh * 2; cpb < cpn; cpb += 2 * ksplit) {   // two channel pairs per trip: 2*K*K loads in flight
            float a[2][K * K];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const int ci = 2 * (cp0 + cpb + u) + h;
                const bool cok = (cpb + u) < cpn && ci < Cin;
#pragma unroll
                for (int t = 0; t < K * K; t++) {
                    const bool ok = cok && off[t] >= 0;
                    const float v = nX[ok ? off[t] + ci : 0];
                    a[u][t] = ok ? v : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (cpb + u < cpn) {
#pragma unroll
                    for (int t = 0; t < K * K; t++) {
                        float b;
                        if (raw) {
                            const int ci = 2 * (cpb + u) + h, co = co0 + l31;
                            const bool ok = ci < Cin && co < Cout;
                            const int idx = !BWD ? (ci * K * K + t) * C0 + co : (co * K * K + (K * K - 1 - t)) * C0 + ci;
                            const float v = Bl[ok ? idx : 0];
                            b = ok ? v : 0.f;
                        } else b = Bl[(((cpb + u) * K * K + t) * 2 + h) * 32 + l31];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], b, acc, 0, 0, 0);
                    }
                }
            }
        }
    }
    if (ksplit == 2) {                                      // the two k-halves of a tile meet in LDS (the filter stage is free now)
        __syncthreads();
        if (kh == 1) {
#pragma unroll
            for (int r = 0; r < 16; r++) Bl[((w >> 1) * 16 + r) * 64 + lane] = acc[r];
        }
        __syncthreads();
        if (kh == 1) return;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] += Bl[((w >> 1) * 16 + r) * 64 + lane];
    }
    // ---- epilogue: D[row = pixel][col = channel]; col = lane&31, row = (r&3)+8*(r>>2)+4*h
    const int co = co0 + l31;
    if (POOL) {
        // rows 4q+{0..3} (+4h) of this lane are the four positions of pool window tile*8 + 2q + h
        uint64_t rbase = 0, rseed = 0;
        const bool draw = pe->pre == T4K_L_DROPOUT;
        if (draw) rng_begin(pe->rng, rbase, rseed);
        if (co < Cout) {
            const float bias = B ? B[co] : 0.f;
            const int W2 = Wy >> 1, H2 = Hy >> 1;
            const long nwin = npix >> 2;
            // window coordinates: one split for the lane's first window, the other three advance by two windows each
            int j0, i0, nn0; split3(tile * 8 + h, W2, H2, j0, i0, nn0);
            long nn = nn0;
            // Cout % 4 == 0: the four lanes of a quad (channels 4g..4g+3) sit in ONE Philox counter block per pixel, so lane j
            // generates only the block of window position j and the quad exchanges components (4 blocks per lane, not 16)
            const bool quad = draw && (Cout & 3) == 0;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const long wdx = tile * 8 + 2 * q + h;
                if (wdx < nwin) {
                    const long a0 = (((nn * Hy + 2 * i0) * Wy) + 2 * j0) * Cout + co;    // window position 0; +Cout, +Wy*Cout, +both
                    float uq[4] = { 0.f, 0.f, 0.f, 0.f };
                    if (quad) {
                        const int j = lane & 3;
                        const long aj = a0 + (long)((j >> 1) * Wy + (j & 1)) * Cout;
                        uint32_t r4[4];
                        philox4x32_10(rbase + (uint64_t)(aj >> 2), rseed, r4);
                        uq[0] = quad_pick<0>(r4, j); uq[1] = quad_pick<1>(r4, j); uq[2] = quad_pick<2>(r4, j); uq[3] = quad_pick<3>(r4, j);
                    }
                    float pv = 0.f; bool first = true;
#pragma unroll
                    for (int pos = 0; pos < 4; pos++) {
                        const long a = a0 + (long)((pos >> 1) * Wy + (pos & 1)) * Cout;
                        float e = acc[4 * q + pos] + bias;
                        Y[a] = e;
                        if (pe->pre) {
                            float o, f;
                            act_rt_lean(pe->pre, e, quad ? uq[pos] : (draw ? philox_u01_at(rbase, rseed, a) : 0.f), pe->a_pre, o, f);
                            pe->Fpre[a] = f; pe->P[a] = o; e = o;
                        }
                        if (pe->pool == T4K_L_MAXPOOL)      pv = first ? e : fmaxf(e, pv);
                        else if (pe->pool == T4K_L_MINPOOL) pv = first ? e : fminf(e, pv);
                        else                                pv += e;
                        first = false;
                    }
                    if (pe->pool == T4K_L_AVGPOOL) pv /= 4.0f;
                    const long z = wdx * Cout + co;
                    pe->Q[z] = pv;
                    if (pe->post) { float o, f; act_rt_lean(pe->post, pv, 0.f, pe->a_post, o, f); pe->Fpost[z] = f; pe->R[z] = o; pv = o; }
                    if (pe->R2) pe->R2[z] = pv;
                }
                j0 += 2;                                                          // next window of this lane: wdx + 2
                while (j0 >= W2) { j0 -= W2; if (++i0 >= H2) { i0 = 0; nn++; } }
            }
        }
        if (draw && pe->rng.state) rng_advance_n(pe->rng.state, rbase, (uint64_t)((npix * Cout + 3) >> 2), gridDim.x * gridDim.y);
        return;
    }
    if (co < Cout) {
        const float bias = (!BWD && B) ? B[co] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const long p2 = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (p2 < npix) { const float v = acc[r] + bias; Y[p2 * Cout + co] = v; if (Y2) Y2[p2 * Cout + co] = v; }
        }
    }
}
// forward convolution with the element-wise run behind it (t4k_conv2d_block_fwd)
template <int K, int S, int P>
__global__ void __launch_bounds__(256) k_conv_gemm_pool(const float *__restrict__ X, float *__restrict__ Y, const float *__restrict__ F, const float *__restrict__ B,
                                                        int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout, int C0, int pairs_per_chunk, int ksplit, PoolEpi pe, float *__restrict__ XC) {
    conv_gemm_body<K, S, P, false, true>(X, Y, nullptr, F, B, N, Hx, Wx, Cin, Hy, Wy, Cout, C0, pairs_per_chunk, blockIdx.x, blockIdx.y, ksplit, &pe, XC);
}

template <int K, int S, int P, bool BWD>
__global__ void __launch_bounds__(256) k_conv_gemm(const float *__restrict__ X, float *__restrict__ Y, float *__restrict__ Y2,
                                                   const float *__restrict__ F, const float *__restrict__ B,
                                                   int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout, int C0, int pairs_per_chunk, int ksplit) {
    conv_gemm_body<K, S, P, BWD>(X, Y, Y2, F, B, N, Hx, Wx, Cin, Hy, Wy, Cout, C0, pairs_per_chunk, blockIdx.x, blockIdx.y, ksplit);
}

// ------------------------------------------------------------------ dF | dB
// grid = (slices, m_tiles, c0_tiles); each wave accumulates D[tap][c0] over its output rows
template <int K, int S, int P>
__device__ __forceinline__ void conv_df_body(const float *__restrict__ I, const float *__restrict__ DO,
                                             float *__restrict__ part,
                                             int N, int H1, int W1, int C1, int H0, int W0, int C0,
                                             int rows_per_wave, int bx, int by, int bz) {
    __shared__ float red[4][32][33];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int ntaps = C1 * K * K;                           // row `ntaps` is the bias row (all ones)
    const int tap = by * 32 + l31;
    const int co  = bz * 32 + l31;
    int c1 = 0, ky = 0, kx = 0;
    const bool is_tap = tap < ntaps, is_bias = tap == ntaps;
    if (is_tap) { kx = tap % K; ky = (tap / K) % K; c1 = tap / (K * K); }
    const bool cok = co < C0;
    const int rows = N * H0;
    const int row_beg = (bx * 4 + w) * rows_per_wave;
    const int row_end = min(rows, row_beg + rows_per_wave);

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;

    for (int row = row_beg; row < row_end; row++) {
        const int n = row / H0, i0 = row - n * H0;          // wave-uniform
        const int gi = i0 * S + ky - P;
        const bool iok = is_tap && gi >= 0 && gi < H1;
        const float *rI = iok ? I + (((long)n * H1 + gi) * W1) * C1 + c1 : I;
        const float *rO = DO + ((long)row * W0) * C0 + (cok ? co : 0);
        const int nit = (W0 + 1) / 2;                       // wave-uniform trip count; lane half h takes pixel 2*it + h
        for (int itb = 0; itb < nit; itb += 7) {            // 7 pixel pairs per trip (W0 = 14, 28: no tail): 14 loads in flight
            float av[7], bv[7]; bool aok[7], jv[7];
#pragma unroll
            for (int u = 0; u < 7; u++) {
                const int j0 = 2 * (itb + u) + h;
                jv[u] = (itb + u) < nit && j0 < W0;
                const int gj = j0 * S + kx - P;
                aok[u] = jv[u] && iok && gj >= 0 && gj < W1;
                av[u] = rI[aok[u] ? gj * C1 : 0];           // unconditional (clamped) loads
                bv[u] = rO[jv[u] ? j0 * C0 : 0];
            }
#pragma unroll
            for (int u = 0; u < 7; u++) {
                if (itb + u < nit) {
                    const float a = (jv[u] && is_bias) ? 1.f : (aok[u] ? av[u] : 0.f);
                    const float b = (jv[u] && cok) ? bv[u] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
                }
            }
        }
    }
    // wave -> workgroup reduction through LDS, then one slab entry per (slice, tap, c0)
#pragma unroll
    for (int r = 0; r < 16; r++) red[w][(r & 3) + 8 * (r >> 2) + 4 * h][l31] = acc[r];
    __syncthreads();
    const int nrow1 = ntaps + 1;
    for (int e = tid; e < 1024; e += 256) {
        const int tr = e >> 5, tc = e & 31;
        const int gt = by * 32 + tr, gc = bz * 32 + tc;
        if (gt < nrow1 && gc < C0)
            part[((long)bx * nrow1 + gt) * C0 + gc] = (red[0][tr][tc] + red[1][tr][tc]) + (red[2][tr][tc] + red[3][tr][tc]);
    }
}
template <int K, int S, int P>
__global__ void __launch_bounds__(256) k_conv_df_mfma(const float *__restrict__ I, const float *__restrict__ DO, float *__restrict__ part,
                                                      int N, int H1, int W1, int C1, int H0, int W0, int C0, int rows_per_wave) {
    conv_df_body<K, S, P>(I, DO, part, N, H1, W1, C1, H0, W0, C0, rows_per_wave, blockIdx.x, blockIdx.y, blockIdx.z);
}
// The dF fold and the layer's dX are independent once the dF partials exist, so they share a launch: the first nfold
// workgroups fold, the rest run the dX implicit GEMM (hx x hy grid, linearised).  dX may now overwrite the layer input
// (DX2 = I, the reference's `in = dx`): the dF kernel that read I finished with the previous launch.
template <int K, int S, int P>
__global__ void __launch_bounds__(256) k_conv_dx_and_fold(const float *__restrict__ part, float *DF, float *DB, int nslice, int ndf, int ntot, int nfold,
                                                          const float *__restrict__ DO, float *__restrict__ DX, float *__restrict__ DX2, const float *__restrict__ F,
                                                          int N, int H1, int W1, int C1, int H0, int W0, int C0, int hx, int ppc, int ksplit) {
    const int b = blockIdx.x;
    if (b < nfold) conv_df_fold_body(part, DF, DB, nslice, ndf, ntot, b);
    else { const int b2 = b - nfold; conv_gemm_body<K, S, P, true>(DO, DX, DX2, F, nullptr, N, H0, W0, C0, H1, W1, C1, C0, ppc, b2 % hx, b2 / hx, ksplit); }
}

// ------------------------------------------------------------------ host: shapes of the gather kernel, admission tests
// two waves per tile when the layer is small enough to leave SIMDs empty and has enough k-work to split
int conv_gemm_ksplit(long npix, int Cout, int Cin, int K) {
    const long waves = ((npix + 31) / 32) * ((Cout + 31) / 32);
    return (conv_lab().ksplit && waves < 1536 && ((Cin + 1) / 2) * K * K >= 18) ? 2 : 1;
}
// launch shape of conv_gemm_body for npix output pixels x Cout channels gathered from Cin: 128 / ksplit pixels per workgroup
struct GatherShape { int ksplit, ppc, gx, gy; };
GatherShape gather_shape(long npix, int Cout, int Cin, int K) {
    const int ksplit = conv_gemm_ksplit(npix, Cout, Cin, K);
    return { ksplit, LDS_FILTER_FLOATS / (K * K * 2 * 32) /* channel pairs per LDS filter slice */, (int)((npix + (128 / ksplit) - 1) / (128 / ksplit)), (Cout + 31) / 32 };
}
// what conv_gemm_body decides from the filter's size: copied verbatim into the LDS stage (raw) or staged per chunk of channel pairs
const char *gather_filter(int C1, int K, int C0) { return C1 * K * K * C0 <= LDS_FILTER_FLOATS ? "raw" : "staged"; }
// many channels: the LDS-staged GEMM tiling of conv_big.hip (16-byte loads of both operands)
bool big_path(int Cin, int Cout, const void *a, const void *b) { return conv_lab().big && conv_big_ok(Cin, Cout) && aligned16(a) && aligned16(b); }
// 3x3 / stride 1 / padding 1 on a shared pixel grid: what the kernels of conv_img.hip serve
bool same3x3(int K, int S, int P, int H1, int W1, int H0, int W0) { return K == 3 && S == 1 && P == 1 && H0 == H1 && W0 == W1; }
// t4k_conv2d_block_fwd: the element-wise run can leave from the conv epilogue (2x2 pool windows of a stride-1 3x3 / 5x5 layer that is not a many-channel one)
bool fusable(const t4k_poolblock *blk, int H0, int W0, int C1, int C0, int K, int S, int P) {
    return blk->pool_layer && blk->KS == 2 && (H0 % 2) == 0 && (W0 % 2) == 0 && S == 1 && (K == 3 || K == 5) &&
           blk->pool_out && (!blk->pre_layer || (blk->pre_mask && blk->pre_out)) && (!blk->post_layer || (blk->post_mask && blk->post_out)) &&
           blk->post_layer != T4K_L_DROPOUT &&           // a dropout BEHIND the pool draws in the element-wise run kernel (fused.hip), not in the conv epilogue
           !(conv_lab().big && conv_big_ok(C1, C0)) && conv_supported(K, S, P) && conv_lab().block;
}
// the layer-0 copy of the batch (forward.cu:39) where no kernel writes it from its own launch
int copy_input(float *ICOPY, const float *I, int N, int H1, int W1, int C1, hipStream_t hs) {
    conv_plan_note("memcpy");
    T4K_HIP(hipMemcpyAsync(ICOPY, I, sizeof(float) * (size_t)N * H1 * W1 * C1, hipMemcpyDeviceToDevice, hs));
    return T4K_OK;
}

template <bool BWD>
void launch_conv_gemm(int K, int S, int P, hipStream_t hs, const float *X, float *Y, float *Y2, const float *F, const float *B,
                      int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout, int C0) {
    const GatherShape gs = gather_shape((long)N * Hy * Wy, Cout, Cin, K);
    conv_plan_note("gather<%s,ks%d>", gather_filter(BWD ? Cout : Cin, K, C0), gs.ksplit);
    with_geometry(K, S, P, [&](auto geo) {
        using Ge = decltype(geo);
        T4K_LAUNCH((k_conv_gemm<Ge::K, Ge::S, Ge::P, BWD>), dim3(gs.gx, gs.gy), dim3(256), 0, hs, X, Y, Y2, F, B, N, Hx, Wx, Cin, Hy, Wy, Cout, C0, gs.ppc, gs.ksplit);
    });
}

// the forward of one layer; bn_part (may be NULL): where the layer's kernel may leave the per-channel sums of O as chunk partials (*bn_chunks > 0 says it did)
int conv2d_fwd_impl(const float *I, float *ICOPY, float *O, const float *F, const float *B,
                    int N, int H1, int W1, int C1, int H0, int W0, int C0,
                    int K, int S, int P, float *bn_part, size_t bn_part_floats, int *bn_chunks, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (bn_chunks) *bn_chunks = 0;
    if (!conv_supported(K, S, P))
        return fail(T4K_ERR_UNSUPPORTED, "nn#fconv kernel_size=%d stride=%d padding=%d not supported", K, S, P);
    if (!I || !O || !F || !B || N <= 0 || C0 <= 0 || C1 <= 0 || H0 <= 0 || W0 <= 0) return fail(T4K_ERR_ARG, "t4k_conv2d_fwd: bad argument");
    hipStream_t hs = t4k::S(s);
    const bool same_grid = H0 == H1 && W0 == W1;
    int fG, fNG;
    if (conv_lab().few && conv_few_ok(K, C1, C0, &fG, &fNG)) {                  // the copy leaves from the conv launch when the pixel grid is shared
        launch_conv_few<false>(K, hs, I, O, nullptr, same_grid ? ICOPY : nullptr, F, B, N, H1, W1, C1, H0, W0, C0, C0, fG, fNG);
        if (ICOPY && !same_grid) { int rc = copy_input(ICOPY, I, N, H1, W1, C1, hs); if (rc) return rc; }
        T4K_LAUNCH_CHECK();
        return T4K_OK;
    }
    // image in, a full MFMA tile or two of channels out (3 -> 64): filter in registers, the layer-0 copy from the same launch (conv_img.hip)
    if (same3x3(K, S, P, H1, W1, H0, W0) && ICOPY != O && conv_thin_fwd(I, ICOPY, O, F, B, N, H0, W0, C1, C0, hs, bn_part, bn_part_floats, bn_chunks)) { T4K_LAUNCH_CHECK(); return T4K_OK; }
    if (ICOPY) { int rc = copy_input(ICOPY, I, N, H1, W1, C1, hs); if (rc) return rc; }
    if (big_path(C1, C0, I, F)) launch_conv_big<false>(K, S, P, hs, I, O, nullptr, F, B, N, H1, W1, C1, H0, W0, C0, C0, bn_part, bn_part_floats, bn_chunks);
    else                        launch_conv_gemm<false>(K, S, P, hs, I, O, nullptr, F, B, N, H1, W1, C1, H0, W0, C0, C0);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}
// the conv forward in front of a batch-norm layer: where the conv kernel can carry them (k_convbig8, k_conv_thin_fwd) the per-channel sums leave its epilogue
// as *chunks partials in the stream's workspace.  Synchronised statistics go through the all-reduce path of t4k_batchnorm_fwd: no rider
int conv2d_fwd_with_bn_rider(const float *I, float *ICOPY, float *Y, const float *F, const float *Bc, int N, int H1, int W1, int C1, int H0, int W0, int C0,
                             int K, int S, int P, int *chunks, t4k_stream_t s) {
    const bool rider = conv_lab().bn_rider && !(st().bn_sync && t4k_comm_world() > 0);
    return conv2d_fwd_impl(I, ICOPY, Y, F, Bc, N, H1, W1, C1, H0, W0, C0, K, S, P, rider ? ws_for(s) : nullptr, st().ws_bytes / 8, chunks, s);
}

// ---- t4k_conv2d_bwd2, stage 1: dF | dB partial slabs (they read I, which the host layer may let DX overwrite).  The many-channel path folds
// its slabs at once (*pending stays empty); the others leave the fold pending for the dX stage
int conv_df_stage(const float *I, const float *DO, float *DF, float *DB, int N, int H1, int W1, int C1, int H0, int W0, int C0,
                  int K, int S, int P, FoldArgs *pending, t4k_stream_t s) {
    hipStream_t hs = t4k::S(s);
    const int ntaps = C1 * K * K, nrow1 = ntaps + 1;         // row `ntaps` of a slab is the bias row
    float *part = ws_for(s);
    const FoldArgs with_bias_row = { part, DF, DB, 0, ntaps * C0, nrow1 * C0, (nrow1 * C0 + 3) / 4 };
    if (big_path(C1, C0, I, DO)) {                           // many channels: split-K GEMM over pixel slices
        const int nbig = launch_conv_big_df(K, S, P, hs, I, DO, part, st().ws_bytes / 8, N, H1, W1, C1, H0, W0, C0);
        if (nbig > 0) {
            const int ntot = ntaps * C0;                     // no bias row in these slabs: dB is a plain column sum of dO
            // few slices x many outputs: one thread per output walks the slices (coalesced); the wave-per-output fold is
            // for the opposite shape (hundreds of slices, few outputs) and would run 8 of 64 lanes here
            if (nbig <= 32) { conv_plan_note("fold_add"); launch_fold_add(part, DF, ntot, nbig, hs); }
            else            { conv_plan_note("df_fold");  launch_df_fold(part, DF, DB, nbig, ntot, ntot, hs); }
            return colsum_add(DO, DB, (long)N * H0 * W0, C0, hs);
        }
    }
    int nthin = 0;                                           // image in, a tile or two of channels out: 32 pixels per wave and trip (conv_img.hip)
    if (same3x3(K, S, P, H1, W1, H0, W0) && conv_thin_df(I, DO, part, st().ws_bytes / 2, N, H0, W0, C1, C0, &nthin, hs)) {
        conv_plan_note("thin_dfx%d+b", nthin);
        *pending = with_bias_row; pending->nslice = nthin;
        return T4K_OK;
    }
    const int rows = N * H0;
    const int tiles = ((nrow1 + 31) / 32) * ((C0 + 31) / 32);
    int nslice = (conv_lab().df_wg + tiles - 1) / tiles; if (nslice > (rows + 3) / 4) nslice = (rows + 3) / 4; if (nslice < 1) nslice = 1;
    while (nslice > 1 && (size_t)nslice * nrow1 * C0 * sizeof(float) > st().ws_bytes / 8) nslice >>= 1;
    const int rpw = (rows + nslice * 4 - 1) / (nslice * 4);
    nslice = (rows + rpw * 4 - 1) / (rpw * 4);
    if ((size_t)nslice * nrow1 * C0 * sizeof(float) > st().ws_bytes / 2) return fail(T4K_ERR_NOMEM, "conv dF workspace");
    const dim3 g(nslice, (nrow1 + 31) / 32, (C0 + 31) / 32);
    conv_plan_note("df_mfmax%d+b", nslice);
    with_geometry(K, S, P, [&](auto geo) {
        using Ge = decltype(geo);
        T4K_LAUNCH((k_conv_df_mfma<Ge::K, Ge::S, Ge::P>), g, dim3(256), 0, hs, I, DO, part, N, H1, W1, C1, H0, W0, C0, rpw);
    });
    *pending = with_bias_row; pending->nslice = nslice;
    return T4K_OK;
}
// ---- stage 2: dX (DX == NULL: none) and the pending fold.  k_conv_dx_few / _wide and k_conv_dx_and_fold carry the fold in their first workgroups;
// the many-channel and the few-output-channel dX kernels do not, and neither does a missing dX: the fold is then launched on its own, first
void conv_dx_stage(const float *DO, float *DX, float *DX2, const float *F, int N, int H1, int W1, int C1, int H0, int W0, int C0,
                   int K, int S, int P, FoldArgs fa, hipStream_t hs) {
    int fG = 0, fNG = 0;
    const bool dx_big   = DX && big_path(C0, C1, DO, F);
    const bool dx_few   = DX && !dx_big && conv_dx_few_ok(K, C1, C0, DO);
    const bool dx_fewch = DX && !dx_big && !dx_few && conv_lab().few && conv_few_ok(K, C0, C1, &fG, &fNG);
    if (fa.nfold && (!DX || dx_big || dx_fewch)) { conv_plan_note("df_fold"); launch_df_fold(fa.part, fa.DF, fa.DB, fa.nslice, fa.ndf, fa.ntot, hs); fa.nfold = 0; }
    if (!DX) return;
    if (dx_big)        launch_conv_big<true>(K, S, P, hs, DO, DX, DX2, F, nullptr, N, H0, W0, C0, H1, W1, C1, C0);
    else if (dx_few)   launch_conv_dx_few(K, S, P, hs, DO, DX, DX2, F, N, H0, W0, C0, H1, W1, C1, fa);     // image-input layer: one thread (or C0 / 4 lanes) per input pixel
    else if (dx_fewch) launch_conv_few<true>(K, hs, DO, DX, DX2, nullptr, F, nullptr, N, H0, W0, C0, H1, W1, C1, C0, fG, fNG);
    else {
        // gather over dO (Hx = H0, Wx = W0, Cin = C0), output the input grid (Hy = H1, Wy = W1, Cout = C1), grid linearised behind the fold's workgroups
        const GatherShape gs = gather_shape((long)N * H1 * W1, C1, C0, K);
        conv_plan_note("dx_and_fold<%s,ks%d>%s", gather_filter(C1, K, C0), gs.ksplit, fa.nfold ? "+fold" : "");
        with_geometry(K, S, P, [&](auto geo) {
            using Ge = decltype(geo);
            T4K_LAUNCH((k_conv_dx_and_fold<Ge::K, Ge::S, Ge::P>), dim3((unsigned)(fa.nfold + gs.gx * gs.gy)), dim3(256), 0, hs, fa.part, fa.DF, fa.DB, fa.nslice, fa.ndf, fa.ntot, fa.nfold,
                       DO, DX, DX2, F, N, H1, W1, C1, H0, W0, C0, gs.gx, gs.ppc, gs.ksplit);
        });
    }
}

} // namespace

extern "C" {

int t4k_conv2d_fwd(const float *I, float *O, const float *F, const float *B,
                   int N, int H1, int W1, int C1, int H0, int W0, int C0,
                   int K, int S, int P, t4k_stream_t s) {
    return t4k_conv2d_fwd2(I, nullptr, O, F, B, N, H1, W1, C1, H0, W0, C0, K, S, P, s);
}
int t4k_conv2d_fwd2(const float *I, float *ICOPY, float *O, const float *F, const float *B,
                    int N, int H1, int W1, int C1, int H0, int W0, int C0,
                    int K, int S, int P, t4k_stream_t s) {
    ConvPlanScope plan;
    return conv2d_fwd_impl(I, ICOPY, O, F, B, N, H1, W1, C1, H0, W0, C0, K, S, P, nullptr, 0, nullptr, s);
}
// conv forward + the batch-norm forward behind it: same tensors, same arithmetic per element as t4k_conv2d_fwd2 + t4k_batchnorm_fwd; with the rider
// (conv2d_fwd_with_bn_rider) the statistics pass over the conv output (a full read of it) is not launched.  T4K_CONV_BN_RIDER=0: always the two calls.
int t4k_conv2d_bn_fwd(const float *I, float *ICOPY, float *Y, const float *F, const float *Bc,
                      int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P,
                      float *O, float *XH, const float *W, const float *B, float *stat_dev, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!O || !XH || !W || !B || !stat_dev) return fail(T4K_ERR_ARG, "t4k_conv2d_bn_fwd: null batch-norm tensor");
    ConvPlanScope plan;
    int chunks = 0;
    int rc = conv2d_fwd_with_bn_rider(I, ICOPY, Y, F, Bc, N, H1, W1, C1, H0, W0, C0, K, S, P, &chunks, s);
    if (rc != T4K_OK) return rc;
    if (chunks > 0) return bn_fwd_from_parts(Y, O, XH, W, B, stat_dev, (long)N * H0 * W0, C0, ws_for(s), chunks, t4k::S(s));
    return t4k_batchnorm_fwd(Y, O, XH, W, B, stat_dev, N, H0 * W0, C0, s);
}

// conv + batch-norm + the element-wise run behind them (the CIFAR-style block conv -> batchnorm -> relu -> maxpool -> dropout): the conv (its epilogue carrying the
// per-channel sums where it can), the finalise of the statistics, then ONE pass that reads the conv output once and writes x-hat, the batch-norm output and
// every tensor of the run (t4k_bn_poolblock_fwd) - the batch-norm output is not read back from memory.  Same tensors as the three calls.
int t4k_conv2d_bn_block_fwd(const float *I, float *ICOPY, float *Y, const float *F, const float *Bc,
                            int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P,
                            float *O, float *XH, const float *W, const float *B, float *stat_dev,
                            const t4k_poolblock *blk, int Hq, int Wq, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!O || !XH || !W || !B || !stat_dev || !blk) return fail(T4K_ERR_ARG, "t4k_conv2d_bn_block_fwd: null tensor");
    ConvPlanScope plan;
    int chunks = 0;
    int rc = conv2d_fwd_with_bn_rider(I, ICOPY, Y, F, Bc, N, H1, W1, C1, H0, W0, C0, K, S, P, &chunks, s);
    if (rc != T4K_OK) return rc;
    rc = bn_stats_for(Y, stat_dev, N, H0 * W0, C0, ws_for(s), chunks, s); if (rc != T4K_OK) return rc;
    return t4k_bn_poolblock_fwd(Y, O, XH, W, B, stat_dev, blk, N, H0, W0, Hq, Wq, C0, s);
}

// conv forward + the element-wise run behind it (dropout/activation -> 2x2 pool -> activation -> flatten copy) in ONE launch
// when the layer takes the gather-MFMA kernel; otherwise the two launches t4k_conv2d_fwd2 + t4k_poolblock_fwd.
int t4k_conv2d_block_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B, const t4k_poolblock *blk,
                         int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!blk) return fail(T4K_ERR_ARG, "t4k_conv2d_block_fwd: null block");
    ConvPlanScope plan;
    // the block is validated BEFORE the convolution runs and before H0 / KS is formed (KS = 0 divided by zero here): a rejected block writes nothing
    { int rc = poolblock_check(blk, "t4k_conv2d_block_fwd"); if (rc) return rc; }
    if (!(I && O && F && B && fusable(blk, H0, W0, C1, C0, K, S, P))) {
        int rc = t4k_conv2d_fwd2(I, ICOPY, O, F, B, N, H1, W1, C1, H0, W0, C0, K, S, P, s); if (rc) return rc;
        return t4k_poolblock_fwd(O, blk, N, H0, W0, H0 / blk->KS, W0 / blk->KS, C0, s);
    }
    hipStream_t hs = t4k::S(s);
    // image-input layer (1 or 3 channels in, <= 16 out): the thread-per-pool-window vector kernel of conv_img.hip
    if (K == 3 && P == 1 && H1 == H0 && W1 == W0 && conv_img_block_fwd(I, ICOPY, O, F, B, blk, N, H0, W0, C1, C0, hs)) { conv_plan_note("img_block"); T4K_LAUNCH_CHECK(); return T4K_OK; }
    // layer-0 copy: written by the conv launch itself when input and output share the pixel grid and the channels are few
    float *xc = (ICOPY && H1 == H0 && W1 == W0 && C1 <= 4) ? ICOPY : nullptr;
    if (ICOPY && !xc) { int rc = copy_input(ICOPY, I, N, H1, W1, C1, hs); if (rc) return rc; }
    PoolEpi pe;
    pe.P = blk->pre_out; pe.Q = blk->pool_out; pe.R = blk->post_out; pe.R2 = blk->copy_out; pe.Fpre = blk->pre_mask; pe.Fpost = blk->post_mask;
    pe.pre = blk->pre_layer; pe.pool = blk->pool_layer; pe.post = blk->post_layer; pe.a_pre = blk->pre_alpha; pe.a_post = blk->post_alpha;
    const long npix = (long)N * H0 * W0;
    pe.rng = RngArg{0, 0, nullptr};
    if (pe.pre == T4K_L_DROPOUT) pe.rng = rng_draw(hs, (uint64_t)((npix * C0 + 3) >> 2), true);
    const GatherShape gs = gather_shape(npix, C0, C1, K);
    conv_plan_note("gather_pool<%s,ks%d>", gather_filter(C1, K, C0), gs.ksplit);
    with_geometry(K, S, P, [&](auto geo) {                  // fusable(): stride 1, K 3 or 5
        using Ge = decltype(geo);
        if constexpr (Ge::K == 3 || Ge::K == 5)
            T4K_LAUNCH((k_conv_gemm_pool<Ge::K, Ge::S, Ge::P>), dim3(gs.gx, gs.gy), dim3(256), 0, hs, I, O, F, B, N, H1, W1, C1, H0, W0, C0, C0, gs.ppc, gs.ksplit, pe, xc);
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_conv2d_bwd(const float *I, const float *DO, float *DX, const float *F, float *DF, float *DB,
                   int N, int H1, int W1, int C1, int H0, int W0, int C0,
                   int K, int S, int P, int train, t4k_stream_t s) {
    return t4k_conv2d_bwd2(I, DO, DX, nullptr, F, DF, DB, N, H1, W1, C1, H0, W0, C0, K, S, P, train, s);
}

// DF == NULL: dX only (the caller runs dF|dB on another stream); DX == NULL: dF|dB only; DX2: optional second copy of dX from the same launch
int t4k_conv2d_bwd2(const float *I, const float *DO, float *DX, float *DX2, const float *F, float *DF, float *DB,
                    int N, int H1, int W1, int C1, int H0, int W0, int C0,
                    int K, int S, int P, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    ConvPlanScope plan;
    if (!conv_supported(K, S, P))
        return fail(T4K_ERR_UNSUPPORTED, "nn#bconv kernel_size=%d stride=%d padding=%d not supported", K, S, P);
    if (!I || !DO || !F || N <= 0 || H0 <= 0 || W0 <= 0) return fail(T4K_ERR_ARG, "t4k_conv2d_bwd: bad argument");
    if ((DF == nullptr) != (DB == nullptr)) return fail(T4K_ERR_ARG, "t4k_conv2d_bwd: DF and DB go together");
    FoldArgs pending = { nullptr, nullptr, nullptr, 0, 0, 0, 0 };
    if (train && DF) { int rc = conv_df_stage(I, DO, DF, DB, N, H1, W1, C1, H0, W0, C0, K, S, P, &pending, s); if (rc) return rc; }
    conv_dx_stage(DO, DX, DX2, F, N, H1, W1, C1, H0, W0, C0, K, S, P, pending, t4k::S(s));
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
