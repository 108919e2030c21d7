// conv_few.hip - convolution forward / dX for FEW channels on the vector ALUs: a thread (or a few lanes) per pixel, no MFMA.
// Image-input and LeNet-class layers are HBM / latency bound; padding 1..10 channels to the 32-wide MFMA tile wastes the matrix unit.
//   k_conv_few      forward / dX, Cin <= 4 and Cout <= 32, K 3 or 5
//   k_conv_dx_few   dX into C1 <= 4 input channels, every admitted geometry
//   k_conv_dx_wide  the same for 32 / 64 / 128 output channels (3x3): C0 / 4 lanes per pixel
// The two dX kernels carry the layer's dF fold in their first workgroups (FoldArgs, conv_types.h).
#include "conv_types.h"

namespace {

// ------------------------------------------------------------------ forward / dX for few channels (Cin, Cout <= 32)
// LeNet-class layers (1->10, 10->20 channels) are HBM/latency bound; padding 10 channels to the 32-wide MFMA tile and
// gathering one float per MFMA wastes the matrix unit.  A thread owns one output pixel x G output channels (G = 4 or 12
// accumulators; the channel group is uniform per workgroup, so filter reads are 16 B LDS broadcasts).  With < 1 wave per
// SIMD there is nothing to hide a load behind, so per image row of taps the thread first issues ALL its input loads
// (K taps x CH channels, unconditional: clamped address + select) and only then the FMAs: a 3x3x10 layer makes 6 memory
// round trips per pixel instead of 45.  Outputs leave through an LDS transpose so every store instruction is contiguous.
// The filter is staged once per workgroup as Wl[tap][ci][co] (taps flipped for dX, nmath.tcu:304-324).
template <int K, int S, int P, bool BWD, int G, int CH, int VW>
__global__ void __launch_bounds__(256) k_conv_few(const float *__restrict__ X, float *__restrict__ Y, float *__restrict__ Y2, float *__restrict__ XC,
                                                  const float *__restrict__ F, const float *__restrict__ B,
                                                  int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout, int C0f, int NG) {
    __shared__ __attribute__((aligned(16))) float Wl[LDS_FILTER_FLOATS];
    __shared__ float Os[256 * G];
    constexpr int KK = K * K;
    const int COPT = NG * G;
    {
        const int nF = (BWD ? Cout : Cin) * KK * C0f;
        for (int e = threadIdx.x; e < KK * Cin * COPT; e += 256) Wl[e] = 0.f;
        __syncthreads();
        for (int e = threadIdx.x; e < nF; e += 256) {
            const int c0 = e % C0f; const int r = e / C0f; const int t = r % KK; const int c1 = r / KK;   // F[c1][t][c0]
            if (!BWD) Wl[(t * Cin + c1) * COPT + c0] = F[e];                  // ci = c1, co = c0
            else      Wl[((KK - 1 - t) * Cin + c0) * COPT + c1] = F[e];       // ci = c0, co = c1, taps flipped
        }
        __syncthreads();
    }
    const int g = blockIdx.y, co0 = g * G;
    const int gv = min(G, Cout - co0);                           // valid channels of this group
    const long npix = (long)N * Hy * Wy;
    for (long pix0 = (long)blockIdx.x * 256; pix0 < npix; pix0 += (long)gridDim.x * 256) {
        const long pix = pix0 + threadIdx.x;
        const bool live = pix < npix;
        const long pc = live ? pix : 0;
        int x, y, n; split3(pc, Wy, Hy, x, y, n);
        float acc[G];
#pragma unroll
        for (int u = 0; u < G; u++) acc[u] = 0.f;
        const float *nX = X + (long)n * Hx * Wx * Cin;
#pragma unroll
        for (int ky = 0; ky < K; ky++) {
            int gi; bool iok;
            if (!BWD) { gi = y * S + ky - P; iok = gi >= 0 && gi < Hx; }
            else { const int ti = y + P - ky; gi = ti / S; iok = ti >= 0 && (ti % S) == 0 && gi < Hx; }
            const float *d[K]; bool ok[K];
#pragma unroll
            for (int kx = 0; kx < K; kx++) {
                int gj; bool jok;
                if (!BWD) { gj = x * S + kx - P; jok = gj >= 0 && gj < Wx; }
                else { const int tj = x + P - kx; gj = tj / S; jok = tj >= 0 && (tj % S) == 0 && gj < Wx; }
                ok[kx] = live && iok && jok;
                d[kx] = nX + (ok[kx] ? ((long)gi * Wx + gj) * Cin : 0);
            }
            for (int ci0 = 0; ci0 < Cin; ci0 += CH) {
                float v[K][CH];
#pragma unroll
                for (int kx = 0; kx < K; kx++)
#pragma unroll
                    for (int q = 0; q < CH; q += VW) {
                        const int ci = (ci0 + q < Cin) ? ci0 + q : 0;          // clamped: the load is unconditional
                        if (VW == 4)      { const float4 t4 = *reinterpret_cast<const float4 *>(d[kx] + ci); v[kx][q] = t4.x; v[kx][(q + 1) % CH] = t4.y; v[kx][(q + 2) % CH] = t4.z; v[kx][(q + 3) % CH] = t4.w; }
                        else if (VW == 2) { const float2 t2 = *reinterpret_cast<const float2 *>(d[kx] + ci); v[kx][q] = t2.x; v[kx][(q + 1) % CH] = t2.y; }
                        else              v[kx][q] = d[kx][ci];
                    }
#pragma unroll
                for (int kx = 0; kx < K; kx++)
#pragma unroll
                    for (int q = 0; q < CH; q++) {
                        const float xv = (ok[kx] && ci0 + q < Cin) ? v[kx][q] : 0.f;
                        const float *wq = Wl + (((ky * K + kx) * Cin) + min(ci0 + q, Cin - 1)) * COPT + co0;
#pragma unroll
                        for (int u4 = 0; u4 < G; u4 += 4) {
                            const float4 f4 = *reinterpret_cast<const float4 *>(wq + u4);
                            acc[u4] = fmaf(xv, f4.x, acc[u4]); acc[u4 + 1] = fmaf(xv, f4.y, acc[u4 + 1]);
                            acc[u4 + 2] = fmaf(xv, f4.z, acc[u4 + 2]); acc[u4 + 3] = fmaf(xv, f4.w, acc[u4 + 3]);
                        }
                    }
            }
        }
        if (XC && g == 0 && live)                               // layer 0 keeps a COPY of the batch (forward.cu:39): same-size conv, pixel index is shared
            for (int ci = 0; ci < Cin; ci++) XC[pix * Cin + ci] = X[pix * Cin + ci];
        // transpose through LDS: the workgroup's 256 x gv results leave as contiguous runs
        __syncthreads();
#pragma unroll
        for (int u = 0; u < G; u++) Os[threadIdx.x * G + u] = acc[u] + ((!BWD && B && co0 + u < Cout) ? B[co0 + u] : 0.f);
        __syncthreads();
        const int nval = (int)min((long)256, npix - pix0) * gv;
        for (int e = threadIdx.x; e < nval; e += 256) {
            const int pp = e / gv, u = e - pp * gv;
            const float r = Os[pp * G + u];
            const long o = (pix0 + pp) * Cout + co0 + u;
            Y[o] = r; if (Y2) Y2[o] = r;
        }
    }
}

// ------------------------------------------------------------------ dX for very few input channels (C1 <= 4)
// The first layer of an image net has 1 (MNIST) or 3 (CIFAR) input channels: as an implicit GEMM its dX would use 1/32
// of the matrix unit's N dimension and gather one float per MFMA.  Here a thread owns one pixel of the input grid and its
// CO accumulators, reads the C0 contiguous gradients of each tap's output pixel (adjacent lanes = adjacent pixels, so a
// wave streams a contiguous span of dO) and takes the flipped filter (nmath.tcu:304-324) from LDS at a wave-uniform address.
template <int K, int S, int P, int CO>
__device__ __forceinline__ void conv_dx_few_body(const float *__restrict__ DO, float *__restrict__ DX, float *__restrict__ DX2,
                                                 const float *__restrict__ F, int N, int H0, int W0, int C0, int H1, int W1, int bx, int gx) {
    __shared__ __attribute__((aligned(16))) float Fl[LDS_FILTER_FLOATS];
    const int nF = CO * K * K * C0;
    for (int e = threadIdx.x; e < nF; e += 256) Fl[e] = F[e];
    __syncthreads();
    const long npix = (long)N * H1 * W1;
    for (long pix = (long)bx * 256 + threadIdx.x; pix < npix; pix += (long)gx * 256) {
        int x, y, n; split3(pix, W1, H1, x, y, n);
        float acc[CO];
#pragma unroll
        for (int c = 0; c < CO; c++) acc[c] = 0.f;
        const float *nD = DO + (long)n * H0 * W0 * C0;
#pragma unroll
        for (int ky = 0; ky < K; ky++) {
            const int ti = y + P - ky, gi = ti / S;
            const bool iok = ti >= 0 && (ti % S) == 0 && gi < H0;
#pragma unroll
            for (int kx = 0; kx < K; kx++) {
                const int tj = x + P - kx, gj = tj / S;
                const bool ok = iok && tj >= 0 && (tj % S) == 0 && gj < W0;
                const float *d = nD + (ok ? ((long)gi * W0 + gj) * C0 : 0);
                const float *f = Fl + ((K - 1 - ky) * K + (K - 1 - kx)) * C0;     // F[c1][K-1-ky][K-1-kx][c0]
                if ((C0 & 3) == 0) {                              // 16 B loads of dO and of the weights (LDS rows are 16 B aligned: C0 % 4 == 0)
#pragma unroll 4
                    for (int c0 = 0; c0 < C0; c0 += 4) {
                        const float4 v4 = *reinterpret_cast<const float4 *>(d + c0);
                        const float v0 = ok ? v4.x : 0.f, v1 = ok ? v4.y : 0.f, v2 = ok ? v4.z : 0.f, v3 = ok ? v4.w : 0.f;
#pragma unroll
                        for (int c = 0; c < CO; c++) {
                            const float4 w4 = *reinterpret_cast<const float4 *>(f + c * K * K * C0 + c0);
                            acc[c] = fmaf(v0, w4.x, acc[c]); acc[c] = fmaf(v1, w4.y, acc[c]); acc[c] = fmaf(v2, w4.z, acc[c]); acc[c] = fmaf(v3, w4.w, acc[c]);
                        }
                    }
                } else if ((C0 & 1) == 0) {                       // even channel count: 8 B loads (pixel rows are 8 B aligned)
#pragma unroll 5
                    for (int c0 = 0; c0 < C0; c0 += 2) {
                        const float2 v2 = *reinterpret_cast<const float2 *>(d + c0);
                        const float v0 = ok ? v2.x : 0.f, v1 = ok ? v2.y : 0.f;
#pragma unroll
                        for (int c = 0; c < CO; c++) { acc[c] = fmaf(v0, f[c * K * K * C0 + c0], acc[c]); acc[c] = fmaf(v1, f[c * K * K * C0 + c0 + 1], acc[c]); }
                    }
                } else {
                    for (int c0 = 0; c0 < C0; c0++) {
                        const float v0 = d[c0], v = ok ? v0 : 0.f;
#pragma unroll
                        for (int c = 0; c < CO; c++) acc[c] = fmaf(v, f[c * K * K * C0 + c0], acc[c]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CO; c++) { DX[pix * CO + c] = acc[c]; if (DX2) DX2[pix * CO + c] = acc[c]; }
    }
}
template <int K, int S, int P, int CO>
__global__ void __launch_bounds__(256) k_conv_dx_few(const float *__restrict__ DO, float *__restrict__ DX, float *__restrict__ DX2,
                                                     const float *__restrict__ F, int N, int H0, int W0, int C0, int H1, int W1, FoldArgs fa) {
    const int b = blockIdx.x;
    if (b < fa.nfold) conv_df_fold_body(fa.part, fa.DF, fa.DB, fa.nslice, fa.ndf, fa.ntot, b);
    else conv_dx_few_body<K, S, P, CO>(DO, DX, DX2, F, N, H0, W0, C0, H1, W1, b - fa.nfold, (int)gridDim.x - fa.nfold);
}
// Same layer shape (C1 = CO <= 4 input channels) but MANY output channels (C0 = 32 / 64 / 128, e.g. the 3 -> 64 first layer of a
// CIFAR net): with a thread per pixel every lane walks its own 4*C0-byte run of dO, a wave touches 64 different runs per load and
// the L1 thrashes (90 us for N=256, 32x32, 3->64 = 6 % of the vector peak).  Here LPP = C0/4 lanes share a pixel, lane q owns
// channels 4q..4q+3: a load instruction reads whole pixels (fully coalesced 16 B per lane), the lane's 4 x 9 x CO weights live in
// registers for the whole grid-stride loop, and the LPP partial sums meet through an xor tree.  3x3, stride 1 only.
template <int CO, int LPP>
__device__ __forceinline__ void conv_dx_wide_body(const float *__restrict__ DO, float *__restrict__ DX, float *__restrict__ DX2,
                                                  const float *__restrict__ F, int N, int H0, int W0, int H1, int W1, int bx, int gx) {
    constexpr int K = 3, KK = 9, C0 = LPP * 4, PPW = 64 / LPP, PPB = 4 * PPW;    // pixels per wave / per workgroup
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = lane % LPP, sub = lane / LPP;
    float4 wt[CO][KK];                                                           // F[c1][K-1-ky][K-1-kx][4q..4q+3]
#pragma unroll
    for (int c = 0; c < CO; c++)
#pragma unroll
        for (int t = 0; t < KK; t++) wt[c][t] = *reinterpret_cast<const float4 *>(F + ((long)c * KK + (KK - 1 - t)) * C0 + 4 * q);
    const long npix = (long)N * H1 * W1;
    for (long p0 = (long)bx * PPB; p0 < npix; p0 += (long)gx * PPB) {
        const long pix = p0 + w * PPW + sub;
        const bool live = pix < npix;
        int x, y, n; split3(live ? pix : 0, W1, H1, x, y, n);
        const float *nD = DO + (long)n * H0 * W0 * C0 + 4 * q;
        float4 v[KK]; bool ok[KK];
#pragma unroll
        for (int ky = 0; ky < K; ky++)
#pragma unroll
            for (int kx = 0; kx < K; kx++) {
                const int gi = y + 1 - ky, gj = x + 1 - kx;                       // P = 1, S = 1
                ok[ky * K + kx] = live && gi >= 0 && gi < H0 && gj >= 0 && gj < W0;
                v[ky * K + kx] = *reinterpret_cast<const float4 *>(nD + (ok[ky * K + kx] ? ((long)gi * W0 + gj) * C0 : 0));   // unconditional
            }
        float acc[CO];
#pragma unroll
        for (int c = 0; c < CO; c++) acc[c] = 0.f;
#pragma unroll
        for (int t = 0; t < KK; t++) {
            const float v0 = ok[t] ? v[t].x : 0.f, v1 = ok[t] ? v[t].y : 0.f, v2 = ok[t] ? v[t].z : 0.f, v3 = ok[t] ? v[t].w : 0.f;
#pragma unroll
            for (int c = 0; c < CO; c++) {
                acc[c] = fmaf(v0, wt[c][t].x, acc[c]); acc[c] = fmaf(v1, wt[c][t].y, acc[c]);
                acc[c] = fmaf(v2, wt[c][t].z, acc[c]); acc[c] = fmaf(v3, wt[c][t].w, acc[c]);
            }
        }
#pragma unroll
        for (int off = LPP / 2; off > 0; off >>= 1)
#pragma unroll
            for (int c = 0; c < CO; c++) acc[c] += __shfl_xor(acc[c], off, 64);
        if (live && q == 0) {
#pragma unroll
            for (int c = 0; c < CO; c++) { DX[pix * CO + c] = acc[c]; if (DX2) DX2[pix * CO + c] = acc[c]; }
        }
    }
}
template <int CO, int LPP>
__global__ void __launch_bounds__(256) k_conv_dx_wide(const float *__restrict__ DO, float *__restrict__ DX, float *__restrict__ DX2,
                                                      const float *__restrict__ F, int N, int H0, int W0, int H1, int W1, FoldArgs fa) {
    const int b = blockIdx.x;
    if (b < fa.nfold) conv_df_fold_body(fa.part, fa.DF, fa.DB, fa.nslice, fa.ndf, fa.ntot, b);
    else conv_dx_wide_body<CO, LPP>(DO, DX, DX2, F, N, H0, W0, H1, W1, b - fa.nfold, (int)gridDim.x - fa.nfold);
}

// dX with 16-byte loads of whole pixels: 3x3, stride 1, a tile or more of output channels, both operands aligned
bool dx_wide(int K, int S, int P, int C0, const float *DO, const float *F) {
    return conv_lab().dx_wide && K == 3 && S == 1 && P == 1 && (C0 == 32 || C0 == 64 || C0 == 128) && aligned16(DO) && aligned16(F);
}

} // namespace

namespace t4k {

bool conv_few_ok(int K, int Cin, int Cout, int *G_out, int *NG_out) {
    // measured on MI355X: wins for image-input layers (1->10: 6.1 vs 8.4 us); at 10<->20 channels the thread-per-pixel
    // kernel is FMA/LDS bound with < 1 wave per SIMD and loses to the MFMA implicit GEMM (13.9 vs 10.3 us)
    if (Cin > 4 || Cout > 32 || (K != 3 && K != 5)) return false;
    const int G = Cout <= 4 ? 4 : 12;
    const int NG = (Cout + G - 1) / G;
    if (K * K * Cin * NG * G > LDS_FILTER_FLOATS) return false;
    *G_out = G; *NG_out = NG;
    return true;
}
template <bool BWD>
void launch_conv_few(int K, hipStream_t hs, const float *X, float *Y, float *Y2, float *XC, const float *F, const float *B,
                     int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout, int C0f, int G, int NG) {
    const long npix = (long)N * Hy * Wy;
    long gx = (npix + 255) / 256; if (gx > 8192) gx = 8192;
    const dim3 g((unsigned)gx, (unsigned)NG), b(256);
    const bool v2 = (Cin & 1) == 0 && (((uintptr_t)X) & 7) == 0;
    // conv_few_ok() admits K 3 / 5 and Cin <= 4: one channel per trip for Cin == 1, else four, loaded in pairs where the input allows
    pick<4, 12>(G, [&](auto gg) {
        auto go = [&](auto geo, auto ch, auto vw) {
            using Ge = decltype(geo);
            T4K_LAUNCH((k_conv_few<Ge::K, Ge::S, Ge::P, BWD, decltype(gg)::value, decltype(ch)::value, decltype(vw)::value>), g, b, 0, hs,
                       X, Y, Y2, XC, F, B, N, Hx, Wx, Cin, Hy, Wy, Cout, C0f, NG);
        };
        auto geo = [&](auto ch, auto vw) { if (K == 3) go(Geo<3, 1, 1>{}, ch, vw); else go(Geo<5, 1, 2>{}, ch, vw); };
        conv_plan_note("%s<%d,%d,%d>", BWD ? "fewch" : "few", G, Cin == 1 ? 1 : 4, Cin == 1 ? 1 : v2 ? 2 : 1);
        if (Cin == 1) geo(int_c<1>{}, int_c<1>{});
        else if (v2)  geo(int_c<4>{}, int_c<2>{});
        else          geo(int_c<4>{}, int_c<1>{});
    });
}
template void launch_conv_few<false>(int, hipStream_t, const float *, float *, float *, float *, const float *, const float *, int, int, int, int, int, int, int, int, int, int);
template void launch_conv_few<true>(int, hipStream_t, const float *, float *, float *, float *, const float *, const float *, int, int, int, int, int, int, int, int, int, int);

bool conv_dx_few_ok(int K, int C1, int C0, const float *DO) {
    const uintptr_t need = (C0 & 3) == 0 ? 15 : (C0 & 1) == 0 ? 7 : 3;       // the widest load k_conv_dx_few makes of a dO pixel row (a row starts C0 floats after the last)
    return C1 <= 4 && C1 * K * K * C0 <= LDS_FILTER_FLOATS && (((uintptr_t)DO) & need) == 0;
}

void launch_conv_dx_few(int K, int S, int P, hipStream_t hs, const float *DO, float *DX, float *DX2, const float *F,
                        int N, int H0, int W0, int C0, int H1, int W1, int C1, FoldArgs fa) {
    const long npix = (long)N * H1 * W1;
    pick<1, 2, 3, 4>(C1, [&](auto co) {
        constexpr int CO = decltype(co)::value;
        if (dx_wide(K, S, P, C0, DO, F)) {
            const int ppb = 4 * (64 / (C0 / 4));
            long gw = (npix + ppb - 1) / ppb; if (gw > (long)st().cu_count * conv_lab().dx_wide_wpc) gw = (long)st().cu_count * conv_lab().dx_wide_wpc;
            const dim3 gg((unsigned)gw + fa.nfold), bb(256);
            conv_plan_note("dx_wide<%d>%s", C0 / 4, fa.nfold ? "+fold" : "");
            pick<8, 16, 32>(C0 / 4, [&](auto lpp) { T4K_LAUNCH((k_conv_dx_wide<CO, decltype(lpp)::value>), gg, bb, 0, hs, DO, DX, DX2, F, N, H0, W0, H1, W1, fa); });
            return;
        }
        long gx = (npix + 255) / 256; if (gx > 8192) gx = 8192;
        const dim3 g((unsigned)gx + fa.nfold), b(256);
        conv_plan_note("dx_few%s", fa.nfold ? "+fold" : "");
        with_geometry(K, S, P, [&](auto geo) {
            using Ge = decltype(geo);
            T4K_LAUNCH((k_conv_dx_few<Ge::K, Ge::S, Ge::P, CO>), g, b, 0, hs, DO, DX, DX2, F, N, H0, W0, C0, H1, W1, fa);
        });
    });
}

} // namespace t4k
