// patch.hip - patch embedding: conv2d with K == S, no padding, K 2..32 (t4k_patch_fwd / _bwd / _plan).
//
// Non-overlapping windows make the layer a plain GEMM, [M = N H0 W0 tokens] x [Kd = K K C1] x [C0], whose A rows are K runs of R = K C1 contiguous floats of
// the NHWC image: the k-index runs over (ky, kx, c1) with c1 fastest, so k = ky R + j and element k of token t is I[tb(t) + ky W1 C1 + j].  The matching
// filter row of F = T4(C1, K, K, C0) is ((c1 K + ky) K + kx) with kx = j / C1, c1 = j % C1 - the summation index is permuted on both operands alike.
// A k-step is 32 CONSECUTIVE k: every lane of it holds a pixel for any C1 (conv_geo.hip's k-step, 32 channels of one tap, would hold 3 of 32 at C1 = 3).
// Three products, exact fp32 on v_mfma_f32_32x32x2_f32:
//   forward  O[t, c0]  = B[c0] + sum_k A[t, k] F[row(k), c0]                 k_patch<false>: 128 tokens x BN channels, 32 k a stage
//   dX       dX[t, k]  = sum_c0 dO[t, c0] F[row(k), c0]                      k_patch<true>:  128 tokens x BN columns k, 32 c0 a stage; column k is stored
//                                                                            at tb(t) + ky W1 C1 + j - every covered pixel once -, and the workgroups
//                                                                            behind the tiles store 0 to the rows / columns past H0 K, W0 K
//   dF | dB  slab[slice][row(k) | bias][c0] = sum_{t of the slice} A[t, k] dO[t, c0]     k_patch_df: 64 columns k x 64 c0 on conv_tile.h's conv_df_tile4
//                                                                            (both operands token-major), one spare column whose A operand is 1: dB
// The slabs live in the workspace half the run-time-geometry layers use and are folded by colsum.h's two folds (conv_types.h's slab_plan picks the slices).
// 16-byte loads where the run and the image row are multiples of 4 floats (I) / C0 is (F, dO) and the pointer sits on 16 bytes; dwords otherwise.
// No atomics, a fixed summation order, nothing outside the tensors is read or written.
#include "conv_tile.h"
#include "fastdiv.h"

namespace {

constexpr int PBM = 128, PBK = 32, PCH = PBK / 4, PSW = 64 / PBK;

struct PatP {
    const float *X, *F, *B;            // A operand (forward: I, dX: dO), filter, bias (forward)
    float *Y, *Y2;                     // produced tensor (+ optional second copy, dX)
    int N, H1, W1, C1, C0, K, H0, W0;
    int R, Kd, M;                      // run K C1, contraction K K C1, tokens N H0 W0
    int tiles_n, nst, tiles;           // column tiles, k-steps, tile workgroups (the workgroups behind them zero dX's uncovered pixels)
    FastDiv dR, dC1, dW0, dH0;
};

// k -> where element k of a token lies behind the token's first pixel
__device__ __forceinline__ int patch_aoff(int k, int R, int rowp, const FastDiv &dR) { const int ky = (int)fdiv((unsigned)k, dR); return ky * rowp + (k - ky * R); }
// k -> its filter row (c1 K + ky) K + kx
__device__ __forceinline__ int patch_frow(int k, int R, int C1, int K, const FastDiv &dR, const FastDiv &dC1) {
    const int ky = (int)fdiv((unsigned)k, dR), j = k - ky * R, kx = (int)fdiv((unsigned)j, dC1), c1 = j - kx * C1;
    return (c1 * K + ky) * K + kx;
}
// token -> offset of its first pixel in the image tensor (below 2^31: the admission)
__device__ __forceinline__ int patch_tbase(unsigned t, const PatP &p) {
    const unsigned q = fdiv(t, p.dW0), n = fdiv(q, p.dH0);
    const int pw = (int)(t - q * (unsigned)p.W0), ph = (int)(q - n * (unsigned)p.H0);
    return (((int)n * p.H1 + ph * p.K) * p.W1 + pw * p.K) * p.C1;
}

template <bool BWD, bool VA, bool VB, int BN>
__global__ void __launch_bounds__(256) k_patch(PatP p) {
    constexpr int BM = PBM, BK = PBK, CH = PCH, SW = PSW, MT = BM / 64, NT = BN / 64;
    constexpr int PA = BM * BK / 1024, PB = BN * BK / 1024;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ __attribute__((aligned(16))) int s_tb[BM];            // first pixel of the tile's tokens, -1 past the last (512 bytes: the stage buffers stay on 16)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int R = p.R, Kd = p.Kd, C0 = p.C0, rowp = p.W1 * p.C1;
    if (BWD && (int)blockIdx.x >= p.tiles) {                          // dX: rows from H0 K and columns from W0 K of every image get 0
        const long HK = (long)p.H0 * p.K, WK = (long)p.W0 * p.K;
        const long za = ((long)p.H1 - HK) * rowp, cw = ((long)p.W1 - WK) * p.C1, zper = za + HK * cw, total = (long)p.N * zper, img = (long)p.H1 * rowp;
        const long step = (long)((int)gridDim.x - p.tiles) * 256;
        for (long i = (long)((int)blockIdx.x - p.tiles) * 256 + tid; i < total; i += step) {
            const long n = i / zper; long r = i - n * zper, a;
            if (r < za) a = n * img + HK * rowp + r;
            else { r -= za; const long y = r / cw; a = n * img + y * rowp + WK * p.C1 + (r - y * cw); }
            p.Y[a] = 0.f; if (p.Y2) p.Y2[a] = 0.f;
        }
        return;
    }
    float *sA = lds, *sB = lds + 2 * BM * BK;
    const int wm = w >> 1, wn = w & 1, h = lane >> 5, l31 = lane & 31;
    const int tn = blockIdx.x % p.tiles_n, tm = blockIdx.x / p.tiles_n;
    const long m0 = (long)tm * BM;
    const int n0 = tn * BN;
    const int Kc = BWD ? C0 : Kd, Nc = BWD ? Kd : C0;                // contraction length, columns
    if (tid < BM) s_tb[tid] = m0 + tid < p.M ? patch_tbase((unsigned)(m0 + tid), p) : -1;
    __syncthreads();

    // this thread's A rows (tokens) and its 16-byte chunk of a k-step
    long abase[PA];
    const int aq = tid % CH;
#pragma unroll
    for (int pp = 0; pp < PA; pp++) {
        const int row = pp * (256 / CH) + tid / CH;
        abase[pp] = BWD ? (m0 + row < p.M ? (m0 + row) * C0 : -1L) : (long)s_tb[row];
    }
    long brow[PB];                                                   // dX: the filter row of this thread's columns
    if (BWD) {
#pragma unroll
        for (int pp = 0; pp < PB; pp++) {
            const int n = n0 + (pp * 256 + tid) / CH;
            brow[pp] = n < Kd ? (long)patch_frow(n, R, p.C1, p.K, p.dR, p.dC1) * C0 : -1L;
        }
    }
    v4f ra[PA], rb[PB];
    auto load_tiles = [&](int kt) __attribute__((always_inline)) {
        const v4f z = {0.f, 0.f, 0.f, 0.f};
        const int k = kt * BK + aq * 4;
        if (VA) {                                                    // (R % 4 == 0: the four k of a chunk lie in one run)
            const int off = BWD ? k : patch_aoff(k, R, rowp, p.dR);
#pragma unroll
            for (int pp = 0; pp < PA; pp++) ra[pp] = (k < Kc && abase[pp] >= 0) ? *reinterpret_cast<const v4f *>(p.X + abase[pp] + off) : z;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bool ok = k + e < Kc;
                const int off = BWD ? k + e : (ok ? patch_aoff(k + e, R, rowp, p.dR) : 0);
#pragma unroll
                for (int pp = 0; pp < PA; pp++) ra[pp][e] = (ok && abase[pp] >= 0) ? p.X[abase[pp] + off] : 0.f;
            }
        }
#pragma unroll
        for (int pp = 0; pp < PB; pp++) {
            const int id = pp * 256 + tid;
            if (!BWD) {                                              // B[k][n = c0] = F[row(k)][c0]: n-contiguous
                const int kk = kt * BK + id / (BN / 4), n = n0 + (id % (BN / 4)) * 4;
                const bool ok = kk < Kd;
                const float *src = p.F + (ok ? (long)patch_frow(kk, R, p.C1, p.K, p.dR, p.dC1) * C0 : 0L) + n;
                if (VB) rb[pp] = (ok && n < C0) ? *reinterpret_cast<const v4f *>(src) : z;
                else {
#pragma unroll
                    for (int e = 0; e < 4; e++) rb[pp][e] = (ok && n + e < C0) ? src[e] : 0.f;
                }
            } else {                                                 // B[n = k][c0] = F[row(k)][c0]: contraction-contiguous
                const int c = kt * BK + (id % CH) * 4;
                const float *src = p.F + (brow[pp] >= 0 ? brow[pp] : 0L) + c;
                if (VB) rb[pp] = (brow[pp] >= 0 && c < C0) ? *reinterpret_cast<const v4f *>(src) : z;
                else {
#pragma unroll
                    for (int e = 0; e < 4; e++) rb[pp][e] = (brow[pp] >= 0 && c + e < C0) ? src[e] : 0.f;
                }
            }
        }
    };
    // A rows (and dX's B rows) at pitch 32 with the 16-byte chunk xor-ed by row / 2: the 32 rows a fragment read touches spread over every bank
    int soa[PA], sob[PB];
#pragma unroll
    for (int pp = 0; pp < PA; pp++) { const int id = pp * 256 + tid, r = id / CH, q = id % CH; soa[pp] = r * BK + ((q ^ ((r / SW) & (CH - 1))) << 2); }
#pragma unroll
    for (int pp = 0; pp < PB; pp++) {
        const int id = pp * 256 + tid;
        if (BWD) { const int r = id / CH, q = id % CH; sob[pp] = r * BK + ((q ^ ((r / SW) & (CH - 1))) << 2); }
        else     sob[pp] = (id / (BN / 4)) * BN + (id % (BN / 4)) * 4;
    }
    auto store_tiles = [&](int buf) __attribute__((always_inline)) {
        float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
        for (int pp = 0; pp < PA; pp++) *reinterpret_cast<v4f *>(a + soa[pp]) = ra[pp];
#pragma unroll
        for (int pp = 0; pp < PB; pp++) *reinterpret_cast<v4f *>(b + sob[pp]) = rb[pp];
    };
    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    const int nst = p.nst;
    if (nst > 0) { load_tiles(0); store_tiles(0); }
    __syncthreads();
    for (int kt = 0; kt < nst; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nst) load_tiles(kt + 1);                        // in flight during the MFMAs below
        const float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
        for (int ci = 0; ci < BK / 8; ci++) {                        // lane half h holds k = 8 ci + 4 h + {0..3}
            float av[MT][4], bv[NT][4];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int r = wm * (BM / 2) + mt * 32 + l31;
                const v4f t = *reinterpret_cast<const v4f *>(a + r * BK + (((ci * 2 + h) ^ ((r / SW) & (CH - 1))) << 2));
                av[mt][0] = t[0]; av[mt][1] = t[1]; av[mt][2] = t[2]; av[mt][3] = t[3];
            }
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const int r = wn * (BN / 2) + nt * 32 + l31;
                if (BWD) { const v4f t = *reinterpret_cast<const v4f *>(b + r * BK + (((ci * 2 + h) ^ ((r / SW) & (CH - 1))) << 2));
                           bv[nt][0] = t[0]; bv[nt][1] = t[1]; bv[nt][2] = t[2]; bv[nt][3] = t[3]; }
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) bv[nt][j] = b[(ci * 8 + 4 * h + j) * BN + r];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int nt = 0; nt < NT; nt++)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][j], bv[nt][j], acc[mt][nt], 0, 0, 0);
        }
        if (kt + 1 < nst) store_tiles(buf ^ 1);
        __syncthreads();
    }
    // epilogue: column = lane & 31, row = frag_row(r, h).  Forward: the bias rides here, O[token][c0]; dX: column k goes to its place behind the token's first pixel
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const int gn = n0 + wn * (BN / 2) + nt * 32 + l31;
            if (gn >= Nc) continue;
            const float bias = BWD ? 0.f : p.B[gn];
            const int coff = BWD ? patch_aoff(gn, R, rowp, p.dR) : 0;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int row = wm * (BM / 2) + mt * 32 + frag_row(r, h), tb = s_tb[row];
                if (tb < 0) continue;
                if (BWD) { const long a = (long)tb + coff; p.Y[a] = acc[mt][nt][r]; if (p.Y2) p.Y2[a] = acc[mt][nt][r]; }
                else p.Y[(m0 + row) * C0 + gn] = acc[mt][nt][r] + bias;
            }
        }
}

// ------------------------------------------------------------------ dF | dB partial slabs
// grid = (slices, column tiles of k, c0 tiles); tile 64 k x 64 c0, the contraction = the slice's tokens, 32 a stage.  Both operands are token-major with
// their tile extent contiguous - 64 k of a token are (pieces of) its runs, 64 c0 of a token a piece of its dO row - which is conv_df_tile4's layout.
// A thread keeps one 16-byte chunk of k (decoded once) and two tokens of the stage.  Column Kd is the bias column: its A operand is 1.
// Every element of every slab is stored (an empty slice stores zeros), at the FILTER's row of its k.
struct PatD { const float *I, *DO; float *part; int N, H1, W1, C1, C0, K, H0, W0, R, Kd, M, pps; FastDiv dR, dC1, dW0, dH0; };

template <bool VA, bool VB>
__global__ void __launch_bounds__(256) k_patch_df(PatD p) {
    constexpr int BM = 64, BN = 64, BKP = 32;
    __shared__ __attribute__((aligned(16))) float sA[2][BKP * BM];
    __shared__ __attribute__((aligned(16))) float sB[2][BKP * BN];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, h = lane >> 5, l31 = lane & 31;
    const int Kd = p.Kd, C0 = p.C0, rowp = p.W1 * p.C1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.z * BN;
    const long k_beg = (long)blockIdx.x * p.pps, k_end = min((long)p.M, k_beg + p.pps);
    const int nst = k_end > k_beg ? (int)((k_end - k_beg + BKP - 1) / BKP) : 0;
    const int rq = tid & 15, kq = tid >> 4;                          // this thread's 16-byte column of a stage row, and its rows kq, kq + 16
    int aoff[4];                                                     // where k = m0 + 4 rq + e lies behind a token's first pixel; -1 the bias column, -2 none
#pragma unroll
    for (int e = 0; e < 4; e++) { const int k = m0 + rq * 4 + e; aoff[e] = k < Kd ? patch_aoff(k, p.R, rowp, p.dR) : (k == Kd ? -1 : -2); }
    v4f ra[2], rb[2];
    auto load_tiles = [&](int kt) __attribute__((always_inline)) {
        const long k0 = k_beg + (long)kt * BKP;
        const v4f z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            const long t = k0 + kq + pp * 16;
            const bool in = t < k_end;
            const unsigned tt = in ? (unsigned)t : 0u, q = fdiv(tt, p.dW0), n = fdiv(q, p.dH0);
            const int pw = (int)(tt - q * (unsigned)p.W0), ph = (int)(q - n * (unsigned)p.H0);
            const float *src = p.I + (((int)n * p.H1 + ph * p.K) * p.W1 + pw * p.K) * p.C1;
            if (VA && aoff[0] >= 0) ra[pp] = in ? *reinterpret_cast<const v4f *>(src + aoff[0]) : z;      // (Kd % 4 == 0: a chunk is whole or behind the end)
            else {
#pragma unroll
                for (int e = 0; e < 4; e++) ra[pp][e] = !in ? 0.f : aoff[e] >= 0 ? src[aoff[e]] : aoff[e] == -1 ? 1.f : 0.f;
            }
            const int n1 = n0 + rq * 4;
            if (VB) rb[pp] = (in && n1 < C0) ? *reinterpret_cast<const v4f *>(p.DO + t * C0 + n1) : z;
            else {
#pragma unroll
                for (int e = 0; e < 4; e++) rb[pp][e] = (in && n1 + e < C0) ? p.DO[t * C0 + n1 + e] : 0.f;
            }
        }
    };
    auto store_tiles = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            *reinterpret_cast<v4f *>(&sA[buf][(kq + pp * 16) * BM + rq * 4]) = ra[pp];
            *reinterpret_cast<v4f *>(&sB[buf][(kq + pp * 16) * BN + rq * 4]) = rb[pp];
        }
    };
    f32x16 acc0, acc1;
    conv_df_tile4(&sA[0][0], &sB[0][0], nst, acc0, acc1, load_tiles, store_tiles);
    // slab [slice][filter row | bias row][c0] (the fold's layout: outputs [0, Kd C0) are dF, the C0 behind them dB)
    const int co = n0 + wn * 32 + l31;
    if (co < C0) {
        const long ntot = ((long)Kd + 1) * C0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int k = m0 + wm * 32 + frag_row(r, h);
            if (k > Kd) continue;
            const int row = k < Kd ? patch_frow(k, p.R, p.C1, p.K, p.dR, p.dC1) : Kd;
            p.part[(long)blockIdx.x * ntot + (long)row * C0 + co] = acc0[r] + acc1[r];
        }
    }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_patch_plan reports
struct PatchPlan {
    int H0, W0, R, Kd, M;
    int fwd_bn, fwd_va, fwd_vb;        // forward: channel tile (the token tile is 128), 16-byte gather of I, 16-byte loads of F
    int dx_bn, dx_v;                   // dX: column tile, 16-byte loads of dO and F
    int df_va, df_vb, nslice, pps, fold;    // dF: 16-byte gather of I, 16-byte loads of dO, slices, tokens per slice, the fold (1 fold_add, 2 df_fold)
    int zero_wg;                       // dX: workgroups behind the tiles that zero the uncovered pixels
};
// aligned: bit 0 I, bit 1 F, bit 2 dO on 16 bytes; bit 3: DB does NOT lie right behind DF
constexpr int PAL_I = 1, PAL_F = 2, PAL_DO = 4, PAL_DB_APART = 8;
// admission (who: the entry's name for the message) and the plan.  T4K_ERR_ARG: an extent below 1; T4K_ERR_UNSUPPORTED: anything else outside the admitted set.
// Every product is formed in 64 bits behind a test that bounds it: the extents may be anything an int holds
int patch_plan(PatchPlan &g, const char *who, int N, int H1, int W1, int C1, int C0, int K, int aligned) {
    if (N < 1 || H1 < 1 || W1 < 1 || C1 < 1 || C0 < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (N=%d H1=%d W1=%d C1=%d C0=%d)", who, N, H1, W1, C1, C0);
    if (K < 2 || K > 32) return fail(T4K_ERR_UNSUPPORTED, "%s: kernel_size=%d stride=%d padding=0 not supported (K 2..32)", who, K, K);
    if (H1 < K || W1 < K) return fail(T4K_ERR_UNSUPPORTED, "%s: the %dx%d patch does not fit the %dx%d image", who, K, K, H1, W1);
    g.H0 = H1 / K; g.W0 = W1 / K;
    const long lim = 1L << 31;
    long a = (long)N * H1, b = (long)N * g.H0;
    if (a >= lim || (a *= W1) >= lim || (a *= C1) >= lim || (b *= g.W0) >= lim || b * C0 >= lim)      // (b < 2^31 and C0 < 2^31: the last product fits)
        return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 elements or more in the image or in the token tensor", who);
    const long rows = (long)K * K * C1 + 1;
    if (rows > (long)(CONV_WS_BYTES / sizeof(float)) / C0) return fail(T4K_ERR_UNSUPPORTED, "%s: one dF | dB slab (%ld x %d floats) does not fit the workspace", who, rows, C0);
    g.R = K * C1; g.Kd = K * g.R; g.M = (int)b;
    const long tm = (b + PBM - 1) / PBM, tdf = (g.Kd + 64) / 64;
    if (tdf > 65535 || (C0 + 63) / 64 > 65535 || tm * ((C0 + 63) / 64) >= lim || tm * ((g.Kd + 63) / 64) + 256 >= lim)
        return fail(T4K_ERR_UNSUPPORTED, "%s: more tiles than a launch takes", who);
    const bool vi = (aligned & PAL_I) && g.R % 4 == 0 && ((long)W1 * C1) % 4 == 0;
    const bool vf = (aligned & PAL_F) && C0 % 4 == 0, vd = (aligned & PAL_DO) && C0 % 4 == 0;
    g.fwd_va = vi; g.fwd_vb = vf;
    g.fwd_bn = (vi && vf && C0 > 64) ? 128 : 64;
    g.dx_v = vf && vd;
    g.dx_bn = (g.dx_v && g.Kd > 64) ? 128 : 64;
    g.df_va = vi; g.df_vb = vd;
    const SlabPlan sp = slab_plan(b, tdf * ((C0 + 63) / 64), rows * C0, !(aligned & PAL_DB_APART), 0x7fffffe0);     // (PatD::pps is an int)
    g.pps = (int)sp.pps; g.nslice = sp.nslice; g.fold = sp.fold;
    const long zeros = (long)N * ((long)H1 * W1 - (long)g.H0 * K * g.W0 * K) * C1;
    g.zero_wg = (int)std::min((zeros + 1023) / 1024, 256L);
    return T4K_OK;
}

template <typename P> void patch_divs(P &p) { p.dR = fast_div(p.R); p.dC1 = fast_div(p.C1); p.dW0 = fast_div(p.W0); p.dH0 = fast_div(p.H0); }

template <bool BWD>
void launch_patch(const PatP &p, bool va, bool vb, int bn, int zero_wg, hipStream_t hs) {
    const dim3 grid((unsigned)p.tiles + (unsigned)zero_wg);
    const size_t lds = (size_t)2 * (PBM + bn) * PBK * sizeof(float);
    if (bn == 128) { launch_lds<k_patch<BWD, true, true, 128>>(grid, dim3(256), lds, hs, p); return; }
    if constexpr (BWD) with_flags([&](auto v) { launch_lds<k_patch<BWD, v.value, v.value, 64>>(grid, dim3(256), lds, hs, p); }, va);
    else               with_flags([&](auto a, auto b) { launch_lds<k_patch<BWD, a.value, b.value, 64>>(grid, dim3(256), lds, hs, p); }, va, vb);
}

} // namespace

extern "C" {

int t4k_patch_plan(int N, int H1, int W1, int C1, int C0, int K, int aligned, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_patch_plan: null");
    PatchPlan g;
    const int rc = patch_plan(g, "t4k_patch_plan", N, H1, W1, C1, C0, K, aligned); if (rc != T4K_OK) return rc;
    out[0] = g.fwd_bn; out[1] = g.fwd_va | (g.fwd_vb << 1);
    out[2] = g.dx_bn;  out[3] = g.dx_v;
    out[4] = g.df_va | (g.df_vb << 1); out[5] = g.nslice; out[6] = g.fold; out[7] = 3;
    return T4K_OK;
}

int t4k_patch_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B, int N, int H1, int W1, int C1, int C0, int K, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    ConvPlanScope plan;
    if (!I || !O || !F || !B) return fail(T4K_ERR_ARG, "t4k_patch_fwd: null tensor");
    PatchPlan g;
    const int rc = patch_plan(g, "t4k_patch_fwd", N, H1, W1, C1, C0, K, (aligned16(I) ? PAL_I : 0) | (aligned16(F) ? PAL_F : 0)); if (rc != T4K_OK) return rc;
    hipStream_t hs = t4k::S(s);
    if (ICOPY) { conv_plan_note("memcpy"); T4K_HIP(hipMemcpyAsync(ICOPY, I, sizeof(float) * (size_t)N * H1 * W1 * C1, hipMemcpyDeviceToDevice, hs)); }
    PatP p = { I, F, B, O, nullptr, N, H1, W1, C1, C0, K, g.H0, g.W0, g.R, g.Kd, g.M };
    p.tiles_n = (C0 + g.fwd_bn - 1) / g.fwd_bn; p.nst = (g.Kd + PBK - 1) / PBK; p.tiles = (g.M + PBM - 1) / PBM * p.tiles_n;
    patch_divs(p);
    conv_plan_note("patch<%d,%s,%s>", g.fwd_bn, g.fwd_va ? "v4" : "v1", g.fwd_vb ? "f4" : "f1");
    launch_patch<false>(p, g.fwd_va, g.fwd_vb, g.fwd_bn, 0, hs);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_patch_bwd(const float *I, const float *DO, float *DX, float *DX2, const float *F, float *DF, float *DB,
                  int N, int H1, int W1, int C1, int C0, int K, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    ConvPlanScope plan;
    if (!I || !DO || !F) return fail(T4K_ERR_ARG, "t4k_patch_bwd: null tensor");
    if ((DF == nullptr) != (DB == nullptr)) return fail(T4K_ERR_ARG, "t4k_patch_bwd: DF and DB go together");
    PatchPlan g;
    const bool adjacent = DF && C1 >= 1 && C0 >= 1 && K >= 2 && K <= 32 && DB == DF + (long)C1 * K * K * C0;
    const int rc = patch_plan(g, "t4k_patch_bwd", N, H1, W1, C1, C0, K,
                              (aligned16(I) ? PAL_I : 0) | (aligned16(F) ? PAL_F : 0) | (aligned16(DO) ? PAL_DO : 0) | (adjacent ? 0 : PAL_DB_APART)); if (rc != T4K_OK) return rc;
    hipStream_t hs = t4k::S(s);
    if (train && DF) {                                           // stage 1 reads I, which DX2 may overwrite: slabs, then their fold in slice order
        if (st().ws_bytes / 2 < CONV_WS_BYTES) return fail(T4K_ERR_NOMEM, "t4k_patch_bwd: workspace");
        const int ndf = g.Kd * C0, ntot = ndf + C0;
        PatD d = { I, DO, ws_for(s), N, H1, W1, C1, C0, K, g.H0, g.W0, g.R, g.Kd, g.M, g.pps };
        patch_divs(d);
        conv_plan_note("patch_dfx%d<%s,%s>", g.nslice, g.df_va ? "i4" : "i1", g.df_vb ? "d4" : "d1");
        const dim3 grid(g.nslice, (g.Kd + 64) / 64, (C0 + 63) / 64);
        with_flags([&](auto a, auto b) { T4K_LAUNCH((k_patch_df<a.value, b.value>), grid, dim3(256), 0, hs, d); }, g.df_va != 0, g.df_vb != 0);
        if (g.fold == 1) { conv_plan_note("fold_add"); launch_fold_add(d.part, DF, ntot, g.nslice, hs); }
        else             { conv_plan_note("df_fold");  launch_df_fold(d.part, DF, DB, g.nslice, ndf, ntot, hs); }
    }
    if (DX) {
        PatP p = { DO, F, nullptr, DX, DX2, N, H1, W1, C1, C0, K, g.H0, g.W0, g.R, g.Kd, g.M };
        p.tiles_n = (g.Kd + g.dx_bn - 1) / g.dx_bn; p.nst = (C0 + PBK - 1) / PBK; p.tiles = (g.M + PBM - 1) / PBM * p.tiles_n;
        patch_divs(p);
        conv_plan_note("patch_dx<%d,%s>", g.dx_bn, g.dx_v ? "v4" : "v1");
        launch_patch<true>(p, g.dx_v, g.dx_v, g.dx_bn, g.zero_wg, hs);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
