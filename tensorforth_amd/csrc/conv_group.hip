// conv_group.hip - grouped and depthwise conv2d with RUN-TIME geometry (t4k_conv2d_grp_fwd / _bwd / _plan): conv_geo.hip's K 1..7,
// stride 1..4, dilation 1..4, padding 0..D(K-1), with the channels cut into G groups.  Output channel c0 belongs to group g = c0 / Cg0 (Cg0 = C0 / G) and
// reads the Cg1 = C1 / G input channels g Cg1 .. g Cg1 + Cg1 - 1 only; the filter is T4(Cg1, K, K, C0):
//   forward  O[pix, c0]  = B[c0] + sum_{cg, tap} I[pix*S + tap*D - P, g Cg1 + cg] * F[cg, tap, c0]
//   dX       dX[pix, c1] = sum_{c0 of c1's group, tap} dO[(pix + P - tap*D) / S, c0] * F[c1 - g Cg1, tap, c0]     over the taps that divide (textbook)
//   dF | dB  slab[slice][(cg, tap) | bias][c0] = sum_{pix of the slice} I[pix*S + tap*D - P, g Cg1 + cg] * dO[pix, c0], folded in slice order by colsum.h
// The reference has no groups (Model::_iconv model.cpp:121-180 allocates T4(C1, K, K, C0) and k_conv2d nmath.tcu:12 walks every input channel).
// A depthwise layer (Cg1 == 1) is K K multiply-adds per output element: bandwidth, not arithmetic - k_geo's 32-channel MFMA k-step per tap has nothing to
// contract over.  So these kernels run on the vector ALUs with the lanes along the NHWC channels: a thread owns 4 consecutive channels (16-byte loads and
// stores) or one (dwords), a workgroup walks 2-D TILES of pixels so that the window rows its threads share are found in L1, and a whole row of K taps is
// loaded before the first is used (K is a kernel argument; the row width is dispatched once per kernel, so no remainder loop waits behind each load).
// Every element of every produced tensor is stored exactly once; no atomics; fixed summation order; nothing outside the tensors is read.
#include "conv_types.h"
#include "fastdiv.h"

namespace {

constexpr int GRP_MAX_WG = 4096;                        // forward / dX: the grid walks the tiles with this stride at most

// the load paths (the template argument of every kernel): how a thread's output channels and the input channels under them are fetched
enum { GM_V1 = 0,      // one channel per thread, dwords everywhere
       GM_DW,          // 4 channels, depthwise with multiplier 1: the four inputs are ONE 16-byte load per tap
       GM_G4S,         // 4 channels of ONE group (Cg0 % 4 == 0): one dword of the input per (cg, tap), 16-byte filter loads
       GM_G4E };       // 4 channels of up to four groups (depthwise, multiplier not a multiple of 4): four dwords of the input per tap
template <int M> constexpr int vw_of = M == GM_V1 ? 1 : 4;

struct GrpP {
    const float *X, *F, *B;            // gathered tensor (forward: I, dX: dO), filter [Cg1][K][K][C0], bias (forward)
    float *Y, *Y2;                     // produced tensor (+ optional second copy)
    int N, H1, W1, C1, H0, W0, C0;     // the layer's input and output grids, whichever is produced
    int Cg1, Cg0, K, S, P, D;
    int CV, tl, tiles_x, tiles_y;      // channel groups of a produced pixel; log2 of the tile edge; tiles per image
    long ntile;
    FastDiv dCV, dTX, dTY, dCg, dS;    // by CV, by the tiles per row / column, by the channels per group of the PRODUCED tensor's counterpart (see the kernels), by S
};

template <int VW> __device__ __forceinline__ void ld_vec(float (&v)[VW], const float *q) {
    if constexpr (VW == 4) { const float4 t = *reinterpret_cast<const float4 *>(q); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *q;
}
template <int VW> __device__ __forceinline__ void st_vec(float *q, const float (&v)[VW]) {
    if constexpr (VW == 4) *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
    else *q = v[0];
}
// the inputs under a thread's output channels at one pixel (`px`: the pixel's first channel); ci[e] = the first input channel of output channel e's group
template <int M> __device__ __forceinline__ void ld_in(float (&x)[vw_of<M>], bool ok, const float *px, const int (&ci)[vw_of<M>], int cg) {
    constexpr int VW = vw_of<M>;
    if (!ok) {
#pragma unroll
        for (int e = 0; e < VW; e++) x[e] = 0.f;
        return;
    }
    if constexpr (M == GM_DW) ld_vec<4>(x, px + ci[0]);
    else if constexpr (M == GM_G4S) { const float t = px[ci[0] + cg]; x[0] = t; x[1] = t; x[2] = t; x[3] = t; }
    else {
#pragma unroll
        for (int e = 0; e < VW; e++) x[e] = px[ci[e] + cg];
    }
}
// K -> the compile-time width of a tap row: f(int_c<K>{}) once per kernel, wave-uniform
template <typename F> __device__ __forceinline__ void with_row(int K, F &&f) {
    switch (K) {
    case 1: f(int_c<1>{}); break; case 2: f(int_c<2>{}); break; case 3: f(int_c<3>{}); break; case 4: f(int_c<4>{}); break;
    case 5: f(int_c<5>{}); break; case 6: f(int_c<6>{}); break; default: f(int_c<7>{}); break;
    }
}
// a workgroup's walk over its tiles: f(n, i, j, cv) for every (pixel, channel group) of the H x W grid.  The channel group is the fastest digit of a tile's
// items, the tile column the next: neighbouring lanes store neighbouring addresses, and the 256 items of one pass are a few tile rows of neighbouring pixels
template <typename F> __device__ __forceinline__ void walk_tiles(const GrpP &p, int H, int W, F &&f) {
    const int te = 1 << p.tl, items = p.CV << (2 * p.tl);
    for (long t = blockIdx.x; t < p.ntile; t += gridDim.x) {
        const unsigned q = (unsigned)t, tq = fdiv(q, p.dTX), n = fdiv(tq, p.dTY);
        const int bx = (int)(q - tq * (unsigned)p.tiles_x) << p.tl, by = (int)(tq - n * (unsigned)p.tiles_y) << p.tl;
        for (int it = threadIdx.x; it < items; it += 256) {
            const unsigned px = fdiv((unsigned)it, p.dCV);
            const int cv = it - (int)px * p.CV, j = bx + (int)(px & (unsigned)(te - 1)), i = by + (int)(px >> p.tl);
            if (i < H && j < W) f((int)n, i, j, cv);
        }
    }
}

// ------------------------------------------------------------------ forward: a thread owns (output pixel, VW output channels); dCg divides by Cg0
template <int M>
__global__ void __launch_bounds__(256) k_grp_fwd(GrpP p) {
    constexpr int VW = vw_of<M>;
    with_row(p.K, [&](auto kw) {
        constexpr int KW = decltype(kw)::value;
        walk_tiles(p, p.H0, p.W0, [&](int n, int i, int j, int cv) {
            const int c0 = cv * VW;
            float acc[VW]; int ci[VW];
#pragma unroll
            for (int e = 0; e < VW; e++) { acc[e] = p.B[c0 + e]; ci[e] = M == GM_DW ? c0 + e : (int)fdiv((unsigned)(c0 + e), p.dCg) * p.Cg1; }
            const int iy0 = i * p.S - p.P, ix0 = j * p.S - p.P;
            const float *img = p.X + (long)n * p.H1 * p.W1 * p.C1;
#pragma unroll 1
            for (int cg = 0; cg < p.Cg1; cg++) {
#pragma unroll 1
                for (int ky = 0; ky < KW; ky++) {
                    const int gy = iy0 + ky * p.D;
                    if ((unsigned)gy >= (unsigned)p.H1) continue;
                    const float *row = img + (long)gy * p.W1 * p.C1, *f = p.F + (long)((cg * KW + ky) * KW) * p.C0 + c0;
                    float x[KW][VW], w[KW][VW];
#pragma unroll
                    for (int kx = 0; kx < KW; kx++) {                     // the whole row in flight
                        const int gx = ix0 + kx * p.D;
                        ld_in<M>(x[kx], (unsigned)gx < (unsigned)p.W1, row + (long)gx * p.C1, ci, cg);
                        ld_vec<VW>(w[kx], f + (long)kx * p.C0);
                    }
#pragma unroll
                    for (int kx = 0; kx < KW; kx++)
#pragma unroll
                        for (int e = 0; e < VW; e++) acc[e] += x[kx][e] * w[kx][e];
                }
            }
            st_vec<VW>(p.Y + (((long)n * p.H0 + i) * p.W0 + j) * p.C0 + c0, acc);
        });
    });
}

// ------------------------------------------------------------------ dX: a thread owns (input pixel, VW input channels); dCg divides by Cg1
// The contributing taps of row y are those ky with (y + P - ky D) % S == 0 and the quotient inside the output grid - k_geo<dX>'s residue classes, decided
// per thread here; columns likewise.  The Cg0 output channels of the group are summed in ascending order.  VW == 4 is the depthwise layer with
// multiplier 1 only (c0 == c1); a pixel no window covers stores 0.
template <int VW>
__global__ void __launch_bounds__(256) k_grp_dx(GrpP p) {
    with_row(p.K, [&](auto kw) {
        constexpr int KW = decltype(kw)::value;
        walk_tiles(p, p.H1, p.W1, [&](int n, int y, int x, int cv) {
            const int c1 = cv * VW;
            const int g = VW == 4 ? 0 : (int)fdiv((unsigned)c1, p.dCg), cg = VW == 4 ? 0 : c1 - g * p.Cg1;
            float acc[VW];
#pragma unroll
            for (int e = 0; e < VW; e++) acc[e] = 0.f;
            const float *img = p.X + (long)n * p.H0 * p.W0 * p.C0;
#pragma unroll 1
            for (int q = 0; q < p.Cg0; q++) {
                const int c0 = VW == 4 ? c1 : g * p.Cg0 + q;
#pragma unroll 1
                for (int ky = 0; ky < KW; ky++) {
                    const int ty = y + p.P - ky * p.D;
                    if (ty < 0) break;                                     // ty falls with ky
                    const int i = (int)fdiv((unsigned)ty, p.dS);
                    if (i * p.S != ty || i >= p.H0) continue;
                    const float *row = img + (long)i * p.W0 * p.C0 + c0, *f = p.F + (long)((cg * KW + ky) * KW) * p.C0 + c0;
                    float d[KW][VW], w[KW][VW];
#pragma unroll
                    for (int kx = 0; kx < KW; kx++) {
                        const int tx = x + p.P - kx * p.D, jj = (int)fdiv((unsigned)max(tx, 0), p.dS);
                        if (tx >= 0 && jj * p.S == tx && jj < p.W0) ld_vec<VW>(d[kx], row + (long)jj * p.C0);
                        else {
#pragma unroll
                            for (int e = 0; e < VW; e++) d[kx][e] = 0.f;
                        }
                        ld_vec<VW>(w[kx], f + (long)kx * p.C0);
                    }
#pragma unroll
                    for (int kx = 0; kx < KW; kx++)
#pragma unroll
                        for (int e = 0; e < VW; e++) acc[e] += d[kx][e] * w[kx][e];
                }
            }
            const long o = (((long)n * p.H1 + y) * p.W1 + x) * p.C1 + c1;
            st_vec<VW>(p.Y + o, acc);
            if (p.Y2) st_vec<VW>(p.Y2 + o, acc);
        });
    });
}

// ------------------------------------------------------------------ dF | dB partial slabs
// grid = (slices, Cg1, channel tiles).  The 256 threads of a workgroup are CL channel lanes (a power of two, at most 32) x R = 256 / CL rows; row r is
// (tap row ky = r % K, pixel sub-slice ps = r / K), so the K threads that need one pixel's dO and its window rows sit in ONE workgroup at the same time.
// A thread owns (VW output channels, input channel cg, tap row ky): K x VW sums over the pixels k_beg + ps, + NPS, ... of its slice, plus the bias sums
// where ky == 0 and cg == 0.  The sub-slices are added through LDS in ascending ps by the threads of ps == 0, which store the slab rows: a fixed order.
struct GrpD {
    const float *I, *DO; float *part;
    int N, H1, W1, C1, H0, W0, C0, Cg1, Cg0, K, S, P, D;
    int CV, cll, nps; long pps;        // channel groups of an output pixel; log2 CL; pixel sub-slices of a workgroup; pixels per slice
    FastDiv dW0, dH0, dK, dCg;         // dCg divides by Cg0
};

template <int M>
__global__ void __launch_bounds__(256) k_grp_df(GrpD p) {
    constexpr int VW = vw_of<M>;
    __shared__ __attribute__((aligned(16))) float sm[8 * VW * 256];        // [K tap columns + the bias][VW][thread]
    with_row(p.K, [&](auto kw) {
        constexpr int KW = decltype(kw)::value;
        const int tid = threadIdx.x, cl = tid & ((1 << p.cll) - 1), r = tid >> p.cll;
        const int ps = (int)fdiv((unsigned)r, p.dK), ky = r - ps * KW;
        const int cvi = (int)blockIdx.z * (1 << p.cll) + cl, c0 = cvi * VW, cg = blockIdx.y;
        const bool act = ps < p.nps && cvi < p.CV, bias = ky == 0 && cg == 0;
        const long npix = (long)p.N * p.H0 * p.W0;
        const long k_beg = (long)blockIdx.x * p.pps, k_end = min(npix, k_beg + p.pps);
        float acc[KW][VW], accb[VW];
#pragma unroll
        for (int e = 0; e < VW; e++) {
            accb[e] = 0.f;
#pragma unroll
            for (int kx = 0; kx < KW; kx++) acc[kx][e] = 0.f;
        }
        if (act) {
            int ci[VW];
#pragma unroll
            for (int e = 0; e < VW; e++) ci[e] = M == GM_DW ? c0 + e : (int)fdiv((unsigned)(c0 + e), p.dCg) * p.Cg1;
#pragma unroll 2
            for (long pix = k_beg + ps; pix < k_end; pix += p.nps) {
                const unsigned q = (unsigned)pix, t = fdiv(q, p.dW0), n = fdiv(t, p.dH0);
                const int j = (int)(q - t * (unsigned)p.W0), i = (int)(t - n * (unsigned)p.H0);
                float g[VW]; ld_vec<VW>(g, p.DO + pix * p.C0 + c0);
                const int gy = i * p.S + ky * p.D - p.P, ix0 = j * p.S - p.P;
                const bool rok = (unsigned)gy < (unsigned)p.H1;
                const float *row = p.I + ((long)n * p.H1 + gy) * p.W1 * p.C1;
                float x[KW][VW];
#pragma unroll
                for (int kx = 0; kx < KW; kx++) {
                    const int gx = ix0 + kx * p.D;
                    ld_in<M>(x[kx], rok && (unsigned)gx < (unsigned)p.W1, row + (long)gx * p.C1, ci, cg);
                }
#pragma unroll
                for (int e = 0; e < VW; e++) {
                    accb[e] += g[e];
#pragma unroll
                    for (int kx = 0; kx < KW; kx++) acc[kx][e] += x[kx][e] * g[e];
                }
            }
#pragma unroll
            for (int e = 0; e < VW; e++) {
#pragma unroll
                for (int kx = 0; kx < KW; kx++) sm[(kx * VW + e) * 256 + tid] = acc[kx][e];
                sm[(KW * VW + e) * 256 + tid] = accb[e];
            }
        }
        __syncthreads();
        if (act && ps == 0) {
            const long ntot = ((long)p.Cg1 * KW * KW + 1) * p.C0;
            float *slab = p.part + (long)blockIdx.x * ntot + c0;
            for (int a = 0; a < (bias ? KW + 1 : KW); a++) {          // the tap columns of this row, then the bias sums
                float s[VW];
#pragma unroll
                for (int e = 0; e < VW; e++) {
                    float v = 0.f;
                    for (int u = 0; u < p.nps; u++) v += sm[(a * VW + e) * 256 + (((u * KW + ky) << p.cll) + cl)];
                    s[e] = v;
                }
                st_vec<VW>(slab + (a == KW ? (long)p.Cg1 * KW * KW : (long)((cg * KW + ky) * KW + a)) * p.C0, s);
            }
        }
    });
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_conv2d_grp_plan reports
struct GrpPlan {
    int H0, W0, Cg1, Cg0;
    int mode;                          // GM_*: the forward's and the dF kernel's load path
    int dx_v;                          // dX: 4 channels per thread (depthwise, multiplier 1) or one
    int cll, nps, nslice, fold; long pps;   // dF: log2 channel lanes, pixel sub-slices per workgroup, slices, pixels per slice, the fold (1 fold_add, 2 df_fold)
};
// admission (who: the entry's name for the message) and the plan.  T4K_ERR_ARG: an extent below 1; T4K_ERR_UNSUPPORTED: a geometry or a group count outside
// the admitted set (conv_geo_admit, conv_types.h, shared with conv_geo.hip)
int grp_plan(GrpPlan &g, const char *who, int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D, int G, bool aligned, bool db_adjacent) {
    const int rc = conv_geo_admit(who, N, H1, W1, C1, C0, K, S, P, D, &G, &g.H0, &g.W0); if (rc != T4K_OK) return rc;
    g.Cg1 = C1 / G; g.Cg0 = C0 / G;
    const long np0 = (long)N * g.H0 * g.W0, ntot = ((long)g.Cg1 * K * K + 1) * C0;
    g.mode = (!aligned || C0 % 4 != 0) ? GM_V1 : (g.Cg1 == 1 && g.Cg0 == 1) ? GM_DW : g.Cg0 % 4 == 0 ? GM_G4S : g.Cg1 == 1 ? GM_G4E : GM_V1;
    g.dx_v = g.mode == GM_DW;
    // dF: CL = the power of two that holds the channel groups, at most 32 (R = 256 / CL >= 8 > K - 1 rows: every tap row has a thread)
    const int cv = g.mode == GM_V1 ? C0 : C0 / 4;
    g.cll = 0; while (g.cll < 5 && (1 << g.cll) < cv) g.cll++;
    g.nps = (256 >> g.cll) / K;
    const long ctiles = ((long)cv + (1 << g.cll) - 1) >> g.cll;
    if (g.Cg1 > 65535 || ctiles > 65535) return fail(T4K_ERR_UNSUPPORTED, "%s: more tiles than a launch takes", who);
    const SlabPlan sp = slab_plan(np0, (long)g.Cg1 * ctiles, ntot, db_adjacent, 1L << 62);   // (GrpD::pps is a long: no cap)
    g.pps = sp.pps; g.nslice = sp.nslice; g.fold = sp.fold;
    return T4K_OK;
}

// the tile walk of forward (the output grid) and dX (the input grid): 8 x 8 pixels, 16 x 16 where a pixel has fewer than four channel groups
GrpP grp_parms(const GrpPlan &g, bool bwd, int vw, const float *X, const float *F, const float *B, float *Y, float *Y2,
               int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D) {
    GrpP p;
    p.X = X; p.F = F; p.B = B; p.Y = Y; p.Y2 = Y2;
    p.N = N; p.H1 = H1; p.W1 = W1; p.C1 = C1; p.H0 = g.H0; p.W0 = g.W0; p.C0 = C0;
    p.Cg1 = g.Cg1; p.Cg0 = g.Cg0; p.K = K; p.S = S; p.P = P; p.D = D;
    const int H = bwd ? H1 : g.H0, W = bwd ? W1 : g.W0;
    p.CV = (bwd ? C1 : C0) / vw;
    p.tl = p.CV >= 4 ? 3 : 4;
    const int te = 1 << p.tl;
    p.tiles_x = (W + te - 1) / te; p.tiles_y = (H + te - 1) / te;
    p.ntile = (long)N * p.tiles_y * p.tiles_x;
    p.dCV = fast_div(p.CV); p.dTX = fast_div(p.tiles_x); p.dTY = fast_div(p.tiles_y); p.dCg = fast_div(bwd ? g.Cg1 : g.Cg0); p.dS = fast_div(S);
    return p;
}
template <typename F> void with_mode(int mode, F &&f) { pick<GM_V1, GM_DW, GM_G4S, GM_G4E>(mode, f); }

} // namespace

extern "C" {

int t4k_conv2d_grp_plan(int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D, int G, int aligned, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_conv2d_grp_plan: null");
    GrpPlan g;
    const int rc = grp_plan(g, "t4k_conv2d_grp_plan", N, H1, W1, C1, C0, K, S, P, D, G, (aligned & 1) != 0, !(aligned & 2)); if (rc != T4K_OK) return rc;
    out[0] = g.Cg1 == 1 ? 1 : 2; out[1] = g.mode; out[2] = g.dx_v ? 4 : 1; out[3] = 1 << g.cll;
    out[4] = g.nps; out[5] = g.nslice; out[6] = g.fold; out[7] = 3;
    return T4K_OK;
}

int t4k_conv2d_grp_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, int D, int G, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    ConvPlanScope plan;
    if (!I || !O || !F || !B) return fail(T4K_ERR_ARG, "t4k_conv2d_grp_fwd: null tensor");
    GrpPlan g;
    const int rc = grp_plan(g, "t4k_conv2d_grp_fwd", N, H1, W1, C1, C0, K, S, P, D, G, all16(I, F, O), true); if (rc != T4K_OK) return rc;
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_conv2d_grp_fwd: output %dx%d, the geometry gives %dx%d", H0, W0, g.H0, g.W0);
    hipStream_t hs = t4k::S(s);
    if (ICOPY) { conv_plan_note("memcpy"); T4K_HIP(hipMemcpyAsync(ICOPY, I, sizeof(float) * (size_t)N * H1 * W1 * C1, hipMemcpyDeviceToDevice, hs)); }
    const GrpP p = grp_parms(g, false, g.mode == GM_V1 ? 1 : 4, I, F, B, O, nullptr, N, H1, W1, C1, C0, K, S, P, D);
    conv_plan_note("%s<%s>", g.Cg1 == 1 ? "grp_dw" : "grp", g.mode == GM_V1 ? "v1" : "v4");
    const dim3 grid((unsigned)std::min(p.ntile, (long)GRP_MAX_WG));
    with_mode(g.mode, [&](auto m) { T4K_LAUNCH((k_grp_fwd<decltype(m)::value>), grid, dim3(256), 0, hs, p); });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_conv2d_grp_bwd(const float *I, const float *DO, float *DX, float *DX2, const float *F, float *DF, float *DB,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, int D, int G, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    ConvPlanScope plan;
    if (!I || !DO || !F) return fail(T4K_ERR_ARG, "t4k_conv2d_grp_bwd: null tensor");
    if ((DF == nullptr) != (DB == nullptr)) return fail(T4K_ERR_ARG, "t4k_conv2d_grp_bwd: DF and DB go together");
    GrpPlan g;
    // one flag for every 16-byte path of the backward, as the plan entry takes it: dO, F and I are read, DX and DX2 stored, 16 bytes at a time
    const int rc = grp_plan(g, "t4k_conv2d_grp_bwd", N, H1, W1, C1, C0, K, S, P, D, G, all16(DO, F, I, DX, DX2), true); if (rc != T4K_OK) return rc;
    const long ndf = (long)g.Cg1 * K * K * C0;                   // (an admitted geometry: the product fits)
    if (!(DF && DB == DF + ndf)) g.fold = 2;                     // DB elsewhere: the fold that splits the slab
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_conv2d_grp_bwd: output %dx%d, the geometry gives %dx%d", H0, W0, g.H0, g.W0);
    hipStream_t hs = t4k::S(s);
    if (train && DF) {                                           // stage 1 reads I, which DX2 may overwrite: slabs, then their fold in slice order
        if (st().ws_bytes / 2 < CONV_WS_BYTES) return fail(T4K_ERR_NOMEM, "t4k_conv2d_grp_bwd: workspace");
        float *part = ws_for(s);
        const int ntot = (int)ndf + C0;
        GrpD d = { I, DO, part, N, H1, W1, C1, H0, W0, C0, g.Cg1, g.Cg0, K, S, P, D, g.mode == GM_V1 ? C0 : C0 / 4, g.cll, g.nps, g.pps,
                   fast_div(W0), fast_div(H0), fast_div(K), fast_div(g.Cg0) };
        conv_plan_note("grp_dfx%d", g.nslice);
        const dim3 grid(g.nslice, g.Cg1, (unsigned)((d.CV + (1 << g.cll) - 1) >> g.cll));
        with_mode(g.mode, [&](auto m) { T4K_LAUNCH((k_grp_df<decltype(m)::value>), grid, dim3(256), 0, hs, d); });
        if (g.fold == 1) { conv_plan_note("fold_add"); launch_fold_add(part, DF, ntot, g.nslice, hs); }
        else             { conv_plan_note("df_fold");  launch_df_fold(part, DF, DB, g.nslice, (int)ndf, ntot, hs); }
    }
    if (DX) {
        const GrpP p = grp_parms(g, true, g.dx_v ? 4 : 1, DO, F, nullptr, DX, DX2, N, H1, W1, C1, C0, K, S, P, D);
        conv_plan_note("grp_dx<%s>", g.dx_v ? "v4" : "v1");
        const dim3 grid((unsigned)std::min(p.ntile, (long)GRP_MAX_WG));
        pick<4, 1>(g.dx_v ? 4 : 1, [&](auto vw) { T4K_LAUNCH((k_grp_dx<decltype(vw)::value>), grid, dim3(256), 0, hs, p); });
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
