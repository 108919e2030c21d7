// addnorm.hip - "add & norm" for NHWC fp32 tokens, forward and backward: out = norm(x + skip), either half optional.  rows = N H W tokens of
// C contiguous floats; mode 0 no norm, 1 torch's layer_norm(z, (C,), W, B, eps), 2 RMS norm z rsqrt(mean(z z) + eps) W + B.  The reference has neither a
// residual connection nor a per-token norm (its README lists "add block - residual map" as to do).
// A TEAM owns a token at a time: T = 8 .. 64 lanes of a wave on rung 1 (a 256-thread workgroup holds 256 / T tokens), the whole workgroup on rung 2.  Lane l
// of the team owns the column items l, l + T, l + 2T .. (at most 8 of them, each VW floats), so neighbouring lanes load neighbouring addresses, z = x + s lives
// in registers between the sums, and a thread's gamma, beta and its dW | dB partial sums never change column.  A workgroup walks a contiguous slab of
// tokens and leaves ONE row of 2 C partial sums; colsum.h's launchers fold the rows.  The variance is the sum of squared deviations from the token's own
// computed mean, a second pass over the registers.  No atomics anywhere: every sum is a fixed tree.
#include "t4k_common.h"
#include "launch.h"
#include "colsum.h"

using namespace t4k;

namespace {

constexpr int AN_ITEMS  = 8;            // column items of the load width a lane keeps in registers at most (the backward holds g = gamma t, xhat and two partial sums of each)
constexpr int AN_BLK    = 256;          // the workgroup: four waves, one per SIMD
constexpr int AN_WG     = 2048;         // workgroups the forward spreads the tokens over at most: 256 CUs x 8 resident workgroups
constexpr int AN_SLICES = 1024;         // ... and the backward, one dW | dB slab row each: the device's width, whatever rows is

struct AnP {
    long rows, per;                    // tokens, tokens of a workgroup's slab (a multiple of tpw)
    int  C, items, T, tsh, tpw;        // channels, column items C / VW, lanes per token and its log2, tokens a workgroup holds at a time
    float eps, fC;                     // fC = (float)C
};

template <int VW> __device__ __forceinline__ void an_ld(const float *q, float (&v)[VW]) {
    if constexpr (VW == 4) { const float4 t = *reinterpret_cast<const float4 *>(q); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *q;
}
template <int VW> __device__ __forceinline__ void an_st(float *q, const float (&v)[VW]) {
    if constexpr (VW == 4) *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
    else *q = v[0];
}
// the sums of NV values over the team, in every lane of it.  Rung 1: xor butterflies over the team's T lanes of the wave (the partner of a lane is in its
// own team: off < T), every lane of the wave arriving.  Rung 2: wave butterflies, then the four wave sums through LDS, added in one order
template <int RUNG, int NV> __device__ __forceinline__ void an_sum(float (&a)[NV], int T, float *sm) {
    if constexpr (RUNG == 1) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            if (off < T) {                                                  // (uniform: T is a kernel argument)
#pragma unroll
                for (int v = 0; v < NV; v++) a[v] += __shfl_xor(a[v], off, 64);
            }
        }
    } else {
        const int w = threadIdx.x >> 6;
#pragma unroll
        for (int v = 0; v < NV; v++) { a[v] = wave_sum_all(a[v]); if ((threadIdx.x & 63) == 0) sm[v * 4 + w] = a[v]; }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < NV; v++) a[v] = (sm[v * 4] + sm[v * 4 + 1]) + (sm[v * 4 + 2] + sm[v * 4 + 3]);
        __syncthreads();
    }
}
// a walking pointer stays a per-lane value: without this the compiler splits every item's address into a uniform base (a scalar pair per item and tensor,
// hoisted out of the token loop - they spilled scalar registers on the dword path) and one lane offset
template <typename P> __device__ __forceinline__ void an_keep(P *&q) { asm volatile("" : "+v"(q)); }
// t = dy + dy2 and g = W t, each rounded wherever it is used: contracted into g - m1 they would be other numbers than the ones that were summed
__device__ __forceinline__ float an_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// ------------------------------------------------------------------ rung 0: mode 0, flat.  O = X + S (S NULL: O = X); the backward is the same kernel on DY, DY2
template <int VW>
__global__ void __launch_bounds__(AN_BLK) k_an_flat(const float *X, const float *S, float *O, long nitems) {
    for (long i = (long)blockIdx.x * AN_BLK + threadIdx.x; i < nitems; i += (long)gridDim.x * AN_BLK) {
        float x[VW], s[VW];
        an_ld<VW>(X + i * VW, x);
        if (S) {
            an_ld<VW>(S + i * VW, s);
#pragma unroll
            for (int v = 0; v < VW; v++) x[v] += s[v];
        }
        an_st<VW>(O + i * VW, x);
    }
}

// ------------------------------------------------------------------ rungs 1 and 2: the token lives in the team's registers
// Every tensor is walked by one pointer per lane, item to item (kT floats on; an_keep).  gamma and beta are re-read per token - C floats that stay in the CU's cache - and do
// not hold registers across the slab: the forward keeps z alone (three waves a SIMD and more), the backward t, xhat and its dW | dB partial sums.
// X, S and O carry no __restrict__: O may be X or S - a thread stores only what it loaded, after all its loads of the token (the sums depend on them)
template <int RUNG, int VW, int MODE>
__global__ void __launch_bounds__(AN_BLK) k_an_fwd(const float *X, const float *S, float *O, float *__restrict__ XH, float *__restrict__ RSTD,
                                                   const float *__restrict__ W, const float *__restrict__ B, AnP p) {
    __shared__ float sm[8];
    const int T = RUNG == 1 ? p.T : AN_BLK, kT = T * VW;
    const int tm = RUNG == 1 ? (int)(threadIdx.x >> p.tsh) : 0, l = (int)threadIdx.x & (T - 1);
    const int mine = l < p.items ? (p.items - l + T - 1) / T : 0;           // column items of this lane: l, l + T .. (at most AN_ITEMS)
    const long r0 = (long)blockIdx.x * p.per, r1 = min(p.rows, r0 + p.per);
    for (long t0 = r0; t0 < r1; t0 += p.tpw) {                              // (uniform over the workgroup: every lane arrives at the sums)
        const long tok = t0 + tm;
        const int n = tok < r1 ? mine : 0;                                  // items this lane loads and stores for this token
        const long base = tok * p.C + (long)l * VW;
        float z[AN_ITEMS][VW], a[1] = { 0.f };
        const float *px = X + base, *ps = S + base;
#pragma unroll
        for (int k = 0; k < AN_ITEMS; k++, px += kT, ps += kT) {
            an_keep(px); an_keep(ps);
#pragma unroll
            for (int v = 0; v < VW; v++) z[k][v] = 0.f;
            if (k < n) {
                an_ld<VW>(px, z[k]);
                if (S) {
                    float s[VW]; an_ld<VW>(ps, s);
#pragma unroll
                    for (int v = 0; v < VW; v++) z[k][v] += s[v];
                }
            }
#pragma unroll
            for (int v = 0; v < VW; v++) a[0] += MODE == 1 ? z[k][v] : z[k][v] * z[k][v];
        }
        an_sum<RUNG, 1>(a, T, sm);
        float mean = 0.f;
        if constexpr (MODE == 1) {
            mean = a[0] / p.fC;
            a[0] = 0.f;
#pragma unroll
            for (int k = 0; k < AN_ITEMS; k++) {
                if (k < n) {
#pragma unroll
                    for (int v = 0; v < VW; v++) { const float d = z[k][v] - mean; a[0] += d * d; }
                }
            }
            an_sum<RUNG, 1>(a, T, sm);
        }
        const float rstd = 1.0f / sqrtf(a[0] / p.fC + p.eps);
        if (n > 0 && l == 0) RSTD[tok] = rstd;
        float *po = O + base, *ph = XH + base;
        const float *pw = W + l * VW, *pb = B + l * VW;
#pragma unroll
        for (int k = 0; k < AN_ITEMS; k++, po += kT, ph += kT, pw += kT, pb += kT) {
            an_keep(po); an_keep(ph); an_keep(pw); an_keep(pb);
            if (k < n) {
                float gw[VW], gb[VW], xh[VW], y[VW];
                an_ld<VW>(pw, gw); an_ld<VW>(pb, gb);
#pragma unroll
                for (int v = 0; v < VW; v++) { xh[v] = (z[k][v] - mean) * rstd; y[v] = xh[v] * gw[v] + gb[v]; }
                an_st<VW>(ph, xh); an_st<VW>(po, y);
            }
        }
    }
}

// DY, DY2 and DX carry no __restrict__: DX may be DY or DY2.  slab: the workgroup's row of 2 C partial sums (NULL: no dW | dB, uniform over the launch)
template <int RUNG, int VW, int MODE>
__global__ void __launch_bounds__(AN_BLK) k_an_bwd(const float *__restrict__ W, const float *DY, const float *DY2, const float *__restrict__ XH,
                                                   const float *__restrict__ RSTD, float *DX, float *__restrict__ slab, AnP p) {
    __shared__ float sm[8];
    __shared__ float red[RUNG == 1 ? 2 * VW * AN_BLK : 1];
    const int T = RUNG == 1 ? p.T : AN_BLK, kT = T * VW;
    const int tm = RUNG == 1 ? (int)(threadIdx.x >> p.tsh) : 0, l = (int)threadIdx.x & (T - 1);
    const int mine = l < p.items ? (p.items - l + T - 1) / T : 0;
    float aw[AN_ITEMS][VW], ab[AN_ITEMS][VW];
#pragma unroll
    for (int k = 0; k < AN_ITEMS; k++) {
#pragma unroll
        for (int v = 0; v < VW; v++) { aw[k][v] = 0.f; ab[k][v] = 0.f; }
    }
    const long r0 = (long)blockIdx.x * p.per, r1 = min(p.rows, r0 + p.per);
    for (long t0 = r0; t0 < r1; t0 += p.tpw) {
        const long tok = t0 + tm;
        const int n = tok < r1 ? mine : 0;
        const long base = tok * p.C + (long)l * VW;
        float g[AN_ITEMS][VW], xh[AN_ITEMS][VW], a[2] = { 0.f, 0.f };       // g = W t
        const float *pd = DY + base, *p2 = DY2 + base, *ph = XH + base, *pw = W + l * VW;
#pragma unroll
        for (int k = 0; k < AN_ITEMS; k++, pd += kT, p2 += kT, ph += kT, pw += kT) {
            an_keep(pd); an_keep(p2); an_keep(ph); an_keep(pw);
#pragma unroll
            for (int v = 0; v < VW; v++) { g[k][v] = 0.f; xh[k][v] = 0.f; }
            if (k < n) {
                float t[VW], gw[VW];
                an_ld<VW>(pd, t); an_ld<VW>(ph, xh[k]); an_ld<VW>(pw, gw);
                if (DY2) {
                    float d2[VW]; an_ld<VW>(p2, d2);
#pragma unroll
                    for (int v = 0; v < VW; v++) t[v] += d2[v];
                }
#pragma unroll
                for (int v = 0; v < VW; v++) {
                    g[k][v] = an_mul(gw[v], t[v]);
                    aw[k][v] += t[v] * xh[k][v]; ab[k][v] += t[v];
                }
            }
#pragma unroll
            for (int v = 0; v < VW; v++) {
                if (MODE == 1) a[0] += g[k][v];
                a[1] += g[k][v] * xh[k][v];
            }
        }
        an_sum<RUNG, 2>(a, T, sm);
        const float m1 = a[0] / p.fC, m2 = a[1] / p.fC, rstd = n > 0 ? RSTD[tok] : 0.f;
        float *po = DX + base;
#pragma unroll
        for (int k = 0; k < AN_ITEMS; k++, po += kT) {
            an_keep(po);
            if (k < n) {
                float dx[VW];
#pragma unroll
                for (int v = 0; v < VW; v++) dx[v] = rstd * (g[k][v] - m1 - xh[k][v] * m2);
                an_st<VW>(po, dx);
            }
        }
    }
    if (!slab) return;
    float *row = slab + (long)blockIdx.x * 2 * p.C;
    if constexpr (RUNG == 2) {                                              // a column has one thread
#pragma unroll
        for (int k = 0; k < AN_ITEMS; k++) {
            if (k < mine) {
                const int c = (l + k * T) * VW;
#pragma unroll
                for (int v = 0; v < VW; v++) { row[c + v] = aw[k][v]; row[p.C + c + v] = ab[k][v]; }
            }
        }
    } else {
        // the tpw threads that share a column (lane l of every team) are joined by a fixed tree: the teams of a wave by xor butterflies over the lane bits above
        // the team's (off = T .. 32: the partner holds the same column), then the four waves' sums through LDS, added in one order, one column item at a
        // time.  Every thread of the workgroup arrives at every barrier
        const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < AN_ITEMS; k++) {
            if (k * T >= p.items) break;                                    // (uniform: no lane has this item or a later one)
            float v2[2 * VW];
#pragma unroll
            for (int v = 0; v < VW; v++) { v2[v] = aw[k][v]; v2[VW + v] = ab[k][v]; }
#pragma unroll
            for (int off = 8; off <= 32; off <<= 1) {
                if (off >= T) {                                             // (uniform)
#pragma unroll
                    for (int v = 0; v < 2 * VW; v++) v2[v] += __shfl_xor(v2[v], off, 64);
                }
            }
#pragma unroll
            for (int v = 0; v < 2 * VW; v++) red[(v * 4 + w) * WAVE + lane] = v2[v];
            __syncthreads();
            if (tm == 0 && k < mine) {                                      // (team 0: lanes 0 .. T - 1 of wave 0)
                const int c = (l + k * T) * VW;
#pragma unroll
                for (int v = 0; v < 2 * VW; v++) {
                    const float *r4 = red + v * 4 * WAVE + lane;
                    const float sum = (r4[0] + r4[WAVE]) + (r4[2 * WAVE] + r4[3 * WAVE]);
                    if (v < VW) row[c + v] = sum; else row[p.C + c + v - VW] = sum;
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_addnorm_plan reports
struct AnPlan { int rung, vw, tpw, T, tsh, nslice, fold; long fper, bper; int fgrid; };
long an_cdiv(long a, long b) { return (a + b - 1) / b; }
// admission (who: the entry's name for the message) in 64 bits: the extents may be anything their types hold
int an_plan(AnPlan &g, const char *who, long rows, int C, int mode, bool aligned, long ws_bytes) {
    if (rows < 1 || C < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (rows=%ld C=%d)", who, rows, C);
    if (mode < 0 || mode > 2) return fail(T4K_ERR_ARG, "%s: mode=%d (0 none, 1 layer norm, 2 RMS norm)", who, mode);
    if (ws_bytes < 0) return fail(T4K_ERR_ARG, "%s: ws_bytes below 0", who);
    const long lim = 1L << 31;
    if (rows >= lim || rows * C >= lim) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 tokens or elements, or more", who);
    g.vw = (aligned && C % 4 == 0) ? 4 : 1;
    const int items = C / g.vw;
    g.tpw = 0; g.T = 0; g.tsh = 0; g.nslice = 0; g.fold = 0; g.fper = g.bper = 0; g.fgrid = 0;
    if (mode == 0) { g.rung = 0; return T4K_OK; }
    g.rung = 0;
    for (int T = 8, sh = 3; T <= WAVE; T <<= 1, sh++)
        if (an_cdiv(items, T) <= AN_ITEMS) { g.rung = 1; g.T = T; g.tsh = sh; g.tpw = AN_BLK / T; break; }
    if (!g.rung) {
        if (an_cdiv(items, AN_BLK) > AN_ITEMS)
            return fail(T4K_ERR_UNSUPPORTED, "%s: channels=%d not supported (at most %d with every pointer on 16 bytes and C %% 4 == 0, else %d)", who, C,
                        AN_BLK * AN_ITEMS * 4, AN_BLK * AN_ITEMS);
        g.rung = 2; g.T = AN_BLK; g.tsh = 8; g.tpw = 1;
    }
    const long groups = an_cdiv(rows, g.tpw);                              // workgroup visits the tokens need
    g.fper = an_cdiv(groups, std::min(groups, (long)AN_WG)) * g.tpw; g.fgrid = (int)an_cdiv(rows, g.fper);
    // the dW | dB slab: one row of 2 C floats per workgroup of the backward, as many as the device is wide and the workspace holds - never as many as rows
    const long fit = ws_bytes / (long)sizeof(float) / (2L * C);
    if (fit < 1) return fail(T4K_ERR_UNSUPPORTED, "%s: a dW | dB slab row (%ld floats) does not fit the workspace", who, 2L * C);
    g.bper = an_cdiv(groups, std::min(groups, std::min((long)AN_SLICES, fit))) * g.tpw; g.nslice = (int)an_cdiv(rows, g.bper);
    g.fold = g.nslice <= 32 ? 1 : 2;                                       // as groupnorm.hip: few slices walk whole slabs, else a wave per output
    return T4K_OK;
}
AnP an_parms(const AnPlan &g, long rows, int C, long per, float eps) {
    AnP p;
    p.rows = rows; p.per = per; p.C = C; p.items = C / g.vw; p.T = g.T; p.tsh = g.tsh; p.tpw = g.tpw; p.eps = eps; p.fC = (float)C;
    return p;
}
bool an16(const void *a, const void *b, const void *c, const void *d, const void *e = nullptr, const void *f = nullptr, const void *h = nullptr) {
    return aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) && aligned16(e) && aligned16(f) && aligned16(h);
}
// do [a, a + na) and [b, b + nb) floats share a byte?  (NULL: no.)  same_ok: the two being ONE tensor is no overlap
bool an_clash(const float *a, long na, const float *b, long nb, bool same_ok = false) {
    if (!a || !b) return false;
    if (same_ok && a == b) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float), b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
    return a0 < b1 && b0 < a1;
}
int an_flat(const float *X, const float *S, float *O, long n, bool aligned, hipStream_t hs) {
    const int vw = (aligned && n % 4 == 0) ? 4 : 1;
    const long nitems = n / vw;
    const unsigned grid = (unsigned)std::min(an_cdiv(nitems, AN_BLK), (long)AN_WG);
    if (vw == 4) T4K_LAUNCH((k_an_flat<4>), dim3(grid), dim3(AN_BLK), 0, hs, X, S, O, nitems);
    else         T4K_LAUNCH((k_an_flat<1>), dim3(grid), dim3(AN_BLK), 0, hs, X, S, O, nitems);
    return T4K_OK;
}

} // namespace

extern "C" {

int t4k_addnorm_plan(long rows, int C, int mode, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_addnorm_plan: null");
    AnPlan g;
    const int rc = an_plan(g, "t4k_addnorm_plan", rows, C, mode, aligned != 0, ws_bytes); if (rc != T4K_OK) return rc;
    out[0] = g.rung; out[1] = g.vw; out[2] = g.tpw; out[3] = g.T; out[4] = 1; out[5] = g.nslice; out[6] = g.fold; out[7] = g.rung == 0 ? 1 : 2;
    return T4K_OK;
}

int t4k_addnorm_fwd(const float *X, const float *S, float *O, float *XH, float *RSTD, const float *W, const float *B,
                    long rows, int C, int mode, float eps, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !O) return fail(T4K_ERR_ARG, "t4k_addnorm_fwd: null tensor");
    if (mode != 0 && (!XH || !RSTD || !W || !B)) return fail(T4K_ERR_ARG, "t4k_addnorm_fwd: XH, RSTD, W and B are required when mode != 0");
    if (!(eps > 0.0f)) return fail(T4K_ERR_ARG, "t4k_addnorm_fwd: eps must be above 0");
    if (mode == 0) XH = nullptr, RSTD = nullptr, W = nullptr, B = nullptr;
    AnPlan g;
    const int rc = an_plan(g, "t4k_addnorm_fwd", rows, C, mode, an16(X, S, O, XH, W, B), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long n = rows * C;
    // O may be X or S, the tensor itself; nothing else that is written may share a byte with another operand
    if (an_clash(O, n, X, n, true) || an_clash(O, n, S, n, true) || an_clash(O, n, XH, n) || an_clash(O, n, RSTD, rows) || an_clash(O, n, W, C) || an_clash(O, n, B, C) ||
        an_clash(XH, n, X, n) || an_clash(XH, n, S, n) || an_clash(XH, n, RSTD, rows) || an_clash(XH, n, W, C) || an_clash(XH, n, B, C) ||
        an_clash(RSTD, rows, X, n) || an_clash(RSTD, rows, S, n) || an_clash(RSTD, rows, W, C) || an_clash(RSTD, rows, B, C))
        return fail(T4K_ERR_ARG, "t4k_addnorm_fwd: an output overlaps another operand (O may be X or S, nothing else)");
    hipStream_t hs = t4k::S(s);
    if (g.rung == 0) { an_flat(X, S, O, n, g.vw == 4, hs); T4K_LAUNCH_CHECK(); return T4K_OK; }
    const AnP p = an_parms(g, rows, C, g.fper, eps);
    pick<1, 2>(g.rung, [&](auto rung) {
        pick<4, 1>(g.vw, [&](auto vw) {
            pick<1, 2>(mode, [&](auto md) {
                T4K_LAUNCH((k_an_fwd<decltype(rung)::value, decltype(vw)::value, decltype(md)::value>), dim3((unsigned)g.fgrid), dim3(AN_BLK), 0, hs, X, S, O, XH, RSTD, W, B, p);
            });
        });
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_addnorm_bwd(const float *W, const float *DY, const float *DY2, const float *XH, const float *RSTD, float *DX,
                    float *DW, float *DB, long rows, int C, int mode, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!DY || !DX) return fail(T4K_ERR_ARG, "t4k_addnorm_bwd: null tensor");
    if (mode != 0 && (!W || !XH || !RSTD)) return fail(T4K_ERR_ARG, "t4k_addnorm_bwd: W, XH and RSTD are required when mode != 0");
    if (mode == 0) W = nullptr, XH = nullptr, RSTD = nullptr, train = 0;       // no parameters: DW and DB stay untouched
    if (train && (!DW || !DB)) return fail(T4K_ERR_ARG, "t4k_addnorm_bwd: DW and DB are required when train != 0");
    if (!train) DW = nullptr, DB = nullptr;
    AnPlan g;
    const int rc = an_plan(g, "t4k_addnorm_bwd", rows, C, mode, an16(W, DY, DY2, XH, DX), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long n = rows * C;
    if (an_clash(DX, n, DY, n, true) || an_clash(DX, n, DY2, n, true) || an_clash(DX, n, XH, n) || an_clash(DX, n, RSTD, rows) || an_clash(DX, n, W, C) ||
        an_clash(DX, n, DW, C) || an_clash(DX, n, DB, C) || an_clash(DW, C, DB, C))
        return fail(T4K_ERR_ARG, "t4k_addnorm_bwd: an output overlaps another operand (DX may be DY or DY2, nothing else)");
    for (const float *g2 : { DW, DB })
        if (an_clash(g2, C, DY, n) || an_clash(g2, C, DY2, n) || an_clash(g2, C, XH, n) || an_clash(g2, C, RSTD, rows) || an_clash(g2, C, W, C))
            return fail(T4K_ERR_ARG, "t4k_addnorm_bwd: DW or DB overlaps another operand");
    hipStream_t hs = t4k::S(s);
    if (g.rung == 0) { an_flat(DY, DY2, DX, n, g.vw == 4, hs); T4K_LAUNCH_CHECK(); return T4K_OK; }
    const AnP p = an_parms(g, rows, C, g.bper, 0.0f);
    float *slab = train ? ws_for(s) : nullptr;
    pick<1, 2>(g.rung, [&](auto rung) {
        pick<4, 1>(g.vw, [&](auto vw) {
            pick<1, 2>(mode, [&](auto md) {
                T4K_LAUNCH((k_an_bwd<decltype(rung)::value, decltype(vw)::value, decltype(md)::value>), dim3((unsigned)g.nslice), dim3(AN_BLK), 0, hs, W, DY, DY2, XH, RSTD, DX, slab, p);
            });
        });
    });
    if (train) {
        if (g.fold == 1 && DB == DW + C) launch_fold_add(slab, DW, 2 * C, g.nslice, hs);
        else launch_df_fold(slab, DW, DB, g.nslice, C, 2 * C, hs);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
