// groupnorm.hip - group, layer and instance norm for NHWC fp32 tensors, forward and backward: torch.nn.functional.group_norm(x, G, W, B, eps).
// The reference has one normalisation layer, batchnorm (k_batchnorm_1/2 nmath.cu:177-242): C long columns.  This layer has N G independent groups, each HW rows
// of Cg = C / G contiguous floats at pitch C, from one element to a whole sample.  A TEAM of T threads (a wave on rung 1, a 1024-thread workgroup on rungs 2-4)
// owns a group (rung 4: a part of its rows).  Thread t of the team owns ONE column: with CgV = Cg / VW column items, RT = T / CgV rows are swept at a time
// by the first Tact = RT CgV threads, thread t at column t % CgV from row t / CgV on, so neighbouring threads load neighbouring addresses and a thread's
// gamma, beta and its dW | dB partial sums never change column (a group wider than the team, CgV > T, walks its columns in chunks of T, every row each).
// The variance is the sum of squared deviations from the group's own computed mean: a second pass over registers (rungs 1, 2) or over L2 (rung 3), Chan's
// merge of per-part (count, mean, M2) in part order on rung 4.  No atomics anywhere: every sum is a fixed tree.
#include "t4k_common.h"
#include "launch.h"
#include "fastdiv.h"
#include "colsum.h"

using namespace t4k;

namespace {

constexpr int GN_R1     = 8;            // rows of 16 bytes a thread keeps in registers on rung 1 (256-thread workgroups: the backward's 2 x 8 x 16 bytes leave 3 waves per SIMD)
constexpr int GN_R2     = 4;            // ... and on rung 2 (1024-thread workgroups: 128 VGPRs at most), twice as many on dwords (sixteen dword rows on rung 1 spill SGPRs: one lane mask per row)
constexpr int GN_T      = 1024;         // the team of rungs 2-4: one workgroup of 16 waves
constexpr int GN_FILL   = 256;          // groups that fill the device (one workgroup per CU): fewer, and a large group is cut into parts
constexpr int GN_WANT   = 1024;         // workgroups the split rung aims at
constexpr int GN_PMAX   = 64;           // parts per group at most
constexpr int GN_PITEMS = 1024;         // items a part holds at least: one per thread
constexpr int GN_MAX_WG = 1 << 20;      // grid cap: above it the teams stride over the groups

struct GnP {
    int N, HW, C, G, Cg, CgV, NG;
    int RT, Tact, ncc, h0;             // rows per sweep, active threads, column chunks (1 unless CgV > T), the first step of the column tree: pow2ceil(RT) / 2
    int P, rp;                         // parts per group, rows per part
    float eps, fE;                     // fE = (float)E
    FastDiv dCgV, dG, dP;
};

template <int VW> __device__ __forceinline__ void gn_ld(const float *q, float (&v)[VW]) {
    if constexpr (VW == 4) { const float4 t = *reinterpret_cast<const float4 *>(q); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *q;
}
template <int VW> __device__ __forceinline__ void gn_st(float *q, const float (&v)[VW]) {
    if constexpr (VW == 4) *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
    else *q = v[0];
}

// the sum of two values over the team, in every thread: a fixed xor tree inside a wave, the 16 wave sums added in wave order
template <int T> __device__ __forceinline__ void team_sum2(float &a, float &b, float *sm) {
    a = wave_sum_all(a); b = wave_sum_all(b);
    if constexpr (T != 64) {
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { sm[w] = a; sm[16 + w] = b; }
        __syncthreads();
        float ra = 0.f, rb = 0.f;
#pragma unroll
        for (int i = 0; i < T / 64; i++) { ra += sm[i]; rb += sm[16 + i]; }
        __syncthreads();
        a = ra; b = rb;
    }
}

// the column sums of the team: thread (row group j, column) adds the threads (j + h, column), h = h0, h0 / 2 .. 1; threads t < CgV (row group 0) hold the
// result.  A wave does it with shuffles, a workgroup through LDS (red: NV x T floats).  Every thread of the team must arrive.
template <int T, int NV>
__device__ __forceinline__ void team_colsum(float (&acc)[NV], const GnP &p, int t, int j, bool act, float *red) {
    if constexpr (T == 64) {
        for (int h = p.h0; h >= 1; h >>= 1) {
            const bool take = j < h && j + h < p.RT;
#pragma unroll
            for (int v = 0; v < NV; v++) { const float o = __shfl_down(acc[v], h * p.CgV, 64); if (take) acc[v] += o; }
        }
    } else {
        if (p.RT == 1) return;                                            // a column has one thread
#pragma unroll
        for (int v = 0; v < NV; v++) red[v * T + t] = acc[v];
        __syncthreads();
        for (int h = p.h0; h >= 1; h >>= 1) {
            if (act && j < h && j + h < p.RT) {
#pragma unroll
                for (int v = 0; v < NV; v++) red[v * T + t] += red[v * T + t + h * p.CgV];
            }
            __syncthreads();
        }
#pragma unroll
        for (int v = 0; v < NV; v++) acc[v] = red[v * T + t];
        __syncthreads();
    }
}
// t = W dy, rounded wherever it is used: contracted into t - s1 it would be another number than the t that was summed, and a group of one element would
// not get dx = 0
__device__ __forceinline__ float gn_t(float w, float dy) {
#pragma clang fp contract(off)
    return w * dy;
}
// a slab row's cells of one column item: dW at [c], dB at [C + c]
template <int VW> __device__ __forceinline__ void slab_put(float *row, int C, int c, const float (&acc)[2 * VW]) {
#pragma unroll
    for (int v = 0; v < VW; v++) { row[c + v] = acc[v]; row[C + c + v] = acc[VW + v]; }
}

// Workgroup id -> its place in group order.  Workgroup ids go round the 8 XCDs, and the groups of one sample interleave in memory: the Cg floats of group g
// and of group g + 1 share a 128-byte line of every pixel.  With groups dealt in id order the up to 8 workgroups that share a line sit behind 8 different
// L2s and each fetches it over the fabric; with ids w, w + 8, w + 16 .. (one XCD) on CONSECUTIVE groups the second to last reader hit the first one's L2 line.
// A permutation of who does what: no sum changes.
__device__ __forceinline__ unsigned gn_place(unsigned b, unsigned nb) {
    const unsigned per = nb >> 3;
    return b < (per << 3) ? (b & 7u) * per + (b >> 3) : b;
}

// ------------------------------------------------------------------ rungs 1 and 2: the group lives in the team's registers
// T = 64: a workgroup of four waves holds four groups, shuffles only, no LDS and no barrier.  T = 1024: one workgroup per group.
template <int T, int VW>
__global__ void __launch_bounds__(T == 64 ? 256 : T) k_gn_fwd_res(const float *I, float *O, float *XH, const float *__restrict__ W, const float *__restrict__ B,
                                                                  float *__restrict__ STAT, GnP p) {
    constexpr int GPW = T == 64 ? 4 : 1, GN_R = T == 64 ? GN_R1 : GN_R2 * (VW == 1 ? 2 : 1);
    __shared__ float sm[32];
    const int t = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int j = (int)fdiv((unsigned)t, p.dCgV), col = t - j * p.CgV;
    const bool act = t < p.Tact;
    for (long gid = (long)gn_place(blockIdx.x, gridDim.x) * GPW + (T == 64 ? (int)(threadIdx.x >> 6) : 0); gid < p.NG; gid += (long)gridDim.x * GPW) {
        const int n = (int)fdiv((unsigned)gid, p.dG), g = (int)gid - n * p.G;
        const long base = (long)n * p.HW * p.C + (long)g * p.Cg + col * VW;
        const long first = base + (long)j * p.C, step = (long)p.RT * p.C;
        float x[GN_R][VW];
        float s = 0.f, q = 0.f;
        unsigned have = 0;                                                  // bit k: row k of this thread exists (one VGPR, not a lane mask per row in SGPR pairs)
        const float *pi = I + first;
#pragma unroll
        for (int k = 0; k < GN_R; k++, pi += step) {
            const int row = j + k * p.RT;
#pragma unroll
            for (int v = 0; v < VW; v++) x[k][v] = 0.f;
            if (act && row < p.HW) { gn_ld<VW>(pi, x[k]); have |= 1u << k; }
#pragma unroll
            for (int v = 0; v < VW; v++) s += x[k][v];
        }
        team_sum2<T>(s, q, sm);
        const float mean = s / p.fE;
        q = 0.f; s = 0.f;
#pragma unroll
        for (int k = 0; k < GN_R; k++) {
            if ((have >> k) & 1u) {
#pragma unroll
                for (int v = 0; v < VW; v++) { const float d = x[k][v] - mean; q += d * d; }
            }
        }
        team_sum2<T>(q, s, sm);
        const float rstd = 1.0f / sqrtf(q / p.fE + p.eps);
        if (t == 0) { STAT[gid] = mean; STAT[p.NG + gid] = rstd; }
        if (act) {
            float gw[VW], gb[VW];
            gn_ld<VW>(W + g * p.Cg + col * VW, gw); gn_ld<VW>(B + g * p.Cg + col * VW, gb);
            float *po = O + first, *px = XH + first;
#pragma unroll
            for (int k = 0; k < GN_R; k++, po += step, px += step) {
                if ((have >> k) & 1u) {
                    float xh[VW], y[VW];
#pragma unroll
                    for (int v = 0; v < VW; v++) { xh[v] = (x[k][v] - mean) * rstd; y[v] = xh[v] * gw[v] + gb[v]; }
                    gn_st<VW>(px, xh); gn_st<VW>(po, y);
                }
            }
        }
    }
}

template <int T, int VW>
__global__ void __launch_bounds__(T == 64 ? 256 : T) k_gn_bwd_res(const float *__restrict__ W, const float *DY, const float *__restrict__ XH, float *__restrict__ STAT,
                                                                  float *DX, float *__restrict__ slab, GnP p) {
    constexpr int GPW = T == 64 ? 4 : 1, GN_R = T == 64 ? GN_R1 : GN_R2 * (VW == 1 ? 2 : 1);
    __shared__ float sm[32];
    __shared__ float red[T == 64 ? 1 : 2 * VW * T];
    const int t = T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int j = (int)fdiv((unsigned)t, p.dCgV), col = t - j * p.CgV;
    const bool act = t < p.Tact;
    for (long gid = (long)gn_place(blockIdx.x, gridDim.x) * GPW + (T == 64 ? (int)(threadIdx.x >> 6) : 0); gid < p.NG; gid += (long)gridDim.x * GPW) {
        const int n = (int)fdiv((unsigned)gid, p.dG), g = (int)gid - n * p.G;
        const long base = (long)n * p.HW * p.C + (long)g * p.Cg + col * VW;
        float dy[GN_R][VW], xh[GN_R][VW], gw[VW], acc[2 * VW];
#pragma unroll
        for (int v = 0; v < VW; v++) { gw[v] = 0.f; acc[v] = 0.f; acc[VW + v] = 0.f; }
        if (act) gn_ld<VW>(W + g * p.Cg + col * VW, gw);
        float a1 = 0.f, a2 = 0.f;
        const long first = base + (long)j * p.C, step = (long)p.RT * p.C;
        const float *pd = DY + first, *px = XH + first;
        unsigned have = 0;
#pragma unroll
        for (int k = 0; k < GN_R; k++, pd += step, px += step) {
            const int row = j + k * p.RT;
#pragma unroll
            for (int v = 0; v < VW; v++) { dy[k][v] = 0.f; xh[k][v] = 0.f; }
            if (act && row < p.HW) { gn_ld<VW>(pd, dy[k]); gn_ld<VW>(px, xh[k]); have |= 1u << k; }
#pragma unroll
            for (int v = 0; v < VW; v++) {
                const float tt = gn_t(gw[v], dy[k][v]);
                a1 += tt; a2 += tt * xh[k][v];
                acc[v] += dy[k][v] * xh[k][v]; acc[VW + v] += dy[k][v];
            }
        }
        team_sum2<T>(a1, a2, sm);
        const float s1 = a1 / p.fE, s2 = a2 / p.fE, rstd = STAT[p.NG + gid];
        if (t == 0) { STAT[2L * p.NG + gid] = s1; STAT[3L * p.NG + gid] = s2; }
        if (act) {
            float *po = DX + first;
#pragma unroll
            for (int k = 0; k < GN_R; k++, po += step) {
                if ((have >> k) & 1u) {
                    float dx[VW];
#pragma unroll
                    for (int v = 0; v < VW; v++) dx[v] = rstd * (gn_t(gw[v], dy[k][v]) - s1 - xh[k][v] * s2);
                    gn_st<VW>(po, dx);
                }
            }
        }
        if (slab) {                                                        // (uniform over the launch)
            team_colsum<T, 2 * VW>(acc, p, t, j, act, red);
            if (t < p.CgV) slab_put<VW>(slab + (long)n * 2 * p.C, p.C, g * p.Cg + col * VW, acc);
        }
    }
}

// ------------------------------------------------------------------ rungs 3 and 4: the rows [rb, re) of a group, re-read from L2 / HBM by a 1024-thread workgroup
struct GnT { int t, j, col0; bool act; };
__device__ __forceinline__ GnT gn_thread(const GnP &p) {
    GnT m; m.t = (int)threadIdx.x; m.j = (int)fdiv((unsigned)m.t, p.dCgV); m.col0 = m.t - m.j * p.CgV; m.act = m.t < p.Tact;
    return m;
}
// f(offset of the item from the group's first element, column item) for every item the thread owns
template <int VW, typename F>
__device__ __forceinline__ void gn_items(const GnP &p, const GnT &m, int rb, int re, F &&f) {
    for (int cc = 0; cc < p.ncc; cc++) {
        const int col = m.col0 + cc * GN_T;
        if (!m.act || col >= p.CgV) continue;
#pragma unroll 4
        for (int row = rb + m.j; row < re; row += p.RT) f((long)row * p.C + col * VW, col);
    }
}
template <int VW>
__device__ __forceinline__ float gn_sum_rows(const float *I, const GnP &p, const GnT &m, int rb, int re) {
    float s = 0.f;
    gn_items<VW>(p, m, rb, re, [&](long o, int) { float x[VW]; gn_ld<VW>(I + o, x);
#pragma unroll
        for (int v = 0; v < VW; v++) s += x[v]; });
    return s;
}
template <int VW>
__device__ __forceinline__ float gn_sq_rows(const float *I, const GnP &p, const GnT &m, int rb, int re, float mean) {
    float q = 0.f;
    gn_items<VW>(p, m, rb, re, [&](long o, int) { float x[VW]; gn_ld<VW>(I + o, x);
#pragma unroll
        for (int v = 0; v < VW; v++) { const float d = x[v] - mean; q += d * d; } });
    return q;
}
// I, O, XH, W, B already at the group's first element / channel
template <int VW>
__device__ __forceinline__ void gn_apply_rows(const float *I, float *O, float *XH, const float *W, const float *B, const GnP &p, const GnT &m, int rb, int re,
                                              float mean, float rstd) {
    for (int cc = 0; cc < p.ncc; cc++) {
        const int col = m.col0 + cc * GN_T;
        if (!m.act || col >= p.CgV) continue;
        float gw[VW], gb[VW];
        gn_ld<VW>(W + col * VW, gw); gn_ld<VW>(B + col * VW, gb);
#pragma unroll 4
        for (int row = rb + m.j; row < re; row += p.RT) {
            const long o = (long)row * p.C + col * VW;
            float x[VW], xh[VW], y[VW];
            gn_ld<VW>(I + o, x);
#pragma unroll
            for (int v = 0; v < VW; v++) { xh[v] = (x[v] - mean) * rstd; y[v] = xh[v] * gw[v] + gb[v]; }
            gn_st<VW>(XH + o, xh); gn_st<VW>(O + o, y);
        }
    }
}
// the group sums of t = W dy and t xhat over the rows, and the rows' dW | dB partial sums into a slab row (srow: at the group's first channel; NULL: none)
template <int VW>
__device__ __forceinline__ void gn_bwd_sum_rows(const float *W, const float *DY, const float *XH, float *srow, const GnP &p, const GnT &m, int rb, int re,
                                                float *red, float &a1, float &a2) {
    a1 = 0.f; a2 = 0.f;
    for (int cc = 0; cc < p.ncc; cc++) {                                   // (every thread walks every chunk: the column tree has barriers)
        const int col = m.col0 + cc * GN_T;
        const bool ok = m.act && col < p.CgV;
        float acc[2 * VW], gw[VW];
#pragma unroll
        for (int v = 0; v < VW; v++) { acc[v] = 0.f; acc[VW + v] = 0.f; gw[v] = 0.f; }
        if (ok) {
            gn_ld<VW>(W + col * VW, gw);
#pragma unroll 4
            for (int row = rb + m.j; row < re; row += p.RT) {
                const long o = (long)row * p.C + col * VW;
                float dy[VW], xh[VW];
                gn_ld<VW>(DY + o, dy); gn_ld<VW>(XH + o, xh);
#pragma unroll
                for (int v = 0; v < VW; v++) {
                    const float tt = gn_t(gw[v], dy[v]);
                    a1 += tt; a2 += tt * xh[v];
                    acc[v] += dy[v] * xh[v]; acc[VW + v] += dy[v];
                }
            }
        }
        if (srow) {
            team_colsum<GN_T, 2 * VW>(acc, p, m.t, m.j, m.act, red);
            if (ok && m.j == 0) slab_put<VW>(srow, p.C, col * VW, acc);
        }
    }
}
template <int VW>
__device__ __forceinline__ void gn_dx_rows(const float *W, const float *DY, const float *XH, float *DX, const GnP &p, const GnT &m, int rb, int re,
                                           float rstd, float s1, float s2) {
    for (int cc = 0; cc < p.ncc; cc++) {
        const int col = m.col0 + cc * GN_T;
        if (!m.act || col >= p.CgV) continue;
        float gw[VW];
        gn_ld<VW>(W + col * VW, gw);
#pragma unroll 4
        for (int row = rb + m.j; row < re; row += p.RT) {
            const long o = (long)row * p.C + col * VW;
            float dy[VW], xh[VW], dx[VW];
            gn_ld<VW>(DY + o, dy); gn_ld<VW>(XH + o, xh);
#pragma unroll
            for (int v = 0; v < VW; v++) dx[v] = rstd * (gn_t(gw[v], dy[v]) - s1 - xh[v] * s2);
            gn_st<VW>(DX + o, dx);
        }
    }
}

// rung 3: one workgroup per group, three passes forward (sum, centred squares, apply), two backward (sums, dX).  A group here has more than a thousand
// elements, so N G stays below 2^21 and the grid is N G
template <int VW>
__global__ void __launch_bounds__(GN_T) k_gn_fwd_stream(const float *I, float *O, float *XH, const float *__restrict__ W, const float *__restrict__ B,
                                                        float *__restrict__ STAT, GnP p) {
    __shared__ float sm[32];
    const GnT m = gn_thread(p);
    const int gid = (int)gn_place(blockIdx.x, gridDim.x), n = (int)fdiv((unsigned)gid, p.dG), g = gid - n * p.G;
    const long base = (long)n * p.HW * p.C + (long)g * p.Cg;
    float s = gn_sum_rows<VW>(I + base, p, m, 0, p.HW), q = 0.f;
    team_sum2<GN_T>(s, q, sm);
    const float mean = s / p.fE;
    q = gn_sq_rows<VW>(I + base, p, m, 0, p.HW, mean); s = 0.f;
    team_sum2<GN_T>(q, s, sm);                                             // (its barriers also order every read of I before the first store to O, which may be I)
    const float rstd = 1.0f / sqrtf(q / p.fE + p.eps);
    if (m.t == 0) { STAT[gid] = mean; STAT[(long)p.NG + gid] = rstd; }
    gn_apply_rows<VW>(I + base, O + base, XH + base, W + g * p.Cg, B + g * p.Cg, p, m, 0, p.HW, mean, rstd);
}
template <int VW>
__global__ void __launch_bounds__(GN_T) k_gn_bwd_stream(const float *__restrict__ W, const float *DY, const float *__restrict__ XH, float *__restrict__ STAT,
                                                        float *DX, float *__restrict__ slab, GnP p) {
    __shared__ float sm[32];
    __shared__ float red[2 * VW * GN_T];
    const GnT m = gn_thread(p);
    const int gid = (int)gn_place(blockIdx.x, gridDim.x), n = (int)fdiv((unsigned)gid, p.dG), g = gid - n * p.G;
    const long base = (long)n * p.HW * p.C + (long)g * p.Cg;
    float a1, a2;
    gn_bwd_sum_rows<VW>(W + g * p.Cg, DY + base, XH + base, slab ? slab + (long)n * 2 * p.C + g * p.Cg : nullptr, p, m, 0, p.HW, red, a1, a2);
    team_sum2<GN_T>(a1, a2, sm);
    const float s1 = a1 / p.fE, s2 = a2 / p.fE, rstd = STAT[(long)p.NG + gid];
    if (m.t == 0) { STAT[2L * p.NG + gid] = s1; STAT[3L * p.NG + gid] = s2; }
    gn_dx_rows<VW>(W + g * p.Cg, DY + base, XH + base, DX + base, p, m, 0, p.HW, rstd, s1, s2);
}

// rung 4: workgroup b owns part b % P of group b / P, rows [part rp, min(HW, (part + 1) rp)).  The first launch leaves per-part results in the workspace
// (forward: mean and M2 of the part; backward: its two raw sums and its slab row), the second merges a group's parts IN PART ORDER - every workgroup of the
// group the same arithmetic, so all agree - and applies to its own rows.
__device__ __forceinline__ void gn_part_of(const GnP &p, int &gid, int &part, int &rb, int &re) {
    gid = (int)fdiv(blockIdx.x, p.dP); part = (int)blockIdx.x - gid * p.P;
    rb = part * p.rp; re = min(p.HW, rb + p.rp);
}
template <int VW>
__global__ void __launch_bounds__(GN_T) k_gn_fwd_part(const float *__restrict__ I, float *__restrict__ ws, GnP p) {
    __shared__ float sm[32];
    const GnT m = gn_thread(p);
    int gid, part, rb, re; gn_part_of(p, gid, part, rb, re);
    const int n = (int)fdiv((unsigned)gid, p.dG), g = gid - n * p.G;
    const long base = (long)n * p.HW * p.C + (long)g * p.Cg;
    float s = gn_sum_rows<VW>(I + base, p, m, rb, re), q = 0.f;
    team_sum2<GN_T>(s, q, sm);
    const float mean = s / (float)((long)(re - rb) * p.Cg);
    q = gn_sq_rows<VW>(I + base, p, m, rb, re, mean); s = 0.f;
    team_sum2<GN_T>(q, s, sm);
    if (m.t == 0) { ws[2L * blockIdx.x] = mean; ws[2L * blockIdx.x + 1] = q; }
}
template <int VW>
__global__ void __launch_bounds__(GN_T) k_gn_fwd_split(const float *I, float *O, float *XH, const float *__restrict__ W, const float *__restrict__ B,
                                                       float *__restrict__ STAT, const float *__restrict__ ws, GnP p) {
    const GnT m = gn_thread(p);
    int gid, part, rb, re; gn_part_of(p, gid, part, rb, re);
    const int n = (int)fdiv((unsigned)gid, p.dG), g = gid - n * p.G;
    const long base = (long)n * p.HW * p.C + (long)g * p.Cg;
    // Chan, Golub & LeVeque's pairwise update of (count, mean, M2), the parts taken in order
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    for (int k = 0; k < p.P; k++) {
        const float nb = (float)((long)(min(p.HW, (k + 1) * p.rp) - k * p.rp) * p.Cg), mb = ws[2L * (gid * p.P + k)], qb = ws[2L * (gid * p.P + k) + 1];
        if (k == 0) { cnt = nb; mean = mb; m2 = qb; }
        else { const float d = mb - mean, tot = cnt + nb; mean += d * (nb / tot); m2 += qb + d * d * (cnt * (nb / tot)); cnt = tot; }
    }
    const float rstd = 1.0f / sqrtf(m2 / p.fE + p.eps);
    if (m.t == 0 && part == 0) { STAT[gid] = mean; STAT[p.NG + gid] = rstd; }
    gn_apply_rows<VW>(I + base, O + base, XH + base, W + g * p.Cg, B + g * p.Cg, p, m, rb, re, mean, rstd);
}
template <int VW>
__global__ void __launch_bounds__(GN_T) k_gn_bwd_part(const float *__restrict__ W, const float *__restrict__ DY, const float *__restrict__ XH, float *__restrict__ ws,
                                                      float *__restrict__ slab, GnP p) {
    __shared__ float sm[32];
    __shared__ float red[2 * VW * GN_T];
    const GnT m = gn_thread(p);
    int gid, part, rb, re; gn_part_of(p, gid, part, rb, re);
    const int n = (int)fdiv((unsigned)gid, p.dG), g = gid - n * p.G;
    const long base = (long)n * p.HW * p.C + (long)g * p.Cg;
    float a1, a2;
    gn_bwd_sum_rows<VW>(W + g * p.Cg, DY + base, XH + base, slab ? slab + ((long)n * p.P + part) * 2 * p.C + g * p.Cg : nullptr, p, m, rb, re, red, a1, a2);
    team_sum2<GN_T>(a1, a2, sm);
    if (m.t == 0) { ws[2L * blockIdx.x] = a1; ws[2L * blockIdx.x + 1] = a2; }
}
template <int VW>
__global__ void __launch_bounds__(GN_T) k_gn_bwd_split(const float *__restrict__ W, const float *DY, const float *__restrict__ XH, float *__restrict__ STAT,
                                                       float *DX, const float *__restrict__ ws, GnP p) {
    const GnT m = gn_thread(p);
    int gid, part, rb, re; gn_part_of(p, gid, part, rb, re);
    const int n = (int)fdiv((unsigned)gid, p.dG), g = gid - n * p.G;
    const long base = (long)n * p.HW * p.C + (long)g * p.Cg;
    float a1 = 0.f, a2 = 0.f;
    for (int k = 0; k < p.P; k++) { a1 += ws[2L * (gid * p.P + k)]; a2 += ws[2L * (gid * p.P + k) + 1]; }
    const float s1 = a1 / p.fE, s2 = a2 / p.fE, rstd = STAT[p.NG + gid];
    if (m.t == 0 && part == 0) { STAT[2L * p.NG + gid] = s1; STAT[3L * p.NG + gid] = s2; }
    gn_dx_rows<VW>(W + g * p.Cg, DY + base, XH + base, DX + base, p, m, rb, re, rstd, s1, s2);
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_groupnorm_plan reports
struct GnPlan { int rung, vw, gpw, P, rp, nslice, fold; long part_floats; };
int gn_team(int rung) { return rung == 1 ? WAVE : GN_T; }
// admission (who: the entry's name for the message) in 64 bits: the extents may be anything an int holds
int gn_plan(GnPlan &g, const char *who, int N, int HW, int C, int G, bool aligned, long ws_bytes) {
    if (N < 1 || HW < 1 || C < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (N=%d HW=%d C=%d)", who, N, HW, C);
    if (ws_bytes < 0) return fail(T4K_ERR_ARG, "%s: ws_bytes below 0", who);
    if (G < 1 || C % G != 0) return fail(T4K_ERR_UNSUPPORTED, "%s: groups=%d not supported (1 <= G, G divides C=%d)", who, G, C);
    const long lim = 1L << 31, px = (long)N * HW;
    if (px >= lim || px * C >= lim || (long)N * G >= lim) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 elements or groups, or more", who);
    const int Cg = C / G, NG = N * G;
    g.vw = (aligned && Cg % 4 == 0) ? 4 : 1;
    const int cgv = Cg / g.vw;
    const long items = (long)HW * cgv;
    auto rows_per_thread = [&](int T) { const long rt = T / cgv; return (HW + rt - 1) / rt; };
    g.P = 1; g.rp = HW; g.gpw = 1;
    const int dw = g.vw == 1 ? 2 : 1;
    const int lowest = T4K_LAB_ENV("T4K_GN_RUNG", 1);                      // LAB: 2 sends the wave rung's groups to the workgroup rung, 3 every resident group to the stream rung (the threshold sweep)
    if (lowest <= 1 && cgv <= WAVE && rows_per_thread(WAVE) <= GN_R1) { g.rung = 1; g.gpw = 4; }
    else if (lowest <= 2 && cgv <= GN_T && rows_per_thread(GN_T) <= GN_R2 * dw) g.rung = 2;
    else {
        g.rung = 3;
        if (NG < GN_FILL) {                                                // few groups of many elements: cut each into parts of whole rows
            long want = (GN_WANT + NG - 1) / NG;
            want = std::min(want, std::min((long)GN_PMAX, std::min((long)HW, items / GN_PITEMS)));
            if (want >= 2) {
                g.rp = (int)((HW + want - 1) / want); g.P = (int)(((long)HW + g.rp - 1) / g.rp);
                if (g.P >= 2) g.rung = 4; else { g.P = 1; g.rp = HW; }
            }
        }
    }
    g.nslice = N * g.P;                                                    // (N < 2^31 / G, P <= 64 only where N G < 256)
    g.part_floats = g.rung == 4 ? (2L * NG * g.P + 3) / 4 * 4 : 0;
    const long avail = ws_bytes / (long)sizeof(float);
    if (g.part_floats > avail || (long)g.nslice > (avail - g.part_floats) / (2L * C))
        return fail(T4K_ERR_UNSUPPORTED, "%s: the dW | dB slab (%d x %ld floats) does not fit the workspace", who, g.nslice, 2L * C);
    g.fold = g.nslice <= 32 ? 1 : 2;                                       // as conv_geo.hip: few slices x many outputs walk whole slabs, else a wave per output
    return T4K_OK;
}
GnP gn_parms(const GnPlan &g, int N, int HW, int C, int G, float eps) {
    GnP p;
    p.N = N; p.HW = HW; p.C = C; p.G = G; p.Cg = C / G; p.CgV = p.Cg / g.vw; p.NG = N * G;
    const int T = gn_team(g.rung);
    if (p.CgV <= T) { p.RT = T / p.CgV; p.Tact = p.RT * p.CgV; p.ncc = 1; }
    else            { p.RT = 1; p.Tact = T; p.ncc = (int)(((long)p.CgV + T - 1) / T); }
    int h = 1; while (h < p.RT) h <<= 1;
    p.h0 = h >> 1;
    p.P = g.P; p.rp = g.rp;
    p.eps = eps; p.fE = (float)((long)HW * p.Cg);
    p.dCgV = fast_div(p.CgV); p.dG = fast_div(G); p.dP = fast_div(g.P);
    return p;
}
bool gn16(const void *a, const void *b, const void *c, const void *d, const void *e = nullptr, const void *f = nullptr) {
    return aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) && aligned16(e) && aligned16(f);
}

} // namespace

extern "C" {

int t4k_groupnorm_plan(int N, int HW, int C, int G, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_groupnorm_plan: null");
    GnPlan g;
    const int rc = gn_plan(g, "t4k_groupnorm_plan", N, HW, C, G, aligned != 0, ws_bytes); if (rc != T4K_OK) return rc;
    out[0] = g.rung; out[1] = g.vw; out[2] = g.gpw; out[3] = g.P; out[4] = g.rung == 4 ? 2 : 1; out[5] = g.nslice; out[6] = g.fold; out[7] = g.rung == 4 ? 3 : 2;
    return T4K_OK;
}

int t4k_groupnorm_fwd(const float *I, float *O, float *XH, const float *W, const float *B, float *STAT,
                      int N, int HW, int C, int G, float eps, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!I || !O || !XH || !W || !B || !STAT) return fail(T4K_ERR_ARG, "t4k_groupnorm_fwd: null tensor");
    if (!(eps > 0.0f)) return fail(T4K_ERR_ARG, "t4k_groupnorm_fwd: eps must be above 0");
    GnPlan g;
    const int rc = gn_plan(g, "t4k_groupnorm_fwd", N, HW, C, G, gn16(I, O, XH, W, B), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const GnP p = gn_parms(g, N, HW, C, G, eps);
    hipStream_t hs = t4k::S(s);
    float *ws = ws_for(s);
    pick<4, 1>(g.vw, [&](auto vw) {
        constexpr int VW = decltype(vw)::value;
        if (g.rung == 1) T4K_LAUNCH((k_gn_fwd_res<WAVE, VW>), dim3((unsigned)std::min(((long)p.NG + 3) / 4, (long)GN_MAX_WG)), dim3(256), 0, hs, I, O, XH, W, B, STAT, p);
        else if (g.rung == 2) T4K_LAUNCH((k_gn_fwd_res<GN_T, VW>), dim3((unsigned)std::min(p.NG, GN_MAX_WG)), dim3(GN_T), 0, hs, I, O, XH, W, B, STAT, p);
        else if (g.rung == 3) T4K_LAUNCH((k_gn_fwd_stream<VW>), dim3((unsigned)p.NG), dim3(GN_T), 0, hs, I, O, XH, W, B, STAT, p);
        else {
            T4K_LAUNCH((k_gn_fwd_part<VW>), dim3((unsigned)(p.NG * p.P)), dim3(GN_T), 0, hs, I, ws, p);
            T4K_LAUNCH((k_gn_fwd_split<VW>), dim3((unsigned)(p.NG * p.P)), dim3(GN_T), 0, hs, I, O, XH, W, B, STAT, (const float *)ws, p);
        }
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_groupnorm_bwd(const float *W, const float *DY, const float *XH, float *STAT, float *DX,
                      float *DW, float *DB, int N, int HW, int C, int G, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!W || !DY || !XH || !STAT || !DX) return fail(T4K_ERR_ARG, "t4k_groupnorm_bwd: null tensor");
    if (train && (!DW || !DB)) return fail(T4K_ERR_ARG, "t4k_groupnorm_bwd: DW and DB are required when train != 0");
    GnPlan g;
    const int rc = gn_plan(g, "t4k_groupnorm_bwd", N, HW, C, G, gn16(W, DY, XH, DX), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const GnP p = gn_parms(g, N, HW, C, G, 0.0f);
    hipStream_t hs = t4k::S(s);
    float *ws = ws_for(s), *slab = train ? ws + g.part_floats : nullptr;
    pick<4, 1>(g.vw, [&](auto vw) {
        constexpr int VW = decltype(vw)::value;
        if (g.rung == 1) T4K_LAUNCH((k_gn_bwd_res<WAVE, VW>), dim3((unsigned)std::min(((long)p.NG + 3) / 4, (long)GN_MAX_WG)), dim3(256), 0, hs, W, DY, XH, STAT, DX, slab, p);
        else if (g.rung == 2) T4K_LAUNCH((k_gn_bwd_res<GN_T, VW>), dim3((unsigned)std::min(p.NG, GN_MAX_WG)), dim3(GN_T), 0, hs, W, DY, XH, STAT, DX, slab, p);
        else if (g.rung == 3) T4K_LAUNCH((k_gn_bwd_stream<VW>), dim3((unsigned)p.NG), dim3(GN_T), 0, hs, W, DY, XH, STAT, DX, slab, p);
        else {
            T4K_LAUNCH((k_gn_bwd_part<VW>), dim3((unsigned)(p.NG * p.P)), dim3(GN_T), 0, hs, W, DY, XH, ws, slab, p);
            T4K_LAUNCH((k_gn_bwd_split<VW>), dim3((unsigned)(p.NG * p.P)), dim3(GN_T), 0, hs, W, DY, XH, STAT, DX, (const float *)ws, p);
        }
    });
    if (train) {
        if (g.fold == 1 && DB == DW + C) launch_fold_add(slab, DW, 2 * C, g.nslice, hs);
        else launch_df_fold(slab, DW, DB, g.nslice, C, 2 * C, hs);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
