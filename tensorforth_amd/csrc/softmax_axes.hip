// softmax_axes.hip - softmax along any subset of the axes of a dense NHWC tensor: for every index of the unmasked axes
// the elements along the masked axes form one group, x <- exp(x - max_group) / sum_group exp(x - max_group).  k_softmax's arithmetic
// (reduce.hip: max shift, __expf, fp32 sum, one fp32 division per element), fixed trees, no floating-point atomics: the same bits on
// every run.  No reference definition: the reference's only softmax is the layer's row form (_fsoftmax forward.cu:222-243) and the
// whole-tensor word (netvm.cpp:36-39).
#include "t4k_common.h"
#include <float.h>
#include <type_traits>

using namespace t4k;

namespace {

// x = q * d + rem; the 32-bit divide whenever x fits.  Used once per workgroup iteration or once per group, never per element.
__device__ __forceinline__ void divmod(long x, unsigned d, long &q, unsigned &rem) {
    if (x < 0xffffffffL) { const unsigned v = (unsigned)x, t = v / d; rem = v - t * d; q = (long)t; }
    else { const long t = x / (long)d; rem = (unsigned)(x - t * (long)d); q = t; }
}

// the planner's constants: the first two and MAX_SPLIT / SPLIT_UNITS are k_red_row's (reduce_axes.hip), the third is this unit's
constexpr long TARGET_LANES = 64L * 4 * 256 * 2;   // two waves on every SIMD of 256 CUs: below this a group gets more lanes
constexpr long TARGET_ITEMS = 1024;                // workgroups a split aims for: four on every CU
constexpr int  NV           = 8;                   // loads (floats, or float4s on the vector path) a lane keeps in registers: the register-resident
                                                   // regime holds a lane's whole share in NV of them, the other regimes walk theirs NV at a time
constexpr long SPLIT_UNITS  = 8;                   // loads a lane keeps at least when a group is split across workgroups
constexpr long MAX_SPLIT    = 4096;

// what a launch does.  REG: a lane's share of the group stays in registers (read once, written once).  ONLINE: pass 1 keeps a running
// (max, sum), pass 2 reads again and writes.  PART: pass 1 over one part of a group, the pair left in the workspace.  NORM: pass 2 with
// the merged pair read from the workspace.
enum { M_REG = 0, M_ONLINE, M_PART, M_NORM };

template <bool VEC> struct Val;
template <> struct Val<true> {
    static constexpr int V = 4;
    static __device__ __forceinline__ void ld(const float *p, float (&d)[4]) { const float4 t = *reinterpret_cast<const float4 *>(p); d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w; }
    static __device__ __forceinline__ void st(float *p, const float (&d)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(d[0], d[1], d[2], d[3]); }
};
template <> struct Val<false> {
    static constexpr int V = 1;
    static __device__ __forceinline__ void ld(const float *p, float (&d)[1]) { d[0] = *p; }
    static __device__ __forceinline__ void st(float *p, const float (&d)[1]) { *p = d[0]; }
};

// ---- row family: the innermost merged group is reduced.  Group o is r1 runs (sr1 apart) of r0 contiguous floats starting at
// base(o) = o * sk0, or (o / k0) * sk1 + (o % k0) * sk0 when a second kept group lies outside the runs.  1 << shift lanes share a group
// (shift 0..5: several groups per wave, 6: a wave per group, 8: a workgroup per group), 1 << su of them side by side along a run and
// the rest over the runs; a lane walks its units (a float, or a float4 on the vector path) run by run with two counters, no division.
// S > 1 (PART / NORM): the units of a run (split_u) or the runs are dealt to S workgroups of `per` each.
struct RowPlan {
    long nout, U, r1;             // groups, units per run, runs per group
    long sk0, sr1, sk1, per, nitem;
    unsigned k0, shift, su, S;
    int four, split_u;
};

template <bool MAX> __device__ __forceinline__ float row_fold(float v, unsigned G, unsigned shift, float *sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const float t = __shfl_xor(v, off, 64); if ((unsigned)off < G) v = MAX ? fmaxf(v, t) : v + t; }
    if (shift == 8) {                                                       // the four waves of a workgroup-wide group through LDS
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
        __syncthreads();
        v = MAX ? fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])) : (sm[0] + sm[1]) + (sm[2] + sm[3]);
        __syncthreads();
    }
    return v;
}

// X and O may be the same tensor: neither is __restrict__, and within a pass a lane loads a whole chunk before it stores any of it
template <int MODE, bool VEC>
__global__ void __launch_bounds__(BLK) k_smax_row(const float *X, float *O, float *Wk, const RowPlan p) {
    constexpr int V = Val<VEC>::V;
    __shared__ float sm[4];
    const unsigned G = 1u << p.shift, Gu = 1u << p.su, Gr = G >> p.su;
    const unsigned l = threadIdx.x & (G - 1), lu = l & (Gu - 1), lr = l >> p.su;
    const unsigned opb = (unsigned)BLK >> p.shift;
    for (long w = blockIdx.x; w < p.nitem; w += gridDim.x) {
        long og = w; unsigned s = 0;
        if (p.S > 1) divmod(w, p.S, og, s);                                 // uniform over the workgroup
        const long o = og * opb + (threadIdx.x >> p.shift);
        const bool live = o < p.nout;
        long base = 0, ra = 0, rb = p.r1, ua = 0, ub = p.U;
        if (live) {
            if (p.four) { long q; unsigned i; divmod(o, p.k0, q, i); base = q * p.sk1 + (long)i * p.sk0; }
            else base = o * p.sk0;
        }
        if (p.S > 1) {
            if (p.split_u) { ua = (long)s * p.per; ub = min(p.U, ua + p.per); }
            else           { ra = (long)s * p.per; rb = min(p.r1, ra + p.per); }
        }
        const long u0 = ua + lu, r0 = ra + lr;
        if (!live || u0 >= ub) rb = ra;                                     // nothing for this lane
        const float *xb = X + base; float *ob = O + base;
        // the walk: unit u of run r, then Gu further along the run, at its end the lane's first unit of the run Gr further
#define ROW_STEP(r, u) do { u += Gu; if (u >= ub) { u = u0; r += Gr; } } while (0)
        float m = -FLT_MAX, sum = 0.0f;
        if (MODE == M_REG) {
            float v[NV][V]; int cnt = 0;
            long r = r0, u = u0;
#pragma unroll
            for (int i = 0; i < NV; i++) {
                if (r < rb) {
                    Val<VEC>::ld(xb + r * p.sr1 + u * V, v[i]); cnt = i + 1;
#pragma unroll
                    for (int q = 0; q < V; q++) m = fmaxf(m, v[i][q]);
                    ROW_STEP(r, u);
                }
            }
            m = row_fold<true>(m, G, p.shift, sm);
            float a[V];
#pragma unroll
            for (int q = 0; q < V; q++) a[q] = 0.0f;
#pragma unroll
            for (int i = 0; i < NV; i++) {
                if (i < cnt) {
#pragma unroll
                    for (int q = 0; q < V; q++) { v[i][q] = __expf(v[i][q] - m); a[q] += v[i][q]; }
                }
            }
            sum = VEC ? (a[0] + a[V > 1 ? 1 : 0]) + (a[V > 2 ? 2 : 0] + a[V > 3 ? 3 : 0]) : a[0];
            sum = row_fold<false>(sum, G, p.shift, sm);
            r = r0; u = u0;
#pragma unroll
            for (int i = 0; i < NV; i++) {
                if (i < cnt) {
#pragma unroll
                    for (int q = 0; q < V; q++) v[i][q] = v[i][q] / sum;
                    Val<VEC>::st(ob + r * p.sr1 + u * V, v[i]);
                    ROW_STEP(r, u);
                }
            }
            continue;
        }
        if (MODE == M_ONLINE || MODE == M_PART) {                           // pass 1: one rescale per chunk of NV loads
            long r = r0, u = u0;
            while (r < rb) {
                float v[NV][V]; int cnt = 0; float cm = -FLT_MAX;
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (r < rb) {
                        Val<VEC>::ld(xb + r * p.sr1 + u * V, v[i]); cnt = i + 1;
#pragma unroll
                        for (int q = 0; q < V; q++) cm = fmaxf(cm, v[i][q]);
                        ROW_STEP(r, u);
                    }
                }
                const float mn = fmaxf(m, cm);
                float cs = 0.0f;
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (i < cnt) {
#pragma unroll
                        for (int q = 0; q < V; q++) cs += __expf(v[i][q] - mn);
                    }
                }
                sum = sum * __expf(m - mn) + cs; m = mn;
            }
            const float mg = row_fold<true>(m, G, p.shift, sm);
            sum = row_fold<false>(sum * __expf(m - mg), G, p.shift, sm);
            m = mg;
            if (MODE == M_PART) {
                if (live && l == 0) { Wk[2 * (o * (long)p.S + s)] = m; Wk[2 * (o * (long)p.S + s) + 1] = sum; }
                continue;
            }
        }
        if (MODE == M_NORM && live) { m = Wk[2 * o]; sum = Wk[2 * o + 1]; }
        {                                                                   // pass 2
            long r = r0, u = u0;
            while (r < rb) {
                float v[NV][V]; int cnt = 0;
                long rs = r, us = u;
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (r < rb) { Val<VEC>::ld(xb + r * p.sr1 + u * V, v[i]); cnt = i + 1; ROW_STEP(r, u); }
                }
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (i < cnt) {
#pragma unroll
                        for (int q = 0; q < V; q++) v[i][q] = __expf(v[i][q] - m) / sum;
                        Val<VEC>::st(ob + rs * p.sr1 + us * V, v[i]);
                        ROW_STEP(rs, us);
                    }
                }
            }
        }
#undef ROW_STEP
    }
}

// ---- column family: the innermost merged group (k0 floats) is kept.  A workgroup iteration takes one tile of TX = 1 << sx lanes along
// k0 (one column a lane, four on the vector path: every load of a wave is a contiguous run) of one outer kept index; its 256 >> sx row
// groups deal the reduced rows (r0 of them sr0 apart, inside r1 of them sr1 apart) among themselves.  Max and sum fold inside the wave by
// xor shuffles over the lane bits above sx, the four waves through LDS.  S > 1 (PART / NORM): the rows (or the outer reduced extent,
// split_r1) are dealt to S workgroups.
struct ColPlan {
    long k0, r0, r1, sr0, sk1, sr1, per, nitem, nout;
    unsigned sx, ntile, S;
    int split_r1;
};

// every lane leaves with the fold of its own columns over all row groups
template <bool MAX, int V> __device__ __forceinline__ void col_fold(float (&a)[V], unsigned TX, unsigned tx, float (*sm)[64 * V]) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < V; q++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const float f = __shfl_xor(a[q], off, 64); if ((unsigned)off >= TX) a[q] = MAX ? fmaxf(a[q], f) : a[q] + f; }
    }
    if (lane < TX) {
#pragma unroll
        for (int q = 0; q < V; q++) sm[wave][lane * V + q] = a[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < V; q++) {
        const float s0 = sm[0][tx * V + q], s1 = sm[1][tx * V + q], s2 = sm[2][tx * V + q], s3 = sm[3][tx * V + q];
        a[q] = MAX ? fmaxf(fmaxf(s0, s1), fmaxf(s2, s3)) : (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
}

template <int MODE, bool VEC>
__global__ void __launch_bounds__(BLK) k_smax_col(const float *X, float *O, float *Wk, const ColPlan p) {
    constexpr int V = Val<VEC>::V;
    __shared__ float sm[4][64 * V];
    const unsigned TX = 1u << p.sx, TY = (unsigned)BLK >> p.sx;
    const unsigned tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> p.sx;
    for (long w = blockIdx.x; w < p.nitem; w += gridDim.x) {
        long t = w; unsigned s = 0, tile = 0;
        if (p.S > 1) divmod(t, p.S, t, s);                                  // uniform over the workgroup
        if (p.ntile > 1) divmod(t, p.ntile, t, tile);
        const long ik1 = t;
        const long col = (((long)tile << p.sx) + tx) * V;
        const bool live = col < p.k0;
        long ra = 0, rb = p.r0, ja = 0, jb = p.r1;
        if (p.S > 1) {
            if (p.split_r1) { ja = (long)s * p.per; jb = min(p.r1, ja + p.per); }
            else            { ra = (long)s * p.per; rb = min(p.r0, ra + p.per); }
        }
        const long r0 = ra + ty;
        if (!live || r0 >= rb) jb = ja;                                     // nothing for this lane
        const long off = ik1 * p.sk1 + (live ? col : 0);
        const float *xb = X + off; float *ob = O + off;
        // the walk: row r of outer index j, then TY rows further, at the end the lane's first row of the next outer index
#define COL_STEP(j, r) do { r += TY; if (r >= rb) { r = r0; j++; } } while (0)
        float m[V], sum[V];
#pragma unroll
        for (int q = 0; q < V; q++) { m[q] = -FLT_MAX; sum[q] = 0.0f; }
        if (MODE == M_REG) {
            float v[NV][V]; int cnt = 0;
            long j = ja, r = r0;
#pragma unroll
            for (int i = 0; i < NV; i++) {
                if (j < jb) {
                    Val<VEC>::ld(xb + j * p.sr1 + r * p.sr0, v[i]); cnt = i + 1;
#pragma unroll
                    for (int q = 0; q < V; q++) m[q] = fmaxf(m[q], v[i][q]);
                    COL_STEP(j, r);
                }
            }
            col_fold<true, V>(m, TX, tx, sm);
#pragma unroll
            for (int i = 0; i < NV; i++) {
                if (i < cnt) {
#pragma unroll
                    for (int q = 0; q < V; q++) { v[i][q] = __expf(v[i][q] - m[q]); sum[q] += v[i][q]; }
                }
            }
            col_fold<false, V>(sum, TX, tx, sm);
            j = ja; r = r0;
#pragma unroll
            for (int i = 0; i < NV; i++) {
                if (i < cnt) {
#pragma unroll
                    for (int q = 0; q < V; q++) v[i][q] = v[i][q] / sum[q];
                    Val<VEC>::st(ob + j * p.sr1 + r * p.sr0, v[i]);
                    COL_STEP(j, r);
                }
            }
            continue;
        }
        if (MODE == M_ONLINE || MODE == M_PART) {                           // pass 1: one rescale per chunk of NV rows
            long j = ja, r = r0;
            while (j < jb) {
                float v[NV][V], cm[V]; int cnt = 0;
#pragma unroll
                for (int q = 0; q < V; q++) cm[q] = -FLT_MAX;
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (j < jb) {
                        Val<VEC>::ld(xb + j * p.sr1 + r * p.sr0, v[i]); cnt = i + 1;
#pragma unroll
                        for (int q = 0; q < V; q++) cm[q] = fmaxf(cm[q], v[i][q]);
                        COL_STEP(j, r);
                    }
                }
#pragma unroll
                for (int q = 0; q < V; q++) {
                    const float mn = fmaxf(m[q], cm[q]);
                    float cs = 0.0f;
#pragma unroll
                    for (int i = 0; i < NV; i++) if (i < cnt) cs += __expf(v[i][q] - mn);
                    sum[q] = sum[q] * __expf(m[q] - mn) + cs; m[q] = mn;
                }
            }
            float mg[V];
#pragma unroll
            for (int q = 0; q < V; q++) mg[q] = m[q];
            col_fold<true, V>(mg, TX, tx, sm);
#pragma unroll
            for (int q = 0; q < V; q++) { sum[q] = sum[q] * __expf(m[q] - mg[q]); m[q] = mg[q]; }
            col_fold<false, V>(sum, TX, tx, sm);
            if (MODE == M_PART) {
                if (live && ty == 0) {
#pragma unroll
                    for (int q = 0; q < V; q++) { const long at = 2 * ((long)s * p.nout + ik1 * p.k0 + col + q); Wk[at] = m[q]; Wk[at + 1] = sum[q]; }
                }
                continue;
            }
        }
        if (MODE == M_NORM && live) {
#pragma unroll
            for (int q = 0; q < V; q++) { const long at = 2 * (ik1 * p.k0 + col + q); m[q] = Wk[at]; sum[q] = Wk[at + 1]; }
        }
        {                                                                   // pass 2
            long j = ja, r = r0;
            while (j < jb) {
                float v[NV][V]; int cnt = 0;
                long js = j, rs = r;
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (j < jb) { Val<VEC>::ld(xb + j * p.sr1 + r * p.sr0, v[i]); cnt = i + 1; COL_STEP(j, r); }
                }
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (i < cnt) {
#pragma unroll
                        for (int q = 0; q < V; q++) v[i][q] = __expf(v[i][q] - m[q]) / sum[q];
                        Val<VEC>::st(ob + js * p.sr1 + rs * p.sr0, v[i]);
                        COL_STEP(js, rs);
                    }
                }
            }
        }
#undef COL_STEP
    }
}

// ---- merge: the S (max, sum) pairs of a group, at Wk[2 * (o * os + s * ps)], into one pair F[2 * o]: the max of the maxima, then the
// sums rescaled to it and added in index order by 1 << g lanes (a fixed xor tree over them)
__global__ void __launch_bounds__(BLK) k_smax_merge(const float *__restrict__ Wk, float *__restrict__ F, long nout, unsigned S, long os, long ps, unsigned g) {
    const unsigned G = 1u << g, l = threadIdx.x & (G - 1), opb = (unsigned)BLK >> g;
    for (long w = blockIdx.x; w * opb < nout; w += gridDim.x) {
        const long o = w * opb + (threadIdx.x >> g);
        const bool live = o < nout;
        float m = -FLT_MAX, a = 0.0f;
        if (live) for (unsigned s = l; s < S; s += G) m = fmaxf(m, Wk[2 * (o * os + (long)s * ps)]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const float t = __shfl_xor(m, off, 64); if ((unsigned)off < G) m = fmaxf(m, t); }
        if (live) for (unsigned s = l; s < S; s += G) { const long at = 2 * (o * os + (long)s * ps); a += Wk[at + 1] * __expf(Wk[at] - m); }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const float t = __shfl_xor(a, off, 64); if ((unsigned)off < G) a += t; }
        if (live && l == 0) { F[2 * o] = m; F[2 * o + 1] = a; }
    }
}

inline unsigned log2_ceil(long x, unsigned cap) { unsigned k = 0; while (k < cap && (1L << k) < x) k++; return k; }
inline long ceil_div(long a, long b) { return (a + b - 1) / b; }
// how many workgroups share one group: enough for TARGET_ITEMS, never leaving a lane fewer than SPLIT_UNITS loads, never more pairs
// (S per group and the merged one) than the stream's workspace holds
inline long split_for(long items, long max_by_work, long nout) {
    long S = std::min(std::min(ceil_div(TARGET_ITEMS, items), max_by_work), MAX_SPLIT);
    S = std::min(S, (long)(st().ws_bytes / sizeof(float)) / (2 * nout) - 1);
    return S < 2 ? 1 : S;
}

// what the planner decided, for the launcher and for t4k_softmax_axes_plan
struct Plan {
    bool col, vec;
    int regime;                   // 0 register-resident, 1 online, 2 multi-launch
    int chunks;                   // chunks of NV loads a lane walks in pass 1 (the rescales of its running pair)
    RowPlan row; ColPlan cl;
};

void plan_row(Plan &P, long nout, long r0, long r1, long k0, bool four, bool vec) {
    RowPlan &p = P.row; p = RowPlan{};
    P.col = false; P.vec = vec;
    p.nout = nout; p.U = vec ? r0 >> 2 : r0; p.r1 = r1; p.k0 = (unsigned)k0; p.four = four;
    p.sk0 = r0; p.sr1 = r0 * k0; p.sk1 = r0 * k0 * r1;
    const long T = p.U * r1;                                                 // loads behind one group
    p.shift = log2_ceil(ceil_div(T, NV), 8);
    const unsigned cap = log2_ceil(T, 8);
    while (p.shift < cap && (nout << p.shift) < TARGET_LANES) p.shift++;
    if (p.shift == 7) p.shift = (nout << 6) >= TARGET_LANES ? 6 : 8;         // a wave or a workgroup: nothing between
    auto slots = [&](long ext_u) {
        p.su = std::min(p.shift, log2_ceil(ext_u, 8));
        return ceil_div(ext_u, 1L << p.su) * ceil_div(r1, (1L << p.shift) >> p.su);
    };
    long n = slots(p.U);
    while (n > NV && p.shift < 8) { p.shift = p.shift >= 6 ? 8 : p.shift + 1; n = slots(p.U); }   // the ceilings left a lane more than NV: more lanes
    p.S = 1; p.split_u = 0; p.per = 0;
    P.regime = n <= NV ? 0 : 1;
    if (P.regime == 1) {                                                     // shift == 8 here
        const long S = split_for(nout, T / (BLK * SPLIT_UNITS), nout);
        if (S > 1) {
            P.regime = 2;
            p.split_u = p.U >= r1;
            const long ext = p.split_u ? p.U : r1;
            p.per = ceil_div(ext, S); p.S = (unsigned)ceil_div(ext, p.per);
            n = p.split_u ? slots(p.per) : ceil_div(p.U, 1L << p.su) * ceil_div(p.per, (1L << p.shift) >> p.su);
        }
    }
    P.chunks = (int)ceil_div(n, NV);
    p.nitem = ceil_div(nout, BLK >> p.shift) * p.S;
}

void plan_col(Plan &P, long k0, long r0, long k1, long r1, bool vec) {
    ColPlan &p = P.cl; p = ColPlan{};
    P.col = true; P.vec = vec;
    p.k0 = k0; p.r0 = r0; p.r1 = r1; p.sr0 = k0; p.sk1 = k0 * r0; p.sr1 = k0 * r0 * k1; p.nout = k0 * k1;
    const long Uk = vec ? k0 >> 2 : k0;
    p.sx = log2_ceil(Uk, 6);
    const long TY = BLK >> p.sx;
    p.ntile = (unsigned)ceil_div(Uk, 1L << p.sx);
    const long items = k1 * p.ntile;
    p.S = 1; p.split_r1 = 0; p.per = 0;
    long n = ceil_div(r0, TY) * r1;
    P.regime = n <= NV ? 0 : 1;
    if (P.regime == 1 && items < TARGET_ITEMS) {
        const bool by_r1 = r1 > r0;
        const long S = split_for(items, by_r1 ? r1 / 4 : r0 / (TY * SPLIT_UNITS), p.nout);
        if (S > 1) {
            P.regime = 2;
            p.split_r1 = by_r1;
            const long ext = by_r1 ? r1 : r0;
            p.per = ceil_div(ext, S); p.S = (unsigned)ceil_div(ext, p.per);
            n = by_r1 ? ceil_div(r0, TY) * p.per : ceil_div(p.per, TY) * r1;
        }
    }
    P.chunks = (int)ceil_div(n, NV);
    p.nitem = items * p.S;
}

// axes of extent 1 drop out, neighbours that are both kept or both reduced merge: at most four alternating groups (as t4k_reduce_axes)
int make_plan(Plan &P, const int dim[4], int mask, bool aligned, const char *who) {
    long e[5]; bool red[5]; int n = 0; bool any = false;
    for (int i = 0; i < 4; i++) {
        if (dim[i] == 1) continue;
        const bool r = (mask & (8 >> i)) != 0;
        any = any || r;
        if (n && red[n - 1] == r) e[n - 1] *= dim[i];
        else { e[n] = dim[i]; red[n] = r; n++; }
    }
    if (!any) { e[n] = 1; red[n] = true; n++; }                              // only axes of extent 1 are masked: every element is its own group
    if (red[n - 1]) {
        const long r0 = e[n - 1], k0 = n >= 2 ? e[n - 2] : 1, r1 = n >= 3 ? e[n - 3] : 1, k1 = n >= 4 ? e[n - 4] : 1;
        if (k0 > 0xffffffffL) return fail(T4K_ERR_ARG, "%s: merged extent too large", who);
        plan_row(P, k0 * k1, r0, r1, k0, n == 4, aligned && (r0 & 3) == 0);  // every run starts on a multiple of r0 elements
    } else {
        const long k0 = e[n - 1], r0 = e[n - 2], k1 = n >= 3 ? e[n - 3] : 1, r1 = n >= 4 ? e[n - 4] : 1;
        plan_col(P, k0, r0, k1, r1, aligned && (k0 & 3) == 0);               // every row starts on a multiple of k0 elements
    }
    return T4K_OK;
}

int check_args(const float *src, float *dst, const int dim[4], int mask, bool pointers, const char *who) {
    if ((pointers && (!src || !dst)) || !dim) return fail(T4K_ERR_ARG, "%s: null", who);
    if (mask < 1 || mask > 15) return fail(T4K_ERR_ARG, "%s: mask %d outside 1..15", who, mask);
    long total = 1;
    for (int i = 0; i < 4; i++) {
        if (dim[i] < 1) return fail(T4K_ERR_ARG, "%s: extent %d", who, dim[i]);
        if (total > (1L << 40) / dim[i]) return fail(T4K_ERR_ARG, "%s: more than 2^40 elements", who);
        total *= dim[i];
    }
    if (pointers && src != dst && src < dst + total && dst < src + total) return fail(T4K_ERR_ARG, "%s: dst overlaps src", who);
    return T4K_OK;
}

template <int MODE, typename PlanT>
void launch(bool col, bool vec, const float *X, float *O, float *Wk, const PlanT &p, hipStream_t hs) {
    const int g = (int)std::min(p.nitem, (long)MAX_WG);
    if constexpr (std::is_same<PlanT, ColPlan>::value) {
        if (vec) T4K_LAUNCH((k_smax_col<MODE, true>), dim3(g), dim3(BLK), 0, hs, X, O, Wk, p);
        else     T4K_LAUNCH((k_smax_col<MODE, false>), dim3(g), dim3(BLK), 0, hs, X, O, Wk, p);
    } else {
        if (vec) T4K_LAUNCH((k_smax_row<MODE, true>), dim3(g), dim3(BLK), 0, hs, X, O, Wk, p);
        else     T4K_LAUNCH((k_smax_row<MODE, false>), dim3(g), dim3(BLK), 0, hs, X, O, Wk, p);
    }
}
template <typename PlanT>
void run(const Plan &P, const PlanT &p, long nout, long os, long ps, const float *X, float *O, hipStream_t hs) {
    if (P.regime == 0) { launch<M_REG>(P.col, P.vec, X, O, nullptr, p, hs); return; }
    if (P.regime == 1) { launch<M_ONLINE>(P.col, P.vec, X, O, nullptr, p, hs); return; }
    float *part = ws_for(hs), *fin = part + 2 * nout * (long)p.S;            // S pairs per group, then the merged pair of every group
    launch<M_PART>(P.col, P.vec, X, O, part, p, hs);
    const unsigned g = log2_ceil(p.S, 6);
    const int grid = (int)std::min(ceil_div(nout, BLK >> g), (long)MAX_WG);
    T4K_LAUNCH(k_smax_merge, dim3(grid), dim3(BLK), 0, hs, part, fin, nout, p.S, os, ps, g);
    launch<M_NORM>(P.col, P.vec, X, O, fin, p, hs);
}

} // namespace

extern "C" {

int t4k_softmax_axes(const float *src, float *dst, const int dim[4], int mask, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    int rc = check_args(src, dst, dim, mask, true, "t4k_softmax_axes"); if (rc != T4K_OK) return rc;
    Plan P;
    rc = make_plan(P, dim, mask, aligned16(src) && aligned16(dst), "t4k_softmax_axes"); if (rc != T4K_OK) return rc;
    if (P.col) run(P, P.cl, P.cl.nout, 1, P.cl.nout, src, dst, S(s));        // pairs laid out [S, groups]
    else       run(P, P.row, P.row.nout, (long)P.row.S, 1, src, dst, S(s));  // a row of S pairs per group
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

int t4k_softmax_axes_plan(const int dim[4], int mask, int aligned, int out[6]) {
    T4K_REQUIRE_INIT();
    if (!out) return fail(T4K_ERR_ARG, "t4k_softmax_axes_plan: null");
    int rc = check_args(nullptr, nullptr, dim, mask, false, "t4k_softmax_axes_plan"); if (rc != T4K_OK) return rc;
    Plan P;
    rc = make_plan(P, dim, mask, aligned != 0, "t4k_softmax_axes_plan"); if (rc != T4K_OK) return rc;
    out[0] = P.col ? 1 : 0; out[1] = P.regime; out[2] = P.vec ? 1 : 0;
    out[3] = P.col ? (int)P.cl.sx : (int)P.row.shift;
    out[4] = P.col ? (int)P.cl.S : (int)P.row.S;
    out[5] = P.regime == 0 ? 0 : P.chunks + 1 + (P.regime == 2 ? 1 : 0);     // rescales on an element's way into the sum: the lane's chunks, lane -> group, part -> whole
    return T4K_OK;
}

} // extern "C"
