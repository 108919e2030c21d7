// softmax_axes.hip - softmax along any subset of the axes of a dense NHWC tensor: for every index of the unmasked axes
// the elements along the masked axes form one group, x <- exp(x - max_group) / sum_group exp(x - max_group).  k_softmax's arithmetic
// (reduce.hip: max shift, __expf, fp32 sum, one fp32 division per element), fixed trees, no floating-point atomics: the same bits on
// every run.  No reference definition: the reference's only softmax is the layer's row form (_fsoftmax forward.cu:222-243) and the
// whole-tensor word (netvm.cpp:36-39).
#include "axes.h"

using namespace t4k;

namespace {

constexpr int NV = 8;                              // loads (floats, or float4s on the vector path) a lane keeps in registers: the register-resident
                                                   // regime holds a lane's whole share in NV of them, the other regimes walk theirs NV at a time

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

// ---- row family (RowPlan, axes.h); a lane walks its units (a float, or a float4 on the vector path) run by run.  S > 1: PART / NORM.
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
        // the walk (walk_step): unit u of run r, then Gu further along the run, at its end the lane's first unit of the run Gr further
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
                    walk_step(r, u, u0, ub, Gu, Gr);
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
                    walk_step(r, u, u0, ub, Gu, Gr);
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
                        walk_step(r, u, u0, ub, Gu, Gr);
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
                    if (r < rb) { Val<VEC>::ld(xb + r * p.sr1 + u * V, v[i]); cnt = i + 1; walk_step(r, u, u0, ub, Gu, Gr); }
                }
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (i < cnt) {
#pragma unroll
                        for (int q = 0; q < V; q++) v[i][q] = __expf(v[i][q] - m) / sum;
                        Val<VEC>::st(ob + rs * p.sr1 + us * V, v[i]);
                        walk_step(rs, us, u0, ub, Gu, Gr);
                    }
                }
            }
        }
    }
}

// ---- column family (ColPlan, axes.h); max and sum fold over the row groups.  S > 1: PART / NORM.
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
        // the walk (walk_step): row r of outer index j, then TY rows further, at the end the lane's first row of the next outer index
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
                    walk_step(j, r, r0, rb, TY, 1u);
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
                    walk_step(j, r, r0, rb, TY, 1u);
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
                        walk_step(j, r, r0, rb, TY, 1u);
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
                    if (j < jb) { Val<VEC>::ld(xb + j * p.sr1 + r * p.sr0, v[i]); cnt = i + 1; walk_step(j, r, r0, rb, TY, 1u); }
                }
#pragma unroll
                for (int i = 0; i < NV; i++) {
                    if (i < cnt) {
#pragma unroll
                        for (int q = 0; q < V; q++) v[i][q] = __expf(v[i][q] - m[q]) / sum[q];
                        Val<VEC>::st(ob + js * p.sr1 + rs * p.sr0, v[i]);
                        walk_step(js, rs, r0, rb, TY, 1u);
                    }
                }
            }
        }
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

// what the planner decided, for the launcher and for t4k_softmax_axes_plan
struct Plan {
    bool col, vec;
    int regime;                   // 0 register-resident, 1 online, 2 multi-launch
    int chunks;                   // chunks of NV loads a lane walks in pass 1 (the rescales of its running pair)
    RowPlan row; ColPlan cl;
};

// a split costs a workspace of S pairs per group and the merged pair: two floats per group and part, one part reserved
void plan_row(Plan &P, const Merged &m, long ws_floats) {
    RowPlan &p = P.row;
    row_geometry(p, m, P.vec);
    p.shift = row_lanes(p.U * p.r1, NV, p.nout);
    auto slots = [&](long ext_u, long ext_r) {                               // loads of a lane over ext_u units of ext_r runs
        p.su = std::min(p.shift, log2_ceil(ext_u, 8));
        return ceil_div(ext_u, 1L << p.su) * ceil_div(ext_r, (1L << p.shift) >> p.su);
    };
    long n = slots(p.U, p.r1);
    while (n > NV && p.shift < 8) { p.shift = p.shift >= 6 ? 8 : p.shift + 1; n = slots(p.U, p.r1); }   // the ceilings left a lane more than NV: more lanes
    P.regime = n <= NV ? 0 : 1;
    if (P.regime == 1 && row_split(p, 2, 1, ws_floats)) {                    // shift == 8 here
        P.regime = 2;
        n = p.split_u ? slots(p.per, p.r1) : slots(p.U, p.per);
    }
    P.chunks = (int)ceil_div(n, NV);
    p.nitem = ceil_div(p.nout, BLK >> p.shift) * p.S;
}

void plan_col(Plan &P, const Merged &m, long ws_floats) {
    ColPlan &p = P.cl;
    col_geometry(p, m, P.vec);
    const long TY = BLK >> p.sx;
    long n = ceil_div(p.r0, TY) * p.r1;
    P.regime = n <= NV ? 0 : 1;
    if (P.regime == 1 && col_split(p, 2, 1, ws_floats)) {
        P.regime = 2;
        n = p.split_r1 ? ceil_div(p.r0, TY) * p.per : ceil_div(p.per, TY) * p.r1;
    }
    P.chunks = (int)ceil_div(n, NV);
}

int make_plan(Plan &P, const int dim[4], int mask, bool aligned, long ws_floats, const char *who) {
    Merged m;
    const int rc = merge_axes(dim, mask, who, m); if (rc != T4K_OK) return rc;
    P.col = m.col;
    P.vec = aligned && ((m.col ? m.k0 : m.r0) & 3) == 0;                     // every row starts on a multiple of k0 elements, every run on one of r0
    if (m.col) plan_col(P, m, ws_floats); else plan_row(P, m, ws_floats);
    return T4K_OK;
}

template <int MODE, typename PlanT>
void launch(bool vec, const float *X, float *O, float *Wk, const PlanT &p, hipStream_t hs) {
    const int g = (int)std::min(p.nitem, (long)MAX_WG);
    with_flags([&](auto v) {
        if constexpr (std::is_same<PlanT, ColPlan>::value) T4K_LAUNCH((k_smax_col<MODE, v.value>), dim3(g), dim3(BLK), 0, hs, X, O, Wk, p);
        else                                               T4K_LAUNCH((k_smax_row<MODE, v.value>), dim3(g), dim3(BLK), 0, hs, X, O, Wk, p);
    }, vec);
}
template <typename PlanT>
void run(const Plan &P, const PlanT &p, long nout, long os, long ps, const float *X, float *O, hipStream_t hs) {
    if (P.regime == 0) { launch<M_REG>(P.vec, X, O, nullptr, p, hs); return; }
    if (P.regime == 1) { launch<M_ONLINE>(P.vec, X, O, nullptr, p, hs); return; }
    float *part = ws_for(hs), *fin = part + 2 * nout * (long)p.S;            // S pairs per group, then the merged pair of every group
    launch<M_PART>(P.vec, X, O, part, p, hs);
    const unsigned g = log2_ceil(p.S, 6);
    const int grid = (int)std::min(ceil_div(nout, BLK >> g), (long)MAX_WG);
    T4K_LAUNCH(k_smax_merge, dim3(grid), dim3(BLK), 0, hs, part, fin, nout, p.S, os, ps, g);
    launch<M_NORM>(P.vec, X, O, fin, p, hs);
}

} // namespace

extern "C" {

int t4k_softmax_axes(const float *src, float *dst, const int dim[4], int mask, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!src || !dst) return fail(T4K_ERR_ARG, "t4k_softmax_axes: null");
    long total; Plan P;
    int rc = check_axes(dim, mask, "t4k_softmax_axes", &total); if (rc != T4K_OK) return rc;
    if (src != dst && src < dst + total && dst < src + total) return fail(T4K_ERR_ARG, "t4k_softmax_axes: dst overlaps src");
    rc = make_plan(P, dim, mask, aligned16(src) && aligned16(dst), (long)(st().ws_bytes / sizeof(float)), "t4k_softmax_axes"); if (rc != T4K_OK) return rc;
    if (P.col) run(P, P.cl, P.cl.nout, 1, P.cl.nout, src, dst, S(s));        // pairs laid out [S, groups]
    else       run(P, P.row, P.row.nout, (long)P.row.S, 1, src, dst, S(s));  // a row of S pairs per group
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

int t4k_softmax_axes_plan(const int dim[4], int mask, int aligned, int out[6]) {
    T4K_REQUIRE_INIT();
    if (!out) return fail(T4K_ERR_ARG, "t4k_softmax_axes_plan: null");
    long total; Plan P;
    int rc = check_axes(dim, mask, "t4k_softmax_axes_plan", &total); if (rc != T4K_OK) return rc;
    rc = make_plan(P, dim, mask, aligned != 0, (long)(st().ws_bytes / sizeof(float)), "t4k_softmax_axes_plan"); if (rc != T4K_OK) return rc;
    out[0] = P.col ? 1 : 0; out[1] = P.regime; out[2] = P.vec ? 1 : 0;
    out[3] = P.col ? (int)P.cl.sx : (int)P.row.shift;
    out[4] = P.col ? (int)P.cl.S : (int)P.row.S;
    out[5] = P.regime == 0 ? 0 : P.chunks + 1 + (P.regime == 2 ? 1 : 0);     // rescales on an element's way into the sum: the lane's chunks, lane -> group, part -> whole
    return T4K_OK;
}

int t4k_softmax_axes_geometry(const int dim[4], int mask, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_softmax_axes_geometry: null");
    long total, ws_floats; Plan P;
    int rc = check_axes(dim, mask, "t4k_softmax_axes_geometry", &total); if (rc != T4K_OK) return rc;
    rc = plan_workspace(ws_bytes, "t4k_softmax_axes_geometry", &ws_floats); if (rc != T4K_OK) return rc;
    rc = make_plan(P, dim, mask, aligned != 0, ws_floats, "t4k_softmax_axes_geometry"); if (rc != T4K_OK) return rc;
    const int launches = P.regime == 2 ? 3 : 1;
    if (P.col) report_plan(out, P.cl, P.vec, launches); else report_plan(out, P.row, P.vec, launches);
    return T4K_OK;
}

} // extern "C"
