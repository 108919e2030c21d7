// reduce_axes.hip - sum / n*var / max / min along any subset of the axes of a dense NHWC tensor, keepdims layout.
// Deterministic like reduce.hip: fixed trees, no floating-point atomics, the same bits on every run.  No reference definition: the
// reference's k_sum / k_nvar / k_max (src/t4math.cu:23-131) fold a whole tensor into one scalar, and its only axis reductions are
// welded to nn layers (k_dlinear_db nmath.cu:274, k_batchnorm_1 :177, the softmax row sum forward.cu:222-243).
#include "axes.h"

using namespace t4k;

namespace {

constexpr long LANE_UNITS = 16;                    // loads a lane should have before an output gets more lanes

// ---- row family (RowPlan, axes.h).  S > 1: the parts leave partials O[o * S + s] for a second launch of this kernel (a row of S partials
// per output).
template <int OP, bool VEC>
__global__ void __launch_bounds__(BLK) k_red_row(const float *__restrict__ X, const float *__restrict__ Cn, float *__restrict__ O, const RowPlan p) {
    __shared__ float sm[4];
    const unsigned G = 1u << p.shift, Gu = 1u << p.su, Gr = G >> p.su;
    const unsigned l = threadIdx.x & (G - 1), lu = l & (Gu - 1), lr = l >> p.su;
    const unsigned opb = (unsigned)BLK >> p.shift;
    for (long w = blockIdx.x; w < p.nitem; w += gridDim.x) {
        long og = w; unsigned s = 0;
        if (p.S > 1) divmod(w, p.S, og, s);                                 // uniform over the workgroup
        const long o = og * opb + (threadIdx.x >> p.shift);
        const bool live = o < p.nout;
        float v0 = r_init<OP>(), v1 = r_init<OP>(), v2 = r_init<OP>(), v3 = r_init<OP>();
        if (live) {
            long base;
            if (p.four) { long q; unsigned i; divmod(o, p.k0, q, i); base = q * p.sk1 + (long)i * p.sk0; }
            else base = o * p.sk0;
            const float c = (OP == R_NVAR && Cn) ? Cn[o] : 0.0f;
            long ra = 0, rb = p.r1, ua = 0, ub = p.U;
            if (p.S > 1) {
                if (p.split_u) { ua = (long)s * p.per; ub = min(p.U, ua + p.per); }
                else           { ra = (long)s * p.per; rb = min(p.r1, ra + p.per); }
            }
            const float *xb = X + base;
            if (ub - ua <= (long)Gu) {                                      // short runs: a lane owns one unit of every run it visits
                if (ua + lu < ub) {
                    const long u = ua + lu;
#pragma unroll 4
                    for (long r = ra + lr; r < rb; r += Gr) {
                        if (VEC) {
                            const float4 t = reinterpret_cast<const float4 *>(xb + r * p.sr1)[u];
                            v0 = r_comb<OP>(v0, r_term<OP>(t.x, 0.0f, c)); v1 = r_comb<OP>(v1, r_term<OP>(t.y, 0.0f, c));
                            v2 = r_comb<OP>(v2, r_term<OP>(t.z, 0.0f, c)); v3 = r_comb<OP>(v3, r_term<OP>(t.w, 0.0f, c));
                        } else v0 = r_comb<OP>(v0, r_term<OP>(xb[r * p.sr1 + u], 0.0f, c));
                    }
                }
            } else {
                for (long r = ra + lr; r < rb; r += Gr) {
                    const float *x = xb + r * p.sr1;
#pragma unroll 4
                    for (long u = ua + lu; u < ub; u += Gu) {
                        if (VEC) {
                            const float4 t = reinterpret_cast<const float4 *>(x)[u];
                            v0 = r_comb<OP>(v0, r_term<OP>(t.x, 0.0f, c)); v1 = r_comb<OP>(v1, r_term<OP>(t.y, 0.0f, c));
                            v2 = r_comb<OP>(v2, r_term<OP>(t.z, 0.0f, c)); v3 = r_comb<OP>(v3, r_term<OP>(t.w, 0.0f, c));
                        } else v0 = r_comb<OP>(v0, r_term<OP>(x[u], 0.0f, c));
                    }
                }
            }
        }
        float v = VEC ? r_comb<OP>(r_comb<OP>(v0, v1), r_comb<OP>(v2, v3)) : v0;
        // the lanes of an output: a fixed xor tree inside the wave (an output's lanes are all live or all idle) ...
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const float t = __shfl_xor(v, off, 64); if ((unsigned)off < G) v = r_comb<OP>(v, t); }
        if (p.shift == 8) {                                                 // ... and the four waves of a workgroup-wide output through LDS
            if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
            __syncthreads();
            v = r_comb<OP>(r_comb<OP>(sm[0], sm[1]), r_comb<OP>(sm[2], sm[3]));
            __syncthreads();
        }
        if (live && l == 0) O[p.S > 1 ? o * (long)p.S + s : o] = v;
    }
}

// ---- column family (ColPlan, axes.h).  S > 1: the parts leave partials O[s * nout + o] - a [S, nout] matrix whose column sums a second
// launch of this kernel takes.
template <int OP, bool VEC>
__global__ void __launch_bounds__(BLK) k_red_col(const float *__restrict__ X, const float *__restrict__ Cn, float *__restrict__ O, const ColPlan p) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float sm[4][64 * V];
    const unsigned TX = 1u << p.sx, TY = (unsigned)BLK >> p.sx;
    const unsigned tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> p.sx, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long w = blockIdx.x; w < p.nitem; w += gridDim.x) {
        long t = w; unsigned s = 0, tile = 0;
        if (p.S > 1) divmod(t, p.S, t, s);                                  // uniform over the workgroup
        if (p.ntile > 1) divmod(t, p.ntile, t, tile);
        const long ik1 = t;
        const long col = (((long)tile << p.sx) + tx) * V;
        float a[V], c[V];
#pragma unroll
        for (int q = 0; q < V; q++) { a[q] = r_init<OP>(); c[q] = 0.0f; }
        if (col < p.k0) {
            if (OP == R_NVAR && Cn) {
#pragma unroll
                for (int q = 0; q < V; q++) c[q] = Cn[ik1 * p.k0 + col + q];
            }
            long ra = 0, rb = p.r0, ja = 0, jb = p.r1;
            if (p.S > 1) {
                if (p.split_r1) { ja = (long)s * p.per; jb = min(p.r1, ja + p.per); }
                else            { ra = (long)s * p.per; rb = min(p.r0, ra + p.per); }
            }
            const float *xb = X + ik1 * p.sk1 + col;
            for (long j = ja; j < jb; j++) {
                const float *x = xb + j * p.sr1;
#pragma unroll 4
                for (long r = ra + ty; r < rb; r += TY) {
                    if constexpr (VEC) {
                        const float4 f = *reinterpret_cast<const float4 *>(x + r * p.sr0);
                        a[0] = r_comb<OP>(a[0], r_term<OP>(f.x, 0.0f, c[0])); a[1] = r_comb<OP>(a[1], r_term<OP>(f.y, 0.0f, c[1]));
                        a[2] = r_comb<OP>(a[2], r_term<OP>(f.z, 0.0f, c[2])); a[3] = r_comb<OP>(a[3], r_term<OP>(f.w, 0.0f, c[3]));
                    } else a[0] = r_comb<OP>(a[0], r_term<OP>(x[r * p.sr0], 0.0f, c[0]));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < V; q++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const float f = __shfl_xor(a[q], off, 64); if ((unsigned)off >= TX) a[q] = r_comb<OP>(a[q], f); }
        }
        if (lane < TX) {
#pragma unroll
            for (int q = 0; q < V; q++) sm[wave][lane * V + q] = a[q];
        }
        __syncthreads();
        if (threadIdx.x < TX * V) {
            const long cc = ((long)tile << p.sx) * V + threadIdx.x;
            if (cc < p.k0)
                O[(long)s * p.nout + ik1 * p.k0 + cc] = r_comb<OP>(r_comb<OP>(sm[0][threadIdx.x], sm[1][threadIdx.x]), r_comb<OP>(sm[2][threadIdx.x], sm[3][threadIdx.x]));
        }
        __syncthreads();                                                    // the tile is rewritten by the next iteration
    }
}

// what folds the partials of `op`: the squares are taken already
inline int fold_op(int op) { return op == R_NVAR ? R_SUM : op; }

template <typename PlanT>
void launch(int op, bool vec, const float *X, const float *Cn, float *O, const PlanT &p, hipStream_t hs) {
    const int g = (int)std::min(p.nitem, (long)MAX_WG);
    pick<R_SUM, R_NVAR, R_MAX, R_MIN>(op, [&](auto o) { with_flags([&](auto v) {
        if constexpr (std::is_same<PlanT, ColPlan>::value) T4K_LAUNCH((k_red_col<o.value, v.value>), dim3(g), dim3(BLK), 0, hs, X, Cn, O, p);
        else                                               T4K_LAUNCH((k_red_row<o.value, v.value>), dim3(g), dim3(BLK), 0, hs, X, Cn, O, p);
    }, vec); });
}

// the plan of one launch, for the launcher and for t4k_reduce_axes_plan: one float per part in a workspace of ws_floats, nothing reserved;
// true when the groups are split and a second launch folds the partials
bool plan_row(RowPlan &p, const Merged &m, bool vec, bool may_split, long ws_floats) {
    row_geometry(p, m, vec);
    p.shift = row_lanes(p.U * p.r1, LANE_UNITS, p.nout);
    const bool split = may_split && p.shift == 8 && row_split(p, 1, 0, ws_floats);
    p.su = std::min(p.shift, log2_ceil(split && p.split_u ? p.per : p.U, 8));
    p.nitem = ceil_div(p.nout, BLK >> p.shift) * p.S;
    return split;
}
bool plan_col(ColPlan &p, const Merged &m, bool vec, bool may_split, long ws_floats) {
    col_geometry(p, m, vec);
    return may_split && col_split(p, 1, 0, ws_floats);
}

void launch_row(int op, const float *X, const float *Cn, float *O, const Merged &m, bool may_split, hipStream_t hs) {
    const bool vec = (m.r0 & 3) == 0 && aligned16(X);
    RowPlan p;
    const bool split = plan_row(p, m, vec, may_split, (long)(st().ws_bytes / sizeof(float)));
    float *dst = split ? ws_for(hs) : O;
    launch(op, vec, X, Cn, dst, p, hs);
    if (split) launch_row(fold_op(op), dst, nullptr, O, Merged{false, false, (long)p.S, p.nout, 1, 1}, false, hs);   // a row of S partials per output
}

void launch_col(int op, const float *X, const float *Cn, float *O, const Merged &m, bool may_split, hipStream_t hs) {
    const bool vec = (m.k0 & 3) == 0 && aligned16(X);
    ColPlan p;
    const bool split = plan_col(p, m, vec, may_split, (long)(st().ws_bytes / sizeof(float)));
    float *dst = split ? ws_for(hs) : O;
    launch(op, vec, X, Cn, dst, p, hs);
    if (split) launch_col(fold_op(op), dst, nullptr, O, Merged{true, false, (long)p.S, p.nout, 1, 1}, false, hs);   // column sums of the [S, nout] partials
}

} // namespace

extern "C" {

int t4k_reduce_axes(int red_op, const float *src, float *dst, const int dim[4], int mask, const float *center, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!src || !dst) return fail(T4K_ERR_ARG, "t4k_reduce_axes: null");
    long total; Merged m;
    int rc = check_axes(dim, mask, "t4k_reduce_axes", &total); if (rc != T4K_OK) return rc;
    if (red_op != T4K_RED_SUM && red_op != T4K_RED_NVAR && red_op != T4K_RED_MAX && red_op != T4K_RED_MIN) return fail(T4K_ERR_ARG, "t4k_reduce_axes: op %d", red_op);
    long nout = 1;
    for (int i = 0; i < 4; i++) if (!(mask & (8 >> i))) nout *= dim[i];
    if (src < dst + nout && dst < src + total) return fail(T4K_ERR_ARG, "t4k_reduce_axes: dst overlaps src");
    rc = merge_axes(dim, mask, "t4k_reduce_axes", m); if (rc != T4K_OK) return rc;
    const int op = red_op == T4K_RED_SUM ? R_SUM : red_op == T4K_RED_NVAR ? R_NVAR : red_op == T4K_RED_MAX ? R_MAX : R_MIN;
    const float *cn = op == R_NVAR ? center : nullptr;
    if (m.col) launch_col(op, src, cn, dst, m, true, S(s));
    else       launch_row(op, src, cn, dst, m, true, S(s));
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

int t4k_reduce_axes_plan(const int dim[4], int mask, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_reduce_axes_plan: null");
    long total, ws_floats; Merged m;
    int rc = check_axes(dim, mask, "t4k_reduce_axes_plan", &total); if (rc != T4K_OK) return rc;
    rc = plan_workspace(ws_bytes, "t4k_reduce_axes_plan", &ws_floats); if (rc != T4K_OK) return rc;
    rc = merge_axes(dim, mask, "t4k_reduce_axes_plan", m); if (rc != T4K_OK) return rc;
    const bool vec = aligned != 0 && ((m.col ? m.k0 : m.r0) & 3) == 0;
    if (m.col) { ColPlan p; const bool split = plan_col(p, m, vec, true, ws_floats); report_plan(out, p, vec, split ? 2 : 1); }
    else       { RowPlan p; const bool split = plan_row(p, m, vec, true, ws_floats); report_plan(out, p, vec, split ? 2 : 1); }
    return T4K_OK;
}

} // extern "C"
