// reduce_axes.hip - sum / n*var / max / min along any subset of the axes of a dense NHWC tensor, keepdims layout.
// Deterministic like reduce.hip: fixed trees, no floating-point atomics, the same bits on every run.  No reference definition: the
// reference's k_sum / k_nvar / k_max (src/t4math.cu:23-131) fold a whole tensor into one scalar, and its only axis reductions are
// welded to nn layers (k_dlinear_db nmath.cu:274, k_batchnorm_1 :177, the softmax row sum forward.cu:222-243).
#include "t4k_common.h"
#include <float.h>

using namespace t4k;

namespace {

enum { R_SUM = 0, R_NVAR, R_MAX, R_MIN };

// the arithmetic of reduce.hip's r_init / r_comb / r_term, restated (NVAR subtracts the output's own centre)
template <int OP> __device__ __forceinline__ float r_init() {
    return OP == R_MAX ? -FLT_MAX : (OP == R_MIN ? FLT_MAX : 0.0f);
}
template <int OP> __device__ __forceinline__ float r_comb(float a, float b) {
    return OP == R_MAX ? fmaxf(a, b) : (OP == R_MIN ? fminf(a, b) : a + b);
}
template <int OP> __device__ __forceinline__ float r_term(float x, float c) {
    if (OP == R_NVAR) { float d = x - c; return d * d; }
    return x;
}

// x = q * d + rem; the 32-bit divide whenever x fits.  Used once per workgroup iteration or once per output, never per element.
__device__ __forceinline__ void divmod(long x, unsigned d, long &q, unsigned &rem) {
    if (x < 0xffffffffL) { const unsigned v = (unsigned)x, t = v / d; rem = v - t * d; q = (long)t; }
    else { const long t = x / (long)d; rem = (unsigned)(x - t * (long)d); q = t; }
}

constexpr long TARGET_LANES = 64L * 4 * 256 * 2;   // two waves on every SIMD of 256 CUs: below this an output gets more lanes
constexpr long TARGET_ITEMS = 1024;                // workgroups a split aims for: four on every CU
constexpr long LANE_UNITS   = 16;                  // loads a lane should have before an output gets more lanes
constexpr long SPLIT_UNITS  = 8;                   // loads a lane keeps at least when a reduction is split across workgroups
constexpr long MAX_SPLIT    = 4096;

// ---- row family: the innermost merged group is reduced.  Output o folds r1 runs (sr1 apart) of r0 contiguous floats starting at
// base(o) = o * sk0, or (o / k0) * sk1 + (o % k0) * sk0 when a second kept group lies outside the runs.  1 << shift lanes share an
// output (shift 0..5: several outputs per wave, 6: a wave per output, 8: a workgroup per output), 1 << su of them side by side along
// a run and the rest over the runs.  S > 1: the units of a run (split_u) or the runs are dealt to S workgroups of `per` each, which
// leave partials O[o * S + s] for a second launch of this kernel (a row of S partials per output).
struct RowPlan {
    long nout, U, r1;             // outputs, units per run (r0 / 4 float4s on the vector path, else r0), runs per output
    long sk0, sr1, sk1, per, nitem;
    unsigned k0, shift, su, S;
    int four, split_u;
};

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
                            v0 = r_comb<OP>(v0, r_term<OP>(t.x, c)); v1 = r_comb<OP>(v1, r_term<OP>(t.y, c));
                            v2 = r_comb<OP>(v2, r_term<OP>(t.z, c)); v3 = r_comb<OP>(v3, r_term<OP>(t.w, c));
                        } else v0 = r_comb<OP>(v0, r_term<OP>(xb[r * p.sr1 + u], c));
                    }
                }
            } else {
                for (long r = ra + lr; r < rb; r += Gr) {
                    const float *x = xb + r * p.sr1;
#pragma unroll 4
                    for (long u = ua + lu; u < ub; u += Gu) {
                        if (VEC) {
                            const float4 t = reinterpret_cast<const float4 *>(x)[u];
                            v0 = r_comb<OP>(v0, r_term<OP>(t.x, c)); v1 = r_comb<OP>(v1, r_term<OP>(t.y, c));
                            v2 = r_comb<OP>(v2, r_term<OP>(t.z, c)); v3 = r_comb<OP>(v3, r_term<OP>(t.w, c));
                        } else v0 = r_comb<OP>(v0, r_term<OP>(x[u], c));
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

// ---- column family: the innermost merged group (k0 floats) is kept.  A workgroup iteration takes one tile of TX = 1 << sx lanes
// along k0 (one column a lane, four on the vector path: every load of a wave is a contiguous run, also for k0 = 3 or 64) of one outer
// kept index; its 256 >> sx row groups deal the reduced rows (r0 of them sr0 apart, inside r1 of them sr1 apart) among themselves.
// Row groups fold inside the wave by xor shuffles over the lane bits above sx, the four waves through LDS.  S > 1: the rows (or the
// outer reduced extent, split_r1) are dealt to S workgroups leaving partials O[s * nout + o] - a [S, nout] matrix whose column sums
// a second launch of this kernel takes.
struct ColPlan {
    long k0, r0, r1, sr0, sk1, sr1, per, nitem, nout;
    unsigned sx, ntile, S;
    int split_r1;
};

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
                        a[0] = r_comb<OP>(a[0], r_term<OP>(f.x, c[0])); a[1] = r_comb<OP>(a[1], r_term<OP>(f.y, c[1]));
                        a[2] = r_comb<OP>(a[2], r_term<OP>(f.z, c[2])); a[3] = r_comb<OP>(a[3], r_term<OP>(f.w, c[3]));
                    } else a[0] = r_comb<OP>(a[0], r_term<OP>(x[r * p.sr0], c[0]));
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

inline unsigned log2_ceil(long x, unsigned cap) { unsigned k = 0; while (k < cap && (1L << k) < x) k++; return k; }
inline long ceil_div(long a, long b) { return (a + b - 1) / b; }
// how many workgroups share one reduction: enough for TARGET_ITEMS, never leaving a lane fewer than SPLIT_UNITS loads, never more
// partials than the stream's workspace holds
inline long split_for(long items, long max_by_work, long nout) {
    long S = std::min(std::min(ceil_div(TARGET_ITEMS, items), max_by_work), MAX_SPLIT);
    S = std::min(S, (long)(st().ws_bytes / sizeof(float)) / nout);
    return S < 2 ? 1 : S;
}

#define RA_LAUNCH(K, OPV, ...) do { if (vec) T4K_LAUNCH((K<OPV, true>), __VA_ARGS__); else T4K_LAUNCH((K<OPV, false>), __VA_ARGS__); } while (0)
#define RA_SWITCH(K, ...) switch (op) { \
    case R_SUM:  RA_LAUNCH(K, R_SUM, __VA_ARGS__); break; case R_NVAR: RA_LAUNCH(K, R_NVAR, __VA_ARGS__); break; \
    case R_MAX:  RA_LAUNCH(K, R_MAX, __VA_ARGS__); break; default:     RA_LAUNCH(K, R_MIN, __VA_ARGS__); break; }

// what folds the partials of `op`: the squares are taken already
inline int fold_op(int op) { return op == R_NVAR ? R_SUM : op; }

void launch_row(int op, const float *X, const float *Cn, float *O, long nout, long r0, long r1, long k0, bool four, bool may_split, hipStream_t hs) {
    const bool vec = (r0 & 3) == 0 && aligned16(X);                          // every run starts on a multiple of r0 elements
    RowPlan p = {};
    p.nout = nout; p.U = vec ? r0 >> 2 : r0; p.r1 = r1; p.k0 = (unsigned)k0; p.four = four;
    p.sk0 = r0; p.sr1 = r0 * k0; p.sk1 = r0 * k0 * r1;
    const long T = p.U * r1;                                                 // loads behind one output
    p.shift = log2_ceil(ceil_div(T, LANE_UNITS), 8);
    const unsigned cap = log2_ceil(T, 8);
    while (p.shift < cap && (nout << p.shift) < TARGET_LANES) p.shift++;
    if (p.shift == 7) p.shift = (nout << 6) >= TARGET_LANES ? 6 : 8;         // a wave or a workgroup: nothing between
    p.S = 1; p.split_u = 0; p.per = 0;
    long ext_u = p.U;
    if (may_split && p.shift == 8) {
        const long S = split_for(nout, T / (BLK * SPLIT_UNITS), nout);
        if (S > 1) {
            p.split_u = p.U >= r1;
            const long ext = p.split_u ? p.U : r1;
            p.per = ceil_div(ext, S); p.S = (unsigned)ceil_div(ext, p.per);
            if (p.split_u) ext_u = p.per;
        }
    }
    p.su = std::min(p.shift, log2_ceil(ext_u, 8));
    const long opb = BLK >> p.shift;
    p.nitem = ceil_div(nout, opb) * p.S;
    const int g = (int)std::min(p.nitem, (long)MAX_WG);
    float *dst = p.S > 1 ? ws_for(hs) : O;
    RA_SWITCH(k_red_row, dim3(g), dim3(BLK), 0, hs, X, Cn, dst, p);
    if (p.S > 1) launch_row(fold_op(op), dst, nullptr, O, nout, p.S, 1, nout, false, false, hs);   // a row of S partials per output
}

void launch_col(int op, const float *X, const float *Cn, float *O, long k0, long r0, long k1, long r1, bool may_split, hipStream_t hs) {
    const bool vec = (k0 & 3) == 0 && aligned16(X);                          // every row starts on a multiple of k0 elements
    ColPlan p = {};
    p.k0 = k0; p.r0 = r0; p.r1 = r1; p.sr0 = k0; p.sk1 = k0 * r0; p.sr1 = k0 * r0 * k1; p.nout = k0 * k1;
    const long Uk = vec ? k0 >> 2 : k0;
    p.sx = log2_ceil(Uk, 6);
    const long TY = BLK >> p.sx;
    p.ntile = (unsigned)ceil_div(Uk, 1L << p.sx);
    const long items = k1 * p.ntile;
    p.S = 1; p.split_r1 = 0; p.per = 0;
    if (may_split && items < TARGET_ITEMS) {
        const bool by_r1 = r1 > r0;
        const long S = split_for(items, by_r1 ? r1 / 4 : r0 / (TY * SPLIT_UNITS), p.nout);
        if (S > 1) {
            p.split_r1 = by_r1;
            const long ext = by_r1 ? r1 : r0;
            p.per = ceil_div(ext, S); p.S = (unsigned)ceil_div(ext, p.per);
        }
    }
    p.nitem = items * p.S;
    const int g = (int)std::min(p.nitem, (long)MAX_WG);
    float *dst = p.S > 1 ? ws_for(hs) : O;
    RA_SWITCH(k_red_col, dim3(g), dim3(BLK), 0, hs, X, Cn, dst, p);
    if (p.S > 1) launch_col(fold_op(op), dst, nullptr, O, p.nout, p.S, 1, 1, false, hs);            // column sums of the [S, nout] partials
}

} // namespace

extern "C" {

int t4k_reduce_axes(int red_op, const float *src, float *dst, const int dim[4], int mask, const float *center, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!src || !dst || !dim) return fail(T4K_ERR_ARG, "t4k_reduce_axes: null");
    if (mask < 1 || mask > 15) return fail(T4K_ERR_ARG, "t4k_reduce_axes: mask %d outside 1..15", mask);
    if (red_op != T4K_RED_SUM && red_op != T4K_RED_NVAR && red_op != T4K_RED_MAX && red_op != T4K_RED_MIN) return fail(T4K_ERR_ARG, "t4k_reduce_axes: op %d", red_op);
    long total = 1, nout = 1;
    for (int i = 0; i < 4; i++) {
        if (dim[i] < 1) return fail(T4K_ERR_ARG, "t4k_reduce_axes: extent %d", dim[i]);
        if (total > (1L << 40) / dim[i]) return fail(T4K_ERR_ARG, "t4k_reduce_axes: more than 2^40 elements");
        total *= dim[i];
        if (!(mask & (8 >> i))) nout *= dim[i];
    }
    if (src < dst + nout && dst < src + total) return fail(T4K_ERR_ARG, "t4k_reduce_axes: dst overlaps src");
    // axes of extent 1 drop out, neighbours that are both kept or both reduced merge: at most four alternating groups
    long e[5]; bool red[5]; int n = 0; bool any = false;
    for (int i = 0; i < 4; i++) {
        if (dim[i] == 1) continue;
        const bool r = (mask & (8 >> i)) != 0;
        any = any || r;
        if (n && red[n - 1] == r) e[n - 1] *= dim[i];
        else { e[n] = dim[i]; red[n] = r; n++; }
    }
    if (!any) { e[n] = 1; red[n] = true; n++; }                              // only axes of extent 1 are masked: every element is its own output
    const int op = red_op == T4K_RED_SUM ? R_SUM : red_op == T4K_RED_NVAR ? R_NVAR : red_op == T4K_RED_MAX ? R_MAX : R_MIN;
    const float *cn = op == R_NVAR ? center : nullptr;
    if (red[n - 1]) {
        const long r0 = e[n - 1], k0 = n >= 2 ? e[n - 2] : 1, r1 = n >= 3 ? e[n - 3] : 1, k1 = n >= 4 ? e[n - 4] : 1;
        if (k0 > 0xffffffffL) return fail(T4K_ERR_ARG, "t4k_reduce_axes: merged extent too large");
        launch_row(op, src, cn, dst, k0 * k1, r0, r1, k0, n == 4, true, S(s));
    } else {
        const long k0 = e[n - 1], r0 = e[n - 2], k1 = n >= 3 ? e[n - 3] : 1, r1 = n >= 4 ? e[n - 4] : 1;
        launch_col(op, src, cn, dst, k0, r0, k1, r1, true, S(s));
    }
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

} // extern "C"
