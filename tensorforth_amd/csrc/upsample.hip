// upsample.hip - up-sampling by any integer factor K 1..16 for NHWC fp32 tensors: nearest, (bi)linear and bicubic, forward and backward.
// Beyond the reference, whose _iup (model.cpp:294-310) admits 2x2 and 3x3, whose forward and backward (`///< upsample method, TODO` forward.cu:318,
// backprop.cu:289) run k_dpool / k_pool whatever the method, and whose enum UP_NEAREST .. UP_CUBIC (ntypes.h:53-58) no kernel reads.
// The map is separable and the same on both axes: output row i = q K + r reads T taps at input rows clamp(q + base[r] + a, 0, H1 - 1), a = 0 .. T - 1, with
// weights wt[r][a]; base and wt depend on the method, K and the phase r only.  The HOST works that table out once per call (up_table below) and the kernels
// take it as an argument: they evaluate no polynomial and divide nothing per tap.  The backward is the transpose, a GATHER: a thread owns input cells, walks
// the output rows and columns that read them in ascending order and stores every dX element exactly once - no atomics, no read of the forward input.
#include "t4k_common.h"
#include "launch.h"
#include "fastdiv.h"

using namespace t4k;

namespace {

struct UpP {
    int N, H1, W1, C, H0, W0, K;
    int CV;                            // channel groups of a pixel: C / VW
    long total;                        // work items: pixels * CV
    FastDiv dCV, dW, dH, dK;           // by CV, by the width and height of the grid the work items run over (outputs forward, inputs backward), by K
    int base[16];                      // base[r]: the first tap of phase r, relative to q
    float wt[64];                      // wt[r * 4 + a]: the weight of tap a of phase r; unused cells 0
};

template <int VW> __device__ __forceinline__ float4 up_ld(const float *q) {
    if constexpr (VW == 4) return *reinterpret_cast<const float4 *>(q);
    else return make_float4(*q, 0.f, 0.f, 0.f);
}
template <int VW> __device__ __forceinline__ void up_st(float *q, const float4 &v) {
    if constexpr (VW == 4) *reinterpret_cast<float4 *>(q) = v;
    else *q = v.x;
}
template <int VW> __device__ __forceinline__ void up_fma(float4 &a, float w, const float4 &d) {
    a.x += w * d.x;
    if constexpr (VW == 4) { a.y += w * d.y; a.z += w * d.z; a.w += w * d.w; }
}

// ------------------------------------------------------------------ forward: a thread owns (output pixel, VW channels)
// Lanes that neighbour in (c, j) store neighbouring addresses: the channel group is the fastest digit of the work item, the output column the next.  The T
// row and T column indices are clamped once, the T x T loads are issued together, the sum runs in ascending (a, b) order.  T = 1 is a copy.
template <int T, int VW>
__global__ void __launch_bounds__(BLK) k_up_fwd(const float *__restrict__ I, float *__restrict__ O, UpP p) {
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < p.total; z += (long)gridDim.x * BLK) {
        int cv, j, i, n; long pix; fd_digits(z, p.CV, p.W0, p.H0, p.dCV, p.dW, p.dH, cv, j, i, n, pix);
        const int qi = (int)fdiv((unsigned)i, p.dK), qj = (int)fdiv((unsigned)j, p.dK);
        const int c = cv * VW;
        const float *img = I + (long)n * p.H1 * p.W1 * p.C + c;
        if constexpr (T == 1) {
            up_st<VW>(O + pix * p.C + c, up_ld<VW>(img + ((long)qi * p.W1 + qj) * p.C));
        } else {
            const int ri = i - qi * p.K, rj = j - qj * p.K;
            const int bi = qi + p.base[ri], bj = qj + p.base[rj];
            long row[T], col[T]; float wy[T], wx[T];
#pragma unroll
            for (int a = 0; a < T; a++) {
                row[a] = (long)min(max(bi + a, 0), p.H1 - 1) * p.W1 * p.C; wy[a] = p.wt[ri * 4 + a];
                col[a] = (long)min(max(bj + a, 0), p.W1 - 1) * p.C;        wx[a] = p.wt[rj * 4 + a];
            }
            float4 e[T][T];
#pragma unroll
            for (int a = 0; a < T; a++)
#pragma unroll
                for (int b = 0; b < T; b++) e[a][b] = up_ld<VW>(img + row[a] + col[b]);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int a = 0; a < T; a++)
#pragma unroll
                for (int b = 0; b < T; b++) up_fma<VW>(v, wy[a] * wx[b], e[a][b]);
            up_st<VW>(O + pix * p.C + c, v);
        }
    }
}

// ------------------------------------------------------------------ backward: a thread owns (input pixel, VW channels)
// Output row (q, r) reads input row y through the taps a with clamp(q + base[r] + a) == y: the one tap a0 = y - q - base[r] and, where y is the first
// (last) row, every tap below (above) it, which the clamp folded onto y.  Only q in [y - T/2, y + T/2] can: |base[r] + a| <= T/2.  A row's weight is the sum
// of its taps' weights in ascending a - worked out once per row; a column's is re-selected for each row, T compares, because the up to 3 K column weights
// of a thread indexed by a run-time K would have to live in scratch memory.  Rows and columns that read nothing of the cell are skipped: in the interior
// that is decided by (q - y, r) alone, the same for a whole wave.
template <int T>
__device__ __forceinline__ bool up_taps(const UpP &p, int r, int dq, bool first, bool last, float &w) {
    if constexpr (T == 1) { w = 1.0f; return true; }
    const int a0 = -dq - p.base[r];
    bool hit = false; w = 0.0f;
#pragma unroll
    for (int a = 0; a < T; a++) {
        const bool sel = a == a0 || (first && a < a0) || (last && a > a0);
        w += sel ? p.wt[r * 4 + a] : 0.0f; hit |= sel;
    }
    return hit;
}

template <int T, int VW>
__global__ void __launch_bounds__(BLK) k_up_bwd(const float *__restrict__ DY, float *__restrict__ DX, UpP p) {
    constexpr int R = T / 2;
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < p.total; z += (long)gridDim.x * BLK) {
        int cv, x, y, n; long pix; fd_digits(z, p.CV, p.W1, p.H1, p.dCV, p.dW, p.dH, cv, x, y, n, pix);
        const bool top = y == 0, bot = y == p.H1 - 1, lef = x == 0, rig = x == p.W1 - 1;
        const int c = cv * VW;
        const float *img = DY + (long)n * p.H0 * p.W0 * p.C + c;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
        for (int dy = -R; dy <= R; dy++) {
            const int qy = y + dy; if (qy < 0 || qy >= p.H1) continue;
#pragma unroll 1
            for (int ry = 0; ry < p.K; ry++) {
                float wy; if (!up_taps<T>(p, ry, dy, top, bot, wy)) continue;
                const float *row = img + (long)(qy * p.K + ry) * p.W0 * p.C;
#pragma unroll 1
                for (int dx = -R; dx <= R; dx++) {
                    const int qx = x + dx; if (qx < 0 || qx >= p.W1) continue;
                    const float *q = row + (long)qx * p.K * p.C;
                    for (int rx = 0; rx < p.K; rx++, q += p.C) {
                        float wx; if (!up_taps<T>(p, rx, dx, lef, rig, wx)) continue;
                        const float4 d = up_ld<VW>(q);
                        if constexpr (T == 1) { acc.x += d.x; if (VW == 4) { acc.y += d.y; acc.z += d.z; acc.w += d.w; } }
                        else up_fma<VW>(acc, wy * wx, d);
                    }
                }
            }
        }
        up_st<VW>(DX + pix * p.C + c, acc);
    }
}

// ------------------------------------------------------------------ the plan and the table: what the launch code uses, and what t4k_upsample_plan reports
struct UpPlan { int H0, W0, vw_fwd, vw_bwd; };
int up_taps_of(int method) { return method == T4K_UP_NEAREST ? 1 : (method == T4K_UP_CUBIC ? 4 : 2); }
// admission (who: the entry's name for the message).  T4K_ERR_ARG: an extent below 1; T4K_ERR_UNSUPPORTED: a method, factor or size outside the admitted set
int up_plan(UpPlan &g, const char *who, int method, int N, int H1, int W1, int C, int K, bool al_fwd, bool al_bwd) {
    if (method < T4K_UP_NEAREST || method > T4K_UP_CUBIC) return fail(T4K_ERR_UNSUPPORTED, "%s: method %d not supported (0 nearest, 1 linear, 2 bilinear, 3 cubic)", who, method);
    if (N < 1 || H1 < 1 || W1 < 1 || C < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (N=%d H1=%d W1=%d C=%d)", who, N, H1, W1, C);
    const int kmax = method == T4K_UP_CUBIC ? 8 : 16;
    if (K < 1 || K > kmax) return fail(T4K_ERR_UNSUPPORTED, "%s: size=%d method=%d not supported (K 1..%d)", who, K, method, kmax);
    const long h0 = (long)K * H1, w0 = (long)K * W1, lim = 1L << 31;
    if (h0 >= lim || w0 >= lim || (long)N * h0 >= lim || (long)N * h0 * w0 >= lim) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 pixels or more", who);
    g.H0 = (int)h0; g.W0 = (int)w0;
    g.vw_fwd = (al_fwd && C % 4 == 0) ? 4 : 1;
    g.vw_bwd = (al_bwd && C % 4 == 0) ? 4 : 1;
    return T4K_OK;
}
// the table of an admitted (method, K): lambda as a rational over 2 K, the cubic-convolution polynomials (A = -0.75, torch's bicubic) in double, each weight
// rounded once to float
void up_table(int method, int K, float wt[64], int base[16]) {
    for (int k = 0; k < 64; k++) wt[k] = 0.0f;
    for (int k = 0; k < 16; k++) base[k] = 0;
    for (int r = 0; r < K; r++) {
        float *w = wt + r * 4;
        if (method == T4K_UP_NEAREST) { w[0] = 1.0f; continue; }
        const int u = 2 * r + 1 - K, num = u >= 0 ? u : u + 2 * K, b = u >= 0 ? 0 : -1;          // the source row is q + b + num / 2K
        const double den = 2.0 * K, l = num / den;
        if (method != T4K_UP_CUBIC) { base[r] = b; w[0] = (float)((2 * K - num) / den); w[1] = (float)l; continue; }
        const double A = -0.75;
        auto c1 = [A](double t) { return ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0; };
        auto c2 = [A](double t) { return ((A * t - 5.0 * A) * t + 8.0 * A) * t - 4.0 * A; };
        base[r] = b - 1;
        w[0] = (float)c2(l + 1.0); w[1] = (float)c1(l); w[2] = (float)c1(1.0 - l); w[3] = (float)c2(2.0 - l);
    }
}

UpP up_parms(int method, int N, int H1, int W1, int C, int H0, int W0, int K, int vw, bool fwd) {
    UpP p;
    p.N = N; p.H1 = H1; p.W1 = W1; p.C = C; p.H0 = H0; p.W0 = W0; p.K = K; p.CV = C / vw;
    p.total = (long)N * (fwd ? (long)H0 * W0 : (long)H1 * W1) * p.CV;
    p.dCV = fast_div(p.CV); p.dW = fast_div(fwd ? W0 : W1); p.dH = fast_div(fwd ? H0 : H1); p.dK = fast_div(K);
    up_table(method, K, p.wt, p.base);
    return p;
}

} // namespace

extern "C" {

int t4k_upsample_plan(int method, int N, int H1, int W1, int C, int K, int aligned, int out[4], float wt[64], int base[16]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_upsample_plan: null");
    UpPlan g;
    const int rc = up_plan(g, "t4k_upsample_plan", method, N, H1, W1, C, K, (aligned & 1) != 0, (aligned & 2) != 0); if (rc != T4K_OK) return rc;
    out[0] = g.H0; out[1] = g.W0; out[2] = g.vw_fwd; out[3] = g.vw_bwd;
    if (wt || base) {
        float w[64]; int b[16]; up_table(method, K, w, b);
        if (wt) for (int k = 0; k < 64; k++) wt[k] = w[k];
        if (base) for (int k = 0; k < 16; k++) base[k] = b[k];
    }
    return T4K_OK;
}

int t4k_upsample_fwd(int method, const float *I, float *O, int N, int H1, int W1, int C, int H0, int W0, int K, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!I || !O) return fail(T4K_ERR_ARG, "t4k_upsample_fwd: null tensor");
    UpPlan g;
    const int rc = up_plan(g, "t4k_upsample_fwd", method, N, H1, W1, C, K, aligned16(I) && aligned16(O), false); if (rc != T4K_OK) return rc;
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_upsample_fwd: output %dx%d, the factor gives %dx%d", H0, W0, g.H0, g.W0);
    const UpP p = up_parms(method, N, H1, W1, C, H0, W0, K, g.vw_fwd, true);
    hipStream_t hs = t4k::S(s);
    pick<1, 2, 4>(up_taps_of(method), [&](auto t) { pick<4, 1>(g.vw_fwd, [&](auto vw) {
        T4K_LAUNCH((k_up_fwd<decltype(t)::value, decltype(vw)::value>), dim3(grid_for(p.total)), dim3(BLK), 0, hs, I, O, p); }); });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_upsample_bwd(int method, const float *DY, float *DX, int N, int H1, int W1, int C, int H0, int W0, int K, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!DY || !DX) return fail(T4K_ERR_ARG, "t4k_upsample_bwd: null tensor");
    UpPlan g;
    const int rc = up_plan(g, "t4k_upsample_bwd", method, N, H1, W1, C, K, false, aligned16(DY) && aligned16(DX)); if (rc != T4K_OK) return rc;
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_upsample_bwd: output %dx%d, the factor gives %dx%d", H0, W0, g.H0, g.W0);
    const UpP p = up_parms(method, N, H1, W1, C, H0, W0, K, g.vw_bwd, false);
    hipStream_t hs = t4k::S(s);
    pick<1, 2, 4>(up_taps_of(method), [&](auto t) { pick<4, 1>(g.vw_bwd, [&](auto vw) {
        T4K_LAUNCH((k_up_bwd<decltype(t)::value, decltype(vw)::value>), dim3(grid_for(p.total)), dim3(BLK), 0, hs, DY, DX, p); }); });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
