// pool_geo.hip - avg / max / min pooling with RUN-TIME geometry for NHWC fp32 tensors: any K 1..16, stride 1..16, padding 0..K/2.
// Beyond the reference, whose k_pool / k_dpool (src/nn/nmath.tcu:400-568) and Model::_ipool (model.cpp:261-274) know window = stride in {2, 3} only.
// The forward stores, beside O, the winning tap ky*K + kx of every max / min output as one byte; the backward is a GATHER over those bytes - a thread owns
// input cells and walks the windows that cover them in ascending order - so windows may overlap, nothing is atomic, every dX element is stored exactly
// once (zeros included) and the forward input is never read: dX may land in its buffer.
#include "t4k_common.h"
#include "launch.h"
#include "fastdiv.h"

using namespace t4k;

namespace {

enum { PG_AVG = 0, PG_MAX = 1, PG_MIN = 2 };

struct PoolGeoP {
    int N, H1, W1, C, H0, W0, K, S, P;
    int CV;                            // channel groups of a pixel: C / VW
    int pitch;                         // bytes of a pixel's codes: 4 * ceil(C / 4)
    long total;                        // work items: pixels * CV
    FastDiv dCV, dW, dH, dS;           // by CV, by the width and height of the grid the work items run over (outputs forward, inputs backward), by S
};
__device__ __forceinline__ void pg_digits(long z, const PoolGeoP &p, int W, int H, int &cv, int &j, int &i, int &n, long &pix) {
    fd_digits(z, p.CV, W, H, p.dCV, p.dW, p.dH, cv, j, i, n, pix);
}

template <int KIND> __device__ __forceinline__ bool pg_better(float e, float best) { return KIND == PG_MAX ? e > best : e < best; }   // strict: the first extreme wins
template <int KIND> __device__ __forceinline__ float pg_start() { return KIND == PG_MAX ? -INFINITY : (KIND == PG_MIN ? INFINITY : 0.0f); }

// ------------------------------------------------------------------ forward: a thread owns (output pixel, VW channels)
// Lanes that neighbour in (c, j) read neighbouring addresses: the channel group is the fastest digit of the work item, the output column the next.
template <int KIND, int VW>
__global__ void __launch_bounds__(BLK) k_pool_geo_fwd(const float *__restrict__ I, float *__restrict__ O, unsigned char *__restrict__ CODE, PoolGeoP p) {
    const float kk = (float)(p.K * p.K);
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < p.total; z += (long)gridDim.x * BLK) {
        int cv, j, i, n; long pix; pg_digits(z, p, p.W0, p.H0, cv, j, i, n, pix);
        // the taps inside the image, worked out once: rows ky0 .. ky1 - 1, columns kx0 .. kx1 - 1 (never empty: P <= K / 2 and the floor grid)
        const int y0 = i * p.S - p.P, x0 = j * p.S - p.P;
        const int ky0 = y0 < 0 ? -y0 : 0, ky1 = min(p.K, p.H1 - y0);
        const int kx0 = x0 < 0 ? -x0 : 0, kx1 = min(p.K, p.W1 - x0);
        const int c = cv * VW;
        const float *row = I + (((long)n * p.H1 + (y0 + ky0)) * p.W1 + (x0 + kx0)) * p.C + c;
        const long rstep = (long)p.W1 * p.C;
        const int first = ky0 * p.K + kx0;
        if constexpr (VW == 4) {
            float4 v = make_float4(pg_start<KIND>(), pg_start<KIND>(), pg_start<KIND>(), pg_start<KIND>());
            unsigned t0 = first, t1 = first, t2 = first, t3 = first;
            for (int ky = ky0; ky < ky1; ky++, row += rstep) {
                const float *q = row;
#pragma unroll 4
                for (int kx = kx0; kx < kx1; kx++, q += p.C) {
                    const float4 e = *reinterpret_cast<const float4 *>(q);
                    if constexpr (KIND == PG_AVG) { v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w; }
                    else {
                        const unsigned tap = ky * p.K + kx;
                        if (pg_better<KIND>(e.x, v.x)) { v.x = e.x; t0 = tap; }
                        if (pg_better<KIND>(e.y, v.y)) { v.y = e.y; t1 = tap; }
                        if (pg_better<KIND>(e.z, v.z)) { v.z = e.z; t2 = tap; }
                        if (pg_better<KIND>(e.w, v.w)) { v.w = e.w; t3 = tap; }
                    }
                }
            }
            if constexpr (KIND == PG_AVG) { v.x /= kk; v.y /= kk; v.z /= kk; v.w /= kk; }       // the divisor is always K * K: padding counts as zeros
            *reinterpret_cast<float4 *>(O + pix * p.C + c) = v;
            if (KIND != PG_AVG && CODE) *reinterpret_cast<unsigned *>(CODE + pix * p.pitch + c) = t0 | (t1 << 8) | (t2 << 16) | (t3 << 24);
        } else {
            float v = pg_start<KIND>(); unsigned t0 = first;
            for (int ky = ky0; ky < ky1; ky++, row += rstep) {
                const float *q = row;
#pragma unroll 4
                for (int kx = kx0; kx < kx1; kx++, q += p.C) {
                    const float e = *q;
                    if constexpr (KIND == PG_AVG) v += e;
                    else if (pg_better<KIND>(e, v)) { v = e; t0 = ky * p.K + kx; }
                }
            }
            if constexpr (KIND == PG_AVG) v /= kk;
            O[pix * p.C + c] = v;
            if (KIND != PG_AVG && CODE) {
                unsigned char *cd = CODE + pix * p.pitch;
                cd[c] = (unsigned char)t0;
                if (c == p.C - 1) for (int k = p.C; k < p.pitch; k++) cd[k] = 0;               // the pad bytes of the pixel
            }
        }
    }
}

// ------------------------------------------------------------------ backward: a thread owns (input pixel, VW channels)
// The windows that cover input row y are i in [ceil((y + P - K + 1) / S), floor((y + P) / S)] within [0, H0), columns likewise: at most ceil(K / S)^2
// of them, summed in ascending (i, j) order.  A cell no window covers (S > K, rows / columns behind the last window) gets its 0 stored.
template <int KIND, int VW>
__global__ void __launch_bounds__(BLK) k_pool_geo_bwd(const unsigned char *__restrict__ CODE, const float *__restrict__ DY, float *__restrict__ DX, PoolGeoP p) {
    const float kk = (float)(p.K * p.K);
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < p.total; z += (long)gridDim.x * BLK) {
        int cv, x, y, n; long pix; pg_digits(z, p, p.W1, p.H1, cv, x, y, n, pix);
        const unsigned S = (unsigned)p.S;
        const int ty = y + p.P - p.K + 1, tx = x + p.P - p.K + 1;
        const int i0 = ty > 0 ? (int)fdiv((unsigned)ty + S - 1, p.dS) : 0, i1 = min((int)fdiv((unsigned)(y + p.P), p.dS), p.H0 - 1);
        const int j0 = tx > 0 ? (int)fdiv((unsigned)tx + S - 1, p.dS) : 0, j1 = min((int)fdiv((unsigned)(x + p.P), p.dS), p.W0 - 1);
        const int c = cv * VW;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = i0; i <= i1; i++) {
            const int ky = y + p.P - i * p.S;
            long opix = ((long)n * p.H0 + i) * p.W0 + j0;
            for (int j = j0; j <= j1; j++, opix++) {
                const unsigned tap = (unsigned)(ky * p.K + (x + p.P - j * p.S));           // this cell's tap in window (i, j)
                if constexpr (VW == 4) {
                    const float4 d = *reinterpret_cast<const float4 *>(DY + opix * p.C + c);
                    if constexpr (KIND == PG_AVG) { a.x += d.x; a.y += d.y; a.z += d.z; a.w += d.w; }
                    else {
                        const unsigned cd = *reinterpret_cast<const unsigned *>(CODE + opix * p.pitch + c);
                        if ((cd & 255u) == tap)         a.x += d.x;
                        if (((cd >> 8) & 255u) == tap)  a.y += d.y;
                        if (((cd >> 16) & 255u) == tap) a.z += d.z;
                        if ((cd >> 24) == tap)          a.w += d.w;
                    }
                } else {
                    const float d = DY[opix * p.C + c];
                    if constexpr (KIND == PG_AVG) a.x += d;
                    else if ((unsigned)CODE[opix * p.pitch + c] == tap) a.x += d;
                }
            }
        }
        if constexpr (KIND == PG_AVG) { a.x /= kk; if (VW == 4) { a.y /= kk; a.z /= kk; a.w /= kk; } }
        if constexpr (VW == 4) *reinterpret_cast<float4 *>(DX + pix * p.C + c) = a;
        else                   DX[pix * p.C + c] = a.x;
    }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_pool_geo_plan reports
struct PoolGeoPlan { int H0, W0, vw_fwd, vw_bwd; };
// admission (who: the entry's name for the message).  T4K_ERR_ARG: an extent below 1; T4K_ERR_UNSUPPORTED: a layer or geometry outside the admitted set
int pool_geo_plan(PoolGeoPlan &g, const char *who, int layer, int N, int H1, int W1, int C, int K, int S, int P, bool al_fwd, bool al_bwd) {
    if (layer != T4K_L_AVGPOOL && layer != T4K_L_MAXPOOL && layer != T4K_L_MINPOOL) return fail(T4K_ERR_UNSUPPORTED, "%s: layer %d is no avg / max / min pool", who, layer);
    if (N < 1 || H1 < 1 || W1 < 1 || C < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (N=%d H1=%d W1=%d C=%d)", who, N, H1, W1, C);
    if (K < 1 || K > 16 || S < 1 || S > 16 || P < 0 || P > K / 2)
        return fail(T4K_ERR_UNSUPPORTED, "%s: kernel_size=%d stride=%d padding=%d not supported (K 1..16, S 1..16, 0 <= P <= K/2)", who, K, S, P);
    if (K > H1 + 2 * P || K > W1 + 2 * P) return fail(T4K_ERR_UNSUPPORTED, "%s: the %dx%d window does not fit the padded %dx%d image", who, K, K, H1 + 2 * P, W1 + 2 * P);
    g.H0 = (H1 + 2 * P - K) / S + 1; g.W0 = (W1 + 2 * P - K) / S + 1;
    if ((long)N * H1 * W1 >= (1L << 31) || (long)N * g.H0 * g.W0 >= (1L << 31)) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 pixels or more", who);
    g.vw_fwd = (al_fwd && C % 4 == 0) ? 4 : 1;
    g.vw_bwd = (al_bwd && C % 4 == 0) ? 4 : 1;
    return T4K_OK;
}

int kind_of(int layer) { return layer == T4K_L_MAXPOOL ? PG_MAX : (layer == T4K_L_MINPOOL ? PG_MIN : PG_AVG); }
bool aligned4(const void *p) { return (((uintptr_t)p) & 3) == 0; }

} // namespace

extern "C" {

int t4k_pool_geo_plan(int layer, int N, int H1, int W1, int C, int K, int S, int P, int aligned, int out[4]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_pool_geo_plan: null");
    PoolGeoPlan g;
    const int rc = pool_geo_plan(g, "t4k_pool_geo_plan", layer, N, H1, W1, C, K, S, P, (aligned & 1) != 0, (aligned & 2) != 0); if (rc != T4K_OK) return rc;
    out[0] = g.H0; out[1] = g.W0; out[2] = g.vw_fwd; out[3] = g.vw_bwd;
    return T4K_OK;
}

int t4k_pool_geo_fwd(int layer, const float *I, float *O, unsigned char *CODE,
                     int N, int H1, int W1, int C, int H0, int W0, int K, int S, int P, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!I || !O) return fail(T4K_ERR_ARG, "t4k_pool_geo_fwd: null tensor");
    PoolGeoPlan g;
    // the 16-byte path: I and O on 16 bytes, and a code store (one dword per thread) on 4
    const int rc = pool_geo_plan(g, "t4k_pool_geo_fwd", layer, N, H1, W1, C, K, S, P, aligned16(I) && aligned16(O) && aligned4(CODE), false); if (rc != T4K_OK) return rc;
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_pool_geo_fwd: output %dx%d, the geometry gives %dx%d", H0, W0, g.H0, g.W0);
    PoolGeoP p = { N, H1, W1, C, H0, W0, K, S, P, C / g.vw_fwd, 4 * ((C + 3) / 4), (long)N * H0 * W0 * (C / g.vw_fwd),
                   fast_div(C / g.vw_fwd), fast_div(W0), fast_div(H0), fast_div(S) };
    hipStream_t hs = t4k::S(s);
    pick<PG_AVG, PG_MAX, PG_MIN>(kind_of(layer), [&](auto kind) { pick<4, 1>(g.vw_fwd, [&](auto vw) {
        T4K_LAUNCH((k_pool_geo_fwd<decltype(kind)::value, decltype(vw)::value>), dim3(grid_for(p.total)), dim3(BLK), 0, hs, I, O, CODE, p); }); });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_pool_geo_bwd(int layer, const unsigned char *CODE, const float *DY, float *DX,
                     int N, int H1, int W1, int C, int H0, int W0, int K, int S, int P, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!DY || !DX) return fail(T4K_ERR_ARG, "t4k_pool_geo_bwd: null tensor");
    const bool avg = layer == T4K_L_AVGPOOL;
    if (!CODE && (layer == T4K_L_MAXPOOL || layer == T4K_L_MINPOOL)) return fail(T4K_ERR_ARG, "t4k_pool_geo_bwd: a max / min backward needs the codes of its forward");
    PoolGeoPlan g;
    const int rc = pool_geo_plan(g, "t4k_pool_geo_bwd", layer, N, H1, W1, C, K, S, P, false, aligned16(DY) && aligned16(DX) && (avg || aligned4(CODE))); if (rc != T4K_OK) return rc;
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_pool_geo_bwd: output %dx%d, the geometry gives %dx%d", H0, W0, g.H0, g.W0);
    PoolGeoP p = { N, H1, W1, C, H0, W0, K, S, P, C / g.vw_bwd, 4 * ((C + 3) / 4), (long)N * H1 * W1 * (C / g.vw_bwd),
                   fast_div(C / g.vw_bwd), fast_div(W1), fast_div(H1), fast_div(S) };
    hipStream_t hs = t4k::S(s);
    pick<PG_AVG, PG_MAX, PG_MIN>(kind_of(layer), [&](auto kind) { pick<4, 1>(g.vw_bwd, [&](auto vw) {
        T4K_LAUNCH((k_pool_geo_bwd<decltype(kind)::value, decltype(vw)::value>), dim3(grid_for(p.total)), dim3(BLK), 0, hs, CODE, DY, DX, p); }); });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
