// attention.hip - multi-head scaled-dot-product attention on NHWC fp32 tokens, forward and backward: torch's
// scaled_dot_product_attention(q, k, v, is_causal) on qkv.reshape(B, L, 3, heads, d).  The reference has no such layer (README v5.0 "Transformer: developing").
// A token's 3E channels are [ Q(E) | K(E) | V(E) ], head h owning channels h d .. (h + 1) d - 1 of each E.  Every product runs on v_mfma_f32_16x16x4_f32,
// and every product is computed TRANSPOSED so that the 16 columns of a wave's MFMA blocks are the wave's own 16 rows of the tile it owns (lane & 15 = row):
//   forward / dQ pass (a wave owns 16 queries i):  S^T = K Q^T,  Y^T += V^T P^T,  dP^T = V dY^T,  dQ^T += K^T dS^T
//   dK | dV pass      (a wave owns 16 keys j):     S = Q K^T,    dP = dY V^T,     dV^T += dY^T P,  dK^T += Q^T dS
// The C/D layout (column = lane & 15, row = 4 (lane >> 4) + reg) then IS the B-operand layout of the next product (k = 4 (lane >> 4) + reg with MFMA number reg),
// so S and P never leave the registers - no LDS transpose, no HBM - and the row statistics (max, sum, LSE, D) are per-lane scalars.  The accumulators hold 4
// consecutive channels per register quad: 16-byte stores.  The wave's own rows (Q and dY, or K and V) stay in registers, 16 bytes per lane per 16 channels, the k
// index of the four MFMAs of a quad being 16 kc + 4 (lane >> 4) + (0..3) on both operands; the tiles of the other side go through LDS.
// The head size is padded with zeros to DP in { 16, 32, 64, 128 } (the rung).  No atomics: every sum has a fixed order, the same bits on every call.
#include "t4k_common.h"
#include "launch.h"
#include <cmath>

using namespace t4k;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AT_BQ = 64;                                // rows a workgroup owns: four waves of 16
// rows of the streamed side per tile.  Two tiles of [rows][DP + pad] floats are live: 64 rows of 132 floats twice are 67.6 KB, above the 64 KB a workgroup's
// static LDS may hold and two workgroups per CU at most; 32 rows are 33.8 KB, four workgroups per CU (160 KB), which is what the registers allow at DP = 128 too
constexpr int at_bk(int DP) { return DP == 128 ? 32 : 64; }
// LDS row pitch in floats: DP + 4 is 4 mod 32 for every DP here.  The transposed reads (ds_read_b32, lane -> row 4 (lane >> 4) + r, column lane & 15) then
// fall on banks 16 (lane >> 4) + (lane & 15) mod 32: no conflict inside a 32-lane half; the row reads (ds_read_b128, lane -> row lane & 15, column 4 (lane >> 4))
// start on bank 4 (row + (lane >> 4)) mod 64: 16 distinct slots in three of the four lane groups, one shared slot in the fourth
constexpr int at_pitch(int DP) { return DP + 4; }

struct AtP {
    int N, L, heads, d, E, causal, nqt;                  // nqt: tiles of AT_BQ rows over L
    float scale;
};

template <int VW> __device__ __forceinline__ float4 at_ld(const float *q) {
    if constexpr (VW == 4) return *reinterpret_cast<const float4 *>(q);
    else return make_float4(q[0], q[1], q[2], q[3]);
}
template <int VW> __device__ __forceinline__ void at_st(float *q, const float4 v) {
    if constexpr (VW == 4) *reinterpret_cast<float4 *>(q) = v;
    else { q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
}
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// c += A B over 4 x 4 values of k: the quad a from LDS (or registers), the quad b from registers
__device__ __forceinline__ f32x4 mfma_quad(const float4 a, const float4 b, f32x4 c) {
    c = mfma4(a.x, b.x, c); c = mfma4(a.y, b.y, c); c = mfma4(a.z, b.z, c); c = mfma4(a.w, b.w, c);
    return c;
}
// the sum over the four lanes that share lane & 15: (x + x^16) + (x^32 + x^48), the same bits in all four
__device__ __forceinline__ float quad_sum(float x) { x += __shfl_xor(x, 16, 64); x += __shfl_xor(x, 32, 64); return x; }
__device__ __forceinline__ float quad_max(float x) { x = fmaxf(x, __shfl_xor(x, 16, 64)); x = fmaxf(x, __shfl_xor(x, 32, 64)); return x; }

// rows [0, ROWS) x channels [0, DP) of a head's Q, K, V (row pitch 3E) or dY (row pitch E) into LDS, zeros beyond `rows` rows and d channels: every MFMA
// operand is a number.  All 256 threads.
template <int ROWS, int DP, int VW>
__device__ __forceinline__ void at_tile(float *lds, const float *src, long pitch, int rows, int d) {
    constexpr int C4 = DP / 4, P = at_pitch(DP);
    for (int it = (int)threadIdx.x; it < ROWS * C4; it += 256) {
        const int r = it / C4, c = (it - r * C4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows && c < d) v = at_ld<VW>(src + (long)r * pitch + c);
        *reinterpret_cast<float4 *>(lds + r * P + c) = v;
    }
}
// the wave's own row `row` (pointer at its channel 0) as 16-byte quads: quad kc holds channels 16 kc + 4 g .. + 3
template <int DP, int VW>
__device__ __forceinline__ void at_row(float4 (&f)[DP / 16], const float *row, bool live, int g, int d) {
#pragma unroll
    for (int kc = 0; kc < DP / 16; kc++) {
        const int c = 16 * kc + 4 * g;
        f[kc] = (live && c < d) ? at_ld<VW>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// workgroup id -> (sample n, head h, tile t).  Unmasked, the tiles of one (n, head) take consecutive ids: they read the same K and V.  Under the causal mask
// tile t visits t + 1 key tiles, so the ids go tile-major, the LAST tiles of every (n, head) first: the workgroups resident on a CU at one time are ids a
// multiple of the device's width apart, and (n, head)-major those would be the same tile of different heads - the CU with the last tiles would run 16 times
// as long as the one with the first (L = 1024).  Longest first, the late arrivals are the short ones; id % 8, the XCD, still keeps a head's K and V behind one L2
__device__ __forceinline__ void at_place(const AtP &p, int &n, int &h, int &t) {
    const int b = (int)blockIdx.x, NH = p.N * p.heads;
    int nh;
    if (p.causal) { const int r = b / NH; nh = b - r * NH; t = p.nqt - 1 - r; }
    else          { nh = b / p.nqt; t = b - nh * p.nqt; }
    n = nh / p.heads; h = nh - n * p.heads;
}

// ------------------------------------------------------------------ forward: a workgroup owns (n, head, 64 queries), K and V tiles of BK keys stream through LDS
template <int DP, int VW>
__global__ void __launch_bounds__(256) k_attn_fwd(const float *__restrict__ QKV, float *__restrict__ O, float *__restrict__ OK, float *__restrict__ LSE, AtP p) {
    constexpr int BK = at_bk(DP), P = at_pitch(DP), KC = DP / 16, JB = BK / 16;
    __shared__ __attribute__((aligned(16))) float sK[BK * P];
    __shared__ __attribute__((aligned(16))) float sV[BK * P];
    int n, h, qt; at_place(p, n, h, qt);
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), il = lane & 15, g = lane >> 4;
    const int q0 = qt * AT_BQ, wq0 = q0 + w * 16, qi = wq0 + il;
    const long E3 = 3L * p.E;
    const float *base = QKV + (long)n * p.L * E3 + (long)h * p.d;          // Q of the sample's token 0
    float4 q[KC];
    at_row<DP, VW>(q, base + (long)qi * E3, qi < p.L, g, p.d);
    f32x4 acc[KC];
#pragma unroll
    for (int cb = 0; cb < KC; cb++) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;                                          // the running max of the row, and THIS lane's share of its running sum
    const int kend = p.causal ? min(p.L, q0 + AT_BQ) : p.L;                // key tiles wholly above the diagonal are not visited
    for (int k0 = 0; k0 < kend; k0 += BK) {
        __syncthreads();
        at_tile<BK, DP, VW>(sK, base + p.E + (long)k0 * E3, E3, p.L - k0, p.d);
        at_tile<BK, DP, VW>(sV, base + 2 * p.E + (long)k0 * E3, E3, p.L - k0, p.d);
        __syncthreads();
        if (wq0 >= p.L || (p.causal && k0 > wq0 + 15)) continue;           // (wave-uniform) no query, or every key of the tile above every query of the wave
        // S^T[j][i]: A = K rows from LDS, B = the wave's Q
        f32x4 s[JB];
#pragma unroll
        for (int jb = 0; jb < JB; jb++) {
            s[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *kr = sK + (jb * 16 + il) * P + 4 * g;
#pragma unroll
            for (int kc = 0; kc < KC; kc++) s[jb] = mfma_quad(*reinterpret_cast<const float4 *>(kr + 16 * kc), q[kc], s[jb]);
        }
        // the lane holds S[i = qi][j = k0 + 16 jb + 4 g + r].  Only a tile that reaches past L or over the diagonal is masked; k0 <= wq0 here, so key k0 is
        // live for every row of the wave and the tile's max is a number
        const bool edge = k0 + BK > p.L || (p.causal && k0 + BK - 1 > wq0);
        float tmax = -INFINITY;
#pragma unroll
        for (int jb = 0; jb < JB; jb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = k0 + jb * 16 + 4 * g + r;
                float v = s[jb][r] * p.scale;
                if (edge && (j >= p.L || (p.causal && j > qi))) v = -INFINITY;
                s[jb][r] = v; tmax = fmaxf(tmax, v);
            }
        const float mn = fmaxf(m, quad_max(tmax));
        const float alpha = __expf(m - mn);                                // the first tile: exp(-inf) = 0 times l = 0 and acc = 0
        float ps = 0.f;
#pragma unroll
        for (int jb = 0; jb < JB; jb++)
#pragma unroll
            for (int r = 0; r < 4; r++) { const float e = __expf(s[jb][r] - mn); s[jb][r] = e; ps += e; }
        l = l * alpha + ps; m = mn;
#pragma unroll
        for (int cb = 0; cb < KC; cb++) acc[cb] *= alpha;
        // Y^T[c][i] += V^T[c][j] P^T[j][i]: A = V read transposed from LDS, B = P as it sits
#pragma unroll
        for (int jb = 0; jb < JB; jb++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float *vr = sV + (jb * 16 + 4 * g + r) * P + il;
#pragma unroll
                for (int cb = 0; cb < KC; cb++) acc[cb] = mfma4(vr[cb * 16], s[jb][r], acc[cb]);
            }
    }
    if (qi >= p.L) return;
    const float lt = quad_sum(l);
    float *o = O + ((long)n * p.L + qi) * p.E + (long)h * p.d, *ok = OK ? OK + ((long)n * p.L + qi) * p.E + (long)h * p.d : nullptr;
#pragma unroll
    for (int cb = 0; cb < KC; cb++) {
        const int c = cb * 16 + 4 * g;
        if (c < p.d) {
            const float4 y = make_float4(acc[cb][0] / lt, acc[cb][1] / lt, acc[cb][2] / lt, acc[cb][3] / lt);
            at_st<VW>(o + c, y);
            if (ok) at_st<VW>(ok + c, y);
        }
    }
    // once per row, so in double and rounded once: ln of an exact key count is then the correctly rounded float
    if (g == 0) LSE[((long)n * p.heads + h) * p.L + qi] = (float)((double)m + log((double)lt));
}

// ------------------------------------------------------------------ backward, first pass: a workgroup owns (n, head, 64 queries): D into the workspace, dQ
template <int DP, int VW>
__global__ void __launch_bounds__(256) k_attn_dq(const float *__restrict__ QKV, const float *__restrict__ OK, const float *__restrict__ DY, const float *__restrict__ LSE,
                                                 float *__restrict__ DQKV, float *__restrict__ Dws, AtP p) {
    constexpr int BK = at_bk(DP), P = at_pitch(DP), KC = DP / 16, JB = BK / 16;
    __shared__ __attribute__((aligned(16))) float sK[BK * P];
    __shared__ __attribute__((aligned(16))) float sV[BK * P];
    int n, h, qt; at_place(p, n, h, qt);
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), il = lane & 15, g = lane >> 4;
    const int q0 = qt * AT_BQ, wq0 = q0 + w * 16, qi = wq0 + il;
    const bool live = qi < p.L;
    const long E3 = 3L * p.E, orow = ((long)n * p.L + qi) * p.E + (long)h * p.d, srow = ((long)n * p.heads + h) * p.L + qi;
    const float *base = QKV + (long)n * p.L * E3 + (long)h * p.d;
    float4 q[KC], dy[KC];
    at_row<DP, VW>(q, base + (long)qi * E3, live, g, p.d);
    at_row<DP, VW>(dy, DY + orow, live, g, p.d);
    float D = 0.f;                                                         // D_i = sum_c dY_ic Y_ic: this lane's channels in order, then the four lanes of the row
    {
        float4 y[KC];
        at_row<DP, VW>(y, OK + orow, live, g, p.d);
#pragma unroll
        for (int kc = 0; kc < KC; kc++) { D += dy[kc].x * y[kc].x; D += dy[kc].y * y[kc].y; D += dy[kc].z * y[kc].z; D += dy[kc].w * y[kc].w; }
        D = quad_sum(D);
    }
    if (live && g == 0) Dws[srow] = D;
    const float lse = live ? LSE[srow] : 0.f;
    f32x4 acc[KC];
#pragma unroll
    for (int kb = 0; kb < KC; kb++) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kend = p.causal ? min(p.L, q0 + AT_BQ) : p.L;
    for (int k0 = 0; k0 < kend; k0 += BK) {
        __syncthreads();
        at_tile<BK, DP, VW>(sK, base + p.E + (long)k0 * E3, E3, p.L - k0, p.d);
        at_tile<BK, DP, VW>(sV, base + 2 * p.E + (long)k0 * E3, E3, p.L - k0, p.d);
        __syncthreads();
        if (wq0 >= p.L || (p.causal && k0 > wq0 + 15)) continue;
        const bool edge = k0 + BK > p.L || wq0 + 16 > p.L || (p.causal && k0 + BK - 1 > wq0);
#pragma unroll
        for (int jb = 0; jb < JB; jb++) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *kr = sK + (jb * 16 + il) * P + 4 * g, *vr = sV + (jb * 16 + il) * P + 4 * g;
#pragma unroll
            for (int kc = 0; kc < KC; kc++) {
                s  = mfma_quad(*reinterpret_cast<const float4 *>(kr + 16 * kc), q[kc], s);       // S^T[j][i]
                dp = mfma_quad(*reinterpret_cast<const float4 *>(vr + 16 * kc), dy[kc], dp);     // dP^T[j][i] = sum_c V[j][c] dY[i][c]
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = k0 + jb * 16 + 4 * g + r;
                float pj = __expf(s[r] * p.scale - lse);
                if (edge && (!live || j >= p.L || (p.causal && j > qi))) pj = 0.f;
                const float ds = pj * (dp[r] - D);
                // dQ^T[k][i] += K^T[k][j] dS^T[j][i]: A = K read transposed
                const float *kt = sK + (jb * 16 + 4 * g + r) * P + il;
#pragma unroll
                for (int kb = 0; kb < KC; kb++) acc[kb] = mfma4(kt[kb * 16], ds, acc[kb]);
            }
        }
    }
    if (!live) return;
    float *dq = DQKV + ((long)n * p.L + qi) * E3 + (long)h * p.d;
#pragma unroll
    for (int kb = 0; kb < KC; kb++) {
        const int c = kb * 16 + 4 * g;
        if (c < p.d) at_st<VW>(dq + c, make_float4(p.scale * acc[kb][0], p.scale * acc[kb][1], p.scale * acc[kb][2], p.scale * acc[kb][3]));
    }
}

// ------------------------------------------------------------------ backward, second pass: a workgroup owns (n, head, 64 keys), Q and dY tiles of BK queries stream
// through LDS with their LSE and D: dK and dV
template <int DP, int VW>
__global__ void __launch_bounds__(256) k_attn_dkv(const float *__restrict__ QKV, const float *__restrict__ DY, const float *__restrict__ LSE, const float *__restrict__ Dws,
                                                  float *__restrict__ DQKV, AtP p) {
    constexpr int BQ = at_bk(DP), P = at_pitch(DP), KC = DP / 16, IB = BQ / 16;
    __shared__ __attribute__((aligned(16))) float sQ[BQ * P];
    __shared__ __attribute__((aligned(16))) float sDY[BQ * P];
    __shared__ __attribute__((aligned(16))) float sL[BQ];
    __shared__ __attribute__((aligned(16))) float sD[BQ];
    int n, h, kt; at_place(p, n, h, kt);
    if (p.causal) kt = p.nqt - 1 - kt;                                     // here the FIRST tiles hold the most queries under the causal mask
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), il = lane & 15, g = lane >> 4;
    const int j0 = kt * AT_BQ, wj0 = j0 + w * 16, kj = wj0 + il;
    const bool live = kj < p.L;
    const long E3 = 3L * p.E, srow = ((long)n * p.heads + h) * p.L;
    const float *base = QKV + (long)n * p.L * E3 + (long)h * p.d;
    const float *dyb = DY + (long)n * p.L * p.E + (long)h * p.d;
    float4 kf[KC], vf[KC];
    at_row<DP, VW>(kf, base + p.E + (long)kj * E3, live, g, p.d);
    at_row<DP, VW>(vf, base + 2 * p.E + (long)kj * E3, live, g, p.d);
    f32x4 ak[KC], av[KC];
#pragma unroll
    for (int cb = 0; cb < KC; cb++) { ak[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; av[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const int ibeg = p.causal ? j0 / BQ * BQ : 0;                          // query tiles wholly in front of the workgroup's keys are not visited
    for (int i0 = ibeg; i0 < p.L; i0 += BQ) {
        __syncthreads();
        at_tile<BQ, DP, VW>(sQ, base + (long)i0 * E3, E3, p.L - i0, p.d);
        at_tile<BQ, DP, VW>(sDY, dyb + (long)i0 * p.E, p.E, p.L - i0, p.d);
        if ((int)threadIdx.x < BQ) {
            const int i = i0 + (int)threadIdx.x;
            sL[threadIdx.x] = i < p.L ? LSE[srow + i] : 0.f;
            sD[threadIdx.x] = i < p.L ? Dws[srow + i] : 0.f;
        }
        __syncthreads();
        if (wj0 >= p.L || (p.causal && i0 + BQ - 1 < wj0)) continue;      // (wave-uniform) no key, or every query of the tile in front of every key of the wave
        const bool edge = i0 + BQ > p.L || wj0 + 16 > p.L || (p.causal && wj0 + 15 > i0);
#pragma unroll
        for (int ib = 0; ib < IB; ib++) {
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *qr = sQ + (ib * 16 + il) * P + 4 * g, *dr = sDY + (ib * 16 + il) * P + 4 * g;
#pragma unroll
            for (int kc = 0; kc < KC; kc++) {
                s  = mfma_quad(*reinterpret_cast<const float4 *>(qr + 16 * kc), kf[kc], s);      // S[i][j]
                dp = mfma_quad(*reinterpret_cast<const float4 *>(dr + 16 * kc), vf[kc], dp);     // dP[i][j] = sum_c dY[i][c] V[j][c]
            }
            const float4 ls = *reinterpret_cast<const float4 *>(sL + ib * 16 + 4 * g), dd = *reinterpret_cast<const float4 *>(sD + ib * 16 + 4 * g);
            const float lsr[4] = { ls.x, ls.y, ls.z, ls.w }, ddr[4] = { dd.x, dd.y, dd.z, dd.w };
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int ir = ib * 16 + 4 * g + r, i = i0 + ir;
                float pj = __expf(s[r] * p.scale - lsr[r]);
                if (edge && (!live || i >= p.L || (p.causal && kj > i))) pj = 0.f;
                const float ds = pj * (dp[r] - ddr[r]);
                // dV^T[c][j] += dY^T[c][i] P[i][j],  dK^T[k][j] += Q^T[k][i] dS[i][j]: A read transposed
                const float *dt = sDY + ir * P + il, *qt = sQ + ir * P + il;
#pragma unroll
                for (int cb = 0; cb < KC; cb++) { av[cb] = mfma4(dt[cb * 16], pj, av[cb]); ak[cb] = mfma4(qt[cb * 16], ds, ak[cb]); }
            }
        }
    }
    if (!live) return;
    float *dk = DQKV + ((long)n * p.L + kj) * E3 + p.E + (long)h * p.d, *dv = dk + p.E;
#pragma unroll
    for (int cb = 0; cb < KC; cb++) {
        const int c = cb * 16 + 4 * g;
        if (c < p.d) {
            at_st<VW>(dk + c, make_float4(p.scale * ak[cb][0], p.scale * ak[cb][1], p.scale * ak[cb][2], p.scale * ak[cb][3]));
            at_st<VW>(dv + c, make_float4(av[cb][0], av[cb][1], av[cb][2], av[cb][3]));
        }
    }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_attention_plan reports
struct AtPlan { int rung, vw, dp, bk, nqt, wgs; long ws; };
// admission (who: the entry's name for the message) in 64 bits: the extents may be anything an int holds
int attn_plan(AtPlan &a, const char *who, int N, int L, int heads, int d, bool aligned, long ws_bytes) {
    if (N < 1 || L < 1 || heads < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (N=%d L=%d heads=%d)", who, N, L, heads);
    if (ws_bytes < 0) return fail(T4K_ERR_ARG, "%s: ws_bytes below 0", who);
    if (d < 4 || d > 128 || d % 4 != 0) return fail(T4K_ERR_UNSUPPORTED, "%s: head size d=%d not supported (4 <= d <= 128, d %% 4 == 0)", who, d);
    const long lim = 1L << 31, tok = (long)N * L;                          // tok < 2^62; E3 < 2^31: the products below are taken one factor at a time
    const long E3 = 3L * heads * d;
    if (tok >= lim || E3 >= lim || tok * E3 >= lim) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 elements or more", who);
    a.ws = tok * heads * (long)sizeof(float);                              // D_i of the backward, one float per (n, head, token): below 2^31 / 3
    if (a.ws > ws_bytes) return fail(T4K_ERR_UNSUPPORTED, "%s: the backward's row sums (%ld bytes) do not fit the workspace", who, a.ws);
    a.rung = d <= 16 ? 1 : d <= 32 ? 2 : d <= 64 ? 3 : 4;
    a.dp = 8 << a.rung;
    a.bk = at_bk(a.dp);
    a.vw = aligned ? 4 : 1;                                                // d % 4 == 0, so E and 3E are too: every 16-byte item of an aligned tensor is aligned
    a.nqt = (L + AT_BQ - 1) / AT_BQ;
    a.wgs = (int)((long)N * heads * a.nqt);                                // <= N heads L < 2^31 / 12
    return T4K_OK;
}
AtP attn_parms(const AtPlan &a, int N, int L, int heads, int d, int causal) {
    AtP p;
    p.N = N; p.L = L; p.heads = heads; p.d = d; p.E = heads * d; p.causal = causal != 0; p.nqt = a.nqt;
    p.scale = (float)(1.0 / std::sqrt((double)d));                         // in double, rounded once
    return p;
}
bool at16(const void *a, const void *b, const void *c, const void *d, const void *e = nullptr) {
    return aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) && aligned16(e);
}
bool overlap(const float *a, long na, const float *b, long nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float), b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
    return a0 < b1 && b0 < a1;
}

} // namespace

extern "C" {

int t4k_attention_plan(int N, int L, int heads, int d, int causal, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_attention_plan: null");
    AtPlan a;
    const int rc = attn_plan(a, "t4k_attention_plan", N, L, heads, d, aligned != 0, ws_bytes); if (rc != T4K_OK) return rc;
    (void)causal;                                                          // the mask changes the tiles a workgroup visits, not the plan
    out[0] = a.rung; out[1] = a.vw; out[2] = AT_BQ; out[3] = a.bk; out[4] = 1; out[5] = 2; out[6] = a.wgs; out[7] = (int)a.ws;
    return T4K_OK;
}

int t4k_attention_fwd(const float *QKV, float *O, float *OK, float *LSE, int N, int L, int heads, int d, int causal, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!QKV || !O || !LSE) return fail(T4K_ERR_ARG, "t4k_attention_fwd: null tensor");
    AtPlan a;
    const int rc = attn_plan(a, "t4k_attention_fwd", N, L, heads, d, at16(QKV, O, OK, LSE), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const AtP p = attn_parms(a, N, L, heads, d, causal);
    hipStream_t hs = t4k::S(s);
    pick<16, 32, 64, 128>(a.dp, [&](auto dp) {
        pick<4, 1>(a.vw, [&](auto vw) {
            T4K_LAUNCH((k_attn_fwd<decltype(dp)::value, decltype(vw)::value>), dim3((unsigned)a.wgs), dim3(256), 0, hs, QKV, O, OK, LSE, p);
        });
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_attention_bwd(const float *QKV, const float *OK, const float *DY, const float *LSE, float *DQKV,
                      int N, int L, int heads, int d, int causal, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!QKV || !OK || !DY || !LSE || !DQKV) return fail(T4K_ERR_ARG, "t4k_attention_bwd: null tensor");
    AtPlan a;
    const int rc = attn_plan(a, "t4k_attention_bwd", N, L, heads, d, at16(QKV, OK, DY, LSE, DQKV), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long ne = (long)N * L * heads * d;
    if (overlap(DQKV, 3 * ne, QKV, 3 * ne) || overlap(DQKV, 3 * ne, OK, ne) || overlap(DQKV, 3 * ne, DY, ne))
        return fail(T4K_ERR_ARG, "t4k_attention_bwd: DQKV overlaps QKV, OK or DY");
    const AtP p = attn_parms(a, N, L, heads, d, causal);
    hipStream_t hs = t4k::S(s);
    float *ws = ws_for(s);
    pick<16, 32, 64, 128>(a.dp, [&](auto dp) {
        pick<4, 1>(a.vw, [&](auto vw) {
            constexpr int DP = decltype(dp)::value, VW = decltype(vw)::value;
            T4K_LAUNCH((k_attn_dq<DP, VW>), dim3((unsigned)a.wgs), dim3(256), 0, hs, QKV, OK, DY, LSE, DQKV, ws, p);
            T4K_LAUNCH((k_attn_dkv<DP, VW>), dim3((unsigned)a.wgs), dim3(256), 0, hs, QKV, DY, LSE, (const float *)ws, DQKV, p);
        });
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
