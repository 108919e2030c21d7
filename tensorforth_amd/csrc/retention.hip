// retention.hip - multi-scale retention (RetNet) on NHWC fp32 tokens, forward and backward, in its chunkwise form.  The reference has no
// such layer (its README lists "Retentive" for v4.2).  A token's 3E channels are [ Q(E) | K(E) | V(E) ], head h owning channels h d .. (h + 1) d - 1 of each E
// - attention.hip's layout.  With g = 1 - 2^(-5-h) and scale = (float)(1 / sqrt(d)):  Y_i = scale sum_{j <= i} g^(i-j) (Q_i . K_j) V_j.
// The L tokens of a (sample, head) are cut into chunks of B.  With S_c = sum_{j < cB} g^(cB-1-j) K_j^T V_j, the d x d state in front of chunk c, token i = cB + r is
//   Y_i = scale ( sum_{j in chunk, j <= i} g^(i-j) (Q_i . K_j) V_j  +  g^(r+1) Q_i S_c ),        S_(c+1) = g^B S_c + U_c,  U_c = sum_r g^(B-1-r) K_r^T V_r
// and the backward is the same shape with the reverse state R_c = sum_{i >= (c+1)B} g^(i-(c+1)B+1) Q_i^T dY_i:
//   dQ_i = scale ( sum_{j<=i} g^(i-j) (dY_i . V_j) K_j + g^(r+1) dY_i S_c^T ),  dK_j = scale ( sum_{i>=j} g^(i-j) (dY_i . V_j) Q_i + g^(B-1-r) V_j R_c^T ),
//   dV_j = scale ( sum_{i>=j} g^(i-j) (Q_i . K_j) dY_i + g^(B-1-r) K_j R_c ).
// Every power of g is exp2f(log2(g) dist) of an integer distance, log2(g) formed in double on the host; every factor is at most 1 where it is used.
// All products run on v_mfma_f32_16x16x4_f32 in attention.hip's transposed tile map (mfma_rows.h): a wave owns 16 rows (lane & 15 = row), the scores come out in
// the B-operand layout of the product that consumes them and never leave the registers, and the state is one more A operand read from LDS.
// No atomics: every sum has a fixed order, the same bits on every call.
#include "t4k_common.h"
#include "launch.h"
#include "mfma_rows.h"
#include <climits>
#include <cmath>

using namespace t4k;

namespace {

// tokens per chunk.  Two tiles of [B][DP + 4] floats are live, and the states stream through one of them B rows at a time: 34.8 KB at DP = 64.  At DP = 128
// 64 rows twice are 67.6 KB, above a workgroup's static LDS, so that rung works on chunks of 32 (33.8 KB); two of its four waves then own no rows
constexpr int rt_b(int DP) { return DP == 128 ? 32 : 64; }
constexpr int RT_MAXH = 32;                              // beyond 32 heads g rounds to 1 in float

struct RtP {
    int N, L, heads, d, E, chunks;
    float scale;
    float lam[RT_MAXH];                                  // log2(g_h)
};

__device__ __forceinline__ float rt_pow(float lam, int dist) { return exp2f(lam * (float)dist); }
__device__ __forceinline__ float4 rt_mul4(const float4 a, const float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 rt_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// at_tile with row r scaled by g^(off + sgn r): the decayed side of a state product
template <int ROWS, int DP, int VW>
__device__ __forceinline__ void rt_tile_decayed(float *lds, const float *src, long pitch, int rows, int d, float lam, int off, int sgn) {
    constexpr int C4 = DP / 4, P = at_pitch(DP);
    for (int it = (int)threadIdx.x; it < ROWS * C4; it += 256) {
        const int r = it / C4, c = (it - r * C4) * 4;
        float4 v = rt_zero4();
        if (r < rows && c < d) v = rt_mul4(at_ld<VW>(src + (long)r * pitch + c), rt_pow(lam, off + sgn * r));
        *reinterpret_cast<float4 *>(lds + r * P + c) = v;
    }
}
// acc^T[c][i] += sum_k T[k][c] b_i[k] over the B rows k0 .. of a d x d state tile in LDS (rows = k): A read transposed, B the wave's row quads
template <int DP>
__device__ __forceinline__ void rt_cross_t(f32x4 (&acc)[DP / 16], const float *tile, int k0, const float4 (&b)[DP / 16], int il, int g) {
    constexpr int B = rt_b(DP), P = at_pitch(DP), KC = DP / 16, KK = (B < DP ? B : DP) / 16;
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
        const float4 q = b[k0 / 16 + kk];
        const float bx[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const float *sr = tile + (kk * 16 + 4 * g + x) * P + il;
#pragma unroll
            for (int cb = 0; cb < KC; cb++) acc[cb] = mfma4(sr[cb * 16], bx[x], acc[cb]);
        }
    }
}
// acc^T[k][i] += sum_c T[k][c] b_i[c] for the B rows k0 .. of the tile (rows = k, the output): A read along the rows
template <int DP>
__device__ __forceinline__ void rt_cross_r(f32x4 (&acc)[DP / 16], const float *tile, int k0, const float4 (&b)[DP / 16], int il, int g) {
    constexpr int B = rt_b(DP), P = at_pitch(DP), KC = DP / 16, KK = (B < DP ? B : DP) / 16;
#pragma unroll
    for (int kk = 0; kk < KK; kk++) {
        const float *sr = tile + (kk * 16 + il) * P + 4 * g;
#pragma unroll
        for (int kc = 0; kc < KC; kc++) acc[k0 / 16 + kk] = mfma_quad(*reinterpret_cast<const float4 *>(sr + 16 * kc), b[kc], acc[k0 / 16 + kk]);
    }
}
template <int DP, int VW>
__device__ __forceinline__ void rt_store(float *row, const f32x4 (&acc)[DP / 16], float scale, int g, int d) {
#pragma unroll
    for (int cb = 0; cb < DP / 16; cb++) {
        const int c = cb * 16 + 4 * g;
        if (c < d) at_st<VW>(row + c, make_float4(scale * acc[cb][0], scale * acc[cb][1], scale * acc[cb][2], scale * acc[cb][3]));
    }
}

// ------------------------------------------------------------------ chunk-local state: a workgroup owns (n, head, chunk) and writes one d x d product.
// Forward (REV = false), chunks 0 .. chunks - 2 into ST's slot c:      U_c[k][c'] = sum_r K_r[k] g^(B-1-r) V_r[c']
// reverse (REV = true),  chunks 1 .. chunks - 1 into the workspace's slot c - 1:  W_c[k][c'] = sum_r Q_r[k] g^(r+1) dY_r[c']
// Both operands are staged once through LDS; wave w owns the 16-row blocks w, w + 4, .. of the product
template <int DP, int VW, bool REV>
__global__ void __launch_bounds__(256) k_retn_state(const float *__restrict__ QKV, const float *__restrict__ DY, float *__restrict__ U, RtP p) {
    constexpr int B = rt_b(DP), P = at_pitch(DP), KC = DP / 16;
    __shared__ __attribute__((aligned(16))) float sA[B * P];
    __shared__ __attribute__((aligned(16))) float sB[B * P];
    const int nch = p.chunks - 1, nh = (int)blockIdx.x / nch, cl = (int)blockIdx.x - nh * nch, n = nh / p.heads, h = nh - n * p.heads;
    const int c = cl + (REV ? 1 : 0), r0 = c * B, rows = p.L - r0;
    const long E3 = 3L * p.E;
    const float lam = p.lam[h];
    const float *base = QKV + ((long)n * p.L + r0) * E3 + (long)h * p.d;
    if constexpr (REV) {
        at_tile<B, DP, VW>(sA, base, E3, rows, p.d);
        rt_tile_decayed<B, DP, VW>(sB, DY + ((long)n * p.L + r0) * p.E + (long)h * p.d, p.E, rows, p.d, lam, 1, 1);
    } else {
        at_tile<B, DP, VW>(sA, base + p.E, E3, rows, p.d);
        rt_tile_decayed<B, DP, VW>(sB, base + 2 * p.E, E3, rows, p.d, lam, B - 1, -1);
    }
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6), il = lane & 15, g = lane >> 4;
    float *u = U + ((long)nh * (REV ? nch : p.chunks) + cl) * p.d * p.d;
    for (int kb = w; kb * 16 < p.d; kb += 4) {
        f32x4 acc[KC];
#pragma unroll
        for (int cb = 0; cb < KC; cb++) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int row = 4 * g; row < B; row += 16)
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const float a = sA[(row + x) * P + kb * 16 + il];
                const float *br = sB + (row + x) * P + il;
#pragma unroll
                for (int cb = 0; cb < KC; cb++) acc[cb] = mfma4(a, br[cb * 16], acc[cb]);
            }
        // the lane holds rows kb 16 + 4 g + (0..3) of column cb 16 + il
#pragma unroll
        for (int cb = 0; cb < KC; cb++) {
            const int cc = cb * 16 + il;
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int k = kb * 16 + 4 * g + x;
                if (cc < p.d && k < p.d) u[(long)k * p.d + cc] = acc[cb][x];
            }
        }
    }
}

// ------------------------------------------------------------------ the scan over the chunks of one (n, head): a thread owns one of the d d elements.
// Forward, in place over `chunks` slots: slot c holds U_c and receives the exclusive state S_c (S_0 = 0, S_(c+1) = g^B S_c + U_c; the last slot held nothing).
// Reverse, in place over chunks - 1 slots: slot s holds W_(s+1) and receives R_s = W_(s+1) + g^B R_(s+1), R_(chunks-1) = 0.
// Eight loads are in flight per step; the sums are serial: a fixed order
__global__ void __launch_bounds__(64) k_retn_scan(float *__restrict__ S, RtP p, int B, int rev) {
    const long dd = (long)p.d * p.d, per = (dd + 63) / 64;
    const long nh = (long)blockIdx.x / per, e = ((long)blockIdx.x - nh * per) * 64 + threadIdx.x;
    if (e >= dd) return;
    const float gB = rt_pow(p.lam[(int)(nh % p.heads)], B);
    float carry = 0.f, u[8];
    if (!rev) {
        float *q = S + nh * p.chunks * dd + e;
        for (int c = 0; c < p.chunks; c += 8) {
#pragma unroll
            for (int k = 0; k < 8; k++) u[k] = c + k + 1 < p.chunks ? q[(c + k) * dd] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; k++) if (c + k < p.chunks) { q[(c + k) * dd] = carry; carry = fmaf(gB, carry, u[k]); }
        }
    } else {
        float *q = S + nh * (p.chunks - 1) * dd + e;
        for (int s = p.chunks - 2; s >= 0; s -= 8) {
#pragma unroll
            for (int k = 0; k < 8; k++) u[k] = s - k >= 0 ? q[(s - k) * dd] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; k++) if (s - k >= 0) { carry = fmaf(gB, carry, u[k]); q[(s - k) * dd] = carry; }
        }
    }
}

// what every chunk kernel works out of its workgroup and lane ids
struct RtWho { int nh, n, h, c, w, il, g, r; long tok; bool live, wave_live; float lam; };
template <int DP> __device__ __forceinline__ RtWho rt_who(const RtP &p) {
    constexpr int B = rt_b(DP);
    RtWho o;
    o.nh = (int)blockIdx.x / p.chunks; o.c = (int)blockIdx.x - o.nh * p.chunks; o.n = o.nh / p.heads; o.h = o.nh - o.n * p.heads;
    const int lane = (int)(threadIdx.x & 63);
    o.w = (int)(threadIdx.x >> 6); o.il = lane & 15; o.g = lane >> 4; o.r = o.w * 16 + o.il;             // the lane's row of the chunk
    const int t = o.c * B + o.r;
    o.wave_live = o.w * 16 < B && o.c * B + o.w * 16 < p.L;                                              // (wave-uniform) the wave owns a token
    o.live = o.r < B && t < p.L;
    o.tok = (long)o.n * p.L + t;
    o.lam = p.lam[o.h];
    return o;
}

// ------------------------------------------------------------------ forward: a workgroup owns (n, head, chunk), a wave 16 of its queries
template <int DP, int VW>
__global__ void __launch_bounds__(256) k_retn_out(const float *__restrict__ QKV, float *__restrict__ O, const float *__restrict__ ST, RtP p) {
    constexpr int B = rt_b(DP), P = at_pitch(DP), KC = DP / 16, JB = B / 16;
    __shared__ __attribute__((aligned(16))) float sK[B * P];
    __shared__ __attribute__((aligned(16))) float sV[B * P];
    const RtWho o = rt_who<DP>(p);
    const int il = o.il, g = o.g;
    const long E3 = 3L * p.E;
    const float *base = QKV + ((long)o.n * p.L + (long)o.c * B) * E3 + (long)o.h * p.d;                 // Q of the chunk's first token
    float4 q[KC];
    at_row<DP, VW>(q, QKV + o.tok * E3 + (long)o.h * p.d, o.live, g, p.d);
    f32x4 acc[KC];
#pragma unroll
    for (int cb = 0; cb < KC; cb++) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    at_tile<B, DP, VW>(sK, base + p.E, E3, p.L - o.c * B, p.d);
    at_tile<B, DP, VW>(sV, base + 2 * p.E, E3, p.L - o.c * B, p.d);
    __syncthreads();
    if (o.wave_live) {
#pragma unroll
        for (int jb = 0; jb < JB; jb++) {
            if (jb > o.w) break;                                           // (wave-uniform) every key of the block behind every query of the wave
            // S^T[j][i]: A = K rows from LDS, B = the wave's Q; the lane holds S[i = r][j = 16 jb + 4 g + x]
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *kr = sK + (jb * 16 + il) * P + 4 * g;
#pragma unroll
            for (int kc = 0; kc < KC; kc++) s = mfma_quad(*reinterpret_cast<const float4 *>(kr + 16 * kc), q[kc], s);
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int dist = o.r - (jb * 16 + 4 * g + x);
                const float pj = dist < 0 ? 0.f : s[x] * rt_pow(o.lam, dist);
                // Y^T[c][i] += V^T[c][j] P^T[j][i]: A = V read transposed from LDS, B = P as it sits
                const float *vr = sV + (jb * 16 + 4 * g + x) * P + il;
#pragma unroll
                for (int cb = 0; cb < KC; cb++) acc[cb] = mfma4(vr[cb * 16], pj, acc[cb]);
            }
        }
    }
    if (o.c > 0) {                                                         // the cross term g^(r+1) Q_i S_c: Q decayed in place, S_c through sK in tiles of B rows
        const float dec = rt_pow(o.lam, o.r + 1);
#pragma unroll
        for (int kc = 0; kc < KC; kc++) q[kc] = rt_mul4(q[kc], dec);
        const float *S = ST + ((long)o.nh * p.chunks + o.c) * p.d * p.d;
#pragma unroll
        for (int k0 = 0; k0 < DP; k0 += B) {
            if (k0 >= p.d) break;
            __syncthreads();
            at_tile<B, DP, VW>(sK, S + (long)k0 * p.d, p.d, p.d - k0, p.d);
            __syncthreads();
            if (o.wave_live) rt_cross_t<DP>(acc, sK, k0, q, il, g);
        }
    }
    if (o.live) rt_store<DP, VW>(O + o.tok * p.E + (long)o.h * p.d, acc, p.scale, g, p.d);
}

// ------------------------------------------------------------------ backward: a workgroup owns (n, head, chunk); its waves first own 16 queries each (dQ: K and
// V, then S_c, through LDS), then the same 16 tokens as keys (dK and dV: Q and dY, then R_c, through LDS).  Two tiles are live at any time
template <int DP, int VW>
__global__ void __launch_bounds__(256) k_retn_grad(const float *__restrict__ QKV, const float *__restrict__ DY, const float *__restrict__ ST,
                                                   const float *__restrict__ R, float *__restrict__ DQKV, RtP p) {
    constexpr int B = rt_b(DP), P = at_pitch(DP), KC = DP / 16, JB = B / 16;
    __shared__ __attribute__((aligned(16))) float s0[B * P];
    __shared__ __attribute__((aligned(16))) float s1[B * P];
    const RtWho o = rt_who<DP>(p);
    const int il = o.il, g = o.g, rows = p.L - o.c * B;
    const long E3 = 3L * p.E;
    const float *base = QKV + ((long)o.n * p.L + (long)o.c * B) * E3 + (long)o.h * p.d;
    const float *dyb = DY + ((long)o.n * p.L + (long)o.c * B) * p.E + (long)o.h * p.d;
    const float *own = QKV + o.tok * E3 + (long)o.h * p.d;
    float *down = DQKV + o.tok * E3 + (long)o.h * p.d;
    {   // ---- the wave's tokens as queries: G^T = V dY^T decayed and masked, dQ^T += K^T G^T
        float4 dy[KC];
        at_row<DP, VW>(dy, DY + o.tok * p.E + (long)o.h * p.d, o.live, g, p.d);
        f32x4 acc[KC];
#pragma unroll
        for (int kb = 0; kb < KC; kb++) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        at_tile<B, DP, VW>(s0, base + p.E, E3, rows, p.d);
        at_tile<B, DP, VW>(s1, base + 2 * p.E, E3, rows, p.d);
        __syncthreads();
        if (o.wave_live) {
#pragma unroll
            for (int jb = 0; jb < JB; jb++) {
                if (jb > o.w) break;
                f32x4 gq = f32x4{0.f, 0.f, 0.f, 0.f};
                const float *vr = s1 + (jb * 16 + il) * P + 4 * g;
#pragma unroll
                for (int kc = 0; kc < KC; kc++) gq = mfma_quad(*reinterpret_cast<const float4 *>(vr + 16 * kc), dy[kc], gq);
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    const int dist = o.r - (jb * 16 + 4 * g + x);
                    const float gj = dist < 0 ? 0.f : gq[x] * rt_pow(o.lam, dist);
                    const float *kt = s0 + (jb * 16 + 4 * g + x) * P + il;
#pragma unroll
                    for (int kb = 0; kb < KC; kb++) acc[kb] = mfma4(kt[kb * 16], gj, acc[kb]);
                }
            }
        }
        if (o.c > 0) {                                                     // g^(r+1) dY_i S_c^T
            const float dec = rt_pow(o.lam, o.r + 1);
#pragma unroll
            for (int kc = 0; kc < KC; kc++) dy[kc] = rt_mul4(dy[kc], dec);
            const float *S = ST + ((long)o.nh * p.chunks + o.c) * p.d * p.d;
#pragma unroll
            for (int k0 = 0; k0 < DP; k0 += B) {
                if (k0 >= p.d) break;
                __syncthreads();
                at_tile<B, DP, VW>(s0, S + (long)k0 * p.d, p.d, p.d - k0, p.d);
                __syncthreads();
                if (o.wave_live) rt_cross_r<DP>(acc, s0, k0, dy, il, g);
            }
        }
        if (o.live) rt_store<DP, VW>(down, acc, p.scale, g, p.d);
    }
    // ---- the same tokens as keys: S = Q K^T and G = dY V^T decayed and masked, dV^T += dY^T S, dK^T += Q^T G
    __syncthreads();
    at_tile<B, DP, VW>(s0, base, E3, rows, p.d);
    at_tile<B, DP, VW>(s1, dyb, p.E, rows, p.d);
    __syncthreads();
    float4 kf[KC], vf[KC];
    at_row<DP, VW>(kf, own + p.E, o.live, g, p.d);
    at_row<DP, VW>(vf, own + 2 * p.E, o.live, g, p.d);
    f32x4 ak[KC], av[KC];
#pragma unroll
    for (int cb = 0; cb < KC; cb++) { ak[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; av[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (o.wave_live) {
#pragma unroll
        for (int ib = 0; ib < JB; ib++) {
            if (ib < o.w) continue;                                        // (wave-uniform) every query of the block in front of every key of the wave
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, gp = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *qr = s0 + (ib * 16 + il) * P + 4 * g, *dr = s1 + (ib * 16 + il) * P + 4 * g;
#pragma unroll
            for (int kc = 0; kc < KC; kc++) {
                s  = mfma_quad(*reinterpret_cast<const float4 *>(qr + 16 * kc), kf[kc], s);      // S[i][j]
                gp = mfma_quad(*reinterpret_cast<const float4 *>(dr + 16 * kc), vf[kc], gp);     // G[i][j] = sum_c dY[i][c] V[j][c]
            }
#pragma unroll
            for (int x = 0; x < 4; x++) {
                const int ir = ib * 16 + 4 * g + x, dist = ir - o.r;
                const float pw = rt_pow(o.lam, dist), pj = dist < 0 ? 0.f : s[x] * pw, gj = dist < 0 ? 0.f : gp[x] * pw;
                const float *dt = s1 + ir * P + il, *qt = s0 + ir * P + il;
#pragma unroll
                for (int cb = 0; cb < KC; cb++) { av[cb] = mfma4(dt[cb * 16], pj, av[cb]); ak[cb] = mfma4(qt[cb * 16], gj, ak[cb]); }
            }
        }
    }
    if (o.c + 1 < p.chunks) {                                              // g^(B-1-r) K_j R_c and g^(B-1-r) V_j R_c^T
        const float dec = rt_pow(o.lam, B - 1 - o.r);
#pragma unroll
        for (int kc = 0; kc < KC; kc++) { kf[kc] = rt_mul4(kf[kc], dec); vf[kc] = rt_mul4(vf[kc], dec); }
        const float *Rc = R + ((long)o.nh * (p.chunks - 1) + o.c) * p.d * p.d;
#pragma unroll
        for (int k0 = 0; k0 < DP; k0 += B) {
            if (k0 >= p.d) break;
            __syncthreads();
            at_tile<B, DP, VW>(s0, Rc + (long)k0 * p.d, p.d, p.d - k0, p.d);
            __syncthreads();
            if (o.wave_live) { rt_cross_t<DP>(av, s0, k0, kf, il, g); rt_cross_r<DP>(ak, s0, k0, vf, il, g); }
        }
    }
    if (o.live) { rt_store<DP, VW>(down + p.E, ak, p.scale, g, p.d); rt_store<DP, VW>(down + 2 * p.E, av, p.scale, g, p.d); }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_retention_plan reports
struct RtPlan { int rung, vw, dp, b, chunks, wgs, launches; long ws; };
// admission (who: the entry's name for the message) in 64 bits: the extents may be anything an int holds
int retn_plan(RtPlan &a, const char *who, int N, int L, int heads, int d, bool aligned, long ws_bytes) {
    if (N < 1 || L < 1 || heads < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (N=%d L=%d heads=%d)", who, N, L, heads);
    if (heads > RT_MAXH) return fail(T4K_ERR_ARG, "%s: heads=%d, more than %d (the decay of a further head rounds to 1)", who, heads, RT_MAXH);
    if (ws_bytes < 0) return fail(T4K_ERR_ARG, "%s: ws_bytes below 0", who);
    if (d < 4 || d > 128 || d % 4 != 0) return fail(T4K_ERR_UNSUPPORTED, "%s: head size d=%d not supported (4 <= d <= 128, d %% 4 == 0)", who, d);
    const long lim = 1L << 31, tok = (long)N * L, E3 = 3L * heads * d;     // tok < 2^62, E3 < 2^14
    if (tok >= lim || tok * E3 >= lim) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 elements or more", who);
    a.rung = d <= 16 ? 1 : d <= 32 ? 2 : d <= 64 ? 3 : 4;
    a.dp = 8 << a.rung;
    a.b = rt_b(a.dp);
    a.chunks = (L + a.b - 1) / a.b;
    a.ws = (long)N * heads * (a.chunks - 1) * d * d * (long)sizeof(float);    // the reverse states R_0 .. R_(chunks-2): below 2^31 x 2^9
    if (a.ws > ws_bytes) return fail(T4K_ERR_UNSUPPORTED, "%s: the backward's reverse states (%ld bytes) do not fit the workspace", who, a.ws);
    a.vw = aligned ? 4 : 1;                                                // d % 4 == 0: every row of Q, K, V, dY and of a state starts on 16 bytes then
    a.wgs = (int)((long)N * heads * a.chunks);                             // <= N heads L < 2^31
    a.launches = a.chunks > 1 ? 3 : 1;                                     // chunk-local states, scan, the chunk launch; one chunk has no state
    return T4K_OK;
}
RtP retn_parms(const RtPlan &a, int N, int L, int heads, int d) {
    RtP p;
    p.N = N; p.L = L; p.heads = heads; p.d = d; p.E = heads * d; p.chunks = a.chunks;
    p.scale = (float)(1.0 / std::sqrt((double)d));                         // in double, rounded once
    for (int h = 0; h < RT_MAXH; h++) p.lam[h] = (float)std::log2(1.0 - std::ldexp(1.0, -5 - h));
    return p;
}

} // namespace

extern "C" {

int t4k_retention_plan(int N, int L, int heads, int d, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_retention_plan: null");
    RtPlan a;
    const int rc = retn_plan(a, "t4k_retention_plan", N, L, heads, d, aligned != 0, ws_bytes); if (rc != T4K_OK) return rc;
    out[0] = a.rung; out[1] = a.vw; out[2] = a.b; out[3] = a.chunks; out[4] = a.launches; out[5] = a.launches; out[6] = a.wgs;
    out[7] = a.ws > INT_MAX ? INT_MAX : (int)a.ws;
    return T4K_OK;
}

int t4k_retention_fwd(const float *QKV, float *O, float *ST, int N, int L, int heads, int d, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!QKV || !O || !ST) return fail(T4K_ERR_ARG, "t4k_retention_fwd: null tensor");
    RtPlan a;
    const int rc = retn_plan(a, "t4k_retention_fwd", N, L, heads, d, all16(QKV, O, ST), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const RtP p = retn_parms(a, N, L, heads, d);
    hipStream_t hs = t4k::S(s);
    const unsigned nh = (unsigned)(N * heads), scan = (unsigned)(nh * (((long)d * d + 63) / 64));
    pick<16, 32, 64, 128>(a.dp, [&](auto dp) {
        pick<4, 1>(a.vw, [&](auto vw) {
            constexpr int DP = decltype(dp)::value, VW = decltype(vw)::value;
            if (a.chunks > 1) {
                T4K_LAUNCH((k_retn_state<DP, VW, false>), dim3(nh * (unsigned)(a.chunks - 1)), dim3(256), 0, hs, QKV, (const float *)nullptr, ST, p);
                T4K_LAUNCH(k_retn_scan, dim3(scan), dim3(64), 0, hs, ST, p, a.b, 0);
            }
            T4K_LAUNCH((k_retn_out<DP, VW>), dim3((unsigned)a.wgs), dim3(256), 0, hs, QKV, O, (const float *)ST, p);
        });
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_retention_bwd(const float *QKV, const float *DY, const float *ST, float *DQKV, int N, int L, int heads, int d, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!QKV || !DY || !ST || !DQKV) return fail(T4K_ERR_ARG, "t4k_retention_bwd: null tensor");
    RtPlan a;
    const int rc = retn_plan(a, "t4k_retention_bwd", N, L, heads, d, all16(QKV, DY, ST, DQKV), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long ne = (long)N * L * heads * d;
    if (clash(DQKV, 3 * ne, QKV, 3 * ne) || clash(DQKV, 3 * ne, DY, ne) || clash(DQKV, 3 * ne, ST, (long)N * heads * a.chunks * d * d))
        return fail(T4K_ERR_ARG, "t4k_retention_bwd: DQKV overlaps QKV, DY or ST");
    const RtP p = retn_parms(a, N, L, heads, d);
    hipStream_t hs = t4k::S(s);
    float *ws = ws_for(s);
    const unsigned nh = (unsigned)(N * heads), scan = (unsigned)(nh * (((long)d * d + 63) / 64));
    pick<16, 32, 64, 128>(a.dp, [&](auto dp) {
        pick<4, 1>(a.vw, [&](auto vw) {
            constexpr int DP = decltype(dp)::value, VW = decltype(vw)::value;
            if (a.chunks > 1) {
                T4K_LAUNCH((k_retn_state<DP, VW, true>), dim3(nh * (unsigned)(a.chunks - 1)), dim3(256), 0, hs, QKV, DY, ws, p);
                T4K_LAUNCH(k_retn_scan, dim3(scan), dim3(64), 0, hs, ws, p, a.b, 1);
            }
            T4K_LAUNCH((k_retn_grad<DP, VW>), dim3((unsigned)a.wgs), dim3(256), 0, hs, QKV, DY, ST, (const float *)ws, DQKV, p);
        });
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
