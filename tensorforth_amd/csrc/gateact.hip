// gateact.hip - the smooth and gated feed-forward activations on NHWC fp32 tokens: GELU, tanh-GELU, SiLU, Mish, and their gated forms
// (GeGLU, SwiGLU).  X is [T, C], T = N H W tokens.  kind picks f:
//   0  a Phi(a), Phi(a) = (1 + erf(a / sqrt 2)) / 2          1  a s(2 u), u = sqrt(2 / pi) (a + 0.044715 a^3)  (= a (1 + tanh u) / 2)
//   2  a s(a),   s the logistic function                       3  a tanh(softplus(a))
//   gate 0: Y [T, C]  = f(X);                       dX = dY f'(X)
//   gate 1: Y [T, Hc] = f(A) B, X = [ A | B ] per token, Hc = C / 2;   dA = dY B f'(A), dB = dY f(A), stored where A and B were.
// Nothing is kept between the passes: the backward forms f' from x again.  The reference has no such layer.
// Work split: an ITEM is VW consecutive channels (16 bytes, or a dword).  gate 0 - the tensor is one flat span of T C / VW items.  gate 1 - an item is VW
// channels of the OUTPUT; item i of token t belongs to one lane, which loads item i of A and item i of B of that token - two requests in which
// consecutive lanes read consecutive addresses - and in the backward stores dA and dB to the addresses it loaded.  No other lane touches those
// addresses, so DX may be X itself: a store's value depends only on loads of the same addresses by the same lane (k_tc_jbwd's argument, token_ce.hip).
// A lane has GA_UN items in flight: every load of a workgroup's chunk is issued before the first arithmetic.  An item's token is a multiply-shift
// division (fastdiv.h).  No LDS, no atomics, no reduction: the same bits on every call.  kind, gate and the load path are template arguments.
// Finite for every finite input: every exponential is taken of a non-positive argument, q = exp(-|z|) in (0, 1], and the two signs of z select between
// expressions in q that are exact images of each other (s(z) = 1 / (1 + q) or q / (1 + q)), so nothing overflows and no inf - inf or 0 inf arises.  In
// the tail where f' itself is about to leave the float range, q is formed as h h with h = exp(-|z| / 2) and the factors are multiplied h first, h last:
// the product underflows where f' does, not where q does.
#include "t4k_common.h"
#include "launch.h"
#include "fastdiv.h"

using namespace t4k;

namespace {

constexpr int GA_BLK = 256;             // the workgroup: four waves
constexpr int GA_UN  = 4;               // items a lane has in flight (forward: 4 | 8 loads of 16 bytes before the first arithmetic; backward 8 | 12)

struct GaP { long items; int C, Hc, ipt; FastDiv di; };     // ipt: items of a token's output row (gate 1)

__device__ __forceinline__ float ga_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// ------------------------------------------------------------------ the functions.  ga_f: f(a).  ga_fd: f(a) and f'(a) (the caller that wants one of them
// leaves the other unused, and its arithmetic is dropped)
constexpr float GA_K0 = 0.7978845608028654f, GA_K1 = 0.044715f;      // sqrt(2 / pi), the cubic's coefficient
constexpr float GA_RSQRT2 = 0.7071067811865476f, GA_RSQRT2PI = 0.3989422804014327f;
// the polynomial factors of f' are formed from a clamped argument: beyond the clamp q is 0 (kind 1: |2 u| > 317 from |a| = 16; kinds 2 and 3: exp(-256)), so the
// factor multiplies a zero either way - with the clamp it is a modest float, without it the cubic's derivative is inf (0 inf) and a (1 + ulp) leaves the range
constexpr float GA_TANH_CLAMP = 16.0f, GA_EXP_CLAMP = 256.0f;

// z and dz/da of the logistic kinds: kind 1 z = 2 u(a), kind 2 z = a.  ac: the argument the derivative's polynomial factors are formed from
template <int KIND> __device__ __forceinline__ void ga_logit(float a, float &z, float &c, float &ac) {
    if constexpr (KIND == 1) {
        ac = fminf(fmaxf(a, -GA_TANH_CLAMP), GA_TANH_CLAMP);
        const float p = ac * ac;
        z = (2.0f * GA_K0 * ac) * fmaf(GA_K1, p, 1.0f);
        c = 2.0f * GA_K0 * fmaf(3.0f * GA_K1, p, 1.0f);
    } else { ac = fminf(fmaxf(a, -GA_EXP_CLAMP), GA_EXP_CLAMP); z = a; c = 1.0f; }
}

template <int KIND> __device__ __forceinline__ float ga_f(float a) {
    if constexpr (KIND == 0) return (0.5f * a) * (1.0f + erff(a * GA_RSQRT2));
    else if constexpr (KIND == 3) {
        // tanh(softplus a) = n / (n + 2), n = e (e + 2), e = exp(a); for a >= 0 the same ratio in q = 1 / e: (1 + 2 q) / (1 + 2 q + 2 q q)
        const bool neg = a < 0.0f;
        const float q = __expf(-fabsf(a));
        const float num = fmaf(2.0f, q, neg ? q * q : 1.0f), den = num + (neg ? 2.0f : 2.0f * q * q);
        return a * (num * ga_rcp(den));
    } else {
        float z, c, ac; ga_logit<KIND>(a, z, c, ac);
        const float q = __expf(-fabsf(z)), r = ga_rcp(1.0f + q);
        return a * (z < 0.0f ? q * r : r);
    }
}

template <int KIND> __device__ __forceinline__ void ga_fd(float a, float &f, float &d) {
    if constexpr (KIND == 0) {
        // Phi from erfc: accurate to the end of the negative tail, where 1 + erf has no bits left; a phi(a) as (a h) h, h = exp(-a a / 4)
        const float Phi = 0.5f * erfcf(-a * GA_RSQRT2);
        const float h = __expf(-0.25f * (a * a));                  // (a a = inf: exp(-inf) = 0)
        f = a * Phi;
        d = Phi + ((a * h) * GA_RSQRT2PI) * h;
    } else if constexpr (KIND == 3) {
        // t = num / den as in ga_f; 1 - t t = e2 (den + num) / den^2 with e2 = den - num EXACTLY (2, or 2 q q); softplus' = 1 / (1 + q) or q / (1 + q).
        // a < 0: every term carries a factor q = h h, taken out: f' = (h G) h
        const bool neg = a < 0.0f;
        const float h = __expf(-0.5f * fabsf(a)), q = h * h;
        const float num = fmaf(2.0f, q, neg ? q * q : 1.0f), den = num + (neg ? 2.0f : 2.0f * q * q);
        const float rden = ga_rcp(den);
        f = a * (num * rden);
        const float a1 = neg ? q + 2.0f : num;                     // num, less its factor q where a < 0
        const float ea = neg ? fmaxf(a, -GA_EXP_CLAMP) : (a * q) * q;                    // a e2 softplus' (1 + q) / 2, less the same factor
        const float w2 = (2.0f * (den + num)) * ga_rcp((den * den) * (1.0f + q));      // (at most 1: a w2 stays a float at the ends of the range)
        const float G = fmaf(ea, w2, a1 * rden);
        d = neg ? (h * G) * h : G;
    } else {
        // s = s(z): z >= 0: s = r, 1 - s = q r; z < 0: s = q r, 1 - s = r, r = 1 / (1 + q).  f' = s + a s (1 - s) c = [q] r (1 + a c (1 - s))
        float z, c, ac; ga_logit<KIND>(a, z, c, ac);
        const bool neg = z < 0.0f;
        const float h = __expf(-0.5f * fabsf(z)), q = h * h, r = ga_rcp(1.0f + q);
        f = a * (neg ? q * r : r);
        const float G = r * fmaf(ac * c, neg ? r : q * r, 1.0f);
        d = neg ? (h * G) * h : G;
    }
}

// where item f lives: the offset of its A (or only) operand in X and of its output in Y
template <int GATE, int VW> __device__ __forceinline__ void ga_at(const GaP &p, long f, long &ox, long &oy) {
    if constexpr (GATE) {
        const unsigned t = fdiv((unsigned)f, p.di), c = (unsigned)f - t * (unsigned)p.ipt;      // (items below 2^31: the plan's admission)
        ox = (long)t * p.C + (long)c * VW; oy = f * VW;
    } else ox = oy = f * VW;
}

// ------------------------------------------------------------------ forward: Y = f(X) | f(A) B.  Plain stores: the next layer reads Y
template <int KIND, int GATE, int VW>
__global__ void __launch_bounds__(GA_BLK) k_ga_fwd(const float *__restrict__ X, float *__restrict__ Y, GaP p) {
    const long f0 = (long)blockIdx.x * (GA_BLK * GA_UN) + threadIdx.x;
    float a[GA_UN][VW], b[GA_UN][VW]; long oy[GA_UN];
#pragma unroll
    for (int u = 0; u < GA_UN; u++) {
        const long f = f0 + u * GA_BLK;
        if (f < p.items) {
            long ox; ga_at<GATE, VW>(p, f, ox, oy[u]);
            ldv<VW>(X + ox, a[u]);
            if constexpr (GATE) ldv<VW>(X + ox + p.Hc, b[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < GA_UN; u++) {
        if (f0 + u * GA_BLK < p.items) {
#pragma unroll
            for (int q = 0; q < VW; q++) { a[u][q] = ga_f<KIND>(a[u][q]); if constexpr (GATE) a[u][q] *= b[u][q]; }
            stv<VW>(Y + oy[u], a[u]);
        }
    }
}

// ------------------------------------------------------------------ backward: DX = DY f'(X) | (DY B f'(A), DY f(A)).  DX may be X (neither is __restrict__): a
// lane stores to the addresses it loaded, after every load of its chunk.  Nontemporal stores: measured against plain ones they take 0.85 of the time
// where DX is a tensor of its own and the row exceeds the last-level cache, and the same time over X and on the rows that fit
typedef float ga_v4f __attribute__((ext_vector_type(4)));
template <int VW> __device__ __forceinline__ void ga_stnt(float *q, const float (&v)[VW]) {
    if constexpr (VW == 4) __builtin_nontemporal_store(ga_v4f{v[0], v[1], v[2], v[3]}, reinterpret_cast<ga_v4f *>(q));
    else __builtin_nontemporal_store(v[0], q);
}
template <int KIND, int GATE, int VW>
__global__ void __launch_bounds__(GA_BLK) k_ga_bwd(const float *X, const float *__restrict__ DY, float *DX, GaP p) {
    const long f0 = (long)blockIdx.x * (GA_BLK * GA_UN) + threadIdx.x;
    float a[GA_UN][VW], b[GA_UN][VW], g[GA_UN][VW]; long ox[GA_UN];
#pragma unroll
    for (int u = 0; u < GA_UN; u++) {
        const long f = f0 + u * GA_BLK;
        if (f < p.items) {
            long oy; ga_at<GATE, VW>(p, f, ox[u], oy);
            ldv<VW>(X + ox[u], a[u]);
            if constexpr (GATE) ldv<VW>(X + ox[u] + p.Hc, b[u]);
            ldv<VW>(DY + oy, g[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < GA_UN; u++) {
        if (f0 + u * GA_BLK < p.items) {
#pragma unroll
            for (int q = 0; q < VW; q++) {
                float f, d; ga_fd<KIND>(a[u][q], f, d);
                if constexpr (GATE) { a[u][q] = (g[u][q] * b[u][q]) * d; b[u][q] = g[u][q] * f; }
                else a[u][q] = g[u][q] * d;
            }
            ga_stnt<VW>(DX + ox[u], a[u]);
            if constexpr (GATE) ga_stnt<VW>(DX + ox[u] + p.Hc, b[u]);
        }
    }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_gateact_plan reports
struct GaPlan { int rung, vw, grid; GaP p; };
// admission (who: the entry's name for the message) in 64 bits, a function of its arguments only.  o is written on T4K_OK alone
int ga_plan(GaPlan &o, const char *who, long T, long C, int kind, int gate, bool aligned) {
    if (T < 1 || C < 1) return fail(T4K_ERR_ARG, "%s: T=%ld or C=%ld below 1", who, T, C);
    if (kind < 0 || kind > 3) return fail(T4K_ERR_ARG, "%s: kind=%d outside 0..3", who, kind);
    if (gate < 0 || gate > 1) return fail(T4K_ERR_ARG, "%s: gate=%d outside 0..1", who, gate);
    if (gate && C % 2) return fail(T4K_ERR_ARG, "%s: gate=1 halves the channels, C=%ld is odd", who, C);
    if (T >= (1L << 31) || C >= (1L << 31) || T * C >= (1L << 31)) return fail(T4K_ERR_UNSUPPORTED, "%s: T C = %ld x %ld at or above 2^31", who, T, C);
    GaPlan g;
    const long Hc = gate ? C / 2 : C, n = T * Hc;            // output elements
    // 16 bytes a lane: gate 0 - the flat span in whole items; gate 1 - Hc floats keep B's rows, and every token's, on 16 bytes
    g.vw = (aligned && (gate ? Hc : n) % 4 == 0) ? 4 : 1;
    g.rung = gate * 2 + (g.vw == 1 ? 1 : 0);
    g.p.items = n / g.vw; g.p.C = (int)C; g.p.Hc = (int)Hc; g.p.ipt = (int)(Hc / g.vw); g.p.di = fast_div(g.p.ipt);
    g.grid = (int)ceil_div(g.p.items, (long)GA_BLK * GA_UN);
    o = g; return T4K_OK;
}

template <int GATE, int VW, typename... A> void ga_launch_fwd(int kind, dim3 grid, hipStream_t hs, A... a) {
    switch (kind) {
    case 0: T4K_LAUNCH((k_ga_fwd<0, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    case 1: T4K_LAUNCH((k_ga_fwd<1, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    case 2: T4K_LAUNCH((k_ga_fwd<2, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    default: T4K_LAUNCH((k_ga_fwd<3, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    }
}
template <int GATE, int VW, typename... A> void ga_launch_bwd(int kind, dim3 grid, hipStream_t hs, A... a) {
    switch (kind) {
    case 0: T4K_LAUNCH((k_ga_bwd<0, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    case 1: T4K_LAUNCH((k_ga_bwd<1, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    case 2: T4K_LAUNCH((k_ga_bwd<2, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    default: T4K_LAUNCH((k_ga_bwd<3, GATE, VW>), grid, dim3(GA_BLK), 0, hs, a...); break;
    }
}

} // namespace

extern "C" {

int t4k_gateact_plan(long T, int C, int kind, int gate, int aligned, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_gateact_plan: null");
    GaPlan g;
    const int rc = ga_plan(g, "t4k_gateact_plan", T, C, kind, gate, aligned != 0); if (rc != T4K_OK) return rc;
    out[0] = g.rung; out[1] = g.vw; out[2] = GA_UN; out[3] = g.grid; out[4] = g.grid; out[5] = 1; out[6] = 1; out[7] = 0;
    return T4K_OK;
}

int t4k_gateact_fwd(const float *X, float *Y, long T, int C, int kind, int gate, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !Y) return fail(T4K_ERR_ARG, "t4k_gateact_fwd: null");
    GaPlan g;
    const int rc = ga_plan(g, "t4k_gateact_fwd", T, C, kind, gate, all16(X, Y)); if (rc != T4K_OK) return rc;
    if (clash(Y, T * g.p.Hc, X, T * C)) return fail(T4K_ERR_ARG, "t4k_gateact_fwd: Y overlaps X");
    hipStream_t hs = t4k::S(s);
    const dim3 grid((unsigned)g.grid);
    if (gate)  { if (g.vw == 4) ga_launch_fwd<1, 4>(kind, grid, hs, X, Y, g.p); else ga_launch_fwd<1, 1>(kind, grid, hs, X, Y, g.p); }
    else       { if (g.vw == 4) ga_launch_fwd<0, 4>(kind, grid, hs, X, Y, g.p); else ga_launch_fwd<0, 1>(kind, grid, hs, X, Y, g.p); }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_gateact_bwd(const float *X, const float *DY, float *DX, long T, int C, int kind, int gate, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !DY || !DX) return fail(T4K_ERR_ARG, "t4k_gateact_bwd: null");
    GaPlan g;
    const int rc = ga_plan(g, "t4k_gateact_bwd", T, C, kind, gate, all16(X, DY, DX)); if (rc != T4K_OK) return rc;
    const long n = T * C, no = T * g.p.Hc;
    if (clash(DX, n, X, n, true) || clash(DX, n, DY, no) || clash(X, n, DY, no))
        return fail(T4K_ERR_ARG, "t4k_gateact_bwd: operands overlap (DX may be X itself, nothing else)");
    hipStream_t hs = t4k::S(s);
    const dim3 grid((unsigned)g.grid);
    if (gate)  { if (g.vw == 4) ga_launch_bwd<1, 4>(kind, grid, hs, X, DY, DX, g.p); else ga_launch_bwd<1, 1>(kind, grid, hs, X, DY, DX, g.p); }
    else       { if (g.vw == 4) ga_launch_bwd<0, 4>(kind, grid, hs, X, DY, DX, g.p); else ga_launch_bwd<0, 1>(kind, grid, hs, X, DY, DX, g.p); }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
