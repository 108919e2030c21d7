// token_ce.hip - the per-token softmax and cross-entropy head on NHWC fp32 tokens: T = N H W rows of V contiguous logits.
//   m_t = max_c x[t,c]   s_t = sum_c exp(x[t,c] - m_t)   lse_t = m_t + ln s_t   P[t,c] = exp(x[t,c] - m_t) / s_t   amax_t = the smallest c with x[t,c] == m_t
//   STAT[t] = (lse_t, (float)amax_t).  Targets are ids as floats, one per token: valid <=> 0 <= id < V in float compares, k_t = (int)id (token_id of
//   t4k_common.h, the rule of embed.hip); a token that is not valid is padding - no loss term, no hit, a zero gradient row.  The reference has no such layer.
// Rows run from 2 floats to tens of thousands, so the forward and the Jacobian backward have three rungs over one row structure.  An ITEM is what a lane
// loads at a time (16 bytes or a dword), a row has V / width items, a lane keeps up to TC_NV of them in registers, item it0 + i * team of the row in slot i:
//   rung 0  a TEAM of 2^k lanes of a wave owns a token (the power of two that leaves a lane at most TC_IPL items, at most a wave), 64 / team tokens of the
//           wave in flight at a time; the row is read once into registers; max | first arg-max and the sum fold over the team on the vector ALUs
//           (lane_ops.h: DPP inside a row of 16 lanes, lane swaps across).  Up to 64 TC_NV items.
//   rung 1  the workgroup is the team: the four waves fold as on rung 0 and meet in LDS.  Up to 256 TC_NV items.
//   rung 2  beyond the register budget: the workgroup walks the row twice in one launch.  Pass 1 keeps a running (max, sum, arg-max) per lane, rescaled once
//           per chunk of TC_NV loads (softmax_axes.hip's regime 1), folded once; pass 2 reads the row again - from L2, where a 200 KB row sits - and stores.
// The arg-max is a fold over (value, index), the smaller index winning ties (lane_argmax_take), inside a lane, over the team and over the waves: the first
// maximum whichever lanes held the copies.  STAT is stored once per token by the team's first lane.  A lane stores exactly the items it loaded, so the
// Jacobian backward may write DX over X: a store's value depends on the load of the same address by the same lane, and no other lane reads that address.
// CE backward: a wave takes a batch of up to 64 consecutive tokens, lane i reads token i's id once, and the batch's rows - one contiguous span of P - are
// streamed flat, 64 items a step; an item's token is a multiply-shift division (fastdiv.h), its k a lane exchange, the one-hot a compare on the column.  A
// padding row is stored as zeros without its P being loaded.  8 bytes an element, no third [T, V] operand.
// Score: a thread a token gathers P[t, k_t] and the stored arg-max; loss, hits and valid count fold per workgroup, and a one-workgroup launch folds the
// workgroups' partial records (left in the stream's workspace) in order.  Fixed trees everywhere, no atomics: the same bits on every call.
#include "t4k_common.h"
#include "launch.h"
#include "fastdiv.h"
#include "lane_ops.h"

using namespace t4k;

namespace {

constexpr int TC_BLK  = 256;            // the workgroup: four waves, one per SIMD
constexpr int TC_NV   = 8;              // items a lane keeps in registers (32 VGPRs on the 16-byte path; the Jacobian backward holds x and dY: 64)
constexpr int TC_IPL  = 4;              // items a lane of a sub-wave team takes at most: short rows keep several tokens of a wave in flight
constexpr int TC_WG   = 2048;           // workgroups a launch spreads over at most (256 CUs x 8 resident)
constexpr int TC_CEW  = 8192;           // wave batches the CE backward aims at before a batch grows beyond one token (256 CUs x 4 SIMDs x 8)
constexpr int TC_UN   = 4;              // CE backward: items a lane has in flight
constexpr int TC_SWG  = 256;            // score: workgroups at most - their partial records are folded by one workgroup, a thread a record
constexpr int TC_NONE = 0x7fffffff;     // the index of no element (lane_ops.h's convention for the arg-max forms)

struct TcP { long T; int V, items, tl, tsh, G; };
struct TcC { long T; int V, items, wb; float fV; FastDiv di; };

// ------------------------------------------------------------------ team folds.  CALLED FROM UNIFORM CODE WITH ALL 64 LANES LIVE (lane_ops.h): a token
// beyond T or an item beyond the row is filled (-inf, TC_NONE, 0), never branched around
template <int OFF> __device__ __forceinline__ unsigned tc_from(unsigned v) {                  // the value lane i ^ OFF holds
    if constexpr (OFF >= 16) return lane_swap_partner(lane_swap<OFF>(v), v);
    else return lane_dpp_xor<OFF>(v);
}
template <int OFF> __device__ __forceinline__ void tc_sum_step(float &a, int tl) { if (tl > OFF) a += __builtin_bit_cast(float, tc_from<OFF>(__builtin_bit_cast(unsigned, a))); }
template <int OFF> __device__ __forceinline__ void tc_isum_step(int &a) { a += (int)tc_from<OFF>((unsigned)a); }
template <int OFF> __device__ __forceinline__ void tc_amax_step(float &m, int &i, int tl) {
    if (tl > OFF) lane_argmax_take(m, i, __builtin_bit_cast(float, tc_from<OFF>(__builtin_bit_cast(unsigned, m))), (int)tc_from<OFF>((unsigned)i));
}
// the sum over a team of tl lanes (tl a power of two, uniform over the launch), every lane of the team; WG: the workgroup is the team, the waves meet in sm
template <bool WG> __device__ __forceinline__ float tc_sum(float a, int tl, float *sm) {
    tc_sum_step<32>(a, tl); tc_sum_step<16>(a, tl); tc_sum_step<8>(a, tl); tc_sum_step<4>(a, tl); tc_sum_step<2>(a, tl); tc_sum_step<1>(a, tl);
    if constexpr (WG) {
        if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
        __syncthreads();
        a = (sm[0] + sm[1]) + (sm[2] + sm[3]);
        __syncthreads();
    }
    return a;
}
__device__ __forceinline__ int tc_isum_wg(int a, int *smi) {
    tc_isum_step<32>(a); tc_isum_step<16>(a); tc_isum_step<8>(a); tc_isum_step<4>(a); tc_isum_step<2>(a); tc_isum_step<1>(a);
    if ((threadIdx.x & 63) == 0) smi[threadIdx.x >> 6] = a;
    __syncthreads();
    a = (smi[0] + smi[1]) + (smi[2] + smi[3]);
    __syncthreads();
    return a;
}
// (m, i) <- the team's largest m and the lowest index among the elements that hold it
template <bool WG> __device__ __forceinline__ void tc_amax(float &m, int &i, int tl, float *sm, int *smi) {
    tc_amax_step<32>(m, i, tl); tc_amax_step<16>(m, i, tl); tc_amax_step<8>(m, i, tl); tc_amax_step<4>(m, i, tl); tc_amax_step<2>(m, i, tl); tc_amax_step<1>(m, i, tl);
    if constexpr (WG) {
        if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = m; smi[threadIdx.x >> 6] = i; }
        __syncthreads();
        m = sm[0]; i = smi[0];
#pragma unroll
        for (int k = 1; k < 4; k++) lane_argmax_take(m, i, sm[k], smi[k]);
        __syncthreads();
    }
}
template <int VW> __device__ __forceinline__ float tc_add(const float (&a)[VW]) {            // a lane's VW column sums, one tree
    if constexpr (VW == 4) return (a[0] + a[1]) + (a[2] + a[3]); else return a[0];
}
// where a lane of a register rung stands: RUNG 0 - wave batch b holds G tokens, the lane's team the token b G + (lane >> tsh); RUNG 1 - token b, the
// workgroup.  The loop bounds are uniform over the wave (rung 0, which has no barrier) or over the workgroup (rung 1)
template <int RUNG> struct TcAt {
    int it0, step; long nb, b0, bs;
    __device__ __forceinline__ TcAt(const TcP &p) {
        const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
        if (RUNG) { it0 = (int)threadIdx.x; step = TC_BLK; nb = p.T; b0 = blockIdx.x; bs = gridDim.x; }
        else { it0 = lane & (p.tl - 1); step = p.tl; nb = (p.T + p.G - 1) / p.G; b0 = (long)blockIdx.x * 4 + w; bs = (long)gridDim.x * 4; }
    }
    __device__ __forceinline__ long token(const TcP &p, long b) const { return RUNG ? b : b * p.G + (((int)threadIdx.x & 63) >> p.tsh); }
};

// ------------------------------------------------------------------ forward, rungs 0 and 1: the row in registers, read once
template <int VW, int RUNG>
__global__ void __launch_bounds__(TC_BLK) k_tc_fwd(const float *__restrict__ X, float *__restrict__ P, float *__restrict__ STAT, TcP p) {
    __shared__ float sm[4]; __shared__ int smi[4];
    const TcAt<RUNG> at(p);
    for (long b = at.b0; b < at.nb; b += at.bs) {
        const long t = at.token(p, b);
        const bool live = t < p.T;
        const float *x = X + t * p.V;
        float v[TC_NV][VW], m = -FLT_MAX; int am = TC_NONE;
#pragma unroll
        for (int i = 0; i < TC_NV; i++) {
            const int it = at.it0 + i * at.step;
#pragma unroll
            for (int q = 0; q < VW; q++) v[i][q] = -INFINITY;
            if (live && it < p.items) {
                ldv<VW>(x + it * VW, v[i]);
#pragma unroll
                for (int q = 0; q < VW; q++) lane_argmax_take(m, am, v[i][q], it * VW + q);
            }
        }
        tc_amax<RUNG != 0>(m, am, p.tl, sm, smi);
        float a[VW];
#pragma unroll
        for (int q = 0; q < VW; q++) a[q] = 0.0f;
#pragma unroll
        for (int i = 0; i < TC_NV; i++) {
#pragma unroll
            for (int q = 0; q < VW; q++) { v[i][q] = __expf(v[i][q] - m); a[q] += v[i][q]; }      // a slot that holds no element: exp(-inf) = +0
        }
        const float s = tc_sum<RUNG != 0>(tc_add<VW>(a), p.tl, sm);
        if (!live) continue;                                                     // (past the folds: every lane took them)
        float *o = P + t * p.V;
#pragma unroll
        for (int i = 0; i < TC_NV; i++) {
            const int it = at.it0 + i * at.step;
            if (it < p.items) {
#pragma unroll
                for (int q = 0; q < VW; q++) v[i][q] = v[i][q] / s;
                stv<VW>(o + it * VW, v[i]);
            }
        }
        if (at.it0 == 0) { STAT[2 * t] = m + __logf(s); STAT[2 * t + 1] = (float)am; }
    }
}

// forward, rung 2: a token a workgroup, two passes.  Item c * 256 TC_NV + i * 256 + thread of the row is slot i of the thread's chunk c
template <int VW>
__global__ void __launch_bounds__(TC_BLK) k_tc_fwd2(const float *__restrict__ X, float *__restrict__ P, float *__restrict__ STAT, TcP p) {
    __shared__ float sm[4]; __shared__ int smi[4];
    for (long t = blockIdx.x; t < p.T; t += gridDim.x) {                         // (uniform over the workgroup)
        const float *x = X + t * p.V;
        float m = -FLT_MAX, sum = 0.0f; int am = TC_NONE;
        for (int c0 = (int)threadIdx.x; c0 < p.items; c0 += TC_BLK * TC_NV) {     // pass 1 (no barrier inside: the last chunk is not every thread's)
            float v[TC_NV][VW], cm = m; int ca = am;
#pragma unroll
            for (int i = 0; i < TC_NV; i++) {
                const int it = c0 + i * TC_BLK;
#pragma unroll
                for (int q = 0; q < VW; q++) v[i][q] = -INFINITY;
                if (it < p.items) {
                    ldv<VW>(x + it * VW, v[i]);
#pragma unroll
                    for (int q = 0; q < VW; q++) lane_argmax_take(cm, ca, v[i][q], it * VW + q);
                }
            }
            float a[VW];
#pragma unroll
            for (int q = 0; q < VW; q++) a[q] = 0.0f;
#pragma unroll
            for (int i = 0; i < TC_NV; i++) {
#pragma unroll
                for (int q = 0; q < VW; q++) a[q] += __expf(v[i][q] - cm);
            }
            sum = sum * __expf(m - cm) + tc_add<VW>(a); m = cm; am = ca;          // one rescale a chunk (m = -FLT_MAX at first: 0 x 0)
        }
        float mg = m;
        tc_amax<true>(mg, am, TC_BLK, sm, smi);
        const float s = tc_sum<true>(sum * __expf(m - mg), TC_BLK, sm);          // ... and one from the lane to the workgroup
        float *o = P + t * p.V;
        for (int c0 = (int)threadIdx.x; c0 < p.items; c0 += TC_BLK * TC_NV) {     // pass 2
            float v[TC_NV][VW];
#pragma unroll
            for (int i = 0; i < TC_NV; i++) if (c0 + i * TC_BLK < p.items) ldv<VW>(x + (c0 + i * TC_BLK) * VW, v[i]);
#pragma unroll
            for (int i = 0; i < TC_NV; i++) {
                if (c0 + i * TC_BLK < p.items) {
#pragma unroll
                    for (int q = 0; q < VW; q++) v[i][q] = __expf(v[i][q] - mg) / s;
                    stv<VW>(o + (c0 + i * TC_BLK) * VW, v[i]);
                }
            }
        }
        if (threadIdx.x == 0) { STAT[2 * t] = mg + __logf(s); STAT[2 * t + 1] = (float)am; }
    }
}

// ------------------------------------------------------------------ Jacobian backward: p = exp(x - lse), g = sum_c dY p, DX = p (dY - g).  DX may be X (not
// __restrict__): a lane stores the items it loaded, each store's value comes from that load
template <int VW, int RUNG>
__global__ void __launch_bounds__(TC_BLK) k_tc_jbwd(const float *X, const float *__restrict__ STAT, const float *__restrict__ DY, float *DX, TcP p) {
    __shared__ float sm[4];
    const TcAt<RUNG> at(p);
    for (long b = at.b0; b < at.nb; b += at.bs) {
        const long t = at.token(p, b);
        const bool live = t < p.T;
        const float *x = X + t * p.V, *dy = DY + t * p.V;
        const float lse = live ? STAT[2 * t] : 0.0f;
        float v[TC_NV][VW], d[TC_NV][VW];
#pragma unroll
        for (int i = 0; i < TC_NV; i++) {
            const int it = at.it0 + i * at.step;
#pragma unroll
            for (int q = 0; q < VW; q++) { v[i][q] = -INFINITY; d[i][q] = 0.0f; }
            if (live && it < p.items) { ldv<VW>(x + it * VW, v[i]); ldv<VW>(dy + it * VW, d[i]); }
        }
        float a[VW];
#pragma unroll
        for (int q = 0; q < VW; q++) a[q] = 0.0f;
#pragma unroll
        for (int i = 0; i < TC_NV; i++) {
#pragma unroll
            for (int q = 0; q < VW; q++) { v[i][q] = __expf(v[i][q] - lse); a[q] += d[i][q] * v[i][q]; }
        }
        const float g = tc_sum<RUNG != 0>(tc_add<VW>(a), p.tl, sm);
        if (!live) continue;
        float *o = DX + t * p.V;
#pragma unroll
        for (int i = 0; i < TC_NV; i++) {
            const int it = at.it0 + i * at.step;
            if (it < p.items) {
#pragma unroll
                for (int q = 0; q < VW; q++) v[i][q] = v[i][q] * (d[i][q] - g);
                stv<VW>(o + it * VW, v[i]);
            }
        }
    }
}
// rung 2: pass 1 folds the dot, the barrier of the fold ends it for the whole workgroup, pass 2 forms p again and stores
template <int VW>
__global__ void __launch_bounds__(TC_BLK) k_tc_jbwd2(const float *X, const float *__restrict__ STAT, const float *__restrict__ DY, float *DX, TcP p) {
    __shared__ float sm[4];
    for (long t = blockIdx.x; t < p.T; t += gridDim.x) {
        const float *x = X + t * p.V, *dy = DY + t * p.V;
        float *o = DX + t * p.V;
        const float lse = STAT[2 * t];
        float a[VW];
#pragma unroll
        for (int q = 0; q < VW; q++) a[q] = 0.0f;
        for (int pass = 0; pass < 2; pass++) {
            float g = 0.0f;
            if (pass) g = tc_sum<true>(tc_add<VW>(a), TC_BLK, sm);
            for (int c0 = (int)threadIdx.x; c0 < p.items; c0 += TC_BLK * TC_NV) {
                float v[TC_NV][VW], d[TC_NV][VW];
#pragma unroll
                for (int i = 0; i < TC_NV; i++) if (c0 + i * TC_BLK < p.items) { ldv<VW>(x + (c0 + i * TC_BLK) * VW, v[i]); ldv<VW>(dy + (c0 + i * TC_BLK) * VW, d[i]); }
#pragma unroll
                for (int i = 0; i < TC_NV; i++) {
                    if (c0 + i * TC_BLK < p.items) {
#pragma unroll
                        for (int q = 0; q < VW; q++) {
                            const float e = __expf(v[i][q] - lse);
                            if (pass) v[i][q] = e * (d[i][q] - g); else a[q] += d[i][q] * e;
                        }
                        if (pass) stv<VW>(o + (c0 + i * TC_BLK) * VW, v[i]);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------ CE backward: DX[t, c] = valid(t) ? P[t, c] - (c == k_t) : 0
template <int VW>
__global__ void __launch_bounds__(TC_BLK) k_tc_ce_bwd(const float *__restrict__ Pm, const float *__restrict__ IDS, float *__restrict__ DX, TcC p) {
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const long nb = (p.T + p.wb - 1) / p.wb;
    for (long b = (long)blockIdx.x * 4 + w; b < nb; b += (long)gridDim.x * 4) {    // (uniform over the wave; no barrier)
        const long t0 = b * p.wb;
        const int nt = (int)min((long)p.wb, p.T - t0), n = nt * p.items;          // the batch's span: nt rows, n items (wb items <= 64 x 2^24)
        int k = -1;
        if (lane < nt) k = token_id(IDS[t0 + lane], p.fV, p.V);                   // lane i reads token i's id, once
        const float *src = Pm + t0 * p.V; float *dst = DX + t0 * p.V;
        for (int f0 = 0; f0 < n; f0 += 64 * TC_UN) {                             // (uniform)
            float v[TC_UN][VW]; int kc[TC_UN];
#pragma unroll
            for (int u = 0; u < TC_UN; u++) {
                const int f = f0 + u * 64 + lane;
                const int j = f < n ? (int)fdiv((unsigned)f, p.di) : 0;           // the item's token of the batch, its column below
                const int kj = __shfl(k, j, 64);
                kc[u] = kj < 0 ? -1 : kj - (f - j * p.items) * VW;                // where in the item the 1 falls (outside 0 .. VW - 1: nowhere)
#pragma unroll
                for (int q = 0; q < VW; q++) v[u][q] = 0.0f;
                if (f < n && kj >= 0) ldv<VW>(src + (long)f * VW, v[u]);          // a padding row is not loaded
            }
#pragma unroll
            for (int u = 0; u < TC_UN; u++) {
                const int f = f0 + u * 64 + lane;
                if (f < n) {
#pragma unroll
                    for (int q = 0; q < VW; q++) if (kc[u] == q) v[u][q] -= 1.0f;
                    stv<VW>(dst + (long)f * VW, v[u]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------ score: REC = (float sum of nll, int hits, int valid tokens), three 32-bit words
struct TcRec { float nll; int hit, val; };
__device__ __forceinline__ void tc_rec_fold(TcRec &r, float *sm, int *smi) {
    r.nll = tc_sum<true>(r.nll, TC_BLK, sm); r.hit = tc_isum_wg(r.hit, smi); r.val = tc_isum_wg(r.val, smi);
}
__device__ __forceinline__ void tc_rec_store(unsigned *q, const TcRec &r) { q[0] = __float_as_uint(r.nll); q[1] = (unsigned)r.hit; q[2] = (unsigned)r.val; }
// PART NULL: the one workgroup of the launch stores REC itself; else every workgroup leaves its record at PART[4 blockIdx.x]
__global__ void __launch_bounds__(TC_BLK) k_tc_score(const float *__restrict__ Pm, const float *__restrict__ STAT, const float *__restrict__ IDS,
                                                     unsigned *__restrict__ PART, unsigned *__restrict__ REC, long T, int V, float fV) {
    __shared__ float sm[4]; __shared__ int smi[4];
    TcRec r = { 0.0f, 0, 0 };
    for (long t = (long)blockIdx.x * TC_BLK + threadIdx.x; t < T; t += (long)gridDim.x * TC_BLK) {      // a thread's tokens in ascending order
        const int k = token_id(IDS[t], fV, V);
        if (k >= 0) {
            r.nll -= __logf(fmaxf(Pm[t * V + k], FLT_MIN));
            r.hit += (int)STAT[2 * t + 1] == k ? 1 : 0;
            r.val++;
        }
    }
    tc_rec_fold(r, sm, smi);
    if (threadIdx.x == 0) tc_rec_store(PART ? PART + 4 * blockIdx.x : REC, r);
}
__global__ void __launch_bounds__(TC_BLK) k_tc_score_fold(const unsigned *__restrict__ PART, unsigned *__restrict__ REC, int n) {
    __shared__ float sm[4]; __shared__ int smi[4];
    TcRec r = { 0.0f, 0, 0 };
    if ((int)threadIdx.x < n) { const unsigned *q = PART + 4 * threadIdx.x; r.nll = __uint_as_float(q[0]); r.hit = (int)q[1]; r.val = (int)q[2]; }
    tc_rec_fold(r, sm, smi);
    if (threadIdx.x == 0) tc_rec_store(REC, r);
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_token_ce_plan reports
struct TcPlan { int rung, vw, items, tl, tsh, G, passes, R, fgrid, wb, cgrid, swg, sl; long ws; };
// admission (who: the entry's name for the message) in 64 bits, a function of its arguments only.  o is written on T4K_OK alone
int tc_plan(TcPlan &o, const char *who, long T, long V, bool aligned, long ws_bytes) {
    if (T < 1 || V < 2) return fail(T4K_ERR_ARG, "%s: T=%ld below 1 or V=%ld below 2", who, T, V);
    if (ws_bytes < 0) return fail(T4K_ERR_ARG, "%s: ws_bytes below 0", who);
    if (V > (1L << 24)) return fail(T4K_ERR_UNSUPPORTED, "%s: V=%ld above 2^24 (a float holds no larger id exactly)", who, V);
    if (T >= (1L << 31) || T * V >= (1L << 31)) return fail(T4K_ERR_UNSUPPORTED, "%s: T V = %ld x %ld at or above 2^31", who, T, V);
    TcPlan g;
    g.vw = (aligned && V % 4 == 0) ? 4 : 1;
    g.items = (int)(V / g.vw);
    g.tl = 1; g.tsh = 0; g.G = 1; g.passes = 1; g.R = 0;
    if (g.items <= 64 * TC_NV) {
        g.rung = 0;
        while (g.tl < 64 && g.tl * TC_IPL < g.items) { g.tl <<= 1; g.tsh++; }
        g.G = 64 / g.tl;
        g.fgrid = (int)std::min(ceil_div(ceil_div(T, g.G), 4), (long)TC_WG);
    } else {
        g.rung = g.items <= TC_BLK * TC_NV ? 1 : 2;
        g.tl = TC_BLK; g.tsh = 8;
        if (g.rung == 2) { g.passes = 2; g.R = (int)ceil_div(g.items, TC_BLK * TC_NV) + 1; }      // a rescale a chunk and one from the lane to the workgroup
        g.fgrid = (int)std::min(T, (long)TC_WG);
    }
    g.wb = 64;                                                                  // CE backward: a wave's batch shrinks until the launch is TC_CEW batches wide
    while (g.wb > 1 && ceil_div(T, g.wb) < TC_CEW) g.wb >>= 1;
    g.cgrid = (int)std::min(ceil_div(ceil_div(T, g.wb), 4), (long)TC_WG);
    g.swg = (int)std::min(ceil_div(T, TC_BLK), (long)TC_SWG);                   // score: partial records of 16 bytes where they fit, else one workgroup
    if (g.swg > 1 && (long)g.swg * 16 > ws_bytes) g.swg = 1;
    g.sl = g.swg > 1 ? 2 : 1;
    g.ws = g.swg > 1 ? (long)g.swg * 16 : 0;
    o = g; return T4K_OK;
}
TcP tc_args(const TcPlan &g, long T, int V) { TcP p; p.T = T; p.V = V; p.items = g.items; p.tl = g.tl; p.tsh = g.tsh; p.G = g.G; return p; }

} // namespace

extern "C" {

int t4k_token_ce_plan(long T, int V, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_token_ce_plan: null");
    TcPlan g;
    const int rc = tc_plan(g, "t4k_token_ce_plan", T, V, aligned != 0, ws_bytes); if (rc != T4K_OK) return rc;
    out[0] = g.rung; out[1] = g.vw; out[2] = g.tl; out[3] = g.G; out[4] = g.passes; out[5] = g.R; out[6] = g.sl; out[7] = (int)g.ws;
    return T4K_OK;
}

int t4k_token_softmax_fwd(const float *X, float *P, float *STAT, long T, int V, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !P || !STAT) return fail(T4K_ERR_ARG, "t4k_token_softmax_fwd: null");
    TcPlan g;
    const int rc = tc_plan(g, "t4k_token_softmax_fwd", T, V, all16(X, P), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long n = T * V;
    if (clash(P, n, X, n) || clash(STAT, 2 * T, X, n) || clash(STAT, 2 * T, P, n)) return fail(T4K_ERR_ARG, "t4k_token_softmax_fwd: an output overlaps another operand");
    hipStream_t hs = t4k::S(s);
    const TcP p = tc_args(g, T, V);
    const dim3 grid((unsigned)g.fgrid), blk(TC_BLK);
    pick<4, 1>(g.vw, [&](auto vw) {
        constexpr int VW = decltype(vw)::value;
        if (g.rung == 0)      T4K_LAUNCH((k_tc_fwd<VW, 0>), grid, blk, 0, hs, X, P, STAT, p);
        else if (g.rung == 1) T4K_LAUNCH((k_tc_fwd<VW, 1>), grid, blk, 0, hs, X, P, STAT, p);
        else                  T4K_LAUNCH((k_tc_fwd2<VW>), grid, blk, 0, hs, X, P, STAT, p);
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_token_softmax_bwd(const float *X, const float *STAT, const float *DY, float *DX, long T, int V, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !STAT || !DY || !DX) return fail(T4K_ERR_ARG, "t4k_token_softmax_bwd: null");
    TcPlan g;
    const int rc = tc_plan(g, "t4k_token_softmax_bwd", T, V, all16(X, DY, DX), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long n = T * V;
    if (clash(DX, n, X, n, true) || clash(DX, n, DY, n) || clash(DX, n, STAT, 2 * T))
        return fail(T4K_ERR_ARG, "t4k_token_softmax_bwd: DX overlaps another operand (it may be X itself, nothing else)");
    hipStream_t hs = t4k::S(s);
    const TcP p = tc_args(g, T, V);
    const dim3 grid((unsigned)g.fgrid), blk(TC_BLK);
    pick<4, 1>(g.vw, [&](auto vw) {
        constexpr int VW = decltype(vw)::value;
        if (g.rung == 0)      T4K_LAUNCH((k_tc_jbwd<VW, 0>), grid, blk, 0, hs, X, STAT, DY, DX, p);
        else if (g.rung == 1) T4K_LAUNCH((k_tc_jbwd<VW, 1>), grid, blk, 0, hs, X, STAT, DY, DX, p);
        else                  T4K_LAUNCH((k_tc_jbwd2<VW>), grid, blk, 0, hs, X, STAT, DY, DX, p);
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_token_ce_bwd(const float *P, const float *IDS, float *DX, long T, int V, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!P || !IDS || !DX) return fail(T4K_ERR_ARG, "t4k_token_ce_bwd: null");
    TcPlan g;
    const int rc = tc_plan(g, "t4k_token_ce_bwd", T, V, all16(P, DX), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long n = T * V;
    if (clash(DX, n, P, n) || clash(DX, n, IDS, T)) return fail(T4K_ERR_ARG, "t4k_token_ce_bwd: DX overlaps another operand");
    hipStream_t hs = t4k::S(s);
    TcC p;
    p.T = T; p.V = V; p.items = g.items; p.wb = g.wb; p.fV = (float)V; p.di = fast_div(g.items);
    const dim3 grid((unsigned)g.cgrid), blk(TC_BLK);
    if (g.vw == 4) T4K_LAUNCH((k_tc_ce_bwd<4>), grid, blk, 0, hs, P, IDS, DX, p);
    else           T4K_LAUNCH((k_tc_ce_bwd<1>), grid, blk, 0, hs, P, IDS, DX, p);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_token_ce_score(const float *P, const float *STAT, const float *IDS, void *REC, long T, int V, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!P || !STAT || !IDS || !REC) return fail(T4K_ERR_ARG, "t4k_token_ce_score: null");
    TcPlan g;
    const int rc = tc_plan(g, "t4k_token_ce_score", T, V, false, (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const float *R = (const float *)REC;
    if (clash(R, 3, P, T * V) || clash(R, 3, STAT, 2 * T) || clash(R, 3, IDS, T)) return fail(T4K_ERR_ARG, "t4k_token_ce_score: REC overlaps an operand");
    hipStream_t hs = t4k::S(s);
    unsigned *part = g.swg > 1 ? (unsigned *)ws_for(s) : nullptr;
    T4K_LAUNCH(k_tc_score, dim3((unsigned)g.swg), dim3(TC_BLK), 0, hs, P, STAT, IDS, part, (unsigned *)REC, T, V, (float)V);
    if (part) T4K_LAUNCH(k_tc_score_fold, dim3(1), dim3(TC_BLK), 0, hs, part, (unsigned *)REC, g.swg);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
