// embed.hip - the embedding layer for NHWC fp32 tokens, forward and backward: a token-embedding lookup, a learned position table, or both.
// T = N L tokens of E contiguous floats, t = n L + l.  Token mode (V >= 1): out[t] = (valid(t) ? TABLE[id_t] : 0) + (POS ? POS[l] : 0) with the id a float,
// valid <=> 0 <= x < V in float compares, id = (int)x.  Position mode (V = 0): out[t] = x[t] + POS[l].  The reference has no such layer.
// Forward: a TEAM of tl lanes of a wave owns a token at a time (tl = the power of two that covers the row's items, at most 64); one lane of the wave reads a
// token's id and its position, the team receives them by a lane exchange; the output is streamed (nothing in the launch reads it again).
// Backward: ownership by table row.  A wave UNIT owns a slab of R table rows x 64 lanes' worth of channels x one of P token parts; it walks its part of the id
// list in ascending token order, 64 ids a load, ballots the lanes whose id falls in the slab and adds the matching dY rows onto its accumulators in LDS, a
// lane touching its own columns only - no barrier, no atomic.  P = 1: the unit adds its rows onto DTABLE itself.  P > 1 (a small vocabulary, which would leave
// the device idle): it stores its rows, zeros included, into the [P, V, E] slab of the workspace and a second launch folds the parts in order.  dPOS is a
// role of the same launch: 16 items x 16 groups of samples a workgroup, the groups joined in order through LDS; in position mode the same load feeds DX.
#include "t4k_common.h"
#include "launch.h"

using namespace t4k;

namespace {

constexpr int EM_BLK   = 256;           // the workgroup: four waves, one per SIMD
constexpr int EM_R     = 16;            // table rows of a slab (EM_R x 64 lanes x 16 bytes = 16 KiB of LDS a wave)
constexpr int EM_UNITS = 1024;          // wave units the scatter is spread over where the vocabulary alone gives fewer: 256 CUs x 4 SIMDs, a constant
constexpr int EM_PART  = 64;            // tokens a part holds at least: one id load of a wave
constexpr int EM_MB    = 8;             // dY rows a unit has in flight
constexpr int EM_WG    = 2048;          // workgroups the forward and the fold spread over at most
constexpr int EM_PI    = 16;            // dPOS role: items of a workgroup, and groups of samples

typedef float v4f __attribute__((ext_vector_type(4)));

struct EmF { long T; int L, V, E, items, tl, tsh, wb; float fV; };
struct EmB { long T, per, units, pitems; int L, V, E, N, slabs, chunks, swg; float fV; };

template <int VW> __device__ __forceinline__ void em_ld(const float *q, float (&v)[VW]) {
    if constexpr (VW == 4) { const float4 t = *reinterpret_cast<const float4 *>(q); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *q;
}
template <int VW> __device__ __forceinline__ void em_st(float *q, const float (&v)[VW]) {
    if constexpr (VW == 4) *reinterpret_cast<float4 *>(q) = make_float4(v[0], v[1], v[2], v[3]);
    else *q = v[0];
}
template <int VW> __device__ __forceinline__ void em_st_nt(float *q, const float (&v)[VW]) {     // streaming store
    if constexpr (VW == 4) __builtin_nontemporal_store(v4f{v[0], v[1], v[2], v[3]}, reinterpret_cast<v4f *>(q));
    else __builtin_nontemporal_store(v[0], q);
}
// the id of a token: -1 for padding (NaN, negatives, -0.5, V and above: every compare is a float compare, the id is formed only where they hold)
__device__ __forceinline__ int em_id(float x, float fV, int V) {
    if (!(x >= 0.0f && x < fV)) return -1;
    const int id = (int)x;
    return id < V ? id : -1;
}

// ------------------------------------------------------------------ forward: one launch.  SRC = the ids (TOK) or x
template <int VW, bool TOK>
__global__ void __launch_bounds__(EM_BLK) k_em_fwd(const float *__restrict__ SRC, const float *__restrict__ TABLE, const float *__restrict__ POS, float *__restrict__ O, EmF p) {
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int sub = lane >> p.tsh, it0 = lane & (p.tl - 1), G = 64 >> p.tsh;      // G tokens of the wave's batch are in flight at a time
    const long nb = (p.T + p.wb - 1) / p.wb;
    for (long b = (long)blockIdx.x * 4 + w; b < nb; b += (long)gridDim.x * 4) {    // (uniform over the wave)
        const long t0 = b * p.wb, tm = t0 + lane;
        int id = -1, l = 0;
        if (lane < p.wb && tm < p.T) {                                          // one lane reads a token's id and works out its position, once
            if constexpr (TOK) id = em_id(SRC[tm], p.fV, p.V);
            if (POS) l = (int)(tm % p.L);
        }
        for (int k = 0; k < p.wb; k += G) {                                     // (uniform; k + sub < wb <= 64)
            const int j = k + sub, idj = __shfl(id, j, 64), lj = __shfl(l, j, 64);
            const long t = t0 + j;
            if (t >= p.T) continue;
            const float *row = TOK ? TABLE + (long)(idj < 0 ? 0 : idj) * p.E : SRC + t * p.E;
            const float *pr = POS + (long)lj * p.E;
            float *o = O + t * p.E;
            for (int it = it0; it < p.items; it += p.tl) {
                float v[VW], q[VW];
#pragma unroll
                for (int e = 0; e < VW; e++) v[e] = 0.0f;
                if (!TOK || idj >= 0) em_ld<VW>(row + it * VW, v);
                if (POS) {
                    em_ld<VW>(pr + it * VW, q);
#pragma unroll
                    for (int e = 0; e < VW; e++) v[e] += q[e];
                }
                em_st_nt<VW>(o + it * VW, v);
            }
        }
    }
}

// ------------------------------------------------------------------ backward: the scatter units (ROLES & 1) and the dPOS | DX role (ROLES & 2) of one launch
// PART NULL: rung 1, a unit adds onto DTABLE; else rung 2, it stores its rows at PART[part][v][c].  DX is never DY here (the entry passes NULL then)
template <int VW, int ROLES>
__global__ void __launch_bounds__(EM_BLK) k_em_bwd(const float *__restrict__ IDS, const float *__restrict__ DY, float *__restrict__ DTABLE, float *__restrict__ PART,
                                                   float *__restrict__ DPOS, float *__restrict__ DX, EmB p) {
    constexpr int CH = 64 * VW;
    __shared__ float sm[(ROLES & 1) ? 4 * EM_R * CH : EM_PI * EM_PI * VW];
    if ((ROLES & 1) && (int)blockIdx.x < p.swg) {
        const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
        const long u = (long)blockIdx.x * 4 + w;
        if (u >= p.units) return;                                              // (the whole wave; this role has no barrier)
        const int chunk = (int)(u % p.chunks); const long rest = u / p.chunks;
        const int slab = (int)(rest % p.slabs), part = (int)(rest / p.slabs);
        const int v0 = slab * EM_R, c = chunk * CH + lane * VW;
        const bool active = c < p.E;                                            // (E % VW == 0: the lane's whole item is inside or outside)
        float *acc = sm + w * EM_R * CH + lane * VW;                            // acc[r * CH + e]: this lane's columns of slab row r, touched by no other lane
#pragma unroll
        for (int r = 0; r < EM_R; r++) {
#pragma unroll
            for (int e = 0; e < VW; e++) acc[r * CH + e] = 0.0f;
        }
        const long t0 = (long)part * p.per, t1 = min(p.T, t0 + p.per);
        const float *dyc = DY + c;
        unsigned hit = 0;                                                       // (uniform) the slab rows some token of the part names
        for (long b4 = t0; b4 < t1; b4 += 4 * 64) {                             // (uniform) four id loads of the wave in flight: the walk is a chain of L2 round trips
            int r4[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const long tm = b4 + u * 64 + lane;
                r4[u] = -1;
                if (tm < t1) {
                    const int id = em_id(IDS[tm], p.fV, p.V);
                    if (id >= v0 && id < v0 + EM_R) r4[u] = id - v0;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const long base = b4 + u * 64;
                const int r = r4[u];
                unsigned long long mask = __ballot(r >= 0);
                while (mask) {                                                  // the matches in ascending token order, EM_MB dY loads in flight
                    int j[EM_MB];
#pragma unroll
                    for (int q = 0; q < EM_MB; q++) {
                        j[q] = -1;
                        if (mask) { j[q] = __builtin_ctzll(mask); mask &= mask - 1; }
                    }
                    float v[EM_MB][VW];
#pragma unroll
                    for (int q = 0; q < EM_MB; q++) {
#pragma unroll
                        for (int e = 0; e < VW; e++) v[q][e] = 0.0f;
                        if (j[q] >= 0 && active) em_ld<VW>(dyc + (base + j[q]) * p.E, v[q]);
                    }
#pragma unroll
                    for (int q = 0; q < EM_MB; q++) {
                        if (j[q] < 0) break;                                    // (uniform: j comes from the ballot)
                        const int rq = __builtin_amdgcn_readfirstlane(__shfl(r, j[q], 64));     // 0 .. EM_R - 1 by the test above; the same in every lane
                        hit |= 1u << rq;
                        if (active) {
#pragma unroll
                            for (int e = 0; e < VW; e++) acc[rq * CH + e] += v[q][e];
                        }
                    }
                }
            }
        }
        if (!active) return;
        if (PART) {
            for (int r = 0; r < EM_R && v0 + r < p.V; r++) {
                float a[VW];
#pragma unroll
                for (int e = 0; e < VW; e++) a[e] = acc[r * CH + e];
                em_st<VW>(PART + ((long)part * p.V + v0 + r) * p.E + c, a);
            }
            return;
        }
        float d[EM_R][VW];                                                      // every row's load in flight before the first store (a store per row would chain them)
#pragma unroll
        for (int r = 0; r < EM_R; r++) {
#pragma unroll
            for (int e = 0; e < VW; e++) d[r][e] = 0.0f;
            if (hit >> r & 1) em_ld<VW>(DTABLE + (long)(v0 + r) * p.E + c, d[r]);      // (a named row is below V)
        }
#pragma unroll
        for (int r = 0; r < EM_R; r++) {
            bool any = false;
#pragma unroll
            for (int e = 0; e < VW; e++) { const float a = acc[r * CH + e]; if (a != 0.0f) { d[r][e] += a; any = true; } }     // a sum of exactly 0 leaves the element's bits
            if (any && (hit >> r & 1)) em_st<VW>(DTABLE + (long)(v0 + r) * p.E + c, d[r]);
        }
        return;
    }
    if constexpr ((ROLES & 2) != 0) {
        // dPOS[l, c] += sum over n of dY[n, l, c]: thread (g, i) adds the samples of group g for item i in ascending order, the 16 groups are added in order
        const int i = (int)threadIdx.x & (EM_PI - 1), g = (int)threadIdx.x / EM_PI;
        const long item = (long)((int)blockIdx.x - ((ROLES & 1) ? p.swg : 0)) * EM_PI + i;
        const int nper = (p.N + EM_PI - 1) / EM_PI, n0 = g * nper, n1 = min(p.N, n0 + nper);
        const long LE = (long)p.L * p.E;
        float s[VW];
#pragma unroll
        for (int e = 0; e < VW; e++) s[e] = 0.0f;
        if (item < p.pitems) {
#pragma unroll 4
            for (int n = n0; n < n1; n++) {
                float v[VW];
                em_ld<VW>(DY + n * LE + item * VW, v);
                if (DX) em_st<VW>(DX + n * LE + item * VW, v);
#pragma unroll
                for (int e = 0; e < VW; e++) s[e] += v[e];
            }
        }
        if (!DPOS) return;                                                      // (uniform: train == 0, the copy alone)
#pragma unroll
        for (int e = 0; e < VW; e++) sm[(g * EM_PI + i) * VW + e] = s[e];
        __syncthreads();
        if (g == 0 && item < p.pitems) {
            float a[VW];
#pragma unroll
            for (int e = 0; e < VW; e++) a[e] = sm[i * VW + e];
            for (int k = 1; k < EM_PI; k++) {
#pragma unroll
                for (int e = 0; e < VW; e++) a[e] += sm[(k * EM_PI + i) * VW + e];
            }
            float *d = DPOS + item * VW;
#pragma unroll
            for (int e = 0; e < VW; e++) d[e] += a[e];
        }
    }
}

// rung 2's second launch: DTABLE[i] += ((part 0 + part 1) + ..) in part order, an item a thread
template <int VW>
__global__ void __launch_bounds__(EM_BLK) k_em_fold(const float *__restrict__ PART, float *__restrict__ DTABLE, long nitems, long VE, int P) {
    for (long i = (long)blockIdx.x * EM_BLK + threadIdx.x; i < nitems; i += (long)gridDim.x * EM_BLK) {
        float a[VW];
        em_ld<VW>(PART + i * VW, a);
#pragma unroll 8
        for (int q = 1; q < P; q++) {
            float b[VW];
            em_ld<VW>(PART + q * VE + i * VW, b);
#pragma unroll
            for (int e = 0; e < VW; e++) a[e] += b[e];
        }
        float *d = DTABLE + i * VW;
#pragma unroll
        for (int e = 0; e < VW; e++) if (a[e] != 0.0f) d[e] += a[e];
    }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_embed_plan reports
struct EmPlan { int rung, vw, R, P, fl, bl, swg, tl, tsh, wb, fgrid, slabs, chunks, pwg; long per, units, ws; };
long em_cdiv(long a, long b) { return (a + b - 1) / b; }
// admission (who: the entry's name for the message) in 64 bits: the extents may be anything their types hold.  g is written on T4K_OK alone
int em_plan(EmPlan &o, const char *who, long T, int L, int V, int E, int pos, bool aligned, long ws_bytes) {
    if (T < 1 || L < 1 || E < 1 || V < 0) return fail(T4K_ERR_ARG, "%s: an extent below 1 (T=%ld L=%d V=%d E=%d)", who, T, L, V, E);
    if (T % L) return fail(T4K_ERR_ARG, "%s: T=%ld is no multiple of L=%d", who, T, L);
    if (ws_bytes < 0) return fail(T4K_ERR_ARG, "%s: ws_bytes below 0", who);
    if (pos != 0 && pos != 1) return fail(T4K_ERR_ARG, "%s: pos=%d (0 none, 1 learned table)", who, pos);
    if (V == 0 && pos == 0) return fail(T4K_ERR_ARG, "%s: neither a token table (V=0) nor a position table (pos=0)", who);
    const long lim = 1L << 31;
    if (T >= lim || T * E >= lim || (long)V * E >= lim) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 elements or more (T E or V E)", who);
    EmPlan g;
    g.vw = (aligned && E % 4 == 0) ? 4 : 1;
    const int items = E / g.vw;
    // forward: the team is the power of two that covers the row's items (at most a wave); the wave's batch of tokens shrinks until the launch is 1024
    // workgroups wide or a batch is one round of teams
    g.tl = 1; g.tsh = 0;
    while (g.tl < 64 && g.tl < items) { g.tl <<= 1; g.tsh++; }
    g.wb = 64;
    while (g.wb > 64 / g.tl && em_cdiv(T, 4L * g.wb) < 1024) g.wb >>= 1;
    g.fgrid = (int)std::min(em_cdiv(T, 4L * g.wb), (long)EM_WG);
    g.fl = 1;
    g.pwg = pos ? (int)em_cdiv((long)L * items, EM_PI) : 0;                 // workgroups of the dPOS | DX role
    if (V == 0) {                                                           // position mode
        g.rung = 0; g.R = 0; g.P = 1; g.bl = 1; g.swg = g.pwg; g.slabs = g.chunks = 0; g.per = 0; g.units = 0; g.ws = 0;
        o = g; return T4K_OK;
    }
    g.R = EM_R;
    g.slabs = (int)em_cdiv(V, EM_R); g.chunks = (int)em_cdiv(items, 64);
    const long base = (long)g.slabs * g.chunks;                             // units the vocabulary gives by itself
    const long bytes = (long)V * E * (long)sizeof(float);                   // one part's rows in the workspace
    long P = std::min(std::min(em_cdiv(EM_UNITS, base), std::max(1L, T / EM_PART)), std::min(ws_bytes, 0x7fffffffL) / bytes);   // (the bytes used are reported in an int)
    if (P < 1) P = 1;
    g.per = em_cdiv(em_cdiv(T, 64), P) * 64;                                // tokens of a part: whole id loads
    g.P = (int)em_cdiv(T, g.per);
    g.rung = g.P > 1 ? 2 : 1;
    g.units = base * g.P;
    g.swg = (int)(em_cdiv(g.units, 4) + g.pwg);
    g.bl = g.rung;
    g.ws = g.P > 1 ? g.P * bytes : 0;
    o = g; return T4K_OK;
}
// do [a, a + na) and [b, b + nb) floats share a byte?  (NULL: no.)  same_ok: the two being ONE tensor is no overlap
bool em_clash(const float *a, long na, const float *b, long nb, bool same_ok = false) {
    if (!a || !b) return false;
    if (same_ok && a == b) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * sizeof(float), b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * sizeof(float);
    return a0 < b1 && b0 < a1;
}
bool em16(const void *a, const void *b, const void *c, const void *d, const void *e) {
    return aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) && aligned16(e);
}

} // namespace

extern "C" {

int t4k_embed_plan(long T, int L, int V, int E, int pos, int aligned, long ws_bytes, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_embed_plan: null");
    EmPlan g;
    const int rc = em_plan(g, "t4k_embed_plan", T, L, V, E, pos, aligned != 0, ws_bytes); if (rc != T4K_OK) return rc;
    out[0] = g.rung; out[1] = g.vw; out[2] = g.R; out[3] = g.P; out[4] = g.fl; out[5] = g.bl; out[6] = g.swg; out[7] = (int)g.ws;
    return T4K_OK;
}

int t4k_embed_fwd(const float *IDS, const float *X, const float *TABLE, const float *POS, float *O, long T, int L, int V, int E, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!O) return fail(T4K_ERR_ARG, "t4k_embed_fwd: null output");
    if ((IDS != nullptr) == (X != nullptr)) return fail(T4K_ERR_ARG, "t4k_embed_fwd: exactly one of IDS (token mode) and X (position mode)");
    if (IDS && (V < 1 || !TABLE)) return fail(T4K_ERR_ARG, "t4k_embed_fwd: token mode needs V >= 1 and TABLE");
    if (X && (V != 0 || !POS || TABLE)) return fail(T4K_ERR_ARG, "t4k_embed_fwd: position mode needs V = 0, POS and no TABLE");
    EmPlan g;
    const int rc = em_plan(g, "t4k_embed_fwd", T, L, V, E, POS ? 1 : 0, em16(IDS, X, TABLE, POS, O), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long n = T * E;
    if (em_clash(O, n, IDS, T) || em_clash(O, n, X, n) || em_clash(O, n, TABLE, (long)V * E) || em_clash(O, n, POS, (long)L * E))
        return fail(T4K_ERR_ARG, "t4k_embed_fwd: the output overlaps another operand");
    hipStream_t hs = t4k::S(s);
    EmF p;
    p.T = T; p.L = L; p.V = V; p.E = E; p.items = E / g.vw; p.tl = g.tl; p.tsh = g.tsh; p.wb = g.wb; p.fV = (float)V;
    const dim3 grid((unsigned)g.fgrid), blk(EM_BLK);
    if (IDS) {
        if (g.vw == 4) T4K_LAUNCH((k_em_fwd<4, true>), grid, blk, 0, hs, IDS, TABLE, POS, O, p);
        else           T4K_LAUNCH((k_em_fwd<1, true>), grid, blk, 0, hs, IDS, TABLE, POS, O, p);
    } else {
        if (g.vw == 4) T4K_LAUNCH((k_em_fwd<4, false>), grid, blk, 0, hs, X, TABLE, POS, O, p);
        else           T4K_LAUNCH((k_em_fwd<1, false>), grid, blk, 0, hs, X, TABLE, POS, O, p);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_embed_bwd(const float *IDS, const float *DY, float *DTABLE, float *DPOS, float *DX, long T, int L, int V, int E, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!DY) return fail(T4K_ERR_ARG, "t4k_embed_bwd: null DY");
    if (V >= 1 && !IDS) return fail(T4K_ERR_ARG, "t4k_embed_bwd: token mode needs IDS");
    if (V == 0 && (IDS || !DX)) return fail(T4K_ERR_ARG, "t4k_embed_bwd: position mode needs DX and no IDS");
    if (V >= 1) DX = nullptr;                                                // no dX: the id tensor is left as it is
    if (!train) DTABLE = nullptr, DPOS = nullptr;
    if (train && V >= 1 && !DTABLE) return fail(T4K_ERR_ARG, "t4k_embed_bwd: DTABLE is required when train != 0");
    if (train && V == 0 && !DPOS) return fail(T4K_ERR_ARG, "t4k_embed_bwd: DPOS is required when train != 0");
    if (V == 0) DTABLE = nullptr;
    EmPlan g;
    const int rc = em_plan(g, "t4k_embed_bwd", T, L, V, E, (V == 0 || DPOS) ? 1 : 0, em16(IDS, DY, DTABLE, DPOS, DX), (long)(st().ws_bytes / 2)); if (rc != T4K_OK) return rc;
    const long n = T * E, ve = (long)V * E, le = (long)L * E;
    if (em_clash(DX, n, DY, n, true) || em_clash(DX, n, DPOS, le) || em_clash(DTABLE, ve, DPOS, le) ||
        em_clash(DTABLE, ve, DY, n) || em_clash(DTABLE, ve, IDS, T) || em_clash(DPOS, le, DY, n) || em_clash(DPOS, le, IDS, T))
        return fail(T4K_ERR_ARG, "t4k_embed_bwd: an output overlaps another operand (DX may be DY, nothing else)");
    if (DX == DY) DX = nullptr;                                              // in place: nothing to copy
    if (!DTABLE && !DPOS && !DX) return T4K_OK;                              // train == 0 and no dX to move: nothing to do
    hipStream_t hs = t4k::S(s);
    EmB p;
    p.T = T; p.per = g.per; p.units = g.units; p.pitems = le / g.vw; p.L = L; p.V = V; p.E = E; p.N = (int)(T / L);
    p.slabs = g.slabs; p.chunks = g.chunks; p.swg = DTABLE ? (int)em_cdiv(g.units, 4) : 0; p.fV = (float)V;
    const int pwg = (DPOS || DX) ? g.pwg : 0;
    float *part = (DTABLE && g.P > 1) ? ws_for(s) : nullptr;
    const dim3 grid((unsigned)(p.swg + pwg)), blk(EM_BLK);
    const int roles = (DTABLE ? 1 : 0) | (pwg ? 2 : 0);
    pick<4, 1>(g.vw, [&](auto vw) {
        constexpr int VW = decltype(vw)::value;
        if (roles == 1)      T4K_LAUNCH((k_em_bwd<VW, 1>), grid, blk, 0, hs, IDS, DY, DTABLE, part, DPOS, DX, p);
        else if (roles == 2) T4K_LAUNCH((k_em_bwd<VW, 2>), grid, blk, 0, hs, IDS, DY, DTABLE, part, DPOS, DX, p);
        else                 T4K_LAUNCH((k_em_bwd<VW, 3>), grid, blk, 0, hs, IDS, DY, DTABLE, part, DPOS, DX, p);
        if (part) {
            const long nitems = ve / VW;
            T4K_LAUNCH((k_em_fold<VW>), dim3((unsigned)std::min(em_cdiv(nitems, EM_BLK), (long)EM_WG)), blk, 0, hs, part, DTABLE, nitems, ve, g.P);
        }
    });
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
