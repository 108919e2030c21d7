// window.hip - a box of one dense NHWC tensor copied onto a box of another: dst[doff + i] = src[soff + i] for every i of the
// box.  A slice is doff = 0, ddim = ext; a store is soff = 0, sdim = ext.  Pure data movement, HBM-bound: an element is loaded and stored
// and nothing else, one launch per call, no allocation, no synchronisation, no workspace.
// No reference definition: the nearest thing is MMU::slice (src/mu/mmu.cu:307-330), one memcpy per (sample, row) of an H / W window.
#include "launch.h"

using namespace t4k;

namespace {

enum { F_COPY = 0, F_RUNS };

// What the host leaves after folding axes of extent 1 into the two base offsets and merging every axis with an inner neighbour taken whole
// on both sides: R runs of L contiguous floats, the same on both sides, the run index r splitting into at most three digits (ext,
// outermost first, unused = 1) with source strides ss and destination strides ds.  Work is dealt by (run, position in run) as
// k_permute_runs deals it (permute.hip): a pass of 256 lanes takes `rpb` runs of 1 << shift lanes each (short runs), or one 256-lane
// chunk of the `nc` chunks of one run (long runs).  The copy family is R == 1: nothing is left above the run.
struct WinPlan {
    long R, L, U;                 // runs, run length, units per run (L / 4 float4s on the vector path, else L)
    long nitem, nc;               // passes: ceil(R / rpb) * nc; 256-lane chunks per run
    long ss[3], ds[3];
    unsigned ext[3];
    unsigned rpb, shift;          // one of nc / rpb is 1
    int digits;
};

typedef float vec4 __attribute__((ext_vector_type(4)));   // the bare vector type: an array of them stays in registers
constexpr int NW = 4;                              // passes a lane keeps in flight: their loads are all issued before the first store waits for one

// pass w of the plan, this lane: where its unit lies in the two boxes (in floats from the box starts); false when the lane has nothing to move
template <bool VEC>
__device__ __forceinline__ bool locate(const WinPlan &p, long w, unsigned lane_run, unsigned lane_u, long &so, long &dn) {
    if (w >= p.nitem) return false;
    long rb = w, c = 0;
    if (p.nc > 1) {                                                        // uniform over the workgroup: once per 256-lane chunk
        if (p.R == 1) { rb = 0; c = w; }                                   // one run (the copy family): the chunk count may exceed 32 bits, and nothing is divided
        else { unsigned cc; divmod(w, (unsigned)p.nc, rb, cc); c = cc; }
    }
    const long r = rb * p.rpb + lane_run, u = (c << p.shift) + lane_u;
    if (r >= p.R || u >= p.U) return false;
    long t = r;
    unsigned i;
    so = dn = VEC ? u << 2 : u;
    if (p.ext[2] > 1) { divmod(t, p.ext[2], t, i); so += (long)i * p.ss[2]; dn += (long)i * p.ds[2]; }
    if (p.ext[1] > 1) { divmod(t, p.ext[1], t, i); so += (long)i * p.ss[1]; dn += (long)i * p.ds[1]; }
    so += t * p.ss[0]; dn += t * p.ds[0];
    return true;
}

// src and dst point at the first element of the two boxes.  VEC - host: L % 4 == 0, every stride a multiple of 4, both box starts 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(BLK) k_window(const float *__restrict__ src, float *__restrict__ dst, const WinPlan p) {
    using T = std::conditional_t<VEC, vec4, float>;
    const unsigned lane_run = threadIdx.x >> p.shift, lane_u = threadIdx.x & ((1u << p.shift) - 1u);
    for (long w0 = blockIdx.x; w0 < p.nitem; w0 += (long)NW * gridDim.x) {
        T v[NW]; long to[NW]; bool on[NW];
#pragma unroll
        for (int k = 0; k < NW; k++) {
            long so = 0;
            on[k] = locate<VEC>(p, w0 + (long)k * gridDim.x, lane_run, lane_u, so, to[k]);
            if (on[k]) v[k] = *reinterpret_cast<const T *>(src + so);
        }
#pragma unroll
        for (int k = 0; k < NW; k++) if (on[k]) *reinterpret_cast<T *>(dst + to[k]) = v[k];
    }
}

struct Plan {
    int family;
    bool vec;
    long sbase, dbase;            // the two box starts, in floats from the base pointers
    long stotal, dtotal;
    WinPlan run;
};

int check_side(const int dim[4], const int off[4], const int ext[4], const char *who, const char *side, long *total) {
    long n = 1;
    for (int i = 0; i < 4; i++) {
        if (dim[i] < 1 || ext[i] < 1) return fail(T4K_ERR_ARG, "%s: extent < 1", who);
        if (off[i] < 0) return fail(T4K_ERR_ARG, "%s: negative offset", who);
        if ((long)off[i] + ext[i] > dim[i]) return fail(T4K_ERR_ARG, "%s: the box leaves %s on axis %d", who, side, i);
        if (n > (1L << 40) / dim[i]) return fail(T4K_ERR_ARG, "%s: more than 2^40 elements", who);
        n *= dim[i];
    }
    *total = n;
    return T4K_OK;
}

int make_plan(Plan &P, const int sdim[4], const int soff[4], const int ddim[4], const int doff[4], const int ext[4], const char *who) {
    if (!sdim || !soff || !ddim || !doff || !ext) return fail(T4K_ERR_ARG, "%s: null", who);
    int rc = check_side(sdim, soff, ext, who, "src", &P.stotal); if (rc != T4K_OK) return rc;
    rc = check_side(ddim, doff, ext, who, "dst", &P.dtotal); if (rc != T4K_OK) return rc;
    long sstr[4], dstr[4], a = 1, b = 1;
    P.sbase = P.dbase = 0;
    for (int i = 3; i >= 0; i--) {
        sstr[i] = a; a *= sdim[i]; dstr[i] = b; b *= ddim[i];
        P.sbase += soff[i] * sstr[i]; P.dbase += doff[i] * dstr[i];
    }
    // outermost first; axes of extent 1 have gone into the base offsets; an axis joins the group outside it when both sides step through
    // the two as through one axis, which is what "the inner one is taken whole on both sides" leaves
    long e[4], s[4], d[4]; int n = 0;
    for (int i = 0; i < 4; i++) {
        if (ext[i] == 1) continue;
        if (n && s[n - 1] == sstr[i] * ext[i] && d[n - 1] == dstr[i] * ext[i]) { e[n - 1] *= ext[i]; s[n - 1] = sstr[i]; d[n - 1] = dstr[i]; }
        else { e[n] = ext[i]; s[n] = sstr[i]; d[n] = dstr[i]; n++; }
    }
    if (!n || s[n - 1] != 1 || d[n - 1] != 1) { e[n] = 1; s[n] = 1; d[n] = 1; n++; }   // C has extent 1: the run is one float (a single element included)
    WinPlan &p = P.run; p = WinPlan{};
    P.family = n == 1 ? F_COPY : F_RUNS;
    p.L = e[n - 1]; p.R = 1; p.digits = n - 1;
    for (int k = 0; k < 3; k++) { p.ext[k] = 1; p.ss[k] = p.ds[k] = 0; }
    bool str4 = true;
    for (int i = 0; i < n - 1; i++) {                                       // left-aligned: the outermost digit is what the divisions leave, so only the inner ones are divisors
        if (i && e[i] > 0xffffffffL) return fail(T4K_ERR_ARG, "%s: merged extent too large", who);
        p.ext[i] = i ? (unsigned)e[i] : (unsigned)std::min(e[i], 0xffffffffL);  // ext[0] is only compared with 1
        p.ss[i] = s[i]; p.ds[i] = d[i]; p.R *= e[i]; str4 = str4 && !(s[i] & 3) && !(d[i] & 3);
    }
    P.vec = !(p.L & 3) && str4;                                            // so far: whole runs of float4s a multiple of 16 bytes apart; finish() adds the starts
    return T4K_OK;
}
// `starts`: both box starts (base pointer plus folded offset) on 16 bytes
void finish(Plan &P, bool starts) {
    WinPlan &p = P.run;
    P.vec = P.vec && starts;
    p.U = P.vec ? p.L >> 2 : p.L;
    p.shift = 0; while (p.shift < 8 && (1L << p.shift) < p.U) p.shift++;
    p.rpb = (unsigned)BLK >> p.shift;                                      // runs per pass (1 once a run fills 256 lanes)
    p.nc = (p.U + BLK - 1) / BLK;                                          // 256-lane chunks per run (1 below that)
    p.nitem = ((p.R + p.rpb - 1) / p.rpb) * p.nc;
}

} // namespace

extern "C" {

int t4k_window(const float *src, const int sdim[4], const int soff[4], float *dst, const int ddim[4], const int doff[4], const int ext[4], t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!src || !dst) return fail(T4K_ERR_ARG, "t4k_window: null");
    Plan P;
    const int rc = make_plan(P, sdim, soff, ddim, doff, ext, "t4k_window"); if (rc != T4K_OK) return rc;
    if (src < dst + P.dtotal && dst < src + P.stotal) return fail(T4K_ERR_ARG, "t4k_window: dst overlaps src");
    finish(P, aligned16(src + P.sbase) && aligned16(dst + P.dbase));
    const WinPlan &p = P.run;
    const int g = (int)std::min(p.nitem, (long)MAX_WG);
    with_flags([&](auto v) { T4K_LAUNCH((k_window<v.value>), dim3(g), dim3(BLK), 0, S(s), src + P.sbase, dst + P.dbase, p); }, P.vec);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

int t4k_window_plan(const int sdim[4], const int soff[4], const int ddim[4], const int doff[4], const int ext[4], int aligned, int out[6]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_window_plan: null");
    Plan P;
    const int rc = make_plan(P, sdim, soff, ddim, doff, ext, "t4k_window_plan"); if (rc != T4K_OK) return rc;
    finish(P, aligned != 0 && !(P.sbase & 3) && !(P.dbase & 3));
    out[0] = P.family; out[1] = P.vec ? 1 : 0;
    out[2] = (int)std::min(P.run.L, 0x7fffffffL); out[3] = (int)std::min(P.run.R, 0x7fffffffL);
    out[4] = P.run.digits; out[5] = (int)std::min(P.run.nitem, 0x7fffffffL);
    return T4K_OK;
}

} // extern "C"
