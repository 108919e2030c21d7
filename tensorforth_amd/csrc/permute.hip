// permute.hip - any order of the four axes of a dense NHWC tensor: dst = numpy.transpose(src, perm).  Pure data movement,
// HBM-bound: an element is loaded and stored and nothing else, one launch per call, no allocation, no synchronisation, no workspace.
// No reference definition: the nearest thing is k_transpose (src/t4math.cu:150), which swaps H and W of one sample.
#include "launch.h"

using namespace t4k;

namespace {

enum { F_COPY = 0, F_RUNS, F_TILES };

// What the host leaves after dropping axes of extent 1 and merging source axes that stay neighbours, in the same order, in the output:
// at most four groups, listed in OUTPUT order (the output is dense over them), each with its source stride.
//
// copy / runs: the innermost group is innermost in the source too - R runs of L contiguous floats, the run index r splitting into at
// most three digits (ext, outermost first, unused = 1) with source strides ss; the output run r starts at r * L.  Work is dealt by
// (run, position in run) exactly as k_tt_bcast deals it (bcast.hip): a workgroup iteration takes `rpb` runs of 1 << shift lanes each
// (short runs), or one 256-lane chunk of the `nc` chunks of one run (long runs).  The copy family is R == 1.
struct RunPlan {
    long R, L, U;                 // runs, run length, units per run (L / 4 float4s on the vector path, else L)
    long nitem, nc;               // workgroup iterations: ceil(R / rpb) * nc; 256-lane chunks per run
    long ss[3];
    unsigned ext[3];
    unsigned rpb, shift;          // one of nc / rpb is 1
};

template <bool VEC>
__global__ void __launch_bounds__(BLK) k_permute_runs(const float *__restrict__ src, float *__restrict__ dst, const RunPlan p) {
    const unsigned lane_run = threadIdx.x >> p.shift, lane_u = threadIdx.x & ((1u << p.shift) - 1u);
    for (long w = blockIdx.x; w < p.nitem; w += gridDim.x) {
        long rb = w, c = 0;
        if (p.nc > 1) {                                                    // uniform over the workgroup: once per 256-lane chunk
            if (p.R == 1) { rb = 0; c = w; }                               // one run (the copy family): the chunk count may exceed 32 bits, and nothing is divided
            else { unsigned cc; divmod(w, (unsigned)p.nc, rb, cc); c = cc; }
        }
        const long r = rb * p.rpb + lane_run, u = (c << p.shift) + lane_u;
        if (r >= p.R || u >= p.U) continue;
        long t = r, off = 0;
        unsigned i;
        if (p.ext[2] > 1) { divmod(t, p.ext[2], t, i); off += (long)i * p.ss[2]; }
        if (p.ext[1] > 1) { divmod(t, p.ext[1], t, i); off += (long)i * p.ss[1]; }
        off += t * p.ss[0];
        if (VEC) {                                                         // host: L % 4 == 0, both pointers and every run start 16-byte aligned
            const long e = u << 2;
            *reinterpret_cast<float4 *>(dst + r * p.L + e) = *reinterpret_cast<const float4 *>(src + off + e);
        } else
            dst[r * p.L + u] = src[off + u];
    }
}

// tiles: the innermost source group `a` (source stride 1, output stride da) is not innermost in the output, where group `b` is (output
// stride 1, source stride sb).  A workgroup moves a TA x TB tile through LDS: the fill walks the tile with `a` fastest (contiguous
// reads), the drain with `b` fastest (contiguous writes).  TA and TB are powers of two fitted to the extents (the host's tile rule);
// extents below a tile side are masked.  The LDS pitch TA + 1 is odd: the fill's lanes write consecutive words, the drain's lanes read
// words an odd stride apart, so neither piles onto a bank.  The other groups, at most two, are the batch index with their own source
// and output strides bs / bd: [0] the outer one, [1] the inner one `z` (extent 1 where there is none).  Where both tiled extents are
// narrow the tile takes TZ entries of z as well - TZ planes of TB rows - so that TA * TB * TZ <= 4096 floats keep the lanes busy.
struct TilePlan {
    long nitem;                   // ext0 * ntz * ntb * nta
    long ea, eb, ez;              // extents of a, b and z
    long da, sb;
    long bs[2], bd[2];
    unsigned nta, ntb, ntz;
    unsigned la, lb, lz;          // log2 TA, log2 TB, log2 TZ
};

constexpr int NB = 8;                              // elements of a tile a lane keeps in flight

// Z: the tile takes entries of z (TZ > 1); without it the plane index and its mask are not computed at all
template <bool Z>
__global__ void __launch_bounds__(BLK) k_permute_tiles(const float *__restrict__ src, float *__restrict__ dst, const TilePlan p) {
    extern __shared__ float tile[];                                        // TZ planes of TB rows of TA + 1
    const unsigned TA = 1u << p.la, TB = 1u << p.lb, P = TA + 1, plane = P * TB, lab = p.la + p.lb, cnt = 1u << (lab + p.lz);
    for (long w = blockIdx.x; w < p.nitem; w += gridDim.x) {
        long t = w; unsigned ta = 0, tb = 0, tz = 0;                        // uniform over the workgroup: at most three divisions per tile; t is left as the outer batch index
        if (p.nta > 1) divmod(t, p.nta, t, ta);
        if (p.ntb > 1) divmod(t, p.ntb, t, tb);
        if (p.ntz > 1) divmod(t, p.ntz, t, tz);
        const long a0 = (long)ta << p.la, b0 = (long)tb << p.lb, z0 = (long)tz << p.lz;
        const float *s = src + t * p.bs[0] + z0 * p.bs[1] + b0 * p.sb + a0;
        float *d = dst + t * p.bd[0] + z0 * p.bd[1] + a0 * p.da + b0;
        const long na = p.ea - a0, nb = p.eb - b0, nz = p.ez - z0;          // what is left of the three extents from this tile's corner
        // NB elements of a lane at a time: all their loads are issued before the first LDS store waits for one
        for (unsigned e0 = threadIdx.x; e0 < cnt; e0 += NB * BLK) {
            float v[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const unsigned e = e0 + k * BLK, ia = e & (TA - 1), ib = Z ? (e >> p.la) & (TB - 1) : e >> p.la, iz = Z ? e >> lab : 0;
                v[k] = (e < cnt && ia < na && ib < nb && (!Z || iz < nz)) ? s[(Z ? (long)iz * p.bs[1] : 0L) + (long)ib * p.sb + ia] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const unsigned e = e0 + k * BLK, ia = e & (TA - 1), ib = Z ? (e >> p.la) & (TB - 1) : e >> p.la, iz = Z ? e >> lab : 0;
                if (e < cnt && ia < na && ib < nb && (!Z || iz < nz)) tile[iz * plane + ib * P + ia] = v[k];
            }
        }
        __syncthreads();
        for (unsigned e0 = threadIdx.x; e0 < cnt; e0 += NB * BLK) {
            float v[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const unsigned e = e0 + k * BLK, jb = e & (TB - 1), ja = Z ? (e >> p.lb) & (TA - 1) : e >> p.lb, jz = Z ? e >> lab : 0;
                v[k] = e < cnt ? tile[jz * plane + jb * P + ja] : 0.0f;     // inside the tile's LDS whatever the mask says
            }
#pragma unroll
            for (int k = 0; k < NB; k++) {
                const unsigned e = e0 + k * BLK, jb = e & (TB - 1), ja = Z ? (e >> p.lb) & (TA - 1) : e >> p.lb, jz = Z ? e >> lab : 0;
                if (e < cnt && ja < na && jb < nb && (!Z || jz < nz)) d[(Z ? (long)jz * p.bd[1] : 0L) + (long)ja * p.da + jb] = v[k];
            }
        }
        __syncthreads();                                                   // the tile is rewritten by the next item
    }
}

// what the planner decided, for the launcher and for t4k_permute_plan
struct Plan {
    int family, groups;
    bool vec;
    RunPlan run; TilePlan tl;
};

inline unsigned log2_ceil(long v) { unsigned s = 0; while ((1L << s) < v) s++; return s; }

int check(const int dim[4], const int perm[4], const char *who, long *total) {
    if (!dim || !perm) return fail(T4K_ERR_ARG, "%s: null", who);
    long n = 1; int seen = 0;
    for (int i = 0; i < 4; i++) {
        if (dim[i] < 1) return fail(T4K_ERR_ARG, "%s: extent < 1", who);
        if (n > (1L << 40) / dim[i]) return fail(T4K_ERR_ARG, "%s: more than 2^40 elements", who);
        n *= dim[i];
        if (perm[i] < 0 || perm[i] > 3 || (seen & (1 << perm[i]))) return fail(T4K_ERR_ARG, "%s: perm is not a permutation of 0..3", who);
        seen |= 1 << perm[i];
    }
    *total = n;
    return T4K_OK;
}

// `aligned`: both pointers on 16 bytes
int make_plan(Plan &P, const int dim[4], const int perm[4], bool aligned, const char *who) {
    long sstr[4], d = 1;
    for (int i = 3; i >= 0; i--) { sstr[i] = d; d *= dim[i]; }
    // output order; axes of extent 1 drop out; neighbours merge when the source steps through them as through one axis
    long e[4], s[4]; int n = 0;
    for (int i = 0; i < 4; i++) {
        const int a = perm[i];
        if (dim[a] == 1) continue;
        if (n && s[n - 1] == sstr[a] * dim[a]) { e[n - 1] *= dim[a]; s[n - 1] = sstr[a]; }
        else { e[n] = dim[a]; s[n] = sstr[a]; n++; }
    }
    if (!n) { e[0] = 1; s[0] = 1; n = 1; }                                  // a single element
    P.groups = n; P.vec = false;
    if (s[n - 1] == 1) {                                                   // copy / runs
        RunPlan &p = P.run; p = RunPlan{};
        P.family = n == 1 ? F_COPY : F_RUNS;
        p.L = e[n - 1]; p.R = 1;
        for (int k = 0; k < 3; k++) { p.ext[k] = 1; p.ss[k] = 0; }
        bool str4 = true;
        for (int i = 0; i < n - 1; i++) {                                   // left-aligned: the outermost digit is what the divisions leave
            if (e[i] > 0xffffffffL) return fail(T4K_ERR_ARG, "%s: merged extent too large", who);
            p.ext[i] = (unsigned)e[i]; p.ss[i] = s[i]; p.R *= e[i]; str4 = str4 && !(s[i] & 3);
        }
        P.vec = aligned && (p.L & 3) == 0 && str4;                          // whole runs of float4s, every run of both sides starting on 16 bytes
        p.U = P.vec ? p.L >> 2 : p.L;
        p.shift = 0; while (p.shift < 8 && (1L << p.shift) < p.U) p.shift++;
        p.rpb = (unsigned)BLK >> p.shift;                                  // runs per workgroup iteration (1 once a run fills 256 lanes)
        p.nc = (p.U + BLK - 1) / BLK;                                      // 256-lane chunks per run (1 below that)
        p.nitem = ((p.R + p.rpb - 1) / p.rpb) * p.nc;
        return T4K_OK;
    }
    TilePlan &p = P.tl; p = TilePlan{};
    P.family = F_TILES;
    int ga = 0; while (s[ga] != 1) ga++;                                   // the source's innermost group: some group has stride 1, and it is not the last
    long dstr[4]; d = 1;
    for (int i = n - 1; i >= 0; i--) { dstr[i] = d; d *= e[i]; }
    for (int i = 0; i < n; i++) if (e[i] > 0xffffffffL) return fail(T4K_ERR_ARG, "%s: merged extent too large", who);
    p.ea = e[ga]; p.eb = e[n - 1]; p.da = dstr[ga]; p.sb = s[n - 1];
    p.bs[0] = p.bs[1] = p.bd[0] = p.bd[1] = 0; p.ez = 1;
    long outer = 1;
    for (int i = n - 2, k = 1; i >= 0; i--) {                               // right-aligned: the inner batch group is z
        if (i == ga) continue;
        p.bs[k] = s[i]; p.bd[k] = dstr[i];
        if (k) p.ez = e[i]; else outer = e[i];
        k--;
    }
    // the tile fits the shape: each side the smallest power of two >= min(extent, 64); the side with room grows until the tile holds 4096
    // floats; two narrow sides leave room for entries of z
    p.la = log2_ceil(std::min(p.ea, 64L)); p.lb = log2_ceil(std::min(p.eb, 64L)); p.lz = 0;
    while (p.la + p.lb < 12 && (1L << p.la) < p.ea) p.la++;
    while (p.la + p.lb < 12 && (1L << p.lb) < p.eb) p.lb++;
    while (p.la + p.lb + p.lz < 12 && (1L << p.lz) < p.ez) p.lz++;
    const long nta = (p.ea + (1L << p.la) - 1) >> p.la, ntb = (p.eb + (1L << p.lb) - 1) >> p.lb, ntz = (p.ez + (1L << p.lz) - 1) >> p.lz;
    p.nta = (unsigned)nta; p.ntb = (unsigned)ntb; p.ntz = (unsigned)ntz;
    p.nitem = outer * ntz * nta * ntb;
    return T4K_OK;
}

} // namespace

extern "C" {

int t4k_permute(const float *src, float *dst, const int dim[4], const int perm[4], t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!src || !dst) return fail(T4K_ERR_ARG, "t4k_permute: null");
    long total; Plan P;
    int rc = check(dim, perm, "t4k_permute", &total); if (rc != T4K_OK) return rc;
    if (src < dst + total && dst < src + total) return fail(T4K_ERR_ARG, "t4k_permute: dst overlaps src");
    rc = make_plan(P, dim, perm, aligned16(src) && aligned16(dst), "t4k_permute"); if (rc != T4K_OK) return rc;
    if (P.family == F_TILES) {
        const TilePlan &p = P.tl;
        const int g = (int)std::min(p.nitem, (long)MAX_WG);
        const size_t lds = ((((size_t)1 << p.la) + 1) << (p.lb + p.lz)) * sizeof(float);      // <= 24 KiB (TA = 2: 3 x 2048 floats)
        with_flags([&](auto z) { T4K_LAUNCH((k_permute_tiles<z.value>), dim3(g), dim3(BLK), lds, S(s), src, dst, p); }, p.lz > 0);
    } else {
        const RunPlan &p = P.run;
        const int g = (int)std::min(p.nitem, (long)MAX_WG);
        with_flags([&](auto v) { T4K_LAUNCH((k_permute_runs<v.value>), dim3(g), dim3(BLK), 0, S(s), src, dst, p); }, P.vec);
    }
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

int t4k_permute_plan(const int dim[4], const int perm[4], int aligned, int out[7]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_permute_plan: null");
    long total; Plan P;
    int rc = check(dim, perm, "t4k_permute_plan", &total); if (rc != T4K_OK) return rc;
    rc = make_plan(P, dim, perm, aligned != 0, "t4k_permute_plan"); if (rc != T4K_OK) return rc;
    const bool tiles = P.family == F_TILES;
    out[0] = P.family; out[1] = P.vec ? 1 : 0;
    out[2] = tiles ? 1 << P.tl.la : 1 << P.run.shift;
    out[3] = tiles ? 1 << P.tl.lb : (int)P.run.rpb;
    out[4] = (int)std::min(tiles ? P.tl.nitem : P.run.nitem, 0x7fffffffL);
    out[5] = P.groups;
    out[6] = tiles ? 1 << P.tl.lz : 1;
    return T4K_OK;
}

} // extern "C"
