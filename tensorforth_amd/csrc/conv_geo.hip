// conv_geo.hip - conv2d with RUN-TIME geometry: any K 1..7, stride 1..4, dilation 1..4, padding 0..D(K-1) (t4k_conv2d_geo_fwd / _bwd / _plan).
//
// conv.hip's gather body and conv_big.hip's k_convbig are compiled around Geo<K, S, P> (launch.h: the reference's four cases, forward.cu:142-151);
// here K, S, P, D are kernel ARGUMENTS and the templates name only the load path.  Three implicit GEMMs, exact fp32 on v_mfma_f32_32x32x2_f32:
//   forward  O[pix, c0]  = B[c0] + sum_{tap, c1} I[pix*S + tap*D - P, c1] * F[c1, tap, c0]
//   dX       dX[pix, c1] = sum_{tap, c0} dO[(pix + P - tap*D) / S, c0] * F[c1, tap, c0]      over the taps that divide: the TEXTBOOK gradient, not the
//            reference's rotated-filter one (quirk a-11 stays with the four geometries the reference computes)
//   dF | dB  slab[slice][(c1, tap) | bias][c0] = sum_{pix of the slice} I[pix*S + tap*D - P, c1] * dO[pix, c0], folded in slice order by colsum.h
// k_geo serves forward and dX.  Its pixels are those of ONE residue class (y mod S, x mod S) of the produced grid - the forward has one class, the whole
// output - because inside a class every pixel has the same contributing taps: those ky with (ry + P - ky D) % S == 0, at row offset (ry + P - ky D) / S of
// the class grid.  A workgroup is (class, 128 pixels of it, BN channels) and contracts over the class's OWN tap list x channels: no divisibility test per
// tap, none of the (S^2 - 1) / S^2 wasted MFMAs of a gather over all K^2 taps.  A class without taps (S above the dilated window; rows behind the last
// window) stores zeros.  Every element of the produced tensor is stored exactly once; no atomics; fixed summation order.
// A k-step is 32 channels of one tap: the A gather is one contiguous run per pixel (16-byte loads when the channel count is a multiple of 4 and the
// tensor sits on 16 bytes, dwords otherwise), a tap outside the image or a channel past the end contributes zeros by predicate - nothing outside the
// tensors is read.  Row / column validity of every tap is two 7-bit masks per pixel, worked out once per tile.
// k_geo_dft's stage pipeline is conv_big.hip's k_convbig_df's, written once in conv_tile.h (conv_df_tile4); admission and the slice planner are shared with
// conv_group.hip (conv_types.h).
#include "conv_tile.h"

namespace {

constexpr int GBK = 32, GCH = GBK / 4, GSW = 64 / GBK, GNC = GBK / 8, GBM = 128;

struct GeoP {
    const float *X, *F, *B;            // gathered tensor (forward: I, dX: dO), filter [C1][K][K][C0], bias (forward)
    float *Y, *Y2;                     // produced tensor (+ optional second copy)
    int N, Hx, Wx, Cin;                // gathered grid
    int Hy, Wy, Cout;                  // produced grid
    int C0f;                           // the filter's inner extent
    int K, S, P, D;
    int tiles_n, cpt;                  // channel tiles; 32-channel k-steps per tap
};

// pixels of residue class r of an extent H under stride S
__host__ __device__ inline int class_extent(int H, int r, int S) { return r < H ? (H - r + S - 1) / S : 0; }

template <bool BWD, bool VA, bool VB, int BN>
__global__ void __launch_bounds__(256) k_geo(GeoP p) {
    constexpr int BM = GBM, BK = GBK, CH = GCH, SW = GSW, MT = BM / 64, NT = BN / 64;
    constexpr int PA = BM * BK / 1024, PB = BN * BK / 1024;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // the static block lies in front of the dynamic one: its size stays a multiple of 16 bytes, or the ds_read_b128 of the A stage would lose their alignment
    struct Sm { int dy[8], dx[8], ky[8], kx[8], cnt[4], opix[BM]; };
    static_assert(sizeof(Sm) % 16 == 0, "k_geo: static LDS must keep the dynamic stage buffers on 16 bytes");
    __shared__ __attribute__((aligned(16))) Sm sm;
    int *const s_dy = sm.dy, *const s_dx = sm.dx, *const s_ky = sm.ky, *const s_kx = sm.kx, *const s_cnt = sm.cnt, *const s_opix = sm.opix;
    float *sA = lds, *sB = lds + 2 * BM * BK;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, h = lane >> 5, l31 = lane & 31;
    const int K = p.K, KK = K * K, Cin = p.Cin, Cout = p.Cout;
    const int tn = blockIdx.x % p.tiles_n;
    int tm = blockIdx.x / p.tiles_n;
    // the class of this workgroup and its pixel grid (forward: the whole output)
    int ry = 0, rx = 0, Hc = p.Hy, Wc = p.Wy;
    if (BWD) {
        for (int cls = 0; cls < p.S * p.S; cls++) {
            ry = cls / p.S; rx = cls - ry * p.S;
            Hc = class_extent(p.Hy, ry, p.S); Wc = class_extent(p.Wy, rx, p.S);
            const int t = (int)(((long)p.N * Hc * Wc + BM - 1) / BM);
            if (tm < t) break;
            tm -= t;
        }
    }
    const long npc = (long)p.N * Hc * Wc;
    const long m0 = (long)tm * BM;
    const int n0 = tn * BN;
    const int SS = BWD ? 1 : p.S, OS = BWD ? p.S : 1;    // gather step and store step per class pixel
    if (tid == 0) {                                      // the class's tap lists: offsets into the gathered grid, and the filter's own ky / kx
        int ny = 0, nx = 0;
        for (int k = 0; k < K; k++) {
            if (!BWD) { s_dy[ny] = k * p.D - p.P; s_ky[ny++] = k; s_dx[nx] = k * p.D - p.P; s_kx[nx++] = k; }
            else {
                const int ty = ry + p.P - k * p.D, tx = rx + p.P - k * p.D;
                if (ty % p.S == 0) { s_dy[ny] = ty / p.S; s_ky[ny++] = k; }
                if (tx % p.S == 0) { s_dx[nx] = tx / p.S; s_kx[nx++] = k; }
            }
        }
        s_cnt[0] = ny; s_cnt[1] = nx;
    }
    if (tid < BM) {                                      // where row `tid` of the tile is stored: a pixel index of the produced tensor, -1 past the class
        const long m = m0 + tid;
        int op = -1;
        if (m < npc) {
            const unsigned q = (unsigned)m, t = q / (unsigned)Wc, n = t / (unsigned)Hc;
            const int px = (int)(q - t * (unsigned)Wc), py = (int)(t - n * (unsigned)Hc);
            op = ((int)n * p.Hy + ry + py * OS) * p.Wy + rx + px * OS;
        }
        s_opix[tid] = op;
    }
    __syncthreads();
    const int nky = s_cnt[0], nkx = s_cnt[1];
    const int nst = nky * nkx * p.cpt;

    // this thread's A rows (pixels) and its 16-byte chunk of a k-step's 32 channels
    long pbase[PA]; unsigned vmask[PA];
    const int aq = tid % CH;
#pragma unroll
    for (int pp = 0; pp < PA; pp++) {
        const long m = m0 + pp * (256 / CH) + tid / CH;
        const bool pok = m < npc;
        const unsigned q = pok ? (unsigned)m : 0u, t = q / (unsigned)Wc, n = t / (unsigned)Hc;
        const int gx0 = (int)(q - t * (unsigned)Wc) * SS, gy0 = (int)(t - n * (unsigned)Hc) * SS;
        pbase[pp] = (((long)n * p.Hx + gy0) * p.Wx + gx0) * Cin + aq * 4;
        unsigned v = 0;
        for (int a = 0; a < nky; a++) if ((unsigned)(gy0 + s_dy[a]) < (unsigned)p.Hx) v |= 1u << a;
        for (int b = 0; b < nkx; b++) if ((unsigned)(gx0 + s_dx[b]) < (unsigned)p.Wx) v |= 256u << b;
        vmask[pp] = pok ? v : 0u;
    }
    v4f ra[PA], rb[PB];
    auto load_tiles = [&](int kt) __attribute__((always_inline)) {
        const int tap = kt / p.cpt, cb = (kt - tap * p.cpt) * BK;
        const int a = tap / nkx, b = tap - a * nkx;
        const int ftap = s_ky[a] * K + s_kx[b];
        const long shift = ((long)s_dy[a] * p.Wx + s_dx[b]) * Cin + cb;
        const v4f z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pp = 0; pp < PA; pp++) {
            const bool ok = ((vmask[pp] >> a) & (vmask[pp] >> (8 + b)) & 1u) != 0;
            const int c = cb + aq * 4;
            const float *src = p.X + (pbase[pp] + shift);
            if (VA) ra[pp] = (ok && c < Cin) ? *reinterpret_cast<const v4f *>(src) : z;
            else {
#pragma unroll
                for (int e = 0; e < 4; e++) ra[pp][e] = (ok && c + e < Cin) ? src[e] : 0.f;
            }
        }
#pragma unroll
        for (int pp = 0; pp < PB; pp++) {
            const int id = pp * 256 + tid;
            if (!BWD) {                                          // B[k = c1][n = c0] = F[c1][tap][c0]: n-contiguous
                const int kk = id / (BN / 4), rq = id % (BN / 4), n = n0 + rq * 4, c = cb + kk;
                const float *src = p.F + ((long)c * KK + ftap) * p.C0f + n;
                if (VB) rb[pp] = (c < Cin && n < Cout) ? *reinterpret_cast<const v4f *>(src) : z;
                else {
#pragma unroll
                    for (int e = 0; e < 4; e++) rb[pp][e] = (c < Cin && n + e < Cout) ? src[e] : 0.f;
                }
            } else {                                             // B[n = c1][k = c0] = F[c1][tap][c0]: k-contiguous
                const int r = id / CH, q = id % CH, n = n0 + r, c = cb + q * 4;
                const float *src = p.F + ((long)n * KK + ftap) * p.C0f + c;
                if (VB) rb[pp] = (n < Cout && c < Cin) ? *reinterpret_cast<const v4f *>(src) : z;
                else {
#pragma unroll
                    for (int e = 0; e < 4; e++) rb[pp][e] = (n < Cout && c + e < Cin) ? src[e] : 0.f;
                }
            }
        }
    };
    int soa[PA], sob[PB];
#pragma unroll
    for (int pp = 0; pp < PA; pp++) { const int id = pp * 256 + tid, r = id / CH, q = id % CH; soa[pp] = r * BK + ((q ^ ((r / SW) & (CH - 1))) << 2); }
#pragma unroll
    for (int pp = 0; pp < PB; pp++) {
        const int id = pp * 256 + tid;
        if (BWD) { const int r = id / CH, q = id % CH; sob[pp] = r * BK + ((q ^ ((r / SW) & (CH - 1))) << 2); }
        else     sob[pp] = (id / (BN / 4)) * BN + (id % (BN / 4)) * 4;
    }
    auto store_tiles = [&](int buf) __attribute__((always_inline)) {
        float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
        for (int pp = 0; pp < PA; pp++) *reinterpret_cast<v4f *>(a + soa[pp]) = ra[pp];
#pragma unroll
        for (int pp = 0; pp < PB; pp++) *reinterpret_cast<v4f *>(b + sob[pp]) = rb[pp];
    };
    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

    if (nst > 0) { load_tiles(0); store_tiles(0); }
    __syncthreads();
    for (int kt = 0; kt < nst; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nst) load_tiles(kt + 1);                     // in flight during the MFMAs below
        const float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
        for (int ci = 0; ci < GNC; ci++) {                        // lane half h holds k = 8*ci + 4*h + {0..3}
            float av[MT][4], bv[NT][4];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int r = wm * (BM / 2) + mt * 32 + l31;
                const v4f t = *reinterpret_cast<const v4f *>(a + r * BK + (((ci * 2 + h) ^ ((r / SW) & (CH - 1))) << 2));
                av[mt][0] = t[0]; av[mt][1] = t[1]; av[mt][2] = t[2]; av[mt][3] = t[3];
            }
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                const int r = wn * (BN / 2) + nt * 32 + l31;
                if (BWD) { const v4f t = *reinterpret_cast<const v4f *>(b + r * BK + (((ci * 2 + h) ^ ((r / SW) & (CH - 1))) << 2));
                           bv[nt][0] = t[0]; bv[nt][1] = t[1]; bv[nt][2] = t[2]; bv[nt][3] = t[3]; }
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) bv[nt][j] = b[(ci * 8 + 4 * h + j) * BN + r];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int nt = 0; nt < NT; nt++)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][j], bv[nt][j], acc[mt][nt], 0, 0, 0);
        }
        if (kt + 1 < nst) store_tiles(buf ^ 1);
        __syncthreads();
    }
    // epilogue: col = lane & 31, row = frag_row(r, h); the bias rides here (forward)
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const int gn = n0 + wn * (BN / 2) + nt * 32 + l31;
            if (gn >= Cout) continue;
            const float bias = (!BWD && p.B) ? p.B[gn] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int op = s_opix[wm * (BM / 2) + mt * 32 + frag_row(r, h)];
                if (op >= 0) { const float v = acc[mt][nt][r] + bias; p.Y[(long)op * Cout + gn] = v; if (p.Y2) p.Y2[(long)op * Cout + gn] = v; }
            }
        }
}

// ------------------------------------------------------------------ dF | dB partial slabs
// grid = (slices, row tiles, c0 tiles); tile 64 rows x 64 c0, the contraction = the slice's output pixels, 32 per stage.  The rows are (c1, ky, kx) in the
// filter's own order plus ONE spare row whose A operand is 1: it yields dB.  A thread keeps ONE pixel of the stage and eight rows: a row's tap offset and
// channel are worked out once, a pixel's (n, y, x) once per stage.  Every element of every slab is stored (an empty slice stores zeros).
struct GeoD { const float *I, *DO; float *part; int N, H1, W1, C1, H0, W0, C0, K, S, P, D; int pps; };

template <bool VB>
__global__ void __launch_bounds__(256) k_geo_df(GeoD p) {
    constexpr int BM = 64, BN = 64, BKP = 32, PM = BM + 1;        // A rows are stored a pixel per lane: an odd pitch keeps the 32 banks apart
    __shared__ __attribute__((aligned(16))) float sA[2][BKP * PM];
    __shared__ __attribute__((aligned(16))) float sB[2][BKP * BN];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, h = lane >> 5, l31 = lane & 31;
    const int K = p.K, KK = K * K, ntaps = p.C1 * KK;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.z * BN;
    const long npix = (long)p.N * p.H0 * p.W0;
    const long k_beg = (long)blockIdx.x * p.pps, k_end = min(npix, k_beg + p.pps);
    const int nst = k_end > k_beg ? (int)((k_end - k_beg + BKP - 1) / BKP) : 0;
    const int kk = tid & 31, mg = tid >> 5;
    long roff[8]; int rk[8];                                      // per row: offset of (tap, c1) from the window's corner; ky D | kx D << 8 | kind << 16 (0 row, 1 bias, 2 none)
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int row = m0 + mg + 8 * j;
        if (row < ntaps) {
            const int c1 = row / KK, tap = row - c1 * KK, ky = tap / K, kx = tap - ky * K;
            roff[j] = ((long)ky * p.D * p.W1 + kx * p.D) * p.C1 + c1;
            rk[j] = (ky * p.D) | ((kx * p.D) << 8);
        } else { roff[j] = 0; rk[j] = (row == ntaps ? 1 : 2) << 16; }
    }
    float ra[8]; v4f rb[2]; float rbs[8];
    auto load_tiles = [&](int kt) __attribute__((always_inline)) {
        const long k0 = k_beg + (long)kt * BKP, pix = k0 + kk;
        const bool in = pix < k_end;
        const unsigned q = in ? (unsigned)pix : 0u, t = q / (unsigned)p.W0, n = t / (unsigned)p.H0;
        const int ix0 = (int)(q - t * (unsigned)p.W0) * p.S - p.P, iy0 = (int)(t - n * (unsigned)p.H0) * p.S - p.P;
        const long pb = (((long)n * p.H1 + iy0) * p.W1 + ix0) * p.C1;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int kind = rk[j] >> 16, gi = iy0 + (rk[j] & 255), gj = ix0 + ((rk[j] >> 8) & 255);
            const bool ok = in && kind == 0 && (unsigned)gi < (unsigned)p.H1 && (unsigned)gj < (unsigned)p.W1;
            ra[j] = ok ? p.I[pb + roff[j]] : ((in && kind == 1) ? 1.f : 0.f);
        }
        if (VB) {
#pragma unroll
            for (int pp = 0; pp < 2; pp++) {                      // B[k = pixel][n = c0] = dO[pixel][c0]
                const int id = pp * 256 + tid, bk = id / (BN / 4), rq = id % (BN / 4), n1 = n0 + rq * 4;
                const v4f z = {0.f, 0.f, 0.f, 0.f};
                rb[pp] = (k0 + bk < k_end && n1 < p.C0) ? *reinterpret_cast<const v4f *>(p.DO + (k0 + bk) * p.C0 + n1) : z;
            }
        } else {
#pragma unroll
            for (int pp = 0; pp < 8; pp++) {
                const int id = pp * 256 + tid, bk = id / BN, n1 = n0 + id % BN;
                rbs[pp] = (k0 + bk < k_end && n1 < p.C0) ? p.DO[(k0 + bk) * p.C0 + n1] : 0.f;
            }
        }
    };
    auto store_tiles = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 8; j++) sA[buf][kk * PM + mg + 8 * j] = ra[j];
        if (VB) {
#pragma unroll
            for (int pp = 0; pp < 2; pp++) { const int id = pp * 256 + tid; *reinterpret_cast<v4f *>(&sB[buf][(id / (BN / 4)) * BN + (id % (BN / 4)) * 4]) = rb[pp]; }
        } else {
#pragma unroll
            for (int pp = 0; pp < 8; pp++) sB[buf][pp * 256 + tid] = rbs[pp];
        }
    };
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }
    if (nst > 0) { load_tiles(0); store_tiles(0); }
    __syncthreads();
    for (int kt = 0; kt < nst; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nst) load_tiles(kt + 1);
        const float *a = sA[buf], *b = sB[buf];
        const int ra_ = wm * 32 + l31, rb_ = wn * 32 + l31;
#pragma unroll
        for (int ci = 0; ci < BKP / 8; ci++) {
            float av[4], bv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { av[j] = a[(ci * 8 + 4 * h + j) * PM + ra_]; bv[j] = b[(ci * 8 + 4 * h + j) * BN + rb_]; }
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], bv[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], bv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], bv[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], bv[3], acc1, 0, 0, 0);
        }
        if (kt + 1 < nst) store_tiles(buf ^ 1);
        __syncthreads();
    }
    // slab [slice][row][c0], row C1 K K = the bias row (the fold's layout: outputs [0, ndf) are dF, [ndf, ntot) dB)
    const int co = n0 + wn * 32 + l31;
    if (co < p.C0) {
        const long ntot = (long)(ntaps + 1) * p.C0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (row <= ntaps) p.part[(long)blockIdx.x * ntot + (long)row * p.C0 + co] = acc0[r] + acc1[r];
        }
    }
}

// the same slabs for many input channels (C1 % 4 == 0, C1 >= 32, everything on 16 bytes): a tile's 64 rows are 64 channels of ONE tap, so a row of the A stage is
// one contiguous run of the input pixel under that tap - 16-byte loads instead of the dwords of k_geo_df (conv_big.hip's k_convbig_df with the geometry in
// arguments: the same conv_df_tile4, conv_tile.h).  grid.y = taps x channel tiles, plus ONE tile whose first row is all ones: the bias row.
__global__ void __launch_bounds__(256) k_geo_dft(GeoD p, int ci_tiles) {
    constexpr int BM = 64, BN = 64, BKP = 32;
    __shared__ __attribute__((aligned(16))) float sA[2][BKP * BM];
    __shared__ __attribute__((aligned(16))) float sB[2][BKP * BN];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, h = lane >> 5, l31 = lane & 31;
    const int K = p.K, KK = K * K, ntaps = p.C1 * KK;
    const bool bias_tile = (int)blockIdx.y == KK * ci_tiles;
    const int tap = bias_tile ? 0 : blockIdx.y / ci_tiles, cit = bias_tile ? 0 : blockIdx.y - tap * ci_tiles;
    const int ky = tap / K, kx = tap - ky * K;
    const int m0 = cit * BM, n0 = blockIdx.z * BN;
    const long npix = (long)p.N * p.H0 * p.W0;
    const long k_beg = (long)blockIdx.x * p.pps, k_end = min(npix, k_beg + p.pps);
    const int nst = k_end > k_beg ? (int)((k_end - k_beg + BKP - 1) / BKP) : 0;
    const int rq = tid & 15, kq = tid >> 4;                      // this thread's 16-byte column of a stage row, and its rows kq, kq + 16
    const int dy = ky * p.D - p.P, dx = kx * p.D - p.P;
    v4f ra[2], rb[2];
    auto load_tiles = [&](int kt) __attribute__((always_inline)) {
        const long k0 = k_beg + (long)kt * BKP;
        const v4f z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            const long pix = k0 + kq + pp * 16;
            const bool in = pix < k_end;
            if (bias_tile) { ra[pp] = z; ra[pp][0] = (in && rq == 0) ? 1.f : 0.f; }
            else {
                const unsigned q = in ? (unsigned)pix : 0u, t = q / (unsigned)p.W0, n = t / (unsigned)p.H0;
                const int gj = (int)(q - t * (unsigned)p.W0) * p.S + dx, gi = (int)(t - n * (unsigned)p.H0) * p.S + dy;
                const int m = m0 + rq * 4;
                const bool ok = in && m < p.C1 && (unsigned)gi < (unsigned)p.H1 && (unsigned)gj < (unsigned)p.W1;
                ra[pp] = ok ? *reinterpret_cast<const v4f *>(p.I + (((long)n * p.H1 + gi) * p.W1 + gj) * p.C1 + m) : z;
            }
            const int n1 = n0 + rq * 4;
            rb[pp] = (in && n1 < p.C0) ? *reinterpret_cast<const v4f *>(p.DO + pix * p.C0 + n1) : z;
        }
    };
    auto store_tiles = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int pp = 0; pp < 2; pp++) {
            *reinterpret_cast<v4f *>(&sA[buf][(kq + pp * 16) * BM + rq * 4]) = ra[pp];
            *reinterpret_cast<v4f *>(&sB[buf][(kq + pp * 16) * BN + rq * 4]) = rb[pp];
        }
    };
    f32x16 acc0, acc1;
    conv_df_tile4(&sA[0][0], &sB[0][0], nst, acc0, acc1, load_tiles, store_tiles);
    const int co = n0 + wn * 32 + l31;
    if (co < p.C0) {
        const long ntot = (long)(ntaps + 1) * p.C0;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int m = wm * 32 + frag_row(r, h), ci = m0 + m;
            if (bias_tile) { if (m == 0) p.part[(long)blockIdx.x * ntot + (long)ntaps * p.C0 + co] = acc0[r] + acc1[r]; }
            else if (ci < p.C1) p.part[(long)blockIdx.x * ntot + ((long)ci * KK + tap) * p.C0 + co] = acc0[r] + acc1[r];
        }
    }
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_conv2d_geo_plan reports
struct GeoPlan {
    int H0, W0;
    int fwd_bn, fwd_va, fwd_vb;        // forward: channel tile (the pixel tile is 128), 16-byte gather of I, 16-byte loads of F
    int dx_bn, dx_v;                   // dX: channel tile, 16-byte loads of dO and F
    int df_vb, df_tap, nslice, pps, fold;   // dF: 16-byte loads of dO, the tap-per-tile kernel with its 16-byte gather of I, slices, pixels per slice, the fold (1 fold_add, 2 df_fold)
};
// admission (who: the entry's name for the message) and the plan.  T4K_ERR_ARG: an extent below 1; T4K_ERR_UNSUPPORTED: a geometry outside the admitted set
int geo_plan(GeoPlan &g, const char *who, int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D, bool aligned, bool db_adjacent) {
    const int rc = conv_geo_admit(who, N, H1, W1, C1, C0, K, S, P, D, nullptr, &g.H0, &g.W0); if (rc != T4K_OK) return rc;
    const long np0 = (long)N * g.H0 * g.W0, np1 = (long)N * H1 * W1, ntot = ((long)C1 * K * K + 1) * C0;
    if (((long)C1 * K * K + 64) / 64 > 65535 || (C0 + 63) / 64 > 65535 ||                                  // the dF grid's y and z, the 1-D grids of forward and dX
        ((np0 + GBM - 1) / GBM) * ((C0 + 63) / 64) >= (1L << 31) || ((np1 + GBM - 1) / GBM + 16) * ((C1 + 63) / 64) >= (1L << 31))
        return fail(T4K_ERR_UNSUPPORTED, "%s: more tiles than a launch takes", who);
    g.fwd_va = aligned && C1 % 4 == 0; g.fwd_vb = aligned && C0 % 4 == 0;
    g.fwd_bn = (g.fwd_va && g.fwd_vb && C0 > 64) ? 128 : 64;
    g.dx_v = aligned && C0 % 4 == 0;
    g.dx_bn = (g.dx_v && C1 > 64) ? 128 : 64;
    g.df_vb = aligned && C0 % 4 == 0;
    g.df_tap = g.df_vb && C1 % 4 == 0 && C1 >= 32;              // below 32 channels a tap fills less than half of a tile's rows: (c1, tap) rows side by side then
    const long tiles = (g.df_tap ? (long)K * K * ((C1 + 63) / 64) + 1 : ((long)C1 * K * K + 1 + 63) / 64) * ((C0 + 63) / 64);
    const SlabPlan sp = slab_plan(np0, tiles, ntot, db_adjacent, 0x7fffffe0);     // (GeoD::pps is an int)
    g.pps = (int)sp.pps; g.nslice = sp.nslice; g.fold = sp.fold;
    return T4K_OK;
}

int geo_tiles_m(bool bwd, int N, int Hy, int Wy, int S) {
    if (!bwd) return (int)(((long)N * Hy * Wy + GBM - 1) / GBM);
    long t = 0;
    for (int ry = 0; ry < S; ry++)
        for (int rx = 0; rx < S; rx++) t += ((long)N * class_extent(Hy, ry, S) * class_extent(Wy, rx, S) + GBM - 1) / GBM;
    return (int)t;
}

template <bool BWD>
void launch_geo(const GeoP &p, bool va, bool vb, int bn, hipStream_t hs) {
    const int tiles_m = geo_tiles_m(BWD, p.N, p.Hy, p.Wy, p.S);
    const dim3 grid((unsigned)tiles_m * (unsigned)p.tiles_n);
    const size_t lds = (size_t)2 * (GBM + bn) * GBK * sizeof(float);
    if (bn == 128) { launch_lds<k_geo<BWD, true, true, 128>>(grid, dim3(256), lds, hs, p); return; }
    if constexpr (BWD) with_flags([&](auto v) { launch_lds<k_geo<BWD, v.value, v.value, 64>>(grid, dim3(256), lds, hs, p); }, va);
    else               with_flags([&](auto a, auto b) { launch_lds<k_geo<BWD, a.value, b.value, 64>>(grid, dim3(256), lds, hs, p); }, va, vb);
}

} // namespace

extern "C" {

int t4k_conv2d_geo_plan(int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D, int aligned, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_conv2d_geo_plan: null");
    GeoPlan g;
    const int rc = geo_plan(g, "t4k_conv2d_geo_plan", N, H1, W1, C1, C0, K, S, P, D, (aligned & 1) != 0, !(aligned & 2)); if (rc != T4K_OK) return rc;
    out[0] = g.fwd_bn; out[1] = g.fwd_va | (g.fwd_vb << 1);
    out[2] = g.dx_bn;  out[3] = g.dx_v;
    out[4] = g.df_vb | (g.df_tap << 1);  out[5] = g.nslice; out[6] = g.fold; out[7] = 3;
    return T4K_OK;
}

int t4k_conv2d_geo_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, int D, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    ConvPlanScope plan;
    if (!I || !O || !F || !B) return fail(T4K_ERR_ARG, "t4k_conv2d_geo_fwd: null tensor");
    GeoPlan g;
    const int rc = geo_plan(g, "t4k_conv2d_geo_fwd", N, H1, W1, C1, C0, K, S, P, D, all16(I, F), true); if (rc != T4K_OK) return rc;
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_conv2d_geo_fwd: output %dx%d, the geometry gives %dx%d", H0, W0, g.H0, g.W0);
    hipStream_t hs = t4k::S(s);
    if (ICOPY) { conv_plan_note("memcpy"); T4K_HIP(hipMemcpyAsync(ICOPY, I, sizeof(float) * (size_t)N * H1 * W1 * C1, hipMemcpyDeviceToDevice, hs)); }
    GeoP p = { I, F, B, O, nullptr, N, H1, W1, C1, H0, W0, C0, C0, K, S, P, D, (C0 + g.fwd_bn - 1) / g.fwd_bn, (C1 + GBK - 1) / GBK };
    conv_plan_note("geo<%d,%s,%s>", g.fwd_bn, g.fwd_va ? "v4" : "v1", g.fwd_vb ? "f4" : "f1");
    launch_geo<false>(p, g.fwd_va, g.fwd_vb, g.fwd_bn, hs);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

int t4k_conv2d_geo_bwd(const float *I, const float *DO, float *DX, float *DX2, const float *F, float *DF, float *DB,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, int D, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    ConvPlanScope plan;
    if (!I || !DO || !F) return fail(T4K_ERR_ARG, "t4k_conv2d_geo_bwd: null tensor");
    if ((DF == nullptr) != (DB == nullptr)) return fail(T4K_ERR_ARG, "t4k_conv2d_geo_bwd: DF and DB go together");
    GeoPlan g;
    // every 16-byte path of the backward needs ALL of its operands on 16 bytes: dO and F for dX, dO (and I, tap per tile) for dF - one flag, as the plan entry takes it
    const int rc = geo_plan(g, "t4k_conv2d_geo_bwd", N, H1, W1, C1, C0, K, S, P, D, all16(DO, F, I), DF && DB == DF + (long)C1 * K * K * C0); if (rc != T4K_OK) return rc;
    if (H0 != g.H0 || W0 != g.W0) return fail(T4K_ERR_ARG, "t4k_conv2d_geo_bwd: output %dx%d, the geometry gives %dx%d", H0, W0, g.H0, g.W0);
    hipStream_t hs = t4k::S(s);
    if (train && DF) {                                           // stage 1 reads I, which DX2 may overwrite: slabs, then their fold in slice order
        if (st().ws_bytes / 2 < CONV_WS_BYTES) return fail(T4K_ERR_NOMEM, "t4k_conv2d_geo_bwd: workspace");
        float *part = ws_for(s);
        const int ntaps = C1 * K * K, ndf = ntaps * C0, ntot = ndf + C0;
        GeoD d = { I, DO, part, N, H1, W1, C1, H0, W0, C0, K, S, P, D, g.pps };
        conv_plan_note("geo_dfx%d<%s>", g.nslice, g.df_tap ? "tap" : g.df_vb ? "rows,d4" : "rows,d1");
        if (g.df_tap) {
            const int ci_tiles = (C1 + 63) / 64;
            T4K_LAUNCH(k_geo_dft, dim3(g.nslice, K * K * ci_tiles + 1, (C0 + 63) / 64), dim3(256), 0, hs, d, ci_tiles);
        } else {
            const dim3 grid(g.nslice, (ntaps + 1 + 63) / 64, (C0 + 63) / 64);
            with_flags([&](auto v) { T4K_LAUNCH((k_geo_df<v.value>), grid, dim3(256), 0, hs, d); }, g.df_vb != 0);
        }
        if (g.fold == 1) { conv_plan_note("fold_add"); launch_fold_add(part, DF, ntot, g.nslice, hs); }
        else             { conv_plan_note("df_fold");  launch_df_fold(part, DF, DB, g.nslice, ndf, ntot, hs); }
    }
    if (DX) {                                                    // gather over dO (Cin = C0), produce the input grid (Cout = C1)
        GeoP p = { DO, F, nullptr, DX, DX2, N, H0, W0, C0, H1, W1, C1, C0, K, S, P, D, (C1 + g.dx_bn - 1) / g.dx_bn, (C0 + GBK - 1) / GBK };
        conv_plan_note("geo_dx<%d,%s>", g.dx_bn, g.dx_v ? "v4" : "v1");
        launch_geo<true>(p, g.dx_v, g.dx_v, g.dx_bn, hs);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
