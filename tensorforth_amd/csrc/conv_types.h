// conv_types.h - what the convolution units share (conv.hip, conv_few.hip, conv_big.hip, conv_geo.hip, conv_group.hip, conv_img.hip, dconv.hip): every host
// function that crosses a unit, declared once with its default arguments; the pending-fold block; the LAB switches; the dF slice planners and the admission
// of the run-time-geometry layers.  Every kernel template is instantiated in exactly
// one unit - the one that launches it.
#pragma once
#include "launch.h"
#include "colsum.h"
#include <algorithm>

namespace t4k {
// ---- conv_few.hip: thread-per-pixel vector kernels for few channels
// forward / dX with Cin <= 4 and Cout <= 32 (K 3 or 5): true when the shape is served, *G / *NG = channels per group / groups
bool conv_few_ok(int K, int Cin, int Cout, int *G, int *NG);
template <bool BWD>
void launch_conv_few(int K, hipStream_t hs, const float *X, float *Y, float *Y2, float *XC, const float *F, const float *B,
                     int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout, int C0f, int G, int NG);
// the dF fold a dX launch may carry in its first `nfold` workgroups (nfold == 0: nothing pending); see k_conv_dx_and_fold
struct FoldArgs { const float *part; float *DF, *DB; int nslice, ndf, ntot, nfold; };
// dX of an image-input layer (C1 <= 4, filter within the LDS stage): k_conv_dx_wide or k_conv_dx_few, either carries `fa`
// (k_conv_dx_few reads dO 16 bytes at a time when C0 % 4 == 0 and 8 when C0 is even: DO must sit on that boundary, or the gather kernel takes the layer)
bool conv_dx_few_ok(int K, int C1, int C0, const float *DO);
void launch_conv_dx_few(int K, int S, int P, hipStream_t hs, const float *DO, float *DX, float *DX2, const float *F,
                        int N, int H0, int W0, int C0, int H1, int W1, int C1, FoldArgs fa);

// ---- conv_big.hip: LDS-staged MFMA GEMM tiling for many channels
bool conv_big_ok(int Cin, int Cout);
// forward (BWD = false) or dX (BWD = true); X / Cin are the gathered tensor, Y / Cout the produced one.  bn_part: where k_convbig8 may leave the
// per-channel sums of Y as chunk partials (*bn_chunks > 0 says it did)
template <bool BWD>
void launch_conv_big(int K, int S, int P, hipStream_t hs, const float *X, float *Y, float *Y2, const float *F, const float *B,
                     int N, int Hx, int Wx, int Cin, int Hy, int Wy, int Cout, int C0f, float *bn_part = nullptr, size_t bn_part_floats = 0, int *bn_chunks = nullptr);
// dF partial slabs [slice][C1*K*K][C0]; returns the number of slices written (0: workspace too small)
int launch_conv_big_df(int K, int S, int P, hipStream_t hs, const float *I, const float *DO, float *part, size_t part_floats,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0);

// ---- conv_img.hip: image-input layers (3x3, stride 1, padding 1).  Each returns true when the layer was launched there
bool conv_thin_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B, int N, int H, int W, int C1, int C0, hipStream_t hs,
                   float *bn_part = nullptr, size_t bn_part_floats = 0, int *bn_chunks = nullptr);
bool conv_thin_df(const float *I, const float *DO, float *part, size_t part_bytes, int N, int H, int W, int C1, int C0, int *nslice, hipStream_t hs);
bool conv_img_block_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B, const t4k_poolblock *blk,
                        int N, int H, int W, int C1, int C0, hipStream_t hs);

// ---- fused.hip: the validation of t4k_poolblock_fwd on its own (T4K_OK, or the status it would return, with the message set)
int poolblock_check(const t4k_poolblock *b, const char *who);

// ---- reduce.hip: batch-norm forward from the chunk partials a conv epilogue left
int bn_stats_for(const float *I, float *stat, int N, int HW, int C, const float *part, int nchunk, t4k_stream_t s);
int bn_fwd_from_parts(const float *I, float *O, float *XH, const float *W, const float *B, float *stat, long NHW, int C, const float *part, int nchunk, hipStream_t hs);
}

using namespace t4k;

namespace {

constexpr int LDS_FILTER_FLOATS = 8192;          // 32 KiB filter slice per workgroup

// The LAB switches of the convolution units, read once per unit (release builds: the defaults, no environment read).  Each is an ablation of one
// rung of the dispatch; the measured reason for its default is given here or at the condition that uses it.
struct ConvLab {
    // the entry points (conv.hip)
    int block      = T4K_LAB_ENV("T4K_CONV_BLOCK", 1);            // t4k_conv2d_block_fwd: the element-wise run in the conv epilogue
    int big        = T4K_LAB_ENV("T4K_CONV_BIG", 1);              // many channels on the LDS-staged kernels of conv_big.hip
    int few        = T4K_LAB_ENV("T4K_CONV_FEW", 1);              // few channels on the vector kernels of conv_few.hip
    int ksplit     = T4K_LAB_ENV("T4K_CONV_KSPLIT", 1);           // gather kernel: two waves per tile on small layers
    int bn_rider   = T4K_LAB_ENV("T4K_CONV_BN_RIDER", 1);         // 0: t4k_conv2d_bn_fwd / _bn_block_fwd are always the separate calls
    // enough slices that ~2000 waves are in flight (each wave then issues only a few batches of loads) without
    // inflating the partial slab the fold has to read: 512 workgroups in total across the (tap, c0) tiles
    int df_wg      = std::max(1, T4K_LAB_ENV("T4K_CONV_DF_WG", 512));
    // conv_few.hip
    int dx_wide    = T4K_LAB_ENV("T4K_DX_WIDE", 1);               // C0 / 4 lanes per pixel for the image-input dX with 32 / 64 / 128 output channels
    int dx_wide_wpc = T4K_LAB_ENV("T4K_DX_WIDE_WPC", 8);          // its workgroups per CU: the weights are loaded once per workgroup
    // conv_big.hip, forward / dX
    int big8       = T4K_LAB_ENV("T4K_CONVBIG8", 1);              // the 8-wave LDS-DMA kernel (k_convbig8)
    int big8_bk32  = T4K_LAB_ENV("T4K_CONVBIG8_BK32", 1);         // 32-channel stages, two workgroups per CU: 0 off, 1 from two tiles per CU, 2 always
    int big8_nt    = T4K_LAB_ENV("T4K_CONVBIG8_NT", 0);           // non-temporal output stores
    int wide_mul   = T4K_LAB_ENV("T4K_CONVBIG_WIDE_MUL", 1);      // k_convbig: 128-wide tiles from this many workgroups per CU
    // conv_big.hip, dF
    int df_wpc     = std::max(1, T4K_LAB_ENV("T4K_DF_WGS_PER_CU", 3));   // k_convbig_df: workgroups per CU in total
    int df_xcd     = T4K_LAB_ENV("T4K_DF_XCD", 1);                // slice counts in multiples of 8: a pixel slice stays on one XCD's L2
    // 0 off, 1 (default) 64-pixel stages and one workgroup per CU, 2 32-pixel stages and two per CU, 3 / 4: the same with two or four taps of
    // 64 / 32 channels per tile too - they lose: 9 taps fill 10 / 12 tap slots and the fold reads 51 slices (64 -> 128 @ 16x16: 96.3 + 24 us of fold against 89 + 12)
    int dfw        = T4K_LAB_ENV("T4K_CONVBIG_DFW", 1);
    int df8        = T4K_LAB_ENV("T4K_CONVBIG_DF8", 64);          // 0: the 4-wave register-staged kernel; 32 / 64 / 128: pixels per stage of the 8-wave LDS-DMA kernel
    int df8_wpc    = T4K_LAB_ENV("T4K_CONVBIG_DF8_WPC", 0);       // 0: as many workgroups per CU as the LDS holds, at most 3
    int df8_nst    = T4K_LAB_ENV("T4K_CONVBIG_DF8_NST", (df8 >= 64 ? 2 : 4));   // stage buffers
    int df8_tp2    = T4K_LAB_ENV("T4K_CONVBIG_DF8_TP2", 1);       // two taps per 64-row tile when C1 == 32
    int df8_dbg    = T4K_LAB_ENV("T4K_CONVBIG_DF8_DBG", 0);
    // conv_img.hip
    int thin       = T4K_LAB_ENV("T4K_CONV_THIN", 1);             // k_conv_thin_fwd
    int thin_wg    = std::max(1, T4K_LAB_ENV("T4K_CONV_THIN_WG", 512));      // a wave walks ntile / (4 wg) tiles with its filter in registers
    int thin_nt    = T4K_LAB_ENV("T4K_CONV_THIN_NT", 1);          // non-temporal output stores
    int thin_df    = T4K_LAB_ENV("T4K_CONV_THIN_DF", 1);          // k_conv_thin_df
    int thin_df_wg = std::max(1, T4K_LAB_ENV("T4K_CONV_THIN_DF_WG", 512));
    int img        = T4K_LAB_ENV("T4K_CONV_IMG", 1);              // k_conv_img_block
    int img_nt     = T4K_LAB_ENV("T4K_CONV_IMG_NT", 1);           // non-temporal stores of its full-size outputs
};
inline const ConvLab &conv_lab() { static const ConvLab v; return v; }

// ---- host-side planning shared by the units that cut dF into pixel slices
inline bool all16(const void *a, const void *b, const void *c = nullptr, const void *d = nullptr, const void *e = nullptr) {
    return aligned16(a) && aligned16(b) && aligned16(c) && aligned16(d) && aligned16(e);
}
// `want_slices` (at least one) over npix pixels: pixels per slice in whole stages, at least min_pixels, and the slices that then cover npix
struct DfSlices { long pps, n; };
inline DfSlices df_slices(long npix, long want_slices, int stage_pixels, int min_pixels) {
    if (want_slices < 1) want_slices = 1;
    long pps = (npix + want_slices - 1) / want_slices;
    pps = (pps + stage_pixels - 1) / stage_pixels * stage_pixels;
    if (pps < min_pixels) pps = min_pixels;
    return { pps, (npix + pps - 1) / pps };
}

// the run-time-geometry layers (conv_geo.hip, conv_group.hip): their dF | dB slabs live in the first half of a stream's workspace (colsum_add owns the
// second) - ONE slab may fill it, but the slice count shrinks until the slabs fit 8 MiB (conv.hip's ws / 8): what the fold reads back stays cache-sized
constexpr size_t CONV_WS_BYTES = (size_t)32 << 20, CONV_SLAB_AIM = (size_t)8 << 20;
constexpr int CONV_DF_WG = 1024;                        // workgroups their dF launch aims at
// slices: enough that ~CONV_DF_WG workgroups run (`tiles` per slice), whole 32-pixel stages each, no more than CONV_SLAB_AIM holds slabs of ntot floats;
// pps_cap: what the kernel's pixels-per-slice argument holds.  k_fold_add walks whole slabs into ONE destination: it serves up to 32 slices when DB lies
// right behind DF (a layer's gradient block); otherwise the wave-per-output fold splits the slab between the two (fold: 1 fold_add, 2 df_fold)
struct SlabPlan { long pps; int nslice, fold; };
inline SlabPlan slab_plan(long np0, long tiles, long ntot, bool db_adjacent, long pps_cap) {
    const long want = std::min((CONV_DF_WG + tiles - 1) / tiles, (long)(CONV_SLAB_AIM / sizeof(float)) / ntot);
    SlabPlan s;
    s.pps = std::min(df_slices(np0, want, 32, 0).pps, pps_cap);
    s.nslice = (int)((np0 + s.pps - 1) / s.pps);
    s.fold = (s.nslice <= 32 && db_adjacent) ? 1 : 2;
    return s;
}
// what both admit alike (who: the entry's name for the message; groups: the group count, null for the layer without groups).  T4K_ERR_ARG: an extent below 1;
// T4K_ERR_UNSUPPORTED: a geometry or a group count outside the admitted set, 2^31 pixels, a slab beyond the workspace.  Every product is formed in 64
// bits: the extents may be anything an int holds.  *H0, *W0: the output grid
inline int conv_geo_admit(const char *who, int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D, const int *groups, int *H0, int *W0) {
    if (N < 1 || H1 < 1 || W1 < 1 || C1 < 1 || C0 < 1) return fail(T4K_ERR_ARG, "%s: an extent below 1 (N=%d H1=%d W1=%d C1=%d C0=%d)", who, N, H1, W1, C1, C0);
    if (K < 1 || K > 7 || S < 1 || S > 4 || D < 1 || D > 4 || P < 0 || P > D * (K - 1))
        return fail(T4K_ERR_UNSUPPORTED, "%s: kernel_size=%d stride=%d padding=%d dilation=%d not supported (K 1..7, S 1..4, D 1..4, 0 <= P <= D(K-1))", who, K, S, P, D);
    const int G = groups ? *groups : 1;
    if (G < 1 || C1 % G != 0 || C0 % G != 0) return fail(T4K_ERR_UNSUPPORTED, "%s: groups=%d not supported (1 <= G, G divides C1=%d and C0=%d)", who, G, C1, C0);
    const long eh = (long)H1 + 2 * P - D * (K - 1) - 1, ew = (long)W1 + 2 * P - D * (K - 1) - 1;
    if (eh < 0 || ew < 0) return fail(T4K_ERR_UNSUPPORTED, "%s: the %dx%d window (dilation %d) does not fit the padded %ldx%ld image", who, K, K, D, (long)H1 + 2 * P, (long)W1 + 2 * P);
    const long h0 = eh / S + 1, w0 = ew / S + 1, lim = 1L << 31;
    if ((long)N * h0 >= lim || (long)N * h0 * w0 >= lim || (long)N * H1 >= lim || (long)N * H1 * W1 >= lim) return fail(T4K_ERR_UNSUPPORTED, "%s: 2^31 pixels or more", who);
    *H0 = (int)h0; *W0 = (int)w0;
    const long rows = (long)(C1 / G) * K * K + 1;       // (rows x C0 may pass 64 bits: divide)
    if (rows > (long)(CONV_WS_BYTES / sizeof(float)) / C0)
        return groups ? fail(T4K_ERR_UNSUPPORTED, "%s: one dF | dB slab (%ld x %d floats) does not fit the workspace", who, rows, C0)
                      : fail(T4K_ERR_UNSUPPORTED, "%s: one dF | dB slab (%ld floats) does not fit the workspace", who, (long)((unsigned long)rows * (unsigned long)C0));
    return T4K_OK;
}

}
