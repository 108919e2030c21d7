// gemm_types.h - what the GEMM translation units share (gemm.hip, linear.hip): the kernels' parameter blocks, the
// host functions that cross units, and with_layout (launch_lds / with_flags: launch.h).
// The kernels live in headers beside their host files (gemm_tile.h, gemm_l32.h, gemm_head_bwd.h) or in the one unit that launches them; every kernel template is
// instantiated in exactly one unit - the one that launches it.
#pragma once
#include "launch.h"
#include "colsum.h"
#include <stdlib.h>
#include <mutex>

namespace t4k {
// mask-multiply backward of the element-wise run in front of a linear layer, applied to dX where it is produced:
// d1 = dX * m1 (the run's last stage), d2 = d1 * m2 (the stage in front of it); absent stages are nullptr
struct MaskChain { const float *m1; float *d1; const float *m2; float *d2; };
// riders of a GEMM's last launch (its split-K fold, or the epilogue of the small-tile kernel): see k_splitk_fold
struct FoldRider { ActEpi ep2; const float *cp_src; float *cp_dst; long cp_n; int cp_blocks, cp_vec; MaskChain mc; int mc_done; };
// column sums of X [rows, E] added into out: the bias gradient of a linear layer, offered to the launch of its weight-gradient GEMM
struct ColSum { const float *X; float *out; int rows, E; bool done; };

// gemm.hip: the dispatch ladder behind t4k_gemm and the linear layers.  rider: in ep2 / cp_*, out cp_blocks > 0 when the copy went with the fold
int gemm_launch(const float *A, const float *B, float *O, const float *bias, float alpha, float beta,
                int tA, int tB, int M, int N, int K, int C, t4k_stream_t s, const ActEpi *epi = nullptr, bool *epi_done = nullptr,
                ColSum *cs = nullptr, XFold *defer = nullptr, FoldRider *rider = nullptr);
// linear_small.hip: classifier-head sized layers on the vector ALUs, one launch each way
bool linear_small_ok(int E0, int E1);
int  linear_small_fwd(const float *X, const float *W, const float *B, float *Y, float *P, int N, int E0, int E1, hipStream_t hs, const XFold *xf = nullptr,
                      const ActEpi *oep = nullptr);   // oep: element-wise layer behind the linear layer, applied in the same launch
bool linear_small_bwd(const float *X, const float *W, const float *DY, float *DX, float *DW, float *DB, int N, int E0, int E1, bool train, hipStream_t hs,
                      const float *MASK = nullptr, float *DXM = nullptr, const float *TGT = nullptr, float *DY2 = nullptr,
                      const float *MASKB = nullptr, float *DXMB = nullptr);
}

using namespace t4k;

namespace {
T4K_SPIN_DECL                                                  // per unit (no relocatable device code): gemm.hip and linear.hip hold kernels that wait and have a setter each

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));       // first-class 16-byte value (HIP's float4 is a struct: its
                                                               // copies become memcpy and can pin staging arrays in scratch)

// One unsplit product with alpha = 1, beta = 0 and no riders unless a fill site says otherwise
struct GemmP {
    const float *A = nullptr, *B = nullptr;
    const float *bias = nullptr;       // optional per-column bias fused in the epilogue (k_bias nmath.cu:27)
    float *O = nullptr, *part = nullptr;
    int M = 0, N = 0, K = 0, C = 1;
    int tiles_m = 0, tiles_n = 0;
    int kchunk = 0, nsplit = 1;
    float alpha = 1.0f, beta = 0.0f;
    int *sync = nullptr;               // [0,2048) tickets, [2048,4096) flags (self-cleaning)
    // optional rider (generic 64x64 kernel only): workgroups beyond the tile grid add the column sums of a [rows, E] matrix
    // into cs_out - the bias gradient of a linear layer shares the launch of its weight-gradient GEMM
    const float *cs_X = nullptr; float *cs_out = nullptr; int cs_rows = 0, cs_E = 0;
    int xmap = 0;                      // 32x32 kernels: 0 = tiles in launch order; 1 / 2 = XCD x (workgroup id % 8) owns a contiguous run of the row-major / column-major tile order
    const float *Z = nullptr;          // 4 KiB of zeros (State::d_zero): source of LDS-DMA lanes past the K range / the matrix edge (DMA variants of the 32x32 kernels)
};

// (tA, tB) -> the kernels' <AKC, BKC>: an operand's K axis is contiguous in memory when A is not transposed / when B is
template <typename F, typename... Bs>
void with_layout(int tA, int tB, F &&f, Bs... more) { with_flags(f, !tA, tB != 0, more...); }

// The LAB switches of the GEMM units, read once per unit (release builds: the defaults, no environment read).  Each is an ablation of one
// rung of the ladder; the measured reason for its default is given here or at the condition that uses it.
struct GemmLab {
    // gemm_launch (gemm.hip)
    int s32        = T4K_LAB_ENV("T4K_GEMM_S32", 1);              // slivers on 32x32 tiles (k_gemm_l32)
    int s32_maxk   = T4K_LAB_ENV("T4K_GEMM_S32_MAXK", 832);       // measured: 256 x 512 x K wins up to K = 784 (7.6 vs 10.6 us at 512), loses at 1024 (12.8 vs 10.7 us split-K + fold)
    int xmap       = T4K_LAB_ENV("T4K_GEMM_XMAP", 0);             // measured: no effect on the GAN layers (the Infinity Cache serves all eight L2s), off
    int plain_pair = T4K_LAB_ENV("T4K_GEMM_PLAIN_PAIR", 1);       // two workgroups per tile on the lean kernel (k_gemm_nn_plain<.., PAIR>)
    int split_div  = std::max(1, T4K_LAB_ENV("T4K_GEMM_SPLIT_DIV", 1));
    int ragged_dma = T4K_LAB_ENV("T4K_GEMM_RAGGED_DMA", 1);       // ragged M / N with whole K stages on the 8-wave LDS-DMA kernel
    int ragged_k   = T4K_LAB_ENV("T4K_GEMM_RAGGED_K", 1);         // 0 off, 1 unsplit products (default), 2 split-K slabs too
    int plain_big  = T4K_LAB_ENV("T4K_GEMM_PLAIN_BIG", 1);        // large plain products on the 64x64 LDS-DMA kernel
    int plain_ragk = T4K_LAB_ENV("T4K_GEMM_PLAIN_RAGK", 2);       // 0 off (the general kernel's tail), 1 only K % 64 != 0, 2 (default) every K % 128 != 0 (K = 960: 18.9 vs 19.6 us on the 64-deep general kernel)
    // 0 off, 1 (default) where it wins, 2 every eligible shape (tests).  A workgroup per CU at a time either way, so the choice is wave quantisation:
    // tiles / (rounds x CUs) of each tiling, the 128x128 pipeline being ~3.5 % faster per FLOP (2048^3: 136 -> 131 us)
    int plain128   = T4K_LAB_ENV("T4K_GEMM_PLAIN128", 1);
    int plain128_ragk = T4K_LAB_ENV("T4K_GEMM_PLAIN128_RAGK", 1); // 0: a partial last K stage keeps the product on 64x64 tiles
    // the lean kernel for every layout and epilogue: 0 off, 1 one-tile-per-CU shapes only (!= 0), 2 (default) large ones too (>= 2).  Unset, 0, 1 and 2 behave
    // as they did when the two uses read the variable separately with defaults 1 and 2: unset took both, and so does 2.
    int plain_any  = T4K_LAB_ENV("T4K_GEMM_PLAIN_ANY", 2);
    int big_dma    = T4K_LAB_ENV("T4K_GEMM_BIG_DMA", 1);          // the other large products on the 8-wave LDS-DMA kernel (needs gates_ok())
    int big_fullk  = T4K_LAB_ENV("T4K_GEMM_BIG_FULLK", 1);        // 128x128 tiles: whole K stages are enough for the predicate-free pipeline
    int fullk      = T4K_LAB_ENV("T4K_GEMM_FULLK", 0);            // measured on the GAN nets: the skewed kernel is 1 % faster for ragged split-K shapes, off
    // launchers of the lean kernels (gemm.hip)
    int fastpro    = T4K_LAB_ENV("T4K_GEMM_FASTPRO", 1);          // k_gemm_nn_plain<POW2>: shift / mask tile prologue on power-of-two grids
    int tt_swap    = T4K_LAB_ENV("T4K_GEMM_TT_SWAP", 0);          // tile order with the roles of M and N exchanged when both operands are transposed
    int plain256   = T4K_LAB_ENV("T4K_GEMM_PLAIN256", 1);         // the 16-wave 256x256 kernel: 0 off, 1 default, 2 any grid of whole 256-tiles
    int plain128_bk32 = T4K_LAB_ENV("T4K_GEMM_PLAIN128_BK32", 1); // 32-deep stages, two workgroups per CU: 0 / 1 / 2 (always)
    // the linear layers (linear.hip)
    int dual       = T4K_LAB_ENV("T4K_GEMM_DUAL", 1);             // dW || dX in one launch (needs gates_ok())
    int dual_maxk  = T4K_LAB_ENV("T4K_GEMM_DUAL_MAXK", 1024);     // deep-K shapes would go split-K + fold (2 launches per GEMM); up to K = 1024 the single dual launch, unsplit, is faster (GAN round 0.318 ms of GPU time; with 256: 0.341)
    int dual_full  = T4K_LAB_ENV("T4K_GEMM_DUAL_FULL", 1);        // 0: interior-tile shapes on the LDS-DMA kernels, 5 launches with their folds and the column sum: GAN round 0.356 instead of 0.318 ms of GPU time
    int dual32     = T4K_LAB_ENV("T4K_GEMM_DUAL32", 1);           // small layers on 32x32 tiles (k_gemm_dual_l32)
    int dual_fullk = T4K_LAB_ENV("T4K_GEMM_DUAL_FULLK", 1);       // k_gemm_dual<.., F1, F2>: the predicate-free pipeline for a half whose K is whole stages
    int head_fold  = T4K_LAB_ENV("T4K_HEAD_FOLD", 1);             // t4k_mlp_head_fwd: the head kernel folds the first layer's split-K slabs
    int head_bwd   = T4K_LAB_ENV("T4K_HEAD_BWD", 1);              // t4k_mlp_head_bwd: the one-launch head backward (k_head_bwd_l32)
};
inline const GemmLab &gemm_lab() { static const GemmLab v; return v; }

// The first inequalities of the ladder, shared by gemm_plan (gemm.hip) and the callers that decline what it would split (linear_bwd_dual, linear.hip)
inline long gemm_tiles64(int m, int n)  { return (long)((m + 63) / 64) * ((n + 63) / 64); }
inline long gemm_tiles128(int m, int n) { return (long)((m + 127) / 128) * ((n + 127) / 128); }
inline bool gemm_big(int m, int n, int cu) { return gemm_tiles128(m, n) >= (long)cu * 3 / 4; }        // 128x128 tiles for >= ~3/4 of the CUs
inline bool gemm_splits(long tiles, int k, int cu) { return tiles * 2 <= cu && k >= 256; }            // the output alone cannot fill the chip and K holds four 64-deep stages

// the LDS-DMA kernels address their operands with 32-bit lane offsets: both must span less than 4 GiB
inline bool span32(int M, int N, int K) { return (size_t)M * K * sizeof(float) < ((size_t)1 << 32) && (size_t)K * N * sizeof(float) < ((size_t)1 << 32); }
inline bool capturing(hipStream_t hs) { hipStreamCaptureStatus st_ = hipStreamCaptureStatusNone; return hipStreamIsCapturing(hs, &st_) == hipSuccess && st_ != hipStreamCaptureStatusNone; }   // a replayed graph would repeat the epoch argument
}
