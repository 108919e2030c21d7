// conv_stack_kernels.hip.inc - device source of the SAMPLE-RESIDENT convolution stacks, compiled AT RUN TIME by hipRTC for one
// model's shapes (csrc/conv_stack.hip holds the host side: preamble generation, compile cache, launch).
//
// Why run-time specialisation: the stack is a chain of short phases (stage a window in LDS, implicit-GEMM conv on MFMA, element-wise
// run, stores) that one workgroup walks for one band of one image.  Written for run-time shapes the phases drown in index arithmetic
// (integer divisions by run-time divisors, un-unrollable k loops whose LDS-read -> MFMA chains serialise, ~2 600 instructions per
// wave, 21 us for the LeNet front end); with every dimension a compile-time constant the divisions are multiplications, the k loops
// unroll with all their LDS reads issued in front of the MFMAs, dead layer branches vanish.  The host generates a preamble
//     #define CS_NS 2   #define CS_SPLIT 2   #define CS_SHAPES {H,W,C1,C0,K, pre,pool,post,KS, a_pre,a_post, flat}, {...}
// and prepends it to this text.  Arithmetic per element is that of k_conv2d (nmath.tcu:34-104), k_activate (nmath.cu:37-70),
// k_pool / k_dpool (nmath.tcu:122-186, 475-568); dropout draws the Philox slice t4k_dropout_mask would draw for its mask tensor.
#ifdef CS_SELFCHECK              // build-time syntax check (Makefile): the LeNet front end of bench.py
#define CS_NS 2
#define CS_SPLIT 2
#define CS_BSPLIT 2
#define CS_SHAPES {28, 28, 1, 10, 3, 0, 14, 4, 2, 0.f, 0.f, 0}, {14, 14, 10, 20, 3, 10, 14, 4, 2, 0.5f, 0.f, 1}
#define CS_HEAD 1
#define CS_H_EA 100
#define CS_H_EB 10
#define CS_H_MID 10
#define CS_H_ALPHA 0.5f
#define CS_H_PF 6
#ifndef CS_STREAM_DEAD          // (the Makefile compiles this check twice: -DCS_STREAM_DEAD=0 is the second)
#define CS_STREAM_DEAD 1
#endif
#endif

#ifndef CS_VALU_FWD
#define CS_VALU_FWD 1
#endif
#ifndef CS_SPLIT_FLOOR
#define CS_SPLIT_FLOOR 1
#endif

typedef unsigned int u32;
typedef unsigned long long u64;
typedef float v4f __attribute__((ext_vector_type(4)));

// layer codes of include/t4k.h (t4k_layer)
#define L_RELU 4
#define L_TANH 5
#define L_SIGMOID 6
#define L_SELU 7
#define L_LEAKYRL 8
#define L_ELU 9
#define L_DROPOUT 10
#define L_AVGPOOL 13
#define L_MAXPOOL 14
#define L_MINPOOL 15

#define CS_THREADS 512
#define CS_WAVES 8
// the banded backward (cs_bwd_b) runs 16 waves: in the middle phase of a stage waves 0 .. 7 take the dF items and waves 8 .. 15 the stage's dX, side by side
#define CS_BTHREADS 1024
#define CS_BWAVES 16
// lab hook (tools/experiments/cs_lab.hip, T4K_STACK_PROF_PTR): s_memtime stamps of wave 0 of every workgroup, 32 per workgroup
#define CS_STAMP_P(pp, k) do { if ((pp) && threadIdx.x == 0) (pp)[(blockIdx.x * gridDim.y + blockIdx.y) * 32 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#define CS_STAMP(k) do { if (p.prof && threadIdx.x == 0) p.prof[(blockIdx.x * gridDim.y + blockIdx.y) * 32 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
// the same from the first lane of wave 8: begin / end of the dX role of the banded backward (stamps 24 + 2 S, 25 + 2 S)
#define CS_STAMP_X(k) do { if (p.prof && threadIdx.x == CS_THREADS) p.prof[(blockIdx.x * gridDim.y + blockIdx.y) * 32 + (k)] = __builtin_amdgcn_s_memtime(); } while (0)

struct Shape { int H, W, C1, C0, K, pre, pool, post, KS; float a_pre, a_post; int flat; };
constexpr Shape SH[CS_NS] = { CS_SHAPES };

// ---- compile-time geometry
constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int cmin(int a, int b) { return a < b ? a : b; }
constexpr int H0(int s) { return SH[s].H / SH[s].KS; }
constexpr int W0(int s) { return SH[s].W / SH[s].KS; }
constexpr int jp_of(int kc) { return (kc + 3) & ~3; }
constexpr int JP(int s) { return jp_of(SH[s].K * SH[s].C1); }                  // k extent of one filter row (kx, c1), padded to the MFMA's 4
constexpr int NT(int s) { return (SH[s].C0 + 15) / 16; }
constexpr int NC(int s) { return NT(s) * 16 + (NT(s) > 1 ? 16 : 0); }         // B-operand row stride, 16 mod 32: a ds_read_b32 is served in two halves of 32 lanes = k rows (kq, kq+1) x 16
                                                                              // columns - the two rows must sit 16 banks apart (16 and 48 do; the 40 of round 3 overlapped on 8 banks)
constexpr int JPb(int s) { return jp_of(SH[s].K * SH[s].C0); }                 // dX conv: input = dO (C0 channels), output channels = C1
constexpr int NTb(int s) { return (SH[s].C1 + 15) / 16; }
constexpr int NCb(int s) { return NTb(s) * 16 + (NTb(s) > 1 ? 16 : 0); }
// bands: band b OWNS pooled rows [ceil(H0 b / split), ceil(H0 (b+1) / split)) of every stage (what it stores) and COMPUTES the rows
// the next stage's window needs (halo rows are recomputed, never exchanged)
struct Win { int po_lo, po_hi, pc_lo, pc_hi; };
constexpr int po_lo(int s, int b) { return CS_SPLIT_FLOOR ? (H0(s) * b) / CS_SPLIT : (H0(s) * b + CS_SPLIT - 1) / CS_SPLIT; }          // floor: the LAST band (the head's collector) takes an odd row count's extra row (conv_stack.hip)
constexpr int po_hi(int s, int b) { return CS_SPLIT_FLOOR ? (H0(s) * (b + 1)) / CS_SPLIT : (H0(s) * (b + 1) + CS_SPLIT - 1) / CS_SPLIT; }
constexpr int pc_lo(int s, int b) { return s == CS_NS - 1 ? po_lo(s, b) : cmax(pc_lo(s + 1 < CS_NS ? s + 1 : s, b) * SH[s + 1 < CS_NS ? s + 1 : s].KS - SH[s + 1 < CS_NS ? s + 1 : s].K / 2, 0); }
constexpr int pc_hi(int s, int b) { return s == CS_NS - 1 ? po_hi(s, b) : cmin(pc_hi(s + 1 < CS_NS ? s + 1 : s, b) * SH[s + 1 < CS_NS ? s + 1 : s].KS + SH[s + 1 < CS_NS ? s + 1 : s].K / 2, H0(s)); }
constexpr int nr_max(int s) { int m = 0; for (int b = 0; b < CS_SPLIT; b++) m = cmax(m, (pc_hi(s, b) - pc_lo(s, b)) * SH[s].KS); return m; }   // conv rows of the largest window
constexpr int win_rows(int s) { return nr_max(s) + SH[s].K - 1; }
constexpr int win_cols(int s) { return SH[s].W + SH[s].K - 1; }
constexpr int pad4(int n) { return (n + 3) & ~3; }
constexpr int own_rows_max(int s) { int m = 0; for (int b = 0; b < CS_SPLIT; b++) m = cmax(m, po_hi(s, b) - po_lo(s, b)); return m; }   // pooled rows the largest band owns
// LDS plan (floats), forward: per stage the zero-bordered input window and the B-operand filter + bias, then one conv-output buffer
#ifdef CS_HEAD
constexpr int head_keep(int s) { return s == CS_NS - 1 ? own_rows_max(s) * W0(s) * SH[s].C0 : 0; }     // the band's slice of the flattened image stays in the last stage's (dead) window for the head
#else
constexpr int head_keep(int) { return 0; }
#endif
constexpr int in_size(int s) { return pad4(cmax(win_rows(s) * win_cols(s) * SH[s].C1 + 16, head_keep(s))); }     // + slack: the padded-k reads (zero weights) run past the last pixel
constexpr int w_size(int s) { return pad4(SH[s].K * JP(s) * NC(s)); }
constexpr int in_off(int s) { int o = 0; for (int t = 0; t < s; t++) o += in_size(t) + w_size(t) + pad4(SH[t].C0); return o; }
constexpr int w_off(int s) { return in_off(s) + in_size(s); }
constexpr int b_off(int s) { return w_off(s) + w_size(s); }
constexpr int out_off() { return in_off(CS_NS - 1) + in_size(CS_NS - 1) + w_size(CS_NS - 1) + pad4(SH[CS_NS - 1].C0); }
constexpr int out_size() { int m = 0; for (int s = 0; s < CS_NS; s++) m = cmax(m, nr_max(s) * SH[s].W * cmax(SH[s].C0, SH[s].C1)); return pad4(m); }
constexpr int fwd_lds_floats() { return out_off() + out_size(); }

// ---- Philox4x32-10 (counter = element index / 4, key = seed): the same definition as csrc/t4k_common.h and the oracle
__device__ __forceinline__ void philox4x32_10(u64 ctr, u64 key, u32 out[4]) {
    u32 c0 = (u32)ctr, c1 = (u32)(ctr >> 32), c2 = 0, c3 = 0, k0 = (u32)key, k1 = (u32)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const u32 h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const u32 n0 = h1 ^ c1 ^ k0, n1 = l1, n2 = h0 ^ c3 ^ k1, n3 = l0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float u01(u32 x) { return __fmaf_rn((float)x, 2.3283064365386963e-10f, 1.1641532182693481e-10f); }   // (0,1]

// one activation element (k_activate nmath.cu:37-70): i = input, u = uniform draw (dropout only); o = output, f = derivative mask
template <int L> __device__ __forceinline__ void act1(float i, float u, float alpha, float &o, float &f) {
    if (L == L_RELU)         { if (i > 0.0f) { f = 1.0f; o = i; } else { f = 0.0f; o = 0.0f; } }
    else if (L == L_TANH)    { o = tanhf(i); f = 1.0f - o * o; }
    else if (L == L_SIGMOID) { o = 1.0f / (1.0f + expf(-i)); f = o * (1.0f - o); }
    else if (L == L_SELU)    { if (i > 0.0f) { f = (float)1.0507; o = i; } else { f = (float)(1.7581 * (double)__expf(i)); o = (float)((double)f - 1.7581); } }
    else if (L == L_LEAKYRL) { if (i > 0.0f) { f = 1.0f; o = i; } else { f = alpha; o = alpha * i; } }
    else if (L == L_ELU)     { if (i > 0.0f) { f = 1.0f; o = i; } else { f = alpha * __expf(i); o = f - alpha; } }
    else if (L == L_DROPOUT) { if (u > alpha) { f = 1.0f; o = i; } else { f = 0.0f; o = 0.0f; } }
    else                     { o = i; f = 1.0f; }
}

// workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding GLOBAL store (s_waitcnt vmcnt(0)
// in front of s_barrier); the tensors these kernels store are never read back by them, so only the LDS counter has to drain.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

#ifdef CS_LAB_NOSTORE
#define CS_LAST_STORES(S) ((S) != CS_NS - 1)
#else
#define CS_LAST_STORES(S) true
#endif
// ---- store policy of a global store site.  Under the BANDED plan (CS_BSPLIT > 1) most of what the two large kernels store is read by no launch of the step: the
// banded backward reads the forward's saves instead of the layer tensors, and the next forward overwrites every dX.  Left to plain stores those lines stay dirty
// in the L2s until the kernel ends and are written back at the boundary, in front of the next launch; a STREAMING store hands them to the memory side while the
// body still runs.  A policy changes no value, order or address - only the cache bits of the store instruction.
//   ST_PLAIN  global_store_*                the default; every LIVE site, every site of a one-band module, all of cs_bwd
//   ST_NT     global_store_* ... nt         __builtin_nontemporal_store: what cs_bwd_b's dead sites take
//   ST_WT     global_store_* ... sc0 sc1    write-through (the form of the group head's slice stores below): what cs_fwd's dead sites take
// LIVE = read by a later launch of the step; DEAD = everything else (the host, t4k_conv_stack_dx0 on demand and a whole-image backward behind a banded forward
// still read them correctly: the policy is a hint, not a scope).  Bytes per image: the LeNet front end at batch 128.
//   kernel     site                                   tensor                          B/image  class  reader
//   cs_fwd     image rows                             X0 (layer-0 copy of the batch)    3 136  dead
//   cs_fwd     image rows                             save_x[0]                         3 136  LIVE   cs_bwd_b (stage_bwd_b: X window of the dF rows)
//   cs_fwd     stage_fwd, conv-output copy            O                        31 360 + 15 680  dead   (the LAST tensor of a stack without flatten - O, P, Q or R
//   cs_fwd     run_fwd, pre                           P                                15 680  dead    of the last stage - is LIVE: the layer behind the stack)
//   cs_fwd     run_fwd, pre                           Fpre                             15 680  LIVE   cs_bwd_b (run_bwd: mask multiply)
//   cs_fwd     run_fwd, pool                          Q                         7 840 + 3 920  dead
//   cs_fwd     run_fwd, pool                          save_am                   1 960 +   980  LIVE   cs_bwd_b (run_bwd<S, true>: the pool's winning cell)
//   cs_fwd     run_fwd, post                          R                         7 840 + 3 920  dead
//   cs_fwd     run_fwd, post                          Fpost                     7 840 + 3 920  LIVE   cs_bwd_b (run_bwd: mask multiply)
//   cs_fwd     run_fwd, flatten                       R2                                3 920  LIVE   k_head_bwd_l32 (dW1 = dY1^T x), the layer behind the stack
//   cs_fwd     run_fwd, next conv's input             save_x[1]                         7 840  LIVE   cs_bwd_b (stage_bwd_b)
//   cs_fwd     head_fwd                               Y1 Fm Am Y2 P hot hit slots       2 121  LIVE   k_head_bwd_l32; the collector band (slots)
//   cs_bwd_b   run_bwd, flatten / post / pool / pre   R, Q, P, O (dX of each layer)    78 400  dead   (stage 0's O holds the dO t4k_conv_stack_dx0 reads ON DEMAND)
//   cs_bwd_b   stage_bwd_b, dX copy-out               X, DXS of stages >= 1    7 840 + 7 840  dead   (X is the R of the stage in front, counted there)
//   cs_bwd_b   stage_bwd_b, dX copy-out               X, DXS of stage 0         3 136 + 3 136  LIVE   the backward of the layer in front of the stack, when there is one
//   cs_bwd_b   df_fold                                partial rows (2 bands)           15 360  LIVE   k_opt_step / k_cs_fold
//   cs_bwd_b   kernel end                             f0_save                    (360 once)    LIVE   t4k_conv2d_bwd2 (t4k_conv_stack_dx0)
// CS_STREAM_DEAD (preamble, conv_stack.hip: written for CS_BSPLIT > 1 only, part of the cache key) turns the dead sites' policy on; CS_STREAM_FWD / CS_STREAM_BWD are
// the policy each kernel's dead sites then take - the defaults are what measured fastest (profiles/LAB_NOTES.md 19: write-through took 0.9 us off a cs_fwd launch where
// nt took 0.15, nt 0.75 us off cs_bwd_b where write-through ADDED 1.9), lab builds override them (T4K_STACK_STREAM_FWD / _BWD).
#define ST_PLAIN 0
#define ST_NT 1
#define ST_WT 2
#ifndef CS_STREAM_DEAD
#define CS_STREAM_DEAD 0
#endif
#ifndef CS_STREAM_FWD
#define CS_STREAM_FWD ST_WT
#endif
#ifndef CS_STREAM_BWD
#define CS_STREAM_BWD ST_NT
#endif
constexpr int ST_FWD = (CS_STREAM_DEAD && CS_BSPLIT > 1) ? CS_STREAM_FWD : ST_PLAIN;      // dead sites of cs_fwd
constexpr int ST_BWD = (CS_STREAM_DEAD && CS_BSPLIT > 1) ? CS_STREAM_BWD : ST_PLAIN;      // dead sites of cs_bwd_b
typedef float v2f __attribute__((ext_vector_type(2)));
// The write-through forms are inline asm: the compiler does not look inside the string, so each ends with the wait states (s_nop 1) that keep whatever instruction
// follows from overwriting the data registers before the store has read them, and each is a compiler memory barrier ("memory"), so no access of the
// compiler's own is moved across a store it cannot see.
template <int POL> __device__ __forceinline__ void gstore4(float *p, const float4 &t) {      // 16 bytes (the copy loops hand their LDS read over as it is)
    if constexpr (POL == ST_NT)      __builtin_nontemporal_store(v4f{t.x, t.y, t.z, t.w}, reinterpret_cast<v4f *>(p));
    else if constexpr (POL == ST_WT) { const v4f u = v4f{t.x, t.y, t.z, t.w}; asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(u) : "memory"); }
    else                             *reinterpret_cast<float4 *>(p) = t;
}
template <int POL> __device__ __forceinline__ void gstore2(float *p, const float2 &t) {
    if constexpr (POL == ST_NT)      __builtin_nontemporal_store(v2f{t.x, t.y}, reinterpret_cast<v2f *>(p));
    else if constexpr (POL == ST_WT) { const v2f u = v2f{t.x, t.y}; asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(u) : "memory"); }
    else                             *reinterpret_cast<float2 *>(p) = t;
}
template <int POL> __device__ __forceinline__ void gstore1(float *p, const float t) {
    if constexpr (POL == ST_NT)      __builtin_nontemporal_store(t, p);
    else if constexpr (POL == ST_WT) asm volatile("global_store_dword %0, %1, off sc0 sc1\n\ts_nop 1" :: "v"(p), "v"(t) : "memory");
    else                             *p = t;
}
template <int VW, int POL = ST_PLAIN> __device__ __forceinline__ void gstore(float *p, const float *v) {
    if constexpr (POL == ST_PLAIN) {
        if (VW == 4)      *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1 % VW], v[2 % VW], v[3 % VW]);
        else if (VW == 2) *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1 % VW]);
        else              *p = v[0];
    } else {
        if (VW == 4)      gstore4<POL>(p, make_float4(v[0], v[1 % VW], v[2 % VW], v[3 % VW]));
        else if (VW == 2) gstore2<POL>(p, make_float2(v[0], v[1 % VW]));
        else              gstore1<POL>(p, v[0]);
    }
}
// the policy of a forward store to run tensor `kind` (0 = O, 1 = P, 2 = Q, 3 = R) of stage S: the stack's LAST tensor, when no flatten copies it, is the input of
// the layer behind the stack and stays plain
constexpr int last_kind(int s) { return SH[s].post ? 3 : (SH[s].pool ? 2 : (SH[s].pre ? 1 : 0)); }
constexpr int st_fwd_of(int s, int kind) { return (s == CS_NS - 1 && !SH[s].flat && kind == last_kind(s)) ? ST_PLAIN : ST_FWD; }
constexpr int vw_of(int n) { return (n & 3) == 0 ? 4 : ((n & 1) == 0 ? 2 : 1); }
template <int CV> struct VecF { float v[CV]; };
template <int CV> __device__ __forceinline__ VecF<CV> gload(const float *p) {
    VecF<CV> r;
    if (CV == 4)      { const float4 t = *reinterpret_cast<const float4 *>(p); r.v[0] = t.x; r.v[1 % CV] = t.y; r.v[2 % CV] = t.z; r.v[3 % CV] = t.w; }
    else if (CV == 2) { const float2 t = *reinterpret_cast<const float2 *>(p); r.v[0] = t.x; r.v[1 % CV] = t.y; }
    else              r.v[0] = *p;
    return r;
}
// the same on LDS addresses that are CV-float aligned (the LDS base is 16-byte aligned, every region offset a multiple of 4 floats)
template <int CV> __device__ __forceinline__ VecF<CV> lload(const float *p) { return gload<CV>(p); }
template <int CV> __device__ __forceinline__ void lstore(float *p, const float *v) { gstore<CV>(p, v); }

// ---- implicit-GEMM convolution out of LDS on v_mfma_f32_16x16x4_f32.  In: zero-bordered window [nr+K-1][W+K-1][CIN]; Wl: B operand
// [K][JPK][NCK] (zero padded); Out[p*COUT + c] = bias[c] + sum over the window's nr*W pixels.  A lane (i = l%16, kq = l/16) holds
// A[i][kq], B[kq][i]; D[4*kq + r][i].  A wave owns an M tile (16 pixels) with ALL its N tiles, and every loop below has constant
// bounds: the K * JPK/4 * (1 + NTK) LDS reads of a tile are all issued in front of its MFMAs.
// MTMAX = the most M tiles any caller's window has.  With one N tile a tile is a single chain of dependent MFMAs: a wave then takes two
// tiles at once when there are more tiles than waves, and otherwise splits the tile's k steps between two accumulators (added at the end) -
// two tiles per wave would leave half the waves idle (the 20 -> 10 dX of the LeNet backward: 7 tiles, 4 busy waves, 5.6 k cycles).
constexpr int conv_mt(int rows, int w) { return (rows * w + 15) / 16; }
// WV0 / WVN: the waves that share the tiles (the dX role of the banded backward: waves 8 .. 15 of 16); only those waves may call.
// PIPE = false (banded backward, whose 1024-thread workgroup may use 128 registers): no double buffer over the filter rows - a row's operands are read in
// chunks of at most 64 registers, each chunk in front of its MFMAs.  The MFMAs and their order are the same: same sums.
constexpr int conv_tpw(int ntk, int mtmax, int wvn) { return (ntk == 1 && mtmax > wvn) ? 2 : 1; }
constexpr bool conv_pipe_fits(int jpk, int ntk, int mtmax, int wvn) { return 2 * (jpk / 4) * (conv_tpw(ntk, mtmax, wvn) + ntk) <= 96; }
template <int W, int CIN, int COUT, int K, int JPK, int NTK, int NCK, int MTMAX = 1 << 20, int RSIN = 0, int WV0 = 0, int WVN = CS_WAVES, bool PIPE = true>
__device__ __forceinline__ void conv_mfma(const float *In, const float *Wl, const float *bias, float *Out, int nr) {
    const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) - WV0, i = lane & 15, kq = lane >> 4;
    constexpr int RS = RSIN ? RSIN : (W + K - 1) * CIN, STEPS = JPK / 4;     // RSIN: the window's row stride when it is padded (backward windows)
    constexpr int TPW = conv_tpw(NTK, MTMAX, WVN);                  // M tiles a wave works on at once
    constexpr int QC = (NTK == 1 && TPW == 1) ? 2 : 1;              // accumulators per tile (k steps alternate between them)
    // ROWT (backward windows of rows shorter than a tile, LeNet's 14-wide dX conv): a tile is ONE window row, lanes W .. 15 read on into the row's right
    // border and are not stored.  16 consecutive pixels of a row sit CIN floats apart - with CIN = 20 the lanes (i, kq) cover the 64 banks exactly once -
    // but a tile that wraps into the next row (every one of the 13 tiles of a 14 x 14 grid) breaks the progression at the wrap: 2-way conflicts on every A
    // read (VERDICT r5: 37 % of cs_bwd_b's LDS cycles).  14 row tiles take the waves the same number of rounds as 13 wrapped ones; same sums, same order.
    constexpr bool ROWT = W < 16 && W + K - 1 >= 16;            // (forward windows too: their pixel pitch of 10 floats is conflict-free as long as a tile does not wrap)
    const int M = nr * W, MT = ROWT ? nr : (M + 15) >> 4;
    float bb[NTK];
#pragma unroll
    for (int n = 0; n < NTK; n++) bb[n] = (bias && n * 16 + i < COUT) ? bias[n * 16 + i] : 0.f;
    for (int mt0 = wave * TPW; mt0 < MT; mt0 += WVN * TPW) {
        const float *a0[TPW];
#pragma unroll
        for (int t = 0; t < TPW; t++) {
            if (ROWT) a0[t] = In + min(mt0 + t, nr - 1) * RS + i * CIN + kq;
            else {
                const int p = min((mt0 + t) * 16 + i, M - 1), py = p / W, px = p - py * W;
                a0[t] = In + py * RS + px * CIN + kq;
            }
        }
        const float *b0 = Wl + kq * NCK + i;
        v4f acc[TPW][NTK], acc2[NTK];
#pragma unroll
        for (int t = 0; t < TPW; t++)
#pragma unroll
            for (int n = 0; n < NTK; n++) acc[t][n] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int n = 0; n < NTK; n++) acc2[n] = v4f{0.f, 0.f, 0.f, 0.f};
        // Software pipeline over the filter rows, pinned with scheduling barriers: the LDS reads of row ky+1 are ISSUED in front of the MFMAs of
        // row ky (left alone, hipcc sinks every read next to its MFMA to save registers and waits lgkmcnt(0) in front of each pair - one exposed
        // LDS round trip per two MFMAs, 24 per tile of the 10 -> 20 layer).  Reads return in order, so the waits become counted.
        if constexpr (!PIPE) {
            constexpr int QCH = cmax(1, cmin(STEPS, 64 / (TPW + NTK))), NCH = (STEPS + QCH - 1) / QCH;
#pragma unroll
            for (int ky = 0; ky < K; ky++)
#pragma unroll
                for (int ch = 0; ch < NCH; ch++) {
                    float av[TPW][QCH], bv[QCH][NTK];
#pragma unroll
                    for (int qq = 0; qq < QCH; qq++) {
                        const int q = ch * QCH + qq;
                        if (q < STEPS) {
#pragma unroll
                            for (int t = 0; t < TPW; t++) av[t][qq] = a0[t][ky * RS + q * 4];
#pragma unroll
                            for (int n = 0; n < NTK; n++) bv[qq][n] = b0[(ky * JPK + q * 4) * NCK + n * 16];
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int qq = 0; qq < QCH; qq++) {
                        const int q = ch * QCH + qq;
                        if (q < STEPS) {
#pragma unroll
                            for (int t = 0; t < TPW; t++)
#pragma unroll
                                for (int n = 0; n < NTK; n++) {
                                    if (QC == 2 && ((ky * STEPS + q) & 1)) acc2[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][qq], bv[qq][n], acc2[n], 0, 0, 0);
                                    else acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][qq], bv[qq][n], acc[t][n], 0, 0, 0);
                                }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        } else {
        float av[2][TPW][STEPS], bv[2][STEPS][NTK];
        auto load_row = [&](int buf, int ky) {
#pragma unroll
            for (int q = 0; q < STEPS; q++) {
#pragma unroll
                for (int t = 0; t < TPW; t++) av[buf][t][q] = a0[t][ky * RS + q * 4];
#pragma unroll
                for (int n = 0; n < NTK; n++) bv[buf][q][n] = b0[(ky * JPK + q * 4) * NCK + n * 16];
            }
        };
        load_row(0, 0);
#pragma unroll
        for (int ky = 0; ky < K; ky++) {
            if (ky + 1 < K) load_row((ky + 1) & 1, ky + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < STEPS; q++)
#pragma unroll
                for (int t = 0; t < TPW; t++)
#pragma unroll
                    for (int n = 0; n < NTK; n++) {
                        if (QC == 2 && ((ky * STEPS + q) & 1)) acc2[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ky & 1][t][q], bv[ky & 1][q][n], acc2[n], 0, 0, 0);
                        else acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ky & 1][t][q], bv[ky & 1][q][n], acc[t][n], 0, 0, 0);
                    }
            __builtin_amdgcn_sched_barrier(0);
        }
        }
        if (QC == 2) {
#pragma unroll
            for (int n = 0; n < NTK; n++) acc[0][n] += acc2[n];
        }
#pragma unroll
        for (int t = 0; t < TPW; t++)
#pragma unroll
            for (int n = 0; n < NTK; n++) {
                const int c = n * 16 + i;
                if (c < COUT && mt0 + t < MT) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (ROWT) { const int px = 4 * kq + r; if (px < W) Out[((mt0 + t) * W + px) * COUT + c] = acc[t][n][r] + bb[n]; }
                        else { const int pr = (mt0 + t) * 16 + 4 * kq + r; if (pr < M) Out[pr * COUT + c] = acc[t][n][r] + bb[n]; }
                    }
                }
            }
    }
}

// ======================================================================================================== forward
struct FwdStage {
    const float *F, *B; float *O;                    // filter T4(C1,K,K,C0), bias, conv output [N,H,W,C0]
    float *P, *Fpre, *Q, *Fpost, *R, *R2;            // run tensors (t4k_poolblock): pre out / mask, pool out, post mask / out, flatten copy
    u64 base, base2, seed;                           // Philox slices of a dropout pre / post stage (counter units)
    // what the BANDED backward reads instead of the layer tensors (which a neighbouring band overwrites in place): a copy of this
    // conv's input, and per pooled element the window cell (0..3) that won a max / min pool.  NULL: not saved.
    float *save_x; unsigned char *save_am;
};
#ifndef CS_XSCOPE
#define CS_XSCOPE __HIP_MEMORY_SCOPE_AGENT
#endif
#ifdef CS_HEAD
// the classifier head behind the stack's flatten (CS_HEAD builds only): linear E1 -> CS_H_EA, one element-wise layer CS_H_MID (dropout / activation / 0),
// linear CS_H_EA -> CS_H_EB, softmax.  `slots` [N][CS_SPLIT - 1][CS_H_EA] carry the other bands' partial sums tagged with this launch's `epoch`.
struct HeadArgs { const float *W1, *B1; float *Y1, *Fm, *Am; u64 base, seed; const float *W2, *B2; float *Y2, *P; u64 *slots; int *spin_err; u32 epoch; u32 n_label; const u32 *label; float *hot; unsigned char *hit_flag;
                  float *xs; u32 *xflag; };      // CS_H_GRP: the flattened images [N][E1] and their per-band ready flags (tagged with the launch's epoch)
struct FwdArgs { const float *X; float *X0; u64 *prof; int N; HeadArgs hd; FwdStage st[CS_NS]; };
#else
struct FwdArgs { const float *X; float *X0; u64 *prof; int N; FwdStage st[CS_NS]; };
#endif

// the element-wise run behind conv stage S for the window whose conv output sits in LDS (Out[nr][W][C0]); see conv_stack.hip
template <int S>
__device__ __forceinline__ void run_fwd(const FwdStage &g, float *gnext_save, float *Out, float *L, int img, int band) {
    constexpr int H = SH[S].H, W = SH[S].W, C = SH[S].C0, KS = SH[S].KS, PRE = SH[S].pre, POOL = SH[S].pool, POST = SH[S].post;
    constexpr int rowC = W * C, row0C = W0(S) * C;
    const int wpl = pc_lo(S, band), wph = pc_hi(S, band), wol = po_lo(S, band), woh = po_hi(S, band);
    const int cl = wpl * KS, nr = (wph - wpl) * KS, ol = wol * KS, oh = woh * KS;
    if (PRE) {                                        // pre: activation | dropout over the window's conv outputs, result back into Out
        lds_barrier();                                // ... which the conv-output copy (caller) must have read first
        constexpr int VW = vw_of(rowC);
        const long abs0 = ((long)img * H + cl) * rowC;
        const int n = nr * rowC, o_lo = (ol - cl) * rowC, o_hi = (oh - cl) * rowC;
        for (int l = threadIdx.x * VW; l < n; l += CS_THREADS * VW) {
            const long a = abs0 + l;
            float o[VW], f[VW];
            const VecF<VW> ev_ = lload<VW>(Out + l);             // one ds_read_b128 / b64 instead of VW scalar reads at a lane stride of VW floats (4-way bank conflicts)
            const float *e = ev_.v;
            u32 r[4] = {0, 0, 0, 0};
            if (PRE == L_DROPOUT) philox4x32_10(g.base + (u64)(a >> 2), g.seed, r);
#pragma unroll
            for (int q = 0; q < VW; q++) act1<PRE>(e[q], PRE == L_DROPOUT ? u01(r[(a + q) & 3]) : 0.f, SH[S].a_pre, o[q], f[q]);
            if (CS_LAST_STORES(S) && l >= o_lo && l < o_hi) { gstore<VW>(g.Fpre + a, f); gstore<VW, st_fwd_of(S, 1)>(g.P + a, o); }
            lstore<VW>(Out + l, o);
        }
        lds_barrier();
    }
    constexpr bool HAS_NEXT = S + 1 < CS_NS;
    if (POOL || POST || SH[S].flat || HAS_NEXT) {     // pool + post + flatten over the window's pooled rows; the result feeds the next stage's window
        constexpr int VW = vw_of(row0C);
        constexpr int SN = HAS_NEXT ? S + 1 : S, Kn = SH[SN].K, Pn = Kn / 2, RSN = (W0(S) + Kn - 1) * C;
        const long abs0 = ((long)img * H0(S) + wpl) * row0C;
        const int n = (wph - wpl) * row0C, o_lo = (wol - wpl) * row0C, o_hi = (woh - wpl) * row0C;
        float *next = L + in_off(SN);
        const int next_row0 = wpl - pc_lo(SN, band) * SH[SN].KS + Pn + Pn;    // window row of pooled row wpl: (wpl - (cl' - Pn)), + Pn border
        for (int lo = threadIdx.x * VW; lo < n; lo += CS_THREADS * VW) {
            float acc[VW]; int nx[VW]; int am[VW] = {};
#pragma unroll
            for (int q = 0; q < VW; q++) {
                const int l1 = lo + q, ir = l1 / row0C, r1 = l1 - ir * row0C, j0 = r1 / C, c = r1 - j0 * C;
                const int l = (ir * KS * W + j0 * KS) * C + c;
                float v = Out[l];
                if (POOL) {
                    const float e0 = v, e1 = Out[l + C], e2 = Out[l + W * C], e3 = Out[l + W * C + C];
                    if (POOL == L_MAXPOOL)      v = fmaxf(e3, fmaxf(e2, fmaxf(e1, v)));
                    else if (POOL == L_MINPOOL) v = fminf(e3, fminf(e2, fminf(e1, v)));
                    else                        v = (((v + e1) + e2) + e3) / 4.0f;
                    if (POOL != L_AVGPOOL) {                     // the cell k_dpool would pick: first extreme wins (strict comparison, nmath.tcu:531-545)
                        float best = e0; int a = 0;
                        if (POOL == L_MAXPOOL ? e1 > best : e1 < best) { best = e1; a = 1; }
                        if (POOL == L_MAXPOOL ? e2 > best : e2 < best) { best = e2; a = 2; }
                        if (POOL == L_MAXPOOL ? e3 > best : e3 < best) { best = e3; a = 3; }
                        am[q] = a;
                    }
                }
                acc[q] = v;
                nx[q] = (ir + next_row0 - Pn) * RSN + (j0 + Pn) * C + c;
            }
            const long zo = abs0 + lo;
            const bool own = lo >= o_lo && lo < o_hi;
            const bool ownst = own && CS_LAST_STORES(S);
            if (POOL && ownst) gstore<VW, st_fwd_of(S, 2)>(g.Q + zo, acc);
            if (POOL && POOL != L_AVGPOOL && ownst && g.save_am) {
                if (VW == 4) *reinterpret_cast<u32 *>(g.save_am + zo) = (u32)am[0] | ((u32)am[1 % VW] << 8) | ((u32)am[2 % VW] << 16) | ((u32)am[3 % VW] << 24);
                else {
#pragma unroll
                    for (int q = 0; q < VW; q++) g.save_am[zo + q] = (unsigned char)am[q];
                }
            }
            if (POST) {
                float o[VW], f[VW];
                u32 r[4] = {0, 0, 0, 0};
                if (POST == L_DROPOUT) philox4x32_10(g.base2 + (u64)(zo >> 2), g.seed, r);
#pragma unroll
                for (int q = 0; q < VW; q++) act1<POST>(acc[q], POST == L_DROPOUT ? u01(r[(zo + q) & 3]) : 0.f, SH[S].a_post, o[q], f[q]);
                if (ownst) { gstore<VW>(g.Fpost + zo, f); gstore<VW, st_fwd_of(S, 3)>(g.R + zo, o); }
#pragma unroll
                for (int q = 0; q < VW; q++) acc[q] = o[q];
            }
            if (SH[S].flat && ownst) gstore<VW>(g.R2 + zo, acc);
#ifdef CS_HEAD
            if (S == CS_NS - 1 && own) {                          // the head's input vector (this band's slice of the flattened image) stays in LDS: the dead conv-input window
#pragma unroll
                for (int q = 0; q < VW; q++) L[in_off(S) + (lo - o_lo) + q] = acc[q];
            }
#endif
            if (HAS_NEXT && own && gnext_save) gstore<VW>(gnext_save + zo, acc);      // the next conv's input, for its dF in the banded backward
            if (HAS_NEXT) {
#pragma unroll
                for (int q = 0; q < VW; q++) next[nx[q]] = acc[q];
            }
        }
    }
}

// Forward conv of a layer with FEW input channels (C1 <= 4: the image layer) on the vector ALUs: as an MFMA tile its K = 9 C1 taps fill 1/16
// (C1 = 1) of the k slots and the operand reads cost what a full tile's do (2.65 k cycles for 0.7 MFLOP on the LeNet input).  A lane owns a
// pixel with all its C0 <= 16 outputs; the window reads are its own 9 C1 floats, the weights 16-byte LDS broadcasts out of the B-operand
// image the filter already has (Wl[(ky JP + kx C1 + c1) NC + c0]).  The arithmetic is the reference kernel's, step for step (nmath.tcu:34-104
// as restated by the oracle: per input channel sum = bias | 0, then `sum += F * v` in (ky, kx) order, unfused, O += sum) - bit-identical to the
// oracle, so no relu / arg-max tie of this layer can fall the other way.
template <int S>
__device__ __forceinline__ void conv_valu_fwd(const float *Xw, const float *Wl, const float *Bl, float *Out, int nrows) {
    constexpr int W = SH[S].W, C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K, RSX = (W + K - 1) * C1, JP_ = JP(S), NC_ = NC(S), CQ = (C0 + 3) / 4;
    for (int pix = threadIdx.x; pix < nrows * W; pix += CS_THREADS) {
        const int y = pix / W, x = pix - y * W;
        float o[CQ * 4];
#pragma unroll
        for (int c1 = 0; c1 < C1; c1++) {
            float sm[CQ * 4];
#pragma unroll
            for (int q = 0; q < CQ; q++) {
                const float4 b = c1 == 0 ? *reinterpret_cast<const float4 *>(Bl + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
                sm[4 * q] = b.x; sm[4 * q + 1] = b.y; sm[4 * q + 2] = b.z; sm[4 * q + 3] = b.w;
            }
#pragma unroll
            for (int ky = 0; ky < K; ky++)
#pragma unroll
                for (int kx = 0; kx < K; kx++) {
                    const float v = Xw[(y + ky) * RSX + (x + kx) * C1 + c1];
                    const float *wr = Wl + (ky * JP_ + kx * C1 + c1) * NC_;
#pragma unroll
                    for (int q = 0; q < CQ; q++) {
                        const float4 w = *reinterpret_cast<const float4 *>(wr + 4 * q);
                        sm[4 * q]     = __fadd_rn(sm[4 * q],     __fmul_rn(w.x, v)); sm[4 * q + 1] = __fadd_rn(sm[4 * q + 1], __fmul_rn(w.y, v));
                        sm[4 * q + 2] = __fadd_rn(sm[4 * q + 2], __fmul_rn(w.z, v)); sm[4 * q + 3] = __fadd_rn(sm[4 * q + 3], __fmul_rn(w.w, v));
                    }
                }
#pragma unroll
            for (int c = 0; c < CQ * 4; c++) o[c] = c1 == 0 ? sm[c] : __fadd_rn(o[c], sm[c]);
        }
        float *dst = Out + pix * C0;
        if ((C0 & 1) == 0) {
#pragma unroll
            for (int c = 0; c < C0; c += 2) *reinterpret_cast<float2 *>(dst + c) = make_float2(o[c], o[c + 1]);
        } else {
#pragma unroll
            for (int c = 0; c < C0; c++) dst[c] = o[c];
        }
    }
}

template <int S>
__device__ __forceinline__ void stage_fwd(const FwdArgs &p, float *L, int img, int band) {
    if constexpr (S < CS_NS) {
        const FwdStage &g = p.st[S];
        constexpr int H = SH[S].H, W = SH[S].W, C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K, KS = SH[S].KS, rowC = W * C0;
        float *Out = L + out_off();
        const int wpl = pc_lo(S, band), wph = pc_hi(S, band), cl = wpl * KS, nr = (wph - wpl) * KS;
        CS_STAMP(3 + 4 * S);
        if constexpr (C1 <= 4 && C0 <= 16 && CS_VALU_FWD) conv_valu_fwd<S>(L + in_off(S), L + w_off(S), L + b_off(S), Out, nr);
        else conv_mfma<W, C1, C0, K, JP(S), NT(S), NC(S), conv_mt(nr_max(S), W)>(L + in_off(S), L + w_off(S), L + b_off(S), Out, nr);
        CS_STAMP(4 + 4 * S);
        lds_barrier();
        CS_STAMP(5 + 4 * S);
        const int ol = po_lo(S, band) * KS, oh = po_hi(S, band) * KS;         // owned conv rows: the conv output tensor
        {
            const int n = CS_LAST_STORES(S) ? (oh - ol) * rowC : 0;
            const float *src = Out + (ol - cl) * rowC;
            float *o = g.O + ((long)img * H + ol) * rowC;
            constexpr int POL = st_fwd_of(S, 0);
            if ((rowC & 3) == 0) { for (int e = threadIdx.x * 4; e < n; e += CS_THREADS * 4) gstore4<POL>(o + e, *reinterpret_cast<const float4 *>(src + e)); }
            else for (int e = threadIdx.x; e < n; e += CS_THREADS) gstore1<POL>(o + e, src[e]);
        }
        run_fwd<S>(g, S + 1 < CS_NS ? p.st[S + 1 < CS_NS ? S + 1 : S].save_x : nullptr, Out, L, img, band);
        CS_STAMP(6 + 4 * S);
        lds_barrier();
        stage_fwd<S + 1>(p, L, img, band);
    }
}

// filter element e of T4(C1,K,K,C0) -> its place in the forward conv's B operand: Wl[(ky*JP + kx*C1 + c1) * NC + c0]
template <int S> __device__ __forceinline__ int wl_fwd(int e) {
    constexpr int C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K;
    const int c0 = e % C0, t = e / C0, kx = t % K, t2 = t / K, ky = t2 % K, c1 = t2 / K;
    return (ky * JP(S) + kx * C1 + c1) * NC(S) + c0;
}
template <int S> __device__ __forceinline__ void load_filter(const FwdArgs &p, float (&vf)[CS_NS][8], float (&vb)[CS_NS]) {
    if constexpr (S < CS_NS) {
        constexpr int nF = SH[S].C1 * SH[S].K * SH[S].K * SH[S].C0;
        static_assert(nF <= 8 * CS_THREADS, "filter too large for the register-staged path");
#pragma unroll
        for (int q = 0; q < (nF + CS_THREADS - 1) / CS_THREADS; q++) { const int e = threadIdx.x + q * CS_THREADS; vf[S][q] = e < nF ? p.st[S].F[e] : 0.f; }
        vb[S] = threadIdx.x < SH[S].C0 ? p.st[S].B[threadIdx.x] : 0.f;
        load_filter<S + 1>(p, vf, vb);
    }
}
template <int S> __device__ __forceinline__ void put_filter(float *L, const float (&vf)[CS_NS][8], const float (&vb)[CS_NS]) {
    if constexpr (S < CS_NS) {
        constexpr int nF = SH[S].C1 * SH[S].K * SH[S].K * SH[S].C0;
#pragma unroll
        for (int q = 0; q < (nF + CS_THREADS - 1) / CS_THREADS; q++) { const int e = threadIdx.x + q * CS_THREADS; if (e < nF) L[w_off(S) + wl_fwd<S>(e)] = vf[S][q]; }
        if (threadIdx.x < SH[S].C0) L[b_off(S) + threadIdx.x] = vb[S];
        put_filter<S + 1>(L, vf, vb);
    }
}

#ifdef CS_HEAD
// ---- the classifier head, per image, in the same launch (the forward then is ONE launch instead of stack + split-K GEMM + fold/head kernel).
// Every band multiplies ITS slice of the flattened image into the first linear layer: y1[e] = sum_k x[k] W1[e, k] over the band's k range
// (a wave per output row, lanes along k: coalesced reads of W1's rows).  Bands 0 .. SPLIT-2 PUBLISH their CS_H_EA partial sums - one 64-bit
// agent-scope store per element, {this launch's epoch, value}, so a reader can tell a fresh word from last launch's without any counter or
// clean-up - and are done.  The LAST band collects them (polls each word until its tag is the epoch: one fabric round trip when the
// publisher was ahead), adds them in band order = ascending k (deterministic), then bias, the element-wise layer (same Philox positions as
// t4k_mlp_head_fwd), the second linear layer and the softmax, and stores every layer tensor.  Liveness: workgroups are dispatched in
// blockIdx order, bands of lower index first, and a publisher never waits - so the collector's partners are always running or done;
// the wait is bounded all the same (error word as in csrc/t4k_common.h).
constexpr bool head_v4_ok() {
    constexpr int S = CS_NS - 1, row0C = W0(S) * SH[S].C0;
    if ((H0(S) * row0C) & 3) return false;                       // row pitch of W1
    for (int b = 0; b < CS_SPLIT; b++) if (((po_lo(S, b) * row0C) & 3) || (((po_hi(S, b) - po_lo(S, b)) * row0C) & 3)) return false;
    return true;
}
// A wave's share of W1's rows: slots 0 .. nrw-1 <-> rows w0 + (slot + rot) % nrw.  Every workgroup walks the same rows of W1; started in
// the same order they would all ask the same L2 channel for the same line at the same time, so each workgroup starts at its own row (`rot`;
// the rows are independent sums: the order changes nothing in the result).
struct HeadRows { int w0, nrw, rot; __device__ __forceinline__ int row(int slot) const { int t = slot + rot; if (t >= nrw) t -= nrw; return w0 + t; } };
__device__ __forceinline__ HeadRows head_rows(int img, int band) {
    constexpr int RPW = (CS_H_EA + CS_WAVES - 1) / CS_WAVES;
    const int wave = threadIdx.x >> 6;
    HeadRows r; r.w0 = wave * RPW; r.nrw = max(min(CS_H_EA, r.w0 + RPW) - r.w0, 0); r.rot = r.nrw > 0 ? (img * 5 + band * 3) % r.nrw : 0;
    return r;
}
constexpr int head_nk_max() { return own_rows_max(CS_NS - 1) * W0(CS_NS - 1) * SH[CS_NS - 1].C0; }
constexpr int head_pf_row() { return pad4(head_nk_max()); }            // floats per prefetched row slice in LDS
constexpr int head_pf_off() { return fwd_lds_floats(); }               // behind everything the stack uses
#ifndef CS_H_PF
#define CS_H_PF 0
#endif
// GROUP HEAD (CS_H_GRP, VERDICT r4 #3): the first linear layer of 8 images at once.  A per-sample workgroup has no reuse of W1 across images: every one
// of the N x SPLIT workgroups streamed its band's slice of ALL of W1 through its CU's miss path (196 KB each, 50 MB through the L2s per step: 5.4 of
// the forward's 18 us).  Here the 8 workgroups of a GROUP - images img0 + r + 8 j (j = 0..7) of one band, which the dispatcher places on ONE XCD (workgroup
// id mod 8), behind one L2 - share the work the other way round: member j keeps rows [j RPG, (j + 1) RPG) of W1's band slice in LDS (prefetched by the
// LDS-DMA engine under the convolutions: 1/8 of the bytes), every member publishes its slice of the flattened image (global memory + an epoch-tagged
// ready flag), and wave w of member j multiplies image w of the group into j's rows: W1 moves once per group instead of once per image.  The dot
// products keep their lane <-> k mapping and reduction tree, so every partial sum is bit-identical to the per-image path; they reach the image's
// collector through the same epoch-tagged 64-bit words as before (now from 8 writers per band).  Needs all workgroups co-resident (N x SPLIT <= CUs,
// N a multiple of 64: conv_stack.hip); waits are bounded as everywhere (error word).
#ifndef CS_H_GRP
#define CS_H_GRP 0
#endif
constexpr int head_rpg() { return (CS_H_EA + CS_WAVES - 1) / CS_WAVES; }                   // rows of W1 per group member
__device__ __forceinline__ int grp_member(int img) { return (img >> 3) & 7; }
__device__ __forceinline__ int grp_image(int img, int j) { return (img & ~63) | (img & 7) | (j << 3); }
// W1 PREFETCH (CS_H_PF rows per wave, as many as the LDS left over by the stack holds).  The first linear layer reads the band's slice of
// every row of W1 - 196 KB per workgroup for the LeNet head.  The bytes cannot shrink (a per-sample kernel has no reuse of W1 across images), but their latency can hide: at
// kernel START every wave asks the LDS-DMA engine (global_load_lds_dwordx4: no VGPRs, no instruction slots while in flight) for its first
// CS_H_PF rows, which land under the two convolution stages; the head then reads those rows out of LDS and fetches only the rest.
__device__ __forceinline__ void head_prefetch(const FwdArgs &p, float *L, int img, int band) {
    if constexpr (CS_H_GRP != 0) {                     // this member's rows of W1 (band slice) -> LDS, row ri at head_pf_off() + ri * head_pf_row()
        constexpr int S = CS_NS - 1, row0C = W0(S) * SH[S].C0, E1 = H0(S) * row0C, KI4 = (head_nk_max() / 4 + 63) / 64, RPG = head_rpg();
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int k_lo = po_lo(S, band) * row0C, nk4 = ((po_hi(S, band) - po_lo(S, band)) * row0C) >> 2;
        const int r0 = grp_member(img) * RPG, nr = max(min(CS_H_EA, r0 + RPG) - r0, 0);
        const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) void *)L;
#pragma unroll
        for (int sl = 0; sl < (RPG + CS_WAVES - 1) / CS_WAVES; sl++) {
            const int ri = wave + sl * CS_WAVES;
            if (ri < nr) {
                const unsigned rowb = (unsigned)(((r0 + ri) * E1 + k_lo) * 4);
#pragma unroll
                for (int q = 0; q < KI4; q++) {
                    const int k4 = lane + q * 64;
                    const unsigned voff = rowb + (unsigned)k4 * 16u;
                    const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((head_pf_off() + ri * head_pf_row() + q * 256) * 4));
                    if (k4 < nk4) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(p.hd.W1), "s"(la) : "memory");
                }
            }
        }
    } else
    if constexpr (CS_H_PF > 0 && head_v4_ok()) {
        constexpr int S = CS_NS - 1, row0C = W0(S) * SH[S].C0, E1 = H0(S) * row0C, KI4 = (head_nk_max() / 4 + 63) / 64;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int k_lo = po_lo(S, band) * row0C, nk4 = ((po_hi(S, band) - po_lo(S, band)) * row0C) >> 2;
        const HeadRows hr = head_rows(img, band);
        const unsigned lds0 = (unsigned)(unsigned long long)(__attribute__((address_space(3))) void *)L;
#pragma unroll
        for (int sl = 0; sl < CS_H_PF; sl++) {
            if (sl < hr.nrw) {
                const unsigned rowb = (unsigned)((hr.row(sl) * E1 + k_lo) * 4);
#pragma unroll
                for (int q = 0; q < KI4; q++) {
                    const int k4 = lane + q * 64;
                    const unsigned voff = rowb + (unsigned)k4 * 16u;
                    const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((head_pf_off() + (wave * CS_H_PF + sl) * head_pf_row() + q * 256) * 4));
                    if (k4 < nk4) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(p.hd.W1), "s"(la) : "memory");
                }
            }
        }
    }
}
// The lanes' shares of NR dot products added up across the wave, all rows SIDE BY SIDE: one butterfly step of every row is issued before the first is waited
// for.  A row's own chain - six dependent cross-lane exchanges through the LDS crossbar, ~110 cycles each - is unchanged, so every sum keeps its order and
// its bits; done row after row, the 13 rows of a wave's share of W1 were 78 exchange latencies in a chain (8.6 k of the matvec's 10.2 k cycles, and the
// reason neither a prefetch of W1 nor a warm L2 ever changed it); side by side they are 6.
// Since round 9 the steps themselves run on the vector ALUs (lane_ops.h, in front of this text: lane swaps and DPP, the same pairs i <-> i ^ off in the same
// order, so the same bits) and no step waits for the LDS counter.  CS_LANES_XBAR (lab builds: T4K_STACK_LANES_XBAR=1) selects the crossbar form for the stamped
// timeline.  Either form reads lanes whatever EXEC says or needs them all: every call site below is wave-uniform with 64 live lanes.
#ifndef CS_LANES_XBAR
#define CS_LANES_XBAR 0
#endif
template <int NR> __device__ __forceinline__ void lanes_sum(float (&a)[NR]) {
    if constexpr (CS_LANES_XBAR == 0) lanes_sum_valu(a);
    else {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            float t[NR];
#pragma unroll
            for (int r = 0; r < NR; r++) t[r] = __shfl_xor(a[r], off, 64);
#pragma unroll
            for (int r = 0; r < NR; r++) a[r] += t[r];
        }
    }
}
__device__ __forceinline__ float lanes_max1(float v) {
    if constexpr (CS_LANES_XBAR == 0) { float a[1] = {v}; lanes_max_valu(a); return a[0]; }
    else {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
        return v;
    }
}
__device__ __forceinline__ void lanes_argmax1(float &bm, int &bi) {      // largest value, lowest index among its holders (k_hit's first-arg-max rule)
    if constexpr (CS_LANES_XBAR == 0) { float m[1] = {bm}; int i[1] = {bi}; lanes_argmax_valu(m, i); bm = m[0]; bi = i[0]; }
    else {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float m2 = __shfl_xor(bm, off, 64); const int i2 = __shfl_xor(bi, off, 64);
            if (m2 > bm || (m2 == bm && i2 < bi)) { bm = m2; bi = i2; }
        }
    }
}
__device__ __forceinline__ void head_fwd(const FwdArgs &p, float *L, int img, int band) {
    constexpr int S = CS_NS - 1, row0C = W0(S) * SH[S].C0, E1 = H0(S) * row0C, EA = CS_H_EA, EB = CS_H_EB, MID = CS_H_MID;
    constexpr int nk_max_ = own_rows_max(S) * row0C, KI = (nk_max_ + 63) / 64, RB = KI <= 9 ? 7 : (KI <= 12 ? 5 : 3);      // rows of W1 in flight per trip (RB x KI registers)
    const HeadArgs &h = p.hd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k_lo = po_lo(S, band) * row0C, nk = (po_hi(S, band) - po_lo(S, band)) * row0C;
    const float *x = L + in_off(S);
    float *part = L + out_off(), *x2 = part + ((EA + 3) & ~3), *y2 = x2 + ((EA + 3) & ~3);
    // 16-byte loads when every band's slice of a W1 row starts and ends on a 16-byte boundary (LeNet: 560 | 420 floats): a quarter of the load
    // instructions for the same bytes.  The matvec moves N x E1 x EA x 4 bytes through the L2s (50 MB for the LeNet head: every image reads W1
    // once - a per-sample kernel has no reuse across images); what the phase costs is one round trip, those bytes through the CU's L1 and the
    // lanes' sums (lanes_sum above: they were most of it while they ran row after row).
    constexpr bool V4 = head_v4_ok();
    CS_STAMP(11);
    // The collector's later operands depend on nothing computed here: their loads leave in front of the first trip's W1 loads, in the same round trip (issued
    // behind the matvec they were a round trip of their own in front of the second linear layer).  The sched_barrier behind the W1 load loops keeps them there.
    constexpr int NR2 = (EB + CS_WAVES - 1) / CS_WAVES, NE2 = (EA + 63) / 64;
    float w2v[NR2][NE2], b1v = 0.f, b2v[NR2];
    u32 lbl = 0;                                                  // the image's label, when the one-hot row and the hit flag ride along (HeadArgs)
    if (CS_SPLIT == 1 || band == CS_SPLIT - 1) {
#pragma unroll
        for (int r = 0; r < NR2; r++) {
#pragma unroll
            for (int q = 0; q < NE2; q++) { const int j = wave + r * CS_WAVES, e = lane + q * 64; w2v[r][q] = (j < EB && e < EA) ? h.W2[(long)j * EA + e] : 0.f; }
            const int j = wave + r * CS_WAVES; b2v[r] = (h.B2 && j < EB) ? h.B2[j] : 0.f;
        }
        if (tid < EA && h.B1) b1v = h.B1[tid];
        if (h.hit_flag && (u32)img < h.n_label) lbl = h.label[img];
    }
#if CS_H_GRP
    {
        static_assert(head_v4_ok(), "group head: 16-byte row geometry");
        constexpr int KI4 = (nk_max_ / 4 + 63) / 64, RPG = head_rpg();
        const int nk4 = nk >> 2;
        // ---- A: this band's slice of the flattened image -> memory, then the ready flag.  NO release fence: at agent scope that is a write-back of the
        // whole L2 (buffer_wbl2: +40 us with every layer tensor of the step dirty in it - measured).  The slice leaves with system-scope write-through
        // stores instead (sc0 sc1: they are acknowledged once the data is beyond the L2), the flag follows them after vmcnt(0), and the readers use
        // system-scope loads (past their L1 and L2): only these 2 KB are made coherent, and no assumption is made about which XCD a partner runs on.
        float *xmine = h.xs + (long)img * E1 + k_lo;
        for (int k4 = tid; k4 < nk4; k4 += CS_THREADS) {
            const v4f v = *reinterpret_cast<const v4f *>(x + 4 * k4);
            asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(xmine + 4 * k4), "v"(v) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the slice is out; this wave's W1 DMA (invisible to the compiler's counters) has landed
        lds_barrier();                                               // ... so has every other wave's: all RPG rows are in LDS
        if (tid == 0) __hip_atomic_store(h.xflag + (long)img * CS_SPLIT + band, h.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        // ---- B: wave w takes image w of the group through this member's rows
        const int gi = grp_image(img, wave);
        {
            const u32 *fl = h.xflag + (long)gi * CS_SPLIT + band;
            u32 f = __hip_atomic_load(fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            for (int it = 0; f != h.epoch; it++) {
                if (it > (1 << 22)) { if (h.spin_err) __hip_atomic_store(h.spin_err, 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                __builtin_amdgcn_s_sleep(1);
                f = __hip_atomic_load(fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        v4f xq[KI4];
        {
            const float *xg = h.xs + (long)gi * E1 + k_lo;
#pragma unroll
            for (int q = 0; q < KI4; q++) {
                const int k4 = lane + q * 64;
                asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1" : "=v"(xq[q]) : "v"(xg + 4 * (k4 < nk4 ? k4 : 0)) : "memory");
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int q = 0; q < KI4; q++) { const int k4 = lane + q * 64; if (k4 >= nk4) xq[q] = v4f{0.f, 0.f, 0.f, 0.f}; }
        }
        const int r0 = grp_member(img) * RPG, nr = max(min(EA, r0 + RPG) - r0, 0);
        u64 *slot = h.slots + ((long)gi * CS_SPLIT + band) * EA + r0;
#pragma unroll
        for (int ri = 0; ri < RPG; ri++) {
            const float *src = L + head_pf_off() + ri * head_pf_row();
            float a = 0.f;
#pragma unroll
            for (int q = 0; q < KI4; q++) {
                const int k4 = lane + q * 64;
                const v4f w = *reinterpret_cast<const v4f *>(src + 4 * (k4 < nk4 ? k4 : 0));
                a = fmaf(xq[q][0], w[0], a); a = fmaf(xq[q][1], w[1], a); a = fmaf(xq[q][2], w[2], a); a = fmaf(xq[q][3], w[3], a);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
            if (lane == 0 && ri < nr) __hip_atomic_store(slot + ri, ((u64)h.epoch << 32) | (u64)__float_as_uint(a), __ATOMIC_RELAXED, CS_XSCOPE);
        }
    }
#elif defined(CS_LAB_NOW1)
    if (tid < EA) part[tid] = x[tid % 64];
#else
    if (V4) {
        constexpr int KI4 = (nk_max_ / 4 + 63) / 64, RPW = (EA + CS_WAVES - 1) / CS_WAVES;      // float4 per lane per row, rows per wave
        constexpr int PF = CS_H_PF < RPW ? CS_H_PF : RPW, RG = RPW - PF;                         // slots [0, PF) were prefetched into LDS, [PF, nrw) come from global
        constexpr int RB4 = RG == 0 ? 1 : (RG * KI4 * 4 <= 160 ? RG : (RG + 1) / 2);            // all of a wave's global rows in ONE round trip when they fit the registers
        const int nk4 = nk >> 2;
        const HeadRows hr = head_rows(img, band);
        v4f xq[KI4];
#pragma unroll
        for (int q = 0; q < KI4; q++) { const int k4 = lane + q * 64; xq[q] = k4 < nk4 ? *reinterpret_cast<const v4f *>(x + 4 * k4) : v4f{0.f, 0.f, 0.f, 0.f}; }
        auto dot_lane = [&](const v4f (&wr)[KI4]) {                                                // this lane's share of a row's dot product (lanes_sum adds the lanes up)
            float a = 0.f;
#pragma unroll
            for (int q = 0; q < KI4; q++) { a = fmaf(xq[q][0], wr[q][0], a); a = fmaf(xq[q][1], wr[q][1], a); a = fmaf(xq[q][2], wr[q][2], a); a = fmaf(xq[q][3], wr[q][3], a); }
            return a;
        };
        for (int e0 = PF, trip = 0; e0 < hr.nrw || trip == 0; e0 += RB4, trip++) {
            v4f wq[RB4][KI4]; int row[RB4];
            if (RG > 0) {
#pragma unroll
                for (int r = 0; r < RB4; r++) {
                    row[r] = e0 + r < hr.nrw ? hr.row(e0 + r) : -1;
                    const v4f *w = reinterpret_cast<const v4f *>(h.W1 + (long)max(row[r], 0) * E1 + k_lo);
#pragma unroll
                    for (int q = 0; q < KI4; q++) { const int k4 = lane + q * 64; wq[r][q] = w[k4 < nk4 ? k4 : 0]; }
                }
            }
            __builtin_amdgcn_sched_barrier(0);                    // every load of the trip is issued before the first row is consumed: ONE round trip (the scheduler would otherwise
                                                                  // sink loads between the rows' multiply-adds to save registers, a dependent round trip each)
            if (PF > 0 && trip == 0) {
                // the prefetched rows first, while those loads fly.  vmcnt counts in issue order: once no more than the loads just issued are
                // outstanding, this wave's DMA transfers (its oldest vector-memory operations) have landed; a wave reads only rows it fetched itself
                if (RG > 0) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(RB4 * KI4 < 63 ? RB4 * KI4 : 63) : "memory");
                else        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                float al[PF > 0 ? PF : 1];
#pragma unroll
                for (int sl = 0; sl < PF; sl++) {
                    v4f wl[KI4];
                    const float *src = L + head_pf_off() + (wave * CS_H_PF + sl) * head_pf_row();
#pragma unroll
                    for (int q = 0; q < KI4; q++) { const int k4 = lane + q * 64; wl[q] = *reinterpret_cast<const v4f *>(src + 4 * (k4 < nk4 ? k4 : 0)); }
                    al[sl] = dot_lane(wl);
                }
                lanes_sum(al);
#pragma unroll
                for (int sl = 0; sl < PF; sl++) if (lane == 0 && sl < hr.nrw) part[hr.row(sl)] = al[sl];
            }
            if (RG > 0) {
                float ar[RB4];
#pragma unroll
                for (int r = 0; r < RB4; r++) ar[r] = dot_lane(wq[r]);
                lanes_sum(ar);
#pragma unroll
                for (int r = 0; r < RB4; r++) if (lane == 0 && row[r] >= 0) part[row[r]] = ar[r];
            }
        }
    } else {
        float xv[KI];
#pragma unroll
        for (int q = 0; q < KI; q++) { const int k = lane + q * 64; xv[q] = k < nk ? x[k] : 0.f; }
        for (int e0 = wave * RB; e0 < EA; e0 += CS_WAVES * RB) {        // RB rows of W1 per trip: their loads are all in flight together
            float wv[RB][KI];
#pragma unroll
            for (int r = 0; r < RB; r++) {
                const float *w = h.W1 + (long)min(e0 + r, EA - 1) * E1 + k_lo;
#pragma unroll
                for (int q = 0; q < KI; q++) { const int k = lane + q * 64; wv[r][q] = w[k < nk ? k : 0]; }
            }
            __builtin_amdgcn_sched_barrier(0);                    // (as above: all loads of the trip first)
            float ar[RB];
#pragma unroll
            for (int r = 0; r < RB; r++) {
                float a = 0.f;
#pragma unroll
                for (int q = 0; q < KI; q++) a = fmaf(xv[q], wv[r][q], a);
                ar[r] = a;
            }
            lanes_sum(ar);
#pragma unroll
            for (int r = 0; r < RB; r++) if (lane == 0 && e0 + r < EA) part[e0 + r] = ar[r];
        }
    }
#endif
    CS_STAMP(12);
    lds_barrier();
#if CS_H_GRP
    if (band < CS_SPLIT - 1) return;                              // every band's partial sums are on their way to the collectors
#else
    if (CS_SPLIT > 1 && band < CS_SPLIT - 1) {                    // publisher
        if (tid < EA) {
            const u64 wv_ = ((u64)h.epoch << 32) | (u64)__float_as_uint(part[tid]);
            __hip_atomic_store(h.slots + ((long)img * (CS_SPLIT - 1) + band) * EA + tid, wv_, __ATOMIC_RELAXED, CS_XSCOPE);
        }
        return;
    }
#endif
    if (tid < EA) {
        const long z = (long)img * EA + tid;
        float y = 0.f;
        constexpr int NPUB = CS_H_GRP ? CS_SPLIT : CS_SPLIT - 1;      // group head: the collector's own band arrives through the words as well (from its group)
        // the dropout draw is a function of the position alone: its ten Philox rounds run here, in front of the poll, and only u01 and act1 stay behind it.
        // (The empty asm takes the words as operands: they exist at this point, whatever the compiler would rather sink behind the poll loop.)
        u32 rz = 0;
        if (MID == L_DROPOUT) {
            u32 r[4]; philox4x32_10(h.base + (u64)(z >> 2), h.seed, r);
            rz = r[z & 3];
            asm volatile("" : "+v"(rz));
        }
        if (NPUB > 0) {
#pragma unroll
            for (int b = 0; b < NPUB; b++) {
                const u64 *sl = h.slots + ((long)img * NPUB + b) * EA + tid;
                u64 v = __hip_atomic_load(sl, __ATOMIC_RELAXED, CS_XSCOPE);
#ifdef CS_LAB_NOXCHG
                for (int it = 0; false; it++) {
#else
                for (int it = 0; (u32)(v >> 32) != h.epoch; it++) {
#endif
                    if (it > (1 << 22)) { if (h.spin_err) __hip_atomic_store(h.spin_err, 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                    __builtin_amdgcn_s_sleep(1);
                    v = __hip_atomic_load(sl, __ATOMIC_RELAXED, CS_XSCOPE);
                }
                y += __uint_as_float((u32)v);
            }
        }
        CS_STAMP(15);
        if (!CS_H_GRP) y += part[tid];
        y += b1v;
        h.Y1[z] = y;
        float o = y, f = 1.f;
        if (MID) {
            act1<MID>(y, MID == L_DROPOUT ? u01(rz) : 0.f, CS_H_ALPHA, o, f);
            h.Fm[z] = f; h.Am[z] = o;
        }
        x2[tid] = o;
        CS_STAMP(16);
    }
    lds_barrier();
    CS_STAMP(13);
    float a2[NR2];
#pragma unroll
    for (int r = 0; r < NR2; r++) {                                 // second linear layer: a wave per output, lanes along its EA inputs
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < NE2; q++) { const int e = lane + q * 64; a = fmaf(e < EA ? x2[e] : 0.f, w2v[r][q], a); }
        a2[r] = a;
    }
    lanes_sum(a2);
    CS_STAMP(17);
#pragma unroll
    for (int r = 0; r < NR2; r++) { const int j = wave + r * CS_WAVES; if (lane == 0 && j < EB) y2[j] = a2[r] + b2v[r]; }
    lds_barrier();
    if (tid < 64) {                                               // softmax over the EB outputs (k_softmax's arithmetic, as k_linsmall_fwd)
        const bool live = tid < EB;
        const float v = live ? y2[tid] : -3.402823466e+38f;
        const float mx = lanes_max1(v);
        CS_STAMP(18);
        const float e = live ? __expf(v - mx) : 0.f;
        float sm1[1] = {e};
        lanes_sum(sm1);
        CS_STAMP(19);
        const float pv = e / sm1[0];
        if (live) { h.Y2[(long)img * EB + tid] = v; if (h.P) h.P[(long)img * EB + tid] = pv; }
        if (h.hit_flag) {                                         // Model::onehot(Dataset&) + hit (loss.cpp:47-72, forward.cu:57-60; k_hit's first-arg-max rule) for this image
            float bm = live ? pv : -3.402823466e+38f; int bi = live ? tid : 0x7fffffff;
            lanes_argmax1(bm, bi);
            const bool lab = (u32)img < h.n_label;
            const int m = lbl < (u32)EB ? (int)lbl : 0;
            if (lab && live) h.hot[(long)img * EB + tid] = tid == m ? 1.0f : 0.0f;
            if (tid == 0) h.hit_flag[img] = (lab && bi == m) ? 1 : 0;
        }
    }
    CS_STAMP(14);
}
#endif

extern "C" __global__ void __launch_bounds__(CS_THREADS) cs_fwd(const FwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    const int img = blockIdx.x, band = blockIdx.y, tid = threadIdx.x;
    CS_STAMP(0);
    // ---- every global load this workgroup needs, issued before anything waits: its rows of the image, the filters, the biases
    constexpr int K0 = SH[0].K, P0 = K0 / 2, wc0 = SH[0].W * SH[0].C1, RS0 = (SH[0].W + K0 - 1) * SH[0].C1;
    const int cl0 = pc_lo(0, band) * SH[0].KS, ch0 = pc_hi(0, band) * SH[0].KS;
    const int ir_lo = max(cl0 - P0, 0), ir_hi = min(ch0 + P0, SH[0].H);       // image rows in the window
    const int nimg = (ir_hi - ir_lo) * wc0;
    const float *xg = p.X + ((long)img * SH[0].H + ir_lo) * wc0;
    constexpr int NI = ((nr_max(0) + K0 - 1) * wc0 + CS_THREADS - 1) / CS_THREADS;
    float vi[NI], vf[CS_NS][8], vb[CS_NS];
#pragma unroll
    for (int q = 0; q < NI; q++) { const int e = tid + q * CS_THREADS; vi[q] = e < nimg ? xg[e] : 0.f; }
    load_filter<0>(p, vf, vb);
    // ---- zero the padded windows / operands while those are in flight
    for (int e = tid * 4; e < out_off(); e += CS_THREADS * 4) *reinterpret_cast<float4 *>(L + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    lds_barrier();
    CS_STAMP(1);
    {   // the image rows: into stage 0's window, and (owned rows) the model's layer-0 copy of the batch (forward.cu:39)
        const int own_lo = (po_lo(0, band) * SH[0].KS - ir_lo) * wc0, own_hi = (po_hi(0, band) * SH[0].KS - ir_lo) * wc0;
        float *x0 = p.X0 ? p.X0 + ((long)img * SH[0].H + ir_lo) * wc0 : nullptr;
        float *xs = p.st[0].save_x ? p.st[0].save_x + ((long)img * SH[0].H + ir_lo) * wc0 : nullptr;
#pragma unroll
        for (int q = 0; q < NI; q++) {
            const int e = tid + q * CS_THREADS;
            if (e < nimg) {
                const int y = e / wc0, r = e - y * wc0;
                L[in_off(0) + (y + ir_lo - (cl0 - P0)) * RS0 + P0 * SH[0].C1 + r] = vi[q];
                if (x0 && e >= own_lo && e < own_hi) gstore1<ST_FWD>(x0 + e, vi[q]);
                if (xs && e >= own_lo && e < own_hi) xs[e] = vi[q];
            }
        }
    }
    put_filter<0>(L, vf, vb);
#ifdef CS_HEAD
    // Issued only now, behind the last consumer of the loads above: the compiler does not see these transfers in its vmcnt bookkeeping, and a
    // counted wait for an OLDER load issued with them in flight would wait for them as well.  From here to the head nothing waits on vmcnt.
    head_prefetch(p, L, img, band);
#endif
    lds_barrier();
    CS_STAMP(2);
    stage_fwd<0>(p, L, img, band);
#ifdef CS_HEAD
    head_fwd(p, L, img, band);
#endif
}
#ifndef CS_ONLY_FWD

// ======================================================================================================== backward
// One workgroup per IMAGE (no bands: the reference's in-place convention - every layer's input buffer receives its dX - would let
// a neighbouring band overwrite forward values this band still needs for an arg-max or a dF halo).  Per stage, last to first:
//   run backward  (k_poolblock_bwd's arithmetic: flatten `in = out`, mask multiplies, pool scatter with first-extreme-wins) from dY
//                 (global for the last stage, the previous step's dX in LDS otherwise) -> every run tensor's dX to global, dO into
//                 a zero-bordered LDS window
//   dF | dB       per-image partials: dF[(ky, kx*C1+c1), c0] = sum over pixels X[(y+ky-P), (x+kx-P), c1] * dO[y, x, c0] on MFMA
//                 (M = filter taps x input channels, N = c0, contraction = pixels, 4 per step), dB = column sums of dO; written to
//                 this image's row of the partial slab in the filter's own layout - cs_fold adds the rows up in image order
//   dX            the forward conv routine on the dO window with the SAME tap order (the reference's dX is the un-flipped correlation
//                 of dO with F, nmath.tcu:304-324) -> LDS (the next step's dY), the conv input tensor (`in = dx`) and its scratch copy
struct BwdStage {
    const float *F;                                  // filter
    float *O, *P, *Q, *R;                            // conv output, pre out, pool out, post out: forward values in, dX of the layer behind out
    const float *Fpre, *Fpost;                       // derivative masks
    float *X, *DXS;                                  // conv input tensor (forward values in, dX out) and the optional second dX copy
    const float *save_x; const unsigned char *save_am;   // banded backward: the forward's copy of the conv input and its pool arg-max codes
};
// train: bit 0 = parameter gradients wanted, bit 1 (banded kernel) = skip the dX of stage 0 (nobody reads the first layer's dX in a
// classifier's training loop; f0_save then receives a copy of stage 0's filter so the host can still produce it later, t4k_conv_stack_dx0)
struct BwdArgs { const float *DY; float *part; u64 *prof; float *f0_save; int N, train; BwdStage st[CS_NS]; };

constexpr int nF(int s) { return SH[s].C1 * SH[s].K * SH[s].K * SH[s].C0; }
// Row strides of the BACKWARD's LDS windows (X window, dO window), padded to 16 mod 32 floats.  The dF partial's MFMA contraction runs over
// 4 consecutive ROWS of one pixel column (k = lane / 16): a ds_read_b32 is served 32 lanes at a time = k rows (kq, kq + 1) x 16 lanes of
// consecutive floats, so the two rows must sit 16 banks apart - with the round-4 layout (k = 4 consecutive pixels, pitch C0 = 20 floats)
// every B read and the wrapped A reads were 2-way conflicts (SQ_LDS_BANK_CONFLICT 45 % of SQ_LDS_IDX_ACTIVE in cs_bwd_b, VERDICT r4).
constexpr int p16of32(int n) { return n + ((16 - n % 32) % 32 + 32) % 32; }
constexpr int RSXw(int s) { return p16of32((SH[s].W + SH[s].K - 1) * SH[s].C1); }
constexpr int RSOw(int s) { return p16of32((SH[s].W + SH[s].K - 1) * SH[s].C0); }
constexpr int part_off(int s) { int o = 0; for (int t = 0; t < s; t++) o += pad4(nF(t) + SH[t].C0); return o; }
constexpr int part_row() { return part_off(CS_NS - 1) + pad4(nF(CS_NS - 1) + SH[CS_NS - 1].C0); }
// LDS plan, backward (whole image): per stage the dX-conv filter; shared by the stages (sized by the largest): dO window, X window,
// dX buffers (two: stage S reads the one stage S+1 wrote), dF partial slots
constexpr int wb_size(int s) { return pad4(cmax(SH[s].K * JPb(s) * NCb(s), nF(s))); }
constexpr int wb_off(int s) { int o = 0; for (int t = 0; t < s; t++) o += wb_size(t); return o; }
constexpr int do_size() { int m = 0; for (int s = 0; s < CS_NS; s++) m = cmax(m, (SH[s].H + SH[s].K - 1) * RSOw(s) + 16); return pad4(m); }
constexpr int xw_size() { int m = 0; for (int s = 0; s < CS_NS; s++) m = cmax(m, (SH[s].H + SH[s].K - 1) * RSXw(s) + 16); return pad4(m); }
constexpr int dx_size() { int m = 0; for (int s = 0; s < CS_NS; s++) m = cmax(m, SH[s].H * SH[s].W * SH[s].C1); return pad4(m); }
constexpr int df_units(int s) { return ((SH[s].K * SH[s].K * SH[s].C1 + 15) / 16) * NT(s); }          // (tile of the K*K*C1 taps, tile of c0)
constexpr int cgcd(int a, int b) { return b == 0 ? a : cgcd(b, a % b); }
constexpr int df_mgn_(int s) { const int mtt = (SH[s].K * SH[s].K * SH[s].C1 + 15) / 16, mg = cmin(mtt, 3); return (mtt + mg - 1) / mg; }
constexpr int DF_WAVES = 8;                                                                        // waves that take dF items - in cs_bwd the whole workgroup, in cs_bwd_b its dF role: the slot geometry is the same in both
constexpr int df_rg(int s) { return cmin(DF_WAVES / cgcd(df_mgn_(s), DF_WAVES), cmax(1, SH[s].W / 2)); }   // pixel-column groups per M-tile block: work items a multiple of the wave count
constexpr int slot_size() { int m = 0; for (int s = 0; s < CS_NS; s++) { const int mtt = (SH[s].K * SH[s].K * SH[s].C1 + 15) / 16, mg = cmin(mtt, 3); m = cmax(m, df_mgn_(s) * df_rg(s) * mg * NT(s) * 256 + 16 * SH[s].C0); } return pad4(m); }
constexpr int do_off() { return wb_off(CS_NS - 1) + wb_size(CS_NS - 1); }
constexpr int xw_off() { return do_off() + do_size(); }
constexpr int dx_off(int which) { return xw_off() + xw_size() + which * dx_size(); }
constexpr int slot_off() { return dx_off(2); }
constexpr int bwd_lds_floats() { return slot_off() + slot_size(); }

template <int S> __device__ __forceinline__ int wl_bwd(int e) {       // filter element -> dX conv B operand: Wl[(ky*JPb + kx*C0 + c0) * NCb + c1]
    constexpr int C0 = SH[S].C0, K = SH[S].K;
    const int c0 = e % C0, t = e / C0, kx = t % K, t2 = t / K, ky = t2 % K, c1 = t2 / K;
    return (ky * JPb(S) + kx * C0 + c0) * NCb(S) + c1;
}
// NTH = threads of the workgroup, VFQ = filter elements a thread stages (8 x 512 = 4 x 1024 = the largest filter the host admits)
template <int S, int NTH = CS_THREADS, int VFQ = 8> __device__ __forceinline__ void load_filter_b(const BwdArgs &p, float (&vf)[CS_NS][VFQ]) {
    if constexpr (S < CS_NS) {
        static_assert(nF(S) <= VFQ * NTH, "filter too large for the register-staged path");
#pragma unroll
        for (int q = 0; q < (nF(S) + NTH - 1) / NTH; q++) { const int e = threadIdx.x + q * NTH; vf[S][q] = e < nF(S) ? p.st[S].F[e] : 0.f; }
        load_filter_b<S + 1, NTH, VFQ>(p, vf);
    }
}
template <int S, int NTH = CS_THREADS, int VFQ = 8> __device__ __forceinline__ void put_filter_b(float *L, const float (&vf)[CS_NS][VFQ]) {
    if constexpr (S < CS_NS) {
#pragma unroll
        for (int q = 0; q < (nF(S) + NTH - 1) / NTH; q++) { const int e = threadIdx.x + q * NTH; if (e < nF(S)) L[wb_off(S) + ((SH[S].C1 <= 4 && nF(S) <= 160) ? e : wl_bwd<S>(e))] = vf[S][q]; }   // few input channels, small filter: verbatim (dx_valu)
        put_filter_b<S + 1, NTH, VFQ>(L, vf);
    }
}

// run backward of stage S for one image: dY (global or LDS, [H0][W0][C]) -> tensors (global) + dO window (LDS, zero border).
// A lane handles CV consecutive channels of one pooled pixel (vector loads / stores); ALL its global loads (dY, masks, the pool window's
// forward values) are issued before the first store - a store in between would make the compiler wait for it before the next load
// of a may-alias buffer, one HBM round trip per element.
// Pooled rows [ql, qh) are processed (dY in LDS and the dO window start at row ql), rows [pol, poh) are stored.  SAVED: the pool's winning
// cell comes from the forward's arg-max codes instead of the forward values in the pool's input buffer (banded backward: a neighbouring
// band overwrites those in place).  POL: the store policy of every dX tensor the run writes (cs_bwd_b: ST_BWD; cs_bwd shares this routine and keeps plain stores).
template <int S, bool SAVED, int NTH = CS_THREADS, int POL = ST_PLAIN>
__device__ __forceinline__ void run_bwd(const BwdStage &g, const float *dY, bool dy_global, float *dOw, int img, int ql = 0, int qh = H0(S), int pol = 0, int poh = H0(S)) {
    constexpr int W = SH[S].W, C = SH[S].C0, KS = SH[S].KS, K = SH[S].K, PD = K / 2, PRE = SH[S].pre, POOL = SH[S].pool, POST = SH[S].post;
    constexpr int CV = vw_of(C), CQ = C / CV, RSO = RSOw(S), NW = POOL ? 4 : 1;
    const int NIT = (qh - ql) * W0(S) * CQ;
    const long e0 = (long)img * H0(S) * W0(S) * C, e1 = (long)img * SH[S].H * W * C;
    // the buffers of the run, in the reference's in-place convention (k_poolblock_bwd, fused.hip)
    float *Rb = SH[S].flat ? (POST ? g.R : (POOL ? g.Q : (PRE ? g.P : g.O))) : nullptr;     // flatten: in = out
    float *Qb = POOL ? g.Q : (PRE ? g.P : g.O);                                             // the post activation's input buffer
    float *Pb = PRE ? g.P : g.O;                                                            // pool input buffer: forward values -> dX
    for (int it = threadIdx.x; it < NIT; it += NTH) {
        const int cq = it % CQ, t = it / CQ, j0 = t % W0(S), ir = t / W0(S), i0 = ql + ir, c = cq * CV;
        const int lo = (i0 * W0(S) + j0) * C + c, lloc = (ir * W0(S) + j0) * C + c;
        const long zo = e0 + lo;
        const bool own = i0 >= pol && i0 < poh;
        const int l1 = ((i0 * KS) * W + j0 * KS) * C + c;                   // first cell of the window in the conv grid
        const int cell[4] = { l1, l1 + C, l1 + W * C, l1 + W * C + C };
        // ---- loads
        VecF<CV> gq, fpost, ev[NW], fv[NW];
        if (dy_global) gq = gload<CV>(dY + zo);
        else gq = lload<CV>(dY + lloc);                          // (dX buffer of the stage above: CV-float aligned; CV scalar reads at a lane stride of CV floats are CV-way conflicts)
        if (POST) fpost = gload<CV>(g.Fpost + zo);
        u32 amw = 0;
        if (SAVED && POOL && POOL != L_AVGPOOL) {
            if (CV == 4) amw = *reinterpret_cast<const u32 *>(g.save_am + zo);
            else {
#pragma unroll
                for (int q = 0; q < CV; q++) amw |= (u32)g.save_am[zo + q] << (8 * q);
            }
        }
#pragma unroll
        for (int w = 0; w < NW; w++) {
            if (!SAVED && POOL && POOL != L_AVGPOOL) ev[w] = gload<CV>(Pb + e1 + cell[w]);
            if (PRE) fv[w] = gload<CV>(g.Fpre + e1 + cell[w]);
        }
        // ---- arithmetic + stores
        if (Rb && own) gstore<CV, POL>(Rb + zo, gq.v);
        if (POST) {
#pragma unroll
            for (int q = 0; q < CV; q++) gq.v[q] *= fpost.v[q];
            if (own) gstore<CV, POL>(Qb + zo, gq.v);
        }
        int arg[CV];
#pragma unroll
        for (int q = 0; q < CV; q++) {
            arg[q] = SAVED ? (int)((amw >> (8 * q)) & 3u) : 0;
            if (!SAVED && POOL && POOL != L_AVGPOOL) {
                float best = ev[0].v[q];
#pragma unroll
                for (int w = 1; w < NW; w++) { const bool better = POOL == L_MAXPOOL ? ev[w].v[q] > best : ev[w].v[q] < best; if (better) { best = ev[w].v[q]; arg[q] = w; } }   // first extreme wins
            }
        }
#pragma unroll
        for (int w = 0; w < NW; w++) {
            float d[CV];
#pragma unroll
            for (int q = 0; q < CV; q++) d[q] = !POOL ? gq.v[q] : (POOL == L_AVGPOOL ? gq.v[q] / 4.0f : (arg[q] == w ? gq.v[q] : 0.f));
            if (POOL && own) gstore<CV, POL>(Pb + e1 + cell[w], d);
            if (PRE) {
#pragma unroll
                for (int q = 0; q < CV; q++) d[q] *= fv[w].v[q];
                if (own) gstore<CV, POL>(g.O + e1 + cell[w], d);
            }
            const int wy = ir * KS + (w >> 1), wx = j0 * KS + (w & 1);
            lstore<CV>(dOw + (wy + PD) * RSO + (wx + PD) * C + c, d);      // one ds_write_b128 / b64 (CV scalar writes at a lane stride of CV floats are CV-way bank conflicts)
        }
    }
}

// per-image dF | dB partial of stage S: X window (LDS, zero border, [H+K-1][W+K-1][C1]) and dO window (LDS, [H+K-1][W+K-1][C0]).
// GEMM with M = the K*K*C1 filter taps (a lane's A row is ITS tap: row offset ky, column offset kx*C1 + c1 - no padding per ky),
// N = c0, contraction over the pixels of a row, 4 per MFMA step.  A wave takes a block of MG M tiles x all N tiles for one group
// of rows: MG + NT LDS reads feed MG*NT MFMAs per step (one read per operand per MFMA would saturate the LDS before the MFMA pipe),
// and the MG*NT accumulator chains are independent.
// lab builds (T4K_STACK_LAB_SKIP): phases of the banded backward left out - timing / counters only, wrong results: 1 dF partial, 2 dX conv, 4 run backward, 8 X window fill,
// 16 window zero fill, 32 dX copy-out, 64 the dF partial's MFMAs (operand reads kept), 128 its fold, 256 its slot writes
#ifdef CS_LAB_SKIP
constexpr int LAB_SKIP = CS_LAB_SKIP;
#else
constexpr int LAB_SKIP = 0;
#endif
constexpr int df_mg(int s) { return cmin((SH[s].K * SH[s].K * SH[s].C1 + 15) / 16, 3); }
constexpr int df_mgn(int s) { return ((SH[s].K * SH[s].K * SH[s].C1 + 15) / 16 + df_mg(s) - 1) / df_mg(s); }
// Two parts with a workgroup barrier between them: df_items (waves 0 .. DF_WAVES - 1: the MFMA items into the LDS slots, dB column sums) and
// df_fold (NTH threads: fold of the slots in a fixed order, partial-row stores).  cs_bwd runs them back to back (df_partial); cs_bwd_b runs the
// items beside the stage's dX and the fold in the store phase behind the barrier the two share.
template <int S, int NRMAX>
__device__ __forceinline__ void df_items(const float *Xw, const float *dOw, float *slots, u64 *prof, int nrows = SH[S].H) {
    constexpr int W = SH[S].W, C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K, PD = K / 2, KC = K * C1, TAPS = K * KC;
    constexpr int NTK = NT(S), MG = df_mg(S), MGN = df_mgn(S), RG = df_rg(S), BLK = MG * NTK * 256;
    constexpr int RSX = RSXw(S), RSO = RSOw(S), YQ = (NRMAX + 3) / 4;      // row quads: MFMA k = 4 consecutive rows of one pixel column
    constexpr bool ONES = (TAPS & 15) != 0;          // a spare row in the last M tile: fed with 1.0 it yields dB = the column sums of dO for free
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, kq = lane >> 4;
    if (S == CS_NS - 1) CS_STAMP_P(prof, 16);
    // the lane's rows: quad yq covers rows 4 yq + kq.  Rows past the band are read from a clamped row (the address stays inside the window) and zeroed
    // by a select - a predicated LDS read costs a compare, an exec-mask save / branch / restore and cannot be batched
    int yoff_x[YQ], yoff_o[YQ]; bool rok[YQ];
#pragma unroll
    for (int yq = 0; yq < YQ; yq++) { const int y = yq * 4 + kq; rok[yq] = y < nrows; const int yc = min(y, nrows - 1); yoff_x[yq] = yc * RSX; yoff_o[yq] = yc * RSO; }
    for (int item = wave; item < MGN * RG; item += DF_WAVES) {
        const int mgi = item / RG, rg = item - mgi * RG;
        const float *a0[MG]; bool one[MG];
#pragma unroll
        for (int m = 0; m < MG; m++) {
            const int t0 = (mgi * MG + m) * 16 + i, tap = min(t0, TAPS - 1), ky = tap / KC, j = tap - ky * KC;     // rows beyond TAPS are discarded below
            a0[m] = Xw + ky * RSX + j; one[m] = ONES && t0 == TAPS;
        }
        const float *b0 = dOw + PD * RSO + PD * C0 + i;
        v4f acc[MG][NTK];
#pragma unroll
        for (int m = 0; m < MG; m++)
#pragma unroll
            for (int n = 0; n < NTK; n++) acc[m][n] = v4f{0.f, 0.f, 0.f, 0.f};
        // an item's pixel columns x = rg, rg + RG, ... (HH of them): with few columns every operand read of the item is issued before its first MFMA - one LDS
        // round trip per item instead of one per pair of columns (round 6: the phase is a chain of LDS latency + MFMA burst + barrier, not a pipe limit)
        constexpr int HH = (W + RG - 1) / RG, HB = HH <= 4 ? HH : 2;       // columns per batch
        for (int x = rg; x < W; x += HB * RG) {
            float av[HB][MG][YQ], bv[HB][NTK][YQ];
#pragma unroll
            for (int h = 0; h < HB; h++) {
                const int xx = x + h * RG; const bool live = xx < W; const int xc = live ? xx : x;
#pragma unroll
                for (int yq = 0; yq < YQ; yq++) {
                    const bool in = live && rok[yq];
#pragma unroll
                    for (int m = 0; m < MG; m++) { const float v = a0[m][yoff_x[yq] + xc * C1]; av[h][m][yq] = in ? (one[m] ? 1.0f : v) : 0.f; }
#pragma unroll
                    for (int n = 0; n < NTK; n++) { const float v = b0[yoff_o[yq] + xc * C0 + n * 16]; bv[h][n][yq] = (in && n * 16 + i < C0) ? v : 0.f; }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int h = 0; h < HB; h++)
#pragma unroll
                for (int yq = 0; yq < YQ; yq++)
#pragma unroll
                    for (int m = 0; m < MG; m++)
#pragma unroll
                        for (int n = 0; n < NTK; n++) {
                            if (LAB_SKIP & 64) acc[m][n][0] += av[h][m][yq] * bv[h][n][yq];
                            else acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[h][m][yq], bv[h][n][yq], acc[m][n], 0, 0, 0);
                        }
        }
#pragma unroll
        for (int m = 0; m < MG; m++)
#pragma unroll
            for (int n = 0; n < NTK; n++)
#pragma unroll
                for (int r = 0; r < 4; r++) if (!(LAB_SKIP & 256) || acc[m][n][r] == 12345.f) slots[item * BLK + (m * NTK + n) * 256 + (4 * r + kq) * 16 + i] = acc[m][n][r];     // D[4*kq + r][i] at row 4 r + kq of the block:
                                                                                                                      // one write = 64 consecutive floats (row 4 kq + r put the four k-quads on the same 16 banks: 4-way conflicts)
    }
    if (S == CS_NS - 1) CS_STAMP_P(prof, 17);
    float *dbs = slots + MGN * RG * BLK;
    if (!ONES && threadIdx.x < 16 * C0) {                      // no spare row: column sums on the vector ALUs, 16 lanes per channel, fixed order
        const int c = threadIdx.x % C0, gq = threadIdx.x / C0;
        float sacc = 0.f;
#pragma unroll 8
        for (int pq = gq; pq < nrows * W; pq += 16) { const int y = pq / W, x = pq - y * W; sacc += dOw[(y + PD) * RSO + (x + PD) * C0 + c]; }
        dbs[gq * C0 + c] = sacc;
    }
}
template <int S, int NTH = CS_THREADS>
__device__ __forceinline__ void df_fold(const float *slots, float *part, u64 *prof) {
    constexpr int C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K, KC = K * C1, TAPS = K * KC;
    constexpr int MTT = (TAPS + 15) / 16, NTK = NT(S), MG = df_mg(S), MGN = df_mgn(S), RG = df_rg(S), BLK = MG * NTK * 256;
    constexpr bool ONES = (TAPS & 15) != 0;
    const float *dbs = slots + MGN * RG * BLK;
    if (S == CS_NS - 1) CS_STAMP_P(prof, 18);
    // fold the row groups (fixed order) and scatter into the filter's own layout ((c1*K + ky)*K + kx)*C0 + c0, VF consecutive c0 per lane
    constexpr int VF = (C0 & 3) == 0 ? 4 : 1;
    for (int e4 = threadIdx.x; e4 < ((LAB_SKIP & 128) ? 0 : MGN * BLK / VF); e4 += NTH) {
        const int e = e4 * VF, mgi = e / BLK, r1 = e - mgi * BLK, mn = r1 >> 8, m = mn / NTK, n = mn - m * NTK, rw = (r1 >> 4) & 15, mm = 4 * (rw & 3) + (rw >> 2), nn = r1 & 15;   // block row rw holds D row mm
        const int tap = ((mgi * MG + m) * 16) + mm, c0 = n * 16 + nn;
        if (mgi * MG + m < MTT && tap <= TAPS && c0 < C0 && (tap < TAPS || ONES)) {
            float v[VF];
#pragma unroll
            for (int q = 0; q < VF; q++) v[q] = 0.f;
#pragma unroll
            for (int rg = 0; rg < RG; rg++)
#pragma unroll
                for (int q = 0; q < VF; q++) v[q] += slots[(mgi * RG + rg) * BLK + r1 + q];
            float *dst;
            if (tap < TAPS) { const int ky = tap / KC, j = tap - ky * KC, kx = j / C1, c1 = j - kx * C1; dst = part + ((c1 * K + ky) * K + kx) * C0 + c0; }
            else dst = part + nF(S) + c0;                        // the ones row: dB
            gstore<VF>(dst, v);
        }
    }
    if (!ONES && threadIdx.x < C0) {
        float v = 0.f;
#pragma unroll
        for (int gq = 0; gq < 16; gq++) v += dbs[gq * C0 + threadIdx.x];
        part[nF(S) + threadIdx.x] = v;
    }
}
template <int S, int NRMAX>
__device__ __forceinline__ void df_partial(const float *Xw, const float *dOw, float *slots, float *part, u64 *prof, int nrows = SH[S].H) {
    df_items<S, NRMAX>(Xw, dOw, slots, prof, nrows);
    lds_barrier();
    df_fold<S>(slots, part, prof);
}

// dX of a conv layer with FEW input channels (C1 <= 4: the image layer) on the vector ALUs: an MFMA tile would be 1..4 useful columns
// of 16.  A lane owns one pixel: dX[y, x, c1] = sum over (ky, kx, c0) F[c1, ky, kx, c0] * dO[y+ky-P, x+kx-P, c0] (the reference's un-flipped
// correlation, nmath.tcu:304-324); the (kx, c0) run of a filter row is contiguous in the dO window, the weights are LDS broadcasts.
// T0 / TN: the threads that share the pixels (the dX role of the banded backward: threads 512 .. 1023); only those threads may call.
// ROWW: the weights are read one filter row at a time inside the pixel loop instead of all K rows once per lane - a third of the registers (the banded
// backward's 1024-thread workgroup may use 128; its bands are at most a pixel or two per thread, so nothing is read twice that was read once before).
template <int S, int T0 = 0, int TN = CS_THREADS, bool ROWW = false>
__device__ __forceinline__ void dx_valu(const float *dOw, const float *Wf, float *dXb, int nrows = SH[S].H) {
    constexpr int H = SH[S].H, W = SH[S].W, C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K, KC0 = K * C0, RSO = RSOw(S);
    constexpr bool PAIR = (C0 & 1) == 0;                  // (x * C0) and the row stride are even: 8-byte LDS reads
    float wv[C1][ROWW ? 1 : K][KC0];                      // the filter, once per lane (the same for all of them: LDS broadcasts)
    if (!ROWW) {
#pragma unroll
        for (int c1 = 0; c1 < C1; c1++)
#pragma unroll
            for (int ky = 0; ky < K; ky++)
#pragma unroll
                for (int j = 0; j < KC0; j++) wv[c1][ky][j] = Wf[(c1 * K + ky) * KC0 + j];
    }
    for (int pix = threadIdx.x - T0; pix < nrows * W; pix += TN) {
        const int y = pix / W, x = pix - y * W;
        float acc[C1];
#pragma unroll
        for (int c1 = 0; c1 < C1; c1++) acc[c1] = 0.f;
#pragma unroll
        for (int ky = 0; ky < K; ky++) {
            const float *d = dOw + (y + ky) * RSO + x * C0;
            if (ROWW) {
#pragma unroll
                for (int c1 = 0; c1 < C1; c1++)
#pragma unroll
                    for (int j = 0; j < KC0; j++) wv[c1][0][j] = Wf[(c1 * K + ky) * KC0 + j];
            }
            float dv[KC0];
            if (PAIR) {
#pragma unroll
                for (int j = 0; j < KC0; j += 2) { const float2 t = *reinterpret_cast<const float2 *>(d + j); dv[j] = t.x; dv[j + 1] = t.y; }
            } else {
#pragma unroll
                for (int j = 0; j < KC0; j++) dv[j] = d[j];
            }
#pragma unroll
            for (int j = 0; j < KC0; j++)
#pragma unroll
                for (int c1 = 0; c1 < C1; c1++) acc[c1] = fmaf(wv[c1][ROWW ? 0 : ky][j], dv[j], acc[c1]);
        }
#pragma unroll
        for (int c1 = 0; c1 < C1; c1++) dXb[pix * C1 + c1] = acc[c1];
    }
}

template <int S>
__device__ __forceinline__ void stage_bwd(const BwdArgs &p, float *L, int img, const float *dY, bool dy_global) {
    if constexpr (S >= 0) {
        const BwdStage &g = p.st[S];
        constexpr int H = SH[S].H, W = SH[S].W, C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K, PD = K / 2, nX = H * W * C1, RSX = RSXw(S);
        float *dOw = L + do_off(), *Xw = L + xw_off(), *dXb = L + dx_off(S & 1);
        // the conv input's forward values, in flight while the run backward works
        constexpr int NXQ = (nX + CS_THREADS - 1) / CS_THREADS;
        float vx[NXQ];
        const float *xg = g.X + (long)img * nX;
#pragma unroll
        for (int q = 0; q < NXQ; q++) { const int e = threadIdx.x + q * CS_THREADS; vx[q] = e < nX ? xg[e] : 0.f; }
        // zero the two windows (their borders must be zero; the interiors are rewritten below)
        for (int e = threadIdx.x * 4; e < do_size() + xw_size(); e += CS_THREADS * 4) *reinterpret_cast<float4 *>(dOw + e) = make_float4(0.f, 0.f, 0.f, 0.f);
        lds_barrier();
        CS_STAMP(1 + 8 * S);
        run_bwd<S, false>(g, dY, dy_global, dOw, img);
        CS_STAMP(2 + 8 * S);
#pragma unroll
        for (int q = 0; q < NXQ; q++) {
            const int e = threadIdx.x + q * CS_THREADS;
            if (e < nX) { const int y = e / (W * C1), r = e - y * (W * C1); Xw[(y + PD) * RSX + PD * C1 + r] = vx[q]; }
        }
        lds_barrier();
        CS_STAMP(3 + 8 * S);
        if (p.train & 1) df_partial<S, SH[S].H>(Xw, dOw, L + slot_off(), p.part + (long)img * part_row() + part_off(S), p.prof);
        CS_STAMP(4 + 8 * S);
        if constexpr (C1 <= 4 && nF(S) <= 160) dx_valu<S>(dOw, L + wb_off(S), dXb);
        else conv_mfma<W, C0, C1, K, JPb(S), NTb(S), NCb(S), conv_mt(H, W), RSOw(S)>(dOw, L + wb_off(S), nullptr, dXb, H);
        CS_STAMP(5 + 8 * S);
        lds_barrier();
        CS_STAMP(6 + 8 * S);
        {   // dX: the conv input tensor (`in = dx`, backprop.cu:185) and its scratch copy
            float *x = g.X + (long)img * nX, *x2 = g.DXS ? g.DXS + (long)img * nX : nullptr;
            if ((nX & 3) == 0) {
                for (int e = threadIdx.x * 4; e < nX; e += CS_THREADS * 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(dXb + e);
                    *reinterpret_cast<float4 *>(x + e) = v; if (x2) *reinterpret_cast<float4 *>(x2 + e) = v;
                }
            } else for (int e = threadIdx.x; e < nX; e += CS_THREADS) { const float v = dXb[e]; x[e] = v; if (x2) x2[e] = v; }
        }
        CS_STAMP(7 + 8 * S);
        stage_bwd<S - 1>(p, L, img, dXb, false);
    }
}

extern "C" __global__ void __launch_bounds__(CS_THREADS) cs_bwd(const BwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    const int img = blockIdx.x;
    CS_STAMP(0);
    float vf[CS_NS][8];
    load_filter_b<0>(p, vf);
    for (int e = threadIdx.x * 4; e < do_off(); e += CS_THREADS * 4) *reinterpret_cast<float4 *>(L + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    lds_barrier();
    put_filter_b<0>(L, vf);
    stage_bwd<CS_NS - 1>(p, L, img, p.DY, true);
}

// ======================================================================================================== backward, banded
// CS_BSPLIT workgroups per image.  Possible only because the FORWARD saved what a band would otherwise have to read from a buffer
// its neighbour overwrites in place (the reference's `in = dx` convention): a copy of every conv input (for the dF halo rows) and the
// pool arg-max codes (instead of the forward values in the pool's input buffer).  Everything a band reads is then read-only, and it
// stores only the rows it owns.  Halo rows of dO / dX are recomputed, never exchanged - the windows GROW towards the last stage:
//   bx(0) = the band's own input rows;  dO rows needed  bo(s) = bx(s) +- P;  pooled rows  bq(s) = cover(bo(s));  bx(s+1) = bq(s)
constexpr int bpo_lo(int s, int b) { return (H0(s) * b + CS_BSPLIT - 1) / CS_BSPLIT; }            // pooled rows a band owns (stores)
constexpr int bpo_hi(int s, int b) { return (H0(s) * (b + 1) + CS_BSPLIT - 1) / CS_BSPLIT; }
constexpr int bq_lo(int s, int b);
constexpr int bq_hi(int s, int b);
constexpr int bx_lo(int s, int b) { return s == 0 ? bpo_lo(0, b) * SH[0].KS : bq_lo(s - 1 >= 0 ? s - 1 : 0, b); }   // dX rows computed (input grid of stage s)
constexpr int bx_hi(int s, int b) { return s == 0 ? bpo_hi(0, b) * SH[0].KS : bq_hi(s - 1 >= 0 ? s - 1 : 0, b); }
constexpr int bq_lo(int s, int b) { return cmax(bx_lo(s, b) - SH[s].K / 2, 0) / SH[s].KS; }                         // pooled rows whose run backward is computed
constexpr int bq_hi(int s, int b) { return (cmin(bx_hi(s, b) + SH[s].K / 2, SH[s].H) + SH[s].KS - 1) / SH[s].KS; }
constexpr int oi_lo(int s, int b) { return s == 0 ? bpo_lo(0, b) * SH[0].KS : bpo_lo(s - 1 >= 0 ? s - 1 : 0, b); }  // input rows of stage s a band owns
constexpr int oi_hi(int s, int b) { return s == 0 ? bpo_hi(0, b) * SH[0].KS : bpo_hi(s - 1 >= 0 ? s - 1 : 0, b); }
constexpr int bmax_q(int s) { int m = 0; for (int b = 0; b < CS_BSPLIT; b++) m = cmax(m, bq_hi(s, b) - bq_lo(s, b)); return m; }
constexpr int bmax_o(int s) { int m = 0; for (int b = 0; b < CS_BSPLIT; b++) m = cmax(m, bpo_hi(s, b) - bpo_lo(s, b)); return m; }
constexpr int bmax_x(int s) { int m = 0; for (int b = 0; b < CS_BSPLIT; b++) m = cmax(m, bx_hi(s, b) - bx_lo(s, b)); return m; }
// LDS plan: dX-conv filters (as unbanded), then windows sized by the largest band
constexpr int bdo_size() { int m = 0; for (int s = 0; s < CS_NS; s++) m = cmax(m, (bmax_q(s) * SH[s].KS + SH[s].K - 1) * RSOw(s) + 16); return pad4(m); }
constexpr int bxw_size() { int m = 0; for (int s = 0; s < CS_NS; s++) m = cmax(m, (bmax_o(s) * SH[s].KS + SH[s].K - 1) * RSXw(s) + 16); return pad4(m); }
constexpr int bdx_size() { int m = 0; for (int s = 0; s < CS_NS; s++) m = cmax(m, bmax_x(s) * SH[s].W * SH[s].C1); return pad4(m); }
constexpr int bdo_off() { return wb_off(CS_NS - 1) + wb_size(CS_NS - 1); }
constexpr int bxw_off() { return bdo_off() + bdo_size(); }
constexpr int bdx_off(int which) { return bxw_off() + bxw_size() + which * bdx_size(); }
constexpr int bslot_off() { return bdx_off(2); }
constexpr int bwdb_lds_floats() { return bslot_off() + slot_size(); }

// The workgroup has CS_BWAVES = 16 waves.  The phases whose loops stride by the thread count (window zero fill, run backward, X-window fill, filter
// staging, the store phase) run on all of them.  The MIDDLE phase of a stage is two independent latency chains - the dF items (LDS round trip -> MFMA burst per
// item) and the stage's dX (which alone feeds the next stage) - and runs them side by side: waves 0 .. 7 take the dF items exactly as the 8 waves of cs_bwd
// do (item = wave, wave + 8, ...: same slots, same sums), waves 8 .. 15 the dX.  Lab stamps (thread 0 unless noted), per stage S: 1 + 8 S windows zeroed,
// 2 + 8 S run backward done, 3 + 8 S roles begin, 4 + 8 S dF items done, 5 + 8 S past the shared barrier, 6 + 8 S fold done, 7 + 8 S dX copied out;
// from the first lane of wave 8: 24 + 2 S dX role begins, 25 + 2 S dX role done.
template <int S>
__device__ __forceinline__ void stage_bwd_b(const BwdArgs &p, float *L, int img, int band, const float *dY, bool dy_global, const float (&vf)[CS_NS][4]) {
    if constexpr (S >= 0) {
        const BwdStage &g = p.st[S];
        constexpr int H = SH[S].H, W = SH[S].W, C1 = SH[S].C1, C0 = SH[S].C0, K = SH[S].K, KS = SH[S].KS, PD = K / 2;
        constexpr int RSX = RSXw(S), RSO = RSOw(S), rowX = W * C1;
        const int ql = bq_lo(S, band), qh = bq_hi(S, band), pol = bpo_lo(S, band), poh = bpo_hi(S, band);
        const int xl = bx_lo(S, band), xh = bx_hi(S, band), il = oi_lo(S, band), ih = oi_hi(S, band);
        const int dq0 = ql * KS, ol = pol * KS, oh = poh * KS;                  // first conv row of the dO window; own conv rows (dF)
        float *dOw = L + bdo_off(), *Xw = L + bxw_off(), *dXb = L + bdx_off(S & 1);
        // the conv input's forward values for the dF rows (own conv rows +- P), from the forward's copy; in flight under the run backward
        const int xr_lo = max(ol - PD, 0), xr_hi = min(oh + PD, H), nxw = (xr_hi - xr_lo) * rowX;
        constexpr int NXQ = ((bmax_o(S) * KS + K - 1) * rowX + CS_BTHREADS - 1) / CS_BTHREADS;
        float vx[NXQ];
        const float *xg = g.save_x + ((long)img * H + xr_lo) * rowX;
#pragma unroll
        for (int q = 0; q < NXQ; q++) { const int e = threadIdx.x + q * CS_BTHREADS; vx[q] = e < nxw ? xg[e] : 0.f; }
        if (!(LAB_SKIP & 16)) for (int e = threadIdx.x * 4; e < bdo_size() + bxw_size(); e += CS_BTHREADS * 4) *reinterpret_cast<float4 *>(dOw + e) = make_float4(0.f, 0.f, 0.f, 0.f);
        lds_barrier();
        CS_STAMP(1 + 8 * S);
        if (!(LAB_SKIP & 4)) run_bwd<S, true, CS_BTHREADS, ST_BWD>(g, dY, dy_global, dOw, img, ql, qh, pol, poh);
        CS_STAMP(2 + 8 * S);
        // round 6: the dX-conv filters (requested in the kernel's first instructions) go to LDS HERE, behind the last stage's run backward: the first
        // consumer is that stage's dX convolution one barrier further on, and placed at the kernel's start the wait for them was a round trip of its own in
        // front of the run backward's loads (cs_lab: "setup" 2.7 k cycles)
        if constexpr (S == CS_NS - 1) put_filter_b<0, CS_BTHREADS>(L, vf);
#pragma unroll
        for (int q = 0; q < NXQ; q++) {
            const int e = threadIdx.x + q * CS_BTHREADS;
            if (e < nxw && !(LAB_SKIP & 8)) { const int y = e / rowX, r = e - y * rowX; Xw[(y + xr_lo - (ol - PD)) * RSX + PD * C1 + r] = vx[q]; }
        }
        lds_barrier();
        // ---- the two roles.  Both only READ the windows (the dF role Xw and dOw, the dX role dOw and the filter) and they WRITE disjoint regions - the slots
        // and the dX buffer - so neither needs anything from the other and ONE barrier behind both orders everything the store phase and the next stage read.
        // No branch below contains a barrier: a role with nothing to do (no parameter gradients, the first layer's dX left to t4k_conv_stack_dx0, a lab skip)
        // falls through to the barrier every wave executes.
        const bool grads = (p.train & 1) && !(LAB_SKIP & 1), lazy0 = S == 0 && (p.train & 2);
        float *slots = L + bslot_off();
        if (threadIdx.x < CS_THREADS) {
            CS_STAMP(3 + 8 * S);
            if (grads) df_items<S, bmax_o(S) * KS>(Xw, dOw + (ol - dq0) * RSO, slots, p.prof, oh - ol);
            CS_STAMP(4 + 8 * S);
        } else {
            CS_STAMP_X(24 + 2 * S);
            if (!lazy0 && !(LAB_SKIP & 2)) {
                if constexpr (C1 <= 4 && nF(S) <= 160) dx_valu<S, CS_THREADS, CS_THREADS, (nF(S) > 64)>(dOw + (xl - dq0) * RSO, L + wb_off(S), dXb, xh - xl);
                else conv_mfma<W, C0, C1, K, JPb(S), NTb(S), NCb(S), conv_mt(bmax_x(S), W), RSOw(S), CS_WAVES, CS_WAVES, conv_pipe_fits(JPb(S), NTb(S), conv_mt(bmax_x(S), W), CS_WAVES)>(dOw + (xl - dq0) * RSO, L + wb_off(S), nullptr, dXb, xh - xl);
            }
            CS_STAMP_X(25 + 2 * S);
        }
        lds_barrier();
        CS_STAMP(5 + 8 * S);
        // ---- one store phase on all 16 waves: the fold of the slots into this workgroup's partial row (every sum in its fixed order), then the dX copy-out
        if (grads) df_fold<S, CS_BTHREADS>(slots, p.part + ((long)img * CS_BSPLIT + band) * part_row() + part_off(S), p.prof);
        CS_STAMP(6 + 8 * S);
        if (lazy0) return;                                       // lazy dX of the first layer (see BwdArgs)
        if (!(LAB_SKIP & 32)) {   // dX, own input rows: the conv input tensor (`in = dx`) and its scratch copy
            const int n = (ih - il) * rowX;
            const float *src = dXb + (il - xl) * rowX;
            float *x = g.X + ((long)img * H + il) * rowX, *x2 = g.DXS ? g.DXS + ((long)img * H + il) * rowX : nullptr;
            constexpr int POL = S == 0 ? ST_PLAIN : ST_BWD;       // stage 0's dX belongs to the layer in front of the stack
            if ((rowX & 3) == 0) {
                for (int e = threadIdx.x * 4; e < n; e += CS_BTHREADS * 4) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + e);
                    gstore4<POL>(x + e, v); if (x2) gstore4<POL>(x2 + e, v);
                }
            } else for (int e = threadIdx.x; e < n; e += CS_BTHREADS) { const float v = src[e]; gstore1<POL>(x + e, v); if (x2) gstore1<POL>(x2 + e, v); }
        }
        CS_STAMP(7 + 8 * S);
        stage_bwd_b<S - 1>(p, L, img, band, dXb, false, vf);
    }
}

extern "C" __global__ void __launch_bounds__(CS_BTHREADS) cs_bwd_b(const BwdArgs p) {
    extern __shared__ __attribute__((aligned(16))) float L[];
    const int img = blockIdx.x, band = blockIdx.y;
    CS_STAMP(0);
    float vf[CS_NS][4];
    load_filter_b<0, CS_BTHREADS>(p, vf);
    for (int e = threadIdx.x * 4; e < bdo_off(); e += CS_BTHREADS * 4) *reinterpret_cast<float4 *>(L + e) = make_float4(0.f, 0.f, 0.f, 0.f);
    stage_bwd_b<CS_NS - 1>(p, L, img, band, p.DY, true, vf);     // (the zeroed filter region is fenced by the stage's first barrier; the filters follow its run backward)
    if (p.f0_save && img == 0 && band == 0) {                    // the filter the skipped dX of stage 0 belongs to (the optimizer changes F before anyone asks)
#pragma unroll
        for (int q = 0; q < (nF(0) + CS_BTHREADS - 1) / CS_BTHREADS; q++) { const int e = threadIdx.x + q * CS_BTHREADS; if (e < nF(0)) p.f0_save[e] = vf[0][q]; }
    }
}
#endif // CS_ONLY_FWD
