// gemm_head_bwd.h - k_head_bwd_l32: the classifier head's backward and the backward of the linear layer in front of it in one launch
// (launched by linear.hip, head_bwd_launch).  Its tiles follow gemm_s32_body (gemm_l32.h); what it knows about is softmax targets and mask chains.
#pragma once
#include "gemm_types.h"

namespace {

// ---- classifier-head backward + the backward of the linear layer in front of it, ONE launch (t4k_mlp_head_bwd).
// The head backward (loss preparation out -= target, dW2 | dB2, dX2 = dY2 W2 in place, mask multiply -> dY1) and the big layer's dW1 += dY1^T X1,
// dX1 = dY1 W1 are dependent: the second needs dY1 [N][EA].  But dY1 is CHEAP to recompute - dY1[n, e] = mask[n, e] sum_j (P - T)[n, j] W2[j, e], EB <= 16
// terms - so every GEMM tile prepares the 32 rows / columns of dY1 it multiplies with in LDS from P, T, W2 and the mask (all there before the launch) and
// nothing waits for the head: GEMM tiles and the column-sliced head workgroups (k_linsmall_bwd_cols's body as riders) run side by side.  The riders store
// dY1, dX2, dW2, dB2 and dB1 (the column sums of the dY1 slice they have in hand).  The only shared write is `out -= target` over P: a rider of its own
// stores it once EVERY workgroup has its P and T values in registers (counter; off everybody's critical path).
// Round 6 (k_head_bwd_l32): round 3's form of this launch (16.2 us) lost to two launches (7.0 + 6.0 us) because its tiles made three dependent memory round
// trips in front of the GEMM and gathered the B operand row by row.  Here a tile workgroup
//   1. issues the LDS-DMA of its B blocks (X1 or W1: 32 k x 32 columns per block, whole 128-byte runs, wave-private slots as gemm_s32_body<.., DMA>),
//   2. requests P, T, W2 and the mask values it needs STRAIGHT INTO REGISTERS in MFMA operand layout - the same round trip as the DMA -
//   3. multiplies (P - T) W2 on the matrix cores (ceil(EB / 2) v_mfma_f32_32x32x2_f32 per 32 x 32 block of dY1), applies the mask and leaves the block in LDS
//      k-major with a pitch of 33 floats (conflict-free for the writes of either tile kind and for the fragment reads),
//   4. one barrier, then the K loop proper: B fragments from the wave's DMA slots, A fragments from the dY1 tile, k-groups meet in LDS, epilogue as
//      gemm_s32_body's (in-place dX1 behind the epoch-tagged arrival slots of the dW1 readers).
// The tiles' dY1 comes from an MFMA sum, the riders' stored dY1 from the oracle's fmaf chain: the two differ by rounding only (1e-7 relative to the
// largest term), far inside the 1e-4 bar of dW1 / dX1; every tensor the reference materialises is the riders' (P, Y2, dX2, dY1 and, from EB = 5, dW2 bit-equal to the two-launch path;
// dB2 and dB1 add row groups where that path adds sample by sample).
struct HeadBwd {
    const float *P, *T, *W2, *MASK;     // softmax output [N][EB], target, W2 [EB][EA], derivative mask of the layer between the linear layers [N][EA]
    float *X2, *DW2, *DB2, *Y1, *Y2;    // head input [N][EA] (receives dX2), gradients, dY1 tensor (= dX2 * mask), second copy of out - target
    float *DB1;
    int N, EA, EB, train, nwg; int *sync;
    const float *MSKB; float *Y1B;     // a second mask layer between the linear layers (`leakyrelu dropout`): dY1 = dX2 * MASK * MSKB, Y1 keeps the first product, Y1B the second
    MaskChain mc1;                      // mask multiplies behind the big layer's dX1 (the run in front of it), as linear_bwd_dual
    const float *Z;                     // 4 KiB of zeros: source of DMA lanes past the K range / the matrix edge (the operand loads are range-checked buffer loads and need none)
#ifdef T4K_LAB
    int lab;                            // LAB build only: timing ablations (wrong results; bit 128, the other order of the roles, right ones), the bits of T4K_HB_LAB, read at run time
    unsigned long long *prof;           // LAB build only: role stamps, HB_PROF_WORDS per workgroup (T4K_HB_PROF_PTR, tools/experiments/head_bwd_lab.py); nullptr: none
#endif
};
// ---- role stamps (LAB build only; the release build compiles every HB_* macro below to nothing).  Wave 0 of a workgroup reads the shader clock at the
// links of its role's chain and KEEPS the readings in scalar registers; thread 0 stores them once, behind the role's last store, so no stamp adds a
// memory operation or a wait to the chain it measures.  Words of a workgroup's record: [0, 14) s_memtime at the role's links (see the HB_STAMP calls),
// 14 | 15 the 100 MHz clock (one for all XCDs) at the start | end, 16 spins of the role's wait, 17 role (0 dW1 tile, 1 dX1 tile, 2 store rider, 3 column
// rider), 18 HW_ID, 19 XCC_ID.
#ifdef T4K_LAB
constexpr int HB_PROF_WORDS = 32;
__device__ __forceinline__ unsigned long long hb_clock() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
__device__ __forceinline__ unsigned long long hb_wallclock() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define HB_STAMP(k) do { if (hb.prof) hb_ts[k] = hb_clock(); } while (0)
#define HB_WALL(k) do { if (hb.prof) hb_ts[k] = hb_wallclock(); } while (0)
#define HB_LABX(...) __VA_ARGS__
// behind the role's last store: wait for the stores (word n - 1 is `drained`), then thread 0 writes the record
#define HB_FLUSH(n, role) do { if (hb.prof) { \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); hb_ts[(n) - 1] = hb_clock(); hb_ts[15] = hb_wallclock(); \
        if (tid == 0) { \
            unsigned long long *rec_ = hb.prof + (long)bx * HB_PROF_WORDS; \
            _Pragma("unroll") for (int k_ = 0; k_ < 16; k_++) if (k_ < (n) || k_ >= 14) rec_[k_] = hb_ts[k_]; \
            rec_[16] = (unsigned long long)hb_spins; rec_[17] = (role); \
            rec_[18] = __builtin_amdgcn_s_getreg(4 | (31 << 11)); rec_[19] = __builtin_amdgcn_s_getreg(20 | (31 << 11)); \
        } } } while (0)
#else
#define HB_STAMP(k) do {} while (0)
#define HB_WALL(k) do {} while (0)
#define HB_LABX(...)
#define HB_FLUSH(n, role) do {} while (0)
#endif
constexpr int HB_CW = 4;                // columns of the head's input per rider workgroup (k_linsmall_bwd_cols: LSC_CW)
constexpr int HB_AP = 33;               // pitch of the dY1 tile in LDS
// workgroups [0, a1): dW1 tiles (read X1, never wait) | [a1, nwg - nr): dX1 tiles (write X1 in place, wait for the dW1 tiles of their column only) | the last
// nr: riders - the store rider, then the column riders.  (T4K_HB_RIDERS_LAST 0, the order up to round 10: the riders between the two tile kinds; the LAB
// build's bit 128 takes the other order at run time.)  Correctness does not depend on the order: admission keeps every workgroup resident, the gate reads
// tagged slots, pslots is indexed by workgroup.  slots == nullptr: a frozen layer (a1 == 0) - nothing to wait for.
#ifndef T4K_HB_RIDERS_LAST
#define T4K_HB_RIDERS_LAST 1
#endif
__global__ void __launch_bounds__(256) k_head_bwd_l32(GemmP p1, GemmP p2, int a1, int nr, unsigned *slots, unsigned *pslots, unsigned epoch, HeadBwd hb) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    typedef __attribute__((address_space(3))) const float lds_f;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), h = lane >> 5, l31 = lane & 31;
    const int N = hb.N, EA = hb.EA, EB = hb.EB, bx = blockIdx.x;
#ifdef T4K_LAB
    const int lab = hb.lab;
#else
    constexpr int lab = 0;              // release build: every HB_LAB branch below folds away
#endif
    const auto HB_LAB = [=](int bit) { return (lab & bit) != 0; };
    HB_LABX(unsigned long long hb_ts[16] = {}; int hb_spins = 0;)
    HB_WALL(14); HB_STAMP(0);
    // the roles over blockIdx.x, a pure function of bx: the workgroups dispatched last are the ones that double up on a CU (274 on 256 at the flagship shape)
    const bool riders_last = (T4K_HB_RIDERS_LAST != 0) != HB_LAB(128);
    const int r0 = riders_last ? hb.nwg - nr : a1;                   // the store rider; the column riders behind it
    const bool first = bx < a1, is_tile = first || (riders_last ? bx < r0 : bx >= a1 + nr);
    if (is_tile) {
        // ---------------------------------------------------------------- GEMM tile
        if (HB_LAB(2)) return;
        const int tile = first ? bx : bx - (riders_last ? a1 : a1 + nr), tiles_n = p1.tiles_n;        // both GEMMs have the same column tiling (E1)
        const int tm = tile / tiles_n, tn = tile - tm * tiles_n, m0 = tm * 32, n0 = tn * 32;
        const int M = first ? EA : N, Nn = p2.N, K = first ? N : EA;   // dW1: M = EA, K = N;  dX1: M = N, K = EA;  both: B = [K][Nn] rows (X1 / W1)
        const float *pB = first ? p1.B : p2.B;
        float *pO = first ? p1.O : p2.O;
        const int nblk = (K + 31) >> 5;
        const int b0 = w * nblk / 4, nb = (w + 1) * nblk / 4 - b0;   // this wave's k blocks (nblk <= 8: at most two, both requested up front)
        float *Bs = lds + w * 2048, *Ad = lds + 8192;                // wave-private B slots (2 x 4 KiB; the wave's partial accumulators afterwards) | dY1 tile [nblk * 32][33]
        {   // 1. B blocks by LDS-DMA
            const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)Bs;
            const int i8 = lane >> 3, i7 = lane & 7;
            const bool bcol = n0 + 4 * i7 < Nn;
            const float *zsrc = hb.Z + 4 * i7;
#pragma unroll
            for (int s = 0; s < 2; s++) {
                if (s < nb) {
                    const int k0 = 32 * (b0 + s);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int r = 8 * j + i8;
                        const float *sb = (k0 + r < K && bcol) ? pB + (long)(k0 + r) * Nn + n0 + 4 * i7 : zsrc;
                        const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((s * 1024 + j * 256) * 4));
                        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(sb), "s"(la) : "memory");
                    }
                }
            }
        }
        // Operand loads (round 11): range-checked buffer loads.  Round 10 made them straight-line code by letting every bound pick the ADDRESS (the element,
        // or a word of the zero strip hb.Z); the selects and the 64-bit address arithmetic of that form were ~1 300 instructions per wave in front of the
        // first MFMA (profiles/LAB_NOTES.md 16, 17).  Here a tensor is a buffer descriptor of its logical size, built from kernel arguments and blockIdx-derived
        // scalars only, and a lane keeps ONE 32-bit byte offset per operand family: what lies past the tensor's END reads 0.0f from the hardware's range check,
        // and every bound that is not the tensor's end (a column bound inside a row, a block past nblk, an ablation) turns the lane's offset into HB_OOR once
        // per family.  The range check covers the lane's offset and the instruction's immediate, NOT the scalar offset (tools/experiments/buf_lds_probe.hip),
        // so the run-time row strides go into the lane's offset (one v_add per request) and the scalar offset stays 0.  No load is skipped: the requests of a
        // block go out together and the first MFMA waits for them once (`ok ? P[i] - T[i] : 0.f` with the load inside the branch made one round trip per pair).
        // HB_OOR: the lane offsets are unsigned.  Under head_bwd_ok's limits (N, EA <= 256, EB <= 16, at most 768 workgroups, so E1 is a few thousand) the largest
        // descriptor is N E1 4 or EA E1 4 bytes, a few MiB, and what is added to a lane's offset is at most 3 erow, 15 mrow, 14 mrow or 56 bytes: 2^31 + that neither
        // falls inside a descriptor nor wraps.  The bound rests on those admission limits - widen them and revisit it.
        constexpr unsigned HB_OOR = 0x80000000u;
        const auto hb_srd = [](const float *base, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, (int)(base ? bytes : 0u), 0x00020000); };   // (a null base: 0 bytes, every lane reads 0.0f)
        const auto hb_ld = [](__amdgpu_buffer_rsrc_t rs, unsigned vo) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, 0, 0)); };
        // epilogue operands, requested with everything else: what dW1 accumulates onto | the first mask behind dX1, and the second mask
        const int gn = n0 + l31;
        const float *const e1p = first ? pO : hb.mc1.d1 ? hb.mc1.m1 : nullptr, *const e2p = (!first && hb.mc1.d2) ? hb.mc1.m2 : nullptr;
        float e1[4], e2[4];
        {
            const unsigned ebytes = (unsigned)M * (unsigned)Nn * 4u, erow = (unsigned)Nn * 4u;       // [EA][E1] (dW1's accumuland) | [N][E1] (the masks behind dX1): a row gm >= M lies past the end
            const auto r1 = hb_srd(e1p, ebytes), r2 = hb_srd(e2p, ebytes);
            const unsigned evo = gn < Nn ? ((unsigned)(m0 + 8 * w + 4 * h) * (unsigned)Nn + (unsigned)gn) * 4u : HB_OOR;   // row gm = m0 + q + 8 w + 4 h of the epilogue below
#pragma unroll
            for (int q = 0; q < 4; q++) { e1[q] = hb_ld(r1, evo + q * erow); e2[q] = hb_ld(r2, evo + q * erow); }
        }
        // 2. operands of the dY1 blocks this wave prepares (blocks w and w + 4 of the tile's k range), in MFMA layout
        //    dW1 tile: block = 32 samples, the tile's 32 columns e of dY1;   dX1 tile: block = 32 columns e, the tile's 32 samples
        const unsigned mbytes = (unsigned)N * (unsigned)EA * 4u, mrow = (unsigned)EA * 4u;
        const auto rP = hb_srd(hb.P, (unsigned)N * (unsigned)EB * 4u), rT = hb_srd(hb.T, (unsigned)N * (unsigned)EB * 4u);
        const auto rW = hb_srd(hb.W2, (unsigned)EB * (unsigned)EA * 4u), rM = hb_srd(hb.MASK, mbytes);
        const int jl = EB - h;                                       // MFMA slot s of this lane is k index j = 2 s + h: a term of the sum while 2 s < jl
        float av[2][8], bv[2][8], mk[2][16];
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int s = 0; s < 8; s++) av[t][s] = bv[t][s] = 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) mk[t][r] = 0.f;
            if (t == 0 || nblk > 4) {                                // (no wave has a second block up to K = 128)
                const int blk = w + 4 * t;
                const int arow = first ? 32 * blk + l31 : m0 + l31;  // sample of this lane's A values (P - T): a dX1 tile's second block reads the first one's again
                const int bcl = first ? m0 + l31 : 32 * blk + l31;   // column e of this lane's B values (W2): a dW1 tile's likewise; the column of its mask values too
                const int mr0 = first ? 32 * blk : m0;               // first sample of the block's mask values
                const bool on = blk < nblk, lon = on && !HB_LAB(8);
                // P / T: [N][EB], the slots 8 s bytes apart in the immediate.  A slot j >= EB of a used s (odd EB, h == 1: the next row's first element, no
                // end of the tensor) is dropped from the VALUE below; W2 [EB][EA]: row j >= EB lies past the end
                const unsigned avo = lon && arow < N ? ((unsigned)arow * (unsigned)EB + (unsigned)h) * 4u : HB_OOR;
                const unsigned bvo = lon && bcl < EA ? ((unsigned)h * (unsigned)EA + (unsigned)bcl) * 4u : HB_OOR;
                // mask: [N][EA], value r of the accumulator layout is sample mr0 + (r & 3) + 8 (r >> 2) + 4 h: a sample >= N lies past the end
                const unsigned mvo = on && bcl < EA && !HB_LAB(64) ? ((unsigned)(mr0 + 4 * h) * (unsigned)EA + (unsigned)bcl) * 4u : HB_OOR;
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const float pv = hb_ld(rP, avo + 8u * s), tv = hb_ld(rT, avo + 8u * s);
                    av[t][s] = 2 * s < jl ? pv - tv : 0.f;
                    bv[t][s] = hb_ld(rW, bvo + 2u * s * mrow);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) mk[t][r] = hb_ld(rM, mvo + (unsigned)((r & 3) + 8 * (r >> 2)) * mrow);
            }
        }
        if (hb.MSKB) {                                               // a second mask layer: its values multiply the first one's, one more round trip
            const auto rMB = hb_srd(hb.MSKB, mbytes);
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int blk = w + 4 * t;
                if (blk < nblk) {
                    const int bcl = first ? m0 + l31 : 32 * blk + l31, mr0 = first ? 32 * blk : m0;
                    const unsigned mvo = bcl < EA ? ((unsigned)(mr0 + 4 * h) * (unsigned)EA + (unsigned)bcl) * 4u : HB_OOR;
                    float m2[16];
#pragma unroll
                    for (int r = 0; r < 16; r++) m2[r] = hb_ld(rMB, mvo + (unsigned)((r & 3) + 8 * (r >> 2)) * mrow);
#pragma unroll
                    for (int r = 0; r < 16; r++) mk[t][r] *= m2[r];
                }
            }
        }
        HB_STAMP(1);                                                 // B DMA and operand loads issued
        // 3. dY1 blocks on the matrix cores -> LDS
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int blk = w + 4 * t;
            if (blk < nblk) {
                f32x16 d;
#pragma unroll
                for (int r = 0; r < 16; r++) d[r] = 0.f;
#pragma unroll
                for (int s = 0; s < 8; s++) if (2 * s < EB) {
                    d = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][s], bv[t][s], d, 0, 0, 0);
                    if (t == 0 && s == 0) HB_STAMP(2);               // first dY1 MFMA issued: its operands have landed
                }
                // value r of the accumulator is row (r & 3) + 8 (r >> 2) + 4 h, column l31 of the block; a dW1 tile keeps it sample-major, a dX1 tile
                // column-major: one base and one stride (`first ? .. : ..` per element compiled to two scalar branches round every store)
                const int abase = first ? (32 * blk + 4 * h) * HB_AP + l31 : (32 * blk + l31) * HB_AP + 4 * h, astep = first ? HB_AP : 1;
#pragma unroll
                for (int r = 0; r < 16; r++) Ad[abase + ((r & 3) + 8 * (r >> 2)) * astep] = d[r] * mk[t][r];
            }
        }
        HB_STAMP(3);                                                 // dY1 blocks in LDS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the wave's DMA blocks have landed (they were requested first)
        __builtin_amdgcn_s_waitcnt(0x0F70);                          // the same wait once more, in the form the compiler's own count of requests in flight sees (it is blind
                                                                     // to the statement above, and waited for the dW1 tag store below before it reused a register)
        HB_STAMP(4);
        const bool early = slots && a1 <= 128;                       // per-wave arrival slots: X1 is consumed as far as this wave is concerned
        if (first && early && lane == 0) __hip_atomic_store(slots + 4 * tile + w, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // in-place dX1: the first look at the arrival slots of this column's dW1 tiles goes out here, as soon as a request no longer lengthens the wait for the
        // DMA blocks - its round trip passes under barrier 1 and the K loop (the look only reads tags; the stores at the end are what waits for them)
        const int gsh = early ? 2 : 0, gper = 1 << gsh, gslot = (a1 / tiles_n) * gper;   // (slots per dW1 tile: a shift, the look sits in front of barrier 1)
        const bool gated = !first && slots && w == 0 && !HB_LAB(32);
        unsigned gv[8];                                              // the tags as they come back, compared only where the verdict is needed: a comparison beside the
#pragma unroll                                                       // request waits for it there (the parent's look sat behind barrier 1 with its wait: a round trip in
        for (int u = 0; u < 8; u++) gv[u] = epoch;                   // front of the K loop, not under it)
        const auto gate_look = [&]() {
#pragma unroll
            for (int u = 0; u < 8; u++) {                            // a1 <= 512 slots
                const int i = lane + 64 * u;
                if (i < gslot) { const int e0t = i >> gsh, ww = i - e0t * gper; gv[u] = __hip_atomic_load(slots + gper * (e0t * tiles_n + tn) + ww, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            }
        };
        const auto gate_open = [&]() {
            unsigned bad = 0;
#pragma unroll
            for (int u = 0; u < 8; u++) bad |= gv[u] ^ epoch;
            return __all(bad == 0);
        };
        if (gated) gate_look();
        // barrier 1: the dY1 tile is in LDS.  Not __syncthreads(): its fence would wait for the look (and for a dW1 tile's tag store) to come back
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        HB_STAMP(5);                                                 // past barrier 1
        if (tid == 0 && !HB_LAB(4)) __hip_atomic_store(pslots + bx, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // P and T are in registers everywhere: `out -= target` may land as far as this workgroup is concerned
        if (HB_LAB(16)) return;
        if (first && slots && !early && tid == 0) __hip_atomic_store(slots + tile, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // 4. K loop
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (s < nb) {
                lds_f *b = (lds_f *)Bs + s * 1024, *a = (lds_f *)Ad + 32 * (b0 + s) * HB_AP;
                float fa[4][4], fb[4][4];
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int j = 0; j < 4; j++) { fa[c][j] = a[(8 * c + 4 * h + j) * HB_AP + l31]; fb[c][j] = b[(8 * c + 4 * h + j) * 32 + l31]; }
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0], fb[c][0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1], fb[c][1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][2], fb[c][2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][3], fb[c][3], acc1, 0, 0, 0);
                }
            }
        }
        HB_STAMP(6);                                                 // K loop: every MFMA issued
        if (gated && !gate_open()) { HB_LABX(hb_spins = 1;) gate_look(); }     // the first look came too early: the second one's round trip passes under the MFMAs' drain and the meeting
        // the four k-groups meet in LDS (each wave's partial sums over its own, consumed, B slots)
#pragma unroll
        for (int r = 0; r < 16; r++) Bs[r * 64 + lane] = acc0[r] + acc1[r];
        HB_STAMP(7);                                                 // meeting written
        if (gated && !gate_open()) {                                 // the dW1 tiles of this column have consumed X1 (see gemm_s32_body gate_mode 2)
            HB_LABX(hb_spins++;)                                     // (looks that failed, the first two included)
            for (int spin_it = 0;; spin_it++) {
                if (spin_it > T4K_SPIN_MAX) { if (lane == 0 && g_spin_err_dev) __hip_atomic_store(g_spin_err_dev, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                unsigned bad = 0;
#pragma unroll 4
                for (int i = lane; i < gslot; i += 64) {
                    const int e0t = i / gper, ww = i - e0t * gper;
                    bad |= __hip_atomic_load(slots + gper * (e0t * tiles_n + tn) + ww, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ epoch;
                }
                if (__all(bad == 0)) break;
                HB_LABX(hb_spins++;)
                __builtin_amdgcn_s_sleep(2);
            }
        }
        HB_STAMP(8);                                                 // gate passed
        __syncthreads();
        HB_STAMP(9);                                                 // past barrier 2
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r = 4 * w + q, gm = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float v = lds[r * 64 + lane];
#pragma unroll
            for (int g = 1; g < 4; g++) v += lds[g * 2048 + r * 64 + lane];       // k-groups in order
            if (gm < M && gn < Nn) {
                const long z = (long)gm * Nn + gn;
                if (first) pO[z] = v + e1[q];                                  // dW1 accumulates (beta = 1)
                else {
                    pO[z] = v;
                    if (hb.mc1.d1) { const float g1 = v * e1[q]; hb.mc1.d1[z] = g1; if (hb.mc1.d2) hb.mc1.d2[z] = g1 * e2[q]; }
                }
            }
        }
        HB_STAMP(10);                                                // stores issued
        HB_FLUSH(12, first ? 0 : 1);
        return;
    }
    if (bx == r0) {
        // ---------------------------------------------------------------- store rider: `out -= target` in place (+ its copy), once every other workgroup holds P and T
        const int tot = N * EB;
        for (int i = tid; i < tot; i += 256) lds[i] = hb.P[i] - hb.T[i];
        HB_STAMP(1);                                                 // P - T in LDS
        if (w == 0 && !HB_LAB(4 | 1 | 2 | 16)) {         // (ablations that drop arrivals must drop the wait too)
            // every other workgroup tags its slot once its P / T values sit in registers / LDS: plain stores to separate words (an arrival COUNTER serialised
            // 270 agent-scope atomics on one address: +1.2 us on the launch), polled here with the 64 lanes' loads in flight together
            for (int spin_it = 0;; spin_it++) {
                if (spin_it > T4K_SPIN_MAX) { if (lane == 0 && g_spin_err_dev) __hip_atomic_store(g_spin_err_dev, 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                unsigned bad = 0;
#pragma unroll 4
                for (int i = lane; i < hb.nwg; i += 64) if (i != bx) bad |= __hip_atomic_load(pslots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ epoch;
                if (__all(bad == 0)) break;
                HB_LABX(hb_spins++;)
                __builtin_amdgcn_s_sleep(2);
            }
        }
        HB_STAMP(2);                                                 // poll passed
        __syncthreads();
        float *Pw = const_cast<float *>(hb.P);
        for (int i = tid; i < tot; i += 256) { const float v = lds[i]; Pw[i] = v; if (hb.Y2) hb.Y2[i] = v; }
        HB_STAMP(3);                                                 // stored
        HB_FLUSH(5, 2);
        return;
    }
    // -------------------------------------------------------------------- column riders: k_linsmall_bwd_cols's slice of HB_CW columns of the head's input
    if (HB_LAB(1)) return;
    constexpr int CW = HB_CW, ZI = 8;
    const int cb = bx - r0 - 1, c0 = cb * CW, cw = min(CW, EA - c0);
    float *dys = lds, *Ws = dys + N * EB, *Xs = Ws + EB * CW, *red = Xs + N * CW;       // dY2 [N][EB], W2 slice [EB][CW], X2 slice [N][CW] (then the dY1 slice), partial sums [4][EB * CW] / [32][CW]
    const int nout = EB * CW, G = min(4, 256 / nout);               // thread groups splitting the batch of one dW2 output (contiguous ranges, summed in order)
    float mk[ZI], mkb[ZI];
    float odw2 = 0.f, odb1 = 0.f, odb2 = 0.f;                        // what DW2 / DB1 / DB2 hold: each element has ONE writer in the launch, so the values are requested
                                                                     // with the staging loads and the three accumulations end in plain stores, not in round trips of their own
#pragma unroll
    for (int k = 0; k < ZI; k++) {
        const int z = tid + k * 256, n = z / CW, c = z - n * CW;
        const bool ok = z < N * CW && c < cw;
        const long o = (long)n * EA + c0 + c;
        mk[k] = ok ? hb.MASK[o] : 0.f; mkb[k] = (ok && hb.MSKB) ? hb.MSKB[o] : 0.f;
    }
    {   // staging: every global load goes out before the first LDS store (one round trip)
        constexpr int PRE = 6;
        float pd[PRE], pt[PRE], px[PRE], pw = 0.f;
#pragma unroll
        for (int q = 0; q < PRE; q++) { const int i = tid + q * 256; const bool ok = i < N * EB; pd[q] = ok ? hb.P[i] : 0.f; pt[q] = ok ? hb.T[i] : 0.f; }
        if (tid < EB * CW) { const int j = tid / CW, c = tid - j * CW; pw = c < cw ? hb.W2[(long)j * EA + c0 + c] : 0.f; }
#pragma unroll
        for (int q = 0; q < PRE; q++) { const int i = tid + q * 256, n = i / CW, c = i - n * CW; px[q] = (hb.train && i < N * CW && c < cw) ? hb.X2[(long)n * EA + c0 + c] : 0.f; }
        if (hb.train) {
            if (tid < nout) { const int j = tid / CW, c = tid - j * CW; if (c < cw) odw2 = hb.DW2[(long)j * EA + c0 + c]; }
            if (tid < cw) odb1 = hb.DB1[c0 + tid];
            if (cb == 0 && tid < EB) odb2 = hb.DB2[tid];
        }
#pragma unroll
        for (int q = 0; q < PRE; q++) { const int i = tid + q * 256; if (i < N * EB) dys[i] = pd[q] - pt[q]; }
        if (tid < EB * CW) Ws[tid] = pw;
        if (hb.train) {
#pragma unroll
            for (int q = 0; q < PRE; q++) { const int i = tid + q * 256; if (i < N * CW) Xs[i] = px[q]; }
        }
        for (int i = tid + PRE * 256; i < N * EB; i += 256) dys[i] = hb.P[i] - hb.T[i];
        if (hb.train)
            for (int i = tid + PRE * 256; i < N * CW; i += 256) { const int n = i / CW, c = i - n * CW; Xs[i] = c < cw ? hb.X2[(long)n * EA + c0 + c] : 0.f; }
    }
    __syncthreads();
    HB_STAMP(1);                                                     // staged
    if (tid == 0 && !HB_LAB(4)) __hip_atomic_store(pslots + bx, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // P and the target are staged here
    float dwacc = 0.f;
    if (hb.train && tid < nout * G) {
        const int g = tid / nout, t = tid - g * nout, j = t / CW, c = t - j * CW;
        const int nbt = (N + G - 1) / G, n0 = g * nbt, n1 = min(N, n0 + nbt);
#pragma unroll 8
        for (int n = n0; n < n1; n++) dwacc = fmaf(dys[n * EB + j], Xs[n * CW + c], dwacc);
        if (G > 1) red[g * nout + t] = dwacc;
    }
    __syncthreads();                                                 // the X2 slice is consumed: its place takes the dY1 slice
    HB_STAMP(2);                                                     // dW2 loop done
    if (hb.train && tid < nout) {                                    // the groups in order, onto what DW2 held: the store passes under the dX2 chain
        const int j = tid / CW, c = tid - j * CW;
        float a = dwacc;
        for (int g = 1; g < G; g++) a += red[g * nout + tid];
        if (c < cw) hb.DW2[(long)j * EA + c0 + c] = odw2 + a;
    }
    HB_STAMP(3);                                                     // DW2 accumulated
    {
        float g1v[ZI];
#pragma unroll
        for (int k = 0; k < ZI; k++) {                               // dX2[n, c0 + c] over X2 in place: fmaf chain ascending j (the oracle's order); dY1 = dX2 * mask
            const int z = tid + k * 256, n = z / CW, c = z - n * CW;
            g1v[k] = 0.f;
            if (z >= N * CW || c >= cw) continue;
            float acc = 0.f;
            for (int j = 0; j < EB; j++) acc = fmaf(dys[n * EB + j], Ws[j * CW + c], acc);
            const long o = (long)n * EA + c0 + c;
            hb.X2[o] = acc;
            float g1 = acc * mk[k]; hb.Y1[o] = g1;
            if (hb.MSKB) { g1 *= mkb[k]; hb.Y1B[o] = g1; }
            g1v[k] = g1;
        }
#pragma unroll
        for (int k = 0; k < ZI; k++) { const int z = tid + k * 256; if (z < N * CW) Xs[z] = g1v[k]; }
    }
    __syncthreads();                                                 // (every read of the dW2 partial sums lies in front of this barrier: red is free again)
    HB_STAMP(4);                                                     // dX2 / dY1 stored
    if (hb.train) {
        {   // dB1[c0 + c] = sum_n dY1[n, c0 + c] (k_dlinear_db nmath.cu:274-280): 64 row groups per column, then the groups in order
            const int c = tid & (CW - 1), g = tid >> 2;
            float b = 0.f;
#pragma unroll 4
            for (int n = g; n < N; n += 64) b += Xs[n * CW + c];
            red[g * CW + c] = b;
        }
        __syncthreads();
        if (tid < CW) {
            float b = 0.f;
#pragma unroll 8
            for (int g = 0; g < 64; g++) b += red[g * CW + tid];
            if (tid < cw) hb.DB1[c0 + tid] = odb1 + b;
        }
        HB_STAMP(5);                                                 // DB1 accumulated
        if (cb == 0) {                                               // dB2[j] = sum_n dY2[n, j]: 16 row groups per output
            __syncthreads();
            const int j = tid & 15, g = tid >> 4;
            float b = 0.f;
            if (j < EB) {
#pragma unroll 4
                for (int n = g; n < N; n += 16) b += dys[n * EB + j];
            }
            red[g * 16 + j] = b;
            __syncthreads();
            if (tid < EB) {
                float t = 0.f;
#pragma unroll
                for (int g2 = 0; g2 < 16; g2++) t += red[g2 * 16 + tid];
                hb.DB2[tid] = odb2 + t;
            }
            HB_STAMP(6);                                             // DB2 accumulated (rider 0)
        }
    }
    HB_FLUSH(8, 3);
}

} // namespace
