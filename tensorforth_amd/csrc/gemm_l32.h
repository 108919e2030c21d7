// gemm_l32.h - the sliver kernels: one 32x32 output tile per workgroup, K split over its waves, operand blocks through LDS-DMA.
// k_gemm_l32 is launched by gemm.hip (gemm_launch), k_gemm_dual_l32 by linear.hip (linear_bwd_dual); gemm_head_bwd.h follows the same body.
#pragma once
#include "gemm_types.h"

namespace {

// ------------------------------------------------------------------------------------------
// Latency-shaped GEMM for the slivers of small-batch training (a 256-row batch gives 8..100 tiles of 64x64: most CUs idle, every
// workgroup a serial chain of memory round trips).  One workgroup = one 32x32 output tile; its four waves split K (k-groups) and
// fetch their operand fragments STRAIGHT INTO REGISTERS in the MFMA operand layout - no LDS staging, no barriers in the K loop,
// 64 k of loads in flight per wave before the first MFMA and the next 64 issued under it.  The four partial accumulators meet in
// LDS once; each wave then finishes a quarter of the tile (alpha / beta / bias, mask chain).  4x the workgroups of the 64x64
// kernels, each with 1/16 of the matrix work per wave.
// Operand layout of v_mfma_f32_32x32x2_f32: lane (l31, h) supplies A[row = l31][k] and B[k][col = l31] for one k per instruction;
// chunk c covers k = 8c + 4h + {0..3}, as in the LDS kernels above.
// One 32x32 output tile per workgroup, K split over its NW waves (k-groups) which meet once in LDS; the whole epilogue rides (bias, activation + dropout riders, mask
// chain, column-sum and copy riders, split-K slabs).  The operand fragments come through wave-private LDS blocks filled by global_load_lds_dwordx4 (see the K loop):
// `red` is the workgroup's dynamic LDS of NW x 16 KiB; k-group w's partial accumulators land at red + w RS.  (Round 6: the register-fetch form of this body -
// k_gemm_s32 / k_gemm_dual32, row gathers of 16 bytes - is gone; shapes whose operands the DMA cannot take go to the 64x64 kernels.)
template <bool AKC, bool BKC, int NW = 4, bool RST = false>   // NW waves = NW k-groups per 32x32 tile; RST: blocks 2, 3 of a wave's range wait in registers
__device__ __forceinline__ void gemm_s32_body(const GemmP &p, const int bx, float *red,
                                              const int gate_mode = 0, const int gate_n = 0,
                                              const MaskChain *mc = nullptr, unsigned *slots = nullptr, const unsigned epoch = 0,
                                              const int by = 0, const FoldRider *fe = nullptr, const ActEpi *ep1 = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int M = p.M, N = p.N, K = p.K;
    const int kbeg = by * p.kchunk, kend = min(K, kbeg + p.kchunk);      // this workgroup's k range (split-K: slab `by`)
    const int T = p.tiles_m * p.tiles_n;
    if (bx >= T) {                                 // rider workgroups: cs_out[e] += sum_r cs_X[r, e] (k_dlinear_db nmath.cu:274-280)
        const int ex = tid & 63, ry = tid >> 6, e = (bx - T) * 64 + ex;
        float a = 0.f;
        if (e < p.cs_E && ry < 4) {
#pragma unroll 8
            for (int r = ry; r < p.cs_rows; r += 4) a += p.cs_X[(long)r * p.cs_E + e];
        }
        if (ry < 4) red[ry * 64 + ex] = a;
        __syncthreads();
        if (ry == 0 && e < p.cs_E) p.cs_out[e] += (red[ex] + red[64 + ex]) + (red[128 + ex] + red[192 + ex]);
        return;
    }
    // XCD-aware tile order (xmap): workgroup id % 8 is the XCD a workgroup runs on (private L2s).  In launch order neighbouring tiles - which share
    // an operand - sit on eight different XCDs and every L2 pulls both operands whole; a contiguous run of the column-major order gives an XCD
    // its own slice of B (2: outputs wider than tall), of the row-major order its own slice of A (1).
    int tm, tn;
    {
        int Lt = bx;                                           // (bx may be offset by a constant from the physical id - second GEMM of a dual launch: the groups bx % 8 are still the XCDs)
        if (p.xmap) { const int q8 = T >> 3, r8 = T & 7, x = bx & 7, i = bx >> 3; Lt = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i; }
        if (p.xmap == 2) { tn = Lt / p.tiles_m; tm = Lt - tn * p.tiles_m; } else { tm = Lt / p.tiles_n; tn = Lt - tm * p.tiles_n; }
    }
    const int tile = tm * p.tiles_n + tn;                  // logical id: the arrival slots are indexed by it
    const int m0 = tm * 32, n0 = tn * 32;
    // the share of the tile this wave finishes: accumulator registers QN w .. QN w + QN - 1 (QN = 16 / NW), row of register r = (r & 3) + 8 (r >> 2) + 4 h
    constexpr int QN = 16 / NW;
    const int gn = n0 + l31;
    float oprev[QN];
#pragma unroll
    for (int q = 0; q < QN; q++) oprev[q] = 0.f;
    if (p.beta != 0.f && p.nsplit == 1) {
#pragma unroll
        for (int q = 0; q < QN; q++) { const int r = QN * w + q, gm = m0 + (r & 3) + 8 * (r >> 2) + 4 * h; if (gm < M && gn < N) oprev[q] = p.O[(long)gm * N + gn]; }
    }
    // every read-only operand of the epilogue is requested here, with the K loop's first loads: fetched behind the reduction barrier, the
    // bias and the masks of the chain would each add a memory round trip to a launch that is little else
    float bias_v = 0.f, mk1[QN], mk2[QN];
    if (p.bias && p.nsplit == 1 && gn < N) bias_v = p.bias[gn];
#pragma unroll
    for (int q = 0; q < QN; q++) {
        mk1[q] = 0.f; mk2[q] = 0.f;
        if (mc && mc->d1 && p.nsplit == 1) {
            const int r = QN * w + q, gm = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (gm < M && gn < N) { const long z = (long)gm * N + gn; mk1[q] = mc->m1[z]; if (mc->d2) mk2[q] = mc->m2[z]; }
        }
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }
    // gate_mode 1 with per-wave slots (gate_n <= 128 reader workgroups): a wave reports as soon as its LAST operand fragments sit in
    // registers, in front of its last MFMA batch - the writers' wait then overlaps that batch, the LDS reduction and the epilogue
    const bool early = gate_mode == 1 && gate_n <= 128 && NW == 4;       // per-wave slots: 4 per reader workgroup
    auto arrive = [&]() __attribute__((always_inline)) {
        if (!early) return;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(slots + 4 * tile + w, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    constexpr int RS = 4096;                                      // floats between two k-groups' partial accumulators in `red`
    {
        // Coalesced operand fetch for slivers.  The register path above makes every wave load a gather (32 rows x 16 bytes: 64 cache-line
        // look-ups per instruction for 1 KiB, the address unit's queue stalls the wave's issue - SQ_WAIT_INST_ANY 42 % on the K-contiguous
        // forward layers).  Here a wave moves its k range in blocks of 32 k through two private LDS slots (A 4 KiB + B 4 KiB each):
        // a DMA instruction takes whole 128-byte runs (8 rows x 32 k of a K-contiguous operand, 8 k rows x 32 columns of the other kind),
        // no VGPR round trip, no barrier in the K loop (the blocks are the wave's own: s_waitcnt vmcnt only).
        //   K-contiguous block [32 rows][32 k]: the 16-byte quad q of row r sits at quad (q ^ ((r >> 1) & 7)) - the 16 lanes of a
        //   ds_read_b128 group ({0-3,12-15,20-27} ...) then cover all 64 banks once;  [K][M] block: [32 k][32 columns], ds_read_b32 rows.
        typedef __attribute__((address_space(3))) const float lds_f;
        typedef __attribute__((address_space(3))) const v4f lds_v4;
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)red;
        const int wu = __builtin_amdgcn_readfirstlane(w);
        const int nblk = (kend - kbeg + 31) >> 5;
        const int b0 = wu * nblk / NW, b1 = (wu + 1) * nblk / NW;
        const int i8 = lane >> 3, i7 = lane & 7;
        const float *pa[4], *pb[4]; int ka[4], kb[4];            // lane's source of DMA instruction j at k = 0, and the k (within a block) its validity hangs on
        const bool acol = AKC || m0 + 4 * i7 < M, bcol = BKC || n0 + 4 * i7 < N;
        const float *zsrc = p.Z + 4 * i7;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int r = 8 * j + i8, q = i7 ^ ((r >> 1) & 7);
            if (AKC) { pa[j] = p.A + (long)min(m0 + r, M - 1) * K + 4 * q; ka[j] = 4 * q; } else { pa[j] = p.A + (long)r * M + m0 + 4 * i7; ka[j] = r; }
            if (BKC) { pb[j] = p.B + (long)min(n0 + r, N - 1) * K + 4 * q; kb[j] = 4 * q; } else { pb[j] = p.B + (long)r * N + n0 + 4 * i7; kb[j] = r; }
        }
        auto issue = [&](int b, int slot) __attribute__((always_inline)) {
            const int k0 = kbeg + 32 * b;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float *sa = (k0 + ka[j] < kend && acol) ? (AKC ? pa[j] + k0 : pa[j] + (long)k0 * M) : zsrc;
                const float *sb = (k0 + kb[j] < kend && bcol) ? (BKC ? pb[j] + k0 : pb[j] + (long)k0 * N) : zsrc;
                const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((wu * 4096 + slot * 2048 + j * 256) * 4));
                asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(sa), "s"(la) : "memory");
                asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(sb), "s"(la + 4096u) : "memory");
            }
        };
        const int sw = (l31 >> 1) & 7;
        auto frag = [&](int slot, float (&fa)[4][4], float (&fb)[4][4]) __attribute__((always_inline)) {
            lds_f *a = (lds_f *)red + wu * 4096 + slot * 2048, *b = a + 1024;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (AKC) { const v4f t = *(lds_v4 *)(a + l31 * 32 + (((2 * c + h) ^ sw) << 2)); fa[c][0] = t[0]; fa[c][1] = t[1]; fa[c][2] = t[2]; fa[c][3] = t[3]; }
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) fa[c][j] = a[(8 * c + 4 * h + j) * 32 + l31];
                }
                if (BKC) { const v4f t = *(lds_v4 *)(b + l31 * 32 + (((2 * c + h) ^ sw) << 2)); fb[c][0] = t[0]; fb[c][1] = t[1]; fb[c][2] = t[2]; fb[c][3] = t[3]; }
                else {
#pragma unroll
                    for (int j = 0; j < 4; j++) fb[c][j] = b[(8 * c + 4 * h + j) * 32 + l31];
                }
            }
        };
        // Everything a wave needs is requested before its first wait: blocks 0 and 1 by DMA into the two slots, blocks 2 and 3 (RST) into
        // registers with the DMA's own lane -> address map (coalesced) - they are written to a slot (ds_write_b128, the DMA's image) once
        // its fragments have been read.  A second round trip would cost more than the copies: the fetch is what bounds these launches.
        const int nb = b1 - b0;
        v4f rs[RST ? 2 : 1][8];
        auto regload = [&](int b, int x) __attribute__((always_inline)) {
            const int k0 = kbeg + 32 * b;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float *sa = (k0 + ka[j] < kend && acol) ? (AKC ? pa[j] + k0 : pa[j] + (long)k0 * M) : zsrc;
                const float *sb = (k0 + kb[j] < kend && bcol) ? (BKC ? pb[j] + k0 : pb[j] + (long)k0 * N) : zsrc;
                rs[x][j] = *reinterpret_cast<const v4f *>(sa); rs[x][4 + j] = *reinterpret_cast<const v4f *>(sb);
            }
        };
        auto regstore = [&](int x, int slot) __attribute__((always_inline)) {
            typedef __attribute__((address_space(3))) v4f lds_w4;
            lds_w4 *d = (lds_w4 *)((__attribute__((address_space(3))) float *)red + wu * 4096 + slot * 2048) + lane;
#pragma unroll
            for (int j = 0; j < 4; j++) { d[j * 64] = rs[x][j]; d[256 + j * 64] = rs[x][4 + j]; }
        };
        auto wait_vm = [&](int blocks_after) __attribute__((always_inline)) {       // DMA and register loads return in issue order
            if (blocks_after >= 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
            else if (blocks_after == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else if (blocks_after == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        auto mm4 = [&](float (&fa)[4][4], float (&fb)[4][4]) __attribute__((always_inline)) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][0], fb[c][0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][1], fb[c][1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][2], fb[c][2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][3], fb[c][3], acc1, 0, 0, 0);
            }
        };
        if (nb > 0) {
            issue(b0, 0);
            if (nb > 1) issue(b0 + 1, 1);
            if (RST) { if (nb > 2) regload(b0 + 2, 0); if (nb > 3) regload(b0 + 3, 1); }
            constexpr int AHEAD = RST ? 4 : 2;                   // blocks requested up front
            int slot = 0;
            for (int i = 0; i < nb; i++) {
                if (i < 2 || !RST) wait_vm(min(nb, i < AHEAD ? AHEAD : i + 2) - 1 - i);   // blocks 2, 3 of RST: the register copies' own waits (compiler-counted) cover them
                else if (i >= 4) wait_vm(0);                      // deeper ranges (not dispatched today): DMA again, one block at a time
                float fa[4][4], fb[4][4];
                frag(slot, fa, fb);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (RST) { if (i == 0 && nb > 2) regstore(0, 0); if (i == 1 && nb > 3) regstore(1, 1); if (i + 2 < nb && i >= 2) issue(b0 + i + 2, slot); }
                else if (i + 2 < nb) issue(b0 + i + 2, slot);    // the slot's fragments sit in registers
                if (i + 1 >= nb) arrive();
                mm4(fa, fb);
                slot ^= 1;
            }
        } else arrive();
    }
    // the four k-groups meet in LDS: red[w][r][lane]
#pragma unroll
    for (int r = 0; r < 16; r++) red[w * RS + r * 64 + lane] = acc0[r] + acc1[r];
    // In-place dX: a writer waits until the reader workgroups of ITS columns have consumed their loads of the shared buffer.  No
    // counters: a reader stores this launch's epoch into its slot (fire and forget), the writer's first wave polls those slots with
    // agent-scope loads until all of them carry the epoch - one store and one load round trip on the critical path, nothing to re-arm.
    if (gate_mode == 1) {
        __syncthreads();
        if (!early && tid == 0) __hip_atomic_store(slots + tile, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (gate_mode == 2) {
        if (w == 0) {
            // only the readers of the columns this tile overwrites matter: dW tiles (e0t, tn), e0t = 0 .. gate_n / tiles_n - 1 (both GEMMs
            // have the same column tiling), each with 4 per-wave slots when those fit the 512-int block (gate_n <= 128)
            const int per = (gate_n <= 128 && NW == 4) ? 4 : 1, rows = gate_n / p.tiles_n, nslot = rows * per;
            for (int spin_it = 0;; spin_it++) {
                if (spin_it > T4K_SPIN_MAX) { if (lane == 0 && g_spin_err_dev) __hip_atomic_store(g_spin_err_dev, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }   // bounded: see t4k_common.h
                bool ok = true;
                unsigned bad = 0;                                  // no short-circuit: the loads of one pass are independent and go out together
#pragma unroll 4
                for (int i = lane; i < nslot; i += 64) {
                    const int e0t = i / per, ww = i - e0t * per;
                    bad |= __hip_atomic_load(slots + per * (e0t * p.tiles_n + tn) + ww, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ^ epoch;
                }
                ok = bad == 0;
                if (__all(ok)) break;
                __builtin_amdgcn_s_sleep(2);
            }
        }
        __syncthreads();
    } else __syncthreads();
    const float alpha = p.alpha, beta = p.beta;
#pragma unroll
    for (int q = 0; q < QN; q++) {
        const int r = QN * w + q, gm = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float v = red[r * 64 + lane];
#pragma unroll
        for (int g = 1; g < NW; g++) v += red[g * RS + r * 64 + lane];           // k-groups in order
        if (gm < M && gn < N) {
            const long z = (long)gm * N + gn;
            if (p.nsplit > 1) { p.part[(long)by * M * N + z] = v; continue; }       // split-K slab: the consumer folds (XFold / k_splitk_fold)
            float o = v * alpha;
            if (beta != 0.f) o += oprev[q] * beta;
            if (p.bias) o += bias_v;
            p.O[z] = o;
            if (mc && mc->d1) { const float g1 = o * mk1[q]; mc->d1[z] = g1; if (mc->d2) mc->d2[z] = g1 * mk2[q]; }
            if (ep1 && ep1->layer) {                                              // element-wise layer(s) behind a linear layer: as k_splitk_fold
                const bool d1 = ep1->layer == T4K_L_DROPOUT, d2 = fe && fe->ep2.layer == T4K_L_DROPOUT;
                float u = 0.f;
                if (d1 || d2) { uint64_t base, seed; rng_begin(d2 ? fe->ep2.rng : ep1->rng, base, seed); u = philox_u01_at(base, seed, z); }
                float a, f; act_rt(ep1->layer, o, d1 ? u : 0.f, ep1->alpha, a, f); ep1->F[z] = f; ep1->A[z] = a;
                if (fe && fe->ep2.layer) { float a2, f2; act_rt(fe->ep2.layer, a, d2 ? u : 0.f, fe->ep2.alpha, a2, f2); fe->ep2.F[z] = f2; fe->ep2.A[z] = a2; }
            }
        }
    }
}
// one GEMM on 32x32 tiles (see gemm_s32_body): grid = (tiles + column-sum riders + copy riders, k slabs); epilogue riders as the fold launch's; dynamic LDS = NW x 16 KiB
template <bool AKC, bool BKC, int NW, bool RST>
__global__ void __launch_bounds__(64 * NW) k_gemm_l32(GemmP p, ActEpi ep, FoldRider fr) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int nwork = (int)gridDim.x - fr.cp_blocks;
    if ((int)blockIdx.x >= nwork) {                              // the model's copy of the batch into its layer 0 rides along (forward.cu:39)
        if (blockIdx.y) return;
        const long t0 = (long)((int)blockIdx.x - nwork) * (64 * NW) + threadIdx.x, step = (long)fr.cp_blocks * (64 * NW);
        if (fr.cp_vec) {
            const long n4 = fr.cp_n >> 2;
            for (long z = t0; z < n4; z += step) reinterpret_cast<float4 *>(fr.cp_dst)[z] = reinterpret_cast<const float4 *>(fr.cp_src)[z];
            for (long z = (n4 << 2) + t0; z < fr.cp_n; z += step) fr.cp_dst[z] = fr.cp_src[z];
        } else
            for (long z = t0; z < fr.cp_n; z += step) fr.cp_dst[z] = fr.cp_src[z];
        return;
    }
    if ((int)blockIdx.x >= p.tiles_m * p.tiles_n && blockIdx.y) return;   // column-sum riders run once
    gemm_s32_body<AKC, BKC, NW, RST>(p, blockIdx.x, lds, 0, 0, fr.mc.d1 ? &fr.mc : nullptr, nullptr, 0, blockIdx.y, &fr, &ep);
}
template <bool AKC, bool BKC, int NW, bool RST>
void launch_l32(const GemmP &p, const ActEpi &ep, const FoldRider &fr, dim3 grid, hipStream_t s) {
    launch_lds<k_gemm_l32<AKC, BKC, NW, RST>>(grid, dim3(64 * NW), (size_t)NW * 16384, s, p, ep, fr);
}
// dW += dY^T X (+ dB rider) and dX = dY W of one linear layer on 32x32 tiles (see k_gemm_dual for the gate): NW waves, NW x 16 KiB of dynamic LDS.  More workgroups than resident slots are
// fine here although the dX writers spin on the dW readers' slots: a writer's readers all have LOWER workgroup ids, each XCD dispatches its
// workgroups in id order and a reader never waits - so every reader is running or done before the first writer of its XCD takes a slot
// (the same dispatch-order argument as the conv stack's band exchange; the wait is bounded and reported anyway).
template <bool RST, int NW = 4>
__global__ void __launch_bounds__(64 * NW) k_gemm_dual_l32(GemmP p1, GemmP p2, int nb1, int t1, int t2, unsigned *slots, unsigned epoch, MaskChain mc) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if ((int)blockIdx.x < nb1) gemm_s32_body<false, false, NW, RST>(p1, blockIdx.x, lds, slots ? 1 : 0, t1, nullptr, slots, epoch);
    else                       gemm_s32_body<true, false, NW, RST>(p2, (int)blockIdx.x - nb1, lds, slots ? 2 : 0, t1, &mc, slots, epoch);
}

} // namespace
