// gemm.hip - fp32 GEMM on gfx950 matrix cores (v_mfma_f32_32x32x2_f32, exact f32 fma chain).
//
//   O[M,N,C] = alpha * op(A) @ op(B) + beta * O      (reference k_gemm_tile_claude,
//   src/t4math.cu:478-583; host wrappers Tensor::gemm3 / mm / linear, src/mu/tensor.cu:73-87,161-180)
//
// Design (MI355X-first, not a translation of the reference's 64x64x16 VALU tiling):
//   * workgroup = 256 threads = 4 waves in a 2x2 grid; macro tile 64x64 (one 32x32 MFMA
//     accumulator per wave) when that yields <= ~1 tile per CU (the 1024^2 case: exactly 256
//     tiles on 256 CUs), 128x128 (2x2 accumulators per wave) for larger problems.
//   * K is consumed in stages of BK (32 or 64); LDS is double buffered; the global loads of a
//     later stage are issued into registers before the MFMAs of the current one and written
//     to LDS after them (issue-early / write-late), one barrier per stage.
//   * SKEW: the MFMAs of a stage's last 8-deep k chunk are issued AFTER the barrier, so the
//     matrix pipe stays busy while the next stage's first operand reads are in flight.
//   * an operand whose K axis is contiguous in memory (A normal, B transposed) is kept
//     [row][k] in LDS with a 16-byte XOR swizzle and read with ds_read_b128 (4 k-values per
//     lane, conflict free); the other kind is kept [k][row] and read with ds_read_b32.
//     Within each 8-deep k chunk, MFMA j consumes k = {j, 4+j} (lane halves), so one b128
//     read feeds four MFMAs.  Summation order inside a chunk is therefore 0,4,1,5,2,6,3,7.
//   * blockIdx -> tile mapping is XCD aware (block b runs on XCD b%8): each XCD gets a
//     compact 4-row band of tiles so its private 4 MiB L2 holds the A rows / B columns it re-reads.
//   * small outputs (few tiles, deep K - the CNN's linear layers) are split along K across
//     workgroups; partial slabs go to the library workspace and a second launch folds them in
//     slice order (deterministic; no fp32 atomics).
//   * arbitrary M/N/K tails, channel stride C > 1 and unaligned operands take the same
//     kernel with per-element predicated loads (VEC = false).
//
// This unit holds the dispatch ladder (gemm_launch) with the kernels only it launches - the LDS-DMA pipelines, the split-K fold, the
// f64-accumulate kernel - and the words' entry points.  The kernel bodies shared with other units sit in headers: gemm_tile.h
// (register-staged tile), gemm_l32.h (32x32 slivers); the linear layers' policy and entry points are linear.hip.  gemm_batched.hip's
// tile kernel stays here: it shares the tile body's instantiations with k_gemm_mfma, and only so does its code come out as before.
#include "gemm_types.h"
#include "gemm_tile.h"
#include "gemm_l32.h"

namespace {

// ------------------------------------------------------------------------------------------
// planner -> plan -> launch.  gemm_plan (in front of gemm_launch, below) answers a GemmAsk in a GemmEnv with a GemmPlan and launches nothing;
// gemm_launch and the launch wrappers read the plan and decide nothing.  GemmRung is the one list of rungs: a value per string of
// t4k_gemm_last_plan, in the order of rung_text[].
enum GemmRung : int { GR_UNSET = 0, GR_NONE, GR_K0, GR_L32_W4, GR_L32_W4_RST, GR_L32_W8, GR_L32_W8_RST, GR_PAIR, GR_NN_PLAIN, GR_PLAIN_ANY, GR_PLAIN_RAGK,
                      GR_PLAIN128, GR_PLAIN128_RAGK, GR_PLAIN128_BK32, GR_PLAIN256, GR_GLDS8_128, GR_GLDS8_64, GR_GLDS8_128_RAGK, GR_GLDS8_64_RAGK,
                      GR_MFMA128_FULL, GR_MFMA128_SKEW, GR_MFMA128, GR_MFMA64_32, GR_MFMA64_FULL, GR_MFMA64_SKEW, GR_COUNT };
const char *const rung_text[GR_COUNT] = { "", "none", "k0", "l32/w4", "l32/w4/rst", "l32/w8", "l32/w8/rst", "pair", "nn_plain", "plain_any", "plain_ragk",
                      "plain128", "plain128/ragk", "plain128/bk32", "plain256", "glds8<128>", "glds8<64>", "glds8<128,ragk>", "glds8<64,ragk>",
                      "mfma<128,128,32,vec,full>", "mfma<128,128,32,vec,skew>", "mfma<128,128,32>", "mfma<64,64,32>", "mfma<64,64,64,vec,full>", "mfma<64,64,64,vec,skew>" };
// the question: one product as its caller describes it
struct GemmAsk {
    int M, N, K, C, tA, tB;
    bool a16, b16;          // A, B on 16 bytes
    bool plain;             // (alpha, beta) == (1, 0)
    bool bias;
    bool riders;            // an activation epilogue or a FoldRider is asked for
    bool defer;             // the caller folds split slabs itself
    bool cs; int cs_rows, cs_E;   // a column-sum request and its extents
};
// what gemm_launch reads from State and the stream
struct GemmEnv { int cu; size_t ws_bytes; bool d_zero, d_sync, gates; int lane; bool capturing; };
enum { RIDE_NONE = 0, RIDE_LAUNCH, RIDE_FOLD };
struct GemmPlan {
    GemmRung rung = GR_NONE;
    int tiles_m = 0, tiles_n = 0;
    unsigned gx = 0, gy = 1, gz = 1;     // the grid of the product's launch, column-sum workgroups included (a sliver's copy rider adds its own at launch)
    int nsplit = 1, kchunk = 0;
    bool w8 = false, rst = false;        // slivers: 8 waves (k-groups) per workgroup; a wave walks more than two blocks
    int xmap = 0;
    bool pow2 = false, swap = false;     // k_gemm_nn_plain: shift / mask tile prologue; tile order with M and N exchanged
    bool epi = false;                    // lean kernels: alpha / beta / bias epilogue
    bool cs_rides = false; unsigned cs_wgs = 0;
    int riders = RIDE_NONE;              // where an activation / mask-chain / copy rider is applied: the product's launch, the fold, nowhere
    bool deferred = false, fold = false;
    int launches = 0;
};

// ------------------------------------------------------------------------------------------
// 64x64 interior tiles, direct-to-LDS staging: global_load_lds_dwordx4 (LDS-DMA, no VGPR round
// trip, no ds_write pass), 3 LDS stage buffers, loads two stages ahead, counted vmcnt waits and
// raw s_barrier so the DMA of later stages stays in flight across barriers.  The DMA writes LDS
// lane-linearly (wave-uniform base + lane*16 B), so the XOR swizzle of a K-contiguous operand is
// applied to the per-lane SOURCE address and undone on the ds_read_b128 side.
// 8-wave workgroups: two waves per SIMD.  Waves 4..7 take the upper half of every stage's k chunks
// into their own accumulators, so one wave's LDS reads and waits sit under the other's MFMAs; the halves are summed
// through LDS in the epilogue (fixed order).  (Round 6: the 4-wave form of this pipeline, k_gemm_glds, and the variant switch that selected it are gone.)
//
// RAGK: K need not be a whole number of stages.  The last, partial stage is one more DMA stage whose source addresses are clamped to the
// operand's last valid 16-byte group / row (so every lane still moves 16 bytes and the vmcnt bookkeeping is unchanged); the 8-deep chunks
// past the tail are never read, and in a partial last chunk the k positions past the tail are zeroed in registers on BOTH operands
// (0 x stale-LDS garbage could be NaN).  The tail's chunks alternate between the two k-groups.  K = 784 (a 28 x 28 image row, the GAN
// layer width) = 6 stages of 128 + 16: this kernel instead of the predicated register-staged one.
template <int BK, bool AKC, bool BKC, bool PRIO = false, bool RAGK = false>   // PRIO: s_setprio around the MFMA burst - measured +1.2 us at 1024^3, kept off
__global__ void __launch_bounds__(512) k_gemm_glds8(GemmP p) {
    constexpr int BM = 64, BN = 64;
    constexpr int NC = BK / 8, CH = BK / 4, SW = (64 / BK) > 0 ? (64 / BK) : 1;
    constexpr int NST = (BK >= 128) ? 2 : 3;         // stage buffers: a 128-deep stage is 64 KiB, two of them fit (half the barriers per K)
    constexpr int STAGE = (BM + BN) * BK;          // floats per stage buffer
    constexpr int NI = BK / 4;                     // 1-KiB DMA instructions per operand per stage
    constexpr int NJ = NI / 8;                     // ... per wave (8 waves)
    constexpr int NPW = 2 * NJ;                    // DMA instructions per wave per stage
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = w >> 2, w4 = w & 3;               // k-group (which half of every stage's chunks), wave within the 2x2 tile grid
    const int wm = w4 >> 1, wn = w4 & 1, h = lane >> 5, l31 = lane & 31;
    constexpr int NCG = NC / 2;                       // chunks per k-group per stage
    const int c0 = kg * NCG;
    const int M = p.M, N = p.N, K = p.K;

    const int T = p.tiles_m * p.tiles_n;
    int L;
    {
        const int b = blockIdx.x, q8 = T >> 3, r8 = T & 7, x = b & 7, i = b >> 3;
        L = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i;
    }
    constexpr int GROUP_M = 4;
    const int per_group = GROUP_M * p.tiles_n;
    const int grp = L / per_group, first_m = grp * GROUP_M;
    const int gsz = min(p.tiles_m - first_m, GROUP_M);
    const int tm = first_m + (L % per_group) % gsz, tn = (L % per_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = blockIdx.y * p.kchunk;
    const int kend = min(K, kbeg + p.kchunk);
    const int nst  = (kend - kbeg) / BK;
    const int tail = RAGK ? (kend - kbeg) - nst * BK : 0;      // k positions of the partial last stage
    const int nstT = nst + (tail > 0 ? 1 : 0);                 // stages the DMA pipeline moves

    // per-lane DMA source offsets (bytes from the operand base) of stage 0; the launcher guarantees both operands span < 4 GiB
    unsigned voffA[NJ], voffB[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int i = w * NJ + j;
        // rows / 4-column groups past a ragged edge are clamped to the last valid one (valid memory; they only feed accumulator rows /
        // columns the epilogue never stores), so N = 1000 classes or a 784-wide image row run this kernel like interior tiles
        if (AKC) { const int r = i * (256 / BK) + lane / CH, ql = lane % CH, q = ql ^ ((r / SW) & (CH - 1));
                   voffA[j] = (unsigned)(((long)min(m0 + r, M - 1) * K + kbeg + q * 4) * 4); }
        else     { const int kk = i * 4 + lane / 16, ch = lane % 16;
                   voffA[j] = (unsigned)(((long)(kbeg + kk) * M + min(m0 + ch * 4, M - 4)) * 4); }
        if (BKC) { const int r = i * (256 / BK) + lane / CH, ql = lane % CH, q = ql ^ ((r / SW) & (CH - 1));
                   voffB[j] = (unsigned)(((long)min(n0 + r, N - 1) * K + kbeg + q * 4) * 4); }
        else     { const int kk = i * 4 + lane / 16, ch = lane % 16;
                   voffB[j] = (unsigned)(((long)(kbeg + kk) * N + min(n0 + ch * 4, N - 4)) * 4); }
    }
    const long stepA = AKC ? BK : (long)BK * M, stepB = BKC ? BK : (long)BK * N;

    // The DMA is issued from inline asm (saddr form: scalar base + each lane's fixed 32-bit byte offset).  Through the
    // __builtin_amdgcn_global_load_lds builtin hipcc books the load as "flat, may touch LDS": while one is pending it turns every LDS
    // dependency into s_waitcnt lgkmcnt(0), so the operand reads just issued for the NEXT chunk were waited for at once - one exposed LDS
    // round trip per 8 MFMAs (1024^3: 21.5 us).  Invisible to the compiler, it emits counted lgkmcnt(N) ladders instead (19.4 us); the
    // DMA's own completion is waited for by the explicit vmcnt waits in wait_next().
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)lds;
    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        const float *ba = p.A + kt * stepA, *bb = p.B + kt * stepB;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((buf * STAGE + (w * NJ + j) * 256) * 4));
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffA[j]), "s"(ba), "s"(la) : "memory");
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffB[j]), "s"(bb), "s"(la + BM * BK * 4) : "memory");
        }
    };
    // the partial last stage: same LDS placement (a lane's 16 bytes land at its own slot whatever the exec mask), but only the lanes /
    // instructions whose k lies inside the tail move anything - a clamped full stage would cost a full stage of L2 bandwidth for 16 columns.
    // Three-buffer pipelines count vmcnt per stage, so there every instruction is issued (sources clamped into [kb, kend)).
    auto issue_tail = [&](int buf) __attribute__((always_inline)) {
        const int kb = kbeg + nst * BK;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int i = w * NJ + j;
            unsigned va, vb; bool oka, okb;
            if (AKC) { const int r = i * (256 / BK) + lane / CH, ql = lane % CH, q = ql ^ ((r / SW) & (CH - 1));
                       oka = q * 4 < tail;
                       va = (unsigned)(((long)min(m0 + r, M - 1) * K + min(kb + q * 4, kend - 4)) * 4); }
            else     { const int kk = i * 4 + lane / 16, ch = lane % 16;
                       oka = i * 4 < tail;                                  // wave-uniform: whole instructions past the tail are skipped
                       va = (unsigned)(((long)min(kb + kk, kend - 1) * M + min(m0 + ch * 4, M - 4)) * 4); }
            if (BKC) { const int r = i * (256 / BK) + lane / CH, ql = lane % CH, q = ql ^ ((r / SW) & (CH - 1));
                       okb = q * 4 < tail;
                       vb = (unsigned)(((long)min(n0 + r, N - 1) * K + min(kb + q * 4, kend - 4)) * 4); }
            else     { const int kk = i * 4 + lane / 16, ch = lane % 16;
                       okb = i * 4 < tail;
                       vb = (unsigned)(((long)min(kb + kk, kend - 1) * N + min(n0 + ch * 4, N - 4)) * 4); }
            const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((buf * STAGE + i * 256) * 4));
            if (NST == 3 || oka) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(va), "s"(p.A), "s"(la) : "memory");
            if (NST == 3 || okb) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(vb), "s"(p.B), "s"(la + BM * BK * 4) : "memory");
        }
    };
    auto issue_any = [&](int kt, int buf) __attribute__((always_inline)) {
        if (!RAGK || kt < nst) issue(kt, buf); else issue_tail(buf);
    };

    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }

    const int ra_ = wm * 32 + l31, rb_ = wn * 32 + l31;
    // operand fragments of one 8-deep k chunk (lane half h holds k = 8*ci + 4*h + {0..3})
    auto rd = [&](const float *a, const float *b, int ci, float (&av)[4], float (&bv)[4]) __attribute__((always_inline)) {
        if (AKC) { const v4f t = *reinterpret_cast<const v4f *>(a + ra_ * BK + (((ci * 2 + h) ^ ((ra_ / SW) & (CH - 1))) << 2));
                   av[0] = t[0]; av[1] = t[1]; av[2] = t[2]; av[3] = t[3]; }
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) av[j] = a[(ci * 8 + 4 * h + j) * BM + ra_];
        }
        if (BKC) { const v4f t = *reinterpret_cast<const v4f *>(b + rb_ * BK + (((ci * 2 + h) ^ ((rb_ / SW) & (CH - 1))) << 2));
                   bv[0] = t[0]; bv[1] = t[1]; bv[2] = t[2]; bv[3] = t[3]; }
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) bv[j] = b[(ci * 8 + 4 * h + j) * BN + rb_];
        }
    };
    auto mm = [&](float (&av)[4], float (&bv)[4]) __attribute__((always_inline)) {
        if (PRIO) __builtin_amdgcn_s_setprio(2);                 // keep the matrix pipe fed: the MFMA burst outranks the other wave's loads
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], bv[0], acc0, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);                       // keep the two accumulators alternating (hipcc pairs them otherwise)
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], bv[1], acc1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], bv[2], acc0, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], bv[3], acc1, 0, 0, 0);
        if (PRIO) __builtin_amdgcn_s_setprio(0);
    };
    auto wait_next = [&](bool more) __attribute__((always_inline)) {      // next stage landed; later one may fly
        if (more) { if (NPW == 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
                    else          asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory"); }
        else        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    if (nstT > 0) issue_any(0, 0);
    if (NST == 3 && nstT > 1) issue_any(1, 1);
    wait_next(NST == 3 && nstT > 1);

    // Software pipeline: the operands of chunk c+1 are read BEFORE the MFMAs of chunk c are issued,
    // and the MFMAs of a stage's last chunk are issued after the barrier, behind the first reads of
    // the next stage - the matrix pipe never waits on an LDS round trip.
    float ca[4], cb[4];
    if (nst > 0) rd(lds, lds + BM * BK, c0, ca, cb);
    int buf = 0;
    for (int kt = 0; kt < nst; kt++) {
        int nb = buf + 2; if (nb >= 3) nb -= 3;
        int b1 = buf + 1; if (b1 >= NST) b1 = 0;
        if (NST == 3) { if (kt + 2 < nstT) issue_any(kt + 2, nb); }      // overwrites the buffer read in stage kt-1
        else          { if (kt + 1 < nstT) issue_any(kt + 1, b1); }      // two buffers: the other one was read in stage kt-1
        const float *a = lds + buf * STAGE, *b = a + BM * BK;
#pragma unroll
        for (int ci = 0; ci + 1 < NCG; ci++) {
            float na[4], nbv[4];
            rd(a, b, c0 + ci + 1, na, nbv);
            __builtin_amdgcn_sched_barrier(0);
            mm(ca, cb);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; j++) { ca[j] = na[j]; cb[j] = nbv[j]; }
        }
        wait_next(NST == 3 && kt + 2 < nstT);               // all my reads of stage kt done; stage kt+1 visible
        float na[4], nbv[4];
        if (kt + 1 < nst) rd(lds + b1 * STAGE, lds + b1 * STAGE + BM * BK, c0, na, nbv);
        __builtin_amdgcn_sched_barrier(0);
        mm(ca, cb);
        if (kt + 1 < nst) {
#pragma unroll
            for (int j = 0; j < 4; j++) { ca[j] = na[j]; cb[j] = nbv[j]; }
        }
        buf = b1;
    }
    if (RAGK && tail > 0) {                                  // the partial stage sits in `buf`, visible since the last barrier
        const float *a = lds + buf * STAGE, *b = a + BM * BK;
        const int nct = (tail + 7) >> 3;
        // k positions past the tail are zeroed when the fragment is handed to the MFMAs (not at the read: that would wait for the LDS round trip)
        auto zf = [&](int c, float (&dv)[4], float (&ev)[4], const float (&av)[4], const float (&bv)[4]) __attribute__((always_inline)) {
            const int k0 = c * 8 + 4 * h;
#pragma unroll
            for (int j = 0; j < 4; j++) { const bool in = k0 + j < tail; dv[j] = in ? av[j] : 0.f; ev[j] = in ? bv[j] : 0.f; }
        };
        int c = kg;                                          // its chunks alternate between the k-groups; same read-ahead as the main loop
        float ra4[4], rb4[4];
        if (c < nct) { rd(a, b, c, ra4, rb4); zf(c, ca, cb, ra4, rb4); }
        for (; c < nct; c += 2) {
            if (c + 2 < nct) rd(a, b, c + 2, ra4, rb4);
            __builtin_amdgcn_sched_barrier(0);
            mm(ca, cb);
            __builtin_amdgcn_sched_barrier(0);
            if (c + 2 < nct) zf(c + 2, ca, cb, ra4, rb4);
        }
    }

    const float alpha = p.alpha, beta = p.beta;
    const int gn = n0 + wn * 32 + l31;
    float add[16];
    // the two k-groups meet in LDS (the stage buffers are free now): group 1 parks its 32x32 blocks, group 0 adds them
    __syncthreads();
    if (kg == 1) {
#pragma unroll
        for (int r = 0; r < 16; r++) lds[(w4 * 16 + r) * 64 + lane] = acc0[r] + acc1[r];
    }
    __syncthreads();
    if (kg == 1) return;
#pragma unroll
    for (int r = 0; r < 16; r++) add[r] = lds[(w4 * 16 + r) * 64 + lane];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int gm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = (acc0[r] + acc1[r]) + add[r];
        if (gm >= M || gn >= N) continue;                   // ragged edge tile
        if (p.nsplit > 1) p.part[((long)blockIdx.y * M + gm) * N + gn] = v;
        else {
            const long z = (long)gm * N + gn;
            float o = v * alpha;
            if (beta != 0.f) o += p.O[z] * beta;
            if (p.bias) o += p.bias[gn];
            __builtin_nontemporal_store(o, &p.O[z]);        // streaming store: no dirty L2 lines left for the kernel-end write-back (-0.27 us at 1024^3)
        }
    }
}

// The plain product O = A @ B (word `matmul`, tA = tB = 0, alpha = 1, beta = 0, no bias, interior 64x64 tiles, K % 128 == 0) has its own
// copy of the 8-wave kernel with nothing else in it: the same loop inside the general template above measures 20.1 us at 1024^3, this
// one 19.4 (tools/gemm_lab.hip: every variant with in-kernel cycle stamps; the loop is sensitive to the code around it).
#ifndef T4K_GEMM_EARLY_ISSUE
#define T4K_GEMM_EARLY_ISSUE 1      // k_gemm_plain128: stage kt + 2 requested right behind stage kt's closing barrier (0: at the top of stage kt + 1; 2048^2 x 1024: 67.7 -> 66.7 us).
#endif                              // Measured and dropped: the same in k_gemm_nn_plain (19.1 -> 19.9 us at 1024^3), and the DMA instructions spread between the MFMAs of either kernel (-2..3 %)
struct PlainP { const float *A, *B; float *O; int M, N, K; float alpha, beta; const float *bias; int *sync; float *part; int swap; };   // swap: tile order with the roles of M and N exchanged (lab: T4K_GEMM_TT_SWAP)
// The other operand layouts (word `matmul` on transposed views; Tensor::linear tensor.cu:79-87 = X @ W^T + b with alpha / beta) get the same
// lean kernel instead of the general template: AKC / BKC pick the operand layout (K-contiguous rows, read with ds_read_b128 through the
// XOR swizzle, or k-major rows read per k), EPI adds alpha / beta / bias to the store.  Interior 64x64 tiles, K % 128 == 0, unsplit.
// PAIR: an output of 65..128 tiles would leave half the CUs idle (512 x 1024 x 1024: 128 tiles).  gridDim.y = 2 workgroups share a tile,
// one K half each; the first to finish parks its 64x64 partial in the workspace and raises a flag, the second adds it and stores -
// a + b == b + a, so the result does not depend on who arrives first and no fold launch follows.  The parker never waits, so the
// waiter's (bounded) spin cannot deadlock whatever the residency.
// RAGK: K >= 128 with a partial last stage (784 = 6 x 128 + 16), see k_gemm_glds8: the tail is one more DMA stage in which only the lanes whose
// k lies inside the tail move anything, its 8-deep chunks alternate between the k-groups, positions past the tail are zeroed in registers.
template <bool POW2, bool AKC = true, bool BKC = false, bool EPI = false, bool PAIR = false, bool RAGK = false>
__global__ void __launch_bounds__(512) k_gemm_nn_plain(PlainP p) {
    constexpr int BM = 64, BN = 64, BK = 128;
    constexpr int NC = BK / 8, CH = BK / 4;
    constexpr int STAGE = (BM + BN) * BK, NI = BK / 4, NJ = NI / 8, NCG = NC / 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = w >> 2, w4 = w & 3, wm = w4 >> 1, wn = w4 & 1, h = lane >> 5, l31 = lane & 31;
    const int c0 = kg * NCG;
    const int M = p.M, N = p.N, K = p.K;
    const int tiles_m = M / BM, tiles_n = N / BN, T = tiles_m * tiles_n;
    int tm, tn;
    if (POW2) {                                             // power-of-two tile grid with T % 32 == 0 (1024^2: 16 x 16): the XCD-aware tile order in shifts -
        const int tnb = 31 - __builtin_clz(p.swap ? tiles_m : tiles_n), b = blockIdx.x;     // the general form below costs three integer divisions (~400 cycles) before the first DMA
        const int L = (b & 7) * (T >> 3) + (b >> 3), pg = 2 + tnb, r = L & ((1 << pg) - 1);
        const int u = ((L >> pg) << 2) + (r & 3), v = r >> 2;
        tm = p.swap ? v : u; tn = p.swap ? u : v;
    } else {
        int L;
        {
            const int b = blockIdx.x, q8 = T >> 3, r8 = T & 7, x = b & 7, i = b >> 3;
            L = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i;
        }
        constexpr int GROUP_M = 4;
        const int per_group = GROUP_M * tiles_n;
        const int grp = L / per_group, first_m = grp * GROUP_M;
        const int gsz = min(tiles_m - first_m, GROUP_M);
        tm = first_m + (L % per_group) % gsz; tn = (L % per_group) / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN, nst = PAIR ? (K >> 1) / BK : K / BK;
    const int kt0 = PAIR ? (int)blockIdx.y * nst : 0;      // first stage of this workgroup's K half
    const int tail = RAGK ? K - nst * BK : 0;
    unsigned voffA[NJ], voffB[NJ];
    {
        const int r0 = w * 8 + (lane >> 5), ql = lane & 31, kk0 = w * 16 + (lane >> 4);
        // one multiply per operand: a K-contiguous operand's instruction j covers rows r0 + 2j (swizzled 16-byte groups), a k-major one's k rows kk0 + 4j
        const unsigned ba = AKC ? (unsigned)((m0 + r0) * K) * 4u : (unsigned)(kk0 * M + m0 + (lane & 15) * 4) * 4u;
        const unsigned bb = BKC ? (unsigned)((n0 + r0) * K) * 4u : (unsigned)(kk0 * N + n0 + (lane & 15) * 4) * 4u;
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            voffA[j] = AKC ? ba + (unsigned)(2 * j * K) * 4u + (unsigned)((ql ^ ((r0 + 2 * j) & 31)) << 4) : ba + (unsigned)(4 * j * M) * 4u;
            voffB[j] = BKC ? bb + (unsigned)(2 * j * K) * 4u + (unsigned)((ql ^ ((r0 + 2 * j) & 31)) << 4) : bb + (unsigned)(4 * j * N) * 4u;
        }
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)lds;
    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        const long ks = kt0 + kt;
        const float *ba = p.A + (AKC ? ks * BK : ks * BK * M), *bb = p.B + (BKC ? ks * BK : ks * BK * N);
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((buf * STAGE + (w * NJ + j) * 256) * 4));
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffA[j]), "s"(ba), "s"(la) : "memory");
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffB[j]), "s"(bb), "s"(la + BM * BK * 4) : "memory");
        }
    };
    auto issue_tail = [&](int buf) __attribute__((always_inline)) {        // stage nst: same lane offsets, lanes past the tail switched off (nothing read out of bounds)
        const float *ba = p.A + (AKC ? (long)nst * BK : (long)nst * BK * M), *bb = p.B + (BKC ? (long)nst * BK : (long)nst * BK * N);
        const int r0 = w * 8 + (lane >> 5), ql = lane & 31, kk0 = w * 16 + (lane >> 4);
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((buf * STAGE + (w * NJ + j) * 256) * 4));
            const bool kin = ((ql ^ ((r0 + 2 * j) & 31)) << 2) < tail, rin = kk0 + 4 * j < tail;
            if (AKC ? kin : rin) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffA[j]), "s"(ba), "s"(la) : "memory");
            if (BKC ? kin : rin) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffB[j]), "s"(bb), "s"(la + BM * BK * 4) : "memory");
        }
    };
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const int ra_ = wm * 32 + l31, rb_ = wn * 32 + l31;
    auto rd = [&](const float *a, const float *b, int ci, float (&av)[4], float (&bv)[4]) __attribute__((always_inline)) {
        if (AKC) { const v4f t = *reinterpret_cast<const v4f *>(a + ra_ * BK + (((ci * 2 + h) ^ (ra_ & (CH - 1))) << 2));
                   av[0] = t[0]; av[1] = t[1]; av[2] = t[2]; av[3] = t[3]; }
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) av[j] = a[(ci * 8 + 4 * h + j) * BM + ra_];
        }
        if (BKC) { const v4f t = *reinterpret_cast<const v4f *>(b + rb_ * BK + (((ci * 2 + h) ^ (rb_ & (CH - 1))) << 2));
                   bv[0] = t[0]; bv[1] = t[1]; bv[2] = t[2]; bv[3] = t[3]; }
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) bv[j] = b[(ci * 8 + 4 * h + j) * BN + rb_];
        }
    };
    auto mm = [&](float (&av)[4], float (&bv)[4]) __attribute__((always_inline)) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], bv[0], acc0, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], bv[1], acc1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], bv[2], acc0, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], bv[3], acc1, 0, 0, 0);
    };
    float ca[4], cb[4];
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    rd(lds, lds + BM * BK, c0, ca, cb);
    int buf = 0;
    for (int kt = 0; kt < nst; kt++) {
        const int b1 = buf ^ 1;
        if (kt + 1 < nst) issue(kt + 1, b1);
        else if (RAGK && tail > 0) issue_tail(b1);
        const float *a = lds + buf * STAGE, *b = a + BM * BK;
#pragma unroll
        for (int ci = 0; ci + 1 < NCG; ci++) {
            float na[4], nbv[4];
            rd(a, b, c0 + ci + 1, na, nbv);
            __builtin_amdgcn_sched_barrier(0);
            mm(ca, cb);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 4; j++) { ca[j] = na[j]; cb[j] = nbv[j]; }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        float na[4], nbv[4];
        if (kt + 1 < nst) rd(lds + b1 * STAGE, lds + b1 * STAGE + BM * BK, c0, na, nbv);
        __builtin_amdgcn_sched_barrier(0);
        mm(ca, cb);
        if (kt + 1 < nst) {
#pragma unroll
            for (int j = 0; j < 4; j++) { ca[j] = na[j]; cb[j] = nbv[j]; }
        }
        buf = b1;
    }
    if (RAGK && tail > 0) {                                  // the partial stage sits in `buf`, visible since the last barrier
        const float *a = lds + buf * STAGE, *b = a + BM * BK;
        const int nct = (tail + 7) >> 3;
        auto zf = [&](int c, float (&dv)[4], float (&ev)[4], const float (&av)[4], const float (&bv)[4]) __attribute__((always_inline)) {
            const int k0 = c * 8 + 4 * h;
#pragma unroll
            for (int j = 0; j < 4; j++) { const bool in = k0 + j < tail; dv[j] = in ? av[j] : 0.f; ev[j] = in ? bv[j] : 0.f; }
        };
        int c = kg;
        float ra4[4], rb4[4];
        if (c < nct) { rd(a, b, c, ra4, rb4); zf(c, ca, cb, ra4, rb4); }
        for (; c < nct; c += 2) {
            if (c + 2 < nct) rd(a, b, c + 2, ra4, rb4);
            __builtin_amdgcn_sched_barrier(0);
            mm(ca, cb);
            __builtin_amdgcn_sched_barrier(0);
            if (c + 2 < nct) zf(c + 2, ca, cb, ra4, rb4);
        }
    }
    const int gn = n0 + wn * 32 + l31;
    float add[16];
    // the epilogue's operands (bias, the old C of a beta != 0 product) are requested here, in front of the k-groups' meeting: behind it they
    // were a memory round trip of their own at the very end of a single-wave launch (alpha / beta at 1024^3: 69.5 % of the MFMA peak)
    float bv_ = 0.f, old[16];
    if (EPI && kg == 0) {
        bv_ = p.bias ? p.bias[gn] : 0.f;
        if (p.beta != 0.f) {
#pragma unroll
            for (int r = 0; r < 16; r++) old[r] = p.O[(long)(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * N + gn];
        }
    }
    __syncthreads();
    if (kg == 1) {
#pragma unroll
        for (int r = 0; r < 16; r++) lds[(w4 * 16 + r) * 64 + lane] = acc0[r] + acc1[r];
    }
    __syncthreads();
    if (!PAIR && kg == 1) return;
    if (PAIR) {
        if (kg == 0) {
#pragma unroll
            for (int r = 0; r < 16; r++) add[r] = (acc0[r] + acc1[r]) + lds[(w4 * 16 + r) * 64 + lane];      // this workgroup's K half, complete
        }
        __shared__ int role_s;
        const int tile_id = tm * tiles_n + tn;
        int *ticket = p.sync + tile_id, *flag = p.sync + 2048 + tile_id;
        float *slot = p.part + (long)tile_id * (BM * BN);
        const int t4 = tid & 255;
        if (tid == 0) role_s = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        // agent-scope (cache-bypassing) stores and loads carry the payload: the two workgroups may sit on different XCDs (private L2s)
        if (role_s == 0) {
            if (kg == 0) {
#pragma unroll
                for (int r = 0; r < 16; r++) __hip_atomic_store(&slot[r * 256 + t4], add[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (tid == 0) {
            T4K_SPIN_WAIT(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0, 3);
            __hip_atomic_store(flag, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (kg == 1) return;
#pragma unroll
        for (int r = 0; r < 16; r++) { acc0[r] = add[r]; acc1[r] = 0.f; add[r] = __hip_atomic_load(&slot[r * 256 + t4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) add[r] = lds[(w4 * 16 + r) * 64 + lane];
    }
    if (EPI) {
        const float alpha = p.alpha, beta = p.beta;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int gm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            float o = ((acc0[r] + acc1[r]) + add[r]) * alpha;
            if (beta != 0.f) o += old[r] * beta;
            if (p.bias) o += bv_;
            __builtin_nontemporal_store(o, &p.O[(long)gm * N + gn]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int gm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            __builtin_nontemporal_store((acc0[r] + acc1[r]) + add[r], &p.O[(long)gm * N + gn]);
        }
    }
}
template <bool AKC, bool BKC, bool EPI, bool PAIR = false, bool RAGK = false>
void launch_plain_(const PlainP &q, const GemmPlan &pl, hipStream_t s) {
    constexpr size_t lds_bytes = (size_t)2 * 128 * 128 * sizeof(float);
    const dim3 grid(pl.gx, PAIR ? 2 : 1);
    if (pl.pow2) launch_lds<k_gemm_nn_plain<true, AKC, BKC, EPI, PAIR, RAGK>>(grid, dim3(512), lds_bytes, s, q);
    else         launch_lds<k_gemm_nn_plain<false, AKC, BKC, EPI, PAIR, RAGK>>(grid, dim3(512), lds_bytes, s, q);
}
void launch_nn_plain(const GemmP &p, const GemmPlan &pl, hipStream_t s) {
    PlainP q{ p.A, p.B, p.O, p.M, p.N, p.K, 1.0f, 0.0f, nullptr, nullptr, nullptr };
    launch_plain_<true, false, false>(q, pl, s);
}
// any layout, alpha / beta / bias: interior tiles, K % 128 == 0, unsplit (GR_PLAIN_ANY) - or a K tail (GR_PLAIN_RAGK) - or K % 256 == 0 and two workgroups per tile (GR_PAIR)
void launch_plain_any(const GemmP &p, const GemmPlan &pl, int tA, int tB, hipStream_t s) {
    PlainP q{ p.A, p.B, p.O, p.M, p.N, p.K, p.alpha, p.beta, p.bias, p.sync, p.part };
    q.swap = pl.swap ? 1 : 0;
    with_layout(tA, tB, [&](auto akc, auto bkc, auto epi) {
        if (pl.rung == GR_PLAIN_RAGK) launch_plain_<akc(), bkc(), epi(), false, true>(q, pl, s);
        else if (pl.rung == GR_PAIR)  launch_plain_<akc(), bkc(), epi(), true>(q, pl, s);
        else                          launch_plain_<akc(), bkc(), epi()>(q, pl, s);
    }, pl.epi);
}

// Large outputs (>= ~3/4 of the CUs in 128x128 tiles): the lean pipeline on a 128x128 tile.  Same 8 waves = 2 k-groups x 2x2 waves, but every
// wave owns a 64x64 block (2x2 accumulators of 32x32): one A fragment feeds two MFMAs and so does one B fragment - half the LDS reads and half
// the L2 -> LDS bytes per MFMA of the 64x64 tile, which is what limits that kernel once the fixed costs are amortised (2048^3: 80 %).
// 64-deep double-buffered stages (64 KiB each).  Interior tiles, K % 64 == 0, unsplit; layouts and epilogue as k_gemm_nn_plain.
// RAGK: K >= 256 with a partial last stage (784 = 12 x 64 + 16), as k_gemm_nn_plain<RAGK>: one more DMA stage in which only the lanes inside the
// tail move anything, its 8-deep chunks alternate between the k-groups, positions past the tail zeroed in registers (2048 x 2048 x 784: 58.5 -> measured below).
// BK_ = 32 (round 5): 32-deep stages, 64 KiB of LDS, at most 128 registers - TWO workgroups per CU, each with its own stage barrier, so one's MFMAs fill the pipe
// while the other's waves meet (grids of >= 2 tiles per CU; the 64-deep form keeps one workgroup per CU).
template <bool AKC, bool BKC, bool EPI, bool RAGK = false, int BK_ = 64>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(BK_ == 32 ? 4 : 2, BK_ == 32 ? 4 : 2))) k_gemm_plain128(PlainP p) {
    constexpr int BM = 128, BN = 128, BK = BK_;
    constexpr int NC = BK / 8, CH = BK / 4, NCG = NC / 2;
    constexpr int STAGE = (BM + BN) * BK;
    constexpr int NJ = (BM * BK / 256) / 8;                // 1-KiB DMA instructions per operand per wave per stage (4)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = w >> 2, w4 = w & 3, wm = w4 >> 1, wn = w4 & 1, h = lane >> 5, l31 = lane & 31;
    const int c0 = kg * NCG;
    const int M = p.M, N = p.N, K = p.K;
    const int tiles_m = M / BM, tiles_n = N / BN, T = tiles_m * tiles_n;
    int tm, tn;
    {
        int L;
        { const int b = blockIdx.x, q8 = T >> 3, r8 = T & 7, x = b & 7, i = b >> 3;
          L = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i; }           // XCD x owns a contiguous run of the tile order
        constexpr int GROUP_M = 4;
        const int per_group = GROUP_M * tiles_n;
        const int grp = L / per_group, first_m = grp * GROUP_M;
        const int gsz = min(tiles_m - first_m, GROUP_M);
        tm = first_m + (L % per_group) % gsz; tn = (L % per_group) / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN, nst = K / BK;
    const int tail = RAGK ? K - nst * BK : 0;
    unsigned voffA[NJ], voffB[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int i = w * NJ + j;
        constexpr int RPI = 64 / CH;                       // rows of a K-contiguous operand one 1-KiB DMA instruction covers (CH quads of 16 bytes per row)
        if (AKC) { const int r = i * RPI + lane / CH, q = (lane % CH) ^ (r & (CH - 1)); voffA[j] = (unsigned)((m0 + r) * K + q * 4) * 4u; }
        else     { const int kk = i * 2 + (lane >> 5);                                  voffA[j] = (unsigned)(kk * M + m0 + (lane & 31) * 4) * 4u; }
        if (BKC) { const int r = i * RPI + lane / CH, q = (lane % CH) ^ (r & (CH - 1)); voffB[j] = (unsigned)((n0 + r) * K + q * 4) * 4u; }
        else     { const int kk = i * 2 + (lane >> 5);                                  voffB[j] = (unsigned)(kk * N + n0 + (lane & 31) * 4) * 4u; }
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)lds;
    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        const float *ba = p.A + (AKC ? (long)kt * BK : (long)kt * BK * M), *bb = p.B + (BKC ? (long)kt * BK : (long)kt * BK * N);
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((buf * STAGE + (w * NJ + j) * 256) * 4));
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffA[j]), "s"(ba), "s"(la) : "memory");
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffB[j]), "s"(bb), "s"(la + BM * BK * 4) : "memory");
        }
    };
    auto issue_tail = [&](int buf) __attribute__((always_inline)) {        // stage nst: same lane offsets, lanes past the tail switched off (nothing read out of bounds)
        const float *ba = p.A + (AKC ? (long)nst * BK : (long)nst * BK * M), *bb = p.B + (BKC ? (long)nst * BK : (long)nst * BK * N);
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int i = w * NJ + j;
            const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((buf * STAGE + i * 256) * 4));
            const bool kin = ((((lane % CH) ^ ((i * (64 / CH) + lane / CH) & (CH - 1)))) << 2) < tail, rin = i * 2 + (lane >> 5) < tail;
            if (AKC ? kin : rin) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffA[j]), "s"(ba), "s"(la) : "memory");
            if (BKC ? kin : rin) asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffB[j]), "s"(bb), "s"(la + BM * BK * 4) : "memory");
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
    const int ra_ = wm * 64 + l31, rb_ = wn * 64 + l31;
    auto rd = [&](const float *a, const float *b, int ci, float (&av)[2][4], float (&bv)[2][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int ra = ra_ + t * 32, rb = rb_ + t * 32;
            if (AKC) { const v4f v = *reinterpret_cast<const v4f *>(a + ra * BK + (((ci * 2 + h) ^ (ra & (CH - 1))) << 2));
                       av[t][0] = v[0]; av[t][1] = v[1]; av[t][2] = v[2]; av[t][3] = v[3]; }
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) av[t][j] = a[(ci * 8 + 4 * h + j) * BM + ra];
            }
            if (BKC) { const v4f v = *reinterpret_cast<const v4f *>(b + rb * BK + (((ci * 2 + h) ^ (rb & (CH - 1))) << 2));
                       bv[t][0] = v[0]; bv[t][1] = v[1]; bv[t][2] = v[2]; bv[t][3] = v[3]; }
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) bv[t][j] = b[(ci * 8 + 4 * h + j) * BN + rb];
            }
        }
    };
    auto mm = [&](float (&av)[2][4], float (&bv)[2][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; j++) {                       // four independent accumulators per k step: no MFMA waits on its predecessor
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][j], bv[0][j], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][j], bv[1][j], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][j], bv[0][j], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][j], bv[1][j], acc[1][1], 0, 0, 0);
        }
    };
    float ca[2][4], cb[2][4];
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#if T4K_GEMM_EARLY_ISSUE
    if (nst > 1) issue(1, 1);                              // stage kt + 2 is requested right behind stage kt's closing barrier (its buffer is free from there on)
    else if (RAGK && tail > 0) issue_tail(1);
#endif
    rd(lds, lds + BM * BK, c0, ca, cb);
    int buf = 0;
    for (int kt = 0; kt < nst; kt++) {
        const int b1 = buf ^ 1;
#if !T4K_GEMM_EARLY_ISSUE
        if (kt + 1 < nst) issue(kt + 1, b1);
        else if (RAGK && tail > 0) issue_tail(b1);
#endif
        const float *a = lds + buf * STAGE, *b = a + BM * BK;
#pragma unroll
        for (int ci = 0; ci + 1 < NCG; ci++) {
            float na[2][4], nbv[2][4];
            rd(a, b, c0 + ci + 1, na, nbv);
            __builtin_amdgcn_sched_barrier(0);
            mm(ca, cb);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int j = 0; j < 4; j++) { ca[t][j] = na[t][j]; cb[t][j] = nbv[t][j]; }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#if T4K_GEMM_EARLY_ISSUE
        if (kt + 2 < nst) issue(kt + 2, buf);
        else if (RAGK && tail > 0 && kt + 2 == nst) issue_tail(buf);
#endif
        float na[2][4], nbv[2][4];
        if (kt + 1 < nst) rd(lds + b1 * STAGE, lds + b1 * STAGE + BM * BK, c0, na, nbv);
        __builtin_amdgcn_sched_barrier(0);
        mm(ca, cb);
        if (kt + 1 < nst) {
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int j = 0; j < 4; j++) { ca[t][j] = na[t][j]; cb[t][j] = nbv[t][j]; }
        }
        buf = b1;
    }
    if (RAGK && tail > 0) {                                  // the partial stage sits in `buf`, visible since the last barrier
        const float *a = lds + buf * STAGE, *b = a + BM * BK;
        const int nct = (tail + 7) >> 3;
        for (int c = kg; c < nct; c += 2) {
            float ta[2][4], tb[2][4];
            rd(a, b, c, ta, tb);
            const int k0 = c * 8 + 4 * h;
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int j = 0; j < 4; j++) { if (k0 + j >= tail) { ta[t][j] = 0.f; tb[t][j] = 0.f; } }
            mm(ta, tb);
        }
    }
    // the two k-groups meet in LDS (64 KiB: 4 waves x 64 accumulator registers x 64 lanes), group 0 stores
    __syncthreads();
    if (kg == 1) {
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) lds[((w4 * 4 + a * 2 + b) * 16 + r) * 64 + lane] = acc[a][b][r];
    }
    __syncthreads();
    if (kg == 1) return;
    const float alpha = EPI ? p.alpha : 1.f, beta = EPI ? p.beta : 0.f;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int gn = n0 + wn * 64 + b * 32 + l31;
            const float bsv = (EPI && p.bias) ? p.bias[gn] : 0.f;
            float old[16];
            if (EPI && beta != 0.f) {                        // all 16 loads of the block in flight before the first store (a store ahead of a may-alias load serialises them)
#pragma unroll
                for (int r = 0; r < 16; r++) old[r] = p.O[(long)(m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * N + gn];
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int gm = m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                float o = acc[a][b][r] + lds[((w4 * 4 + a * 2 + b) * 16 + r) * 64 + lane];
                if (EPI) { o *= alpha; if (beta != 0.f) o += old[r] * beta; o += bsv; }
                __builtin_nontemporal_store(o, &p.O[(long)gm * N + gn]);
            }
        }
}
template <bool AKC, bool BKC, bool EPI, bool RAGK = false, int BK_ = 64>
void launch_plain128_(const PlainP &q, unsigned gx, hipStream_t s) {
    launch_lds<k_gemm_plain128<AKC, BKC, EPI, RAGK, BK_>>(dim3(gx), dim3(512), (size_t)2 * 256 * BK_ * sizeof(float), s, q);
}

// 256 x 256 tile, 16 waves (round 5): for outputs of at least one such tile per CU (4096^2 and up).  The 128 x 128 kernel pays its stage barrier once per 8 192 MFMA
// cycles of a SIMD (two waves); here sixteen waves - a 4 x 4 grid of 64 x 64 blocks, no k-groups, no meeting in LDS at the end - put 16 384 cycles of MFMAs behind every
// barrier on 32-deep stages of the same 64 KiB, and a stage moves half the bytes per flop (512 rows for 256 x 256 outputs).  126 registers: four waves per SIMD.
// Interior tiles, K % 32 == 0; layouts and epilogue as k_gemm_plain128.
template <bool AKC, bool BKC, bool EPI>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4))) k_gemm_plain256(PlainP p) {
    constexpr int BM = 256, BN = 256, BK = 32;
    constexpr int NC = BK / 8, CH = BK / 4, RPI = 64 / CH;
    constexpr int STAGE = (BM + BN) * BK;
    constexpr int NJ = (BM * BK / 256) / 16;               // 1-KiB DMA instructions per operand per wave per stage (2)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 2, wn = w & 3, h = lane >> 5, l31 = lane & 31;
    const int M = p.M, N = p.N, K = p.K;
    const int tiles_m = M / BM, tiles_n = N / BN, T = tiles_m * tiles_n;
    int tm, tn;
    {
        int L;
        { const int b = blockIdx.x, q8 = T >> 3, r8 = T & 7, x = b & 7, i = b >> 3;
          L = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i; }           // XCD x owns a contiguous run of the tile order
        constexpr int GROUP_M = 4;
        const int per_group = GROUP_M * tiles_n;
        const int grp = L / per_group, first_m = grp * GROUP_M;
        const int gsz = min(tiles_m - first_m, GROUP_M);
        tm = first_m + (L % per_group) % gsz; tn = (L % per_group) / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN, nst = K / BK;
    unsigned voffA[NJ], voffB[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int i = w * NJ + j;
        if (AKC) { const int r = i * RPI + lane / CH, q = (lane % CH) ^ (r & (CH - 1)); voffA[j] = (unsigned)((m0 + r) * K + q * 4) * 4u; }
        else     {                                                                      voffA[j] = (unsigned)(i * M + m0 + lane * 4) * 4u; }     // one k row of 256 floats per instruction
        if (BKC) { const int r = i * RPI + lane / CH, q = (lane % CH) ^ (r & (CH - 1)); voffB[j] = (unsigned)((n0 + r) * K + q * 4) * 4u; }
        else     {                                                                      voffB[j] = (unsigned)(i * N + n0 + lane * 4) * 4u; }
    }
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void *)lds;
    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        const float *ba = p.A + (AKC ? (long)kt * BK : (long)kt * BK * M), *bb = p.B + (BKC ? (long)kt * BK : (long)kt * BK * N);
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const unsigned la = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)((buf * STAGE + (w * NJ + j) * 256) * 4));
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffA[j]), "s"(ba), "s"(la) : "memory");
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voffB[j]), "s"(bb), "s"(la + BM * BK * 4) : "memory");
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
    const int ra_ = wm * 64 + l31, rb_ = wn * 64 + l31;
    auto rd = [&](const float *a, const float *b, int ci, float (&av)[2][4], float (&bv)[2][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int ra = ra_ + t * 32, rb = rb_ + t * 32;
            if (AKC) { const v4f v = *reinterpret_cast<const v4f *>(a + ra * BK + (((ci * 2 + h) ^ (ra & (CH - 1))) << 2));
                       av[t][0] = v[0]; av[t][1] = v[1]; av[t][2] = v[2]; av[t][3] = v[3]; }
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) av[t][j] = a[(ci * 8 + 4 * h + j) * BM + ra];
            }
            if (BKC) { const v4f v = *reinterpret_cast<const v4f *>(b + rb * BK + (((ci * 2 + h) ^ (rb & (CH - 1))) << 2));
                       bv[t][0] = v[0]; bv[t][1] = v[1]; bv[t][2] = v[2]; bv[t][3] = v[3]; }
            else {
#pragma unroll
                for (int j = 0; j < 4; j++) bv[t][j] = b[(ci * 8 + 4 * h + j) * BN + rb];
            }
        }
    };
    auto mm = [&](float (&av)[2][4], float (&bv)[2][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][j], bv[0][j], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][j], bv[1][j], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][j], bv[0][j], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][j], bv[1][j], acc[1][1], 0, 0, 0);
        }
    };
    // four waves per SIMD: a wave reads a chunk's fragments and multiplies them - while it waits for LDS the other three keep the MFMA pipe busy, so no
    // second fragment set is carried (with it the kernel spills, and a compiler-counted scratch reload waits for vmcnt(0), i.e. for the DMA of the NEXT stage)
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (nst > 1) issue(1, 1);
    int buf = 0;
    for (int kt = 0; kt < nst; kt++) {
        const float *a = lds + buf * STAGE, *b = a + BM * BK;
#pragma unroll
        for (int ci = 0; ci < NC; ci++) {
            float ca[2][4], cb[2][4];
            rd(a, b, ci, ca, cb);
            mm(ca, cb);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (kt + 2 < nst) issue(kt + 2, buf);
        buf ^= 1;
    }
    const float alpha = EPI ? p.alpha : 1.f, beta = EPI ? p.beta : 0.f;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int gn = n0 + wn * 64 + b * 32 + l31;
            const float bsv = (EPI && p.bias) ? p.bias[gn] : 0.f;
            float old[16];
            if (EPI && beta != 0.f) {
#pragma unroll
                for (int r = 0; r < 16; r++) old[r] = p.O[(long)(m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * N + gn];
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int gm = m0 + wm * 64 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                float o = acc[a][b][r];
                if (EPI) { o *= alpha; if (beta != 0.f) o += old[r] * beta; o += bsv; }
                __builtin_nontemporal_store(o, &p.O[(long)gm * N + gn]);
            }
        }
}
template <bool AKC, bool BKC, bool EPI>
void launch_plain256_(const PlainP &q, unsigned gx, hipStream_t s) {
    launch_lds<k_gemm_plain256<AKC, BKC, EPI>>(dim3(gx), dim3(1024), (size_t)2 * 512 * 32 * sizeof(float), s, q);
}
void launch_plain128(const GemmP &p, const GemmPlan &pl, int tA, int tB, hipStream_t s) {
    PlainP q{ p.A, p.B, p.O, p.M, p.N, p.K, p.alpha, p.beta, p.bias, nullptr, nullptr };
    with_layout(tA, tB, [&](auto akc, auto bkc, auto e) {
        if (pl.rung == GR_PLAIN256)           launch_plain256_<akc(), bkc(), e()>(q, pl.gx, s);
        else if (pl.rung == GR_PLAIN128_BK32) launch_plain128_<akc(), bkc(), e(), false, 32>(q, pl.gx, s);
        else if (pl.rung == GR_PLAIN128_RAGK) launch_plain128_<akc(), bkc(), e(), true>(q, pl.gx, s);
        else                                  launch_plain128_<akc(), bkc(), e()>(q, pl.gx, s);
    }, pl.epi);
}

// RAGK: K with a partial last stage
template <int BK, bool RAGK = false>
void launch_glds8(const GemmP &p, dim3 grid, int tA, int tB, hipStream_t s) {
    constexpr size_t lds_bytes = (size_t)((BK >= 128) ? 2 : 3) * 128 * BK * sizeof(float);
    with_layout(tA, tB, [&](auto akc, auto bkc) { launch_lds<k_gemm_glds8<BK, akc(), bkc(), false, RAGK>>(grid, dim3(512), lds_bytes, s, p); });
}

// fold split-K slabs in slice order, then the alpha/beta epilogue (reference t4math.cu:580)
// Optional activation epilogue (the layer that follows a linear layer: relu / tanh / ... / dropout): O keeps the linear
// output, ACT_O / ACT_F receive the activation output and derivative mask (k_activate nmath.cu:37-70); dropout draws its
// Philox slice here, exactly the values t4k_rand would have stored in the mask tensor.
// Riders of the fold launch: a second element-wise layer behind the first (the run `leakyrelu dropout` of the GAN nets), and a plain
// copy done by cp_blocks extra workgroups (the model's copy of the batch into its layer 0, forward.cu:39, rides with the first
// linear layer's fold instead of taking a launch of its own).
__global__ void __launch_bounds__(BLK) k_splitk_fold(const float *__restrict__ part, float *O, long mn, int nsplit,
                                                     float alpha, float beta, const float *__restrict__ bias, int N, ActEpi ep, FoldRider fr) {
    uint64_t base = 0, seed = 0;
    const ActEpi &ep2 = fr.ep2;
    const bool draw1 = ep.layer == T4K_L_DROPOUT, draw2 = ep2.layer == T4K_L_DROPOUT;      // at most one of the two (one dropout per run)
    const RngArg &rg = draw2 ? ep2.rng : ep.rng;
    if (draw1 || draw2) rng_begin(rg, base, seed);
    const int nfold = (int)gridDim.x - fr.cp_blocks;
    if ((int)blockIdx.x >= nfold) {
        const long t0 = (long)((int)blockIdx.x - nfold) * BLK + threadIdx.x, step = (long)fr.cp_blocks * BLK;
        if (fr.cp_vec) {
            const long n4 = fr.cp_n >> 2;
            for (long z = t0; z < n4; z += step) reinterpret_cast<float4 *>(fr.cp_dst)[z] = reinterpret_cast<const float4 *>(fr.cp_src)[z];
            for (long z = (n4 << 2) + t0; z < fr.cp_n; z += step) fr.cp_dst[z] = fr.cp_src[z];
        } else
            for (long z = t0; z < fr.cp_n; z += step) fr.cp_dst[z] = fr.cp_src[z];
    } else
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < mn; z += (long)nfold * BLK) {
        float s = 0.f;
#pragma unroll 4
        for (int k = 0; k < nsplit; k++) s += part[(long)k * mn + z];
        float o = s * alpha;
        if (beta != 0.f) o += O[z] * beta;
        if (bias) o += bias[z % N];
        O[z] = o;
        if (fr.mc.d1) { const float g1 = o * fr.mc.m1[z]; fr.mc.d1[z] = g1; if (fr.mc.d2) fr.mc.d2[z] = g1 * fr.mc.m2[z]; }
        if (ep.layer) {
            float a, f; act_rt(ep.layer, o, draw1 ? philox_u01_at(base, seed, z) : 0.f, ep.alpha, a, f); ep.F[z] = f; ep.A[z] = a;
            if (ep2.layer) { float a2, f2; act_rt(ep2.layer, a, draw2 ? philox_u01_at(base, seed, z) : 0.f, ep2.alpha, a2, f2); ep2.F[z] = f2; ep2.A[z] = a2; }
        }
    }
    if ((draw1 || draw2) && rg.state) rng_advance_last_block(rg.state, base, (uint64_t)((mn + 3) >> 2));
}

// words gemm1/gemm2 (k_gemm src/t4math.cu:370, k_gemm_claude :411): double accumulator
__global__ void __launch_bounds__(BLK) k_gemm_f64(const float *__restrict__ A, const float *__restrict__ B, float *O,
                                                  float alpha, float beta, int M, int N, int K, int C) {
    const long total = (long)M * N * C;
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < total; z += (long)gridDim.x * BLK) {
        const int c = (int)(z % C); const long mn = z / C; const int n = (int)(mn % N), m = (int)(mn / N);
        double acc = 0.0;
        for (int k = 0; k < K; k++) acc += (double)(A[((long)m * K + k) * C + c] * B[((long)k * N + n) * C + c]);
        O[z] = (float)(alpha * acc + (beta == 0.f ? 0.0 : (double)(beta * O[z])));
    }
}

template <int BM, int BN, int BK, bool VEC, bool SKEW, bool FULL>
void launch_variant(const GemmP &p, dim3 grid, int tA, int tB, hipStream_t s) {
    with_layout(tA, tB, [&](auto akc, auto bkc) {
        launch_lds<k_gemm_mfma<BM, BN, BK, akc(), bkc(), VEC, SKEW, FULL>>(grid, dim3(256), (size_t)2 * (BM + BN) * BK * sizeof(float), s, p);
    });
}

// the column-sum rider (GemmP::cs_*) goes with a launch whose every tile is written by one workgroup (GemmPlan::cs_rides; its cs_wgs workgroups are in the plan's grid)
void take_colsum(GemmP &p, ColSum *cs) {
    p.cs_X = cs->X; p.cs_out = cs->out; p.cs_rows = cs->rows; p.cs_E = cs->E; cs->done = true;
}
// The riders of a GEMM's last launch - the sliver kernel's epilogue or the split-K fold: the activation behind a linear layer (ep), a second
// stage behind it (fr.ep2), the mask chain and the layer-0 copy, the latter on at most cp_max extra workgroups of cp_per elements per thread.
// Called only when the launch will really apply them: a dropout stage reserves its Philox slice here, ep first, then ep2 - the masks'
// positions depend on that order.  Reports to the caller through epi_done, rider->mc_done and rider->cp_blocks.
struct Riders { ActEpi ep; FoldRider fr; };
Riders make_riders(hipStream_t hs, long mn, const ActEpi *epi, bool *epi_done, FoldRider *rider, int cp_per, int cp_max) {
    Riders r = { ActEpi{0, 0.f, nullptr, nullptr, RngArg{0, 0, nullptr}}, FoldRider{} };
    if (epi && epi->layer) {
        r.ep = *epi; if (epi_done) *epi_done = true;
        if (r.ep.layer == T4K_L_DROPOUT) r.ep.rng = rng_draw(hs, (uint64_t)((mn + 3) >> 2), true);
        if (rider && rider->ep2.layer) {
            r.fr.ep2 = rider->ep2;
            if (r.fr.ep2.layer == T4K_L_DROPOUT) r.fr.ep2.rng = rng_draw(hs, (uint64_t)((mn + 3) >> 2), true);
        }
    }
    if (rider && rider->mc.d1) { r.fr.mc = rider->mc; rider->mc_done = 1; }
    if (rider && rider->cp_src && rider->cp_dst && rider->cp_n > 0) {
        r.fr.cp_src = rider->cp_src; r.fr.cp_dst = rider->cp_dst; r.fr.cp_n = rider->cp_n; r.fr.cp_vec = aligned16(r.fr.cp_src) && aligned16(r.fr.cp_dst);
        r.fr.cp_blocks = std::min(grid_for(rider->cp_n, cp_per), cp_max);
        rider->cp_blocks = r.fr.cp_blocks;
    }
    return r;
}

// ------------------------------------------------------------------------------------------
// Batched products of large matrices (t4k_gemm_batched, gemm_batched.hip): the tile kernel above, one output tile of one batch entry per
// workgroup - grid = (tiles, batch entries, channels).  Operand b sits at A + b * sA (sA == 0: one A for every entry), likewise B and O.
// Entries beyond the 65535 of grid.y are walked by the same workgroups.  Split-K, riders and the gates stay off (nsplit = 1).
template <int BM, int BN, int BK, bool AKC, bool BKC, bool VEC, bool SKEW, bool FULL>
__global__ void __launch_bounds__(256) k_gemm_mfma_batched(GemmP p, long sA, long sB, long sO, int batch) {
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        GemmP q = p;
        q.A += b * sA; q.B += b * sB; q.O += b * sO;
        gemm_mfma_body<BM, BN, BK, AKC, BKC, VEC, SKEW, FULL>(q, blockIdx.x, 0, blockIdx.z);
        __syncthreads();                                   // the next entry's first stage overwrites LDS
    }
}
template <int BM, int BN, int BK, bool VEC, bool SKEW, bool FULL>
void launch_batched(const GemmP &p, dim3 grid, int tA, int tB, long sA, long sB, long sO, int batch, hipStream_t s) {
    with_layout(tA, tB, [&](auto akc, auto bkc) {
        launch_lds<k_gemm_mfma_batched<BM, BN, BK, akc(), bkc(), VEC, SKEW, FULL>>(grid, dim3(256), (size_t)2 * (BM + BN) * BK * sizeof(float), s, p, sA, sB, sO, batch);
    });
}

// ------------------------------------------------------------------------------------------
// The dispatch ladder as a pure function: no launch, no HIP call, no global state beyond gemm_lab().  Every product in it is formed in long / size_t.
GemmPlan gemm_plan(const GemmAsk &q, const GemmEnv &e) {
    const GemmLab &lab = gemm_lab();
    const int M = q.M, N = q.N, K = q.K, C = q.C, tA = q.tA, tB = q.tB, cu = e.cu;
    const long Kl = K;                                   // the round-ups of K are formed in long: K + 63 may pass INT_MAX
    GemmPlan pl;
    if (M == 0 || N == 0) return pl;                     // GR_NONE: nothing to launch
    pl.launches = 1;
    if (K == 0) {
        // an empty product: O = alpha 0 + beta O (+ bias) on the fold kernel with no slab to add.  The ladder below would reach a K-loop kernel, and the lean
        // ones (k_gemm_nn_plain, which a large plain product takes at K % 128 == 0) issue their first stage's DMA before they look at the stage count:
        // 64 rows of an operand that has no byte to read
        pl.rung = GR_K0; pl.gx = (unsigned)grid_for((long)M * N * C);
        return pl;
    }
    const bool aligned = q.a16 && q.b16;
    const bool cs_ok = q.cs && q.cs_rows > 0 && q.cs_rows <= 4096 && q.cs_E > 0;
    const unsigned cs_wgs = cs_ok ? (unsigned)((q.cs_E + 63) / 64) : 0;      // the column-sum rider's workgroups, where a launch carries it
    pl.epi = !q.plain || q.bias;

    // 16-byte loads need: C == 1, aligned bases, contiguous extents divisible by 4
    const int a_contig = tA ? M : K, b_contig = tB ? K : N;
    const bool vec = (C == 1) && aligned && (a_contig % 4 == 0) && (b_contig % 4 == 0);

    const bool big = gemm_big(M, N, cu);
    const int BMv = big ? 128 : 64;
    pl.tiles_m = (M + BMv - 1) / BMv; pl.tiles_n = (N + BMv - 1) / BMv;
    const long tiles = (long)pl.tiles_m * pl.tiles_n;
    const bool dma32 = span32(M, N, K);                  // the LDS-DMA kernels' 32-bit lane offsets reach both operands
    const bool interior64 = M % 64 == 0 && N % 64 == 0;  // no ragged 64x64 tile
    // the lean 64x64 kernel's tile prologue and tile order (k_gemm_nn_plain<POW2>, PlainP::swap)
    const int tmq = M / 64, tnq = N / 64;
    pl.pow2 = lab.fastpro && (tmq & (tmq - 1)) == 0 && (tnq & (tnq - 1)) == 0 && tmq >= 4 && ((long)tmq * tnq) % 32 == 0;
    pl.swap = lab.tt_swap && tA && tB;

    // Slivers (the output gives at most half the CUs a 64x64 tile, K moderate): 32x32 tiles, K split over the waves, operand blocks through
    // LDS-DMA, the whole epilogue (bias, activation riders, mask chain, layer-0 copy, column sums) in the same launch - no fold
    {
        const bool akc = !tA, bkc = tB != 0;
        const bool al = (!akc || (K % 4 == 0 && q.a16)) && (!bkc || (K % 4 == 0 && q.b16));
        const long t32 = (long)((M + 31) / 32) * ((N + 31) / 32);
        int ns = 1, kc = (int)((Kl + 7) / 8 * 8);
        if (q.defer && q.plain && K >= 256) {               // a consumer folds the slabs anyway: spread K over idle CUs
            int want = (int)((cu + t32 - 1) / t32); if (want > K / 128) want = K / 128; if (want > 16) want = 16;
            if (want > 1) { kc = (int)((((Kl + want - 1) / want) + 7) / 8 * 8); ns = (int)((Kl + kc - 1) / kc); }
            if ((size_t)ns * M * N * sizeof(float) > e.ws_bytes / 2) { ns = 1; kc = (int)((Kl + 7) / 8 * 8); }
        }
        // operands through LDS-DMA blocks: every 16-byte DMA lane aligned and whole (other shapes: the 64x64 kernels below)
        const bool dma_ok = e.d_zero && aligned && (akc ? K % 4 == 0 : M % 4 == 0) && (bkc ? K % 4 == 0 : N % 4 == 0);
        if (lab.s32 && C == 1 && !big && tiles * 2 <= cu && K >= 1 && kc <= lab.s32_maxk && al && dma_ok && !e.capturing) {   // kc: depth one workgroup walks
            pl.tiles_m = (M + 31) / 32; pl.tiles_n = (N + 31) / 32;
            pl.kchunk = kc; pl.nsplit = ns;
            const bool last = ns == 1;                 // this launch finishes the product and carries its riders; split slabs (a deferred fold) carry none
            pl.cs_rides = cs_ok && last; pl.cs_wgs = pl.cs_rides ? cs_wgs : 0;
            pl.gx = (unsigned)t32 + pl.cs_wgs; pl.gy = (unsigned)ns;
            pl.riders = last ? RIDE_LAUNCH : RIDE_NONE; pl.deferred = !last;
            pl.xmap = (lab.xmap && t32 >= 16) ? (N >= M ? 2 : 1) : 0;       // XCD-aware tile order: an XCD's L2 pulls its own slice of the wider operand only
            const int nblk = (kc + 31) / 32;
            // waves per workgroup (= k-groups) and whether a wave walks more than two blocks (RST: blocks 2, 3 wait in registers)
            pl.w8 = nblk > 16 || (nblk >= 6 && t32 * ns <= (long)cu);
            pl.rst = nblk > (pl.w8 ? 16 : 8);
            pl.rung = pl.w8 ? (pl.rst ? GR_L32_W8_RST : GR_L32_W8) : (pl.rst ? GR_L32_W4_RST : GR_L32_W4);
            return pl;
        }
    }
    // 65..128 interior tiles, K in whole 256s: two workgroups per tile on the lean kernel, combined in its epilogue (k_gemm_nn_plain<.., PAIR>) -
    // 512 x 1024 x 1024: one launch instead of split-K slabs + a fold launch.  Tickets are per tile: default stream only.
    if (lab.plain_pair && e.gates && !big && vec && C == 1 && interior64 && K % 256 == 0 && K >= 512 &&
        tiles * 2 <= cu && tiles * 3 > cu && tiles <= 2048 && !q.defer && !q.riders && !q.cs &&
        e.d_sync && e.lane == 0 && (size_t)tiles * 4096 * sizeof(float) <= e.ws_bytes / 2 && dma32) {
        pl.rung = GR_PAIR; pl.kchunk = K; pl.gx = (unsigned)tiles;
        return pl;
    }
    // split K when the output alone cannot fill the chip (granularity = the deepest stage, 64)
    constexpr int KG = 64;
    int nsplit = 1, kchunk = (int)((Kl + KG - 1) / KG * KG); if (kchunk == 0) kchunk = KG;
    if (!big && C == 1 && gemm_splits(tiles, K, cu)) {
        int want = (int)((cu + tiles - 1) / tiles);
        int maxs = K / (lab.split_div * KG); if (want > maxs) want = maxs; if (want > 64) want = 64;
        if (want > 1) {
            kchunk = (int)((((Kl + want - 1) / want) + KG - 1) / KG * KG);
            nsplit = (int)((Kl + kchunk - 1) / kchunk);
            if ((size_t)nsplit * M * N * sizeof(float) > e.ws_bytes / 2) { nsplit = 1; kchunk = (int)((Kl + KG - 1) / KG * KG); }
        }
    }
    pl.kchunk = kchunk; pl.nsplit = nsplit;
    const bool whole_k = kchunk % 64 == 0 && K % kchunk == 0;   // every K slice is whole 64-deep stages

    // ragged M / N with whole K stages on the 8-wave LDS-DMA kernel (clamped source rows, predicated stores) when the K loop is long enough
    // to matter: unsplit products (N = 1000 classes: 1024 x 1000 x 4096 122 -> measured below) - split slivers stay with the skewed kernel
    const bool ragged8 = lab.ragged_dma && !big && vec && C == 1 && nsplit == 1 && !interior64 && whole_k && M >= 4 && N >= 4 && dma32;
    // ragged K (784 = 28 x 28, the GAN layer width; any K when no operand is K-contiguous): the same kernel with a partial last stage
    // (k_gemm_glds8<.., RAGK>) instead of the predicated register-staged one (1024 x 1024 x 784: 28.5 us there).  T4K_GEMM_RAGGED_K: 0 off,
    // 1 unsplit products (default), 2 split-K slabs too
    const bool ragk = lab.ragged_k && !big && vec && C == 1 && !whole_k && (nsplit == 1 || lab.ragged_k >= 2) && M >= 4 && N >= 4 && K >= 8 && dma32;
    {   // column-sum rider: only the generic kernel carries it, and only when one workgroup per tile writes the output
        const bool full64 = !big && vec && interior64 && whole_k;
        const bool generic = big || !vec || !(full64 || ragged8 || ragk);
        pl.cs_rides = cs_ok && generic && nsplit == 1 && C == 1; pl.cs_wgs = pl.cs_rides ? cs_wgs : 0;
    }
    pl.gx = (unsigned)tiles + pl.cs_wgs; pl.gy = (unsigned)nsplit; pl.gz = (unsigned)C;      // the grid of the generic and the split kernels
    pl.deferred = nsplit > 1 && q.defer && q.plain;      // the consumer folds the slabs (fused head)
    pl.fold = nsplit > 1 && !pl.deferred;
    if (pl.fold) { pl.riders = RIDE_FOLD; pl.launches = 2; }
    auto fill_of = [](long tiles_, long cu_) { return (double)tiles_ / (double)(((tiles_ + cu_ - 1) / cu_) * cu_); };
    const long t128i = (long)(M / 128) * (N / 128), t64i = gemm_tiles64(M, N);
    const unsigned g64i = (unsigned)((long)(M / 64) * (N / 64));     // interior 64x64 tiles, one workgroup each
    auto one_launch = [&](GemmRung r, unsigned gx) { pl.rung = r; pl.gx = gx; pl.gy = pl.gz = 1; pl.kchunk = K; pl.nsplit = 1; };   // the lean rungs: unsplit, a tile per workgroup
    const bool lean = vec && C == 1 && nsplit == 1 && !pl.cs_rides && dma32;   // what every lean LDS-DMA kernel asks for besides its tile shape and K stages
    if (lab.plain128 > 0 && lean && M % 128 == 0 && N % 128 == 0 && (K % 64 == 0 || (lab.plain128_ragk && lab.ragged_k && K % 4 == 0)) && K >= 256 &&
        (lab.plain128 >= 2 || (t128i >= cu && fill_of(t128i, cu) * 1.035 > fill_of(t64i, cu)))) {
        // one 256 x 256 tile or more per CU: the 16-wave kernel (T4K_GEMM_PLAIN256: 0 off, 1 default, 2 any grid of whole 256-tiles)
        const int p256 = lab.plain256;
        const long t256 = (long)(M / 256) * (N / 256), t128 = 4 * t256;
        // Two co-resident workgroups per CU on 32-deep stages once every CU gets at least two tiles (4096^2 x 1024: 261 -> 254 us, 8192 x 4096 x 512: 282 -> 264 us;
        // with one tile per CU the doubled barrier count loses: 2048^3 129.5 -> 135.4 us).  K in whole 32s is unragged for this form.  T4K_GEMM_PLAIN128_BK32 = 0 / 1 / 2 (always).
        const int bk32 = lab.plain128_bk32;
        // wave quantisation: 4352^2 is 289 tiles of 256^2 - two rounds, the second 13 % full - but 1156 tiles of 128^2 at 90 % fill; the 256-tile pipeline is worth ~4 % per FLOP
        if (p256 && M % 256 == 0 && N % 256 == 0 && K % 32 == 0 && K >= 64 && (p256 >= 2 || (t256 >= cu && fill_of(t256, cu) * 1.04 > fill_of(t128, cu))) &&
            (long)M * K < (1L << 30) && (long)N * K < (1L << 30)) one_launch(GR_PLAIN256, (unsigned)t256);
        else if (bk32 && K % 32 == 0 && (bk32 >= 2 || t128i >= 2L * cu)) one_launch(GR_PLAIN128_BK32, (unsigned)t128i);
        else one_launch(K % 64 != 0 ? GR_PLAIN128_RAGK : GR_PLAIN128, (unsigned)t128i);
    } else if (lab.plain_ragk && lab.ragged_k && lean && interior64 && K > 128 && K % 128 != 0 && (lab.plain_ragk >= 2 || K % 64 != 0)) {
        // interior tiles, unsplit, K >= 128 with a partial last stage: the lean kernel with a tail (any size of output)
        one_launch(GR_PLAIN_RAGK, g64i);
    } else if (big && lab.plain_big && vec && C == 1 && !tA && !tB && q.plain && !q.bias && !pl.cs_rides && interior64 && K % 128 == 0 && dma32) {
        pl.rung = GR_NN_PLAIN; pl.gx = g64i; pl.gy = pl.gz = 1;     // large plain products on the 64x64 LDS-DMA kernel, several tiles per CU
    } else if (big && lab.plain_any >= 2 && lean && interior64 && K % 128 == 0) {
        pl.rung = GR_PLAIN_ANY; pl.gx = g64i; pl.gy = pl.gz = 1;    // large interior products of every layout on the lean kernel (2048^2 x 1024 linear + bias: 86 -> 72 us vs the 128x128 register-staged kernel)
    } else if (big && lab.big_dma != 0 && e.gates && lean && K % 64 == 0 && K >= 2048 && M >= 4 && N >= 4) {   // deep K only: at K = 1024 the 128x128 kernel's fewer, fatter tiles win (292 vs 318 us at 4096 x 4096 x 1024)
        // every other large product (transposed operands, alpha / beta / bias: the linear layers of an MLP) on the 8-wave LDS-DMA kernel too,
        // 64x64 tiles, several per CU, ragged edges clamped (the 128x128 register-staged kernel: 69-78 % of peak)
        pl.tiles_m = (M + 63) / 64; pl.tiles_n = (N + 63) / 64;
        one_launch(K % 128 == 0 ? GR_GLDS8_128 : GR_GLDS8_64, (unsigned)(pl.tiles_m * pl.tiles_n));
    } else if (big) {
        // whole K stages are enough for the predicate-free pipeline: ragged M / N edges are clamped source rows + predicated stores
        const bool full = vec && kchunk % 32 == 0 && K % kchunk == 0 && M >= 4 && N >= 4 && (lab.big_fullk || (M % 128 == 0 && N % 128 == 0));
        pl.rung = full ? GR_MFMA128_FULL : vec ? GR_MFMA128_SKEW : GR_MFMA128;
    } else if (!vec) {
        pl.rung = GR_MFMA64_32;
    } else if (ragk) {
        pl.rung = (K >= 128 && (nsplit == 1 || kchunk % 128 == 0)) ? GR_GLDS8_128_RAGK : GR_GLDS8_64_RAGK;
    } else if (ragged8) {
        pl.rung = kchunk % 128 == 0 ? GR_GLDS8_128 : GR_GLDS8_64;
    } else if (interior64 && whole_k) {
        if (!dma32) pl.rung = GR_MFMA64_FULL;          // operands of 4 GiB and more: the register-staged kernel (64-bit addresses)
        else if (kchunk % 128 == 0 && !tA && !tB && nsplit == 1 && q.plain && !q.bias) pl.rung = GR_NN_PLAIN;   // `matmul`
        else if (lab.plain_any != 0 && kchunk % 128 == 0 && nsplit == 1) pl.rung = GR_PLAIN_ANY;   // the other layouts, alpha / beta / bias: the same lean kernel
        else pl.rung = kchunk % 128 == 0 ? GR_GLDS8_128 : GR_GLDS8_64;   // split-K slabs of whole 128-deep stages, or 64-deep
    } else {
        const int am = tA ? M : K, bn = tB ? K : N;     // the contiguous extents hold at least one 16-byte group (vec) - the clamp needs M, N >= 4 on the non-K-contiguous side
        pl.rung = (lab.fullk && whole_k && M >= 4 && N >= 4 && am >= 4 && bn >= 4) ? GR_MFMA64_FULL : GR_MFMA64_SKEW;   // ragged M / N, whole K stages: the full form
    }
    return pl;
}
void plan_text(char *text, size_t n, int rung, int nsplit, bool fold) {       // t4k_gemm_last_plan / t4k_gemm_plan: "rung", "xN" for N split-K slabs, "+fold"
    int k = snprintf(text, n, "%s", rung_text[rung >= 0 && rung < GR_COUNT ? rung : 0]);
    if (nsplit > 1 && k < (int)n) k += snprintf(text + k, n - k, "x%d", nsplit);
    if (fold && k < (int)n) snprintf(text + k, n - k, "+fold");
}

} // namespace

namespace t4k {

int gemm_launch(const float *A, const float *B, float *O, const float *bias, float alpha, float beta,
                int tA, int tB, int M, int N, int K, int C, t4k_stream_t s, const ActEpi *epi, bool *epi_done,
                ColSum *cs, XFold *defer, FoldRider *rider) {
    if (epi_done) *epi_done = false;
    if (defer) defer->part = nullptr;
    if (!A || !B || !O || M < 0 || N < 0 || K < 0 || C < 1) return fail(T4K_ERR_ARG, "t4k_gemm: bad argument");
    // 1. the environment
    State &g = st();
    hipStream_t hs = S(s);
    const GemmEnv env{ g.cu_count, g.ws_bytes, g.d_zero != nullptr, g.d_sync != nullptr, gates_ok(), lane_of(hs), capturing(hs) };
    const GemmAsk ask{ M, N, K, C, tA, tB, aligned16(A), aligned16(B), alpha == 1.0f && beta == 0.0f, bias != nullptr,
                       (epi && epi->layer) || rider, defer != nullptr, cs != nullptr, cs ? cs->rows : 0, cs ? cs->E : 0 };
    // 2. the plan
    const GemmPlan pl = gemm_plan(ask, env);
    g.gemm_last = { pl.rung, pl.nsplit, pl.fold };
    if (pl.rung == GR_NONE) return T4K_OK;
    // 3. run it
    const long mn = (long)M * N;
    const ActEpi no_epi{0, 0.f, nullptr, nullptr, RngArg{0, 0, nullptr}};
    GemmP p;
    p.A = A; p.B = B; p.O = O; p.bias = bias; p.part = ws_for(s);
    p.M = M; p.N = N; p.K = K; p.C = C; p.alpha = alpha; p.beta = beta; p.sync = g.d_sync;
    p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.kchunk = pl.kchunk; p.nsplit = pl.nsplit; p.xmap = pl.xmap;
    if (pl.cs_rides) take_colsum(p, cs);
    const dim3 grid(pl.gx, pl.gy, pl.gz);
    switch (pl.rung) {
    case GR_K0:
        T4K_LAUNCH(k_splitk_fold, grid, dim3(BLK), 0, hs, p.part, O, mn * C, 0, alpha, beta, bias, N, no_epi, FoldRider{});
        break;
    case GR_L32_W4: case GR_L32_W4_RST: case GR_L32_W8: case GR_L32_W8_RST: {
        // the last launch of the product carries its riders; split slabs (a deferred fold) carry none
        const bool last = pl.riders == RIDE_LAUNCH;
        const Riders r = make_riders(hs, mn, last ? epi : nullptr, epi_done, last ? rider : nullptr, 16, 128);
        p.Z = g.d_zero;
        with_layout(tA, tB, [&](auto a, auto b, auto w, auto rs) { launch_l32<a(), b(), w() ? 8 : 4, rs()>(p, r.ep, r.fr, dim3(pl.gx + (unsigned)r.fr.cp_blocks, pl.gy), hs); }, pl.w8, pl.rst);
        break;
    }
    case GR_PAIR: launch_plain_any(p, pl, tA, tB, hs); break;
    case GR_PLAIN128: case GR_PLAIN128_RAGK: case GR_PLAIN128_BK32: case GR_PLAIN256: launch_plain128(p, pl, tA, tB, hs); break;
    case GR_PLAIN_RAGK: case GR_PLAIN_ANY: launch_plain_any(p, pl, tA, tB, hs); break;
    case GR_NN_PLAIN:        launch_nn_plain(p, pl, hs); break;
    case GR_GLDS8_128:       launch_glds8<128>(p, grid, tA, tB, hs); break;
    case GR_GLDS8_64:        launch_glds8<64>(p, grid, tA, tB, hs); break;
    case GR_MFMA128_FULL:    launch_variant<128, 128, 32, true, true, true>(p, grid, tA, tB, hs); break;
    case GR_MFMA128_SKEW:    launch_variant<128, 128, 32, true, true, false>(p, grid, tA, tB, hs); break;
    case GR_MFMA128:         launch_variant<128, 128, 32, false, false, false>(p, grid, tA, tB, hs); break;
    case GR_MFMA64_32:       launch_variant<64, 64, 32, false, false, false>(p, grid, tA, tB, hs); break;
    case GR_GLDS8_128_RAGK:  launch_glds8<128, true>(p, grid, tA, tB, hs); break;
    case GR_GLDS8_64_RAGK:   launch_glds8<64, true>(p, grid, tA, tB, hs); break;
    case GR_MFMA64_FULL:     launch_variant<64, 64, 64, true, false, true>(p, grid, tA, tB, hs); break;
    case GR_MFMA64_SKEW:     launch_variant<64, 64, 64, true, true, false>(p, grid, tA, tB, hs); break;
    default: return fail(T4K_ERR_ARG, "t4k_gemm: no launch for rung %d", (int)pl.rung);
    }
    if (pl.deferred) {                                   // the consumer folds the slabs (fused head)
        defer->part = p.part; defer->nsplit = pl.nsplit; defer->mn = mn;
    } else if (pl.fold) {
        const Riders r = make_riders(hs, mn, epi, epi_done, rider, 4, 1024);
        T4K_LAUNCH(k_splitk_fold, dim3(grid_for(mn) + r.fr.cp_blocks), dim3(BLK), 0, hs, p.part, O, mn, pl.nsplit, alpha, beta, bias, N, r.ep, r.fr);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}
// every channel of every operand present (no channel broadcast); the caller has checked the arguments
int gemm_batched_tiles(const float *A, const float *B, float *O, float alpha, float beta, int tA, int tB,
                       int M, int N, int K, int C, int batch, long sA, long sB, long sO, hipStream_t hs) {
    GemmP p;
    p.A = A; p.B = B; p.O = O; p.M = M; p.N = N; p.K = K; p.C = C; p.alpha = alpha; p.beta = beta;
    p.kchunk = K; p.sync = st().d_sync;
    // 16-byte loads: C == 1, every entry's base aligned (strides too), contiguous extents divisible by 4
    const int a_contig = tA ? M : K, b_contig = tB ? K : N;
    const bool vec = C == 1 && aligned16(A) && aligned16(B) && sA % 4 == 0 && sB % 4 == 0 && a_contig % 4 == 0 && b_contig % 4 == 0;
    const long per = (long)batch * C;
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    const bool big = t128 * per >= (long)st().cu_count * 3 / 4;
    const int BMv = big ? 128 : 64;
    p.tiles_m = (M + BMv - 1) / BMv; p.tiles_n = (N + BMv - 1) / BMv;
    const dim3 grid((unsigned)(p.tiles_m * p.tiles_n), (unsigned)std::min(batch, 65535), (unsigned)C);
    if (big) {
        const bool full = vec && K % 32 == 0 && M >= 4 && N >= 4;
        if (full)     launch_batched<128, 128, 32, true, true, true>(p, grid, tA, tB, sA, sB, sO, batch, hs);
        else if (vec) launch_batched<128, 128, 32, true, true, false>(p, grid, tA, tB, sA, sB, sO, batch, hs);
        else          launch_batched<128, 128, 32, false, false, false>(p, grid, tA, tB, sA, sB, sO, batch, hs);
    } else if (!vec) {
        launch_batched<64, 64, 32, false, false, false>(p, grid, tA, tB, sA, sB, sO, batch, hs);
    } else if (K % 64 == 0 && M >= 4 && N >= 4) {
        launch_batched<64, 64, 64, true, false, true>(p, grid, tA, tB, sA, sB, sO, batch, hs);
    } else {
        launch_batched<64, 64, 64, true, true, false>(p, grid, tA, tB, sA, sB, sO, batch, hs);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

void gemm_set_spin_err(int *p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_spin_err_dev), &p, sizeof(p)); }

} // namespace t4k

extern "C" {

int t4k_gemm(const float *A, const float *B, float *O, float alpha, float beta,
             int tA, int tB, int M, int N, int K, int C, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    return gemm_launch(A, B, O, nullptr, alpha, beta, tA, tB, M, N, K, C, s);
}

const char *t4k_gemm_last_plan(void) {
    static char text[96];
    const State::GemmLast last = st().gemm_last;
    plan_text(text, sizeof(text), last.rung, last.nsplit, last.fold);
    return text;
}

int t4k_gemm_plan(int M, int N, int K, int C, int tA, int tB, unsigned flags, int cs_rows, int cu, long ws_bytes, char text[64], int out[6]) {
    if (!text || !out || cu < 0 || ws_bytes < 0) return fail(T4K_ERR_ARG, "t4k_gemm_plan: bad argument");
    if (M < 0 || N < 0 || K < 0 || C < 1) return fail(T4K_ERR_ARG, "t4k_gemm: bad argument");
    const State &g = st();
    // the environment of an initialised library: the zero block and the tickets exist
    const GemmEnv env{ cu ? cu : g.cu_count, ws_bytes ? (size_t)ws_bytes : g.ws_bytes ? g.ws_bytes : WS_BYTES, true, true, !(flags & T4K_GP_GATES_OFF),
                       (flags & T4K_GP_LANE) ? 1 : 0, (flags & T4K_GP_CAPTURING) != 0 };
    const GemmAsk ask{ M, N, K, C, tA, tB, (flags & T4K_GP_A16) != 0, (flags & T4K_GP_B16) != 0, !(flags & T4K_GP_EPILOGUE), (flags & T4K_GP_BIAS) != 0,
                       (flags & T4K_GP_RIDER) != 0, (flags & T4K_GP_DEFER) != 0, cs_rows != 0, cs_rows, 1 };
    const GemmPlan pl = gemm_plan(ask, env);
    plan_text(text, 64, pl.rung, pl.nsplit, pl.fold);
    out[0] = pl.nsplit; out[1] = pl.kchunk; out[2] = pl.launches; out[3] = pl.riders != RIDE_NONE; out[4] = pl.cs_rides; out[5] = pl.deferred;
    return T4K_OK;
}

int t4k_gemm_f64acc(const float *A, const float *B, float *O, float alpha, float beta,
                    int M, int N, int K, int C, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!A || !B || !O || M < 0 || N < 0 || K < 0 || C < 1) return fail(T4K_ERR_ARG, "t4k_gemm_f64acc: bad argument");
    const long total = (long)M * N * C; if (total == 0) return T4K_OK;
    T4K_LAUNCH(k_gemm_f64, dim3(grid_for(total)), dim3(BLK), 0, S(s), A, B, O, alpha, beta, M, N, K, C);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // extern "C"
