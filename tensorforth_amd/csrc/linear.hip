// linear.hip - the linear layers on the GEMM kernels: which launches a layer's forward / backward becomes (the dual dW || dX launch,
// the one-launch classifier-head backward, riders in a GEMM's last launch, or plain gemm_launch calls) and the t4k_linear_* / t4k_mlp_*
// entry points.  The kernels launched here: k_gemm_dual (gemm_tile.h), k_gemm_dual_l32 (gemm_l32.h), k_head_bwd_l32 (gemm_head_bwd.h);
// classifier-head sized layers go to linear_small.hip, everything else through gemm_launch (gemm.hip).
#include "gemm_types.h"
#include "gemm_tile.h"
#include "gemm_l32.h"
#include "gemm_head_bwd.h"

namespace {

bool dual_on() { return gemm_lab().dual != 0 && gates_ok(); }
// one GEMM of a linear layer's backward on 32x32 tiles, unsplit (k_gemm_dual_l32, k_head_bwd_l32): O = A B (beta 0) or O += A B (beta 1)
GemmP bwd_gemm32(const float *A, const float *B, float *O, int M, int N, int K, float beta) {
    GemmP p;
    p.A = A; p.B = B; p.O = O; p.M = M; p.N = N; p.K = K; p.beta = beta;
    p.tiles_m = (M + 31) / 32; p.tiles_n = (N + 31) / 32; p.kchunk = K; p.sync = st().d_sync; p.Z = st().d_zero;
    return p;
}
// dW += dY^T X (+ dB += column sums of dY) and dX = dY W of one linear layer in a single launch (k_gemm_dual); false when the
// shapes belong to the other kernels (deep K -> split-K, large -> 128x128 tiles).  Interior-tile shapes take it too since round 2
// (T4K_GEMM_DUAL_FULL=0: the LDS-DMA kernels, 5 launches with their folds and the column sum: GAN round 0.356 instead of 0.318 ms of GPU time)
bool linear_bwd_dual(const float *X, const float *W, const float *DY, float *DX, float *DW, float *DB, int N, int E0, int E1, hipStream_t hs,
                     const MaskChain *mcp = nullptr) {
    State &g = st();
    const GemmLab &lab = gemm_lab();
    int *gate = gate_for(hs, 1);                             // nullptr: unknown stream, the two GEMMs go out as separate launches
    if (!dual_on() || !g.d_sync || !gate || (E0 & 3) || (E1 & 3) || !aligned16(DY) || !aligned16(X) || !aligned16(W) || N < 1) return false;
    const int cu = g.cu_count;
    auto full = [](int m, int n, int k) { return m % 64 == 0 && n % 64 == 0 && k % 64 == 0; };
    const long t1 = gemm_tiles64(E0, E1), t2 = gemm_tiles64(N, E1), riders = (E0 + 63) / 64;
    // deep-K shapes would go split-K + fold (2 launches per GEMM); up to K = 1024 the single dual launch, unsplit, is faster (GAN round 0.318 ms of GPU time; with T4K_GEMM_DUAL_MAXK=256: 0.341)
    const bool sp = gemm_splits(t1, N, cu) || gemm_splits(t2, E0, cu);
    if (gemm_big(E0, E1, cu) || gemm_big(N, E1, cu) || (sp && (N > lab.dual_maxk || E0 > lab.dual_maxk))) return false;
    if (!lab.dual_full && (full(E0, E1, N) || full(N, E1, E0))) return false;
    if (t1 + riders + t2 > cu || N > 4096) return false;
    const bool alias = (const float *)DX == X || (const float *)DX == DY || (const float *)DX == W;   // only an in-place dX needs the arrival gate
    const MaskChain mc = mcp ? *mcp : MaskChain{nullptr, nullptr, nullptr, nullptr};
    {   // small layers: 32x32 tiles, K split over the waves of a workgroup, operand blocks through LDS-DMA (k_gemm_dual_l32)
        auto t32 = [](int m, int n) { return (long)((m + 31) / 32) * ((n + 31) / 32); };
        const long a1 = t32(E0, E1), a2 = t32(N, E1), ar = (E0 + 63) / 64;
        // the gated (in-place dX) launch may hold more workgroups than fit the chip at 1-2 per CU (64*W threads, W*16 KiB of LDS): progress then rests on the
        // dispatcher handing out workgroups in id order - the dW blocks [0, a1 + ar) never wait, the dX writers behind them wait only for those - so the
        // id -> tile map stays the identity; a device that dispatches out of order ends in the bounded-spin error
        if (lab.dual32 && g.d_zero && a1 + ar + a2 <= 4L * cu - 32 && a1 <= 512 && N <= 1024 && E0 <= 1024 && !capturing(hs)) {      // a wave walks at most four 32-deep blocks; deeper K stays with the staged kernels
            GemmP q1 = bwd_gemm32(DY, X, DW, E0, E1, N, 1.0f);
            q1.cs_X = DY; q1.cs_out = DB; q1.cs_rows = N; q1.cs_E = E0;
            const GemmP q2 = bwd_gemm32(DY, W, DX, N, E1, E0, 0.0f);
            // arrival slots: ints [512, 1024) of the stream's gate block; the epoch is this stream's launch count (never 0, slots cleared when it wraps)
            unsigned *slots = reinterpret_cast<unsigned *>(gate_for(hs, 0)) + 512;
            const unsigned epoch = next_slot_epoch(hs, slots);     // the lane's ONE counter, shared with k_head_bwd_l32 (t4k_common.h)
            const dim3 gd((unsigned)(a1 + ar + a2));
            auto go = [&](auto rst, auto nw) {
                launch_lds<k_gemm_dual_l32<rst(), nw()>>(gd, dim3(64 * nw()), (size_t)nw() * 16384, hs, q1, q2, (int)(a1 + ar), (int)a1, (int)a2, alias ? slots : nullptr, epoch, mc);
            };
            if (N > 512 || E0 > 512) go(std::true_type{}, std::integral_constant<int, 8>{});            // deep K: 8 k-groups (one arrival slot per workgroup)
            else if (N > 256 || E0 > 256) go(std::true_type{}, std::integral_constant<int, 4>{});
            else go(std::false_type{}, std::integral_constant<int, 4>{});
            return true;
        }
    }
    auto fill = [&](const float *A, const float *B, float *O, int M, int Nn, int K, float beta) {
        GemmP p;
        p.A = A; p.B = B; p.O = O; p.M = M; p.N = Nn; p.K = K; p.beta = beta;
        p.tiles_m = (M + 63) / 64; p.tiles_n = (Nn + 63) / 64; p.kchunk = ((K + 63) / 64) * 64; p.sync = g.d_sync;
        return p;
    };
    GemmP p1 = fill(DY, X, DW, E0, E1, N, 1.0f);             // A = dY^T ([K][M]), B = X ([K][N])
    p1.cs_X = DY; p1.cs_out = DB; p1.cs_rows = N; p1.cs_E = E0;
    const GemmP p2 = fill(DY, W, DX, N, E1, E0, 0.0f);       // A = dY ([M][K]), B = W ([K][N])
    const bool f1 = lab.dual_fullk && N % 64 == 0 && E0 >= 4 && E1 >= 4, f2 = lab.dual_fullk && E0 % 64 == 0 && E1 >= 4;
    with_flags([&](auto F1, auto F2) {
        launch_lds<k_gemm_dual<false, false, true, false, F1(), F2()>>(dim3((unsigned)(t1 + riders + t2)), dim3(256), (size_t)2 * (64 + 64) * 64 * sizeof(float), hs,
                                                                     p1, p2, (int)(t1 + riders), (int)t1, (int)t2, alias ? gate : nullptr, mc);
    }, f1, f2);
    return true;
}

size_t head_bwd_lds(int N, int EA, int EB) {                       // dynamic LDS of k_head_bwd_l32: the larger of a tile's and a rider's
    const size_t kd = (size_t)((std::max(N, EA) + 31) / 32) * 32;
    const size_t lt = 8192 + kd * HB_AP, lr = (size_t)N * EB + (size_t)EB * HB_CW + (size_t)N * HB_CW + 256;
    return sizeof(float) * std::max(std::max(lt, lr), (size_t)N * EB);
}
// do the shapes take the one-launch head backward (t4k_mlp_head_bwd_ok)?  Asked twice per training step: the occupancy answer is remembered for the
// last LDS request (a model asks with one)
bool head_bwd_ok(int N, int E1, int EA, int EB) {
    if (!gemm_lab().head_bwd || st().capturing || !st().d_sync || !st().d_zero || !dual_on()) return false;
    if (N < 1 || N > 256 || EA < 4 || EA > 256 || (EA & 3) || EB < 1 || EB > 16 || E1 < 4 || (E1 & 3)) return false;
    auto t32 = [](int m, int n) { return (long)((m + 31) / 32) * ((n + 31) / 32); };
    const long a1 = t32(EA, E1), a2 = t32(N, E1), nr = 1 + (EA + HB_CW - 1) / HB_CW;
    const size_t lds = head_bwd_lds(N, EA, EB);
    int nb;                                                       // resident workgroups per CU at this LDS request (0: the query failed)
    {
        static std::mutex m; static size_t lds_asked = 0; static int nb_answer = 0;      // the pair is read and replaced as one (callers on several threads)
        std::lock_guard<std::mutex> hold(m);
        if (lds != lds_asked) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb_answer, k_head_bwd_l32, 256, lds) != hipSuccess) nb_answer = 0;
            lds_asked = lds;
        }
        nb = nb_answer;
    }
    if (nb < 1) return false;
    return a1 + a2 + nr <= (long)nb * st().cu_count - 32 && a1 <= 512 && a1 + a2 + nr <= 768;      // every workgroup resident (the in-place gate and the target store spin); 768 per-workgroup slots
}
int head_bwd_launch(float *X2, const float *W2, float *P, const float *TGT, float *Y2, const MaskChain &mc2, float *DW2, float *DB2,
                    float *X1, const float *W1, const MaskChain &mc1, float *DW1, float *DB1, int N, int E1, int EA, int EB, bool train, hipStream_t hs, const char *who) {
    int *gate = gate_for(hs, 0);
    float *DY1 = mc2.d2 ? mc2.d2 : mc2.d1;                        // what the big layer differentiates against: the product of all masks
    if (!head_bwd_ok(N, E1, EA, EB) || !gate || capturing(hs) || !aligned16(X1) || !aligned16(W1) || !aligned16(DY1))
        return fail(T4K_ERR_UNSUPPORTED, "%s: shapes do not qualify (t4k_mlp_head_bwd_ok)", who);
    State &g = st();
    auto t32 = [](int m, int n) { return (long)((m + 31) / 32) * ((n + 31) / 32); };
    const long a1 = train ? t32(EA, E1) : 0, a2 = t32(N, E1), nr = 1 + (EA + HB_CW - 1) / HB_CW;
    const GemmP q1 = bwd_gemm32(DY1, X1, DW1, EA, E1, N, 1.0f);   // dW1 += dY1^T X1   (A is prepared in LDS: the pointer is not read)
    const GemmP q2 = bwd_gemm32(DY1, W1, X1, N, E1, EA, 0.0f);    // dX1 = dY1 W1, over X1 (backprop.cu:240)
    // arrival slots, all tagged with the lane's ONE epoch counter (shared with k_gemm_dual32): ints [512, 1024) of the lane's gate block for the in-place dX
    // (as linear_bwd_dual; a frozen layer has no dW readers to wait for), ints [1280, 2048) one per workgroup for the `out -= target` store
    unsigned *slots = reinterpret_cast<unsigned *>(gate) + 512, *pslots = reinterpret_cast<unsigned *>(gate) + 1280;
    const unsigned epoch = next_slot_epoch(hs, slots);
    if (!train) slots = nullptr;
    HeadBwd hb = { P, TGT, W2, mc2.m1, X2, DW2, DB2, mc2.d1, Y2, DB1, N, EA, EB, train ? 1 : 0, (int)(a1 + a2 + nr), gate, mc2.m2, mc2.d2, mc1, g.d_zero };
#ifdef T4K_LAB
    { const char *e = getenv("T4K_HB_LAB"); hb.lab = e ? atoi(e) : 0; }    // timing ablations (wrong results): see the kernel's HB_LAB bits
    { const char *e = getenv("T4K_HB_PROF_PTR"); hb.prof = e ? reinterpret_cast<unsigned long long *>(strtoull(e, nullptr, 16)) : nullptr; }   // role stamps: a device address, hex, of HB_PROF_WORDS x 8 bytes per workgroup (tools/experiments/head_bwd_lab.py)
#endif
    // a1 dW1 tiles, a2 dX1 tiles, then the nr riders (the kernel maps blockIdx.x to the roles: gemm_head_bwd.h, T4K_HB_RIDERS_LAST)
    launch_lds<k_head_bwd_l32>(dim3((unsigned)(a1 + a2 + nr)), dim3(256), head_bwd_lds(N, EA, EB), hs, q1, q2, (int)a1, (int)nr, slots, pslots, epoch, hb);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // namespace

namespace t4k {
void linear_set_spin_err(int *p) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_spin_err_dev), &p, sizeof(p)); }
}

extern "C" {

// Model::_flinear src/nn/forward.cu:157-198: Y[N,E0] = X[N,E1] @ W[E0,E1]^T + B[E0], bias fused
int t4k_linear_fwd(const float *X, const float *W, const float *B, float *Y, int N, int E0, int E1, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !W || !Y || N < 0) return fail(T4K_ERR_ARG, "t4k_linear_fwd: bad argument");
    if (N > 0 && linear_small_ok(E0, E1)) { linear_small_fwd(X, W, B, Y, nullptr, N, E0, E1, S(s)); T4K_LAUNCH_CHECK(); return T4K_OK; }
    return gemm_launch(X, W, Y, B, 1.0f, 0.0f, 0, 1, N, E0, E1, 1, s);
}
// linear followed by an element-wise layer (relu, tanh, ..., dropout): Y = X W^T + b; ACT_O, ACT_F = activation(Y).
// When the GEMM is split-K the activation rides in the fold launch; otherwise it is a second launch.
int t4k_linear_act_fwd(const float *X, const float *W, const float *B, float *Y, int layer, float alpha, float *ACT_F, float *ACT_O,
                       int N, int E0, int E1, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !W || !Y || !ACT_F || !ACT_O || N < 0) return fail(T4K_ERR_ARG, "t4k_linear_act_fwd: bad argument");
    if (N == 0) return T4K_OK;
    bool done = false;
    if (linear_small_ok(E0, E1)) {
        ActEpi ep = { layer, alpha, ACT_F, ACT_O, RngArg{0, 0, nullptr} };
        const bool fuse = !(layer == T4K_L_DROPOUT && st().capturing);   // a captured mask draw advances a device-resident counter: the separate launches below do that
        if (fuse && layer == T4K_L_DROPOUT) ep.rng = rng_draw(S(s), (uint64_t)(((long)N * E0 + 3) >> 2), true);
        linear_small_fwd(X, W, B, Y, nullptr, N, E0, E1, S(s), nullptr, fuse ? &ep : nullptr);
        done = fuse;
    } else {
        // the mask's Philox slice is reserved only if the fold launch will really apply the epilogue (decided inside gemm_launch)
        ActEpi ep = { layer, alpha, ACT_F, ACT_O, RngArg{0, 0, nullptr} };
        int rc = gemm_launch(X, W, Y, B, 1.0f, 0.0f, 0, 1, N, E0, E1, 1, s, &ep, &done); if (rc) return rc;
    }
    if (!done) {
        const long n = (long)N * E0;
        if (layer == T4K_L_DROPOUT) { int rc = t4k_dropout_mask(ACT_F, n, s); if (rc) return rc; }
        return t4k_activate(layer, Y, ACT_O, ACT_F, alpha, n, s);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}
// linear layer + the element-wise run behind it (one or two layers, no pool) + optionally the model's copy of its input batch: when the
// GEMM is split along K all of it rides in the fold launch; otherwise the same tensors come from the separate launches.
int t4k_linear_block_fwd(const float *X, float *XCOPY, const float *W, const float *B, float *Y, const t4k_poolblock *blk,
                         int N, int E0, int E1, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !W || !Y || N < 0 || E0 < 1 || E1 < 1) return fail(T4K_ERR_ARG, "t4k_linear_block_fwd: bad argument");
    int n1 = 0, n2 = 0; float a1 = 0.f, a2 = 0.f; float *F1 = nullptr, *A1 = nullptr, *F2 = nullptr, *A2 = nullptr;
    if (blk) {
        if (blk->pool_layer || blk->copy_out || blk->KS != 1) return fail(T4K_ERR_UNSUPPORTED, "t4k_linear_block_fwd: the run behind a linear layer has no pool / flatten stage");
        if (blk->pre_layer)  { n1 = blk->pre_layer; a1 = blk->pre_alpha; F1 = blk->pre_mask; A1 = blk->pre_out; }
        if (blk->post_layer) { if (n1) { n2 = blk->post_layer; a2 = blk->post_alpha; F2 = blk->post_mask; A2 = blk->post_out; }
                               else    { n1 = blk->post_layer; a1 = blk->post_alpha; F1 = blk->post_mask; A1 = blk->post_out; } }
        if ((n1 && (!F1 || !A1)) || (n2 && (!F2 || !A2))) return fail(T4K_ERR_ARG, "t4k_linear_block_fwd: stage tensors missing");
        if (n1 == T4K_L_DROPOUT && n2 == T4K_L_DROPOUT) return fail(T4K_ERR_UNSUPPORTED, "t4k_linear_block_fwd: one dropout per run");
    }
    if (N == 0) return T4K_OK;
    bool done = false;
    FoldRider fr = {ActEpi{n2, a2, F2, A2, RngArg{0, 0, nullptr}}, (XCOPY && XCOPY != X) ? X : nullptr, XCOPY, (long)N * E1, 0, 0, MaskChain{nullptr, nullptr, nullptr, nullptr}, 0};
    if (linear_small_ok(E0, E1)) {
        ActEpi ep = { n1, a1, F1, A1, RngArg{0, 0, nullptr} };
        const bool fuse = n1 && !n2 && !(n1 == T4K_L_DROPOUT && st().capturing);     // one stage rides in the head kernel
        if (fuse && n1 == T4K_L_DROPOUT) ep.rng = rng_draw(S(s), (uint64_t)(((long)N * E0 + 3) >> 2), true);
        linear_small_fwd(X, W, B, Y, nullptr, N, E0, E1, S(s), nullptr, fuse ? &ep : nullptr);
        done = fuse;
    } else {
        ActEpi ep = { n1, a1, F1, A1, RngArg{0, 0, nullptr} };
        int rc = gemm_launch(X, W, Y, B, 1.0f, 0.0f, 0, 1, N, E0, E1, 1, s, &ep, &done, nullptr, nullptr, &fr); if (rc) return rc;
    }
    if (XCOPY && !fr.cp_blocks && XCOPY != X) { int rc = t4k_copy(X, XCOPY, (long)N * E1, s); if (rc) return rc; }
    if (!done && n1) {
        const long n = (long)N * E0;
        if (n2) return t4k_poolblock_fwd(Y, blk, N, 1, 1, 1, 1, E0, s);
        if (n1 == T4K_L_DROPOUT) { int rc = t4k_dropout_mask(F1, n, s); if (rc) return rc; }
        return t4k_activate(n1, Y, A1, F1, a1, n, s);
    }
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}
// classifier head: [linear + element-wise layer] + [linear (+ softmax)].  When the first GEMM is split along K and the second
// layer is head-sized, the second layer's kernel folds the slabs, applies bias + activation (writing Y1, F1, A1 as the fold
// launch would) while staging its input rows: two launches instead of three.  Otherwise the two fused entries in sequence.
int t4k_mlp_head_fwd(const float *X, const float *W1, const float *B1, float *Y1, int layer, float alpha, float *F1, float *A1,
                     const float *W2, const float *B2, float *Y2, float *P2, int N, int H, int E1, int E2, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !W1 || !Y1 || !F1 || !A1 || !W2 || !Y2 || N < 0) return fail(T4K_ERR_ARG, "t4k_mlp_head_fwd: bad argument");
    if (N == 0) return T4K_OK;
    if (gemm_lab().head_fold && !linear_small_ok(H, E1) && linear_small_ok(E2, H)) {
        XFold xf; xf.part = nullptr;
        int rc = gemm_launch(X, W1, Y1, B1, 1.0f, 0.0f, 0, 1, N, H, E1, 1, s, nullptr, nullptr, nullptr, &xf); if (rc) return rc;
        if (xf.part) {
            xf.bias = B1; xf.Y = Y1; xf.ep = ActEpi{ layer, alpha, F1, A1, RngArg{0, 0, nullptr} };
            if (layer == T4K_L_DROPOUT) xf.ep.rng = rng_draw(S(s), (uint64_t)((xf.mn + 3) >> 2), true);
            linear_small_fwd(A1, W2, B2, Y2, P2, N, E2, H, S(s), &xf);
            T4K_LAUNCH_CHECK(); return T4K_OK;
        }
        const long n = (long)N * H;                         // the GEMM ran unsplit: Y1 is complete, continue layer by layer
        if (layer == T4K_L_DROPOUT) { rc = t4k_dropout_mask(F1, n, s); if (rc) return rc; }
        rc = t4k_activate(layer, Y1, A1, F1, alpha, n, s); if (rc) return rc;
    } else {
        int rc = t4k_linear_act_fwd(X, W1, B1, Y1, layer, alpha, F1, A1, N, H, E1, s); if (rc) return rc;
    }
    if (P2) return t4k_linear_softmax_fwd(A1, W2, B2, Y2, P2, N, E2, H, s);
    return t4k_linear_fwd(A1, W2, B2, Y2, N, E2, H, s);
}
// linear followed by a softmax layer: Y = X W^T + b, P = softmax(Y); one launch when the head is small
int t4k_linear_softmax_fwd(const float *X, const float *W, const float *B, float *Y, float *P, int N, int E0, int E1, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !W || !Y || !P || N < 0) return fail(T4K_ERR_ARG, "t4k_linear_softmax_fwd: bad argument");
    if (N == 0) return T4K_OK;
    if (linear_small_ok(E0, E1)) { linear_small_fwd(X, W, B, Y, P, N, E0, E1, S(s)); T4K_LAUNCH_CHECK(); return T4K_OK; }
    int rc = gemm_launch(X, W, Y, B, 1.0f, 0.0f, 0, 1, N, E0, E1, 1, s); if (rc) return rc;
    return t4k_softmax(Y, P, N, E0, s);
}
// Model::_blinear src/nn/backprop.cu:193-254
int t4k_linear_bwd(const float *X, const float *W, const float *DY, float *DX, float *DW, float *DB,
                   int N, int E0, int E1, int train, t4k_stream_t s) {
    return t4k_linear_bwd2(X, W, DY, DX, nullptr, nullptr, DW, DB, N, E0, E1, train, s);
}
// same, plus the mask-multiply backward of the element-wise layer in front of this linear layer (dropout, relu, ...):
// DXM = DX (*) MASK (`in = out * mask`, _bactivate backprop.cu:256-263) from the same launch when the head is small
int t4k_linear_bwd2(const float *X, const float *W, const float *DY, float *DX, const float *MASK, float *DXM, float *DW, float *DB,
                    int N, int E0, int E1, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if ((MASK == nullptr) != (DXM == nullptr) || (DXM && !DX)) return fail(T4K_ERR_ARG, "t4k_linear_bwd2: MASK and DXM go together (with DX)");
    if (DXM && !(N > 0 && linear_small_ok(E0, E1))) {    // large layer: the GEMM path, then the mask multiply on its own
        int rc = t4k_linear_bwd2(X, W, DY, DX, nullptr, nullptr, DW, DB, N, E0, E1, train, s); if (rc) return rc;
        return t4k_tt_op(T4K_MUL, DX, MASK, DXM, (long)N * E1, s);
    }
    if ((DW == nullptr) != (DB == nullptr)) return fail(T4K_ERR_ARG, "t4k_linear_bwd: DW and DB go together");
    if (N > 0 && linear_small_ok(E0, E1) && linear_small_bwd(X, W, DY, DX, DW, DB, N, E0, E1, train != 0, S(s), MASK, DXM)) { T4K_LAUNCH_CHECK(); return T4K_OK; }
    if (DXM) { int rc = t4k_linear_bwd2(X, W, DY, DX, nullptr, nullptr, DW, DB, N, E0, E1, train, s); if (rc) return rc; return t4k_tt_op(T4K_MUL, DX, MASK, DXM, (long)N * E1, s); }
    if (train && DW && DX && N > 0 && linear_bwd_dual(X, W, DY, DX, DW, DB, N, E0, E1, S(s))) { T4K_LAUNCH_CHECK(); return T4K_OK; }
    if (train && DW) {                                  // DW == NULL: dX only (the caller forks dW|dB to another stream)
        ColSum cs = { DY, DB, N, E0, false };           // dB += sum_n dY rides in the dW launch when the generic kernel runs it
        int rc = gemm_launch(DY, X, DW, nullptr, 1.0f, 1.0f, 1, 0, E0, E1, N, 1, s, nullptr, nullptr, &cs);   // dW += dY^T @ X
        if (rc) return rc;
        if (!cs.done) { rc = colsum_add(DY, DB, N, E0, S(s)); if (rc) return rc; }
    }
    if (!DX) return T4K_OK;                             // DX == NULL: dW|dB only
    return gemm_launch(DY, W, DX, nullptr, 1.0f, 0.0f, 0, 0, N, E1, E0, 1, s);   // dX = dY @ W (may overwrite X)
}

// backprop's `out -= target` (+ the output layer's pass-through copy) folded into the last linear layer's backward
int t4k_loss_linear_bwd(const float *X, const float *W, float *OUT, const float *TGT, float *OUT2, float *DX,
                        const float *MASK, float *DXM, float *DW, float *DB, int N, int E0, int E1, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !W || !OUT || !TGT || N < 0 || E0 < 1 || E1 < 1) return fail(T4K_ERR_ARG, "t4k_loss_linear_bwd: bad argument");
    if ((MASK == nullptr) != (DXM == nullptr) || (DXM && !DX)) return fail(T4K_ERR_ARG, "t4k_loss_linear_bwd: MASK and DXM go together (with DX)");
    if ((DW == nullptr) != (DB == nullptr)) return fail(T4K_ERR_ARG, "t4k_loss_linear_bwd: DW and DB go together");
    if (N == 0) return T4K_OK;
    if (linear_small_ok(E0, E1) && linear_small_bwd(X, W, OUT, DX, DW, DB, N, E0, E1, train != 0, S(s), MASK, DXM, TGT, OUT2)) { T4K_LAUNCH_CHECK(); return T4K_OK; }
    int rc = t4k_tt_op2(T4K_SUB, OUT, TGT, OUT, OUT2, (long)N * E0, s); if (rc) return rc;
    return t4k_linear_bwd2(X, W, OUT, DX, MASK, DXM, DW, DB, N, E0, E1, train, s);
}

// linear backward + the backward of the element-wise run IN FRONT of the layer (the run that produced X), + optionally backprop's
// `out -= target` start: one launch when the shapes allow (vector-ALU head kernel, or the dual dW || dX launch), else layer by layer
int t4k_linear_block_bwd(const float *X, const float *W, float *DY, const float *TGT, float *DY2, float *DX, const t4k_poolblock *blk, float *XRUN,
                         float *DW, float *DB, int N, int E0, int E1, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X || !W || !DY || !DX || !blk || !XRUN || N < 0 || E0 < 1 || E1 < 1) return fail(T4K_ERR_ARG, "t4k_linear_block_bwd: bad argument");
    if ((DW == nullptr) != (DB == nullptr)) return fail(T4K_ERR_ARG, "t4k_linear_block_bwd: DW and DB go together");
    if (blk->pool_layer || blk->copy_out || blk->KS != 1 || (!blk->pre_layer && !blk->post_layer)) return fail(T4K_ERR_UNSUPPORTED, "t4k_linear_block_bwd: the run in front of a linear layer has no pool / flatten stage");
    if ((blk->pre_layer && (!blk->pre_mask || (blk->post_layer && !blk->pre_out))) || (blk->post_layer && !blk->post_mask)) return fail(T4K_ERR_ARG, "t4k_linear_block_bwd: stage tensors missing");
    if (N == 0) return T4K_OK;
    MaskChain mc = {nullptr, nullptr, nullptr, nullptr};
    if (blk->post_layer) { mc.m1 = blk->post_mask; mc.d1 = blk->pre_layer ? blk->pre_out : XRUN; if (blk->pre_layer) { mc.m2 = blk->pre_mask; mc.d2 = XRUN; } }
    else                 { mc.m1 = blk->pre_mask; mc.d1 = XRUN; }
    hipStream_t hs = S(s);
    if (linear_small_ok(E0, E1) &&
        linear_small_bwd(X, W, DY, DX, DW, DB, N, E0, E1, train != 0, hs, mc.m1, mc.d1, TGT, DY2, mc.m2, mc.d2)) { T4K_LAUNCH_CHECK(); return T4K_OK; }
    if (TGT) { int rc = t4k_tt_op2(T4K_SUB, DY, TGT, DY, DY2, (long)N * E0, s); if (rc) return rc; }
    if (linear_small_ok(E0, E1) &&                              // the head kernel could not take the target (dX apart from X): masks still ride
        linear_small_bwd(X, W, DY, DX, DW, DB, N, E0, E1, train != 0, hs, mc.m1, mc.d1, nullptr, nullptr, mc.m2, mc.d2)) { T4K_LAUNCH_CHECK(); return T4K_OK; }
    if (train && DW && linear_bwd_dual(X, W, DY, DX, DW, DB, N, E0, E1, hs, &mc)) { T4K_LAUNCH_CHECK(); return T4K_OK; }
    if (!(train && DW) && !linear_small_ok(E0, E1)) {       // dX only (a frozen net in the middle of a chain): the mask chain rides in the GEMM's fold launch
        FoldRider fr = {ActEpi{0, 0.f, nullptr, nullptr, RngArg{0, 0, nullptr}}, nullptr, nullptr, 0, 0, 0, mc, 0};
        int rc = gemm_launch(DY, W, DX, nullptr, 1.0f, 0.0f, 0, 0, N, E1, E0, 1, s, nullptr, nullptr, nullptr, nullptr, &fr); if (rc) return rc;
        if (fr.mc_done) return T4K_OK;
        return t4k_poolblock_bwd(DX, XRUN, blk, N, 1, 1, 1, 1, E1, s);
    }
    int rc = t4k_linear_bwd2(X, W, DY, DX, nullptr, nullptr, DW, DB, N, E0, E1, train, s); if (rc) return rc;
    return t4k_poolblock_bwd(DX, XRUN, blk, N, 1, 1, 1, 1, E1, s);
}

// Classifier-head backward AND the backward of the linear layer in front of it in ONE launch (k_head_bwd_l32): what
// t4k_loss_linear_bwd(X2, W2, P, TGT, Y2, X2, MASK, Y1, DW2, DB2, N, EB, EA, 1) followed by t4k_linear_bwd(X1, W1, Y1, X1, DW1, DB1, N, EA, E1, 1)
// compute (backprop.cu:103-121, 226-254; gradients accumulate), for a training pass with the in-place convention.  T4K_ERR_UNSUPPORTED when the shapes
// do not qualify - the caller then makes the two calls.
int t4k_mlp_head_bwd_ok(int N, int E1, int EA, int EB) { return st().ready && head_bwd_ok(N, E1, EA, EB) ? 1 : 0; }
int t4k_mlp_head_bwd(float *X2, const float *W2, float *P, const float *TGT, float *Y2, const float *MASK, float *Y1, float *DW2, float *DB2,
                     float *X1, const float *W1, float *DW1, float *DB1, int N, int E1, int EA, int EB, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X2 || !W2 || !P || !TGT || !MASK || !Y1 || !DW2 || !DB2 || !X1 || !W1 || !DW1 || !DB1) return fail(T4K_ERR_ARG, "t4k_mlp_head_bwd: null argument");
    const MaskChain mc2 = { MASK, Y1, nullptr, nullptr }, none = { nullptr, nullptr, nullptr, nullptr };
    return head_bwd_launch(X2, W2, P, TGT, Y2, mc2, DW2, DB2, X1, W1, none, DW1, DB1, N, E1, EA, EB, true, S(s), "t4k_mlp_head_bwd");
}
// The same with element-wise RUNS instead of a single mask layer (the GAN nets: `leakyrelu dropout` between the linear layers): run2 stands in front of the
// head layer (it produced X2; its backward lands in its own tensors, the run's input tensor XRUN2 = the big layer's output receives dY1), run1 in front of
// the big layer (NULL: none; its mask multiplies ride in the dX1 epilogue into run1's tensors / XRUN1).  train = 0: a frozen net (no dW / dB, DW* may be NULL).
int t4k_mlp_block_bwd(float *X2, const float *W2, float *P, const float *TGT, float *Y2, const t4k_poolblock *run2, float *XRUN2, float *DW2, float *DB2,
                      float *X1, const float *W1, const t4k_poolblock *run1, float *XRUN1, float *DW1, float *DB1, int N, int E1, int EA, int EB, int train, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!X2 || !W2 || !P || !TGT || !run2 || !XRUN2 || !X1 || !W1) return fail(T4K_ERR_ARG, "t4k_mlp_block_bwd: null argument");
    if (train && (!DW2 || !DB2 || !DW1 || !DB1)) return fail(T4K_ERR_ARG, "t4k_mlp_block_bwd: a training pass needs the gradient tensors");
    auto chain = [&](const t4k_poolblock *b, float *xrun, MaskChain &mc) -> bool {
        mc = MaskChain{nullptr, nullptr, nullptr, nullptr};
        if (!b) return true;
        if (b->pool_layer || b->copy_out || b->KS != 1 || (!b->pre_layer && !b->post_layer) || !xrun) return false;
        if ((b->pre_layer && (!b->pre_mask || (b->post_layer && !b->pre_out))) || (b->post_layer && !b->post_mask)) return false;
        if (b->post_layer) { mc.m1 = b->post_mask; mc.d1 = b->pre_layer ? b->pre_out : xrun; if (b->pre_layer) { mc.m2 = b->pre_mask; mc.d2 = xrun; } }
        else               { mc.m1 = b->pre_mask; mc.d1 = xrun; }
        return true;
    };
    MaskChain mc2, mc1;
    if (!chain(run2, XRUN2, mc2) || !mc2.d1 || !chain(run1, XRUN1, mc1)) return fail(T4K_ERR_UNSUPPORTED, "t4k_mlp_block_bwd: the runs must be one or two mask-multiply layers without pool / flatten");
    return head_bwd_launch(X2, W2, P, TGT, Y2, mc2, DW2, DB2, X1, W1, mc1, DW1, DB1, N, E1, EA, EB, train != 0, S(s), "t4k_mlp_block_bwd");
}

} // extern "C"
