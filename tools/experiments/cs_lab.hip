// cs_lab.hip - lab harness for the conv-stack kernels (csrc/conv_stack.hip): event timing of the LeNet front end through the C-ABI.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include tools/experiments/cs_lab.hip -L tensorforth_amd -lt4hip -Wl,-rpath,'$ORIGIN/../../tensorforth_amd' -o tools/experiments/cs_lab.bin
//   (link against -lt4hip_lab, the LAB build `make -C tensorforth_amd/csrc LAB=1`, for the s_memtime stamps: CS_LAB_PROF=1)
//   usage: cs_lab.bin [N] [fwd|bwd|head]      (T4K_STACK_SPLIT=1|2|4 forces the number of bands per image; head = forward with the classifier head)
#include <hip/hip_runtime.h>
#include "t4k.h"
#include <cstdio>
#include <cstring>
#include <vector>
#include <cstdlib>
static float *dalloc(size_t n, bool rnd = false) {
    float *d; hipMalloc((void **)&d, n * 4);
    std::vector<float> h(n, 0.f); if (rnd) for (auto &v : h) v = (float)rand() / RAND_MAX - 0.5f;
    hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice); return d;
}
int main(int argc, char **argv) {
    const int N = argc > 1 ? atoi(argv[1]) : 128;
    if (t4k_init(0) != 0) { printf("init failed\n"); return 1; }
    unsigned long long *prof; hipMalloc((void **)&prof, (size_t)N * 4 * 32 * 8); hipMemset(prof, 0, (size_t)N * 4 * 32 * 8);
    { static char e[64]; snprintf(e, sizeof(e), "T4K_STACK_PROF_PTR=%llx", (unsigned long long)prof); if (getenv("CS_LAB_PROF")) putenv(e); }
    t4k_conv_stage st[2]; memset(st, 0, sizeof(st));
    st[0].H = 28; st[0].W = 28; st[0].C1 = 1; st[0].C0 = 10; st[0].K = 3;
    st[1].H = 14; st[1].W = 14; st[1].C1 = 10; st[1].C0 = 20; st[1].K = 3;
    for (int s = 0; s < 2; s++) {
        t4k_conv_stage &t = st[s];
        t.F = dalloc(t.C1 * 9 * t.C0, true); t.B = dalloc(t.C0, true); t.O = dalloc((size_t)N * t.H * t.W * t.C0);
        t.DF = dalloc(t.C1 * 9 * t.C0); t.DB = dalloc(t.C0); t.X = dalloc((size_t)N * t.H * t.W * t.C1, true); t.DXS = dalloc((size_t)N * t.H * t.W * t.C1);
        t4k_poolblock &b = t.run; b.KS = 2; b.pool_layer = T4K_L_MAXPOOL; b.pool_out = dalloc((size_t)N * t.H * t.W * t.C0 / 4);
        b.post_layer = T4K_L_RELU; b.post_mask = dalloc((size_t)N * t.H * t.W * t.C0 / 4); b.post_out = dalloc((size_t)N * t.H * t.W * t.C0 / 4);
        if (s == 1) { b.pre_layer = T4K_L_DROPOUT; b.pre_alpha = 0.5f; b.pre_mask = dalloc((size_t)N * t.H * t.W * t.C0); b.pre_out = dalloc((size_t)N * t.H * t.W * t.C0);
                      b.copy_out = dalloc((size_t)N * t.H * t.W * t.C0 / 4); }
    }
    float *X = dalloc((size_t)N * 784, true), *X0 = dalloc((size_t)N * 784), *DY = dalloc((size_t)N * 980, true);
    const char *mode = argc > 2 ? argv[2] : "fwd";
    const bool bwd = mode[0] == 'b', head = mode[0] == 'h';
    t4k_stack_head hd; memset(&hd, 0, sizeof(hd));
    hd.W1 = dalloc(100 * 980, true); hd.B1 = dalloc(100, true); hd.Y1 = dalloc((size_t)N * 100); hd.mid_layer = T4K_L_DROPOUT; hd.mid_alpha = 0.5f;
    hd.mid_mask = dalloc((size_t)N * 100); hd.mid_out = dalloc((size_t)N * 100); hd.W2 = dalloc(1000, true); hd.B2 = dalloc(10, true);
    hd.Y2 = dalloc((size_t)N * 10); hd.P = dalloc((size_t)N * 10); hd.E1 = 980; hd.E0a = 100; hd.E0b = 10;
    if (head) printf("head ok=%d\n", t4k_conv_stack_head_ok(st, 2, N, &hd));
    printf("N=%d mode=%s ok=%d\n", N, mode, t4k_conv_stack_ok(st, 2, N));
    if (bwd && !getenv("CS_LAB_NOFWD")) t4k_conv_stack_fwd(X, X0, st, 2, N, nullptr);      // the banded backward runs on what a forward saved
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipStream_t ls = (hipStream_t)t4k_default_stream();
    for (int rep = 0; rep < 4; rep++) {
        hipEventRecord(e0, ls);
        int rc = 0;
        for (int i = 0; i < 200; i++) rc |= bwd ? t4k_conv_stack_bwd(DY, st, 2, N, getenv("CS_LAB_TRAIN") ? atoi(getenv("CS_LAB_TRAIN")) : 1, nullptr) : (head ? t4k_conv_stack_head_fwd(X, X0, st, 2, N, &hd, nullptr) : t4k_conv_stack_fwd(X, X0, st, 2, N, nullptr));
        hipEventRecord(e1, ls); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); printf("%s: %.2f us per call (rc %d %s)\n", mode, ms * 1000 / 200, rc, rc ? t4k_last_error() : "");
    }
    if (getenv("CS_LAB_PROF")) {
        hipDeviceSynchronize();
        std::vector<unsigned long long> h((size_t)N * 4 * 32); hipMemcpy(h.data(), prof, h.size() * 8, hipMemcpyDeviceToHost);
        printf("  stamp: cycles since the workgroup's stamp 0, averaged over workgroups\n");
        for (int k = 1; k < 32; k++) {
            double sum = 0; int cnt = 0;
            double mx = 0;
            for (int b = 0; b < N * 4; b++) if (h[b * 32 + k] && h[b * 32]) { const double d = (double)(h[b * 32 + k] - h[b * 32]); sum += d; cnt++; if (d > mx) mx = d; }
            if (cnt) printf("  %2d: avg %8.0f  max %8.0f  (%d workgroups)\n", k, sum / cnt, mx, cnt);
        }
        // forward: the same per DISPATCH ROUND.  Workgroups are placed in the order of their linear id (blockIdx.x fastest); the first `cus` of them start on
        // L2s that hold none of the launch's operands, the later ones on CUs whose XCD has already read W1.  11 -> 12 is the head's W1 matvec.
        if (!bwd) {
            int split = 1, bsplit = 1, cus = 256; t4k_conv_stack_plan(st, 2, N, &split, &bsplit);
            { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, 0) == hipSuccess) cus = pr.multiProcessorCount; }
            for (int late = 0; late < 2; late++) {
                double sum[32] = {0}, d1112 = 0, mx1112 = 0; int cnt[32] = {0}, c1112 = 0;
                for (int b = 0; b < N * split; b++) {
                    const unsigned long long *s = &h[(size_t)b * 32];
                    const int w = b / split + N * (b % split);
                    if ((w >= cus) != (late != 0) || !s[0]) continue;
                    for (int k = 1; k < 32; k++) if (s[k]) { sum[k] += (double)(s[k] - s[0]); cnt[k]++; }
                    if (s[11] && s[12]) { const double d = (double)(s[12] - s[11]); d1112 += d; c1112++; if (d > mx1112) mx1112 = d; }
                }
                if (!cnt[2]) continue;
                printf("  %s (linear id %s %d, split %d):", late ? "later rounds" : "first round", late ? ">=" : "<", cus, split);
                for (int k = 1; k < 32; k++) if (cnt[k]) printf(" %d:%.0f", k, sum[k] / cnt[k]);
                if (c1112) printf("  | 11->12 avg %.0f max %.0f (%d workgroups)", d1112 / c1112, mx1112, c1112);
                printf("\n");
                // the head's collector band (the only one that writes stamps 13 .. 19), link by link: 12 matvec done -> [barrier, poll] -> 15 -> [+ B1, Y1 store,
                // draw, act1, x2 to LDS] -> 16 -> [barrier] -> 13 -> [layer 2 dot products, lane sums] -> 17 -> [y2 to LDS, barrier, softmax max] -> 18 ->
                // [exp, softmax sum] -> 19 -> [divide, stores, hit rider] -> 14
                static const int chain[] = {12, 15, 16, 13, 17, 18, 19, 14};
                double lk[8] = {0}; int nc = 0;
                for (int b = 0; b < N * split; b++) {
                    const unsigned long long *s = &h[(size_t)b * 32];
                    const int w = b / split + N * (b % split);
                    if ((w >= cus) != (late != 0) || !s[0]) continue;
                    bool all = true; for (int k : chain) all = all && s[k] != 0;
                    if (!all) continue;
                    for (int i = 1; i < 8; i++) lk[i] += (double)(long long)(s[chain[i]] - s[chain[i - 1]]);
                    nc++;
                }
                if (nc) {
                    printf("    head collector (%d workgroups):", nc);
                    for (int i = 1; i < 8; i++) printf(" %d->%d:%.0f", chain[i - 1], chain[i], lk[i] / nc);
                    printf("  | 12->14 %.0f\n", (lk[1] + lk[2] + lk[3] + lk[4] + lk[5] + lk[6] + lk[7]) / nc);
                }
            }
        }
        // banded backward: the two wave roles of every stage (stamps 3 / 4 + 8 S: dF role, thread 0; 24 / 25 + 2 S: dX role, first lane of wave 8;
        // 5 + 8 S: thread 0 past the barrier the roles share) - how long each role ran and how long it then stood at the barrier
        for (int S = 2; bwd && S >= 0; S--) {
            double df = 0, dx = 0, wf = 0, wx = 0, skew = 0; int cnt = 0;
            for (int b = 0; b < N * 4; b++) {
                const unsigned long long *s = &h[(size_t)b * 32];
                if (!s[3 + 8 * S] || !s[4 + 8 * S] || !s[5 + 8 * S] || !s[24 + 2 * S] || !s[25 + 2 * S]) continue;
                df += (double)(s[4 + 8 * S] - s[3 + 8 * S]); dx += (double)(s[25 + 2 * S] - s[24 + 2 * S]);
                wf += (double)(s[5 + 8 * S] - s[4 + 8 * S]); wx += (double)(long long)(s[5 + 8 * S] - s[25 + 2 * S]);
                skew += (double)(long long)(s[24 + 2 * S] - s[3 + 8 * S]); cnt++;
            }
            if (cnt) printf("  stage %d roles: dF %6.0f cycles then %6.0f at the barrier | dX %6.0f cycles then %6.0f at the barrier | dX began %+.0f after dF  (%d workgroups)\n",
                            S, df / cnt, wf / cnt, dx / cnt, wx / cnt, skew / cnt, cnt);
        }
    }
    return 0;
}
