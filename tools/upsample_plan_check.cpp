// upsample_plan_check.cpp - t4k_upsample_plan (csrc/upsample.hip) over its admission grid, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/upsample.hip tools/upsample_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/upsample_plan_check
//   build/upsample_plan_check
// (from the repository root, after the library is built: upsample.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the three entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  Every method -1..4 x K -1..18 x extents around the 2^31 limits, with and without
// the table pointers; the admitted calls must fill exactly K rows of the table with weights that sum to 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include "t4k.h"

int main() {
    const int ext[] = { -1, 0, 1, 2, 5, 1 << 10, 1 << 20, (1 << 27) - 1, 1 << 27, 0x7fffffff };
    long calls = 0, ok = 0;
    for (int method = -1; method <= 4; method++)
        for (int K = -1; K <= 18; K++)
            for (int N : ext) for (int H1 : ext) for (int W1 : ext)
                for (int C : { 0, 1, 3, 4 }) for (int aligned = 0; aligned < 4; aligned++) {
                    int out[4] = { -7, -7, -7, -7 }, base[16]; float wt[64];
                    memset(base, 0x5a, sizeof base); memset(wt, 0x5a, sizeof wt);
                    const bool tab = (aligned & 1) != 0;
                    const int rc = t4k_upsample_plan(method, N, H1, W1, C, K, aligned, out, tab ? wt : nullptr, tab ? base : nullptr);
                    calls++;
                    const bool admit = method >= 0 && method <= 3 && N >= 1 && H1 >= 1 && W1 >= 1 && C >= 1 && K >= 1 && K <= (method == 3 ? 8 : 16) &&
                                       (__int128)N * K * H1 * K * W1 < ((__int128)1 << 31);
                    if ((rc == T4K_OK) != admit) { printf("admission: method %d K %d N %d H1 %d W1 %d C %d -> %d\n", method, K, N, H1, W1, C, rc); return 1; }
                    if (rc != T4K_OK) { if (out[0] != -7 || !t4k_last_error()[0]) { printf("a refusal wrote, or left no text\n"); return 1; } continue; }
                    ok++;
                    if (out[0] != K * H1 || out[1] != K * W1) { printf("extents\n"); return 1; }
                    if (!tab) continue;
                    const int T = method == 0 ? 1 : (method == 3 ? 4 : 2);
                    for (int r = 0; r < 16; r++) {
                        float s = 0; for (int a = 0; a < 4; a++) { s += wt[r * 4 + a]; if ((r >= K || a >= T) && wt[r * 4 + a] != 0.0f) { printf("unused cell\n"); return 1; } }
                        if (r < K ? std::fabs(s - 1.0f) > 2.4e-7f : (s != 0.0f || base[r] != 0)) { printf("row %d of method %d K %d sums to %g\n", r, method, K, s); return 1; }
                        if (r < K && (base[r] < -(T / 2) || base[r] + T - 1 > T / 2)) { printf("base\n"); return 1; }
                    }
                }
    printf("t4k_upsample_plan: %ld calls, %ld admitted, all as the rule says\n", calls, ok);
    return 0;
}
