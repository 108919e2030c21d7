// attention_plan_check.cpp - t4k_attention_plan (csrc/attention.hip) around every limit, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/attention.hip tools/attention_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/attention_plan_check
//   build/attention_plan_check
// (from the repository root, after the library is built: attention.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the three entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  Extents around 0, 1 and 2^31, d in { -4, 0, 2, 4, 6, 16, 20, 32, 36, 64, 68, 128, 132 }, both
// load paths, both masks, workspaces from nothing to plenty: each verdict and each out[] against the rule restated here in 128-bit arithmetic.
#include <cstdio>
#include "t4k.h"

typedef __int128 i128;

int main() {
    const int ext[] = { -1, 0, 1, 2, 3, 63, 64, 65, 196, 1024, 4097, 1 << 16, (1 << 20) + 4, 44739242, 44739243, 0x7ffffffc, 0x7fffffff };
    const int ds[] = { -4, 0, 2, 4, 6, 16, 20, 32, 36, 64, 68, 128, 132 };
    const long wss[] = { -1, 0, 64, 1 << 20, 32L << 20, 1L << 50 };
    long calls = 0, ok = 0;
    for (int N : ext) for (int L : ext) for (int heads : ext) for (int d : ds) for (int aligned = 0; aligned < 2; aligned++) for (long ws : wss) {
        const int causal = (int)(calls & 1);
        int out[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
        const int rc = t4k_attention_plan(N, L, heads, d, causal, aligned, ws, out);
        calls++;
        int want = T4K_OK;
        i128 need = 0;
        if (N < 1 || L < 1 || heads < 1 || ws < 0) want = T4K_ERR_ARG;
        else if (d < 4 || d > 128 || d % 4 != 0) want = T4K_ERR_UNSUPPORTED;
        else if ((i128)N * L * 3 * heads * d >= ((i128)1 << 31)) want = T4K_ERR_UNSUPPORTED;
        else { need = (i128)4 * N * heads * L; if (need > (i128)ws) want = T4K_ERR_UNSUPPORTED; }
        if (rc != want) { printf("verdict: N %d L %d heads %d d %d aligned %d ws %ld -> %d, the rule says %d\n", N, L, heads, d, aligned, ws, rc, want); return 1; }
        if (rc != T4K_OK) {
            for (int v : out) if (v != -7) { printf("a refusal wrote out\n"); return 1; }
            if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
            continue;
        }
        ok++;
        const int rung = d <= 16 ? 1 : d <= 32 ? 2 : d <= 64 ? 3 : 4;
        const i128 wgs = (i128)N * heads * (((i128)L + 63) / 64);
        const int exp[8] = { rung, aligned ? 4 : 1, 64, rung == 4 ? 32 : 64, 1, 2, (int)wgs, (int)need };
        for (int k = 0; k < 8; k++)
            if (out[k] != exp[k]) { printf("out[%d]: N %d L %d heads %d d %d aligned %d -> %d, the rule says %d\n", k, N, L, heads, d, aligned, out[k], exp[k]); return 1; }
    }
    if (t4k_attention_plan(1, 1, 1, 4, 0, 1, 64, nullptr) != T4K_ERR_ARG) { printf("null out\n"); return 1; }
    printf("t4k_attention_plan: %ld calls, %ld admitted, all as the rule says\n", calls + 1, ok);
    return 0;
}
