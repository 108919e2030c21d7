// token_ce_plan_check.cpp - t4k_token_ce_plan (csrc/token_ce.hip) around every limit, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/token_ce.hip tools/token_ce_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/token_ce_plan_check
//   build/token_ce_plan_check
// (from the repository root, after the library is built: token_ce.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  Tokens around 0, 1, a score workgroup, the score's widest launch and 2^31, classes
// around every team switch, both register limits on both load paths, 2^24 and the int's end, workspaces from nothing to plenty: each verdict and each out[]
// against the rule restated here in 128-bit arithmetic.
#include <cstdio>
#include "t4k.h"

typedef __int128 i128;
static i128 cdiv(i128 a, i128 b) { return (a + b - 1) / b; }
static i128 min2(i128 a, i128 b) { return a < b ? a : b; }

int main() {
    const long ts[] = { -1, 0, 1, 2, 63, 64, 65, 127, 128, 255, 256, 257, 511, 512, 513, 4096, 65535, 65536, 65537, 1L << 20, 0x7ffffffL, 0x8000000L, 0x3fffffffL, 0x40000000L,
                        0x7fffffffL, 0x80000000L, 1L << 40, 0x7fffffffffffffffL };
    const int vs[] = { -3, 0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260, 511, 512, 513, 1024, 1028, 2044, 2047, 2048, 2049, 2052,
                       8188, 8191, 8192, 8193, 8196, 32768, 50257, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0x7fffffff };
    const long wss[] = { -1, 0, 15, 16, 31, 32, 4095, 4096, 32L << 20, 1L << 50 };
    long calls = 0, ok = 0;
    for (long T : ts) for (int V : vs) for (int aligned = 0; aligned < 2; aligned++) for (long ws : wss) {
        int out[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
        const int rc = t4k_token_ce_plan(T, V, aligned, ws, out);
        calls++;
        int want = T4K_OK; i128 exp[8] = { 0, 1, 1, 1, 1, 0, 1, 0 };
        if (T < 1 || V < 2 || ws < 0) want = T4K_ERR_ARG;
        else if (V > (1 << 24) || (i128)T * V >= ((i128)1 << 31)) want = T4K_ERR_UNSUPPORTED;
        else {
            const int vw = (aligned && V % 4 == 0) ? 4 : 1, items = V / vw;
            exp[1] = vw;
            if (items <= 512) { i128 tl = 1; while (tl < 64 && tl * 4 < items) tl *= 2; exp[2] = tl; exp[3] = 64 / tl; }
            else { exp[0] = items <= 2048 ? 1 : 2; exp[2] = 256; if (items > 2048) { exp[4] = 2; exp[5] = cdiv(items, 2048) + 1; } }
            const i128 swg = min2(cdiv(T, 256), 256);
            if (swg > 1 && swg * 16 <= ws) { exp[6] = 2; exp[7] = swg * 16; }
            if (exp[2] * 8 < items && exp[0] < 2) { printf("the rule itself: V %d: %ld lanes do not hold %d items\n", V, (long)exp[2], items); return 1; }
        }
        if (rc != want) { printf("verdict: T %ld V %d aligned %d ws %ld -> %d, the rule says %d\n", T, V, aligned, ws, rc, want); return 1; }
        if (rc != T4K_OK) {
            for (int v : out) if (v != -7) { printf("a refusal wrote out\n"); return 1; }
            if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
            continue;
        }
        ok++;
        for (int k = 0; k < 8; k++)
            if (out[k] != exp[k]) { printf("out[%d]: T %ld V %d aligned %d ws %ld -> %d, the rule says %ld\n", k, T, V, aligned, ws, out[k], (long)exp[k]); return 1; }
    }
    if (t4k_token_ce_plan(8, 8, 1, 64, nullptr) != T4K_ERR_ARG) { printf("null out\n"); return 1; }
    printf("t4k_token_ce_plan: %ld calls, %ld admitted, all as the rule says\n", calls + 1, ok);
    return 0;
}
