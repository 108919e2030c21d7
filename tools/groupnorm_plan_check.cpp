// groupnorm_plan_check.cpp - t4k_groupnorm_plan (csrc/groupnorm.hip) around every limit, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/groupnorm.hip tools/groupnorm_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/groupnorm_plan_check
//   build/groupnorm_plan_check
// (from the repository root, after the library is built: groupnorm.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the three entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  Extents around 1 and 2^31, G in { -1, 0, 1, 2, 3, C, C + 1 }, both load paths, workspaces
// from nothing to plenty: each verdict and each out[] against the rule restated here in 128-bit arithmetic.
#include <cstdio>
#include "t4k.h"

typedef __int128 i128;
static i128 cdiv(i128 a, i128 b) { return (a + b - 1) / b; }
static i128 min2(i128 a, i128 b) { return a < b ? a : b; }

int main() {
    const int ext[] = { -1, 0, 1, 2, 3, 4, 7, 8, 12, 63, 64, 65, 260, 512, 513, 1 << 12, (1 << 12) + 1, 4100, 1 << 16, (1 << 20) + 4, 0x7ffffffc, 0x7fffffff };
    const long wss[] = { -1, 0, 64, 1 << 20, 32L << 20, 1L << 50 };
    long calls = 0, ok = 0;
    for (int N : ext) for (int HW : ext) for (int C : ext) {
        const int gs[] = { -1, 0, 1, 2, 3, C, C == 0x7fffffff ? C : C + 1 };
        for (int G : gs) for (int aligned = 0; aligned < 2; aligned++) for (long ws : wss) {
            int out[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
            const int rc = t4k_groupnorm_plan(N, HW, C, G, aligned, ws, out);
            calls++;
            int want = T4K_OK;
            i128 rung = 0, vw = 1, P = 1, ns = 0;
            if (N < 1 || HW < 1 || C < 1 || ws < 0) want = T4K_ERR_ARG;
            else if (G < 1 || C % G != 0 || (i128)N * HW * C >= ((i128)1 << 31) || (i128)N * G >= ((i128)1 << 31)) want = T4K_ERR_UNSUPPORTED;
            else {
                const i128 Cg = C / G, NG = (i128)N * G;
                vw = (aligned && Cg % 4 == 0) ? 4 : 1;
                const i128 cgv = Cg / vw;
                rung = 3;
                const int dw = vw == 1 ? 2 : 1;                         // rows a thread keeps: 8 on rung 1; 4 of 16 bytes or 8 dwords on rung 2
                if (cgv <= 64 && cdiv(HW, 64 / cgv) <= 8) rung = 1;
                else if (cgv <= 1024 && cdiv(HW, 1024 / cgv) <= 4 * dw) rung = 2;
                else if (NG < 256) {
                    const i128 w = min2(min2(cdiv(1024, NG), 64), min2(HW, (i128)HW * cgv / 1024));
                    if (w >= 2) { const i128 rp = cdiv(HW, w); P = cdiv(HW, rp); if (P >= 2) rung = 4; else P = 1; }
                }
                ns = (i128)N * P;
                const i128 parts = rung == 4 ? (2 * NG * P + 3) / 4 * 4 : 0;
                if ((parts + ns * 2 * C) * 4 > (i128)ws / 4 * 4) want = T4K_ERR_UNSUPPORTED;
            }
            if (rc != want) { printf("verdict: N %d HW %d C %d G %d aligned %d ws %ld -> %d, the rule says %d\n", N, HW, C, G, aligned, ws, rc, want); return 1; }
            if (rc != T4K_OK) {
                for (int v : out) if (v != -7) { printf("a refusal wrote out\n"); return 1; }
                if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
                continue;
            }
            ok++;
            const int exp[8] = { (int)rung, (int)vw, rung == 1 ? 4 : 1, (int)P, rung == 4 ? 2 : 1, (int)ns, ns <= 32 ? 1 : 2, rung == 4 ? 3 : 2 };
            for (int k = 0; k < 8; k++)
                if (out[k] != exp[k]) { printf("out[%d]: N %d HW %d C %d G %d aligned %d -> %d, the rule says %d\n", k, N, HW, C, G, aligned, out[k], exp[k]); return 1; }
        }
    }
    if (t4k_groupnorm_plan(1, 1, 1, 1, 1, 64, nullptr) != T4K_ERR_ARG) { printf("null out\n"); return 1; }
    printf("t4k_groupnorm_plan: %ld calls, %ld admitted, all as the rule says\n", calls + 1, ok);
    return 0;
}
