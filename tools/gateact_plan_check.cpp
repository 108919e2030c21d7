// gateact_plan_check.cpp - t4k_gateact_plan (csrc/gateact.hip) around every limit, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/gateact.hip tools/gateact_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/gateact_plan_check
//   build/gateact_plan_check
// (from the repository root, after the library is built: gateact.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  Tokens around 0, 1, a workgroup's chunk and 2^31, channels around the item, odd and
// even, and the int's end, every kind and gate and one beyond on either side: each verdict and each out[] against the rule restated here in 128-bit
// arithmetic.
#include <cstdio>
#include "t4k.h"

typedef __int128 i128;

int main() {
    const long ts[] = { -1, 0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 65537, 1L << 20, 0x7ffffffL, 0x8000000L, 0x3fffffffL, 0x40000000L,
                        0x7fffffffL, 0x80000000L, 1L << 40, 0x7fffffffffffffffL };
    const int cs[] = { -2, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 24, 520, 768, 1023, 1024, 1025, 2048, 4096, 4097, 8192, 0x3fffffff, 0x40000000, 0x7ffffffe, 0x7fffffff };
    long calls = 0, ok = 0;
    for (long T : ts) for (int C : cs) for (int kind = -1; kind <= 4; kind++) for (int gate = -1; gate <= 2; gate++) for (int aligned = 0; aligned < 2; aligned++) {
        int out[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
        const int rc = t4k_gateact_plan(T, C, kind, gate, aligned, out);
        calls++;
        int want = T4K_OK; i128 exp[8] = { 0, 1, 4, 0, 0, 1, 1, 0 };
        if (T < 1 || C < 1 || kind < 0 || kind > 3 || gate < 0 || gate > 1 || (gate == 1 && C % 2)) want = T4K_ERR_ARG;
        else if ((i128)T * C >= ((i128)1 << 31)) want = T4K_ERR_UNSUPPORTED;
        else {
            const i128 Hc = gate ? C / 2 : C, n = (i128)T * Hc;
            const int vw = (aligned && (gate ? Hc : n) % 4 == 0) ? 4 : 1;
            exp[0] = 2 * gate + (vw == 1); exp[1] = vw;
            exp[3] = exp[4] = (n / vw + 1023) / 1024;
            if (exp[3] < 1 || exp[3] * 1024 * vw < n || n % vw) { printf("the rule itself: T %ld C %d: %ld workgroups do not cover %ld elements\n", T, C, (long)exp[3], (long)n); return 1; }
        }
        if (rc != want) { printf("verdict: T %ld C %d kind %d gate %d aligned %d -> %d, the rule says %d\n", T, C, kind, gate, aligned, rc, want); return 1; }
        if (rc != T4K_OK) {
            for (int v : out) if (v != -7) { printf("a refusal wrote out\n"); return 1; }
            if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
            continue;
        }
        ok++;
        for (int k = 0; k < 8; k++)
            if (out[k] != exp[k]) { printf("out[%d]: T %ld C %d kind %d gate %d aligned %d -> %d, the rule says %ld\n", k, T, C, kind, gate, aligned, out[k], (long)exp[k]); return 1; }
    }
    if (t4k_gateact_plan(8, 8, 0, 0, 1, nullptr) != T4K_ERR_ARG) { printf("null out\n"); return 1; }
    printf("t4k_gateact_plan: %ld calls, %ld admitted, all as the rule says\n", calls + 1, ok);
    return 0;
}
