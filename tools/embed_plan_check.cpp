// embed_plan_check.cpp - t4k_embed_plan (csrc/embed.hip) around every limit, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/embed.hip tools/embed_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/embed_plan_check
//   build/embed_plan_check
// (from the repository root, after the library is built: embed.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the three entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  Tokens around 0, 1, every part and id-load boundary and 2^31, vocabularies on both sides
// of a slab and of a full device, widths on both sides of a chunk on both load paths, position flags that are none, workspaces from nothing to plenty: each
// verdict and each out[] against the rule restated here in 128-bit arithmetic.
#include <cstdio>
#include "t4k.h"

typedef __int128 i128;
static i128 cdiv(i128 a, i128 b) { return (a + b - 1) / b; }
static i128 min2(i128 a, i128 b) { return a < b ? a : b; }
static i128 max2(i128 a, i128 b) { return a > b ? a : b; }

int main() {
    const long ts[] = { -1, 0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2304, 2305, 16384, 25088, 65536, (1L << 20) + 3, (1L << 21) - 1, 1L << 21,
                        0x7ffffffcL, 0x7fffffffL, 0x80000000L, 0x80000001L, 1L << 40, 0x7fffffffffffffffL };
    const int ls[] = { -3, 0, 1, 2, 5, 64, 65, 196, 512 };
    const int vs[] = { -1, 0, 1, 15, 16, 17, 35, 64, 65, 1000, 16367, 16368, 16369, 16384, 16385, 32768, 1 << 21, 1 << 27, 0x7fffffff };
    const int es[] = { -4, 0, 1, 3, 4, 5, 20, 63, 64, 65, 68, 128, 252, 256, 257, 260, 512, 1024, 1 << 20, 0x7fffffff };
    const int poss[] = { -1, 0, 1, 2 };
    const long wss[] = { -1, 0, 3, 4, 255, 256, 1023, 1024, 65536, 32L << 20, 0x7fffffffL, 0x80000000L, 1L << 50 };
    long calls = 0, ok = 0;
    for (long T : ts) for (int L : ls) for (int V : vs) for (int E : es) for (int pos : poss) for (int aligned = 0; aligned < 2; aligned++) for (long ws : wss) {
        int out[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
        const int rc = t4k_embed_plan(T, L, V, E, pos, aligned, ws, out);
        calls++;
        int want = T4K_OK; i128 exp[8] = { 0, 0, 0, 1, 1, 1, 0, 0 };
        if (T < 1 || L < 1 || E < 1 || V < 0 || T % L || ws < 0 || pos < 0 || pos > 1 || (V == 0 && pos == 0)) want = T4K_ERR_ARG;
        else if ((i128)T >= ((i128)1 << 31) || (i128)T * E >= ((i128)1 << 31) || (i128)V * E >= ((i128)1 << 31)) want = T4K_ERR_UNSUPPORTED;
        else {
            const int vw = (aligned && E % 4 == 0) ? 4 : 1, items = E / vw;
            const i128 pwg = pos ? cdiv((i128)L * items, 16) : 0;
            exp[1] = vw; exp[6] = pwg;
            if (V > 0) {
                const i128 base = cdiv(V, 16) * cdiv(items, 64), bytes = (i128)4 * V * E;
                i128 P = max2(1, min2(min2(cdiv(1024, base), max2(1, T / 64)), min2(ws, 0x7fffffffL) / bytes));
                const i128 per = cdiv(cdiv(T, 64), P) * 64;
                P = cdiv(T, per);
                exp[0] = P > 1 ? 2 : 1; exp[2] = 16; exp[3] = P; exp[5] = exp[0]; exp[6] = cdiv(base * P, 4) + pwg; exp[7] = P > 1 ? P * bytes : 0;
                if (exp[7] > min2(ws, 0x7fffffffL) || exp[6] >= ((i128)1 << 31) || P > 1024) { printf("the rule itself: T %ld V %d E %d: %ld parts\n", T, V, E, (long)P); return 1; }
            }
        }
        if (rc != want) { printf("verdict: T %ld L %d V %d E %d pos %d aligned %d ws %ld -> %d, the rule says %d\n", T, L, V, E, pos, aligned, ws, rc, want); return 1; }
        if (rc != T4K_OK) {
            for (int v : out) if (v != -7) { printf("a refusal wrote out\n"); return 1; }
            if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
            continue;
        }
        ok++;
        for (int k = 0; k < 8; k++)
            if (out[k] != exp[k]) { printf("out[%d]: T %ld L %d V %d E %d pos %d aligned %d ws %ld -> %d, the rule says %ld\n", k, T, L, V, E, pos, aligned, ws, out[k], (long)exp[k]); return 1; }
    }
    if (t4k_embed_plan(10, 5, 7, 4, 1, 1, 64, nullptr) != T4K_ERR_ARG) { printf("null out\n"); return 1; }
    printf("t4k_embed_plan: %ld calls, %ld admitted, all as the rule says\n", calls + 1, ok);
    return 0;
}
