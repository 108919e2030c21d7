// linalg_plan_check.cpp - t4k_linalg_batched_plan (csrc/linalg_batched.hip) around every limit, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/linalg_batched.hip tools/linalg_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/linalg_plan_check
//   build/linalg_plan_check
// (from the repository root, after the library is built: the unit's host code is compiled again here, instrumented, and the program's own definitions
// take precedence over the library's; the library supplies the error text.)  Pure host arithmetic: nothing is launched and no device is needed.
// Entries -1 .. 4, K around 0, 32, 140, 200, 1024 and INT_MAX, batches around 0, 4 and INT_MAX, both load paths: each verdict and out[] against the rule restated.
#include <cstdio>
#include "t4k.h"

static long words(long K, long mats) { return (mats * K * (K | 1) + 2 * K + 12 + 3) & ~3L; }

int main() {
    const int Ks[] = { -2147483647 - 1, -1, 0, 1, 2, 4, 5, 8, 9, 16, 17, 31, 32, 33, 139, 140, 141, 192, 193, 199, 200, 201, 202, 204, 223, 224, 1023, 1024, 1025, 0x7fffffff };
    const int Bs[] = { -2147483647 - 1, -1, 0, 1, 3, 4, 5, 0x7ffffffc, 0x7ffffffd, 0x7fffffff };
    long calls = 0, ok = 0;
    for (int e = -1; e <= 4; e++) for (int K : Ks) for (int b : Bs) for (int al = 0; al < 2; al++) {
        int out[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
        const int rc = t4k_linalg_batched_plan(e, K, b, al, out);
        calls++;
        const int want = (e < 0 || e > 3 || K <= 0 || b < 0) ? T4K_ERR_ARG : K > 1024 ? T4K_ERR_UNSUPPORTED : T4K_OK;
        if (rc != want) { printf("verdict: entry %d K %d batch %d -> %d, the rule says %d\n", e, K, b, rc, want); return 1; }
        if (rc != T4K_OK) {
            for (int v : out) if (v != -7) { printf("a refusal wrote out\n"); return 1; }
            if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
            continue;
        }
        ok++;
        const bool two = e == 0 || e == 2, vec = al && (long)K * K % 4 == 0;
        const long mats = two ? 2 : 1;
        long ex[8] = { 0, 256, 0, 0, 1, b, vec ? 4 : 1, 0 };
        if (K <= 32) { ex[3] = 16 * words(K, mats); ex[5] = ((long)b + 3) / 4; }
        else if (K <= (two ? 140 : 200)) { ex[0] = 1; ex[3] = 4 * words(K, mats); }
        else if (two && K <= 192) { ex[0] = 2; ex[3] = 4 * words(K, 0); ex[6] = 1; }
        else {
            long panel = ((K + 31L) & ~31L) * 33;
            if (two && panel < 8 * 32 * 33) panel = 8 * 32 * 33;              // the substitution's tiles: four waves, two [32][33] each
            ex[0] = 3; ex[2] = 32; ex[3] = 4 * ((panel + 32 + K + 12 + 3) & ~3L); ex[6] = (al && K % 4 == 0) ? 4 : 1;
        }
        if (ex[3] > 160 * 1024) { printf("LDS: entry %d K %d needs %ld bytes\n", e, K, ex[3]); return 1; }
        for (int k = 0; k < 8; k++)
            if (out[k] != ex[k]) { printf("out[%d]: entry %d K %d batch %d aligned %d -> %d, the rule says %ld\n", k, e, K, b, al, out[k], ex[k]); return 1; }
    }
    if (t4k_linalg_batched_plan(1, 4, 1, 1, nullptr) != T4K_ERR_ARG) { printf("null out\n"); return 1; }
    calls++;
    printf("t4k_linalg_batched_plan: %ld calls, %ld admitted, all as the rule says\n", calls, ok);
    return 0;
}
