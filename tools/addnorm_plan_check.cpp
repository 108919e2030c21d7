// addnorm_plan_check.cpp - t4k_addnorm_plan (csrc/addnorm.hip) around every limit, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/addnorm.hip tools/addnorm_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/addnorm_plan_check
//   build/addnorm_plan_check
// (from the repository root, after the library is built: addnorm.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the three entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  Rows around 0, 1, every multiple of the tokens per workgroup times the slab rows and
// 2^31, channels on both sides of every T and rung limit of both load paths, the three modes and two that are none, workspaces from nothing to plenty: each
// verdict and each out[] against the rule restated here in 128-bit arithmetic.
#include <cstdio>
#include "t4k.h"

typedef __int128 i128;
static i128 cdiv(i128 a, i128 b) { return (a + b - 1) / b; }
static i128 min3(i128 a, i128 b, i128 c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }

int main() {
    const long rws[] = { -1, 0, 1, 2, 3, 4, 5, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 4097, 25088, 32768, 32769, 65536, 65537, (1L << 20) + 3, (1L << 21) - 1, 1L << 21,
                         0x7ffffffcL, 0x7fffffffL, 0x80000000L, 0x80000001L, 1L << 40, 0x7fffffffffffffffL };
    const int cs[] = { -8, 0, 1, 2, 3, 4, 5, 20, 63, 64, 65, 68, 127, 128, 129, 252, 256, 257, 260, 511, 512, 513, 516, 1024, 1025, 1028, 2047, 2048, 2049, 2052, 4096, 8188, 8192, 8193,
                       8196, 1 << 20, 0x7fffffff };
    const int modes[] = { -1, 0, 1, 2, 3 };
    const long wss[] = { -1, 0, 7, 8, 159, 160, 65536, 98304, 1 << 20, 32L << 20, 1L << 50 };
    long calls = 0, ok = 0;
    for (long rows : rws) for (int C : cs) for (int mode : modes) for (int aligned = 0; aligned < 2; aligned++) for (long ws : wss) {
        int out[8] = { -7, -7, -7, -7, -7, -7, -7, -7 };
        const int rc = t4k_addnorm_plan(rows, C, mode, aligned, ws, out);
        calls++;
        int want = T4K_OK, exp[8] = { 0, 0, 0, 0, 1, 0, 0, 1 };
        if (rows < 1 || C < 1 || mode < 0 || mode > 2 || ws < 0) want = T4K_ERR_ARG;
        else if ((i128)rows >= ((i128)1 << 31) || (i128)rows * C >= ((i128)1 << 31)) want = T4K_ERR_UNSUPPORTED;
        else {
            const int vw = (aligned && C % 4 == 0) ? 4 : 1, items = C / vw;
            exp[1] = vw;
            if (mode != 0) {
                int T = 0;
                for (int t = 8; t <= 64 && !T; t *= 2) if (cdiv(items, t) <= 8) T = t;
                if (!T && cdiv(items, 256) > 8) want = T4K_ERR_UNSUPPORTED;
                else {
                    exp[0] = T ? 1 : 2; if (!T) T = 256;
                    const int tpw = 256 / T;
                    const i128 visits = cdiv(rows, tpw), fit = (i128)(ws / 4) / ((i128)2 * C);
                    if (fit < 1) want = T4K_ERR_UNSUPPORTED;
                    else {
                        const i128 per = cdiv(visits, min3(visits, 1024, fit)) * tpw, nslice = cdiv(rows, per);
                        exp[2] = tpw; exp[3] = T; exp[5] = (int)nslice; exp[6] = nslice <= 32 ? 1 : 2; exp[7] = 2;
                        if (nslice > fit || nslice > 1024) { printf("the rule itself: %ld rows, C %d: %ld slab rows\n", rows, C, (long)nslice); return 1; }
                    }
                }
            }
        }
        if (rc != want) { printf("verdict: rows %ld C %d mode %d aligned %d ws %ld -> %d, the rule says %d\n", rows, C, mode, aligned, ws, rc, want); return 1; }
        if (rc != T4K_OK) {
            for (int v : out) if (v != -7) { printf("a refusal wrote out\n"); return 1; }
            if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
            continue;
        }
        ok++;
        for (int k = 0; k < 8; k++)
            if (out[k] != exp[k]) { printf("out[%d]: rows %ld C %d mode %d aligned %d ws %ld -> %d, the rule says %d\n", k, rows, C, mode, aligned, ws, out[k], exp[k]); return 1; }
    }
    if (t4k_addnorm_plan(1, 1, 1, 1, 64, nullptr) != T4K_ERR_ARG) { printf("null out\n"); return 1; }
    printf("t4k_addnorm_plan: %ld calls, %ld admitted, all as the rule says\n", calls + 1, ok);
    return 0;
}
