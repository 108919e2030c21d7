// patch_plan_check.cpp - t4k_patch_plan (csrc/patch.hip) over its admission grid, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/patch.hip tools/patch_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/patch_plan_check
//   build/patch_plan_check
// (from the repository root, after the library is built: patch.hip's host code is compiled again here, instrumented, and the program's own definitions of
// the three entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  K on and either side of its limits x extents around the 2^31 limits x channel pairs up
// to the slab limit and the grid limit x every value of `aligned`; every call is held against the admission rule restated here in 128-bit arithmetic, every
// admitted plan against the rule of the load paths, the tiles and the slices, and a refusal must leave a text and write nothing.
#include <cstdio>
#include <cstring>
#include "t4k.h"

int main() {
    const int ext[] = { -1, 0, 1, 7, 8, 31, 32, 33, 224, 1 << 10, 1 << 16, (1 << 27) - 1, 1 << 27, 0x7fffffff }, exn[] = { 0, 1, 7, 128, 1 << 20, 0x7fffffff };
    const int chan[][2] = { { 0, 4 }, { 4, 0 }, { 1, 1 }, { 3, 6 }, { 3, 64 }, { 3, 768 }, { 4, 68 }, { 64, 127 }, { 64, 128 }, { 8191, 1 }, { 4096, 2 }, { 4095, 2 }, { 1 << 22, 1 << 22 }, { 0x7fffffff, 0x7fffffff } };
    long calls = 0, ok = 0;
    for (int K : { -1, 0, 1, 2, 4, 7, 8, 14, 16, 31, 32, 33 })
        for (int N : exn) for (int H1 : ext) for (int W1 : ext) for (const auto &c : chan) for (int aligned = 0; aligned < 16; aligned++) {
            const int C1 = c[0], C0 = c[1];
            int out[8]; for (int &v : out) v = -7;
            const int rc = t4k_patch_plan(N, H1, W1, C1, C0, K, aligned, out);
            calls++;
            const bool arg = N < 1 || H1 < 1 || W1 < 1 || C1 < 1 || C0 < 1;
            bool admit = !arg && K >= 2 && K <= 32 && H1 >= K && W1 >= K;
            const __int128 lim = (__int128)1 << 31;
            __int128 m = 0, kd = 0, slab = 0;
            if (admit) {
                m = (__int128)N * (H1 / K) * (W1 / K); kd = (__int128)K * K * C1; slab = (kd + 1) * C0;
                admit = (__int128)N * H1 * W1 * C1 < lim && m * C0 < lim && slab * 4 <= ((__int128)32 << 20);
            }
            if (admit) {                                             // what a launch takes: the dF grid's y and z within 65535, the 1-D grids of forward and dX within 2^31
                const __int128 tm = (m + 127) / 128, tn = ((__int128)C0 + 63) / 64;
                admit = (kd + 64) / 64 <= 65535 && tn <= 65535 && tm * tn < lim && tm * ((kd + 63) / 64) + 256 < lim;
            }
            if ((rc == T4K_OK) != admit) { printf("admission: N %d H1 %d W1 %d C1 %d C0 %d K %d -> %d\n", N, H1, W1, C1, C0, K, rc); return 1; }
            if (rc != T4K_OK) {
                if ((rc == T4K_ERR_ARG) != arg || (rc != T4K_ERR_ARG && rc != T4K_ERR_UNSUPPORTED)) { printf("an extent below 1 is T4K_ERR_ARG and nothing else is: %d\n", rc); return 1; }
                for (int v : out) if (v != -7) { printf("a refusal wrote\n"); return 1; }
                if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
                continue;
            }
            ok++;
            const bool vi = (aligned & 1) && (K * C1) % 4 == 0 && ((long)W1 * C1) % 4 == 0, vf = (aligned & 2) && C0 % 4 == 0, vd = (aligned & 4) && C0 % 4 == 0;
            const long tiles = (long)((kd + 64) / 64) * ((C0 + 63) / 64), np0 = (long)m;
            long want = (1024 + tiles - 1) / tiles; const long fit = (long)(((__int128)2 << 20) / slab);
            if (want > fit) want = fit;
            if (want < 1) want = 1;
            const long pps = ((np0 + want - 1) / want + 31) / 32 * 32;
            const long nslice = (np0 + pps - 1) / pps;
            const int want_out[8] = { (vi && vf && C0 > 64) ? 128 : 64, vi | (vf << 1), (vf && vd && kd > 64) ? 128 : 64, vf && vd, vi | (vd << 1),
                                      (int)nslice, (nslice <= 32 && !(aligned & 8)) ? 1 : 2, 3 };
            if (memcmp(out, want_out, sizeof out)) {
                printf("plan: N %d H1 %d W1 %d C1 %d C0 %d K %d aligned %d -> {%d %d %d %d %d %d %d %d}\n", N, H1, W1, C1, C0, K, aligned,
                       out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7]);
                return 1;
            }
            if (nslice < 1 || (nslice != 1 && nslice * (long)slab > (2L << 20))) { printf("slabs beyond 8 MiB\n"); return 1; }
        }
    printf("t4k_patch_plan: %ld calls, %ld admitted, all as the rule says\n", calls, ok);
    return 0;
}
