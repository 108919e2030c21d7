// conv_grp_plan_check.cpp - t4k_conv2d_grp_plan (csrc/conv_group.hip) over its admission grid, for a host build under sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Iinclude -Itensorforth_amd/csrc -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tensorforth_amd/csrc/conv_group.hip tools/conv_grp_plan_check.cpp -Ltensorforth_amd -lt4hip -Wl,-rpath,$PWD/tensorforth_amd -o build/conv_grp_plan_check
//   build/conv_grp_plan_check
// (from the repository root, after the library is built: conv_group.hip's host code is compiled again here, instrumented, and the program's own definitions
// of the three entries take precedence over the library's; the library supplies the error text and the state the launch entries look at.)
// Pure host arithmetic: nothing is launched and no device is needed.  K, S, P, D on and either side of their limits x extents around the 2^31 limits x channel
// pairs up to the slab limit and the grid limit x G in {-1, 0, 1, 2, 3, 64, C1, C1 + 1}; every call is held against the admission rule restated here in 128-bit arithmetic, every admitted plan against the
// rule of the slices and the lanes, and a refusal must leave a text and write nothing.
#include <cstdio>
#include <cstring>
#include "t4k.h"

int main() {
    const int ext[] = { -1, 0, 1, 7, 1 << 10, 1 << 16, (1 << 27) - 1, 1 << 27, 0x7fffffff }, exn[] = { 0, 1, 7, 1 << 20, 0x7fffffff }, exw[] = { 0, 1, 7, 1 << 16, 0x7fffffff };
    const int chan[][2] = { { 0, 4 }, { 4, 0 }, { 1, 1 }, { 3, 6 }, { 4, 8 }, { 12, 20 }, { 64, 64 }, { 2624, 4096 }, { 2688, 4096 }, { 1 << 22, 1 << 22 }, { 0x7fffffff, 0x7fffffff } };
    long calls = 0, ok = 0;
    for (int K : { -1, 0, 1, 3, 7, 8 }) for (int S : { 0, 1, 2, 4, 5 }) for (int P : { -1, 0, 2, 7 }) for (int D : { 0, 1, 2, 4, 5 })
        for (int N : exn) for (int H1 : ext) for (int W1 : exw) for (const auto &c : chan) {
            const int C1 = c[0], C0 = c[1];
            const int groups[] = { -1, 0, 1, 2, 3, 64, C1, C1 == 0x7fffffff ? 5 : C1 + 1 };
            for (int G : groups) for (int aligned = 0; aligned < 4; aligned += 3) {
                int out[8]; for (int &v : out) v = -7;
                const int rc = t4k_conv2d_grp_plan(N, H1, W1, C1, C0, K, S, P, D, G, aligned, out);
                calls++;
                bool admit = N >= 1 && H1 >= 1 && W1 >= 1 && C1 >= 1 && C0 >= 1 && K >= 1 && K <= 7 && S >= 1 && S <= 4 && D >= 1 && D <= 4 && P >= 0 && P <= D * (K - 1) &&
                             G >= 1 && C1 % G == 0 && C0 % G == 0;
                __int128 h0 = 0, w0 = 0, slab = 0;
                if (admit) {
                    const __int128 eh = (__int128)H1 + 2 * P - D * (K - 1) - 1, ew = (__int128)W1 + 2 * P - D * (K - 1) - 1, lim = (__int128)1 << 31;
                    admit = eh >= 0 && ew >= 0;
                    if (admit) {
                        h0 = eh / S + 1; w0 = ew / S + 1; slab = ((__int128)(C1 / G) * K * K + 1) * C0;
                        admit = (__int128)N * h0 * w0 < lim && (__int128)N * H1 * W1 < lim && slab * 4 <= ((__int128)32 << 20);
                    }
                }
                // the plan of an admitted layer; a layer whose dF grid (Cg1 x channel tiles) passes 65535 either way is refused too
                const int Cg1 = admit ? C1 / G : 1, Cg0 = admit ? C0 / G : 1;
                const bool v4 = (aligned & 1) && C0 % 4 == 0;
                const int mode = !v4 ? 0 : (Cg1 == 1 && Cg0 == 1) ? 1 : Cg0 % 4 == 0 ? 2 : Cg1 == 1 ? 3 : 0;
                const long cv = mode ? C0 / 4 : C0;
                long lanes = 1; while (lanes < 32 && lanes < cv) lanes *= 2;
                const long ctiles = (cv + lanes - 1) / lanes;
                if (admit && (Cg1 > 65535 || ctiles > 65535)) admit = false;
                if ((rc == T4K_OK) != admit) { printf("admission: N %d H1 %d W1 %d C1 %d C0 %d K %d S %d P %d D %d G %d -> %d\n", N, H1, W1, C1, C0, K, S, P, D, G, rc); return 1; }
                if (rc != T4K_OK) {
                    if (rc != T4K_ERR_ARG && rc != T4K_ERR_UNSUPPORTED) { printf("code %d\n", rc); return 1; }
                    const bool arg = N < 1 || H1 < 1 || W1 < 1 || C1 < 1 || C0 < 1;
                    if ((rc == T4K_ERR_ARG) != arg) { printf("an extent below 1 is T4K_ERR_ARG and nothing else is: %d\n", rc); return 1; }
                    for (int v : out) if (v != -7) { printf("a refusal wrote\n"); return 1; }
                    if (!t4k_last_error()[0]) { printf("a refusal left no text\n"); return 1; }
                    continue;
                }
                ok++;
                const long tiles = (long)Cg1 * ctiles, np0 = (long)((__int128)N * h0 * w0);
                long want = (1024 + tiles - 1) / tiles; const long fit = (long)(((__int128)2 << 20) / slab);
                if (want > fit) want = fit;
                if (want < 1) want = 1;
                const long pps = ((np0 + want - 1) / want + 31) / 32 * 32;
                const long nslice = (np0 + pps - 1) / pps;
                const int want_out[8] = { Cg1 == 1 ? 1 : 2, mode, mode == 1 ? 4 : 1, (int)lanes, (int)(256 / lanes / K), (int)nslice, (nslice <= 32 && !(aligned & 2)) ? 1 : 2, 3 };
                if (memcmp(out, want_out, sizeof out)) {
                    printf("plan: N %d H1 %d W1 %d C1 %d C0 %d K %d S %d P %d D %d G %d aligned %d -> {%d %d %d %d %d %d %d %d}\n", N, H1, W1, C1, C0, K, S, P, D, G, aligned,
                           out[0], out[1], out[2], out[3], out[4], out[5], out[6], out[7]);
                    return 1;
                }
                if (nslice < 1 || (nslice != 1 && nslice * (long)slab > (2L << 20))) { printf("slabs beyond 8 MiB\n"); return 1; }
            }
        }
    printf("t4k_conv2d_grp_plan: %ld calls, %ld admitted, all as the rule says\n", calls, ok);
    return 0;
}
