// fastdiv.h - division by a launch invariant without a divide, and the work-item digits built on it: what the kernels with run-time geometry share
// (pool_geo.hip, upsample.hip).
#pragma once
#include "t4k_common.h"

namespace {

// x / d for x below 2^31 without a divide instruction sequence: m = ceil(2^(31 + l) / d) with l = ceil(log2 d) fits 32 bits and (x m) >> (31 + l) is the
// quotient for every 31-bit x (Granlund & Montgomery, "Division by invariant integers using multiplication", PLDI 1994, theorem 4.2 with N = 31); d = 1 has
// m = 0 and passes x through.  The host works m out once per launch; a work item's digits and its window range cost a multiply and a shift each instead
// of the ~30 instructions of a 32-bit divide, which made the backward - seven divisions per 16 bytes stored - instruction-bound.
struct FastDiv { unsigned m, s, d; };
FastDiv fast_div(int d) {
    FastDiv f = { 0u, 0u, (unsigned)d };
    if (d > 1) {
        const int l = 32 - __builtin_clz((unsigned)d - 1);
        f.m = (unsigned)((((uint64_t)1 << (31 + l)) + (unsigned)d - 1) / (unsigned)d); f.s = (unsigned)(l - 1);
    }
    return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned x, const FastDiv &f) { return f.m ? __umulhi(x, f.m) >> f.s : x; }

// work item -> (channel group, column, row, image) of an [N][H][W][CV] grid; the pixel index comes back too.  Items that fit 31 bits (every tensor below
// 2^31 items) take the multiplies, the others the 64-bit divides of t4k_common.h
__device__ __forceinline__ void fd_digits(long z, int CV, int W, int H, const FastDiv &dCV, const FastDiv &dW, const FastDiv &dH,
                                          int &cv, int &j, int &i, int &n, long &pix) {
    if (z < 0x7fffffffL) {
        const unsigned q = (unsigned)z, px = fdiv(q, dCV), t = fdiv(px, dW), m = fdiv(t, dH);
        cv = (int)(q - px * (unsigned)CV); j = (int)(px - t * (unsigned)W); i = (int)(t - m * (unsigned)H); n = (int)m; pix = (long)px;
    } else { t4k::split2(z, CV, cv, pix); t4k::split3(pix, W, H, j, i, n); }
}

}
