// lane_ops.h - wave-wide xor butterflies (sum, max, first arg-max) on the vector ALUs of gfx950, NR rows side by side.
//
// Self-contained: no includes, plain __device__ __forceinline__ templates.  The Makefile embeds this text in front of the conv-stack source that
// hipRTC compiles (conv_stack_kernels.hip.inc); the ahead-of-time units may include it behind <hip/hip_runtime.h>.
//
// What it replaces: `for (off = 32; off; off >>= 1) a += __shfl_xor(a, off, 64)` comes out as six ds_bpermute_b32, each a trip through the LDS
// crossbar behind an s_waitcnt lgkmcnt - six dependent exchange latencies per reduction.  gfx950 can form every step's partner on the vector ALUs:
//     xor 32   v_permlane32_swap_b32            xor 4   DPP quad_perm:[3,2,1,0] then row_half_mirror   (i ^ 3 ^ 7 = i ^ 4)
//     xor 16   v_permlane16_swap_b32            xor 2   DPP quad_perm:[2,3,0,1]
//     xor 8    DPP row_ror:8                    xor 1   DPP quad_perm:[1,0,3,2]
// The steps run in the order 32, 16, 8, 4, 2, 1 and every step pairs lane i with lane i ^ off: each lane ends with the bits the __shfl_xor loop
// gave it (fp32 add is commutative bit for bit; fmaxf is too for everything but zeros of mixed sign, which the upper half of a swap step sees in
// the other operand order).  All NR rows take a step before the next step starts, so the rows' chains overlap as they did through the crossbar.
//
// CALL SITES MUST BE WAVE-UNIFORM WITH ALL 64 LANES LIVE.  DPP and the lane swaps read their source lanes whatever EXEC says: a lane switched off
// by a divergent branch still delivers whatever its register holds, and receives nothing.  Dead elements of a row are filled by the caller (0 for
// a sum; -FLT_MAX and index 0x7fffffff for the max forms), never masked off.  In the classifier head the softmax runs under `tid < 64` (wave 0,
// whole) and the matvec and the second linear layer run in uniform code.  Do not call these from divergent code.
#ifndef LANE_OPS_H
#define LANE_OPS_H

// the value lane i ^ OFF holds, OFF = 8, 4, 2 or 1 (within a row of 16 lanes: DPP)
template <int OFF> __device__ __forceinline__ unsigned lane_dpp_xor(unsigned v) {
    static_assert(OFF == 8 || OFF == 4 || OFF == 2 || OFF == 1, "DPP reaches within a row of 16 lanes");
    if (OFF == 8) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);                              // row_ror:8
    if (OFF == 4) return (unsigned)__builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, (int)v, 0x1B, 0xf, 0xf, true), 0x141, 0xf, 0xf, true);   // quad_perm:[3,2,1,0], row_half_mirror
    if (OFF == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);                               // quad_perm:[2,3,0,1]
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);                                             // quad_perm:[1,0,3,2]
}
template <int OFF> __device__ __forceinline__ float lane_dpp_xor_f(float v) { return __builtin_bit_cast(float, lane_dpp_xor<OFF>(__builtin_bit_cast(unsigned, v))); }
// The swap steps, OFF = 32 or 16.  Given v in both operands the instruction returns two registers: `lo` holds, in EVERY lane, the value of the
// lane of the pair {i, i ^ OFF} whose OFF bit is clear, `hi` that of the lane whose OFF bit is set.  A commutative step needs no more than
// op(lo, hi); the pair forms take the partner's value from lane_swap_partner.
struct LanePair { unsigned lo, hi; };
template <int OFF> __device__ __forceinline__ LanePair lane_swap(unsigned v) {
    static_assert(OFF == 32 || OFF == 16, "swap steps: halves of the wave, or neighbouring rows of 16");
    LanePair p;
    if (OFF == 32) { const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false); p.lo = r[0]; p.hi = r[1]; }
    else           { const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); p.lo = r[0]; p.hi = r[1]; }
    return p;
}
__device__ __forceinline__ unsigned lane_swap_partner(const LanePair &p, unsigned v) { return p.lo ^ p.hi ^ v; }   // the value lane i ^ OFF held: v is one of the two, this is the other

// a[r] <- sum over the wave of a[r], every lane, for r = 0 .. NR-1
template <int NR> __device__ __forceinline__ void lanes_sum_valu(float (&a)[NR]) {
#pragma unroll
    for (int r = 0; r < NR; r++) { const LanePair p = lane_swap<32>(__builtin_bit_cast(unsigned, a[r])); a[r] = __builtin_bit_cast(float, p.lo) + __builtin_bit_cast(float, p.hi); }
#pragma unroll
    for (int r = 0; r < NR; r++) { const LanePair p = lane_swap<16>(__builtin_bit_cast(unsigned, a[r])); a[r] = __builtin_bit_cast(float, p.lo) + __builtin_bit_cast(float, p.hi); }
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] += lane_dpp_xor_f<8>(a[r]);
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] += lane_dpp_xor_f<4>(a[r]);
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] += lane_dpp_xor_f<2>(a[r]);
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] += lane_dpp_xor_f<1>(a[r]);
}
// a[r] <- max over the wave of a[r] (fmaxf; no NaN expected), every lane
template <int NR> __device__ __forceinline__ void lanes_max_valu(float (&a)[NR]) {
#pragma unroll
    for (int r = 0; r < NR; r++) { const LanePair p = lane_swap<32>(__builtin_bit_cast(unsigned, a[r])); a[r] = __builtin_fmaxf(__builtin_bit_cast(float, p.lo), __builtin_bit_cast(float, p.hi)); }
#pragma unroll
    for (int r = 0; r < NR; r++) { const LanePair p = lane_swap<16>(__builtin_bit_cast(unsigned, a[r])); a[r] = __builtin_fmaxf(__builtin_bit_cast(float, p.lo), __builtin_bit_cast(float, p.hi)); }
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] = __builtin_fmaxf(a[r], lane_dpp_xor_f<8>(a[r]));
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] = __builtin_fmaxf(a[r], lane_dpp_xor_f<4>(a[r]));
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] = __builtin_fmaxf(a[r], lane_dpp_xor_f<2>(a[r]));
#pragma unroll
    for (int r = 0; r < NR; r++) a[r] = __builtin_fmaxf(a[r], lane_dpp_xor_f<1>(a[r]));
}
// (m[r], i[r]) <- the largest m of the wave and the LOWEST index among the lanes that hold it (k_hit's first-arg-max rule), every lane
__device__ __forceinline__ void lane_argmax_take(float &m, int &i, float m2, int i2) { if (m2 > m || (m2 == m && i2 < i)) { m = m2; i = i2; } }
template <int NR> __device__ __forceinline__ void lanes_argmax_valu(float (&m)[NR], int (&i)[NR]) {
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const LanePair pm = lane_swap<32>(__builtin_bit_cast(unsigned, m[r])), pi = lane_swap<32>((unsigned)i[r]);
        lane_argmax_take(m[r], i[r], __builtin_bit_cast(float, lane_swap_partner(pm, __builtin_bit_cast(unsigned, m[r]))), (int)lane_swap_partner(pi, (unsigned)i[r]));
    }
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const LanePair pm = lane_swap<16>(__builtin_bit_cast(unsigned, m[r])), pi = lane_swap<16>((unsigned)i[r]);
        lane_argmax_take(m[r], i[r], __builtin_bit_cast(float, lane_swap_partner(pm, __builtin_bit_cast(unsigned, m[r]))), (int)lane_swap_partner(pi, (unsigned)i[r]));
    }
#pragma unroll
    for (int r = 0; r < NR; r++) lane_argmax_take(m[r], i[r], lane_dpp_xor_f<8>(m[r]), (int)lane_dpp_xor<8>((unsigned)i[r]));
#pragma unroll
    for (int r = 0; r < NR; r++) lane_argmax_take(m[r], i[r], lane_dpp_xor_f<4>(m[r]), (int)lane_dpp_xor<4>((unsigned)i[r]));
#pragma unroll
    for (int r = 0; r < NR; r++) lane_argmax_take(m[r], i[r], lane_dpp_xor_f<2>(m[r]), (int)lane_dpp_xor<2>((unsigned)i[r]));
#pragma unroll
    for (int r = 0; r < NR; r++) lane_argmax_take(m[r], i[r], lane_dpp_xor_f<1>(m[r]), (int)lane_dpp_xor<1>((unsigned)i[r]));
}
#endif
