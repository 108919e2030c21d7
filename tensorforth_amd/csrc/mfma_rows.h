// mfma_rows.h - what the units that own 16 token rows per wave share (attention.hip, retention.hip): v_mfma_f32_16x16x4_f32 on quads of k,
// the LDS tiles of the streamed side with their conflict-free pitch, and the wave's own rows kept in registers.
#pragma once
#include "t4k_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// LDS row pitch in floats: DP + 4 is 4 mod 32 for every DP here.  The transposed reads (ds_read_b32, lane -> row 4 (lane >> 4) + r, column lane & 15) then
// fall on banks 16 (lane >> 4) + (lane & 15) mod 32: no conflict inside a 32-lane half; the row reads (ds_read_b128, lane -> row lane & 15, column 4 (lane >> 4))
// start on bank 4 (row + (lane >> 4)) mod 64: 16 distinct slots in three of the four lane groups, one shared slot in the fourth
constexpr int at_pitch(int DP) { return DP + 4; }

template <int VW> __device__ __forceinline__ float4 at_ld(const float *q) {
    if constexpr (VW == 4) return *reinterpret_cast<const float4 *>(q);
    else return make_float4(q[0], q[1], q[2], q[3]);
}
template <int VW> __device__ __forceinline__ void at_st(float *q, const float4 v) {
    if constexpr (VW == 4) *reinterpret_cast<float4 *>(q) = v;
    else { q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
}
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// c += A B over 4 x 4 values of k: the quad a from LDS (or registers), the quad b from registers
__device__ __forceinline__ f32x4 mfma_quad(const float4 a, const float4 b, f32x4 c) {
    c = mfma4(a.x, b.x, c); c = mfma4(a.y, b.y, c); c = mfma4(a.z, b.z, c); c = mfma4(a.w, b.w, c);
    return c;
}
// rows [0, ROWS) x channels [0, DP) of a head's Q, K, V (row pitch 3E) or dY (row pitch E) into LDS, zeros beyond `rows` rows and d channels: every MFMA
// operand is a number.  All 256 threads.
template <int ROWS, int DP, int VW>
__device__ __forceinline__ void at_tile(float *lds, const float *src, long pitch, int rows, int d) {
    constexpr int C4 = DP / 4, P = at_pitch(DP);
    for (int it = (int)threadIdx.x; it < ROWS * C4; it += 256) {
        const int r = it / C4, c = (it - r * C4) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows && c < d) v = at_ld<VW>(src + (long)r * pitch + c);
        *reinterpret_cast<float4 *>(lds + r * P + c) = v;
    }
}
// the wave's own row `row` (pointer at its channel 0) as 16-byte quads: quad kc holds channels 16 kc + 4 g .. + 3
template <int DP, int VW>
__device__ __forceinline__ void at_row(float4 (&f)[DP / 16], const float *row, bool live, int g, int d) {
#pragma unroll
    for (int kc = 0; kc < DP / 16; kc++) {
        const int c = 16 * kc + 4 * g;
        f[kc] = (live && c < d) ? at_ld<VW>(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

} // namespace
