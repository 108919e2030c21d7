// gemm_batched.hip - batched / broadcast fp32 products in ONE launch (t4k_gemm_batched).
//
//   O[b] = alpha * op(A[b]) @ op(B[b]) + beta * O[b]   for b in [0, batch), per channel c in [0, C)
//
// The reference's tensor product (src/vm/tenvm.cpp:277-287 documents NumPy `@`, _tdot :328-366 implements the rank-2 and
// N-broadcast cases as one Tensor::mm per sample, src/mu/tensor.cu:161-180).  Operand b sits at A + b * sA; sA == 0 gives every
// entry the same A (likewise B).  cA == 1: A has one channel that serves every channel of the output (likewise cB).
//
// Two regimes:
//   * small matrices (M, N <= 64) and every channel-broadcast shape: one WAVE per output tile of one (entry, channel) pair, four
//     per workgroup, operands fetched straight into registers in the MFMA operand layout (no LDS, no barriers).  A 16x16, 32x32
//     or 64x64 tile covers a whole small matrix, so 128 products of 28 x 28 are 128 waves spread over the CUs instead of 128
//     launches each padding one 64x64 workgroup tile.  v_mfma_f32_16x16x4_f32 for M, N <= 16, v_mfma_f32_32x32x2_f32 above.
//   * large matrices with every channel present: the LDS-staged tile kernel of gemm.hip with the batch entry in grid.y
//     (k_gemm_mfma_batched, gemm_batched_tiles).
// Both are exact fp32 (the f32-input MFMA is a k-ordered fma chain; gfx950 has no xf32).  beta == 0 never reads O.
#include "t4k_common.h"

using namespace t4k;

namespace t4k {
int gemm_batched_tiles(const float *A, const float *B, float *O, float alpha, float beta, int tA, int tB,
                       int M, int N, int K, int C, int batch, long sA, long sB, long sO, hipStream_t hs);
}

namespace {

struct BmmP {
    const float *A, *B;
    float *O;
    float alpha, beta;
    int tA, tB, M, N, K, C, cA, cB;
    long sA, sB, sO;
    int tiles_m, tiles_n;              // wave tiles per matrix
    long items;                        // batch * C * tiles_m * tiles_n
};

template <int TS> struct Acc;
template <> struct Acc<32> { typedef float T __attribute__((ext_vector_type(16))); static constexpr int R = 16; };
template <> struct Acc<16> { typedef float T __attribute__((ext_vector_type(4)));  static constexpr int R = 4; };

// TS: MFMA shape (32: 32x32x2, 16: 16x16x4); a wave owns MT x NT of them.  Lane l feeds row / column l % TS at k slot l / TS
// (KPI = 64 / TS k-values per instruction); a step of four instructions covers 4 * KPI consecutive k.
template <int TS, int MT, int NT>
__global__ void __launch_bounds__(256) k_bmm_wave(BmmP p) {
    typedef typename Acc<TS>::T acc_t;
    constexpr int R = Acc<TS>::R, KPI = 64 / TS, KS = 4 * KPI;
    constexpr int NACC = (TS == 16 && MT * NT == 1) ? 2 : 1;   // 16x16x4: 40-cycle dependent latency over a 32-cycle issue
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= p.items) return;                                // whole waves only: nothing below synchronises
    const int M = p.M, N = p.N, K = p.K, C = p.C;
    const int tn = (int)(item % p.tiles_n);
    long r = item / p.tiles_n;
    const int tm = (int)(r % p.tiles_m); r /= p.tiles_m;
    const int c = (int)(r % C);
    const long b = r / C;
    const int cA = p.cA, cB = p.cB, ca = cA == 1 ? 0 : c, cb = cB == 1 ? 0 : c;
    const float *__restrict__ A = p.A + b * p.sA + ca;
    const float *__restrict__ B = p.B + b * p.sB + cb;
    const int row = lane % TS, ks = lane / TS;
    const int m0 = tm * (MT * TS), n0 = tn * (NT * TS);

    // element offsets (before the channel stride) of this lane's rows / columns; out-of-range ones are never loaded
    long am[MT], bn[NT];
    bool okm[MT], okn[NT];
#pragma unroll
    for (int i = 0; i < MT; i++) { const int m = m0 + i * TS + row; okm[i] = m < M; am[i] = p.tA ? m : (long)m * K; }
#pragma unroll
    for (int j = 0; j < NT; j++) { const int n = n0 + j * TS + row; okn[j] = n < N; bn[j] = p.tB ? (long)n * K : n; }
    const long akstep = p.tA ? M : 1, bkstep = p.tB ? 1 : N;

    acc_t acc[MT][NT][NACC];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int q = 0; q < NACC; q++)
#pragma unroll
                for (int e = 0; e < R; e++) acc[i][j][q][e] = 0.f;

    float av[2][MT][4], bv[2][NT][4];
    auto load = [&](int k0, float (&a)[MT][4], float (&bb)[NT][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const int k = k0 + s * KPI + ks;
            const bool okk = k < K;
#pragma unroll
            for (int i = 0; i < MT; i++) a[i][s] = (okk && okm[i]) ? A[(am[i] + k * akstep) * cA] : 0.f;
#pragma unroll
            for (int j = 0; j < NT; j++) bb[j][s] = (okk && okn[j]) ? B[(bn[j] + k * bkstep) * cB] : 0.f;
        }
    };
    auto mma = [&](float (&a)[MT][4], float (&bb)[NT][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int i = 0; i < MT; i++)
#pragma unroll
                for (int j = 0; j < NT; j++) {
                    if constexpr (TS == 32) acc[i][j][s % NACC] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][s], bb[j][s], acc[i][j][s % NACC], 0, 0, 0);
                    else                    acc[i][j][s % NACC] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][s], bb[j][s], acc[i][j][s % NACC], 0, 0, 0);
                }
    };
    // one step of loads in flight under the MFMAs of the previous one
    const int nst = (K + KS - 1) / KS;
    if (nst > 0) load(0, av[0], bv[0]);
    for (int kt = 0; kt < nst; kt += 2) {
        if (kt + 1 < nst) load((kt + 1) * KS, av[1], bv[1]);
        mma(av[0], bv[0]);
        if (kt + 1 < nst) {
            if (kt + 2 < nst) load((kt + 2) * KS, av[0], bv[0]);
            mma(av[1], bv[1]);
        }
    }

    // epilogue, standard C/D maps: 32x32 col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5); 16x16 col = lane & 15, row = 4 (lane >> 4) + e
    float *O = p.O + b * p.sO + c;
    const float alpha = p.alpha, beta = p.beta;
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const int n = n0 + j * TS + (lane % TS);
            if (n >= N) continue;
#pragma unroll
            for (int e = 0; e < R; e++) {
                const int m = m0 + i * TS + (TS == 32 ? (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5) : 4 * (lane >> 4) + e);
                if (m >= M) continue;
                float v = acc[i][j][0][e];
                if (NACC == 2) v += acc[i][j][NACC - 1][e];
                const long z = ((long)m * N + n) * C;
                float o = v * alpha;
                if (beta != 0.f) o += O[z] * beta;
                O[z] = o;
            }
        }
}

template <int TS, int MT, int NT>
int launch_wave(BmmP p, hipStream_t hs) {
    p.tiles_m = (p.M + MT * TS - 1) / (MT * TS); p.tiles_n = (p.N + NT * TS - 1) / (NT * TS);
    p.items *= (long)p.tiles_m * p.tiles_n;
    const long blocks = (p.items + 3) / 4;
    if (blocks >= (1L << 24)) return fail(T4K_ERR_ARG, "t4k_gemm_batched: %ld wave tiles exceed one launch", p.items);   // 2^32 work-items
    auto kern = k_bmm_wave<TS, MT, NT>;
    T4K_LAUNCH(kern, dim3((unsigned)blocks), dim3(256), 0, hs, p);
    T4K_LAUNCH_CHECK();
    return T4K_OK;
}

} // namespace

extern "C" {

int t4k_gemm_batched(const float *A, const float *B, float *O, float alpha, float beta, int tA, int tB,
                     int M, int N, int K, int C, int cA, int cB, int batch, long sA, long sB, long sO, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!A || !B || !O || M < 0 || N < 0 || K < 0 || C < 1 || C > 65535 || batch < 0 || sA < 0 || sB < 0 ||
        (cA != 1 && cA != C) || (cB != 1 && cB != C))
        return fail(T4K_ERR_ARG, "t4k_gemm_batched: bad argument");
    if (batch > 1 && sO < (long)M * N * C) return fail(T4K_ERR_ARG, "t4k_gemm_batched: output entries overlap (sO < M*N*C)");
    if (M == 0 || N == 0 || batch == 0) return T4K_OK;
    hipStream_t hs = S(s);
    const bool chan_bcast = C > 1 && (cA != C || cB != C);
    if (!chan_bcast && (M > 64 || N > 64))
        return gemm_batched_tiles(A, B, O, alpha, beta, tA, tB, M, N, K, C, batch, sA, sB, sO, hs);
    BmmP p;
    p.A = A; p.B = B; p.O = O; p.alpha = alpha; p.beta = beta;
    p.tA = tA != 0; p.tB = tB != 0; p.M = M; p.N = N; p.K = K; p.C = C; p.cA = C == 1 ? 1 : cA; p.cB = C == 1 ? 1 : cB;
    p.sA = sA; p.sB = sB; p.sO = sO; p.items = (long)batch * C;
    if (M <= 16 && N <= 16) return launch_wave<16, 1, 1>(p, hs);
    if (M <= 32 && N <= 32) return launch_wave<32, 1, 1>(p, hs);
    if (M <= 32)            return launch_wave<32, 1, 2>(p, hs);
    if (N <= 32)            return launch_wave<32, 2, 1>(p, hs);
    return launch_wave<32, 2, 2>(p, hs);              // up to 64 x 64 whole; larger channel-broadcast products in 64x64 wave tiles
}

} // extern "C"
