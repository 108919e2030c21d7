// gemm_tile.h - the register-staged MFMA tile body (see the design notes at the top of gemm.hip) and the kernels made of it alone:
// k_gemm_mfma and its batched wrapper (launched by gemm.hip), k_gemm_dual (linear.hip).
#pragma once
#include "gemm_types.h"

namespace {

// FULL: every K slice is whole stages (K-slice%BK == 0, VEC): no predicates, no branches in the K loop, so the compiler can sink the
// next stage's loads and address math under the MFMAs.  Ragged M / N edges are handled by clamped source rows and predicated stores.
// gate (dual launches, see k_gemm_dual): mode 1 = this GEMM READS a buffer the other one overwrites: signal once the K loop
// has consumed every load; mode 2 = this GEMM is the writer: hold the epilogue stores until gate_n readers have signalled.
template <int BM, int BN, int BK, bool AKC, bool BKC, bool VEC, bool SKEW, bool FULL>
__device__ __forceinline__ void gemm_mfma_body(const GemmP &p, const int bx, const int by, const int bz,
                                               int *gate = nullptr, const int gate_mode = 0, const int gate_n = 0, const int gate_m = 0,
                                               const MaskChain *mc = nullptr) {
    constexpr int MT = BM / 64, NT = BN / 64;      // 32x32 fragments per wave (wave grid is 2x2)
    constexpr int PA = BM * BK / 1024, PB = BN * BK / 1024;   // 16-byte loads per thread per stage
    constexpr int NC = BK / 8;                     // 8-deep k chunks per stage
    constexpr int CH = BK / 4;                     // 16-byte chunks per LDS row of a K-contiguous operand
    constexpr int SW = (64 / BK) > 0 ? (64 / BK) : 1;   // rows per 256-byte LDS bank row
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *sA = lds, *sB = lds + 2 * BM * BK;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, h = lane >> 5, l31 = lane & 31;
    const int c = bz, C = p.C;
    const int M = p.M, N = p.N, K = p.K;

    // ---- XCD-aware, L2-friendly tile order ----
    const int T = p.tiles_m * p.tiles_n;
    if (bx >= T) {                                 // rider workgroups: cs_out[e] += sum_r cs_X[r, e] (k_dlinear_db nmath.cu:274-280)
        const int ex = tid & 63, ry = tid >> 6, e = (bx - T) * 64 + ex;
        float a = 0.f;
        if (e < p.cs_E) {
#pragma unroll 8
            for (int r = ry; r < p.cs_rows; r += 4) a += p.cs_X[(long)r * p.cs_E + e];
        }
        lds[ry * 64 + ex] = a;
        __syncthreads();
        if (ry == 0 && e < p.cs_E) p.cs_out[e] += (lds[ex] + lds[64 + ex]) + (lds[128 + ex] + lds[192 + ex]);
        return;
    }
    int L;
    {
        const int b = bx, q8 = T >> 3, r8 = T & 7, x = b & 7, i = b >> 3;
        L = (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + i;
    }
    constexpr int GROUP_M = 4;
    const int per_group = GROUP_M * p.tiles_n;
    const int grp = L / per_group, first_m = grp * GROUP_M;
    const int gsz = min(p.tiles_m - first_m, GROUP_M);
    const int tm = first_m + (L % per_group) % gsz, tn = (L % per_group) / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const int kbeg = by * p.kchunk;
    const int kend = min(K, kbeg + p.kchunk);
    const int nst  = (kend - kbeg + BK - 1) / BK;

    const float *__restrict__ A = p.A;
    const float *__restrict__ B = p.B;

    v4f ra[PA], rb[PB];                 // staging register set 0
    v4f ra2[PA], rb2[PB];               // set 1 (FULL path: loads run two stages ahead)

    auto ldg = [&](const float *X, bool ok, long idx) -> v4f {          // VEC: one 16-byte load
        v4f z = {0.f, 0.f, 0.f, 0.f};
        return ok ? *reinterpret_cast<const v4f *>(X + idx) : z;
    };
    // !VEC: 4 predicated scalar loads; v0 is the fixed coordinate, v1.. the contiguous one
    auto lds4 = [&](const float *X, long idx, int lim0, int lim1, int v0, int v1) -> v4f {
        v4f v;
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = (v0 < lim0 && v1 + e < lim1) ? X[(idx + e) * C + c] : 0.f;
        return v;
    };
    // FULL: per-thread source pointers of stage 0; stage kt is at + kt * step
    const v4f *ga[PA], *gb[PB];
    if (FULL) {
#pragma unroll
        for (int pp = 0; pp < PA; pp++) {
            const int id = pp * 256 + tid;
            // rows / 4-column groups beyond the matrix edge are CLAMPED to the last valid one: the loads stay unpredicated (valid memory,
            // finite or not - those values only reach accumulator rows / columns the epilogue never stores)
            if (AKC) ga[pp] = reinterpret_cast<const v4f *>(A + (long)min(m0 + id / CH, M - 1) * K + kbeg + (id % CH) * 4);
            else     ga[pp] = reinterpret_cast<const v4f *>(A + (long)(kbeg + id / (BM / 4)) * M + min(m0 + (id % (BM / 4)) * 4, M - 4));
        }
#pragma unroll
        for (int pp = 0; pp < PB; pp++) {
            const int id = pp * 256 + tid;
            if (BKC) gb[pp] = reinterpret_cast<const v4f *>(B + (long)min(n0 + id / CH, N - 1) * K + kbeg + (id % CH) * 4);
            else     gb[pp] = reinterpret_cast<const v4f *>(B + (long)(kbeg + id / (BN / 4)) * N + min(n0 + (id % (BN / 4)) * 4, N - 4));
        }
    }
    const long ga_step = AKC ? BK / 4 : (long)BK * M / 4, gb_step = BKC ? BK / 4 : (long)BK * N / 4;   // in float4
    auto load_into = [&](int kt, v4f (&ra)[PA], v4f (&rb)[PB]) __attribute__((always_inline)) {
        if (FULL) {
#pragma unroll
            for (int pp = 0; pp < PA; pp++) ra[pp] = ga[pp][(long)kt * ga_step];
#pragma unroll
            for (int pp = 0; pp < PB; pp++) rb[pp] = gb[pp][(long)kt * gb_step];
            return;
        }
        const int k0 = kbeg + kt * BK;
#pragma unroll
        for (int pp = 0; pp < PA; pp++) {
            const int id = pp * 256 + tid;
            if (AKC) {                                      // A stored [M][K]
                const int r = id / CH, q = id % CH, m = m0 + r, k = k0 + q * 4;
                ra[pp] = VEC ? ldg(A, m < M && k < kend, (long)m * K + k) : lds4(A, (long)m * K + k, M, kend, m, k);
            } else {                                        // A stored [K][M]
                const int kk = id / (BM / 4), rq = id % (BM / 4), k = k0 + kk, m = m0 + rq * 4;
                ra[pp] = VEC ? ldg(A, k < kend && m < M, (long)k * M + m) : lds4(A, (long)k * M + m, kend, M, k, m);
            }
        }
#pragma unroll
        for (int pp = 0; pp < PB; pp++) {
            const int id = pp * 256 + tid;
            if (BKC) {                                      // B stored [N][K]
                const int r = id / CH, q = id % CH, n = n0 + r, k = k0 + q * 4;
                rb[pp] = VEC ? ldg(B, n < N && k < kend, (long)n * K + k) : lds4(B, (long)n * K + k, N, kend, n, k);
            } else {                                        // B stored [K][N]
                const int kk = id / (BN / 4), rq = id % (BN / 4), k = k0 + kk, n = n0 + rq * 4;
                rb[pp] = VEC ? ldg(B, k < kend && n < N, (long)k * N + n) : lds4(B, (long)k * N + n, kend, N, k, n);
            }
        }
    };
    // LDS store offsets (floats) are loop invariant
    int soa[PA], sob[PB];
#pragma unroll
    for (int pp = 0; pp < PA; pp++) {
        const int id = pp * 256 + tid;
        if (AKC) { const int r = id / CH, q = id % CH; soa[pp] = r * BK + ((q ^ ((r / SW) & (CH - 1))) << 2); }
        else     { soa[pp] = (id / (BM / 4)) * BM + (id % (BM / 4)) * 4; }
    }
#pragma unroll
    for (int pp = 0; pp < PB; pp++) {
        const int id = pp * 256 + tid;
        if (BKC) { const int r = id / CH, q = id % CH; sob[pp] = r * BK + ((q ^ ((r / SW) & (CH - 1))) << 2); }
        else     { sob[pp] = (id / (BN / 4)) * BN + (id % (BN / 4)) * 4; }
    }
    auto store_from = [&](int buf, v4f (&ra)[PA], v4f (&rb)[PB]) __attribute__((always_inline)) {
        float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
        for (int pp = 0; pp < PA; pp++) *reinterpret_cast<v4f *>(a + soa[pp]) = ra[pp];
#pragma unroll
        for (int pp = 0; pp < PB; pp++) *reinterpret_cast<v4f *>(b + sob[pp]) = rb[pp];
    };
    auto load_tiles  = [&](int kt)  __attribute__((always_inline)) { load_into(kt, ra, rb); };
    auto store_tiles = [&](int buf) __attribute__((always_inline)) { store_from(buf, ra, rb); };
    // operand fragments of one 8-deep k chunk: lane half h holds k = 8*ci + 4*h + {0..3}
    auto read_chunk = [&](const float *a, const float *b, int ci, float (&av)[MT][4], float (&bv)[NT][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            const int r = wm * (BM / 2) + mt * 32 + l31;
            if (AKC) {
                const v4f t = *reinterpret_cast<const v4f *>(a + r * BK + (((ci * 2 + h) ^ ((r / SW) & (CH - 1))) << 2));
                av[mt][0] = t[0]; av[mt][1] = t[1]; av[mt][2] = t[2]; av[mt][3] = t[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) av[mt][j] = a[(ci * 8 + 4 * h + j) * BM + r];
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const int r = wn * (BN / 2) + nt * 32 + l31;
            if (BKC) {
                const v4f t = *reinterpret_cast<const v4f *>(b + r * BK + (((ci * 2 + h) ^ ((r / SW) & (CH - 1))) << 2));
                bv[nt][0] = t[0]; bv[nt][1] = t[1]; bv[nt][2] = t[2]; bv[nt][3] = t[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) bv[nt][j] = b[(ci * 8 + 4 * h + j) * BN + r];
            }
        }
    };

    // A wave with a single 32x32 fragment keeps NACC = 2 accumulator chains (even / odd k-pairs):
    // back-to-back MFMAs on ONE accumulator lose the forwarding path as soon as a ds_read or
    // s_waitcnt sits between them (+43 cycles per pair, MI355X_MICROARCH.md), two chains do not.
    constexpr int NACC = (MT * NT == 1) ? 2 : 1;
    f32x16 acc[MT][NT][NACC];
#pragma unroll
    for (int i = 0; i < MT; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int q = 0; q < NACC; q++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[i][j][q][r] = 0.f;

    auto mma_chunk = [&](float (&av)[MT][4], float (&bv)[NT][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int nt = 0; nt < NT; nt++)
                    acc[mt][nt][j % NACC] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt][j], bv[nt][j], acc[mt][nt][j % NACC], 0, 0, 0);
    };

    // beta != 0 (dW += ...): the old output values are fetched up front instead of as dependent loads after the K loop
    constexpr bool PRE = (MT * NT == 1);
    float oprev[16];
    if (PRE && p.beta != 0.f && p.nsplit == 1) {
        const int gn = n0 + wn * (BN / 2) + l31;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int gm = m0 + wm * (BM / 2) + (r & 3) + 8 * (r >> 2) + 4 * h;
            oprev[r] = (gm < M && gn < N) ? p.O[((long)gm * N + gn) * C + c] : 0.f;
        }
    }

    if (nst > 0) { load_tiles(0); store_tiles(0); }
    __syncthreads();

    if (FULL && !SKEW) {
        // loads run TWO stages ahead: stage t+1 sits in one register set while stage t+2 lands in the other
        if (nst > 1) load_into(1, ra, rb);
        if (nst > 2) load_into(2, ra2, rb2);
        auto stage = [&](int kt, v4f (&rx)[PA], v4f (&ry)[PB]) __attribute__((always_inline)) {
            const int buf = kt & 1;
            const float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
            for (int ci = 0; ci < NC; ci++) {
                float av[MT][4], bv[NT][4];
                read_chunk(a, b, ci, av, bv);
                mma_chunk(av, bv);
            }
            if (kt + 1 < nst) store_from(buf ^ 1, rx, ry);      // stage kt+1 (loaded a full stage ago)
            __syncthreads();
            if (kt + 3 < nst) load_into(kt + 3, rx, ry);        // refill the freed set
        };
        for (int kt = 0; kt < nst; kt += 2) {
            stage(kt, ra, rb);
            if (kt + 1 < nst) stage(kt + 1, ra2, rb2);
        }
    } else if (!SKEW) {
        for (int kt = 0; kt < nst; kt++) {
            const int buf = kt & 1;
            if (kt + 1 < nst) load_tiles(kt + 1);           // in flight during the MFMAs below
            const float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
            for (int ci = 0; ci < NC; ci++) {
                float av[MT][4], bv[NT][4];
                read_chunk(a, b, ci, av, bv);
                mma_chunk(av, bv);
            }
            if (kt + 1 < nst) store_tiles(buf ^ 1);
            __syncthreads();
        }
    } else if (nst > 0) {
        float cav[MT][4], cbv[NT][4];                       // chunk whose MFMAs are pending
        if (nst > 1) load_tiles(1);
        read_chunk(sA, sB, 0, cav, cbv);
        for (int kt = 0; kt < nst; kt++) {
            const int buf = kt & 1;
            const float *a = sA + buf * BM * BK, *b = sB + buf * BN * BK;
#pragma unroll
            for (int ci = 0; ci + 1 < NC; ci++) {
                float nav[MT][4], nbv[NT][4];
                read_chunk(a, b, ci + 1, nav, nbv);
                mma_chunk(cav, cbv);
#pragma unroll
                for (int j = 0; j < 4; j++) {
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) cav[mt][j] = nav[mt][j];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) cbv[nt][j] = nbv[nt][j];
                }
            }
            if (kt + 1 < nst) store_tiles(buf ^ 1);         // stage kt+1: registers -> the other buffer
            __syncthreads();
            if (kt + 2 < nst) load_tiles(kt + 2);
            float nav[MT][4], nbv[NT][4];
            if (kt + 1 < nst) read_chunk(sA + (buf ^ 1) * BM * BK, sB + (buf ^ 1) * BN * BK, 0, nav, nbv);
            mma_chunk(cav, cbv);                            // last chunk of stage kt covers the reads above
            if (kt + 1 < nst) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) cav[mt][j] = nav[mt][j];
#pragma unroll
                    for (int nt = 0; nt < NT; nt++) cbv[nt][j] = nbv[nt][j];
                }
            }
        }
    }

    // ---- epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const float alpha = p.alpha, beta = p.beta;
    if (gate_mode == 1) {                                   // every load of the shared buffer has been consumed
        __syncthreads();
        if (tid == 0) __hip_atomic_fetch_add(gate, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (gate_mode == 2) {
        if (tid == 0) T4K_SPIN_WAIT(__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gate_n, 1);
        __syncthreads();
    }
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < NT; nt++) {
            const int gn = n0 + wn * (BN / 2) + nt * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int gm = m0 + wm * (BM / 2) + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (gm < M && gn < N) {
                    float v = acc[mt][nt][0][r];
                    if (NACC == 2) v += acc[mt][nt][NACC - 1][r];
                    if (p.nsplit > 1) {
                        p.part[((long)by * M + gm) * N + gn] = v;
                    } else {
                        const long z = ((long)gm * N + gn) * C + c;
                        float o = v * alpha;
                        if (beta != 0.f) o += (PRE ? oprev[r] : p.O[z]) * beta;
                        if (p.bias) o += p.bias[gn];
                        p.O[z] = o;
                        if (mc && mc->d1) { const float g1 = o * mc->m1[z]; mc->d1[z] = g1; if (mc->d2) mc->d2[z] = g1 * mc->m2[z]; }
                    }
                }
            }
        }
    if (gate_mode == 2) {                                   // last writer re-arms the gate for the next launch
        __syncthreads();
        if (tid == 0) {
            const int t = __hip_atomic_fetch_add(gate + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t == gate_m - 1) {
                __hip_atomic_store(gate, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(gate + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}
template <int BM, int BN, int BK, bool AKC, bool BKC, bool VEC, bool SKEW, bool FULL>
__global__ void __launch_bounds__(256) k_gemm_mfma(GemmP p) {
    gemm_mfma_body<BM, BN, BK, AKC, BKC, VEC, SKEW, FULL>(p, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Two independent 64x64-tiled GEMMs in ONE launch (a linear layer's dW += dY^T X and dX = dY W): workgroups [0, nb1) run the
// first, the rest the second.  When the second overwrites an operand of the first (dX lands in X's buffer, backprop.cu:240)
// its stores wait on an arrival counter; every workgroup is resident (grid <= CU count), so the wait cannot deadlock.
// F1 / F2: that GEMM's K is whole 64-deep stages -> the predicate-free pipeline with loads two stages ahead (unskewed)
template <bool A1, bool B1, bool A2, bool B2, bool F1 = false, bool F2 = false>
__global__ void __launch_bounds__(256) k_gemm_dual(GemmP p1, GemmP p2, int nb1, int t1, int t2, int *gate, MaskChain mc) {
    // gate == nullptr: dX does not land in a buffer the dW half reads (no aliasing) - nothing to wait for
    if ((int)blockIdx.x < nb1) gemm_mfma_body<64, 64, 64, A1, B1, true, !F1, F1>(p1, blockIdx.x, 0, 0, gate, gate ? 1 : 0);
    else                       gemm_mfma_body<64, 64, 64, A2, B2, true, !F2, F2>(p2, (int)blockIdx.x - nb1, 0, 0, gate, gate ? 2 : 0, t1, t2, &mc);
}

} // namespace
