// linalg_batched.hip - the linear-algebra entries of linalg.hip over a BATCH of K x K matrices (entries K*K floats apart), one launch per
// call whatever the batch is.  No reference definition for the batch: the reference's Tensor::inverse / plu / lu_inverse / lu / det
// (src/mu/tensor.cu:344-456, kernels src/t4math.cu:742-979) take one rank-2 matrix.  Pivot rule, singularity test and the per-element
// expressions are those of linalg.hip (largest |a|, lowest row wins a tie, < DU_EPS is singular; lik = a[j,z] / pivot, a[j,k] -= lik * a[z,k];
// Gauss-Jordan: row z /= pivot, a[j,k] -= a[j,z] * a[z,k]), so pivots agree with the per-matrix kernels; only the
// WAY the trailing block is swept differs, and no element's operation order depends on that.
//
// Three regimes, chosen by K alone:
//   wave      K <= 32: one wave64 per matrix, four matrices per workgroup.  The matrix (and the inverse being built) lives in a wave-PRIVATE
//             LDS region at the odd row pitch K | 1, so a row walk and a column walk both touch 32 different banks per 32-lane group.  No
//             workgroup barrier anywhere: wave-private data needs LDS ordering only (a wave's LDS operations complete in order).
//   workgroup A and X fit in LDS (K <= 140; K <= 200 for plu / det, which hold A alone): one 256-thread workgroup per matrix, each wave
//             sweeping whole rows of the trailing block 64 columns at a time, two barriers per column.
//   global    up to K = 1024: the same column loop on global memory (pitch K), one workgroup per matrix.
// A column costs two group synchronisations: [B1] after the pivot partials are published, [B2] after the row swap and the column scaling.
// The pivot search of column z + 1 rides in the sweep of column z: the thread that owns row j updates a[j, z+1] first and keeps its
// candidate, the 2-D sweep then covers the columns from z + 2 on.
#include "t4k_common.h"

using namespace t4k;

namespace {

enum { M_WAVE = 0, M_BLOCK = 1, M_GLOBAL = 2 };
enum { OP_INV = 0, OP_PLU = 1, OP_LUINV = 2, OP_DET = 3 };

constexpr int LAB_K_WAVE  = 32;       // one wave per matrix up to here
constexpr int LAB_K_BLK2  = 140;      // A and X in LDS: (2 K (K|1) + 2 K + 12) * 4 B = 159 088 B at K = 140
constexpr int LAB_K_BLK1  = 200;      // A alone in LDS: (K (K|1) + 2 K + 12) * 4 B = 162 448 B at K = 200
constexpr int LAB_K_MAX   = 1024;     // the per-matrix kernels' working set
constexpr int LAB_LDS_MAX = 160 * 1024;
constexpr int PNONE = 0x7fffffff;

// LDS words of one group (a wave in the wave regime, else the workgroup): A, X, colz[K] (float), perm[K] (int), 12 reduction slots
__host__ __device__ inline int lab_words(int mode, int op, int K) {
    const int P = K | 1, two = (op == OP_INV || op == OP_LUINV) ? 2 : 1;
    const int mat = mode == M_GLOBAL ? 0 : two * K * P;
    return (mat + 2 * K + 12 + 3) & ~3;
}

template <int MODE> struct Grp {
    int tid, nt;                      // thread inside the group, threads of the group
    float *red;                       // 12 LDS words: [0,4) |pivot|, [4,8) pivot, [8,12) row  (workgroup regimes; the sums of det reuse [0,4) and [8,12))
    __device__ __forceinline__ void sync() const {
        if (MODE == M_WAVE) {         // wave-private LDS: keep the compiler from moving LDS accesses across; the hardware keeps a wave's own in order
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        } else __syncthreads();
    }
};

// pivot candidate: (|v|, v, row); none = (-1, 0, PNONE).  Larger |v| wins, the lower row on a tie (block_find_pivot of linalg.hip).
struct Cand { float a, v; int i; };
__device__ __forceinline__ void cand_scan(Cand &c, float v, int j) { const float av = fabsf(v); if (av > c.a) { c.a = av; c.v = v; c.i = j; } }   // rows come in rising order
__device__ __forceinline__ void cand_take(Cand &c, float a2, float v2, int i2) { if (a2 > c.a || (a2 == c.a && i2 < c.i)) { c.a = a2; c.v = v2; c.i = i2; } }
// before [B1]: every lane of a wave ends with the wave's best; the workgroup regimes publish it
template <int MODE> __device__ __forceinline__ void cand_publish(const Grp<MODE> &g, Cand &c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float a2 = __shfl_xor(c.a, off, 64), v2 = __shfl_xor(c.v, off, 64); const int i2 = __shfl_xor(c.i, off, 64);
        cand_take(c, a2, v2, i2);
    }
    if (MODE != M_WAVE && (g.tid & 63) == 0) { const int w = g.tid >> 6; g.red[w] = c.a; g.red[4 + w] = c.v; ((int *)g.red)[8 + w] = c.i; }
}
// after [B1]
template <int MODE> __device__ __forceinline__ void cand_collect(const Grp<MODE> &g, Cand &c) {
    if (MODE == M_WAVE) return;
    c.a = g.red[0]; c.v = g.red[4]; c.i = ((int *)g.red)[8];
#pragma unroll
    for (int w = 1; w < 4; w++) cand_take(c, g.red[w], g.red[4 + w], ((int *)g.red)[8 + w]);
}
template <int MODE> __device__ __forceinline__ float grp_sum(const Grp<MODE> &g, float v, int slot) {   // workgroup regimes: one barrier, slot = 0 or 8
    v = wave_sum_all(v);
    if (MODE == M_WAVE) return v;
    if ((g.tid & 63) == 0) g.red[slot + (g.tid >> 6)] = v;
    __syncthreads();
    return ((g.red[slot] + g.red[slot + 1]) + g.red[slot + 2]) + g.red[slot + 3];
}

// PLU of a[K,K] (pitch P) in place: packed L\U, piv_out[z] = pivot row of column z (-1 where it is singular), perm = the row order the swaps
// leave (row i of P A is row perm[i] of A).  Returns 0 or z + 1; nswap = number of columns that swapped.  The caller synchronises before it reads a.
template <int MODE>
__device__ __forceinline__ int plu_engine(const Grp<MODE> &g, float *a, int P, int K, int *perm, int *piv_out, int cwsh, int &nswap) {
    const int CW = 1 << cwsh, tx = g.tid & (CW - 1), ty = g.tid >> cwsh, RW = g.nt >> cwsh;
    Cand c = { -1.0f, 0.0f, PNONE };
    for (int j = g.tid; j < K; j += g.nt) cand_scan(c, a[j * P], j);
    nswap = 0;
    for (int z = 0; z < K; z++) {
        cand_publish(g, c);
        g.sync();                                                                    // [B1]
        cand_collect(g, c);
        const bool singular = c.a < DU_EPS;
        const int u = c.i; const float pv = c.v;
        if (g.tid == 0) piv_out[z] = singular ? -1 : u;
        if (singular) return z + 1;
        nswap += (u != z);
        // column z below the pivot becomes l = a / pivot, rows z and u change places.  Column z of those two rows belongs to ONE thread
        // (the one of row u), every other element to exactly one thread: no element is read by one thread and written by another.
        for (int t = g.tid; t < 2 * K; t += g.nt) {
            if (t < K) {
                const int j = t;
                if (j > z) {
                    if (j == u) { const float old = a[z * P + z]; a[z * P + z] = pv; a[u * P + z] = old / pv; }
                    else a[j * P + z] = a[j * P + z] / pv;
                }
            } else if (u != z) {
                const int k = t - K;
                if (k != z) { const float q = a[z * P + k]; a[z * P + k] = a[u * P + k]; a[u * P + k] = q; }
            }
        }
        if (g.tid == 0 && u != z) { const int q = perm[z]; perm[z] = perm[u]; perm[u] = q; }
        g.sync();                                                                    // [B2]
        c.a = -1.0f; c.v = 0.0f; c.i = PNONE;
        if (z + 1 < K) {
            const int n = z + 1; const float top = a[z * P + n];
            for (int j = n + g.tid; j < K; j += g.nt) {                              // column z + 1 by the rows' owners, who keep their candidate
                const float v = a[j * P + n] - a[j * P + z] * top;
                a[j * P + n] = v; cand_scan(c, v, j);
            }
            for (int j = n + ty; j < K; j += RW) {                                   // the rest of the trailing block, CW columns of RW rows at a time
                const float l = a[j * P + z];
                for (int k = n + 1 + tx; k < K; k += CW) a[j * P + k] -= l * a[z * P + k];
            }
        }
    }
    return 0;
}

// Gauss-Jordan on a | x (x holds the identity on entry): x leaves as the inverse, a as scratch (column z is dead once it has been eliminated:
// its multipliers are kept in colz, nobody reads it again, so it is not written either).  Returns 0 or z + 1.
// One departure from k_inverse: a row whose multiplier is below DU_EPS is eliminated like any other.  k_inverse (as k_elim) skips it, which
// leaves up to 1e-6 |a[z,k]| in that row - an ABSOLUTE error the residual bar |A X - I| <= c K u |A| |X| does not allow where |A| |X| is small
// (measured: one entry of 128 at K = 33 at 1.12 x the bar, in k_inverse and here alike while the skip was kept).  Everywhere else the two agree bit for bit.
template <int MODE>
__device__ __forceinline__ int gj_engine(const Grp<MODE> &g, float *a, float *x, int P, int K, float *colz, int cwsh) {
    const int CW = 1 << cwsh, tx = g.tid & (CW - 1), ty = g.tid >> cwsh, RW = g.nt >> cwsh;
    Cand c = { -1.0f, 0.0f, PNONE };
    for (int j = g.tid; j < K; j += g.nt) cand_scan(c, a[j * P], j);
    for (int z = 0; z < K; z++) {
        cand_publish(g, c);
        g.sync();                                                                    // [B1]
        cand_collect(g, c);
        if (c.a < DU_EPS) return z + 1;
        const int u = c.i; const float pv = c.v;
        // new row z = old row u / pivot, new row u = old row z (a: the columns right of z; x: all); colz[j] = a[j,z] as the swap leaves it
        for (int t = g.tid; t < 3 * K; t += g.nt) {
            if (t < K) { const int j = t; if (j != z) colz[j] = a[(j == u ? z : j) * P + z]; }
            else if (t < 2 * K) {
                const int k = t - K;
                if (k > z) { const float au = a[u * P + k]; if (u != z) a[u * P + k] = a[z * P + k]; a[z * P + k] = au / pv; }
            } else {
                const int k = t - 2 * K;
                const float xu = x[u * P + k]; if (u != z) x[u * P + k] = x[z * P + k]; x[z * P + k] = xu / pv;
            }
        }
        g.sync();                                                                    // [B2]
        c.a = -1.0f; c.v = 0.0f; c.i = PNONE;
        const int n = z + 1;
        if (n < K) {
            const float top = a[z * P + n];
            for (int j = g.tid; j < K; j += g.nt) {
                if (j == z) continue;
                const float v = a[j * P + n] - colz[j] * top;
                a[j * P + n] = v;
                if (j > z) cand_scan(c, v, j);
            }
        }
        for (int j = ty; j < K; j += RW) {
            if (j == z) continue;
            const float r1 = colz[j];
            for (int k = n + 1 + tx; k < K; k += CW) a[j * P + k] -= r1 * a[z * P + k];
            for (int k = tx; k < K; k += CW) x[j * P + k] -= r1 * x[z * P + k];
        }
    }
    return 0;
}

// forward and backward substitution on the columns of x (= P on entry), one thread per column as k_lu_inverse
template <int MODE>
__device__ __forceinline__ void lu_subst(const Grp<MODE> &g, const float *a, float *x, int P, int K) {
    for (int i = g.tid; i < K; i += g.nt) {
        for (int k = 1; k < K; k++) {
            float s = x[k * P + i];
            for (int j = 0; j < k; j++) s -= a[k * P + j] * x[j * P + i];
            x[k * P + i] = s;
        }
        for (int j = K - 1; j >= 0; j--) {
            float s = x[j * P + i];
            for (int k = j + 1; k < K; k++) s -= a[j * P + k] * x[k * P + i];
            x[j * P + i] = s / a[j * P + j];
        }
    }
}

// HBM <-> LDS: consecutive threads take consecutive 16-byte (vec) or 4-byte pieces of the row-major entry
template <int MODE> __device__ __forceinline__ void lab_load(const Grp<MODE> &g, const float *src, float *dst, int K, int P, bool vec) {
    const unsigned n = (unsigned)K * K;
    if (vec) {
        for (unsigned q = g.tid; q < (n >> 2); q += g.nt) {
            const float4 v = ((const float4 *)src)[q];
            unsigned r = (q * 4) / (unsigned)K, cc = q * 4 - r * K;
            const float e[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
            for (int t = 0; t < 4; t++) { dst[r * P + cc] = e[t]; if (++cc == (unsigned)K) { cc = 0; r++; } }
        }
    } else for (unsigned q = g.tid; q < n; q += g.nt) { const unsigned r = q / (unsigned)K; dst[r * P + (q - r * K)] = src[q]; }
}
template <int MODE> __device__ __forceinline__ void lab_store(const Grp<MODE> &g, const float *src, float *dst, int K, int P, bool vec) {
    const unsigned n = (unsigned)K * K;
    if (vec) {
        for (unsigned q = g.tid; q < (n >> 2); q += g.nt) {
            unsigned r = (q * 4) / (unsigned)K, cc = q * 4 - r * K;
            float e[4];
#pragma unroll
            for (int t = 0; t < 4; t++) { e[t] = src[r * P + cc]; if (++cc == (unsigned)K) { cc = 0; r++; } }
            ((float4 *)dst)[q] = make_float4(e[0], e[1], e[2], e[3]);
        }
    } else for (unsigned q = g.tid; q < n; q += g.nt) { const unsigned r = q / (unsigned)K; dst[q] = src[r * P + (q - r * K)]; }
}
// dst[i,k] = (k == perm[i]) at pitch P (LDS, or global with P = K)
template <int MODE> __device__ __forceinline__ void lab_perm_matrix(const Grp<MODE> &g, const int *perm, float *dst, int K, int P) {
    const unsigned n = (unsigned)K * K;
    for (unsigned q = g.tid; q < n; q += g.nt) { const unsigned r = q / (unsigned)K, cc = q - r * K; dst[r * P + cc] = ((int)cc == perm[r]) ? 1.0f : 0.0f; }
}

// One kernel body for the four factorising entries.  X: the inverse (OP_INV, OP_LUINV) or the permutation matrix (OP_PLU, may be null).
template <int MODE, int OP>
__global__ void __launch_bounds__(BLK) k_lab(float *A, float *X, int *piv, float *det, int *status, int K, int batch, int cwsh, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lab_sm[];
    Grp<MODE> g;
    int b; float *sm = lab_sm;
    if (MODE == M_WAVE) {
        g.tid = threadIdx.x & 63; g.nt = WAVE; b = blockIdx.x * 4 + (threadIdx.x >> 6);
        sm += (threadIdx.x >> 6) * lab_words(MODE, OP, K);
        if (b >= batch) return;                         // a whole wave leaves: nothing here waits for another wave
    } else { g.tid = threadIdx.x; g.nt = BLK; b = blockIdx.x; }
    constexpr bool TWO = OP == OP_INV || OP == OP_LUINV;
    const int P = MODE == M_GLOBAL ? K : (K | 1);
    const long ent = (long)b * K * K;
    float *ga = A + ent, *gx = X ? X + ent : nullptr;
    float *a = MODE == M_GLOBAL ? ga : sm;
    float *x = MODE == M_GLOBAL ? gx : (TWO ? sm + K * P : nullptr);
    float *colz = sm + (MODE == M_GLOBAL ? 0 : (TWO ? 2 : 1) * K * P);
    int *perm = (int *)(colz + K);
    g.red = colz + 2 * K;
    int *pv = piv ? piv + (long)b * K : nullptr;

    if (MODE != M_GLOBAL) lab_load(g, ga, a, K, P, vec != 0);
    int st, nswap = 0;
    if (OP == OP_INV) {
        const unsigned n = (unsigned)K * K;             // the kernel writes the identity: X is a pure output
        for (unsigned q = g.tid; q < n; q += g.nt) { const unsigned r = q / (unsigned)K, cc = q - r * K; x[r * P + cc] = r == cc ? 1.0f : 0.0f; }
        g.sync();
        st = gj_engine(g, a, x, P, K, colz, cwsh);
        g.sync();
        if (st == 0 && MODE != M_GLOBAL) lab_store(g, x, gx, K, P, vec != 0);
    } else {
        for (int i = g.tid; i < K; i += g.nt) perm[i] = i;
        g.sync();
        st = plu_engine(g, a, P, K, perm, pv, cwsh, nswap);
        g.sync();
        if (st == 0) {
            if (OP == OP_LUINV) {
                lab_perm_matrix(g, perm, x, K, P);
                g.sync();
                lu_subst(g, a, x, P, K);
                g.sync();
                if (MODE != M_GLOBAL) lab_store(g, x, gx, K, P, vec != 0);
            }
            if (OP == OP_PLU && gx) lab_perm_matrix(g, perm, gx, K, K);
            if (OP == OP_DET) {                         // Tensor::det: expf(sum ln|u_jj|) * parity of the swaps * product of the signs
                float acc = 0.0f; int neg = 0;
                for (int j = g.tid; j < K; j += g.nt) { float d = a[j * P + j]; if (d < 0.0f) { neg ^= 1; d = -d; } acc += logf(d); }
                const float ld = grp_sum(g, acc, 0), ng = grp_sum(g, (float)neg, 8);
                if (g.tid == 0) det[b] = expf(ld) * (((nswap + (int)ng) & 1) ? -1.0f : 1.0f);
            }
            if (MODE != M_GLOBAL) lab_store(g, a, ga, K, P, vec != 0);
        } else if (OP == OP_DET && g.tid == 0) det[b] = 0.0f;
    }
    if (g.tid == 0) status[b] = st;
}

// keep U, or unit L, of every packed L\U of the batch (k_lu_extract per entry)
__global__ void __launch_bounds__(BLK) k_lab_extract(float *LU, int get_u, int K, long total) {
    const unsigned kk = (unsigned)K * K;
    for (long z = (long)blockIdx.x * BLK + threadIdx.x; z < total; z += (long)gridDim.x * BLK) {
        const unsigned e = (unsigned)(z % kk), ty = e / (unsigned)K, tx = e - ty * K;
        if (get_u) { if (tx < ty) LU[z] = 0.f; }
        else { if (tx == ty) LU[z] = 1.f; else if (tx > ty) LU[z] = 0.f; }
    }
}

template <int MODE, int OP>
int lab_go(float *A, float *X, int *piv, float *det, int *status, int K, int batch, int cwsh, int vec, hipStream_t hs) {
    const int wpg = MODE == M_WAVE ? 4 : 1;
    const size_t lds = (size_t)lab_words(MODE, OP, K) * wpg * sizeof(float);
    if (lds > (size_t)LAB_LDS_MAX) return fail(T4K_ERR_UNSUPPORTED, "linalg_batched: K = %d needs %zu bytes of LDS", K, lds);
    if (lds > 65536) {
        static size_t granted = 0;                      // per instantiation
        if (lds > granted) { T4K_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lab<MODE, OP>), hipFuncAttributeMaxDynamicSharedMemorySize, LAB_LDS_MAX)); granted = LAB_LDS_MAX; }
    }
    T4K_LAUNCH((k_lab<MODE, OP>), dim3((batch + wpg - 1) / wpg), dim3(BLK), lds, hs, A, X, piv, det, status, K, batch, cwsh, vec);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}
template <int OP>
int lab_dispatch(const char *who, float *A, float *X, int *piv, float *det, int *status, int K, int batch, t4k_stream_t s) {
    if (K <= 0 || batch < 0) return fail(T4K_ERR_ARG, "%s: bad argument", who);
    if (K > LAB_K_MAX) return fail(T4K_ERR_UNSUPPORTED, "%s: K = %d above %d", who, K, LAB_K_MAX);
    if (batch == 0) return T4K_OK;
    const int vec = ((long)K * K % 4 == 0) && aligned16(A) && (!X || aligned16(X));
    const int kblk = (OP == OP_INV || OP == OP_LUINV) ? LAB_K_BLK2 : LAB_K_BLK1;
    if (K <= LAB_K_WAVE) return lab_go<M_WAVE, OP>(A, X, piv, det, status, K, batch, K <= 4 ? 2 : K <= 8 ? 3 : K <= 16 ? 4 : 5, vec, S(s));
    if (K <= kblk)       return lab_go<M_BLOCK, OP>(A, X, piv, det, status, K, batch, 6, vec, S(s));
    return lab_go<M_GLOBAL, OP>(A, X, piv, det, status, K, batch, 6, 0, S(s));
}

} // namespace

extern "C" {

int t4k_inverse_batched(float *A, float *X, int K, int batch, int *status_dev, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!A || !X || !status_dev) return fail(T4K_ERR_ARG, "t4k_inverse_batched: bad argument");
    return lab_dispatch<OP_INV>("t4k_inverse_batched", A, X, nullptr, nullptr, status_dev, K, batch, s);
}
int t4k_plu_batched(float *A, float *Pm, int *piv_dev, int K, int batch, int *status_dev, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!A || !piv_dev || !status_dev) return fail(T4K_ERR_ARG, "t4k_plu_batched: bad argument");
    return lab_dispatch<OP_PLU>("t4k_plu_batched", A, Pm, piv_dev, nullptr, status_dev, K, batch, s);
}
int t4k_lu_inverse_batched(float *A, float *X, int *piv_dev, int K, int batch, int *status_dev, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!A || !X || !piv_dev || !status_dev) return fail(T4K_ERR_ARG, "t4k_lu_inverse_batched: bad argument");
    return lab_dispatch<OP_LUINV>("t4k_lu_inverse_batched", A, X, piv_dev, nullptr, status_dev, K, batch, s);
}
int t4k_det_batched(float *A, int *piv_dev, int K, int batch, float *det_dev, int *status_dev, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!A || !piv_dev || !det_dev || !status_dev) return fail(T4K_ERR_ARG, "t4k_det_batched: bad argument");
    return lab_dispatch<OP_DET>("t4k_det_batched", A, nullptr, piv_dev, det_dev, status_dev, K, batch, s);
}
int t4k_lu_extract_batched(float *LU, int get_u, int K, int batch, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!LU || K <= 0 || batch < 0) return fail(T4K_ERR_ARG, "t4k_lu_extract_batched: bad argument");
    if (K > LAB_K_MAX) return fail(T4K_ERR_UNSUPPORTED, "t4k_lu_extract_batched: K = %d above %d", K, LAB_K_MAX);
    if (batch == 0) return T4K_OK;
    const long total = (long)batch * K * K;
    T4K_LAUNCH(k_lab_extract, dim3(grid_for(total)), dim3(BLK), 0, S(s), LU, get_u, K, total);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

} // extern "C"
