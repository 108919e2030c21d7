// linalg_batched.hip - the linear-algebra entries of linalg.hip over a BATCH of K x K matrices (entries K*K floats apart), one launch per
// call whatever the batch is.  No reference definition for the batch: the reference's Tensor::inverse / plu / lu_inverse / lu / det
// (src/mu/tensor.cu:344-456, kernels src/t4math.cu:742-979) take one rank-2 matrix.  Pivot rule, singularity test and the per-element
// expressions are those of linalg.hip (largest |a|, lowest row wins a tie, < DU_EPS is singular; lik = a[j,z] / pivot, a[j,k] -= lik * a[z,k];
// Gauss-Jordan: row z /= pivot, a[j,k] -= a[j,z] * a[z,k]), so pivots agree with the per-matrix kernels; only the
// WAY the trailing block is swept differs, and no element's operation order depends on that.
//
// Four regimes, chosen by K alone (lab_plan below; the fourth, blocked, from K = 193 (plu, det: 201) to 1024, has its own kernel):
//   wave      K <= 32: one wave64 per matrix, four matrices per workgroup.  The matrix (and the inverse being built) lives in a wave-PRIVATE
//             LDS region at the odd row pitch K | 1, so a row walk and a column walk both touch 32 different banks per 32-lane group.  No
//             workgroup barrier anywhere: wave-private data needs LDS ordering only (a wave's LDS operations complete in order).
//   workgroup A and X fit in LDS (K <= 140; K <= 200 for plu / det, which hold A alone): one 256-thread workgroup per matrix, each wave
//             sweeping whole rows of the trailing block 64 columns at a time, two barriers per column.
//   global    inverse, luinv up to K = 192: the same column loop on global memory (pitch K), one workgroup per matrix.
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

// ------------------------------------------------------------------ the blocked regime: right-looking PLU in panels of NB = 32
// columns, the trailing update on v_mfma_f32_32x32x2_f32.  One 256-thread workgroup per matrix.
//   panel     rows j.. of columns [j, j + 32) live in LDS at pitch 33 (rows padded with zeros to a multiple of 32) and are factored there column by
//             column with the pivot search, swap and scale expressions of plu_engine, a thread per ROW for the rank-1 update inside the panel.
//   swaps     the panel's row swaps reach the columns left and right of it in global memory: a thread owns a 16-byte (vec) or 4-byte column
//             piece and walks the 32 swaps in order, so a wave moves whole coalesced rows and no swap waits for another thread.
//   trailing  a wave owns 32-column tiles.  Lane (n, h) solves column n of U12 = L11^-1 A12 in registers (L11 broadcast from the LDS panel; both
//             halves h solve the same column), which leaves the MFMA B operand k = 2 kk + h in place: U12 never goes through LDS.  Then, 32 rows
//             at a time, C = A22 tile (global, read and written once per panel step), A operand = -L21 from the LDS panel, 16 MFMAs.
// Every global element of the trailing block is read and written by the SAME lane between two workgroup barriers: the C / D layout
// (column n = lane & 31, rows (v & 3) + 8 (v >> 2) + 4 h) decides the owner, and the column solve stores by it.
// inverse and luinv run the same PLU and then the substitution further down (labb_subst).
typedef float lab_f16 __attribute__((ext_vector_type(16)));
typedef float lab_f4 __attribute__((ext_vector_type(4)));
typedef float lab_f32 __attribute__((ext_vector_type(32)));
constexpr int LAB_NB = 32, LAB_LP = LAB_NB + 1;
constexpr int LAB_KB_X = 192;         // inverse, luinv: blocked above this (measured).  plu, det: blocked above LAB_K_BLK1, the global
                                      // regime no longer serves them (the sweep's first K, 224, already wins; k_lab<M_GLOBAL, plu | det> stay instantiated, unreached)
constexpr int LAB_SUBST_WORDS = 2 * LAB_NB * LAB_LP;   // a wave's two tiles in the substitution: they reuse the panel
__host__ __device__ inline int labb_rows(int K) { return (K + LAB_NB - 1) & ~(LAB_NB - 1); }
// LDS words: the panel [rows][33], the panel's 32 pivots, perm[K], 12 reduction slots
// (inverse, luinv: the panel region is at least the four waves' substitution tiles, which reuse it)
__host__ __device__ inline int labb_panel(int K, bool two) { const int w = labb_rows(K) * LAB_LP; return two && w < 4 * LAB_SUBST_WORDS ? 4 * LAB_SUBST_WORDS : w; }
__host__ __device__ inline int labb_words(int K, bool two) { return (labb_panel(K, two) + LAB_NB + K + 12 + 3) & ~3; }
__device__ __forceinline__ int labb_crow(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// x = L^-1 x, L[32][33] unit lower in LDS (every lane reads the same word), a column of L at a time: the products of a column are independent,
// and each x[i] still meets its terms in rising k, the order the column loop of plu_engine gives.  The fences keep the compiler from lifting
// the 496 reads out of the caller's loop or in front of the first product (either costs some 500 registers).
__device__ __forceinline__ void labb_fence() { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }
// the same pointer with its offset in a vector register the compiler cannot see through: the reads become one base and 16-bit immediates, not
// 496 uniform addresses computed ahead of the loop and kept
__device__ __forceinline__ const float *labb_opaque(const float *p) { int off = 0; asm volatile("" : "+v"(off)); return p + off; }
__device__ __forceinline__ void labb_lsolve(lab_f32 &x, const float *L) {
    L = labb_opaque(L);
    labb_fence();
#pragma unroll
    for (int k = 0; k < LAB_NB - 1; k++) {
#pragma unroll
        for (int i = k + 1; i < LAB_NB; i++) x[i] -= L[i * LAB_LP + k] * x[k];
        if (k & 1) labb_fence();
    }
}
// a solved column x (the same in lanes (n, 0) and (n, 1)) back to the rows its lane owns in the C / D layout, and as the B operand k = 2 kk + h
__device__ __forceinline__ lab_f16 labb_column_out(const lab_f32 &x, float *base, unsigned t, int K, int rows, bool cv, int h) {
    lab_f16 bv;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        const int i0 = (v & 3) + 8 * (v >> 2);
        if (cv && i0 + 4 * h < rows) base[t + (unsigned)((i0 + 4 * h) * K)] = h ? x[i0 + 4] : x[i0];
        bv[v] = h ? x[2 * v + 1] : x[2 * v];
    }
    return bv;
}
// the C tile of 32 rows at base[t] (base: the entry, the same in every lane; t: this lane's 32-bit offset, so every access is scalar base + vector
// offset; rows / cv: what lies inside the matrix).  Loads are clamped, not predicated: they go out together.
__device__ __forceinline__ lab_f16 labb_ctile(const float *base, unsigned t, int K, int rows, bool cv, int h) {
    lab_f16 acc;
#pragma unroll
    for (int v = 0; v < 16; v++) { const int r = labb_crow(v, h); const float q = base[t + (unsigned)((r < rows ? r : rows - 1) * K)]; acc[v] = (cv && r < rows) ? q : 0.0f; }
    return acc;
}
__device__ __forceinline__ void labb_ctile_out(float *base, unsigned t, const lab_f16 &acc, int K, int rows, bool cv, int h) {
    if (!cv) return;
#pragma unroll
    for (int v = 0; v < 16; v++) { const int r = labb_crow(v, h); if (r < rows) base[t + (unsigned)(r * K)] = acc[v]; }
}

// one panel step at column j.  Returns 0 or z + 1 of the singular column.
__device__ __forceinline__ int labb_step(const Grp<M_GLOBAL> &g, float *a, int K, int j, float *Lp, int *pivl, int *perm, int *pv, int vec, int &nswap) {
    const int m = K - j, nb = m < LAB_NB ? m : LAB_NB, mr = labb_rows(m);
    const int lane = g.tid & 63, wv = g.tid >> 6, n31 = lane & 31, h = lane >> 5;
    g.sync();                                                                        // the step before has left the panel and written A
    for (int q = g.tid; q < mr * LAB_NB; q += g.nt) { const int r = q >> 5, c = q & 31; Lp[r * LAB_LP + c] = (r < m && c < nb) ? a[(j + r) * K + j + c] : 0.0f; }
    g.sync();
    Cand c = { -1.0f, 0.0f, PNONE };
    for (int r = g.tid; r < m; r += g.nt) cand_scan(c, Lp[r * LAB_LP], r);
    for (int z = 0; z < nb; z++) {
        cand_publish(g, c);
        g.sync();                                                                    // [B1]
        cand_collect(g, c);
        const bool singular = c.a < DU_EPS;
        const int u = c.i; const float pvt = c.v;
        if (g.tid == 0 && pv) pv[j + z] = singular ? -1 : j + u;
        if (singular) return j + z + 1;
        nswap += (u != z);
        if (g.tid == 0) { pivl[z] = u; if (u != z) { const int q = perm[j + z]; perm[j + z] = perm[j + u]; perm[j + u] = q; } }
        for (int t = g.tid; t < m + LAB_NB; t += g.nt) {                             // as plu_engine: column z scaled, rows z and u change places
            if (t < m) {
                if (t > z) {
                    if (t == u) { const float old = Lp[z * LAB_LP + z]; Lp[z * LAB_LP + z] = pvt; Lp[u * LAB_LP + z] = old / pvt; }
                    else Lp[t * LAB_LP + z] = Lp[t * LAB_LP + z] / pvt;
                }
            } else if (u != z) {
                const int k = t - m;
                if (k != z) { const float q = Lp[z * LAB_LP + k]; Lp[z * LAB_LP + k] = Lp[u * LAB_LP + k]; Lp[u * LAB_LP + k] = q; }
            }
        }
        g.sync();                                                                    // [B2]
        c.a = -1.0f; c.v = 0.0f; c.i = PNONE;
        const int n = z + 1;
        for (int r = n + g.tid; r < m; r += g.nt) {                                  // a thread per row: 32 lanes, 32 banks at pitch 33
            const float l = Lp[r * LAB_LP + z];
            if (n < nb) { const float v = Lp[r * LAB_LP + n] - l * Lp[z * LAB_LP + n]; Lp[r * LAB_LP + n] = v; cand_scan(c, v, r); }
            for (int k = n + 1; k < nb; k++) Lp[r * LAB_LP + k] -= l * Lp[z * LAB_LP + k];
        }
    }
    g.sync();
    for (int q = g.tid; q < m * nb; q += g.nt) { const int r = q / nb, cc = q - r * nb; a[(j + r) * K + j + cc] = Lp[r * LAB_LP + cc]; }
    {                                                                                // the swaps, on the columns outside the panel
        const int W = vec ? 4 : 1, ng = (K - nb) / W;                                // vec: K % 4 == 0, so nb % 4 == 0 too
        for (int q = g.tid; q < ng; q += g.nt) {
            int col = q * W; if (col >= j) col += nb;
            for (int z = 0; z < nb; z++) {
                const int u = pivl[z];
                if (u == z) continue;
                float *rz = a + (j + z) * K + col, *ru = a + (j + u) * K + col;
                if (vec) { const lab_f4 t = *(lab_f4 *)rz; *(lab_f4 *)rz = *(lab_f4 *)ru; *(lab_f4 *)ru = t; }
                else { const float t = *rz; *rz = *ru; *ru = t; }
            }
        }
    }
    if (m <= LAB_NB) return 0;
    g.sync();                                                                        // swapped rows are read by other waves
    const int nct = (m - 1) / LAB_NB;                                                // 32-column tiles right of the panel
    for (int ct = wv; ct < nct; ct += 4) {
        const int col = j + LAB_NB * (ct + 1) + n31; const bool cv = col < K;
        const unsigned top = (unsigned)(j * K + (cv ? col : K - 1));                 // row j of this lane's column (clamped: read, never written)
        lab_f32 x;
#pragma unroll
        for (int i = 0; i < LAB_NB; i++) { const float q = a[top + (unsigned)(i * K)]; x[i] = cv ? q : 0.0f; }
        labb_lsolve(x, Lp);
        const lab_f16 bv = labb_column_out(x, a, top, K, LAB_NB, cv, h);
        for (int r0 = LAB_NB; r0 < m; r0 += 2 * LAB_NB) {                            // two row blocks in flight
            const int rows0 = m - r0 < LAB_NB ? m - r0 : LAB_NB, rows1 = m - r0 - LAB_NB < LAB_NB ? m - r0 - LAB_NB : LAB_NB;   // rows1 <= 0: no second block
            const unsigned t0 = top + (unsigned)(r0 * K), t1 = rows1 > 0 ? t0 + (unsigned)(LAB_NB * K) : t0;
            lab_f16 acc0 = labb_ctile(a, t0, K, rows0, cv, h), acc1 = labb_ctile(a, t1, K, rows1 > 0 ? rows1 : 1, cv && rows1 > 0, h);
            const float *l0 = Lp + (r0 + n31) * LAB_LP + h, *l1 = rows1 > 0 ? l0 + LAB_NB * LAB_LP : l0;   // rows past m are zeros in the panel
            lab_f16 av0, av1;
#pragma unroll
            for (int kk = 0; kk < 16; kk++) { av0[kk] = -l0[2 * kk]; av1[kk] = -l1[2 * kk]; }
#pragma unroll
            for (int kk = 0; kk < 16; kk++) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[kk], bv[kk], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[kk], bv[kk], acc1, 0, 0, 0);
            }
            labb_ctile_out(a, t0, acc0, K, rows0, cv, h);
            labb_ctile_out(a, t1, acc1, K, rows1, cv, h);
        }
    }
    return 0;
}

// ---- the substitution of inverse / luinv: X = U^-1 L^-1 P on the packed L\U, a wave per 32-column tile of X and no workgroup barrier, so all K
// right-hand columns are in flight over the four waves.  Each wave has two private LDS tiles [32][33]: T, a staged 32 x 32 block of L or U,
// and Xs, the block of right-hand sides being solved.  Right-looking over the block rows: solve the diagonal block in LDS, then one staged
// block and 16 MFMAs for every block row still to come.  X is touched in the C / D layout only, so every element stays with one lane.
__device__ __forceinline__ void labb_wave_sync() { Grp<M_WAVE> w; w.sync(); }
// T = the 32 x 32 block of a at (r0, c0), negated where it is an MFMA operand, zeros outside the matrix
__device__ __forceinline__ void labb_stage(float *T, const float *a, int K, int r0, int c0, int n31, int h, bool neg) {
    labb_wave_sync();                                                                // the tile's readers are done
    const bool cin = c0 + n31 < K;
    const unsigned src = (unsigned)(cin ? c0 + n31 : K - 1);
#pragma unroll
    for (int it = 0; it < 16; it++) {
        const int r = r0 + 2 * it + h;
        const float q = a[src + (unsigned)((r < K ? r : K - 1) * K)], v = (cin && r < K) ? q : 0.0f;
        T[(2 * it + h) * LAB_LP + n31] = neg ? -v : v;
    }
    labb_wave_sync();
}
// Xs (column n of lanes (n, 0) and (n, 1)) = T^-1 Xs, a column k of T at a time, the rows below (above) it dealt to the two halves.
// UPPER: divide by the diagonal; `rows` rows lie inside the matrix and the zero padding of a ragged block divides by 1.
template <bool UPPER>
__device__ __forceinline__ void labb_solve(float *Xs, const float *T, int rows, int n31, int h) {
    for (int s = 0; s < LAB_NB; s++) {
        const int k = UPPER ? LAB_NB - 1 - s : s;
        float xk = Xs[k * LAB_LP + n31];
        if (UPPER) { xk = xk / (k < rows ? T[k * LAB_LP + k] : 1.0f); labb_wave_sync(); if (h == 0) Xs[k * LAB_LP + n31] = xk; }
        if (UPPER) { for (int i = h; i < k; i += 2) Xs[i * LAB_LP + n31] -= T[i * LAB_LP + k] * xk; }
        else       { for (int i = k + 1 + h; i < LAB_NB; i += 2) Xs[i * LAB_LP + n31] -= T[i * LAB_LP + k] * xk; }
        labb_wave_sync();
    }
}
// the tile at gx[t] -= (block of a at (r0, c0)) * bv
__device__ __forceinline__ void labb_update(float *T, const float *a, float *gx, unsigned t, const lab_f16 &bv, int K, int r0, int c0, bool cv, int n31, int h) {
    const int rows = K - r0 < LAB_NB ? K - r0 : LAB_NB;
    lab_f16 acc = labb_ctile(gx, t, K, rows, cv, h);
    labb_stage(T, a, K, r0, c0, n31, h, true);
#pragma unroll
    for (int kk = 0; kk < 16; kk++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(T[n31 * LAB_LP + 2 * kk + h], bv[kk], acc, 0, 0, 0);
    labb_ctile_out(gx, t, acc, K, rows, cv, h);
}
// the diagonal step at block row r0: the tile of X into Xs, solved against the diagonal block, back to X; returns it as the B operand k = 2 kk + h
template <bool UPPER>
__device__ __forceinline__ lab_f16 labb_diag(float *T, float *Xs, const float *a, float *gx, unsigned t, int K, int r0, bool cv, int n31, int h) {
    const int rows = K - r0 < LAB_NB ? K - r0 : LAB_NB;
    lab_f16 c = labb_ctile(gx, t, K, rows, cv, h);
    labb_stage(T, a, K, r0, r0, n31, h, false);                                      // its syncs also fence Xs against the step before
#pragma unroll
    for (int v = 0; v < 16; v++) Xs[labb_crow(v, h) * LAB_LP + n31] = c[v];
    labb_wave_sync();
    labb_solve<UPPER>(Xs, T, rows, n31, h);
    lab_f16 bv;
#pragma unroll
    for (int v = 0; v < 16; v++) { c[v] = Xs[labb_crow(v, h) * LAB_LP + n31]; bv[v] = Xs[(2 * v + h) * LAB_LP + n31]; }
    labb_ctile_out(gx, t, c, K, rows, cv, h);
    return bv;
}
__device__ __forceinline__ void labb_subst(const float *a, float *gx, const int *perm, float *T, float *Xs, int K, int wv, int n31, int h) {
    const int nblk = labb_rows(K) / LAB_NB;
    for (int ct = wv; ct < nblk; ct += 4) {
        const int col = ct * LAB_NB + n31; const bool cv = col < K;
        const unsigned xc = (unsigned)(cv ? col : K - 1);                            // this lane's column of X (clamped: read, never written)
        for (int row = 4 * h; cv && row < K; row += 8) {                             // P, by the lanes that own the rows: X is a pure output
#pragma unroll
            for (int r = 0; r < 4; r++) if (row + r < K) gx[xc + (unsigned)((row + r) * K)] = perm[row + r] == col ? 1.0f : 0.0f;
        }
        for (int bk = 0; bk < nblk; bk++) {                                          // Y = L^-1 P, unit lower
            const lab_f16 bv = labb_diag<false>(T, Xs, a, gx, xc + (unsigned)(bk * LAB_NB * K), K, bk * LAB_NB, cv, n31, h);
            for (int bi = bk + 1; bi < nblk; bi++) labb_update(T, a, gx, xc + (unsigned)(bi * LAB_NB * K), bv, K, bi * LAB_NB, bk * LAB_NB, cv, n31, h);
        }
        for (int bk = nblk - 1; bk >= 0; bk--) {                                     // X = U^-1 Y
            const lab_f16 bv = labb_diag<true>(T, Xs, a, gx, xc + (unsigned)(bk * LAB_NB * K), K, bk * LAB_NB, cv, n31, h);
            for (int bi = 0; bi < bk; bi++) labb_update(T, a, gx, xc + (unsigned)(bi * LAB_NB * K), bv, K, bi * LAB_NB, bk * LAB_NB, cv, n31, h);
        }
    }
}

template <int OP>
__global__ void __launch_bounds__(BLK) k_lab_blocked(float *A, float *X, int *piv, float *det, int *status, int K, int vec) {
    extern __shared__ __attribute__((aligned(16))) float lab_sm[];
    Grp<M_GLOBAL> g; g.tid = threadIdx.x; g.nt = BLK;
    const int b = blockIdx.x;
    float *Lp = lab_sm;
    int *pivl = (int *)(Lp + labb_panel(K, OP == OP_INV || OP == OP_LUINV)), *perm = pivl + LAB_NB;
    g.red = (float *)(perm + K);
    const long ent = (long)b * K * K;
    float *a = A + ent, *gx = X ? X + ent : nullptr;
    int *pv = piv ? piv + (long)b * K : nullptr;
    for (int i = g.tid; i < K; i += g.nt) perm[i] = i;
    int st = 0, nswap = 0;
    for (int j = 0; j < K && st == 0; j += LAB_NB) st = labb_step(g, a, K, j, Lp, pivl, perm, pv, vec, nswap);
    g.sync();
    if (st == 0) {
        if (OP == OP_INV || OP == OP_LUINV) { float *T = Lp + (g.tid >> 6) * LAB_SUBST_WORDS; labb_subst(a, gx, perm, T, T + LAB_NB * LAB_LP, K, g.tid >> 6, g.tid & 31, (g.tid & 63) >> 5); }
        if (OP == OP_PLU && gx) lab_perm_matrix(g, perm, gx, K, K);
        if (OP == OP_DET) {
            float acc = 0.0f; int neg = 0;
            for (int j = g.tid; j < K; j += g.nt) { float d = a[j * K + j]; if (d < 0.0f) { neg ^= 1; d = -d; } acc += logf(d); }
            const float ld = grp_sum(g, acc, 0), ng = grp_sum(g, (float)neg, 8);
            if (g.tid == 0) det[b] = expf(ld) * (((nswap + (int)ng) & 1) ? -1.0f : 1.0f);
        }
    } else if (OP == OP_DET && g.tid == 0) det[b] = 0.0f;
    if (g.tid == 0) status[b] = st;
}

// ------------------------------------------------------------------ the plan: what the launch code uses, and what t4k_linalg_batched_plan reports
struct LabPlan { int regime, threads, nb, lds, wgs, vw, cwsh; };
enum { M_BLOCKED = 3 };
int lab_plan(LabPlan &p, const char *who, int op, int K, int batch, bool aligned) {
    if (op < OP_INV || op > OP_DET) return fail(T4K_ERR_ARG, "%s: no entry %d", who, op);
    if (K <= 0 || batch < 0) return fail(T4K_ERR_ARG, "%s: bad argument", who);
    if (K > LAB_K_MAX) return fail(T4K_ERR_UNSUPPORTED, "%s: K = %d above %d", who, K, LAB_K_MAX);
    const bool two = op == OP_INV || op == OP_LUINV;
    const int kblk = two ? LAB_K_BLK2 : LAB_K_BLK1, kb = two ? LAB_KB_X : LAB_K_BLK1;   // plu, det: no global regime
    const bool vec = ((long)K * K % 4 == 0) && aligned;
    p.threads = BLK; p.nb = 0; p.cwsh = 6;
    if (K <= LAB_K_WAVE)            { p.regime = M_WAVE;   p.lds = lab_words(M_WAVE, op, K) * 4 * (int)sizeof(float); p.wgs = (int)(((long)batch + 3) / 4); p.vw = vec ? 4 : 1;
                                      p.cwsh = K <= 4 ? 2 : K <= 8 ? 3 : K <= 16 ? 4 : 5; }
    else if (K <= kblk)             { p.regime = M_BLOCK;  p.lds = lab_words(M_BLOCK, op, K) * (int)sizeof(float);  p.wgs = batch; p.vw = vec ? 4 : 1; }
    else if (K <= kb)               { p.regime = M_GLOBAL; p.lds = lab_words(M_GLOBAL, op, K) * (int)sizeof(float); p.wgs = batch; p.vw = 1; }
    else                            { p.regime = M_BLOCKED; p.nb = LAB_NB; p.lds = labb_words(K, two) * (int)sizeof(float); p.wgs = batch; p.vw = (K % 4 == 0 && aligned) ? 4 : 1; }
    return T4K_OK;
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
int lab_go(float *A, float *X, int *piv, float *det, int *status, int K, int batch, const LabPlan &p, hipStream_t hs) {
    const size_t lds = (size_t)p.lds;
    if (lds > (size_t)LAB_LDS_MAX) return fail(T4K_ERR_UNSUPPORTED, "linalg_batched: K = %d needs %zu bytes of LDS", K, lds);
    if (lds > 65536) {
        static size_t granted = 0;                      // per instantiation
        if (lds > granted) { T4K_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lab<MODE, OP>), hipFuncAttributeMaxDynamicSharedMemorySize, LAB_LDS_MAX)); granted = LAB_LDS_MAX; }
    }
    T4K_LAUNCH((k_lab<MODE, OP>), dim3(p.wgs), dim3(BLK), lds, hs, A, X, piv, det, status, K, batch, p.cwsh, MODE == M_GLOBAL ? 0 : p.vw == 4);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}
template <int OP>
int lab_go_blocked(float *A, float *X, int *piv, float *det, int *status, int K, const LabPlan &p, hipStream_t hs) {
    static bool granted = false;                        // per instantiation
    if (!granted) { T4K_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lab_blocked<OP>), hipFuncAttributeMaxDynamicSharedMemorySize, LAB_LDS_MAX)); granted = true; }
    T4K_LAUNCH((k_lab_blocked<OP>), dim3(p.wgs), dim3(BLK), (size_t)p.lds, hs, A, X, piv, det, status, K, p.vw == 4);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}
template <int OP>
int lab_dispatch(const char *who, float *A, float *X, int *piv, float *det, int *status, int K, int batch, t4k_stream_t s) {
    LabPlan p;
    const bool al = aligned16(A) && (!X || aligned16(X));
    const int rc = lab_plan(p, who, OP, K, batch, al); if (rc != T4K_OK) return rc;
    if (batch == 0) return T4K_OK;
    if (p.regime == M_WAVE)   return lab_go<M_WAVE, OP>(A, X, piv, det, status, K, batch, p, S(s));
    if (p.regime == M_BLOCK)  return lab_go<M_BLOCK, OP>(A, X, piv, det, status, K, batch, p, S(s));
    if (p.regime == M_GLOBAL) return lab_go<M_GLOBAL, OP>(A, X, piv, det, status, K, batch, p, S(s));
    return lab_go_blocked<OP>(A, X, piv, det, status, K, p, S(s));
}

} // namespace

extern "C" {

int t4k_linalg_batched_plan(int entry, int K, int batch, int aligned, int out[8]) {
    if (!out) return fail(T4K_ERR_ARG, "t4k_linalg_batched_plan: null");
    LabPlan p;
    const int rc = lab_plan(p, "t4k_linalg_batched_plan", entry, K, batch, aligned != 0); if (rc != T4K_OK) return rc;
    out[0] = p.regime; out[1] = p.threads; out[2] = p.nb; out[3] = p.lds; out[4] = 1; out[5] = p.wgs; out[6] = p.vw; out[7] = 0;
    return T4K_OK;
}
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
