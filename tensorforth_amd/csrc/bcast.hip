// bcast.hip - NumPy-style broadcast arithmetic and the batched transpose of the rank-4 words.  Both are
// HBM-bound streaming kernels: one launch per call, no allocation, no synchronisation.  No reference definition: the
// reference's k_tt_op (src/t4math.cu:222) takes two flat tensors of one size, its k_transpose (:150) one sample.
#include "launch.h"

using namespace t4k;

namespace {

// the per-element expression of k_tt<OP> (elementwise.hip), restated: a result here is bit-identical to t4k_tt_op on
// operands expanded to the full shape
template <int OP> __device__ __forceinline__ float bin(float a, float b) {
    switch (OP) {
    case T4K_ADD: return a + b;
    case T4K_SUB: return a - b;
    case T4K_MUL: return a * b;
    case T4K_DIV: return a / b;
    }
    return a;
}

// What the host leaves after merging adjacent axes of equal broadcast status: a dense output of R runs of L elements.
// A run is the innermost merged axis (operand strides ia / ib along it: 1 = dense, 0 = one value for the whole run);
// the run index r splits into at most three outer digits (ext, outermost first, unused = 1) with operand strides sa / sb.
// Work is dealt by (run, position in run), never by a flat element index: a workgroup iteration takes `rpb` runs of
// `tpr` = 1 << shift lanes each (short runs), or one 256-lane chunk of the `nc` chunks of one run (long runs).
struct BcastPlan {
    long R, L, U;                 // runs, run length, units per run (L / 4 float4s on the vector path, else L)
    long nitem;                   // workgroup iterations: ceil(R / rpb) * nc
    long sa[3], sb[3], ia, ib;
    unsigned ext[3];
    unsigned nc, rpb, shift;      // one of nc / rpb is 1
};

template <int OP, bool VEC>
__global__ void __launch_bounds__(BLK) k_tt_bcast(const float *A, const float *B, float *O, const BcastPlan p) {
    const unsigned lane_run = threadIdx.x >> p.shift, lane_u = threadIdx.x & ((1u << p.shift) - 1u);
    for (long w = blockIdx.x; w < p.nitem; w += gridDim.x) {
        long rb = w; unsigned c = 0;
        if (p.nc > 1) divmod(w, p.nc, rb, c);                              // uniform over the workgroup: once per 256-lane chunk
        const long r = rb * p.rpb + lane_run, u = ((long)c << p.shift) + lane_u;
        if (r >= p.R || u >= p.U) continue;
        long t = r, offA = 0, offB = 0;
        unsigned i;
        if (p.ext[2] > 1) { divmod(t, p.ext[2], t, i); offA += (long)i * p.sa[2]; offB += (long)i * p.sb[2]; }
        if (p.ext[1] > 1) { divmod(t, p.ext[1], t, i); offA += (long)i * p.sa[1]; offB += (long)i * p.sb[1]; }
        offA += t * p.sa[0]; offB += t * p.sb[0];
        if (VEC) {                                                         // host: L % 4 == 0, 16-byte aligned runs, ia / ib in {0, 1}
            const long e = u << 2;
            float4 a, b;
            if (p.ia) a = *reinterpret_cast<const float4 *>(A + offA + e); else { const float v = A[offA]; a = make_float4(v, v, v, v); }
            if (p.ib) b = *reinterpret_cast<const float4 *>(B + offB + e); else { const float v = B[offB]; b = make_float4(v, v, v, v); }
            a.x = bin<OP>(a.x, b.x); a.y = bin<OP>(a.y, b.y); a.z = bin<OP>(a.z, b.z); a.w = bin<OP>(a.w, b.w);
            *reinterpret_cast<float4 *>(O + r * p.L + e) = a;
        } else
            O[r * p.L + u] = bin<OP>(A[offA + u * p.ia], B[offB + u * p.ib]);
    }
}

// k_transpose (elementwise.hip) with the entry and the channel folded into grid.z: z = b * C + c, walked in a loop when
// batch * C exceeds what the grid holds.  Same 64 x 65 LDS tile, same element order: bit exact.
__global__ void __launch_bounds__(BLK) k_transpose_batched(const float *__restrict__ src, float *__restrict__ dst, int H, int W, int C, long nz) {
    __shared__ float tile[64][65];
    const int j0 = blockIdx.x * 64, i0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;        // 64 x 4
    const long hw = (long)H * W;
    for (long z = blockIdx.z; z < nz; z += gridDim.z) {
        long b; unsigned c;
        divmod(z, (unsigned)C, b, c);
        const float *s = src + b * hw * C + c;
        float *d = dst + b * hw * C + c;
        for (int r = ty; r < 64; r += 4) {
            int i = i0 + r, j = j0 + tx;
            if (i < H && j < W) tile[r][tx] = s[((long)W * i + j) * C];
        }
        __syncthreads();
        for (int r = ty; r < 64; r += 4) {
            int j = j0 + r, i = i0 + tx;
            if (i < H && j < W) d[((long)H * j + i) * C] = tile[tx][r];
        }
        __syncthreads();                                           // the tile is rewritten by the next z
    }
}

// may an operand be read 16 bytes at a time along a run?  constant along it (one dword serves the run), or dense with every run
// starting on a multiple of four elements
inline bool run_vec_ok(long inner, const long outer[3]) {
    return inner == 0 || (inner == 1 && !((outer[0] | outer[1] | outer[2]) & 3));
}

} // namespace

extern "C" {

int t4k_tt_op_bcast(int op, const float *A, const float *B, float *O, const int dim[4], const long sA[4], const long sB[4], t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (!A || !B || !O || !dim || !sA || !sB) return fail(T4K_ERR_ARG, "t4k_tt_op_bcast: null");
    for (int i = 0; i < 4; i++)
        if (dim[i] < 0 || sA[i] < 0 || sB[i] < 0) return fail(T4K_ERR_ARG, "t4k_tt_op_bcast: negative extent or stride");
    if (op != T4K_ADD && op != T4K_SUB && op != T4K_MUL && op != T4K_DIV) return fail(T4K_ERR_UNSUPPORTED, "k_tt_op op=%d not supported", op);
    if (!dim[0] || !dim[1] || !dim[2] || !dim[3]) return T4K_OK;
    long total = 1;
    for (int i = 0; i < 4; i++) { if (total > (1L << 40) / dim[i]) return fail(T4K_ERR_ARG, "t4k_tt_op_bcast: more than 2^40 elements"); total *= dim[i]; }
    // axes of extent 1 drop out; neighbours merge when BOTH operands step through them as through one axis (dense on
    // dense, or broadcast on broadcast: s[outer] == s[inner] * d[inner]); the output is dense, so it always does
    long d[4], a[4], b[4]; int n = 0;
    for (int i = 0; i < 4; i++) {
        if (dim[i] == 1) continue;
        if (n && a[n - 1] == sA[i] * dim[i] && b[n - 1] == sB[i] * dim[i]) { d[n - 1] *= dim[i]; a[n - 1] = sA[i]; b[n - 1] = sB[i]; }
        else { d[n] = dim[i]; a[n] = sA[i]; b[n] = sB[i]; n++; }
    }
    if (!n) { d[0] = 1; a[0] = b[0] = 0; n = 1; }                          // a single element
    BcastPlan p = {};
    p.L = d[n - 1]; p.ia = a[n - 1]; p.ib = b[n - 1]; p.R = 1;
    for (int k = 0; k < 3; k++) { p.ext[k] = 1; p.sa[k] = p.sb[k] = 0; }
    for (int i = 0, k = 0; i < n - 1; i++, k++) {                          // left-aligned: the outermost digit is what the divisions leave
        if (d[i] > 0xffffffffL) return fail(T4K_ERR_ARG, "t4k_tt_op_bcast: merged extent too large");
        p.ext[k] = (unsigned)d[i]; p.sa[k] = a[i]; p.sb[k] = b[i]; p.R *= d[i];
    }
    // float4 path: whole runs of float4s, every run of O and of a dense operand starting on 16 bytes; an operand that is
    // constant along the run is read as one dword
    const bool vec = (p.L & 3) == 0 && aligned16(A) && aligned16(B) && aligned16(O) && run_vec_ok(p.ia, p.sa) && run_vec_ok(p.ib, p.sb);
    p.U = vec ? p.L >> 2 : p.L;
    p.shift = 0; while (p.shift < 8 && (1L << p.shift) < p.U) p.shift++;
    p.rpb = (unsigned)BLK >> p.shift;                                     // runs per workgroup iteration (1 once a run fills 256 lanes)
    p.nc = (unsigned)((p.U + BLK - 1) / BLK);                             // 256-lane chunks per run (1 below that)
    p.nitem = ((p.R + p.rpb - 1) / p.rpb) * p.nc;
    const int g = grid_for(p.nitem * BLK);
    pick<T4K_ADD, T4K_SUB, T4K_MUL, T4K_DIV>(op, [&](auto o) { with_flags([&](auto v) {
        T4K_LAUNCH((k_tt_bcast<o.value, v.value>), dim3(g), dim3(BLK), 0, S(s), A, B, O, p);
    }, vec); });
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

int t4k_transpose_batched(const float *src, float *dst, int H, int W, int C, int batch, t4k_stream_t s) {
    T4K_REQUIRE_INIT();
    if (H <= 0 || W <= 0 || C <= 0 || batch < 0) return fail(T4K_ERR_ARG, "t4k_transpose_batched: shape");
    if (!src || !dst) return fail(T4K_ERR_ARG, "t4k_transpose_batched: null");
    if (!batch) return T4K_OK;
    const long nz = (long)batch * C;
    const long gx = (W + 63) / 64, gy = (H + 63) / 64;
    if (gy > 65535) return fail(T4K_ERR_ARG, "t4k_transpose_batched: H too large");
    const long gz = std::max(1L, std::min(std::min(nz, 65535L), (1L << 31) / (gx * gy)));   // grid.z <= 65535 and 2^31 workgroups in all: the kernel walks the rest
    T4K_LAUNCH(k_transpose_batched, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(BLK), 0, S(s), src, dst, H, W, C, nz);
    T4K_LAUNCH_CHECK(); return T4K_OK;
}

} // extern "C"
