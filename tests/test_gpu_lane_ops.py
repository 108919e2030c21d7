"""The wave-wide butterflies of csrc/lane_ops.h (sum, max, first arg-max on the vector ALUs: lane swaps and DPP) against their __shfl_xor twins,
bit for bit.  The header's text is read from the tree, probe kernels are appended and the whole is compiled with hipRTC here; the GPU test loads the
code object through the HIP module API (ctypes, this process) and launches one wave per workgroup.  Per kernel: one header helper or one twin written
out below, NR rows side by side, NR in {1, 2, 13, 16}; all 64 lanes of every row are compared as uint32.

Inputs of the sums: (a) normal draws scaled by 2^k, k uniform in [-20, 20], mixed signs - a sum of those depends on the ORDER of its additions, so equal
bits pin the pairing tree and not just the total; (b) a single 1.0 walking through all 64 lanes - every lane is counted exactly once; (c) denormals,
zeros of both signs and infinities of one sign per row (no NaN).  Inputs of max and arg-max: ties at several lanes (the lowest index must win), the
-FLT_MAX / 0x7fffffff fill of dead lanes as the classifier head uses it; no zeros of mixed sign in a max row (the swap steps hand fmaxf its operands
in the other order in the upper half).

test_lane_ops_compile_for_gfx950 needs no device: the same text must compile for gfx950."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NRS = (1, 2, 13, 16)
FLT_MAX = np.float32(3.402823466e+38)
DEAD_I = 0x7fffffff

PROBES = r"""
template <int NR> __device__ __forceinline__ void twin_sum(float (&a)[NR]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float t[NR];
#pragma unroll
        for (int r = 0; r < NR; r++) t[r] = __shfl_xor(a[r], off, 64);
#pragma unroll
        for (int r = 0; r < NR; r++) a[r] += t[r];
    }
}
template <int NR> __device__ __forceinline__ void twin_max(float (&a)[NR]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int r = 0; r < NR; r++) a[r] = fmaxf(a[r], __shfl_xor(a[r], off, 64));
    }
}
template <int NR> __device__ __forceinline__ void twin_argmax(float (&m)[NR], int (&i)[NR]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const float m2 = __shfl_xor(m[r], off, 64); const int i2 = __shfl_xor(i[r], off, 64);
            if (m2 > m[r] || (m2 == m[r] && i2 < i[r])) { m[r] = m2; i[r] = i2; }
        }
    }
}
// one wave per workgroup; workgroup g owns rows [g NR, (g + 1) NR) of 64 lanes each.  Uniform code, all 64 lanes live.
#define PROBE1(name, fn, NR) extern "C" __global__ void __launch_bounds__(64) name##_##NR(const float *in, float *out) { \
    float a[NR]; const long base = (long)blockIdx.x * NR * 64 + threadIdx.x; \
    _Pragma("unroll") for (int r = 0; r < NR; r++) a[r] = in[base + r * 64]; \
    fn(a); \
    _Pragma("unroll") for (int r = 0; r < NR; r++) out[base + r * 64] = a[r]; }
#define PROBE2(name, fn, NR) extern "C" __global__ void __launch_bounds__(64) name##_##NR(const float *in, const int *idx, float *out, int *oidx) { \
    float m[NR]; int i[NR]; const long base = (long)blockIdx.x * NR * 64 + threadIdx.x; \
    _Pragma("unroll") for (int r = 0; r < NR; r++) { m[r] = in[base + r * 64]; i[r] = idx[base + r * 64]; } \
    fn(m, i); \
    _Pragma("unroll") for (int r = 0; r < NR; r++) { out[base + r * 64] = m[r]; oidx[base + r * 64] = i[r]; } }
#define PROBES_FOR(NR) PROBE1(sum_valu, lanes_sum_valu, NR) PROBE1(sum_twin, twin_sum, NR) PROBE1(max_valu, lanes_max_valu, NR) PROBE1(max_twin, twin_max, NR) \
    PROBE2(argmax_valu, lanes_argmax_valu, NR) PROBE2(argmax_twin, twin_argmax, NR)
PROBES_FOR(1) PROBES_FOR(2) PROBES_FOR(13) PROBES_FOR(16)
"""


def _source():
    return open(os.path.join(ROOT, "tensorforth_amd", "csrc", "lane_ops.h")).read() + PROBES


def _loaded(name):
    """the copy of a shared library this process already holds (torch brings its own HIP runtime), else the system's"""
    try:
        for line in open("/proc/self/maps"):
            path = line.split()[-1]
            if os.path.basename(path).startswith(name + ".so"):
                return ctypes.CDLL(path)
    except OSError:
        pass
    for cand in (name + ".so", "/opt/rocm/lib/" + name + ".so"):
        try:
            return ctypes.CDLL(cand)
        except OSError:
            continue
    raise RuntimeError(name + ".so not found")


def _compile(src):
    """hipRTC, gfx950, no device needed: the code object's bytes"""
    rtc = _loaded("libhiprtc")
    prog = ctypes.c_void_p()
    assert rtc.hiprtcCreateProgram(ctypes.byref(prog), src.encode(), b"lane_ops_probe.hip", 0, None, None) == 0
    opts = (ctypes.c_char_p * 3)(b"--offload-arch=gfx950", b"-O3", b"-std=c++17")
    rc = rtc.hiprtcCompileProgram(prog, 3, opts)
    if rc != 0:
        n = ctypes.c_size_t(); rtc.hiprtcGetProgramLogSize(prog, ctypes.byref(n))
        log = ctypes.create_string_buffer(n.value + 1); rtc.hiprtcGetProgramLog(prog, log)
        raise AssertionError("hiprtcCompileProgram failed (%d):\n%s" % (rc, log.value.decode(errors="replace")[-4000:]))
    n = ctypes.c_size_t(); assert rtc.hiprtcGetCodeSize(prog, ctypes.byref(n)) == 0
    code = ctypes.create_string_buffer(n.value); assert rtc.hiprtcGetCode(prog, code) == 0
    rtc.hiprtcDestroyProgram(ctypes.byref(prog))
    return code.raw


@pytest.fixture(scope="module")
def code():
    return _compile(_source())


def test_lane_ops_compile_for_gfx950(code):
    assert code[:4] == b"\177ELF" and len(code) > 4096
    for nr in NRS:
        for k in ("sum_valu", "sum_twin", "max_valu", "max_twin", "argmax_valu", "argmax_twin"):
            assert ("%s_%d" % (k, nr)).encode() in code


# ------------------------------------------------------------------------------------------------ inputs (rows of 64 lanes)
def _rows_sum():
    rng = np.random.default_rng(915)
    a = (rng.standard_normal((48, 64)) * np.exp2(rng.integers(-20, 21, (48, 64)))).astype(np.float32)           # (a)
    b = np.eye(64, dtype=np.float32)                                                                             # (b)
    den = np.float32(1e-45)
    c = np.zeros((8, 64), np.float32)                                                                            # (c)
    c[0] = rng.integers(1, 1 << 20, 64).astype(np.uint32).view(np.float32)                                       # denormals only
    c[1] = np.where(rng.random(64) < 0.5, den, -den)
    c[2] = -0.0
    c[3] = np.where(rng.random(64) < 0.5, np.float32(0.0), np.float32(-0.0))
    c[4] = rng.standard_normal(64).astype(np.float32); c[4, [5, 40]] = np.inf
    c[5] = rng.standard_normal(64).astype(np.float32); c[5, 63] = -np.inf
    c[6] = 0.0; c[6, 17] = den; c[6, 49] = -0.0
    c[7] = np.float32(1.17549435e-38); c[7, ::2] = -np.float32(1.17549435e-38); c[7, 3] = den
    rows = np.concatenate([a, b, c])
    assert not np.isnan(rows).any()
    return rows


def _rows_max():
    """(values, indices): the max kernels read the values alone"""
    rng = np.random.default_rng(916)
    v = rng.standard_normal((24, 64)).astype(np.float32)
    v[v == 0] = 1.0                                             # no zeros at all in these rows
    idx = np.tile(np.arange(64, dtype=np.int32), (24, 1))
    v[0] = 2.5                                                  # every lane ties: lane 0 wins
    v[1, [7, 39, 40, 63]] = 9.0                                 # ties across both halves and both rows of 16
    v[2, [33, 35]] = 9.0                                        # ties in the upper half only
    v[3, [16, 31]] = 9.0
    v[4, [62, 63]] = 9.0
    v[5] = -FLT_MAX; idx[5] = DEAD_I                            # a row of dead lanes only
    for r, live in ((6, 1), (7, 10), (8, 16), (9, 17), (10, 33), (11, 63)):        # the head's fill: lanes >= EB are dead
        v[r, live:] = -FLT_MAX; idx[r, live:] = DEAD_I
    v[12, :10] = 0.1; v[12, 10:] = -FLT_MAX; idx[12, 10:] = DEAD_I                  # softmax of equal logits: all live lanes tie
    v[13] = np.abs(v[13]); v[13, [20, 52]] = np.inf
    v[14] = -np.abs(v[14]) * np.float32(1e-40)                  # negative denormals
    v[15] = rng.permutation(64).astype(np.float32) + 1.0        # distinct values: a single winner somewhere
    return v, idx


def _pad(rows, nr, fill=0.0):
    g = -(-rows.shape[0] // nr)
    out = np.full((g * nr, 64), fill, rows.dtype); out[:rows.shape[0]] = rows
    return out, g


# ------------------------------------------------------------------------------------------------ the GPU run
class _Hip:
    def __init__(self, code):
        import torch
        self.torch = torch
        torch.cuda.init(); torch.zeros(1, device="cuda")        # the primary context, before the module API is used
        self.hip = _loaded("libamdhip64")
        self.mod = ctypes.c_void_p()
        assert self.hip.hipModuleLoadData(ctypes.byref(self.mod), code) == 0

    def launch(self, name, grid, *tensors):
        fn = ctypes.c_void_p()
        assert self.hip.hipModuleGetFunction(ctypes.byref(fn), self.mod, name.encode()) == 0, name
        ptrs = [ctypes.c_void_p(t.data_ptr()) for t in tensors]
        args = (ctypes.c_void_p * len(ptrs))(*[ctypes.cast(ctypes.byref(q), ctypes.c_void_p) for q in ptrs])
        self.torch.cuda.synchronize()
        assert self.hip.hipModuleLaunchKernel(fn, grid, 1, 1, 64, 1, 1, 0, None, args, None) == 0, name
        assert self.hip.hipDeviceSynchronize() == 0, name


@pytest.fixture(scope="module")
def hip(code):
    return _Hip(code)


@pytest.mark.gpu
@pytest.mark.parametrize("nr", NRS)
def test_lanes_sum_bits(hip, nr):
    torch = hip.torch
    rows, g = _pad(_rows_sum(), nr)
    x = torch.from_numpy(rows).cuda()
    got, want = torch.full_like(x, 7.0), torch.full_like(x, 9.0)
    hip.launch("sum_valu_%d" % nr, g, x, got)
    hip.launch("sum_twin_%d" % nr, g, x, want)
    got, want = got.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "NR %d: %d lanes differ, first (row, lane) %s: %08x vs %08x" % (nr, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    # the twin itself: the walking 1.0 sums to exactly 1.0 in every lane, whichever lane held it
    walk = want[48:48 + 64].view(np.float32)
    assert np.array_equal(walk, np.ones((64, 64), np.float32))
    assert not np.isnan(want.view(np.float32)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("nr", NRS)
def test_lanes_max_bits(hip, nr):
    torch = hip.torch
    v, _ = _rows_max()
    rows, g = _pad(v, nr, -FLT_MAX)
    x = torch.from_numpy(rows).cuda()
    got, want = torch.full_like(x, 7.0), torch.full_like(x, 9.0)
    hip.launch("max_valu_%d" % nr, g, x, got)
    hip.launch("max_twin_%d" % nr, g, x, want)
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "NR %d: rows %s differ" % (nr, np.unique(np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:, 0]))
    assert np.array_equal(want, np.repeat(rows.max(axis=1, keepdims=True), 64, axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("nr", NRS)
def test_lanes_argmax_bits(hip, nr):
    torch = hip.torch
    v, idx = _rows_max()
    rows, g = _pad(v, nr, -FLT_MAX)
    irows, _ = _pad(idx, nr, DEAD_I)
    x, xi = torch.from_numpy(rows).cuda(), torch.from_numpy(irows).cuda()
    out = [torch.full_like(x, 7.0), torch.full_like(xi, -5), torch.full_like(x, 9.0), torch.full_like(xi, -6)]
    hip.launch("argmax_valu_%d" % nr, g, x, xi, out[0], out[1])
    hip.launch("argmax_twin_%d" % nr, g, x, xi, out[2], out[3])
    gm, gi, wm, wi = (t.cpu().numpy() for t in out)
    assert np.array_equal(gm.view(np.uint32), wm.view(np.uint32)), "NR %d: max differs in rows %s" % (nr, np.unique(np.argwhere(gm.view(np.uint32) != wm.view(np.uint32))[:, 0]))
    assert np.array_equal(gi, wi), "NR %d: index differs in rows %s" % (nr, np.unique(np.argwhere(gi != wi)[:, 0]))
    # the twin itself: the largest value, and the lowest index among the lanes that hold it
    mx = rows.max(axis=1)
    first = np.array([irows[r][rows[r] == mx[r]].min() for r in range(rows.shape[0])], np.int32)
    assert np.array_equal(wm, np.repeat(mx[:, None], 64, axis=1)) and np.array_equal(wi, np.repeat(first[:, None], 64, axis=1))
