"""GPU parity: every t4k_* entry point of libt4hip.so (called through the C-ABI with raw
device pointers) against the CPU oracle on the same seeded inputs.
Bar: bit-exact for index/shape/integer work; 1e-4 relative for fp32 math (north_star)."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt

pytestmark = pytest.mark.gpu
RTOL = 1e-4


ELEM_FLOOR, ELEM_MIN = 1e-3, 0.9999


def rel(a, b):
    """tensor-norm figure max|a - b| / max|b| (the bit-level / 1e-6 checks of this file use it alone)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def relx(a, b, depth=1, elem_min=ELEM_MIN):
    """The figure every fp32-MATH comparison of this file is held to (`relx(got, want) < RTOL`; round 6) - the LARGER of
      * the tensor-norm figure max|a - b| / max|b|, and
      * the ELEMENT-aware figure (the bar of vm_util.check_tensor): the smallest t such that at least 99.99 % of the elements satisfy
        |a - b| <= t (|b| + floor max|b|) - every element held to its OWN magnitude, down to a floor of one thousandth of the tensor's largest element.
    depth = length of the fp32 sum behind an element (K of a GEMM, taps x channels of a conv, batch x pixels of a filter gradient).  BOTH sides are fp32
    sums of `depth` terms in different orders (the oracle's is the reference's sequential one): an element that cancels to near zero carries the rounding
    noise of its partial sums, ~sqrt(depth) eps max|b| on either side, and no implementation - the reference's included - has relative accuracy below
    that.  Measured with floor 1e-3: K = 980 products 1.2e-4, K = 2048 2.7e-4 (one element of 4 096).  So the floor grows with the depth,
    floor = 1e-3 max(1, sqrt(depth / 32)): 1e-3 up to 32-term sums and for every element-wise kernel, 5.7e-3 at K = 1 024, 2.8e-2 for the 25 088-term
    filter gradients (vm_util.check_tensor uses 1e-2 there for the same reason)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.size == 0:
        return 0.0
    floor = ELEM_FLOOR * max(1.0, (float(depth) / 32.0) ** 0.5)
    mx = max(1e-30, float(np.max(np.abs(b))))
    d = np.abs(a - b)
    r = np.sort((d / (np.abs(b) + floor * mx)).ravel())
    allowed = int((1.0 - elem_min) * r.size + 1e-9)
    return max(float(np.max(d)) / mx, float(r[r.size - 1 - allowed]))


class Dev:
    """device buffers via torch (plumbing only); pointers cross the ABI as integers"""

    def __init__(self, t4k):
        import torch
        self.torch = torch
        self.h = t4k
        t4k.call("t4k_set_default_stream", None)        # legacy null stream == torch's default stream
        self.keep = []      # hold every buffer: `p(dev.up(x))` temporaries must not be recycled mid-call

    def up(self, a, dtype=None):
        t = self.torch.from_numpy(np.array(a, copy=True)).cuda()
        self.keep.append(t)
        if len(self.keep) > 4000:
            del self.keep[:2000]
        return t

    def zeros(self, shape, dtype=None):
        t = self.torch.zeros(shape, dtype=dtype or self.torch.float32, device="cuda")
        self.keep.append(t)
        return t

    def down(self, t):
        self.h.call("t4k_sync", None)
        return t.cpu().numpy()


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


def p(t):
    return t.data_ptr()


# ----------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (128, 100, 1960), (100, 1960, 128), (128, 1960, 100),
                                   (128, 10, 100), (33, 17, 5), (1, 1, 1), (256, 256, 256), (200, 300, 77)])
@pytest.mark.parametrize("tA,tB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_vs_oracle(t4k, dev, oracle, M, N, K, tA, tB):
    rng = np.random.default_rng(M * 7 + N * 3 + K + tA * 2 + tB)
    D = K                                   # depth of the deepest fp32 sum behind a compared element (relx)
    A = rng.uniform(-1, 1, (K, M) if tA else (M, K)).astype(np.float32)
    B = rng.uniform(-1, 1, (N, K) if tB else (K, N)).astype(np.float32)
    O0 = rng.uniform(-1, 1, (M, N)).astype(np.float32)
    for alpha, beta in ((1.0, 0.0), (0.5, 2.0)):
        ref = oracle.gemm(A, B, O0.copy(), alpha, beta, tA, tB)
        dA, dB_, dO = dev.up(A), dev.up(B), dev.up(O0)
        t4k.call("t4k_gemm", p(dA), p(dB_), p(dO), alpha, beta, tA, tB, M, N, K, 1, None)
        assert relx(dev.down(dO), ref, D) < RTOL
        w = wt.gemm(A, B, O0, alpha, beta, tA, tB)                      # float64, every element within its own bound
        wt.check("gemm %dx%dx%d" % (M, N, K), dev.down(dO), w); wt.check("oracle gemm", ref, w)


def test_gemm_channel_interleaved_and_unaligned(t4k, dev, oracle):
    rng = np.random.default_rng(1)
    M, N, K, C = 20, 12, 9, 3
    A = rng.uniform(-1, 1, (M, K, C)).astype(np.float32); B = rng.uniform(-1, 1, (K, N, C)).astype(np.float32)
    ref = oracle.gemm(A, B, C=C)
    dA, dB_, dO = dev.up(A), dev.up(B), dev.zeros((M, N, C))
    t4k.call("t4k_gemm", p(dA), p(dB_), p(dO), 1.0, 0.0, 0, 0, M, N, K, C, None)
    assert relx(dev.down(dO), ref, K) < RTOL
    # operands at a 4-byte (not 16-byte) aligned address take the scalar-load path
    M, N, K = 64, 64, 64
    A = rng.uniform(-1, 1, (M * K + 1)).astype(np.float32); B = rng.uniform(-1, 1, (K * N + 1)).astype(np.float32)
    ref = oracle.gemm(A[1:].reshape(M, K), B[1:].reshape(K, N))
    dA, dB_, dO = dev.up(A), dev.up(B), dev.zeros((M, N))
    t4k.call("t4k_gemm", p(dA) + 4, p(dB_) + 4, p(dO), 1.0, 0.0, 0, 0, M, N, K, 1, None)
    assert relx(dev.down(dO), ref, K) < RTOL


def test_gemm_1024_exact_on_integer_operands(t4k, dev):
    """BASELINE config #2 at full size: small-integer operands make every fp32 partial sum
    exact, so the MFMA result must equal the int64 product bit for bit, in any k order."""
    rng = np.random.default_rng(1234)
    A = rng.integers(-2, 3, (1024, 1024)).astype(np.float32); B = rng.integers(-2, 3, (1024, 1024)).astype(np.float32)
    ref = (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float32)
    dA, dB_, dO = dev.up(A), dev.up(B), dev.zeros((1024, 1024))
    t4k.call("t4k_gemm", p(dA), p(dB_), p(dO), 1.0, 0.0, 0, 0, 1024, 1024, 1024, 1, None)
    assert np.array_equal(dev.down(dO), ref)
    # linearity: gemm(A, B; alpha=2, beta=1 on previous result) == 3 * ref
    t4k.call("t4k_gemm", p(dA), p(dB_), p(dO), 2.0, 1.0, 0, 0, 1024, 1024, 1024, 1, None)
    assert np.array_equal(dev.down(dO), 3 * ref)
    # the 128x128-tile variant (2048^2 output) on the same kind of data
    A2 = rng.integers(-2, 3, (2048, 512)).astype(np.float32); B2 = rng.integers(-2, 3, (512, 2048)).astype(np.float32)
    ref2 = (A2.astype(np.int64) @ B2.astype(np.int64)).astype(np.float32)
    dA, dB_, dO = dev.up(A2), dev.up(B2), dev.zeros((2048, 2048))
    t4k.call("t4k_gemm", p(dA), p(dB_), p(dO), 1.0, 0.0, 0, 0, 2048, 2048, 512, 1, None)
    assert np.array_equal(dev.down(dO), ref2)


def test_gemm_1024_uniform_vs_oracle(t4k, dev, oracle):
    rng = np.random.default_rng(1234)
    A = rng.uniform(0, 1, (1024, 1024)).astype(np.float32); B = rng.uniform(0, 1, (1024, 1024)).astype(np.float32)
    ref = oracle.gemm(A, B)
    dA, dB_, dO = dev.up(A), dev.up(B), dev.zeros((1024, 1024))
    t4k.call("t4k_gemm", p(dA), p(dB_), p(dO), 1.0, 0.0, 0, 0, 1024, 1024, 1024, 1, None)
    assert rel(dev.down(dO), ref) < 1e-5
    dO2 = dev.zeros((1024, 1024))
    t4k.call("t4k_gemm_f64acc", p(dA), p(dB_), p(dO2), 1.0, 0.0, 1024, 1024, 1024, 1, None)
    assert rel(dev.down(dO2), ref) < 1e-5


# ---------------------------------------------------------------- elementwise / reductions
def test_elementwise_ops(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(2)
    for n in (1, 3, 1000, 100003):
        x = rng.uniform(0.1, 2.0, n).astype(np.float32); y = rng.uniform(0.5, 2.0, n).astype(np.float32)
        for op in (oracle.ABS, oracle.NEG, oracle.EXP, oracle.LN, oracle.LOG, oracle.TANH, oracle.RELU, oracle.SIGM,
                   oracle.SQRT, oracle.RCP, oracle.SAT, oracle.FILL, oracle.GFILL, oracle.SCALE, oracle.POW,
                   oracle.ADD, oracle.SUB, oracle.MUL, oracle.DIV):
            a = (x - 1.0).copy() if op in (oracle.ABS, oracle.NEG, oracle.RELU, oracle.TANH, oracle.SAT) else x.copy()
            d = dev.up(a); o.t4o_math(op, P(a), 1.5, n)
            t4k.call("t4k_math", op, p(d), 1.5, n, None)
            assert relx(dev.down(d), a) < RTOL, op
        for op in (oracle.ADD, oracle.SUB, oracle.MUL, oracle.DIV):
            r = np.zeros_like(x); o.t4o_tt_op(op, P(x), P(y), P(r), n)
            dx, dy, dr = dev.up(x), dev.up(y), dev.zeros(n)
            t4k.call("t4k_tt_op", op, p(dx), p(dy), p(dr), n, None)
            assert np.array_equal(dev.down(dr), r)                 # single IEEE op: bit exact
            o.t4o_ts_op(op, P(x), 0.3, P(r), n)
            t4k.call("t4k_ts_op", op, p(dx), 0.3, p(dr), n, None)
            assert np.array_equal(dev.down(dr), r)
        dc = dev.zeros(n); t4k.call("t4k_copy", p(dev.up(x)), p(dc), n, None)
        assert np.array_equal(dev.down(dc), x)
    assert t4k.lib.t4k_math(99, p(dev.zeros(4)), 0.0, 4, None) == -4     # unsupported op reports, never aborts


def test_transpose_identity_bit_exact(t4k, dev, oracle):
    rng = np.random.default_rng(3)
    for H, W, C in ((5, 7, 1), (64, 64, 1), (100, 130, 3), (1, 9, 2)):
        a = rng.standard_normal((H, W, C)).astype(np.float32)
        d, t = dev.up(a), dev.zeros((W, H, C))
        t4k.call("t4k_transpose", p(d), p(t), H, W, C, None)
        assert np.array_equal(dev.down(t), a.transpose(1, 0, 2))
        e = dev.up(a); t4k.call("t4k_identity", p(e), H, W, C, None)
        ref = np.zeros((H, W, C), np.float32)
        for i in range(min(H, W)):
            ref[i, i, :] = 1
        assert np.array_equal(dev.down(e), ref)


def test_reductions(t4k, dev, oracle):
    rng = np.random.default_rng(4)
    for n in (5, 1000, 65536, 1 << 20):
        x = rng.standard_normal(n).astype(np.float32)
        d, out = dev.up(x), dev.zeros(1)
        t4k.call("t4k_reduce", oracle.RED_SUM, p(d), n, 0.0, p(out), None)
        assert abs(dev.down(out)[0] - x.astype(np.float64).sum()) < 1e-4 * max(1.0, np.abs(x).sum())
        avg = float(x.mean())
        t4k.call("t4k_reduce", oracle.RED_NVAR, p(d), n, avg, p(out), None)
        assert relx(dev.down(out)[0], ((x.astype(np.float64) - avg) ** 2).sum(), n) < RTOL
        t4k.call("t4k_reduce", oracle.RED_MAX, p(d), n, 0.0, p(out), None); assert dev.down(out)[0] == x.max()
        t4k.call("t4k_reduce", oracle.RED_MIN, p(d), n, 0.0, p(out), None); assert dev.down(out)[0] == x.min()
    x[17] = np.nan; x[99] = np.inf
    cnt = dev.zeros(1, dev.torch.int32)
    t4k.call("t4k_nan_inf", p(dev.up(x)), x.size, p(cnt), None); assert dev.down(cnt)[0] == 2
    # BCE
    o = oracle.lib(); P = oracle.P
    t = rng.integers(0, 2, 5000).astype(np.float32); y = rng.uniform(0.01, 0.99, 5000).astype(np.float32)
    r = np.zeros(1, np.float32); o.t4o_bce(P(t), P(y), 5000, P(r)); out = dev.zeros(1)
    t4k.call("t4k_bce", p(dev.up(t)), p(dev.up(y)), 5000, p(out), None)
    assert relx(dev.down(out)[0], r[0], 300) < RTOL
    # dot with channel stride
    A = rng.standard_normal((300, 3)).astype(np.float32); B = rng.standard_normal((300, 3)).astype(np.float32)
    O = np.ones(3, np.float32); dO = dev.up(O)
    o.t4o_dot(P(A), P(B), P(O), 2.0, 0.5, 300, 3)
    t4k.call("t4k_dot", p(dev.up(A)), p(dev.up(B)), p(dO), 2.0, 0.5, 300, 3, None)
    assert relx(dev.down(dO), O, 300) < RTOL


# ------------------------------------------------------------------------------- nn
@pytest.mark.parametrize("K,S,P_", [(1, 1, 0), (3, 1, 1), (4, 2, 1), (5, 1, 2)])
@pytest.mark.parametrize("N,H1,C1,C0", [(2, 6, 2, 3), (3, 14, 10, 20), (4, 28, 1, 10), (2, 8, 40, 72), (2, 10, 3, 16), (1, 12, 64, 33),
                                        (2, 8, 32, 64), (3, 10, 64, 32), (2, 6, 96, 128), (2, 9, 32, 20),    # these four: LDS-staged many-channel kernels
                                        (2, 8, 64, 128), (3, 8, 128, 64), (1, 12, 128, 256), (5, 6, 64, 68),
                                        (2, 10, 3, 64), (3, 9, 4, 64), (5, 7, 1, 64), (2, 11, 2, 64)])   # ... and the image-input layer with a full tile or two of output channels (k_conv_thin_fwd), odd grids, ragged last tile; the four before: round 4: 8-wave LDS-DMA kernel (64-channel stages; 128- and 64-wide tiles, ragged pixel / channel edges)
def test_conv2d(t4k, dev, oracle, K, S, P_, N, H1, C1, C0):
    o = oracle.lib(); P = oracle.P
    D = max(K * K * max(C1, C0), N * H1 * H1)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    rng = np.random.default_rng(K + N)
    I = rng.standard_normal((N, H1, H1, C1)).astype(np.float32)
    F = rng.standard_normal((C1, K, K, C0)).astype(np.float32); B = rng.standard_normal(C0).astype(np.float32)
    ref = oracle.conv2d_fwd(I, F, B, K, S, P_); H0 = ref.shape[1]
    dI, dF, dB_, dO = dev.up(I), dev.up(F), dev.up(B), dev.zeros(ref.shape)
    t4k.call("t4k_conv2d_fwd", p(dI), p(dO), p(dF), p(dB_), N, H1, H1, C1, H0, H0, C0, K, S, P_, None)
    assert relx(dev.down(dO), ref, D) < RTOL
    w = wt.conv_fwd(I, F, B, S, P_)
    wt.check("conv2d fwd", dev.down(dO), w); wt.check("oracle conv2d fwd", ref, w)
    g = rng.standard_normal(ref.shape).astype(np.float32)
    DX = np.zeros_like(I); DF = rng.standard_normal(F.shape).astype(np.float32); DB = rng.standard_normal(C0).astype(np.float32)
    DF0, DB0 = DF.copy(), DB.copy()
    dDX, dDF, dDB, dg = dev.zeros(I.shape), dev.up(DF), dev.up(DB), dev.up(g)
    o.t4o_conv2d_bwd(P(I), P(g), P(DX), P(F), P(DF), P(DB), N, H1, H1, C1, H0, H0, C0, K, S, P_, 1)
    t4k.call("t4k_conv2d_bwd", p(dI), p(dg), p(dDX), p(dF), p(dDF), p(dDB), N, H1, H1, C1, H0, H0, C0, K, S, P_, 1, None)
    assert relx(dev.down(dDX), DX, D) < RTOL and relx(dev.down(dDF), DF, D) < RTOL and relx(dev.down(dDB), DB, D) < RTOL
    wdx, wdf, wdb = wt.conv_dx(g, F, H1, H1, S, P_), wt.conv_df(I, g, K, S, P_, acc=DF0), wt.conv_db(g, acc=DB0)
    wt.check("conv2d dX", dev.down(dDX), wdx); wt.check("conv2d dF", dev.down(dDF), wdf); wt.check("conv2d dB", dev.down(dDB), wdb)
    wt.check("oracle conv2d dX", DX, wdx); wt.check("oracle conv2d dF", DF, wdf); wt.check("oracle conv2d dB", DB, wdb)
    # train == 0 leaves DF/DB untouched
    t4k.call("t4k_conv2d_bwd", p(dI), p(dg), p(dDX), p(dF), p(dDF), p(dDB), N, H1, H1, C1, H0, H0, C0, K, S, P_, 0, None)
    assert relx(dev.down(dDF), DF, D) < RTOL
    wt.check("conv2d dF (train 0)", dev.down(dDF), wdf)


def test_conv2d_unsupported_geometry_is_reported(t4k, dev):
    z = dev.zeros(16)
    assert t4k.lib.t4k_conv2d_fwd(p(z), p(z), p(z), p(z), 1, 4, 4, 1, 4, 4, 1, 7, 1, 3, None) == -4
    assert b"not supported" in t4k.lib.t4k_last_error()


@pytest.mark.parametrize("KS", [2, 3])
@pytest.mark.parametrize("H1", [12, 7])
def test_pool_and_dpool(t4k, dev, oracle, KS, H1):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(KS * H1)
    N, C = 3, 5; H0 = (H1 + KS - 1) // KS
    I = rng.standard_normal((N, H1, H1, C)).astype(np.float32)
    dy = rng.standard_normal((N, H0, H0, C)).astype(np.float32)
    for layer in (oracle.L_MAXPOOL, oracle.L_AVGPOOL, oracle.L_MINPOOL):
        O = np.zeros((N, H0, H0, C), np.float32); o.t4o_pool(layer, P(I), P(O), N, H1, H1, H0, H0, C, KS)
        dI, dO = dev.up(I), dev.zeros(O.shape)
        t4k.call("t4k_pool", layer, p(dI), p(dO), N, H1, H1, H0, H0, C, KS, None)
        got = dev.down(dO)
        assert np.array_equal(got, O) if layer != oracle.L_AVGPOOL else rel(got, O) < 1e-6
        X = I.copy(); o.t4o_dpool(layer, P(X), P(dy), N, H1, H1, H0, H0, C, KS)
        t4k.call("t4k_dpool", layer, p(dI), p(dev.up(dy)), N, H1, H1, H0, H0, C, KS, None)
        got = dev.down(dI)
        assert np.array_equal(got, X) if layer != oracle.L_AVGPOOL else rel(got, X) < 1e-6


def test_activations_softmax_bias(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(6)
    n = 12345
    x = rng.standard_normal(n).astype(np.float32); r = rng.random(n).astype(np.float32)
    for layer, alpha in ((oracle.L_RELU, 0), (oracle.L_TANH, 0), (oracle.L_SIGMOID, 0), (oracle.L_SELU, 0),
                         (oracle.L_LEAKYRL, 0.01), (oracle.L_ELU, 1.0), (oracle.L_DROPOUT, 0.5)):
        y = np.zeros_like(x); f = r.copy(); o.t4o_activate(layer, P(x), P(y), P(f), alpha, n)
        dx, dy_, df = dev.up(x), dev.zeros(n), dev.up(r)
        t4k.call("t4k_activate", layer, p(dx), p(dy_), p(df), alpha, n, None)
        gy, gf = dev.down(dy_), dev.down(df)
        if layer in (oracle.L_RELU, oracle.L_DROPOUT):
            assert np.array_equal(gy, y) and np.array_equal(gf, f)          # masks are exact
        else:
            assert relx(gy, y) < RTOL and relx(gf, f) < RTOL
    for N, C in ((128, 10), (5, 300), (1, 1)):
        a = (rng.standard_normal((N, C)) * 4).astype(np.float32); y = np.zeros_like(a)
        o.t4o_softmax(P(a), P(y), N, C); dy_ = dev.zeros((N, C))
        t4k.call("t4k_softmax", p(dev.up(a)), p(dy_), N, C, None)
        assert relx(dev.down(dy_), y) < RTOL
    Y = rng.standard_normal((128, 100)).astype(np.float32); b = rng.standard_normal(100).astype(np.float32)
    dY = dev.up(Y); o.t4o_bias(P(b), P(Y), 128, 100)
    t4k.call("t4k_bias", p(dev.up(b)), p(dY), 128, 100, None)
    assert np.array_equal(dev.down(dY), Y)


@pytest.mark.parametrize("N,E0,E1", [(128, 100, 1960), (128, 10, 100), (3, 2, 2), (256, 512, 784), (128, 100, 980), (200, 72, 516), (31, 68, 12)])
def test_linear_fwd_bwd(t4k, dev, oracle, N, E0, E1):
    o = oracle.lib(); P = oracle.P
    D = max(E1, E0, N)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    rng = np.random.default_rng(N + E0)
    X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) * 0.1).astype(np.float32)
    b = rng.standard_normal(E0).astype(np.float32)
    Y = np.zeros((N, E0), np.float32); o.t4o_linear_fwd(P(X), P(W), P(b), P(Y), N, E0, E1)
    dX, dW, db, dY = dev.up(X), dev.up(W), dev.up(b), dev.zeros((N, E0))
    t4k.call("t4k_linear_fwd", p(dX), p(dW), p(db), p(dY), N, E0, E1, None)
    assert relx(dev.down(dY), Y, D) < RTOL
    G = rng.standard_normal((N, E0)).astype(np.float32)
    DW = rng.standard_normal((E0, E1)).astype(np.float32); DB = rng.standard_normal(E0).astype(np.float32)
    DX = np.zeros_like(X)
    dG, dDW, dDB = dev.up(G), dev.up(DW), dev.up(DB)
    o.t4o_linear_bwd(P(X), P(W), P(G), P(DX), P(DW), P(DB), N, E0, E1, 1)
    t4k.call("t4k_linear_bwd", p(dX), p(dW), p(dG), p(dX), p(dDW), p(dDB), N, E0, E1, 1, None)   # dX in place (as the host does)
    assert relx(dev.down(dX), DX, D) < RTOL and relx(dev.down(dDW), DW, D) < RTOL and relx(dev.down(dDB), DB, D) < RTOL
    # again on fresh buffers (the one-launch dW|dX path re-arms its arrival gate), accumulating into the same dW / dB
    o.t4o_linear_bwd(P(X), P(W), P(G), P(DX), P(DW), P(DB), N, E0, E1, 1)
    dX2 = dev.up(X)
    t4k.call("t4k_linear_bwd", p(dX2), p(dW), p(dG), p(dX2), p(dDW), p(dDB), N, E0, E1, 1, None)
    assert relx(dev.down(dX2), DX, D) < RTOL and relx(dev.down(dDW), DW, D) < RTOL and relx(dev.down(dDB), DB, D) < RTOL
    DBo = DB.copy(); o.t4o_dlinear_db(P(G), P(DBo), N, E0)
    t4k.call("t4k_dlinear_db", p(dG), p(dDB), N, E0, None)
    assert relx(dev.down(dDB), DBo, D) < RTOL


@pytest.mark.parametrize("N,HW,C", [(8, 49, 6), (16, 256, 70), (4, 1024, 128)])   # single-launch stats / chunked column sums
def test_batchnorm(t4k, dev, oracle, N, HW, C):
    _batchnorm_case(t4k, dev, oracle, N, HW, C)


@pytest.mark.parametrize("N,HW,C", [(8, 49, 6), (16, 256, 70)])
def test_batchnorm_synchronised_statistics_world_one(t4k, dev, oracle, N, HW, C):
    """With a communicator attached the statistics go partials -> sums -> all-reduce -> finalise (data-parallel batch norm);
    one rank must reproduce the plain path's (= the oracle's) result."""
    import ctypes
    lib = t4k.lib
    raw = (ctypes.c_ubyte * 128)()
    assert lib.t4k_comm_unique_id(raw) == 0 and lib.t4k_comm_init(raw, 0, 1) == 0, lib.t4k_last_error()
    try:
        _batchnorm_case(t4k, dev, oracle, N, HW, C)          # a communicator alone changes nothing: synchronised statistics are opt-in
        assert lib.t4k_comm_sync_batchnorm(1) == 0
        _batchnorm_case(t4k, dev, oracle, N, HW, C)          # ... and this is the all-reduce path
        # conv + batch-norm (+ run) in one call under synchronised statistics: no epilogue rider, the sums go through the all-reduce; same tensors
        test_conv_with_batchnorm_behind_it_matches_the_two_layers(t4k, dev, oracle, 8, 16, 64, 128)
        test_conv_batchnorm_and_the_run_behind_them_in_one_call(t4k, dev, oracle, 8, 16, 64, 128)
    finally:
        lib.t4k_comm_destroy()


def _batchnorm_case(t4k, dev, oracle, N, HW, C):
    o = oracle.lib(); P = oracle.P
    D = N * HW                                   # depth of the deepest fp32 sum behind a compared element (relx)
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((N, HW, C)) * 2 + 1).astype(np.float32)
    g = rng.standard_normal(C).astype(np.float32); b = rng.standard_normal(C).astype(np.float32)
    y = np.zeros_like(x); xh = np.zeros_like(x); stat = np.zeros(3 * C, np.float32)
    o.t4o_batchnorm_fwd(P(x), P(y), P(xh), P(g), P(b), P(stat), N, HW, C)
    dx, dg, db, dy_, dxh, dst = dev.up(x), dev.up(g), dev.up(b), dev.zeros(x.shape), dev.zeros(x.shape), dev.zeros(3 * C)
    t4k.call("t4k_batchnorm_fwd", p(dx), p(dy_), p(dxh), p(dg), p(db), p(dst), N, HW, C, None)
    assert relx(dev.down(dy_), y, D) < RTOL and relx(dev.down(dxh), xh, D) < RTOL and relx(dev.down(dst)[:2 * C], stat[:2 * C], D) < RTOL
    gy = rng.standard_normal(x.shape).astype(np.float32)
    DX = np.zeros_like(x); DW = np.ones(C, np.float32); DB = np.ones(C, np.float32)
    o.t4o_batchnorm_bwd(P(g), P(gy), P(xh), P(DX), P(DW), P(DB), P(stat), N, HW, C, 1)
    dDX, dDW, dDB = dev.zeros(x.shape), dev.up(np.ones(C, np.float32)), dev.up(np.ones(C, np.float32))
    t4k.call("t4k_batchnorm_bwd", p(dg), p(dev.up(gy)), p(dxh), p(dDX), p(dDW), p(dDB), p(dst), N, HW, C, 1, None)
    assert relx(dev.down(dDX), DX, D) < 5e-4 and relx(dev.down(dDW), DW, D) < RTOL and relx(dev.down(dDB), DB, D) < RTOL


@pytest.mark.parametrize("N,H,C1,C0", [(64, 16, 3, 64),      # image in, 64 channels out: k_conv_thin_fwd carries the sums (a partial pair per workgroup)
                                       (8, 16, 64, 128),     # k_convbig8, 128-wide tiles (16 of them: two 64-row partial pairs each)
                                       (16, 8, 64, 64),      # k_convbig8, 64-wide tiles
                                       (5, 7, 64, 128),      # 245 pixels: a ragged tile -> no rider, the two layers one after the other
                                       (16, 8, 10, 20)])     # a layer whose kernel carries no rider
def test_conv_with_batchnorm_behind_it_matches_the_two_layers(t4k, dev, oracle, N, H, C1, C0):
    """t4k_conv2d_bn_fwd (Model::_fconv + Model::_fbatchnorm): the conv output, x-hat, the batch-norm output and the statistics equal the oracle's conv followed by
    its batch norm; where the conv kernel carries the per-channel sums in its epilogue the separate statistics pass is not launched - same tensors, the sums in
    another (fixed) order.  T4K_CONV_BN_RIDER=0 (tests/test_gpu_switches.py) runs the two calls."""
    D = max(9 * max(C1, C0), N * H * H)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(21)
    x = rng.standard_normal((N, H, H, C1)).astype(np.float32); f = (rng.standard_normal((C1, 3, 3, C0)) * 0.2).astype(np.float32); bc = rng.standard_normal(C0).astype(np.float32)
    g = rng.standard_normal(C0).astype(np.float32); b = rng.standard_normal(C0).astype(np.float32)
    y = np.zeros((N, H, H, C0), np.float32); out = np.zeros_like(y); xh = np.zeros_like(y); stat = np.zeros(3 * C0, np.float32)
    o.t4o_conv2d_fwd(P(x), P(y), P(f), P(bc), N, H, H, C1, H, H, C0, 3, 1, 1)
    o.t4o_batchnorm_fwd(P(y), P(out), P(xh), P(g), P(b), P(stat), N, H * H, C0)
    dx, df, dbc, dg, db = dev.up(x), dev.up(f), dev.up(bc), dev.up(g), dev.up(b)
    dic, dy, do, dxh, dst = dev.zeros(x.shape), dev.zeros(y.shape), dev.zeros(y.shape), dev.zeros(y.shape), dev.zeros(3 * C0)
    t4k.call("t4k_conv2d_bn_fwd", p(dx), p(dic), p(dy), p(df), p(dbc), N, H, H, C1, H, H, C0, 3, 1, 1, p(do), p(dxh), p(dg), p(db), p(dst), None)
    assert np.array_equal(dev.down(dic), x)
    assert relx(dev.down(dy), y, D) < RTOL and relx(dev.down(dst)[:2 * C0], stat[:2 * C0], D) < RTOL
    assert relx(dev.down(dxh), xh, D) < 5e-4 and relx(dev.down(do), out, D) < 5e-4
    # the same call twice gives the same bits (fixed fold order), and so do the two separate calls up to the order of the sums
    do2, dxh2, dst2, dy2 = dev.zeros(y.shape), dev.zeros(y.shape), dev.zeros(3 * C0), dev.zeros(y.shape)
    t4k.call("t4k_conv2d_bn_fwd", p(dx), None, p(dy2), p(df), p(dbc), N, H, H, C1, H, H, C0, 3, 1, 1, p(do2), p(dxh2), p(dg), p(db), p(dst2), None)
    assert np.array_equal(dev.down(do2), dev.down(do)) and np.array_equal(dev.down(dst2)[:2 * C0], dev.down(dst)[:2 * C0])
    t4k.call("t4k_conv2d_fwd", p(dx), p(dy2), p(df), p(dbc), N, H, H, C1, H, H, C0, 3, 1, 1, None)
    t4k.call("t4k_batchnorm_fwd", p(dy2), p(do2), p(dxh2), p(dg), p(db), p(dst2), N, H * H, C0, None)
    assert np.array_equal(dev.down(dy2), dev.down(dy)) and rel(dev.down(do2), dev.down(do)) < 1e-5


def test_optimizers_and_multi_tensor_step(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(9)
    n = 197210                                                     # C128 parameter count (SURVEY a-18)
    w = rng.standard_normal(n).astype(np.float32); g = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32); v = (np.abs(rng.standard_normal(n)) * 0.1).astype(np.float32)
    for kind in ("sgd0", "sgdm", "adam", "adamw"):
        W, G, M, V = w.copy(), g.copy(), m.copy(), v.copy()
        dW, dG, dM, dV = dev.up(w), dev.up(g), dev.up(m), dev.up(v)
        if kind == "sgd0":
            o.t4o_sgd(P(W), P(G), P(M), 3, 0.01, 0.0, n); t4k.call("t4k_sgd", p(dW), p(dG), p(dM), 3, 0.01, 0.0, n, None)
        elif kind == "sgdm":
            o.t4o_sgd(P(W), P(G), P(M), 1, 0.01, 0.9, n); t4k.call("t4k_sgd", p(dW), p(dG), p(dM), 1, 0.01, 0.9, n, None)
        elif kind == "adam":
            o.t4o_adam(P(W), P(G), P(M), P(V), 1e-3, 0.9, 0.999, n); t4k.call("t4k_adam", p(dW), p(dG), p(dM), p(dV), 1e-3, 0.9, 0.999, n, None)
        else:
            o.t4o_adamw(P(W), P(G), P(M), P(V), 1e-3, 0.9, 0.999, 0.01, n); t4k.call("t4k_adamw", p(dW), p(dG), p(dM), p(dV), 1e-3, 0.9, 0.999, 0.01, n, None)
        # optim.hip is compiled without floating-point contraction and spells the update out in the oracle's operation order: SGD (with and without
        # momentum) and both moment tensors of Adam agree bit for bit; Adam's weights differ on a few elements per thousand by a rounding of the quotient (root / division)
        got_w, got_m, got_v = dev.down(dW), dev.down(dM), dev.down(dV)
        assert np.array_equal(got_m, M) and np.array_equal(got_v, V)
        if kind in ("sgd0", "sgdm"):
            assert np.array_equal(got_w, W)
        else:
            ulp = np.abs(got_w.view(np.int32).astype(np.int64) - W.view(np.int32).astype(np.int64))
            assert (ulp != 0).mean() < 0.01 and rel(got_w, W) < 1e-6     # (an element that cancels to near zero shows a rounding of the quotient as many of ITS ulps)
        assert not dev.down(dG).any()                               # gradients zeroed by the step
    # multi-tensor launch == per-tensor launches
    sizes = [90, 10, 196000, 100, 1000, 10]
    import struct
    bufs = []; recs = b""
    for i, sz in enumerate(sizes):
        W = rng.standard_normal(sz).astype(np.float32); G = rng.standard_normal(sz).astype(np.float32)
        dW, dG, dM, dV = dev.up(W), dev.up(G), dev.zeros(sz), dev.zeros(sz)
        M = np.zeros(sz, np.float32); V = np.zeros(sz, np.float32)
        o.t4o_adam(P(W), P(G), P(M), P(V), 1e-3, 0.9, 0.999, sz)
        bufs.append((dW, dG, dM, dV, W))
        recs += struct.pack("<QQQQqii", p(dW), p(dG), p(dM), p(dV), sz, 1, 0)
    tab = dev.up(np.frombuffer(recs, np.uint8))
    t4k.call("t4k_opt_multi", 1, p(tab), len(sizes), max(sizes), 1e-3, 0.9, 0.999, 0.0, None)
    for dW, dG, dM, dV, W in bufs:
        assert rel(dev.down(dW), W) < 1e-6 and not dev.down(dG).any()
    # launch sized to the parameters (t4k_opt_chunked): `pad` = the tensor's first 1024-element chunk; SGD with momentum, second step
    bufs = []; recs = b""; chunk = 0
    for i, sz in enumerate(sizes):
        W = rng.standard_normal(sz).astype(np.float32); G = rng.standard_normal(sz).astype(np.float32); M = (rng.standard_normal(sz) * 0.1).astype(np.float32)
        dW, dG, dM = dev.up(W), dev.up(G), dev.up(M)
        o.t4o_sgd(P(W), P(G), P(M), 1 + i % 3, 0.01, 0.9, sz)
        bufs.append((dW, dG, dM, W, M))
        recs += struct.pack("<QQQQqii", p(dW), p(dG), p(dM), p(dM), sz, 1 + i % 3, chunk); chunk += (sz + 1023) // 1024
    tab = dev.up(np.frombuffer(recs, np.uint8))
    t4k.call("t4k_opt_chunked", 0, p(tab), len(sizes), chunk, 0.01, 0.9, 0.0, 0.0, None)
    for dW, dG, dM, W, M in bufs:
        assert np.array_equal(dev.down(dW), W) and np.array_equal(dev.down(dM), M) and not dev.down(dG).any()


def test_onehot_hit_u8(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(10)
    N, E = 128, 10
    lab = rng.integers(0, 12, N).astype(np.uint32)                  # some labels >= classes -> class 0
    hot = np.zeros((N, E), np.float32); o.t4o_onehot(P(lab), P(hot), N, E)
    dhot = dev.zeros((N, E)); dlab = dev.up(lab.view(np.int32))
    t4k.call("t4k_onehot", p(dlab), p(dhot), N, E, None)
    assert np.array_equal(dev.down(dhot), hot)
    out = rng.standard_normal((N, E)).astype(np.float32); out[5, 3] = out[5, 7] = 9.0     # tie: first max wins
    c = ctypes.c_int(0); o.t4o_hit(P(out), P(hot), N, E, ctypes.byref(c))
    dc = dev.zeros(1, dev.torch.int32)
    t4k.call("t4k_hit", p(dev.up(out)), p(dhot), N, E, p(dc), None)
    assert int(dev.down(dc)[0]) == c.value
    u8 = rng.integers(0, 256, 128 * 784).astype(np.uint8); ref = np.zeros(u8.size, np.float32)
    o.t4o_u8_normalize(P(u8), P(ref), u8.size, 128.0, 1 / 128.0)
    d = dev.zeros(u8.size); t4k.call("t4k_u8_normalize", p(dev.up(u8)), p(d), u8.size, 128.0, 1 / 128.0, None)
    assert np.array_equal(dev.down(d), ref)
    for n, nlab in ((128 * 784, 128), (1003, 5), (3, 700), (0, 9)):  # pixels + labels in one launch; ragged tail; more labels than pixel lanes
        d = dev.zeros(max(n, 1)); dl = dev.zeros(nlab, dev.torch.int32); lab2 = rng.integers(0, 1 << 31, nlab).astype(np.int32)
        t4k.call("t4k_stage_batch", p(dev.up(u8[:max(n, 1)])), p(d), n, 128.0, 1 / 128.0, p(dev.up(lab2)), p(dl), nlab, None)
        assert np.array_equal(dev.down(d)[:n], ref[:n]) and np.array_equal(dev.down(dl), lab2), (n, nlab)


@pytest.mark.parametrize("N,E", [(128, 10), (77, 10), (300, 7), (1, 1), (513, 32), (64, 100), (301, 256), (37, 1000), (260, 257)])
def test_hit_count_shapes(t4k, dev, oracle, N, E):
    """every lanes-per-sample variant of k_hit (1 / 8 / 64), ragged batch counts, ties resolved towards the first maximum"""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N * 1000 + E)
    out = rng.integers(-3, 4, (N, E)).astype(np.float32)             # small integers: many ties in every row
    hot = np.zeros((N, E), np.float32); hot[np.arange(N), rng.integers(0, E, N)] = 1.0
    hot[::3] = 0; hot[::3, 0] = 1.0                                  # a third of the rows point at class 0 (the common first-max)
    c = ctypes.c_int(0); o.t4o_hit(P(out), P(hot), N, E, ctypes.byref(c))
    dc = dev.zeros(1, dev.torch.int32)
    t4k.call("t4k_hit", p(dev.up(out)), p(dev.up(hot)), N, E, p(dc), None)
    assert int(dev.down(dc)[0]) == c.value
    want = int(hot[np.arange(N), out.argmax(1)].sum())               # numpy's argmax is the first maximum too
    assert c.value == want
    # labels -> one-hot rows and the count in one launch (labels >= E fall on class 0, as t4k_onehot)
    lab = rng.integers(0, E + 2, N).astype(np.uint32)
    hot2 = np.zeros((N, E), np.float32); o.t4o_onehot(P(lab), P(hot2), N, E); c2 = ctypes.c_int(0); o.t4o_hit(P(out), P(hot2), N, E, ctypes.byref(c2))
    dh = dev.up(np.full((N, E), 7.0, np.float32)); dc.zero_()
    t4k.call("t4k_onehot_hit", p(dev.up(lab.view(np.int32))), p(dh), p(dev.up(out)), N, E, p(dc), None)
    assert np.array_equal(dev.down(dh), hot2) and int(dev.down(dc)[0]) == c2.value


def test_rand_matches_oracle_stream(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    for n in (1, 5, 4096, 100001):
        o.t4o_rand_init(777); t4k.call("t4k_rand_init", 777)
        a = np.zeros(n, np.float32); b = np.zeros(n, np.float32)
        o.t4o_rand(P(a), n, 0, -0.5, 0.2); o.t4o_rand(P(b), n, 1, 0.0, 1.0)
        da, db = dev.zeros(n), dev.zeros(n)
        t4k.call("t4k_rand", p(da), n, 0, -0.5, 0.2, None); t4k.call("t4k_rand", p(db), n, 1, 0.0, 1.0, None)
        assert np.array_equal(dev.down(da), a)                       # integer stream + one fma: bit exact
        assert np.max(np.abs(dev.down(db) - b)) < 1e-4               # Box-Muller: libm vs device ulps
        assert t4k.lib.t4k_rand_offset() == o.t4o_rand_offset()


def test_linear_algebra(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(11)
    for K in (3, 4, 17, 64):
        A = (rng.standard_normal((K, K)) + np.eye(K) * 2).astype(np.float32)
        a, I = A.copy(), np.eye(K, dtype=np.float32); st = ctypes.c_int(0)
        o.t4o_inverse(P(a), P(I), K, ctypes.byref(st))
        dA, dI, dst = dev.up(A), dev.up(np.eye(K, dtype=np.float32)), dev.zeros(1, dev.torch.int32)
        t4k.call("t4k_inverse", p(dA), p(dI), K, p(dst), None)
        assert dev.down(dst)[0] == 0 and relx(dev.down(dI), I) < 1e-3
        a, I, piv = A.copy(), np.eye(K, dtype=np.float32), np.zeros(K, np.int32)
        o.t4o_lu_inverse(P(a), P(I), P(piv), K, ctypes.byref(st))
        dA, dI, dpiv = dev.up(A), dev.up(np.eye(K, dtype=np.float32)), dev.zeros(K, dev.torch.int32)
        t4k.call("t4k_lu_inverse", p(dA), p(dI), p(dpiv), K, p(dst), None)
        assert np.array_equal(dev.down(dpiv), piv) and relx(dev.down(dI), I) < 1e-3 and relx(dev.down(dA), a) < 1e-3
        ld = np.zeros(1, np.float32); sg = ctypes.c_int(0); o.t4o_logdet(P(a), K, P(ld), ctypes.byref(sg))
        dld, dsg = dev.zeros(1), dev.zeros(1, dev.torch.int32)
        t4k.call("t4k_logdet", p(dA), K, p(dld), p(dsg), None)
        assert abs(dev.down(dld)[0] - ld[0]) < 1e-3 and dev.down(dsg)[0] == sg.value
        for get_u in (0, 1):
            ref = a.copy(); o.t4o_lu_extract(P(ref), get_u, K)
            d = dev.up(a); t4k.call("t4k_lu_extract", p(d), get_u, K, None)
            assert np.array_equal(dev.down(d), ref)
    sing = np.array([[1, 2], [2, 4]], np.float32)
    dst = dev.zeros(1, dev.torch.int32)
    t4k.call("t4k_inverse", p(dev.up(sing)), p(dev.up(np.eye(2, dtype=np.float32))), 2, p(dst), None)
    assert dev.down(dst)[0] == 2


def test_graph_capture_replays_a_launch_sequence(t4k, dev):
    """hipGraph capture of t4k launches on a private stream (the step-graph mechanism)."""
    s = ctypes.c_void_p(); t4k.call("t4k_stream_create", ctypes.byref(s))
    x = dev.up(np.ones(1000, np.float32)); dev.h.call("t4k_sync", None)
    g = ctypes.c_void_p()
    t4k.call("t4k_graph_begin", s)
    t4k.call("t4k_math", 14, p(x), 2.0, 1000, s)          # SCALE by 2
    t4k.call("t4k_math", 16, p(x), 1.0, 1000, s)          # ADD 1
    t4k.call("t4k_graph_end", s, ctypes.byref(g))
    for _ in range(3):
        t4k.call("t4k_graph_launch", g, s)
    t4k.call("t4k_sync", s)
    assert np.all(x.cpu().numpy() == 15.0)                # ((1*2+1)*2+1)*2+1
    t4k.call("t4k_graph_destroy", g); t4k.call("t4k_stream_destroy", s)


# ----------------------------------------------------------------------------- fused element-wise runs
class PoolBlock(ctypes.Structure):
    _fields_ = [("pre_layer", ctypes.c_int), ("pre_alpha", ctypes.c_float), ("pre_mask", ctypes.c_void_p), ("pre_out", ctypes.c_void_p),
                ("pool_layer", ctypes.c_int), ("KS", ctypes.c_int), ("pool_out", ctypes.c_void_p),
                ("post_layer", ctypes.c_int), ("post_alpha", ctypes.c_float), ("post_mask", ctypes.c_void_p), ("post_out", ctypes.c_void_p),
                ("copy_out", ctypes.c_void_p)]


@pytest.mark.parametrize("C", [5, 6, 8])             # scalar, 8-byte and 16-byte channel vectors
@pytest.mark.parametrize("pre,pool,post,flat,KS,H1", [
    ("dropout", "max", "relu", True, 2, 14),      # LeNet block 2: conv -> dropout -> maxpool -> relu -> flatten
    (None, "max", "relu", False, 2, 28),          # LeNet block 1: conv -> maxpool -> relu
    ("leaky", "avg", "tanh", True, 3, 9),
    ("relu", None, "elu", False, 1, 6),
    ("dropout", None, None, True, 1, 5),
    (None, "min", "selu", True, 2, 8),
])
def test_poolblock_matches_unfused_oracle(t4k, dev, oracle, pre, pool, post, flat, KS, H1, C):
    """One fused launch each way == the oracle's separate layers (activate / rand / pool / dpool / mask multiply),
    every intermediate tensor included.  Dropout masks come from the same Philox slice => bit-exact."""
    o = oracle.lib(); P = oracle.P
    LAY = {"dropout": (oracle.L_DROPOUT, 0.5), "relu": (oracle.L_RELU, 0.0), "leaky": (oracle.L_LEAKYRL, 0.1), "tanh": (oracle.L_TANH, 0.0),
           "elu": (oracle.L_ELU, 1.0), "selu": (oracle.L_SELU, 0.0), "max": oracle.L_MAXPOOL, "avg": oracle.L_AVGPOOL, "min": oracle.L_MINPOOL}
    rng = np.random.default_rng(H1 * 31 + KS)
    N = 3; H0 = H1 // KS
    n1, n0 = N * H1 * H1 * C, N * H0 * H0 * C
    X = rng.standard_normal((N, H1, H1, C)).astype(np.float32)
    DY = rng.standard_normal((N, H0, H0, C)).astype(np.float32)
    seed, off = 77, 4096
    # ---- oracle: separate layers
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    ref = {}; x = X
    if pre:
        L, a = LAY[pre]; f = np.zeros(n1, np.float32); y = np.zeros_like(X)
        if pre == "dropout":
            o.t4o_rand(P(f), n1, 0, 0.0, 1.0)
        o.t4o_activate(L, P(x), P(y), P(f), a, n1); ref["pre_mask"] = f; ref["pre_out"] = y; x = y
    if pool:
        q = np.zeros((N, H0, H0, C), np.float32); o.t4o_pool(LAY[pool], P(x), P(q), N, H1, H1, H0, H0, C, KS); ref["pool_out"] = q; x = q
    if post:
        L, a = LAY[post]; f = np.zeros(n0, np.float32); y = np.zeros((N, H0, H0, C), np.float32)
        o.t4o_activate(L, P(x), P(y), P(f), a, n0); ref["post_mask"] = f; ref["post_out"] = y; x = y
    if flat:
        ref["copy_out"] = x.copy()
    # ---- GPU: one launch
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
    d = {k: dev.zeros(v.shape) for k, v in ref.items()}
    dX = dev.up(X)
    blk = PoolBlock()
    blk.KS = KS
    if pre:
        blk.pre_layer, blk.pre_alpha = LAY[pre]; blk.pre_mask = p(d["pre_mask"]); blk.pre_out = p(d["pre_out"])
    if pool:
        blk.pool_layer = LAY[pool]; blk.pool_out = p(d["pool_out"])
    if post:
        blk.post_layer, blk.post_alpha = LAY[post]; blk.post_mask = p(d["post_mask"]); blk.post_out = p(d["post_out"])
    if flat:
        blk.copy_out = p(d["copy_out"])
    t4k.call("t4k_poolblock_fwd", p(dX), ctypes.byref(blk), N, H1, H1, H0, H0, C, None)
    for k_, v in ref.items():
        got = dev.down(d[k_]).reshape(v.shape)
        assert rel(got, v) < 1e-6, k_
    if pre == "dropout":
        assert np.array_equal(dev.down(d["pre_mask"]).ravel(), ref["pre_mask"])        # masks are 0/1: exact
        assert t4k.lib.t4k_rand_offset() == o.t4o_rand_offset()                        # stream advanced identically
    # ---- backward: oracle separate layers (in-place convention), GPU one launch
    g = DY.copy()
    bufs = {k_: v.copy() for k_, v in ref.items()}; Xb = X.copy()
    last = "post_out" if post else ("pool_out" if pool else ("pre_out" if pre else None))
    if flat:
        (bufs[last] if last else Xb)[...] = g.reshape((bufs[last] if last else Xb).shape)
    if post:
        tgt = bufs["pool_out"] if pool else (bufs["pre_out"] if pre else Xb)
        t = np.zeros(n0, np.float32); o.t4o_tt_op(oracle.MUL, P(g), P(ref["post_mask"]), P(t), n0); tgt[...] = t.reshape(tgt.shape); g = tgt.copy()
    if pool:
        tgt = bufs["pre_out"] if pre else Xb
        o.t4o_dpool(LAY[pool], P(tgt), P(g), N, H1, H1, H0, H0, C, KS); g = tgt.copy()
    if pre:
        t = np.zeros(n1, np.float32); o.t4o_tt_op(oracle.MUL, P(g), P(ref["pre_mask"]), P(t), n1); Xb[...] = t.reshape(Xb.shape)
    t4k.call("t4k_poolblock_bwd", p(dev.up(DY)), p(dX), ctypes.byref(blk), N, H1, H1, H0, H0, C, None)
    assert rel(dev.down(dX), Xb) < 1e-6
    for k_ in ("pre_out", "pool_out", "post_out"):
        if k_ in bufs and not (k_ == last and not flat):
            assert rel(dev.down(d[k_]).reshape(bufs[k_].shape), bufs[k_]) < 1e-6, "bwd " + k_


@pytest.mark.parametrize("N,H,C1,C0,K,pre,post,flat,icopy", [
    (128, 14, 10, 20, 3, "dropout", "relu", True, False),      # LeNet conv2 block
    (16, 28, 1, 10, 3, None, "relu", False, True),             # LeNet conv1 block: layer-0 copy written by the conv launch
    (5, 12, 3, 8, 5, "relu", None, False, True),               # 5x5, 3 input channels, odd batch
    (4, 8, 6, 40, 3, "dropout", "leaky", True, False),         # two output-channel tiles (40 > 32), Cout % 4 == 0 -> quad-shared Philox
    (3, 6, 5, 7, 3, "dropout", None, False, False),            # Cout % 4 != 0 -> per-element Philox path
    (2, 16, 64, 64, 3, None, "relu", False, False),            # many channels: not fusable in-kernel, the entry composes the launches
    (3, 10, 3, 64, 3, None, "relu", False, True),              # image-input layer with many output channels: coalesced dX (16 lanes per pixel)
    (2, 8, 1, 32, 3, None, None, False, False),                # ... 8 lanes per pixel
    (1, 6, 4, 128, 3, "relu", None, False, False),             # ... 32 lanes per pixel
])
def test_conv_block_forward_and_dual_store_backward(t4k, dev, oracle, N, H, C1, C0, K, pre, post, flat, icopy):
    """t4k_conv2d_block_fwd == t4k_conv2d_fwd + the element-wise run as separate oracle layers (every tensor of the run, the
    optional layer-0 copy, dropout masks bit-exact and the Philox stream advanced identically); t4k_conv2d_bwd2's second dX
    copy equals dX."""
    D = max(K * K * max(C1, C0), N * H * H)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    LAY = {"dropout": (oracle.L_DROPOUT, 0.5), "relu": (oracle.L_RELU, 0.0), "leaky": (oracle.L_LEAKYRL, 0.1)}
    rng = np.random.default_rng(N * 7 + C0)
    Pd = K // 2; H0 = H; Hp = H // 2
    X = rng.standard_normal((N, H, H, C1)).astype(np.float32); F = (rng.standard_normal((C1, K, K, C0)) * 0.3).astype(np.float32)
    B = rng.standard_normal(C0).astype(np.float32)
    n1, n0 = N * H0 * H0 * C0, N * Hp * Hp * C0
    seed, off = 91, 8192
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    Y = np.zeros((N, H0, H0, C0), np.float32); o.t4o_conv2d_fwd(P(X), P(Y), P(F), P(B), N, H, H, C1, H0, H0, C0, K, 1, Pd)
    ref = {}; x = Y
    if pre:
        L, a = LAY[pre]; f = np.zeros(n1, np.float32); y = np.zeros_like(Y)
        if pre == "dropout": o.t4o_rand(P(f), n1, 0, 0.0, 1.0)
        o.t4o_activate(L, P(x), P(y), P(f), a, n1); ref["pre_mask"] = f; ref["pre_out"] = y; x = y
    q = np.zeros((N, Hp, Hp, C0), np.float32); o.t4o_pool(oracle.L_MAXPOOL, P(x), P(q), N, H0, H0, Hp, Hp, C0, 2); ref["pool_out"] = q; x = q
    if post:
        L, a = LAY[post]; f = np.zeros(n0, np.float32); y = np.zeros_like(q)
        o.t4o_activate(L, P(x), P(y), P(f), a, n0); ref["post_mask"] = f; ref["post_out"] = y; x = y
    if flat: ref["copy_out"] = x.copy()
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
    d = {k: dev.zeros(v.shape) for k, v in ref.items()}
    dX, dF, dB, dY, dXC = dev.up(X), dev.up(F), dev.up(B), dev.zeros(Y.shape), dev.zeros(X.shape)
    blk = PoolBlock(); blk.KS = 2; blk.pool_layer = oracle.L_MAXPOOL; blk.pool_out = p(d["pool_out"])
    if pre: blk.pre_layer, blk.pre_alpha = LAY[pre]; blk.pre_mask = p(d["pre_mask"]); blk.pre_out = p(d["pre_out"])
    if post: blk.post_layer, blk.post_alpha = LAY[post]; blk.post_mask = p(d["post_mask"]); blk.post_out = p(d["post_out"])
    if flat: blk.copy_out = p(d["copy_out"])
    t4k.call("t4k_conv2d_block_fwd", p(dX), p(dXC) if icopy else None, p(dY), p(dF), p(dB), ctypes.byref(blk), N, H, H, C1, H0, H0, C0, K, 1, Pd, None)
    assert relx(dev.down(dY), Y, D) < RTOL
    if icopy: assert np.array_equal(dev.down(dXC), X)
    if pre == "dropout":
        assert np.array_equal(dev.down(d["pre_mask"]).ravel(), ref["pre_mask"])
        assert t4k.lib.t4k_rand_offset() == o.t4o_rand_offset()
    for k_, v in ref.items():
        if k_.endswith("mask") and k_ != "pre_mask" or (k_ == "pre_mask" and pre != "dropout"):
            # derivative masks flip where the pre-activation sits within rounding distance of zero: compare away from it
            continue
        assert relx(dev.down(d[k_]).reshape(v.shape), v, D) < RTOL, k_
    # backward with the second dX copy (the reference's `in = dx`)
    G = rng.standard_normal(Y.shape).astype(np.float32)
    DX = np.zeros_like(X); DF = np.zeros_like(F); DB = np.zeros_like(B)
    o.t4o_conv2d_bwd(P(X), P(G), P(DX), P(F), P(DF), P(DB), N, H, H, C1, H0, H0, C0, K, 1, Pd, 1)
    dG, dDX, dDX2, dDF, dDB = dev.up(G), dev.zeros(X.shape), dev.zeros(X.shape), dev.zeros(F.shape), dev.zeros(B.shape)
    t4k.call("t4k_conv2d_bwd2", p(dX), p(dG), p(dDX), p(dDX2), p(dF), p(dDF), p(dDB), N, H, H, C1, H0, H0, C0, K, 1, Pd, 1, None)
    assert relx(dev.down(dDX), DX, D) < RTOL and np.array_equal(dev.down(dDX2), dev.down(dDX))
    assert relx(dev.down(dDF), DF, D) < RTOL and relx(dev.down(dDB), DB, D) < RTOL


@pytest.mark.parametrize("N,H,C1,C0", [(16, 16, 3, 64), (8, 16, 64, 128), (4, 7, 64, 64), (8, 8, 10, 20)])
def test_conv_batchnorm_and_the_run_behind_them_in_one_call(t4k, dev, oracle, N, H, C1, C0):
    """t4k_conv2d_bn_block_fwd (the CIFAR-style block conv -> batchnorm -> relu -> maxpool -> dropout): conv output, x-hat, batch-norm output, relu mask / output, pool
    output, dropout mask / output against the oracle's layers one after the other (dropout mask bit-exact, the Philox stream advanced identically), and bit-equal
    to the library's own separate calls t4k_conv2d_bn_fwd + t4k_poolblock_fwd (the fused pass reads the conv output once; same expressions per element)."""
    D = max(9 * max(C1, C0), N * H * H)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N + H + C0)
    Hp = (H + 1) // 2
    X = rng.standard_normal((N, H, H, C1)).astype(np.float32); F = (rng.standard_normal((C1, 3, 3, C0)) * 0.3).astype(np.float32); Bc = rng.standard_normal(C0).astype(np.float32)
    g = rng.standard_normal(C0).astype(np.float32); b = rng.standard_normal(C0).astype(np.float32)
    n1, n0 = N * H * H * C0, N * Hp * Hp * C0
    seed, off = 77, 4096
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    Y = np.zeros((N, H, H, C0), np.float32); o.t4o_conv2d_fwd(P(X), P(Y), P(F), P(Bc), N, H, H, C1, H, H, C0, 3, 1, 1)
    BO = np.zeros_like(Y); XH = np.zeros_like(Y); stat = np.zeros(3 * C0, np.float32)
    o.t4o_batchnorm_fwd(P(Y), P(BO), P(XH), P(g), P(b), P(stat), N, H * H, C0)
    rm = np.zeros(n1, np.float32); ro = np.zeros_like(Y); o.t4o_activate(oracle.L_RELU, P(BO), P(ro), P(rm), 0.0, n1)
    q = np.zeros((N, Hp, Hp, C0), np.float32); o.t4o_pool(oracle.L_MAXPOOL, P(ro), P(q), N, H, H, Hp, Hp, C0, 2)
    dm = np.zeros(n0, np.float32); o.t4o_rand(P(dm), n0, 0, 0.0, 1.0); do_ = np.zeros_like(q); o.t4o_activate(oracle.L_DROPOUT, P(q), P(do_), P(dm), 0.25, n0)

    def run(fused):
        t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
        d = {k: dev.zeros(v) for k, v in (("Y", Y.shape), ("BO", Y.shape), ("XH", Y.shape), ("st", (3 * C0,)), ("rm", Y.shape), ("ro", Y.shape), ("q", q.shape), ("dm", q.shape), ("do", q.shape))}
        blk = PoolBlock(); blk.KS = 2; blk.pool_layer = oracle.L_MAXPOOL; blk.pool_out = p(d["q"])
        blk.pre_layer, blk.pre_alpha = oracle.L_RELU, 0.0; blk.pre_mask = p(d["rm"]); blk.pre_out = p(d["ro"])
        blk.post_layer, blk.post_alpha = oracle.L_DROPOUT, 0.25; blk.post_mask = p(d["dm"]); blk.post_out = p(d["do"])
        dX, dF, dBc, dg, db = dev.up(X), dev.up(F), dev.up(Bc), dev.up(g), dev.up(b)
        if fused:
            t4k.call("t4k_conv2d_bn_block_fwd", p(dX), None, p(d["Y"]), p(dF), p(dBc), N, H, H, C1, H, H, C0, 3, 1, 1,
                     p(d["BO"]), p(d["XH"]), p(dg), p(db), p(d["st"]), ctypes.byref(blk), Hp, Hp, None)
        else:
            t4k.call("t4k_conv2d_bn_fwd", p(dX), None, p(d["Y"]), p(dF), p(dBc), N, H, H, C1, H, H, C0, 3, 1, 1, p(d["BO"]), p(d["XH"]), p(dg), p(db), p(d["st"]), None)
            t4k.call("t4k_poolblock_fwd", p(d["BO"]), ctypes.byref(blk), N, H, H, Hp, Hp, C0, None)
        return {k: dev.down(v) for k, v in d.items()}, t4k.lib.t4k_rand_offset()
    a, offa = run(True)
    assert offa == o.t4o_rand_offset()
    assert relx(a["Y"], Y, D) < RTOL and relx(a["st"][:2 * C0], stat[:2 * C0], D) < RTOL and relx(a["XH"], XH, D) < 5e-4 and relx(a["BO"], BO, D) < 5e-4
    assert np.array_equal(a["dm"].ravel(), dm) and relx(a["ro"], ro, D) < 5e-4 and relx(a["q"], q, D) < 5e-4 and relx(a["do"], do_, D) < 5e-4
    c, offc = run(False)
    assert offc == offa
    for k in a: assert np.array_equal(a[k], c[k]), k


@pytest.mark.parametrize("N,E0,E1", [(128, 10, 100), (7, 3, 17), (256, 1, 256), (64, 40, 200), (33, 48, 130)])
def test_small_linear_head_is_bit_identical_to_oracle(t4k, dev, oracle, N, E0, E1):
    """Classifier-head path (linear_small.hip): fmaf chains in ascending k, the oracle's order => exact equality
    for Y and dX (dX written over X, as the host does); dW, dB (batch split over lane groups) and the fused softmax within 1e-6."""
    D = max(E1, E0, N)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N * 3 + E0)
    X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) * 0.2).astype(np.float32)
    b = rng.standard_normal(E0).astype(np.float32)
    Y = np.zeros((N, E0), np.float32); o.t4o_linear_fwd(P(X), P(W), P(b), P(Y), N, E0, E1)
    Pr = np.zeros_like(Y); o.t4o_softmax(P(Y), P(Pr), N, E0)
    dX, dW, db, dY, dP = dev.up(X), dev.up(W), dev.up(b), dev.zeros((N, E0)), dev.zeros((N, E0))
    t4k.call("t4k_linear_softmax_fwd", p(dX), p(dW), p(db), p(dY), p(dP), N, E0, E1, None)
    assert np.array_equal(dev.down(dY), Y)
    assert rel(dev.down(dP), Pr) < 1e-6
    G = rng.standard_normal((N, E0)).astype(np.float32)
    DW = rng.standard_normal((E0, E1)).astype(np.float32); DB = rng.standard_normal(E0).astype(np.float32)
    DX = np.zeros_like(X)
    dG, dDW, dDB = dev.up(G), dev.up(DW), dev.up(DB)
    o.t4o_linear_bwd(P(X), P(W), P(G), P(DX), P(DW), P(DB), N, E0, E1, 1)
    t4k.call("t4k_linear_bwd", p(dX), p(dW), p(dG), p(dX), p(dDW), p(dDB), N, E0, E1, 1, None)
    assert np.array_equal(dev.down(dX), DX) and rel(dev.down(dDW), DW) < 1e-6 and relx(dev.down(dDB), DB, D) < RTOL
    # second launch on fresh buffers (counter re-armed), separate DX buffer (no aliasing)
    dXb, dDXb = dev.up(X), dev.zeros(X.shape)
    DW2 = np.zeros((E0, E1), np.float32); DB2 = np.zeros(E0, np.float32); DXb = np.zeros_like(X)
    o.t4o_linear_bwd(P(X), P(W), P(G), P(DXb), P(DW2), P(DB2), N, E0, E1, 1)
    dDW2, dDB2 = dev.zeros((E0, E1)), dev.zeros(E0)
    t4k.call("t4k_linear_bwd", p(dXb), p(dW), p(dG), p(dDXb), p(dDW2), p(dDB2), N, E0, E1, 1, None)
    assert np.array_equal(dev.down(dDXb), DXb) and rel(dev.down(dDW2), DW2) < 1e-6 and relx(dev.down(dDB2), DB2, D) < RTOL
    dXc = dev.up(X)
    t4k.call("t4k_linear_bwd", p(dXc), p(dW), p(dG), p(dXc), p(dDW2), p(dDB2), N, E0, E1, 1, None)   # aliasing again
    assert np.array_equal(dev.down(dXc), DX)


@pytest.mark.parametrize("N,E0,E1,mask,train", [(128, 10, 100, True, 1), (128, 10, 100, False, 1), (7, 3, 17, True, 1), (64, 40, 200, False, 1),
                                                 (128, 10, 100, True, 0), (32, 100, 700, False, 1)])
def test_loss_prep_folded_into_linear_backward(t4k, dev, oracle, N, E0, E1, mask, train):
    """t4k_loss_linear_bwd == `out -= target` + pass-through copy + t4k_linear_bwd2 (backprop.cu:60-75, 122-131, 193-254), in one
    launch when the head is small (in-place store gated by arrival counters), as separate launches otherwise: same values."""
    D = max(E1, E0, N)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N + E0 + E1)
    X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) * 0.2).astype(np.float32)
    OUT = rng.random((N, E0)).astype(np.float32); TGT = (rng.random((N, E0)) > 0.9).astype(np.float32)
    M = (rng.random((N, E1)) > 0.5).astype(np.float32)
    DW = rng.standard_normal((E0, E1)).astype(np.float32); DB = rng.standard_normal(E0).astype(np.float32)
    G = OUT - TGT
    DX = np.zeros_like(X); DWr, DBr = DW.copy(), DB.copy()
    o.t4o_linear_bwd(P(X), P(W), P(G), P(DX), P(DWr), P(DBr), N, E0, E1, train)
    for rep_ in range(2):                                                        # twice: the counters must re-arm
        dX, dW_, dOUT, dTGT, dOUT2, dM, dXM = dev.up(X), dev.up(W), dev.up(OUT), dev.up(TGT), dev.zeros((N, E0)), dev.up(M), dev.zeros((N, E1))
        dDW, dDB = dev.up(DW), dev.up(DB)
        t4k.call("t4k_loss_linear_bwd", p(dX), p(dW_), p(dOUT), p(dTGT), p(dOUT2), p(dX), p(dM) if mask else None, p(dXM) if mask else None,
                 p(dDW) if train else None, p(dDB) if train else None, N, E0, E1, train, None)
        assert np.array_equal(dev.down(dOUT), G) and np.array_equal(dev.down(dOUT2), G)
        small = E0 <= 64 and E1 <= 512
        if small: assert np.array_equal(dev.down(dX), DX)
        else:     assert relx(dev.down(dX), DX, D) < RTOL
        if mask: assert rel(dev.down(dXM), DX * M) < (1e-6 if small else RTOL)
        if train: assert relx(dev.down(dDW), DWr, D) < RTOL and relx(dev.down(dDB), DBr, D) < RTOL


@pytest.mark.parametrize("N,E1,EA,EB", [(128, 980, 100, 10), (64, 512, 64, 16), (37, 260, 52, 3), (256, 1024, 128, 10), (160, 256, 64, 10), (96, 132, 200, 7)])
def test_head_backward_and_the_linear_layer_in_front_in_one_launch(t4k, dev, oracle, N, E1, EA, EB):
    """t4k_mlp_head_bwd == t4k_loss_linear_bwd (head: out -= target, dW2 | dB2, dX2 in place, mask multiply -> dY1) followed by t4k_linear_bwd
    (dW1 | dB1, dX1 in place) of the oracle: the GEMM tiles recompute their rows of dY1 instead of waiting for the head, so every tensor both
    kernels write is compared (1e-4 relative; `out - target` and its copy bit-exact), twice in a row (gate counter and epoch slots re-arm),
    gradients ACCUMULATE onto what the tensors held."""
    D = max(N, EA, EB)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    if t4k.lib.t4k_mlp_head_bwd_ok(N, E1, EA, EB) != 1:
        pytest.skip("shape does not qualify on this device")
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N + E1 + EA)
    X1 = rng.standard_normal((N, E1)).astype(np.float32); W1 = (rng.standard_normal((EA, E1)) * 0.1).astype(np.float32)
    X2 = rng.standard_normal((N, EA)).astype(np.float32); W2 = (rng.standard_normal((EB, EA)) * 0.3).astype(np.float32)
    Pr = rng.random((N, EB)).astype(np.float32); T = (rng.random((N, EB)) > 0.9).astype(np.float32)
    M = ((rng.random((N, EA)) > 0.5) * 1.0).astype(np.float32)
    DW1 = rng.standard_normal((EA, E1)).astype(np.float32); DB1 = rng.standard_normal(EA).astype(np.float32)
    DW2 = rng.standard_normal((EB, EA)).astype(np.float32); DB2 = rng.standard_normal(EB).astype(np.float32)
    G2 = Pr - T
    DX2 = np.zeros_like(X2); DW2r, DB2r = DW2.copy(), DB2.copy()
    assert o.t4o_linear_bwd(P(X2), P(W2), P(G2), P(DX2), P(DW2r), P(DB2r), N, EB, EA, 1) == 0
    G1 = (DX2 * M).astype(np.float32)
    DX1 = np.zeros_like(X1); DW1r, DB1r = DW1.copy(), DB1.copy()
    assert o.t4o_linear_bwd(P(X1), P(W1), P(np.ascontiguousarray(G1)), P(DX1), P(DW1r), P(DB1r), N, EA, E1, 1) == 0
    for rep_ in range(2):
        d = {k: dev.up(v) for k, v in dict(X1=X1, W1=W1, X2=X2, W2=W2, P=Pr, T=T, M=M, DW1=DW1, DB1=DB1, DW2=DW2, DB2=DB2).items()}
        d["Y1"] = dev.zeros((N, EA)); d["Y2"] = dev.zeros((N, EB))
        t4k.call("t4k_mlp_head_bwd", p(d["X2"]), p(d["W2"]), p(d["P"]), p(d["T"]), p(d["Y2"]), p(d["M"]), p(d["Y1"]), p(d["DW2"]), p(d["DB2"]),
                 p(d["X1"]), p(d["W1"]), p(d["DW1"]), p(d["DB1"]), N, E1, EA, EB, None)
        assert t4k.lib.t4k_sync(None) == 0
        assert np.array_equal(dev.down(d["P"]), G2) and np.array_equal(dev.down(d["Y2"]), G2), "rep %d: out -= target" % rep_
        assert np.array_equal(dev.down(d["X2"]), DX2), "rep %d: dX2 (fmaf chain in the oracle's order)" % rep_
        assert rel(dev.down(d["Y1"]), G1) < 1e-6, "rep %d: dY1" % rep_
        assert relx(dev.down(d["DW2"]), DW2r, D) < RTOL and relx(dev.down(d["DB2"]), DB2r, D) < RTOL, "rep %d: head gradients" % rep_
        assert relx(dev.down(d["DW1"]), DW1r, D) < RTOL, "rep %d: dW1 %.3g" % (rep_, rel(dev.down(d["DW1"]), DW1r))
        assert relx(dev.down(d["DB1"]), DB1r, D) < RTOL, "rep %d: dB1 %.3g" % (rep_, rel(dev.down(d["DB1"]), DB1r))
        assert relx(dev.down(d["X1"]), DX1, D) < RTOL, "rep %d: dX1 (in place) %.3g" % (rep_, rel(dev.down(d["X1"]), DX1))


@pytest.mark.parametrize("N,E1,EA,EB,run1,train", [(256, 512, 256, 1, True, 1), (256, 512, 256, 1, True, 0), (256, 784, 512 // 2, 1, False, 1), (64, 128, 96, 4, True, 1)])
def test_head_backward_with_runs_and_the_linear_layer_in_front_in_one_launch(t4k, dev, oracle, N, E1, EA, EB, run1, train):
    """t4k_mlp_block_bwd: the GAN discriminator's tail - linear, [leakyrelu, dropout], linear, (sigmoid) - differentiated in one launch: head
    (out -= target, dW2 | dB2, dX2 in place), the run's two mask multiplies (both intermediate tensors stored), the big layer's dW1 | dB1 and
    dX1 in place, and the mask multiplies of the run in front of THAT layer in its dX epilogue; frozen variant (train = 0: dX only).  Against the
    oracle's linear backward + numpy mask products, 1e-4 relative, twice in a row."""
    D = max(N, EA, EB)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    if t4k.lib.t4k_mlp_head_bwd_ok(N, E1, EA, EB) != 1:
        pytest.skip("shape does not qualify on this device")
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N + E1 + EA + train)
    X1 = rng.standard_normal((N, E1)).astype(np.float32); W1 = (rng.standard_normal((EA, E1)) * 0.1).astype(np.float32)
    X2 = rng.standard_normal((N, EA)).astype(np.float32); W2 = (rng.standard_normal((EB, EA)) * 0.3).astype(np.float32)
    Pr = rng.random((N, EB)).astype(np.float32); T = (rng.random((N, EB)) > 0.5).astype(np.float32)
    Mdrop = ((rng.random((N, EA)) > 0.4) * 1.0).astype(np.float32); Mleak = np.where(rng.random((N, EA)) > 0.5, 1.0, 0.2).astype(np.float32)
    M1d = ((rng.random((N, E1)) > 0.4) * 1.0).astype(np.float32); M1l = np.where(rng.random((N, E1)) > 0.5, 1.0, 0.2).astype(np.float32)
    DW1 = rng.standard_normal((EA, E1)).astype(np.float32); DB1 = rng.standard_normal(EA).astype(np.float32)
    DW2 = rng.standard_normal((EB, EA)).astype(np.float32); DB2 = rng.standard_normal(EB).astype(np.float32)
    G2 = Pr - T
    DX2 = np.zeros_like(X2); DW2r, DB2r = DW2.copy(), DB2.copy()
    assert o.t4o_linear_bwd(P(X2), P(W2), P(G2), P(DX2), P(DW2r), P(DB2r), N, EB, EA, train) == 0
    D1 = (DX2 * Mdrop).astype(np.float32); D2 = (D1 * Mleak).astype(np.float32)          # dropout is the run's second layer: its mask comes first on the way back
    DX1 = np.zeros_like(X1); DW1r, DB1r = DW1.copy(), DB1.copy()
    assert o.t4o_linear_bwd(P(X1), P(W1), P(np.ascontiguousarray(D2)), P(DX1), P(DW1r), P(DB1r), N, EA, E1, train) == 0
    E1d = (DX1 * M1d).astype(np.float32); E2d = (E1d * M1l).astype(np.float32)
    for rep_ in range(2):
        d = {k: dev.up(v) for k, v in dict(X1=X1, W1=W1, X2=X2, W2=W2, P=Pr, T=T, Mdrop=Mdrop, Mleak=Mleak, M1d=M1d, M1l=M1l, DW1=DW1, DB1=DB1, DW2=DW2, DB2=DB2).items()}
        for k_, shp in (("Y2", (N, EB)), ("R2pre", (N, EA)), ("R2in", (N, EA)), ("R1pre", (N, E1)), ("R1in", (N, E1))):
            d[k_] = dev.zeros(shp)
        b2 = PoolBlock(); b2.KS = 1
        b2.pre_layer, b2.pre_alpha, b2.pre_mask, b2.pre_out = oracle.L_LEAKYRL, 0.2, p(d["Mleak"]), p(d["R2pre"])
        b2.post_layer, b2.post_alpha, b2.post_mask, b2.post_out = oracle.L_DROPOUT, 0.4, p(d["Mdrop"]), p(d["X2"])
        b1 = PoolBlock(); b1.KS = 1
        b1.pre_layer, b1.pre_alpha, b1.pre_mask, b1.pre_out = oracle.L_LEAKYRL, 0.2, p(d["M1l"]), p(d["R1pre"])
        b1.post_layer, b1.post_alpha, b1.post_mask, b1.post_out = oracle.L_DROPOUT, 0.4, p(d["M1d"]), p(d["X1"])
        t4k.call("t4k_mlp_block_bwd", p(d["X2"]), p(d["W2"]), p(d["P"]), p(d["T"]), p(d["Y2"]), ctypes.byref(b2), p(d["R2in"]),
                 p(d["DW2"]) if train else None, p(d["DB2"]) if train else None, p(d["X1"]), p(d["W1"]), ctypes.byref(b1) if run1 else None, p(d["R1in"]) if run1 else None,
                 p(d["DW1"]) if train else None, p(d["DB1"]) if train else None, N, E1, EA, EB, train, None)
        assert t4k.lib.t4k_sync(None) == 0
        assert np.array_equal(dev.down(d["P"]), G2) and np.array_equal(dev.down(d["Y2"]), G2), "rep %d: out -= target" % rep_
        assert np.array_equal(dev.down(d["X2"]), DX2), "rep %d: dX2" % rep_
        assert rel(dev.down(d["R2pre"]), D1) < 1e-6 and rel(dev.down(d["R2in"]), D2) < 1e-6, "rep %d: the run's two products" % rep_
        assert relx(dev.down(d["X1"]), DX1, D) < RTOL, "rep %d: dX1 %.3g" % (rep_, rel(dev.down(d["X1"]), DX1))
        if run1:
            assert relx(dev.down(d["R1pre"]), E1d, D) < RTOL and relx(dev.down(d["R1in"]), E2d, D) < RTOL, "rep %d: mask chain behind dX1" % rep_
        if train:
            assert relx(dev.down(d["DW2"]), DW2r, D) < RTOL and relx(dev.down(d["DB2"]), DB2r, D) < RTOL, "rep %d: head gradients" % rep_
            assert relx(dev.down(d["DW1"]), DW1r, D) < RTOL and relx(dev.down(d["DB1"]), DB1r, D) < RTOL, "rep %d: dW1 / dB1" % rep_
        else:
            assert np.array_equal(dev.down(d["DW1"]), DW1) and np.array_equal(dev.down(d["DW2"]), DW2), "rep %d: a frozen net's gradients were touched" % rep_


def test_plu_and_second_destination_entries(t4k, dev, oracle):
    """t4k_plu (packed L\\U + pivots + permutation applied to I), t4k_tt_op2 (second destination) and t4k_conv2d_fwd2 (layer-0 copy)."""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(4)
    for K in (2, 5, 33):
        a0 = (rng.standard_normal((K, K)) + np.eye(K) * 0.5).astype(np.float32)
        a, I = a0.copy(), np.eye(K, dtype=np.float32); piv = np.zeros(K, np.int32); st = ctypes.c_int(0)
        o.t4o_plu(P(a), P(I), P(piv), K, ctypes.byref(st))
        dA, dI, dpiv, dst = dev.up(a0), dev.up(np.eye(K, dtype=np.float32)), dev.zeros(K, dev.torch.int32), dev.zeros(1, dev.torch.int32)
        t4k.call("t4k_plu", p(dA), p(dI), p(dpiv), K, p(dst), None)
        assert rel(dev.down(dA), a) < 1e-5 and np.array_equal(dev.down(dI), I)
        assert np.array_equal(dev.down(dpiv), piv) and dev.down(dst)[0] == st.value == 0
    A = rng.standard_normal(1000).astype(np.float32); B = rng.standard_normal(1000).astype(np.float32)
    dO, dO2 = dev.zeros(1000), dev.zeros(1000)
    t4k.call("t4k_tt_op2", oracle.SUB, p(dev.up(A)), p(dev.up(B)), p(dO), p(dO2), 1000, None)
    assert np.array_equal(dev.down(dO), A - B) and np.array_equal(dev.down(dO2), A - B)
    for (N, H, C1, C0) in ((4, 12, 1, 10), (2, 8, 16, 8), (3, 10, 3, 64), (2, 9, 4, 64)):   # direct image-input kernel / gather-MFMA kernel (+ copy launch) / thin-input MFMA kernel (copy from its registers)
        X = rng.standard_normal((N, H, H, C1)).astype(np.float32); F = rng.standard_normal((C1, 3, 3, C0)).astype(np.float32)
        Bv = rng.standard_normal(C0).astype(np.float32); Y = np.zeros((N, H, H, C0), np.float32)
        o.t4o_conv2d_fwd(P(X), P(Y), P(F), P(Bv), N, H, H, C1, H, H, C0, 3, 1, 1)
        dXC, dY = dev.zeros(X.shape), dev.zeros(Y.shape)
        t4k.call("t4k_conv2d_fwd2", p(dev.up(X)), p(dXC), p(dY), p(dev.up(F)), p(dev.up(Bv)), N, H, H, C1, H, H, C0, 3, 1, 1, None)
        assert relx(dev.down(dY), Y, 9 * C1) < RTOL and np.array_equal(dev.down(dXC), X)


@pytest.mark.parametrize("N,E0,E1,layer", [(128, 100, 980, "dropout"), (128, 100, 980, "relu"), (64, 16, 40, "dropout"), (32, 256, 64, "tanh"),
                                           (256, 128, 1024, "dropout")])
def test_linear_with_activation_epilogue(t4k, dev, oracle, N, E0, E1, layer):
    """t4k_linear_act_fwd == linear forward + the element-wise layer behind it (mask and output), whichever kernel takes the
    shape (small head, split-K GEMM with the activation in the fold, plain GEMM + separate launch); dropout draws the slice
    t4k_rand would have drawn."""
    D = E1                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    LAY = {"dropout": (oracle.L_DROPOUT, 0.5), "relu": (oracle.L_RELU, 0.0), "tanh": (oracle.L_TANH, 0.0)}
    L, alpha = LAY[layer]
    rng = np.random.default_rng(E0 + E1)
    X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) * 0.1).astype(np.float32)
    b = rng.standard_normal(E0).astype(np.float32)
    Y = np.zeros((N, E0), np.float32); o.t4o_linear_fwd(P(X), P(W), P(b), P(Y), N, E0, E1)
    seed, off = 5, 1 << 20
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    f = np.zeros(N * E0, np.float32); a = np.zeros((N, E0), np.float32)
    if layer == "dropout": o.t4o_rand(P(f), N * E0, 0, 0.0, 1.0)
    o.t4o_activate(L, P(Y), P(a), P(f), alpha, N * E0)
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
    dY, dF, dA = dev.zeros((N, E0)), dev.zeros(N * E0), dev.zeros((N, E0))
    t4k.call("t4k_linear_act_fwd", p(dev.up(X)), p(dev.up(W)), p(dev.up(b)), p(dY), L, alpha, p(dF), p(dA), N, E0, E1, None)
    assert relx(dev.down(dY), Y, D) < RTOL and relx(dev.down(dA), a, D) < RTOL
    if layer == "dropout":
        assert np.array_equal(dev.down(dF), f) and t4k.lib.t4k_rand_offset() == o.t4o_rand_offset()


@pytest.mark.parametrize("N,E1,H,E2,layer,softmax", [(128, 980, 100, 10, "dropout", True), (128, 980, 100, 10, "relu", True), (64, 2048, 64, 16, "dropout", False),
                                                      (32, 40, 16, 4, "relu", True), (128, 256, 512, 10, "dropout", True), (7, 1000, 30, 3, "tanh", True)])
def test_mlp_head_forward(t4k, dev, oracle, N, E1, H, E2, layer, softmax):
    """t4k_mlp_head_fwd == [linear + element-wise layer] + [linear (+ softmax)] layer by layer: every tensor (Y1, mask, A1, Y2, P2), the
    dropout mask bit-exact and the Philox stream advanced identically - whether the second launch folds the first GEMM's split-K
    slabs (980 -> 100 -> 10), the first layer is itself head-sized, or the shapes fall back to the separate entries."""
    D = max(E1, H)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    LAY = {"dropout": (oracle.L_DROPOUT, 0.5), "relu": (oracle.L_RELU, 0.0), "tanh": (oracle.L_TANH, 0.0)}
    L, alpha = LAY[layer]
    rng = np.random.default_rng(E1 + H)
    X = rng.standard_normal((N, E1)).astype(np.float32)
    W1 = (rng.standard_normal((H, E1)) * 0.05).astype(np.float32); b1 = rng.standard_normal(H).astype(np.float32)
    W2 = (rng.standard_normal((E2, H)) * 0.2).astype(np.float32); b2 = rng.standard_normal(E2).astype(np.float32)
    Y1 = np.zeros((N, H), np.float32); o.t4o_linear_fwd(P(X), P(W1), P(b1), P(Y1), N, H, E1)
    seed, off = 3, 1 << 22
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    f = np.zeros(N * H, np.float32); A1 = np.zeros((N, H), np.float32)
    if layer == "dropout": o.t4o_rand(P(f), N * H, 0, 0.0, 1.0)
    o.t4o_activate(L, P(Y1), P(A1), P(f), alpha, N * H)
    Y2 = np.zeros((N, E2), np.float32); o.t4o_linear_fwd(P(A1), P(W2), P(b2), P(Y2), N, E2, H)
    P2 = np.zeros_like(Y2); o.t4o_softmax(P(Y2), P(P2), N, E2)
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
    dY1, dF, dA1, dY2, dP2 = dev.zeros((N, H)), dev.zeros(N * H), dev.zeros((N, H)), dev.zeros((N, E2)), dev.zeros((N, E2))
    for rep_ in range(2):                                                          # second call: same stream position again
        t4k.call("t4k_rand_set_offset", off)
        t4k.call("t4k_mlp_head_fwd", p(dev.up(X)), p(dev.up(W1)), p(dev.up(b1)), p(dY1), L, alpha, p(dF), p(dA1),
                 p(dev.up(W2)), p(dev.up(b2)), p(dY2), p(dP2) if softmax else None, N, H, E1, E2, None)
        assert relx(dev.down(dY1), Y1, D) < RTOL and relx(dev.down(dA1), A1, D) < RTOL and relx(dev.down(dY2), Y2, D) < RTOL
        if softmax: assert relx(dev.down(dP2), P2, D) < RTOL
        if layer == "dropout":
            assert np.array_equal(dev.down(dF), f) and t4k.lib.t4k_rand_offset() == o.t4o_rand_offset()


@pytest.mark.parametrize("N,E0,E1", [(128, 10, 100), (256, 512, 784), (256, 256, 512), (64, 100, 980), (33, 70, 45), (256, 784, 512)])
def test_linear_backward_with_mask_multiply(t4k, dev, oracle, N, E0, E1):
    """t4k_linear_bwd2: dX (in place over X), dW, dB as t4k_linear_bwd, plus DXM = dX (*) MASK (the element-wise layer in front) -
    from the small-head kernel, from the dual GEMM launch's dX epilogue, or as a separate launch, depending on the shape."""
    D = max(E1, E0, N)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N + E0 * 3 + E1)
    X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) / np.sqrt(E0)).astype(np.float32)
    G = rng.standard_normal((N, E0)).astype(np.float32); M = (rng.random((N, E1)) > 0.4).astype(np.float32) * 1.5
    DW = rng.standard_normal((E0, E1)).astype(np.float32); DB = rng.standard_normal(E0).astype(np.float32); DX = np.zeros_like(X)
    dDW, dDB = dev.up(DW), dev.up(DB)
    o.t4o_linear_bwd(P(X), P(W), P(G), P(DX), P(DW), P(DB), N, E0, E1, 1)
    for rep_ in range(2):
        dX, dXM = dev.up(X), dev.zeros((N, E1))
        if rep_ == 1: o.t4o_linear_bwd(P(X), P(W), P(G), P(DX), P(DW), P(DB), N, E0, E1, 1)     # accumulate dW / dB once more
        t4k.call("t4k_linear_bwd2", p(dX), p(dev.up(W)), p(dev.up(G)), p(dX), p(dev.up(M)), p(dXM), p(dDW), p(dDB), N, E0, E1, 1, None)
        assert relx(dev.down(dX), DX, D) < RTOL and relx(dev.down(dXM), DX * M, D) < RTOL
        assert relx(dev.down(dDW), DW, D) < RTOL and relx(dev.down(dDB), DB, D) < RTOL


def test_linear_random_shapes(t4k, dev, oracle):
    """Seeded sweep of linear forward / in-place backward over every GEMM regime: unaligned (no 16-byte loads), head-sized,
    split-K, dual dW|dX launch, interior LDS-DMA tiles, 128x128 tiles."""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(99)
    shapes = [(5, 3, 7), (17, 33, 45), (64, 64, 64), (128, 128, 256), (100, 36, 1000), (30, 130, 70), (256, 256, 512), (48, 20, 2048),
              (9, 64, 513), (512, 1024, 1024), (1, 10, 100), (200, 7, 19), (96, 72, 516), (64, 1000, 128)]
    for (N, E0, E1) in shapes:
        X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) / np.sqrt(E1)).astype(np.float32)
        b = rng.standard_normal(E0).astype(np.float32)
        Y = np.zeros((N, E0), np.float32); o.t4o_linear_fwd(P(X), P(W), P(b), P(Y), N, E0, E1)
        dX, dW, db, dY = dev.up(X), dev.up(W), dev.up(b), dev.zeros((N, E0))
        t4k.call("t4k_linear_fwd", p(dX), p(dW), p(db), p(dY), N, E0, E1, None)
        tag = "N=%d E0=%d E1=%d" % (N, E0, E1)
        assert relx(dev.down(dY), Y, max(E1, E0, N)) < RTOL, tag
        G = rng.standard_normal((N, E0)).astype(np.float32)
        DW = rng.standard_normal((E0, E1)).astype(np.float32); DB = rng.standard_normal(E0).astype(np.float32); DX = np.zeros_like(X)
        dDW, dDB = dev.up(DW), dev.up(DB)
        o.t4o_linear_bwd(P(X), P(W), P(G), P(DX), P(DW), P(DB), N, E0, E1, 1)
        dX2, dXk = dev.zeros((N, E1)), dev.up(X)
        DW0 = rng.standard_normal((E0, E1)).astype(np.float32)      # dX to its own buffer first (no arrival gate in the dual launches), fresh accumulators
        DWb, DBb, DXb = DW0.copy(), np.zeros(E0, np.float32), np.zeros_like(X)
        o.t4o_linear_bwd(P(X), P(W), P(G), P(DXb), P(DWb), P(DBb), N, E0, E1, 1)
        dDWb, dDBb = dev.up(DW0), dev.zeros(E0)
        t4k.call("t4k_linear_bwd", p(dXk), p(dW), p(dev.up(G)), p(dX2), p(dDWb), p(dDBb), N, E0, E1, 1, None)
        assert relx(dev.down(dX2), DXb, max(E1, E0, N)) < RTOL and relx(dev.down(dDWb), DWb, max(E1, E0, N)) < RTOL and relx(dev.down(dDBb), DBb, max(E1, E0, N)) < RTOL, tag + " (dX apart)"
        assert np.array_equal(dev.down(dXk), X), tag + " (X untouched)"
        t4k.call("t4k_linear_bwd", p(dX), p(dW), p(dev.up(G)), p(dX), p(dDW), p(dDB), N, E0, E1, 1, None)      # dX over X
        assert relx(dev.down(dX), DX, max(E1, E0, N)) < RTOL and relx(dev.down(dDW), DW, max(E1, E0, N)) < RTOL and relx(dev.down(dDB), DB, max(E1, E0, N)) < RTOL, tag


def test_poolblock_non_square_grids(t4k, dev, oracle):
    """Fused element-wise runs on non-square grids (H != W), 2x2 and 3x3 pooling, every vector width (C % 4, % 2, odd): forward
    tensors and the in-place backward vs the oracle's separate layers."""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(77)
    for case, (KS, C, pool) in enumerate([(2, 8, "max"), (2, 6, "avg"), (2, 5, "min"), (3, 4, "max"), (3, 7, "avg"), (2, 20, "max")]):
        N = int(rng.integers(1, 5)); H0 = int(rng.integers(2, 6)); W0 = H0 + int(rng.integers(1, 5)); H1, W1 = H0 * KS, W0 * KS
        L = {"max": oracle.L_MAXPOOL, "avg": oracle.L_AVGPOOL, "min": oracle.L_MINPOOL}[pool]
        n1, n0 = N * H1 * W1 * C, N * H0 * W0 * C
        X = rng.standard_normal((N, H1, W1, C)).astype(np.float32); DY = rng.standard_normal((N, H0, W0, C)).astype(np.float32)
        f1 = np.zeros(n1, np.float32); y1 = np.zeros_like(X); o.t4o_activate(oracle.L_RELU, P(X), P(y1), P(f1), 0.0, n1)
        q = np.zeros((N, H0, W0, C), np.float32); o.t4o_pool(L, P(y1), P(q), N, H1, W1, H0, W0, C, KS)
        f0 = np.zeros(n0, np.float32); r = np.zeros_like(q); o.t4o_activate(oracle.L_LEAKYRL, P(q), P(r), P(f0), 0.1, n0)
        dX, d1, dm1, dq, dm0, dr = dev.up(X), dev.zeros(X.shape), dev.zeros(n1), dev.zeros(q.shape), dev.zeros(n0), dev.zeros(q.shape)
        blk = PoolBlock(); blk.KS = KS; blk.pre_layer = oracle.L_RELU; blk.pre_mask = p(dm1); blk.pre_out = p(d1)
        blk.pool_layer = L; blk.pool_out = p(dq); blk.post_layer = oracle.L_LEAKYRL; blk.post_alpha = 0.1; blk.post_mask = p(dm0); blk.post_out = p(dr)
        t4k.call("t4k_poolblock_fwd", p(dX), ctypes.byref(blk), N, H1, W1, H0, W0, C, None)
        tag = "case %d" % case
        assert rel(dev.down(d1), y1) < 1e-6 and rel(dev.down(dq), q) < 1e-6 and rel(dev.down(dr), r) < 1e-6, tag
        assert np.array_equal(dev.down(dm1), f1) and np.array_equal(dev.down(dm0), f0), tag
        # backward, layer by layer in the oracle (each stage's input buffer receives its dX)
        t = np.zeros(n0, np.float32); o.t4o_tt_op(oracle.MUL, P(DY), P(f0), P(t), n0); qb = t.reshape(q.shape).copy()
        y1b = y1.copy(); o.t4o_dpool(L, P(y1b), P(qb), N, H1, W1, H0, W0, C, KS)
        t1 = np.zeros(n1, np.float32); o.t4o_tt_op(oracle.MUL, P(y1b), P(f1), P(t1), n1)
        t4k.call("t4k_poolblock_bwd", p(dev.up(DY)), p(dX), ctypes.byref(blk), N, H1, W1, H0, W0, C, None)
        assert rel(dev.down(dX), t1.reshape(X.shape)) < 1e-6 and rel(dev.down(d1), y1b) < 1e-6 and rel(dev.down(dq), qb) < 1e-6, tag


def test_conv_random_shapes_non_square(t4k, dev, oracle):
    """Seeded sweep over non-square grids, odd batches and channel counts on every kernel family (direct image-input kernels,
    gather-MFMA, LDS-staged many-channel tiling): forward (+ the fused pool block where the grid is even) and backward vs the oracle."""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(2024)
    combos = [(1, 10), (3, 16), (3, 64), (4, 7), (5, 9), (10, 20), (12, 33), (20, 10), (32, 16), (64, 24), (64, 64), (96, 20)]
    for case in range(24):
        C1, C0 = combos[case % len(combos)]
        K = (3, 5, 3, 1)[case % 4]; Pd = K // 2
        N = int(rng.integers(1, 6)); H = int(rng.integers(2, 8)) * 2; W = int(rng.integers(2, 9)) * 2 + (2 if case % 3 == 0 else 0)
        X = rng.standard_normal((N, H, W, C1)).astype(np.float32); F = (rng.standard_normal((C1, K, K, C0)) * 0.2).astype(np.float32)
        B = rng.standard_normal(C0).astype(np.float32)
        Y = np.zeros((N, H, W, C0), np.float32); o.t4o_conv2d_fwd(P(X), P(Y), P(F), P(B), N, H, W, C1, H, W, C0, K, 1, Pd)
        tag = "case %d: N=%d %dx%d %d->%d K=%d" % (case, N, H, W, C1, C0, K)
        dX, dF, dB, dY = dev.up(X), dev.up(F), dev.up(B), dev.zeros(Y.shape)
        t4k.call("t4k_conv2d_fwd", p(dX), p(dY), p(dF), p(dB), N, H, W, C1, H, W, C0, K, 1, Pd, None)
        assert relx(dev.down(dY), Y, max(K * K * max(C1, C0), N * H * W)) < RTOL, tag
        if K in (3, 5):                                               # fused block: maxpool + relu behind the conv
            q = np.zeros((N, H // 2, W // 2, C0), np.float32); o.t4o_pool(oracle.L_MAXPOOL, P(Y), P(q), N, H, W, H // 2, W // 2, C0, 2)
            f = np.zeros(q.size, np.float32); r = np.zeros_like(q); o.t4o_activate(oracle.L_RELU, P(q), P(r), P(f), 0.0, q.size)
            dq, dm, dr, dY2 = dev.zeros(q.shape), dev.zeros(q.size), dev.zeros(q.shape), dev.zeros(Y.shape)
            blk = PoolBlock(); blk.KS = 2; blk.pool_layer = oracle.L_MAXPOOL; blk.pool_out = p(dq)
            blk.post_layer = oracle.L_RELU; blk.post_mask = p(dm); blk.post_out = p(dr)
            t4k.call("t4k_conv2d_block_fwd", p(dX), None, p(dY2), p(dF), p(dB), ctypes.byref(blk), N, H, W, C1, H, W, C0, K, 1, Pd, None)
            assert relx(dev.down(dY2), Y, max(K * K * max(C1, C0), N * H * W)) < RTOL and relx(dev.down(dq), q, max(K * K * max(C1, C0), N * H * W)) < RTOL and relx(dev.down(dr), r, max(K * K * max(C1, C0), N * H * W)) < RTOL, tag
        G = rng.standard_normal(Y.shape).astype(np.float32)
        DX = np.zeros_like(X); DF = np.zeros_like(F); DB = np.zeros_like(B)
        o.t4o_conv2d_bwd(P(X), P(G), P(DX), P(F), P(DF), P(DB), N, H, W, C1, H, W, C0, K, 1, Pd, 1)
        dDX, dDX2, dDF, dDB = dev.zeros(X.shape), dev.zeros(X.shape), dev.zeros(F.shape), dev.zeros(B.shape)
        t4k.call("t4k_conv2d_bwd2", p(dX), p(dev.up(G)), p(dDX), p(dDX2), p(dF), p(dDF), p(dDB), N, H, W, C1, H, W, C0, K, 1, Pd, 1, None)
        assert relx(dev.down(dDX), DX, max(K * K * max(C1, C0), N * H * W)) < RTOL and np.array_equal(dev.down(dDX2), dev.down(dDX)), tag
        assert relx(dev.down(dDF), DF, max(K * K * max(C1, C0), N * H * W)) < RTOL and relx(dev.down(dDB), DB, max(K * K * max(C1, C0), N * H * W)) < RTOL, tag


# ----------------------------------------------------------------------------- error behaviour (reference: print-and-continue, never abort)
def test_error_paths_return_status_and_reference_messages(t4k, dev):
    """Unsupported geometry / bad arguments come back as negative status codes with the reference's own message text
    (forward.cu:149-151, backprop.cu:181-183, model.cpp:262) in t4k_last_error(); nothing throws or aborts."""
    lib = t4k.lib
    ARG, UNSUP = -1, -4                                  # T4K_ERR_ARG, T4K_ERR_UNSUPPORTED (include/t4k.h)
    x = dev.zeros((2, 8, 8, 3)); y = dev.zeros((2, 8, 8, 4)); f = dev.zeros((3, 2, 2, 4)); b = dev.zeros(4)
    rc = lib.t4k_conv2d_fwd(p(x), p(y), p(f), p(b), 2, 8, 8, 3, 8, 8, 4, 2, 1, 0, None)
    assert rc == UNSUP and b"nn#fconv kernel_size=2 stride=1 padding=0 not supported" in lib.t4k_last_error()
    rc = lib.t4k_conv2d_bwd(p(x), p(y), p(x), p(f), p(f), p(b), 2, 8, 8, 3, 8, 8, 4, 3, 2, 1, 1, None)
    assert rc == UNSUP and b"nn#bconv kernel_size=3 stride=2 padding=1 not supported" in lib.t4k_last_error()
    assert lib.t4k_pool(14, p(x), p(y), 2, 8, 8, 2, 2, 3, 4, None) == UNSUP and b"kernel_size=4" in lib.t4k_last_error()
    assert lib.t4k_gemm(None, p(x), p(y), 1.0, 0.0, 0, 0, 4, 4, 4, 1, None) == ARG             # T4K_ERR_ARG
    assert lib.t4k_math(99, p(x), 0.0, 10, None) == UNSUP                                         # unknown math_op
    assert lib.t4k_linear_bwd(p(x), p(f), p(y), p(x), p(f), None, 2, 4, 3, 1, None) == ARG     # dW without dB
    assert lib.t4k_allreduce_sum(p(x), 16, None) == UNSUP or lib.t4k_comm_world() > 0            # no communicator attached
    # the library is still healthy afterwards
    t4k.call("t4k_math", 12, p(x), 2.0, x.numel(), None)                                       # FILL
    assert float(dev.down(x).sum()) == 2.0 * x.numel()


def test_conv2d_many_channels_full_size_spot_checks(t4k, dev):
    """CIFAR-class layer (N=64, 32x32, 64 -> 128 channels: the LDS-staged MFMA kernels) checked against float64 numpy on
    randomly chosen output elements of forward, dX (reference's flipped-filter scatter, nmath.tcu:304-324) and dF / dB -
    the oracle's scalar loops would take minutes at this size."""
    rng = np.random.default_rng(2024)
    N, H, C1, C0, K, Pd = 64, 32, 64, 128, 3, 1
    I = rng.standard_normal((N, H, H, C1)).astype(np.float32)
    F = (rng.standard_normal((C1, K, K, C0)) * 0.05).astype(np.float32)
    B = rng.standard_normal(C0).astype(np.float32)
    G = rng.standard_normal((N, H, H, C0)).astype(np.float32)
    dI, dF_, dB_, dG = dev.up(I), dev.up(F), dev.up(B), dev.up(G)
    dO, dDX = dev.zeros((N, H, H, C0)), dev.zeros((N, H, H, C1))
    dDF, dDB = dev.zeros((C1, K, K, C0)), dev.zeros(C0)
    t4k.call("t4k_conv2d_fwd", p(dI), p(dO), p(dF_), p(dB_), N, H, H, C1, H, H, C0, K, 1, Pd, None)
    t4k.call("t4k_conv2d_bwd", p(dI), p(dG), p(dDX), p(dF_), p(dDF), p(dDB), N, H, H, C1, H, H, C0, K, 1, Pd, 1, None)
    O, DX, DF, DB = dev.down(dO), dev.down(dDX), dev.down(dDF), dev.down(dDB)
    Ip = np.pad(I.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    Gp = np.pad(G.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    F64 = F.astype(np.float64)
    for _ in range(48):
        n, i, j = rng.integers(0, N), rng.integers(0, H), rng.integers(0, H)
        co, ci = rng.integers(0, C0), rng.integers(0, C1)
        # forward: O[n,i,j,co] = B[co] + sum I[n,i+ky-1,j+kx-1,:] . F[:,ky,kx,co]
        want = B[co] + sum(Ip[n, i + ky, j + kx, :] @ F64[:, ky, kx, co] for ky in range(K) for kx in range(K))
        assert abs(O[n, i, j, co] - want) <= 1e-4 * max(1.0, abs(want))
        # dX[n,y,x,c1] = sum dO[n, y+1-ky, x+1-kx, :] . F[c1, 2-ky, 2-kx, :]   (padded index y+1-ky+1 = y+2-ky)
        want = sum(Gp[n, i + 2 - ky, j + 2 - kx, :] @ F64[ci, K - 1 - ky, K - 1 - kx, :] for ky in range(K) for kx in range(K))
        assert abs(DX[n, i, j, ci] - want) <= 1e-4 * max(1.0, abs(want))
    for _ in range(12):
        ci, co, ky, kx = rng.integers(0, C1), rng.integers(0, C0), rng.integers(0, K), rng.integers(0, K)
        want = float(np.sum(Ip[:, ky:ky + H, kx:kx + H, ci] * G[:, :, :, co].astype(np.float64)))
        assert abs(DF[ci, ky, kx, co] - want) <= 2e-4 * max(1.0, abs(want))            # 65536-term fp32 accumulation
    np.testing.assert_allclose(DB, G.astype(np.float64).sum(axis=(0, 1, 2)), rtol=2e-4, atol=2e-3)


@pytest.mark.parametrize("N,H1,C1,C0", [(6, 4, 12, 8), (2, 7, 3, 4), (4, 8, 64, 32), (3, 16, 8, 1), (2, 5, 32, 64)])
def test_transposed_conv_layer(t4k, dev, oracle, N, H1, C1, C0):
    """t4k_dconv2d_fwd / _bwd (word `dconv2d`: K=4, S=2, P=1, output padding for odd grids) against the oracle's direct-loop definition
    (itself pinned to torch ConvTranspose2d in test_oracle_vs_torch.py): few-channel, many-channel (LDS-staged MFMA) and image-output
    shapes; DX overwritten, DF / DB accumulated over two calls, the dX-only and dF-only forms."""
    o = oracle.lib(); P = oracle.P
    K, S, Pd = 4, 2, 1
    H0 = (H1 - 1) * S - 2 * Pd + K + (H1 + 2 * Pd - K) % S
    D = max(16 * max(C1, C0), N * H0 * H0)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    rng = np.random.default_rng(N * 100 + C0)
    I = rng.standard_normal((N, H1, H1, C1)).astype(np.float32); F = (rng.standard_normal((C1, K, K, C0)) * 0.2).astype(np.float32)
    B = rng.standard_normal(C0).astype(np.float32); G = rng.standard_normal((N, H0, H0, C0)).astype(np.float32)
    O = np.zeros((N, H0, H0, C0), np.float32)
    assert o.t4o_dconv2d_fwd(P(I), P(O), P(F), P(B), N, H1, H1, C1, H0, H0, C0, K, S, Pd) == 0
    dI, dF, dB, dO, dG = dev.up(I), dev.up(F), dev.up(B), dev.zeros(O.shape), dev.up(G)
    t4k.call("t4k_dconv2d_fwd", p(dI), p(dO), p(dF), p(dB), N, H1, H1, C1, H0, H0, C0, K, S, Pd, None)
    assert relx(dev.down(dO), O, D) < RTOL
    DX = np.zeros_like(I); DF = np.zeros_like(F); DB = np.zeros_like(B)
    dDX, dDF, dDB = dev.up(np.full_like(I, 3.0)), dev.zeros(F.shape), dev.zeros(B.shape)
    for rep in range(2):
        assert o.t4o_dconv2d_bwd(P(I), P(G), P(DX), P(F), P(DF), P(DB), N, H1, H1, C1, H0, H0, C0, K, S, Pd, 1) == 0
        t4k.call("t4k_dconv2d_bwd", p(dI), p(dG), p(dDX), p(dF), p(dDF), p(dDB), N, H1, H1, C1, H0, H0, C0, K, S, Pd, 1, None)
        assert relx(dev.down(dDX), DX, D) < RTOL and relx(dev.down(dDF), DF, D) < RTOL and relx(dev.down(dDB), DB, D) < RTOL
    dDX2 = dev.zeros(I.shape); t4k.call("t4k_dconv2d_bwd", p(dI), p(dG), p(dDX2), p(dF), None, None, N, H1, H1, C1, H0, H0, C0, K, S, Pd, 0, None)
    assert np.array_equal(dev.down(dDX2), dev.down(dDX))
    before = dev.down(dDF).copy(); t4k.call("t4k_dconv2d_bwd", p(dI), p(dG), None, p(dF), p(dDF), p(dDB), N, H1, H1, C1, H0, H0, C0, K, S, Pd, 0, None)
    assert np.array_equal(dev.down(dDF), before)                                    # train == 0: parameter gradients untouched
    assert t4k.lib.t4k_dconv2d_fwd(p(dI), p(dO), p(dF), p(dB), N, H1, H1, C1, H0 + 2, H0 + 2, C0, K, S, Pd, None) == -1   # inconsistent geometry is reported


@pytest.mark.parametrize("N,E0,E1", [(128, 100, 980), (128, 10, 100)])     # dW || dX dual launch with an arrival gate; small head with arrival counters
def test_gated_linear_backward_on_concurrent_streams(t4k, dev, oracle, N, E0, E1):
    """the one-launch producer / consumer kernels synchronise through counters in library memory.  Three streams run the
    in-place linear backward (dX lands in X's buffer) at the same time on different data: the library's default stream and a
    t4k_stream_create()d one have private counters, a stream the library does not know (torch's) must fall back to ungated launches."""
    D = max(E1, E0, N)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    torch = dev.torch
    o = oracle.lib(); P = oracle.P
    s_lib = ctypes.c_void_p(); t4k.call("t4k_stream_create", ctypes.byref(s_lib))
    s_ext = torch.cuda.Stream()
    streams = [None, s_lib, ctypes.c_void_p(s_ext.cuda_stream)]
    rng = np.random.default_rng(E1)
    W = (rng.standard_normal((E0, E1)) * 0.1).astype(np.float32); dW_ = dev.up(W)
    jobs = []
    for k, s in enumerate(streams):
        X = rng.standard_normal((N, E1)).astype(np.float32); DY = rng.standard_normal((N, E0)).astype(np.float32)
        DX = np.zeros_like(X); DW = np.zeros_like(W); DB = np.zeros(E0, np.float32)
        o.t4o_linear_bwd(P(X), P(W), P(DY), P(DX), P(DW), P(DB), N, E0, E1, 1)
        jobs.append(dict(s=s, X0=dev.up(X), X=dev.zeros(X.shape), DY=dev.up(DY), DW=dev.zeros(W.shape), DB=dev.zeros(E0), ref=(DX, DW, DB)))
    torch.cuda.synchronize()
    REPS = 30
    try:
        for it in range(REPS):
            for j in jobs:                                    # interleaved issue: the three streams overlap on the device
                t4k.call("t4k_copy", p(j["X0"]), p(j["X"]), N * E1, j["s"])
                if it == REPS - 1:
                    t4k.call("t4k_memset", p(j["DW"]), 0, 4 * E0 * E1, j["s"]); t4k.call("t4k_memset", p(j["DB"]), 0, 4 * E0, j["s"])
                t4k.call("t4k_linear_bwd", p(j["X"]), p(dW_), p(j["DY"]), p(j["X"]), p(j["DW"]), p(j["DB"]), N, E0, E1, 1, j["s"])
        for j in jobs:
            t4k.call("t4k_sync", j["s"])
        torch.cuda.synchronize()
        for k, j in enumerate(jobs):
            DX, DW, DB = j["ref"]
            assert relx(j["X"].cpu().numpy(), DX, D) < RTOL, "dX stream %d" % k
            assert relx(j["DW"].cpu().numpy(), DW, D) < RTOL, "dW stream %d" % k
            assert relx(j["DB"].cpu().numpy(), DB, D) < RTOL, "dB stream %d" % k
    finally:
        t4k.call("t4k_stream_destroy", s_lib)


@pytest.mark.parametrize("pre,pool,KS,C", [("leaky", None, 1, 8), ("relu", "max", 2, 6), (None, "max", 2, 5), ("tanh", "avg", 3, 4)])
def test_poolblock_with_dropout_behind(t4k, dev, oracle, pre, pool, KS, C):
    """A dropout layer as the LAST stage of an element-wise run (`leakyrelu dropout` of the GAN nets, `maxpool dropout` of the CIFAR nets):
    one launch each way == the oracle's separate layers; the mask is the Philox slice t4k_dropout_mask draws for that tensor."""
    o = oracle.lib(); P = oracle.P
    LAY = {"leaky": (oracle.L_LEAKYRL, 0.2), "relu": (oracle.L_RELU, 0.0), "tanh": (oracle.L_TANH, 0.0), "max": oracle.L_MAXPOOL, "avg": oracle.L_AVGPOOL}
    rng = np.random.default_rng(KS * 10 + C)
    N, H1 = 4, 12; H0 = H1 // KS
    n1, n0 = N * H1 * H1 * C, N * H0 * H0 * C
    X = rng.standard_normal((N, H1, H1, C)).astype(np.float32); DY = rng.standard_normal((N, H0, H0, C)).astype(np.float32)
    seed, off = 21, 1 << 12
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    ref = {}; x = X
    if pre:
        L, a = LAY[pre]; f = np.zeros(n1, np.float32); y = np.zeros_like(X)
        o.t4o_activate(L, P(x), P(y), P(f), a, n1); ref["pre_mask"] = f.reshape(X.shape); ref["pre_out"] = y; x = y
    if pool:
        q = np.zeros((N, H0, H0, C), np.float32); o.t4o_pool(LAY[pool], P(x), P(q), N, H1, H1, H0, H0, C, KS); ref["pool_out"] = q; x = q
    m = np.zeros(n0, np.float32); o.t4o_dropout_mask(P(m), n0)
    y = np.zeros((N, H0, H0, C), np.float32); o.t4o_activate(oracle.L_DROPOUT, P(x), P(y), P(m), 0.3, n0)
    ref["post_mask"] = m.reshape(y.shape); ref["post_out"] = y
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
    d = {k: dev.zeros(v.shape) for k, v in ref.items()}
    dX = dev.up(X)
    blk = PoolBlock(); blk.KS = KS
    if pre: blk.pre_layer, blk.pre_alpha = LAY[pre]; blk.pre_mask = p(d["pre_mask"]); blk.pre_out = p(d["pre_out"])
    if pool: blk.pool_layer = LAY[pool]; blk.pool_out = p(d["pool_out"])
    blk.post_layer, blk.post_alpha = oracle.L_DROPOUT, 0.3; blk.post_mask = p(d["post_mask"]); blk.post_out = p(d["post_out"])
    t4k.call("t4k_poolblock_fwd", p(dX), ctypes.byref(blk), N, H1, H1, H0, H0, C, None)
    assert np.array_equal(dev.down(d["post_mask"]), ref["post_mask"]) and t4k.lib.t4k_rand_offset() == o.t4o_rand_offset()
    for k_ in ("post_out", "pool_out", "pre_out"):
        if k_ in ref: assert rel(dev.down(d[k_]), ref[k_]) < 1e-6, k_
    # backward: gradient through the dropout mask, the pool scatter and the pre activation
    g = np.zeros(n0, np.float32); o.t4o_tt_op(oracle.MUL, P(DY), P(ref["post_mask"]), P(g), n0)
    Xb = X.copy(); src = ref["pre_out"].copy() if pre else Xb
    if pool:
        o.t4o_dpool(LAY[pool], P(src), P(g), N, H1, H1, H0, H0, C, KS); g1 = src.ravel().copy()
    else:
        g1 = g
    if pre:
        t = np.zeros(n1, np.float32); o.t4o_tt_op(oracle.MUL, P(g1), P(ref["pre_mask"]), P(t), n1); want = t
    else:
        want = g1
    t4k.call("t4k_poolblock_bwd", p(dev.up(DY)), p(dX), ctypes.byref(blk), N, H1, H1, H0, H0, C, None)
    assert rel(dev.down(dX).ravel(), want.ravel()) < 1e-6


@pytest.mark.parametrize("M,N,K", [(2048, 2048, 256), (1024, 4096, 384), (4096, 1024, 128)])
def test_gemm_large_plain_products_exact_on_integer_operands(t4k, dev, M, N, K):
    """Large plain products (more than one 64x64 tile per CU) run on the same LDS-DMA kernel as the 1024^3 `matmul`: entries in {-2..2}
    make every partial sum exact in fp32, so the result must equal numpy's integer product bit for bit, whatever the tile order."""
    rng = np.random.default_rng(M + N + K)
    A = rng.integers(-2, 3, (M, K)).astype(np.float32); B = rng.integers(-2, 3, (K, N)).astype(np.float32)
    want = (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float32)
    dO = dev.zeros((M, N))
    t4k.call("t4k_gemm", p(dev.up(A)), p(dev.up(B)), p(dO), 1.0, 0.0, 0, 0, M, N, K, 1, None)
    assert np.array_equal(dev.down(dO), want)


@pytest.mark.parametrize("M,N,K,tA,tB", [(1024, 1000, 512, 0, 0), (1000, 1028, 256, 0, 1), (996, 1000, 384, 1, 0), (516, 2044, 128, 1, 1),
                                         (40, 72, 64, 0, 1), (200, 100, 832, 0, 1), (36, 28, 96, 1, 0),
                                         # ragged K on the LDS-DMA kernel (partial last stage): 784 = 6 x 128 + 16, every layout; a tail of 4 (half a
                                         # chunk: zeroed in registers); K below one stage; K % 4 != 0 where no operand is K-contiguous; ragged M, N and K
                                         (1024, 1024, 784, 0, 0), (1024, 1024, 784, 0, 1), (1024, 1024, 784, 1, 0), (1024, 1024, 784, 1, 1),
                                         (1024, 1024, 132, 0, 1), (1024, 1024, 100, 0, 0), (1024, 1088, 50, 1, 0), (1024, 1024, 1021, 1, 0),
                                         (1000, 1028, 1004, 0, 1), (1028, 1000, 252, 1, 1), (1024, 1024, 8, 0, 1), (1024, 1024, 12, 0, 0),
                                         # 86..128 interior tiles, K in 256s from 1024: two workgroups per tile, combined in the epilogue (k_gemm_nn_plain<.., PAIR>) - the
                                         # two K = 1024 shapes; K = 512 and 768 are <= 832 and stay on the sliver kernel (l32/w4/rst, l32/w8/rst): the rung in front
                                         # takes them.  tests/test_gpu_gemm_sweep.py asserts the rung of its own pair rows (576 x 640 x 1024, 1024 x 512 x 1024, 640 x 576 x 1280)
                                         (512, 1024, 1024, 0, 0), (512, 1024, 1024, 0, 1), (1024, 512, 512, 1, 0), (576, 832, 768, 1, 1),
                                         # interior tiles, every layout, on the lean kernel (one tile per CU and several)
                                         (1024, 1024, 1024, 0, 1), (1024, 1024, 512, 1, 0), (1024, 1024, 256, 1, 1), (1088, 1024, 384, 0, 1),
                                         # round 4: slivers on LDS-DMA operand blocks (k_gemm_l32) - the GAN's 256-row layers in the layouts of forward / dX / dW,
                                         # K tails of half a block (784 = 24.5 x 32) and of 4 (100, 980, 772), 4 and 8 k-groups, ranges with blocks 2-3 held in
                                         # registers (K > 256 with 4 waves, K > 512 with 8), ragged M / N edge tiles in every layout
                                         (256, 512, 784, 0, 1), (256, 784, 512, 0, 0), (512, 784, 256, 1, 0), (256, 256, 128, 0, 1), (256, 100, 980, 0, 1),
                                         (128, 980, 100, 0, 0), (100, 980, 128, 1, 0), (252, 500, 772, 0, 1), (252, 500, 772, 0, 0), (252, 500, 260, 1, 0),
                                         (260, 36, 516, 1, 1), (256, 512, 832, 0, 1), (64, 2000, 416, 0, 0), (256, 1, 256, 0, 1)])
def test_gemm_ragged_edges_and_slivers_exact_on_integer_operands(t4k, dev, M, N, K, tA, tB):
    """Ragged M / N (not multiples of the tile) on the LDS-DMA kernel with clamped source rows, and sliver shapes on the 32x32
    register-fetch kernel, every operand layout: entries in {-2..2} keep fp32 sums exact, so the product must equal numpy's bit for bit
    (a clamped row or column leaking into a stored element, or a k group counted twice, would show)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + tA * 2 + tB)
    A = rng.integers(-2, 3, (M, K)).astype(np.float32); B = rng.integers(-2, 3, (K, N)).astype(np.float32)
    want = (A.astype(np.int64) @ B.astype(np.int64)).astype(np.float32)
    O0 = rng.integers(-3, 4, (M, N)).astype(np.float32); bias = None
    dA = dev.up(np.ascontiguousarray(A.T) if tA else A); dB = dev.up(np.ascontiguousarray(B.T) if tB else B)
    dO = dev.up(O0)
    t4k.call("t4k_gemm", p(dA), p(dB), p(dO), 2.0, -1.0, tA, tB, M, N, K, 1, None)        # alpha, beta exact in fp32 too
    assert np.array_equal(dev.down(dO), 2.0 * want - O0)
    t4k.call("t4k_gemm", p(dA), p(dB), p(dO), 1.0, 0.0, tA, tB, M, N, K, 1, None)         # again, no epilogue (tickets / flags of a paired launch were left clean)
    assert np.array_equal(dev.down(dO), want)


@pytest.mark.parametrize("M,N,K,tA,tB", [(2048, 2048, 2048, 0, 1), (1024, 4096, 2048, 1, 0), (2040, 2048, 2112, 1, 1),
                                         # 128x128 tiles on the lean pipeline (k_gemm_plain128): every layout, K in 64s, several tiles per CU, non-square tile grids
                                         (2048, 2048, 512, 0, 0), (2048, 2048, 320, 1, 1), (2176, 4096, 256, 1, 0), (4096, 2304, 448, 0, 1),
                                         # ... with a partial last K stage (k_gemm_plain128<RAGK>): tails of 16, 8 (one k-group idle), 44 (a partial chunk), 60
                                         (2048, 2048, 784, 0, 1), (2048, 2048, 328, 1, 0), (2048, 2304, 300, 0, 0), (2304, 2048, 444, 1, 1), (2048, 2048, 784, 0, 0),
                                         # ... two workgroups per CU on 32-deep stages (k_gemm_plain128<.., 32>, grids of >= 512 tiles; the two shapes above with 544 / 576 tiles take it too):
                                         # every layout, K in whole 32s that are not whole 64s (unragged for this form), a deep K
                                         (2048, 4096, 288, 0, 0), (4096, 2048, 480, 1, 1), (4096, 2048, 512, 0, 1), (2048, 4096, 1056, 1, 0),
                                         # ... grids of 256 x 256 tiles and more with K < 256: launch_plain128 (the only way to k_gemm_plain256) sits behind K >= 256, so these take
                                         # plain_ragk (K = 160, 224), mfma<128,128,32,vec,skew> (K = 96) and mfma<128,128,32,vec,full> (K = 64; ragged 64-tile grid 4352 = 34 x 128);
                                         # k_gemm_plain256 itself: the plain256 rows of tests/test_gpu_gemm_sweep.py (4096 x 4096 x 256 .. 320, every layout)
                                         (4096, 4096, 160, 0, 0), (4096, 4096, 96, 1, 1), (4096, 4352, 224, 0, 1), (4352, 4096, 64, 1, 0)])
def test_gemm_large_transposed_products_exact_on_integer_operands(t4k, dev, M, N, K, tA, tB):
    """Large products with transposed operands and alpha / beta (the linear layers of an MLP) on the 8-wave LDS-DMA kernel, several 64x64
    tiles per CU, one shape with a ragged M: small-integer entries keep every fp32 sum exact, so the result equals the float64 product."""
    rng = np.random.default_rng(M + N + K + tA + 2 * tB)
    A = rng.integers(-2, 3, (M, K)).astype(np.float32); B = rng.integers(-2, 3, (K, N)).astype(np.float32)
    want = A.astype(np.float64) @ B.astype(np.float64)
    O0 = rng.integers(-3, 4, (M, N)).astype(np.float32)
    dA = dev.up(np.ascontiguousarray(A.T) if tA else A); dB = dev.up(np.ascontiguousarray(B.T) if tB else B); dO = dev.up(O0)
    t4k.call("t4k_gemm", p(dA), p(dB), p(dO), 2.0, -1.0, tA, tB, M, N, K, 1, None)
    assert np.array_equal(dev.down(dO).astype(np.float64), 2.0 * want - O0)
    t4k.call("t4k_gemm", p(dA), p(dB), p(dO), 1.0, 0.0, tA, tB, M, N, K, 1, None)         # and the kernels without an epilogue
    assert np.array_equal(dev.down(dO).astype(np.float64), want)


@pytest.mark.parametrize("N,E1,E0,stages,copy", [
    (256, 784, 512, ("leaky", "drop"), True),      # GAN discriminator layer 0: split-K, run of two and the layer-0 copy in the fold launch
    (256, 512, 256, ("leaky", "drop"), False),
    (256, 128, 256, ("leaky",), True),             # GAN generator layer 0
    (64, 300, 128, ("drop", "tanh"), True),        # dropout first, ragged K
    (2048, 256, 1024, ("relu", "drop"), True),     # output fills the chip: unsplit GEMM, separate launches, same tensors
    (128, 320, 10, ("relu", "drop"), True),        # classifier-head sized: the vector-ALU linear kernel
    (32, 100, 64, (), True),                       # no run at all: linear + copy
])
def test_linear_block_forward(t4k, dev, oracle, N, E1, E0, stages, copy):
    """t4k_linear_block_fwd == copy + linear + the element-wise layers of the oracle, one after the other (masks bit-exact, stream position equal)"""
    o = oracle.lib(); P = oracle.P
    LAY = {"leaky": (oracle.L_LEAKYRL, 0.2), "relu": (oracle.L_RELU, 0.0), "tanh": (oracle.L_TANH, 0.0), "drop": (oracle.L_DROPOUT, 0.3)}
    rng = np.random.default_rng(N + E1 + E0)
    X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) / np.sqrt(E1)).astype(np.float32)
    B = rng.standard_normal(E0).astype(np.float32)
    seed, off = 5, 1 << 10
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off)
    Y = np.zeros((N, E0), np.float32); o.t4o_linear_fwd(P(X), P(W), P(B), P(Y), N, E0, E1)
    ref = []; x = Y
    for st_ in stages:
        L, a = LAY[st_]; f = np.zeros(N * E0, np.float32); y = np.zeros_like(Y)
        if st_ == "drop": o.t4o_dropout_mask(P(f), N * E0)
        o.t4o_activate(L, P(x), P(y), P(f), a, N * E0); ref.append((f.reshape(Y.shape), y)); x = y
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
    dY = dev.zeros((N, E0)); dC = dev.zeros((N, E1)); d = [(dev.zeros((N, E0)), dev.zeros((N, E0))) for _ in stages]
    blk = PoolBlock(); blk.KS = 1
    if len(stages) >= 1:
        if len(stages) == 2 or stages[0] != "drop":
            blk.pre_layer, blk.pre_alpha = LAY[stages[0]]; blk.pre_mask = p(d[0][0]); blk.pre_out = p(d[0][1])
        else:                                       # a lone stage may sit in either slot: exercise `post` for the lone dropout
            blk.post_layer, blk.post_alpha = LAY[stages[0]]; blk.post_mask = p(d[0][0]); blk.post_out = p(d[0][1])
    if len(stages) == 2:
        blk.post_layer, blk.post_alpha = LAY[stages[1]]; blk.post_mask = p(d[1][0]); blk.post_out = p(d[1][1])
    t4k.call("t4k_linear_block_fwd", p(dev.up(X)), p(dC) if copy else None, p(dev.up(W)), p(dev.up(B)), p(dY),
             ctypes.byref(blk) if stages else None, N, E0, E1, None)
    assert t4k.lib.t4k_rand_offset() == o.t4o_rand_offset()
    assert rel(dev.down(dY), Y) < 2e-6
    if copy: assert np.array_equal(dev.down(dC), X)
    for (f, y), (df, dy), st_ in zip(ref, d, stages):
        if st_ == "drop": assert np.array_equal(dev.down(df), f), "mask"
        else: assert rel(dev.down(df), f) < 1e-5
        assert rel(dev.down(dy), y) < 2e-6, st_


@pytest.mark.parametrize("N,E1,E0,stages,train,tgt", [
    (256, 512, 256, ("leaky", "drop"), 1, False),   # interior tiles: the dual dW || dX launch carries the mask chain
    (256, 784, 512, ("leaky", "drop"), 1, False),   # ragged E1
    (256, 256, 1, ("leaky", "drop"), 1, True),      # GAN discriminator head: vector-ALU kernel, `out -= target` in the same launch
    (256, 256, 1, ("leaky", "drop"), 0, True),      # frozen discriminator head (train_g): target, dX and both masks in the head kernel, no dW workgroups
    (256, 512, 256, ("leaky", "drop"), 0, False),   # frozen net: dX only, the chain rides in the GEMM launch
    (64, 128, 64, ("relu",), 0, False),             # shallow K: unsplit GEMM, separate launches
    (128, 320, 100, ("drop",), 1, True),            # lone stage in the post slot + target
    (2048, 1024, 1024, ("tanh", "drop"), 1, False), # large: 128x128 tiles, layer by layer
])
def test_linear_block_backward(t4k, dev, oracle, N, E1, E0, stages, train, tgt):
    """t4k_linear_block_bwd == (out -= target) + linear backward + the mask multiplies of the run in front, oracle layer by layer"""
    D = max(E1, E0, N)                                   # depth of the deepest fp32 sum behind a compared element (relx)
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(N + E1 + E0 + train)
    X = rng.standard_normal((N, E1)).astype(np.float32); W = (rng.standard_normal((E0, E1)) / np.sqrt(E1)).astype(np.float32)
    DY = rng.standard_normal((N, E0)).astype(np.float32); T = rng.standard_normal((N, E0)).astype(np.float32)
    DW0 = rng.standard_normal((E0, E1)).astype(np.float32); DB0 = rng.standard_normal(E0).astype(np.float32)
    masks = [(rng.random((N, E1)) < 0.6).astype(np.float32) * np.float32(1.5) for _ in stages]    # forward order: stage 0 sits in front
    dy = DY - T if tgt else DY.copy()
    DX = np.zeros((N, E1), np.float32); DW = DW0.copy(); DB = DB0.copy()
    Xc = X.copy()                                                  # keep the array alive across the call
    o.t4o_linear_bwd(P(Xc), P(W), P(dy), P(DX), P(DW), P(DB), N, E0, E1, train)
    g = [DX]
    for m in reversed(masks): g.append(g[-1] * m)                  # last stage first
    dX = dev.up(X); dDY = dev.up(DY); dDY2 = dev.zeros((N, E0)); dDW = dev.up(DW0); dDB = dev.up(DB0)
    dm = [dev.up(m) for m in masks]; dpre_out = dev.zeros((N, E1)); dxrun = dev.zeros((N, E1))
    blk = PoolBlock(); blk.KS = 1
    if len(stages) == 2:
        blk.pre_layer = oracle.L_LEAKYRL; blk.pre_mask = p(dm[0]); blk.pre_out = p(dpre_out)
        blk.post_layer = oracle.L_DROPOUT; blk.post_mask = p(dm[1]); blk.post_out = p(dX)
    elif stages[0] == "drop":
        blk.post_layer = oracle.L_DROPOUT; blk.post_mask = p(dm[0]); blk.post_out = p(dX)
    else:
        blk.pre_layer = oracle.L_RELU; blk.pre_mask = p(dm[0]); blk.pre_out = p(dX)
    t4k.call("t4k_linear_block_bwd", p(dX), p(dev.up(W)), p(dDY), p(dev.up(T)) if tgt else None, p(dDY2) if tgt else None, p(dX),
             ctypes.byref(blk), p(dxrun), p(dDW) if train else None, p(dDB) if train else None, N, E0, E1, train, None)
    tol = 3e-6 * max(1.0, np.sqrt(max(N, E0) / 256.0))          # (float64 reference: the tensor-norm figure at a few ulps; the element-aware bar follows at RTOL)
    assert rel(dev.down(dX), g[0]) < tol, "dX"
    if len(stages) == 2: assert rel(dev.down(dpre_out), g[1]) < tol, "post stage input gradient"
    assert rel(dev.down(dxrun), g[-1]) < tol, "run input gradient"
    assert relx(dev.down(dX), g[0], D) < RTOL and relx(dev.down(dxrun), g[-1], D) < RTOL, "element-aware bar"
    if tgt: assert np.array_equal(dev.down(dDY), dy) and np.array_equal(dev.down(dDY2), dy)
    if train:
        assert rel(dev.down(dDW), DW) < tol and rel(dev.down(dDB), DB) < tol
    else:
        assert np.array_equal(dev.down(dDW), DW0) and np.array_equal(dev.down(dDB), DB0)


@pytest.mark.parametrize("N,C", [(128, 10), (5, 1), (300, 1000), (1, 37)])
def test_logsoftmax_layer_as_the_reference_writes_it(t4k, dev, N, C):
    """O = exp(I) - log10(max(sum exp(I), 1e-6)), the row sum taken in index order (_flogsoftmax forward.cu:245-259, quirk a-16)"""
    rng = np.random.default_rng(N + C)
    X = (rng.standard_normal((N, C)) * 2).astype(np.float32); X[0, :] = -40.0      # one row whose sum falls below the epsilon floor
    e = np.exp(X.astype(np.float64)).astype(np.float32)
    s = np.zeros(N, np.float32)
    for c in range(C): s = (s + e[:, c]).astype(np.float32)                         # sequential fp32 row sums
    want = e - np.log10(np.maximum(s, np.float32(1e-6)))[:, None].astype(np.float32)
    d = dev.zeros((N, C))
    t4k.call("t4k_logsoftmax", p(dev.up(X)), p(d), N, C, None)
    np.testing.assert_allclose(dev.down(d), want, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("N,E0,E1", [(256, 512, 784), (256, 256, 512), (256, 784, 512), (128, 100, 980), (256, 512, 256), (252, 260, 516), (64, 36, 132)])
def test_linear_backward_dual_launch_on_lds_dma_blocks_exact_on_integer_operands(t4k, dev, N, E0, E1):
    """dW += dY^T X (+ dB) and dX = dY W of one linear layer in ONE launch on LDS-DMA operand blocks (k_gemm_dual_l32: 4 waves, 8 waves for the
    deep 784 -> 512 dX, blocks 2-3 in registers for K > 256), dX over X in place behind the arrival slots and apart, twice in a row (epochs):
    entries in {-2..2} keep every fp32 sum exact, so dW, dB and dX must equal numpy's integer products bit for bit - a reader that reported
    early, a k block counted twice or a clamped edge row leaking into a stored element would show."""
    rng = np.random.default_rng(N + 3 * E0 + 7 * E1)
    X = rng.integers(-2, 3, (N, E1)).astype(np.float32); W = rng.integers(-2, 3, (E0, E1)).astype(np.float32)
    G = rng.integers(-2, 3, (N, E0)).astype(np.float32)
    DW0 = rng.integers(-3, 4, (E0, E1)).astype(np.float32); DB0 = rng.integers(-3, 4, E0).astype(np.float32)
    wdw = (G.astype(np.int64).T @ X.astype(np.int64)).astype(np.float32); wdb = G.astype(np.int64).sum(0).astype(np.float32)
    wdx = (G.astype(np.int64) @ W.astype(np.int64)).astype(np.float32)
    dW, dG = dev.up(W), dev.up(G)
    for rep in range(2):
        dX, dDW, dDB = dev.up(X), dev.up(DW0), dev.up(DB0)
        t4k.call("t4k_linear_bwd", p(dX), p(dW), p(dG), p(dX), p(dDW), p(dDB), N, E0, E1, 1, None)      # in place
        assert np.array_equal(dev.down(dX), wdx), rep
        assert np.array_equal(dev.down(dDW), DW0 + wdw) and np.array_equal(dev.down(dDB), DB0 + wdb), rep
        dX2, dDX, dDW2, dDB2 = dev.up(X), dev.zeros((N, E1)), dev.up(DW0), dev.up(DB0)
        t4k.call("t4k_linear_bwd", p(dX2), p(dW), p(dG), p(dDX), p(dDW2), p(dDB2), N, E0, E1, 1, None)  # apart
        assert np.array_equal(dev.down(dDX), wdx) and np.array_equal(dev.down(dX2), X), rep
        assert np.array_equal(dev.down(dDW2), DW0 + wdw) and np.array_equal(dev.down(dDB2), DB0 + wdb), rep
