"""The small kernels every training step runs (reduce.hip, elementwise.hip, optim.hip, linalg.hip, dconv.hip) at the sizes their launchers
branch on, through the C ABI.  Every case holds the product AND the oracle to the float64 witness (tests/f64_witness.py); sums over
small-integer operands must be bit-equal to the int64 sum (any order is exact, so a dropped or doubled element shows); exact ops stay
bit-equal to the oracle.  Where the launch plan is observable it is asserted with t4k_launch_count() deltas, so a case proves it reached the
branch it names.  Sizes and inputs: tests/small_kernel_cases.py (shared with the CPU self-test of the witnesses).

Kernels with a `bool vec` flag and the case that runs their scalar branch (base pointer offset by 4 bytes): k_reduce1 (test_reductions_*,
test_bce_*), k_math / k_ts / k_tt / k_copy (test_elementwise_*), k_activate (test_activations_*); launch_bn_part's scalar k_bn_part for
C % 4 == 0 (test_batchnorm_from_a_four_byte_offset_base)."""
import ctypes
import struct

import numpy as np
import pytest

import f64_witness as wt
import small_kernel_cases as sk
from test_gpu_parity import Dev, p, rel, relx, RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


def launches(t4k):
    return int(t4k.lib.t4k_launch_count())


def up_off(dev, a, off):
    """`a` uploaded so that it starts `off` elements into a 16-byte aligned buffer: (tensor, pointer of a[0])"""
    a = np.ascontiguousarray(a); buf = np.zeros(a.size + off + 4, a.dtype); buf[off:off + a.size] = a.ravel()
    t = dev.up(buf)
    assert p(t) % 16 == 0
    return t, p(t) + 4 * off


def dn_off(dev, t, off, shape):
    return dev.down(t)[off:off + int(np.prod(shape))].reshape(shape)


# ----------------------------------------------------------------------------- reductions
def _reduce_many(t4k, dev, oracle, x, op, avg, ns, offs, plan=True):
    """t4k_reduce over x[off : off + n] for every (n, off), each result into its own slot; ONE upload, one download"""
    d = dev.up(x); out = dev.zeros(len(ns) * len(offs)); k = 0
    for n in ns:
        for off in offs:
            assert off + n <= x.size
            l0 = launches(t4k)
            t4k.call("t4k_reduce", op, p(d) + 4 * off, n, avg, p(out) + 4 * k, None)
            if plan:
                assert launches(t4k) - l0 == (1 if n <= sk.RED_PER_BLOCK else 2), (n, off)       # one workgroup finishes alone; more leave partials for k_reduce2
            k += 1
    return dev.down(out).reshape(len(ns), len(offs))


def test_reductions_are_bit_exact_on_integer_operands_at_every_launch_plan(t4k, dev, oracle):
    """SUM / MAX / MIN at every n of the sweep, from a 16-byte aligned base, a 4-byte aligned one (k_reduce1's scalar loop) and 16 bytes on;
    NVAR with an integer mean where (x - avg)^2 keeps the sum below 2^24.  One launch up to 4096 elements, two above (asserted)."""
    rng = np.random.default_rng(40)
    x = sk.ints(rng, sk.RED_N[-1] + 8)
    got = _reduce_many(t4k, dev, oracle, x, oracle.RED_SUM, 0.0, sk.RED_N, sk.RED_OFFSETS)
    gmx = _reduce_many(t4k, dev, oracle, x, oracle.RED_MAX, 0.0, sk.RED_N, sk.RED_OFFSETS)
    gmn = _reduce_many(t4k, dev, oracle, x, oracle.RED_MIN, 0.0, sk.RED_N, sk.RED_OFFSETS)
    for i, n in enumerate(sk.RED_N):
        for j, off in enumerate(sk.RED_OFFSETS):
            s = x[off:off + n]
            wt.check("sum n=%d off=%d" % (n, off), got[i, j], wt.reduce_sum(s, exact=True), kind="reduce sum (integer)")
            wt.equal("max n=%d off=%d" % (n, off), gmx[i, j], s.max(), kind="reduce max/min"); wt.equal("min n=%d off=%d" % (n, off), gmn[i, j], s.min(), kind="reduce max/min")
        wt.check("oracle sum n=%d" % n, oracle.reduce(oracle.RED_SUM, x[:n]), wt.reduce_sum(x[:n], exact=True))
    # NVAR: x in +-{1, 2, 3} about avg = 1 (terms <= 16) up to a million elements; x = +-1 about avg = 0 at every n (terms = 1)
    ns = tuple(n for n in sk.RED_N if wt.is_int_exact(n, 16)) + (1000003,)
    got = _reduce_many(t4k, dev, oracle, x, oracle.RED_NVAR, 1.0, ns, sk.RED_OFFSETS)
    for i, n in enumerate(ns):
        for j, off in enumerate(sk.RED_OFFSETS):
            wt.check("nvar n=%d off=%d" % (n, off), got[i, j], wt.reduce_nvar(x[off:off + n], 1.0, exact=True), kind="reduce nvar (integer)")
    y = np.sign(x)
    got = _reduce_many(t4k, dev, oracle, y, oracle.RED_NVAR, 0.0, sk.RED_N, sk.RED_OFFSETS)
    assert np.array_equal(got, np.repeat(np.array(sk.RED_N, np.float32)[:, None], len(sk.RED_OFFSETS), 1))


@pytest.mark.parametrize("kind", ["normal", "scaled"])
def test_reductions_on_float_operands_against_float64(t4k, dev, oracle, kind):
    rng = np.random.default_rng(41)
    x = sk.floats(rng, sk.RED_FLOAT_N[-1] + 8, kind)
    got = _reduce_many(t4k, dev, oracle, x, oracle.RED_SUM, 0.0, sk.RED_FLOAT_N, sk.RED_OFFSETS)
    avg = float(np.float32(x.mean()))
    gv = _reduce_many(t4k, dev, oracle, x, oracle.RED_NVAR, avg, sk.RED_FLOAT_N, sk.RED_OFFSETS)
    for i, n in enumerate(sk.RED_FLOAT_N):
        for j, off in enumerate(sk.RED_OFFSETS):
            s = x[off:off + n]
            wt.check("sum %s n=%d off=%d" % (kind, n, off), got[i, j], wt.reduce_sum(s), kind="reduce sum"); wt.check("oracle sum", oracle.reduce(oracle.RED_SUM, s), wt.reduce_sum(s))
            wt.check("nvar %s n=%d off=%d" % (kind, n, off), gv[i, j], wt.reduce_nvar(s, avg), kind="reduce nvar"); wt.check("oracle nvar", oracle.reduce(oracle.RED_NVAR, s, avg), wt.reduce_nvar(s, avg))
            assert abs(float(got[i, j]) - s.astype(np.float64).sum()) < 1e-4 * max(1.0, np.abs(s).sum())          # the earlier bar, kept beside the witness


def test_max_min_find_an_extreme_wherever_it_sits_and_nan_inf_counts_the_tail(t4k, dev, oracle):
    """the extreme in the vector tail (n % 4 != 0), in the last block's last lane, at index 0; signed zeros as the oracle has them"""
    rng = np.random.default_rng(42)
    for n in (4097, 65539, sk.RED_STRIDE_N + 1):
        for off in (0, 1):
            for pos in (0, n - 1, (n // 4) * 4, ((n - 1) // sk.BLK) * sk.BLK - 1, sk.RED_PER_BLOCK * 3 + 255 if n > 20000 else 255):
                x = rng.standard_normal(n + off).astype(np.float32)
                x[off + pos] = 9.0; d = dev.up(x); out = dev.zeros(2)
                t4k.call("t4k_reduce", oracle.RED_MAX, p(d) + 4 * off, n, 0.0, p(out), None)
                x[off + pos] = -9.0; d2 = dev.up(x)
                t4k.call("t4k_reduce", oracle.RED_MIN, p(d2) + 4 * off, n, 0.0, p(out) + 4, None)
                assert tuple(dev.down(out)) == (9.0, -9.0), (n, off, pos)
    for z in (np.array([-0.0, 0.0, -0.0], np.float32), np.array([0.0, -0.0], np.float32), np.full(4097, -0.0, np.float32)):
        for op in (oracle.RED_MAX, oracle.RED_MIN):
            out = dev.zeros(1); t4k.call("t4k_reduce", op, p(dev.up(z)), z.size, 0.0, p(out), None)
            g = dev.down(out)[0]; o = np.float32(oracle.reduce(op, z))
            assert g == o == 0.0                                           # equal as numbers (the witness's sense of exact) ...
            if np.all(np.signbit(z)):
                assert np.signbit(g) and np.signbit(o)                     # ... and with nothing but -0.0 to pick from, -0.0 on both sides
    n = 5000003; x = rng.standard_normal(n + 1).astype(np.float32); cnt = dev.zeros(2, dev.torch.int32)
    hits = (0, 17, sk.GRID1_STRIDE_N * 8, n - 1, n - 2, n - 3)
    for k, h in enumerate(hits):
        x[1 + h] = (np.nan, np.inf, -np.inf)[k % 3]
    d = dev.up(x)
    t4k.call("t4k_nan_inf", p(d) + 4, n, p(cnt), None); t4k.call("t4k_nan_inf", p(d), n - 3, p(cnt) + 4, None)
    assert tuple(dev.down(cnt)) == (len(hits), len(hits) - 3)           # the second call stops short of the three hits in the tail
    wt.equal("nan_inf", dev.down(cnt)[0], wt.nan_inf(x[1:]).exact)


def _bce_many(t4k, dev, T, O, ns, offs):
    dT, dO = dev.up(T), dev.up(O); out = dev.zeros(len(ns) * len(offs)); k = 0
    for n in ns:
        for off in offs:
            assert off + n <= T.size
            l0 = launches(t4k)
            t4k.call("t4k_bce", p(dT) + 4 * off, p(dO) + 4 * off, n, p(out) + 4 * k, None)
            assert launches(t4k) - l0 == (1 if n <= sk.RED_PER_BLOCK else 2)
            k += 1
    return dev.down(out).reshape(len(ns), len(offs))


def test_bce_at_every_launch_plan_against_float64(t4k, dev, oracle):
    """targets in {0, 1} and soft targets, outputs in [0.01, 0.99] (|log| >= 0.01); the device's __logf carries wt.ULP_LOG, libm 2 ulp"""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(43)
    N = sk.RED_N[-1] + 8
    for soft in (False, True):
        T = (rng.random(N) if soft else rng.integers(0, 2, N)).astype(np.float32); O = rng.uniform(0.01, 0.99, N).astype(np.float32)
        got = _bce_many(t4k, dev, T, O, sk.RED_N, sk.RED_OFFSETS)
        for i, n in enumerate(sk.RED_N):
            for j, off in enumerate(sk.RED_OFFSETS):
                t, y = T[off:off + n].copy(), O[off:off + n].copy()
                wt.check("bce n=%d off=%d" % (n, off), got[i, j], wt.bce(t, y), kind="bce")
                if j == 0:
                    r = np.zeros(1, np.float32); o.t4o_bce(P(t), P(y), n, P(r)); wt.check("oracle bce n=%d" % n, r[0], wt.bce(t, y, wt.ULP_LOG_LIBM))


def test_device_log_error_is_inside_the_allowance(t4k, dev, oracle):
    """measures what wt.ULP_LOG allows for: the worst |__logf(x) - ln x| / (2^-24 |ln x|) over the BCE arguments, through t4k_math LN (the same
    __logf) and through single-term t4k_bce calls (t = 1: the term IS ln(o + eps)); printed, and held to HALF the allowance"""
    x = np.concatenate([np.linspace(0.01, 0.99 + 1e-6, 1500000), 1.0 - np.linspace(0.01, 0.99, 4000) + 1e-6]).astype(np.float32)
    d = dev.up(x); t4k.call("t4k_math", oracle.LN, p(d), 0.0, x.size, None)
    ex = np.log(x.astype(np.float64)); r_ln = float(np.max(np.abs(dev.down(d) - ex) / (wt.U * np.abs(ex))))
    y = np.linspace(0.01, 0.99, 3000).astype(np.float32); one = dev.up(np.ones(1, np.float32)); dy = dev.up(y); out = dev.zeros(y.size)
    for k in range(y.size):
        t4k.call("t4k_bce", p(one), p(dy) + 4 * k, 1, p(out) + 4 * k, None)
    ex = np.log(y.astype(np.float64) + wt.EPS)
    r_bce = float(np.max((np.abs(dev.down(out) - ex) - 2.0 * wt.U) / (wt.U * np.abs(ex))))       # net of the argument's rounding (o + eps: 2 u absolute)
    print("\ndevice log error, ulps of |ln x|: t4k_math LN %.3f, single BCE terms %.3f (allowance wt.ULP_LOG = %.1f)" % (r_ln, r_bce, wt.ULP_LOG))
    wt.WORST["device log ulps (measured, not a ratio)"] = (max(r_ln, r_bce), "LN %.3f / BCE term %.3f" % (r_ln, r_bce))
    assert 2.0 * max(r_ln, r_bce) <= wt.ULP_LOG


def test_dot_integer_exact_and_float(t4k, dev, oracle):
    """k_dot: K across the 256-lane trip boundary, C from 1 to 300.  beta == 0 over an output pre-filled with NaN: the ORACLE multiplies the
    stale output by beta as the reference does (0 * NaN = NaN); the kernel special-cases beta == 0 and never reads it (the BLAS convention,
    the witness's too).  Both are asserted: the quirk is the reference's, and `dot` on the host relies on the kernel's reading."""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(44)
    for K in sk.DOT_K:
        for C in sk.DOT_C:
            for ints in (True, False):
                A = sk.ints(rng, (K, C)) if ints else rng.standard_normal((K, C)).astype(np.float32)
                B = sk.ints(rng, (K, C)) if ints else rng.standard_normal((K, C)).astype(np.float32)
                O0 = sk.ints(rng, C) if ints else rng.standard_normal(C).astype(np.float32)
                dA, dB = dev.up(A), dev.up(B)
                for alpha, beta in sk.DOT_AB:
                    w = wt.dot(A, B, O0, alpha, beta, exact=ints)
                    dO = dev.up(O0); t4k.call("t4k_dot", p(dA), p(dB), p(dO), alpha, beta, K, C, None)
                    wt.check("dot K=%d C=%d %s" % (K, C, (alpha, beta)), dev.down(dO), w, kind="dot (integer)" if ints else "dot")
                    r = O0.copy(); o.t4o_dot(P(A), P(B), P(r), alpha, beta, K, C); wt.check("oracle dot", r, w)
                dO = dev.up(np.full(C, np.nan, np.float32)); t4k.call("t4k_dot", p(dA), p(dB), p(dO), 1.0, 0.0, K, C, None)
                wt.check("dot over NaN, beta = 0", dev.down(dO), wt.dot(A, B, None, 1.0, 0.0, exact=ints))
                r = np.full(C, np.nan, np.float32); o.t4o_dot(P(A), P(B), P(r), 1.0, 0.0, K, C); assert np.all(np.isnan(r))


def test_dlinear_db_accumulates_exactly_on_integers_and_within_bound_on_floats(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(45)
    for E0 in sk.DB_E0:
        for N in sk.DB_N:
            for ints in (True, False):
                DY = sk.ints(rng, (N, E0)) if ints else rng.standard_normal((N, E0)).astype(np.float32)
                DB0 = sk.ints(rng, E0) if ints else rng.standard_normal(E0).astype(np.float32)
                w = wt.W(DY.astype(np.float64).sum(0) + DB0, 0.0, 0) if ints else wt.dlinear_db(DY, DB0)
                for off in (0, 1):
                    t, ptr = up_off(dev, DY, off); dDB = dev.up(DB0)
                    t4k.call("t4k_dlinear_db", ptr, p(dDB), N, E0, None)
                    wt.check("dlinear_db N=%d E0=%d off=%d" % (N, E0, off), dev.down(dDB), w, kind="dlinear_db (integer)" if ints else "dlinear_db")
                r = DB0.copy(); o.t4o_dlinear_db(P(DY), P(r), N, E0); wt.check("oracle dlinear_db", r, w)


# ----------------------------------------------------------------------------- softmax, log-softmax
def test_softmax_rows(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(46)
    for C in sk.SOFTMAX_C:
        for N in sk.SOFTMAX_N:
            Z = sk.softmax_rows(rng, N, C); w = wt.softmax(Z)
            d = dev.zeros((N, C)); t4k.call("t4k_softmax", p(dev.up(Z)), p(d), N, C, None); g = dev.down(d)
            wt.check("softmax N=%d C=%d" % (N, C), g, w, kind="softmax")
            y = np.zeros_like(Z); o.t4o_softmax(P(Z), P(y), N, C); wt.check("oracle softmax", y, w)
            assert np.all(np.abs(g.astype(np.float64).sum(1) - 1.0) <= C * wt.U), (N, C)     # rows sum to 1: the stored terms over their own fp32 sum (C - 1 roundings) and one rounding of each quotient
            assert relx(g, y) < RTOL


def test_logsoftmax_rows(t4k, dev, oracle):
    rng = np.random.default_rng(47)
    for N, C in sk.LOGSOFTMAX_NC:
        X = (rng.standard_normal((N, C)) * 2).astype(np.float32); X[0] = -40.0
        if N > 2:
            X[2] = 80.0 - np.log(C)                                     # the largest row sum below the exp overflow the sweep asks for
        d = dev.zeros((N, C)); t4k.call("t4k_logsoftmax", p(dev.up(X)), p(d), N, C, None)
        wt.check("logsoftmax N=%d C=%d" % (N, C), dev.down(d), wt.logsoftmax(X), kind="logsoftmax")


# ----------------------------------------------------------------------------- batch norm
def _bn_case(t4k, dev, oracle, rows, C, mean=0.0, off=0, sync=False, ints=False, train=1, seed=48):
    o = oracle.lib(); P = oracle.P
    N, HW = sk.bn_split(rows)
    rng = np.random.default_rng(seed + rows + C)
    x = sk.ints(rng, (rows, C)) if ints else sk.bn_input(rng, rows, C, mean)
    g = rng.standard_normal(C).astype(np.float32); b = rng.standard_normal(C).astype(np.float32)
    gy = sk.ints(rng, (rows, C)) if ints else rng.standard_normal((rows, C)).astype(np.float32)
    DW0 = rng.standard_normal(C).astype(np.float32); DB0 = rng.standard_normal(C).astype(np.float32)
    name = "bn %dx%d mean=%g off=%d%s" % (rows, C, mean, off, " sync" if sync else "")
    # oracle
    y = np.zeros_like(x); xh = np.zeros_like(x); stat = np.zeros(3 * C, np.float32)
    o.t4o_batchnorm_fwd(P(x), P(y), P(xh), P(g), P(b), P(stat), N, HW, C)
    wm, wr = wt.bn_stats(x)
    wt.check("oracle mean " + name, stat[C:2 * C], wm); wt.check("oracle rstd " + name, stat[:C], wr)
    wt.check("oracle xhat " + name, xh, wt.bn_xhat(x, stat)); wt.check("oracle y " + name, y, wt.bn_y(xh, g, b))
    # product
    tx, px = up_off(dev, x, off); ty, py = up_off(dev, y * 0, off); txh, pxh = up_off(dev, y * 0, off)
    dg, db, dst = dev.up(g), dev.up(b), dev.zeros(3 * C)
    l0 = launches(t4k)
    t4k.call("t4k_batchnorm_fwd", px, py, pxh, p(dg), p(db), p(dst), N, HW, C, None)
    if not sync:
        assert launches(t4k) - l0 == (2 if rows < sk.BN_CHUNKED_ROWS else 3), name       # stats + apply, or column sums + fold + apply
    gst = dev.down(dst).copy(); gxh = dn_off(dev, txh, off, x.shape); gyy = dn_off(dev, ty, off, x.shape)
    wt.check("mean " + name, gst[C:2 * C], wm, kind="bn mean"); wt.check("rstd " + name, gst[:C], wr, kind="bn 1/(sigma+eps)")
    wt.check("xhat " + name, gxh, wt.bn_xhat(x, gst), kind="bn xhat"); wt.check("y " + name, gyy, wt.bn_y(gxh, g, b), kind="bn y")
    if ints:
        isum = x.astype(np.int64).sum(0)
        assert np.array_equal(gst[C:2 * C], isum.astype(np.float32) / np.float32(rows)), name          # integer column sums: exact in any order, one rounding in the division
    if mean == 0.0 and not ints:
        assert relx(gyy, y, rows) < RTOL and relx(gxh, xh, rows) < RTOL                  # the earlier bar, beside the witness
    # backward, on the product's own xhat / stats (and the oracle on its own)
    DX = np.zeros_like(x); DW = DW0.copy(); DB = DB0.copy()
    o.t4o_batchnorm_bwd(P(g), P(gy), P(xh), P(DX), P(DW), P(DB), P(stat), N, HW, C, train)
    w1, w2, wdw, wdb = wt.bn_bwd_stats(gy, xh, DW0, DB0, train)
    wt.check("oracle s1 " + name, stat[C:2 * C], w1); wt.check("oracle s2 " + name, stat[2 * C:], w2)
    wt.check("oracle dW " + name, DW, wdw); wt.check("oracle dB " + name, DB, wdb); wt.check("oracle dx " + name, DX, wt.bn_dx(g, gy, xh, stat))
    tgy, pgy = up_off(dev, gy, off); tdx, pdx = up_off(dev, y * 0, off); dDW, dDB = dev.up(DW0), dev.up(DB0)
    l0 = launches(t4k)
    t4k.call("t4k_batchnorm_bwd", p(dg), pgy, pxh, pdx, p(dDW), p(dDB), p(dst), N, HW, C, train, None)
    if not sync:
        assert launches(t4k) - l0 == (2 if rows < sk.BN_CHUNKED_ROWS else 3), name
    gst2 = dev.down(dst).copy(); gdx = dn_off(dev, tdx, off, x.shape)
    w1, w2, wdw, wdb = wt.bn_bwd_stats(gy, gxh, DW0, DB0, train)
    wt.check("s1 " + name, gst2[C:2 * C], w1, kind="bn mean dy"); wt.check("s2 " + name, gst2[2 * C:], w2, kind="bn mean dy*xhat")
    wt.check("dW " + name, dev.down(dDW), wdw, kind="bn dW/dB"); wt.check("dB " + name, dev.down(dDB), wdb, kind="bn dW/dB")
    wt.check("dx " + name, gdx, wt.bn_dx(g, gy, gxh, gst2), kind="bn dx")
    assert np.array_equal(gst2[:C], gst[:C])                                             # 1 / (sigma + eps) is the forward's
    if ints:
        assert np.array_equal(gst2[C:2 * C], gy.astype(np.int64).sum(0).astype(np.float32) / np.float32(rows)), name


@pytest.mark.parametrize("rows,C", sk.BN_SHAPES)
@pytest.mark.parametrize("train", [1, 0])
def test_batchnorm_at_the_chunking_edges(t4k, dev, oracle, rows, C, train):
    """2047 | 2048 rows: one-launch statistics | chunked column sums; ragged last chunks (2049 = 8 x 257 rows but for the last, 4099, 10 007), a
    chunk length off the 4 row groups' multiple, the 2048-chunk cap (540 672 rows), C = 1, 3 (< 4), 4, 64, 65, 70, 130 (partial 64-channel slabs)"""
    if rows >= sk.BN_CHUNKED_ROWS:
        nch, rpc = sk.bn_plan(rows); assert nch <= sk.BN_MAX_CHUNKS and (nch - 1) * rpc < rows <= nch * rpc
    _bn_case(t4k, dev, oracle, rows, C, train=train)


@pytest.mark.parametrize("rows,C", sk.BN_MEAN_SHAPES)
@pytest.mark.parametrize("mean", sk.BN_MEANS[1:])
def test_batchnorm_with_an_offset_mean(t4k, dev, oracle, rows, C, mean):
    """mean = 1 and 8 sigma: E[x^2] - mean^2 cancels 65-fold, and the witness's bound for 1 / (sigma + eps) grows with it (tests/test_f64_witness.py)"""
    _bn_case(t4k, dev, oracle, rows, C, mean=mean)


@pytest.mark.parametrize("rows,C", [(4099, 64), (2049, 4), (392, 130)])
def test_batchnorm_from_a_four_byte_offset_base(t4k, dev, oracle, rows, C):
    """C % 4 == 0 on a base that is not 16-byte aligned: launch_bn_part takes the scalar k_bn_part"""
    _bn_case(t4k, dev, oracle, rows, C, off=1)


@pytest.mark.parametrize("rows,C", [(2049, 4), (4099, 65), (540672, 4), (392, 130)])
def test_batchnorm_column_sums_exact_on_integer_operands(t4k, dev, oracle, rows, C):
    _bn_case(t4k, dev, oracle, rows, C, ints=True)
    _bn_case(t4k, dev, oracle, rows, C, ints=True, off=1)


@pytest.mark.parametrize("rows,C", sk.BN_SYNC_SHAPES)
def test_batchnorm_synchronised_statistics_world_one_at_ragged_chunks(t4k, dev, oracle, rows, C):
    lib = t4k.lib
    raw = (ctypes.c_ubyte * 128)()
    assert lib.t4k_comm_unique_id(raw) == 0 and lib.t4k_comm_init(raw, 0, 1) == 0, lib.t4k_last_error()
    try:
        assert lib.t4k_comm_sync_batchnorm(1) == 0
        _bn_case(t4k, dev, oracle, rows, C, sync=True)
        _bn_case(t4k, dev, oracle, rows, C, sync=True, ints=True)
    finally:
        lib.t4k_comm_destroy()


# ----------------------------------------------------------------------------- element-wise, activations, copies
EXACT_MATH = ("ABS", "NEG", "RELU", "SAT", "FILL", "SCALE", "ADD", "SUB", "MUL", "DIV", "SQRT", "RCP")


def test_elementwise_vector_and_scalar_paths_at_the_grid_stride(t4k, dev, oracle):
    """k_math / k_ts / k_tt (with the second destination) / k_copy: 16-byte aligned and 4-byte-offset bases, n across the float4 tail and across
    grid_for(n, 4)'s stride.  Single IEEE operations: bit-equal to the oracle.  The largest sizes run one op per kernel template."""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(49)
    for n in sk.EW_N:
        big = n > 100000
        x = rng.uniform(0.1, 2.0, n).astype(np.float32); y = rng.uniform(0.5, 2.0, n).astype(np.float32)
        for off in (0, 1):
            for name in (("ABS", "SCALE", "SQRT") if big else EXACT_MATH):
                op = getattr(oracle, name); a = (x - 1.0).copy() if name in ("ABS", "NEG", "RELU", "SAT") else x.copy()
                t, ptr = up_off(dev, a, off); o.t4o_math(op, P(a), 1.5, n)
                t4k.call("t4k_math", op, ptr, 1.5, n, None)
                g = dev.down(t); assert np.array_equal(g[off:off + n], a), (name, n, off)
                assert not g[:off].any() and not g[off + n:].any(), (name, n, off)                 # nothing written outside
            for name in (("EXP", "GFILL") if big else ("EXP", "LN", "LOG", "TANH", "SIGM", "POW", "GFILL")):
                op = getattr(oracle, name); a = x.copy(); t, ptr = up_off(dev, a, off); o.t4o_math(op, P(a), 1.5, n)
                t4k.call("t4k_math", op, ptr, 1.5, n, None)
                assert relx(dev.down(t)[off:off + n], a) < RTOL, (name, n, off)
            for name in (("MUL",) if big else ("ADD", "SUB", "MUL", "DIV")):
                op = getattr(oracle, name); r = np.zeros_like(x); o.t4o_tt_op(op, P(x), P(y), P(r), n)
                (tx, px), (ty, py), (tr, pr), (t2, p2) = up_off(dev, x, off), up_off(dev, y, off), up_off(dev, r * 0, off), up_off(dev, r * 0, off)
                t4k.call("t4k_tt_op2", op, px, py, pr, p2, n, None)
                g, g2 = dev.down(tr), dev.down(t2)
                assert np.array_equal(g[off:off + n], r) and np.array_equal(g2, g) and not g[off + n:].any(), (name, n, off)
                t4k.call("t4k_tt_op", op, px, py, pr, n, None); assert np.array_equal(dev.down(tr)[off:off + n], r)
                o.t4o_ts_op(op, P(x), 0.3, P(r), n); t4k.call("t4k_ts_op", op, px, 0.3, pr, n, None)
                g = dev.down(tr); assert np.array_equal(g[off:off + n], r) and not g[off + n:].any(), (name, n, off)
            (tx, px), (tc, pc) = up_off(dev, x, off), up_off(dev, x * 0, off)
            t4k.call("t4k_copy", px, pc, n, None); assert np.array_equal(dev.down(tc), dev.down(tx))
            tc2, pc2 = up_off(dev, x * 0, 1 - off); t4k.call("t4k_copy", px, pc2, n, None)         # mixed alignment: source and destination differ
            assert np.array_equal(dn_off(dev, tc2, 1 - off, n), x)


def test_copy_mask_bias_and_broadcast_rows_at_the_grid_stride(t4k, dev, oracle):
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(50)
    for n in (1, 3, 1023, 1025, sk.GRID1_STRIDE_N, sk.GRID1_STRIDE_N + 3, 3000001):
        T = rng.standard_normal(n).astype(np.float32); M = (rng.random(n) < 0.5).astype(np.float32) * np.float32(0.75)
        for off in (0, 1):
            (tT, pT), (tM, pM), (tO, pO), (tI, pI) = up_off(dev, T, off), up_off(dev, M, off), up_off(dev, T * 0, off), up_off(dev, T * 0, off)
            t4k.call("t4k_copy_mask", pT, pM, pO, pI, n, None)
            assert np.array_equal(dn_off(dev, tO, off, n), T)
            wt.check("copy_mask n=%d" % n, dn_off(dev, tI, off, n), wt.mul(T, M), kind="copy_mask"); assert np.array_equal(dn_off(dev, tI, off, n), T * M)
    for N, E in ((1, 1), (3, 1), (257, 65), (4099, 130), (3, 1000001)):
        Y = rng.standard_normal((N, E)).astype(np.float32); b = rng.standard_normal(E).astype(np.float32)
        for off in (0, 1):
            tY, pY = up_off(dev, Y, off); r = Y.copy(); o.t4o_bias(P(b), P(r), N, E)
            t4k.call("t4k_bias", p(dev.up(b)), pY, N, E, None); assert np.array_equal(dn_off(dev, tY, off, Y.shape), r)
            t = rng.standard_normal(N).astype(np.float32); tO, pO = up_off(dev, Y * 0, off)
            t4k.call("t4k_broadcast_rows", p(dev.up(t)), pO, N, E, None)
            assert np.array_equal(dn_off(dev, tO, off, Y.shape), np.repeat(t[:, None], E, 1))


def test_activations_vector_and_scalar_paths(t4k, dev, oracle):
    """k_activate on aligned and 4-byte-offset bases: masks of relu / dropout bit-equal to the oracle, everything against wt.act"""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(51)
    kinds = (("relu", oracle.L_RELU, 0.0), ("tanh", oracle.L_TANH, 0.0), ("sigmoid", oracle.L_SIGMOID, 0.0), ("selu", oracle.L_SELU, 0.0),
             ("leaky", oracle.L_LEAKYRL, 0.01), ("elu", oracle.L_ELU, 1.0), ("dropout", oracle.L_DROPOUT, 0.5))
    for n in sk.EW_N:
        x = (rng.standard_normal(n) * 3).astype(np.float32); u = rng.random(n).astype(np.float32)
        for kind, L, alpha in (kinds if n < 100000 else (kinds[0], kinds[2], kinds[6])):
            y = np.zeros_like(x); f = u.copy(); o.t4o_activate(L, P(x), P(y), P(f), alpha, n)
            wo, wm = wt.act(kind, x, alpha, u)
            wt.check("oracle %s" % kind, y, wo); wt.check("oracle %s mask" % kind, f, wm)
            for off in (0, 1):
                (tx, px), (ty, py), (tf, pf) = up_off(dev, x, off), up_off(dev, x * 0, off), up_off(dev, u, off)
                t4k.call("t4k_activate", L, px, py, pf, alpha, n, None)
                gy, gf = dn_off(dev, ty, off, n), dn_off(dev, tf, off, n)
                wt.check("%s n=%d off=%d" % (kind, n, off), gy, wo, kind="activation"); wt.check("%s mask n=%d off=%d" % (kind, n, off), gf, wm, kind="activation")
                if kind in ("relu", "dropout"):
                    assert np.array_equal(gy, y) and np.array_equal(gf, f)
                assert not dev.down(ty)[off + n:].any()


def test_transpose_edge_tiles(t4k, dev):
    rng = np.random.default_rng(52)
    for H, W, C in sk.TRANSPOSE_HWC:
        a = rng.standard_normal((H, W, C)).astype(np.float32); t = dev.zeros((W, H, C))
        t4k.call("t4k_transpose", p(dev.up(a)), p(t), H, W, C, None)
        assert np.array_equal(dev.down(t), a.transpose(1, 0, 2))


# ----------------------------------------------------------------------------- optimizers
def _opt_inputs(rng, n):
    return (rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 0.1).astype(np.float32),
            (np.abs(rng.standard_normal(n)) * 0.1).astype(np.float32))


def _opt_witness(kind, w, g, m, v):
    if kind == "sgd0": return wt.sgd(w, g, m, 3, 0.01, 0.0) + (None,)
    if kind == "sgdm": return wt.sgd(w, g, m, 2, 0.01, 0.9) + (None,)
    if kind == "adam": return wt.adam(w, g, m, v, 1e-3, 0.9, 0.999)
    return wt.adamw(w, g, m, v, 1e-3, 0.9, 0.999, 0.01)


def _opt_oracle(oracle, kind, W, G, M, V):
    o = oracle.lib(); P = oracle.P; n = W.size
    if kind == "sgd0": o.t4o_sgd(P(W), P(G), P(M), 3, 0.01, 0.0, n)
    elif kind == "sgdm": o.t4o_sgd(P(W), P(G), P(M), 2, 0.01, 0.9, n)
    elif kind == "adam": o.t4o_adam(P(W), P(G), P(M), P(V), 1e-3, 0.9, 0.999, n)
    else: o.t4o_adamw(P(W), P(G), P(M), P(V), 1e-3, 0.9, 0.999, 0.01, n)


def _opt_check(name, kind, got, orc, ws, ini):
    """got / orc = (w, g, m, v) after the step; ws = witnesses (w, m, v); ini = the inputs"""
    ww, wm, wv = ws
    for who, (W, G, M, V) in (("", got), ("oracle ", orc)):
        wt.check(who + name + " w", W, ww, kind=None if who else "optimizer w")
        if wm is not None: wt.check(who + name + " m", M, wm, kind=None if who else "optimizer m/v")
        else: assert np.array_equal(M, ini[2])                                              # plain SGD leaves the momentum tensor alone
        if wv is not None: wt.check(who + name + " v", V, wv, kind=None if who else "optimizer m/v")
        assert not G.any(), name                                                             # gradient zeroed: exact
    assert np.array_equal(got[2], orc[2]) and np.array_equal(got[3], orc[3]), name           # the existing bit-equality to the oracle, kept
    if kind in ("sgd0", "sgdm"):
        assert np.array_equal(got[0], orc[0]), name
    else:
        assert rel(got[0], orc[0]) < 1e-6, name


@pytest.mark.parametrize("kind", ["sgd0", "sgdm", "adam", "adamw"])
def test_optimizer_steps_across_the_grid_stride(t4k, dev, oracle, kind):
    rng = np.random.default_rng(53)
    for n in sk.OPT_N:
        ini = _opt_inputs(rng, n); W, G, M, V = (a.copy() for a in ini)
        _opt_oracle(oracle, kind, W, G, M, V)
        dW, dG, dM, dV = (dev.up(a) for a in ini)
        if kind == "sgd0": t4k.call("t4k_sgd", p(dW), p(dG), p(dM), 3, 0.01, 0.0, n, None)
        elif kind == "sgdm": t4k.call("t4k_sgd", p(dW), p(dG), p(dM), 2, 0.01, 0.9, n, None)
        elif kind == "adam": t4k.call("t4k_adam", p(dW), p(dG), p(dM), p(dV), 1e-3, 0.9, 0.999, n, None)
        else: t4k.call("t4k_adamw", p(dW), p(dG), p(dM), p(dV), 1e-3, 0.9, 0.999, 0.01, n, None)
        _opt_check("%s n=%d" % (kind, n), kind, tuple(dev.down(t) for t in (dW, dG, dM, dV)), (W, G, M, V), _opt_witness(kind, *ini), ini)


def test_optimizer_tables_chunked_and_multi(t4k, dev, oracle):
    """t4k_opt_chunked with tensors around the 1024-element chunk in one table (SGD with momentum, Nw per tensor); t4k_opt_multi (Adam) with
    max_n above 65 536 (its 256-workgroup cap strides)"""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(54)
    bufs = []; recs = b""; chunk = 0
    for i, sz in enumerate(sk.OPT_CHUNKED_SIZES):
        ini = _opt_inputs(rng, sz); W, G, M, V = (a.copy() for a in ini); Nw = 1 + i % 3
        o.t4o_sgd(P(W), P(G), P(M), Nw, 0.01, 0.9, sz)
        dW, dG, dM = dev.up(ini[0]), dev.up(ini[1]), dev.up(ini[2])
        bufs.append((dW, dG, dM, (W, G, M, V), ini, Nw))
        recs += struct.pack("<QQQQqii", p(dW), p(dG), p(dM), p(dM), sz, Nw, chunk); chunk += (sz + 1023) // 1024
    tab = dev.up(np.frombuffer(recs, np.uint8))
    t4k.call("t4k_opt_chunked", 0, p(tab), len(bufs), chunk, 0.01, 0.9, 0.0, 0.0, None)
    for dW, dG, dM, orc, ini, Nw in bufs:
        ww, wm = wt.sgd(ini[0], ini[1], ini[2], Nw, 0.01, 0.9)
        got = (dev.down(dW), dev.down(dG), dev.down(dM), ini[3])
        _opt_check("chunked n=%d" % ini[0].size, "sgdm", got, orc, (ww, wm, None), ini)
    bufs = []; recs = b""
    for sz in sk.OPT_MULTI_SIZES:
        ini = _opt_inputs(rng, sz); W, G, M, V = (a.copy() for a in ini)
        o.t4o_adam(P(W), P(G), P(M), P(V), 1e-3, 0.9, 0.999, sz)
        d = tuple(dev.up(a) for a in ini); bufs.append((d, (W, G, M, V), ini))
        recs += struct.pack("<QQQQqii", p(d[0]), p(d[1]), p(d[2]), p(d[3]), sz, 1, 0)
    tab = dev.up(np.frombuffer(recs, np.uint8))
    t4k.call("t4k_opt_multi", 1, p(tab), len(bufs), max(sk.OPT_MULTI_SIZES), 1e-3, 0.9, 0.999, 0.0, None)
    for d, orc, ini in bufs:
        _opt_check("multi n=%d" % ini[0].size, "adam", tuple(dev.down(t) for t in d), orc, wt.adam(*ini, 1e-3, 0.9, 0.999), ini)


# ----------------------------------------------------------------------------- linear algebra
@pytest.mark.parametrize("K", sk.LINALG_K)
def test_linear_algebra_by_residual(t4k, dev, oracle, K):
    """inverse (Gauss-Jordan) and lu_inverse by |A X - I|, plu by |P A - L U|, logdet on the stored factors; pivots, status and lu_extract
    bit-equal to the oracle.  K across the 256-lane trip of the column loops; a matrix that swaps at every column; cond ~ 1e4."""
    o = oracle.lib(); P = oracle.P
    rng = np.random.default_rng(55 + K)
    eye = np.eye(K, dtype=np.float32)
    for kind in sk.LINALG_KINDS:
        A = sk.matrix(rng, K, kind); name = "K=%d %s" % (K, kind)
        a, I = A.copy(), eye.copy(); st = ctypes.c_int(0); o.t4o_inverse(P(a), P(I), K, ctypes.byref(st)); assert st.value == 0
        wt.inverse_check("oracle inverse " + name, A, I)
        dA, dI, dst = dev.up(A), dev.up(eye), dev.zeros(1, dev.torch.int32)
        t4k.call("t4k_inverse", p(dA), p(dI), K, p(dst), None)
        assert dev.down(dst)[0] == 0; wt.inverse_check("inverse " + name, A, dev.down(dI), kind="inverse residual")
        a, I, piv = A.copy(), eye.copy(), np.zeros(K, np.int32); o.t4o_plu(P(a), P(I), P(piv), K, ctypes.byref(st)); assert st.value == 0
        wt.plu_check("oracle plu " + name, A, a, piv)
        if kind == "permuted" and K > 1:
            assert np.all(piv[:-1] != np.arange(K - 1)), "the permuted matrix swaps at every column"
        dA, dI, dpiv = dev.up(A), dev.up(eye), dev.zeros(K, dev.torch.int32)
        t4k.call("t4k_plu", p(dA), p(dI), p(dpiv), K, p(dst), None)
        gpiv, gLU = dev.down(dpiv), dev.down(dA)
        assert dev.down(dst)[0] == 0 and np.array_equal(gpiv, piv), name
        wt.plu_check("plu " + name, A, gLU, gpiv, kind="plu residual")
        assert np.array_equal(dev.down(dI), eye[wt.perm_of(gpiv)]) and np.array_equal(I, eye[wt.perm_of(piv)])           # I leaves as P
        wl, sg = wt.logdet(gLU); dld, dsg = dev.zeros(1), dev.zeros(1, dev.torch.int32)
        t4k.call("t4k_logdet", p(dA), K, p(dld), p(dsg), None)
        wt.check("logdet " + name, dev.down(dld), wl, kind="logdet"); assert dev.down(dsg)[0] == sg
        ld = np.zeros(1, np.float32); sgo = ctypes.c_int(0); o.t4o_logdet(P(a), K, P(ld), ctypes.byref(sgo))
        wt.check("oracle logdet " + name, ld, wt.logdet(a)[0]); assert sgo.value == wt.logdet(a)[1]
        s64, l64 = np.linalg.slogdet(A.astype(np.float64)); par = -1 if np.count_nonzero(gpiv != np.arange(K)) % 2 else 1
        assert sg * par == s64 and abs(float(dev.down(dld)[0]) - l64) <= 1e-3 * max(1.0, abs(l64)), name     # and the determinant it stands for
        for get_u in (0, 1):
            d = dev.up(gLU); t4k.call("t4k_lu_extract", p(d), get_u, K, None); wt.equal("lu_extract", dev.down(d), wt.lu_extract(gLU, get_u).exact)
            ref = gLU.copy(); o.t4o_lu_extract(P(ref), get_u, K); assert np.array_equal(dev.down(d), ref)
        a, I, piv2 = A.copy(), eye.copy(), np.zeros(K, np.int32); o.t4o_lu_inverse(P(a), P(I), P(piv2), K, ctypes.byref(st)); assert st.value == 0
        wt.inverse_check("oracle lu_inverse " + name, A, I, piv2)
        dA, dI, dpiv = dev.up(A), dev.up(eye), dev.zeros(K, dev.torch.int32)
        t4k.call("t4k_lu_inverse", p(dA), p(dI), p(dpiv), K, p(dst), None)
        assert dev.down(dst)[0] == 0 and np.array_equal(dev.down(dpiv), piv2), name
        wt.inverse_check("lu_inverse " + name, A, dev.down(dI), dev.down(dpiv), kind="lu_inverse residual")
    for kind, want in (("singular_last", K), ("singular_first", 1)):                       # a status, not a fault
        A = sk.matrix(rng, K, kind); st = ctypes.c_int(0); a, I = A.copy(), eye.copy(); o.t4o_inverse(P(a), P(I), K, ctypes.byref(st))
        dst = dev.zeros(3, dev.torch.int32); dpiv = dev.zeros(K, dev.torch.int32)
        t4k.call("t4k_inverse", p(dev.up(A)), p(dev.up(eye)), K, p(dst), None)
        t4k.call("t4k_plu", p(dev.up(A)), p(dev.up(eye)), p(dpiv), K, p(dst) + 4, None)
        t4k.call("t4k_lu_inverse", p(dev.up(A)), p(dev.up(eye)), p(dpiv), K, p(dst) + 8, None)
        assert tuple(dev.down(dst)) == (want, want, want) and st.value == want, (K, kind)


# ----------------------------------------------------------------------------- transposed convolution
@pytest.mark.parametrize("N,H1,W1,C1,C0", sk.DCONV_SHAPES)
def test_transposed_conv_against_float64(t4k, dev, oracle, N, H1, W1, C1, C0):
    o = oracle.lib(); P = oracle.P
    K, S, Pd = 4, 2, 1
    H0, W0 = wt.dconv_out(H1), wt.dconv_out(W1)
    rng = np.random.default_rng(56 + N * 100 + C0)
    I = rng.standard_normal((N, H1, W1, C1)).astype(np.float32); F = (rng.standard_normal((C1, K, K, C0)) * 0.2).astype(np.float32)
    B = rng.standard_normal(C0).astype(np.float32); G = rng.standard_normal((N, H0, W0, C0)).astype(np.float32)
    name = "dconv %dx%dx%dx%d->%d" % (N, H1, W1, C1, C0)
    O = np.zeros((N, H0, W0, C0), np.float32)
    assert o.t4o_dconv2d_fwd(P(I), P(O), P(F), P(B), N, H1, W1, C1, H0, W0, C0, K, S, Pd) == 0
    w = wt.dconv_fwd(I, F, B, H0, W0); wt.check("oracle fwd " + name, O, w)
    dI, dF, dB, dO, dG = dev.up(I), dev.up(F), dev.up(B), dev.zeros(O.shape), dev.up(G)
    t4k.call("t4k_dconv2d_fwd", p(dI), p(dO), p(dF), p(dB), N, H1, W1, C1, H0, W0, C0, K, S, Pd, None)
    wt.check("fwd " + name, dev.down(dO), w, kind="dconv fwd")
    DX = np.zeros_like(I); DF = np.full_like(F, 0.25); DB = np.full_like(B, -0.5)
    dDX, dDF, dDB = dev.up(np.full_like(I, 3.0)), dev.up(DF), dev.up(DB)
    for rep in range(2):                                                    # DF / DB accumulate over two calls: each call witnessed on what it started from
        DF0, DB0 = DF.copy(), DB.copy(); gDF0, gDB0 = dev.down(dDF).copy(), dev.down(dDB).copy()
        assert o.t4o_dconv2d_bwd(P(I), P(G), P(DX), P(F), P(DF), P(DB), N, H1, W1, C1, H0, W0, C0, K, S, Pd, 1) == 0
        wdx, wdf, wdb = wt.dconv_bwd(I, G, F, DF0, DB0)
        wt.check("oracle dX " + name, DX, wdx); wt.check("oracle dF " + name, DF, wdf); wt.check("oracle dB " + name, DB, wdb)
        t4k.call("t4k_dconv2d_bwd", p(dI), p(dG), p(dDX), p(dF), p(dDF), p(dDB), N, H1, W1, C1, H0, W0, C0, K, S, Pd, 1, None)
        wdx, wdf, wdb = wt.dconv_bwd(I, G, F, gDF0, gDB0)
        wt.check("dX " + name, dev.down(dDX), wdx, kind="dconv dX"); wt.check("dF " + name, dev.down(dDF), wdf, kind="dconv dF"); wt.check("dB " + name, dev.down(dDB), wdb, kind="dconv dB")


def test_zz_report_worst_ratios():
    """the worst |error| / bound the sweep saw per op kind (pytest -s prints it; tests/README.md quotes it)"""
    print("\nsmall-kernel sweep, worst |err| / bound per op kind:")
    for kind in sorted(wt.WORST):
        print("  %-40s %.3g   %s" % (kind, wt.WORST[kind][0], wt.WORST[kind][1]))
    assert all(r <= 1.0 for k, (r, _) in wt.WORST.items() if "measured" not in k)
