"""t4k_inverse_batched / t4k_plu_batched / t4k_lu_inverse_batched / t4k_lu_extract_batched / t4k_det_batched (include/t4k.h) through the C ABI:
every regime of csrc/linalg_batched.hip and both sides of every regime boundary (wave K <= 32, workgroup K <= 140 with A and X in LDS and
K <= 200 with A alone, global above), batches of 1, 2, 7 and 128 entries that cycle through the matrix kinds of tests/small_kernel_cases.py so a
batch mixes pivot patterns.  Every entry is held to the float64 witnesses of tests/f64_witness.py with the bars the per-matrix kernels are
held to (tests/test_gpu_small_kernels_sweep.py), every call to exactly one kernel launch."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt
import small_kernel_cases as sk
from test_gpu_parity import Dev, p

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 16, 31, 32, 33, 64, 100, 140, 141, 200, 201, 257, 300)
BATCHES = (1, 2, 7, 128)
KINDS = ("dominant", "permuted", "cond1e4")
CASES = [(K, b) for K in KS for b in BATCHES if K < 257 or b <= 7]
ERR_ARG, ERR_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


def one_launch(t4k, name, *args):
    l0 = int(t4k.lib.t4k_launch_count())
    t4k.call(name, *args)
    assert int(t4k.lib.t4k_launch_count()) - l0 == 1, name


def make_batch(rng, K, batch, kinds=KINDS, first=0):
    ks = [kinds[(first + i) % len(kinds)] for i in range(batch)]
    return ks, np.stack([sk.matrix(rng, K, k) for k in ks])


def oracle_plu(oracle, A):
    K = A.shape[0]; a, I, piv, st = A.copy(), np.eye(K, dtype=np.float32), np.zeros(K, np.int32), ctypes.c_int(0)
    oracle.lib().t4o_plu(oracle.P(a), oracle.P(I), oracle.P(piv), K, ctypes.byref(st))
    return piv, st.value


def check_plu_entry(oracle, name, kind, A, LU, piv, Pm=None):
    K = A.shape[0]
    wt.plu_check("plu " + name, A, LU, piv, kind="batched plu residual")
    if kind in ("dominant", "permuted"):
        opiv, ost = oracle_plu(oracle, A)
        assert ost == 0 and np.array_equal(piv, opiv), name
    if Pm is not None:
        assert np.array_equal(Pm, np.eye(K, dtype=np.float32)[wt.perm_of(piv)]), name


@pytest.mark.parametrize("K,batch", CASES)
def test_inverse_and_lu_inverse(t4k, dev, oracle, K, batch):
    rng = np.random.default_rng(1000 + K * 131 + batch)
    kinds, A = make_batch(rng, K, batch, first=K)
    dA, dX, dst = dev.up(A), dev.up(np.full_like(A, 7.0)), dev.up(np.full(batch, -9, np.int32))       # X is a pure output: no identity handed in
    one_launch(t4k, "t4k_inverse_batched", p(dA), p(dX), K, batch, p(dst), None)
    X, st = dev.down(dX), dev.down(dst)
    assert not st.any(), st
    for n in range(batch):
        wt.inverse_check("inverse K=%d b=%d/%d %s" % (K, n, batch, kinds[n]), A[n], X[n], kind="batched inverse residual")
    dA, dX, dst, dpiv = dev.up(A), dev.up(np.full_like(A, 7.0)), dev.up(np.full(batch, -9, np.int32)), dev.zeros(batch * K, dev.torch.int32)
    one_launch(t4k, "t4k_lu_inverse_batched", p(dA), p(dX), p(dpiv), K, batch, p(dst), None)
    X, st, piv, LU = dev.down(dX), dev.down(dst), dev.down(dpiv).reshape(batch, K), dev.down(dA)
    assert not st.any(), st
    for n in range(batch):
        name = "lu_inverse K=%d b=%d/%d %s" % (K, n, batch, kinds[n])
        wt.inverse_check(name, A[n], X[n], piv[n], kind="batched lu_inverse residual")
        check_plu_entry(oracle, name, kinds[n], A[n], LU[n], piv[n])


@pytest.mark.parametrize("K,batch", CASES)
def test_plu_and_lu_extract(t4k, dev, oracle, K, batch):
    rng = np.random.default_rng(2000 + K * 131 + batch)
    kinds, A = make_batch(rng, K, batch, first=K + 1)
    dA, dP, dst, dpiv = dev.up(A), dev.up(np.full_like(A, 7.0)), dev.up(np.full(batch, -9, np.int32)), dev.zeros(batch * K, dev.torch.int32)
    one_launch(t4k, "t4k_plu_batched", p(dA), p(dP), p(dpiv), K, batch, p(dst), None)
    LU, Pm, st, piv = dev.down(dA), dev.down(dP), dev.down(dst), dev.down(dpiv).reshape(batch, K)
    assert not st.any(), st
    for n in range(batch):
        check_plu_entry(oracle, "K=%d b=%d/%d %s" % (K, n, batch, kinds[n]), kinds[n], A[n], LU[n], piv[n], Pm[n])
    dA2, dpiv2 = dev.up(A), dev.zeros(batch * K, dev.torch.int32)                                        # Pm may be NULL
    one_launch(t4k, "t4k_plu_batched", p(dA2), None, p(dpiv2), K, batch, p(dst), None)
    assert np.array_equal(dev.down(dA2), LU) and np.array_equal(dev.down(dpiv2).reshape(batch, K), piv)
    for get_u in (0, 1):
        d = dev.up(LU)
        one_launch(t4k, "t4k_lu_extract_batched", p(d), get_u, K, batch, None)
        got = dev.down(d)
        for n in range(batch):
            wt.equal("lu_extract K=%d b=%d get_u=%d" % (K, n, get_u), got[n], wt.lu_extract(LU[n], get_u).exact)


def normalised(A):
    """A / exp(logdet64 / K), rounded to fp32: |det| ~ 1 at every K, so every entry's determinant is an fp32 number and is value-checked"""
    K = A.shape[0]
    _, l64 = np.linalg.slogdet(A.astype(np.float64))
    return (A.astype(np.float64) / np.exp(l64 / K)).astype(np.float32)


def check_det_entry(name, A, LU, piv, d):
    """(a) the factors, (b) ln|det| against the witness on the stored factors widened for the expf, (c) the sign, (d) float64 on the fp32 input"""
    wt.plu_check("det factors " + name, A, LU, piv)
    assert np.isfinite(d) and d != 0.0, (name, d)
    w, _ = wt.logdet(LU); ld = float(np.log(abs(float(d))))
    bound = float(w.bound()) + (wt.ULP_EXP + 2.0 * abs(ld)) * wt.U
    r = abs(ld - float(w.exact)) / bound
    s64, l64 = np.linalg.slogdet(A.astype(np.float64))
    print("%s: det %.7g  ln|det| - witness %.3g (ratio to the bound %.3g)  ln|det| - float64 %.3g" % (name, d, ld - float(w.exact), r, ld - l64))
    assert r <= 1.0, (name, ld, float(w.exact), bound)
    assert np.sign(d) == s64, (name, d, s64)
    assert abs(ld - l64) <= 1e-3 * max(1.0, abs(l64)), (name, ld, l64)
    return r


@pytest.mark.parametrize("K,batch", CASES)
def test_det(t4k, dev, K, batch):
    rng = np.random.default_rng(3000 + K * 131 + batch)
    kinds, A = make_batch(rng, K, batch, first=K + 2)
    A = np.stack([normalised(a) for a in A])
    dA, dd, dst, dpiv = dev.up(A), dev.up(np.full(batch, 7.0, np.float32)), dev.up(np.full(batch, -9, np.int32)), dev.zeros(batch * K, dev.torch.int32)
    one_launch(t4k, "t4k_det_batched", p(dA), p(dpiv), K, batch, p(dd), p(dst), None)
    LU, d, st, piv = dev.down(dA), dev.down(dd), dev.down(dst), dev.down(dpiv).reshape(batch, K)
    assert not st.any(), st
    for n in range(batch):
        check_det_entry("K=%d b=%d/%d %s" % (K, n, batch, kinds[n]), A[n], LU[n], piv[n], d[n])


@pytest.mark.parametrize("K", KS)
def test_singular_entries_do_not_stop_the_batch(t4k, dev, oracle, K):
    """singular entries first, in the middle and last: their status is the per-matrix entry's (K for a zero last column, 1 for a zero first one),
    every other entry passes the bars, det of the singular ones is 0.  A status on valid inputs, not a fault."""
    rng = np.random.default_rng(4000 + K)
    batch = 7
    kinds = ["singular_last", "dominant", "permuted", "singular_first", "cond1e4", "dominant", "singular_last"]
    A = np.stack([sk.matrix(rng, K, k) for k in kinds])
    want = np.array([{"singular_last": K, "singular_first": 1}.get(k, 0) for k in kinds], np.int32)
    eye = np.eye(K, dtype=np.float32)
    for n in (0, 3):                                                                                       # what the per-matrix entries report
        st1 = dev.zeros(3, dev.torch.int32); dpiv1 = dev.zeros(K, dev.torch.int32)
        t4k.call("t4k_inverse", p(dev.up(A[n])), p(dev.up(eye)), K, p(st1), None)
        t4k.call("t4k_plu", p(dev.up(A[n])), p(dev.up(eye)), p(dpiv1), K, p(st1) + 4, None)
        t4k.call("t4k_lu_inverse", p(dev.up(A[n])), p(dev.up(eye)), p(dpiv1), K, p(st1) + 8, None)
        assert tuple(dev.down(st1)) == (want[n],) * 3, (K, kinds[n])
    good = [n for n in range(batch) if want[n] == 0]
    dA, dX, dst = dev.up(A), dev.zeros(A.shape), dev.up(np.full(batch, -9, np.int32))
    one_launch(t4k, "t4k_inverse_batched", p(dA), p(dX), K, batch, p(dst), None)
    assert np.array_equal(dev.down(dst), want), (dev.down(dst), want)
    X = dev.down(dX)
    for n in good:
        wt.inverse_check("inverse beside singular K=%d b=%d" % (K, n), A[n], X[n])
    dA, dX, dst, dpiv = dev.up(A), dev.zeros(A.shape), dev.up(np.full(batch, -9, np.int32)), dev.zeros(batch * K, dev.torch.int32)
    one_launch(t4k, "t4k_lu_inverse_batched", p(dA), p(dX), p(dpiv), K, batch, p(dst), None)
    assert np.array_equal(dev.down(dst), want)
    X, piv = dev.down(dX), dev.down(dpiv).reshape(batch, K)
    for n in good:
        wt.inverse_check("lu_inverse beside singular K=%d b=%d" % (K, n), A[n], X[n], piv[n])
    dA, dP, dst = dev.up(A), dev.zeros(A.shape), dev.up(np.full(batch, -9, np.int32))
    one_launch(t4k, "t4k_plu_batched", p(dA), p(dP), p(dpiv), K, batch, p(dst), None)
    assert np.array_equal(dev.down(dst), want)
    LU, Pm, piv = dev.down(dA), dev.down(dP), dev.down(dpiv).reshape(batch, K)
    for n in good:
        check_plu_entry(oracle, "plu beside singular K=%d b=%d" % (K, n), kinds[n], A[n], LU[n], piv[n], Pm[n])
    An = A.copy()
    for n in good:
        An[n] = normalised(A[n])
    dA, dd, dst = dev.up(An), dev.up(np.full(batch, 7.0, np.float32)), dev.up(np.full(batch, -9, np.int32))
    one_launch(t4k, "t4k_det_batched", p(dA), p(dpiv), K, batch, p(dd), p(dst), None)
    assert np.array_equal(dev.down(dst), want)
    LU, d, piv = dev.down(dA), dev.down(dd), dev.down(dpiv).reshape(batch, K)
    for n in range(batch):
        if want[n]:
            assert d[n] == 0.0, (K, n, d[n])
        else:
            check_det_entry("det beside singular K=%d b=%d" % (K, n), An[n], LU[n], piv[n], d[n])


def test_empty_batch_and_argument_errors(t4k, dev):
    A = dev.zeros((2, 4, 4)); X = dev.zeros((2, 4, 4)); st = dev.zeros(2, dev.torch.int32); piv = dev.zeros(8, dev.torch.int32); d = dev.zeros(2)
    L = t4k.lib
    calls = {
        "inverse": lambda K, b, a=p(A), x=p(X), s=p(st): L.t4k_inverse_batched(a, x, K, b, s, None),
        "plu": lambda K, b, a=p(A), pv=p(piv), s=p(st): L.t4k_plu_batched(a, None, pv, K, b, s, None),
        "lu_inverse": lambda K, b, a=p(A), x=p(X), pv=p(piv), s=p(st): L.t4k_lu_inverse_batched(a, x, pv, K, b, s, None),
        "lu_extract": lambda K, b, a=p(A): L.t4k_lu_extract_batched(a, 1, K, b, None),
        "det": lambda K, b, a=p(A), pv=p(piv), dd=p(d), s=p(st): L.t4k_det_batched(a, pv, K, b, dd, s, None),
    }
    for name, f in calls.items():
        l0 = int(L.t4k_launch_count())
        assert f(4, 0) == 0, name                                       # empty batch: T4K_OK, nothing launched
        assert int(L.t4k_launch_count()) == l0, name
        assert f(0, 2) == ERR_ARG and f(-3, 2) == ERR_ARG and f(4, -1) == ERR_ARG, name
        assert f(4, 2, a=None) == ERR_ARG, name
        assert f(1025, 1) == ERR_UNSUPPORTED, name
        assert int(L.t4k_launch_count()) == l0, name
    assert L.t4k_inverse_batched(p(A), None, 4, 2, p(st), None) == ERR_ARG
    assert L.t4k_inverse_batched(p(A), p(X), 4, 2, None, None) == ERR_ARG
    assert L.t4k_plu_batched(p(A), None, None, 4, 2, p(st), None) == ERR_ARG
    assert L.t4k_lu_inverse_batched(p(A), None, p(piv), 4, 2, p(st), None) == ERR_ARG
    assert L.t4k_det_batched(p(A), p(piv), 4, 2, None, p(st), None) == ERR_ARG


def test_unaligned_entries_take_the_dword_path(t4k, dev):
    """K * K % 4 != 0 puts odd entries off the 16-byte grid (covered by K = 3, 5, 31 ... above); here an even K from a base 4 bytes off it"""
    K, batch = 16, 5
    rng = np.random.default_rng(5)
    kinds, A = make_batch(rng, K, batch)
    buf = np.zeros(A.size + 8, np.float32); buf[1:1 + A.size] = A.ravel()
    dA, dX, dst = dev.up(buf), dev.zeros(A.size + 8), dev.zeros(batch, dev.torch.int32)
    assert p(dA) % 16 == 0 and p(dX) % 16 == 0
    one_launch(t4k, "t4k_inverse_batched", p(dA) + 4, p(dX) + 4, K, batch, p(dst), None)
    X = dev.down(dX)
    assert X[0] == 0.0 and not X[1 + A.size:].any()                       # nothing written outside the entries
    X = X[1:1 + A.size].reshape(A.shape)
    for n in range(batch):
        wt.inverse_check("unaligned inverse b=%d %s" % (n, kinds[n]), A[n], X[n])
