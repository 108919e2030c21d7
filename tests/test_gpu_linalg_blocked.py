"""The blocked regime of csrc/linalg_batched.hip through the four factorising t4k_*_batched entries: every case first asks
t4k_linalg_batched_plan for regime 3.  Sizes: the first blocked K (201; 193 for inverse / lu_inverse), one ragged row and column more, K % 32 == 31
(223), a K on the 16-byte path (204) and K = 1024 alone.  A batch mixes a random matrix, a row-reversed diagonally dominant one (every pivot from the far end,
across panel boundaries), one that needs no swap, and a singular one whose column 40 - inside the second panel - is exactly zero.
References are float64 NumPy on the fp32 operands; the bars are those of tests/test_gpu_linalg_batched.py restated:
  factors   |P A - L U| <= 2 K u |L||U| + K 2^-126, element by element
  inverse   |A X - I| <= 8 K u rho |A||X| + K 2^-126, rho the pivot growth of float64 elimination on A
  det       ln|det| within (K + 3) u sum|ln|u_jj|| + (4 + 2 |ln|det||) u of the stored diagonal's float64 sum, the sign and 1e-3 of float64 on A."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import Dev, p

pytestmark = pytest.mark.gpu
U, TINY, ZCOL = 2.0 ** -24, 2.0 ** -126, 40
I8 = ctypes.c_int * 8
CASES = [(201, 1), (201, 3), (202, 3), (204, 3), (223, 3), (1024, 1)]
CASES_X = [(193, 1), (193, 3), (194, 3), (204, 3), (223, 3), (1024, 1)]


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


def matrix(rng, K, kind):
    A = rng.standard_normal((K, K))
    if kind != "random":
        A += np.eye(K) * (2.0 + 3.0 * np.sqrt(K))                    # no swap needed
    if kind == "reversed":
        A = A[::-1]
    if kind == "singular":
        A[:, ZCOL] = 0.0
    return A.astype(np.float32)


def batch_of(K, batch, off=0):
    rng = np.random.default_rng(K * 10 + batch)
    kinds = [("random", "reversed", "singular", "noswap")[(i + K + off) % 4] for i in range(batch)]
    return kinds, np.stack([matrix(rng, K, k) for k in kinds])


def perm_of(piv):
    q = np.arange(len(piv))
    for k, u in enumerate(piv):
        q[[k, u]] = q[[u, k]]
    return q


def f64_pivots(A):
    """partial pivoting in float64: piv[z], -1 from the first column whose runner-up is within 1e-5 of the pivot (rounding may pick either), and
    the pivot growth max_k max|a^(k)| / max|a|"""
    a = A.astype(np.float64); K = len(a); piv = np.full(K, -1); sure = True; top0 = g = np.abs(a).max()
    for z in range(K):
        col = np.abs(a[z:, z]); u = int(np.argmax(col)); top = np.partition(col, -2)[-2:] if len(col) > 1 else [0.0, col[0]]
        sure = sure and not top[0] > top[1] * (1 - 1e-5)
        if sure:
            piv[z] = z + u
        a[[z, z + u]] = a[[z + u, z]]
        a[z + 1:, z] /= a[z, z]; a[z + 1:, z + 1:] -= np.outer(a[z + 1:, z], a[z, z + 1:]); a[z + 1:, z] = 0.0
        g = max(g, np.abs(a).max())
    return piv, g / top0


def check_factors(name, A, LU, piv):
    K = len(A)
    assert sorted(perm_of(piv)) == list(range(K)) and all(piv[z] >= z for z in range(K)), name
    want = f64_pivots(A)[0]; sure = want >= 0
    assert np.array_equal(piv[sure], want[sure]), name
    LU = LU.astype(np.float64); L, Uu = np.tril(LU, -1) + np.eye(K), np.triu(LU)
    err, bar = np.abs(A.astype(np.float64)[perm_of(piv)] - L @ Uu), 2.0 * K * U * (np.abs(L) @ np.abs(Uu)) + K * TINY
    print("%s: worst |PA - LU| / bar %.3g" % (name, float(np.max(err / bar))))
    assert np.all(err <= bar), (name, float(np.max(err / bar)))


def check_det(name, A, LU, d):
    s64, l64 = np.linalg.slogdet(A.astype(np.float64))
    dg = np.log(np.abs(np.diag(LU).astype(np.float64))); ld = float(np.log(abs(float(d)))); K = len(A)
    bound = (K + 3) * U * np.abs(dg).sum() + (K + 3) * TINY + (4.0 + 2.0 * abs(ld)) * U
    print("%s: det %.7g, ln|det| - stored %.3g (bound %.3g), - float64 %.3g" % (name, d, ld - dg.sum(), bound, ld - l64))
    assert np.isfinite(d) and abs(ld - dg.sum()) <= bound and np.sign(d) == s64 and abs(ld - l64) <= 1e-3 * max(1.0, abs(l64)), name


def blocked(t4k, entry, K, batch, aligned):
    out = I8()
    assert t4k.lib.t4k_linalg_batched_plan(entry, K, batch, aligned, out) == 0 and out[0] == 3 and out[2] == 32, list(out)
    return out[6]


def run_plu(t4k, dev, A, off=0):
    batch, K = A.shape[:2]
    buf = np.zeros(A.size + 8, np.float32); buf[off:off + A.size] = A.ravel()
    dA, dP, dpiv, dst = dev.up(buf), dev.up(np.full(A.size + 8, 7.0, np.float32)), dev.zeros(batch * K, dev.torch.int32), dev.up(np.full(batch, -9, np.int32))
    l0 = int(t4k.lib.t4k_launch_count())
    t4k.call("t4k_plu_batched", p(dA) + 4 * off, p(dP) + 4 * off, p(dpiv), K, batch, p(dst), None)
    assert int(t4k.lib.t4k_launch_count()) - l0 == 1
    return dev.down(dA), dev.down(dP), dev.down(dpiv).reshape(batch, K), dev.down(dst)


@pytest.mark.parametrize("K,batch", CASES)
def test_plu(t4k, dev, K, batch):
    assert blocked(t4k, 1, K, batch, 1) == (4 if K % 4 == 0 else 1)
    kinds, A = batch_of(K, batch)
    first = run_plu(t4k, dev, A)
    buf, Pm, piv, st = first
    assert not buf[A.size:].any()
    LU, Pm = buf[:A.size].reshape(A.shape), Pm[:A.size].reshape(A.shape)
    for n, kind in enumerate(kinds):
        name = "plu K=%d b=%d/%d %s" % (K, n, batch, kind)
        if kind == "singular":
            assert st[n] == ZCOL + 1 and piv[n, ZCOL] == -1, (name, st)
            continue
        assert st[n] == 0, (name, st)
        check_factors(name, A[n], LU[n], piv[n])
        assert np.array_equal(Pm[n], np.eye(K, dtype=np.float32)[perm_of(piv[n])]), name
    again = run_plu(t4k, dev, A)                                          # the same bits on a second call (a singular entry's A and Pm are unspecified)
    good = [n for n, kind in enumerate(kinds) if kind != "singular"]
    assert np.array_equal(again[2], piv) and np.array_equal(again[3], st)
    assert np.array_equal(again[0][:A.size].reshape(A.shape)[good], LU[good]) and np.array_equal(again[1][:A.size].reshape(A.shape)[good], Pm[good])


@pytest.mark.parametrize("K,batch", CASES)
def test_det(t4k, dev, K, batch):
    blocked(t4k, 3, K, batch, 1)
    kinds, A = batch_of(K, batch, off=1)
    for n, kind in enumerate(kinds):                                       # |det| ~ 1: the determinant is an fp32 number
        if kind != "singular":
            A[n] = (A[n].astype(np.float64) / np.exp(np.linalg.slogdet(A[n].astype(np.float64))[1] / K)).astype(np.float32)
    dA, dd, dpiv, dst = dev.up(A), dev.up(np.full(batch, 7.0, np.float32)), dev.zeros(batch * K, dev.torch.int32), dev.up(np.full(batch, -9, np.int32))
    l0 = int(t4k.lib.t4k_launch_count())
    t4k.call("t4k_det_batched", p(dA), p(dpiv), K, batch, p(dd), p(dst), None)
    assert int(t4k.lib.t4k_launch_count()) - l0 == 1
    LU, d, piv, st = dev.down(dA), dev.down(dd), dev.down(dpiv).reshape(batch, K), dev.down(dst)
    for n, kind in enumerate(kinds):
        name = "det K=%d b=%d/%d %s" % (K, n, batch, kind)
        if kind == "singular":
            assert st[n] == ZCOL + 1 and d[n] == 0.0, (name, st, d)
            continue
        assert st[n] == 0, (name, st)
        check_factors(name, A[n], LU[n], piv[n])
        check_det(name, A[n], LU[n], d[n])


def check_inverse(name, A, X):
    K = len(A); A64, X64 = A.astype(np.float64), X.astype(np.float64)
    err, bar = np.abs(A64 @ X64 - np.eye(K)), 8.0 * K * U * f64_pivots(A)[1] * (np.abs(A64) @ np.abs(X64)) + K * TINY
    print("%s: worst |AX - I| / bar %.3g" % (name, float(np.max(err / bar))))
    assert np.all(err <= bar), (name, float(np.max(err / bar)))


@pytest.mark.parametrize("K,batch", CASES_X)
@pytest.mark.parametrize("entry", ("inverse", "lu_inverse"))
def test_inverse(t4k, dev, entry, K, batch):
    blocked(t4k, 0 if entry == "inverse" else 2, K, batch, 1)
    kinds, A = batch_of(K, batch, off=3)                                    # K = 1024 alone: the matrix that needs no swap
    good = [n for n, kind in enumerate(kinds) if kind != "singular"]
    runs = []
    for _ in range(2):
        dA, dX, dpiv, dst = dev.up(A), dev.up(np.full_like(A, 7.0)), dev.zeros(batch * K, dev.torch.int32), dev.up(np.full(batch, -9, np.int32))
        l0 = int(t4k.lib.t4k_launch_count())
        if entry == "inverse":
            t4k.call("t4k_inverse_batched", p(dA), p(dX), K, batch, p(dst), None)
        else:
            t4k.call("t4k_lu_inverse_batched", p(dA), p(dX), p(dpiv), K, batch, p(dst), None)
        assert int(t4k.lib.t4k_launch_count()) - l0 == 1
        runs.append((dev.down(dX)[good], dev.down(dA)[good], dev.down(dpiv).reshape(batch, K), dev.down(dst)))
    assert all(np.array_equal(x, y) for x, y in zip(*runs))                # the same bits on a second call
    X, LU, piv, st = runs[0]
    assert list(st) == [ZCOL + 1 if kind == "singular" else 0 for kind in kinds], st
    for i, n in enumerate(good):
        name = "%s K=%d b=%d/%d %s" % (entry, K, n, batch, kinds[n])
        check_inverse(name, A[n], X[i])
        if entry == "lu_inverse":
            check_factors(name, A[n], LU[i], piv[n])


def test_a_base_four_bytes_off_takes_the_dword_path(t4k, dev):
    K, batch = 204, 2
    assert blocked(t4k, 1, K, batch, 0) == 1
    kinds, A = batch_of(K, batch, off=3)                                   # noswap, random
    buf, Pm, piv, st = run_plu(t4k, dev, A, off=1)
    assert buf[0] == 0.0 and not buf[1 + A.size:].any() and Pm[0] == 7.0 and np.all(Pm[1 + A.size:] == 7.0)   # nothing written outside the entries
    for n in range(batch):
        assert st[n] == 0
        check_factors("unaligned plu b=%d %s" % (n, kinds[n]), A[n], buf[1:1 + A.size].reshape(A.shape)[n], piv[n])
