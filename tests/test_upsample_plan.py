"""t4k_upsample_plan (include/t4k.h, csrc/upsample.hip): admission, output extents, channel vector widths and the tap table of the
up-sampling entries, on the host alone - nothing is launched and no device is needed, so these rows run wherever the library loads.

out = { H0, W0, channel vector width of the forward (4 | 1), of the backward (4 | 1) }; wt[r * 4 + a] and base[r] are the table the kernels take as an
argument.  Output row i = q K + r reads input rows clamp(q + base[r] + a, 0, H1 - 1) with weights wt[r][a]: `matrix` builds that map as My (H0 x H1), and
My X Mx^T in float64 is held against torch.nn.functional.interpolate in float64.  The bound per element is 64 * 2^-24 * sum |w| |x|: the table's weights are
floats, each within 2^-24 relative of its exact value, and a bicubic element is 16 products of two of them (with the weights kept in double the same
comparison stands at 1e-14)."""
import ctypes

import numpy as np
import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
NEAREST, LINEAR, BILINEAR, CUBIC = range(4)                              # T4K_UP_* of include/t4k.h, the reference's enum
TAPS = {NEAREST: 1, LINEAR: 2, BILINEAR: 2, CUBIC: 4}
MODE = {NEAREST: "nearest", LINEAR: "bilinear", BILINEAR: "bilinear", CUBIC: "bicubic"}
I4, F64, I16 = ctypes.c_int * 4, ctypes.c_float * 64, ctypes.c_int * 16
SHAPES = [(1, 1), (1, 5), (2, 3), (3, 2), (5, 4), (7, 6)]


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def kmax(method):
    return 8 if method == CUBIC else 16


def admitted():
    for method in range(4):
        for K in range(1, kmax(method) + 1):
            yield method, K


def plan(lib, method, N, H1, W1, C, K, aligned=3, table=True):
    out, wt, base = I4(), F64(), I16()
    rc = lib.t4k_upsample_plan(method, N, H1, W1, C, K, aligned, out, wt if table else None, base if table else None)
    return rc, list(out), np.array(wt, np.float32).reshape(16, 4), np.array(base, np.int64)


def matrix(wt, base, method, K, H1):
    """My (K H1 x H1) in float64 from the table: clamped taps add up on the border rows"""
    M = np.zeros((K * H1, H1))
    for i in range(K * H1):
        q, r = divmod(i, K)
        for a in range(TAPS[method]):
            M[i, min(max(q + int(base[r]) + a, 0), H1 - 1)] += float(wt[r, a])
    return M


def torch_up(X, method, K):
    kw = {} if method == NEAREST else {"align_corners": False}
    return torch.nn.functional.interpolate(torch.tensor(X, dtype=torch.float64)[None, None], scale_factor=K, mode=MODE[method], **kw)[0, 0].numpy()


def test_the_methods_are_the_headers():
    import os
    import re
    from tensorforth_amd.lib import root_dir
    text = open(os.path.join(root_dir(), "include", "t4k.h")).read()
    body = re.search(r"enum\s*\{\s*(T4K_UP_NEAREST[^}]*)\}", text).group(1)
    assert [t.strip().split("=")[0].strip() for t in body.split(",")] == ["T4K_UP_NEAREST", "T4K_UP_LINEAR", "T4K_UP_BILINEAR", "T4K_UP_CUBIC"]
    assert "T4K_UP_NEAREST = 0" in body


def test_the_table_against_torch(lib):
    """every admitted (method, K) on every shape: extents, My X Mx^T against interpolate, rows of wt summing to 1, unused cells 0"""
    rng = np.random.default_rng(1)
    n = 0
    for method, K in admitted():
        T = TAPS[method]
        for H1, W1 in SHAPES:
            rc, out, wt, base = plan(lib, method, 2, H1, W1, 3, K)
            assert rc == OK and out[:2] == [K * H1, K * W1], (method, K, H1, W1, rc, out)
            My, Mx = matrix(wt, base, method, K, H1), matrix(wt, base, method, K, W1)
            X = rng.uniform(-2.0, 2.0, size=(H1, W1))
            want = torch_up(X, method, K)
            assert want.shape == (K * H1, K * W1)
            got = My @ X @ Mx.T
            bound = 64 * 2.0 ** -24 * (np.abs(My) @ np.abs(X) @ np.abs(Mx).T)
            assert np.all(np.abs(got - want) <= bound), (method, K, H1, W1, float(np.max(np.abs(got - want) / bound)))
            n += 1
        # the table itself: K rows of T weights that sum to 1 within 2 ulp, every other cell 0; the bases in the range the kernels assume
        assert not wt[K:].any() and not wt[:, T:].any() and not base[K:].any(), (method, K)
        s = wt[:K].astype(np.float64).sum(1)
        assert np.all(np.abs(s - 1.0) <= 2 * 2.0 ** -23), (method, K, s)
        assert np.all(base[:K] >= -(T // 2)) and np.all(base[:K] + T - 1 <= T // 2), (method, K, base)
    assert n == (16 * 3 + 8) * len(SHAPES)


def test_the_table_is_the_rule(lib):
    """the table's cells against the rule worked out here in exact rationals: lambda = num / 2K, the cubic-convolution polynomials with A = -3/4"""
    from fractions import Fraction as Fr
    A = Fr(-3, 4)
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    for method, K in admitted():
        _, _, wt, base = plan(lib, method, 1, 1, 1, 1, K)
        for r in range(K):
            u = 2 * r + 1 - K
            b, lam = (0, Fr(u, 2 * K)) if u >= 0 else (-1, Fr(u + 2 * K, 2 * K))
            if method == NEAREST:
                wb, ww = 0, [Fr(1)]
            elif method == CUBIC:
                wb, ww = b - 1, [c2(lam + 1), c1(lam), c1(1 - lam), c2(2 - lam)]
            else:
                wb, ww = b, [1 - lam, lam]
            assert base[r] == wb, (method, K, r)
            for a, w in enumerate(ww):
                assert abs(float(wt[r, a]) - float(w)) <= 2.0 ** -24 * abs(float(w)) + 2.0 ** -48, (method, K, r, a)   # one float rounding, and the double polynomial (terms below 8)
    assert np.array_equal(plan(lib, LINEAR, 1, 1, 1, 1, 5)[2], plan(lib, BILINEAR, 1, 1, 1, 1, 5)[2])       # the same arithmetic under two names


def test_rejections(lib):
    good = dict(method=BILINEAR, N=3, H1=5, W1=4, C=4, K=3)
    call = lambda **kw: plan(lib, **{**good, **kw})[0]
    assert call() == OK
    assert lib.t4k_upsample_plan(BILINEAR, 3, 5, 4, 4, 3, 3, None, None, None) == ERR_ARG
    rc, out, wt, base = plan(lib, BILINEAR, 3, 5, 4, 4, 3, table=False)                             # wt and base may be NULL
    assert rc == OK and out == [15, 12, 4, 4]
    for m in (-1, 4, 100):
        assert call(method=m) == ERR_UNSUPPORTED and b"method" in lib.t4k_last_error()
    for m in (NEAREST, LINEAR, BILINEAR):
        assert call(method=m, K=1) == OK and call(method=m, K=16) == OK
        for K in (0, -1, 17, 100):
            assert call(method=m, K=K) == ERR_UNSUPPORTED and b"not supported" in lib.t4k_last_error(), (m, K)
    assert call(method=CUBIC, K=1) == OK and call(method=CUBIC, K=8) == OK
    for K in (0, 9, 16):
        assert call(method=CUBIC, K=K) == ERR_UNSUPPORTED and b"not supported" in lib.t4k_last_error(), K
    for name in ("N", "H1", "W1", "C"):                                                              # an extent below 1: a bad argument
        assert call(**{name: 0}) == ERR_ARG and call(**{name: -2}) == ERR_ARG, name
        assert b"extent" in lib.t4k_last_error()
    # N H0 W0 below 2^31
    assert call(N=1 << 19, H1=32, W1=32, K=2) == ERR_UNSUPPORTED and b"2^31" in lib.t4k_last_error()
    assert call(N=(1 << 19) - 1, H1=32, W1=32, K=2) == OK
    assert call(N=1, H1=1 << 27, W1=1, K=16) == ERR_UNSUPPORTED and call(N=1, H1=1, W1=1 << 27, K=16) == ERR_UNSUPPORTED
    assert call(N=(1 << 31) - 1, H1=(1 << 31) - 1, W1=(1 << 31) - 1, K=16) == ERR_UNSUPPORTED       # no overflow on the way to the verdict
    assert call(N=(1 << 31) - 1, H1=1, W1=1, K=1, method=NEAREST) == OK


@pytest.mark.parametrize("C", [3, 4, 8])
@pytest.mark.parametrize("aligned", [0, 1, 2, 3])
def test_vector_widths(lib, C, aligned):
    """a width of 4 needs C % 4 == 0 and the pass's own alignment bit - the forward bit 0, the backward bit 1 - for every method"""
    for method in range(4):
        rc, out, _, _ = plan(lib, method, 3, 5, 4, C, 3, aligned)
        assert rc == OK
        assert out == [15, 12, 4 if (C % 4 == 0 and aligned & 1) else 1, 4 if (C % 4 == 0 and aligned & 2) else 1], (method, C, aligned, out)
