"""t4k_retention_fwd / _bwd (include/t4k.h, csrc/retention.hip) through the C ABI, against the O(L^2) rule in float64
(tests/test_retention_plan.rule) on the float32 operands the kernels were given.

Every element of Y, dQ, dK and dV is held to K u M: M the same sum over absolute values, u = 2^-24, K the next power of two above the worst ratio
err / (u M) measured over test_grid's shapes on one MI355X (DESIGN.md 3.26 lists the ratios).  Outputs are pre-filled with NaN between guard floats (Dev): an
element that was not written shows, and so does a store outside the tensor.  B, the chunk count and the launch counts come from t4k_retention_plan."""
import ctypes

import numpy as np
import pytest

from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount
from test_retention_plan import ERR_ARG, ERR_UNSUPPORTED, I8, OK, rule

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K = {"y": 4, "dq": 4, "dk": 4, "dv": 4}                                     # measured worst ratios: DESIGN.md 3.26


def plan(h, N, L, heads, d, aligned=1):
    out = I8()
    assert h.lib.t4k_retention_plan(N, L, heads, d, aligned, 32 << 20, out) == OK, h.lib.t4k_last_error()
    return list(out)


def nan(k):
    return np.full(k, np.nan, np.float32)


def data(seed, N, L, heads, d):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (N, L, 3 * heads * d)).astype(np.float32), rng.normal(0.0, 1.0, (N, L, heads * d)).astype(np.float32)


def ratios(Y, G, QKV, DY, heads):
    """worst err / (u M) of Y, dQ, dK, dV; an element with M = 0 must be exact"""
    wy, wg = rule(QKV, DY, heads)
    my, mg = rule(np.abs(QKV), np.abs(DY), heads)
    N, L, E = Y.shape
    def worst(got, want, m):
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err[m == 0] == 0)
        return float(np.max(err / np.where(m == 0, 1.0, U * m)))
    part = lambda a, k: a.reshape(N, L, 3, E)[:, :, k]
    return {"y": worst(Y, wy, my), **{nm: worst(part(G, k), part(wg, k), part(mg, k)) for k, nm in enumerate(("dq", "dk", "dv"))}}


def run_case(h, N, L, heads, d, off=0, operands=None, seed=0):
    """forward, then backward: launches against the plan, operands intact, guards, every element written.  off: floats every pointer starts off 16 bytes"""
    E = heads * d
    QKV, DY = operands or data(seed + 1000 * L + 10 * d + heads, N, L, heads, d)
    p = plan(h, N, L, heads, d, int(off % 4 == 0))
    assert p[1] == (4 if off % 4 == 0 else 1) and p[4] == p[5] == (1 if L <= p[2] else 3) and p[3] == -(-L // p[2]), p
    dQ, dDY, dO, dS, dG = Dev(QKV, off), Dev(DY, off), Dev(nan(N * L * E), off), Dev(nan(N * heads * p[3] * d * d), off), Dev(nan(3 * N * L * E), off)
    l0 = lcount(h)
    h.call("t4k_retention_fwd", dQ.p, dO.p, dS.p, N, L, heads, d, None)
    assert lcount(h) - l0 == p[4], p
    ST = dS.get(h, (dS.n,)).copy()
    l0 = lcount(h)
    h.call("t4k_retention_bwd", dQ.p, dDY.p, dS.p, dG.p, N, L, heads, d, None)
    assert lcount(h) - l0 == p[5], p
    Y, G = dO.get(h, (N, L, E)).copy(), dG.get(h, (N, L, 3 * E)).copy()
    assert not np.isnan(Y).any() and not np.isnan(G).any()
    assert np.isnan(ST).all() if p[3] == 1 else not np.isnan(ST).any()      # one chunk leaves ST alone; more write every state
    assert np.array_equal(dQ.get(h, QKV.shape), QKV) and np.array_equal(dDY.get(h, DY.shape), DY)
    assert np.array_equal(dS.get(h, ST.shape).view(np.uint32), ST.view(np.uint32))
    guards_intact(dQ, dDY, dO, dS, dG)
    return p, Y, G


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_grid(t4k, d):
    B = plan(t4k, 1, 1, 1, d)[2]
    worst = dict.fromkeys(K, 0.0)
    for L in (1, 2, B - 1, B, B + 1, 2 * B + 3, 3 * B):
        for heads in (1, 3):
            for N in (1, 2):
                QKV, DY = data(7, N, L, heads, d)
                _, Y, G = run_case(t4k, N, L, heads, d, operands=(QKV, DY))
                r = ratios(Y, G, QKV, DY, heads)
                print("d %d L %d heads %d N %d: err / (u M)" % (d, L, heads, N), {k: round(v, 3) for k, v in r.items()})
                worst = {k: max(worst[k], r[k]) for k in K}
                if L == 1:                                               # Y = scale (Q . K) V to the dot product's rounding: d products, the score's and the scale's
                    assert r["y"] <= d + 3, r
    print("d %d worst" % d, worst)
    assert all(worst[k] <= K[k] for k in K), worst


@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_exact_cases(t4k, d):
    """Q = 0 gives Y = 0 and dY = 0 gives DQKV = 0, bit for bit, over three chunks"""
    N, heads, L = 2, 3, 2 * plan(t4k, 1, 1, 1, d)[2] + 3
    QKV, DY = data(3, N, L, heads, d)
    QKV.reshape(N, L, 3, heads * d)[:, :, 0] = 0.0
    _, Y, _ = run_case(t4k, N, L, heads, d, operands=(QKV, DY))
    assert not Y.view(np.uint32).any()
    _, _, G = run_case(t4k, N, L, heads, d, operands=(data(4, N, L, heads, d)[0], np.zeros_like(DY)))
    assert not G.view(np.uint32).any()


@pytest.mark.parametrize("shape", [(131, 3, 20), (65, 2, 64), (70, 1, 128), (5, 2, 4)], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_twice_on_dwords_and_per_sample(t4k, shape):
    """a second call, the call with every pointer 4 bytes off (the plan's dword path, asserted in run_case), and two N = 1 calls give the N = 2 call's bits"""
    L, heads, d = shape
    QKV, DY = data(11, 2, L, heads, d)
    p, Y, G = run_case(t4k, 2, L, heads, d, operands=(QKV, DY))
    for off in (0, 1):
        q, Y2, G2 = run_case(t4k, 2, L, heads, d, off=off, operands=(QKV, DY))
        assert q[1] == (1 if off else 4) and same(Y, Y2) and same(G, G2), (shape, off)
    for n in (0, 1):
        q, Y1, G1 = run_case(t4k, 1, L, heads, d, operands=(QKV[n:n + 1], DY[n:n + 1]))
        assert q[:4] == p[:4] and same(Y[n:n + 1], Y1) and same(G[n:n + 1], G1), (shape, n)
    r = ratios(Y, G, QKV, DY, heads)
    assert all(r[k] <= K[k] for k in K), r


def test_rejections(t4k):
    """every rejection: its code, a text, nothing launched, nothing written"""
    h = t4k
    N, L, heads, d = 2, 70, 3, 8
    E = heads * d
    QKV, DY = data(9, N, L, heads, d)
    dQ, dDY, dS = Dev(QKV), Dev(DY), Dev(np.zeros(N * heads * 2 * d * d, np.float32))
    dO, dT, dG = Dev(nan(N * L * E)), Dev(nan(N * heads * 2 * d * d)), Dev(nan(3 * N * L * E))
    fwd = lambda a=None, shape=(N, L, heads, d): h.lib.t4k_retention_fwd(*(a or (dQ.p, dO.p, dT.p)), *shape, None)
    bwd = lambda a=None, shape=(N, L, heads, d): h.lib.t4k_retention_bwd(*(a or (dQ.p, dDY.p, dS.p, dG.p)), *shape, None)
    err = h.lib.t4k_last_error
    l0 = lcount(h)
    for k in range(3):
        a = [dQ.p, dO.p, dT.p]; a[k] = None
        assert fwd(a) == ERR_ARG and b"null" in err(), k
    for k in range(4):
        a = [dQ.p, dDY.p, dS.p, dG.p]; a[k] = None
        assert bwd(a) == ERR_ARG and b"null" in err(), k
    for f in (fwd, bwd):
        for k in range(3):
            for v in (0, -1):
                s = [N, L, heads, d]; s[k] = v
                assert f(shape=s) == ERR_ARG and b"extent" in err(), s
        assert f(shape=(N, L, 33, d)) == ERR_ARG and b"heads=33" in err()
        for dd in (0, -4, 2, 6, 132):
            assert f(shape=(N, L, heads, dd)) == ERR_UNSUPPORTED and b"head size" in err(), dd
        assert f(shape=(1 << 10, 1 << 10, 8, 128)) == ERR_UNSUPPORTED and b"2^31" in err()
        assert f(shape=(1, 1 << 20, 4, 128)) == ERR_UNSUPPORTED and b"workspace" in err()          # 8 GB of reverse states
    at = lambda dev, k: ctypes.c_void_p(dev.t.data_ptr() + 4 * (dev.off + k))
    for a in ([dQ.p, dDY.p, dS.p, dQ.p], [dQ.p, dDY.p, dS.p, at(dQ, 4)], [dQ.p, at(dG, 3 * N * L * E - 4), dS.p, dG.p], [dQ.p, dDY.p, at(dG, 8), dG.p]):
        assert bwd(a) == ERR_ARG and b"overlap" in err()
    assert lcount(h) == l0
    for dv in (dO, dT, dG):
        assert np.isnan(dv.get(h, (dv.n,))).all()
    guards_intact(dO, dT, dG)
    assert fwd() == OK and bwd() == OK
