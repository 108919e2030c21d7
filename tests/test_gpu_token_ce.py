"""t4k_token_softmax_fwd / _softmax_bwd / _ce_bwd / _ce_score (csrc/token_ce.hip) through the C ABI, against float64.

One case function over (T, V, pointer offset) rows chosen from the plan: every rung on both load paths, each register limit at -1 item / exact / +1 item
(512 and 2048 items; the +1 of the second is the first two-pass V), T on both sides of a wave's token batch, one pointer 4 bytes off 16.  P is held to
f64_witness.softmax (plus, on the two-pass rung, the rescale term tests/test_gpu_softmax_axes.py derives with R from the plan), lse and the Jacobian product
to the witnesses below, the CE gradient bit for bit (one exactly rounded subtraction of the stored P), the loss to a T-term sum plus ULP_LOG a term."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt
from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
WS = 32 << 20
F = np.float32
U = wt.U
PADS = np.array([-1.0, -0.5, 0.0, 1e9, np.nan, np.inf, -np.inf], F)        # (the third is replaced by V: the first id that is none)

# (T, V, floats X and P start off 16 bytes, rung)
CASES = [(1, 2, 0, 0), (2, 3, 0, 0), (63, 4, 0, 0), (65, 63, 0, 0), (257, 64, 0, 0), (65, 65, 0, 0), (63, 255, 0, 0), (2, 260, 0, 0), (65, 64, 1, 0),
         (3, 2044, 0, 0), (3, 2048, 0, 0), (2, 2052, 0, 1), (2, 8188, 0, 1), (2, 8192, 0, 1), (3, 8196, 0, 2),
         (3, 511, 0, 0), (2, 512, 1, 0), (2, 513, 0, 1), (2, 2047, 0, 1), (2, 2048, 1, 1), (3, 2049, 0, 2)]


def nan(k):
    return np.full(k, np.nan, F)


def bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).ravel().view(np.uint32), np.ascontiguousarray(b, F).ravel().view(np.uint32))


def plan(h, T, V, aligned):
    out = I8()
    assert h.lib.t4k_token_ce_plan(T, V, aligned, WS, out) == OK, h.lib.t4k_last_error()
    return list(out)


def make_ids(rng, T, V):
    ids = (rng.integers(0, V, T) + rng.choice([0.0, 0.75], T)).astype(F)    # k + 0.75 truncates to k
    pads = PADS.copy(); pads[2] = V
    where = np.arange(T) % 3 == 1
    ids[where] = np.resize(pads, T)[where]
    return ids


def id_rule(ids, V):
    with np.errstate(invalid="ignore"):
        valid = (ids >= 0) & (ids < F(V))
    return valid, np.where(valid, np.nan_to_num(ids, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)


def jacobian_witness(X, DY, lse, dl):
    """DX = p (dY - g), p = exp(x - lse), g = sum dY p, with lse stored to within dl: p errs relatively by ep (the exp, its argument, the stored lse), the
    V-term dot by the classical C_SUM bound plus ep, and a subtraction and a product stand behind it"""
    x, dy = wt.f64(X), wt.f64(DY); V = x.shape[-1]
    p = np.exp(x - lse[:, None]); g = (dy * p).sum(-1, keepdims=True); A = (np.abs(dy) * p).sum(-1, keepdims=True)
    ep = (wt.ULP_EXP + 2.0 * np.abs(x - lse[:, None]) + 1.0) * U + dl[:, None]
    eg = wt.C_SUM * (V + 1) * U * A + ep.max(-1, keepdims=True) * A
    jb = ep * p * np.abs(dy - g) + p * (eg + U * (np.abs(dy) + np.abs(g))) + 2.0 * U * np.abs(p * (dy - g)) + wt.TINY
    return wt.W(p * (dy - g), jb / U, 1, 1.0)


def lse_witness(X, extra=0.0):
    """(lse, its bound): the sum's ulps (f64_witness.softmax) through ln, one __logf (ULP_LOG) and one add"""
    x = wt.f64(X); V = x.shape[-1]
    m = x.max(-1); s = np.exp(x - m[:, None]).sum(-1); lse = m + np.log(s)
    esum = (wt.ULP_EXP + 2.0 * (m - x.min(-1))) + V + extra
    return lse, U * (esum + wt.ULP_LOG * np.abs(np.log(s)) + np.abs(lse))


@pytest.mark.parametrize("T,V,off,rung", CASES, ids=["t%d_v%d_o%d" % c[:3] for c in CASES])
def test_every_rung_against_float64(t4k, T, V, off, rung):
    h = t4k
    rng = np.random.default_rng(1000 * V + T)
    pl = plan(h, T, V, int(off == 0))
    assert pl[0] == rung and pl[1] == (4 if V % 4 == 0 and off == 0 else 1) and pl[4] == (2 if rung == 2 else 1), pl
    X = rng.normal(0.0, 2.0, (T, V)).astype(F)
    c1, c2 = V // 3, V - 1                                                   # the maximum twice, in other lanes, waves and chunks: the first wins
    X[1::2, c1] = X[1::2, c2] = X[1::2].max(-1) + F(1.0)
    DY = rng.normal(0.0, 1.0, (T, V)).astype(F)
    IDS = make_ids(rng, T, V)
    dX, dDY, dI = Dev(X, off), Dev(DY), Dev(IDS)
    dP, dS, dDX, dJ, dR = Dev(nan(T * V), off), Dev(nan(2 * T)), Dev(nan(T * V)), Dev(nan(T * V)), Dev(nan(3))
    l0 = lcount(h)
    h.call("t4k_token_softmax_fwd", dX.p, dP.p, dS.p, T, V, None)
    assert lcount(h) - l0 == 1
    P, S = dP.get(h, (T, V)).copy(), dS.get(h, (T, 2)).copy()
    x = wt.f64(X)
    w = wt.softmax(X)
    extra = pl[5] * (wt.ULP_EXP + 1.0) + 2.0 * (x.max(-1, keepdims=True) - x.min(-1, keepdims=True)) if rung == 2 else 0.0
    w.n = w.n + extra
    print("P worst ratio %.3f" % wt.check("P", P, w))
    assert np.array_equal(S[:, 1], np.argmax(X, -1).astype(F)), "the arg-max is not the first maximum"
    lse, dl = lse_witness(X, np.max(extra) if rung == 2 else 0.0)
    print("lse worst ratio %.3f" % wt.check("lse", S[:, 0], wt.W(lse, dl / U, 1, 1.0)))
    dP2, dS2 = Dev(nan(T * V), off), Dev(nan(2 * T))
    h.call("t4k_token_softmax_fwd", dX.p, dP2.p, dS2.p, T, V, None)
    assert bits(dP2.get(h, (T, V)), P) and bits(dS2.get(h, (T, 2)), S)
    # CE backward: one exactly rounded subtraction of the stored P; padding rows are zeros
    valid, k = id_rule(IDS, V)
    l0 = lcount(h)
    h.call("t4k_token_ce_bwd", dP.p, dI.p, dDX.p, T, V, None)
    assert lcount(h) - l0 == 1
    want = P.copy(); want[np.arange(T), k] -= F(1.0); want[~valid] = 0.0
    assert bits(dDX.get(h, (T, V)), want), "the CE gradient"
    l0 = lcount(h)
    h.call("t4k_token_softmax_bwd", dX.p, dS.p, dDY.p, dJ.p, T, V, None)
    assert lcount(h) - l0 == 1
    J = dJ.get(h, (T, V)).copy()
    print("Jacobian worst ratio %.3f" % wt.check("dx", J, jacobian_witness(X, DY, lse, dl)))
    assert bits(dX.get(h, (T, V)), X) and bits(dDY.get(h, (T, V)), DY) and bits(dP.get(h, (T, V)), P), "an operand changed"
    l0 = lcount(h)
    h.call("t4k_token_ce_score", dP.p, dS.p, dI.p, dR.p, T, V, None)
    assert lcount(h) - l0 == pl[6] == (2 if T > 256 else 1)
    rec = dR.get(h, (3,)).copy()
    nll = np.where(valid, -np.log(np.maximum(wt.f64(P)[np.arange(T), k], float(np.finfo(F).tiny))), 0.0)
    assert list(rec[1:].view(np.int32)) == [int(np.sum(valid & (np.argmax(X, -1) == k))), int(valid.sum())], rec.view(np.int32)
    wt.check("loss", rec[:1], wt.W([nll.sum()], [(wt.C_SUM * T + wt.ULP_LOG + 1.0) * np.abs(nll).sum()], 1, 1.0))
    h.call("t4k_token_softmax_bwd", dX.p, dS.p, dDY.p, dX.p, T, V, None)                              # DX = X
    assert bits(dX.get(h, (T, V)), J), "in place is not out of place"
    guards_intact(dX, dDY, dI, dP, dS, dDX, dJ, dR, dP2, dS2)


@pytest.mark.parametrize("T,V", [(5, 11), (2, 2052), (2, 8196)])
def test_constant_masked_and_all_padding_rows(t4k, T, V):
    h = t4k
    dP, dS, dR, dD = Dev(nan(T * V)), Dev(nan(2 * T)), Dev(nan(3)), Dev(nan(T * V))
    dC = Dev(np.full((T, V), 0.75, F))
    h.call("t4k_token_softmax_fwd", dC.p, dP.p, dS.p, T, V, None)
    assert bits(dP.get(h, (T, V)), np.full((T, V), F(1) / F(V), F)) and not dS.get(h, (T, 2))[:, 1].any()      # no element dropped or doubled
    X = np.random.default_rng(V).normal(0.0, 1.0, (T, V)).astype(F)
    X[:, 1::2] = -np.inf                                                     # masked logits store exactly +0
    dX = Dev(X)
    h.call("t4k_token_softmax_fwd", dX.p, dP.p, dS.p, T, V, None)
    P = dP.get(h, (T, V)).copy()
    assert bits(P[:, 1::2], np.zeros_like(P[:, 1::2])) and np.allclose(P.sum(-1), 1.0, atol=1e-4) and np.isfinite(dS.get(h, (T, 2))).all()
    pads = PADS.copy(); pads[2] = V
    ids = Dev(np.resize(pads, T))                                             # every token padding
    h.call("t4k_token_ce_score", dP.p, dS.p, ids.p, dR.p, T, V, None)
    h.call("t4k_token_ce_bwd", dP.p, ids.p, dD.p, T, V, None)
    assert not dR.get(h, (3,)).view(np.uint32).any() and bits(dD.get(h, (T, V)), np.zeros((T, V), F))
    guards_intact(dC, dX, dP, dS, dR, dD)


def test_rejections_launch_and_write_nothing(t4k):
    h = t4k
    T, V = 6, 8
    x, dy, ids, st = Dev(np.ones((T, V), F)), Dev(np.ones((T, V), F)), Dev(np.zeros(T, F)), Dev(np.ones(2 * T, F))
    can = lambda n: Dev(np.full(n, 77.0, F))
    P, S, DX, R = can(T * V), can(2 * T), can(T * V), can(3)
    f, j, c, sc = "t4k_token_softmax_fwd", "t4k_token_softmax_bwd", "t4k_token_ce_bwd", "t4k_token_ce_score"

    def refused(code, fn, *a):
        l0 = lcount(h)
        rc = getattr(h.lib, fn)(*a)
        assert rc == code and lcount(h) == l0 and h.lib.t4k_last_error(), (fn, a, rc)
    for fn, a in ((f, [x.p, P.p, S.p]), (j, [x.p, st.p, dy.p, DX.p]), (c, [x.p, ids.p, DX.p]), (sc, [x.p, st.p, ids.p, R.p])):
        for i in range(len(a)):
            refused(ERR_ARG, fn, *(a[:i] + [None] + a[i + 1:]), T, V, None)                       # a NULL pointer
        refused(ERR_ARG, fn, *a, 0, V, None)
        refused(ERR_ARG, fn, *a, T, 1, None)
        refused(ERR_UNSUPPORTED, fn, *a, 1, (1 << 24) + 1, None)
        refused(ERR_UNSUPPORTED, fn, *a, 1 << 28, V, None)                                       # T V = 2^31
    refused(ERR_ARG, f, x.p, x.p, S.p, T, V, None)                                               # P over X
    refused(ERR_ARG, j, x.p, st.p, dy.p, dy.p, T, V, None)                                       # DX over DY
    refused(ERR_ARG, j, x.p, st.p, dy.p, ctypes.c_void_p(x.p.value + 4), T - 1, V, None)         # DX overlaps X but is not X
    refused(ERR_ARG, c, x.p, ids.p, x.p, T, V, None)                                             # DX over P
    out = I8(*[-7] * 8)
    for a in ((0, V, 1, WS), (T, 1, 1, WS), (T, V, 1, -1)):
        assert h.lib.t4k_token_ce_plan(*a, out) == ERR_ARG and list(out) == [-7] * 8
    for d, n in ((P, T * V), (S, 2 * T), (DX, T * V), (R, 3)):
        assert (d.get(h, (n,)) == 77.0).all()
    guards_intact(x, dy, ids, st, P, S, DX, R)
