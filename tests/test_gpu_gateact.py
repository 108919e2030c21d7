"""t4k_gateact_fwd / _bwd (csrc/gateact.hip) through the C ABI, against float64.

One case function over kind x gate x (T, C): both load paths, the gated 16-byte path falling back to dwords (Hc = 5), a partial last workgroup, more than one
item a lane, a token boundary inside a wave.  The inputs are test_gateact_plan.operands: a in [-30, 30], dense near 0 and +-6, with 0, +-88, +-1e4 and
+-3.4e38 at the end (the last of them where the tensor is smaller), dY ~ N(0, 1).  Every element is held to test_gateact_plan.bound with K below: twice
the worst ratio measured over the sweep on an MI355X, rounded up to a power of two (DESIGN.md 3.24 has the ratios)."""
import ctypes

import numpy as np
import pytest

from test_gateact_plan import ERR_ARG, ERR_UNSUPPORTED, I8, OK, bound, operands, rule
from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount
from test_gpu_token_ce import bits, nan

pytestmark = pytest.mark.gpu

F = np.float32
K_FWD = {0: 4.0, 1: 4.0, 2: 4.0, 3: 4.0}
K_BWD = {0: 32.0, 1: 64.0, 2: 16.0, 3: 16.0}
SHAPES = [(1, 2), (3, 10), (65, 8), (2, 520), (130, 24)]


def held(what, got, ref, cond, scale, k):
    err = np.abs(got.astype(np.float64) - ref)
    r = (np.maximum(err - bound(0.0, ref, cond, scale), 0.0) / (bound(1.0, ref, cond, scale) - bound(0.0, ref, cond, scale) + 1e-300)).max()
    print("%s worst ratio %.2f" % (what, r))
    assert np.isfinite(got).all() and (err <= bound(k, ref, cond, scale)).all(), (what, r, k)


@pytest.mark.parametrize("T,C", SHAPES, ids=["t%d_c%d" % s for s in SHAPES])
@pytest.mark.parametrize("gate", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_every_rung_against_float64(t4k, kind, gate, T, C):
    h = t4k
    Hc = C // 2 if gate else C
    X, DY = operands(gate, T, C, 100 * T + C)
    (y, cy, sy), (dx, cdx, sdx) = rule(kind, gate, X, DY)
    for off in (0, 1):                                                       # once with X, Y and DX 4 bytes off a 16-byte boundary: the dword rungs
        out = I8()
        assert h.lib.t4k_gateact_plan(T, C, kind, gate, int(off == 0), out) == OK
        wide = off == 0 and (Hc if gate else T * C) % 4 == 0
        assert list(out)[:3] == [2 * gate + (0 if wide else 1), 4 if wide else 1, 4] and out[3] == out[4] == -(-T * Hc // (out[1] * 1024)), list(out)
        dX, dDY, dY, dDX = Dev(X, off), Dev(DY), Dev(nan(T * Hc), off), Dev(nan(T * C), off)
        l0 = lcount(h)
        h.call("t4k_gateact_fwd", dX.p, dY.p, T, C, kind, gate, None)
        assert lcount(h) - l0 == 1
        Y = dY.get(h, (T, Hc)).copy()
        assert bits(dX.get(h, (T, C)), X), "the forward changed X"
        l0 = lcount(h)
        h.call("t4k_gateact_bwd", dX.p, dDY.p, dDX.p, T, C, kind, gate, None)
        assert lcount(h) - l0 == 1
        DX = dDX.get(h, (T, C)).copy()
        assert bits(dX.get(h, (T, C)), X) and bits(dDY.get(h, (T, Hc)), DY), "an operand changed"
        held("y", Y, y, cy, sy, K_FWD[kind]); held("dx", DX, dx, cdx, sdx, K_BWD[kind])
        dY2 = Dev(nan(T * Hc), off)
        h.call("t4k_gateact_fwd", dX.p, dY2.p, T, C, kind, gate, None)
        assert bits(dY2.get(h, (T, Hc)), Y), "two calls, two results"
        h.call("t4k_gateact_bwd", dX.p, dDY.p, dX.p, T, C, kind, gate, None)                          # DX = X
        assert bits(dX.get(h, (T, C)), DX), "in place is not out of place"
        guards_intact(dX, dDY, dY, dDX, dY2)


def test_rejections_launch_and_write_nothing(t4k):
    h = t4k
    T, C = 6, 8
    x, dy = Dev(np.ones((T, C), F)), Dev(np.ones((T, C), F))
    Y, DX = Dev(np.full(T * C, 77.0, F)), Dev(np.full(T * C, 77.0, F))
    f, b = "t4k_gateact_fwd", "t4k_gateact_bwd"

    def refused(code, fn, *a):
        l0 = lcount(h)
        rc = getattr(h.lib, fn)(*a)
        assert rc == code and lcount(h) == l0 and h.lib.t4k_last_error(), (fn, a, rc)
    for fn, a in ((f, [x.p, Y.p]), (b, [x.p, dy.p, DX.p])):
        for i in range(len(a)):
            refused(ERR_ARG, fn, *(a[:i] + [None] + a[i + 1:]), T, C, 0, 0, None)                     # a NULL pointer
        for bad in ((0, C, 0, 0), (T, 0, 0, 0), (T, C, 4, 0), (T, C, -1, 0), (T, C, 0, 2), (T, C, 0, -1), (T, 7, 2, 1)):
            refused(ERR_ARG, fn, *a, *bad, None)
        refused(ERR_UNSUPPORTED, fn, *a, 1 << 28, C, 0, 0, None)                                     # T C = 2^31
    off4 = lambda d: ctypes.c_void_p(d.p.value + 4)
    refused(ERR_ARG, f, x.p, x.p, T, C, 0, 0, None)                                                  # Y over X
    refused(ERR_ARG, f, x.p, off4(x), T - 1, C, 2, 1, None)                                          # Y inside X
    refused(ERR_ARG, b, x.p, dy.p, dy.p, T, C, 0, 0, None)                                           # DX over DY
    refused(ERR_ARG, b, x.p, dy.p, off4(x), T - 1, C, 0, 0, None)                                    # DX overlaps X but is not X
    refused(ERR_ARG, b, x.p, x.p, DX.p, T, C, 2, 1, None)                                            # DY inside X
    for d in (Y, DX):
        assert (d.get(h, (T * C,)) == 77.0).all()
    guards_intact(x, dy, Y, DX)
