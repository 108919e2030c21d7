"""t4k_upsample_fwd / _bwd (include/t4k.h, csrc/upsample.hip) through the C ABI: up-sampling by a run-time factor, nearest / bilinear / bicubic.

The witness is the float64 product with the FLOAT-ROUNDED table as the operand - the very operands the kernel read: My (H0 x H1) and Mx (W0 x W1) are built
from t4k_upsample_plan's wt and base (tests/test_upsample_plan.py holds that table against torch), O = My X Mx^T and dX = My^T dY Mx per sample and channel,
mag = the same product on absolute values, and the roundings behind an element are an ARRAY: T^2 + 4 forward, (non-zeros of the element's My column) x (of its
Mx column) + 4 backward.  tests/f64_witness.py's check excepts no element.  Every case runs on two kinds of operands:
  floats in +-[0.5, 2): inside the bound;
  integers in [-4, 4]: bit-equal where every partial sum fits 24 bits.  The premise is worked out per case on the witness's own terms (`fits24`): every weight
      a multiple of 2^-s, so every term a multiple of 2^-(sy + sx), and sum |terms| below 2^24 of those - then every partial sum in ANY order is exact.  It holds
      for nearest at any K, bilinear at K in {1, 2, 4, 8, 16} and bicubic at K in {1, 2}, forward and backward (asserted); elsewhere the bound applies.
Outputs are pre-filled with NaN between guard floats (Dev of tests/test_gpu_bcast.py): an element that was not written shows, and so does a store outside
the tensor."""
import ctypes
import zlib

import numpy as np
import pytest

import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount, operands

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
NEAREST, LINEAR, BILINEAR, CUBIC = range(4)                              # T4K_UP_* of include/t4k.h
TAPS = {NEAREST: 1, LINEAR: 2, BILINEAR: 2, CUBIC: 4}
AVG, USAMPLE = 13, 17                                                    # T4K_L_* of include/t4k.h
I4, F64, I16 = ctypes.c_int * 4, ctypes.c_float * 64, ctypes.c_int * 16

METHODS = [NEAREST, BILINEAR, CUBIC]
FACTORS = [1, 2, 3, 4, 5, 8, 16]
GRID = [(m, K) for m in METHODS for K in FACTORS if K <= (8 if m == CUBIC else 16)]
IMAGES = [(1, 1), (1, 5), (2, 3), (5, 4), (7, 6)]
CHANNELS = [1, 3, 4, 7, 8, 36]
BATCHES = [1, 3]
EXACT = {NEAREST: FACTORS, BILINEAR: [1, 2, 4, 8, 16], CUBIC: [1, 2]}      # where integers in [-4, 4] must come out bit-equal


def plan(h, method, n, H1, W1, C, K, aligned=3):
    out, wt, base = I4(), F64(), I16()
    assert h.lib.t4k_upsample_plan(method, n, H1, W1, C, K, aligned, out, wt, base) == OK, h.lib.t4k_last_error()
    return list(out), np.array(wt, np.float32).reshape(16, 4), np.array(base, np.int64)


_MATS = {}


def mats(h, method, K, H1):
    """(My, Ay, s): the signed map H0 x H1 in float64 from the float table, the same with |w| added up (the taps the forward sums one by one), and the
    smallest s with every weight a multiple of 2^-s (None beyond 2^-40)"""
    key = (method, K, H1)
    if key not in _MATS:
        _, wt, base = plan(h, method, 1, H1, 1, 1, K)
        M, A = np.zeros((K * H1, H1)), np.zeros((K * H1, H1))
        for i in range(K * H1):
            q, r = divmod(i, K)
            for a in range(TAPS[method]):
                y = min(max(q + int(base[r]) + a, 0), H1 - 1)
                M[i, y] += float(wt[r, a]); A[i, y] += abs(float(wt[r, a]))
        w = wt[:K].astype(np.float64)
        s = next((s for s in range(41) if np.all(w * 2.0 ** s == np.rint(w * 2.0 ** s))), None)
        _MATS[key] = (M, A, s)
    return _MATS[key]


def up(My, X, Mx):
    """My X Mx^T per sample and channel on NHWC"""
    return np.einsum("ih,nhwc,jw->nijc", My, X, Mx, optimize=True)


def down(My, G, Mx):
    """the transpose, My^T G Mx"""
    return np.einsum("ih,nijc,jw->nhwc", My, G, Mx, optimize=True)


def fits24(sy, sx, mag_taps, wmax):
    """every term a multiple of q = 2^-(sy + sx), sum |terms| and the largest weight product below 2^24 q: every partial sum is exact in fp32"""
    if sy is None or sx is None:
        return False
    return float(np.max(mag_taps)) * 2.0 ** (sy + sx) < 2.0 ** 24 and wmax * 2.0 ** (sy + sx) < 2.0 ** 24


def witness(h, method, K, X, G, kind):
    """(O witness, dX witness, (forward exact?, backward exact?))"""
    _, H1, W1, _ = X.shape
    T = TAPS[method]
    My, Ay, sy = mats(h, method, K, H1)
    Mx, Ax, sx = mats(h, method, K, W1)
    X64, G64 = fw.f64(X), fw.f64(G)
    o, dx = up(My, X64, Mx), down(My, G64, Mx)
    mo, mdx = up(np.abs(My), np.abs(X64), np.abs(Mx)), down(np.abs(My), np.abs(G64), np.abs(Mx))
    nb = (np.count_nonzero(My, axis=0)[:, None] * np.count_nonzero(Mx, axis=0)[None, :] + 4)[None, :, :, None]
    exact = (False, False)
    if kind == "int":
        wmax = float(Ay.max() * Ax.max())
        exact = (fits24(sy, sx, up(Ay, np.abs(X64), Ax), wmax), fits24(sy, sx, down(Ay, np.abs(G64), Ax), wmax))
    wo = fw.W(o, 0.0, 0) if exact[0] else fw.W(o, mo, T * T + 4)
    wdx = fw.W(dx, 0.0, 0) if exact[1] else fw.W(dx, mdx, np.broadcast_to(nb, dx.shape))
    return wo, wdx, exact


def run_case(h, name, method, n, H1, W1, C, K, off=0, kinds=("int", "float"), twice=False):
    """forward, then the backward into a separate DX, each against the witness; one launch per entry, guards, operands intact.
    off: floats every buffer starts off 16 bytes.  twice: a second run gives the same bits, and DX = the forward-input buffer gives them too"""
    H0, W0 = K * H1, K * W1
    geo = (n, H1, W1, C, H0, W0, K)
    pl = plan(h, method, n, H1, W1, C, K, 0 if off % 4 else 3)[0]
    assert pl[:2] == [H0, W0] and pl[2] == pl[3] == (4 if (C % 4 == 0 and off % 4 == 0) else 1), pl
    nan = lambda k: np.full(k, np.nan, np.float32)
    for kind in kinds:
        X, G = operands(kind, zlib.crc32(repr((name, method, kind, geo)).encode()), n, H1, W1, C, H0, W0)
        wo, wdx, exact = witness(h, method, K, X, G, kind)
        if kind == "int" and K in EXACT[method]:
            assert exact == (True, True), (name, method, geo, exact)
        dI, dG, dO, dDX = Dev(X, off), Dev(G, off), Dev(nan(G.size), off), Dev(nan(X.size), off)
        l0 = lcount(h)
        h.call("t4k_upsample_fwd", method, dI.p, dO.p, *geo, None)
        assert lcount(h) - l0 == 1, name
        O = dO.get(h, G.shape)
        fw.check("%s m%d %s O %s" % (name, method, kind, geo), O, wo)
        l0 = lcount(h)
        h.call("t4k_upsample_bwd", method, dG.p, dDX.p, *geo, None)
        assert lcount(h) - l0 == 1, name
        dx = dDX.get(h, X.shape)
        fw.check("%s m%d %s dX %s" % (name, method, kind, geo), dx, wdx)
        guards_intact(dO, dDX, dI, dG)
        assert np.array_equal(dI.get(h, X.shape), X) and np.array_equal(dG.get(h, G.shape), G)      # the operands are intact
        if twice:
            dO2, dDX2 = Dev(nan(G.size), off), Dev(nan(X.size), off)
            h.call("t4k_upsample_fwd", method, dI.p, dO2.p, *geo, None)
            h.call("t4k_upsample_bwd", method, dG.p, dDX2.p, *geo, None)
            assert np.array_equal(dO2.get(h, G.shape), O) and np.array_equal(dDX2.get(h, X.shape), dx), name
            h.call("t4k_upsample_bwd", method, dG.p, dI.p, *geo, None)                               # DX = the forward-input buffer: the in-place convention
            assert np.array_equal(dI.get(h, X.shape), dx), "%s m%d in place" % (name, method)
            guards_intact(dI, dO2, dDX2)
    return pl


@pytest.mark.parametrize("method,K", GRID, ids=["m%dk%d" % g for g in GRID])
def test_factors(t4k, method, K):
    for H1, W1 in IMAGES:
        for C in CHANNELS:
            for n in BATCHES:
                run_case(t4k, "grid", method, n, H1, W1, C, K)


def test_linear_is_bilinear(t4k):
    """method 1 and method 2: the same arithmetic under two names, the same bits"""
    h = t4k
    n, H1, W1, C, K = 2, 5, 4, 8, 3
    X, G = operands("float", 11, n, H1, W1, C, K * H1, K * W1)
    got = []
    for method in (LINEAR, BILINEAR):
        dI, dG, dO, dDX = Dev(X), Dev(G), Dev(np.full(G.size, np.nan, np.float32)), Dev(np.full(X.size, np.nan, np.float32))
        h.call("t4k_upsample_fwd", method, dI.p, dO.p, n, H1, W1, C, K * H1, K * W1, K, None)
        h.call("t4k_upsample_bwd", method, dG.p, dDX.p, n, H1, W1, C, K * H1, K * W1, K, None)
        got.append((dO.get(h, G.shape), dDX.get(h, X.shape)))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    fw.check("linear O", got[0][0], witness(h, LINEAR, K, X, G, "float")[0])


@pytest.mark.parametrize("C", [3, 8])
def test_twice_and_in_place(t4k, C):
    """the same bits on a second run; DX = the forward-input buffer gives the bits of a separate DX (the backward reads no forward input)"""
    for method, K in ((NEAREST, 4), (BILINEAR, 3), (BILINEAR, 16), (CUBIC, 2), (CUBIC, 5)):
        for H1, W1 in ((5, 4), (1, 5)):
            run_case(t4k, "twice", method, 2, H1, W1, C, K, kinds=("float",), twice=True)


@pytest.mark.parametrize("C", [3, 4, 8, 36])
def test_pointers_off_16_bytes(t4k, C):
    """every pointer 4 bytes (and 12 bytes) off 16-byte alignment: one channel per thread, asserted through the plan, which is the function the entries call"""
    assert plan(t4k, BILINEAR, 2, 5, 4, C, 3, 0)[0][2:] == [1, 1]
    assert plan(t4k, BILINEAR, 2, 5, 4, C, 3, 3)[0][2:] == ([4, 4] if C % 4 == 0 else [1, 1])
    for method in METHODS:
        run_case(t4k, "off", method, 2, 5, 4, C, 3, off=1)
        run_case(t4k, "off", method, 3, 7, 6, C, 2, off=3, kinds=("int",))


@pytest.mark.parametrize("shape", [(9, 64, 64, 64), (3, 448, 448, 1)], ids=["v4", "v1"])
def test_above_the_launch_cap(t4k, shape):
    """more work items than MAX_WG * BLK = 2048 * 256 threads, with a remainder, forward (outputs) and backward (inputs): the grid-stride loop per vector width"""
    n, H1, W1, C = shape
    items = n * H1 * W1 * (C // 4 if C % 4 == 0 else C)
    assert items > 2048 * 256 and items % (2048 * 256) and (4 * items) % (2048 * 256)
    pl = run_case(t4k, "cap", BILINEAR, n, H1, W1, C, 2, kinds=("int",))
    assert pl[2] == pl[3] == (4 if C % 4 == 0 else 1)


def test_rejections(t4k):
    """a bad argument: T4K_ERR_ARG; an inadmissible method or factor: T4K_ERR_UNSUPPORTED; a text either way, nothing launched, the outputs untouched"""
    h = t4k
    n, H1, W1, C = 2, 4, 3, 3
    nan = lambda k: np.full(k, np.nan, np.float32)
    big = n * 17 * H1 * 17 * W1 * C
    dI, dG, dO, dDX = Dev(np.ones(n * H1 * W1 * C, np.float32)), Dev(np.ones(big, np.float32)), Dev(nan(big)), Dev(nan(n * H1 * W1 * C))
    bad = [((BILINEAR, 2, 8, 7), ERR_ARG, b"gives 8x6"), ((NEAREST, 2, 9, 6), ERR_ARG, b"gives 8x6"), ((CUBIC, 2, 6, 8), ERR_ARG, b"gives 8x6"),
           ((NEAREST, 2, 4, 3), ERR_ARG, b"gives 8x6"),
           ((-1, 2, 8, 6), ERR_UNSUPPORTED, b"method"), ((4, 2, 8, 6), ERR_UNSUPPORTED, b"method"),
           ((NEAREST, 0, 0, 0), ERR_UNSUPPORTED, b"not supported"), ((NEAREST, 17, 68, 51), ERR_UNSUPPORTED, b"not supported"),
           ((LINEAR, 17, 68, 51), ERR_UNSUPPORTED, b"not supported"), ((BILINEAR, -2, 8, 6), ERR_UNSUPPORTED, b"not supported"),
           ((CUBIC, 9, 36, 27), ERR_UNSUPPORTED, b"not supported"), ((CUBIC, 16, 64, 48), ERR_UNSUPPORTED, b"not supported")]
    for (m, K, H0, W0), code, text in bad:
        l0 = lcount(h)
        assert h.lib.t4k_upsample_fwd(m, dI.p, dO.p, n, H1, W1, C, H0, W0, K, None) == code, (m, K)
        assert text in h.lib.t4k_last_error(), h.lib.t4k_last_error()
        assert h.lib.t4k_upsample_bwd(m, dG.p, dDX.p, n, H1, W1, C, H0, W0, K, None) == code, (m, K)
        assert text in h.lib.t4k_last_error() and lcount(h) == l0
    good = (n, H1, W1, C, 8, 6, 2)
    l0 = lcount(h)
    assert h.lib.t4k_upsample_fwd(BILINEAR, None, dO.p, *good, None) == ERR_ARG
    assert h.lib.t4k_upsample_fwd(BILINEAR, dI.p, None, *good, None) == ERR_ARG
    assert h.lib.t4k_upsample_bwd(BILINEAR, None, dDX.p, *good, None) == ERR_ARG
    assert h.lib.t4k_upsample_bwd(BILINEAR, dG.p, None, *good, None) == ERR_ARG and b"null" in h.lib.t4k_last_error()
    for k, name in enumerate(("N", "H1", "W1", "C")):
        a = list(good); a[k] = 0
        assert h.lib.t4k_upsample_fwd(NEAREST, dI.p, dO.p, *a, None) == ERR_ARG and b"extent" in h.lib.t4k_last_error(), name
        assert h.lib.t4k_upsample_bwd(NEAREST, dG.p, dDX.p, *a, None) == ERR_ARG and b"extent" in h.lib.t4k_last_error(), name
    # 2^31 output pixels or more: refused before anything is touched (the pointers are never followed)
    assert h.lib.t4k_upsample_fwd(NEAREST, dI.p, dO.p, 1 << 19, 32, 32, 1, 64, 64, 2, None) == ERR_UNSUPPORTED and b"2^31" in h.lib.t4k_last_error()
    assert h.lib.t4k_upsample_bwd(NEAREST, dG.p, dDX.p, 1 << 19, 32, 32, 1, 64, 64, 2, None) == ERR_UNSUPPORTED and b"2^31" in h.lib.t4k_last_error()
    assert lcount(h) == l0
    for d in (dO, dDX):
        assert np.isnan(d.get(h, (d.n,))).all()
    guards_intact(dO, dDX)


@pytest.mark.parametrize("KS", [2, 3])
@pytest.mark.parametrize("C", [3, 8])
def test_beside_the_old_entries(t4k, KS, C):
    """nearest at K in {2, 3} beside the route `2 upsample` / `3 upsample` keep: the forward bit-equal to t4k_dpool(USAMPLE); the backward bit-equal to
    t4k_pool(AVGPOOL) x 4 at K = 2 (both factors are powers of two) and, at K = 3, both inside the bound of the float64 tile sum - the old route rounds
    the division by 9 and the scale by 9 on top of its eight additions: 10 roundings, inside the 2 (9 + 4) the witness grants"""
    h = t4k
    n, H1, W1 = 2, 5, 4
    H0, W0 = KS * H1, KS * W1
    nan = lambda k: np.full(k, np.nan, np.float32)
    for kind in ("int", "float"):
        X, G = operands(kind, zlib.crc32(repr((KS, C, kind)).encode()), n, H1, W1, C, H0, W0)
        dI, dG, oo, on, xo, xn = Dev(X), Dev(G), Dev(nan(G.size)), Dev(nan(G.size)), Dev(nan(X.size)), Dev(nan(X.size))
        h.call("t4k_dpool", USAMPLE, oo.p, dI.p, n, H0, W0, H1, W1, C, KS, None)
        h.call("t4k_upsample_fwd", NEAREST, dI.p, on.p, n, H1, W1, C, H0, W0, KS, None)
        assert np.array_equal(oo.get(h, G.shape), on.get(h, G.shape)), kind
        h.call("t4k_pool", AVG, dG.p, xo.p, n, H0, W0, H1, W1, C, KS, None)
        h.call("t4k_upsample_bwd", NEAREST, dG.p, xn.p, n, H1, W1, C, H0, W0, KS, None)
        old = xo.get(h, X.shape) * np.float32(KS * KS)                  # the scale map of the old route, one fp32 product
        assert old.dtype == np.float32
        new = xn.get(h, X.shape)
        if KS == 2:
            assert np.array_equal(old, new), kind
        My, Mx = mats(h, NEAREST, KS, H1)[0], mats(h, NEAREST, KS, W1)[0]
        w = fw.W(down(My, fw.f64(G), Mx), down(My, np.abs(fw.f64(G)), Mx), KS * KS + 4)
        fw.check("new dX", new, w)
        fw.check("old dX", old, w)
        guards_intact(oo, on, xo, xn)
