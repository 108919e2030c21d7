"""t4k_patch_fwd / _bwd (include/t4k.h, csrc/patch.hip) through the C ABI: conv2d with stride == kernel size, no padding, K 2..32.

The witnesses are tests/f64_witness.py's conv_fwd / conv_df / conv_db / conv_dx with S = K, P = 0 on the image cropped to H0 K x W0 K (conv_dx applies the
reference's tap flip, so it is handed the flipped filter: the textbook dX), with n = K K C1 + 1 roundings for the forward, C0 for dX and N H0 W0 for dF and
dB, and the float64 sum of |terms| as the magnitude.  Every case runs on integers in [-4, 4] - exact in fp32 in any order, so the result must be BIT-EQUAL
and no element can be left out, doubled or taken from the wrong tap - and on floats in +-[0.5, 2) inside the bound, no element excepted.  Outputs are
pre-filled with NaN between guard floats.  The image is (2 K + 3) x 3 K: a remainder on H, an exact W, a 2 x 3 token grid."""
import zlib

import numpy as np
import pytest

import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_conv_geo import I8, OK, ERR_ARG, ERR_UNSUPPORTED, at, guards_intact, last_plan, lcount, operands

pytestmark = pytest.mark.gpu

CASES = [(8, 1, 4, 1), (8, 3, 20, 3), (8, 4, 64, 1), (8, 4, 68, 3), (14, 3, 64, 1), (14, 3, 20, 3), (14, 1, 68, 1), (14, 4, 4, 3),
         (16, 3, 64, 3), (16, 3, 68, 1), (16, 1, 20, 1), (16, 4, 4, 1), (32, 3, 4, 1), (32, 1, 64, 3), (32, 4, 20, 1), (32, 3, 68, 3), (4, 3, 20, 3),
         (16, 3, 6, 1), (14, 3, 5, 1)]     # K, C1, C0, N; the last two: C0 off a multiple of 4, F and dO by dwords beside either gather of I


def plan(h, N, H1, W1, C1, C0, K, aligned):
    out = I8()
    assert h.lib.t4k_patch_plan(N, H1, W1, C1, C0, K, aligned, out) == OK, h.lib.t4k_last_error()
    return list(out)


def witness(kind, a, K):
    """(O, dX, DF, DB): dX is 0 on the rows and columns no patch covers; DF and DB accumulate onto DF0 and DB0"""
    I, F, G = a["I"], a["F"], a["G"]
    N, H0, W0, C0 = G.shape
    Ic = I[:, :H0 * K, :W0 * K]
    wo = fw.conv_fwd(Ic, F, a["B"], K, 0)
    d = fw.conv_dx(G, F[:, ::-1, ::-1, :], H0 * K, W0 * K, K, 0)
    ex, mg = np.zeros(I.shape), np.zeros(I.shape)
    ex[:, :H0 * K, :W0 * K] = d.exact; mg[:, :H0 * K, :W0 * K] = d.mag
    wdf, wdb = fw.conv_df(Ic, G, K, K, 0, acc=a["DF0"]), fw.conv_db(G, acc=a["DB0"])
    n = lambda k: 0 if kind == "int" else k                               # integers: exact equality
    return (fw.W(wo.exact, wo.mag, n(F.shape[0] * K * K + 1)), fw.W(ex, mg, n(C0)), fw.W(wdf.exact, wdf.mag, n(N * H0 * W0)),
            fw.W(wdb.exact, wdb.mag, n(N * H0 * W0)))


def run_case(h, name, N, H1, W1, C1, C0, K, off=0, kinds=("int", "float")):
    """forward, then a whole backward (train = 1, DX and DX2, DB right behind DF) against the witnesses; the plan's paths against the rule, the launches, the
    tokens, the guards, a second run.  off: floats every buffer starts off 16 bytes"""
    H0, W0 = H1 // K, W1 // K
    geo = (N, H1, W1, C1, C0, K)
    pl = plan(h, *geo, 0 if off % 4 else 7)
    vi = int(off % 4 == 0 and (K * C1) % 4 == 0 and (W1 * C1) % 4 == 0); vf = int(off % 4 == 0 and C0 % 4 == 0)
    assert pl[1] == vi | (vf << 1) and pl[3] == vf and pl[4] == vi | (vf << 1) and pl[5] == -(-N * H0 * W0 // 32) and pl[6] == (1 if pl[5] <= 32 else 2), pl
    v = lambda b, y, n: y if b else n
    t_fwd = "patch<%d,%s,%s>" % (pl[0], v(vi, "v4", "v1"), v(vf, "f4", "f1"))
    t_bwd = "patch_dfx%d<%s,%s> %s patch_dx<%d,%s>" % (pl[5], v(vi, "i4", "i1"), v(vf, "d4", "d1"), v(pl[6] == 1, "fold_add", "df_fold"), pl[2], v(vf, "v4", "v1"))
    ndf = C1 * K * K * C0
    nan = lambda n: np.full(n, np.nan, np.float32)
    for kind in kinds:
        a = operands(kind, zlib.crc32(repr((name, kind, geo)).encode()), N, H1, W1, C1, H0, W0, C0, K)
        wo, wdx, wdf, wdb = witness(kind, a, K)
        dI, dF, dB, dG = Dev(a["I"], off), Dev(a["F"], off), Dev(a["B"], off), Dev(a["G"], off)
        dO = Dev(nan(a["G"].size), off)
        l0 = lcount(h)
        h.call("t4k_patch_fwd", dI.p, None, dO.p, dF.p, dB.p, *geo, None)
        assert lcount(h) - l0 == 1 and last_plan(h) == t_fwd, (name, last_plan(h), t_fwd)
        o = dO.get(h, a["G"].shape).copy()
        fw.check("%s %s O" % (name, kind), o, wo)

        def backward():
            dDX, dDX2, dD = Dev(nan(a["I"].size), off), Dev(nan(a["I"].size), off), Dev(np.concatenate([a["DF0"].ravel(), a["DB0"]]), off)
            l0 = lcount(h)
            h.call("t4k_patch_bwd", dI.p, dG.p, dDX.p, dDX2.p, dF.p, dD.p, at(dD, ndf), *geo, 1, None)
            assert lcount(h) - l0 == 3 == pl[7] and last_plan(h) == t_bwd, (name, last_plan(h), t_bwd)
            dx, g = dDX.get(h, a["I"].shape).copy(), dD.get(h, (ndf + C0,)).copy()
            assert np.array_equal(dx, dDX2.get(h, a["I"].shape)), name
            guards_intact(dDX, dDX2, dD)
            return dx, g[:ndf].reshape(a["F"].shape), g[ndf:]

        dx, df, db = backward()
        fw.check("%s %s dX" % (name, kind), dx, wdx)
        assert not dx[:, H0 * K:].any() and not dx[:, :, W0 * K:].any() and not np.signbit(dx[:, H0 * K:]).any()      # the remainder: exactly +0, and written
        fw.check("%s %s dF" % (name, kind), df, wdf)
        fw.check("%s %s dB" % (name, kind), db, wdb)
        if kind == "float":                                             # the same bits on a second run
            dO2 = Dev(nan(a["G"].size), off)
            h.call("t4k_patch_fwd", dI.p, None, dO2.p, dF.p, dB.p, *geo, None)
            assert np.array_equal(dO2.get(h, a["G"].shape), o)
            r = backward()
            assert np.array_equal(r[0], dx) and np.array_equal(r[1], df) and np.array_equal(r[2], db), name
        guards_intact(dO, dI, dF, dB, dG)
        assert np.array_equal(dI.get(h, a["I"].shape), a["I"]) and np.array_equal(dG.get(h, a["G"].shape), a["G"])   # the operands are intact
    return pl


@pytest.mark.parametrize("K,C1,C0,N", CASES, ids=lambda v: str(v))
def test_shapes(t4k, K, C1, C0, N):
    run_case(t4k, "grid", N, 2 * K + 3, 3 * K, C1, C0, K)


@pytest.mark.parametrize("N,H1,W1,C1,C0,slices", [(3, 40, 40, 1, 4, 3), (3, 59, 56, 3, 20, 5)])
def test_token_tiles_and_slices(t4k, N, H1, W1, C1, C0, slices):
    """75 tokens (5 x 5 patches of 8): past a wave's 64 rows, three dF slices; 147 (7 x 7): past the 128-token tile, five slices, the dword paths"""
    assert run_case(t4k, "tokens", N, H1, W1, C1, C0, 8)[5] == slices


def test_every_load_path_is_taken(t4k):
    seen = {tuple(plan(t4k, N, 2 * K + 3, 3 * K, C1, C0, K, 7)[i] for i in (1, 3, 4)) for K, C1, C0, N in CASES}
    assert {(3, 1, 3), (0, 0, 0), (1, 0, 1), (2, 1, 2)} <= seen, seen


@pytest.mark.parametrize("K,C1,C0", [(16, 3, 64), (8, 4, 68), (14, 3, 20)])
def test_pointers_off_16_bytes(t4k, K, C1, C0):
    """every pointer 4 bytes off: the dword paths (asserted in run_case through the plan and the tokens), the same values"""
    run_case(t4k, "off", 3, 2 * K + 3, 3 * K, C1, C0, K, off=1)
    run_case(t4k, "off", 1, 2 * K + 3, 3 * K, C1, C0, K, off=3, kinds=("int",))


def test_backward_forms(t4k):
    """ICOPY; DX == NULL; DF == DB == NULL; train = 0; DX2 == I in place; DB apart from DF (the wave-per-output fold)"""
    h = t4k
    N, H1, W1, C1, C0, K = 3, 19, 24, 3, 20, 8
    geo = (N, H1, W1, C1, C0, K)
    a = operands("float", 11, N, H1, W1, C1, 2, 3, C0, K)
    wo, wdx, wdf, wdb = witness("float", a, K)
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dF, dB, dG = Dev(a["I"]), Dev(a["F"]), Dev(a["B"]), Dev(a["G"])
    dO, dC = Dev(nan(a["G"].size)), Dev(nan(a["I"].size))
    l0 = lcount(h)
    h.call("t4k_patch_fwd", dI.p, dC.p, dO.p, dF.p, dB.p, *geo, None)
    assert lcount(h) - l0 == 1 and last_plan(h).startswith("memcpy patch<")
    assert np.array_equal(dC.get(h, a["I"].shape), a["I"]); fw.check("icopy O", dO.get(h, a["G"].shape), wo)
    # DX == NULL: slabs and fold; DB apart from DF: df_fold
    dDF, dDB, dDX = Dev(a["DF0"]), Dev(a["DB0"]), Dev(nan(a["I"].size))
    l0 = lcount(h)
    h.call("t4k_patch_bwd", dI.p, dG.p, None, dDX.p, dF.p, dDF.p, dDB.p, *geo, 1, None)
    assert lcount(h) - l0 == 2 and last_plan(h).endswith("df_fold") and np.isnan(dDX.get(h, a["I"].shape)).all()
    fw.check("dF alone", dDF.get(h, a["F"].shape), wdf); fw.check("dB alone", dDB.get(h, (C0,)), wdb)
    # DF == DB == NULL, and train = 0 with them given: dX alone, one launch; the gradients bit-unchanged
    dDF, dDB = Dev(a["DF0"]), Dev(a["DB0"])
    for pdf, pdb, train in ((None, None, 1), (dDF.p, dDB.p, 0)):
        dDX = Dev(nan(a["I"].size))
        l0 = lcount(h)
        h.call("t4k_patch_bwd", dI.p, dG.p, dDX.p, None, dF.p, pdf, pdb, *geo, train, None)
        assert lcount(h) - l0 == 1
        fw.check("dX alone", dDX.get(h, a["I"].shape), wdx)
    assert np.array_equal(dDF.get(h, a["F"].shape), a["DF0"]) and np.array_equal(dDB.get(h, (C0,)), a["DB0"])
    assert h.lib.t4k_patch_bwd(dI.p, dG.p, dDX.p, None, dF.p, dDF.p, None, *geo, 1, None) == ERR_ARG      # DF and DB go together
    # DX2 == I, in place: dF | dB read I first
    dI2, dDX, dDF, dDB = Dev(a["I"]), Dev(nan(a["I"].size)), Dev(a["DF0"]), Dev(a["DB0"])
    h.call("t4k_patch_bwd", dI2.p, dG.p, dDX.p, dI2.p, dF.p, dDF.p, dDB.p, *geo, 1, None)
    fw.check("in place dX", dI2.get(h, a["I"].shape), wdx); fw.check("in place dX'", dDX.get(h, a["I"].shape), wdx)
    fw.check("in place dF", dDF.get(h, a["F"].shape), wdf); fw.check("in place dB", dDB.get(h, (C0,)), wdb)
    guards_intact(dI2, dDX, dDF, dDB, dO, dC)


def test_rejections(t4k):
    """a bad argument: T4K_ERR_ARG; outside the admitted set: T4K_ERR_UNSUPPORTED; a text either way, nothing launched, the outputs untouched"""
    h = t4k
    N, H1, W1, C1, C0 = 2, 19, 24, 3, 5
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dF, dB = Dev(np.ones(N * H1 * W1 * C1, np.float32)), Dev(np.ones(C1 * 33 * 33 * C0, np.float32)), Dev(np.ones(C0, np.float32))
    dO, dG, dDX, dDF, dDB = Dev(nan(N * H1 * W1 * C0)), Dev(np.ones(N * H1 * W1 * C0, np.float32)), Dev(nan(N * H1 * W1 * C1)), Dev(nan(C1 * 33 * 33 * C0)), Dev(nan(C0))
    fwd = lambda I=dI.p, O=dO.p, F=dF.p, B=dB.p, g=(N, H1, W1, C1, C0, 8): h.lib.t4k_patch_fwd(I, None, O, F, B, *g, None)
    bwd = lambda I=dI.p, G=dG.p, F=dF.p, g=(N, H1, W1, C1, C0, 8): h.lib.t4k_patch_bwd(I, G, dDX.p, None, F, dDF.p, dDB.p, *g, 1, None)
    l0 = lcount(h)
    for g, code, text in [((N, H1, W1, C1, C0, 1), ERR_UNSUPPORTED, b"not supported"), ((N, H1, W1, C1, C0, 33), ERR_UNSUPPORTED, b"not supported"),
                          ((N, H1, W1, C1, C0, 20), ERR_UNSUPPORTED, b"does not fit"), ((0, H1, W1, C1, C0, 8), ERR_ARG, b"extent"),
                          ((N, H1, W1, C1, -1, 8), ERR_ARG, b"extent")]:
        assert fwd(g=g) == code and text in h.lib.t4k_last_error(), (g, h.lib.t4k_last_error())
        assert bwd(g=g) == code and text in h.lib.t4k_last_error(), (g, h.lib.t4k_last_error())
    assert fwd(I=None) == ERR_ARG and fwd(O=None) == ERR_ARG and fwd(F=None) == ERR_ARG and fwd(B=None) == ERR_ARG
    assert bwd(I=None) == ERR_ARG and bwd(G=None) == ERR_ARG and bwd(F=None) == ERR_ARG
    assert lcount(h) == l0
    for d in (dO, dDX, dDF, dDB):
        assert np.isnan(d.get(h, (d.n,))).all()
