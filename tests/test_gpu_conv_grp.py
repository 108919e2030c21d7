"""t4k_conv2d_grp_fwd / _bwd (include/t4k.h, csrc/conv_group.hip) through the C ABI: grouped and depthwise conv2d with run-time K, stride,
padding, dilation and group count.

The witness is torch on the CPU in float64 - torch.nn.functional.conv2d(groups=G) and its autograd - on tensors permuted from NHWC / T4(C1 / G, K, K, C0).
Every case runs on two kinds of operands (tests/test_gpu_conv_geo.py's, whose helpers are imported):
  integers in [-4, 4]: every product and partial sum is an integer far below 2^24, exact in fp32 in ANY order - the result must be BIT-EQUAL to the witness;
  floats in +-[0.5, 2): inside tests/f64_witness.py's per-element bound with n = K K Cg1 + 1 (forward), K K Cg0 (dX), pixels + 1 (dF, dB), no element excepted.
Outputs are pre-filled with NaN between guard floats.  Two checks do not involve torch: G = 1 against t4k_conv2d_geo_fwd / _bwd, and a grouped call against
t4k_conv2d_geo_fwd / _bwd on the block-diagonal dense filter - the only way the library had to compute such a layer - bit for bit on integer operands."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_conv_geo import at, extent, guards_intact, last_plan, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8

GEOS = [(1, 1, 0, 1), (2, 2, 0, 1), (3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 2, 2), (4, 2, 1, 1), (5, 2, 2, 1), (7, 4, 6, 1), (3, 4, 0, 1)]
IMAGES = [(11, 9), (8, 13)]
GROUPS = [(1, 1, 1), (3, 3, 3), (4, 4, 4), (33, 33, 33), (64, 64, 64), (4, 8, 4), (3, 6, 3), (6, 4, 2), (8, 8, 2), (64, 64, 2), (12, 20, 4)]   # (C1, C0, G)


def plan(h, N, H1, W1, C1, C0, K, S, P, D, G, aligned=1):
    out = I8()
    assert h.lib.t4k_conv2d_grp_plan(N, H1, W1, C1, C0, K, S, P, D, G, aligned, out) == OK, h.lib.t4k_last_error()
    return list(out)


def operands(kind, seed, N, H1, W1, C1, H0, W0, C0, K, G):
    rng = np.random.default_rng(seed)
    if kind == "int":
        g = lambda *sh: rng.integers(-4, 5, size=sh).astype(np.float32)
    else:
        g = lambda *sh: (rng.uniform(0.5, 2.0, size=sh) * rng.choice([-1.0, 1.0], size=sh)).astype(np.float32)
    return dict(I=g(N, H1, W1, C1), F=g(C1 // G, K, K, C0), B=g(C0), G=g(N, H0, W0, C0), DF0=g(C1 // G, K, K, C0), DB0=g(C0))


def _torch_pass(I, F, B, Gr, S, P, D, G):
    x = torch.tensor(I, dtype=torch.float64).permute(0, 3, 1, 2).contiguous().requires_grad_()
    w = torch.tensor(F, dtype=torch.float64).permute(3, 0, 1, 2).contiguous().requires_grad_()         # weight[c0][cg][ky][kx] = F[cg, ky, kx, c0]
    o = torch.nn.functional.conv2d(x, w, torch.tensor(B, dtype=torch.float64), stride=S, padding=P, dilation=D, groups=G)
    o.backward(torch.tensor(Gr, dtype=torch.float64).permute(0, 3, 1, 2))
    return (o.detach().permute(0, 2, 3, 1).numpy(), x.grad.permute(0, 2, 3, 1).numpy(), w.grad.permute(1, 2, 3, 0).numpy())


def witness(kind, a, K, S, P, D, G):
    """(O, dX, DF, DB) witnesses of the float64 forward and autograd backward; the magnitudes are the same pass on absolute values"""
    o, dx, df = _torch_pass(a["I"], a["F"], a["B"], a["G"], S, P, D, G)
    Cg1, C0 = a["F"].shape[0], a["F"].shape[3]
    npix = a["G"].size // C0
    db = fw.f64(a["G"]).reshape(-1, C0).sum(0)
    df = df + fw.f64(a["DF0"]); db = db + fw.f64(a["DB0"])                 # train = 1 accumulates into the gradients it finds
    if kind == "int":
        Wd = lambda e: fw.W(e, 0.0, 0)
        return Wd(o), Wd(dx), Wd(df), Wd(db)
    mo, mdx, mdf = _torch_pass(np.abs(a["I"]), np.abs(a["F"]), np.abs(a["B"]), np.abs(a["G"]), S, P, D, G)
    mdb = np.abs(fw.f64(a["G"])).reshape(-1, C0).sum(0)
    return (fw.W(o, mo, K * K * Cg1 + 1), fw.W(dx, mdx, K * K * (C0 // G)), fw.W(df, mdf + np.abs(fw.f64(a["DF0"])), npix + 1),
            fw.W(db, mdb + np.abs(fw.f64(a["DB0"])), npix + 1))


def tokens(pl):
    v = lambda b: "v4" if b else "v1"
    return ("%s<%s>" % ("grp_dw" if pl[0] == 1 else "grp", v(pl[1])), "grp_dfx%d" % pl[5], "fold_add" if pl[6] == 1 else "df_fold", "grp_dx<%s>" % v(pl[2] == 4))


def run_case(h, name, N, H1, W1, C1, C0, G, K, S, P, D, off=0, kinds=("int", "float"), split_grads=False):
    """forward, then a whole backward (train = 1, DX and DX2), each against the witness; launches, tokens against the plan entry, guards, a second run.
    off: floats EVERY buffer starts off 16 bytes"""
    H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
    geo = (N, H1, W1, C1, H0, W0, C0, K, S, P, D, G)
    pl = plan(h, N, H1, W1, C1, C0, K, S, P, D, G, (0 if off % 4 else 1) | (2 if split_grads else 0))
    t_fwd, t_df, t_fold, t_dx = tokens(pl)
    ndf = (C1 // G) * K * K * C0
    nan = lambda n: np.full(n, np.nan, np.float32)
    for kind in kinds:
        a = operands(kind, zlib.crc32(repr((name, kind, geo)).encode()), N, H1, W1, C1, H0, W0, C0, K, G)
        wo, wdx, wdf, wdb = witness(kind, a, K, S, P, D, G)
        dI, dF, dB, dG = Dev(a["I"], off), Dev(a["F"], off), Dev(a["B"], off), Dev(a["G"], off)
        dO = Dev(nan(N * H0 * W0 * C0), off)
        l0 = lcount(h)
        h.call("t4k_conv2d_grp_fwd", dI.p, None, dO.p, dF.p, dB.p, *geo, None)
        assert lcount(h) - l0 == 1 and last_plan(h) == t_fwd, (name, last_plan(h), t_fwd)
        fw.check("%s %s O" % (name, kind), dO.get(h, wo.exact.shape), wo)

        def backward():
            dDX, dDX2 = Dev(nan(a["I"].size), off), Dev(nan(a["I"].size), off)
            if split_grads:
                dDF, dDB = Dev(a["DF0"], off), Dev(a["DB0"], off)
                pdf, pdb = dDF.p, dDB.p
            else:                                                        # DB right behind DF, as a layer's gradient block: k_fold_add can serve
                dDF = dDB = Dev(np.concatenate([a["DF0"].ravel(), a["DB0"]]), off)
                pdf, pdb = dDF.p, at(dDF, ndf)
            l0 = lcount(h)
            h.call("t4k_conv2d_grp_bwd", dI.p, dG.p, dDX.p, dDX2.p, dF.p, pdf, pdb, *geo, 1, None)
            nl = lcount(h) - l0
            assert nl == 3 == pl[7] and last_plan(h) == "%s %s %s" % (t_df, t_fold, t_dx), (name, nl, last_plan(h))
            dx, dx2 = dDX.get(h, a["I"].shape), dDX2.get(h, a["I"].shape)
            if split_grads:
                df, db = dDF.get(h, a["F"].shape), dDB.get(h, (C0,))
            else:
                g = dDF.get(h, (ndf + C0,)); df, db = g[:ndf].reshape(a["F"].shape), g[ndf:]
            guards_intact(dDX, dDX2, dDF, dDB)
            return dx, dx2, df, db

        dx, dx2, df, db = backward()
        fw.check("%s %s dX" % (name, kind), dx, wdx)
        assert np.array_equal(dx, dx2), name
        fw.check("%s %s dF" % (name, kind), df, wdf)
        fw.check("%s %s dB" % (name, kind), db, wdb)
        if kind == "float":                                             # the same bits on a second run: fixed summation order
            dO2 = Dev(nan(N * H0 * W0 * C0), off)
            h.call("t4k_conv2d_grp_fwd", dI.p, None, dO2.p, dF.p, dB.p, *geo, None)
            assert np.array_equal(dO2.get(h, wo.exact.shape), dO.get(h, wo.exact.shape))
            r = backward()
            assert np.array_equal(r[0], dx) and np.array_equal(r[2], df) and np.array_equal(r[3], db), name
        guards_intact(dO, dI, dF, dB, dG)
        assert np.array_equal(dI.get(h, a["I"].shape), a["I"]) and np.array_equal(dG.get(h, a["G"].shape), a["G"])   # the operands are intact
    return pl


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "k%ds%dp%dd%d" % g)
def test_geometries(t4k, geo):
    """every geometry x every (C1, C0, G): depthwise on dwords and on 16 bytes, ragged channels, multipliers 2 (four dwords of I), groups of 3 -> 2, 4 -> 4 (one
    dword of I for four outputs), 32 -> 32 and 3 -> 5 (a thread's four channels would straddle groups); the images alternate, floats on one of them"""
    K, S, P, D = geo
    for i, (C1, C0, G) in enumerate(GROUPS):
        H1, W1 = IMAGES[(i + GEOS.index(geo)) % 2]
        run_case(t4k, "grp", 3, H1, W1, C1, C0, G, K, S, P, D)
        if (C1, C0, G) in ((3, 3, 3), (64, 64, 64), (4, 8, 4), (12, 20, 4)):
            H1, W1 = IMAGES[(i + GEOS.index(geo) + 1) % 2]
            run_case(t4k, "grp", 3, H1, W1, C1, C0, G, K, S, P, D, kinds=("int",))


def test_load_paths_are_the_plans(t4k):
    """which engine and load path each channel triple takes, aligned: asserted through the plan (run_case asserts the tokens against it)"""
    want = {(1, 1, 1): (1, 0, 1), (3, 3, 3): (1, 0, 1), (4, 4, 4): (1, 1, 4), (33, 33, 33): (1, 0, 1), (64, 64, 64): (1, 1, 4), (4, 8, 4): (1, 3, 1),
            (3, 6, 3): (1, 0, 1), (6, 4, 2): (2, 0, 1), (8, 8, 2): (2, 2, 1), (64, 64, 2): (2, 2, 1), (12, 20, 4): (2, 0, 1)}
    for (C1, C0, G), w in want.items():
        assert tuple(plan(t4k, 3, 11, 9, C1, C0, 3, 1, 1, 1, G)[:3]) == w, (C1, C0, G)
        assert tuple(plan(t4k, 3, 11, 9, C1, C0, 3, 1, 1, 1, G, 0)[1:3]) == (0, 1)


@pytest.mark.parametrize("npix,H1,W1", [(1, 2, 2), (63, 14, 18), (65, 10, 26), (257, 2, 514)])
def test_pixel_counts(t4k, npix, H1, W1):
    """N H0 W0 = 1, 63, 65, 257 under 2x2 / 2: one pixel, one and two slices either side of 64, a row of 257 tiles a pixel high"""
    assert extent(H1, 2, 2, 0, 1) * extent(W1, 2, 2, 0, 1) == npix
    pl = run_case(t4k, "npix", 1, H1, W1, 4, 4, 4, 2, 2, 0, 1)
    assert pl[5] == -(-npix // 32)
    run_case(t4k, "npix", 1, H1, W1, 3, 6, 3, 2, 2, 0, 1, kinds=("int",))
    run_case(t4k, "npix", 1, H1, W1, 6, 4, 2, 2, 2, 0, 1, kinds=("int",))


def test_stride_above_the_window(t4k):
    """(3, 4, 0, 1) and (1, 2, 0, 1): input pixels nothing reads - their dX is exactly 0, and written (the NaN fill is gone)"""
    for K, S in ((3, 4), (1, 2)):
        for C1, C0, G in ((4, 4, 4), (6, 4, 2)):
            N, H1, W1 = 2, 11, 9
            H0, W0 = extent(H1, K, S, 0, 1), extent(W1, K, S, 0, 1)
            a = operands("float", 7, N, H1, W1, C1, H0, W0, C0, K, G)
            dI, dG, dF, dDX = Dev(a["I"]), Dev(a["G"]), Dev(a["F"]), Dev(np.full(a["I"].size, np.nan, np.float32))
            l0 = lcount(t4k)
            t4k.call("t4k_conv2d_grp_bwd", dI.p, dG.p, dDX.p, None, dF.p, None, None, N, H1, W1, C1, H0, W0, C0, K, S, 0, 1, G, 0, None)
            assert lcount(t4k) - l0 == 1
            dx = dDX.get(t4k, a["I"].shape)
            fw.check("unread dX", dx, witness("float", a, K, S, 0, 1, G)[1])
            read = np.zeros((H1, W1), bool)
            for i in range(H0):
                for j in range(W0):
                    read[i * S:i * S + K, j * S:j * S + K] = True
            assert (~read).sum() > 0 and not np.isnan(dx).any()
            assert np.all(dx[:, ~read, :] == 0.0)


@pytest.mark.parametrize("C1,C0,G", [(4, 4, 4), (64, 64, 64), (4, 8, 4), (8, 8, 2)])
def test_pointers_off_16_bytes(t4k, C1, C0, G):
    """every pointer 4 bytes off 16-byte alignment: the dword paths, asserted through the plan and the tokens"""
    pl = plan(t4k, 3, 11, 9, C1, C0, 3, 2, 1, 1, G, 0)
    assert pl[1] == 0 and pl[2] == 1
    assert plan(t4k, 3, 11, 9, C1, C0, 3, 2, 1, 1, G, 1)[1] != 0
    run_case(t4k, "off", 3, 11, 9, C1, C0, G, 3, 2, 1, 1, off=1)
    run_case(t4k, "off", 3, 8, 13, C1, C0, G, 3, 1, 2, 2, off=3, kinds=("int",))


def test_one_pointer_off_16_bytes(t4k):
    """only I, only dO, only F, only O / DX 4 bytes off on a 64-channel depthwise layer: no 16-byte access may start there - the engines through
    t4k_conv_last_plan"""
    N, H1, W1, C, K, S, P, D = 3, 11, 9, 64, 3, 2, 1, 1
    H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
    geo = (N, H1, W1, C, H0, W0, C, K, S, P, D, C)
    a = operands("int", 3, N, H1, W1, C, H0, W0, C, K, C)
    wo, wdx, wdf, wdb = witness("int", a, K, S, P, D, C)
    ns = plan(t4k, N, H1, W1, C, C, K, S, P, D, C, 2)[5]
    for which in "IGFO":
        o = lambda k: 1 if k == which else 0
        dI, dF, dB, dG = Dev(a["I"], o("I")), Dev(a["F"], o("F")), Dev(a["B"]), Dev(a["G"], o("G"))
        dO, dDX, dDF, dDB = Dev(np.zeros(a["G"].size, np.float32), o("O")), Dev(np.zeros(a["I"].size, np.float32), o("O")), Dev(a["DF0"]), Dev(a["DB0"])
        t4k.call("t4k_conv2d_grp_fwd", dI.p, None, dO.p, dF.p, dB.p, *geo, None)
        assert last_plan(t4k) == ("grp_dw<v4>" if which == "G" else "grp_dw<v1>"), (which, last_plan(t4k))
        fw.check("O", dO.get(t4k, wo.exact.shape), wo)
        t4k.call("t4k_conv2d_grp_bwd", dI.p, dG.p, dDX.p, None, dF.p, dDF.p, dDB.p, *geo, 1, None)
        assert last_plan(t4k) == "grp_dfx%d df_fold grp_dx<v1>" % ns, (which, last_plan(t4k))
        fw.check("dX", dDX.get(t4k, a["I"].shape), wdx); fw.check("dF", dDF.get(t4k, a["F"].shape), wdf); fw.check("dB", dDB.get(t4k, (C,)), wdb)
        guards_intact(dO, dDX, dDF, dDB)


def test_slices_and_both_folds(t4k):
    """one slice, two, and the batch with more than 32 - found through the plan entry: k_fold_add up to 32 slices (DB right behind DF), k_conv_df_fold above
    and for a DB elsewhere"""
    assert run_case(t4k, "fold", 1, 5, 6, 4, 4, 4, 3, 1, 1, 1)[5:7] == [1, 1]
    assert run_case(t4k, "fold", 1, 8, 8, 4, 8, 4, 3, 1, 1, 1)[5:7] == [2, 1]
    N = next(n for n in range(1, 64) if plan(t4k, n, 11, 9, 4, 4, 3, 1, 1, 1, 4)[5] > 32)
    assert N * 11 * 9 < 4000
    pl = run_case(t4k, "fold", N, 11, 9, 4, 4, 4, 3, 1, 1, 1)
    assert pl[5] > 32 and pl[6] == 2
    pl = run_case(t4k, "fold", N - 1, 11, 9, 4, 4, 4, 3, 1, 1, 1, kinds=("float",))
    assert pl[5] <= 32 and pl[6] == 1
    run_case(t4k, "fold", 3, 11, 9, 4, 8, 4, 3, 2, 1, 1, split_grads=True)   # few slices, DB not behind DF: df_fold (asserted in run_case)
    run_case(t4k, "fold", N, 11, 9, 12, 20, 4, 3, 1, 1, 1, split_grads=True, kinds=("float",))


def test_backward_forms(t4k):
    """DX == NULL, DF == DB == NULL, train = 0, DX2 == DX, DX2 == I in place, ICOPY"""
    h = t4k
    N, H1, W1, C1, C0, G, K, S, P, D = 3, 11, 9, 8, 8, 8, 3, 2, 1, 1
    H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
    geo = (N, H1, W1, C1, H0, W0, C0, K, S, P, D, G)
    a = operands("float", 11, N, H1, W1, C1, H0, W0, C0, K, G)
    wo, wdx, wdf, wdb = witness("float", a, K, S, P, D, G)
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dF, dB, dG = Dev(a["I"]), Dev(a["F"]), Dev(a["B"]), Dev(a["G"])
    # ICOPY: a copy command beside the one launch
    dO, dC = Dev(nan(wo.exact.size)), Dev(nan(a["I"].size))
    l0 = lcount(h)
    h.call("t4k_conv2d_grp_fwd", dI.p, dC.p, dO.p, dF.p, dB.p, *geo, None)
    assert lcount(h) - l0 == 1 and last_plan(h) == "memcpy grp_dw<v4>"
    assert np.array_equal(dC.get(h, a["I"].shape), a["I"]); fw.check("icopy O", dO.get(h, wo.exact.shape), wo)
    # DX == NULL: slabs and fold
    dDF, dDB, dDX = Dev(a["DF0"]), Dev(a["DB0"]), Dev(nan(a["I"].size))
    l0 = lcount(h)
    h.call("t4k_conv2d_grp_bwd", dI.p, dG.p, None, dDX.p, dF.p, dDF.p, dDB.p, *geo, 1, None)
    assert lcount(h) - l0 == 2 and np.isnan(dDX.get(h, a["I"].shape)).all()
    fw.check("dF alone", dDF.get(h, a["F"].shape), wdf); fw.check("dB alone", dDB.get(h, (C0,)), wdb)
    # DF == DB == NULL and train = 0: dX alone, one launch; the gradients bit-unchanged
    for train in (1, 0):
        l0 = lcount(h)
        h.call("t4k_conv2d_grp_bwd", dI.p, dG.p, dDX.p, None, dF.p, None, None, *geo, train, None)
        assert lcount(h) - l0 == 1 and last_plan(h) == "grp_dx<v4>"
        fw.check("dX alone", dDX.get(h, a["I"].shape), wdx)
    dDF, dDB = Dev(a["DF0"]), Dev(a["DB0"])
    l0 = lcount(h)
    h.call("t4k_conv2d_grp_bwd", dI.p, dG.p, dDX.p, None, dF.p, dDF.p, dDB.p, *geo, 0, None)
    assert lcount(h) - l0 == 1
    assert np.array_equal(dDF.get(h, a["F"].shape), a["DF0"]) and np.array_equal(dDB.get(h, (C0,)), a["DB0"])
    assert h.lib.t4k_conv2d_grp_bwd(dI.p, dG.p, dDX.p, None, dF.p, dDF.p, None, *geo, 1, None) == ERR_ARG      # DF and DB go together
    # DX2 == DX
    dDX = Dev(nan(a["I"].size))
    h.call("t4k_conv2d_grp_bwd", dI.p, dG.p, dDX.p, dDX.p, dF.p, None, None, *geo, 0, None)
    fw.check("DX2 == DX", dDX.get(h, a["I"].shape), wdx)
    # DX2 == I, in place: dF | dB read I first
    dI2, dDX, dDF, dDB = Dev(a["I"]), Dev(nan(a["I"].size)), Dev(a["DF0"]), Dev(a["DB0"])
    h.call("t4k_conv2d_grp_bwd", dI2.p, dG.p, dDX.p, dI2.p, dF.p, dDF.p, dDB.p, *geo, 1, None)
    fw.check("in place dX", dI2.get(h, a["I"].shape), wdx); fw.check("in place dX'", dDX.get(h, a["I"].shape), wdx)
    fw.check("in place dF", dDF.get(h, a["F"].shape), wdf); fw.check("in place dB", dDB.get(h, (C0,)), wdb)
    guards_intact(dI2, dDX, dDF, dDB, dO, dC)


def test_rejections(t4k):
    """a bad argument: T4K_ERR_ARG; an inadmissible geometry or group count: T4K_ERR_UNSUPPORTED; a text either way, nothing launched, the outputs untouched"""
    h = t4k
    N, H1, W1, C1, C0 = 2, 8, 8, 4, 8
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dF, dB = Dev(np.ones(N * H1 * W1 * C1, np.float32)), Dev(np.ones(C1 * 49 * C0, np.float32)), Dev(np.ones(C0, np.float32))
    dO, dG, dDX, dDF, dDB = Dev(nan(N * 64 * C0)), Dev(np.ones(N * 64 * C0, np.float32)), Dev(nan(N * H1 * W1 * C1)), Dev(nan(C1 * 49 * C0)), Dev(nan(C0))
    bad = [((3, 2, 1, 1, 4, 5, 4), ERR_ARG, b"gives 4x4"), ((3, 2, 1, 1, 3, 4, 4), ERR_ARG, b"gives 4x4"), ((8, 1, 3, 1, 7, 7, 4), ERR_UNSUPPORTED, b"not supported"),
           ((3, 5, 1, 1, 2, 2, 4), ERR_UNSUPPORTED, b"not supported"), ((3, 1, 1, 5, 1, 1, 4), ERR_UNSUPPORTED, b"not supported"),
           ((3, 1, 3, 1, 12, 12, 4), ERR_UNSUPPORTED, b"not supported"), ((7, 1, 0, 2, 1, 1, 4), ERR_UNSUPPORTED, b"does not fit"),
           ((3, 2, 1, 1, 4, 4, 0), ERR_UNSUPPORTED, b"groups=0"), ((3, 2, 1, 1, 4, 4, -1), ERR_UNSUPPORTED, b"groups=-1"),
           ((3, 2, 1, 1, 4, 4, 3), ERR_UNSUPPORTED, b"groups=3"), ((3, 2, 1, 1, 4, 4, 8), ERR_UNSUPPORTED, b"groups=8")]
    for (K, S, P, D, H0, W0, G), code, text in bad:
        l0 = lcount(h)
        assert h.lib.t4k_conv2d_grp_fwd(dI.p, None, dO.p, dF.p, dB.p, N, H1, W1, C1, H0, W0, C0, K, S, P, D, G, None) == code, (K, S, P, D, G)
        assert text in h.lib.t4k_last_error(), h.lib.t4k_last_error()
        assert h.lib.t4k_conv2d_grp_bwd(dI.p, dG.p, dDX.p, None, dF.p, dDF.p, dDB.p, N, H1, W1, C1, H0, W0, C0, K, S, P, D, G, 1, None) == code
        assert text in h.lib.t4k_last_error() and lcount(h) == l0
    assert h.lib.t4k_conv2d_grp_fwd(dI.p, None, dO.p, dF.p, dB.p, N, H1, W1, C1, 4, 4, 6, 3, 2, 1, 1, 4, None) == ERR_UNSUPPORTED     # C0 % G
    good = (N, H1, W1, C1, 4, 4, C0, 3, 2, 1, 1, 4)
    assert h.lib.t4k_conv2d_grp_fwd(None, None, dO.p, dF.p, dB.p, *good, None) == ERR_ARG
    assert h.lib.t4k_conv2d_grp_fwd(dI.p, None, dO.p, dF.p, None, *good, None) == ERR_ARG
    assert h.lib.t4k_conv2d_grp_bwd(dI.p, None, dDX.p, None, dF.p, dDF.p, dDB.p, *good, 1, None) == ERR_ARG
    assert h.lib.t4k_conv2d_grp_fwd(dI.p, None, dO.p, dF.p, dB.p, 0, H1, W1, C1, 4, 4, C0, 3, 2, 1, 1, 4, None) == ERR_ARG
    for d in (dO, dDX, dDF, dDB):
        assert np.isnan(d.get(h, (d.n,))).all()


def _both(h, a, geo_g, dense_F, G):
    """the grouped entries on a["F"] and the dense run-time-geometry entries on dense_F, same tensors otherwise: (O, dX, dF, dB) of each"""
    N, H1, W1, C1, H0, W0, C0, K, S, P, D = geo_g
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dB, dG = Dev(a["I"]), Dev(a["B"]), Dev(a["G"])
    res = []
    for entry, F, tail in (("grp", a["F"], (G,)), ("geo", dense_F, ())):
        dF, dO, dDX = Dev(F), Dev(nan(a["G"].size)), Dev(nan(a["I"].size))
        dDF, dDB = Dev(np.zeros(F.size, np.float32)), Dev(a["DB0"])
        h.call("t4k_conv2d_%s_fwd" % entry, dI.p, None, dO.p, dF.p, dB.p, *geo_g, *tail, None)
        assert last_plan(h).startswith(entry)
        h.call("t4k_conv2d_%s_bwd" % entry, dI.p, dG.p, dDX.p, None, dF.p, dDF.p, dDB.p, *geo_g, *tail, 1, None)
        assert entry + "_dx<" in last_plan(h)
        res.append((dO.get(h, a["G"].shape), dDX.get(h, a["I"].shape), dDF.get(h, F.shape), dDB.get(h, (C0,))))
        guards_intact(dO, dDX, dDF, dDB)
    return res


@pytest.mark.parametrize("C1,C0", [(3, 5), (4, 8), (64, 64)])
@pytest.mark.parametrize("geo", [(3, 2, 1, 1), (3, 1, 2, 2), (5, 1, 2, 1)], ids=lambda g: "k%ds%dp%dd%d" % g)
def test_g_1_beside_the_dense_entries(t4k, geo, C1, C0):
    """G = 1, integer operands: forward, dX, dF and dB bit-equal to t4k_conv2d_geo_fwd / _bwd on the same filter"""
    K, S, P, D = geo
    N, H1, W1 = 3, 11, 9
    H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
    a = operands("int", zlib.crc32(repr((geo, C1, C0)).encode()), N, H1, W1, C1, H0, W0, C0, K, 1)
    g, d = _both(t4k, a, (N, H1, W1, C1, H0, W0, C0, K, S, P, D), a["F"], 1)
    for x, y, what in zip(g, d, ("O", "dX", "dF", "dB")):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("C1,C0,G", [(4, 4, 4), (64, 64, 64), (4, 8, 4), (6, 4, 2), (8, 8, 2), (12, 20, 4)])
@pytest.mark.parametrize("geo", [(3, 1, 1, 1), (3, 2, 1, 1), (5, 2, 4, 2)], ids=lambda g: "k%ds%dp%dd%d" % g)
def test_beside_the_block_diagonal_dense_filter(t4k, geo, C1, C0, G):
    """a grouped call against t4k_conv2d_geo_fwd / _bwd on the dense filter that is zero outside the groups' blocks - how such a layer had to be computed:
    O, dX and dB bit-equal on integer operands, dF bit-equal inside the blocks (the dense call also fills the blocks' outside, which no grouped layer has)"""
    K, S, P, D = geo
    N, H1, W1 = 3, 11, 9
    H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
    Cg1, Cg0 = C1 // G, C0 // G
    a = operands("int", zlib.crc32(repr((geo, C1, C0, G)).encode()), N, H1, W1, C1, H0, W0, C0, K, G)
    dense = np.zeros((C1, K, K, C0), np.float32)
    for g in range(G):
        dense[g * Cg1:(g + 1) * Cg1, :, :, g * Cg0:(g + 1) * Cg0] = a["F"][:, :, :, g * Cg0:(g + 1) * Cg0]
    (o, dx, df, db), (o2, dx2, df2, db2) = _both(t4k, a, (N, H1, W1, C1, H0, W0, C0, K, S, P, D), dense, G)
    assert np.array_equal(o, o2) and np.array_equal(dx, dx2) and np.array_equal(db, db2)
    for g in range(G):
        assert np.array_equal(df[:, :, :, g * Cg0:(g + 1) * Cg0], df2[g * Cg1:(g + 1) * Cg1, :, :, g * Cg0:(g + 1) * Cg0]), g
