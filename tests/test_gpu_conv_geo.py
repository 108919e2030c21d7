"""t4k_conv2d_geo_fwd / _bwd (include/t4k.h, csrc/conv_geo.hip) through the C ABI: conv2d with run-time K, stride, padding, dilation.

The witness is torch on the CPU in float64 - torch.nn.functional.conv2d(stride, padding, dilation) and its autograd - on tensors permuted from
NHWC / T4(C1, K, K, C0).  Every case runs on two kinds of operands:
  integers in [-4, 4]: every product and partial sum is an integer far below 2^24, exact in fp32 in ANY order - the result must be BIT-EQUAL to
      the witness, so no element can be left out, doubled or taken from the wrong tap;
  floats in +-[0.5, 2): inside tests/f64_witness.py's per-element bound C_SUM n 2^-24 mag + n 2^-126 (n = the roundings behind the element: the
      products of one sum plus the bias / the accumulated gradient; mag = the same op on absolute values), no element excepted.
Outputs are pre-filled with NaN between guard floats (Dev of tests/test_gpu_bcast.py): an element that was not written shows, and so does a
store outside the tensor.  dX is the TEXTBOOK gradient (autograd's), not the reference's rotated-filter dX of t4k_conv2d_bwd - the last test
lays the two side by side."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import f64_witness as fw
from test_gpu_bcast import Dev

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8

GEOS = [(1, 2, 0, 1), (2, 1, 0, 1), (2, 2, 0, 1), (3, 2, 1, 1), (3, 1, 0, 1), (3, 1, 2, 2), (3, 2, 2, 2), (3, 3, 1, 1), (3, 4, 0, 1), (3, 1, 4, 4),
        (4, 1, 1, 1), (5, 2, 2, 1), (5, 1, 4, 2), (6, 2, 2, 1), (6, 3, 5, 1), (7, 1, 3, 1), (7, 2, 3, 1), (7, 4, 6, 1)]
IMAGES = [(11, 9), (8, 13)]
CHANNELS = [(1, 1), (3, 5), (4, 8), (33, 31), (64, 64)]


def lcount(h):
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return int(h.lib.t4k_launch_count())


def last_plan(h):
    h.lib.t4k_conv_last_plan.restype = ctypes.c_char_p
    return h.lib.t4k_conv_last_plan().decode()


def plan(h, N, H1, W1, C1, C0, K, S, P, D, aligned=1):
    out = I8()
    assert h.lib.t4k_conv2d_geo_plan(N, H1, W1, C1, C0, K, S, P, D, aligned, out) == OK, h.lib.t4k_last_error()
    return list(out)


def extent(H1, K, S, P, D):
    return (H1 + 2 * P - D * (K - 1) - 1) // S + 1


def operands(kind, seed, N, H1, W1, C1, H0, W0, C0, K):
    rng = np.random.default_rng(seed)
    if kind == "int":
        g = lambda *sh: rng.integers(-4, 5, size=sh).astype(np.float32)
    else:
        g = lambda *sh: (rng.uniform(0.5, 2.0, size=sh) * rng.choice([-1.0, 1.0], size=sh)).astype(np.float32)
    return dict(I=g(N, H1, W1, C1), F=g(C1, K, K, C0), B=g(C0), G=g(N, H0, W0, C0), DF0=g(C1, K, K, C0), DB0=g(C0))


def _torch_pass(I, F, B, G, S, P, D):
    x = torch.tensor(I, dtype=torch.float64).permute(0, 3, 1, 2).contiguous().requires_grad_()
    w = torch.tensor(F, dtype=torch.float64).permute(3, 0, 1, 2).contiguous().requires_grad_()
    o = torch.nn.functional.conv2d(x, w, torch.tensor(B, dtype=torch.float64), stride=S, padding=P, dilation=D)
    o.backward(torch.tensor(G, dtype=torch.float64).permute(0, 3, 1, 2))
    return (o.detach().permute(0, 2, 3, 1).numpy(), x.grad.permute(0, 2, 3, 1).numpy(), w.grad.permute(1, 2, 3, 0).numpy())


def witness(kind, a, K, S, P, D):
    """(O, dX, DF, DB) witnesses of the float64 forward and autograd backward; the magnitudes are the same pass on absolute values"""
    o, dx, df = _torch_pass(a["I"], a["F"], a["B"], a["G"], S, P, D)
    C1, C0 = a["F"].shape[0], a["F"].shape[3]
    npix = a["G"].size // C0
    db = fw.f64(a["G"]).reshape(-1, C0).sum(0)
    df = df + fw.f64(a["DF0"]); db = db + fw.f64(a["DB0"])                 # train = 1 accumulates into the gradients it finds
    if kind == "int":
        Wd = lambda e: fw.W(e, 0.0, 0)
        return Wd(o), Wd(dx), Wd(df), Wd(db)
    mo, mdx, mdf = _torch_pass(np.abs(a["I"]), np.abs(a["F"]), np.abs(a["B"]), np.abs(a["G"]), S, P, D)
    mdb = np.abs(fw.f64(a["G"])).reshape(-1, C0).sum(0)
    return (fw.W(o, mo, K * K * C1 + 1), fw.W(dx, mdx, K * K * C0), fw.W(df, mdf + np.abs(fw.f64(a["DF0"])), npix + 1),
            fw.W(db, mdb + np.abs(fw.f64(a["DB0"])), npix + 1))


def guards_intact(*devs):
    for d in devs:
        t = d.t.cpu().numpy()
        assert not t[:d.off].any() and not t[d.off + d.n:].any(), "a store outside the tensor"


def at(dev, k):
    return ctypes.c_void_p(dev.t.data_ptr() + 4 * (dev.off + k))


def tokens(pl):
    v = lambda b: "v4" if b else "v1"
    fwd = "geo<%d,%s,%s>" % (pl[0], v(pl[1] & 1), "f4" if pl[1] & 2 else "f1")
    df = "geo_dfx%d<%s>" % (pl[5], "tap" if pl[4] & 2 else "rows,d4" if pl[4] & 1 else "rows,d1")
    dx = "geo_dx<%d,%s>" % (pl[2], v(pl[3]))
    return fwd, df, "fold_add" if pl[6] == 1 else "df_fold", dx


def run_case(h, name, N, H1, W1, C1, C0, K, S, P, D, off=0, kinds=("int", "float"), split_grads=False):
    """forward, then a whole backward (train = 1, DX and DX2), each against the witness; launches, tokens, guards, a second run.
    off: floats every buffer starts off 16 bytes, or a dict per operand (I, F, B, G; the others 0).  The tokens come from the plan entry, asked
    with what the entries see: the forward's 16-byte paths need I and F on 16 bytes, the backward's dO, F and I; bit 1 = DB not behind DF"""
    H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
    geo = (N, H1, W1, C1, H0, W0, C0, K, S, P, D)
    per = off if isinstance(off, dict) else {k: off for k in "IFBGO"}
    of = lambda k: per.get(k, 0)
    al = lambda *ks: 0 if any(of(k) % 4 for k in ks) else 1
    pl_f = plan(h, N, H1, W1, C1, C0, K, S, P, D, al("I", "F"))
    pl = plan(h, N, H1, W1, C1, C0, K, S, P, D, al("I", "F", "G") | (2 if split_grads else 0))
    t_fwd = tokens(pl_f)[0]
    _, t_df, t_fold, t_dx = tokens(pl)
    off = of("O")                                                        # the outputs' offset
    ndf = C1 * K * K * C0
    nan = lambda n: np.full(n, np.nan, np.float32)
    for kind in kinds:
        a = operands(kind, zlib.crc32(repr((name, kind, geo)).encode()), N, H1, W1, C1, H0, W0, C0, K)
        wo, wdx, wdf, wdb = witness(kind, a, K, S, P, D)
        dI, dF, dB, dG = Dev(a["I"], of("I")), Dev(a["F"], of("F")), Dev(a["B"], of("B")), Dev(a["G"], of("G"))
        dO = Dev(nan(N * H0 * W0 * C0), off)
        l0 = lcount(h)
        h.call("t4k_conv2d_geo_fwd", dI.p, None, dO.p, dF.p, dB.p, *geo, None)
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
            h.call("t4k_conv2d_geo_bwd", dI.p, dG.p, dDX.p, dDX2.p, dF.p, pdf, pdb, *geo, 1, None)
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
        if kind == "float":                                             # the same bits on a second run: fixed summation trees
            dO2 = Dev(nan(N * H0 * W0 * C0), off)
            h.call("t4k_conv2d_geo_fwd", dI.p, None, dO2.p, dF.p, dB.p, *geo, None)
            assert np.array_equal(dO2.get(h, wo.exact.shape), dO.get(h, wo.exact.shape))
            r = backward()
            assert np.array_equal(r[0], dx) and np.array_equal(r[2], df) and np.array_equal(r[3], db), name
        guards_intact(dO, dI, dF, dB, dG)
        assert np.array_equal(dI.get(h, a["I"].shape), a["I"]) and np.array_equal(dG.get(h, a["G"].shape), a["G"])   # the operands are intact
    return pl


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "k%ds%dp%dd%d" % g)
def test_geometries(t4k, geo):
    K, S, P, D = geo
    for i, (C1, C0) in enumerate(CHANNELS):
        H1, W1 = IMAGES[(i + GEOS.index(geo)) % 2]
        run_case(t4k, "geo", 3, H1, W1, C1, C0, K, S, P, D)
        if (C1, C0) in ((3, 5), (64, 64)):                               # both images on a ragged and on a full channel pair
            H1, W1 = IMAGES[(i + GEOS.index(geo) + 1) % 2]
            run_case(t4k, "geo", 3, H1, W1, C1, C0, K, S, P, D, kinds=("int",))


def test_wide_output_channels(t4k):
    """C0 = 130: three channel tiles on the scalar filter path, five bias columns past two dF tiles"""
    run_case(t4k, "wide", 3, 11, 9, 5, 130, 3, 2, 1, 1)
    run_case(t4k, "wide", 2, 8, 13, 130, 5, 3, 1, 2, 2, kinds=("int",))


@pytest.mark.parametrize("C1,C0", [(1, 1), (3, 31), (31, 33), (33, 65), (68, 132), (132, 68)])
def test_channel_remainders(t4k, C1, C0):
    """C0 = 1, 31, 33, 65 and C1 = 1, 3, 31, 33: the k remainder of a 32-channel step and the ragged channel tile; 68 / 132: the 128-wide
    tiles of forward and dX with a 16-byte remainder"""
    pl = run_case(t4k, "chan", 2, 8, 13, C1, C0, 3, 2, 1, 1)
    if (C1, C0) == (68, 132):
        assert pl[0] == 128 and pl[1] == 3 and pl[2] == 128 and pl[3] == 1
    run_case(t4k, "chan", 1, 9, 7, C1, C0, 5, 1, 4, 2, kinds=("int",))


@pytest.mark.parametrize("npix,H1,W1", [(1, 2, 2), (63, 14, 18), (65, 10, 26), (257, 2, 514)])
def test_pixel_counts(t4k, npix, H1, W1):
    """N H0 W0 = 1, 63, 65, 257 under 2x2 / 2: one pixel, either side of a half tile, one past two tiles"""
    assert extent(H1, 2, 2, 0, 1) * extent(W1, 2, 2, 0, 1) == npix
    run_case(t4k, "npix", 1, H1, W1, 3, 5, 2, 2, 0, 1)
    run_case(t4k, "npix", 1, H1, W1, 4, 8, 2, 2, 0, 1, kinds=("int",))


def test_stride_above_the_window(t4k):
    """(3, 4, 0, 1) and (1, 2, 0, 1): input pixels nothing reads - their dX is exactly 0, and written (the NaN fill is gone)"""
    for K, S in ((3, 4), (1, 2)):
        N, H1, W1, C1, C0 = 2, 11, 9, 3, 5
        H0, W0 = extent(H1, K, S, 0, 1), extent(W1, K, S, 0, 1)
        a = operands("float", 7, N, H1, W1, C1, H0, W0, C0, K)
        dI, dG, dF, dDX = Dev(a["I"]), Dev(a["G"]), Dev(a["F"]), Dev(np.full(a["I"].size, np.nan, np.float32))
        l0 = lcount(t4k)
        t4k.call("t4k_conv2d_geo_bwd", dI.p, dG.p, dDX.p, None, dF.p, None, None, N, H1, W1, C1, H0, W0, C0, K, S, 0, 1, 0, None)
        assert lcount(t4k) - l0 == 1
        dx = dDX.get(t4k, a["I"].shape)
        fw.check("unread dX", dx, witness("float", a, K, S, 0, 1)[1])
        read = np.zeros((H1, W1), bool)
        for i in range(H0):
            for j in range(W0):
                read[i * S:i * S + K, j * S:j * S + K] = True
        assert (~read).sum() > 0 and not np.isnan(dx).any()
        assert np.all(dx[:, ~read, :] == 0.0)


def test_single_window_and_small_images(t4k):
    run_case(t4k, "one", 1, 5, 5, 3, 5, 5, 1, 0, 1)                      # H0 = W0 = 1: the window is the image
    run_case(t4k, "one", 2, 7, 7, 4, 8, 3, 3, 0, 3)                      # ... dilated: 3 taps, 3 apart
    run_case(t4k, "small", 3, 2, 2, 3, 5, 7, 1, 3, 1)                    # an image smaller than the window
    run_case(t4k, "small", 3, 2, 3, 4, 8, 7, 2, 3, 1)
    run_case(t4k, "small", 1, 1, 1, 1, 1, 1, 1, 0, 1)


@pytest.mark.parametrize("C1,C0", [(4, 8), (64, 64), (3, 5)])
def test_pointers_off_16_bytes(t4k, C1, C0):
    """every pointer 4 bytes off 16-byte alignment: the dword paths, asserted through the plan and the tokens"""
    pl = plan(t4k, 3, 11, 9, C1, C0, 3, 2, 1, 1, 0)
    assert pl[1] == 0 and pl[3] == 0 and pl[4] == 0
    assert plan(t4k, 3, 11, 9, C1, C0, 3, 2, 1, 1, 1)[1] == (3 if C1 % 4 == 0 else 0)
    run_case(t4k, "off", 3, 11, 9, C1, C0, 3, 2, 1, 1, off=1)
    run_case(t4k, "off", 3, 8, 13, C1, C0, 3, 1, 2, 2, off=3, kinds=("int",))


@pytest.mark.parametrize("which", ["I", "G", "F"])
def test_one_pointer_off_16_bytes(t4k, which):
    """only I, only dO or only F 4 bytes off, 64 -> 64 channels (whole 16-byte paths otherwise): no 16-byte load may start there.  I off: the
    forward gathers dwords and the backward - whose dF tile would gather I 16 bytes at a time - takes its dword engines; dO off: the forward keeps
    its 16-byte paths, the backward does not; the engines asserted through t4k_conv_last_plan (run_case), here against what they must be"""
    pl = run_case(t4k, "one_off", 3, 11, 9, 64, 64, 3, 2, 1, 1, off={which: 1})
    assert pl[3] == 0 and pl[4] == 0, pl                                 # dX and dF on dwords, rows side by side
    al = plan(t4k, 3, 11, 9, 64, 64, 3, 2, 1, 1, 1)
    assert al[3] == 1 and al[4] == 3, al                                 # ... where all three on 16 bytes take the tap-per-tile dF
    N, H1, W1, C = 3, 11, 9, 64
    H0, W0 = extent(H1, 3, 2, 1, 1), extent(W1, 3, 2, 1, 1)
    a = operands("int", 3, N, H1, W1, C, H0, W0, C, 3)
    o = lambda k: 1 if k == which else 0
    dI, dF, dB, dG = Dev(a["I"], o("I")), Dev(a["F"], o("F")), Dev(a["B"], o("B")), Dev(a["G"], o("G"))
    dO, dDX, dDF, dDB = Dev(np.zeros(a["G"].size, np.float32)), Dev(np.zeros(a["I"].size, np.float32)), Dev(a["DF0"]), Dev(a["DB0"])
    t4k.call("t4k_conv2d_geo_fwd", dI.p, None, dO.p, dF.p, dB.p, N, H1, W1, C, H0, W0, C, 3, 2, 1, 1, None)
    assert last_plan(t4k) == ("geo<64,v4,f4>" if which == "G" else "geo<64,v1,f1>")
    t4k.call("t4k_conv2d_geo_bwd", dI.p, dG.p, dDX.p, None, dF.p, dDF.p, dDB.p, N, H1, W1, C, H0, W0, C, 3, 2, 1, 1, 1, None)
    assert last_plan(t4k) == "geo_dfx%d<rows,d1> df_fold geo_dx<64,v1>" % pl[5], last_plan(t4k)


def test_both_folds(t4k):
    """k_fold_add up to 32 slices (DB right behind DF), k_conv_df_fold above and for a DB elsewhere; the batch with more than 32 slices is
    found through the plan"""
    N = next(n for n in range(1, 64) if plan(t4k, n, 11, 9, 3, 5, 3, 1, 1, 1)[5] > 32)
    assert N * 11 * 9 < 4000
    pl = run_case(t4k, "fold", N, 11, 9, 3, 5, 3, 1, 1, 1)
    assert pl[5] > 32 and pl[6] == 2
    pl = run_case(t4k, "fold", N - 1, 11, 9, 3, 5, 3, 1, 1, 1, kinds=("float",))
    assert pl[5] <= 32 and pl[6] == 1
    run_case(t4k, "fold", 3, 11, 9, 4, 8, 3, 2, 1, 1, split_grads=True)   # few slices, DB not behind DF: df_fold (asserted in run_case)
    run_case(t4k, "fold", N, 11, 9, 33, 31, 3, 1, 1, 1, split_grads=True, kinds=("float",))


def test_backward_forms(t4k):
    """DX == NULL, DF == DB == NULL, train = 0, DX2 == DX, DX2 == I in place, ICOPY"""
    h = t4k
    N, H1, W1, C1, C0, K, S, P, D = 3, 11, 9, 4, 8, 3, 2, 1, 1
    H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
    geo = (N, H1, W1, C1, H0, W0, C0, K, S, P, D)
    a = operands("float", 11, N, H1, W1, C1, H0, W0, C0, K)
    wo, wdx, wdf, wdb = witness("float", a, K, S, P, D)
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dF, dB, dG = Dev(a["I"]), Dev(a["F"]), Dev(a["B"]), Dev(a["G"])
    # ICOPY: a copy command beside the one launch
    dO, dC = Dev(nan(wo.exact.size)), Dev(nan(a["I"].size))
    l0 = lcount(h)
    h.call("t4k_conv2d_geo_fwd", dI.p, dC.p, dO.p, dF.p, dB.p, *geo, None)
    assert lcount(h) - l0 == 1 and last_plan(h).startswith("memcpy geo<")
    assert np.array_equal(dC.get(h, a["I"].shape), a["I"]); fw.check("icopy O", dO.get(h, wo.exact.shape), wo)
    # DX == NULL: slabs and fold
    dDF, dDB, dDX = Dev(a["DF0"]), Dev(a["DB0"]), Dev(nan(a["I"].size))
    l0 = lcount(h)
    h.call("t4k_conv2d_geo_bwd", dI.p, dG.p, None, dDX.p, dF.p, dDF.p, dDB.p, *geo, 1, None)
    assert lcount(h) - l0 == 2 and np.isnan(dDX.get(h, a["I"].shape)).all()
    fw.check("dF alone", dDF.get(h, a["F"].shape), wdf); fw.check("dB alone", dDB.get(h, (C0,)), wdb)
    # DF == DB == NULL and train = 0: dX alone, one launch; the gradients bit-unchanged
    for pdf, pdb, train in ((None, None, 1), (None, None, 0)):
        l0 = lcount(h)
        h.call("t4k_conv2d_geo_bwd", dI.p, dG.p, dDX.p, None, dF.p, pdf, pdb, *geo, train, None)
        assert lcount(h) - l0 == 1
        fw.check("dX alone", dDX.get(h, a["I"].shape), wdx)
    dDF, dDB = Dev(a["DF0"]), Dev(a["DB0"])
    l0 = lcount(h)
    h.call("t4k_conv2d_geo_bwd", dI.p, dG.p, dDX.p, None, dF.p, dDF.p, dDB.p, *geo, 0, None)
    assert lcount(h) - l0 == 1
    assert np.array_equal(dDF.get(h, a["F"].shape), a["DF0"]) and np.array_equal(dDB.get(h, (C0,)), a["DB0"])
    assert h.lib.t4k_conv2d_geo_bwd(dI.p, dG.p, dDX.p, None, dF.p, dDF.p, None, *geo, 1, None) == ERR_ARG      # DF and DB go together
    # DX2 == DX
    dDX = Dev(nan(a["I"].size))
    h.call("t4k_conv2d_geo_bwd", dI.p, dG.p, dDX.p, dDX.p, dF.p, None, None, *geo, 0, None)
    fw.check("DX2 == DX", dDX.get(h, a["I"].shape), wdx)
    # DX2 == I, in place: dF | dB read I first
    dI2, dDX, dDF, dDB = Dev(a["I"]), Dev(nan(a["I"].size)), Dev(a["DF0"]), Dev(a["DB0"])
    h.call("t4k_conv2d_geo_bwd", dI2.p, dG.p, dDX.p, dI2.p, dF.p, dDF.p, dDB.p, *geo, 1, None)
    fw.check("in place dX", dI2.get(h, a["I"].shape), wdx); fw.check("in place dX'", dDX.get(h, a["I"].shape), wdx)
    fw.check("in place dF", dDF.get(h, a["F"].shape), wdf); fw.check("in place dB", dDB.get(h, (C0,)), wdb)
    guards_intact(dI2, dDX, dDF, dDB, dO, dC)


def test_rejections(t4k):
    """a bad argument: T4K_ERR_ARG; an inadmissible geometry: T4K_ERR_UNSUPPORTED; a text either way, nothing launched, the outputs untouched"""
    h = t4k
    N, H1, W1, C1, C0 = 2, 8, 8, 3, 5
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dF, dB = Dev(np.ones(N * H1 * W1 * C1, np.float32)), Dev(np.ones(C1 * 49 * C0, np.float32)), Dev(np.ones(C0, np.float32))
    dO, dG, dDX, dDF, dDB = Dev(nan(N * 64 * C0)), Dev(np.ones(N * 64 * C0, np.float32)), Dev(nan(N * H1 * W1 * C1)), Dev(nan(C1 * 49 * C0)), Dev(nan(C0))
    bad = [((3, 2, 1, 1, 4, 5), ERR_ARG, b"gives 4x4"), ((3, 2, 1, 1, 5, 4), ERR_ARG, b"gives 4x4"), ((3, 2, 1, 1, 3, 4), ERR_ARG, b"gives 4x4"), ((3, 2, 1, 1, 4, 3), ERR_ARG, b"gives 4x4"), ((8, 1, 3, 1, 7, 7), ERR_UNSUPPORTED, b"not supported"),
           ((3, 5, 1, 1, 2, 2), ERR_UNSUPPORTED, b"not supported"), ((3, 1, 1, 5, 1, 1), ERR_UNSUPPORTED, b"not supported"),
           ((3, 1, 3, 1, 12, 12), ERR_UNSUPPORTED, b"not supported"), ((3, 1, 5, 2, 14, 14), ERR_UNSUPPORTED, b"not supported"),
           ((7, 1, 0, 2, 1, 1), ERR_UNSUPPORTED, b"does not fit")]
    for (K, S, P, D, H0, W0), code, text in bad:
        l0 = lcount(h)
        assert h.lib.t4k_conv2d_geo_fwd(dI.p, None, dO.p, dF.p, dB.p, N, H1, W1, C1, H0, W0, C0, K, S, P, D, None) == code, (K, S, P, D)
        assert text in h.lib.t4k_last_error(), h.lib.t4k_last_error()
        assert h.lib.t4k_conv2d_geo_bwd(dI.p, dG.p, dDX.p, None, dF.p, dDF.p, dDB.p, N, H1, W1, C1, H0, W0, C0, K, S, P, D, 1, None) == code
        assert text in h.lib.t4k_last_error() and lcount(h) == l0
    good = (N, H1, W1, C1, 4, 4, C0, 3, 2, 1, 1)
    assert h.lib.t4k_conv2d_geo_fwd(None, None, dO.p, dF.p, dB.p, *good, None) == ERR_ARG
    assert h.lib.t4k_conv2d_geo_fwd(dI.p, None, dO.p, dF.p, None, *good, None) == ERR_ARG
    assert h.lib.t4k_conv2d_geo_bwd(dI.p, None, dDX.p, None, dF.p, dDF.p, dDB.p, *good, 1, None) == ERR_ARG
    assert h.lib.t4k_conv2d_geo_fwd(dI.p, None, dO.p, dF.p, dB.p, 0, H1, W1, C1, 4, 4, C0, 3, 2, 1, 1, None) == ERR_ARG
    for d in (dO, dDX, dDF, dDB):
        assert np.isnan(d.get(h, (d.n,))).all()


@pytest.mark.parametrize("K,S,P", [(1, 1, 0), (3, 1, 1), (4, 2, 1), (5, 1, 2)])
@pytest.mark.parametrize("C1,C0", [(3, 5), (64, 64)])
def test_beside_the_specialised_kernels(t4k, K, S, P, C1, C0):
    """the four geometries both families admit, integer operands: forward and dF | dB bit-equal to t4k_conv2d_fwd / t4k_conv2d_bwd; dX bit-equal
    to t4k_conv2d_bwd's dX computed with the filter rotated by 180 degrees - the reference's quirk a-11, stated as a test"""
    h = t4k
    N, H1, W1 = 3, 11, 9
    H0, W0 = extent(H1, K, S, P, 1), extent(W1, K, S, P, 1)
    old, new = (N, H1, W1, C1, H0, W0, C0, K, S, P), (N, H1, W1, C1, H0, W0, C0, K, S, P, 1)
    a = operands("int", zlib.crc32(repr(old).encode()), N, H1, W1, C1, H0, W0, C0, K)
    nan = lambda n: np.full(n, np.nan, np.float32)
    dI, dF, dB, dG = Dev(a["I"]), Dev(a["F"]), Dev(a["B"]), Dev(a["G"])
    dFr = Dev(np.ascontiguousarray(a["F"][:, ::-1, ::-1, :]))
    oo, on = Dev(nan(a["G"].size)), Dev(nan(a["G"].size))
    h.call("t4k_conv2d_fwd", dI.p, oo.p, dF.p, dB.p, *old, None)
    h.call("t4k_conv2d_geo_fwd", dI.p, None, on.p, dF.p, dB.p, *new, None)
    assert last_plan(h).startswith("geo<")
    assert np.array_equal(oo.get(h, a["G"].shape), on.get(h, a["G"].shape))
    xo, xn = Dev(nan(a["I"].size)), Dev(nan(a["I"].size))
    fo, bo, fn, bn = Dev(a["DF0"]), Dev(a["DB0"]), Dev(a["DF0"]), Dev(a["DB0"])
    h.call("t4k_conv2d_bwd", dI.p, dG.p, None, dF.p, fo.p, bo.p, *old, 1, None)                # dF | dB from the filter as it is ...
    h.call("t4k_conv2d_bwd", dI.p, dG.p, xo.p, dFr.p, None, None, *old, 0, None)               # ... dX from the rotated one
    h.call("t4k_conv2d_geo_bwd", dI.p, dG.p, xn.p, None, dF.p, fn.p, bn.p, *new, 1, None)
    assert "geo_dfx" in last_plan(h) and "geo_dx<" in last_plan(h)
    assert np.array_equal(fo.get(h, a["F"].shape), fn.get(h, a["F"].shape)) and np.array_equal(bo.get(h, (C0,)), bn.get(h, (C0,)))
    assert np.array_equal(xo.get(h, a["I"].shape), xn.get(h, a["I"].shape))
    _, wdx, _, _ = witness("int", a, K, S, P, 1)
    fw.equal("textbook dX", xn.get(h, a["I"].shape), wdx.exact)
