"""t4k_groupnorm_fwd / _bwd (include/t4k.h, csrc/groupnorm.hip) through the C ABI: group, layer and instance norm on NHWC.

Every stored tensor is held against its staged float64 witness (tests/gn_witness.py), each computed from the operands the kernel itself stored: STAT's
mean | rstd from I, XH from I and the stored statistics, O from the stored XH, STAT's s1 | s2 from DY and the stored XH, DX from the stored rstd | s1 | s2, DW and
DB on top of their prior values.  No element is excepted.  Outputs are pre-filled with NaN between guard floats (Dev of tests/test_gpu_bcast.py): an element that
was not written shows, and so does a store outside the tensor.  The rung and the launch counts come from t4k_groupnorm_plan, the function the entries call."""
import ctypes
import zlib

import numpy as np
import pytest

import gn_witness as gw
from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
EPS = gw.EPS
FWD_PTRS, BWD_PTRS = ("I", "O", "XH", "W", "B"), ("W", "DY", "XH", "DX")       # what the 16-byte path asks of a call


def plan(h, N, HW, C, G, aligned=1):
    out = I8()
    assert h.lib.t4k_groupnorm_plan(N, HW, C, G, aligned, 32 << 20, out) == OK, h.lib.t4k_last_error()
    return list(out)


def nan(k):
    return np.full(k, np.nan, np.float32)


def data(seed, N, HW, C, kind="normal"):
    rng = np.random.default_rng(seed)
    sh = (N, HW, 1, C)
    if kind == "offset":
        X = (1024.0 + rng.normal(0.0, 1.0, sh)).astype(np.float32)
    elif kind == "const":
        X = np.full(sh, 3.0, np.float32)
    else:
        X = rng.normal(0.5, 2.0, sh).astype(np.float32)
    DY = rng.normal(0.0, 1.0, sh).astype(np.float32)
    Wg = rng.uniform(0.5, 1.5, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
    B = rng.normal(0.0, 0.5, C).astype(np.float32)
    return X, DY, Wg, B, rng.normal(0.0, 1.0, C).astype(np.float32), rng.normal(0.0, 1.0, C).astype(np.float32)


def run_case(h, name, N, HW, C, G, kind="normal", off=None, train=1, inplace=False, rung=None):
    """forward, then backward, every stored tensor against its witness; launches against the plan; guards.  off: floats a pointer starts off 16 bytes, by name.
    Returns (plan, O, XH, STAT, DX, DW, DB)"""
    off = off or {}
    o = lambda k: off.get(k, 0)
    X, DY, Wg, B, DW0, DB0 = data(zlib.crc32(repr((name, N, HW, C, G, kind)).encode()), N, HW, C, kind)
    NG = N * G
    pf = plan(h, N, HW, C, G, int(all(o(k) % 4 == 0 for k in FWD_PTRS)))
    pb = plan(h, N, HW, C, G, int(all(o(k) % 4 == 0 for k in BWD_PTRS)))
    if rung is not None:
        assert pf[0] == rung and pb[0] == rung, (name, pf, pb)
    assert pf[1] == (4 if (C // G) % 4 == 0 and all(o(k) % 4 == 0 for k in FWD_PTRS) else 1), (name, pf)
    dI, dW, dB = Dev(X, o("I")), Dev(Wg, o("W")), Dev(B, o("B"))
    dO = dI if inplace else Dev(nan(X.size), o("O"))
    dXH, dST = Dev(nan(X.size), o("XH")), Dev(nan(4 * NG), o("STAT"))
    l0 = lcount(h)
    h.call("t4k_groupnorm_fwd", dI.p, dO.p, dXH.p, dW.p, dB.p, dST.p, N, HW, C, G, EPS, None)
    assert lcount(h) - l0 == pf[4], (name, pf)
    tag = "%s n%d hw%d c%d g%d %s" % (name, N, HW, C, G, kind)
    ST = dST.get(h, (4 * NG,)).copy(); XH = dXH.get(h, X.shape).copy(); O = dO.get(h, X.shape).copy()
    assert np.isnan(ST[2 * NG:]).all(), tag                                  # the forward writes the first two quarters only
    wm, wr = gw.gn_stats(X, G)
    gw.check(tag + " mean", ST[:NG], wm); gw.check(tag + " rstd", ST[NG:2 * NG], wr)
    gw.check(tag + " xhat", XH, gw.gn_xhat(X, ST, G))
    gw.check(tag + " y", O, gw.gn_y(XH, Wg, B))
    if not inplace:
        assert np.array_equal(dI.get(h, X.shape), X), tag
    # backward
    dDY = Dev(DY, o("DY"))
    dDX = dDY if inplace else Dev(nan(X.size), o("DX"))
    dDW, dDB = Dev(DW0, o("DW")), Dev(DB0, o("DB"))
    l0 = lcount(h)
    h.call("t4k_groupnorm_bwd", dW.p, dDY.p, dXH.p, dST.p, dDX.p, dDW.p if train != "null" else None, dDB.p if train != "null" else None, N, HW, C, G,
           1 if train == 1 else 0, None)
    assert lcount(h) - l0 == (pb[7] if train == 1 else pb[7] - 1), (name, pb)
    ST2 = dST.get(h, (4 * NG,)).copy(); DX = dDX.get(h, X.shape).copy(); DW = dDW.get(h, (C,)).copy(); DB = dDB.get(h, (C,)).copy()
    assert np.array_equal(ST2[:2 * NG], ST[:2 * NG]), tag
    ws1, ws2, wdw, wdb = gw.gn_bwd_stats(Wg, DY, XH, G, DW0, DB0, train == 1)
    gw.check(tag + " s1", ST2[2 * NG:3 * NG], ws1); gw.check(tag + " s2", ST2[3 * NG:], ws2)
    gw.check(tag + " dx", DX, gw.gn_dx(Wg, DY, XH, ST2, G))
    gw.check(tag + " dw", DW, wdw); gw.check(tag + " db", DB, wdb)
    assert np.array_equal(dXH.get(h, X.shape), XH) and np.array_equal(dW.get(h, (C,)), Wg), tag
    guards_intact(dI, dO, dXH, dST, dW, dB, dDY, dDX, dDW, dDB)
    return pf, O, XH, ST2, DX, DW, DB


PAIRS = [(1, 1), (3, 1), (3, 3), (8, 1), (8, 2), (8, 8), (12, 4), (64, 32), (7, 7)]


@pytest.mark.parametrize("C,G", PAIRS, ids=["c%dg%d" % p for p in PAIRS])
def test_grid(t4k, C, G):
    for HW in (1, 63, 65, 257):
        for N in (1, 3):
            run_case(t4k, "grid", N, HW, C, G)


def test_one_element_groups(t4k):
    """E = 1 (HW = 1, G = C): xhat = 0, y = beta, dx = 0, exactly"""
    for C in (1, 7, 8):
        N = 3
        _, O, XH, ST, DX, _, _ = run_case(t4k, "e1", N, 1, C, C)
        B = data(zlib.crc32(repr(("e1", N, 1, C, C, "normal")).encode()), N, 1, C)[3]
        assert not XH.any() and not DX.any() and np.array_equal(O, np.broadcast_to(B, O.shape))
        assert np.array_equal(ST[N * C:2 * N * C], np.full(N * C, np.float32(1.0) / np.sqrt(np.float32(EPS), dtype=np.float32)))


# (rung, (N, HW, C, G), floats every pointer is off): the boundary shapes of tests/test_groupnorm_plan.py's hand-worked rows, small enough to run
RUNGS = [
    (1, (3, 512, 1, 1), 0), (2, (3, 513, 1, 1), 0), (1, (3, 512, 8, 2), 0), (2, (3, 513, 8, 2), 0), (1, (3, 128, 8, 2), 1), (2, (3, 129, 8, 2), 1),
    (1, (3, 8, 64, 1), 1), (2, (3, 9, 64, 1), 1), (2, (2, 8192, 1, 1), 0), (2, (2, 600, 3, 1), 0), (2, (2, 40, 384, 1), 0), (2, (2, 4096, 16, 4), 0),
    (3, (64, 8193, 4, 4), 0), (3, (1, 1, 8192, 1), 0), (3, (2, 1, 8192, 1), 1), (3, (2, 4200, 256, 128), 0),
    (4, (1, 4097, 4, 1), 0), (4, (1, 8193, 1, 1), 0), (4, (2, 41, 384, 1), 0), (4, (3, 3, 1100, 1), 1), (4, (2, 3136, 64, 1), 0),
]


@pytest.mark.parametrize("rung,shape,off", RUNGS, ids=["r%d_%s_o%d" % (r, "x".join(map(str, s)), o) for r, s, o in RUNGS])
def test_every_rung(t4k, rung, shape, off):
    offs = {k: off for k in ("I", "O", "XH", "W", "B", "DY", "DX")}
    run_case(t4k, "rung", *shape, off=offs, rung=rung)


OFFSET = [(1, (2, 63, 1, 1)), (1, (2, 63, 8, 2)), (2, (2, 600, 3, 1)), (2, (2, 1024, 4, 1)), (3, (2, 1, 8192, 1)), (3, (64, 8193, 4, 4)), (4, (1, 4097, 4, 1)), (4, (2, 41, 384, 1))]


@pytest.mark.parametrize("rung,shape", OFFSET, ids=["r%d_%s" % (r, "x".join(map(str, s))) for r, s in OFFSET])
def test_offset_data_on_each_rung(t4k, rung, shape):
    """x = 1024 + N(0, 1): the bound carries no cancellation term, so E[x^2] - mean^2 would leave it (tests/test_groupnorm_plan.py)"""
    run_case(t4k, "offset", *shape, kind="offset", rung=rung)


@pytest.mark.parametrize("rung,shape", [(1, (2, 64, 4, 2)), (2, (2, 1024, 4, 1)), (3, (2, 1, 8192, 1)), (4, (1, 4096, 8, 1))])
def test_constant_group(t4k, rung, shape):
    """a constant group whose sums are exact: var = 0 and rstd = 1 / sqrt(eps) within its three roundings"""
    N, HW, C, G = shape
    _, O, XH, ST, _, _, _ = run_case(t4k, "const", N, HW, C, G, kind="const", rung=rung)
    r = 1.0 / np.sqrt(EPS)
    assert np.all(ST[:N * G] == 3.0) and np.all(np.abs(ST[N * G:2 * N * G].astype(np.float64) - r) <= 3 * gw.U * r) and not XH.any()


SINGLE = [{}] + [{k: 1} for k in ("I", "O", "XH", "W", "B", "DY", "DX")] + [{k: 1 for k in ("I", "O", "XH", "W", "B", "DY", "DX", "STAT", "DW", "DB")}]


@pytest.mark.parametrize("off", SINGLE, ids=["+".join(sorted(o)) or "aligned" for o in SINGLE])
def test_pointers_off_16_bytes(t4k, off):
    """every pointer, and each single pointer, 4 bytes off: the dword path at Cg % 4 == 0, asserted through the plan (run_case)"""
    for shape in ((2, 65, 8, 2), (2, 257, 12, 1), (2, 700, 8, 1), (1, 4097, 4, 1)):
        run_case(t4k, "off", *shape, off=off)


def test_in_place(t4k):
    """O == I and DX == DY give the bits of separate buffers"""
    for shape in ((3, 65, 8, 2), (2, 600, 3, 1), (2, 1, 8192, 1), (1, 4097, 4, 1), (2, 4200, 256, 128)):
        a = run_case(t4k, "inpl", *shape)
        b = run_case(t4k, "inpl", *shape, inplace=True)
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y), shape


def test_train_0(t4k):
    """train == 0: DW and DB untouched (run_case holds them to their prior values exactly), and allowed NULL"""
    for shape in ((3, 65, 8, 2), (2, 600, 3, 1), (2, 1, 8192, 1), (1, 4097, 4, 1)):
        a = run_case(t4k, "tr", *shape, train=1)
        b = run_case(t4k, "tr", *shape, train=0)
        c = run_case(t4k, "tr", *shape, train="null")
        assert np.array_equal(a[4], b[4]) and np.array_equal(a[4], c[4]) and np.array_equal(a[3], b[3])


def test_the_same_bits_twice(t4k):
    for shape in ((3, 65, 8, 2), (3, 257, 7, 7), (2, 600, 3, 1), (2, 1, 8192, 1), (1, 4097, 4, 1), (2, 4200, 256, 128)):
        a = run_case(t4k, "twice", *shape)
        b = run_case(t4k, "twice", *shape)
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x, y), shape


@pytest.mark.parametrize("shape", [(63, 8, 2), (600, 1, 1), (1, 8192, 1), (257, 12, 4)], ids=lambda s: "x".join(map(str, s)))
def test_sample_independence(t4k, shape):
    """rows of an N = 4 call are bit-equal to two N = 2 calls, O and DX: a sharded batch trains like the whole one (the rung is the same: asserted)"""
    h = t4k
    HW, C, G = shape
    assert plan(h, 4, HW, C, G)[0] == plan(h, 2, HW, C, G)[0]
    X, DY, Wg, B, _, _ = data(5, 4, HW, C)
    outs = []
    for lo, hi in ((0, 4), (0, 2), (2, 4)):
        N = hi - lo
        dI, dDY, dW, dB = Dev(X[lo:hi]), Dev(DY[lo:hi]), Dev(Wg), Dev(B)
        dO, dXH, dDX, dST = Dev(nan(N * HW * C)), Dev(nan(N * HW * C)), Dev(nan(N * HW * C)), Dev(nan(4 * N * G))
        h.call("t4k_groupnorm_fwd", dI.p, dO.p, dXH.p, dW.p, dB.p, dST.p, N, HW, C, G, EPS, None)
        h.call("t4k_groupnorm_bwd", dW.p, dDY.p, dXH.p, dST.p, dDX.p, None, None, N, HW, C, G, 0, None)
        outs.append((dO.get(h, (N, HW, C)).copy(), dDX.get(h, (N, HW, C)).copy()))
    assert np.array_equal(outs[0][0], np.concatenate([outs[1][0], outs[2][0]])) and np.array_equal(outs[0][1], np.concatenate([outs[1][1], outs[2][1]]))


def test_rejections(t4k):
    """every rejection: its code, a text, nothing launched, nothing written"""
    h = t4k
    N, HW, C, G = 2, 5, 8, 2
    X, DY, Wg, B, DW0, DB0 = data(9, N, HW, C)
    dI, dDY, dW, dB = Dev(X), Dev(DY), Dev(Wg), Dev(B)
    dO, dXH, dDX, dST, dDW, dDB = Dev(nan(X.size)), Dev(nan(X.size)), Dev(nan(X.size)), Dev(nan(4 * N * G)), Dev(nan(C)), Dev(nan(C))
    fwd = lambda a=None, shape=(N, HW, C, G), eps=EPS: h.lib.t4k_groupnorm_fwd(*(a or (dI.p, dO.p, dXH.p, dW.p, dB.p, dST.p)), *shape, eps, None)
    bwd = lambda a=None, shape=(N, HW, C, G), train=1: h.lib.t4k_groupnorm_bwd(*(a or (dW.p, dDY.p, dXH.p, dST.p, dDX.p, dDW.p, dDB.p)), *shape, train, None)
    l0 = lcount(h)
    for k in range(6):
        a = [dI.p, dO.p, dXH.p, dW.p, dB.p, dST.p]; a[k] = None
        assert fwd(a) == ERR_ARG and b"null" in h.lib.t4k_last_error(), k
    for k in range(5):
        a = [dW.p, dDY.p, dXH.p, dST.p, dDX.p, dDW.p, dDB.p]; a[k] = None
        assert bwd(a) == ERR_ARG and b"null" in h.lib.t4k_last_error(), k
    for k in (5, 6):
        a = [dW.p, dDY.p, dXH.p, dST.p, dDX.p, dDW.p, dDB.p]; a[k] = None
        assert bwd(a) == ERR_ARG and b"required" in h.lib.t4k_last_error(), k
    for eps in (0.0, -1e-5, float("nan")):
        assert fwd(eps=eps) == ERR_ARG and b"eps" in h.lib.t4k_last_error()
    for k in range(3):
        for v in (0, -1):
            s = [N, HW, C, G]; s[k] = v
            assert fwd(shape=s) == ERR_ARG and b"extent" in h.lib.t4k_last_error(), s
            assert bwd(shape=s) == ERR_ARG and b"extent" in h.lib.t4k_last_error(), s
    for g in (0, -1, 3, 16):
        assert fwd(shape=(N, HW, C, g)) == ERR_UNSUPPORTED and b"groups" in h.lib.t4k_last_error(), g
        assert bwd(shape=(N, HW, C, g)) == ERR_UNSUPPORTED and b"groups" in h.lib.t4k_last_error(), g
    # 2^31 elements, and a slab beyond the workspace: refused before a pointer is followed
    assert fwd(shape=(1 << 16, 1 << 15, 1, 1)) == ERR_UNSUPPORTED and b"2^31" in h.lib.t4k_last_error()
    assert bwd(shape=(1 << 16, 1 << 15, 1, 1)) == ERR_UNSUPPORTED and b"2^31" in h.lib.t4k_last_error()
    assert fwd(shape=((1 << 31) - 1, 1, 1, 1)) == ERR_UNSUPPORTED and b"workspace" in h.lib.t4k_last_error()
    assert bwd(shape=((1 << 31) - 1, 1, 1, 1)) == ERR_UNSUPPORTED and b"workspace" in h.lib.t4k_last_error()
    assert lcount(h) == l0
    for d in (dO, dXH, dDX, dST, dDW, dDB):
        assert np.isnan(d.get(h, (d.n,))).all()
    guards_intact(dO, dXH, dDX, dST, dDW, dDB)
    assert fwd() == OK and bwd() == OK
