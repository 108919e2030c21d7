"""t4k_addnorm_fwd / _bwd (include/t4k.h, csrc/addnorm.hip) through the C ABI: out = norm(x + skip) on [rows, C] tokens, mode 0 none, 1 layer
norm, 2 RMS norm, and its backward on t = dy + dy2.

Every stored tensor is held against its staged float64 witness (tests/an_witness.py), each computed from the operands the kernel itself stored: RSTD from X and
S, XH from X, S and the stored RSTD, O from the stored XH, DX from the stored XH and RSTD, DW and DB on top of their prior values.  No element is excepted.
Outputs are pre-filled with NaN between guard floats (Dev of tests/test_gpu_bcast.py): an element that was not written shows, and so does a store outside the
tensor.  The rung, the lanes per token, the tokens per workgroup and the launch counts come from t4k_addnorm_plan, the function the entries call; the grid's
row counts are built from them."""
import ctypes
import zlib

import numpy as np
import pytest

import an_witness as an
from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
EPS = an.EPS
WS = 32 << 20
FWD_PTRS, BWD_PTRS = ("X", "S", "O", "XH", "W", "B"), ("W", "DY", "DY2", "XH", "DX")       # what the 16-byte path asks of a call


def plan(h, rows, C, mode, aligned=1):
    out = I8()
    assert h.lib.t4k_addnorm_plan(rows, C, mode, aligned, WS, out) == OK, h.lib.t4k_last_error()
    return list(out)


def nan(k):
    return np.full(k, np.nan, np.float32)


def data(seed, rows, C, kind="normal"):
    rng = np.random.default_rng(seed)
    sh = (rows, C)
    X = rng.normal(0.5, 2.0, sh).astype(np.float32); S = rng.normal(-0.25, 1.0, sh).astype(np.float32)
    if kind == "offset":
        X = (1024.0 + rng.normal(0.0, 1.0, sh)).astype(np.float32)
    DY = rng.normal(0.0, 1.0, sh).astype(np.float32); DY2 = rng.normal(0.0, 1.0, sh).astype(np.float32)
    if kind == "cancel":
        S = -X
    if kind == "zero_dy":
        DY[:] = 0.0; DY2[:] = 0.0
    Wg = rng.uniform(0.5, 1.5, C).astype(np.float32) * rng.choice([-1.0, 1.0], C).astype(np.float32)
    B = rng.normal(0.0, 0.5, C).astype(np.float32)
    return X, S, Wg, B, DY, DY2, rng.normal(0.0, 1.0, C).astype(np.float32), rng.normal(0.0, 1.0, C).astype(np.float32)


def run_case(h, name, rows, C, mode, skip=1, dy2=1, off=None, train=1, inplace=(), kind="normal", rung=None, T=None):
    """forward, then backward, every stored tensor against its witness; launches against the plan; operands intact; guards.  off: floats a pointer starts off
    16 bytes, by name.  inplace: any of "O=X", "O=S", "DX=DY", "DX=DY2".  Returns (plan, O, XH, RSTD, DX, DW, DB)"""
    off = off or {}
    o = lambda k: off.get(k, 0)
    X, S, Wg, B, DY, DY2, DW0, DB0 = data(zlib.crc32(repr((name, rows, C, kind)).encode()), rows, C, kind)
    S = S if skip else None; DY2 = DY2 if dy2 else None
    used_f = [k for k in FWD_PTRS if not (k == "S" and not skip) and not (mode == 0 and k in ("XH", "W", "B"))]
    used_b = [k for k in BWD_PTRS if not (k == "DY2" and not dy2) and not (mode == 0 and k in ("XH", "W"))]
    al_f, al_b = all(o(k) % 4 == 0 for k in used_f), all(o(k) % 4 == 0 for k in used_b)
    pf, pb = plan(h, rows, C, mode, int(al_f)), plan(h, rows, C, mode, int(al_b))
    if rung is not None:
        assert pf[0] == rung and pb[0] == rung, (name, pf, pb)
    if T is not None:
        assert pf[3] == T, (name, pf)
    assert pf[1] == (4 if C % 4 == 0 and al_f else 1) and pb[1] == (4 if C % 4 == 0 and al_b else 1), (name, pf, pb)
    n = rows * C
    dX, dS, dW, dB = Dev(X, o("X")), (Dev(S, o("S")) if skip else None), Dev(Wg, o("W")), Dev(B, o("B"))
    dO = dX if "O=X" in inplace else dS if "O=S" in inplace else Dev(nan(n), o("O"))
    dXH, dR = Dev(nan(n), o("XH")), Dev(nan(rows), o("RSTD"))
    P = lambda d: d.p if d is not None else None
    norm = mode != 0
    l0 = lcount(h)
    h.call("t4k_addnorm_fwd", dX.p, P(dS), dO.p, dXH.p if norm else None, dR.p if norm else None, dW.p if norm else None, dB.p if norm else None,
           rows, C, mode, EPS, None)
    assert lcount(h) - l0 == pf[4] == 1, (name, pf)
    tag = "%s r%d c%d m%d s%d d%d %s %s" % (name, rows, C, mode, skip, dy2, kind, sorted(off))
    O = dO.get(h, (rows, C)).copy(); XH = dXH.get(h, (rows, C)).copy(); R = dR.get(h, (rows,)).copy()
    if norm:
        an.check(tag + " rstd", R, an.an_rstd(X, S, C, mode))
        an.check(tag + " xhat", XH, an.an_xhat(X, S, R, C, mode))
        an.check(tag + " y", O, an.an_y(XH, Wg, B, C))
    else:
        assert np.isnan(XH).all() and np.isnan(R).all(), tag                # mode 0 stores neither
        want = X if S is None else X + S                                    # NumPy float32: one rounding, the kernel's
        assert np.array_equal(O.view(np.uint32), want.view(np.uint32)), tag
    if "O=X" not in inplace:
        assert np.array_equal(dX.get(h, (rows, C)), X), tag
    if skip and "O=S" not in inplace:
        assert np.array_equal(dS.get(h, (rows, C)), S), tag
    assert np.array_equal(dW.get(h, (C,)), Wg) and np.array_equal(dB.get(h, (C,)), B), tag
    # backward
    dDY, dD2 = Dev(DY, o("DY")), (Dev(DY2, o("DY2")) if dy2 else None)
    dDX = dDY if "DX=DY" in inplace else dD2 if "DX=DY2" in inplace else Dev(nan(n), o("DX"))
    dDW, dDB = Dev(DW0, o("DW")), Dev(DB0, o("DB"))
    null = train == "null"
    l0 = lcount(h)
    h.call("t4k_addnorm_bwd", dW.p if norm else None, dDY.p, P(dD2), dXH.p if norm else None, dR.p if norm else None, dDX.p,
           None if null else dDW.p, None if null else dDB.p, rows, C, mode, 1 if train == 1 else 0, None)
    assert lcount(h) - l0 == (pb[7] if train == 1 else 1), (name, pb)
    DX = dDX.get(h, (rows, C)).copy(); DW = dDW.get(h, (C,)).copy(); DB = dDB.get(h, (C,)).copy()
    an.check(tag + " dx", DX, an.an_dx(Wg, DY, DY2, XH, R, C, mode))
    wdw, wdb = an.an_dwdb(DY, DY2, XH, DW0, DB0, C, train == 1 and norm)
    an.check(tag + " dw", DW, wdw); an.check(tag + " db", DB, wdb)
    if norm:
        assert np.array_equal(dXH.get(h, (rows, C)), XH) and np.array_equal(dR.get(h, (rows,)), R) and np.array_equal(dW.get(h, (C,)), Wg), tag
    if "DX=DY" not in inplace:
        assert np.array_equal(dDY.get(h, (rows, C)), DY), tag
    if dy2 and "DX=DY2" not in inplace:
        assert np.array_equal(dD2.get(h, (rows, C)), DY2), tag
    guards_intact(*[d for d in (dX, dS, dO, dXH, dR, dW, dB, dDY, dD2, dDX, dDW, dDB) if d is not None])
    return pf, O, XH, R, DX, DW, DB


# (C, floats every pointer is off 16 bytes): the issue's list, each rung and T boundary +- one load width on either load path, the largest admitted
GRID = [(1, 0), (3, 0), (4, 0), (5, 0), (20, 0), (64, 0), (252, 0), (256, 0), (260, 0), (512, 0), (516, 0), (1024, 0), (1028, 0), (2048, 0), (2052, 0), (8192, 0),
        (64, 1), (65, 0), (128, 1), (129, 0), (256, 1), (257, 0), (512, 1), (513, 0), (2047, 0), (2048, 1)]
CASES = [(mode, skip, dy2) for mode in (0, 1, 2) for skip in (0, 1) for dy2 in (0, 1)]


@pytest.mark.parametrize("C,off", GRID, ids=["c%d_o%d" % g for g in GRID])
def test_grid(t4k, C, off):
    """rows 1, 2, TPW - 1, TPW, TPW + 1, 2 TPW + 3 with TPW read from the plan, every mode, with and without a skip and a dy2; the rung and T asserted against
    the rule restated in tests/an_witness.py (team_of)"""
    vw = 4 if C % 4 == 0 and not off else 1
    T, rung = an.team_of(C, vw)
    tpw = plan(t4k, 1, C, 1, int(not off))[2]
    assert tpw == 256 // T
    offs = {k: off for k in ("X", "S", "O", "XH", "W", "B", "DY", "DY2", "DX")}
    for rows in sorted({1, 2, max(tpw - 1, 1), tpw, tpw + 1, 2 * tpw + 3}):
        for mode, skip, dy2 in CASES:
            run_case(t4k, "grid", rows, C, mode, skip, dy2, off=offs, rung=rung if mode else 0, T=T if mode else 0)


WALK = [(20, 8, 1), (260, 16, 1), (516, 32, 1), (1028, 64, 1), (2052, 256, 2)]


@pytest.mark.parametrize("C,T,rung", WALK, ids=["c%d" % w[0] for w in WALK])
def test_a_workgroup_walks_its_slab_more_than_once(t4k, C, T, rung):
    """one token visit more than the backward has workgroups: every workgroup of the backward but the last makes two visits (the plan's slab rows show it), and
    the forward's spread over twice as many workgroups is another split of the same tokens"""
    tpw = 256 // T
    rows = 1024 * tpw + 1
    p = plan(t4k, rows, C, 1)
    assert p[5] == 513 and p[2] == tpw, p
    for mode in (1, 2):
        run_case(t4k, "walk", rows, C, mode, 1, 1, rung=rung, T=T)


def test_offset_data(t4k):
    """x = 1024 + N(0, 1): the bound carries no cancellation term, so E[z^2] - mean^2 would leave it (tests/test_addnorm_plan.py)"""
    for C in (20, 260, 2052):
        run_case(t4k, "offset", 37, C, 1, 1, 1, kind="offset")


SINGLE = [{}] + [{k: 1} for k in ("X", "S", "O", "XH", "W", "B", "DY", "DY2", "DX")] + \
         [{k: 1 for k in ("X", "S", "O", "XH", "W", "B", "DY", "DY2", "DX", "RSTD", "DW", "DB")}]


@pytest.mark.parametrize("off", SINGLE, ids=["+".join(sorted(o)) or "aligned" for o in SINGLE])
def test_pointers_off_16_bytes(t4k, off):
    """every pointer, and each single pointer, 4 bytes off: the dword path at C % 4 == 0, asserted through the plan (run_case)"""
    for rows, C in ((35, 20), (35, 256), (9, 516), (3, 2048)):
        for mode in (0, 1, 2):
            run_case(t4k, "off", rows, C, mode, off=off)


SHAPES = [(67, 20), (35, 260), (9, 1028), (5, 2052)]


def test_in_place(t4k):
    """O == X, O == S, DX == DY and DX == DY2 give the bits of separate buffers"""
    for rows, C in SHAPES:
        for mode in (0, 1, 2):
            a = run_case(t4k, "inpl", rows, C, mode)
            for where in (("O=X", "DX=DY"), ("O=S", "DX=DY2")):
                b = run_case(t4k, "inpl", rows, C, mode, inplace=where)
                for x, y in zip(a[1:], b[1:]):
                    assert np.array_equal(x, y, equal_nan=True), (rows, C, mode, where)


def test_train_0(t4k):
    """train == 0: DW and DB untouched (run_case holds them to their prior values exactly), and allowed NULL; one launch"""
    for rows, C in SHAPES:
        for mode in (1, 2):
            a = run_case(t4k, "tr", rows, C, mode, train=1)
            b = run_case(t4k, "tr", rows, C, mode, train=0)
            c = run_case(t4k, "tr", rows, C, mode, train="null")
            assert np.array_equal(a[4], b[4]) and np.array_equal(a[4], c[4])


def test_the_same_bits_twice(t4k):
    for rows, C in SHAPES + [(32 * 1024 + 1, 20)]:
        for mode in (1, 2):
            a = run_case(t4k, "twice", rows, C, mode)
            b = run_case(t4k, "twice", rows, C, mode)
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y), (rows, C, mode)


@pytest.mark.parametrize("rows,C", [(67, 20), (130, 260), (9, 2052), (2 * 2048 * 32 + 5, 4)], ids=lambda v: str(v))
def test_a_split_of_the_rows_gives_the_same_bits(t4k, rows, C):
    """a token's results depend on that token alone: O, XH, RSTD and DX of one call are bit-equal to two calls on the two parts (a sharded batch trains like the
    whole one); the last shape has more token visits than the forward has workgroups, so the parts are walked otherwise than the whole"""
    h = t4k
    X, S, Wg, B, DY, DY2, _, _ = data(5, rows, C)
    for mode in (1, 2):
        outs = []
        for lo, hi in ((0, rows), (0, rows // 3), (rows // 3, rows)):
            r = hi - lo
            dX, dS, dDY, dD2, dW, dB = Dev(X[lo:hi]), Dev(S[lo:hi]), Dev(DY[lo:hi]), Dev(DY2[lo:hi]), Dev(Wg), Dev(B)
            dO, dXH, dDX, dR = Dev(nan(r * C)), Dev(nan(r * C)), Dev(nan(r * C)), Dev(nan(r))
            h.call("t4k_addnorm_fwd", dX.p, dS.p, dO.p, dXH.p, dR.p, dW.p, dB.p, r, C, mode, EPS, None)
            h.call("t4k_addnorm_bwd", dW.p, dDY.p, dD2.p, dXH.p, dR.p, dDX.p, None, None, r, C, mode, 0, None)
            outs.append([d.get(h, (r, -1)).copy() for d in (dO, dXH, dR, dDX)])
        for k in range(4):
            assert np.array_equal(outs[0][k], np.concatenate([outs[1][k], outs[2][k]])), (mode, k)


def test_exact_cases(t4k):
    """S = -X: z = 0 exactly, so XH = 0 and O = beta; DY = DY2 = 0: DX = 0 and DW | DB keep their bits"""
    for rows, C in SHAPES:
        for mode in (1, 2):
            _, O, XH, R, _, _, _ = run_case(t4k, "cancel", rows, C, mode, kind="cancel")
            B = data(zlib.crc32(repr(("cancel", rows, C, "cancel")).encode()), rows, C, "cancel")[3]
            assert not XH.any() and np.array_equal(O, np.broadcast_to(B, O.shape))
            assert np.array_equal(R, np.full(rows, np.float32(1.0) / np.sqrt(np.float32(EPS), dtype=np.float32)))
            _, _, _, _, DX, DW, DB = run_case(t4k, "zdy", rows, C, mode, kind="zero_dy")
            d = data(zlib.crc32(repr(("zdy", rows, C, "zero_dy")).encode()), rows, C, "zero_dy")
            assert not DX.any() and np.array_equal(DW, d[6]) and np.array_equal(DB, d[7])
        _, O, _, _, DX, _, _ = run_case(t4k, "cancel", rows, C, 0, kind="cancel")
        assert not O.any()


def test_rejections(t4k):
    """every rejection: its code, a text, nothing launched, nothing written"""
    h = t4k
    rows, C = 5, 8
    n = rows * C
    X, S, Wg, B, DY, DY2, DW0, DB0 = data(9, rows, C)
    dX, dS, dW, dB, dDY, dD2 = Dev(X), Dev(S), Dev(Wg), Dev(B), Dev(DY), Dev(DY2)
    big = Dev(nan(4 * n))                                                    # room for operands that overlap
    dO, dXH, dR, dDX, dDW, dDB = Dev(nan(n)), Dev(nan(n)), Dev(nan(rows)), Dev(nan(n)), Dev(nan(C)), Dev(nan(C))
    at = lambda d, k: ctypes.c_void_p(d.t.data_ptr() + 4 * (d.off + k))
    F = lambda: [dX.p, dS.p, dO.p, dXH.p, dR.p, dW.p, dB.p]
    G = lambda: [dW.p, dDY.p, dD2.p, dXH.p, dR.p, dDX.p, dDW.p, dDB.p]
    fwd = lambda a=None, shape=(rows, C, 1), eps=EPS: h.lib.t4k_addnorm_fwd(*(a or F()), *shape, eps, None)
    bwd = lambda a=None, shape=(rows, C, 1), train=1: h.lib.t4k_addnorm_bwd(*(a or G()), *shape, train, None)
    err = lambda: h.lib.t4k_last_error()
    l0 = lcount(h)
    for k in (0, 2):
        a = F(); a[k] = None
        assert fwd(a) == ERR_ARG and b"null" in err(), k
        assert fwd(a, (rows, C, 0)) == ERR_ARG and b"null" in err(), k
    for k in (3, 4, 5, 6):
        a = F(); a[k] = None
        assert fwd(a) == ERR_ARG and b"required" in err() and fwd(a, (rows, C, 2)) == ERR_ARG, k
    for k in (1, 5):
        a = G(); a[k] = None
        assert bwd(a) == ERR_ARG and b"null" in err(), k
    for k in (0, 3, 4):
        a = G(); a[k] = None
        assert bwd(a) == ERR_ARG and b"required" in err(), k
    for k in (6, 7):
        a = G(); a[k] = None
        assert bwd(a) == ERR_ARG and b"required" in err(), k
    for eps in (0.0, -1e-5, float("nan")):
        assert fwd(eps=eps) == ERR_ARG and b"eps" in err()
    for shape in ((0, C, 1), (-1, C, 1), (rows, 0, 1), (rows, -8, 2)):
        assert fwd(shape=shape) == ERR_ARG and b"extent" in err(), shape
        assert bwd(shape=shape) == ERR_ARG and b"extent" in err(), shape
    for mode in (-1, 3):
        assert fwd(shape=(rows, C, mode)) == ERR_ARG and b"mode" in err()
        assert bwd(shape=(rows, C, mode)) == ERR_ARG and b"mode" in err()
    # sizes: refused before a pointer is followed
    for shape in ((1 << 31, 1, 1), (1 << 21, 1 << 10, 2)):
        assert fwd(shape=shape) == ERR_UNSUPPORTED and b"2^31" in err(), shape
        assert bwd(shape=shape) == ERR_UNSUPPORTED and b"2^31" in err(), shape
    for shape in ((1, 8196, 1), (1, 8193, 2), (1, 1 << 20, 1)):
        assert fwd(shape=shape) == ERR_UNSUPPORTED and b"channels" in err(), shape
        assert bwd(shape=shape) == ERR_UNSUPPORTED and b"channels" in err(), shape
    a = F(); a[0] = at(dX, 1); a[2] = at(dO, 1)                               # a pointer off 16 bytes: the dword path ends at 2048 channels
    assert fwd(a, (1, 2052, 1)) == ERR_UNSUPPORTED and b"channels" in err()
    # overlaps: O may be X or S itself and DX may be DY or DY2 itself, nothing else
    for k, other in ((2, 0), (2, 1)):                                       # O one float into X / S
        a = F(); a[other] = big.p; a[k] = at(big, 1)
        assert fwd(a) == ERR_ARG and b"overlap" in err(), (k, other)
        assert fwd(a, (rows, C, 0)) == ERR_ARG and b"overlap" in err(), (k, other)
    for k, other in ((3, 0), (3, 1), (3, 2), (4, 0), (4, 3), (2, 5), (2, 6), (3, 5), (4, 6), (2, 3), (2, 4)):
        a = F(); a[other] = big.p; a[k] = big.p
        assert fwd(a) == ERR_ARG and b"overlap" in err(), (k, other)
    for k, other in ((5, 1), (5, 2)):                                       # DX one float into DY / DY2
        a = G(); a[other] = big.p; a[k] = at(big, 1)
        assert bwd(a) == ERR_ARG and b"overlap" in err(), (k, other)
        assert bwd(a, (rows, C, 0)) == ERR_ARG and b"overlap" in err(), (k, other)
    for k, other in ((5, 3), (5, 4), (5, 0), (6, 5), (7, 5), (6, 7), (6, 1), (7, 2), (6, 3), (7, 4), (6, 0)):
        a = G(); a[other] = big.p; a[k] = big.p
        assert bwd(a) == ERR_ARG and b"overlap" in err(), (k, other)
    assert lcount(h) == l0
    for d in (dO, dXH, dR, dDX, dDW, dDB, big):
        assert np.isnan(d.get(h, (d.n,))).all()
    guards_intact(dO, dXH, dR, dDX, dDW, dDB, big)
    assert fwd() == OK and bwd() == OK
    a = F(); a[2] = a[0]
    assert fwd(a) == OK
    a = F(); a[2] = a[1]
    assert fwd(a) == OK
