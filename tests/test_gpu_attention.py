"""t4k_attention_fwd / _bwd (include/t4k.h, csrc/attention.hip) through the C ABI: multi-head scaled-dot-product attention on [N, L, 3E] tokens.

Every stored tensor is held against its staged float64 witness (tests/attn_witness.py), each computed from the operands the kernel itself stored: LSE and Y from
QKV (bounds (b) and (c)), DQKV from QKV, the stored OK, DY and the stored LSE (bound (d)).  No element is excepted.  Outputs are pre-filled with NaN between guard
floats (Dev of tests/test_gpu_bcast.py): an element that was not written shows, and so does a store outside the tensor.  The rung, the tiles BQ and BK, the load
path and the launch counts come from t4k_attention_plan, the function the entries call - the shapes below are built from the tiles it reports."""
import ctypes
import zlib

import numpy as np
import pytest

import attn_witness as aw
from test_gpu_bcast import Dev
from test_gpu_pool_geo import guards_intact, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
FWD_PTRS, BWD_PTRS = ("QKV", "O", "OK", "LSE"), ("QKV", "OK", "DY", "LSE", "DQKV")       # what the 16-byte path asks of a call


def plan(h, N, L, heads, d, causal=0, aligned=1):
    out = I8()
    assert h.lib.t4k_attention_plan(N, L, heads, d, causal, aligned, 32 << 20, out) == OK, h.lib.t4k_last_error()
    return list(out)


def nan(k):
    return np.full(k, np.nan, np.float32)


def data(seed, N, L, heads, d, kind="normal"):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (N, L, 3, heads, d)).astype(np.float32)
    if kind == "peaked":
        x[:, :, 0] *= 8.0
    elif kind == "wide":                                                     # S = scale q.k has deviation 1 on N(0, 1): x 300 spans +-1e3, where exp(S) itself overflows
        x[:, :, :2] *= np.float32(np.sqrt(300.0))
    return x.reshape(N, L, 3 * heads * d), rng.normal(0.0, 1.0, (N, L, heads * d)).astype(np.float32)


def run_case(h, name, N, L, heads, d, causal, kind="normal", off=None, rung=None, ok_null=False, operands=None):
    """forward, then backward, every stored tensor against its witness; launches against the plan; operands intact; guards.  off: floats a pointer starts off
    16 bytes, by name.  Returns (plan, Y, LSE, DQKV)"""
    off = off or {}
    o = lambda k: off.get(k, 0)
    E = heads * d
    QKV, DY = operands or data(zlib.crc32(repr((name, N, L, heads, d, causal, kind)).encode()), N, L, heads, d, kind)
    fa = int(all(o(k) % 4 == 0 for k in FWD_PTRS if not (ok_null and k == "OK"))); ba = int(all(o(k) % 4 == 0 for k in BWD_PTRS))
    pf, pb = plan(h, N, L, heads, d, causal, fa), plan(h, N, L, heads, d, causal, ba)
    if rung is not None:
        assert pf[0] == rung and pb[0] == rung, (name, pf, pb)
    assert pf[1] == (4 if fa else 1) and pb[1] == (4 if ba else 1), (name, pf, pb)
    BK = pf[3]
    dQ, dO, dOK, dL = Dev(QKV, o("QKV")), Dev(nan(N * L * E), o("O")), Dev(nan(N * L * E), o("OK")), Dev(nan(N * heads * L), o("LSE"))
    tag = "%s n%d l%d h%d d%d c%d %s" % (name, N, L, heads, d, causal, kind)
    l0 = lcount(h)
    h.call("t4k_attention_fwd", dQ.p, dO.p, None if ok_null else dOK.p, dL.p, N, L, heads, d, causal, None)
    assert lcount(h) - l0 == pf[4], (tag, pf)
    Y = dO.get(h, (N, L, E)).copy(); LSE = dL.get(h, (N, heads, L)).copy(); YK = dOK.get(h, (N, L, E)).copy()
    wl, wy = aw.fwd(QKV, heads, causal, BK)
    aw.check(tag + " lse", LSE, wl); aw.check(tag + " y", Y, wy)
    if ok_null:
        assert np.isnan(YK).all(), tag
        dOK = Dev(Y, o("OK"))
    else:
        assert np.array_equal(Y.view(np.uint32), YK.view(np.uint32)), tag        # OK == O bit for bit
    assert np.array_equal(dQ.get(h, QKV.shape), QKV), tag
    # backward
    dDY, dG = Dev(DY, o("DY")), Dev(nan(3 * N * L * E), o("DQKV"))
    l0 = lcount(h)
    h.call("t4k_attention_bwd", dQ.p, dOK.p, dDY.p, dL.p, dG.p, N, L, heads, d, causal, None)
    assert lcount(h) - l0 == pb[5], (tag, pb)
    G = dG.get(h, (N, L, 3 * E)).copy()
    aw.check(tag + " dqkv", G, aw.bwd(QKV, Y, DY, LSE, heads, causal)[1])
    assert np.array_equal(dQ.get(h, QKV.shape), QKV) and np.array_equal(dDY.get(h, DY.shape), DY), tag
    assert np.array_equal(dOK.get(h, Y.shape).view(np.uint32), Y.view(np.uint32)) and np.array_equal(dL.get(h, LSE.shape), LSE), tag
    guards_intact(dQ, dO, dOK, dL, dDY, dG)
    return pf, Y, LSE, G


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_grid(t4k, d, causal):
    p = plan(t4k, 1, 1, 1, d)
    BQ, BK = p[2], p[3]
    for L in sorted({1, 2, BK - 1, BK, BK + 1, 2 * BK + 3, BQ + 1}):
        for heads in (1, 3):
            for N in (1, 2):
                for kind in ("normal", "peaked", "wide"):
                    run_case(t4k, "grid", N, L, heads, d, causal, kind)


# (rung, d): the boundary head sizes of tests/test_attention_plan.py's hand-worked rows
RUNGS = [(1, 4), (1, 16), (2, 20), (2, 32), (3, 36), (3, 64), (4, 68), (4, 128)]


@pytest.mark.parametrize("rung,d", RUNGS, ids=["r%d_d%d" % r for r in RUNGS])
def test_every_rung(t4k, rung, d):
    for causal in (0, 1):
        for off in (0, 1):
            run_case(t4k, "rung", 2, 131, 2, d, causal, off={k: off for k in set(FWD_PTRS + BWD_PTRS)}, rung=rung)


SINGLE = [{}] + [{k: 1} for k in ("QKV", "O", "OK", "LSE", "DY", "DQKV")] + [{k: 1 for k in ("QKV", "O", "OK", "LSE", "DY", "DQKV")}]


@pytest.mark.parametrize("off", SINGLE, ids=["+".join(sorted(o)) or "aligned" for o in SINGLE])
def test_pointers_off_16_bytes(t4k, off):
    """every pointer, and each single pointer, 4 bytes off: the dword path, asserted through the plan (run_case)"""
    for shape in ((2, 67, 3, 20), (1, 130, 2, 64), (2, 33, 1, 128)):
        run_case(t4k, "off", *shape, 1, off=off)
        run_case(t4k, "off", *shape, 0, off=off)


def test_ok_null_is_accepted(t4k):
    a = run_case(t4k, "oknull", 2, 70, 3, 20, 1)
    b = run_case(t4k, "oknull", 2, 70, 3, 20, 1, ok_null=True)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_the_same_bits_twice(t4k):
    for shape in ((2, 131, 3, 20, 0), (2, 131, 3, 20, 1), (1, 200, 2, 64, 1), (2, 70, 1, 128, 0)):
        a = run_case(t4k, "twice", *shape)
        b = run_case(t4k, "twice", *shape)
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), shape


@pytest.mark.parametrize("shape", [(131, 3, 20), (70, 2, 64), (67, 1, 128), (5, 2, 4)], ids=lambda s: "x".join(map(str, s)))
def test_sample_independence(t4k, shape):
    """an N = 2 call equals two N = 1 calls bit for bit, Y, LSE and DQKV (the rung is the same: asserted first)"""
    L, heads, d = shape
    for causal in (0, 1):
        assert plan(t4k, 2, L, heads, d, causal)[:4] == plan(t4k, 1, L, heads, d, causal)[:4]
        QKV, DY = data(11 + causal, 2, L, heads, d)
        whole = run_case(t4k, "indep", 2, L, heads, d, causal, operands=(QKV, DY))
        for n in (0, 1):
            part = run_case(t4k, "indep", 1, L, heads, d, causal, operands=(QKV[n:n + 1], DY[n:n + 1]))
            for x, y in zip(whole[1:], part[1:]):
                assert np.array_equal(x[n:n + 1].view(np.uint32), y.view(np.uint32)), (shape, causal, n)


@pytest.mark.parametrize("shape", [(131, 3, 20), (70, 4, 16), (40, 3, 128)], ids=lambda s: "x".join(map(str, s)))
def test_head_independence(t4k, shape):
    """permuting the heads of QKV and DY permutes Y, LSE and DQKV, bit for bit"""
    L, heads, d = shape
    N, perm = 2, np.roll(np.arange(heads), 1)
    QKV, DY = data(13, N, L, heads, d)
    QKVp = QKV.reshape(N, L, 3, heads, d)[:, :, :, perm].reshape(QKV.shape); DYp = DY.reshape(N, L, heads, d)[:, :, perm].reshape(DY.shape)
    for causal in (0, 1):
        _, Y, LSE, G = run_case(t4k, "heads", N, L, heads, d, causal, operands=(QKV, DY))
        _, Yp, LSEp, Gp = run_case(t4k, "heads", N, L, heads, d, causal, operands=(np.ascontiguousarray(QKVp), np.ascontiguousarray(DYp)))
        same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
        assert same(Y.reshape(N, L, heads, d)[:, :, perm], Yp.reshape(N, L, heads, d))
        assert same(LSE[:, perm], LSEp) and same(G.reshape(N, L, 3, heads, d)[:, :, :, perm], Gp.reshape(N, L, 3, heads, d))


@pytest.mark.parametrize("L", [64, 128])
@pytest.mark.parametrize("d", [4, 20, 64, 128])
def test_exact_cases(t4k, L, d):
    """Q = 0 and integer V in [-8, 8]: every live key weighs 1 / keys and the sums are exact.  Not causal: Y = sum_j V_jc / L bit for bit; causal: the same on the
    rows whose key count i + 1 is a power of two (the division is exact there).  LSE = ln(keys) within 1 ulp.  dY = 0 gives DQKV = 0 bit for bit."""
    N, heads = 2, 3
    rng = np.random.default_rng(17 * L + d)
    x = rng.normal(0.0, 1.0, (N, L, 3, heads, d)).astype(np.float32)
    x[:, :, 0] = 0.0; x[:, :, 2] = rng.integers(-8, 9, (N, L, heads, d)).astype(np.float32)
    QKV = x.reshape(N, L, 3 * heads * d); V = x[:, :, 2]
    for causal in (0, 1):
        _, Y, LSE, G = run_case(t4k, "exact", N, L, heads, d, causal, operands=(QKV, np.zeros((N, L, heads * d), np.float32)))
        assert not G.view(np.uint32).any(), (L, d, causal)
        keys = (np.arange(L) + 1 if causal else np.full(L, L)).astype(np.float32)
        sums = np.cumsum(V.astype(np.float64), 1) if causal else np.broadcast_to(V.astype(np.float64).sum(1, keepdims=True), V.shape)
        want = (sums.astype(np.float32) / keys[None, :, None, None]).astype(np.float32).reshape(N, L, heads * d)
        rows = (np.arange(L) + 1) & np.arange(L) == 0 if causal else np.ones(L, bool)
        assert np.array_equal(Y[:, rows].view(np.uint32), want[:, rows].view(np.uint32)), (L, d, causal)
        ref = np.log(keys).astype(np.float32)
        ulp = np.spacing(np.maximum(np.abs(ref), np.float32(2.0 ** -126)))
        off = np.abs(LSE.astype(np.float64) - ref[None, None].astype(np.float64)) / ulp[None, None].astype(np.float64)
        print("exact L %d d %d causal %d: LSE at most %.3g ulp from numpy's float32 log (row %d)" % (L, d, causal, off.max(), int(off.max((0, 1)).argmax())))
        assert np.all(off <= 1.0), (L, d, causal)


def test_rejections(t4k):
    """every rejection: its code, a text, nothing launched, nothing written"""
    h = t4k
    N, L, heads, d = 2, 5, 3, 8
    E = heads * d
    QKV, DY = data(9, N, L, heads, d)
    dQ, dDY, dYK, dLS = Dev(QKV), Dev(DY), Dev(np.zeros(N * L * E, np.float32)), Dev(np.zeros(N * heads * L, np.float32))
    dO, dOK, dL, dG = Dev(nan(N * L * E)), Dev(nan(N * L * E)), Dev(nan(N * heads * L)), Dev(nan(3 * N * L * E))
    fwd = lambda a=None, shape=(N, L, heads, d): h.lib.t4k_attention_fwd(*(a or (dQ.p, dO.p, dOK.p, dL.p)), *shape, 0, None)
    bwd = lambda a=None, shape=(N, L, heads, d): h.lib.t4k_attention_bwd(*(a or (dQ.p, dYK.p, dDY.p, dLS.p, dG.p)), *shape, 0, None)
    l0 = lcount(h)
    for k in (0, 1, 3):
        a = [dQ.p, dO.p, dOK.p, dL.p]; a[k] = None
        assert fwd(a) == ERR_ARG and b"null" in h.lib.t4k_last_error(), k
    for k in range(5):
        a = [dQ.p, dYK.p, dDY.p, dLS.p, dG.p]; a[k] = None
        assert bwd(a) == ERR_ARG and b"null" in h.lib.t4k_last_error(), k
    for k in range(3):
        for v in (0, -1):
            s = [N, L, heads, d]; s[k] = v
            assert fwd(shape=s) == ERR_ARG and b"extent" in h.lib.t4k_last_error(), s
            assert bwd(shape=s) == ERR_ARG and b"extent" in h.lib.t4k_last_error(), s
    for dd in (0, -4, 2, 6, 132, 256):
        assert fwd(shape=(N, L, heads, dd)) == ERR_UNSUPPORTED and b"head size" in h.lib.t4k_last_error(), dd
        assert bwd(shape=(N, L, heads, dd)) == ERR_UNSUPPORTED and b"head size" in h.lib.t4k_last_error(), dd
    # 2^31 elements, and row sums beyond the workspace: refused before a pointer is followed
    assert fwd(shape=(1 << 10, 1 << 10, 8, 128)) == ERR_UNSUPPORTED and b"2^31" in h.lib.t4k_last_error()
    assert bwd(shape=(1 << 10, 1 << 10, 8, 128)) == ERR_UNSUPPORTED and b"2^31" in h.lib.t4k_last_error()
    assert fwd(shape=(1, 44739242, 1, 16)) == ERR_UNSUPPORTED and b"workspace" in h.lib.t4k_last_error()
    assert bwd(shape=(1, 44739242, 1, 16)) == ERR_UNSUPPORTED and b"workspace" in h.lib.t4k_last_error()
    # DQKV over QKV, OK or DY: an overlap the pointers and extents show
    at = lambda dev, k: ctypes.c_void_p(dev.t.data_ptr() + 4 * (dev.off + k))
    for a in ([dQ.p, dYK.p, dDY.p, dLS.p, dQ.p], [dQ.p, dYK.p, dDY.p, dLS.p, at(dQ, 4)], [at(dG, 3 * N * L * E - 4), dYK.p, dDY.p, dLS.p, dG.p],
              [dQ.p, at(dG, 8), dDY.p, dLS.p, dG.p], [dQ.p, dYK.p, at(dG, 3 * N * L * E - N * L * E), dLS.p, dG.p]):
        assert bwd(a) == ERR_ARG and b"overlap" in h.lib.t4k_last_error()
    assert lcount(h) == l0
    for dv in (dO, dOK, dL, dG):
        assert np.isnan(dv.get(h, (dv.n,))).all()
    guards_intact(dO, dOK, dL, dG)
    assert fwd() == OK and bwd() == OK
