"""t4k_pool_geo_fwd / _bwd (include/t4k.h, csrc/pool_geo.hip) through the C ABI: avg / max / min pooling with run-time K, stride, padding.

The witness is torch on the CPU in float64 with autograd - max_pool2d, the negated max_pool2d (min) and avg_pool2d(count_include_pad=True) - on tensors
permuted from NHWC.  Every case runs on two kinds of operands (tests/test_gpu_conv_geo.py's):
  integers in [-4, 4]: ties in most windows, so bit-equality of max / min forward AND backward holds the first-wins rule; the avg forward is bit-equal to
      numpy's fp32 sum / float32(K K) (the sum of at most 256 small integers is exact), the avg backward is bit-equal where K K is a power of two (an
      exact division) and inside the bound otherwise;
  floats in +-[0.5, 2): max / min forward only select - bit-equal; the others stay inside tests/f64_witness.py's per-element bound
      C_SUM n 2^-24 mag + n 2^-126 with n the roundings behind the element: ceil(K / S)^2 for a max / min backward (the covering windows), K K + 1 for an
      avg forward (the cells and the division), 2 ceil(K / S)^2 for an avg backward; mag = the same pass on absolute values.  No element is excepted.
The code bytes equal the witness's arg-max tap (return_indices=True), the pad bytes of a pixel are 0.  Outputs are pre-filled with NaN (the codes with
0xA5 bytes) between guard floats (Dev of tests/test_gpu_bcast.py): an element that was not written shows, and so does a store outside the tensor."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import f64_witness as fw
from test_gpu_bcast import Dev

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
AVG, MAXP, MINP, USAMPLE, CONV = 13, 14, 15, 17, 1                       # T4K_L_* of include/t4k.h (tests/test_pool_geo_plan.py reads them from the header)
KINDS = {"max": MAXP, "avg": AVG, "min": MINP}
I4 = ctypes.c_int * 4

GEOS = [(1, 1, 0), (1, 2, 0), (2, 2, 0), (2, 1, 1), (3, 2, 1), (3, 1, 1), (3, 3, 0), (3, 3, 1), (2, 3, 0), (3, 5, 1), (4, 2, 2), (5, 1, 2), (5, 3, 0),
        (7, 2, 3), (7, 4, 1), (9, 2, 4), (16, 3, 8)]
IMAGES = [(11, 9), (8, 13)]
GLOBALS = [(11, 11), (16, 16)]                                           # K = H1 = W1: one window, the image
CHANNELS = [1, 3, 4, 7, 8, 36]
N = 2


def lcount(h):
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return int(h.lib.t4k_launch_count())


def extent(H1, K, S, P):
    return (H1 + 2 * P - K) // S + 1


def cdiv(a, b):
    return -(-a // b)


def operands(kind, seed, n, H1, W1, C, H0, W0):
    rng = np.random.default_rng(seed)
    if kind == "int":
        g = lambda *sh: rng.integers(-4, 5, size=sh).astype(np.float32)
    else:
        g = lambda *sh: (rng.uniform(0.5, 2.0, size=sh) * rng.choice([-1.0, 1.0], size=sh)).astype(np.float32)
    return g(n, H1, W1, C), g(n, H0, W0, C)


def _nchw(a):
    return torch.tensor(a, dtype=torch.float64).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def torch_pass(layer, X, G, K, S, P):
    """(O, dX, codes | None) of the float64 forward and its autograd backward on NHWC arrays"""
    x = _nchw(X).requires_grad_()
    idx = None
    if layer == "avg":
        o = torch.nn.functional.avg_pool2d(x, K, S, P, count_include_pad=True)
    elif layer == "max":
        o, idx = torch.nn.functional.max_pool2d(x, K, S, P, return_indices=True)
    else:
        o, idx = torch.nn.functional.max_pool2d(-x, K, S, P, return_indices=True); o = -o
    o.backward(_nchw(G))
    codes = None
    if idx is not None:                                                  # flat index into the H1 x W1 plane -> tap ky * K + kx of window (i, j)
        W1 = X.shape[2]
        H0, W0 = idx.shape[2], idx.shape[3]
        y, xx = idx // W1, idx % W1
        i = torch.arange(H0).view(1, 1, H0, 1); j = torch.arange(W0).view(1, 1, 1, W0)
        ky, kx = y - (i * S - P), xx - (j * S - P)
        assert bool(((ky >= 0) & (ky < K) & (kx >= 0) & (kx < K)).all())
        codes = _nhwc(ky * K + kx).astype(np.uint8)
    return _nhwc(o), _nhwc(x.grad), codes


def witness(layer, kind, X, G, K, S, P):
    """(O witness, dX witness, codes)"""
    o, dx, codes = torch_pass(layer, X, G, K, S, P)
    cover = cdiv(K, S) ** 2
    if layer == "avg":
        if kind == "int":
            # numpy's fp32 sum / float32(K K): the window sums (divisor_override=1) of small integers are exact in fp32 in any order
            s = _nhwc(torch.nn.functional.avg_pool2d(_nchw(X), K, S, P, count_include_pad=True, divisor_override=1)).astype(np.float32)
            wo = fw.W(fw.f64(s / np.float32(K * K)), 0.0, 0)
            wdx = fw.W(dx, 0.0, 0) if (K * K) & (K * K - 1) == 0 else fw.W(dx, torch_pass(layer, np.abs(X), np.abs(G), K, S, P)[1], 2 * cover)
            return wo, wdx, None
        mo, mdx, _ = torch_pass(layer, np.abs(X), np.abs(G), K, S, P)
        return fw.W(o, mo, K * K + 1), fw.W(dx, mdx, 2 * cover), None
    wo = fw.W(o, 0.0, 0)                                                 # max / min only select
    if kind == "int":
        return wo, fw.W(dx, 0.0, 0), codes
    # the magnitude of the routed sum: the same routing (the codes come from X) on |G|
    mdx = torch_pass(layer, X, np.abs(G), K, S, P)[1]
    return wo, fw.W(dx, mdx, cover), codes


CODE_FILL = np.frombuffer(np.uint32(0xA5A5A5A5).tobytes(), np.float32)[0]


def code_dev(n, H0, W0, C, off=0):
    return Dev(np.full(n * H0 * W0 * cdiv(C, 4), CODE_FILL, np.float32), off)


def code_bytes(dev, h, n, H0, W0, C):
    return dev.get(h, (dev.n,)).view(np.uint8).reshape(n, H0, W0, 4 * cdiv(C, 4))


def guards_intact(*devs):
    for d in devs:
        t = d.t.cpu().numpy()
        assert not t[:d.off].any() and not t[d.off + d.n:].any(), "a store outside the tensor"


def plan(h, layer, n, H1, W1, C, K, S, P, aligned=3):
    out = I4()
    assert h.lib.t4k_pool_geo_plan(layer, n, H1, W1, C, K, S, P, aligned, out) == OK, h.lib.t4k_last_error()
    return list(out)


def run_case(h, name, layer, n, H1, W1, C, K, S, P, off=0, kinds=("int", "float"), twice=False):
    """forward (with codes for max / min), then the backward into a separate DX, each against the witness; one launch per entry, guards, operands intact.
    off: floats every buffer starts off 16 bytes.  twice: a second run gives the same bits, and DX = the forward-input buffer gives them too"""
    H0, W0 = extent(H1, K, S, P), extent(W1, K, S, P)
    L = KINDS[layer]
    geo = (n, H1, W1, C, H0, W0, K, S, P)
    pl = plan(h, L, n, H1, W1, C, K, S, P, 0 if off % 4 else 3)
    assert pl[:2] == [H0, W0] and pl[2] == pl[3] == (4 if (C % 4 == 0 and off % 4 == 0) else 1), pl
    nan = lambda k: np.full(k, np.nan, np.float32)
    for kind in kinds:
        X, G = operands(kind, zlib.crc32(repr((name, layer, kind, geo)).encode()), n, H1, W1, C, H0, W0)
        wo, wdx, wcodes = witness(layer, kind, X, G, K, S, P)
        dI, dG, dO = Dev(X, off), Dev(G, off), Dev(nan(G.size), off)
        dC = None if layer == "avg" else code_dev(n, H0, W0, C, off)
        pc = dC.p if dC else None
        l0 = lcount(h)
        h.call("t4k_pool_geo_fwd", L, dI.p, dO.p, pc, *geo, None)
        assert lcount(h) - l0 == 1, name
        O = dO.get(h, G.shape)
        fw.check("%s %s %s O" % (name, layer, kind), O, wo)
        if dC:
            cb = code_bytes(dC, h, n, H0, W0, C)
            assert np.array_equal(cb[..., :C], wcodes), "%s %s %s codes" % (name, layer, kind)
            assert not cb[..., C:].any(), "%s %s pad bytes" % (name, layer)
        dDX = Dev(nan(X.size), off)
        l0 = lcount(h)
        h.call("t4k_pool_geo_bwd", L, pc, dG.p, dDX.p, *geo, None)
        assert lcount(h) - l0 == 1, name
        dx = dDX.get(h, X.shape)
        fw.check("%s %s %s dX" % (name, layer, kind), dx, wdx)
        guards_intact(dO, dDX, dI, dG, *([dC] if dC else []))
        assert np.array_equal(dI.get(h, X.shape), X) and np.array_equal(dG.get(h, G.shape), G)      # the operands are intact
        if twice:
            dO2, dDX2 = Dev(nan(G.size), off), Dev(nan(X.size), off)
            dC2 = code_dev(n, H0, W0, C, off) if dC else None
            h.call("t4k_pool_geo_fwd", L, dI.p, dO2.p, dC2.p if dC2 else None, *geo, None)
            h.call("t4k_pool_geo_bwd", L, dC2.p if dC2 else None, dG.p, dDX2.p, *geo, None)
            assert np.array_equal(dO2.get(h, G.shape), O) and np.array_equal(dDX2.get(h, X.shape), dx), name
            if dC:
                assert np.array_equal(code_bytes(dC2, h, n, H0, W0, C), cb)
            h.call("t4k_pool_geo_bwd", L, pc, dG.p, dI.p, *geo, None)                             # DX = the forward-input buffer: the in-place convention
            assert np.array_equal(dI.get(h, X.shape), dx), "%s %s in place" % (name, layer)
            guards_intact(dI, dO2, dDX2)
    return pl


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: "k%ds%dp%d" % g)
def test_geometries(t4k, geo):
    K, S, P = geo
    ran = 0
    for H1, W1 in IMAGES:
        if K > H1 + 2 * P or K > W1 + 2 * P:
            continue
        for C in CHANNELS:
            for layer in KINDS:
                run_case(t4k, "geo", layer, N, H1, W1, C, K, S, P)
                ran += 1
    assert ran == len(IMAGES) * len(CHANNELS) * 3                        # none of the listed geometries is too large for either image


@pytest.mark.parametrize("HW", GLOBALS, ids=lambda g: "%dx%d" % g)
def test_global_pools(t4k, HW):
    H1, W1 = HW
    for C in CHANNELS:
        for layer in KINDS:
            run_case(t4k, "global", layer, N, H1, W1, C, H1, H1, 0)


def test_uncovered_cells_are_zero(t4k):
    """(2, 3, 0), (3, 5, 1) and (1, 2, 0): S > K leaves input cells that no window covers, (5, 3, 0) on 11 x 9 leaves rows / columns behind the last window:
    their dX is exactly 0, and written (the NaN fill is gone)"""
    h = t4k
    for K, S, P in ((2, 3, 0), (3, 5, 1), (1, 2, 0), (5, 3, 0)):
        H1, W1, C = 11, 9, 4
        H0, W0 = extent(H1, K, S, P), extent(W1, K, S, P)
        covered = np.zeros((H1 + 2 * P, W1 + 2 * P), bool)
        for i in range(H0):
            for j in range(W0):
                covered[i * S:i * S + K, j * S:j * S + K] = True
        covered = covered[P:P + H1, P:P + W1]
        assert (~covered).sum() > 0
        for layer in KINDS:
            X, G = operands("float", 7, N, H1, W1, C, H0, W0)
            dI, dG, dO, dDX = Dev(X), Dev(G), Dev(np.zeros(G.size, np.float32)), Dev(np.full(X.size, np.nan, np.float32))
            dC = code_dev(N, H0, W0, C)
            h.call("t4k_pool_geo_fwd", KINDS[layer], dI.p, dO.p, dC.p, N, H1, W1, C, H0, W0, K, S, P, None)
            h.call("t4k_pool_geo_bwd", KINDS[layer], dC.p, dG.p, dDX.p, N, H1, W1, C, H0, W0, K, S, P, None)
            dx = dDX.get(h, X.shape)
            assert not np.isnan(dx).any() and np.all(dx[:, ~covered, :] == 0.0), (layer, K, S, P)


@pytest.mark.parametrize("C", [3, 8])
def test_twice_and_in_place(t4k, C):
    """the same bits on a second run; DX = the forward-input buffer gives the bits of a separate DX (the backward reads no forward input)"""
    for K, S, P in ((3, 2, 1), (3, 1, 1), (5, 3, 0), (2, 3, 0)):
        for layer in KINDS:
            run_case(t4k, "twice", layer, N, 11, 9, C, K, S, P, kinds=("float",), twice=True)


def test_forward_without_codes(t4k):
    """CODE == NULL: inference - O alone, the same bits"""
    h = t4k
    for C in (3, 8):
        for layer in ("max", "min"):
            K, S, P, H1, W1 = 3, 2, 1, 11, 9
            H0, W0 = extent(H1, K, S, P), extent(W1, K, S, P)
            X, G = operands("float", 3, N, H1, W1, C, H0, W0)
            dI, dO = Dev(X), Dev(np.full(G.size, np.nan, np.float32))
            l0 = lcount(h)
            h.call("t4k_pool_geo_fwd", KINDS[layer], dI.p, dO.p, None, N, H1, W1, C, H0, W0, K, S, P, None)
            assert lcount(h) - l0 == 1
            fw.check("no codes", dO.get(h, G.shape), witness(layer, "float", X, G, K, S, P)[0])
            guards_intact(dI, dO)


@pytest.mark.parametrize("C", [3, 4, 8, 36])
def test_pointers_off_16_bytes(t4k, C):
    """every pointer 4 bytes (and 12 bytes) off 16-byte alignment: the scalar path - one channel per thread, byte stores of the codes -, asserted through the plan, which is the function the entries call"""
    assert plan(t4k, MAXP, N, 11, 9, C, 3, 2, 1, 0)[2:] == [1, 1]
    assert plan(t4k, MAXP, N, 11, 9, C, 3, 2, 1, 3)[2:] == ([4, 4] if C % 4 == 0 else [1, 1])
    for layer in KINDS:
        run_case(t4k, "off", layer, N, 11, 9, C, 3, 2, 1, off=1)
        run_case(t4k, "off", layer, N, 8, 13, C, 4, 2, 2, off=3, kinds=("int",))


@pytest.mark.parametrize("shape", [(15, 48, 48, 64), (3, 448, 448, 1)], ids=["v4", "v1"])
def test_above_the_launch_cap(t4k, shape):
    """more work items than MAX_WG * BLK = 2048 * 256 threads, with a remainder: the grid-stride loop, forward and backward, per vector width"""
    n, H1, W1, C = shape
    items = n * H1 * W1 * (C // 4 if C % 4 == 0 else C)
    assert items > 2048 * 256 and items % (2048 * 256)
    pl = run_case(t4k, "cap", "max", n, H1, W1, C, 3, 1, 1, kinds=("int",))
    assert pl[2] == pl[3] == (4 if C % 4 == 0 else 1)


def test_rejections(t4k):
    """a bad argument: T4K_ERR_ARG; an inadmissible layer or geometry: T4K_ERR_UNSUPPORTED; a text either way, nothing launched, the outputs untouched"""
    h = t4k
    n, H1, W1, C = 2, 8, 8, 3
    nan = lambda k: np.full(k, np.nan, np.float32)
    dI, dG = Dev(np.ones(n * H1 * W1 * C, np.float32)), Dev(np.ones(n * 17 * 17 * C, np.float32))
    dO, dDX, dC = Dev(nan(n * 17 * 17 * C)), Dev(nan(n * H1 * W1 * C)), Dev(nan(n * 17 * 17))
    bad = [((MAXP, 3, 2, 1, 4, 5), ERR_ARG, b"gives 4x4"), ((MAXP, 3, 2, 1, 5, 4), ERR_ARG, b"gives 4x4"), ((AVG, 3, 2, 1, 3, 4), ERR_ARG, b"gives 4x4"),
           ((MINP, 3, 2, 1, 4, 3), ERR_ARG, b"gives 4x4"), ((MAXP, 17, 1, 8, 8, 8), ERR_UNSUPPORTED, b"not supported"), ((MAXP, 0, 1, 0, 8, 8), ERR_UNSUPPORTED, b"not supported"),
           ((AVG, 3, 17, 1, 1, 1), ERR_UNSUPPORTED, b"not supported"), ((AVG, 3, 0, 1, 1, 1), ERR_UNSUPPORTED, b"not supported"),
           ((MINP, 3, 1, 2, 10, 10), ERR_UNSUPPORTED, b"not supported"), ((MINP, 3, 1, -1, 4, 4), ERR_UNSUPPORTED, b"not supported"),
           ((MAXP, 9, 1, 0, 1, 1), ERR_UNSUPPORTED, b"does not fit"), ((USAMPLE, 2, 2, 0, 4, 4), ERR_UNSUPPORTED, b"layer"), ((CONV, 3, 1, 1, 8, 8), ERR_UNSUPPORTED, b"layer")]
    for (L, K, S, P, H0, W0), code, text in bad:
        l0 = lcount(h)
        assert h.lib.t4k_pool_geo_fwd(L, dI.p, dO.p, dC.p, n, H1, W1, C, H0, W0, K, S, P, None) == code, (L, K, S, P)
        assert text in h.lib.t4k_last_error(), h.lib.t4k_last_error()
        assert h.lib.t4k_pool_geo_bwd(L, dC.p, dG.p, dDX.p, n, H1, W1, C, H0, W0, K, S, P, None) == code, (L, K, S, P)
        assert text in h.lib.t4k_last_error() and lcount(h) == l0
    good = (n, H1, W1, C, 4, 4, 3, 2, 1)
    l0 = lcount(h)
    assert h.lib.t4k_pool_geo_fwd(MAXP, None, dO.p, dC.p, *good, None) == ERR_ARG
    assert h.lib.t4k_pool_geo_fwd(MAXP, dI.p, None, dC.p, *good, None) == ERR_ARG
    assert h.lib.t4k_pool_geo_bwd(MAXP, dC.p, None, dDX.p, *good, None) == ERR_ARG
    assert h.lib.t4k_pool_geo_bwd(MAXP, dC.p, dG.p, None, *good, None) == ERR_ARG
    assert h.lib.t4k_pool_geo_bwd(MAXP, None, dG.p, dDX.p, *good, None) == ERR_ARG                  # a max / min backward needs its codes ...
    assert h.lib.t4k_pool_geo_bwd(MINP, None, dG.p, dDX.p, *good, None) == ERR_ARG and b"codes" in h.lib.t4k_last_error()
    for k, name in enumerate(("N", "H1", "W1", "C")):
        a = list(good); a[k] = 0
        assert h.lib.t4k_pool_geo_fwd(AVG, dI.p, dO.p, None, *a, None) == ERR_ARG and b"extent" in h.lib.t4k_last_error(), name
    assert lcount(h) == l0
    for d in (dO, dDX, dC):
        assert np.isnan(d.get(h, (d.n,))).all()
    assert h.lib.t4k_pool_geo_bwd(AVG, None, dG.p, dDX.p, *good, None) == OK and lcount(h) == l0 + 1   # ... an avg backward ignores them
    assert not np.isnan(dDX.get(h, (dDX.n,))).any()


@pytest.mark.parametrize("KS", [2, 3])
@pytest.mark.parametrize("C", [3, 8])
def test_beside_the_old_entries(t4k, KS, C):
    """K = S in {2, 3}, P = 0 on an image K divides (ceil grid = floor grid, every cell covered): O bit-equal to t4k_pool and dX bit-equal to t4k_dpool - which
    works in place on the forward input and finds the arg-max again - for all three layer kinds, on tied integers and on floats"""
    h = t4k
    H1, W1 = 12, 6
    H0, W0 = H1 // KS, W1 // KS
    for layer, L in KINDS.items():
        for kind in ("int", "float"):
            X, G = operands(kind, zlib.crc32(repr((KS, C, layer, kind)).encode()), N, H1, W1, C, H0, W0)
            nan = lambda k: np.full(k, np.nan, np.float32)
            dI, dG, oo, on, xn, xo = Dev(X), Dev(G), Dev(nan(G.size)), Dev(nan(G.size)), Dev(nan(X.size)), Dev(X)
            dC = code_dev(N, H0, W0, C)
            h.call("t4k_pool", L, dI.p, oo.p, N, H1, W1, H0, W0, C, KS, None)
            h.call("t4k_pool_geo_fwd", L, dI.p, on.p, dC.p, N, H1, W1, C, H0, W0, KS, KS, 0, None)
            assert np.array_equal(oo.get(h, G.shape), on.get(h, G.shape)), (layer, kind)
            h.call("t4k_dpool", L, xo.p, dG.p, N, H1, W1, H0, W0, C, KS, None)
            h.call("t4k_pool_geo_bwd", L, dC.p, dG.p, xn.p, N, H1, W1, C, H0, W0, KS, KS, 0, None)
            assert np.array_equal(xo.get(h, X.shape), xn.get(h, X.shape)), (layer, kind)
            guards_intact(oo, on, xn, xo, dC)
