"""One case per rung of the release conv dispatch, bit for bit against float64.

Operands, bias, output gradients and the pre-loaded DF / DB are integers in {-2..2}: a product is at most 4, a forward / dX
element sums at most 25 * 128 taps x channels of them (12 800), a dF / dB element at most 65 536 pixels (2^18): every fp32 partial sum is an
integer below 2^24 and therefore exact in ANY order.  Whatever kernel a rung selects must equal the float64 reference (torch on the
CPU) exactly; `np.array_equal`, no tolerance.  Each shape is the smallest its rung's own admission test accepts (a few ragged /
multi-block extents where they cost nothing); the comment of a case says which predicate fixes which extent.  CU count = 256 (MI355X).
Rungs reachable only in a LAB build stay with test_lab_conv_parity_under_the_conv_engine_switches."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L_RELU, L_AVGPOOL, L_MAXPOOL, L_MINPOOL, L_USAMPLE = 4, 13, 14, 15, 17        # t4_layer, include/t4k.h
GEO = {1: (1, 1, 0), 3: (3, 1, 1), 4: (4, 2, 1), 5: (5, 1, 2)}                 # the four admitted (K, S, P)


class PoolBlock(ctypes.Structure):
    _fields_ = [("pre_layer", ctypes.c_int), ("pre_alpha", ctypes.c_float), ("pre_mask", ctypes.c_void_p), ("pre_out", ctypes.c_void_p),
                ("pool_layer", ctypes.c_int), ("KS", ctypes.c_int), ("pool_out", ctypes.c_void_p),
                ("post_layer", ctypes.c_int), ("post_alpha", ctypes.c_float), ("post_mask", ctypes.c_void_p), ("post_out", ctypes.c_void_p),
                ("copy_out", ctypes.c_void_p)]


class Dev:
    """device buffers via torch (plumbing only); pointers cross the ABI as integers"""

    def __init__(self, t4k):
        import torch
        self.torch = torch
        self.h = t4k
        t4k.call("t4k_set_default_stream", None)
        self.keep = []

    def up(self, a, skew=0):
        """skew: leading floats, so that the tensor starts 4 * skew bytes past a 16-byte boundary"""
        flat = np.concatenate([np.zeros(skew, np.float32), np.asarray(a, np.float32).ravel()])
        t = self.torch.from_numpy(flat).cuda()
        self.keep.append(t)
        del self.keep[:-64]
        return t[skew:].view(*np.shape(a))

    def zeros(self, shape):
        return self.up(np.zeros(shape, np.float32))

    def down(self, t):
        self.h.call("t4k_sync", None)
        return t.cpu().numpy()


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


def p(t):
    return None if t is None else t.data_ptr()


def ints(rng, *shape):
    return rng.integers(-2, 3, shape).astype(np.float32)


def out_hw(H1, W1, K, S, P):
    return (H1 + 2 * P - K) // S + 1, (W1 + 2 * P - K) // S + 1


# ---- float64 references (NHWC tensors, filter [C1][K][K][C0]) ----
def _nchw(torch, a):
    return torch.from_numpy(np.asarray(a, np.float64)).permute(0, 3, 1, 2).contiguous()


def ref_fwd(torch, I, F, B, S, P):
    w = torch.from_numpy(F.astype(np.float64)).permute(3, 0, 1, 2).contiguous()
    return torch.nn.functional.conv2d(_nchw(torch, I), w, torch.from_numpy(B.astype(np.float64)), stride=S, padding=P).permute(0, 2, 3, 1).numpy()


def ref_dx(torch, G, F, H1, W1, S, P):
    K = F.shape[1]; H0, W0 = G.shape[1:3]
    # the library's dX is the reference's (nmath.tcu:304-324, conv.hip): dX[pix1, c1] = sum dO[pix1 shifted, c0] * F[c1, K-1-ky, K-1-kx, c0], the transposed
    # convolution with the taps FLIPPED.  conv_transpose2d: weight [in = C0][out = C1][K][K]
    w = torch.from_numpy(F[:, ::-1, ::-1, :].astype(np.float64)).permute(3, 0, 1, 2).contiguous()
    op = (H1 - ((H0 - 1) * S - 2 * P + K), W1 - ((W0 - 1) * S - 2 * P + K))
    return torch.nn.functional.conv_transpose2d(_nchw(torch, G), w, stride=S, padding=P, output_padding=op).permute(0, 2, 3, 1).numpy()


def ref_df(torch, I, G, K, S, P):
    C1, C0 = I.shape[3], G.shape[3]
    return torch.nn.grad.conv2d_weight(_nchw(torch, I), (C0, C1, K, K), _nchw(torch, G), stride=S, padding=P).permute(1, 2, 3, 0).numpy()


def same(got, want):
    want = np.asarray(want)
    return got.shape == want.shape and np.array_equal(got.astype(np.float64), want.astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ forward
# (id, N, H1, W1, C1, C0, K, icopy, skew)
FWD = [
    # conv_few_ok: Cin <= 4, Cout <= 32, K in {3, 5}.  Cin == 1 -> CH 1; Cout <= 4 -> G 4.  297 pixels: two workgroups, ragged
    ("few_cin1_ch1_g4", 3, 11, 9, 1, 3, 3, True, 0),
    # odd Cin in 2..4 -> CH 4, VW 1; Cout = 5 > 4 -> G 12, one channel group
    ("few_cin3_vw1_g12", 3, 11, 9, 3, 5, 3, False, 0),
    # even Cin, input on an 8-byte boundary -> VW 2
    ("few_cin2_vw2", 3, 11, 9, 2, 4, 3, False, 0),
    # even Cin, input 4 bytes past the boundary -> v2 false, VW 1
    ("few_cin4_unaligned_vw1", 2, 6, 5, 4, 4, 3, False, 1),
    # Cout = 13 > 12 -> two channel groups of 12 (the second with one valid channel)
    ("few_g12_two_groups", 2, 6, 5, 2, 13, 3, False, 0),
    # K = 5
    ("few_k5", 2, 6, 5, 1, 3, 5, False, 0),
    # conv_thin_fwd: K 3, C1 in 1..4, C0 in {32, 64}; conv_few_ok takes C0 <= 32 first, so C0 = 64.  70 pixels: ragged last 32-pixel tile
    ("thin_fwd", 2, 5, 7, 3, 64, 3, False, 0),
    ("thin_fwd_icopy", 2, 5, 7, 4, 64, 3, True, 0),
    # gather GEMM (no other rung admits: K = 1 is not a few-channel kernel, C1 % 32 != 0 is not a many-channel one).
    # conv_gemm_ksplit: pairs * K * K = 2 < 18 -> ksplit 1
    ("gather_ksplit1_k1", 2, 5, 7, 3, 5, 1, True, 0),
    # pairs * K * K = 3 * 9 >= 18 and 3 waves < 1536 -> ksplit 2
    ("gather_ksplit2", 2, 5, 7, 5, 7, 3, False, 0),
    # (4,2,1) geometry on the gather kernel, ksplit 2 (2 * 16 >= 18)
    ("gather_k4s2", 2, 6, 8, 3, 5, 4, False, 0),
    # filter larger than the 8192-float LDS stage (40 * 9 * 72): staged per chunk of channel pairs, three channel tiles
    ("gather_staged_filter", 1, 4, 5, 40, 72, 3, False, 0),
    # 768 pixel tiles x 2 channel tiles = 1536 waves -> ksplit 1 by size
    ("gather_1536_waves", 6, 64, 64, 5, 33, 3, False, 0),
    # conv_big_ok: Cin >= 32, % 32 == 0, Cout >= 16, % 4 == 0.  k_convbig8 wants Cin % 64 == 0: Cin = 32 -> k_convbig
    ("convbig_cin32", 2, 8, 8, 32, 16, 3, False, 0),
    # ... stride 2 -> k_convbig
    ("convbig_k4s2", 2, 8, 8, 64, 16, 4, False, 0),
    # ... 25 pixels < 128 -> k_convbig
    ("convbig_under_128_pixels", 1, 5, 5, 64, 16, 3, False, 0),
    # k_convbig 128-wide tile: Cout = 68 > 64 and 256 pixel tiles x 1 >= CUs
    ("convbig_wide", 8, 64, 64, 32, 68, 1, False, 0),
    # k_convbig8: S 1, P K/2, Cin % 64 == 0, same grid, >= 128 pixels.  Cout <= 64 -> 64-wide tile
    ("convbig8_n64", 2, 8, 8, 64, 16, 3, False, 0),
    ("convbig8_k5", 2, 8, 8, 64, 20, 5, False, 0),
    # Cout = 128 > 64 and 256 pixel tiles x 1 >= CUs -> 128-wide; 256 tiles < 2 per CU -> 64-deep stages
    ("convbig8_n128", 8, 64, 64, 64, 128, 1, False, 0),
    # 512 tiles >= 2 per CU -> 32-deep stages, two workgroups per CU (64-wide tile)
    ("convbig8_bk32", 16, 64, 64, 64, 64, 1, False, 0),
    # 256 pixel tiles x 2 channel tiles: 128-wide and 32-deep
    ("convbig8_n128_bk32", 8, 64, 64, 64, 256, 1, False, 0),
    # 210 pixels (ragged second 128-pixel tile), 68 channels (ragged second 64-wide tile)
    ("convbig8_ragged", 5, 6, 7, 64, 68, 3, False, 0),
]


@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_forward_rung(t4k, dev, case):
    _, N, H1, W1, C1, C0, K, icopy, skew = case
    _, S, P = GEO[K]
    H0, W0 = out_hw(H1, W1, K, S, P)
    rng = np.random.default_rng(N * 1000 + C1 * 10 + C0)
    I, F, B = ints(rng, N, H1, W1, C1), ints(rng, C1, K, K, C0), ints(rng, C0)
    want = ref_fwd(dev.torch, I, F, B, S, P)
    dI, dF, dB, dO = dev.up(I, skew), dev.up(F), dev.up(B), dev.up(np.full(want.shape, 7.0, np.float32))
    dC = dev.zeros(I.shape) if icopy else None
    t4k.call("t4k_conv2d_fwd2", p(dI), p(dC), p(dO), p(dF), p(dB), N, H1, W1, C1, H0, W0, C0, K, S, P, None)
    assert same(dev.down(dO), want)
    if icopy: assert np.array_equal(dev.down(dC), I)


# (id, N, H, W, C1, C0, K, icopy): t4k_conv2d_block_fwd, `fusable`: 2x2 pool on an even grid, S 1, K in {3, 5}, not a many-channel layer
BLOCK = [
    # conv_img_block_fwd: K 3, C1 in {1, 3}, C0 in {4, 6, 8, 10, 12, 16}.  70 pool windows: two 64-window workgroups
    ("img_block", 2, 10, 14, 3, 6, 3, True),
    # C1 = 2 is no image layer -> k_conv_gemm_pool<3,1,1>
    ("gemm_pool_k3", 2, 6, 10, 2, 5, 3, True),
    # K = 5 is no image layer -> k_conv_gemm_pool<5,1,2>; C1 = 5 > 4: the layer-0 copy is a memcpy
    ("gemm_pool_k5", 2, 6, 10, 5, 3, 5, True),
]


@pytest.mark.parametrize("case", BLOCK, ids=[c[0] for c in BLOCK])
def test_block_forward_rung(t4k, dev, case):
    _, N, H, W, C1, C0, K, icopy = case
    _, S, P = GEO[K]
    rng = np.random.default_rng(N * 1000 + C1 * 10 + C0)
    I, F, B = ints(rng, N, H, W, C1), ints(rng, C1, K, K, C0), ints(rng, C0)
    Y = ref_fwd(dev.torch, I, F, B, S, P)
    Q = Y.reshape(N, H // 2, 2, W // 2, 2, C0).max(axis=(2, 4)); R = np.maximum(Q, 0.0)          # maxpool 2x2, relu behind it
    dI, dF, dB, dY, dC = dev.up(I), dev.up(F), dev.up(B), dev.zeros(Y.shape), dev.zeros(I.shape)
    dQ, dR, dM, dR2 = dev.zeros(Q.shape), dev.zeros(Q.shape), dev.zeros(Q.shape), dev.zeros(Q.shape)
    blk = PoolBlock(); blk.KS = 2; blk.pool_layer = L_MAXPOOL; blk.pool_out = p(dQ)
    blk.post_layer = L_RELU; blk.post_mask = p(dM); blk.post_out = p(dR); blk.copy_out = p(dR2)
    t4k.call("t4k_conv2d_block_fwd", p(dI), p(dC) if icopy else None, p(dY), p(dF), p(dB), ctypes.byref(blk), N, H, W, C1, H, W, C0, K, S, P, None)
    assert same(dev.down(dY), Y) and same(dev.down(dQ), Q) and same(dev.down(dR), R) and same(dev.down(dR2), R)
    if icopy: assert np.array_equal(dev.down(dC), I)


# k_convbig8's batch-norm rider (t4k_conv2d_bn_fwd): pixels % 128 == 0 and Cout % tile width == 0 admit it; 210 pixels refuse it
@pytest.mark.parametrize("N,H,W", [(2, 8, 8), (5, 6, 7)], ids=["rider", "refused"])
def test_convbig8_batchnorm_rider(t4k, dev, N, H, W):
    """The conv output is exact.  So are the per-channel sum and sum of squares in fp32, in either path: |y| <= 64 * 9 * 4 + 2 sums to far less than
    2^24 over 210 pixels, and y^2 (variance 64 * 9 * 4) to about 2^19; the test asserts both.  The mean is then one correctly rounded division: compared
    bitwise.  1 / (sigma + 1e-6) goes through var = sumsq / n - mean^2 (rounded once with an fma, twice without; no cancellation, the means are small beside
    sigma), a square root, an addition and a division, each within half an ulp: held to 8 * 2^-24 relative.  x-hat = (y - mean) / (sigma + eps) from the library's
    own factor is a subtraction and a product, the output one or two roundings more: each held to 8 * 2^-24 of the magnitudes that enter it."""
    C1, C0, K, S, P = 64, 64, 3, 1, 1
    U = 2.0 ** -24
    rng = np.random.default_rng(N)
    I, F, Bc, g, b = ints(rng, N, H, W, C1), ints(rng, C1, K, K, C0), ints(rng, C0), ints(rng, C0), ints(rng, C0)
    Y = ref_fwd(dev.torch, I, F, Bc, S, P)
    n = N * H * W
    s1, s2 = Y.sum(axis=(0, 1, 2)), (Y * Y).sum(axis=(0, 1, 2))
    assert s2.max() < 2 ** 24 and np.abs(Y).sum(axis=(0, 1, 2)).max() < 2 ** 24
    mean = s1 / n; var = s2 / n - mean * mean
    dI, dF, dBc, dg, db = dev.up(I), dev.up(F), dev.up(Bc), dev.up(g), dev.up(b)
    dY, dO, dXH, dst = dev.zeros(Y.shape), dev.zeros(Y.shape), dev.zeros(Y.shape), dev.zeros((3 * C0,))
    t4k.call("t4k_conv2d_bn_fwd", p(dI), None, p(dY), p(dF), p(dBc), N, H, W, C1, H, W, C0, K, S, P, p(dO), p(dXH), p(dg), p(db), p(dst), None)
    assert same(dev.down(dY), Y)
    st = dev.down(dst).astype(np.float64)
    m32 = mean.astype(np.float32).astype(np.float64)
    assert np.array_equal(st[C0:2 * C0], m32)
    istd = st[:C0]
    want_istd = 1.0 / (np.sqrt(var) + 1.0e-6)
    assert np.all(np.abs(istd - want_istd) <= 8 * U * want_istd)
    xh = (Y - m32) * istd
    assert np.all(np.abs(dev.down(dXH) - xh) <= 8 * U * (np.abs(Y) + np.abs(m32)) * istd)
    assert np.all(np.abs(dev.down(dO) - (xh * g + b)) <= 8 * U * ((np.abs(Y) + np.abs(m32)) * istd * np.abs(g) + np.abs(b)))


# ------------------------------------------------------------------------------------------------------------------ backward
# (id, N, H1, W1, C1, C0, K).  The comment names the dF | dB engine, the fold and the dX engine the release dispatch picks.
BWD = [
    # dF: conv_big_ok(C1, C0); k_convbig_dfw wants C1 % 128 == 0 and C0 % 64 == 0, S 1, same grid.  128 pixels -> 1 slice (<= 32: k_fold_add); dB: colsum_add, one chunk
    # dX: conv_big_ok(C0, C1), C0 % 64 == 0, 128 pixels -> k_convbig8<BWD>
    ("dfw__fold_add__dx_convbig8", 2, 8, 8, 128, 64, 3),
    # k_convbig_dfw, 12 288 pixels / 256 per slice = 48 slices (> 32: k_conv_df_fold); dB: colsum_add, 48 chunks
    ("dfw_48_slices__df_fold", 3, 64, 64, 128, 64, 1),
    # dF: C1 = 32 is no whole 128 -> k_convbig_df8, C1 == 32 -> two taps per tile.  dX: Cin = C0 = 64 -> k_convbig8<BWD>
    ("df8_tp2__dx_convbig8", 2, 8, 8, 32, 64, 3),
    # dF: k_convbig_df8, one tap per tile (C1 = 64).  dX: C0 = 16 < 32 is no many-channel dX, C1 > 4, K = 1 -> k_conv_dx_and_fold (no fold left to carry)
    # 12 288 pixels -> 48 slices -> k_conv_df_fold, colsum_add with 48 chunks
    ("df8_48_slices__df_fold__dx_gather", 3, 64, 64, 64, 16, 1),
    # k_convbig_df8 on the (4,2,1) geometry; 32 output pixels -> 1 slice -> k_fold_add
    ("df8_k4s2", 2, 8, 8, 64, 16, 4),
    # dF: conv_big_ok(16, 32) fails, C1 = 16 is no image layer -> k_conv_df_mfma; dX: conv_big_ok(32, 16), Cin = 32 -> k_convbig<BWD>: the fold is launched alone
    ("df_mfma__fold_alone__dx_convbig", 2, 8, 8, 16, 32, 3),
    # conv_thin_df: K 3, C1 in 1..3, C0 in {32, 64}.  dX: dx_few (C1 <= 4) and dx_wide (K 3, C0 in {32, 64, 128}): k_conv_dx_wide<C1, C0 / 4> carries the fold
    ("thin_df__dx_wide_c32", 2, 5, 7, 1, 32, 3),
    ("thin_df__dx_wide_c64", 2, 5, 7, 3, 64, 3),
    # C0 = 128 is no thin layer -> k_conv_df_mfma; dx_wide with 32 lanes per pixel; C1 = 4
    ("df_mfma__dx_wide_c128", 2, 5, 7, 4, 128, 3),
    # k_conv_df_mfma with one slice: N * H0 = 4 rows = one wave row each
    ("df_mfma_one_slice__dx_and_fold", 1, 4, 5, 5, 7, 3),
    # ... with several: 33 rows -> 9 slices; dX: nothing else admits (C1 = 5 > 4, C0 = 7 > 4) -> k_conv_dx_and_fold carries the fold
    ("df_mfma_slices__dx_and_fold", 3, 11, 9, 5, 7, 3),
    # k_conv_dx_and_fold on the other geometries
    ("dx_and_fold_k1", 2, 5, 7, 5, 7, 1),
    ("dx_and_fold_k4s2", 2, 6, 8, 5, 7, 4),
    ("dx_and_fold_k5", 2, 5, 7, 5, 7, 5),
    # dx_fewch: conv_few_ok(K, C0, C1) with C0 <= 4 and 4 < C1 <= 32 -> k_conv_few<BWD>; it carries no fold: launched alone
    ("dx_fewch", 3, 11, 9, 7, 3, 3),
    ("dx_fewch_k5_g12_two_groups", 2, 6, 5, 13, 2, 5),
]
# dx_few: C1 <= 4 and the filter fits the LDS stage -> k_conv_dx_few<K, S, P, C1>, every C1 in 1..4 on every geometry;
# C0 = 5 / 6 / 8 / 3: the scalar, 8-byte and 16-byte channel loops.  297 input pixels: two workgroups
BWD += [("dx_few_c%d_k%d" % (c1, k), 3, 11 if k != 4 else 12, 9 if k != 4 else 10, c1, (5, 6, 8, 3)[c1 - 1], k) for c1 in (1, 2, 3, 4) for k in (1, 3, 4, 5)]


def run_bwd(t4k, dev, I, G, F, DF0, DB0, geo, dx, dx2, df):
    N, H1, W1, C1 = I.shape; _, H0, W0, C0 = G.shape; K, S, P = geo
    dI, dG, dF = dev.up(I), dev.up(G), dev.up(F)
    dDX = dev.up(np.full(I.shape, 7.0, np.float32)) if dx else None
    dDX2 = dev.up(np.full(I.shape, 9.0, np.float32)) if dx2 else None
    dDF, dDB = (dev.up(DF0), dev.up(DB0)) if df else (None, None)
    t4k.call("t4k_conv2d_bwd2", p(dI), p(dG), p(dDX), p(dDX2), p(dF), p(dDF), p(dDB), N, H1, W1, C1, H0, W0, C0, K, S, P, 1, None)
    return [None if t is None else dev.down(t) for t in (dDX, dDX2, dDF, dDB)]


@pytest.mark.parametrize("case", BWD, ids=[c[0] for c in BWD])
def test_backward_rung(t4k, dev, case):
    """Four calls per rung: the fold riding (DX, DF, DB), the same with the second dX copy, the fold alone (DX == NULL), dX alone (DF == DB == NULL)"""
    _, N, H1, W1, C1, C0, K = case
    geo = GEO[K]; _, S, P = geo
    H0, W0 = out_hw(H1, W1, K, S, P)
    rng = np.random.default_rng(N * 1000 + C1 * 10 + C0 + K)
    I, G, F = ints(rng, N, H1, W1, C1), ints(rng, N, H0, W0, C0), ints(rng, C1, K, K, C0)
    DF0, DB0 = ints(rng, C1, K, K, C0), ints(rng, C0)
    torch = dev.torch
    wdx = ref_dx(torch, G, F, H1, W1, S, P)
    wdf = ref_df(torch, I, G, K, S, P) + DF0
    wdb = G.astype(np.float64).sum(axis=(0, 1, 2)) + DB0
    dx, _, df, db = run_bwd(t4k, dev, I, G, F, DF0, DB0, geo, True, False, True)
    assert same(dx, wdx) and same(df, wdf) and same(db, wdb)
    dx, dx2, df, db = run_bwd(t4k, dev, I, G, F, DF0, DB0, geo, True, True, True)
    assert same(dx, wdx) and np.array_equal(dx2, dx) and same(df, wdf) and same(db, wdb)
    _, _, df, db = run_bwd(t4k, dev, I, G, F, DF0, DB0, geo, False, False, True)
    assert same(df, wdf) and same(db, wdb)
    dx, dx2, _, _ = run_bwd(t4k, dev, I, G, F, DF0, DB0, geo, True, True, False)
    assert same(dx, wdx) and np.array_equal(dx2, dx)


# ------------------------------------------------------------------------------------------------------------------ other
def ref_pool(layer, I, KS, H0, W0):
    N, H1, W1, C = I.shape
    O = np.zeros((N, H0, W0, C))
    for i in range(H0):
        for j in range(W0):
            win = I[:, i * KS:min(H1, i * KS + KS), j * KS:min(W1, j * KS + KS), :].astype(np.float64)     # clipped at the edge of an odd grid
            if layer == L_MAXPOOL: O[:, i, j, :] = win.max(axis=(1, 2))
            elif layer == L_MINPOOL: O[:, i, j, :] = win.min(axis=(1, 2))
            else: O[:, i, j, :] = (win.sum(axis=(1, 2)) / (KS * KS)).astype(np.float32)                   # one correctly rounded fp32 division of an exact sum
    return O


def ref_dpool(layer, X, DY, KS):
    """in place on the forward input: avg / upsample spread dy, max / min zero the window and give dy to its first extreme (row-major scan)"""
    N, H1, W1, C = X.shape; _, H0, W0, _ = DY.shape
    R = X.astype(np.float64).copy()
    for i in range(H0):
        for j in range(W0):
            ys, xs = range(i * KS, min(H1, i * KS + KS)), range(j * KS, min(W1, j * KS + KS))
            dy = DY[:, i, j, :].astype(np.float64)
            if layer == L_AVGPOOL or layer == L_USAMPLE:
                for y in ys:
                    for x in xs: R[:, y, x, :] = (dy / (KS * KS)).astype(np.float32) if layer == L_AVGPOOL else dy
                continue
            best = None; arg = None
            for y in ys:
                for x in xs:
                    v = X[:, y, x, :].astype(np.float64)
                    if best is None: best = v.copy(); arg = np.full(v.shape, y * W1 + x)
                    else:
                        better = v > best if layer == L_MAXPOOL else v < best
                        best = np.where(better, v, best); arg = np.where(better, y * W1 + x, arg)
                    R[:, y, x, :] = 0.0
            for y in ys:
                for x in xs: R[:, y, x, :] = np.where(arg == y * W1 + x, dy, R[:, y, x, :])
    return R


@pytest.mark.parametrize("KS", [2, 3])
@pytest.mark.parametrize("layer", [L_AVGPOOL, L_MAXPOOL, L_MINPOOL, L_USAMPLE], ids=["avg", "max", "min", "usample"])
def test_pool_rung(t4k, dev, layer, KS):
    """k_pool<KS> / k_dpool<KS> on a 7 x 5 grid (odd: the last window of each axis is clipped), 3 x 7 x 5 x 5 = 525 elements: three workgroups"""
    N, H1, W1, C = 3, 7, 5, 5
    H0, W0 = (H1 + KS - 1) // KS, (W1 + KS - 1) // KS
    rng = np.random.default_rng(KS * 100 + layer)
    I, DY = ints(rng, N, H1, W1, C), ints(rng, N, H0, W0, C)
    dI, dO = dev.up(I), dev.zeros((N, H0, W0, C))
    t4k.call("t4k_pool", layer, p(dI), p(dO), N, H1, W1, H0, W0, C, KS, None)
    assert same(dev.down(dO), ref_pool(layer, I, KS, H0, W0))
    t4k.call("t4k_dpool", layer, p(dI), p(dev.up(DY)), N, H1, W1, H0, W0, C, KS, None)
    assert same(dev.down(dI), ref_dpool(layer, I, DY, KS))


def test_transposed_conv_rung(t4k, dev):
    """t4k_dconv2d_fwd / _bwd (K 4, S 2, P 1): the forward is the conv dX (k_conv_dx_and_fold, no fold), the backward the conv forward (gather GEMM)
    + k_conv_df_mfma with its fold alone + colsum_add for dB: 2 x 10 x 12 = 240 output pixels, one chunk"""
    torch = dev.torch
    N, H1, W1, C1, C0, K, S, P = 2, 5, 6, 6, 5, 4, 2, 1
    H0, W0 = (H1 - 1) * S - 2 * P + K, (W1 - 1) * S - 2 * P + K
    rng = np.random.default_rng(4)
    I, F, B, G = ints(rng, N, H1, W1, C1), ints(rng, C1, K, K, C0), ints(rng, C0), ints(rng, N, H0, W0, C0)
    DF0, DB0 = ints(rng, C1, K, K, C0), ints(rng, C0)
    w = torch.from_numpy(F.astype(np.float64)).permute(0, 3, 1, 2).contiguous()                 # [in = C1][out = C0][K][K]
    O = torch.nn.functional.conv_transpose2d(_nchw(torch, I), w, torch.from_numpy(B.astype(np.float64)), stride=S, padding=P).permute(0, 2, 3, 1).numpy()
    DX = torch.nn.functional.conv2d(_nchw(torch, G), w, None, stride=S, padding=P).permute(0, 2, 3, 1).numpy()
    DF = torch.nn.grad.conv2d_weight(_nchw(torch, G), (C1, C0, K, K), _nchw(torch, I), stride=S, padding=P).permute(0, 2, 3, 1).numpy() + DF0
    DB = G.astype(np.float64).sum(axis=(0, 1, 2)) + DB0
    dI, dF, dB, dG, dO = dev.up(I), dev.up(F), dev.up(B), dev.up(G), dev.zeros(O.shape)
    t4k.call("t4k_dconv2d_fwd", p(dI), p(dO), p(dF), p(dB), N, H1, W1, C1, H0, W0, C0, K, S, P, None)
    assert same(dev.down(dO), O)
    dDX, dDF, dDB = dev.up(np.full(I.shape, 7.0, np.float32)), dev.up(DF0), dev.up(DB0)
    t4k.call("t4k_dconv2d_bwd", p(dI), p(dG), p(dDX), p(dF), p(dDF), p(dDB), N, H1, W1, C1, H0, W0, C0, K, S, P, 1, None)
    assert same(dev.down(dDX), DX) and same(dev.down(dDF), DF) and same(dev.down(dDB), DB)


@pytest.mark.parametrize("rows", [1000, 3000], ids=["one_chunk", "12_chunks"])
def test_colsum_add_rung(t4k, dev, rows):
    """colsum_add behind the bias gradient of t4k_dconv2d_bwd (rows = output pixels): <= 1024 rows accumulate in place in one launch (k_colsum_part), more go
    through chunk partials and the wave-per-output fold (k_conv_df_fold); 70 columns: two 64-column groups, the second ragged"""
    N, H1, W1, C1, C0, K, S, P = 1, rows // 40, 10, 2, 70, 4, 2, 1                # output 2 H1 x 20 = rows pixels
    H0, W0 = 2 * H1, 2 * W1
    rng = np.random.default_rng(rows)
    I, F, G = ints(rng, N, H1, W1, C1), ints(rng, C1, K, K, C0), ints(rng, N, H0, W0, C0)
    DF0, DB0 = ints(rng, C1, K, K, C0), ints(rng, C0)
    dDF, dDB = dev.up(DF0), dev.up(DB0)
    t4k.call("t4k_dconv2d_bwd", p(dev.up(I)), p(dev.up(G)), None, p(dev.up(F)), p(dDF), p(dDB), N, H1, W1, C1, H0, W0, C0, K, S, P, 1, None)
    assert same(dev.down(dDB), G.astype(np.float64).sum(axis=(0, 1, 2)) + DB0)
