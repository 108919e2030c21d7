"""t4k_conv2d_grp_plan (include/t4k.h, csrc/conv_group.hip): admission and launch plan of the grouped / depthwise convolution, on the
host alone - nothing is launched and no device is needed, so these rows run wherever the library loads.

out = { engine (1 depthwise: Cg1 == 1; 2 general), load path of the forward and of dF (0 dwords; 1 depthwise multiplier 1, 16-byte I; 2 Cg0 % 4 == 0, one
        dword of I per tap; 3 depthwise with another multiplier, four dwords of I per tap), channels of a dX thread (4 | 1), channel lanes of a dF
        workgroup, its pixel sub-slices, dF slices, fold (1 fold_add, 2 df_fold), launches of a backward }.
The expected rows are worked out by hand from the rule of 3.18: a 16-byte path needs the pointers on 16 bytes (`aligned` bit 0) and C0 % 4 == 0; the
channel lanes are the power of two that holds the C0 / 4 (dwords: C0) channel groups, at most 32; the sub-slices are (256 / lanes) / K; the slices are
ceil(1024 / tiles) with tiles = Cg1 ceil(groups / lanes), no more than floor(2^21 / slab floats) (8 MiB) and at least one, over whole 32-pixel stages,
slab = (Cg1 K K + 1) C0 floats; up to 32 slices fold through k_fold_add when DB lies right behind DF (bit 1 says it does not)."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, N, H1, W1, C1, C0, K, S, P, D, G, aligned=1):
    out = I8(*([-7] * 8))
    rc = lib.t4k_conv2d_grp_plan(N, H1, W1, C1, C0, K, S, P, D, G, aligned, out)
    return rc, list(out)


def admitted():
    for K in range(1, 8):
        for S in range(1, 5):
            for D in range(1, 5):
                for P in range(0, D * (K - 1) + 1):
                    yield K, S, P, D


def test_extent_rule_against_torch(lib):
    """every admitted (K, S, P, D) at H1 = 1..20 on a 2-channel depthwise layer: the plan admits exactly the images torch can convolve with groups = 2,
    and the LIBRARY's extents are torch's output shape.  The plan does not return H0 and W0, but its slice count is made of them: one tile wants 1024
    slices of whole 32-pixel stages (a slab is at most 100 floats: nothing else caps them), so an extent off by one changes the count"""
    n = 0
    w = {K: torch.zeros(2, 1, K, K) for K in range(1, 8)}
    for K, S, P, D in admitted():
        for H1 in range(1, 21):
            rc, out = plan(lib, 32, H1, 40, 2, 2, K, S, P, D, 2)             # W1 = 40 holds every window
            fits = H1 + 2 * P - D * (K - 1) - 1 >= 0
            assert rc == (OK if fits else ERR_UNSUPPORTED), (K, S, P, D, H1, rc)
            if fits:
                o = torch.nn.functional.conv2d(torch.zeros(1, 2, H1, 40), w[K], stride=S, padding=P, dilation=D, groups=2)
                assert o.shape[2] == (H1 + 2 * P - D * (K - 1) - 1) // S + 1, (K, S, P, D, H1)
                np0 = 32 * o.shape[2] * o.shape[3]
                pps = -(-(-(-np0 // 1024)) // 32) * 32
                assert out[5] == -(-np0 // pps), (K, S, P, D, H1, out, tuple(o.shape))
                n += 1
            else:
                assert out == [-7] * 8
                with pytest.raises(RuntimeError):
                    torch.nn.functional.conv2d(torch.zeros(1, 2, H1, 40), w[K], stride=S, padding=P, dilation=D, groups=2)
    assert n > 15000


def test_rejections(lib):
    """every rejection with its code; a refusal leaves a text and writes nothing into out"""
    good = dict(N=3, H1=11, W1=9, C1=4, C0=8, K=3, S=2, P=1, D=1, G=4)

    def call(**kw):
        lib.t4k_conv2d_grp_plan(*good.values(), 1, I8())                    # a good call in between: the text below is the refusal's own
        rc, out = plan(lib, **{**good, **kw})
        if rc != OK:
            assert out == [-7] * 8 and lib.t4k_last_error(), kw
        return rc

    assert call() == OK
    assert lib.t4k_conv2d_grp_plan(3, 11, 9, 4, 8, 3, 2, 1, 1, 4, 1, None) == ERR_ARG
    for name in ("N", "H1", "W1", "C1", "C0"):                           # an extent below 1: a bad argument
        assert call(**{name: 0}) == ERR_ARG and call(**{name: -2}) == ERR_ARG, name
        assert b"extent" in lib.t4k_last_error()
    for kw in (dict(K=0), dict(K=8), dict(S=0), dict(S=5), dict(D=0), dict(D=5), dict(P=-1), dict(P=3), dict(K=1, P=1), dict(K=3, D=2, P=5)):
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert b"not supported" in lib.t4k_last_error()
    for kw in (dict(G=0), dict(G=-1), dict(G=3), dict(G=8), dict(G=5), dict(C1=6, C0=8, G=3), dict(C1=8, C0=6, G=4), dict(C1=4, C0=4, G=8)):
        assert call(**kw) == ERR_UNSUPPORTED, kw                         # G below 1, G not dividing C1 (3, 8: above C1), not dividing C0
        assert b"groups=" in lib.t4k_last_error()
    assert call(G=1) == OK and call(G=2) == OK and call(C1=6, C0=9, G=3) == OK
    assert call(K=3, D=2, P=4) == OK and call(K=7, P=6) == OK
    assert call(H1=2, K=7, P=3) == OK                                    # an image smaller than the window, inside its padding: one row
    assert call(H1=2, K=7, P=2) == ERR_UNSUPPORTED                       # 2 + 4 < 7: the window does not fit
    assert call(W1=2, K=5, P=0) == ERR_UNSUPPORTED and b"does not fit" in lib.t4k_last_error()
    assert call(N=1 << 20, H1=64, W1=32, K=1, S=1, P=0) == ERR_UNSUPPORTED             # 2^31 pixels
    assert call(N=(1 << 20) - 1, H1=64, W1=32, K=1, S=1, P=0) == OK
    assert call(N=1 << 20, H1=64, W1=64, K=1, S=2, P=0) == ERR_UNSUPPORTED             # ... on the input side alone
    # the slab limit, (Cg1 K K + 1) C0 floats within 32 MiB = 2^23 floats: 64 groups of 42 -> 64 channels under 7x7 are 2059 * 4096 floats, of 41 are 2010 * 4096
    assert call(C1=2688, C0=4096, K=7, P=3, G=64) == ERR_UNSUPPORTED and b"slab" in lib.t4k_last_error()
    assert call(C1=2624, C0=4096, K=7, P=3, G=64) == OK
    assert call(C1=2688, C0=4096, K=7, P=3, G=128) == OK                 # the same channels in twice the groups: half the slab


ROWS = {
    # (3, 11, 9) under 3x3 / 1, P 1: 297 pixels -> 10 stages of 32; one tile wants 1024 slices, a stage is the least.  8 channels = 2 groups of four: 2 lanes,
    # 128 rows / 3 = 42 sub-slices
    "depthwise_aligned":   ((3, 11, 9, 8, 8, 3, 1, 1, 1, 8, 1), [1, 1, 4, 2, 42, 10, 1, 3]),
    # dwords: 8 channel groups -> 8 lanes, 32 rows / 3 = 10 sub-slices
    "depthwise_unaligned": ((3, 11, 9, 8, 8, 3, 1, 1, 1, 8, 0), [1, 0, 1, 8, 10, 10, 1, 3]),
    "depthwise_db_apart":  ((3, 11, 9, 8, 8, 3, 1, 1, 1, 8, 3), [1, 1, 4, 2, 42, 10, 2, 3]),
    "depthwise_c_6":       ((3, 11, 9, 6, 6, 3, 1, 1, 1, 6, 1), [1, 0, 1, 8, 10, 10, 1, 3]),      # C0 % 4 != 0: dwords whatever the pointers
    # 4 -> 8 channels in 4 groups: a thread's four outputs read two inputs
    "multiplier_2":        ((3, 11, 9, 4, 8, 3, 1, 1, 1, 4, 1), [1, 3, 1, 2, 42, 10, 1, 3]),
    # 4 -> 16 in 4 groups: Cg0 = 4, the four outputs of a thread share their input; 4 lanes, 64 rows / 3 = 21
    "multiplier_4":        ((3, 11, 9, 4, 16, 3, 1, 1, 1, 4, 1), [1, 2, 1, 4, 21, 10, 1, 3]),
    # 12 -> 20 in 4 groups under 3x3 / 2: Cg1 = 3, Cg0 = 5 - a thread's four channels would straddle groups: dwords, 20 -> 32 lanes, 8 rows / 3 = 2;
    # 6 x 5 outputs, 90 pixels -> 3 stages; 3 tiles want 342 slices
    "general_cg1_3":       ((3, 11, 9, 12, 20, 3, 2, 1, 1, 4, 1), [2, 0, 1, 32, 2, 3, 1, 3]),
    "general_cg_4":        ((3, 11, 9, 8, 8, 3, 2, 1, 1, 2, 1), [2, 2, 1, 2, 42, 3, 1, 3]),
    "dense_g_1":           ((3, 11, 9, 4, 8, 3, 2, 1, 1, 1, 1), [2, 2, 1, 2, 42, 3, 1, 3]),      # G = 1 is admitted: Cg0 = 8
    "dense_1_to_1":        ((3, 11, 9, 1, 1, 3, 1, 1, 1, 1, 1), [1, 0, 1, 1, 85, 10, 1, 3]),
    # slice counts on both sides of 32: (11, 11, 9) is 1089 pixels, ceil(1089 / 1024) = 2 -> a stage per slice -> 35
    "slices_32":           ((1, 32, 32, 8, 8, 3, 1, 1, 1, 8, 1), [1, 1, 4, 2, 42, 32, 1, 3]),
    "slices_35":           ((11, 11, 9, 8, 8, 3, 1, 1, 1, 8, 1), [1, 1, 4, 2, 42, 35, 2, 3]),
    # 256 x 32 x 32 x 64 depthwise: 16 lanes, 16 rows / 3 = 5; one tile wants 1024 slices of 256 pixels
    "mobilenet_block":     ((256, 32, 32, 64, 64, 3, 1, 1, 1, 64, 1), [1, 1, 4, 16, 5, 1024, 2, 3]),
    # 128 -> 128 in 2 groups: 32 lanes, one channel tile, 64 tiles (one per cg) want 16 slices; 2^21 / (577 * 128) = 28 fit
    "fat_groups":          ((256, 16, 16, 128, 128, 3, 1, 1, 1, 2, 1), [2, 2, 1, 32, 2, 16, 1, 3]),
    # the workspace cap: a slab of 2010 * 4096 floats (31.4 MiB) does not fit 8 MiB even once - one slice whatever the pixels; 1024 groups of four -> 32 tiles
    "slab_limit":          ((1, 8, 8, 2624, 4096, 7, 1, 3, 1, 64, 1), [2, 2, 1, 32, 1, 1, 1, 3]),
    # ... and 2^21 / (50 * 4096) = 10 slices where 1024 / 32 = 32 were wanted: ceil(4096 / 10) = 410 -> 416 pixels -> 10
    "cap_shrinks":         ((4, 32, 32, 4096, 4096, 7, 1, 3, 1, 4096, 1), [1, 1, 4, 32, 1, 10, 1, 3]),
}


@pytest.mark.parametrize("row", list(ROWS))
def test_plan_rows(lib, row):
    args, want = ROWS[row]
    rc, got = plan(lib, *args)
    assert rc == OK and got == want, (lib.t4k_last_error(), got)
