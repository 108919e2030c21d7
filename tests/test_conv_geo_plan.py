"""t4k_conv2d_geo_plan (include/t4k.h, csrc/conv_geo.hip): admission and launch plan of the run-time-geometry convolution, on
the host alone - nothing is launched and no device is needed, so these rows run wherever the library loads.

out = { forward channel tile, forward load path (bit 0: 16-byte gather of I, bit 1: 16-byte loads of F), dX channel tile, dX 16-byte path,
        dF path (bit 0: 16-byte dO, bit 1: tap-per-tile rows with a 16-byte gather of I), dF slices, fold (1 fold_add, 2 df_fold), launches of a backward }.
The expected rows are worked out by hand from the rule of 3.15: a 16-byte path needs the pointers on 16 bytes and the contiguous channel
count a multiple of 4 (C1 for the gather of I, C0 for F, for dO and for the dX operands); the 128-wide channel tile needs the 16-byte paths
and more than 64 produced channels; from 32 input channels (a multiple of 4) on the 16-byte paths a dF tile's rows are the channels of one tap;
the slices are ceil(1024 / tiles) with tiles = ceil((C1 K K + 1) / 64) ceil(C0 / 64) - (K K ceil(C1 / 64) + 1) ceil(C0 / 64) tap-per-tile -, no more than
floor(2^21 / slab floats) (8 MiB) and at least one, over whole 32-pixel stages; up to 32 slices fold through k_fold_add when DB lies right behind DF
(the `aligned` argument's bit 1 says it does not)."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, N, H1, W1, C1, C0, K, S, P, D, aligned=1):
    out = I8()
    rc = lib.t4k_conv2d_geo_plan(N, H1, W1, C1, C0, K, S, P, D, aligned, out)
    return rc, list(out)


def admitted():
    for K in range(1, 8):
        for S in range(1, 5):
            for D in range(1, 5):
                for P in range(0, D * (K - 1) + 1):
                    yield K, S, P, D


def test_extent_rule_against_torch(lib):
    """every admitted (K, S, P, D) at H1 = 1..20: the plan admits exactly the images torch can convolve, and the LIBRARY's extents are torch's output
    shape.  The plan does not return H0 and W0, but its slice count is made of them: one channel in and out is one dF tile, which wants 1024
    slices of whole 32-pixel stages, so a batch of 32 gives H0 W0 slices up to 1024 pixels an image and ceil(32 H0 W0 / pps) above, pps = ceil(H0 W0 / 32)
    stages (at most 50 floats a slab: nothing else caps them) - an extent off by one changes the count"""
    n = 0
    w = {K: torch.zeros(1, 1, K, K) for K in range(1, 8)}
    for K, S, P, D in admitted():
        for H1 in range(1, 21):
            rc, out = plan(lib, 32, H1, 40, 1, 1, K, S, P, D)                # W1 = 40 holds every window
            fits = H1 + 2 * P - D * (K - 1) - 1 >= 0
            assert rc == (OK if fits else ERR_UNSUPPORTED), (K, S, P, D, H1, rc)
            if fits:
                o = torch.nn.functional.conv2d(torch.zeros(1, 1, H1, 40), w[K], stride=S, padding=P, dilation=D)
                assert o.shape[2] == (H1 + 2 * P - D * (K - 1) - 1) // S + 1, (K, S, P, D, H1)
                np0 = 32 * o.shape[2] * o.shape[3]                           # the slice rule on TORCH's extents: up to 1024 slices of whole stages
                pps = -(-(-(-np0 // 1024)) // 32) * 32
                assert out[5] == -(-np0 // pps), (K, S, P, D, H1, out, tuple(o.shape))
                n += 1
            else:
                with pytest.raises(RuntimeError):
                    torch.nn.functional.conv2d(torch.zeros(1, 1, H1, 40), w[K], stride=S, padding=P, dilation=D)
    assert n > 15000


def test_rejections(lib):
    good = dict(N=3, H1=11, W1=9, C1=4, C0=8, K=3, S=2, P=1, D=1)
    call = lambda **kw: plan(lib, **{**good, **kw})[0]
    assert call() == OK
    assert lib.t4k_conv2d_geo_plan(3, 11, 9, 4, 8, 3, 2, 1, 1, 1, None) == ERR_ARG
    for name in ("N", "H1", "W1", "C1", "C0"):                           # an extent below 1: a bad argument
        assert call(**{name: 0}) == ERR_ARG and call(**{name: -2}) == ERR_ARG, name
        assert b"extent" in lib.t4k_last_error()
    for kw in (dict(K=0), dict(K=8), dict(S=0), dict(S=5), dict(D=0), dict(D=5), dict(P=-1), dict(P=3), dict(K=1, P=1),
               dict(K=3, D=2, P=5)):                                     # outside K 1..7, S 1..4, D 1..4, 0 <= P <= D(K-1): an inadmissible geometry
        assert call(**kw) == ERR_UNSUPPORTED, kw
        assert b"not supported" in lib.t4k_last_error()
    assert call(K=3, D=2, P=4) == OK and call(K=7, P=6) == OK
    assert call(H1=2, K=7, P=3) == OK                                    # an image smaller than the window, inside its padding: one row
    assert call(H1=2, K=7, P=2) == ERR_UNSUPPORTED                       # 2 + 4 < 7: the window does not fit
    assert call(W1=2, K=5, P=0) == ERR_UNSUPPORTED and b"does not fit" in lib.t4k_last_error()
    assert call(N=1 << 20, H1=64, W1=32, K=1, S=1, P=0) == ERR_UNSUPPORTED             # 2^31 pixels
    assert call(N=(1 << 20) - 1, H1=64, W1=32, K=1, S=1, P=0) == OK
    assert call(N=1 << 20, H1=64, W1=64, K=1, S=2, P=0) == ERR_UNSUPPORTED             # ... on the input side alone
    assert call(C1=512, C0=512, K=7, P=3) == ERR_UNSUPPORTED and b"slab" in lib.t4k_last_error()   # 25089 * 512 floats > 32 MiB
    assert call(C1=64, C0=512, K=7, P=3) == OK


ROWS = {
    # (3, 11, 9) under 3x3 / 2, P 1: 6 x 5 outputs, 90 pixels -> 3 stages of 32; one 64 x 64 tile wants 1024 slices, a stage is the least
    "vec_all":            ((3, 11, 9, 4, 8, 3, 2, 1, 1, 1), [64, 3, 64, 1, 1, 3, 1, 3]),
    "unaligned_pointers": ((3, 11, 9, 4, 8, 3, 2, 1, 1, 0), [64, 0, 64, 0, 0, 3, 1, 3]),
    "c1_3_c0_5":          ((3, 11, 9, 3, 5, 3, 2, 1, 1, 1), [64, 0, 64, 0, 0, 3, 1, 3]),
    "c1_4_c0_5":          ((3, 11, 9, 4, 5, 3, 2, 1, 1, 1), [64, 1, 64, 0, 0, 3, 1, 3]),     # the gather of I alone takes 16 bytes
    "c1_3_c0_8":          ((3, 11, 9, 3, 8, 3, 2, 1, 1, 1), [64, 2, 64, 1, 1, 3, 1, 3]),     # F, dO and the dX operands do, the gather of I does not
    # 32x32x64 -> 16x16x128, N = 256: 65536 pixels; tiles = ceil(577 / 64) * 2 = 20 -> 52 slices wanted, 2^21 / (577 * 128) = 28 fit;
    # ceil(65536 / 28) = 2341 -> 2368 pixels a slice -> 28 slices
    "resnet_down":        ((256, 32, 32, 64, 128, 3, 2, 1, 1, 1), [128, 3, 64, 1, 3, 28, 1, 3]),
    # 16x16x128 dilated 3x3: tiles = 19 * 2 -> 27 wanted, 2^21 / (1153 * 128) = 14 fit; ceil(65536 / 14) = 4682 -> 4704 -> 14 slices
    "dilated_128":        ((256, 16, 16, 128, 128, 3, 1, 2, 2, 1), [128, 3, 128, 1, 3, 14, 1, 3]),
    # slice counts on both sides of 32: one tile, a stage per slice
    "slices_10":          ((3, 11, 9, 1, 1, 3, 1, 1, 1, 1), [64, 0, 64, 0, 0, 10, 1, 3]),
    # DB somewhere else than right behind DF (aligned bit 1): k_fold_add has one destination, so the wave-per-output fold takes the ten slices
    "slices_10_db_apart": ((3, 11, 9, 1, 1, 3, 1, 1, 1, 3), [64, 0, 64, 0, 0, 10, 2, 3]),
    "vec_all_db_apart":   ((3, 11, 9, 4, 8, 3, 2, 1, 1, 3), [64, 3, 64, 1, 1, 3, 2, 3]),
    "unaligned_db_apart": ((3, 11, 9, 4, 8, 3, 2, 1, 1, 2), [64, 0, 64, 0, 0, 3, 2, 3]),
    "slices_32":          ((1, 32, 32, 1, 1, 3, 1, 1, 1, 1), [64, 0, 64, 0, 0, 32, 1, 3]),
    "slices_33":          ((1, 33, 32, 1, 1, 3, 1, 1, 1, 1), [64, 0, 64, 0, 0, 33, 2, 3]),
    "slices_35":          ((11, 11, 9, 1, 1, 3, 1, 1, 1, 1), [64, 0, 64, 0, 0, 35, 2, 3]),
    # 7x7 on 33 -> 31 channels: 26 tiles want 40 slices, 41 fit; ceil(297 / 40) = 8 -> one stage a slice -> 10
    "k7_ragged":          ((3, 11, 9, 33, 31, 7, 1, 3, 1, 1), [64, 0, 64, 0, 0, 10, 1, 3]),
    # the workspace cap: a slab of 3137 * 512 floats (6.1 MiB) fits 8 MiB once - one slice whatever the pixels
    "cap_one_slice":      ((8, 32, 32, 64, 512, 7, 2, 3, 1, 1), [128, 3, 64, 1, 3, 1, 1, 3]),
    # ... and 2^21 / (217 * 256) = 37 slices where 1024 / (4 * 4) = 64 were wanted: ceil(16384 / 37) = 443 -> 448 -> 37
    "cap_shrinks":        ((64, 16, 16, 24, 256, 3, 1, 1, 1, 1), [128, 3, 64, 1, 1, 37, 2, 3]),
    # from 32 input channels a dF tile is one tap: (9 + 1) * 4 tiles want 26 slices, 28 fit; ceil(16384 / 26) = 631 -> 640 -> 26
    "df_tap_tiles":       ((64, 16, 16, 32, 256, 3, 1, 1, 1, 1), [128, 3, 64, 1, 3, 26, 1, 3]),
    "df_tap_unaligned":   ((64, 16, 16, 32, 256, 3, 1, 1, 1, 0), [64, 0, 64, 0, 0, 27, 1, 3]),
}


@pytest.mark.parametrize("row", list(ROWS))
def test_plan_rows(lib, row):
    args, want = ROWS[row]
    rc, got = plan(lib, *args)
    assert rc == OK and got == want, (lib.t4k_last_error(), got)
