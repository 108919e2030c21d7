"""t4k_patch_plan (include/t4k.h, csrc/patch.hip): admission and launch plan of the patch embedding, on the host alone - nothing is
launched and no device is needed.

out = { forward channel tile, forward load path (bit 0: 16-byte gather of I, bit 1: 16-byte loads of F), dX column tile, dX 16-byte path,
        dF load path (bit 0: 16-byte gather of I, bit 1: 16-byte loads of dO), dF slices, fold (1 fold_add, 2 df_fold), launches of a backward };
aligned: bit 0 I, bit 1 F, bit 2 dO on 16 bytes, bit 3: DB not right behind DF.
The expected rows are worked out by hand from the rule of 3.25: the gather of I takes 16 bytes when K C1 and W1 C1 are multiples of 4 and I is aligned; F and
dO when C0 is a multiple of 4 and they are; the 128-wide tiles need the 16-byte paths and more than 64 columns (C0 forward, K K C1 for dX); the slices are
min(ceil(1024 / tiles), floor(2^21 / slab floats)), at least one, with tiles = ceil((K K C1 + 1) / 64) ceil(C0 / 64), over whole 32-token stages; up to 32
slices fold through k_fold_add when DB lies right behind DF."""
import ctypes

import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, N, H1, W1, C1, C0, K, aligned=7):
    out = I8(*([-7] * 8))
    rc = lib.t4k_patch_plan(N, H1, W1, C1, C0, K, aligned, out)
    return rc, list(out)


ROWS = {
    # ViT-B/16: 25088 tokens; 13 x 12 tiles want 7 slices, 2^21 / (769 * 768) = 3 fit; ceil(25088 / 3) = 8363 -> 8384 tokens a slice -> 3
    "vit_b16":          ((128, 224, 224, 3, 768, 16, 7), [128, 3, 128, 1, 3, 3, 1, 3]),
    # 16 x 3 = 48 floats a run, 48 x 3 = 144 a row: I on 16 bytes; C0 = 64 is no more than a tile, K K C1 = 768 is
    "k16_c0_64":        ((2, 35, 48, 3, 64, 16, 7), [64, 3, 128, 1, 3, 1, 1, 3]),
    "k16_c0_66":        ((2, 35, 48, 3, 66, 16, 7), [64, 1, 64, 0, 1, 1, 1, 3]),      # C0 off 4: F and dO by dwords, the gather of I stays
    "k14_c0_64":        ((2, 31, 42, 3, 64, 14, 7), [64, 2, 128, 1, 2, 1, 1, 3]),     # 14 x 3 = 42 floats a run: I by dwords, F and dO stay
    "k14_c0_66":        ((2, 31, 42, 3, 66, 14, 7), [64, 0, 64, 0, 0, 1, 1, 3]),
    "k16_row_100":      ((2, 35, 50, 2, 64, 16, 7), [64, 3, 128, 1, 3, 1, 1, 3]),     # runs of 32 floats in rows of 100: both multiples of 4
    "k16_row_98":       ((2, 35, 49, 2, 64, 16, 7), [64, 2, 128, 1, 2, 1, 1, 3]),     # rows of 98 floats: the second row of an image is off 16 bytes
    "unaligned":        ((2, 35, 48, 3, 64, 16, 0), [64, 0, 64, 0, 0, 1, 1, 3]),
    "only_i":           ((2, 35, 48, 3, 64, 16, 1), [64, 1, 64, 0, 1, 1, 1, 3]),
    "only_f":           ((2, 35, 48, 3, 64, 16, 2), [64, 2, 64, 0, 0, 1, 1, 3]),      # dX needs dO and F
    "i_and_do":         ((2, 35, 48, 3, 64, 16, 5), [64, 1, 64, 0, 3, 1, 1, 3]),
    "db_apart":         ((2, 35, 48, 3, 64, 16, 15), [64, 3, 128, 1, 3, 1, 2, 3]),    # one slice, but k_fold_add has one destination
    "wide_c0":          ((2, 35, 48, 3, 68, 16, 7), [128, 3, 128, 1, 3, 1, 1, 3]),
    # 8 x 8 x 1: K K C1 = 64 columns, no more than a tile; 65 rows are 2 tiles: 512 slices wanted, a stage each: 75 tokens -> 3
    "slices_3":         ((3, 40, 40, 1, 4, 8, 7), [64, 3, 64, 1, 3, 3, 1, 3]),
    "slices_32":        ((16, 64, 64, 1, 4, 8, 7), [64, 3, 64, 1, 3, 32, 1, 3]),
    "slices_34":        ((17, 64, 64, 1, 4, 8, 7), [64, 3, 64, 1, 3, 34, 2, 3]),
    # the slab cap: 1025 x 2048 floats fit 2^21 floats 0 times - one slice whatever the tokens
    "cap_one_slice":    ((64, 64, 64, 1, 2048, 32, 7), [128, 3, 128, 1, 3, 1, 1, 3]),
    "k4_stem":          ((2, 16, 16, 3, 8, 4, 7), [64, 3, 64, 1, 3, 1, 1, 3]),        # ConvNeXt's 4 / 4 / 0: 48 columns, no more than a tile
}


@pytest.mark.parametrize("row", list(ROWS))
def test_plan_rows(lib, row):
    args, want = ROWS[row]
    rc, got = plan(lib, *args)
    assert rc == OK and got == want, (lib.t4k_last_error(), got)


def test_rejections(lib):
    good = dict(N=3, H1=19, W1=24, C1=3, C0=8, K=8)
    def call(code=None, text=None, **kw):
        rc, out = plan(lib, **{**good, **kw})
        if rc != OK:
            assert out == [-7] * 8, (kw, out)                                # a refusal leaves out as it was
            assert text in lib.t4k_last_error(), (kw, lib.t4k_last_error())
        return rc
    assert call() == OK
    assert lib.t4k_patch_plan(3, 19, 24, 3, 8, 8, 7, None) == ERR_ARG
    for name in ("N", "H1", "W1", "C1", "C0"):
        assert call(text=b"extent", **{name: 0}) == ERR_ARG and call(text=b"extent", **{name: -2}) == ERR_ARG, name
    for K in (-1, 0, 1, 33):
        assert call(text=b"not supported", K=K) == ERR_UNSUPPORTED, K
    assert call(K=2) == OK and call(K=32, H1=32, W1=32) == OK
    assert call(text=b"does not fit", H1=7) == ERR_UNSUPPORTED and call(text=b"does not fit", W1=7) == ERR_UNSUPPORTED
    assert call(H1=8, W1=8) == OK
    # 2^31 elements: the image, then the token tensor
    assert call(text=b"2^31", N=1 << 17, H1=128, W1=128, C1=1, C0=1) == ERR_UNSUPPORTED
    assert call(N=(1 << 17) - 1, H1=128, W1=128, C1=1, C0=1) == OK
    assert call(text=b"2^31", N=1 << 16, H1=16, W1=16, C1=1, C0=512, K=2) == ERR_UNSUPPORTED
    assert call(N=1 << 16, H1=16, W1=16, C1=1, C0=511, K=2) == OK
    assert call(text=b"2^31", N=0x7fffffff, H1=0x7fffffff, W1=0x7fffffff, C1=0x7fffffff, C0=0x7fffffff) == ERR_UNSUPPORTED
    # one slab within 32 MiB: (32 * 32 * 64 + 1) * 128 floats are 128 too many
    assert call(text=b"slab", H1=32, W1=32, C1=64, C0=128, K=32) == ERR_UNSUPPORTED
    assert call(H1=32, W1=32, C1=64, C0=127, K=32) == OK
