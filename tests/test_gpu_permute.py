"""t4k_permute / t4k_permute_plan (include/t4k.h, csrc/permute.hip) through the C ABI.

Operands are random 32-bit patterns viewed as float32 (NaN payloads, denormals and infinities among them) and results are compared as
uint32 against numpy.transpose: pure data movement, nothing to tolerate.  Every case also checks that src is intact, that the guard
floats in front of and behind dst (Dev of tests/test_gpu_bcast.py, 4 floats in front here) are untouched, and that the call was exactly
one launch.  The family, the float4 path, the tile sides and the work items a case means to reach are asserted through t4k_permute_plan.

A run family with ONE outer digit does not exist: two groups of which the second is the source's innermost would have merged into a
copy.  The run cases therefore use 0 (the copy), 2 and 3 outer digits."""
import ctypes
import itertools
import zlib

import numpy as np
import pytest

from test_gpu_bcast import Dev, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
COPY, RUNS, TILES = 0, 1, 2
I4 = ctypes.c_int * 4
I7 = ctypes.c_int * 7
ORDERS = list(itertools.permutations(range(4)))
WEIGHT = (8, 4, 2, 1)
FRONT = 4                                                               # guard floats in front of a buffer: 16 bytes, the alignment stays
SENTINEL = np.uint32(0x7FC0DEAD)


def word(perm):
    return "%d%d%d%d" % tuple(WEIGHT[a] for a in perm)


def plan(h, dim, perm, aligned=1):
    out = I7()
    assert h.lib.t4k_permute_plan(I4(*dim), I4(*perm), aligned, out) == OK, h.lib.t4k_last_error()
    return list(out)


def pow2_ceil(v):
    p = 1
    while p < v:
        p *= 2
    return p


def tile_rule(ea, eb, ez=1):
    """each side the smallest power of two >= min(extent, 64); the side with room grows until the tile holds 4096 floats;
    what two narrow sides leave goes to entries of the inner batch group"""
    ta, tb, tz = pow2_ceil(min(ea, 64)), pow2_ceil(min(eb, 64)), 1
    while ta * tb < 4096 and ta < ea:
        ta *= 2
    while ta * tb < 4096 and tb < eb:
        tb *= 2
    while ta * tb * tz < 4096 and tz < ez:
        tz *= 2
    return ta, tb, tz


def bits(shape, tag=""):
    rng = np.random.default_rng(zlib.crc32(repr((tuple(shape), tag)).encode()))
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32)


def run_case(h, dim, perm, offs=(FRONT, FRONT)):
    dim, perm = tuple(int(d) for d in dim), tuple(int(p) for p in perm)
    a = bits(dim, perm)
    n = a.size
    out_shape = tuple(dim[p] for p in perm)
    dS = Dev(a.view(np.float32), offs[0])
    dD = Dev(np.full(n, SENTINEL, np.uint32).view(np.float32), offs[1])
    l0 = lcount(h)
    h.call("t4k_permute", dS.p, dD.p, I4(*dim), I4(*perm), None)
    assert lcount(h) - l0 == 1, (dim, perm)
    got = dD.get(h, out_shape).view(np.uint32)
    want = np.ascontiguousarray(a.transpose(perm))
    assert np.array_equal(got, want), (dim, perm, int(np.sum(got != want)))
    assert np.array_equal(dS.get(h, dim).view(np.uint32), a)            # src is intact
    whole = dD.t.cpu().numpy()
    assert not whole[:dD.off].any() and not whole[dD.off + n:].any()     # nothing written in front of or behind dst
    return plan(h, dim, perm, int(offs[0] % 4 == 0 and offs[1] % 4 == 0))


# ---------------------------------------------------------------- every order
@pytest.mark.parametrize("dim", [(3, 5, 7, 2), (2, 1, 66, 5), (1, 1, 1, 1)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("perm", ORDERS, ids=[word(p) for p in ORDERS])
def test_every_order_on_odd_shapes(t4k, dim, perm):
    p = run_case(t4k, dim, perm)
    if dim == (1, 1, 1, 1):
        assert p[0] == COPY and p[5] == 1
    if dim == (2, 1, 66, 5):                                            # the extent-1 axis drops out wherever the order puts it: at most three groups
        assert p[5] <= 3, (perm, p)


def test_all_three_families(t4k):
    assert run_case(t4k, (3, 5, 7, 2), (0, 1, 2, 3))[0] == COPY         # 8421
    assert run_case(t4k, (2, 1, 66, 5), (1, 0, 2, 3))[0] == COPY        # only an axis of extent 1 moves
    assert run_case(t4k, (2, 1, 66, 5), (0, 2, 3, 1))[0] == COPY
    assert run_case(t4k, (3, 5, 7, 2), (0, 2, 1, 3))[0] == RUNS         # 8241 with C > 1
    assert run_case(t4k, (3, 5, 7, 2), (1, 0, 2, 3))[0] == RUNS         # C stays last
    assert run_case(t4k, (3, 5, 7, 1), (0, 2, 1, 3))[0] == TILES        # 8241 with C = 1
    assert run_case(t4k, (3, 5, 7, 2), (0, 3, 1, 2))[0] == TILES        # 8142
    assert run_case(t4k, (3, 5, 7, 2), (3, 2, 1, 0))[0] == TILES        # 1248


# ---------------------------------------------------------------- tiles
EDGES = [1, 3, 4, 5, 63, 64, 65, 130]
BATCHES = {"n1": ("one", 1, 1), "n2": ("one", 2, 1), "n7": ("one", 7, 1), "n2w7": ("both", 2, 7), "n7w2": ("both", 7, 2)}


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("ea", EDGES)
def test_tile_family_wide_sides(t4k, ea, batch):
    """ea: the extent of the source's innermost group, eb (every edge): that of the output's; one outer group (8241 on C = 1: N) or two
    (8124 read backwards, the output (N,C,W,H): N and W)"""
    kind, n, w = BATCHES[batch]
    for eb in EDGES:
        if kind == "one":
            p = run_case(t4k, (n, eb, ea, 1), (0, 2, 1, 3))
        else:
            p = run_case(t4k, (n, eb, w, ea), (0, 3, 2, 1))
        if ea > 1 and eb > 1:
            outer, ez = (1, n) if kind == "one" else (n, w)
            assert p[0] == TILES and p[1] == 0, p
            assert (p[2], p[3], p[6]) == tile_rule(ea, eb, ez) and p[2] * p[3] * p[6] <= 4096, p
            assert p[4] == outer * -(-ez // p[6]) * -(-ea // p[2]) * -(-eb // p[3]), p


@pytest.mark.parametrize("hw", [(9, 7), (33, 65)], ids=["9x7", "33x65"])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 16, 17, 64, 65])
def test_tile_family_narrow_side_channel_first(t4k, C, hw):
    """NHWC -> channel-first (8142) and back (8214, the extents (N,C,H,W) stored in the slots).  A fixed 64 x 65 tile would report 64
    along C: the side along the narrow extent is at most the next power of two above it, the other side takes the room"""
    H, W = hw
    p = run_case(t4k, (2, H, W, C), (0, 3, 1, 2))
    q = run_case(t4k, (2, C, H, W), (0, 2, 3, 1))
    if C == 1:
        assert p[0] == COPY and q[0] == COPY
        return
    assert p[0] == TILES and q[0] == TILES and p[5] == 3 and q[5] == 3    # H and W merged
    side = pow2_ceil(min(C, 64))
    assert p[2] == side and q[3] == side, (p, q)
    other = min(pow2_ceil(H * W), 4096 // side)
    assert p[3] == other and q[2] == other, (p, q)
    assert p[6] == q[6] == min(2, 4096 // (side * other)), (p, q)        # the two entries of N where the plane leaves room


@pytest.mark.parametrize("heads", [4, 16])
@pytest.mark.parametrize("D", [8, 64])
def test_tile_family_narrow_side_heads(t4k, heads, D):
    """[N,L,heads,D] <-> [N,L,D,heads] (8412): N and L merge into one batch digit"""
    tz = min(16, 4096 // (heads * D))                                    # 15 entries of (N,L): 16 of them where the tile has room
    p = run_case(t4k, (3, 5, heads, D), (0, 1, 3, 2))
    assert p[0] == TILES and p[5] == 3 and p[2] == D and p[3] == heads and p[6] == tz and p[4] == -(-15 // tz), p
    q = run_case(t4k, (3, 5, D, heads), (0, 1, 3, 2))
    assert q[0] == TILES and q[2] == heads and q[3] == D and q[6] == tz and q[4] == -(-15 // tz), q


def test_no_merge(t4k):
    """all four groups distinct: the tile family with two batch digits, the run family with three run digits - both divisions of each"""
    p = run_case(t4k, (3, 4, 5, 6), (3, 2, 1, 0))                       # 1248
    assert p[0] == TILES and p[5] == 4, p
    p = run_case(t4k, (3, 4, 5, 6), (2, 1, 0, 3))                       # 2481
    assert p[0] == RUNS and p[5] == 4, p


# ---------------------------------------------------------------- runs
@pytest.mark.parametrize("L", [1, 3, 4, 5, 64, 1028])
@pytest.mark.parametrize("dim3", [(1, 1, 7), (1, 5, 7), (3, 5, 7)], ids=["0digits", "2digits", "3digits"])
def test_run_family(t4k, L, dim3):
    """8241 on (N,H,W,L): runs of L floats; 1028 = 257 float4s, one more than 256 lanes take in one pass, and 1028 > 256 floats on the
    scalar path.  L = 1 leaves no run: the shape goes to the tiles (or is a copy) and is checked all the same"""
    dim = dim3 + (L,)
    perm = (0, 2, 1, 3)
    p = run_case(t4k, dim, perm)
    digits = sum(1 for d in dim3 if d > 1)
    if digits <= 1:
        assert p[0] == COPY, p
    elif L == 1:
        assert p[0] == TILES, p
    else:
        assert p[0] == RUNS and p[5] == digits + 1, p
        assert p[1] == (1 if L % 4 == 0 else 0), p
        assert plan(t4k, dim, perm, 0)[1] == 0
    if L > 1:
        for offs in ((FRONT + 1, FRONT), (FRONT, FRONT + 1)):           # either pointer 4 bytes off 16: the scalar path
            q = run_case(t4k, dim, perm, offs=offs)
            assert q[1] == 0 and q[0] == p[0], q
        if L == 1028 and digits > 1:                                    # 257 float4s = 2 chunks of 256 lanes, 1028 floats = 5
            R = dim3[0] * dim3[1] * dim3[2]
            assert p[2] == 256 and p[3] == 1 and p[4] == 2 * R, p
            assert q[2] == 256 and q[3] == 1 and q[4] == 5 * R, q


def test_copy_family_paths(t4k):
    """the flat copy: float4 when the count and the pointers allow, scalar otherwise, a count below one lane group"""
    assert run_case(t4k, (3, 5, 7, 8), (0, 1, 2, 3))[:2] == [COPY, 1]
    assert run_case(t4k, (3, 5, 7, 8), (0, 1, 2, 3), offs=(FRONT + 1, FRONT))[:2] == [COPY, 0]
    assert run_case(t4k, (3, 5, 7, 8), (0, 1, 2, 3), offs=(FRONT, FRONT + 3))[:2] == [COPY, 0]
    assert run_case(t4k, (3, 5, 7, 3), (0, 1, 2, 3))[:2] == [COPY, 0]
    assert run_case(t4k, (1, 1, 1, 3), (3, 2, 1, 0))[:2] == [COPY, 0]


# ---------------------------------------------------------------- the stride loop wraps
def test_grid_cap_runs(t4k):
    """70 000 runs of 3 (64 runs to a pass: 1 094 passes, below the cap of 2 048 workgroups) and 140 000, whose 2 188 passes wrap; 9 runs
    of 60 001 floats and of 240 000, whose 235 chunks each wrap on the scalar and on the float4 path"""
    p = run_case(t4k, (350, 200, 1, 3), (1, 0, 2, 3))
    assert p[0] == RUNS and p[2] == 4 and p[3] == 64 and p[4] == 1094, p
    p = run_case(t4k, (350, 400, 1, 3), (1, 0, 2, 3))
    assert p[0] == RUNS and p[4] == 2188, p
    p = run_case(t4k, (3, 3, 1, 60001), (1, 0, 2, 3))
    assert p[0] == RUNS and p[1] == 0 and p[4] == 9 * 235, p
    p = run_case(t4k, (3, 3, 1, 240000), (1, 0, 2, 3))
    assert p[0] == RUNS and p[1] == 1 and p[4] == 9 * 235, p


def test_grid_cap_tiles(t4k):
    """more tiles than the cap of 2 048 workgroups: a 128 x 32 tile per entry of 2 100, a 64 x 32 tile per two entries of 4 100 (the
    entry index split off the work item), then 2 x 2 tiles of 64 x 64 per entry; 2 100 small entries, 128 to a tile, for the ragged last
    tile of entries"""
    p = run_case(t4k, (2100, 17, 65, 1), (0, 2, 1, 3))
    assert p[0] == TILES and p[2:4] == [128, 32] and p[6] == 1 and p[4] == 2100, p
    p = run_case(t4k, (4100, 17, 33, 1), (0, 2, 1, 3))
    assert p[0] == TILES and p[2:4] == [64, 32] and p[6] == 2 and p[4] == 2050, p
    p = run_case(t4k, (2100, 3, 5, 1), (0, 2, 1, 3))
    assert p[0] == TILES and p[2:4] == [8, 4] and p[6] == 128 and p[4] == 17, p
    p = run_case(t4k, (520, 65, 65, 1), (0, 2, 1, 3))
    assert p[0] == TILES and p[2] == 64 and p[3] == 64 and p[4] == 2080, p


# ---------------------------------------------------------------- against the existing entry
@pytest.mark.parametrize("C", [1, 3])
def test_8241_equals_transpose_batched(t4k, C):
    a = bits((5, 70, 33, C), "xb")
    dS = Dev(a.view(np.float32))
    dP, dT = Dev(np.zeros(a.size, np.float32)), Dev(np.zeros(a.size, np.float32))
    t4k.call("t4k_permute", dS.p, dP.p, I4(5, 70, 33, C), I4(0, 2, 1, 3), None)
    t4k.call("t4k_transpose_batched", dS.p, dT.p, 70, 33, C, 5, None)
    shape = (5, 33, 70, C)
    assert np.array_equal(dP.get(t4k, shape).view(np.uint32), dT.get(t4k, shape).view(np.uint32))
    assert np.array_equal(dP.get(t4k, shape).view(np.uint32), a.transpose(0, 2, 1, 3))


# ---------------------------------------------------------------- error returns
def test_error_returns_launch_nothing(t4k):
    a = np.arange(64, dtype=np.float32)
    d, e = Dev(a), Dev(np.ones(64, np.float32))
    f, g = t4k.lib.t4k_permute, t4k.lib.t4k_permute_plan
    dim, perm, out = I4(2, 2, 4, 4), I4(0, 2, 1, 3), I7()
    l0 = lcount(t4k)
    assert f(None, e.p, dim, perm, None) == ERR_ARG
    assert f(d.p, None, dim, perm, None) == ERR_ARG
    assert f(d.p, e.p, None, perm, None) == ERR_ARG
    assert f(d.p, e.p, dim, None, None) == ERR_ARG
    for bad in ((0, 2, 4, 4), (2, 0, 4, 4), (2, 2, 4, 0), (2, 2, -4, 4)):  # an extent < 1
        assert f(d.p, e.p, I4(*bad), perm, None) == ERR_ARG
        assert g(I4(*bad), perm, 1, out) == ERR_ARG
    assert f(d.p, e.p, I4(1 << 11, 1 << 10, 1 << 10, 1 << 10), perm, None) == ERR_ARG     # 2^41 elements
    for bad in ((0, 1, 1, 3), (0, 0, 0, 0), (0, 1, 2, 4), (-1, 1, 2, 3), (1, 2, 3, 4)):   # a repeated axis, an axis 4, a negative one
        assert f(d.p, e.p, dim, I4(*bad), None) == ERR_ARG
        assert g(dim, I4(*bad), 1, out) == ERR_ARG
    assert f(d.p, d.p, dim, perm, None) == ERR_ARG                      # dst == src
    assert f(d.p, d.p, dim, I4(0, 1, 2, 3), None) == ERR_ARG            # ... for the copy too
    half = ctypes.c_void_p(d.p.value + 4 * 32)
    assert f(d.p, half, I4(1, 2, 4, 4), I4(0, 2, 1, 3), None) == OK     # 32 elements each, back to back: no overlap
    assert f(d.p, ctypes.c_void_p(d.p.value + 4 * 31), I4(1, 2, 4, 4), I4(0, 2, 1, 3), None) == ERR_ARG   # the last element of src
    assert f(ctypes.c_void_p(d.p.value + 4 * 31), d.p, I4(1, 2, 4, 4), I4(0, 2, 1, 3), None) == ERR_ARG   # dst in front, its last element
    assert g(dim, perm, 1, None) == ERR_ARG
    assert g(None, perm, 1, out) == ERR_ARG and g(dim, None, 1, out) == ERR_ARG
    # a merged extent above 2^32 where the kernels keep it in 32 bits: (N,H) and (W,C) of 2^34 elements each swap places
    big = I4(1 << 17, 1 << 17, 1 << 3, 1 << 3)
    assert g(big, I4(2, 3, 0, 1), 1, out) == ERR_ARG
    assert g(big, I4(0, 1, 2, 3), 1, out) == OK and list(out)[0] == COPY  # the contiguous run itself may be that long
    assert lcount(t4k) - l0 == 1                                         # the one legal call above
    got = d.get(t4k, (64,))
    assert np.array_equal(got[:32], a[:32]) and np.array_equal(got[32:].reshape(4, 2, 4), a[:32].reshape(2, 4, 4).transpose(1, 0, 2))
    assert np.array_equal(e.get(t4k, (64,)), np.ones(64, np.float32))
