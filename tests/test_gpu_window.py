"""t4k_window / t4k_window_plan (include/t4k.h, csrc/window.hip) through the C ABI.

Operands are random 32-bit patterns viewed as float32 (NaN payloads, denormals and infinities among them) and results are compared as
uint32 against NumPy slicing and assignment: pure data movement, nothing to tolerate.  dst is pre-filled with a second pattern and
checked everywhere outside the box; every case also checks that src is intact, that the guard floats in front of and behind both buffers
(Dev of tests/test_gpu_bcast.py, 4 floats in front here) are untouched, and that the call was exactly one launch.  The family, the
float4 path, the run length, the runs, the digits and the work items a case means to reach are asserted through t4k_window_plan; the
rule behind them is worked out by hand in tests/test_window_plan.py.

Unlike the runs of t4k_permute, a run family with ONE digit exists here (a C-range: N, H and W merge into one digit above the run), so
the run cases use 0 (the copy), 1, 2 and 3 digits."""
import ctypes
import zlib

import numpy as np
import pytest

from test_gpu_bcast import Dev, lcount

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
COPY, RUNS = 0, 1
I4 = ctypes.c_int * 4
I6 = ctypes.c_int * 6
FRONT = 4                                                               # guard floats in front of a buffer: 16 bytes, the alignment stays
Z = (0, 0, 0, 0)


def plan(h, sdim, soff, ddim, doff, ext, aligned=1):
    out = I6()
    assert h.lib.t4k_window_plan(I4(*sdim), I4(*soff), I4(*ddim), I4(*doff), I4(*ext), aligned, out) == OK, h.lib.t4k_last_error()
    return list(out)


def bits(shape, tag=""):
    rng = np.random.default_rng(zlib.crc32(repr((tuple(shape), tag)).encode()))
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32)


def guards_intact(dev):
    whole = dev.t.cpu().numpy().view(np.uint32)
    return not whole[:dev.off].any() and not whole[dev.off + dev.n:].any()


def run_case(h, sdim, soff, ddim, doff, ext, offs=(FRONT, FRONT)):
    sdim, soff, ddim, doff, ext = (tuple(int(v) for v in t) for t in (sdim, soff, ddim, doff, ext))
    a, fill = bits(sdim, (soff, ext)), bits(ddim, (doff, ext, "fill"))
    dS, dD = Dev(a.view(np.float32), offs[0]), Dev(fill.view(np.float32), offs[1])
    l0 = lcount(h)
    h.call("t4k_window", dS.p, I4(*sdim), I4(*soff), dD.p, I4(*ddim), I4(*doff), I4(*ext), None)
    assert lcount(h) - l0 == 1, (sdim, soff, ddim, doff, ext)
    got = dD.get(h, ddim).view(np.uint32)
    want = fill.copy()
    want[tuple(slice(o, o + e) for o, e in zip(doff, ext))] = a[tuple(slice(o, o + e) for o, e in zip(soff, ext))]
    assert np.array_equal(got, want), (sdim, soff, ddim, doff, ext, int(np.sum(got != want)))   # the box, and everything outside it
    assert np.array_equal(dS.get(h, sdim).view(np.uint32), a)           # src is intact
    assert guards_intact(dD) and guards_intact(dS)                      # nothing written in front of or behind either buffer
    return plan(h, sdim, soff, ddim, doff, ext, int(offs[0] % 4 == 0 and offs[1] % 4 == 0))


def slice_case(h, sdim, box, **kw):
    """box -> dense"""
    ext = [hi - lo for lo, hi in box]
    return run_case(h, sdim, [lo for lo, _ in box], ext, Z, ext, **kw)


def store_case(h, ddim, box, **kw):
    """dense -> box"""
    ext = [hi - lo for lo, hi in box]
    return run_case(h, ext, Z, ddim, [lo for lo, _ in box], ext, **kw)


# ---------------------------------------------------------------- every subset of axes, three directions
DIM = (3, 5, 7, 6)


def mask_id(m):
    return "".join(c for i, c in enumerate("NHWC") if m & (8 >> i)) or "whole"


@pytest.mark.parametrize("mask", range(16), ids=mask_id)
def test_every_subset_of_axes_in_three_directions(t4k, mask):
    cutb = [bool(mask & (8 >> i)) for i in range(4)]
    box = [(1, e - 1) if c else (0, e) for c, e in zip(cutb, DIM)]
    ext = [hi - lo for lo, hi in box]
    groups = []                                                         # what the merge leaves, outermost first (N cut has extent 1 and vanishes)
    for i in range(4):
        if ext[i] == 1:
            continue
        if groups and not cutb[i]:                                      # whole on both sides: it joins its outer neighbour
            groups[-1] *= ext[i]
        else:
            groups.append(ext[i])
    p = slice_case(t4k, DIM, box)
    q = store_case(t4k, DIM, box)
    assert p == q, (p, q)
    assert p[0] == (COPY if len(groups) == 1 else RUNS) and p[2] == groups[-1] and p[4] == len(groups) - 1, (mask, p, groups)
    # box -> box: the box lands 2 in on the cut axes of a destination one larger there, and at 0 of an axis of the same extent elsewhere
    ddim = [e + 1 if c else e for c, e in zip(cutb, DIM)]
    r = run_case(t4k, DIM, [lo for lo, _ in box], ddim, [2 if c else 0 for c in cutb], ext)
    assert r[2] == p[2] and r[3] == p[3] and r[4] == p[4], (mask, p, r)
    # ... and in a destination that is larger on EVERY axis nothing merges: N (where it is not of extent 1), H, W and a run of C
    ddim = [e + 2 for e in DIM]
    r = run_case(t4k, DIM, [lo for lo, _ in box], ddim, [1, 2, 0, 1], ext)
    assert r[0] == RUNS and r[2] == ext[3] and r[4] == (2 if ext[0] == 1 else 3), (mask, r)


# ---------------------------------------------------------------- run lengths, digits, pointer alignment
LENGTHS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1024, 1028]


@pytest.mark.parametrize("digits", [0, 1, 2, 3])
@pytest.mark.parametrize("L", LENGTHS)
def test_run_lengths_digits_and_pointers(t4k, L, digits):
    """a C-range [0, L) of a tensor with C = L + pad (pad = 4 where L is a multiple of 4, so that the float4 path is reached; 1 elsewhere):
    0 digits - the tensor is (1,1,1,L) and whole; 1 - N, H and W merge above the run; 2 - H is cut as well, W = 1; 3 - H and W are cut.
    1028 = 257 float4s, one more than 256 lanes take in one pass, and 1028 > 256 floats on the scalar path"""
    pad = 4 if L % 4 == 0 else 1
    sdim, box = {0: ((1, 1, 1, L), [(0, 1), (0, 1), (0, 1), (0, L)]),
                 1: ((3, 2, 2, L + pad), [(0, 3), (0, 2), (0, 2), (0, L)]),
                 2: ((3, 4, 1, L + pad), [(0, 3), (1, 3), (0, 1), (0, L)]),
                 3: ((2, 4, 4, L + pad), [(0, 2), (1, 3), (1, 4), (0, L)])}[digits]
    R = {0: 1, 1: 12, 2: 6, 3: 12}[digits]
    for offs in ((FRONT, FRONT), (FRONT + 1, FRONT), (FRONT, FRONT + 1)):   # either pointer 4 bytes off 16: the scalar path
        vec = int(L % 4 == 0 and offs == (FRONT, FRONT))
        units = L // 4 if vec else L
        lanes = 1
        while lanes < min(units, 256):
            lanes *= 2
        items = -(-R // (256 // lanes)) * -(-units // 256)
        for case in (slice_case, store_case):
            p = case(t4k, sdim, box, offs=offs)
            assert p == [RUNS if digits else COPY, vec, L, R, digits, items], (L, digits, offs, p)


@pytest.mark.parametrize("c0", [0, 1, 4])
def test_channel_offset_against_a_float4_able_run(t4k, c0):
    """runs of 8 floats, 16 and 8 apart: float4s when the box starts on 16 bytes, which c0 = 1 breaks"""
    box = [(0, 2), (0, 3), (0, 2), (c0, c0 + 8)]
    assert slice_case(t4k, (2, 3, 2, 16), box)[:5] == [RUNS, int(c0 % 4 == 0), 8, 12, 1]
    assert store_case(t4k, (2, 3, 2, 16), box)[:5] == [RUNS, int(c0 % 4 == 0), 8, 12, 1]
    # a base pointer 12 bytes off and c0 = 1 put the box start back on 16 bytes: the result is the same whichever path is taken
    slice_case(t4k, (2, 3, 2, 16), box, offs=(FRONT + 3, FRONT))


# ---------------------------------------------------------------- the stride loop wraps
def test_grid_cap_short_runs(t4k):
    """70 000 runs of 3 (64 runs to a pass: 1 094 passes, below the cap of 2 048 workgroups), 140 000, whose 2 188 passes wrap, and
    600 000, whose 9 375 passes are more than the four a workgroup keeps in flight per sweep of the grid"""
    for n, items in ((70000, 1094), (140000, 2188), (600000, 9375)):
        p = slice_case(t4k, (n, 1, 1, 4), [(0, n), (0, 1), (0, 1), (0, 3)])
        assert p == [RUNS, 0, 3, n, 1, items], p
    p = store_case(t4k, (140000, 1, 1, 4), [(0, 140000), (0, 1), (0, 1), (1, 4)])
    assert p == [RUNS, 0, 3, 140000, 1, 2188], p


def test_grid_cap_long_runs(t4k):
    """9 runs of 235 chunks on both paths: 60 001 floats on the scalar one, 240 000 (60 000 float4s) on the other; 2 115 passes wrap"""
    p = slice_case(t4k, (3, 3, 1, 60002), [(0, 3), (0, 3), (0, 1), (1, 60002)])
    assert p == [RUNS, 0, 60001, 9, 1, 9 * 235], p
    p = slice_case(t4k, (3, 3, 1, 240004), [(0, 3), (0, 3), (0, 1), (4, 240004)])
    assert p == [RUNS, 1, 240000, 9, 1, 9 * 235], p
    p = store_case(t4k, (3, 3, 1, 240004), [(0, 3), (0, 3), (0, 1), (0, 240000)])
    assert p == [RUNS, 1, 240000, 9, 1, 9 * 235], p


def test_copy_family_chunks(t4k):
    """one run of many chunks: an N-range of 2 400 000 floats, 2 344 passes of float4s and 9 375 scalar ones"""
    box = [(1, 4), (0, 100), (0, 100), (0, 80)]
    assert slice_case(t4k, (5, 100, 100, 80), box) == [COPY, 1, 2400000, 1, 0, 2344]
    assert slice_case(t4k, (5, 100, 100, 80), box, offs=(FRONT + 1, FRONT)) == [COPY, 0, 2400000, 1, 0, 9375]


def test_single_element(t4k):
    assert run_case(t4k, (1, 1, 1, 1), Z, (1, 1, 1, 1), Z, (1, 1, 1, 1)) == [COPY, 0, 1, 1, 0, 1]
    assert run_case(t4k, (3, 5, 7, 6), (2, 4, 6, 5), (2, 2, 2, 2), (1, 0, 1, 1), (1, 1, 1, 1)) == [COPY, 0, 1, 1, 0, 1]


# ---------------------------------------------------------------- against the existing entry
def test_n_range_equals_t4k_copy(t4k):
    dim, n0, n1 = (6, 9, 7, 5), 2, 5
    a = bits(dim, "copy")
    block = dim[1] * dim[2] * dim[3]
    cnt = (n1 - n0) * block
    dS = Dev(a.view(np.float32))
    dW, dC = Dev(np.zeros(cnt, np.float32)), Dev(np.zeros(cnt, np.float32))
    ext = (n1 - n0,) + dim[1:]
    t4k.call("t4k_window", dS.p, I4(*dim), I4(n0, 0, 0, 0), dW.p, I4(*ext), I4(*Z), I4(*ext), None)
    t4k.call("t4k_copy", ctypes.c_void_p(dS.p.value + 4 * n0 * block), dC.p, cnt, None)
    assert np.array_equal(dW.get(t4k, ext).view(np.uint32), dC.get(t4k, ext).view(np.uint32))
    assert np.array_equal(dW.get(t4k, ext).view(np.uint32), a[n0:n1])


# ---------------------------------------------------------------- error returns
def test_error_returns_launch_nothing(t4k):
    a = np.arange(64, dtype=np.float32)
    d, e = Dev(a), Dev(np.ones(64, np.float32))
    f = t4k.lib.t4k_window
    good = dict(sdim=(2, 2, 4, 4), soff=(0, 0, 1, 0), ddim=(2, 2, 2, 4), doff=Z, ext=(2, 2, 2, 4))

    def call(src=d.p, dst=e.p, **kw):
        v = {k: (None if x is None else I4(*x)) for k, x in {**good, **kw}.items()}
        return f(src, v["sdim"], v["soff"], dst, v["ddim"], v["doff"], v["ext"], None)

    l0 = lcount(t4k)
    assert call(src=None) == ERR_ARG and call(dst=None) == ERR_ARG
    for name in good:
        assert call(**{name: None}) == ERR_ARG, name
    assert call(ext=(2, 2, 0, 4)) == ERR_ARG and call(ext=(2, -2, 2, 4)) == ERR_ARG      # an extent < 1
    assert call(sdim=(2, 0, 4, 4)) == ERR_ARG and call(ddim=(2, 2, 2, 0)) == ERR_ARG
    assert call(soff=(0, 0, -1, 0)) == ERR_ARG and call(doff=(0, -1, 0, 0)) == ERR_ARG   # a negative offset
    assert call(soff=(0, 0, 3, 0)) == ERR_ARG and call(soff=(1, 0, 0, 0)) == ERR_ARG     # off + ext > dim on the source side
    assert call(doff=(0, 0, 1, 0)) == ERR_ARG and call(doff=(0, 0, 0, 1)) == ERR_ARG     # ... on the destination side
    big, one = (1 << 11, 1 << 10, 1 << 10, 1 << 10), (1, 1, 1, 1)                         # 2^41 elements on either side
    assert call(sdim=big, soff=Z, ddim=one, doff=Z, ext=one) == ERR_ARG
    assert call(sdim=one, soff=Z, ddim=big, doff=Z, ext=one) == ERR_ARG
    wide, ext = (2, 1 << 17, 1 << 17, 3), (2, (1 << 17) - 1, 1 << 17, 2)                  # an inner digit of 2^34 - 2^17 (tests/test_window_plan.py)
    assert call(sdim=wide, soff=Z, ddim=ext, doff=Z, ext=ext) == ERR_ARG
    # any overlap of the two tensors' whole byte ranges, the boxes apart or not
    assert call(dst=d.p) == ERR_ARG                                                       # dst == src
    at = lambda k: ctypes.c_void_p(d.p.value + 4 * k)
    small = dict(sdim=(1, 2, 4, 4), soff=Z, ddim=(1, 2, 2, 4), doff=Z, ext=(1, 2, 2, 4))  # 32 elements of src, 16 of dst
    assert call(dst=at(31), **small) == ERR_ARG                                           # the last element of src
    assert call(src=at(15), dst=d.p, **small) == ERR_ARG                                  # dst in front, its last element
    assert lcount(t4k) == l0
    assert call(dst=at(32), **small) == OK                                                # back to back: no overlap
    assert call() == OK
    assert lcount(t4k) - l0 == 2                                                          # the two legal calls
    got = d.get(t4k, (64,))
    assert np.array_equal(got[:32], a[:32]) and np.array_equal(got[32:48].reshape(2, 2, 4), a[:32].reshape(2, 4, 4)[:, :2])
    assert np.array_equal(got[48:], a[48:])
    src = got.reshape(2, 2, 4, 4)                                                         # what d held when the second call read it
    got = e.get(t4k, (64,))
    assert np.array_equal(got[:32].reshape(2, 2, 2, 4), src[:, :, 1:3]) and np.array_equal(got[32:], np.ones(32, np.float32))
