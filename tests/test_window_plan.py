"""t4k_window_plan (include/t4k.h, csrc/window.hip): the plan of a box copy, on the host alone - nothing is launched and no
device is needed, so these rows run wherever the library loads.

out = { family (0 copy, 1 runs), float4 path, run length L, runs R, digits of the run index, work items }.  The expected rows are worked
out by hand from the rule of 3.14: axes of extent 1 fold into the two box starts; an axis merges with its inner neighbour when that one
is taken whole on both sides; the float4 path needs L % 4 == 0, every stride left a multiple of 4 and both box starts on 16 bytes; a
256-lane pass takes 256 / 2^k runs of 2^k lanes (2^k the smallest power of two holding a run's units) or one 256-unit chunk of a run."""
import ctypes

import pytest

OK, ERR_ARG = 0, -1
COPY, RUNS = 0, 1
I4 = ctypes.c_int * 4
I6 = ctypes.c_int * 6
SAT = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, sdim, soff, ddim, doff, ext, aligned=1):
    out = I6()
    rc = lib.t4k_window_plan(I4(*sdim), I4(*soff), I4(*ddim), I4(*doff), I4(*ext), aligned, out)
    assert rc == OK, lib.t4k_last_error()
    return list(out)


def cut(lib, sdim, box, aligned=1):
    """box -> dense: the slice of `sdim` over the (lo, hi) pairs of `box`"""
    ext = [hi - lo for lo, hi in box]
    return plan(lib, sdim, [lo for lo, _ in box], ext, (0, 0, 0, 0), ext, aligned)


Z = (0, 0, 0, 0)
ROWS = {
    # an N-range: nothing is left above the run, which is the whole block; the box starts 30 floats in, so no float4s ...
    "n_range_copy": (((4, 3, 5, 2), (1, 0, 0, 0), (2, 3, 5, 2), Z, (2, 3, 5, 2), 1), [COPY, 0, 60, 1, 0, 1]),
    # ... and 60 floats in it has them
    "n_range_copy_float4": (((4, 3, 5, 2), (2, 0, 0, 0), (2, 3, 5, 2), Z, (2, 3, 5, 2), 1), [COPY, 1, 60, 1, 0, 1]),
    "whole_tensor": (((4, 3, 5, 2), Z, (4, 3, 5, 2), Z, (4, 3, 5, 2), 1), [COPY, 1, 120, 1, 0, 1]),
    # a C-range [2,5) of (2,3,4,6): N, H and W are one digit of 24 runs of 3
    "c_range": (((2, 3, 4, 6), (0, 0, 0, 2), (2, 3, 4, 3), Z, (2, 3, 4, 3), 1), [RUNS, 0, 3, 24, 1, 1]),
    # a W-crop [0,2) of (2,3,3,2): runs of 4 floats, but 6 apart in the source
    "w_crop_stride_6": (((2, 3, 3, 2), Z, (2, 3, 2, 2), Z, (2, 3, 2, 2), 1), [RUNS, 0, 4, 6, 1, 1]),
    # a C-range [4,8) of (2,3,1,12): runs of 4, 12 and 4 apart, starting 4 floats in
    "c_range_float4": (((2, 3, 1, 12), (0, 0, 0, 4), (2, 3, 1, 4), Z, (2, 3, 1, 4), 1), [RUNS, 1, 4, 6, 1, 1]),
    "c_range_unaligned_pointers": (((2, 3, 1, 12), (0, 0, 0, 4), (2, 3, 1, 4), Z, (2, 3, 1, 4), 0), [RUNS, 0, 4, 6, 1, 1]),
    "c_range_from_5": (((2, 3, 1, 12), (0, 0, 0, 5), (2, 3, 1, 4), Z, (2, 3, 1, 4), 1), [RUNS, 0, 4, 6, 1, 1]),
    # the same run stored 1 float into the destination
    "c_range_to_1": (((2, 3, 1, 4), Z, (2, 3, 1, 12), (0, 0, 0, 1), (2, 3, 1, 4), 1), [RUNS, 0, 4, 6, 1, 1]),
    # an H-and-C box of (3,5,7,6) into a dense tensor: W is whole on both sides and joins H - N, HW and the run
    "h_and_c_box_to_dense": (((3, 5, 7, 6), (0, 1, 0, 1), (3, 3, 7, 4), Z, (3, 3, 7, 4), 1), [RUNS, 0, 4, 63, 2, 1]),
    # ... and into a box of (3,6,8,7), where W is not whole: N, H, W and the run - three digits
    "h_and_c_box_to_box": (((3, 5, 7, 6), (0, 1, 0, 1), (3, 6, 8, 7), (0, 1, 1, 2), (3, 3, 7, 4), 1), [RUNS, 0, 4, 63, 3, 1]),
    # extent-1 axes vanish: one row of one column of every sample leaves N above a run of C
    "extent_1_h_w": (((3, 5, 7, 6), (0, 2, 3, 0), (3, 1, 1, 6), Z, (3, 1, 1, 6), 1), [RUNS, 0, 6, 3, 1, 1]),
    # ... one sample is a copy of its block
    "extent_1_n": (((4, 3, 5, 2), (2, 0, 0, 0), (1, 3, 5, 2), Z, (1, 3, 5, 2), 1), [COPY, 0, 30, 1, 0, 1]),
    # ... one channel of one sample: H and W are one digit of 35 runs of one float
    "extent_1_n_c": (((3, 5, 7, 6), (1, 0, 0, 2), (1, 5, 7, 1), Z, (1, 5, 7, 1), 1), [RUNS, 0, 1, 35, 1, 1]),
    "single_element": (((1, 1, 1, 1), Z, (1, 1, 1, 1), Z, (1, 1, 1, 1), 1), [COPY, 0, 1, 1, 0, 1]),
    "single_element_of_a_tensor": (((3, 5, 7, 6), (2, 4, 6, 5), (2, 2, 2, 2), (1, 1, 1, 1), (1, 1, 1, 1), 1), [COPY, 0, 1, 1, 0, 1]),
    # work items: 20 000 float4s are 79 chunks of 256 lanes, 80 000 floats 313
    "long_run_float4": (((4, 100, 100, 4), (1, 0, 0, 0), (2, 100, 100, 4), Z, (2, 100, 100, 4), 1), [COPY, 1, 80000, 1, 0, 79]),
    "long_run_scalar": (((4, 100, 100, 4), (1, 0, 0, 0), (2, 100, 100, 4), Z, (2, 100, 100, 4), 0), [COPY, 0, 80000, 1, 0, 313]),
    # 70 000 runs of 3: 4 lanes a run, 64 runs a pass
    "many_short_runs": (((70000, 1, 1, 4), Z, (70000, 1, 1, 3), Z, (70000, 1, 1, 3), 1), [RUNS, 0, 3, 70000, 1, 1094]),
    # 9 runs of 240 000 floats 240 004 apart: 235 chunks each on the float4 path, 938 on the scalar one
    "long_runs_float4": (((3, 3, 1, 240004), Z, (3, 3, 1, 240000), Z, (3, 3, 1, 240000), 1), [RUNS, 1, 240000, 9, 1, 9 * 235]),
    "long_runs_scalar": (((3, 3, 1, 240004), Z, (3, 3, 1, 240000), Z, (3, 3, 1, 240000), 0), [RUNS, 0, 240000, 9, 1, 9 * 938]),
    # L and R saturate at 2^31 - 1: a whole tensor of 2^39 floats, and 2^32 runs of 2
    "run_length_saturates": (((1 << 10, 1 << 10, 1 << 10, 1 << 9),) + (Z, (1 << 10, 1 << 10, 1 << 10, 1 << 9), Z, (1 << 10, 1 << 10, 1 << 10, 1 << 9), 1),
                             [COPY, 1, SAT, 1, 0, 1 << 29]),
    "runs_saturate": (((1 << 16, 1 << 16, 1, 4), Z, (1 << 16, 1 << 16, 1, 2), Z, (1 << 16, 1 << 16, 1, 2), 1), [RUNS, 0, 2, SAT, 1, 1 << 25]),
}


@pytest.mark.parametrize("row", list(ROWS))
def test_plan_rows(lib, row):
    args, want = ROWS[row]
    assert plan(lib, *args) == want


def test_a_store_plans_like_the_slice_of_the_same_box(lib):
    for name, (args, want) in ROWS.items():
        sdim, soff, ddim, doff, ext, aligned = args
        assert plan(lib, ddim, doff, sdim, soff, ext, aligned) == want, name


def test_sixteen_subsets_of_a_shape(lib):
    """(4,5,7,6) cut to [1, extent - 1) on every subset of axes, box -> dense: the digits are the groups the merge rule leaves above the run"""
    dim = (4, 5, 7, 6)
    for mask in range(16):
        box = [(1, e - 1) if mask & (8 >> i) else (0, e) for i, e in enumerate(dim)]
        ext = [hi - lo for lo, hi in box]
        groups = []                                                     # outermost first
        for i in range(4):
            if i and not mask & (8 >> i):                               # this axis is whole on both sides: it joins its outer neighbour
                groups[-1] *= ext[i]
            else:
                groups.append(ext[i])
        p = cut(lib, dim, box)
        assert p[0] == (COPY if len(groups) == 1 else RUNS), (mask, p)
        assert p[2] == groups[-1] and p[4] == len(groups) - 1, (mask, p, groups)
        R = 1
        for g in groups[:-1]:
            R *= g
        assert p[3] == R, (mask, p)


def test_error_returns(lib):
    f = lib.t4k_window_plan
    out = I6()
    good = dict(sdim=(3, 5, 7, 6), soff=(0, 1, 2, 3), ddim=(4, 4, 4, 4), doff=(1, 0, 1, 0), ext=(2, 3, 3, 2))
    call = lambda **kw: f(*[None if v is None else I4(*v) for v in {**good, **kw}.values()], 1, out)
    assert call() == OK
    for name in good:                                                   # NULL for each of the five arrays, and for out
        assert call(**{name: None}) == ERR_ARG, name
    assert f(*[I4(*v) for v in good.values()], 1, None) == ERR_ARG
    for axis in range(4):
        bump = lambda v, by: tuple(x + (by if i == axis else 0) for i, x in enumerate(v))
        zero = lambda v: tuple(0 if i == axis else x for i, x in enumerate(v))
        assert call(ext=zero(good["ext"])) == ERR_ARG                   # an extent < 1
        assert call(ext=bump(zero(good["ext"]), -1)) == ERR_ARG
        assert call(sdim=zero(good["sdim"])) == ERR_ARG and call(ddim=zero(good["ddim"])) == ERR_ARG
        assert call(soff=bump(zero(good["soff"]), -1)) == ERR_ARG       # a negative offset
        assert call(doff=bump(zero(good["doff"]), -1)) == ERR_ARG
        room_s = good["sdim"][axis] - good["ext"][axis] - good["soff"][axis]
        room_d = good["ddim"][axis] - good["ext"][axis] - good["doff"][axis]
        assert call(soff=bump(good["soff"], room_s)) == OK and call(soff=bump(good["soff"], room_s + 1)) == ERR_ARG   # off + ext > dim
        assert call(doff=bump(good["doff"], room_d)) == OK and call(doff=bump(good["doff"], room_d + 1)) == ERR_ARG
    big, fits = (1 << 11, 1 << 10, 1 << 10, 1 << 10), (1 << 10, 1 << 10, 1 << 10, 1 << 10)      # 2^41 and 2^40 elements
    one = (1, 1, 1, 1)
    assert call(sdim=big, soff=Z, ddim=one, doff=Z, ext=one) == ERR_ARG
    assert call(sdim=one, soff=Z, ddim=big, doff=Z, ext=one) == ERR_ARG
    assert call(sdim=fits, soff=Z, ddim=one, doff=Z, ext=one) == OK and call(sdim=one, soff=Z, ddim=fits, doff=Z, ext=one) == OK
    # a digit kept in 32 bits: H (cut) and W (whole) merge into 2^34 - 2^17 rows of a C-range, beneath N - but as the outermost digit,
    # which no division touches, the same extent is taken
    wide = (2, 1 << 17, 1 << 17, 3)
    ext = (2, (1 << 17) - 1, 1 << 17, 2)
    assert call(sdim=wide, soff=Z, ddim=ext, doff=Z, ext=ext) == ERR_ARG
    ext = (1,) + ext[1:]
    assert call(sdim=wide, soff=Z, ddim=ext, doff=Z, ext=ext) == OK and list(out)[:5] == [RUNS, 0, 2, SAT, 1]
