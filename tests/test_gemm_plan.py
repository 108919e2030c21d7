"""t4k_gemm_plan (include/t4k.h, csrc/gemm.hip): the plan gemm_launch makes for one product, on the host alone - nothing is
launched and no device is needed, so these rows run wherever the library loads (the arrangement of test_conv_geo_plan.py).

The entry calls the planner gemm_launch calls.  The table of gemm_cases.py is held against it at 256 CUs, and the Python mirror of the ladder
(gemm_cases.ladder, which the GPU sweeps size their rows with) field by field - plan text, launches, nsplit, kchunk, riders_ride, cs_ride,
deferred - over a grid of extents round every threshold of the ladder at 64, 256 and 304 CUs, with every input the mirror takes that the C++
could only be asked about by staging the situation on a device: the alignment of each operand, the epilogue, a bias, a library stream, a
capture in progress, a caller that folds, a column-sum request, riders, gates switched off."""
import ctypes
import itertools

import numpy as np
import pytest

import gemm_cases as gc

OK, ERR_ARG = 0, -1
A16, B16, EPILOGUE, BIAS, RIDER, DEFER, LANE, CAPTURING, GATES_OFF = (gc.GP_A16, gc.GP_B16, gc.GP_EPILOGUE, gc.GP_BIAS, gc.GP_RIDER, gc.GP_DEFER, gc.GP_LANE,
                                                                          gc.GP_CAPTURING, gc.GP_GATES_OFF)
FIELDS = ("plan", "launches", "nsplit", "kchunk", "riders_ride", "cs_ride", "deferred")
EXTENTS = (1, 2, 3, 4, 33, 64, 100, 128, 256, 500, 512, 576, 640, 768, 1024, 1536, 2048, 2050, 4096, 4352)
DEPTHS = (0, 1, 4, 8, 12, 13, 64, 100, 128, 132, 192, 256, 288, 300, 512, 784, 832, 836, 896, 1024, 1280, 2048, 2112, 4096)
CS_ROWS = (0, 128, 5000)
I6 = ctypes.c_int * 6
entry = gc.plan_entry


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def mirror(M, N, K, C, tA, tB, flags, cs_rows=0, cu=256):
    """gemm_cases.ladder asked what the flags word asks; its `aligned` is both alignment bits"""
    r = gc.ladder(M, N, K, tA, tB, C, cu, aligned=bool(flags & A16) and bool(flags & B16), alpha=2.0 if flags & EPILOGUE else 1.0, beta=0.0,
                  bias=bool(flags & BIAS), lane=1 if flags & LANE else 0, capturing=bool(flags & CAPTURING), defer=bool(flags & DEFER),
                  cs_rows=cs_rows, riders=bool(flags & RIDER), gates=not flags & GATES_OFF)
    return tuple(r[f] for f in FIELDS)


def test_the_table_at_256_cus(lib):
    for r in gc.ROWS:
        got = entry(lib, r.M, r.N, r.K, r.C, r.tA, r.tB, 0 if r.skew else A16 | B16)
        assert got[0] == r.label, (r.id, got)
        assert got[1] == r.plan(256)[1], (r.id, got)


def test_the_mirror_against_the_planner(lib):
    """the full product of the extents, layouts and channel counts at three CU counts, the other inputs drawn per case; on the table's rows
    the full product of those inputs.  Every base form of the mirror, "none" and "k0" are reached at 256 CUs"""
    n, seen = 0, set()

    def same(cu, *q):
        got, want = entry(lib, *q, cu=cu), mirror(*q, cu=cu)
        assert got == want, "M N K C tA tB flags cs_rows = %s at %d CUs: the planner %s, the mirror %s" % (q, cu, got, want)
        return got[0]

    for cu in (64, 256, 304):
        cases = list(itertools.product(EXTENTS, EXTENTS, DEPTHS, (0, 1), (0, 1), (1, 2)))
        rng = np.random.default_rng(cu)
        # the odds keep most cases on aligned operands of the default stream, where the ladder has the most rungs
        p_set = dict(((A16, .85), (B16, .85), (EPILOGUE, .4), (BIAS, .3), (RIDER, .3), (DEFER, .25), (LANE, .2), (CAPTURING, .15), (GATES_OFF, .15)))
        flags = sum((rng.random(len(cases)) < p).astype(np.int64) * bit for bit, p in p_set.items())
        rows = rng.choice(CS_ROWS, len(cases), p=(.6, .3, .1))
        for (M, N, K, tA, tB, C), f, cs in zip(cases, flags.tolist(), rows.tolist()):
            plan = same(cu, M, N, K, C, tA, tB, f, cs)
            if cu == 256:
                seen.add(plan.split("x")[0].split("+")[0])
        n += len(cases)
    for M, N, K in ((0, 8, 8), (8, 0, 8), (0, 0, 0), (0, 4096, 4096)):             # the grid holds no empty output
        seen.add(same(256, M, N, K, 1, 0, 0, A16 | B16, 0)); n += 1
    for r in gc.ROWS:
        for f in range(1 << 9):
            for cs in CS_ROWS:
                same(256, r.M, r.N, r.K, r.C, r.tA, r.tB, f, cs)
        n += 3 << 9
    assert seen == set(gc.ALL_BASES) | {"none", "k0"}, seen ^ (set(gc.ALL_BASES) | {"none", "k0"})
    assert n >= 200000, n


def test_only_both_operands_aligned_counts(lib):
    """the sliver rung tests each operand's alignment by itself, but its DMA lanes and the 16-byte loads of every other rung need both: one
    operand off 16 bytes plans as both off"""
    for r in gc.ROWS:
        for f in (0, EPILOGUE, DEFER, RIDER | BIAS):
            off = entry(lib, r.M, r.N, r.K, r.C, r.tA, r.tB, f)
            assert off == entry(lib, r.M, r.N, r.K, r.C, r.tA, r.tB, f | A16) == entry(lib, r.M, r.N, r.K, r.C, r.tA, r.tB, f | B16), r.id


def test_defaults_of_cu_and_workspace(lib):
    """cu = 0 is the library's count - 256 before t4k_init -, ws_bytes = 0 the 64 MiB workspace"""
    q = (512, 512, 1024, 1, 0, 0, A16 | B16)
    assert entry(lib, *q, cu=0) == entry(lib, *q, cu=256) == entry(lib, *q, cu=256, ws=gc.WS_BYTES)
    assert entry(lib, *q)[0] == "glds8<128>x4+fold" and entry(lib, *q, ws=4 << 20)[0] == "nn_plain"    # four slabs of 1 MiB do not fit half of 4 MiB


def test_rejections(lib):
    text, out = ctypes.create_string_buffer(64), I6()
    good = (64, 64, 64, 1, 0, 0, A16 | B16, 0, 256, 0)
    assert lib.t4k_gemm_plan(*good, text, out) == OK and text.value == b"l32/w4"
    assert lib.t4k_gemm_plan(*good, None, out) == ERR_ARG and lib.t4k_gemm_plan(*good, text, None) == ERR_ARG
    for k, v in ((0, -1), (1, -1), (2, -1), (3, 0), (3, -2), (8, -1), (9, -1)):           # M, N, K < 0; C < 1; cu < 0; ws_bytes < 0
        bad = list(good); bad[k] = v
        out[:] = [-7] * 6
        assert lib.t4k_gemm_plan(*bad, text, out) == ERR_ARG, bad
        assert list(out) == [-7] * 6 and b"bad argument" in lib.t4k_last_error()
