"""The planner of the axis kernels (csrc/axes.h) and its two users (csrc/reduce_axes.hip, csrc/softmax_axes.hip) restated in Python, inequality by
inequality, and the table of shapes that tests/test_gpu_axes_sweep.py runs: one row for every pair of factor values the planner can reach together.

`reduce_plan` / `softmax_plan` return a Plan whose `fields()` are the eight numbers t4k_reduce_axes_plan / t4k_softmax_axes_geometry report
(include/t4k.h), plus the softmax regime and chunks.  tests/test_axes_cases.py holds the mirror equal to the library on a random walk, so a
planner change that moves a row off its label fails there (CPU) and in the sweep (GPU), never silently.

A label (`label`) names the code a launch runs: kernel, family, float4 path, lanes (row: shift, column: sx), split extent, regime (softmax),
an outer reduced extent (r1 > 1: the walk wraps from one run / outer index to the next), a second kept group (the divmod of the output
index), more than one tile (column), more than one pass of the grid-stride loop, and for k_red_row which of its two loops the lanes take."""
import collections
import itertools

import numpy as np

BLK, MAX_WG = 256, 2048                                                 # csrc/t4k_common.h
TARGET_LANES, TARGET_ITEMS, SPLIT_UNITS, MAX_SPLIT = 64 * 4 * 256 * 2, 1024, 8, 4096      # csrc/axes.h
LANE_UNITS = 16                                                         # csrc/reduce_axes.hip
NV = 8                                                                  # csrc/softmax_axes.hip
WS_BYTES = 64 << 20                                                     # csrc/runtime.hip: the library's workspace
ROW, COL = 0, 1
NONE, INNER, OUTER = 0, 1, 2                                            # split extent: none; U (row) or r0 (column); r1
REG, ONLINE, MULTI = 0, 1, 2

Merged = collections.namedtuple("Merged", "col four r0 k0 r1 k1")


def log2_ceil(x, cap):
    k = 0
    while k < cap and (1 << k) < x:
        k += 1
    return k


def ceil_div(a, b):
    return (a + b - 1) // b


def merge_axes(dim, mask):
    e, red, anyred = [], [], False
    for i in range(4):
        if dim[i] == 1:
            continue
        r = (mask & (8 >> i)) != 0
        anyred = anyred or r
        if e and red[-1] == r:
            e[-1] *= dim[i]
        else:
            e.append(dim[i]); red.append(r)
    if not anyred:
        e.append(1); red.append(True)
    n = len(e)
    at = lambda back: e[n - back] if n >= back else 1
    col = not red[-1]
    if col:
        return Merged(True, n == 4, at(2), at(1), at(4), at(3))
    if at(2) > 0xffffffff:
        raise ValueError("merged extent too large")                      # RowPlan::k0 is a 32-bit divisor: T4K_ERR_ARG
    return Merged(False, n == 4, at(1), at(2), at(3), at(4))


class Plan:
    """what one call launches first: the geometry the kernels take and what the plan entries report of it"""

    def __init__(self, kernel, m, vec):
        self.kernel, self.m, self.vec = kernel, m, bool(vec)
        self.family = COL if m.col else ROW
        self.S, self.per, self.split, self.regime, self.chunks, self.capped = 1, 0, NONE, None, 0, False

    def fields(self):
        return [self.family, self.launches, int(self.vec), self.lanes, self.sub, self.S, self.split, ceil_div(self.nitem, MAX_WG)]

    @property
    def launches(self):
        if self.kernel == "reduce":
            return 2 if self.S > 1 else 1
        return 3 if self.regime == MULTI else 1

    @property
    def trips(self):
        return ceil_div(self.nitem, MAX_WG)

    @property
    def rescales(self):
        """t4k_softmax_axes_plan's out[5]"""
        return 0 if self.regime == REG else self.chunks + 1 + (1 if self.regime == MULTI else 0)

    def __repr__(self):
        return "Plan(%s %s regime %s chunks %s nitem %d per %d %s)" % (self.kernel, self.fields(), self.regime, self.chunks, self.nitem, self.per, self.m)


def row_geometry(p):
    m = p.m
    p.nout, p.U, p.r1 = m.k0 * m.k1, (m.r0 >> 2 if p.vec else m.r0), m.r1


def col_geometry(p):
    m = p.m
    p.nout = m.k0 * m.k1
    Uk = m.k0 >> 2 if p.vec else m.k0
    p.lanes = log2_ceil(Uk, 6)                                          # sx
    p.sub = ceil_div(Uk, 1 << p.lanes)                                  # ntile
    p.nitem = m.k1 * p.sub


def row_lanes(T, loads_per_lane, nout):
    shift = log2_ceil(ceil_div(T, loads_per_lane), 8)
    cap = log2_ceil(T, 8)
    while shift < cap and (nout << shift) < TARGET_LANES:
        shift += 1
    if shift == 7:
        shift = 6 if (nout << 6) >= TARGET_LANES else 8
    return shift


def split_for(p, items, max_by_work, floats_per_part, parts_reserved, ws_floats):
    S = min(ceil_div(TARGET_ITEMS, items), max_by_work, MAX_SPLIT)
    cap = ws_floats // floats_per_part - parts_reserved
    p.capped = S >= 2 and cap < S                                       # the workspace decided
    S = min(S, cap)
    return 1 if S < 2 else S


def split_extent(ext, S):
    per = ceil_div(ext, S)
    return per, ceil_div(ext, per)


def row_split(p, floats_per_group, parts_reserved, ws_floats):
    S = split_for(p, p.nout, p.U * p.r1 // (BLK * SPLIT_UNITS), floats_per_group * p.nout, parts_reserved, ws_floats)
    if S < 2:
        return False
    p.split = INNER if p.U >= p.r1 else OUTER
    p.per, p.S = split_extent(p.U if p.split == INNER else p.r1, S)
    return True


def col_split(p, floats_per_group, parts_reserved, ws_floats):
    if p.nitem >= TARGET_ITEMS:
        return False
    by_r1 = p.m.r1 > p.m.r0
    S = split_for(p, p.nitem, p.m.r1 // 4 if by_r1 else p.m.r0 // ((BLK >> p.lanes) * SPLIT_UNITS), floats_per_group * p.nout, parts_reserved, ws_floats)
    if S < 2:
        return False
    p.split = OUTER if by_r1 else INNER
    p.per, p.S = split_extent(p.m.r1 if by_r1 else p.m.r0, S)
    p.nitem *= p.S
    return True


def _vec(m, aligned):
    return bool(aligned) and ((m.k0 if m.col else m.r0) & 3) == 0


def reduce_plan_merged(m, vec, may_split=True, ws_bytes=WS_BYTES):
    """launch_row / launch_col of reduce_axes.hip: LANE_UNITS loads a lane; a split only of a workgroup-wide group; one float per part"""
    ws_floats = ws_bytes // 4
    p = Plan("reduce", m, vec)
    if m.col:
        col_geometry(p)
        if may_split:
            col_split(p, 1, 0, ws_floats)
        return p
    row_geometry(p)
    p.lanes = row_lanes(p.U * p.r1, LANE_UNITS, p.nout)
    split = may_split and p.lanes == 8 and row_split(p, 1, 0, ws_floats)
    p.sub = min(p.lanes, log2_ceil(p.per if split and p.split == INNER else p.U, 8))
    p.nitem = ceil_div(p.nout, BLK >> p.lanes) * p.S
    return p


def reduce_plan(dim, mask, aligned=True, ws_bytes=WS_BYTES):
    m = merge_axes(dim, mask)
    return reduce_plan_merged(m, _vec(m, aligned), True, ws_bytes)


def reduce_stage_two(p):
    """the launch that folds the partials of a split plan: rows of S partials (row family) or an [S, nout] matrix (column family); a
    workspace is 16-byte aligned"""
    m = Merged(p.m.col, False, p.S, p.nout, 1, 1)
    return reduce_plan_merged(m, _vec(m, True), False)


def softmax_plan(dim, mask, aligned=True, ws_bytes=WS_BYTES):
    """make_plan of softmax_axes.hip: NV loads a lane, more lanes while the ceilings leave a lane more; two floats per part, one part reserved"""
    ws_floats = ws_bytes // 4
    m = merge_axes(dim, mask)
    p = Plan("softmax", m, _vec(m, aligned))
    if m.col:
        col_geometry(p)
        TY = BLK >> p.lanes
        n = ceil_div(m.r0, TY) * m.r1
        p.regime = REG if n <= NV else ONLINE
        if p.regime == ONLINE and col_split(p, 2, 1, ws_floats):
            p.regime = MULTI
            n = ceil_div(m.r0, TY) * p.per if p.split == OUTER else ceil_div(p.per, TY) * m.r1
        p.chunks = ceil_div(n, NV)
        return p
    row_geometry(p)
    p.lanes = row_lanes(p.U * p.r1, NV, p.nout)

    def slots(ext_u, ext_r):
        p.sub = min(p.lanes, log2_ceil(ext_u, 8))
        return ceil_div(ext_u, 1 << p.sub) * ceil_div(ext_r, (1 << p.lanes) >> p.sub)
    n = slots(p.U, p.r1)
    while n > NV and p.lanes < 8:
        p.lanes = 8 if p.lanes >= 6 else p.lanes + 1
        n = slots(p.U, p.r1)
    p.regime = REG if n <= NV else ONLINE
    if p.regime == ONLINE:
        assert p.lanes == 8
        if row_split(p, 2, 1, ws_floats):
            p.regime = MULTI
            n = slots(p.per, p.r1) if p.split == INNER else slots(p.U, p.per)
    p.chunks = ceil_div(n, NV)
    p.nitem = ceil_div(p.nout, BLK >> p.lanes) * p.S
    return p


# ---------------------------------------------------------------------------------------------------------------- labels
Label = collections.namedtuple("Label", "kernel family vec lanes split regime outer second tiles wrap loop")


def label(p):
    m = p.m
    loop = None
    if p.kernel == "reduce" and not m.col:                              # k_red_row: `ub - ua <= Gu` (a lane owns one unit of every run) or the two nested loops
        ext = p.per if p.split == INNER else p.U
        loop = "short" if ext <= (1 << p.sub) else "long"
    return Label(p.kernel, p.family, int(p.vec), p.lanes, p.split, p.regime, m.r1 > 1, (m.four if not m.col else m.k1 > 1),
                 m.col and p.sub > 1, p.trips > 1, loop)


FACTORS = Label._fields[2:]


def pairs(L):
    """every two factor values a label holds together, inside its (kernel, family)"""
    vals = L[2:]
    return {((L.kernel, L.family), FACTORS[i], vals[i], FACTORS[j], vals[j]) for i, j in itertools.combinations(range(len(vals)), 2)}


# What no shape reaches, with the arithmetic; tests/test_axes_cases.py holds each against the random walk.
UNREACHABLE = {
    # S <= ceil(1024 / items) and a split needs items < 1024, so nitem = items S < items (1024 / items + 1) = 1024 + items <= 2047 < MAX_WG
    # (row: a split is workgroup-wide, items = nout; column: col_split refuses nitem >= TARGET_ITEMS).  The walk's largest is 2032.
    "a split plan wraps": lambda p: p.S > 1 and p.trips > 1,
    # k_smax_merge folds 256 >> g groups a workgroup, g = log2_ceil(S, 6): nout <= 256 items (a tile holds at most 64 float4 columns) and
    # items <= 1023 / (S - 1), so S = 2: ceil(1023 * 256 / 128) = 2046; S in 3..4: 511 * 256 / 64 = 2044; ...; S > 32: 31 * 256 / 4 = 1984
    "the merge's grid-stride wraps": lambda p: p.regime == MULTI and merge_grid_items(p) > MAX_WG,
    # nout S <= 2047 floats (or 2 (S + 1) nout pairs) against 16 Mi floats: split_for's workspace term never decides at 64 MiB
    "the workspace caps a split at 64 MiB": lambda p: p.capped,
}


def merge_grid_items(p):
    return ceil_div(p.nout, BLK >> log2_ceil(p.S, 6))


# ---------------------------------------------------------------------------------------------------------------- the table
class R:
    """dim (N, H, W, C), mask, the eight fields each kernel's plan entry must report, the softmax regime and chunks"""

    def __init__(self, dim, mask, red, smx, regime, chunks, name=None):
        self.dim, self.mask, self.red, self.smx, self.regime, self.chunks = dim, mask, list(red), list(smx), regime, chunks
        self.id = "%s-%d" % ("x".join(str(e) for e in dim), mask)
        self.name = name or self.id
        self.size = int(np.prod(dim))

    def plan(self, kernel, aligned=True):
        return (reduce_plan if kernel == "reduce" else softmax_plan)(self.dim, self.mask, aligned)

    def want(self, kernel):
        return self.red if kernel == "reduce" else self.smx


TABLE = [
    # ---- the crossings no earlier test reached (tests/README.md "Axis kernels at every plan" names each)
    R((2100, 2, 1, 3),        4, (1, 1, 0, 2, 1, 1, 0, 2),  (1, 1, 0, 2, 1, 1, 0, 2),  0, 1, "column second trip, scalar"),
    R((2100, 2, 1, 260),      4, (1, 1, 1, 6, 2, 1, 0, 3),  (1, 1, 1, 6, 2, 1, 0, 3),  0, 1, "column second and third trip, float4, two tiles"),
    R((530000, 1, 3, 1),      2, (0, 1, 0, 0, 0, 1, 0, 2),  (0, 1, 0, 0, 0, 1, 0, 2),  0, 1, "row second trip, 256 groups a workgroup"),
    R((270000, 2, 2, 3),      5, (0, 1, 0, 0, 0, 1, 0, 2),  (0, 1, 0, 0, 0, 1, 0, 2),  0, 1, "row second trip, second kept group"),
    R((8200, 1, 1, 517),      1, (0, 1, 0, 6, 6, 1, 0, 2),  (0, 1, 0, 8, 8, 1, 0, 5),  0, 1, "row second trip, a wave per group (reduce)"),
    R((2100, 1, 1, 2049),     1, (0, 1, 0, 8, 8, 1, 0, 2),  (0, 1, 0, 8, 8, 1, 0, 2),  1, 2, "row second trip, a workgroup per group, ONLINE"),
    R((2100, 1, 1, 8196),     1, (0, 1, 1, 8, 8, 1, 0, 2),  (0, 1, 1, 8, 8, 1, 0, 2),  1, 2, "row second trip, float4, ONLINE"),
    R((1, 1000, 3, 5),        5, (0, 2, 0, 8, 3, 2, 2, 1),  (0, 3, 0, 8, 3, 2, 2, 1),  2, 2, "row split over the runs"),
    R((2, 1000, 3, 5),        5, (0, 2, 0, 8, 3, 2, 2, 1),  (0, 3, 0, 8, 3, 2, 2, 1),  2, 2, "row split over the runs, second kept group"),
    R((3, 1000, 2, 700),      5, (0, 2, 1, 8, 8, 84, 2, 1), (0, 3, 1, 8, 8, 84, 2, 1), 2, 2, "row split over the runs, float4, 84 parts"),
    R((40, 2, 3, 5),         10, (1, 2, 0, 3, 1, 10, 2, 1), (1, 3, 0, 3, 1, 10, 2, 1), 2, 1, "column split over r1"),
    R((3, 2, 2100, 64),      10, (1, 2, 1, 4, 1, 16, 1, 1), (1, 3, 1, 4, 1, 16, 1, 1), 2, 4, "column split over r0, r1 = 3, k1 = 2, 16 parts"),
    R((3, 2, 300, 64),       10, (1, 2, 1, 4, 1, 2, 1, 1),  (1, 3, 1, 4, 1, 2, 1, 1),  2, 4, "column split over r0, r1 = 3, k1 = 2, chunks 4"),
    R((3, 2, 40, 64),        10, (1, 1, 1, 4, 1, 1, 0, 1),  (1, 1, 1, 4, 1, 1, 0, 1),  1, 2, "column ONLINE, r1 = 3"),
    R((2, 3, 3, 683),         5, (0, 1, 0, 8, 8, 1, 0, 1),  (0, 1, 0, 8, 8, 1, 0, 1),  1, 2, "row ONLINE by the ceilings alone, four groups, r1 = 3"),
    R((1, 1, 1, 4097),        1, (0, 2, 0, 8, 8, 2, 1, 1),  (0, 3, 0, 8, 8, 2, 1, 1),  2, 2, "ragged last part"),
    # ---- the smallest shapes found for every other pair of factor values, by size
    R((4, 1, 1, 1),          15, (0, 1, 1, 0, 0, 1, 0, 1),  (0, 1, 1, 0, 0, 1, 0, 1),  0, 1),
    R((2, 1, 4, 1),          13, (1, 1, 1, 0, 1, 1, 0, 1),  (1, 1, 1, 0, 1, 1, 0, 1),  0, 1),
    R((8, 1, 1, 1),          12, (0, 1, 1, 1, 1, 1, 0, 1),  (0, 1, 1, 1, 1, 1, 0, 1),  0, 1),
    R((2, 1, 9, 1),           9, (1, 1, 0, 4, 1, 1, 0, 1),  (1, 1, 0, 4, 1, 1, 0, 1),  0, 1),
    R((1, 1, 2, 20),          2, (1, 1, 1, 3, 1, 1, 0, 1),  (1, 1, 1, 3, 1, 1, 0, 1),  0, 1),
    R((4, 4, 8, 4),           5, (0, 1, 1, 2, 0, 1, 0, 1),  (0, 1, 1, 2, 0, 1, 0, 1),  0, 1),
    R((2, 15, 7, 4),          5, (0, 1, 1, 4, 0, 1, 0, 1),  (0, 1, 1, 4, 0, 1, 0, 1),  0, 1),
    R((1, 1, 33, 33),        14, (1, 1, 0, 6, 1, 1, 0, 1),  (1, 1, 0, 6, 1, 1, 0, 1),  1, 2),
    R((65, 1, 17, 1),        12, (1, 1, 0, 5, 1, 1, 0, 1),  (1, 1, 0, 5, 1, 1, 0, 1),  1, 2),
    R((1, 257, 5, 1),         5, (1, 1, 0, 3, 1, 1, 0, 1),  (1, 1, 0, 3, 1, 1, 0, 1),  1, 2),
    R((5, 2, 2, 68),         10, (1, 1, 1, 5, 1, 1, 0, 1),  (1, 1, 1, 5, 1, 1, 0, 1),  0, 1),
    R((513, 1, 3, 1),        12, (1, 1, 0, 2, 1, 1, 0, 1),  (1, 1, 0, 2, 1, 1, 0, 1),  1, 2),
    R((9, 3, 4, 15),         10, (1, 2, 0, 4, 1, 2, 2, 1),  (1, 3, 0, 4, 1, 2, 2, 1),  2, 1),
    R((1, 1025, 1, 2),       12, (1, 1, 0, 1, 1, 1, 0, 1),  (1, 1, 0, 1, 1, 1, 0, 1),  1, 2),
    R((6, 11, 4, 8),          5, (0, 1, 1, 5, 1, 1, 0, 1),  (0, 1, 1, 5, 1, 1, 0, 1),  0, 1),
    R((33, 65, 1, 1),         9, (1, 1, 0, 6, 2, 1, 0, 1),  (1, 1, 0, 6, 2, 1, 0, 1),  1, 2),
    R((128, 17, 1, 1),        9, (1, 2, 0, 5, 1, 2, 1, 1),  (1, 3, 0, 5, 1, 2, 1, 1),  2, 1),
    R((1, 512, 5, 1),        12, (1, 2, 0, 3, 1, 2, 1, 1),  (1, 3, 0, 3, 1, 2, 1, 1),  2, 1),
    R((17, 5, 2, 17),        10, (1, 2, 0, 5, 1, 4, 2, 1),  (1, 3, 0, 5, 1, 4, 2, 1),  2, 1),
    R((1, 1, 1024, 3),       10, (1, 2, 0, 2, 1, 2, 1, 1),  (1, 3, 0, 2, 1, 2, 1, 1),  2, 1),
    R((15, 4, 7, 8),         10, (1, 2, 1, 1, 1, 3, 2, 1),  (1, 3, 1, 1, 1, 3, 2, 1),  2, 1),
    R((1, 2048, 2, 1),        5, (1, 2, 0, 1, 1, 2, 1, 1),  (1, 3, 0, 1, 1, 2, 1, 1),  2, 1),
    R((16, 4, 1, 65),        14, (1, 2, 0, 6, 2, 2, 1, 1),  (1, 3, 0, 6, 2, 2, 1, 1),  2, 1),
    R((2, 8, 9, 32),          5, (0, 1, 1, 6, 3, 1, 0, 1),  (0, 1, 1, 6, 3, 1, 0, 1),  0, 1),
    R((16, 9, 3, 12),        10, (1, 2, 1, 2, 1, 4, 2, 1),  (1, 3, 1, 2, 1, 4, 2, 1),  2, 1),
    R((2049, 2, 1, 2),        6, (1, 1, 0, 1, 1, 1, 0, 2),  (1, 1, 0, 1, 1, 1, 0, 2),  0, 1),
    R((376, 2, 3, 4),        10, (1, 2, 1, 0, 1, 94, 2, 1), (1, 3, 1, 0, 1, 94, 2, 1), 2, 1),
    R((9, 9, 2, 65),         10, (1, 2, 0, 6, 2, 2, 2, 1),  (1, 3, 0, 6, 2, 2, 2, 1),  2, 1),
    R((1, 1, 4096, 4),        6, (1, 2, 1, 0, 1, 2, 1, 1),  (1, 3, 1, 0, 1, 2, 1, 1),  2, 1),
    R((2049, 2, 1, 7),        4, (1, 1, 0, 3, 1, 1, 0, 2),  (1, 1, 0, 3, 1, 1, 0, 2),  0, 1),
    R((32, 2, 1, 512),       11, (0, 2, 1, 8, 6, 2, 1, 1),  (0, 3, 1, 8, 6, 2, 1, 1),  2, 1),
    R((9, 8, 127, 4),         5, (0, 1, 1, 3, 0, 1, 0, 1),  (0, 1, 1, 3, 0, 1, 0, 1),  0, 1),
    R((2100, 1, 2, 9),        6, (1, 1, 0, 4, 1, 1, 0, 2),  (1, 1, 0, 4, 1, 1, 0, 2),  0, 1),
    R((3, 4, 2, 2901),        5, (0, 2, 0, 8, 8, 5, 1, 1),  (0, 3, 0, 8, 8, 5, 1, 1),  2, 2),
    R((31, 68, 3, 17),        2, (1, 1, 0, 5, 1, 1, 0, 2),  (1, 1, 0, 5, 1, 1, 0, 2),  0, 1),
    R((260, 2, 257, 1),      11, (0, 2, 0, 8, 8, 29, 2, 1), (0, 3, 0, 8, 8, 29, 2, 1), 2, 3),
    R((256, 2, 257, 2),       5, (0, 1, 0, 1, 1, 1, 0, 1),  (0, 1, 0, 1, 1, 1, 0, 1),  0, 1),
    R((9, 2100, 5, 4),       10, (1, 1, 1, 0, 1, 1, 0, 2),  (1, 1, 1, 0, 1, 1, 0, 2),  1, 2),
    R((1, 1, 524300, 1),      1, (0, 1, 0, 0, 0, 1, 0, 2),  (0, 1, 0, 0, 0, 1, 0, 2),  0, 1),
    R((2, 4097, 128, 1),      9, (1, 1, 1, 6, 2049, 1, 0, 2), (1, 1, 1, 6, 2049, 1, 0, 2), 0, 1),
    R((8196, 32, 9, 1),       2, (0, 1, 0, 0, 0, 1, 0, 1),  (0, 1, 0, 1, 1, 1, 0, 2),  0, 1),
    R((2049, 1, 8, 257),      1, (0, 1, 0, 5, 5, 1, 0, 2),  (0, 1, 0, 6, 6, 1, 0, 3),  0, 1),
    R((8196, 4, 129, 1),      3, (0, 1, 0, 4, 4, 1, 0, 2),  (0, 1, 0, 5, 5, 1, 0, 3),  0, 1),
    R((4097, 16, 1, 65),      1, (0, 1, 0, 3, 3, 1, 0, 2),  (0, 1, 0, 4, 4, 1, 0, 3),  0, 1),
    R((2, 16, 4097, 33),      1, (0, 1, 0, 2, 2, 1, 0, 2),  (0, 1, 0, 3, 3, 1, 0, 3),  0, 1),
    R((1, 64, 4097, 17),      1, (0, 1, 0, 1, 1, 1, 0, 2),  (0, 1, 0, 2, 2, 1, 0, 3),  0, 1),
]
BY_ID = {r.id: r for r in TABLE}
KERNELS = ("reduce", "softmax")


def row(dim, mask):
    return BY_ID["%s-%d" % ("x".join(str(e) for e in dim), mask)]


def all_labels():
    """ALL_LABELS: what the table lands on, a label -> the ids of its rows"""
    out = {}
    for r in TABLE:
        for k in KERNELS:
            out.setdefault(label(r.plan(k)), []).append(r.id)
    return out


def all_pairs():
    out = set()
    for L in all_labels():
        out |= pairs(L)
    return out


# The crossings of more than two factors that must have a row of their own: (kernel, name, predicate on (plan, label)).
CROSSINGS = [
    ("reduce", "k_red_col second trip, scalar", lambda p, L: L.family == COL and L.wrap and not L.vec),
    ("reduce", "k_red_col second trip, float4, two tiles", lambda p, L: L.family == COL and L.wrap and L.vec and L.tiles),
    ("reduce", "k_red_row second trip, several groups a wave", lambda p, L: L.family == ROW and L.wrap and L.lanes < 6),
    ("reduce", "k_red_row second trip, second kept group", lambda p, L: L.family == ROW and L.wrap and L.second),
    ("reduce", "k_red_row second trip, a wave per group", lambda p, L: L.family == ROW and L.wrap and L.lanes == 6),
    ("reduce", "k_red_row second trip, a workgroup per group", lambda p, L: L.family == ROW and L.wrap and L.lanes == 8),
    ("reduce", "row split over the runs, short-run loop", lambda p, L: L.family == ROW and L.split == OUTER and L.loop == "short" and not L.second),
    ("reduce", "row split over the runs, second kept group", lambda p, L: L.family == ROW and L.split == OUTER and L.second),
    ("reduce", "row split over the runs, float4", lambda p, L: L.family == ROW and L.split == OUTER and L.vec),
    ("reduce", "row split over the units, ragged last part", lambda p, L: L.family == ROW and L.split == INNER and p.U % p.per != 0),
    ("reduce", "column split over r1", lambda p, L: L.family == COL and L.split == OUTER),
    ("reduce", "column split over r0 with r1 > 1 and k1 > 1", lambda p, L: L.family == COL and L.split == INNER and L.outer and L.second),
    ("softmax", "k_smax_col second trip, regime 0", lambda p, L: L.family == COL and L.wrap and L.regime == REG and not L.vec),
    ("softmax", "k_smax_col second trip, float4, two tiles", lambda p, L: L.family == COL and L.wrap and L.vec and L.tiles),
    ("softmax", "k_smax_col second trip, ONLINE", lambda p, L: L.family == COL and L.wrap and L.regime == ONLINE),
    ("softmax", "k_smax_row second trip, several groups a wave", lambda p, L: L.family == ROW and L.wrap and L.lanes < 6),
    ("softmax", "k_smax_row second trip, second kept group", lambda p, L: L.family == ROW and L.wrap and L.second),
    ("softmax", "k_smax_row second trip, ONLINE, chunks 2", lambda p, L: L.family == ROW and L.wrap and L.regime == ONLINE and not L.vec and p.chunks == 2),
    ("softmax", "k_smax_row second trip, ONLINE, float4", lambda p, L: L.family == ROW and L.wrap and L.regime == ONLINE and L.vec),
    ("softmax", "ONLINE, column, r1 > 1", lambda p, L: L.family == COL and L.regime == ONLINE and L.outer),
    ("softmax", "ONLINE, row, four groups, r1 > 1", lambda p, L: L.family == ROW and L.regime == ONLINE and L.outer and L.second),
    ("softmax", "PART / NORM, column split over r0, r1 > 1, k1 > 1", lambda p, L: L.family == COL and L.split == INNER and L.outer and L.second),
    ("softmax", "PART / NORM, column split over r1", lambda p, L: L.family == COL and L.split == OUTER),
    ("softmax", "PART / NORM, row split over the runs", lambda p, L: L.family == ROW and L.split == OUTER),
    ("softmax", "PART / NORM, row split over the units, ragged last part", lambda p, L: L.family == ROW and L.split == INNER and p.U % p.per != 0),
] + [(k, "row: fewer lanes along a run than in a group (su < shift)", lambda p, L: L.family == ROW and p.sub < p.lanes) for k in KERNELS] \
  + [(k, "row: every lane along the run (su == shift > 0)", lambda p, L: L.family == ROW and p.sub == p.lanes > 0) for k in KERNELS]


# ---------------------------------------------------------------------------------------------------------------- the random walk
POOL = [1, 1, 1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 31, 32, 33, 63, 64, 65, 68, 127, 128, 129, 255, 256, 257, 260, 511, 512, 513, 1023, 1024, 1025,
        2047, 2048, 2049, 2100, 4096, 4097, 8192, 8196, 16384, 40000, 70000, 270000, 530000, 1 << 20, 1 << 22]
WALK_LIMIT = 1 << 36                                                    # floats: about the MI355X's memory


def walk(seed, n, limit=WALK_LIMIT):
    """n draws of (dim, mask, aligned): extents from the thresholds' neighbourhoods or log-uniform, a third of them 1, any mask"""
    import random
    rnd = random.Random(seed)
    for _ in range(n):
        while True:
            d = [rnd.choice(POOL) for _ in range(4)] if rnd.random() < 0.6 else [max(1, int(2 ** rnd.uniform(0, 22))) for _ in range(4)]
            d = [1 if rnd.random() < 0.3 else e for e in d]
            if d[0] * d[1] * d[2] * d[3] <= limit:
                break
        yield tuple(d), rnd.randint(1, 15), rnd.random() < 0.6


# ---------------------------------------------------------------------------------------------------------------- numpy evaluations by plan
# An fp32 evaluation of a plan in numpy, in another order than the kernels' (NumPy's pairwise sums inside a part, the parts in index order),
# and the mutations the sweep has to notice.  tests/test_axes_cases.py runs them through the sweep's pass criteria.
def to_groups(x, m):
    """the tensor as [groups, r1, r0] (a copy), groups in dst order"""
    x = np.asarray(x)
    if m.col:
        return np.ascontiguousarray(x.reshape(m.r1, m.k1, m.r0, m.k0).transpose(1, 3, 0, 2)).reshape(m.k1 * m.k0, m.r1, m.r0)
    return np.ascontiguousarray(x.reshape(m.k1, m.r1, m.k0, m.r0).transpose(0, 2, 1, 3)).reshape(m.k1 * m.k0, m.r1, m.r0)


def from_groups(g, m, dim):
    if m.col:
        return np.ascontiguousarray(g.reshape(m.k1, m.k0, m.r1, m.r0).transpose(2, 0, 3, 1)).reshape(dim)
    return np.ascontiguousarray(g.reshape(m.k1, m.k0, m.r1, m.r0).transpose(0, 2, 1, 3)).reshape(dim)


def parts_of(p):
    """the (axis of [groups, r1, r0], begin, end) of every part, in elements"""
    if p.S == 1:
        return [(1, 0, p.m.r1)]
    if p.split == OUTER:
        return [(1, s * p.per, min(p.m.r1, (s + 1) * p.per)) for s in range(p.S)]
    V = 4 if (p.vec and not p.m.col) else 1                             # the row family deals float4 units of a run, the column family rows
    return [(2, s * p.per * V, min(p.m.r0, (s + 1) * p.per * V)) for s in range(p.S)]


def groups_beyond_first_trip(p):
    """the groups whose work items lie behind the first MAX_WG: what a single pass of the grid-stride loop never writes"""
    dead = np.zeros(p.nout, bool)
    if p.nitem <= MAX_WG:
        return dead
    assert p.S == 1
    if not p.m.col:
        dead[MAX_WG * (BLK >> p.lanes):] = True
        return dead
    V = 4 if p.vec else 1
    w = np.arange(MAX_WG, p.nitem)
    tile, ik1 = w % p.sub, w // p.sub
    for t, k in zip(tile, ik1):
        c0 = t * (V << p.lanes)
        dead[k * p.m.k0 + c0:k * p.m.k0 + min(p.m.k0, c0 + (V << p.lanes))] = True
    return dead


def _slice(g, part):
    ax, a, b = part
    return g[:, a:b, :] if ax == 1 else g[:, :, a:b]


SUM, NVAR, MAX, MIN = 0, 1, 2, 3                                        # include/t4k.h T4K_RED_*
# mutate: "drop_last_part", "single_trip", "twice" (both kernels); "merge_unscaled", "online_unscaled" (softmax)


def _twice_index(g):
    """[groups] the flat index inside the group of the element a mutated lane takes twice: the first that is not 0"""
    flat = g.reshape(g.shape[0], -1)
    return np.argmax(flat != 0, axis=1)


def reduce_by_plan(op, x, c, p, mutate=None):
    """t4k_reduce_axes as plan p lays it out, in fp32: [groups] in dst order"""
    f32 = np.float32
    g = to_groups(x, p.m)
    if op == NVAR:
        d = g - (np.asarray(c, f32).reshape(-1, 1, 1) if c is not None else f32(0))
        t = (d * d).astype(f32)
    else:
        t = g
    parts = parts_of(p)
    if mutate == "drop_last_part":
        assert p.S > 1
        parts = parts[:-1]
    fold = {SUM: lambda a: a.sum((1, 2), dtype=f32), NVAR: lambda a: a.sum((1, 2), dtype=f32), MAX: lambda a: a.max((1, 2)), MIN: lambda a: a.min((1, 2))}[op]
    acc = None
    for part in parts:
        v = fold(_slice(t, part))
        acc = v if acc is None else (np.maximum(acc, v) if op == MAX else np.minimum(acc, v) if op == MIN else (acc + v).astype(f32))
    if mutate == "twice":
        k = _twice_index(g)
        e = t.reshape(t.shape[0], -1)[np.arange(t.shape[0]), k]
        acc = np.maximum(acc, e) if op == MAX else np.minimum(acc, e) if op == MIN else (acc + e).astype(f32)
    acc = acc.astype(f32)
    if mutate == "single_trip":
        acc[groups_beyond_first_trip(p)] = np.nan                       # the prefill
    return acc


def softmax_by_plan(x, p, mutate=None):
    """t4k_softmax_axes as plan p lays it out, in fp32 and in the tensor's own layout.  Regime 0: max, exp, sum, divide.  Regime 1: a running
    (max, sum) over `chunks` slabs of the group.  Regime 2: a pair per part, the merge, the normalisation."""
    f32 = np.float32
    g = to_groups(x, p.m).astype(f32)
    G = g.shape[0]
    flat = g.reshape(G, -1)

    def pair(a):                                                        # a: [G, n] -> (max, sum exp(a - max))
        m = a.max(1)
        return m, np.exp(a - m[:, None], dtype=f32).sum(1, dtype=f32)

    def fold(pairs_, rescale):
        m, s = pairs_[0]
        for m2, s2 in pairs_[1:]:
            mn = np.maximum(m, m2)
            s = (s * np.exp(m - mn, dtype=f32) + s2 * np.exp(m2 - mn, dtype=f32)).astype(f32) if rescale else (s + s2).astype(f32)
            m = mn
        return m, s
    if p.regime == REG:
        m, s = pair(flat)
    elif p.regime == ONLINE:
        n = flat.shape[1]
        step = ceil_div(n, max(2, p.chunks))
        m, s = fold([pair(flat[:, a:a + step]) for a in range(0, n, step)], mutate != "online_unscaled")
    else:
        parts = parts_of(p)
        if mutate == "drop_last_part":
            parts = parts[:-1]
        m, s = fold([pair(_slice(g, part).reshape(G, -1)) for part in parts], mutate != "merge_unscaled")
    if mutate == "twice":
        k = _twice_index(g + f32(1e30))                                 # any element: the first
        s = (s + np.exp(flat[np.arange(G), k] - m, dtype=f32)).astype(f32)
    with np.errstate(over="ignore"):                                    # a mutated max may lie below an element
        out = (np.exp(flat - m[:, None], dtype=f32) / s[:, None]).astype(f32)
    if mutate == "single_trip":
        out[groups_beyond_first_trip(p)] = np.nan
    return from_groups(out.reshape(g.shape), p.m, x.shape)


# ---------------------------------------------------------------------------------------------------------------- operands and pass criteria
# What tests/test_gpu_axes_sweep.py feeds a row and how it judges the result: the operands and bounds of tests/test_gpu_reduce_axes.py and
# tests/test_gpu_softmax_axes.py, nothing new.  tests/test_axes_cases.py runs the evaluations above through the same functions.
def axes_of(mask):
    return tuple(i for i in range(4) if mask & (8 >> i))


def kept(dim, mask):
    return tuple(1 if mask & (8 >> i) else e for i, e in enumerate(dim))


def group_len(dim, mask):
    return int(np.prod([dim[i] for i in axes_of(mask)]))


def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def reduce_passes(dim, mask):
    """[(name, op, x, centre or None, exact)]: +-[0.5, 2) floats for the float64 bound (NVAR with a centre and with NULL), small integers
    whose every partial sum is exact in fp32 for bit equality: {-3 .. 3}, or {-1, 0, 1} where a group is too long for 16 a term"""
    import f64_witness as wt
    from test_gpu_bcast import operand
    rng, ks, cnt = _rng(dim, mask), kept(dim, mask), group_len(dim, mask)
    x = operand(rng, dim)
    c = (wt.f64(x).mean(axes_of(mask), keepdims=True) + rng.uniform(-0.25, 0.25, size=ks)).astype(np.float32)
    lo, hi = (-3, 4) if wt.is_int_exact(cnt, 16) else (-1, 2)
    assert wt.is_int_exact(cnt, max(abs(lo), abs(hi - 1) + 1) ** 2), (dim, mask, cnt)
    xi = rng.integers(lo, hi, size=dim).astype(np.float32)
    ci = rng.integers(0, 2, size=ks).astype(np.float32)
    out = [("float op %d" % op, op, x, c if op == NVAR else None, False) for op in (SUM, NVAR, MAX, MIN)]
    out.append(("float nvar NULL", NVAR, x, None, False))
    out += [("int op %d" % op, op, xi, ci if op == NVAR else None, True) for op in (SUM, NVAR, MAX, MIN)]
    out.append(("int nvar NULL", NVAR, xi, None, True))
    return out


def judge_reduce(name, op, x, mask, c, got, exact, kind=None):
    """AssertionError unless `got` ([kept] fp32) passes; returns the worst |error| / bound (0 for the exact passes)"""
    import f64_witness as wt
    from test_gpu_reduce_axes import witness
    assert not np.isnan(got).any(), "%s: %d outputs still hold the NaN prefill" % (name, int(np.isnan(got).sum()))
    w = witness(op, x, mask, c)
    if exact or op in (MAX, MIN):
        assert np.array_equal(np.asarray(got, np.float64).reshape(w.exact.shape), w.exact), "%s: %d outputs differ" % (name, int(np.sum(np.asarray(got, np.float64).reshape(w.exact.shape) != w.exact)))
        return 0.0
    return wt.check(name, got, w, kind=kind)


def softmax_passes(dim, mask):
    """[(name, x, exact)]: N(0, 2) logits, logits over +-1e4, and the constant tensor whose result is 1 / len bit for bit"""
    rng = _rng(dim, mask)
    return [("normal", (rng.standard_normal(dim) * 2.0).astype(np.float32), False), ("wide", rng.uniform(-1e4, 1e4, size=dim).astype(np.float32), False),
            ("constant", np.full(dim, 0.75, np.float32), True)]


def judge_softmax(name, x, mask, got, rescales, exact, kind=None):
    """as tests/test_gpu_softmax_axes.py run_case: check_values with `extra` from the plan's rescale count; the constant tensor bit for bit"""
    import f64_witness as wt
    from test_softmax_axes_words_oracle import check_values
    assert not np.isnan(got).any(), "%s: %d elements still hold the NaN prefill" % (name, int(np.isnan(got).sum()))
    if exact:
        L = group_len(x.shape, mask)
        assert L < 2 ** 24
        want = np.full(x.shape, np.float32(1) / np.float32(L), np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %d elements differ from 1 / %d" % (name, int(np.sum(got != want)), L)
        return
    ax, x64 = axes_of(mask), wt.f64(x)
    extra = 0.0 if rescales == 0 else rescales * (wt.ULP_EXP + 1.0) + 2.0 * (x64.max(ax, keepdims=True) - x64.min(ax, keepdims=True))
    mine, before = None, wt.WORST.pop("softmax", None)                  # check_values files its ratio under "softmax": refile it under `kind`
    try:
        check_values(name, x, mask, got, extra)
    finally:
        mine = wt.WORST.pop("softmax", None)
        if before is not None:
            wt.WORST["softmax"] = before
        if kind is not None and mine is not None and mine[0] > wt.WORST.get(kind, (-1.0, ""))[0]:
            wt.WORST[kind] = mine
