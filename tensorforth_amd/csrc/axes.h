// axes.h - what the kernels over a subset of the axes of a dense NHWC tensor share (reduce_axes.hip, softmax_axes.hip): the
// argument checks, the merge of (extents, mask) into at most four alternating groups, the two plans with their geometry, lane and split
// choices, and the step of a lane's walk.  The planner is plain host C++: it reads no library state, the caller passes the workspace size in.
// The kernels keep their own work-item decode and folds: shared forms of them changed the generated code (profiles/axes_shared_isa.txt).
#pragma once
#include "launch.h"

namespace {

using namespace t4k;

constexpr long TARGET_LANES = 64L * 4 * 256 * 2;   // two waves on every SIMD of 256 CUs: below this a group gets more lanes
constexpr long TARGET_ITEMS = 1024;                // workgroups a split aims for: four on every CU
constexpr long SPLIT_UNITS  = 8;                   // loads a lane keeps at least when a group is split across workgroups
constexpr long MAX_SPLIT    = 4096;

inline unsigned log2_ceil(long x, unsigned cap) { unsigned k = 0; while (k < cap && (1L << k) < x) k++; return k; }
inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// ---- row family: the innermost merged group is reduced.  Group o (one output of a reduction) is r1 runs (sr1 apart) of r0 contiguous
// floats starting at base(o) = o * sk0, or (o / k0) * sk1 + (o % k0) * sk0 when a second kept group lies outside the runs.  1 << shift lanes
// share a group (shift 0..5: several groups per wave, 6: a wave per group, 8: a workgroup per group), 1 << su of them side by side along a
// run and the rest over the runs.  S > 1: the units of a run (split_u) or the runs are dealt to S workgroups of `per` each.
struct RowPlan {
    long nout, U, r1;             // groups, units per run (r0 / 4 float4s on the vector path, else r0), runs per group
    long sk0, sr1, sk1, per, nitem;
    unsigned k0, shift, su, S;
    int four, split_u;
};

// ---- column family: the innermost merged group (k0 floats) is kept.  A workgroup iteration takes one tile of TX = 1 << sx lanes along k0
// (one column a lane, four on the vector path: every load of a wave is a contiguous run, also for k0 = 3 or 64) of one outer kept index;
// its 256 >> sx row groups deal the reduced rows (r0 of them sr0 apart, inside r1 of them sr1 apart) among themselves.  S > 1: the rows (or
// the outer reduced extent, split_r1) are dealt to S workgroups of `per` each.
struct ColPlan {
    long k0, r0, r1, sr0, sk1, sr1, per, nitem, nout;
    unsigned sx, ntile, S;
    int split_r1;
};

// ---- host: arguments, merge, geometry, lanes, split

// the checks both entries make on (dim, mask); `total` = the element count
inline int check_axes(const int dim[4], int mask, const char *who, long *total) {
    if (!dim) return fail(T4K_ERR_ARG, "%s: null", who);
    if (mask < 1 || mask > 15) return fail(T4K_ERR_ARG, "%s: mask %d outside 1..15", who, mask);
    *total = 1;
    for (int i = 0; i < 4; i++) {
        if (dim[i] < 1) return fail(T4K_ERR_ARG, "%s: extent %d", who, dim[i]);
        if (*total > (1L << 40) / dim[i]) return fail(T4K_ERR_ARG, "%s: more than 2^40 elements", who);
        *total *= dim[i];
    }
    return T4K_OK;
}

// axes of extent 1 drop out, neighbours that are both kept or both masked merge: at most four alternating groups, innermost first r0 k0 r1 k1
// (row family, `four` when k1 is there) or k0 r0 k1 r1 (column family); absent groups are 1.  k0 * k1 groups of r0 * r1 elements.
struct Merged { bool col, four; long r0, k0, r1, k1; };
inline int merge_axes(const int dim[4], int mask, const char *who, Merged &m) {
    long e[5]; bool red[5]; int n = 0; bool any = false;
    for (int i = 0; i < 4; i++) {
        if (dim[i] == 1) continue;
        const bool r = (mask & (8 >> i)) != 0;
        any = any || r;
        if (n && red[n - 1] == r) e[n - 1] *= dim[i];
        else { e[n] = dim[i]; red[n] = r; n++; }
    }
    if (!any) { e[n] = 1; red[n] = true; n++; }                              // only axes of extent 1 are masked: every element is its own group
    auto at = [&](int back) { return n >= back ? e[n - back] : 1; };
    m.col = !red[n - 1]; m.four = n == 4;
    if (m.col) { m.k0 = at(1); m.r0 = at(2); m.k1 = at(3); m.r1 = at(4); }
    else       { m.r0 = at(1); m.k0 = at(2); m.r1 = at(3); m.k1 = at(4); }
    if (!m.col && m.k0 > 0xffffffffL) return fail(T4K_ERR_ARG, "%s: merged extent too large", who);   // RowPlan::k0 is a 32-bit divisor
    return T4K_OK;
}

// vec: a unit is a float4 (every run starts on a multiple of r0 elements, every row on a multiple of k0: the caller checks the pointers)
inline void row_geometry(RowPlan &p, const Merged &m, bool vec) {
    p = RowPlan{};
    p.nout = m.k0 * m.k1; p.U = vec ? m.r0 >> 2 : m.r0; p.r1 = m.r1; p.k0 = (unsigned)m.k0; p.four = m.four;
    p.sk0 = m.r0; p.sr1 = m.r0 * m.k0; p.sk1 = m.r0 * m.k0 * m.r1;
    p.S = 1;
}
// nitem is left at the tiles: col_split multiplies the parts in
inline void col_geometry(ColPlan &p, const Merged &m, bool vec) {
    p = ColPlan{};
    p.k0 = m.k0; p.r0 = m.r0; p.r1 = m.r1; p.sr0 = m.k0; p.sk1 = m.k0 * m.r0; p.sr1 = m.k0 * m.r0 * m.k1; p.nout = m.k0 * m.k1;
    const long Uk = vec ? m.k0 >> 2 : m.k0;
    p.sx = log2_ceil(Uk, 6);
    p.ntile = (unsigned)ceil_div(Uk, 1L << p.sx);
    p.nitem = m.k1 * p.ntile;
    p.S = 1;
}
// lanes per group (the shift) for T loads behind each of nout groups: a lane should have loads_per_lane of them, unless that leaves the device short of lanes
inline unsigned row_lanes(long T, long loads_per_lane, long nout) {
    unsigned shift = log2_ceil(ceil_div(T, loads_per_lane), 8);
    const unsigned cap = log2_ceil(T, 8);
    while (shift < cap && (nout << shift) < TARGET_LANES) shift++;
    if (shift == 7) shift = (nout << 6) >= TARGET_LANES ? 6 : 8;             // a wave or a workgroup: nothing between
    return shift;
}
// how many workgroups share one group: enough for TARGET_ITEMS, never leaving a lane fewer than SPLIT_UNITS loads (max_by_work), never more
// parts of floats_per_part floats, beside parts_reserved further ones, than a workspace of ws_floats holds
inline long split_for(long items, long max_by_work, long floats_per_part, long parts_reserved, long ws_floats) {
    long S = std::min(std::min(ceil_div(TARGET_ITEMS, items), max_by_work), MAX_SPLIT);
    S = std::min(S, ws_floats / floats_per_part - parts_reserved);
    return S < 2 ? 1 : S;
}
// an extent dealt to about S parts: `per` each, and the parts that leaves
inline void split_extent(long ext, long S, long &per, unsigned &S_out) { per = ceil_div(ext, S); S_out = (unsigned)ceil_div(ext, per); }
// the split of a workgroup-wide row plan (shift == 8) along the longer of run and runs, of a column plan along the longer of rows and outer
// extent; false: one workgroup per group stays
inline bool row_split(RowPlan &p, long floats_per_group, long parts_reserved, long ws_floats) {
    const long S = split_for(p.nout, p.U * p.r1 / (BLK * SPLIT_UNITS), floats_per_group * p.nout, parts_reserved, ws_floats);
    if (S < 2) return false;
    p.split_u = p.U >= p.r1;
    split_extent(p.split_u ? p.U : p.r1, S, p.per, p.S);
    return true;
}
inline bool col_split(ColPlan &p, long floats_per_group, long parts_reserved, long ws_floats) {
    if (p.nitem >= TARGET_ITEMS) return false;
    const bool by_r1 = p.r1 > p.r0;
    const long S = split_for(p.nitem, by_r1 ? p.r1 / 4 : p.r0 / ((BLK >> p.sx) * SPLIT_UNITS), floats_per_group * p.nout, parts_reserved, ws_floats);
    if (S < 2) return false;
    p.split_r1 = by_r1;
    split_extent(by_r1 ? p.r1 : p.r0, S, p.per, p.S);
    p.nitem *= p.S;
    return true;
}

// ---- host: what t4k_reduce_axes_plan and t4k_softmax_axes_geometry report

// the workspace a plan entry plans for, in floats: ws_bytes > 0 as given (no device, no t4k_init), 0 the initialised library's own
inline int plan_workspace(long ws_bytes, const char *who, long *ws_floats) {
    if (ws_bytes < 0) return fail(T4K_ERR_ARG, "%s: ws_bytes %ld", who, ws_bytes);
    if (ws_bytes == 0) {
        if (!st().ready) return fail(T4K_ERR_NODEVICE, "%s: ws_bytes 0 asks for the library's workspace: t4k_init not called or no gfx950 device", who);
        ws_bytes = (long)st().ws_bytes;
    }
    *ws_floats = ws_bytes / (long)sizeof(float);
    return T4K_OK;
}
// out = { family, launches, float4 path, shift | sx, su | ntile, parts, split extent (0 none, 1 U | r0, 2 r1), trips of the grid-stride loop }
inline void report_plan(int out[8], const RowPlan &p, bool vec, int launches) {
    out[0] = 0; out[1] = launches; out[2] = vec ? 1 : 0; out[3] = (int)p.shift; out[4] = (int)p.su; out[5] = (int)p.S;
    out[6] = p.S > 1 ? (p.split_u ? 1 : 2) : 0; out[7] = (int)ceil_div(p.nitem, (long)MAX_WG);
}
inline void report_plan(int out[8], const ColPlan &p, bool vec, int launches) {
    out[0] = 1; out[1] = launches; out[2] = vec ? 1 : 0; out[3] = (int)p.sx; out[4] = (int)p.ntile; out[5] = (int)p.S;
    out[6] = p.S > 1 ? (p.split_r1 ? 2 : 1) : 0; out[7] = (int)ceil_div(p.nitem, (long)MAX_WG);
}

// ---- device

// one step of a lane's walk over its units, two counters and no division: `in` goes on by in_step, at in_end back to the lane's first (in0)
// with `out` one out_step further
__device__ __forceinline__ void walk_step(long &out, long &in, long in0, long in_end, unsigned in_step, unsigned out_step) {
    in += in_step;
    if (in >= in_end) { in = in0; out += out_step; }
}

}
