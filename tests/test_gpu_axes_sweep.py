"""t4k_reduce_axes and t4k_softmax_axes (csrc/reduce_axes.hip, csrc/softmax_axes.hip) at every plan of their shared planner (csrc/axes.h), the plan asserted.

Every row of tests/axes_cases.py TABLE runs through both kernels.  Before anything is launched the eight fields of t4k_reduce_axes_plan /
t4k_softmax_axes_geometry (asked with ws_bytes = 0: the initialised library's own workspace) must equal the mirror's and the row's, the
regime and rescale count of t4k_softmax_axes_plan the mirror's, and the launch count of every call the plan's: a row off its label FAILS.

Criteria (tests/axes_cases.py judge_reduce / judge_softmax: the operands and bounds of tests/test_gpu_reduce_axes.py and
tests/test_gpu_softmax_axes.py, no new tolerance): reduce - +-[0.5, 2) floats inside f64_witness's c n 2^-24 mag for SUM and NVAR (a centre,
NULL), MAX / MIN bit for bit, small integers bit for bit in all four; softmax - N(0, 2) and +-1e4 logits inside check_values with `extra`
from the plan's rescale count, the constant tensor 1 / len bit for bit.  Every call: dst prefilled with NaN and free of it afterwards, four
guard floats in front of dst and four behind untouched, src bit-identical.

Further: buffers 4 bytes off alignment on rows whose aligned plan is float4; -inf logits in every regime of both families; library streams,
two of them at once, graph capture with three replays over new contents; a closed walk over all ordered pairs of six families that share
the stream workspace.  tests/README.md "Axis kernels at every plan" names the row behind every branch and quotes the measurements."""
import ctypes
import time

import numpy as np
import pytest

import axes_cases as ac
import f64_witness as wt
from test_gpu_bcast import Dev, lcount

pytestmark = pytest.mark.gpu

I4, I6, I8 = ctypes.c_int * 4, ctypes.c_int * 6, ctypes.c_int * 8
FRONT = 4                                                               # guard floats in front of a destination (16 bytes: the alignment stays)
CLOCK = {}
IDS = [r.id for r in ac.TABLE]


@pytest.fixture(scope="module", autouse=True)
def _clock():
    CLOCK.setdefault("t0", time.time())


def fields(h, kernel, dim, mask, aligned=True):
    out = I8()
    h.call("t4k_reduce_axes_plan" if kernel == "reduce" else "t4k_softmax_axes_geometry", I4(*dim), mask, int(aligned), ctypes.c_long(0), out)
    return list(out)


def asserted_plan(h, kernel, dim, mask, aligned=True, want=None):
    """the mirror's plan, equal to the library's report (and to the row's pinned fields)"""
    p = (ac.reduce_plan if kernel == "reduce" else ac.softmax_plan)(dim, mask, aligned)
    got = fields(h, kernel, dim, mask, aligned)
    assert got == p.fields(), (kernel, dim, mask, aligned, got, p)
    assert want is None or got == want, (kernel, dim, mask, got, want)
    if kernel == "softmax":
        out = I6()
        h.call("t4k_softmax_axes_plan", I4(*dim), mask, int(aligned), out)
        assert list(out) == [p.family, p.regime, int(p.vec), p.lanes, p.S, p.rescales], (dim, mask, list(out), p)
    return p


def kind_of(p):
    fam = "row" if p.family == ac.ROW else "column"
    return "axes: reduce %s%s" % (fam, ", two launches" if p.S > 1 else "") if p.kernel == "reduce" else "axes: softmax regime %d %s" % (p.regime, fam)


def put(d, a):
    """new contents into a device buffer that stays where it is"""
    import torch
    d.t[d.off:d.off + d.n].copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel()))
    torch.cuda.synchronize()


def fetch(h, d, shape, stream=None):
    """the buffer's contents after the stream's work; the guard floats around it still zero"""
    if stream is not None:
        h.call("t4k_sync", stream)
    got = d.get(h, shape)
    flat = d.t.cpu().numpy()
    assert not flat[:d.off].any() and not flat[d.off + d.n:].any(), "written outside the destination"
    return got


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def reduce_call(h, op, dx, dim, mask, dc, launches, stream=None, off=FRONT, do=None):
    ks = ac.kept(dim, mask)
    do = do or Dev(np.full(int(np.prod(ks)), np.nan, np.float32), off)
    l0 = lcount(h)
    h.call("t4k_reduce_axes", op, dx.p, do.p, I4(*dim), mask, dc.p if dc is not None else None, stream)
    assert lcount(h) - l0 == launches, (dim, mask, lcount(h) - l0, launches)
    return fetch(h, do, ks, stream)


def softmax_call(h, dx, dim, mask, launches, stream=None, off=FRONT, do=None):
    do = do or Dev(np.full(dx.n, np.nan, np.float32), off)
    l0 = lcount(h)
    h.call("t4k_softmax_axes", dx.p, do.p, I4(*dim), mask, stream)
    assert lcount(h) - l0 == launches, (dim, mask, lcount(h) - l0, launches)
    return fetch(h, do, dim, stream)


def run_reduce(h, dim, mask, p, off=0, stream=None, judge=True, passes=None):
    """every pass of a row through t4k_reduce_axes: {pass name: result}"""
    out, dev = {}, {}
    for name, op, x, c, exact in passes or ac.reduce_passes(dim, mask):
        dx = dev.setdefault(id(x), Dev(x, off))
        dc = dev.setdefault(id(c), Dev(c)) if c is not None else None
        got = reduce_call(h, op, dx, dim, mask, dc, p.launches, stream)
        if judge:
            ac.judge_reduce("%s dim %s mask %d %s" % (name, dim, mask, p.fields()), op, x, mask, c, got, exact, kind=kind_of(p))
        assert same_bits(dx.get(h, dim), x)                             # src intact
        out[name] = got
    return out


def run_softmax(h, dim, mask, p, off=(0, FRONT), stream=None, judge=True, passes=None):
    out = {}
    for name, x, exact in passes or ac.softmax_passes(dim, mask):
        dx = Dev(x, off[0])
        got = softmax_call(h, dx, dim, mask, p.launches, stream, off[1])
        if judge:
            ac.judge_softmax("%s dim %s mask %d %s regime %d" % (name, dim, mask, p.fields(), p.regime), x, mask, got, p.rescales, exact, kind=kind_of(p))
        assert same_bits(dx.get(h, dim), x)
        out[name] = got
    return out


# ----------------------------------------------------------------------------------------------------------------- every row of the table
@pytest.mark.parametrize("rid", IDS)
def test_reduce_row(t4k, rid):
    r = ac.BY_ID[rid]
    p = asserted_plan(t4k, "reduce", r.dim, r.mask, want=r.red)
    if p.S > 1:                                                         # stage two is the same planner on the partials: one launch, never split
        assert ac.reduce_stage_two(p).launches == 1
    run_reduce(t4k, r.dim, r.mask, p)


@pytest.mark.parametrize("rid", IDS)
def test_softmax_row(t4k, rid):
    r = ac.BY_ID[rid]
    p = asserted_plan(t4k, "softmax", r.dim, r.mask, want=r.smx)
    assert (p.regime, p.chunks) == (r.regime, r.chunks)
    run_softmax(t4k, r.dim, r.mask, p)


# ----------------------------------------------------------------------------------------------------------------- skewed bases
# one row per family and split kind whose aligned plan is float4
SKEW = [((6, 11, 4, 8), 5), ((32, 2, 1, 512), 11), ((3, 1000, 2, 700), 5), ((5, 2, 2, 68), 10), ((3, 2, 300, 64), 10), ((16, 9, 3, 12), 10)]


@pytest.mark.parametrize("dim,mask", SKEW)
def test_buffers_four_bytes_off_alignment(t4k, dim, mask):
    """src (and dst of the softmax) one float past a 16-byte boundary: the mirror's scalar plan, asserted; everything inside the criteria; the
    integer passes and the constant tensor bit-equal to the aligned run"""
    assert {(ac.row(d, m).plan("reduce").family, ac.row(d, m).plan("reduce").split) for d, m in SKEW} == {(f, s) for f in (0, 1) for s in (0, 1, 2)}
    pa, ps = asserted_plan(t4k, "reduce", dim, mask, True), asserted_plan(t4k, "reduce", dim, mask, False)
    assert pa.vec and not ps.vec and ps.family == pa.family
    a, s = run_reduce(t4k, dim, mask, pa, judge=False), run_reduce(t4k, dim, mask, ps, off=1)
    for name in a:
        if name.startswith("int"):
            assert same_bits(a[name], s[name]), name
    pa, ps = asserted_plan(t4k, "softmax", dim, mask, True), asserted_plan(t4k, "softmax", dim, mask, False)
    assert pa.vec and not ps.vec
    a = run_softmax(t4k, dim, mask, pa, judge=False)
    for off in ((1, FRONT + 1), (0, FRONT + 1), (1, FRONT)):
        s = run_softmax(t4k, dim, mask, ps, off=off)
        assert same_bits(a["constant"], s["constant"])


# ----------------------------------------------------------------------------------------------------------------- -inf logits
NINF = np.float32(-np.inf)
# (dim, mask, family, regime): r1 = 1 everywhere but the last two, so that a lane's walk is its units (row) or rows (column) in order
INF_SHAPES = [((2, 1, 3, 100), 1, ac.ROW, ac.REG), ((2, 7, 1, 5), 4, ac.COL, ac.REG), ((3, 1, 1, 3001), 1, ac.ROW, ac.ONLINE), ((1, 300, 1, 5), 4, ac.COL, ac.ONLINE),
              ((1, 1, 1, 4097), 1, ac.ROW, ac.MULTI), ((1, 1, 1024, 3), 2, ac.COL, ac.MULTI), ((2, 3, 3, 683), 5, ac.ROW, ac.ONLINE), ((3, 2, 300, 64), 10, ac.COL, ac.MULTI)]


def inf_masks(p, rng):
    """{configuration: bool [groups, r1, r0]} - where the logits are -inf; every group keeps a finite element"""
    m = p.m
    G, shape = m.k0 * m.k1, (m.k0 * m.k1, m.r1, m.r0)
    r, u = np.arange(m.r1)[None, :, None], np.arange(m.r0)[None, None, :]
    out = {"isolated": rng.random(shape) < 0.15}
    if p.family == ac.ROW:
        V = 4 if p.vec else 1
        Gu, Gr = 1 << p.sub, (1 << p.lanes) >> p.sub
        lane = ((u // V) % Gu == 1 % Gu) & (r % Gr == 0)                # the lane lu = 1 (0 where a run has one lane), lr = 0
        n_chunk = ac.NV * Gu * V                                        # every lane's first NV loads, the part's first when the units are split
    else:
        TY = ac.BLK >> p.lanes
        lane = (u % TY == 1 % TY) & (r >= 0)                            # the row group ty = 1, every column
        n_chunk = ac.NV * TY
    out["a lane's whole share"] = np.broadcast_to(lane, shape).copy()
    if p.regime != ac.REG and m.r1 == 1:
        out["every lane's first chunk"] = np.broadcast_to(u < n_chunk, shape).copy()
        last = (m.r0 - 1) // n_chunk * n_chunk
        out["every lane's last chunk"] = np.broadcast_to(u >= last, shape).copy()
    if p.regime == ac.MULTI:
        for name, part in (("the first part", ac.parts_of(p)[0]), ("the last part", ac.parts_of(p)[-1])):
            w = np.zeros(shape, bool)
            ac._slice(w, part)[...] = True
            out[name] = w
    single = np.zeros(shape, bool)
    single[G // 2] = True
    single[G // 2].flat[(m.r1 * m.r0) // 3] = False
    out["one group with a single finite element"] = single
    for name, w in out.items():
        for g in np.nonzero(w.reshape(G, -1).all(1))[0]:                # a group of nothing but -inf is unspecified: keep its middle element
            w[g].flat[(m.r1 * m.r0) // 2] = False
    return out


def check_finite_subset(name, x, got, p, kind):
    """-inf positions exactly +0; the finite positions of every group against f64_witness.softmax of the finite elements alone, with `extra`
    as tests/test_gpu_softmax_axes.py derives it; their stored values sum to 1 within count * 2^-24"""
    assert not np.isnan(got).any(), name
    gx, gg = ac.to_groups(x, p.m), ac.to_groups(got, p.m)
    gx, gg = gx.reshape(gx.shape[0], -1), gg.reshape(gx.shape[0], -1)
    dead = np.isneginf(gx)
    assert not gg[dead].view(np.uint32).any(), "%s: %d of %d -inf positions are not +0" % (name, int(np.count_nonzero(gg[dead].view(np.uint32))), int(dead.sum()))
    for g in range(gx.shape[0]):
        xf, gf = gx[g][~dead[g]], gg[g][~dead[g]]
        w = wt.softmax(xf[None, :])
        extra = 0.0 if p.rescales == 0 else p.rescales * (wt.ULP_EXP + 1.0) + 2.0 * (float(xf.max()) - float(xf.min()))
        wt.check("%s group %d" % (name, g), gf[None, :], wt.W(w.exact, w.mag, w.n + extra, 1.0), kind=kind)
        assert abs(wt.f64(gf).sum() - 1.0) <= xf.size * wt.U, (name, g)


@pytest.mark.parametrize("dim,mask,family,regime", INF_SHAPES)
def test_minus_infinity_logits_become_exact_zeros(t4k, dim, mask, family, regime):
    """include/t4k.h: -inf is admitted where the group keeps a finite element"""
    p = asserted_plan(t4k, "softmax", dim, mask)
    assert (p.family, p.regime) == (family, regime), p
    rng = ac._rng(dim, mask, "inf")
    base = (rng.standard_normal(dim) * 2.0).astype(np.float32)
    for name, where in inf_masks(p, rng).items():
        x = base.copy()
        x[ac.from_groups(where, p.m, dim)] = NINF
        assert np.isneginf(x).any() and np.isfinite(ac.to_groups(x, p.m)).reshape(where.shape[0], -1).any(1).all(), name
        for inplace in (False, True):
            dx = Dev(x, FRONT)
            got = softmax_call(t4k, dx, dim, mask, p.launches, do=dx if inplace else None)
            check_finite_subset("-inf %s dim %s mask %d%s" % (name, dim, mask, " in place" if inplace else ""), x, got, p, kind_of(p) + ", -inf")
            assert inplace or same_bits(dx.get(t4k, dim), x)


# ----------------------------------------------------------------------------------------------------------------- streams and capture
SINGLE, MULTI_ROW = ((2100, 2, 1, 3), 4), ((40, 2, 3, 5), 10)           # one wrapped launch; a column split over r1: two launches (reduce), three (softmax)


class stream:
    def __init__(self, h):
        self.h, self.s = h, ctypes.c_void_p()

    def __enter__(self):
        self.h.call("t4k_stream_create", ctypes.byref(self.s))
        return self.s

    def __exit__(self, *exc):
        self.h.call("t4k_sync", self.s)
        self.h.call("t4k_stream_destroy", self.s)


@pytest.mark.parametrize("dim,mask", [SINGLE, MULTI_ROW])
def test_on_a_library_stream(t4k, dim, mask):
    """the plan, the launch count (asserted by every call) and the bits of the default stream"""
    pr, ps = asserted_plan(t4k, "reduce", dim, mask), asserted_plan(t4k, "softmax", dim, mask)
    assert (pr.launches, ps.launches) == ((1, 1) if (dim, mask) == SINGLE else (2, 3))
    ref_r, ref_s = run_reduce(t4k, dim, mask, pr, judge=False), run_softmax(t4k, dim, mask, ps, judge=False)
    with stream(t4k) as s:
        assert fields(t4k, "reduce", dim, mask) == pr.fields() and fields(t4k, "softmax", dim, mask) == ps.fields()
        got_r, got_s = run_reduce(t4k, dim, mask, pr, stream=s), run_softmax(t4k, dim, mask, ps, stream=s)
    for k in ref_r:
        assert same_bits(ref_r[k], got_r[k]), k
    for k in ref_s:
        assert same_bits(ref_s[k], got_s[k]), k


def pair_operands(dim, mask, tag):
    rng = ac._rng(dim, mask, tag)
    return (rng.standard_normal(dim) * 2.0).astype(np.float32), rng.integers(-3, 4, size=dim).astype(np.float32)


def test_two_library_streams_at_once(t4k):
    """each stream: a three-launch softmax, then a two-stage reduction, on its own data and its own workspace; bit-equal to the serial results"""
    dim, mask = MULTI_ROW
    pr, ps = asserted_plan(t4k, "reduce", dim, mask), asserted_plan(t4k, "softmax", dim, mask)
    ks = ac.kept(dim, mask)
    data = [pair_operands(dim, mask, t) for t in ("a", "b")]
    serial = []
    for xs, xr in data:
        got_s = softmax_call(t4k, Dev(xs), dim, mask, 3)
        ac.judge_softmax("serial", xs, mask, got_s, ps.rescales, False)
        got_r = reduce_call(t4k, ac.SUM, Dev(xr), dim, mask, None, 2)
        ac.judge_reduce("serial", ac.SUM, xr, mask, None, got_r, True)
        serial.append((got_s, got_r))
    with stream(t4k) as s0, stream(t4k) as s1:
        bufs = [(Dev(xs), Dev(np.full(xs.size, np.nan, np.float32), FRONT), Dev(xr), Dev(np.full(int(np.prod(ks)), np.nan, np.float32), FRONT)) for xs, xr in data]
        l0 = lcount(t4k)
        for rounds in range(3):                                         # interleaved: both streams hold work at the same time
            for s, (dxs, dos, dxr, dor) in zip((s0, s1), bufs):
                t4k.call("t4k_softmax_axes", dxs.p, dos.p, I4(*dim), mask, s)
                t4k.call("t4k_reduce_axes", ac.SUM, dxr.p, dor.p, I4(*dim), mask, None, s)
        assert lcount(t4k) - l0 == 3 * 2 * (3 + 2)
        for s, (dxs, dos, dxr, dor), (want_s, want_r) in zip((s0, s1), bufs, serial):
            assert same_bits(fetch(t4k, dos, dim, s), want_s) and same_bits(fetch(t4k, dor, ks, s), want_r)


def test_graph_capture_replays_with_new_contents(t4k):
    """the three-launch softmax and the two-stage reduction captured once on a private stream (a linear graph) and replayed three times, new
    source contents uploaded into the same buffers before each: every replay gives that upload's result bit for bit - the pairs and the
    partials in the workspace are rewritten by each replay"""
    dim, mask = MULTI_ROW
    asserted_plan(t4k, "reduce", dim, mask); asserted_plan(t4k, "softmax", dim, mask)
    ks = ac.kept(dim, mask)
    uploads = [pair_operands(dim, mask, "replay %d" % i) for i in range(3)]
    want = [(softmax_call(t4k, Dev(xs), dim, mask, 3), reduce_call(t4k, ac.SUM, Dev(xr), dim, mask, None, 2)) for xs, xr in uploads]
    assert not same_bits(want[0][0], want[1][0]) and not same_bits(want[0][1], want[1][1])
    dxs, dxr = Dev(np.zeros(dim, np.float32)), Dev(np.zeros(dim, np.float32))
    dos, dor = Dev(np.full(dxs.n, np.nan, np.float32), FRONT), Dev(np.full(int(np.prod(ks)), np.nan, np.float32), FRONT)
    with stream(t4k) as s:
        g = ctypes.c_void_p()
        t4k.call("t4k_graph_begin", s)
        l0 = lcount(t4k)
        rc = [t4k.lib.t4k_softmax_axes(dxs.p, dos.p, I4(*dim), mask, s), t4k.lib.t4k_reduce_axes(ac.SUM, dxr.p, dor.p, I4(*dim), mask, None, s)]
        n = lcount(t4k) - l0
        t4k.call("t4k_graph_end", s, ctypes.byref(g))
        try:
            assert rc == [0, 0] and n == 5, (rc, n)
            assert np.isnan(fetch(t4k, dos, dim, s)).all()              # captured, not run
            for (xs, xr), (want_s, want_r) in zip(uploads, want):
                put(dxs, xs); put(dxr, xr); put(dos, np.full(dxs.n, np.nan, np.float32)); put(dor, np.full(dor.n, np.nan, np.float32))
                t4k.call("t4k_graph_launch", g, s)
                assert same_bits(fetch(t4k, dos, dim, s), want_s) and same_bits(fetch(t4k, dor, ks, s), want_r)
        finally:
            t4k.call("t4k_graph_destroy", g)


# ----------------------------------------------------------------------------------------------------------------- back to back on one stream
def test_plans_back_to_back_share_the_workspace(t4k):
    """six families in a closed walk over all 36 ordered pairs (a family after itself among them) on the default stream, nothing synchronised
    between two calls of a pair: five of them leave partials or pairs in the stream workspace, one is a wrapped single launch; every output
    is bit-equal to the family's solitary result, which passes the criteria"""
    fam = [("reduce", (1, 1, 1, 4097), 1, ac.ROW, ac.INNER), ("reduce", (1, 1000, 3, 5), 5, ac.ROW, ac.OUTER), ("reduce", (40, 2, 3, 5), 10, ac.COL, ac.OUTER),
           ("softmax", (1, 1, 1, 4097), 1, ac.ROW, ac.INNER), ("softmax", (1, 1, 1024, 3), 2, ac.COL, ac.INNER), ("reduce", (2100, 2, 1, 3), 4, ac.COL, ac.NONE)]
    state = []
    for i, (k, dim, mask, family, split) in enumerate(fam):
        p = asserted_plan(t4k, k, dim, mask)
        assert (p.family, p.split) == (family, split) and (p.trips > 1) == (split == ac.NONE), p
        xs, xr = pair_operands(dim, mask, "walk %d" % i)
        x = xs if k == "softmax" else xr
        dx = Dev(x)
        if k == "softmax":
            solo = softmax_call(t4k, dx, dim, mask, p.launches)
            ac.judge_softmax("solo", x, mask, solo, p.rescales, False)
            shape = dim
        else:
            solo = reduce_call(t4k, ac.SUM, dx, dim, mask, None, p.launches)
            ac.judge_reduce("solo", ac.SUM, x, mask, None, solo, True)
            shape = ac.kept(dim, mask)
        state.append((k, dim, mask, dx, shape, solo))
    n = len(fam)
    left = {a: list(range(n)) for a in range(n)}                        # Hierholzer on the complete digraph with loops
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if left[a]:
            stack.append(left[a].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == n * n + 1 and walk[0] == walk[-1] and {(a, b) for a, b in zip(walk, walk[1:])} == {(a, b) for a in range(n) for b in range(n)}
    outs = []
    for a in walk:
        k, dim, mask, dx, shape, solo = state[a]
        do = Dev(np.full(int(np.prod(shape)), np.nan, np.float32), FRONT)
        if k == "softmax":
            t4k.call("t4k_softmax_axes", dx.p, do.p, I4(*dim), mask, None)
        else:
            t4k.call("t4k_reduce_axes", ac.SUM, dx.p, do.p, I4(*dim), mask, None, None)
        outs.append((a, do))
    for step, (a, do) in enumerate(outs):
        assert same_bits(fetch(t4k, do, state[a][4]), state[a][5]), (step, fam[a])


def test_zz_report_worst_ratios_and_wall_time():
    """the worst |error| / bound per kernel, family and regime over the float passes above, and the file's wall time (pytest -s prints both;
    tests/README.md quotes them)"""
    print("\naxes sweep, worst |err| / bound:")
    for kind in sorted(k for k in wt.WORST if k.startswith("axes:")):
        print("  %-44s %.3g   %s" % (kind, wt.WORST[kind][0], wt.WORST[kind][1]))
        assert wt.WORST[kind][0] <= 1.0
    print("axes sweep wall time: %.1f s" % (time.time() - CLOCK.get("t0", time.time())))
