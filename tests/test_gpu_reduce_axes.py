"""t4k_reduce_axes (include/t4k.h, csrc/reduce_axes.hip) through the C ABI: SUM / NVAR / MAX / MIN along every subset of (N,H,W,C).

Two operands per case.  (1) +-[0.5, 2) floats against the exact value in float64 on the very fp32 operands (tests/f64_witness.py), within
C_SUM n 2^-24 mag + n 2^-126 - SUM: n = cnt, mag = sum |x|; NVAR: the exact value uses the fp32 centre that was passed, n = cnt + 2,
mag = sum (x - c)^2 - a bound that holds for ANY summation order, so nothing here is a measured tolerance; MAX / MIN bit for bit.
(2) small integers, whose sums are exact in fp32 in any order: SUM and NVAR bit for bit, so that no element can be left out or taken
twice however long the reduction is (the float bound of a million-term sum is wider than one element).

Cases: all 15 masks on two odd shapes; the row family over run lengths around every lane / float4 / workgroup boundary with 1 and 3
outer runs; the column family over kept extents around the tile edges against reduced extents 1, 2, 257; both non-adjacent patterns; the
two-stage paths; many outputs; a source 4 bytes off 16-byte alignment; determinism; mask 15 against t4k_reduce; the error returns."""
import ctypes
import zlib

import numpy as np
import pytest

import f64_witness as wt
from test_gpu_bcast import Dev, lcount, operand

pytestmark = pytest.mark.gpu

SUM, NVAR, MAX, MIN = 0, 1, 2, 3                                       # include/t4k.h T4K_RED_*
OPS = [SUM, NVAR, MAX, MIN]
OK, ERR_ARG = 0, -1
I4 = ctypes.c_int * 4


def axes_of(mask):
    return tuple(i for i in range(4) if mask & (8 >> i))


def kept(dim, mask):
    return tuple(1 if mask & (8 >> i) else e for i, e in enumerate(dim))


def witness(op, x, mask, c):
    ax, x64 = axes_of(mask), wt.f64(x)
    cnt = int(np.prod([x.shape[i] for i in ax]))
    if op == SUM:
        return wt.W(x64.sum(ax, keepdims=True), np.abs(x64).sum(ax, keepdims=True), cnt)
    if op == NVAR:
        d = x64 - (wt.f64(c) if c is not None else 0.0)
        return wt.W((d * d).sum(ax, keepdims=True), (d * d).sum(ax, keepdims=True), cnt + 2)
    return wt.W(x64.max(ax, keepdims=True) if op == MAX else x64.min(ax, keepdims=True), 0.0, 0)


def call(h, op, dx, dim, mask, dc, out_shape, launches=None):
    do = Dev(np.full(int(np.prod(out_shape)), np.nan, np.float32))
    l0 = lcount(h)
    h.call("t4k_reduce_axes", op, dx.p, do.p, I4(*dim), mask, dc.p if dc is not None else None, None)
    n = lcount(h) - l0
    assert n in (1, 2) if launches is None else n == launches, (dim, mask, n)
    got = do.get(h, out_shape)
    tail = do.t.cpu().numpy()
    assert not tail[do.n:].any()                                        # nothing written behind dst
    return got


def run_case(h, dim, mask, ops=OPS, off=0, launches=None, ints=(-3, 4)):
    rng = np.random.default_rng(zlib.crc32(repr((dim, mask)).encode()))
    ks = kept(dim, mask)
    # ---- floats against the float64 witness
    x = operand(rng, dim)
    c = (wt.f64(x).mean(axes_of(mask), keepdims=True) + rng.uniform(-0.25, 0.25, size=ks)).astype(np.float32)
    dx, dc = Dev(x, off), Dev(c)
    for op in ops:
        got = call(h, op, dx, dim, mask, dc if op == NVAR else None, ks, launches)
        wt.check("op %d dim %s mask %d" % (op, dim, mask), got, witness(op, x, mask, c))
        if op == NVAR:                                                  # NULL centre: sum x^2
            wt.check("nvar0 dim %s mask %d" % (dim, mask), call(h, op, dx, dim, mask, None, ks, launches), witness(op, x, mask, None))
    assert np.array_equal(dx.get(h, dim), x)                            # src intact
    # ---- small integers: every partial sum is exact, the result must be bit-equal
    lo, hi = ints
    xi = rng.integers(lo, hi, size=dim).astype(np.float32)
    ci = rng.integers(0, 2, size=ks).astype(np.float32)
    cnt = int(np.prod([dim[i] for i in axes_of(mask)]))
    assert wt.is_int_exact(cnt, max(abs(lo), abs(hi - 1) + 1) ** 2)
    dx, dc = Dev(xi, off), Dev(ci)
    for op in ops:
        got = call(h, op, dx, dim, mask, dc if op == NVAR else None, ks, launches)
        w = witness(op, xi, mask, ci)
        assert np.array_equal(got.astype(np.float64), w.exact), (op, dim, mask, int(np.sum(got != w.exact)))


@pytest.mark.parametrize("mask", range(1, 16))
@pytest.mark.parametrize("dim", [(2, 3, 4, 3), (3, 5, 7, 2)])
def test_every_mask(t4k, dim, mask):
    run_case(t4k, dim, mask)


@pytest.mark.parametrize("outer", [1, 3])
@pytest.mark.parametrize("r0", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1028])
def test_row_family_run_lengths(t4k, r0, outer):
    """the innermost axis reduced: runs of r0 floats, `outer` of them per output (H and C reduced, N and W kept)"""
    run_case(t4k, (2, outer, 3, r0), 5)


@pytest.mark.parametrize("red", [1, 2, 257])
@pytest.mark.parametrize("k0", [1, 3, 4, 5, 64, 65, 260])
def test_column_family_kept_extents(t4k, k0, red):
    """the innermost axis kept: k0 contiguous outputs, `red` rows folded (H reduced, N and C kept)"""
    run_case(t4k, (2, red, 1, k0), 4)


@pytest.mark.parametrize("mask", [10, 5])
def test_non_adjacent_patterns(t4k, mask):
    run_case(t4k, (3, 4, 5, 6), mask)


@pytest.mark.parametrize("dim,mask,ints", [((1, 1, 300000, 3), 2, (-3, 4)),      # column family: 3 outputs behind 300 000 rows
                                           ((1, 1, 1, 1 << 20), 1, (-1, 2))])    # row family: one output behind 2^20 floats
def test_two_stage_paths(t4k, dim, mask, ints):
    run_case(t4k, dim, mask, launches=2, ints=ints)


def test_many_outputs(t4k):
    run_case(t4k, (70000, 1, 3, 1), 2, launches=1)


@pytest.mark.parametrize("dim,mask", [((2, 3, 4, 64), 1), ((2, 3, 4, 64), 14), ((1, 1, 5, 1028), 1), ((3, 257, 1, 8), 4), ((1, 1, 1, 40000), 15)])
def test_source_four_bytes_off_alignment(t4k, dim, mask):
    """extents the float4 path would take: the scalar path when src sits one float past a 16-byte boundary"""
    run_case(t4k, dim, mask, off=1)


@pytest.mark.parametrize("dim,mask", [((3, 5, 7, 2), 6), ((1, 1, 300000, 3), 2), ((1, 1, 1, 1 << 20), 1), ((64, 33, 5, 3), 14)])
def test_same_call_twice_gives_identical_bits(t4k, dim, mask):
    rng = np.random.default_rng(2)
    x = rng.standard_normal(dim).astype(np.float32)
    dx = Dev(x)
    for op in (SUM, NVAR):
        a = call(t4k, op, dx, dim, mask, None, kept(dim, mask))
        b = call(t4k, op, dx, dim, mask, None, kept(dim, mask))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n", [1, 210, 4096, 100003, 1 << 20])
def test_mask_15_agrees_with_t4k_reduce(t4k, n):
    rng = np.random.default_rng(n)
    x = operand(rng, (1, 1, 1, n))
    dx, ds = Dev(x), Dev(np.zeros(1, np.float32))
    avg = np.float32(0.125)
    dc = Dev(np.array([avg], np.float32))
    for op in OPS:
        got = call(t4k, op, dx, (1, 1, 1, n), 15, dc if op == NVAR else None, (1, 1, 1, 1))
        t4k.call("t4k_reduce", op, dx.p, n, float(avg) if op == NVAR else 0.0, ds.p, None)
        ref = ds.get(t4k, (1,))
        w = witness(op, x, 15, np.array(avg) if op == NVAR else None)
        wt.check("reduce_axes op %d" % op, got, w); wt.check("reduce op %d" % op, ref, w)
        assert abs(float(got.ravel()[0]) - float(ref[0])) <= 2.0 * float(np.max(w.bound()))


def test_error_returns(t4k):
    x = Dev(np.ones(64, np.float32)); o = Dev(np.zeros(64, np.float32))
    f = t4k.lib.t4k_reduce_axes
    dim = I4(2, 2, 4, 4)
    l0 = lcount(t4k)
    assert f(SUM, None, o.p, dim, 6, None, None) == ERR_ARG
    assert f(SUM, x.p, None, dim, 6, None, None) == ERR_ARG
    assert f(SUM, x.p, o.p, None, 6, None, None) == ERR_ARG
    for bad in [(0, 2, 4, 4), (2, -1, 4, 4), (2, 2, 0, 4), (2, 2, 4, 0)]:
        assert f(SUM, x.p, o.p, I4(*bad), 6, None, None) == ERR_ARG
    for mask in (0, 16, -1, 31):
        assert f(SUM, x.p, o.p, dim, mask, None, None) == ERR_ARG
    for op in (-1, 4, 99):
        assert f(op, x.p, o.p, dim, 6, None, None) == ERR_ARG
    assert f(SUM, x.p, o.p, I4(1 << 11, 1 << 10, 1 << 10, 1 << 10), 6, None, None) == ERR_ARG      # 2^41 elements
    # dst inside src, dst ending inside src, dst == src; dst right behind src is fine
    P = lambda d, k: ctypes.c_void_p(d.p.value + 4 * k)
    assert f(SUM, x.p, P(x, 8), dim, 6, None, None) == ERR_ARG
    assert f(SUM, P(x, 4), P(x, 2), I4(1, 2, 4, 4), 6, None, None) == ERR_ARG                     # dst = x[2:6], src = x[4:36]
    assert f(SUM, x.p, x.p, dim, 6, None, None) == ERR_ARG
    assert lcount(t4k) == l0
    assert f(SUM, x.p, P(x, 32), I4(1, 2, 4, 4), 6, None, None) == OK                              # src = x[0:32], dst = x[32:36]
    assert lcount(t4k) == l0 + 1
    assert np.array_equal(x.get(t4k, (64,))[:32], np.ones(32, np.float32)) and np.array_equal(x.get(t4k, (64,))[32:36], np.full(4, 8.0, np.float32))
