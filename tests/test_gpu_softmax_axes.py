"""t4k_softmax_axes (include/t4k.h, csrc/softmax_axes.hip) through the C ABI: softmax of every group along any subset of (N,H,W,C).

Three operands per case.  (1) N(0, 2) logits and (2) logits spread over +-1e4 (exp(x) itself would overflow), against f64_witness.softmax
after moving the masked axes last: |P_i - exact| <= (E_i + max_j E_j + len) u P_i with E_j = ULP_EXP + 2 |x_j - max| - the project's own
derived bound.  Every group's stored values sum to 1 within len u.  (3) a constant tensor: exp(0) = 1 and a sum of len ones are exact, so
every element must be np.float32(1) / np.float32(len) BIT FOR BIT in every regime - a dropped or doubled element changes the quotient,
and no share of the elements is excused.

The regimes (t4k_softmax_axes_plan reports the planner's choice, so the cases below name the regime they are meant to reach):
 0 a lane's share in registers: the arithmetic above exactly.
 1 two passes in one launch, 2 three launches: the terms of the sum are first formed against a running max m_1 <= max, exp(x_j - m_1)
   (error ULP_EXP + 2 |x_j - m_1| <= E_j ulps, as x_j <= m_1 <= max), and then multiplied R times by a factor exp(m_k - m_k+1): once per
   chunk of a lane's walk, once from the lane to its group, once (regime 2) from the part to the whole.  Each factor is one more __expf,
   ULP_EXP + 2 (m_k+1 - m_k) ulps, and one multiply, 1 ulp.  The maxima only rise, so the differences telescope to at most
   max - min of the group.  The per-element ulp count is therefore widened by R (ULP_EXP + 1) + 2 (max - min), R being the plan's count;
   nothing is fitted to the output.  The values stored are exp(x_i - max) / sum with the true max, as in regime 0.

Cases: all 15 masks on two odd shapes; the row family over group lengths around every lane-count switch, the float4 switch and the
register limit, with 1 and 3 outer runs; the column family over kept extents around the tile edges against 1, 2, 257 reduced rows; both
non-adjacent patterns; regime 1 and regime 2 in both families on the smallest shapes their thresholds admit; 70 000 groups of 3; buffers
4 bytes off 16-byte alignment; in place = out of place and two runs, bit for bit; the innermost axis of [N,C] against t4k_softmax; the
error returns."""
import ctypes
import zlib

import numpy as np
import pytest

import f64_witness as wt
from test_gpu_bcast import Dev, lcount
from test_softmax_axes_words_oracle import axes_of, check_values

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
I4 = ctypes.c_int * 4
I6 = ctypes.c_int * 6
REG, ONLINE, MULTI = 0, 1, 2


def plan(h, dim, mask, aligned=True):
    out = I6()
    h.call("t4k_softmax_axes_plan", I4(*dim), mask, int(aligned), out)
    return list(out)


def group_len(dim, mask):
    return int(np.prod([dim[i] for i in axes_of(mask)]))


def call(h, x, dim, mask, off=(0, 0), inplace=False, launches=None):
    dx = Dev(x, off[0])
    do = dx if inplace else Dev(np.full(x.size, np.nan, np.float32), off[1])
    l0 = lcount(h)
    h.call("t4k_softmax_axes", dx.p, do.p, I4(*dim), mask, None)
    n = lcount(h) - l0
    assert launches is None or n == launches, (dim, mask, n, launches)
    got = do.get(h, dim)
    flat = do.t.cpu().numpy()
    assert not flat[:do.off].any() and not flat[do.off + do.n:].any()   # nothing written in front of or behind dst
    if not inplace:
        assert np.array_equal(dx.get(h, dim), x)                        # src intact
    return got


def operands(dim, mask):
    rng = np.random.default_rng(zlib.crc32(repr((dim, mask)).encode()))
    return [("normal", (rng.standard_normal(dim) * 2.0).astype(np.float32)), ("wide", rng.uniform(-1e4, 1e4, size=dim).astype(np.float32))]


def run_case(h, dim, mask, off=(0, 0), regime=None, family=None):
    pl = plan(h, dim, mask, off[0] % 4 == 0 and off[1] % 4 == 0)
    assert regime is None or pl[1] == regime, (dim, mask, pl)
    assert family is None or pl[0] == family, (dim, mask, pl)
    launches = 3 if pl[1] == MULTI else 1
    ax = axes_of(mask)
    for name, x in operands(dim, mask):
        got = call(h, x, dim, mask, off, launches=launches)
        x64 = wt.f64(x)
        extra = 0.0 if pl[1] == REG else pl[5] * (wt.ULP_EXP + 1.0) + 2.0 * (x64.max(ax, keepdims=True) - x64.min(ax, keepdims=True))
        check_values("%s dim %s mask %d plan %s" % (name, dim, mask, pl), x, mask, got, extra)
    L = group_len(dim, mask)
    assert L < 2 ** 24
    got = call(h, np.full(dim, 0.75, np.float32), dim, mask, off, launches=launches)
    want = np.full(dim, np.float32(1) / np.float32(L), np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dim, mask, pl, int(np.sum(got != want)))
    return pl


@pytest.mark.parametrize("mask", range(1, 16))
@pytest.mark.parametrize("dim", [(3, 5, 7, 2), (2, 4, 6, 5)])
def test_every_mask(t4k, dim, mask):
    run_case(t4k, dim, mask)


@pytest.mark.parametrize("outer", [1, 3])
@pytest.mark.parametrize("r0", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 255, 256, 257, 1028])
def test_row_family_group_lengths(t4k, r0, outer):
    """the innermost axis masked: runs of r0 floats, `outer` of them per group (H and C masked, N and W kept); 2^k and 2^k + 1 floats
    sit either side of every lane-count switch of the scalar path"""
    run_case(t4k, (2, outer, 3, r0), 5, regime=REG, family=0 if r0 > 1 else None)    # r0 = 1: C drops out and W is the innermost group


@pytest.mark.parametrize("r0", [12, 20, 36, 68, 132, 260, 516, 1024])
def test_row_family_float4_lane_switches(t4k, r0):
    """4 (2^k + 1) floats: one float4 past every lane-count switch of the vector path"""
    assert run_case(t4k, (2, 1, 3, r0), 5, regime=REG, family=0)[2] == 1


@pytest.mark.parametrize("r0,regime", [(2047, REG), (2048, REG), (2049, ONLINE), (8188, REG), (8192, REG), (8196, ONLINE)])
def test_row_family_register_limit(t4k, r0, regime):
    """a workgroup per group holds 256 lanes x 8 loads: 2048 floats on the scalar path (odd lengths), 8192 on the float4 path"""
    run_case(t4k, (2, 1, 3, r0), 5, regime=regime, family=0)


@pytest.mark.parametrize("red", [1, 2, 257])
@pytest.mark.parametrize("k0", [1, 3, 4, 5, 64, 65, 260])
def test_column_family_kept_extents(t4k, k0, red):
    """the innermost axis kept: k0 contiguous columns, `red` rows in a group (H masked, N and C kept)"""
    run_case(t4k, (2, red, 1, k0), 4)


@pytest.mark.parametrize("dim", [(2, 300, 1, 5), (2, 1100, 1, 8)])
def test_column_family_two_passes_in_one_launch(t4k, dim):
    """more rows than a lane's registers hold, too few to split: scalar and float4 columns"""
    run_case(t4k, dim, 4, regime=ONLINE, family=1)


@pytest.mark.parametrize("mask", [10, 5])
def test_non_adjacent_patterns(t4k, mask):
    run_case(t4k, (3, 4, 5, 6), mask)


@pytest.mark.parametrize("dim,mask,family", [((1, 1, 1, 4097), 1, 0),          # row, scalar path: 2 x 2048 loads + 1, split along the run
                                             ((1, 1, 1, 16384), 1, 0),         # row, float4 path: 2 x 2048 loads
                                             ((2, 1000, 3, 5), 5, 0),          # row, runs shorter than their count: split over the runs
                                             ((1, 1, 1024, 3), 2, 1),          # column: 2 x 64 row groups x 8 rows, split over the rows
                                             ((40, 2, 3, 5), 10, 1)])          # column, the outer masked extent the longer one: split over it
def test_three_launch_regime_on_its_smallest_shapes(t4k, dim, mask, family):
    run_case(t4k, dim, mask, regime=MULTI, family=family)


def test_many_groups(t4k):
    run_case(t4k, (70000, 1, 3, 1), 2, regime=REG)


@pytest.mark.parametrize("off", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("dim,mask", [((2, 3, 4, 64), 1), ((2, 3, 4, 64), 14), ((1, 1, 5, 1028), 1), ((3, 257, 1, 8), 4)])
def test_buffers_four_bytes_off_alignment(t4k, dim, mask, off):
    """extents the float4 path would take: the scalar path when src or dst sits one float past a 16-byte boundary"""
    assert run_case(t4k, dim, mask, off=off)[2] == 0


BITS = [((3, 5, 7, 2), 6), ((2, 3, 3, 1028), 5), ((2, 1, 3, 2049), 5), ((1, 1, 1, 16384), 1), ((2, 257, 1, 64), 4), ((2, 300, 1, 5), 4), ((40, 2, 3, 5), 10)]


@pytest.mark.parametrize("dim,mask", BITS)
def test_in_place_equals_out_of_place_and_two_runs_agree_bit_for_bit(t4k, dim, mask):
    x = operands(dim, mask)[0][1]
    a = call(t4k, x, dim, mask)
    b = call(t4k, x, dim, mask)
    c = call(t4k, x, dim, mask, inplace=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("N,C", [(7, 10), (5, 64), (3, 257), (2, 1028)])
def test_innermost_axis_agrees_with_t4k_softmax(t4k, N, C):
    x = operands((1, 1, N, C), 1)[0][1]
    got = call(t4k, x, (1, 1, N, C), 1, launches=1)
    dx, do = Dev(x), Dev(np.zeros(x.size, np.float32))
    t4k.call("t4k_softmax", dx.p, do.p, N, C, None)
    ref = do.get(t4k, (1, 1, N, C))
    w = wt.softmax(x)
    wt.check("softmax_axes", got, w, kind="softmax"); wt.check("softmax", ref, w, kind="softmax")
    assert np.all(np.abs(wt.f64(got) - wt.f64(ref)) <= 2.0 * w.bound())


def test_error_returns(t4k):
    x = Dev(np.ones(64, np.float32)); o = Dev(np.zeros(64, np.float32))
    f = t4k.lib.t4k_softmax_axes
    dim = I4(2, 2, 4, 4)
    l0 = lcount(t4k)
    assert f(None, o.p, dim, 6, None) == ERR_ARG
    assert f(x.p, None, dim, 6, None) == ERR_ARG
    assert f(x.p, o.p, None, 6, None) == ERR_ARG
    for bad in [(0, 2, 4, 4), (2, -1, 4, 4), (2, 2, 0, 4), (2, 2, 4, 0)]:
        assert f(x.p, o.p, I4(*bad), 6, None) == ERR_ARG
    for mask in (0, 16, -1, 31):
        assert f(x.p, o.p, dim, mask, None) == ERR_ARG
    assert f(x.p, o.p, I4(1 << 11, 1 << 10, 1 << 10, 1 << 10), 6, None) == ERR_ARG                 # 2^41 elements
    # a partial overlap either way is refused; dst == src and dst right behind src are fine
    P = lambda d, k: ctypes.c_void_p(d.p.value + 4 * k)
    assert f(x.p, P(x, 8), I4(1, 2, 4, 4), 6, None) == ERR_ARG                                      # dst = x[8:40], src = x[0:32]
    assert f(P(x, 8), x.p, I4(1, 2, 4, 4), 6, None) == ERR_ARG
    assert lcount(t4k) == l0
    assert f(x.p, P(x, 32), I4(1, 2, 4, 4), 6, None) == OK                                         # src = x[0:32], dst = x[32:64]
    assert f(x.p, x.p, I4(1, 2, 4, 4), 6, None) == OK
    assert lcount(t4k) == l0 + 2
    assert np.array_equal(x.get(t4k, (64,)), np.full(64, 0.125, np.float32))                       # groups of 8 ones, both halves
