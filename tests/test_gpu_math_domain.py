"""t4k_math (elementwise.hip, k_math<OP>) over the whole domain of each of its 21 ops, element by element against float64 (wt.math): the
clamps of LN / LOG and SQRT, __expf towards overflow and underflow, SIGM where expf(-a) overflows, TANH where it saturates and where
tanh x = x, LN next to 1, POW with negative and zero bases and nine exponents, SIN / COS out to 3e38, GFILL past 2^24, subnormal operands
and results, NaN / inf / 0 in every op.  Tables: small_kernel_cases.MATH_DOMAIN and MATH_SPECIALS; every table is laid out with its edge
values in the float4 body and again in the scalar tail (n % 4 == 3) and runs from a 16-byte aligned base and from one 4 bytes off (the
scalar path throughout).  The binary entries (t4k_tt_op / t4k_tt_op2 / t4k_ts_op) run on the pairs of the specials, k_activate on
linspace(-104, 104) and the specials.  Every buffer lies between guard words that must come back unchanged, every call is one launch.
The CPU half (tests/test_f64_witness.py) holds libm and NumPy float32 to the same witness on the same tables and fails the defects."""
import ctypes
import functools

import numpy as np
import pytest

import f64_witness as wt
import small_kernel_cases as sk
from test_gpu_gemm_sweep import call
from test_gpu_parity import Dev, p
from test_gpu_small_kernels_sweep import launches

pytestmark = pytest.mark.gpu

SIN, COS = 25, 26                            # include/t4k.h T4K_SIN / T4K_COS: the oracle's enum stops at DIV, as the reference's switch does
GUARD = 8                                    # words behind every buffer (and `off` words in front of it)
SENTINEL = np.uint32(0x7FC5A5A5)             # a NaN with a payload: no op of this file produces it
MEASURED = {}                                # op -> worst |got - exact| / (2^-24 |exact|) of POW / SIN / COS over their tables
BIN_OPS = ("ADD", "SUB", "MUL", "DIV")


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


def code(oracle, op):
    return {"SIN": SIN, "COS": COS}[op] if op in ("SIN", "COS") else getattr(oracle, op)


def up_guard(dev, a, off):
    """`a` uploaded `off` elements into a 16-byte aligned buffer of guard words: (tensor, pointer of a[0])"""
    a = np.ascontiguousarray(a, np.float32).ravel(); buf = np.full(a.size + off + GUARD, SENTINEL, np.uint32).view(np.float32); buf[off:off + a.size] = a
    t = dev.up(buf)
    assert p(t) % 16 == 0
    return t, p(t) + 4 * off


def dn_guard(dev, t, off, n):
    """the n elements behind the front guard; the guard words in front and behind must be what was uploaded"""
    call(dev.h, "t4k_sync", None)                                             # (a device fault ends the session here: test_gpu_gemm_sweep.call)
    g = dev.down(t); bits = g.view(np.uint32)
    assert np.all(bits[:off] == SENTINEL) and np.all(bits[off + n:] == SENTINEL) and bits.size == off + n + GUARD, "guard words overwritten"
    return g[off:off + n]


def same_bits(got, want):
    """bit for bit, a NaN matching any NaN"""
    ok = ~np.isnan(want)
    return bool(np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)) and np.all(np.isnan(got[~ok])))


def run_math(t4k, dev, oracle, op, x, v, off):
    t, ptr = up_guard(dev, x, off); l0 = launches(t4k)
    call(t4k, "t4k_math", code(oracle, op), ptr, float(v), x.size, None)
    assert launches(t4k) - l0 == 1, (op, x.size)
    return dn_guard(dev, t, off, x.size)


@functools.lru_cache(maxsize=None)
def witness(k):
    c = sk.MATH_DOMAIN[k]
    return wt.math(c.op, np.zeros(c.n, np.float32) if c.x is None else c.x, c.v, c.n)


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("k", range(len(sk.MATH_DOMAIN)), ids=[c.id for c in sk.MATH_DOMAIN])
def test_math_op_over_its_domain(t4k, dev, oracle, k, off):
    c = sk.MATH_DOMAIN[k]; w = witness(k)
    got = run_math(t4k, dev, oracle, c.op, np.zeros(c.n, np.float32) if c.x is None else c.x, c.v, off)
    if c.op in ("POW", "SIN", "COS"):                                          # the figure ULP_POW / ULP_SIN / ULP_COS are set from, before it is held to them
        with np.errstate(all="ignore"):
            u = np.abs(got.astype(np.float64) - w.exact) / (wt.U * np.abs(w.exact))
        u = np.where(np.isfinite(u) & (np.abs(w.exact) >= wt.TINY), u, 0.0)    # (below FLT_MIN the n 2^-126 term holds a result, not its ulps)
        i = int(np.argmax(u)); MEASURED[c.op] = max(MEASURED.get(c.op, 0.0), float(u[i]))
        print("\n%s off=%d: worst %.5f ulps of |exact| at x = %r" % (c.id, off, float(u[i]), float(c.x[i])))
    wt.check("%s off=%d" % (c.id, off), got, w, kind="math " + c.op)
    if c.op in wt.MATH_EXACT + ("GFILL",) and c.op not in ("RELU", "SAT", "SQRT"):
        assert same_bits(got, w.f32), c.id                                      # ... the sign of a zero included (fmaxf(-0, 0) of the three guards may return either)


SPECIAL_RUNS = tuple((op, v) for op in wt.MATH_OPS for v in ((1.5, 3.0, -1.0) if op == "POW" else (1.5,)))


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("op,v", SPECIAL_RUNS, ids=["%s-v%g" % r for r in SPECIAL_RUNS])
def test_math_specials(t4k, dev, oracle, op, v, off):
    """NaN, +-inf, +-0, the subnormals, FLT_MIN, +-FLT_MAX, +-1 through every op.  Expected: the oracle's t4o_math (libm), the witness for
    SIN / COS (sin(inf) = NaN).  NaN matches NaN and an infinity the infinity of its sign; zeros match whatever their sign, because
    fmaxf(-0, 0) is free to return either; finite values are held to the op's witness.  This pins what the clamps do with a NaN: LN / LOG
    return the clamp's log, SQRT / RELU / SAT return 0 (include/t4k.h says so)."""
    x = sk.MATH_SPECIALS_ROW; w = wt.math(op, x, v)
    got = run_math(t4k, dev, oracle, op, x, v, off)
    if op in ("SIN", "COS"):
        want = w.exact
    else:
        want = x.copy(); assert oracle.lib().t4o_math(getattr(oracle, op), oracle.P(want), float(v), want.size) == 0
    assert np.array_equal(wt.kinds(got), wt.kinds(want)), (op, got, want)
    wt.check("specials %s v=%g off=%d" % (op, v, off), got, w, kind="math specials")
    if op in ("LN", "LOG"):
        assert abs(float(got[0]) - float(w.exact[0])) <= wt.ULP_LOG * wt.U * abs(float(w.exact[0])) and w.exact[0] < -11.9
    if op in ("SQRT", "RELU", "SAT"):
        assert got[0] == 0


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("op", BIN_OPS)
def test_binary_entries_on_the_pairs_of_the_specials(t4k, dev, oracle, op, off):
    """t4k_tt_op, t4k_tt_op2 (both destinations) and t4k_ts_op on the 12 x 12 pairs (and three more: the scalar tail): bit-equal to NumPy
    float32, a NaN matching a NaN"""
    s = sk.MATH_SPECIALS; a = np.concatenate([np.repeat(s, s.size), s[:3]]); b = np.concatenate([np.tile(s, s.size), s[-3:]]); n = a.size
    assert n % 4 == 3
    f = {"ADD": np.add, "SUB": np.subtract, "MUL": np.multiply, "DIV": np.divide}[op]; c = getattr(oracle, op)
    with np.errstate(all="ignore"):
        want = f(a, b)
    (ta, pa), (tb, pb), (t1, p1), (t2, p2) = up_guard(dev, a, off), up_guard(dev, b, off), up_guard(dev, np.full(n, 7, np.float32), off), up_guard(dev, np.full(n, 7, np.float32), off)
    l0 = launches(t4k); call(t4k, "t4k_tt_op2", c, pa, pb, p1, p2, n, None); assert launches(t4k) - l0 == 1
    assert same_bits(dn_guard(dev, t1, off, n), want) and same_bits(dn_guard(dev, t2, off, n), want), op
    t1, p1 = up_guard(dev, np.full(n, 7, np.float32), off)
    l0 = launches(t4k); call(t4k, "t4k_tt_op", c, pa, pb, p1, n, None); assert launches(t4k) - l0 == 1
    assert same_bits(dn_guard(dev, t1, off, n), want), op
    outs = []
    for v in s:
        t1, p1 = up_guard(dev, np.full(n, 7, np.float32), off)
        l0 = launches(t4k); call(t4k, "t4k_ts_op", c, pa, float(v), p1, n, None); assert launches(t4k) - l0 == 1
        outs.append(t1)
    for v, t1 in zip(s, outs):
        with np.errstate(all="ignore"):
            assert same_bits(dn_guard(dev, t1, off, n), f(a, v)), (op, v)
    assert same_bits(dn_guard(dev, ta, off, n), a) and same_bits(dn_guard(dev, tb, off, n), b)          # operands untouched


@pytest.mark.parametrize("off", (0, 1))
@pytest.mark.parametrize("kind,alpha", sk.ACT_DOMAIN_KINDS, ids=[k for k, _ in sk.ACT_DOMAIN_KINDS])
def test_activations_out_to_the_saturation_of_exp(t4k, dev, oracle, kind, alpha, off):
    """k_activate on linspace(-104, 104) (the other sweeps stop near |x| = 15): output and mask through wt.act as it stands; then on the
    specials: NaN / infinities as t4o_activate gives them (the comparison of test_math_specials), finite values through wt.act"""
    L = getattr(oracle, {"leaky": "L_LEAKYRL"}.get(kind, "L_" + kind.upper())); o = oracle.lib(); P = oracle.P
    for x, specials in ((sk.ACT_DOMAIN, False), (sk.MATH_SPECIALS_ROW, True)):
        n = x.size
        (tx, px), (ty, py), (tf, pf) = up_guard(dev, x, off), up_guard(dev, np.zeros_like(x), off), up_guard(dev, np.zeros_like(x), off)
        l0 = launches(t4k); call(t4k, "t4k_activate", L, px, py, pf, alpha, n, None); assert launches(t4k) - l0 == 1
        gy, gf = dn_guard(dev, ty, off, n), dn_guard(dev, tf, off, n)
        assert same_bits(dn_guard(dev, tx, off, n), x)
        with np.errstate(all="ignore"):
            wo, wm = wt.act(kind, x, alpha)
        if specials:
            y = np.zeros_like(x); f = np.zeros_like(x); assert o.t4o_activate(L, P(x), P(y), P(f), alpha, n) == 0
            assert np.array_equal(wt.kinds(gy), wt.kinds(y)) and np.array_equal(wt.kinds(gf), wt.kinds(f)), (kind, gy, y, gf, f)
        name = "%s %s off=%d" % (kind, "specials" if specials else "row", off)
        wt.check(name, gy, wo, kind="activation domain"); wt.check(name + " mask", gf, wm, kind="activation domain")


def test_zz_report_worst_ratios():
    """the worst |error| / bound per op (pytest -s prints it; tests/README.md quotes it) and the three measured figures beside their allowances"""
    print("\nmath-op domain sweep, worst |err| / bound per op:")
    mine = {k: v for k, v in wt.WORST.items() if k.startswith("math ") or k == "activation domain"}
    for kind in sorted(mine):
        print("  %-28s %.3g   %s" % (kind, mine[kind][0], mine[kind][1]))
    for op in sorted(MEASURED):
        print("  %s measured %.5f ulps of |exact| (wt.MEASURED_%s = %s, allowance wt.ULP_%s = %.1f)"
              % (op, MEASURED[op], op, getattr(wt, "MEASURED_" + op), op, getattr(wt, "ULP_" + op)))
    assert all(r <= 1.0 for r, _ in mine.values())
