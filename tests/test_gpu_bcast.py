"""t4k_tt_op_bcast / t4k_transpose_batched (include/t4k.h, csrc/bcast.hip) through the C ABI.

Broadcast arithmetic: every axis pattern (each single axis of B, each single axis of A, the two-sided outer product, an all-ones
operand, no broadcast) x ADD / SUB / MUL / DIV over extents whose innermost merged run is 1, 3, 4, 5, 64 and 1028 elements long, shapes
whose work exceeds the grid cap (the stride loop wraps, on the packed scalar path and on the chunked float4 path), operands 4 bytes off
16-byte alignment, the output aliasing the dense operand.  Expected: t4k_tt_op on np.broadcast_to copies of the same operands, BIT FOR
BIT; ADD / SUB / MUL also against NumPy float32 (single correctly rounded operations on operands from +-[0.5, 2): nothing subnormal, no
tolerance anywhere).  Every call is exactly one launch, an empty dim none.

Batched transpose: H, W over the tile edges {1, 63, 64, 65, 130} x C in {1, 3} x batch in {1, 2, 7, 128}, equal to
a.transpose(0, 2, 1, 3); one launch; batch == 0; error returns."""
import ctypes
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ADD, SUB, MUL, DIV = 16, 17, 18, 19                                   # include/t4k.h math_op
OPS = [ADD, SUB, MUL, DIV]
NP_OP = {ADD: np.add, SUB: np.subtract, MUL: np.multiply}
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4

I4 = ctypes.c_int * 4
L4 = ctypes.c_long * 4

# (axes of A with extent 1, axes of B with extent 1) over (N, H, W, C)
PATTERNS = {"B_n": ((), (0,)), "B_h": ((), (1,)), "B_w": ((), (2,)), "B_c": ((), (3,)),
            "A_n": ((0,), ()), "A_h": ((1,), ()), "A_w": ((2,), ()), "A_c": ((3,), ()),
            "outer": ((1, 3), (0, 2)),                                # (N,1,W,1) op (1,H,1,C)
            "B_ones": ((), (0, 1, 2, 3)), "none": ((), ())}


def lcount(h):
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return int(h.lib.t4k_launch_count())


def operand(rng, shape):
    """+-[0.5, 2): sums, differences, products and quotients of two of them are normal numbers or exact zeros"""
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def strides(shape):
    s, d = [0] * 4, 1
    for i in (3, 2, 1, 0):
        s[i] = 0 if shape[i] == 1 else d
        d *= shape[i]
    return s


class Dev:
    """a device buffer holding `a` starting `off` floats into a 16-byte aligned allocation"""

    def __init__(self, a, off=0):
        import torch
        self.off, self.n = off, a.size
        self.t = torch.from_numpy(np.concatenate([np.zeros(off, np.float32), np.ascontiguousarray(a, np.float32).ravel(), np.zeros(4, np.float32)])).cuda()
        torch.cuda.synchronize()

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr() + 4 * self.off)

    def get(self, h, shape):
        h.call("t4k_sync", None)
        return self.t.cpu().numpy()[self.off:self.off + self.n].reshape(shape)


def run_case(h, op, dim, pat, offs=(0, 0, 0), alias=False):
    ones_a, ones_b = PATTERNS[pat]
    sha = tuple(1 if i in ones_a else dim[i] for i in range(4))
    shb = tuple(1 if i in ones_b else dim[i] for i in range(4))
    rng = np.random.default_rng(zlib.crc32(repr((dim, pat)).encode()))
    A, B = operand(rng, sha), operand(rng, shb)
    Af, Bf = np.ascontiguousarray(np.broadcast_to(A, dim)), np.ascontiguousarray(np.broadcast_to(B, dim))
    n = Af.size
    # expected: the flat kernel on expanded operands
    dAf, dBf, dE = Dev(Af), Dev(Bf), Dev(np.zeros(n, np.float32))
    h.call("t4k_tt_op", op, dAf.p, dBf.p, dE.p, n, None)
    want = dE.get(h, dim)
    dA, dB = Dev(A, offs[0]), Dev(B, offs[1])
    dO = dA if alias else Dev(np.full(n, np.nan, np.float32), offs[2])
    l0 = lcount(h)
    h.call("t4k_tt_op_bcast", op, dA.p, dB.p, dO.p, I4(*dim), L4(*strides(sha)), L4(*strides(shb)), None)
    assert lcount(h) - l0 == 1
    got = dO.get(h, dim)
    assert np.array_equal(got, want), (dim, pat, op, int(np.sum(got != want)))
    if op in NP_OP:
        assert np.array_equal(got, NP_OP[op](Af, Bf))
    if not alias:
        assert np.array_equal(dA.get(h, sha), A)                       # the operands are intact
    assert np.array_equal(dB.get(h, shb), B)
    tail = dO.t.cpu().numpy()
    assert not tail[:dO.off].any() and not tail[dO.off + dO.n:].any()   # nothing written outside O


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("pat", list(PATTERNS))
@pytest.mark.parametrize("inner", [3, 4, 5, 64])
def test_axis_patterns(t4k, op, pat, inner):
    run_case(t4k, op, (2, 3, 5, inner), pat)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dim", [(1, 1, 1, 1), (7, 1, 1, 1), (1, 1, 5, 1), (3, 1, 1, 4)])
def test_degenerate_extents(t4k, op, dim):
    """a single element (the run of length 1) and shapes most of whose axes are 1"""
    for pat in ("B_ones", "none", "A_n"):
        run_case(t4k, op, dim, pat)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("pat", list(PATTERNS))
def test_run_longer_than_a_workgroup(t4k, op, pat):
    """1028 elements = 257 float4s: one more than 256 lanes take in one pass"""
    run_case(t4k, op, (2, 2, 3, 1028), pat)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dim,pat", [((3, 257, 129, 5), "B_c"),       # 99 459 runs of 5, 32 to a workgroup: 3 109 workgroup passes over a grid of 2 048
                                     ((3, 257, 129, 5), "outer"),
                                     ((3, 257, 129, 5), "none"),      # one odd run of 497 295 on the scalar path
                                     ((9, 257, 129, 8), "none"),      # one run of 596 754 float4s: 2 332 chunks of 256 lanes
                                     ((9, 257, 129, 8), "B_n")])
def test_grid_stride_wraps(t4k, op, dim, pat):
    run_case(t4k, op, dim, pat)


@pytest.mark.parametrize("pat", list(PATTERNS))
@pytest.mark.parametrize("which", [0, 1, 2])
def test_four_byte_offsets_take_the_scalar_path(t4k, pat, which):
    offs = [0, 0, 0]; offs[which] = 1
    run_case(t4k, OPS[(which + len(pat)) % 4], (2, 3, 5, 64), pat, offs=tuple(offs))
    run_case(t4k, OPS[(which + len(pat) + 1) % 4], (2, 2, 3, 1028), pat, offs=tuple(offs))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("pat", ["B_n", "B_h", "B_w", "B_c", "B_ones", "none"])
def test_output_may_alias_the_dense_operand(t4k, op, pat):
    run_case(t4k, op, (3, 5, 7, 8), pat, alias=True)
    run_case(t4k, op, (3, 5, 7, 3), pat, alias=True)


def test_general_strides(t4k):
    """strides that are neither dense nor zero (every second column of a wider operand): the scalar path"""
    rng = np.random.default_rng(5)
    A, B = operand(rng, (2, 3, 10, 1)), operand(rng, (1, 3, 1, 1))
    dA, dB, dO = Dev(A), Dev(B), Dev(np.zeros(30, np.float32))
    l0 = lcount(t4k)
    t4k.call("t4k_tt_op_bcast", SUB, dA.p, dB.p, dO.p, I4(2, 3, 5, 1), L4(30, 10, 2, 0), L4(0, 1, 0, 0), None)
    assert lcount(t4k) - l0 == 1
    assert np.array_equal(dO.get(t4k, (2, 3, 5, 1)), A[:, :, ::2] - B)


def test_empty_dim_launches_nothing(t4k):
    d = Dev(np.zeros(16, np.float32))
    for dim in [(0, 3, 5, 4), (2, 0, 5, 4), (2, 3, 0, 4), (2, 3, 5, 0)]:
        l0 = lcount(t4k)
        assert t4k.lib.t4k_tt_op_bcast(ADD, d.p, d.p, d.p, I4(*dim), L4(0, 0, 0, 1), L4(0, 0, 0, 1), None) == OK
        assert lcount(t4k) == l0


def test_bcast_error_returns(t4k):
    d = Dev(np.ones(16, np.float32))
    dim, s = I4(1, 1, 4, 4), L4(0, 0, 4, 1)
    f = t4k.lib.t4k_tt_op_bcast
    l0 = lcount(t4k)
    assert f(ADD, None, d.p, d.p, dim, s, s, None) == ERR_ARG
    assert f(ADD, d.p, None, d.p, dim, s, s, None) == ERR_ARG
    assert f(ADD, d.p, d.p, None, dim, s, s, None) == ERR_ARG
    assert f(ADD, d.p, d.p, d.p, None, s, s, None) == ERR_ARG
    assert f(ADD, d.p, d.p, d.p, dim, None, s, None) == ERR_ARG
    assert f(ADD, d.p, d.p, d.p, dim, s, None, None) == ERR_ARG
    assert f(ADD, d.p, d.p, d.p, I4(1, 1, -4, 4), s, s, None) == ERR_ARG
    assert f(ADD, d.p, d.p, d.p, dim, L4(0, 0, -4, 1), s, None) == ERR_ARG
    assert f(ADD, d.p, d.p, d.p, dim, s, L4(0, 0, 4, -1), None) == ERR_ARG
    for op in (0, 15, 20, 26, 99):                                      # ABS, POW, MOD, COS, nothing
        assert f(op, d.p, d.p, d.p, dim, s, s, None) == ERR_UNSUPPORTED
        assert ("k_tt_op op=%d not supported" % op).encode() in t4k.lib.t4k_last_error()
    assert lcount(t4k) == l0
    assert np.array_equal(d.get(t4k, (16,)), np.ones(16, np.float32))


# ---------------------------------------------------------------- transpose
EDGES = [1, 63, 64, 65, 130]
HW = [(h, w) for h in EDGES for w in EDGES if h in (1, 65) or w in (1, 65) or h == w or (h, w) in ((63, 130), (130, 64), (64, 63))]


@pytest.fixture(scope="module")
def source():
    """one pool of distinct values every transpose case cuts its operand from"""
    return np.arange(128 * 130 * 130 * 3 // 4, dtype=np.float32)      # 1.6 M distinct integers, exact in fp32


@pytest.mark.parametrize("batch", [1, 2, 7, 128])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", HW)
def test_transpose_batched(t4k, source, H, W, C, batch):
    n = batch * H * W * C
    if n > source.size:                                                 # 128 x 130 x 130 x 3: values repeat, positions inside a tile do not
        a = np.resize(source, n).reshape(batch, H, W, C)
    else:
        a = source[:n].reshape(batch, H, W, C)
    dS, dD = Dev(a), Dev(np.full(n, np.nan, np.float32))
    l0 = lcount(t4k)
    t4k.call("t4k_transpose_batched", dS.p, dD.p, H, W, C, batch, None)
    assert lcount(t4k) - l0 == 1
    assert np.array_equal(dD.get(t4k, (batch, W, H, C)), a.transpose(0, 2, 1, 3))
    tail = dD.t.cpu().numpy()
    assert not tail[n:].any()


def test_transpose_batched_equals_the_per_entry_kernel(t4k):
    rng = np.random.default_rng(9)
    a = rng.standard_normal((5, 70, 33, 3)).astype(np.float32)
    dS, dD, dL = Dev(a), Dev(np.zeros(a.size, np.float32)), Dev(np.zeros(a.size, np.float32))
    t4k.call("t4k_transpose_batched", dS.p, dD.p, 70, 33, 3, 5, None)
    for b in range(5):
        o = 4 * b * 70 * 33 * 3
        t4k.call("t4k_transpose", ctypes.c_void_p(dS.p.value + o), ctypes.c_void_p(dL.p.value + o), 70, 33, 3, None)
    assert np.array_equal(dD.get(t4k, a.shape), dL.get(t4k, a.shape))


def test_transpose_batch_beyond_the_grid_limit(t4k):
    """batch x C = 70 000 > 65 535 grid.z slots: the kernel walks the rest"""
    a = np.arange(70000 * 2 * 3, dtype=np.float32).reshape(70000, 2, 3, 1)
    dS, dD = Dev(a), Dev(np.zeros(a.size, np.float32))
    l0 = lcount(t4k)
    t4k.call("t4k_transpose_batched", dS.p, dD.p, 2, 3, 1, 70000, None)
    assert lcount(t4k) - l0 == 1
    assert np.array_equal(dD.get(t4k, (70000, 3, 2, 1)), a.transpose(0, 2, 1, 3))


def test_transpose_empty_batch_and_error_returns(t4k):
    d = Dev(np.ones(16, np.float32))
    f = t4k.lib.t4k_transpose_batched
    l0 = lcount(t4k)
    assert f(d.p, d.p, 2, 2, 1, 0, None) == OK
    assert f(None, d.p, 2, 2, 1, 1, None) == ERR_ARG
    assert f(d.p, None, 2, 2, 1, 1, None) == ERR_ARG
    assert f(d.p, d.p, 0, 2, 1, 1, None) == ERR_ARG
    assert f(d.p, d.p, 2, 0, 1, 1, None) == ERR_ARG
    assert f(d.p, d.p, 2, 2, 0, 1, None) == ERR_ARG
    assert f(d.p, d.p, -2, 2, 1, 1, None) == ERR_ARG
    assert f(d.p, d.p, 2, 2, 1, -1, None) == ERR_ARG
    assert lcount(t4k) == l0
    assert np.array_equal(d.get(t4k, (16,)), np.ones(16, np.float32))
