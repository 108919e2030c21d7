"""`transpose` with an axis order ( T p -- T T' ) (DESIGN.md 3.13 "Beyond the reference: axis permutation") on the CPU oracle VM - the
product's host sources over the oracle's C-ABI, which has no t4k_permute, so Tensor::permute reaches the order by swaps of neighbouring
axes, each a loop of t4k_transpose calls, here.

All 24 orders on (2,3,4,5) and on two shapes with extent-1 axes: the shape, every element equal to numpy.transpose (pure copies: no
tolerance), T kept beneath T' and untouched, p gone; the inverse order giving the operand back; 8241 equal to `T transpose`.  The rejected
p values keep the text of the axis words and T; a matrix, a vector, a scalar or a model beneath the scalar keeps today's `tensor2?` and
stack.  Two scripts against NumPy: multi-head attention from [N,L,heads,D] (8412 in, the attention script of DESIGN.md 3.12, 8412 out) and
a channel-first batch brought to NHWC with 8214 and fed to `14 avg`.
tests/test_gpu_permute_words.py runs the same checks on the product VM."""
import itertools
import os
import zlib

import numpy as np
import pytest

import f64_witness as wt
import test_softmax_axes_words_oracle as smax_rows
from test_bcast_words_oracle import depth
from vm_util import ROOT, OracleVM

WEIGHT = (8, 4, 2, 1)                                                   # N, H, W, C
ORDERS = list(itertools.permutations(range(4)))
SHAPES = [(2, 3, 4, 5), (3, 1, 4, 1), (1, 2, 1, 3)]
REJECTED = ["0", "842", "8422", "1234", "84210", "8421.5", "-8421"]
RTOL, ATOL = 2e-4, 2.5e-4                                               # vm_util.compare's tolerances (the attention script's bar in 3.12)


def word(perm):
    """the scalar p that names `perm` (perm[i] = the source axis output axis i takes)"""
    return "%d%d%d%d" % tuple(WEIGHT[a] for a in perm)


def operand(shape, tag=""):
    rng = np.random.default_rng(zlib.crc32(repr((shape, tag)).encode()))
    return rng.standard_normal(shape).astype(np.float32)


def check_order(vm, shape, perm):
    A = operand(shape)
    d0 = depth(vm)
    vm.store(A, "%d %d %d %d tensor" % shape)
    out = vm.eval("%s transpose" % word(perm))
    assert "tensor2?" not in out and "axes" not in out, out
    assert depth(vm) == d0 + 2, (shape, perm)                           # p is gone, T stays, T' is pushed
    R = vm.fetch(None)
    assert R.shape == tuple(shape[a] for a in perm), (R.shape, shape, perm)
    assert np.array_equal(R, A.transpose(perm)), (shape, perm)
    B = vm.fetch("%s transpose" % word(np.argsort(perm)))               # the inverse order gives the operand back
    assert depth(vm) == d0 + 3
    assert B.shape == tuple(shape) and np.array_equal(B, A), (shape, perm)
    vm.eval("drop drop")
    assert np.array_equal(vm.fetch(None), A)                            # T beneath is untouched
    vm.eval("drop")
    assert depth(vm) == d0


def check_8241_is_the_tensor_word(vm, shape=(2, 3, 4, 5)):
    A = operand(shape, "8241")
    d0 = depth(vm)
    vm.store(A, "%d %d %d %d tensor" % shape)
    P = vm.fetch("8241 transpose")
    vm.eval("drop")
    T = vm.fetch("transpose")
    assert depth(vm) == d0 + 2
    vm.eval("drop drop")
    assert P.shape == T.shape and np.array_equal(P, T)
    assert np.array_equal(T, A.transpose(0, 2, 1, 3))


def check_rejected(vm):
    for p in REJECTED:
        d0 = depth(vm)
        vm.eval("2 3 2 3 tensor ones")
        out = vm.eval("%s transpose" % p)
        assert "transpose: axes 8421?\n" in out and "tensor2?" not in out, (p, out)
        assert depth(vm) == d0 + 1, p                                   # p is consumed, nothing is pushed
        assert np.array_equal(vm.fetch(None), np.ones((2, 3, 2, 3), np.float32))
        vm.eval("drop")


def check_other_cells_keep_their_text(vm):
    """a matrix, a vector, a scalar or a model beneath the scalar: the word prints what it printed and moves nothing"""
    for make, n_obj in (("2 3 matrix ones", 1), ("5 vector ones", 1), ("7", 0), ("4 1 1 1 nn.model", 1)):
        d0 = depth(vm)
        out = vm.eval("%s 8241 transpose" % make)
        assert "tensor2?" in out and "axes" not in out, (make, out)
        assert depth(vm) == d0 + 2, make
        assert vm.eval(".").split()[0] == "8241"
        if n_obj:
            if "matrix" in make:
                assert np.array_equal(vm.fetch(None), np.ones((1, 2, 3, 1), np.float32))
            vm.eval("drop")
        else:
            assert vm.eval(".").split()[0] == "7"
        assert depth(vm) == d0


def check_multi_head_attention(vm, N, L, heads, D):
    """Q, K, V as a projection leaves them, [N,L,heads,D]: 8412 into the [N,L,D,heads] layout of the attention script, 8412 back out"""
    Q, K, V = (operand((N, L, heads, D), t) for t in "QKV")
    shape = "%d %d %d %d tensor" % (N, L, heads, D)
    scale = 1.0 / np.sqrt(D)
    d0 = depth(vm)
    vm.store(K, shape); vm.eval("8412 transpose transpose")             # Kh Kt Kt'
    vm.store(Q, shape); vm.eval("8412 transpose swap drop swap")        # Kh Kt Qt Kt'
    vm.eval("@ %.7f *= 2 softmax" % scale)                              # Kh Kt Qt Kt' P
    vm.store(V, shape); vm.eval("8412 transpose swap drop")             # Kh Kt Qt Kt' P Vt
    Ot = vm.fetch("@")                                                  # ... O
    Oh = vm.fetch("8412 transpose")                                     # ... O Oh
    assert depth(vm) == d0 + 8
    vm.eval("drop drop drop drop drop drop drop drop")
    assert depth(vm) == d0
    assert Ot.shape == (N, L, D, heads) and Oh.shape == (N, L, heads, D)
    assert np.array_equal(Oh, Ot.transpose(0, 1, 3, 2))
    t = lambda X: X.transpose(0, 1, 3, 2)
    _, want = smax_rows.attention_numpy(t(Q), t(K), t(V), scale)         # [N,L,D,heads], float64
    want = want.transpose(0, 1, 3, 2)
    assert np.all(np.abs(wt.f64(Oh) - want) <= ATOL + RTOL * np.maximum(np.abs(Oh), np.abs(want))), float(np.max(np.abs(Oh - want)))


def check_channel_first_batch(vm, n, c, h, w):
    """a channel-first batch stored flat, given its extents through reshape4, brought to NHWC with 8214 and averaged per channel"""
    X = operand((n, c, h, w), "nchw")
    d0 = depth(vm)
    vm.store(X, "1 1 1 %d tensor" % X.size)
    vm.eval("%d %d %d %d reshape4" % (n, c, h, w))
    Y = vm.fetch("8214 transpose")
    M = vm.fetch("14 avg")
    assert depth(vm) == d0 + 3
    vm.eval("drop drop drop")
    assert Y.shape == (n, h, w, c) and np.array_equal(Y, X.transpose(0, 2, 3, 1))
    assert M.shape == (1, 1, 1, c)
    cnt = n * h * w
    # an fp32 sum of cnt terms in any order, then one fp32 division: (cnt + 1) roundings, each at most 2^-24 of the sum of magnitudes
    x64 = wt.f64(X)
    bound = (cnt + 1) * wt.U * np.abs(x64).sum((0, 2, 3)) / cnt
    assert np.all(np.abs(wt.f64(M).ravel() - x64.mean((0, 2, 3))) <= bound)


@pytest.fixture(scope="module")
def ovm():
    if not os.path.exists(os.path.join(ROOT, "oracle", "libten4_oracle.so")):
        pytest.skip("oracle/libten4_oracle.so not built")
    v = OracleVM(seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("perm", ORDERS, ids=[word(p) for p in ORDERS])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_order(ovm, shape, perm):
    check_order(ovm, shape, perm)


def test_8241_is_the_tensor_word(ovm):
    check_8241_is_the_tensor_word(ovm)


def test_rejected_orders_keep_text_and_stack(ovm):
    check_rejected(ovm)


def test_other_cells_beneath_the_scalar_keep_their_text(ovm):
    check_other_cells_keep_their_text(ovm)


def test_multi_head_attention_script_against_numpy(ovm):
    check_multi_head_attention(ovm, 2, 5, 3, 4)


def test_channel_first_batch_script_against_numpy(ovm):
    check_channel_first_batch(ovm, 2, 3, 5, 4)
