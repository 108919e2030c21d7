"""`sum avg std norm` with an axis mask ( T m -- T R ) (DESIGN.md 3.10 "Beyond the reference: axis reductions") on the CPU oracle VM - the
product's host sources over the oracle's C-ABI, which has no t4k_reduce_axes, so Tensor::reduce_axes gathers every output's elements
with t4k_copy and takes one t4k_reduce per output here.

Every row of the table: the result's shape and the name `.` prints, values against float64 on the very fp32 operands (tests/f64_witness.py:
bounds that hold for any summation order), stack effects, the rejected masks keeping their text and their stack, the cells that leave the
words no-ops, the scalar forms unchanged, and `T 6 avg -` against NumPy.  tests/test_gpu_axis_words.py runs the same rows on the product VM."""
import os
import zlib

import numpy as np
import pytest

import f64_witness as wt
from test_bcast_words_oracle import depth, operand
from test_bmm_words_oracle import ctor, nhwc
from vm_util import ROOT, OracleVM

WORDS = ["sum", "avg", "std", "norm"]
T = ("t", 2, 3, 4, 3)
# (operand, mask, the name `.` gives the result)
TABLE = [(T, 7, "tensor[2,1,1,1]"), (T, 14, "tensor[1,1,1,3]"), (("m", 3, 4), 4, "matrix[1,4]"), (("m", 3, 4), 2, "matrix[3,1]"), (("v", 5), 4, "vector[1]")]
MORE = [(T, 6, "tensor[2,1,1,3]"), (T, 15, "tensor[1,1,1,1]"), (T, 10, "tensor[1,3,1,3]"), (T, 5, "tensor[2,1,4,1]"), (T, 1, "tensor[2,3,4,1]"), (T, 8, "tensor[1,3,4,3]"),
        (("m", 3, 4), 6, "matrix[1,1]"), (("m", 3, 4), 13, "matrix[1,4]"),      # bits on the axes of extent 1 (N, C) change nothing
        (("v", 5), 11, "vector[5]"), (("t", 3, 1, 5, 2), 6, "tensor[3,1,1,2]")]
IDS = lambda rows: ["%s_m%d" % ("x".join(map(str, d[1:])) + d[0], m) for d, m, _ in rows]


def axes_of(mask):
    return tuple(i for i in range(4) if mask & (8 >> i))


def kept_shape(d, mask):
    return tuple(1 if mask & (8 >> i) else e for i, e in enumerate(nhwc(d)))


def count(d, mask):
    return int(np.prod([e for i, e in enumerate(nhwc(d)) if mask & (8 >> i)]))


def relative(name, got, exact, cnt):
    """std / norm: |got - exact| <= 2 (cnt + 4) 2^-24 |exact| on every element"""
    err, bound = np.abs(wt.f64(got) - exact), 2.0 * (cnt + 4) * wt.U * np.abs(exact)
    assert np.all(err <= bound), (name, float(np.max(err / np.maximum(bound, 1e-300))))


def check_value(word, A, mask, R, avg32=None):
    """R against float64 on the fp32 operand A; std's centre is the fp32 tensor the VM's own `avg` gave for the mask"""
    ax, a64 = axes_of(mask), wt.f64(A)
    cnt = int(np.prod([A.shape[i] for i in ax]))
    if word == "sum":
        wt.check("sum", R, wt.W(a64.sum(ax, keepdims=True), np.abs(a64).sum(ax, keepdims=True), cnt))
    elif word == "avg":
        wt.check("avg", R, wt.W(a64.sum(ax, keepdims=True) / cnt, np.abs(a64).sum(ax, keepdims=True) / cnt, cnt + 1))
    elif word == "norm":
        relative("norm", R, np.sqrt((a64 * a64).sum(ax, keepdims=True)), cnt)
    else:
        d = a64 - wt.f64(avg32)
        relative("std", R, np.sqrt((d * d).sum(ax, keepdims=True)) / cnt, cnt)


def run_row(vm, d, mask, word):
    """( -- ) stores an operand of d, runs `mask word`, checks the stack effect; returns (A, R, avg32)"""
    rng = np.random.default_rng(zlib.crc32(repr((d, mask)).encode()))
    A = operand(rng, d)
    d0 = depth(vm)
    vm.store(A, ctor(d))
    avg32 = None
    if word == "std":
        avg32 = vm.fetch("%d avg" % mask); vm.eval("drop")
    R = vm.fetch("%d %s" % (mask, word))
    assert depth(vm) == d0 + 2, (d, mask, word)                          # the mask is consumed, T stays, R is new
    vm.eval("drop")
    assert np.array_equal(vm.fetch(None), A)                            # T untouched bit for bit
    vm.eval("drop")
    assert depth(vm) == d0
    return A, R, avg32


def check_row(vm, d, mask, word):
    A, R, avg32 = run_row(vm, d, mask, word)
    assert R.shape == kept_shape(d, mask), (R.shape, kept_shape(d, mask))
    check_value(word, A, mask, R, avg32)
    return A, R


def check_names(vm, rows):
    for d, mask, text in rows:
        for word in WORDS:
            out = vm.eval("%s ones %d %s . cr" % (ctor(d), mask, word))
            assert text in out, (d, mask, word, out)
            vm.eval("drop")


REJECTED = ["0", "16", "-1", "2.5"]


def check_rejected(vm):
    for word in WORDS:
        for m in REJECTED:
            d0 = depth(vm)
            vm.eval("2 3 matrix ones")
            out = vm.eval("%s %s" % (m, word))
            assert "%s: axes 1..15?\n" % word in out, (word, m, out)
            assert depth(vm) == d0 + 1, (word, m)                       # the mask is consumed, nothing is pushed
            assert np.array_equal(vm.fetch(None), np.ones((1, 2, 3, 1), np.float32))
            vm.eval("drop")


def check_noops(vm):
    """a scalar or a model beneath the mask: the words stay the no-ops they are"""
    for word in WORDS:
        d0 = depth(vm)
        out = vm.eval("5 3 %s" % word)
        assert "axes" not in out and depth(vm) == d0 + 2
        assert vm.eval(". .").split()[:2] == ["3", "5"]
        vm.eval("4 1 1 1 nn.model 6 %s" % word)
        assert depth(vm) == d0 + 2
        assert vm.eval(".").split()[0] == "6"
        vm.eval("drop")
        assert depth(vm) == d0


def check_scalar_forms(vm):
    """a tensor on top: one scalar, as before"""
    a = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    d0 = depth(vm)
    vm.store(a, "3 4 matrix")
    a64 = wt.f64(a)
    want = {"sum": a64.sum(), "avg": a64.mean(), "norm": np.sqrt((a64 * a64).sum()), "std": np.sqrt(((a64 - a64.mean()) ** 2).sum()) / 12}
    for word in WORDS:
        got = float(vm.eval("%s ." % word).split()[0])
        assert depth(vm) == d0 + 1
        assert abs(got - want[word]) <= 1e-3 * abs(want[word]), (word, got, want[word])
    for word in WORDS:                                                  # mask 15 means what the scalar form means
        R = vm.fetch("15 %s" % word)
        got = float(vm.eval("drop %s ." % word).split()[0])
        assert abs(got - float(R.ravel()[0])) <= 2e-4 * abs(got) + 1e-4, (word, got, R)
    vm.eval("drop")
    assert depth(vm) == d0


def check_centre(vm, d=T):
    """T 6 avg - : every (entry, channel) plane centred, R feeding the broadcast `-` of 3.9"""
    rng = np.random.default_rng(6)
    A = operand(rng, d)
    d0 = depth(vm)
    vm.store(A, ctor(d))
    M = vm.fetch("6 avg")
    O = vm.fetch("-")                                                   # T M O
    assert depth(vm) == d0 + 3 and O.shape == A.shape
    vm.eval("drop drop drop")
    check_value("avg", A, 6, M)
    assert np.array_equal(O, A - M)                                     # one correctly rounded subtraction of the broadcast mean
    a64 = wt.f64(A); mean = a64.mean((1, 2), keepdims=True)
    cnt = A.shape[1] * A.shape[2]
    bound = wt.bound_of(mean, np.abs(a64).mean((1, 2), keepdims=True), cnt + 1) + wt.U * np.abs(a64 - wt.f64(M))
    assert np.all(np.abs(wt.f64(O) - (a64 - mean)) <= bound)


@pytest.fixture(scope="module")
def ovm():
    if not os.path.exists(os.path.join(ROOT, "oracle", "libten4_oracle.so")):
        pytest.skip("oracle/libten4_oracle.so not built")
    v = OracleVM(seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("d,mask,text", TABLE + MORE, ids=IDS(TABLE + MORE))
def test_table_rows(ovm, d, mask, text, word):
    check_row(ovm, d, mask, word)


def test_result_names(ovm):
    check_names(ovm, TABLE + MORE)


def test_rejected_masks_keep_text_and_stack(ovm):
    check_rejected(ovm)


def test_scalar_or_model_beneath_the_mask_is_a_noop(ovm):
    check_noops(ovm)


def test_scalar_forms_unchanged(ovm):
    check_scalar_forms(ovm)


def test_centre_planes_against_numpy(ovm):
    check_centre(ovm)


def test_std_of_every_axis_is_the_scalar_std(ovm):
    """the reference's formula sqrt(sum (x - avg)^2) / n, with the fp32 avg: `T 15 std` against `T std` to the printer's digits"""
    rng = np.random.default_rng(15)
    A = operand(rng, T)
    ovm.store(A, ctor(T))
    R = ovm.fetch("15 std"); ovm.eval("drop")
    s = float(ovm.eval("std .").split()[0]); ovm.eval("drop")
    assert abs(s - float(R.ravel()[0])) <= 1e-4
