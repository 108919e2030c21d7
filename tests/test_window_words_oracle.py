"""Box windows (DESIGN.md 3.14 "Beyond the reference: box windows"): `slice` with eight scalars ( T n0 n1 h0 h1 w0 w1 c0 c1 -- T T' ) and
`t!` with four scalars on two tensors ( T S n0 h0 w0 c0 -- T ), on the CPU oracle VM - the product's host sources over the oracle's
C-ABI, which has no t4k_window, so Tensor::window walks the box run by run with t4k_copy here.

Every comparison of elements is exact: the words copy and do nothing else.  For each of the 16 subsets of axes cut to [1, extent - 1) on
(3,4,5,6): `slice` against NumPy slicing with T untouched beneath, `t!` against NumPy assignment on random 32-bit patterns compared as
uint32, so that everything outside the box is bit-identical.  The same on a matrix and a vector with the rank kept, the four-scalar
`slice` against the eight-scalar one, the round trips (slice then t! back; concatenation along C and along N), the rejected operands
with their text and stack, the cells that keep what they did before, and a script against NumPy: a fused [N,L,1,3D] projection split into
Q, K and V by three slices, multi-head attention on them, the heads joined again with t!.
tests/test_gpu_window_words.py runs the same checks on the product VM."""
import os
import zlib

import numpy as np
import pytest

import f64_witness as wt
import test_softmax_axes_words_oracle as smax_rows
from test_bcast_words_oracle import depth
from vm_util import ROOT, OracleVM

SHAPE = (3, 4, 5, 6)
MASKS = list(range(16))                                                 # bit 8 >> axis: the axis is cut to [1, extent - 1)
RTOL, ATOL = 2e-4, 2.5e-4                                               # vm_util.compare's tolerances (the attention script's bar in 3.13)
MODEL = "4 1 1 1 nn.model"


def mask_id(m):
    return "".join(c for i, c in enumerate("NHWC") if m & (8 >> i)) or "whole"


def operand(shape, tag=""):
    rng = np.random.default_rng(zlib.crc32(repr((tuple(shape), tag)).encode()))
    return rng.standard_normal(shape).astype(np.float32)


def bits(shape, tag=""):
    """random 32-bit patterns viewed as float32: NaN payloads, denormals and infinities among them"""
    rng = np.random.default_rng(zlib.crc32(repr((tuple(shape), tag, "bits")).encode()))
    return rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ctor(shape, rank=4):
    """shape is always (N,H,W,C): a matrix is (1,H,W,1), a vector (1,K,1,1)"""
    return {4: "%d %d %d %d tensor" % tuple(shape), 2: "%d %d matrix" % (shape[1], shape[2]), 1: "%d vector" % shape[1]}[rank]


def cut(shape, mask):
    """the box of the subset `mask`: (lo, hi) per axis, and the same as the words take it (an uncut axis as 0 -1)"""
    box = [(1, e - 1) if mask & (8 >> i) else (0, e) for i, e in enumerate(shape)]
    text = " ".join("%d %d" % b if mask & (8 >> i) else "0 -1" for i, b in enumerate(box))
    return box, text


def index(box):
    return tuple(slice(lo, hi) for lo, hi in box)


def top_name(vm):
    """how `.` names the tensor on top (tensor[..] / matrix[..] / vector[..]); the tensor is consumed by `.`, so a view of it is printed"""
    return vm.eval("dup .").strip().split("[")[0]


def check_slice(vm, shape, mask, rank=4):
    A = operand(shape, ("slice", mask))
    box, text = cut(shape, mask)
    d0 = depth(vm)
    vm.store(A, ctor(shape, rank))
    out = vm.eval("%s slice" % text)
    assert "range?" not in out and "dim?" not in out, out
    assert depth(vm) == d0 + 2, (shape, mask)                           # the eight scalars are gone, T stays, T' is pushed
    R = vm.fetch(None)
    want = A[index(box)]
    assert R.shape == want.shape, (R.shape, want.shape, mask)
    assert np.array_equal(R, want), (shape, mask)
    assert top_name(vm) == {4: "tensor", 2: "matrix", 1: "vector"}[rank], (rank, mask)
    vm.eval("drop")
    assert np.array_equal(vm.fetch(None), A)                            # T beneath is untouched
    vm.eval("drop")
    assert depth(vm) == d0


def check_four_equals_eight(vm, shape=SHAPE, rank=4):
    A = operand(shape, "four")
    (_, (h0, h1), (w0, w1), _), _ = cut(shape, 6)
    d0 = depth(vm)
    vm.store(A, ctor(shape, rank))
    F = vm.fetch("%d %d %d %d slice" % (w0, w1, h0, h1))               # ( T x0 x1 y0 y1 -- T T' ): x along W, y along H
    vm.eval("drop")
    E = vm.fetch("0 -1 %d %d %d %d 0 -1 slice" % (h0, h1, w0, w1))
    assert depth(vm) == d0 + 2
    vm.eval("drop drop")
    assert F.shape == E.shape and np.array_equal(F, E)
    assert np.array_equal(F, A[:, h0:h1, w0:w1, :])
    vm.store(A, ctor(shape, rank))                                      # -1 as the upper bound of the four-scalar form, as before
    F = vm.fetch("%d -1 %d -1 slice" % (w0, h0))
    vm.eval("drop drop")
    assert np.array_equal(F, A[:, h0:, w0:, :])
    assert depth(vm) == d0


def check_store(vm, shape, mask, rank=4):
    T = bits(shape, ("T", mask))
    box, _ = cut(shape, mask)
    S = bits(tuple(hi - lo for lo, hi in box), ("S", mask))
    d0 = depth(vm)
    vm.store(T, ctor(shape, rank))
    vm.store(S, ctor(S.shape, rank))
    vm.eval("%d %d %d %d" % tuple(lo for lo, _ in box))
    assert depth(vm) == d0 + 6
    out = vm.eval("t!")
    assert "range?" not in out, out
    assert depth(vm) == d0 + 1, (shape, mask)                           # the four scalars and S are gone, T stays
    got = vm.fetch(None)
    want = T.copy(); want[index(box)] = S
    assert got.shape == want.shape and np.array_equal(u32(got), u32(want)), (shape, mask)
    vm.eval("drop")
    assert depth(vm) == d0


def check_slice_then_store_is_identity(vm, shape=SHAPE):
    for mask in (0, 5, 10, 15):
        T = bits(shape, ("rt", mask))
        box, text = cut(shape, mask)
        d0 = depth(vm)
        vm.store(T, ctor(shape))
        vm.eval("%s slice %d %d %d %d t!" % ((text,) + tuple(lo for lo, _ in box)))
        assert depth(vm) == d0 + 1
        assert np.array_equal(u32(vm.fetch(None)), u32(T)), mask
        vm.eval("drop")


def check_concatenate(vm):
    for axis, sa, sb in ((3, (2, 3, 4, 5), (2, 3, 4, 7)), (0, (2, 3, 4, 5), (3, 3, 4, 5)), (1, (2, 3, 4, 5), (2, 1, 4, 5))):
        A, B = operand(sa, ("cat", axis)), operand(sb, ("cat", axis, 1))
        whole = list(sa); whole[axis] += sb[axis]
        at = [0, 0, 0, 0]; at[axis] = sa[axis]
        d0 = depth(vm)
        vm.eval(ctor(whole))                                            # a fresh tensor: every element is written by one of the two stores
        vm.store(A, ctor(sa)); vm.eval("0 0 0 0 t!")
        vm.store(B, ctor(sb)); vm.eval("%d %d %d %d t!" % tuple(at))
        assert depth(vm) == d0 + 1
        got = vm.fetch(None)
        vm.eval("drop")
        assert got.shape == tuple(whole) and np.array_equal(got, np.concatenate([A, B], axis)), axis


def bad_ranges(e):
    """lo = hi, lo > hi, hi = extent + 1, lo = -1, a fraction"""
    return ["1 1", "2 1", "0 %d" % (e + 1), "-1 %d" % e, "1.5 %d" % e, "0 1.5"]


def check_rejected_slices(vm, shape=SHAPE):
    A = operand(shape, "rej")
    d0 = depth(vm)
    vm.store(A, ctor(shape))
    for axis in range(4):
        for bad in bad_ranges(shape[axis]):
            words = ["0 -1"] * 4; words[axis] = bad
            out = vm.eval("%s slice" % " ".join(words))
            assert "slice: range?\n" in out, (axis, bad, out)
            assert depth(vm) == d0 + 1, (axis, bad)                     # the eight scalars are consumed, nothing is pushed
    assert np.array_equal(vm.fetch(None), A)
    vm.eval("drop")
    M = operand((1, 4, 5, 1), "rejm")
    vm.store(M, "4 5 matrix")
    for words in ("0 2 0 -1 0 -1 0 -1", "1 2 0 -1 0 -1 0 -1", "0 -1 0 -1 0 -1 0 2", "0 -1 0 -1 0 -1 1 2", "0 -1 0 5 0 -1 0 -1"):
        out = vm.eval("%s slice" % words)
        assert "slice: range?\n" in out, (words, out)
        assert depth(vm) == d0 + 1, words
    out = vm.eval("0 1 1 3 1 4 0 1 slice")                              # N and C as `0 1` are the matrix's own extents
    assert "range?" not in out and depth(vm) == d0 + 2
    assert np.array_equal(vm.fetch(None), M[:, 1:3, 1:4, :])
    vm.eval("drop")
    assert np.array_equal(vm.fetch(None), M)
    vm.eval("drop")
    assert depth(vm) == d0


def check_rejected_stores(vm, shape=SHAPE):
    T, S = bits(shape, "rejT"), bits((2, 2, 3, 4), "rejS")
    room = [e - s for e, s in zip(shape, S.shape)]                      # the last offset that fits
    d0 = depth(vm)
    vm.store(T, ctor(shape)); vm.store(S, ctor(S.shape))
    cases = []
    for axis in range(4):
        at = list(room); at[axis] += 1                                  # one too far on this axis
        cases.append("%d %d %d %d" % tuple(at))
    cases += ["0 -1 0 0", "-1 0 0 0", "0 0 0.5 0", "0.5 0 0 0"]
    for at in cases:
        out = vm.eval("%s t!" % at)
        assert "t!: range?\n" in out, (at, out)
        assert depth(vm) == d0 + 2, at                                  # the four scalars are consumed, T and S stay
    assert np.array_equal(u32(vm.fetch(None)), u32(S))
    vm.eval("%d %d %d %d t!" % tuple(room))                             # ... and the last offset that fits is taken
    assert depth(vm) == d0 + 1
    want = T.copy(); want[tuple(slice(o, o + s) for o, s in zip(room, S.shape))] = S
    assert np.array_equal(u32(vm.fetch(None)), u32(want))
    out = vm.eval("dup 0 0 0 0 t!")                                     # S shares T's storage
    assert "t!: range?\n" in out, out
    assert depth(vm) == d0 + 2
    vm.eval("drop")
    assert np.array_equal(u32(vm.fetch(None)), u32(want))
    vm.eval("drop")
    assert depth(vm) == d0


def check_cells_that_keep_their_behaviour(vm):
    d0 = depth(vm)
    A = operand((1, 2, 3, 1), "old")
    vm.store(A, "2 3 matrix")                                           # ( T v i -- T ) stores one scalar
    out = vm.eval("7.5 4 t!")
    assert "range?" not in out and depth(vm) == d0 + 1
    want = A.copy(); want.ravel()[4] = 7.5
    assert np.array_equal(vm.fetch(None), want)
    vm.eval("drop")
    for beneath, n_obj in (("7", 0), (MODEL, 1)):                       # eight scalars with no tensor beneath: four cells go, as before
        out = vm.eval("%s 1 2 3 4 5 6 7 8 slice" % beneath)
        assert "range?" not in out, out
        assert depth(vm) == d0 + 5, beneath
        assert vm.eval(". . . .").split()[:4] == ["4", "3", "2", "1"]
        vm.eval("drop")
        assert depth(vm) == d0
    out = vm.eval("%s 2 2 2 2 tensor ones 0 0 0 0 t!" % MODEL)          # the lower of the two is a model: two cells go, as before
    assert "range?" not in out, out
    assert depth(vm) == d0 + 4
    assert vm.eval(". .").split()[:2] == ["0", "0"]
    assert np.array_equal(vm.fetch(None), np.ones((2, 2, 2, 2), np.float32))
    vm.eval("drop drop")
    assert depth(vm) == d0


def check_qkv_script(vm, N, L, heads, Dh):
    """X [N,L,1,3D], a fused projection: three slices give Q, K and V, reshape4 gives them their heads, the multi-head attention script of
    tests/test_permute_words_oracle.py (8412 in, @ scale *= 2 softmax @, 8412 out) runs on them, and the heads are written side by side
    into a fresh [N,L,1,D] with one t! each"""
    D = heads * Dh
    X = operand((N, L, 1, 3 * D), "qkv")
    scale = 1.0 / np.sqrt(Dh)
    heads4 = "%d %d %d %d reshape4" % (N, L, heads, Dh)
    part = lambda k: "0 -1 0 -1 0 -1 %d %d slice %s" % (k * D, (k + 1) * D, heads4)
    d0 = depth(vm)
    vm.store(X, ctor(X.shape))
    V = vm.fetch(part(2)); vm.eval("swap")                              # V X
    K = vm.fetch(part(1)); vm.eval("swap")                              # V K X
    Q = vm.fetch(part(0)); vm.eval("swap drop")                         # V K Q
    assert depth(vm) == d0 + 3
    Xh = X.reshape(N, L, 3, heads, Dh)
    for got, k in ((Q, 0), (K, 1), (V, 2)):
        assert got.shape == (N, L, heads, Dh) and np.array_equal(got, Xh[:, :, k]), k
    vm.eval("8412 transpose swap drop")                                 # V K Qt
    vm.eval("swap 8412 transpose swap drop transpose swap drop")        # V Qt Kt'
    vm.eval("@ %.7f *= 2 softmax" % scale)                              # V Qt Kt' P
    vm.eval("swap drop swap drop swap")                                 # P V
    vm.eval("8412 transpose swap drop @")                               # P Vt O
    Oh = vm.fetch("8412 transpose")                                     # P Vt O Oh
    assert Oh.shape == (N, L, heads, Dh)
    vm.eval("%d %d 1 %d tensor" % (N, L, D))                            # ... Oh J
    for h in range(heads):
        vm.eval("swap 0 -1 0 -1 %d %d 0 -1 slice rot swap 0 0 0 %d t!" % (h, h + 1, h * Dh))   # J Oh -> J Oh S -> Oh S J -> Oh J S -> Oh J
    J = vm.fetch(None)
    assert depth(vm) == d0 + 5
    vm.eval("drop drop drop drop drop")
    assert depth(vm) == d0
    assert J.shape == (N, L, 1, D) and np.array_equal(J, Oh.reshape(N, L, 1, D))
    t = lambda A: wt.f64(A).transpose(0, 1, 3, 2)
    _, want = smax_rows.attention_numpy(t(Xh[:, :, 0]), t(Xh[:, :, 1]), t(Xh[:, :, 2]), scale)      # [N,L,Dh,heads], float64
    want = want.transpose(0, 1, 3, 2).reshape(N, L, 1, D)
    assert np.all(np.abs(wt.f64(J) - want) <= ATOL + RTOL * np.maximum(np.abs(J), np.abs(want))), float(np.max(np.abs(J - want)))


@pytest.fixture(scope="module")
def ovm():
    if not os.path.exists(os.path.join(ROOT, "oracle", "libten4_oracle.so")):
        pytest.skip("oracle/libten4_oracle.so not built")
    v = OracleVM(seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
def test_slice_every_subset_of_axes(ovm, mask):
    check_slice(ovm, SHAPE, mask)


@pytest.mark.parametrize("mask", [0, 2, 4, 6], ids=mask_id)
def test_slice_of_a_matrix_and_a_vector_keeps_the_rank(ovm, mask):
    check_slice(ovm, (1, 5, 7, 1), mask, rank=2)
    if not mask & 2:
        check_slice(ovm, (1, 9, 1, 1), mask, rank=1)


def test_four_scalar_slice_equals_the_eight_scalar_one(ovm):
    check_four_equals_eight(ovm)
    check_four_equals_eight(ovm, (1, 6, 7, 1), rank=2)


@pytest.mark.parametrize("mask", MASKS, ids=mask_id)
def test_store_every_subset_of_axes(ovm, mask):
    check_store(ovm, SHAPE, mask)


def test_store_into_a_matrix_and_a_vector(ovm):
    check_store(ovm, (1, 5, 7, 1), 6, rank=2)
    check_store(ovm, (1, 9, 1, 1), 4, rank=1)


def test_slice_then_store_leaves_the_tensor_as_it_was(ovm):
    check_slice_then_store_is_identity(ovm)


def test_stores_side_by_side_are_a_concatenation(ovm):
    check_concatenate(ovm)


def test_rejected_slices_keep_text_and_stack(ovm):
    check_rejected_slices(ovm)


def test_rejected_stores_keep_text_and_stack(ovm):
    check_rejected_stores(ovm)


def test_other_cells_keep_their_behaviour(ovm):
    check_cells_that_keep_their_behaviour(ovm)


def test_qkv_split_attention_and_join_against_numpy(ovm):
    check_qkv_script(ovm, 2, 5, 3, 4)
