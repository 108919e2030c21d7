"""`softmax` with an axis mask ( T m -- T ) (DESIGN.md 3.12 "Beyond the reference: axis softmax") on the CPU oracle VM - the product's host
sources over the oracle's C-ABI, which has no t4k_softmax_axes, so Tensor::softmax_axes gathers every group into a temporary row with
t4k_copy, takes it through t4k_softmax and copies it back here.

Every (operand, mask) row of the axis-reduction table (tests/test_axis_words_oracle.py, the non-adjacent masks 10 and 5 among them): T is
rewritten in place with its shape, the mask is consumed and nothing is pushed; values against tests/f64_witness.py `softmax` after moving
the masked axes last (the project's derived bound, nothing measured), every group's stored values summing to 1 within len * 2^-24.
`T 15 softmax` against `T softmax`; the rejected masks keeping their text and T; a scalar or a model beneath the mask keeping today's
text; an attention script `Q K' @ scale *= 2 softmax V @` against NumPy, with one head and with two heads in C.
tests/test_gpu_softmax_axes_words.py runs the same checks on the product VM."""
import os
import zlib

import numpy as np
import pytest

import f64_witness as wt
import test_axis_words_oracle as axis_rows
from test_bcast_words_oracle import depth
from test_bmm_words_oracle import ctor, nhwc
from vm_util import ROOT, OracleVM

ROWS = [(d, m) for d, m, _ in axis_rows.TABLE + axis_rows.MORE]
IDS = axis_rows.IDS(axis_rows.TABLE + axis_rows.MORE)
RTOL, ATOL = 2e-4, 2.5e-4                                               # vm_util.compare's tolerances


def axes_of(mask):
    return tuple(i for i in range(4) if mask & (8 >> i))


def witness(A, mask, extra=0.0):
    """f64_witness.softmax of A (N,H,W,C) along the masked axes, back in A's layout; `extra` more ulps on every element"""
    ax = axes_of(mask)
    keep = [i for i in range(4) if i not in ax]
    perm = keep + list(ax)
    P = np.asarray(A).transpose(perm)
    rows = P.reshape(P.shape[:len(keep)] + (-1,))
    w = wt.softmax(rows)
    back = lambda x: np.broadcast_to(x, rows.shape).reshape(P.shape).transpose(np.argsort(perm))
    return wt.W(back(w.exact), back(w.mag), back(w.n) + extra, 1.0)


def group_sums(R, mask):
    ax = axes_of(mask)
    return wt.f64(R).sum(ax), int(np.prod([R.shape[i] for i in ax]))


def check_values(name, A, mask, R, extra=0.0):
    assert R.shape == A.shape, (R.shape, A.shape)
    wt.check(name, R, witness(A, mask, extra), kind="softmax")
    s, cnt = group_sums(R, mask)
    assert np.all(np.abs(s - 1.0) <= cnt * wt.U), (name, float(np.max(np.abs(s - 1.0))), cnt)


def logits(rng, shape, scale=2.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def check_row(vm, d, mask, scale=2.0):
    """stores logits of d, runs `mask softmax`: the mask is consumed, T stays and is rewritten, nothing is pushed"""
    rng = np.random.default_rng(zlib.crc32(repr((d, mask, "softmax")).encode()))
    A = logits(rng, nhwc(d), scale)
    d0 = depth(vm)
    vm.store(A, ctor(d))
    out = vm.eval("%d softmax" % mask)
    assert "no param" not in out and "axes" not in out, out
    assert depth(vm) == d0 + 1, (d, mask)
    R = vm.fetch(None)
    vm.eval("drop")
    assert depth(vm) == d0
    check_values("softmax %s mask %d" % (d, mask), A, mask, R)
    return A, R


def check_all_axes_is_the_tensor_word(vm, d=("t", 2, 3, 4, 3)):
    """`T 15 softmax` means what `T softmax` means: both inside the witness of the flattened tensor, so within twice its bound of each other"""
    rng = np.random.default_rng(15)
    A = logits(rng, nhwc(d))
    d0 = depth(vm)
    vm.store(A, ctor(d)); R15 = vm.fetch("15 softmax"); vm.eval("drop")
    vm.store(A, ctor(d)); R = vm.fetch("softmax"); vm.eval("drop")
    assert depth(vm) == d0
    w = witness(A, 15)
    wt.check("T 15 softmax", R15, w); wt.check("T softmax", R, w)
    assert np.all(np.abs(wt.f64(R15) - wt.f64(R)) <= 2.0 * w.bound())


REJECTED = ["0", "16", "2.5"]


def check_rejected(vm):
    for m in REJECTED:
        d0 = depth(vm)
        vm.eval("2 3 matrix ones")
        out = vm.eval("%s softmax" % m)
        assert "softmax: axes 1..15?\n" in out, (m, out)
        assert depth(vm) == d0 + 1, m                                   # the mask is consumed, nothing is pushed
        assert np.array_equal(vm.fetch(None), np.ones((1, 2, 3, 1), np.float32))
        vm.eval("drop")


def check_other_cells_keep_their_text(vm):
    """a scalar or a model beneath the mask: the word prints what it printed and moves nothing"""
    d0 = depth(vm)
    out = vm.eval("5 3 softmax")
    assert "( N -- ) no param needed!" in out and "axes" not in out, out
    assert depth(vm) == d0 + 2
    assert vm.eval(". .").split()[:2] == ["3", "5"]
    out = vm.eval("4 1 1 1 nn.model 6 softmax")
    assert "( N -- ) no param needed!" in out and "axes" not in out, out
    assert depth(vm) == d0 + 2
    assert vm.eval(".").split()[0] == "6"
    vm.eval("drop")
    assert depth(vm) == d0


def attention_numpy(Q, K, V, scale):
    """softmax(Q K' scale) V per entry n and head c, in float64 on the fp32 operands"""
    q, k, v = wt.f64(Q), wt.f64(K), wt.f64(V)
    s = np.einsum("nikc,njkc->nijc", q, k) * float(np.float32(scale))
    e = np.exp(s - s.max(2, keepdims=True))
    p = e / e.sum(2, keepdims=True)
    return p, np.einsum("nijc,njkc->nikc", p, v)


def check_attention(vm, N, L, D, C):
    """Q K' @ scale *= 2 softmax V @ on T4[N,L,D,C]: every word a batched one, no loop and nothing read back"""
    shape = "%d %d %d %d tensor" % (N, L, D, C)
    scale = 1.0 / np.sqrt(D)
    d0 = depth(vm)
    K = vm.fetch(shape + " rand")                                       # K
    vm.eval("transpose")                                                # K K'
    Q = vm.fetch(shape + " gradfill")                                   # K K' Q
    vm.eval("swap")                                                     # K Q K'
    P = vm.fetch("@ %.7f *= 2 softmax" % scale)                         # K Q K' P
    V = vm.fetch(shape + " rand")                                       # K Q K' P V
    O = vm.fetch("@")                                                   # K Q K' P V O
    assert depth(vm) == d0 + 6
    vm.eval("drop drop drop drop drop drop")
    assert depth(vm) == d0
    assert P.shape == (N, L, L, C) and O.shape == (N, L, D, C)
    p, o = attention_numpy(Q, K, V, scale)
    for name, got, want in (("P", P, p), ("O", O, o)):
        assert np.all(np.abs(wt.f64(got) - want) <= ATOL + RTOL * np.maximum(np.abs(got), np.abs(want))), (name, float(np.max(np.abs(got - want))))
    assert np.all(np.abs(wt.f64(P).sum(2) - 1.0) <= L * wt.U)


@pytest.fixture(scope="module")
def ovm():
    if not os.path.exists(os.path.join(ROOT, "oracle", "libten4_oracle.so")):
        pytest.skip("oracle/libten4_oracle.so not built")
    v = OracleVM(seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("d,mask", ROWS, ids=IDS)
def test_table_rows(ovm, d, mask):
    check_row(ovm, d, mask)


def test_logits_the_naive_form_overflows_on(ovm):
    check_row(ovm, ("t", 2, 3, 4, 3), 6, scale=3000.0)


def test_every_axis_is_the_tensor_word(ovm):
    check_all_axes_is_the_tensor_word(ovm)


def test_rejected_masks_keep_text_and_stack(ovm):
    check_rejected(ovm)


def test_scalar_or_model_beneath_the_mask_keeps_its_text(ovm):
    check_other_cells_keep_their_text(ovm)


@pytest.mark.parametrize("C", [1, 2])
def test_attention_script_against_numpy(ovm, C):
    check_attention(ovm, 2, 5, 3, C)
