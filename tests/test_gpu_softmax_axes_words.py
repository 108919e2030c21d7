"""`softmax` with an axis mask on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so, where Tensor::softmax_axes is one
t4k_softmax_axes call): the checks of tests/test_softmax_axes_words_oracle.py within the same float64 witness, the printed text = the
oracle VM's, a launch count that does not depend on N and equals the documented one, and the attention script on a (128,16,8,4) batch."""
import ctypes

import pytest

import test_softmax_axes_words_oracle as rows
from test_bmm_words_oracle import ctor
from vm_util import OracleVM, compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=1)
    yield v
    v.close()


@pytest.fixture(scope="module")
def ovm():
    v = OracleVM(seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("d,mask", rows.ROWS, ids=rows.IDS)
def test_table_rows(vm, d, mask):
    rows.check_row(vm, d, mask)


@pytest.mark.parametrize("d,mask", [(("t", 128, 8, 8, 3), 6), (("t", 128, 8, 8, 3), 14), (("m", 300, 257), 2), (("m", 300, 257), 4), (("v", 70000), 4)])
def test_larger_operands(vm, d, mask):
    rows.check_row(vm, d, mask)


def test_logits_the_naive_form_overflows_on(vm):
    rows.check_row(vm, ("t", 2, 3, 4, 3), 6, scale=3000.0)


def test_every_axis_is_the_tensor_word(vm):
    rows.check_all_axes_is_the_tensor_word(vm)


def test_rejected_masks_keep_text_and_stack(vm):
    rows.check_rejected(vm)


def test_scalar_or_model_beneath_the_mask_keeps_its_text(vm):
    rows.check_other_cells_keep_their_text(vm)


def script():
    lines = ["%s gradfill %d softmax . cr\ndrop" % (ctor(d), mask) for d, mask in rows.ROWS]
    lines += ["2 3 matrix ones 0 softmax depth . cr\ndrop", "2 3 matrix ones 16 softmax depth . cr\ndrop", "2 3 matrix ones 2.5 softmax depth . cr\ndrop",
              "5 3 softmax . . cr", "2 3 4 3 tensor gradfill 15 softmax . cr\ndrop"]
    return "\n".join(lines) + "\n"


def test_word_prints_what_the_oracle_vm_prints(vm, ovm):
    src = script()
    own, ref = vm.eval(src), ovm.eval(src)
    assert own.count("] = {") >= len(rows.ROWS) and own.count("axes 1..15?") == 3 and own.count("no param needed!") == 1
    bad = compare(own, ref)
    assert not bad, bad


def launches(t4k, vm, src):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    l0 = int(t4k.lib.t4k_launch_count())
    vm.eval(src)
    return int(t4k.lib.t4k_launch_count()) - l0


@pytest.mark.parametrize("mask", [1, 2, 6, 7, 5])
def test_one_launch_whatever_n_is(vm, t4k, mask):
    """a lane's share of a group fits its registers here: the word is one kernel, for 2 entries and for 128"""
    counts = []
    for N in (2, 128):
        vm.eval("%d 4 4 3 tensor ones" % N)
        counts.append(launches(t4k, vm, "%d softmax" % mask))
        vm.eval("drop")
    assert counts == [1, 1], counts


def test_attention_script_on_a_batch(vm):
    rows.check_attention(vm, 128, 16, 8, 4)
