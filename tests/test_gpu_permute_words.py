"""`transpose` with an axis order on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so, where Tensor::permute is one
t4k_permute call): the rows and scripts of tests/test_permute_words_oracle.py with the same exact comparison, the printed text = the
oracle VM's, one launch per word for 2 entries and for 128, and the multi-head attention script on a (128,16,4,8) batch."""
import ctypes

import pytest

import test_permute_words_oracle as rows
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


@pytest.mark.parametrize("perm", rows.ORDERS, ids=[rows.word(p) for p in rows.ORDERS])
@pytest.mark.parametrize("shape", rows.SHAPES, ids=["x".join(map(str, s)) for s in rows.SHAPES])
def test_every_order(vm, shape, perm):
    rows.check_order(vm, shape, perm)


def test_8241_is_the_tensor_word(vm):
    rows.check_8241_is_the_tensor_word(vm)
    rows.check_8241_is_the_tensor_word(vm, (128, 9, 7, 1))


def test_rejected_orders_keep_text_and_stack(vm):
    rows.check_rejected(vm)


def test_other_cells_beneath_the_scalar_keep_their_text(vm):
    rows.check_other_cells_keep_their_text(vm)


def test_multi_head_attention_script_against_numpy(vm):
    rows.check_multi_head_attention(vm, 2, 5, 3, 4)


def test_channel_first_batch_script_against_numpy(vm):
    rows.check_channel_first_batch(vm, 2, 3, 5, 4)
    rows.check_channel_first_batch(vm, 16, 3, 33, 65)


def script():
    lines = ["2 3 4 5 tensor gradfill %s transpose . cr\ndrop drop" % rows.word(p) for p in rows.ORDERS]
    lines += ["3 1 4 1 tensor gradfill 1248 transpose . cr\ndrop drop"]
    lines += ["2 3 2 3 tensor ones %s transpose depth . cr\ndrop" % p for p in rows.REJECTED]
    lines += ["2 3 matrix ones 8241 transpose . cr\ndrop", "5 vector ones 8241 transpose . cr\ndrop", "7 8241 transpose . . cr"]
    return "\n".join(lines) + "\n"


def test_word_prints_what_the_oracle_vm_prints(vm, ovm):
    src = script()
    own, ref = vm.eval(src), ovm.eval(src)
    assert own.count("] = {") >= 25 and own.count("transpose: axes 8421?") == len(rows.REJECTED) and own.count("tensor2?") == 3
    bad = compare(own, ref)
    assert not bad, bad


def launches(t4k, vm, src):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    l0 = int(t4k.lib.t4k_launch_count())
    vm.eval(src)
    return int(t4k.lib.t4k_launch_count()) - l0


@pytest.mark.parametrize("p", ["8421", "8241", "8412", "8142", "8214", "1248", "4821"])
def test_one_launch_whatever_n_is(vm, t4k, p):
    counts = []
    for N in (2, 128):
        vm.eval("%d 6 5 3 tensor ones" % N)
        counts.append(launches(t4k, vm, "%s transpose" % p))
        vm.eval("drop drop")
    assert counts == [1, 1], counts


def test_existing_forms_keep_their_one_launch(vm, t4k):
    """`T transpose` with the tensor on top: rank 4 one t4k_transpose_batched launch; rank 2 the deep copy that makes T' and one
    t4k_transpose launch, as before"""
    vm.eval("128 6 5 3 tensor ones")
    assert launches(t4k, vm, "transpose") == 1
    vm.eval("drop drop 6 5 matrix ones")
    assert launches(t4k, vm, "transpose") == 2
    vm.eval("drop drop")


def test_multi_head_attention_script_on_a_batch(vm):
    rows.check_multi_head_attention(vm, 128, 16, 4, 8)
