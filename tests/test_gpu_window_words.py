"""Box windows on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so, where Tensor::window is one t4k_window call and
the four-scalar `slice` of a valid window is that call too): the rows and the script of tests/test_window_words_oracle.py with the same
exact comparison, the printed text = the oracle VM's, one launch per word for 2 entries and for 128, and the Q/K/V script on a
(128,16,1,3*32) batch."""
import ctypes

import pytest

import test_window_words_oracle as rows
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


@pytest.mark.parametrize("mask", rows.MASKS, ids=rows.mask_id)
def test_slice_every_subset_of_axes(vm, mask):
    rows.check_slice(vm, rows.SHAPE, mask)


@pytest.mark.parametrize("mask", [0, 2, 4, 6], ids=rows.mask_id)
def test_slice_of_a_matrix_and_a_vector_keeps_the_rank(vm, mask):
    rows.check_slice(vm, (1, 5, 7, 1), mask, rank=2)
    if not mask & 2:
        rows.check_slice(vm, (1, 9, 1, 1), mask, rank=1)


def test_four_scalar_slice_equals_the_eight_scalar_one(vm):
    rows.check_four_equals_eight(vm)
    rows.check_four_equals_eight(vm, (1, 6, 7, 1), rank=2)
    rows.check_four_equals_eight(vm, (128, 28, 28, 1))


@pytest.mark.parametrize("mask", rows.MASKS, ids=rows.mask_id)
def test_store_every_subset_of_axes(vm, mask):
    rows.check_store(vm, rows.SHAPE, mask)


def test_store_into_a_matrix_and_a_vector(vm):
    rows.check_store(vm, (1, 5, 7, 1), 6, rank=2)
    rows.check_store(vm, (1, 9, 1, 1), 4, rank=1)


def test_slice_then_store_leaves_the_tensor_as_it_was(vm):
    rows.check_slice_then_store_is_identity(vm)


def test_stores_side_by_side_are_a_concatenation(vm):
    rows.check_concatenate(vm)


def test_rejected_slices_keep_text_and_stack(vm):
    rows.check_rejected_slices(vm)


def test_rejected_stores_keep_text_and_stack(vm):
    rows.check_rejected_stores(vm)


def test_other_cells_keep_their_behaviour(vm):
    rows.check_cells_that_keep_their_behaviour(vm)


def test_qkv_split_attention_and_join_against_numpy(vm):
    rows.check_qkv_script(vm, 2, 5, 3, 4)


def test_qkv_script_on_a_batch(vm):
    rows.check_qkv_script(vm, 128, 16, 4, 8)


REJECTED_SLICES = ["0 -1 2 2 0 -1 0 -1", "0 -1 0 -1 3 1 0 -1", "0 3 0 -1 0 -1 0 -1", "0 -1 0 -1 0 -1 -1 2", "0 -1 1.5 2 0 -1 0 -1"]
REJECTED_STORES = ["1 0 0 0", "0 3 0 0", "0 0 -1 0", "0 0 0 0.5"]


def script():
    lines = ["3 3 4 5 tensor gradfill %s slice . cr\ndrop" % rows.cut((3, 3, 4, 5), m)[1] for m in (0, 1, 6, 8, 15)]
    lines += ["2 3 4 5 tensor gradfill 1 3 0 2 slice . cr\ndrop", "4 5 matrix gradfill 1 3 0 2 slice . cr\ndrop"]
    lines += ["4 5 matrix gradfill 0 1 1 3 2 -1 0 1 slice . cr\ndrop", "7 vector gradfill 0 1 2 5 0 1 0 1 slice . cr\ndrop"]
    lines += ["2 3 4 5 tensor gradfill 2 2 2 2 tensor ones 0 1 2 3 t! . cr", "4 5 matrix gradfill 2 2 matrix ones 0 1 3 0 t! . cr",
              "7 vector gradfill 3 vector ones 0 4 0 0 t! . cr", "2 3 matrix gradfill 9.5 4 t! . cr"]
    lines += ["2 3 4 5 tensor ones %s slice depth . cr\ndrop" % r for r in REJECTED_SLICES]
    lines += ["2 3 4 5 tensor ones 2 2 3 5 tensor gradfill %s t! depth . cr\ndrop drop" % r for r in REJECTED_STORES]
    lines += ["2 3 4 5 tensor ones dup 0 0 0 0 t! depth . cr\ndrop drop", "7 1 2 3 4 5 6 7 8 slice . . . . . cr"]
    return "\n".join(lines) + "\n"


def test_words_print_what_the_oracle_vm_prints(vm, ovm):
    src = script()
    own, ref = vm.eval(src), ovm.eval(src)
    assert own.count("] = {") == 13 and own.count("slice: range?") == len(REJECTED_SLICES) and own.count("t!: range?") == len(REJECTED_STORES) + 1
    bad = compare(own, ref)
    assert not bad, bad


def launches(t4k, vm, src):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    l0 = int(t4k.lib.t4k_launch_count())
    vm.eval(src)
    return int(t4k.lib.t4k_launch_count()) - l0


WORDS = {"eight_scalar_slice": ("{n} 28 28 3 tensor ones", "0 -1 4 24 4 24 1 3 slice", "drop drop"),
         "eight_scalar_slice_of_n": ("{n} 28 28 3 tensor ones", "1 2 0 -1 0 -1 0 -1 slice", "drop drop"),
         "four_scalar_slice": ("{n} 28 28 1 tensor ones", "4 24 4 24 slice", "drop drop"),
         "four_scalar_slice_with_channels": ("{n} 9 7 3 tensor ones", "2 -1 1 8 slice", "drop drop"),
         "box_store": ("{n} 28 28 3 tensor ones {n} 20 20 2 tensor ones", "0 4 4 1 t!", "drop")}


@pytest.mark.parametrize("word", list(WORDS))
def test_one_launch_whatever_n_is(vm, t4k, word):
    make, run, clean = WORDS[word]
    counts = []
    for N in (2, 128):
        vm.eval(make.format(n=N))
        counts.append(launches(t4k, vm, run))
        vm.eval(clean)
    assert counts == [1, 1], counts
