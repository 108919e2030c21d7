"""`sum avg std norm` with an axis mask on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so, where Tensor::reduce_axes is
one t4k_reduce_axes call plus the word's element-wise sqrt / division): the rows of tests/test_axis_words_oracle.py within the same
float64 witnesses, the printed text = the oracle VM's, launch counts that do not depend on N, and a standardisation script chaining
`avg - std /` on a batch."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt
import test_axis_words_oracle as rows
from test_bcast_words_oracle import depth
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


@pytest.mark.parametrize("word", rows.WORDS)
@pytest.mark.parametrize("d,mask,text", rows.TABLE + rows.MORE, ids=rows.IDS(rows.TABLE + rows.MORE))
def test_table_rows(vm, d, mask, text, word):
    rows.check_row(vm, d, mask, word)


@pytest.mark.parametrize("word", rows.WORDS)
@pytest.mark.parametrize("d,mask", [(("t", 128, 8, 8, 3), 14), (("t", 128, 8, 8, 3), 7), (("m", 300, 257), 4), (("m", 300, 257), 2), (("v", 70000), 4)])
def test_larger_operands(vm, d, mask, word):
    rows.check_row(vm, d, mask, word)


def test_result_names(vm):
    rows.check_names(vm, rows.TABLE + rows.MORE)


def test_rejected_masks_keep_text_and_stack(vm):
    rows.check_rejected(vm)


def test_scalar_or_model_beneath_the_mask_is_a_noop(vm):
    rows.check_noops(vm)


def test_scalar_forms_unchanged(vm):
    rows.check_scalar_forms(vm)


def test_centre_planes_against_numpy(vm):
    rows.check_centre(vm)
    rows.check_centre(vm, ("t", 128, 8, 8, 3))


def script():
    lines = []
    for d, mask, _ in rows.TABLE + rows.MORE:
        for word in rows.WORDS:
            lines.append("%s gradfill 1 += %d %s . cr\ndrop" % (ctor(d), mask, word))
    lines += ["2 3 matrix ones 0 sum depth . cr\ndrop", "2 3 matrix ones 16 norm depth . cr\ndrop", "2 3 matrix ones 2.5 avg depth . cr\ndrop",
              "5 3 sum . . cr", "2 3 4 3 tensor gradfill 6 avg - . cr\ndrop drop"]
    return "\n".join(lines) + "\n"


def test_words_print_what_the_oracle_vm_prints(vm, ovm):
    src = script()
    own, ref = vm.eval(src), ovm.eval(src)
    assert own.count("] = {") >= 4 * len(rows.TABLE + rows.MORE) and own.count("axes 1..15?") == 3
    bad = compare(own, ref)
    assert not bad, bad


def launches(t4k, vm, src):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    l0 = int(t4k.lib.t4k_launch_count())
    vm.eval(src)
    return int(t4k.lib.t4k_launch_count()) - l0


@pytest.mark.parametrize("word,want", [("sum", 1), ("norm", 2), ("avg", 2), ("std", 5)])
@pytest.mark.parametrize("mask", [6, 7, 1])
def test_launches_of_a_word_do_not_depend_on_n(vm, t4k, word, want, mask):
    """the reduce, plus sqrt (norm), plus the division (avg); std = avg, the reduce, sqrt, the division"""
    counts = []
    for N in (2, 128):
        vm.eval("%d 4 4 3 tensor ones" % N)
        counts.append(launches(t4k, vm, "%d %s" % (mask, word)))
        vm.eval("drop drop")
    assert counts == [want, want], counts


def test_standardisation_script_on_a_batch(vm):
    """T 14 avg - 14 std / : centre every channel of a (128,8,8,3) batch and divide by the channel's std, no loop and no scalar read back"""
    rng = np.random.default_rng(14)
    T = (rng.standard_normal((128, 8, 8, 3)) * np.array([0.5, 2.0, 7.0]) + np.array([3.0, -1.0, 0.25])).astype(np.float32)
    cnt = 128 * 8 * 8
    d0 = depth(vm)
    vm.store(T, "128 8 8 3 tensor")
    A = vm.fetch("14 avg")                                              # T A
    D = vm.fetch("-")                                                   # T A D
    DA = vm.fetch("14 avg"); vm.eval("drop")                            # the centre `std` takes: the same call, the same bits
    S = vm.fetch("14 std")                                              # T A D S
    Z = vm.fetch("/")                                                   # T A D S Z
    assert depth(vm) == d0 + 5
    vm.eval("drop drop drop drop drop")
    assert depth(vm) == d0
    assert A.shape == S.shape == (1, 1, 1, 3) and D.shape == Z.shape == T.shape
    rows.check_value("avg", T, 14, A)
    assert np.array_equal(D, T - A)
    rows.check_value("std", D, 14, S, DA)
    q = wt.f64(D) / wt.f64(S)
    wt.check("D / S", Z, wt.W(q, np.abs(q), 1, 1.0))
    z = wt.f64(Z)                                                       # what the script is for: centred channels whose reference-style std is 1
    assert np.all(np.abs(z.mean((0, 1, 2))) < 1e-4 * np.abs(z).mean((0, 1, 2)) * cnt ** 0.5)
    assert np.allclose(np.sqrt((z * z).sum((0, 1, 2))) / cnt, 1.0, rtol=1e-5)
