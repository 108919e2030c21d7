"""The batched linear-algebra words on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so, where each Tensor::*_b method is one
t4k_*_batched launch): the rows of tests/test_linalg_batched_words_oracle.py with the same witnesses, a script of the new cases printing what
the CPU oracle VM prints (the comparison the golden tests use), and the launch count of `inverse` not depending on the batch."""
import ctypes

import numpy as np
import pytest

import test_linalg_batched_words_oracle as rows
from vm_util import OracleVM, compare

pytestmark = pytest.mark.gpu

BIG = [(128, 16), (5, 64), (3, 141), (2, 201)]              # (N, K): the workgroup and global regimes through the words


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("N,K", rows.UNARY + BIG)
def test_one_operand_words_on_a_batch(vm, N, K):
    rows.check_unary_words(vm, N, K)


@pytest.mark.parametrize("N,K,rhs", rows.SOLVE + [(128, 16, ("t", 4)), (4, 100, ("m", 7))])
def test_solve_on_a_batch(vm, N, K, rhs):
    rows.check_solve(vm, N, K, rhs)


@pytest.mark.parametrize("N,K,lhs", rows.MATDIV + [(128, 16, ("t", 4)), (4, 100, ("m", 7))])
def test_matdiv_on_a_batch(vm, N, K, lhs):
    rows.check_matdiv(vm, N, K, lhs)


def test_a_singular_entry_prints_one_line_and_the_others_are_right(vm):
    rows.check_singular_entry(vm)


@pytest.mark.parametrize("ops,word,text", rows.REJECTED)
def test_rejected_operands_keep_the_stack(vm, ops, word, text):
    rows.check_rejected(vm, ops, word, text)


# two diagonally dominant 3 x 3 entries with small integer entries: four printed decimals agree between the VMs
BATCH = "2 3 3 1 tensor ={ 8 1 2 1 9 3 2 1 7 6 2 1 1 7 2 3 1 9 }"
SINGULAR = "2 3 3 1 tensor ={ 8 1 2 1 9 3 2 1 7 1 2 3 2 4 6 1 1 1 } inverse drop drop"       # entry 1: row 1 = 2 x row 0


def new_cases_script():
    lines = [BATCH + " %s . cr\ndrop" % w for w in ("inverse", "luinv", "det")]
    lines += [BATCH + " plu . cr\ndrop . cr\ndrop", BATCH + " plu upper . cr\ndrop drop drop", BATCH + " plu lower . cr\ndrop drop drop"]
    lines += ["3 vector{ 1 2 3 } " + BATCH + " solve . cr\ndrop drop", "3 2 matrix{ 1 2 3 4 5 6 } " + BATCH + " solve . cr\ndrop drop",
              "2 3 2 1 tensor ={ 1 2 3 4 5 6 6 5 4 3 2 1 } " + BATCH + " solve . cr\ndrop drop",
              "2 3 matrix{ 1 2 3 4 5 6 } " + BATCH + " matdiv . cr\ndrop drop", "2 2 3 1 tensor ={ 1 2 3 4 5 6 6 5 4 3 2 1 } " + BATCH + " matdiv . cr\ndrop drop",
              "2 3 4 1 tensor ones inverse . cr\ndrop", "3 3 3 1 tensor ones " + BATCH + " solve . cr\ndrop drop"]          # the last two are rejected
    return "\n".join(lines) + "\n"


def test_new_cases_print_what_the_oracle_vm_prints(vm):
    src = new_cases_script()
    own, msg_own = vm.eval(src), vm.eval(SINGULAR)          # a singular entry's contents are unspecified: only its message is compared
    ovm = OracleVM(seed=1)
    try:
        ref, msg_ref = ovm.eval(src), ovm.eval(SINGULAR)
    finally:
        ovm.close()
    assert own.count("] = {") >= 12 and "tensor2?" in own and "batch dim?" in own
    bad = compare(own, ref)
    assert not bad, bad
    assert "singular matrix at column" in msg_own and " entry 1" in msg_own
    assert not compare(msg_own, msg_ref)


def test_launches_of_inverse_do_not_depend_on_the_batch(vm, t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    counts = []
    for N in (2, 64):
        _, A = rows.make_batch(5, N, 16)
        rows.push_batch(vm, A)
        l0 = int(t4k.lib.t4k_launch_count())
        vm.eval("inverse")
        counts.append(int(t4k.lib.t4k_launch_count()) - l0)
        vm.eval("drop drop")
    assert counts[0] == counts[1] and counts[0] >= 1, counts
