"""`transpose` of a batch and the broadcast arithmetic words on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so, where
Tensor::ten_bcast is one t4k_tt_op_bcast launch and Tensor::transpose of a rank-4 tensor one t4k_transpose_batched launch): the rows of
tests/test_bcast_words_oracle.py, `+ - *` bit for bit against NumPy and `/` against the CPU oracle VM's result within one rounding
(tests/f64_witness.py), the printed text = the oracle VM's, launch counts that do not depend on N, and a least-squares script chaining
`transpose` `@` `solve` on a batch."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt
import test_bcast_words_oracle as rows
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


@pytest.mark.parametrize("word", ["+", "-", "*", "+=", "*="])
@pytest.mark.parametrize("a,b", rows.ROWS, ids=rows.IDS(rows.ROWS))
def test_table_rows_equal_numpy(vm, a, b, word):
    rows.check_row(vm, a, b, word)


@pytest.mark.parametrize("word", ["/", "/="])
@pytest.mark.parametrize("a,b", rows.ROWS, ids=rows.IDS(rows.ROWS))
def test_table_rows_quotient_against_the_oracle_vm(vm, ovm, a, b, word):
    _, _, got = rows.check_row(vm, a, b, word, exact_div=False)
    _, _, ref = rows.check_row(ovm, a, b, word)                         # the same seeded operands
    wt.check("%s %s %s" % (a, word, b), got, wt.W(wt.f64(ref), np.abs(wt.f64(ref)), 1, 1.0))


@pytest.mark.parametrize("word", ["+", "-", "*", "/", "*="])
@pytest.mark.parametrize("a,b", rows.N_ROWS, ids=rows.IDS(rows.N_ROWS))
def test_equal_hwc_n_broadcast_keeps_its_result(vm, ovm, a, b, word):
    _, _, got = rows.check_n_row(vm, a, b, word)
    _, _, ref = rows.check_n_row(ovm, a, b, word)
    wt.check("%s %s %s" % (a, word, b), got, wt.W(wt.f64(ref), np.abs(wt.f64(ref)), 1 if word[0] == "/" else 0, 1.0))


def test_result_rank(vm):
    rows.check_result_names(vm)


@pytest.mark.parametrize("N,H,W,C", rows.TRANSPOSE + [(128, 64, 64, 1), (3, 130, 63, 3)])
def test_transpose_of_a_batch_and_back(vm, N, H, W, C):
    rows.check_transpose(vm, N, H, W, C)


@pytest.mark.parametrize("a,b,text,pushed", rows.REJECTED)
def test_rejected_pairs_keep_text_and_stack(vm, a, b, text, pushed):
    rows.check_rejected(vm, a, b, text, pushed)


def new_cases_script():
    lines = []
    for i, (a, b) in enumerate(rows.ROWS[:23]):
        lines.append("%s gradfill 1 += %s gradfill 2 += %s . cr\ndrop drop" % (ctor(a), ctor(b), "+-*/"[i % 4]))
    lines += ["2 3 3 1 tensor ={ 8 1 2 1 9 3 2 1 7 6 2 1 1 7 2 3 1 9 } transpose . cr\ndrop", "2 2 3 2 tensor gradfill transpose . cr\ndrop",
              "3 vector transpose\ndrop", "2 3 matrix ones 3 3 matrix ones + depth . cr\ndrop drop", "5 vector ones 4 vector ones * depth . cr\ndrop drop",
              "2 2 3 1 tensor ones 3 2 2 1 tensor ones + . cr\ndrop drop"]
    return "\n".join(lines) + "\n"


def test_new_cases_print_what_the_oracle_vm_prints(vm, ovm):
    src = new_cases_script()
    own, ref = vm.eval(src), ovm.eval(src)
    assert own.count("] = {") >= 25 and "tensor2?" in own and own.count("} dim?") == 2 and "tensor#ten_op" in own
    bad = compare(own, ref)
    assert not bad, bad


def launches(t4k, vm, src):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    l0 = int(t4k.lib.t4k_launch_count())
    vm.eval(src)
    return int(t4k.lib.t4k_launch_count()) - l0


@pytest.mark.parametrize("word,other", [("+", "1 4 4 1 tensor"), ("*", "%d 1 1 1 tensor"), ("-", "4 4 matrix"), ("/", "1 4 matrix"), ("transpose", None)])
def test_launches_of_a_word_do_not_depend_on_n(vm, t4k, word, other):
    counts = []
    for N in (2, 128):
        vm.eval("%d 4 4 1 tensor ones" % N)
        if other:
            vm.eval((other % N if "%" in other else other) + " ones")
        counts.append(launches(t4k, vm, word))
        vm.eval("drop drop" + (" drop" if other else ""))
    assert counts[0] == counts[1] and counts[0] >= 1, counts


def lstsq_bound(A, b, AtA, Atb, Inv, x):
    """|x - x64| for the normal equations, x64 the float64 least-squares solution of the fp32 (A, b).  With G = A^T A and g = A^T b in
    float64, x - x64 = G^-1 (G x - g), and G x - g = (G - AtA) x + (AtA x - Atb) + (Atb - g): two fp32 dot products of length M
    (2 M u |A^T||A| and 2 M u |A^T||b|, the bound tests/test_bmm_words_oracle.py holds `@` to) and the residual of `solve` =
    luinv then @ ((C_LINALG rho + 2) K u |AtA||Inv||Atb|: the inverse_residual bound of tests/f64_witness.py on AtA Inv - I, plus
    the product's own rounding).  Element-wise through |G^-1|."""
    M, K = A.shape
    A64, b64 = wt.f64(A), wt.f64(b)
    rho, _ = wt.pivot_growth(AtA)
    r = 2 * M * wt.U * (np.abs(A64.T) @ np.abs(A64)) @ np.abs(wt.f64(x)) + 2 * M * wt.U * np.abs(A64.T) @ np.abs(b64) \
        + (wt.C_LINALG * rho + 2) * K * wt.U * np.abs(wt.f64(AtA)) @ np.abs(wt.f64(Inv)) @ np.abs(wt.f64(Atb))
    return np.abs(np.linalg.inv(A64.T @ A64)) @ r


def test_least_squares_script_on_a_batch(vm):
    """7 well-conditioned 5 x 3 problems min |A x - b|: x = solve(A^T A, A^T b), A^T from the batched `transpose`"""
    rng = np.random.default_rng(31)
    N, M, K = 7, 5, 3
    A = np.stack([np.linalg.qr(rng.standard_normal((M, K)))[0] * np.array([1.0, 1.5, 2.0]) + 0.05 * rng.standard_normal((M, K)) for _ in range(N)]).astype(np.float32)
    b = rng.standard_normal((N, M, 1)).astype(np.float32)
    d0 = rows.depth(vm)
    vm.store(b, "%d %d 1 1 tensor" % (N, M))                            # b
    vm.store(A, "%d %d %d 1 tensor" % (N, M, K))                        # b A
    At = vm.fetch("transpose")                                          # b A At
    assert np.array_equal(At.reshape(N, K, M), A.transpose(0, 2, 1))
    Atb = vm.fetch("rot @")                                             # A At b Atb
    AtA = vm.fetch("swap drop -rot swap @")                             # Atb At A AtA   (`@` keeps its operands)
    assert Atb.shape == (N, K, 1, 1) and AtA.shape == (N, K, K, 1)
    Inv = vm.fetch("luinv"); vm.eval("drop")
    x = vm.fetch("swap drop swap drop solve")                           # Atb AtA x
    assert x.shape == (N, K, 1, 1)
    vm.eval("drop drop drop")
    assert rows.depth(vm) == d0
    for n in range(N):
        wt.inverse_check("luinv(AtA) entry %d" % n, AtA[n, :, :, 0], Inv[n, :, :, 0])
        x64 = np.linalg.lstsq(wt.f64(A[n]), wt.f64(b[n]), rcond=None)[0]
        bound = lstsq_bound(A[n], b[n], AtA[n, :, :, 0], Atb[n, :, :, 0], Inv[n, :, :, 0], x[n, :, :, 0])
        err = np.abs(wt.f64(x[n, :, :, 0]) - x64)
        assert np.all(err <= bound), (n, float(np.max(err / bound)))
