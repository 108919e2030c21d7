"""The linear-algebra words in the blocked regime of csrc/linalg_batched.hip on the product VM: `inverse`, `luinv`, `plu`, `upper`,
`lower`, `det` and `solve` on a batch T4[2,201,201,1] (the rows and bars of tests/test_linalg_batched_words_oracle.py at the first K every entry
runs blocked), and the rank-2 words on one 201 x 201 matrix, which reach the same kernels as a batch of one.  Results are bit-equal to the C-ABI
entries on the same operand, launches do not depend on N, and a singular matrix prints the rank-2 word's own line."""
import ctypes

import numpy as np
import pytest

import test_linalg_batched_words_oracle as rows
from test_gpu_parity import Dev, p

pytestmark = pytest.mark.gpu
K = 201
I8 = ctypes.c_int * 8


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=1)
    yield v
    v.close()


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    for entry in range(4):
        out = I8()
        assert t4k.lib.t4k_linalg_batched_plan(entry, K, 2, 1, out) == 0 and out[0] == 3, (entry, list(out))
    return Dev(t4k)


def cabi(t4k, dev, name, A):
    """X (inverse, lu_inverse), LU (plu) or det of the batch A through the C-ABI entry"""
    N = len(A); dA, dX, dpiv, dst, dd = dev.up(A), dev.zeros(A.shape), dev.zeros(N * K, dev.torch.int32), dev.zeros(N, dev.torch.int32), dev.zeros(N)
    if name == "inverse": t4k.call("t4k_inverse_batched", p(dA), p(dX), K, N, p(dst), None)
    elif name == "luinv": t4k.call("t4k_lu_inverse_batched", p(dA), p(dX), p(dpiv), K, N, p(dst), None)
    elif name == "plu":   t4k.call("t4k_plu_batched", p(dA), p(dX), p(dpiv), K, N, p(dst), None)
    else:                 t4k.call("t4k_det_batched", p(dA), p(dpiv), K, N, p(dd), p(dst), None)
    return dev.down(dd) if name == "det" else dev.down(dA) if name == "plu" else dev.down(dX)


def test_words_on_a_batch_hold_the_bars(vm, dev):
    rows.check_unary_words(vm, 2, K)
    rows.check_solve(vm, 2, K, ("t", 3))


@pytest.mark.parametrize("word", ("inverse", "luinv", "plu", "det"))
@pytest.mark.parametrize("rank2", (False, True))
def test_words_give_the_bits_of_the_c_abi(vm, t4k, dev, word, rank2):
    _, A = rows.make_batch(77, 1 if rank2 else 2, K)
    if word == "det":
        A = np.stack([rows.normalised(a) for a in A])
    want = cabi(t4k, dev, word, A)
    d0 = rows.depth(vm)
    if rank2:
        vm.store(A[0], "%d %d matrix" % (K, K))
    else:
        rows.push_batch(vm, A)
    if rank2 and word == "det":
        got = np.float32(vm.eval("det .").split()[0])                                      # a printed scalar: to its printed digits
        assert abs(got - want[0]) <= 1e-3 * abs(want[0]), (got, want)
    else:
        assert np.array_equal(vm.fetch(word).reshape(want.shape), want), word
    vm.eval(" ".join(["drop"] * (rows.depth(vm) - d0)))


def test_launches_do_not_depend_on_the_batch(vm, t4k, dev):
    for word in ("inverse", "luinv", "plu", "det"):
        counts = []
        for N in (1, 3):
            _, A = rows.make_batch(5, N, K)
            rows.push_batch(vm, A)
            d0 = rows.depth(vm)
            l0 = int(t4k.lib.t4k_launch_count())
            vm.eval(word)
            counts.append(int(t4k.lib.t4k_launch_count()) - l0)
            vm.eval(" ".join(["drop"] * (rows.depth(vm) - d0 + 1)))
        assert counts[0] == counts[1] and counts[0] >= 1, (word, counts)


def test_a_singular_rank2_matrix_prints_the_words_own_line(vm, dev):
    _, A = rows.make_batch(9, 1, K, kinds=("dominant",))
    A[0][:, 40] = 0.0                                                                      # inside the second panel
    for word, line in (("inverse", "tensor#inverse: singular matrix at column 40"), ("luinv", "tensor#plu: singular at column 40"),
                       ("plu", "tensor#plu: singular at column 40")):
        d0 = rows.depth(vm)
        vm.store(A[0], "%d %d matrix" % (K, K))
        out = vm.eval(word)
        assert line in out and " entry" not in out, (word, out)
        vm.eval(" ".join(["drop"] * (rows.depth(vm) - d0)))
