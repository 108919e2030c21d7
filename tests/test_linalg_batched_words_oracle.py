"""`inverse` `luinv` `plu` `upper` `lower` `det` `solve` `matdiv` on a batch T4[N,K,K,1] (DESIGN.md 3.8 "Beyond the reference: batched linear
algebra") on the CPU oracle VM - the product's host sources over the oracle's C-ABI, which has no t4k_*_batched entries, so the Tensor::*_b
methods take their per-matrix loops here.

Every row of the word table: result shape, stack depth, values by the witnesses of tests/f64_witness.py (solve / matdiv: against the float64
product of the fp32 inverse the VM's own `luinv` returns with the fp32 right-hand side, within 2 K 2^-24 (|Inv| |B|), and `luinv` itself by
inverse_check).  Rejected operands keep their text and the stack; rank <= 2 operands print what the reference's VM prints
(oracle/_ref/ten4_refhost, build container only).  tests/test_gpu_linalg_batched_words.py runs the same rows on the product VM."""
import os
import subprocess
import sys

import numpy as np
import pytest

import f64_witness as wt
import small_kernel_cases as sk
from vm_util import GOLDEN, ROOT, SCRIPTS, TEN4_ORACLE, OracleVM, compare, run_vm

REFHOST = os.path.join(ROOT, "oracle", "_ref", "ten4_refhost")
KINDS = ("dominant", "permuted", "cond1e4")
UNARY = [(1, 3), (2, 4), (7, 5), (3, 16), (2, 33)]          # (N, K)


@pytest.fixture(scope="module")
def ovm():
    if not os.path.exists(os.path.join(ROOT, "oracle", "libten4_oracle.so")):
        pytest.skip("oracle/libten4_oracle.so not built")
    v = OracleVM(seed=1)
    yield v
    v.close()


def depth(vm):
    return int(vm.eval("depth .").split()[0])


def make_batch(seed, N, K, kinds=KINDS):
    rng = np.random.default_rng(seed)
    ks = [kinds[(K + i) % len(kinds)] for i in range(N)]
    return ks, np.stack([sk.matrix(rng, K, k) for k in ks])


def normalised(A):
    K = A.shape[0]
    _, l64 = np.linalg.slogdet(A.astype(np.float64))
    return (A.astype(np.float64) / np.exp(l64 / K)).astype(np.float32)


def push_batch(vm, A):
    N, K = A.shape[0], A.shape[1]
    vm.store(A, "%d %d %d 1 tensor" % (N, K, K))


def perm_from(Pm):
    """row order of an exact permutation matrix"""
    assert set(np.unique(Pm)) <= {0.0, 1.0} and np.all(Pm.sum(0) == 1) and np.all(Pm.sum(1) == 1)
    return np.argmax(Pm, axis=1)


def check_unary_words(vm, N, K):
    kinds, A = make_batch(100 + N * 37 + K, N, K)
    d0 = depth(vm)
    push_batch(vm, A)
    for word in ("inverse", "luinv"):
        X = vm.fetch(word)
        assert X.shape == (N, K, K, 1) and depth(vm) == d0 + 2, (word, X.shape)
        for n in range(N):
            wt.inverse_check("%s N=%d K=%d entry %d %s" % (word, N, K, n, kinds[n]), A[n], X[n, :, :, 0])
        vm.eval("drop")
    LU = vm.fetch("plu")                                                            # ( A -- A P LU )
    assert LU.shape == (N, K, K, 1) and depth(vm) == d0 + 3
    U = vm.fetch("upper"); vm.eval("drop")
    L = vm.fetch("lower"); vm.eval("drop drop")
    Pm = vm.fetch(None); vm.eval("drop")
    assert Pm.shape == (N, K, K, 1) and depth(vm) == d0 + 1
    for n in range(N):
        lu = LU[n, :, :, 0]; perm = perm_from(Pm[n, :, :, 0]); Lf, Uf = wt.split_lu(lu)
        wt.check("plu N=%d K=%d entry %d %s" % (N, K, n, kinds[n]), Lf @ Uf, wt.W(wt.f64(A[n])[perm], np.abs(Lf) @ np.abs(Uf), K, wt.C_SUM))
        wt.equal("upper", U[n, :, :, 0], wt.lu_extract(lu, 1).exact); wt.equal("lower", L[n, :, :, 0], wt.lu_extract(lu, 0).exact)
    assert np.array_equal(vm.fetch(None).reshape(A.shape), A)                       # the operand is intact
    vm.eval("drop")
    An = np.stack([normalised(a) for a in A])                                       # |det| ~ 1: every determinant is an fp32 number
    push_batch(vm, An)
    D = vm.fetch("det")
    assert D.size == N and D.shape[1] == N and depth(vm) == d0 + 2, D.shape         # a VECTOR of N
    for n in range(N):
        s64, l64 = np.linalg.slogdet(An[n].astype(np.float64)); d = float(D.ravel()[n])
        assert np.sign(d) == s64 and abs(np.log(abs(d)) - l64) <= 1e-3 * max(1.0, abs(l64)), (N, K, n, d, s64, l64)
    vm.eval("drop drop")
    assert depth(vm) == d0


@pytest.mark.parametrize("N,K", UNARY)
def test_one_operand_words_on_a_batch(ovm, N, K):
    check_unary_words(ovm, N, K)


SOLVE = [(2, 4, ("t", 3)), (7, 5, ("t", 1)), (3, 16, ("m", 6)), (2, 6, ("v",)), (1, 3, ("t", 2)), (1, 4, ("v",))]     # N, K, right-hand side


def check_solve(vm, N, K, rhs):
    kinds, A = make_batch(200 + N * 37 + K, N, K)
    rng = np.random.default_rng(N * 11 + K)
    d0 = depth(vm)
    if rhs[0] == "t":
        P = rhs[1]; B = rng.standard_normal((N, K, P)).astype(np.float32); ctor = "%d %d %d 1 tensor" % (N, K, P)
    elif rhs[0] == "m":
        P = rhs[1]; B = rng.standard_normal((K, P)).astype(np.float32); ctor = "%d %d matrix" % (K, P)
    else:
        P = 1; B = rng.standard_normal((K, 1)).astype(np.float32); ctor = "%d vector" % K
    vm.store(B, ctor)
    push_batch(vm, A)
    Inv = vm.fetch("luinv").reshape(N, K, K); vm.eval("drop")
    for n in range(N):
        wt.inverse_check("luinv for solve entry %d" % n, A[n], Inv[n])
    X = vm.fetch("solve")                                                           # ( B A -- B A X )
    assert X.shape == (N, K, P, 1) and depth(vm) == d0 + 3, X.shape
    B3 = np.broadcast_to(B.reshape((-1, K, P)), (N, K, P)).astype(np.float64)
    want, mag = np.matmul(Inv.astype(np.float64), B3), np.matmul(np.abs(Inv).astype(np.float64), np.abs(B3))
    err = np.abs(X.reshape(N, K, P).astype(np.float64) - want)
    assert np.all(err <= 2 * K * 2.0 ** -24 * mag + 1e-30), float(np.max(err / (mag + 1e-30)))
    vm.eval("drop")
    assert np.array_equal(vm.fetch(None).reshape(A.shape), A)
    vm.eval("drop drop")
    assert depth(vm) == d0


@pytest.mark.parametrize("N,K,rhs", SOLVE)
def test_solve_on_a_batch(ovm, N, K, rhs):
    check_solve(ovm, N, K, rhs)


MATDIV = [(2, 4, ("t", 3)), (7, 5, ("m", 2)), (3, 16, ("t", 1)), (1, 3, ("m", 3))]                                     # N, K, left operand A [.., M, K]


def check_matdiv(vm, N, K, lhs):
    kinds, Bm = make_batch(300 + N * 37 + K, N, K)
    rng = np.random.default_rng(N * 13 + K)
    d0 = depth(vm)
    M = lhs[1]
    if lhs[0] == "t":
        A = rng.standard_normal((N, M, K)).astype(np.float32); ctor = "%d %d %d 1 tensor" % (N, M, K)
    else:
        A = rng.standard_normal((M, K)).astype(np.float32); ctor = "%d %d matrix" % (M, K)
    vm.store(A, ctor)
    push_batch(vm, Bm)
    Inv = vm.fetch("luinv").reshape(N, K, K); vm.eval("drop")
    C = vm.fetch("matdiv")                                                          # ( A B -- A B C )
    assert C.shape == (N, M, K, 1) and depth(vm) == d0 + 3, C.shape
    A3 = np.broadcast_to(A.reshape((-1, M, K)), (N, M, K)).astype(np.float64)
    want, mag = np.matmul(A3, Inv.astype(np.float64)), np.matmul(np.abs(A3), np.abs(Inv).astype(np.float64))
    err = np.abs(C.reshape(N, M, K).astype(np.float64) - want)
    assert np.all(err <= 2 * K * 2.0 ** -24 * mag + 1e-30), float(np.max(err / (mag + 1e-30)))
    vm.eval("drop")
    assert np.array_equal(vm.fetch(None).reshape(Bm.shape), Bm)                     # a batch B is factored on a copy and left intact
    vm.eval("drop drop")
    assert depth(vm) == d0


@pytest.mark.parametrize("N,K,lhs", MATDIV)
def test_matdiv_on_a_batch(ovm, N, K, lhs):
    check_matdiv(ovm, N, K, lhs)


def check_singular_entry(vm, K=5):
    """entry 1 of 3 has a zero last column: one line with its entry number, the other entries complete and right, det = 0"""
    rng = np.random.default_rng(7)
    A = np.stack([sk.matrix(rng, K, k) for k in ("dominant", "singular_last", "permuted")])
    d0 = depth(vm)
    push_batch(vm, A)
    for word, line in (("inverse", "tensor#inverse: singular matrix at column %d entry 1" % (K - 1)),
                       ("luinv", "tensor#plu: singular at column %d entry 1" % (K - 1))):
        out = vm.eval(word)
        assert out.count(line) == 1 and out.count(" entry ") == 1, out
        X = vm.fetch(None).reshape(3, K, K)
        for n in (0, 2):
            wt.inverse_check("%s beside a singular entry %d" % (word, n), A[n], X[n])
        vm.eval("drop")
    out = vm.eval("plu")
    assert out.count("tensor#plu: singular at column %d entry 1" % (K - 1)) == 1 and out.count(" entry ") == 1, out
    vm.eval("drop drop")
    An = A.copy(); An[0], An[2] = normalised(A[0]), normalised(A[2])
    push_batch(vm, An)
    out = vm.eval("det")
    assert out.count("tensor#plu: singular at column %d entry 1" % (K - 1)) == 1 and out.count(" entry ") == 1, out
    D = vm.fetch(None).ravel()
    assert D[1] == 0.0
    for n in (0, 2):
        s64, l64 = np.linalg.slogdet(An[n].astype(np.float64))
        assert np.sign(D[n]) == s64 and abs(np.log(abs(float(D[n]))) - l64) <= 1e-3 * max(1.0, abs(l64))
    vm.eval("drop drop drop")
    assert depth(vm) == d0


def test_a_singular_entry_prints_one_line_and_the_others_are_right(ovm):
    check_singular_entry(ovm)


REJECTED = [("2 3 4 1 tensor", w, "tensor2?") for w in ("inverse", "luinv", "plu", "upper", "lower", "det")] + \
           [("2 3 3 3 tensor", w, "tensor2?") for w in ("inverse", "det")] + \
           [("3 vector", w, "tensor2?") for w in ("inverse", "luinv", "plu", "det")] + \
           [("2 3 2 1 tensor 2 3 4 1 tensor", "solve", "batch dim?"),          # A not square
            ("2 3 2 3 tensor 2 3 3 1 tensor", "solve", "batch dim?"),          # C = 3 on the right-hand side
            ("2 3 2 1 tensor 2 3 3 3 tensor", "solve", "batch dim?"),          # C = 3 batch
            ("3 3 2 1 tensor 2 3 3 1 tensor", "solve", "batch dim?"),          # N mismatch
            ("2 4 2 1 tensor 2 3 3 1 tensor", "solve", "batch dim?"),          # K mismatch
            ("2 3 3 1 tensor 3 3 matrix", "solve", "batch dim?"),              # the matrix operand must be the batch
            ("2 2 3 1 tensor 2 3 4 1 tensor", "matdiv", "batch dim?"),
            ("3 2 3 1 tensor 2 3 3 1 tensor", "matdiv", "batch dim?"),
            ("2 2 3 3 tensor 2 3 3 1 tensor", "matdiv", "batch dim?"),
            ("3 vector 2 3 3 1 tensor", "matdiv", "batch dim?"),               # rank 1 on the left
            ("2 2 4 1 tensor 2 3 3 1 tensor", "matdiv", "batch dim?")]


def check_rejected(vm, ops, word, text):
    d0 = depth(vm)
    vm.eval(ops + " ones")
    d1 = depth(vm)
    out = vm.eval(word)
    assert text in out, (ops, word, out)
    assert depth(vm) == d1, (ops, word)
    vm.eval(" ".join(["drop"] * (d1 - d0)))


@pytest.mark.parametrize("ops,word,text", REJECTED)
def test_rejected_operands_keep_the_stack(ovm, ops, word, text):
    check_rejected(ovm, ops, word, text)


def test_rank2_script_prints_what_it_prints_today():
    if not os.path.exists(TEN4_ORACLE):
        pytest.skip("oracle/ten4_oracle not built")
    out = run_vm(TEN4_ORACLE, os.path.join(SCRIPTS, "kat_linalg.4th"))
    bad = compare(out, open(os.path.join(GOLDEN, "kat_linalg.out")).read())
    assert not bad, bad


# ---------------------------------------------------------------- rank <= 2 operands against the reference's own VM
M33 = "3 3 matrix{ 5 7 4 3 -1 3 6 7 5 }"
M22 = "2 2 matrix{ 4 7 2 6 }"
S22 = "2 2 matrix{ 1 2 2 4 }"
M23 = "2 3 matrix{ 1 2 3 4 5 6 }"
V3, V2 = "3 vector{ 1 1 1 }", "2 vector{ 1 2 }"
# Left out, because the host already differs from the reference there for reasons outside these words' rank-4 branches (code this work does
# not touch): a NON-SQUARE matrix through `luinv` / `upper` / `lower` (the reference prints "square matrix required", Tensor::lu_inverse /
# Tensor::lu of the host return silently), and a `solve` the reference rejects (its stack dump then shows an aliased object whose size is
# whatever memory holds).  Non-square `inverse`, `plu` and `det` print the same on both and stay in.
RANK2 = [op + " " + w + " . cr" for op in (M33, M22, S22, V3) for w in ("inverse", "luinv", "plu", "det")] + \
        [M23 + " " + w + " . cr" for w in ("inverse", "plu", "det")] + \
        [M33 + " plu upper . cr", M33 + " plu lower . cr", M22 + " plu upper . cr", M22 + " plu lower . cr", V3 + " upper . cr"] + \
        [a + " " + b + " solve . cr" for a, b in ((V3, M33), (V2, M22))] + \
        [a + " " + b + " matdiv . cr" for a, b in ((V3, M33), (V2, M22), (M22, M22), (M33, M33), (V2, M33), (M23, M33), (M33, M23), (V3, V3), (M22, S22))]


def test_rank2_operands_agree_with_the_reference_vm():
    if not os.path.exists(REFHOST):
        pytest.skip("oracle/_ref/ten4_refhost not built (build container only)")
    if not os.path.exists(TEN4_ORACLE):
        pytest.skip("oracle/ten4_oracle not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from regen_vm_goldens import normalise_refhost
    env = dict(os.environ, T4_SEED="1")
    for case in RANK2:                                                               # one VM per case: an error path may leave anything on the stack
        src = "0 trace\n" + case + "\n"
        ref = subprocess.run([REFHOST], input=src, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
        ora = subprocess.run([TEN4_ORACLE], input=src, capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
        assert ref.returncode == 0 and ora.returncode == 0, (case, ref.returncode, ora.returncode, ora.stdout[-500:])
        bad = compare(ora.stdout, normalise_refhost(ref.stdout), rtol=0, atol=0)
        assert not bad, (case, bad)
