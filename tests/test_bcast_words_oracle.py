"""`transpose` of a batch and NumPy broadcasting for `+ - * /` `+= -= *= /=` (DESIGN.md 3.9 "Beyond the reference: batched transpose and
broadcast arithmetic") on the CPU oracle VM - the product's host sources over the oracle's C-ABI, which has neither t4k_tt_op_bcast nor
t4k_transpose_batched, so Tensor::ten_bcast expands the broadcast operands and Tensor::transpose loops over the entries here.

Every row of the table: result shape and values bit for bit against NumPy float32 (single correctly rounded operations; operands from
+-[0.5, 2)), stack effects, the rejected pairs keeping their text and their stack, and a seeded sweep of rank <= 2 pairs against the
reference's own VM (oracle/_ref/ten4_refhost, build container only).  tests/test_gpu_bcast_words.py runs the same rows on the product VM."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from test_bmm_words_oracle import ctor, nhwc, numel
from vm_util import ROOT, TEN4_ORACLE, OracleVM, compare

REFHOST = os.path.join(ROOT, "oracle", "_ref", "ten4_refhost")
NP_OP = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide}

# ---------------------------------------------------------------- the table: operand descriptions as in tests/test_bmm_words_oracle.py
T = ("t", 2, 3, 4, 3)
ROWS = [
    (T, ("t", 2, 1, 1, 1)),                    # every entry by its own scalar
    (T, ("t", 1, 3, 1, 1)),                    # per row
    (T, ("t", 1, 1, 4, 1)),                    # a bias row
    (T, ("t", 1, 1, 1, 3)),                    # per channel
    (T, ("t", 2, 3, 4, 1)),                    # one channel for all
    (T, ("t", 1, 3, 4, 1)),
    (("t", 7, 3, 4, 1), ("t", 7, 3, 1, 1)),    # both N > 1
    (("t", 2, 1, 4, 1), ("t", 1, 3, 1, 3)),    # two-sided: (N,1,W,1) op (1,H,1,C)
    (T, ("m", 3, 4)), (T, ("m", 1, 4)), (T, ("m", 3, 1)), (T, ("m", 1, 1)),
    (("t", 1, 3, 4, 1), ("m", 1, 4)),          # N = 1 on both sides
    (T, ("v", 3)),                             # a vector is a column
    (T, ("v", 1)),
    (("m", 3, 4), ("m", 1, 4)), (("m", 3, 4), ("m", 3, 1)), (("m", 3, 1), ("m", 1, 4)), (("m", 3, 4), ("m", 1, 1)),
    (("m", 3, 4), ("v", 3)), (("m", 1, 4), ("v", 3)), (("m", 3, 4), ("v", 1)),
    (("v", 5), ("v", 1)),
    (("t", 128, 2, 2, 1), ("t", 128, 1, 1, 1)),
]
ROWS = ROWS + [(b, a) for a, b in ROWS]
# H*W*C equal and one N is 1: today's branch (one launch on the product VM now), result = the shape of the operand with N > 1
N_ROWS = [(("t", 3, 2, 5, 1), ("m", 2, 5)), (("m", 2, 5), ("t", 3, 2, 5, 1)), (("t", 2, 3, 2, 2), ("t", 1, 3, 2, 2)), (("t", 1, 3, 2, 2), ("t", 7, 3, 2, 2))]
IDS = lambda rows: ["%s_%s" % ("x".join(map(str, a[1:])) + a[0], "x".join(map(str, b[1:])) + b[0]) for a, b in rows]


def fits(a, b):
    """the new rule: H*W*C differ and every axis of (N,H,W,C) is equal or 1 on one side"""
    sa, sb = nhwc(a), nhwc(b)
    return int(np.prod(sa[1:])) != int(np.prod(sb[1:])) and all(x == y or x == 1 or y == 1 for x, y in zip(sa, sb))


def result_shape(a, b):
    return tuple(max(x, y) for x, y in zip(nhwc(a), nhwc(b)))


def result_text(a, b):
    """how `.` names the result: rank 4 if either operand is, a vector if both are, else a matrix"""
    n, h, w, c = result_shape(a, b)
    if "t" in (a[0], b[0]):
        return "tensor[%d,%d,%d,%d]" % (n, h, w, c)
    return "vector[%d]" % h if a[0] == b[0] == "v" else "matrix[%d,%d]" % (h, w)


def operand(rng, d):
    shape = nhwc(d)
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def depth(vm):
    return int(vm.eval("depth .").split()[0])


def run_row(vm, a, b, word):
    """( -- ) stores operands of a, b, runs `word`, returns (A, B, O) and leaves the stack as it found it"""
    rng = np.random.default_rng(zlib.crc32(repr((a, b, word)).encode()))
    A, B = operand(rng, a), operand(rng, b)
    d0 = depth(vm)
    vm.store(A, ctor(a)); vm.store(B, ctor(b))
    O = vm.fetch(word)
    keep = len(word) == 1
    assert depth(vm) == d0 + (3 if keep else 1), (a, b, word)
    if keep:                                                            # both operands are still there, untouched
        vm.eval("drop")
        assert np.array_equal(vm.fetch(None), B); vm.eval("drop")
        assert np.array_equal(vm.fetch(None), A)
    vm.eval("drop")
    assert depth(vm) == d0
    return A, B, O


def check_row(vm, a, b, word, exact_div=True):
    assert fits(a, b)
    A, B, O = run_row(vm, a, b, word)
    assert O.shape == result_shape(a, b), (O.shape, result_shape(a, b))
    op = word[0]
    want = NP_OP[op](A, B)
    if op != "/" or exact_div:
        assert np.array_equal(O, want), (a, b, word, int(np.sum(O != want)))
    return A, B, O


@pytest.fixture(scope="module")
def ovm():
    if not os.path.exists(os.path.join(ROOT, "oracle", "libten4_oracle.so")):
        pytest.skip("oracle/libten4_oracle.so not built")
    v = OracleVM(seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("word", ["+", "-", "*", "/"])
@pytest.mark.parametrize("a,b", ROWS, ids=IDS(ROWS))
def test_table_rows(ovm, a, b, word):
    check_row(ovm, a, b, word)                  # the oracle's division is the host's IEEE one: exact against NumPy too


@pytest.mark.parametrize("word", ["+=", "-=", "*=", "/="])
@pytest.mark.parametrize("a,b", ROWS[::5], ids=IDS(ROWS[::5]))
def test_assigning_words_drop_both_operands(ovm, a, b, word):
    check_row(ovm, a, b, word)


def check_n_row(vm, a, b, word):
    A, B, O = run_row(vm, a, b, word)
    assert O.shape == (nhwc(a) if nhwc(a)[0] > 1 else nhwc(b))
    if word[0] != "/":
        assert np.array_equal(O, NP_OP[word[0]](A, B))
    return A, B, O


@pytest.mark.parametrize("word", ["+", "-", "*", "/", "*="])
@pytest.mark.parametrize("a,b", N_ROWS, ids=IDS(N_ROWS))
def test_equal_hwc_n_broadcast_keeps_its_result(ovm, a, b, word):
    A, B, O = check_n_row(ovm, a, b, word)
    assert np.array_equal(O, NP_OP[word[0]](A, B))


def check_result_names(vm):
    for a, b in ROWS:
        out = vm.eval("%s ones %s ones + . cr" % (ctor(a), ctor(b)))
        assert result_text(a, b) in out, (a, b, out)
        vm.eval("drop drop")


def test_result_rank(ovm):
    check_result_names(ovm)


TRANSPOSE = [(1, 3, 4, 1), (2, 3, 3, 1), (2, 3, 5, 1), (7, 5, 2, 3), (3, 1, 6, 2), (2, 66, 65, 1)]


def check_transpose(vm, N, H, W, C):
    a = np.arange(N * H * W * C, dtype=np.float32).reshape(N, H, W, C)
    d0 = depth(vm)
    vm.store(a, "%d %d %d %d tensor" % (N, H, W, C))
    t = vm.fetch("transpose")                                           # ( A -- A A' )
    assert t.shape == (N, W, H, C) and depth(vm) == d0 + 2
    assert np.array_equal(t, a.transpose(0, 2, 1, 3))
    back = vm.fetch("transpose")
    assert back.shape == a.shape and np.array_equal(back, a)            # twice gives back the operand
    vm.eval("drop drop")
    assert np.array_equal(vm.fetch(None), a)
    vm.eval("drop")
    assert depth(vm) == d0


@pytest.mark.parametrize("N,H,W,C", TRANSPOSE)
def test_transpose_of_a_batch(ovm, N, H, W, C):
    check_transpose(ovm, N, H, W, C)


def test_transpose_rank2_and_rank1_as_before(ovm):
    a = np.arange(6, dtype=np.float32)
    ovm.store(a, "2 3 matrix")
    t = ovm.fetch("transpose")
    assert t.shape == (1, 3, 2, 1) and np.array_equal(t.reshape(3, 2), a.reshape(2, 3).T)
    ovm.eval("drop drop")
    d0 = depth(ovm)
    out = ovm.eval("3 vector transpose")
    assert "tensor2?" in out and depth(ovm) == d0 + 1
    ovm.eval("drop")


# ---------------------------------------------------------------- what stays rejected
REJECTED = [("2 3 matrix", "3 3 matrix", "} dim?", 0),                  # tests/golden/vm/error_paths.out
            ("5 vector", "4 vector", "} dim?", 0),                      # ditto
            ("2 3 4 1 tensor", "1 2 4 1 tensor", "} dim?", 0),          # an axis with 2 against 3
            ("2 3 4 3 tensor", "1 3 4 2 tensor", "} dim?", 0),
            ("2 3 4 1 tensor", "4 vector", "} dim?", 0),                # a vector is a column: 4 against H = 3
            ("2 2 3 1 tensor", "3 2 2 1 tensor", "tensor#ten_op A.HWC(6)!=B.HWC(4) or N, C diff", 1),   # both N > 1: the line, and a copy of A pushed
            ("2 2 3 1 tensor", "2 4 2 1 tensor", "tensor#ten_op A.HWC(6)!=B.HWC(8) or N, C diff", 1)]


def check_rejected(vm, a, b, text, pushed):
    for word in ("+", "/", "*="):
        d0 = depth(vm)
        vm.eval(a + " ones " + b + " ones")
        out = vm.eval(word)
        assert text in out, (a, b, word, out)
        keep = len(word) == 1
        want = d0 + 2 + pushed if (keep or not pushed) else d0 + 1      # the ten_op path of an assigning word drops both operands and pushes the copy
        assert depth(vm) == want, (a, b, word, depth(vm), want)
        vm.eval(" ".join(["drop"] * (depth(vm) - d0)))


@pytest.mark.parametrize("a,b,text,pushed", REJECTED)
def test_rejected_pairs_keep_text_and_stack(ovm, a, b, text, pushed):
    check_rejected(ovm, a, b, text, pushed)


def test_error_paths_golden_lines():
    if not os.path.exists(TEN4_ORACLE):
        pytest.skip("oracle/ten4_oracle not built")
    src = "2 3 matrix ones 1 3 matrix ones + . cr\n2 3 matrix 3 3 matrix + depth . cr\n5 vector 4 vector + depth . cr\n"
    out = subprocess.run([TEN4_ORACLE], input=src, capture_output=True, text=True, timeout=120, env=dict(os.environ, T4_SEED="1"), cwd=ROOT).stdout
    assert "matrix[2,3]" in out and "+2.0000 +2.0000 +2.0000" in out     # `} dim?` on the parent commit
    assert out.count("} dim?") == 2


# ---------------------------------------------------------------- regression sweep of rank <= 2 pairs against the reference's own VM
def ref_accepts(a, b):
    """xop2's tensor-tensor branch as it was (tenvm.cpp:96-113): N is 1 for rank <= 2, so H*W*C must be equal"""
    return numel(a) == numel(b)


def random_operand(rng):
    if rng.integers(2):
        return ("v", int(rng.integers(1, 5)))
    return ("m", int(rng.integers(1, 5)), int(rng.integers(1, 5)))


def sweep_pairs(n=150):
    rng = np.random.default_rng(20261017)
    out = []
    while len(out) < n:
        a, b = random_operand(rng), random_operand(rng)
        if rng.random() < 0.5 and b[0] == "m":                          # bias towards pairs one of the rules answers
            b = ("m", nhwc(a)[1], b[2]) if rng.integers(2) else ("m", b[1], nhwc(a)[2])
        out.append((a, b))
    return out


def sweep_line(a, b, op):
    return "%s gradfill %s gradfill %s . cr" % (ctor(a), ctor(b), op)


def test_sweep_pairs_are_meaningful():
    pairs = sweep_pairs()
    assert sum(ref_accepts(a, b) for a, b in pairs) >= 20
    assert sum(fits(a, b) for a, b in pairs) >= 20
    assert sum(not ref_accepts(a, b) and not fits(a, b) for a, b in pairs) >= 20


def test_sweep_matches_reference_vm(ovm):
    if not os.path.exists(REFHOST):
        pytest.skip("oracle/_ref/ten4_refhost not built (build container only)")
    if not os.path.exists(TEN4_ORACLE):
        pytest.skip("oracle/ten4_oracle not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from regen_vm_goldens import normalise_refhost
    env = dict(os.environ, T4_SEED="1")
    pairs = sweep_pairs()
    ops = "+-*"                                                         # gradfill starts at 0: no quotients here
    same = [(a, b, ops[i % 3]) for i, (a, b) in enumerate(pairs) if not fits(a, b)]      # the reference answers, or both reject
    src = "0 trace\n" + "\n".join(sweep_line(a, b, op) + "\n" + " ".join(["drop"] * (2 if ref_accepts(a, b) else 1)) for a, b, op in same) + "\n"
    ref = subprocess.run([REFHOST], input=src, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    ora = subprocess.run([TEN4_ORACLE], input=src, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert ref.returncode == 0 and ora.returncode == 0, (ref.returncode, ref.stdout[-1000:], ora.stdout[-1000:])
    assert ora.stdout.count("} dim?") >= 20
    bad = compare(ora.stdout, normalise_refhost(ref.stdout), rtol=0, atol=0)
    assert not bad, bad
    for i, (a, b) in enumerate(pairs):                                  # accepted only by the new rule: NumPy is the meaning
        if fits(a, b):
            check_row(ovm, a, b, ops[i % 3])
