"""`@` / `matmul` / `@=` beyond the reference's _tdot: batched rank-4 products, N and C broadcast from either side, vector @ matrix
and vector @ rank-4 (DESIGN.md "Beyond the reference"), on the CPU oracle VM - the product's host sources over the oracle's C-ABI,
which has no t4k_gemm_batched, so Tensor::bmm takes its per-matrix t4k_gemm loop here.

Values are checked against float64 NumPy within the fp32 dot-product bound |O - O64| <= 2 K 2^-24 (|A| @ |B|).  A sweep of random
shape pairs then pins that the pairs the reference answers still print what the reference prints, and the pairs both the reference
and the new rules reject print the same error (oracle/_ref/ten4_refhost, build container only)."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from vm_util import ROOT, TEN4_ORACLE, OracleVM, compare

REFHOST = os.path.join(ROOT, "oracle", "_ref", "ten4_refhost")


# ---------------------------------------------------------------- operand descriptions: ("v", K) | ("m", H, W) | ("t", N, H, W, C)
def ctor(d):
    if d[0] == "v":
        return "%d vector" % d[1]
    if d[0] == "m":
        return "%d %d matrix" % d[1:]
    return "%d %d %d %d tensor" % d[1:]


def nhwc(d):
    """(N, H, W, C) as the host's Tensor sees it (a vector [K] is H = K, W = 1)."""
    if d[0] == "v":
        return (1, d[1], 1, 1)
    if d[0] == "m":
        return (1, d[1], d[2], 1)
    return d[1:]


def numel(d):
    return int(np.prod(nhwc(d)))


def ref_accepts(a, b):
    """The reference's _tdot (tenvm.cpp:328-366) as the host restates it: the branches that existed before."""
    (Na, Ha, Wa, Ca), (Nb, Hb, Wb, Cb) = nhwc(a), nhwc(b)
    if a[0] == "v" and b[0] == "v" and numel(a) == numel(b):
        return True
    if b[0] == "v" and Wa == numel(b):
        return True
    if a[0] == "m" and b[0] == "m" and Wa == Hb:
        return True
    return (Na == 1 or Nb == 1) and Na != Nb and Ca == Cb and Wa == Hb


def new_result(a, b):
    """Shape (N, H, W, C) the new branches give, or None when they reject the pair too."""
    (Na, Ha, Wa, Ca), (Nb, Hb, Wb, Cb) = nhwc(a), nhwc(b)
    if a[0] != "v" and b[0] != "v" and "t" in (a[0], b[0]) and Wa == Hb and \
            (Na == Nb or 1 in (Na, Nb)) and (Ca == Cb or 1 in (Ca, Cb)):
        return (max(Na, Nb), Ha, Wb, max(Ca, Cb))
    if a[0] == "v" and b[0] == "m" and a[1] == Hb:
        return (1, Wb, 1, 1)                   # vector [P]
    if a[0] == "v" and b[0] == "t" and a[1] == Hb:
        return (Nb, 1, Wb, Cb)
    return None


def want64(a, b, A, B):
    """float64 product and the |A| @ |B| magnitude of the bound, both as (N, H, P, C)."""
    A4 = A.reshape(nhwc(a)).astype(np.float64)
    B4 = B.reshape(nhwc(b)).astype(np.float64)
    if a[0] == "v":
        A4 = A4.transpose(0, 2, 1, 3)          # [K] -> a [1, K] row
    At, Bt = A4.transpose(0, 3, 1, 2), B4.transpose(0, 3, 1, 2)           # (N, C, H, K) @ (N, C, K, P)
    o, m = np.matmul(At, Bt), np.matmul(np.abs(At), np.abs(Bt))
    return o.transpose(0, 2, 3, 1), m.transpose(0, 2, 3, 1)


@pytest.fixture(scope="module")
def ovm():
    if not os.path.exists(os.path.join(ROOT, "oracle", "libten4_oracle.so")):
        pytest.skip("oracle/libten4_oracle.so not built")
    v = OracleVM(seed=1)
    yield v
    v.close()


def run_pair(vm, a, b, rng, word="@"):
    A = rng.standard_normal(numel(a)).astype(np.float32)
    B = rng.standard_normal(numel(b)).astype(np.float32)
    vm.store(A, ctor(a))
    vm.store(B, ctor(b))
    O = vm.fetch(word)
    return A, B, O


CASES = []
for N, Nb in [(1, 1), (2, 2), (7, 7), (1, 2), (7, 1), (1, 7)]:
    for C in (1, 3):
        CASES.append((("t", N, 5, 9, C), ("t", Nb, 9, 6, C)))
for C, Cb in [(1, 3), (3, 1)]:
    CASES.append((("t", 2, 7, 4, C), ("t", 2, 4, 3, Cb)))
    CASES.append((("t", 7, 3, 5, C), ("t", 1, 5, 8, Cb)))
CASES += [
    (("m", 20, 9), ("t", 2, 9, 12, 1)),        # rank 2 @ rank 4 (ragged 20 x 12 x 9)
    (("m", 6, 4), ("t", 7, 4, 5, 3)),          # rank 2 broadcast over N and C
    (("t", 2, 6, 4, 3), ("m", 4, 5)),
    (("t", 7, 33, 17, 1), ("m", 17, 40)),
    (("t", 1, 4, 4, 1), ("t", 1, 4, 4, 1)),    # N = 1 both
    (("t", 1, 3, 5, 1), ("m", 5, 2)),
    (("t", 2, 70, 66, 1), ("t", 2, 66, 65, 1)),   # above the small-matrix regime
    (("v", 9), ("m", 9, 5)),
    (("v", 1), ("m", 1, 7)),
    (("v", 33), ("m", 33, 20)),
    (("v", 6), ("t", 1, 6, 4, 1)),
    (("v", 6), ("t", 2, 6, 4, 3)),
    (("v", 5), ("t", 7, 5, 9, 1)),
]


@pytest.mark.parametrize("a,b", CASES, ids=["%s@%s" % ("x".join(map(str, a[1:])) + a[0], "x".join(map(str, b[1:])) + b[0]) for a, b in CASES])
def test_new_pairs_shape_and_values(ovm, a, b):
    shape = new_result(a, b)                    # N broadcast with equal C keeps the existing per-sample branch: same meaning
    assert shape is not None
    rng = np.random.default_rng(zlib.crc32(repr((a, b)).encode()))
    A, B, O = run_pair(ovm, a, b, rng)
    ovm.eval("drop drop drop")
    if a[0] == "v" and b[0] == "m":
        assert O.shape == (1, shape[1], 1, 1), O.shape     # a vector [P]
    else:
        assert O.shape == shape, (O.shape, shape)
    o64, mag = want64(a, b, A, B)
    K = nhwc(b)[1]
    got = O.reshape(o64.shape).astype(np.float64)
    err = np.abs(got - o64)
    assert np.all(err <= 2 * K * 2.0 ** -24 * mag + 1e-30), float(np.max(err / (mag + 1e-30)))


def test_at_equals_drops_operands(ovm):
    rng = np.random.default_rng(3)
    a, b = ("t", 2, 3, 4, 1), ("t", 2, 4, 5, 1)
    d0 = ovm.eval("depth .").split()[0]
    ovm.store(rng.standard_normal(numel(a)), ctor(a))
    ovm.store(rng.standard_normal(numel(b)), ctor(b))
    O = ovm.fetch("@=")
    assert O.shape == (2, 3, 5, 1)
    assert ovm.eval("drop depth .").split()[0] == d0      # @= leaves only the product


def test_matmul_keeps_operands(ovm):
    a, b = ("t", 2, 3, 4, 3), ("m", 4, 5)
    d0 = ovm.eval("depth .").split()[0]
    ovm.eval(ctor(a) + " " + ctor(b))
    O = ovm.fetch("matmul")
    assert O.shape == (2, 3, 5, 3)
    assert ovm.eval("drop drop drop depth .").split()[0] == d0   # matmul keeps both operands under the product


@pytest.mark.parametrize("a,b", [(("t", 2, 3, 4, 1), ("t", 3, 4, 5, 1)),     # Na = 2 against Nb = 3
                                 (("t", 2, 3, 4, 1), ("t", 2, 5, 5, 1)),     # K mismatch
                                 (("t", 2, 3, 4, 2), ("t", 2, 4, 5, 3)),     # Ca = 2 against Cb = 3
                                 (("v", 4), ("m", 5, 2)),
                                 (("v", 4), ("t", 2, 3, 2, 1))])
def test_rejected_pairs_keep_the_error(ovm, a, b):
    out = ovm.eval(ctor(a) + " " + ctor(b) + " @ depth .")
    assert "A.W != B.H dim?" in out, out
    ovm.eval("drop drop")


# ---------------------------------------------------------------- regression sweep against the reference's own VM
def random_operand(rng):
    k = rng.integers(3)
    if k == 0:
        return ("v", int(rng.integers(1, 5)))
    if k == 1:
        return ("m", int(rng.integers(1, 5)), int(rng.integers(1, 5)))
    return ("t", int(rng.integers(1, 4)), int(rng.integers(1, 5)), int(rng.integers(1, 5)), int(rng.integers(1, 4)))


def sweep_pairs(n=200):
    rng = np.random.default_rng(20261016)
    out = []
    while len(out) < n:
        a, b = random_operand(rng), random_operand(rng)
        if rng.random() < 0.6:                  # bias towards matching inner dimensions
            Wa = nhwc(a)[2] if a[0] != "v" else None
            if b[0] == "m" and Wa:
                b = ("m", Wa, b[2])
            elif b[0] == "t" and Wa:
                b = ("t", b[1], Wa, b[3], b[4])
            elif a[0] == "v" and b[0] == "m":
                b = ("m", a[1], b[2])
            elif a[0] == "v" and b[0] == "t":
                b = ("t", b[1], a[1], b[3], b[4])
        if b[0] == "v" and nhwc(a)[0] > 1 and nhwc(a)[2] == b[1]:
            continue                            # rank 4 (N > 1) @ vector: Tensor::mm refuses (N, C diff) and prints an unwritten tensor - arena contents
        if ref_accepts(a, b) or new_result(a, b) is None:   # pairs only the new rules answer have no reference text
            out.append((a, b))
    return out


def sweep_script(pairs):
    lines = []
    for a, b in pairs:
        keep = 2 if ref_accepts(a, b) else 1    # `.` took the product (or, after the error, B)
        lines.append("%s gradfill %s gradfill @ . cr\n%s" % (ctor(a), ctor(b), " ".join(["drop"] * keep)))   # `.` of a tensor prints at the end of the line
    return "\n".join(lines) + "\n"


def test_sweep_pairs_are_meaningful():
    pairs = sweep_pairs()
    assert sum(ref_accepts(a, b) for a, b in pairs) >= 40
    assert sum(not ref_accepts(a, b) for a, b in pairs) >= 40


def test_sweep_matches_reference_vm():
    if not os.path.exists(REFHOST):
        pytest.skip("oracle/_ref/ten4_refhost not built (build container only)")
    if not os.path.exists(TEN4_ORACLE):
        pytest.skip("oracle/ten4_oracle not built")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from regen_vm_goldens import normalise_refhost
    src = "0 trace\n" + sweep_script(sweep_pairs())     # the reference starts at T4_VERBOSE = 1 (ten4.cu:155)
    env = dict(os.environ, T4_SEED="1")
    ref = subprocess.run([REFHOST], input=src, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    ora = subprocess.run([TEN4_ORACLE], input=src, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert ref.returncode == 0 and ora.returncode == 0, (ref.returncode, ref.stdout[-1000:], ora.stdout[-1000:])
    assert ora.stdout.count("A.W != B.H dim?") >= 40
    bad = compare(ora.stdout, normalise_refhost(ref.stdout), rtol=0, atol=0)
    assert not bad, bad
