"""CPU half of the GEMM sweep (tests/test_gpu_gemm_sweep.py): the case table against the Python mirror of gemm_launch at 256 CUs, the
sweep's own assertions (gemm_cases.hold, check_moat) run on two honest fp32 implementations - the oracle, and a second summation order (K in
the slabs of the row's kchunk, each slab in blocks of 32 summed pairwise, the slabs folded in order) - which must pass both the exact and the
float bar on every row, and on injected defects, each of which must fail the row its test names.  No GPU needed."""
import numpy as np
import pytest

import f64_witness as wt
import gemm_cases as gc

CPU_FLOPS = 1e9                                            # rows above this run at a reduced K with the same residue mod 64


# ----------------------------------------------------------------------------- the table and the mirror
def test_every_row_is_on_its_label_at_256_cus():
    ids = [r.id for r in gc.ROWS]
    assert len(set(ids)) == len(ids)
    for r in gc.ROWS:
        lab, n = r.plan(256)
        assert lab == r.label, "%s: the mirror says %s (%d launches)" % (r.id, lab, n)
        assert r.why and n == (2 if lab.endswith("+fold") else 1) and gc.exact_ok(r)
        assert r.K <= 4096 and r.skew in (0, 1)


def test_every_label_of_the_mirror_has_a_row():
    labels = {r.label for r in gc.ROWS}
    bases = {gc.ladder(r.M, r.N, r.K, r.tA, r.tB, r.C, aligned=not r.skew)["base"] for r in gc.ROWS}
    assert bases == set(gc.ALL_BASES), set(gc.ALL_BASES) ^ bases
    for want in gc.REQUIRED:
        assert want in labels, "no row reaches %s" % want
    # every base form under a fold that the ladder can split: the three slab kernels of the issue and the 64-deep LDS-DMA one
    assert {r.label.split("x")[0] for r in gc.ROWS if r.label.endswith("+fold")} == {"glds8<128>", "glds8<64>", "mfma<64,64,64,vec,skew>", "mfma<64,64,32>"}
    nsplits = sorted(gc.ladder(r.M, r.N, r.K, r.tA, r.tB)["nsplit"] for r in gc.ROWS if r.label.endswith("+fold"))
    assert nsplits[0] == 2 and nsplits[-1] == 64 and len(set(nsplits)) >= 5
    # every layout on the sliver, pair, lean and 256-tile forms
    for fam in ("l32", "plain256"):
        assert {(r.tA, r.tB) for r in gc.ROWS if r.label.startswith(fam)} == {(0, 0), (0, 1), (1, 0), (1, 1)}, fam
    assert all(isinstance(v, str) and v for v in gc.UNREACHABLE.values())
    # a random walk over shapes finds no base the table does not name
    rng = np.random.default_rng(5)
    for _ in range(20000):
        M, N = (int(rng.choice([1, 2, 3, 4, 33, 64, 100, 128, 256, 500, 512, 768, 1024, 1536, 2048, 2050, 4096])) for _ in range(2))
        K = int(rng.choice([1, 4, 8, 12, 64, 100, 128, 132, 256, 300, 512, 784, 832, 836, 1024, 2048, 2112, 4096]))
        C = int(rng.choice([1, 1, 1, 2]))
        b = gc.ladder(M, N, K, int(rng.integers(2)), int(rng.integers(2)), C, aligned=bool(rng.integers(4)), alpha=float(rng.choice([1.0, 2.0])), lane=int(rng.integers(2)),
                      capturing=bool(rng.integers(2)))["base"]
        assert b in gc.ALL_BASES, (M, N, K, C, b)


def test_the_mirror_at_the_edges_the_table_is_sized_from():
    P = lambda *a, **k: gc.gemm_kernel_plan(*a, **k)[0]
    assert P(64, 64, 832, 0, 1) == "l32/w8/rst" and P(64, 64, 836, 0, 1).endswith("+fold")                    # kc = 832 | 840
    assert P(64, 64, 830, 0, 1) == "mfma<64,64,32>x7+fold"                                                   # K % 4 != 0 on K-contiguous operands
    assert P(1024, 512, 512, 0, 0).startswith("l32") and P(1024, 576, 512, 0, 0) == "nn_plain"               # 128 | 144 64-tiles
    assert P(576, 576, 256, 0, 0) == "l32/w4" and P(576, 576, 288, 0, 0) == "l32/w4/rst"                     # nblk = 8 | 9 on 4 waves
    assert P(512, 512, 256, 0, 0) == "l32/w8" and P(512, 544, 256, 0, 0) == "l32/w4"                         # t32 = 256 | 272
    assert P(64, 64, 160, 0, 0) == "l32/w4" and P(64, 64, 168, 0, 0) == "l32/w8"                             # nblk = 5 | 6
    assert P(64, 64, 512, 0, 0) == "l32/w8" and P(64, 64, 516, 0, 0) == "l32/w8/rst"                         # nblk = 16 | 17
    assert P(576, 640, 1024, 0, 0) == "pair" and P(576, 576, 1024, 0, 0) != "pair"                           # 90 | 81 tiles: 81 x 3 = 243 <= 256
    assert P(576, 640, 1024, 0, 0, lane=1) == "mfma<64,64,64,vec,skew>x3+fold"                               # tickets are the default stream's
    assert P(576, 640, 1280, 0, 0) == "pair" and P(576, 640, 1088, 0, 0) != "pair"                           # K % 256
    assert P(1536, 2048, 128, 0, 0) == "nn_plain" and P(1536, 1920, 128, 0, 0) == "nn_plain"                 # t128 = 192 (big) | 180: the same kernel from either branch
    assert P(1536, 2040, 64, 0, 0) == "mfma<128,128,32,vec,full>" and P(1536, 1912, 64, 0, 0) == "glds8<64>" # ... ragged: 128-tiles | 64-tiles
    assert P(2048, 2048, 256, 0, 0) == "plain128" and P(2048, 2048, 192, 0, 0) == "plain_ragk" and P(2048, 1920, 256, 0, 0) == "nn_plain"   # K >= 256, t128i >= 256
    assert P(2048, 4096, 288, 0, 0) == "plain128/bk32" and P(2048, 3968, 288, 0, 0) == "plain128/ragk"       # 512 | 496 tiles
    assert P(4096, 4096, 256, 0, 0) == "plain256" and P(4096, 3840, 256, 0, 0) != "plain256"                 # t256 = 256 | 240
    assert P(4096, 4096, 128, 0, 0) == "nn_plain" and P(4096, 4096, 160, 0, 0) == "plain_ragk"               # K < 256 never reaches launch_plain128
    assert P(1540, 2048, 2048, 0, 0) == "glds8<128>" and P(1540, 2048, 1984, 0, 0) == "mfma<128,128,32,vec,full>"   # big_dma from K = 2048
    assert P(768, 704, 8, 0, 0) == "glds8<64,ragk>" and P(768, 704, 4, 0, 0) == "mfma<64,64,64,vec,skew>"
    assert P(768, 704, 128, 0, 0) == "nn_plain" and P(768, 704, 128, 0, 0, alpha=2, beta=-1) == "plain_any"
    assert P(33, 68, 100, 0, 1, capturing=True) == "glds8<64,ragk>" and P(64, 96, 516, 1, 1, capturing=True) == "mfma<64,64,64,vec,skew>x5+fold"
    assert P(5, 7, 0, 0, 0) == "k0" and gc.gemm_kernel_plan(0, 7, 3, 0, 0) == ("none", 0)
    for M, N, K, tA, tB, named, taken in gc.DRIFTED:                                                          # the drifted cases of test_gpu_parity.py
        assert P(M, N, K, tA, tB) == taken != named


# ----------------------------------------------------------------------------- two honest fp32 implementations
def cpu_k(r):
    if r.flops() <= CPU_FLOPS:
        return r.K
    per = 2.0 * r.M * r.N * r.C
    k = r.K % 64 or 64
    while per * (k + 64) <= CPU_FLOPS and k + 64 <= r.K:
        k += 64
    return k


def mats(r, A, B):
    """A [C, M, K], B [C, K, N] views of the stored operands"""
    a = np.moveaxis(A, -1, 0) if r.C > 1 else A[None]; b = np.moveaxis(B, -1, 0) if r.C > 1 else B[None]
    return (a.transpose(0, 2, 1) if r.tA else a), (b.transpose(0, 2, 1) if r.tB else b)


def blocked(a, b, kchunk):
    """fp32: K in slabs of kchunk, a slab in blocks of 32 summed pairwise, the slabs added in order"""
    tot = None
    for k0 in range(0, a.shape[-1], kchunk):
        parts = [a[..., k:k + 32] @ b[:, k:k + 32] for k in range(k0, min(k0 + kchunk, a.shape[-1]), 32)]
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        tot = parts[0] if tot is None else tot + parts[0]
    return tot.astype(np.float32)


def honest(oracle, order, r, A, B, O0, alpha, beta, K):
    a, b = mats(r, A, B)
    if order == "oracle" and 2.0 * r.M * r.N * K * r.C <= 2e8:
        return oracle.gemm(A, B, O0.copy(), alpha, beta, r.tA, r.tB, r.C)
    if order == "oracle":
        ab = np.ascontiguousarray(a) @ np.ascontiguousarray(b)        # fp32 BLAS: an honest order of its own where the oracle's loop is too slow
    else:
        kchunk = gc.ladder(r.M, r.N, r.K, r.tA, r.tB, r.C, aligned=not r.skew)["kchunk"] or 64
        ab = blocked(np.ascontiguousarray(a), np.ascontiguousarray(b), kchunk)
    ab = np.moveaxis(ab, 0, -1) if r.C > 1 else ab[0]
    o = np.float32(alpha) * ab
    if beta != 0:
        o = o + np.float32(beta) * O0
    return o.astype(np.float32)


_LAST = {}


@pytest.mark.parametrize("order", ["oracle", "blocked"])
@pytest.mark.parametrize("row", gc.ROWS, ids=[r.id for r in gc.ROWS])
def test_honest_orders_pass_both_bars_on_every_row(oracle, row, order):
    r, K = row, cpu_k(row)
    assert K % 64 == r.K % 64 and K <= r.K
    q = gc.Row(r.label, r.M, r.N, K, r.tA, r.tB, r.why, r.C, r.skew)
    if _LAST.get("id") != r.id:                              # the two orders of a row share its operands and float64 products
        _LAST.clear(); _LAST["id"] = r.id
        for exact in (True, False):
            A, B, O0 = gc.operands(r, exact, K)
            _LAST[exact] = (A, B, O0, gc.Product(q, A, B))
    for exact in (True, False):
        A, B, O0, prod = _LAST[exact]
        for alpha, beta in (((1.0, 0.0), (2.0, -1.0)) if exact else ((0.5, 2.0),)):
            gc.hold("%s %s (%g, %g)" % (r.id, order, alpha, beta), honest(oracle, order, q, A, B, O0, alpha, beta, K), prod, alpha, beta, O0, exact, "cpu " + order)


# ----------------------------------------------------------------------------- injected defects
def _must_fail(text, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    assert text in str(e.value), str(e.value)[:300]


def _setup(oracle, label, exact, alpha=1.0, beta=0.0):
    r = gc.first(label)
    A, B, O0 = gc.operands(r, exact)
    prod = gc.Product(r, A, B)
    got = honest(oracle, "oracle", r, A, B, O0, alpha, beta, r.K)
    gc.hold("honest", got, prod, alpha, beta, O0, exact, "cpu defects")
    a, b = mats(r, A.astype(np.float64), B.astype(np.float64))
    return r, a[0], b[0], O0, prod, got


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
def test_injected_defects_fail_their_rows(oracle, exact):
    """each defect is applied to the oracle's (passing) result of the named row and must fail the sweep's own assertion there:
      a K tail dropped                         l32/w4            33 x 68 x 100: the 4 behind three blocks
      a slab left out of the fold              glds8<128>x4+fold 512 x 512 x 1024: the last of four slabs of 256
      a k-group added twice                    l32/w8            70 x 68 x 208: block 1 of 7
      a clamped edge row stored                glds8<128>        770 x 704 x 128: row 770 = a copy of row 769, behind the tensor
      beta applied to the product, not to O    plain_any         768 x 704 x 128 at (2, -1) | (0.5, 2)
      O read at beta = 0                       nn_plain          768 x 704 x 128 over an O prefilled with NaN"""
    ab = (2.0, -1.0) if exact else (0.5, 2.0)
    r, a, b, O0, prod, got = _setup(oracle, "l32/w4", exact)
    bad = (got - a[:, 96:] @ b[96:]).astype(np.float32)
    _must_fail(r.id, lambda: gc.hold(r.id + " tail dropped", bad, prod, 1.0, 0.0, O0, exact, "cpu defects"))

    r, a, b, O0, prod, got = _setup(oracle, "glds8<128>x4+fold", exact)
    bad = (got - a[:, 768:] @ b[768:]).astype(np.float32)
    _must_fail(r.id, lambda: gc.hold(r.id + " slab left out", bad, prod, 1.0, 0.0, O0, exact, "cpu defects"))

    r, a, b, O0, prod, got = _setup(oracle, "l32/w8", exact)
    bad = (got + a[:, 32:64] @ b[32:64]).astype(np.float32)
    _must_fail(r.id, lambda: gc.hold(r.id + " k-group twice", bad, prod, 1.0, 0.0, O0, exact, "cpu defects"))

    r, a, b, O0, prod, got = _setup(oracle, "glds8<128>", exact)
    for skew in (0, 1, 2):
        img, k = gc.moated(got, skew)
        assert img.size == got.size + 2 * gc.MOAT + skew and np.array_equal(gc.check_moat("t", img.copy(), k, got.size).reshape(got.shape), got)
        after = img.copy(); m = min(r.N, gc.MOAT); after[k + got.size:k + got.size + m] = got[-1][:m]
        _must_fail("behind the tensor", lambda: gc.check_moat("clamped row stored", after, k, got.size))
        after = img.copy(); after[k - 1] = 0.0
        _must_fail("in front of the tensor", lambda: gc.check_moat("store in front", after, k, got.size))
        after = img.copy(); after[-1] = 1.0
        _must_fail("behind the tensor", lambda: gc.check_moat("the last float of the moat", after, k, got.size))

    r, a, b, O0, prod, got = _setup(oracle, "plain_any", exact, *ab)
    bad = (ab[1] * (ab[0] * (a @ b)) + O0).astype(np.float32)
    _must_fail(r.id, lambda: gc.hold(r.id + " beta on the product", bad, prod, ab[0], ab[1], O0, exact, "cpu defects"))

    r, a, b, O0, prod, got = _setup(oracle, "nn_plain", exact)
    bad = (got + np.float32(0.0) * np.full(got.shape, np.nan, np.float32)).astype(np.float32)
    _must_fail("NaN in O", lambda: gc.hold(r.id + " O read at beta = 0", bad, prod, 1.0, 0.0, O0, exact, "cpu defects"))
