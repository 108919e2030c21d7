"""CPU half of the linear-layer sweep (tests/test_gpu_linear_sweep.py): the case table against the Python mirror of the dispatch at 256 CUs,
the sweep's own assertions (linear_cases.check_fwd / check_bwd, the guard words) run on two honest fp32 implementations - the oracle, and a
second summation order (K in blocks of 32, the blocks' partial products summed pairwise) - which must pass both the exact and the float bar
on every shape of the table, and on injected defects, each of which must fail the case its test names.  No GPU needed."""
import numpy as np
import pytest

import f64_witness as wt
import linear_cases as lc

SEED, OFFSET = 91, 1 << 18


# ----------------------------------------------------------------------------- the table and the mirror
def test_every_row_is_on_its_label_at_256_cus():
    ids = [c.id for c in lc.ALL_CASES]
    assert len(set(ids)) == len(ids)
    for c in lc.ALL_CASES:
        lab, n = c.plan(256)
        assert lab == c.label, "%s: the mirror says %s (%d launches)" % (c.id, lab, n)
        assert c.why and n >= (0 if "refused" in lab and c.entry.startswith("mlp_") else 1)


def test_every_label_of_the_issue_has_a_row():
    labels = [c.label for c in lc.ALL_CASES]
    for want in lc.REQUIRED_LABELS:
        assert any(want in lab for lab in labels), "no row reaches %s" % want
    # forms inside k_linsmall_bwd: CBK = 1 and > 1, one trip and several, in place behind the counter and apart
    forms = {lc.small_bwd_form(c.N, c.E0, c.E1) for c in lc.BWD_CASES if c.label.endswith("small_bwd") and c.kw.get("train", 1)}
    assert {cbk for cbk, _ in forms} >= {1, 4, 8} and any(cbk == 1 and t > 1 for cbk, t in forms) and any(t == 1 for _, t in forms)
    assert any(c.label == "small_bwd" and c.kw.get("in_place") is False for c in lc.BWD_CASES)
    assert all(isinstance(v, str) and v for v in lc.UNREACHABLE.values())


def test_the_mirror_at_the_edges_the_table_is_sized_from():
    ok = lc.small_ok
    assert ok(64, 128) and not ok(64, 129) and not ok(64, 152) and ok(7, 512) and not ok(8, 512) and not ok(65, 16) and not ok(4, 513)
    sb = lambda N, E0, E1, **k: lc.small_bwd(N, E0, E1, 256, **k)
    assert sb(128, 5, 256) == "small_bwd_cols" and sb(129, 5, 256) == "small_bwd"               # N E1 = 32768 | + E1
    assert sb(512, 16, 64) == "small_bwd_cols" and sb(513, 16, 64) == "small_bwd"               # N = 512 | 513
    assert sb(200, 51, 12) == "small_bwd_cols" and sb(200, 52, 12) == "small_bwd"               # E0 = 51 | 52
    assert sb(1024, 2, 256) == "thin_bwd_cols8" and sb(1025, 2, 256) == "thin_bwd_ticket"       # N = 1024 | 1025
    assert sb(9, 4, 8) == "thin_bwd_cols8" and sb(9, 4, 7) == "thin_bwd_ticket" and sb(9, 5, 7) == "small_bwd_cols"
    assert lc.small_bwd_form(64, 5, 256) == (1, 1) and lc.small_bwd_form(65, 5, 256) == (4, 2)  # the trip boundary at E1 = 256
    assert sb(600, 7, 512) == "refused:residency" and sb(600, 7, 512, in_place=False) == "small_bwd"
    assert sb(400, 7, 512) == "small_bwd" and sb(402, 7, 512) == "refused:residency"           # nA + nB = 200 + 56 | 201 + 56 against 256 CUs
    assert lc.small_fwd_label(16, 9) == "small_fwd_16" and lc.small_fwd_label(17, 9) == "small_fwd_32" and lc.small_fwd_label(33, 9) == "small_fwd_64"
    assert lc.dual(64, 256, 2048) == "dual_l32_4" and lc.dual(64, 260, 2048).startswith("dual_64")            # a1 = 512 | 520
    assert lc.dual(256, 68, 36) == "dual_l32_4" and lc.dual(257, 68, 36) == "dual_l32_rst4" and lc.dual(513, 68, 36) == "dual_l32_rst8"
    assert lc.dual(40, 70, 36) is None and lc.dual(2048, 68, 64) is None and lc.dual(4100, 8, 8) is None
    assert lc.head_bwd_ok(128, 2784, 128, 10) and not lc.head_bwd_ok(128, 2816, 128, 10)                       # 729 | 737 against 3 x 256 - 32
    assert lc.head_resident(33, 256, 3) == 2 and lc.head_resident(1, 4, 1) == 3
    assert lc.head_bwd_ok(1, 4, 4, 1) and not lc.head_bwd_ok(1, 4, 4, 17) and not lc.head_bwd_ok(257, 4, 4, 1) and not lc.head_bwd_ok(1, 4, 260, 1)
    assert lc.gemm_plan(33, 68, 100, 0, 1)[0] == "sliver" and lc.gemm_plan(40, 72, 896, 0, 1)[:2] == ("splitk", 2) and lc.gemm_plan(20, 70, 130, 0, 1)[0] == "unsplit"
    assert lc.gemm_plan(70, 36, 40, 1, 0, cs_rows=40)[3] and not lc.gemm_plan(68, 64, 2048, 1, 0, cs_rows=2048)[3]


def test_exact_pass_operands_keep_every_case_inside_2_24():
    """the precondition of the bit-equal pass, no case exempted: the analytic bound of linear_cases.exact_bound, and the largest magnitude any
    tensor of the case actually takes on the operands the sweep draws"""
    for c in lc.ALL_CASES:
        n, mag = lc.exact_bound(c)
        assert wt.is_int_exact(n, mag), "%s: %d terms of %g" % (c.id, n, mag)


# ----------------------------------------------------------------------------- two honest fp32 implementations
def blocked32(A, B):
    """A[M, K] @ B[K, N] in fp32: K in blocks of 32, each block's product in fp32, the blocks summed pairwise"""
    A = np.asarray(A, np.float32); B = np.asarray(B, np.float32)
    parts = [A[:, k:k + 32] @ B[k:k + 32] for k in range(0, A.shape[1], 32)]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0].astype(np.float32)


def honest_fwd(oracle, order, ops, stages=(), softmax=False, copy=False):
    o = oracle.lib(); P = oracle.P
    X, W, B = ops["X"], ops["W"], ops["B"]; N, E1 = X.shape; E0 = W.shape[0]
    if order == "oracle":
        Y = np.zeros((N, E0), np.float32); o.t4o_linear_fwd(P(X), P(W), P(B), P(Y), N, E0, E1)
    else:
        Y = (blocked32(X, W.T) + B).astype(np.float32)
    got = {"Y": Y, "X": X.copy(), "W": W.copy(), "B": B.copy()}
    o.t4o_rand_init(SEED); o.t4o_rand_set_offset(OFFSET)
    us, x = [], Y
    L = {"relu": oracle.L_RELU, "leaky": oracle.L_LEAKYRL, "drop": oracle.L_DROPOUT, "tanh": oracle.L_TANH}
    for i, st in enumerate(stages):
        f = np.zeros(N * E0, np.float32); y = np.zeros_like(Y)
        if st == "drop":
            o.t4o_dropout_mask(P(f), N * E0); us.append(f.copy())
        xc = np.ascontiguousarray(x)
        o.t4o_activate(L[st], P(xc), P(y), P(f), lc.ALPHA[st], N * E0)
        got["F%d" % i], got["A%d" % i] = f.reshape(Y.shape), y; x = y
    if softmax:
        Pr = np.zeros_like(Y); o.t4o_softmax(P(Y), P(Pr), N, E0); got["P"] = Pr
    if copy:
        got["C"] = X.copy()
    return got, us


def honest_bwd(oracle, order, ops, train=1, has_dw=True, tgt=False, masks=0, in_place=True):
    o = oracle.lib(); P = oracle.P
    X, W = ops["X"], ops["W"]; N, E1 = X.shape; E0 = W.shape[0]
    dy = (ops["DY"] - ops["T"]).astype(np.float32) if tgt else ops["DY"].copy()
    DW, DB = ops["DW0"].copy(), ops["DB0"].copy()
    tr = bool(train) and has_dw
    if order == "oracle":
        DX = np.zeros((N, E1), np.float32); Xc = X.copy()
        assert o.t4o_linear_bwd(P(Xc), P(W), P(dy), P(DX), P(DW), P(DB), N, E0, E1, 1 if tr else 0) == 0
    else:
        DX = blocked32(dy, W)
        if tr:
            DW = (DW + blocked32(dy.T, X)).astype(np.float32)
            DB = (DB + blocked32(np.ones((1, N), np.float32), dy)[0]).astype(np.float32)
    got = {"DX": DX, "DW": DW, "DB": DB, "DY": dy if tgt else ops["DY"].copy(), "W": W.copy(), "T": ops["T"].copy(), "X": X.copy()}
    if tgt:
        got["OUT2"] = dy.copy()
    g = DX
    for i in range(masks):
        g = (g * ops["M%d" % i]).astype(np.float32); got["D%d" % i] = g; got["M%d" % i] = ops["M%d" % i].copy()
    return got


def _layers(c):
    """the linear layers a case differentiates / evaluates: (N, E0, E1) each"""
    if c.entry in ("mlp_head_bwd", "mlp_block_bwd"):
        return [(c.N, c.E0, c.kw["H"]), (c.N, c.kw["H"], c.E1)]
    if c.entry == "mlp_head_fwd":
        return [(c.N, c.kw["H"], c.E1), (c.N, c.E0, c.kw["H"])]
    return [(c.N, c.E0, c.E1)]


@pytest.mark.parametrize("order", ["oracle", "blocked32"])
@pytest.mark.parametrize("case", lc.ALL_CASES, ids=[c.id for c in lc.ALL_CASES])
def test_honest_orders_pass_both_bars_on_every_shape(oracle, case, order):
    c = case; kw = c.kw
    fwd = c in lc.FWD_CASES
    for N, E0, E1 in _layers(c):
        for exact in (True, False):
            tag = "%s %s %s %dx%dx%d" % (c.id, order, "exact" if exact else "float", N, E0, E1)
            if fwd:
                stages = kw.get("stages", ()) if (E0, E1) == _layers(c)[0][1:] else ()
                softmax = (kw.get("softmax", False) or c.entry == "linear_softmax_fwd") and (N, E0, E1) == _layers(c)[-1]
                ops = lc.fwd_operands(exact, N, E0, E1)
                got, us = honest_fwd(oracle, order, ops, stages, softmax, kw.get("copy", False))
                lc.check_fwd(tag, exact, ops, got, stages, us, softmax, kw.get("copy", False))
            else:
                masks, tgt = kw.get("masks", 0), kw.get("tgt", False) or c.entry in ("loss_linear_bwd", "mlp_head_bwd", "mlp_block_bwd")
                flags = dict(train=kw.get("train", 1), has_dw=kw.get("has_dw", True), tgt=tgt, masks=masks)
                ops = lc.bwd_operands(exact, N, E0, E1, masks)
                for in_place in (True, False):
                    lc.check_bwd(tag, exact, ops, honest_bwd(oracle, order, ops, in_place=in_place, **flags), in_place=in_place, **flags)


# ----------------------------------------------------------------------------- injected defects
def _case(label, **kw):
    return next(c for c in lc.ALL_CASES if c.label == label and all(c.kw.get(k) == v for k, v in kw.items()))


def _bwd(oracle, c, exact, in_place=True):
    masks, tgt = c.kw.get("masks", 0), c.kw.get("tgt", False) or c.entry == "loss_linear_bwd"
    flags = dict(train=c.kw.get("train", 1), has_dw=c.kw.get("has_dw", True), tgt=tgt, masks=masks)
    ops = lc.bwd_operands(exact, c.N, c.E0, c.E1, masks)
    return ops, honest_bwd(oracle, "oracle", ops, in_place=in_place, **flags), flags


def _must_fail(text, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    assert text in str(e.value), str(e.value)[:300]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
def test_injected_defects_fail_their_cases(oracle, exact):
    """each defect is applied to the oracle's (passing) result of the named case and must fail the sweep's own assertion there:
      a dropped 32-deep K block, a K tail of 4 counted twice     gemm_sliver+riders  33 x 68 x 100 (three blocks and a tail of 4): Y
      a clamped edge row added into the last stored row          dual_l32_4          33 x 68 x 36 (ragged 32-tiles): dX, dW
      a dB that misses the last row group                        thin_bwd_ticket     1025 x 1 x 256 (129 row groups of 8, the last holds one row): dB
      the two masks of a chain applied to each other's tensors   dual_64_f11         64 x 1024 x 544, two masks: stage 0
      DW overwritten instead of accumulated                      small_bwd           129 x 5 x 256 (CBK = 4): dW
      out - target written to one destination only               small_bwd_cols      33 x 10 x 100 with a target: the second destination
      a sentinel word overwritten                                any guarded tensor: the word behind, the word in front"""
    c = _case("gemm_sliver+riders", copy=True)
    ops = lc.fwd_operands(exact, c.N, c.E0, c.E1)
    got, us = honest_fwd(oracle, "oracle", ops, c.kw["stages"], False, True)
    lc.check_fwd("honest", exact, ops, got, c.kw["stages"], us, False, True)
    X64, W64 = ops["X"].astype(np.float64), ops["W"].astype(np.float64)
    for name, delta in (("dropped block", -(X64[:, 32:64] @ W64[:, 32:64].T)), ("tail twice", X64[:, 96:] @ W64[:, 96:].T)):
        bad = dict(got); bad["Y"] = (got["Y"] + delta).astype(np.float32)
        _must_fail(" Y:", lambda: lc.check_fwd(name, exact, ops, bad, (), (), False, True))

    c = _case("dual_l32_4"); assert (c.N, c.E0, c.E1) == (33, 68, 36)
    ops, got, fl = _bwd(oracle, c, exact)
    lc.check_bwd("honest", exact, ops, got, **fl)
    bad = dict(got); bad["DX"] = got["DX"].copy(); bad["DX"][-1] += got["DX"][-1]
    _must_fail(" dX:", lambda: lc.check_bwd("clamped row in dX", exact, ops, bad, **fl))
    dy64 = ops["DY"].astype(np.float64)
    bad = dict(got); bad["DW"] = got["DW"].copy(); bad["DW"][-1] = (bad["DW"][-1] + dy64[:, -1] @ ops["X"].astype(np.float64)).astype(np.float32)
    _must_fail(" dW:", lambda: lc.check_bwd("clamped row in dW", exact, ops, bad, **fl))

    c = next(c for c in lc.BWD_CASES if c.label == "thin_bwd_ticket" and c.N == 1025)
    ops, got, fl = _bwd(oracle, c, exact)
    lc.check_bwd("honest", exact, ops, got, **fl)
    last = ops["DY"][8 * ((c.N - 1) // 8):].astype(np.float64).sum(0)
    assert np.all(last != 0), "the case's last row group sums to zero: reseed"
    bad = dict(got); bad["DB"] = (got["DB"] - last).astype(np.float32)
    _must_fail(" dB:", lambda: lc.check_bwd("dB short of a row group", exact, ops, bad, **fl))

    c = _case("dual_64_f11", masks=2)
    ops, got, fl = _bwd(oracle, c, exact)
    lc.check_bwd("honest", exact, ops, got, **fl)
    bad = dict(got); bad["D0"] = (got["DX"] * ops["M1"]).astype(np.float32); bad["D1"] = (bad["D0"] * ops["M0"]).astype(np.float32)
    _must_fail("mask chain stage 0", lambda: lc.check_bwd("masks swapped", exact, ops, bad, **fl))

    c = next(c for c in lc.BWD_CASES if c.label == "small_bwd" and (c.N, c.E0, c.E1) == (129, 5, 256))
    ops, got, fl = _bwd(oracle, c, exact)
    bad = dict(got); bad["DW"] = (got["DW"] - ops["DW0"]).astype(np.float32)
    _must_fail(" dW:", lambda: lc.check_bwd("DW overwritten", exact, ops, bad, **fl))

    c = _case("small_bwd_cols", tgt=True, masks=1)
    ops, got, fl = _bwd(oracle, c, exact)
    lc.check_bwd("honest", exact, ops, got, **fl)
    a, k, n = lc.guarded(got["OUT2"].shape)                                                      # what the sweep allocates and the call then never writes
    bad = dict(got); bad["OUT2"] = lc.unguard(a, k, n, got["OUT2"].shape)
    _must_fail("second destination", lambda: lc.check_bwd("one destination", exact, ops, bad, **fl))

    for off in (0, 4, 8):
        a, k, n = lc.guarded((5, 3), off, np.ones((5, 3)))
        assert a.size == n + 2 * lc.LEAD + off // 4 and np.array_equal(lc.unguard(a, k, n, (5, 3)), np.ones((5, 3)))
        for word in (k - 1, k + n, 0, a.size - 1):
            b = a.copy(); b[word] = 1.0
            _must_fail("guard word overwritten", lambda: lc.unguard(b, k, n, (5, 3), "t"))
