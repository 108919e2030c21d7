"""The linear-layer entries (linear.hip, linear_small.hip, and gemm_launch where a linear entry reaches it with riders) at every launch plan
their host-side dispatch branches on, through the C ABI: t4k_linear_fwd / _act_fwd / _block_fwd / _softmax_fwd, t4k_mlp_head_fwd,
t4k_linear_bwd / _bwd2, t4k_loss_linear_bwd, t4k_linear_block_bwd, t4k_mlp_head_bwd / t4k_mlp_block_bwd.

Every case of tests/linear_cases.py names the plan it is meant to reach; the plan is recomputed from the device's CU count with the Python
mirror of the dispatch and the case FAILS when it no longer reaches its label, and the launch count of the call is asserted.  Each case runs
  exact   operands in {-2 .. 2}, masks in {0, 1, 2}: every partial sum an integer (or a half) below 2^24, so EVERY tensor the call writes must
          be bit-equal to the float64 result - Y, the copy, masks and stage outputs, dX, each stage of the mask chain, DW, DB, out - target
          in both destinations, X1 / X2 / Y1 / Y2 of the head backward; dropout draws and the stream offset are the oracle's;
  float   standard-normal operands: the same tensors element by element inside the float64 witness's bound c n 2^-24 mag
          (tests/f64_witness.py: linear, gemm, dlinear_db, mul, act, softmax), each witnessed on the operands the call itself stored;
with guard words round every tensor, and every tensor the call must not touch bit-equal to what was uploaded.  Backward cases run with dX
over X and with dX apart wherever the entry allows both."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt
import gemm_cases as gc
import linear_cases as lc
from test_gpu_parity import Dev, PoolBlock, p

pytestmark = pytest.mark.gpu

SEED, OFFSET = 91, 1 << 18
UNSUPPORTED = -4
ALPHA = lc.ALPHA


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


class Buf:
    """a device tensor `off` bytes into a 16-byte aligned allocation, guard words on either side (linear_cases.guarded)"""

    def __init__(self, dev, shape, off=0, data=None):
        self.shape = tuple(np.atleast_1d(shape))
        a, self.k, self.n = lc.guarded(self.shape, off, data)
        self.t = dev.up(a); assert p(self.t) % 16 == 0
        self.ptr = p(self.t) + 4 * self.k

    def get(self, dev, name=""):
        return lc.unguard(dev.down(self.t), self.k, self.n, self.shape, name)


def launches(t4k):
    return int(t4k.lib.t4k_launch_count())


def cu_count(t4k):
    cu, khz, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    t4k.call("t4k_device_info", ctypes.byref(cu), ctypes.byref(khz), ctypes.byref(hbm))
    assert cu.value > 0
    return cu.value


def layer_id(oracle, st):
    return {"relu": oracle.L_RELU, "leaky": oracle.L_LEAKYRL, "drop": oracle.L_DROPOUT, "tanh": oracle.L_TANH}[st]


hold = lc.hold


def assert_label(t4k, case, want=None, **over):
    cu = cu_count(t4k)
    lab, n = case.plan(cu, **over)
    want = case.label if want is None else want
    assert lab == want, "%s: with %d CUs this case takes the plan %s, not %s - resize the table (tests/linear_cases.py)" % (case.id, cu, lab, want)
    return n


def assert_gemm_entry(t4k, tag, M, N, K, tA, tB, a_ptr, b_ptr, more=0):
    """behind an entry whose last product went through gemm_launch: t4k_gemm_plan, asked with the device's CU count, the real alignment of the
    product's A and B and what the entry hands gemm_launch (`more`: GP_BIAS, GP_RIDER), gives the text t4k_gemm_last_plan() reports"""
    want = t4k.lib.t4k_gemm_last_plan().decode()
    got = gc.plan_entry(t4k.lib, M, N, K, 1, tA, tB, gc.plan_flags(a_ptr, b_ptr, more=more), cu=cu_count(t4k))[0]
    assert got == want, "%s: t4k_gemm_plan() says %s, the launch took %s" % (tag, got, want)


def draws(oracle, sizes):
    """uniform draws of the dropout stages, in call order, from the oracle's stream; the offset behind them"""
    o = oracle.lib(); o.t4o_rand_init(SEED); o.t4o_rand_set_offset(OFFSET)
    out = []
    for n in sizes:
        u = np.zeros(n, np.float32); o.t4o_dropout_mask(oracle.P(u), n); out.append(u)
    return out, int(o.t4o_rand_offset())


# ----------------------------------------------------------------------------- forward
def run_fwd(t4k, dev, oracle, case, exact, want_label=None, check_plan=True, core=None, oskew=0):
    c = case; N, E0, E1 = c.N, c.E0, c.E1; kw = c.kw
    stages, copy, H = kw.get("stages", ()), kw.get("copy", False), kw.get("H", 0)
    softmax = kw.get("softmax", False) or c.entry == "linear_softmax_fwd"
    want_n = assert_label(t4k, c, want_label) if check_plan else None
    assert wt.is_int_exact(*lc.exact_bound(c)), c.id
    tag = "%s %s" % (c.id, "exact" if exact else "float")
    t4k.call("t4k_rand_init", SEED); t4k.call("t4k_rand_set_offset", OFFSET)
    head = c.entry == "mlp_head_fwd"
    EO = H if head else E0                                                                       # width of the (first) product
    ops = lc.fwd_operands(exact, N, EO, E1, core)
    us, off_want = draws(oracle, [N * EO for st in stages if st == "drop"])
    bX, bW, bB, bY = Buf(dev, (N, E1), kw.get("base_skew", 0), ops["X"]), Buf(dev, (EO, E1), 0, ops["W"]), Buf(dev, EO, 0, ops["B"]), Buf(dev, (N, EO), oskew)
    sb = [(Buf(dev, (N, EO), oskew), Buf(dev, (N, EO), oskew)) for _ in stages]
    bP = Buf(dev, (N, E0), oskew) if softmax else None
    bC = Buf(dev, (N, E1), oskew) if copy else None
    if head:
        ops2 = lc.fwd_operands(exact, N, E0, H)
        bW2, bB2, bY2 = Buf(dev, (E0, H), 0, ops2["W"]), Buf(dev, E0, 0, ops2["B"]), Buf(dev, (N, E0), oskew)
    l0 = launches(t4k)
    if head:
        t4k.call("t4k_mlp_head_fwd", bX.ptr, bW.ptr, bB.ptr, bY.ptr, layer_id(oracle, stages[0]), ALPHA[stages[0]], sb[0][0].ptr, sb[0][1].ptr,
                 bW2.ptr, bB2.ptr, bY2.ptr, bP.ptr if softmax else None, N, H, E1, E0, None)
    elif c.entry == "linear_fwd":
        t4k.call("t4k_linear_fwd", bX.ptr, bW.ptr, bB.ptr, bY.ptr, N, E0, E1, None)
    elif c.entry == "linear_softmax_fwd":
        t4k.call("t4k_linear_softmax_fwd", bX.ptr, bW.ptr, bB.ptr, bY.ptr, bP.ptr, N, E0, E1, None)
    elif c.entry == "linear_act_fwd":
        t4k.call("t4k_linear_act_fwd", bX.ptr, bW.ptr, bB.ptr, bY.ptr, layer_id(oracle, stages[0]), ALPHA[stages[0]], sb[0][0].ptr, sb[0][1].ptr, N, E0, E1, None)
    else:
        blk = PoolBlock(); blk.KS = 1
        if len(stages) == 2 or (len(stages) == 1 and stages[0] != "drop"):
            blk.pre_layer, blk.pre_alpha, blk.pre_mask, blk.pre_out = layer_id(oracle, stages[0]), ALPHA[stages[0]], sb[0][0].ptr, sb[0][1].ptr
        elif len(stages) == 1:                              # a lone dropout sits in the post slot
            blk.post_layer, blk.post_alpha, blk.post_mask, blk.post_out = layer_id(oracle, stages[0]), ALPHA[stages[0]], sb[0][0].ptr, sb[0][1].ptr
        if len(stages) == 2:
            blk.post_layer, blk.post_alpha, blk.post_mask, blk.post_out = layer_id(oracle, stages[1]), ALPHA[stages[1]], sb[1][0].ptr, sb[1][1].ptr
        t4k.call("t4k_linear_block_fwd", bX.ptr, bC.ptr if copy else None, bW.ptr, bB.ptr, bY.ptr, ctypes.byref(blk) if stages else None, N, E0, E1, None)
    n = launches(t4k) - l0; off = int(t4k.lib.t4k_rand_offset())
    if not head and not lc.small_ok(E0, E1):                # Y = X W^T + B on gemm_launch: an activation epilogue or the block's rider is asked for
        asked = c.entry == "linear_block_fwd" or (c.entry == "linear_act_fwd" and bool(stages))
        assert_gemm_entry(t4k, tag, N, E0, E1, 0, 1, bX.ptr, bW.ptr, gc.GP_BIAS | (gc.GP_RIDER if asked else 0))
    assert t4k.lib.t4k_sync(None) == 0, tag
    got = {"Y": bY.get(dev, tag + " Y"), "X": bX.get(dev, "X"), "W": bW.get(dev, "W"), "B": bB.get(dev, "B")}
    for i, (f, a) in enumerate(sb):
        got["F%d" % i], got["A%d" % i] = f.get(dev, tag + " F"), a.get(dev, tag + " A")
    if softmax and not head:
        got["P"] = bP.get(dev, tag + " P")
    if copy:
        got["C"] = bC.get(dev, tag + " copy")
    a1 = lc.check_fwd(tag + (" layer 1" if head else ""), exact, ops, got, stages, us, softmax and not head, copy)
    assert off == off_want, "%s: stream offset %d, oracle %d" % (tag, off, off_want)
    if head:
        got2 = {"Y": bY2.get(dev, tag + " Y2"), "W": bW2.get(dev, "W2"), "B": bB2.get(dev, "B2")}
        if softmax:
            got2["P"] = bP.get(dev, tag + " P2")
        lc.check_fwd(tag + " layer 2", exact, dict(X=a1, W=ops2["W"], B=ops2["B"]), got2, softmax=softmax)
    if check_plan:
        assert n == want_n, "%s: %d launches, the plan %s makes %d" % (tag, n, want_label or c.label, want_n)
    return got


# ----------------------------------------------------------------------------- backward
def run_bwd(t4k, dev, oracle, case, exact, in_place, want_label=None, check_plan=True, core=None, oskew=0):
    c = case; N, E0, E1 = c.N, c.E0, c.E1; kw = c.kw
    train, has_dw, masks = kw.get("train", 1), kw.get("has_dw", True), kw.get("masks", 0)
    tgt = kw.get("tgt", False) or c.entry == "loss_linear_bwd"
    want_n = assert_label(t4k, c, want_label, in_place=in_place) if check_plan else None
    assert wt.is_int_exact(*lc.exact_bound(c)), c.id
    tag = "%s %s %s" % (c.id, "exact" if exact else "float", "in place" if in_place else "apart")
    ops = lc.bwd_operands(exact, N, E0, E1, masks, core)
    b = {k: Buf(dev, v.shape, 0, v) for k, v in ops.items()}
    bD = [Buf(dev, (N, E1), oskew) for _ in range(masks)]                                        # bD[0] = dX * M0, bD[1] = bD[0] * M1
    bDX = b["X"] if in_place else Buf(dev, (N, E1), oskew)
    bDY2 = Buf(dev, (N, E0), oskew) if tgt else None
    pDW, pDB = (b["DW0"].ptr, b["DB0"].ptr) if has_dw else (None, None)
    X, W, DY, T = b["X"].ptr, b["W"].ptr, b["DY"].ptr, b["T"].ptr
    l0 = launches(t4k)
    if c.entry == "linear_bwd" and not masks:
        t4k.call("t4k_linear_bwd", X, W, DY, bDX.ptr, pDW, pDB, N, E0, E1, train, None)
    elif c.entry == "linear_bwd":
        t4k.call("t4k_linear_bwd2", X, W, DY, bDX.ptr, b["M0"].ptr, bD[0].ptr, pDW, pDB, N, E0, E1, train, None)
    elif c.entry == "loss_linear_bwd":
        t4k.call("t4k_loss_linear_bwd", X, W, DY, T, bDY2.ptr, bDX.ptr, b["M0"].ptr if masks else None, bD[0].ptr if masks else None,
                 pDW, pDB, N, E0, E1, train, None)
    else:
        blk = PoolBlock(); blk.KS = 1
        blk.post_layer, blk.post_mask, blk.post_out = oracle.L_DROPOUT, b["M0"].ptr, X
        if masks == 2:
            blk.pre_layer, blk.pre_mask, blk.pre_out = oracle.L_LEAKYRL, b["M1"].ptr, bD[0].ptr
        t4k.call("t4k_linear_block_bwd", X, W, DY, T if tgt else None, bDY2.ptr if tgt else None, bDX.ptr, ctypes.byref(blk),
                 bD[-1].ptr, pDW, pDB, N, E0, E1, train, None)
    n = launches(t4k) - l0
    lab = want_label or c.label
    if "dx_only" in lab:                                    # dX = dY W on gemm_launch with the mask chain as its rider
        assert_gemm_entry(t4k, tag, N, E1, E0, 0, 0, DY, W, gc.GP_RIDER)
    elif "+dx_" in lab or lab.startswith("dx_"):            # the separate launches: dX = dY W is the last product
        assert_gemm_entry(t4k, tag, N, E1, E0, 0, 0, DY, W)
    assert t4k.lib.t4k_sync(None) == 0, tag
    got = {"DX": bDX.get(dev, tag + " DX"), "DW": b["DW0"].get(dev, tag + " DW"), "DB": b["DB0"].get(dev, tag + " DB"), "DY": b["DY"].get(dev, tag + " DY"),
           "W": b["W"].get(dev, "W"), "T": b["T"].get(dev, "T"), "X": b["X"].get(dev, "X")}
    if tgt:
        got["OUT2"] = bDY2.get(dev, tag + " OUT2")
    for i in range(masks):
        got["D%d" % i], got["M%d" % i] = bD[i].get(dev, tag + " chain"), b["M%d" % i].get(dev, "M")
    lc.check_bwd(tag, exact, ops, got, train=train, has_dw=has_dw, tgt=tgt, masks=masks, in_place=in_place)
    if check_plan:
        assert n == want_n, "%s: %d launches, the plan %s makes %d" % (tag, n, want_label or c.label, want_n)
    return got


def run_head(t4k, dev, oracle, case, exact, check_plan=True):
    """t4k_mlp_head_bwd / t4k_mlp_block_bwd: (N, EB, E1) = (case.N, case.E0, case.E1), EA = H"""
    c = case; N, EB, E1, EA = c.N, c.E0, c.E1, c.kw["H"]; kw = c.kw
    train, masks, runs = kw.get("train", 1), kw.get("masks", 1), c.entry == "mlp_block_bwd"
    cu = cu_count(t4k)
    ok = t4k.lib.t4k_mlp_head_bwd_ok(N, E1, EA, EB) == 1
    assert ok == lc.head_bwd_ok(N, E1, EA, EB, cu), "%s: t4k_mlp_head_bwd_ok says %d, the mirror %d with %d resident workgroups per CU at %d bytes of LDS" % (
        c.id, ok, not ok, lc.head_resident(N, EA, EB), lc.head_bwd_lds(N, EA, EB))
    want_n = assert_label(t4k, c) if check_plan else (1 if ok else 0)
    assert wt.is_int_exact(*lc.exact_bound(c)), c.id
    rng = np.random.default_rng(lc.seed_of(N, EB, E1, EA, exact, 3))
    tag = "%s %s" % (c.id, "exact" if exact else "float")
    shp = dict(X1=(N, E1), W1=(EA, E1), X2=(N, EA), W2=(EB, EA), P=(N, EB), T=(N, EB), DW1=(EA, E1), DB1=EA, DW2=(EB, EA), DB2=EB)
    h = {k: lc.draw(rng, exact, v) for k, v in shp.items()}
    M2 = [lc.draw_mask(rng, exact, (N, EA)) for _ in range(masks)]
    M1 = [lc.draw_mask(rng, exact, (N, E1)) for _ in range(masks if runs else 0)]
    b = {k: Buf(dev, v.shape, 0, v) for k, v in h.items()}
    bM2 = [Buf(dev, m.shape, 0, m) for m in M2]; bM1 = [Buf(dev, m.shape, 0, m) for m in M1]
    bR2 = [Buf(dev, (N, EA)) for _ in M2]; bR1 = [Buf(dev, (N, E1)) for _ in M1]
    bY2 = Buf(dev, (N, EB))
    SENT = np.float32(4242.5)
    if not ok:                                                                                   # a refusal must write nothing: sentinels instead of NaN
        bR2 = [Buf(dev, (N, EA), 0, np.full((N, EA), SENT)) for _ in M2]; bY2 = Buf(dev, (N, EB), 0, np.full((N, EB), SENT))

    def block(bm, bd, first_out):
        k = PoolBlock(); k.KS = 1
        k.post_layer, k.post_mask, k.post_out = oracle.L_DROPOUT, bm[0].ptr, first_out
        if len(bm) == 2:
            k.pre_layer, k.pre_mask, k.pre_out = oracle.L_LEAKYRL, bm[1].ptr, bd[0].ptr
        return k
    l0 = launches(t4k)
    if not runs:
        rc = t4k.lib.t4k_mlp_head_bwd(b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, bY2.ptr, bM2[0].ptr, bR2[0].ptr, b["DW2"].ptr, b["DB2"].ptr,
                                      b["X1"].ptr, b["W1"].ptr, b["DW1"].ptr, b["DB1"].ptr, N, E1, EA, EB, None)
    else:
        k2 = block(bM2, bR2, b["X2"].ptr); k1 = block(bM1, bR1, b["X1"].ptr)
        rc = t4k.lib.t4k_mlp_block_bwd(b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, bY2.ptr, ctypes.byref(k2), bR2[-1].ptr, b["DW2"].ptr, b["DB2"].ptr,
                                       b["X1"].ptr, b["W1"].ptr, ctypes.byref(k1), bR1[-1].ptr, b["DW1"].ptr, b["DB1"].ptr, N, E1, EA, EB, train, None)
    n = launches(t4k) - l0
    assert n == want_n, "%s: %d launches, expected %d" % (tag, n, want_n)
    if not ok:
        assert rc == UNSUPPORTED and "t4k_mlp_head_bwd_ok" in t4k.lib.t4k_last_error().decode(), (tag, rc)
        for k, v in b.items():
            wt.equal(tag + " refusal left %s alone" % k, v.get(dev, k), h[k])
        for bm, m in zip(bM2 + bM1, M2 + M1):
            wt.equal(tag + " refusal left a mask alone", bm.get(dev, "M"), m)
        assert np.all(bY2.get(dev, "Y2") == SENT) and all(np.all(x.get(dev, "R2") == SENT) for x in bR2), tag + ": a refusal wrote an output"
        return None
    assert rc == 0, (tag, rc, t4k.lib.t4k_last_error().decode())
    assert t4k.lib.t4k_sync(None) == 0, tag
    g2 = h["P"] - h["T"]
    wt.equal(tag + " out - target in place", b["P"].get(dev, "P"), g2, kind="linear exact: out - target")
    wt.equal(tag + " out - target, second destination", bY2.get(dev, "Y2"), g2, kind="linear exact: out - target")
    dx2 = b["X2"].get(dev, "X2")
    hold(exact, tag + " dX2 (over X2)", dx2, wt.gemm(g2, h["W2"]), "head dX2")
    g = dx2
    for i in range(masks):
        d = bR2[i].get(dev, "R2_%d" % i)
        hold(exact, tag + " head run stage %d" % i, d, wt.mul(g, M2[i]), "mask chain")
        g = d
    dy1 = g
    dx1 = b["X1"].get(dev, "X1")
    hold(exact, tag + " dX1 (over X1)", dx1, wt.gemm(dy1, h["W1"]), "head dX1")
    g = dx1
    for i in range(len(M1)):
        d = bR1[i].get(dev, "R1_%d" % i)
        hold(exact, tag + " big layer's run stage %d" % i, d, wt.mul(g, M1[i]), "mask chain")
        g = d
    got = {k: b[k].get(dev, k) for k in ("DW1", "DB1", "DW2", "DB2")}
    if train:
        hold(exact, tag + " dW2", got["DW2"], wt.gemm(g2, h["X2"], O0=h["DW2"], beta=1.0, tA=1), "head dW2")
        hold(exact, tag + " dB2", got["DB2"], wt.dlinear_db(g2, h["DB2"]), "head dB2")
        hold(exact, tag + " dW1", got["DW1"], wt.gemm(dy1, h["X1"], O0=h["DW1"], beta=1.0, tA=1), "head dW1")
        hold(exact, tag + " dB1", got["DB1"], wt.dlinear_db(dy1, h["DB1"]), "head dB1")
    else:
        for k in got:
            wt.equal(tag + " %s untouched (frozen)" % k, got[k], h[k])
    for k in ("W1", "W2", "T"):
        wt.equal(tag + " %s untouched" % k, b[k].get(dev, k), h[k])
    for i, m in enumerate(M2 + M1):
        wt.equal(tag + " mask %d untouched" % i, (bM2 + bM1)[i].get(dev, "M"), m)
    return True


def free(dev):
    del dev.keep[:]; dev.torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 1. every plan
@pytest.mark.parametrize("case", lc.FWD_CASES, ids=[c.id for c in lc.FWD_CASES])
def test_forward_at_every_plan(t4k, dev, oracle, case):
    for exact in (True, False):
        run_fwd(t4k, dev, oracle, case, exact)
    free(dev)


@pytest.mark.parametrize("case", lc.BWD_CASES, ids=[c.id for c in lc.BWD_CASES])
def test_backward_at_every_plan(t4k, dev, oracle, case):
    """in place or apart as the row says, both passes; then the other placement with the plan the mirror gives for it"""
    first = case.kw.get("in_place", True)
    for exact in (True, False):
        run_bwd(t4k, dev, oracle, case, exact, first)
    if "in_place" not in case.kw:                                                                # the row does not pin the placement: dX apart as well
        lab, _ = case.plan(cu_count(t4k), in_place=False)
        for exact in (True, False):
            run_bwd(t4k, dev, oracle, case, exact, False, want_label=lab)
    free(dev)


@pytest.mark.parametrize("case", lc.HEAD_CASES, ids=[c.id for c in lc.HEAD_CASES])
def test_head_backward_at_every_plan_and_refusal(t4k, dev, oracle, case):
    for exact in (True, False):
        run_head(t4k, dev, oracle, case, exact)
    free(dev)


SKEWED = ("thin_fwd_vec+stage", "small_fwd_16+softmax", "small_fwd_32+stage", "gemm_sliver+riders", "gemm_splitk+riders", "gemm_unsplit+separate",
          "gemm_sliver_deferred+small_fwd_16_narrow", "thin_bwd_cols8", "thin_bwd_ticket", "small_bwd_cols", "small_bwd", "dual_l32_4", "dual_l32_rst8",
          "dual_64_f00", "separate_colsum_rider+dw_unsplit+dx_unsplit", "dx_only_fold_rider:sliver", "dx_only_fold_rider:splitk", "dx_only_unfused:unsplit")


@pytest.mark.parametrize("label", SKEWED)
def test_outputs_from_skewed_bases(t4k, dev, oracle, label):
    """every tensor the call only WRITES (Y, stage masks and outputs, P, the copy; dX apart, the chain's tensors, the second destination of
    out - target) 4, then 8 bytes into its allocation: the dispatch looks at the operands' alignment alone, so the plan and the launch count
    stay, the exact pass stays bit-equal and the guard words on either side of every tensor stay intact"""
    c = _representative(label)
    for off in (4, 8):
        if c in lc.FWD_CASES:
            run_fwd(t4k, dev, oracle, c, True, oskew=off)
        else:
            run_bwd(t4k, dev, oracle, c, True, False, want_label=c.plan(cu_count(t4k), in_place=False)[0], oskew=off)
    free(dev)


# ----------------------------------------------------------------------------- 2. state between launches
def _euler(n):
    """a closed walk over the complete directed graph on n nodes that takes every edge once: every node follows every other"""
    out = {i: [j for j in range(n) if j != i] for i in range(n)}
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


B2B = ("thin_bwd_cols8", "thin_bwd_ticket", "small_bwd_cols", "small_bwd", "dual_l32_4", "dual_l32_rst8", "dual_64_f00",
       "separate_colsum_add+dw_splitk+dx_sliver", "dx_only_fold_rider:splitk", "head_bwd", "head_bwd_runs",
       "gemm_splitk+riders", "gemm_sliver_deferred+small_fwd_16_narrow")


def _representative(label):
    """the first row of the label that carries a target (the shared counters serve the in-place out - target), else its first row"""
    rows = [c for c in lc.ALL_CASES if c.label == label]
    return next((c for c in rows if c.kw.get("tgt") or c.entry == "loss_linear_bwd"), rows[0])


def test_plans_back_to_back_leave_the_gate_block_clean(t4k, dev, oracle):
    """one exact-operand case of every backward family and of the forward forms that pass slabs between launches, on one stream, in an order
    in which every one follows every other (a closed walk over all ordered pairs), twice through; targets ride wherever a row has one, dX goes
    in place (the gated form).  Every call's tensors are checked: a ticket, counter, arrival slot or epoch that one kernel leaves behind and
    the next one trips over shows as a wrong tensor or a bounded-spin error"""
    reps = [_representative(lab) for lab in B2B]
    walk = _euler(len(reps))
    steps = set(zip(walk, walk[1:]))
    assert all((a, b) in steps for a in range(len(reps)) for b in range(len(reps)) if a != b)
    for rep in range(2):
        for i in walk:
            c = reps[i]
            if c in lc.HEAD_CASES:
                run_head(t4k, dev, oracle, c, True, check_plan=False)
            elif c in lc.FWD_CASES:
                run_fwd(t4k, dev, oracle, c, True, check_plan=False)
            else:
                run_bwd(t4k, dev, oracle, c, True, c.kw.get("in_place", True), check_plan=False)
        free(dev)
    assert t4k.lib.t4k_sync(None) == 0


# ----------------------------------------------------------------------------- 3. the linear_small_ok boundary
@pytest.mark.parametrize("pair", lc.BOUNDARY_PAIRS, ids=["%dx%d_%dx%d" % (a + b) for a, b in lc.BOUNDARY_PAIRS])
def test_small_ok_boundary_pairs(t4k, dev, oracle, pair):
    """either side of each boundary, forward and backward (in place and apart), on exact operands: the two sides take different plans and both
    equal the float64 result.  The far side's operands are the near side's with a zero row of W / column of X appended, so the two runs are the
    same sums: what both sides write at equal indices must also agree with each other bit for bit"""
    cu = cu_count(t4k)
    (a0, a1), (b0, b1) = pair
    for N in (6, 40):
        plans, outs = [], []
        for E0, E1 in pair:
            f = lc.Case("?", "linear_fwd", N, E0, E1, "boundary")
            bw = lc.Case("?", "linear_bwd", N, E0, E1, "boundary")
            f.label, bw.label = f.plan(cu)[0], bw.plan(cu)[0]
            o = {"fwd": run_fwd(t4k, dev, oracle, f, True, core=(a0, a1)),
                 "in place": run_bwd(t4k, dev, oracle, bw, True, True, core=(a0, a1)),
                 "apart": run_bwd(t4k, dev, oracle, bw, True, False, want_label=bw.plan(cu, in_place=False)[0], core=(a0, a1))}
            plans.append((f.label, bw.label)); outs.append(o)
        assert plans[0][0] != plans[1][0] and plans[0][1] != plans[1][1], "N = %d: both sides of %s take the plans %s" % (N, pair, plans)
        for run in outs[0]:
            for k in ("Y", "DX", "DW", "DB"):
                if k in outs[0][run]:
                    x, y = outs[0][run][k], outs[1][run][k]
                    cut = tuple(slice(0, s) for s in x.shape)
                    assert np.array_equal(x, y[cut]), "N = %d %s %s: the two sides of %s differ" % (N, run, k, pair)
    free(dev)


def test_zz_report_worst_ratios():
    """the worst |error| / bound per tensor kind over everything above (pytest -s prints it; tests/README.md quotes it)"""
    print("\nlinear sweep, worst |err| / bound per tensor kind:")
    for kind in sorted(k for k in wt.WORST if k.startswith("linear")):
        print("  %-40s %.3g   %s" % (kind, wt.WORST[kind][0], wt.WORST[kind][1]))
        assert wt.WORST[kind][0] <= 1.0
