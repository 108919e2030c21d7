"""k_head_bwd_l32 (t4k_mlp_head_bwd / t4k_mlp_block_bwd) after its dependent chains were cut: the tiles' operand loads go out together, the
column riders ask for what DW2 / DB1 / DB2 hold together with their staging loads and accumulate with plain stores, the dX1 tiles look at the
in-place gate ahead of barrier 1.  Through the C ABI, on four small shapes (N, E1, EA, EB):

  (1, 4, 4, 1)        every lower edge
  (33, 36, 36, 3)     a ragged second sample block, ragged column tiles of both GEMMs, odd EB (the last MFMA k slot is padding), nine riders
  (40, 132, 96, 1)    three whole e blocks: waves 0 - 2 own one k block each, wave 3 none
  (128, 68, 100, 10)  the flagship's head on three column tiles: four k blocks for both tile kinds, 26 riders, dB2's rider present

Each shape checks
  * every tensor the reference materialises - P, Y2, dX2 over X2, Y1 (and Y1B with a second mask), DW2, DB2, DB1 - bit for bit, gradient
    buffers starting non-zero: P, Y2, X2, Y1, Y1B (and DW2 from EB = 5) against the separate entries t4k_loss_linear_bwd /
    t4k_linear_block_bwd + t4k_linear_bwd on the same operands, and DW2, DB2, DB1 against what the kernel left on these operands BEFORE the
    chains were cut (tests/golden/head_bwd_chain/parent_gradients.npz, recorded on an MI355X from the commit in front of this change).  The
    record is there because the separate entries are no bit reference for the three sums: k_linsmall_bwd_cols adds dB2 over n = 0 .. N - 1
    where the rider adds 16 row groups, t4k_linear_bwd's column sums are the dual launch's where the rider adds 64 row groups, and up to
    EB = 4 the separate head is a thin kernel with its own dW2 order - the kernel in front of this change differed from them in DB2 and DB1
    at every shape here but the first, and in DW2 at the two shapes with EB <= 4 behind it (measured with this file's operands).  All three
    are also held to the float64 witnesses; dW1 and dX1 against the witnesses and bars of tests/test_gpu_linear_sweep.py;
  * three calls back to back on one stream with no host synchronisation between them, X1, X2 and P re-uploaded in stream order, the four
    gradient tensors accumulating: each is held to its witness applied three times (the early-requested accumulators across launches, the
    re-tagged epochs of the arrival slots);
  * the mask-chain form (two masks behind either layer, train = 1) and the frozen form (train = 0: no dW1 tiles, no gate), every tensor held
    as the sweep holds it.
No tolerance of its own: lc.hold with the sweep's kinds, and bit equality."""
import ctypes
import os

import numpy as np
import pytest

import f64_witness as wt
import linear_cases as lc
from test_gpu_parity import Dev, PoolBlock
from test_gpu_linear_sweep import Buf, free, launches, run_head

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 4, 1), (33, 36, 36, 3), (40, 132, 96, 1), (128, 68, 100, 10)]
IDS = ["N%d-E1_%d-EA%d-EB%d" % s for s in SHAPES]
hold = lc.hold
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_bwd_chain", "parent_gradients.npz")


def gold_key(dims, masks, name):
    return "N%d_E1_%d_EA%d_EB%d_m%d_%s" % (tuple(dims) + (masks, name))


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


def operands(N, E1, EA, EB, exact, masks, salt):
    rng = np.random.default_rng(lc.seed_of(N, EB, E1, EA, exact, masks, salt))
    shp = dict(X1=(N, E1), W1=(EA, E1), X2=(N, EA), W2=(EB, EA), P=(N, EB), T=(N, EB), DW1=(EA, E1), DB1=EA, DW2=(EB, EA), DB2=EB)
    h = {k: lc.draw(rng, exact, v) for k, v in shp.items()}                                      # the gradient tensors start non-zero
    return h, [lc.draw_mask(rng, exact, (N, EA)) for _ in range(masks)]


def run2_block(oracle, bM, bR, x2):
    """the run between the linear layers as the entries take it: the dropout's mask multiplies first (its product lands in bR[0]), then the leaky one"""
    k = PoolBlock(); k.KS = 1
    k.post_layer, k.post_mask, k.post_out = oracle.L_DROPOUT, bM[0].ptr, x2
    if len(bM) == 2:
        k.pre_layer, k.pre_mask, k.pre_out = oracle.L_LEAKYRL, bM[1].ptr, bR[0].ptr
    return k


class Set:
    """one set of device tensors for a head backward"""

    def __init__(self, dev, h, M2):
        N, EA = h["X2"].shape; EB = h["P"].shape[1]
        self.b = {k: Buf(dev, v.shape, 0, v) for k, v in h.items()}
        self.M = [Buf(dev, m.shape, 0, m) for m in M2]
        self.R = [Buf(dev, (N, EA)) for _ in M2]                                                 # Y1, Y1B
        self.Y2 = Buf(dev, (N, EB))

    def fused(self, t4k, oracle, dims):
        N, E1, EA, EB = dims; b = self.b
        if len(self.M) == 1:
            return t4k.lib.t4k_mlp_head_bwd(b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, self.Y2.ptr, self.M[0].ptr, self.R[0].ptr, b["DW2"].ptr, b["DB2"].ptr,
                                            b["X1"].ptr, b["W1"].ptr, b["DW1"].ptr, b["DB1"].ptr, N, E1, EA, EB, None)
        k2 = run2_block(oracle, self.M, self.R, b["X2"].ptr)
        return t4k.lib.t4k_mlp_block_bwd(b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, self.Y2.ptr, ctypes.byref(k2), self.R[-1].ptr, b["DW2"].ptr, b["DB2"].ptr,
                                         b["X1"].ptr, b["W1"].ptr, None, None, b["DW1"].ptr, b["DB1"].ptr, N, E1, EA, EB, 1, None)

    def separate(self, t4k, oracle, dims):
        N, E1, EA, EB = dims; b = self.b
        if len(self.M) == 1:
            t4k.call("t4k_loss_linear_bwd", b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, self.Y2.ptr, b["X2"].ptr, self.M[0].ptr, self.R[0].ptr,
                     b["DW2"].ptr, b["DB2"].ptr, N, EB, EA, 1, None)
        else:
            k2 = run2_block(oracle, self.M, self.R, b["X2"].ptr)
            t4k.call("t4k_linear_block_bwd", b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, self.Y2.ptr, b["X2"].ptr, ctypes.byref(k2), self.R[-1].ptr,
                     b["DW2"].ptr, b["DB2"].ptr, N, EB, EA, 1, None)
        t4k.call("t4k_linear_bwd", b["X1"].ptr, b["W1"].ptr, self.R[-1].ptr, b["X1"].ptr, b["DW1"].ptr, b["DB1"].ptr, N, EA, E1, 1, None)

    def get(self, dev):
        out = {k: v.get(dev, k) for k, v in self.b.items()}
        out["Y2"] = self.Y2.get(dev, "Y2")
        for i, r in enumerate(self.R):
            out["Y1" if i == 0 else "Y1B"] = r.get(dev, "R2_%d" % i)
        return out


def admitted(t4k, dims):
    N, E1, EA, EB = dims
    assert t4k.lib.t4k_mlp_head_bwd_ok(N, E1, EA, EB) == 1, "%s no longer takes the one-launch head backward" % (dims,)


@pytest.mark.parametrize("masks", [1, 2])
@pytest.mark.parametrize("dims", SHAPES, ids=IDS)
def test_riders_tensors_bit_for_bit(t4k, dev, oracle, dims, masks):
    N, E1, EA, EB = dims
    admitted(t4k, dims)
    tag = "head chain %s masks %d" % (dims, masks)
    h, M2 = operands(N, E1, EA, EB, False, masks, 1)
    one, two = Set(dev, h, M2), Set(dev, h, M2)
    l0 = launches(t4k)
    rc = one.fused(t4k, oracle, dims)
    assert rc == 0, (tag, rc, t4k.lib.t4k_last_error().decode())
    assert launches(t4k) - l0 == 1, tag
    two.separate(t4k, oracle, dims)
    assert t4k.lib.t4k_sync(None) == 0, tag
    got, ref = one.get(dev), two.get(dev)
    for k in ("P", "Y2", "X2", "Y1", "Y1B") + (("DW2",) if EB >= 5 else ()):
        if k in got:
            wt.equal("%s: %s against the separate entries" % (tag, k), got[k], ref[k])
    with np.load(GOLD) as gold:
        for k in ("DW2", "DB2", "DB1"):
            wt.equal("%s: %s against the kernel in front of the change" % (tag, k), got[k], gold[gold_key(dims, masks, k)])
    g2 = h["P"] - h["T"]
    wt.equal(tag + " out - target in place", got["P"], g2, kind="linear exact: out - target")
    dy1 = got["Y1B"] if masks == 2 else got["Y1"]
    hold(False, tag + " dX1 (over X1)", got["X1"], wt.gemm(dy1, h["W1"]), "head dX1")
    hold(False, tag + " dW1", got["DW1"], wt.gemm(dy1, h["X1"], O0=h["DW1"], beta=1.0, tA=1), "head dW1")
    hold(False, tag + " dW2", got["DW2"], wt.gemm(g2, h["X2"], O0=h["DW2"], beta=1.0, tA=1), "head dW2")
    hold(False, tag + " dB2", got["DB2"], wt.dlinear_db(g2, h["DB2"]), "head dB2")
    hold(False, tag + " dB1", got["DB1"], wt.dlinear_db(dy1, h["DB1"]), "head dB1")
    for k in ("W1", "W2", "T"):
        wt.equal(tag + " %s untouched" % k, got[k], h[k])
    free(dev)


class Thrice(wt.W):
    """a witness applied three times: call i accumulates onto what call i - 1 left, so the bounds of the three applications add up"""

    def __init__(self, step, O0):
        exact, bound = wt.f64(O0), 0.0
        for _ in range(3):
            w = step(exact)
            exact, bound = w.exact, bound + w.bound()
        wt.W.__init__(self, exact, 0.0, 0)
        self.total = bound

    def bound(self):
        return self.total


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
@pytest.mark.parametrize("dims", SHAPES, ids=IDS)
def test_three_calls_back_to_back_accumulate(t4k, dev, oracle, dims, exact):
    N, E1, EA, EB = dims
    admitted(t4k, dims)
    assert wt.is_int_exact(3 * (max(N, EA) + 1), EB * 8 * 2 * 2), dims                           # the exact pass stays exact over three accumulations
    tag = "head chain %s three calls %s" % (dims, "exact" if exact else "float")
    h, M2 = operands(N, E1, EA, EB, exact, 1, 2)
    one = Set(dev, h, M2)
    fresh = {k: one.b[k].t.clone() for k in ("X1", "X2", "P")}                                   # device images, guard words included
    for rep in range(3):
        if rep:
            for k, t in fresh.items():
                one.b[k].t.copy_(t)                                                               # in stream order, no host synchronisation
        rc = one.fused(t4k, oracle, dims)
        assert rc == 0, (tag, rep, rc, t4k.lib.t4k_last_error().decode())
    assert t4k.lib.t4k_sync(None) == 0, tag
    got = one.get(dev)
    g2 = h["P"] - h["T"]
    wt.equal(tag + " out - target in place", got["P"], g2, kind="linear exact: out - target")
    wt.equal(tag + " out - target, second destination", got["Y2"], g2, kind="linear exact: out - target")
    hold(exact, tag + " dX2 (over X2)", got["X2"], wt.gemm(g2, h["W2"]), "head dX2")
    hold(exact, tag + " dY1", got["Y1"], wt.mul(got["X2"], M2[0]), "mask chain")
    dy1 = got["Y1"]
    hold(exact, tag + " dX1 (over X1)", got["X1"], wt.gemm(dy1, h["W1"]), "head dX1")
    hold(exact, tag + " dW2 x 3", got["DW2"], Thrice(lambda o: wt.gemm(g2, h["X2"], O0=o, beta=1.0, tA=1), h["DW2"]), "head dW2")
    hold(exact, tag + " dB2 x 3", got["DB2"], Thrice(lambda o: wt.dlinear_db(g2, o), h["DB2"]), "head dB2")
    hold(exact, tag + " dW1 x 3", got["DW1"], Thrice(lambda o: wt.gemm(dy1, h["X1"], O0=o, beta=1.0, tA=1), h["DW1"]), "head dW1")
    hold(exact, tag + " dB1 x 3", got["DB1"], Thrice(lambda o: wt.dlinear_db(dy1, o), h["DB1"]), "head dB1")
    free(dev)


@pytest.mark.parametrize("train", [1, 0], ids=["mask_chain", "frozen"])
@pytest.mark.parametrize("dims", SHAPES, ids=IDS)
def test_mask_chain_and_frozen_forms(t4k, dev, oracle, dims, train):
    """t4k_mlp_block_bwd with two masks behind the head and two behind the big layer: every tensor as the sweep's run_head holds it"""
    N, E1, EA, EB = dims
    admitted(t4k, dims)
    case = lc.Case("head_bwd_runs" + ("" if train else "_frozen"), "mlp_block_bwd", N, EB, E1, "the chain test's shape", H=EA, masks=2, train=train)
    for exact in (True, False):
        assert run_head(t4k, dev, oracle, case, exact, check_plan=False)
    free(dev)
