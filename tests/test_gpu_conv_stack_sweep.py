"""The sample-resident conv stack across the geometries it admits (K = 3 | 5, C1 / C0 <= 32, H W <= 4096, C1 K^2 C0 <= 4096, 1 - 3 stages),
against the oracle's separate layers (as tests/test_gpu_conv_stack.py) AND against float64 element by element (tests/f64_witness.py).
Every row names the kernel branch or launch plan it exists for; N is derived from the device's CU count, because the plan - forward bands
`split`, backward bands `bsplit`, 1 - 4 each - follows from N (t4k_conv_stack_plan reports it).  The coverage test asserts that the rows
reach every split and every bsplit, and the branches ROWT, VALU forward, dx_valu and two N tiles."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt
from test_gpu_conv_stack import (ConvStage, StackHead, _build, _lay, _oracle_backward, _oracle_forward, _params, BWD_KEYS, FWD_KEYS,
                                 down_stage, oracle_bwd_as_got, witness_backward, witness_forward, witness_head)
from test_gpu_parity import Dev, p, rel

pytestmark = pytest.mark.gpu
RTOL = 1e-4

# N: an int, or a share of the CU count - "cu/4" (4 bands fit: N * 4 <= CUs), "cu/3", "cu/2", "cu/2+1" (two bands would not: one band)
# (N, H, W, C_in, [(C0, K, pre, pool, post)], flatten, head (EA, EB, mid) or None, whole-image backward fits)
# The last field: the whole-image backward (`train | 2`, or bsplit = 1) keeps the image's dO / input windows, both dX buffers and the dF slot
# in LDS; past 38 K floats t4k_conv_stack_bwd_ok says 0, t4k_conv_stack_bwd refuses, and the host runs its per-layer backward instead
# (model.cpp asks bwd_ok first).  Rows marked False assert exactly that refusal.
ROWS = [
    ("cu/4", 12, 12, 3, [(8, 5, "relu", "max", None), (16, 3, None, None, "elu")], True, (64, 10, "relu"), True),
    #   K = 5 at stage 0 with W = 12: ROWT (W < 16 <= W + K - 1); C1 = 3 VALU forward; split 4 over H0 = 6 (bands of 1 and 2 rows); head
    ("cu/3", 10, 15, 1, [(6, 5, "tanh", None, None)], False, None, True),
    #   K = 5, W = 15 (last ROWT width), odd W without a pool, non-square; C1 = 1, nF = 150: dx_valu; split 3 over H0 = 10 (3, 3, 4 rows)
    ("cu/2", 9, 11, 5, [(17, 5, None, None, "leaky")], False, None, True),
    #   K = 5, W = 11 (just below ROWT: W + K - 1 = 15); C1 = 5: MFMA forward (VALU needs C1 <= 4); C0 = 17: two N tiles; odd H0 = 9, split 2
    ("cu/4", 16, 16, 4, [(16, 5, "selu", "avg", None), (28, 3, None, "min", "relu")], True, None, False),
    #   K = 5, W = 16 (above ROWT); C1 = 4 / C0 = 16: VALU forward, C1 = 4 nF = 1600: MFMA dX; stage 1 C0 = 28: two N tiles, nF = 4032;
    #   whole image: 39 520 floats (the K = 5 dF slot), banded: fits
    ("cu/4", 14, 14, 10, [(20, 3, "dropout", "max", "relu")], True, (37, 5, "dropout"), True),
    #   K = 3, W = 14: ROWT (LeNet's second stage as a stack of its own); C1 = 10; split 4 over H0 = 7 (1, 2, 2, 2 rows); head
    ("cu/3", 7, 13, 32, [(14, 3, None, None, "sigmoid")], False, None, True),
    #   K = 3, W = 13 (below ROWT), odd H and W; C1 = 32: filter volume 32 * 9 * 14 = 4032 (the limit is 4096); sigmoid: forward only
    ("cu/4", 16, 16, 17, [(26, 3, "elu", "max", None)], True, None, False),
    #   K = 3, W = 16 (above ROWT); C1 = 17 (above 16: two dX N tiles), C0 = 26 (two N tiles), nF = 3978
    ("cu/4", 64, 64, 1, [(4, 3, "relu", "max", None), (8, 3, None, "avg", "tanh"), (8, 3, None, "max", None)], True, (32, 16, "tanh"), False),
    #   the 64 x 64 grid (H W = 4096); C0 = 4 with 16+ M tiles per band: two tiles per wave (TPW); three stages, every pool kind; head
    ("cu/2", 16, 16, 3, [(8, 3, "leaky", "max", None), (12, 5, None, "max", "relu"), (6, 3, "dropout", None, None)], True, None, True),
    #   K = 5 at a LATER stage (W = 8), three stages; split 2
    ("cu/4", 16, 16, 2, [(6, 3, None, "max", "relu"), (9, 3, None, "max", None)], True, None, True),
    #   H0 of the last stage = 4 = the band count: every band owns one row; C1 = 2 nF = 108: dx_valu
    ("cu/3", 12, 12, 4, [(8, 3, "relu", "max", None), (8, 3, None, "max", None)], True, (20, 7, None), True),
    #   H0 of the last stage = 3 = the band count (split 3); head without a middle layer
    ("cu/2+1", 8, 8, 32, [(12, 3, None, None, "relu"), (32, 3, "tanh", "max", None)], True, None, False),
    #   C1 = 32 at stage 0 (nF = 3456), C0 = 32 at stage 1 (nF = 3456), a stage without a pool in front; one band (whole image: too large)
    ("cu/2+1", 8, 8, 4, [(8, 3, "relu", "max", None), (16, 3, None, None, "tanh")], True, None, True),
    #   one band whose whole-image backward fits: bsplit 1 runs (N > CUs / 2); C1 = 4 nF = 288: MFMA dX
]


# just outside the limits: t4k_conv_stack_ok must refuse (the model then runs its per-layer kernels)
REFUSED = [
    (4, 8, 8, 33, 8, 3, False),          # C1 = 33
    (4, 8, 8, 8, 33, 3, False),          # C0 = 33
    (4, 8, 8, 4, 4, 7, False),           # K = 7
    (4, 41, 100, 1, 4, 3, False),        # H W = 4100
    (4, 8, 8, 32, 15, 3, False),         # filter volume 32 * 9 * 15 = 4320 > 4096
    (4, 7, 8, 4, 4, 3, True),            # odd H with a pool
]


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def n_of(spec):
    if isinstance(spec, int):
        return spec
    cu = cu_count()
    return {"cu/4": cu // 4, "cu/3": cu // 3, "cu/2": cu // 2, "cu/2+1": cu // 2 + 1}[spec]


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


def _setup(dev, oracle, row, seed):
    spec, H, W, Cin, stages, flat, _head, _whole = ROWS[row]
    N = n_of(spec)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    params = _params(rng, Cin, stages)
    ref, end = _oracle_forward(oracle, X, stages, flat, params, seed, 4096)
    arr, bufs = _build(dev, oracle, X, stages, flat, params, ref)
    return N, rng, X, stages, flat, params, ref, end, arr, bufs


def plan(t4k, arr, n_stage, N):
    sp, bs = ctypes.c_int(0), ctypes.c_int(0)
    ok = t4k.lib.t4k_conv_stack_plan(arr, n_stage, N, ctypes.byref(sp), ctypes.byref(bs))
    return ok, sp.value, bs.value


def _check_fwd_vs_oracle(dev, stages, ref, bufs, tag):
    for si, (C0, K, pre, pool, post) in enumerate(stages):
        t, d = ref[si], bufs[si]
        for k_ in FWD_KEYS:
            if k_ not in t:
                continue
            got = dev.down(d[k_]).reshape(t[k_].shape)
            if k_.endswith("mask"):
                which = pre if k_ == "pre_mask" else post
                if which == "dropout":
                    assert np.array_equal(got, t[k_]), "%s stage %d %s" % (tag, si, k_)
                else:
                    assert np.mean(np.abs(got - t[k_]) > 1e-3) < 1e-4, "%s stage %d %s" % (tag, si, k_)
                continue
            assert rel(got, t[k_]) < RTOL, "%s stage %d %s: %.3g" % (tag, si, k_, rel(got, t[k_]))


def _check_bwd_vs_oracle(dev, stages, want, bufs, tag, skip_dx0=False):
    for si in range(len(stages) - 1, -1, -1):
        t, d = want[si], bufs[si]
        if not (skip_dx0 and si == 0):
            assert rel(dev.down(d["DXS"]), t["DX"]) < RTOL, "%s stage %d dX" % (tag, si)
            assert np.array_equal(dev.down(d["X"]), dev.down(d["DXS"])), "%s stage %d: in = dx" % (tag, si)
        assert rel(dev.down(d["DF"]) - 0.25, t["DF"]) < RTOL, "%s stage %d dF" % (tag, si)
        assert rel(dev.down(d["DB"]) + 0.5, t["DB"]) < RTOL, "%s stage %d dB" % (tag, si)


def _has_sigmoid(stages):
    return any(a == "sigmoid" for st_ in stages for a in st_[2:])


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_sweep_forward(t4k, dev, oracle, row):
    N, rng, X, stages, flat, params, ref, end, arr, bufs = _setup(dev, oracle, row, 1000 + row)
    assert t4k.lib.t4k_conv_stack_ok(arr, len(stages), N) == 1
    t4k.call("t4k_rand_init", 1000 + row); t4k.call("t4k_rand_set_offset", 4096)
    dX, dX0 = dev.up(X), dev.zeros(X.shape)
    t4k.call("t4k_conv_stack_fwd", p(dX), p(dX0), arr, len(stages), N, None)
    assert np.array_equal(dev.down(dX0), X)
    assert t4k.lib.t4k_rand_offset() == end
    _check_fwd_vs_oracle(dev, stages, ref, bufs, "row %d" % row)
    witness_forward(X, stages, params, down_stage(dev, bufs, ref, FWD_KEYS), who="row %d stack" % row)
    witness_forward(X, stages, params, ref, who="row %d oracle" % row)


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_sweep_backward_whole_image(t4k, dev, oracle, row):
    """train | 2: the layer tensors (loaded with the oracle's forward state) are all the backward may read - the whole-image kernel"""
    N, rng, X, stages, flat, params, ref, end, arr, bufs = _setup(dev, oracle, row, 2000 + row)
    assert t4k.lib.t4k_conv_stack_ok(arr, len(stages), N) == 1
    for si in range(len(stages)):
        for k_, v in ref[si].items():
            if k_ in bufs[si]:
                bufs[si][k_].copy_(dev.torch.from_numpy(np.ascontiguousarray(v)))
        bufs[si]["DF"].fill_(0.25); bufs[si]["DB"].fill_(-0.5)
    bufs[0]["X"].copy_(dev.torch.from_numpy(X))
    DY = rng.standard_normal(ref[-1]["last"].shape).astype(np.float32)
    if _has_sigmoid(stages):                       # pass-through activation in the reference's backprop: the stack refuses the backward
        assert t4k.lib.t4k_conv_stack_bwd(p(dev.up(DY)), arr, len(stages), N, 3, None) != 0
        return
    assert t4k.lib.t4k_conv_stack_bwd_ok(arr, len(stages), N, 3, None) == int(ROWS[row][7])
    if not ROWS[row][7]:                           # too large for the whole-image kernel: refused, the host keeps its per-layer backward
        assert t4k.lib.t4k_conv_stack_bwd(p(dev.up(DY)), arr, len(stages), N, 3, None) == -4
        return
    want = _oracle_backward(oracle, ref, stages, flat, params, DY)
    t4k.call("t4k_conv_stack_bwd", p(dev.up(DY)), arr, len(stages), N, 3, None)
    _check_bwd_vs_oracle(dev, stages, want, bufs, "row %d whole-image" % row)
    witness_backward(stages, params, ref, down_stage(dev, bufs, ref, BWD_KEYS), DY, 0.25, -0.5, who="row %d whole-image" % row)
    witness_backward(stages, params, ref, oracle_bwd_as_got(want), DY, None, None, who="row %d oracle" % row)


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_sweep_forward_then_banded_backward(t4k, dev, oracle, row):
    """a stack forward, then the backward on what it saved (banded when the plan's bsplit > 1); on banded rows once more with train | 8
    (stage 0's dX skipped) followed by t4k_conv_stack_dx0, which must produce the same dX"""
    N, rng, X, stages, flat, params, ref, end, arr, bufs = _setup(dev, oracle, row, 3000 + row)
    ok, split, bsplit = plan(t4k, arr, len(stages), N)
    assert ok == 1
    DY = rng.standard_normal(ref[-1]["last"].shape).astype(np.float32)
    for lazy in ((False, True) if bsplit > 1 else (False,)):
        t4k.call("t4k_rand_init", 3000 + row); t4k.call("t4k_rand_set_offset", 4096)
        bufs[0]["X"].copy_(dev.torch.from_numpy(X))
        t4k.call("t4k_conv_stack_fwd", p(bufs[0]["X"]), None, arr, len(stages), N, None)
        got_fwd = down_stage(dev, bufs, ref, FWD_KEYS)
        x = X
        for si, st_ in enumerate(stages):
            got_fwd[si]["in"] = x
            x = got_fwd[si]["post_out" if st_[4] else ("pool_out" if st_[3] else ("pre_out" if st_[2] else "O"))]
            got_fwd[si]["last"] = x
        if _has_sigmoid(stages):
            assert t4k.lib.t4k_conv_stack_bwd(p(dev.up(DY)), arr, len(stages), N, 1, None) != 0
            return
        if bsplit == 1:                            # the backward after the forward is the whole-image kernel
            assert t4k.lib.t4k_conv_stack_bwd_ok(arr, len(stages), N, 1, None) == int(ROWS[row][7])
            if not ROWS[row][7]:
                assert t4k.lib.t4k_conv_stack_bwd(p(dev.up(DY)), arr, len(stages), N, 1, None) == -4
                return
        for si in range(len(stages)):
            bufs[si]["DF"].fill_(0.25); bufs[si]["DB"].fill_(-0.5)
        want = _oracle_backward(oracle, got_fwd, stages, flat, params, DY)
        tag = "row %d banded%s (split %d, bsplit %d)" % (row, " lazy dX0" if lazy else "", split, bsplit)
        t4k.call("t4k_conv_stack_bwd", p(dev.up(DY)), arr, len(stages), N, 9 if lazy else 1, None)
        if lazy:
            first_out = ctypes.c_void_p(arr[0].O)
            assert t4k.lib.t4k_conv_stack_dx0_pending(first_out) == 1, tag
            _check_bwd_vs_oracle(dev, stages, want, bufs, tag, skip_dx0=True)
            witness_backward(stages, params, got_fwd, down_stage(dev, bufs, ref, BWD_KEYS), DY, 0.25, -0.5, who=tag, skip_dx0=True)
            t4k.call("t4k_conv_stack_dx0", arr, N, None)
            assert t4k.lib.t4k_conv_stack_dx0_pending(first_out) == 0, tag
        _check_bwd_vs_oracle(dev, stages, want, bufs, tag)
        witness_backward(stages, params, got_fwd, down_stage(dev, bufs, ref, BWD_KEYS), DY, 0.25, -0.5, who=tag)
        witness_backward(stages, params, got_fwd, oracle_bwd_as_got(want), DY, None, None, who="row %d oracle" % row)


HEAD_ROWS = [r for r in range(len(ROWS)) if ROWS[r][6]]


@pytest.mark.parametrize("row", HEAD_ROWS)
def test_sweep_head_forward(t4k, dev, oracle, row):
    """t4k_conv_stack_head_fwd: the stack's tensors, Y1, the middle layer, Y2 and P against the oracle and float64"""
    N, rng, X, stages, flat, params, ref, end, arr, bufs = _setup(dev, oracle, row, 4000 + row)
    EA, EB, mid = ROWS[row][6]
    o = oracle.lib(); P = oracle.P; LAY = _lay(oracle)
    ref, _ = _oracle_forward(oracle, X, stages, flat, params, 4000 + row, 4096)       # (again: the head's draws continue this stream)
    xf = np.ascontiguousarray(ref[-1]["last"].reshape(N, -1)); E1 = xf.shape[1]
    W1 = (rng.standard_normal((EA, E1)) * 0.1).astype(np.float32); B1 = rng.standard_normal(EA).astype(np.float32)
    W2 = (rng.standard_normal((EB, EA)) * 0.3).astype(np.float32); B2 = rng.standard_normal(EB).astype(np.float32)
    Y1 = np.zeros((N, EA), np.float32); assert o.t4o_linear_fwd(P(xf), P(W1), P(B1), P(Y1), N, EA, E1) == 0
    cur = Y1; Fm = Am = None
    if mid:
        L, a = LAY[mid]; Fm = np.zeros(Y1.size, np.float32); Am = np.zeros_like(Y1)
        if mid == "dropout":
            o.t4o_rand(P(Fm), Fm.size, 0, 0.0, 1.0)
        o.t4o_activate(L, P(Y1), P(Am), P(Fm), a, Y1.size); Fm = Fm.reshape(Y1.shape); cur = Am
    Y2 = np.zeros((N, EB), np.float32); assert o.t4o_linear_fwd(P(np.ascontiguousarray(cur)), P(W2), P(B2), P(Y2), N, EB, EA) == 0
    Pr = np.zeros_like(Y2); o.t4o_softmax(P(Y2), P(Pr), N, EB)
    end = o.t4o_rand_offset()
    hd = StackHead()
    d = {"W1": dev.up(W1), "B1": dev.up(B1), "Y1": dev.zeros(Y1.shape), "Fm": dev.zeros(Y1.shape), "Am": dev.zeros(Y1.shape),
         "W2": dev.up(W2), "B2": dev.up(B2), "Y2": dev.zeros(Y2.shape), "P": dev.zeros(Y2.shape)}
    hd.W1, hd.B1, hd.Y1, hd.W2, hd.B2, hd.Y2, hd.P = p(d["W1"]), p(d["B1"]), p(d["Y1"]), p(d["W2"]), p(d["B2"]), p(d["Y2"]), p(d["P"])
    if mid:
        hd.mid_layer, hd.mid_alpha = LAY[mid]; hd.mid_mask, hd.mid_out = p(d["Fm"]), p(d["Am"])
    hd.E1, hd.E0a, hd.E0b = E1, EA, EB
    assert t4k.lib.t4k_conv_stack_head_ok(arr, len(stages), N, ctypes.byref(hd)) == 1
    t4k.call("t4k_rand_init", 4000 + row); t4k.call("t4k_rand_set_offset", 4096)
    t4k.call("t4k_conv_stack_head_fwd", p(dev.up(X)), None, arr, len(stages), N, ctypes.byref(hd), None)
    assert t4k.lib.t4k_rand_offset() == end
    _check_fwd_vs_oracle(dev, stages, ref, bufs, "row %d head" % row)
    assert rel(dev.down(d["Y1"]), Y1) < RTOL and rel(dev.down(d["Y2"]), Y2) < RTOL and rel(dev.down(d["P"]), Pr) < RTOL
    if mid == "dropout":
        assert np.array_equal(dev.down(d["Fm"]), Fm)
    witness_forward(X, stages, params, down_stage(dev, bufs, ref, FWD_KEYS), who="row %d head stack" % row)
    witness_head(xf, W1, B1, W2, B2, mid, Y1, Fm, Am, Y2, Pr, who="row %d oracle" % row)
    witness_head(dev.down(bufs[-1]["copy_out"]).reshape(N, -1), W1, B1, W2, B2, mid, dev.down(d["Y1"]), dev.down(d["Fm"]),
                 dev.down(d["Am"]), dev.down(d["Y2"]), dev.down(d["P"]), who="row %d head" % row)


def _branches(stages, Cin):
    """the kernel branches a row's stages take (mirrors of the constexpr conditions in conv_stack_kernels.hip.inc)"""
    out = set(); c1 = Cin
    for C0, K, *_ in stages:
        out.add("K%d" % K)
        nF = c1 * K * K * C0
        if c1 <= 4 and C0 <= 16:
            out.add("valu_fwd")
        if c1 <= 4 and nF <= 160:
            out.add("dx_valu")
        if C0 > 16:
            out.add("two_n_tiles")
        c1 = C0
    return out


def test_sweep_covers_every_plan_and_branch(t4k, dev):
    """over all rows: forward splits 1 - 4 and backward splits 1 - 4 each ran at least once, and so did the ROWT tiles (forward and
    dX windows of W < 16 <= W + K - 1), the VALU forward, dx_valu and two N tiles.  The splits come from t4k_conv_stack_plan, which
    reports what the launches above took."""
    splits, bsplits, branches, rowt = set(), set(), set(), set()
    for row, (spec, H, W, Cin, stages, flat, _h, _w) in enumerate(ROWS):
        N = n_of(spec)
        arr = (ConvStage * len(stages))()
        h, w, c1 = H, W, Cin
        keep = []
        for si, (C0, K, pre, pool, post) in enumerate(stages):
            s = arr[si]; s.H, s.W, s.C1, s.C0, s.K = h, w, c1, C0, K
            s.F = s.B = s.O = s.X = 1
            LAY = {"relu": 4, "tanh": 5, "sigmoid": 6, "selu": 7, "leaky": 8, "elu": 9, "dropout": 10, "avg": 13, "max": 14, "min": 15}
            b = s.run; b.KS = 2 if pool else 1
            if pre:
                b.pre_layer = LAY[pre]; b.pre_mask = b.pre_out = 1
            if pool:
                b.pool_layer = LAY[pool]; b.pool_out = 1
            if post:
                b.post_layer = LAY[post]; b.post_mask = b.post_out = 1
            if flat and si == len(stages) - 1:
                b.copy_out = 1
            if w < 16 <= w + K - 1:
                rowt.add((K, w))
            h, w, c1 = h // b.KS, w // b.KS, C0
        ok, sp, bs = plan(t4k, arr, len(stages), N)
        assert ok == 1, "row %d does not qualify" % row
        print("row %2d N %4d split %d bsplit %d" % (row, N, sp, bs))
        splits.add(sp); bsplits.add(bs); branches |= _branches(stages, Cin)
    assert splits == {1, 2, 3, 4}, splits
    assert bsplits == {1, 2, 3, 4}, bsplits
    assert {(5, 12), (5, 15), (3, 14)} <= rowt, rowt
    assert {"K3", "K5", "valu_fwd", "dx_valu", "two_n_tiles"} <= branches, branches


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_sweep_refuses_just_outside_the_limits(t4k, dev, case):
    N, H, W, C1, C0, K, pool = REFUSED[case]
    arr = (ConvStage * 1)()
    s = arr[0]; s.H, s.W, s.C1, s.C0, s.K = H, W, C1, C0, K
    s.F = s.B = s.O = s.X = 1                                                 # non-null placeholders: the check is on shapes
    s.run.KS = 2 if pool else 1
    if pool:
        s.run.pool_layer = 14; s.run.pool_out = 1
    assert t4k.lib.t4k_conv_stack_ok(arr, 1, N) == 0
    assert plan(t4k, arr, 1, N)[0] == 0


def test_sweep_worst_witness_ratio_per_tensor_kind():
    """runs last in this module: the worst |err| / bound per tensor kind over everything above (printed with -s; every one is <= 1 or an
    earlier check failed)"""
    for k_, (r, name) in sorted(wt.WORST.items()):
        print("%-16s %.3g  (%s)" % (k_, r, name))
        assert r <= 1.0
