"""The pool kernels (pool.hip: k_pool / k_dpool) and the fused element-wise runs (fused.hip: t4k_poolblock_fwd / _bwd, t4k_bn_poolblock_fwd)
at the launch plans their entries branch on, through the C ABI.  EVERY tensor a call writes is held element by element to the float64 witness
(tests/f64_witness.py) of its own op on the operands the kernel itself stored: relu / leaky / dropout masks and outputs, max / min pool, all
dpool routing, avg at KS = 2, the flatten copy and the stream offset exact; tanh / sigmoid / elu / selu, avg at KS = 3, the mask multiplies and
the batch-norm apply within c n 2^-24 mag.  Dropout draws are the oracle's Philox (pinned by test_philox_witness.py).

Plans (tests/small_kernel_cases.py, checked at 256 CUs by test_f64_witness.py and against the device's CU count here):
  wave64 / wg256       64-thread workgroups below 512 x CUs threads, 256 from there: N 8, grid 32 x 32, C 60 | 64 (VW 4), 30 | 34 (VW 2), 15 | 17 (VW 1)
  wg256_wrap           the grid capped at 8192 workgroups, a ragged second grid-stride trip: N 4, 64 x 64, C 129, KS 2; N 8, 64 x 64, C 65, no pool
  k_pool / k_dpool     past MAX_WG = 2048 workgroups with a clipped last window: 3 x 75 x 75 x 123 at KS 2, 3 x 113 x 113 x 123 at KS 3
  vw4 / vw2 / vw1      by C, and at C = 8 by every tensor sitting 4 or 8 bytes into its allocation (misaligned_<tensor>)

avg at KS = 2 "exact" means: bit-equal to the fp32 sum of the window in scan order, divided by 4 (the order k_pool defines; a sum of four
floats rounds, so no kernel equals the float64 mean) - and exact against float64 on integer operands.  leaky's output likewise: bit-equal to
the fp32 product alpha * x."""
import ctypes

import numpy as np
import pytest

import f64_witness as wt
import small_kernel_cases as sk
from test_gpu_parity import Dev, PoolBlock, p

pytestmark = pytest.mark.gpu

GUARD = np.float32(-777.25)
LEAD = 4                                        # guard words in front of and behind every tensor (16 bytes: the alignment class is the offset's)
ACT = {"relu": ("L_RELU", 0.0), "leaky": ("L_LEAKYRL", 0.1), "tanh": ("L_TANH", 0.0), "sigmoid": ("L_SIGMOID", 0.0), "elu": ("L_ELU", 1.0),
       "selu": ("L_SELU", 0.0), "dropout": ("L_DROPOUT", 0.5)}
POOL = {"max": "L_MAXPOOL", "min": "L_MINPOOL", "avg": "L_AVGPOOL", "usample": "L_USAMPLE"}
SEED, OFFSET = 77, 1 << 20


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


def launches(t4k):
    return int(t4k.lib.t4k_launch_count())


def cu_count(t4k):
    cu, khz, hbm = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_size_t(0)
    t4k.call("t4k_device_info", ctypes.byref(cu), ctypes.byref(khz), ctypes.byref(hbm))
    assert cu.value > 0
    return cu.value


class Buf:
    """a device tensor `off` bytes into a 16-byte aligned allocation, guard words on either side"""

    def __init__(self, dev, shape, off=0, data=None):
        self.shape, self.n, self.k = tuple(shape), int(np.prod(shape)), LEAD + off // 4
        a = np.full(self.k + self.n + LEAD, GUARD, np.float32)
        a[self.k:self.k + self.n] = np.nan if data is None else np.asarray(data, np.float32).ravel()      # NaN: an element left unwritten fails every witness
        self.t = dev.up(a); assert p(self.t) % 16 == 0
        self.ptr = p(self.t) + 4 * self.k

    def get(self, dev, name=""):
        a = dev.down(self.t)
        assert np.all(a[:self.k] == GUARD) and np.all(a[self.k + self.n:] == GUARD), "%s: guard word overwritten" % name
        return a[self.k:self.k + self.n].reshape(self.shape)


class Spec:
    def __init__(self, pre, pool, post, flat, KS, alpha_pre=None, alpha_post=None):
        self.pre, self.pool, self.post, self.flat, self.KS = pre, pool, post, flat, KS
        self.a_pre = ACT[pre][1] if pre and alpha_pre is None else alpha_pre
        self.a_post = (0.3 if post == "dropout" else ACT[post][1]) if post and alpha_post is None else alpha_post

    def names(self):
        return (["pre_mask", "pre_out"] if self.pre else []) + (["pool_out"] if self.pool else []) + \
               (["post_mask", "post_out"] if self.post else []) + (["copy_out"] if self.flat else [])

    def __repr__(self):
        return "%s-%s%d-%s%s" % (self.pre, self.pool, self.KS, self.post, "-flat" if self.flat else "")


def run_block(t4k, dev, oracle, spec, X, DY, H0, W0, offs=None, bn=None, backward=True):
    """forward (+ backward) of one run through the C ABI.  Returns {tensor: array after the forward}, {tensor: array after the backward},
    the stream offset behind the forward.  offs: {tensor name: byte offset of its base}; bn = (W, B, stat): the batch-norm form (X = Y)"""
    offs = offs or {}
    N, H1, W1, C = X.shape
    shp = {"pre_mask": X.shape, "pre_out": X.shape, "pool_out": (N, H0, W0, C), "post_mask": (N, H0, W0, C), "post_out": (N, H0, W0, C),
           "copy_out": (N, H0, W0, C), "XH": X.shape, "O": X.shape}
    b = {k: Buf(dev, shp[k], offs.get(k, 0)) for k in spec.names() + (["XH", "O"] if bn else [])}
    b["X"] = Buf(dev, X.shape, offs.get("X", 0), X)
    blk = PoolBlock(); blk.KS = spec.KS
    if spec.pre:
        blk.pre_layer, blk.pre_alpha = getattr(oracle, ACT[spec.pre][0]), spec.a_pre; blk.pre_mask, blk.pre_out = b["pre_mask"].ptr, b["pre_out"].ptr
    if spec.pool:
        blk.pool_layer = getattr(oracle, POOL[spec.pool]); blk.pool_out = b["pool_out"].ptr
    if spec.post:
        blk.post_layer, blk.post_alpha = getattr(oracle, ACT[spec.post][0]), spec.a_post; blk.post_mask, blk.post_out = b["post_mask"].ptr, b["post_out"].ptr
    if spec.flat:
        blk.copy_out = b["copy_out"].ptr
    t4k.call("t4k_rand_init", SEED); t4k.call("t4k_rand_set_offset", OFFSET)
    l0 = launches(t4k)
    if bn:
        Wg, Bb, stat = bn
        t4k.call("t4k_bn_poolblock_fwd", b["X"].ptr, b["O"].ptr, b["XH"].ptr, p(Wg), p(Bb), p(stat), ctypes.byref(blk), N, H1, W1, H0, W0, C, None)
    else:
        t4k.call("t4k_poolblock_fwd", b["X"].ptr, ctypes.byref(blk), N, H1, W1, H0, W0, C, None)
    rest = spec.KS > 1 and (H0 * spec.KS < H1 or W0 * spec.KS < W1)         # cells no window visits: the stages in front of the pool take a launch of their own there
    assert launches(t4k) - l0 == 1 + int(rest and bool(spec.pre or bn))     # one launch each way is the point of the run
    fwd = {k: v.get(dev, k) for k, v in b.items()}
    off_after = int(t4k.lib.t4k_rand_offset())
    bwd = None
    if backward and not bn:
        dDY = Buf(dev, DY.shape, offs.get("DY", 0), DY)
        l0 = launches(t4k)
        t4k.call("t4k_poolblock_bwd", dDY.ptr, b["X"].ptr, ctypes.byref(blk), N, H1, W1, H0, W0, C, None)
        assert launches(t4k) - l0 == 1 + int(rest and bool(spec.pre))
        bwd = {k: v.get(dev, k) for k, v in b.items()}
        assert np.array_equal(dDY.get(dev, "DY"), DY)
    return fwd, bwd, off_after


def draws(oracle, spec, n1, n0):
    """the uniform draws of the run's dropout stage from the oracle's stream, and the stream offset behind them"""
    o = oracle.lib(); o.t4o_rand_init(SEED); o.t4o_rand_set_offset(OFFSET)
    u1 = u0 = None
    if spec.pre == "dropout":
        u1 = np.zeros(n1, np.float32); o.t4o_dropout_mask(oracle.P(u1), n1)
    if spec.post == "dropout":
        u0 = np.zeros(n0, np.float32); o.t4o_dropout_mask(oracle.P(u0), n0)
    return u1, u0, int(o.t4o_rand_offset())


def avg_scan32(x, KS, H0, W0):
    """the fp32 sum of each window's existing cells in scan order, divided by KS^2 in fp32: the order k_pool defines"""
    t, m = wt._windows(np.asarray(x, np.float64), KS, H0, W0)
    t = (t * m).astype(np.float32); acc = np.zeros(t.shape[:-1], np.float32)
    for q in range(KS * KS):
        acc = acc + t[..., q]
    return acc / np.float32(KS * KS)


def check_act(tag, kind, alpha, x, u, out, mask):
    wo, wm = wt.act(kind, x, alpha, None if u is None else u.reshape(x.shape))
    wt.check("%s %s mask" % (tag, kind), mask, wm, kind="run: %s mask" % kind)
    wt.check("%s %s out" % (tag, kind), out, wo, kind="run: %s out" % kind)
    if kind == "leaky":
        wt.equal("%s leaky out (fp32 product)" % tag, out, np.where(x > 0, x, np.float32(alpha) * x), kind="run: exact tensors")


def check_forward(tag, oracle, spec, X, fwd, H0, W0, off_after):
    N, H1, W1, C = X.shape; n1, n0 = X.size, N * H0 * W0 * C
    u1, u0, off_want = draws(oracle, spec, n1, n0)
    x = X
    if spec.pre:
        check_act(tag + " pre", spec.pre, spec.a_pre, x, u1, fwd["pre_out"], fwd["pre_mask"]); x = fwd["pre_out"]
    if spec.pool:
        wt.check("%s pool %s" % (tag, spec.pool), fwd["pool_out"], wt.pool(spec.pool, x, spec.KS, H0, W0), kind="run: %s pool KS %d" % (spec.pool, spec.KS))
        if spec.pool == "avg" and spec.KS == 2:
            wt.equal("%s avg KS 2 (fp32 scan order)" % tag, fwd["pool_out"], avg_scan32(x, 2, H0, W0), kind="run: exact tensors")
        x = fwd["pool_out"]
    if spec.post:
        check_act(tag + " post", spec.post, spec.a_post, x, u0, fwd["post_out"], fwd["post_mask"]); x = fwd["post_out"]
    if spec.flat:
        wt.equal(tag + " flatten copy", fwd["copy_out"], x, kind="run: exact tensors")
    wt.equal(tag + " X after the forward", fwd["X"], X)
    assert off_after == off_want, "%s: stream offset %d, oracle %d" % (tag, off_after, off_want)


def check_backward(tag, spec, X, DY, fwd, bwd, H0, W0):
    """the in-place convention: each stage's INPUT buffer receives its dX; a buffer no stage writes keeps its forward values"""
    want = {}                                                                # buffer name -> witness
    last = "post_out" if spec.post else "pool_out" if spec.pool else "pre_out" if spec.pre else "X"
    g = DY
    if spec.flat:
        want[last] = wt.W(g, 0.0, 0)
    if spec.post:
        tgt = "pool_out" if spec.pool else "pre_out" if spec.pre else "X"
        want[tgt] = wt.mul(g, fwd["post_mask"]); g = bwd[tgt]
    if spec.pool:
        tgt = "pre_out" if spec.pre else "X"
        w = wt.dpool(spec.pool, g, fwd[tgt], spec.KS, H0, W0, keep=fwd[tgt])
        want[tgt] = w; g = bwd[tgt]
        if spec.pre:
            want["X"] = wt.mul(g, fwd["pre_mask"])           # over the WHOLE tensor, as the separate layer: where no window visits, g holds the pool input's forward values
    elif spec.pre:
        want["X"] = wt.mul(g.reshape(X.shape), fwd["pre_mask"])
    for k in ("X", "pre_out", "pool_out", "post_out"):
        if k in bwd:
            if k in want:
                exact = not np.any(want[k].n)
                wt.check("%s bwd %s" % (tag, k), bwd[k], want[k], kind="run: bwd routing / copies" if exact else "run: bwd mask multiply, avg spread")
            else:
                wt.equal("%s bwd %s (not written)" % (tag, k), bwd[k], fwd[k])
    for k in ("pre_mask", "post_mask", "copy_out"):
        if k in bwd:
            wt.equal("%s bwd %s (read only)" % (tag, k), bwd[k], fwd[k])
    return want


def both(t4k, dev, oracle, tag, spec, X, DY, H0, W0, offs=None):
    fwd, bwd, off = run_block(t4k, dev, oracle, spec, X, DY, H0, W0, offs)
    check_forward(tag, oracle, spec, X, fwd, H0, W0, off)
    check_backward(tag, spec, X, DY, fwd, bwd, H0, W0)
    return fwd, bwd, off


# ----------------------------------------------------------------------------- 1. every launch plan
def _variants(c):
    v = [("relu", "leaky")]
    if (c.plan, c.vw) in (("wg256", 2), ("wave64", 1)):
        v.append(("dropout", "leaky"))                                      # a dropout pre-stage on either side of the switch
    if c.plan == "wg256_wrap":
        v.append(("relu", "dropout"))                                       # dropout behind the pool: zo >> 2 far into the tensor
    return v


@pytest.mark.parametrize("case", sk.RUN_CASES, ids=[c.id for c in sk.RUN_CASES])
def test_runs_at_every_launch_plan(t4k, dev, oracle, case):
    c = case; cu = cu_count(t4k)
    assert sk.run_label(c.nthr, cu) == c.plan and sk.run_vw(c.C) == c.vw, \
        "%s: with %d CUs this case takes the plan %s %s - resize the table (tests/small_kernel_cases.py), it no longer reaches its label" % (c.id, cu, sk.run_label(c.nthr, cu), sk.run_plan(c.nthr, cu))
    rng = np.random.default_rng(100 + c.C)
    X = rng.standard_normal((c.N, c.H1, c.W1, c.C)).astype(np.float32)
    DY = rng.standard_normal((c.N, c.H0, c.W0, c.C)).astype(np.float32)
    for pre, post in _variants(c):
        spec = Spec(pre, c.pool, post, True, c.KS)
        both(t4k, dev, oracle, "%s %r" % (c.id, spec), spec, X, DY, c.H0, c.W0)
        del dev.keep[:]; dev.torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("C", [5, 6, 8])
@pytest.mark.parametrize("KS", [2, 3])
@pytest.mark.parametrize("kind", ["max", "min"])
@pytest.mark.parametrize("pre", [None, "relu"])
def test_runs_with_tied_windows(t4k, dev, oracle, pre, kind, KS, C):
    """operands in {-2 .. 2}: almost every window holds its extreme more than once and many are constant (behind a relu: all zero).  The first
    extreme in row-major scan order takes dy; values are compared, not the sign of a zero"""
    rng = np.random.default_rng(200 + KS * 10 + C)
    N, H0, W0 = 3, 5, 4
    X = rng.integers(-2, 3, (N, H0 * KS, W0 * KS, C)).astype(np.float32)
    X[0, :KS, :KS] = 1.0; X[1, :KS, :KS] = -1.0                             # constant windows: all ones, all zero behind a relu
    DY = sk.ints(rng, (N, H0, W0, C))                                       # never 0: a misrouted dy always shows
    t, _ = wt._windows(np.maximum(X, 0) if pre else X.astype(np.float64), KS, H0, W0)
    ext = t.max(-1, keepdims=True) if kind == "max" else t.min(-1, keepdims=True)
    assert ((t == ext).sum(-1) > 1).mean() > 0.3 and (np.ptp(t, -1) == 0).any()            # the case is what it claims: ties in a third of the windows or more
    spec = Spec(pre, kind, None, False, KS)
    fwd, bwd, _ = both(t4k, dev, oracle, "ties %r C=%d" % (spec, C), spec, X, DY, H0, W0)
    src = fwd["pre_out"] if pre else X
    wt.equal("ties dpool", bwd["pre_out" if pre else "X"], wt.dpool(kind, DY, src, KS).exact, kind="run: bwd routing / copies")
    # the plain kernels route the same way
    L = getattr(oracle, POOL[kind]); g = dev.up(src)
    t4k.call("t4k_dpool", L, p(g), p(dev.up(DY)), N, H0 * KS, W0 * KS, H0, W0, C, KS, None)
    wt.equal("ties k_dpool", dev.down(g), wt.dpool(kind, DY, src, KS).exact, kind="pool: k_dpool")


# ----------------------------------------------------------------------------- 3. misaligned bases
def _same(tag, a, b):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s: %s differs from the aligned run" % (tag, k)


@pytest.mark.parametrize("pre,post", [("relu", "leaky"), ("dropout", "leaky"), ("relu", "dropout")])
def test_runs_from_misaligned_bases(t4k, dev, oracle, pre, post):
    """C = 8: each tensor of the run in turn 4, then 8 bytes into its allocation (the run must drop to one / two channels per thread), every
    result bit-equal to the aligned run's - masks and stream offset included - and the guard words round every tensor untouched"""
    rng = np.random.default_rng(300)
    N, H0, W0, C, KS = 2, 3, 5, 8, 2
    X = rng.standard_normal((N, H0 * KS, W0 * KS, C)).astype(np.float32); DY = rng.standard_normal((N, H0, W0, C)).astype(np.float32)
    spec = Spec(pre, "max", post, True, KS)
    f0, b0, o0 = both(t4k, dev, oracle, "aligned %r" % spec, spec, X, DY, H0, W0)
    for label, tensor, off, vw in sk.RUN_MISALIGNED:
        if tensor in ("XH", "O"):
            continue                                                         # the BN form: test_bn_runs_from_misaligned_bases
        if "dropout" in (pre, post) and tensor not in ("X", "pre_mask", "post_mask", "DY"):
            continue                                                         # the dropout runs repeat the mask tensors, X and DY
        f, b, o = run_block(t4k, dev, oracle, spec, X, DY, H0, W0, {tensor: off})
        _same("%s +%d fwd" % (label, off), f0, f); _same("%s +%d bwd" % (label, off), b0, b)
        assert o == o0, (label, off)


def test_bn_runs_from_misaligned_bases(t4k, dev, oracle):
    rng = np.random.default_rng(301)
    N, H0, W0, C, KS = 2, 3, 5, 8, 2
    Y = rng.standard_normal((N, H0 * KS, W0 * KS, C)).astype(np.float32)
    Wg, Bb, stat, O, XH = _bn_stats(t4k, dev, rng, Y)
    spec = Spec("relu", "max", "dropout", False, KS)
    f0, _, o0 = run_block(t4k, dev, oracle, spec, Y, None, H0, W0, None, (Wg, Bb, stat))
    wt.equal("bn O aligned", f0["O"], O); wt.equal("bn XH aligned", f0["XH"], XH)
    for tensor in ("XH", "O", "X", "pre_out", "post_mask"):
        for off in (4, 8):
            f, _, o = run_block(t4k, dev, oracle, spec, Y, None, H0, W0, {tensor: off}, (Wg, Bb, stat))
            _same("bn misaligned_%s +%d" % (tensor, off), f0, f); assert o == o0


# ----------------------------------------------------------------------------- 4. every stage combination
COMBOS = [(pre, pool, post, flat) for pre in (None, "leaky", "dropout") for pool in (None, ("max", 2), ("avg", 3), ("min", 2))
          for post in (None, "tanh", "dropout") for flat in (False, True)
          if (pre or pool or post or flat) and not (pre == "dropout" and post == "dropout")]


@pytest.mark.parametrize("pre,pool,post,flat", COMBOS, ids=["%s-%s-%s-%s" % (a, b and b[0] + str(b[1]), c, "flat" if d else "noflat") for a, b, c, d in COMBOS])
def test_every_stage_combination(t4k, dev, oracle, pre, pool, post, flat):
    """N = 2, 6 x 6, C = 6.  The flatten-only block: `in = out`, so after the backward X holds DY (each layer's input buffer receives its dX)"""
    rng = np.random.default_rng(400)
    KS = pool[1] if pool else 1
    N, H1, C = 2, 6, 6; H0 = H1 // KS
    X = rng.standard_normal((N, H1, H1, C)).astype(np.float32); DY = rng.standard_normal((N, H0, H0, C)).astype(np.float32)
    spec = Spec(pre, pool[0] if pool else None, post, flat, KS)
    fwd, bwd, _ = both(t4k, dev, oracle, repr(spec), spec, X, DY, H0, H0)
    if flat and not (pre or pool or post):
        assert np.array_equal(bwd["X"], DY)


# ----------------------------------------------------------------------------- 5. clipped grids
@pytest.mark.parametrize("kind", ["max", "avg", "min"])
@pytest.mark.parametrize("KS", [2, 3])
@pytest.mark.parametrize("H1,W1", [(7, 5), (8, 7)])
def test_runs_on_clipped_grids(t4k, dev, oracle, H1, W1, KS, kind):
    """the ceil grid: edge windows run over the cells that exist, avg still divides by KS^2; fused run == t4k_pool + t4k_dpool bit for bit"""
    rng = np.random.default_rng(500 + H1 + KS)
    H0, W0 = sk.ceil_div(H1, KS), sk.ceil_div(W1, KS)
    for C in (5, 6, 8):
        _clipped(t4k, dev, oracle, rng, kind, KS, 2, H1, W1, H0, W0, C)


@pytest.mark.parametrize("kind", ["max", "avg", "min"])
def test_runs_on_a_floor_grid_leave_the_unvisited_cells(t4k, dev, oracle, kind):
    """7 x 7, KS = 2, H0 = 3: row 6 and column 6 belong to no window.  The pool input buffer keeps its forward values there, in the run and in
    k_dpool alike; the stages in front of the pool run over their whole tensors as the separate layers do (forward: relu of every element;
    backward: X = that buffer (*) mask everywhere)"""
    rng = np.random.default_rng(510)
    for C in (5, 8):
        _clipped(t4k, dev, oracle, rng, kind, 2, 2, 7, 7, 3, 3, C)


def _clipped(t4k, dev, oracle, rng, kind, KS, N, H1, W1, H0, W0, C):
    X = rng.standard_normal((N, H1, W1, C)).astype(np.float32); DY = rng.standard_normal((N, H0, W0, C)).astype(np.float32)
    spec = Spec("relu", kind, None, False, KS)
    tag = "clipped %dx%d->%dx%d KS %d %s C %d" % (H1, W1, H0, W0, KS, kind, C)
    fwd, bwd, _ = both(t4k, dev, oracle, tag, spec, X, DY, H0, W0)
    L = getattr(oracle, POOL[kind])
    src = dev.up(fwd["pre_out"]); q = dev.up(np.full((N, H0, W0, C), np.nan, np.float32))
    t4k.call("t4k_pool", L, p(src), p(q), N, H1, W1, H0, W0, C, KS, None)
    assert np.array_equal(dev.down(q), fwd["pool_out"]), tag + ": t4k_pool differs from the run"
    t4k.call("t4k_dpool", L, p(src), p(dev.up(DY)), N, H1, W1, H0, W0, C, KS, None)
    assert np.array_equal(dev.down(src), bwd["pre_out"]), tag + ": t4k_dpool differs from the run"
    w = wt.dpool(kind, DY, fwd["pre_out"], KS, H0, W0, keep=fwd["pre_out"])
    if H0 * KS < H1:
        assert not w.written[:, H0 * KS:].any() and not w.written[:, :, W0 * KS:].any()
        assert np.array_equal(bwd["pre_out"][:, H0 * KS:], np.maximum(X, 0)[:, H0 * KS:]) and np.array_equal(bwd["pre_out"][:, :, W0 * KS:], np.maximum(X, 0)[:, :, W0 * KS:])
        assert np.array_equal(bwd["X"][:, H0 * KS:], np.maximum(X, 0)[:, H0 * KS:]) and np.array_equal(bwd["X"][:, :, W0 * KS:], np.maximum(X, 0)[:, :, W0 * KS:])   # relu(x) * (x > 0)


# ----------------------------------------------------------------------------- 6. plain pools past the grid cap
@pytest.mark.parametrize("kind", ["max", "min", "avg", "usample"])
@pytest.mark.parametrize("N,H1,W1,C,KS", sk.POOL_WRAP_CASES)
def test_plain_pool_past_the_grid_cap(t4k, dev, oracle, N, H1, W1, C, KS, kind):
    """k_pool / k_dpool in their second grid-stride trip, the last window of every row and column clipped; operands in +-{0, 36, 72} so that
    every window sum and its division by KS^2 (4 or 9) is exact: bit-equal"""
    H0, W0 = sk.ceil_div(H1, KS), sk.ceil_div(W1, KS); n = N * H0 * W0 * C
    grid, trips, tail = sk.pool_plan(n)
    assert grid == sk.MAX_WG and trips == 2 and tail > 0
    rng = np.random.default_rng(600 + KS)
    X = (rng.integers(-2, 3, (N, H1, W1, C)) * 36).astype(np.float32)
    DY = (sk.ints(rng, (N, H0, W0, C)) * 36).astype(np.float32)
    L = getattr(oracle, POOL[kind])
    dX = dev.up(X); q = dev.up(np.full((N, H0, W0, C), np.nan, np.float32))
    l0 = launches(t4k)
    t4k.call("t4k_pool", L, p(dX), p(q), N, H1, W1, H0, W0, C, KS, None)
    t4k.call("t4k_dpool", L, p(dX), p(dev.up(DY)), N, H1, W1, H0, W0, C, KS, None)
    assert launches(t4k) - l0 == 2
    wp = wt.pool(kind, X, KS, H0, W0)
    wt.equal("k_pool %s KS %d" % (kind, KS), dev.down(q), wp.exact, kind="pool: k_pool")
    wt.equal("k_dpool %s KS %d" % (kind, KS), dev.down(dX), wt.dpool(kind, DY, X, KS, H0, W0, keep=X).exact, kind="pool: k_dpool")
    del dev.keep[:]; dev.torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 7. the batch-norm apply with a run behind it
def _bn_stats(t4k, dev, rng, Y):
    """gamma, beta, stat_dev as t4k_batchnorm_fwd leaves them, and the O / XH it wrote"""
    N, H1, W1, C = Y.shape
    Wg = dev.up((rng.standard_normal(C) * 0.5 + 1.0).astype(np.float32)); Bb = dev.up(rng.standard_normal(C).astype(np.float32))
    stat = dev.zeros(3 * C); O = dev.zeros(Y.shape); XH = dev.zeros(Y.shape)
    t4k.call("t4k_batchnorm_fwd", p(dev.up(Y)), p(O), p(XH), p(Wg), p(Bb), p(stat), N, H1 * W1, C, None)
    return Wg, Bb, stat, dev.down(O), dev.down(XH)


@pytest.mark.parametrize("N,H0,W0,C,plan", [(2, 3, 4, 5, "wave64"), (2, 3, 4, 6, "wave64"), (3, 4, 4, 64, "wave64"), (8, 32, 32, 64, "wg256")])
def test_bn_apply_with_a_run_behind_it(t4k, dev, oracle, N, H0, W0, C, plan):
    """t4k_bn_poolblock_fwd called directly on statistics t4k_batchnorm_fwd left: XH and O held to the float64 witness AND bit-equal to what
    t4k_batchnorm_fwd wrote (the header's "exactly as"); the run relu -> max 2 -> dropout (the CIFAR group) witnessed on the stored O"""
    KS = 2; vw = sk.run_vw(C); nthr = N * H0 * W0 * C // vw
    assert sk.run_label(nthr, cu_count(t4k)) == plan, "with %d CUs this case takes %s" % (cu_count(t4k), sk.run_label(nthr, cu_count(t4k)))
    rng = np.random.default_rng(700 + C)
    Y = (rng.standard_normal((N, H0 * KS, W0 * KS, C)) * 1.5 + 0.5).astype(np.float32)
    Wg, Bb, stat, O, XH = _bn_stats(t4k, dev, rng, Y)
    spec = Spec("relu", "max", "dropout", False, KS)
    fwd, _, off = run_block(t4k, dev, oracle, spec, Y, None, H0, W0, None, (Wg, Bb, stat))
    st = dev.down(stat)
    wt.check("bn run xhat C=%d" % C, fwd["XH"].reshape(-1, C), wt.bn_xhat(Y, st), kind="run: bn xhat")
    wt.check("bn run y C=%d" % C, fwd["O"].reshape(-1, C), wt.bn_y(fwd["XH"], dev.down(Wg), dev.down(Bb)), kind="run: bn y")
    wt.equal("bn run XH == t4k_batchnorm_fwd's", fwd["XH"], XH); wt.equal("bn run O == t4k_batchnorm_fwd's", fwd["O"], O)
    f2 = dict(fwd); f2["X"] = fwd["O"]                                       # the run's input is the stored O
    check_forward("bn run C=%d" % C, oracle, spec, fwd["O"], f2, H0, W0, off)
    wt.equal("bn run input untouched", fwd["X"], Y)
    del dev.keep[:]; dev.torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- 8. rejected blocks
def test_rejected_blocks_write_nothing(t4k, dev, oracle):
    """the documented status, t4k_last_error() set, no launch, every destination and X untouched - forward, batch-norm form and backward"""
    rng = np.random.default_rng(800)
    N, H1, C = 2, 6, 8; H0 = 3
    X = rng.standard_normal((N, H1, H1, C)).astype(np.float32); DY = rng.standard_normal((N, H0, H0, C)).astype(np.float32)
    SENT = np.float32(12345.5)
    big = {k: dev.up(np.full(X.shape, SENT)) for k in ("pre_mask", "pre_out", "pool_out", "post_mask", "post_out", "copy_out", "O", "XH")}
    dX = dev.up(X); dDY = dev.up(DY); Wg = dev.up(np.ones(C, np.float32)); stat = dev.up(np.ones(3 * C, np.float32))
    DROP, RELU, MAXP = oracle.L_DROPOUT, oracle.L_RELU, oracle.L_MAXPOOL
    UNSUP, ARG = -4, -1

    def blk(pre=0, pool=0, KS=1, post=0, tensors=("pre", "pool", "post")):
        b = PoolBlock(); b.pre_layer, b.pool_layer, b.post_layer, b.KS = pre, pool, post, KS; b.pre_alpha = b.post_alpha = 0.5
        if "pre" in tensors: b.pre_mask, b.pre_out = p(big["pre_mask"]), p(big["pre_out"])
        if "pool" in tensors: b.pool_out = p(big["pool_out"])
        if "post" in tensors: b.post_mask, b.post_out = p(big["post_mask"]), p(big["post_out"])
        b.copy_out = p(big["copy_out"])
        return b
    cases = [("two dropouts", blk(DROP, MAXP, 2, DROP), UNSUP, "post layer"),
             ("KS = 4", blk(RELU, MAXP, 4, RELU), UNSUP, "kernel_size=4"),
             ("KS = 2 without a pool layer", blk(RELU, 0, 2, RELU), UNSUP, "kernel_size=2"),
             ("KS = 1 with a pool layer", blk(RELU, MAXP, 1, RELU), UNSUP, "kernel_size=1"),
             ("pre tensors missing", blk(RELU, MAXP, 2, RELU, ("pool", "post")), ARG, "pre tensors missing"),
             ("post tensors missing", blk(RELU, MAXP, 2, RELU, ("pre", "pool")), ARG, "post tensors missing"),
             ("pool output missing", blk(RELU, MAXP, 2, RELU, ("pre", "post")), ARG, "pool output missing"),
             ("null block", None, ARG, "null block")]
    t4k.call("t4k_rand_init", SEED); t4k.call("t4k_rand_set_offset", OFFSET)
    l0 = launches(t4k)
    for name, b, status, text in cases:
        ref = ctypes.byref(b) if b is not None else None
        calls = (("t4k_poolblock_fwd", lambda: t4k.lib.t4k_poolblock_fwd(p(dX), ref, N, H1, H1, H0, H0, C, None)),
                 ("t4k_bn_poolblock_fwd", lambda: t4k.lib.t4k_bn_poolblock_fwd(p(dX), p(big["O"]), p(big["XH"]), p(Wg), p(Wg), p(stat), ref, N, H1, H1, H0, H0, C, None)),
                 ("t4k_poolblock_bwd", lambda: t4k.lib.t4k_poolblock_bwd(p(dDY), p(dX), ref, N, H1, H1, H0, H0, C, None)))
        for fn, call in calls:
            rc = call(); err = t4k.lib.t4k_last_error().decode()
            assert rc == status, "%s %s: status %d, documented %d (%s)" % (fn, name, rc, status, err)
            assert text in err and "t4k_poolblock" in err, "%s %s: t4k_last_error() = %r" % (fn, name, err)
    assert launches(t4k) == l0
    assert int(t4k.lib.t4k_rand_offset()) == OFFSET                         # a rejected dropout run draws nothing
    for k, t in big.items():
        assert np.all(dev.down(t) == SENT), k
    assert np.array_equal(dev.down(dX), X) and np.array_equal(dev.down(dDY), DY)
    # null tensors behind a valid block
    b = blk(RELU, MAXP, 2, RELU)
    assert t4k.lib.t4k_poolblock_fwd(None, ctypes.byref(b), N, H1, H1, H0, H0, C, None) == ARG and "null input" in t4k.lib.t4k_last_error().decode()
    assert t4k.lib.t4k_poolblock_bwd(None, p(dX), ctypes.byref(b), N, H1, H1, H0, H0, C, None) == ARG and "null tensor" in t4k.lib.t4k_last_error().decode()
    assert t4k.lib.t4k_bn_poolblock_fwd(p(dX), None, p(big["XH"]), p(Wg), p(Wg), p(stat), ctypes.byref(b), N, H1, H1, H0, H0, C, None) == ARG
    assert launches(t4k) == l0 and np.all(dev.down(big["pre_out"]) == SENT)


def test_zz_report_worst_ratios():
    """the worst |error| / bound per tensor kind over everything above (pytest -s prints it; tests/README.md quotes it)"""
    print("\npool / fused-run sweep, worst |err| / bound per tensor kind:")
    for kind in sorted(k for k in wt.WORST if k.startswith(("run:", "pool:"))):
        print("  %-40s %.3g   %s" % (kind, wt.WORST[kind][0], wt.WORST[kind][1]))
        assert wt.WORST[kind][0] <= 1.0
