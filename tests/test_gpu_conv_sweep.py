"""The conv entries at every rung of their dispatch (conv.hip, conv_few.hip, conv_img.hip, conv_big.hip, colsum.hip, dconv.hip), with the rung asserted.

Every row of tests/conv_cases.py names the plan it is meant to reach.  The plan is recomputed from the device's CU count with the Python mirror
of the dispatch and the row FAILS when it no longer reaches its label; t4k_conv_last_plan() must report the mirror's string and t4k_launch_count()
the mirror's launch count, for every call form a row runs.  Every tensor sits inside a larger allocation with 256 NaN floats in front and behind
(a skewed one: 1 or 2 floats more in front): inputs and moats must be bit-identical after the call, outputs are prefilled with NaN and may hold
none afterwards - an element skipped, or one from outside an operand that reaches a sum, shows as one.
  exact   operands, DF0 and DB0 in {-2 .. 2}, every partial sum below 2^24 (conv_cases.exact_ok, asserted per row): every written tensor
          bit-equal to the float64 result, the layer-0 copy, the block's tensors and the batch-norm mean included;
  float   standard-normal operands: forward, dX, dF and dB element by element inside f64_witness.conv_fwd / conv_dx / conv_df / conv_db's bound as
          it stands, each witnessed on the operands the call itself stored.
Backward rows run five call forms: (DX, DF, DB), the same with a second dX copy, the fold alone (DX == NULL), dX alone (DF == DB == NULL), and
DX2 == I as the host model calls it (dX overwrites the layer input in the launch behind the dF stage; the reference is computed from the uploaded I)."""
import ctypes
import time

import numpy as np
import pytest

import conv_cases as cc
import f64_witness as wt
from test_gpu_conv_rungs import BLOCK as RUNG_BLOCK, BWD as RUNG_BWD, FWD as RUNG_FWD, PoolBlock
from test_gpu_gemm_sweep import Buf, call, cu_count, free, launches
from test_gpu_parity import Dev

pytestmark = pytest.mark.gpu

UNSUPPORTED = -4                                           # T4K_ERR_UNSUPPORTED (include/t4k.h)
CLOCK = {}
ACT = {0: None, cc.L_RELU: ("relu", 0.0), cc.L_LEAKY: ("leaky", 0.1), cc.L_TANH: ("tanh", 0.0), cc.L_DROPOUT: ("dropout", 0.5)}
POOL = {cc.L_MAXPOOL: "max", cc.L_MINPOOL: "min", cc.L_AVGPOOL: "avg"}
SEED, OFFSET = 77, 1 << 20


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    t4k.lib.t4k_conv_last_plan.restype = ctypes.c_char_p
    CLOCK["t0"] = time.time()
    return Dev(t4k)


def last_plan(t4k):
    return t4k.lib.t4k_conv_last_plan().decode()


def nans(*shape):
    return np.full(shape, np.nan, np.float32)


def planned(t4k, name, want, fn):
    """run one entry: the hook's string and the launch count against the mirror's"""
    l0 = launches(t4k)
    fn()
    n, plan = launches(t4k) - l0, last_plan(t4k)
    assert plan == want[0], "%s: t4k_conv_last_plan() says '%s', the mirror '%s'" % (name, plan, want[0])
    assert n == want[1], "%s: %d launches, the plan '%s' makes %d" % (name, n, plan, want[1])
    return plan


def on_label(r, cu):
    want = r.plan(cu)
    assert want[0] == r.label, "%s: with %d CUs this row takes the plan '%s', not '%s' - resize the table (tests/conv_cases.py)" % (r.id, cu, want[0], r.label)
    return want


# ----------------------------------------------------------------------------- one row
def run_forward(t4k, dev, r, exact, skew=None, stream=None, tag="", check_plan=True):
    """fwd / bn / block / dconv_fwd rows; returns {name: array} of what the call wrote"""
    cu = cu_count(t4k)
    sk = dict(r.skew, **(skew or {}))
    o = cc.operands(r, exact)
    w = cc.witnesses(r, o)["O"]
    H0, W0 = r.out_hw()
    N, C0 = r.N, r.C0
    name = "%s%s %s" % (tag, r.id, "exact" if exact else "float")
    b = {k: Buf(dev, o[k], sk.get(k, 0)) for k in ("I", "F", "B")}
    b["O"] = Buf(dev, nans(N, H0, W0, C0), sk.get("O", 0))
    if r.icopy:
        b["ICOPY"] = Buf(dev, nans(*o["I"].shape), sk.get("ICOPY", 0))
    pc = b["ICOPY"].ptr if r.icopy else None
    K, S, P = cc.GEO[r.K]
    geo = (N, r.H1, r.W1, r.C1, H0, W0, C0, K, S, P)
    want = r.plan(cu, skew=sk)
    if r.entry == "fwd":
        fn = lambda: call(t4k, "t4k_conv2d_fwd2", b["I"].ptr, pc, b["O"].ptr, b["F"].ptr, b["B"].ptr, *geo, stream)
    elif r.entry == "dconv_fwd":
        fn = lambda: call(t4k, "t4k_dconv2d_fwd", b["I"].ptr, b["O"].ptr, b["F"].ptr, b["B"].ptr, *geo, stream)
    elif r.entry == "bn":
        for k in ("G", "BB"):
            b[k] = Buf(dev, o[k])
        b["Y"], b["XH"], b["ST"] = Buf(dev, nans(N, H0, W0, C0)), Buf(dev, nans(N, H0, W0, C0)), Buf(dev, nans(3 * C0))
        fn = lambda: call(t4k, "t4k_conv2d_bn_fwd", b["I"].ptr, pc, b["O"].ptr, b["F"].ptr, b["B"].ptr, *geo, b["Y"].ptr, b["XH"].ptr, b["G"].ptr, b["BB"].ptr, b["ST"].ptr, stream)
    else:
        q = (N, H0 // 2, W0 // 2, C0)
        blk = PoolBlock(); blk.KS = r.blk["KS"]
        if r.blk["pre"]:
            b["PRE"], b["PREM"] = Buf(dev, nans(N, H0, W0, C0), sk.get("PRE", 0)), Buf(dev, nans(N, H0, W0, C0), sk.get("PREM", 0))
            blk.pre_layer, blk.pre_alpha, blk.pre_out, blk.pre_mask = r.blk["pre"], ACT[r.blk["pre"]][1], b["PRE"].ptr, b["PREM"].ptr
        b["POOL"] = Buf(dev, nans(*q), sk.get("POOL", 0))
        blk.pool_layer, blk.pool_out = r.blk["pool"], b["POOL"].ptr
        if r.blk["post"]:
            b["POST"], b["POSTM"] = Buf(dev, nans(*q), sk.get("POST", 0)), Buf(dev, nans(*q), sk.get("POSTM", 0))
            blk.post_layer, blk.post_alpha, blk.post_out, blk.post_mask = r.blk["post"], ACT[r.blk["post"]][1], b["POST"].ptr, b["POSTM"].ptr
        if r.blk["copy"]:
            b["COPY"] = Buf(dev, nans(*q), sk.get("COPY", 0)); blk.copy_out = b["COPY"].ptr
        if r.blk["pre"] == cc.L_DROPOUT:
            call(t4k, "t4k_rand_init", SEED); call(t4k, "t4k_rand_set_offset", OFFSET)
        fn = lambda: call(t4k, "t4k_conv2d_block_fwd", b["I"].ptr, pc, b["O"].ptr, b["F"].ptr, b["B"].ptr, ctypes.byref(blk), *geo, stream)
    dev.torch.cuda.synchronize()
    if check_plan:
        plan = planned(t4k, name, want, fn)
    else:
        fn(); plan = last_plan(t4k)
    got = {"O": b["O"].get(name + " O", (N, H0, W0, C0), stream)}
    for k in ("I", "F", "B", "G", "BB"):
        if k in b:
            b[k].untouched(name + " " + k)
    if r.icopy:
        got["ICOPY"] = b["ICOPY"].get(name + " ICOPY", o["I"].shape)
    cc.hold_all(name, got, {"O": w}, o, exact, plan)
    if r.entry == "bn":
        for k in ("Y", "XH", "ST"):
            got[k] = b[k].get(name + " " + k, (-1, C0) if k != "ST" else (3 * C0,))
        cc.hold_bn(name, got, o, exact, plan)
    if r.entry == "block":
        for k in ("PRE", "PREM", "POOL", "POST", "POSTM", "COPY"):
            if k in b:
                got[k] = b[k].get(name + " " + k, (N, H0, W0, C0) if k in ("PRE", "PREM") else (N, H0 // 2, W0 // 2, C0))
        check_block_tensors(name, r.blk, got, exact, plan)
    return got


def check_block_tensors(name, blk, got, exact, plan, u=None):
    """every tensor of the run against the witness of its own op, on the tensor in front of it as stored; masks bit-equal"""
    x = got["O"]
    if blk["pre"]:
        kind, alpha = ACT[blk["pre"]]
        if kind == "dropout" and u is None:                # the draws are held to the oracle's by test_block_with_dropout_in_front: here the mask as stored
            assert np.isin(got["PREM"], (0.0, 1.0)).all()
            wo, wm = wt.act_from(kind, x, alpha, got["PREM"]), wt.W(got["PREM"], 0.0, 0)
        else:
            wo, wm = wt.act(kind, x, alpha, None if u is None else u.reshape(x.shape))
        if kind != "tanh":
            wt.equal(name + " pre mask", got["PREM"], wm.exact, kind="conv exact: block masks")
        wt.check(name + " pre mask", got["PREM"], wm, kind="conv: block %s mask" % kind)
        wt.check(name + " pre out", got["PRE"], wo, kind="conv: block %s out" % kind)
        x = got["PRE"]
    wt.check(name + " pool", got["POOL"], wt.pool(POOL[blk["pool"]], x, 2), kind="conv: block pool %s" % POOL[blk["pool"]])
    x = got["POOL"]
    if blk["post"]:
        kind, alpha = ACT[blk["post"]]
        wo, wm = wt.act(kind, x, alpha)
        if kind != "tanh":
            wt.equal(name + " post mask", got["POSTM"], wm.exact, kind="conv exact: block masks")
        wt.check(name + " post mask", got["POSTM"], wm, kind="conv: block %s mask" % kind)
        wt.check(name + " post out", got["POST"], wo, kind="conv: block %s out" % kind)
        x = got["POST"]
    if blk["copy"]:
        wt.equal(name + " flatten copy", got["COPY"], x, kind="conv exact: block copy")


FORMS = ("dx+df", "dx+dx2+df", "df", "dx+dx2", "dx2=I")


def run_backward(t4k, dev, r, exact, skew=None, stream=None, tag="", forms=FORMS, check_plan=True):
    """bwd / dconv_bwd rows, the call forms in turn on one set of inputs; returns the last form's tensors"""
    cu = cu_count(t4k)
    sk = dict(r.skew, **(skew or {}))
    o = cc.operands(r, exact)
    w = cc.witnesses(r, o)
    H0, W0 = r.out_hw()
    K, S, P = cc.GEO[r.K]
    geo = (r.N, r.H1, r.W1, r.C1, H0, W0, r.C0, K, S, P)
    b = {k: Buf(dev, o[k], sk.get(k, 0)) for k in ("I", "DO", "F")}
    b["DX"], b["DX2"] = Buf(dev, nans(*o["I"].shape), sk.get("DX", 0)), Buf(dev, nans(*o["I"].shape), sk.get("DX2", 0))
    b["DF"], b["DB"] = Buf(dev, o["DF0"], sk.get("DF", 0)), Buf(dev, o["DB0"], sk.get("DB", 0))
    got = {}
    if r.entry == "dconv_bwd":
        forms = [f for f in forms if "dx2" not in f] if r.dx else ["df"]
    for form in forms:
        name = "%s%s %s [%s]" % (tag, r.id, "exact" if exact else "float", form)
        dx, dx2, df, inplace = "dx" in form.split("+") or form == "dx2=I", "dx2" in form, "df" in form or form == "dx2=I", form == "dx2=I"
        if form == "dx2=I":
            dx2 = True
        b["DX"].put(nans(*o["I"].shape)); b["DX2"].put(nans(*o["I"].shape)); b["DF"].put(o["DF0"]); b["DB"].put(o["DB0"])
        if inplace:
            b["I"].put(o["I"])
        dev.torch.cuda.synchronize()
        pdx, pdx2 = (b["DX"].ptr if dx else None), ((b["I"].ptr if inplace else b["DX2"].ptr) if dx2 else None)
        pdf, pdb = (b["DF"].ptr, b["DB"].ptr) if df else (None, None)
        if r.entry == "bwd":
            fn = lambda: call(t4k, "t4k_conv2d_bwd2", b["I"].ptr, b["DO"].ptr, pdx, pdx2, b["F"].ptr, pdf, pdb, *geo, 1, stream)
        else:
            fn = lambda: call(t4k, "t4k_dconv2d_bwd", b["I"].ptr, b["DO"].ptr, pdx, b["F"].ptr, pdf, pdb, *geo, 1, stream)
        want = r.plan(cu, dx=dx, df=df, skew=sk)
        if check_plan:
            plan = planned(t4k, name, want, fn)
        else:
            fn(); plan = last_plan(t4k)
        got = {}
        if dx:
            got["DX"] = b["DX"].get(name + " DX", o["I"].shape, stream)
            if dx2:
                got["DX2"] = (b["I"] if inplace else b["DX2"]).get(name + " DX2", o["I"].shape, stream)
        if df:
            got["DF"], got["DB"] = b["DF"].get(name + " DF", o["DF0"].shape, stream), b["DB"].get(name + " DB", o["DB0"].shape, stream)
        cc.hold_all(name, got, w, o, exact, plan)
        if inplace:
            b["I"].put(o["I"])
        else:
            b["I"].untouched(name + " I")
        b["DO"].untouched(name + " DO"); b["F"].untouched(name + " F")
    return got


def run_row(t4k, dev, r, exact, **kw):
    assert cc.exact_ok(r), r.id
    return (run_backward if r.entry in ("bwd", "dconv_bwd") else run_forward)(t4k, dev, r, exact, **kw)


# ----------------------------------------------------------------------------- 1. every rung
@pytest.mark.parametrize("row", cc.ROWS, ids=[r.id for r in cc.ROWS])
def test_every_rung_exact_and_float(t4k, dev, row):
    on_label(row, cu_count(t4k))
    run_row(t4k, dev, row, True)
    free(dev)
    run_row(t4k, dev, row, False)
    free(dev)


# ----------------------------------------------------------------------------- 2. the engines that share the stream's workspace
B2B = ("dfw_48_slices__df_fold", "df8_tp2__dx_convbig8", "thin_df__dx_wide_c64", "df_mfma_slices__dx_and_fold", "dx_fewch", "bn_thin_rider", "bn_big8_rider")


def test_engines_back_to_back(t4k, dev):
    """one exact row of each family that uses the workspace halves - dfw + df_fold + colsum, df8 + fold_add, thin_df riding dx_wide, df_mfma riding
    dx_and_fold, the fold alone + fewch, the thin and the big8 batch-norm riders - on one stream, in an order in which every one follows every
    other (a closed walk over all ordered pairs); every output checked"""
    reps = [cc.BY_ID[i] for i in B2B]
    walk = cc.euler_walk(len(reps))
    steps = set(zip(walk, walk[1:]))
    assert all((a, c) in steps for a in range(len(reps)) for c in range(len(reps)) if a != c)
    for n, i in enumerate(walk):
        run_row(t4k, dev, reps[i], True, **({"forms": ("dx+df",)} if reps[i].entry == "bwd" else {}))
        if n % 8 == 7:
            free(dev)
    free(dev)
    assert t4k.lib.t4k_sync(None) == 0


# ----------------------------------------------------------------------------- 3. outputs off their 16-byte boundary
def _one_row_per_label():
    seen, out = set(), []
    for r in cc.ROWS:
        if r.label not in seen and r.pixels() <= 4096 and not r.skew:
            seen.add(r.label); out.append(r)
    return out


@pytest.mark.parametrize("row", _one_row_per_label(), ids=[r.id for r in _one_row_per_label()])
def test_outputs_from_skewed_bases(t4k, dev, row):
    """O / ICOPY / DX / DX2 / DF / DB and the block's tensors 4, then 8 bytes into their allocations.  The mirror says which kernel the dispatch then
    picks (thin and img_block look at their outputs); whatever runs must be right, the exact pass bit-equal and every moat intact.  The rows of
    the table with a skewed INPUT (I, F, DO 4 bytes off) are asserted on their other kernel by test_every_rung_exact_and_float."""
    cu = cu_count(t4k)
    for off in (1, 2):
        sk = {k: off for k in ("O", "ICOPY", "DX", "DX2", "DF", "DB", "PRE", "PREM", "POOL", "POST", "POSTM", "COPY")}
        run_row(t4k, dev, row, True, skew=sk, tag="outputs + %d bytes " % (4 * off))
    if row.label.startswith("thin") and row.entry == "fwd":
        assert row.plan(cu, skew={"O": 1})[0].startswith("gather") or "gather" in row.plan(cu, skew={"O": 1})[0]
    if row.label == "img_block" and row.C0 % 2 == 0:
        for t in ("POOL", "POST", "POSTM", "COPY"):
            if t in ("POOL", "COPY") or row.blk["post"]:
                assert row.plan(cu, skew={t: 1})[0].startswith("gather_pool"), t
                run_row(t4k, dev, row, True, skew={t: 1}, tag="%s + 4 bytes " % t)
    free(dev)


def test_skewed_inputs_move_the_rows_the_mirror_says(t4k):
    """every row of the table with a skewed input takes another plan than the same shape aligned"""
    cu = cu_count(t4k)
    moved = [r for r in cc.ROWS if any(k in r.skew for k in ("I", "F", "DO"))]
    assert len(moved) >= 7
    for r in moved:
        if r.id != "gather_raw_skewed_f":                  # the raw path's copy loop changes inside the kernel, not the plan
            assert r.plan(cu)[0] != r.plan(cu, skew={})[0], r.id


# ----------------------------------------------------------------------------- 4. the block entry
def _blocks():
    out = []
    for c1, c0, tag in ((1, 8, "img_block"), (3, 6, "img_block"), (2, 8, "gather_pool"), (2, 5, "gather_pool")):
        for pre in (0, cc.L_RELU, cc.L_LEAKY, cc.L_TANH):
            for pool in (cc.L_MAXPOOL, cc.L_MINPOOL, cc.L_AVGPOOL):
                post = (0, cc.L_RELU, cc.L_LEAKY, cc.L_TANH)[(pre // 4 + pool) % 4]
                for copy in (False, True):
                    lab = "img_block" if tag == "img_block" else "gather_pool<raw,ks%d>" % (1 if c1 * 9 < 36 and (c1 + 1) // 2 * 9 < 18 else 2)
                    out.append(cc.Row("%s_%dto%d_%s_%s_%s%s" % (tag, c1, c0, ACT[pre][0] if pre else "none", POOL[pool], ACT[post][0] if post else "none", "_copy" if copy else ""),
                                      "block", 2, 6, 10, c1, c0, 3, lab, "stage combination", icopy=copy, blk=cc.blk(pre=pre, pool=pool, post=post, copy=copy)))
    return out


@pytest.mark.parametrize("row", _blocks(), ids=[r.id for r in _blocks()])
def test_block_stage_combinations(t4k, dev, row):
    """img_block and gather_pool under relu / leaky / tanh in front, max / min / avg, an activation behind (rotated through the combinations),
    with and without the flatten copy: every tensor against the witness of its own op, masks bit-equal"""
    on_label(row, cu_count(t4k))
    run_forward(t4k, dev, row, True)
    run_forward(t4k, dev, row, False)
    free(dev)


@pytest.mark.parametrize("c0", [8, 5], ids=["c0_mod4", "c0_odd"])
def test_block_with_dropout_in_front(t4k, dev, oracle, c0):
    """gather_pool draws the mask in its epilogue (one Philox block per quad of channels when C0 % 4 == 0, per element otherwise): the draws are the
    oracle's stream at the same seed and offset, the mask bit-equal, the stream advanced as the oracle's"""
    r = cc.Row("gather_pool_dropout_c%d" % c0, "block", 2, 6, 10, 2, c0, 3, "gather_pool<raw,ks1>", "dropout in front", blk=cc.blk(pre=cc.L_DROPOUT, post=0, copy=True))
    on_label(r, cu_count(t4k))
    n = r.N * r.H1 * r.W1 * c0
    orc = oracle.lib(); orc.t4o_rand_init(SEED); orc.t4o_rand_set_offset(OFFSET)
    u = np.zeros(n, np.float32); orc.t4o_dropout_mask(oracle.P(u), n)
    for exact in (True, False):
        got = run_forward(t4k, dev, r, exact)              # sets the library's stream to (SEED, OFFSET) in front of the call
        wo, wm = wt.act("dropout", got["O"], 0.5, u.reshape(got["O"].shape))
        wt.equal(r.id + " mask", got["PREM"], wm.exact, kind="conv exact: block masks")
        wt.equal(r.id + " out", got["PRE"], wo.exact, kind="conv exact: block masks")
        assert int(t4k.lib.t4k_rand_offset()) == int(orc.t4o_rand_offset())
    free(dev)


def test_rejected_blocks_write_nothing(t4k, dev):
    """a block t4k_poolblock_fwd would refuse is refused BEFORE the convolution runs: the status comes back, O and every tensor of the block keep
    their NaN.  KS = 0 used to divide by zero on the host (H0 / KS) in front of the validation."""
    r = cc.BY_ID["gemm_pool_k3"]
    o = cc.operands(r, True)
    K, S, P = cc.GEO[r.K]
    for ks, pool, post in ((0, cc.L_MAXPOOL, 0), (4, cc.L_MAXPOOL, 0), (2, 0, 0), (2, 99, 0), (2, cc.L_MAXPOOL, 99)):
        b = {k: Buf(dev, o[k]) for k in ("I", "F", "B")}
        b["O"], b["POOL"] = Buf(dev, nans(r.N, r.H1, r.W1, r.C0)), Buf(dev, nans(r.N, r.H1 // 2, r.W1 // 2, r.C0))
        b["POST"], b["POSTM"] = Buf(dev, nans(r.N, r.H1 // 2, r.W1 // 2, r.C0)), Buf(dev, nans(r.N, r.H1 // 2, r.W1 // 2, r.C0))
        blk = PoolBlock(); blk.KS = ks; blk.pool_layer = pool; blk.pool_out = b["POOL"].ptr
        blk.post_layer = post; blk.post_out = b["POST"].ptr; blk.post_mask = b["POSTM"].ptr
        dev.torch.cuda.synchronize()
        l0 = launches(t4k)
        rc = t4k.lib.t4k_conv2d_block_fwd(b["I"].ptr, None, b["O"].ptr, b["F"].ptr, b["B"].ptr, ctypes.byref(blk), r.N, r.H1, r.W1, r.C1, r.H1, r.W1, r.C0, K, S, P, None)
        assert rc == UNSUPPORTED and launches(t4k) == l0, (ks, pool, post, rc)
        call(t4k, "t4k_sync", None)
        for k in b:
            b[k].untouched("rejected block (KS %d, pool %d, post %d) %s" % (ks, pool, post, k))
    free(dev)


# ----------------------------------------------------------------------------- 5. the rung file's comments
def test_the_rung_files_comments(t4k, dev):
    """every id of tests/test_gpu_conv_rungs.py through the hook (pytest -s prints what it reports): the plan is the mirror's, and the table row
    of the same id - whose label was written from that file's comment - is on it"""
    cu = cu_count(t4k)
    rows = [cc.Row(c[0], "fwd", c[1], c[2], c[3], c[4], c[5], c[6], None, "rung file", icopy=c[7], skew={"I": c[8]} if c[8] else None) for c in RUNG_FWD]
    rows += [cc.Row(c[0], "block", c[1], c[2], c[3], c[4], c[5], c[6], None, "rung file", icopy=c[7], blk=cc.blk(copy=True)) for c in RUNG_BLOCK]
    rows += [cc.Row(c[0], "bwd", *c[1:], None, "rung file") for c in RUNG_BWD]
    for r in rows:
        got = run_row(t4k, dev, r, True, **({"forms": ("dx+df",)} if r.entry == "bwd" else {}))
        plan = last_plan(t4k)
        print("rung %-40s %s" % (r.id, plan))
        assert got and plan == r.plan(cu)[0]
        named = {"img_block": "img_block_c3_to_6"}.get(r.id, r.id)
        if cu == cc.CU:
            assert plan == cc.BY_ID[named].label, (r.id, plan, cc.BY_ID[named].label)
        free(dev)
    assert not cc.DRIFTED


# ----------------------------------------------------------------------------- 6. streams and capture
@pytest.mark.parametrize("rid", ["gather_ksplit2", "convbig8_n64", "df_mfma_slices__dx_and_fold", "dfw__fold_add__dx_convbig8"])
def test_streams_and_capture(t4k, dev, rid):
    """a gather, a big8 and two backward rows on a library stream (its own workspace) and replayed from a captured graph: bit-equal to the
    default-stream result, on the plan the mirror gives"""
    r = cc.BY_ID[rid]
    kw = {"forms": ("dx+df",)} if r.entry == "bwd" else {}
    ref = run_row(t4k, dev, r, True, **kw)
    s = ctypes.c_void_p(); t4k.call("t4k_stream_create", ctypes.byref(s))
    try:
        got = run_row(t4k, dev, r, True, stream=s, tag="library stream ", **kw)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), k
        # captured: the same call recorded, then replayed onto NaN-prefilled outputs
        cu = cu_count(t4k)
        o = cc.operands(r, True)
        H0, W0 = r.out_hw(); K, S, P = cc.GEO[r.K]
        geo = (r.N, r.H1, r.W1, r.C1, H0, W0, r.C0, K, S, P)
        if r.entry == "fwd":
            b = {k: Buf(dev, o[k]) for k in ("I", "F", "B")}; b["O"] = Buf(dev, nans(r.N, H0, W0, r.C0))
            fn = lambda: t4k.lib.t4k_conv2d_fwd2(b["I"].ptr, None, b["O"].ptr, b["F"].ptr, b["B"].ptr, *geo, s)
            outs = {"O": (r.N, H0, W0, r.C0)}
        else:
            b = {k: Buf(dev, o[k]) for k in ("I", "DO", "F")}
            b["DX"], b["DF"], b["DB"] = Buf(dev, nans(*o["I"].shape)), Buf(dev, o["DF0"]), Buf(dev, o["DB0"])
            fn = lambda: t4k.lib.t4k_conv2d_bwd2(b["I"].ptr, b["DO"].ptr, b["DX"].ptr, None, b["F"].ptr, b["DF"].ptr, b["DB"].ptr, *geo, 1, s)
            outs = {"DX": o["I"].shape, "DF": o["DF0"].shape, "DB": o["DB0"].shape}
        dev.torch.cuda.synchronize()
        g = ctypes.c_void_p()
        t4k.call("t4k_graph_begin", s)
        l0 = launches(t4k)
        rc = fn()
        n, plan = launches(t4k) - l0, last_plan(t4k)
        t4k.call("t4k_graph_end", s, ctypes.byref(g))
        assert rc == 0 and (plan, n) == r.plan(cu, **({"dx": True, "df": True} if r.entry == "bwd" else {})), (rid, rc, plan, n)
        t4k.call("t4k_graph_launch", g, s)
        for k, shape in outs.items():
            assert np.array_equal(b[k].get(rid + " captured " + k, shape, s), ref[k]), k
        t4k.call("t4k_graph_destroy", g)
        free(dev)
    finally:
        t4k.call("t4k_stream_destroy", s)


def test_zz_report_worst_ratios_and_wall_time():
    """the worst |error| / bound per engine over the float passes above, and the file's wall time (pytest -s prints both; tests/README.md quotes them)"""
    print("\nconv sweep, worst |err| / bound per engine:")
    for kind in sorted(k for k in wt.WORST if k.startswith("conv:")):
        print("  %-44s %.3g   %s" % (kind, wt.WORST[kind][0], wt.WORST[kind][1]))
        assert wt.WORST[kind][0] <= 1.0
    for kind in sorted(k for k in wt.WORST if k.startswith("conv exact:")):
        assert wt.WORST[kind][0] == 0.0, kind
    print("conv sweep wall time: %.1f s" % (time.time() - CLOCK.get("t0", time.time())))
