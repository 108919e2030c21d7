"""k_head_bwd_l32 (t4k_mlp_head_bwd / t4k_mlp_block_bwd) with its tile prologue on range-checked buffer loads: a tensor is a descriptor of its
logical size, a lane keeps one 32-bit offset per operand family, and what lies past a tensor's end reads 0.0f from the hardware.  What can go
wrong with that is a bound that is NOT the tensor's end and is left to the range check, an offset that wraps, a descriptor one row short or long.
Through the C ABI, on five shapes (N, E1, EA, EB), each the smallest that reaches one of those:

  (1, 4, 4, 1)          every descriptor at its smallest: every lane but one is out of range
  (33, 36, 36, 3)       odd EB: the MFMA slot j == EB is the next row's first element and is excluded by the lane, not by the range check; ragged
                        column bound inside a row for both tile kinds; ragged second sample block
  (65, 132, 100, 16)    EB = 16: all eight MFMA slots, the immediate offsets at their largest; EA = 100: the fourth e block ragged
  (256, 36, 256, 16)    the upper edge of admission: nblk = 8, every wave has a second block (the flagship never runs it); largest descriptors
  (128, 68, 100, 10)    the flagship's head on three column tiles

in three forms: one mask (t4k_mlp_head_bwd), masks behind both layers (t4k_mlp_block_bwd, train = 1), and the frozen form (train = 0).  Each checks

  1. guarded operands: every input and output tensor sits in an allocation of its own with 4 KiB of quiet NaN in front of it and behind it (the
     pointer keeps its 16-byte alignment).  Every stored tensor is finite and held to its float64 witness as tests/test_gpu_linear_sweep.py holds
     it, on the exact and on the float pass, and both guards of every tensor are bit-unchanged: a read past a tensor's end that reaches an MFMA
     shows as NaN, a store past it shows in the guard;
  2. bit equality with the kernel in front of this change: the SHA-256 of every stored tensor's bytes on the float pass - P, Y2, X2, Y1, Y1B,
     DW2, DB2, DB1, DW1, X1 as dX1 and the outputs of the mask chain behind it - against tests/golden/head_bwd_addr/parent_digests.json.  The file
     was recorded once on an MI355X by running digests() below, with this file's operands, against a library built from commit 1f097db
     ("k_head_bwd_l32: role stamps; serial operand round trips removed"), the commit in front of this change.  Same MFMAs in the same order:
     nothing may differ;
  3. three launches back to back on one stream with no host synchronisation between them, in every form (X1, X2 and P re-uploaded in stream
     order, the payload only: the guards stay as the launches left them), the gradients accumulating: every tensor held as in 1, the gradients to
     the witness applied three times, untouched in the frozen form.

A shape that t4k_mlp_head_bwd_ok refuses on the box is skipped, and at most one of the five may be: on an MI355X none is.  The role order is the
library's.  When T4K_LIB names a LAB build, test_the_other_role_order_on_the_lab_library runs this file and the chain test once more in a child
process with T4K_HB_LAB=128, the other order of the roles over blockIdx.x (the release library compiles one order in and has no such switch).
No tolerance of its own: lc.hold with the sweep's kinds, and bit equality."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import f64_witness as wt
import linear_cases as lc
from test_gpu_parity import Dev, PoolBlock, p
from test_gpu_linear_sweep import free, launches
from test_gpu_head_bwd_chain import Thrice

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 4, 1), (33, 36, 36, 3), (65, 132, 100, 16), (256, 36, 256, 16), (128, 68, 100, 10)]
IDS = ["N%d-E1_%d-EA%d-EB%d" % s for s in SHAPES]
FORMS = ("one_mask", "mask_chain", "frozen")
GW = 1024                                                                                        # guard words on either side: 4 KiB
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_bwd_addr", "parent_digests.json")
hold = lc.hold


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


class GBuf:
    """a device tensor in an allocation of its own, 4 KiB of quiet NaN in front of it and behind it; NaN where no data is given"""

    def __init__(self, dev, shape, data=None):
        self.shape = tuple(np.atleast_1d(shape)); self.n = int(np.prod(self.shape))
        a = np.full(GW + self.n + GW, np.nan, np.float32)
        if data is not None:
            a[GW:GW + self.n] = np.asarray(data, np.float32).ravel()
        self.guard = a[:GW].view(np.uint32).copy()
        self.t = dev.up(a); assert p(self.t) % 16 == 0
        self.ptr = p(self.t) + 4 * GW

    def get(self, dev, name):
        a = dev.down(self.t)
        assert np.array_equal(a[:GW].view(np.uint32), self.guard), "%s: the guard in front of the tensor was written" % name
        assert np.array_equal(a[GW + self.n:].view(np.uint32), self.guard), "%s: the guard behind the tensor was written" % name
        return a[GW:GW + self.n].reshape(self.shape)


def admit(t4k, dims):
    N, E1, EA, EB = dims
    if t4k.lib.t4k_mlp_head_bwd_ok(N, E1, EA, EB) != 1:
        pytest.skip("%s: t4k_mlp_head_bwd_ok refuses the shape on this device" % (dims,))


def test_at_most_one_shape_is_refused(t4k):
    refused = [s for s in SHAPES if t4k.lib.t4k_mlp_head_bwd_ok(s[0], s[1], s[2], s[3]) != 1]
    assert len(refused) <= 1, refused


class Set:
    """the device tensors of one head backward in one of the three forms, every one guarded"""

    def __init__(self, dev, oracle, dims, form, exact, salt):
        N, E1, EA, EB = dims
        self.dims, self.form, self.oracle = dims, form, oracle
        self.masks = 1 if form == "one_mask" else 2
        rng = np.random.default_rng(lc.seed_of(N, EB, E1, EA, exact, self.masks, salt))
        shp = dict(X1=(N, E1), W1=(EA, E1), X2=(N, EA), W2=(EB, EA), P=(N, EB), T=(N, EB), DW1=(EA, E1), DB1=EA, DW2=(EB, EA), DB2=EB)
        self.h = {k: lc.draw(rng, exact, v) for k, v in shp.items()}                             # the gradient tensors start non-zero
        self.M2 = [lc.draw_mask(rng, exact, (N, EA)) for _ in range(self.masks)]
        self.M1 = [lc.draw_mask(rng, exact, (N, E1)) for _ in range(0 if form == "one_mask" else 2)]
        self.b = {k: GBuf(dev, v.shape, v) for k, v in self.h.items()}
        self.bM2 = [GBuf(dev, m.shape, m) for m in self.M2]; self.bM1 = [GBuf(dev, m.shape, m) for m in self.M1]
        self.bR2 = [GBuf(dev, (N, EA)) for _ in self.M2]; self.bR1 = [GBuf(dev, (N, E1)) for _ in self.M1]
        self.bY2 = GBuf(dev, (N, EB))

    def block(self, bm, bd, first_out):
        k = PoolBlock(); k.KS = 1
        k.post_layer, k.post_mask, k.post_out = self.oracle.L_DROPOUT, bm[0].ptr, first_out
        if len(bm) == 2:
            k.pre_layer, k.pre_mask, k.pre_out = self.oracle.L_LEAKYRL, bm[1].ptr, bd[0].ptr
        return k

    def launch(self, t4k):
        N, E1, EA, EB = self.dims; b = self.b
        if self.form == "one_mask":
            return t4k.lib.t4k_mlp_head_bwd(b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, self.bY2.ptr, self.bM2[0].ptr, self.bR2[0].ptr, b["DW2"].ptr,
                                            b["DB2"].ptr, b["X1"].ptr, b["W1"].ptr, b["DW1"].ptr, b["DB1"].ptr, N, E1, EA, EB, None)
        k2 = self.block(self.bM2, self.bR2, b["X2"].ptr); k1 = self.block(self.bM1, self.bR1, b["X1"].ptr)
        return t4k.lib.t4k_mlp_block_bwd(b["X2"].ptr, b["W2"].ptr, b["P"].ptr, b["T"].ptr, self.bY2.ptr, ctypes.byref(k2), self.bR2[-1].ptr, b["DW2"].ptr,
                                         b["DB2"].ptr, b["X1"].ptr, b["W1"].ptr, ctypes.byref(k1), self.bR1[-1].ptr, b["DW1"].ptr, b["DB1"].ptr,
                                         N, E1, EA, EB, 0 if self.form == "frozen" else 1, None)

    def get(self, dev):
        """every tensor of the call by name, the guards of each checked on the way: operands, Y2, Y1 / Y1B, R1_0 / R1_1, the masks as M2_i / M1_i"""
        out = {k: v.get(dev, k) for k, v in self.b.items()}
        out["Y2"] = self.bY2.get(dev, "Y2")
        for i, r in enumerate(self.bR2):
            out["Y1" if i == 0 else "Y1B"] = r.get(dev, "Y1" if i == 0 else "Y1B")
        for i, r in enumerate(self.bR1):
            out["R1_%d" % i] = r.get(dev, "R1_%d" % i)
        for i, m in enumerate(self.bM2):
            out["M2_%d" % i] = m.get(dev, "M2_%d" % i)
        for i, m in enumerate(self.bM1):
            out["M1_%d" % i] = m.get(dev, "M1_%d" % i)
        return out

    def stored(self):
        """the tensors the form stores"""
        names = ["P", "Y2", "X2", "Y1", "X1"] + (["Y1B"] if self.masks == 2 else []) + ["R1_%d" % i for i in range(len(self.M1))]
        return names + ([] if self.form == "frozen" else ["DW2", "DB2", "DB1", "DW1"])


def run_once(t4k, dev, oracle, dims, form, exact):
    s = Set(dev, oracle, dims, form, exact, 5)
    l0 = launches(t4k)
    rc = s.launch(t4k)
    assert rc == 0, (dims, form, rc, t4k.lib.t4k_last_error().decode())
    assert launches(t4k) - l0 == 1, (dims, form)
    assert t4k.lib.t4k_sync(None) == 0, (dims, form)
    return s, s.get(dev)


def digests(t4k, dev, oracle):
    """{shape-form-tensor: SHA-256 of the tensor's bytes} of the float pass at every admitted shape and form: what the golden file holds"""
    out = {}
    for dims, sid in zip(SHAPES, IDS):
        if t4k.lib.t4k_mlp_head_bwd_ok(*dims) != 1:
            continue
        for form in FORMS:
            s, got = run_once(t4k, dev, oracle, dims, form, False)
            for k in s.stored():
                out["%s-%s-%s" % (sid, form, k)] = hashlib.sha256(np.ascontiguousarray(got[k]).tobytes()).hexdigest()
            free(dev)
    return out


def check_witnesses(tag, s, got, exact, times=1):
    """every tensor of the call against its witness; times = 3: the gradients have accumulated over three launches (Thrice)"""
    h, train = s.h, s.form != "frozen"
    acc = (lambda step, O0: step(O0)) if times == 1 else Thrice
    for k in s.stored():
        assert np.all(np.isfinite(got[k])), "%s: %s is not finite" % (tag, k)
    g2 = h["P"] - h["T"]
    wt.equal(tag + " out - target in place", got["P"], g2, kind="linear exact: out - target")
    wt.equal(tag + " out - target, second destination", got["Y2"], g2, kind="linear exact: out - target")
    hold(exact, tag + " dX2 (over X2)", got["X2"], wt.gemm(g2, h["W2"]), "head dX2")
    g = got["X2"]
    for i, m in enumerate(s.M2):
        d = got["Y1" if i == 0 else "Y1B"]
        hold(exact, tag + " head run stage %d" % i, d, wt.mul(g, m), "mask chain")
        g = d
    dy1 = g
    hold(exact, tag + " dX1 (over X1)", got["X1"], wt.gemm(dy1, h["W1"]), "head dX1")
    g = got["X1"]
    for i, m in enumerate(s.M1):
        d = got["R1_%d" % i]
        hold(exact, tag + " big layer's run stage %d" % i, d, wt.mul(g, m), "mask chain")
        g = d
    if train:
        hold(exact, tag + " dW2 x %d" % times, got["DW2"], acc(lambda o: wt.gemm(g2, h["X2"], O0=o, beta=1.0, tA=1), h["DW2"]), "head dW2")
        hold(exact, tag + " dB2 x %d" % times, got["DB2"], acc(lambda o: wt.dlinear_db(g2, o), h["DB2"]), "head dB2")
        hold(exact, tag + " dW1 x %d" % times, got["DW1"], acc(lambda o: wt.gemm(dy1, h["X1"], O0=o, beta=1.0, tA=1), h["DW1"]), "head dW1")
        hold(exact, tag + " dB1 x %d" % times, got["DB1"], acc(lambda o: wt.dlinear_db(dy1, o), h["DB1"]), "head dB1")
    else:
        for k in ("DW1", "DB1", "DW2", "DB2"):
            wt.equal(tag + " %s untouched (frozen)" % k, got[k], h[k])
    for k in ("W1", "W2", "T"):
        wt.equal(tag + " %s untouched" % k, got[k], h[k])
    for i, m in enumerate(s.M2):
        wt.equal(tag + " mask %d behind the head untouched" % i, got["M2_%d" % i], m)
    for i, m in enumerate(s.M1):
        wt.equal(tag + " mask %d behind the big layer untouched" % i, got["M1_%d" % i], m)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", SHAPES, ids=IDS)
def test_guarded_operands_and_the_parents_bits(t4k, dev, oracle, dims, form):
    admit(t4k, dims)
    N, E1, EA, EB = dims
    case = lc.Case("head_bwd_runs", "mlp_block_bwd", N, EB, E1, "the addressing test's shape", H=EA, masks=2)
    assert wt.is_int_exact(*lc.exact_bound(case)), dims
    with open(GOLD) as f:
        gold = json.load(f)
    for exact in (True, False):
        tag = "head addr %s %s %s" % (dims, form, "exact" if exact else "float")
        s, got = run_once(t4k, dev, oracle, dims, form, exact)
        check_witnesses(tag, s, got, exact)
        if not exact:
            for k in s.stored():
                key = "%s-%s-%s" % (IDS[SHAPES.index(dims)], form, k)
                assert hashlib.sha256(np.ascontiguousarray(got[k]).tobytes()).hexdigest() == gold[key], "%s: %s differs from the kernel in front of the change" % (tag, k)
        free(dev)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dims", SHAPES, ids=IDS)
def test_three_launches_back_to_back(t4k, dev, oracle, dims, form):
    admit(t4k, dims)
    tag = "head addr %s %s three launches" % (dims, form)
    s = Set(dev, oracle, dims, form, False, 6)
    pay = lambda b: b.t[GW:GW + b.n]                                                             # the tensor without its guards
    fresh = {k: pay(s.b[k]).clone() for k in ("X1", "X2", "P")}
    for rep in range(3):
        if rep:
            for k, t in fresh.items():
                pay(s.b[k]).copy_(t)                                                              # in stream order, no host synchronisation; the guards stay as the launches left them
        rc = s.launch(t4k)
        assert rc == 0, (tag, rep, rc, t4k.lib.t4k_last_error().decode())
    assert t4k.lib.t4k_sync(None) == 0, tag
    check_witnesses(tag, s, s.get(dev), False, times=3)
    free(dev)


def _is_lab(path):
    """a LAB build reads T4K_HB_LAB from the environment; the release library does not even hold the name (tests/test_cabi.py)"""
    with open(path, "rb") as f:
        return b"T4K_HB_LAB" in f.read()


LAB_LIB = os.environ.get("T4K_LIB") or ""


@pytest.mark.skipif(not (LAB_LIB and os.path.exists(LAB_LIB) and os.environ.get("T4K_HB_LAB") is None and _is_lab(LAB_LIB)),
                    reason="the other role order: T4K_LIB must name a LAB build (make -C tensorforth_amd/csrc LAB=1), T4K_HB_LAB unset")
def test_the_other_role_order_on_the_lab_library():
    """every case of this file and of the chain test once more with the roles over blockIdx.x in the OTHER order (LAB bit 128), in a fresh child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    here = os.path.abspath(__file__)
    r = subprocess.run([sys.executable, "-m", "pytest", here, os.path.join(os.path.dirname(here), "test_gpu_head_bwd_chain.py"), "-x", "-q", "-m", "gpu",
                        "-k", "not other_role_order"], capture_output=True, text=True, timeout=600, env=dict(os.environ, T4K_HB_LAB="128"), cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-3000:] + r.stderr[-2000:]
