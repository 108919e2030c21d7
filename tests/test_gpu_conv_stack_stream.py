"""Streaming stores of the conv stack's dead layer tensors (csrc/conv_stack_kernels.hip.inc, the table at `gstore`): under the banded plan the
forward stores X0, O, P, Q, R and the banded backward every dX of a layer tensor with a streaming cache policy, because no launch of the step reads
them.  A policy changes no value - what can go wrong is a vector form of the store helper (1, 2, 4 floats) and a tensor written under one policy and
then read or rewritten under another.  Three small stacks, N = 3 each, all planned with more than one backward band:

  a  one stage, 10 x 10 x 1 -> 3 channels, K = 3, maxpool + relu, no flatten: pooled rows of 15 floats (store width 1), one-byte arg-max codes; the
     stack's last tensor has a reader behind the stack and keeps its plain stores.  (The pooled grid is 5 x 5: a pooled stage needs even H and W, so
     a 5 x 5 input itself is not a stack.)
  b  two stages, 6 x 6 x 2 -> 5 -> 6 channels, K = 3, a bare conv in front, then dropout | maxpool | relu and the flatten: rows of 30 and pooled rows
     of 18 floats (store width 2), two-byte arg-max codes
  c  the LeNet front end 28 x 28 x 1 -> 10 -> 20: store width 4, four-byte arg-max codes

Operands, the oracle's separate layers and the tolerances are those of test_gpu_conv_stack.py (1e-4 relative, dropout masks bit-exact, the Philox
position exact).  The reference of a stack - the oracle's forward of batch B, the stack's own forward of B read back through the host, and the
oracle's backward on those tensors (so masks and arg-max positions agree by construction) - is computed once and shared by the three tests."""
import ctypes

import numpy as np
import pytest

from test_gpu_conv_stack import ConvStage, RTOL, _build, _oracle_backward, _oracle_forward, _params
from test_gpu_parity import Dev, p, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


# (N, H, W, C_in, [(C0, K, pre, pool, post)], flatten)
STACKS = {
    "a": (3, 10, 10, 1, [(3, 3, None, "max", "relu")], False),
    "b": (3, 6, 6, 2, [(5, 3, None, None, None), (6, 3, "dropout", "max", "relu")], True),
    "c": (3, 28, 28, 1, [(10, 3, None, "max", "relu"), (20, 3, "dropout", "max", "relu")], True),
}
SEED_A, OFF_A, SEED_B, OFF_B = 911, 4096, 733, 8192
FWD_KEYS = ("O", "pre_mask", "pre_out", "pool_out", "post_mask", "post_out", "copy_out")
_REF = {}


def _last(st_):
    C0, K, pre, pool, post = st_
    return "post_out" if post else ("pool_out" if pool else ("pre_out" if pre else "O"))


def _banded(t4k, arr, n_stage, N):
    sp, bs = ctypes.c_int(0), ctypes.c_int(0)
    assert t4k.lib.t4k_conv_stack_plan(arr, n_stage, N, ctypes.byref(sp), ctypes.byref(bs)) == 1
    return bs.value


def _fresh(dev, oracle, R):
    """buffers of their own for one test: the stage records, the batch and gradient uploads, DF | DB preloaded (the fold must add)"""
    N, H, W, Cin, stages, flat = R["stack"]
    arr, bufs = _build(dev, oracle, R["XB"], stages, flat, R["params"], R["ref"])
    for d in bufs:
        d["DF"].fill_(0.25); d["DB"].fill_(-0.5)
    return arr, bufs


def _forward(t4k, arr, bufs, n_stage, N, dX, seed, off):
    """the batch enters through a buffer of its own; the layer-0 copy (a dead store site) lands in stage 0's input tensor"""
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off)
    t4k.call("t4k_conv_stack_fwd", p(dX), p(bufs[0]["X"]), arr, n_stage, N, None)


def _download_fwd(dev, bufs, ref):
    return [{k_: dev.down(d[k_]).reshape(ref[si][k_].shape).copy() for k_ in FWD_KEYS if k_ in ref[si]} for si, d in enumerate(bufs)]


def _reference(t4k, dev, oracle, name):
    if name in _REF:
        return _REF[name]
    N, H, W, Cin, stages, flat = STACKS[name]
    rng = np.random.default_rng(1200 + ord(name))
    XA = rng.standard_normal((N, H, W, Cin)).astype(np.float32) * 2
    XB = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    params = _params(rng, Cin, stages)
    ref, end = _oracle_forward(oracle, XB, stages, flat, params, SEED_B, OFF_B)
    R = {"stack": STACKS[name], "XA": XA, "XB": XB, "params": params, "ref": ref, "end": end}
    arr, bufs = _fresh(dev, oracle, R)
    assert t4k.lib.t4k_conv_stack_ok(arr, len(stages), N) == 1
    assert _banded(t4k, arr, len(stages), N) > 1, "stack %s plans one backward band on this part: take the next larger H" % name
    _forward(t4k, arr, bufs, len(stages), N, dev.up(XB), SEED_B, OFF_B)
    got = _download_fwd(dev, bufs, ref)
    x = XB
    for si, st_ in enumerate(stages):
        got[si]["in"] = x; x = got[si][_last(st_)]; got[si]["last"] = x
    R["got_fwd"] = got
    R["DYA"] = rng.standard_normal(x.shape).astype(np.float32)
    R["DYB"] = rng.standard_normal(x.shape).astype(np.float32)
    R["want"] = _oracle_backward(oracle, got, stages, flat, params, R["DYB"])
    _REF[name] = R
    return R


def _check_forward(R, got, x0, rand_end):
    """every layer tensor of the forward against the oracle's separate layers (the dead ones included: read back through the host)"""
    N, H, W, Cin, stages, flat = R["stack"]
    assert np.array_equal(x0, R["XB"]), "layer-0 copy of the batch"
    assert rand_end == R["end"], "Philox position"
    for si, (C0, K, pre, pool, post) in enumerate(stages):
        for k_ in FWD_KEYS:
            if k_ not in R["ref"][si]:
                continue
            want, g = R["ref"][si][k_], got[si][k_]
            if k_.endswith("mask"):
                if (pre if k_ == "pre_mask" else post) == "dropout":
                    assert np.array_equal(g, want), "stage %d %s" % (si, k_)
                else:
                    assert np.mean(np.abs(g - want) > 1e-3) < 1e-4, "stage %d %s" % (si, k_)
                continue
            e = rel(g, want)
            assert e < RTOL, "stage %d %s: %.3g" % (si, k_, e)


def _check_survivors(dev, R, bufs):
    """what a backward leaves of the forward of batch B - the masks and the flatten copy - is the reference forward's, bit for bit (and that one is
    held to the oracle by _check_forward)"""
    for si, d in enumerate(bufs):
        for k_ in ("pre_mask", "post_mask", "copy_out"):
            if k_ in R["ref"][si]:
                assert np.array_equal(dev.down(d[k_]).reshape(R["ref"][si][k_].shape), R["got_fwd"][si][k_]), "stage %d %s" % (si, k_)


def _check_backward(dev, R, bufs):
    """every dX tensor and dF | dB against the oracle's separate layers in reverse"""
    N, H, W, Cin, stages, flat = R["stack"]
    for si in range(len(stages) - 1, -1, -1):
        t, d = R["want"][si], bufs[si]
        e = rel(dev.down(d["DXS"]), t["DX"])
        assert e < RTOL, "stage %d dX (scratch copy): %.3g" % (si, e)
        assert np.array_equal(dev.down(d["X"]), dev.down(d["DXS"])), "stage %d: in = dx" % si
        e = rel(dev.down(d["DF"]) - 0.25, t["DF"])
        assert e < RTOL, "stage %d dF: %.3g" % (si, e)
        e = rel(dev.down(d["DB"]) + 0.5, t["DB"])
        assert e < RTOL, "stage %d dB: %.3g" % (si, e)
        last = _last(stages[si])
        for k_ in ("O", "pre_out", "pool_out", "post_out"):
            if k_ not in t or (si + 1 < len(stages) and k_ == last) or (k_ == last and "copy_out" not in t):
                continue              # the next stage's input tensor (its dX: checked above) / the last tensor without a flatten: nothing writes it
            e = rel(dev.down(d[k_]).reshape(t[k_].shape), t[k_])
            assert e < RTOL, "stage %d bwd %s: %.3g" % (si, k_, e)


@pytest.mark.parametrize("name", sorted(STACKS))
def test_forward_then_banded_backward(t4k, dev, oracle, name):
    R = _reference(t4k, dev, oracle, name)
    N, H, W, Cin, stages, flat = R["stack"]
    arr, bufs = _fresh(dev, oracle, R)
    _forward(t4k, arr, bufs, len(stages), N, dev.up(R["XB"]), SEED_B, OFF_B)
    end = t4k.lib.t4k_rand_offset()
    got = _download_fwd(dev, bufs, R["ref"])
    _check_forward(R, got, dev.down(bufs[0]["X"]), end)
    for si in range(len(stages)):
        for k_ in got[si]:
            assert np.array_equal(got[si][k_], R["got_fwd"][si][k_]), "stage %d %s differs from the reference forward" % (si, k_)
    t4k.call("t4k_conv_stack_bwd", p(dev.up(R["DYB"])), arr, len(stages), N, 1, None)
    _check_survivors(dev, R, bufs)
    _check_backward(dev, R, bufs)


@pytest.mark.parametrize("name", sorted(STACKS))
def test_forward_then_whole_image_backward(t4k, dev, oracle, name):
    """train bit 1: the whole-image kernel, which reads the forward values of the streamed layer tensors (conv inputs, pool inputs) on the GPU in the
    very next launch"""
    R = _reference(t4k, dev, oracle, name)
    N, H, W, Cin, stages, flat = R["stack"]
    arr, bufs = _fresh(dev, oracle, R)
    dX, dDY = dev.up(R["XB"]), dev.up(R["DYB"])
    _forward(t4k, arr, bufs, len(stages), N, dX, SEED_B, OFF_B)
    t4k.call("t4k_conv_stack_bwd", p(dDY), arr, len(stages), N, 3, None)
    assert t4k.lib.t4k_rand_offset() == R["end"]
    _check_survivors(dev, R, bufs)
    _check_backward(dev, R, bufs)


@pytest.mark.parametrize("name", sorted(STACKS))
def test_plain_and_streamed_stores_alternate_on_the_same_lines(t4k, dev, oracle, name):
    """forward A | whole-image backward (plain stores over the streamed tensors) | forward B | banded backward, in stream order with no synchronise
    inside: two launches of the same module back to back, both policies on the same lines.  The first backward's gradients go to buffers of their
    own, so dF | dB of the second are checked as in the other tests."""
    R = _reference(t4k, dev, oracle, name)
    N, H, W, Cin, stages, flat = R["stack"]
    n = len(stages)
    arr, bufs = _fresh(dev, oracle, R)
    arr2 = (ConvStage * n)()
    ctypes.memmove(arr2, arr, ctypes.sizeof(arr))
    side = [(dev.zeros(d["DF"].shape), dev.zeros(d["DB"].shape)) for d in bufs]
    for si in range(n):
        arr2[si].DF, arr2[si].DB = p(side[si][0]), p(side[si][1])
    dXA, dXB, dDYA, dDYB = dev.up(R["XA"]), dev.up(R["XB"]), dev.up(R["DYA"]), dev.up(R["DYB"])
    dev.torch.cuda.synchronize()
    _forward(t4k, arr, bufs, n, N, dXA, SEED_A, OFF_A)
    t4k.call("t4k_conv_stack_bwd", p(dDYA), arr2, n, N, 3, None)
    _forward(t4k, arr, bufs, n, N, dXB, SEED_B, OFF_B)
    t4k.call("t4k_conv_stack_bwd", p(dDYB), arr, n, N, 1, None)
    assert t4k.lib.t4k_rand_offset() == R["end"]
    _check_survivors(dev, R, bufs)
    _check_backward(dev, R, bufs)
    assert all(float(df.abs().max()) > 0 for df, _ in side), "the first backward's gradients"
