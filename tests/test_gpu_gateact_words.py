"""`vector{ kind gate } elu`, the smooth and gated feed-forward activations, on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over
libt4hip.so).

The net is `2 4 4 6 nn.model 0.5 16 conv1x1 <vector> elu 0.5 6 conv1x1 flatten 10 linear softmax` with SwiGLU (`vector{ 2 1 }`) and with plain GELU
(`vector{ 0 }`).  After `forward` the layer's output is bit-equal to t4k_gateact_fwd on the layer's own fetched input, after `T backprop` the dX it leaves in
its input tensor bit-equal to t4k_gateact_bwd on the dY the VM itself stored.  The first conv1x1's dW is held against torch's float64 autograd through
conv1x1 and the activation, with the bounds propagated: test_gateact_plan.bound for the layer's dX, f64_witness.conv_df for the conv's own sum.  The layer is
one launch each way, counted as the difference between two nets that differ by the layer alone; an `nn.adam` step runs; the `.t4` round trip gives the
same forward bits."""
import numpy as np
import pytest
import torch

import attn_witness as aw
import f64_witness as fw
from test_gateact_plan import bound, rule, torch_f
from test_gpu_attention_words import set_conv
from test_gpu_bcast import Dev
from test_gpu_gateact import K_BWD
from test_gpu_pool_geo import lcount
from test_gpu_pool_geo_words import layer_tensors, operand
from test_gpu_token_ce import bits, nan

pytestmark = pytest.mark.gpu

N, H, W, C, CH = 2, 4, 4, 6, 16
T = N * H * W
NET = "0.5 16 conv1x1 %s elu 0.5 6 conv1x1 flatten 10 linear softmax"
VEC = {(2, 1): "2 vector{ 2 1 }", (0, 0): "1 vector{ 0 }"}


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def clean(out):
    assert "not supported" not in out and "failed" not in out and "nn#i" not in out and "error" not in out, out


def build(vm, name, kind, gate, rng):
    clean(vm.eval("%d %d %d %d nn.model %s constant %s" % (N, H, W, C, NET % VEC[(kind, gate)], name)))
    Hc = CH // 2 if gate else CH
    F0, B0 = operand(rng, C, 1, 1, CH) / np.float32(np.sqrt(C)), operand(rng, CH) / np.float32(4.0)
    set_conv(vm, name, 0, F0, B0); set_conv(vm, name, 2, operand(rng, Hc, 1, 1, C) / np.float32(np.sqrt(Hc)), operand(rng, C) / np.float32(4.0))
    return F0, B0


@pytest.mark.parametrize("kind,gate", list(VEC), ids=["swiglu", "gelu"])
def test_the_layer_inside_a_net(vm, t4k, kind, gate):
    name = "gan%d%d" % (kind, gate)
    rng = np.random.default_rng(5 + kind)
    F0, B0 = build(vm, name, kind, gate, rng)
    Hc = CH // 2 if gate else CH
    assert "[  1] gateact: T4[2,4,4,16] #p=0 kind=%d, gate=%d\n[  2] conv2d : T4[2,4,4,%d]" % (kind, gate, Hc) in vm.eval("%s network drop" % name)
    X = operand(rng, N, H, W, C)
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    clean(vm.eval("%s x%s forward drop" % (name, name)))
    acts = layer_tensors(vm, name, 3)
    assert acts[1].shape == (N, H, W, CH) and acts[2].shape == (N, H, W, Hc), [a.shape for a in acts]
    TG = np.zeros((N, 1, 10, 1), np.float32); TG[np.arange(N), 0, rng.integers(0, 10, N), 0] = 1.0
    vm.store(TG, "%d 1 10 1 tensor constant t%s t%s" % (N, name, name)); vm.eval("drop")
    clean(vm.eval("%s t%s backprop drop" % (name, name)))
    grads = layer_tensors(vm, name, 3)                                    # layer i now holds dX of op i
    XL, DY = acts[1].reshape(T, CH), grads[2].reshape(T, Hc)
    assert DY.any()
    dX, dDY, dY, dDX = Dev(XL), Dev(DY), Dev(nan(T * Hc)), Dev(nan(T * CH))
    t4k.call("t4k_gateact_fwd", dX.p, dY.p, T, CH, kind, gate, None)
    t4k.call("t4k_gateact_bwd", dX.p, dDY.p, dDX.p, T, CH, kind, gate, None)
    assert bits(acts[2], dY.get(t4k, (T, Hc))), "the layer's output is not the entry's"
    assert bits(grads[1], dDX.get(t4k, (T, CH))), "the layer's dX is not the entry's"
    # the first conv1x1's dW against torch's float64 autograd through conv1x1 -> the activation on the stored input, the upstream gradient the stored dY
    x = torch.tensor(X.reshape(T, C).astype(np.float64))
    w = torch.tensor(F0.reshape(C, CH).astype(np.float64), requires_grad=True)
    xl = x @ w + torch.tensor(B0.astype(np.float64))
    xl = xl + (torch.tensor(XL.astype(np.float64)) - xl).detach()         # the values the layer read, the gradient path of the conv
    y = torch_f(kind, xl[:, :Hc]) * xl[:, Hc:] if gate else torch_f(kind, xl)
    y.backward(torch.tensor(DY.astype(np.float64)))
    _, (dx, cdx, sdx) = rule(kind, gate, XL, DY)
    own = fw.conv_df(X, grads[1], 1, 1, 0)                                # the conv's sum over the dY it read
    b = np.abs(x.numpy()).T @ bound(K_BWD[kind], dx, cdx, sdx) + own.bound().reshape(C, CH)
    dw = vm.fetch("%s 0 nn.dw" % name).copy(); vm.eval("drop drop")
    assert dw.size == C * CH and np.isfinite(dw).all() and dw.any()
    aw.check(name + " conv1x1 dW", dw.reshape(C, CH), aw.WB(w.grad.numpy(), b))
    clean(vm.eval("%s 0.001 0.9 nn.adam drop" % name))                    # one step runs and moves the first projection
    w1 = vm.fetch("%s 0 nn.w" % name).copy(); vm.eval("drop drop")
    assert np.isfinite(w1).all() and np.count_nonzero(w1.ravel() != F0.ravel()) > F0.size // 2


def test_the_layer_is_one_launch_each_way(vm, t4k):
    def launches(w):
        clean(vm.eval(w)); l0 = lcount(t4k); clean(vm.eval(w)); return lcount(t4k) - l0
    rng = np.random.default_rng(3)
    vm.eval("2 4 4 16 nn.model sigmoid 2 vector{ 2 1 } elu sigmoid constant gala  2 4 4 16 nn.model sigmoid sigmoid constant galb")
    vm.store(operand(rng, 2, 4, 4, 16), "2 4 4 16 tensor constant xgal xgal"); vm.eval("drop")
    vm.store(operand(rng, 2, 4, 4, 8), "2 4 4 8 tensor constant tgala tgala"); vm.eval("drop")
    fa, fb = launches("gala xgal forward drop"), launches("galb xgal forward drop")
    ba, bb = launches("gala tgala backprop drop"), launches("galb xgal backprop drop")
    print("forward launches %d against %d, backward %d against %d" % (fa, fb, ba, bb))
    assert fa - fb == 1 and ba - bb == 1, (fa, fb, ba, bb)


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes the layer's line and no blob for it; `load` into a net built with another kind gives the same forward bits"""
    rng = np.random.default_rng(17)
    build(vm, "gava", 2, 1, rng)
    f = str(tmp_path / "g.t4")
    vm.eval('gava s" %s" save' % f); vm.eval("drop")
    blob = open(f, "rb").read()
    assert b"\nkind=2, gate=1gateact\n" in blob and blob.count(b"\n--- w.") == 3      # two conv1x1 and the linear layer: none for the activation
    clean(vm.eval("%d %d %d %d nn.model %s constant gavb" % (N, H, W, C, NET % "2 vector{ 3 1 }")))
    out = vm.eval('gavb s" %s" load' % f); out += vm.eval("drop")
    assert "error" not in out, out
    assert "kind=2, gate=1" in vm.eval("gavb network drop")
    vm.store(operand(rng, N, H, W, C), "%d %d %d %d tensor constant xgav xgav" % (N, H, W, C)); vm.eval("drop")
    outs = []
    for m in ("gava", "gavb"):
        clean(vm.eval("%s xgav forward drop" % m))
        outs.append([t.copy() for t in layer_tensors(vm, m, 7)])
    for x, y in zip(*outs):
        assert bits(x, y)
