"""`vector{ heads causal } linear`, the attention layer, on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so).

The net is `2 4 4 8 nn.model 0.5 24 conv1x1 <vector> linear 0.5 8 conv1x1 flatten 10 linear softmax` (16 tokens, 2 heads of 4 channels) with the two
conv1x1 layers' weights set through `nn.w=` / `nn.b=`.  After `forward` the attention layer's output is bit-equal to t4k_attention_fwd called on the layer's
own fetched input, and after `T backprop` the dX it leaves in its input tensor is bit-equal to t4k_attention_bwd on the dY the VM itself stored; both are
inside the staged float64 witnesses of tests/attn_witness.py.  The first conv1x1's dW is held against torch's float64 autograd through conv1x1 and
scaled_dot_product_attention, with the witnesses propagated: attn_witness.bwd_chain for the attention stage, f64_witness.conv_df for the conv's own sum.  The
layer's launches are the plan's forward and the plan's backward plus one copy, counted as the difference between two nets that differ by the layer alone.
`nn.sgd` and `nn.adam` steps run and move both conv1x1 layers; the `.t4` round trip gives the same forward bits."""
import ctypes

import numpy as np
import pytest
import torch

import attn_witness as aw
import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_pool_geo import lcount
from test_gpu_pool_geo_words import layer_tensors, operand

pytestmark = pytest.mark.gpu

H, W, C, E, HEADS, D = 4, 4, 8, 8, 2, 4
L = H * W
NET = "0.5 24 conv1x1 %s linear 0.5 8 conv1x1 flatten 10 linear softmax"
VEC = {0: "1 vector{ 2 }", 1: "2 vector{ 2 1 }"}


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def nan(k):
    return np.full(k, np.nan, np.float32)


def set_conv(vm, name, i, F, B):
    vm.store(F, "%s %d %d %d %d tensor" % ((name,) + F.shape)); out = vm.eval("%d nn.w=" % i)
    vm.store(B, "%d vector" % B.size); out += vm.eval("%d nn.b= drop" % i)
    assert "?" not in out and "shape" not in out, out


def build(vm, name, N, causal, rng):
    vm.eval("%d %d %d %d nn.model %s constant %s" % (N, H, W, C, NET % VEC[causal], name))
    F0, B0 = operand(rng, C, 1, 1, 3 * E) / np.float32(np.sqrt(C)), operand(rng, 3 * E) / np.float32(4.0)
    F2, B2 = operand(rng, E, 1, 1, E) / np.float32(np.sqrt(E)), operand(rng, E) / np.float32(4.0)
    set_conv(vm, name, 0, F0, B0); set_conv(vm, name, 2, F2, B2)
    return F0, B0, F2, B2


def entries(t4k, QKV, DY, causal):
    """the two entries on the same tensors: (Y, LSE, DQKV)"""
    N = QKV.shape[0]
    dQ, dDY = Dev(QKV), Dev(DY)
    dO, dOK, dL, dG = Dev(nan(N * L * E)), Dev(nan(N * L * E)), Dev(nan(N * HEADS * L)), Dev(nan(3 * N * L * E))
    t4k.call("t4k_attention_fwd", dQ.p, dO.p, dOK.p, dL.p, N, L, HEADS, D, causal, None)
    t4k.call("t4k_attention_bwd", dQ.p, dOK.p, dDY.p, dL.p, dG.p, N, L, HEADS, D, causal, None)
    return dO.get(t4k, (N, L, E)).copy(), dL.get(t4k, (N, HEADS, L)).copy(), dG.get(t4k, (N, L, 3 * E)).copy()


def test_network_text(vm):
    vm.eval("2 4 4 8 nn.model " + (NET % VEC[1]) + " constant atxt")
    txt = vm.eval("atxt network drop")
    assert "[  1] attentn: T4[2,4,4,24] #p=0 T4[2,4,4,8] heads=2, causal=1\n[  2] conv2d : T4[2,4,4,8]" in txt, txt
    assert "nn#iattention heads=5? channels=24" in vm.eval("2 4 4 24 nn.model 1 vector{ 5 } linear drop")
    assert "nn#iattention heads=6? channels=24" in vm.eval("2 4 4 24 nn.model 1 vector{ 6 } linear drop")     # d = 4 / 3: the plan's rule, through t4k_attention_plan


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("N", [2, 64])
def test_the_layer_inside_a_net(vm, t4k, N, causal):
    name = "atn%dc%d" % (N, causal)
    rng = np.random.default_rng(5 + N + causal)
    F0, B0, _, _ = build(vm, name, N, causal, rng)
    X = operand(rng, N, H, W, C)
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    acts = layer_tensors(vm, name, 4)
    assert acts[1].shape == (N, H, W, 3 * E) and acts[2].shape == (N, H, W, E), [a.shape for a in acts]
    T = np.zeros((N, 1, 10, 1), np.float32); T[np.arange(N), 0, rng.integers(0, 10, N), 0] = 1.0
    vm.store(T, "%d 1 10 1 tensor constant t%s t%s" % (N, name, name)); vm.eval("drop")
    out = vm.eval("%s t%s backprop drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    grads = layer_tensors(vm, name, 4)                                   # layer i now holds dX of op i
    QKV, DY = acts[1].reshape(N, L, 3 * E), grads[2].reshape(N, L, E)
    assert DY.any()
    Y, LSE, G = entries(t4k, QKV, DY, causal)
    assert np.array_equal(acts[2].reshape(N, L, E).view(np.uint32), Y.view(np.uint32)), "the layer's output is not the entry's"
    assert np.array_equal(grads[1].reshape(N, L, 3 * E).view(np.uint32), G.view(np.uint32)), "the layer's dX is not the entry's"
    out8 = (ctypes.c_int * 8)()
    assert t4k.lib.t4k_attention_plan(N, L, HEADS, D, causal, 1, 32 << 20, out8) == 0
    wl, wy = aw.fwd(QKV, HEADS, causal, out8[3])
    aw.check(name + " lse", LSE, wl); aw.check(name + " y", Y, wy)
    aw.check(name + " dqkv", G, aw.bwd(QKV, Y, DY, LSE, HEADS, causal)[1])
    # the first conv1x1's dW against torch's float64 autograd through conv1x1 -> attention on the stored QKV, the upstream gradient the stored dY
    x = torch.tensor(X.reshape(N * L, C).astype(np.float64))
    w = torch.tensor(F0.reshape(C, 3 * E).astype(np.float64), requires_grad=True)
    qkv = x @ w + torch.tensor(B0.astype(np.float64))
    qkv = qkv + (torch.tensor(QKV.reshape(N * L, 3 * E).astype(np.float64)) - qkv).detach()       # the values the layer read, the gradient path of the conv
    t = qkv.reshape(N, L, 3, HEADS, D).permute(2, 0, 3, 1, 4)
    ty = torch.nn.functional.scaled_dot_product_attention(t[0], t[1], t[2], is_causal=bool(causal), scale=aw.scale_of(D))
    ty.backward(torch.tensor(DY.astype(np.float64)).reshape(N, L, HEADS, D).permute(0, 2, 1, 3))
    wg = aw.bwd_chain(QKV, Y, DY, LSE, HEADS, causal, out8[3])
    own = fw.conv_df(X, grads[1], 1, 1, 0)                                # the conv's sum over the dY it read
    bound = np.abs(x.numpy()).T @ wg.bound().reshape(N * L, 3 * E) + own.bound().reshape(C, 3 * E)
    dw = vm.fetch("%s 0 nn.dw" % name).copy(); vm.eval("drop drop")
    assert dw.size == C * 3 * E and np.isfinite(dw).all() and dw.any()
    aw.check(name + " conv1x1 dW", dw.reshape(C, 3 * E), aw.WB(w.grad.numpy(), bound))


def launches(vm, t4k, words):
    vm.eval(words)
    l0 = lcount(t4k); vm.eval(words); return lcount(t4k) - l0


@pytest.mark.parametrize("causal", [0, 1])
def test_the_layers_launches(vm, t4k, causal):
    """two nets that differ by the attention layer alone (sigmoid layers on either side join no fused group): the forward's difference is the plan's forward
    launches, the backward's the plan's backward launches and the one copy of dX over x"""
    N = 2
    a, b = "atla%d" % causal, "atlb%d" % causal
    vm.eval("%d 4 4 24 nn.model sigmoid %s linear sigmoid constant %s" % (N, VEC[causal], a))
    vm.eval("%d 4 4 24 nn.model sigmoid sigmoid constant %s" % (N, b))
    rng = np.random.default_rng(3)
    vm.store(operand(rng, N, 4, 4, 24), "%d 4 4 24 tensor constant xatl%d xatl%d" % (N, causal, causal)); vm.eval("drop")
    vm.store(operand(rng, N, 4, 4, 8), "%d 4 4 8 tensor constant tatla%d tatla%d" % (N, causal, causal)); vm.eval("drop")
    vm.store(operand(rng, N, 4, 4, 24), "%d 4 4 24 tensor constant tatlb%d tatlb%d" % (N, causal, causal)); vm.eval("drop")
    fa, fb = (launches(vm, t4k, "%s xatl%d forward drop" % (m, causal)) for m in (a, b))
    ba, bb = (launches(vm, t4k, "%s t%s backprop drop" % (m, m)) for m in (a, b))
    out8 = (ctypes.c_int * 8)()
    assert t4k.lib.t4k_attention_plan(N, 16, 2, 4, causal, 1, 32 << 20, out8) == 0
    print("forward launches %d against %d, backward %d against %d; the plan %s" % (fa, fb, ba, bb, list(out8)))
    assert fa - fb == out8[4] and ba - bb == out8[5] + 1, (fa, fb, ba, bb, list(out8))


@pytest.mark.parametrize("opt", ["0.01 0.0 nn.sgd", "0.001 0.9 nn.adam"], ids=["sgd", "adam"])
def test_the_optimizers_move_both_conv1x1_layers(vm, opt):
    name = "ato" + opt.split(".")[-1]
    rng = np.random.default_rng(13)
    F0, B0, F2, B2 = build(vm, name, 2, 1, rng)
    vm.store(operand(rng, 2, H, W, C), "2 %d %d %d tensor constant x%s x%s" % (H, W, C, name, name)); vm.eval("drop")
    T = np.zeros((2, 1, 10, 1), np.float32); T[0, 0, 3, 0] = T[1, 0, 7, 0] = 1.0
    vm.store(T, "2 1 10 1 tensor constant t%s t%s" % (name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward t%s backprop drop" % (name, name, name))
    assert "not supported" not in out and "failed" not in out, out
    out = vm.eval("%s %s drop" % (name, opt))
    assert "not supported" not in out and "failed" not in out, out
    for i, F in ((0, F0), (2, F2)):
        w = vm.fetch("%s %d nn.w" % (name, i)).copy(); vm.eval("drop drop")
        assert np.isfinite(w).all() and np.count_nonzero(w.ravel() != F.ravel()) > F.size // 2, (i, w.ravel()[:8], F.ravel()[:8])
    txt = vm.eval("%s network drop" % name)
    assert "attentn: T4[2,4,4,24] #p=0 T4[2,4,4,8] heads=2, causal=1" in txt, txt


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes the layer's line and no blob for it; `load` into a net built alike (other weights) gives the same forward bits"""
    rng = np.random.default_rng(17)
    build(vm, "atva", 2, 1, rng)
    f = str(tmp_path / "a.t4")
    vm.eval('atva s" %s" save' % f); vm.eval("drop")
    blob = open(f, "rb").read()
    assert b"\nheads=2, causal=1attentn\n" in blob and b"attentn\n\n---" not in blob.split(b"\n\n", 1)[1]
    assert blob.count(b"\n--- w.") == 3                                    # two conv1x1 and the linear layer: none for attention
    vm.eval("2 %d %d %d nn.model %s constant atvb" % (H, W, C, NET % VEC[0]))     # built with the other mask: the file's line rebuilds the layer
    out = vm.eval('atvb s" %s" load' % f); out += vm.eval("drop")
    assert "error" not in out, out
    assert "heads=2, causal=1" in vm.eval("atvb network drop")
    X = operand(rng, 2, H, W, C)
    vm.store(X, "2 %d %d %d tensor constant xatv xatv" % (H, W, C)); vm.eval("drop")
    outs = []
    for m in ("atva", "atvb"):
        out = vm.eval("%s xatv forward drop" % m)
        assert "not supported" not in out and "failed" not in out, out
        outs.append([t.copy() for t in layer_tensors(vm, m, 7)])
    for x, y in zip(*outs):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert outs[0][6].shape[-2] == 10 or outs[0][6].size == 20
