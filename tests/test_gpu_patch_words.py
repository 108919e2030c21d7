"""The patch form of conv2d on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so), DESIGN.md 3.25: `bias C0 4 vector{ K K 0 1 } conv2d` adds the
layer, forward / backprop run it through t4k_patch_fwd / _bwd.

The net is `0.5 24 4 vector{ 8 8 0 1 } conv2d 1 vector{ 2 } linear 0.5 8 conv1x1 flatten 10 linear softmax` on [2,19,24,3]: six tokens of 24 channels, two
attention heads of 4.  After `forward` the layer's output is bit-equal to t4k_patch_fwd on the stored input and weights, after `T backprop` its `nn.dw` and
`nn.db` bit-equal to t4k_patch_bwd on the dY the VM itself stored; each is inside the float64 witness of test_gpu_patch.py on those stored operands
(f64_witness.py's principle: no error is carried from layer to layer).  The layer is one launch forward and three backward, counted as the difference
between two nets that differ by the layer alone; an `nn.adam` step changes F; the `.t4` round trip gives the same forward bits; behind a relu the layer's
dX reaches the layer in front."""
import numpy as np
import pytest

import f64_witness as fw
from test_gpu_attention_words import set_conv
from test_gpu_bcast import Dev
from test_gpu_conv_geo import at, lcount
from test_gpu_patch import witness
from test_gpu_pool_geo_words import layer_tensors, operand

pytestmark = pytest.mark.gpu

N, H1, W1, C1, C0, K = 2, 19, 24, 3, 24, 8
GEO = (N, H1, W1, C1, C0, K)
PATCH = "0.5 24 4 vector{ 8 8 0 1 } conv2d"
NET = PATCH + " 1 vector{ 2 } linear 0.5 8 conv1x1 flatten 10 linear softmax"


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def clean(out):
    assert "not supported" not in out and "failed" not in out and "nn#i" not in out and "error" not in out, out


def build(vm, name, rng, net=NET, layer=0):
    clean(vm.eval("%d %d %d %d nn.model %s constant %s" % (N, H1, W1, C1, net, name)))
    F, B = operand(rng, C1, K, K, C0) / np.float32(K * np.sqrt(C1)), operand(rng, C0) / np.float32(4.0)
    set_conv(vm, name, layer, F, B)
    return F, B


def test_the_layer_inside_a_net(vm, t4k):
    rng = np.random.default_rng(5)
    F, B = build(vm, "pan", rng)
    txt = vm.eval("pan network drop")
    assert " T4[3,8,8,24] T1[24] T4[2,19,24,3] bias=0.5, C=24, K=8, S=8, P=0\n[  1] attentn: T4[2,2,3,24]" in txt, txt
    X = operand(rng, N, H1, W1, C1)
    vm.store(X, "%d %d %d %d tensor constant xpan xpan" % (N, H1, W1, C1)); vm.eval("drop")
    clean(vm.eval("pan xpan forward drop"))
    acts = layer_tensors(vm, "pan", 2)
    assert np.array_equal(acts[0], X) and acts[1].shape == (N, 2, 3, C0)
    dI, dF, dB, dO = Dev(X), Dev(F), Dev(B), Dev(np.full(acts[1].size, np.nan, np.float32))
    t4k.call("t4k_patch_fwd", dI.p, None, dO.p, dF.p, dB.p, *GEO, None)
    assert np.array_equal(dO.get(t4k, acts[1].shape), acts[1]), "the layer's output is not the entry's"
    TG = np.zeros((N, 1, 10, 1), np.float32); TG[np.arange(N), 0, rng.integers(0, 10, N), 0] = 1.0
    vm.store(TG, "%d 1 10 1 tensor constant tpan tpan" % N); vm.eval("drop")
    clean(vm.eval("pan tpan backprop drop"))
    DY = layer_tensors(vm, "pan", 2)[1]                                   # the attention layer left its dX here: the patch layer's dY
    assert DY.any()
    dw = vm.fetch("pan 0 nn.dw").copy(); vm.eval("drop drop")
    db = vm.fetch("pan 0 nn.db").copy().ravel(); vm.eval("drop drop")
    dG, dD = Dev(DY), Dev(np.zeros(F.size + C0, np.float32))
    t4k.call("t4k_patch_bwd", dI.p, dG.p, None, None, dF.p, dD.p, at(dD, F.size), *GEO, 1, None)    # the first layer: dF | dB alone, dX on demand
    g = dD.get(t4k, (F.size + C0,))
    assert np.array_equal(g[:F.size].reshape(F.shape), dw) and np.array_equal(g[F.size:], db), "the layer's dF | dB are not the entry's"
    a = dict(I=X, F=F, B=B, G=DY, DF0=np.zeros_like(F), DB0=np.zeros_like(B))
    wo, _, wdf, wdb = witness("float", a, K)
    fw.check("O", acts[1], wo); fw.check("dF", dw, wdf); fw.check("dB", db, wdb)
    clean(vm.eval("pan 0.001 0.9 nn.adam drop"))                          # one step runs and moves the filter
    w1 = vm.fetch("pan 0 nn.w").copy(); vm.eval("drop drop")
    assert np.isfinite(w1).all() and np.count_nonzero(w1.ravel() != F.ravel()) > F.size // 2


def test_the_layers_launches(vm, t4k):
    """two nets that differ by the layer alone (sigmoid layers on either side join no fused group): one launch forward, the plan's three backward"""
    def launches(w):
        clean(vm.eval(w)); l0 = lcount(t4k); clean(vm.eval(w)); return lcount(t4k) - l0
    rng = np.random.default_rng(3)
    vm.eval("%d %d %d %d nn.model sigmoid %s sigmoid constant pala  %d %d %d %d nn.model sigmoid sigmoid constant palb" % (N, H1, W1, C1, PATCH, N, H1, W1, C1))
    vm.store(operand(rng, N, H1, W1, C1), "%d %d %d %d tensor constant xpal xpal" % (N, H1, W1, C1)); vm.eval("drop")
    vm.store(operand(rng, N, 2, 3, C0), "%d 2 3 %d tensor constant tpal tpal" % (N, C0)); vm.eval("drop")
    fa, fb = launches("pala xpal forward drop"), launches("palb xpal forward drop")
    ba, bb = launches("pala tpal backprop drop"), launches("palb xpal backprop drop")
    print("forward launches %d against %d, backward %d against %d" % (fa, fb, ba, bb))
    assert fa - fb == 1 and ba - bb == 3, (fa, fb, ba, bb)


def test_t4_file_round_trip(vm, tmp_path):
    rng = np.random.default_rng(17)
    build(vm, "pava", rng)
    f = str(tmp_path / "p.t4")
    vm.eval('pava s" %s" save' % f); vm.eval("drop")
    assert b"bias=0.5, C=24, K=8, S=8, P=0" in open(f, "rb").read()
    clean(vm.eval("%d %d %d %d nn.model %s constant pavb" % (N, H1, W1, C1, NET)))
    out = vm.eval('pavb s" %s" load' % f); out += vm.eval("drop")
    assert "error" not in out, out
    vm.store(operand(rng, N, H1, W1, C1), "%d %d %d %d tensor constant xpav xpav" % (N, H1, W1, C1)); vm.eval("drop")
    outs = []
    for m in ("pava", "pavb"):
        clean(vm.eval("%s xpav forward drop" % m))
        outs.append(layer_tensors(vm, m, 7))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_behind_a_relu_the_layer_in_front_receives_dx(vm, t4k):
    rng = np.random.default_rng(23)
    F, B = build(vm, "parl", rng, net="relu " + PATCH + " flatten 10 linear softmax", layer=1)
    X = operand(rng, N, H1, W1, C1)
    vm.store(X, "%d %d %d %d tensor constant xparl xparl" % (N, H1, W1, C1)); vm.eval("drop")
    clean(vm.eval("parl xparl forward drop"))
    I = layer_tensors(vm, "parl", 2)[1]
    assert np.array_equal(I, np.maximum(X, 0))
    TG = np.zeros((N, 1, 10, 1), np.float32); TG[np.arange(N), 0, rng.integers(0, 10, N), 0] = 1.0
    vm.store(TG, "%d 1 10 1 tensor constant tparl tparl" % N); vm.eval("drop")
    clean(vm.eval("parl tparl backprop drop"))
    g = layer_tensors(vm, "parl", 3)                                      # layer i now holds dX of op i
    a = dict(I=I, F=F, B=B, G=g[2], DF0=np.zeros_like(F), DB0=np.zeros_like(B))
    wdx = witness("float", a, K)[1]
    fw.check("dX", g[1], wdx)
    assert g[1][:, :16].any() and not g[1][:, 16:].any()                  # three rows no patch covers
    assert np.array_equal(g[0], g[1] * (X > 0))                           # ... and the relu in front received it
