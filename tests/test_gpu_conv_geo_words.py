"""conv2d layers of any K 1..7 with stride, padding and dilation on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so), DESIGN.md 3.15:
`bias C 4 vector{ K S P D } conv2d` adds the layer, forward / backprop run it through t4k_conv2d_geo_fwd / _bwd.

A conv-only net on a square input, weights set with `nn.w=` / `nn.b=`.  After `forward` every layer's output is bit-equal to t4k_conv2d_geo_fwd on the
layer's own fetched input and weights, and inside the float64 witness bound of torch on those operands.  After `T backprop` every layer's `nn.dw`,
`nn.db` and in-place dX (`i n@`) is held against the float64 backward of the operands the VM itself stored (f64_witness.py's principle: no error is
carried from layer to layer) - layer 0's dX with the lazy plan on and off.  Launches per pass do not depend on the batch; a (3,1,1) layer in the same
model keeps its specialised engine; three `nn.sgd` steps lower `loss.mse`."""

import numpy as np
import pytest

import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_conv_geo import extent, last_plan, lcount, witness

pytestmark = pytest.mark.gpu

LAYERS = [(8, 3, 2, 1, 1), (8, 3, 1, 2, 2), (4, 7, 2, 3, 1)]            # C0, K, S, P, D
NET = "%d 12 12 3 nn.model " + " ".join("0.5 %d 4 vector{ %d %d %d %d } conv2d" % l for l in LAYERS)


def operand(rng, *shape):
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def build(vm, name, N, rng, tail=""):
    """the net as constant `name`, its weights from rng (scaled so that the activations keep their size through the layers)"""
    vm.eval((NET % N) + tail + " constant " + name)
    C1, Ws = 3, []
    for i, (C0, K, S, P, D) in enumerate(LAYERS):
        F = operand(rng, C1, K, K, C0) / np.float32(K * np.sqrt(C1)); B = operand(rng, C0)
        vm.store(F, "%s %d %d %d %d tensor" % (name, C1, K, K, C0)); out = vm.eval("%d nn.w=" % i)
        vm.store(B, "%d vector" % C0); out += vm.eval("%d nn.b= drop" % i)
        assert "?" not in out and "shape" not in out, out
        Ws.append((F, B)); C1 = C0
    return Ws


def layer_tensors(vm, name, n):
    out = []
    for i in range(n):
        out.append(vm.fetch("%s %d n@" % (name, i)).copy()); vm.eval("drop drop")
    return out


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def test_network_text_and_shapes(vm):
    build(vm, "netp", 2, np.random.default_rng(1))
    txt = vm.eval("netp network drop")
    assert "K=3, S=2, P=1\n" in txt and "K=3, S=1, P=2, D=2\n" in txt and "K=7, S=2, P=3\n" in txt, txt
    assert "T4[2,6,6,8]" in txt and "T4[2,3,3,4]" in txt


@pytest.mark.parametrize("lazy", [True, False], ids=["lazy_dx0", "eager_dx0"])
def test_forward_and_backprop_layer_by_layer(vm, t4k, lazy):
    from tensorforth_amd.vm import set_lazy_dx0
    prev = set_lazy_dx0(lazy)
    try:
        N = 2
        name = "netl" if lazy else "nete"
        rng = np.random.default_rng(5)
        Ws = build(vm, name, N, rng)
        X = operand(rng, N, 12, 12, 3)
        vm.store(X, "%d 12 12 3 tensor constant x%s x%s" % (N, name, name)); vm.eval("drop")
        vm.eval("%s x%s forward drop" % (name, name))
        assert last_plan(t4k).startswith("geo<"), last_plan(t4k)
        acts = layer_tensors(vm, name, len(LAYERS) + 1)
        assert np.array_equal(acts[0], X)
        for i, (C0, K, S, P, D) in enumerate(LAYERS):
            I, (F, B) = acts[i], Ws[i]
            assert np.array_equal(vm.fetch("%s %d nn.w" % (name, i)), F); vm.eval("drop drop")
            _, H1, W1, C1 = I.shape
            H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
            assert acts[i + 1].shape == (N, H0, W0, C0)
            dI, dF, dB, dO = Dev(I), Dev(F), Dev(B), Dev(np.full(acts[i + 1].size, np.nan, np.float32))
            t4k.call("t4k_conv2d_geo_fwd", dI.p, None, dO.p, dF.p, dB.p, N, H1, W1, C1, H0, W0, C0, K, S, P, D, None)
            assert np.array_equal(dO.get(t4k, acts[i + 1].shape), acts[i + 1]), "layer %d" % i
            a = dict(I=I, F=F, B=B, G=np.zeros_like(acts[i + 1]), DF0=np.zeros_like(F), DB0=np.zeros_like(B))
            fw.check("layer %d O" % i, acts[i + 1], witness("float", a, K, S, P, D)[0])
        T = operand(rng, *acts[-1].shape)
        vm.store(T, "%d %d %d %d tensor constant t%s t%s" % (acts[-1].shape + (name, name))); vm.eval("drop")
        vm.eval("%s t%s backprop drop" % (name, name))
        grads = layer_tensors(vm, name, len(LAYERS) + 1)                # layer i now holds dX of op i; the last one the loss derivative (the target)
        assert np.array_equal(grads[-1], T)
        for i, (C0, K, S, P, D) in enumerate(LAYERS):
            F, B = Ws[i]
            a = dict(I=acts[i], F=F, B=B, G=grads[i + 1], DF0=np.zeros_like(F), DB0=np.zeros_like(B))
            _, wdx, wdf, wdb = witness("float", a, K, S, P, D)
            fw.check("layer %d dX" % i, grads[i], wdx)
            fw.check("layer %d dF" % i, vm.fetch("%s %d nn.dw" % (name, i)), wdf); vm.eval("drop drop")
            fw.check("layer %d dB" % i, vm.fetch("%s %d nn.db" % (name, i)), wdb); vm.eval("drop drop")
    finally:
        set_lazy_dx0(prev)


def test_launches_do_not_depend_on_the_batch(vm, t4k):
    counts = []
    for N in (2, 64):
        name = "netn%d" % N
        rng = np.random.default_rng(9)
        build(vm, name, N, rng)
        vm.store(operand(rng, N, 12, 12, 3), "%d 12 12 3 tensor constant xn%d xn%d" % (N, N, N)); vm.eval("drop")
        vm.store(operand(rng, N, 3, 3, 4), "%d 3 3 4 tensor constant tn%d tn%d" % (N, N, N)); vm.eval("drop")
        step = "%s xn%d forward tn%d backprop drop" % (name, N, N)
        vm.eval(step)
        l0 = lcount(t4k); vm.eval("%s xn%d forward drop" % (name, N)); f = lcount(t4k) - l0
        l0 = lcount(t4k); vm.eval("%s tn%d backprop drop" % (name, N)); b = lcount(t4k) - l0
        counts.append((f, b))
    assert counts[0] == counts[1] and counts[0][0] >= 3 and counts[0][1] >= 3, counts


def test_a_3_1_1_layer_keeps_its_engine(vm, t4k):
    rng = np.random.default_rng(13)
    build(vm, "netm", 2, rng, tail=" 0.5 4 conv2d")
    vm.store(operand(rng, 2, 12, 12, 3), "2 12 12 3 tensor constant xm xm"); vm.eval("drop")
    out = vm.eval("netm xm forward drop")
    assert "not supported" not in out and "failed" not in out, out
    acts = layer_tensors(vm, "netm", 5)
    F = vm.fetch("netm 3 nn.w").copy(); vm.eval("drop drop")
    B = vm.fetch("netm 3 nn.b").copy().ravel(); vm.eval("drop drop")
    a = dict(I=acts[3], F=F, B=B, G=np.zeros_like(acts[4]), DF0=np.zeros_like(F), DB0=np.zeros_like(B))
    fw.check("the (3,1,1) layer behind the three", acts[4], witness("float", a, 3, 1, 1, 1)[0])
    vm.eval("1 trace netm xm forward drop 0 trace")                      # under trace every layer is a call of its own: the last conv entry is the (3,1,1) layer's
    p = last_plan(t4k)
    assert p.startswith(("few<", "thin", "gather<", "big<", "big8<")) and "geo" not in p, p     # one of t4k_conv2d_fwd's own engines (include/t4k.h lists them)
    txt = vm.eval("netm network drop")
    assert "K=3, S=1, P=1\n" in txt and txt.count("T4[2,3,3,4]") >= 2, txt


def test_three_sgd_steps_lower_the_loss(vm):
    rng = np.random.default_rng(17)
    build(vm, "nets", 2, rng, tail=" flatten 10 linear sigmoid")
    vm.store(operand(rng, 2, 12, 12, 3), "2 12 12 3 tensor constant xs xs"); vm.eval("drop")
    vm.store(rng.uniform(0.1, 0.9, size=(2, 1, 10, 1)).astype(np.float32), "2 1 10 1 tensor constant ts ts"); vm.eval("drop")
    losses = []
    for _ in range(4):
        txt = vm.eval('nets xs forward ts loss.mse ." loss " . ts backprop 0.02 0.0 nn.sgd drop')
        assert "not supported" not in txt and "failed" not in txt, txt
        losses.append(float(txt.split("loss")[1].split()[0]))
    assert losses[3] < losses[2] < losses[1] < losses[0], losses
