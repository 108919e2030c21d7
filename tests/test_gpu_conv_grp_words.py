"""grouped and depthwise conv2d layers on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so), DESIGN.md 3.18: the fifth cell of
`bias C 5 vector{ K S P D G } conv2d` adds the layer, forward / backprop run it through t4k_conv2d_grp_fwd / _bwd.

The net is a depthwise-separable block on a square 12x12x8 image (conv2d takes W0 from H1): depthwise 3x3, conv1x1, batchnorm, relu, a strided depthwise
{ 3 2 1 1 16 }, a G = 2 layer.  After `forward` every grouped layer's output is bit-equal to t4k_conv2d_grp_fwd on the layer's own fetched input and weights,
and inside the float64 witness bound of torch's conv2d(groups=G) on those operands.  After `T backprop` every grouped layer's `nn.dw`, `nn.db` and in-place
dX (`i n@`) is held against the float64 backward of the operands the VM itself stored (no error is carried from layer to layer) - layer 0's dX with the
lazy plan on and off.  A batch-norm behind a grouped conv runs as a launch of its own and gives, bit for bit, what the stand-alone batch-norm launch gives
behind a dense layer that hands it the same tensor.  Launches per pass do not depend on the batch; a (3,1,1) dense layer in the same model keeps its
specialised engine; three `nn.sgd` steps lower `loss.mse`; `save` / `load` round-trip the `.t4` text and the smaller blobs."""
import numpy as np
import pytest

import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_conv_geo import extent, last_plan, lcount
from test_gpu_conv_grp import witness

pytestmark = pytest.mark.gpu

NET = ("%d 12 12 8 nn.model 0.5 8 5 vector{ 3 1 1 1 8 } conv2d 0.5 16 conv1x1 0.1 batchnorm relu 0.5 16 5 vector{ 3 2 1 1 16 } conv2d "
       "0.5 8 5 vector{ 3 1 1 1 2 } conv2d")
CONVS = {0: (8, 8, 3, 1, 1, 1, 8), 1: (8, 16, 1, 1, 0, 1, 1), 4: (16, 16, 3, 2, 1, 1, 16), 5: (16, 8, 3, 1, 1, 1, 2)}      # op -> C1, C0, K, S, P, D, G
GROUPED = (0, 4, 5)
SHAPES = [(12, 12, 8), (12, 12, 8), (12, 12, 16), (12, 12, 16), (12, 12, 16), (6, 6, 16), (6, 6, 8)]


def operand(rng, *shape):
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def build(vm, name, N, rng, net=NET, convs=CONVS, tail=""):
    """the net as constant `name`, its conv weights from rng (scaled so that the activations keep their size through the layers)"""
    vm.eval((net % N) + tail + " constant " + name)
    Ws = {}
    for i, (C1, C0, K, S, P, D, G) in convs.items():
        Cg1 = C1 // G
        F = operand(rng, Cg1, K, K, C0) / np.float32(K * np.sqrt(Cg1)); B = operand(rng, C0)
        vm.store(F, "%s %d %d %d %d tensor" % (name, Cg1, K, K, C0)); out = vm.eval("%d nn.w=" % i)
        vm.store(B, "%d vector" % C0); out += vm.eval("%d nn.b= drop" % i)
        assert "?" not in out and "shape" not in out, out
        Ws[i] = (F, B)
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
    want = """NN Model[6/128]
[  0] conv2d : T4[2,12,12,8] #p=2464 T4[1,3,3,8] T1[8] T4[2,12,12,8] bias=0.5, C=8, K=3, S=1, P=1, G=8
[  1] conv2d : T4[2,12,12,8] #p=2592 T4[8,1,1,16] T1[16] T4[2,12,12,8] bias=0.5, C=16, K=1, S=1, P=0
"""
    assert want in txt, txt
    assert "[  4] conv2d : T4[2,12,12,16] #p=4928 T4[1,3,3,16] T1[16] T4[2,12,12,16] bias=0.5, C=16, K=3, S=2, P=1, G=16\n" in txt, txt
    assert "[  5] conv2d : T4[2,6,6,16] #p=2320 T4[8,3,3,8] T1[8] T4[2,6,6,16] bias=0.5, C=8, K=3, S=1, P=1, G=2\n" in txt, txt
    assert "[  6] output : T4[2,6,6,8] #p=0 \n" in txt, txt


@pytest.mark.parametrize("lazy", [True, False], ids=["lazy_dx0", "eager_dx0"])
def test_forward_and_backprop_layer_by_layer(vm, t4k, lazy):
    from tensorforth_amd.vm import set_lazy_dx0
    prev = set_lazy_dx0(lazy)
    try:
        N = 2
        name = "netl" if lazy else "nete"
        rng = np.random.default_rng(5)
        Ws = build(vm, name, N, rng)
        X = operand(rng, N, 12, 12, 8)
        vm.store(X, "%d 12 12 8 tensor constant x%s x%s" % (N, name, name)); vm.eval("drop")
        out = vm.eval("%s x%s forward drop" % (name, name))
        assert "not supported" not in out and "failed" not in out, out
        assert last_plan(t4k) == "grp<v4>", last_plan(t4k)              # the last conv entry of the pass: the G = 2 layer, four outputs of one group per thread
        acts = layer_tensors(vm, name, len(SHAPES))
        assert np.array_equal(acts[0], X)
        for i, s in enumerate(SHAPES):
            assert acts[i].shape == (N,) + s, (i, acts[i].shape)
        for i in GROUPED:
            C1, C0, K, S, P, D, G = CONVS[i]
            I, (F, B) = acts[i], Ws[i]
            assert np.array_equal(vm.fetch("%s %d nn.w" % (name, i)), F); vm.eval("drop drop")
            _, H1, W1, _ = I.shape
            H0, W0 = extent(H1, K, S, P, D), extent(W1, K, S, P, D)
            dI, dF, dB, dO = Dev(I), Dev(F), Dev(B), Dev(np.full(acts[i + 1].size, np.nan, np.float32))
            t4k.call("t4k_conv2d_grp_fwd", dI.p, None, dO.p, dF.p, dB.p, N, H1, W1, C1, H0, W0, C0, K, S, P, D, G, None)
            assert np.array_equal(dO.get(t4k, acts[i + 1].shape), acts[i + 1]), "layer %d" % i
            a = dict(I=I, F=F, B=B, G=np.zeros_like(acts[i + 1]), DF0=np.zeros_like(F), DB0=np.zeros_like(B))
            fw.check("layer %d O" % i, acts[i + 1], witness("float", a, K, S, P, D, G)[0])
        assert np.array_equal(acts[4], np.maximum(acts[3], 0))             # the relu in front of the strided depthwise layer ran as it runs anywhere
        T = operand(rng, *acts[-1].shape)
        vm.store(T, "%d %d %d %d tensor constant t%s t%s" % (acts[-1].shape + (name, name))); vm.eval("drop")
        out = vm.eval("%s t%s backprop drop" % (name, name))
        assert "not supported" not in out and "failed" not in out, out
        grads = layer_tensors(vm, name, len(SHAPES))                    # layer i now holds dX of op i; the last one the loss derivative (the target)
        assert np.array_equal(grads[-1], T)
        for i in GROUPED:
            C1, C0, K, S, P, D, G = CONVS[i]
            F, B = Ws[i]
            a = dict(I=acts[i], F=F, B=B, G=grads[i + 1], DF0=np.zeros_like(F), DB0=np.zeros_like(B))
            _, wdx, wdf, wdb = witness("float", a, K, S, P, D, G)
            fw.check("layer %d dX" % i, grads[i], wdx)
            dw = vm.fetch("%s %d nn.dw" % (name, i)).copy(); vm.eval("drop drop")
            assert dw.shape == F.shape
            fw.check("layer %d dF" % i, dw, wdf)
            fw.check("layer %d dB" % i, vm.fetch("%s %d nn.db" % (name, i)), wdb); vm.eval("drop drop")
            # ... and the in-place dX is bit-equal to the entry's on the same operands
            _, H1, W1, _ = acts[i].shape
            dI, dG, dF, dDX = Dev(acts[i]), Dev(grads[i + 1]), Dev(F), Dev(np.full(acts[i].size, np.nan, np.float32))
            t4k.call("t4k_conv2d_grp_bwd", dI.p, dG.p, dDX.p, None, dF.p, None, None, N, H1, W1, C1, grads[i + 1].shape[1], grads[i + 1].shape[2], C0, K, S, P, D, G, 0, None)
            assert np.array_equal(dDX.get(t4k, acts[i].shape), grads[i]), "layer %d dX" % i
    finally:
        set_lazy_dx0(prev)


def test_batchnorm_behind_a_grouped_conv(vm, t4k):
    """`depthwise conv2d, batchnorm`: launches of their own (no statistics ride in the grouped kernel's epilogue: its plan has one token), and the batch-norm output is what the
    stand-alone batch-norm launch gives behind a dense conv1x1 with the identity filter, which hands it the same tensor (every layer a call of its own
    under `1 trace`)"""
    N = 2
    rng = np.random.default_rng(7)
    net = "%d 12 12 8 nn.model 0.5 8 5 vector{ 3 1 1 1 8 } conv2d 0.1 batchnorm"
    build(vm, "netb", N, rng, net=net, convs={0: CONVS[0]})
    X = operand(rng, N, 12, 12, 8)
    vm.store(X, "%d 12 12 8 tensor constant xb xb" % N); vm.eval("drop")
    vm.eval("netb xb forward drop")
    l0 = lcount(t4k); out = vm.eval("netb xb forward drop"); f = lcount(t4k) - l0
    assert "failed" not in out and f >= 2 and last_plan(t4k) == "memcpy grp_dw<v4>", (out, f, last_plan(t4k))     # the layer-0 copy is a copy command
    _, Y, Z = layer_tensors(vm, "netb", 3)
    vm.eval((("%d 12 12 8 nn.model 0.5 8 conv1x1 0.1 batchnorm") % N) + " constant netd")
    eye = np.zeros((8, 1, 1, 8), np.float32); eye[np.arange(8), 0, 0, np.arange(8)] = 1.0
    vm.store(eye, "netd 8 1 1 8 tensor"); out = vm.eval("0 nn.w=")
    vm.store(np.zeros(8, np.float32), "8 vector"); out += vm.eval("0 nn.b= drop")
    assert "?" not in out and "shape" not in out, out
    vm.store(Y, "%d 12 12 8 tensor constant yb yb" % N); vm.eval("drop")
    vm.eval("1 trace netd yb forward drop 0 trace")
    _, Y2, Z2 = layer_tensors(vm, "netd", 3)
    assert np.array_equal(Y2, Y)                                         # 1 * y + 0 * the others + 0: the dense layer hands the same tensor on
    assert np.array_equal(Z2, Z)


def test_launches_do_not_depend_on_the_batch(vm, t4k):
    """the three grouped layers alone: one launch each forward (the layer-0 copy is a copy command); backward slabs, fold and dX each, but layer 0's dX, which
    the lazy plan leaves for the word that asks - whatever the batch"""
    net = "%d 12 12 8 nn.model 0.5 8 5 vector{ 3 1 1 1 8 } conv2d 0.5 16 5 vector{ 3 2 1 1 8 } conv2d 0.5 8 5 vector{ 3 1 1 1 2 } conv2d"
    convs = {0: CONVS[0], 1: (8, 16, 3, 2, 1, 1, 8), 2: CONVS[5]}
    counts = []
    for N in (2, 64):
        name = "netn%d" % N
        rng = np.random.default_rng(9)
        build(vm, name, N, rng, net=net, convs=convs)
        vm.store(operand(rng, N, 12, 12, 8), "%d 12 12 8 tensor constant xn%d xn%d" % (N, N, N)); vm.eval("drop")
        vm.store(operand(rng, N, 6, 6, 8), "%d 6 6 8 tensor constant tn%d tn%d" % (N, N, N)); vm.eval("drop")
        out = vm.eval("%s xn%d forward tn%d backprop drop" % (name, N, N))
        assert "not supported" not in out and "failed" not in out, out
        l0 = lcount(t4k); vm.eval("%s xn%d forward drop" % (name, N)); f = lcount(t4k) - l0
        l0 = lcount(t4k); vm.eval("%s tn%d backprop drop" % (name, N)); b = lcount(t4k) - l0
        counts.append((f, b))
    assert counts[0] == counts[1] and counts[0][0] == 3 and counts[0][1] in (8, 9), counts


def test_a_3_1_1_dense_layer_keeps_its_engine(vm, t4k):
    rng = np.random.default_rng(13)
    Ws = build(vm, "netm", 2, rng, tail=" 0.5 4 conv2d")
    vm.store(operand(rng, 2, 12, 12, 8), "2 12 12 8 tensor constant xm xm"); vm.eval("drop")
    out = vm.eval("netm xm forward drop")
    assert "not supported" not in out and "failed" not in out, out
    vm.eval("1 trace netm xm forward drop 0 trace")                      # under trace every layer is a call of its own: the last conv entry is the (3,1,1) layer's
    p = last_plan(t4k)
    assert p.startswith(("few<", "thin", "gather<", "big<", "big8<")) and "grp" not in p and "geo" not in p, p     # one of t4k_conv2d_fwd's own engines
    txt = vm.eval("netm network drop")
    assert "T4[8,3,3,4] T1[4] T4[2,6,6,8] bias=0.5, C=4, K=3, S=1, P=1\n" in txt, txt
    # ... and a fifth cell of 1 builds that same dense layer
    vm.eval((NET % 2) + " 0.5 4 5 vector{ 3 1 1 1 1 } conv2d constant netm1")
    assert "T4[8,3,3,4] T1[4] T4[2,6,6,8] bias=0.5, C=4, K=3, S=1, P=1\n" in vm.eval("netm1 network drop")


def test_three_sgd_steps_lower_the_loss(vm):
    rng = np.random.default_rng(17)
    build(vm, "nets", 2, rng, tail=" flatten 10 linear sigmoid")
    vm.store(operand(rng, 2, 12, 12, 8), "2 12 12 8 tensor constant xs xs"); vm.eval("drop")
    vm.store(rng.uniform(0.1, 0.9, size=(2, 1, 10, 1)).astype(np.float32), "2 1 10 1 tensor constant ts ts"); vm.eval("drop")
    losses = []
    for _ in range(4):
        txt = vm.eval('nets xs forward ts loss.mse ." loss " . ts backprop 0.001 0.0 nn.sgd drop')
        assert "not supported" not in txt and "failed" not in txt, txt
        losses.append(float(txt.split("loss")[1].split()[0]))
    assert losses[3] < losses[2] < losses[1] < losses[0], losses


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes a grouped layer's line with `, G=<g>` and the SMALLER filter blob; `load` into a net built alike reads the blobs behind that text, and
    saving that net gives the same file, byte for byte"""
    rng = np.random.default_rng(19)
    build(vm, "netv", 2, rng)
    a, b = str(tmp_path / "a.t4"), str(tmp_path / "b.t4")
    vm.eval('netv s" %s" save' % a); vm.eval("drop")
    head = open(a, "rb").read().split(b"\n\n")[0].decode().split("\n")
    assert head[0] == "\\ tensorForth v4.0 model" and head[1] == "bias=0.5, C=8, K=3, S=1, P=1, G=8conv2d " and head[2] == "bias=0.5, C=16, K=1, S=1, P=0conv2d ", head
    assert head[5] == "bias=0.5, C=16, K=3, S=2, P=1, G=16conv2d " and head[6] == "bias=0.5, C=8, K=3, S=1, P=1, G=2conv2d ", head
    vm.eval((NET % 2) + " constant netw")
    out = vm.eval('netw s" %s" load' % a); out += vm.eval("drop")
    assert "error" not in out, out
    vm.eval('netw s" %s" save' % b); vm.eval("drop")
    assert open(a, "rb").read() == open(b, "rb").read()
    for i in GROUPED:
        w = vm.fetch("netw %d nn.w" % i).copy(); vm.eval("drop drop")
        v = vm.fetch("netv %d nn.w" % i).copy(); vm.eval("drop drop")
        assert w.shape == (CONVS[i][0] // CONVS[i][6], 3, 3, CONVS[i][1]) and np.array_equal(w, v), i
