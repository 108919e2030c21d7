"""pooling layers of any K 1..16 with stride and padding on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so), DESIGN.md 3.16:
`vector{ K S P } maxpool | avgpool | minpool` adds the layer, forward / backprop run it through t4k_pool_geo_fwd / _bwd.

The net is a 7x7 / 2 stem convolution with the 3x3 / 2, P 1 max-pool behind it, a relu, an overlapping 2x2 / 1, P 1 min-pool and a 4x4 / 2 avg-pool; a second
net on a RECTANGULAR input ends in a global avg-pool whose K is its input extent.  After `forward` every pool layer's output is bit-equal to
t4k_pool_geo_fwd on the layer's own fetched input and inside the float64 witness bound of torch on it.  After `T backprop` every pool layer's in-place
dX (`i n@`) is held against the float64 backward of the tensors the VM itself stored (f64_witness.py's principle: no error is carried from layer to
layer).  Launches per pass do not depend on the batch; a `2 maxpool` in the same model still rides in its fused run; three `nn.sgd` steps lower
`loss.mse`; `save` / `load` round-trip the `.t4` text of the layers."""
import numpy as np
import pytest

import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_pool_geo import KINDS, code_dev, extent, lcount, witness

pytestmark = pytest.mark.gpu

# the square net (the conv2d layer takes its W0 from H1 - the reference's quirk - so the stem wants a square image): 24 -> 12 -> 6 -> 6 -> 7 -> 2
NET = "%d 24 24 3 nn.model 0.5 8 4 vector{ 7 2 3 1 } conv2d 3 vector{ 3 2 1 } maxpool relu 3 vector{ 2 1 1 } minpool 2 vector{ 4 2 } avgpool"
POOLS = {1: ("max", 3, 2, 1), 3: ("min", 2, 1, 1), 4: ("avg", 4, 2, 0)}             # op -> layer kind, K, S, P
SHAPES = [(24, 24, 3), (12, 12, 8), (6, 6, 8), (6, 6, 8), (7, 7, 8), (2, 2, 8)]
# the rectangular net: 12 x 11 -> 6 x 6 (both extents give 6 under 3x3 / 2, P 1) -> relu -> the global 6x6 average -> 1 x 1
NET_G = "%d 12 11 3 nn.model 3 vector{ 3 2 1 } maxpool relu 1 vector{ 6 } avgpool"
POOLS_G = {0: ("max", 3, 2, 1), 2: ("avg", 6, 6, 0)}
SHAPES_G = [(12, 11, 3), (6, 6, 3), (6, 6, 3), (1, 1, 3)]


def operand(rng, *shape):
    return (rng.uniform(0.5, 2.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def set_conv0(vm, name, rng, C1=3, K=7, C0=8):
    F = operand(rng, C1, K, K, C0) / np.float32(K * np.sqrt(C1)); B = operand(rng, C0)
    vm.store(F, "%s %d %d %d %d tensor" % (name, C1, K, K, C0)); out = vm.eval("0 nn.w=")
    vm.store(B, "%d vector" % C0); out += vm.eval("0 nn.b= drop")
    assert "?" not in out and "shape" not in out, out


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
    vm.eval((NET % 2) + " constant netp")
    txt = vm.eval("netp network drop")
    want = """NN Model[5/128]
[  0] conv2d : T4[2,24,24,3] #p=5824 T4[3,7,7,8] T1[8] T4[2,24,24,3] bias=0.5, C=8, K=7, S=2, P=3
[  1] maxpool: T4[2,12,12,8] #p=144 T4[2,6,6,2] 3x3, S=2, P=1
[  2] relu   : T4[2,6,6,8] #p=576 T4[2,6,6,8] 
[  3] minpool: T4[2,6,6,8] #p=196 T4[2,7,7,2] 2x2, S=1, P=1
[  4] avgpool: T4[2,7,7,8] #p=0 4x4, S=2, P=0
[  5] output : T4[2,2,2,8] #p=0 
"""
    assert want in txt, txt
    vm.eval((NET_G % 2) + " constant netq")
    txt = vm.eval("netq network drop")
    assert "[  0] maxpool: T4[2,12,11,3] #p=72 T4[2,6,6,1] 3x3, S=2, P=1\n" in txt and "[  2] avgpool: T4[2,6,6,3] #p=0 6x6, S=6, P=0\n" in txt, txt
    assert "[  3] output : T4[2,1,1,3] #p=0 \n" in txt, txt


def check_pools(vm, t4k, name, N, pools, shapes, X, T):
    """forward then `T backprop` on net `name`; every pool layer of `pools` against the entry and the float64 witness"""
    H, W, C = shapes[0]
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    acts = layer_tensors(vm, name, len(shapes))
    assert np.array_equal(acts[0], X)
    for i, s in enumerate(shapes):
        assert acts[i].shape == (N,) + s, (i, acts[i].shape)
    zero = {}
    for i, (layer, K, S, P) in pools.items():
        I, O = acts[i], acts[i + 1]
        _, H1, W1, C = I.shape
        H0, W0 = extent(H1, K, S, P), extent(W1, K, S, P)
        assert O.shape == (N, H0, W0, C)
        dI, dO, dC = Dev(I), Dev(np.full(O.size, np.nan, np.float32)), code_dev(N, H0, W0, C)
        t4k.call("t4k_pool_geo_fwd", KINDS[layer], dI.p, dO.p, dC.p, N, H1, W1, C, H0, W0, K, S, P, None)
        assert np.array_equal(dO.get(t4k, O.shape), O), "layer %d" % i
        zero[i] = np.zeros_like(O)
        fw.check("layer %d O" % i, O, witness(layer, "float", I, zero[i], K, S, P)[0])
    h, w, c = shapes[-1]
    vm.store(T, "%d %d %d %d tensor constant t%s t%s" % (N, h, w, c, name, name)); vm.eval("drop")
    out = vm.eval("%s t%s backprop drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    grads = layer_tensors(vm, name, len(shapes))                        # layer i now holds dX of op i; the last one the loss derivative (the target)
    assert np.array_equal(grads[-1], T)
    for i, (layer, K, S, P) in pools.items():
        fw.check("layer %d dX" % i, grads[i], witness(layer, "float", acts[i], grads[i + 1], K, S, P)[1])
    return acts, grads


def test_forward_and_backprop_layer_by_layer(vm, t4k):
    N = 2
    rng = np.random.default_rng(5)
    vm.eval((NET % N) + " constant netl")
    set_conv0(vm, "netl", rng)
    acts, grads = check_pools(vm, t4k, "netl", N, POOLS, SHAPES, operand(rng, N, 24, 24, 3), operand(rng, N, 2, 2, 8))
    assert np.array_equal(acts[3], np.maximum(acts[2], 0))             # the relu between the pools ran as it runs anywhere
    assert np.array_equal(grads[2], grads[3] * (acts[2] > 0))


def test_global_pool_on_a_rectangular_input(vm, t4k):
    N = 2
    rng = np.random.default_rng(6)
    vm.eval((NET_G % N) + " constant netg")
    acts, grads = check_pools(vm, t4k, "netg", N, POOLS_G, SHAPES_G, operand(rng, N, 12, 11, 3), operand(rng, N, 1, 1, 3))
    # the global average: every cell of an image's channel gets dY / 36
    want = np.broadcast_to(grads[3] / np.float32(36), grads[2].shape)
    assert np.array_equal(grads[2], want)


def test_launches_do_not_depend_on_the_batch(vm, t4k):
    counts = []
    for N in (2, 64):
        name = "netn%d" % N
        rng = np.random.default_rng(9)
        vm.eval((NET % N) + " constant " + name)
        set_conv0(vm, name, rng)
        vm.store(operand(rng, N, 24, 24, 3), "%d 24 24 3 tensor constant xn%d xn%d" % (N, N, N)); vm.eval("drop")
        vm.store(operand(rng, N, 2, 2, 8), "%d 2 2 8 tensor constant tn%d tn%d" % (N, N, N)); vm.eval("drop")
        vm.eval("%s xn%d forward tn%d backprop drop" % (name, N, N))
        l0 = lcount(t4k); vm.eval("%s xn%d forward drop" % (name, N)); f = lcount(t4k) - l0
        l0 = lcount(t4k); vm.eval("%s tn%d backprop drop" % (name, N)); b = lcount(t4k) - l0
        counts.append((f, b))
    assert counts[0] == counts[1] and counts[0][0] >= 5 and counts[0][1] >= 5, counts


def test_a_2_maxpool_still_rides_in_its_fused_run(vm, t4k):
    """`0.5 8 conv2d relu 2 maxpool sigmoid`: relu and the 2x2 pool are a fused run.  Two geometry pools between that run and the sigmoid add exactly one
    launch each, each way - the group finder neither takes them into a run nor breaks the run in front of them"""
    counts = {}
    for name, mid, shape in (("netf0", "", (6, 6, 8)), ("netf2", " 3 vector{ 3 2 1 } maxpool 1 vector{ 3 } avgpool", (1, 1, 8))):
        rng = np.random.default_rng(13)
        vm.eval("2 12 12 3 nn.model 0.5 8 conv2d relu 2 maxpool" + mid + " sigmoid constant " + name)
        vm.store(operand(rng, 2, 12, 12, 3), "2 12 12 3 tensor constant x%s x%s" % (name, name)); vm.eval("drop")
        vm.store(rng.uniform(0.1, 0.9, size=(2,) + shape).astype(np.float32), "2 %d %d %d tensor constant t%s t%s" % (shape + (name, name))); vm.eval("drop")
        out = vm.eval("%s x%s forward t%s backprop drop" % (name, name, name))
        assert "not supported" not in out and "failed" not in out, out
        l0 = lcount(t4k); vm.eval("%s x%s forward drop" % (name, name)); f = lcount(t4k) - l0
        l0 = lcount(t4k); vm.eval("%s t%s backprop drop" % (name, name)); b = lcount(t4k) - l0
        counts[name] = (f, b)
    assert counts["netf2"] == (counts["netf0"][0] + 2, counts["netf0"][1] + 2), counts
    txt = vm.eval("netf2 network drop")
    assert "[  2] maxpool: T4[2,12,12,8] #p=0 2x2\n" in txt and "[  3] maxpool: T4[2,6,6,8] #p=36 T4[2,3,3,2] 3x3, S=2, P=1\n" in txt, txt
    # the fused run computed what its layers compute - the 2x2 max of the relu of the conv output - and the geometry pool behind it read that
    vm.eval("netf2 xnetf2 forward drop")
    a = layer_tensors(vm, "netf2", 5)
    assert np.array_equal(a[3], np.maximum(a[1], 0).reshape(2, 6, 2, 6, 2, 8).max(axis=(2, 4)))
    fw.check("behind the run", a[4], witness("max", "float", a[3], np.zeros_like(a[4]), 3, 2, 1)[0])


def test_three_sgd_steps_lower_the_loss(vm):
    rng = np.random.default_rng(17)
    vm.eval((NET % 2) + " flatten 10 linear sigmoid constant nets")
    set_conv0(vm, "nets", rng)
    vm.store(operand(rng, 2, 24, 24, 3), "2 24 24 3 tensor constant xs xs"); vm.eval("drop")
    vm.store(rng.uniform(0.1, 0.9, size=(2, 1, 10, 1)).astype(np.float32), "2 1 10 1 tensor constant ts ts"); vm.eval("drop")
    losses = []
    for _ in range(4):
        txt = vm.eval('nets xs forward ts loss.mse ." loss " . ts backprop 0.02 0.0 nn.sgd drop')
        assert "not supported" not in txt and "failed" not in txt, txt
        losses.append(float(txt.split("loss")[1].split()[0]))
    assert losses[3] < losses[2] < losses[1] < losses[0], losses


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes a marked layer as `KxK, S=<s>, P=<p><name>`; `load` into a net built alike reads the blobs behind that text, and saving that net
    gives the same file, byte for byte"""
    rng = np.random.default_rng(19)
    vm.eval((NET % 2) + " 2 maxpool constant netv")
    set_conv0(vm, "netv", rng)
    a, b = str(tmp_path / "a.t4"), str(tmp_path / "b.t4")
    vm.eval('netv s" %s" save' % a); vm.eval("drop")
    head = open(a, "rb").read().split(b"\n\n")[0].decode().split("\n")
    assert head == ["\\ tensorForth v4.0 model", "bias=0.5, C=8, K=7, S=2, P=3conv2d ", "3x3, S=2, P=1maxpool", "relu   ", "2x2, S=1, P=1minpool",
                    "4x4, S=2, P=0avgpool", "2x2maxpool"], head
    vm.eval((NET % 2) + " 2 maxpool constant netw")
    out = vm.eval('netw s" %s" load' % a); out += vm.eval("drop")
    assert "error" not in out, out
    vm.eval('netw s" %s" save' % b); vm.eval("drop")
    assert open(a, "rb").read() == open(b, "rb").read()
    w = vm.fetch("netw 0 nn.w").copy(); vm.eval("drop drop")
    v = vm.fetch("netv 0 nn.w").copy(); vm.eval("drop drop")
    assert np.array_equal(w, v)
