"""upsample layers of any factor and method on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so), DESIGN.md 3.17: `n upsample` and
`m n upsample` add the layer, forward / backprop run it through t4k_upsample_fwd / _bwd, one launch each.

The net is `0.5 8 conv2d`, `2 2 upsample` (bilinear x2), `relu`, `3 2 upsample` (bicubic x2), `4 upsample` (nearest x4), `0.5 3 conv2d`.  It runs on a SQUARE
6 x 6 x 3 image, because conv2d takes its W0 from H1 (the reference's quirk) and a rectangular image would hand the convolutions extents
they do not have; the same three upsample layers with the relu between them run on a RECTANGULAR 6 x 5 x 8 tensor in a net without convolutions.  After
`forward` every upsample layer's output is bit-equal to t4k_upsample_fwd on the layer's own fetched input and inside the float64 witness bound on it
(tests/test_gpu_upsample.py's witness: the float-rounded table as the operand).  After `T backprop` every upsample layer's in-place dX (`i n@`) is held
against the float64 transpose applied to the dY the VM itself stored (f64_witness.py's principle: no error is carried from layer to layer).  Launches per
pass do not depend on the batch; a `2 upsample` in the same model still takes its old calls - one forward, two backward; two `nn.sgd` steps lower
`loss.mse`; `save` / `load` round-trip the `.t4` text of the layers."""
import numpy as np
import pytest

import f64_witness as fw
from test_gpu_bcast import Dev
from test_gpu_pool_geo import lcount
from test_gpu_pool_geo_words import layer_tensors, operand
from test_gpu_upsample import BILINEAR, CUBIC, NEAREST, witness

pytestmark = pytest.mark.gpu

NET = "%d 6 6 3 nn.model 0.5 8 conv2d 2 2 upsample relu 3 2 upsample 4 upsample 0.5 3 conv2d"
UPS = {1: (BILINEAR, 2), 3: (CUBIC, 2), 4: (NEAREST, 4)}                 # op -> method, K
SHAPES = [(6, 6, 3), (6, 6, 8), (12, 12, 8), (12, 12, 8), (24, 24, 8), (96, 96, 8), (96, 96, 3)]
NET_R = "%d 6 5 8 nn.model 2 2 upsample relu 3 2 upsample 4 upsample"
UPS_R = {0: (BILINEAR, 2), 2: (CUBIC, 2), 3: (NEAREST, 4)}
SHAPES_R = [(6, 5, 8), (12, 10, 8), (12, 10, 8), (24, 20, 8), (96, 80, 8)]


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def test_network_text_and_shapes(vm):
    vm.eval((NET % 2) + " constant netu")
    txt = vm.eval("netu network drop")
    want = """NN Model[6/128]
[  0] conv2d : T4[2,6,6,3] #p=664 T4[3,3,3,8] T1[8] T4[2,6,6,3] bias=0.5, C=8, K=3, S=1, P=1
[  1] upsampl: T4[2,6,6,8] #p=0 2x2 bilinear
[  2] relu   : T4[2,12,12,8] #p=2304 T4[2,12,12,8] 
[  3] upsampl: T4[2,12,12,8] #p=0 2x2 cubic
[  4] upsampl: T4[2,24,24,8] #p=0 4x4 nearest
[  5] conv2d : T4[2,96,96,8] #p=147894 T4[8,3,3,3] T1[3] T4[2,96,96,8] bias=0.5, C=3, K=3, S=1, P=1
[  6] output : T4[2,96,96,3] #p=0 
"""
    assert want in txt, txt
    vm.eval((NET_R % 2) + " constant netr")
    txt = vm.eval("netr network drop")
    assert "[  0] upsampl: T4[2,6,5,8] #p=0 2x2 bilinear\n" in txt and "[  2] upsampl: T4[2,12,10,8] #p=0 2x2 cubic\n" in txt, txt
    assert "[  3] upsampl: T4[2,24,20,8] #p=0 4x4 nearest\n[  4] output : T4[2,96,80,8] #p=0 \n" in txt, txt


def check_ups(vm, t4k, name, N, ups, shapes, X, T):
    """forward then `T backprop` on net `name`; every upsample layer of `ups` against the entry and the float64 witness"""
    H, W, C = shapes[0]
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    acts = layer_tensors(vm, name, len(shapes))
    assert np.array_equal(acts[0], X)
    for i, s in enumerate(shapes):
        assert acts[i].shape == (N,) + s, (i, acts[i].shape)
    for i, (method, K) in ups.items():
        I, O = acts[i], acts[i + 1]
        _, H1, W1, C = I.shape
        dI, dO = Dev(I), Dev(np.full(O.size, np.nan, np.float32))
        t4k.call("t4k_upsample_fwd", method, dI.p, dO.p, N, H1, W1, C, K * H1, K * W1, K, None)
        assert np.array_equal(dO.get(t4k, O.shape), O), "layer %d" % i
        fw.check("layer %d O" % i, O, witness(t4k, method, K, I, np.zeros_like(O), "float")[0])
    h, w, c = shapes[-1]
    vm.store(T, "%d %d %d %d tensor constant t%s t%s" % (N, h, w, c, name, name)); vm.eval("drop")
    out = vm.eval("%s t%s backprop drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    grads = layer_tensors(vm, name, len(shapes))                        # layer i now holds dX of op i; the last one the loss derivative (the target)
    assert np.array_equal(grads[-1], T)
    for i, (method, K) in ups.items():
        fw.check("layer %d dX" % i, grads[i], witness(t4k, method, K, acts[i], grads[i + 1], "float")[1])
    return acts, grads


def test_forward_and_backprop_layer_by_layer(vm, t4k):
    N = 2
    rng = np.random.default_rng(5)
    vm.eval((NET % N) + " constant netl")
    acts, grads = check_ups(vm, t4k, "netl", N, UPS, SHAPES, operand(rng, N, 6, 6, 3), operand(rng, N, 96, 96, 3))
    assert np.array_equal(acts[3], np.maximum(acts[2], 0))             # the relu between the layers ran as it runs anywhere
    assert np.array_equal(grads[2], grads[3] * (acts[2] > 0))
    assert np.array_equal(acts[5], acts[4].repeat(4, axis=1).repeat(4, axis=2))     # nearest x4: every cell a 4 x 4 tile


def test_the_layers_on_a_rectangular_input(vm, t4k):
    N = 2
    rng = np.random.default_rng(6)
    vm.eval((NET_R % N) + " constant netq")
    acts, grads = check_ups(vm, t4k, "netq", N, UPS_R, SHAPES_R, operand(rng, N, 6, 5, 8), operand(rng, N, 96, 80, 8))
    assert np.array_equal(acts[4], acts[3].repeat(4, axis=1).repeat(4, axis=2))


def test_launches_do_not_depend_on_the_batch(vm, t4k):
    counts = []
    for N in (2, 64):
        name = "netn%d" % N
        rng = np.random.default_rng(9)
        vm.eval((NET % N) + " constant " + name)
        vm.store(operand(rng, N, 6, 6, 3), "%d 6 6 3 tensor constant xn%d xn%d" % (N, N, N)); vm.eval("drop")
        vm.store(operand(rng, N, 96, 96, 3), "%d 96 96 3 tensor constant tn%d tn%d" % (N, N, N)); vm.eval("drop")
        vm.eval("%s xn%d forward tn%d backprop drop" % (name, N, N))
        l0 = lcount(t4k); vm.eval("%s xn%d forward drop" % (name, N)); f = lcount(t4k) - l0
        l0 = lcount(t4k); vm.eval("%s tn%d backprop drop" % (name, N)); b = lcount(t4k) - l0
        counts.append((f, b))
    assert counts[0] == counts[1] and counts[0][0] >= 6 and counts[0][1] >= 6, counts


def test_a_2_upsample_still_takes_its_old_calls(vm, t4k):
    """`2 upsample sigmoid` against the same net with one more layer between the two: a `2 upsample` or a `0 3 upsample` adds the old route's launches - one
    forward (t4k_dpool), two backward (t4k_pool and the scale map) -, a `2 2 upsample` or a `4 upsample` one each way"""
    counts = {}
    nets = {"netf0": ("", 2), "netf1": (" 2 upsample", 4), "netf2": (" 0 3 upsample", 6), "netf3": (" 2 2 upsample", 4), "netf4": (" 4 upsample", 8)}
    for name, (mid, k) in nets.items():
        rng = np.random.default_rng(13)
        vm.eval("2 4 4 3 nn.model 2 upsample" + mid + " sigmoid constant " + name)
        vm.store(operand(rng, 2, 4, 4, 3), "2 4 4 3 tensor constant x%s x%s" % (name, name)); vm.eval("drop")
        vm.store(rng.uniform(0.1, 0.9, size=(2, 4 * k, 4 * k, 3)).astype(np.float32), "2 %d %d 3 tensor constant t%s t%s" % (4 * k, 4 * k, name, name)); vm.eval("drop")
        out = vm.eval("%s x%s forward t%s backprop drop" % (name, name, name))
        assert "not supported" not in out and "failed" not in out, out
        l0 = lcount(t4k); vm.eval("%s x%s forward drop" % (name, name)); f = lcount(t4k) - l0
        l0 = lcount(t4k); vm.eval("%s t%s backprop drop" % (name, name)); b = lcount(t4k) - l0
        counts[name] = (f, b)
    f0, b0 = counts["netf0"]
    assert counts["netf1"] == (f0 + 1, b0 + 2) and counts["netf2"] == (f0 + 1, b0 + 2), counts
    assert counts["netf3"] == (f0 + 1, b0 + 1) and counts["netf4"] == (f0 + 1, b0 + 1), counts
    # the old route computed what it computes - every cell a 2 x 2 tile - and the new layer behind it read that
    vm.eval("netf3 xnetf3 forward drop")
    a = layer_tensors(vm, "netf3", 3)
    assert np.array_equal(a[1], a[0].repeat(2, axis=1).repeat(2, axis=2))
    fw.check("behind the old route", a[2], witness(t4k, BILINEAR, 2, a[1], np.zeros_like(a[2]), "float")[0])


def test_two_sgd_steps_lower_the_loss(vm):
    rng = np.random.default_rng(17)
    vm.eval((NET % 2) + " flatten 10 linear sigmoid constant nets")
    vm.store(operand(rng, 2, 6, 6, 3), "2 6 6 3 tensor constant xs xs"); vm.eval("drop")
    vm.store(rng.uniform(0.1, 0.9, size=(2, 1, 10, 1)).astype(np.float32), "2 1 10 1 tensor constant ts ts"); vm.eval("drop")
    losses = []
    for _ in range(3):
        txt = vm.eval('nets xs forward ts loss.mse ." loss " . ts backprop 0.0001 0.0 nn.sgd drop')
        assert "not supported" not in txt and "failed" not in txt, txt
        losses.append(float(txt.split("loss")[1].split()[0]))
    assert losses[2] < losses[1] < losses[0], losses


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes an upsample layer as `KxK <method>upsampl`; `load` into a net built alike reads the blobs behind that text, and saving that net gives the
    same file, byte for byte"""
    vm.eval((NET % 2) + " 2 upsample constant netv")
    a, b = str(tmp_path / "a.t4"), str(tmp_path / "b.t4")
    vm.eval('netv s" %s" save' % a); vm.eval("drop")
    head = open(a, "rb").read().split(b"\n\n")[0].decode().split("\n")
    assert head == ["\\ tensorForth v4.0 model", "bias=0.5, C=8, K=3, S=1, P=1conv2d ", "2x2 bilinearupsampl", "relu   ", "2x2 cubicupsampl",
                    "4x4 nearestupsampl", "bias=0.5, C=3, K=3, S=1, P=1conv2d ", "2x2 nearestupsampl"], head
    vm.eval((NET % 2) + " 2 upsample constant netw")
    out = vm.eval('netw s" %s" load' % a); out += vm.eval("drop")
    assert "error" not in out, out
    vm.eval('netw s" %s" save' % b); vm.eval("drop")
    assert open(a, "rb").read() == open(b, "rb").read()
    w = vm.fetch("netw 0 nn.w").copy(); vm.eval("drop drop")
    v = vm.fetch("netv 0 nn.w").copy(); vm.eval("drop drop")
    assert np.array_equal(w, v)
