"""`vector{ V E pos } upsample`, the embedding layer, on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so).

Two nets, each closed with `flatten 10 linear softmax`: a token net - ids in a `N 4 4 1` input, an 11-row table of 8 floats plus learned positions, then a
1x1 projection, attention and a 1x1 projection - and a position net, a 4x4 stride-4 patch convolution on `N 8 8 3` with the position table behind it.  TABLE
and POS are set through the write-through views of `nn.w` / `nn.b`.  After `forward` the layer's output is bit-equal to t4k_embed_fwd on the layer's own
fetched input, and to the NumPy float32 rule; after `T backprop` `nn.dw` (dTABLE) and `nn.db` (dPOS) are bit-equal to t4k_embed_bwd on the dY the layer
received (read from the model) and inside the float64 witness of tests/embed_witness.py; the id tensor is unchanged by `backprop`, the position layer's
input holds dX = dY.  The layer's launches are the plan's, counted as the difference between two nets that differ by the layer alone.  `nn.sgd` and
`nn.adam` steps move TABLE and POS; the `.t4` round trip gives the same forward bits."""
import ctypes

import numpy as np
import pytest

import embed_witness as ew
from test_gpu_bcast import Dev
from test_gpu_pool_geo import lcount
from test_gpu_pool_geo_words import layer_tensors, operand

pytestmark = pytest.mark.gpu

F = np.float32
TAIL = " 0.5 24 conv1x1  2 vector{ 2 %d } linear  0.5 8 conv1x1 flatten 10 linear softmax"
# name: (input shape H W C, words, index of the embed layer, V, E, L, layers)
NETS = {
    "tok": ((4, 4, 1), "3 vector{ 11 8 1 } upsample" + TAIL % 1, 0, 11, 8, 16, 7),
    "pos": ((8, 8, 3), "0.5 8 3 vector{ 4 4 0 } conv2d  3 vector{ 0 0 1 } upsample" + TAIL % 0, 1, 0, 8, 4, 8),
}


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def nan(k):
    return np.full(k, np.nan, F)


def bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).ravel().view(np.uint32), np.ascontiguousarray(b, F).ravel().view(np.uint32))


def put(vm, name, i, word, a):
    vm.store(a, "%s %d %s" % (name, i, word)); vm.eval("drop drop")


def get(vm, name, i, word):
    a = vm.fetch("%s %d %s" % (name, i, word)).copy(); vm.eval("drop drop")
    return a


def build(vm, name, net, N, rng):
    (H, W, C), words, k, V, E, L, _ = NETS[net]
    out = vm.eval("%d %d %d %d nn.model %s constant %s" % (N, H, W, C, words, name))
    assert "nn#iembed" not in out and "required" not in out, out
    TAB = rng.normal(0.0, 1.0, (V, E)).astype(F) if V else None
    POS = rng.normal(0.0, 0.5, (L, E)).astype(F)
    if V:
        put(vm, name, k, "nn.w", TAB)
    put(vm, name, k, "nn.b", POS)
    return TAB, POS


def inputs(net, N, rng):
    (H, W, C), _, _, V, _, _, _ = NETS[net]
    if V:
        X = ew.make_ids(rng, N * H * W, V, "mixed").reshape(N, H, W, 1)
        X.ravel()[:3] = (0.75, V - 0.25, -1.0)
        return X
    return operand(rng, N, H, W, C)


def entries(t4k, x, TAB, POS, dy, V, E, L):
    T = dy.size // E
    dX, dDY, dP, dO = Dev(x), Dev(dy), Dev(POS), Dev(nan(T * E))
    dT = Dev(TAB) if V else None
    dDT, dDP, dDX = (Dev(np.zeros(V * E, F)) if V else None), Dev(np.zeros(L * E, F)), (None if V else Dev(nan(T * E)))
    p = lambda d: d.p if d is not None else None
    t4k.call("t4k_embed_fwd", dX.p if V else None, None if V else dX.p, p(dT), dP.p, dO.p, T, L, V, E, None)
    t4k.call("t4k_embed_bwd", dX.p if V else None, dDY.p, p(dDT), dDP.p, p(dDX), T, L, V, E, 1, None)
    return (dO.get(t4k, (T, E)).copy(), dDT.get(t4k, (V, E)).copy() if V else None, dDP.get(t4k, (L, E)).copy(), dDX.get(t4k, (T, E)).copy() if dDX else None)


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("N", [2, 64])
def test_the_layer_inside_a_net(vm, t4k, N, net):
    name = "em%s%d" % (net, N)
    rng = np.random.default_rng(5 + N + len(net))
    (H, W, C), _, k, V, E, L, nl = NETS[net]
    TAB, POS = build(vm, name, net, N, rng)
    X = inputs(net, N, rng)
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    acts = layer_tensors(vm, name, nl + 1)
    tg = np.zeros((N, 1, 10, 1), F); tg[np.arange(N), 0, rng.integers(0, 10, N), 0] = 1.0
    vm.store(tg, "%d 1 10 1 tensor constant t%s t%s" % (N, name, name)); vm.eval("drop")
    out = vm.eval("%s t%s backprop drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    grads = layer_tensors(vm, name, nl + 1)
    x, dy = acts[k], grads[k + 1]                                          # the layer's input, and the dY it received
    assert dy.any() and dy.shape[-1] == E
    T = dy.size // E
    O, DT, DP, DX = entries(t4k, x, TAB, POS, dy, V, E, L)
    assert bits(acts[k + 1], O), "the layer's output is not the entry's"
    assert bits(O, ew.fwd32(x.ravel() if V else x.reshape(T, E), TAB, POS, T, L, V, E))
    if V:
        assert bits(grads[k], X) and bits(acts[k], X), "backprop wrote into the ids"
        dw = get(vm, name, k, "nn.dw")
        assert bits(dw, DT), "dTABLE is not the entry's"
        ew.check(name + " dtable", dw.reshape(V, E), ew.em_dtable(x.ravel(), dy, np.zeros((V, E)), V, E))
        pad = ~ew.valid_ids(x.ravel(), V)[0]
        assert pad.any() and bits(acts[k + 1].reshape(T, E)[pad], np.broadcast_to(POS, (N, L, E)).reshape(T, E)[pad])      # padding: the position alone
    else:
        assert bits(grads[k], dy) and bits(DX, dy), "the position layer's dX is not dY"
    db = get(vm, name, k, "nn.db")
    assert bits(db, DP), "dPOS is not the entry's"
    ew.check(name + " dpos", db.reshape(L, E), ew.em_dpos(dy, np.zeros((L, E)), T, L, E))
    if V:                                                                   # a second backprop without a forward still finds the ids
        vm.eval("%s t%s backprop drop" % (name, name))
        assert bits(layer_tensors(vm, name, 1)[0], X)


def launches(vm, t4k, w):
    vm.eval(w)
    l0 = lcount(t4k); vm.eval(w); return lcount(t4k) - l0


@pytest.mark.parametrize("mode", ["tok", "tokpos", "pos"])
def test_the_layers_launches(vm, t4k, mode):
    """two nets that differ by the layer alone (sigmoid layers join no fused group): the forward's difference is one launch, the backward's the plan's"""
    N = 2
    V, pos, C = {"tok": (11, 0, 1), "tokpos": (11, 1, 1), "pos": (0, 1, 8)}[mode]
    a, b = "emla" + mode, "emlb" + mode
    vm.eval("%d 4 4 %d nn.model 3 vector{ %d %d %d } upsample sigmoid sigmoid constant %s" % (N, C, V, 8, pos, a))
    vm.eval("%d 4 4 8 nn.model sigmoid sigmoid constant %s" % (N, b))
    rng = np.random.default_rng(3)
    xa = ew.make_ids(rng, N * 16, 11, "plain").reshape(N, 4, 4, 1) if V else operand(rng, N, 4, 4, 8)
    vm.store(xa, "%d 4 4 %d tensor constant xa%s xa%s" % (N, C, mode, mode)); vm.eval("drop")
    vm.store(operand(rng, N, 4, 4, 8), "%d 4 4 8 tensor constant xb%s xb%s" % (N, mode, mode)); vm.eval("drop")
    fa, fb = launches(vm, t4k, "%s xa%s forward drop" % (a, mode)), launches(vm, t4k, "%s xb%s forward drop" % (b, mode))
    ba, bb = launches(vm, t4k, "%s xb%s backprop drop" % (a, mode)), launches(vm, t4k, "%s xb%s backprop drop" % (b, mode))
    out8 = (ctypes.c_int * 8)()
    assert t4k.lib.t4k_embed_plan(N * 16, 16, V, 8, pos, 1, 32 << 20, out8) == 0
    print("forward launches %d against %d, backward %d against %d; the plan %s" % (fa, fb, ba, bb, list(out8)))
    assert fa - fb == out8[4] == 1 and ba - bb == out8[5] == 1, (fa, fb, ba, bb, list(out8))


@pytest.mark.parametrize("opt", ["0.01 0.0 nn.sgd", "0.001 0.9 nn.adam"], ids=["sgd", "adam"])
@pytest.mark.parametrize("net", list(NETS))
def test_the_optimizers_move_the_tables(vm, net, opt):
    name = "emo" + net + opt.split(".")[-1]
    rng = np.random.default_rng(13)
    (H, W, C), _, k, V, E, L, _ = NETS[net]
    TAB, POS = build(vm, name, net, 2, rng)
    X = inputs(net, 2, rng)
    if V:
        X.ravel()[:] = np.arange(X.size) % V                               # every row is named
    vm.store(X, "2 %d %d %d tensor constant x%s x%s" % (H, W, C, name, name)); vm.eval("drop")
    tg = np.zeros((2, 1, 10, 1), F); tg[0, 0, 3, 0] = tg[1, 0, 7, 0] = 1.0
    vm.store(tg, "2 1 10 1 tensor constant t%s t%s" % (name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward t%s backprop drop" % (name, name, name))
    assert "not supported" not in out and "failed" not in out, out
    out = vm.eval("%s %s drop" % (name, opt))
    assert "not supported" not in out and "failed" not in out, out
    for word, dword, a0 in (("nn.w", "nn.dw", TAB), ("nn.b", "nn.db", POS)):
        if a0 is None:
            continue
        a = get(vm, name, k, word)
        assert np.isfinite(a).all() and np.count_nonzero(a.ravel() != a0.ravel()) > a0.size // 2, (word, a.ravel()[:8], a0.ravel()[:8])
        assert not get(vm, name, k, dword).any()                           # the step consumed the gradients


@pytest.mark.parametrize("net", list(NETS))
def test_t4_file_round_trip(vm, tmp_path, net):
    """`save` writes the layer's line and TABLE | POS; `load` into a net built alike (other parameters) gives the same forward bits"""
    rng = np.random.default_rng(17)
    (H, W, C), _, k, V, E, L, nl = NETS[net]
    a, b = "emva" + net, "emvb" + net
    build(vm, a, net, 2, rng)
    f = str(tmp_path / "a.t4")
    vm.eval('%s s" %s" save' % (a, f)); vm.eval("drop")
    blob = open(f, "rb").read()
    assert b"\nvocab=%d, pos=1embed  \n" % V in blob
    assert blob.count(b"\n--- w.embed  \n") == (1 if V else 0) and blob.count(b"\n--- b.embed  \n") == 1
    build(vm, b, net, 2, rng)
    out = vm.eval('%s s" %s" load' % (b, f)); out += vm.eval("drop")
    assert "error" not in out, out
    X = inputs(net, 2, rng)
    vm.store(X, "2 %d %d %d tensor constant xv%s xv%s" % (H, W, C, net, net)); vm.eval("drop")
    outs = []
    for m in (a, b):
        out = vm.eval("%s xv%s forward drop" % (m, net))
        assert "not supported" not in out and "failed" not in out, out
        outs.append([t.copy() for t in layer_tensors(vm, m, nl + 1)])
    for x, y in zip(*outs):
        assert bits(x, y)
    open(f, "wb").write(blob.replace(b"vocab=%d, pos=1embed" % V, b"vocab=%d, pos=1embed" % (V + 1)))
    out = vm.eval('%s s" %s" load' % (b, f)); out += vm.eval("drop")
    assert "format error" in out, out
