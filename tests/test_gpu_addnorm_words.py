"""`vector{ back mode } selu`, the add & norm layer, on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so).

Five nets on `N 4 4 C` inputs, each closed with `flatten 10 linear softmax`: the pre-norm attention block and the post-norm ResNet block of the design, the
pre-norm block behind a `0.5 8 conv2d` stem, a chain of two blocks where the second taps the first one's add, and a nested pair of spans.  Every parameter is
set through the write-through views of `nn.w` / `nn.b`.  After `forward` every addnorm layer's output is bit-equal to t4k_addnorm_fwd called on the layer's own
fetched input and skip source (and, with mode 0, to NumPy's float32 input + source); after `T backprop` the dX it leaves in its input tensor, `nn.dw` and
`nn.db` are bit-equal to t4k_addnorm_bwd on the dY the VM itself stored and - for a tapped layer - the dX the tapping layer left in ITS input tensor; all of it
inside the staged float64 witnesses of tests/an_witness.py.  Every conv layer's dW and every norm's dgamma | dbeta are held against torch's float64 autograd of
the same net (the fetched weights, the stored dY of the block's last tensor as the upstream gradient; a 3x3 conv with the reference's mirrored dX): this is the check of the wiring - which tensor is the
skip, which gradient arrives over it - since a wrong edge is wrong by the size of the gradient.  Its bound is the reference's own float32 error: the same torch
net in float32 differs from the float64 one by e = max |g32 - g64|; the kernels sum in another order, another sample of the same error, so 4 e, plus the
C_SUM (rows + 3) u max|g| of the last sum's own roundings.  The layer's launches are the plan's, counted as the difference between two nets that differ by the
layer alone.  `nn.sgd` and `nn.adam` steps run and move the conv layers and gamma | beta; the `.t4` round trip gives the same forward bits."""
import ctypes

import numpy as np
import pytest
import torch

import an_witness as an
from test_gpu_bcast import Dev
from test_gpu_pool_geo import lcount
from test_gpu_pool_geo_words import layer_tensors, operand

pytestmark = pytest.mark.gpu

H, W = 4, 4
TAIL = " flatten 10 linear softmax"
# a net: (input channels, [layer]); a layer is ("an", back, mode) | ("c1", C0) conv1x1 | ("c3", C0) conv2d 3x3 | ("relu",) | ("attn", heads)
NETS = {
    "pre":    (8, [("an", 0, 0), ("an", 0, 1), ("c1", 24), ("attn", 2), ("c1", 8), ("an", 4, 0)]),
    "post":   (8, [("an", 0, 0), ("c3", 8), ("relu",), ("c3", 8), ("an", 3, 1), ("relu",)]),
    "stem":   (3, [("c3", 8), ("an", 0, 0), ("an", 0, 2), ("c1", 24), ("attn", 2), ("c1", 8), ("an", 4, 0)]),
    "chain":  (8, [("an", 0, 0), ("c1", 8), ("an", 1, 0), ("c1", 8), ("an", 1, 1)]),
    "nested": (8, [("an", 0, 0), ("relu",), ("an", 0, 0), ("c1", 8), ("an", 1, 0), ("c1", 8), ("an", 5, 2)]),
}


def words(layers):
    w = {"an": "2 vector{ %d %d } selu", "c1": "0.5 %d conv1x1", "c3": "0.5 %d conv2d", "relu": "relu", "attn": "1 vector{ %d } linear"}
    return " ".join(w[l[0]] % l[1:] for l in layers)


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def nan(k):
    return np.full(k, np.nan, np.float32)


def put(vm, name, i, word, a):
    vm.store(a, "%s %d %s" % (name, i, word)); vm.eval("drop drop")


def get(vm, name, i, word):
    a = vm.fetch("%s %d %s" % (name, i, word)).copy(); vm.eval("drop drop")
    return a


def build(vm, name, net, N, rng):
    """the net as constant `name`, every parameter from rng (scaled so that the activations keep their size); returns {layer: (w, b)}"""
    C, layers = NETS[net]
    out = vm.eval("%d %d %d %d nn.model %s constant %s" % (N, H, W, C, words(layers) + TAIL, name))
    assert "nn#iaddnorm" not in out and "no param" not in out, out
    P = {}
    for i, l in enumerate(layers):
        if l[0] in ("c1", "c3"):
            K = 1 if l[0] == "c1" else 3
            F = operand(rng, C, K, K, l[1]) / np.float32(K * np.sqrt(C)); B = operand(rng, l[1]) / np.float32(4.0)
            put(vm, name, i, "nn.w", F); put(vm, name, i, "nn.b", B); P[i] = (F, B); C = l[1]
        elif l[0] == "attn":
            C //= 3
        elif l[0] == "an" and l[2]:
            G = operand(rng, C); B = operand(rng, C) / np.float32(4.0)
            put(vm, name, i, "nn.w", G); put(vm, name, i, "nn.b", B); P[i] = (G, B)
    return P


class RefConv3(torch.autograd.Function):
    """`0.5 C conv2d` (3x3, stride 1, padding 1) on NCHW as the library computes it: the textbook forward, dF and dB, and the reference's dX, which runs the
    filter mirrored (f64_witness.conv_dx: DX[i + ky - P] += F[K - 1 - ky] dO[i]) - the layers in front of such a conv train on that gradient"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.nn.functional.conv2d(x, w, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return (torch.nn.functional.conv_transpose2d(g, w.flip(2, 3), padding=1), torch.nn.grad.conv2d_weight(x, w.shape, g, padding=1), g.sum((0, 2, 3)))


def torch_net(layers, P, X, dt):
    """the block in torch at precision dt: (tensors t[0..L], parameters {layer: (w, b)} that require grad)"""
    t = [torch.tensor(X.astype(np.float64)).to(dt)]
    Q = {}
    for i, l in enumerate(layers):
        x = t[-1]
        if i in P:
            Q[i] = tuple(torch.tensor(p.astype(np.float64)).to(dt).requires_grad_(True) for p in P[i])
        if l[0] == "c1":
            w, b = Q[i]; y = x @ w.reshape(w.shape[0], w.shape[3]) + b
        elif l[0] == "c3":
            w, b = Q[i]                                                     # F[c1, ky, kx, c0] -> weight[c0][c1][ky][kx]
            y = RefConv3.apply(x.permute(0, 3, 1, 2), w.permute(3, 0, 1, 2), b).permute(0, 2, 3, 1)
        elif l[0] == "relu":
            y = torch.relu(x)
        elif l[0] == "attn":
            N, E, hd = x.shape[0], x.shape[3] // 3, l[1]
            q = x.reshape(N, H * W, 3, hd, E // hd).permute(2, 0, 3, 1, 4)
            y = torch.nn.functional.scaled_dot_product_attention(q[0], q[1], q[2], scale=float(np.float32(1.0 / np.sqrt(E // hd))))
            y = y.permute(0, 2, 1, 3).reshape(N, H, W, E)
        else:
            _, back, mode = l
            z = x + t[i - back] if back else x
            if mode == 1:
                y = torch.nn.functional.layer_norm(z, (z.shape[-1],), Q[i][0], Q[i][1], an.EPS)
            elif mode == 2:
                y = z * torch.rsqrt((z * z).mean(-1, keepdim=True) + an.EPS) * Q[i][0] + Q[i][1]
            else:
                y = z + 0
        t.append(y)
    return t, Q


def entries(t4k, x, s, dy, dy2, G, B, mode):
    """the two entries on the same tensors: (O, XH, RSTD, DX, DW, DB), DW | DB from zero"""
    C = x.shape[-1]; rows = x.size // C; norm = mode != 0
    dX, dS, dDY, dD2 = Dev(x), (Dev(s) if s is not None else None), Dev(dy), (Dev(dy2) if dy2 is not None else None)
    dW, dB = (Dev(G), Dev(B)) if norm else (None, None)
    dO, dXH, dR, dDX, dDW, dDB = Dev(nan(x.size)), Dev(nan(x.size)), Dev(nan(rows)), Dev(nan(x.size)), Dev(np.zeros(C, np.float32)), Dev(np.zeros(C, np.float32))
    p = lambda d: d.p if d is not None else None
    t4k.call("t4k_addnorm_fwd", dX.p, p(dS), dO.p, dXH.p if norm else None, dR.p if norm else None, p(dW), p(dB), rows, C, mode, an.EPS, None)
    t4k.call("t4k_addnorm_bwd", p(dW), dDY.p, p(dD2), dXH.p if norm else None, dR.p if norm else None, dDX.p, dDW.p, dDB.p, rows, C, mode, 1, None)
    return [d.get(t4k, sh).copy() for d, sh in ((dO, x.shape), (dXH, x.shape), (dR, (rows,)), (dDX, x.shape), (dDW, (C,)), (dDB, (C,)))]


def bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).ravel().view(np.uint32), np.ascontiguousarray(b, np.float32).ravel().view(np.uint32))


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("N", [2, 64])
def test_the_layer_inside_a_net(vm, t4k, N, net):
    name = "an%s%d" % (net, N)
    rng = np.random.default_rng(5 + N + len(net))
    C0, layers = NETS[net]
    L = len(layers)
    P = build(vm, name, net, N, rng)
    X = operand(rng, N, H, W, C0)
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C0, name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    acts = layer_tensors(vm, name, L + 1)
    T = np.zeros((N, 1, 10, 1), np.float32); T[np.arange(N), 0, rng.integers(0, 10, N), 0] = 1.0
    vm.store(T, "%d 1 10 1 tensor constant t%s t%s" % (N, name, name)); vm.eval("drop")
    out = vm.eval("%s t%s backprop drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    grads = layer_tensors(vm, name, L + 1)                               # tensor i now holds the dX of layer i; a tapped one what arrived from the layer behind it
    assert grads[L].any()
    tapper = {j - l[1]: j for j, l in enumerate(layers) if l[0] == "an" and l[1]}     # tapped tensor -> the tapping layer (whose input tensor has its index)
    for i, l in enumerate(layers):
        if l[0] != "an":
            continue
        _, back, mode = l
        x, s = acts[i], (acts[i - back] if back else None)
        dy, dy2 = grads[i + 1], (grads[tapper[i + 1]] if i + 1 in tapper else None)
        G, B = P.get(i, (None, None))
        O, XH, R, DX, DW, DB = entries(t4k, x, s, dy, dy2, G, B, mode)
        tag = "%s layer %d" % (name, i)
        assert bits(acts[i + 1], O), tag + ": the layer's output is not the entry's"
        assert bits(grads[i], DX), tag + ": the layer's dX is not the entry's"
        C = x.shape[-1]
        if mode == 0:
            assert bits(O, x + s if back else x), tag                       # bit-equal to input + source
            assert bits(DX, dy + dy2 if dy2 is not None else dy), tag
        else:
            assert bits(get(vm, name, i, "nn.ex"), XH), tag
            assert bits(get(vm, name, i, "nn.dw"), DW) and bits(get(vm, name, i, "nn.db"), DB), tag + ": dgamma | dbeta are not the entry's"
            an.check(tag + " rstd", R, an.an_rstd(x, s, C, mode)); an.check(tag + " xhat", XH, an.an_xhat(x, s, R, C, mode))
            an.check(tag + " y", O, an.an_y(XH, G, B, C))
            wdw, wdb = an.an_dwdb(dy, dy2, XH, np.zeros(C), np.zeros(C), C, 1)
            an.check(tag + " dw", DW, wdw); an.check(tag + " db", DB, wdb)
        an.check(tag + " dx", DX, an.an_dx(G, dy, dy2, XH, R, C, mode))
    # the wiring, against torch's float64 autograd of the block; the bound from the same net in float32 (the module's docstring)
    g = {}
    for dt in (torch.float64, torch.float32):
        t, Q = torch_net(layers, P, X, dt)
        t[L].backward(torch.tensor(grads[L].astype(np.float64)).to(dt))
        g[dt] = {i: [q.grad.double().numpy() for q in qs] for i, qs in Q.items()}
        if dt == torch.float64:
            for k in range(1, L + 1):                                       # and the forward: every tensor of the block
                e = np.max(np.abs(acts[k].astype(np.float64) - t[k].detach().numpy()))
                assert e <= 1e-3 * max(1.0, float(t[k].detach().abs().max())), (name, k, e)
    rows = N * H * W
    for i in P:
        for k, word in ((0, "nn.dw"), (1, "nn.db")):
            got = get(vm, name, i, word).astype(np.float64).reshape(g[torch.float64][i][k].shape)
            ex = g[torch.float64][i][k]
            e32 = np.max(np.abs(g[torch.float32][i][k] - ex))
            bound = 4.0 * e32 + an.C_SUM * (rows + 3) * an.U * np.max(np.abs(ex))
            err = np.max(np.abs(got - ex))
            print("%s layer %d %s: |err| %.3g, torch float32 %.3g, bound %.3g, max|g| %.3g" % (name, i, word, err, e32, bound, np.max(np.abs(ex))))
            assert err <= bound, (name, i, word, err, bound)


def launches(vm, t4k, w):
    vm.eval(w)
    l0 = lcount(t4k); vm.eval(w); return lcount(t4k) - l0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_layers_launches(vm, t4k, mode):
    """two nets that differ by the adding layer alone (sigmoid layers on either side join no fused group): the forward's difference is one launch, the
    backward's the plan's - one for a plain add, one and the fold for a norm"""
    N = 2
    a, b = "anla%d" % mode, "anlb%d" % mode
    vm.eval("%d 4 4 8 nn.model 2 vector{ 0 0 } selu sigmoid 2 vector{ 1 %d } selu sigmoid constant %s" % (N, mode, a))
    vm.eval("%d 4 4 8 nn.model 2 vector{ 0 0 } selu sigmoid sigmoid constant %s" % (N, b))
    rng = np.random.default_rng(3)
    vm.store(operand(rng, N, 4, 4, 8), "%d 4 4 8 tensor constant xanl%d xanl%d" % (N, mode, mode)); vm.eval("drop")
    vm.store(operand(rng, N, 4, 4, 8), "%d 4 4 8 tensor constant tanl%d tanl%d" % (N, mode, mode)); vm.eval("drop")
    fa, fb = (launches(vm, t4k, "%s xanl%d forward drop" % (m, mode)) for m in (a, b))
    ba, bb = (launches(vm, t4k, "%s tanl%d backprop drop" % (m, mode)) for m in (a, b))
    out8 = (ctypes.c_int * 8)()
    assert t4k.lib.t4k_addnorm_plan(N * 16, 8, mode, 1, 32 << 20, out8) == 0
    print("forward launches %d against %d, backward %d against %d; the plan %s" % (fa, fb, ba, bb, list(out8)))
    assert fa - fb == out8[4] == 1 and ba - bb == out8[7] == (2 if mode else 1), (fa, fb, ba, bb, list(out8))


@pytest.mark.parametrize("opt", ["0.01 0.0 nn.sgd", "0.001 0.9 nn.adam"], ids=["sgd", "adam"])
@pytest.mark.parametrize("net", ["pre", "post"])
def test_the_optimizers_move_the_block(vm, net, opt):
    name = "ano" + net + opt.split(".")[-1]
    rng = np.random.default_rng(13)
    C0, layers = NETS[net]
    P = build(vm, name, net, 2, rng)
    vm.store(operand(rng, 2, H, W, C0), "2 %d %d %d tensor constant x%s x%s" % (H, W, C0, name, name)); vm.eval("drop")
    T = np.zeros((2, 1, 10, 1), np.float32); T[0, 0, 3, 0] = T[1, 0, 7, 0] = 1.0
    vm.store(T, "2 1 10 1 tensor constant t%s t%s" % (name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward t%s backprop drop" % (name, name, name))
    assert "not supported" not in out and "failed" not in out, out
    out = vm.eval("%s %s drop" % (name, opt))
    assert "not supported" not in out and "failed" not in out, out
    for i, (w0, b0) in P.items():
        w, b = get(vm, name, i, "nn.w"), get(vm, name, i, "nn.b")
        assert np.isfinite(w).all() and np.count_nonzero(w.ravel() != w0.ravel()) > w0.size // 2, (i, w.ravel()[:8], w0.ravel()[:8])
        assert np.isfinite(b).all() and np.count_nonzero(b.ravel() != b0.ravel()) > b0.size // 2, (i, b.ravel()[:8], b0.ravel()[:8])
        assert not get(vm, name, i, "nn.dw").any() and not get(vm, name, i, "nn.db").any()        # the step consumed the gradients


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes the layers' lines and gamma | beta of the norm; `load` into a net built alike (other parameters) gives the same forward bits"""
    rng = np.random.default_rng(17)
    build(vm, "anva", "post", 2, rng)
    f = str(tmp_path / "a.t4")
    vm.eval('anva s" %s" save' % f); vm.eval("drop")
    blob = open(f, "rb").read()
    assert b"\nback=0, mode=0addnorm\n" in blob and b"\nback=3, mode=1addnorm\n" in blob
    assert blob.count(b"\n--- w.addnorm\n") == 1 and blob.count(b"\n--- b.addnorm\n") == 1 and blob.count(b"\n--- w.") == 4
    build(vm, "anvb", "post", 2, rng)
    out = vm.eval('anvb s" %s" load' % f); out += vm.eval("drop")
    assert "error" not in out, out
    X = operand(rng, 2, H, W, 8)
    vm.store(X, "2 %d %d 8 tensor constant xanv xanv" % (H, W)); vm.eval("drop")
    outs = []
    for m in ("anva", "anvb"):
        out = vm.eval("%s xanv forward drop" % m)
        assert "not supported" not in out and "failed" not in out, out
        outs.append([t.copy() for t in layer_tensors(vm, m, len(NETS["post"][1]) + 4)])
    for x, y in zip(*outs):
        assert bits(x, y)
    assert outs[0][-1].size == 20
    # a file whose span differs is refused and changes nothing
    open(f, "wb").write(blob.replace(b"back=3, mode=1addnorm", b"back=2, mode=1addnorm"))
    out = vm.eval('anvb s" %s" load' % f); out += vm.eval("drop")
    assert "format error" in out, out
    vm.eval("anvb xanv forward drop")
    assert bits(layer_tensors(vm, "anvb", 6)[5], outs[0][5])
