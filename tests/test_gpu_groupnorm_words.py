"""`vector{ G } batchnorm`, the group / layer / instance norm layer, on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so).

Two blocks: `conv2d -> vector{ G } batchnorm -> relu` (group norm behind an ordinary conv) and depthwise `conv2d -> vector{ 1 } batchnorm -> conv1x1` (a
ConvNeXt-style layer norm).  After `forward` every norm layer's output is bit-equal to t4k_groupnorm_fwd called on the layer's own fetched input, gamma and
beta, and every tensor that call stored is inside the staged float64 witnesses of tests/gn_witness.py; after `T backprop` the layer's in-place dX, `nn.dw` and
`nn.db` are bit-equal to t4k_groupnorm_bwd on the dY the VM itself stored, and inside the witnesses.  The conv in front of the norm runs on its own engine:
its output is the convolution of its input (float64 witness), and the forward's launches are that entry's plus the norm's plus the layer behind - no conv +
batch-norm epilogue.  The same model with plain `batchnorm` still takes the epilogue route (its four launches).  Lazy and eager dX0, N = 2 and N = 64, `nn.sgd` and
`nn.adam` move gamma and beta, the `.t4` round trip restores them bit for bit."""
import ctypes

import numpy as np
import pytest

import f64_witness as fw
import gn_witness as gw
from test_gpu_bcast import Dev
from test_gpu_pool_geo import lcount
from test_gpu_pool_geo_words import layer_tensors, operand

pytestmark = pytest.mark.gpu

EPS = gw.EPS
F_BN_PARENT = 4                                                          # forward launches of conv2d -> 0.1 batchnorm -> relu (the route of a layer with iparm == 0 is the parent's: conv with the statistics in its epilogue, their fold, the apply, the relu)
# name -> (layers, op of the norm layer, G, shapes of the layer tensors)
NETS = {
    "gn": ("0.5 8 conv2d 1 vector{ %d } batchnorm relu", 1, [(6, 6, 3), (6, 6, 8), (6, 6, 8), (6, 6, 8)]),
    "ln": ("0.5 8 5 vector{ 3 1 1 1 8 } conv2d 1 vector{ %d } batchnorm 0.5 4 conv1x1", 1, [(6, 6, 8), (6, 6, 8), (6, 6, 8), (6, 6, 4)]),
}


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def nan(k):
    return np.full(k, np.nan, np.float32)


def build(vm, name, kind, N, G, rng):
    layers, op, shapes = NETS[kind]
    H, W, C = shapes[0]
    vm.eval("%d %d %d %d nn.model %s constant %s" % (N, H, W, C, layers % G, name))
    Cn = shapes[op][2]
    Wg, B = operand(rng, Cn), operand(rng, Cn)
    vm.store(Wg, "%s %d nn.w" % (name, op)); vm.eval("drop drop")
    vm.store(B, "%s %d nn.b" % (name, op)); vm.eval("drop drop")
    assert np.array_equal(vm.fetch("%s %d nn.w" % (name, op)).ravel(), Wg); vm.eval("drop drop")
    return op, shapes, Wg, B


def entry(t4k, X, DY, Wg, B, G):
    """the two entries on the same tensors: (O, XH, STAT, DX, DW, DB), DW | DB from zero"""
    N, H, W, C = X.shape
    dI, dDY, dW, dB = Dev(X), Dev(DY), Dev(Wg), Dev(B)
    dO, dXH, dDX, dST, dDW, dDB = Dev(nan(X.size)), Dev(nan(X.size)), Dev(nan(X.size)), Dev(nan(4 * N * G)), Dev(np.zeros(C, np.float32)), Dev(np.zeros(C, np.float32))
    t4k.call("t4k_groupnorm_fwd", dI.p, dO.p, dXH.p, dW.p, dB.p, dST.p, N, H * W, C, G, EPS, None)
    t4k.call("t4k_groupnorm_bwd", dW.p, dDY.p, dXH.p, dST.p, dDX.p, dDW.p, dDB.p, N, H * W, C, G, 1, None)
    return dO.get(t4k, X.shape).copy(), dXH.get(t4k, X.shape).copy(), dST.get(t4k, (4 * N * G,)).copy(), dDX.get(t4k, X.shape).copy(), dDW.get(t4k, (C,)).copy(), dDB.get(t4k, (C,)).copy()


def run_block(vm, t4k, name, kind, N, G, seed):
    rng = np.random.default_rng(seed)
    op, shapes, Wg, B = build(vm, name, kind, N, G, rng)
    H, W, C = shapes[0]
    X = operand(rng, N, H, W, C)
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    acts = layer_tensors(vm, name, len(shapes))
    for i, s in enumerate(shapes):
        assert acts[i].shape == (N,) + s, (i, acts[i].shape)
    h, w, c = shapes[-1]
    T = operand(rng, N, h, w, c)
    vm.store(T, "%d %d %d %d tensor constant t%s t%s" % (N, h, w, c, name, name)); vm.eval("drop")
    out = vm.eval("%s t%s backprop drop" % (name, name))
    assert "not supported" not in out and "failed" not in out, out
    grads = layer_tensors(vm, name, len(shapes))                       # layer i now holds dX of op i
    I, DY = acts[op], grads[op + 1]
    O, XH, ST, DX, DW, DB = entry(t4k, I, DY, Wg, B, G)
    assert np.array_equal(acts[op + 1], O), "%s: the layer's output is not the entry's" % name
    assert np.array_equal(grads[op], DX), "%s: the layer's dX is not the entry's" % name
    assert np.array_equal(vm.fetch("%s %d nn.dw" % (name, op)).ravel(), DW); vm.eval("drop drop")
    assert np.array_equal(vm.fetch("%s %d nn.db" % (name, op)).ravel(), DB); vm.eval("drop drop")
    NG = N * G
    wm, wr = gw.gn_stats(I, G)
    gw.check(name + " mean", ST[:NG], wm); gw.check(name + " rstd", ST[NG:2 * NG], wr)
    gw.check(name + " xhat", XH, gw.gn_xhat(I, ST, G)); gw.check(name + " y", O, gw.gn_y(XH, Wg, B))
    ws1, ws2, wdw, wdb = gw.gn_bwd_stats(Wg, DY, XH, G, np.zeros(len(Wg)), np.zeros(len(Wg)), True)
    gw.check(name + " s1", ST[2 * NG:3 * NG], ws1); gw.check(name + " s2", ST[3 * NG:], ws2)
    gw.check(name + " dx", DX, gw.gn_dx(Wg, DY, XH, ST, G)); gw.check(name + " dw", DW, wdw); gw.check(name + " db", DB, wdb)
    return acts, grads


def test_network_text(vm):
    vm.eval("2 6 6 3 nn.model " + (NETS["gn"][0] % 2) + " constant nett")
    txt = vm.eval("nett network drop")
    assert "[  1] batchnm: T4[2,6,6,8] #p=608 T1[8] T1[8] T4[2,6,6,8] G=2, eps=1e-05\n[  2] relu   :" in txt, txt
    assert "nn#ibatchnorm groups=3? channels=8" in vm.eval("2 6 6 8 nn.model 1 vector{ 3 } batchnorm drop")


@pytest.mark.parametrize("lazy", [True, False], ids=["lazy_dx0", "eager_dx0"])
@pytest.mark.parametrize("N", [2, 64])
def test_blocks_layer_by_layer(vm, t4k, N, lazy):
    from tensorforth_amd.vm import set_lazy_dx0
    prev = set_lazy_dx0(lazy)
    try:
        tag = "%d%s" % (N, "l" if lazy else "e")
        acts, grads = run_block(vm, t4k, "gna" + tag, "gn", N, 2, 5)
        assert np.array_equal(acts[3], np.maximum(acts[2], 0)) and np.array_equal(grads[2], grads[3] * (acts[2] > 0))      # the relu behind the norm ran as it runs anywhere
        run_block(vm, t4k, "gnb" + tag, "gn", N, 8, 6)                  # instance norm
        run_block(vm, t4k, "lna" + tag, "ln", N, 1, 7)                  # layer norm behind a depthwise conv
        assert grads[0].shape == acts[0].shape and np.isfinite(grads[0]).all()                                             # dX0, whichever plan produced it
    finally:
        set_lazy_dx0(prev)


def fwd_launches(vm, t4k, name):
    vm.eval("%s x%s forward drop" % (name, name))
    l0 = lcount(t4k); vm.eval("%s x%s forward drop" % (name, name)); return lcount(t4k) - l0


def test_the_conv_in_front_runs_on_its_own_engine(vm, t4k):
    """conv -> group norm -> relu: the conv's output is the plain convolution (float64 witness), and the forward launches are that entry's + the norm's (its plan) + the relu's one;
    the same model with plain `batchnorm` keeps the conv + batch-norm epilogue route and its four launches"""
    N = 2
    rng = np.random.default_rng(11)
    build(vm, "nete", "gn", N, 2, rng)
    X = operand(rng, N, 6, 6, 3)
    vm.store(X, "%d 6 6 3 tensor constant xnete xnete" % N); vm.eval("drop")
    f_gn = fwd_launches(vm, t4k, "nete")
    acts = layer_tensors(vm, "nete", 2)
    F = vm.fetch("nete 0 nn.w").copy(); vm.eval("drop drop")
    Bc = vm.fetch("nete 0 nn.b").copy(); vm.eval("drop drop")
    dX, dF, dB, dCP, dO = Dev(X), Dev(F), Dev(Bc), Dev(nan(X.size)), Dev(nan(acts[1].size))
    l0 = lcount(t4k)
    t4k.call("t4k_conv2d_fwd2", dX.p, dCP.p, dO.p, dF.p, dB.p, N, 6, 6, 3, 6, 6, 8, 3, 1, 1, None)
    f_conv = lcount(t4k) - l0
    fw.check("the conv entry alone", dO.get(t4k, acts[1].shape), fw.conv_fwd(X, F, Bc.ravel(), 1, 1))
    fw.check("the conv layer in front of the norm", acts[1], fw.conv_fwd(X, F, Bc.ravel(), 1, 1))
    out = (ctypes.c_int * 8)()
    assert t4k.lib.t4k_groupnorm_plan(N, 36, 8, 2, 1, 32 << 20, out) == 0
    # plain batchnorm in the same place: what the parent launched - the statistics ride in the conv's epilogue, the apply in the run's launch
    vm.eval("%d 6 6 3 nn.model 0.5 8 conv2d 0.1 batchnorm relu constant netp" % N)
    vm.store(X, "%d 6 6 3 tensor constant xnetp xnetp" % N); vm.eval("drop")
    f_bn = fwd_launches(vm, t4k, "netp")
    assert f_gn == f_conv + out[4] + 1, (f_gn, f_conv, list(out))
    print("forward launches: conv alone %d, conv + group norm + relu %d, conv + batchnorm + relu %d" % (f_conv, f_gn, f_bn))
    assert f_bn == F_BN_PARENT, f_bn
    a = layer_tensors(vm, "netp", 4)
    assert np.array_equal(a[3], np.maximum(a[2], 0))


@pytest.mark.parametrize("opt", ["0.01 0.0 nn.sgd", "0.001 0.9 nn.adam"], ids=["sgd", "adam"])
def test_the_optimizers_move_gamma_and_beta(vm, opt):
    name = "neto" + opt.split(".")[-1]
    rng = np.random.default_rng(13)
    op, shapes, Wg, B = build(vm, name, "gn", 2, 2, rng)
    vm.store(operand(rng, 2, 6, 6, 3), "2 6 6 3 tensor constant x%s x%s" % (name, name)); vm.eval("drop")
    vm.store(operand(rng, 2, 6, 6, 8), "2 6 6 8 tensor constant t%s t%s" % (name, name)); vm.eval("drop")
    out = vm.eval("%s x%s forward t%s backprop drop" % (name, name, name))
    assert "not supported" not in out and "failed" not in out, out
    dw = vm.fetch("%s %d nn.dw" % (name, op)).ravel().copy(); vm.eval("drop drop")
    db = vm.fetch("%s %d nn.db" % (name, op)).ravel().copy(); vm.eval("drop drop")
    assert np.count_nonzero(dw) >= 4 and np.count_nonzero(db) >= 4, (dw, db)        # (a channel the relu behind the norm shuts off everywhere has no gradient)
    out = vm.eval("%s %s drop" % (name, opt))
    assert "not supported" not in out and "failed" not in out, out
    w = vm.fetch("%s %d nn.w" % (name, op)).ravel().copy(); vm.eval("drop drop")
    b = vm.fetch("%s %d nn.b" % (name, op)).ravel().copy(); vm.eval("drop drop")
    assert np.isfinite(w).all() and np.isfinite(b).all()
    assert np.array_equal(w != Wg, dw != 0) and np.array_equal(b != B, db != 0), (w, Wg, dw, b, B, db)     # moved exactly where there is a gradient
    assert not vm.fetch("%s %d nn.dw" % (name, op)).any(); vm.eval("drop drop")          # the step consumed the gradients


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes gamma AND beta of the vector form; `load` into a net built alike restores both bit for bit"""
    rng = np.random.default_rng(17)
    op, _, Wg, B = build(vm, "netv", "gn", 2, 2, rng)
    a, b = str(tmp_path / "a.t4"), str(tmp_path / "b.t4")
    vm.eval('netv s" %s" save' % a); vm.eval("drop")
    blob = open(a, "rb").read()
    assert b"\nG=2, eps=1e-05batchnm\n" in blob and b"\n--- w.batchnm\n" + Wg.tobytes() + b"\n--- b.batchnm\n" + B.tobytes() in blob
    build(vm, "netw", "gn", 2, 2, np.random.default_rng(18))
    out = vm.eval('netw s" %s" load' % a); out += vm.eval("drop")
    assert "error" not in out, out
    assert np.array_equal(vm.fetch("netw %d nn.w" % op).ravel(), Wg); vm.eval("drop drop")
    assert np.array_equal(vm.fetch("netw %d nn.b" % op).ravel(), B); vm.eval("drop drop")
    vm.eval('netw s" %s" save' % b); vm.eval("drop")
    assert open(a, "rb").read() == open(b, "rb").read()
