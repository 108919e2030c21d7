"""`vector{ heads 1 1 } linear`, the retention layer, on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so).

The net is `2 4 4 8 nn.model 0.5 24 conv1x1 3 vector{ 2 1 1 } linear 0.5 8 conv1x1 flatten 10 linear softmax` (16 tokens, 2 heads of 4 channels).  After
`forward` the layer's output is bit-equal to t4k_retention_fwd on the layer's own fetched input, after `T backprop` the dX it leaves in its input tensor
bit-equal to t4k_retention_bwd on the dY the VM itself stored, and both are inside test_gpu_retention's bounds.  An `nn.sgd` step runs and moves both
conv1x1 layers; the `.t4` round trip gives the same forward bits."""
import numpy as np
import pytest

from test_gpu_bcast import Dev
from test_gpu_pool_geo_words import layer_tensors, operand
from test_gpu_retention import K, nan, ratios

pytestmark = pytest.mark.gpu

N, H, W, C, E, HEADS, D = 2, 4, 4, 8, 8, 2, 4
L = H * W
NET = "0.5 24 conv1x1 3 vector{ %d 1 1 } linear 0.5 8 conv1x1 flatten 10 linear softmax"


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def clean(out):
    assert "not supported" not in out and "failed" not in out and "error" not in out, out


def forward(vm, name, X):
    vm.store(X, "%d %d %d %d tensor constant x%s x%s" % (N, H, W, C, name, name)); vm.eval("drop")
    clean(vm.eval("%s x%s forward drop" % (name, name)))
    return [t.copy() for t in layer_tensors(vm, name, 7)]


def test_the_layer_inside_a_net(vm, t4k):
    rng = np.random.default_rng(5)
    vm.eval("%d %d %d %d nn.model %s constant rtn" % (N, H, W, C, NET % HEADS))
    assert "[  1] retentn: T4[2,4,4,24] #p=0 heads=2, decay=1\n[  2] conv2d : T4[2,4,4,8]" in vm.eval("rtn network drop")
    W0 = vm.fetch("rtn 0 nn.w").copy(); vm.eval("drop drop")
    W2 = vm.fetch("rtn 2 nn.w").copy(); vm.eval("drop drop")
    acts = forward(vm, "rtn", operand(rng, N, H, W, C))
    assert acts[1].shape == (N, H, W, 3 * E) and acts[2].shape == (N, H, W, E), [a.shape for a in acts]
    T = np.zeros((N, 1, 10, 1), np.float32); T[np.arange(N), 0, rng.integers(0, 10, N), 0] = 1.0
    vm.store(T, "%d 1 10 1 tensor constant trtn trtn" % N); vm.eval("drop")
    clean(vm.eval("rtn trtn backprop drop"))
    grads = layer_tensors(vm, "rtn", 4)                                  # layer i now holds dX of op i
    QKV, DY = acts[1].reshape(N, L, 3 * E), grads[2].reshape(N, L, E).copy()
    assert DY.any()
    dQ, dDY, dO, dS, dG = Dev(QKV), Dev(DY), Dev(nan(N * L * E)), Dev(nan(N * HEADS * D * D)), Dev(nan(3 * N * L * E))
    t4k.call("t4k_retention_fwd", dQ.p, dO.p, dS.p, N, L, HEADS, D, None)
    t4k.call("t4k_retention_bwd", dQ.p, dDY.p, dS.p, dG.p, N, L, HEADS, D, None)
    Y, G = dO.get(t4k, (N, L, E)), dG.get(t4k, (N, L, 3 * E))
    assert np.array_equal(acts[2].reshape(N, L, E).view(np.uint32), Y.view(np.uint32)), "the layer's output is not the entry's"
    assert np.array_equal(grads[1].reshape(N, L, 3 * E).view(np.uint32), G.view(np.uint32)), "the layer's dX is not the entry's"
    r = ratios(Y, G, QKV, DY, HEADS)
    assert all(r[k] <= K[k] for k in K), r
    clean(vm.eval("rtn 0.01 0.0 nn.sgd drop"))
    for i, F in ((0, W0), (2, W2)):
        w = vm.fetch("rtn %d nn.w" % i).copy(); vm.eval("drop drop")
        assert np.isfinite(w).all() and np.count_nonzero(w.ravel() != F.ravel()) > F.size // 2, i


def test_t4_file_round_trip(vm, tmp_path):
    """`save` writes the layer's line and no blob for it; `load` into a net built with another head count gives the same forward bits"""
    rng = np.random.default_rng(17)
    vm.eval("%d %d %d %d nn.model %s constant rtva" % (N, H, W, C, NET % 2))
    vm.eval("%d %d %d %d nn.model %s constant rtvb" % (N, H, W, C, NET % 1))
    f = str(tmp_path / "r.t4")
    vm.eval('rtva s" %s" save' % f); vm.eval("drop")
    blob = open(f, "rb").read()
    assert b"\nheads=2, decay=1retentn\n" in blob and blob.count(b"\n--- w.") == 3      # two conv1x1 and the linear layer: none for retention
    clean(vm.eval('rtvb s" %s" load' % f) + vm.eval("drop"))
    assert "heads=2, decay=1" in vm.eval("rtvb network drop")
    X = operand(rng, N, H, W, C)
    for x, y in zip(forward(vm, "rtva", X), forward(vm, "rtvb", X)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
