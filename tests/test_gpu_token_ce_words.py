"""`N 1 softmax`, the per-token softmax / cross-entropy head, on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so).

The issue's net - ids in a `N 4 4 1` input, an 11-row embedding, a 1x1 projection, attention, a 1x1 projection to 11 classes, `1 softmax` - trains against
id targets `[N,4,4,1]` that include padding: the head's output is inside f64_witness.softmax of the logits it read, `backprop` leaves P - onehot (zeros for
padding) over the head's input, bit-equal to t4k_token_ce_bwd, and changes neither P nor the ids; `loss.ce`, `nn.loss` and `nn.hit` report the token values of the float64 rule.  Inside a net the layer's backward is the Jacobian product (test_gpu_token_ce.jacobian_witness).  A dense one-hot target gives the id
form's gradient bit for bit, and one `nn.adam` step from either leaves the same weights.  The head is one launch each way: the difference of two nets."""
import numpy as np
import pytest

import f64_witness as wt
from test_gpu_bcast import Dev
from test_gpu_pool_geo import lcount
from test_gpu_pool_geo_words import layer_tensors, operand
from test_gpu_token_ce import PADS, bits, id_rule, jacobian_witness, lse_witness, nan
from test_token_ce_words_oracle import SCRIPT

pytestmark = pytest.mark.gpu

F = np.float32
V = 11


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=3)
    yield v
    v.close()


def clean(out):
    assert "not supported" not in out and "failed" not in out and "wrong shape" not in out and "nn#i" not in out, out


def tensor(vm, name, a):
    vm.store(a, "%d %d %d %d tensor constant %s %s" % (a.shape + (name, name))); vm.eval("drop")


def scalar(vm, words):
    """the scalar `words` leave on top of the stack, at full precision: added onto a zero vector and fetched"""
    clean(vm.eval(words + " 1 vector zeros swap +"))
    v = float(vm.fetch().ravel()[0]); vm.eval("drop drop drop")
    return v


def targets(rng, N):
    ids = rng.integers(0, V, (N, 4, 4, 1)).astype(F)
    pads = PADS.copy(); pads[2] = V
    ids.ravel()[1::3] = np.resize(pads, ids.size)[1::3]
    ids.ravel()[0] += F(0.75)
    return ids


@pytest.mark.parametrize("N", [2, 24])
def test_the_head_trains_against_id_targets(vm, t4k, N):
    m = "tsh%d" % N
    rng = np.random.default_rng(N)
    clean(vm.eval(SCRIPT.replace("2 4 4 1 nn.model", "%d 4 4 1 nn.model" % N) + " constant " + m))
    X, IDS = rng.integers(0, V, (N, 4, 4, 1)).astype(F), targets(rng, N)
    tensor(vm, "x" + m, X); tensor(vm, "t" + m, IDS)
    clean(vm.eval("%s x%s forward drop" % (m, m)))
    acts = layer_tensors(vm, m, 6)
    T = N * 16
    logits, P = acts[4].reshape(T, V), acts[5].reshape(T, V)
    wt.check("P", P, wt.softmax(logits))
    valid, k = id_rule(IDS.ravel(), V)
    assert valid.any() and not valid.all()
    nll = np.where(valid, -np.log(wt.f64(P)[np.arange(T), k]), 0.0)
    loss = wt.W([nll.sum() / N], [(wt.C_SUM * T + wt.ULP_LOG + 2.0) * np.abs(nll).sum() / N], 1, 1.0)    # a T-term sum in any order, a log a term, the division
    for word in ("loss.ce", "nn.loss"):
        wt.check(word, [scalar(vm, "%s t%s %s" % (m, m, word))], loss); vm.eval("drop")
    vm.store(IDS, "%s %d 4 4 1 tensor" % (m, N)); clean(vm.eval("nn.onehot="))           # (a tensor of its own: the model keeps it)
    assert scalar(vm, "nn.hit") == int(np.sum(valid & (np.argmax(logits, -1) == k)))
    wt.check("loss.ce of the model's own target", [scalar(vm, "loss.ce")], loss)
    clean(vm.eval("backprop drop"))                                                        # N backprop: the model's own target
    grads = layer_tensors(vm, m, 6)
    dP, dI, dD = Dev(P), Dev(IDS), Dev(nan(T * V))
    t4k.call("t4k_token_ce_bwd", dP.p, dI.p, dD.p, T, V, None)
    DX = dD.get(t4k, (T, V))
    want = P.copy(); want[np.arange(T), k] -= F(1.0); want[~valid] = 0.0
    assert bits(grads[4], DX) and bits(DX, want), "the head's dX is not the entry's"
    assert bits(grads[5], P), "backprop changed P"
    assert bits(vm.fetch("t" + m), IDS), "backprop changed the ids"
    vm.eval("drop")


def test_inside_a_net_the_backward_is_the_jacobian_product(vm, t4k):
    N, C = 3, 6
    rng = np.random.default_rng(7)
    clean(vm.eval("%d 4 4 %d nn.model 1 softmax 0.5 5 conv1x1 constant tsm" % (N, C)))
    X, TG = operand(rng, N, 4, 4, C), operand(rng, N, 4, 4, 5)
    tensor(vm, "xtsm", X); tensor(vm, "ttsm", TG)
    clean(vm.eval("tsm xtsm forward drop"))
    P = layer_tensors(vm, "tsm", 2)[1]
    wt.check("P", P.reshape(-1, C), wt.softmax(X.reshape(-1, C)))
    clean(vm.eval("tsm ttsm backprop drop"))
    grads = layer_tensors(vm, "tsm", 2)
    dy = grads[1].reshape(-1, C)                                           # what the convolution left for the layer
    assert dy.any()
    lse, dl = lse_witness(X.reshape(-1, C))
    wt.check("dx", grads[0].reshape(-1, C), jacobian_witness(X.reshape(-1, C), dy, lse, dl))
    assert not bits(grads[0], dy), "a pass-through"


def test_a_dense_target_gives_the_id_forms_gradient_and_adam_step(vm):
    N, C = 2, 6
    rng = np.random.default_rng(9)
    X = operand(rng, N, 4, 4, C)
    IDS = rng.integers(0, V, (N, 4, 4, 1)).astype(F)
    HOT = np.zeros((N, 4, 4, V), F); np.put_along_axis(HOT, IDS.astype(np.int64), 1.0, -1)
    tensor(vm, "xtsd", X); tensor(vm, "itsd", IDS); tensor(vm, "htsd", HOT)
    Wc, Bc = operand(rng, C, 1, 1, V) / F(3.0), operand(rng, V)
    res = []
    for m, tg in (("tsda", "itsd"), ("tsdb", "htsd")):
        clean(vm.eval("%d 4 4 %d nn.model 0.5 %d conv1x1 1 softmax constant %s" % (N, C, V, m)))
        vm.store(Wc, "%s 0 nn.w" % m); vm.eval("drop drop"); vm.store(Bc, "%s 0 nn.b" % m); vm.eval("drop drop")
        clean(vm.eval("%s xtsd forward %s backprop drop" % (m, tg)))
        dx = layer_tensors(vm, m, 2)[1].copy()
        clean(vm.eval("%s 0.001 0.9 nn.adam drop" % m))
        w = vm.fetch("%s 0 nn.w" % m).copy(); vm.eval("drop drop")
        b = vm.fetch("%s 0 nn.b" % m).copy(); vm.eval("drop drop")
        res.append((dx, w, b))
    for a, b in zip(*res):
        assert bits(a, b)
    assert np.count_nonzero(res[0][1].ravel() != Wc.ravel()) > Wc.size // 2 and np.isfinite(res[0][1]).all()


def test_the_head_is_one_launch_each_way(vm, t4k):
    def launches(w):
        clean(vm.eval(w)); l0 = lcount(t4k); clean(vm.eval(w)); return lcount(t4k) - l0
    rng = np.random.default_rng(3)
    vm.eval("2 4 4 %d nn.model sigmoid sigmoid 1 softmax constant tsla  2 4 4 %d nn.model sigmoid sigmoid constant tslb" % (V, V))
    tensor(vm, "xtsl", operand(rng, 2, 4, 4, V)); tensor(vm, "itsl", rng.integers(0, V, (2, 4, 4, 1)).astype(F))
    fa, fb = launches("tsla xtsl forward drop"), launches("tslb xtsl forward drop")
    ba, bb = launches("tsla itsl backprop drop"), launches("tslb xtsl backprop drop")
    print("forward launches %d against %d, backward %d against %d" % (fa, fb, ba, bb))
    assert fa - fb == 1 and ba - bb == 1, (fa, fb, ba, bb)
