"""`N 1 softmax`, the per-token softmax / cross-entropy head, on the CPU oracle VM - the product's host sources over the oracle's C-ABI, which
has no t4k_token_* entries: the word consumes the mask and adds a `toksmax` layer of the input's shape with STAT T4[N,H,W,2] and `#p=0`, every refusal
prints its one line and adds nothing, `forward` / `backprop` and the id-target words refuse the layer by name and compute nothing, and the .t4 file carries
the layer's line.  Every other operand set of `softmax` prints and builds what it did.  On the parent commit `N 1 softmax` prints
"( N -- ) no param needed!" and leaves the scalar.  tests/test_gpu_token_ce_words.py runs the layer on the product VM."""
import pytest

from vm_util import OracleVM

SCRIPT = "2 4 4 1 nn.model  3 vector{ 11 8 1 } upsample  0.5 24 conv1x1  2 vector{ 2 1 } linear  0.5 11 conv1x1  1 softmax"


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, words, shape="2 4 4 3"):
    return vm.eval("%s nn.model %s network drop" % (shape, words))


def test_the_layer_line_and_the_stack_effect(vm):
    depth = vm.eval("depth .").split()[0]
    txt = vm.eval(SCRIPT + " network drop")
    assert "no param needed" not in txt and "nn#itoksmax" not in txt, txt
    assert ("NN Model[5/128]\n" in txt and "[  3] conv2d : T4[2,4,4,8] #p=454 T4[8,1,1,11] T1[11] T4[2,4,4,8] bias=0.5, C=11, K=1, S=1, P=0\n"
            "[  4] toksmax: T4[2,4,4,11] #p=0 T4[2,4,4,2] axes=1\n[  5] output : T4[2,4,4,11] #p=0 \n") in txt, txt
    assert vm.eval("depth .").split()[0] == depth                           # ( N m -- N ): the mask is gone
    # inside a net: the same line, the next layer sees the input's shape
    assert "[  0] toksmax: T4[2,4,4,3] #p=0 T4[2,4,4,2] axes=1\n[  1] relu   : T4[2,4,4,3] #p=96 T4[2,4,4,3] \n" in net(vm, "1 softmax relu")


@pytest.mark.parametrize("shape,line", [("2 4 4 1", "axes=1? channels"), ("1 1 1 16777220", "axes=1? shape")], ids=["channels", "shape"])
def test_refusals_add_nothing_and_consume_the_mask(vm, shape, line):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, "1 softmax", shape)
    assert txt.count("nn#itoksmax") == 1 and "nn#itoksmax " + line + "\n" in txt and "NN Model[0/128]\n" in txt, txt
    assert vm.eval("depth .").split()[0] == depth


def test_the_other_operand_sets_print_and_build_what_they_did(vm):
    assert "NN Model[1/128]\n[  0] softmax: T4[2,4,4,3] #p=48 T4[1,4,4,3] \n[  1] output : T4[2,4,4,3] #p=0 \n" in net(vm, "softmax")     # N softmax
    assert "+0.3333" in vm.eval("1 1 2 3 tensor ones 1 softmax . ")                                                                         # T m softmax
    assert "+0.1667" in vm.eval("1 1 2 3 tensor ones softmax . ")                                                                           # T softmax
    assert "softmax: axes 1..15?" in vm.eval("1 1 2 3 tensor ones 16 softmax drop")
    for m in ("7", "1.5", "0"):                                             # any other mask over a model: the text and the scalar stay (m = 6 is pinned elsewhere)
        out = vm.eval("2 4 4 3 nn.model %s softmax" % m)
        assert "( N -- ) no param needed!" in out and "nn#itoksmax" not in out and vm.eval(".").split()[0] == m and "NN Model[0/128]\n" in vm.eval("network drop")
    out = vm.eval("1 1 softmax . .")                                                                                                        # a scalar over a scalar
    assert "( N -- ) no param needed!" in out and out.split("!")[1].split()[:2] == ["1", "1"], out


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 4 4 3 nn.model 1 softmax constant ts1  2 4 4 3 tensor ones constant tsx  2 4 4 1 tensor ones constant tsi")
    assert "nn#ftoksmax failed: nn#ftoksmax axes=1 not supported" in vm.eval("ts1 tsx forward drop")
    assert "nn#btoksmax failed: nn#btoksmax axes=1 not supported" in vm.eval("ts1 tsi backprop drop")
    for words in ("ts1 tsi loss.ce . drop", "ts1 tsi nn.loss . drop", "ts1 2 4 4 1 tensor ones nn.onehot= nn.hit . drop"):
        out = vm.eval(words)
        assert "nn#ftoksmax failed: nn#ftoksmax score not supported" in out and "shape" not in out and "dimension" not in out, out
    assert "nn::loss model output shape[2,4,4,3] != tgt[2,4,4,1]" in vm.eval("ts1 tsi loss.mse . drop")     # through another loss: the shape message
    assert "[  0] toksmax: T4[2,4,4,3] #p=0 T4[2,4,4,2] axes=1\n" in vm.eval("ts1 network drop")          # and the VM goes on


def test_save_and_load(vm, tmp_path):
    f, g = str(tmp_path / "ts.t4"), str(tmp_path / "ts2.t4")
    vm.eval("2 4 4 3 nn.model 1 softmax constant ts2")
    vm.eval('ts2 s" %s" save' % f); vm.eval("drop")
    want = b"\\ tensorForth v4.0 model\naxes=1toksmax\n\n---\n"
    assert open(f, "rb").read() == want
    txt = vm.eval('ts2 s" %s" load' % f); vm.eval("drop")
    assert "format error" not in txt, txt
    assert "[  0] toksmax: T4[2,4,4,3] #p=0 T4[2,4,4,2] axes=1\n" in vm.eval("ts2 network drop")
    for bad in (b"axes=7toksmax", b"softmax", b"axes=1toksmaxX", b"axes=1addnorm"):       # a line that is not the layer's own: one format error, nothing changes
        open(f, "wb").write(want.replace(b"axes=1toksmax", bad))
        txt = vm.eval('ts2 s" %s" load' % f); vm.eval("drop")
        assert txt.count("format error") == 1, (bad, txt)
        vm.eval('ts2 s" %s" save' % g); vm.eval("drop")
        assert open(g, "rb").read() == want, bad
