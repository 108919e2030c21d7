"""`N 1 vector{ G } batchnorm`, the group / layer / instance norm layer, on the CPU oracle VM - the product's host sources over the oracle's
C-ABI, which has no t4k_groupnorm_fwd / _bwd: the word admits the layer and shapes it, `network` prints `G=<g>, eps=1e-05` in place of `mtum=<p>`, a group
count that does not divide the channels is refused and adds nothing, `forward` / `backprop` refuse the layer by name and compute nothing, and the .t4 file
carries gamma AND beta.  Plain `batchnorm` and `0.1 batchnorm` print what they did.  tests/test_gpu_groupnorm_words.py runs the layer on the product VM."""
import numpy as np
import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, words, shape="2 6 6 8"):
    return vm.eval("%s nn.model %s network drop" % (shape, words))


LINE = "NN Model[1/128]\n[  0] batchnm: T4[2,6,6,8] #p=608 T1[8] T1[8] T4[2,6,6,8] %s\n[  1] output : T4[2,6,6,8] #p=0 \n"      # #p = 4 x 8 + 2 x 6 x 6 x 8


@pytest.mark.parametrize("G", [1, 2, 8])
def test_the_layer_line(vm, G):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, "1 vector{ %d } batchnorm" % G)
    assert LINE % ("G=%d, eps=1e-05" % G) in txt and "required" not in txt, txt
    assert vm.eval("depth .").split()[0] == depth                           # ( N V -- N ): the vector is gone


def test_groups_that_do_not_divide_the_channels(vm):
    for g in (3, 0, 16):
        txt = net(vm, "1 vector{ %d } batchnorm" % g)
        assert "nn#ibatchnorm groups=%d? channels=8" % g in txt and "NN Model[0/128]\n[  0] output : T4[2,6,6,8] #p=0 \n" in txt, txt


def test_further_cells_are_ignored(vm):
    assert LINE % "G=2, eps=1e-05" in net(vm, "3 vector{ 2 7 9 } batchnorm")


def test_the_old_forms_print_what_they_did(vm):
    assert LINE % "mtum=0.1" in net(vm, "batchnorm")
    assert LINE % "mtum=0.1" in net(vm, "0.1 batchnorm")
    assert LINE % "mtum=0.5" in net(vm, "0.5 batchnorm")
    assert "( N n -- ) one param required!" in vm.eval("batchnorm")
    # a rank-2 tensor on top of a model is no group vector
    assert "required" in vm.eval("2 6 6 8 nn.model 1 1 matrix ones batchnorm drop drop")


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 6 6 8 nn.model 1 vector{ 2 } batchnorm relu 1 vector{ 8 } batchnorm constant g1  2 6 6 8 tensor ones constant gx")
    txt = vm.eval("g1 gx forward drop")
    for g in (2, 8):
        assert "nn#fbatchnorm failed: nn#fbatchnorm groups=%d not supported" % g in txt, txt
    txt = vm.eval("g1 2 6 6 8 tensor ones backprop drop")
    for g in (2, 8):
        assert "nn#bbatchnorm failed: nn#bbatchnorm groups=%d not supported" % g in txt, txt


def test_the_t4_file_carries_gamma_and_beta(vm, tmp_path):
    """the layer line carries the printer's text; `--- w.batchnm` and `--- b.batchnm` for the vector form, gamma alone for batchnorm proper (as the reference)"""
    f = str(tmp_path / "gn.t4")
    vm.eval('2 6 6 8 nn.model 1 vector{ 2 } batchnorm batchnorm constant g2')
    assert "format error" not in vm.eval('g2 s" %s" save drop' % f)
    blob = open(f, "rb").read()
    head, rest = blob.split(b"\n\n--- w.batchnm\n", 1)
    assert head == b"\\ tensorForth v4.0 model\nG=2, eps=1e-05batchnm\nmtum=0.1batchnm", head
    ones, zeros = np.ones(8, np.float32).tobytes(), np.zeros(8, np.float32).tobytes()
    assert rest == ones + b"\n--- b.batchnm\n" + zeros + b"\n--- w.batchnm\n" + ones + b"\n---\n", rest
    assert "format error" not in vm.eval('g2 s" %s" load drop' % f)
    # a file written for batchnorm proper (gamma alone) does not fit a model with the vector form in that place
    vm.eval('2 6 6 8 nn.model batchnorm batchnorm constant g3')
    vm.eval('g3 s" %s" save drop' % f)
    assert "format error" in vm.eval('g2 s" %s" load drop' % f)
