"""The patch form of conv2d, `bias C0 4 vector{ K K 0 1 } conv2d` with K 8..32, on the CPU oracle VM - the product's host sources over the
oracle's C-ABI, which has no t4k_patch_fwd / _bwd: `add` admits the layer and shapes it (a floor grid, W0 from W1; the P cell's 0 is no padding), `network`
prints a convolution's line, `save` / `load` carry it, and `forward` keeps the refusal a run-time-geometry layer gets there.  Every other K > 7 keeps the
"1x1 to 7x7" line.  tests/test_gpu_patch_words.py runs the layer on the product VM."""
import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, layers, shape="2 35 48 3"):
    return vm.eval("%s nn.model %s network drop" % (shape, " ".join(layers)))


@pytest.mark.parametrize("K,shape,out", [(16, "2 35 48 3", "T4[2,2,3,8]"), (8, "2 35 48 3", "T4[2,4,6,8]"), (14, "2 31 42 3", "T4[2,2,3,8]"),
                                         (32, "2 70 96 3", "T4[2,2,3,8]")])
def test_layer_shapes_and_network_text(vm, K, shape, out):
    txt = net(vm, ["0.5 8 4 vector{ %d %d 0 1 } conv2d" % (K, K)], shape)
    assert "NN Model[1/128]" in txt and "bias=0.5, C=8, K=%d, S=%d, P=0\n" % (K, K) in txt and "[  1] output : " + out in txt, txt
    assert "T4[3,%d,%d,8] T1[8] T4[%s]" % (K, K, shape.replace(" ", ",")) in txt and ", D=" not in txt, txt


@pytest.mark.parametrize("cells", ["3 vector{ 16 16 0 }", "4 vector{ 16 16 0 0 }", "5 vector{ 16 16 0 1 0 }", "5 vector{ 16 16 0 1 1 }"])
def test_the_d_and_g_cells_may_be_absent_or_trivial(vm, cells):
    assert "K=16, S=16, P=0\n" in net(vm, ["0.5 8 %s conv2d" % cells])


@pytest.mark.parametrize("cells,text", [
    ("4 vector{ 8 1 1 1 }", "f=[8,8]? 1x1 to 7x7 supported only."),
    ("4 vector{ 8 8 1 1 }", "f=[8,8]? 1x1 to 7x7 supported only."),
    ("4 vector{ 16 8 0 1 }", "f=[16,16]? 1x1 to 7x7 supported only."),
    ("4 vector{ 16 16 0 2 }", "f=[16,16]? 1x1 to 7x7 supported only."),
    ("5 vector{ 16 16 0 1 2 }", "f=[16,16]? 1x1 to 7x7 supported only."),
    ("4 vector{ 33 33 0 1 }", "f=[33,33]? 1x1 to 7x7 supported only."),
    ("4 vector{ 36 36 0 1 }", "f=[36,36]? 1x1 to 7x7 supported only."),
    ("4 vector{ 32 32 0 1 }", "stride=32 padding=0 dilation=1?"),        # an image of 31 rows is lower than the patch
])
def test_refusals_of_add(vm, cells, text):
    txt = net(vm, ["0.5 8 %s conv2d" % cells], "2 31 48 3")
    assert "nn#iconv conv2d  " + text in txt and "NN Model[0/128]" in txt, txt      # nothing was added
    assert "output : T4[2,1,2,8]" in net(vm, ["0.5 8 4 vector{ 20 20 0 1 } conv2d"], "2 31 48 3")      # ... one patch of 20 fits it


def test_forward_and_backprop_keep_their_refusal_without_the_entries(vm):
    vm.eval("2 35 48 3 nn.model 0.5 8 4 vector{ 16 16 0 1 } conv2d constant p1  2 35 48 3 tensor constant px  2 2 3 8 tensor constant pt")
    assert "nn#fconv failed: nn#fconv kernel_size=16 stride=16 padding=0 not supported" in vm.eval("p1 px forward drop")
    assert "nn#bconv failed: nn#bconv kernel_size=16 stride=16 padding=0 not supported" in vm.eval("p1 pt backprop drop")


def test_t4_round_trip_reprints_the_network(vm, tmp_path):
    words = "2 35 48 3 nn.model 0.5 8 4 vector{ 16 16 0 1 } conv2d relu flatten 10 linear"
    vm.eval(words + " constant p2  " + words + " constant p3")
    f = str(tmp_path / "p.t4")
    vm.eval('p2 s" %s" save' % f); vm.eval("drop")
    assert b"K=16, S=16, P=0" in open(f, "rb").read()
    out = vm.eval('p3 s" %s" load' % f); out += vm.eval("drop")
    assert "error" not in out, out
    a, b = vm.eval("p2 network drop"), vm.eval("p3 network drop")
    assert a == b and "K=16, S=16, P=0\n" in a, (a, b)
    assert (vm.eval("p2 0 nn.w sum . drop drop") == vm.eval("p3 0 nn.w sum . drop drop"))
