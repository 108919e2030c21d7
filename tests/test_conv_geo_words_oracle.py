"""conv2d layers of any K 1..7 with stride, padding and dilation on the CPU oracle VM - the product's host sources over the
oracle's C-ABI, which has no t4k_conv2d_geo_fwd / _bwd: `add` admits the layer and shapes it, `network` prints it (", D=" only where the layer
is dilated), and `forward` keeps the refusal it had.  tests/test_gpu_conv_geo_words.py runs the layers on the product VM."""
import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, layers, shape="2 12 12 3"):
    return vm.eval("%s nn.model %s network drop" % (shape, " ".join(layers)))


@pytest.mark.parametrize("opt,line,out", [
    ("3 2 1 1", "bias=0.5, C=8, K=3, S=2, P=1\n", "T4[2,6,6,8]"),
    ("7 2 3 1", "bias=0.5, C=8, K=7, S=2, P=3\n", "T4[2,6,6,8]"),
    ("2 2 1 1", "bias=0.5, C=8, K=2, S=2, P=1\n", "T4[2,7,7,8]"),
    ("3 1 2 2", "bias=0.5, C=8, K=3, S=1, P=2, D=2\n", "T4[2,12,12,8]"),
    ("3 1 1 2", "bias=0.5, C=8, K=3, S=1, P=1, D=2\n", "T4[2,10,10,8]"),      # the D cell was ignored before: this built an undilated 12x12 layer
    ("5 3 0 3", "bias=0.5, C=8, K=5, S=3, P=2, D=3\n", "T4[2,2,2,8]"),         # a P cell of 0 still means (K - 1) / 2; (12 + 4 - 12 - 1) / 3 + 1
    ("6 1 5 0", "bias=0.5, C=8, K=6, S=1, P=5\n", "T4[2,17,17,8]"),            # a D cell of 0 means 1
    ("4 4 1 1", "bias=0.5, C=8, K=4, S=4, P=1\n", "T4[2,3,3,8]"),
])
def test_layer_shapes_and_network_text(vm, opt, line, out):
    txt = net(vm, ["0.5 8 4 vector{ %s } conv2d" % opt])
    assert "NN Model[1/128]" in txt and line in txt and "[  1] output : " + out in txt, txt
    K = int(opt.split()[0])
    assert "T4[3,%d,%d,8] T1[8] T4[2,12,12,3]" % (K, K) in txt, txt


def test_d_is_printed_only_where_the_layer_is_dilated(vm):
    txt = net(vm, ["0.5 8 4 vector{ 3 2 1 1 } conv2d", "0.5 8 4 vector{ 3 1 2 2 } conv2d", "0.5 4 4 vector{ 7 2 3 1 } conv2d", "0.5 6 conv2d", "0.5 6 conv1x1"])
    assert txt.count(", D=") == 1 and "NN Model[5/128]" in txt, txt
    assert "[  3] conv2d : T4[2,3,3,4] #p=" in txt and "bias=0.5, C=6, K=3, S=1, P=1\n" in txt and "bias=0.5, C=6, K=1, S=1, P=0\n" in txt, txt


@pytest.mark.parametrize("opt,text", [
    ("8 1 1 1", "nn#iconv conv2d  f=[8,8]? 1x1 to 7x7 supported only."),
    ("0 1 1 1", "nn#iconv conv2d  f=[0,0]? 1x1 to 7x7 supported only."),
    ("3 5 1 1", "nn#iconv conv2d  stride=5 padding=1 dilation=1?"),
    ("3 0 1 1", "nn#iconv conv2d  stride=0 padding=1 dilation=1?"),
    ("3 1 1 5", "nn#iconv conv2d  stride=1 padding=1 dilation=5?"),
    ("3 1 3 1", "nn#iconv conv2d  stride=1 padding=3 dilation=1?"),
    ("3 1 5 2", "nn#iconv conv2d  stride=1 padding=5 dilation=2?"),
])
def test_refusals_of_add(vm, opt, text):
    txt = net(vm, ["0.5 8 4 vector{ %s } conv2d" % opt])
    assert text in txt and "NN Model[0/128]" in txt, txt                # nothing was added


def test_dconv2d_stays_4x4(vm):
    txt = net(vm, ["0.5 8 4 vector{ 3 2 1 1 } dconv2d"])
    assert "nn#iconv dconv2d f=[3,3]? 1x1, 3x3, 4x4, and 5x5 supported only." in txt and "NN Model[0/128]" in txt, txt
    txt = net(vm, ["0.5 8 dconv2d"])
    assert "bias=0.5, C=8, K=4, S=2, P=1\n" in txt and ", D=" not in txt and "T4[2,24,24,8]" in txt, txt


def test_forward_keeps_its_refusal_without_the_entries(vm):
    vm.eval("2 12 12 3 nn.model 0.5 8 4 vector{ 3 2 1 1 } conv2d 0.5 4 4 vector{ 7 2 3 1 } conv2d constant g1  2 12 12 3 tensor constant gx")
    txt = vm.eval("g1 gx forward drop")
    assert "nn#fconv failed: nn#fconv kernel_size=3 stride=2 padding=1 not supported" in txt, txt
    assert "nn#fconv failed: nn#fconv kernel_size=7 stride=2 padding=3 not supported" in txt, txt
    vm.eval("2 12 12 3 nn.model 0.5 8 4 vector{ 3 1 1 2 } conv2d constant g2")
    txt = vm.eval("g2 gx forward drop")
    assert "nn#fconv failed: nn#fconv kernel_size=3 stride=1 padding=1 dilation=2 not supported" in txt, txt
    vm.eval("2 3 3 4 tensor constant gt")
    txt = vm.eval("g1 gt backprop drop")
    assert "nn#bconv failed: nn#bconv kernel_size=7 stride=2 padding=3 not supported" in txt, txt


def test_a_3_1_1_net_prints_what_it_printed(vm):
    txt = net(vm, ["0.5 8 conv2d", "2 maxpool", "relu", "0.5 4 4 vector{ 5 1 2 1 } conv2d"])
    want = """NN Model[4/128]
[  0] conv2d : T4[2,12,12,3] #p=1312 T4[3,3,3,8] T1[8] T4[2,12,12,3] bias=0.5, C=8, K=3, S=1, P=1
[  1] maxpool: T4[2,12,12,8] #p=0 2x2
[  2] relu   : T4[2,6,6,8] #p=576 T4[2,6,6,8] 
[  3] conv2d : T4[2,6,6,8] #p=2184 T4[8,5,5,4] T1[4] T4[2,6,6,8] bias=0.5, C=4, K=5, S=1, P=2
[  4] output : T4[2,6,6,4] #p=0 
"""
    assert want in txt, txt
    vm.eval("2 12 12 3 nn.model 0.5 8 conv2d constant g3")
    out = vm.eval("g3 gx forward drop g3 1 n@ sum . drop drop")
    assert "not supported" not in out and "failed" not in out, out
