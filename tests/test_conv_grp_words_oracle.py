"""grouped and depthwise conv2d layers through the fifth cell of the option vector, `vector{ K S P D G } conv2d`, on the CPU oracle VM -
the product's host sources over the oracle's C-ABI, which has no t4k_conv2d_grp_fwd / _bwd: `add` admits the layer and shapes it (the filter and its
gradient are T4(C1 / G, K, K, C0)), `network` prints it (", G=" only where the layer is grouped, behind ", D=" where that is there), `save` writes the same
text into the `.t4` layer section, and `forward` / `backprop` refuse it by name.  No word is added: a 4-cell vector and the scalar forms build what they
built.  tests/test_gpu_conv_grp_words.py runs the layers on the product VM.

`#p=` is the sum of the layer's five tensors, as on every line of `network` (filter, bias, their two gradients and the dX scratch tensor): a depthwise 3x3
over 2x12x12x8 prints 72 + 8 + 72 + 8 + 2304 = 2464 where the dense layer prints 576 + 8 + 576 + 8 + 2304 = 3472."""
import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, layers, shape="2 12 12 8"):
    return vm.eval("%s nn.model %s network drop" % (shape, " ".join(layers)))


def test_depthwise_layer_line(vm):
    txt = net(vm, ["0.5 8 5 vector{ 3 1 1 1 8 } conv2d"])
    assert "NN Model[1/128]" in txt, txt
    assert "T4[1,3,3,8] T1[8] T4[2,12,12,8]" in txt, txt
    assert "bias=0.5, C=8, K=3, S=1, P=1, G=8\n" in txt, txt
    assert "[  0] conv2d : T4[2,12,12,8] #p=2464 T4[1,3,3,8] T1[8] T4[2,12,12,8] bias=0.5, C=8, K=3, S=1, P=1, G=8\n" in txt, txt
    assert "[  1] output : T4[2,12,12,8]" in txt, txt


@pytest.mark.parametrize("c0,opt,filt,line,out", [
    (16, "3 2 1 1 4", "T4[2,3,3,16] T1[16]", "bias=0.5, C=16, K=3, S=2, P=1, G=4\n", "T4[2,6,6,16]"),          # 8 -> 16 in 4 groups: 2 inputs, 4 outputs a group
    (8, "3 1 2 2 2", "T4[4,3,3,8] T1[8]", "bias=0.5, C=8, K=3, S=1, P=2, D=2, G=2\n", "T4[2,12,12,8]"),          # dilated and grouped: both say so, D first
    (16, "3 2 1 1 8", "T4[1,3,3,16] T1[16]", "bias=0.5, C=16, K=3, S=2, P=1, G=8\n", "T4[2,6,6,16]"),          # depthwise with multiplier 2
    (12, "3 1 1 1 4", "T4[2,3,3,12] T1[12]", "bias=0.5, C=12, K=3, S=1, P=1, G=4\n", "T4[2,12,12,12]"),        # 2 inputs, 3 outputs a group
    (4, "1 1 0 1 4", "T4[2,1,1,4] T1[4]", "bias=0.5, C=4, K=1, S=1, P=0, G=4\n", "T4[2,12,12,4]"),              # a grouped 1x1
])
def test_grouped_layer_lines(vm, c0, opt, filt, line, out):
    txt = net(vm, ["0.5 %d 5 vector{ %s } conv2d" % (c0, opt)])
    assert "NN Model[1/128]" in txt and filt + " T4[2,12,12,8] " + line in txt and "[  1] output : " + out in txt, txt


@pytest.mark.parametrize("layer", ["0.5 8 5 vector{ 3 1 1 1 0 } conv2d", "0.5 8 5 vector{ 3 1 1 1 1 } conv2d", "0.5 8 4 vector{ 3 1 1 1 } conv2d", "0.5 8 conv2d"])
def test_a_g_cell_of_0_or_1_is_dense(vm, layer):
    txt = net(vm, [layer])
    assert ", G=" not in txt, txt
    assert "[  0] conv2d : T4[2,12,12,8] #p=3472 T4[8,3,3,8] T1[8] T4[2,12,12,8] bias=0.5, C=8, K=3, S=1, P=1\n" in txt, txt


@pytest.mark.parametrize("c0,g,text", [
    (8, 3, "nn#iconv conv2d  groups=3? in=8 out=8"),                     # C1 % G
    (6, 4, "nn#iconv conv2d  groups=4? in=8 out=6"),                     # C0 % G
    (16, 16, "nn#iconv conv2d  groups=16? in=8 out=16"),                 # G > C1
    (8, 65535, "nn#iconv conv2d  groups=65535? in=8 out=8"),
])
def test_refusals_of_add(vm, c0, g, text):
    txt = net(vm, ["0.5 %d 5 vector{ 3 1 1 1 %d } conv2d" % (c0, g)])
    assert text in txt and "NN Model[0/128]" in txt, txt                # nothing was added


def test_a_geometry_refusal_comes_first_and_reads_as_before(vm):
    txt = net(vm, ["0.5 8 5 vector{ 3 5 1 1 8 } conv2d"])
    assert "nn#iconv conv2d  stride=5 padding=1 dilation=1?" in txt and "NN Model[0/128]" in txt, txt


def test_dconv2d_ignores_the_cell(vm):
    with_g = net(vm, ["0.5 8 5 vector{ 4 2 1 1 8 } dconv2d"])
    without = net(vm, ["0.5 8 4 vector{ 4 2 1 1 } dconv2d"])
    assert ", G=" not in with_g and "T4[8,4,4,8] T1[8]" in with_g and "bias=0.5, C=8, K=4, S=2, P=1\n" in with_g, with_g
    strip = lambda t: t[t.index("NN Model"):]
    assert strip(with_g) == strip(without)
    txt = net(vm, ["0.5 8 5 vector{ 3 2 1 1 8 } dconv2d"])
    assert "nn#iconv dconv2d f=[3,3]? 1x1, 3x3, 4x4, and 5x5 supported only." in txt and "NN Model[0/128]" in txt, txt


def test_forward_and_backprop_refuse_by_name(vm):
    vm.eval("2 12 12 8 nn.model 0.5 8 5 vector{ 3 1 1 1 8 } conv2d constant q1  2 12 12 8 tensor constant qx")
    txt = vm.eval("q1 qx forward drop")
    assert "nn#fconv failed: nn#fconv kernel_size=3 stride=1 padding=1 groups=8 not supported" in txt, txt
    txt = vm.eval("q1 qx backprop drop")
    assert "nn#bconv failed: nn#bconv kernel_size=3 stride=1 padding=1 groups=8 not supported" in txt, txt
    vm.eval("2 12 12 8 nn.model 0.5 8 5 vector{ 3 1 2 2 2 } conv2d constant q2")
    txt = vm.eval("q2 qx forward drop")
    assert "nn#fconv failed: nn#fconv kernel_size=3 stride=1 padding=2 dilation=2 groups=2 not supported" in txt, txt
    # an ungrouped layer beside them keeps the line it had, and the reference's own geometry still runs
    vm.eval("2 12 12 8 nn.model 0.5 8 4 vector{ 3 2 1 1 } conv2d constant q3")
    txt = vm.eval("q3 qx forward drop")
    assert "nn#fconv failed: nn#fconv kernel_size=3 stride=2 padding=1 not supported" in txt and "groups" not in txt, txt
    vm.eval("2 12 12 8 nn.model 0.5 8 5 vector{ 3 1 1 1 1 } conv2d constant q4")
    out = vm.eval("q4 qx forward drop q4 1 n@ sum . drop drop")
    assert "not supported" not in out and "failed" not in out, out


def test_t4_layer_section_carries_the_text(vm, tmp_path):
    vm.eval("2 12 12 8 nn.model 0.5 8 5 vector{ 3 1 1 1 8 } conv2d 0.5 16 conv1x1 0.5 16 5 vector{ 3 1 2 2 2 } conv2d constant q5")
    a = str(tmp_path / "g.t4")
    vm.eval('q5 s" %s" save' % a); vm.eval("drop")
    blob = open(a, "rb").read()
    head = blob.split(b"\n\n")[0].decode().split("\n")
    assert head == ["\\ tensorForth v4.0 model", "bias=0.5, C=8, K=3, S=1, P=1, G=8conv2d ", "bias=0.5, C=16, K=1, S=1, P=0conv2d ",
                    "bias=0.5, C=16, K=3, S=1, P=2, D=2, G=2conv2d "], head
    # the blobs are the smaller tensors: 72 + 8, 128 + 16 and 8 * 9 * 16 + 16 floats
    assert len(blob) < len("\n".join(head)) + 4 * (80 + 144 + 1168) + 400, len(blob)
