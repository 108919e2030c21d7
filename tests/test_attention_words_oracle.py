"""`N vector{ heads causal } linear`, the attention layer, on the CPU oracle VM - the product's host sources over the oracle's C-ABI, which has no
t4k_attention_plan / _fwd / _bwd: the word admits the layer and shapes it, `network` prints `attentn` with `heads=<h>, causal=<c>` and `#p=0`, channels that are
no 3 x heads x d with a head size the kernels take are refused and add nothing, `forward` / `backprop` refuse the layer by name and compute nothing, and the .t4
file carries the layer's line, from which `load` rebuilds it.  `128 linear` and `0.5 128 linear` print and build what they did.  On the parent commit every
vector form here prints "( N [bias] n -- ) for linear required!".  tests/test_gpu_attention_words.py runs the layer on the product VM."""
import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, words, shape="2 8 8 48"):
    return vm.eval("%s nn.model %s network drop" % (shape, words))


LINE = "NN Model[1/128]\n[  0] attentn: T4[2,8,8,48] #p=0 T4[2,8,8,16] heads=%d, causal=%d\n[  1] output : T4[2,8,8,16] #p=0 \n"
EMPTY = "NN Model[0/128]\n[  0] output : T4[2,8,8,%d] #p=0 \n"


def test_the_layer_line(vm):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, "2 vector{ 4 0 } linear")
    assert LINE % (4, 0) in txt and "required" not in txt, txt
    assert vm.eval("depth .").split()[0] == depth                           # ( N V -- N ): the vector is gone
    assert LINE % (2, 1) in net(vm, "2 vector{ 2 1 } linear")
    assert LINE % (1, 1) in net(vm, "2 vector{ 1 7 } linear")               # any non-zero cell is causal


def test_a_missing_causal_cell_means_0_and_further_cells_are_ignored(vm):
    assert LINE % (4, 0) in net(vm, "1 vector{ 4 } linear")
    assert LINE % (4, 1) in net(vm, "4 vector{ 4 1 9 9 } linear")


def test_channels_the_layer_cannot_split(vm):
    txt = net(vm, "2 vector{ 4 0 } linear", "2 8 8 50")                     # 50 is no multiple of 3
    assert "nn#iattention heads=4? channels=50" in txt and EMPTY % 50 in txt, txt
    txt = net(vm, "2 vector{ 5 0 } linear")                                 # 16 is no multiple of 5
    assert "nn#iattention heads=5? channels=48" in txt and EMPTY % 48 in txt, txt
    txt = net(vm, "2 vector{ 0 0 } linear")
    assert "nn#iattention heads=0? channels=48" in txt and EMPTY % 48 in txt, txt


def test_a_head_size_the_kernels_do_not_take(vm):
    txt = net(vm, "2 vector{ 8 0 } linear")                                 # d = 2
    assert "nn#iattention heads=8? channels=48" in txt and EMPTY % 48 in txt, txt
    txt = net(vm, "2 vector{ 1 0 } linear", "1 2 2 18")                     # d = 6: no multiple of 4
    assert "nn#iattention heads=1? channels=18" in txt, txt
    txt = net(vm, "2 vector{ 1 0 } linear", "1 2 2 396")                    # d = 132: above 128
    assert "nn#iattention heads=1? channels=396" in txt, txt
    assert "attentn: T4[1,2,2,384] #p=0 T4[1,2,2,128] heads=1, causal=0" in net(vm, "2 vector{ 1 0 } linear", "1 2 2 384")


def test_the_old_forms_print_and_build_what_they_did(vm):
    want = ("    WARN linear: treats in[2,8,8,48] as [2,1,3072,1]\nNN Model[1/128]\n[  0] linear : T4[2,8,8,48] #p=786688 T4[1,128,3072,1] T1[128] bias=%s, H=128\n"
            "[  1] output : T4[2,1,128,1] #p=0 \n")
    assert want % "1" in net(vm, "128 linear")
    assert want % "0.5" in net(vm, "0.5 128 linear")
    assert "( N [bias] n -- ) for linear required!" in vm.eval("linear")
    # a rank-2 tensor on top of a model is no head vector, and a vector without a model under it none either
    assert "required" in vm.eval("2 8 8 48 nn.model 1 1 matrix ones linear drop drop")
    assert "required" in vm.eval("2 vector{ 4 0 } linear drop")


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 8 8 48 nn.model 2 vector{ 4 1 } linear constant at1  2 8 8 48 tensor ones constant atx")
    txt = vm.eval("at1 atx forward drop")
    assert "nn#fattention failed: nn#fattention heads=4 not supported" in txt, txt
    txt = vm.eval("at1 2 8 8 16 tensor ones backprop drop")
    assert "nn#battention failed: nn#battention heads=4 not supported" in txt, txt
    assert LINE % (4, 1) in vm.eval("at1 network drop")                     # and the VM goes on


def test_save_and_load_rebuild_the_layer_from_its_line(vm, tmp_path):
    """no blobs: the file is the layer section and the closing `---`; loading into a fresh model whose attention layer has other heads and mask gives the saved
    layer's `network` text"""
    f = str(tmp_path / "at.t4")
    vm.eval("2 8 8 48 nn.model 2 vector{ 4 1 } linear constant at2")
    saved = vm.eval("at2 network drop")
    vm.eval('at2 s" %s" save' % f); vm.eval("drop")
    assert open(f, "rb").read() == b"\\ tensorForth v4.0 model\nheads=4, causal=1attentn\n\n---\n"
    vm.eval("2 8 8 48 nn.model 2 vector{ 2 0 } linear constant at3")
    assert LINE % (2, 0) in vm.eval("at3 network drop")
    txt = vm.eval('at3 s" %s" load' % f); vm.eval("drop")
    assert "format error" not in txt, txt
    assert LINE % (4, 1) in saved and vm.eval("at3 network drop") == saved
    # heads the layer's channels cannot have, and a line that is no attention line, are format errors and change nothing
    open(f, "wb").write(b"\\ tensorForth v4.0 model\nheads=5, causal=0attentn\n\n---\n")
    txt = vm.eval('at3 s" %s" load' % f); vm.eval("drop")
    assert "format error" in txt and vm.eval("at3 network drop") == saved, txt
    open(f, "wb").write(b"\\ tensorForth v4.0 model\nbias=1, H=16linear \n\n---\n")
    txt = vm.eval('at3 s" %s" load' % f); vm.eval("drop")
    assert "format error" in txt and vm.eval("at3 network drop") == saved, txt
