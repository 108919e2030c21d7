"""`N vector{ back mode } selu`, the add & norm layer, on the CPU oracle VM - the product's host sources over the oracle's C-ABI, which has no
t4k_addnorm_plan / _fwd / _bwd: the word admits the layer and shapes it, `network` prints `addnorm` with `back=<b>, mode=<m>` and `#p=` 2 C for a norm, 0
otherwise, every refusal prints its one line and adds nothing, `forward` / `backprop` refuse the layer by name and compute nothing, and the .t4 file carries the
layer's line and, for a norm, gamma and beta.  `N selu` and the scalar forms print and build what they did.  On the parent commit every vector form here prints
"( N -- ) no param needed!".  tests/test_gpu_addnorm_words.py runs the layer on the product VM."""
import struct

import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, words, shape="2 4 4 8"):
    return vm.eval("%s nn.model %s network drop" % (shape, words))


EMPTY = "NN Model[0/128]\n[  0] output : T4[2,4,4,%d] #p=0 \n"
MARK = "[  0] addnorm: T4[2,4,4,8] #p=0 back=0, mode=0\n"
PRE = ("2 vector{ 0 0 } selu  2 vector{ 0 1 } selu  0.5 24 conv1x1  2 vector{ 2 0 } linear  0.5 8 conv1x1  2 vector{ 4 0 } selu")
POST = "2 vector{ 0 0 } selu  0.5 8 conv2d relu 0.5 8 conv2d  2 vector{ 3 1 } selu  relu"


def test_the_layer_lines(vm):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, PRE)
    assert "no param" not in txt and "nn#iaddnorm" not in txt, txt
    assert ("NN Model[6/128]\n" + MARK +
            "[  1] addnorm: T4[2,4,4,8] #p=16 T1[8] T1[8] T4[2,4,4,8] back=0, mode=1\n"
            "[  2] conv2d : T4[2,4,4,8] #p=688 T4[8,1,1,24] T1[24] T4[2,4,4,8] bias=0.5, C=24, K=1, S=1, P=0\n"
            "[  3] attentn: T4[2,4,4,24] #p=0 T4[2,4,4,8] heads=2, causal=0\n"
            "[  4] conv2d : T4[2,4,4,8] #p=400 T4[8,1,1,8] T1[8] T4[2,4,4,8] bias=0.5, C=8, K=1, S=1, P=0\n"
            "[  5] addnorm: T4[2,4,4,8] #p=0 back=4, mode=0\n"
            "[  6] output : T4[2,4,4,8] #p=0 \n") in txt, txt
    assert vm.eval("depth .").split()[0] == depth                           # ( N V -- N ): the vector is gone
    txt = net(vm, POST)
    assert "[  4] addnorm: T4[2,4,4,8] #p=16 T1[8] T1[8] T4[2,4,4,8] back=3, mode=1\n[  5] relu   : T4[2,4,4,8] #p=256 T4[2,4,4,8] \n" in txt, txt
    assert "[  0] addnorm: T4[2,4,4,8] #p=16 T1[8] T1[8] T4[2,4,4,8] back=0, mode=2\n" in net(vm, "2 vector{ 0 2 } selu")


def test_a_missing_mode_cell_means_0_and_further_cells_are_ignored(vm):
    assert "NN Model[1/128]\n" + MARK in net(vm, "1 vector{ 0 } selu")
    assert "[  0] addnorm: T4[2,4,4,8] #p=16 T1[8] T1[8] T4[2,4,4,8] back=0, mode=1\n" in net(vm, "4 vector{ 0 1 9 9 } selu")
    assert "[  2] addnorm: T4[2,4,4,8] #p=0 back=1, mode=0\n" in net(vm, "2 vector{ 0 0 } selu relu 1 vector{ 1 } selu")


REFUSALS = [
    ("2 vector{ 0 3 } selu",                                                        "back=0 mode=3? mode 0..2", 0),
    ("2 vector{ 1 0 } selu",                                                        "back=1 mode=0? no layer there", 0),
    ("relu 2 vector{ 1 2 } selu",                                                   "back=1 mode=2? no layer there", 1),   # tensor 0 is the model's input, no layer's output
    ("2 vector{ 0 0 } selu 2 vector{ 5 0 } selu",                                   "back=5 mode=0? no layer there", 1),
    ("relu relu 2 vector{ 1 0 } selu",                                              "back=1 mode=0? layer 0 is no addnorm", 2),
    ("2 vector{ 0 0 } selu relu relu 2 vector{ 1 1 } selu",                         "back=1 mode=1? layer 1 is no addnorm", 3),
    ("2 vector{ 0 0 } selu 0.5 16 conv1x1 2 vector{ 1 0 } selu",                    "back=1 mode=0? shape", 2),
    ("2 vector{ 0 0 } selu 2 maxpool 2 vector{ 1 0 } selu",                         "back=1 mode=0? shape", 2),
    ("2 vector{ 0 0 } selu relu 2 vector{ 1 0 } selu relu 2 vector{ 3 0 } selu",    "back=3 mode=0? taken", 4),
]


@pytest.mark.parametrize("words,line,layers", REFUSALS, ids=[r[1].split("? ")[1].replace(" ", "_") + "_%d" % i for i, r in enumerate(REFUSALS)])
def test_refusals_add_nothing(vm, words, line, layers):
    txt = net(vm, words)
    assert txt.count("nn#iaddnorm") == 1 and "nn#iaddnorm " + line + "\n" in txt and "NN Model[%d/128]\n" % layers in txt, txt


def test_channels_the_plan_refuses(vm):
    for C, ok in ((8192, True), (8196, False), (2049, False), (2047, True)):
        for mode in (1, 2):
            txt = net(vm, "2 vector{ 0 %d } selu" % mode, "1 1 1 %d" % C)
            if ok:
                assert "addnorm: T4[1,1,1,%d] #p=%d " % (C, 2 * C) in txt, txt
            else:
                assert "nn#iaddnorm back=0 mode=%d? channels=%d\n" % (mode, C) in txt and "NN Model[0/128]" in txt, txt
        assert "addnorm: T4[1,1,1,%d] #p=0 back=0, mode=0" % C in net(vm, "2 vector{ 0 0 } selu", "1 1 1 %d" % C)     # a mark takes any C


def test_a_refused_add_leaves_its_source_untapped(vm):
    """the `taken` mark is set by an add that was admitted, not by one that was refused"""
    txt = net(vm, "2 vector{ 0 0 } selu 0.5 16 conv1x1 2 vector{ 1 0 } selu 0.5 8 conv1x1 2 vector{ 2 0 } selu")
    assert "? shape" in txt and "taken" not in txt and "[  3] addnorm: T4[2,4,4,8] #p=0 back=2, mode=0\n" in txt, txt


def test_chains_and_nested_spans(vm):
    txt = net(vm, "2 vector{ 0 0 } selu relu 2 vector{ 1 0 } selu relu 2 vector{ 1 1 } selu")       # block 2 taps block 1's add
    assert "nn#iaddnorm" not in txt and "[  4] addnorm: T4[2,4,4,8] #p=16 T1[8] T1[8] T4[2,4,4,8] back=1, mode=1\n" in txt, txt
    txt = net(vm, "2 vector{ 0 0 } selu relu 2 vector{ 0 0 } selu relu 2 vector{ 1 0 } selu relu 2 vector{ 5 2 } selu")      # an inner span inside an outer one
    assert "nn#iaddnorm" not in txt and "back=1, mode=0" in txt and "back=5, mode=2" in txt, txt


def test_the_old_forms_print_and_build_what_they_did(vm):
    assert "NN Model[1/128]\n[  0] selu   : T4[2,4,4,8] #p=256 T4[2,4,4,8] bias=0\n[  1] output : T4[2,4,4,8] #p=0 \n" in net(vm, "selu")
    assert "( N -- ) no param needed!" in vm.eval("selu")
    # a rank-2 tensor or a scalar on top of a model is no { back mode } vector, and a vector without a model under it none either
    assert "( N -- ) no param needed!" in vm.eval("2 4 4 8 nn.model 1 1 matrix ones selu drop drop")
    assert "( N -- ) no param needed!" in vm.eval("2 4 4 8 nn.model 3 selu drop drop")
    assert "( N -- ) no param needed!" in vm.eval("2 vector{ 0 0 } selu drop")


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 4 4 8 nn.model 2 vector{ 0 0 } selu relu 2 vector{ 1 2 } selu constant an1  2 4 4 8 tensor ones constant anx")
    txt = vm.eval("an1 anx forward drop")
    assert "nn#faddnorm failed: nn#faddnorm mode=0 not supported" in txt and "nn#faddnorm failed: nn#faddnorm mode=2 not supported" in txt, txt
    txt = vm.eval("an1 2 4 4 8 tensor ones backprop drop")
    assert "nn#baddnorm failed: nn#baddnorm mode=2 not supported" in txt and "nn#baddnorm failed: nn#baddnorm mode=0 not supported" in txt, txt
    assert "[  2] addnorm: T4[2,4,4,8] #p=16 T1[8] T1[8] T4[2,4,4,8] back=1, mode=2\n" in vm.eval("an1 network drop")      # and the VM goes on


def test_save_and_load(vm, tmp_path):
    """the file is the layer section, gamma and beta of the one norm, and the closing `---`; `load` reads them back, and refuses a file whose addnorm line is
    not the layer's own without changing anything"""
    f, g = str(tmp_path / "an.t4"), str(tmp_path / "an2.t4")
    words = "2 4 4 8 nn.model 2 vector{ 0 0 } selu relu 2 vector{ 1 1 } selu constant %s"
    head = b"\\ tensorForth v4.0 model\nback=0, mode=0addnorm\nrelu   \nback=1, mode=1addnorm\n"
    blob = lambda gam, bet: b"\n--- w.addnorm\n" + struct.pack("<8f", *gam) + b"\n--- b.addnorm\n" + struct.pack("<8f", *bet) + b"\n---\n"
    vm.eval(words % "an2")
    vm.eval('an2 s" %s" save' % f); vm.eval("drop")
    assert open(f, "rb").read() == head + blob([1.0] * 8, [0.0] * 8)
    # other values come back: load, save again, compare the bytes
    other = head + blob([2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0], [-1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -7.0, -8.0])
    open(f, "wb").write(other)
    vm.eval(words % "an3")
    txt = vm.eval('an3 s" %s" load' % f); vm.eval("drop")
    assert "format error" not in txt, txt
    vm.eval('an3 s" %s" save' % g); vm.eval("drop")
    assert open(g, "rb").read() == other
    # another span, another mode, or a line that is no addnorm line: format errors that change nothing
    for bad in (b"back=2, mode=1addnorm", b"back=1, mode=2addnorm", b"back=1, mode=1attentn", b"bias=0selu   ", b"back=1, mode=1addnormX"):
        open(f, "wb").write(head.replace(b"back=1, mode=1addnorm", bad) + blob([0.5] * 8, [0.5] * 8))
        txt = vm.eval('an3 s" %s" load' % f); vm.eval("drop")
        assert "format error" in txt, (bad, txt)
        vm.eval('an3 s" %s" save' % g); vm.eval("drop")
        assert open(g, "rb").read() == other, bad
    open(f, "wb").write(b"\\ tensorForth v4.0 model\nback=0, mode=0addnorm\n\n---\n")       # the file ends before the layer's line
    txt = vm.eval('an3 s" %s" load' % f); vm.eval("drop")
    assert "format error" in txt, txt
