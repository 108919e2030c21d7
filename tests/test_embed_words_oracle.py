"""`N vector{ V E pos } upsample`, the embedding layer, on the CPU oracle VM - the product's host sources over the oracle's C-ABI, which has no
t4k_embed_plan / _fwd / _bwd: the word admits the layer and shapes it, `network` prints `embed  ` with `vocab=<V>, pos=<p>` and `#p=` V E + pos L E, every
refusal prints its one line and adds nothing, `forward` / `backprop` refuse the layer by name and compute nothing, and the .t4 file carries the layer's line,
TABLE and POS.  The scalar forms `n upsample` and `m n upsample` print and build what they did.  On the parent commit every vector form here prints
"( N [mtum] n -- ) for upsample required?".  tests/test_gpu_embed_words.py runs the layer on the product VM."""
import struct

import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, words, shape="2 4 4 1"):
    return vm.eval("%s nn.model %s network drop" % (shape, words))


TOKPOS = "[  0] embed  : T4[2,4,4,1] #p=216 T4[1,11,8,1] T4[1,4,4,8] vocab=11, pos=1\n"
TOK = "[  0] embed  : T4[2,4,4,1] #p=88 T4[1,11,8,1] vocab=11, pos=0\n"


def test_the_layer_lines(vm):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, "3 vector{ 11 8 1 } upsample  0.5 24 conv1x1  2 vector{ 2 1 } linear  0.5 8 conv1x1 flatten 10 linear softmax")
    assert "required" not in txt and "nn#iembed" not in txt, txt
    assert ("NN Model[7/128]\n" + TOKPOS +
            "[  1] conv2d : T4[2,4,4,8] #p=688 T4[8,1,1,24] T1[24] T4[2,4,4,8] bias=0.5, C=24, K=1, S=1, P=0\n"
            "[  2] attentn: T4[2,4,4,24] #p=0 T4[2,4,4,8] heads=2, causal=1\n") in txt, txt
    assert vm.eval("depth .").split()[0] == depth                           # ( N V -- N ): the vector is gone
    assert "NN Model[1/128]\n" + TOK + "[  1] output : T4[2,4,4,8] #p=0 \n" in net(vm, "3 vector{ 11 8 0 } upsample")
    # position mode behind a patch convolution: out = x + pos, same shape; the E cell 0 or the channels
    for cell in (0, 8):
        txt = net(vm, "0.5 8 3 vector{ 4 4 0 } conv2d  3 vector{ 0 %d 1 } upsample" % cell, "2 8 8 3")
        assert ("NN Model[2/128]\n[  0] conv2d : T4[2,8,8,3] #p=1168 T4[3,4,4,8] T1[8] T4[2,8,8,3] bias=0.5, C=8, K=4, S=4, P=1\n"
                "[  1] embed  : T4[2,2,2,8] #p=32 T4[1,2,2,8] vocab=0, pos=1\n[  2] output : T4[2,2,2,8] #p=0 \n") in txt, txt
    assert "[  0] embed  : T4[2,4,4,3] #p=48 T4[1,4,4,3] vocab=0, pos=1\n" in net(vm, "3 vector{ 0 0 1 } upsample", "2 4 4 3")     # ... or first
    assert "[  0] embed  : T4[2,4,4,1] #p=140000 T4[1,70000,2,1] vocab=70000, pos=0\n" in net(vm, "2 vector{ 70000 2 } upsample")  # V is no 16-bit cell


def test_missing_cells_mean_0_and_further_cells_are_ignored(vm):
    assert "NN Model[1/128]\n" + TOK in net(vm, "2 vector{ 11 8 } upsample")
    assert "NN Model[1/128]\n" + TOKPOS in net(vm, "5 vector{ 11 8 1 9 9 } upsample")
    assert "nn#iembed vocab=11 dim=0 pos=0? dim\n" in net(vm, "1 vector{ 11 } upsample")


REFUSALS = [
    ("3 vector{ 11 8 2 } upsample",                      "2 4 4 1", "vocab=11 dim=8 pos=2? pos 0..1", 0),
    ("3 vector{ 0 0 0 } upsample",                       "2 4 4 1", "vocab=0 dim=0 pos=0? no table", 0),
    ("relu 3 vector{ 11 8 1 } upsample",                 "2 4 4 1", "vocab=11 dim=8 pos=1? not the first layer", 1),
    ("3 vector{ 11 8 1 } upsample",                      "2 4 4 3", "vocab=11 dim=8 pos=1? ids have 1 channel", 0),
    ("3 vector{ 11 0 1 } upsample",                      "2 4 4 1", "vocab=11 dim=0 pos=1? dim", 0),
    ("3 vector{ 0 5 1 } upsample",                       "2 4 4 3", "vocab=0 dim=5 pos=1? dim is the channels", 0),
    ("relu 3 vector{ 0 4 1 } upsample",                  "2 4 4 3", "vocab=0 dim=4 pos=1? dim is the channels", 1),
    ("3 vector{ 16000000 200 0 } upsample",              "2 4 4 1", "vocab=16000000 dim=200 pos=0? shape", 0),     # V E >= 2^31: what the planner refuses
]


@pytest.mark.parametrize("words,shape,line,layers", REFUSALS, ids=[r[2].split("? ")[1].replace(" ", "_") + "_%d" % i for i, r in enumerate(REFUSALS)])
def test_refusals_add_nothing(vm, words, shape, line, layers):
    txt = net(vm, words, shape)
    assert txt.count("nn#iembed") == 1 and "nn#iembed " + line + "\n" in txt and "NN Model[%d/128]\n" % layers in txt, txt


def test_the_scalar_forms_print_and_build_what_they_did(vm):
    txt = net(vm, "2 upsample 2 3 upsample")
    assert "NN Model[2/128]\n[  0] upsampl: T4[2,4,4,1] #p=0 2x2 nearest\n[  1] upsampl: T4[2,8,8,1] #p=0 3x3 bilinear\n[  2] output : T4[2,24,24,1] #p=0 \n" in txt, txt
    assert "( N [mtum] n -- ) for upsample required?" in vm.eval("upsample")
    # a rank-2 tensor on top of a model is no { V E pos } vector, and a vector without a model under it none either
    assert "( N [mtum] n -- ) for upsample required?" in vm.eval("2 4 4 1 nn.model 1 1 matrix ones upsample drop drop")
    assert "( N [mtum] n -- ) for upsample required?" in vm.eval("3 vector{ 11 8 1 } upsample drop")


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 4 4 1 nn.model 3 vector{ 11 8 1 } upsample 3 vector{ 0 0 1 } upsample constant em1  2 4 4 1 tensor ones constant emx")
    txt = vm.eval("em1 emx forward drop")
    assert "nn#fembed failed: nn#fembed vocab=11 not supported" in txt and "nn#fembed failed: nn#fembed vocab=0 not supported" in txt, txt
    txt = vm.eval("em1 2 4 4 8 tensor ones backprop drop")
    assert "nn#bembed failed: nn#bembed vocab=11 not supported" in txt and "nn#bembed failed: nn#bembed vocab=0 not supported" in txt, txt
    assert "[  1] embed  : T4[2,4,4,8] #p=128 T4[1,4,4,8] vocab=0, pos=1\n" in vm.eval("em1 network drop")      # and the VM goes on


def test_save_and_load(vm, tmp_path):
    """the file is the layer section, TABLE and POS of the token layer, POS of the position layer, and the closing `---`; `load` reads them back, and
    refuses a file whose embed line is not the layer's own, once, without changing anything"""
    f, g = str(tmp_path / "em.t4"), str(tmp_path / "em2.t4")
    words = "1 1 2 1 nn.model 3 vector{ 3 2 1 } upsample 3 vector{ 0 0 1 } upsample constant %s"
    head = b"\\ tensorForth v4.0 model\nvocab=3, pos=1embed  \nvocab=0, pos=1embed  \n"
    blob = lambda tab, p1, p2: (b"\n--- w.embed  \n" + struct.pack("<6f", *tab) + b"\n--- b.embed  \n" + struct.pack("<4f", *p1) +
                                b"\n--- b.embed  \n" + struct.pack("<4f", *p2) + b"\n---\n")
    vm.eval(words % "em2")
    vm.eval('em2 s" %s" save' % f); vm.eval("drop")
    got = open(f, "rb").read()
    assert got.startswith(head) and len(got) == len(head + blob([0] * 6, [0] * 4, [0] * 4))
    tab = struct.unpack("<6f", got[len(head) + 15:len(head) + 39]); p1 = struct.unpack("<4f", got[len(head) + 54:len(head) + 70])
    assert all(-1.0 <= v < 1.0 for v in tab) and any(abs(v) > 0.02 for v in tab) and all(-0.02 <= v < 0.02 for v in p1) and any(p1)     # the two scales
    # other values come back: load, save again, compare the bytes
    other = head + blob([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [-1.0, -2.0, -3.0, -4.0], [0.5, 0.25, 0.125, 8.0])
    open(f, "wb").write(other)
    vm.eval(words % "em3")
    txt = vm.eval('em3 s" %s" load' % f); vm.eval("drop")
    assert "format error" not in txt, txt
    vm.eval('em3 s" %s" save' % g); vm.eval("drop")
    assert open(g, "rb").read() == other
    # another vocabulary, another pos, or a line that is no embed line: one format error that changes nothing
    for bad in (b"vocab=4, pos=1embed  ", b"vocab=3, pos=0embed  ", b"vocab=3, pos=1addnorm", b"2x2 nearestupsampl", b"vocab=3, pos=1embed  X", b"vocab=3, pos=1embed"):
        open(f, "wb").write(head.replace(b"vocab=3, pos=1embed  ", bad) + blob([0.5] * 6, [0.5] * 4, [0.5] * 4))
        txt = vm.eval('em3 s" %s" load' % f); vm.eval("drop")
        assert txt.count("format error") == 1, (bad, txt)
        vm.eval('em3 s" %s" save' % g); vm.eval("drop")
        assert open(g, "rb").read() == other, bad
    open(f, "wb").write(b"\\ tensorForth v4.0 model\nvocab=3, pos=1embed  \n\n---\n")       # the file ends before the second layer's line
    txt = vm.eval('em3 s" %s" load' % f); vm.eval("drop")
    assert "format error" in txt, txt
