"""`N vector{ heads 1 1 } linear`, the retention layer, on the CPU oracle VM - the product's host sources over the oracle's C-ABI, which has
no t4k_retention_* entries: a third cell of 1 picks the layer, `network` prints `retentn` with `heads=<h>, decay=1` and `#p=0`, a decay without the
causal cell is refused and adds nothing, a third cell that is missing or no 1 is the attention layer as before, `forward` / `backprop` refuse the layer by name,
and the .t4 file carries the layer's line, from which `load` rebuilds it.  On the parent commit, which reads two cells, every `retentn` line here is an
`attentn` line.  tests/test_gpu_retention_words.py runs the layer on the product VM."""
import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, words, shape="2 4 4 24"):
    return vm.eval("%s nn.model %s network drop" % (shape, words))


LINE = "NN Model[1/128]\n[  0] retentn: T4[2,4,4,24] #p=0 heads=%d, decay=1\n[  1] output : T4[2,4,4,8] #p=0 \n"
ATTN = "NN Model[1/128]\n[  0] attentn: T4[2,4,4,24] #p=0 T4[2,4,4,8] heads=2, causal=1\n[  1] output : T4[2,4,4,8] #p=0 \n"
EMPTY = "NN Model[0/128]\n[  0] output : T4[2,4,4,24] #p=0 \n"


def test_the_third_cell_picks_the_layer(vm):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, "3 vector{ 2 1 1 } linear")
    assert LINE % 2 in txt and "required" not in txt and "nn#i" not in txt, txt
    assert vm.eval("depth .").split()[0] == depth                           # ( N V -- N ): the vector is gone
    assert LINE % 1 in net(vm, "4 vector{ 1 7 1 9 } linear")                # any non-zero causal cell counts; a fourth cell is ignored
    for words in ("3 vector{ 2 1 0 }", "2 vector{ 2 1 }", "3 vector{ 2 1 9 }"):    # decay 0, missing, or no 1: the attention layer, as before
        assert ATTN in net(vm, words + " linear"), words


@pytest.mark.parametrize("words,heads", [("3 vector{ 2 0 1 }", 2), ("3 vector{ 5 1 1 }", 5), ("3 vector{ 0 1 1 }", 0), ("3 vector{ 3 1 1 }", 3)])
def test_what_the_layer_refuses(vm, words, heads):
    """a decay without the causal cell; heads that do not divide E; no head; d = 8 / 3"""
    txt = net(vm, words + " linear")
    assert "nn#iretention heads=%d? channels=24" % heads in txt and EMPTY in txt, txt


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 4 4 24 nn.model 3 vector{ 2 1 1 } linear constant rt1  2 4 4 24 tensor ones constant rtx")
    assert "nn#fretention failed: nn#fretention heads=2 not supported" in vm.eval("rt1 rtx forward drop")
    assert "nn#bretention failed: nn#bretention heads=2 not supported" in vm.eval("rt1 2 4 4 8 tensor ones backprop drop")
    assert LINE % 2 in vm.eval("rt1 network drop")                          # and the VM goes on


def test_save_and_load_rebuild_the_layer_from_its_line(vm, tmp_path):
    f = str(tmp_path / "rt.t4")
    vm.eval("2 4 4 24 nn.model 3 vector{ 2 1 1 } linear constant rt2")
    saved = vm.eval("rt2 network drop")
    vm.eval('rt2 s" %s" save' % f); vm.eval("drop")
    assert open(f, "rb").read() == b"\\ tensorForth v4.0 model\nheads=2, decay=1retentn\n\n---\n"
    vm.eval("2 4 4 24 nn.model 3 vector{ 1 1 1 } linear constant rt3")
    assert LINE % 1 in vm.eval("rt3 network drop")
    txt = vm.eval('rt3 s" %s" load' % f); vm.eval("drop")
    assert "format error" not in txt and LINE % 2 in saved and vm.eval("rt3 network drop") == saved, txt
    for bad in (b"heads=5, decay=1retentn", b"heads=2, decay=0retentn", b"heads=2, causal=1attentn", b"heads=2, decay=1retentnX"):
        open(f, "wb").write(b"\\ tensorForth v4.0 model\n" + bad + b"\n\n---\n")
        txt = vm.eval('rt3 s" %s" load' % f); vm.eval("drop")
        assert "format error" in txt and vm.eval("rt3 network drop") == saved, (bad, txt)
