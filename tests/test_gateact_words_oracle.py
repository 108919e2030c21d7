"""`N vector{ kind gate } elu`, the smooth and gated feed-forward activations, on the CPU oracle VM - the product's host sources over the
oracle's C-ABI, which has no t4k_gateact_* entries: the word consumes the vector and adds a `gateact` layer with no tensor of its own and `#p=0`, gate 1
halves the channels, every refusal prints its one line and adds nothing, `forward` / `backprop` refuse the layer by name and compute nothing, and the .t4
file carries the layer's line.  Every other operand set of `elu` prints and builds what it did.  On the parent commit the vector form prints
"( N n -- ) one param required!".  tests/test_gpu_gateact_words.py runs the layer on the product VM."""
import pytest

from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, words, shape="2 4 4 48"):
    return vm.eval("%s nn.model %s network drop" % (shape, words))


@pytest.mark.parametrize("vec,line,C", [("1 vector{ 0 }", "kind=0, gate=0", 48), ("2 vector{ 2 1 }", "kind=2, gate=1", 24), ("3 vector{ 3 1 9 }", "kind=3, gate=1", 24)])
def test_the_layer_line_the_shape_and_the_stack_effect(vm, vec, line, C):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, vec + " elu relu")
    assert "one param required" not in txt and "nn#igateact" not in txt, txt
    assert ("NN Model[2/128]\n[  0] gateact: T4[2,4,4,48] #p=0 %s\n[  1] relu   : T4[2,4,4,%d] #p=%d T4[2,4,4,%d] \n[  2] output : T4[2,4,4,%d] #p=0 \n"
            % (line, C, 32 * C, C, C)) in txt, txt
    assert vm.eval("depth .").split()[0] == depth                           # ( N V -- N ): the vector is gone


@pytest.mark.parametrize("vec,shape,line", [("2 vector{ 2 1 }", "2 4 4 7", "kind=2 gate=1? channels=7"), ("1 vector{ 4 }", "2 4 4 8", "kind=4 gate=0? channels=8"),
                                            ("1 vector{ -1 }", "2 4 4 8", "kind=-1 gate=0? channels=8"), ("2 vector{ 0 2 }", "2 4 4 8", "kind=0 gate=2? channels=8")],
                         ids=["odd", "kind4", "kind-1", "gate2"])
def test_refusals_add_nothing_and_consume_the_vector(vm, vec, shape, line):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, vec + " elu", shape)
    assert txt.count("nn#igateact") == 1 and "nn#igateact " + line + "\n" in txt and "NN Model[0/128]\n" in txt, txt
    assert vm.eval("depth .").split()[0] == depth


def test_the_other_operand_sets_print_and_build_what_they_did(vm):
    assert "NN Model[1/128]\n[  0] elu    : T4[2,4,4,3] #p=96 T4[2,4,4,3] bias=1\n" in net(vm, "elu", "2 4 4 3")
    assert "[  0] elu    : T4[2,4,4,3] #p=96 T4[2,4,4,3] bias=0.5\n" in net(vm, "0.5 elu", "2 4 4 3")
    assert "[  0] leakyrl: T4[2,4,4,3] #p=96 T4[2,4,4,3] bias=0.01\n" in net(vm, "leakyrelu", "2 4 4 3")
    out = vm.eval("1 vector{ 2 } elu")                                      # a vector with no model under it: the old text
    assert "( N n -- ) one param required!" in out
    vm.eval("drop")


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 4 4 8 nn.model 2 vector{ 2 1 } elu constant ga1  2 4 4 8 tensor ones constant gax  2 4 4 4 tensor ones constant gat")
    assert "nn#fgateact failed: nn#fgateact kind=2 not supported" in vm.eval("ga1 gax forward drop")
    assert "nn#bgateact failed: nn#bgateact kind=2 not supported" in vm.eval("ga1 gat backprop drop")
    assert "[  0] gateact: T4[2,4,4,8] #p=0 kind=2, gate=1\n[  1] output : T4[2,4,4,4] #p=0 \n" in vm.eval("ga1 network drop")     # and the VM goes on


def test_save_and_load(vm, tmp_path):
    f, g = str(tmp_path / "ga.t4"), str(tmp_path / "ga2.t4")
    vm.eval("2 4 4 8 nn.model 2 vector{ 2 1 } elu constant ga2")
    vm.eval('ga2 s" %s" save' % f); vm.eval("drop")
    want = b"\\ tensorForth v4.0 model\nkind=2, gate=1gateact\n\n---\n"
    assert open(f, "rb").read() == want
    open(f, "wb").write(want.replace(b"kind=2", b"kind=1"))                  # another kind on the same gate: read back into the layer
    txt = vm.eval('ga2 s" %s" load' % f); vm.eval("drop")
    assert "format error" not in txt, txt
    assert "[  0] gateact: T4[2,4,4,8] #p=0 kind=1, gate=1\n" in vm.eval("ga2 network drop")
    for bad in (b"kind=1, gate=0gateact", b"kind=4, gate=1gateact", b"bias=1elu    ", b"kind=1, gate=1gateactX", b"kind=1, gate=1addnorm"):
        open(f, "wb").write(want.replace(b"kind=2, gate=1gateact", bad))     # a line the layer cannot take: one format error, nothing changes
        txt = vm.eval('ga2 s" %s" load' % f); vm.eval("drop")
        assert txt.count("format error") == 1, (bad, txt)
        vm.eval('ga2 s" %s" save' % g); vm.eval("drop")
        assert open(g, "rb").read() == want.replace(b"kind=2", b"kind=1"), bad
