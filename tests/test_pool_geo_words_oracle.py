"""pooling layers of any K 1..16 with stride and padding on the CPU oracle VM - the product's host sources over the oracle's C-ABI,
which has no t4k_pool_geo_fwd / _bwd: `M vector{ K S P } maxpool | avgpool | minpool` admits the layer, shapes it on a floor grid (W0 from W1) and
drops the vector, `network` prints `KxK, S=<s>, P=<p>` and lists the code tensor of a max / min layer, and `forward` / `backprop` refuse the layer by
name and compute nothing.  `M n maxpool` keeps its 2x2 / 3x3 form, its text and its kernels.  tests/test_gpu_pool_geo_words.py runs the layers on the
product VM."""
import pytest

from vm_util import OracleVM

WORDS = ["maxpool", "avgpool", "minpool"]


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, layers, shape="2 12 12 3"):
    return vm.eval("%s nn.model %s network drop" % (shape, " ".join(layers)))


# vector, text, (H0, W0) on 12 x 12 and on 12 x 10 (None: the window does not fit the 10 columns)
CASES = [
    ("3 vector{ 3 2 1 }", "3x3, S=2, P=1", (6, 6), (6, 5)),
    ("1 vector{ 2 }", "2x2, S=2, P=0", (6, 6), (6, 5)),                  # a missing S cell means K, a missing P cell 0
    ("3 vector{ 3 1 1 }", "3x3, S=1, P=1", (12, 12), (12, 10)),
    ("2 vector{ 7 7 }", "7x7, S=7, P=0", (1, 1), (1, 1)),
    ("2 vector{ 2 3 }", "2x2, S=3, P=0", (4, 4), (4, 3)),                 # S > K: cells no window covers
    ("1 vector{ 12 }", "12x12, S=12, P=0", (1, 1), None),                  # the window is the image
]


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("vec,text,sq,rect", CASES, ids=[c[0].split("{")[1].strip(" }").replace(" ", "_") for c in CASES])
def test_layer_shapes_and_network_text(vm, word, vec, text, sq, rect):
    depth = vm.eval("depth .").split()[0]
    for shape, W1, ext in (("2 12 12 3", 12, sq), ("2 12 10 3", 10, rect)):
        if ext is None:
            continue
        txt = net(vm, ["%s %s" % (vec, word)], shape)
        H0, W0 = ext
        code = "" if word == "avgpool" else "T4[2,%d,%d,1] " % (H0, W0)      # bytes in a float tensor: ceil(3 / 4) floats a pixel; listed, and counted in #p
        want = "[  0] %s: T4[2,12,%d,3] #p=%d %s%s\n[  1] output : T4[2,%d,%d,3] #p=0 \n" % (word, W1, 0 if word == "avgpool" else 2 * H0 * W0, code, text, H0, W0)
        assert "NN Model[1/128]" in txt and want in txt, txt
    assert vm.eval("depth .").split()[0] == depth                          # ( N V -- N ): the vector is dropped, `drop` takes the model - nothing is left behind


def test_wide_channels_code_tensor(vm):
    """C = 9: ceil(9 / 4) = 3 floats of codes a pixel"""
    txt = net(vm, ["3 vector{ 3 2 1 } minpool"], "2 12 12 9")
    assert "[  0] minpool: T4[2,12,12,9] #p=216 T4[2,6,6,3] 3x3, S=2, P=1\n" in txt, txt


def test_ignored_and_zero_cells(vm):
    txt = net(vm, ["5 vector{ 3 2 1 9 9 } maxpool"])                     # cells behind the third are ignored
    assert "3x3, S=2, P=1\n" in txt and "T4[2,6,6,3]" in txt, txt
    txt = net(vm, ["3 vector{ 3 0 1 } maxpool"])                         # an S cell of 0 means K
    assert "3x3, S=3, P=1\n" in txt and "[  1] output : T4[2,4,4,3]" in txt, txt
    txt = net(vm, ["3 vector{ 3 2 0 } maxpool"])                         # a P cell of 0 means NO padding (unlike conv2d)
    assert "3x3, S=2, P=0\n" in txt and "[  1] output : T4[2,5,5,3]" in txt, txt


def test_the_scalar_form_beside_the_vector_form(vm):
    txt = net(vm, ["3 maxpool", "3 vector{ 3 1 1 } maxpool", "2 avgpool", "1 vector{ 2 } avgpool"])
    want = """NN Model[4/128]
[  0] maxpool: T4[2,12,12,3] #p=0 3x3
[  1] maxpool: T4[2,4,4,3] #p=32 T4[2,4,4,1] 3x3, S=1, P=1
[  2] avgpool: T4[2,4,4,3] #p=0 2x2
[  3] avgpool: T4[2,2,2,3] #p=0 2x2, S=2, P=0
[  4] output : T4[2,1,1,3] #p=0 
"""
    assert want in txt, txt


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("vec,text", [
    ("1 vector{ 17 }", "nn#ipool %s k=17x17? 1x1 to 16x16 supported only"),
    ("1 vector{ 0 }", "nn#ipool %s k=0x0? 1x1 to 16x16 supported only"),
    ("2 vector{ 3 17 }", "nn#ipool %s stride=17 padding=0?"),
    ("3 vector{ 3 1 2 }", "nn#ipool %s stride=1 padding=2?"),             # P > K / 2
    ("3 vector{ 1 1 1 }", "nn#ipool %s stride=1 padding=1?"),
    ("2 vector{ 13 1 }", "nn#ipool %s stride=1 padding=0?"),              # the window is larger than the image
    ("3 vector{ 16 4 1 }", "nn#ipool %s stride=4 padding=1?"),            # ... than the padded image
])
def test_refusals_of_add(vm, word, vec, text):
    txt = net(vm, ["%s %s" % (vec, word)])
    assert (text % word) in txt and "NN Model[0/128]" in txt, txt        # nothing was added
    txt = net(vm, ["2 vector{ 11 1 } %s" % word], "2 12 10 3")           # W1 = 10 alone is too small
    assert ("nn#ipool %s stride=1 padding=0?" % word) in txt and "NN Model[0/128]" in txt, txt


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 12 12 3 nn.model 3 vector{ 3 2 1 } maxpool 2 vector{ 4 2 } avgpool constant p1  2 12 12 3 tensor constant px")
    txt = vm.eval("p1 px forward drop")
    assert "nn#fpool failed: nn#fpool kernel_size=3 stride=2 padding=1 not supported" in txt, txt
    assert "nn#fpool failed: nn#fpool kernel_size=4 stride=2 padding=0 not supported" in txt, txt
    vm.eval("2 2 2 3 tensor constant pt")
    txt = vm.eval("p1 pt backprop drop")
    assert "nn#bpool failed: nn#bpool kernel_size=4 stride=2 padding=0 not supported" in txt, txt
    assert "nn#bpool failed: nn#bpool kernel_size=3 stride=2 padding=1 not supported" in txt, txt


def test_the_old_forms_print_what_they_printed(vm):
    txt = net(vm, ["0.5 8 conv2d", "2 maxpool", "relu", "3 minpool"])
    want = """NN Model[4/128]
[  0] conv2d : T4[2,12,12,3] #p=1312 T4[3,3,3,8] T1[8] T4[2,12,12,3] bias=0.5, C=8, K=3, S=1, P=1
[  1] maxpool: T4[2,12,12,8] #p=0 2x2
[  2] relu   : T4[2,6,6,8] #p=576 T4[2,6,6,8] 
[  3] minpool: T4[2,6,6,8] #p=0 3x3
[  4] output : T4[2,2,2,8] #p=0 
"""
    assert want in txt, txt
    txt = net(vm, ["4 maxpool"])
    assert "nn#ipool k=4x4? 2x2 and 3x3 supported only" in txt and "NN Model[0/128]" in txt, txt
    vm.eval("2 12 12 3 nn.model 2 maxpool constant p2")
    out = vm.eval("p2 px forward drop p2 1 n@ sum . drop drop")
    assert "not supported" not in out and "failed" not in out, out
    for word in WORDS:                                                   # a tensor without a model under it: the reference's line, whatever its rank
        assert "( N n -- ) one param required!" in vm.eval("3 vector{ 3 2 1 } %s drop" % word)
        assert "( N n -- ) one param required!" in vm.eval("2 2 matrix{ 1 2 3 4 } %s drop" % word)
    txt = vm.eval("2 12 12 3 nn.model 2 2 matrix{ 1 2 3 4 } maxpool drop network drop")      # a matrix on a model is no geometry
    assert "( N n -- ) one param required!" in txt and "NN Model[0/128]" in txt, txt
