"""upsample layers of any factor 1..16 and the methods linear / bilinear / cubic on the CPU oracle VM - the product's host sources over the
oracle's C-ABI, which has no t4k_upsample_fwd / _bwd: `n upsample` and `m n upsample` admit the layer and shape it (H0 = n H1, W0 = n W1, rectangular
inputs included), `network` prints `KxK <method>`, and `forward` / `backprop` refuse the layer by name and compute nothing.  `2 upsample` and `3 upsample`
with method 0 keep their kernels and their text.  tests/test_gpu_upsample_words.py runs the layers on the product VM."""
import pytest

from vm_util import OracleVM

NAMES = ["nearest", "linear", "bilinear", "cubic"]


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


def net(vm, layers, shape="2 3 5 3"):
    return vm.eval("%s nn.model %s network drop" % (shape, " ".join(layers)))


# words, method, K
CASES = [("1 upsample", 0, 1), ("4 upsample", 0, 4), ("5 upsample", 0, 5), ("16 upsample", 0, 16),
         ("2 2 upsample", 2, 2), ("1 3 upsample", 1, 3), ("3 4 upsample", 3, 4), ("3 8 upsample", 3, 8)]


@pytest.mark.parametrize("words,method,K", CASES, ids=[c[0].replace(" ", "_") for c in CASES])
def test_layer_shapes_and_network_text(vm, words, method, K):
    depth = vm.eval("depth .").split()[0]
    txt = net(vm, [words])
    want = "NN Model[1/128]\n[  0] upsampl: T4[2,3,5,3] #p=0 %dx%d %s\n[  1] output : T4[2,%d,%d,3] #p=0 \n" % (K, K, NAMES[method], 3 * K, 5 * K)
    assert want in txt, txt
    assert vm.eval("depth .").split()[0] == depth


@pytest.mark.parametrize("words,text", [
    ("0 upsample", "nn#iup k=0x0? 1x1 to 16x16 supported only"),
    ("17 upsample", "nn#iup k=17x17? 1x1 to 16x16 supported only"),
    ("2 17 upsample", "nn#iup k=17x17? 1x1 to 16x16 supported only"),
    ("3 9 upsample", "nn#iup k=9x9? 1x1 to 8x8 supported only"),
    ("3 0 upsample", "nn#iup k=0x0? 1x1 to 8x8 supported only"),
    ("4 2 upsample", "nn#iup method=4?"),
    ("-1 2 upsample", "nn#iup method=-1?"),
])
def test_refusals_of_add(vm, words, text):
    txt = net(vm, [words])
    assert text in txt and "NN Model[0/128]\n[  0] output : T4[2,3,5,3] #p=0 \n" in txt, txt      # nothing was added


def test_forward_and_backprop_refuse_without_the_entries(vm):
    vm.eval("2 3 5 3 nn.model 2 2 upsample 4 upsample 3 1 upsample constant u1  2 3 5 3 tensor constant ux")
    txt = vm.eval("u1 ux forward drop")
    for K, m in ((2, 2), (4, 0), (1, 3)):
        assert "nn#fupsample failed: nn#fupsample size=%d method=%d not supported" % (K, m) in txt, txt
    vm.eval("2 24 40 3 tensor constant ut")
    txt = vm.eval("u1 ut backprop drop")
    for K, m in ((2, 2), (4, 0), (1, 3)):
        assert "nn#bupsample failed: nn#bupsample size=%d method=%d not supported" % (K, m) in txt, txt


def test_the_old_forms_compute_and_print_what_they_did(vm):
    txt = net(vm, ["2 upsample", "0 3 upsample", "0.5 2 conv2d"], "2 4 4 1")
    want = """NN Model[3/128]
[  0] upsampl: T4[2,4,4,1] #p=0 2x2 nearest
[  1] upsampl: T4[2,8,8,1] #p=0 3x3 nearest
[  2] conv2d : T4[2,24,24,1] #p=1192 T4[1,3,3,2] T1[2] T4[2,24,24,1] bias=0.5, C=2, K=3, S=1, P=1
[  3] output : T4[2,24,24,2] #p=0 
"""
    assert want in txt, txt
    # `2 upsample` then `3 upsample` (method 0) on the oracle: every cell becomes a 2x2, then a 3x3 tile; the backward sums the tiles
    vm.eval("2 4 4 1 nn.model 2 upsample 3 upsample constant u2  2 4 4 1 tensor ones constant uy")
    out = vm.eval('u2 uy forward ." mid " 1 n@ sum . drop ." out " 2 n@ sum . drop drop')
    assert "not supported" not in out and "failed" not in out, out
    assert float(out.split("mid")[1].split()[0]) == 2 * 8 * 8 and float(out.split("out")[1].split()[0]) == 2 * 24 * 24, out
    out = vm.eval('u2 2 24 24 1 tensor ones backprop ." dmid " 1 n@ sum . drop ." dx " 0 n@ sum . drop drop')
    assert "not supported" not in out and "failed" not in out, out
    assert float(out.split("dmid")[1].split()[0]) == 9 * 2 * 8 * 8 and float(out.split("dx")[1].split()[0]) == 36 * 2 * 4 * 4, out
    assert "( N [mtum] n -- ) for upsample required?" in vm.eval("upsample")
