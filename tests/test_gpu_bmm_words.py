"""`@` / `matmul` / `@=` beyond the reference's _tdot on the PRODUCT VM (tensorforth_amd/vm.py: libten4.so over libt4hip.so, where
Tensor::bmm is one t4k_gemm_batched launch): every row of the DESIGN.md "Beyond the reference" table within the fp32 dot-product bound
against float64, and a script of the new cases printing what the CPU oracle VM prints (the comparison the golden tests use)."""
import numpy as np
import pytest

from test_bmm_words_oracle import CASES, ctor, new_result, numel, run_pair, want64, nhwc
from vm_util import OracleVM, compare

pytestmark = pytest.mark.gpu

BIG = [(("t", 8, 128, 96, 1), ("t", 8, 96, 130, 1)),        # the tile-kernel regime
       (("t", 128, 28, 28, 1), ("t", 128, 28, 28, 1)),
       (("t", 4, 100, 70, 3), ("m", 70, 90)),                # channel broadcast beyond 64 x 64
       (("v", 200), ("t", 3, 200, 150, 1))]


@pytest.fixture(scope="module")
def vm():
    from tensorforth_amd.vm import VM
    v = VM(device=0, seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("a,b", CASES + BIG)
def test_table_rows_on_the_product(vm, a, b):
    shape = new_result(a, b)
    rng = np.random.default_rng(len(ctor(a)) * 31 + numel(b))
    A, B, O = run_pair(vm, a, b, rng)
    vm.eval("drop drop drop")
    if a[0] == "v" and b[0] == "m":
        assert O.shape == (1, shape[1], 1, 1), O.shape
    else:
        assert O.shape == shape, (O.shape, shape)
    o64, mag = want64(a, b, A, B)
    K = nhwc(b)[1]
    err = np.abs(O.reshape(o64.shape).astype(np.float64) - o64)
    assert np.all(err <= 2 * K * 2.0 ** -24 * mag + 1e-30), float(np.max(err / (mag + 1e-30)))


def new_cases_script():
    lines = []
    for a, b in CASES:
        lines.append("%s gradfill %s gradfill @ . cr\ndrop drop" % (ctor(a), ctor(b)))
        lines.append("%s gradfill %s gradfill matmul . cr\ndrop drop" % (ctor(a), ctor(b)))
        lines.append("%s gradfill %s gradfill @= . cr" % (ctor(a), ctor(b)))
    lines.append("2 3 4 1 tensor 3 4 5 1 tensor @ . cr\ndrop")     # still rejected
    return "\n".join(lines) + "\n"


def test_new_cases_print_what_the_oracle_vm_prints(vm):
    src = new_cases_script()
    own = vm.eval(src)
    ovm = OracleVM(seed=1)
    try:
        ref = ovm.eval(src)
    finally:
        ovm.close()
    assert own.count("] = {") >= len(CASES) * 3        # every product printed
    bad = compare(own, ref)
    assert not bad, bad
