"""The three nets of tests/geo_plan_worker.py (what tests/test_gpu_geo_layer_plans.py steps under every launch plan on the GPU) on the CPU oracle VM: the
product's host sources over the oracle's C-ABI admit, shape and print every layer - the table each net text must give is the worker's TABLES, line for line,
the `#p=` sums included - and the shapes the GPU test's witnesses assume are the table's.  A typo in a net text fails here, without a GPU."""
import re

import pytest

import geo_plan_worker as gw
from vm_util import OracleVM


@pytest.fixture(scope="module")
def vm():
    v = OracleVM(seed=1)
    yield v
    v.close()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_net_text_builds_the_expected_layer_table(vm, name):
    txt = vm.eval(gw.NETS[name]["text"] + " network drop")
    assert "?" not in txt.replace("-> ok", ""), txt
    gw.check_table(name, txt)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_worker_shapes_and_ops_are_the_tables(name):
    """the worker's `shapes` and `ops` (what the witnesses are built from) against the printed table: layer i's input tensor, its kind and its geometry text"""
    net = gw.NETS[name]
    rows = re.findall(r"^\[ *(\d+)\] (\w+) *: T4\[(\d+),(\d+),(\d+),(\d+)\] #p=\d+ ?(.*?) ?$", gw.TABLES[name], re.M)
    assert len(rows) == len(net["shapes"]) == len(net["ops"]) + 1
    kinds = {"conv": "conv2d", "pool": None, "up": "upsampl", "relu": "relu", "bn": "batchnm", "flatten": "flatten", "linear": "linear", "softmax": "softmax"}
    methods = {gw.NEAREST: "nearest", gw.LINEAR: "linear", gw.BILINEAR: "bilinear", gw.CUBIC: "cubic"}
    for (i, kind, n, h, w, c, tail), shape, op in zip(rows, net["shapes"], net["ops"] + [("output",)]):
        assert (int(n), int(h), int(w), int(c)) == (gw.N,) + shape, (name, i)
        if op[0] == "conv":
            _, C1, C0, K, S, P, D, G = op
            want = "T4[%d,%d,%d,%d] T1[%d] T4[%d,%d,%d,%d] bias=0.5, C=%d, K=%d, S=%d, P=%d" % ((C1 // G, K, K, C0, C0, gw.N) + shape + (C0, K, S, P))
            want += (", D=%d" % D if D > 1 else "") + (", G=%d" % G if G > 1 else "")
            assert kind == "conv2d" and tail == want and shape[2] == C1, (name, i, tail, want)
        elif op[0] == "pool":
            assert kind == op[1] + "pool" and tail.endswith("%dx%d, S=%d, P=%d" % (op[2], op[2], op[3], op[4])), (name, i, tail)
        elif op[0] == "up":
            assert kind == "upsampl" and tail == "%dx%d %s" % (op[2], op[2], methods[op[1]]), (name, i, tail)
        elif op[0] == "linear":
            assert kind == "linear" and shape[0] * shape[1] * shape[2] == op[1] and "T4[1,%d,%d,1] T1[%d]" % (op[2], op[1], op[2]) in tail, (name, i, tail)
        else:
            assert kind == (kinds[op[0]] if op[0] != "output" else "output"), (name, i, kind)


def test_the_learning_rate_survives_the_scalar_cell():
    """a scalar on the VM's stack keeps 23 of its 24 mantissa bits (the last one is the object tag): the rate the worker writes must be the fp32 number the GPU
    test computes with, last bit included"""
    import numpy as np
    assert float(gw.LR_TEXT) == gw.LR and float(np.float32(gw.LR)) == gw.LR
    assert int(np.array([gw.LR], np.float32).view(np.uint32)[0]) & 1 == 0


def test_the_nets_hold_what_the_plans_need():
    """net A: a grouped layer 0, a dense run-time-geometry layer and a grouped layer inside, a max and an avg pool of the vector form, a bilinear and a bicubic
    upsample; net B: the min pool, nearest x4 (not the old 2 / 3 route) and the linear method on a rectangular grid; net C: batch-norm, linear + softmax"""
    A, B, C = (gw.NETS[n]["ops"] for n in "ABC")
    assert A[0][0] == "conv" and A[0][7] > 1
    inner = [op for op in A[1:] if op[0] == "conv"]
    assert any(op[7] > 1 for op in inner) and any(op[7] == 1 and op[3:7] not in ((1, 1, 0, 1), (3, 1, 1, 1), (4, 2, 1, 1), (5, 1, 2, 1)) for op in inner)
    assert {op[1] for op in A if op[0] == "pool"} == {"max", "avg"} and {op[1] for op in A if op[0] == "up"} == {gw.BILINEAR, gw.CUBIC}
    assert ("pool", "min", 3, 1, 1) in B and ("up", gw.NEAREST, 4) in B and ("up", gw.LINEAR, 2) in B and not any(op[0] == "conv" for op in B)
    assert gw.NETS["B"]["shapes"][0][0] != gw.NETS["B"]["shapes"][0][1]
    assert [op[0] for op in C] == ["conv", "bn", "relu", "pool", "flatten", "linear", "softmax"]
