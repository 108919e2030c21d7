"""GPU: the classifier head inside cs_fwd (csrc/conv_stack_kernels.hip.inc head_fwd) at the edges of its row arithmetic.  A wave owns
ceil(EA / 8) rows of W1 and adds the lanes' shares of ALL of them up side by side (lanes_sum: one butterfly step of every row in flight at a time),
so what can go wrong is a row count: waves without a row, a wave with fewer rows than its slots, a second trip, the scalar (non 16-byte) row path,
one or several outputs per wave in the second linear layer.  Every row runs t4k_conv_stack_head_fwd three times from the same inputs: all outputs
bit-identical across the runs, run 0 within the oracle's bar and the float64 witness exactly as tests/test_gpu_conv_stack_sweep.py
test_sweep_head_forward asks, and the band split the row is written for as t4k_conv_stack_plan reports it."""
import ctypes

import numpy as np
import pytest

from test_gpu_conv_stack import (StackHead, _build, _lay, _oracle_forward, _params, FWD_KEYS, down_stage, witness_forward, witness_head)
from test_gpu_conv_stack_sweep import RTOL, _check_fwd_vs_oracle, cu_count, plan
from test_gpu_parity import Dev, p, rel

pytestmark = pytest.mark.gpu

LENET = [(10, 3, None, "max", "relu"), (20, 3, "dropout", "max", "relu")]
# (N, H, W, C_in, stages, head (EA, EB, mid), the split t4k_conv_stack_plan must report)
ROWS = [
    (11, 12, 12, 1, [(6, 3, None, "max", "relu")], (1, 1, None), 4),             # one row of W1: seven waves have none; one output: 16-byte rows (216 = 4 x 54 floats, bands of 36 | 72)
    (11, 12, 12, 1, [(6, 3, None, "max", "relu")], (9, 9, "relu"), 4),            # two slots per wave: waves 0 - 3 fill both, wave 4 one, waves 5 - 7 none; two outputs on wave 0
    ("cu+8", 12, 12, 1, [(8, 3, None, "max", "relu")], (256, 64, "dropout"), 1),  # the largest head: 32 rows per wave of 288 floats, two trips of 16; eight outputs per wave; one band, two dispatch rounds
    (11, 12, 12, 1, [(5, 3, None, "max", "relu")], (100, 10, "tanh"), 4),         # bands of 30 | 60 floats: the 4-byte row path, 7 rows per trip, two trips, the second partly empty
    (16, 28, 28, 1, LENET, (100, 10, "dropout"), 4),                              # LeNet's own stages and head: 13 rows per wave (waves 0 - 6; wave 7 has 9) in one trip
]


def n_of(spec):
    return spec if isinstance(spec, int) else {"cu+8": cu_count() + 8}[spec]


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_head_rows_forward(t4k, dev, oracle, row):
    spec, H, W, Cin, stages, (EA, EB, mid), want_split = ROWS[row]
    N = n_of(spec); seed = 5000 + row; flat = True
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    params = _params(rng, Cin, stages)
    o = oracle.lib(); P = oracle.P; LAY = _lay(oracle)
    ref, _ = _oracle_forward(oracle, X, stages, flat, params, seed, 4096)          # (the head's draws continue this stream)
    arr, bufs = _build(dev, oracle, X, stages, flat, params, ref)
    xf = np.ascontiguousarray(ref[-1]["last"].reshape(N, -1)); E1 = xf.shape[1]
    W1 = (rng.standard_normal((EA, E1)) * 0.1).astype(np.float32); B1 = rng.standard_normal(EA).astype(np.float32)
    W2 = (rng.standard_normal((EB, EA)) * 0.3).astype(np.float32); B2 = rng.standard_normal(EB).astype(np.float32)
    Y1 = np.zeros((N, EA), np.float32); assert o.t4o_linear_fwd(P(xf), P(W1), P(B1), P(Y1), N, EA, E1) == 0
    cur = Y1; Fm = Am = None
    if mid:
        L, a = LAY[mid]; Fm = np.zeros(Y1.size, np.float32); Am = np.zeros_like(Y1)
        if mid == "dropout":
            o.t4o_rand(P(Fm), Fm.size, 0, 0.0, 1.0)
        o.t4o_activate(L, P(Y1), P(Am), P(Fm), a, Y1.size); Fm = Fm.reshape(Y1.shape); cur = Am
    Y2 = np.zeros((N, EB), np.float32); assert o.t4o_linear_fwd(P(np.ascontiguousarray(cur)), P(W2), P(B2), P(Y2), N, EB, EA) == 0
    Pr = np.zeros_like(Y2); o.t4o_softmax(P(Y2), P(Pr), N, EB)
    end = o.t4o_rand_offset()
    hd = StackHead()
    d = {"W1": dev.up(W1), "B1": dev.up(B1), "Y1": dev.zeros(Y1.shape), "Fm": dev.zeros(Y1.shape), "Am": dev.zeros(Y1.shape),
         "W2": dev.up(W2), "B2": dev.up(B2), "Y2": dev.zeros(Y2.shape), "P": dev.zeros(Y2.shape)}
    hd.W1, hd.B1, hd.Y1, hd.W2, hd.B2, hd.Y2, hd.P = p(d["W1"]), p(d["B1"]), p(d["Y1"]), p(d["W2"]), p(d["B2"]), p(d["Y2"]), p(d["P"])
    if mid:
        hd.mid_layer, hd.mid_alpha = LAY[mid]; hd.mid_mask, hd.mid_out = p(d["Fm"]), p(d["Am"])
    hd.E1, hd.E0a, hd.E0b = E1, EA, EB
    assert t4k.lib.t4k_conv_stack_head_ok(arr, len(stages), N, ctypes.byref(hd)) == 1
    ok, split, _bsplit = plan(t4k, arr, len(stages), N)
    assert ok == 1 and split == want_split, "row %d: split %d, the row is written for %d" % (row, split, want_split)
    dX = dev.up(X)
    outs = ("Y1", "Fm", "Am", "Y2", "P")
    runs = []
    for rep in range(3):
        for k_ in outs:
            d[k_].zero_()
        for b in bufs:
            for k_ in FWD_KEYS:
                if k_ in b:
                    b[k_].zero_()
        t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", 4096)
        t4k.call("t4k_conv_stack_head_fwd", p(dX), None, arr, len(stages), N, ctypes.byref(hd), None)
        assert t4k.lib.t4k_rand_offset() == end
        got = {k_: dev.down(d[k_]).copy() for k_ in outs}
        for si, t in enumerate(down_stage(dev, bufs, ref, FWD_KEYS)):
            for k_, v in t.items():
                got["s%d.%s" % (si, k_)] = v.copy()
        if rep == 0:
            _check_fwd_vs_oracle(dev, stages, ref, bufs, "row %d head" % row)
            assert rel(got["Y1"], Y1) < RTOL and rel(got["Y2"], Y2) < RTOL and rel(got["P"], Pr) < RTOL
            if mid == "dropout":
                assert np.array_equal(got["Fm"], Fm)
            witness_forward(X, stages, params, down_stage(dev, bufs, ref, FWD_KEYS), who="head rows row %d head stack" % row)
            witness_head(xf, W1, B1, W2, B2, mid, Y1, Fm, Am, Y2, Pr, who="head rows row %d oracle" % row)
            witness_head(dev.down(bufs[-1]["copy_out"]).reshape(N, -1), W1, B1, W2, B2, mid, got["Y1"], got["Fm"] if mid else None,
                         got["Am"] if mid else None, got["Y2"], got["P"], who="head rows row %d head" % row)
        runs.append(got)
    for rep in (1, 2):
        for k_ in runs[0]:
            assert np.array_equal(runs[0][k_].view(np.uint32), runs[rep][k_].view(np.uint32)), "row %d: %s differs between run 0 and run %d" % (row, k_, rep)
