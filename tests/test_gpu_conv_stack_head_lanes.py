"""GPU: the classifier head inside cs_fwd (csrc/conv_stack_kernels.hip.inc head_fwd) at the shapes its lane arithmetic hangs on.  The wave-wide sums,
the softmax's max and sum and the hit rider's first arg-max run on the vector ALUs (csrc/lane_ops.h: lane swaps and DPP, which read lanes whatever
EXEC says), the collector's W2 / B2 / B1 / label loads leave in front of the matvec, and the dropout draw is computed in front of the poll.  What can
go wrong is a lane count: one softmax lane, exactly one row of 16 lanes, one lane into the second row of 16, all 64; one input of the second linear
layer, one more than a wave holds (a second `q`); the hoisted draw (the mask must be the oracle's, and t4k_rand_offset must end where the oracle's
does); no element-wise layer at all; the one-hot rows and hit flags that ride along with a labelled batch.

Every row runs t4k_conv_stack_head_fwd three times from the same inputs: all outputs bit-identical across the runs, run 0 within the oracle's bar
and the float64 witnesses exactly as tests/test_gpu_conv_stack_head_rows.py asks (whose helpers this file imports)."""
import ctypes

import numpy as np
import pytest

from test_gpu_conv_stack_head_rows import (RTOL, FWD_KEYS, Dev, StackHead, _build, _check_fwd_vs_oracle, _lay, _oracle_forward, _params, down_stage, p, plan,
                                            rel, witness_forward, witness_head)

pytestmark = pytest.mark.gpu

S6 = [(6, 3, None, "max", "relu")]          # 12 x 12 x 1 -> 6 x 6 x 6 = 216 inputs of the head: 16-byte rows, bands of 36 | 72 | 36 | 72 floats
# (N, H, W, C_in, stages, head (EA, EB, mid), labelled batch)
ROWS = [
    (11, 12, 12, 1, S6, (9, 1, "relu"), False),               # EB = 1: one live softmax lane (P = 1 exactly), 63 dead ones
    (11, 12, 12, 1, S6, (9, 16, None), False),                # EB = 16: the softmax fills exactly one row of 16 lanes; no element-wise layer
    (11, 12, 12, 1, S6, (9, 17, "tanh"), False),              # EB = 17: one lane into the second row of 16 (the xor-16 step carries a live value); three outputs on wave 0
    (16, 12, 12, 1, S6, (9, 64, "relu"), False),              # EB = 64: no dead lane; eight outputs per wave
    (11, 12, 12, 1, S6, (1, 10, "relu"), False),              # EA = 1: one lane of layer 2 holds an input, one thread polls
    (11, 12, 12, 1, S6, (65, 10, "dropout"), False),          # EA = 65: layer 2 needs a second q; the hoisted draw: Fm is the oracle's mask, the offset ends at the oracle's
    (16, 12, 12, 1, S6, (100, 10, "dropout"), True),          # labels ride along: one-hot rows and hit flags (first arg-max of P), a label >= EB, images behind n_label
]


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


@pytest.mark.parametrize("row", range(len(ROWS)))
def test_head_lanes_forward(t4k, dev, oracle, row):
    N, H, W, Cin, stages, (EA, EB, mid), labelled = ROWS[row]
    seed = 5100 + row; flat = True
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
    outs = ["Y1", "Fm", "Am", "Y2", "P"]
    n_label = N - 3
    if labelled:
        label = rng.integers(0, EB, N).astype(np.uint32)
        label[:N // 2] = np.argmax(Pr[:N // 2], axis=1)           # some hits for certain (the oracle's arg-max; the check below reads the device's own P) ...
        label[N // 2:] = (np.argmax(Pr[N // 2:], axis=1) + 1) % EB   # ... some misses ...
        label[1] = EB + 5                                         # ... and a label beyond the classes: counts as class 0
        d["label"] = dev.up(label.view(np.int32)); d["hot"] = dev.zeros((N, EB)); d["hit"] = dev.zeros((N,), dtype=dev.torch.uint8)
        hd.label, hd.hot, hd.hit_flag, hd.n_label = p(d["label"]), p(d["hot"]), p(d["hit"]), n_label
        outs += ["hot", "hit"]
    assert t4k.lib.t4k_conv_stack_head_ok(arr, len(stages), N, ctypes.byref(hd)) == 1
    ok, split, _bsplit = plan(t4k, arr, len(stages), N)
    assert ok == 1 and split == 4, "row %d: split %d, the row is written for 4 bands (a collector that polls three publishers)" % (row, split)
    dX = dev.up(X)
    runs = []
    for rep in range(3):
        for k_ in outs:
            d[k_].fill_(3 if k_ == "hit" else 0)
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
            _check_fwd_vs_oracle(dev, stages, ref, bufs, "lanes row %d head" % row)
            assert rel(got["Y1"], Y1) < RTOL and rel(got["Y2"], Y2) < RTOL and rel(got["P"], Pr) < RTOL
            if mid == "dropout":
                assert np.array_equal(got["Fm"], Fm)
            witness_forward(X, stages, params, down_stage(dev, bufs, ref, FWD_KEYS), who="head lanes row %d head stack" % row)
            witness_head(xf, W1, B1, W2, B2, mid, Y1, Fm, Am, Y2, Pr, who="head lanes row %d oracle" % row)
            witness_head(dev.down(bufs[-1]["copy_out"]).reshape(N, -1), W1, B1, W2, B2, mid, got["Y1"], got["Fm"] if mid else None,
                         got["Am"] if mid else None, got["Y2"], got["P"], who="head lanes row %d head" % row)
            if EB == 1:
                assert np.array_equal(got["P"], np.ones((N, 1), np.float32))
            if labelled:
                m = np.where(label < EB, label, 0).astype(np.int64)
                hot = np.zeros((N, EB), np.float32); hot[np.arange(n_label), m[:n_label]] = 1.0      # rows behind n_label are not written
                assert np.array_equal(got["hot"], hot)
                hit = (np.argmax(got["P"], axis=1) == m).astype(np.uint8); hit[n_label:] = 0         # np.argmax: the first of equal maxima, as k_hit
                assert np.array_equal(got["hit"], hit) and 0 < int(hit.sum()) < n_label
        runs.append(got)
    for rep in (1, 2):
        for k_ in runs[0]:
            a, b = runs[0][k_], runs[rep][k_]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "row %d: %s differs between run 0 and run %d" % (row, k_, rep)

