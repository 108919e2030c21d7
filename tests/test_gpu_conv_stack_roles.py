"""The banded conv-stack backward with its two wave roles (cs_bwd_b: 16 waves; in the middle phase of a stage waves 0 - 7 take the dF items
while waves 8 - 15 take the stage's dX, one barrier behind both, then one store phase on all waves).  Rows chosen for how the two roles meet:
fewer dF items than dF waves, exactly as many, several rounds; a dX role that ends long before the dF role and one that is the longer of
the two; both dX engines (dx_valu on the vector ALUs, the MFMA convolution); 2, 3 and 4 bands, even and uneven.  Every row runs with three
train words - parameter gradients plus every dX, the first layer's dX on demand (the early-return path, then t4k_conv_stack_dx0), and no
parameter gradients (the dF role has no work) - and every (row, word) runs three times from the same inputs: all outputs bit-identical.

Each run is a stack forward followed by the banded backward through the C ABI; every backward tensor (each layer's dX, the dF and dB
after the fold, the run's gradient tensors behind the masks) is compared with the oracle's separate layers at the sweep's bar and with
float64 element by element under the sweep's witness rule (tests/f64_witness.py)."""
import ctypes
from math import gcd

import numpy as np
import pytest

import f64_witness as wt
from test_gpu_conv_stack import (ConvStage, _build, _oracle_backward, _oracle_forward, _params, BWD_KEYS, FWD_KEYS,
                                 down_stage, oracle_bwd_as_got, witness_backward)
from test_gpu_conv_stack_sweep import _check_bwd_vs_oracle, n_of, plan
from test_gpu_parity import Dev, p

pytestmark = pytest.mark.gpu

# (N as a share of the CU count, H, W, C_in, [(C0, K, pre, pool, post)], flatten, the bsplit t4k_conv_stack_plan must report)
ROWS = [
    ("cu/2", 12, 12, 1, [(6, 3, None, "max", "relu"), (12, 3, "dropout", "max", "relu")], True, 2),
    #   the LeNet pattern in small.  Stage 0: 6 dF items < 8 dF waves (two idle) beside dx_valu (nF = 54); stage 1: 6 items beside the MFMA dX at W = 6
    ("cu/4", 14, 14, 10, [(16, 5, "relu", "max", None)], False, 4),
    #   TAPS = 250: 24 dF items, three rounds per dF wave; the dX role is done long before the dF role
    ("cu/4", 32, 32, 1, [(4, 3, "relu", "max", None), (8, 3, None, "avg", "tanh")], False, 4),
    #   both stages exactly 8 items; stage 0 many pixels per thread in dx_valu; stage 1 C1 = 4, nF = 288: MFMA dX, several tiles per dX wave (the longer role)
    ("cu/3", 10, 10, 3, [(8, 3, "relu", None, None)], False, 3),
    #   three uneven bands; 5 items; MFMA dX with C1 = 3 (nF = 216 > 160)
    ("cu/4", 8, 8, 2, [(6, 3, None, "max", "relu")], False, 4),
    #   four bands of one pooled row = two conv rows each, fewer than one MFMA row quad; dx_valu (nF = 108)
]

# the train words of t4k_conv_stack_bwd: bit 0 parameter gradients, bit 3 the first layer's dX left to t4k_conv_stack_dx0
WORDS = [("grads+dx", 1), ("grads+lazy-dx0", 9), ("no-grads", 0)]
DF0, DB0 = 0.25, -0.5                       # what the gradient tensors hold before a backward: the fold adds


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


_ROW = {}                                   # per row: inputs, the oracle's forward, device buffers - built once, shared by the three train words


def _row(dev, oracle, row):
    if row not in _ROW:
        spec, H, W, Cin, stages, flat, _bs = ROWS[row]
        N = n_of(spec)
        seed = 7000 + row
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
        params = _params(rng, Cin, stages)
        ref, _end = _oracle_forward(oracle, X, stages, flat, params, seed, 4096)
        arr, bufs = _build(dev, oracle, X, stages, flat, params, ref)
        DY = rng.standard_normal(ref[-1]["last"].shape).astype(np.float32)
        _ROW[row] = dict(N=N, seed=seed, X=X, params=params, ref=ref, arr=arr, bufs=bufs, DY=DY, dDY=dev.up(DY), fwd=None, want=None)
    return _ROW[row]


def _forward(t4k, dev, r, stages):
    t4k.call("t4k_rand_init", r["seed"]); t4k.call("t4k_rand_set_offset", 4096)
    r["bufs"][0]["X"].copy_(dev.torch.from_numpy(r["X"]))
    t4k.call("t4k_conv_stack_fwd", p(r["bufs"][0]["X"]), None, r["arr"], len(stages), r["N"], None)
    for d in r["bufs"]:
        d["DF"].fill_(DF0); d["DB"].fill_(DB0)


def _snapshot(dev, bufs):
    """every buffer a backward may write, whole: the run's tensors, the conv input (`in = dx`), its scratch copy, dF, dB"""
    return [{k_: dev.down(d[k_]).copy() for k_ in ("O", "pre_out", "pool_out", "post_out", "X", "DXS", "DF", "DB") if k_ in d} for d in bufs]


@pytest.mark.parametrize("word", range(len(WORDS)), ids=[w[0] for w in WORDS])
@pytest.mark.parametrize("row", range(len(ROWS)))
def test_roles_banded_backward(t4k, dev, oracle, row, word):
    spec, H, W, Cin, stages, flat, want_bs = ROWS[row]
    wname, train = WORDS[word]
    r = _row(dev, oracle, row)
    N, arr, bufs, ref, params, DY = r["N"], r["arr"], r["bufs"], r["ref"], r["params"], r["DY"]
    ok, split, bsplit = plan(t4k, arr, len(stages), N)
    assert ok == 1, "row %d: the plan does not admit it" % row
    assert bsplit == want_bs, "row %d: bsplit %d, the row is written for %d" % (row, bsplit, want_bs)
    tag = "row %d %s (split %d, bsplit %d)" % (row, wname, split, bsplit)
    first_out = ctypes.c_void_p(arr[0].O)
    snaps = []
    for rep in range(3):
        _forward(t4k, dev, r, stages)
        if rep == 0 and r["fwd"] is None:          # the forward state this backward reads, and the oracle's backward from that very state
            got_fwd = down_stage(dev, bufs, ref, FWD_KEYS)
            x = r["X"]
            for si, st_ in enumerate(stages):
                got_fwd[si]["in"] = x
                x = got_fwd[si]["post_out" if st_[4] else ("pool_out" if st_[3] else ("pre_out" if st_[2] else "O"))]
                got_fwd[si]["last"] = x
            r["fwd"] = got_fwd
            r["want"] = _oracle_backward(oracle, got_fwd, stages, flat, params, DY)
        got_fwd, want = r["fwd"], r["want"]
        t4k.call("t4k_conv_stack_bwd", p(r["dDY"]), arr, len(stages), N, train, None)
        if train & 8:
            assert t4k.lib.t4k_conv_stack_dx0_pending(first_out) == 1, tag
            if rep == 0:
                _check_bwd_vs_oracle(dev, stages, want, bufs, tag, skip_dx0=True)
                witness_backward(stages, params, got_fwd, down_stage(dev, bufs, ref, BWD_KEYS), DY, DF0, DB0, who=tag, skip_dx0=True)
            t4k.call("t4k_conv_stack_dx0", arr, N, None)
            assert t4k.lib.t4k_conv_stack_dx0_pending(first_out) == 0, tag
        if rep == 0:
            got = down_stage(dev, bufs, ref, BWD_KEYS)
            if train & 1:
                _check_bwd_vs_oracle(dev, stages, want, bufs, tag)
                witness_backward(stages, params, got_fwd, got, DY, DF0, DB0, who=tag)
            else:
                # no parameter gradients: dF and dB keep what they held, bit for bit; the dX path and the run's tensors are checked as above
                # (the two helpers always look at dF / dB: they are handed the oracle's, which the last line below witnesses anyway)
                for si, d in enumerate(bufs):
                    assert np.all(dev.down(d["DF"]) == np.float32(DF0)) and np.all(dev.down(d["DB"]) == np.float32(DB0)), "%s stage %d: dF / dB written" % (tag, si)
                    d["DF"].copy_(dev.torch.from_numpy(want[si]["DF"] + np.float32(DF0))); d["DB"].copy_(dev.torch.from_numpy(want[si]["DB"] + np.float32(DB0)))
                _check_bwd_vs_oracle(dev, stages, want, bufs, tag)
                for si, d in enumerate(bufs):
                    d["DF"].fill_(DF0); d["DB"].fill_(DB0)
                got = [dict(g, DF=want[si]["DF"], DB=want[si]["DB"]) for si, g in enumerate(got)]
                witness_backward(stages, params, got_fwd, got, DY, None, None, who=tag)
            witness_backward(stages, params, got_fwd, oracle_bwd_as_got(want), DY, None, None, who="row %d oracle" % row)
        snaps.append(_snapshot(dev, bufs))
    for rep in (1, 2):
        for si in range(len(stages)):
            for k_, v in snaps[0][si].items():
                assert np.array_equal(v.view(np.uint32), snaps[rep][si][k_].view(np.uint32)), "%s: run %d differs from run 0 in stage %d %s" % (tag, rep, si, k_)


def _df_items(c1, C0, K, W):
    """dF work items of a stage: df_mgn x df_rg, the formulas of conv_stack_kernels.hip.inc (8 = the dF waves, not the workgroup's 16)"""
    mtt = (K * K * c1 + 15) // 16
    mg = min(mtt, 3)
    mgn = (mtt + mg - 1) // mg
    return mgn * min(8 // gcd(mgn, 8), max(1, W // 2))


def test_roles_rows_cover_what_they_are_written_for(t4k, dev):
    """over the rows: both dX engines, dF item counts below, at and above the 8 dF waves, and 2, 3 and 4 bands as reported by the plan"""
    engines, items, bsplits = set(), [], set()
    for row, (spec, H, W, Cin, stages, flat, want_bs) in enumerate(ROWS):
        N = n_of(spec)
        arr = (ConvStage * len(stages))()
        LAY = {"relu": 4, "tanh": 5, "dropout": 10, "avg": 13, "max": 14}
        h, w, c1 = H, W, Cin
        for si, (C0, K, pre, pool, post) in enumerate(stages):
            s = arr[si]; s.H, s.W, s.C1, s.C0, s.K = h, w, c1, C0, K
            s.F = s.B = s.O = s.X = 1                                         # non-null placeholders: the plan looks at shapes
            b = s.run; b.KS = 2 if pool else 1
            if pre:
                b.pre_layer = LAY[pre]; b.pre_mask = b.pre_out = 1
            if pool:
                b.pool_layer = LAY[pool]; b.pool_out = 1
            if post:
                b.post_layer = LAY[post]; b.post_mask = b.post_out = 1
            if flat and si == len(stages) - 1:
                b.copy_out = 1
            engines.add("dx_valu" if (c1 <= 4 and c1 * K * K * C0 <= 160) else "dx_mfma")
            items.append(_df_items(c1, C0, K, w))
            h, w, c1 = h // b.KS, w // b.KS, C0
        ok, sp, bs = plan(t4k, arr, len(stages), N)
        assert ok == 1 and bs == want_bs, "row %d: ok %d bsplit %d (wanted %d)" % (row, ok, bs, want_bs)
        bsplits.add(bs)
    print("dF items per stage:", items)
    assert engines == {"dx_valu", "dx_mfma"}, engines
    assert min(items) < 8 and 8 in items and max(items) > 8, items
    assert bsplits == {2, 3, 4}, bsplits


def test_roles_worst_witness_ratio_per_tensor_kind():
    """runs last in this module: the worst |err| / bound per tensor kind over everything above (printed with -s)"""
    for k_, (r, name) in sorted(wt.WORST.items()):
        print("%-16s %.3g  (%s)" % (k_, r, name))
        assert r <= 1.0
