"""t4k_groupnorm_plan (include/t4k.h, csrc/groupnorm.hip) and the witnesses of tests/gn_witness.py, on the host alone: nothing is launched
and no device is needed.

out = { rung (1 wave, 2 workgroup, 3 stream, 4 split), load path (4 | 1), groups per workgroup, parts per group, forward launches, dW | dB slices, fold kind
(1 fold_add, 2 df_fold), backward launches }.  The plan's rule, restated here (`expect`) and worked by hand in ROWS: with vw = 4 where aligned and Cg % 4 == 0
(else 1) and cgv = Cg / vw column items, a team of T threads sweeps RT = T / cgv rows at a time and a thread holds ceil(HW / RT) rows;
  rung 1  cgv <= 64 and at most 8 rows per thread of a wave;
  rung 2  else cgv <= 1024 and at most 4 rows of 16 bytes, or 8 of dwords, per thread of a 1024-thread workgroup;
  rung 4  else, where N G < 256: P = min(ceil(1024 / (N G)), 64, HW, HW cgv / 1024) parts of rp = ceil(HW / P) whole rows, P = ceil(HW / rp), if that is 2 or more;
  rung 3  else."""
import ctypes

import numpy as np
import pytest
import torch

import gn_witness as gw

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
WS = 32 << 20                                                            # what the entries hand the plan: half of the library's workspace
SENTINEL = [-7] * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, N, HW, C, G, aligned=1, ws=WS):
    out = I8(*SENTINEL)
    rc = lib.t4k_groupnorm_plan(N, HW, C, G, aligned, ws, out)
    return rc, list(out)


def cdiv(a, b):
    return -(-a // b)


def expect(N, HW, C, G, aligned):
    Cg = C // G; vw = 4 if aligned and Cg % 4 == 0 else 1; cgv = Cg // vw; NG = N * G
    rung, P, dw = 3, 1, (2 if vw == 1 else 1)
    if cgv <= 64 and cdiv(HW, 64 // cgv) <= 8:
        rung = 1
    elif cgv <= 1024 and cdiv(HW, 1024 // cgv) <= 4 * dw:
        rung = 2
    elif NG < 256:
        want = min(cdiv(1024, NG), 64, HW, HW * cgv // 1024)
        if want >= 2:
            rp = cdiv(HW, want); P = cdiv(HW, rp)
            rung = 4 if P >= 2 else 3
    ns = N * P
    return [rung, vw, 4 if rung == 1 else 1, P, 2 if rung == 4 else 1, ns, 1 if ns <= 32 else 2, 3 if rung == 4 else 2]


# ((N, HW, C, G, aligned), out) worked by hand; for every rung the largest E the plan still sends there and the smallest it sends on
ROWS = [
    ((2, 1, 7, 7, 1),        [1, 1, 4, 1, 1, 2, 1, 2]),        # E = 1
    ((3, 512, 1, 1, 1),      [1, 1, 4, 1, 1, 3, 1, 2]),        # cgv = 1: 64 rows a sweep, 8 sweeps: the largest wave group on dwords, E = 512
    ((3, 513, 1, 1, 1),      [2, 1, 1, 1, 1, 3, 1, 2]),        # ... E = 513: the workgroup
    ((3, 512, 8, 2, 1),      [1, 4, 4, 1, 1, 3, 1, 2]),        # Cg = 4 on 16 bytes: cgv = 1, E = 2048 is the largest wave group
    ((3, 513, 8, 2, 1),      [2, 4, 1, 1, 1, 3, 1, 2]),        # ... E = 2052
    ((3, 128, 8, 2, 0),      [1, 1, 4, 1, 1, 3, 1, 2]),        # the same layer off 16 bytes: cgv = 4, 16 rows a sweep, 8 sweeps
    ((3, 129, 8, 2, 0),      [2, 1, 1, 1, 1, 3, 1, 2]),
    ((3, 8, 64, 1, 0),       [1, 1, 4, 1, 1, 3, 1, 2]),        # cgv = 64: one row a sweep
    ((3, 9, 64, 1, 0),       [2, 1, 1, 1, 1, 3, 1, 2]),
    ((256, 8192, 1, 1, 1),   [2, 1, 1, 1, 1, 256, 2, 2]),      # the largest workgroup group on dwords, E = 8192 (more than 32 slices: df_fold)
    ((256, 8193, 1, 1, 1),   [3, 1, 1, 1, 1, 256, 2, 2]),      # ... E = 8193 with 256 groups: stream
    ((255, 8193, 1, 1, 1),   [4, 1, 1, 5, 2, 1275, 2, 3]),     # ... with 255: min(5, 64, 8193, 8) = 5 parts of 1639 rows
    ((64, 4096, 16, 4, 1),   [2, 4, 1, 1, 1, 64, 2, 2]),       # 16 bytes: E = 16384 is the largest workgroup group
    ((1, 4097, 4, 1, 1),     [4, 4, 1, 4, 2, 4, 1, 3]),        # one group of 16388 floats: 4 parts
    ((2, 40, 384, 1, 1),     [2, 4, 1, 1, 1, 2, 1, 2]),        # cgv = 96: 10 rows a sweep, 4 sweeps
    ((2, 41, 384, 1, 1),     [4, 4, 1, 3, 2, 6, 1, 3]),        # ... 5 sweeps: min(512, 64, 41, 3) = 3 parts of 14 rows
    ((256, 196, 384, 1, 1),  [3, 4, 1, 1, 1, 256, 2, 2]),      # layer norm 14 x 14 x 384 at N = 256
    ((8, 3136, 64, 1, 1),    [4, 4, 1, 49, 2, 392, 2, 3]),     # layer norm 56 x 56 x 64 at N = 8: min(128, 64, 3136, 49) = 49 parts of 64 rows
    ((1, 1, 8192, 1, 1),     [3, 4, 1, 1, 1, 1, 1, 2]),        # cgv = 2048 > 1024 and one row: nothing to cut
    ((3, 3, 1100, 1, 0),     [4, 1, 1, 3, 2, 9, 1, 3]),        # cgv = 1100 > 1024: two column chunks, 3 parts of one row
]


@pytest.mark.parametrize("args,out", ROWS, ids=["n%d_hw%d_c%d_g%d_a%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, out):
    rc, got = plan(lib, *args)
    assert rc == OK and got == out, (args, got, lib.t4k_last_error())
    assert got == expect(*args)
    assert got[4] == (2 if got[0] == 4 else 1) and got[7] == got[4] + 1            # the launch counts: the fold launch follows the backward's


def test_the_rule_over_a_sweep(lib):
    n = 0
    for N in (1, 3, 64, 255, 256):
        for HW in (1, 5, 63, 64, 65, 257, 512, 513, 4096, 4097):
            for C, G in ((1, 1), (3, 1), (3, 3), (8, 1), (8, 2), (8, 8), (12, 4), (64, 32), (7, 7), (384, 1), (260, 1), (4100, 1)):
                for al in (0, 1):
                    rc, got = plan(lib, N, HW, C, G, al, 1 << 40)
                    if N * HW * C >= 1 << 31:
                        assert rc == ERR_UNSUPPORTED and got == SENTINEL, (N, HW, C, G, al, got)
                    else:
                        assert rc == OK and got == expect(N, HW, C, G, al), (N, HW, C, G, al, got)
                    n += 1
    assert n == 5 * 10 * 12 * 2


def test_rejections(lib):
    """every rejection with its code, a text, and an untouched out"""
    def refused(code, text, *a, **kw):
        rc, out = plan(lib, *a, **kw)
        assert rc == code and out == SENTINEL and text in lib.t4k_last_error(), (a, kw, rc, out, lib.t4k_last_error())
    assert plan(lib, 3, 5, 8, 2)[0] == OK
    assert lib.t4k_groupnorm_plan(3, 5, 8, 2, 1, WS, None) == ERR_ARG
    for a in ((0, 5, 8, 2), (-1, 5, 8, 2), (3, 0, 8, 2), (3, -2, 8, 2), (3, 5, 0, 1), (3, 5, -8, 2)):
        refused(ERR_ARG, b"extent", *a)
    refused(ERR_ARG, b"ws_bytes", 3, 5, 8, 2, ws=-1)
    for G in (0, -1, 3, 5, 9, 16):
        refused(ERR_UNSUPPORTED, b"groups", 3, 5, 8, G)
    big = 1 << 40
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 16, 1 << 15, 1, 1, ws=big)
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 10, 1 << 10, 1 << 11, 1, ws=big)
    refused(ERR_UNSUPPORTED, b"2^31", (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, 1, ws=big)      # no overflow on the way to the verdict
    assert plan(lib, (1 << 31) - 1, 1, 1, 1, ws=big)[0] == OK and plan(lib, 1, (1 << 31) - 1, 1, 1, ws=big)[0] == OK
    assert plan(lib, 1, 1, (1 << 31) - 1, (1 << 31) - 1, ws=big)[0] == OK                            # N G below 2^31 whenever N HW C is
    # the slab: N P rows of 2 C floats behind the parts' 2 N G P floats (rounded up to 4)
    assert plan(lib, 3, 5, 8, 2, ws=3 * 16 * 4)[0] == OK
    refused(ERR_UNSUPPORTED, b"workspace", 3, 5, 8, 2, ws=3 * 16 * 4 - 1)
    assert plan(lib, 1, 4097, 4, 1, ws=(8 + 4 * 8) * 4)[0] == OK
    refused(ERR_UNSUPPORTED, b"workspace", 1, 4097, 4, 1, ws=(8 + 4 * 8) * 4 - 1)
    refused(ERR_UNSUPPORTED, b"workspace", (1 << 31) - 1, 1, 1, 1)


# ----------------------------------------------------------------------------- the witnesses against torch
PAIRS = [(1, 1), (3, 1), (3, 3), (8, 1), (8, 2), (8, 8), (12, 4), (6, 2)]


@pytest.mark.parametrize("C,G", PAIRS)
@pytest.mark.parametrize("HW", [1, 5, 63])
def test_witness_chain_is_group_norm(C, G, HW):
    """the staged witnesses chained end to end against torch.nn.functional.group_norm and its autograd in float64, NHWC <-> NCHW: the rule, the
    channel-to-group map and where eps sits"""
    rng = np.random.default_rng(100 * C + 10 * G + HW)
    N = 3
    X = rng.normal(0.5, 2.0, (N, HW, 1, C)); DY = rng.normal(0.0, 1.0, (N, HW, 1, C))
    Wg = rng.normal(1.0, 0.5, C); B = rng.normal(0.0, 0.5, C)
    DW0 = rng.normal(0.0, 1.0, C); DB0 = rng.normal(0.0, 1.0, C)
    wm, wr = gw.gn_stats(X, G)
    stat = np.concatenate([wm.exact.ravel(), wr.exact.ravel(), np.zeros(2 * N * G)])
    xh = gw.gn_xhat(X, stat, G).exact
    y = gw.gn_y(xh, Wg, B).exact
    ws1, ws2, wdw, wdb = gw.gn_bwd_stats(Wg, DY, xh, G, DW0, DB0, 1)
    stat[2 * N * G:3 * N * G] = ws1.exact.ravel(); stat[3 * N * G:] = ws2.exact.ravel()
    dx = gw.gn_dx(Wg, DY, xh, stat, G).exact
    tx = torch.tensor(X).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    tw = torch.tensor(Wg, requires_grad=True); tb = torch.tensor(B, requires_grad=True)
    ty = torch.nn.functional.group_norm(tx, G, tw, tb, gw.EPS)
    ty.backward(torch.tensor(DY).permute(0, 3, 1, 2).contiguous())
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).numpy()
    close = lambda a, b: np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b)))
    assert close(y, nhwc(ty)) and close(dx, nhwc(tx.grad))
    assert close(wdw.exact - DW0, tw.grad.numpy()) and close(wdb.exact - DB0, tb.grad.numpy())
    untouched = gw.gn_bwd_stats(Wg, DY, xh, G, DW0, DB0, 0)
    assert np.array_equal(untouched[2].exact, DW0) and np.array_equal(untouched[3].exact, DB0) and untouched[2].n == 0


def f32_sum(a, pairwise):
    a = np.asarray(a, np.float32)
    if pairwise:
        return np.sum(a, dtype=np.float32)
    s = np.float32(0.0)
    for v in a:
        s = np.float32(s + v)
    return s


@pytest.mark.parametrize("seed", range(5))
def test_the_rstd_bound_separates_the_two_formulas(seed):
    """x = 1024 + N(0, 1), one group of 63 x 1: a float32 restatement of the centred formula stays inside the rstd bound, a float32 E[x^2] - mean^2 leaves it"""
    x = (1024.0 + np.random.default_rng(seed).normal(0.0, 1.0, 63)).astype(np.float32)
    E = np.float32(63.0); eps = np.float32(gw.EPS)
    w = gw.gn_stats(x.reshape(1, 63, 1, 1), 1)[1]
    for pairwise in (True, False):
        m = np.float32(f32_sum(x, pairwise) / E)
        d = (x - m).astype(np.float32)
        centred = np.float32(1.0) / np.sqrt(np.float32(f32_sum(d * d, pairwise) / E + eps), dtype=np.float32)
        var = np.float32(np.float32(f32_sum(x * x, pairwise) / E) - np.float32(m * m))
        naive = np.float32(1.0) / np.sqrt(np.maximum(var, np.float32(0.0)) + eps, dtype=np.float32)
        rc = abs(float(centred) - float(w.exact[0, 0])) / float(w.bound()[0, 0])
        rn = abs(float(naive) - float(w.exact[0, 0])) / float(w.bound()[0, 0])
        print("seed %d %s: centred %.3g, naive %.3g of the bound" % (seed, "pairwise" if pairwise else "sequential", rc, rn))
        assert rc < 1.0 < rn, (seed, pairwise, rc, rn)
