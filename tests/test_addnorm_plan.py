"""t4k_addnorm_plan (include/t4k.h, csrc/addnorm.hip) and the witnesses of tests/an_witness.py, on the host alone: nothing is launched and no
device is needed.

out = { rung, load path (4 | 1), tokens per workgroup, lanes per token T, forward launches, dW | dB slab rows, fold kind, backward launches with train }.  The
plan's rule, restated here (`expect`) and worked by hand in ROWS: mode 0 is rung 0 (flat, no slab, one launch each way).  Else the load path is 16 bytes where
the call is aligned and C % 4 == 0; with items = C / load width, T is the first of 8, 16, 32, 64 with ceil(items / T) <= 8 (rung 1, 256 / T tokens per
workgroup), else the 256-thread workgroup where ceil(items / 256) <= 8 (rung 2, one token), else the call is refused.  The backward's workgroups - one slab
row of 2 C floats each - are as many as the token visits need, at most 1024 and at most what the workspace holds; each walks a contiguous slab of
ceil(visits / workgroups) visits.  Up to 32 rows a thread per output folds them, above a wave per output."""
import ctypes

import numpy as np
import pytest
import torch

import an_witness as an

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
WS = 32 << 20                                                            # what the entries hand the plan: half of the library's workspace
SENTINEL = [-7] * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, rows, C, mode, aligned=1, ws=WS):
    out = I8(*SENTINEL)
    rc = lib.t4k_addnorm_plan(rows, C, mode, aligned, ws, out)
    return rc, list(out)


def expect(rows, C, mode, aligned, ws=WS):
    """the rule in Python's unbounded integers; None: refused for its size"""
    if rows >= 1 << 31 or rows * C >= 1 << 31:
        return None
    vw = 4 if aligned and C % 4 == 0 else 1
    if mode == 0:
        return [0, vw, 0, 0, 1, 0, 0, 1]
    items = C // vw
    T = next((t for t in (8, 16, 32, 64) if -(-items // t) <= 8), None)
    if T is None and -(-items // 256) > 8:
        return None
    rung, T = (1, T) if T else (2, 256)
    tpw = 256 // T
    visits = -(-rows // tpw)
    fit = ws // 4 // (2 * C)
    if fit < 1:
        return None
    per = -(-visits // min(visits, 1024, fit)) * tpw
    nslice = -(-rows // per)
    return [rung, vw, tpw, T, 1, nslice, 1 if nslice <= 32 else 2, 2]


# ((rows, C, mode, aligned, ws), out) worked by hand: both sides of every threshold and of each T
ROWS = [
    ((7, 5, 0, 1, WS),          [0, 1, 0, 0, 1, 0, 0, 1]),               # mode 0: flat, whatever C
    ((7, 8, 0, 1, WS),          [0, 4, 0, 0, 1, 0, 0, 1]),
    ((7, 100000, 0, 0, WS),     [0, 1, 0, 0, 1, 0, 0, 1]),
    ((1, 1, 1, 1, WS),          [1, 1, 32, 8, 1, 1, 1, 2]),              # one item: T = 8, 32 tokens a workgroup
    ((25088, 192, 1, 1, WS),    [1, 4, 32, 8, 1, 784, 2, 2]),            # ViT-tiny: 48 items, 6 a lane; 784 visits, one each
    ((16384, 256, 2, 1, WS),    [1, 4, 32, 8, 1, 512, 2, 2]),            # 64 items: the last C of T = 8 on 16 bytes
    ((16384, 260, 1, 1, WS),    [1, 4, 16, 16, 1, 1024, 2, 2]),          # 65 items: T = 16
    ((100000, 512, 1, 1, WS),   [1, 4, 16, 16, 1, 893, 2, 2]),           # 128 items: the last of T = 16; 6250 visits over 1024 workgroups: 7 each = 112 tokens, 893 slabs
    ((10, 516, 2, 1, WS),       [1, 4, 8, 32, 1, 2, 1, 2]),              # 129 items: T = 32
    ((10, 1024, 1, 1, WS),      [1, 4, 8, 32, 1, 2, 1, 2]),              # 256 items: the last of T = 32
    ((10, 1028, 1, 1, WS),      [1, 4, 4, 64, 1, 3, 1, 2]),              # 257 items: T = 64
    ((10, 2048, 1, 1, WS),      [1, 4, 4, 64, 1, 3, 1, 2]),              # 512 items: the last of rung 1
    ((10, 2052, 1, 1, WS),      [2, 4, 1, 256, 1, 10, 1, 2]),            # 513 items: rung 2, a workgroup per token
    ((4096, 4096, 1, 1, WS),    [2, 4, 1, 256, 1, 1024, 2, 2]),          # 8192 floats a row: 1024 of them are the 32 MiB; 4 tokens a slab
    ((40, 8192, 2, 1, WS),      [2, 4, 1, 256, 1, 40, 2, 2]),            # 2048 items: the largest C
    ((10, 64, 1, 0, WS),        [1, 1, 32, 8, 1, 1, 1, 2]),              # dwords: 64 items, the last of T = 8
    ((10, 65, 1, 1, WS),        [1, 1, 16, 16, 1, 1, 1, 2]),             # 65 is no multiple of 4: dwords whatever the pointers; T = 16
    ((33, 128, 2, 0, WS),       [1, 1, 16, 16, 1, 3, 1, 2]),
    ((10, 129, 1, 0, WS),       [1, 1, 8, 32, 1, 2, 1, 2]),
    ((10, 256, 1, 0, WS),       [1, 1, 8, 32, 1, 2, 1, 2]),
    ((10, 257, 1, 0, WS),       [1, 1, 4, 64, 1, 3, 1, 2]),
    ((10, 512, 1, 0, WS),       [1, 1, 4, 64, 1, 3, 1, 2]),
    ((10, 513, 1, 0, WS),       [2, 1, 1, 256, 1, 10, 1, 2]),
    ((10, 2048, 2, 0, WS),      [2, 1, 1, 256, 1, 10, 1, 2]),            # the largest C on dwords
    ((5000, 4096, 1, 1, 98304), [2, 4, 1, 256, 1, 3, 1, 2]),             # a workspace of three slab rows: 1667 tokens a slab, rows no matter
    ((33, 20, 1, 1, WS),        [1, 4, 32, 8, 1, 2, 1, 2]),              # 33 tokens are two visits of 32
    ((32 * 1024 + 1, 20, 1, 1, WS), [1, 4, 32, 8, 1, 513, 2, 2]),        # 1025 visits over 1024 workgroups: two each, 513 slabs
]


@pytest.mark.parametrize("args,out", ROWS, ids=["r%d_c%d_m%d_a%d_w%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, out):
    rc, got = plan(lib, *args)
    assert rc == OK and got == out, (args, got, lib.t4k_last_error())
    assert out == expect(*args)
    assert out[4] == 1 and out[7] == (1 if args[2] == 0 else 2)             # the launch counts


def test_the_rule_over_a_sweep(lib):
    n = 0
    for rows in (1, 2, 31, 32, 33, 255, 256, 257, 4097, 25088, 32 * 1024, 32 * 1024 + 1, 1 << 20, (1 << 31) - 1, 1 << 31):
        for C in (1, 2, 3, 4, 5, 20, 63, 64, 65, 68, 128, 129, 252, 256, 257, 260, 512, 513, 516, 1024, 1028, 2048, 2049, 2052, 4096, 8192, 8193, 8196, 10000):
            for mode in (0, 1, 2):
                for al in (0, 1):
                    for ws in (WS, 1 << 40, 65536):
                        rc, got = plan(lib, rows, C, mode, al, ws)
                        want = expect(rows, C, mode, al, ws)
                        if want is None:
                            assert rc == ERR_UNSUPPORTED and got == SENTINEL, (rows, C, mode, al, ws, got)
                        else:
                            assert rc == OK and got == want, (rows, C, mode, al, ws, got, want)
                        n += 1
    assert n >= 5000


def test_rejections(lib):
    """every rejection with its code, a text, and an untouched out"""
    def refused(code, text, *a, **kw):
        rc, out = plan(lib, *a, **kw)
        assert rc == code and out == SENTINEL and text in lib.t4k_last_error(), (a, kw, rc, out, lib.t4k_last_error())
    assert plan(lib, 5, 20, 1)[0] == OK
    assert lib.t4k_addnorm_plan(5, 20, 1, 1, WS, None) == ERR_ARG
    for a in ((0, 20, 1), (-1, 20, 1), (5, 0, 1), (5, -20, 2), (0, 0, 0)):
        refused(ERR_ARG, b"extent", *a)
    for mode in (-1, 3, 7):
        refused(ERR_ARG, b"mode", 5, 20, mode)
    refused(ERR_ARG, b"ws_bytes", 5, 20, 1, ws=-1)
    big = 1 << 40
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 31, 1, 1, ws=big)
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 31, 1, 0, ws=big)
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 21, 1 << 10, 0, ws=big)
    refused(ERR_UNSUPPORTED, b"2^31", (1 << 31) - 1, (1 << 31) - 1, 2, ws=big)                        # no overflow on the way to the verdict
    assert plan(lib, (1 << 31) - 1, 1, 1, ws=big)[0] == OK
    assert plan(lib, (1 << 21) - 1, 1 << 10, 2, ws=big)[0] == OK
    # the channels: 8192 on 16 bytes, 2048 on dwords, any with mode 0
    for C, al in ((8196, 1), (8193, 1), (2049, 0), (2052, 0), (8192, 0), (1 << 20, 1)):
        refused(ERR_UNSUPPORTED, b"channels", 5, C, 1, al)
        refused(ERR_UNSUPPORTED, b"channels", 5, C, 2, al)
        assert plan(lib, 5, C, 0, al)[0] == OK
    # the workspace: one slab row of 2 C floats at least
    assert plan(lib, 5, 20, 1, ws=160)[0] == OK
    refused(ERR_UNSUPPORTED, b"workspace", 5, 20, 1, ws=159)
    refused(ERR_UNSUPPORTED, b"workspace", 5, 20, 2, ws=0)
    assert plan(lib, 5, 20, 0, ws=0)[0] == OK                                                         # mode 0 has no slab


# ----------------------------------------------------------------------------- the witnesses against torch
SHAPES = [(rows, C) for rows in (1, 5, 130) for C in (1, 3, 4, 20, 260)]
IDS = ["r%d_c%d" % s for s in SHAPES]
CASES = [(mode, skip, dy2) for mode in (0, 1, 2) for skip in (0, 1) for dy2 in (0, 1)]
CASE_IDS = ["m%d_s%d_d%d" % c for c in CASES]


def operands(rows, C, kind, seed, skip=1, dy2=1):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (rows, C)).astype(np.float32)
    s = rng.normal(0.0, 1.0, (rows, C)).astype(np.float32)
    if kind == "offset":
        x += np.float32(1024.0)
    elif kind == "small":                                                  # a variance near eps: where eps sits shows
        x *= np.float32(0.01); s *= np.float32(0.01)
    elif kind == "constant":
        x[:] = rng.normal(0.0, 1.0, (rows, 1)).astype(np.float32); s[:] = rng.normal(0.0, 1.0, (rows, 1)).astype(np.float32)
    w = rng.normal(1.0, 0.5, C).astype(np.float32); b = rng.normal(0.0, 0.5, C).astype(np.float32)
    dy = rng.normal(0.0, 1.0, (rows, C)).astype(np.float32); d2 = rng.normal(0.0, 1.0, (rows, C)).astype(np.float32)
    dw0 = rng.normal(0.0, 1.0, C).astype(np.float32); db0 = rng.normal(0.0, 1.0, C).astype(np.float32)
    return x, (s if skip else None), w, b, dy, (d2 if dy2 else None), dw0, db0


def torch_rule(x, s, w, b, mode, eps):
    z = x if s is None else x + s
    if mode == 0:
        return z
    if mode == 1:
        return torch.nn.functional.layer_norm(z, (z.shape[-1],), w, b, eps)
    return z * torch.rsqrt((z * z).mean(-1, keepdim=True) + eps) * w + b


@pytest.mark.parametrize("mode,skip,dy2", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("rows,C", SHAPES, ids=IDS)
def test_witness_chain_is_layer_norm_and_rms_norm(rows, C, mode, skip, dy2):
    """the staged witnesses chained end to end - every stage fed the exact value of the one in front - against torch's layer_norm / the RMS expression and its
    autograd in float64, to 1e-12: the rule, eps inside the root, the biased variance, dgamma | dbeta as sums on top of the prior value, and that x and the
    skip receive the same gradient"""
    X, S, Wg, B, DY, DY2, DW0, DB0 = operands(rows, C, "normal", 1000 * rows + 10 * C + mode + 3 * skip + 5 * dy2, skip, dy2)
    t64 = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64))
    x, s, w, b = t64(X).requires_grad_(True), t64(S), t64(Wg).requires_grad_(True), t64(B).requires_grad_(True)
    if s is not None:
        s.requires_grad_(True)
    y = torch_rule(x, s, w, b, mode, an.EPS)
    y.backward(t64(DY) if DY2 is None else t64(DY) + t64(DY2))
    close = lambda a, e: np.max(np.abs(np.asarray(a) - e.detach().numpy().reshape(np.shape(a)))) <= 1e-12 * max(1.0, float(e.detach().abs().max()))
    if mode == 0:
        assert close(an.an_z(X, S, C).exact, y)
        assert close(an.an_dx(None, DY, DY2, None, None, C, 0).exact, x.grad)
    else:
        r = an.an_rstd(X, S, C, mode).exact
        xh = an.an_xhat(X, S, r, C, mode).exact
        assert close(an.an_y(xh, Wg, B, C).exact, y)
        assert close(an.an_dx(Wg, DY, DY2, xh, r, C, mode).exact, x.grad)
        wdw, wdb = an.an_dwdb(DY, DY2, xh, DW0, DB0, C, 1)
        assert close(wdw.exact - DW0.astype(np.float64), w.grad) and close(wdb.exact - DB0.astype(np.float64), b.grad)
        wdw, wdb = an.an_dwdb(DY, DY2, xh, DW0, DB0, C, 0)
        assert np.array_equal(wdw.exact, DW0.astype(np.float64)) and np.array_equal(wdb.exact, DB0.astype(np.float64))
        z = X.astype(np.float64) + (0 if S is None else S.astype(np.float64))
        if mode == 1:
            assert np.max(np.abs(r - 1.0 / np.sqrt(z.var(1) + an.EPS))) <= 1e-12 * np.max(r)
    if s is not None:
        assert torch.equal(s.grad, x.grad)


PATHS = [(rows, C, vw) for rows, C in SHAPES for vw in (1, 4) if vw == 1 or C % 4 == 0]          # the 16-byte path needs C % 4 == 0


@pytest.mark.parametrize("kind", ["normal", "offset", "constant"])
@pytest.mark.parametrize("mode,skip,dy2", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("rows,C,vw", PATHS, ids=["r%d_c%d_v%d" % s for s in PATHS])
def test_a_float32_restatement_passes_every_bound(rows, C, vw, mode, skip, dy2, kind):
    """the team algorithm in NumPy float32 (a lane's items in order, the xor butterfly, the centred second pass) inside every bound, no element excepted: on
    N(0, 1), on 1024 + N(0, 1), and on constant rows"""
    ops = operands(rows, C, kind, 7 + rows + C + mode, skip, dy2)
    got = an.f32_addnorm(*ops, C, mode, 1, an.EPS, vw)
    r = an.ratios(*ops, C, mode, 1, *got)
    print(rows, C, mode, skip, dy2, vw, kind, r)
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("C", [1, 3, 4, 20, 260])
def test_constant_rows_have_no_variance(C):
    """x and s constant over a token's channels: var = 0, so rstd = 1 / sqrt(eps) and xhat = 0 to within their bounds (the witness's exact values are those)"""
    X, S, Wg, B, DY, DY2, DW0, DB0 = operands(5, C, "constant", 11 + C)
    w = an.an_rstd(X, S, C, 1)
    assert np.allclose(w.exact, 1.0 / np.sqrt(an.EPS), rtol=1e-12)
    assert np.max(np.abs(an.an_xhat(X, S, w.exact, C, 1).exact)) == 0.0
    O, XH, RSTD, DX, DW, DB = an.f32_addnorm(X, S, Wg, B, DY, DY2, DW0, DB0, C, 1)
    assert an.ratio(RSTD, w)[0] <= 1.0 and an.ratio(XH, an.an_xhat(X, S, RSTD, C, 1))[0] <= 1.0


def worst(ops, C, mode, wrong, vw=1):
    got = an.f32_addnorm(*ops, C, mode, 1, an.EPS, vw, wrong=wrong)
    return an.ratios(*ops, C, mode, 1, *got)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("rows,C", [s for s in SHAPES if s[1] >= 3], ids=["r%d_c%d" % s for s in SHAPES if s[1] >= 3])
def test_wrong_restatements_leave_the_bounds(rows, C, seed):
    """the bounds are tight enough to mean something: each of these leaves the bound of the stage it breaks, on every shape and seed"""
    ops = operands(rows, C, "normal", 31 * seed + rows + C)
    assert worst(operands(rows, C, "small", 31 * seed + rows + C), C, 1, "eps_outside")["rstd"] > 1.0     # (at var = 1 the two differ by 5e-6, inside the bound of a long row)
    if C <= 5:
        assert worst(ops, C, 1, "unbiased")["rstd"] > 1.0
    assert worst(operands(rows, C, "offset", 31 * seed + rows + C), C, 1, "ex2")["rstd"] > 1.0
    if rows > 1:
        assert worst(ops, C, 1, "dw_mean")["dw"] > 1.0 and worst(ops, C, 2, "dw_mean")["dw"] > 1.0
    for mode in (0, 1, 2):
        assert worst(ops, C, mode, "no_dy2")["dx"] > 1.0
    assert worst(ops, C, 1, "no_dy2")["dw"] > 1.0 and worst(ops, C, 2, "no_dy2")["db"] > 1.0
    assert worst(ops, C, 2, "rms_centred")["rstd"] > 1.0
