"""t4k_attention_plan (include/t4k.h, csrc/attention.hip) and the witnesses of tests/attn_witness.py, on the host alone: nothing is launched and
no device is needed.

out = { rung, load path (4 | 1), query tile BQ, key tile BK, forward launches, backward launches, workgroups of the forward, workspace bytes }.  The plan's rule,
restated here (`expect`) and worked by hand in ROWS: the head size is padded to DP = 16, 32, 64 or 128, the first that holds d, and the rung is that tier (1..4);
BQ = 64 always; BK = 64, but 32 on rung 4 (two LDS tiles of BK x 132 floats: 67.6 KB at 64 rows, 33.8 KB at 32); the forward is one launch of
N heads ceil(L / 64) workgroups, the backward two; the workspace holds one float per (n, head, token)."""
import ctypes

import numpy as np
import pytest
import torch

import attn_witness as aw

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
WS = 32 << 20                                                            # what the entries hand the plan: half of the library's workspace
SENTINEL = [-7] * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, N, L, heads, d, causal=0, aligned=1, ws=WS):
    out = I8(*SENTINEL)
    rc = lib.t4k_attention_plan(N, L, heads, d, causal, aligned, ws, out)
    return rc, list(out)


def expect(N, L, heads, d, aligned):
    rung = 1 if d <= 16 else 2 if d <= 32 else 3 if d <= 64 else 4
    return [rung, 4 if aligned else 1, 64, 32 if rung == 4 else 64, 1, 2, N * heads * -(-L // 64), 4 * N * heads * L]


# ((N, L, heads, d, aligned), out) worked by hand: both sides of every threshold - the head sizes 16 | 20, 32 | 36, 64 | 68, and the tile count at L = 64 | 65
ROWS = [
    ((1, 1, 1, 4, 1),        [1, 4, 64, 64, 1, 2, 1, 4]),
    ((2, 64, 3, 16, 1),      [1, 4, 64, 64, 1, 2, 6, 1536]),         # d = 16: the last head size of rung 1; one tile of 64 queries
    ((2, 65, 3, 20, 1),      [2, 4, 64, 64, 1, 2, 12, 1560]),        # d = 20: rung 2; 65 tokens are two tiles
    ((256, 64, 4, 32, 1),    [2, 4, 64, 64, 1, 2, 1024, 262144]),
    ((1, 128, 1, 36, 0),     [3, 1, 64, 64, 1, 2, 2, 512]),          # d = 36: rung 3, on dwords
    ((128, 196, 3, 64, 1),   [3, 4, 64, 64, 1, 2, 1536, 301056]),    # the ViT-tiny-like row: 4 tiles of 64 over 196 tokens
    ((8, 1024, 8, 68, 1),    [4, 4, 64, 32, 1, 2, 1024, 262144]),    # d = 68: rung 4, key tiles of 32
    ((1, 63, 2, 128, 0),     [4, 1, 64, 32, 1, 2, 2, 504]),
]


@pytest.mark.parametrize("args,out", ROWS, ids=["n%d_l%d_h%d_d%d_a%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, out):
    N, L, heads, d, al = args
    for causal in (0, 1):                                                  # the mask changes the tiles a workgroup visits, not the plan
        rc, got = plan(lib, N, L, heads, d, causal, al)
        assert rc == OK and got == out, (args, got, lib.t4k_last_error())
    assert out == expect(*args)
    assert out[4] == 1 and out[5] == 2                                     # the launch counts


def test_the_rule_over_a_sweep(lib):
    n = 0
    for N in (1, 2, 7, 256):
        for L in (1, 2, 63, 64, 65, 196, 1024, 4097):
            for heads in (1, 3, 8):
                for d in (4, 8, 16, 20, 32, 36, 60, 64, 68, 100, 128):
                    for al in (0, 1):
                        rc, got = plan(lib, N, L, heads, d, n & 1, al, 1 << 40)
                        if N * L * 3 * heads * d >= 1 << 31:
                            assert rc == ERR_UNSUPPORTED and got == SENTINEL, (N, L, heads, d, al, got)
                        else:
                            assert rc == OK and got == expect(N, L, heads, d, al), (N, L, heads, d, al, got)
                        n += 1
    assert n == 4 * 8 * 3 * 11 * 2 and n >= 1000


def test_rejections(lib):
    """every rejection with its code, a text, and an untouched out"""
    def refused(code, text, *a, **kw):
        rc, out = plan(lib, *a, **kw)
        assert rc == code and out == SENTINEL and text in lib.t4k_last_error(), (a, kw, rc, out, lib.t4k_last_error())
    assert plan(lib, 2, 5, 3, 8)[0] == OK
    assert lib.t4k_attention_plan(2, 5, 3, 8, 0, 1, WS, None) == ERR_ARG
    for a in ((0, 5, 3, 8), (-1, 5, 3, 8), (2, 0, 3, 8), (2, -5, 3, 8), (2, 5, 0, 8), (2, 5, -3, 8)):
        refused(ERR_ARG, b"extent", *a)
    refused(ERR_ARG, b"ws_bytes", 2, 5, 3, 8, ws=-1)
    for d in (-4, 0, 1, 2, 3, 5, 6, 18, 127, 130, 132, 256):
        refused(ERR_UNSUPPORTED, b"head size", 2, 5, 3, d)
    for d in (4, 8, 124, 128):
        assert plan(lib, 2, 5, 3, d)[0] == OK
    big = 1 << 40
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 10, 1 << 10, 8, 128, ws=big)                               # 3 x 2^30
    refused(ERR_UNSUPPORTED, b"2^31", (1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1, 128, ws=big)         # no overflow on the way to the verdict
    refused(ERR_UNSUPPORTED, b"2^31", 1, 1, (1 << 31) - 1, 4, ws=big)
    assert plan(lib, 1, 44739242, 1, 16, ws=big)[0] == OK                                              # 48 x 44739242 = 2^31 - 32
    refused(ERR_UNSUPPORTED, b"2^31", 1, 44739243, 1, 16, ws=big)                                     # ... + 16
    # the workspace: one float per (n, head, token)
    assert plan(lib, 2, 5, 3, 8, ws=120)[0] == OK
    refused(ERR_UNSUPPORTED, b"workspace", 2, 5, 3, 8, ws=119)
    refused(ERR_UNSUPPORTED, b"workspace", 2, 5, 3, 8, ws=0)


# ----------------------------------------------------------------------------- the witnesses against torch
SHAPES = [(L, d, heads) for L in (1, 5, 64, 130) for d in (4, 20, 64) for heads in (1, 3)]
IDS = ["l%d_d%d_h%d" % s for s in SHAPES]


def operands(L, d, heads, kind, seed, N=2):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (N, L, 3, heads, d)).astype(np.float32)
    if kind == "peaked":
        x[:, :, 0] *= 8.0
    elif kind == "zero":
        x[:, :, 0] = 0.0
    dy = rng.normal(0.0, 1.0, (N, L, heads * d)).astype(np.float32)
    return x.reshape(N, L, 3 * heads * d), dy


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("L,d,heads", SHAPES, ids=IDS)
def test_witness_chain_is_scaled_dot_product_attention(L, d, heads, causal):
    """the staged witnesses chained end to end against torch's scaled_dot_product_attention and its autograd in float64, to 1e-12: the rule, the [ Q | K | V ] and
    head order, the scale, the mask, and the log-sum-exp"""
    QKV, DY = operands(L, d, heads, "normal", 1000 * L + 10 * d + heads + causal)
    wl, wy = aw.fwd(QKV, heads, causal, 64)
    wd, wg = aw.bwd(QKV, wy.exact, DY, wl.exact, heads, causal)
    N = QKV.shape[0]
    t = torch.tensor(QKV.astype(np.float64)).reshape(N, L, 3, heads, d).permute(2, 0, 3, 1, 4).contiguous().requires_grad_(True)
    ty = torch.nn.functional.scaled_dot_product_attention(t[0], t[1], t[2], is_causal=bool(causal), scale=aw.scale_of(d))
    ty.backward(torch.tensor(DY.astype(np.float64)).reshape(N, L, heads, d).permute(0, 2, 1, 3))
    close = lambda a, b: np.max(np.abs(a - b)) <= 1e-12 * max(1.0, np.max(np.abs(b)))
    assert close(wy.exact, ty.detach().permute(0, 2, 1, 3).reshape(N, L, heads * d).numpy())
    assert close(wg.exact, t.grad.permute(1, 3, 0, 2, 4).reshape(N, L, 3 * heads * d).numpy())
    s = torch.einsum("nhid,nhjd->nhij", t[0], t[1]).detach() * aw.scale_of(d)
    if causal:
        s = s.masked_fill(~torch.tensor(aw.live(L, 1)), -np.inf)
    assert close(wl.exact, torch.logsumexp(s, -1).numpy())
    assert close(wd.exact, (aw.to_heads(DY, heads) * aw.to_heads(wy.exact, heads)).sum(-1))


@pytest.mark.parametrize("kind", ["normal", "peaked", "zero"])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("L,d,heads", SHAPES, ids=IDS)
def test_a_float32_restatement_passes_every_bound(L, d, heads, causal, kind):
    """the tiled online algorithm in NumPy float32 (tiles of 64, a rescale per tile, np.exp in float32 - within ULP_EXP's allowance) inside every bound, no
    element excepted"""
    QKV, DY = operands(L, d, heads, kind, 7 + L + d + heads)
    r = aw.ratios(QKV, DY, heads, causal, 64, *aw.f32_attention(QKV, DY, heads, causal, 64))
    print(L, d, heads, causal, kind, r)
    assert all(v <= 1.0 for v in r.values()), r


WRONG_SHAPES = [s for s in SHAPES if s[0] >= 5]


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("L,d,heads", WRONG_SHAPES, ids=["l%d_d%d_h%d" % s for s in WRONG_SHAPES])
def test_wrong_restatements_leave_the_bounds(L, d, heads, seed):
    """the bounds are tight enough to mean something: the scale omitted, and the causal mask with j < i (judged on the rows behind the first, which has no key
    at all then), each leave at least one bound on every shape and seed"""
    QKV, DY = operands(L, d, heads, "normal", 31 * seed + L + d + heads)
    for causal in (0, 1):
        r = aw.ratios(QKV, DY, heads, causal, 64, *aw.f32_attention(QKV, DY, heads, causal, 64, wrong="noscale"))
        assert max(r.values()) > 1.0, ("noscale", causal, r)
    Y, LSE, D, G = aw.f32_attention(QKV, DY, heads, 1, 64, wrong="strict")
    from f64_witness import ratio
    wl, wy = aw.fwd(QKV, heads, 1, 64)
    assert ratio(Y[:, 1:], aw.WB(wy.exact[:, 1:], wy.bound()[:, 1:]))[0] > 1.0 and ratio(LSE[:, :, 1:], aw.WB(wl.exact[:, :, 1:], wl.bound()[:, :, 1:]))[0] > 1.0


@pytest.mark.parametrize("d,heads", [(4, 1), (20, 3), (64, 1)])
def test_a_missing_rescale_leaves_the_bounds(d, heads):
    """the running output not rescaled when the max rises: only an operand whose max rises behind the first tile shows it - peaked rows over 130 keys"""
    QKV, DY = operands(130, d, heads, "peaked", 5 + d)
    for causal in (0, 1):
        r = aw.ratios(QKV, DY, heads, causal, 64, *aw.f32_attention(QKV, DY, heads, causal, 64, wrong="norescale"))
        assert r["y"] > 1.0, (causal, r)
