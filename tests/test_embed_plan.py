"""t4k_embed_plan (include/t4k.h, csrc/embed.hip) and the witnesses of tests/embed_witness.py, on the host alone: nothing is launched and no
device is needed.

out = { rung, load path (4 | 1), table rows of a slab R, token parts P, forward launches, backward launches with train, workgroups of the scatter launch,
workspace bytes used }.  The rule, restated in embed_witness.expect and worked by hand in ROWS: the load path is 16 bytes where the call is aligned and E % 4
== 0; items = E / width.  Position mode (V = 0) is rung 0: one launch each way, ceil(L items / 16) workgroups of the dPOS | DX role.  Token mode: a wave unit
owns 16 table rows x 64 items x one part, so the vocabulary alone gives ceil(V / 16) ceil(items / 64) units; P = min(ceil(1024 / units), T / 64, workspace /
(4 V E)), at least 1, then re-counted from whole 64-id loads per part; rung 1 for P = 1, 2 above; four units a workgroup, plus the dPOS role's where pos."""
import ctypes

import numpy as np
import pytest
import torch

import embed_witness as ew
from embed_witness import OK, ERR_ARG, ERR_UNSUPPORTED

I8 = ctypes.c_int * 8
WS = 32 << 20                                                            # what the entries hand the plan: half of the library's workspace
SENTINEL = [-7] * 8


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, T, L, V, E, pos, aligned=1, ws=WS):
    out = I8(*SENTINEL)
    rc = lib.t4k_embed_plan(T, L, V, E, pos, aligned, ws, out)
    return rc, list(out)


# ((T, L, V, E, pos, aligned, ws), out) worked by hand: both sides of every threshold
ROWS = [
    ((16384, 256, 65, 128, 1, 1, WS),      [2, 4, 16, 128, 1, 2, 672, 4259840]),  # a character model: 5 slabs x 1 chunk; P = min(205, 256, 1008) = 205 -> 2 id loads a part = 128 parts; 160 + 512 workgroups
    ((8192, 512, 32768, 512, 0, 1, WS),    [1, 4, 16, 1, 1, 1, 1024, 0]),         # a BPE table: 2048 slabs x 2 chunks fill the device, and one part's rows (64 MiB) fit no workspace
    ((25088, 196, 0, 192, 1, 1, WS),       [0, 4, 0, 1, 1, 1, 588, 0]),           # ViT-tiny positions: 196 x 48 items, 16 a workgroup
    ((64, 64, 64, 4, 0, 1, WS),            [1, 4, 16, 1, 1, 1, 1, 0]),            # R: 64 rows are 4 slabs = one workgroup of four units
    ((64, 64, 65, 4, 0, 1, WS),            [1, 4, 16, 1, 1, 1, 2, 0]),            # ... 65 a fifth slab
    ((64, 64, 64, 256, 0, 1, WS),          [1, 4, 16, 1, 1, 1, 1, 0]),            # 64 items: one chunk
    ((64, 64, 64, 260, 0, 1, WS),          [1, 4, 16, 1, 1, 1, 2, 0]),            # 65 items: two
    ((127, 127, 16, 4, 0, 1, WS),          [1, 4, 16, 1, 1, 1, 1, 0]),            # P: 127 tokens are one part
    ((128, 64, 16, 4, 0, 1, WS),           [2, 4, 16, 2, 1, 2, 1, 512]),          # ... 128 two of 64
    ((1024, 64, 16368, 4, 0, 1, WS),       [2, 4, 16, 2, 1, 2, 512, 523776]),     # 1023 units by themselves: ceil(1024 / 1023) = 2 parts
    ((1024, 64, 16384, 4, 0, 1, WS),       [1, 4, 16, 1, 1, 1, 256, 0]),          # 1024: the device is full, one part
    ((1024, 64, 16, 4, 0, 1, 1023),        [2, 4, 16, 3, 1, 2, 1, 768]),          # the workspace bound: three parts' rows (256 bytes each) fit 1023 bytes
    ((1024, 64, 16, 4, 0, 1, 1024),        [2, 4, 16, 4, 1, 2, 1, 1024]),         # ... four fit 1024
    ((1024, 64, 16, 4, 0, 1, 255),         [1, 4, 16, 1, 1, 1, 1, 0]),            # ... none fits 255: direct
    ((1024, 64, 16, 4, 0, 1, 0),           [1, 4, 16, 1, 1, 1, 1, 0]),
    ((2305, 2305, 16, 4, 0, 1, WS),        [2, 4, 16, 19, 1, 2, 5, 4864]),        # T / 64 = 36 parts of ceil(37 / 36) = 2 id loads = 128 tokens are 19 parts
    ((64, 64, 16, 6, 1, 1, WS),            [1, 1, 16, 1, 1, 1, 25, 0]),           # E % 4 != 0: dwords whatever the pointers; 64 x 6 items for dPOS = 24 workgroups
    ((64, 64, 16, 8, 1, 0, WS),            [1, 1, 16, 1, 1, 1, 33, 0]),           # E % 4 == 0, a pointer off 16 bytes: dwords
    ((64, 64, 16, 8, 1, 1, WS),            [1, 4, 16, 1, 1, 1, 9, 0]),            # ... aligned: 16 bytes, 64 x 2 items = 8 workgroups
    ((6, 3, 0, 5, 1, 1, WS),               [0, 1, 0, 1, 1, 1, 1, 0]),             # position mode, 15 items
    ((1, 1, 1, 1, 0, 1, WS),               [1, 1, 16, 1, 1, 1, 1, 0]),            # the smallest call
]


@pytest.mark.parametrize("args,out", ROWS, ids=["t%d_l%d_v%d_e%d_p%d_a%d_w%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, out):
    rc, got = plan(lib, *args)
    assert rc == OK and got == out, (args, got, lib.t4k_last_error())
    assert out == ew.expect(*args)
    assert out[4] == 1 and out[5] == max(1, out[0]) and out[0] == (0 if args[2] == 0 else 1 if out[3] == 1 else 2)


def test_the_rule_over_a_sweep(lib):
    n = 0
    for N in (1, 2, 3, 64, 129):
        for L in (1, 5, 64, 65, 196, 512):
            for V in (0, 1, 15, 16, 17, 35, 65, 1000, 16368, 16384, 32768, 1 << 22):
                for E in (1, 3, 4, 20, 64, 128, 256, 260, 512, 513):
                    for pos in (0, 1):
                        for al, ws in ((1, WS), (0, WS), (1, 1 << 40), (1, 65536)):
                            rc, got = plan(lib, N * L, L, V, E, pos, al, ws)
                            want = ew.expect(N * L, L, V, E, pos, al, ws)
                            if isinstance(want, int):
                                assert rc == want and got == SENTINEL, (N, L, V, E, pos, al, ws, rc, got)
                            else:
                                assert rc == OK and got == want, (N, L, V, E, pos, al, ws, got, want)
                                assert want[7] <= min(ws, (1 << 31) - 1) and want[3] >= 1
                            n += 1
    assert n >= 5000


def test_rejections(lib):
    """every rejection with its code, a text, and an untouched out"""
    def refused(code, text, *a, **kw):
        rc, out = plan(lib, *a, **kw)
        assert rc == code and out == SENTINEL and text in lib.t4k_last_error(), (a, kw, rc, out, lib.t4k_last_error())
    assert plan(lib, 10, 5, 7, 4, 1)[0] == OK
    assert lib.t4k_embed_plan(10, 5, 7, 4, 1, 1, WS, None) == ERR_ARG
    for a in ((0, 5, 7, 4, 1), (-10, 5, 7, 4, 1), (10, 0, 7, 4, 1), (10, -5, 7, 4, 1), (10, 5, -1, 4, 1), (10, 5, 7, 0, 1), (10, 5, 7, -4, 0), (0, 0, 0, 0, 0)):
        refused(ERR_ARG, b"extent", *a)
    refused(ERR_ARG, b"multiple", 10, 3, 7, 4, 1)
    refused(ERR_ARG, b"multiple", 3, 10, 7, 4, 1)
    refused(ERR_ARG, b"ws_bytes", 10, 5, 7, 4, 1, ws=-1)
    for pos in (-1, 2, 7):
        refused(ERR_ARG, b"pos=", 10, 5, 7, 4, pos)
    refused(ERR_ARG, b"neither", 10, 5, 0, 4, 0)
    big = 1 << 40
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 31, 1, 1, 1, 0, ws=big)
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 21, 1, 1, 1 << 10, 0, ws=big)                            # T E
    refused(ERR_UNSUPPORTED, b"2^31", 10, 5, 1 << 21, 1 << 10, 0, ws=big)                           # V E
    refused(ERR_UNSUPPORTED, b"2^31", 10, 5, (1 << 31) - 1, (1 << 31) - 1, 1, ws=big)               # no overflow on the way to the verdict
    refused(ERR_UNSUPPORTED, b"2^31", (1 << 62), 1, 1, (1 << 31) - 1, 1, ws=big)
    assert plan(lib, (1 << 31) - 1, 1, 1, 1, 1, ws=big)[0] == OK
    assert plan(lib, (1 << 21) - 1, 1, (1 << 21) - 1, 1 << 10, 0, ws=big)[0] == OK


# ----------------------------------------------------------------------------- the witnesses
GRID = [(N, L, V, E) for N in (1, 2, 3) for L in (1, 5, 65) for V in (2, 17, 35) for E in (1, 4, 20)]
GRID_IDS = ["n%d_l%d_v%d_e%d" % g for g in GRID]


def operands(N, L, V, E, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    T = N * L
    ids = ew.make_ids(rng, T, V, kind)
    ids[0] = np.float32(0.75)                                              # row 0 is named (by truncation) ...
    if T > 1:
        ids[1] = np.float32(-1.0)                                          # ... and one token is padding
    table = rng.normal(0.0, 1.0, (V, E)).astype(np.float32); pos = rng.normal(0.0, 0.02, (L, E)).astype(np.float32)
    dy = rng.normal(0.0, 1.0, (T, E)).astype(np.float32)
    dt0 = rng.normal(0.0, 1.0, (V, E)).astype(np.float32); dp0 = rng.normal(0.0, 1.0, (L, E)).astype(np.float32)
    return ids, table, pos, dy, dt0, dp0


@pytest.mark.parametrize("N,L,V,E", GRID, ids=GRID_IDS)
def test_the_witness_is_torch_embedding_with_padding(N, L, V, E):
    """the float64 rule and its gradients against torch's F.embedding(padding_idx) + position and autograd in float64, and fwd32 against the token loop"""
    T = N * L
    ids, table, pos, dy, dt0, dp0 = operands(N, L, V, E, 100 * N + 10 * L + V + E)
    ok, idv = ew.valid_ids(ids, V)
    tab = torch.tensor(np.concatenate([table.astype(np.float64), np.zeros((1, E))]), requires_grad=True)     # row V: the padding row
    p = torch.tensor(pos.astype(np.float64), requires_grad=True)
    y = torch.nn.functional.embedding(torch.tensor(np.where(ok, idv, V)), tab, padding_idx=V).reshape(N, L, E) + p
    y.backward(torch.tensor(dy.astype(np.float64)).reshape(N, L, E))
    f64 = ew.fwd64(ids, table, pos, T, L, V, E)
    assert np.max(np.abs(f64 - y.detach().numpy().reshape(T, E))) <= 1e-12
    assert np.max(np.abs(ew.fwd32(ids, table, pos, T, L, V, E).astype(np.float64) - f64)) <= 2.0 ** -24 * np.max(np.abs(f64))    # one rounding
    wt, wp = ew.em_dtable(ids, dy, dt0, V, E), ew.em_dpos(dy, dp0, T, L, E)
    assert np.max(np.abs(wt.exact - dt0 - tab.grad.numpy()[:V])) <= 1e-12 * max(1.0, np.abs(wt.exact).max())
    assert np.max(np.abs(wp.exact - dp0 - p.grad.numpy())) <= 1e-12 * max(1.0, np.abs(wp.exact).max())
    assert np.array_equal(ew.em_dtable(ids, dy, dt0, V, E, 0).exact, dt0.astype(np.float64))
    # position mode: out = x + pos
    x = np.random.default_rng(5).normal(0, 1, (T, E)).astype(np.float32)
    assert np.array_equal(ew.fwd32(x, None, pos, T, L, 0, E), (x.reshape(N, L, E) + pos).reshape(T, E))
    assert np.max(np.abs(ew.fwd64(x, None, pos, T, L, 0, E) - (x.astype(np.float64).reshape(N, L, E) + pos).reshape(T, E))) == 0.0


@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("N,L,V,E", GRID, ids=GRID_IDS)
def test_a_float32_restatement_passes_the_bound(N, L, V, E, P):
    """the slab / parts / fold order in NumPy float32 inside the bound, no element excepted; rows no token names keep their bits"""
    T = N * L
    ids, table, pos, dy, dt0, dp0 = operands(N, L, V, E, 7 + N + L + V + E)
    P = min(P, ew.cdiv(T, 64))
    P = ew.cdiv(T, ew.part_len(T, P))
    DT, DP = ew.bwd32(ids, dy, dt0, dp0, T, L, V, E, P)
    wt = ew.em_dtable(ids, dy, dt0, V, E)
    rt, rp = ew.ratio(DT, wt)[0], ew.ratio(DP, ew.em_dpos(dy, dp0, T, L, E))[0]
    print(N, L, V, E, P, rt, rp)
    assert rt <= 1.0 and rp <= 1.0
    unhit = np.asarray(wt.n)[:, 0] == 0
    assert np.array_equal(DT[unhit].view(np.uint32), dt0[unhit].view(np.uint32))


@pytest.mark.parametrize("N,L,V,E", GRID, ids=GRID_IDS)
def test_wrong_restatements_leave_the_bounds(N, L, V, E):
    """the checks are tight enough to mean something: each of these fails on every shape of the grid - ids rounded instead of truncated (ids at k + 0.75),
    padding tokens contributing gradient, and (N >= 2, L >= 2: with one position or one sample the two indexings are one) the position indexed by t"""
    T = N * L
    ids, table, pos, dy, dt0, dp0 = operands(N, L, V, E, 31 + N + L + V + E, "frac")
    wt = ew.em_dtable(ids, dy, dt0, V, E)
    good = ew.fwd32(ids, table, pos, T, L, V, E)
    assert not np.array_equal(ew.fwd32(ids, table, pos, T, L, V, E, wrong="round"), good)
    assert ew.ratio(ew.bwd32(ids, dy, dt0, None, T, L, V, E, 1, wrong="round")[0], wt)[0] > 1.0
    if T > 1:
        assert ew.ratio(ew.bwd32(ids, dy, dt0, None, T, L, V, E, 1, wrong="pad_row0")[0], wt)[0] > 1.0
        assert not np.array_equal(ew.fwd32(ids, table, pos, T, L, V, E, wrong="pad_row0"), good)
    if N >= 2 and L >= 2:
        assert not np.array_equal(ew.fwd32(ids, table, pos, T, L, V, E, wrong="pos_t"), good)
        assert ew.ratio(ew.bwd32(ids, dy, dt0, dp0, T, L, V, E, 1, wrong="pos_t")[1], ew.em_dpos(dy, dp0, T, L, E))[0] > 1.0
