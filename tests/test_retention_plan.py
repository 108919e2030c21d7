"""t4k_retention_plan (include/t4k.h, csrc/retention.hip) on the host alone, and the float64 rule the GPU tests hold the kernels to.

out = { rung, load path (4 | 1), chunk B, chunks, forward launches, backward launches, workgroups of the chunk launch, workspace bytes }.  The head size is
padded to 16, 32, 64 or 128 (rung 1..4); B = 64, but 32 on rung 4; one chunk is one launch each way, more are three; the workspace holds the reverse
states, 4 N heads (chunks - 1) d d bytes."""
import ctypes

import numpy as np
import pytest

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
I8 = ctypes.c_int * 8
WS = 32 << 20                                                            # what the entries hand the plan: half of the library's workspace
SENTINEL = [-7] * 8


def rule(QKV, DY, heads):
    """Y [N, L, E] and DQKV [N, L, 3E] of the O(L^2) rule in float64 from float32 operands.  Called on the operands' absolute values it gives the bound's M:
    the same sums taken over absolute values"""
    N, L, C = QKV.shape
    d = C // 3 // heads
    x = QKV.astype(np.float64).reshape(N, L, 3, heads, d)
    q, k, v, dy = x[:, :, 0], x[:, :, 1], x[:, :, 2], DY.astype(np.float64).reshape(N, L, heads, d)
    scale = float(np.float32(1.0 / np.sqrt(float(d))))
    dist = np.arange(L)[:, None] - np.arange(L)[None, :]
    Y, G = np.zeros((N, L, heads, d)), np.zeros((N, L, 3, heads, d))
    for h in range(heads):
        D = np.where(dist >= 0, (1.0 - 2.0 ** (-5 - h)) ** np.maximum(dist, 0), 0.0)
        S = np.einsum("nik,njk->nij", q[:, :, h], k[:, :, h]) * D
        T = np.einsum("nic,njc->nij", dy[:, :, h], v[:, :, h]) * D
        Y[:, :, h] = scale * np.einsum("nij,njc->nic", S, v[:, :, h])
        G[:, :, 0, h] = scale * np.einsum("nij,njk->nik", T, k[:, :, h])
        G[:, :, 1, h] = scale * np.einsum("nij,nik->njk", T, q[:, :, h])
        G[:, :, 2, h] = scale * np.einsum("nij,nic->njc", S, dy[:, :, h])
    return Y.reshape(N, L, C // 3), G.reshape(N, L, C)


@pytest.fixture(scope="module")
def lib():
    from tensorforth_amd.lib import load
    return load().lib


def plan(lib, N, L, heads, d, aligned=1, ws=WS):
    out = I8(*SENTINEL)
    rc = lib.t4k_retention_plan(N, L, heads, d, aligned, ws, out)
    return rc, list(out)


# ((N, L, heads, d, aligned), out) worked by hand: both sides of the head sizes 16 | 20, 32 | 36, 64 | 68 and of the chunk count at L = B | B + 1
ROWS = [
    ((1, 1, 1, 4, 1),       [1, 4, 64, 1, 1, 1, 1, 0]),
    ((2, 64, 3, 16, 1),     [1, 4, 64, 1, 1, 1, 6, 0]),               # L = B: one chunk, one launch, no reverse state
    ((2, 65, 3, 20, 1),     [2, 4, 64, 2, 3, 3, 12, 9600]),           # L = B + 1: two chunks; 4 x 2 x 3 x 1 x 400
    ((4, 131, 2, 32, 0),    [2, 1, 64, 3, 3, 3, 24, 65536]),          # on dwords; 4 x 4 x 2 x 2 x 1024
    ((1, 128, 1, 36, 1),    [3, 4, 64, 2, 3, 3, 2, 5184]),
    ((2, 2048, 8, 64, 1),   [3, 4, 64, 32, 3, 3, 512, 8126464]),      # 4 x 2 x 8 x 31 x 4096
    ((1, 32, 2, 68, 1),     [4, 4, 32, 1, 1, 1, 2, 0]),               # rung 4: chunks of 32, L = B
    ((1, 33, 2, 128, 0),    [4, 1, 32, 2, 3, 3, 4, 131072]),          # L = B + 1; 4 x 2 x 1 x 16384
]


@pytest.mark.parametrize("args,out", ROWS, ids=["n%d_l%d_h%d_d%d_a%d" % r[0] for r in ROWS])
def test_hand_worked_rows(lib, args, out):
    rc, got = plan(lib, *args)
    assert rc == OK and got == out, (args, got, lib.t4k_last_error())


def test_rejections(lib):
    """every rejection with its code, a text, and an untouched out"""
    def refused(code, text, *a, **kw):
        rc, out = plan(lib, *a, **kw)
        assert rc == code and out == SENTINEL and text in lib.t4k_last_error(), (a, kw, rc, out, lib.t4k_last_error())
    assert plan(lib, 2, 5, 3, 8)[0] == OK
    assert lib.t4k_retention_plan(2, 5, 3, 8, 1, WS, None) == ERR_ARG
    for a in ((0, 5, 3, 8), (-1, 5, 3, 8), (2, 0, 3, 8), (2, -5, 3, 8), (2, 5, 0, 8), (2, 5, -3, 8)):
        refused(ERR_ARG, b"extent", *a)
    assert plan(lib, 2, 5, 32, 8)[0] == OK
    refused(ERR_ARG, b"heads=33", 2, 5, 33, 8)
    refused(ERR_ARG, b"ws_bytes", 2, 5, 3, 8, ws=-1)
    for d in (-4, 0, 2, 3, 6, 18, 130, 132, 256):
        refused(ERR_UNSUPPORTED, b"head size", 2, 5, 3, d)
    big = 1 << 40
    refused(ERR_UNSUPPORTED, b"2^31", 1 << 10, 1 << 10, 8, 128, ws=big)                               # 3 x 2^30
    refused(ERR_UNSUPPORTED, b"2^31", (1 << 31) - 1, (1 << 31) - 1, 32, 128, ws=big)                  # no overflow on the way to the verdict
    assert plan(lib, 1, 44739242, 1, 16, ws=big)[0] == OK                                              # 48 x 44739242 = 2^31 - 32
    refused(ERR_UNSUPPORTED, b"2^31", 1, 44739243, 1, 16, ws=big)
    assert plan(lib, 1, 1 << 20, 4, 128, ws=big) == (OK, [4, 4, 32, 32768, 3, 3, 131072, (1 << 31) - 1])   # 4 x 4 x 32767 x 16384 bytes: reported saturated
    # the workspace: the reverse states of all chunks but the last
    assert plan(lib, 2, 65, 3, 20, ws=9600)[0] == OK
    refused(ERR_UNSUPPORTED, b"workspace", 2, 65, 3, 20, ws=9599)
    assert plan(lib, 2, 64, 3, 20, ws=0)[0] == OK                                                      # one chunk needs none
