"""t4k_gemm_batched (include/t4k.h) against float64: both regimes (whole small matrices one per wave, large ones on the tile kernel with
the entry in the grid), transposed operands, alpha / beta, broadcast entries (sA / sB = 0) and channels (cA / cB = 1), 4-byte-aligned
operands, batch sizes that do not fill the last workgroup, exact integer products, beta = 0 never reading O, and graph capture."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def up(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def down(t, h):
    h.call("t4k_sync", None)
    return t.cpu().numpy()


def operand(rng, batch, rows, cols, ch, integer=False):
    """[batch, rows, cols, ch] (ch = 1 stored without a channel axis, as every rank-2 operand is)"""
    if integer:
        return rng.integers(-4, 5, size=(batch, rows, cols, ch)).astype(np.float32)
    return rng.standard_normal((batch, rows, cols, ch)).astype(np.float32)


def reference(A, B, O0, alpha, beta, tA, tB, C):
    """float64 O = alpha op(A) @ op(B) + beta O0 per entry and channel, plus |alpha| |op(A)| @ |op(B)| for the bound"""
    A = A.astype(np.float64); B = B.astype(np.float64)
    if tA:
        A = A.transpose(0, 2, 1, 3)
    if tB:
        B = B.transpose(0, 2, 1, 3)
    A = np.broadcast_to(A, A.shape[:3] + (C,)) if A.shape[3] == 1 else A
    B = np.broadcast_to(B, B.shape[:3] + (C,)) if B.shape[3] == 1 else B
    At, Bt = A.transpose(0, 3, 1, 2), B.transpose(0, 3, 1, 2)
    o = (alpha * np.matmul(At, Bt)).transpose(0, 2, 3, 1)
    m = (abs(alpha) * np.matmul(np.abs(At), np.abs(Bt))).transpose(0, 2, 3, 1)
    if beta != 0:
        o = o + beta * O0.astype(np.float64); m = m + abs(beta) * np.abs(O0.astype(np.float64))
    return o, m


def run(h, M, N, K, C=1, batch=4, tA=0, tB=0, alpha=1.0, beta=0.0, bcA=False, bcB=False, cA=None, cB=None, integer=False,
        offset=0, seed=0, nan_out=False):
    rng = np.random.default_rng(seed)
    cA = C if cA is None else cA
    cB = C if cB is None else cB
    ba, bb = (1 if bcA else batch), (1 if bcB else batch)
    A = operand(rng, ba, K if tA else M, M if tA else K, cA, integer)
    B = operand(rng, bb, N if tB else K, K if tB else N, cB, integer)
    O0 = np.full((batch, M, N, C), np.nan, np.float32) if nan_out else operand(rng, batch, M, N, C, integer)
    # `offset` floats in front of each buffer: bases that are 4-byte but not 16-byte aligned
    dA = up(np.concatenate([np.zeros(offset, np.float32), A.ravel()]))
    dB = up(np.concatenate([np.zeros(offset, np.float32), B.ravel()]))
    dO = up(np.concatenate([np.zeros(offset, np.float32), O0.ravel()]))
    sA = 0 if bcA else A[0].size
    sB = 0 if bcB else B[0].size
    pa, pb, po = (ctypes.c_void_p(t.data_ptr() + 4 * offset) for t in (dA, dB, dO))
    h.call("t4k_gemm_batched", pa, pb, po, alpha, beta, tA, tB, M, N, K, C, cA, cB, batch, sA, sB, M * N * C, None)
    got = down(dO, h)[offset:].reshape(batch, M, N, C)
    want, mag = reference(A, B, O0, alpha, beta, tA, tB, C)
    return got, want, mag


def check(got, want, mag, K):
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - want)
    bound = 2 * (K + 2) * 2.0 ** -24 * mag + 1e-30     # K products plus the alpha / beta roundings
    assert np.all(err <= bound), float(np.max(err / (mag + 1e-30)))


SMALL = [(28, 28, 28), (32, 32, 32), (20, 12, 9), (16, 16, 16), (5, 3, 7), (64, 64, 64), (33, 17, 40), (1, 64, 5), (64, 1, 3), (48, 60, 1)]


@pytest.mark.parametrize("M,N,K", SMALL)
@pytest.mark.parametrize("batch", [1, 5, 128])
def test_small_regime(t4k, M, N, K, batch):
    got, want, mag = run(t4k, M, N, K, batch=batch, seed=M * 7 + N + K)
    check(got, want, mag, K)


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (130, 70, 99), (65, 300, 64), (512, 256, 128), (100, 100, 3)])
@pytest.mark.parametrize("batch", [1, 3])
def test_large_regime(t4k, M, N, K, batch):
    got, want, mag = run(t4k, M, N, K, batch=batch, seed=K)
    check(got, want, mag, K)


@pytest.mark.parametrize("M,N,K", [(28, 20, 12), (96, 80, 64), (130, 66, 36)])
@pytest.mark.parametrize("tA,tB", [(0, 1), (1, 0), (1, 1)])
def test_transposed(t4k, M, N, K, tA, tB):
    got, want, mag = run(t4k, M, N, K, batch=3, tA=tA, tB=tB, seed=tA * 2 + tB)
    check(got, want, mag, K)


@pytest.mark.parametrize("M,N,K", [(20, 12, 9), (128, 128, 64)])
def test_alpha_beta(t4k, M, N, K):
    got, want, mag = run(t4k, M, N, K, batch=5, alpha=0.5, beta=-1.25)
    check(got, want, mag, K)


@pytest.mark.parametrize("M,N,K", [(28, 28, 28), (20, 12, 9), (128, 96, 72)])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("bc", ["A", "B"])
def test_broadcast_entry(t4k, M, N, K, C, bc):
    got, want, mag = run(t4k, M, N, K, C=C, batch=7, bcA=bc == "A", bcB=bc == "B")
    check(got, want, mag, K)


@pytest.mark.parametrize("M,N,K", [(28, 28, 28), (64, 64, 64), (20, 12, 9), (100, 90, 40)])
@pytest.mark.parametrize("cA,cB", [(1, 3), (3, 1), (1, 1), (3, 3)])
def test_channels(t4k, M, N, K, cA, cB):
    got, want, mag = run(t4k, M, N, K, C=3, batch=2, cA=cA, cB=cB)
    check(got, want, mag, K)


@pytest.mark.parametrize("M,N,K", [(28, 28, 28), (256, 128, 64), (20, 12, 9)])
def test_four_byte_aligned(t4k, M, N, K):
    got, want, mag = run(t4k, M, N, K, batch=3, offset=1)
    check(got, want, mag, K)


@pytest.mark.parametrize("M,N,K,batch", [(28, 28, 28, 128), (1024, 1024, 1024, 8)])
def test_integer_operands_exact(t4k, M, N, K, batch):
    got, want, _ = run(t4k, M, N, K, batch=batch, integer=True)
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("M,N,K,C,cA", [(28, 28, 28, 1, 1), (300, 200, 100, 1, 1), (20, 12, 9, 3, 1)])
def test_beta_zero_never_reads_output(t4k, M, N, K, C, cA):
    got, want, mag = run(t4k, M, N, K, C=C, cA=cA, batch=6, nan_out=True)
    check(got, want, mag, K)


def test_bad_arguments(t4k):
    import torch
    x = torch.zeros(64, device="cuda")
    p = P(x)
    assert t4k.lib.t4k_gemm_batched(p, p, p, 1.0, 0.0, 0, 0, 2, 2, 2, 3, 2, 3, 1, 0, 0, 12, None) != 0     # cA neither 1 nor C
    assert t4k.lib.t4k_gemm_batched(p, p, p, 1.0, 0.0, 0, 0, 2, 2, 2, 1, 1, 1, 2, 4, 4, 3, None) != 0     # overlapping outputs
    assert t4k.lib.t4k_gemm_batched(p, p, p, 1.0, 0.0, 0, 0, 2, 2, 2, 1, 1, 1, 0, 4, 4, 4, None) == 0     # empty batch: nothing to do


@pytest.mark.parametrize("M,N,K,batch", [(28, 28, 28, 128), (256, 256, 256, 4)])
def test_graph_capture_replay(t4k, M, N, K, batch):
    import torch
    rng = np.random.default_rng(11)
    A = operand(rng, batch, M, K, 1); B = operand(rng, batch, K, N, 1)
    dA, dB = up(A), up(B)
    dO = torch.zeros(batch * M * N, device="cuda"); torch.cuda.synchronize()
    eager = torch.zeros_like(dO)
    t4k.call("t4k_gemm_batched", P(dA), P(dB), P(eager), 1.0, 0.0, 0, 0, M, N, K, 1, 1, 1, batch, M * K, K * N, M * N, None)
    t4k.call("t4k_sync", None)
    s = ctypes.c_void_p(); t4k.call("t4k_stream_create", ctypes.byref(s))
    g = ctypes.c_void_p()
    t4k.call("t4k_graph_begin", s)
    t4k.call("t4k_gemm_batched", P(dA), P(dB), P(dO), 1.0, 0.0, 0, 0, M, N, K, 1, 1, 1, batch, M * K, K * N, M * N, s)
    t4k.call("t4k_graph_end", s, ctypes.byref(g))
    assert not dO.abs().sum().item()                     # captured, not run
    t4k.call("t4k_graph_launch", g, s); t4k.call("t4k_graph_launch", g, s)
    t4k.call("t4k_sync", s)
    assert torch.equal(dO, eager)
    t4k.call("t4k_graph_destroy", g); t4k.call("t4k_stream_destroy", s)
    want, mag = reference(A, B, None, 1.0, 0.0, 0, 0, 1)
    check(eager.cpu().numpy().reshape(batch, M, N, 1), want, mag, K)


def test_one_launch_per_call(t4k):
    """the library counts its launches (t4k_launch_count): one per call in both regimes, whatever batch and C are"""
    import torch
    x = torch.zeros(3 * 300 * 300 * 8, device="cuda"); torch.cuda.synchronize()
    p = P(x)
    for M, N, K, C, cA, batch in [(28, 28, 28, 1, 1, 8), (20, 12, 9, 3, 1, 7), (300, 200, 100, 1, 1, 4), (130, 66, 36, 3, 3, 2)]:
        before = t4k.lib.t4k_launch_count()
        t4k.call("t4k_gemm_batched", p, p, p, 1.0, 0.0, 0, 0, M, N, K, C, cA, C, batch, 0, 0, M * N * C, None)
        assert t4k.lib.t4k_launch_count() - before == 1
    t4k.call("t4k_sync", None)
