"""Shapes and inputs of the small-kernel sweep, shared by the GPU sweep (tests/test_gpu_small_kernels_sweep.py) and the CPU self-test of its
witnesses (tests/test_f64_witness.py): the CPU test runs the oracle through every shape listed here, so the inputs are known to keep an
honest fp32 implementation inside each bound before a GPU sees them.

The sizes come from the launchers' thresholds - tensorforth_amd/csrc/t4k_common.h (BLK, MAX_WG, grid_for) and reduce.hip (RED_MAX_PARTS,
launch_reduce's 16 elements per lane, the batch-norm chunking).  A change there must be followed here."""
import numpy as np

BLK = 256                                   # t4k_common.h: workgroup size
MAX_WG = 2048                               # t4k_common.h: grid_for() strides above MAX_WG workgroups
RED_MAX_PARTS = 1024                        # reduce.hip: launch_reduce caps its grid here
RED_PER_BLOCK = BLK * 16                    # reduce.hip: launch_reduce gives a workgroup 4096 elements -> 1 launch up to here, 2 above
RED_STRIDE_N = RED_MAX_PARTS * RED_PER_BLOCK    # 4 194 304: k_reduce1 takes a second grid-stride trip above
GRID4_STRIDE_N = MAX_WG * BLK * 4           # 2 097 152: grid_for(n, 4) (k_math / k_ts / k_tt / k_copy / k_activate) strides above
GRID1_STRIDE_N = MAX_WG * BLK               # 524 288: grid_for(n) (optimizers, k_bias, k_copy_mask, k_bn_apply) strides above
BN_CHUNKED_ROWS = 2048                      # reduce.hip bn_fwd_stats: one-launch statistics below, chunked column sums from here
BN_CHUNK_ROWS, BN_MAX_CHUNKS = 256, 2048    # ... in chunks of >= 256 rows, at most 2048 of them (N*HW > 524 288 grows the chunk)

RED_N = (1, 3, 255, 256, 257, 4095, 4096, 4097, 65539, RED_STRIDE_N, RED_STRIDE_N + 1, 5000003)
RED_OFFSETS = (0, 1, 4)                     # base pointer offsets in elements: 16-byte aligned, 4-byte aligned (scalar path), 16 again
RED_FLOAT_N = (1, 3, 255, 256, 257, 4095, 4096, 4097, 65539)
DOT_K, DOT_C, DOT_AB = (1, 255, 256, 257, 5000), (1, 3, 64, 300), ((1.0, 0.0), (2.0, -1.0))
DB_E0, DB_N = (1, 63, 64, 65, 130), (1, 3, 4, 5, 257)
SOFTMAX_C, SOFTMAX_N = (1, 2, 63, 64, 65, 300, 1000), (1, 3, 4, 5, 257)
LOGSOFTMAX_NC = ((255, 10), (256, 63), (257, 64), (5, 1000), (1, 1), (300, 65))
BN_SHAPES = ((2047, 5), (2048, 4), (2049, 4), (2049, 70), (4099, 64), (4099, 65), (10007, 1), (10007, 3), (540672, 4), (392, 130))
BN_SYNC_SHAPES = ((2049, 70), (4099, 64))
BN_MEANS = (0.0, 1.0, 8.0)                  # input mean in units of sigma
BN_MEAN_SHAPES = ((2047, 5), (4099, 64), (10007, 3))
EW_N = (1, 3, 1023, 1025, GRID4_STRIDE_N, GRID4_STRIDE_N + 3, 3000001)
TRANSPOSE_HWC = ((63, 65, 1), (129, 64, 2), (1, 1, 1))
OPT_N = (1, 255, 1024, 1025, GRID1_STRIDE_N, GRID1_STRIDE_N + 1, 1200001)
OPT_CHUNKED_SIZES = (1, 1023, 1024, 1025, 3000)
OPT_MULTI_SIZES = (7, 70001, 1024, 65537)
LINALG_K = (1, 2, 5, 255, 256, 257, 300)
LINALG_KINDS = ("dominant", "permuted", "cond1e4")
DCONV_SHAPES = ((6, 4, 4, 12, 8), (2, 7, 7, 3, 4), (4, 8, 8, 64, 32), (3, 16, 16, 8, 1), (2, 5, 5, 32, 64), (2, 5, 8, 6, 3), (1, 9, 6, 16, 3))   # N, H1, W1, C1, C0


def bn_split(rows):
    """(N, HW) of a row count: the oracle and the kernels see the same [N*HW, C] matrix"""
    for n in (132, 8):
        if rows % n == 0:
            return n, rows // n
    return 1, rows


def bn_plan(rows):
    """(chunks, rows per chunk) of the chunked statistics, as reduce.hip computes them"""
    nch = min((rows + BN_CHUNK_ROWS - 1) // BN_CHUNK_ROWS, BN_MAX_CHUNKS)
    rpc = (rows + nch - 1) // nch
    return (rows + rpc - 1) // rpc, rpc


def ints(rng, shape, lo=1, hi=3):
    """small non-zero integers in +-[lo, hi] as fp32: every fp32 partial sum of fewer than 2^24 / hi of them is exact in any order"""
    return (rng.integers(lo, hi + 1, shape) * rng.choice((-1, 1), shape)).astype(np.float32)


def floats(rng, n, kind):
    """standard normal, or the badly scaled mix 1e4 a + b"""
    a = rng.standard_normal(n)
    return (a if kind == "normal" else 1e4 * a * (rng.random(n) < 0.01) + rng.standard_normal(n)).astype(np.float32)


def bn_input(rng, rows, C, mean):
    return (rng.standard_normal((rows, C)) * 2.0 + 2.0 * mean).astype(np.float32)


def matrix(rng, K, kind):
    """dominant: random + K^(1/2)-weighted diagonal (no swaps needed); permuted: the same with rows rotated so every column swaps;
    cond1e4: orthogonal x diag(1 .. 1e-4) x orthogonal; singular_last / singular_first: a zero last / first column"""
    if kind in ("dominant", "permuted", "singular_last", "singular_first"):
        A = rng.standard_normal((K, K)) + np.eye(K) * (2.0 + 3.0 * np.sqrt(K))
        if kind == "permuted":
            A = np.roll(A, 1, axis=0)
        if kind == "singular_last":
            A[:, K - 1] = 0.0
        if kind == "singular_first":
            A[:, 0] = 0.0
        return A.astype(np.float32)
    q1, _ = np.linalg.qr(rng.standard_normal((K, K))); q2, _ = np.linalg.qr(rng.standard_normal((K, K)))
    return (q1 @ np.diag(np.logspace(0, -4, K)) @ q2).astype(np.float32)


def softmax_rows(rng, N, C):
    """rows of scale 4, then (cyclically) a row with one logit 80 above the rest, an all-equal row, a row at -80"""
    Z = (rng.standard_normal((N, C)) * 4.0).astype(np.float32)
    if N > 1:
        Z[1 % N, rng.integers(0, C)] += 80.0
    if N > 2:
        Z[2] = 1.25
    if N > 3:
        Z[3] = -80.0
    return Z
