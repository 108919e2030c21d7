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
RUN_MAX_GRID = 8192                         # fused.hip: t4k_poolblock_fwd / _bwd cap their grid here
RUN_WAVE64_BELOW = BLK * 2                  # ... and take 64-thread workgroups below BLK * 2 threads per CU (512 x cu_count threads)
RUN_CU = 256                                # the MI355X's CU count: the table below is sized for it
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


# ----------------------------------------------------------------------------- pool and fused element-wise runs (pool.hip, fused.hip)
def ceil_div(a, b):
    return -(-a // b)


def run_vw(C, *ptrs):
    """fused.hip vec_width: the widest of 4 / 2 / 1 channels per thread that divides C with EVERY tensor's base address a multiple of
    4 * VW bytes (t4k_poolblock_bwd falls straight to 1 for a misaligned DY, the BN form for XH / O: see run_vw_bwd / run_vw_bn)"""
    for vw in (4, 2):
        if C % vw == 0 and all(q % (4 * vw) == 0 for q in ptrs):
            return vw
    return 1


def run_vw_tail(vw, *ptrs):
    """the second step of the backward (DY) and of the BN form (XH, O): a misaligned one of these drops the run to scalar at once"""
    return vw if all(q % (4 * vw) == 0 for q in ptrs) else 1


def run_plan(nthr, cu=RUN_CU):
    """(workgroup size, grid, grid-stride trips of the longest thread, threads at work in the last trip) of a fused run of nthr threads"""
    bs = 64 if nthr < RUN_WAVE64_BELOW * cu else BLK
    grid = min(ceil_div(nthr, bs), RUN_MAX_GRID)
    trips = ceil_div(nthr, grid * bs)
    return bs, grid, trips, nthr - (trips - 1) * grid * bs


def run_label(nthr, cu=RUN_CU):
    bs, grid, trips, _ = run_plan(nthr, cu)
    return "wave64" if bs == 64 and trips == 1 else "wg256" if bs == BLK and trips == 1 else "wg256_wrap" if bs == BLK else "wave64_wrap"


def pool_plan(n):
    """(grid, trips, threads at work in the last trip) of k_pool / k_dpool over n outputs: grid_for(n)"""
    grid = min(ceil_div(n, BLK), MAX_WG)
    trips = ceil_div(n, grid * BLK)
    return grid, trips, n - (trips - 1) * grid * BLK


class RunCase:
    """one fused run: N images, pooled grid H0 x W0 (input grid H0 * KS x W0 * KS), C channels; `plan` / `vw` = what it is meant to hit"""

    def __init__(self, plan, vw, N, H0, W0, C, KS, pool, why):
        self.plan, self.vw, self.N, self.H0, self.W0, self.C, self.KS, self.pool, self.why = plan, vw, N, H0, W0, C, KS, pool, why
        self.H1, self.W1 = H0 * KS, W0 * KS
        self.nthr = N * H0 * W0 * C // vw
        self.id = "%s-vw%d-N%d-%dx%d-C%d-KS%d" % (plan, vw, N, H0, W0, C, KS)


RUN_CASES = (
    RunCase("wave64", 4, 8, 32, 32, 60, 2, "max", "last 64-thread plan: 122 880 threads"),
    RunCase("wg256", 4, 8, 32, 32, 64, 2, "max", "first 256-thread plan: 131 072 threads"),
    RunCase("wave64", 2, 8, 32, 32, 30, 2, "max", "the same boundary at two channels per thread: 122 880"),
    RunCase("wg256", 2, 8, 32, 32, 34, 2, "max", "... 139 264"),
    RunCase("wave64", 1, 8, 32, 32, 15, 2, "max", "the same boundary at one channel per thread: 122 880"),
    RunCase("wg256", 1, 8, 32, 32, 17, 2, "max", "... 139 264"),
    RunCase("wg256_wrap", 1, 4, 64, 64, 129, 2, "max", "second grid-stride trip, ragged: 2 113 536 threads, 16 384 of them in trip two"),
    RunCase("wg256_wrap", 1, 8, 64, 64, 65, 1, None, "the same without a pool: 2 129 920 threads, 32 768 in trip two"),
)
RUN_WRAP_THREADS = RUN_MAX_GRID * BLK       # 2 097 152: a run strides above

# plain k_pool / k_dpool past MAX_WG workgroups with a clipped last window: N, H1, W1, C, KS (ceil grid)
POOL_WRAP_CASES = ((3, 75, 75, 123, 2), (3, 113, 113, 123, 3))       # 3 x 38 x 38 x 123 = 532 836 outputs > 524 288 (8 548 in trip two)

# the narrow-vector fallbacks at C = 8: a tensor that sits `off` bytes into its allocation -> the width the run must take
RUN_TENSORS = ("X", "pre_mask", "pre_out", "pool_out", "post_mask", "post_out", "copy_out")
RUN_MISALIGNED = tuple(("misaligned_%s" % t, t, off, vw) for t in RUN_TENSORS for off, vw in ((4, 1), (8, 2))) + \
    tuple(("misaligned_%s" % t, t, off, 1) for t in ("DY", "XH", "O") for off in (4, 8))      # the second step drops to scalar, never to 2


# ----------------------------------------------------------------------------- t4k_math over its whole domain (tests/test_gpu_math_domain.py)
F32_MAX = np.finfo(np.float32).max
F32_MIN = np.finfo(np.float32).tiny                     # the smallest normal
SUB_MAX = np.nextafter(F32_MIN, np.float32(0))          # the largest subnormal
SUB_MIN = np.float32(1.4e-45)                           # the smallest
MATH_N = 8191                                           # n % 4 == 3: the last three elements are k_math's scalar tail behind 2047 float4s
MATH_SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, SUB_MIN, SUB_MAX, F32_MIN, F32_MAX, -F32_MAX, 1.0, -1.0], np.float32)
MATH_SPECIALS_ROW = np.concatenate([MATH_SPECIALS, MATH_SPECIALS[:3]])          # 15 = 3 float4s and a tail of NaN, +inf, -inf
MATH_V = (1.5, -0.0, 2.0 ** -100)                       # the scalar operand of FILL / SCALE / ADD / SUB / MUL / DIV
POW_V = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 7.0, -1.0, -2.5)
POW_NEG_V, POW_ZERO_V = (2.0, 3.0, -1.0, 0.5), (0.0, 2.0, -1.0)   # exponents that also meet negative bases (sign; 0.5: NaN) / a zero base
GFILL_CASES = ((1, 1.5), (3, 1.5), (1025, 1.5), (2 ** 24 - 1, 1.5), (2 ** 24 + 7, 1.5), (1025, -0.3))   # (n, v): float(j) repeats past 2^24
ACT_DOMAIN_KINDS = (("relu", 0.0), ("tanh", 0.0), ("sigmoid", 0.0), ("selu", 0.0), ("leaky", 0.01), ("elu", 1.0))


def _f32(*v):
    return np.array(v, np.float32)


def _uni(lo, hi):
    return lambda rng, k: rng.uniform(lo, hi, k)


def _logu(lo, hi, signed=False):
    """10^uniform(log10 lo, log10 hi), with a random sign if asked"""
    return lambda rng, k: 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), k) * (rng.choice((-1.0, 1.0), k) if signed else 1.0)


def _table(seed, edges, tail, *parts, true=None):
    """MATH_N fp32 values: the edge values first (in the float4 body), the random parts in equal shares, three of the edges again as the last
    three elements (the scalar tail).  `true` = the op in float64: an element whose exact result lies within 1 % of FLT_MAX, where an honest
    rounding may or may not overflow, is replaced by 1."""
    rng = np.random.default_rng(seed); edges = np.asarray(edges, np.float32); tail = np.asarray(tail, np.float32)
    assert tail.size == 3 and all(np.any((edges == t) | (np.isnan(edges) & np.isnan(t))) for t in tail), "the tail repeats edge values"
    fill = MATH_N - 3 - edges.size; share = [fill // len(parts)] * len(parts); share[-1] += fill - sum(share)
    x = np.concatenate([edges] + [np.asarray(f(rng, k)) for f, k in zip(parts, share)] + [tail]).astype(np.float32)
    if true is not None:
        with np.errstate(all="ignore"):
            t = np.abs(true(x.astype(np.float64)))
        x[(t >= 0.98 * float(F32_MAX)) & (t <= 1.02 * float(F32_MAX))] = 1.0
    assert x.size == MATH_N and MATH_N % 4 == 3
    return x


class MathCase:
    """one table: op name, scalar operand v, operands x (GFILL: None, n elements are generated by the op itself)"""

    def __init__(self, op, v, x, n=None, tag=""):
        self.op, self.v, self.x, self.n = op, float(v), x, (x.size if n is None else n)
        self.id = op + (tag and "-" + tag)


def _math_domain():
    cases = []
    cases.append(MathCase("EXP", 0.0, _table(80, _f32(-104, -103.97, -87.4, -87.3, -1e-30, 0, 1e-30, 88.5, 89, 100, 3e38), _f32(-87.4, 88.5, 100),
                                             _uni(-104.0, 88.5))))
    ln_edges = _f32(np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)), 1, 1e-12,
                    np.nextafter(np.float32(1e-12), np.float32(1)), np.nextafter(np.float32(1e-12), np.float32(0)), F32_MAX,
                    1e-20, 1e-40, 0.0, -0.0, -1, -F32_MAX)
    for k, op in enumerate(("LN", "LOG")):
        cases.append(MathCase(op, 0.0, _table(81 + k, ln_edges, ln_edges[[1, 5, 11]], _logu(1e-12, 3e38), lambda rng, n: 1.0 + rng.uniform(-1e-3, 1e-3, n))))
    cases.append(MathCase("TANH", 0.0, _table(83, _f32(9.01, -9.01, 20, -20, 0.0, -0.0), _f32(-9.01, 20, -0.0), _uni(-12.0, 12.0), _logu(1e-38, 1e-2, True))))
    cases.append(MathCase("SIGM", 0.0, _table(84, _f32(88.7, -88.7, 89, -89), _f32(-88.7, 89, -89), _uni(-104.0, 104.0))))
    cases.append(MathCase("SQRT", 0.0, _table(85, _f32(-0.0, -F32_MAX, 0.0, SUB_MIN, SUB_MAX, F32_MIN, F32_MAX, -1, -1e-40), _f32(-0.0, -F32_MAX, SUB_MIN),
                                              _logu(1e-45, 3e38), _logu(1e-45, 3e38), _logu(1e-45, 3e38), lambda rng, n: -_logu(1e-45, 3e38)(rng, n))))
    cases.append(MathCase("RCP", 0.0, _table(86, _f32(0.0, -0.0, SUB_MIN, -SUB_MAX, F32_MAX, -3e38, 1, -1), _f32(0.0, -0.0, SUB_MIN),
                                             _logu(1e-45, 3e38, True), true=lambda x: 1.0 / x)))
    # single IEEE operations: normal-scale values, subnormals, and magnitudes whose product / quotient with v goes subnormal or overflows
    # (v = 1.5: 3e38 x 1.5 overflows, 1e-38 / 1.5 is subnormal; v = 2^-100: 1e-8 x v is subnormal, 1e9 / v overflows; v = -0: x / v = -+inf, 0 / v = NaN)
    ew_edges = _f32(0.0, -0.0, SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, F32_MIN, -F32_MIN, 3e38, -3e38, 1e-39, -1e-39, 1e-8, -1e-8, 1e9, -1e9, 1e-38, 1.5e-38,
                    1, -1, 0.5, 2.5e38)
    for k, op in enumerate(("ABS", "NEG", "RELU", "SAT")):
        cases.append(MathCase(op, 0.0, _table(87 + k, ew_edges, _f32(-0.0, -SUB_MAX, 3e38), lambda rng, n: rng.standard_normal(n) * 3.0, _logu(1e-45, 3e38, True))))
    for k, op in enumerate(("FILL", "SCALE", "ADD", "SUB", "MUL", "DIV")):
        for q, v in enumerate(MATH_V):
            vd = float(np.float32(v))
            true = {"FILL": lambda x: x * 0 + vd, "ADD": lambda x: x + vd, "SUB": lambda x: x - vd, "DIV": lambda x: x / vd}.get(op, lambda x: x * vd)
            cases.append(MathCase(op, v, _table(100 + 3 * k + q, ew_edges, _f32(-0.0, -SUB_MAX, 3e38), lambda rng, n: rng.standard_normal(n) * 3.0,
                                                _logu(1e-45, 3e38, True), true=true), tag="v%g" % v))
    # bases whose 7th power and whose -2.5th power overflow and underflow, in every table
    pow_edges = _f32(1e-17, 1e-16, 2e-6, 5e5, 1e6, 1e16, 1e17, 1)
    for q, v in enumerate(POW_V):
        edges = np.concatenate([pow_edges, _f32(0.0) if v in POW_ZERO_V else _f32()])
        parts = [_logu(1e-6, 1e6)] * (3 if v in POW_NEG_V else 1) + ([lambda rng, n: -_logu(1e-6, 1e6)(rng, n)] if v in POW_NEG_V else [])
        cases.append(MathCase("POW", v, _table(120 + q, edges, _f32(1e-17, 1e17, 5e5), *parts, true=lambda x, v=v: np.power(x, v)), tag="v%g" % v))
    # the fp32 neighbours of k pi / 2, k = 0 .. 8 (k = 0: 0 and the smallest subnormals)
    hp = np.array([np.float32(k * np.pi / 2) for k in range(9)], np.float32)
    near = np.concatenate([hp, np.nextafter(hp, np.float32(100)), np.nextafter(hp, np.float32(-100))])
    for k, op in enumerate(("SIN", "COS")):
        cases.append(MathCase(op, 0.0, _table(130 + k, near, near[[1, 2, 12]], _uni(-8.0, 8.0), _uni(-1e3, 1e3), _uni(-1e5, 1e5), _uni(-1e8, 1e8), _uni(-3e38, 3e38),
                                              _logu(1e-38, 1e-3, True))))
    for n, v in GFILL_CASES:
        cases.append(MathCase("GFILL", v, None, n=n, tag="n%d-v%g" % (n, v)))
    return tuple(cases)


MATH_DOMAIN = _math_domain()
ACT_DOMAIN = np.concatenate([np.linspace(-104.0, 104.0, MATH_N - 3).astype(np.float32), _f32(-104, 88.7, -0.0)])   # k_activate: the rows today stop near |x| = 15
