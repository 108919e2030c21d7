"""GPU: every kernel that draws from the Philox stream, far out in the stream, against an independent numpy generator (philox_witness.py).

The rest of the suite holds the drawing kernels to the oracle bit for bit, but only at seeds <= 4321 and offsets <= 2^22, where the high key word
(seed >> 32) and the high counter word (counter >> 32) are both zero: a kernel, a repacked host struct or the device-resident copy used under graph
capture that narrows either to 32 bits passes all of it.  Here each entry runs at the positions of philox_witness.POSITIONS (offsets in elements,
nq = ceil(n / 4) of the entry's FIRST draw):

    P0  seed 777                  offset 0                    control
    P1  seed 0x9E3779B97F4A7C15   offset 2^34 - 4 (nq // 2)   the draw straddles the carry into the high counter word; high key word set
    P2  seed 0xFFFFFFFF00000001   offset 2^36 + 48            high counter word 16 throughout
    P3  seed 1 << 32              offset 4096                 only the high key word set
    P4  seed 5                    offset 2^64 - 4 (nq // 2)   the element offset wraps mod 2^64 inside the draw (counter 2^62: a carry into the high word)

and every case asserts: each mask written == the witness's (np.array_equal; a second dropout stage starts 4 ceil(n1 / 4) elements behind the
first), t4k_rand_offset() == the expected end, and every output element of the dropout layer is its input or 0 as the witness's mask says.
tests/test_philox_witness.py shows on the CPU that a generator without the high counter word, the high key word or the carry between the
counter words draws another mask at P1 / P2 (and which of P3 / P4 see which).  alpha = 0.5 throughout.

Every `rng_draw(` call site of csrc/ and the case that reaches it (a site without a case would be a gap):

    optim.hip:384    t4k_rand                                         test_rand_uniform_and_dropout_mask_entries, test_normal_draws_*, captured
    optim.hip:377    t4k_dropout_mask                                 test_rand_uniform_and_dropout_mask_entries, test_sharded_dropout_mask_entry, captured;
                                                                      and behind an unsplit GEMM: test_linear_with_dropout[1024-1024-64]
    fused.hip:226    t4k_poolblock_fwd, dropout pre-stage             test_poolblock_run[pre-*], test_sharded_poolblock_run, captured
    fused.hip:227    t4k_poolblock_fwd, dropout post-stage            test_poolblock_run[post-*]
    conv.hip:538     t4k_conv2d_block_fwd, dropout pre-stage          test_conv_block_with_dropout (quad-shared block: 4-8-6-40 and 8-14-10-20; per element: 3-6-5-7), captured
    gemm.hip:965     first stage of a GEMM's riders (ep1)             split-K fold: test_linear_with_dropout[128-100-980], [256-128-1024]; gemm_l32.h epilogue: test_linear_block_run[64-300-128-drop-tanh]
    gemm.hip:968     second stage of a GEMM's riders (ep2)            gemm_l32.h epilogue: test_linear_block_run[256-512-256-leaky-drop]; split-K fold: test_linear_block_run[256-1024-128-leaky-drop]
    linear.hip:159   t4k_linear_act_fwd, head-sized layer             test_linear_with_dropout[64-16-40] (k_linsmall_fwd), [33-3-17] (k_linthin_fwd)
    linear.hip:196   t4k_linear_block_fwd, head-sized, lone stage     test_linear_block_run[128-320-10-drop]
    linear.hip:226   t4k_mlp_head_fwd, the head folds the slabs       test_mlp_head_with_dropout
    conv_stack.hip:546 / 547   t4k_conv_stack_fwd pre / post stage    test_conv_stack_with_dropout_stages (post-stage in stage 0, pre-stage in stage 2)
    conv_stack.hip:598 / 599   t4k_conv_stack_head_fwd pre / post     test_conv_stack_head_with_dropout[odd] (both), [lenet] (pre)
    conv_stack.hip:607         t4k_conv_stack_head_fwd mid-dropout    test_conv_stack_head_with_dropout[odd], [lenet]

The conv-stack kernels carry their own copy of the generator and repacked (base, base2, seed) arguments; they refuse graph capture
(t4k_conv_stack_ok == 0 while capturing), so only the four captured entries below reach the device-resident copy of the stream."""
import ctypes

import numpy as np
import pytest

import philox_witness as pw
from test_gpu_conv_stack import CASES, StackHead, _build, _params
from test_gpu_parity import Dev, PoolBlock, p

pytestmark = pytest.mark.gpu
ALPHA = 0.5
NAMES = ("P0", "P1", "P2", "P3", "P4")


@pytest.fixture(scope="module")
def dev(t4k):
    return Dev(t4k)


@pytest.fixture(autouse=True)
def unsharded(t4k):
    """every test leaves the stream unsharded, whatever happens in it"""
    try:
        yield
    finally:
        t4k.call("t4k_rand_set_shard", 0, 1)


def _set(t4k, seed, off):
    """(seed, offset) immediately before the call under test; `off` may be an unwrapped position >= 2^64"""
    t4k.call("t4k_rand_init", seed); t4k.call("t4k_rand_set_offset", off % 2 ** 64)


def _launches(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return int(t4k.lib.t4k_launch_count())


def _nq(n):
    return (n + 3) // 4


def _check_dropout(what, mask_got, out_got, inp, seed, off, n):
    """the stored mask is the witness's, and the layer's output is its input or 0 accordingly"""
    want = pw.mask(seed, off, n, ALPHA)
    m = np.asarray(mask_got).reshape(-1)
    assert np.array_equal(m, want), "%s: mask differs from the witness in %d of %d elements" % (what, int(np.sum(m != want)), n)
    assert np.array_equal(np.asarray(out_got).reshape(-1), np.where(want > 0, np.asarray(inp).reshape(-1), np.float32(0))), what + ": output"


# ------------------------------------------------------------------------------------------- t4k_rand / t4k_dropout_mask
@pytest.mark.parametrize("n", [1, 5, 4099, 2098179])       # the last: k_rand's grid-stride loop takes a second trip (nq > 2048 x 256)
@pytest.mark.parametrize("name", NAMES)
def test_rand_uniform_and_dropout_mask_entries(t4k, dev, name, n):
    seed, off = pw.position(name, n)
    u = pw.uniform(seed, off, n)
    u2 = pw.uniform(seed, off + 4 * _nq(n), n)                    # the mask entry draws right behind
    bias, scale = np.float32(-0.5), np.float32(0.2)
    for shift in (0, 1):                                         # 16-byte aligned base, and one 4 bytes further
        a, m = dev.zeros(n + 4), dev.zeros(n + 4)
        _set(t4k, seed, off)
        t4k.call("t4k_rand", p(a) + 4 * shift, n, 0, -0.5, 0.2, None)
        assert t4k.lib.t4k_rand_offset() == pw.end_offset(off, n)
        t4k.call("t4k_dropout_mask", p(m) + 4 * shift, n, None)
        assert t4k.lib.t4k_rand_offset() == pw.end_offset(off + 4 * _nq(n), n)
        ga, gm = dev.down(a), dev.down(m)
        assert np.array_equal(ga[shift:shift + n], scale * (bias + u)), "uniform, shift %d" % shift     # two fp32 roundings, as the kernel's
        assert np.array_equal(gm[shift:shift + n], u2), "mask entry, shift %d" % shift
        assert np.array_equal((gm[shift:shift + n] > np.float32(ALPHA)).astype(np.float32), pw.mask(seed, off + 4 * _nq(n), n, ALPHA))
        assert not ga[:shift].any() and not ga[shift + n:].any() and not gm[:shift].any() and not gm[shift + n:].any()   # nothing outside


def test_offsets_are_rounded_down_to_a_whole_counter(t4k, dev):
    """include/t4k.h: the remainder of an offset that is no multiple of 4 is dropped, not remembered"""
    seed, base, n = pw.SEED_P2, 2 ** 36 + 48, 9
    for rem in (0, 1, 2, 3):
        _set(t4k, seed, base + rem)
        assert t4k.lib.t4k_rand_offset() == base, rem
        a = dev.zeros(n); t4k.call("t4k_rand", p(a), n, 0, 0.0, 1.0, None)
        assert np.array_equal(dev.down(a), pw.uniform(seed, base, n)), rem
        assert t4k.lib.t4k_rand_offset() == base + 12 == pw.end_offset(base + rem, n), rem


# ------------------------------------------------------------------------------------------- shards
def _shard_offset(where, nq, world):
    """P1 with the carry into the high counter word BETWEEN two ranks' slices (behind the last but one rank's) or INSIDE a rank's slice (rank 1's); P2"""
    if where == "P1-between":
        return pw.SEED_P1, 2 ** 34 - 4 * nq * (world - 1)
    if where == "P1-inside":
        return pw.SEED_P1, 2 ** 34 - 4 * nq - 4 * (nq // 2)
    return pw.position("P2", 4 * nq)


@pytest.mark.parametrize("where", ["P1-between", "P1-inside", "P2"])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_dropout_mask_entry(t4k, dev, world, where):
    n = 4099; nq = _nq(n)
    seed, off = _shard_offset(where, nq, world)
    for r in range(world):
        m = dev.zeros(n)
        t4k.call("t4k_rand_set_shard", r, world); _set(t4k, seed, off)
        t4k.call("t4k_dropout_mask", p(m), n, None)
        assert t4k.lib.t4k_rand_offset() == off + 4 * world * nq == pw.end_offset(off, n, world), "rank %d" % r
        assert np.array_equal(dev.down(m), pw.uniform(seed, off + r * 4 * nq, n)), "rank %d" % r


def _poolblock(t4k, dev, oracle, X, kind, C):
    """one fused run on X [N, H1, H1, C]: kind "pre" = dropout, max, relu; "post" = leaky, max, dropout.  Returns host copies of its tensors."""
    N, H1 = X.shape[0], X.shape[1]; H0 = H1 // 2
    d = {"pre_mask": dev.zeros(X.shape), "pre_out": dev.zeros(X.shape), "pool_out": dev.zeros((N, H0, H0, C)),
         "post_mask": dev.zeros((N, H0, H0, C)), "post_out": dev.zeros((N, H0, H0, C))}
    blk = PoolBlock(); blk.KS = 2; blk.pool_layer = oracle.L_MAXPOOL; blk.pool_out = p(d["pool_out"])
    blk.pre_mask, blk.pre_out, blk.post_mask, blk.post_out = p(d["pre_mask"]), p(d["pre_out"]), p(d["post_mask"]), p(d["post_out"])
    if kind == "pre":
        blk.pre_layer, blk.pre_alpha, blk.post_layer, blk.post_alpha = oracle.L_DROPOUT, ALPHA, oracle.L_RELU, 0.0
    else:
        blk.pre_layer, blk.pre_alpha, blk.post_layer, blk.post_alpha = oracle.L_LEAKYRL, 0.2, oracle.L_DROPOUT, ALPHA
    t4k.call("t4k_poolblock_fwd", p(dev.up(X)), ctypes.byref(blk), N, H1, H1, H0, H0, C, None)
    return {k: dev.down(v) for k, v in d.items()}


@pytest.mark.parametrize("where", ["P1-between", "P1-inside", "P2"])
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_poolblock_run(t4k, dev, oracle, world, where):
    N, H1, C = 3, 14, 8
    n = N * H1 * H1 * C; nq = _nq(n)
    seed, off = _shard_offset(where, nq, world)
    X = np.random.default_rng(world).standard_normal((world, N, H1, H1, C)).astype(np.float32)
    for r in range(world):
        t4k.call("t4k_rand_set_shard", r, world); _set(t4k, seed, off)
        got = _poolblock(t4k, dev, oracle, X[r], "pre", C)
        assert t4k.lib.t4k_rand_offset() == off + 4 * world * nq, "rank %d" % r
        _check_dropout("rank %d of %d" % (r, world), got["pre_mask"], got["pre_out"], X[r], seed, off + r * 4 * nq, n)


# ------------------------------------------------------------------------------------------- fused element-wise run
@pytest.mark.parametrize("C", [5, 6, 8])                  # scalar, 8-byte and 16-byte channel vectors
@pytest.mark.parametrize("kind,H1", [("pre", 14), ("post", 12)])
@pytest.mark.parametrize("name", NAMES)
def test_poolblock_run(t4k, dev, oracle, name, kind, H1, C):
    N = 3; H0 = H1 // 2
    n = N * H1 * H1 * C if kind == "pre" else N * H0 * H0 * C
    seed, off = pw.position(name, n)
    X = np.random.default_rng(C + H1).standard_normal((N, H1, H1, C)).astype(np.float32)
    _set(t4k, seed, off)
    got = _poolblock(t4k, dev, oracle, X, kind, C)
    assert t4k.lib.t4k_rand_offset() == pw.end_offset(off, n)
    if kind == "pre":
        _check_dropout("pre-stage", got["pre_mask"], got["pre_out"], X, seed, off, n)
    else:
        _check_dropout("post-stage", got["post_mask"], got["post_out"], got["pool_out"], seed, off, n)


# ------------------------------------------------------------------------------------------- conv epilogue
def _conv_block_bufs(dev, N, H, C1, C0):
    rng = np.random.default_rng(C0)
    return {"X": dev.up(rng.standard_normal((N, H, H, C1)).astype(np.float32)), "F": dev.up((rng.standard_normal((C1, 3, 3, C0)) * 0.3).astype(np.float32)),
            "B": dev.up(rng.standard_normal(C0).astype(np.float32)), "Y": dev.zeros((N, H, H, C0)), "pre_mask": dev.zeros((N, H, H, C0)),
            "pre_out": dev.zeros((N, H, H, C0)), "pool_out": dev.zeros((N, H // 2, H // 2, C0))}


def _conv_block(t4k, oracle, b, N, H, C1, C0, stream=None):
    """conv 3x3 + dropout + max pool in one call, on buffers made beforehand (so that the call can be captured)"""
    blk = PoolBlock(); blk.KS = 2; blk.pool_layer = oracle.L_MAXPOOL; blk.pool_out = p(b["pool_out"])
    blk.pre_layer, blk.pre_alpha = oracle.L_DROPOUT, ALPHA; blk.pre_mask = p(b["pre_mask"]); blk.pre_out = p(b["pre_out"])
    t4k.call("t4k_conv2d_block_fwd", p(b["X"]), None, p(b["Y"]), p(b["F"]), p(b["B"]), ctypes.byref(blk), N, H, H, C1, H, H, C0, 3, 1, 1, stream)


@pytest.mark.parametrize("N,H,C1,C0", [(4, 8, 6, 40), (3, 6, 5, 7), (8, 14, 10, 20)])    # quad-shared block, two channel tiles; per-element path; LeNet conv2
@pytest.mark.parametrize("name", NAMES)
def test_conv_block_with_dropout(t4k, dev, oracle, name, N, H, C1, C0):
    n = N * H * H * C0
    seed, off = pw.position(name, n)
    b = _conv_block_bufs(dev, N, H, C1, C0)
    _set(t4k, seed, off)
    _conv_block(t4k, oracle, b, N, H, C1, C0)
    assert t4k.lib.t4k_rand_offset() == pw.end_offset(off, n)
    _check_dropout("conv epilogue", dev.down(b["pre_mask"]), dev.down(b["pre_out"]), dev.down(b["Y"]), seed, off, n)


# ------------------------------------------------------------------------------------------- linear layers
# launches: 1 = the head-sized kernels (k_linsmall_fwd / k_linthin_fwd) or the 32x32-sliver GEMM with the run in its epilogue; 2 = split-K GEMM + the
# fold that carries the run (K > 832 keeps a sliver off the 32x32 kernel); 3 = unsplit GEMM (its 256 tiles fill the chip), t4k_dropout_mask, t4k_activate
@pytest.mark.parametrize("N,E0,E1,launches", [(128, 100, 980, 2), (64, 16, 40, 1), (33, 3, 17, 1), (256, 128, 1024, 2), (1024, 1024, 64, 3)])
@pytest.mark.parametrize("name", NAMES)
def test_linear_with_dropout(t4k, dev, oracle, name, N, E0, E1, launches):
    n = N * E0
    seed, off = pw.position(name, n)
    rng = np.random.default_rng(E0 + E1)
    dX, dW, dB = dev.up(rng.standard_normal((N, E1)).astype(np.float32)), dev.up((rng.standard_normal((E0, E1)) * 0.1).astype(np.float32)), dev.up(rng.standard_normal(E0).astype(np.float32))
    dY, dF, dA = dev.zeros((N, E0)), dev.zeros((N, E0)), dev.zeros((N, E0))
    _set(t4k, seed, off)
    l0 = _launches(t4k)
    t4k.call("t4k_linear_act_fwd", p(dX), p(dW), p(dB), p(dY), oracle.L_DROPOUT, ALPHA, p(dF), p(dA), N, E0, E1, None)
    assert _launches(t4k) - l0 == launches, "the shape moved to another engine"
    assert t4k.lib.t4k_rand_offset() == pw.end_offset(off, n)
    _check_dropout("linear + dropout", dev.down(dF), dev.down(dA), dev.down(dY), seed, off, n)


@pytest.mark.parametrize("name", NAMES)
def test_mlp_head_with_dropout(t4k, dev, oracle, name):
    N, E1, H, E2 = 128, 980, 100, 10                 # the 100 -> 10 head kernel folds the 980 -> 100 split-K slabs and draws the mask: 2 launches
    n = N * H
    seed, off = pw.position(name, n)
    rng = np.random.default_rng(4)
    dX = dev.up(rng.standard_normal((N, E1)).astype(np.float32))
    dW1, dB1 = dev.up((rng.standard_normal((H, E1)) * 0.05).astype(np.float32)), dev.up(rng.standard_normal(H).astype(np.float32))
    dW2, dB2 = dev.up((rng.standard_normal((E2, H)) * 0.2).astype(np.float32)), dev.up(rng.standard_normal(E2).astype(np.float32))
    dY1, dF, dA1, dY2, dP2 = dev.zeros((N, H)), dev.zeros((N, H)), dev.zeros((N, H)), dev.zeros((N, E2)), dev.zeros((N, E2))
    _set(t4k, seed, off)
    l0 = _launches(t4k)
    t4k.call("t4k_mlp_head_fwd", p(dX), p(dW1), p(dB1), p(dY1), oracle.L_DROPOUT, ALPHA, p(dF), p(dA1), p(dW2), p(dB2), p(dY2), p(dP2), N, H, E1, E2, None)
    assert _launches(t4k) - l0 == 2, "the head no longer folds the slabs"
    assert t4k.lib.t4k_rand_offset() == pw.end_offset(off, n)
    _check_dropout("folding head", dev.down(dF), dev.down(dA1), dev.down(dY1), seed, off, n)


@pytest.mark.parametrize("N,E1,E0,stages,launches", [
    (256, 512, 256, ("leaky", "drop"), 1),       # a row of test_linear_block_forward: 32x32-sliver GEMM, the SECOND stage (ep2) draws in its epilogue
    (64, 300, 128, ("drop", "tanh"), 1),         # a row of test_linear_block_forward: the same kernel, the FIRST stage (ep1) draws
    (256, 1024, 128, ("leaky", "drop"), 2),      # K > 832: split-K, the fold's second stage draws
    (128, 320, 10, ("drop",), 1),                # head-sized: the lone stage rides in k_linsmall_fwd
], ids=["256-512-256-leaky-drop", "64-300-128-drop-tanh", "256-1024-128-leaky-drop", "128-320-10-drop"])
@pytest.mark.parametrize("name", NAMES)
def test_linear_block_run(t4k, dev, oracle, name, N, E1, E0, stages, launches):
    LAY = {"leaky": (oracle.L_LEAKYRL, 0.2), "tanh": (oracle.L_TANH, 0.0), "drop": (oracle.L_DROPOUT, ALPHA)}
    n = N * E0
    seed, off = pw.position(name, n)
    rng = np.random.default_rng(N + E1 + E0)
    dX, dW, dB = dev.up(rng.standard_normal((N, E1)).astype(np.float32)), dev.up((rng.standard_normal((E0, E1)) / np.sqrt(E1)).astype(np.float32)), dev.up(rng.standard_normal(E0).astype(np.float32))
    dY = dev.zeros((N, E0)); d = [(dev.zeros((N, E0)), dev.zeros((N, E0))) for _ in stages]
    blk = PoolBlock(); blk.KS = 1
    blk.pre_layer, blk.pre_alpha = LAY[stages[0]]; blk.pre_mask = p(d[0][0]); blk.pre_out = p(d[0][1])
    if len(stages) == 2:
        blk.post_layer, blk.post_alpha = LAY[stages[1]]; blk.post_mask = p(d[1][0]); blk.post_out = p(d[1][1])
    _set(t4k, seed, off)
    l0 = _launches(t4k)
    t4k.call("t4k_linear_block_fwd", p(dX), None, p(dW), p(dB), p(dY), ctypes.byref(blk), N, E0, E1, None)
    assert _launches(t4k) - l0 == launches, "the shape moved to another engine"
    assert t4k.lib.t4k_rand_offset() == pw.end_offset(off, n)
    k = stages.index("drop")
    inp = dev.down(dY) if k == 0 else dev.down(d[0][1])
    _check_dropout("linear block", dev.down(d[k][0]), dev.down(d[k][1]), inp, seed, off, n)


# ------------------------------------------------------------------------------------------- conv stack (own generator copy, repacked arguments)
def _stack(dev, oracle, case):
    """device buffers of CASES[case] of test_gpu_conv_stack.py and, per dropout stage in draw order, (stage, slot, n)"""
    N, H, W, Cin, stages, flat = CASES[case]
    rng = np.random.default_rng(900 + case)
    X = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    params = _params(rng, Cin, stages)
    shp = []; draws = []; h, w, c = H, W, Cin
    for si, (C0, K, pre, pool, post) in enumerate(stages):           # only the SHAPES of these host tensors are used (by _build)
        t = {"in": np.zeros((N, h, w, c), np.float32), "O": np.zeros((N, h, w, C0), np.float32)}
        if pre:
            t["pre_mask"] = t["pre_out"] = t["O"]
            if pre == "dropout": draws.append((si, "pre", N * h * w * C0))
        if pool:
            h, w = h // 2, w // 2; t["pool_out"] = np.zeros((N, h, w, C0), np.float32)
        if post:
            t["post_mask"] = t["post_out"] = np.zeros((N, h, w, C0), np.float32)
            if post == "dropout": draws.append((si, "post", N * h * w * C0))
        if flat and si == len(stages) - 1:
            t["copy_out"] = np.zeros((N, h, w, C0), np.float32)
        shp.append(t); c = C0
    arr, bufs = _build(dev, oracle, X, stages, flat, params, shp)
    return N, X, stages, arr, bufs, draws, h * w * c


def _check_stack_draws(dev, bufs, stages, draws, seed, off):
    """every dropout stage of the stack at consecutive positions; returns the unwrapped position behind the last"""
    for si, slot, n in draws:
        d = bufs[si]; pool = stages[si][3]
        inp = d["O"] if slot == "pre" else (d["pool_out"] if pool else (d["pre_out"] if stages[si][2] else d["O"]))
        _check_dropout("stage %d %s" % (si, slot), dev.down(d[slot + "_mask"]), dev.down(d[slot + "_out"]), dev.down(inp), seed, off, n)
        off += 4 * _nq(n)
    return off


@pytest.mark.parametrize("name", ["P1", "P2"])
def test_conv_stack_with_dropout_stages(t4k, dev, oracle, name):
    N, X, stages, arr, bufs, draws, _ = _stack(dev, oracle, 2)      # 3 stages: a dropout post-stage in stage 0, a dropout pre-stage in stage 2
    assert [s for _, s, _ in draws] == ["post", "pre"]
    assert t4k.lib.t4k_conv_stack_ok(arr, len(stages), N) == 1
    seed, off = pw.position(name, draws[0][2])
    dX = dev.up(X)
    _set(t4k, seed, off)
    t4k.call("t4k_conv_stack_fwd", p(dX), None, arr, len(stages), N, None)
    end = _check_stack_draws(dev, bufs, stages, draws, seed, off)
    assert t4k.lib.t4k_rand_offset() == end % 2 ** 64


@pytest.mark.parametrize("case,EA,EB", [(2, 37, 5), (0, 100, 10)], ids=["odd", "lenet"])
@pytest.mark.parametrize("name", ["P1", "P2"])
def test_conv_stack_head_with_dropout(t4k, dev, oracle, name, case, EA, EB):
    N, X, stages, arr, bufs, draws, E1 = _stack(dev, oracle, case)
    rng = np.random.default_rng(EA)
    d = {"W1": dev.up((rng.standard_normal((EA, E1)) * 0.1).astype(np.float32)), "B1": dev.up(rng.standard_normal(EA).astype(np.float32)),
         "W2": dev.up((rng.standard_normal((EB, EA)) * 0.3).astype(np.float32)), "B2": dev.up(rng.standard_normal(EB).astype(np.float32)),
         "Y1": dev.zeros((N, EA)), "Fm": dev.zeros((N, EA)), "Am": dev.zeros((N, EA)), "Y2": dev.zeros((N, EB)), "P": dev.zeros((N, EB))}
    hd = StackHead()
    hd.W1, hd.B1, hd.Y1, hd.W2, hd.B2, hd.Y2, hd.P = p(d["W1"]), p(d["B1"]), p(d["Y1"]), p(d["W2"]), p(d["B2"]), p(d["Y2"]), p(d["P"])
    hd.mid_layer, hd.mid_alpha = oracle.L_DROPOUT, ALPHA; hd.mid_mask, hd.mid_out = p(d["Fm"]), p(d["Am"])
    hd.E1, hd.E0a, hd.E0b = E1, EA, EB
    assert t4k.lib.t4k_conv_stack_head_ok(arr, len(stages), N, ctypes.byref(hd)) == 1
    seed, off = pw.position(name, draws[0][2])
    dX = dev.up(X)
    _set(t4k, seed, off)
    t4k.call("t4k_conv_stack_head_fwd", p(dX), None, arr, len(stages), N, ctypes.byref(hd), None)
    mid = _check_stack_draws(dev, bufs, stages, draws, seed, off)
    _check_dropout("head mid-dropout", dev.down(d["Fm"]), dev.down(d["Am"]), dev.down(d["Y1"]), seed, mid, N * EA)     # behind the stack's own draws
    assert t4k.lib.t4k_rand_offset() == (mid + 4 * _nq(N * EA)) % 2 ** 64


# ------------------------------------------------------------------------------------------- captured draws: the device-resident copy of the stream
@pytest.mark.parametrize("seed", [pw.SEED_P1, pw.SEED_P2], ids=["seed-P1", "seed-P2"])
def test_captured_draws_follow_the_stream_across_the_high_counter_word(t4k, dev, oracle, seed):
    """One private stream, linear capture: t4k_rand (1001), t4k_dropout_mask (6), a fused run with a dropout pre-stage (C = 8) and the conv block
    4-8-6-40 with a dropout pre-stage.  The kernels read and advance the device copy of (counter, seed); three replays, the SECOND straddling counter
    2^32, must draw the witness's values at consecutive positions; an eager draw goes on from there; a re-seed makes the device copy stale and the
    next replay draws from the new seed at position 0."""
    N, H1, C = 3, 14, 8
    n = [1001, 6, N * H1 * H1 * C, 4 * 8 * 8 * 40]
    adv = sum(_nq(k) for k in n)                                         # counters one replay draws
    start = 4 * (2 ** 32 - adv - adv // 2)
    other = 0x0123456789ABCDEF
    a, m = dev.zeros(n[0]), dev.zeros(n[1])
    X = np.random.default_rng(8).standard_normal((N, H1, H1, C)).astype(np.float32)
    dX, pm, po, pq = dev.up(X), dev.zeros(X.shape), dev.zeros(X.shape), dev.zeros((N, H1 // 2, H1 // 2, C))
    cb = _conv_block_bufs(dev, 4, 8, 6, 40)
    blk = PoolBlock(); blk.KS = 2; blk.pool_layer = oracle.L_MAXPOOL; blk.pool_out = p(pq)
    blk.pre_layer, blk.pre_alpha = oracle.L_DROPOUT, ALPHA; blk.pre_mask = p(pm); blk.pre_out = p(po)
    dev.torch.cuda.synchronize()

    def check(sd, off, what):
        t4k.call("t4k_sync", s)
        ga, gm, gpm, gpo = a.cpu().numpy(), m.cpu().numpy(), pm.cpu().numpy(), po.cpu().numpy()
        gc = {k: v.cpu().numpy() for k, v in cb.items()}
        assert np.array_equal(ga, pw.uniform(sd, off, n[0])), what + ": t4k_rand"
        off += 4 * _nq(n[0])
        assert np.array_equal(gm, pw.uniform(sd, off, n[1])), what + ": t4k_dropout_mask"
        off += 4 * _nq(n[1])
        _check_dropout(what + ": fused run", gpm, gpo, X, sd, off, n[2])
        off += 4 * _nq(n[2])
        _check_dropout(what + ": conv block", gc["pre_mask"], gc["pre_out"], gc["Y"], sd, off, n[3])
        return off + 4 * _nq(n[3])

    s = ctypes.c_void_p(); t4k.call("t4k_stream_create", ctypes.byref(s))
    g = ctypes.c_void_p()
    try:
        def sequence():
            t4k.call("t4k_rand", p(a), n[0], 0, 0.0, 1.0, s)
            t4k.call("t4k_dropout_mask", p(m), n[1], s)
            t4k.call("t4k_poolblock_fwd", p(dX), ctypes.byref(blk), N, H1, H1, H1 // 2, H1 // 2, C, s)
            _conv_block(t4k, oracle, cb, 4, 8, 6, 40, s)

        _set(t4k, seed, start)
        sequence(); t4k.call("t4k_sync", s)               # once eagerly: whatever an entry sets up on its first call is not recorded
        _set(t4k, seed, start)
        t4k.call("t4k_graph_begin", s)
        try:
            sequence()
        finally:
            t4k.call("t4k_graph_end", s, ctypes.byref(g))
        _set(t4k, seed, start)
        pos = start
        for rep in range(3):
            assert (pos // 4 < 2 ** 32 < pos // 4 + adv) == (rep == 1)                       # only the second replay straddles counter 2^32
            t4k.call("t4k_graph_launch", g, s)
            pos = check(seed, pos, "replay %d" % rep)
            assert pos == start + 4 * adv * (rep + 1) == t4k.lib.t4k_rand_offset()
        e = dev.zeros(9); t4k.call("t4k_rand", p(e), 9, 0, 0.0, 1.0, s); t4k.call("t4k_sync", s)
        assert np.array_equal(e.cpu().numpy(), pw.uniform(seed, pos, 9)), "eager draw behind the replays"
        assert t4k.lib.t4k_rand_offset() == pos + 12
        t4k.call("t4k_rand_init", other)                                                    # the device copy is stale now
        t4k.call("t4k_graph_launch", g, s)
        assert check(other, 0, "replay behind a re-seed") == 4 * adv == t4k.lib.t4k_rand_offset()
    finally:
        t4k.call("t4k_sync", s)
        if g: t4k.call("t4k_graph_destroy", g)
        t4k.call("t4k_stream_destroy", s)


# ------------------------------------------------------------------------------------------- normal draws
def _normal_case(t4k, dev, oracle, seed, off, n):
    """Box-Muller on the device against the float64 witness, element by element, at 4 x the CPU oracle's own worst error (in units of 2^-24 rad).
    The factor 4 is a margin over the reference, not a figure for the device: glibc's logf / sinf / cosf stay within about 1 ulp each, the device's
    are not correctly rounded and three of them chain; a draw from a wrong stream position errs by the order of rad itself, about 10^7 units."""
    o = oracle.lib()
    d = dev.zeros(n)
    _set(t4k, seed, off)
    t4k.call("t4k_rand", p(d), n, 1, 0.0, 1.0, None)
    assert t4k.lib.t4k_rand_offset() == pw.end_offset(off, n)
    got = dev.down(d)
    ratio = pw.normal_ratio(got, seed, off, n)
    worst, bound = float(ratio.max()), 4.0 * pw.NORMAL_ORACLE_WORST
    print("normal draw: seed %#x offset %d n %d: worst |device - float64| = %.3f x 2^-24 rad (bound %.2f)" % (seed, off, n, worst, bound))
    assert worst <= bound, "worst |device - float64| = %.3f x 2^-24 rad at element %d, bound %.2f" % (worst, int(ratio.argmax()), bound)
    ref = np.zeros(n, np.float32)
    o.t4o_rand_init(seed); o.t4o_rand_set_offset(off % 2 ** 64); o.t4o_rand(oracle.P(ref), n, 1, 0.0, 1.0)
    assert np.max(np.abs(got - ref)) < 1e-4                             # the project's bar against libm
    return got


@pytest.mark.parametrize("name", ["P1", "P2", "P3"])
def test_normal_draws_far_out(t4k, dev, oracle, name):
    seed, off = pw.position(name, 4099)
    _normal_case(t4k, dev, oracle, seed, off, 4099)


def test_normal_draws_at_the_tail(t4k, dev, oracle):
    """256 draws from 64 elements before the counter that holds the smallest u1 of the first 2^24 counters (word 154: u1 = 3.6e-8, rad = 5.855)"""
    got = _normal_case(t4k, dev, oracle, pw.TAIL_SEED, 4 * pw.TAIL_COUNTER - 64, 256)
    i = 64 + pw.TAIL_SLOT
    assert abs(float(np.hypot(got[i], got[i + 1])) - 5.855) < 1e-3
