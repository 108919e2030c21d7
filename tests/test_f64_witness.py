"""CPU self-test of the float64 witness (tests/f64_witness.py): honest fp32 results - the oracle's sequential order and numpy's pairwise /
reversed orders - pass it, and the defects a banded, tiled kernel makes fail it: a tap dropped at a band's halo row or a padded edge, a bias
missing in one channel, an image missing from dF / dB, bf16 operands, the last pixel of a ragged tile copied from its neighbour, one small
softmax probability 10x off.  The old tensor-norm bar (`rel` < 1e-4) accepts the last of these; the test asserts that too."""
import numpy as np
import pytest

import f64_witness as wt

RTOL = 1e-4


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-30, np.max(np.abs(b))))


def passes(got, w):
    return wt.ratio(got, w)[0] <= 1.0


def bf16(a):
    """round-to-nearest-even to bfloat16, kept in fp32"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


# ---- honest fp32 implementations in orders other than the oracle's
def _f32_terms(X, F, K):
    """fp32 products of every tap: [N, H, W, C0, K*K*C1] (rounded once each), for stride 1 / padding K // 2"""
    N, H, Wd, C1 = X.shape; C0 = F.shape[3]; P = K // 2
    Xp = np.zeros((N, H + 2 * P, Wd + 2 * P, C1), np.float32); Xp[:, P:P + H, P:P + Wd] = X
    t = np.empty((N, H, Wd, C0, K * K * C1), np.float32)
    q = 0
    for ky in range(K):
        for kx in range(K):
            for c in range(C1):
                t[..., q] = Xp[:, ky:ky + H, kx:kx + Wd, c][..., None] * F[c, ky, kx][None, None, None, :]
                q += 1
    return t


def conv_pairwise(X, F, B, K):
    return (np.sum(_f32_terms(X, F, K), -1, dtype=np.float32) + B).astype(np.float32)   # numpy's pairwise (blocked) fp32 sum


def conv_reversed(X, F, B, K):
    t = _f32_terms(X, F, K)
    acc = np.zeros(t.shape[:-1], np.float32)
    for q in range(t.shape[-1] - 1, -1, -1):
        acc = acc + t[..., q]
    return (acc + B).astype(np.float32)


def seq_reversed(terms, axis):
    """fp32 sum along `axis`, last term first"""
    terms = np.moveaxis(np.asarray(terms, np.float32), axis, -1)
    acc = np.zeros(terms.shape[:-1], np.float32)
    for q in range(terms.shape[-1] - 1, -1, -1):
        acc = acc + terms[..., q]
    return acc


@pytest.fixture(scope="module")
def o(oracle):
    return oracle.lib()


def _conv_problem(K, seed=0):
    rng = np.random.default_rng(seed + K)
    N, H, Wd, C1, C0 = 3, 7, 9, 3, 5                     # odd grid: M = 63 pixels, a ragged last 16-pixel tile
    X = rng.standard_normal((N, H, Wd, C1)).astype(np.float32)
    F = (rng.standard_normal((C1, K, K, C0)) * 0.3).astype(np.float32)
    B = rng.standard_normal(C0).astype(np.float32)
    return X, F, B


def _oracle_conv(oracle, o, X, F, B, K):
    N, H, Wd, C1 = X.shape; C0 = F.shape[3]
    Y = np.zeros((N, H, Wd, C0), np.float32)
    assert o.t4o_conv2d_fwd(oracle.P(X), oracle.P(Y), oracle.P(F), oracle.P(B), N, H, Wd, C1, H, Wd, C0, K, 1, K // 2) == 0
    return Y


def _oracle_conv_bwd(oracle, o, X, F, dO, K, DF0, DB0):
    N, H, Wd, C1 = X.shape; C0 = F.shape[3]
    DX = np.zeros_like(X); DF = DF0.copy(); DB = DB0.copy()
    assert o.t4o_conv2d_bwd(oracle.P(X), oracle.P(np.ascontiguousarray(dO)), oracle.P(DX), oracle.P(F), oracle.P(DF), oracle.P(DB),
                            N, H, Wd, C1, H, Wd, C0, K, 1, K // 2, 1) == 0
    return DX, DF, DB


@pytest.mark.parametrize("K", [3, 5])
def test_conv_forward_honest_orders_pass_and_defects_fail(oracle, o, K):
    X, F, B = _conv_problem(K)
    w = wt.conv_fwd(X, F, B)
    honest = {"oracle": _oracle_conv(oracle, o, X, F, B, K), "pairwise": conv_pairwise(X, F, B, K), "reversed": conv_reversed(X, F, B, K)}
    for name, got in honest.items():
        wt.check("conv fwd %s" % name, got, w)
    Y = honest["oracle"]
    N, H, Wd, C1 = X.shape; P = K // 2
    # one tap dropped at a band-boundary row: the output row H // 2 loses its tap from the row above (the halo row of a second band)
    r = H // 2; c0 = 1
    taps = [(abs(F[c, 0, kx, c0] * X[0, r - P, j + kx - P, c]), c, kx, j) for c in range(C1) for kx in range(K) for j in range(Wd)
            if 0 <= j + kx - P < Wd]
    _, c, kx, j = max(taps)
    d = Y.copy(); d[0, r, j, c0] -= F[c, 0, kx, c0] * X[0, r - P, j + kx - P, c]
    assert not passes(d, w), "halo-row tap"
    # ... and one at the padded edge: column 0's rightmost in-image tap of its first row
    d = Y.copy(); cc = int(np.argmax(np.abs(F[:, P, K - 1, c0] * X[1, 0, K - 1 - P, :])))
    d[1, 0, 0, c0] -= F[cc, P, K - 1, c0] * X[1, 0, K - 1 - P, cc]
    assert not passes(d, w), "edge tap"
    # bias missing in one channel
    d = Y.copy(); d[..., 3] -= B[3]
    assert not passes(d, w), "bias"
    # operands rounded to bf16 before the multiply (fp32 accumulation)
    d = conv_pairwise(bf16(X), bf16(F), B, K)
    assert not passes(d, w), "bf16 operands"
    # the last pixel of a ragged tile (63 = 3 x 16 + 15: pixel 62 is the last of the fourth tile) copied from its neighbour
    d = Y.copy().reshape(N, H * Wd, -1); d[2, -1] = d[2, -2]
    assert not passes(d.reshape(Y.shape), w), "ragged tile"


@pytest.mark.parametrize("K", [3, 5])
def test_conv_backward_honest_orders_pass_and_defects_fail(oracle, o, K):
    X, F, B = _conv_problem(K, seed=10)
    rng = np.random.default_rng(20 + K)
    N, H, Wd, C1 = X.shape; C0 = F.shape[3]; P = K // 2
    dO = rng.standard_normal((N, H, Wd, C0)).astype(np.float32)
    DF0 = np.full(F.shape, 0.25, np.float32); DB0 = np.full(C0, -0.5, np.float32)     # accumulation onto earlier gradients
    wdx, wdf, wdb = wt.conv_dx(dO, F, H, Wd), wt.conv_df(X, dO, K, acc=DF0), wt.conv_db(dO, acc=DB0)
    DX, DF, DB = _oracle_conv_bwd(oracle, o, X, F, dO, K, DF0, DB0)
    wt.check("dX oracle", DX, wdx); wt.check("dF oracle", DF, wdf); wt.check("dB oracle", DB, wdb)
    # numpy orders: dX as the un-flipped correlation of dO with the channel-transposed filter (pairwise sum); dF / dB reversed over pixels
    Fr = np.ascontiguousarray(F.transpose(3, 1, 2, 0))                         # [C0, K, K, C1]
    wt.check("dX pairwise", conv_pairwise(dO, Fr, np.zeros(C1, np.float32), K), wdx)
    A = np.zeros((N, H + 2 * P, Wd + 2 * P, C1), np.float32); A[:, P:P + H, P:P + Wd] = X
    terms = np.stack([np.stack([A[:, ky:ky + H, kx:kx + Wd, :, None] * dO[:, :, :, None, :] for kx in range(K)], 0) for ky in range(K)], 0)
    df = seq_reversed(terms.reshape(K, K, -1, C1, C0), 2).transpose(2, 0, 1, 3) + DF0
    wt.check("dF reversed", df, wdf)
    wt.check("dB reversed", seq_reversed(dO.reshape(-1, C0), 0) + DB0, wdb)
    # one image missing from dF and dB
    _, DFm, DBm = _oracle_conv_bwd(oracle, o, X[1:].copy(), F, dO[1:].copy(), K, DF0, DB0)
    assert not passes(DFm, wdf), "dF without image 0"
    assert not passes(DBm, wdb), "dB without image 0"
    # dX: one tap dropped at a band-boundary row
    d = DX.copy(); d[0, H // 2, 2, 1] -= F[1, K - 1, P, 0] * dO[0, H // 2 - P, 2, 0]
    assert not passes(d, wdx), "dX halo tap"


def test_linear_and_softmax(oracle, o):
    rng = np.random.default_rng(3)
    N, E1, E0 = 6, 37, 11
    X = rng.standard_normal((N, E1)).astype(np.float32); Wt = (rng.standard_normal((E0, E1)) * 0.3).astype(np.float32)
    B = rng.standard_normal(E0).astype(np.float32)
    Y = np.zeros((N, E0), np.float32); assert o.t4o_linear_fwd(oracle.P(X), oracle.P(Wt), oracle.P(B), oracle.P(Y), N, E0, E1) == 0
    w = wt.linear(X, Wt, B)
    wt.check("linear oracle", Y, w)
    wt.check("linear reversed", seq_reversed(X[:, None, :] * Wt[None], 2) + B, w)
    wt.check("linear pairwise", np.sum(X[:, None, :] * Wt[None], -1, dtype=np.float32) + B, w)
    d = Y.copy(); d[:, 4] -= B[4]
    assert not passes(d, w), "linear bias"
    assert not passes(np.sum(bf16(X)[:, None, :] * bf16(Wt)[None], -1, dtype=np.float32) + B, w), "linear bf16"
    # softmax over logits wide enough for probabilities near 1e-6
    Z = (rng.standard_normal((N, E0)) * 4.0).astype(np.float32)
    Pr = np.zeros_like(Z); o.t4o_softmax(oracle.P(Z), oracle.P(Pr), N, E0)
    w = wt.softmax(Z)
    wt.check("softmax oracle", Pr, w)
    e = np.exp(Z - Z.max(1, keepdims=True)).astype(np.float32)
    wt.check("softmax reversed", e / seq_reversed(e, 1)[:, None], w)
    i = np.unravel_index(np.argmin(Pr), Pr.shape)
    assert Pr[i] < 1e-4
    d = Pr.copy(); d[i] *= 10.0
    assert not passes(d, w), "small probability 10x"
    assert rel(d, Pr) < RTOL and rel(d, w.exact) < RTOL                        # ... which the tensor-norm bar accepts: the gap is real


@pytest.mark.parametrize("kind,alpha", [("relu", 0.0), ("leaky", 0.1), ("elu", 1.0), ("selu", 0.0), ("tanh", 0.0), ("sigmoid", 0.0), ("dropout", 0.5)])
def test_activation_witness_holds_the_oracle(oracle, o, kind, alpha):
    L = {"relu": oracle.L_RELU, "leaky": oracle.L_LEAKYRL, "elu": oracle.L_ELU, "selu": oracle.L_SELU, "tanh": oracle.L_TANH,
         "sigmoid": oracle.L_SIGMOID, "dropout": oracle.L_DROPOUT}[kind]
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.standard_normal(4000) * 3, [0.0, -0.0, 1e-7, -1e-7, -30.0, 30.0, -88.0]]).astype(np.float32)
    f = rng.uniform(0, 1, x.size).astype(np.float32) if kind == "dropout" else np.zeros_like(x)
    u = f.copy(); y = np.zeros_like(x)
    assert o.t4o_activate(L, oracle.P(x), oracle.P(y), oracle.P(f), alpha, x.size) == 0
    wo, wm = wt.act(kind, x, alpha, u)
    wt.check("%s out" % kind, y, wo); wt.check("%s mask" % kind, f, wm)
    if kind in ("relu", "leaky"):
        d = f.copy(); k = int(np.argmin(np.abs(x) + (x <= 0) * 1e9)); d[k] = 0.0 if kind == "relu" else np.float32(alpha)
        assert not passes(d, wm), "mask flipped at the smallest positive input"
    if kind in ("elu", "tanh"):
        assert not passes(y * np.float32(1 + 2 ** -10), wo), "output off by 2^-10"


@pytest.mark.parametrize("kind", ["max", "avg", "min"])
def test_pool_witness_holds_the_oracle(oracle, o, kind):
    L = {"max": oracle.L_MAXPOOL, "avg": oracle.L_AVGPOOL, "min": oracle.L_MINPOOL}[kind]
    rng = np.random.default_rng(9)
    N, H, Wd, C = 2, 6, 8, 3
    x = rng.standard_normal((N, H, Wd, C)).astype(np.float32)
    x[0, :2, :2, 0] = 0.0                                                       # a tied window (after a relu): the first cell wins
    q = np.zeros((N, H // 2, Wd // 2, C), np.float32)
    assert o.t4o_pool(L, oracle.P(x), oracle.P(q), N, H, Wd, H // 2, Wd // 2, C, 2) == 0
    wt.check("pool %s" % kind, q, wt.pool(kind, x))
    dy = rng.standard_normal(q.shape).astype(np.float32)
    g = x.copy(); assert o.t4o_dpool(L, oracle.P(g), oracle.P(dy), N, H, Wd, H // 2, Wd // 2, C, 2) == 0
    w = wt.dpool(kind, dy, x)
    wt.check("dpool %s" % kind, g, w)
    if kind != "avg":
        d = g.copy(); d[0, 0, 0, 0], d[0, 0, 1, 0] = d[0, 0, 1, 0], d[0, 0, 0, 0]    # a tie routed to the second cell
        assert not passes(d, w), "tie routing"


def test_defect_table_against_both_bars(oracle, o):
    """what the old bar (`rel` < 1e-4; masks: fewer than 1e-4 of the elements off) and the witness say about each defect - asserted,
    so the table in the change description is what this test prints (pytest -s)"""
    K = 3
    X, F, B = _conv_problem(K, seed=30)
    Y = _oracle_conv(oracle, o, X, F, B, K); w = wt.conv_fwd(X, F, B)
    N, H, Wd, C1 = X.shape; C0 = F.shape[3]
    rows = []                                       # (defect, got, witness, old bar's figure: fails the old bar when >= 1e-4)
    d = Y.copy(); d[0, H // 2, 3, 1] -= F[0, 0, 1, 1] * X[0, H // 2 - 1, 3, 0]; rows.append(("tap dropped at a halo row", d, w))
    d = Y.copy(); d[1, 0, 0, 1] -= F[0, 1, 2, 1] * X[1, 0, 1, 0]; rows.append(("tap dropped at a padded edge", d, w))
    d = Y.copy(); d[..., 3] -= B[3]; rows.append(("bias missing in one channel", d, w))
    rows.append(("bf16 operands", conv_pairwise(bf16(X), bf16(F), B, K), w))
    d = Y.copy().reshape(N, H * Wd, -1); d[2, -1] = d[2, -2]; rows.append(("ragged tile's last pixel copied", d.reshape(Y.shape), w))
    dO = np.random.default_rng(32).standard_normal(Y.shape).astype(np.float32)
    DF0 = np.zeros(F.shape, np.float32); DB0 = np.zeros(C0, np.float32)
    _, DFm, DBm = _oracle_conv_bwd(oracle, o, X[1:].copy(), F, dO[1:].copy(), K, DF0, DB0)
    rows.append(("image missing from dF", DFm, wt.conv_df(X, dO, K, acc=DF0)))
    rows.append(("image missing from dB", DBm, wt.conv_db(dO, acc=DB0)))
    Z = (np.random.default_rng(31).standard_normal((4, 10)) * 4).astype(np.float32)
    Pr = np.zeros_like(Z); o.t4o_softmax(oracle.P(Z), oracle.P(Pr), 4, 10)
    d = Pr.copy(); d[np.unravel_index(np.argmin(Pr), Pr.shape)] *= 10; rows.append(("small probability 10x", d, wt.softmax(Z)))
    old_misses = {"small probability 10x"}
    for name, d, ww in rows:
        r = rel(d, ww.exact)
        print("%-32s old bar rel %.3g (%s)  witness ratio %.3g (rejects)" % (name, r, "misses" if r < RTOL else "catches", wt.ratio(d, ww)[0]))
        assert not passes(d, ww), name
        assert (r < RTOL) == (name in old_misses), (name, r)
    # a relu mask flipped in ONE of 20 000 elements: the stack tests' mask bar (fraction off < 1e-4) accepts it, the exact witness does not
    x = np.random.default_rng(33).standard_normal(20000).astype(np.float32)
    m = (x > 0).astype(np.float32); m[int(np.argmin(np.where(x > 0, x, 9.0)))] = 0.0
    assert np.mean(np.abs(m - (x > 0)) > 1e-3) < 1e-4
    assert not passes(m, wt.act("relu", x)[1])
    print("%-32s old bar fraction %.3g (misses)  witness rejects" % ("relu mask flipped at one element", np.mean(np.abs(m - (x > 0)) > 1e-3)))


# ============================================================================= the small kernels (tests/test_gpu_small_kernels_sweep.py)
# The oracle runs through EVERY shape of the GPU sweep (tests/small_kernel_cases.py) and a second honest fp32 order with it: the inputs are
# known to keep an honest implementation inside each bound before a GPU sees them.  Then the defects a tiled reduction makes.
import ctypes

import small_kernel_cases as sk


def old_sum_bar(got, x):
    """tests/test_gpu_parity.py::test_reductions' bar for a sum: within 1e-4 sum |x|"""
    return abs(float(got) - f64sum(x)) < 1e-4 * max(1.0, float(np.abs(np.asarray(x, np.float64)).sum()))


def f64sum(x):
    return float(np.asarray(x, np.float64).sum())


def relx_old(a, b, depth=1):
    """test_gpu_parity.relx's figure (tensor norm and element-aware, the floor growing with the depth)"""
    a = np.atleast_1d(np.asarray(a, np.float64)); b = np.atleast_1d(np.asarray(b, np.float64))
    floor = 1e-3 * max(1.0, (float(depth) / 32.0) ** 0.5); mx = max(1e-30, float(np.max(np.abs(b)))); d = np.abs(a - b)
    r = np.sort((d / (np.abs(b) + floor * mx)).ravel()); allowed = int((1.0 - 0.9999) * r.size + 1e-9)
    return max(float(np.max(d)) / mx, float(r[r.size - 1 - allowed]))


def test_reductions_every_sweep_size_and_the_defects_of_a_tiled_sum(oracle, o):
    rng = np.random.default_rng(60)
    x = sk.ints(rng, sk.RED_N[-1] + 8)
    for n in sk.RED_N:
        for off in sk.RED_OFFSETS:
            s = x[off:off + n]; w = wt.reduce_sum(s, exact=True)
            wt.check("oracle int sum n=%d" % n, oracle.reduce(oracle.RED_SUM, s), w); wt.check("pairwise int sum", np.sum(s, dtype=np.float32), w)
            if wt.is_int_exact(n, 16):
                wv = wt.reduce_nvar(s, 1.0, exact=True)
                wt.check("oracle int nvar n=%d" % n, oracle.reduce(oracle.RED_NVAR, s, 1.0), wv); wt.check("pairwise int nvar", np.sum((s - np.float32(1)) ** 2, dtype=np.float32), wv)
        assert oracle.reduce(oracle.RED_NVAR, np.sign(x[:n]), 0.0) == n
    for kind in ("normal", "scaled"):
        f = sk.floats(rng, sk.RED_FLOAT_N[-1] + 8, kind); avg = float(np.float32(f.mean()))
        for n in sk.RED_FLOAT_N:
            s = f[1:1 + n]
            wt.check("oracle sum", oracle.reduce(oracle.RED_SUM, s), wt.reduce_sum(s)); wt.check("pairwise sum", np.sum(s, dtype=np.float32), wt.reduce_sum(s))
            wt.check("reversed sum", seq_reversed(s[:4097], 0), wt.reduce_sum(s[:4097]))
            wt.check("oracle nvar", oracle.reduce(oracle.RED_NVAR, s, avg), wt.reduce_nvar(s, avg)); wt.check("pairwise nvar", np.sum((s - np.float32(avg)) ** 2, dtype=np.float32), wt.reduce_nvar(s, avg))
            wt.check("max", oracle.reduce(oracle.RED_MAX, s), wt.reduce_ext(s, "max")); wt.check("min", oracle.reduce(oracle.RED_MIN, s), wt.reduce_ext(s, "min"))
    # defects.  One element dropped from a 5 M-element sum; a workgroup's 4096-element slice dropped; the same slice counted twice
    n = 5000003; s = x[:n]; w = wt.reduce_sum(s, exact=True); good = np.float32(f64sum(s))
    assert passes(good, w)
    assert not passes(np.float32(f64sum(s) - float(s[n - 1])), w), "dropped element"
    sl = f64sum(s[5 * 4096:6 * 4096]) or f64sum(s[6 * 4096:7 * 4096])
    assert sl != 0.0
    assert not passes(np.float32(f64sum(s) + sl), w), "slice counted twice"
    assert not passes(np.float32(f64sum(s) - sl), w), "slice dropped"
    # ... the OLD bars accept the dropped slice (that is why the integer-exact cases exist): 1e-4 sum|x| on the sum, relx with depth on nvar
    assert old_sum_bar(np.float32(f64sum(s) - sl), s)
    m = 1 << 20; fx = rng.standard_normal(m).astype(np.float32); a = float(fx.mean())
    nv = ((fx.astype(np.float64) - a) ** 2).sum(); gone = ((fx[:4096].astype(np.float64) - a) ** 2).sum()
    assert old_sum_bar(np.float32(f64sum(fx) - f64sum(fx[:4096])), fx) or abs(f64sum(fx[:4096])) < 1e-4 * np.abs(fx).sum()
    assert relx_old(np.float32(nv - gone), nv, m) >= RTOL                    # (relx alone does see 4096 of 2^20 terms of a positive sum ...)
    assert relx_old(np.float32(nv - ((fx[:64].astype(np.float64) - a) ** 2).sum()), nv, m) < RTOL      # ... but not a wave's 64)
    y = np.sign(x[:n]); assert not passes(np.float32(n - 64), wt.reduce_nvar(y, 0.0, exact=True)), "a wave's 64 terms dropped from nvar"
    assert wt.nan_inf(np.array([1.0, np.nan, np.inf, -np.inf], np.float32)).exact == 3


def test_bce_dot_and_bias_gradient_witnesses(oracle, o):
    P = oracle.P
    rng = np.random.default_rng(61)
    N = sk.RED_N[-1] + 8
    T = rng.integers(0, 2, N).astype(np.float32); O = rng.uniform(0.01, 0.99, N).astype(np.float32); Ts = rng.random(N).astype(np.float32)
    for n in sk.RED_N:
        for t in (T, Ts):
            tn, on = t[:n].copy(), O[:n].copy()
            r = np.zeros(1, np.float32); o.t4o_bce(P(tn), P(on), n, P(r))
            w = wt.bce(t[:n], O[:n], wt.ULP_LOG_LIBM)                                  # libm: 2 ulp
            wt.check("oracle bce n=%d" % n, r[0], w)
            t32 = (t[:n] * np.log(O[:n] + np.float32(1e-6)) + (np.float32(1) - t[:n]) * np.log(np.float32(1) - O[:n] + np.float32(1e-6))).astype(np.float32)
            wt.check("pairwise bce n=%d" % n, np.sum(t32, dtype=np.float32), w)
    n = 257; w = wt.bce(T[:n], O[:n]); term, _, _ = wt.bce_terms(T[:n], O[:n])       # (where the any-order bound of a float sum still sees one term)
    assert passes(np.float32(term.sum()), w) and not passes(np.float32(term.sum() - term[-1]), w), "BCE: last (tail) term dropped"
    assert not passes(np.float32(np.sum(T[:n] * np.log(O[:n].astype(np.float64)) + (1 - T[:n]) * np.log(1 - O[:n].astype(np.float64))) * 1.001), w), "BCE 1e-3 off"
    for K in sk.DOT_K:
        for C in sk.DOT_C:
            for ints in (True, False):
                A = sk.ints(rng, (K, C)) if ints else rng.standard_normal((K, C)).astype(np.float32)
                B = sk.ints(rng, (K, C)) if ints else rng.standard_normal((K, C)).astype(np.float32)
                O0 = sk.ints(rng, C) if ints else rng.standard_normal(C).astype(np.float32)
                for alpha, beta in sk.DOT_AB:
                    w = wt.dot(A, B, O0, alpha, beta, exact=ints)
                    r = O0.copy(); o.t4o_dot(P(A), P(B), P(r), alpha, beta, K, C); wt.check("oracle dot K=%d C=%d" % (K, C), r, w)
                    wt.check("reversed dot", np.float32(alpha) * seq_reversed(A * B, 0) + np.float32(beta) * O0, w)
                    if beta != 0 and ints:                                  # (integer operands: exact, so the miss shows at every K)
                        assert not passes(r - np.float32(beta) * O0, w), "dot: beta * O missing"
                r = np.full(C, np.nan, np.float32); o.t4o_dot(P(A), P(B), P(r), 1.0, 0.0, K, C)
                assert np.all(np.isnan(r))                      # the reference's 0 * stale-O quirk; the witness (and the kernel) follow BLAS: O unread
    for E0 in sk.DB_E0:
        for N_ in sk.DB_N:
            DY = rng.standard_normal((N_, E0)).astype(np.float32); DB0 = rng.standard_normal(E0).astype(np.float32); w = wt.dlinear_db(DY, DB0)
            r = DB0.copy(); o.t4o_dlinear_db(P(DY), P(r), N_, E0); wt.check("oracle db", r, w); wt.check("reversed db", seq_reversed(DY, 0) + DB0, w)
            assert not passes(r - DB0, w) or np.all(np.abs(DB0) <= w.bound()), "db: accumulation dropped"
            DI = sk.ints(rng, (N_, E0)); r = np.zeros(E0, np.float32); o.t4o_dlinear_db(P(DI), P(r), N_, E0); assert np.array_equal(r, DI.astype(np.float64).sum(0))


def _oracle_bn(oracle, o, x, g, b, gy, DW0, DB0, train=1):
    P = oracle.P; rows, C = x.shape; N, HW = sk.bn_split(rows)
    y = np.zeros_like(x); xh = np.zeros_like(x); stat = np.zeros(3 * C, np.float32)
    o.t4o_batchnorm_fwd(P(x), P(y), P(xh), P(g), P(b), P(stat), N, HW, C)
    st1 = stat.copy(); DX = np.zeros_like(x); DW = DW0.copy(); DB = DB0.copy()
    o.t4o_batchnorm_bwd(P(g), P(gy), P(xh), P(DX), P(DW), P(DB), P(stat), N, HW, C, train)
    return y, xh, st1, DX, DW, DB, stat


def _bn_numpy(x, chunks=None, rows_used=None, eps_inside=False):
    """fp32 statistics in numpy's pairwise order (a second honest order), or with a defect"""
    rows, C = x.shape; xs = x if chunks is None else x[:chunks]
    n = np.float32(rows if rows_used is None else rows_used)
    m = np.sum(xs, 0, dtype=np.float32) / n; q = np.sum(xs * xs, 0, dtype=np.float32) / n
    var = np.maximum(q - m * m, np.float32(0))
    r = np.float32(1) / np.sqrt(var + np.float32(1e-6)) if eps_inside else np.float32(1) / (np.sqrt(var) + np.float32(1e-6))
    return np.concatenate([r, m]).astype(np.float32)


@pytest.mark.parametrize("rows,C", sk.BN_SHAPES)
def test_batchnorm_witness_at_every_sweep_shape(oracle, o, rows, C):
    rng = np.random.default_rng(62 + rows + C)
    means = sk.BN_MEANS if (rows, C) in sk.BN_MEAN_SHAPES else (0.0,)
    for mean in means:
        x = sk.bn_input(rng, rows, C, mean); g = rng.standard_normal(C).astype(np.float32); b = rng.standard_normal(C).astype(np.float32)
        gy = rng.standard_normal((rows, C)).astype(np.float32); DW0 = rng.standard_normal(C).astype(np.float32); DB0 = rng.standard_normal(C).astype(np.float32)
        for train in (1, 0):
            y, xh, st1, DX, DW, DB, st2 = _oracle_bn(oracle, o, x, g, b, gy, DW0, DB0, train)
            wm, wr = wt.bn_stats(x)
            wt.check("mean", st1[C:2 * C], wm); wt.check("rstd", st1[:C], wr); wt.check("xhat", xh, wt.bn_xhat(x, st1)); wt.check("y", y, wt.bn_y(xh, g, b))
            w1, w2, wdw, wdb = wt.bn_bwd_stats(gy, xh, DW0, DB0, train)
            wt.check("s1", st2[C:2 * C], w1); wt.check("s2", st2[2 * C:], w2); wt.check("dW", DW, wdw); wt.check("dB", DB, wdb)
            wt.check("dx", DX, wt.bn_dx(g, gy, xh, st2))
        s = _bn_numpy(x)                                                     # the second honest order
        wt.check("pairwise mean", s[C:], wm); wt.check("pairwise rstd", s[:C], wr)
        wt.check("pairwise xhat", (x - s[C:]) * s[:C], wt.bn_xhat(x, np.concatenate([s, np.zeros(C, np.float32)])))
        xi = sk.ints(rng, (rows, C)); _, _, sti, _, _, _, _ = _oracle_bn(oracle, o, xi, g, b, gy, DW0, DB0)
        assert np.array_equal(sti[C:2 * C], xi.astype(np.int64).sum(0).astype(np.float32) / np.float32(rows))
        # defects, on the integer operands (exact in any order, so one row or one chunk shows at every size; a float mean's any-order bound
        # is wider than one row in thousands): the mean taken over N*HW - 1, the last chunk of the column sums dropped
        assert not np.array_equal(sti[C:2 * C], xi.astype(np.int64).sum(0).astype(np.float32) / np.float32(rows - 1)), "mean over N*HW - 1"
        if rows >= sk.BN_CHUNKED_ROWS:
            nch, rpc = sk.bn_plan(rows); part = xi[:(nch - 1) * rpc].astype(np.int64).sum(0)
            assert part.any() and not np.array_equal(sti[C:2 * C], part.astype(np.float32) / np.float32(rows)), "last chunk dropped"


def test_batchnorm_eps_inside_the_root_and_the_cancellation_term(oracle, o):
    """eps inside the root shows on a channel of sigma = 1e-3; the bound for 1 / (sigma + eps) grows with (mean / sigma)^2 and the oracle stays
    inside it: 2.5e-4 of the value at mean 0, 1e-3 at 1 sigma, 5e-2 at 8 sigma - the largest offset of the sweep; at 64 sigma the any-order error of
    E[x^2] exceeds the variance itself (dvar >= var) and the bound opens to 1 / eps: no fp32 implementation has a variance left to speak of there"""
    rng = np.random.default_rng(63)
    rows, C = 4099, 4
    x = (rng.standard_normal((rows, C)) * 1e-3).astype(np.float32)
    wm, wr = wt.bn_stats(x)
    assert passes(_bn_numpy(x)[:C], wr) and not passes(_bn_numpy(x, eps_inside=True)[:C], wr), "eps inside the root"
    g = np.ones(C, np.float32); last = None
    for mean in (0.0, 1.0, 8.0, 64.0, 512.0):
        x = sk.bn_input(rng, rows, C, mean); y, xh, st1, *_ = _oracle_bn(oracle, o, x, g, g, x, g, g)
        wm, wr = wt.bn_stats(x)
        wt.check("rstd at mean %g sigma" % mean, st1[:C], wr); wt.check("mean", st1[C:2 * C], wm)
        rb = float(np.max(wr.bound() / wr.exact))
        assert (last is None or rb > last) if mean <= 8.0 else rb > 1e5      # the cancellation term at work: the relative bound grows with the offset, then opens
        assert mean > 8.0 or rb < 0.1; last = rb
        print("mean %5g sigma: relative bound of 1/(sigma+eps) %.3g, oracle uses %.3g of it" % (mean, rb, wt.ratio(st1[:C], wr)[0]))


def test_softmax_and_logsoftmax_at_every_sweep_shape(oracle, o):
    P = oracle.P
    rng = np.random.default_rng(64)
    for C in sk.SOFTMAX_C:
        for N in sk.SOFTMAX_N:
            Z = sk.softmax_rows(rng, N, C); y = np.zeros_like(Z); o.t4o_softmax(P(Z), P(y), N, C)
            wt.check("softmax N=%d C=%d" % (N, C), y, wt.softmax(Z))
            assert np.all(np.abs(y.astype(np.float64).sum(1) - 1.0) <= C * wt.U)
    for N, C in sk.LOGSOFTMAX_NC:
        X = (rng.standard_normal((N, C)) * 2).astype(np.float32); X[0] = -40.0
        if N > 2:
            X[2] = 80.0 - np.log(C)
        e = np.exp(X.astype(np.float64)).astype(np.float32); s = np.zeros(N, np.float32)
        for c in range(C): s = (s + e[:, c]).astype(np.float32)
        seq = e - np.log10(np.maximum(s, np.float32(1e-6)))[:, None].astype(np.float32)
        w = wt.logsoftmax(X, wt.ULP_LOG_LIBM)
        wt.check("logsoftmax sequential", seq, w)
        wt.check("logsoftmax pairwise", e - np.log10(np.maximum(np.sum(e, 1, dtype=np.float32), np.float32(1e-6)))[:, None].astype(np.float32), w)
        if N > 1:
            assert not passes(e - np.log(np.maximum(s, np.float32(1e-6)))[:, None].astype(np.float32), w), "natural log instead of log10"


@pytest.mark.parametrize("kind", ["sgd0", "sgdm", "adam", "adamw"])
def test_optimizer_witnesses(oracle, o, kind):
    P = oracle.P
    rng = np.random.default_rng(65)
    for n in sk.OPT_N + sk.OPT_CHUNKED_SIZES + sk.OPT_MULTI_SIZES:
        w0 = rng.standard_normal(n).astype(np.float32); g0 = rng.standard_normal(n).astype(np.float32)
        m0 = (rng.standard_normal(n) * 0.1).astype(np.float32); v0 = (np.abs(rng.standard_normal(n)) * 0.1).astype(np.float32)
        W_, G, M, V = w0.copy(), g0.copy(), m0.copy(), v0.copy()
        if kind == "sgd0": o.t4o_sgd(P(W_), P(G), P(M), 3, 0.01, 0.0, n); ws = wt.sgd(w0, g0, m0, 3, 0.01, 0.0) + (None,)
        elif kind == "sgdm": o.t4o_sgd(P(W_), P(G), P(M), 2, 0.01, 0.9, n); ws = wt.sgd(w0, g0, m0, 2, 0.01, 0.9) + (None,)
        elif kind == "adam": o.t4o_adam(P(W_), P(G), P(M), P(V), 1e-3, 0.9, 0.999, n); ws = wt.adam(w0, g0, m0, v0, 1e-3, 0.9, 0.999)
        else: o.t4o_adamw(P(W_), P(G), P(M), P(V), 1e-3, 0.9, 0.999, 0.01, n); ws = wt.adamw(w0, g0, m0, v0, 1e-3, 0.9, 0.999, 0.01)
        wt.check("%s w n=%d" % (kind, n), W_, ws[0]); assert not G.any()
        if ws[1] is not None: wt.check("m", M, ws[1])
        if ws[2] is not None: wt.check("v", V, ws[2])
    if kind == "sgd0":
        assert not passes(w0 - np.float32(0.01) * g0, ws[0]), "Nw scaling missing"
    if kind in ("adam", "adamw"):
        b2 = np.float32(0.999); bad = b2 * v0 + (np.float32(1) - b2) * g0
        assert not passes(bad, ws[2]), "v updated with g instead of g^2"
        assert not passes(w0 - np.float32(1e-3) * M / np.sqrt(V + np.float32(1e-6)), ws[0]) or kind == "adamw", "eps inside the root"


@pytest.mark.parametrize("K", sk.LINALG_K)
def test_linear_algebra_residual_witnesses(oracle, o, K):
    P = oracle.P
    rng = np.random.default_rng(66 + K)
    eye = np.eye(K, dtype=np.float32); st = ctypes.c_int(0)
    for kind in sk.LINALG_KINDS:
        A = sk.matrix(rng, K, kind)
        a, I = A.copy(), eye.copy(); o.t4o_inverse(P(a), P(I), K, ctypes.byref(st)); assert st.value == 0
        wt.inverse_check("inverse K=%d %s" % (K, kind), A, I)
        wt.inverse_check("numpy inverse", A, np.linalg.inv(A.astype(np.float32)).astype(np.float32))       # LAPACK's blocked order
        a, I2, piv = A.copy(), eye.copy(), np.zeros(K, np.int32); o.t4o_plu(P(a), P(I2), P(piv), K, ctypes.byref(st)); assert st.value == 0
        wt.plu_check("plu K=%d %s" % (K, kind), A, a, piv)
        assert np.array_equal(piv, wt.pivot_growth(A)[1]) or kind == "cond1e4"                # float64 picks the same pivots where they are clear
        wl, sg = wt.logdet(a); ld = np.zeros(1, np.float32); sgo = ctypes.c_int(0); o.t4o_logdet(P(a), K, P(ld), ctypes.byref(sgo))
        wt.check("logdet", ld, wl); assert sgo.value == sg
        for get_u in (0, 1):
            ref = a.copy(); o.t4o_lu_extract(P(ref), get_u, K); wt.equal("lu_extract", ref, wt.lu_extract(a, get_u).exact)
        a2, I3, piv2 = A.copy(), eye.copy(), np.zeros(K, np.int32); o.t4o_lu_inverse(P(a2), P(I3), P(piv2), K, ctypes.byref(st)); assert st.value == 0
        wt.inverse_check("lu_inverse K=%d %s" % (K, kind), A, I3, piv2)
        if K >= 5 and kind == "permuted":
            # a stale row after a pivot swap: the inverse of A with two rows exchanged back (what a swap that missed I would leave)
            bad = I3.copy(); bad[:, [0, 1]] = bad[:, [1, 0]]
            assert not passes(A.astype(np.float64) @ bad, wt.inverse_residual(A, bad, piv2)), "stale row after a swap"
            badlu = a.copy(); badlu[[1, 2], :1] = badlu[[2, 1], :1]            # L's multipliers not swapped with their rows
            L, Uu = wt.split_lu(badlu)
            assert not passes(L @ Uu, wt.W(wt.plu_residual(A, piv), np.abs(L) @ np.abs(Uu), K, wt.C_SUM)), "stale multipliers after a swap"
    for kind, want in (("singular_last", K), ("singular_first", 1)):
        A = sk.matrix(rng, K, kind); a, I = A.copy(), eye.copy(); o.t4o_inverse(P(a), P(I), K, ctypes.byref(st)); assert st.value == want


@pytest.mark.parametrize("N,H1,W1,C1,C0", sk.DCONV_SHAPES)
def test_transposed_conv_witness(oracle, o, N, H1, W1, C1, C0):
    P = oracle.P
    K, S, Pd = 4, 2, 1
    H0, W0 = wt.dconv_out(H1), wt.dconv_out(W1)
    rng = np.random.default_rng(67 + N * 100 + C0)
    I = rng.standard_normal((N, H1, W1, C1)).astype(np.float32); F = (rng.standard_normal((C1, K, K, C0)) * 0.2).astype(np.float32)
    B = rng.standard_normal(C0).astype(np.float32); G = rng.standard_normal((N, H0, W0, C0)).astype(np.float32)
    O = np.zeros((N, H0, W0, C0), np.float32)
    assert o.t4o_dconv2d_fwd(P(I), P(O), P(F), P(B), N, H1, W1, C1, H0, W0, C0, K, S, Pd) == 0
    w = wt.dconv_fwd(I, F, B, H0, W0); wt.check("dconv fwd", O, w)
    d = O.copy(); d[..., 0] -= B[0]; assert not passes(d, w), "bias"
    DX = np.zeros_like(I); DF = np.full_like(F, 0.25); DB = np.full_like(B, -0.5)
    for rep in range(2):
        DF0, DB0 = DF.copy(), DB.copy()
        assert o.t4o_dconv2d_bwd(P(I), P(G), P(DX), P(F), P(DF), P(DB), N, H1, W1, C1, H0, W0, C0, K, S, Pd, 1) == 0
        wdx, wdf, wdb = wt.dconv_bwd(I, G, F, DF0, DB0)
        wt.check("dconv dX", DX, wdx); wt.check("dconv dF", DF, wdf); wt.check("dconv dB", DB, wdb)
    assert not passes(DF - DF0, wdf), "dF not accumulated"
    assert not passes(np.ascontiguousarray(DF[:, ::-1, ::-1, :]), wdf), "taps flipped"


# ============================================================================= pools on clipped grids and the fused-run case table (tests/test_gpu_pool_runs_sweep.py)
POOL_L = {"max": "L_MAXPOOL", "min": "L_MINPOOL", "avg": "L_AVGPOOL", "usample": "L_USAMPLE"}


def _oracle_pool(oracle, o, kind, x, KS, H0, W0):
    N, H, Wd, C = x.shape; q = np.zeros((N, H0, W0, C), np.float32)
    assert o.t4o_pool(getattr(oracle, POOL_L[kind]), oracle.P(x), oracle.P(q), N, H, Wd, H0, W0, C, KS) == 0
    return q


def _oracle_dpool(oracle, o, kind, x, dy, KS, H0, W0):
    N, H, Wd, C = x.shape; g = x.copy()
    assert o.t4o_dpool(getattr(oracle, POOL_L[kind]), oracle.P(g), oracle.P(dy), N, H, Wd, H0, W0, C, KS) == 0
    return g


def _tied(rng, shape):
    """integers in {-2 .. 2}: almost every window holds its extreme more than once"""
    return rng.integers(-2, 3, shape).astype(np.float32)


@pytest.mark.parametrize("kind", ["max", "min", "avg", "usample"])
@pytest.mark.parametrize("KS", [2, 3])
@pytest.mark.parametrize("H,Wd", [(7, 5), (8, 7)])
def test_pool_witness_on_clipped_grids_holds_the_oracle_and_fails_the_defects(oracle, o, kind, KS, H, Wd):
    rng = np.random.default_rng(70 + H * 10 + KS)
    N, C = 2, 3; H0, W0 = -(-H // KS), -(-Wd // KS)                           # the ceil grid: the last window of a row / column is clipped
    assert H0 * KS > H or W0 * KS > Wd
    for x in (rng.standard_normal((N, H, Wd, C)).astype(np.float32), _tied(rng, (N, H, Wd, C))):
        dy = (rng.integers(1, 4, (N, H0, W0, C)) * rng.choice((-1, 1), (N, H0, W0, C))).astype(np.float32)      # never 0: a misrouted dy always shows
        q = _oracle_pool(oracle, o, kind, x, KS, H0, W0); w = wt.pool(kind, x, KS, H0, W0)
        wt.check("pool %s" % kind, q, w)
        g = _oracle_dpool(oracle, o, kind, x, dy, KS, H0, W0); wd = wt.dpool(kind, dy, x, KS, H0, W0, keep=x)
        wt.check("dpool %s" % kind, g, wd)
        assert wd.written.all()                                               # a ceil grid visits every cell
        t, m = wt._windows(x.astype(np.float64), KS, H0, W0); cells = m.sum(-1)
        if kind in ("avg", "usample"):
            bad = ((t * m).sum(-1) / cells).astype(np.float32)               # divided by the cells that exist instead of KS^2
            assert not passes(bad, w), "avg over the cell count"
            assert passes(bad[:, :H // KS, :Wd // KS], wt.W(w.exact[:, :H // KS, :Wd // KS], w.mag[:, :H // KS, :Wd // KS], w.n, w.c))   # ... which only the clipped windows show
        else:
            key = np.where(m, t, -np.inf if kind == "max" else np.inf)
            ext = key.max(-1, keepdims=True) if kind == "max" else key.min(-1, keepdims=True)
            last = (KS * KS - 1) - np.argmax((key == ext)[..., ::-1], -1)     # the LAST extreme of the window
            o_ = np.zeros(t.shape); np.put_along_axis(o_, last[..., None], dy.astype(np.float64)[..., None], -1)
            bad = wt._unwindow(o_, KS, H, Wd)
            if (key == ext).sum(-1).max() > 1:
                assert not passes(bad, wd), "tie routed to the last extreme"
            # a visited cell outside the arg-extreme keeps its forward value instead of 0
            idx = np.argwhere((wd.exact == 0) & (x != 0))
            assert len(idx); bad = g.copy(); bad[tuple(idx[0])] = x[tuple(idx[0])]
            assert not passes(bad, wd), "cell outside the arg-extreme not zeroed"
        # the cells of the clipped windows left holding their forward values (a kernel that skips partial windows)
        full = wt._unwindow(np.ascontiguousarray(np.broadcast_to((cells == KS * KS)[..., None], t.shape)), KS, H, Wd)
        bad = np.where(full, g, x)
        assert not passes(bad, wd), "clipped cells left at their forward value"


@pytest.mark.parametrize("kind", ["max", "min", "avg", "usample"])
def test_pool_witness_floor_grid_keeps_the_unvisited_cells(oracle, o, kind):
    """7 x 7 at KS = 2 on the floor grid 3 x 3: row 6 and column 6 belong to no window; k_dpool works in place, so they keep the forward value"""
    rng = np.random.default_rng(75)
    N, H, C, KS, H0 = 2, 7, 3, 2, 3
    x = rng.standard_normal((N, H, H, C)).astype(np.float32); dy = rng.standard_normal((N, H0, H0, C)).astype(np.float32)
    wt.check("pool", _oracle_pool(oracle, o, kind, x, KS, H0, H0), wt.pool(kind, x, KS))            # the default grid IS the floor grid
    g = _oracle_dpool(oracle, o, kind, x, dy, KS, H0, H0)
    w = wt.dpool(kind, dy, x, KS, keep=x)
    wt.check("dpool", g, w)
    assert not w.written[:, 6].any() and not w.written[:, :, 6].any() and w.written[:, :6, :6].all()
    assert np.array_equal(g[:, 6], x[:, 6]) and np.array_equal(g[:, :, 6], x[:, :, 6])
    w0 = wt.dpool(kind, dy, x, KS)                                           # without `keep` the witness says 0 there (the earlier callers' view)
    assert not w0.exact[:, 6].any() and np.array_equal(w0.exact[:, :6, :6], w.exact[:, :6, :6])
    assert not passes(g, w0)


def test_fused_run_case_table_lands_on_its_plans_at_256_cus():
    """every case of tests/small_kernel_cases.py reaches the launch plan and the vector width its label names on a 256-CU device; every
    label is reached; the boundary cases sit on either side of 512 x 256 threads and the wrap cases leave a ragged second trip"""
    seen = set()
    for c in sk.RUN_CASES:
        assert sk.run_vw(c.C) == c.vw and c.nthr * c.vw == c.N * c.H0 * c.W0 * c.C, c.id
        assert sk.run_label(c.nthr, 256) == c.plan, (c.id, sk.run_plan(c.nthr, 256))
        bs, grid, trips, tail = sk.run_plan(c.nthr, 256)
        if c.plan == "wave64":
            assert bs == 64 and 131072 - 8192 <= c.nthr < 131072 and grid == c.nthr // 64, c.id       # just below the switch
        elif c.plan == "wg256":
            assert bs == 256 and 131072 <= c.nthr <= 131072 + 8192 and grid == c.nthr // 256, c.id  # at / just above it
        else:
            assert bs == 256 and grid == sk.RUN_MAX_GRID and trips == 2 and 0 < tail < grid * bs // 32, (c.id, tail)
        seen.add(c.plan); seen.add("vw%d" % c.vw)
    assert seen == {"wave64", "wg256", "wg256_wrap", "vw4", "vw2", "vw1"}
    assert {(c.plan, c.vw) for c in sk.RUN_CASES} >= {(pl, vw) for pl in ("wave64", "wg256") for vw in (4, 2, 1)}
    for N, H1, W1, C, KS in sk.POOL_WRAP_CASES:
        H0, W0 = sk.ceil_div(H1, KS), sk.ceil_div(W1, KS); n = N * H0 * W0 * C
        grid, trips, tail = sk.pool_plan(n)
        assert grid == sk.MAX_WG and trips == 2 and 0 < tail < grid * sk.BLK and n > sk.GRID1_STRIDE_N
        assert H0 * KS > H1 and W0 * KS > W1                                  # a clipped last window in both directions
    base = 1 << 20                                                          # any 16-byte aligned address
    for label, tensor, off, vw in sk.RUN_MISALIGNED:
        ptrs = {t: base for t in sk.RUN_TENSORS + ("DY", "XH", "O")}; ptrs[tensor] += off
        got = sk.run_vw_tail(sk.run_vw(8, *(ptrs[t] for t in sk.RUN_TENSORS)), *(ptrs[t] for t in ("DY", "XH", "O")))
        assert got == vw and label == "misaligned_" + tensor, (label, off, got)
    assert {t for _, t, _, _ in sk.RUN_MISALIGNED} == set(sk.RUN_TENSORS) | {"DY", "XH", "O"}
    assert sk.run_vw(8, base) == 4 and sk.run_vw(6, base) == 2 and sk.run_vw(5, base) == 1 and sk.run_vw(8, base + 8) == 2 and sk.run_vw(6, base + 4) == 1


# ============================================================================= t4k_math over its whole domain (tests/test_gpu_math_domain.py)
# The oracle's t4o_math (libm) and NumPy's own float32 loops run through every table of sk.MATH_DOMAIN and through sk.MATH_SPECIALS; then the
# defects a k_math<OP> could carry, each on the table it is named for.
ORACLE_MATH = tuple(op for op in wt.MATH_OPS if op not in ("SIN", "COS"))       # the reference's switch has no SIN / COS case


def np32_math(op, x, v, n=None, j0=0):
    """t4k_math in NumPy float32: the second honest implementation (its own exp, log, log10, tanh, power, sin, cos, sqrt)"""
    x = np.ascontiguousarray(x, np.float32); v = np.float32(v); one = np.float32(1)
    with np.errstate(all="ignore"):
        if op == "EXP": return np.exp(x)
        if op == "LN": return np.log(np.fmax(x, wt.LNX))
        if op == "LOG": return np.log10(np.fmax(x, wt.LNX))
        if op == "TANH": return np.tanh(x)
        if op == "SIGM": return one / (one + np.exp(-x))
        if op == "POW": return np.power(x, v)
        if op == "SIN": return np.sin(x)
        if op == "COS": return np.cos(x)
        if op == "GFILL": return v * (j0 + np.arange(x.size, dtype=np.int64)).astype(np.float32) / np.float32(x.size if n is None else n)
        return wt._math_single(op, x, v)


def oracle_math(oracle, o, op, x, v):
    a = np.array(x, np.float32, copy=True); assert o.t4o_math(getattr(oracle, op), oracle.P(a), float(v), a.size) == 0
    return a


def _operands(c):
    return np.zeros(c.n, np.float32) if c.x is None else c.x


def relx_math(op, impl):
    """what tests/test_gpu_parity.py::test_elementwise_ops sees of an implementation: its operands (uniform(0.1, 2), x - 1 for five ops),
    exponent 1.5, the oracle-side value against relx < 1e-4.  None: no test called the op (SIN / COS)."""
    if op in ("SIN", "COS"):
        return None
    x = np.random.default_rng(2).uniform(0.1, 2.0, 100003).astype(np.float32)
    a = (x - 1.0).astype(np.float32) if op in ("ABS", "NEG", "RELU", "TANH", "SAT") else x
    return relx_old(impl(op, a, 1.5), np32_math(op, a, 1.5))


def test_math_tables_are_laid_out_as_the_kernel_reads_them():
    assert np.float32(1e-39) * np.float32(1) != 0 and np.float32(1e-30) * np.float32(1e-10) != 0, "this process flushes subnormals: NumPy float32 is no witness"
    ids = [c.id for c in sk.MATH_DOMAIN]; assert len(set(ids)) == len(ids)
    assert {c.op for c in sk.MATH_DOMAIN} == set(wt.MATH_OPS) and len(wt.MATH_OPS) == 21
    for c in sk.MATH_DOMAIN:
        if c.x is not None:
            assert c.x.dtype == np.float32 and c.x.size == sk.MATH_N and c.n % 4 == 3, c.id
    x = {c.id: c.x for c in sk.MATH_DOMAIN}
    e = x["EXP"]; assert e.min() == -104 and not np.any((e > 88.5) & (e < 89)) and {89.0, 100.0}.issubset(set(e.tolist())) and e.max() > 2.9e38
    l = x["LN"]; assert np.any(l == 1) and np.any(l == wt.LNX) and np.any((l > 0) & (l < sk.F32_MIN)) and np.any(l == 0) and np.any(l < 0) and np.any(np.abs(l - 1) < 1e-6)
    assert np.any((x["SQRT"] > 0) & (x["SQRT"] < sk.F32_MIN)) and np.any(x["SQRT"] < 0) and np.any(np.signbit(x["SQRT"]) & (x["SQRT"] == 0))
    assert np.any(np.abs(x["RCP"]) < sk.F32_MIN) and np.any(np.abs(x["RCP"]) > 1e38) and np.any(x["RCP"] == 0)
    assert np.any(x["POW-v0.5"] < 0) and np.any(x["POW-v3"] < 0) and not np.any(x["POW-v7"] < 0) and np.any(x["POW-v0"] == 0) and not np.any(x["POW-v1"] == 0)
    assert np.abs(x["SIN"]).max() > 1e38 and np.any(x["SIN"] == np.float32(np.pi)) and np.any((x["SIN"] != 0) & (np.abs(x["SIN"]) < 1e-30))
    assert sk.MATH_SPECIALS.size == 12 and np.isnan(sk.MATH_SPECIALS[0]) and sk.MATH_SPECIALS_ROW.size % 4 == 3
    # the float64 sine behind the SIN / COS witness is itself reduced exactly at 3e38: libm's, one argument at a time, agrees
    import math
    big = x["SIN"][np.abs(x["SIN"]) > 1e6][:200].astype(np.float64)
    assert np.allclose(np.sin(big), [math.sin(t) for t in big], rtol=0, atol=1e-13) and np.allclose(np.cos(big), [math.cos(t) for t in big], rtol=0, atol=1e-13)


def test_math_witness_holds_libm_and_numpy_on_every_table(oracle, o):
    """the overflow gap is empty on every table, the oracle passes for the 19 ops it has and NumPy float32 for all 21 - with the SAME ULP_POW /
    ULP_SIN / ULP_COS the device is held to; the worst figure of both in ulps of |exact| is printed beside them (pytest -s)"""
    worst = {}
    for c in sk.MATH_DOMAIN:
        x = _operands(c); w = wt.math(c.op, x, c.v, c.n)
        assert not wt.in_gap(w).any(), "%s: element %d within 1 %% of FLT_MAX" % (c.id, int(np.argmax(wt.in_gap(w))))
        impls = [("numpy", np32_math(c.op, x, c.v, c.n))] + ([("oracle", oracle_math(oracle, o, c.op, x, c.v))] if c.op in ORACLE_MATH else [])
        for name, got in impls:
            wt.check("%s %s" % (name, c.id), got, w)
            if c.op in ("POW", "SIN", "COS"):
                with np.errstate(all="ignore"):
                    u = np.abs(got - w.exact) / (wt.U * np.abs(w.exact))
                u = np.where(np.isfinite(u) & (np.abs(w.exact) >= wt.TINY), u, 0.0)                  # (below FLT_MIN the n 2^-126 term holds a result, not its ulps)
                worst[(c.op, name)] = max(worst.get((c.op, name), 0.0), float(u.max()))
        if c.op in wt.MATH_EXACT + ("GFILL",) and c.op in ORACLE_MATH:
            ok = ~np.isnan(w.f32)
            assert np.array_equal(impls[1][1][ok], w.f32[ok]) and np.all(np.isnan(impls[1][1][~ok])), c.id     # the oracle's single operations ARE NumPy's
    for k in sorted(worst):
        print("%s %s: worst %.3f ulps of |exact| (allowance %.1f)" % (k[0], k[1], worst[k], getattr(wt, "ULP_" + k[0])))
    for op in ("POW", "SIN", "COS"):
        meas, allow = getattr(wt, "MEASURED_" + op), getattr(wt, "ULP_" + op)
        assert allow == np.ceil(2.0 * meas * 10.0 - 1e-9) / 10.0, "%s: the allowance is twice the device's measured worst, rounded up to one decimal" % op
        assert allow * wt.U <= 1e-4, "an allowance past the element bar of 1e-4 relative is a defect of k_math, not a constant"


def test_math_specials_witness_holds_libm_and_numpy(oracle, o):
    """MATH_SPECIALS through every op: NaN / +inf / -inf / finite agree between the witness, the oracle and NumPy; the clamps' answer to a NaN"""
    x = sk.MATH_SPECIALS_ROW
    for op in wt.MATH_OPS:
        for v in ((1.5, 3.0, -1.0) if op == "POW" else (1.5,)):
            w = wt.math(op, x, v)
            assert not (wt.in_gap(w) & (np.broadcast_to(w.n, w.exact.shape) != 0)).any(), op     # (ABS of FLT_MAX IS FLT_MAX: exact ops have no rounding to fear)
            for name, got in [("numpy", np32_math(op, x, v))] + ([("oracle", oracle_math(oracle, o, op, x, v))] if op in ORACLE_MATH else []):
                assert np.array_equal(wt.kinds(got), wt.kinds(w.exact)), (op, v, name)
                wt.check("%s specials %s v=%g" % (name, op, v), got, w)
    nan = np.array([np.nan], np.float32)
    assert wt.math("LN", nan).exact[0] == np.log(np.float64(wt.LNX)) and wt.math("LOG", nan).exact[0] == np.log10(np.float64(wt.LNX))
    assert all(wt.math(op, nan).exact[0] == 0 for op in ("SQRT", "RELU", "SAT")) and np.isnan(wt.math("SIN", np.array([np.inf], np.float32)).exact[0])
    # the pairs of the binary entries: NumPy float32 is the oracle's arithmetic
    a, b = np.repeat(sk.MATH_SPECIALS, 12), np.tile(sk.MATH_SPECIALS, 12)
    with np.errstate(all="ignore"):
        for op, f in (("ADD", np.add), ("SUB", np.subtract), ("MUL", np.multiply), ("DIV", np.divide)):
            r = np.zeros_like(a); assert o.t4o_tt_op(getattr(oracle, op), oracle.P(a), oracle.P(b), oracle.P(r), a.size) == 0
            want = f(a, b); ok = ~np.isnan(want)
            assert np.array_equal(r[ok].view(np.uint32), want[ok].view(np.uint32)) and np.all(np.isnan(r[~ok])), op


def test_activation_witness_holds_the_oracle_on_the_wide_row(oracle, o):
    """k_activate's rows of the domain sweep (linspace(-104, 104), the specials): the oracle stays inside wt.act as it stands"""
    for x in (sk.ACT_DOMAIN, sk.MATH_SPECIALS_ROW):
        for kind, alpha in sk.ACT_DOMAIN_KINDS:
            L = getattr(oracle, {"leaky": "L_LEAKYRL"}.get(kind, "L_" + kind.upper()))
            y = np.zeros_like(x); f = np.zeros_like(x); assert o.t4o_activate(L, oracle.P(x), oracle.P(y), oracle.P(f), alpha, x.size) == 0
            with np.errstate(all="ignore"):
                wo, wm = wt.act(kind, x, alpha)
            wt.check("%s out" % kind, y, wo); wt.check("%s mask" % kind, f, wm)
            assert np.array_equal(wt.kinds(y), wt.kinds(wo.exact)) and np.array_equal(wt.kinds(f), wt.kinds(wm.exact)), kind


# defect -> (the op it replaces, the implementation, the tables that must fail - every other table of every op must pass)
def _d_ln(x, v): return np.log(np.fmax(x, np.float32(1e-6)))
def _d_sqrt(x, v): return np.sqrt(x)
def _d_sigm(x, v): return np.float32(1) / (np.float32(1) + np.exp(x))
def _d_sigm_nan(x, v): e = np.exp(x); return e / (np.float32(1) + e)                      # right where e^x is finite, NaN where it overflows
def _d_pow(x, v): return np.power(np.abs(x), np.float32(v))
def _d_exp(x, v): return np.exp2((x * np.float32(int(np.log2(np.e) * 2 ** 11) / 2.0 ** 11)).astype(np.float32)).astype(np.float32)   # log2(e) cut to 12 bits
def _d_tanh(x, v): return np.where(np.abs(x) < np.float32(1e-2), x, np.tanh(x))
def _d_rcp(x, v): r = np.float32(1) / x; return np.where(np.abs(r) < sk.F32_MIN, np.float32(0), r)


MATH_DEFECTS = (
    ("LN clamped at 1e-6", {"LN": _d_ln}, {"LN"}),
    ("SQRT without the guard", {"SQRT": _d_sqrt}, {"SQRT"}),
    ("SIGM as 1 / (1 + e^x)", {"SIGM": _d_sigm}, {"SIGM"}),
    ("SIN and COS swapped", {"SIN": lambda x, v: np.cos(x), "COS": lambda x, v: np.sin(x)}, {"SIN", "COS"}),
    ("POW on |a|", {"POW": _d_pow}, {"POW-v3", "POW-v-1", "POW-v0.5"}),         # (|a|^2 = a^2: the v = 2 table cannot tell)
    ("EXP through a 12-bit log2(e)", {"EXP": _d_exp}, {"EXP"}),
    ("GFILL with j / n in integers", {"GFILL": None}, {c.id for c in sk.MATH_DOMAIN if c.op == "GFILL" and c.n > 1}),
    ("TANH as x below 1e-2", {"TANH": _d_tanh}, {"TANH"}),
    ("RCP flushing subnormal results", {"RCP": _d_rcp}, {"RCP"}),
    ("SIGM as e^x / (1 + e^x)", {"SIGM": _d_sigm_nan}, {"SIGM"}),
)
OLD_BAR_ACCEPTS = {"LN clamped at 1e-6", "SQRT without the guard", "SIN and COS swapped", "POW on |a|", "TANH as x below 1e-2",
                   "RCP flushing subnormal results", "SIGM as e^x / (1 + e^x)"}


@pytest.mark.parametrize("name,repl,named", MATH_DEFECTS, ids=[d[0] for d in MATH_DEFECTS])
def test_math_defects_fail_on_their_named_tables_only(name, repl, named):
    def impl(op, x, v, n=None):
        if op not in repl:
            return np32_math(op, x, v, n)
        with np.errstate(all="ignore"):
            if op == "GFILL":
                return (np.float32(v) * (np.arange(x.size, dtype=np.int64) // (n or x.size)).astype(np.float32)).astype(np.float32)
            return np.asarray(repl[op](np.ascontiguousarray(x, np.float32), v), np.float32)
    failed = set()
    for c in sk.MATH_DOMAIN:
        if c.n > 100000 and c.op not in repl:
            continue                                                            # (the 2^24 rows: an untouched op is NumPy itself, held above)
        if not passes(impl(c.op, _operands(c), c.v, c.n), wt.math(c.op, _operands(c), c.v, c.n)):
            failed.add(c.id)
    assert failed == named, (name, sorted(failed ^ named))
    # the old bar on today's operands: relx < 1e-4 against libm on uniform(0.1, 2) - asserted either way, so the table in tests/README.md is this test's
    figs = [relx_math(op, impl) for op in repl]
    accepted = all(f is None or f < RTOL for f in figs)
    print("%-34s old bar: %s  -> %s; the witness fails %s" % (name, ", ".join("no test" if f is None else "%.3g" % f for f in figs),
                                                            "accepts" if accepted else "rejects", ", ".join(sorted(named))))
    assert accepted == (name in OLD_BAR_ACCEPTS), (name, figs)
