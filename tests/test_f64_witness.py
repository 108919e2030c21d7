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
