"""float64 witnesses: exact results and per-element forward error bounds for the ops the conv stack (and the per-layer kernels) perform.

An fp32 result `got` of an op passes when EVERY element satisfies

    |got - exact| <= c * n * 2^-24 * mag + n * 2^-126

  exact  the op in float64 on the very fp32 operands the kernel read (so input error never enters: each tensor is witnessed against its own op
         applied to operands the implementation itself stored),
  mag    the same op on absolute values (|X| (*) |F| + |B|, ...): the classical bound of a length-n fp32 sum, gamma_n sum |terms| (Higham,
         Accuracy and Stability of Numerical Algorithms, 3.1), which holds for ANY summation order - sequential, blocked, MFMA accumulation,
         band partials folded in any order.  n counts the roundings behind the element (products + additions of one sum).
  c      C_SUM = 2 for sums: gamma_n = n u / (1 - n u) < 1.01 n u for the n used here, and a kernel without fused multiply-adds rounds each
         product and each addition separately, which doubles the per-term count.  1 for the transcendental layers, whose n already holds
         their ulp counts (see `act`).
  n * 2^-126: flush-to-zero of results / partial sums below the smallest normal fp32 (the GPU flushes denormals in __expf and the MFMA).

No fraction of the elements may exceed the bound (no 99.99 % escape), and nothing grows with the depth but n itself.

Orientation: filters are T4(C1, K, K, C0) as the reference stores them; the forward is a correlation, dF is textbook, dX is the
un-flipped correlation of dO with the 180-degree-rotated filter (the reference's dX quirk, tests/test_oracle_vs_torch.py)."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
C_SUM = 2.0

# element-wise layers: the reference's constants (k_activate; SELU's positive branch passes the input through unscaled)
SELU_L, SELU_LA = 1.0507, 1.7581
# ulps of an fp32 exp / tanh on either side: libm's expf / tanhf <= 1-2 ulp; the GPU's __expf is v_exp_f32 (1 ulp) of x * log2(e), whose own
# rounding moves the argument by u |x| - hence the 2 |x| term on every exp below (relative error of e^x from an argument error d is d).
ULP_EXP = 4.0


class W:
    """a witness: exact value, magnitude, roundings per element (array or scalar), constant"""

    def __init__(self, exact, mag, n, c=C_SUM):
        self.exact, self.mag, self.n, self.c = np.asarray(exact, np.float64), np.asarray(mag, np.float64), n, c

    def bound(self):
        return self.c * np.asarray(self.n, np.float64) * U * self.mag + np.asarray(self.n, np.float64) * TINY


def bound_of(exact, mag, n, c=C_SUM):
    return W(exact, mag, n, c).bound()


def ratio(got, w):
    """worst |got - exact| / bound over the tensor (inf where an exact-only witness differs), its flat index"""
    got = np.asarray(got, np.float64).reshape(w.exact.shape)
    err = np.abs(got - w.exact)
    b = np.broadcast_to(w.bound(), err.shape)
    r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(got), np.inf, r)
    i = int(np.argmax(r)) if r.size else 0
    return (float(r.flat[i]) if r.size else 0.0), i


WORST = {}      # kind -> (worst ratio, name): what the sweep reports


def check(name, got, exact, mag=None, n=0, c=C_SUM, kind=None):
    """assert |got - exact| <= bound element by element; `exact` may be a W.  Returns the worst ratio to the bound.  n = 0: exact equality."""
    w = exact if isinstance(exact, W) else W(exact, np.abs(exact) if mag is None else mag, n, c)
    got = np.asarray(got, np.float64)
    assert got.size == w.exact.size, "%s: %s elements, witness %s" % (name, got.size, w.exact.size)
    r, i = ratio(got, w)
    if kind is not None and r > WORST.get(kind, (-1.0, ""))[0]:
        WORST[kind] = (r, name)
    if not r <= 1.0:
        idx = np.unravel_index(i, w.exact.shape)
        b = float(np.broadcast_to(w.bound(), w.exact.shape)[idx])
        raise AssertionError("%s: element %s got %r, exact %r, |err| %.3g > bound %.3g (ratio %.3g)"
                             % (name, tuple(int(v) for v in idx), float(got.reshape(w.exact.shape)[idx]), float(w.exact[idx]),
                                abs(float(got.reshape(w.exact.shape)[idx]) - float(w.exact[idx])), b, r))
    return r


def equal(name, got, want, kind=None):
    """bit-for-bit equality (masks of relu / leaky, pool routing, dropout): the first differing element"""
    return check(name, got, W(np.asarray(want, np.float64), 0.0, 0), kind=kind)


def f64(a):
    return np.asarray(a, np.float64)


# ----------------------------------------------------------------------------- conv (NHWC, F = T4(C1, K, K, C0))
def _cols(X, K, S, P):
    """im2col of X: [N * H0 * W0, K * K * C1] in (ky, kx, c1) order, and (H0, W0)"""
    X = f64(X); N, H, Wd, C = X.shape
    H0 = (H - K + 2 * P) // S + 1; W0 = (Wd - K + 2 * P) // S + 1
    Xp = np.zeros((N, H + 2 * P, Wd + 2 * P, C)); Xp[:, P:P + H, P:P + Wd] = X
    win = np.lib.stride_tricks.sliding_window_view(Xp, (K, K), axis=(1, 2))[:, ::S, ::S][:, :H0, :W0]   # [N, H0, W0, C, K, K]
    return np.ascontiguousarray(win.transpose(0, 1, 2, 4, 5, 3)).reshape(N * H0 * W0, K * K * C), H0, W0


def _fmat(F):
    C1, K, _, C0 = F.shape
    return f64(F).transpose(1, 2, 0, 3).reshape(K * K * C1, C0)


def conv_fwd(X, F, B, S=1, P=None):
    """O = B + X (*) F (correlation, zero padding P, stride S)"""
    C1, K, _, C0 = F.shape; P = K // 2 if P is None else P
    A, H0, W0 = _cols(X, K, S, P); Fm = _fmat(F)
    sh = (X.shape[0], H0, W0, C0)
    return W((A @ Fm + f64(B)).reshape(sh), (np.abs(A) @ np.abs(Fm) + np.abs(f64(B))).reshape(sh), K * K * C1 + 1)


def conv_dx(dO, F, H1, W1, S=1, P=None):
    """the reference's dX: DX[n, i*S+ky-P, j*S+kx-P, c1] += F[c1, K-1-ky, K-1-kx, c0] dO[n, i, j, c0]"""
    C1, K, _, C0 = F.shape; P = K // 2 if P is None else P
    dO = f64(dO); N, H0, W0, _ = dO.shape
    Ff = f64(F)[:, ::-1, ::-1, :]
    ex = np.zeros((N, H1 + 2 * P + K, W1 + 2 * P + K, C1)); mg = np.zeros_like(ex)
    for ky in range(K):
        for kx in range(K):
            f = Ff[:, ky, kx, :].T                                  # [C0, C1]
            ex[:, ky:ky + S * H0:S, kx:kx + S * W0:S] += dO @ f
            mg[:, ky:ky + S * H0:S, kx:kx + S * W0:S] += np.abs(dO) @ np.abs(f)
    return W(ex[:, P:P + H1, P:P + W1], mg[:, P:P + H1, P:P + W1], K * K * C0)


def conv_df(X, dO, K, S=1, P=None, acc=None):
    """DF[c1, ky, kx, c0] = acc + sum_{n, i, j} dO[n, i, j, c0] X[n, i*S+ky-P, j*S+kx-P, c1]"""
    P = K // 2 if P is None else P
    A, H0, W0 = _cols(X, K, S, P); C1 = X.shape[3]
    d = f64(dO).reshape(-1, dO.shape[3])
    ex = (A.T @ d).reshape(K, K, C1, -1).transpose(2, 0, 1, 3); mg = (np.abs(A).T @ np.abs(d)).reshape(K, K, C1, -1).transpose(2, 0, 1, 3)
    if acc is not None:
        ex = ex + f64(acc); mg = mg + np.abs(f64(acc))
    return W(ex, mg, d.shape[0] + (1 if acc is not None else 0))


def conv_db(dO, acc=None):
    d = f64(dO).reshape(-1, dO.shape[-1])
    ex, mg = d.sum(0), np.abs(d).sum(0)
    if acc is not None:
        ex = ex + f64(acc); mg = mg + np.abs(f64(acc))
    return W(ex, mg, d.shape[0] + (1 if acc is not None else 0))


# ----------------------------------------------------------------------------- linear, softmax
def linear(X, Wt, B):
    """Y[N, E0] = X[N, E1] W[E0, E1]^T + B"""
    X = f64(X).reshape(X.shape[0], -1); Wt = f64(Wt)
    return W(X @ Wt.T + f64(B), np.abs(X) @ np.abs(Wt).T + np.abs(f64(B)), X.shape[1] + 1)


def gemm(A, B, O0=None, alpha=1.0, beta=0.0, tA=0, tB=0):
    A = f64(A).T if tA else f64(A); B = f64(B).T if tB else f64(B)
    ex, mg = alpha * (A @ B), abs(alpha) * (np.abs(A) @ np.abs(B))
    if beta != 0:
        ex = ex + beta * f64(O0); mg = mg + abs(beta) * np.abs(f64(O0))
    return W(ex, mg, A.shape[1] + 2)                     # K products + the alpha / beta roundings


def softmax(Y):
    """P = exp(y - max) / sum exp (rows).  Per element: the exp of term j errs by E_j = ULP_EXP + 2 |y_j - max| ulps (its own rounding and the
    argument's: the subtraction and __expf's scaling by log2 e); the sum of C positive terms adds C - 1 roundings and inherits max E_j;
    the division one more.  So |P_i - exact| <= (E_i + max_j E_j + C) u P_i."""
    y = f64(Y); C = y.shape[-1]
    m = y.max(-1, keepdims=True)
    e = np.exp(y - m); ex = e / e.sum(-1, keepdims=True)
    E = ULP_EXP + 2.0 * np.abs(y - m)
    return W(ex, ex, E + E.max(-1, keepdims=True) + C, c=1.0)


# ----------------------------------------------------------------------------- element-wise layers (k_activate), pools (k_pool / k_dpool)
def act(kind, x, alpha=0.0, u=None):
    """(output witness, mask witness) of one element-wise layer on the fp32 input x.  relu / leaky / dropout: exact (n = 0; leaky's
    alpha x one rounding).  elu / selu: F = a e^x carries (ULP_EXP + 2|x|) ulps plus its multiply; O = F - a adds one rounding (and keeps F's
    absolute error: the bound is on |F|, so O's cancellation near 0 is covered).  tanh: 4 ulps on O; F = 1 - O^2 inherits 2|O| times O's
    error plus two roundings.  sigmoid: 1 / (1 + e^-x) = (ULP_EXP + 2|x| + 2) ulps; F = O (1 - O) inherits O's error (x |1 - 2 O|) plus two
    roundings.  `u`: the dropout layer's uniform draws (mask = u > alpha)."""
    x = f64(x); a = float(np.float32(alpha)); pos = x > 0
    if kind == "relu":
        return W(np.where(pos, x, 0.0), 0.0, 0), W(pos.astype(np.float64), 0.0, 0)
    if kind == "leaky":
        o = np.where(pos, x, a * x)
        return W(o, np.abs(o), np.where(pos, 0, 1), 1.0), W(np.where(pos, 1.0, a), 0.0, 0)
    if kind == "dropout":
        m = (f64(u) > a).astype(np.float64)
        return W(x * m, 0.0, 0), W(m, 0.0, 0)
    if kind in ("elu", "selu"):
        s = a if kind == "elu" else SELU_LA
        f = s * np.exp(np.minimum(x, 0.0)); nf = ULP_EXP + 2.0 * np.abs(x) + 2.0
        of = f - s
        # O's bound in units of u: nf ulps of |F| plus one rounding of |O| -> expressed as n * mag with mag = |F| + |O|
        if kind == "elu":
            o = np.where(pos, x, of); fm = np.where(pos, 1.0, f)
        else:
            o = np.where(pos, x, of); fm = np.where(pos, float(np.float32(SELU_L)), f)
        return (W(o, np.where(pos, 0.0, np.abs(f) + np.abs(of)), np.where(pos, 0, nf + 1.0), 1.0),
                W(fm, np.where(pos, 0.0, np.abs(f)), np.where(pos, 0, nf), 1.0))
    if kind == "tanh":
        o = np.tanh(x); f = 1.0 - o * o
        no = ULP_EXP
        return W(o, np.abs(o), no, 1.0), W(f, 2.0 * no * o * o + o * o + np.abs(f), 1.0, 1.0)
    if kind == "sigmoid":
        o = 1.0 / (1.0 + np.exp(-x)); f = o * (1.0 - o)
        no = ULP_EXP + 2.0 * np.abs(x) + 2.0
        return W(o, np.abs(o), no, 1.0), W(f, no * o * np.abs(1.0 - 2.0 * o) + o * np.abs(1.0 - o) + np.abs(f) + 1e-300, 1.0, 1.0)
    raise ValueError(kind)


def act_from(kind, x, alpha, mask):
    """the element-wise layer's output given the mask it stored (dropout: the mask is the Philox draw's verdict; others: recomputed)"""
    if kind == "dropout":
        return W(f64(x) * f64(mask), 0.0, 0)
    return act(kind, x, alpha)[0]


def pool(kind, x, KS=2):
    """2x2 (KSxKS) pool of NHWC x: max / min exact, avg = sum of KS^2 terms (KS^2 - 1 roundings) / KS^2 (exact for KS = 2)"""
    x = f64(x); N, H, Wd, C = x.shape; H0, W0 = H // KS, Wd // KS
    t = x[:, :H0 * KS, :W0 * KS].reshape(N, H0, KS, W0, KS, C)
    if kind == "max":
        return W(t.max((2, 4)), 0.0, 0)
    if kind == "min":
        return W(t.min((2, 4)), 0.0, 0)
    if kind == "avg":
        return W(t.mean((2, 4)), np.abs(t).mean((2, 4)), KS * KS, 1.0)
    raise ValueError(kind)


def dpool(kind, dy, x, KS=2):
    """k_dpool: avg spreads dy / KS^2 to every cell (exact for KS = 2); max / min route dy to the FIRST extreme cell of the window in scan
    order, every other cell 0.  x = the pool's forward input (its stored values decide the routing)."""
    dy = f64(dy); x = f64(x); N, H, Wd, C = x.shape; H0, W0 = H // KS, Wd // KS
    out = np.zeros_like(x)
    if kind == "avg":
        out[:, :H0 * KS, :W0 * KS] = np.repeat(np.repeat(dy / (KS * KS), KS, 1), KS, 2)
        return W(out, 0.0, 0)
    t = x[:, :H0 * KS, :W0 * KS].reshape(N, H0, KS, W0, KS, C).transpose(0, 1, 3, 5, 2, 4).reshape(N, H0, W0, C, KS * KS)
    k = (t.argmax(-1) if kind == "max" else t.argmin(-1))      # argmax / argmin return the first extreme: the reference's strict compare
    o = np.zeros((N, H0, W0, C, KS * KS)); np.put_along_axis(o, k[..., None], dy[..., None], -1)
    out[:, :H0 * KS, :W0 * KS] = o.reshape(N, H0, W0, C, KS, KS).transpose(0, 1, 4, 2, 5, 3).reshape(N, H0 * KS, W0 * KS, C)
    return W(out, 0.0, 0)


def mul(g, m):
    """g * mask (backward of an element-wise layer): one rounding"""
    e = f64(g) * f64(m)
    return W(e, np.abs(e), 1, 1.0)
