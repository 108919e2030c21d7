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
    """worst |got - exact| / bound over the tensor (inf where an exact-only witness differs), its flat index.  Where the witness itself is
    not finite (the math-op domain, `math` below) no bound applies: an exact NaN asks for a NaN, an exact infinity for that infinity; a NaN
    anywhere else is inf as before."""
    got = np.asarray(got, np.float64).reshape(w.exact.shape)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - w.exact)
        b = np.broadcast_to(w.bound(), err.shape)
        r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(got), np.inf, r)
    special = ~np.isfinite(w.exact)
    if special.any():
        r = np.where(special, np.where((np.isnan(w.exact) & np.isnan(got)) | (got == w.exact), 0.0, np.inf), r)
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


def _windows(x, KS, H0, W0):
    """the pool windows of NHWC x on an H0 x W0 grid in scan order, [N, H0, W0, C, KS * KS], and which of their cells exist,
    [1, H0, W0, 1, KS * KS]: a ceil grid (H0 = ceil(H / KS)) clips its edge windows at the tensor's border, as k_pool does"""
    N, H, Wd, C = x.shape; Hp, Wp = H0 * KS, W0 * KS
    assert 0 < H0 <= -(-H // KS) and 0 < W0 <= -(-Wd // KS), "a window without a cell"
    xp = np.zeros((N, max(Hp, H), max(Wp, Wd), C)); xp[:, :H, :Wd] = x
    ok = np.zeros((max(Hp, H), max(Wp, Wd)), bool); ok[:H, :Wd] = True
    t = xp[:, :Hp, :Wp].reshape(N, H0, KS, W0, KS, C).transpose(0, 1, 3, 5, 2, 4).reshape(N, H0, W0, C, KS * KS)
    m = ok[:Hp, :Wp].reshape(H0, KS, W0, KS).transpose(0, 2, 1, 3).reshape(1, H0, W0, 1, KS * KS)
    return t, m


def _unwindow(o, KS, H, Wd):
    """inverse of _windows: [N, H0, W0, C, KS * KS] back onto the H x Wd grid (cells no window holds: 0)"""
    N, H0, W0, C, _ = o.shape; Hp, Wp = H0 * KS, W0 * KS
    out = np.zeros((N, max(Hp, H), max(Wp, Wd), C), o.dtype)
    out[:, :Hp, :Wp] = o.reshape(N, H0, W0, C, KS, KS).transpose(0, 1, 4, 2, 5, 3).reshape(N, Hp, Wp, C)
    return out[:, :H, :Wd]


def pool(kind, x, KS=2, H0=None, W0=None):
    """KSxKS pool of NHWC x on an H0 x W0 grid (default: the floor grid H // KS): max / min exact, over the cells that exist; avg = sum of
    the existing cells (KS^2 - 1 roundings) / KS^2 - ALWAYS KS^2, also in a clipped edge window, as k_pool divides (exact for KS = 2).
    usample = avg: the up-sample layer's backward is k_pool's L_USAMPLE case, which shares the L_AVGPOOL arithmetic (division included)."""
    x = f64(x); N, H, Wd, C = x.shape
    H0 = H // KS if H0 is None else H0; W0 = Wd // KS if W0 is None else W0
    t, m = _windows(x, KS, H0, W0)
    if kind == "max":
        return W(np.where(m, t, -np.inf).max(-1), 0.0, 0)
    if kind == "min":
        return W(np.where(m, t, np.inf).min(-1), 0.0, 0)
    if kind in ("avg", "usample"):
        return W((t * m).sum(-1) / (KS * KS), (np.abs(t) * m).sum(-1) / (KS * KS), KS * KS, 1.0)
    raise ValueError(kind)


def dpool(kind, dy, x, KS=2, H0=None, W0=None, keep=None):
    """k_dpool on an H0 x W0 grid (default: the floor grid): avg spreads dy / KS^2 to every cell of the window (exact for KS = 2, one rounding for KS = 3), usample
    spreads dy undivided; max / min route dy to the FIRST extreme cell of the window in row-major scan order, every other cell of the window
    0.  x = the pool's forward input (its stored values decide the routing).  Every cell some window holds is written and no other: the
    witness carries that as `.written` ([N, H, W, C] bool).  The kernels work in place on the forward buffer, so the cells NO window visits
    (the last rows / columns of a floor grid on a non-multiple extent) keep what the buffer held - pass it as `keep` to have the witness say
    so; without it those cells are 0 (the callers with H % KS == 0 never see the difference)."""
    dy = f64(dy); x = f64(x); N, H, Wd, C = x.shape
    H0 = H // KS if H0 is None else H0; W0 = Wd // KS if W0 is None else W0
    dy = dy.reshape(N, H0, W0, C)
    t, m = _windows(x, KS, H0, W0)
    if kind in ("avg", "usample"):
        o = np.broadcast_to((dy / (KS * KS) if kind == "avg" else dy)[..., None], t.shape) * m
    elif kind in ("max", "min"):
        k = np.where(m, t, -np.inf).argmax(-1) if kind == "max" else np.where(m, t, np.inf).argmin(-1)   # the first extreme: the reference's strict compare
        o = np.zeros(t.shape); np.put_along_axis(o, k[..., None], dy[..., None], -1)
    else:
        raise ValueError(kind)
    written = _unwindow(np.ascontiguousarray(np.broadcast_to(m, t.shape)), KS, H, Wd)
    out = _unwindow(o, KS, H, Wd)
    if keep is not None:
        out = np.where(written, out, f64(keep).reshape(x.shape))
    # avg at KS = 3: dy / 9 is one rounding (the division by 4 of KS = 2 is exact, as is every routing)
    w = W(out, np.abs(out) * written, 1, 1.0) if kind == "avg" and KS * KS & (KS * KS - 1) else W(out, 0.0, 0)
    w.written = written
    return w


def mul(g, m):
    """g * mask (backward of an element-wise layer): one rounding"""
    e = f64(g) * f64(m)
    return W(e, np.abs(e), 1, 1.0)


# ----------------------------------------------------------------------------- reductions (k_reduce1 / k_reduce2, k_dot, k_dlinear_db)
# ulps of an fp32 natural log on either side, relative to |log x|: libm's logf <= 1 ulp (the oracle passes with ULP_LOG_LIBM = 2).  The GPU's
# __logf is v_log_f32 (a base-2 log) times ln 2; neither kernel guide states the instruction's error near 1, so it was MEASURED: worst
# |__logf(x) - ln x| / (2^-24 |ln x|) over x in [0.01, 0.99 + 1e-6] (the BCE arguments, |ln x| >= 0.01; t4k_math LN on 1.5 M points and single-term
# t4k_bce calls) - see MEASURED_LOG below and tests/README.md.  The allowance is twice the measurement, rounded up.
MEASURED_LOG = 3.137    # MI355X: t4k_math LN 3.137, single BCE terms 2.234 (tests/test_gpu_small_kernels_sweep.py::test_device_log_error_is_inside_the_allowance prints both)
ULP_LOG = 6.3           # 2 x 3.137, rounded up
ULP_LOG_LIBM = 2.0
# t4k_math POW / SIN / COS (powf, sinf, cosf of the device library): no figure in the project or the guides either, so MEASURED the same way -
# worst |got - exact| / (2^-24 |exact|) against float64 over the tables of small_kernel_cases.MATH_DOMAIN on the MI355X
# (tests/test_gpu_math_domain.py prints them) - and the allowance is twice the measurement, rounded up to one decimal (twice: the tables
# sample the domain, and a point release of the device library may move a last ulp).  The same constants hold libm and NumPy's float32
# loops on the CPU (tests/test_f64_witness.py: libm powf 0.990, NumPy power 1.730, sin 1.800, cos 1.781 on the same tables).
MEASURED_POW, MEASURED_SIN, MEASURED_COS = 2.19023, 1.80014, 2.29681     # MI355X: at (-2.0427191)^2, sin 3.1100991, cos 81126.922
ULP_POW, ULP_SIN, ULP_COS = 4.4, 3.7, 4.6                                # 2 x each, rounded up to one decimal
EPS =float(np.float32(1.0e-6))                                    # DU_EPS as the kernels hold it


def is_int_exact(n, max_term):
    """every fp32 partial sum of n terms of magnitude <= max_term (integers) is an integer below 2^24: exact in ANY order"""
    return float(n) * float(max_term) < 2.0 ** 24


def _sum_w(terms, n_extra=0, exact=False, axis=None):
    t = f64(terms)
    if exact:                                                      # small-integer operands: the result must be bit-equal
        assert is_int_exact(t.shape[0] if axis == 0 else t.size, np.max(np.abs(t)) if t.size else 0.0) and np.all(t == np.rint(t)), "not integer-exact"
        return W(t.sum(axis), 0.0, 0)
    return W(t.sum(axis), np.abs(t).sum(axis), (t.shape[0] if axis == 0 else t.size) + n_extra)


def reduce_sum(x, exact=False):
    return _sum_w(np.ravel(x), 0, exact)


def reduce_nvar(x, avg, exact=False):
    """sum (x - avg)^2 with avg as the fp32 scalar the ABI passes: a subtraction and a product behind every term"""
    d = f64(np.ravel(x)) - float(np.float32(avg))
    return _sum_w(d * d, 3, exact)


def reduce_ext(x, op):
    """max / min: exact (fmaxf / fminf pick one of the operands; +0 / -0 compare equal, see the sweep's signed-zero case)"""
    return W(np.max(f64(x)) if op == "max" else np.min(f64(x)), 0.0, 0)


def nan_inf(x):
    x = np.asarray(x); return W(float(np.count_nonzero(np.isnan(x) | np.isinf(x))), 0.0, 0)


def dot(A, B, O0=None, alpha=1.0, beta=0.0, exact=False):
    """O[c] = alpha <A[:, c], B[:, c]> + beta O[c] on [K, C] operands; beta == 0 leaves O unread (the BLAS convention, as `gemm` above)"""
    A = f64(A); B = f64(B); K = A.shape[0]
    alpha = float(np.float32(alpha)); beta = float(np.float32(beta))
    ex = alpha * (A * B).sum(0); mg = abs(alpha) * (np.abs(A) * np.abs(B)).sum(0)
    if beta != 0:
        ex = ex + beta * f64(O0); mg = mg + abs(beta) * np.abs(f64(O0))
    if exact:
        assert is_int_exact(1, np.max(mg)) and np.all(ex == np.rint(ex)), "not integer-exact"
        return W(ex, 0.0, 0)
    return W(ex, mg, K + 2)


def dlinear_db(DY, DB0):
    """DB[e] += sum_n DY[n, e]"""
    return conv_db(DY, acc=DB0)


def bce_terms(T, O):
    """the float64 terms t ln(o + eps) + (1 - t) ln(1 - o + eps) and their two halves' magnitudes"""
    t = f64(np.ravel(T)); o = f64(np.ravel(O))
    a = t * np.log(o + EPS); b = (1.0 - t) * np.log(1.0 - o + EPS)
    return a + b, np.abs(a) + np.abs(b), np.abs(t) + np.abs(1.0 - t)


def bce(T, O, ulp_log=None):
    """sum of the terms.  Per term: each log carries ulp_log ulps of its own value plus the rounding of its argument (o + eps, 1 - o + eps:
    two roundings of a number near its own size = an ABSOLUTE 2 u on the log), the (1 - t), the two products and the addition three more
    roundings of the term's magnitude; the sum adds n roundings of sum |terms| (any order).  Encoded as n * (sum|terms| + E / n)."""
    ulp_log = ULP_LOG if ulp_log is None else ulp_log
    term, mg, tw = bce_terms(T, O)
    n = term.size
    E = float(((ulp_log + 3.0) * mg + 2.0 * tw).sum())
    return W(term.sum(), np.abs(term).sum() + E / max(1, n), n)


# ----------------------------------------------------------------------------- batch norm ([NHW, C] view; stat = [1 / (sigma + eps) | mean | -])
def bn_stats(X):
    """(mean witness, 1 / (sigma + eps) witness) per channel, as the reference writes them: var = E[x^2] - mean^2, eps OUTSIDE the root.
    The computed q = E[x^2] and m = mean each carry gamma = C_SUM (n + 2) u of sum |terms| (n terms, the products, the division), so
        |var_hat - var| <= dvar = gamma (q + 2 |m| mean|x|) + 2 u (q + m^2)        (m^2's product and the subtraction)
    - the cancellation in q - m^2 is NOT in a constant: dvar / var grows as (mean / sigma)^2.  1 / (sigma + eps) is monotone in var, so the
    result lies between r(var + dvar) and r(max(var - dvar, 0)) (first order: dvar / (2 sigma (sigma + eps)^2)), plus three roundings
    (root, sum, quotient) of r itself."""
    x = f64(X).reshape(-1, X.shape[-1]); n = x.shape[0]
    m = x.mean(0); a = np.abs(x).mean(0); q = (x * x).mean(0)
    var = np.maximum(q - m * m, 0.0); sig = np.sqrt(var); r = 1.0 / (sig + EPS)
    gam = C_SUM * (n + 2) * U
    dvar = gam * (q + 2.0 * np.abs(m) * a) + 2.0 * U * (q + m * m)
    lo = 1.0 / (np.sqrt(var + dvar) + EPS); hi = 1.0 / (np.sqrt(np.maximum(var - dvar, 0.0)) + EPS)
    br = np.maximum(hi - r, r - lo) + 3.0 * U * r
    return W(m, a, n + 1), W(r, br / U, 1, 1.0)


def bn_xhat(X, stat):
    """xhat = (x - mean) * rstd from the STORED statistics: two roundings"""
    x = f64(X).reshape(-1, X.shape[-1]); C = x.shape[1]; s = f64(stat)
    e = (x - s[C:2 * C]) * s[:C]
    return W(e, np.abs(e), 2, 1.0)


def bn_y(XH, Wg, B):
    """y = xhat * gamma + beta from the STORED xhat: a product and a sum (or one fused rounding)"""
    xh = f64(XH).reshape(-1, XH.shape[-1]); g = f64(Wg); b = f64(B)
    return W(xh * g + b, np.abs(xh * g) + np.abs(b), 2, 1.0)


def bn_bwd_stats(DY, XH, DW0, DB0, train):
    """(s1 = mean dy, s2 = mean dy * xhat, DW, DB): the MEANS are accumulated into the parameter gradients (reference quirk), train == 0
    leaves them untouched (exact)"""
    dy = f64(DY).reshape(-1, DY.shape[-1]); xh = f64(XH).reshape(dy.shape); n = dy.shape[0]
    s1, a1 = dy.mean(0), np.abs(dy).mean(0); s2, a2 = (dy * xh).mean(0), np.abs(dy * xh).mean(0)
    if train:
        wdw = W(f64(DW0) + s2, np.abs(f64(DW0)) + a2, n + 3); wdb = W(f64(DB0) + s1, np.abs(f64(DB0)) + a1, n + 2)
    else:
        wdw = W(f64(DW0), 0.0, 0); wdb = W(f64(DB0), 0.0, 0)
    return W(s1, a1, n + 1), W(s2, a2, n + 2), wdw, wdb


def bn_dx(Wg, DY, XH, stat):
    """dx = (rstd * gamma) * (dy - s1 - xhat * s2) from the STORED rstd / s1 / s2: five roundings of the magnitude"""
    dy = f64(DY).reshape(-1, DY.shape[-1]); xh = f64(XH).reshape(dy.shape); C = dy.shape[1]; s = f64(stat); g = f64(Wg)
    k = s[:C] * g; s1 = s[C:2 * C]; s2 = s[2 * C:3 * C]
    return W(k * (dy - s1 - xh * s2), np.abs(k) * (np.abs(dy) + np.abs(s1) + np.abs(xh * s2)), 5, 1.0)


# ----------------------------------------------------------------------------- log-softmax layer as the reference writes it
def logsoftmax(X, ulp_log=None):
    """O = exp(x) - log10(max(sum_c exp(x), 1e-6)).  e_j errs by E_j = ULP_EXP + 2 |x_j| ulps; the row sum S by (max E + C) ulps, which
    moves log10 S by that much / ln 10 ABSOLUTELY; the log itself ulp_log ulps of |log10 S|; the subtraction one rounding of e + |log10 S|."""
    ulp_log = ULP_LOG if ulp_log is None else ulp_log
    x = f64(X); C = x.shape[-1]
    e = np.exp(x); E = ULP_EXP + 2.0 * np.abs(x)
    S = np.maximum(e.sum(-1, keepdims=True), EPS); ls = np.log10(S)
    mag = E * e + (E.max(-1, keepdims=True) + C) / np.log(10.0) + ulp_log * np.abs(ls) + (e + np.abs(ls))
    return W(e - ls, mag, 1, 1.0)


# ----------------------------------------------------------------------------- optimizers: one step, element-wise (a handful of roundings)
def _f(v):
    return float(np.float32(v))


def sgd(G, DG, M, Nw, lr, b):
    """(weights, momentum or None): d = dg / Nw; b == 0: g - lr d (3 roundings); else m' = b m + (1 - b) d (5), g' = g - lr m' (7 in all)"""
    g, d, lr, b = f64(G), f64(DG) / float(Nw), _f(lr), _f(b)
    if abs(b) < EPS:
        return W(g - lr * d, np.abs(g) + np.abs(lr * d), 3, 1.0), None
    m = b * f64(M) + (1.0 - b) * d; mm = np.abs(b * f64(M)) + np.abs((1.0 - b) * d)
    return W(g - lr * m, np.abs(g) + lr * mm, 7, 1.0), W(m, mm, 5, 1.0)


def _moments(DG, M, V, b1, b2):
    d = f64(DG)
    m = b1 * f64(M) + (1.0 - b1) * d; mm = np.abs(b1 * f64(M)) + np.abs((1.0 - b1) * d)
    v = b2 * f64(V) + (1.0 - b2) * d * d; vm = np.abs(b2 * f64(V)) + (1.0 - b2) * d * d
    return d, m, mm, v, vm


def adam(G, DG, M, V, lr, b1, b2):
    """(weights, m, v): m' 4 roundings, v' 5, g' = g - lr m' / (sqrt v' + eps): m's 4, half of v's 5, root, sum, product, quotient, difference
    <= 12 of |g| + lr mag(m') / (sqrt v' + eps); no bias correction, eps outside the root (the reference's Adam)"""
    lr, b1, b2 = _f(lr), _f(b1), _f(b2)
    d, m, mm, v, vm = _moments(DG, M, V, b1, b2)
    den = np.sqrt(np.maximum(v, 0.0)) + EPS
    return W(f64(G) - lr * m / den, np.abs(f64(G)) + lr * mm / den, 12, 1.0), W(m, mm, 4, 1.0), W(v, vm, 5, 1.0)


def adamw(G, DG, M, V, lr, b1, b2, wd):
    """g' = g - lr (m' / (sqrt v' + eps) - wd d) as the reference writes it (the decay multiplies the GRADIENT): 14 roundings"""
    lr, b1, b2, wd = _f(lr), _f(b1), _f(b2), _f(wd)
    d, m, mm, v, vm = _moments(DG, M, V, b1, b2)
    den = np.sqrt(np.maximum(v, 0.0)) + EPS
    return (W(f64(G) - lr * (m / den - wd * d), np.abs(f64(G)) + lr * (mm / den + np.abs(wd * d)), 14, 1.0), W(m, mm, 4, 1.0), W(v, vm, 5, 1.0))


# ----------------------------------------------------------------------------- transposed convolution (dconv.hip: K = 4, S = 2, P = 1)
def dconv_out(H1, K=4, S=2, P=1):
    """output extent of the layer, with the output padding the odd grids take"""
    return (H1 - 1) * S - 2 * P + K + (H1 + 2 * P - K) % S


def dconv_fwd(I, F, B, H0, W0, S=2, P=1):
    """O[n, i S + ky - P, j S + kx - P, co] = B[co] + sum_ci F[ci, ky, kx, co] I[n, i, j, ci] (no tap flip): the dX of the virtual conv O -> I,
    whose filter is F with the channel roles swapped; conv_dx applies the reference's flip, so the taps are flipped here to cancel it"""
    Fv = np.ascontiguousarray(f64(F).transpose(3, 1, 2, 0)[:, ::-1, ::-1, :])
    w = conv_dx(I, Fv, H0, W0, S, P)
    return W(w.exact + f64(B), w.mag + np.abs(f64(B)), w.n + 1)


def dconv_bwd(I, dO, F, DF0, DB0, S=2, P=1):
    """(dX, dF, dB): dX is the plain convolution of dO with F (channel roles swapped), dF the virtual conv's filter gradient folded back
    (one more rounding: it is formed apart and added), dB the column sum of dO"""
    K = F.shape[1]
    Fv = np.ascontiguousarray(f64(F).transpose(3, 1, 2, 0))
    wdx = conv_fwd(dO, Fv, np.zeros(F.shape[0]), S, P)
    w = conv_df(dO, I, K, S, P)
    wdf = W(w.exact.transpose(3, 1, 2, 0) + f64(DF0), w.mag.transpose(3, 1, 2, 0) + np.abs(f64(DF0)), w.n + 2)
    return wdx, wdf, conv_db(dO, acc=DB0)


# ----------------------------------------------------------------------------- linear algebra, by residual
# c of the residual bounds.  PLU: |P A - L U| <= gamma_K |L| |U| (Higham 9.3) -> C_SUM.  A column of the inverse solved from computed factors:
# |A x - e| <= 3 gamma_K |L| |U| |x| (Higham 9.4); |L| |U| is held to |A| by the pivot growth (the issue's form), and Gauss-Jordan eliminates
# above the diagonal as well (twice the operations): c = 3 * 2 * 1.01 rounded up.
C_LINALG = 8.0


def perm_of(piv):
    """row order after the sequential swaps row k <-> row piv[k]"""
    p = np.arange(len(piv))
    for k, q in enumerate(np.asarray(piv)):
        if q != k:
            p[[k, q]] = p[[q, k]]
    return p


def pivot_growth(A, piv=None):
    """max_k max|a^(k)_ij| / max|a_ij| of Gaussian elimination in float64 on the given pivot order (None: partial pivoting), and that order"""
    a = f64(A).copy(); K = a.shape[0]; top = g = float(np.max(np.abs(a))); used = []
    for z in range(K):
        u = int(piv[z]) if piv is not None else z + int(np.argmax(np.abs(a[z:, z])))
        used.append(u)
        if u != z:
            a[[z, u]] = a[[u, z]]
        if a[z, z] == 0.0:
            break
        a[z + 1:, z + 1:] -= np.outer(a[z + 1:, z] / a[z, z], a[z, z + 1:]); a[z + 1:, z] = 0.0
        g = max(g, float(np.max(np.abs(a))))
    return g / max(top, 1e-300), np.array(used)


def inverse_residual(A, X, piv=None):
    """witness of R = A @ X (float64 product of the fp32 A and the fp32 X the implementation returned) against I"""
    A = f64(A); K = A.shape[0]; rho, _ = pivot_growth(A, piv)
    return W(np.eye(K), (np.abs(A) @ np.abs(f64(X))) * rho, K, C_LINALG)


def plu_residual(A, piv):
    """witness of L @ U (float64 product of the stored factors) against P A; the magnitude |L| |U| is the caller's (see plu_check)"""
    return f64(A)[perm_of(piv)]


def split_lu(LU):
    LU = f64(LU); return np.tril(LU, -1) + np.eye(LU.shape[0]), np.triu(LU)


def plu_check(name, A, LU, piv, kind=None):
    L, Uu = split_lu(LU); K = L.shape[0]
    return check(name, L @ Uu, W(plu_residual(A, piv), np.abs(L) @ np.abs(Uu), K, C_SUM), kind=kind)


def inverse_check(name, A, X, piv=None, kind=None):
    return check(name, f64(A) @ f64(X), inverse_residual(A, X, piv), kind=kind)


def logdet(LU):
    """(sum log |u_ii| on the STORED factors: K logs of 2 ulps each and K additions; sign exact)"""
    d = np.diag(f64(LU)); l = np.log(np.abs(d)); K = d.size
    return W(l.sum(), np.abs(l).sum(), K + 3, 1.0), int(np.prod(np.sign(d)))


def lu_extract(LU, get_u):
    L, Uu = split_lu(LU); return W(Uu if get_u else L, 0.0, 0)


# ----------------------------------------------------------------------------- t4k_math (k_math<OP>): every op over its whole domain
FLT_MAX = float(np.finfo(np.float32).max)
LNX = np.float32(1.0e-12)                                        # DU_LNX as the kernel holds it: the clamp of LN / LOG
MATH_EXACT = ("ABS", "NEG", "RELU", "SAT", "FILL", "SCALE", "ADD", "SUB", "MUL", "DIV", "SQRT", "RCP")   # single IEEE operations
MATH_OPS = MATH_EXACT + ("GFILL", "EXP", "LN", "LOG", "TANH", "SIGM", "POW", "SIN", "COS")
GAP = (0.99, 1.01)                                               # x FLT_MAX: no table holds an element whose exact value lies in here


def _math_single(op, x, v):
    """the single IEEE operation `op` in the dtype of x (float32: the expected bits; float64: the value before rounding).  fmax / fmin
    return their other operand for a NaN, as fmaxf / fminf do: the guards of RELU, SAT and SQRT turn a NaN into 0."""
    zero, one = x.dtype.type(0), x.dtype.type(1)
    if op == "ABS": return np.abs(x)
    if op == "NEG": return -x
    if op == "RELU": return np.fmax(zero, x)
    if op == "SAT": return np.fmin(one, np.fmax(zero, x))
    if op == "FILL": return np.full_like(x, v)
    if op in ("SCALE", "MUL"): return x * v
    if op == "ADD": return x + v
    if op == "SUB": return x - v
    if op == "DIV": return x / v
    if op == "SQRT": return np.sqrt(np.fmax(x, zero))
    if op == "RCP": return one / x
    raise ValueError(op)


def math(op, x, v=0.0, n_total=None, j0=0):
    """witness of t4k_math(op, x, v) on the fp32 operands x (GFILL / FILL read only its shape; GFILL: element i is index j0 + i of n_total).
      single IEEE operations and GFILL (two of them on the rounded conversions of j and n): n = 0, the same expression in NumPy float32 -
        subnormal operands and results included; the expected bits are `.f32`
      EXP  ULP_EXP + 2|x| ulps of e^x;  SIGM  two more (the sum and the quotient);  TANH  4 ulps: `act`'s figures
      LN / LOG  ULP_LOG ulps of |ln c|, |log10 c| with c = fmaxf(x, 1e-12) - the clamp is part of the witness (a NaN takes it too) - and
        c = 1 gives exactly 0
      POW / SIN / COS  ULP_POW / ULP_SIN / ULP_COS ulps of |exact|; POW follows C powf: a negative base is signed under an integral
        exponent and NaN under a fractional one, 0^0 = 1
    One overflow rule: where |exact| > FLT_MAX the result must be the infinity of that sign (no table holds an element within GAP of
    FLT_MAX, where an honest rounding could go either way - tests/test_f64_witness.py asserts it on `.true`, the float64 value before any
    rounding).  Results below FLT_MIN may flush: the n 2^-126 term.  |x| in the exp terms is capped at 128, past every saturation."""
    x32 = np.ascontiguousarray(x, np.float32); v32 = np.float32(v); xd = x32.astype(np.float64); vd = float(v32)
    with np.errstate(all="ignore"):
        if op == "GFILL":
            n = x32.size if n_total is None else int(n_total)
            j = (j0 + np.arange(x32.size, dtype=np.int64)).astype(np.float32).reshape(x32.shape)
            r = v32 * j / np.float32(n)
            w = W(r.astype(np.float64), 0.0, 0, 1.0); w.f32 = r; w.true = w.exact
            return w
        if op in MATH_EXACT:
            r = _math_single(op, x32, v32); assert r.dtype == np.float32
            w = W(r.astype(np.float64), 0.0, 0, 1.0); w.f32 = r; w.true = _math_single(op, xd, vd)
            return w
        ax = np.minimum(np.nan_to_num(np.abs(xd), nan=0.0), 128.0)
        if op == "EXP":
            t = np.exp(xd); n = ULP_EXP + 2.0 * ax
        elif op in ("LN", "LOG"):
            c = np.fmax(x32, LNX).astype(np.float64)
            t = np.log(c) if op == "LN" else np.log10(c); n = np.where(c == 1.0, 0.0, ULP_LOG)
        elif op == "TANH":
            t = np.tanh(xd); n = ULP_EXP
        elif op == "SIGM":
            t = 1.0 / (1.0 + np.exp(-xd)); n = ULP_EXP + 2.0 * ax + 2.0
        elif op == "POW":
            t = np.power(xd, vd); n = ULP_POW
        elif op == "SIN":
            t = np.sin(xd); n = ULP_SIN
        elif op == "COS":
            t = np.cos(xd); n = ULP_COS
        else:
            raise ValueError(op)
        over = np.abs(t) > FLT_MAX
        w = W(np.where(over, np.copysign(np.inf, t), t), np.where(over | np.isnan(t), 0.0, np.abs(t)), n, 1.0)
    w.true = t
    return w


def in_gap(w):
    """the elements of a `math` witness whose value before rounding lies within GAP of FLT_MAX"""
    a = np.abs(w.true)
    return (a >= GAP[0] * FLT_MAX) & (a <= GAP[1] * FLT_MAX)


def kinds(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf: what two implementations must agree on before their finite values are held to a witness (zeros are
    finite, of either sign)"""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))
