"""Staged float64 witnesses of add & norm (include/t4k.h t4k_addnorm_fwd / _bwd, csrc/addnorm.hip), in the manner of tests/gn_witness.py: every
stage is computed from the operands the kernel itself stored (or was given), so no stage inherits the error of the one in front of it.  Tensors are [rows, C];
RSTD is [rows].  No element is excepted.

The rule, per token: z = x + s (z = x without a skip);
    mode 1: mean = sum z / C, var = sum (z - mean)^2 / C (biased, centred on the token's own computed mean), rstd = 1 / sqrt(var + eps), xhat = (z - mean) rstd
    mode 2: rstd = 1 / sqrt(sum z^2 / C + eps), xhat = z rstd
    both:   y = xhat gamma[c] + beta[c];    mode 0: y = z
backward with t = dy + dy2 (dy2 absent when untapped), g = gamma t:
    mode 0: dz = t;   mode 1: dz = rstd (g - mean_c g - xhat mean_c (g xhat));   mode 2: dz = rstd (g - xhat mean_c (g xhat))
    dgamma[c] += sum_rows t xhat, dbeta[c] += sum_rows t (SUMS).

The bounds, with u = 2^-24 and C_SUM = 2 the allowance every sum of f64_witness.py has (a bound `n` roundings of magnitude `mag` is C_SUM n u mag):
  (a) z: one rounding of |x| + |s| (none without a skip: exact).  mean: the fp32 sum of C ROUNDED z over C - 1 additions, the conversion of C, the division -
      C + 1 + nz roundings of mean|z|, nz = 1 with a skip.  Neither is stored; they bound (b) and (c).
  (b) rstd: `_rstd_bound` below, from the error dv of the quantity under the root.
  (c) xhat from the operands, the mean of (a) and the STORED rstd; y from the STORED xhat.
  (d) dz from the STORED xhat and rstd; the two means are not stored, their error is carried.
  (e) dgamma | dbeta from the STORED xhat: rows products and additions in a fixed tree, on top of the prior value.
The second block is the float32 restatement of the team algorithm the plan test runs inside these bounds, and wrong ones it runs outside them."""
import numpy as np

from f64_witness import C_SUM, U, W, check, ratio     # noqa: F401  (check, ratio: re-exported for the tests)

EPS = float(np.float32(1.0e-5))                # what the host passes


def f64(a, C):
    return np.asarray(a, np.float64).reshape(-1, C)


def z_of(X, S, C):
    """(z, |x| + |s|, nz): z in float64, its magnitude, the roundings it carries in fp32 (1 with a skip, else 0)"""
    x = f64(X, C)
    if S is None:
        return x, np.abs(x), 0
    s = f64(S, C)
    return x + s, np.abs(x) + np.abs(s), 1


def an_z(X, S, C):
    """mode 0's output, and the z of the other modes: one rounding, none without a skip"""
    z, az, nz = z_of(X, S, C)
    return W(z, az, nz, 1.0)


def _mean(z, az, nz, mode):
    """(mean [rows, 1], its error bound dm [rows, 1]): C + 1 + nz roundings of mean|z| under C_SUM; mode 2 subtracts no mean: 0, exactly"""
    C = z.shape[1]
    if mode != 1:
        return np.zeros((z.shape[0], 1)), np.zeros((z.shape[0], 1))
    return z.mean(1, keepdims=True), C_SUM * (C + 1 + nz) * U * az.mean(1, keepdims=True)


def an_mean(X, S, C, mode):
    z, az, nz = z_of(X, S, C)
    m, _ = _mean(z, az, nz, mode)
    return W(m[:, 0], az.mean(1), C + 1 + nz)


def _rstd_bound(v, dv, eps):
    """(r, bound on |r_hat - r|) of r = 1 / sqrt(v + eps) for a v computed with error at most dv: r is monotone in v, so r_hat lies between r(v + dv) and
    r(max(v - dv, 0)), plus three roundings (the sum with eps, the root, the quotient) of r itself"""
    r = 1.0 / np.sqrt(v + eps)
    lo = 1.0 / np.sqrt(v + dv + eps); hi = 1.0 / np.sqrt(np.maximum(v - dv, 0.0) + eps)
    return r, np.maximum(hi - r, r - lo) + 3.0 * U * r


def an_rstd(X, S, C, mode, eps=EPS):
    """rstd [rows].  With e the error of a rounded z (|e| <= nz u (|x| + |s|)) and d the error of the computed mean (|d| <= dm):
    mode 1: sum (z + e - mean - d)^2 / C = var + mean_c (e - d)^2 + 2 mean_c ((z - mean) e) exactly - the cross term with d vanishes, sum (z - mean) = 0 - so
        dv = mean_c (|e| + dm)^2 + 2 mean_c |z - mean| |e|  +  C_SUM (C + 4) u (var + the former)
    (the subtraction, the product, C - 1 additions, the conversion of C, the division, of the sum's own magnitude).  No cancellation term: nothing here grows
    with (mean / sigma)^2, which is what separates the centred formula from E[z^2] - mean^2.
    mode 2: sum (z + e)^2 / C = ms + mean_c (2 z e + e^2):  dv = mean_c (2 |z| |e| + e^2) + C_SUM (C + 3) u (ms + the former)."""
    z, az, nz = z_of(X, S, C)
    e = nz * U * az
    if mode == 1:
        m, dm = _mean(z, az, nz, 1)
        v = ((z - m) ** 2).mean(1)
        din = ((e + dm) ** 2).mean(1) + 2.0 * (np.abs(z - m) * e).mean(1)
        dv = din + C_SUM * (C + 4) * U * (v + din)
    else:
        v = (z * z).mean(1)
        din = (2.0 * np.abs(z) * e + e * e).mean(1)
        dv = din + C_SUM * (C + 3) * U * (v + din)
    r, br = _rstd_bound(v, dv, eps)
    return W(r, br / U, 1, 1.0)


def an_xhat(X, S, RSTD, C, mode):
    """xhat = (z - mean) rstd from the STORED rstd: the errors of z and of the mean times rstd, and three roundings of the result (the subtraction, the product,
    one to spare for a contraction the compiler may or may not take)"""
    z, az, nz = z_of(X, S, C)
    m, dm = _mean(z, az, nz, mode)
    r = np.abs(np.asarray(RSTD, np.float64).reshape(-1, 1))
    e = (z - m) * np.asarray(RSTD, np.float64).reshape(-1, 1)
    return W(e, 3.0 * np.abs(e) + r * (nz * az + dm / U), 1, 1.0)


def an_y(XH, Wg, B, C):
    """y = xhat gamma + beta from the STORED xhat: a product and a sum (or one fused rounding)"""
    xh = f64(XH, C); g = np.asarray(Wg, np.float64); b = np.asarray(B, np.float64)
    return W(xh * g + b, np.abs(xh * g) + np.abs(b), 2, 1.0)


def t_of(DY, DY2, C):
    dy = f64(DY, C)
    if DY2 is None:
        return dy, np.abs(dy), 0
    d2 = f64(DY2, C)
    return dy + d2, np.abs(dy) + np.abs(d2), 1


def an_dx(Wg, DY, DY2, XH, RSTD, C, mode):
    """dz from the STORED xhat and rstd.  mode 0: t, one rounding with a dy2.  Else g = gamma t carries nd + 1 roundings of |gamma| (|dy| + |dy2|) = G; m1 =
    mean_c g carries those and C + 1 more (C - 1 additions, the conversion, the division) of mean G, m2 = mean_c (g xhat) one more of mean (G |xhat|); the
    result five roundings of |rstd| (|g| + |m1| + |xhat m2|) (two differences, two products, one to spare).  All under C_SUM where they are sums."""
    t, at, nd = t_of(DY, DY2, C)
    if mode == 0:
        return W(t, at, nd, 1.0)
    g64 = np.asarray(Wg, np.float64)
    xh = f64(XH, C); r = np.asarray(RSTD, np.float64).reshape(-1, 1)
    g = g64 * t; G = np.abs(g64) * at
    m1 = g.mean(1, keepdims=True) if mode == 1 else np.zeros((g.shape[0], 1))
    m2 = (g * xh).mean(1, keepdims=True)
    e1 = C_SUM * (C + 2 + nd) * G.mean(1, keepdims=True) if mode == 1 else 0.0
    e2 = C_SUM * (C + 3 + nd) * (G * np.abs(xh)).mean(1, keepdims=True)
    e = r * (g - m1 - xh * m2)
    mag = np.abs(r) * ((nd + 1) * G + e1 + np.abs(xh) * e2 + 5.0 * (np.abs(g) + np.abs(m1) + np.abs(xh * m2)))
    return W(e, mag, 1, 1.0)


def an_dwdb(DY, DY2, XH, DW0, DB0, C, train):
    """(DW, DB) from the STORED xhat: DW = DW0 + sum_rows t xhat over rows + 3 + nd roundings (t, the product, rows - 1 additions in the workgroups' and the
    fold's trees, the sum onto the prior value, one to spare), DB = DB0 + sum t over rows + 2 + nd - SUMS on top of the prior value; train == 0 leaves both
    untouched (exact)"""
    d0 = np.asarray(DW0, np.float64); b0 = np.asarray(DB0, np.float64)
    if not train:
        return W(d0, 0.0, 0), W(b0, 0.0, 0)
    t, at, nd = t_of(DY, DY2, C)
    xh = f64(XH, C); rows = t.shape[0]
    return (W(d0 + (t * xh).sum(0), np.abs(d0) + (at * np.abs(xh)).sum(0), rows + 3 + nd),
            W(b0 + t.sum(0), np.abs(b0) + at.sum(0), rows + 2 + nd))


def ratios(X, S, Wg, B, DY, DY2, DW0, DB0, C, mode, train, O, XH, RSTD, DX, DW, DB, eps=EPS):
    """worst ratio to the bound of every stage, each from what the kernel stored"""
    out = {}
    if mode == 0:
        out["o"] = ratio(O, an_z(X, S, C))[0]
    else:
        out["rstd"] = ratio(RSTD, an_rstd(X, S, C, mode, eps))[0]
        out["xhat"] = ratio(XH, an_xhat(X, S, RSTD, C, mode))[0]
        out["o"] = ratio(O, an_y(XH, Wg, B, C))[0]
    out["dx"] = ratio(DX, an_dx(Wg, DY, DY2, XH, RSTD, C, mode))[0]
    if mode != 0:
        wdw, wdb = an_dwdb(DY, DY2, XH, DW0, DB0, C, train)
        out["dw"] = ratio(DW, wdw)[0]; out["db"] = ratio(DB, wdb)[0]
    return out


# ----------------------------------------------------------------------------- the team algorithm in NumPy float32
F = np.float32


def team_of(C, vw):
    """(T, rung) of t4k_addnorm_plan: the smallest T of 8, 16, 32, 64 lanes that leaves a lane at most 8 items of the load width, else the 256-thread workgroup"""
    items = C // vw
    for T in (8, 16, 32, 64):
        if -(-items // T) <= 8:
            return T, 1
    return 256, 2


def team_sum(v, T, vw):
    """v: float32 [rows, C] -> float32 [rows], summed as the kernel does: lane l adds its items l, l + T .. in order, the lanes are joined by an xor butterfly
    (over the wave, then the four wave sums pairwise, on the 256-thread team)"""
    rows, C = v.shape
    items = C // vw
    pad = np.zeros((rows, 8 * T * vw), F); pad[:, :C] = v
    lanes = pad.reshape(rows, 8, T, vw)
    acc = np.zeros((rows, T), F)
    for k in range(8):
        if k * T >= items:
            break
        for q in range(vw):
            acc = (acc + lanes[:, k, :, q]).astype(F)
    width = min(T, 64)
    a = acc.reshape(rows, T // width, width)
    off = width // 2
    idx = np.arange(width)
    while off >= 1:
        a = (a + a[:, :, idx ^ off]).astype(F)
        off //= 2
    a = a[:, :, 0]
    if T == 256:
        return ((a[:, 0] + a[:, 1]).astype(F) + (a[:, 2] + a[:, 3]).astype(F)).astype(F)
    return a[:, 0]


def f32_addnorm(X, S, Wg, B, DY, DY2, DW0, DB0, C, mode, train=1, eps=EPS, vw=1, wrong=None):
    """(O, XH, RSTD, DX, DW, DB) in float32, operation by operation as csrc/addnorm.hip (products and sums rounded separately).  wrong: one of the restatements
    the bounds must refuse - 'eps_outside', 'unbiased', 'ex2', 'dw_mean', 'no_dy2', 'rms_centred'"""
    x = np.asarray(X, F).reshape(-1, C); rows = x.shape[0]
    z = x if S is None else (x + np.asarray(S, F).reshape(-1, C)).astype(F)
    T, _ = team_of(C, vw)
    fC = F(C); e32 = F(eps)
    w = np.asarray(Wg, F); b = np.asarray(B, F)
    dy = np.asarray(DY, F).reshape(-1, C)
    t = dy if (DY2 is None or wrong == "no_dy2") else (dy + np.asarray(DY2, F).reshape(-1, C)).astype(F)
    if mode == 0:
        return z, None, None, t, np.asarray(DW0, F), np.asarray(DB0, F)
    centred = mode == 1 or wrong == "rms_centred"
    mean = (team_sum(z, T, vw) / fC).astype(F)[:, None] if centred else np.zeros((rows, 1), F)
    if wrong == "ex2":
        var = ((team_sum((z * z).astype(F), T, vw) / fC).astype(F) - (mean[:, 0] * mean[:, 0]).astype(F)).astype(F)
    else:
        d = (z - mean).astype(F)
        q = team_sum((d * d).astype(F), T, vw)
        var = (q / (F(C - 1) if wrong == "unbiased" else fC)).astype(F)
    with np.errstate(invalid="ignore"):                                    # ('ex2' can leave a negative variance: the NaN is outside every bound)
        if wrong == "eps_outside":
            rstd = (F(1.0) / (np.sqrt(var).astype(F) + e32).astype(F)).astype(F)
        else:
            rstd = (F(1.0) / np.sqrt((var + e32).astype(F)).astype(F)).astype(F)
    xh = ((z - mean).astype(F) * rstd[:, None]).astype(F)
    o = ((xh * w).astype(F) + b).astype(F)
    g = (w * t).astype(F)
    m1 = (team_sum(g, T, vw) / fC).astype(F)[:, None] if mode == 1 else np.zeros((rows, 1), F)
    m2 = (team_sum((g * xh).astype(F), T, vw) / fC).astype(F)[:, None]
    dx = (rstd[:, None] * ((g - m1).astype(F) - (xh * m2).astype(F)).astype(F)).astype(F)
    dw = np.asarray(DW0, F).copy(); db = np.asarray(DB0, F).copy()
    if train:
        aw = np.zeros(C, F); ab = np.zeros(C, F)
        for r in range(rows):
            aw = (aw + (t[r] * xh[r]).astype(F)).astype(F); ab = (ab + t[r]).astype(F)
        if wrong == "dw_mean":
            aw = (aw / F(rows)).astype(F)
        dw = (dw + aw).astype(F); db = (db + ab).astype(F)
    return o, xh, rstd, dx, dw, db
