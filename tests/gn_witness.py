"""Staged float64 witnesses of group / layer / instance norm (include/t4k.h t4k_groupnorm_fwd / _bwd, csrc/groupnorm.hip), in the manner of
bn_stats / bn_xhat / bn_y / bn_bwd_stats / bn_dx of tests/f64_witness.py: every stage is computed from the operands the kernel itself stored, so no stage
inherits the error of the one in front of it.  Tensors are NHWC, viewed as [N, HW, G, Cg]; STAT is [mean | rstd | s1 | s2], each N G long.  No element is excepted.

The rule: mean and BIASED variance per (sample, group), rstd = 1 / sqrt(var + eps) with eps INSIDE the root, xhat = (x - mean) rstd, y = xhat gamma[c] + beta[c];
backward with t = gamma[c] dy: s1 = mean_g t, s2 = mean_g (t xhat), dx = rstd (t - s1 - xhat s2), dgamma[c] += sum_{n,h,w} dy xhat, dbeta[c] += sum dy (SUMS)."""
import numpy as np

from f64_witness import C_SUM, U, W, check     # noqa: F401  (check: re-exported for the tests)

EPS = float(np.float32(1.0e-5))                # what the host passes


def groups(a, G):
    """[N, ..., C] -> float64 [N, HW, G, Cg]"""
    a = np.asarray(a, np.float64)
    N, C = a.shape[0], a.shape[-1]
    return a.reshape(N, -1, G, C // G)


def stat_parts(stat, N, G):
    """STAT -> (mean, rstd, s1, s2), each float64 [N, 1, G, 1]"""
    s = np.asarray(stat, np.float64).reshape(4, N, 1, G, 1)
    return s[0], s[1], s[2], s[3]


def rstd_bound(var, dm, E, eps=EPS):
    """(r, bound on |r_hat - r|) of r = 1 / sqrt(var + eps) for a variance computed as a sum of squared deviations from a COMPUTED mean m_hat = m + d, |d| <= dm.
    sum (x - m_hat)^2 / E = var + d^2 exactly (the cross term vanishes), and the fp32 sum carries E + 4 roundings (the subtraction, the product, E - 1
    additions, the conversion of E, the division) of its own magnitude var + d^2:
        dvar = C_SUM (E + 4) u (var + dm^2) + dm^2
    - no cancellation term: nothing here grows with (mean / sigma)^2, which is what separates the centred formula from E[x^2] - mean^2.  Chan's merge of
    (count, mean, M2) over parts is the same sum in another order: M2_a + M2_b + d_ab^2 n_a n_b / n is the centred sum about the merged mean, its terms
    non-negative, within the same gamma.  r is monotone in var: r_hat lies between r(var + dvar) and r(max(var - dvar, 0)), plus three roundings (the sum with
    eps, the root, the quotient) of r itself."""
    dvar = C_SUM * (E + 4) * U * (var + dm * dm) + dm * dm
    r = 1.0 / np.sqrt(var + eps)
    lo = 1.0 / np.sqrt(var + dvar + eps); hi = 1.0 / np.sqrt(np.maximum(var - dvar, 0.0) + eps)
    return r, np.maximum(hi - r, r - lo) + 3.0 * U * r


def gn_stats(X, G, eps=EPS):
    """(mean witness, rstd witness), each [N, G]: mean = W(m, mean|x|, E + 1) (E - 1 additions, the conversion of E, the division); rstd by rstd_bound with
    dm = C_SUM (E + 1) u mean|x|, the mean's own error"""
    x = groups(X, G); E = x.shape[1] * x.shape[3]
    m = x.mean((1, 3)); a = np.abs(x).mean((1, 3))
    var = ((x - m[:, None, :, None]) ** 2).mean((1, 3))
    dm = C_SUM * (E + 1) * U * a
    r, br = rstd_bound(var, dm, E, eps)
    return W(m, a, E + 1), W(r, br / U, 1, 1.0)


def gn_xhat(X, stat, G):
    """xhat = (x - mean) rstd from the STORED mean and rstd: two roundings"""
    x = groups(X, G); mean, rstd, _, _ = stat_parts(stat, x.shape[0], G)
    e = ((x - mean) * rstd).reshape(np.shape(X))
    return W(e, np.abs(e), 2, 1.0)


def gn_y(XH, Wg, B):
    """y = xhat gamma + beta from the STORED xhat: a product and a sum (or one fused rounding)"""
    xh = np.asarray(XH, np.float64); g = np.asarray(Wg, np.float64); b = np.asarray(B, np.float64)
    return W(xh * g + b, np.abs(xh * g) + np.abs(b), 2, 1.0)


def gn_bwd_stats(Wg, DY, XH, G, DW0, DB0, train):
    """(s1, s2, DW, DB): s1 = mean_g t over n = E + 2 roundings (the product t, E - 1 additions, the conversion of E, the division), s2 one more (t xhat);
    DW = DW0 + sum dy xhat over n = N HW + 3, DB = DB0 + sum dy over N HW + 2 - SUMS on top of the prior value; train == 0 leaves both untouched (exact)"""
    dy = np.asarray(DY, np.float64); xh = np.asarray(XH, np.float64).reshape(dy.shape); g = np.asarray(Wg, np.float64)
    t = groups(dy * g, G); tx = groups(dy * g * xh, G); E = t.shape[1] * t.shape[3]
    s1, a1 = t.mean((1, 3)), np.abs(t).mean((1, 3)); s2, a2 = tx.mean((1, 3)), np.abs(tx).mean((1, 3))
    C = dy.shape[-1]; rows = dy.size // C
    if train:
        p = (dy * xh).reshape(rows, C); d = dy.reshape(rows, C)
        wdw = W(np.asarray(DW0, np.float64) + p.sum(0), np.abs(np.asarray(DW0, np.float64)) + np.abs(p).sum(0), rows + 3)
        wdb = W(np.asarray(DB0, np.float64) + d.sum(0), np.abs(np.asarray(DB0, np.float64)) + np.abs(d).sum(0), rows + 2)
    else:
        wdw = W(np.asarray(DW0, np.float64), 0.0, 0); wdb = W(np.asarray(DB0, np.float64), 0.0, 0)
    return W(s1, a1, E + 2), W(s2, a2, E + 3), wdw, wdb


def gn_dx(Wg, DY, XH, stat, G):
    """dx = rstd (t - s1 - xhat s2) from the STORED rstd, s1 and s2: six roundings of the magnitude (t, xhat s2, two differences, the product, one to spare
    for a contraction the compiler may or may not take)"""
    dy = np.asarray(DY, np.float64); g = np.asarray(Wg, np.float64)
    t = groups(dy * g, G); xh = groups(XH, G)
    _, rstd, s1, s2 = stat_parts(stat, t.shape[0], G)
    e = rstd * (t - s1 - xh * s2)
    mag = np.abs(rstd) * (np.abs(t) + np.abs(s1) + np.abs(xh * s2))
    return W(e.reshape(dy.shape), mag.reshape(dy.shape), 6, 1.0)
