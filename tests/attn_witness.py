"""Staged float64 witnesses of multi-head attention (include/t4k.h t4k_attention_fwd / _bwd, csrc/attention.hip), in the manner of
tests/gn_witness.py: every stage is computed from the operands the kernel itself stored, so no stage inherits the error of the one in front of it.  Built from
f64_witness's U, C_SUM, ULP_EXP and TINY; nothing is fitted to an output and no element is excepted.

The rule.  QKV is [N, L, 3E], E = heads d, a token's channels [ Q | K | V ], head h owning channels h d .. (h + 1) d - 1 of each E; Y is [N, L, E], LSE
[N, heads, L].  With scale = float32(1 / sqrt(d)) (formed in double, rounded once):
    S_ij = scale sum_k Q_ik K_jk  (causal: keys j <= i only)    LSE_i = ln sum_j exp(S_ij)    P_ij = exp(S_ij - LSE_i)    Y_ic = sum_j P_ij V_jc
    D_i = sum_c dY_ic Y_ic    dP_ij = sum_c dY_ic V_jc    dS_ij = P_ij (dP_ij - D_i)
    dV_jc = sum_i P_ij dY_ic    dQ_ik = scale sum_j dS_ij K_jk    dK_jk = scale sum_i dS_ij Q_ik

The stages and their bounds (u = 2^-24).
(a) score error: dS_ij = C_SUM (d + 2) u scale sum_k |Q_ik K_jk| - d products and additions and the scale, each rounded.
(b) |LSE - LSE64| <= max_j dS_ij + (ULP_EXP + C_SUM L + R RESC) u + 2 u |LSE64|.  The scores move the log-sum by at most their largest error; the terms
    exp(S_ij - m) carry ULP_EXP ulps and their sum L roundings (C_SUM L holds the additions and the terms' argument errors, 2 |x| e^x u <= 0.74 u each against a
    sum of at least 1); the log and the final sum m + ln l two roundings of |LSE|.  R is the number of online rescales of the row, ceil(keys / BK) - the kernel
    merges nothing across waves.
(c) |Y_ic - Y64_ic| <= (relP_i + C_SUM (L + 2) u) sum_j P64_ij |V_jc| + FLUSH,
    relP_i = expm1(2 max_j dS_ij) + (2 ULP_EXP + 2 (max_j S - min_j S) + L + R RESC) u: numerator and denominator of P each move by the score error and one exp, the
    exp's argument by its own size, the sum by L roundings.
(d) D_i within C_SUM (d + 4) u sum_c |dY_ic Y_ic|;  dV within sum_i (relP_ij + C_SUM (L + 4) u) P64_ij |dY_ic|;  dQ and dK within
    scale sum (relP_ij + C_SUM (L + 4) u + INNER) P64_ij (|dP|_ij + |D|_i) |K_jk| (resp. |Q_ik|), with |dP|_ij = sum_c |dY_ic V_jc| and |D|_i = sum_c |dY_ic Y_ic| in
    place of dP - D.  Here P64 = exp(S64 - LSE) from the STORED LSE, so relP_ij = expm1(dS_ij) + (ULP_EXP + 2 |S_ij - LSE_i|) u: (a) plus one __expf.

Two terms the four lines above needed in addition; each is derived here and named in the code:
  RESC   = ULP_EXP + 1 + 2 ln L per rescale.  A rescale multiplies the running sum l by alpha = exp(x), x = m_old - m_new <= 0: one exp and one product,
           ULP_EXP + 1 ulps - and the exp's ARGUMENT error 2 |x| u, which moves l_new = l e^x + (>= 1) by 2 |x| l e^x / (l e^x + 1) u relatively.  With t = |x|
           that is 2 t l / (l + e^t) u <= 2 ln(l) u <= 2 ln(L) u: for t <= ln l the fraction is below t, beyond it t l e^-t falls.
  INNER  = C_SUM (d + 2) u.  dS = P (dP - D) inherits the rounding of the two INNER sums over the d channels, each within C_SUM (d + 1) u of its absolute sum, and
           the subtraction's own; `terms` counts the outer sum alone.  Without it a row with a single key (dP = D exactly, so dS is nothing but that rounding) has
           no allowance at all once d exceeds L.
  FLUSH  = 2^-126 times the absolute sum of the other factors: a P below the smallest normal number is flushed to zero by __expf and the MFMA."""
import numpy as np

from f64_witness import C_SUM, TINY, U, ULP_EXP, W, check     # noqa: F401  (check: re-exported for the tests)


class WB(W):
    """a witness whose bound is given element by element"""

    def __init__(self, exact, bound):
        W.__init__(self, exact, 0.0, 0, 1.0)
        self.b = np.broadcast_to(np.asarray(bound, np.float64), self.exact.shape)

    def bound(self):
        return self.b


def scale_of(d):
    return float(np.float32(1.0 / np.sqrt(float(d))))


def resc(L):
    return ULP_EXP + 1.0 + 2.0 * np.log(max(L, 3))


def split(QKV, heads):
    """[N, L, 3E] -> float64 q, k, v, each [N, heads, L, d]"""
    a = np.asarray(QKV, np.float64); N, L, C = a.shape; d = C // 3 // heads
    t = a.reshape(N, L, 3, heads, d).transpose(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def to_heads(Y, heads):
    a = np.asarray(Y, np.float64); N, L, E = a.shape
    return a.reshape(N, L, heads, E // heads).transpose(0, 2, 1, 3)


def from_heads(y):
    N, H, L, d = y.shape
    return np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(N, L, H * d)


def live(L, causal):
    return np.tril(np.ones((L, L), bool)) if causal else np.ones((L, L), bool)


def scores(QKV, heads, causal):
    """(a): S64, dS, the live keys, v"""
    q, k, v = split(QKV, heads); d = q.shape[-1]; sc = scale_of(d)
    S = sc * (q @ k.transpose(0, 1, 3, 2))
    dS = C_SUM * (d + 2) * U * sc * (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2))
    return S, dS, live(q.shape[2], causal), (q, k, v, sc)


def rescales(L, BK, causal):
    """R per row: the key tiles the row's running sum passes through"""
    keys = np.arange(1, L + 1) if causal else np.full(L, L)
    return -(-keys // BK)


def fwd(QKV, heads, causal, BK):
    """(b) and (c) from the stored QKV: (LSE witness [N, heads, L], Y witness [N, L, E])"""
    S, dS, ok, (q, k, v, sc) = scores(QKV, heads, causal); L = S.shape[-1]
    Sm = np.where(ok, S, -np.inf); m = Sm.max(-1, keepdims=True)
    e = np.exp(Sm - m); l = e.sum(-1, keepdims=True); P = e / l
    lse = (m + np.log(l))[..., 0]
    mdS = np.where(ok, dS, 0.0).max(-1)
    R = rescales(L, BK, causal) * resc(L)                                       # [L], broadcasts over [N, heads, L]
    b_lse = mdS + (ULP_EXP + C_SUM * L + R) * U + 2.0 * U * np.abs(lse)
    spread = m[..., 0] - np.where(ok, S, np.inf).min(-1)
    relP = np.expm1(2.0 * mdS) + (2.0 * ULP_EXP + 2.0 * spread + L + R) * U
    av = np.abs(v)
    b_y = (relP[..., None] + C_SUM * (L + 2) * U) * (P @ av) + TINY * av.sum(-2, keepdims=True)
    return WB(lse, b_lse), WB(from_heads(P @ v), from_heads(np.broadcast_to(b_y, (P @ v).shape)))


def bwd(QKV, OK, DY, LSE, heads, causal):
    """(d) from the stored QKV, OK, DY and LSE: (D witness [N, heads, L], DQKV witness [N, L, 3E])"""
    S, dS, ok, (q, k, v, sc) = scores(QKV, heads, causal); L = S.shape[-1]; d = q.shape[-1]
    x = S - np.asarray(LSE, np.float64).reshape(S.shape[:3])[..., None]
    with np.errstate(over="ignore"):
        P = np.where(ok, np.exp(np.where(ok, x, 0.0)), 0.0)
    relP = np.where(ok, np.expm1(dS) + (ULP_EXP + 2.0 * np.abs(x)) * U, 0.0)
    dy = to_heads(DY, heads); y = to_heads(OK, heads); ady = np.abs(dy)
    D = (dy * y).sum(-1); aD = (ady * np.abs(y)).sum(-1)
    wD = WB(D, C_SUM * (d + 4) * U * aD + d * TINY)
    T = lambda a: a.transpose(0, 1, 3, 2)
    dP = dy @ T(v); adP = ady @ T(np.abs(v))
    dSg = P * (dP - D[..., None]); amag = adP + aD[..., None]
    outer = C_SUM * (L + 4) * U; inner = C_SUM * (d + 2) * U
    dV = T(P) @ dy
    bV = T((relP + outer) * P) @ ady + TINY * ady.sum(-2, keepdims=True)
    fac = (relP + outer + inner) * P * amag
    dQ = sc * (dSg @ k); bQ = sc * (fac @ np.abs(k)) + TINY * sc * (np.where(ok, amag, 0.0) @ np.abs(k))
    dK = sc * (T(dSg) @ q); bK = sc * (T(fac) @ np.abs(q)) + TINY * sc * (T(np.where(ok, amag, 0.0)) @ np.abs(q))
    N, H = q.shape[:2]
    pack = lambda a, b, c: np.stack([from_heads(a).reshape(N, L, H, d), from_heads(b).reshape(N, L, H, d), from_heads(c).reshape(N, L, H, d)], 2).reshape(N, L, 3 * H * d)
    return wD, WB(pack(dQ, dK, dV), pack(bQ, bK, bV))


def bwd_chain(QKV, OK, DY, LSE, heads, causal, BK):
    """DQKV against the END-TO-END float64 attention (torch's autograd of scaled_dot_product_attention on the stored QKV, upstream gradient the stored DY - the
    chain tests/test_attention_plan.py holds to torch at 1e-12): the exact value is that of the float64 Y and LSE, and the bound is (d) at the stored OK and
    LSE plus what (b) and (c) let those two move the result by:
      P = exp(S - LSE) from an LSE within b_lse of the float64 one moves by rl_i = expm1(b_lse_i) relatively;
      D_i = sum_c dY_ic Y_ic from a Y within b_y moves by bD_i = sum_c |dY_ic| b_y_ic;
      so dV moves by sum_i rl_i P_ij |dY_ic|, dS_ij = P_ij (dP_ij - D_i) by P_ij (rl_i (|dP|_ij + |D|_i) + (1 + rl_i) bD_i), dQ and dK by scale times that against |K|, |Q|."""
    wl, wy = fwd(QKV, heads, causal, BK)
    _, wg = bwd(QKV, wy.exact, DY, wl.exact, heads, causal)
    _, ws = bwd(QKV, OK, DY, LSE, heads, causal)
    S, dS, ok, (q, k, v, sc) = scores(QKV, heads, causal); N, H, L, d = q.shape
    P = np.where(ok, np.exp(np.where(ok, S - wl.exact[..., None], 0.0)), 0.0)
    rl = np.expm1(wl.bound())[..., None]
    dy = to_heads(DY, heads); ady = np.abs(dy)
    bD = (ady * to_heads(wy.bound(), heads)).sum(-1)[..., None]
    amag = ady @ np.abs(v).transpose(0, 1, 3, 2) + (ady * np.abs(to_heads(wy.exact, heads))).sum(-1)[..., None]
    eS = P * (rl * amag + (1.0 + rl) * bD)
    T = lambda a: a.transpose(0, 1, 3, 2)
    eV = T(rl * P) @ ady; eQ = sc * (eS @ np.abs(k)); eK = sc * (T(eS) @ np.abs(q))
    e = np.stack([from_heads(eQ).reshape(N, L, H, d), from_heads(eK).reshape(N, L, H, d), from_heads(eV).reshape(N, L, H, d)], 2).reshape(N, L, 3 * H * d)
    return WB(wg.exact, ws.bound() + e)


# ----------------------------------------------------------------------------- a float32 restatement of the tiled online algorithm (and three wrong ones)
def f32_attention(QKV, DY, heads, causal, BK=64, wrong=None):
    """the kernels' algorithm in NumPy float32: key tiles of BK, the running max / sum with the rescale of the running output per tile, np.exp in float32; the
    backward from its own stored LSE and Y.  wrong = "noscale" (the scale omitted), "strict" (the causal mask keeps j < i, not j <= i), "norescale" (the running
    output is not rescaled when the max rises).  Returns Y [N, L, E], LSE [N, heads, L], D [N, heads, L], DQKV [N, L, 3E], all float32."""
    a = np.asarray(QKV, np.float32); N, L, C = a.shape; E = C // 3; d = E // heads
    sc = np.float32(1.0) if wrong == "noscale" else np.float32(scale_of(d))
    t = a.reshape(N, L, 3, heads, d).transpose(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    ii = np.arange(L)[:, None]
    y = np.zeros((N, heads, L, d), np.float32); lse = np.zeros((N, heads, L), np.float32)
    with np.errstate(all="ignore"):
        for n in range(N):
            for h in range(heads):
                m = np.full(L, -np.inf, np.float32); l = np.zeros(L, np.float32); acc = np.zeros((L, d), np.float32)
                for k0 in range(0, L, BK):
                    jj = np.arange(k0, min(L, k0 + BK))[None, :]
                    s = (q[n, h] @ k[n, h, k0:k0 + BK].T).astype(np.float32) * sc
                    if causal:
                        s = np.where((jj < ii) if wrong == "strict" else (jj <= ii), s, np.float32(-np.inf))
                    mn = np.maximum(m, s.max(1))
                    seen = np.isfinite(mn)                                    # rows the tile (and every tile before it) holds no key of keep their state
                    alpha = np.where(np.isfinite(m), np.exp(m - mn, dtype=np.float32), np.float32(0.0))
                    p = np.where(seen[:, None], np.exp(s - np.where(seen, mn, 0)[:, None], dtype=np.float32), np.float32(0.0))
                    l = (l * alpha + p.sum(1, dtype=np.float32)).astype(np.float32)
                    pv = (p @ v[n, h, k0:k0 + BK]).astype(np.float32)
                    acc = (acc + pv if wrong == "norescale" else acc * alpha[:, None] + pv).astype(np.float32)
                    m = mn
                y[n, h] = acc / l[:, None]; lse[n, h] = m + np.log(l, dtype=np.float32)
        Y = np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(N, L, E)
        dy = np.asarray(DY, np.float32).reshape(N, L, heads, d).transpose(0, 2, 1, 3)
        D = (dy * y).sum(-1, dtype=np.float32)
        s = (q @ k.transpose(0, 1, 3, 2)).astype(np.float32) * sc
        keep = (ii > np.arange(L)[None, :]) if (causal and wrong == "strict") else live(L, causal)
        p = np.where(keep, np.exp(s - lse[..., None], dtype=np.float32), np.float32(0.0))
        dp = (dy @ v.transpose(0, 1, 3, 2)).astype(np.float32)
        ds = (p * (dp - D[..., None])).astype(np.float32)
        dv = (p.transpose(0, 1, 3, 2) @ dy).astype(np.float32)
        dq = (sc * (ds @ k)).astype(np.float32); dk = (sc * (ds.transpose(0, 1, 3, 2) @ q)).astype(np.float32)
    g = np.stack([dq, dk, dv], 0).transpose(1, 3, 0, 2, 4)                      # [3, N, heads, L, d] -> [N, L, 3, heads, d]
    return Y, lse, D, np.ascontiguousarray(g).reshape(N, L, 3 * E)


def ratios(QKV, DY, heads, causal, BK, Y, LSE, D, DQKV):
    """worst |got - exact| / bound of the four checked tensors, each stage from the operands stored in front of it: { "lse", "y", "d", "dqkv" }"""
    from f64_witness import ratio
    wl, wy = fwd(QKV, heads, causal, BK)
    wd, wg = bwd(QKV, Y, DY, LSE, heads, causal)
    return {"lse": ratio(LSE, wl)[0], "y": ratio(Y, wy)[0], "d": ratio(D, wd)[0], "dqkv": ratio(DQKV, wg)[0]}
