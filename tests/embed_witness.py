"""Witnesses of the embedding layer (include/t4k.h t4k_embed_*): the rule in float64, the plan's rule in Python's unbounded integers, and a
float32 restatement of the kernels' summation order.

The rule.  T = N L tokens of E floats, t = n L + l.  Token mode (V >= 1): the ids are floats; valid(t) <=> x_t >= 0 and x_t < V in float32 compares, id_t =
(int)x_t (truncation), formed only where valid; out[t] = (valid ? TABLE[id_t] : 0) + (pos ? POS[l] : 0).  Position mode (V = 0): out[t] = x[t] + POS[l].
dTABLE[v] += sum of dY[t] over the valid t with id_t = v; dPOS[l] += sum over n of dY[n L + l].

The forward is at most one fp32 add, so its witness is the float32 restatement itself, bit for bit (`fwd32`).

The gradient bound, derived, not measured: a sum of n terms in ANY fp32 order carries at most n - 1 roundings, each at most u = 2^-24 of a partial sum that is
itself at most sum |terms| (1 + O(n u)): |err| <= (n - 1) u sum |terms| to first order.  C_SUM = 2 of f64_witness.py is the allowance for the higher orders, as
in an_witness.py / attn_witness.py.  For a table row the terms are the dY rows that name it (its hit count h) and the prior DTABLE value: n = h + 1, so h
roundings; h = 0 asks for the prior bits.  For dPOS the terms are the N samples and the prior value: N roundings (the zeros a thread starts from add none).
"""
import numpy as np

from f64_witness import C_SUM, U, W, check, ratio     # noqa: F401  (re-exported for the tests)

F = np.float32
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -4
R_SLAB, UNITS, PART_MIN, PI = 16, 1024, 64, 16     # table rows of a slab, wave units the scatter spreads over, tokens a part holds at least, dPOS items | groups


def cdiv(a, b):
    return -(-a // b)


def valid_ids(ids, V, wrong=None):
    """(valid [T] bool, id [T] int64; 0 where not valid).  wrong: "round" rounds to nearest instead of truncating; "pad_row0" counts padding as id 0"""
    x = np.asarray(ids, F).ravel()
    with np.errstate(invalid="ignore"):
        ok = (x >= F(0)) & (x < F(V))
    idv = np.where(ok, x, F(0))
    idv = (np.rint(idv) if wrong == "round" else np.trunc(idv)).astype(np.int64)
    if wrong == "round":
        idv = np.minimum(idv, V - 1)
    ok = ok & (idv < V)
    if wrong == "pad_row0":
        ok = np.ones_like(ok)
    return ok, np.where(ok, idv, 0)


def pos_index(T, L, wrong=None):
    t = np.arange(T)
    return np.minimum(t, L - 1) if wrong == "pos_t" else t % L


def fwd32(src, table, pos, T, L, V, E, wrong=None):
    """the forward in NumPy float32: src = the ids [T] (V >= 1) or x [T, E] (V = 0); table [V, E] | None; pos [L, E] | None"""
    if V >= 1:
        ok, idv = valid_ids(src, V, wrong)
        out = np.where(ok[:, None], np.asarray(table, F).reshape(V, E)[idv], F(0)).astype(F)
    else:
        out = np.asarray(src, F).reshape(T, E).copy()
    if pos is not None:
        out = (out + np.asarray(pos, F).reshape(L, E)[pos_index(T, L, wrong)]).astype(F)
    return out


def fwd64(src, table, pos, T, L, V, E):
    """the rule in float64, written independently of fwd32: a loop over the tokens"""
    out = np.zeros((T, E), np.float64)
    x = np.asarray(src, np.float64).reshape(T, -1)
    for t in range(T):
        if V >= 1:
            v = float(F(x[t, 0]))
            if v >= 0 and v < float(F(V)) and int(v) < V:
                out[t] = np.asarray(table, np.float64).reshape(V, E)[int(v)]
        else:
            out[t] = x[t]
        if pos is not None:
            out[t] = out[t] + np.asarray(pos, np.float64).reshape(L, E)[t % L]
    return out


def em_dtable(ids, DY, DT0, V, E, train=1):
    """witness of DTABLE after the backward: prior + the sum of the dY rows that name the row; n = the row's hit count"""
    DT0 = np.asarray(DT0, np.float64).reshape(V, E)
    if not train:
        return W(DT0, 0.0, 0)
    ok, idv = valid_ids(ids, V)
    dy = np.asarray(DY, np.float64).reshape(-1, E)
    ex, mag, hits = DT0.copy(), np.abs(DT0), np.zeros(V)
    np.add.at(ex, idv[ok], dy[ok]); np.add.at(mag, idv[ok], np.abs(dy[ok])); np.add.at(hits, idv[ok], 1.0)
    return W(ex, mag, np.broadcast_to(hits[:, None], (V, E)))


def em_dpos(DY, DP0, T, L, E, train=1):
    DP0 = np.asarray(DP0, np.float64).reshape(L, E)
    if not train:
        return W(DP0, 0.0, 0)
    dy = np.asarray(DY, np.float64).reshape(T // L, L, E)
    return W(DP0 + dy.sum(0), np.abs(DP0) + np.abs(dy).sum(0), T // L)


def expect(T, L, V, E, pos, aligned, ws):
    """t4k_embed_plan's rule in unbounded integers: out[8], or the refusal's code"""
    if T < 1 or L < 1 or E < 1 or V < 0 or T % L or ws < 0 or pos not in (0, 1) or (V == 0 and pos == 0):
        return ERR_ARG
    if T >= 1 << 31 or T * E >= 1 << 31 or V * E >= 1 << 31:
        return ERR_UNSUPPORTED
    vw = 4 if aligned and E % 4 == 0 else 1
    items = E // vw
    pwg = cdiv(L * items, PI) if pos else 0
    if V == 0:
        return [0, vw, 0, 1, 1, 1, pwg, 0]
    base, nbytes = cdiv(V, R_SLAB) * cdiv(items, 64), 4 * V * E
    P = max(1, min(cdiv(UNITS, base), max(1, T // PART_MIN), min(ws, (1 << 31) - 1) // nbytes))
    per = cdiv(cdiv(T, 64), P) * 64
    P = cdiv(T, per)
    rung = 2 if P > 1 else 1
    return [rung, vw, R_SLAB, P, 1, rung, cdiv(base * P, 4) + pwg, P * nbytes if P > 1 else 0]


def part_len(T, P):
    """tokens of a part, from the plan's P"""
    return cdiv(cdiv(T, 64), P) * 64 if P > 1 else T


def bwd32(ids, DY, DT0, DP0, T, L, V, E, P, wrong=None):
    """the backward's order in NumPy float32.  Token mode: a part's tokens in ascending order onto zeroed rows (slab and chunk ownership changes no element's
    order); P = 1 adds the rows onto DTABLE, P > 1 adds the parts in order first; an element whose sum is exactly 0 is not written.  dPOS: 16 groups of
    ceil(N / 16) samples each from 0 in ascending order, the groups added in order, then onto DPOS.  Returns (DTABLE | None, DPOS | None)"""
    dy = np.asarray(DY, F).reshape(T, E)
    DT = DP = None
    if V >= 1:
        ok, idv = valid_ids(ids, V, wrong)
        per = part_len(T, P)
        parts = []
        for q in range(P):
            acc = np.zeros((V, E), F)
            for t in range(q * per, min(T, (q + 1) * per)):
                if ok[t]:
                    acc[idv[t]] = acc[idv[t]] + dy[t]
            parts.append(acc)
        s = parts[0]
        for q in range(1, P):
            s = (s + parts[q]).astype(F)
        D0 = np.asarray(DT0, F).reshape(V, E)
        DT = np.where(s != 0, (D0 + s).astype(F), D0)
    if DP0 is not None:
        N = T // L
        nper = cdiv(N, PI)
        d3 = dy.reshape(N, L, E)
        if wrong == "pos_t":                                               # the gradient of a position indexed by t: everything past L - 1 lands there
            d3 = np.zeros((N, L, E), F); idx = pos_index(T, L, wrong)
            tmp = np.zeros((L, E), np.float64); np.add.at(tmp, idx, dy.astype(np.float64))
            d3[0] = tmp.astype(F)
        a = None
        for g in range(PI):
            sg = np.zeros((L, E), F)
            for n in range(g * nper, min(N, (g + 1) * nper)):
                sg = (sg + d3[n]).astype(F)
            a = sg if a is None else (a + sg).astype(F)
        DP = (np.asarray(DP0, F).reshape(L, E) + a).astype(F)
    return DT, DP


def make_ids(rng, T, V, kind="mixed"):
    """float ids.  "frac": k + 0.75 (truncation shows); "mixed": in range with padding values mixed in; "plain": integers in range"""
    k = rng.integers(0, V, T).astype(F)
    if kind == "frac":
        return (k + F(0.75)).astype(F)
    if kind == "mixed":
        pad = np.array([-1.0, -0.5, V, 1e9, np.nan, np.inf, -np.inf], F)
        m = rng.random(T) < 0.25
        k = np.where(m, pad[rng.integers(0, len(pad), T)], k).astype(F)
    return k
