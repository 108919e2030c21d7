"""The case table of the optimizer sweep (tests/test_gpu_optim_sweep.py) and everything about it that needs no GPU: where every tensor of a
parameter table lies, which branch of k_opt_chunked (csrc/optim.hip) the pointers select, the `pad` prefix, the operands, a second honest
implementation of the update (NumPy float32, one rounding per line) and the checks every case is held to.  tests/test_optim_cases.py runs
all of it on the CPU - oracle against float64, NumPy against the oracle, the checks against injected defects - so the GPU half only has to
swap the implementation under test.  Not a test module."""
import numpy as np

import f64_witness as wt

# name -> (kind of the C ABI, lr, b1, b2, wd).  b1 = 0 is plain SGD: M is neither read nor written
KINDS = {"sgd0": (0, 0.01, 0.0, 0.0, 0.0), "sgdm": (0, 0.01, 0.9, 0.0, 0.0), "adam": (1, 1e-3, 0.9, 0.999, 0.0), "adamw": (2, 1e-3, 0.9, 0.999, 0.01)}
EPS = np.float32(1.0e-6)                     # DU_EPS
CHUNK = 1024                                 # elements per workgroup of k_opt_chunked, per chunk-half workgroup of k_opt_step
# one table: a tensor below one 16-byte vector; tensors whose last vector thread straddles the end (3, 5, 1023, 1025, ...); the end of the
# first chunk and a second chunk with a ragged tail; an EMPTY record between two others (it shares its `pad` with the next); a small one behind it
SIZES = (1, 3, 4, 5, 1020, 1023, 1024, 1025, 2047, 2049, 3000, 0, 7)
NW = tuple(1 + i % 3 for i in range(len(SIZES)))
STEPS = 3
MOAT = 64                                    # NaN floats in front of and behind every allocation
TENSORS = ("G", "DG", "M", "V")

# layout -> offset in floats of each tensor inside its own (256-byte aligned, NaN-moated) allocation
LAYOUTS = {
    "aligned":    dict(G=0, DG=0, M=0, V=0),
    "g_off4":     dict(G=1, DG=0, M=0, V=0),
    "dg_off4":    dict(G=0, DG=1, M=0, V=0),
    "m_off4":     dict(G=0, DG=0, M=1, V=0),
    "v_off4":     dict(G=0, DG=0, M=0, V=1),
    "all_off8":   dict(G=2, DG=2, M=2, V=2),
    "host_alias": dict(G=0, DG=0, M=0, V=0),  # + the host's aliasing (host/model.cpp grad_alloc / build_table): M = V = G for sgd0, V = M for sgdm
}
# the branch the INTERIOR threads (jv + 3 < n) of each record take: optim.hip ORs all four pointers of the record whatever the kind reads, so
# one tensor 4 bytes in sends the whole record element by element.  Threads at a ragged end are scalar in every layout.
_V, _S = ("vec",) * len(SIZES), ("scalar",) * len(SIZES)
BRANCH = {"aligned": _V, "g_off4": _S, "dg_off4": _S, "m_off4": _S, "v_off4": _S, "all_off8": _S, "host_alias": _V}


def branch_of(G, DG, M, V, keep_src=0, keep_dst=0):
    """what `const bool vec = ...` of k_opt_chunked decides from the pointers' low bits (the `jv + 3 < r.n` half is the thread's, not the record's)"""
    return "vec" if ((G | DG | M | V | (keep_dst if G == keep_src else 0)) & 15) == 0 else "scalar"


def pads(sizes):
    """(first chunk of every record, chunks in all): the prefix the caller of t4k_opt_chunked fills in"""
    out, c = [], 0
    for n in sizes:
        out.append(c); c += (n + CHUNK - 1) // CHUNK
    return out, c


class Plan:
    """where the tensors of a table lie in ONE buffer of floats (the base 256-byte aligned): rec[i][t] = (start, n) of tensor t of record i; tensors
    that alias share a start.  own = the (record, tensor) pairs that have an allocation of their own; moats = every float that belongs to no tensor."""

    def __init__(self, sizes, layout, kname, extra=()):
        off = LAYOUTS[layout]; alias = layout == "host_alias"
        self.sizes, self.rec, self.own, pos = tuple(sizes), [], [], 0
        for i, n in enumerate(sizes):
            r = {}
            for t in TENSORS:
                if alias and ((kname == "sgd0" and t in ("M", "V")) or (kname == "sgdm" and t == "V")):
                    r[t] = r["G"] if kname == "sgd0" else r["M"]
                    continue
                r[t] = (pos + MOAT + off[t], n); self.own.append((i, t))
                pos += (MOAT + off[t] + n + MOAT + 63) // 64 * 64          # the next allocation starts on 256 bytes again
            self.rec.append(r)
        self.extra = {}
        for name, n, o in extra:                                            # further allocations (snapshot destinations): name, floats, offset
            self.extra[name] = (pos + MOAT + o, n); pos += (MOAT + o + n + MOAT + 63) // 64 * 64
        self.total = pos
        self.moat = np.ones(pos, bool)
        for i, t in self.own:
            s, n = self.rec[i][t]; self.moat[s:s + n] = False
        for s, n in self.extra.values():
            self.moat[s:s + n] = False

    def view(self, buf, i, t):
        s, n = self.rec[i][t]
        return buf[s:s + n]

    def pointers(self, base, i):
        return tuple(base + 4 * self.rec[i][t][0] for t in TENSORS)

    def table(self, base, sizes=None, nw=NW):
        """the records as the C ABI lays them out (t4k_param_rec: four pointers, long n, int Nw, int pad), and the chunk total"""
        import struct
        sizes = self.sizes if sizes is None else sizes
        pad, chunks = pads(sizes)
        raw = b"".join(struct.pack("<QQQQqii", *self.pointers(base, i), sizes[i], nw[i % len(nw)], pad[i]) for i in range(len(sizes)))
        return raw, chunks


# ----------------------------------------------------------------------------- operands
def operands(rng, n):
    """(w, dg, m, v) of one tensor: unit-scale weights and gradients, moments a tenth of that; element 5 of every tensor (and every 77th behind it) has
    dg = 0 AND v = 0, so v' = 0 and Adam divides by eps alone; every 7th v and every 11th dg is 0 on its own"""
    w = rng.standard_normal(n).astype(np.float32); dg = fresh_gradient(rng, n)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32); v = (np.abs(rng.standard_normal(n)) * 0.1).astype(np.float32)
    v[5::7] = 0.0
    return w, dg, m, v


def fresh_gradient(rng, n):
    dg = rng.standard_normal(n).astype(np.float32)
    dg[5::11] = 0.0
    return dg


# gradients at the edges of the arithmetic: d * d underflows (1e-30), overflows (1e20), d itself is subnormal (1e-45), infinite, NaN
SPECIAL_N = 1024
_SG = [0.0, -0.0] + [s * x for x in (1e-45, 1e-30, 1e-19, 1.0, 1e19, 1e20, np.inf) for s in (1.0, -1.0)] + [np.nan]
_SM = [0.0, 1e-38, 1.0, 1e30]
_SW = [0.0, 1.0, -1.0, 1e30, -1e30]


def specials():
    """(w, dg, m, v): 17 gradients x 4 moments x 5 weights are pairwise coprime, so 340 elements hold every combination of one gradient with one
    moment and one weight; v runs one place behind m so that the two moments differ"""
    j = np.arange(SPECIAL_N)
    with np.errstate(over="ignore"):
        g = np.array(_SG, np.float64).astype(np.float32); m = np.array(_SM, np.float64).astype(np.float32); w = np.array(_SW, np.float64).astype(np.float32)
    return w[j % 5].copy(), g[j % 17].copy(), m[j % 4].copy(), m[(j + 1) % 4].copy()


# ----------------------------------------------------------------------------- the update in NumPy float32, one rounding per line (sgd1 / adam1 / adamw1)
DEFECTS = ("wd_times_m", "eps_inside_root", "v_from_d", "momentum_not_stored", "gradient_not_zeroed", "dg_over_batch", "last_three_skipped",
           "snapshot_after_update")
BATCH = 128                                  # what `dg_over_batch` divides by


def np_step(kname, w, dg, m, v, Nw, defect=None):
    """one step on copies: (w', dg', m', v', snapshot of w).  m / v come back untouched where the kind does not write them."""
    kind, lr, b1, b2, wd = KINDS[kname]
    f = np.float32; lr, b1, b2, wd = f(lr), f(b1), f(b2), f(wd); one = f(1.0)
    w0, dg0, m0, v0 = (np.array(a, np.float32, copy=True) for a in (w, dg, m, v))
    keep = w0.copy()
    with np.errstate(all="ignore"):
        if kind == 0:
            d = dg0 / f(BATCH if defect == "dg_over_batch" else Nw)
            if abs(b1) < EPS:
                t = lr * d
                w1, m1 = w0 - t, m0
            else:
                a = b1 * m0
                c = one - b1
                e = c * d
                m1 = a + e
                t = lr * m1
                w1 = w0 - t
            v1 = v0
        else:
            d = dg0
            a = b1 * m0
            c = one - b1
            e = c * d
            m1 = a + e
            a2 = b2 * v0
            c2 = one - b2
            e2 = c2 * d
            e3 = e2 if defect == "v_from_d" else e2 * d
            v1 = a2 + e3
            if defect == "eps_inside_root":
                den = np.sqrt(v1 + EPS)
            else:
                r = np.sqrt(v1)
                den = r + EPS
            if kind == 1:
                num = lr * m1
                q = num / den
                w1 = w0 - q
            else:
                q = m1 / den
                dec = wd * (m1 if defect == "wd_times_m" else d)
                u = q - dec
                t = lr * u
                w1 = w0 - t
    dg1 = dg0.copy() if defect == "gradient_not_zeroed" else np.zeros_like(dg0)
    if defect == "momentum_not_stored":
        m1 = m0
    if defect == "last_three_skipped":
        k = max(0, w0.size - 3)
        w1[k:], dg1[k:] = w0[k:], dg0[k:]
        if m1 is not m0: m1[k:] = m0[k:]
        if v1 is not v0: v1[k:] = v0[k:]
    if defect == "snapshot_after_update":
        keep = w1.copy()
    return w1, dg1, m1, v1, keep


def oracle_step(oracle, kname, w, dg, m, v, Nw):
    """the same step by the CPU oracle (t4o_sgd / t4o_adam / t4o_adamw), on copies"""
    o = oracle.lib(); P = oracle.P
    kind, lr, b1, b2, wd = KINDS[kname]
    w, dg, m, v = (np.array(a, np.float32, copy=True) for a in (w, dg, m, v)); n = w.size
    if n:
        if kind == 0: o.t4o_sgd(P(w), P(dg), P(m), Nw, lr, b1, n)
        elif kind == 1: o.t4o_adam(P(w), P(dg), P(m), P(v), lr, b1, b2, n)
        else: o.t4o_adamw(P(w), P(dg), P(m), P(v), lr, b1, b2, wd, n)
    return w, dg, m, v


def witness(kname, w, dg, m, v, Nw):
    """float64 witnesses (w, m or None, v or None) of f64_witness, bounds as they stand"""
    kind, lr, b1, b2, wd = KINDS[kname]
    if kind == 0: return wt.sgd(w, dg, m, Nw, lr, b1) + (None,)
    if kind == 1: return wt.adam(w, dg, m, v, lr, b1, b2)
    return wt.adamw(w, dg, m, v, lr, b1, b2, wd)


# ----------------------------------------------------------------------------- the checks
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(name, got, want):
    """bit-for-bit, NaN payloads and the sign of zero included; the first differing element"""
    g, w = bits(got).ravel(), bits(want).ravel()
    assert g.size == w.size, "%s: %d elements, want %d" % (name, g.size, w.size)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d elements differ, first [%d] got %r (0x%08x) want %r (0x%08x)" % (
        name, bad.size, g.size, bad[0], float(np.ravel(got)[bad[0]]), g[bad[0]], float(np.ravel(want)[bad[0]]), w[bad[0]])


def same_values(name, got, want):
    """bit-for-bit except that any NaN stands for any NaN (the payload and sign of a NaN that an operation PRODUCES are the implementation's)"""
    g, w = np.ravel(np.asarray(got, np.float32)), np.ravel(np.asarray(want, np.float32))
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), "%s: NaN at other places, first [%d]" % (name, np.flatnonzero(np.isnan(g) != nan)[0])
    same_bits(name, np.where(nan, np.float32(0), g), np.where(nan, np.float32(0), w))


def ulps(a, b):
    """(elements that differ, worst distance in units of the last place) between two finite fp32 tensors"""
    def key(x):
        i = bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    d = np.abs(key(a) - key(b))
    return int((d != 0).sum()), int(d.max()) if d.size else 0


def check_record(name, kname, ini, got, orc, Nw, aliased=(), report="optimizer sweep"):
    """one record after one step.  ini / got / orc = (w, dg, m, v): what was uploaded, what the implementation left, what the oracle left from the
    same operands.  aliased: the tensors of (M, V) that are no tensor of their own in this layout (got holds the operands there).
      DG all +0; W, M, V inside the float64 witness on the operands uploaded; W, M and V the oracle's bits; a tensor the kind does not write bit-equal
      to what was uploaded."""
    kind, lr, b1, b2, wd = KINDS[kname]
    ww, wm, wv = witness(kname, *ini, Nw)
    assert not bits(got[1]).any(), "%s: DG is not all +0" % name
    wt.check(name + " w", got[0], ww, kind=report + " w"); wt.check("oracle " + name + " w", orc[0], ww)
    if wm is not None:
        wt.check(name + " m", got[2], wm, kind=report + " m"); same_bits(name + " m vs oracle", got[2], orc[2])
    elif "M" not in aliased:
        same_bits(name + " m (plain SGD leaves it alone)", got[2], ini[2])
    if wv is not None:
        wt.check(name + " v", got[3], wv, kind=report + " v"); same_bits(name + " v vs oracle", got[3], orc[3])
    elif "V" not in aliased:
        same_bits(name + " v (SGD leaves it alone)", got[3], ini[3])
    same_bits(name + " w vs oracle", got[0], orc[0])                       # every kind: the root of Adam / AdamW is the correctly rounded one


# ----------------------------------------------------------------------------- the tables of the t4k_opt_step cases
# Built on CASES[case] of tests/test_gpu_conv_stack.py: "F<s>" / "B<s>" are the stack's filter and bias records (the tensors a deferred backward leaves to the
# fold half), ("x", n) a plain tensor of n elements (the chunk half), ("one", k) k records of one element each.  what: "fold" - the fold rides in the update, 2
# launches; otherwise the reason t4k_opt_step must refuse it, flush the fold on its own and run the plain step (3 launches).
def fold_order(nstage, shape):
    stack = [t + str(s) for s in range(nstage) for t in ("F", "B")]
    if shape in ("spread", "missing", "short", "null_host"):
        out = [("x", 3000), stack[0], ("x", 5)] + stack[1:] + [("x", 1025)]           # skip bits 1, 3, 4, ...: no prefix, a plain tensor between two folded ones
        if shape == "missing":
            out.remove("F0")
        return out
    if shape in ("rec63", "rec65"):
        return stack[:-1] + [("one", (64 if shape == "rec63" else 65) - len(stack))] + stack[-1:]   # the last bias is record 63 (bit 63 of skip) / 64
    raise KeyError(shape)


FOLD_TABLES = [("spread-0", 0, "spread", "fold"), ("spread-2", 2, "spread", "fold"), ("spread-3", 3, "spread", "fold"), ("rec63", 3, "rec63", "fold"),
               ("rec65", 3, "rec65", "65 records"), ("missing", 3, "missing", "a folded tensor is not in the table"),
               ("short", 3, "short", "a folded tensor's n is one less than the segment's"), ("null-host", 3, "null_host", "tab_host = NULL")]
