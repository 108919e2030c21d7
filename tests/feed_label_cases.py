"""The feed, label and hit-count kernels: k_stage_batch, k_u8norm, k_onehot (csrc/elementwise.hip) and k_hit<1|8|64> (csrc/reduce.hip, behind t4k_hit and
t4k_onehot_hit).  The mirrors of their launch code, the witnesses in numpy (written from the reference's text, not from the oracle) and the case tables, each row
sized by an inequality of the launch code.  tests/test_feed_label_cases.py holds the witnesses to the oracle and the tables to injected defects on the CPU,
tests/test_gpu_feed_label_sweep.py runs every case through the C ABI.  Every check is bit-exact.  Imports neither torch nor the product."""
import zlib

import numpy as np

# ---------------------------------------------------------------- mirrors (csrc/t4k_common.h, reduce.hip, elementwise.hip)
BLK = 256                 # threads of a workgroup
MAX_WG = 2048             # grid_for() caps the grid here: a kernel that does not stride stops at CAP threads
CAP = BLK * MAX_WG        # 524 288
FLT_MAX = np.float32(3.4028234663852886e38)
NAN, INF = np.float32(np.nan), np.float32(np.inf)
ALL_ONES = 0xFFFFFFFF


def hit_lanes(E):
    """lanes that share a row of k_hit: t4k_hit picks k_hit<1> up to 32 classes, k_hit<8> up to 256, k_hit<64> above"""
    return 1 if E <= 32 else (8 if E <= 256 else 64)


def hit_trip(E):
    """rows one pass of the single workgroup takes"""
    return BLK // hit_lanes(E)


def stage_vec(src_addr, dst_addr):
    """t4k_stage_batch: four pixels to a lane when the bytes can be read as a word and the floats stored as a float4"""
    return src_addr % 4 == 0 and dst_addr % 16 == 0


def grid_for(n, per_thread=1):
    g = (n + BLK * per_thread - 1) // (BLK * per_thread)
    return max(1, min(g, MAX_WG))


# ---------------------------------------------------------------- witnesses
def argmax(out):
    """Model::hit's scan, row by row: m = o[0], i = 0, then o[e] > m takes e.  A NaN at o[0] is never displaced, a NaN behind it never taken."""
    out = np.asarray(out, np.float32)
    N, E = out.shape
    m, i = out[:, 0].copy(), np.zeros(N, np.int64)
    with np.errstate(invalid="ignore"):
        for e in range(1, E):
            t = out[:, e] > m
            m, i = np.where(t, out[:, e], m), np.where(t, e, i)
    return i


def count(hot, idx):
    """sum of (int)hot[n, idx[n]]: C truncation towards zero, 32-bit sum"""
    hot = np.asarray(hot, np.float32)
    v = np.trunc(hot[np.arange(hot.shape[0]), idx].astype(np.float64)).astype(np.int64)
    return int(np.int64(v.sum()).astype(np.int32))


def hit(out, hot):
    return count(hot, argmax(out)) if np.asarray(out).shape[0] else 0


def onehot(label, N, E):
    label = np.asarray(label, np.uint32)[:N]
    hot = np.zeros((N, E), np.float32)
    hot[np.arange(N), np.where(label < E, label, 0).astype(np.int64)] = 1.0
    return hot


def normalize(u8, mean, scale):
    """(float(x) - mean) * scale: one float32 subtraction, one float32 multiplication - two roundings, nothing fused"""
    return (np.asarray(u8, np.uint8).astype(np.float32) - np.float32(mean)) * np.float32(scale)


def stage(u8, mean, scale, lab):
    return normalize(u8, mean, scale), np.array(lab, np.uint32, copy=True)


# ---------------------------------------------------------------- injected defects (tests/test_feed_label_cases.py)
def _scan(out, start, idx0, take):
    N, E = out.shape
    m, i = np.full(N, start, np.float32), np.full(N, idx0, np.int64)
    with np.errstate(invalid="ignore"):
        for e in range(E):
            t = take(out[:, e], m)
            m, i = np.where(t, out[:, e], m), np.where(t, e, i)
    return np.where(i >= E, 0, i)


def defect_hit_from_flt_max(out, hot):
    """the kernel in front of this sweep: every lane starts at -FLT_MAX with no index, and no index means class 0"""
    return count(hot, _scan(np.asarray(out, np.float32), -FLT_MAX, 0x7fffffff, lambda v, m: v > m)) if len(out) else 0


def defect_hit_higher_tie(out, hot):
    out = np.asarray(out, np.float32)
    if not len(out):
        return 0
    N, E = out.shape
    m, i = out[:, 0].copy(), np.zeros(N, np.int64)
    with np.errstate(invalid="ignore"):
        for e in range(1, E):
            t = out[:, e] >= m
            m, i = np.where(t, out[:, e], m), np.where(t, e, i)
    return count(hot, i)


def defect_hit_first_trip(out, hot):
    out = np.asarray(out, np.float32)
    k = min(len(out), hit_trip(out.shape[1]))
    return hit(out[:k], np.asarray(hot)[:k])


def defect_hit_tail_lanes(out, hot):
    """a row whose width is no multiple of G: the lanes from E % G on see nothing"""
    out = np.asarray(out, np.float32)
    if not len(out):
        return 0
    E = out.shape[1]; G = hit_lanes(E); r = E % G
    if r == 0:
        return hit(out, hot)
    seen = out.copy(); seen[:, (np.arange(E) % G) >= r] = -INF
    return count(hot, _scan(seen, -INF, 0x7fffffff, lambda v, m: v > m))


def defect_hit_rounds(out, hot):
    if not len(out):
        return 0
    hot = np.asarray(hot, np.float32)
    return int(np.rint(hot[np.arange(len(hot)), argmax(out)].astype(np.float64)).sum())


def defect_onehot_no_clamp(label, N, E):
    label = np.asarray(label, np.uint32)[:N]
    hot = np.zeros((N, E), np.float32)
    ok = label < E
    hot[np.arange(N)[ok], label[ok].astype(np.int64)] = 1.0
    return hot


def defect_normalize_distributed(u8, mean, scale):
    return np.asarray(u8, np.uint8).astype(np.float32) * np.float32(scale) - np.float32(mean) * np.float32(scale)


def defect_stage_labels_stop_at_cap(u8, mean, scale, lab, prefill, vec):
    out = np.array(lab, np.uint32, copy=True)
    out[CAP:] = prefill
    return normalize(u8, mean, scale), out


def defect_stage_swapped_bytes(u8, mean, scale, lab, prefill, vec):
    u8 = np.array(u8, np.uint8, copy=True)
    if vec:
        w = u8[:(u8.size >> 2) << 2].reshape(-1, 4)
        w[:, [1, 2]] = w[:, [2, 1]]
    return normalize(u8, mean, scale), np.array(lab, np.uint32, copy=True)


# ---------------------------------------------------------------- the case tables
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


class Case:
    """a named row; build() makes its operands (the same arrays every time)"""

    def __init__(self, name, make, **kw):
        self.name, self._make = name, make
        self.__dict__.update(kw)

    def build(self):
        return self._make()

    def __repr__(self):
        return self.name


def _ties_out(rng, N, E):
    return rng.integers(-3, 4, (N, E)).astype(np.float32)            # small integers: ties in every row


def _hot_of(idx, E, keep=None):
    """one-hot rows at idx; rows where keep is False point one class further"""
    idx = np.asarray(idx, np.int64)
    if keep is not None:
        idx = np.where(keep, idx, (idx + 1) % E)
    hot = np.zeros((len(idx), E), np.float32)
    hot[np.arange(len(idx)), idx] = 1.0
    return hot


def _lanes_case(E, N=37):
    def make():
        rng = _rng("lanes %d" % E)
        out = _ties_out(rng, N, E)
        odd = np.arange(1, N, 2)
        out[odd, rng.integers(0, E, odd.size)] = 9.0                          # every second row: one maximum, anywhere in the row
        return out, _hot_of(argmax(out), E, keep=np.arange(N) % 3 != 0) if E > 1 else np.ones((N, 1), np.float32)
    return Case("lanes-E%d" % E, make, E=E, N=N, kind="lanes")


def _trip_case(E, N):
    def make():
        rng = _rng("trip %d %d" % (E, N))
        out = _ties_out(rng, N, E)
        return out, _hot_of(argmax(out), E, keep=np.arange(N) % 3 != 0)      # two rows of three count, in every trip
    return Case("trip-G%d-N%d" % (hit_lanes(E), N), make, E=E, N=N, kind="trip")


def _maxpos_case(E):
    def make():
        out = _rng("maxpos %d" % E).uniform(-1.0, 0.0, (E, E)).astype(np.float32)
        out[np.arange(E), np.arange(E)] = 1.0 + np.arange(E, dtype=np.float32) / 1024.0
        perm = np.arange(E)
        a = np.arange(0, E - 1, 4)
        perm[a], perm[a + 1] = a + 1, a                                      # a fixed permutation: half the rows count
        return out, _hot_of(perm, E)
    return Case("maxpos-E%d" % E, make, E=E, N=E, kind="maxpos")


def tie_pairs(E, among=None):
    cols = list(range(E)) if among is None else list(among)
    return [(i, j) for a, i in enumerate(cols) for j in cols[a + 1:]]


def _tie_case(E, among=None):
    pairs = tie_pairs(E, among)

    def make():
        out = _rng("ties %d" % E).uniform(-2.0, -1.0, (len(pairs), E)).astype(np.float32)
        i, j = np.array(pairs).T
        out[np.arange(len(pairs)), i] = 3.0; out[np.arange(len(pairs)), j] = 3.0
        return out, _hot_of(i, E)                                            # the lower index counts, the higher one gives 0
    return Case("ties-E%d" % E, make, E=E, N=len(pairs), kind="ties", pairs=pairs)


def special_rows(E):
    """name -> (row, the class the reference picks), E >= 8"""
    ramp = (np.arange(E, dtype=np.float32) % 7.0) - 3.0
    rows = {}
    r = ramp.copy(); r[0] = NAN; r[E // 2] = 50.0
    rows["lead-nan"] = (r, 0)
    r = ramp.copy(); r[E // 2] = NAN; r[E - 1] = NAN; r[E - 2] = 60.0; r[1] = 59.0
    rows["nan-mid-end"] = (r, E - 2)
    rows["all-nan"] = (np.full(E, NAN, np.float32), 0)
    rows["all-ninf"] = (np.full(E, -INF, np.float32), 0)
    r = np.full(E, -INF, np.float32); r[E - 1] = -FLT_MAX
    rows["ninf-then-fltmax"] = (r, E - 1)
    r = np.full(E, -INF, np.float32); r[0] = -FLT_MAX
    rows["fltmax-then-ninf"] = (r, 0)
    a, b = {1: (3, 6), 8: (9, 16), 64: (65, 128)}[hit_lanes(E)]              # a < b with b in the lower lane
    r = ramp.copy(); r[a] = INF; r[b] = INF
    rows["pinf-twice"] = (r, a)
    r = np.full(E, -1.0, np.float32); r[a] = -0.0; r[b] = 0.0
    rows["zero-signs"] = (r, a)
    r = np.full(E, -1e-40, np.float32); r[a] = 0.0; r[b] = 1e-45; r[E - 1] = -1e-45
    rows["subnormals"] = (r, b)
    return rows


def _special_case(E, name):
    def make():
        row, want = special_rows(E)[name]
        rng = _rng("special %d %s" % (E, name))
        out = rng.uniform(-1.0, 1.0, (3, E)).astype(np.float32)
        out[1] = row
        idx = argmax(out)
        assert idx[1] == want, (name, E, idx[1], want)
        return out, _hot_of(idx, E)                                           # 3 when every row finds the reference's class
    return Case("special-E%d-%s" % (E, name), make, E=E, N=3, kind="special", special=name)


HOT_VALUES = [2.0, 0.9, -0.5, -1.0, 3.99]                                     # (int): 2, 0, 0, -1, 3


def _hotvals_case(E):
    def make():
        rng = _rng("hotvals %d" % E)
        out = rng.uniform(-1.0, 1.0, (10, E)).astype(np.float32)
        hot = rng.uniform(5.0, 9.0, (10, E)).astype(np.float32)               # what a wrong index would add
        hot[np.arange(10), argmax(out)] = np.array(HOT_VALUES * 2, np.float32)
        return out, hot
    return Case("hotvals-E%d" % E, make, E=E, N=10, kind="hotvals")


SPECIAL_E = (10, 40, 300)                                                     # one width per lane count
HIT_CASES = ([_lanes_case(E) for E in (1, 2, 31, 32, 33, 40, 255, 256, 257, 300, 1000)]
             + [_trip_case(10, N) for N in (0, 255, 256, 257, 513)]
             + [_trip_case(40, N) for N in (0, 31, 32, 33, 65)]
             + [_trip_case(257, N) for N in (0, 3, 4, 5, 9)]
             + [_maxpos_case(E) for E in (32, 40, 257)]
             + [_tie_case(40), _tie_case(300, (0, 1, 63, 64, 65, 128, 299))]
             + [_special_case(E, s) for E in SPECIAL_E for s in special_rows(E)]
             + [_hotvals_case(E) for E in SPECIAL_E])


def edge_labels(N, E, rng):
    """every edge label in the first rows, then labels of which about a fifth lie outside"""
    lab = rng.integers(0, E + (E + 3) // 4 + 1, N).astype(np.uint32)
    edge = np.array([E - 1, E, E + 1, ALL_ONES, 0, 0x80000000 + (E - 1), E // 2], np.uint32)
    k = min(N, len(edge))
    lab[:k] = edge[:k]
    lab[N - 1] = ALL_ONES if N > k else lab[N - 1]
    return lab


def _onehot_hit_case(N, E):
    def make():
        rng = _rng("onehot_hit %d %d" % (N, E))
        lab = edge_labels(N, E, rng)
        out = _ties_out(rng, N, E)
        want = np.where(lab < E, lab, 0).astype(np.int64)
        half = np.arange(N) % 2 == 0
        out[np.arange(N)[half], want[half]] = 5.0                             # half the rows hit for certain
        return lab, out
    return Case("onehot_hit-%dx%d" % (N, E), make, E=E, N=N, kind="onehot_hit")


ONEHOT_HIT_CASES = [_onehot_hit_case(N, E) for N, E in ((37, 1), (37, 10), (300, 10), (37, 40), (70, 40), (37, 300), (9, 300))]


def _onehot_case(N, E, in_range=False):
    def make():
        rng = _rng("onehot %d %d" % (N, E))
        return rng.integers(0, E, N).astype(np.uint32) if in_range else edge_labels(N, E, rng)
    return Case("onehot-%dx%d%s" % (N, E, "-inrange" if in_range else ""), make, E=E, N=N, kind="onehot", in_range=in_range)


ONEHOT_CASES = ([_onehot_case(5243, 100), _onehot_case(4096, 128),           # 524 300 and 524 288 = CAP elements
                 _onehot_case(10486, 100), _onehot_case(2 * CAP + 7, 1),      # 2 CAP + 24, and 2 CAP + 7 exactly (a prime: one class): a third trip of 24 / of 7
                 _onehot_case(1, 1), _onehot_case(1, 10), _onehot_case(37, 1), _onehot_case(1, 1, True), _onehot_case(37, 10, True)]
                + [_onehot_case(c.N, c.E) for c in ONEHOT_HIT_CASES if (c.N, c.E) not in ((37, 1),)])

NORMS = [(0.0, 1.0), (128.0, 1.0 / 128.0), (127.5, 1.0 / 255.0), (33.3, 0.017)]
SIZES = list(range(10)) + [CAP - 1, CAP, CAP + 1] + [4 * CAP + t for t in (0, 1, 2, 3, 5)]
SRC_OFFS, DST_OFFS = (0, 1, 2, 3), (0, 4, 8)


def _pixels(name, n):
    return _rng(name).integers(0, 256, n).astype(np.uint8)


def _labels(name, nlab):
    lab = _rng(name).integers(0, 1 << 32, nlab, dtype=np.uint64).astype(np.uint32)
    if nlab:
        lab[0] = ALL_ONES; lab[nlab - 1] = ALL_ONES - 1 if nlab > 1 else ALL_ONES
    if nlab > CAP:
        lab[CAP - 1], lab[CAP] = 0x80000001, 0x7FFFFFFF
    return lab


def _norm_case(name, n, mean, scale, so=0, do=0, bytes_=None):
    def make():
        return np.arange(256, dtype=np.uint8) if bytes_ else _pixels("pix %d" % n, n)       # the same bytes at every offset
    return Case(name, make, n=n, mean=mean, scale=scale, src_off=so, dst_off=do, kind="norm")


NORM_CASES = ([_norm_case("norm-bytes-%d" % k, 256, m, s, bytes_=True) for k, (m, s) in enumerate(NORMS)]
              + [_norm_case("norm-n%d-s%dd%d" % (n, so, do), n, 33.3, 0.017, so, do) for n in SIZES for so, do in ((0, 0), (1, 4))]
              + [_norm_case("norm-n1003-s%dd%d" % (so, do), 1003, 127.5, 1.0 / 255.0, so, do) for so in SRC_OFFS for do in DST_OFFS])


def _stage_case(name, n, mean, scale, nlab, so=0, do=0, bytes_=None):
    def make():
        return (np.arange(256, dtype=np.uint8) if bytes_ else _pixels("pix %d" % n, n)), _labels("lab %d" % nlab, nlab)
    return Case(name, make, n=n, mean=mean, scale=scale, nlab=nlab, src_off=so, dst_off=do, vec=stage_vec(so, do), kind="stage")


STAGE_CASES = ([_stage_case("stage-bytes-%d-%s" % (k, "vec" if so == 0 else "scalar"), 256, m, s, 5, so) for k, (m, s) in enumerate(NORMS) for so in (0, 1)]
               + [_stage_case("stage-n%d-s%dd%d" % (n, so, do), n, 33.3, 0.017, 9, so, do) for n in SIZES for so, do in ((0, 0), (1, 4))]
               + [_stage_case("stage-n1003-s%dd%d" % (so, do), 1003, 127.5, 1.0 / 255.0, 5, so, do) for so in SRC_OFFS for do in DST_OFFS]
               + [_stage_case("stage-n3-nlab%d" % k, 3, 128.0, 1.0 / 128.0, k) for k in (0, 1, 700)]                    # more labels than pixel lanes
               + [_stage_case("stage-n%d-nlab%d" % (n, k), n, 128.0, 1.0 / 128.0, k) for n in (0, 1003) for k in (CAP, CAP + 1)]
               + [_stage_case("stage-n1003-nlab%d" % (2 * CAP + 5), 1003, 128.0, 1.0 / 128.0, 2 * CAP + 5)])
OFFSET_GROUP = [c for c in STAGE_CASES if c.name.startswith("stage-n1003-s")]      # the same 1003 bytes on both paths

# one case per entry on a library stream and under capture
STREAM_HIT = ["lanes-E31", "lanes-E255", "lanes-E300"]
STREAM_STAGE, STREAM_ONEHOT = "stage-n1003-s0d0", "onehot-37x40"


def by_name(table, name):
    return next(c for c in table if c.name == name)


def counts():
    return {"hit": len(HIT_CASES), "onehot_hit": len(ONEHOT_HIT_CASES), "onehot": len(ONEHOT_CASES), "normalize": len(NORM_CASES), "stage": len(STAGE_CASES)}
