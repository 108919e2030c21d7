"""The optimizer step (csrc/optim.hip) at every launch path, through the C ABI: k_opt_chunked in its vector and its element-by-element branch under
every kind and every placement of the four tensors of a record, the host's aliasing included; the snapshot that rides in the launch; k_opt_step<false> with
a conv stack's partial fold inside, at skip bits that are no prefix and at record 63, and every table it must refuse; a captured and replayed step; the
exchanging launch k_opt_step<true> in self mode (one child process); the argument checks.

Every case: t4k_launch_count() asserted, the branch label of tests/optim_cases.py recomputed from the device pointers BEFORE the launch (a case that
stops reaching its branch fails), every NaN moat bit-identical afterwards, DG all +0, W / M / V of every element inside the float64 witness on the
operands uploaded (tests/f64_witness.py, bounds as they stand), W, M and V the oracle's bits, a tensor the kind does not write - and every tensor of a skipped
or empty record - bit-equal to what was uploaded.  Tables, operands and checks: tests/optim_cases.py (the CPU half, tests/test_optim_cases.py, holds the
checks themselves to injected defects)."""
import ctypes
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import f64_witness as wt
import optim_cases as oc
from test_gpu_deferred import ParamRec, _setup
from test_gpu_parity import Dev, p

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
T4K_ERR_ARG = -1
KN = list(oc.KINDS)


@pytest.fixture(scope="module")
def dev(t4k):
    t4k.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return Dev(t4k)


def launches(t4k):
    return int(t4k.lib.t4k_launch_count())


class Arena:
    """every tensor of a table in ONE device buffer at the offsets of an optim_cases.Plan, NaN everywhere else; `cur` = what the device holds"""

    def __init__(self, dev, plan):
        self.dev, self.plan = dev, plan
        self.cur = np.full(plan.total, np.nan, np.float32)
        self.t = dev.up(self.cur); self.base = p(self.t)
        assert self.base % 256 == 0
        self.sizes, self.nw = plan.sizes, oc.NW

    def put(self, s, a):
        """a -> floats [s, s + len) on the host copy and on the device"""
        a = np.ascontiguousarray(a, np.float32)
        self.cur[s:s + a.size] = a
        if a.size:
            self.t[s:s + a.size].copy_(self.dev.torch.from_numpy(a))

    def fill(self, rng, skip=()):
        for i, n in enumerate(self.plan.sizes):
            for t, x in zip(oc.TENSORS, oc.operands(rng, n)):
                if (i, t) in self.plan.own and (i, t) not in skip:
                    self.put(self.plan.rec[i][t][0], x)
        for s, n in self.plan.extra.values():
            self.put(s, np.full(n, -7.0, np.float32))

    def fresh_gradients(self, rng):
        for i, n in enumerate(self.plan.sizes):
            self.put(self.plan.rec[i]["DG"][0], oc.fresh_gradient(rng, n))

    def ptr(self, i, t):
        return self.base + 4 * self.plan.rec[i][t][0]

    def xptr(self, name):
        return self.base + 4 * self.plan.extra[name][0]

    def xview(self, buf, name):
        s, n = self.plan.extra[name]
        return buf[s:s + n]

    def table(self, nw=oc.NW):
        raw, self.chunks = self.plan.table(self.base, nw=nw)
        self.nw = nw
        self.tab = self.dev.up(np.frombuffer(raw, np.uint8)); self.host = (ParamRec * len(self.plan.sizes)).from_buffer_copy(raw)
        return self

    def download(self):
        return self.dev.down(self.t).copy()

    def branches(self, keep_src=0, keep_dst=0):
        return tuple(oc.branch_of(*self.plan.pointers(self.base, i), keep_src, keep_dst) for i in range(len(self.plan.sizes)))

    def aliased(self, i):
        return tuple(t for t in ("M", "V") if (i, t) not in self.plan.own)


def make(dev, kname, layout, rng, sizes=oc.SIZES, extra=(), nw=oc.NW):
    a = Arena(dev, oc.Plan(sizes, layout, kname, extra))
    a.fill(rng)
    return a.table(nw)


def check_step(name, oracle, kname, a, new, skip=(), report="optimizer sweep"):
    """the shared checks of one step over the whole table; then `new` is what the device holds"""
    pl = a.plan
    oc.same_bits(name + " moats", new[pl.moat], a.cur[pl.moat])
    for i, n in enumerate(pl.sizes):
        ini = tuple(pl.view(a.cur, i, t).copy() for t in oc.TENSORS); got = tuple(pl.view(new, i, t) for t in oc.TENSORS)
        if i in skip or n == 0:
            for t, g, x in zip(oc.TENSORS, got, ini):
                oc.same_bits("%s record %d %s left alone" % (name, i, t), g, x)
            continue
        Nw = a.nw[i % len(a.nw)]
        oc.check_record("%s record %d n=%d" % (name, i, n), kname, ini, got, oc.oracle_step(oracle, kname, *ini, Nw), Nw, a.aliased(i), report)
    a.cur = new


def opt_args(kname):
    kind, lr, b1, b2, wd = oc.KINDS[kname]
    return kind, (lr, b1, b2, wd)


def chunked(t4k, a, kname):
    kind, hp = opt_args(kname)
    return t4k.lib.t4k_opt_chunked(kind, p(a.tab), len(a.plan.sizes), a.chunks, *hp, None)


def step(t4k, a, kname, s=None, host=True):
    kind, hp = opt_args(kname)
    return t4k.lib.t4k_opt_step(kind, p(a.tab), a.host if host else None, len(a.plan.sizes), a.chunks, *hp, s)


# ----------------------------------------------------------------------------- k_opt_chunked
@pytest.mark.parametrize("layout", list(oc.LAYOUTS))
@pytest.mark.parametrize("kname", KN)
def test_chunked_every_kind_layout(t4k, dev, oracle, kname, layout):
    """three consecutive steps on one table, a fresh gradient each, every step checked; one launch each"""
    rng = np.random.default_rng(1000 + 10 * KN.index(kname) + list(oc.LAYOUTS).index(layout))
    a = make(dev, kname, layout, rng)
    assert a.branches() == oc.BRANCH[layout], (layout, a.branches())
    for s in range(oc.STEPS):
        if s:
            a.fresh_gradients(rng)
        l0 = launches(t4k)
        assert chunked(t4k, a, kname) == 0
        assert launches(t4k) - l0 == 1
        check_step("%s %s step %d" % (kname, layout, s), oracle, kname, a, a.download())


BITS = {}      # kind -> (elements of the table whose weights differ from the oracle's, worst distance in ulps)


@pytest.mark.parametrize("layout", ["aligned", "all_off8"])
@pytest.mark.parametrize("kname", KN)
def test_chunked_weights_against_the_oracle_bits(t4k, dev, oracle, kname, layout):
    """the header comment of optim.hip: "every kernel that updates a parameter produces the oracle's bits" - SGD's weights (the existing bar) and Adam's and
    AdamW's too, over the whole table in both branches.  With __fsqrt_rn (the bare v_sqrt_f32) 15 of the 11 208 Adam weights of the aligned table differed, by up
    to 8 ulps (v' small, the quotient cancelling against the weight); with the correctly rounded root none does (tests/README.md), and that is asserted."""
    rng = np.random.default_rng(1100 + KN.index(kname))
    a = make(dev, kname, layout, rng)
    assert a.branches() == oc.BRANCH[layout]
    assert chunked(t4k, a, kname) == 0
    new = a.download()
    cnt = worst = tot = 0
    for i, n in enumerate(a.plan.sizes):
        ini = tuple(a.plan.view(a.cur, i, t).copy() for t in oc.TENSORS)
        c, u = oc.ulps(a.plan.view(new, i, "G"), oc.oracle_step(oracle, kname, *ini, oc.NW[i])[0])
        cnt += c; worst = max(worst, u); tot += n
    BITS[(kname, layout)] = (cnt, worst)
    print("\noracle-bits %s %s: %d of %d weights differ, worst %d ulp" % (kname, layout, cnt, tot, worst))
    check_step("%s %s" % (kname, layout), oracle, kname, a, new)
    assert (cnt, worst) == (0, 0), (kname, layout, cnt, worst)


@pytest.mark.parametrize("layout", ["aligned", "all_off8"])
@pytest.mark.parametrize("kname", KN)
def test_specials(t4k, dev, oracle, kname, layout):
    """gradients 0, -0, subnormal, with d * d underflowing and overflowing, infinite and NaN, against moments {0, 1e-38, 1, 1e30} and weights {0, +-1, +-1e30}:
    W, M and V are the NumPy float32 implementation's and the oracle's bits, NaN where they have a NaN (the payload of a NaN an operation produces is the
    implementation's own); Nw = 3, so the SGD kinds divide"""
    a = Arena(dev, oc.Plan((oc.SPECIAL_N,), layout, kname))
    ini = oc.specials()
    for t, x in zip(oc.TENSORS, ini):
        a.put(a.plan.rec[0][t][0], x)
    a.table(nw=(3,))
    assert a.branches() == oc.BRANCH[layout][:1]
    l0 = launches(t4k)
    assert chunked(t4k, a, kname) == 0
    assert launches(t4k) - l0 == 1
    new = a.download()
    oc.same_bits("moats", new[a.plan.moat], a.cur[a.plan.moat])
    ref = oc.np_step(kname, *ini, 3)[:4]; orc = oc.oracle_step(oracle, kname, *ini, 3)
    kind = oc.KINDS[kname][0]
    for j, t in enumerate(oc.TENSORS):
        got = a.plan.view(new, 0, t)
        if t == "DG":
            assert not oc.bits(got).any()
        elif (t == "M" and kname == "sgd0") or (t == "V" and kind == 0):
            oc.same_bits("%s specials %s left alone" % (kname, t), got, ini[j])
        else:
            oc.same_values("%s specials %s vs NumPy float32" % (kname, t), got, ref[j]); oc.same_values("%s specials %s vs oracle" % (kname, t), got, orc[j])


# ----------------------------------------------------------------------------- t4k_opt_snapshot
SNAP_SIZES = (2049, 5, 1025)
SNAP_FORMS = {"vector-branch": ("aligned", 0, "vec"), "scalar-branch": ("g_off4", 0, "scalar"), "destination-4-bytes-off": ("aligned", 1, "scalar")}


@pytest.mark.parametrize("form", list(SNAP_FORMS))
def test_snapshot_rides_in_the_launch(t4k, dev, oracle, form):
    """the pre-update weights of record 0 (two whole chunks and one element) land in the destination inside the update launch, from the vector branch, the scalar
    branch, and with a destination 4 bytes off, which must drop THAT record to the scalar branch (the others stay) and still update it; consumed once"""
    layout, doff, want = SNAP_FORMS[form]
    lib = t4k.lib
    for kname in KN:
        rng = np.random.default_rng(1200 + KN.index(kname))
        a = make(dev, kname, layout, rng, SNAP_SIZES, extra=(("keep", SNAP_SIZES[0], doff),))
        G, dst = a.ptr(0, "G"), a.xptr("keep")
        assert a.branches(G, dst) == (want,) + oc.BRANCH[layout][1:3], (form, a.branches(G, dst))
        assert lib.t4k_opt_snapshot_pending() == 0
        assert lib.t4k_opt_snapshot(G, None) == T4K_ERR_ARG and lib.t4k_opt_snapshot_pending() == 0          # a null destination: refused, nothing pending
        assert lib.t4k_opt_snapshot(G, dst) == 0 and lib.t4k_opt_snapshot_pending() == 1
        l0 = launches(t4k)
        assert chunked(t4k, a, kname) == 0
        assert launches(t4k) - l0 == 1 and lib.t4k_opt_snapshot_pending() == 0
        new = a.download()
        w0 = a.plan.view(a.cur, 0, "G").copy()
        oc.same_bits("%s %s snapshot" % (form, kname), a.xview(new, "keep"), w0)
        check_step("%s %s" % (form, kname), oracle, kname, a, new)                                            # (the destination's moat is one of the moats)
        a.cur[a.plan.extra["keep"][0]:][:SNAP_SIZES[0]] = w0                                                   # what the destination holds from now on
        a.fresh_gradients(rng)
        assert chunked(t4k, a, kname) == 0                                                                    # a second step copies nothing
        new = a.download()
        oc.same_bits("%s %s snapshot after a second step" % (form, kname), a.xview(new, "keep"), w0)
        check_step("%s %s second step" % (form, kname), oracle, kname, a, new)
        assert lib.t4k_opt_snapshot(G, dst) == 0 and lib.t4k_opt_snapshot_pending() == 1
        assert lib.t4k_opt_snapshot(None, None) == 0 and lib.t4k_opt_snapshot_pending() == 0                  # cancelled
        a.fresh_gradients(rng)
        assert chunked(t4k, a, kname) == 0
        new = a.download()
        oc.same_bits("%s %s snapshot after a cancelled request" % (form, kname), a.xview(new, "keep"), w0)
        check_step("%s %s third step" % (form, kname), oracle, kname, a, new)


# ----------------------------------------------------------------------------- t4k_opt_step with a conv stack's fold pending
_STACKS = {}


def _stack(t4k, dev, oracle, case):
    if case not in _STACKS:
        _STACKS[case] = _setup(t4k, dev, oracle, case, 500 + case)
    return _STACKS[case]


def _fold_run(t4k, dev, oracle, name, case, shape, kname, defer):
    """forward, backward (train | 4 when `defer`), the optimizer (t4k_opt_step / t4k_opt_chunked) over the table of `shape`, a second optimizer call.
    Returns what every tensor holds after each of the two calls, the launches of backward + first optimizer call and of the second call, the folded
    gradients (undeferred side) and the table's description."""
    N, X, stages, flat, params, arr, bufs, dDY, _ = _stack(t4k, dev, oracle, case)
    T = dev.torch
    nst = len(stages)
    order = oc.fold_order(nst, shape)
    recs = []                                                   # (token, n in the table, Nw)
    for tok in order:
        if isinstance(tok, str):
            F, B = params[int(tok[1:])]
            recs.append((tok, F.size, F.shape[0]) if tok[0] == "F" else (tok, B.size, B.size))
        elif tok[0] == "x":
            recs.append((tok, tok[1], 1 + len(recs) % 3))
        else:
            recs += [(("x", 1), 1, 1)] * tok[1]
    full = [n for _, n, _ in recs]                              # the arena holds every record's four tensors (a stack record's G / DG there are bystanders)
    snap_i = next(i for i, (tok, _, _) in enumerate(recs) if tok == "F0") if (shape in ("rec63", "rec65") or (shape in ("spread", "null_host") and kname in ("sgd0", "adam"))) \
        else next(i for i, (tok, _, _) in enumerate(recs) if tok == ("x", 3000))
    a = Arena(dev, oc.Plan(full, "aligned", "adam", extra=(("keep", full[snap_i], 0),)))
    a.fill(np.random.default_rng(1300 + case))
    ptr = {}
    for si in range(nst):
        F, B = params[si]
        bufs[si]["F"].copy_(T.from_numpy(F)); bufs[si]["B"].copy_(T.from_numpy(B))
        bufs[si]["DF"].fill_(0.25); bufs[si]["DB"].fill_(-0.5)                    # gradients ACCUMULATE: the fold adds to what is there
        ptr["F%d" % si] = (p(bufs[si]["F"]), p(bufs[si]["DF"])); ptr["B%d" % si] = (p(bufs[si]["B"]), p(bufs[si]["DB"]))
    pad, chunks = oc.pads([n - 1 if (shape == "short" and tok == "F0") else n for tok, n, _ in recs])
    raw = b""
    for i, (tok, n, nw) in enumerate(recs):
        G, DG, M, V = a.plan.pointers(a.base, i)
        if isinstance(tok, str):
            G, DG = ptr[tok]
        raw += struct.pack("<QQQQqii", G, DG, M, V, n - 1 if (shape == "short" and tok == "F0") else n, nw, pad[i])
    tab = dev.up(np.frombuffer(raw, np.uint8)); host = (ParamRec * len(recs)).from_buffer_copy(raw)
    keep_src = struct.unpack_from("<Q", raw, 48 * snap_i)[0]
    kind, hp = opt_args(kname)

    def optimizer():
        if defer:
            return t4k.lib.t4k_opt_step(kind, p(tab), None if shape == "null_host" else host, len(recs), chunks, *hp, None)
        return t4k.lib.t4k_opt_chunked(kind, p(tab), len(recs), chunks, *hp, None)

    def everything():
        out = {"arena": a.download()}
        for si in range(nst):
            for k_ in ("F", "B", "DF", "DB"):
                out["%s%d" % (k_, si)] = dev.down(bufs[si][k_]).copy().ravel()
        return out

    t4k.call("t4k_rand_init", 55 + case); t4k.call("t4k_rand_set_offset", 4096)
    bufs[0]["X"].copy_(T.from_numpy(X))
    t4k.call("t4k_conv_stack_fwd", p(bufs[0]["X"]), None, arr, nst, N, None)
    t4k.call("t4k_sync", None)
    l0 = launches(t4k)
    t4k.call("t4k_conv_stack_bwd", p(dDY), arr, nst, N, 5 if defer else 1, None)
    n1 = launches(t4k) - l0
    folded = None
    if not defer:                                                                 # (any entry point - the sync of a read-back too - would run a deferred fold first)
        folded = {"%s%d" % (k_[1], si): dev.down(bufs[si][k_]).copy().ravel() for si in range(nst) for k_ in ("DF", "DB")}
    assert t4k.lib.t4k_opt_snapshot(keep_src, a.xptr("keep")) == 0
    l0 = launches(t4k)
    assert optimizer() == 0
    n1 += launches(t4k) - l0
    assert t4k.lib.t4k_opt_snapshot_pending() == 0
    first = everything()
    l0 = launches(t4k)
    assert optimizer() == 0
    n2 = launches(t4k) - l0
    return dict(first=first, second=everything(), n1=n1, n2=n2, folded=folded, recs=recs, arena=a, snap_i=snap_i, params=params)


def _fold_pair(t4k, dev, oracle, name, case, shape, what, kname):
    und = _fold_run(t4k, dev, oracle, name, case, shape, kname, False)
    dfr = _fold_run(t4k, dev, oracle, name, case, shape, kname, True)
    assert und["n1"] == 3 and und["n2"] == 1, (und["n1"], und["n2"])               # backward, stand-alone fold, chunked step
    assert dfr["n1"] == (2 if what == "fold" else 3) and dfr["n2"] == 1, (name, what, dfr["n1"], dfr["n2"])   # the fold inside the update; refused: the undeferred launches
    for when in ("first", "second"):
        for k_ in und[when]:
            oc.same_bits("%s %s %s after the %s optimizer call: deferred against undeferred" % (name, kname, k_, when), dfr[when][k_], und[when][k_])
    # the undeferred side against float64 and the oracle, on the operands of ITS update: the parameters uploaded, the folded gradients read back before the step
    a, params, got, new = und["arena"], und["params"], und["first"], und["first"]["arena"]
    pl = a.plan
    oc.same_bits(name + " moats", new[pl.moat], a.cur[pl.moat])
    in_table = set()
    for i, (tok, n, nw) in enumerate(und["recs"]):
        ini = [pl.view(a.cur, i, t).copy() for t in oc.TENSORS]; out = [pl.view(new, i, t) for t in oc.TENSORS]
        nt = n
        if isinstance(tok, str):
            in_table.add(tok)
            for t in (0, 1):                                                        # the arena's own G / DG of a stack record are in no table
                oc.same_bits("%s record %d bystander" % (name, i), out[t], ini[t])
            F, B = params[int(tok[1:])]
            ini[0], ini[1] = (F if tok[0] == "F" else B).ravel(), und["folded"][tok]
            out[0], out[1] = got[tok], got["D" + tok]
            if shape == "short" and tok == "F0":
                nt = n - 1
                for t in range(4):                                                  # the element the table leaves out
                    oc.same_bits("%s %s last element" % (name, tok), out[t][nt:], ini[t][nt:])
        orc = oc.oracle_step(oracle, kname, *(x[:nt] for x in ini), nw)
        oc.check_record("%s %s record %d %s" % (name, kname, i, tok), kname, tuple(x[:nt] for x in ini), tuple(x[:nt] for x in out), orc, nw, report="optimizer sweep (with fold)")
    for si in range(len(params)):                                                   # a stack tensor that is in no table: parameters as uploaded, gradient folded and kept
        for t in ("F%d" % si, "B%d" % si):
            if t not in in_table:
                oc.same_bits(name + " " + t, got[t], params[si][0 if t[0] == "F" else 1].ravel()); oc.same_bits(name + " D" + t, got["D" + t], und["folded"][t])
    # the snapshot: the pre-update values of the tensor asked for, from the fold half (F0) or the chunk half (the plain tensor)
    tok = und["recs"][und["snap_i"]][0]
    w0 = params[0][0].ravel() if tok == "F0" else pl.view(a.cur, und["snap_i"], "G")
    oc.same_bits("%s %s snapshot of %s" % (name, kname, tok), a.xview(new, "keep"), w0)
    oc.same_bits("%s %s snapshot of %s after the second call" % (name, kname, tok), a.xview(und["second"]["arena"], "keep"), w0)


@pytest.mark.parametrize("kname", KN)
@pytest.mark.parametrize("name,case,shape,what", [r for r in oc.FOLD_TABLES if r[3] == "fold"], ids=[r[0] for r in oc.FOLD_TABLES if r[3] == "fold"])
def test_step_with_fold_matches_fold_then_chunked(t4k, dev, oracle, name, case, shape, what, kname):
    """t4k_conv_stack_bwd(train | 4) + t4k_opt_step, 2 launches, against t4k_conv_stack_bwd(train) + t4k_opt_chunked, 3 launches: every tensor bit for bit,
    and the undeferred side against float64, so the pair hangs on a reference.  Plain tensors in front of, between and behind the folded ones (skip bits
    1, 3, 4, ...), a folded tensor as record 63; the snapshot of the first filter (fold half) under sgd0 / adam, of the plain tensor otherwise."""
    _fold_pair(t4k, dev, oracle, name, case, shape, what, kname)


@pytest.mark.parametrize("kname", KN)
@pytest.mark.parametrize("name,case,shape,what", [r for r in oc.FOLD_TABLES if r[3] != "fold"], ids=[r[0] for r in oc.FOLD_TABLES if r[3] != "fold"])
def test_refused_folds_fall_back(t4k, dev, oracle, name, case, shape, what, kname):
    """65 records, a folded tensor missing from the table, one with n one less than its segment, tab_host = NULL: t4k_opt_step runs the stand-alone fold and
    the plain step (the undeferred path's launches and bits), and a following t4k_opt_step finds nothing pending.  All calls on one stream."""
    _fold_pair(t4k, dev, oracle, name, case, shape, what, kname)


# ----------------------------------------------------------------------------- a captured step
@pytest.mark.parametrize("kname", KN)
def test_captured_step_replays(t4k, dev, oracle, kname):
    """t4k_opt_step recorded once (nothing pending: one launch, counted at capture), replayed three times with a fresh gradient uploaded between the replays:
    the moments are carried through the replays, every step bit-equal to the eager step"""
    s = ctypes.c_void_p()
    t4k.call("t4k_stream_create", ctypes.byref(s))
    try:
        eager = []
        a = make(dev, kname, "aligned", np.random.default_rng(1401))
        for k_ in range(3):
            if k_:
                a.fresh_gradients(np.random.default_rng(1410 + k_))
            dev.torch.cuda.synchronize()
            assert step(t4k, a, kname, s) == 0
            t4k.call("t4k_sync", s)
            new = a.download(); check_step("%s eager step %d" % (kname, k_), oracle, kname, a, new); eager.append(new.copy())   # (a.cur is `new` from here on, and the next gradients go into it)
        a = make(dev, kname, "aligned", np.random.default_rng(1401))
        dev.torch.cuda.synchronize()
        g = ctypes.c_void_p()
        t4k.call("t4k_graph_begin", s)
        l0 = launches(t4k)
        rc = step(t4k, a, kname, s)
        n = launches(t4k) - l0
        t4k.call("t4k_graph_end", s, ctypes.byref(g))
        assert rc == 0 and n == 1
        t4k.call("t4k_sync", s)
        oc.same_bits("recording runs nothing", a.download(), a.cur)
        for k_ in range(3):
            if k_:
                a.fresh_gradients(np.random.default_rng(1410 + k_))
            dev.torch.cuda.synchronize()
            l0 = launches(t4k)
            t4k.call("t4k_graph_launch", g, s)
            t4k.call("t4k_sync", s)
            new = a.download()
            oc.same_bits("%s replay %d" % (kname, k_), new, eager[k_])
            a.cur = new
        t4k.call("t4k_graph_destroy", g)
    finally:
        t4k.call("t4k_stream_destroy", s)


# ----------------------------------------------------------------------------- the exchanging launch, in a process of its own
def test_exchanging_launch_in_self_mode():
    """k_opt_step<true> as a single process reaches it (t4k_xchg_self, what bench.py --full times as dp_overhead_us): t4k_opt_step_dp against t4k_opt_step bit
    for bit over a plain table inside one slab, with a conv stack's fold pending, and through the fall-back (a DG outside the slab; slab_n above the window:
    the slab summed in ceil(slab_n / 65536) launches, then the plain step); refused under capture.  ONE child, so the exchange's process-wide state never
    reaches this session (tests/optim_xchg_worker.py prints one JSON line)."""
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "optim_xchg_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.fail("optim_xchg_worker.py did not finish in 120 s: %s" % ((e.stderr or b"")[-2000:],))
    assert r.returncode == 0, "optim_xchg_worker.py exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["ok"] is True and out["failed"] == [], out
    assert out["active_in_self_mode"] == 1 and out["active_after"] == 0 and out["world_after"] == 0, out
    want = {"%s %s" % (f, k_) for f in ("plain", "fold", "dg-outside-slab", "slab-above-window", "capture") for k_ in KN}
    assert set(out["passed"]) == want, sorted(want - set(out["passed"]))
    for k_, (n, ceil_) in out["fallback_launches"].items():
        assert n == ceil_ + 1, (k_, n, ceil_)
    for k_, n in out["exchanging_launches"].items():
        assert n == (2 if k_.startswith("fold") else 1), (k_, n)                    # plain: the update alone; fold: backward + update


# ----------------------------------------------------------------------------- arguments
def test_bad_arguments(t4k, dev, oracle):
    """kind 3, a null table with n_tensors > 0, t4k_sgd with momentum and no M, Nw = 0: an error code, no launch, nothing written; n_tensors = 0 or
    n_chunks = 0: T4K_OK, no launch, nothing written"""
    lib = t4k.lib
    a = make(dev, "adam", "aligned", np.random.default_rng(1500), (5, 1025))
    nt, hp = 2, (1e-3, 0.9, 0.999, 0.01)
    G, DG, M, V = a.plan.pointers(a.base, 1)
    l0 = launches(t4k)
    assert lib.t4k_opt_chunked(3, p(a.tab), nt, a.chunks, *hp, None) == T4K_ERR_ARG
    assert lib.t4k_opt_chunked(-1, p(a.tab), nt, a.chunks, *hp, None) == T4K_ERR_ARG
    assert lib.t4k_opt_step(3, p(a.tab), a.host, nt, a.chunks, *hp, None) == T4K_ERR_ARG
    assert lib.t4k_opt_chunked(1, None, nt, a.chunks, *hp, None) == T4K_ERR_ARG
    assert lib.t4k_opt_step(1, None, a.host, nt, a.chunks, *hp, None) == T4K_ERR_ARG
    assert lib.t4k_sgd(G, DG, None, 2, 0.01, 0.9, 1025, None) == T4K_ERR_ARG
    assert lib.t4k_sgd(G, DG, M, 0, 0.01, 0.9, 1025, None) == T4K_ERR_ARG
    assert lib.t4k_sgd(G, DG, None, 0, 0.01, 0.0, 1025, None) == T4K_ERR_ARG
    assert lib.t4k_opt_chunked(1, p(a.tab), 0, a.chunks, *hp, None) == 0
    assert lib.t4k_opt_chunked(1, p(a.tab), nt, 0, *hp, None) == 0
    assert lib.t4k_opt_step(1, p(a.tab), a.host, 0, a.chunks, *hp, None) == 0
    assert lib.t4k_opt_step(1, p(a.tab), a.host, nt, 0, *hp, None) == 0
    assert launches(t4k) - l0 == 0
    oc.same_bits("nothing written", a.download(), a.cur)
    assert lib.t4k_sgd(G, DG, None, 2, 0.01, 0.0, 1025, None) == 0 and launches(t4k) - l0 == 1     # plain SGD needs no M: the call the refusals above stand beside
    new = a.download()
    ini = tuple(a.plan.view(a.cur, 1, t).copy() for t in oc.TENSORS)
    oc.check_record("t4k_sgd without M", "sgd0", ini, tuple(a.plan.view(new, 1, t) for t in oc.TENSORS), oc.oracle_step(oracle, "sgd0", *ini, 2), 2)
    oc.same_bits("moats", new[a.plan.moat], a.cur[a.plan.moat])


def test_worst_ratios_are_reported():
    """what tests/README.md quotes: worst |error| / bound per tensor kind over the tests above (every ratio was asserted <= 1 where it was measured)"""
    rows = {k_: v for k_, v in wt.WORST.items() if k_.startswith("optimizer sweep")}
    for k_ in sorted(rows):
        print("\nworst |error| / bound, %s: %.3g (%s)" % (k_, rows[k_][0], rows[k_][1]))
    for k_ in sorted(BITS):
        print("\noracle bits %s %s: %d elements differ, worst %d ulp" % (k_ + BITS[k_]))
    assert all(v[0] <= 1.0 for v in rows.values())
