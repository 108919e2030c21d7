"""The feed, label and hit-count entries through the C ABI: t4k_hit and t4k_onehot_hit (k_hit<1|8|64>, csrc/reduce.hip), t4k_onehot, t4k_u8_normalize and
t4k_stage_batch (k_onehot, k_u8norm, k_stage_batch, csrc/elementwise.hip) on every case of tests/feed_label_cases.py - lane counts, trips of the single
workgroup, the maximum and every tie by lane, the specials, labels outside the classes, sizes on both sides of the grid cap, both paths of the staging kernel
from every byte offset, more labels than the capped grid has threads.

Every case: outputs prefilled (NaN, 0xa5 bytes, 0x5a5a5a5a for the count) between guard bytes, one launch (t4k_launch_count), the result equal BIT FOR BIT to
the numpy witness (held to the oracle by tests/test_feed_label_cases.py), the guards and every input bit-identical afterwards.  Then the count in pinned host
memory as host/model.cpp reads it, t4k_onehot + t4k_hit against t4k_onehot_hit, a library stream, a captured and replayed launch, and the rejections."""
import ctypes
import time

import numpy as np
import pytest

import feed_label_cases as fc

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1
GUARD, GUARD_BYTE = 64, 0xC3
CNT_PREFILL = 0x5a5a5a5a
CLOCK = {}


@pytest.fixture(scope="module", autouse=True)
def _clock():
    CLOCK.setdefault("t0", time.time())


def lcount(h):
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    return int(h.lib.t4k_launch_count())


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Dev:
    """the bytes of `a` starting `off` bytes behind GUARD guard bytes in a 256-byte aligned device allocation, GUARD guard bytes behind them; `host` = what
    the device is meant to hold where nothing writes"""

    def __init__(self, a, off=0):
        import torch
        self.torch = torch
        a = np.ascontiguousarray(a)
        self.dtype, self.shape, self.n, self.lo = a.dtype, a.shape, a.nbytes, GUARD + off
        self.host = np.full(self.lo + self.n + GUARD, GUARD_BYTE, np.uint8)
        self.host[self.lo:self.lo + self.n] = a.view(np.uint8).ravel()
        self.t = torch.from_numpy(self.host.copy()).cuda()
        torch.cuda.synchronize()
        assert self.t.data_ptr() % 256 == 0

    @property
    def addr(self):
        return self.t.data_ptr() + self.lo

    @property
    def p(self):
        return ctypes.c_void_p(self.addr)

    def put(self, a):
        """new contents for the payload, the allocation stays where it is"""
        a = np.ascontiguousarray(a, self.dtype)
        assert a.nbytes == self.n
        self.host[self.lo:self.lo + self.n] = a.view(np.uint8).ravel()
        self.t.copy_(self.torch.from_numpy(self.host.copy()))
        self.torch.cuda.synchronize()

    def get(self, h, s=None):
        """the payload after the stream's work; the guards checked on the way"""
        h.call("t4k_sync", s)
        b = self.t.cpu().numpy()
        assert np.array_equal(b[:self.lo], self.host[:self.lo]) and np.array_equal(b[self.lo + self.n:], self.host[self.lo + self.n:]), "written outside the buffer"
        return b[self.lo:self.lo + self.n].copy().view(self.dtype).reshape(self.shape)

    def intact(self, h, s=None):
        return same(self.get(h, s), self.host[self.lo:self.lo + self.n].copy().view(self.dtype).reshape(self.shape))


def nan_like(shape):
    return np.full(shape, np.nan, np.float32)


def a5_words(n):
    return np.full(n, 0xA5A5A5A5, np.uint32)


# ---------------------------------------------------------------- one object per entry: operands up, launch, witness, new operands
class Op:
    launches = 1

    def run(self, h, s=None):
        """launch once: status, launch count, every output against the witness, guards and inputs intact"""
        l0 = lcount(h)
        rc = self.launch(h, s)
        assert rc == OK and lcount(h) - l0 == self.launches, (self.name, rc, lcount(h) - l0)
        got = self.read(h, s)
        self.judge(got)
        return got

    def read(self, h, s=None):
        return [o.get(h, s) for o in self.outs]

    def judge(self, got):
        for k, (g, w) in enumerate(zip(got, self.want())):
            assert same(g, w), "%s output %d: %d of %d elements differ%s" % (self.name, k, int(np.sum(g.view(np.uint32) != w.view(np.uint32))), w.size,
                                                                             " (got %s, want %s)" % (g.ravel()[:4], w.ravel()[:4]) if w.size <= 4 else "")

    def inputs_intact(self, h, s=None):
        return all(d.intact(h, s) for d in self.ins)

    def prefill(self):
        for o, f in zip(self.outs, self.fills):
            o.put(f)

    def still_prefilled(self, h, s=None):
        return all(same(g, f) for g, f in zip(self.read(h, s), self.fills))


class HitOp(Op):
    def __init__(self, case):
        self.name, (self.out, self.hot) = case.name, case.build()
        self.N, self.E = case.N, case.E
        self.ins, self.fills = [Dev(self.out), Dev(self.hot)], [np.array([CNT_PREFILL], np.int32)]
        self.outs = [Dev(self.fills[0])]

    def launch(self, h, s, cnt=None):
        return h.lib.t4k_hit(self.ins[0].p, self.ins[1].p, self.N, self.E, cnt or self.outs[0].p, s)

    def want(self):
        return [np.array([fc.hit(self.out, self.hot)], np.int32)]

    def mutate(self):
        self.out, self.hot = self.out[::-1].copy(), np.roll(self.hot, 1, axis=1)
        self.ins[0].put(self.out); self.ins[1].put(self.hot)


class OnehotHitOp(Op):
    def __init__(self, case):
        self.name, (self.lab, self.out) = case.name, case.build()
        self.N, self.E = case.N, case.E
        self.ins, self.fills = [Dev(self.lab), Dev(self.out)], [nan_like((self.N, self.E)), np.array([CNT_PREFILL], np.int32)]
        self.outs = [Dev(f) for f in self.fills]

    def launch(self, h, s, cnt=None):
        return h.lib.t4k_onehot_hit(self.ins[0].p, self.outs[0].p, self.ins[1].p, self.N, self.E, cnt or self.outs[1].p, s)

    def want(self):
        hot = fc.onehot(self.lab, self.N, self.E)
        return [hot, np.array([fc.hit(self.out, hot)], np.int32)]


class OnehotOp(Op):
    def __init__(self, case):
        self.name, self.lab, self.N, self.E = case.name, case.build(), case.N, case.E
        self.ins, self.fills = [Dev(self.lab)], [nan_like((self.N, self.E))]
        self.outs = [Dev(self.fills[0])]

    def launch(self, h, s):
        return h.lib.t4k_onehot(self.ins[0].p, self.outs[0].p, self.N, self.E, s)

    def want(self):
        return [fc.onehot(self.lab, self.N, self.E)]

    def mutate(self):
        self.lab = self.lab[::-1].copy()
        self.ins[0].put(self.lab)


class NormOp(Op):
    def __init__(self, case):
        self.name, self.u8, self.case = case.name, case.build(), case
        self.launches = 1 if self.u8.size else 0                                 # nothing to do: no launch
        self.ins, self.fills = [Dev(self.u8, case.src_off)], [nan_like(self.u8.size)]
        self.outs = [Dev(self.fills[0], case.dst_off)]

    def launch(self, h, s):
        return h.lib.t4k_u8_normalize(self.ins[0].p, self.outs[0].p, self.u8.size, self.case.mean, self.case.scale, s)

    def want(self):
        return [fc.normalize(self.u8, self.case.mean, self.case.scale) if self.u8.size else self.fills[0]]


class StageOp(Op):
    def __init__(self, case):
        self.name, (self.u8, self.lab), self.case = case.name, case.build(), case
        self.ins, self.fills = [Dev(self.u8, case.src_off), Dev(self.lab)], [nan_like(self.u8.size), a5_words(self.lab.size)]
        self.outs = [Dev(self.fills[0], case.dst_off), Dev(self.fills[1])]
        assert fc.stage_vec(self.ins[0].addr, self.outs[0].addr) == case.vec       # the path the case is in the table for
        self.launches = 1 if self.u8.size or self.lab.size else 0

    def launch(self, h, s):
        return h.lib.t4k_stage_batch(self.ins[0].p, self.outs[0].p, self.u8.size, self.case.mean, self.case.scale, self.ins[1].p, self.outs[1].p, self.lab.size, s)

    def want(self):
        return list(fc.stage(self.u8, self.case.mean, self.case.scale, self.lab))

    def mutate(self):
        self.u8, self.lab = (255 - self.u8).astype(np.uint8), self.lab ^ np.uint32(0x00FFFF00)
        self.ins[0].put(self.u8); self.ins[1].put(self.lab)


def sweep(h, op):
    op.run(h)
    assert op.inputs_intact(h), op.name
    return op


# ---------------------------------------------------------------- every case of the tables
@pytest.mark.parametrize("case", fc.HIT_CASES, ids=repr)
def test_hit(t4k, case):
    """N = 0 is a launch too: the count is written as 0 over its prefill"""
    sweep(t4k, HitOp(case))


@pytest.mark.parametrize("case", fc.ONEHOT_HIT_CASES, ids=repr)
def test_onehot_hit(t4k, case):
    """the one-hot rows bit for bit over NaN, the count against them"""
    sweep(t4k, OnehotHitOp(case))


@pytest.mark.parametrize("case", fc.ONEHOT_HIT_CASES, ids=repr)
def test_onehot_then_hit_equals_onehot_hit(t4k, case):
    one = OnehotHitOp(case)
    hot1, cnt1 = one.run(t4k)
    lab, out = case.build()
    dL, dH, dO, dC = Dev(lab), Dev(nan_like((case.N, case.E))), Dev(out), Dev(np.array([CNT_PREFILL], np.int32))
    l0 = lcount(t4k)
    assert t4k.lib.t4k_onehot(dL.p, dH.p, case.N, case.E, None) == OK and t4k.lib.t4k_hit(dO.p, dH.p, case.N, case.E, dC.p, None) == OK
    assert lcount(t4k) - l0 == 2
    assert same(dH.get(t4k), hot1) and same(dC.get(t4k), cnt1)


@pytest.mark.parametrize("case", fc.ONEHOT_CASES, ids=repr)
def test_onehot(t4k, case):
    sweep(t4k, OnehotOp(case))


@pytest.mark.parametrize("case", fc.NORM_CASES, ids=repr)
def test_u8_normalize(t4k, case):
    sweep(t4k, NormOp(case))


@pytest.mark.parametrize("case", fc.STAGE_CASES, ids=repr)
def test_stage_batch(t4k, case):
    sweep(t4k, StageOp(case))


def test_stage_paths_agree_on_the_same_bytes(t4k):
    """the same 1003 bytes from src 0 .. 3 bytes in to dst 0 / 4 / 8 bytes in: one case takes the vector path, eleven the scalar one"""
    got = {c.name: (c.vec, StageOp(c).run(t4k)) for c in fc.OFFSET_GROUP}
    vec = [g for v, g in got.values() if v]
    assert len(vec) == 1 and len(got) == 12
    for name, (_, g) in got.items():
        assert same(g[0], vec[0][0]) and same(g[1], vec[0][1]), name


# ---------------------------------------------------------------- the count in pinned host memory
class Pinned:
    """16 ints from t4k_host_alloc, all prefilled: what host/model.cpp passes as cnt and reads after t4k_sync, no copy command"""

    def __init__(self, h):
        self.h, self.ptr = h, ctypes.c_void_p()
        h.call("t4k_host_alloc", ctypes.byref(self.ptr), 64)
        self.w = (ctypes.c_int * 16).from_address(self.ptr.value)
        for i in range(16):
            self.w[i] = CNT_PREFILL

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.h.call("t4k_sync", None)
        self.h.call("t4k_host_free", self.ptr)


@pytest.mark.parametrize("name", fc.STREAM_HIT + ["trip-G1-N0", "special-E40-lead-nan"])
def test_hit_count_in_pinned_host_memory(t4k, name):
    op = HitOp(fc.by_name(fc.HIT_CASES, name))
    with Pinned(t4k) as pin:
        l0 = lcount(t4k)
        assert op.launch(t4k, None, cnt=pin.ptr) == OK and lcount(t4k) - l0 == 1
        t4k.call("t4k_sync", None)
        assert list(pin.w) == [int(op.want()[0][0])] + [CNT_PREFILL] * 15
    assert op.still_prefilled(t4k) and op.inputs_intact(t4k)


@pytest.mark.parametrize("case", fc.ONEHOT_HIT_CASES, ids=repr)
def test_onehot_hit_count_in_pinned_host_memory(t4k, case):
    op = OnehotHitOp(case)
    with Pinned(t4k) as pin:
        l0 = lcount(t4k)
        assert op.launch(t4k, None, cnt=pin.ptr) == OK and lcount(t4k) - l0 == 1
        t4k.call("t4k_sync", None)
        assert list(pin.w) == [int(op.want()[1][0])] + [CNT_PREFILL] * 15
    hot, cnt = op.read(t4k)
    assert same(hot, op.want()[0]) and same(cnt, op.fills[1]) and op.inputs_intact(t4k)


# ---------------------------------------------------------------- a library stream, a capture
def stream_ops():
    return ([HitOp(fc.by_name(fc.HIT_CASES, n)) for n in fc.STREAM_HIT]
            + [StageOp(fc.by_name(fc.STAGE_CASES, fc.STREAM_STAGE)), OnehotOp(fc.by_name(fc.ONEHOT_CASES, fc.STREAM_ONEHOT))])


class stream:
    def __init__(self, h):
        self.h, self.s = h, ctypes.c_void_p()

    def __enter__(self):
        self.h.call("t4k_stream_create", ctypes.byref(self.s))
        return self.s

    def __exit__(self, *exc):
        self.h.call("t4k_sync", self.s)
        self.h.call("t4k_stream_destroy", self.s)


def test_on_a_library_stream(t4k):
    """one hit case per lane count, a stage case and a onehot case: the default stream's bits, one launch each"""
    assert {fc.hit_lanes(fc.by_name(fc.HIT_CASES, n).E) for n in fc.STREAM_HIT} == {1, 8, 64}
    eager = [op.run(t4k) for op in stream_ops()]
    with stream(t4k) as s:
        for op, want in zip(stream_ops(), eager):
            got = op.run(t4k, s)
            assert all(same(g, w) for g, w in zip(got, want)) and op.inputs_intact(t4k, s), op.name


def test_captured_and_replayed(t4k):
    """recorded once: one launch counted and the outputs still their prefill; one replay gives the eager bits; the operands are overwritten in place and the
    same graph launched again: the outputs follow the new operands"""
    with stream(t4k) as s:
        for op in stream_ops():
            eager = op.run(t4k, s)
            op.prefill()
            g = ctypes.c_void_p()
            t4k.call("t4k_graph_begin", s)
            l0 = lcount(t4k)
            rc = op.launch(t4k, s)
            n = lcount(t4k) - l0
            t4k.call("t4k_graph_end", s, ctypes.byref(g))
            try:
                assert rc == OK and n == 1, (op.name, rc, n)
                assert op.still_prefilled(t4k, s), op.name                       # captured, not run
                t4k.call("t4k_graph_launch", g, s)
                got = op.read(t4k, s)
                assert all(same(a, b) for a, b in zip(got, eager)), op.name
                before = op.want()
                op.mutate(); op.prefill()
                assert not all(same(a, b) for a, b in zip(op.want(), before)), op.name
                t4k.call("t4k_graph_launch", g, s)
                op.judge(op.read(t4k, s))
                assert op.inputs_intact(t4k, s), op.name
            finally:
                t4k.call("t4k_graph_destroy", g)


# ---------------------------------------------------------------- rejections
def test_rejections_launch_nothing_and_write_nothing(t4k):
    """a NULL tensor, a negative extent, no class, labels without a label pointer: T4K_ERR_ARG; a negative size that an entry takes for "nothing to do":
    T4K_OK; in both no launch, and every output keeps its prefill"""
    lib = t4k.lib
    hit, oh, one = HitOp(fc.by_name(fc.HIT_CASES, "lanes-E31")), OnehotHitOp(fc.by_name(fc.ONEHOT_HIT_CASES, "onehot_hit-37x10")), OnehotOp(fc.by_name(fc.ONEHOT_CASES, "onehot-37x10"))
    norm, st = NormOp(fc.by_name(fc.NORM_CASES, "norm-n9-s0d0")), StageOp(fc.by_name(fc.STAGE_CASES, "stage-n9-s0d0"))
    o, ht, c = hit.ins[0].p, hit.ins[1].p, hit.outs[0].p
    l0 = lcount(t4k)
    for args in ((None, ht, 37, 31, c), (o, None, 37, 31, c), (o, ht, 37, 31, None), (o, ht, -1, 31, c), (o, ht, 37, 0, c), (o, ht, 37, -3, c)):
        assert lib.t4k_hit(*args, None) == ERR_ARG, args
    lb, out, hw, c = oh.ins[0].p, oh.ins[1].p, oh.outs[0].p, oh.outs[1].p
    for args in ((None, hw, out, 37, 10, c), (lb, None, out, 37, 10, c), (lb, hw, None, 37, 10, c), (lb, hw, out, 37, 10, None), (lb, hw, out, -1, 10, c), (lb, hw, out, 37, 0, c)):
        assert lib.t4k_onehot_hit(*args, None) == ERR_ARG, args
    lb, hw = one.ins[0].p, one.outs[0].p
    assert lib.t4k_onehot(None, hw, 37, 10, None) == ERR_ARG and lib.t4k_onehot(lb, None, 37, 10, None) == ERR_ARG
    assert b"t4k_onehot" in lib.t4k_last_error()
    assert lib.t4k_onehot(lb, hw, -1, 10, None) == OK and lib.t4k_onehot(lb, hw, 37, 0, None) == OK and lib.t4k_onehot(lb, hw, 37, -1, None) == OK
    src, dst = norm.ins[0].p, norm.outs[0].p
    assert lib.t4k_u8_normalize(None, dst, 9, 1.0, 1.0, None) == ERR_ARG and lib.t4k_u8_normalize(src, None, 9, 1.0, 1.0, None) == ERR_ARG
    assert b"t4k_u8_normalize" in lib.t4k_last_error()
    assert lib.t4k_u8_normalize(src, dst, -1, 1.0, 1.0, None) == OK
    src, dst, ls, ld = st.ins[0].p, st.outs[0].p, st.ins[1].p, st.outs[1].p
    for args in ((None, dst, 9, ls, ld, 9), (src, None, 9, ls, ld, 9), (src, dst, 9, None, ld, 9), (src, dst, 9, ls, None, 9), (src, dst, 0, None, ld, 9),
                 (src, dst, -1, ls, ld, 9), (src, dst, 9, ls, ld, -1)):
        assert lib.t4k_stage_batch(args[0], args[1], args[2], 1.0, 1.0, args[3], args[4], args[5], None) == ERR_ARG, args
    assert lib.t4k_stage_batch(src, dst, -1, 1.0, 1.0, ls, ld, 0, None) == OK and lib.t4k_stage_batch(src, dst, 0, 1.0, 1.0, None, None, 0, None) == OK
    assert lcount(t4k) == l0
    for op in (hit, oh, one, norm, st):
        assert op.still_prefilled(t4k) and op.inputs_intact(t4k), op.name
    for op in (hit, oh, one, norm, st):                                           # the calls the refusals stand beside
        op.run(t4k)


def test_zz_case_counts_and_wall_time():
    """what tests/README.md quotes"""
    print("\nfeed / label sweep: %s cases, %.1f s" % (", ".join("%d %s" % (v, k) for k, v in fc.counts().items()), time.time() - CLOCK["t0"]))
