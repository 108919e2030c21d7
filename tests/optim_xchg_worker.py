"""The exchanging optimizer launch k_opt_step<true> (csrc/optim.hip) as ONE process reaches it: a one-rank exchange in self mode (t4k_xchg_self, what
bench.py --full times as dp_overhead_us).  tests/test_gpu_optim_sweep.py::test_exchanging_launch_in_self_mode starts this program once - the exchange is
process-wide state, which must not reach the rest of a test session - and asserts on the ONE JSON line it prints.
usage: optim_xchg_worker.py

For the four kinds, t4k_opt_step_dp against t4k_opt_step on the same operands, bit for bit:
  plain              a table whose every DG lies inside the slab (the table's own buffer): the exchanging launch, 1 launch
  fold               the same with a conv stack's partial fold pending (its dF | dB tensors inside the slab): backward + update, 2 launches
  dg-outside-slab    a slab that begins behind record 0's DG: the fall-back - the slab summed in ceil(slab_n / 65536) launches, then the plain step
  slab-above-window  slab_n above the window the exchange was created with: the same fall-back
  capture            t4k_opt_step_dp while a graph is recorded: T4K_ERR_UNSUPPORTED, no launch, nothing written
Not a test module."""
import ctypes
import json
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T4K_ERR_UNSUPPORTED = -4
WINDOW = 1 << 17                                                            # floats; bench.py's
SMALL_WINDOW = 4096


def main():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import t4oracle as oracle
    import optim_cases as oc
    import test_gpu_optim_sweep as sw
    from tensorforth_amd import lib as t4lib
    oracle.lib()
    k = t4lib.load(); k.init(0)
    lib = k.lib; lib.t4k_launch_count.restype = ctypes.c_ulonglong
    dev = sw.Dev(k)
    out = dict(ok=False, passed=[], failed=[], fallback_launches={}, exchanging_launches={})

    def connect(window):
        h = (ctypes.c_ubyte * 64)()
        k.call("t4k_xchg_create", window, 0, 1, h); k.call("t4k_xchg_connect", bytes(h)); k.call("t4k_xchg_self", 1)

    def dp(a, kname, slab, slab_n, s=None, nt=None, tab=None, host=None, chunks=None):
        kind, hp = sw.opt_args(kname)
        return lib.t4k_opt_step_dp(kind, sw.p(a.tab) if tab is None else tab, a.host if host is None else host, len(a.plan.sizes) if nt is None else nt,
                                   a.chunks if chunks is None else chunks, *hp, slab, slab_n, s)

    def twin(kname, seed):
        """the reference: the same table through t4k_opt_step (slab = NULL: never exchanging), held to float64 and the oracle"""
        a = sw.make(dev, kname, "aligned", np.random.default_rng(seed))
        l0 = sw.launches(k)
        assert sw.step(k, a, kname) == 0 and sw.launches(k) - l0 == 1
        new = a.download(); sw.check_step("t4k_opt_step " + kname, oracle, kname, a, new, report="optimizer sweep (exchange)")
        return new

    def plain(kname):
        want = twin(kname, 1600)
        a = sw.make(dev, kname, "aligned", np.random.default_rng(1600))
        assert a.plan.total <= WINDOW
        l0 = sw.launches(k)
        assert dp(a, kname, a.base, a.plan.total) == 0
        out["exchanging_launches"]["plain " + kname] = sw.launches(k) - l0
        oc.same_bits("plain " + kname, a.download(), want)

    def fallback(form, kname):
        want = twin(kname, 1601)
        a = sw.make(dev, kname, "aligned", np.random.default_rng(1601))
        off = a.plan.rec[1]["G"][0] - oc.MOAT if form == "dg-outside-slab" else 0       # record 0's DG lies in front of such a slab
        n = a.plan.total - off
        assert a.plan.rec[0]["DG"][0] < off if form == "dg-outside-slab" else n > SMALL_WINDOW
        l0 = sw.launches(k)
        assert dp(a, kname, a.base + 4 * off, n) == 0
        out["fallback_launches"]["%s %s" % (form, kname)] = (sw.launches(k) - l0, -(-n // 65536))
        got = a.download(); m = a.plan.moat
        oc.same_bits("%s %s" % (form, kname), got[~m], want[~m]); oc.same_values("%s %s moats" % (form, kname), got[m], want[m])   # (the summed slab holds the moats too: 0 + NaN)

    def capture(kname):
        a = sw.make(dev, kname, "aligned", np.random.default_rng(1602))
        s = ctypes.c_void_p(); g = ctypes.c_void_p()
        k.call("t4k_stream_create", ctypes.byref(s))
        dev.torch.cuda.synchronize()
        k.call("t4k_graph_begin", s)
        l0 = sw.launches(k)
        rc = dp(a, kname, a.base, a.plan.total, s)
        n = sw.launches(k) - l0
        lib.t4k_graph_end(s, ctypes.byref(g))
        if g.value:
            lib.t4k_graph_destroy(g)
        k.call("t4k_sync", s); k.call("t4k_stream_destroy", s)
        assert rc == T4K_ERR_UNSUPPORTED and n == 0, (rc, n)
        oc.same_bits("capture %s: nothing written" % kname, a.download(), a.cur)

    stack = {}

    def fold(kname):
        """conv-stack case 3 with its dF | dB tensors inside the slab; backward(train | 4) + t4k_opt_step against backward(train | 4) + t4k_opt_step_dp"""
        import struct
        if not stack:
            N, X, stages, flat, params, arr, bufs, dDY, _ = sw._setup(k, dev, oracle, 3, 503)
            F, B = params[0]
            sizes = (3000, F.size, 5, B.size, 1025)
            a = sw.Arena(dev, oc.Plan(sizes, "aligned", "adam")); a.fill(np.random.default_rng(1603))
            a.put(a.plan.rec[1]["DG"][0], np.full(F.size, 0.25, np.float32)); a.put(a.plan.rec[3]["DG"][0], np.full(B.size, -0.5, np.float32))
            arr[0].DF, arr[0].DB = a.ptr(1, "DG"), a.ptr(3, "DG")
            pad, chunks = oc.pads(sizes); raw = b""
            for i, n in enumerate(sizes):
                G, DG, M, V = a.plan.pointers(a.base, i)
                G = sw.p(bufs[0]["F"]) if i == 1 else sw.p(bufs[0]["B"]) if i == 3 else G
                raw += struct.pack("<QQQQqii", G, DG, M, V, n, (1, F.shape[0], 3, B.size, 2)[i], pad[i])
            stack.update(N=N, X=X, params=params, arr=arr, bufs=bufs, dDY=dDY, a=a, init=a.cur.copy(), chunks=chunks, nt=len(sizes),
                         tab=dev.up(np.frombuffer(raw, np.uint8)), host=(sw.ParamRec * len(sizes)).from_buffer_copy(raw))
        st = stack; a, bufs = st["a"], st["bufs"]; T = dev.torch
        kind, hp = sw.opt_args(kname)
        res = []
        for exchanging in (False, True):
            a.put(0, st["init"])
            bufs[0]["F"].copy_(T.from_numpy(st["params"][0][0])); bufs[0]["B"].copy_(T.from_numpy(st["params"][0][1]))
            k.call("t4k_rand_init", 58); k.call("t4k_rand_set_offset", 4096)
            bufs[0]["X"].copy_(T.from_numpy(st["X"]))
            k.call("t4k_conv_stack_fwd", sw.p(bufs[0]["X"]), None, st["arr"], 1, st["N"], None)
            k.call("t4k_sync", None)
            l0 = sw.launches(k)
            k.call("t4k_conv_stack_bwd", sw.p(st["dDY"]), st["arr"], 1, st["N"], 5, None)
            if exchanging:
                assert dp(a, kname, a.base, a.plan.total, None, st["nt"], sw.p(st["tab"]), st["host"], st["chunks"]) == 0
            else:
                assert lib.t4k_opt_step(kind, sw.p(st["tab"]), st["host"], st["nt"], st["chunks"], *hp, None) == 0
            n = sw.launches(k) - l0
            assert n == 2, n
            if exchanging:
                out["exchanging_launches"]["fold " + kname] = n
            res.append((a.download(), dev.down(bufs[0]["F"]).copy(), dev.down(bufs[0]["B"]).copy()))
        for t, x, y in zip(("arena", "F", "B"), res[1], res[0]):
            oc.same_bits("fold %s %s" % (kname, t), x, y)
        assert not np.array_equal(res[0][1], st["params"][0][0]) and not oc.bits(a.plan.view(res[1][0], 1, "DG")).any()   # ... the filter moved, its gradient is zeroed

    def run(name, fn, *args):
        if out["failed"]:                                                   # after a failure nothing more is started on the device
            return
        try:
            fn(*args); out["passed"].append(name)
        except Exception:
            out["failed"].append([name, traceback.format_exc()[-1500:]])

    connect(WINDOW)
    out["active_in_self_mode"] = int(lib.t4k_xchg_active())
    for kname in oc.KINDS:
        run("plain " + kname, plain, kname)
        run("fold " + kname, fold, kname)
        run("dg-outside-slab " + kname, fallback, "dg-outside-slab", kname)
        run("capture " + kname, capture, kname)
    k.call("t4k_sync", None)
    connect(SMALL_WINDOW)                                                   # (t4k_xchg_create lets go of the first window)
    for kname in oc.KINDS:
        run("slab-above-window " + kname, fallback, "slab-above-window", kname)
    rc = lib.t4k_sync(None)
    if rc != 0:
        out["failed"].append(["t4k_sync", lib.t4k_last_error().decode(errors="replace")[-500:]])
    k.call("t4k_xchg_self", 0)
    out["active_after"] = int(lib.t4k_xchg_active())
    k.call("t4k_xchg_destroy")
    out["world_after"] = int(lib.t4k_xchg_world())
    out["ok"] = not out["failed"]
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
