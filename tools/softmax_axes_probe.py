"""Axis softmax: t4k_softmax_axes against the code it stands beside or replaces, on the same device in the same run.

    python tools/softmax_axes_probe.py [--reps R] [--runs K] [--json out.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R (so it includes the
dispatches a sequence pays for); it is repeated K times, the paths alternating within every repeat, and the MEDIAN and the spread (min .. max)
of the K figures are reported, with the dispatches of one call from t4k_launch_count.  GB/s = 8 bytes per element (one read, one write)
over the median, whatever the regime really moves.

  (a) rows      mask 1 on [4096,10], [4096,1024] and [16,65536] beside t4k_softmax on the same buffers
  (b) attention mask 2 on (256,128,128,1) beside the sequence the words could compose before: copy, exp, the row sums (t4k_reduce_axes), the
                broadcast division (t4k_tt_op_bcast) - unstable, and four launches
  (c) channels  mask 14 on (256,32,32,64): the column family, no rival"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUM, EXP, DIV = 0, 2, 19                                                # include/t4k.h: T4K_RED_SUM, T4K_EXP, T4K_DIV
V = ctypes.c_void_p
I4 = ctypes.c_int * 4
L4 = ctypes.c_long * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong

    def timed(fn, reps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        h.call("t4k_sync", None)
        return (time.perf_counter() - t0) / reps * 1e6

    def compare(case, new, old, old_name, nelem, close):
        paths = [("axes", new)] + ([(old_name, old)] if old else [])
        counts, times = {}, {k: [] for k, _ in paths}
        for k, fn in paths:
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); fn(); counts[k] = int(h.lib.t4k_launch_count()) - l0
        h.call("t4k_sync", None)
        ok = bool(close()) if close else None
        for _ in range(args.runs):
            for k, fn in paths:
                times[k].append(timed(fn, args.reps))
        row = {"case": case, "results_close": ok}
        for k, _ in paths:
            med = statistics.median(times[k])
            row.update({k + "_us": round(med, 2), k + "_min_max_us": [round(min(times[k]), 2), round(max(times[k]), 2)],
                        "launches_" + k: counts[k], k + "_GBps": round(8 * nelem / med / 1e3, 1)})
        if old:
            row["speedup"] = round(row[old_name + "_us"] / row["axes_us"], 2)
        print(json.dumps(row), flush=True)
        return row

    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)

    def rnd(n):
        return (torch.rand(n, device="cuda", generator=g) - 0.5) * 8.0

    # ---- (a) rows of a matrix beside t4k_softmax
    for N, C in ((4096, 10), (4096, 1024), (16, 65536)):
        X, o1, o2 = rnd(N * C), torch.zeros(N * C, device="cuda"), torch.zeros(N * C, device="cuda")
        px, p1, p2 = X.data_ptr(), o1.data_ptr(), o2.data_ptr()
        rows.append(compare("mask 1 on [%d,%d]" % (N, C), lambda: h.call("t4k_softmax_axes", V(px), V(p1), I4(1, 1, N, C), 1, None),
                            lambda: h.call("t4k_softmax", V(px), V(p2), N, C, None), "softmax", N * C,
                            lambda: torch.allclose(o1, o2, rtol=1e-5, atol=1e-9)))
        del X, o1, o2

    # ---- (b) attention scores beside the composable sequence
    N, L = 256, 128
    n = N * L * L
    X, o1, o2, rs = rnd(n), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(N * L, device="cuda")
    px, p1, p2, pr = X.data_ptr(), o1.data_ptr(), o2.data_ptr(), rs.data_ptr()

    def composed():
        h.call("t4k_copy", V(px), V(p2), n, None)
        h.call("t4k_math", EXP, V(p2), 0.0, n, None)
        h.call("t4k_reduce_axes", SUM, V(p2), V(pr), I4(N, L, L, 1), 2, None, None)
        h.call("t4k_tt_op_bcast", DIV, V(p2), V(pr), V(p2), I4(N, L, L, 1), L4(L * L, L, 1, 0), L4(L, 1, 0, 0), None)

    rows.append(compare("mask 2 on (256,128,128,1)", lambda: h.call("t4k_softmax_axes", V(px), V(p1), I4(N, L, L, 1), 2, None),
                        composed, "composed", n, lambda: torch.allclose(o1, o2, rtol=1e-4, atol=1e-8)))
    del X, o1, o2, rs

    # ---- (c) per-channel planes of a conv activation: the column family
    N, H, W, C = 256, 32, 32, 64
    n = N * H * W * C
    X, o1 = rnd(n), torch.zeros(n, device="cuda")
    px, p1 = X.data_ptr(), o1.data_ptr()
    rows.append(compare("mask 14 on (256,32,32,64)", lambda: h.call("t4k_softmax_axes", V(px), V(p1), I4(N, H, W, C), 14, None), None, None, n,
                        lambda: torch.allclose(o1.view(-1, C).sum(0), torch.ones(C, device="cuda"), rtol=0, atol=1e-3)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
