"""Axis reductions: t4k_reduce_axes against the code it stands beside or replaces, on the same device in the same run.

    python tools/reduce_axes_probe.py [--reps R] [--runs K] [--json out.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R (so it includes the
dispatches a loop pays for); it is repeated K times, the paths alternating within every repeat, and the MEDIAN and the spread (min .. max) of
the K figures are reported, with the dispatches of one call from t4k_launch_count.  GB/s = the source bytes over the median.

  (a) all      mask 15 on 16 M floats against t4k_reduce on the same buffer
  (b) columns  mask 4 on [4096,4096] against t4k_dlinear_db(..., 4096, 4096) (which accumulates into its destination)
  (c) rows     mask 2 on [4096,4096] against 4096 t4k_reduce calls, one per row
      channels mask 14 on (256,32,32,64) against t4k_transpose to [64, 262144] and 64 t4k_reduce calls, one per channel"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUM = 0
V = ctypes.c_void_p
I4 = ctypes.c_int * 4


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

    def compare(case, new, old, old_name, nbytes, close, old_reps=None):
        counts = []
        for fn in (new, old):
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); fn(); counts.append(int(h.lib.t4k_launch_count()) - l0)
        h.call("t4k_sync", None)
        ok = bool(close())
        tn, to = [], []
        for _ in range(args.runs):
            tn.append(timed(new, args.reps)); to.append(timed(old, old_reps or args.reps))
        mn, mo = statistics.median(tn), statistics.median(to)
        row = {"case": case, "axes_us": round(mn, 2), "axes_min_max_us": [round(min(tn), 2), round(max(tn), 2)],
               old_name + "_us": round(mo, 2), old_name + "_min_max_us": [round(min(to), 2), round(max(to), 2)],
               "launches_axes": counts[0], "launches_" + old_name: counts[1], "speedup": round(mo / mn, 2),
               "axes_GBps": round(nbytes / mn / 1e3, 1), old_name + "_GBps": round(nbytes / mo / 1e3, 1), "results_close": ok}
        print(json.dumps(row), flush=True)
        return row

    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)

    def rnd(n):
        return torch.rand(n, device="cuda", generator=g) - 0.5

    # ---- (a) everything into one scalar
    n = 16 << 20
    X, o1, o2 = rnd(n), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    px, p1, p2 = X.data_ptr(), o1.data_ptr(), o2.data_ptr()
    rows.append(compare("mask 15 on 16 M floats", lambda: h.call("t4k_reduce_axes", SUM, V(px), V(p1), I4(1, 1, 1, n), 15, None, None),
                        lambda: h.call("t4k_reduce", SUM, V(px), n, 0.0, V(p2), None), "reduce", 4 * n,
                        lambda: abs(float(o1[0]) - float(o2[0])) <= 1e-3 * float(X.abs().sum()) * 2.0 ** -10))
    del X

    # ---- (b) column sums, (c) row sums of a square matrix
    K = 4096
    X, o1, o2 = rnd(K * K), torch.zeros(K, device="cuda"), torch.zeros(K, device="cuda")
    px, p1, p2 = X.data_ptr(), o1.data_ptr(), o2.data_ptr()

    def db():
        h.call("t4k_dlinear_db", V(px), V(p2), K, K, None)

    def close_cols():
        o2.zero_(); torch.cuda.synchronize(); db(); h.call("t4k_sync", None)
        return torch.allclose(o1, o2, rtol=0, atol=1e-3)

    rows.append(compare("mask 4 on [4096,4096] (column sums)", lambda: h.call("t4k_reduce_axes", SUM, V(px), V(p1), I4(1, K, K, 1), 4, None, None),
                        db, "dlinear_db", 4 * K * K, close_cols))

    def row_loop():
        for r in range(K):
            h.call("t4k_reduce", SUM, V(px + 4 * r * K), K, 0.0, V(p2 + 4 * r), None)

    rows.append(compare("mask 2 on [4096,4096] (row sums)", lambda: h.call("t4k_reduce_axes", SUM, V(px), V(p1), I4(1, K, K, 1), 2, None, None),
                        row_loop, "loop", 4 * K * K, lambda: torch.allclose(o1, o2, rtol=0, atol=1e-3)))
    del X

    # ---- (c) per-channel sums of a conv activation
    N, H, W, C = 256, 32, 32, 64
    R = N * H * W
    X, Xt, o1, o2 = rnd(R * C), torch.zeros(R * C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    px, pt, p1, p2 = X.data_ptr(), Xt.data_ptr(), o1.data_ptr(), o2.data_ptr()

    def chan_loop():
        h.call("t4k_transpose", V(px), V(pt), R, C, 1, None)
        for c in range(C):
            h.call("t4k_reduce", SUM, V(pt + 4 * c * R), R, 0.0, V(p2 + 4 * c), None)

    rows.append(compare("mask 14 on (256,32,32,64) (per-channel sums)", lambda: h.call("t4k_reduce_axes", SUM, V(px), V(p1), I4(N, H, W, C), 14, None, None),
                        chan_loop, "loop", 4 * R * C, lambda: torch.allclose(o1, o2, rtol=0, atol=1e-2)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
