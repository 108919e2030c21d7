"""Broadcast arithmetic and batched transpose: t4k_tt_op_bcast / t4k_transpose_batched (one launch) against what they replace, on the same device.

    python tools/bcast_probe.py [--reps R] [--runs K] [--json out.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R (so it includes the
dispatches a loop pays for); it is repeated K times, the paths alternating within every repeat, and the MEDIAN and the spread (min .. max) of
the K figures are reported, with the dispatches of one call from t4k_launch_count.

  n_bcast    128x64x64x1 + 64x64 matrix: one launch against the 128 t4k_tt_op launches Tensor::ten_op made
  row_bcast  64x512x512x1 * (1,512,1,1), entry_bcast 64x512x512x1 * (64,1,1,1): against ONE t4k_tt_op over the same number of output elements
             (two full-size operands: the code this library had before, which reads strictly more bytes)
  transpose  128 x 64x64 and 8 x 1024x1024 against the per-entry t4k_transpose loop"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MUL, ADD = 18, 16
V = ctypes.c_void_p
I4, L4 = ctypes.c_int * 4, ctypes.c_long * 4


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

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        h.call("t4k_sync", None)
        return (time.perf_counter() - t0) / args.reps * 1e6

    def compare(case, new, old, new_name, old_name, bytes_new, bytes_old, same):
        counts = []
        for fn in (new, old):
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); fn(); counts.append(int(h.lib.t4k_launch_count()) - l0)
        h.call("t4k_sync", None)
        tn, to = [], []
        for _ in range(args.runs):
            tn.append(timed(new)); to.append(timed(old))
        row = {"case": case, new_name + "_us": round(statistics.median(tn), 2), new_name + "_min_max_us": [round(min(tn), 2), round(max(tn), 2)],
               old_name + "_us": round(statistics.median(to), 2), old_name + "_min_max_us": [round(min(to), 2), round(max(to), 2)],
               "launches_" + new_name: counts[0], "launches_" + old_name: counts[1],
               "speedup": round(statistics.median(to) / statistics.median(tn), 2),
               new_name + "_GBps": round(bytes_new / statistics.median(tn) / 1e3, 1), old_name + "_GBps": round(bytes_old / statistics.median(to) / 1e3, 1),
               "results_equal": bool(same())}
        print(json.dumps(row), flush=True)
        return row

    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)

    def rnd(n):
        return torch.rand(n, device="cuda", generator=g) + 0.5

    # ---- N broadcast: the loop Tensor::ten_op made
    N, HW = 128, 64 * 64
    A, B, O1, O2 = rnd(N * HW), rnd(HW), torch.zeros(N * HW, device="cuda"), torch.zeros(N * HW, device="cuda")
    pa, pb, p1, p2 = (t.data_ptr() for t in (A, B, O1, O2))
    dim, sa, sb = I4(N, 64, 64, 1), L4(HW, 64, 1, 0), L4(0, 64, 1, 0)

    def n_new():
        h.call("t4k_tt_op_bcast", ADD, V(pa), V(pb), V(p1), dim, sa, sb, None)

    def n_old():
        for n in range(N):
            h.call("t4k_tt_op", ADD, V(pa + 4 * n * HW), V(pb), V(p2 + 4 * n * HW), HW, None)

    rows.append(compare("128x64x64x1 + 64x64 matrix", n_new, n_old, "bcast", "loop", 4 * (2 * N * HW + HW), 4 * 3 * N * HW, lambda: torch.equal(O1, O2)))

    # ---- per-row and per-entry operands against t4k_tt_op at the same output size
    N, H, W = 64, 512, 512
    n = N * H * W
    A, Bf, O1, O2 = rnd(n), rnd(n), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pa, pf, p1, p2 = (t.data_ptr() for t in (A, Bf, O1, O2))
    dim, sa = I4(N, H, W, 1), L4(H * W, W, 1, 0)
    for name, shape, sb in (("(1,512,1,1)", (1, H, 1), L4(0, 1, 0, 0)), ("(64,1,1,1)", (N, 1, 1), L4(1, 0, 0, 0))):
        Bs = rnd(shape[0] * shape[1])
        Bf.copy_(Bs.reshape(shape).expand(N, H, W).reshape(-1)); torch.cuda.synchronize()
        ps = Bs.data_ptr()

        def b_new():
            h.call("t4k_tt_op_bcast", MUL, V(pa), V(ps), V(p1), dim, sa, sb, None)

        def b_old():
            h.call("t4k_tt_op", MUL, V(pa), V(pf), V(p2), n, None)

        rows.append(compare("64x512x512x1 * " + name, b_new, b_old, "bcast", "tt_op", 4 * (2 * n + Bs.numel()), 4 * 3 * n, lambda: torch.equal(O1, O2)))
    del A, Bf, O1, O2

    # ---- transposes
    for batch, K in ((128, 64), (8, 1024)):
        S, D1, D2 = rnd(batch * K * K), torch.zeros(batch * K * K, device="cuda"), torch.zeros(batch * K * K, device="cuda")
        ps, p1, p2 = (t.data_ptr() for t in (S, D1, D2))

        def t_new():
            h.call("t4k_transpose_batched", V(ps), V(p1), K, K, 1, batch, None)

        def t_old():
            for b in range(batch):
                h.call("t4k_transpose", V(ps + 4 * b * K * K), V(p2 + 4 * b * K * K), K, K, 1, None)

        rows.append(compare("%d x %dx%d transpose" % (batch, K, K), t_new, t_old, "batched", "loop", 8 * batch * K * K, 8 * batch * K * K,
                            lambda: torch.equal(D1, D2)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
