"""The patch embedding (t4k_patch_fwd / _bwd): time per call at five shapes beside two yardsticks, neither of them the code under test.
Yardstick 1 is the cheapest route the library could otherwise offer: t4k_gemm (and its transposed forms for dF and dX) on operands ALREADY gathered to
[M, K K C1], plus one t4k_copy of the image's bytes standing in for the gather it is spared (two in the backward: the gather and the scatter of dX).
Yardstick 2, a ratio only, is torch's conv2d(stride=K) and its autograd on the same device.

    python tools/patch_probe.py [--reps R] [--runs K] [--json profiles/patch_probe.json] [--lib PATH]

The protocol of tools/attention_probe.py: each timing is the wall time of R back-to-back calls ending in a device synchronisation, divided by R; it is
repeated K times after a warm-up of every side, the sides of a row alternating within every repeat; the MEDIAN and the spread (min .. max) are reported,
with the launches of one call from t4k_launch_count.

  rows: 1 ViT-B/16 N 128, 224 x 224 x 3 -> 768;  2 ViT-Ti/16 -> 192;  3 /14 -> 768 (the dword gather);  4 /32 -> 768;  5 tiny N 8, 32 x 32, K 8 -> 64
  bars: the unit's slowest repeat no slower than yardstick 1's fastest, forward and backward ("met" | "MISSED"; the tiny row is launch-bound: "reported")
  mfma_fraction: 2 M K K C1 C0 flops a product (one forward, two backward) over the median time, as a fraction of the fp32 MFMA peak (157.3 TFLOP/s)."""
import argparse
import ctypes
import datetime
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VP = ctypes.c_void_p
PEAK = 157.3e12
CASES = [("1 ViT-B/16", 128, 224, 3, 768, 16), ("2 ViT-Ti/16", 128, 224, 3, 192, 16), ("3 ViT-B/14", 128, 224, 3, 768, 14), ("4 ViT-B/32", 128, 224, 3, 768, 32),
         ("5 tiny", 8, 32, 1, 64, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--rows", default="12345")
    ap.add_argument("--json")
    ap.add_argument("--lib")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(args.lib); h.init(0)
    h.lib.t4k_launch_count.restype = ctypes.c_ulonglong
    g = torch.Generator(device="cuda").manual_seed(1)
    p = lambda t: VP(t.data_ptr())

    def timed(f):
        h.call("t4k_sync", None); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            f()
        h.call("t4k_sync", None); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps * 1e6

    def measure(row, sides):
        times = {k: [] for k, _ in sides}
        for k, f in sides:
            f(); h.call("t4k_sync", None); torch.cuda.synchronize()    # warm: code objects loaded
            l0 = int(h.lib.t4k_launch_count()); f(); row["launches_" + k] = int(h.lib.t4k_launch_count()) - l0
        for _ in range(args.runs):
            for k, f in sides:
                times[k].append(timed(f))
        for k, _ in sides:
            row[k + "_us"] = round(statistics.median(times[k]), 2)
            row[k + "_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]

    def one(name, N, HW, C1, C0, K):
        H0 = HW // K; M, Kd = N * H0 * H0, K * K * C1
        row = {"case": name, "N": N, "H1": HW, "W1": HW, "C1": C1, "C0": C0, "K": K, "M": M, "Kd": Kd}
        out = (ctypes.c_int * 8)(); h.call("t4k_patch_plan", N, HW, HW, C1, C0, K, 7, out); row["plan"] = list(out)
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
        I, F, B, DO = rnd(N, HW, HW, C1), rnd(C1, K, K, C0) / K, rnd(C0), rnd(N, H0, H0, C0)
        O, DX, IC = torch.zeros_like(DO), torch.zeros_like(I), torch.zeros_like(I)
        G = torch.zeros(Kd * C0 + C0, device="cuda"); DF, DB = G[:Kd * C0], G[Kd * C0:]
        A, GO, GF, GA = rnd(M, Kd), torch.zeros(M, C0, device="cuda"), torch.zeros(Kd, C0, device="cuda"), torch.zeros(M, Kd, device="cuda")
        Fm = F.reshape(Kd, C0)
        n_img = N * HW * HW * C1
        tx = I.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        tw = F.permute(3, 0, 1, 2).contiguous().requires_grad_(True)
        conv = lambda: torch.nn.functional.conv2d(tx, tw, B, stride=K)
        ty, tdy = conv(), DO.permute(0, 3, 1, 2).contiguous()

        def gemm_fwd():
            h.call("t4k_copy", p(I), p(IC), n_img, None)
            h.call("t4k_gemm", p(A), p(Fm), p(GO), 1.0, 0.0, 0, 0, M, C0, Kd, 1, None)

        def gemm_bwd():
            h.call("t4k_copy", p(I), p(IC), n_img, None)
            h.call("t4k_gemm", p(A), p(DO), p(GF), 1.0, 1.0, 1, 0, Kd, C0, M, 1, None)       # dF += A^T dO
            h.call("t4k_gemm", p(DO), p(Fm), p(GA), 1.0, 0.0, 0, 1, M, Kd, C0, 1, None)      # dA = dO F^T
            h.call("t4k_copy", p(IC), p(DX), n_img, None)

        sides = [("patch_fwd", lambda: h.call("t4k_patch_fwd", p(I), None, p(O), p(F), p(B), N, HW, HW, C1, C0, K, None)),
                 ("gemm_fwd", gemm_fwd),
                 ("patch_bwd", lambda: h.call("t4k_patch_bwd", p(I), p(DO), p(DX), None, p(F), p(DF), p(DB), N, HW, HW, C1, C0, K, 1, None)),
                 ("gemm_bwd", gemm_bwd),
                 ("torch_fwd", conv),
                 ("torch_bwd", lambda: torch.autograd.grad(ty, (tx, tw), tdy, retain_graph=True))]
        measure(row, sides)
        flops = 2.0 * M * Kd * C0
        for k, n in (("fwd", 1), ("bwd", 2)):
            met = row["patch_" + k + "_min_max_us"][1] <= row["gemm_" + k + "_min_max_us"][0]
            row["bar_" + k] = "reported" if M * Kd < (1 << 20) else ("met" if met else "MISSED")
            row["ratio_" + k] = round(row["patch_" + k + "_us"] / row["gemm_" + k + "_us"], 3)
            row["ratio_torch_" + k] = round(row["patch_" + k + "_us"] / row["torch_" + k + "_us"], 3)
            row["mfma_fraction_" + k] = round(n * flops / (row["patch_" + k + "_us"] * 1e-6) / PEAK, 4)
        print(json.dumps(row), flush=True)
        return row

    rows = [one(*c) for c in CASES if c[0][0] in args.rows]
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "devices": 1, "date": datetime.date.today().isoformat(), "reps": args.reps, "runs": args.runs,
                       "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
