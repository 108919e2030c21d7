"""Up-sampling by a run-time factor (t4k_upsample_fwd / _bwd): time per call of forward and backward for nearest, bilinear and bicubic at
four layers, the bytes each call moves by the rule and the achieved GB/s, and - at the two layers the old word forms admit - the route `2 upsample` /
`3 upsample` keep, on the same tensors in the same run.

    python tools/upsample_probe.py [--reps R] [--runs K] [--json profiles/upsample_probe.json]

Each timing is the wall time of R back-to-back calls on the library's default stream, bracketed by t4k_sync, divided by R; it is repeated K times, the
sides of a row alternating within every repeat, and the MEDIAN and the spread (min .. max) of the K figures are reported.

  rows: 16x16x64 -> x2, 32x32x64 -> x2, 8x8x128 -> x4, 32x32x3 -> x2, all at N = 256, three methods each; 32x32x64 -> x3, nearest, for the bar
  bytes by the rule: forward I + O, backward dY + dX; GB/s against SURVEY's 8 TB/s
  the bar, nearest at 32x32x64 x2 and x3 against the old route - forward t4k_dpool(T4K_L_USAMPLE), backward t4k_pool(T4K_L_AVGPOOL) followed by the scale
  map t4k_math(T4K_SCALE, K K), both launches timed together: the new entry takes no longer - "no longer" beyond the two spreads: new min <= old max."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = ctypes.c_void_p
AVG, USAMPLE, SCALE = 13, 17, 14                                          # T4K_L_AVGPOOL, T4K_L_USAMPLE, T4K_SCALE of include/t4k.h
METHODS = [("nearest", 0), ("bilinear", 2), ("bicubic", 3)]
PEAK_GBS = 8000.0

# name, N, H1, W1, C, K, the methods, beside the old route
CASES = [("16x16x64 x2", 256, 16, 16, 64, 2, METHODS, False),
         ("32x32x64 x2", 256, 32, 32, 64, 2, METHODS, True),
         ("8x8x128 x4", 256, 8, 8, 128, 4, METHODS, False),
         ("32x32x3 x2", 256, 32, 32, 3, 2, METHODS, False),
         ("32x32x64 x3", 256, 32, 32, 64, 3, METHODS[:1], True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--json")
    args = ap.parse_args()
    import torch
    from tensorforth_amd.lib import load
    h = load(); h.init(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g) - 0.5

    def timed(fn):
        h.call("t4k_sync", None)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        h.call("t4k_sync", None)
        return (time.perf_counter() - t0) / args.reps * 1e6

    def measure(row, sides):
        """sides: [(name, fn)]; alternating within every repeat"""
        times = {k: [] for k, _ in sides}
        for k, fn in sides:
            fn(); h.call("t4k_sync", None)                              # warm: code objects loaded
        for _ in range(args.runs):
            for k, fn in sides:
                times[k].append(timed(fn))
        for k, _ in sides:
            row[k + "_us"] = round(statistics.median(times[k]), 2)
            row[k + "_min_max_us"] = [round(min(times[k]), 2), round(max(times[k]), 2)]

    rows = []
    for name, N, H1, W1, C, K, methods, beside in CASES:
        H0, W0 = K * H1, K * W1
        I, O, G, DX = rnd(N, H1, W1, C), torch.zeros(N, H0, W0, C, device="cuda"), rnd(N, H0, W0, C), torch.zeros(N, H1, W1, C, device="cuda")
        p = {k: V(t.data_ptr()) for k, t in dict(I=I, O=O, G=G, DX=DX).items()}
        geo = (N, H1, W1, C, H0, W0, K)
        nbytes = 4 * I.numel() + 4 * O.numel()                           # I + O forward, dY + dX backward: the same count
        row = {"case": name, "N": N, "out": [H0, W0], "bytes": nbytes}
        sides = []
        for mn, m in methods:
            sides.append(("%s_fwd" % mn, lambda m=m: h.call("t4k_upsample_fwd", m, p["I"], p["O"], *geo, None)))
            sides.append(("%s_bwd" % mn, lambda m=m: h.call("t4k_upsample_bwd", m, p["G"], p["DX"], *geo, None)))

        def old_bwd():
            h.call("t4k_pool", AVG, p["G"], p["DX"], N, H0, W0, H1, W1, C, K, None)
            h.call("t4k_math", SCALE, p["DX"], float(K * K), DX.numel(), None)

        if beside:
            sides.insert(1, ("old_fwd", lambda: h.call("t4k_dpool", USAMPLE, p["O"], p["I"], N, H0, W0, H1, W1, C, K, None)))
            sides.insert(3, ("old_bwd", old_bwd))
        measure(row, sides)
        for mn, _ in methods:
            for d in ("fwd", "bwd"):
                k = "%s_%s" % (mn, d)
                row[k + "_gbs"] = round(nbytes / row[k + "_us"] / 1e3, 1)
                row[k + "_of_peak"] = round(nbytes / row[k + "_us"] / 1e3 / PEAK_GBS, 3)
        if beside:
            for d in ("fwd", "bwd"):
                row["ratio_" + d] = round(row["nearest_%s_us" % d] / row["old_%s_us" % d], 3)
                row["met_" + d] = row["nearest_%s_min_max_us" % d][0] <= row["old_%s_min_max_us" % d][1]
        print(json.dumps(row), flush=True); rows.append(row)
        del I, O, G, DX
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
